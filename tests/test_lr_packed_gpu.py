"""Distinct-coefficient packing on the GPU: the packed reducer
(dx_lr_reduce_pack: block sum + upper-triangle gather + rounding in one
launch), the encoder's upper launch plan (dx_lr_encode, upper), and
Packing = 1 queries end to end.  A packed value must be the same bits as the
cartesian path's value at (i, j), i <= j.  Run with -m gpu."""
import pytest
import torch

import test_lr_highdim as hd
import test_lr_packed as pk
from drynx_amd import native as nt
from drynx_amd.models import logistic_regression as lr
from drynx_amd.query import LogisticRegressionParameters

pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _gather(tot: torch.Tensor, D: int) -> torch.Tensor:
    """[P, P] totals -> level 1 (row D), then level 2's (i, j), i <= j, row by row."""
    return torch.cat([tot[D, :D]] + [tot[i, i:D] for i in range(D)])


def test_reduce_pack_hand_built_slab(gpu_device):
    """The reducer alone on exact values (D = 3, P = 48, 5 blocks, 2 items):
    rounding half away from zero, -0.0, the largest double below 0.5,
    2^52 + 1, and sums whose value depends on the order of the blocks.
    Everything but the 9 live elements is NaN and must never be read."""
    D, P, nb = 3, 48, 5
    live = [(3, 0), (3, 1), (3, 2), (0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]  # packed order
    slab = torch.full((2, nb, P, P), float("nan"), dtype=torch.float64)
    for r, c in live:
        slab[:, :, r, c] = 0.0
    # item 0: one value per element in block 0, the other blocks add +0.0
    seeds = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, -0.0, 0.49999999999999994, 2.0 ** 52 + 1]
    for (r, c), v in zip(live, seeds):
        slab[0, 0, r, c] = v
    slab[0, :, 1, 1] = -0.0  # -0.0 in every block
    # item 1: values split across the blocks.  Block b goes to accumulator b % 4 (block 4 joins
    # block 0), combined as (s0 + s1) + (s2 + s3): another order gives another double.
    splits = [[1e16, 1.0, -1e16, 1.0, 1.0],  # here 0; left to right 2
              [0.25, 2.0 ** 53, 0.25, -(2.0 ** 53), 1.0],  # here 2; left to right 1
              [0.5, 0.0, 0.0, 0.0, 1.0],  # 1.5 only with block 4
              [-1.0, 0.25, -1.0, 0.25, -0.5],  # -2.0: no half
              [0.1, 0.2, 0.3, 0.4, 0.5],
              [2.0 ** 52, 0.5, 0.5, 0.5, 0.5],
              [-0.0, 0.0, -0.0, 0.0, -0.0],
              [1e-300, -1e-300, 3.5, 0.0, 0.0],
              [-2.5, 0.0, 0.0, 0.0, 0.0]]
    for (r, c), v in zip(live, splits):
        slab[1, :, r, c] = torch.tensor(v, dtype=torch.float64)
    slab = slab.to(gpu_device)
    tot = nt.lr_reduce(slab)
    exp_f = torch.stack([_gather(tot[i], D) for i in range(2)])
    assert not torch.isnan(exp_f).any()
    assert exp_f[1, :3].tolist() == [0.0, 2.0, 1.5]  # the order-dependent sums, in dx_lr_reduce's order
    for precision in (1.0, 100.0):
        exp = lr.round_precision(exp_f, precision)
        got, got_f = nt.lr_reduce_pack(slab, D, precision, floats=True)
        assert got.shape == (2, 9) and got.dtype == torch.int64
        assert not torch.isnan(got_f).any()  # nothing below the diagonal or in the padding was read
        assert torch.equal(got_f.view(torch.int64), exp_f.view(torch.int64))  # same bits, signed zeros included
        assert torch.equal(got, exp), (got.tolist(), exp.tolist())
        assert torch.equal(nt.lr_reduce_pack(slab[1], D, precision)[0], exp[1])  # [nb, P, P]: one item
    got = nt.lr_reduce_pack(slab, D, 1.0).tolist()
    assert got[0][:7] == [1, -1, 2, -2, 3, -3, 0]  # halves away from zero, -0.0 -> 0
    assert got[1][:4] == [0, 2, 2, -2] and got[1][6] == 0 and got[1][8] == -3
    with pytest.raises(ValueError):
        nt.lr_reduce_pack(slab, 48, 1.0)  # row D = 48 is outside a 48 x 48 block


def test_reducers_write_into_a_given_destination(gpu_device, monkeypatch):
    """``out=`` / ``fout=``: rows 1..2 of a larger result hold exactly what the
    reducers return for items 1..2, row 0 is untouched; a destination that is
    not contiguous or of another shape is refused before any launch."""
    D, T, L = 4, 2, 2 * 4 + 4 * 5 // 2
    slab = torch.randn(3, 5, 48, 48, dtype=torch.float64, generator=_gen(11)).to(gpu_device)
    exp, exp_f = nt.lr_reduce_pack(slab[1:3], D, 100.0, floats=True, T=T)
    assert exp.shape == (2, L)
    big = torch.full((3, L), -7, dtype=torch.int64, device=gpu_device)
    fbig = torch.full((3, L), -7.0, dtype=torch.float64, device=gpu_device)
    got, got_f = nt.lr_reduce_pack(slab[1:3], D, 100.0, floats=True, T=T, out=big[1:3], fout=fbig[1:3])
    assert got.data_ptr() == big[1:3].data_ptr() and got_f.data_ptr() == fbig[1:3].data_ptr()
    assert torch.equal(big[1:3], exp) and torch.equal(fbig[1:3].view(torch.int64), exp_f.view(torch.int64))
    assert (big[0] == -7).all() and (fbig[0] == -7.0).all()
    big.fill_(-7)
    assert nt.lr_reduce_pack(slab[1:3], D, 100.0, T=T, out=big[1:3]).data_ptr() == big[1:3].data_ptr()
    assert torch.equal(big[1:3], exp) and (big[0] == -7).all()
    tot = nt.lr_reduce(slab[1:3])
    tbig = torch.full((3, 48, 48), -7.0, dtype=torch.float64, device=gpu_device)
    assert nt.lr_reduce(slab[1:3], out=tbig[1:3]).data_ptr() == tbig[1:3].data_ptr()
    assert torch.equal(tbig[1:3].view(torch.int64), tot.view(torch.int64)) and (tbig[0] == -7.0).all()
    # refused before any launch
    calls = []
    raw = nt._raw_call
    monkeypatch.setattr(nt, "_raw_call", lambda name, *a: calls.append(name) or raw(name, *a))
    wide = torch.zeros((2, 2 * L), dtype=torch.int64, device=gpu_device)
    for bad in (wide[:, :L], big[:1], big[1:3].to(torch.int32)):
        with pytest.raises(ValueError):
            nt.lr_reduce_pack(slab[1:3], D, 100.0, T=T, out=bad)
    for bad in (wide.to(torch.float64)[:, :L], fbig[:1]):
        with pytest.raises(ValueError):
            nt.lr_reduce_pack(slab[1:3], D, 100.0, floats=True, T=T, fout=bad)
    twide = torch.zeros((2, 48, 96), dtype=torch.float64, device=gpu_device)
    for bad in (twide[:, :, :48], tbig[:1], tbig[1:3].reshape(2, 48 * 48)):
        with pytest.raises(ValueError):
            nt.lr_reduce(slab[1:3], out=bad)
    assert calls == []


def _data(gpu_device, N, d):
    X = (torch.rand(N, d, dtype=torch.float64, generator=_gen(N * 1000 + d)) * 4).to(gpu_device)
    y = torch.randint(0, 2, (N,), generator=_gen(d)).to(gpu_device)
    m = torch.full((d,), 2.0, dtype=torch.float64, device=gpu_device)
    s = torch.full((d,), 1.15, dtype=torch.float64, device=gpu_device)
    return X, y, m, s


# one tile | row D = 16 opens the second tile | headline | last one-block width | first wide width,
# row 48 opens a tile-block | wide, mid-tile | single record | row D = 128 opens a tile row
SHAPES = [(5, 3), (77, 15), (123, 44), (70, 46), (77, 47), (211, 100), (1, 100), (130, 127)]


@pytest.mark.parametrize("N,d", SHAPES)
def test_packed_equals_cartesian_upper_triangle(gpu_device, N, d):
    X, y, m, s = _data(gpu_device, N, d)
    D = d + 1
    g1, g2 = nt.lr_encode(X, y, m, s, 0.0, -1.0)
    exp_f = torch.cat([g1] + [g2[i, i:] for i in range(D)])
    for precision in (1e0, 1e2):
        got, got_f = nt.lr_encode_packed_many([X], [y], m, s, 0.0, -1.0, precision, floats=True)
        assert got.shape == (1, lr.n_coeffs(d, 2, 1)) and got.dtype == torch.int64
        assert torch.equal(got_f[0], exp_f)
        exp = torch.cat([lr.round_precision(g1, precision)]
                        + [lr.round_precision(g2, precision)[i, i:] for i in range(D)])
        assert torch.equal(got[0], exp)
        assert torch.equal(nt.lr_encode_packed_many([X], [y], m, s, 0.0, -1.0, precision)[0], exp)
    # against torch fp64, at the tolerances of test_lr_encode_wide_matches_torch
    Xa = lr.augment((X - m) / s)
    ref1, ref2 = Xa.T @ (2 * y.to(torch.float64) - 1), -(Xa.T @ Xa)
    ref = torch.cat([ref1] + [ref2[i, i:] for i in range(D)])
    assert torch.allclose(got_f[0], ref, rtol=1e-10, atol=1e-8), (got_f[0] - ref).abs().max()


def test_upper_plan_skips_the_block_below_the_diagonal(gpu_device):
    """d = 100 (7 x 7 tiles: tile-blocks of rows/columns 0-47, 48-95, 96-111):
    the upper plan launches every tile-block but (1, 0) -- (2, 0) and (2, 1)
    hold the level-1 row 101 -- and what it launches is the full plan's bits.
    DPs of unequal length make the slab zero-filled, so an unwritten block is
    exactly zero."""
    d = 100
    Xs = [(torch.rand(n, d, dtype=torch.float64, generator=_gen(60 + n)) * 4).to(gpu_device) for n in (70, 200)]
    ys = [torch.randint(0, 2, (n,), generator=_gen(n)).to(gpu_device) for n in (70, 200)]
    m, s = [2.0] * d, [1.15] * d
    up, D = nt._lr_launch_many(Xs, ys, m, s, 0.0, -1.0, True)
    full, _ = nt._lr_launch_many(Xs, ys, m, s, 0.0, -1.0, False)
    assert D == 101 and up.shape == full.shape == (2, 4, 112, 112)
    assert not up[:, :, 48:96, :48].any() and full[0, 0, 48:96, :48].ne(0).all()
    keep = torch.ones(112, 112, dtype=torch.bool, device=gpu_device)
    keep[48:96, :48] = False
    assert torch.equal(up[:, :, keep], full[:, :, keep])
    # up to 46 features: the one 3x3 launch as before
    Xn = [X[:, :44] for X in Xs]
    upn, _ = nt._lr_launch_many(Xn, ys, m[:44], s[:44], 0.0, -1.0, True)
    fulln, _ = nt._lr_launch_many(Xn, ys, m[:44], s[:44], 0.0, -1.0, False)
    assert upn.shape[2:] == (48, 48) and torch.equal(upn, fulln)


@pytest.mark.parametrize("d", [44, 100])
def test_packed_many_matches_single(gpu_device, d):
    """DPs of unequal length (one past a block of records): every DP of the
    batch == that DP alone, and the model layer takes the packed path."""
    rows = (70, 70, 71, 9000)
    Xs = [(torch.rand(n, d, dtype=torch.float64, generator=_gen(50 + i)) * 4).to(gpu_device)
          for i, n in enumerate(rows)]
    ys = [torch.randint(0, 2, (n,), generator=_gen(150 + i)).to(gpu_device) for i, n in enumerate(rows)]
    m, s = [2.0] * d, [1.15] * d
    many, many_f = nt.lr_encode_packed_many(Xs, ys, m, s, 0.0, -1.0, 100.0, floats=True)
    assert many.shape == (4, lr.n_coeffs(d, 2, 1))
    lp = LogisticRegressionParameters(NbrRecords=1, NbrFeatures=d, Means=m, StandardDeviations=s, Lambda=1.0,
                                      Step=0.1, MaxIterations=5, InitialWeights=[0.1] * (d + 1), K=2,
                                      PrecisionApproxCoefficients=100.0, Packing=1)
    lp0 = pk.packed_params(lp, 0)
    model = lr.encode_coefficients_int_many(Xs, ys, lp)
    assert model is not None and torch.equal(model, many)
    for i, (X, y) in enumerate(zip(Xs, ys)):
        one, one_f = nt.lr_encode_packed_many([X], [y], m, s, 0.0, -1.0, 100.0, floats=True)
        assert torch.equal(many[i], one[0]) and torch.equal(many_f[i], one_f[0])
        assert torch.equal(lr.encode_coefficients_int(X, y, lp), one[0])
        assert torch.equal(one[0], pk.upper_gather(lr.encode_coefficients_int(X, y, lp0), d))
    lp1 = pk.packed_params(lp)
    lp1.K = 1  # one level: the same vector in both layouts
    assert torch.equal(lr.encode_coefficients_int_many(Xs, ys, lp1), many[:, :d + 1])
    assert torch.equal(lr.encode_coefficients_int(Xs[2], ys[2], lp1), many[2, :d + 1])


def test_packed_strided_rows(gpu_device):
    """A column slice of a wider matrix: row stride 130, unit column stride."""
    N, d = 211, 100
    W = (torch.rand(N, 130, dtype=torch.float64, generator=_gen(7)) * 4).to(gpu_device)
    X = W[:, 17:17 + d]
    assert X.stride() == (130, 1) and not X.is_contiguous()
    y = torch.randint(0, 2, (N,), generator=_gen(8)).to(gpu_device)
    m, s = lr.compute_means_sds(X)
    a, af = nt.lr_encode_packed_many([X], [y], m, s, 0.0, -1.0, 100.0, floats=True)
    b, bf = nt.lr_encode_packed_many([X.contiguous()], [y], m, s, 0.0, -1.0, 100.0, floats=True)
    assert torch.equal(a, b) and torch.equal(af, bf)


@pytest.mark.parametrize("dataset", hd.DATASETS)
@pytest.mark.parametrize("precision", [1e0, 1e2])
def test_fixture_packed_gpu_equals_cpu(gpu_device, dataset, precision):
    X, y = hd.load(dataset, "training")
    lp = pk.packed_params(hd.lr_parameters(dataset, X, precision))
    splits = hd.dp_splits(X, y)
    cpu = [lr.encode_coefficients_int(Xi, yi, lp) for Xi, yi in splits]
    many = lr.encode_coefficients_int_many([Xi.to(gpu_device) for Xi, _ in splits],
                                           [yi.to(gpu_device) for _, yi in splits], lp)
    assert many is not None
    for i, (Xi, yi) in enumerate(splits):
        assert cpu[i].numel() == 5252
        assert torch.equal(lr.encode_coefficients_int(Xi.to(gpu_device), yi.to(gpu_device), lp).cpu(), cpu[i])
        assert torch.equal(many[i].cpu(), cpu[i])


def test_packed_query_gpu(gpu_device, tmp_path):
    """The BC query with Packing = 1, every party and the records on the GPU."""
    w, clear, lp = pk.run_packed_query("BC", gpu_device, str(tmp_path))
    assert len(clear) == hd.N_DPS and all(len(v) == 5252 for v in clear)
    tot = [sum(v[i] for v in clear) for i in range(5252)]
    exp = lr.decode_logistic_regression_values(tot, lp)
    assert len(w) == 101 and w == pytest.approx(list(exp), rel=1e-9, abs=1e-12)
    hd.check_metrics("BC", w, lp)


@pytest.mark.parametrize("packing,n_out", [(1, 27), (0, 42)])
def test_packed_query_with_proofs_gpu(gpu_device, tmp_path, packing, n_out):
    """d = 5 through every layer with proofs on: 3 CNs, 3 VNs, 3 DPs, ranges
    (16, 4, offset), random signatures, thresholds [1, 1, 1, 0, 1]."""
    from drynx_amd.services.api import DrynxClient
    from drynx_amd.services.local import local_cluster, make_survey
    from drynx_amd.wire import onet

    d, rows = 5, (50, 47, 53)
    cl, node = local_cluster(3, 3, 3, device=gpu_device, workdir=str(tmp_path))
    client = DrynxClient(node, device=gpu_device)
    node.dp_data = {}
    for i, (dp, n) in enumerate(zip(cl.dps, rows)):
        X = (torch.rand(n, d, dtype=torch.float64, generator=_gen(300 + i)) * 4).to(gpu_device)
        node.dp_data[dp.id] = (X, torch.randint(0, 2, (n,), generator=_gen(400 + i)).to(gpu_device))
    lp = LogisticRegressionParameters(NbrRecords=sum(rows), NbrFeatures=d, Means=[2.0] * d,
                                      StandardDeviations=[1.15] * d, Lambda=1.0, Step=0.012, MaxIterations=50,
                                      InitialWeights=[0.1] * (d + 1), K=2, PrecisionApproxCoefficients=100.0,
                                      Packing=packing)
    # |coefficient| <= 53 records * 1.74^2 * 100 < 16^4 / 2
    sq = make_survey(client, cl, "logistic regression", proofs=1, ranges=[16, 4, 16 ** 4 // 2], lr_params=lp,
                     thresholds=[1.0, 1.0, 1.0, 0.0, 1.0], sig_device=gpu_device)
    assert sq.Query.Operation.NbrOutput == n_out == len(sq.Query.Ranges)
    assert len(sq.Query.IVSigs.InputValidationSigs) == 3 and len(sq.Query.IVSigs.InputValidationSigs[0]) == n_out
    _, vals, res = client.send_survey_query(sq)
    assert res.block is not None
    codes = res.block.data_block().Proofs
    assert set(codes.values()) == {1}
    assert len(codes) == 3 * (3 + 3 + 3)  # VNs x (range per DP + aggregation per CN + key switch per CN)
    clear = [list(v[0]) for v in res.clear_dp.values()]
    assert len(clear) == 3 and all(len(v) == n_out for v in clear)
    tot = [sum(v[i] for v in clear) for i in range(n_out)]
    assert [int(x) for x in client.last_plaintexts[0]] == tot
    exp = lr.decode_logistic_regression_values(tot, lp)  # mirrors the packed aggregate first
    assert len(vals[0]) == d + 1 and list(vals[0]) == pytest.approx(list(exp), rel=1e-9, abs=1e-12)
    if packing == 1:
        cart = lr.unpack(tot, d, 2, 1)
        assert torch.equal(cart[1].reshape(d + 1, d + 1), cart[1].reshape(d + 1, d + 1).T)
        flat = [int(x) for x in torch.cat(cart).tolist()]
        assert exp == lr.decode_logistic_regression_values(flat, pk.packed_params(lp, 0))
    for vn in cl.vns:
        stored = {k: v for k, v in node.get_proofs(vn.id, sq.SurveyID).items() if "/range/" in k}
        assert len(stored) == 3
        for raw in stored.values():
            name, msg = onet.unmarshal(raw)
            assert name == "libdrynxrange.RangeProofListBytes" and len(msg["Data"]) == n_out
    node.close(remove=True)
