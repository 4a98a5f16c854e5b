"""Multi-target logistic regression on the GPU: the T-row encoder
(dx_lr_encode with T >= 2: level 1 of target t in row D + t of the fp64-MFMA
output, one shared level 2), its upper launch plan, the T-aware packed
reducer, and NbrTargets queries end to end.  Level-1 row t and all of level 2
must be the same bits as the single-label encoder's on (X, Y[:, t]): per
output element the products, their K-step order, the record striding and the
block reduction are the same in every instantiation.  Run with -m gpu."""
import pytest
import torch

import test_lr_targets as tg
from drynx_amd import native as nt
from drynx_amd.models import logistic_regression as lr

pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# (N, d, T): one tile | rows 15, 16 straddle a tile | rows 45..47, the headline's free rows (P stays 48) |
# row 48 makes P = 64: a wide plan under narrow D, rb = 0 | rows 47, 48 straddle the first tile-block row |
# D = 48: level 1 wholly in the second tile-block row | rows 95, 96 straddle tile-block rows 1 and 2 |
# the reference datasets' width | one record | T at its cap, fb = 0
SHAPES = [(5, 3, 2), (77, 14, 2), (123, 44, 3), (123, 44, 4), (70, 46, 2), (77, 47, 2), (64, 94, 2), (211, 100, 5),
          (1, 100, 2), (9, 2, 64)]
PADDED = {(5, 3, 2): 48, (77, 14, 2): 48, (123, 44, 3): 48, (123, 44, 4): 64, (70, 46, 2): 64, (77, 47, 2): 64,
          (64, 94, 2): 112, (211, 100, 5): 112, (1, 100, 2): 112, (9, 2, 64): 80}

_memo: dict = {}


def _case(gpu_device, N, d, T):
    """Inputs and the single-label encoder's totals per target, computed once per shape."""
    key = (str(gpu_device), N, d, T)
    if key not in _memo:
        X = (torch.rand(N, d, dtype=torch.float64, generator=_gen(N * 1000 + d)) * 4).to(gpu_device)
        Y = torch.randint(0, 2, (N, T), generator=_gen(d * 100 + T)).to(gpu_device)
        m = torch.full((d,), 2.0, dtype=torch.float64, device=gpu_device)
        s = torch.full((d,), 1.15, dtype=torch.float64, device=gpu_device)
        single = [nt.lr_encode_many([X], [Y[:, t].contiguous()], m, s, 0.0, -1.0)[0] for t in range(T)]
        _memo[key] = (X, Y, m, s, single)
    return _memo[key]


def _gather(tot: torch.Tensor, D: int, T: int) -> torch.Tensor:
    """[P, P] totals -> level 1 of every target (rows D..D+T-1), then level 2's (i, j), i <= j, row by row."""
    return torch.cat([tot[D:D + T, :D].reshape(-1)] + [tot[i, i:D] for i in range(D)])


@pytest.mark.parametrize("N,d,T", SHAPES)
def test_multi_encoder_totals(gpu_device, N, d, T):
    X, Y, m, s, single = _case(gpu_device, N, d, T)
    D = d + 1
    tot = nt.lr_encode_many([X], [Y], m, s, 0.0, -1.0)[0]
    P = PADDED[(N, d, T)]
    assert tot.shape == (P, P) and nt._lr_padded(D + T) == P
    # against torch fp64, at the tolerances of test_lr_encode_wide_matches_torch
    Xa = lr.augment((X - m) / s)
    ref1, ref2 = Xa.T @ (2 * Y.to(torch.float64) - 1), -(Xa.T @ Xa)
    assert torch.allclose(tot[D:D + T, :D], ref1.T, rtol=1e-10, atol=1e-8), (tot[D:D + T, :D] - ref1.T).abs().max()
    assert torch.allclose(tot[:D, :D], ref2, rtol=1e-10, atol=1e-8), (tot[:D, :D] - ref2).abs().max()
    # the single-label encoder on (X, Y[:, t]): the same bits
    for t in range(T):
        assert torch.equal(tot[D + t, :D], single[t][D, :D]), t
        assert torch.equal(tot[:D, :D], single[t][:D, :D]), t
    # what is neither level 1 nor level 2 is padding: nothing accumulated there
    assert not tot[D + T:, :].any() and not tot[:, D:].any()


@pytest.mark.parametrize("N,d,T", SHAPES)
def test_multi_packed_equals_cartesian(gpu_device, N, d, T):
    X, Y, m, s, single = _case(gpu_device, N, d, T)
    D = d + 1
    tot = nt.lr_encode_many([X], [Y], m, s, 0.0, -1.0)[0]
    exp_f = _gather(tot, D, T)
    for precision in (1e0, 1e2):
        got, got_f = nt.lr_encode_packed_many([X], [Y], m, s, 0.0, -1.0, precision, floats=True)
        assert got.shape == (1, lr.n_coeffs(d, 2, 1, T)) and got.dtype == torch.int64
        assert torch.equal(got_f[0].view(torch.int64), exp_f.view(torch.int64))  # every unrounded value, same bits
        assert torch.equal(got[0], lr.round_precision(exp_f, precision))
    # the model layer: both layouts, both K, against the single-label vectors
    for packing in (0, 1):
        for k in (1, 2):
            vals = lr.encode_coefficients_int(X, Y, tg.lr_params(d, N, T, packing, k, precision=1e2))
            assert vals.numel() == lr.n_coeffs(d, k, packing, T)
            one = lr.encode_coefficients_int(X, Y[:, 0], tg.lr_params(d, N, 1, packing, k, precision=1e2))
            assert torch.equal(vals[:D], one[:D]) and torch.equal(vals[T * D:], one[D:])
            if packing == 0 and k == 2:
                assert torch.equal(vals[:T * D], lr.round_precision(tot[D:D + T, :D].reshape(-1), 1e2))
                assert torch.equal(lr.pack(vals, d, 2), got[0])


def _launch_into(slab, X, Y, m, s, upper, one_cell=False):
    """The one encoder launch into a slab the caller filled: [nb, P, P].
    ``one_cell``: the grouped kernels through the identity plan, one cell that
    holds every record in order."""
    N = X.shape[0]
    p = nt._lr_prepare([X], [Y], m, s, 0.0)
    assert slab.shape == (nt._lr_blocks(N), p.P, p.P)
    cells = None
    if one_cell:
        cells = (torch.arange(N, device=X.device), torch.tensor([0, N], device=X.device), 0, nt._lr_blocks(N))
    nt._lr_launch(p, X, nt._lr_labels(p, X, Y), 0.0, -1.0, slab, slab.shape[0], upper, cells)
    return slab


# the wide shapes (P > 48) and which 48-row tile-blocks (Y, Z) the upper plan skips; the last two: the single-label
# kernels at the smallest shapes with a skipped tile-block and with a ragged edge
@pytest.mark.parametrize("N,d,T,skipped", [(123, 44, 4, []), (70, 46, 2, []), (77, 47, 2, []), (64, 94, 2, []),
                                           (211, 100, 5, [(1, 0)]), (1, 100, 2, [(1, 0)]), (9, 2, 64, []),
                                           (130, 150, 3, [(1, 0), (2, 0), (2, 1)]),
                                           (211, 100, 1, [(1, 0)]), (123, 44, 1, [])])
def test_upper_plan_writes_what_the_packed_reducer_reads(gpu_device, N, d, T, skipped):
    """The slab pre-filled with NaN: the packed reducer's output has no NaN,
    so every element it reads is written and nothing skipped is read; the
    skipped tile-blocks (strictly below the diagonal, no row >= D) stay NaN,
    the padding column tiles too; everything written is the full plan's bits."""
    _check_upper_plan(gpu_device, N, d, T, skipped, False)


@pytest.mark.parametrize("N,d,T,skipped", [(211, 100, 1, [(1, 0)]), (211, 100, 5, [(1, 0)]), (123, 44, 4, [])])
def test_upper_plan_of_the_grouped_kernels(gpu_device, N, d, T, skipped):
    """The same through the grouped instantiations (one cell holding every
    record in order), and each slab is the ungrouped one element for element
    wherever either is written."""
    _check_upper_plan(gpu_device, N, d, T, skipped, True)


def _check_upper_plan(gpu_device, N, d, T, skipped, grouped):
    D = d + 1
    P = nt._lr_padded(D + T)
    X = (torch.rand(N, d, dtype=torch.float64, generator=_gen(N + d)) * 4).to(gpu_device)
    Y = torch.randint(0, 2, (N, T), generator=_gen(T)).to(gpu_device)
    m = torch.full((d,), 2.0, dtype=torch.float64, device=gpu_device)
    s = torch.full((d,), 1.15, dtype=torch.float64, device=gpu_device)
    nb = nt._lr_blocks(N)
    nan = float("nan")

    def launch(upper, one_cell):
        return _launch_into(torch.full((nb, P, P), nan, dtype=torch.float64, device=gpu_device), X, Y, m, s, upper,
                            one_cell)

    up, full = launch(True, grouped), launch(False, grouped)
    if grouped:
        for mine, ungrouped in ((up, launch(True, False)), (full, launch(False, False))):
            assert torch.equal(torch.isnan(mine), torch.isnan(ungrouped))
            assert torch.equal(mine.nan_to_num(0.0), ungrouped.nan_to_num(0.0))
    got, got_f = nt.lr_reduce_pack(up, D, 100.0, floats=True, T=T)
    assert got.shape == (1, T * D + D * (D + 1) // 2) and not torch.isnan(got_f).any()
    ref, ref_f = nt.lr_reduce_pack(full, D, 100.0, floats=True, T=T)
    assert torch.equal(got, ref) and torch.equal(got_f, ref_f)
    # written by the full plan: every row tile by the column tiles that hold a column < D
    wc = 16 * ((D + 15) // 16)
    assert not torch.isnan(full[:, :, :wc]).any() and torch.isnan(full[:, :, wc:]).all()
    keep = torch.zeros(P, P, dtype=torch.bool, device=gpu_device)
    keep[:, :wc] = True
    for (bi, bj) in skipped:
        assert 48 * (bi + 1) <= D and bj < bi
        keep[48 * bi:48 * bi + 48, 48 * bj:48 * bj + 48] = False
    assert torch.isnan(up[:, ~keep]).all()
    assert torch.equal(up[:, keep], full[:, keep])
    assert torch.equal(got_f[0], _gather(nt.lr_reduce(full[None])[0].nan_to_num(0.0), D, T))


def test_strided_label_columns_and_rows(gpu_device):
    """Y as a column slice of a wider matrix (row stride 9), X as one too (row stride 130)."""
    N, d, T = 211, 100, 5
    W = (torch.rand(N, 130, dtype=torch.float64, generator=_gen(7)) * 4).to(gpu_device)
    X = W[:, 17:17 + d]
    L = torch.randint(0, 2, (N, 9), generator=_gen(8)).to(gpu_device)
    Lf = L.to(torch.float64)
    for Y in (L[:, 2:2 + T], Lf[:, 2:2 + T]):
        assert Y.stride() == (9, 1) and not Y.is_contiguous()
        m, s = lr.compute_means_sds(X)
        a = nt.lr_encode_many([X], [Y], m, s, 0.0, -1.0)
        b = nt.lr_encode_many([X.contiguous()], [Y.contiguous()], m, s, 0.0, -1.0)
        assert torch.equal(a, b)
        pa, fa = nt.lr_encode_packed_many([X], [Y], m, s, 0.0, -1.0, 100.0, floats=True)
        pb, fb = nt.lr_encode_packed_many([X.contiguous()], [Y.contiguous()], m, s, 0.0, -1.0, 100.0, floats=True)
        assert torch.equal(pa, pb) and torch.equal(fa, fb)
        assert torch.equal(fa[0], _gather(a[0], d + 1, T))
    # a column order other than unit stride is copied, not misread
    Yt = L.t().contiguous().t()[:, 2:2 + T]
    assert Yt.stride() == (1, N) and torch.equal(Yt, L[:, 2:2 + T])
    assert torch.equal(nt.lr_encode_many([X], [Yt], m, s, 0.0, -1.0), a)


@pytest.mark.parametrize("d,T", [(44, 3), (46, 2), (100, 5)])
def test_unequal_dps_in_one_batch(gpu_device, d, T):
    """4 DPs of unequal length, one of a single record, one past a block of
    records: every DP of the batch == that DP alone, in both layouts."""
    rows = (70, 1, 71, 9000)
    data = [(X.to(gpu_device), Y.to(gpu_device)) for X, Y in tg.dp_records(rows, d, T, seed=50)]
    Xs, Ys = [X for X, _ in data], [Y for _, Y in data]
    for packing in (0, 1):
        for k in (1, 2):
            lp = tg.lr_params(d, 1, T, packing, k, precision=1e2)
            many = lr.encode_coefficients_int_many(Xs, Ys, lp)
            assert many is not None and many.shape == (4, lr.n_coeffs(d, k, packing, T))
            for i, (X, Y) in enumerate(data):
                assert torch.equal(many[i], lr.encode_coefficients_int(X, Y, lp)), (packing, k, i)
                one = lr.encode_coefficients_int_many([X], [Y], lp)
                assert torch.equal(many[i], one[0])
    D = d + 1
    lp0 = tg.lr_params(d, 1, T, 0, 2, precision=1e2)
    many = lr.encode_coefficients_int_many(Xs, Ys, lp0)
    for i, (X, Y) in enumerate(data):
        for t in range(T):
            one = lr.encode_coefficients_int(X, Y[:, t], tg.lr_params(d, 1, 0, 0, 2, precision=1e2))
            assert torch.equal(many[i, t * D:(t + 1) * D], one[:D]) and torch.equal(many[i, T * D:], one[D:])


def test_one_target_is_the_single_label_path(gpu_device):
    """[N, 1] labels == [N] labels exactly, and NbrTargets 0 / 1 queries encode the parent's vectors."""
    for (N, d) in ((123, 44), (211, 100)):
        X, Y, m, s, single = _case(gpu_device, N, d, 5 if d == 100 else 3)
        y = Y[:, 0].contiguous()
        a = nt.lr_encode_many([X], [y], m, s, 0.0, -1.0)
        assert torch.equal(a[0], single[0])
        assert torch.equal(nt.lr_encode_many([X], [Y[:, :1]], m, s, 0.0, -1.0), a)
        pa, fa = nt.lr_encode_packed_many([X], [y], m, s, 0.0, -1.0, 100.0, floats=True)
        pb, fb = nt.lr_encode_packed_many([X], [Y[:, :1]], m, s, 0.0, -1.0, 100.0, floats=True)
        assert torch.equal(pa, pb) and torch.equal(fa, fb)
        g1, g2 = nt.lr_encode(X, y, m, s, 0.0, -1.0)
        D = d + 1
        for packing in (0, 1):
            cart = torch.cat([lr.round_precision(g1, 1e2), lr.round_precision(g2, 1e2).reshape(-1)])
            exp = cart if packing == 0 else lr.pack(cart, d, 2)
            for T in (0, 1):
                lp = tg.lr_params(d, N, T, packing, 2, precision=1e2)
                assert torch.equal(lr.encode_coefficients_int(X, y, lp), exp)
                assert torch.equal(lr.encode_coefficients_int_many([X], [y], lp)[0], exp)
                assert torch.equal(lr.encode_coefficients_int(X, Y[:, :1], lp), exp)
        assert exp.numel() == D + D * (D + 1) // 2


def test_native_refusals(gpu_device):
    X, Y, m, s, _ = _case(gpu_device, 9, 2, 64)
    Y65 = torch.cat([Y, Y[:, :1]], 1)
    with pytest.raises(RuntimeError, match="rc=-2"):
        nt.lr_encode_many([X], [Y65], m, s, 0.0, -1.0)
    with pytest.raises(ValueError):
        nt.lr_encode_many([X], [Y], m, s, 1.0, -1.0)  # no label-dependent level-2 weight with several labels
    with pytest.raises(ValueError):
        nt.lr_encode_many([X, X], [Y, Y[:, :2]], m, s, 0.0, -1.0)  # one T per batch
    slab = torch.zeros((1, 1, 48, 48), dtype=torch.float64, device=gpu_device)
    with pytest.raises(ValueError):
        nt.lr_reduce_pack(slab, 45, 1.0, T=4)  # row 48 is outside a 48 x 48 block
    assert nt.lr_reduce_pack(slab, 45, 1.0, T=3).shape == (1, 3 * 45 + 45 * 46 // 2)


# ----------------------------------------------------------------------------- queries
def test_targets_query_gpu(gpu_device, tmp_path):
    tg.check_targets_query(gpu_device, tmp_path)


@pytest.mark.parametrize("packing", [0, 1])
def test_targets_query_with_proofs_gpu(gpu_device, tmp_path, packing):
    tg.check_proofs_query(gpu_device, tmp_path, packing)
