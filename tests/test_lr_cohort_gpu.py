"""Logistic regression over SQL cohorts on the GPU: the cell plan
(dx_group_cells, a stable sort) and the grouped fused encoder
(dx_lr_encode with a cell plan: the fp64-MFMA tile-block body with the rows read through
the plan, a cell's record blocks one more factor of the grid) against the host
model on exact inputs -- every sum is exact in fp64 in any order, so the
comparison is ``torch.equal`` -- the anchors to the ungrouped encoder and the
grouped moments, and cohort queries end to end.  Run with -m gpu."""
import pytest
import torch

import test_lr_cohort as tc
from drynx_amd import native as nt
from drynx_amd.models import logistic_regression as lr

pytestmark = pytest.mark.gpu

# (N, d, T): one tile, one record | a few K-steps | the P = 48 diagonal block, one label |
# three labels in its spare rows | D = 48: P = 64, a wide plan under two labels | d = 100: P = 112, a ragged edge
SHAPES = [(1, 3, 1), (37, 3, 1), (123, 44, 1), (123, 44, 3), (77, 47, 2), (211, 100, 1)]

_memo: dict = {}


def _case(dev, N, d, T):
    """Exact records, their key tables and the host model's vectors, once per shape."""
    key = (str(dev), N, d, T)
    if key not in _memo:
        X, y = tc.exact_records(N, d, T)
        tables = tc.key_tables(N)
        if N == 123:
            tables["wide"] = tc.wide_table(N)  # G = 4096, almost every cell empty
        ref = {}
        for name, (K, plan) in tables.items():
            for packing in (0, 1):
                ref[name, packing] = tc.host_cells(X, y, K, tc.lr_params(d, N, T if T > 1 else 0, packing), plan)
        m = torch.full((d,), tc.MEAN, dtype=torch.float64, device=dev)
        s = torch.full((d,), tc.SD, dtype=torch.float64, device=dev)
        _memo[key] = (X.to(dev), y.to(dev), {n: (K.to(dev), plan) for n, (K, plan) in tables.items()}, ref, m, s)
    return _memo[key]


def _levels(tot, D, T):
    """[.., P, P] totals -> [.., T*D + D*D]: level 1 of every target, then level 2 row by row."""
    lead = tot.shape[:-2]
    return torch.cat([tot[..., D:D + T, :D].reshape(*lead, -1), tot[..., :D, :D].reshape(*lead, -1)], -1)


@pytest.mark.parametrize("N,d,T", SHAPES)
def test_grouped_encoder_is_the_host_model(gpu_device, N, d, T):
    X, y, tables, ref, m, s = _case(gpu_device, N, d, T)
    D = d + 1
    P = nt._lr_padded(D + T)
    for name, (K, plan) in tables.items():
        keys, filters = tc.terms(plan)
        G = ref[name, 0].shape[0]
        tot = nt.lr_encode_cells_many([X], [y], [K], m, s, -1.0, keys, filters)
        assert tot.shape == (1, G, P, P), name
        # exact inputs: the totals times 4 are the host model's integers, exactly
        assert torch.equal(_levels(tot[0], D, T) * tc.PRECISION, ref[name, 0].to(gpu_device).to(torch.float64)), name
        # what is neither level 1 nor level 2 is padding: nothing accumulated there
        assert not tot[0, :, D + T:, :].any() and not tot[0, :, :, D:].any(), name
        assert torch.equal(tot, nt.lr_encode_cells_many([X], [y], [K], m, s, -1.0, keys, filters)), name
        packed, packed_f = nt.lr_encode_cells_packed_many([X], [y], [K], m, s, -1.0, keys, filters, tc.PRECISION,
                                                          floats=True)
        assert torch.equal(packed[0], ref[name, 1].to(gpu_device)), name
        assert torch.equal(packed_f[0] * tc.PRECISION, packed[0].to(torch.float64)), name
        # the model layer, both layouts
        for packing in (0, 1):
            got = lr.encode_coefficients_int_cells(X, y, K, tc.lr_params(d, N, T if T > 1 else 0, packing), plan)
            assert got.dtype == torch.int64 and torch.equal(got.cpu(), ref[name, packing]), (name, packing)
        if name == "all_dropped":
            assert not tot.any() and not packed.any()


@pytest.mark.parametrize("N,d,T", SHAPES)
def test_strided_inputs_and_unequal_batches(gpu_device, N, d, T):
    X, y, tables, ref, m, s = _case(gpu_device, N, d, T)
    wide = torch.cat([torch.full((N, 5), 7.0, dtype=torch.float64, device=gpu_device), X,
                      torch.full((N, 2), 7.0, dtype=torch.float64, device=gpu_device)], 1)
    Xv = wide[:, 5:5 + d]
    assert Xv.stride() == (d + 7, 1) and torch.equal(Xv, X)
    # a second DP of another length: the first two thirds of the records, the other way round
    n2 = max(1, 2 * N // 3)
    idx = torch.arange(n2 - 1, -1, -1, device=gpu_device)
    for name in ("sizes", "where", "two_columns"):
        K, plan = tables[name]
        keys, filters = tc.terms(plan)
        Kw = torch.cat([torch.full((N, 3), 9, device=gpu_device), K, torch.full((N, 1), 9, device=gpu_device)], 1)
        Kv = Kw[:, 3:3 + K.shape[1]]
        assert Kv.stride() == (K.shape[1] + 4, 1)
        one = nt.lr_encode_cells_many([X], [y], [K], m, s, -1.0, keys, filters)
        assert torch.equal(nt.lr_encode_cells_many([Xv], [y], [Kv], m, s, -1.0, keys, filters), one), name
        onep = nt.lr_encode_cells_packed_many([X], [y], [K], m, s, -1.0, keys, filters, tc.PRECISION)
        assert torch.equal(nt.lr_encode_cells_packed_many([Xv], [y], [Kv], m, s, -1.0, keys, filters, tc.PRECISION),
                           onep), name
        X2, y2, K2 = X[idx], y[idx], K[idx]
        two = nt.lr_encode_cells_many([X2], [y2], [K2], m, s, -1.0, keys, filters)
        many = nt.lr_encode_cells_many([X2, X, X2[:1]], [y2, y, y2[:1]], [K2, K, K2[:1]], m, s, -1.0, keys, filters)
        assert torch.equal(many[1:2], one) and torch.equal(many[0:1], two), name
        manyp = nt.lr_encode_cells_packed_many([X2, X], [y2, y], [K2, K], m, s, -1.0, keys, filters, tc.PRECISION)
        assert torch.equal(manyp[1:2], onep), name
        p = tc.lr_params(d, N, T if T > 1 else 0, 0)
        got = lr.encode_coefficients_int_cells_many([X2, None, X], [y2, None, y], [K2, None, K], p, plan)
        assert torch.equal(got[2].cpu(), ref[name, 0]) and not got[1].any()
        assert torch.equal(got[0].cpu(), tc.host_cells(X2, y2, K2, p, plan))


@pytest.mark.parametrize("N,d,T", [(123, 44, 1), (123, 44, 3), (211, 100, 1)])
def test_windows_give_the_one_window_bits(gpu_device, N, d, T):
    """G = 7 in windows of 3, 2 and 1 cells: the result of the one-window call, bit for bit."""
    X, y, tables, ref, m, s = _case(gpu_device, N, d, T)
    K, plan = tables["sizes"]
    keys, filters = tc.terms(plan)
    P = nt._lr_padded(d + 1 + T)
    nbc = nt._lr_cell_blocks(N, 7)
    block = nbc * P * P * 8
    assert 7 * block < nt.LR_CELLS_MAX_SLAB_BYTES
    one = nt.lr_encode_cells_many([X], [y], [K], m, s, -1.0, keys, filters)
    onep = nt.lr_encode_cells_packed_many([X], [y], [K], m, s, -1.0, keys, filters, tc.PRECISION)
    for cells in (3, 2, 1):  # 3, 4 and 7 windows
        cap = cells * block + block // 2
        assert torch.equal(nt.lr_encode_cells_many([X], [y], [K], m, s, -1.0, keys, filters, max_slab_bytes=cap), one)
        assert torch.equal(nt.lr_encode_cells_packed_many([X], [y], [K], m, s, -1.0, keys, filters, tc.PRECISION,
                                                          max_slab_bytes=cap), onep)
    assert torch.equal(nt.lr_encode_cells_many([X], [y], [K], m, s, -1.0, keys, filters, max_slab_bytes=1), one)
    # the upper plan with the full reducer: what it launches is the full plan's bits, the rest zero
    up = nt.lr_encode_cells_many([X], [y], [K], m, s, -1.0, keys, filters, upper=True)
    D = d + 1
    iu = torch.triu(torch.ones(D, D, dtype=torch.bool, device=gpu_device))
    assert torch.equal(up[0, :, :D, :D][:, iu], one[0, :, :D, :D][:, iu])
    assert torch.equal(up[0, :, D:D + T, :D], one[0, :, D:D + T, :D])


# ----------------------------------------------------------------------------- anchors to existing code
@pytest.mark.parametrize("N,d,T", [(123, 44, 1), (123, 44, 3), (211, 100, 1), (9000, 44, 1), (70001, 5, 2)])
def test_one_cell_is_the_ungrouped_encoder(gpu_device, N, d, T):
    """G = 1 without a Where: the bits of lr_encode_many / lr_encode_packed_many on arbitrary real features."""
    g = torch.Generator().manual_seed(N + d)
    X = (torch.rand(N, d, dtype=torch.float64, generator=g) * 4).to(gpu_device)
    y = torch.randint(0, 2, (N,) if T == 1 else (N, T), generator=g).to(gpu_device)
    m, s = [2.0] * d, [1.15] * d
    assert nt._lr_cell_blocks(N, 1) == nt._lr_blocks(N)
    ref = nt.lr_encode_many([X], [y], m, s, 0.0, -1.0)
    for K in (None, torch.zeros((N, 1), dtype=torch.int64, device=gpu_device)):
        keys = [] if K is None else [(0, 0, 1)]
        got = nt.lr_encode_cells_many([X], [y], [K], m, s, -1.0, keys, [])
        assert got.shape == (1, 1) + tuple(ref.shape[1:])
        D = d + 1
        if ref.shape[-1] == 48 or (D + 15) // 16 == ref.shape[-1] // 16:
            assert torch.equal(got[:, 0], ref)
        else:  # the ungrouped slab leaves the padding column tiles unwritten; everything live is the same bits
            assert torch.equal(got[:, 0, :, :D], ref[:, :, :D])
        refp, reff = nt.lr_encode_packed_many([X], [y], m, s, 0.0, -1.0, 100.0, floats=True)
        gotp, gotf = nt.lr_encode_cells_packed_many([X], [y], [K], m, s, -1.0, keys, [], 100.0, floats=True)
        assert torch.equal(gotp[:, 0], refp) and torch.equal(gotf[:, 0], reff)


def test_counts_match_group_moments_gpu(gpu_device):
    tc.check_counts_match_group_moments(gpu_device)
    # the encoder's own totals: -total[0, 0] per cell
    N, d = 123, 3
    X, y, tables, _, m, s = _case(gpu_device, 123, 44, 1)
    for name, (K, plan) in tables.items():
        keys, filters = tc.terms(plan)
        tot = nt.lr_encode_cells_many([X], [y], [K], m, s, -1.0, keys, filters)
        gm = nt.group_moments(torch.zeros((N, 0), dtype=torch.int64, device=gpu_device), K, [N], [(0, 0)], keys,
                              filters)
        assert torch.equal((-tot[0, :, 0, 0]).to(torch.int64), gm[0, :, 0]), name


@pytest.mark.parametrize("N,d,T", [(123, 44, 3), (77, 47, 2), (211, 100, 1), (5000, 44, 1)])
def test_real_features_against_torch(gpu_device, N, d, T):
    """Real features, G = 6 with a Where: torch fp64 per cell at test_lr_targets_gpu's tolerances."""
    g = torch.Generator().manual_seed(3 * N + d)
    X = (torch.rand(N, d, dtype=torch.float64, generator=g) * 4).to(gpu_device)
    Y = torch.randint(0, 2, (N, T), generator=g).to(gpu_device)
    K = torch.stack([torch.randint(0, 3, (N,), generator=g), torch.randint(0, 2, (N,), generator=g),
                     torch.randint(0, 4, (N,), generator=g)], 1).to(gpu_device)
    plan = tc.plan_of([(0, 3), (1, 2)], [(2, 1)])
    keys, filters = tc.terms(plan)
    m = torch.full((d,), 2.0, dtype=torch.float64, device=gpu_device)
    s = torch.full((d,), 1.15, dtype=torch.float64, device=gpu_device)
    tot = nt.lr_encode_cells_many([X], [Y if T > 1 else Y[:, 0]], [K], m, s, -1.0, keys, filters)[0]
    ids, G = lr.cell_ids(K, plan)
    assert G == 6 and int((ids < G).sum()) > N // 8 and int(torch.bincount(ids, minlength=7)[:6].max()) >= 4
    D = d + 1
    Xa = lr.augment((X - m) / s)
    for c in range(G):
        rows = (ids == c).nonzero().reshape(-1)
        if rows.numel() == 0:  # a small N may leave a cell of the six empty
            assert not tot[c].any()
            continue
        A = Xa[rows]
        ref1, ref2 = A.T @ (2 * Y[rows].to(torch.float64) - 1), -(A.T @ A)
        got1, got2 = tot[c, D:D + T, :D], tot[c, :D, :D]
        assert torch.allclose(got1, ref1.T, rtol=1e-10, atol=1e-8), (got1 - ref1.T).abs().max()
        assert torch.allclose(got2, ref2, rtol=1e-10, atol=1e-8), (got2 - ref2).abs().max()


def test_native_refusals(gpu_device):
    X, y, tables, _, m, s = _case(gpu_device, 37, 3, 1)
    K, plan = tables["where"]
    with pytest.raises(ValueError, match="column 2"):
        nt.lr_encode_cells_many([X], [y], [K], m, s, -1.0, [(2, 0, 3)], [])
    with pytest.raises(ValueError, match="rows"):
        nt.lr_encode_cells_many([X], [y], [K[:5]], m, s, -1.0, [(0, 0, 3)], [])
    with pytest.raises(ValueError, match="key columns"):
        nt.lr_encode_cells_many([X], [y], [K], m, s, -1.0, [(0, 0, 2)] * 5, [])
    with pytest.raises(AssertionError):
        nt.lr_encode_cells_many([X], [y], [K.to(torch.int32)], m, s, -1.0, [(0, 0, 3)], [])
    with pytest.raises(ValueError, match="per DP"):
        nt.lr_encode_cells_many([X], [y], [K, K], m, s, -1.0, [(0, 0, 3)], [])


# ----------------------------------------------------------------------------- queries
def test_cohort_queries_gpu(gpu_device, tmp_path):
    tc.check_cohort_queries(gpu_device, tmp_path)


def test_cohort_query_with_proofs_gpu(gpu_device, tmp_path):
    tc.check_cohort_proofs(gpu_device, tmp_path)
