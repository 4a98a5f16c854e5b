"""The fp64-MFMA logistic-regression encoder past one 48x48 output block
(csrc/kernels/dx_lr.hip: a grid of tile-blocks), up to the reference's
100-feature BC and GSE queries end to end on the GPU.  Run with -m gpu."""
import pytest
import torch

import test_lr_highdim as hd
from drynx_amd import native as nt
from drynx_amd.models import logistic_regression as lr
from drynx_amd.query import LogisticRegressionParameters

pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# the first column past the old limit, tile and tile-block boundaries, N below 4
# and not a multiple of 4, more than one block of records
@pytest.mark.parametrize("N,D", [(123, 49), (70, 101), (4099, 112), (5, 128), (257, 129), (1, 64)])
def test_lr_moments_wide_matches_fp64(gpu_device, N, D):
    X = torch.randn(N, D, dtype=torch.float64, generator=_gen(N * 1000 + D)).to(gpu_device)
    w = torch.randn(N, dtype=torch.float64, generator=_gen(D)).to(gpu_device)
    ref = (X * w[:, None]).T @ X
    got = nt.lr_moments(X, w)
    assert got.shape == (D, D)
    assert torch.allclose(got, ref, rtol=1e-10, atol=1e-9), (got - ref).abs().max()


def _encode_reference(X, y):
    m, s = lr.compute_means_sds(X)
    Xa = lr.augment((X - m) / s)
    return m, s, Xa.T @ (2 * y.to(torch.float64) - 1), -(Xa.T @ Xa)


# the level-1 row D = d + 1 on the first row of a new tile (d = 47, 63, 111,
# 127), of a new tile-block (d = 47: row 48; d = 95 would be the next), and in
# mid-tile (d = 62, 100, 126)
@pytest.mark.parametrize("N,d", [(77, 47), (1001, 62), (4099, 63), (70, 100), (211, 100), (5, 111), (3, 126),
                                 (130, 127), (1, 100)])
def test_lr_encode_wide_matches_torch(gpu_device, N, d):
    X = (torch.rand(N, d, dtype=torch.float64, generator=_gen(N * 1000 + d)) * 4).to(gpu_device)
    y = torch.randint(0, 2, (N,), generator=_gen(d)).to(gpu_device)
    if N == 1:  # a single record has no spread to standardise with
        m = torch.full((d,), 2.0, dtype=torch.float64, device=gpu_device)
        s = torch.full((d,), 1.15, dtype=torch.float64, device=gpu_device)
        Xa = lr.augment((X - m) / s)
        ref1, ref2 = Xa.T @ (2 * y.to(torch.float64) - 1), -(Xa.T @ Xa)
    else:
        m, s, ref1, ref2 = _encode_reference(X, y)
    g1, g2 = nt.lr_encode(X, y, m, s, 0.0, -1.0)
    assert g1.shape == (d + 1,) and g2.shape == (d + 1, d + 1)
    assert torch.allclose(g1, ref1, rtol=1e-10, atol=1e-8), (g1 - ref1).abs().max()
    assert torch.allclose(g2, ref2, rtol=1e-10, atol=1e-8), (g2 - ref2).abs().max()


def test_lr_encode_wide_strided_rows(gpu_device):
    """A column slice of a wider matrix: row stride 130, unit column stride."""
    N, d = 211, 100
    W = (torch.rand(N, 130, dtype=torch.float64, generator=_gen(7)) * 4).to(gpu_device)
    X = W[:, 17:17 + d]
    assert X.stride() == (130, 1) and not X.is_contiguous()
    y = torch.randint(0, 2, (N,), generator=_gen(8)).to(gpu_device)
    m, s, ref1, ref2 = _encode_reference(X, y)
    g1, g2 = nt.lr_encode(X, y, m, s, 0.0, -1.0)
    assert torch.allclose(g1, ref1, rtol=1e-10, atol=1e-8), (g1 - ref1).abs().max()
    assert torch.allclose(g2, ref2, rtol=1e-10, atol=1e-8), (g2 - ref2).abs().max()
    c1, c2 = nt.lr_encode(X.contiguous(), y, m, s, 0.0, -1.0)
    assert torch.equal(g1, c1) and torch.equal(g2, c2)


def _many_vs_single(gpu_device, d, rows, seed):
    Xs = [(torch.rand(n, d, dtype=torch.float64, generator=_gen(seed + i)) * 4).to(gpu_device)
          for i, n in enumerate(rows)]
    ys = [torch.randint(0, 2, (n,), generator=_gen(seed + 100 + i)).to(gpu_device) for i, n in enumerate(rows)]
    m, s = [2.0] * d, [1.15] * d
    tot = nt.lr_encode_many(Xs, ys, m, s, 0.0, -1.0)
    D = d + 1
    mt = torch.tensor(m, dtype=torch.float64, device=gpu_device)
    st = torch.tensor(s, dtype=torch.float64, device=gpu_device)
    for i, (X, y) in enumerate(zip(Xs, ys)):
        g1, g2 = nt.lr_encode(X, y, mt, st, 0.0, -1.0)
        assert torch.equal(tot[i, D, :D], g1) and torch.equal(tot[i, :D, :D], g2)
    lp = LogisticRegressionParameters(NbrRecords=1, NbrFeatures=d, Means=m, StandardDeviations=s, Lambda=1.0,
                                      Step=0.1, MaxIterations=5, InitialWeights=[0.1] * D, K=2,
                                      PrecisionApproxCoefficients=100.0)
    many = lr.encode_coefficients_int_many(Xs, ys, lp)
    assert many is not None and many.shape == (len(rows), lr.n_coeffs(d, 2))
    for i, (X, y) in enumerate(zip(Xs, ys)):
        assert torch.equal(many[i], lr.encode_coefficients_int(X, y, lp))
    return tot


def test_lr_encode_many_wide_matches_single(gpu_device):
    """d = 100, DPs of unequal length (one past a block of records): every DP
    of the batch == that DP alone, bit for bit, floats and rounded integers."""
    tot = _many_vs_single(gpu_device, 100, (70, 70, 71, 9000), 20)
    assert tot.shape[1] == tot.shape[2] >= 102


def test_lr_encode_many_narrow_keeps_48(gpu_device):
    """d = 44: still one 48x48 block per DP, batch == single bit for bit."""
    tot = _many_vs_single(gpu_device, 44, (70, 70, 71, 9000), 40)
    assert tot.shape[1:] == (48, 48)


@pytest.mark.parametrize("dataset", hd.DATASETS)
@pytest.mark.parametrize("precision", [1e0, 1e2])
def test_fixture_coefficients_gpu_equal_cpu(gpu_device, dataset, precision):
    """The integer coefficient vectors of every DP split: fused GPU encoder ==
    the CPU torch path, exactly (every |coefficient * precision| of these
    inputs lies at least 5.8e-6 from a .5 rounding boundary; the two fp64
    paths differ by about 1e-12 on 70-row sums)."""
    X, y = hd.load(dataset, "training")
    lp = hd.lr_parameters(dataset, X, precision)
    splits = hd.dp_splits(X, y)
    cpu = [lr.encode_coefficients_int(Xi, yi, lp) for Xi, yi in splits]
    many = lr.encode_coefficients_int_many([Xi.to(gpu_device) for Xi, _ in splits],
                                           [yi.to(gpu_device) for _, yi in splits], lp)
    assert many is not None
    for i, (Xi, yi) in enumerate(splits):
        assert cpu[i].numel() == 10302
        one = lr.encode_coefficients_int(Xi.to(gpu_device), yi.to(gpu_device), lp)
        assert torch.equal(one.cpu(), cpu[i])
        assert torch.equal(many[i].cpu(), cpu[i])


@pytest.mark.parametrize("dataset", hd.DATASETS)
def test_highdim_query_gpu(gpu_device, tmp_path, dataset):
    """The BC / GSE query with every party and the DPs' records on the GPU."""
    w, exp, lp = hd.run_query(dataset, gpu_device, str(tmp_path))
    assert len(w) == 101
    assert w == pytest.approx(exp, rel=1e-9, abs=1e-12)
    hd.check_metrics(dataset, w, lp)
