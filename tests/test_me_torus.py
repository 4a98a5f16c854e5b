"""First pass of the verifier's GT multi-exponentiation on torus images
(csrc/kernels/dx_me_torus.hip), host paths, against the Fp12 path bit for
bit: the image rows against the ledger's compression, the slice products and
the whole device-plan multi-exponentiation against the Fp12 kernels, and the
verifier's verdicts with DRYNX_ME_TORUS=0 and 1 on clean and forged lists."""
import random

import pytest
import torch

from drynx_amd import native as nt
from drynx_amd.crypto import bn254 as bn
from drynx_amd.crypto import elgamal as eg
from drynx_amd.crypto import oracle as O
from drynx_amd.ops.encoding import CreateProofBatch
from drynx_amd.proofs import range_proof as rp

RNG = random.Random(20261)


@pytest.fixture(scope="module")
def gt_pool():
    """64 random GT elements (powers of four e(P, Q)^x), shared and never modified."""
    g = O.pairing(O.G1_GEN, O.G2_GEN)
    base = bn.gt_tensor([g ** RNG.randrange(1, O.R) for _ in range(4)], "cpu")
    k = bn.scalars_tensor([RNG.randrange(O.R) for _ in range(64)], "cpu")
    return nt.gt_pow(base.repeat(16, 1).contiguous(), k)


def _with_ones(rows: torch.Tensor, ones) -> torch.Tensor:
    a = rows.clone()
    for i in ones:
        a[i] = nt.gt_one("cpu")[0]
    return a


# ----------------------------------------------------------------------------- gt_beta_rows
@pytest.mark.parametrize("rows_per_inv", [1, 3, 8])
@pytest.mark.parametrize("m", [1, 8, 19])
@pytest.mark.parametrize("one_at", ["none", "first", "last"])
def test_beta_rows_match_ledger_compression(gt_pool, m, rows_per_inv, one_at):
    """Both halves against gt_t2_compress limb for limb; the row of 1 is the
    all-zero skip mark.  m = 19 leaves a ragged last chunk (one row at 3 rows
    per inversion, so the row of 1 is alone in it; three at 8); one row per
    inversion and m = 1 put every row alone."""
    ones = {"none": [], "first": [0], "last": [m - 1]}[one_at]
    a = _with_ones(gt_pool[:m], ones)
    beta2 = nt.gt_beta_rows(a, rows_per_inv)
    assert tuple(beta2.shape) == (2 * m, 48)
    c, ok = nt.gt_t2_compress(a)
    cf, okf = nt.gt_t2_compress(nt.gt_frob8(a))
    for i in range(m):
        if i in ones:
            assert not ok[i] and not okf[i]
            assert not beta2[i].any() and not beta2[m + i].any()
        else:
            assert ok[i] and okf[i]
            assert torch.equal(beta2[i], c[i]), i
            assert torch.equal(beta2[m + i], cf[i]), i


def test_beta_rows_noncanonical_zero_h_spares_its_chunk(gt_pool):
    """A row validate_list rejects must not spoil the rows that share its
    inversion: h = (p, 0, ..) is a non-canonical 0 with non-zero limbs."""
    a = gt_pool[:8].clone()
    a[3] = nt.gt_one("cpu")[0]
    a[3, 48:56] = bn.to_tensor(bn.ints_to_limbs([O.P]), "cpu")[0]
    beta2 = nt.gt_beta_rows(a, 8)
    c, ok = nt.gt_t2_compress(gt_pool[:8].contiguous())
    for i in range(8):
        if i == 3:
            assert not beta2[i].any() and not beta2[8 + i].any()
        else:
            assert ok[i] and torch.equal(beta2[i], c[i]), i


# ----------------------------------------------------------------------------- gt_beta_slice_prod
def test_beta_slice_prod_matches_fp12_slices(gt_pool):
    """pi of the numerators == the Fp12 slice products, for slice lengths
    0, 1, 2, 9, 17 (and 1, 3 for the skip cases), contiguous and gathered; a
    row of 1 opens a slice (row 3), sits inside one (rows 20, 31) and is a
    slice's only row (row 29)."""
    n = 40
    src = _with_ones(gt_pool[:n], [3, 20, 29, 31])
    beta = nt.gt_beta_rows(src, 8)[:n].contiguous()
    lens = [0, 1, 2, 9, 17, 1, 3]
    start = torch.tensor([0, 0, 1, 3, 12, 29, 30], dtype=torch.int64)
    length = torch.tensor(lens, dtype=torch.int32)
    idx = torch.tensor([RNG.randrange(n) for _ in range(33)], dtype=torch.int64)
    for i in (3, 20, 29, 31):
        idx[i] = i
    for ix in (None, idx):
        ref = nt.gt_slice_prod(src, ix, start, length)
        got = nt.gt_beta_slice_prod(beta, ix, start, length)
        assert torch.equal(nt.gt_pi(got), ref)
        assert torch.equal(got[0], nt.gt_one("cpu")[0])        # empty slice
        assert torch.equal(got[5], nt.gt_one("cpu")[0])        # the slice of one skipped row


# ----------------------------------------------------------------------------- multi_exp_device
def _me_inputs(gt_pool, m: int, G: int):
    """The verifier's entry layout: G blocks of 2m 32-bit exponents over
    (A, frob^8 A), then G blocks of m 40-bit exponents over A."""
    A = _with_ones(gt_pool[:m], [5])
    k = torch.zeros((3 * G * m, 8), dtype=torch.int64)
    k[: 2 * G * m, 0] = torch.tensor([RNG.randrange(1 << 32) for _ in range(2 * G * m)])
    gam = [RNG.randrange(1 << 40) for _ in range(G * m)]
    k[2 * G * m:, 0] = torch.tensor([g & 0xFFFFFFFF for g in gam])
    k[2 * G * m:, 1] = torch.tensor([g >> 32 for g in gam])
    k[7] = 0                                                                 # a zero exponent enters no bucket
    k = k.to(torch.int32)                                                    # limbs: the low 32 bits, as stored
    e = torch.arange(3 * G * m)
    grp = torch.where(e < 2 * G * m, e // (2 * m), G + (e - 2 * G * m) // m).to(torch.int32)
    groups = ((2 * m, 32),) * G + ((m, 40),) * G
    return A, k, grp, groups, (2 * G * m, m)


@pytest.mark.parametrize("W,c", [(8, 5), (3, 16)])
def test_multi_exp_device_on_images_matches_fp12(gt_pool, W, c):
    """(8, 5) fills every bucket with many entries, (3, 16) leaves most empty."""
    m, G = 37, 2
    A, k, grp, groups, split = _me_inputs(gt_pool, m, G)
    A2 = torch.cat([A, nt.gt_frob8(A)])
    h0 = nt.multi_exp_device(A2, k, grp, groups, W, c, item_split=split)
    h1 = nt.multi_exp_device(nt.gt_beta_rows(A), k, grp, groups, W, c, item_split=split)
    assert h1["torus"] and not h0["torus"]
    r0, r1 = nt.multi_exp_grouped_finish(h0), nt.multi_exp_grouped_finish(h1)
    nt.check_overflow(h0)
    nt.check_overflow(h1)
    assert torch.equal(r0, r1)


# ----------------------------------------------------------------------------- the verifier
@pytest.fixture(scope="module")
def proofs():
    S, u, l = 2, 4, 2
    sigs = [[rp.init_range_proof_signature(u) for _ in range(3)] for _ in range(S)]
    kps = [eg.KeyPair.generate() for _ in range(S)]
    P = eg.aggregate_keys([k.public for k in kps])
    sm = rp.SigMaterial(sigs)
    vals = [0, 13, 5]
    cv, r = eg.encrypt_ints(eg.pk_table(P), vals)
    n = len(vals)
    b = CreateProofBatch(vals, r, cv, [u] * n, [l] * n, [0, 1, 2], [0] * n)
    return rp.create_range_proofs(b, sm, P)[0], sm, P


def _raw_row(coeffs) -> torch.Tensor:
    return bn.to_tensor(bn.ints_to_limbs(coeffs).reshape(1, 96), "cpu")[0]


def _forge(A: torch.Tensor, row: int, how: str) -> torch.Tensor:
    A = A.clone()
    if how == "one":
        A[row] = nt.gt_one("cpu")[0]
    elif how == "minus_one":
        A[row] = _raw_row([bn.mont(O.P - 1)] + [0] * 11)
    elif how == "non_unitary":
        A[row, 0] ^= 1
    elif how == "non_canonical":                                  # the first coefficient plus p: same residue
        v = bn.limbs_to_ints(bn.to_numpy(A[row, :8].contiguous()).reshape(1, 8))[0]
        A[row, :8] = bn.to_tensor(bn.ints_to_limbs([v + O.P]), "cpu")[0]
    elif how == "non_canonical_zero_h":                           # g = 1, h = (p, 0, ..): a 0 with non-zero limbs
        A[row] = nt.gt_one("cpu")[0]
        A[row, 48:56] = bn.to_tensor(bn.ints_to_limbs([O.P]), "cpu")[0]
    else:
        raise AssertionError(how)
    return A


@pytest.mark.parametrize("how", ["clean", "one", "minus_one", "non_unitary", "non_canonical",
                                 "non_canonical_zero_h"])
def test_verdicts_equal_with_and_without_torus(proofs, how, monkeypatch):
    """3 proofs, S = 2, u = 4, l = 2, two VNs, whole and in two segments: the
    Fp12 path names segment 1 for a forged a_ij of proof 1, and the torus path
    gives the same verdicts."""
    rpl, sm, P = proofs
    dev = torch.device("cpu")
    r = rpl.to(dev)
    if how != "clean":
        r.A = _forge(r.A, 1 * r.S * r.l + 1, how)                 # proof 1 = the first of segment 1
    want_seg = [[True, True]] * 2 if how == "clean" else [[True, False]] * 2
    want_all = [how == "clean"] * 2
    got = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("DRYNX_ME_TORUS", flag)
        got[flag] = (rp.verify_range_proof_list_multi(r, sm, P, 2, dev),
                     rp.verify_range_proof_list_multi(r, sm, P, 2, dev, segs=[1, 2]))
    assert got["0"] == (want_all, want_seg)
    assert got["1"] == got["0"]
