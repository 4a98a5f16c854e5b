"""Bucket-plan multi-scalar products (drynx_amd/native/msm.py; csrc/kernels/
dx_plan.hip, dx_rpmsm.hip, dx_g1.hip, dx_me_torus.hip) at multi-lane shapes
and on exceptional points, against the pure-Python oracle.

Every input row is one of eight pool entries with a known discrete log (three
random multiples e of the generator, their negatives, -2 e_0 and infinity /
one), so the expected result of a group is ONE oracle multiplication by
sum k_t log_t mod r -- repeated points, P + P, P + (-P) and infinity operands
sit in every bucket, tree level, running sum and Horner step by construction,
and no expectation comes from the native library.

A  device-resident plans whose buckets own several lanes (tree passes,
   ``index_copy_`` of the multi-lane results, uneven and empty lanes);
B  bucket weights and Horner through infinity, P + (-P) and P + P;
C  digit extraction at the word and width edges, and the overflow report;
D  the counted plans on the same inputs;
E  the slice-sum and chunk-weight kernels directly.
"""
import random

import pytest
import torch

from test_rpmsm import DEVICES, _dev

from drynx_amd import native as nt
from drynx_amd.crypto import bn254 as bn
from drynx_amd.crypto import oracle as O
from drynx_amd.native import msm

Q, NQ, M2Q, INF = 0, 3, 6, 7      # pool slots: e_0 G, -e_0 G, -2 e_0 G, infinity; slots 1, 2, 4, 5: +-e_1 G, +-e_2 G
P1, P2 = 1, 2


# ----------------------------------------------------------------------------- pools with bookkept logs
def _logs(seed):
    rnd = random.Random(seed)
    e = [rnd.randrange(1, O.R) for _ in range(3)]
    return e + [O.R - x for x in e] + [(-2 * e[0]) % O.R, 0]


def _g1_of(s):
    return O.g1_mul(s, O.G1_GEN) if s % O.R else None


def _g2_of(s):
    return O.g2_mul(s, O.G2_GEN) if s % O.R else None


def _g1_jac_rows(points, zs):
    """Jacobian rows (x z^2, y z^3, z) of affine oracle points; None -> (1, 1, 0)."""
    c = []
    for p, z in zip(points, zs):
        c += [1, 1, 0] if p is None else [p[0] * z * z % O.P, p[1] * z * z * z % O.P, z]
    return bn.to_tensor(bn.fp_limbs_mont(c).reshape(-1, 24), "cpu")


def _g1_from_jac(t):
    v = [bn.unmont(x) for x in bn.limbs_to_ints(bn.to_numpy(t))]
    out = []
    for i in range(0, len(v), 3):
        x, y, z = v[i: i + 3]
        zi = O.inv_mod(z, O.P) if z else 0
        out.append((x * zi * zi % O.P, y * zi * zi * zi % O.P) if z else None)
    return out


def _g2_jac_rows(points, zs):
    c = []
    for p, z in zip(points, zs):
        if p is None:
            c += [1, 0, 1, 0, 0, 0]
        else:
            z2 = z * z
            x, y = p[0] * z2, p[1] * z2 * z
            c += [x.c0, x.c1, y.c0, y.c1, z.c0, z.c1]
    return bn.to_tensor(bn.fp_limbs_mont(c).reshape(-1, 48), "cpu")


def _g2_from_jac(t):
    v = [bn.unmont(x) for x in bn.limbs_to_ints(bn.to_numpy(t))]
    out = []
    for i in range(0, len(v), 6):
        x, y, z = O.Fp2(v[i], v[i + 1]), O.Fp2(v[i + 2], v[i + 3]), O.Fp2(v[i + 4], v[i + 5])
        if z.is_zero():
            out.append(None)
        else:
            zi = z.inv()
            out.append((x * zi * zi, y * zi * zi * zi))
    return out


class _Pool:
    """rows[i] (CPU tensor) encodes logs[i] times the generator."""

    def __init__(self, logs, rows, of):
        self.logs, self.rows, self.of = logs, rows, of

    def take(self, idx, dev):
        return self.rows.index_select(0, torch.tensor(idx, dtype=torch.int64)).contiguous().to(dev)

    def log(self, idx, ks, mult=1):
        return sum(k * self.logs[i] for i, k in zip(idx, ks)) * mult % O.R

    def want(self, idx, ks):
        return self.of(self.log(idx, ks))


@pytest.fixture(scope="module")
def g1_pool():
    """Jacobian G1 rows with Z = 1 (infinity: Z = 0); shared, never modified."""
    logs = _logs(101)
    return _Pool(logs, _g1_jac_rows([_g1_of(s) for s in logs], [1] * 8), _g1_of)


@pytest.fixture(scope="module")
def g2_pool():
    """Affine G2 rows (infinity: all zero); shared, never modified."""
    logs = _logs(102)
    return _Pool(logs, bn.g2_aff_tensor([_g2_of(s) for s in logs], "cpu"), _g2_of)


@pytest.fixture(scope="module")
def gt_pool():
    """Fp12 rows g^log, g = e(G1, G2); shared, never modified."""
    logs = _logs(103)
    g = O.pairing(O.G1_GEN, O.G2_GEN)
    pw = {s: g ** s for s in logs[:3] + logs[6:7]}
    vals = [pw[s] for s in logs[:3]] + [pw[s].inv() for s in logs[:3]] + [pw[logs[6]], O.Fp12.one()]
    assert vals[Q] * vals[NQ] == O.Fp12.one() and vals[M2Q] * vals[Q] * vals[Q] == O.Fp12.one()
    return _Pool(logs, bn.gt_tensor(vals, "cpu"), lambda s: g ** (s % O.R))


def _k(vals, dev):
    """Scalars as given (not reduced mod r) -> [n, 8] limbs."""
    return bn.to_tensor(bn.ints_to_limbs(vals), dev)


# ----------------------------------------------------------------------------- the groups of A and D
SCENARIOS = ("random", "skew", "zero", "same", "same_alt", "altneg", "halves", "sparse")


def _scenario(name, n, bits, s, rnd):
    """(pool slot per row, scalar per row) of one group of n (even) rows;
    ``s``: the group's one scalar where all are equal."""
    any_idx = [rnd.randrange(8) for _ in range(n)]
    if name == "random":       # repeated points in every bucket
        return any_idx, [rnd.randrange(1 << bits) for _ in range(n)]
    if name == "skew":         # one bucket per window; every other one is empty
        return any_idx, [s] * n
    if name == "zero":         # no entry at all
        return any_idx, [0] * n
    if name == "same":         # equal lane partials: the tree doubles
        return [Q] * n, [s] * n
    if name == "same_alt":
        return [Q] * n, [s, 0] * (n // 2)
    if name == "altneg":       # Q, -Q with pairwise equal scalars: cancels inside the first pass
        ks = [rnd.randrange(1, 1 << bits) for _ in range(n // 2)]
        return [Q, NQ] * (n // 2), [k for k in ks for _ in range(2)]
    if name == "halves":       # non-zero lane partials that cancel only in the tree
        return [Q] * (n // 2) + [NQ] * (n // 2), [s] * n
    if name == "sparse":       # runs shorter than their buckets' lane counts: lanes without an entry
        return any_idx, [s] * 5 + [0] * (n - 5)
    raise AssertionError(name)


def _tensor_device(dev):
    """The device as tensors name it (cuda -> cuda:0): what the plans key their layouts by."""
    return torch.empty(0, device=dev).device


def _assert_multilane(groups, W, c, sl, dev, lanes=9, passes=2):
    lay = msm._device_layout(tuple(groups), W, c, sl, _tensor_device(dev))
    assert int(lay["lanes"].max()) >= lanes and len(lay["passes"]) >= passes, \
        (int(lay["lanes"].max()), len(lay["passes"]))
    return lay


def _scalars_for(vkind, G, m, bits, s, rnd):
    """G2 plans read V[t % m] in every group, so one call has ONE row pattern
    ``vkind`` and its groups differ in their scalars only."""
    pattern = {"random": ("random", "skew", "zero"), "same": ("same", "same_alt", "sparse"),
               "altneg": ("altneg", "skew", "sparse"), "halves": ("halves", "random", "altneg")}[vkind]
    idx = _scenario(vkind, m, bits, s, rnd)[0]
    return idx, [_scenario(pattern[g % 3], m, bits, s, rnd)[1] for g in range(G)]


# ----------------------------------------------------------------------------- A. device plans, multi-lane buckets
G2_SHAPE = dict(m=1100, c=4, bits=6, s=0x2b)


def _g2_device(pool, dev, idx, ks, c, bits):
    m, G = len(idx), len(ks)
    V = pool.take(idx, dev)
    S, h = nt.g2_msm_device(V, _k([k for g in ks for k in g], dev), m, ((m, bits),) * G, c=c, bits=bits)
    out_dev = nt.g2_msm_finish(S, h).cpu()                    # Horner lanes where the tensor lives
    out_host = nt.g2_msm_finish(S.cpu(), h).cpu()             # and on the host
    nt.check_overflow(h)
    return bn.g2_points_from_aff(out_dev), bn.g2_points_from_aff(out_host), out_dev


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("vkind", ["random", "same", "altneg", "halves"])
def test_g2_device_plan_multilane(device, vkind, g2_pool):
    """1,100 rows, c = 4, bits = 6: the 2-bit top window's buckets own 9 lanes
    (two tree passes), the low window's 3."""
    dev = _dev(device)
    m, c, bits, s = (G2_SHAPE[x] for x in ("m", "c", "bits", "s"))
    G = 3
    _assert_multilane(((m, bits),) * G, -(-bits // c), c, 32, dev)
    idx, ks = _scalars_for(vkind, G, m, bits, s, random.Random(20 + len(vkind)))
    got_dev, got_host, raw = _g2_device(g2_pool, dev, idx, ks, c, bits)
    for g in range(G):
        want = g2_pool.want(idx, ks[g])
        assert got_dev[g] == want and got_host[g] == want, (vkind, g)
        if want is None:
            assert not raw[g].any()                            # infinity is the all-zero affine row
    if vkind in ("altneg", "halves"):
        assert got_dev[0] is None                              # the cancelling group itself


def _group_inputs(n, bits, s, rnd, order=SCENARIOS):
    """One group per scenario, each with rows of its own (G1 and GT plans read one row per entry)."""
    idx, ks = [], []
    for name in order:
        i, k = _scenario(name, n, bits, s, rnd)
        idx.append(i)
        ks.append(k)
    return idx, ks


def _g1_check(got_jac, pool, idx, ks, tag):
    got = bn.g1_points_from_jac(got_jac)
    for g in range(len(idx)):
        assert got[g] == pool.want(idx[g], ks[g]), (tag, g)


def _g1_device(pool, dev, idx, ks, bits):
    n, G = len(idx[0]), len(idx)
    P = pool.take([i for g in idx for i in g], dev)
    h = nt.g1_msm_device(P, _k([k for g in ks for k in g], dev), n, ((n, bits),) * G, bits=bits)
    got = nt.g1_msm_finish(h)
    nt.check_overflow(h)
    return got


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bits,s", [(2, 3), (10, 0x2a5)])
def test_g1_device_plan_multilane(device, bits, s, g1_pool):
    """300 rows per group: bits = 2 is one window of 3 buckets with 10 lanes
    each, bits = 10 a full window of single lanes under a partial top window
    of 10-lane buckets.  One group per scenario."""
    dev = _dev(device)
    n = 300
    _assert_multilane(((n, bits),) * len(SCENARIOS), (bits + 7) // 8, 8, msm._ME_SLICE, dev)
    idx, ks = _group_inputs(n, bits, s, random.Random(bits))
    got = _g1_device(g1_pool, dev, idx, ks, bits)
    _g1_check(got, g1_pool, idx, ks, bits)
    for g, name in enumerate(SCENARIOS):
        if name in ("zero", "altneg", "halves"):
            assert g1_pool.want(idx[g], ks[g]) is None and not got[g, 16:].any()     # Z = 0


GT_SHAPE = dict(n=300, W=2, c=2, bits=4, first_slice=8, s=0b0110)


def _gt_check(got, pool, logs, tag):
    got = bn.gt_from_tensor(got.cpu())
    for g, s in enumerate(logs):
        assert got[g] == pool.of(s), (tag, g)
        if s % O.R == 0:
            assert got[g].is_one()


def _gt_rows_device(pool, dev, idx, ks):
    n, G = len(idx[0]), len(idx)
    W, c, bits, fs = (GT_SHAPE[x] for x in ("W", "c", "bits", "first_slice"))
    a = pool.take([i for g in idx for i in g], dev)
    h = nt.multi_exp_device(a, _k([k for g in ks for k in g], dev), n, ((n, bits),) * G, W, c, first_slice=fs)
    got = nt.multi_exp_grouped_finish(h)
    nt.check_overflow(h)
    return got


@pytest.mark.parametrize("device", DEVICES)
def test_gt_device_plan_multilane_fp12_rows(device, gt_pool):
    """300 Fp12 rows per group, W = 2, c = 2, 8 entries per lane: 10 lanes per
    bucket.  ``altneg`` puts a and 1/a side by side in every slice; its
    product, ``zero``'s and ``halves``' are 1."""
    dev = _dev(device)
    n, W, c, bits, fs, s = (GT_SHAPE[x] for x in ("n", "W", "c", "bits", "first_slice", "s"))
    _assert_multilane(((n, bits),) * len(SCENARIOS), W, c, fs, dev)
    idx, ks = _group_inputs(n, bits, s, random.Random(31))
    got = _gt_rows_device(gt_pool, dev, idx, ks)
    _gt_check(got, gt_pool, [gt_pool.log(idx[g], ks[g]) for g in range(len(idx))], "fp12")


def _gt_torus_device(pool, dev, idx, k_lo, k_hi):
    """Group g: its n rows A_g with exponents k_lo[g], then frob^8 of the same
    rows (log times GLV_LAMBDA) with k_hi[g] -- entry i reads image row i of
    ``gt_beta_rows``, the group of entry i is (i mod N) // n."""
    n, G = len(idx[0]), len(idx)
    N = n * G
    W, c, bits, fs = (GT_SHAPE[x] for x in ("W", "c", "bits", "first_slice"))
    beta2 = nt.gt_beta_rows(pool.take([i for g in idx for i in g], dev))
    assert tuple(beta2.shape) == (2 * N, 48)
    k = _k([k for g in k_lo for k in g] + [k for g in k_hi for k in g], dev)
    grp = ((torch.arange(2 * N) % N) // n).to(torch.int32).to(dev)
    h = nt.multi_exp_device(beta2, k, grp, ((2 * n, bits),) * G, W, c, first_slice=fs)
    assert h["torus"]
    got = nt.multi_exp_grouped_finish(h)
    nt.check_overflow(h)
    return got


def _gt_torus_logs(pool, idx, k_lo, k_hi):
    return [(pool.log(idx[g], k_lo[g]) + pool.log(idx[g], k_hi[g], nt.GLV_LAMBDA)) % O.R for g in range(len(idx))]


@pytest.mark.parametrize("device", DEVICES)
def test_gt_device_plan_multilane_torus_images(device, gt_pool):
    """The same on torus images: 600 entries per group (the rows and their
    frob^8 images), 19 lanes per bucket; a next to 1/a leaves a numerator with
    D = 0 in mid-chain, rows of 1 are the all-zero skip rows."""
    dev = _dev(device)
    n, W, c, bits, fs, s = (GT_SHAPE[x] for x in ("n", "W", "c", "bits", "first_slice", "s"))
    _assert_multilane(((2 * n, bits),) * len(SCENARIOS), W, c, fs, dev, lanes=19)
    rnd = random.Random(32)
    idx, k_lo = _group_inputs(n, bits, s, rnd)
    k_hi = [_scenario(name, n, bits, s, rnd)[1] for name in SCENARIOS]
    got = _gt_torus_device(gt_pool, dev, idx, k_lo, k_hi)
    _gt_check(got, gt_pool, _gt_torus_logs(gt_pool, idx, k_lo, k_hi), "torus")


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("kind", ["g2", "g1", "gt", "gt_torus"])
def test_layout_cache_serves_second_call(device, kind, g1_pool, g2_pool, gt_pool):
    """The same shape twice with other data and another shape in between: the
    second call takes the cached layout and its cached weight plan."""
    dev = _dev(device)
    rnd = random.Random(41)
    order2 = SCENARIOS[3:] + SCENARIOS[:3]
    n, W, c, bits, fs, s = (GT_SHAPE[x] for x in ("n", "W", "c", "bits", "first_slice", "s"))
    if kind == "g2":
        m, c2, b2, s2 = (G2_SHAPE[x] for x in ("m", "c", "bits", "s"))
        key, wkey = (((m, b2),) * 3, -(-b2 // c2), c2, 32), msm.ChunkWeights

        def run(vkind, mm=m, cc=c2):
            idx, ks = _scalars_for(vkind, 3, mm, b2, s2, rnd)
            got = _g2_device(g2_pool, dev, idx, ks, cc, b2)[0]
            assert got == [g2_pool.want(idx, k) for k in ks], vkind

        first, between, second = (lambda: run("halves")), (lambda: run("random", 26, 3)), (lambda: run("random"))
    elif kind == "g1":
        key, wkey = (((n, 2),) * len(SCENARIOS), 1, 8, msm._ME_SLICE), msm.DigitWeights

        def run(order, b=2, sb=3):
            idx, ks = _group_inputs(n, b, sb, rnd, order)
            _g1_check(_g1_device(g1_pool, dev, idx, ks, b), g1_pool, idx, ks, order[0])

        first, between, second = (lambda: run(SCENARIOS)), (lambda: run(SCENARIOS, 10, 0x2a5)), (lambda: run(order2))
    elif kind == "gt":
        key, wkey = (((n, bits),) * len(SCENARIOS), W, c, fs), msm.ChunkWeights

        def run(order, nn=n):
            idx, ks = _group_inputs(nn, bits, s, rnd, order)
            _gt_check(_gt_rows_device(gt_pool, dev, idx, ks), gt_pool,
                      [gt_pool.log(i, k) for i, k in zip(idx, ks)], order[0])

        first, between, second = (lambda: run(SCENARIOS)), (lambda: run(SCENARIOS[:3], 34)), (lambda: run(order2))
    else:
        key, wkey = (((2 * n, bits),) * len(SCENARIOS), W, c, fs), msm.ChunkWeights

        def run(order, nn=n):
            idx, k_lo = _group_inputs(nn, bits, s, rnd, order)
            k_hi = [_scenario(name, nn, bits, s, rnd)[1] for name in order]
            _gt_check(_gt_torus_device(gt_pool, dev, idx, k_lo, k_hi), gt_pool,
                      _gt_torus_logs(gt_pool, idx, k_lo, k_hi), order[0])

        first, between, second = (lambda: run(SCENARIOS)), (lambda: run(SCENARIOS[:3], 34)), (lambda: run(order2))
    key = key + (str(_tensor_device(dev)), wkey)
    first()
    lay = msm._DPLANS[key]
    wp = lay.weights
    assert isinstance(wp, wkey)
    between()
    second()
    assert msm._DPLANS[key] is lay and lay.weights is wp


# ----------------------------------------------------------------------------- B. weights and Horner
# rows of V: Q, -2Q, Q, Q; one group per case (scalars of the four rows), logs in units of e_0
B_ROWS = [Q, M2Q, Q, Q]
B_CASES_G2 = [([0x07, 0x06, 0, 0], -5),       # chunk_weight_one: tot = Q + (Q - 2Q) passes through infinity
              ([0x10, 0x08, 0, 0], 0),        # Horner: 16 Q + (-16 Q)
              ([0x10, 0, 0x0f, 0x01], 32),    # Horner: the accumulator 16 Q meets the window sum 16 Q
              ([0x03, 0, 0x05, 0], 8),        # every window but the lowest is empty: the chain starts at infinity
              ([0, 0, 0, 0], 0)]
B_CASES_G1 = [([0x07, 0x06, 0, 0], -5),
              ([0x100, 0x80, 0, 0], 0),       # 256 Q + (-256 Q)
              ([0x100, 0, 0xff, 0x01], 512),  # 256 Q + 256 Q
              ([0x03, 0, 0x05, 0], 8),
              ([0, 0, 0, 0], 0)]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bits", [8, 16])
def test_g2_weights_and_horner_edges(device, bits, g2_pool):
    """c = 4; bits = 16 declares two more (empty) top windows."""
    dev = _dev(device)
    ks = [k for k, _ in B_CASES_G2]
    got_dev, got_host, raw = _g2_device(g2_pool, dev, B_ROWS, ks, 4, bits)
    for g, (k, mult) in enumerate(B_CASES_G2):
        assert g2_pool.log(B_ROWS, k) == mult * g2_pool.logs[Q] % O.R                # the table above is right
        want = _g2_of(mult * g2_pool.logs[Q])
        assert got_dev[g] == want and got_host[g] == want, g
        assert (want is None) == (not raw[g].any())


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bits", [16, 40])
def test_g1_weights_and_horner_edges(device, bits, g1_pool):
    dev = _dev(device)
    idx, ks = [B_ROWS] * len(B_CASES_G1), [k for k, _ in B_CASES_G1]
    got = bn.g1_points_from_jac(_g1_device(g1_pool, dev, idx, ks, bits))
    for g, (k, mult) in enumerate(B_CASES_G1):
        assert g1_pool.log(B_ROWS, k) == mult * g1_pool.logs[Q] % O.R
        assert got[g] == _g1_of(mult * g1_pool.logs[Q]), g


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("path", ["counted", "device", "device_torus"])
def test_gt_weights_and_horner_edges(device, bits, path, gt_pool):
    """The rows and exponents of the G2 cases, c = 4, five groups of four
    entries, through the counted plan, the device plan on Fp12 rows and the
    device plan on the rows' torus images: a chunk product that passes through
    one, windows that are all empty (bits = 16: two more on top) and a group
    with no entry."""
    dev = _dev(device)
    c, W, G = 4, bits // 4, len(B_CASES_G2)
    a = gt_pool.take(B_ROWS * G, dev)
    k = _k([x for ks, _ in B_CASES_G2 for x in ks], dev)
    if path == "counted":
        h = nt.multi_exp_grouped(a, k, 4, G, W, c)
    else:
        if path == "device_torus":
            a = nt.gt_beta_rows(a)[: 4 * G]                    # the images of the rows themselves, not of frob^8
        h = nt.multi_exp_device(a, k, 4, ((4, bits),) * G, W, c)
    assert h.torus == (path == "device_torus")
    got = nt.multi_exp_grouped_finish(h)
    nt.check_overflow(h)
    for ks, mult in B_CASES_G2:
        assert gt_pool.log(B_ROWS, ks) == mult * gt_pool.logs[Q] % O.R                # the table above is right
    _gt_check(got, gt_pool, [mult * gt_pool.logs[Q] for _, mult in B_CASES_G2], (path, bits))


# ----------------------------------------------------------------------------- C. digits at the word and width edges
# (2^13 - 1) << 247 is the last window's digit position: the 7 bits of it that fit the declared 254 (and the 8
# limbs) are bits 247 .. 253, read from word 7 at shift 23 with no word 8 behind it; 0x1FFF << 221 is window 17,
# whose digit crosses from word 6 into word 7
EDGE_SCALARS = [O.R - 1, 2 ** 254 - 1, 2 ** 253, 2 ** 13 - 1, 2 ** 13, ((2 ** 13 - 1) << 247) & (2 ** 254 - 1), 0, 1,
                0x1FFF << 26, 0x1FFF << 221]
EDGE_ROWS = [Q, P1, P2, NQ, 4, 5, M2Q, P1, P2, 5]


@pytest.mark.parametrize("device", DEVICES)
def test_g2_digits_at_word_and_width_edges(device, g2_pool):
    """c = 13, bits = 254: 20 windows, the last one 7 bits wide and ending in
    word 7; digits that straddle a 32-bit word; a non-canonical scalar inside
    the declared width.  The device plan and the counted plan."""
    dev = _dev(device)
    want = g2_pool.want(EDGE_ROWS, EDGE_SCALARS)
    got_dev, got_host, _ = _g2_device(g2_pool, dev, EDGE_ROWS, [EDGE_SCALARS], 13, 254)
    assert got_dev == [want] and got_host == [want]
    V = g2_pool.take(EDGE_ROWS, dev)
    h = nt.g2_msm_launch(V, _k(EDGE_SCALARS, dev), None, 1, c=13, bits=254)
    assert bn.g2_points_from_aff(nt.g2_msm_finish(nt.g2_msm_run(V, h), h).cpu()) == [want]


@pytest.mark.parametrize("device", DEVICES)
def test_g1_digits_at_word_and_width_edges(device, g1_pool):
    dev = _dev(device)
    want = g1_pool.want(EDGE_ROWS, EDGE_SCALARS)
    assert bn.g1_points_from_jac(_g1_device(g1_pool, dev, [EDGE_ROWS], [EDGE_SCALARS], 254)) == [want]
    P = g1_pool.take(EDGE_ROWS, dev)
    assert bn.g1_points_from_jac(nt.g1_msm_grouped(P, _k(EDGE_SCALARS, dev), None, 1, 254)) == [want]


@pytest.mark.parametrize("device", DEVICES)
def test_g1_g2_overflow_is_reported(device, g1_pool, g2_pool):
    """A scalar one bit wider than declared raises in ``check_overflow``; the
    widest scalar inside the width does not."""
    dev = _dev(device)
    rows = [Q, P1, P2, NQ]
    for wide in (False, True):
        k6 = [5, 63, 1, (64 if wide else 63)]
        S, h = nt.g2_msm_device(g2_pool.take(rows, dev), _k(k6, dev), 4, ((4, 6),), c=4, bits=6)
        got = bn.g2_points_from_aff(nt.g2_msm_finish(S, h).cpu())
        k10 = [5, 1023, (1024 if wide else 1023), 1]
        h1 = nt.g1_msm_device(g1_pool.take(rows, dev), _k(k10, dev), 4, ((4, 10),), bits=10)
        got1 = bn.g1_points_from_jac(nt.g1_msm_finish(h1))
        for hh in (h, h1):
            if wide:
                with pytest.raises(RuntimeError, match="declared scalar widths"):
                    nt.check_overflow(hh)
            else:
                nt.check_overflow(hh)
        if not wide:
            assert got == [g2_pool.want(rows, k6)] and got1 == [g1_pool.want(rows, k10)]


# ----------------------------------------------------------------------------- D. counted plans
def _group_arg(mode, G, n, dev):
    """-> (group argument, n_groups, result row of group g).  ``tensor``: an
    explicit group per entry that leaves group 1 without any entry."""
    if mode == "stride":
        return n, G, list(range(G))
    ids = [0] + list(range(2, G + 1))
    return torch.tensor(ids, dtype=torch.int32).repeat_interleave(n).to(dev), G + 1, ids


D_SCENARIOS = ("altneg", "halves", "same", "same_alt", "skew")


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("mode", ["tensor", "stride"])
@pytest.mark.parametrize("vkind", ["same", "altneg", "halves", "B"])
def test_g2_counted_plan_edges(device, mode, vkind, g2_pool):
    """``g2_msm_launch`` / ``g2_msm_run`` (the segment pass: first_slice = 32)
    on the groups of A at 1,100 rows and on the cases of B."""
    dev = _dev(device)
    if vkind == "B":
        idx, ks, c, bits = B_ROWS, [k for k, _ in B_CASES_G2], 4, 8
    else:
        m, c, bits, s = (G2_SHAPE[x] for x in ("m", "c", "bits", "s"))
        idx, ks = _scalars_for(vkind, 3, m, bits, s, random.Random(51))
    G, m = len(ks), len(idx)
    grp, n_groups, row = _group_arg(mode, G, m, dev)
    V = g2_pool.take(idx, dev)
    h = nt.g2_msm_launch(V, _k([k for g in ks for k in g], dev), grp, n_groups, c=c, bits=bits, first_slice=32)
    S = nt.g2_msm_run(V, h)
    for out in (nt.g2_msm_finish(S, h).cpu(), nt.g2_msm_finish(S.cpu(), h).cpu()):
        got = bn.g2_points_from_aff(out)
        assert len(got) == n_groups
        for g in range(G):
            assert got[row[g]] == g2_pool.want(idx, ks[g]), (vkind, g)
        if mode == "tensor":
            assert got[1] is None and not out[1].any()          # the group without an entry


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("mode", ["tensor", "stride"])
def test_g1_counted_plan_edges(device, mode, g1_pool):
    dev = _dev(device)
    for tag, bits, (idx, ks) in (
            ("A", 10, _group_inputs(300, 10, 0x2a5, random.Random(52), D_SCENARIOS)),
            ("B", 16, ([B_ROWS] * len(B_CASES_G1), [k for k, _ in B_CASES_G1]))):
        G, n = len(idx), len(idx[0])
        grp, n_groups, row = _group_arg(mode, G, n, dev)
        P = g1_pool.take([i for g in idx for i in g], dev)
        out = nt.g1_msm_grouped(P, _k([k for g in ks for k in g], dev), grp, n_groups, bits)
        got = bn.g1_points_from_jac(out)
        assert len(got) == n_groups
        for g in range(G):
            assert got[row[g]] == g1_pool.want(idx[g], ks[g]), (tag, g)
        if mode == "tensor":
            assert got[1] is None


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("mode", ["tensor", "stride"])
def test_gt_counted_plan_edges(device, mode, gt_pool):
    """``multi_exp_grouped`` (Fp12 rows: the counted plan takes no torus images)."""
    dev = _dev(device)
    n, W, c, bits, s = (GT_SHAPE[x] for x in ("n", "W", "c", "bits", "s"))
    idx, ks = _group_inputs(n, bits, s, random.Random(53), D_SCENARIOS)
    G = len(idx)
    grp, n_groups, row = _group_arg(mode, G, n, dev)
    a = gt_pool.take([i for g in idx for i in g], dev)
    h = nt.multi_exp_grouped(a, _k([k for g in ks for k in g], dev), grp, n_groups, W, c)
    got = bn.gt_from_tensor(nt.multi_exp_grouped_finish(h).cpu())
    assert len(got) == n_groups
    for g in range(G):
        assert got[row[g]] == gt_pool.of(gt_pool.log(idx[g], ks[g])), g
    if mode == "tensor":
        assert got[1].is_one()


# ----------------------------------------------------------------------------- E. the kernels directly
SLICES = [[], [Q], [Q, Q], [Q, NQ, Q], [INF, Q, INF], [Q, Q, Q, Q], [Q] * 17,
          [Q, Q, M2Q], [P1, NQ, Q, 4], [INF], [P1, P2, 5, Q, NQ, P1, P1, M2Q, Q, Q]]


def _slice_args(dev):
    flat = [i for sl in SLICES for i in sl]
    lens = [len(sl) for sl in SLICES]
    start = [sum(lens[:i]) for i in range(len(lens))]
    return flat, torch.tensor(start, dtype=torch.int64, device=dev), torch.tensor(lens, dtype=torch.int32, device=dev)


def _assert_slices(got, pool, tag):
    for i, sl in enumerate(SLICES):
        assert got[i] == pool.want(sl, [1] * len(sl)), (tag, i, sl)


@pytest.mark.parametrize("device", DEVICES)
def test_g2_slice_sum_affine_edges(device, g2_pool):
    """Mixed additions through the item index, with and without ``idx_mod``."""
    dev = _dev(device)
    flat, start, length = _slice_args(dev)
    src = g2_pool.rows.to(dev)
    idx = torch.tensor(flat, dtype=torch.int32, device=dev)
    _assert_slices(_g2_from_jac(nt.g2_slice_sum(src, idx, start, length, True)), g2_pool, "idx")
    idx8 = torch.tensor([i + 8 * (t % 5) for t, i in enumerate(flat)], dtype=torch.int32, device=dev)
    _assert_slices(_g2_from_jac(nt.g2_slice_sum(src, idx8, start, length, True, 8)), g2_pool, "idx_mod")
    gathered = g2_pool.take(flat, dev)
    _assert_slices(_g2_from_jac(nt.g2_slice_sum(gathered, None, start, length, True)), g2_pool, "contiguous")


def _fp2_z(rnd):
    return O.Fp2(rnd.randrange(1, O.P), rnd.randrange(O.P))


@pytest.mark.parametrize("device", DEVICES)
def test_g2_slice_sum_jacobian_edges(device, g2_pool):
    """Jacobian rows in which every occurrence of a point has a Z of its own:
    P + P and P + (-P) are recognised across representations."""
    dev = _dev(device)
    flat, start, length = _slice_args(dev)
    rnd = random.Random(61)
    pts = [_g2_of(s) for s in g2_pool.logs]
    src = _g2_jac_rows([pts[i] for i in flat], [_fp2_z(rnd) for _ in flat]).to(dev)
    _assert_slices(_g2_from_jac(nt.g2_slice_sum(src, None, start, length, False)), g2_pool, "jac")
    pool_rows = _g2_jac_rows(pts, [O.Fp2(1, 0)] * 8).to(dev)
    idx = torch.tensor(flat, dtype=torch.int32, device=dev)
    _assert_slices(_g2_from_jac(nt.g2_slice_sum(pool_rows, idx, start, length, False)), g2_pool, "jac idx")


@pytest.mark.parametrize("device", DEVICES)
def test_g1_slice_sum_edges(device, g1_pool):
    dev = _dev(device)
    flat, start, length = _slice_args(dev)
    rnd = random.Random(62)
    pts = [_g1_of(s) for s in g1_pool.logs]
    src = _g1_jac_rows([pts[i] for i in flat], [rnd.randrange(1, O.P) for _ in flat]).to(dev)
    _assert_slices(_g1_from_jac(nt.g1_slice_sum(src, None, start, length)), g1_pool, "jac")
    idx = torch.tensor(flat, dtype=torch.int64, device=dev)
    _assert_slices(_g1_from_jac(nt.g1_slice_sum(g1_pool.rows.to(dev), idx, start, length)), g1_pool, "jac idx")


# (base, [(digit, pool slot), ...]) per chunk, digits ascending inside [base, base + chunk length)
CHUNKS = [(4, [(4, P1), (5, INF), (6, Q), (7, Q)]),            # an infinity bucket, equal buckets at adjacent digits
          (0, [(1, Q), (2, Q), (3, NQ)]),                      # acc and tot both pass through infinity
          (0, [(1, P1), (3, P2)]),                             # a digit without a bucket
          (0, [(2, INF)]),
          (32, [(32, Q), (40, P1), (63, Q)]),                  # a base of one bit
          (12, [(12, P2), (13, Q), (15, NQ)]),                 # a base with two bits set
          (12, [(12, Q)]),                                     # only the base * acc term
          (1, [(2, Q)]),                                       # tot == base * acc: the last addition doubles
          (8, [(9, Q), (10, NQ)]),                             # acc = infinity times the base
          (16, [(16 + i, (Q, P1, INF, NQ)[i % 4]) for i in range(16)])]


@pytest.mark.parametrize("device", DEVICES)
def test_g2_chunk_weight_edges(device, g2_pool):
    dev = _dev(device)
    rnd = random.Random(63)
    pts = [_g2_of(s) for s in g2_pool.logs]
    flat = [(d, slot) for _, ch in CHUNKS for d, slot in ch]
    lens = [len(ch) for _, ch in CHUNKS]
    B = _g2_jac_rows([pts[slot] for _, slot in flat], [_fp2_z(rnd) for _ in flat]).to(dev)
    d = torch.tensor([x for x, _ in flat], dtype=torch.int32, device=dev)
    start = torch.tensor([sum(lens[:i]) for i in range(len(lens))], dtype=torch.int64, device=dev)
    length = torch.tensor(lens, dtype=torch.int32, device=dev)
    base = torch.tensor([b for b, _ in CHUNKS], dtype=torch.int32, device=dev)
    got = _g2_from_jac(nt.g2_chunk_weight(B, d, start, length, base))
    for i, (b, ch) in enumerate(CHUNKS):
        assert got[i] == g2_pool.want([slot for _, slot in ch], [x for x, _ in ch]), (i, b, ch)
