"""Key-grouped U side of the range verifier (csrc/kernels/dx_rpmsm.hip,
proofs/range_proof.py ``_msm_queue(ygroup=...)``): proofs that answer the same
column pair the same G1 key, so one Miller loop per (VN, key) over
sum_p c_p U_p replaces one per (VN, proof, key).  The challenge split, the
signed joint table and the key-group combination against the pure-Python
oracle; the grouped pairing product against the per-item one; the verifier
with the grouped path forced against the ungrouped verdicts."""
import random

import pytest
import torch

from drynx_amd import native as nt
from drynx_amd.crypto import bn254 as bn
from drynx_amd.crypto import elgamal as eg
from drynx_amd.crypto import oracle as O
from drynx_amd.ops.encoding import CreateProofBatch
from drynx_amd.proofs import range_proof as rp

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
LAM = nt.GLV_LAMBDA


def _dev(name):
    if name == "cuda" and not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device(name)


def _g2_points(k, seed):
    rnd = random.Random(seed)
    return [O.g2_mul(rnd.randrange(1, O.R), O.G2_GEN) for _ in range(k)]


def _pos_k2(j):
    """A scalar whose GLV split has k2 > 0.  k2 = f2 B2 - f1 B1 with f1, f2 the
    fractional parts of c B2 / r and c B1 / r (csrc/bn254/glv_split.h; B1 ~ 2^127,
    B2 ~ 2^63), so a uniform c has k2 < 0 except with probability ~2^-63:
    these sit 2^-65 above a multiple of r / B2."""
    B2 = 0x89d3256894d213e3
    return ((j << 65) + 1) * O.R // (B2 << 65) + 1


def _raw_scalars(vals, dev):
    return bn.to_tensor(bn.ints_to_limbs(vals), dev)          # not reduced mod r


def _split_ints(vals, dev="cpu"):
    """-> [(k1, |k2|, k2 < 0)] of ``nt.glv_split`` as Python integers."""
    w = bn.to_numpy(nt.glv_split(_raw_scalars(vals, dev)).cpu()).astype(object)
    out = []
    for row in w:
        k1 = sum(int(row[i]) << (32 * i) for i in range(4))
        k2 = sum(int(row[4 + i]) << (32 * i) for i in range(4))
        out.append((k1, k2, int(row[8])))
    return out


@pytest.mark.parametrize("device", DEVICES)
def test_challenge_split(device):
    dev = _dev(device)
    rnd = random.Random(21)
    cs = [0, 1, O.R - 1, (1 << 256) - 1] + [rnd.getrandbits(256) for _ in range(64)] + [_pos_k2(1), _pos_k2(3)]
    signs = set()
    for c, (k1, k2, s) in zip(cs, _split_ints(cs, dev)):
        assert k1 < 1 << 128 and k2 < 1 << 128 and s in (0, 1), hex(c)
        assert (k1 + (-k2 if s else k2) * LAM - c) % O.R == 0, hex(c)
        if k2:
            signs.add(s)
    assert signs == {0, 1}                                    # both signs of k2 occur


@pytest.mark.parametrize("device", DEVICES)
def test_signed_joint_table(device):
    dev = _dev(device)
    pts = _g2_points(3, 31) + [None]                          # None = infinity row
    V = bn.g2_aff_tensor(pts + pts, dev)
    sign = torch.tensor([0] * 4 + [1] * 4, dtype=torch.int32, device=dev)
    T = bn.g2_points_from_aff(nt.g2_joint_table(V, sign).cpu())
    for i, Q in enumerate(pts + pts):
        lam = -LAM if i >= 4 else LAM
        for e in range(15):
            da, db = (e + 1) % 4, (e + 1) // 4
            want = None if Q is None else O.g2_mul((da + db * lam) % O.R, Q)
            assert T[i * 15 + e] == want, (i, da, db)
    plain = nt.g2_joint_table(V)
    assert torch.equal(nt.g2_joint_table(V, torch.zeros(8, dtype=torch.int32, device=dev)), plain)
    assert torch.equal(nt.g2_joint_table(V, sign)[: 4 * 15], plain[: 4 * 15])


def _group_tensors(groups, dev):
    idx = torch.tensor([q for g in groups for q in g], dtype=torch.int32, device=dev)
    ln = [len(g) for g in groups]
    start = torch.tensor([sum(ln[:k]) for k in range(len(ln))], dtype=torch.int64, device=dev)
    return idx, start, torch.tensor(ln, dtype=torch.int32, device=dev)


def _group_sums(dev, pts, cs, groups, G, nq, S, pad, pos=None, sp=None):
    """The native key-group combinations of the rows ``pts`` (G * nq affine G2
    points) with the per-proof scalars ``cs`` -> [G * pad, 32] rows."""
    U = bn.g2_aff_tensor(pts, dev)
    split = nt.glv_split(_raw_scalars(cs, dev))
    sgn = split[:, 8].repeat_interleave(S)[:nq].repeat(G).contiguous()
    idx, start, ln = _group_tensors(groups, dev)
    out = torch.zeros((G * pad, 32), dtype=torch.int32, device=dev)
    nt.rp_u_group(nt.g2_joint_table(U, sgn), split, idx, start, ln, G, nq, S, out, pad, pos, sp)
    return out


@pytest.mark.parametrize("device", DEVICES)
def test_key_group_combination(device):
    dev = _dev(device)
    G, S, n = 2, 2, 8
    nq = n * S
    rnd = random.Random(41)
    r254 = [rnd.randrange(1 << 253, O.R) for _ in range(4)]
    # scalar of proof p (rows q = 2p, 2p + 1): the edge values and a positive k2 among random 254-bit ones
    cs = [r254[0], 1, O.R - 1, r254[1], _pos_k2(1), r254[2], r254[3], 0]
    assert {s for (_, k2, s) in _split_ints(cs) if k2} == {0, 1}          # both signs of k2
    # sizes [1, 3, 2], an all-infinity group and a group of random scalars and c = 0 on real points;
    # rows 1, 6, 9, 13, 15 belong to no group
    groups = [[8], [2, 3, 7], [4, 5], [12, 10], [0, 14, 11]]
    ng = len(groups)
    pts = _g2_points(G * nq, 42)
    for v in range(G):
        pts[v * nq + 3] = pts[v * nq + 2]                     # two equal members (c = 1 each): a doubling
        pts[v * nq + 12] = pts[v * nq + 10] = None            # infinity members
    pts[5] = O.g2_neg(pts[4])                                 # VN 0: a member and its negative (c = r - 1 each)
    want = []
    for v in range(G):
        for g in groups:
            acc = None
            for q in g:
                if pts[v * nq + q] is not None:
                    acc = O.g2_add(acc, O.g2_mul(cs[q // S], pts[v * nq + q]))
            want.append(acc)
    assert want[2] is None and want[ng + 2] is not None       # the cancellation, and r - 1 on distinct points
    assert want[3] is None and want[ng + 3] is None           # the all-infinity group
    pad = ng + 2
    out = _group_sums(dev, pts, cs, groups, G, nq, S, pad)
    got = bn.g2_points_from_aff(out.cpu())
    for v in range(G):
        for g in range(ng):
            assert got[v * pad + g] == want[v * ng + g], (v, g)
        assert got[v * pad + ng] is None and got[v * pad + ng + 1] is None   # untouched rows stay infinity
    # an explicit row per (v, g): the same points, permuted
    perm = list(range(G * pad))
    random.Random(43).shuffle(perm)
    pos = torch.tensor(perm[: G * ng], dtype=torch.int64, device=dev)
    out2 = _group_sums(dev, pts, cs, groups, G, nq, S, pad, pos)
    assert torch.equal(out2.index_select(0, pos), out.view(G, pad, 32)[:, :ng].reshape(-1, 32))
    rest = torch.tensor(perm[G * ng:], dtype=torch.int64, device=dev)
    assert not bool(out2.index_select(0, rest).any())
    # several lanes per group (the host path: separate partials + reduction)
    assert torch.equal(_group_sums(dev, pts, cs, groups, G, nq, S, pad, sp=4), out)


@pytest.mark.gpu
def test_key_group_split_lanes_match_host():
    """Groups of 1 and 5 members over 4 lanes each (u_group_kernel's LDS
    reduction: empty and uneven lanes), ~50 groups per VN so several
    workgroups run, against the host path, bit for bit."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    G, S = 2, 2
    sizes = [1, 5] * 25
    nq = sum(sizes)
    rnd = random.Random(51)
    order = list(range(nq))
    rnd.shuffle(order)                                        # members are not contiguous
    groups, a = [], 0
    for k in sizes:
        groups.append(order[a: a + k])
        a += k
    base = _g2_points(7, 52)
    pts = [base[rnd.randrange(7)] for _ in range(G * nq)]     # repeated points: doubling cases in the sums
    cs = [0, 1, O.R - 1] + [rnd.randrange(O.R) for _ in range(nq // S - 3)]
    pad = len(groups) + 3
    outs = [_group_sums(torch.device(d), pts, cs, groups, G, nq, S, pad, sp=4).cpu() for d in ("cpu", "cuda")]
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(_group_sums(torch.device("cuda"), pts, cs, groups, G, nq, S, pad, sp=1).cpu(), outs[0])


@pytest.fixture(scope="module")
def proofs():
    S, u, l = 2, 4, 3
    sigs = [[rp.init_range_proof_signature(u) for _ in range(3)] for _ in range(S)]
    kps = [eg.KeyPair.generate() for _ in range(S)]
    P = eg.aggregate_keys([k.public for k in kps])
    sm = rp.SigMaterial(sigs)
    vals = [0, 17, 63, 5]
    cv, r = eg.encrypt_ints(eg.pk_table(P), vals)
    n = len(vals)
    b = CreateProofBatch(vals, r, cv, [u] * n, [l] * n, [0, 1, 2, 0], [0] * n)   # proofs 0 and 3 share their keys
    return rp.create_range_proofs(b, sm, P)[0], sm, P


def _force(monkeypatch):
    monkeypatch.setattr(rp, "_YGROUP_MIN_MULT", 1)


def _verify(*a, **k):
    return rp.verify_range_proof_list_multi(*a, ygroup=True, **k)   # host tensors drive the same plumbing


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("segs", [None, [1, 2, 1]])
def test_grouped_product_matches_per_item(device, proofs, segs, monkeypatch):
    """FE(F_grouped ML(B, R)) == FE(prod_seg useg ML(B, R)) for the same
    weights: useg from the on-demand per-item fold of the grouped queue and
    from the ungrouped queue."""
    dev = _dev(device)
    _force(monkeypatch)
    rpl, sm, _ = proofs
    r = rpl.to(dev)
    n, l, S = len(r), r.l, r.S
    m, G = n * S * l, 2
    y_idx = (torch.arange(S, device=dev).view(1, S) * sm.n_cols
             + torch.tensor(r.cols, device=dev).view(n, 1)).reshape(-1)
    Y = nt.g1_mul(sm.y_jac.to(dev).index_select(0, y_idx).contiguous(), rp._rep(r.challenge, S))
    ab, rho = nt.glv_weights(G * m, dev)
    it = torch.arange(m, device=dev)
    s_r = nt.fr_arith(nt.FR_MUL, rho, r.zphi.index_select(0, (it // (S * l)) * l + it % l).contiguous())
    S_R, hR = nt.g2_msm_device(r.V, s_r, m, ((m, 254),) * G, c=rp._r_window(m, G))
    fR, _ = rp._msm_r_miller(hR, S_R)
    kg = rp._key_groups(r.cols, S, sm.n_cols, dev)
    assert kg.ng == 6 and sorted(kg.len.tolist()) == [1, 1, 1, 1, 2, 2]
    yg = dict(groups=kg, challenge=r.challenge, y_jac=sm.y_jac.to(dev))
    q = rp._msm_queue(Y, r.V, ab, G, n, S, l, None, segs, ygroup=yg)
    k = len(segs) if segs else 1
    assert q.fold.sb == [0] and tuple(q.u_seg.shape) == (G, k) and bool(q.u_seg.all())
    Fg = rp._seg_products(q)                                  # the per-VN product only
    assert tuple(Fg.shape) == (G, 1, 96)
    useg = rp._useg_items(q)
    plain = rp._seg_products(rp._msm_queue(Y, r.V, ab, G, n, S, l, None, segs))
    assert tuple(useg.shape) == tuple(plain.shape) == (G, k, 96)
    for v in range(G):
        fe = [nt.final_exp(nt.gt_mul(nt.gt_prod(x[v].view(-1, 1, 96), chunk=4).view(1, 96), fR[v:v + 1]))
              for x in (Fg, useg, plain)]
        assert bool(nt.gt_eq(fe[0], fe[1]).all()) and bool(nt.gt_eq(fe[0], fe[2]).all()), v
        if k > 1:                                             # per segment: the ungrouped queue's GT element
            assert bool(nt.gt_eq(nt.final_exp(useg[v].contiguous()), nt.final_exp(plain[v].contiguous())).all()), v


def _counted(monkeypatch, mod, name):
    calls, orig = [], getattr(mod, name)
    monkeypatch.setattr(mod, name, lambda *a, **k: calls.append(1) or orig(*a, **k))
    return calls


@pytest.mark.parametrize("device", DEVICES)
def test_grouped_verifier_accepts_and_rejects(device, proofs, monkeypatch):
    dev = _dev(device)
    rpl, sm, P = proofs
    grouped = _counted(monkeypatch, nt, "rp_u_group")
    items = _counted(monkeypatch, rp, "_useg_items")
    # the default constant: 8 U rows per VN over 6 keys stay on the per-item path
    assert rp._YGROUP_MIN_MULT >= 2
    assert _verify(rpl.to(dev), sm, P, 2, dev) == [True] * 2
    assert not grouped
    _force(monkeypatch)
    assert rp.verify_range_proof_list_multi(rpl.to(dev), sm, P, 2, dev, ygroup=False) == [True] * 2
    assert not grouped
    assert _verify(rpl.to(dev), sm, P, 3, dev) == [True] * 3
    assert _verify(rpl.to(dev), sm, P, 2, dev, segs=[1, 2, 1]) == [[True] * 3] * 2
    assert len(grouped) == 2 and not items                    # a clean batch never pays the per-item fold
    bad = rpl.to(dev)
    V = bad.V.clone()
    V[4] = V[5]                                               # a valid G2 point, wrong item
    bad.V = V
    assert _verify(bad, sm, P, 2, dev) == [False] * 2
    assert len(grouped) == 3 and not items                    # no attribution asked: no per-segment products


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("field", ["V", "zr", "A", "A_off_gt"])
def test_grouped_segment_attribution(device, field, proofs, monkeypatch):
    """The four tamperings of test_rpmsm.py::test_segment_attribution: the
    grouped path's per-segment verdicts are those of the ungrouped path on
    the same input, and only a failing batch runs the per-item fold."""
    dev = _dev(device)
    rpl, sm, P = proofs
    bad = rpl.to(dev)
    n, l, S = len(bad), bad.l, bad.S
    if field == "V":
        V = bad.V.clone()
        V[2 * S * l] = V[2 * S * l + 1]
        bad.V = V
        want = [True, False, True]
    elif field == "zr":
        zr = bad.zr.clone()
        zr[3, 0] ^= 1
        bad.zr = zr
        want = [True, True, False]
    elif field == "A":
        A = bad.A.clone()
        A[1] = nt.gt_mul(A[1:2].contiguous(), A[1:2].contiguous())[0]
        bad.A = A
        want = [False, True, True]
    else:
        A = bad.A.clone()
        A[-1, -1] ^= 1
        bad.A = A
        want = [True, True, False]
    grouped = _counted(monkeypatch, nt, "rp_u_group")
    plain = _verify(bad, sm, P, 3, dev, segs=[1, 2, 1])       # the default constant: the per-item path
    assert plain == [want] * 3 and not grouped
    _force(monkeypatch)
    items = _counted(monkeypatch, rp, "_useg_items")
    assert _verify(bad, sm, P, 3, dev, segs=[1, 2, 1]) == plain
    # a proof that does not decode gets zero weights: the batch of the others passes
    assert len(grouped) == 1 and len(items) == (1 if field != "A_off_gt" else 0)
