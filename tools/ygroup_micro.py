"""Kernel-level times of the range verifier's key-grouped U side at the 1-GPU
query's size (3 VNs x 62,100 U rows), each step alone on the chip (device
events, median): the signed joint table, the key-group combination per lane
count, the fold over nq pairs (per-item path) and over nq / mu keys for
several multiplicities mu, and the one-ladder-per-U variant (singleton groups,
then ``g2_slice_sum`` over the members).  The numbers behind
``range_proof._YGROUP_MIN_MULT`` and ``native.rp_u_group_lanes``
(profiles/ygroup/README.md).

Usage: python tools/ygroup_micro.py [out.json]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drynx_amd import native as nt  # noqa: E402
from drynx_amd.crypto import bn254 as bn  # noqa: E402
from drynx_amd.crypto import oracle as O  # noqa: E402
from drynx_amd.native import msm  # noqa: E402
from drynx_amd.proofs import range_proof as rp  # noqa: E402

assert torch.cuda.is_available(), "needs a GPU"
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
G, n, S = 3, 20700, 3
nq = n * S
gen = torch.Generator().manual_seed(1)


def rand_scalars(k):
    t = torch.randint(-2 ** 31, 2 ** 31 - 1, (k, 8), generator=gen, dtype=torch.int64).to(torch.int32)
    t[:, 7] &= 0x0fffffff
    return t.to(dev)


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return round(float(np.median(ts)), 3)


res = {}
tab = nt.g2_fb_table(bn.g2_aff_tensor([O.G2_GEN], dev))
U = nt.g2_fb_mul(tab, rand_scalars(G * nq))
Yall = nt.g1_fb_mul(bn.base_table(dev), rand_scalars(nq))
split = nt.glv_split(rand_scalars(n))
sgn = split[:, 8].repeat_interleave(S).repeat(G).contiguous()
torch.cuda.synchronize()
res["t_table"] = timed(lambda: nt.g2_joint_table(U, sgn))
tU = nt.g2_joint_table(U, sgn)


def fold(rows_U, Y, npairs):
    lay = rp._fold_layout(G, npairs, np.array([npairs]), dev)
    Ul = torch.zeros((G * lay.pad, 32), dtype=torch.int32, device=dev)
    Ul.view(G, lay.pad, 32)[:, :npairs] = rows_U.view(G, -1, 32)[:, :npairs]
    return timed(lambda: rp._fold_items(lay, Ul, Y, G, npairs)), lay.K, lay.coop


res["t_fold_items"], res["K_items"], _ = fold(U, Yall, nq)
print(json.dumps(res), flush=True)
for mu in (10, 5, 4, 3, 2):
    ng = nq // mu
    perm = np.random.RandomState(mu).permutation(nq).astype(np.int32)
    ln = np.full(ng, mu, dtype=np.int32)
    ln[-1] += nq - ng * mu
    idx = bn.h2d(torch.from_numpy(perm), dev)
    start = bn.h2d(torch.from_numpy((np.cumsum(ln) - ln).astype(np.int64)), dev)
    length = bn.h2d(torch.from_numpy(ln), dev)
    out = torch.zeros((G * (ng + 1), 32), dtype=torch.int32, device=dev)
    r = {}
    for sp in ((1, 2, 4, 8, 16) if mu == 10 else (1, 2, 4)):
        r[f"sp{sp}"] = timed(lambda: nt.rp_u_group(tU, split, idx, start, length, G, nq, S, out, ng + 1, None, sp), 3)
    r["auto_sp"] = nt.rp_u_group_lanes(G * ng, True)
    r["t_fold_groups"], r["K_groups"], r["coop"] = fold(out, Yall[:ng].contiguous(), ng)
    res[f"mu{mu}"] = r
    print(json.dumps({f"mu{mu}": r}), flush=True)
# the one-ladder-per-U variant: singleton groups, then the slice sum over the members
mu, ng = 10, nq // 10
one = bn.h2d(torch.ones(nq, dtype=torch.int32), dev)
ident = bn.h2d(torch.arange(nq, dtype=torch.int32), dev)
st1 = bn.h2d(torch.arange(nq, dtype=torch.int64), dev)
cU = torch.zeros((G * nq, 32), dtype=torch.int32, device=dev)
res["simple_ladders"] = timed(lambda: nt.rp_u_group(tU, split, ident, st1, one, G, nq, S, cU, nq, None, 1), 3)
perm = np.random.RandomState(10).permutation(nq).astype(np.int64)
midx = (np.arange(G).reshape(G, 1) * nq + perm.reshape(1, nq)).reshape(-1).astype(np.int32)
mst = (np.arange(G * ng) * mu).astype(np.int64)
mi, ms = bn.h2d(torch.from_numpy(midx), dev), bn.h2d(torch.from_numpy(mst), dev)
ml = bn.h2d(torch.full((G * ng,), mu, dtype=torch.int32), dev)
res["simple_slice_sum"] = timed(lambda: msm.g2_slice_sum(cU, mi, ms, ml, True), 3)
print(json.dumps(res), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
