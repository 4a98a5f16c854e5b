"""The range verifier's GT multi-exponentiation alone at the 1-GPU query's
shape (m = 993,600 items, G = 3 VNs: 2 G m 32-bit GLV halves over
(A, frob^8 A) and G m 40-bit membership coins over A), on Fp12 rows and on
torus images (csrc/kernels/dx_me_torus.hip), alone on the chip (device events,
median of 3 after one warm-up): the input pass (stacking A with its Frobenius
image / the image rows), the multi-exponentiation's device passes, and the
torus first pass with 8, 16 and 32 entries per lane pair.  The two paths' results
are compared bit for bit.  The numbers behind ``range_proof._ME_TORUS_DEFAULT``
and ``msm._ME_TORUS_SLICE`` (profiles/me_torus/README.md).

Usage: python tools/me_torus_bench.py [out.json]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drynx_amd import native as nt  # noqa: E402
from drynx_amd.crypto import bn254 as bn  # noqa: E402
from drynx_amd.crypto import oracle as O  # noqa: E402
from drynx_amd.proofs import range_proof as rp  # noqa: E402

assert torch.cuda.is_available(), "needs a GPU"
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
G, m, gb = 3, 993600, 40
gen = torch.Generator().manual_seed(1)
SLICES = (8, 16, 32)  # entries per lane pair in the torus first pass


def timed(fn, reps=3):
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
    return round(float(np.median(ts)), 3), [round(t, 3) for t in ts]


# m unitary rows: 64-bit powers of four random GT elements
g = O.pairing(O.G1_GEN, O.G2_GEN)
base = bn.gt_tensor([g ** (1 + 7919 * i) for i in range(4)], dev)
sc = torch.zeros((m, 8), dtype=torch.int64)
sc[:, :2] = torch.randint(0, 1 << 32, (m, 2), generator=gen)
A = nt.gt_pow(base.repeat(m // 4, 1).contiguous(), sc.to(torch.int32).to(dev))
k = torch.zeros((3 * G * m, 8), dtype=torch.int64)
k[:, 0] = torch.randint(0, 1 << 32, (3 * G * m,), generator=gen)
k[2 * G * m:, 1] = torch.randint(0, 1 << (gb - 32), (G * m,), generator=gen)
k = k.to(torch.int32).to(dev)
e = torch.arange(3 * G * m, device=dev)
grp = torch.where(e < 2 * G * m, e // (2 * m), G + (e - 2 * G * m) // m).to(torch.int32)
groups = ((2 * m, 32),) * G + ((m, gb),) * G
W, c = nt.me_window(groups)
split = (2 * G * m, m)
torch.cuda.synchronize()

res = {"m": m, "G": G, "window": [W, c]}
res["input_fp12_ms"] = timed(lambda: rp._stack_frob8(A))
res["input_torus_ms"] = timed(lambda: nt.gt_beta_rows(A))
A2, beta2 = rp._stack_frob8(A), nt.gt_beta_rows(A)
res["me_fp12_ms"] = timed(lambda: nt.multi_exp_device(A2, k, grp, groups, W, c, item_split=split))
print(json.dumps(res), flush=True)
for sl in SLICES:
    res[f"me_torus_slice{sl}_ms"] = timed(
        lambda: nt.multi_exp_device(beta2, k, grp, groups, W, c, item_split=split, first_slice=sl))
ref = nt.multi_exp_grouped_finish(nt.multi_exp_device(A2, k, grp, groups, W, c, item_split=split))
res["bit_equal"] = {}
for sl in SLICES:
    h = nt.multi_exp_device(beta2, k, grp, groups, W, c, item_split=split, first_slice=sl)
    res["bit_equal"][f"slice{sl}"] = bool(torch.equal(nt.multi_exp_grouped_finish(h), ref))
    nt.check_overflow(h)
print(json.dumps(res), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
