#!/usr/bin/env python3
"""Microbenchmark + check of the verifier's U-side Miller folds on one GPU:
the coefficient images (raw and normalised), the one-lane K-item accumulation
over the normalised image and the three-lane accumulation over the raw one.
Each fold is first checked against per-item Miller loops on a 4096-item
prefix.  Prints one JSON line per section with ms and Miller loops/s.

Usage: python tools/fold_bench.py [items]   (FOLD_G: verifiers sharing the image)"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drynx_amd import native as nt  # noqa: E402
from drynx_amd.crypto import bn254 as bn  # noqa: E402


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best, out


def padded(P, n, rows, G, dev):
    """G copies of the n points, each padded to a whole number of rows * FOLD_P_ALIGN items."""
    per = rows * nt.FOLD_P_ALIGN
    pad = -(-n // per) * per
    PG = torch.zeros((G * pad, 16), dtype=torch.int32, device=dev)
    for g in range(G):
        PG[g * pad: g * pad + n] = P[:n]
    return PG, pad


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 993_600
    G = int(os.environ.get("FOLD_G", "3"))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    P = nt.g1_to_affine(nt.g1_fb_mul(bn.base_table(dev), bn.random_scalars(n, dev)))
    V = nt.g2_fb_mul(bn.base2_table(dev), bn.random_scalars(n, dev))
    # reference value on a small prefix: FE(prod ML) via per-item Miller loops
    m = min(n, 4096)
    Vm = V[:m].contiguous()
    ref = nt.final_exp(nt._finish_prod_on_host(nt.miller_loop(P[:m].contiguous(), Vm)))

    def check(fb, what):
        got = nt.final_exp(nt._finish_prod_on_host(fb))
        assert bool(nt.gt_eq(got, ref).all()), what

    img = nt.rp_fold_ncoeffs(Vm)
    for K in (1, 2, 4, 8):
        PG, pad = padded(P, m, 64 * K, 1, dev)
        check(nt.rp_fold_accum_n(img, nt.g1_aff_to_uv_(PG), Vm, pad, 1, K), ("normalised", K))
    PG, pad = padded(P, m, 64, 1, dev)
    check(nt.rp_fold_accum_coop_raw(nt.rp_fold_coeffs(Vm), PG, Vm, pad, 1), "coop")
    del img, PG
    print(json.dumps({"check": "ok", "items": m}), flush=True)

    # raw coefficients + three lanes per item (the pool-slice path)
    tc, coef = timed(lambda: nt.rp_fold_coeffs(V))
    PG, pad = padded(P, n, 64, G, dev)
    ta, _ = timed(lambda: nt.rp_fold_accum_coop_raw(coef, PG, V, pad, G))
    print(json.dumps({"fold": "coop-raw", "G": G, "n": n, "coeffs_ms": round(1e3 * tc, 2),
                      "accum_ms": round(1e3 * ta, 2), "ml_per_s": round(G * n / (tc + ta))}), flush=True)
    del coef, PG
    torch.cuda.empty_cache()
    # normalised lines: (c1/c0, c3/c0) per V, (x/y, 1/y) per point, K items per lane
    tn, img = timed(lambda: nt.rp_fold_ncoeffs(V))
    for K in (1, 2, 4, 8):
        PG, pad = padded(P, n, 64 * K, G, dev)
        UV = nt.g1_aff_to_uv_(PG)
        ta, _ = timed(lambda: nt.rp_fold_accum_n(img, UV, V, pad, G, K))
        print(json.dumps({"fold": "normalised", "G": G, "K": K, "n": n, "coeffs_ms": round(1e3 * tn, 2),
                          "accum_ms": round(1e3 * ta, 2), "ml_per_s": round(G * n / (tn + ta))}), flush=True)
        del PG, UV


if __name__ == "__main__":
    main()
