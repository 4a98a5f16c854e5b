"""Time the fused logistic-regression encoder (csrc/kernels/dx_lr.hip) on the GPU.

One DP of N records and d features through ``native.lr_encode_many`` (encoder
launches + the reduction), timed with device events: warm-up, then the median
and the spread of ``--runs`` runs.  ``--torch`` also times the only
alternative on the same box: torch fp64 standardise + augment +
``Xa.T @ (Xa * w)`` and the level-1 ``Xa.T @ g``.  Next to the times it prints
what the algorithm needs, computed from the shapes: the bytes of X, y and of
the partial slab (written once, read once), and 2 N P^2 fp64 flop, as rates
against the chip's limits (HBM 8.0 TB/s spec / ~6.3 TB/s achievable, fp64
matrix 78.6 TFLOP/s spec).

Usage: python tools/bench_lr_encode.py --n 100000 --d 100 --torch [--json-out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drynx_amd import native as nt  # noqa: E402

HBM_SPEC, HBM_ACHIEVABLE, FP64_MATRIX_SPEC = 8.0e12, 6.3e12, 78.6e12


def time_ms(fn, warmup: int, runs: int) -> list:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def summary(ms: list) -> dict:
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "p10_ms": s[len(s) // 10],
            "p90_ms": s[(len(s) * 9) // 10], "max_ms": s[-1], "runs": len(s)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--d", type=int, default=100)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--torch", action="store_true", help="also time the torch fp64 path")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_lr_encode needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    N, d = a.n, a.d
    X = torch.rand(N, d, dtype=torch.float64, device=dev, generator=g) * 4
    y = torch.randint(0, 2, (N,), device=dev, generator=g)
    yf = y.to(torch.float64)
    m, s = X.mean(0), X.std(0, unbiased=False)
    tot = nt.lr_encode_many([X], [yf], m, s, 0.0, -1.0)
    P, D = tot.shape[1], d + 1
    nb = nt._lr_blocks(N)
    need_bytes = 8 * (N * d + N) + 2 * 8 * nb * P * P
    flop = 2 * N * P * P
    res = {"N": N, "d": d, "P": P, "record_blocks": nb, "x_bytes": 8 * N * d, "partial_bytes": 8 * nb * P * P,
           "needed_bytes": need_bytes, "flop": flop}
    k = summary(time_ms(lambda: nt.lr_encode_many([X], [yf], m, s, 0.0, -1.0), a.warmup, a.runs))
    t = k["median_ms"] * 1e-3
    k.update({"bytes_per_s": need_bytes / t, "flop_per_s": flop / t, "share_of_hbm_spec": need_bytes / t / HBM_SPEC,
              "share_of_hbm_achievable": need_bytes / t / HBM_ACHIEVABLE,
              "share_of_fp64_matrix_spec": flop / t / FP64_MATRIX_SPEC})
    res["lr_encode"] = k
    if a.torch:
        def ref():
            Xa = torch.cat([torch.ones((N, 1), dtype=torch.float64, device=dev), (X - m) / s], dim=1)
            w = 0.0 * yf - 1.0
            return Xa.T @ (2 * yf - 1), Xa.T @ (Xa * w[:, None])

        r1, r2 = ref()
        res["max_abs_diff_vs_torch"] = max(float((tot[0, D, :D] - r1).abs().max()),
                                           float((tot[0, :D, :D] - r2).abs().max()))
        res["torch_fp64"] = summary(time_ms(ref, a.warmup, a.runs))
        res["torch_over_kernel"] = res["torch_fp64"]["median_ms"] / k["median_ms"]
    line = json.dumps(res)
    print(line)
    if a.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.json_out)), exist_ok=True)
        with open(a.json_out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
