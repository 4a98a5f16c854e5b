"""Two trees' encoder-alone cases side by side.

Reads a folder of ``<tree>_<pair>_{groupby,lr_cohort,iter}.json`` files, the
outputs of ``tools/bench_groupby.py --no-query``, ``tools/bench_lr_cohort.py
--no-query`` and ``tools/bench_iter.py --groups V`` run on the trees ``parent``
and ``new`` alternating, pair by pair.  Per case it prints the median and the
[min, max] of each tree's per-run medians and marks a case whose ``new`` median
lies above the parent's own maximum (ABOVE) or below its minimum (below).

Usage: python tools/ab_encoder_cases.py DIR
"""
import glob
import json
import os
import statistics as st
import sys


def cases(d, tag, i):
    out = {}
    g = json.load(open(f"{d}/{tag}_{i}_groupby.json"))
    for shape, v in g["encoder"]["shapes"].items():
        for k, m in v["median_ms"].items():
            out[f"groupby {shape} {k}"] = m
    lr = json.load(open(f"{d}/{tag}_{i}_lr_cohort.json"))
    for e in lr["encoder"]:
        for k, m in e["median_ms"].items():
            out[f"lr n={e['records']} {k}"] = m
    it = json.load(open(f"{d}/{tag}_{i}_iter.json"))
    for label, ms in it["encoder"]["ms_per_call"].items():
        for k, v in ms.items():
            out[f"iter {label} {k}"] = st.median(v)
    return out


def main():
    d = sys.argv[1]
    pairs = sorted({int(os.path.basename(f).split("_")[1]) for f in glob.glob(d + "/parent_*_groupby.json")})
    parent, new = [cases(d, "parent", i) for i in pairs], [cases(d, "new", i) for i in pairs]
    rows = []
    for k in parent[0]:
        p, n = [x[k] for x in parent], [x[k] for x in new]
        rows.append((k, st.median(p), min(p), max(p), st.median(n), min(n), max(n)))
    print(f"{len(rows)} cases, {len(pairs)} pairs; new median above the parent's max: "
          f"{sum(r[4] > r[3] for r in rows)}, below its min: {sum(r[4] < r[2] for r in rows)}")
    for r in rows:
        flag = "ABOVE" if r[4] > r[3] else ("below" if r[4] < r[2] else "")
        print(f"{r[0]:55s} parent {r[1]:.4f} [{r[2]:.4f},{r[3]:.4f}]  new {r[4]:.4f} [{r[5]:.4f},{r[6]:.4f}] "
              f"x{r[4] / r[1]:.3f} {flag}")


if __name__ == "__main__":
    main()
