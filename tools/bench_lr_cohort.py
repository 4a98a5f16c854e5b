"""What logistic regression over SQL cohorts costs: the grouped fused encoder
alone, and a verifiable cohort query against the replicated one.  GPU only; one
process.

1. ``native.lr_encode_cells_many`` on one DP of ``--records`` x 44 features
   (1e5 and 1e6 by default) at G = 1 / 6 / 64 / 1024 / 4096 cells (uniform
   keys), without a Where and with one that keeps about a quarter of the rows
   (two terms, each passed by half), beside ``native.lr_encode_many`` on the
   same records and the cell plan alone (``native.lr_cell_plan``: the cell
   kernel, the stable sort, the bucket bounds).  Device events around
   ``--iters`` calls after a warm-up, ``--windows`` windows per case, the cases
   of one size alternating.  The G = 1 result is checked against
   ``lr_encode_many`` (the same bits) and every grouped result against it
   (the cells sum to the whole within rounding) before anything is timed.
   ``--predicate FORMULA``: one more case per G, the ``QuerySQL.Predicate``
   formula over the two terms of the quarter Where (``!(v0 != v1) && !(v2 !=
   v3)`` passes the quarter's rows through the general rule).
2. A verifiable ``logistic regression`` with (16, 5, offset 2^19) range proofs
   over 10 DPs x 10,000 records, d = 8, 3 CNs and 3 VNs: ``GroupBy = [c0, c1]``
   with 3 x 2 real cohorts against the same query without SQL and
   ``GroupByValues = [3, 2, 1]`` (six replicated groups: the same ciphertext
   and proof counts, so the difference is the encoder and the six descents'
   inputs).  A warm-up each, then ``--steps`` timed queries per run,
   alternating, ``--passes`` times; every block is checked outside the timed
   region (all proofs valid).

Prints one JSON object; ``--out-dir`` also writes it as lr_cohort.json.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import tempfile
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from drynx_amd import native as nt  # noqa: E402
from drynx_amd.query import LogisticRegressionParameters, QuerySQL, new_survey_id, parse_predicate  # noqa: E402
from drynx_amd.services.api import DrynxClient  # noqa: E402
from drynx_amd.services.local import local_cluster, make_survey  # noqa: E402

D_FEATURES = 44
GROUPS = {1: [], 6: [(0, 0, 3), (1, 0, 2)], 64: [(2, 0, 64)], 1024: [(3, 0, 32), (4, 0, 32)],
          4096: [(2, 0, 64), (5, 0, 64)]}
FILTERS = {"all": [], "quarter": [(6, 1), (7, 0)]}


def window(f, iters, device) -> float:
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(device)
    a.record()
    for _ in range(iters):
        f()
    e.record()
    torch.cuda.synchronize(device)
    return a.elapsed_time(e) / iters


def encoder_alone(args, device, n) -> dict:
    g = torch.Generator(device=device).manual_seed(11)
    X = torch.rand((n, D_FEATURES), generator=g, device=device, dtype=torch.float64) * 4
    y = torch.randint(0, 2, (n,), generator=g, device=device)
    K = torch.stack([torch.randint(0, v, (n,), generator=g, device=device) for v in (3, 2, 64, 32, 32, 64, 2, 2)], 1)
    m, s = [2.0] * D_FEATURES, [1.15] * D_FEATURES
    calls = {"lr_encode_many": lambda: nt.lr_encode_many([X], [y], m, s, 0.0, -1.0)}
    for G, keys in GROUPS.items():
        for fname, filters in FILTERS.items():
            calls[f"G={G},{fname}"] = (lambda k=keys, f=filters:
                                       nt.lr_encode_cells_many([X], [y], [K], m, s, -1.0, k, f))
            calls[f"plan G={G},{fname}"] = (lambda k=keys, f=filters: nt.lr_cell_plan(K, n, k, f))
        if args.predicate:
            pred = parse_predicate(args.predicate, 2)
            calls[f"G={G},predicate"] = (lambda k=keys, p=pred: nt.lr_encode_cells_many(
                [X], [y], [K], m, s, -1.0, k, FILTERS["quarter"], predicate=p))
            calls[f"plan G={G},predicate"] = (lambda k=keys, p=pred: nt.lr_cell_plan(K, n, k, FILTERS["quarter"],
                                                                                  predicate=p))
    whole = calls["lr_encode_many"]()
    assert torch.equal(calls["G=1,all"]()[:, 0], whole)
    for G in GROUPS:
        parts = calls[f"G={G},all"]().sum(1)
        assert torch.allclose(parts, whole, rtol=1e-9, atol=1e-6), G
    ms = {k: [] for k in calls}
    for f in calls.values():
        for _ in range(3):
            f()
    for _ in range(args.windows):
        for k, f in calls.items():
            ms[k].append(round(window(f, args.iters, device), 5))
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"records": n, "features": D_FEATURES, "ms_per_call": ms, "median_ms": med,
            "spread_ms": {k: round(max(v) - min(v), 5) for k, v in ms.items()},
            "over_lr_encode_many": {k: round(v / med["lr_encode_many"], 3) for k, v in med.items()},
            "record_blocks_per_cell": {f"G={G}": nt._lr_cell_blocks(n, G) for G in GROUPS}}


def verifiable_query(args, device) -> dict:
    rows, n_dps, d = 10_000, 10, 8
    cl, node = local_cluster(3, n_dps, 3, device=device, workdir=tempfile.mkdtemp(prefix="drynx_lr_cohort_"))
    g = torch.Generator(device=device).manual_seed(99)
    data = {}
    for dp in cl.dps:
        X = torch.rand((rows, d), generator=g, device=device, dtype=torch.float64) * 4
        y = torch.randint(0, 2, (rows,), generator=g, device=device)
        K = torch.stack([torch.randint(0, v, (rows,), generator=g, device=device) for v in (3, 2)], 1)
        data[dp.id] = (X, y, K)
    client = DrynxClient(node, device=device)
    lp = LogisticRegressionParameters(NbrRecords=rows * n_dps, NbrFeatures=d, Means=[2.0] * d,
                                      StandardDeviations=[1.15] * d, Lambda=1.0, Step=0.05, MaxIterations=450,
                                      InitialWeights=[0.1] * (d + 1), K=2, PrecisionApproxCoefficients=10.0)
    # |coefficient| <= 1e4 records * 1.74^2 * 10 < 2^19: one (16, 5) range with offset 2^19 for every output
    kw = dict(lr_params=lp, proofs=1, ranges=[16, 5, 1 << 19], thresholds=[1.0, 1.0, 1.0, 0.0, 1.0],
              sig_device=device)
    templates = {"cohorts": make_survey(client, cl, "logistic regression", group_by=(3, 2),
                                        sql=QuerySQL(GroupBy=["c0", "c1"]), **kw),
                 "replicated": make_survey(client, cl, "logistic regression", group_by=(3, 2, 1), **kw)}

    def step(name):
        node.dp_data = data if name == "cohorts" else {k: v[:2] for k, v in data.items()}
        sq = copy.copy(templates[name])
        sq.SurveyID = new_survey_id()
        return client.send_survey_query(sq)

    runs = []
    for name in list(templates) * args.passes:
        step(name)
        node.flush_stores()
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        steps = [step(name) for _ in range(args.steps)]
        node.flush_stores()
        torch.cuda.synchronize(device)
        dt = (time.perf_counter() - t0) / args.steps
        ok = all(r.block is not None and set(r.block.data_block().Proofs.values()) == {1} for _, _, r in steps)
        good = all(len(v) == 6 and all(len(w) == d + 1 and w == w for w in v) for _, v, _ in steps)
        runs.append({"query": name, "s_per_query": round(dt, 5), "all_proofs_valid": ok, "result_ok": good})
    node.close(remove=True)
    per = {k: [r["s_per_query"] for r in runs if r["query"] == k] for k in templates}
    med = {k: statistics.median(v) for k, v in per.items()}
    return {"config": {"cns": 3, "vns": 3, "dps": n_dps, "records_per_dp": rows, "features": d,
                       "range_proof": {"u": 16, "l": 5, "offset": 1 << 19}, "groups": 6, "steps_per_run": args.steps},
            "order": [r["query"] for r in runs], "runs": runs, "s_per_query": per, "median_s": med,
            "spread_s": {k: round(max(v) - min(v), 5) for k, v in per.items()},
            "cohorts_over_replicated": round(med["cohorts"] / med["replicated"], 4),
            "all_proofs_valid": all(r["all_proofs_valid"] for r in runs),
            "result_ok": all(r["result_ok"] for r in runs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--records", type=int, nargs="+", default=[100_000, 1_000_000], help="records of the one DP")
    ap.add_argument("--iters", type=int, default=10, help="encoder calls per timed window")
    ap.add_argument("--windows", type=int, default=3, help="timed windows per encoder case")
    ap.add_argument("--steps", type=int, default=3, help="timed queries per run")
    ap.add_argument("--passes", type=int, default=3, help="times the cohorts / replicated pair is gone through")
    ap.add_argument("--no-query", action="store_true", help="the encoder alone")
    ap.add_argument("--predicate", default="",
                    help="a QuerySQL.Predicate formula over the two terms of the quarter Where: one more case per G")
    ap.add_argument("--out-dir", default=None, help="write lr_cohort.json here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_lr_cohort: no GPU (nothing here is measured on a CPU)")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    out = {"tool": "bench_lr_cohort", "device": torch.cuda.get_device_name(device),
           "calls_per_window": args.iters, "windows": args.windows,
           "what": "ms per call of the binding, device events, the cases of one size alternating",
           "encoder": [encoder_alone(args, device, n) for n in args.records],
           "verifiable_query": None if args.no_query else verifiable_query(args, device)}
    print(json.dumps(out), flush=True)
    if args.out_dir:
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, "lr_cohort.json"), "w") as f:
            json.dump(out, f, indent=1)
    q = out["verifiable_query"]
    if q is not None and not (q["all_proofs_valid"] and q["result_ok"]):
        sys.exit("bench_lr_cohort: a proof was rejected or a decoded result is wrong")


if __name__ == "__main__":
    main()
