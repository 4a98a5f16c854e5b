"""What SQL WHERE / GROUP BY costs: the grouped encoder (K14d) alone, and a
verifiable grouped mean against the replicated one.  GPU only; one process.

1. ``native.group_moments`` alone on 10 DPs x 100,000 rows (1e6 rows) with 1, 2
   and 9 value columns (the pairs of ``mean``, ``cosim`` and ``lin_reg`` at
   d = 8), G = 1 / 6 / 1024 groups (no key, keys of 3 x 2 and of 32 x 32 values,
   uniform) and 0 / 2 filter terms (each passed by half of the rows).  Device
   events around ``--iters`` calls after a warm-up, ``--windows`` windows per
   case, the cases of one shape alternating.  ``--predicate FORMULA``
   (repeatable) adds, per G, the case of that ``QuerySQL.Predicate`` formula
   over the first n of the terms ``PREDICATE_TERMS`` (n from the formula's
   highest variable; the first two are the terms of the 2-filter case, the
   other six hold for every row whatever the comparison ``>=`` (terms 2..5) or
   ``<=`` (terms 6, 7)), after a check that ``!(v0 != v1) && !(v2 != v3)``
   gives the 2-filter case's bits: the same rows through the general path.
2. ``native.int_moments`` (K14, untouched by the grouped kernel: the same code
   as without it) on the same value matrix in the same alternation, for the
   G = 1, no-filter case: what grouping costs when it is not used.
3. A verifiable ``mean`` with (16, 5) range proofs over 10 DPs x 10,000
   records, 3 CNs and 3 VNs: ``GroupBy = [c1, c3]`` with 3 x 2 real groups
   against the same query without SQL and ``GroupByValues = [3, 2, 1]`` (six
   replicated groups: the same ciphertext and proof counts, so the difference
   is the encoder).  A warm-up each, then ``--steps`` timed queries per run,
   alternating, ``--passes`` times; every block is checked outside the timed
   region (all proofs valid) and the grouped results against the clear ones.

Prints one JSON object; ``--out-dir`` also writes it as groupby.json.
"""
import argparse
import copy
import json
import os
import re
import statistics
import sys
import tempfile
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from drynx_amd import native as nt  # noqa: E402
from drynx_amd.ops.encoding import moment_pairs  # noqa: E402
from drynx_amd.query import QuerySQL, new_survey_id, parse_predicate  # noqa: E402
from drynx_amd.services.api import DrynxClient  # noqa: E402
from drynx_amd.services.local import local_cluster, make_survey  # noqa: E402

SHAPES = {1: "mean", 2: "cosim", 9: "lin_reg"}  # value columns -> the operation whose pairs are summed
GROUPS = {1: [], 6: [(0, 0, 3), (1, 0, 2)], 1024: [(2, 0, 32), (3, 0, 32)]}
FILTERS = {0: [], 2: [(4, 1), (5, 0)]}
# the Where terms of --predicate: the two of FILTERS[2], then six that every row passes with >= (2..5) or <= (6, 7)
PREDICATE_TERMS = FILTERS[2] + [(0, 0), (1, 0), (2, 0), (3, 0), (4, 1), (5, 1)]


def predicate_case(formula: str):
    """(filters, (ops, table)) of a --predicate formula over the first terms of PREDICATE_TERMS."""
    n = 1 + max([int(v) for v in re.findall(r"v(\d+)", formula)] or [0]) // 2
    if n > len(PREDICATE_TERMS):
        sys.exit(f"bench_groupby: --predicate {formula!r} names more than {len(PREDICATE_TERMS)} terms")
    try:
        return PREDICATE_TERMS[:n], parse_predicate(formula, n)
    except ValueError as e:
        sys.exit(f"bench_groupby: --predicate {formula!r} {e}")


def window(f, iters, device) -> float:
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(device)
    a.record()
    for _ in range(iters):
        f()
    e.record()
    torch.cuda.synchronize(device)
    return a.elapsed_time(e) / iters


def encoder_alone(args, device) -> dict:
    rows = [100_000] * 10
    n = sum(rows)
    g = torch.Generator(device=device).manual_seed(7)
    K = torch.stack([torch.randint(0, v, (n,), generator=g, device=device) for v in (3, 2, 32, 32, 2, 2)], dim=1)
    out = {"records": "10 DPs x 100000", "calls_per_window": args.iters, "windows": args.windows,
           "what": "ms per call (plan upload + launches), device events, the cases of one shape alternating",
           "max_cells_per_launch": nt.GROUP_MOMENTS_MAX_CELLS, "shapes": {}}
    for C, name in SHAPES.items():
        Z = torch.randint(0, 200, (n, C), generator=g, device=device)
        pairs = moment_pairs(name, C)
        calls = {"int_moments": lambda: nt.int_moments(Z, rows, pairs)}
        for G, keys in GROUPS.items():
            for nf, filters in FILTERS.items():
                calls[f"G={G},filters={nf}"] = (lambda k=keys, f=filters: nt.group_moments(Z, K, rows, pairs, k, f))
            for formula in args.predicate:
                filters, pred = predicate_case(formula)
                calls[f"G={G},predicate={formula}"] = (
                    lambda k=keys, f=filters, p=pred: nt.group_moments(Z, K, rows, pairs, k, f, predicate=p))
        # results must agree before anything is timed
        whole = nt.int_moments(Z, rows, pairs)
        assert torch.equal(calls["G=1,filters=0"]()[:, 0], whole)
        assert torch.equal(calls["G=6,filters=0"]().sum(1), whole) and torch.equal(calls["G=1024,filters=0"]().sum(1),
                                                                                   whole)
        if args.predicate:  # the equalities through the general path: the 2-filter case's bits
            same = parse_predicate("!(v0 != v1) && !(v2 != v3)", 2)
            for G, keys in GROUPS.items():
                assert torch.equal(nt.group_moments(Z, K, rows, pairs, keys, FILTERS[2], predicate=same),
                                   calls[f"G={G},filters=2"]())
        ms = {k: [] for k in calls}
        for f in calls.values():
            for _ in range(5):
                f()
        for _ in range(args.windows):
            for k, f in calls.items():
                ms[k].append(round(window(f, args.iters, device), 5))
        med = {k: statistics.median(v) for k, v in ms.items()}
        out["shapes"][f"columns={C}"] = {
            "pairs": len(pairs), "ms_per_call": ms, "median_ms": med,
            "spread_ms": {k: round(max(v) - min(v), 5) for k, v in ms.items()},
            "grouped_G1_over_int_moments": round(med["G=1,filters=0"] / med["int_moments"], 4)}
    return out


def verifiable_mean(args, device) -> dict:
    rows, n_dps = 10_000, 10
    cl, node = local_cluster(3, n_dps, 3, device=device, workdir=tempfile.mkdtemp(prefix="drynx_groupby_"))
    g = torch.Generator(device=device).manual_seed(99)
    node.dp_data = {dp.id: [torch.randint(0, v, (rows,), generator=g, device=device) for v in (4, 3, 2, 2)]
                    for dp in cl.dps}
    client = DrynxClient(node, device=device)
    kw = dict(query_min=0, query_max=3, rows=rows, proofs=1, ranges=[16, 5], sig_device=device)
    templates = {"grouped": make_survey(client, cl, "mean", group_by=(3, 2), sql=QuerySQL(GroupBy=["c1", "c3"]), **kw),
                 "replicated": make_survey(client, cl, "mean", group_by=(3, 2, 1), **kw)}
    # the clear per-group means
    T = torch.cat([torch.stack(cols, dim=1) for cols in node.dp_data.values()]).cpu()
    clear = [float(T[(T[:, 1] == a) & (T[:, 3] == b), 0].sum()) / int(((T[:, 1] == a) & (T[:, 3] == b)).sum())
             for a in range(3) for b in range(2)]

    def step(name):
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
        good = all(len(v) == 6 for _, v, _ in steps)
        if name == "grouped":
            good = good and all(abs(v[i][0] - clear[i]) < 1e-9 for _, v, _ in steps for i in range(6))
        runs.append({"query": name, "s_per_query": round(dt, 5), "all_proofs_valid": ok, "result_ok": good})
    node.close(remove=True)
    per = {k: [r["s_per_query"] for r in runs if r["query"] == k] for k in templates}
    med = {k: statistics.median(v) for k, v in per.items()}
    return {"config": {"cns": 3, "vns": 3, "dps": n_dps, "records_per_dp": rows, "range_proof": {"u": 16, "l": 5},
                       "groups": 6, "steps_per_run": args.steps},
            "order": [r["query"] for r in runs], "runs": runs, "s_per_query": per, "median_s": med,
            "spread_s": {k: round(max(v) - min(v), 5) for k, v in per.items()},
            "grouped_over_replicated": round(med["grouped"] / med["replicated"], 4),
            "all_proofs_valid": all(r["all_proofs_valid"] for r in runs),
            "result_ok": all(r["result_ok"] for r in runs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=50, help="encoder calls per timed window")
    ap.add_argument("--windows", type=int, default=3, help="timed windows per encoder case")
    ap.add_argument("--steps", type=int, default=5, help="timed queries per run")
    ap.add_argument("--passes", type=int, default=3, help="times the grouped / replicated pair is gone through")
    ap.add_argument("--no-query", action="store_true", help="the encoder alone")
    ap.add_argument("--predicate", action="append", default=[],
                    help="a QuerySQL.Predicate formula over the first terms of PREDICATE_TERMS: one more encoder "
                         "case per G (repeatable)")
    ap.add_argument("--out-dir", default=None, help="write groupby.json here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_groupby: no GPU (nothing here is measured on a CPU)")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    out = {"tool": "bench_groupby", "device": torch.cuda.get_device_name(device),
           "encoder": encoder_alone(args, device),
           "verifiable_mean": None if args.no_query else verifiable_mean(args, device)}
    print(json.dumps(out), flush=True)
    if args.out_dir:
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, "groupby.json"), "w") as f:
            json.dump(out, f, indent=1)
    q = out["verifiable_mean"]
    if q is not None and not (q["all_proofs_valid"] and q["result_ok"]):
        sys.exit("bench_groupby: a proof was rejected or a decoded result is wrong")


if __name__ == "__main__":
    main()
