"""Cartesian vs distinct-coefficient packing of the headline query, one process, one GPU.

The headline configuration of bench.py (its defaults: 3 CNs, 3 VNs, 10 DPs,
d = 44, 1e5 records per DP, u = l = 16 with the offset, random per-CN
per-column signatures, thresholds [1, 1, 1, 0, 1]) is run with
LogisticRegressionParameters.Packing = 0 (2070 outputs per DP at d = 44) and
Packing = 1 (1080), alternating cartesian / distinct / cartesian / distinct on
the same cluster, the same records and warm clocks.  Each run is a warm-up
query plus ``--steps`` timed queries.  Outside the timed region every timed
query is checked: the decrypted aggregate equals the clear sum of the DPs'
vectors and the weights the clear descent on it (bench.py's --full check).

Prints one JSON object: per layout ms_per_step (all its timed queries), step_ms
per run, outputs_per_dp, prover-table bytes and ledger bytes per query,
all_proofs_valid / result_ok, the spread of each layout's two runs and the
ratio distinct / cartesian.
"""
import argparse
import copy
import json
import os
import sys
import tempfile
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402  (the result check of --full, shared)
from drynx_amd.parallel.comm import init_distributed, make_comm  # noqa: E402
from drynx_amd.query import LogisticRegressionParameters, lr_nbr_outputs, new_survey_id  # noqa: E402
from drynx_amd.services.api import DrynxClient  # noqa: E402
from drynx_amd.services.local import local_cluster, make_survey  # noqa: E402
from drynx_amd.utils import timers  # noqa: E402

LAYOUTS = {"cartesian": 0, "distinct": 1}
HEADLINE_PROOFS = 20_700  # range proofs per headline query: what range_proof.table_mode's 48 GB reserve is sized for


def table_plan(args, device) -> str | None:
    """Both layouts' signature sets stay resident (the runs alternate), next
    to the verifier's working set, which grows with the inbox while
    ``SigMaterial.table_mode`` reserves a fixed 48 GB for it: a set that just
    fits that budget (d = 100: 494,496 points, 237 GB of 4-bit combs) leaves
    too little for 103,020 proofs per query and the device runs out of memory.
    So: the default budgets when the most generous layout of BOTH sets fits
    beside a reserve scaled to the cartesian inbox; otherwise the table-free
    prover (``DRYNX_PROVER_TABLE_BITS=0``) for both layouts alike.
    -> the forced value, or None for the default."""
    if os.environ.get("DRYNX_PROVER_TABLE_BITS") is not None:
        return os.environ["DRYNX_PROVER_TABLE_BITS"]
    if device.type != "cuda":
        return None
    from drynx_amd.proofs.range_proof import LAYOUT_OF_MODE

    n_out = [lr_nbr_outputs(args.features, 2, p) for p in LAYOUTS.values()]
    points = args.cns * args.u * sum(n_out)
    tables = points * LAYOUT_OF_MODE[7].bytes_per_point
    reserve = int((48 << 30) * max(1.0, args.dps * n_out[0] / HEADLINE_PROOFS))
    if tables + reserve <= torch.cuda.mem_get_info(device)[0]:
        return None
    os.environ["DRYNX_PROVER_TABLE_BITS"] = "0"
    return "0"


def parse():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=20, help="timed queries per run (two runs per layout)")
    ap.add_argument("--features", type=int, default=44)
    ap.add_argument("--records", type=int, default=1_000_000, help="records in total, split over the DPs")
    # the rest of bench.py's defaults, fixed here
    ap.set_defaults(cns=3, dps=10, vns=3, u=16, l=16, precision=100.0, max_iter=450)
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args()
    if args.steps < 1 or args.features < 1:
        ap.error("--steps and --features must be at least 1")
    return args


def main():
    args = parse()
    from drynx_amd.utils.streams import node_process_setup

    node_process_setup()
    init_distributed()
    comm = make_comm(None)
    if comm.world != 1:
        sys.exit("bench_lr_packing: one process, one GPU")
    device = comm.device
    if device.type == "cuda":
        torch.cuda.set_device(device)
    cl, node = local_cluster(args.cns, args.dps, args.vns, comm=comm, device=device,
                             workdir=tempfile.mkdtemp(prefix="drynx_lr_packing_"),
                             offsets={"cn": 0, "vn": 0, "dp": 0})
    rec_per_dp = max(1, args.records // args.dps)
    d = args.features
    g = torch.Generator(device=device).manual_seed(1234)  # bench.py's records of rank 0
    dp_data = {}
    for dp in cl.dps:
        X = torch.randint(0, 4, (rec_per_dp, d), generator=g, device=device).to(torch.float64)
        X += torch.rand((rec_per_dp, d), generator=g, device=device, dtype=torch.float64)
        dp_data[dp.id] = (X, torch.randint(0, 2, (rec_per_dp,), generator=g, device=device))
    node.dp_data = dp_data
    offset = min((args.u ** args.l) // 2, 1 << 62)
    forced_tables = table_plan(args, device)
    client = DrynxClient(node, device=device)
    lps, templates = {}, {}
    for name, packing in LAYOUTS.items():
        lps[name] = LogisticRegressionParameters(
            NbrRecords=rec_per_dp * args.dps, NbrFeatures=d, Means=[2.0] * d, StandardDeviations=[1.15] * d,
            Lambda=1.0, Step=0.012, MaxIterations=args.max_iter, InitialWeights=[0.1] * (d + 1), K=2,
            PrecisionApproxCoefficients=args.precision, Packing=packing)
        templates[name] = make_survey(client, cl, "logistic regression", proofs=1, ranges=[args.u, args.l, offset],
                                      lr_params=lps[name], thresholds=[1.0, 1.0, 1.0, 0.0, 1.0], sig_device=device)

    def one_step(name):
        sq = copy.copy(templates[name])
        sq.SurveyID = new_survey_id()
        _, vals, res = client.send_survey_query(sq)
        return res, (vals[0], list(client.last_plaintexts[0]))

    def sync():
        if device.type == "cuda":
            torch.cuda.synchronize()

    runs = []
    for name in ("cartesian", "distinct", "cartesian", "distinct"):
        one_step(name)  # warm-up: the layout's prover tables, warm clocks
        node.flush_stores()
        sync()
        timers.reset()
        t0 = time.perf_counter()
        step_ms, blocks, checks = [], [], []
        for _ in range(args.steps):
            ts = time.perf_counter()
            res, weights = one_step(name)
            step_ms.append(round(1000 * (time.perf_counter() - ts), 1))
            blocks.append(res.block)
            checks.append((weights, res.clear_dp))
        node.flush_stores()  # proof persistence overlaps the next step; the tail is timed too
        sync()
        elapsed = time.perf_counter() - t0
        c = timers.counters()
        # outside the timed region
        ok = all(b is not None and all(v == 1 for v in b.data_block().Proofs.values()) for b in blocks)
        n_out = {len(v[0]) for _, clear in checks for v in clear.values()}
        runs.append({"layout": name, "ms_per_step": round(1000 * elapsed / args.steps, 2), "step_ms": step_ms,
                     "outputs_per_dp": sorted(n_out),
                     "ledger_bytes_per_query": c.get("ledger.blob_bytes", 0) // args.steps,
                     "prover_table_bytes": int(node.verifier_cache.sigmat(templates[name], device).table_bytes()),
                     "prover_table_mode": node.verifier_cache.sigmat(templates[name], device).table_mode(device),
                     "all_proofs_valid": ok, "result_ok": bool(bench._check_lr_results(comm, checks, lps[name]))})
    out = {"tool": "bench_lr_packing", "steps_per_run": args.steps, "order": [r["layout"] for r in runs],
           "config": {"features": d, "cns": args.cns, "vns": args.vns, "dps": args.dps, "records_per_dp": rec_per_dp,
                      "range_proof": {"u": args.u, "l": args.l, "offset": offset},
                      "sigs": "random (per CN, per column)", "thresholds": [1, 1, 1, 0, 1],
                      "prover_tables": ("default budgets" if forced_tables is None
                                        else f"DRYNX_PROVER_TABLE_BITS={forced_tables} for both layouts")},
           "runs": runs}
    for name, packing in LAYOUTS.items():
        mine = [r for r in runs if r["layout"] == name]
        per_run = [r["ms_per_step"] for r in mine]
        assert all(r["outputs_per_dp"] == [lr_nbr_outputs(d, 2, packing)] for r in mine), mine
        out[name] = {"ms_per_step": round(sum(per_run) / len(per_run), 2), "ms_per_step_runs": per_run,
                     "run_spread_ms": round(max(per_run) - min(per_run), 2),
                     "step_ms": [r["step_ms"] for r in mine], "outputs_per_dp": lr_nbr_outputs(d, 2, packing),
                     "prover_table_bytes": mine[-1]["prover_table_bytes"],
                     "prover_table_mode": mine[-1]["prover_table_mode"],
                     "ledger_bytes_per_query": mine[-1]["ledger_bytes_per_query"],
                     "all_proofs_valid": all(r["all_proofs_valid"] for r in mine),
                     "result_ok": all(r["result_ok"] for r in mine)}
    ca, di = out["cartesian"], out["distinct"]
    out["ratio_distinct_over_cartesian"] = {
        "ms_per_step": round(di["ms_per_step"] / ca["ms_per_step"], 4),
        "outputs_per_dp": round(di["outputs_per_dp"] / ca["outputs_per_dp"], 4),
        "prover_table_bytes": round(di["prover_table_bytes"] / max(1, ca["prover_table_bytes"]), 4),
        "ledger_bytes_per_query": round(di["ledger_bytes_per_query"] / max(1, ca["ledger_bytes_per_query"]), 4)}
    out["distinct_faster_by_more_than_cartesian_spread"] = \
        (ca["ms_per_step"] - di["ms_per_step"]) > ca["run_spread_ms"]
    print(json.dumps(out), flush=True)
    if args.json_out:
        with open(args.json_out, "w") as f:
            json.dump(out, f, indent=1)
    node.close(remove=True)
    if not all(out[n]["all_proofs_valid"] and out[n]["result_ok"] for n in LAYOUTS):
        sys.exit("bench_lr_packing: a proof was rejected or a decrypted result is wrong")


if __name__ == "__main__":
    main()
