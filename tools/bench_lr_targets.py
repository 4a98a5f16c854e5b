"""One label against several label columns in the headline query, one process, one GPU.

The headline configuration of bench.py (its defaults: 3 CNs, 3 VNs, 10 DPs,
d = 44, 1e5 records per DP, u = l = 16 with the offset, random per-CN
per-column signatures, thresholds [1, 1, 1, 0, 1]) is run with
LogisticRegressionParameters.NbrTargets = 1 (2070 outputs per DP at d = 44)
and NbrTargets = ``--targets`` (3: 2160 outputs, three models), alternating
T=1 / T=3 / T=1 / T=3 on the same cluster, the same features and warm clocks.
Each run is a warm-up query plus ``--steps`` timed queries; one signature set's
prover tables are resident at a time (the warm-up rebuilds them), so both
queries run in the default table layout.  Outside the timed
region every timed query is checked: the decrypted aggregate equals the clear
sum of the DPs' vectors and the weights the clear descents on it (bench.py's
--full check).  The multi-target query is compared with the single-label
steps of the same process, never with itself.

Then the encoder alone (one DP's records, ``lr_encode_many``: the encoder
launches plus the block reduction) for T = 1, 3 and 4 label columns: T = 3
rides in the spare rows of the one 48-row tile-block, T = 4 is the first to
open a fourth row tile.  Device events around ``--encoder-iters`` calls after a
warm-up, the three alternating, twice.

Prints one JSON object; ``--out-dir`` also writes it as bench.json with a
short README.md next to it.
"""
import argparse
import copy
import gc
import json
import os
import sys
import tempfile
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402  (the result check of --full, shared)
from drynx_amd import native as nt  # noqa: E402
from drynx_amd.parallel.comm import init_distributed, make_comm  # noqa: E402
from drynx_amd.query import LogisticRegressionParameters, lr_nbr_outputs, new_survey_id  # noqa: E402
from drynx_amd.services.api import DrynxClient  # noqa: E402
from drynx_amd.services.local import local_cluster, make_survey  # noqa: E402
from drynx_amd.utils import timers  # noqa: E402


def parse():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=20, help="timed queries per run (two runs per target count)")
    ap.add_argument("--features", type=int, default=44)
    ap.add_argument("--targets", type=int, default=3, help="label columns of the multi-target query")
    ap.add_argument("--records", type=int, default=1_000_000, help="records in total, split over the DPs")
    ap.add_argument("--encoder-iters", type=int, default=200, help="encoder calls per timed window")
    # the rest of bench.py's defaults, fixed here
    ap.set_defaults(cns=3, dps=10, vns=3, u=16, l=16, precision=100.0, max_iter=450)
    ap.add_argument("--out-dir", default=None, help="write bench.json and README.md here")
    args = ap.parse_args()
    if args.steps < 1 or args.features < 1 or not 2 <= args.targets <= 64 or args.encoder_iters < 1:
        ap.error("--steps, --features, --encoder-iters at least 1, --targets in 2..64")
    return args


def encoder_alone(args, device, X, labels) -> dict:
    """ms per ``lr_encode_many`` call on one DP's records for T = 1, 3, 4 (device events)."""
    d = args.features
    m, s = [2.0] * d, [1.15] * d
    ys = {1: labels[:, 0].contiguous(), 3: labels[:, :3].contiguous(), 4: labels[:, :4].contiguous()}
    ys = {T: y.to(torch.float64) for T, y in ys.items()}
    out = {T: [] for T in ys}
    for T, y in ys.items():  # warm-up: code objects, allocator
        for _ in range(5):
            nt.lr_encode_many([X], [y], m, s, 0.0, -1.0)
    for _ in range(2):
        for T, y in ys.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(device)
            a.record()
            for _ in range(args.encoder_iters):
                nt.lr_encode_many([X], [y], m, s, 0.0, -1.0)
            b.record()
            torch.cuda.synchronize(device)
            out[T].append(round(a.elapsed_time(b) / args.encoder_iters, 5))
    return {"records": int(X.shape[0]), "features": d, "calls_per_window": args.encoder_iters,
            "what": "lr_encode_many: encoder launches + dx_lr_reduce, device events",
            "ms_per_call": {f"T={T}": v for T, v in out.items()},
            "padded_width": {f"T={T}": nt._lr_padded(d + 1 + T) for T in ys}}


def readme(out: dict) -> str:
    one, many, r = out["T=1"], out["multi"], out["ratio_multi_over_single"]
    T, enc = out["config"]["targets"], out["encoder"]

    def row(*cells):
        return "| " + " | ".join(str(c) for c in cells) + " |"

    def query_row(name, q):
        runs = q["ms_per_step_runs"]
        return row(name, q["outputs_per_dp"], f"{q['ms_per_step']} ({runs[0]} / {runs[1]})",
                   f"{q['prover_table_bytes']:,} (mode {q['prover_table_mode']})", f"{q['ledger_bytes_per_query']:,}")

    lines = [
        "# Multi-target logistic regression (`LogisticRegressionParameters.NbrTargets`)",
        "",
        "One MI355X, one process: `bench.json`, written by",
        f"`tools/bench_lr_targets.py --steps {out['steps_per_run']}`.",
        f"The headline configuration (3 CNs, 3 VNs, 10 DPs, {out['config']['records_per_dp']} records per DP,",
        f"d = {out['config']['features']}, u = l = 16 with the offset, random per-CN per-column signatures, thresholds",
        f"[1, 1, 1, 0, 1]) with one label and with {T} label columns, alternating T=1 / T={T} / T=1 / T={T}.  Each run",
        "is a warm-up query (which rebuilds the run's prover tables: one signature set is resident at a time) plus the",
        "timed queries; every timed query's aggregate and weights are recomputed in the clear outside the timed",
        "region.",
        "",
        row("", "outputs per DP", "ms per query (run 1 / run 2)", "prover-table bytes", "ledger bytes per query"),
        row("---", "---", "---", "---", "---"),
        query_row("T = 1", one),
        query_row(f"T = {T}", many),
        row(f"T = {T} / T = 1", r["outputs_per_dp"], f"**{r['ms_per_step']}**", r["prover_table_bytes"],
            r["ledger_bytes_per_query"]),
        "",
        f"All proofs valid: {one['all_proofs_valid'] and many['all_proofs_valid']}; every result equals the clear",
        f"descent: {one['result_ok'] and many['result_ok']}.  The two T = 1 runs differ by",
        f"{one['run_spread_ms']} ms, the two T = {T} runs by {many['run_spread_ms']} ms.  {T} single-label queries",
        f"would take {T} x {one['ms_per_step']} = {round(T * one['ms_per_step'], 2)} ms and",
        f"{T * one['outputs_per_dp']} outputs per DP: the {T}-target query is",
        f"{out['ratio_multi_over_T_single_queries']} of that.",
        "",
        f"## Encoder alone ({enc['records']} x {enc['features']}, `lr_encode_many`, device events, "
        f"{enc['calls_per_window']} calls per window)",
        "",
        row("label columns", "padded width P", "ms per call (window 1 / window 2)"),
        row("---", "---", "---"),
    ]
    lines += [row(k, enc["padded_width"][k], " / ".join(str(x) for x in v)) for k, v in enc["ms_per_call"].items()]
    lines += [
        "",
        "T = 3 runs the same 3x3 diagonal tile-block as T = 1 (the labels ride in rows 45..47); T = 4 opens a fourth",
        "row tile (P = 64: one 3x3 launch plus one 1x3 launch).  Neither is a gate.",
        ""]
    return "\n".join(lines)


def main():
    args = parse()
    from drynx_amd.utils.streams import node_process_setup

    node_process_setup()
    init_distributed()
    comm = make_comm(None)
    if comm.world != 1:
        sys.exit("bench_lr_targets: one process, one GPU")
    device = comm.device
    if device.type != "cuda":
        sys.exit("bench_lr_targets: needs a GPU (a CPU timing says nothing about the encoder or the provers)")
    torch.cuda.set_device(device)
    cl, node = local_cluster(args.cns, args.dps, args.vns, comm=comm, device=device,
                             workdir=tempfile.mkdtemp(prefix="drynx_lr_targets_"),
                             offsets={"cn": 0, "vn": 0, "dp": 0})
    rec_per_dp = max(1, args.records // args.dps)
    d, T = args.features, args.targets
    g = torch.Generator(device=device).manual_seed(1234)  # bench.py's records of rank 0
    feats, labels = {}, {}
    for dp in cl.dps:
        X = torch.randint(0, 4, (rec_per_dp, d), generator=g, device=device).to(torch.float64)
        X += torch.rand((rec_per_dp, d), generator=g, device=device, dtype=torch.float64)
        feats[dp.id] = X
        labels[dp.id] = torch.randint(0, 2, (rec_per_dp,), generator=g, device=device)
    # further label columns from a generator of their own: column 0 stays bench.py's
    g2 = torch.Generator(device=device).manual_seed(4321)
    more = {dp.id: torch.randint(0, 2, (rec_per_dp, max(T, 4) - 1), generator=g2, device=device) for dp in cl.dps}
    wide = {k: torch.cat([labels[k][:, None], more[k]], 1) for k in labels}
    data = {"T=1": {k: (feats[k], labels[k]) for k in feats},
            "multi": {k: (feats[k], wide[k][:, :T].contiguous()) for k in feats}}
    offset = min((args.u ** args.l) // 2, 1 << 62)
    client = DrynxClient(node, device=device)
    lps, templates = {}, {}
    for name, nt_ in (("T=1", 1), ("multi", T)):
        lps[name] = LogisticRegressionParameters(
            NbrRecords=rec_per_dp * args.dps, NbrFeatures=d, Means=[2.0] * d, StandardDeviations=[1.15] * d,
            Lambda=1.0, Step=0.012, MaxIterations=args.max_iter, InitialWeights=[0.1] * (d + 1), K=2,
            PrecisionApproxCoefficients=args.precision, NbrTargets=nt_)
        templates[name] = make_survey(client, cl, "logistic regression", proofs=1, ranges=[args.u, args.l, offset],
                                      lr_params=lps[name], thresholds=[1.0, 1.0, 1.0, 0.0, 1.0], sig_device=device)

    def one_step(name):
        sq = copy.copy(templates[name])
        sq.SurveyID = new_survey_id()
        _, vals, res = client.send_survey_query(sq)
        return res, (vals[0], list(client.last_plaintexts[0]))

    def drop_tables():
        """One signature set resident at a time: where the two sets' comb tables do not fit together
        beside the verifier's reserve, the second would fall back to a more compact, slower layout.
        Each run's warm-up query rebuilds its set, so both queries get the layout a lone query gets."""
        node.flush_stores()
        node.verifier_cache.drop_signature_tables(device)
        gc.collect()
        torch.cuda.empty_cache()

    runs = []
    for name in ("T=1", "multi", "T=1", "multi"):
        node.dp_data = data[name]
        drop_tables()
        one_step(name)  # warm-up: the query's prover tables, warm clocks
        node.flush_stores()
        torch.cuda.synchronize()
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
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        c = timers.counters()
        # outside the timed region
        ok = all(b is not None and all(v == 1 for v in b.data_block().Proofs.values()) for b in blocks)
        n_out = {len(v[0]) for _, clear in checks for v in clear.values()}
        n_w = {len(w) for (w, _), _ in checks}
        runs.append({"query": name, "ms_per_step": round(1000 * elapsed / args.steps, 2), "step_ms": step_ms,
                     "outputs_per_dp": sorted(n_out), "weights": sorted(n_w),
                     "ledger_bytes_per_query": c.get("ledger.blob_bytes", 0) // args.steps,
                     "prover_table_bytes": int(node.verifier_cache.sigmat(templates[name], device).table_bytes()),
                     "prover_table_mode": node.verifier_cache.sigmat(templates[name], device).table_mode(device),
                     "all_proofs_valid": ok, "result_ok": bool(bench._check_lr_results(comm, checks, lps[name]))})
    out = {"tool": "bench_lr_targets", "steps_per_run": args.steps, "order": [r["query"] for r in runs],
           "config": {"features": d, "targets": T, "cns": args.cns, "vns": args.vns, "dps": args.dps,
                      "records_per_dp": rec_per_dp, "range_proof": {"u": args.u, "l": args.l, "offset": offset},
                      "sigs": "random (per CN, per column)", "thresholds": [1, 1, 1, 0, 1]},
           "runs": runs}
    for name, nt_ in (("T=1", 1), ("multi", T)):
        mine = [r for r in runs if r["query"] == name]
        per_run = [r["ms_per_step"] for r in mine]
        n_out = lr_nbr_outputs(d, 2, 0, nt_)
        assert all(r["outputs_per_dp"] == [n_out] and r["weights"] == [nt_ * (d + 1)] for r in mine), mine
        out[name] = {"targets": nt_, "ms_per_step": round(sum(per_run) / len(per_run), 2), "ms_per_step_runs": per_run,
                     "run_spread_ms": round(max(per_run) - min(per_run), 2),
                     "step_ms": [r["step_ms"] for r in mine], "outputs_per_dp": n_out,
                     "prover_table_bytes": mine[-1]["prover_table_bytes"],
                     "prover_table_mode": mine[-1]["prover_table_mode"],
                     "ledger_bytes_per_query": mine[-1]["ledger_bytes_per_query"],
                     "all_proofs_valid": all(r["all_proofs_valid"] for r in mine),
                     "result_ok": all(r["result_ok"] for r in mine)}
    one, many = out["T=1"], out["multi"]
    out["ratio_multi_over_single"] = {
        "ms_per_step": round(many["ms_per_step"] / one["ms_per_step"], 4),
        "outputs_per_dp": round(many["outputs_per_dp"] / one["outputs_per_dp"], 4),
        "prover_table_bytes": round(many["prover_table_bytes"] / max(1, one["prover_table_bytes"]), 4),
        "ledger_bytes_per_query": round(many["ledger_bytes_per_query"] / max(1, one["ledger_bytes_per_query"]), 4)}
    out["ratio_multi_over_T_single_queries"] = round(many["ms_per_step"] / (T * one["ms_per_step"]), 4)
    first = cl.dps[0].id
    out["encoder"] = encoder_alone(args, device, feats[first][:100_000], wide[first][:100_000])
    print(json.dumps(out), flush=True)
    if args.out_dir:
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, "bench.json"), "w") as f:
            json.dump(out, f, indent=1)
        with open(os.path.join(args.out_dir, "README.md"), "w") as f:
            f.write(readme(out))
    node.close(remove=True)
    if not all(out[n]["all_proofs_valid"] and out[n]["result_ok"] for n in ("T=1", "multi")):
        sys.exit("bench_lr_targets: a proof was rejected or a decrypted result is wrong")


if __name__ == "__main__":
    main()
