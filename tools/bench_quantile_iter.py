"""Iterative (digit-by-digit) quantile against the one-shot frequencyCount over a range of N values.

3 CNs, 3 VNs and 10 DPs with ``--rows`` records each (default 100), uniform in
[0, N), range proofs on every output with ranges sized to a DP's record count
(u = 16, the smallest l with 16^l > rows), random per-CN per-column
signatures, thresholds [1, 1, 1, 0, 1].  The ``--quantile`` (num/den, default
1/2) is searched with ``DrynxClient.send_iterative_quantile`` once per base of
``--bases`` and, where N <= 100000, the classic one-shot ``frequencyCount`` of
the same domain is run and the quantile read off its histogram, alternating
base / ... / classic / base / ... / classic (``--passes`` times, default 2) in
one process on the same cluster and records.  Each run is a warm-up (which
builds the run's prover and verifier tables: one signature set is resident at
a time) plus ``--steps`` timed searches or queries.  Outside the timed region
every round's block is checked (all proofs valid) and every result is compared
with the clear nearest-rank quantile of all DPs' records.

On a GPU the encoder alone is timed too: the two-launch kernel pair
(``native.digit_histogram``) on 10 DPs x 100000 records, uniform and with every
record equal (all LDS atomics of a workgroup on one counter), device events
after a warm-up.

``--gpus W`` (W > 1) starts W ranks; the ranks without the querier serve the
rounds (``serve_iterative``).  Prints one JSON object; ``--out-dir`` also
writes it as range_<N>.json.
"""
import argparse
import copy
import gc
import json
import os
import socket
import subprocess
import sys
import tempfile
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402  (the launcher's argument forwarding and the world check, shared)
from drynx_amd import native as nt  # noqa: E402
from drynx_amd.parallel.comm import init_distributed, make_comm  # noqa: E402
from drynx_amd.query import ITER_MAX_HIST_BASE, iter_rounds, new_survey_id  # noqa: E402
from drynx_amd.services.api import DrynxClient, serve_iterative  # noqa: E402
from drynx_amd.services.local import local_cluster, make_iterative_survey, make_survey  # noqa: E402
from drynx_amd.utils import timers  # noqa: E402

CLASSIC_MAX_RANGE = 100_000


def parse():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--range", dest="value_range", type=int, default=1_000, help="values in [0, RANGE)")
    ap.add_argument("--bases", default="10,32,100,1000", help="comma-separated bases of the iterative search")
    ap.add_argument("--quantile", default="1/2", help="num/den of the nearest-rank quantile")
    ap.add_argument("--rows", type=int, default=100, help="records per DP")
    ap.add_argument("--steps", type=int, default=5, help="timed searches / queries per run")
    ap.add_argument("--passes", type=int, default=2, help="times the whole list of runs is gone through")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--device", default=None)
    ap.add_argument("--no-classic", action="store_true", help="skip the one-shot frequencyCount")
    ap.add_argument("--encoder-iters", type=int, default=200, help="encoder calls per timed window (GPU only)")
    ap.add_argument("--out-dir", default=None, help="write range_<N>.json here")
    ap.set_defaults(cns=3, dps=10, vns=3)
    args = ap.parse_args()
    try:
        args.base_list = [int(b) for b in args.bases.split(",") if b]
        num, _, den = args.quantile.partition("/")
        args.num, args.den = int(num), int(den or 1)
    except ValueError:
        ap.error("--bases is a comma-separated list of integers, --quantile is num/den")
    if args.passes < 1 or args.steps < 1 or args.rows < 1 or args.value_range < 2 or not args.base_list \
            or any(not 2 <= b <= ITER_MAX_HIST_BASE for b in args.base_list):
        ap.error(f"--passes, --steps and --rows at least 1, --range at least 2, bases in 2..{ITER_MAX_HIST_BASE}")
    if args.den < 1 or not 0 <= args.num <= args.den:
        ap.error("--quantile num/den with 0 <= num <= den")
    return args


def launch_ranks(args) -> int | None:
    """``--gpus W`` run directly: W ranks as a child job (this process has made no GPU call)."""
    if "WORLD_SIZE" in os.environ or args.gpus <= 1:
        return None
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__),
           *bench._forward_args(sys.argv[1:])]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS", "1"))
    return subprocess.call(cmd, env=env)


def nearest_rank(values, num, den):
    s = sorted(values)
    return s[max(1, (num * len(s) + den - 1) // den) - 1]


def quantile_of_histogram(counts, num, den):
    """Index of the nearest-rank quantile in a histogram (the classic query's decoded result)."""
    t = max(1, (num * sum(counts) + den - 1) // den)
    cum = 0
    for i, c in enumerate(counts):
        cum += c
        if cum >= t:
            return i
    raise RuntimeError("no records in the domain")


def encoder_alone(args, device) -> dict:
    """ms per call of the kernel pair on uniform records and on all-equal ones (device events)."""
    g = torch.Generator(device=device).manual_seed(7)
    rows = [100_000] * 10
    out = {"records": "10 DPs x 100000", "calls_per_window": args.encoder_iters,
           "what": "digit_histogram (two launches + the plan upload), round 0 over base^2 values, uniform records "
                   "vs every record equal, device events, three windows each, alternating", "ms_per_call": {}}
    for b in (10, 1000, 4096):
        R = b ** 2
        Zu = torch.randint(0, R, (sum(rows), 1), generator=g, device=device)
        Ze = torch.full((sum(rows), 1), R // 2, dtype=torch.int64, device=device)
        calls = {"uniform": lambda: nt.digit_histogram(Zu, rows, 0, R - 1, b, 0, 0),
                 "all_equal": lambda: nt.digit_histogram(Ze, rows, 0, R - 1, b, 0, 0)}
        ms = {k: [] for k in calls}
        for f in calls.values():
            for _ in range(5):
                f()
        for _ in range(3):
            for k, f in calls.items():
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(device)
                a.record()
                for _ in range(args.encoder_iters):
                    f()
                e.record()
                torch.cuda.synchronize(device)
                ms[k].append(round(a.elapsed_time(e) / args.encoder_iters, 5))
        out["ms_per_call"][f"base={b}"] = ms
    return out


def main():
    args = parse()
    rc = launch_ranks(args)
    if rc is not None:
        sys.exit(rc)
    init_distributed()
    comm = make_comm(args.device)
    bench._check_world(args, comm)
    world, rank = comm.world, comm.rank
    device = comm.device
    if device.type == "cuda":
        torch.cuda.set_device(device)
    N, n_dps, rows = args.value_range, args.dps, args.rows
    l = 1
    while 16 ** l <= rows:
        l += 1
    offsets = {"cn": 0, "vn": args.cns % world, "dp": (args.cns + args.vns) % world}
    cl, node = local_cluster(args.cns, n_dps, args.vns, comm=comm, device=device,
                             workdir=tempfile.mkdtemp(prefix=f"drynx_quantile_iter_r{rank}_"), offsets=offsets)
    g = torch.Generator(device=device).manual_seed(99 + rank)
    node.dp_data = {dp.id: list(torch.randint(0, N, (1, rows), generator=g, device=device))
                    for dp in cl.local(rank, "dp")}
    mine = [int(x) for cols in node.dp_data.values() for x in cols[0].cpu().tolist()]
    want = nearest_rank([x for part in comm.all_gather_object(mine) for x in part], args.num, args.den)
    client = DrynxClient(node, device=device) if rank == 0 else None
    classic = not args.no_classic and N <= CLASSIC_MAX_RANGE
    names = [f"base={b}" for b in args.base_list] + (["classic"] if classic else [])
    thresholds = [1.0, 1.0, 1.0, 0.0, 1.0]
    templates, sig_s = {}, {}
    if rank == 0:
        for name in names:
            t0 = time.perf_counter()
            if name == "classic":
                templates[name] = make_survey(client, cl, "frequencyCount", query_min=0, query_max=N - 1, rows=rows,
                                              proofs=1, ranges=[16, l], thresholds=thresholds, sig_device=device)
            else:
                templates[name] = make_iterative_survey(client, cl, "frequencyCount", int(name[5:]), query_min=0,
                                                        query_max=N - 1, rows=rows, proofs=1, ranges=[16, l],
                                                        thresholds=thresholds, sig_device=device)
            sig_s[name] = round(time.perf_counter() - t0, 3)

    def one_step(name):
        """-> (quantile, [blocks], [ms per round]) on rank 0."""
        if name == "classic":
            if rank != 0:
                node.run_survey(None)
                return None
            sq = copy.copy(templates[name])
            sq.SurveyID = new_survey_id()
            _, vals, res = client.send_survey_query(sq)
            return quantile_of_histogram([int(round(v)) for v in vals[0]], args.num, args.den), [res.block], []
        if rank != 0:
            serve_iterative(node)
            return None
        sq = copy.copy(templates[name])
        sq.SurveyID = new_survey_id()
        marks = [time.perf_counter()]
        value, rounds = client.send_iterative_quantile(sq, int(name[5:]), args.num, args.den,
                                                       on_round=lambda *_: marks.append(time.perf_counter()))
        return value, [r.block for r in rounds], [round(1000 * (b - a), 2) for a, b in zip(marks, marks[1:])]

    def drop_tables():
        node.flush_stores()
        if device.type == "cuda":
            node.verifier_cache.drop_signature_tables(device)
            gc.collect()
            torch.cuda.empty_cache()

    def sync():
        comm.barrier()
        if device.type == "cuda":
            torch.cuda.synchronize()

    runs = []
    for name in names * args.passes:
        drop_tables()
        t_first = time.perf_counter()
        one_step(name)  # warm-up: the run's tables, warm clocks
        first_s = time.perf_counter() - t_first
        node.flush_stores()
        sync()
        timers.reset()
        t0 = time.perf_counter()
        steps = [one_step(name) for _ in range(args.steps)]
        node.flush_stores()
        sync()
        elapsed = max(comm.all_gather_object(time.perf_counter() - t0))
        if rank != 0:
            continue
        # outside the timed region
        blocks = [b for _, bl, _ in steps for b in bl]
        ok = all(b is not None and all(v == 1 for v in b.data_block().Proofs.values()) for b in blocks)
        per_round = [ms for _, _, rms in steps for ms in rms]
        runs.append({"query": name, "s_per_result": round(elapsed / args.steps, 5), "first_s": round(first_s, 3),
                     "rounds": len(steps[0][1]) if name != "classic" else None,
                     "blocks_per_result": len(steps[0][1]),
                     "ms_per_round": round(sum(per_round) / len(per_round), 2) if per_round else None,
                     "round_ms": [rms for _, _, rms in steps],
                     "all_proofs_valid": ok, "result_ok": all(int(round(v)) == want for v, _, _ in steps)})
    encoder = encoder_alone(args, device) if rank == 0 and device.type == "cuda" and world == 1 else None
    node.close(remove=True)
    if rank != 0:
        return
    out = {"tool": "bench_quantile_iter", "range": N, "quantile": f"{args.num}/{args.den}",
           "steps_per_run": args.steps, "n_gpus": world, "device": device.type,
           "order": [r["query"] for r in runs], "clear_quantile": want,
           "config": {"cns": args.cns, "vns": args.vns, "dps": n_dps, "records_per_dp": rows,
                      "range_proof": {"u": 16, "l": l}, "sigs": "random (per CN, per column)",
                      "thresholds": [1, 1, 1, 0, 1]},
           "signature_setup_s": sig_s, "runs": runs, "queries": {}}
    for name in names:
        mine = [r for r in runs if r["query"] == name]
        per_run = [r["s_per_result"] for r in mine]
        out["queries"][name] = {
            "s_per_result": round(sum(per_run) / len(per_run), 5), "s_per_result_runs": per_run,
            "rounds": iter_rounds(0, N - 1, int(name[5:])) if name != "classic" else None,
            "outputs_per_dp_and_round": int(name[5:]) if name != "classic" else N,
            "ms_per_round": mine[-1]["ms_per_round"],
            "all_proofs_valid": all(r["all_proofs_valid"] for r in mine),
            "result_ok": all(r["result_ok"] for r in mine)}
    it = {k: v for k, v in out["queries"].items() if k != "classic"}
    best = min(it, key=lambda k: it[k]["s_per_result"])
    out["best_base"] = {"query": best, "s_per_result": it[best]["s_per_result"]}
    if classic:
        out["iterative_over_classic"] = round(it[best]["s_per_result"] / out["queries"]["classic"]["s_per_result"], 4)
    out["all_proofs_valid"] = all(q["all_proofs_valid"] for q in out["queries"].values())
    out["result_ok"] = all(q["result_ok"] for q in out["queries"].values())
    out["encoder"] = encoder
    print(json.dumps(out), flush=True)
    if args.out_dir:
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, f"range_{N}.json"), "w") as f:
            json.dump(out, f, indent=1)
    if not (out["all_proofs_valid"] and out["result_ok"]):
        sys.exit("bench_quantile_iter: a proof was rejected or a decoded result is wrong")


if __name__ == "__main__":
    main()
