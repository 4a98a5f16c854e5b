"""Iterative (digit-by-digit) max or quantile against its one-shot query over a range of N values.

``--query max``: bench.py's ``--query max`` configuration (3 CNs, 3 VNs, 10 DPs
with 100 records each, uniform in [0, N), (2, 1) range proofs on every output,
random per-CN per-column signatures, thresholds [1, 1, 1, 0, 1]) is run as an
iterative search (``DrynxClient.send_iterative_extreme``) and as the classic
one-shot unary ``max``.

``--query quantile``: the same cluster with ``--rows`` records per DP (default
100) and ranges sized to a DP's record count (u = 16, the smallest l with
16^l > rows).  The ``--quantile`` (num/den, default 1/2) is searched with
``DrynxClient.send_iterative_quantile``; the classic query is the one-shot
``frequencyCount`` of the same domain, the quantile read off its histogram.

The search runs once per base of ``--bases`` and, where N <= 100000, the
classic query too, alternating base / ... / classic / base / ... / classic
(``--passes`` times, default 2) in one process on the same cluster and
records.  Each run is a warm-up (which builds the run's prover and verifier
tables: one signature set is resident at a time) plus ``--steps`` timed
searches or queries.  Outside the timed region every round's block is checked
(all proofs valid) and every result is compared with the clear max, or the
clear nearest-rank quantile, of all DPs' records.

On a GPU the encoder alone is timed too, on 10 DPs x 100000 records with device
events after a warm-up: the two-launch kernel pair (``native.iter_round``) for
``max`` against ``ops.encoding.batch_values("max")`` at the same output width;
for ``frequencyCount`` on uniform records and with every record equal (all LDS
atomics of a workgroup on one counter).

``--groups V`` runs the searches over SQL cohorts: every DP holds a table (x,
c1 uniform in [0, V), c2 uniform in [0, 3]), the survey carries ``GROUP BY c1``
(and ``--where c2=1`` a WHERE term, ``--predicate 'v0 >= v1'`` a
``QuerySQL.Predicate`` formula over that one term), and one walk finds the
quantile or max of every cell (``SurveyQuery.IterPrefixes``).  A result is right when every cell's
value equals the clear one of the redrawn tables (NaN, or the one-shot empty
value QueryMin for ``max``, for a cell without records).  The one-shot SQL query
alternates where V * N <= 100000.  The encoder alone is then the grouped digit
histogram ``native.iter_round_cells`` for V in {1, 16, 256, 4096} at base 10 and
1000, uniform keys against every row in one cell and one bin, beside
``native.iter_round`` on the same records and ``native.group_moments(...,
bins=...)`` on the last-round shape; with ``--where`` also the uniform case
under that equality (``uniform_where``) and with ``--predicate`` under the
formula (``uniform_predicate``), on a table with the column c2.

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

import bench  # noqa: E402  (the max configuration, the reference rows, the launcher's argument forwarding, shared)
from drynx_amd import native as nt  # noqa: E402
from drynx_amd.ops import encoding as enc  # noqa: E402
from drynx_amd.parallel.comm import init_distributed, make_comm  # noqa: E402
from drynx_amd.query import QuerySQL, WhereClear, iter_rounds, new_survey_id, parse_predicate  # noqa: E402
from drynx_amd.rounds import ITER_MAX_CELL_OUTPUTS, ITER_MAX_HIST_BASE, max_base  # noqa: E402
from drynx_amd.services.api import DrynxClient, serve_iterative  # noqa: E402
from drynx_amd.services.local import local_cluster, make_iterative_survey, make_survey  # noqa: E402
from drynx_amd.utils import timers  # noqa: E402

# the reference's "Optimized (iterative) max" series (simul/test_data/graphs/TIFS/maxOpti.py:13): totals
REFERENCE_MAX_ITERATIVE_S = {1_000: 5.6, 10_000: 7.6, 100_000: 9.6, 1_000_000: 11.3}
CLASSIC_MAX_RANGE = 100_000
OPERATION = {"max": "max", "quantile": "frequencyCount"}


def parse():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--query", choices=sorted(OPERATION), required=True)
    ap.add_argument("--range", dest="value_range", type=int, default=1_000, help="values in [0, RANGE)")
    ap.add_argument("--bases", default="10,32,100,1000", help="comma-separated bases of the iterative search")
    ap.add_argument("--quantile", default="1/2", help="num/den of the nearest-rank quantile (--query quantile)")
    ap.add_argument("--rows", type=int, default=100, help="records per DP (--query quantile)")
    ap.add_argument("--steps", type=int, default=5, help="timed searches / queries per run")
    ap.add_argument("--passes", type=int, default=2, help="times the whole list of runs is gone through")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--device", default=None)
    ap.add_argument("--no-classic", action="store_true", help="skip the one-shot query")
    ap.add_argument("--groups", type=int, default=0, help="V > 0: GROUP BY c1 over V groups, one search per cell")
    ap.add_argument("--where", default=None, help="with --groups: a WHERE term c2=<0..3> (e.g. c2=1)")
    ap.add_argument("--predicate", default="",
                    help="with --where: a QuerySQL.Predicate formula over the one term, e.g. 'v0 >= v1'")
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
    args.where_value = None
    if args.where is not None:
        col, _, val = args.where.partition("=")
        if not args.groups or col != "c2" or not val.isdigit():
            ap.error("--where c2=<value> goes with --groups")
        args.where_value = int(val)
    args.where_predicate = None
    if args.predicate:
        if args.where_value is None:
            ap.error("--predicate goes with --where")
        try:
            args.where_predicate = parse_predicate(args.predicate, 1)
        except ValueError as e:
            ap.error(f"--predicate {e}")
    top = min(max_base(OPERATION[args.query]), ITER_MAX_HIST_BASE) if args.groups else max_base(OPERATION[args.query])
    if args.groups < 0 or args.groups > 4096 or any(args.groups * b > ITER_MAX_CELL_OUTPUTS for b in args.base_list):
        ap.error(f"--groups in 1..4096 with groups * base at most {ITER_MAX_CELL_OUTPUTS}")
    if args.passes < 1 or args.steps < 1 or args.rows < 1 or args.value_range < 2 or not args.base_list \
            or any(not 2 <= b <= top for b in args.base_list):
        ap.error(f"--passes, --steps and --rows at least 1, --range at least 2, bases in 2..{top}")
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


class MaxQuery:
    """What ``--query max`` sets: bench.py's record count, (2, 1) ranges, the clear max."""
    ranges = None  # make_iterative_survey's own (2, 1)
    classic_ranges = [2, 1]
    range_proof = {"u": 2, "l": 1}

    def __init__(self, args):
        cfg = bench.QUERY_CONFIGS["max"]
        self.dps, self.rows = cfg["dps"], cfg["records"] // cfg["dps"]

    def clear(self, comm, mine):
        mx = comm.all_gather_object(max(mine, default=None))
        return max(v for v in mx if v is not None)

    def clear_cell(self, values):
        """A cell's clear result; without records what the one-shot SQL max decodes to (QueryMin = 0)."""
        return max(values, default=0)

    def search(self, client, sq, base, on_round):
        return client.send_iterative_extreme(sq, base, on_round=on_round)

    def classic_value(self, vals):
        return vals[0][0]

    def classic_cell(self, v):
        return self.classic_value([v])

    def head(self, N, want):
        return {"clear_max": want}

    def reference(self, N):
        return {"reference": {"unary_s": bench.REFERENCE_MAX_UNARY_S.get(N),
                              "iterative_s": REFERENCE_MAX_ITERATIVE_S.get(N),
                              "source": "simul/test_data/graphs/TIFS/maxOpti.py:9-13"}}

    probe_what = ("iter_round('max') (two launches + the plan upload) vs batch_values('max') at the same "
                  "output width, device events, three windows each, alternating")

    def probe_cases(self, rows, g, device):
        for b in (10, 1000):
            Z = torch.randint(0, b ** 2, (sum(rows), 1), generator=g, device=device)
            yield f"width={b}", {"kernel_pair": lambda: nt.iter_round("max", Z, rows, 0, b ** 2 - 1, b, 0, 0),
                                 "batch_values": lambda: enc.batch_values("max", Z, rows, 0, b - 1)}


class QuantileQuery:
    """What ``--query quantile`` sets: ``--rows`` records, (16, l) ranges, the clear nearest-rank quantile."""

    def __init__(self, args):
        self.dps, self.rows, self.num, self.den = args.dps, args.rows, args.num, args.den
        l = 1
        while 16 ** l <= self.rows:
            l += 1
        self.ranges = self.classic_ranges = [16, l]
        self.range_proof = {"u": 16, "l": l}

    def clear(self, comm, mine):
        return nearest_rank([x for part in comm.all_gather_object(mine) for x in part], self.num, self.den)

    def clear_cell(self, values):
        """A cell's clear result, None (a NaN from the search) without records."""
        return nearest_rank(values, self.num, self.den) if values else None

    def search(self, client, sq, base, on_round):
        return client.send_iterative_quantile(sq, base, self.num, self.den, on_round=on_round)

    def classic_value(self, vals):
        return quantile_of_histogram([int(round(v)) for v in vals[0]], self.num, self.den)

    def classic_cell(self, v):
        """A cell of the one-shot SQL query; NaN without records, as the search returns."""
        return self.classic_value([v]) if any(int(round(x)) for x in v) else float("nan")

    def head(self, N, want):
        return {"quantile": f"{self.num}/{self.den}", "clear_quantile": want}

    def reference(self, N):
        return {}

    probe_what = ("iter_round('frequencyCount') (two launches + the plan upload), round 0 over base^2 values, "
                  "uniform records vs every record equal, device events, three windows each, alternating")

    def probe_cases(self, rows, g, device):
        for b in (10, 1000, 4096):
            R = b ** 2
            Zu = torch.randint(0, R, (sum(rows), 1), generator=g, device=device)
            Ze = torch.full((sum(rows), 1), R // 2, dtype=torch.int64, device=device)
            yield f"base={b}", {"uniform": lambda: nt.iter_round("frequencyCount", Zu, rows, 0, R - 1, b, 0, 0),
                                "all_equal": lambda: nt.iter_round("frequencyCount", Ze, rows, 0, R - 1, b, 0, 0)}


QUERIES = {"max": MaxQuery, "quantile": QuantileQuery}

COHORT_PROBE_WHAT = ("iter_round_cells('frequencyCount') (one launch per group window + the plan and prefix uploads), "
                     "round 0 over base^2 values, GROUP BY over V groups: uniform keys vs every row in one cell and "
                     "one bin; at V = 1 iter_round('frequencyCount') on the same records; group_moments(bins=) on "
                     "the last-round shape (V x base cells); device events, three windows each, alternating")


def passes_where(args, c2: int) -> bool:
    """Does a record with this c2 pass --where / --predicate (the one atom's bit indexes the truth table)?"""
    if args.where_value is None:
        return True
    if args.where_predicate is None:
        return c2 == args.where_value
    (op,), table = args.where_predicate
    atom = {"==": c2 == args.where_value, "!=": c2 != args.where_value, "<": c2 < args.where_value,
            "<=": c2 <= args.where_value, ">": c2 > args.where_value, ">=": c2 >= args.where_value}[op]
    return bool(table >> int(atom) & 1)


def cohort_probe_cases(rows, g, device, where_value=None, predicate=None):
    n = sum(rows)
    for b in (10, 1000):
        R = b ** 2
        x = torch.randint(0, R, (n,), generator=g, device=device)
        for V in (1, 16, 256, 4096):
            if V * b > ITER_MAX_CELL_OUTPUTS:
                continue  # refused by the query rules and the entry alike
            Ku = torch.stack([x, torch.randint(0, V, (n,), generator=g, device=device)], dim=1)
            Ke = torch.stack([torch.full_like(x, R // 2), torch.full_like(x, V // 2)], dim=1)
            keys, zero = [(1, 0, V)], [0] * V

            def cells(K, keys=keys, zero=zero, b=b, R=R):
                return lambda: nt.iter_round_cells("frequencyCount", K, rows, 0, 0, R - 1, b, 0, zero, keys)

            calls = {"uniform": cells(Ku), "one_cell_one_bin": cells(Ke),
                     "group_moments_bins": lambda K=Ku, keys=keys, b=b: nt.group_moments(
                         K[:, :0], K, rows, [(0, 0)], keys, bins=(0, 0, b))}
            if where_value is not None:  # the same rows and keys with the filter column c2 in [0, 3]
                Kf = torch.cat([Ku, torch.randint(0, 4, (n, 1), generator=g, device=device)], dim=1)
                calls["uniform_where"] = lambda K=Kf, keys=keys, zero=zero, b=b, R=R: nt.iter_round_cells(
                    "frequencyCount", K, rows, 0, 0, R - 1, b, 0, zero, keys, [(2, where_value)])
                if predicate is not None:
                    calls["uniform_predicate"] = lambda K=Kf, keys=keys, zero=zero, b=b, R=R: nt.iter_round_cells(
                        "frequencyCount", K, rows, 0, 0, R - 1, b, 0, zero, keys, [(2, where_value)], predicate)
            if V == 1:
                calls["iter_round"] = lambda K=Ku, b=b, R=R: nt.iter_round("frequencyCount", K, rows, 0, R - 1, b, 0, 0)
                calls["iter_round_one_bin"] = lambda K=Ke, b=b, R=R: nt.iter_round("frequencyCount", K, rows, 0, R - 1,
                                                                                  b, 0, 0)
            yield f"base={b},V={V}", calls


def encoder_alone(args, query, device) -> dict:
    """ms per call of the query's kernel-probe cases (device events); with ``--groups`` the cohort cases."""
    g = torch.Generator(device=device).manual_seed(7)
    rows = [100_000] * 10
    out = {"records": "10 DPs x 100000", "calls_per_window": args.encoder_iters,
           "what": COHORT_PROBE_WHAT if args.groups else query.probe_what, "ms_per_call": {}}
    cases = cohort_probe_cases(rows, g, device, args.where_value, args.where_predicate) if args.groups else \
        query.probe_cases(rows, g, device)
    for label, calls in cases:
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
        out["ms_per_call"][label] = ms
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
    query, op_name = QUERIES[args.query](args), OPERATION[args.query]
    N, n_dps, rows = args.value_range, query.dps, query.rows
    offsets = {"cn": 0, "vn": args.cns % world, "dp": (args.cns + args.vns) % world}
    cl, node = local_cluster(args.cns, n_dps, args.vns, comm=comm, device=device,
                             workdir=tempfile.mkdtemp(prefix=f"drynx_{args.query}_iter_r{rank}_"), offsets=offsets)
    g = torch.Generator(device=device).manual_seed(99 + rank)  # bench.py's records
    node.dp_data = {dp.id: list(torch.randint(0, N, (1, rows), generator=g, device=device))
                    for dp in cl.local(rank, "dp")}
    V, sql_kw = args.groups, {}
    if V:  # the DPs' tables (x, c1, c2); one search per cell of GROUP BY c1 [WHERE c2 = value]
        for cols in node.dp_data.values():
            cols += [torch.randint(0, V, (rows,), generator=g, device=device),
                     torch.randint(0, 4, (rows,), generator=g, device=device)]
        mine = [r for cols in node.dp_data.values() for r in torch.stack(cols, dim=1).cpu().tolist()]
        table = [r for part in comm.all_gather_object(mine) for r in part]
        keep = [r for r in table if passes_where(args, r[2])]
        want = [query.clear_cell([x for x, c1, _ in keep if c1 == c]) for c in range(V)]
        where = [] if args.where_value is None else [WhereClear("c2", str(args.where_value))]
        sql_kw = {"group_by": (V,), "sql": QuerySQL(Where=where, Predicate=args.predicate, GroupBy=["c1"])}
    else:
        want = query.clear(comm, [int(x) for cols in node.dp_data.values() for x in cols[0].cpu().tolist()])

    def right(v):
        """Is the decoded result the clear one (per cell with --groups: None stands for the NaN of an empty cell)?"""
        if not V:
            return int(round(v)) == want
        return len(v) == V and all((w is None and x != x) or (w is not None and x == x and int(round(x)) == w)
                                   for x, w in zip(v, want))

    client = DrynxClient(node, device=device) if rank == 0 else None
    classic = not args.no_classic and max(1, V) * N <= CLASSIC_MAX_RANGE
    names = [f"base={b}" for b in args.base_list] + (["classic"] if classic else [])
    thresholds = [1.0, 1.0, 1.0, 0.0, 1.0]
    templates, sig_s = {}, {}
    if rank == 0:
        for name in names:
            t0 = time.perf_counter()
            if name == "classic":
                templates[name] = make_survey(client, cl, op_name, query_min=0, query_max=N - 1, rows=rows, proofs=1,
                                              ranges=query.classic_ranges, thresholds=thresholds, sig_device=device,
                                              **sql_kw)
            else:
                kw = {} if query.ranges is None else {"ranges": query.ranges}
                templates[name] = make_iterative_survey(client, cl, op_name, int(name[5:]), query_min=0,
                                                        query_max=N - 1, rows=rows, proofs=1, thresholds=thresholds,
                                                        sig_device=device, **kw, **sql_kw)
            sig_s[name] = round(time.perf_counter() - t0, 3)

    def one_step(name):
        """-> (decoded value, [blocks], [ms per round]) on rank 0."""
        if name == "classic":
            if rank != 0:
                node.run_survey(None)
                return None
            sq = copy.copy(templates[name])
            sq.SurveyID = new_survey_id()
            _, vals, res = client.send_survey_query(sq)
            if V:
                return [query.classic_cell(v) for v in vals], [res.block], []
            return query.classic_value(vals), [res.block], []
        if rank != 0:
            serve_iterative(node)
            return None
        sq = copy.copy(templates[name])
        sq.SurveyID = new_survey_id()
        marks = [time.perf_counter()]
        value, rounds = query.search(client, sq, int(name[5:]), lambda *_: marks.append(time.perf_counter()))
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
                     "all_proofs_valid": ok, "result_ok": all(right(v) for v, _, _ in steps)})
    encoder = encoder_alone(args, query, device) if rank == 0 and device.type == "cuda" and world == 1 else None
    node.close(remove=True)
    if rank != 0:
        return
    out = {"tool": "bench_iter", "query": args.query, "range": N, "steps_per_run": args.steps, "n_gpus": world,
           "device": device.type, "order": [r["query"] for r in runs], **query.head(N, want),
           **({"groups": V, "where": args.where, "predicate": args.predicate} if V else {}),
           "config": {"cns": args.cns, "vns": args.vns, "dps": n_dps, "records_per_dp": rows,
                      "range_proof": query.range_proof, "sigs": "random (per CN, per column)",
                      "thresholds": [1, 1, 1, 0, 1]},
           **query.reference(N), "signature_setup_s": sig_s, "runs": runs, "queries": {}}
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
    if args.query == "max":
        ref = REFERENCE_MAX_ITERATIVE_S.get(N)
        out["below_reference_iterative"] = None if ref is None else it[best]["s_per_result"] < ref
    if classic:
        out["iterative_over_classic"] = round(it[best]["s_per_result"] / out["queries"]["classic"]["s_per_result"], 4)
    out["all_proofs_valid"] = all(q["all_proofs_valid"] for q in out["queries"].values())
    out["result_ok"] = all(q["result_ok"] for q in out["queries"].values())
    out["encoder"] = encoder
    print(json.dumps(out), flush=True)
    if args.out_dir:
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, f"range_{N}_groups_{V}.json" if V else f"range_{N}.json"), "w") as f:
            json.dump(out, f, indent=1)
    if not (out["all_proofs_valid"] and out["result_ok"]):
        sys.exit("bench_iter: a proof was rejected or a decoded result is wrong")


if __name__ == "__main__":
    main()
