"""The k-means encoder (K14f) alone, and one full verifiable k-means run.

Encoder alone (GPU only): 10 DPs x 100000 records of 32 columns, uniform in
[0, 1000), scale 4.  For k in {4, 16, 64} and d in {2, 8, 32} one call of
``native.kmeans_round`` on the first d columns (centroids drawn by
``kmeans.random_centroids``) alternates, in one process, with one call of
``native.int_moments`` on the same columns with the ``lin_reg`` pair list -- the
nearest existing streaming kernel over the same records, a yardstick and not
a competitor: it multiplies d (d + 1) / 2 + d + 1 column pairs per row, the
k-means round k * d differences per row.  Both calls include their one upload
(the tile plan; the centroids or the pairs).  A window is ``--encoder-iters``
calls between two device events after a warm-up, three windows per call and
shape; the device result is compared with the host twin outside the windows.

Full run: 3 CNs, 3 VNs, 10 DPs with ``--rows`` generated records each (default
100) over [0, 99], k = 4, d = 2, scale 4, 5 rounds, (16, l) range proofs on
every output with the smallest l that holds a DP's largest sum of squares,
random per-CN per-column signatures, thresholds [1, 1, 1, 0, 1].  One warm-up
run (which builds the prover and verifier tables), then ``--steps`` timed runs
(``DrynxClient.send_kmeans``) on a host clock that ends in a device
synchronise.  Outside the timed region every round's block is checked (all
proofs valid) and the result is compared with ``kmeans.round_model`` and
``kmeans.update`` run on the redrawn records.

Prints one JSON object; ``--out-dir`` also writes it as kmeans.json.
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

from drynx_amd import kmeans as km  # noqa: E402
from drynx_amd import native as nt  # noqa: E402
from drynx_amd.ops import encoding as enc  # noqa: E402
from drynx_amd.protocols.data_collection import _seed  # noqa: E402
from drynx_amd.query import new_survey_id  # noqa: E402
from drynx_amd.services.api import DrynxClient  # noqa: E402
from drynx_amd.services.local import local_cluster, make_kmeans_survey  # noqa: E402

ENCODER_K, ENCODER_D = (4, 16, 64), (2, 8, 32)
RUN = dict(k=4, d=2, scale=4, rounds=5, qmin=0, qmax=99)


def encoder_alone(iters: int, device) -> dict:
    """ms per call (device events) of the k-means round and of the lin_reg moments, by shape."""
    g = torch.Generator(device=device).manual_seed(7)
    rows, qmin, qmax, scale = [100_000] * 10, 0, 999, 4
    Zall = torch.randint(qmin, qmax + 1, (sum(rows), 32), generator=g, device=device)
    out = {"records": "10 DPs x 100000, 32 int64 columns, uniform in [0, 1000)", "scale": scale,
           "calls_per_window": iters, "windows": 3,
           "what": "kmeans = native.kmeans_round on the first d columns; lin_reg_moments = native.int_moments on "
                   "the same columns with the lin_reg pair list (yardstick only); both with their upload",
           "ms_per_call": {}, "equals_host_twin": True}
    for d in ENCODER_D:
        Zd = Zall[:, :d].contiguous()
        pairs = enc.moment_pairs("lin_reg", d)
        for k in ENCODER_K:
            cen = km.random_centroids(k, d, qmax - qmin + 1, scale, f"bench {k} {d}")
            calls = {"kmeans": lambda: nt.kmeans_round(Zall[:, :d], rows, d, k, qmin, qmax, scale, cen),
                     "lin_reg_moments": lambda: nt.int_moments(Zd, rows, pairs)}
            ms = {name: [] for name in calls}
            for f in calls.values():
                for _ in range(5):
                    f()
            for _ in range(3):
                for name, f in calls.items():
                    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize(device)
                    a.record()
                    for _ in range(iters):
                        f()
                    e.record()
                    torch.cuda.synchronize(device)
                    ms[name].append(round(a.elapsed_time(e) / iters, 5))
            # outside the windows: the device rows are the host twin's
            host = nt.kmeans_round(Zall[:, :d].cpu(), rows, d, k, qmin, qmax, scale, cen)
            if not torch.equal(calls["kmeans"]().cpu(), host):
                out["equals_host_twin"] = False
            out["ms_per_call"][f"k={k},d={d}"] = dict(ms, outputs_per_dp=k * (d + 2), moment_pairs=len(pairs))
    return out


def full_run(args, device) -> dict:
    k, d, S, rounds, qmin, qmax = (RUN[n] for n in ("k", "d", "scale", "rounds", "qmin", "qmax"))
    n_dps, rows = 10, args.rows
    cl, node = local_cluster(3, n_dps, 3, device=device, workdir=tempfile.mkdtemp(prefix="drynx_kmeans_"))
    client = DrynxClient(node, device=device)
    top, l = rows * d * (qmax - qmin) ** 2, 1  # a DP's largest output: its sum of squares
    while 16 ** l <= top:
        l += 1
    t0 = time.perf_counter()
    template = make_kmeans_survey(client, cl, k, d, S, rounds, query_min=qmin, query_max=qmax, rows=rows, proofs=1,
                                  ranges=[16, l], thresholds=[1.0, 1.0, 1.0, 0.0, 1.0], sig_device=device)
    sig_s = time.perf_counter() - t0
    start = km.random_centroids(k, d, qmax - qmin + 1, S, "bench")

    def model(search_id):
        recs = []
        for dp in cl.dps:  # redrawn from the id the rounds share, as the DPs draw them
            gen = torch.Generator().manual_seed(_seed(search_id, dp.id))
            recs += torch.randint(qmin, qmax + 1, (d, rows), generator=gen, dtype=torch.int64).t().tolist()
        cur = list(start)
        for _ in range(rounds):
            answer = km.round_model(recs, k, d, qmin, qmax, S, cur)
            cur = km.update(cur, answer, k, d, S)
        return cur, km.split(answer, k, d)[0]

    def one_run():
        sq = copy.copy(template)
        sq.SurveyID = new_survey_id()
        marks = [time.perf_counter()]
        res = client.send_kmeans(sq, start, on_round=lambda *_: marks.append(time.perf_counter()))
        return sq.SurveyID, res, [round(1000 * (b - a), 2) for a, b in zip(marks, marks[1:])]

    def sync():
        if torch.device(device).type == "cuda":
            torch.cuda.synchronize()

    t0 = time.perf_counter()
    one_run()  # warm-up: the run's tables, warm clocks
    first_s = time.perf_counter() - t0
    node.flush_stores()
    sync()
    t0 = time.perf_counter()
    steps = [one_run() for _ in range(args.steps)]
    node.flush_stores()
    sync()
    elapsed = time.perf_counter() - t0
    # outside the timed region
    blocks = [r.block for _, res, _ in steps for r in res.rounds]
    ok = all(b is not None and all(v == 1 for v in b.data_block().Proofs.values()) for b in blocks)
    right = all((res.centroids, res.counts) == model(sid) for sid, res, _ in steps)
    per_round = [ms for _, _, rms in steps for ms in rms]
    node.close(remove=True)
    return {"config": {"cns": 3, "vns": 3, "dps": n_dps, "records_per_dp": rows, "domain": [qmin, qmax], **RUN,
                       "outputs_per_dp_and_round": k * (d + 2), "range_proof": f"(16, {l}) on every output",
                       "sigs": "random (per CN, per column)", "thresholds": [1, 1, 1, 0, 1]},
            "steps": args.steps, "signature_setup_s": round(sig_s, 3), "first_s": round(first_s, 3),
            "s_per_run": round(elapsed / args.steps, 5), "ms_per_round": round(sum(per_round) / len(per_round), 2),
            "round_ms": [rms for _, _, rms in steps], "blocks_per_run": rounds,
            "converged_at": [res.converged_at for _, res, _ in steps], "all_proofs_valid": ok, "result_ok": right}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--device", default=None)
    ap.add_argument("--rows", type=int, default=100, help="records per DP of the full run")
    ap.add_argument("--steps", type=int, default=3, help="timed full runs")
    ap.add_argument("--encoder-iters", type=int, default=100, help="encoder calls per timed window (GPU only)")
    ap.add_argument("--no-run", action="store_true", help="skip the full run")
    ap.add_argument("--out-dir", default=None, help="write kmeans.json here")
    args = ap.parse_args()
    if args.rows < 1 or args.steps < 1 or args.encoder_iters < 1:
        ap.error("--rows, --steps and --encoder-iters at least 1")
    device = torch.device(args.device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
    if device.type == "cuda":
        torch.cuda.set_device(device)
    out = {"tool": "bench_kmeans", "device": device.type,
           "device_name": torch.cuda.get_device_name(device) if device.type == "cuda" else None,
           # no time is taken without a GPU: a host timing says nothing about the kernel
           "encoder": encoder_alone(args.encoder_iters, device) if device.type == "cuda" else None,
           "run": None if args.no_run else full_run(args, device)}
    print(json.dumps(out), flush=True)
    if args.out_dir:
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, "kmeans.json"), "w") as f:
            json.dump(out, f, indent=1)
    bad = (out["run"] is not None and not (out["run"]["all_proofs_valid"] and out["run"]["result_ok"])) \
        or (out["encoder"] is not None and not out["encoder"]["equals_host_twin"])
    if bad:
        sys.exit("bench_kmeans: a proof was rejected, a result is wrong or the device differs from its host twin")


if __name__ == "__main__":
    main()
