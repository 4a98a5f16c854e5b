"""Iterative quantiles (digit-by-digit frequencyCount): the K14c rows against a
pure-Python model of the specification and the classic histogram, the argument
and validation rules, rank walks end to end (fixed and generated records, with
and without proofs, an inconsistent DP, no records), two gloo ranks through the
tool, and a runfile row.  The checks shared with the GPU suite live here and
take a device."""
import copy
import json
import os
import subprocess
import sys
from collections import Counter

import pytest
import torch

from drynx_amd import native as nt
from drynx_amd import query as Q
from drynx_amd import rounds
from drynx_amd.ops import encoding as enc
from drynx_amd.proofs import requests as prq
from drynx_amd.services.api import DrynxClient
from drynx_amd.services.local import local_cluster, make_iterative_survey, make_survey

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- the model (from the specification)
def model_rounds(R, b):
    L, p = 1, b
    while p < R:
        p *= b
        L += 1
    return L


def model_row(recs, qmin, qmax, b, L, k, prefix):
    c = Counter()
    for x in recs:
        if qmin <= x <= qmax:
            o = x - qmin
            if o // b ** (L - k) == prefix:
                c[(o // b ** (L - 1 - k)) % b] += 1
    return [c[i] for i in range(b)]


def nearest_rank(values, num, den):
    """The num/den nearest-rank (inverted-CDF) quantile of a non-empty list."""
    s = sorted(values)
    return s[max(1, (num * len(s) + den - 1) // den) - 1]


def model_walk(dps, qmin, qmax, b, num, den):
    """The digits D_0 .. D_{L-1} the querier's rank walk finds on the summed model rows."""
    L, prefix, out = model_rounds(qmax - qmin + 1, b), 0, []
    t = None
    for k in range(L):
        agg = [sum(col) for col in zip(*[model_row(r, qmin, qmax, b, L, k, prefix) for r in dps])]
        if k == 0:
            t = max(1, (num * sum(agg) + den - 1) // den)
        cum = 0
        for d, x in enumerate(agg):
            if cum + x >= t:
                break
            cum += x
        t -= cum
        out.append(d)
        prefix = prefix * b + d
    return out


SEG_ROWS = [0, 1, 63, 64, 65, 130, 0, 200]  # 0 .. 4 tiles of 64 rows, ragged ends, empty DPs first and in the middle
DOMAINS = [(-7, 1000, 10), (0, 1001, 10), (3, 4097, 16), (0, 1, 2), (0, 10 ** 6, 1000), (5, 5000, 4096)]  # (qmin, R, b)


def records_for(seg_rows, qmin, qmax, b, seed):
    """Per DP a list of records: uniform in the domain, but none with o div b == 1
    where that is neither QueryMin's nor QueryMax's block (a last-round prefix
    nobody matches); one record below the domain, one above it, one at QueryMin
    and one at QueryMax."""
    g = torch.Generator().manual_seed(seed)
    out = [torch.randint(qmin, qmax + 1, (n,), generator=g).tolist() for n in seg_rows]
    if (qmax - qmin) // b > 1:
        out = [[qmin if (x - qmin) // b == 1 else x for x in r] for r in out]
    full = [r for r in out if len(r) > 1]
    full[0][0] = qmin
    full[1][-1] = qmax
    full[2][len(full[2]) // 2] = qmin - 3
    full[3][-1] = qmax + 5
    return out


def check_rows(device, seg_rows=SEG_ROWS, domains=DOMAINS):
    """nt.iter_round == the model in every round (prefix = the median
    walk's digits), one prefix nobody matches, the last round against the
    classic histogram, round 0 against the in-domain counts; Z has two columns."""
    rows = []
    for n, (qmin, R, b) in enumerate(domains):
        qmax = qmin + R - 1
        dps = records_for(seg_rows, qmin, qmax, b, 23 + n)
        flat = [x for r in dps for x in r]
        assert min(flat) < qmin and max(flat) > qmax and qmin in flat and qmax in flat
        Z = torch.tensor([[x, -(1 << 62) if i % 2 else (1 << 62)] for i, x in enumerate(flat)],
                         dtype=torch.int64).reshape(-1, 2).to(device)
        L = model_rounds(R, b)
        assert Q.iter_rounds(qmin, qmax, b) == L
        digits = model_walk(dps, qmin, qmax, b, 1, 2)
        assert qmin + sum(d * b ** (L - 1 - k) for k, d in enumerate(digits)) == \
            nearest_rank([x for x in flat if qmin <= x <= qmax], 1, 2)
        classic = enc.batch_values("frequencyCount", Z, seg_rows, qmin, qmax).cpu()
        assert classic.shape == (len(seg_rows), R)
        prefix = 0
        for k in range(L):
            got = nt.iter_round("frequencyCount", Z, seg_rows, qmin, qmax, b, k, prefix)
            assert got.dtype == torch.int64 and got.shape == (len(seg_rows), b) and got.device == Z.device
            assert got.cpu().tolist() == [model_row(r, qmin, qmax, b, L, k, prefix) for r in dps]
            if k == 0:
                assert got.sum(1).cpu().tolist() == [sum(qmin <= x <= qmax for x in r) for r in dps]
            rows.append(got.cpu())
            if k < L - 1:
                prefix = prefix * b + digits[k]
        # the last round under the walk's prefix and under the last block of the domain (cut at R)
        for p in {prefix, (R - 1) // b}:
            got = nt.iter_round("frequencyCount", Z, seg_rows, qmin, qmax, b, L - 1, p).cpu()
            want = torch.zeros((len(seg_rows), b), dtype=torch.int64)
            cut = classic[:, p * b: p * b + b]
            want[:, : cut.shape[1]] = cut
            assert torch.equal(got, want)
            rows.append(got)
        if L > 1:  # a prefix no record matches: every row zero
            seen = {(x - qmin) // b for x in flat if qmin <= x <= qmax}
            miss = next(p for p in range(b ** (L - 1)) if p not in seen)
            got = nt.iter_round("frequencyCount", Z, seg_rows, qmin, qmax, b, L - 1, miss).cpu().tolist()
            assert got == [[0] * b for _ in seg_rows]
            assert got == [model_row(r, qmin, qmax, b, L, L - 1, miss) for r in dps]
    return rows


LARGE = (0, 10 ** 6, 1000, 70_000)  # qmin, R, b, rows of the one DP


def check_large(device):
    """One DP of 70000 rows at b = 1000: 68 tiles of 1024 rows and a ragged one of
    368; uniform records, then every record equal (one bin holds 70000)."""
    qmin, R, b, n = LARGE
    qmax = qmin + R - 1
    plan, first = nt._tile_plan(torch.tensor([n]).numpy(), b)
    assert (plan[:, 2] - plan[:, 1]).tolist() == [1024] * 68 + [368] and first.tolist() == [0, 69]
    L = model_rounds(R, b)
    g = torch.Generator().manual_seed(3)
    out = []
    for recs in (torch.randint(qmin, qmax + 1, (n,), generator=g).tolist(), [123_456] * n):
        Z = torch.tensor(recs, dtype=torch.int64)[:, None].to(device)
        digits = model_walk([recs], qmin, qmax, b, 1, 2)
        prefix = 0
        for k in range(L):
            got = nt.iter_round("frequencyCount", Z, [n], qmin, qmax, b, k, prefix).cpu()
            assert got.tolist() == [model_row(recs, qmin, qmax, b, L, k, prefix)] and int(got.sum()) > 0
            out.append(got)
            prefix = prefix * b + digits[k]
        assert qmin + prefix == nearest_rank(recs, 1, 2)
    assert out[2][0, 123] == n and out[3][0, 456] == n  # the contention case: every record in one bin
    return out


def test_rows_equal_the_model():
    check_rows("cpu")


def test_one_large_dp():
    check_large("cpu")


def test_rows_argument_checks():
    Z = torch.zeros((3, 1), dtype=torch.int64)
    for bad in (dict(base=1), dict(base=4097), dict(rnd=3), dict(rnd=-1), dict(prefix=10, rnd=1),
                dict(prefix=1, rnd=0), dict(qmax=1 << 40), dict(seg=[2])):
        a = dict(seg=[3], qmin=0, qmax=999, base=10, rnd=0, prefix=0)
        a.update(bad)
        with pytest.raises(ValueError):
            nt.iter_round("frequencyCount", Z, a["seg"], a["qmin"], a["qmax"], a["base"], a["rnd"], a["prefix"])
    assert nt.iter_round("frequencyCount", Z[:0], [], 0, 9, 10, 0, 0).shape == (0, 10)
    assert nt.iter_round("frequencyCount", Z, [3], 0, (1 << 40) - 1, 4096, 3, 4096 ** 3 - 1).tolist() == [[0] * 4096]
    assert (rounds.ITER_MAX_HIST_BASE, rounds.ITER_MAX_RANGE) == (4096, 1 << 40)


def test_entry_refuses_what_the_binding_refuses():
    """The C entry's own checks (-2), called below the binding: one rule for counts (kind 2), min (0) and max (1)."""
    Z = torch.zeros((3, 1), dtype=torch.int64)
    tiles = torch.tensor([0, 0, 3, 0, 1], dtype=torch.int64)  # one tile, then dp_first
    part, out = torch.empty((1, 8192), dtype=torch.int64), torch.empty((1, 8192), dtype=torch.int64)

    def rc(kind=2, qmin=0, qmax=999, base=10, lo=100, prefix=0, tl=tiles, G=1):
        return nt._raw_call("dx_iter_round", 0, None, nt._ptr(Z), 1, nt._ptr(tl[:3]), 1, nt._ptr(tl[3:]), G, kind,
                            qmin, qmax, base, lo, prefix, nt._ptr(part), nt._ptr(out))

    assert rc() == 0 and out[0, :10].tolist() == [3] + [0] * 9
    assert rc(lo=1, prefix=99) == 0
    assert rc(base=1, lo=1) == -2 and rc(base=4097, lo=1) == -2
    assert rc(qmax=1 << 40) == -2 and rc(qmax=-1) == -2
    assert rc(lo=1000) == -2 and rc(lo=0) == -2 and rc(lo=50) == -2  # no round of the domain
    assert rc(prefix=1) == -2 and rc(prefix=-1) == -2 and rc(lo=1, prefix=100) == -2
    long = torch.tensor([0, 0, 1 << 31, 0, 1], dtype=torch.int64)
    assert rc(tl=long) == -2  # a tile of 2^31 rows: the 32-bit counters could wrap
    for kind, row in ((0, [1] * 10), (1, [0] * 10)):  # three records 0: the digit 0 in unary, [i >= 0] and [i < 0]
        assert rc(kind) == 0 and out[0, :10].tolist() == row
        assert rc(kind, lo=1, prefix=99) == 0
        assert rc(kind, base=1, lo=1) == -2 and rc(kind, base=65537, lo=1) == -2
        assert rc(kind, qmax=1 << 40) == -2 and rc(kind, qmax=-1) == -2
        assert rc(kind, lo=1000) == -2 and rc(kind, lo=0) == -2 and rc(kind, lo=50) == -2
        assert rc(kind, prefix=1) == -2 and rc(kind, prefix=-1) == -2 and rc(kind, lo=1, prefix=100) == -2
    assert rc(1, base=4097, lo=1) == 0 and out[0, :4097].tolist() == [0] * 4097  # the cap is the kind's
    assert rc(3) == -2 and rc(-1) == -2
    # the tile length limits the 32-bit counters only; checked before anything is read (no DP: no row is)
    assert rc(2, tl=long, G=0) == -2 and rc(1, tl=long, G=0) == 0


# ----------------------------------------------------------------------------- validation
@pytest.fixture(scope="module")
def env(tmp_path_factory):
    cl, node = local_cluster(3, 5, 3, device="cpu", workdir=str(tmp_path_factory.mktemp("db")))
    yield cl, node, DrynxClient(node)
    node.close(remove=True)


def _round(env, name="frequencyCount", base=10, qmin=0, qmax=99, k=0, prefix=0, proofs=0, ranges=None):
    cl, node, client = env
    kw = dict(ranges=ranges) if name == "frequencyCount" else {}
    sq = make_iterative_survey(client, cl, name, base, query_min=qmin, query_max=qmax, rows=4, proofs=proofs, **kw)
    return client.iterative_round_query(sq, base, k, prefix, "it")


def test_check_parameters_limits(env):
    ok = _round(env)
    assert Q.check_parameters(ok, False)
    assert (ok.Query.Operation.NbrInput, ok.Query.Operation.NbrOutput, ok.SurveyID) == (1, 10, "it.r0")
    assert Q.check_parameters(_round(env, qmin=-5, qmax=94, k=1, prefix=9), False)
    pr = _round(env, proofs=1, ranges=[16, 2])
    assert Q.check_parameters(pr, False)
    assert pr.Query.Ranges == [[16, 2]] * 10 and all(len(r) == 10 for r in pr.Query.IVSigs.InputValidationSigs)
    assert Q.check_parameters(_round(env, base=4096, qmax=9999), False)

    def refused(sq0=ok, **kw):
        sq = copy.deepcopy(sq0)
        for k, v in kw.items():
            obj, _, attr = k.rpartition("__")
            tgt = sq
            for part in filter(None, obj.split("__")):
                tgt = getattr(tgt, part)
            setattr(tgt, attr, v)
        return not Q.check_parameters(sq, Q.add_diff_p(sq.Query.DiffP))

    assert not refused()
    assert refused(IterBase=4097, Query__Operation__NbrOutput=4097) and refused(IterBase=1) and refused(IterBase=-10)
    assert refused(Query__CuttingFactor=2)
    assert refused(Query__DiffP=Q.QueryDiffP(LapMean=0.0, LapScale=1.0, NoiseListSize=8, Quanta=1.0, Scale=1.0,
                                             Limit=3))
    assert refused(IterRound=2) and refused(IterRound=-1)            # L = 2 for 100 values in base 10
    assert refused(IterPrefix=1) and refused(IterRound=1, IterPrefix=10) and refused(IterPrefix=-1)
    assert not refused(IterRound=1, IterPrefix=9)
    assert refused(Query__Operation__NbrOutput=100) and refused(Query__Operation__NbrOutput=9)
    big = copy.deepcopy(ok)  # R = 2^40 + 1
    big.Query.Operation.QueryMax = big.Query.DPDataGen.GenerateDataMax = 1 << 40
    assert not Q.check_parameters(big, False)
    # with proofs: one range per output, (0, 0) for all of them or for none
    assert refused(pr, Query__Ranges=[[16, 2]] * 9)
    assert refused(pr, Query__Ranges=[[16, 2]] * 9 + [[0, 0]])
    assert not refused(pr, Query__Ranges=[[16, 2]] * 9 + [[4, 4]])
    # min/max keep their rules, the other operations stay refused
    assert Q.ITER_MAX_HIST_BASE == 4096 and Q.ITER_MAX_BASE == 65536
    assert Q.check_parameters(_round(env, "max", 65536, 0, 10 ** 6), False)
    assert refused(_round(env, "max", 10, proofs=1), Query__Ranges=[[16, 2]] * 10)
    assert refused(Query__Operation__NameOp="sum") and refused(Query__Operation__NameOp="union")
    with pytest.raises(ValueError):
        Q.iter_operation("sum", 0, 9, 10)
    assert Q.iter_operation("frequencyCount", -3, 96, 10) == Q.Operation("frequencyCount", 1, 10, -3, 96)
    with pytest.raises(ValueError):
        make_iterative_survey(env[2], env[0], "frequencyCount", 10, query_min=0, query_max=99, proofs=1)


# ----------------------------------------------------------------------------- searches end to end
FIXED = [[20, 37, 99], [99, 5], [], [98, 98, 1], [99]]  # ties, an empty DP, records at QueryMax
QUANTILES = [(0, 1), (1, 4), (1, 2), (3, 4), (1, 1)]


def fixed_data(cl, lists, lo=0):
    return {dp.id: [torch.tensor([x + lo for x in lists[i]], dtype=torch.int64)] for i, dp in enumerate(cl.dps)}


def check_search_fixed(cl, node, client, device, qmin, qmax, base):
    """Every quantile of QUANTILES over the fixed records against the sorted list; 0/1 and 1/1 against the
    iterative min and max."""
    span = qmax - qmin
    lists = [[x * span // 99 for x in r] for r in FIXED]
    flat = [x + qmin for r in lists for x in r]
    L = Q.iter_rounds(qmin, qmax, base)
    node.dp_data = {k: [c.to(device) for c in v] for k, v in fixed_data(cl, lists, qmin).items()}
    try:
        sq = make_survey(client, cl, "frequencyCount", query_min=qmin, query_max=qmax, rows=3)
        for num, den in QUANTILES:
            seen = []
            value, rounds = client.send_iterative_quantile(sq, base, num, den,
                                                           on_round=lambda k, d, r: seen.append((k, d)))
            assert value == float(nearest_rank(flat, num, den)), (num, den)
            assert len(rounds) == L and [k for k, _ in seen] == list(range(L))
            assert qmin + sum(d * base ** (L - 1 - k) for k, d in seen) == value
            assert [r.survey_id for r in rounds] == [f"{sq.SurveyID}.r{k}" for k in range(L)]
            assert all(r.n_out == base and r.block is None for r in rounds)
            assert sum(rounds[0].client_out[0]) == len(flat) and len(rounds[0].client_out[0]) == base
            if (num, den) in ((0, 1), (1, 1)):
                name = "min" if num == 0 else "max"
                ext, _ = client.send_iterative_extreme(
                    make_survey(client, cl, name, query_min=qmin, query_max=qmax, rows=3), base)
                assert ext == value == float(min(flat) if num == 0 else max(flat))
    finally:
        node.dp_data = {}


def check_search_generated(cl, node, client, qmin, qmax, base):
    """Generated records (no dp_data): every round must draw the same ones."""
    from drynx_amd.protocols.data_collection import _seed

    for num, den in ((1, 2), (9, 10)):
        sq = make_iterative_survey(client, cl, "frequencyCount", base, query_min=qmin, query_max=qmax, rows=6)
        value, rounds = client.send_iterative_quantile(sq, base, num, den)
        # the DPs' records, redrawn here from the shared id as the DPs draw them
        recs = []
        for dp in cl.dps:
            gen = torch.Generator().manual_seed(_seed(sq.SurveyID, dp.id))
            recs += torch.randint(qmin, qmax + 1, (1, 6), generator=gen, dtype=torch.int64)[0].tolist()
        assert value == float(nearest_rank(recs, num, den))
        assert len(rounds) == Q.iter_rounds(qmin, qmax, base) and sum(rounds[0].client_out[0]) == len(recs)


def check_search_with_proofs(cl, node, client, device, qmax, base):
    """(16, 2) proofs and 3 VNs: one block per round, every code PROOF_TRUE, 5 + 3 + 3 stored proofs per round id."""
    lists = [[x * qmax // 99 for x in r] for r in FIXED]
    node.dp_data = {k: [c.to(device) for c in v] for k, v in fixed_data(cl, lists).items()}
    try:
        sq = make_iterative_survey(client, cl, "frequencyCount", base, query_min=0, query_max=qmax, rows=3, proofs=1,
                                   ranges=[16, 2], sig_device=device)
        value, rounds = client.send_iterative_quantile(sq, base, 1, 2)
    finally:
        node.dp_data = {}
    L = Q.iter_rounds(0, qmax, base)
    assert value == float(nearest_rank([x for r in lists for x in r], 1, 2))
    assert len(rounds) == L and len({r.block.Hash for r in rounds}) == L
    for k, r in enumerate(rounds):
        codes = r.block.data_block().Proofs
        assert set(codes.values()) == {prq.PROOF_TRUE} and len(codes) == 3 * (5 + 3 + 3)
        assert r.survey_id == f"{sq.SurveyID}.r{k}"
        proofs = client.send_get_proofs("vn0", r.survey_id)
        assert len(proofs) == 5 + 3 + 3 and all(p.startswith(r.survey_id + "/") for p in proofs)
        if k:
            assert r.block.BackLink == rounds[k - 1].block.Hash
    return rounds


def test_search_fixed_records(env):
    cl, node, client = env
    check_search_fixed(cl, node, client, "cpu", 0, 99, 10)
    check_search_fixed(cl, node, client, "cpu", -40, 59, 10)


def test_search_generated_records(env):
    cl, node, client = env
    check_search_generated(cl, node, client, 0, 99, 10)


def test_search_with_proofs(env):
    cl, node, client = env
    check_search_with_proofs(cl, node, client, "cpu", 99, 10)


def test_inconsistent_dp_raises(env):
    cl, node, client = env
    node.dp_data = fixed_data(cl, [[20, 37], [35, 50], [], [41], [64]])

    def swap(k, digit, res):
        if k == 0:  # median 37: two records under the prefix 3; afterwards only one
            assert digit == 3 and res.client_out[0][3] == 2
            node.dp_data = fixed_data(cl, [[20, 77], [35, 50], [], [41], [64]])

    try:
        sq = make_survey(client, cl, "frequencyCount", query_min=0, query_max=99, rows=3)
        with pytest.raises(RuntimeError, match="round 1.*changed between rounds"):
            client.send_iterative_quantile(sq, 10, 1, 2, on_round=swap)
    finally:
        node.dp_data = {}


def test_no_records_and_bad_quantiles(env):
    cl, node, client = env
    sq = make_survey(client, cl, "frequencyCount", query_min=3, query_max=102, rows=3)
    node.dp_data = fixed_data(cl, [[], [2], [], [103, 500], []])  # nothing inside the domain
    try:
        with pytest.raises(RuntimeError, match="no records"):
            client.send_iterative_quantile(sq, 10, 1, 2)
    finally:
        node.dp_data = {}
    for num, den in ((2, 1), (-1, 2), (1, 0)):
        with pytest.raises(ValueError):
            client.send_iterative_quantile(sq, 10, num, den)
    with pytest.raises(ValueError):
        client.send_iterative_quantile(make_survey(client, cl, "max", query_min=0, query_max=99, rows=3), 10, 1, 2)


def test_per_dp_encoder_matches_the_batch(env):
    """dp_encode (one DP at a time) sends the values dp_encode_batch does: integer counts."""
    from drynx_amd.protocols import data_collection as dcp

    cl, node, client = env
    lists = [[20, 37, 37], [35, 50], [], [41, 120, -1], [64]]
    node.dp_data = fixed_data(cl, lists)
    try:
        for k, prefix in ((0, 0), (1, 3), (1, 9)):
            sq = client.iterative_round_query(make_survey(client, cl, "frequencyCount", query_min=0, query_max=99,
                                                          rows=3), 10, k, prefix, "enc")
            batch = dcp.dp_encode_batch(node, sq, cl.dps)
            for i, dp in enumerate(cl.dps):
                one = dcp.dp_encode(node, sq, dp, sync_timer=False)
                assert one["clear"] == batch[dp.id]["clear"] == [model_row(lists[i], 0, 99, 10, 2, k, prefix)]
                assert len(one["cv"]) == len(batch[dp.id]["cv"]) == 10
        assert batch[cl.dps[0].id]["clear"] == [[0] * 10] and one["clear"] == [[0] * 10]
        sq = client.iterative_round_query(make_survey(client, cl, "frequencyCount", query_min=0, query_max=99, rows=3),
                                          10, 1, 3, "enc")
        assert dcp.dp_encode_batch(node, sq, cl.dps)[cl.dps[0].id]["clear"] == [[0, 0, 0, 0, 0, 0, 0, 2, 0, 0]]
    finally:
        node.dp_data = {}


# ----------------------------------------------------------------------------- two ranks, simulation
def test_two_gloo_ranks_through_the_tool(tmp_path):
    env_ = dict(os.environ, OMP_NUM_THREADS="4", DX_NUM_THREADS="4")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_iter.py"), "--query", "quantile", "--gpus",
                        "2", "--range", "1000", "--bases", "10", "--steps", "1", "--passes", "1", "--device", "cpu",
                        "--no-classic", "--out-dir", str(tmp_path)], cwd=ROOT, env=env_, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert line["result_ok"] and line["all_proofs_valid"] and line["n_gpus"] == 2
    assert line["queries"]["base=10"]["rounds"] == 3 and line["runs"][0]["blocks_per_result"] == 3
    assert json.load(open(tmp_path / "range_1000.json"))["clear_quantile"] == line["clear_quantile"]


def test_simul_runfile_column(tmp_path, monkeypatch):
    from drynx_amd.parallel.comm import LocalComm
    from drynx_amd.simul import simul

    seen = []
    send = DrynxClient.send_iterative_quantile

    def recording(self, sq, base, num, den, on_round=None):
        from drynx_amd.protocols.data_collection import _seed

        value, rounds = send(self, sq, base, num, den, on_round)
        recs = []  # each row runs on records of its own (a fresh survey id): redrawn as the DPs draw them
        for dp in sq.all_dps():
            gen = torch.Generator().manual_seed(_seed(sq.SurveyID, dp.id))
            recs += torch.randint(0, 1000, (1, 5), generator=gen, dtype=torch.int64)[0].tolist()
        seen.append((base, num, den, len(rounds), rounds[0].n_out, value, sum(rounds[0].client_out[0]),
                     float(nearest_rank(recs, num, den))))
        return value, rounds

    monkeypatch.setattr(DrynxClient, "send_iterative_quantile", recording)
    row = {"NbrServers": 2, "NbrDPs": 4, "NbrVNs": 0, "Proofs": 0, "OperationName": "frequencyCount", "MinData": 0,
           "MaxData": 999, "DPRows": 5, "IterBase": 10}
    glob, rows = simul.parse_runfile("Rounds = 1\n\nNbrServers, NbrDPs, NbrVNs, Proofs, OperationName, MinData, "
                                     "MaxData, DPRows, IterBase, IterQuantile\n"
                                     "2, 4, 0, 0, frequencyCount, 0, 999, 5, 10, 3/4\n")
    assert rows[0]["IterQuantile"] == "3/4" and rows[0]["IterBase"] == 10
    q3 = simul.run_row(glob, rows[0], LocalComm("cpu"), "cpu", str(tmp_path / "a"), netem="off")
    med = simul.run_row({"Rounds": 1}, row, LocalComm("cpu"), "cpu", str(tmp_path / "b"), netem="off")
    assert [s[:5] for s in seen] == [(10, 3, 4, 3, 10), (10, 1, 2, 3, 10)] and all(s[6] == 20 for s in seen)
    assert q3 == [[seen[0][5]]] and med == [[seen[1][5]]] and all(s[5] == s[7] for s in seen)
