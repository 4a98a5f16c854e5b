"""Iterative (digit-by-digit) min/max: the K14b rows against a pure-Python model
of the protocol, the validation rules and both carriers of the four query
fields, searches end to end (with and without proofs, fixed and generated
records, an inconsistent DP), two gloo ranks through the tool, and a runfile
row.  The checks shared with the GPU suite live here and take a device."""
import copy
import json
import os
import subprocess
import sys

import pytest
import torch

from drynx_amd import native as nt
from drynx_amd import query as Q
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


def model_row(recs, is_max, qmin, qmax, b, L, k, prefix):
    v = 0 if is_max else b
    if recs:
        o = min(max(max(recs) if is_max else min(recs), qmin), qmax) - qmin
        if o // b ** (L - k) == prefix:
            v = (o // b ** (L - 1 - k)) % b
    return [int(i < v) if is_max else int(i >= v) for i in range(b)]


def model_digits(dps, is_max, qmin, qmax, b):
    """The global digits D_0 .. D_{L-1} the querier finds, round by round."""
    L, prefix, out = model_rounds(qmax - qmin + 1, b), 0, []
    for k in range(L):
        agg = [sum(col) for col in zip(*[model_row(r, is_max, qmin, qmax, b, L, k, prefix) for r in dps])]
        d = next(i for i, a in enumerate(agg) if (a == 0) == is_max)
        out.append(d)
        prefix = prefix * b + d
    return out


SEG_ROWS = [0, 1, 63, 64, 65, 130, 0, 200]  # 0 .. 4 tiles of 64 rows, ragged ends, empty DPs first and in the middle
DOMAINS = [(-7, 1000, 10), (0, 1001, 10), (3, 4097, 16), (0, 1, 2), (0, 10 ** 6, 1000)]  # (qmin, R, b)


def records_for(seg_rows, qmin, qmax, seed, outside=True):
    """Per DP a list of records in the domain; with ``outside`` the third DP with
    records also has one below it and the fourth one above it (they clamp)."""
    g = torch.Generator().manual_seed(seed)
    out = [torch.randint(qmin, qmax + 1, (n,), generator=g).tolist() for n in seg_rows]
    full = [r for r in out if r]
    if not outside:
        return out
    below, above = full[2 % len(full)], full[3 % len(full)]  # (with fewer than four DPs with records: two others)
    below[len(below) // 2] = qmin - 3
    above[-1] = qmax + 5
    return out


def check_rows(device, seg_rows=SEG_ROWS, domains=DOMAINS):
    """nt.iter_round == the model, both modes, every round (prefix = the
    model's global digits), one prefix nobody matches; Z has two columns."""
    host = []
    for n, (qmin, R, b) in enumerate(domains):
        qmax = qmin + R - 1
        dps = records_for(seg_rows, qmin, qmax, 11 + n, outside=n % 2 == 0)  # every other domain clamps
        assert (n % 2 == 1) != (any(x < qmin for r in dps for x in r) and any(x > qmax for r in dps for x in r))
        flat = [x for r in dps for x in r]
        Z = torch.tensor([[x, -(1 << 62) if i % 2 else (1 << 62)] for i, x in enumerate(flat)],
                         dtype=torch.int64).reshape(-1, 2).to(device)
        L = model_rounds(R, b)
        assert Q.iter_rounds(qmin, qmax, b) == L
        for name in ("max", "min"):
            is_max = name == "max"
            digits = model_digits(dps, is_max, qmin, qmax, b)
            assert qmin + sum(d * b ** (L - 1 - k) for k, d in enumerate(digits)) == \
                min(max((max if is_max else min)(flat), qmin), qmax)
            prefix = 0
            for k in range(L):
                got = nt.iter_round(name, Z, seg_rows, qmin, qmax, b, k, prefix)
                assert got.dtype == torch.int64 and got.shape == (len(seg_rows), b) and got.device == Z.device
                assert got.cpu().tolist() == [model_row(r, is_max, qmin, qmax, b, L, k, prefix) for r in dps]
                host.append(got.cpu())
                prefix = prefix * b + digits[k]
            if L > 1:  # a prefix no DP matches: every row neutral
                os_ = {min(max((max if is_max else min)(r), qmin), qmax) - qmin for r in dps if r}
                miss = next(p for p in range(b) if all(o // b ** (L - 1) != p for o in os_))
                got = nt.iter_round(name, Z, seg_rows, qmin, qmax, b, 1, miss).cpu().tolist()
                assert got == [[0] * b for _ in seg_rows]  # [i < 0] and [i >= b] alike
                assert got == [model_row(r, is_max, qmin, qmax, b, L, 1, miss) for r in dps]
    return host


def test_rows_equal_the_model():
    check_rows("cpu")


WIDEST = dict(seg_rows=[0, 3, 70], domains=[(-5, 65537, 65536)])  # the cap of the min/max base: L = 2, 65536-wide rows


def test_rows_at_the_widest_base():
    assert len(check_rows("cpu", **WIDEST)) == 4


def test_rows_argument_checks():
    Z = torch.zeros((3, 1), dtype=torch.int64)
    for bad in (dict(base=1), dict(base=65537), dict(rnd=3), dict(rnd=-1), dict(prefix=10, rnd=1),
                dict(prefix=1, rnd=0), dict(qmax=1 << 40), dict(seg=[2])):
        a = dict(seg=[3], qmin=0, qmax=999, base=10, rnd=0, prefix=0)
        a.update(bad)
        with pytest.raises(ValueError):
            nt.iter_round("max", Z, a["seg"], a["qmin"], a["qmax"], a["base"], a["rnd"], a["prefix"])
    assert nt.iter_round("max", Z[:0], [], 0, 9, 10, 0, 0).shape == (0, 10)


# ----------------------------------------------------------------------------- validation and carriers
@pytest.fixture(scope="module")
def env(tmp_path_factory):
    cl, node = local_cluster(3, 5, 3, device="cpu", workdir=str(tmp_path_factory.mktemp("db")))
    yield cl, node, DrynxClient(node)
    node.close(remove=True)


def _round(env, name="max", base=10, qmin=0, qmax=99, k=0, prefix=0, proofs=0):
    cl, node, client = env
    sq = make_iterative_survey(client, cl, name, base, query_min=qmin, query_max=qmax, rows=4, proofs=proofs)
    return client.iterative_round_query(sq, base, k, prefix, "it")


def test_check_parameters_limits(env):
    cl, node, client = env
    ok = _round(env)
    assert Q.check_parameters(ok, False)
    assert Q.check_parameters(_round(env, "min", 10, -5, 94, 1, 9), False)
    assert Q.check_parameters(_round(env, proofs=1), False)

    def refused(**kw):
        sq = copy.deepcopy(ok)
        for k, v in kw.items():
            obj, _, attr = k.rpartition("__")
            tgt = sq
            for part in filter(None, obj.split("__")):
                tgt = getattr(tgt, part)
            setattr(tgt, attr, v)
        return not Q.check_parameters(sq, Q.add_diff_p(sq.Query.DiffP))

    assert refused(IterBase=1) and refused(IterBase=65537) and refused(IterBase=-10)
    assert refused(Query__Operation__NameOp="union") and refused(Query__Operation__NameOp="sum")
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
    big.Query.Operation.QueryMax = big.Query.DPDataGen.GenerateDataMax = (1 << 40) - 1
    big.IterRound = 12  # L = 13 rounds of base 10 for 2^40 values
    assert Q.check_parameters(big, False)
    # the existing rule: the operation's domain is the DPs'
    assert refused(Query__Operation__QueryMax=98)
    # with proofs every range is (2, 1)
    pr = _round(env, proofs=1)
    assert len(pr.Query.Ranges) == 10 and all(len(r) == 10 for r in pr.Query.IVSigs.InputValidationSigs)
    pr.Query.Ranges = [[16, 2]] * 10
    assert not Q.check_parameters(pr, False)
    with pytest.raises(ValueError):
        Q.iter_rounds(0, 9, 1)
    with pytest.raises(ValueError):
        Q.iter_operation("sum", 0, 9, 10)
    assert [Q.iter_rounds(0, R - 1, b) for R, b in ((1, 2), (10, 10), (11, 10), (1000, 10), (1001, 10),
                                                  (10 ** 6, 1000), (1 << 40, 65536))] == [1, 1, 2, 3, 4, 2, 3]


def test_base_zero_is_the_classic_query(env):
    cl, node, client = env
    for kw in (dict(proofs=0), dict(proofs=1, ranges=[2, 1])):
        sq = make_survey(client, cl, "max", query_min=0, query_max=9, rows=4, **kw)
        assert (sq.IterBase, sq.IterRound, sq.IterPrefix, sq.IterSurveyID) == (0, 0, 0, "")
        assert Q.check_parameters(sq, False)
    sq.IterRound = 1  # round fields without a base
    assert not Q.check_parameters(sq, False)


def test_wire_and_dict_carry_the_fields(env):
    from drynx_amd.wire import messages as M
    from drynx_amd.wire import onet
    from drynx_amd.wire import protobuf as pb

    sq = _round(env, "min", 10, -5, 94, 1, 7, proofs=1)
    sq.IterSurveyID = "search-1"
    assert onet.SURVEY_QUERY_ITER[-5:] == (("LRTargets", "sint"), ("IterBase", "sint"), ("IterRound", "sint"),
                                           ("IterPrefix", "sint"), ("IterSurveyID", "string"))
    assert onet.MESSAGES["libdrynx.SurveyQuery"] is onet.SURVEY_QUERY_ITER
    for back in (M.survey_query_from_wire(M.survey_query_to_wire(sq)), Q.SurveyQuery.from_dict(sq.to_dict())):
        assert (back.IterBase, back.IterRound, back.IterPrefix, back.IterSurveyID) == (10, 1, 7, "search-1")
        assert back.SurveyID == sq.SurveyID and back.Query.Operation == sq.Query.Operation
        assert Q.check_parameters(back, False)
    # a sender without the extension: no such fields on the wire / in the dict -> the classic query
    classic = make_survey(env[2], env[0], "max", query_min=0, query_max=9, rows=4)
    msg = M.survey_query_to_msg(classic)
    old = onet.message_type_id("libdrynx.SurveyQuery") + pb.encode(onet.SURVEY_QUERY, msg)
    assert old == M.survey_query_to_wire(classic)  # IterBase = 0: not a byte more than before
    dec = M.survey_query_from_wire(old)
    assert (dec.IterBase, dec.IterRound, dec.IterPrefix, dec.IterSurveyID) == (0, 0, 0, "")
    cut = onet.message_type_id("libdrynx.SurveyQuery") + pb.encode(onet.SURVEY_QUERY, M.survey_query_to_msg(sq))
    assert M.survey_query_from_wire(cut).IterBase == 0 and len(cut) < len(M.survey_query_to_wire(sq))
    jd = sq.to_dict()
    for f in ("IterBase", "IterRound", "IterPrefix", "IterSurveyID"):
        del jd[f]
    assert Q.SurveyQuery.from_dict(jd).IterBase == 0 and Q.SurveyQuery.from_dict(jd).IterSurveyID == ""


# ----------------------------------------------------------------------------- searches end to end
FIXED = {"max": [[20, 37, 99], [99, 5], [], [98, 98, 1], [99]],      # ties, an empty DP, the extreme at QueryMax
         "min": [[20, 37, 99], [0, 5], [], [0, 0, 1], [64]]}         # ... and at QueryMin


def fixed_data(cl, lists, lo=0):
    return {dp.id: [torch.tensor([x + lo for x in lists[i]], dtype=torch.int64)] for i, dp in enumerate(cl.dps)}


def check_search_fixed(cl, node, client, device, qmin, qmax, base):
    """min and max over fixed records: the clear value and the classic query's answer."""
    lo, hi = qmin, qmax
    span = hi - lo
    for name in ("max", "min"):
        lists = [[x * span // 99 for x in r] for r in FIXED[name]]
        node.dp_data = {k: [c.to(device) for c in v] for k, v in fixed_data(cl, lists, lo).items()}
        try:
            sq = make_survey(client, cl, name, query_min=lo, query_max=hi, rows=3)
            _, vals, _ = client.send_survey_query(sq)
            seen = []
            value, rounds = client.send_iterative_extreme(sq, base, on_round=lambda k, d, r: seen.append((k, d)))
        finally:
            node.dp_data = {}
        flat = [x + lo for r in lists for x in r]
        want = max(flat) if name == "max" else min(flat)
        L = Q.iter_rounds(lo, hi, base)
        assert value == float(want) == vals[0][0]
        assert len(rounds) == L and [k for k, _ in seen] == list(range(L))
        assert lo + sum(d * base ** (L - 1 - k) for k, d in seen) == want
        assert [r.survey_id for r in rounds] == [f"{sq.SurveyID}.r{k}" for k in range(L)]
        assert all(r.n_out == base and r.block is None for r in rounds)


def check_search_generated(cl, node, client, qmin, qmax, base):
    """Generated records (no dp_data): every round must draw the same ones."""
    for name in ("max", "min"):
        sq = make_iterative_survey(client, cl, name, base, query_min=qmin, query_max=qmax, rows=6)
        value, rounds = client.send_iterative_extreme(sq, base)
        L = Q.iter_rounds(qmin, qmax, base)
        # round 0's clear rows are every DP's leading digit in unary
        lead = [sum(v[0]) if name == "max" else base - sum(v[0]) for v in rounds[0].clear_dp.values()]
        assert len(lead) == len(cl.dps)
        assert (max(lead) if name == "max" else min(lead)) == int(value - qmin) // base ** (L - 1)
        # the DPs' records, redrawn here from the shared id as the DPs draw them: rounds seeded
        # from their own survey ids would each see other records and miss this value
        from drynx_amd.protocols.data_collection import _seed

        ext = []
        for dp in cl.dps:
            gen = torch.Generator().manual_seed(_seed(sq.SurveyID, dp.id))
            t = torch.randint(qmin, qmax + 1, (1, 6), generator=gen, dtype=torch.int64)
            ext.append(int(t.max() if name == "max" else t.min()))
        assert value == float(max(ext) if name == "max" else min(ext))
        assert len(rounds) == L


def test_search_fixed_records(env):
    cl, node, client = env
    check_search_fixed(cl, node, client, "cpu", 0, 99, 10)
    check_search_fixed(cl, node, client, "cpu", -40, 59, 10)


def test_search_generated_records(env):
    cl, node, client = env
    check_search_generated(cl, node, client, 0, 99, 10)


def test_group_by_takes_one_digit_per_round(env):
    """Every group encodes the same records: the digit of group 0, the others agreeing."""
    cl, node, client = env
    node.dp_data = fixed_data(cl, FIXED["max"])
    try:
        sq = make_iterative_survey(client, cl, "max", 10, query_min=0, query_max=99, rows=3, group_by=(2, 2))
        value, rounds = client.send_iterative_extreme(sq, 10)
    finally:
        node.dp_data = {}
    assert value == 99.0 and [r.n_groups for r in rounds] == [4, 4]
    assert all(r.client_out == [9] * 4 for r in rounds)


def test_min_without_records_is_query_min(env):
    cl, node, client = env
    node.dp_data = fixed_data(cl, [[], [], [], [], []])
    try:
        sq = make_survey(client, cl, "min", query_min=3, query_max=102, rows=3)
        value, rounds = client.send_iterative_extreme(sq, 10)
    finally:
        node.dp_data = {}
    assert value == 3.0 and len(rounds) == 1


def check_search_with_proofs(cl, node, client, device, qmax, base):
    """(2, 1) proofs and 3 VNs: one block per round, every code PROOF_TRUE, 5 + 3 + 3 stored proofs per round id."""
    lists = [[x * qmax // 99 for x in r] for r in FIXED["max"]]
    node.dp_data = {k: [c.to(device) for c in v] for k, v in fixed_data(cl, lists).items()}
    try:
        sq = make_iterative_survey(client, cl, "max", base, query_min=0, query_max=qmax, rows=3, proofs=1,
                                   sig_device=device)
        value, rounds = client.send_iterative_extreme(sq, base)
    finally:
        node.dp_data = {}
    L = Q.iter_rounds(0, qmax, base)
    assert value == float(max(x for r in lists for x in r))
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


def test_search_with_proofs(env):
    cl, node, client = env
    check_search_with_proofs(cl, node, client, "cpu", 99, 10)


def test_inconsistent_dp_raises(env):
    cl, node, client = env
    node.dp_data = fixed_data(cl, [[20, 37], [35, 50], [], [41], [64]])

    def swap(k, digit, res):
        if k == 0:  # the only DP under the prefix 2 moves away: nobody matches in round 1
            assert digit == 2
            node.dp_data = fixed_data(cl, [[70, 71], [35, 50], [], [41], [64]])

    try:
        sq = make_survey(client, cl, "min", query_min=0, query_max=99, rows=3)
        with pytest.raises(RuntimeError, match="no DP matches"):
            client.send_iterative_extreme(sq, 10, on_round=swap)
    finally:
        node.dp_data = {}


def test_per_dp_encoder_matches_the_batch(env):
    """dp_encode (one DP at a time) sends the values dp_encode_batch does."""
    from drynx_amd.protocols import data_collection as dcp

    cl, node, client = env
    node.dp_data = fixed_data(cl, [[20, 37], [35, 50], [], [41], [64]])
    try:
        for name, k, prefix in (("max", 0, 0), ("max", 1, 6), ("min", 1, 2), ("min", 1, 9)):
            sq = client.iterative_round_query(make_survey(client, cl, name, query_min=0, query_max=99, rows=3), 10, k,
                                              prefix, "enc")
            batch = dcp.dp_encode_batch(node, sq, cl.dps)
            for dp in cl.dps:
                one = dcp.dp_encode(node, sq, dp, sync_timer=False)
                assert one["clear"] == batch[dp.id]["clear"] and len(one["cv"]) == 10
    finally:
        node.dp_data = {}


# ----------------------------------------------------------------------------- two ranks, simulation
def test_two_gloo_ranks_through_the_tool(tmp_path):
    env_ = dict(os.environ, OMP_NUM_THREADS="4", DX_NUM_THREADS="4")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_iter.py"), "--query", "max", "--gpus", "2",
                        "--range", "1000", "--bases", "10", "--steps", "1", "--passes", "1", "--device", "cpu",
                        "--no-classic",
                        "--out-dir", str(tmp_path)], cwd=ROOT, env=env_, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert line["result_ok"] and line["all_proofs_valid"] and line["n_gpus"] == 2
    assert line["queries"]["base=10"]["rounds"] == 3 and line["runs"][0]["blocks_per_result"] == 3
    assert json.load(open(tmp_path / "range_1000.json"))["clear_max"] == line["clear_max"]


def test_simul_runfile_column(tmp_path, monkeypatch):
    from drynx_amd.parallel.comm import LocalComm
    from drynx_amd.simul import simul

    seen = []
    send = DrynxClient.send_iterative_extreme

    def recording(self, sq, base, on_round=None):
        value, rounds = send(self, sq, base, on_round)
        seen.append((base, len(rounds), rounds[0].n_out))
        return value, rounds

    monkeypatch.setattr(DrynxClient, "send_iterative_extreme", recording)
    row = {"NbrServers": 2, "NbrDPs": 4, "NbrVNs": 0, "Proofs": 0, "OperationName": "max", "MinData": 0,
           "MaxData": 999, "DPRows": 5}
    it = simul.run_row({"Rounds": 1}, dict(row, IterBase=10), LocalComm("cpu"), "cpu", str(tmp_path / "a"),
                       netem="off")
    assert seen == [(10, 3, 10)] and 0 <= it[0][0] <= 999
    one = simul.run_row({"Rounds": 1}, dict(row), LocalComm("cpu"), "cpu", str(tmp_path / "b"), netem="off")
    assert seen == [(10, 3, 10)] and len(one) == 1
