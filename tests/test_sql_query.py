"""SQL WHERE / GROUP BY over the DPs' records (``Query.SQL``), end to end on a
3 CN / 5 DP / 3 VN cluster with fixed records in ``node.dp_data``: 5 DPs with 3
to 40 records of 4 columns (c0 the value in [0, 7], c1 in [-1, 3] -- group 2
only among records the filter rejects -- c2 the filter column, c3 in [0, 1]);
DP 2 has no record passing c2 = 1.  Plus the query model: check_parameters,
the wire and JSON forms, generated tables and the file loader.  The ``check_*``
functions take the device: tests/test_sql_query_gpu.py runs them on the GPU."""
import logging
import math

import pytest
import torch

from drynx_amd import query as Q
from drynx_amd.models.datasets import load_dp_file
from drynx_amd.proofs import requests as prq
from drynx_amd.protocols import data_collection as dcp
from drynx_amd.services.api import DrynxClient
from drynx_amd.services.local import local_cluster, make_survey
from drynx_amd.wire import messages as wm

SIZES = [3, 8, 17, 40, 5]


def records():
    """[DP][record] = (c0, c1, c2, c3), the same on every call."""
    g = torch.Generator().manual_seed(23)
    out = []
    for i, n in enumerate(SIZES):
        c0 = torch.randint(0, 8, (n,), generator=g)
        c1 = torch.randint(0, 2, (n,), generator=g)
        c2 = torch.randint(0, 2, (n,), generator=g) if i != 2 else torch.zeros(n, dtype=torch.int64)
        c3 = torch.randint(0, 2, (n,), generator=g)
        c1[c2 == 0] = torch.randint(0, 3, (int((c2 == 0).sum()),), generator=g)  # group 2: rejected records only
        if n >= 8:  # out-of-domain group values: dropped
            c1[0], c1[1] = -1, 3
        if i == 0:
            c2[:] = 1
        out.append(torch.stack([c0, c1, c2, c3], dim=1).tolist())
    return out


def pooled(where, group_cols, cards):
    """{group tuple: [c0 of the pooled records of the group that pass ``where``]} over all_possible_groups."""
    cells = {tuple(g): [] for g in dcp.all_possible_groups(cards)}
    for dp in records():
        for r in dp:
            key = tuple(r[c] for c in group_cols)
            if all(r[c] == v for c, v in where) and key in cells:
                cells[key].append(r[0])
    return cells


def set_records(cl, node, device):
    node.dp_data = {dp.id: [torch.tensor(col, dtype=torch.int64, device=device)
                            for col in zip(*records()[i])] for i, dp in enumerate(cl.dps)}


def sql(group_by=(), where=(("c2", "1"),), select=()):
    return Q.QuerySQL(Select=list(select), Where=[Q.WhereClear(n, v) for n, v in where], GroupBy=list(group_by))


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    cl, node = local_cluster(3, 5, 3, device="cpu", workdir=str(tmp_path_factory.mktemp("db")))
    yield cl, node, DrynxClient(node)
    node.close(remove=True)


def _same(got, exp):
    assert len(got) == len(exp)
    for a, b in zip(got, exp):
        assert (math.isnan(a) and math.isnan(b)) or a == pytest.approx(b, rel=1e-12, abs=1e-12), (got, exp)


# ----------------------------------------------------------------------------- surveys (CPU and GPU)
def check_mean_variance(cl, node, client, device):
    cells = pooled([(2, 1)], [1], [3])
    assert cells[(0,)] and cells[(1,)] and not cells[(2,)]
    set_records(cl, node, device)
    try:
        out = {}
        for name in ("mean", "variance"):
            sq = make_survey(client, cl, name, query_min=0, query_max=7, rows=3, group_by=(3,), sql=sql(["c1"]))
            assert Q.check_parameters(sq, False)
            keys, vals, res = client.send_survey_query(sq)
            assert keys == ["[0]", "[1]", "[2]"]
            for (g,), xs in cells.items():
                n = len(xs)
                if name == "mean":
                    exp = [sum(xs) / n] if n else [float("nan")]
                else:
                    exp = [sum(x * x for x in xs) / n - (sum(xs) / n) ** 2] if n else [float("nan")]
                _same(vals[g], exp)
            # every DP's clear cells: its own records of the group
            for i, dp in enumerate(cl.dps):
                for g in range(3):
                    xs = [r[0] for r in records()[i] if r[2] == 1 and r[1] == g]
                    assert res.clear_dp[dp.id][g][:2] == [sum(xs), len(xs)]
            out[name] = vals
        return out
    finally:
        node.dp_data = {}


def check_counting(cl, node, client, device):
    cells = pooled([(2, 1)], [1, 3], [3, 2])
    assert sum(bool(v) for v in cells.values()) >= 3 and not cells[(2, 0)]
    set_records(cl, node, device)
    try:
        for name in ("frequencyCount", "min", "max", "union"):
            sq = make_survey(client, cl, name, query_min=0, query_max=7, rows=3, group_by=(3, 2),
                             sql=sql(["c1", "c3"]))
            assert Q.check_parameters(sq, False)
            keys, vals, _ = client.send_survey_query(sq)
            assert keys == ["[0 0]", "[0 1]", "[1 0]", "[1 1]", "[2 0]", "[2 1]"]
            for g, xs in enumerate(cells.values()):
                exp = {"frequencyCount": [float(xs.count(v)) for v in range(8)],
                       "min": [float(min(xs)) if xs else 0.0], "max": [float(max(xs)) if xs else 0.0],
                       "union": [float(v in xs) for v in range(8)]}[name]
                assert vals[g] == exp, (name, keys[g])
    finally:
        node.dp_data = {}


def check_where_only(cl, node, client, device):
    """WHERE without GROUP BY: the filtered answer, replicated over the groups of GroupByValues."""
    xs = [r[0] for dp in records() for r in dp if r[2] == 1]
    set_records(cl, node, device)
    try:
        sq = make_survey(client, cl, "mean", query_min=0, query_max=7, rows=3, group_by=(2,), sql=sql())
        keys, vals, _ = client.send_survey_query(sq)
        assert keys == ["0", "1"] and vals[0] == vals[1]
        _same(vals[0], [sum(xs) / len(xs)])
        # a DP with too few columns fails to encode: the survey aborts
        first = cl.dps[0].id
        node.dp_data[first] = node.dp_data[first][:2]
        with pytest.raises(Exception, match="record columns"):
            client.send_survey_query(make_survey(client, cl, "mean", query_min=0, query_max=7, rows=3,
                                                 group_by=(2,), sql=sql()))
    finally:
        node.dp_data = {}


def check_proofs(cl, node, client, device, plain):
    """The grouped mean with (16, 2) range proofs and 3 VNs."""
    for dp in records():  # every proved value fits the range [0, 16^2)
        assert sum(r[0] for r in dp) < 256 and len(dp) < 256
    set_records(cl, node, device)
    try:
        sq = make_survey(client, cl, "mean", query_min=0, query_max=7, rows=3, group_by=(3,), sql=sql(["c1"]),
                         proofs=1, ranges=[16, 2], sig_device=device)
        assert Q.check_parameters(sq, False)
        keys, vals, res = client.send_survey_query(sq)
    finally:
        node.dp_data = {}
    codes = res.block.data_block().Proofs
    assert set(codes.values()) == {prq.PROOF_TRUE} and len(codes) == 3 * (5 + 3 + 3)
    assert len([k for k in codes if k.split("/")[1] == "range" and k.endswith("/vn0")]) == len(cl.dps)
    assert keys == ["[0]", "[1]", "[2]"]
    for a, b in zip(vals, plain):
        _same(a, b)


def check_empty_sql(cl, node, client):
    sq = make_survey(client, cl, "mean", query_min=0, query_max=9, rows=10, group_by=(3, 2, 1), sql=Q.QuerySQL())
    keys, vals, res = client.send_survey_query(sq)
    assert keys == [str(g) for g in range(6)] and all(v == vals[0] for v in vals)
    tot = [sum(v[0][k] for v in res.clear_dp.values()) for k in range(2)]
    assert vals[0] == [tot[0] / tot[1]] and tot[1] == 50
    for v in res.clear_dp.values():
        assert len(v) == 6 and all(g == v[0] for g in v)


def check_generated(cl, node, client):
    """Generated tables: the same survey id gives the same answer twice; the
    value columns are generate_fake_data's draws for the seed."""
    runs = []
    for _ in range(2):
        sq = make_survey(client, cl, "variance", query_min=0, query_max=9, rows=30, group_by=(3, 2),
                         sql=sql(["c1", "c3"]), survey_id="sql-generated")
        keys, vals, res = client.send_survey_query(sq)
        runs.append((keys, [[repr(x) for x in v] for v in vals], res.clear_dp))
    assert runs[0] == runs[1]
    plan = Q.sql_plan(sq.Query)
    assert plan.width == 4 and plan.group_by == [(1, 3), (3, 2)] and plan.where == [(2, 1)] and plan.select == [0]
    tot = {}
    for dp in cl.dps:
        t = dcp.generate_sql_table(sq, dp.id, plan)
        gen = torch.Generator().manual_seed(dcp._seed(sq.SurveyID, dp.id))
        fake = dcp.generate_fake_data(sq.Query.Operation, 30, 0, 9, "cpu", gen)
        assert t.shape == (30, 4) and torch.equal(t[:, 0], fake[0])
        assert set(t[:, 1].tolist()) == {0, 1, 2} and set(t[:, 3].tolist()) == {0, 1}
        assert set(t[:, 2].tolist()) == {0, 1, 2, 3}
        for r in t.tolist():
            if r[2] == 1:
                tot.setdefault((r[1], r[3]), []).append(r[0])
    for g, grp in enumerate(dcp.all_possible_groups([3, 2])):
        xs = tot[tuple(grp)]
        assert float(runs[0][1][g][0]) == pytest.approx(sum(x * x for x in xs) / len(xs) - (sum(xs) / len(xs)) ** 2)


def test_mean_and_variance_by_group(env):
    check_mean_variance(*env, "cpu")


def test_counting_operations_by_two_columns(env):
    check_counting(*env, "cpu")


def test_where_without_group_by(env):
    check_where_only(*env, "cpu")


def test_grouped_mean_with_proofs(env):
    plain = check_mean_variance(*env, "cpu")["mean"]
    check_proofs(*env, "cpu", plain)


def test_empty_sql_replicates(env):
    check_empty_sql(*env)


def test_generated_tables(env):
    check_generated(*env)


def test_one_dp_path_refuses_sql(env):
    cl, node, client = env
    sq = make_survey(client, cl, "mean", query_min=0, query_max=7, rows=3, group_by=(3,), sql=sql(["c1"]))
    with pytest.raises(ValueError, match="SQL"):
        dcp.dp_encode(node, sq, cl.dps[0])


# ----------------------------------------------------------------------------- the query model
def _messages(sq):
    seen = []

    class H(logging.Handler):
        def emit(self, record):
            seen.append(record.getMessage())

    lg, h = logging.getLogger("drynx.query"), H()
    lg.addHandler(h)
    try:
        ok = Q.check_parameters(sq, False)
    finally:
        lg.removeHandler(h)
    return ok, seen


def test_check_parameters(env):
    cl, node, client = env

    def survey(name="mean", group_by=(3,), s=None, **kw):
        return make_survey(client, cl, name, query_min=0, query_max=7, rows=3, group_by=group_by,
                           sql=s if s is not None else sql(["c1"]), **kw)

    assert _messages(survey()) == (True, [])
    assert _messages(survey(s=sql(["c1", "c63"], select=["c5"]), group_by=(3, 2))) == (True, [])
    for name in Q.SQL_OPERATIONS:
        assert _messages(survey(name, d=2))[0], name
    bad = {
        "bool_AND": survey("bool_AND"),
        "bool_OR": survey("bool_OR"),
        "iterative": survey("min"),
        "cutting factor": survey(cutting_factor=2),
        "malformed column name 'x1'": survey(s=sql(["x1"])),
        "malformed column name 'c'": survey(s=sql(["c1"], where=[("c", "1")])),
        "malformed column name 'c01'": survey(s=sql(["c1"], select=["c01"])),
        "outside c0..c63": survey(s=sql(["c64"])),
        "is not an integer": survey(s=sql(["c1"], where=[("c2", "1.5")])),
        "'one' is not an integer": survey(s=sql(["c1"], where=[("c2", "one")])),
        "only the conjunction": survey(s=Q.QuerySQL(Predicate="c2 = 1 OR c3 = 0")),
        "more than 8 terms": survey(s=sql(["c1"], where=[("c2", "1")] * 9)),
        "more than 4 columns": survey(s=sql(["c1", "c2", "c3", "c4", "c5"]), group_by=(1,) * 5),
        "one cardinality per": survey(group_by=(3, 2)),
        "cardinality below 1": survey(group_by=(0,)),
        "at most 4096": survey(s=sql(["c1", "c2"]), group_by=(64, 65)),
        "select lists 2 columns": survey(s=sql(["c1"], select=["c0", "c3"])),
    }
    bad["iterative"].IterBase, bad["iterative"].Query.Operation.NbrOutput = 2, 2
    lr = make_survey(client, cl, "sum", query_min=0, query_max=7, rows=3, group_by=(3,), sql=sql(["c1"]))
    lr.Query.Operation.NameOp = "logistic regression"
    bad["logistic regression"] = lr
    for text, sq in bad.items():
        ok, seen = _messages(sq)
        hits = [m for m in seen if "SQL" in m or "column" in m]
        assert not ok and len(hits) == 1 and text in hits[0], (text, seen)
    # with Where only, GroupByValues keeps its meaning: no cardinality rule
    assert _messages(survey(s=sql(), group_by=(3, 2, 1))) == (True, [])


def test_wire_and_json_round_trip(env):
    cl, node, client = env
    s = sql(["c1", "c3"], where=[("c2", "1"), ("c0", "-4")], select=["c0"])
    sq = make_survey(client, cl, "mean", query_min=0, query_max=7, rows=3, group_by=(3, 2), sql=s)
    back = wm.survey_query_from_wire(wm.survey_query_to_wire(sq))
    assert back.Query.SQL == s and back.Query.DPDataGen.GroupByValues == [3, 2]
    assert wm.survey_query_to_wire(back) == wm.survey_query_to_wire(sq)
    assert Q.SurveyQuery.from_dict(sq.to_dict()).Query.SQL == s
    # empty SQL: the bytes and the dict of a survey built without touching the field
    plain = make_survey(client, cl, "mean", query_min=0, query_max=7, rows=3, group_by=(3, 2), survey_id="same")
    empty = make_survey(client, cl, "mean", query_min=0, query_max=7, rows=3, group_by=(3, 2), survey_id="same",
                        sql=Q.QuerySQL())
    assert wm.survey_query_to_wire(empty) == wm.survey_query_to_wire(plain)
    assert wm.survey_query_to_wire(sq) != wm.survey_query_to_wire(plain)
    assert empty.to_dict() == plain.to_dict() and "SQL" not in plain.to_dict()["Query"]
    assert not wm.survey_query_from_wire(wm.survey_query_to_wire(plain)).Query.SQL
    # a peer without the field reads as empty
    d = sq.to_dict()
    del d["Query"]["SQL"]
    assert not Q.SurveyQuery.from_dict(d).Query.SQL
    msg = wm.survey_query_to_msg(sq)
    del msg["Query"]["SQL"]
    assert not wm.survey_query_from_msg(msg).Query.SQL


def test_load_dp_file_reads_the_table(tmp_path):
    path = tmp_path / "dp.csv"
    path.write_text("5,1,1,0,9\n7,0,1,1,9\n2,2,0,1,9\n")
    op = Q.choose_operation("mean", 0, 7, 1, 0)
    assert [c.tolist() for c in load_dp_file(str(path), op)] == [[5, 7, 2]]
    q = Q.Query(Operation=op, DPDataGen=Q.QueryDPDataGen([3, 2], 3, 0, 7), SQL=sql(["c1", "c3"]))
    cols = load_dp_file(str(path), op, "cpu", q)
    assert [c.tolist() for c in cols] == [[5, 7, 2], [1, 0, 2], [1, 1, 0], [0, 1, 1]]
    assert [c.tolist() for c in load_dp_file(str(path), op, "cpu", Q.Query(Operation=op))] == [[5, 7, 2]]
    q.SQL.Where.append(Q.WhereClear("c5", "0"))
    with pytest.raises(ValueError, match="5 values per record"):
        load_dp_file(str(path), op, "cpu", q)
