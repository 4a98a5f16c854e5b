"""Logistic regression over SQL cohorts: a ``logistic regression`` query with
``Query.SQL`` answers one model per cell of its WHERE / GROUP BY.  A DP's
records are (X, y, K): K [N, width] int64 holds the key columns of record i in
row i.  Host side: the query rules, the cell rule against the grouped moments,
the host model, generated key tables and queries end to end.  The inputs are
exact: features in {0, 1, 2, 3}, Means 1.0, StandardDeviations 2.0, so every
standardised value is a multiple of 1/2, every product a multiple of 1/4 and
every sum exact in fp64 in any order.  The ``check_*`` functions take the
device: tests/test_lr_cohort_gpu.py runs them on the GPU."""
import logging
import math

import pytest
import torch

from drynx_amd import native as nt
from drynx_amd import query as Q
from drynx_amd.models import logistic_regression as lr
from drynx_amd.protocols import data_collection as dcp
from drynx_amd.query import LogisticRegressionParameters

MEAN, SD, PRECISION = 1.0, 2.0, 4.0  # products are multiples of 1/4: times 4 they are integers


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def lr_params(d, n, T=0, packing=0, k=2, precision=PRECISION, max_iter=25):
    return LogisticRegressionParameters(NbrRecords=n, NbrFeatures=d, Means=[MEAN] * d, StandardDeviations=[SD] * d,
                                        Lambda=1.0, Step=0.05, MaxIterations=max_iter, InitialWeights=[0.1] * (d + 1),
                                        K=k, PrecisionApproxCoefficients=precision, Packing=packing, NbrTargets=T)


def exact_records(N, d, T, seed=0):
    """(X float64 [N, d] in {0, 1, 2, 3}, y int64 [N] (T = 1) or [N, T] in {0, 1})."""
    X = torch.randint(0, 4, (N, d), generator=_gen(seed + 7 * N + d)).to(torch.float64)
    y = torch.randint(0, 2, (N,) if T == 1 else (N, T), generator=_gen(seed + 13 * N + T))
    return X, y


def sql(group_by=(), where=(), select=()):
    return Q.QuerySQL(Select=list(select), Where=[Q.WhereClear(n, str(v)) for n, v in where], GroupBy=list(group_by))


def plan_of(group_by=(), where=()):
    """SQLPlan from [(column, cardinality)] and [(column, value)]."""
    cols = [c for c, _ in group_by] + [c for c, _ in where]
    return Q.SQLPlan([], list(where), list(group_by), 1 + max(cols))


# ----------------------------------------------------------------------------- key tables of the structural cases
def key_tables(N, seed=0):
    """{case: (K [N, width] int64, plan)}: the key tables every encoder shape is
    checked on.  ``sizes``: G = 7, cells of 0, 1, 3, 4, 5 and all remaining
    records (more than 64 from N = 78 on: below, equal to and straddling a
    K-step of 4, and more than one wave's stride), one more empty cell, the
    membership interleaved by a fixed shuffle."""
    g = _gen(1000 + N + seed)
    out = {}
    ids = []
    for c, n in ((1, 1), (2, 3), (3, 4), (4, 5)):
        ids += [c] * n
    ids = (ids + [5] * N)[:N] if N >= len(ids) else ids[:N]
    ids = torch.tensor(ids, dtype=torch.int64)[torch.randperm(N, generator=g)]
    out["sizes"] = (ids[:, None].clone(), plan_of([(0, 7)]))
    k0 = torch.randint(0, 3, (N,), generator=g)
    k1 = torch.randint(0, 2, (N,), generator=g)
    out["where"] = (torch.stack([k0, k1], 1), plan_of([(0, 3)], [(1, 1)]))
    out["out_of_range"] = (torch.randint(-1, 4, (N, 1), generator=g), plan_of([(0, 3)]))
    out["two_columns"] = (torch.stack([k0, torch.randint(0, 4, (N,), generator=g), k1], 1),
                          plan_of([(0, 3), (2, 2)]))
    out["all_dropped"] = (torch.stack([k0, k1], 1), plan_of([(0, 3)], [(1, 7)]))
    out["where_only"] = (torch.stack([k0, k1], 1), plan_of((), [(1, 0), (0, 2)]))
    return out


def wide_table(N, seed=0):
    """G = 4096 (64 x 64): almost every cell empty."""
    K = torch.randint(0, 64, (N, 2), generator=_gen(2000 + N + seed))
    return K, plan_of([(0, 64), (1, 64)])


def host_cells(X, y, K, params, plan):
    """The host model on CPU copies."""
    return lr.encode_coefficients_int_cells(X.cpu(), y.cpu(), K.cpu(), params, plan)


def terms(plan):
    return [(c, 0, v) for c, v in plan.group_by], list(plan.where)


# ----------------------------------------------------------------------------- the host model
def test_cell_ids_rule():
    K = torch.tensor([[0, 1, 1], [2, 0, 1], [1, 1, 0], [3, 0, 1], [-1, 1, 1], [1, 1, 1], [2, 1, 1]])
    ids, G = lr.cell_ids(K, plan_of([(0, 3), (1, 2)], [(2, 1)]))
    # first column most significant; row 2 fails the filter, rows 3 and 4 are outside [0, 3)
    assert G == 6 and ids.tolist() == [1, 4, 6, 6, 6, 3, 5]
    assert [g for g in dcp.all_possible_groups([3, 2])][4] == [2, 0]
    ids, G = lr.cell_ids(K, plan_of((), [(2, 1)]))
    assert G == 1 and ids.tolist() == [0, 0, 1, 0, 0, 0, 0]


@pytest.mark.parametrize("N,d,T", [(1, 3, 1), (37, 3, 1), (123, 7, 3)])
@pytest.mark.parametrize("packing", [0, 1])
def test_host_model_is_the_encoder_on_each_cells_records(N, d, T, packing):
    X, y = exact_records(N, d, T)
    p = lr_params(d, N, T, packing)
    tables = key_tables(N)
    tables["wide"] = wide_table(N)
    for name, (K, plan) in tables.items():
        vals = lr.encode_coefficients_int_cells(X, y, K, p, plan)
        ids, G = lr.cell_ids(K, plan)
        assert vals.shape == (G, lr.n_coeffs(d, 2, packing, T)) and vals.dtype == torch.int64
        for c in range(G) if G <= 8 else ids[ids < G].unique().tolist():
            rows = [i for i in range(N) if ids[i] == c]
            if rows:
                assert torch.equal(vals[c], lr.encode_coefficients_int(X[rows], y[rows], p)), (name, c)
            else:
                assert not vals[c].any(), (name, c)
        # level 2's (0, 0) counts the cell: the first level-2 value in both layouts
        counts = torch.bincount(ids, minlength=G + 1)[:G]
        assert torch.equal(vals[:, T * (d + 1)], -counts * int(PRECISION)), name
        assert [lr.cohort_records(v.tolist(), p) for v in vals[:8]] == counts[:8].tolist()
    assert not lr.encode_coefficients_int_cells(X, y, tables["all_dropped"][0], p, tables["all_dropped"][1]).any()
    many = lr.encode_coefficients_int_cells_many([X, None, X[:0]], [y, None, y[:0]], [K, None, K[:0]], p, plan)
    assert torch.equal(many[0], vals) and not many[1:].any()


def test_model_refusals():
    X, y = exact_records(9, 3, 1)
    K = torch.zeros((9, 2), dtype=torch.int64)
    plan = plan_of([(1, 2)])
    for bad in (lr_params(3, 9, k=1), lr_params(3, 9, k=3)):
        with pytest.raises(ValueError, match="K = 2"):
            lr.encode_coefficients_int_cells(X, y, K, bad, plan)
    p = lr_params(3, 9)
    p.Means = []
    with pytest.raises(ValueError, match="Means"):
        lr.encode_coefficients_int_cells(X, y, K, p, plan)
    with pytest.raises(ValueError, match="1 columns"):
        lr.encode_coefficients_int_cells(X, y, K[:, :1], lr_params(3, 9), plan)
    with pytest.raises(ValueError, match="key table"):
        lr.encode_coefficients_int_cells(X, y, K[:5], lr_params(3, 9), plan)
    with pytest.raises(ValueError, match="key table"):
        lr.encode_coefficients_int_cells(X, y, None, lr_params(3, 9), plan)


def check_counts_match_group_moments(device):
    """The cell rule of the encoder and the one of the grouped moments are the
    same rule: per-cell record counts, read as -total[0, 0], equal
    ``group_moments`` with the single pair (C, C) on the same K, keys and
    filters; ``group_cells`` gives the ids of the torch rule."""
    N, d = 123, 3
    X, y = exact_records(N, d, 1)
    tables = key_tables(N)
    tables["wide"] = wide_table(N)
    p = lr_params(d, N, precision=1.0)
    for name, (K, plan) in tables.items():
        keys, filters = terms(plan)
        Kd = K.to(device)
        gm = nt.group_moments(torch.zeros((N, 0), dtype=torch.int64, device=device), Kd, [N], [(0, 0)], keys, filters)
        vals = lr.encode_coefficients_int_cells(X.to(device), y.to(device), Kd, p, plan)
        assert torch.equal(-vals[:, d + 1], gm[0, :, 0]), name
        ids, G = lr.cell_ids(K, plan)
        assert torch.equal(nt.group_cells(Kd, N, keys, filters).cpu(), ids), name
        # a strided K (a column slice of a wider table) is read in place
        wide = torch.cat([torch.full((N, 2), 9), K, torch.full((N, 1), 9)], 1).to(device)
        view = wide[:, 2:2 + K.shape[1]]
        assert not view.is_contiguous() or K.shape[1] == wide.shape[1]
        assert torch.equal(nt.group_cells(view, N, keys, filters).cpu(), ids), name
    assert nt.group_cells(None, 5).tolist() == [0] * 5
    with pytest.raises(ValueError, match="column 2"):
        nt.group_cells(K.to(device), N, [(2, 0, 3)], [])
    with pytest.raises(ValueError, match="key columns"):
        nt.group_cells(K.to(device), N, [(0, 0, 2)] * 5, [])
    with pytest.raises(ValueError, match="filter terms"):
        nt.group_cells(K.to(device), N, [], [(0, 0)] * 9)
    with pytest.raises(ValueError, match="rows"):
        nt.group_cells(K.to(device), N + 1, [(0, 0, 2)], [])


def test_counts_match_group_moments_cpu():
    check_counts_match_group_moments("cpu")


# ----------------------------------------------------------------------------- queries end to end
ROWS = (40, 37, 43)


def query_records(T, seed):
    """Per DP (X, y, K [n, 3]): c0 unused, c1 the group column in [-1, 3] --
    value 2 only among the records the filter rejects -- c2 the filter column."""
    out = []
    for i, n in enumerate(ROWS):
        X, y = exact_records(n, 3, T, seed + i)
        g = _gen(seed + 50 + i)
        c0 = torch.randint(0, 4, (n,), generator=g)
        c1 = torch.randint(0, 2, (n,), generator=g)
        c2 = torch.randint(0, 2, (n,), generator=g)
        c1[c2 == 0] = torch.randint(0, 3, (int((c2 == 0).sum()),), generator=g)
        c1[0], c1[1], c2[0], c2[1] = -1, 3, 1, 1  # out of the domain: dropped
        out.append((X, y, torch.stack([c0, c1, c2], 1)))
    return out


def run_cohort_query(data, lp, device, workdir, n_vns=0, **survey):
    from drynx_amd.services.api import DrynxClient
    from drynx_amd.services.local import local_cluster, make_survey

    cl, node = local_cluster(3, len(data), n_vns, device=device, workdir=workdir)
    try:
        client = DrynxClient(node, device=device)
        node.dp_data = {dp.id: tuple(t.to(device) for t in rec) for dp, rec in zip(cl.dps, data)}
        sq = make_survey(client, cl, "logistic regression", lr_params=lp, **survey)
        assert Q.check_parameters(sq, False)
        keys, vals, res = client.send_survey_query(sq)
        return keys, vals, res, [[int(x) for x in v] for v in client.last_plaintexts], sq
    finally:
        node.close(remove=True)


def expected_weights(tot, lp, n):
    """find_minimum_weights on a cell's aggregate with the cell's count as N (NaNs for an empty cell)."""
    D, T = lp.NbrFeatures + 1, lr.n_targets(lp)
    if n == 0:
        return [float("nan")] * (T * D)
    approx = [a / lp.PrecisionApproxCoefficients for a in lr.unpack(tot, lp.NbrFeatures, 2, lp.Packing, T)]
    if T == 1:
        return list(lr.find_minimum_weights(approx, lp.InitialWeights, n, lp.Lambda, lp.Step, lp.MaxIterations))
    out = []
    for t in range(T):
        out += list(lr.find_minimum_weights([approx[0][t]] + approx[1:], lp.InitialWeights, n, lp.Lambda, lp.Step,
                                            lp.MaxIterations))
    return out


def _same_weights(got, exp):
    assert len(got) == len(exp)
    for a, b in zip(got, exp):
        assert (math.isnan(a) and math.isnan(b)) or a == b, (got, exp)


def check_cohort_queries(device, tmp_path):
    # case 1: GROUP BY c1 (3 values) WHERE c2 = 1; group 2 is empty by construction
    for T, packing in ((1, 0), (2, 1)):
        data = query_records(T, seed=10 * T)
        lp = lr_params(3, sum(ROWS), T if T > 1 else 0, packing)
        plan = plan_of([(1, 3)], [(2, 1)])
        keys, vals, res, plain, sq = run_cohort_query(data, lp, device, str(tmp_path / f"g{T}"), group_by=(3,),
                                                      sql=sql(["c1"], [("c2", 1)]))
        assert Q.sql_plan(sq.Query) == plan
        assert keys == ["[0]", "[1]", "[2]"]
        cells = [host_cells(X, y, K, lp, plan) for X, y, K in data]  # per DP [3, n_out]
        for i, dp_vals in enumerate(res.clear_dp.values()):
            assert [list(v) for v in dp_vals] == cells[i].tolist()
        pooled = [sum(int(((K[:, 2] == 1) & (K[:, 1] == g)).sum()) for _, _, K in data) for g in range(3)]
        assert pooled[0] > 4 and pooled[1] > 4 and pooled[2] == 0
        for g in range(3):
            tot = sum(c[g] for c in cells).tolist()
            assert plain[g] == tot
            assert lr.cohort_records(tot, lp) == pooled[g]
            assert len(vals[g]) == max(1, T) * 4
            _same_weights(vals[g], expected_weights(tot, lp, pooled[g]))
        assert all(math.isnan(w) for w in vals[2]) and not any(math.isnan(w) for w in vals[0] + vals[1])
    # case 2: WHERE only; the filtered answer is replicated over the groups of GroupByValues
    data = query_records(1, seed=30)
    lp = lr_params(3, sum(ROWS))
    plan = plan_of((), [(2, 1)])
    keys, vals, res, plain, _ = run_cohort_query(data, lp, device, str(tmp_path / "w"), group_by=(2,),
                                                 sql=sql((), [("c2", 1)]))
    assert keys == ["0", "1"] and plain[0] == plain[1]
    _same_weights(vals[0], vals[1])
    tot = sum(host_cells(X, y, K, lp, plan)[0] for X, y, K in data).tolist()
    n = sum(int((K[:, 2] == 1).sum()) for _, _, K in data)
    assert plain[0] == tot and 0 < n < sum(ROWS)
    _same_weights(vals[0], expected_weights(tot, lp, n))
    # the descent ran with the cohort's count, not NbrRecords
    assert vals[0] != list(lr.decode_logistic_regression_values(tot, lp))


def check_cohort_proofs(device, tmp_path):
    """test_lr_targets' proof setup (3 CNs, 3 DPs, 3 VNs, ranges (4, 4, offset
    128), sd 2.5, rows 5, 6, 4, T = 2) with one GROUP BY column of cardinality
    2: |coefficient| <= 6 records * 1 * precision 10 < 128 in every cell."""
    import test_lr_targets as tg

    d, T, rows = 3, 2, (5, 6, 4)
    D = d + 1
    lp = tg.lr_params(d, sum(rows), T)
    lp.StandardDeviations = [2.5] * d
    data = [(X, Y, torch.randint(0, 2, (len(X), 1), generator=_gen(70 + i)))
            for i, (X, Y) in enumerate(tg.dp_records(rows, d, T, seed=40))]
    plan = plan_of([(0, 2)])
    keys, vals, res, plain, sq = run_cohort_query(data, lp, device, str(tmp_path), n_vns=3, group_by=(2,),
                                                  sql=sql(["c0"]), proofs=1, ranges=[4, 4, 128],
                                                  thresholds=[1.0, 1.0, 1.0, 0.0, 1.0], sig_device=device)
    n_out = T * D + D * D
    assert sq.Query.Operation.NbrOutput == n_out == len(sq.Query.Ranges)
    codes = res.block.data_block().Proofs
    assert set(codes.values()) == {1} and len(codes) == 3 * (3 + 3 + 3)
    assert keys == ["[0]", "[1]"]
    cells = [host_cells(X, Y, K, lp, plan) for X, Y, K in data]
    for g in range(2):
        tot = sum(c[g] for c in cells).tolist()
        n = sum(int((K[:, 0] == g).sum()) for _, _, K in data)
        assert max(abs(v) for v in tot) < 128 and n > 0
        assert plain[g] == tot and len(vals[g]) == T * D
        _same_weights(vals[g], expected_weights(tot, lp, n))


def test_cohort_queries_cpu(tmp_path):
    check_cohort_queries("cpu", tmp_path)


def test_cohort_query_with_proofs_cpu(tmp_path):
    check_cohort_proofs("cpu", tmp_path)


# ----------------------------------------------------------------------------- the query rules
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


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    from drynx_amd.services.api import DrynxClient
    from drynx_amd.services.local import local_cluster

    cl, node = local_cluster(3, 3, 0, device="cpu", workdir=str(tmp_path_factory.mktemp("db")))
    yield cl, node, DrynxClient(node)
    node.close(remove=True)


def _survey(env, lp=None, s=None, group_by=(3,), **kw):
    from drynx_amd.services.local import make_survey

    cl, _, client = env
    return make_survey(client, cl, "logistic regression", lr_params=lp or lr_params(3, 30), group_by=group_by,
                       sql=s if s is not None else sql(["c1"], [("c2", 1)]), **kw)


def test_check_parameters_cohort_rules(env):
    assert _messages(_survey(env)) == (True, [])
    for T, packing in ((0, 1), (1, 0), (2, 0), (64, 1)):
        assert _messages(_survey(env, lr_params(3, 30, T, packing))) == (True, [])
    assert _messages(_survey(env, s=sql((), [("c5", -2)]), group_by=(3, 2))) == (True, [])
    plan = Q.sql_plan(_survey(env, s=sql(["c4", "c1"], [("c2", 1)]), group_by=(3, 2)).Query)
    assert plan == Q.SQLPlan([], [(2, 1)], [(4, 3), (1, 2)], 5)
    none = _survey(env)
    none.Query.Operation.LRParameters = None
    no_means = lr_params(3, 30)
    no_means.Means = []
    no_sds = lr_params(3, 30)
    no_sds.StandardDeviations = []
    bad = {"select": _survey(env, s=sql(["c1"], select=["c0"])), "K = 1": _survey(env, lr_params(3, 30, k=1)),
           "K = 3": _survey(env, lr_params(3, 30, k=3)), "Means": _survey(env, no_means),
           "StandardDeviations": _survey(env, no_sds), "no LRParameters": none}
    for text, sq in bad.items():
        ok, seen = _messages(sq)
        hits = [m for m in seen if "SQL" in m]
        assert not ok and len(hits) == 1 and text in hits[0] and "logistic regression" in hits[0], (text, seen)
    # the refusals that were there stay
    for text, sq in {"iterative rounds": _survey(env), "cutting factor": _survey(env)}.items():
        if text == "iterative rounds":
            sq.IterBase = 2
        else:
            sq.Query.CuttingFactor = 2
        ok, seen = _messages(sq)
        assert not ok and any(m == f"SQL with {'iterative rounds' if sq.IterBase else 'a cutting factor'}"
                              for m in seen), seen
    ok, seen = _messages(_survey(env, s=sql(["c1"] * 5), group_by=(1,) * 5))
    assert not ok and any("more than 4 columns" in m for m in seen)
    # the number of outputs per group is the ungrouped query's
    for T, packing in ((0, 0), (3, 1)):
        sq = _survey(env, lr_params(3, 30, T, packing))
        assert sq.Query.Operation.NbrOutput == Q.lr_nbr_outputs(3, 2, packing, T)
        assert dcp.expected_n_out(sq) == sq.Query.Operation.NbrOutput


def test_a_dp_without_key_table_aborts_the_survey(env):
    cl, node, client = env
    data = query_records(1, seed=3)
    sq = _survey(env, lr_params(3, sum(ROWS)))
    try:
        node.dp_data = {dp.id: rec for dp, rec in zip(cl.dps, data)}
        node.dp_data[cl.dps[1].id] = data[1][:2]
        with pytest.raises(Exception, match=f"DP {cl.dps[1].id} has records without a key table"):
            client.send_survey_query(sq)
        node.dp_data[cl.dps[1].id] = (data[1][0], data[1][1], data[1][2][:, :2])  # narrower than plan.width = 3
        with pytest.raises(Exception, match=f"DP {cl.dps[1].id} has a key table"):
            client.send_survey_query(_survey(env, lr_params(3, sum(ROWS))))
    finally:
        node.dp_data = {}


def test_one_dp_path_refuses_sql(env):
    cl, node, _ = env
    with pytest.raises(ValueError, match="SQL"):
        dcp.dp_encode(node, _survey(env), cl.dps[0])


def test_generated_key_tables(env):
    """Generated K is reproducible and drawn by ``generate_sql_table``'s rule
    for its extra columns; X and y are the draws of the query without SQL."""
    cl, node, client = env
    lp = lr_params(3, 30)
    sq = _survey(env, lp, s=sql(["c1", "c3"], [("c2", 1)]), group_by=(3, 2), survey_id="cohort-generated")
    plan = Q.sql_plan(sq.Query)
    assert plan.width == 4
    for dp in cl.dps:
        K = dcp.generate_lr_keys(sq, dp.id, plan, 30)
        assert K.shape == (30, 4) and K.dtype == torch.int64
        assert torch.equal(K, dcp.generate_lr_keys(sq, dp.id, plan, 30))
        assert set(K[:, 1].tolist()) == {0, 1, 2} and set(K[:, 3].tolist()) == {0, 1}
        assert set(K[:, 0].tolist()) == set(K[:, 2].tolist()) == {0, 1, 2, 3}
        gen = _gen(dcp._seed(sq.SurveyID + "/sql", dp.id))
        assert torch.equal(K[:, 0], torch.randint(0, 4, (30,), generator=gen))
        assert torch.equal(K[:, 1], torch.randint(0, 3, (30,), generator=gen))
    dev = torch.device("cpu")
    a = dcp._lr_values(node, sq, cl.dps, dev)
    assert a.shape == (3, 6, sq.Query.Operation.NbrOutput) and torch.equal(a, dcp._lr_values(node, sq, cl.dps, dev))
    for i, dp in enumerate(cl.dps):
        X, y = dcp.generate_lr_data(lp, dev, _gen(dcp._seed(sq.SurveyID, dp.id)))
        K = dcp.generate_lr_keys(sq, dp.id, plan, 30)
        assert torch.equal(a[i], lr.encode_coefficients_int_cells(X, y, K, lp, plan))
    # one group of cardinality 1 holds every record: the vectors of the query without SQL
    one = _survey(env, lp, s=sql(["c0"]), group_by=(1,), survey_id="cohort-generated")
    plain = _survey(env, lp, s=Q.QuerySQL(), group_by=(1,), survey_id="cohort-generated")
    assert torch.equal(dcp._lr_values(node, one, cl.dps, dev)[:, 0], dcp._lr_values(node, plain, cl.dps, dev))
    keys, vals, _ = client.send_survey_query(sq)
    assert keys == ["[0 0]", "[0 1]", "[1 0]", "[1 1]", "[2 0]", "[2 1]"] and all(len(v) == 4 for v in vals)
    assert client.last_plaintexts == a.sum(0).tolist()
