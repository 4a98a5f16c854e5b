"""``QuerySQL.Predicate``: comparisons and ! && || over the Where terms, from
the membership rule of the grouped kernels (csrc/kernels/group_terms.h) up to
surveys end to end.

The model is this file's own: a predicate case is the operators of its atoms
and a Python function of the atom bits; a row's atoms are numpy comparisons,
the truth table is the function on every assignment, and the expected outputs
are summed row by row in Python.  The library's parser is not used to build an
expectation: it is itself checked against these tables.

Shapes: three DPs of 0, 1 and 130 rows (an empty segment, a one-row tile, a
ragged third 64-row stage) over a 4-column table holding INT64_MIN and
INT64_MAX.  The ``check_*`` functions take the device and return their
outputs: tests/test_sql_predicate_gpu.py runs them on the GPU and compares the
outputs with the host's bit for bit."""
import copy
import math

import numpy as np
import pytest
import torch

from drynx_amd import native as nt
from drynx_amd import query as Q
from drynx_amd.models import logistic_regression as lr
from drynx_amd.ops import encoding as enc
from drynx_amd.ops.encoding import moment_pairs
from drynx_amd.proofs import requests as prq
from drynx_amd.protocols import data_collection as dcp
from drynx_amd.services.api import DrynxClient
from drynx_amd.services.local import local_cluster, make_iterative_survey, make_survey
from drynx_amd.wire import messages as wm

MIN, MAX = -(1 << 63), (1 << 63) - 1
SEG = [0, 1, 130]
N = sum(SEG)
M64 = 1 << 64
KEYS, G = [(1, 0, 3)], 3
CMP = {"==": np.equal, "!=": np.not_equal, "<": np.less, "<=": np.less_equal, ">": np.greater, ">=": np.greater_equal}
BASE, QMIN, QMAX = 4, 0, 15  # the grouped rounds: two base-4 digits over [0, 15]


# ----------------------------------------------------------------------------- the model
def tables():
    """(Z [N, 3], K [N, 4]): c0 the compared column, small values with both ends of int64 and their neighbours
    planted (the one-row DP holds INT64_MIN); c1 the key over 3 values, -1 and 3 present (dropped); c2 the
    counted column of the rounds, values below and above the domain [0, 15] present; c3 in [0, 3]."""
    g = torch.Generator().manual_seed(41)
    K = torch.stack([torch.randint(-3, 4, (N,), generator=g), torch.randint(-1, 4, (N,), generator=g),
                     torch.randint(-2, 18, (N,), generator=g), torch.randint(0, 4, (N,), generator=g)], dim=1)
    K[[0, 5, 70], 0] = MIN
    K[[2, 6, 130], 0] = MAX
    K[3, 0], K[4, 0] = MIN + 1, MAX - 1
    K[[0, 2, 3, 4], 1] = torch.tensor([1, 0, 2, 1])  # the ends belong to groups
    Z = torch.randint(-9, 10, (N, 3), generator=g)
    assert (K[:, 1] == -1).any() and (K[:, 1] == 3).any() and (K[:, 2] < 0).any() and (K[:, 2] > 15).any()
    return Z, K


def table_of(n, f):
    """The truth table of f over n atom bits as an int: bit m is f(the bits of m), atom i being bit i."""
    return sum(1 << m for m in range(1 << n) if f([np.bool_(m >> i & 1) for i in range(n)]))


def keep_of(K, filters, ops, f):
    """[N] bool: the rows for which the formula f holds over the atoms K[:, column] OP value."""
    k = K.numpy()
    return np.broadcast_to(np.asarray(f([CMP[op](k[:, c], v) for (c, v), op in zip(filters, ops)]), dtype=bool),
                           (K.shape[0],))


def groups_of(K, keys, keep):
    """[N] the group of every row, -1 for a row the WHERE or a key digit drops."""
    k = K.numpy()
    g, ok = np.zeros(K.shape[0], dtype=np.int64), np.array(keep, dtype=bool)
    for c, off, card in keys:
        d = k[:, c] - off
        ok &= (d >= 0) & (d < card)
        g = g * card + np.where(ok, d, 0)
    return np.where(ok, g, -1).tolist()


def _signed(v):
    v %= M64
    return v - M64 if v >= 1 << 63 else v


def model_moments(Z, grp, seg, pairs, n_groups):
    z = [r + [1] for r in Z.tolist()]
    out = [[[0] * len(pairs) for _ in range(n_groups)] for _ in seg]
    i = 0
    for dp, cnt in enumerate(seg):
        for _ in range(cnt):
            if grp[i] >= 0:
                for p, (a, b) in enumerate(pairs):
                    out[dp][grp[i]][p] += z[i][a] * z[i][b]
            i += 1
    return torch.tensor([[[_signed(v) for v in g] for g in dp] for dp in out], dtype=torch.int64).reshape(
        len(seg), n_groups, len(pairs))


def model_round(x, grp, seg, n_groups, k, prefixes):
    """The counts of round k of the base-4 searches over [0, 15]: digit k of x under the cell's prefix."""
    lo = BASE ** (1 - k)
    out = torch.zeros((len(seg), n_groups, BASE), dtype=torch.int64)
    i = 0
    for dp, cnt in enumerate(seg):
        for _ in range(cnt):
            if grp[i] >= 0 and QMIN <= x[i] <= QMAX:
                q = (x[i] - QMIN) // lo
                if q // BASE == prefixes[grp[i]]:
                    out[dp, grp[i], q % BASE] += 1
            i += 1
    return out


def run_rule(device, Z, K, filters, predicate, keep, keys=KEYS, n_groups=G):
    """The three grouped entries under (filters, predicate) against the model for the rows ``keep`` ->
    [moments, cells, round 0, round 1]."""
    grp = groups_of(K, keys, keep)
    Zd, Kd = Z.to(device), K.to(device)
    pairs = moment_pairs("cosim", 3)
    mom = nt.group_moments(Zd, Kd, SEG, pairs, keys, filters, predicate=predicate).cpu()
    assert torch.equal(mom, model_moments(Z, grp, SEG, pairs, n_groups))
    cells = nt.group_cells(Kd, N, keys, filters, predicate=predicate).cpu()
    assert cells.tolist() == [g if g >= 0 else n_groups for g in grp]
    x = K[:, 2].tolist()
    outs = [mom, cells]
    for k, prefixes in ((0, [0] * n_groups), (1, [(1 + 2 * g) % BASE for g in range(n_groups)])):
        got = nt.iter_round_cells("frequencyCount", Kd, SEG, 2, QMIN, QMAX, BASE, k, prefixes, keys, filters,
                                  predicate).cpu()
        assert torch.equal(got, model_round(x, grp, SEG, n_groups, k, prefixes))
        outs.append(got)
    return outs


# ----------------------------------------------------------------------------- atoms
def check_atoms(device):
    """Each operator alone, the constant in the middle and at both ends of int64."""
    Z, K = tables()
    outs, kept = [], {}
    for op in nt.GROUP_OPS:
        for c in (0, MIN, MAX):
            filters = [(0, c)]
            keep = keep_of(K, filters, [op], lambda a: a[0])
            kept[op, c] = int(keep.sum())
            outs += run_rule(device, Z, K, filters, ((op,), table_of(1, lambda a: a[0])), keep)
    # exact at the ends: nothing is below INT64_MIN or above INT64_MAX, everything is at or inside them
    assert kept["<", MIN] == kept[">", MAX] == 0 and kept["<=", MAX] == kept[">=", MIN] == N
    assert kept["==", MIN] == kept["<=", MIN] == 3 and kept["==", MAX] == kept[">=", MAX] == 3
    assert kept[">", MIN] == kept["!=", MIN] == N - 3 and kept["<", MAX] == N - 3
    assert 0 < kept["<", 0] < kept["<=", 0] < N and kept[">", 0] == N - kept["<=", 0]
    return outs


# ----------------------------------------------------------------------------- formulas
# eight terms over the four columns (c0 twice against the ends' neighbours, the key column among them)
TERMS8 = [(0, 0), (0, MAX - 1), (1, 1), (2, 8), (2, 3), (3, 1), (3, 2), (1, 2)]
OPS8 = ("<", ">=", "==", ">", "<=", "!=", ">=", "<")


def _inner(a):
    return (a[0] | a[1] & a[2]) & (a[3] | ~a[4] | a[5])


# (name, formula text, function of the atoms, the 64-bit words of the table that hold accepted assignments)
FORMULAS8 = [
    ("or of eight", " || ".join(f"v{2 * i} {op} v{2 * i + 1}" for i, op in enumerate(OPS8)),
     lambda a: a[0] | a[1] | a[2] | a[3] | a[4] | a[5] | a[6] | a[7], {0, 1, 2, 3}),
    ("word 0", "(v0 < v1 || v2 >= v3 && v4 == v5) && (v6 > v7 || !(v8 <= v9) || v10 != v11) && !(v12 >= v13) "
     "&& !(v14 < v15)", lambda a: _inner(a) & ~a[6] & ~a[7], {0}),
    ("word 1", "(v0 < v1 || v2 >= v3 && v4 == v5) && (v6 > v7 || !(v8 <= v9) || v10 != v11) && v12 >= v13 "
     "&& !(v14 < v15)", lambda a: _inner(a) & a[6] & ~a[7], {1}),
    ("word 2", "(v0 < v1 || v2 >= v3 && v4 == v5) && (v6 > v7 || !v8 <= v9 || v10 != v11) && !v12 >= v13 "
     "&& v14 < v15", lambda a: _inner(a) & ~a[6] & a[7], {2}),
    ("word 3", "(v0<v1||v2>=v3&&v4==v5)&&(v6>v7||!(v8<=v9)||v10!=v11)&&v12>=v13&&v14<v15",
     lambda a: _inner(a) & a[6] & a[7], {3}),
    ("nested mix", "!(v0 < v1 && !(v2 >= v3 || v4 == v5)) && ((v6 > v7 || v8 <= v9) && !(v10 != v11 && v12 >= v13) "
     "|| !!(v14 < v15))",
     lambda a: ~(a[0] & ~(a[1] | a[2])) & ((a[3] | a[4]) & ~(a[5] & a[6]) | a[7]), {0, 1, 2, 3}),
]


def _words(table):
    return {w for w in range(4) if table >> (64 * w) & (M64 - 1)}


def check_formulas(device):
    """Eight-term formulas whose accepted assignments fall in each table word; the constant tables (every row,
    no row); an exclusive-or of two terms; one term; the equalities through the general path."""
    Z, K = tables()
    outs = []
    for name, text, f, words in FORMULAS8:
        table = table_of(8, f)
        assert _words(table) == words, name
        assert Q.parse_predicate(text, 8) == (OPS8, table), name  # the parser against the model's table
        keep = keep_of(K, TERMS8, OPS8, f)
        assert 0 < keep.sum() < N, name
        outs += run_rule(device, Z, K, TERMS8, (OPS8, table), keep)
    # accepted assignments in every word and in none: the tautology and the contradiction as tables
    outs += run_rule(device, Z, K, TERMS8, (OPS8, (1 << 256) - 1), np.ones(N, dtype=bool))
    outs += run_rule(device, Z, K, TERMS8, (OPS8, 0), np.zeros(N, dtype=bool))
    assert torch.equal(outs[-3], torch.full((N,), G)) and not outs[-4].any()
    # as formulas they are a column listed twice (every term is used once, so no table is constant)
    twice = [(3, 1), (3, 1)]
    for text, ops, f, n_keep in (("v0 == v1 || v2 != v3", ("==", "!="), lambda a: a[0] | a[1], N),
                                 ("v0 == v1 && v2 != v3", ("==", "!="), lambda a: a[0] & a[1], 0)):
        assert Q.parse_predicate(text, 2) == (ops, table_of(2, f))
        keep = keep_of(K, twice, ops, f)
        assert keep.sum() == n_keep
        outs += run_rule(device, Z, K, twice, (ops, table_of(2, f)), keep)
    # exclusive-or of two terms (written with ! && ||: each term once per atom means two Where entries each)
    xor_terms, xor_ops = [(0, 0), (3, 2), (0, 0), (3, 2)], ("<", ">=", "<", ">=")
    xor = lambda a: a[0] & ~a[1] | ~a[2] & a[3]  # noqa: E731
    assert Q.parse_predicate("v0 < v1 && !(v2 >= v3) || !(v4 < v5) && v6 >= v7", 4) == (xor_ops, table_of(4, xor))
    keep = keep_of(K, xor_terms, xor_ops, xor)
    k = K.numpy()
    assert (keep == ((k[:, 0] < 0) ^ (k[:, 3] >= 2))).all() and 0 < keep.sum() < N
    outs += run_rule(device, Z, K, xor_terms, (xor_ops, table_of(4, xor)), keep)
    # two terms, one term
    two = [(0, 0), (3, 1)]
    keep = keep_of(K, two, (">=", "=="), lambda a: a[0] | a[1])
    outs += run_rule(device, Z, K, two, ((">=", "=="), table_of(2, lambda a: a[0] | a[1])), keep)
    assert Q.parse_predicate("v0 >= v1 || v2 == v3", 2) == ((">=", "=="), 0b1110)
    one = [(3, 2)]
    keep = keep_of(K, one, ("<",), lambda a: ~a[0])
    outs += run_rule(device, Z, K, one, (("<",), table_of(1, lambda a: ~a[0])), keep)
    assert Q.parse_predicate("!(v0 < v1)", 1) == (("<",), 0b01)
    # !(v0 != v1): the equality filter's outputs, bit for bit
    eq = run_rule(device, Z, K, one, None, keep_of(K, one, ("==",), lambda a: a[0]))
    ne = run_rule(device, Z, K, one, Q.parse_predicate("!(v0 != v1)", 1), keep_of(K, one, ("==",), lambda a: a[0]))
    assert all(torch.equal(a, b) for a, b in zip(eq, ne)) and eq[0].any()
    return outs + eq + ne


def _query(where, predicate="", group_by=("c1",), cards=(3,), name="mean", select=()):
    op = Q.choose_operation(name, 0, 7, 1, 0)
    return Q.Query(Operation=op, DPDataGen=Q.QueryDPDataGen(list(cards), 3, 0, 7),
                   SQL=Q.QuerySQL(Select=list(select), Where=[Q.WhereClear(n, str(v)) for n, v in where],
                                  Predicate=predicate, GroupBy=list(group_by)))


def check_plans(device):
    """``v0 == v1 && v2 == v3`` is the plan, and so the outputs, of no predicate; a plan with a predicate
    through ``batch_values_sql`` / ``iterative_values_sql`` / ``cell_ids``."""
    Z, K = tables()
    where = [("c3", 1), ("c0", MIN)]
    plain = Q.sql_plan(_query(where))
    assert plain == Q.SQLPlan([0], [(3, 1), (0, MIN)], [(1, 3)], 4) and plain.predicate is None
    for text in ("v0 == v1 && v2 == v3", " ( v2==v3 )&&((v0 == v1)) ", "!!(v0 == v1) && v2 == v3"):
        assert Q.sql_plan(_query(where, text)) == plain
    plan = Q.sql_plan(_query(where, "v0 == v1 || v2 > v3"))
    assert plan.predicate == (("==", ">"), 0b1110) and plan.where == plain.where and plan != plain
    assert Q.sql_plan(_query(where, "v0 == v1 && v2 != v3")).predicate == (("==", "!="), 0b1000)
    keep = keep_of(K, plan.where, ("==", ">"), lambda a: a[0] | a[1])
    grp = groups_of(K, KEYS, keep)
    Zd, Kd = Z.to(device), K.to(device)
    outs = [enc.batch_values_sql("mean", Zd, Kd, SEG, plan).cpu()]
    assert torch.equal(outs[0], model_moments(Z[:, :1], grp, SEG, moment_pairs("mean", 1), G))
    cnt = enc.batch_values_sql("frequencyCount", Zd, Kd, SEG, Q.sql_plan(_query(
        where, "v0 == v1 || v2 > v3", name="frequencyCount", select=["c2"])), 0, 15).cpu()
    x = K[:, 2].tolist()
    exp = torch.zeros((3, G, 16), dtype=torch.int64)
    seg_of = [dp for dp, c in enumerate(SEG) for _ in range(c)]
    for i in range(N):
        if grp[i] >= 0 and 0 <= x[i] <= 15:
            exp[seg_of[i], grp[i], x[i]] += 1
    assert torch.equal(cnt, exp) and cnt.any()
    outs.append(cnt)
    it_plan = Q.sql_plan(_query(where, "v0 == v1 || v2 > v3", name="frequencyCount", select=["c2"]))
    op = Q.iter_operation("frequencyCount", QMIN, QMAX, BASE)
    rnd = enc.iterative_values_sql(op, Kd, SEG, it_plan, BASE, 0, [0] * G).cpu()
    assert torch.equal(rnd, model_round(x, grp, SEG, G, 0, [0] * G))
    outs.append(rnd)
    ids, n_groups = lr.cell_ids(Kd, plan)
    assert n_groups == G and ids.cpu().tolist() == [g if g >= 0 else G for g in grp]
    outs.append(ids.cpu())
    # the plain plan: today's outputs
    outs.append(enc.batch_values_sql("mean", Zd, Kd, SEG, plain).cpu())
    assert torch.equal(outs[-1], nt.group_moments(Zd[:, :1].contiguous(), Kd, SEG, moment_pairs("mean", 1), KEYS,
                                                  plain.where).cpu())
    return outs


# ----------------------------------------------------------------------------- windows and strides
def check_windows(device):
    """A predicate with two group windows (32 x 32 groups, the lin_reg d = 2 pair list) and K as a
    non-contiguous column view of a wider table."""
    pairs = moment_pairs("lin_reg", 3)
    assert nt.GROUP_MOMENTS_MAX_CELLS // len(pairs) < 1024 <= 2 * (nt.GROUP_MOMENTS_MAX_CELLS // len(pairs))
    g = torch.Generator().manual_seed(43)
    Z = torch.randint(-9, 10, (N, 3), generator=g)
    wide = torch.randint(-1, 33, (N, 8), generator=g)
    wide[:, 4] = torch.randint(-3, 4, (N,), generator=g)
    wide[-1, 2:4] = 31  # the last group, in the second window
    wide[-1, 4:6] = torch.tensor([2, 0])
    keys = [(0, 0, 32), (1, 0, 32)]
    filters, ops = [(2, 0), (3, 16)], (">", "<")
    f = lambda a: a[0] | a[1]  # noqa: E731
    Kd = wide.to(device)[:, 2:6]
    assert Kd.stride(0) == 8 and not Kd.is_contiguous()
    K = wide[:, 2:6].contiguous()
    keep = keep_of(K, filters, ops, f)
    grp = groups_of(K, keys, keep)
    assert grp[-1] == 1023 and 0 < keep.sum() < N
    got = nt.group_moments(Z.to(device), Kd, SEG, pairs, keys, filters, predicate=(ops, table_of(2, f))).cpu()
    assert got.shape == (3, 1024, len(pairs)) and torch.equal(got, model_moments(Z, grp, SEG, pairs, 1024))
    assert got[2, 1023].any()
    cells = nt.group_cells(Kd, N, keys, filters, predicate=(ops, table_of(2, f))).cpu()
    assert cells.tolist() == [c if c >= 0 else 1024 for c in grp]
    perm, start, n_groups = nt.lr_cell_plan(Kd, N, keys, filters, predicate=(ops, table_of(2, f)))
    assert n_groups == 1024 and int(start[-1]) == sum(c >= 0 for c in grp)
    return [got, cells, perm.cpu(), start.cpu()]


# ----------------------------------------------------------------------------- the cohort encoder
def check_lr_cells(device):
    """The logistic-regression encoder per cell of a plan with a predicate: every cell's vector is the ungrouped
    encoder's on the records the model selects (test_lr_cohort's exact inputs, so any order gives the same bits),
    for both level-2 layouts; ``!(v0 != v1)`` gives the equality plan's vectors."""
    from test_lr_cohort import exact_records, lr_params

    _, K = tables()
    X, y = exact_records(N, 3, 1)
    ops, f = ("<", ">="), lambda a: a[0] | a[1]  # noqa: E731
    plan = Q.SQLPlan([], [(0, 0), (3, 2)], [(1, 3)], 4, (ops, table_of(2, f)))
    grp = groups_of(K, KEYS, keep_of(K, plan.where, ops, f))
    outs = []
    for packing in (0, 1):
        lp = lr_params(3, N, packing=packing)
        got = lr.encode_coefficients_int_cells(X.to(device), y.to(device), K.to(device), lp, plan).cpu()
        for g in range(G):
            rows = [i for i in range(N) if grp[i] == g]
            assert len(rows) > 4 and torch.equal(got[g], lr.encode_coefficients_int(X[rows], y[rows], lp))
        outs.append(got)
    lp = lr_params(3, N)
    eq = Q.SQLPlan([], [(3, 2)], [(1, 3)], 4)
    ne = Q.SQLPlan([], [(3, 2)], [(1, 3)], 4, (("!=",), 0b01))
    a, b = (lr.encode_coefficients_int_cells(X.to(device), y.to(device), K.to(device), lp, p).cpu() for p in (eq, ne))
    assert torch.equal(a, b) and a.any()
    return outs + [a, b]


# ----------------------------------------------------------------------------- the host path
def test_lr_cells_host():
    assert len(check_lr_cells("cpu")) == 4


def test_atoms_host():
    assert len(check_atoms("cpu")) == 6 * 3 * 4


def test_formulas_host():
    assert len(check_formulas("cpu")) == (6 + 2 + 2 + 1 + 2 + 2) * 4


def test_plans_host():
    assert len(check_plans("cpu")) == 5


def test_windows_and_strides_host():
    assert len(check_windows("cpu")) == 4


def test_no_predicate_calls_the_entries_of_before(monkeypatch):
    """Without a predicate the bindings make the calls they made before: the same entries, the same arguments."""
    Z, K = tables()
    calls = []
    raw = nt._raw_call
    monkeypatch.setattr(nt, "_raw_call", lambda name, *a: calls.append((name, len(a))) or raw(name, *a))
    nt.group_moments(Z, K, SEG, moment_pairs("cosim", 3), KEYS, [(3, 1)])
    nt.group_cells(K, N, KEYS, [(3, 1)])
    nt.iter_round_cells("frequencyCount", K, SEG, 2, QMIN, QMAX, BASE, 0, [0] * G, KEYS, [(3, 1)])
    assert calls == [("dx_group_moments", 19), ("dx_group_cells", 11), ("dx_iter_round_cells", 20)]
    del calls[:]
    p = (("==",), 2)
    nt.group_moments(Z, K, SEG, moment_pairs("cosim", 3), KEYS, [(3, 1)], predicate=p)
    nt.group_cells(K, N, KEYS, [(3, 1)], predicate=p)
    nt.iter_round_cells("frequencyCount", K, SEG, 2, QMIN, QMAX, BASE, 0, [0] * G, KEYS, [(3, 1)], p)
    assert calls == [("dx_group_moments_pred", 20), ("dx_group_cells_pred", 12), ("dx_iter_round_cells_pred", 21)]


# ----------------------------------------------------------------------------- refusals
def test_binding_refusals():
    Z, K = tables()
    pairs = moment_pairs("cosim", 3)
    for call in (lambda **kw: nt.group_moments(Z, K, SEG, pairs, KEYS, kw.pop("filters", [(3, 1)]), **kw),
                 lambda **kw: nt.group_cells(K, N, KEYS, kw.pop("filters", [(3, 1)]), **kw),
                 lambda **kw: nt.lr_cell_plan(K, N, KEYS, kw.pop("filters", [(3, 1)]), **kw),
                 lambda **kw: nt.iter_round_cells("frequencyCount", K, SEG, 2, QMIN, QMAX, BASE, 0, [0] * G, KEYS,
                                                  kw.pop("filters", [(3, 1)]), **kw)):
        with pytest.raises(ValueError, match="2 operators for 1 filter terms"):
            call(predicate=(("==", "=="), 1))
        with pytest.raises(ValueError, match="0 operators for 1 filter terms"):
            call(predicate=((), 1))
        with pytest.raises(ValueError, match="unknown operator '='"):
            call(predicate=(("=",), 1))
        with pytest.raises(ValueError, match="unknown operator 0"):
            call(predicate=((0,), 1))
        with pytest.raises(ValueError, match="truth table outside"):
            call(predicate=(("==",), 4))
        with pytest.raises(ValueError, match="truth table outside"):
            call(predicate=(("==",), -1))
        with pytest.raises(ValueError, match="predicate without filter terms"):
            call(filters=[], predicate=((), 1))
        call(predicate=(("==",), 3))
    with pytest.raises(ValueError, match="truth table outside"):
        nt.group_cells(K, N, KEYS, TERMS8, predicate=(OPS8, 1 << 256))
    # the filters stay pairs, with the texts of before
    with pytest.raises(ValueError, match="filter terms"):
        nt.group_cells(K, N, KEYS, [(3, 1, 1)])


def test_entry_refusals():
    """set_terms below the bindings: a bad code, a table bit at or above 2^(2^n) and a predicate without a
    term return -2 from every entry, and nothing is written."""
    _, K = tables()
    cell = torch.full((N,), -7, dtype=torch.int64)
    out = torch.zeros((3, G, BASE), dtype=torch.int64)
    tiles = torch.tensor([[1, 0, 1], [2, 1, N]], dtype=torch.int64)
    pre = torch.zeros(G, dtype=torch.int64)
    kd = np.asarray(KEYS, dtype=np.int64).reshape(-1)
    Z = torch.zeros((N, 0), dtype=torch.int64)
    pairs = torch.zeros(2, dtype=torch.int16)
    mom = torch.zeros((3, G, 1), dtype=torch.int64)
    P = nt._P

    def entries(filters, pred):
        fd = np.asarray(list(filters) + [(0, 0)], dtype=np.int64).reshape(-1)
        pd = None if pred is None else np.asarray(pred, dtype=np.uint64).view(np.int64)
        pp = None if pd is None else pd.ctypes.data_as(P)
        n = len(filters)
        return [nt._raw_call("dx_group_cells_pred", 0, None, nt._ptr(K), 4, 4, N, kd.ctypes.data_as(P), 1,
                             fd.ctypes.data_as(P), n, nt._ptr(cell), pp),
                nt._raw_call("dx_group_moments_pred", 0, None, nt._ptr(Z), 0, 0, nt._ptr(K), 4, 4, nt._ptr(tiles), 2,
                             nt._ptr(pairs), 1, kd.ctypes.data_as(P), 1, fd.ctypes.data_as(P), n, 0, G, nt._ptr(mom),
                             pp),
                nt._raw_call("dx_iter_round_cells_pred", 0, None, nt._ptr(K), 4, 4, 2, nt._ptr(tiles), 2,
                             kd.ctypes.data_as(P), 1, fd.ctypes.data_as(P), n, QMIN, QMAX, BASE, BASE, nt._ptr(pre), 0,
                             G, nt._ptr(out), pp)]

    top = 1 << 63
    for filters, pred in (([(3, 1)], [6, 1, 0, 0, 0]), ([(3, 1)], [2 ** 64 - 1, 1, 0, 0, 0]),   # operator codes
                          ([(3, 1)], [0, 4, 0, 0, 0]), ([(3, 1)], [0, 1, 1, 0, 0]),            # 2 table bits
                          ([(3, 1)], [0, 1, 0, 0, top]), ([(3, 1), (0, 0)], [0, 0, 16, 0, 0, 0]),
                          ([(3, 1)] * 6, [0] * 6 + [0, 1, 0, 0]), ([(3, 1)] * 7, [0] * 7 + [0, 0, 1, 0]),
                          ([(3, 1)] * 7, [0] * 7 + [0, 0, 0, top]), ([], [1, 0, 0, 0])):           # no term
        assert entries(filters, pred) == [-2, -2, -2], (filters, pred)
    assert (cell == -7).all() and not out.any() and not mom.any()
    # the largest tables that fit, and NULL: the conjunction of equalities
    for filters, pred in (([(3, 1)], [0, 3, 0, 0, 0]), ([(3, 1)] * 6, [0] * 6 + [M64 - 1, 0, 0, 0]),
                          ([(3, 1)] * 7, [0] * 7 + [M64 - 1, M64 - 1, 0, 0]),
                          ([(3, 1)] * 8, [0] * 8 + [M64 - 1] * 4), ([(3, 1)], None), ([], None)):
        assert entries(filters, pred) == [0, 0, 0], (filters, pred)


REFUSED = {
    "set with no Where term": ([], "v0 == v1"),
    "unknown token '='": ([("c2", 1)], "v0 = v1"),
    "unknown token 'OR'": ([("c2", 1)], "v0 == v1 OR v0 == v1"),
    "unknown token '&'": ([("c2", 1), ("c3", 1)], "v0 == v1 & v2 == v3"),
    "malformed variable 'v01'": ([("c2", 1)], "v0 == v01"),
    "malformed variable 'v'": ([("c2", 1)], "v == v1"),
    "atom at v1 that is not v{2i} OP v{2i+1}": ([("c2", 1)], "v1 == v0"),
    "atom at v0 that is not": ([("c2", 1), ("c3", 1)], "v0 == v3 && v2 == v1"),
    "atom at v2 that is not": ([("c2", 1), ("c3", 1)], "v0 == v1 && v2"),
    "names v2, Where has 1 terms": ([("c2", 1)], "v0 == v1 && v2 == v3"),
    "uses the Where term 0 (v0) twice": ([("c2", 1)], "v0 == v1 || v0 != v1"),
    "never uses the Where term 1 (v2)": ([("c2", 1), ("c3", 1)], "v0 == v1"),
    "a ( is never closed": ([("c2", 1)], "(v0 == v1"),
    "a ) without its (": ([("c2", 1)], "v0 == v1)"),
    "where &&, || or ) is expected": ([("c2", 1), ("c3", 1)], "v0 == v1 v2 == v3"),
    "where an atom, ! or ( is expected": ([("c2", 1), ("c3", 1)], "v0 == v1 && || v2 == v3"),
    "ends where an atom is expected": ([("c2", 1)], "v0 == v1 &&"),
    "is empty": ([("c2", 1)], "   "),
    "longer than 256": ([("c2", 1)], "v0 == v1" + " " * 249),
    "a character outside ASCII": ([("c2", 1)], "v0 == v1 \u2228 v0 == v1"),
    "nests deeper than 16": ([("c2", 1)], "(" * 17 + "v0 == v1" + ")" * 17),
}


def test_check_parameters_refusals(env):
    from test_sql_query import _messages

    cl, node, client = env

    def survey(where, predicate):
        s = Q.QuerySQL(Where=[Q.WhereClear(n, str(v)) for n, v in where], Predicate=predicate, GroupBy=["c1"])
        return make_survey(client, cl, "mean", query_min=0, query_max=7, rows=3, group_by=(3,), sql=s)

    assert len("v0 == v1" + " " * 249) == 257
    for text, (where, predicate) in REFUSED.items():
        ok, seen = _messages(survey(where, predicate))
        assert not ok and len(seen) == 1, (text, seen)
        assert "SQL" in seen[0] and "only the conjunction" in seen[0] and text in seen[0], (text, seen)
    # the limits themselves pass: 256 characters, 16 parentheses, 8 terms
    assert _messages(survey([("c2", 1)], "v0 >= v1" + " " * 248)) == (True, [])
    assert _messages(survey([("c2", 1)], "(" * 16 + "v0 >= v1" + ")" * 16)) == (True, [])
    assert _messages(survey([("c2", 1)], "!" * 200 + "v0>=v1")) == (True, [])
    assert _messages(survey([(f"c{i}", i) for i in range(8)], FORMULAS8[0][1])) == (True, [])
    # a ninth term is refused by the cap of before
    ok, seen = _messages(survey([("c2", 1)] * 9, "v0 == v1"))
    assert not ok and "more than 8 terms" in seen[0]


# ----------------------------------------------------------------------------- the wire
def test_wire_and_dict_round_trip(env):
    cl, node, client = env
    s = Q.QuerySQL(Where=[Q.WhereClear("c2", "2"), Q.WhereClear("c3", "-1")], Predicate="v0 >= v1 || !(v2 == v3)",
                   GroupBy=["c1"])
    kw = dict(query_min=0, query_max=7, rows=3, group_by=(3,), survey_id="same")
    sq = make_survey(client, cl, "mean", sql=s, **kw)
    back = wm.survey_query_from_wire(wm.survey_query_to_wire(sq))
    assert back.Query.SQL == s and back.Query.SQL.Predicate == "v0 >= v1 || !(v2 == v3)"
    assert wm.survey_query_to_wire(back) == wm.survey_query_to_wire(sq)
    assert Q.SurveyQuery.from_dict(sq.to_dict()).Query.SQL == s
    assert Q.sql_plan(back.Query) == Q.sql_plan(sq.Query) and Q.sql_plan(back.Query).predicate[0] == (">=", "==")
    # without a predicate: the bytes and the dict of a survey whose field was never touched
    t = copy.deepcopy(s)
    t.Predicate = ""
    plain = make_survey(client, cl, "mean", sql=t, **kw)
    old = make_survey(client, cl, "mean", sql=Q.QuerySQL(Where=copy.deepcopy(s.Where), GroupBy=["c1"]), **kw)
    assert wm.survey_query_to_wire(plain) == wm.survey_query_to_wire(old) != wm.survey_query_to_wire(sq)
    assert plain.to_dict() == old.to_dict()
    assert len(wm.survey_query_to_wire(sq)) > len(wm.survey_query_to_wire(plain))


# ----------------------------------------------------------------------------- end to end
WHERE = [("c2", 2), ("c3", 1)]
PREDICATE = "v0 >= v1 || v2 == v3"


def passes(row):
    """The test's own reading of WHERE: c2 >= 2 or c3 == 1."""
    return row[2] >= 2 or row[3] == 1


def sql(select=()):
    return Q.QuerySQL(Select=list(select), Where=[Q.WhereClear(n, str(v)) for n, v in WHERE], Predicate=PREDICATE,
                      GroupBy=["c1"])


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    cl, node = local_cluster(3, 5, 3, device="cpu", workdir=str(tmp_path_factory.mktemp("db")))
    yield cl, node, DrynxClient(node)
    node.close(remove=True)


def generated_cells(cl, sq):
    """[group][records]: c0 of the generated tables' rows that pass, by c1; every kind of row is present."""
    plan = Q.sql_plan(sq.Query)
    assert plan.width == 4 and plan.predicate == ((">=", "=="), 0b1110)
    cells = [[] for _ in range(3)]
    kinds = set()
    for dp in cl.dps:
        for r in dcp.generate_sql_table(sq, dp.id, plan).tolist():
            kinds.add((r[2] >= 2, r[3] == 1))
            if passes(r):
                cells[r[1]].append(r[0])
    assert len(kinds) == 4 and all(cells)
    return cells


def check_mean(cl, node, client, device, proofs):
    kw = dict(proofs=1, ranges=[16, 5], sig_device=device) if proofs else {}
    sq = make_survey(client, cl, "mean", query_min=0, query_max=7, rows=24, group_by=(3,), sql=sql(),
                     survey_id=f"predicate-mean-{proofs}", **kw)
    assert Q.check_parameters(sq, False)
    cells = generated_cells(cl, sq)
    keys, vals, res = client.send_survey_query(sq)
    assert keys == ["[0]", "[1]", "[2]"]
    clear = [[sum(v[g][k] for v in res.clear_dp.values()) for k in range(2)] for g in range(3)]
    assert clear == [[sum(c), len(c)] for c in cells]
    for v, c in zip(vals, cells):
        assert v == [pytest.approx(sum(c) / len(c), rel=1e-12)]
    if proofs:
        codes = res.block.data_block().Proofs
        assert set(codes.values()) == {prq.PROOF_TRUE} and len(codes) == 3 * (5 + 3 + 3)
    return vals


def check_counts(cl, node, client):
    sq = make_survey(client, cl, "frequencyCount", query_min=0, query_max=7, rows=24, group_by=(3,), sql=sql(),
                     survey_id="predicate-counts")
    cells = generated_cells(cl, sq)
    keys, vals, _ = client.send_survey_query(sq)
    assert keys == ["[0]", "[1]", "[2]"] and vals == [[float(c.count(v)) for v in range(8)] for c in cells]


def check_median(cl, node, client):
    """The per-cell median over 0..99, one base-10 digit per round."""
    sq = make_iterative_survey(client, cl, "frequencyCount", 10, query_min=0, query_max=99, rows=24, group_by=(3,),
                               sql=sql(), survey_id="predicate-median")
    cells = generated_cells(cl, client.iterative_round_query(sq, 10, 0, [0, 0, 0], sq.SurveyID))
    values, rnds = client.send_iterative_quantile(sq, 10, 1, 2)
    assert len(rnds) == 2 and [sum(c) for c in rnds[0].client_out] == [len(c) for c in cells]
    assert values == [float(sorted(c)[max(1, (len(c) + 1) // 2) - 1]) for c in cells]
    return values


def check_lr_cohorts(cl, node, client):
    """One model per cell: the packed coefficients are those of the ungrouped encoder on the cell's records."""
    from test_lr_cohort import expected_weights, lr_params

    lp = lr_params(3, 30)
    sq = make_survey(client, cl, "logistic regression", lr_params=lp, rows=30, group_by=(3,), sql=sql(),
                     survey_id="predicate-cohorts")
    assert Q.check_parameters(sq, False)
    plan = Q.sql_plan(sq.Query)
    tot = [torch.zeros(sq.Query.Operation.NbrOutput, dtype=torch.int64) for _ in range(3)]
    count = [0, 0, 0]
    for dp in cl.dps:
        X, y = dcp.generate_lr_data(lp, torch.device("cpu"), torch.Generator().manual_seed(
            dcp._seed(sq.SurveyID, dp.id)))
        K = dcp.generate_lr_keys(sq, dp.id, plan, 30).tolist()
        for g in range(3):
            rows = [i for i, r in enumerate(K) if passes(r) and r[1] == g]
            if rows:
                tot[g] += lr.encode_coefficients_int(X[rows], y[rows], lp)
                count[g] += len(rows)
    assert all(n > 4 for n in count)
    keys, vals, _ = client.send_survey_query(sq)
    assert keys == ["[0]", "[1]", "[2]"]
    assert [[int(x) for x in v] for v in client.last_plaintexts] == [t.tolist() for t in tot]
    for g in range(3):
        assert lr.cohort_records(tot[g].tolist(), lp) == count[g]
        exp = expected_weights(tot[g].tolist(), lp, count[g])
        assert len(vals[g]) == 4 and all(a == b and not math.isnan(a) for a, b in zip(vals[g], exp))


def test_mean_and_counts_end_to_end(env):
    check_mean(*env, "cpu", False)
    check_counts(*env)


def test_mean_with_proofs_end_to_end(env):
    check_mean(*env, "cpu", True)


def test_lr_cohorts_end_to_end(env):
    check_lr_cohorts(*env)


def test_median_per_cell_end_to_end(env):
    check_median(*env)
