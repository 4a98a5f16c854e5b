"""Iterative rounds over SQL cohorts (one search per cell of a WHERE / GROUP
BY): the grouped digit histogram (dx_iter_round_cells) against a pure-Python
model of the specification, K14d's counts, the one-shot SQL histogram and K14c;
group windows, contention and several tiles; the C entry below the binding; the
query rules and the wire; per-cell quantile and extreme searches end to end
(fixed and generated tables, with proofs, an inconsistent DP), and two gloo
ranks through the tool.  The checks shared with the GPU suite live here and
take a device."""
import copy
import json
import math
import os
import subprocess
import sys
import time

import pytest
import torch

import test_iter_quantile as tq
from drynx_amd import native as nt
from drynx_amd import query as Q
from drynx_amd import rounds
from drynx_amd.ops import encoding as enc
from drynx_amd.proofs import requests as prq
from drynx_amd.protocols import data_collection as dcp
from drynx_amd.services.api import DrynxClient
from drynx_amd.services.local import local_cluster, make_iterative_survey, make_survey

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- the model (from the specification)
def cell_of(row, keys, filters):
    """The cell of a table row: None if a filter term fails or a key digit is outside its cardinality."""
    if any(row[c] != v for c, v in filters):
        return None
    g = 0
    for c, off, card in keys:
        d = row[c] - off
        if not 0 <= d < card:
            return None
        g = g * card + d
    return g


def cell_records(dps, xcol, keys, filters, G):
    """Per DP and cell the counted column of the cell's rows."""
    out = []
    for rows in dps:
        cells = [[] for _ in range(G)]
        for r in rows:
            g = cell_of(r, keys, filters)
            if g is not None:
                cells[g].append(r[xcol])
        out.append(cells)
    return out


def model_cells(recs, qmin, qmax, b, L, k, prefixes):
    """[n_dp][G][b]: test_iter_quantile.model_row's arithmetic per DP and cell under the cell's prefix."""
    return [[tq.model_row(c, qmin, qmax, b, L, k, prefixes[g]) if c else [0] * b for g, c in enumerate(cells)]
            for cells in recs]


def unary_rows(counts, is_max):
    """K14b's unary rule for v = the first (min) / last (max) occupied digit; all zero without one."""
    occ = [i for i, c in enumerate(counts) if c]
    if not occ:
        return [0] * len(counts)
    return [int(i < occ[-1]) if is_max else int(i >= occ[0]) for i in range(len(counts))]


SEG_ROWS = [0, 1, 63, 64, 65, 130, 0, 200]
DOMAINS = [(-7, 1000, 10), (3, 4097, 16), (0, 1, 2), (5, 5000, 4096)]  # (qmin, R, b)
KEYS, FILTERS, G = [(1, 0, 2), (2, 0, 3)], [(3, 1)], 6
EMPTY_CELL, MISSED_CELL = 5, 1
PLAN = Q.SQLPlan(select=[0], where=[(3, 1)], group_by=[(1, 2), (2, 3)], width=4)


def table_for(seg_rows, qmin, qmax, b, seed):
    """Per DP the rows (x, k1, k2, f) of a table: x is test_iter_quantile's (one below the domain, one above,
    one at QueryMin, one at QueryMax -- those four rows pass the filter in cell 0), k1 in [-1, 2] over the
    cardinality 2 and k2 in [-1, 3] over 3 (a digit of -1 and of the cardinality is dropped), f in {0, 1} with
    f == 1 kept; cell 5 is emptied."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for xs in tq.records_for(seg_rows, qmin, qmax, b, seed):
        n = len(xs)
        k1 = torch.randint(-1, 3, (n,), generator=g).tolist()
        k2 = torch.randint(-1, 4, (n,), generator=g).tolist()
        f = torch.randint(0, 4, (n,), generator=g).clamp(max=1).tolist()
        rows = []
        for x, a, c, w in zip(xs, k1, k2, f):
            if x in (qmin - 3, qmax + 5, qmin, qmax):
                a, c, w = 0, 0, 1
            if (a, c) == (1, 2):
                c = 0
            rows.append([x, a, c, w])
        out.append(rows)
    return out


def to_strided(dps, device, width=4):
    """The rows as a strided view [rows, width] (row stride width + 3) of a wider tensor."""
    flat = [r for rows in dps for r in rows]
    wide = torch.full((len(flat), width + 3), 1 << 61, dtype=torch.int64)
    if flat:
        wide[:, 1: 1 + width] = torch.tensor(flat, dtype=torch.int64)
    K = wide.to(device)[:, 1: 1 + width]
    assert K.stride(0) == width + 3 or K.shape[0] < 2
    return K


def walk_prefixes(recs, qmin, qmax, b, L):
    """[L][G]: in round k every cell under the prefix of its own median walk; an empty cell keeps 0; cell
    MISSED_CELL gets, from round 1 on, a prefix none of its records matches (where the domain has one)."""
    ncell = len(recs[0])
    digits = []
    for g in range(ncell):
        per_dp = [cells[g] for cells in recs]
        inside = [x for c in per_dp for x in c if qmin <= x <= qmax]
        digits.append(tq.model_walk(per_dp, qmin, qmax, b, 1, 2) if inside else [0] * L)
    out = []
    for k in range(L):
        ps = [sum(d * b ** (k - 1 - j) for j, d in enumerate(digits[g][:k])) for g in range(ncell)]
        if k:
            seen = {(x - qmin) // b ** (L - k) for cells in recs for x in cells[MISSED_CELL] if qmin <= x <= qmax}
            miss = next((p for p in range(b ** k) if p not in seen), None)
            if miss is not None:
                ps[MISSED_CELL] = miss
        out.append(ps)
    return out


def check_rows(device):
    """nt.iter_round_cells == the model in every round with per-cell prefixes; round 0 against K14d's counts
    of the in-domain rows, the last round against the one-shot SQL histogram, min / max against the unary
    rule on the model counts; without terms and with one prefix it is nt.iter_round."""
    out = []
    for n, (qmin, R, b) in enumerate(DOMAINS):
        qmax = qmin + R - 1
        dps = table_for(SEG_ROWS, qmin, qmax, b, 41 + n)
        flat = [r[0] for rows in dps for r in rows]
        assert min(flat) < qmin and max(flat) > qmax and qmin in flat and qmax in flat
        K = to_strided(dps, device)
        recs = cell_records(dps, 0, KEYS, FILTERS, G)
        assert not any(cells[EMPTY_CELL] for cells in recs)
        assert R == 1 or any(cells[MISSED_CELL] for cells in recs)  # (R = 1: every row is the QueryMin one)
        L = tq.model_rounds(R, b)
        prefixes = walk_prefixes(recs, qmin, qmax, b, L)
        assert R <= 8 * b or len(set(prefixes[L - 1])) > 2  # the cells walk different paths
        classic = enc.batch_values_sql("frequencyCount", K[:, :1], K, SEG_ROWS, PLAN, qmin, qmax).cpu()
        assert classic.shape == (len(SEG_ROWS), G, R)
        for k in range(L):
            ps = prefixes[k]
            got = nt.iter_round_cells("frequencyCount", K, SEG_ROWS, 0, qmin, qmax, b, k, ps, KEYS, FILTERS)
            assert got.dtype == torch.int64 and got.shape == (len(SEG_ROWS), G, b) and got.device == K.device
            want = model_cells(recs, qmin, qmax, b, L, k, ps)
            assert got.cpu().tolist() == want, (qmin, R, b, k)
            if k == 0:  # K14d's counts of the in-domain rows
                assert torch.equal(got.sum(2).cpu(), classic.sum(2))
            if k and L > 1:
                assert not got[:, MISSED_CELL].any()
            out.append(got.cpu())
            for name in ("min", "max"):
                rows = nt.iter_round_cells(name, K, SEG_ROWS, 0, qmin, qmax, b, k, ps, KEYS, FILTERS).cpu()
                assert rows.tolist() == [[unary_rows(c, name == "max") for c in cells] for cells in want]
                out.append(rows)
        last = torch.zeros((len(SEG_ROWS), G, b), dtype=torch.int64)
        for g, p in enumerate(prefixes[L - 1]):
            cut = classic[:, g, p * b: p * b + b]
            last[:, g, : cut.shape[1]] = cut
        assert torch.equal(out[-3], last)
        # no keys, no filters, one prefix: K14c's counts of the same x
        for k in (0, L - 1):
            p = [prefixes[k][0]]
            one = nt.iter_round_cells("frequencyCount", K, SEG_ROWS, 0, qmin, qmax, b, k, p)
            assert torch.equal(one[:, 0], nt.iter_round("frequencyCount", K[:, :1], SEG_ROWS, qmin, qmax, b, k, p[0]))
    return out


def check_windows(device):
    """More groups than one launch's LDS counters hold: b = 4096 with cap // b + 1 groups (two windows, the
    last ragged), b = 2 with 4096 groups and with cap // 2 + 1 (two windows again); about 600 rows over 3 DPs,
    a record in the first and the last group of every window, distinct prefixes."""
    cap = nt.lib().dx_iter_round_max_counters()
    assert cap == nt.ITER_ROUND_MAX_COUNTERS == 160 * 1024 // 2 // 4
    out = []
    for b, ncell, R in ((4096, cap // 4096 + 1, 8 * 4096), (2, 4096, 64), (2, cap // 2 + 1, 64)):
        gw = cap // b
        assert ncell <= gw or (ncell > gw and ncell % gw)  # one window, or several with a ragged last one
        gen = torch.Generator().manual_seed(b + ncell)
        seg = [199, 0, 401]
        x = torch.randint(-2, R + 2, (600,), generator=gen).tolist()
        key = torch.randint(-1, ncell + 1, (600,), generator=gen).tolist()
        edges = sorted({0, ncell - 1} | {g for w in range(0, ncell, gw) for g in (w, min(w + gw, ncell) - 1)})
        for i, g in enumerate(edges):
            key[i], x[i] = g, (g * 7919) % R
            key[300 + i], x[300 + i] = g, (g * 104729 + 5) % R
        dps = [[[7, x[i], key[i]] for i in range(0, 199)], [], [[7, x[i], key[i]] for i in range(199, 600)]]
        K = to_strided(dps, device, 3)
        keys = [(2, 0, ncell)]
        recs = cell_records(dps, 1, keys, [], ncell)
        L = tq.model_rounds(R, b)
        k = L - 1
        hi = b  # lo = 1 in the last round
        ps = [(x[i] // hi) if (i := next((j for j in range(600) if key[j] == g and 0 <= x[j] < R), None)) is not None
              else g % (R // hi) for g in range(ncell)]
        assert len(set(ps)) > 4
        got = nt.iter_round_cells("frequencyCount", K, seg, 1, 0, R - 1, b, k, ps, keys).cpu()
        assert got.tolist() == model_cells(recs, 0, R - 1, b, L, k, ps)
        assert all(int(got[:, g].sum()) > 0 for g in edges)
        out.append(got)
    return out


def check_contention(device):
    """One DP of 70000 rows (several tiles), G = 3, b = 1000: uniform, then every row in one cell and one
    digit, whose counter holds 70000."""
    qmin, R, b, n = 0, 10 ** 6, 1000, 70_000
    gen = torch.Generator().manual_seed(5)
    keys, out = [(1, 0, 3)], []
    plan, _ = nt._tile_plan(torch.tensor([n]).numpy(), min(3 * b, 2048))
    assert len(plan) > 1 and int((plan[:, 2] - plan[:, 1]).min()) >= 368
    for xs, ks in ((torch.randint(-5, R + 5, (n,), generator=gen).tolist(),
                    torch.randint(-1, 4, (n,), generator=gen).tolist()), ([123_456] * n, [2] * n)):
        dps = [[[x, c] for x, c in zip(xs, ks)]]
        K = torch.tensor(dps[0], dtype=torch.int64).to(device)
        recs = cell_records(dps, 0, keys, [], 3)
        for k, ps in ((0, [0, 0, 0]), (1, [500, 7, 123])):
            got = nt.iter_round_cells("frequencyCount", K, [n], 0, qmin, R - 1, b, k, ps, keys).cpu()
            assert got.tolist() == model_cells(recs, qmin, R - 1, b, 2, k, ps)
            out.append(got)
    assert out[2][0, 2, 123] == n and out[3][0, 2, 456] == n and int(out[3].sum()) == n
    return out


def test_rows_equal_the_model():
    check_rows("cpu")


def test_windows():
    check_windows("cpu")


def test_contention_and_tiles():
    check_contention("cpu")


def test_binding_argument_checks():
    K = torch.zeros((3, 2), dtype=torch.int64)

    def call(seg=(3,), xcol=0, qmax=999, base=10, rnd=0, prefixes=(0, 0), keys=((1, 0, 2),), name="frequencyCount"):
        return nt.iter_round_cells(name, K, list(seg), xcol, 0, qmax, base, rnd, list(prefixes), list(keys))

    assert call().tolist() == [[[3] + [0] * 9, [0] * 10]]
    for bad in (dict(base=1), dict(base=4097), dict(rnd=3), dict(rnd=-1), dict(prefixes=(0,)), dict(prefixes=(0, 0, 0)),
                dict(prefixes=(0, 1)), dict(prefixes=(0, 10), rnd=1), dict(prefixes=(-1, 0), rnd=1),
                dict(qmax=1 << 40), dict(seg=[2]), dict(xcol=2), dict(xcol=-1), dict(keys=[(2, 0, 2)]),
                dict(name="sum"), dict(name="max", base=4097),
                dict(keys=[(1, 0, 1 << 19)], prefixes=[0] * (1 << 19), base=4)):  # G * b > 1 << 20
        with pytest.raises(ValueError):
            call(**bad)
    assert call(rnd=2, prefixes=(99, 0)).shape == (1, 2, 10)
    assert nt.iter_round_cells("min", K[:0], [], 0, 0, 9, 10, 0, [0]).shape == (0, 1, 10)
    none = nt.iter_round_cells("max", K[:0], [0, 0], 0, 0, 9, 10, 0, [0, 0], [(1, 0, 2)])  # two DPs without rows
    assert none.tolist() == [[[0] * 10] * 2] * 2
    assert rounds.ITER_MAX_CELL_OUTPUTS == 1 << 20 == Q.ITER_MAX_CELL_OUTPUTS


def test_entry_below_the_binding():
    """The C entry's own checks (-2) on the host, hostile prefixes, and the shared term checker in K14d."""
    K = torch.tensor([[0, 0], [15, 0], [25, 1], [999, 1], [1000, 1], [-1, 0], [7, 2]], dtype=torch.int64)
    tiles = torch.tensor([0, 0, 7], dtype=torch.int64)
    cap = nt.lib().dx_iter_round_max_counters()
    out = torch.zeros((1, 1 << 20), dtype=torch.int64)
    pre = torch.zeros(1 << 19, dtype=torch.int64)
    P = nt._P

    def rc(CK=2, xcol=0, tl=tiles, n_tiles=1, keys=(1, 0, 2), n_keys=1, filters=(), n_filters=0, qmax=999, base=10,
           lo=100, g0=0, gw=2):
        out.zero_()
        kd, fd = torch.tensor(keys, dtype=torch.int64), torch.tensor(list(filters) + [0], dtype=torch.int64)
        return nt._raw_call("dx_iter_round_cells", 0, None, nt._ptr(K), 2, CK, xcol, nt._ptr(tl), n_tiles,
                            kd.numpy().ctypes.data_as(P), n_keys, fd.numpy().ctypes.data_as(P), n_filters, 0, qmax,
                            base, lo, nt._ptr(pre), g0, gw, nt._ptr(out))

    assert rc() == 0 and out[0, :20].tolist() == [2] + [0] * 9 + [1] + [0] * 8 + [1]
    assert rc(g0=1, gw=1) == 0 and out[0, :20].tolist() == [0] * 10 + [1] + [0] * 8 + [1]  # the other group ignored
    assert rc(lo=10) == 0 and out[0, :20].tolist() == [1, 1] + [0] * 8 + [0, 0, 1] + [0] * 7
    # the terms, through the shared checker
    assert rc(keys=(2, 0, 2)) == -2 and rc(keys=(-1, 0, 2)) == -2 and rc(keys=(1, 0, 0)) == -2
    assert rc(keys=(1, 0, (1 << 24) + 1)) == -2 and rc(n_keys=-1) == -2 and rc(n_filters=9) == -2
    assert rc(keys=(1, 0, 2) * 5, n_keys=5) == -2  # four keys beside the counted column
    assert rc(filters=(2, 0), n_filters=1) == -2 and rc(filters=(1, 1), n_filters=1) == 0
    assert rc(CK=-1) == -2
    # xcol, the round, G * base, the window, the counts, the tile length
    assert rc(xcol=2) == -2 and rc(xcol=-1) == -2
    assert rc(base=1, lo=1) == -2 and rc(base=4097, lo=1) == -2 and rc(base=4096, lo=1, gw=2) == 0
    assert rc(lo=1000) == -2 and rc(lo=0) == -2 and rc(lo=50) == -2 and rc(qmax=1 << 40) == -2 and rc(qmax=-1) == -2
    assert rc(keys=(1, 0, 1 << 19), base=4, lo=256, gw=1) == -2          # G * base = 2^21
    assert rc(keys=(1, 0, 1 << 18), base=4, lo=256, gw=1) == 0
    assert rc(g0=-1) == -2 and rc(gw=0) == -2 and rc(g0=1, gw=2) == -2 and rc(g0=2, gw=1) == -2
    assert rc(keys=(1, 0, 1 << 14), base=2, lo=512, gw=cap // 2 + 1) == -2 and \
        rc(keys=(1, 0, 1 << 14), base=2, lo=512, gw=cap // 2) == 0
    assert rc(n_tiles=-1) == -2 and rc(n_tiles=1 << 31) == -2
    assert rc(tl=torch.tensor([0, 0, 1 << 31], dtype=torch.int64)) == -2  # the 32-bit counters could wrap
    assert rc(n_tiles=0) == 0 and not out.any()
    # a prefix the entry cannot see: -1 and 2^62 match nothing and touch nothing else
    for hostile in (-1, 1 << 62):
        pre[1] = hostile
        assert rc(lo=10) == 0 and out[0, :20].tolist() == [1, 1] + [0] * 18 and not out[0, 20:].any()
        pre[0], pre[1] = hostile, 2
        assert rc(lo=1) == 0 and out[0, :20].tolist() == [0] * 10 + [0, 0, 0, 0, 0, 1] + [0] * 4  # 25 under 2
        pre[:2] = 0
    # K14d refuses the same bad terms it refused before the checker moved
    Z, o2 = torch.zeros((7, 0), dtype=torch.int64), torch.zeros(64, dtype=torch.int64)
    pairs = torch.zeros(2, dtype=torch.int16)

    def gm(CK=2, keys=(1, 0, 2), n_keys=1, filters=(), n_filters=0, g0=0, gw=2):
        kd, fd = torch.tensor(keys, dtype=torch.int64), torch.tensor(list(filters) + [0], dtype=torch.int64)
        return nt._raw_call("dx_group_moments", 0, None, nt._ptr(Z), 0, 0, nt._ptr(K), 2, CK, nt._ptr(tiles), 1,
                            nt._ptr(pairs), 1, kd.numpy().ctypes.data_as(P), n_keys, fd.numpy().ctypes.data_as(P),
                            n_filters, g0, gw, nt._ptr(o2))

    assert gm() == 0 and o2[:2].tolist() == [3, 3]
    assert gm(keys=(2, 0, 2)) == -2 and gm(keys=(-1, 0, 2)) == -2 and gm(keys=(1, 0, 0)) == -2
    assert gm(keys=(1, 0, (1 << 24) + 1)) == -2 and gm(n_keys=6) == -2 and gm(n_keys=-1) == -2
    assert gm(n_filters=9) == -2 and gm(filters=(2, 0), n_filters=1) == -2 and gm(CK=-1) == -2 and gm(g0=1) == -2


# ----------------------------------------------------------------------------- query rules and the wire
@pytest.fixture(scope="module")
def env(tmp_path_factory):
    cl, node = local_cluster(3, 5, 3, device="cpu", workdir=str(tmp_path_factory.mktemp("db")))
    yield cl, node, DrynxClient(node)
    node.close(remove=True)


def sql(group_by=("c1",), where=(("c2", "1"),)):
    return Q.QuerySQL(Where=[Q.WhereClear(n, v) for n, v in where], GroupBy=list(group_by))


def _round(env, name="frequencyCount", base=10, k=0, prefixes=(0, 0, 0), group_by=(3,), s=None, qmax=99):
    cl, node, client = env
    sq = make_iterative_survey(client, cl, name, base, query_min=0, query_max=qmax, rows=4, group_by=group_by,
                               sql=s if s is not None else sql())
    return client.iterative_round_query(sq, base, k, list(prefixes), "it")


def test_check_parameters(env):
    from test_sql_query import _messages

    ok = _round(env)
    assert _messages(ok) == (True, []) and ok.IterPrefixes == [0, 0, 0] and ok.IterPrefix == 0
    assert ok.Query.Operation.NbrOutput == 10 and ok.SurveyID == "it.r0"
    assert _messages(_round(env, prefixes=[0], group_by=(3, 2), s=sql(()))) == (True, [])   # G = 1, WHERE only
    assert _messages(_round(env, "min", prefixes=[0] * 6, group_by=(3, 2), s=sql(("c1", "c3")))) == (True, [])
    assert _messages(_round(env, "max", k=1, prefixes=[9, 0, 4])) == (True, [])

    def refused(sq0=ok, text="SQL with iterative rounds", **kw):
        sq = copy.deepcopy(sq0)
        for k, v in kw.items():
            obj, _, attr = k.rpartition("__")
            tgt = sq
            for part in filter(None, obj.split("__")):
                tgt = getattr(tgt, part)
            setattr(tgt, attr, v)
        good, seen = _messages(sq)
        return not good and any(text in m for m in seen)

    assert refused(IterPrefixes=[]) and refused(IterPrefixes=[0, 0]) and refused(IterPrefixes=[0] * 4)
    assert refused(IterRound=1, IterPrefixes=[0, 10, 0]) and refused(IterRound=1, IterPrefixes=[0, -1, 0])
    assert refused(IterPrefixes=[0, 1, 0]) and refused(IterPrefixes=[0, True, 0]) and refused(IterPrefixes=[0, 0.0, 0])
    assert refused(IterPrefix=1, IterRound=1, IterPrefixes=[0, 0, 0])
    # a round off the wire that is no round of the domain is refused without its power being taken (10^(2^62)
    # has no representation; 10^(10^7) alone took 22 s): the whole check is a few comparisons per cell
    for k in (2, 10 ** 7, 1 << 62, -(1 << 62)):
        t0 = time.perf_counter()
        assert refused(text="iterative round outside 0..1", IterRound=k, IterPrefixes=[0, 5, 0])
        assert time.perf_counter() - t0 < 1.0
    assert refused(text="iterative rounds over", IterRound=1 << 62, Query__Operation__QueryMax=1 << 41,
                   Query__DPDataGen__GenerateDataMax=1 << 41)
    assert refused(text="defined for min, max and frequencyCount", Query__Operation__NameOp="sum")
    assert refused(text="cutting factor", Query__CuttingFactor=2)
    # G * b > 1 << 20: 4096 cells of 512 outputs
    big = _round(env, base=512, prefixes=[0] * 4096, group_by=(64, 64), s=sql(("c1", "c3")), qmax=511)
    assert refused(big, text="4096 cells of 512 outputs")
    assert _messages(_round(env, base=256, prefixes=[0] * 4096, group_by=(64, 64), s=sql(("c1", "c3")),
                            qmax=255)) == (True, [])
    # over cells min / max are derived from counts: the counting base limit
    assert refused(_round(env, "max", 4096, qmax=9999), text="iterative base outside 2..4096", IterBase=4097,
                   Query__Operation__NbrOutput=4097)
    # without SQL the list must be empty, and nothing else changes
    plain = make_iterative_survey(env[2], env[0], "max", 10, query_min=0, query_max=99, rows=4)
    rq = env[2].iterative_round_query(plain, 10, 1, 7, "it")
    assert _messages(rq) == (True, []) and rq.IterPrefixes == [] and rq.IterPrefix == 7
    assert refused(rq, text="IterPrefixes", IterPrefixes=[7])
    classic = make_survey(env[2], env[0], "max", query_min=0, query_max=9, rows=4)
    assert refused(classic, text="without a base", IterPrefixes=[0])
    # the one message of the issue: a min survey with GroupBy, a base and no list
    sq = make_survey(env[2], env[0], "min", query_min=0, query_max=7, rows=3, group_by=(3,), sql=sql(where=()))
    sq.IterBase, sq.Query.Operation.NbrOutput = 2, 2
    good, seen = _messages(sq)
    hits = [m for m in seen if "SQL" in m or "column" in m]
    assert not good and len(hits) == 1 and "iterative" in hits[0] and "one entry per cell (3)" in hits[0]


def test_wire_and_dict(env):
    from drynx_amd.wire import messages as M
    from drynx_amd.wire import onet

    sq = _round(env, "min", k=1, prefixes=[9, 0, 4])
    sq.IterSurveyID = "search-7"
    assert onet.QUERY_SQL[-1] == ("IterPrefixes", ("rep", "sint"))
    for back in (M.survey_query_from_wire(M.survey_query_to_wire(sq)), Q.SurveyQuery.from_dict(sq.to_dict()),
                 Q.SurveyQuery.from_dict(json.loads(json.dumps(sq.to_dict())))):
        assert (back.IterBase, back.IterRound, back.IterPrefix, back.IterPrefixes) == (10, 1, 0, [9, 0, 4])
        assert back.IterSurveyID == "search-7" and back.Query.SQL == sq.Query.SQL
        assert Q.check_parameters(back, False)
    assert len(M.survey_query_to_wire(sq)) > len(M.survey_query_to_wire(_round(env, "min", k=1, prefixes=[0, 0, 0])))
    # an iterative survey without SQL: the bytes and the dict of today (the field is not encoded)
    plain = make_iterative_survey(env[2], env[0], "max", 10, query_min=0, query_max=99, rows=4)
    rq = env[2].iterative_round_query(plain, 10, 1, 7, "it")
    wire = M.survey_query_to_wire(rq)
    assert M.survey_query_to_wire(M.survey_query_from_wire(wire)) == wire
    assert "IterPrefixes" not in rq.to_dict() and M.survey_query_from_wire(wire).IterPrefixes == []
    msg = M.survey_query_to_msg(rq)
    assert msg["Query"]["SQL"].pop("IterPrefixes") == []
    from drynx_amd.wire import protobuf as pb
    assert wire == onet.message_type_id("libdrynx.SurveyQuery") + pb.encode(onet.SURVEY_QUERY_ITER, msg)
    grouped = make_survey(env[2], env[0], "mean", query_min=0, query_max=7, rows=3, group_by=(3,), sql=sql())
    assert "IterPrefixes" not in grouped.to_dict() and "IterPrefixes" not in grouped.to_dict()["Query"]["SQL"]
    old_sql = tuple(f for f in onet.QUERY_SQL if f[0] != "IterPrefixes")
    old_query = tuple((n, ("msg", old_sql)) if n == "SQL" else (n, k) for n, k in onet.QUERY)
    old = tuple((n, ("msg", old_query)) if n == "Query" else (n, k) for n, k in onet.SURVEY_QUERY_ITER)
    for s in (grouped, rq):  # the schema without the field encodes every survey of today to the same bytes
        assert M.survey_query_to_wire(s) == \
            onet.message_type_id("libdrynx.SurveyQuery") + pb.encode(old, M.survey_query_to_msg(s))


# ----------------------------------------------------------------------------- searches end to end
# (x, c1, c2) per DP: ties, an empty DP, cell 1 with one record, cell 2 with none (its one row fails WHERE), a
# key outside the cardinality
FIXED = [[(20, 0, 1), (37, 0, 1), (99, 0, 1), (50, 0, 0), (5, 1, 0)],
         [(99, 0, 1), (5, 0, 1), (42, 1, 1)],
         [],
         [(98, 0, 1), (98, 0, 1), (1, 0, 1), (7, 2, 0)],
         [(99, 0, 1), (64, 3, 1)]]
QUANTILES = [(0, 1), (1, 4), (1, 2), (3, 4), (1, 1)]


def fixed_tables(cl, tables, lo=0, device="cpu"):
    return {dp.id: [torch.tensor([r[c] + (lo if c == 0 else 0) for r in tables[i]], dtype=torch.int64).to(device)
                    for c in range(3)] for i, dp in enumerate(cl.dps)}


def fixed_cells(tables, lo=0, ncell=3):
    return [[r[0] + lo for t in tables for r in t if r[2] == 1 and r[1] == g] for g in range(ncell)]


def _same(a, b):
    assert len(a) == len(b) and all((math.isnan(x) and math.isnan(y)) or x == y for x, y in zip(a, b)), (a, b)


def check_search_fixed(cl, node, client, device, qmin, qmax, base):
    """Per-cell quantiles against the sorted per-cell lists (NaN for the empty cell); min / max per cell against
    the 0/1 and 1/1 quantiles and the one-shot SQL min / max, the empty cell included; WHERE only: a list of one."""
    cells = fixed_cells(FIXED, qmin)
    assert [len(c) for c in cells] == [9, 1, 0]
    L = Q.iter_rounds(qmin, qmax, base)
    node.dp_data = fixed_tables(cl, FIXED, qmin, device)
    kw = dict(query_min=qmin, query_max=qmax, rows=3, group_by=(3,), sql=sql())
    try:
        sq = make_survey(client, cl, "frequencyCount", **kw)
        for num, den in QUANTILES:
            seen = []
            values, rnds = client.send_iterative_quantile(sq, base, num, den,
                                                          on_round=lambda k, d, r: seen.append((k, d)))
            _same(values, [float(tq.nearest_rank(c, num, den)) if c else float("nan") for c in cells])
            assert len(rnds) == L and [k for k, _ in seen] == list(range(L)) and all(len(d) == 3 for _, d in seen)
            assert [r.survey_id for r in rnds] == [f"{sq.SurveyID}.r{k}" for k in range(L)]
            assert all(r.n_out == base for r in rnds)
            assert [sum(c) for c in rnds[0].client_out] == [9, 1, 0]
            if (num, den) in ((0, 1), (1, 1)):
                name = "min" if num == 0 else "max"
                ext, ernds = client.send_iterative_extreme(make_survey(client, cl, name, **kw), base)
                _, shot, _ = client.send_survey_query(make_survey(client, cl, name, **kw))
                assert ext == [v[0] for v in shot] and len(ernds) == L
                assert ext == [float((min if num == 0 else max)(c)) if c else float(qmin) for c in cells]
                assert ext[:2] == values[:2]
        # WHERE only: G = 1, the answer replicated over the groups of GroupByValues
        one = make_survey(client, cl, "frequencyCount", query_min=qmin, query_max=qmax, rows=3, group_by=(2,),
                          sql=sql(()))
        values, rnds = client.send_iterative_quantile(one, base, 1, 2)
        flat = [r[0] + qmin for t in FIXED for r in t if r[2] == 1]
        assert values == [float(tq.nearest_rank(flat, 1, 2))] and len(rnds[0].client_out) == 2
        ext, _ = client.send_iterative_extreme(make_survey(client, cl, "max", query_min=qmin, query_max=qmax, rows=3,
                                                           group_by=(2,), sql=sql(())), base)
        assert ext == [float(max(flat))]
    finally:
        node.dp_data = {}


def check_search_generated(cl, node, client, qmin, qmax, base):
    """Generated tables (no dp_data): every round redraws the same table from the id the rounds share."""
    sq = make_iterative_survey(client, cl, "frequencyCount", base, query_min=qmin, query_max=qmax, rows=12,
                               group_by=(3,), sql=sql(), survey_id=f"cohort-generated-{qmin}-{qmax}-{base}")
    values, rnds = client.send_iterative_quantile(sq, base, 1, 2)
    plan = Q.sql_plan(sq.Query)
    cells = [[] for _ in range(3)]
    for dp in cl.dps:
        tables = [dcp.generate_sql_table(client.iterative_round_query(sq, base, k, [0, 0, 0], sq.SurveyID), dp.id, plan)
                  for k in range(len(rnds))]
        assert all(torch.equal(t, tables[0]) for t in tables) and tables[0].shape == (12, 3)
        for x, c1, c2 in tables[0].tolist():
            if c2 == 1:
                cells[c1].append(x)
    assert sum(map(len, cells)) > 3 and [sum(c) for c in rnds[0].client_out] == [len(c) for c in cells]
    _same(values, [float(tq.nearest_rank(c, 1, 2)) if c else float("nan") for c in cells])


def check_search_with_proofs(cl, node, client, device, base):
    """(16, 2) proofs and 3 VNs: one block per round, every code PROOF_TRUE."""
    node.dp_data = fixed_tables(cl, FIXED, 0, device)
    try:
        sq = make_iterative_survey(client, cl, "frequencyCount", base, query_min=0, query_max=99, rows=3, proofs=1,
                                   ranges=[16, 2], sig_device=device, group_by=(3,), sql=sql())
        values, rnds = client.send_iterative_quantile(sq, base, 1, 2)
    finally:
        node.dp_data = {}
    cells = fixed_cells(FIXED)
    _same(values, [float(tq.nearest_rank(c, 1, 2)) if c else float("nan") for c in cells])
    L = Q.iter_rounds(0, 99, base)
    assert len(rnds) == L and len({r.block.Hash for r in rnds}) == L
    for k, r in enumerate(rnds):
        codes = r.block.data_block().Proofs
        assert codes and set(codes.values()) == {prq.PROOF_TRUE}
        assert r.survey_id == f"{sq.SurveyID}.r{k}"
    return rnds


def test_search_fixed_tables(env):
    cl, node, client = env
    check_search_fixed(cl, node, client, "cpu", 0, 99, 10)
    check_search_fixed(cl, node, client, "cpu", -40, 59, 10)


def test_search_generated_tables(env):
    cl, node, client = env
    check_search_generated(cl, node, client, 0, 99, 10)


def test_search_with_proofs(env):
    cl, node, client = env
    check_search_with_proofs(cl, node, client, "cpu", 10)


def test_inconsistent_dp_names_the_cell(env):
    cl, node, client = env
    node.dp_data = fixed_tables(cl, FIXED)
    changed = [list(t) for t in FIXED]
    changed[1] = [(99, 0, 1), (5, 0, 1), (47, 1, 1)]  # cell 1's record moves inside its round-0 bin

    def swap(k, digits, res):
        if k == 0:
            assert digits[1] == 4 and res.client_out[1][4] == 1
            changed[1][2] = (77, 1, 1)
            node.dp_data = fixed_tables(cl, changed)

    try:
        kw = dict(query_min=0, query_max=99, rows=3, group_by=(3,), sql=sql())
        with pytest.raises(RuntimeError, match="round 1, cell 1: .*changed between rounds"):
            client.send_iterative_quantile(make_survey(client, cl, "frequencyCount", **kw), 10, 1, 2, on_round=swap)
        node.dp_data = fixed_tables(cl, FIXED)

        def fill(k, digits, res):  # the cell empty in round 0 gets a record afterwards
            if k == 0:
                node.dp_data = fixed_tables(cl, [FIXED[0] + [(3, 2, 1)]] + FIXED[1:])

        with pytest.raises(RuntimeError, match="round 1, cell 2: .*changed between rounds"):
            client.send_iterative_quantile(make_survey(client, cl, "frequencyCount", **kw), 10, 1, 2, on_round=fill)
        node.dp_data = fixed_tables(cl, FIXED)
        with pytest.raises(RuntimeError, match="round 1, cell 2: .*changed between rounds"):
            client.send_iterative_extreme(make_survey(client, cl, "min", **kw), 10, on_round=fill)
    finally:
        node.dp_data = {}


def test_one_dp_path_keeps_refusing_sql(env):
    cl, node, client = env
    sq = _round(env)
    with pytest.raises(ValueError, match="batched encoders only"):
        dcp.dp_encode(node, sq, cl.dps[0], sync_timer=False)
    batch = dcp.dp_encode_batch(node, sq, cl.dps)
    assert all(len(v["clear"]) == 3 and all(len(c) == 10 for c in v["clear"]) for v in batch.values())


# ----------------------------------------------------------------------------- two ranks
def test_two_gloo_ranks_through_the_tool(tmp_path):
    env_ = dict(os.environ, OMP_NUM_THREADS="4", DX_NUM_THREADS="4")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_iter.py"), "--query", "quantile", "--gpus",
                        "2", "--range", "1000", "--bases", "10", "--steps", "1", "--passes", "1", "--device", "cpu",
                        "--groups", "3", "--no-classic", "--out-dir", str(tmp_path)], cwd=ROOT, env=env_,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert line["result_ok"] and line["all_proofs_valid"] and line["n_gpus"] == 2 and line["groups"] == 3
    assert line["queries"]["base=10"]["rounds"] == 3 and line["runs"][0]["blocks_per_result"] == 3
    assert len(line["clear_quantile"]) == 3
