"""K-means as a verifiable multi-round query: the K14f rows against the
pure-Python model of the specification (``drynx_amd.kmeans.round_model``), the
querier's update and SSE against Fraction arithmetic, every argument and
validation rule, the wire and dict forms, runs end to end (fixed and generated
records, with proofs, stopping at convergence) and the command line.  The
checks shared with the GPU suite live here and take a device; the model rows
are computed once per case and shared."""
import copy
import functools
import json
import os
import socket
import subprocess
import time
from fractions import Fraction

import pytest
import torch

from drynx_amd import kmeans as km
from drynx_amd import native as nt
from drynx_amd import query as Q
from drynx_amd.proofs import requests as prq
from drynx_amd.services.api import DrynxClient
from drynx_amd.services.local import local_cluster, make_kmeans_survey, make_survey

SEGS = [0, 1, 63, 64, 65, 257]  # an empty DP, one row, around the 64-row step of the tile plan, several chunks
DIMS = [1, 2, 5, 32]


def clusters_of(d):
    return [1, 2, 3, 17, km.max_clusters(d)]


# ----------------------------------------------------------------------------- (a) rows against the model
@functools.lru_cache(maxsize=None)
def table_case(d, k):
    """(table [rows, d + 3], qmin, qmax, scale, centroids, model rows) of the (d, k) case: a negative QueryMin,
    rows outside the domain in one and in all coordinates, the records a strided column view of the table."""
    qmin, qmax, scale = -7, 50, 3
    gen = torch.Generator().manual_seed(1000 * d + k)
    T = torch.randint(qmin, qmax + 1, (sum(SEGS), d + 3), generator=gen, dtype=torch.int64)
    for i in range(T.shape[0]):
        if i % 11 == 3:  # one coordinate outside, alternately below and above
            T[i, 2 + i % d] = qmin - 1 if i % 2 else qmax + 1
        if i % 13 == 5:  # every coordinate outside
            T[i, 2: 2 + d] = qmax + 1 + i
    cen = km.random_centroids(k, d, qmax - qmin + 1, scale, f"case {d} {k}")
    rows, want, at = T[:, 2: 2 + d].tolist(), [], 0
    for n in SEGS:
        want.append(km.round_model(rows[at: at + n], k, d, qmin, qmax, scale, cen))
        at += n
    return T, qmin, qmax, scale, cen, want


def check_rows(device, d):
    """The (d, k) cases on ``device``: equal to the model; returns the rows (for the host twin comparison)."""
    outs = []
    for k in clusters_of(d):
        T, qmin, qmax, scale, cen, want = table_case(d, k)
        Z = T.to(device)[:, 2: 2 + d]
        assert Z.stride(0) == d + 3
        out = nt.kmeans_round(Z, SEGS, d, k, qmin, qmax, scale, cen)
        assert out.shape == (len(SEGS), k * (d + 2)) and out.dtype == torch.int64 and out.device == Z.device
        assert out.cpu().tolist() == want, (d, k)
        assert out[0].abs().sum().item() == 0  # the empty DP
        kept = sum(sum(w[c * (d + 2)] for c in range(k)) for w in want)
        assert 0 < kept < sum(SEGS)  # rows were dropped, rows were kept
        outs.append(out.cpu())
    return outs


M31 = (1 << 31) - 1


@functools.lru_cache(maxsize=None)
def edge_cases():
    """[(name, rows per DP, k, d, qmin, qmax, scale, centroids)] of the ties and the largest distances."""
    cases = [
        # two identical centroids: the lower index takes every row they win
        ("twins", [[(3, 4), (5, 5), (40, 41)], [(4, 4)]], 3, 2, 0, 50, 2, [8, 8, 8, 8, 80, 80]),
        # a row exactly midway between two centroids goes to the lower index (d = 1 and d = 2)
        ("midway-1", [[(15,), (14,), (16,)]], 2, 1, 0, 30, 1, [10, 20]),
        ("midway-1-swapped", [[(15,), (14,), (16,)]], 2, 1, 0, 30, 1, [20, 10]),
        ("midway-2", [[(2, 0), (2, 5), (1, 0), (3, 0)]], 2, 2, 0, 9, 2, [0, 0, 8, 0]),
        # (R - 1) * S = 2^31 - 1, rows at both corners: D up to 2 * (2^31 - 1)^2, just below 2^63
        ("corners", [[(-5, -5)], [(M31 - 5, M31 - 5)], [(-5, -5), (M31 - 5, M31 - 5), (M31 - 5, -5)]], 3, 2, -5,
         M31 - 5, 1, [M31, M31, 0, 0, M31, 0]),
        ("corners-far", [[(-5, -5), (M31 - 5, M31 - 5)]], 2, 2, -5, M31 - 5, 1, [M31, M31, M31, M31 - 1]),
        ("corners-one", [[(-5, -5), (M31 - 5, M31 - 5)]], 1, 2, -5, M31 - 5, 1, [M31, M31]),
        # the same with a scale: S * o reaches 2^31 - 2^10
        ("scaled", [[(0, 0), ((1 << 21) - 1, (1 << 21) - 1), (1 << 20, 5)]], 2, 2, 0, (1 << 21) - 1, 1 << 10,
         [0, 0, ((1 << 21) - 1) << 10, ((1 << 21) - 1) << 10]),
        # one value per column: every offset and centroid is 0
        ("point", [[(7,), (7,), (8,)]], 2, 1, 7, 7, 5, [0, 0]),
    ]
    out = []
    for name, dps, k, d, qmin, qmax, scale, cen in cases:
        want = [km.round_model(rows, k, d, qmin, qmax, scale, cen) for rows in dps]
        out.append((name, dps, k, d, qmin, qmax, scale, cen, want))
    return out


def check_edges(device):
    outs = {}
    for name, dps, k, d, qmin, qmax, scale, cen, want in edge_cases():
        Z = torch.tensor([r for rows in dps for r in rows], dtype=torch.int64).reshape(-1, d).to(device)
        out = nt.kmeans_round(Z, [len(rows) for rows in dps], d, k, qmin, qmax, scale, cen).cpu()
        assert out.tolist() == want, name
        outs[name] = out
    # what the specification says of them, not only the model
    assert outs["twins"].tolist() == [[2, 8, 9, 75, 0, 0, 0, 0, 1, 40, 41, 3281], [1, 4, 4, 32, 0, 0, 0, 0, 0, 0, 0, 0]]
    assert outs["midway-1"].tolist() == [[2, 29, 421, 1, 16, 256]]
    assert outs["midway-1-swapped"].tolist() == [[2, 31, 481, 1, 14, 196]]
    assert outs["midway-2"].tolist() == [[3, 5, 5, 34, 1, 3, 0, 9]]
    assert outs["corners"].tolist()[2] == [1, M31, M31, 2 * M31 * M31, 1, 0, 0, 0, 1, M31, 0, M31 * M31]
    assert outs["corners-far"].tolist() == [[1, M31, M31, 2 * M31 * M31, 1, 0, 0, 0]]
    assert outs["point"].tolist() == [[2, 0, 0, 0, 0, 0]]
    return outs


@pytest.mark.parametrize("d", DIMS)
def test_rows_equal_the_model(d):
    check_rows("cpu", d)


def test_ties_and_largest_distances():
    check_edges("cpu")


@functools.lru_cache(maxsize=None)
def large_case(one_cluster: bool):
    """One DP of 70000 rows at k = 17, d = 5 (many tiles and a ragged one): uniform records, or centroids that
    send every row to cluster 11 (all atomics on one cluster's cells)."""
    k, d, qmin, qmax, scale, n = 17, 5, 0, 200, 2, 70000
    gen = torch.Generator().manual_seed(7 + one_cluster)
    if one_cluster:
        Z = torch.randint(150, qmax + 1, (n, d), generator=gen, dtype=torch.int64)
        cen = [0] * (k * d)
        cen[11 * d: 12 * d] = [350] * d
    else:
        Z = torch.randint(qmin, qmax + 1, (n, d), generator=gen, dtype=torch.int64)
        cen = km.random_centroids(k, d, qmax - qmin + 1, scale, "large")
    return Z, k, d, qmin, qmax, scale, cen, km.round_model(Z.tolist(), k, d, qmin, qmax, scale, cen)


def check_large(device):
    outs = []
    for one in (False, True):
        Z, k, d, qmin, qmax, scale, cen, want = large_case(one)
        out = nt.kmeans_round(Z.to(device), [Z.shape[0]], d, k, qmin, qmax, scale, cen).cpu()
        assert out.tolist() == [want]
        if one:
            assert want[11 * (d + 2)] == Z.shape[0] and sum(want[c * (d + 2)] for c in range(k)) == Z.shape[0]
        outs.append(out)
    return outs


def test_one_large_dp_host():
    check_large("cpu")


# ----------------------------------------------------------------------------- (b) the querier's arithmetic
def test_update_and_sse():
    k, d, S = 3, 2, 4
    cen = [5, 6, 40, 44, 100, 101]
    # cluster 0: n = 2, sums (3, 7): S * 3 / 2 = 6 exactly, S * 7 / 2 = 14; cluster 1 empty; cluster 2: n = 8
    answer = [2, 3, 7, 29, 0, 0, 0, 0, 8, 61, 13, 1000]
    new = km.update(cen, answer, k, d, S)
    assert new == [6, 14, 40, 44, 31, 7]  # 4 * 61 / 8 = 30.5 -> 31 (half up), 4 * 13 / 8 = 6.5 -> 7
    for c, n in enumerate([2, 0, 8]):
        for j in range(d):
            if n:
                mean = Fraction(S * answer[c * 4 + 1 + j], n)
                assert new[c * d + j] == (mean + Fraction(1, 2)).__floor__()
            else:
                assert new[c * d + j] == cen[c * d + j]
    # half-way at scale 1: mean 1.5 -> 2, mean 2.5 -> 3 (up, not to even)
    assert km.update([0], [2, 3, 5], 1, 1, 1) == [2] and km.update([0], [2, 5, 13], 1, 1, 1) == [3]
    assert km.update([9], [0, 0, 0], 1, 1, 1) == [9]
    want = (29 - Fraction(3 * 3 + 7 * 7, 2)) + (1000 - Fraction(61 * 61 + 13 * 13, 8))
    assert km.sse(answer, k, d) == want and isinstance(km.sse(answer, k, d), Fraction)
    assert km.sse([0, 0, 0], 1, 1) == 0
    assert km.split(answer, k, d) == ([2, 0, 8], [[3, 7], [0, 0], [61, 13]], [29, 0, 1000])
    assert km.points([6, 14, 40, 44, 31, 7], 3, 2, -10, 4)[2] == [Fraction(-10) + Fraction(31, 4), Fraction(-33, 4)]
    with pytest.raises(ValueError, match="an answer of 11 values"):
        km.update(cen, answer[:-1], k, d, S)
    a, b = km.random_centroids(4, 2, 100, 3, "s"), km.random_centroids(4, 2, 100, 3, "s")
    assert a == b and len(a) == 8 and all(0 <= c <= 99 * 3 for c in a) and a != km.random_centroids(4, 2, 100, 3, "t")


# ----------------------------------------------------------------------------- (c) every rule
def test_check_rules():
    km.check(512, 4, 0, 9, 1, [0] * 2048)
    km.check(90, 32, -5, 5, 3, None)
    km.check(1, 2, -5, M31 - 5, 1, [M31, 0])
    bad = [
        ((1, 0, 0, 9, 1), "0 columns outside 1..32"), ((1, 33, 0, 9, 1), "33 columns outside 1..32"),
        ((0, 1, 0, 9, 1), "0 clusters outside 1..512"), ((513, 1, 0, 9, 1), "513 clusters outside 1..512"),
        ((439, 5, 0, 9, 1), "3073 outputs"), ((91, 32, 0, 9, 1), "3094 outputs"),
        ((1, 1, 0, 9, 0), "scale 0 below 1"), ((1, 1, 5, 4, 1), "an empty domain"),
        ((1, 1, 0, 1 << 31, 1), "does not stay below 2\\^31"), ((1, 1, 0, 1 << 30, 2), "does not stay below 2\\^31"),
        ((1, 3, 0, M31, 1), "does not stay below 2\\^63"), ((1, 32, 0, 1 << 29, 1), "does not stay below 2\\^63"),
        ((1, 1, 0, 1 << 64, 1), "int64"), ((1, 1, -(1 << 63) - 1, -(1 << 63), 1), "int64"),
        ((1.0, 1, 0, 9, 1), "are integers"), ((1, 1, 0, 9, True), "are integers"),
    ]
    for args, msg in bad:
        with pytest.raises(ValueError, match=msg):
            km.check(*args)
    for cen, msg in (([0], "1 centroid coordinates for 2 clusters of 1 columns"), ([0, 28], "outside 0.."),
                     ([-1, 0], "outside 0.."), ([0, 1.0], "outside 0.."), ("ab", "no list of")):
        with pytest.raises(ValueError, match=msg):
            km.check(2, 1, 0, 9, 3, cen)
    for r, rnd in ((0, 0), (65, 0), (3, 3), (3, -1), ("3", 0)):
        with pytest.raises(ValueError, match="rounds outside|round .* outside"):
            km.check_rounds(r, rnd)
    km.check_rounds(64, 63)
    assert km.max_clusters(1) == 512 and km.max_clusters(5) == 438 and km.max_clusters(32) == 90
    with pytest.raises(ValueError):
        Q.kmeans_operation(0, 9, 32, 91)
    assert Q.kmeans_operation(-3, 9, 5, 17) == Q.Operation("kmeans", 5, 119, -3, 9)
    with pytest.raises(ValueError, match="does not exist"):
        Q.choose_operation("kmeans", 0, 9, 2, 0)  # stays as it is


def test_binding_and_entry_refuse():
    import ctypes

    Z = torch.zeros((4, 2), dtype=torch.int64)
    ok = dict(Z=Z, seg_rows=[4], d=2, k=2, qmin=0, qmax=9, scale=1, centroids=[0, 0, 9, 9])
    assert nt.kmeans_round(**ok).tolist() == [[4, 0, 0, 0, 0, 0, 0, 0]]
    for kw, msg in ((dict(seg_rows=[3]), "segments cover 3 rows"), (dict(seg_rows=[5, -1]), "segments cover"),
                    (dict(d=3, centroids=[0] * 6), "Z has 2 columns"), (dict(centroids=[0, 0, 9, 10]), "outside 0.."),
                    (dict(centroids=[0, 0, 9]), "3 centroid coordinates"), (dict(k=513), "513 clusters"),
                    (dict(scale=0), "scale 0"), (dict(qmax=1 << 31), "2\\^31")):
        with pytest.raises(ValueError, match=msg):
            nt.kmeans_round(**dict(ok, **kw))
    assert nt.kmeans_round(Z[:0], [0, 0], 2, 2, 0, 9, 1, [0, 0, 9, 9]).tolist() == [[0] * 8] * 2
    assert nt.kmeans_round(Z[:0], [], 2, 2, 0, 9, 1, [0, 0, 9, 9]).shape == (0, 8)
    # below the binding: the entry returns -2, it never asserts, and writes nothing
    assert nt.lib().dx_kmeans_max_cells() == km.KMEANS_MAX_CELLS
    tiles = torch.tensor([0, 0, 4], dtype=torch.int64)
    cen = torch.tensor([0, 0, 9, 9], dtype=torch.int64)
    out = torch.zeros(8, dtype=torch.int64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def rc(k=2, d=2, scale=1, qmin=0, qmax=9, n_tiles=1, n_dp=1, ldz=2):
        return nt.lib().dx_kmeans_round(0, None, p(Z), ldz, p(tiles), n_tiles, n_dp, p(cen), k, d, scale, qmin, qmax,
                                        p(out))

    assert rc() == 0 and out.tolist() == [4, 0, 0, 0, 0, 0, 0, 0]
    out.zero_()
    for kw in (dict(k=0), dict(k=513), dict(d=0), dict(d=33), dict(k=439, d=5), dict(scale=0), dict(qmin=1, qmax=0),
               dict(qmax=1 << 31), dict(qmax=1 << 30, scale=2), dict(d=3, qmax=M31), dict(scale=1 << 31),
               dict(qmin=-(1 << 63), qmax=(1 << 63) - 1), dict(n_tiles=-1), dict(n_dp=0), dict(ldz=-1),
               dict(qmax=8)):  # (the host path reads the centroids: 9 > (R - 1) * S = 8)
        assert rc(**kw) == -2, kw
    tiles[0] = 1
    assert rc() == -2  # a tile of a DP the output has no row for
    tiles[0], tiles[1], tiles[2] = 0, 3, 2
    assert rc() == -2  # rows out of order
    assert out.tolist() == [0] * 8 and rc(n_tiles=0) == 0


# ----------------------------------------------------------------------------- validation, wire and dict
@pytest.fixture(scope="module")
def env(tmp_path_factory):
    cl, node = local_cluster(3, 5, 3, device="cpu", workdir=str(tmp_path_factory.mktemp("db")))
    yield cl, node, DrynxClient(node)
    node.close(remove=True)


def _round(env, k=3, d=2, scale=4, rounds=5, r=0, qmin=0, qmax=99, cen=None, proofs=0, ranges=None):
    cl, node, client = env
    sq = make_kmeans_survey(client, cl, k, d, scale, rounds, query_min=qmin, query_max=qmax, rows=4, proofs=proofs,
                            ranges=ranges)
    cen = km.random_centroids(k, d, qmax - qmin + 1, scale, "v") if cen is None else cen
    return client.kmeans_round_query(sq, r, cen, "km")


def test_check_parameters_rules(env):
    ok = _round(env)
    op = ok.Query.Operation
    assert Q.check_parameters(ok, False) and Q._check_kmeans(ok) == []
    assert (op.NameOp, op.NbrInput, op.NbrOutput, ok.SurveyID) == ("kmeans", 2, 12, "km.r0")
    assert (op.KMeans.K, op.KMeans.Scale, op.KMeans.Round, op.KMeans.Rounds, op.KMeans.SearchID) == (3, 4, 0, 5, "km")
    assert Q.check_parameters(_round(env, r=4, qmin=-50, qmax=49), False)
    pr = _round(env, proofs=1, ranges=[16, 2])
    assert Q.check_parameters(pr, False)
    assert pr.Query.Ranges == [[16, 2]] * 12 and all(len(r) == 12 for r in pr.Query.IVSigs.InputValidationSigs)

    def refusal(sq0=ok, **kw):
        sq = copy.deepcopy(sq0)
        for key, v in kw.items():
            obj, _, attr = key.rpartition("__")
            tgt = sq
            for part in filter(None, obj.split("__")):
                tgt = getattr(tgt, part)
            setattr(tgt, attr, v)
        msgs = Q._check_kmeans(sq)
        assert bool(msgs) == (not Q.check_parameters(sq, Q.add_diff_p(sq.Query.DiffP)))
        return " | ".join(msgs)

    P = "Query__Operation__KMeans__"
    assert refusal() == ""
    assert "0 clusters outside" in refusal(**{P + "K": 0})
    assert "centroid coordinates for 4 clusters" in refusal(**{P + "K": 4})
    assert "scale 0 below 1" in refusal(**{P + "Scale": 0})
    assert "a centroid coordinate outside" in refusal(**{P + "Scale": 1, P + "Centroids": [0] * 5 + [100]})
    assert "5 centroid coordinates" in refusal(**{P + "Centroids": [0] * 5})
    assert "a centroid coordinate outside" in refusal(**{P + "Centroids": [0] * 5 + [-1]})
    assert "a centroid coordinate outside" in refusal(**{P + "Centroids": [0] * 5 + [99 * 4 + 1]})
    assert refusal(**{P + "Centroids": [0] * 5 + [99 * 4]}) == ""
    assert "not a list" in refusal(**{P + "Centroids": None})
    assert "round 5 outside 0..4" in refusal(**{P + "Round": 5}) and "round -1" in refusal(**{P + "Round": -1})
    assert "65 rounds outside" in refusal(**{P + "Rounds": 65}) and "0 rounds outside" in refusal(**{P + "Rounds": 0})
    assert "33 columns" in refusal(Query__Operation__NbrInput=33)
    assert "2^31" in refusal(Query__Operation__QueryMax=1 << 31, Query__DPDataGen__GenerateDataMax=1 << 31)
    assert "2^63" in refusal(Query__Operation__QueryMax=M31, Query__DPDataGen__GenerateDataMax=M31,
                             Query__Operation__NbrInput=3, **{P + "Scale": 1})
    assert "exactly K * (d + 2) = 12 outputs" in refusal(Query__Operation__NbrOutput=11)
    assert "without its parameters" in refusal(Query__Operation__KMeans=None)
    assert "cutting factor" in refusal(Query__CuttingFactor=2)
    assert "differential privacy" in refusal(Query__DiffP=Q.QueryDiffP(LapMean=0.0, LapScale=1.0, NoiseListSize=8,
                                                                       Quanta=1.0, Scale=1.0, Limit=3))
    assert "obfuscation" in refusal(Query__Obfuscation=True)
    assert "iterative digits" in refusal(IterBase=12)
    # with proofs: one range per output, none of them (0, 0)
    assert "one range per output (12)" in refusal(pr, Query__Ranges=[[16, 2]] * 11)
    assert "(0, 0) range" in refusal(pr, Query__Ranges=[[16, 2]] * 11 + [[0, 0]])
    assert refusal(pr, Query__Ranges=[[16, 2]] * 11 + [[4, 4]]) == ""
    # the block belongs to the operation kmeans alone; SQL refuses the name
    mean = make_survey(env[2], env[0], "mean", query_min=0, query_max=9, rows=3)
    assert Q.check_parameters(mean, False)
    assert "k-means parameters with the operation mean" in refusal(mean, Query__Operation__KMeans=op.KMeans)
    sql = copy.deepcopy(ok)
    sql.Query.SQL = Q.QuerySQL(Where=[Q.WhereClear("c2", "1")])
    assert not Q.check_parameters(sql, False) and "SQL with the operation kmeans" in Q._check_sql(sql)
    with pytest.raises(ValueError, match="needs the ranges"):
        make_kmeans_survey(env[2], env[0], 2, 1, 1, 2, proofs=1)
    with pytest.raises(ValueError, match="needs a kmeans survey"):
        env[2].kmeans_round_query(mean, 0, [0], "x")


def test_wire_and_dict(env):
    from drynx_amd.wire import messages as M
    from drynx_amd.wire import onet
    from drynx_amd.wire import protobuf as pb

    cen = [0, 1, 396, 5, 17, 200]
    sq = _round(env, r=3, cen=cen)
    assert onet.OPERATION[-1] == ("KMeans", ("msg", onet.KMEANS_PARAMETERS))
    want = Q.KMeansParameters(K=3, Scale=4, Round=3, Rounds=5, Centroids=cen, SearchID="km")
    for back in (M.survey_query_from_wire(M.survey_query_to_wire(sq)), Q.SurveyQuery.from_dict(sq.to_dict()),
                 Q.SurveyQuery.from_dict(json.loads(json.dumps(sq.to_dict())))):
        assert back.Query.Operation.KMeans == want and back.Query.Operation == sq.Query.Operation
        assert Q.check_parameters(back, False)
    assert sq.to_dict()["Query"]["Operation"]["KMeans"]["Centroids"] == cen
    wire = M.survey_query_to_wire(sq)
    assert M.survey_query_to_wire(M.survey_query_from_wire(wire)) == wire
    # every other survey: the dict and the bytes of the schema without the field
    old_op = tuple(f for f in onet.OPERATION if f[0] != "KMeans")
    old_query = tuple((n, ("msg", old_op)) if n == "Operation" else (n, k) for n, k in onet.QUERY)
    old = tuple((n, ("msg", old_query)) if n == "Query" else (n, k) for n, k in onet.SURVEY_QUERY_ITER)
    assert old_op == onet.OPERATION[:-1] and len(old_op) == 6
    from drynx_amd.services.local import make_iterative_survey

    plain = make_survey(env[2], env[0], "variance", query_min=0, query_max=7, rows=3, group_by=(2,))
    it = env[2].iterative_round_query(make_iterative_survey(env[2], env[0], "max", 10, query_min=0, query_max=99,
                                                            rows=4), 10, 1, 7, "it")
    for s in (plain, it):
        assert s.Query.Operation.KMeans is None and "KMeans" not in s.to_dict()["Query"]["Operation"]
        msg = M.survey_query_to_msg(s)
        assert msg["Query"]["Operation"]["KMeans"] is None
        assert M.survey_query_to_wire(s) == onet.message_type_id("libdrynx.SurveyQuery") + pb.encode(old, msg)
        assert M.survey_query_from_wire(M.survey_query_to_wire(s)).Query.Operation.KMeans is None
        assert Q.SurveyQuery.from_dict(s.to_dict()).Query.Operation.KMeans is None
    # the block itself travels: the schema without the field drops its bytes
    assert len(wire) > len(onet.message_type_id("libdrynx.SurveyQuery") + pb.encode(old, M.survey_query_to_msg(sq)))


# ----------------------------------------------------------------------------- (e) runs end to end
# (x, y) per DP: three well-separated blobs, an empty DP, rows outside the domain [0, 99] in one and in both columns
BLOBS = [[(10, 12), (12, 9), (80, 20), (150, 10)],
         [(83, 22), (79, 18), (40, 85), (-1, -1)],
         [],
         [(42, 88), (38, 84), (11, 11), (8, 13), (41, 100)],
         [(82, 19), (39, 86), (44, 83)]]
START = [(0, 0), (50, 20), (60, 40), (99, 99)]  # round 0 splits a blob; the fourth never wins a row and stays
KM = dict(k=4, d=2, scale=4, rounds=5, qmin=0, qmax=99)


def blob_data(cl, device="cpu", lo=0):
    return {dp.id: [torch.tensor([r[c] + lo for r in BLOBS[i]], dtype=torch.int64).to(device) for c in range(2)]
            for i, dp in enumerate(cl.dps)}


def model_run(rows, k, d, scale, rounds, qmin, qmax, start, stop=False):
    """The run on the pooled rows: (final centroids, assigned, last answer, converged_at, rounds run)."""
    cur, conv, answer, assigned, n = list(start), None, None, None, 0
    for r in range(rounds):
        answer, assigned = km.round_model(rows, k, d, qmin, qmax, scale, cur), cur
        cur = km.update(assigned, answer, k, d, scale)
        n += 1
        if cur == assigned and conv is None:
            conv = r
        if stop and conv is not None:
            break
    return cur, assigned, answer, conv, n


def check_run_fixed(cl, node, client, device, lo=0):
    k, d, S, rounds = KM["k"], KM["d"], KM["scale"], KM["rounds"]
    qmin, qmax = KM["qmin"] + lo, KM["qmax"] + lo
    start = [c * S for pt in START for c in pt]
    pooled = [(x + lo, y + lo) for rows in BLOBS for x, y in rows]
    cur, assigned, answer, conv, _ = model_run(pooled, k, d, S, rounds, qmin, qmax, start)
    assert conv == 2  # the third round's update changes nothing
    node.dp_data = blob_data(cl, device, lo)
    try:
        sq = make_kmeans_survey(client, cl, k, d, S, rounds, query_min=qmin, query_max=qmax, rows=3)
        seen = []
        res = client.send_kmeans(sq, start, on_round=lambda r, a, s: seen.append((r, list(a))))
        short = client.send_kmeans(sq, start, stop_when_converged=True)
    finally:
        node.dp_data = {}
    counts, sums, sqs = km.split(answer, k, d)
    assert (res.centroids, res.assigned, res.counts, res.sums, res.sq_sums) == (cur, assigned, counts, sums, sqs)
    assert res.converged_at == conv and res.sse == km.sse(answer, k, d) and isinstance(res.sse, Fraction)
    assert res.points == [[qmin + Fraction(cur[c * d + j], S) for j in range(d)] for c in range(k)]
    assert counts == [4, 4, 5, 0] and sum(counts) == len(pooled) - 3  # three rows lie outside the domain
    assert res.centroids[3 * d:] == start[3 * d:] and res.points[3] == [qmin + 99, qmin + 99]
    # the blobs' exact means, rounded half up to quarters
    assert res.points[0] == [qmin + Fraction(41, 4), qmin + Fraction(45, 4)]
    assert len(res.rounds) == rounds and [r for r, _ in seen] == list(range(rounds)) and seen[-1][1] == answer
    assert [r.survey_id for r in res.rounds] == [f"{sq.SurveyID}.r{r}" for r in range(rounds)]
    assert all(r.n_out == k * (d + 2) and r.block is None for r in res.rounds)
    assert len(short.rounds) == conv + 1 and short.converged_at == conv
    assert (short.centroids, short.counts, short.sse) == (res.centroids, res.counts, res.sse)
    return res


def check_run_generated(cl, node, client, device="cpu"):
    """Generated records (no dp_data): every round must draw the same ones, from the id the rounds share."""
    from drynx_amd.protocols.data_collection import _seed

    k, d, S, rounds, qmin, qmax, n = 3, 2, 2, 4, -20, 43, 6
    sq = make_kmeans_survey(client, cl, k, d, S, rounds, query_min=qmin, query_max=qmax, rows=n)
    start = km.random_centroids(k, d, qmax - qmin + 1, S, "generated")
    seen = []
    res = client.send_kmeans(sq, start, on_round=lambda r, a, s: seen.append(list(a)))
    recs = []
    for dp in cl.dps:  # redrawn here from the shared id as the DPs draw them
        gen = torch.Generator().manual_seed(_seed(sq.SurveyID, dp.id))
        recs += torch.randint(qmin, qmax + 1, (d, n), generator=gen, dtype=torch.int64).t().tolist()
    cur, assigned, answer, conv, _ = model_run(recs, k, d, S, rounds, qmin, qmax, start)
    assert (res.centroids, res.assigned, res.converged_at) == (cur, assigned, conv)
    assert seen[-1] == answer and all(sum(a[c * (d + 2)] for c in range(k)) == len(recs) for a in seen)
    return res


def check_run_with_proofs(cl, node, client, device):
    """(16, 2) proofs and 3 VNs at k = 2, d = 1, two rounds: one block per round, every code PROOF_TRUE."""
    lists = [[1, 2], [8, 9], [], [0, 1, 9], [7]]  # every DP's sum of squares stays below 16^2
    node.dp_data = {dp.id: [torch.tensor(lists[i], dtype=torch.int64).to(device)] for i, dp in enumerate(cl.dps)}
    try:
        sq = make_kmeans_survey(client, cl, 2, 1, 2, 2, query_min=0, query_max=9, rows=3, proofs=1, ranges=[16, 2],
                                sig_device=device)
        res = client.send_kmeans(sq, [2, 12])
    finally:
        node.dp_data = {}
    cur, assigned, answer, conv, _ = model_run([(x,) for r in lists for x in r], 2, 1, 2, 2, 0, 9, [2, 12])
    assert (res.centroids, res.assigned, res.converged_at) == (cur, assigned, conv)
    assert (res.counts, res.sums, res.sq_sums) == km.split(answer, 2, 1) and res.counts == [4, 4]
    rounds = res.rounds
    assert len(rounds) == 2 and len({r.block.Hash for r in rounds}) == 2
    for r, rd in enumerate(rounds):
        codes = rd.block.data_block().Proofs
        assert set(codes.values()) == {prq.PROOF_TRUE} and len(codes) == 3 * (5 + 3 + 3)
        assert rd.survey_id == f"{sq.SurveyID}.r{r}"
        proofs = client.send_get_proofs("vn0", rd.survey_id)
        assert len(proofs) == 5 + 3 + 3 and all(p.startswith(rd.survey_id + "/") for p in proofs)
    assert rounds[1].block.BackLink == rounds[0].block.Hash
    return rounds


def test_run_fixed_records(env):
    cl, node, client = env
    check_run_fixed(cl, node, client, "cpu")
    check_run_fixed(cl, node, client, "cpu", lo=-60)


def test_run_generated_records(env):
    cl, node, client = env
    check_run_generated(cl, node, client)


def test_run_with_proofs(env):
    cl, node, client = env
    check_run_with_proofs(cl, node, client, "cpu")


def test_groups_must_agree_and_per_dp_encoder(env):
    from drynx_amd.crypto import elgamal as eg
    from drynx_amd.ops import encoding as enc

    cl, node, client = env
    node.dp_data = blob_data(cl)
    try:
        sq = make_kmeans_survey(client, cl, 4, 2, 4, 2, query_min=0, query_max=99, rows=3, group_by=(2,))
        start = [c * 4 for pt in START for c in pt]
        res = client.send_kmeans(sq, start)  # two replicated groups agree
        assert res.rounds[0].n_groups == 2 and res.counts == [4, 4, 5, 0]

        class Tampered:  # an entry whose second group differs
            def run_survey(self, rq, on_result=None):
                out = node.run_survey(rq, on_result=on_result)
                out.client_out = [out.client_out[0], [v + 1 for v in out.client_out[1]]]
                return out

        with pytest.raises(RuntimeError, match="round 0: the groups disagree"):
            DrynxClient(Tampered(), keypair=client.keypair).send_kmeans(sq, start)
    finally:
        node.dp_data = {}
    # the per-DP path: encode() of one DP's columns
    rq = client.kmeans_round_query(sq, 0, start, "one")
    pk = eg.pk_table(rq.RosterServers.aggregate(), "cpu")
    cols = [torch.tensor([r[c] for r in BLOBS[0]], dtype=torch.int64) for c in range(2)]
    r = enc.encode(cols, pk, rq.Query.Operation)
    assert r.clear == km.round_model(BLOBS[0], 4, 2, 0, 99, 4, start) and len(r.cv) == 16 and r.proofs is None


def test_stop_when_converged_needs_one_rank(env):
    cl, node, client = env

    class Ranks:
        comm = type("C", (), {"world": 2})()

    sq = make_kmeans_survey(client, cl, 2, 1, 1, 3, query_min=0, query_max=9, rows=3)
    with pytest.raises(ValueError, match="stop_when_converged with several ranks"):
        DrynxClient(Ranks()).send_kmeans(sq, [0, 9], stop_when_converged=True)


# ----------------------------------------------------------------------------- (f) the command line
FILES = {1: [(10, 12, 7), (14, 8, 7), (200, 210, 7), (300, 5, 7)],
         2: [(205, 215, 7), (12, 10, 7), (198, 220, 7)]}  # (c0, c1, an unread column); 300 is outside [0, 256]


def test_cli_centroids_argument():
    from drynx_amd.cli.client import kmeans_centroids

    assert kmeans_centroids("10,20; 200.5,40", 2, 2, 0, 2) == [20, 40, 401, 80]
    assert kmeans_centroids("-3;1/2", 2, 1, -5, 4) == [8, 22]
    for text, k, d, msg in (("1,2", 2, 2, "expected 2 points of 2"), ("1,2;3", 2, 2, "expected 2 points of 2"),
                            ("1,x", 1, 2, "x is not a number"), ("1,0.25", 1, 2, "not a multiple of 1/2")):
        with pytest.raises(SystemExit, match=msg):
            kmeans_centroids(text, k, d, 0, 2)


def test_cli_kmeans_over_record_files(tmp_path):
    from test_cli import PY, ROOT, _port, _run

    addrs = [f"127.0.0.1:{_port()}" for _ in range(3)]
    procs = []
    try:
        cfgs = []
        for i, a in enumerate(addrs):
            cfg = _run(["drynx_amd.cli.server", "new", a])
            if i == 0:
                cfg = _run(["drynx_amd.cli.server", "computing-node", "new"], cfg)
            else:
                f = tmp_path / f"dp{i}.csv"
                f.write_text("".join(",".join(str(v) for v in r) + "\n" for r in FILES[i]))
                cfg = _run(["drynx_amd.cli.server", "data-provider", "new", "file-loader", str(f)], cfg)
            cfgs.append(cfg)
        pubs = [[ln.split('"')[1] for ln in cfg.splitlines() if ln.startswith("Public")][0] for cfg in cfgs]
        group = _run(["drynx_amd.cli.client", "network", "new"])
        for a, pub in zip(addrs, pubs):
            group = _run(["drynx_amd.cli.client", "network", "add-node", a, pub], group)
        (tmp_path / "group.toml").write_text(group)
        for i, cfg in enumerate(cfgs):
            p = subprocess.Popen(PY + ["drynx_amd.cli.server", "run", "--workdir", str(tmp_path / f"n{i}"),
                                       "--device", "cpu", "--group", str(tmp_path / "group.toml")],
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                 stderr=subprocess.PIPE, text=True, cwd=ROOT,
                                 env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
            p.stdin.write(cfg)
            p.stdin.close()
            procs.append(p)
        for a in addrs:
            host, port = a.split(":")
            for _ in range(300):
                try:
                    socket.create_connection((host, int(port)), timeout=1).close()
                    break
                except OSError:
                    time.sleep(0.2)
        net = _run(["drynx_amd.cli.client", "network", "set-client", addrs[0]], group)
        sv = _run(["drynx_amd.cli.client", "survey", "new", "km-survey"], net)
        sv = _run(["drynx_amd.cli.client", "survey", "set-operation", "kmeans"], sv)
        pooled = [r[:2] for rs in FILES.values() for r in rs]

        def lines_of(start, scale, rounds):
            cur, _, answer, _, _ = model_run(pooled, 2, 2, scale, rounds, 0, 256, start)
            counts = km.split(answer, 2, 2)[0]
            pts = km.points(cur, 2, 2, 0, scale)
            return [f"{c}: {counts[c]}: " + " ".join(str(float(x)) for x in pts[c]) for c in range(2)]

        out = _run(["drynx_amd.cli.client", "survey", "run", "--clusters", "2", "--dims", "2", "--rounds", "2",
                    "--scale", "2", "--centroids", "0,0;256,255.5"], sv)
        assert out.strip().splitlines() == lines_of([0, 0, 512, 511], 2, 2)
        assert out.strip().splitlines() == ["0: 3: 12.0 10.0", "1: 3: 201.0 215.0"]
        # the default start: drawn from the survey name
        out = _run(["drynx_amd.cli.client", "survey", "run", "--clusters", "2", "--dims", "2", "--rounds", "2"], sv)
        assert out.strip().splitlines() == lines_of(km.random_centroids(2, 2, 257, 1, "km-survey"), 1, 2)
        # malformed arguments never reach the servers
        shape = ["--clusters", "2", "--dims", "2", "--rounds", "2"]
        for args, msg in ((shape[:4], "needs --clusters K --dims D --rounds N"),
                          (shape + ["--centroids", "1,2;3,0.5"], "not a multiple of 1/1"),
                          (shape + ["--where", "c2=1"], "SQL cohorts")):
            r = subprocess.run(PY + ["drynx_amd.cli.client", "survey", "run"] + args, input=sv, capture_output=True,
                               text=True, cwd=ROOT, timeout=300,
                               env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
            assert r.returncode != 0 and msg in r.stderr, (args, r.stderr[-500:])
    finally:
        from drynx_amd.services.server import RemoteNode

        RemoteNode(addrs[0]).shutdown()
        for p in procs:
            try:
                p.wait(timeout=30)
            except subprocess.TimeoutExpired:
                p.kill()
