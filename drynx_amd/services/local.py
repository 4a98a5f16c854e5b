"""Cluster bootstrap helpers shared by tests, the simulation, bench.py and the CLI.

Mirrors the reference's test/simulation wiring: ``generateNodes`` /
``repartitionDPs`` (services/service_test.go:29-66), signature creation per CN
and output (simul/drynx_simul.go:283-305), thresholds ordering
``[general, aggregation, range, obfuscation, keyswitch]``.
"""
from __future__ import annotations

import tempfile

import torch

from ..crypto import oracle as O
from ..parallel.comm import Comm, LocalComm
from ..parallel.topology import build_cluster
from ..proofs import range_proof as rp
from ..query import QueryDiffP, QueryDPDataGen, choose_operation, lr_nbr_outputs
from .api import DrynxClient
from .service import DrynxNode

RANGE_PRESETS = {  # simul/drynx_simul.go:133-281 `Ranges` codes -> (u, l)
    -1: None, 0: (0, 0), 1: (2, 1), 16: (16, 16), 17: (8, 3), 18: (16, 5), 19: (4, 16),
}


def local_cluster(n_cns=3, n_dps=5, n_vns=3, comm: Comm | None = None, device=None, workdir=None,
                  deterministic_keys=False, dp_data=None, offsets=None):
    comm = comm or LocalComm(device or ("cuda" if torch.cuda.is_available() else "cpu"))
    cl = build_cluster(n_cns, n_dps, n_vns, comm.world, comm.rank, comm, deterministic_keys, offsets)
    node = DrynxNode(cl, comm, workdir or tempfile.mkdtemp(prefix="drynx_db_"), device or comm.device, dp_data)
    return cl, node


def make_signatures(cluster, ranges, device="cpu", deterministic=False):
    """InputValidationSigs[cn][col]: one BB key + u signatures per (CN, output)."""
    if not deterministic:  # the reference default: fresh random keys per CN and per column
        flat = rp.init_range_proof_signatures([int(r[0]) for _ in cluster.cns for r in ranges], device)
        n = len(ranges)
        return [flat[i * n:(i + 1) * n] for i in range(len(cluster.cns))]
    out = []
    det: dict = {}
    for _ in cluster.cns:
        row = []
        for r in ranges:
            u = int(r[0])
            # InitRangeProofSignatureDeterministic: identical keys (x = 12), computed once per u
            if u not in det:
                det[u] = rp.init_range_proof_signature_deterministic(u, device)
            row.append(det[u])
        out.append(row)
    return out


def make_survey(client: DrynxClient, cluster, op_name: str, *, query_min=0, query_max=10, d=1, rows=10,
                group_by=(1,), proofs=0, ranges=None, obfuscation=False, thresholds=None, diffp=None,
                cutting_factor=0, lr_params=None, survey_id=None, sig_device="cpu", deterministic_sigs=False,
                verification_sharding=0, with_vns=None, range_proof_mode=0, sql=None):
    """``sql``: a ``QuerySQL`` (WHERE / GROUP BY over the DPs' records; ``group_by`` then gives the cardinalities
    of its GroupBy columns), None for a query without."""
    op = choose_operation(op_name, query_min, query_max, d, cutting_factor)
    if op_name == "logistic regression":
        op.LRParameters = lr_params
        op.NbrOutput = lr_nbr_outputs(lr_params.NbrFeatures, lr_params.K, lr_params.Packing, lr_params.NbrTargets)
    n_out = op.NbrOutput
    if ranges is not None and (len(ranges) == 0 or not isinstance(ranges[0], (list, tuple))):
        ranges = [list(ranges) for _ in range(n_out)]  # one (u, l[, offset]) for every output
    ps = None
    if proofs and ranges is not None and not all(r[0] == 0 and r[1] == 0 for r in ranges):
        ps = make_signatures(cluster, ranges, sig_device, deterministic_sigs)
    if thresholds is None:
        thresholds = [1.0, 1.0, 1.0, 1.0 if obfuscation else 0.0, 1.0] if proofs else [0.0] * 5
    with_vns = bool(proofs) if with_vns is None else with_vns
    id_to_public = {p.id: p.public for p in cluster.parties}
    gen = QueryDPDataGen(GroupByValues=list(group_by), GenerateRows=rows, GenerateDataMin=query_min,
                         GenerateDataMax=query_max)
    sq = client.generate_survey_query(
        cluster.roster_cns(), cluster.roster_vns() if with_vns else None, cluster.server_to_dp(), id_to_public,
        survey_id, op, ranges, ps, proofs, obfuscation, thresholds, diffp or QueryDiffP(), gen, cutting_factor,
        verification_sharding, range_proof_mode)
    if sql is not None:
        sq.Query.SQL = sql
    return sq


def make_iterative_survey(client: DrynxClient, cluster, op_name: str, base: int, *, query_min=0, query_max=10,
                          rows=10, group_by=(1,), proofs=0, thresholds=None, survey_id=None, sig_device="cpu",
                          deterministic_sigs=False, verification_sharding=0, with_vns=None, range_proof_mode=0,
                          ranges=None, sql=None):
    """The survey ``DrynxClient.send_iterative_extreme(sq, base)`` runs in rounds:
    a ``min``/``max`` over the full domain [query_min, query_max] whose ranges
    and input-validation signatures cover the ``base`` outputs of a round
    ((2, 1) each, made once and shared by every round) instead of one per
    value of the domain.  For ``frequencyCount`` it is the survey
    ``send_iterative_quantile`` runs: the outputs are counts, and with proofs
    the ``ranges`` given ((u, l), or one per output) serve all ``base`` columns.
    ``sql``: ``make_survey``'s -- the searches then run per cell of the WHERE / GROUP BY."""
    from ..query import iter_operation

    if op_name == "frequencyCount":
        if proofs and ranges is None:
            raise ValueError("an iterative frequencyCount with proofs needs the ranges of its counts")
        ranges = ranges if proofs else None
    else:
        ranges = [2, 1] if proofs else None
    sq = make_survey(client, cluster, op_name, query_min=query_min, query_max=query_min + base - 1, rows=rows,
                     group_by=group_by, proofs=proofs, ranges=ranges, thresholds=thresholds,
                     survey_id=survey_id, sig_device=sig_device, deterministic_sigs=deterministic_sigs,
                     verification_sharding=verification_sharding, with_vns=with_vns, range_proof_mode=range_proof_mode,
                     sql=sql)
    sq.Query.Operation = iter_operation(op_name, query_min, query_max, base)
    sq.Query.DPDataGen.GenerateDataMax = int(query_max)
    sq.IterBase = int(base)
    return sq


def make_kmeans_survey(client: DrynxClient, cluster, k: int, d: int, scale: int, rounds: int, *, query_min=0,
                       query_max=10, rows=10, group_by=(1,), proofs=0, ranges=None, thresholds=None, survey_id=None,
                       sig_device="cpu", deterministic_sigs=False, verification_sharding=0, with_vns=None,
                       range_proof_mode=0):
    """The survey ``DrynxClient.send_kmeans(sq, centroids)`` runs in rounds:
    ``k`` clusters of records with ``d`` columns over [query_min, query_max],
    centroids in units of 1 / ``scale``, ``rounds`` Lloyd rounds.  Its k * (d +
    2) outputs are counts and sums: with proofs the ``ranges`` given ((u, l),
    or one per output) must hold a DP's largest sum of squares, and they and
    the input-validation signatures are made once and shared by every round."""
    from ..query import KMeansParameters, kmeans_operation

    op = kmeans_operation(query_min, query_max, d, k)
    if proofs and ranges is None:
        raise ValueError("a k-means survey with proofs needs the ranges of its sums")
    # (a survey with as many outputs: make_survey sizes the ranges and signatures by them)
    sq = make_survey(client, cluster, "frequencyCount", query_min=query_min, query_max=query_min + op.NbrOutput - 1,
                     rows=rows, group_by=group_by, proofs=proofs, ranges=ranges if proofs else None,
                     thresholds=thresholds, survey_id=survey_id, sig_device=sig_device,
                     deterministic_sigs=deterministic_sigs, verification_sharding=verification_sharding,
                     with_vns=with_vns, range_proof_mode=range_proof_mode)
    op.KMeans = KMeansParameters(K=int(k), Scale=int(scale), Round=0, Rounds=int(rounds))
    sq.Query.Operation = op
    sq.Query.DPDataGen.GenerateDataMax = int(query_max)
    return sq


def clear_expected(op_name, clear_dp: dict):
    """Sum of the DPs' clear responses (first group) for checking decoded results."""
    tot = None
    for v in clear_dp.values():
        g0 = v[0]
        tot = list(g0) if tot is None else [a + b for a, b in zip(tot, g0)]
    return tot


__all__ = ["local_cluster", "make_survey", "make_iterative_survey", "make_kmeans_survey", "make_signatures",
           "RANGE_PRESETS", "clear_expected", "O"]
