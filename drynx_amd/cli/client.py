"""``drynx-client``: network new|add-node|set-client ; survey new|set-operation|run
(reference cmd/client/main.go:33-69, network.go, survey.go:61-154).  Config
streams are TOML on stdin/stdout so commands pipe into each other."""
from __future__ import annotations

import argparse
import sys

from . import toml_io


def _read():
    data = sys.stdin.read() if not sys.stdin.isatty() else ""
    return toml_io.loads(data)


def _write(cfg):
    sys.stdout.write(toml_io.dumps(cfg))


def network_new(a):
    cfg = _read()
    cfg["Network"] = {"Nodes": []}
    _write(cfg)


def network_add_node(a):
    cfg = _read()
    net = cfg.setdefault("Network", {})
    net.setdefault("Nodes", []).append({"Address": a.address, "PublicKey": a.public})
    _write(cfg)


def network_set_client(a):
    cfg = _read()
    cfg.setdefault("Network", {})["Client"] = {"URL": a.address}
    _write(cfg)


def survey_new(a):
    cfg = _read()
    cfg["Survey"] = {"Name": a.name}
    _write(cfg)


def survey_set_operation(a):
    cfg = _read()
    cfg.setdefault("Survey", {})["Operation"] = a.operation
    _write(cfg)


_WHERE_OPS = (">=", "<=", "==", "!=", "<", ">", "=")  # two-character operators first


def where_terms(terms, predicate: str):
    """``--where COLUMN OP VALUE`` (repeatable) and ``--predicate`` -> ([(name,
    value)], formula).  ``=`` and ``==`` are the equality of a plain
    conjunction; any other operator makes the formula ``v0 OP v1 && v2 OP v3
    ...`` here, which a ``--predicate`` of the caller's would contradict."""
    where, ops = [], []
    for term in terms or []:
        at = [(term.find(op), op) for op in _WHERE_OPS if op in term]
        if not at:
            raise SystemExit(f"--where {term}: expected COLUMN=VALUE, or COLUMN OP VALUE with OP one of "
                             "== != < <= > >=")
        pos = min(p for p, _ in at)
        op = next(o for p, o in at if p == pos)  # the longest operator at the first position
        where.append((term[:pos].strip(), term[pos + len(op):].strip()))
        ops.append("==" if op == "=" else op)
    if any(op != "==" for op in ops):
        if predicate:
            raise SystemExit("--where with an operator other than = together with --predicate: write the "
                             "comparisons into the formula (v0 >= v1 ...) and give --where COLUMN=VALUE terms")
        predicate = " && ".join(f"v{2 * i} {op} v{2 * i + 1}" for i, op in enumerate(ops))
    return where, predicate or ""


def kmeans_centroids(text: str, k: int, d: int, qmin: int, scale: int) -> list:
    """``--centroids "x,y;x,y"``: k points of d coordinates in record units ->
    the k * d scaled offsets (x - qmin) * scale, which must be whole."""
    from fractions import Fraction

    pts = [[v.strip() for v in pt.split(",") if v.strip()] for pt in text.split(";") if pt.strip()]
    if len(pts) != k or any(len(pt) != d for pt in pts):
        raise SystemExit(f"--centroids {text}: expected {k} points of {d} coordinates, as in \"x,y;x,y\"")
    out = []
    for pt in pts:
        for v in pt:
            try:
                c = (Fraction(v) - qmin) * scale
            except (ValueError, ZeroDivisionError):
                raise SystemExit(f"--centroids {text}: {v} is not a number")
            if c.denominator != 1:
                raise SystemExit(f"--centroids {text}: {v} is not a multiple of 1/{scale} (--scale)")
            out.append(int(c))
    return out


def survey_run_kmeans(a, cfg, client, sq):
    """``survey set-operation kmeans`` ... ``survey run --clusters K --dims D
    --rounds N [--scale S] [--centroids "x,y;x,y"]``: K clusters of the DPs'
    records (their first D columns, over [0, 256]) in N verifiable rounds.
    The default start centroids are ``kmeans.random_centroids`` seeded from the
    survey name.  Prints one line per cluster: its index, the records the last
    round assigned to it, and its centroid in record units."""
    from .. import kmeans as km
    from ..query import KMeansParameters, check_parameters, kmeans_operation

    if a.group_by or a.cardinalities or a.where or a.predicate or a.select:
        raise SystemExit("kmeans over SQL cohorts is not defined: no --group-by, --where, --predicate or --select")
    if a.clusters is None or a.dims is None or a.rounds is None:
        raise SystemExit("kmeans needs --clusters K --dims D --rounds N")
    g = sq.Query.DPDataGen
    try:
        op = kmeans_operation(g.GenerateDataMin, g.GenerateDataMax, a.dims, a.clusters)
        km.check(a.clusters, a.dims, op.QueryMin, op.QueryMax, a.scale)
        km.check_rounds(a.rounds)
    except ValueError as e:
        raise SystemExit(str(e))
    R = op.QueryMax - op.QueryMin + 1
    if a.centroids:
        start = kmeans_centroids(a.centroids, a.clusters, a.dims, op.QueryMin, a.scale)
    else:
        start = km.random_centroids(a.clusters, a.dims, R, a.scale, cfg["Survey"].get("Name") or "")
    op.KMeans = KMeansParameters(K=a.clusters, Scale=a.scale, Round=0, Rounds=a.rounds, Centroids=start)
    sq.Query.Operation = op
    if not check_parameters(sq, False):
        raise SystemExit("the k-means query is not valid (see the log)")
    res = client.send_kmeans(sq, start)
    for c, (n, pt) in enumerate(zip(res.counts, res.points)):
        print(f"{c}: {n}: " + " ".join(str(float(x)) for x in pt))


def survey_run(a):
    """roster[0] is the CN (and the VN roster), roster[1:] are DPs; no proofs;
    GroupBy {3,2,1}; 10 rows in [0, 256] (survey.go:93-132).  ``--group-by c1,c3
    --cardinalities 3,2``, ``--where c2=1`` or ``--where 'c2>=2'`` (repeatable: a
    conjunction), ``--predicate 'v0 == v1 || v2 < v3'`` (a formula over the
    --where terms, ``QuerySQL.Predicate``) and ``--select c0`` fill the query's
    SQL (``query.QuerySQL``); with a GROUP BY every group's key and result are
    printed, one line each."""
    from ..crypto import oracle as O
    from ..query import (QueryDPDataGen, QueryDiffP, QuerySQL, Roster, ServerIdentity, WhereClear, check_parameters,
                         choose_operation)
    from ..services.api import DrynxClient
    from ..services.server import RemoteNode

    terms, predicate = where_terms(a.where, a.predicate)  # refused here: nothing has been sent yet
    where = [WhereClear(name, value) for name, value in terms]
    cfg = _read()
    nodes = cfg["Network"]["Nodes"]
    if len(nodes) < 2:
        raise SystemExit("need at least 2 nodes (1 CN + >=1 DP)")
    entry = cfg["Network"].get("Client", {}).get("URL") or nodes[0]["Address"]
    ids = [n["Address"] for n in nodes]
    pubs = {n["Address"]: O.g1_from_bytes(bytes.fromhex(n["PublicKey"])) for n in nodes}
    cn, dps = ids[0], ids[1:]
    roster = Roster([ServerIdentity(f"cn:{cn}", pubs[cn], cn, 0)])
    id_to_pub = {f"cn:{cn}": pubs[cn], f"vn:{cn}": pubs[cn]}
    id_to_pub.update({f"dp:{d}": pubs[d] for d in dps})
    s2dp = {f"cn:{cn}": [ServerIdentity(f"dp:{d}", pubs[d], d, i + 1) for i, d in enumerate(dps)]}
    kmeans = cfg["Survey"]["Operation"] == "kmeans"  # its operation is survey_run_kmeans' to build
    op = choose_operation("sum" if kmeans else cfg["Survey"]["Operation"], 0, 256, 5, 0)
    client = DrynxClient(RemoteNode(entry))  # the roster travels inside the SurveyQuery
    sq = client.generate_survey_query(roster, None, s2dp, id_to_pub, cfg["Survey"].get("Name"), op, None, None, 0,
                                      False, [0.0] * 5, QueryDiffP(), QueryDPDataGen([3, 2, 1], 10, 0, 256))
    if kmeans:
        return survey_run_kmeans(a, cfg, client, sq)
    csv = lambda v: [x.strip() for x in (v or "").split(",") if x.strip()]  # noqa: E731
    sq.Query.SQL = QuerySQL(Select=csv(a.select), Where=where, Predicate=predicate, GroupBy=csv(a.group_by))
    if sq.Query.SQL.GroupBy:
        try:
            sq.Query.DPDataGen.GroupByValues = [int(v) for v in csv(a.cardinalities)]
        except ValueError:
            raise SystemExit(f"--cardinalities {a.cardinalities}: integers, one per --group-by column")
    elif a.cardinalities:
        raise SystemExit("--cardinalities without --group-by")
    if sq.Query.SQL and not check_parameters(sq, False):
        raise SystemExit("the SQL part of the query is not valid (see the log)")
    groups, values, _ = client.send_survey_query(sq)
    if sq.Query.SQL.GroupBy:  # real groups: one line each
        for g, v in zip(groups, values):
            print(g + ": " + " ".join(str(x) for x in v))
        return
    first = values[0]
    if any(v != first for v in values):
        raise SystemExit(f"groups disagree: {values}")
    print(" ".join(str(v) for v in first))


def main(argv=None):
    ap = argparse.ArgumentParser(prog="drynx-client")
    sub = ap.add_subparsers(dest="group", required=True)
    net = sub.add_parser("network").add_subparsers(dest="cmd", required=True)
    net.add_parser("new").set_defaults(fn=network_new)
    p = net.add_parser("add-node")
    p.add_argument("address")
    p.add_argument("public")
    p.set_defaults(fn=network_add_node)
    p = net.add_parser("set-client")
    p.add_argument("address")
    p.set_defaults(fn=network_set_client)
    sv = sub.add_parser("survey").add_subparsers(dest="cmd", required=True)
    p = sv.add_parser("new")
    p.add_argument("name")
    p.set_defaults(fn=survey_new)
    p = sv.add_parser("set-operation")
    p.add_argument("operation")
    p.set_defaults(fn=survey_set_operation)
    p = sv.add_parser("run")
    p.add_argument("--group-by", default="", help="columns to group by, e.g. c1,c3")
    p.add_argument("--cardinalities", default="", help="values per --group-by column, e.g. 3,2")
    p.add_argument("--where", action="append",
                   help="COLUMN OP VALUE with OP one of = == != < <= > >=, e.g. c2=1 or 'c2>=2' (repeatable: a "
                        "conjunction, or the terms of --predicate)")
    p.add_argument("--predicate", default="",
                   help="a formula over the --where terms, v{2i} the column and v{2i+1} the value of term i, "
                        "e.g. 'v0 == v1 || !(v2 == v3)'")
    p.add_argument("--select", default="", help="the operation's input columns, e.g. c0")
    p.add_argument("--clusters", type=int, help="kmeans: the number of clusters K")
    p.add_argument("--dims", type=int, help="kmeans: the columns D of a record")
    p.add_argument("--rounds", type=int, help="kmeans: the number of rounds N")
    p.add_argument("--scale", type=int, default=1, help="kmeans: centroids move in steps of 1/SCALE (default 1)")
    p.add_argument("--centroids", default="", help="kmeans: the K start points, e.g. \"10,20;200,40\" "
                                                     "(default: drawn from the survey name)")
    p.set_defaults(fn=survey_run)
    a = ap.parse_args(argv)
    a.fn(a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
