"""Survey/query data model, validation and planning.

Mirrors the reference's lib/structs.go:
  * QueryDiffP / QueryDPDataGen / QueryIVSigs / Query / Operation /
    LogisticRegressionParameters / SurveyQuery          (structs.go:144-247)
  * add_diff_p            (structs.go:423)
  * check_parameters      (structs.go:446-533)
  * query_to_proofs_nbrs  (structs.go:536-568)
  * choose_operation      (structs.go:591-642)
Everything serialises to plain JSON-able dicts for the control plane.
"""
from __future__ import annotations

import copy
import hashlib
import uuid
from dataclasses import dataclass, field, fields, is_dataclass
from typing import Optional

from . import kmeans as km
from .crypto import oracle as O
from .rounds import (ITER_MAX_BASE, ITER_MAX_CELL_OUTPUTS, ITER_MAX_HIST_BASE, ITER_MAX_RANGE,  # re-exported
                     ITER_OPERATIONS, iter_rounds)
from .utils.log import get_logger

log = get_logger("query")

OPERATIONS = ("sum", "mean", "variance", "cosim", "frequencyCount", "min", "max", "union", "inter", "bool_OR",
              "bool_AND", "lin_reg", "logistic regression", "MLeval")


# ----------------------------------------------------------------------------- identities
@dataclass
class ServerIdentity:
    """A node of the roster (onet ServerIdentity): id, public key, address, GPU rank."""
    id: str
    public: Optional[tuple] = None  # G1 affine (oracle) point
    address: str = ""
    rank: int = 0
    bls: Optional[tuple] = None     # G2 BLS key (verifying nodes: skipchain collective signature)

    def to_dict(self):
        d = {"id": self.id, "public": O.g1_to_bytes(self.public).hex() if self.public else None,
             "address": self.address, "rank": self.rank}
        if self.bls is not None:
            d["bls"] = O.g2_to_bytes(self.bls).hex()
        return d

    @staticmethod
    def from_dict(d):
        pub = O.g1_from_bytes(bytes.fromhex(d["public"])) if d.get("public") else None
        b = O.g2_from_bytes(bytes.fromhex(d["bls"])) if d.get("bls") else None
        return ServerIdentity(d["id"], pub, d.get("address", ""), d.get("rank", 0), b)

    def __hash__(self):
        return hash(self.id)


@dataclass
class Roster:
    list: list = field(default_factory=list)

    def aggregate(self):
        """Collective public key = sum of member keys (onet Roster.Aggregate)."""
        acc = None
        for si in self.list:
            acc = O.g1_add(acc, si.public)
        return acc

    def ids(self):
        return [s.id for s in self.list]

    def to_dict(self):
        return [s.to_dict() for s in self.list]

    @staticmethod
    def from_dict(d):
        return Roster([ServerIdentity.from_dict(x) for x in (d or [])])


# ----------------------------------------------------------------------------- query structs
@dataclass
class QueryDiffP:
    LapMean: float = 0.0
    LapScale: float = 0.0
    NoiseListSize: int = 0
    Quanta: float = 0.0
    Scale: float = 0.0
    Limit: float = 0.0


@dataclass
class QueryDPDataGen:
    GroupByValues: list = field(default_factory=lambda: [1])
    GenerateRows: int = 0
    GenerateDataMin: int = 0
    GenerateDataMax: int = 0


@dataclass
class PublishSignatureBytes:
    """Per-CN range-proof setup: public y = x*B and BB signatures A_k = (x+k)^-1 B2 (u of them, 128 B each)."""
    Public: bytes = b""
    Signature: bytes = b""

    def to_dict(self):
        return {"Public": self.Public.hex(), "Signature": self.Signature.hex()}

    @staticmethod
    def from_dict(d):
        return PublishSignatureBytes(bytes.fromhex(d["Public"]), bytes.fromhex(d["Signature"]))


@dataclass
class QueryIVSigs:
    # InputValidationSigs[cn][output] -> PublishSignatureBytes
    InputValidationSigs: Optional[list] = None
    InputValidationSize1: int = 0
    InputValidationSize2: int = 0


@dataclass
class LogisticRegressionParameters:
    DatasetName: str = ""
    FilePath: str = ""
    NbrRecords: int = 0
    NbrFeatures: int = 0
    Means: list = field(default_factory=list)
    StandardDeviations: list = field(default_factory=list)
    Lambda: float = 0.0
    Step: float = 0.0
    MaxIterations: int = 0
    InitialWeights: list = field(default_factory=list)
    K: int = 2
    PrecisionApproxCoefficients: float = 1.0
    # extension: layout of the level-2 coefficients.  0 = the reference's
    # cartesian (d+1)^2 values; 1 = distinct: only the upper triangle (i <= j)
    # of the symmetric level-2 matrix, row-major, D(D+1)/2 values (K <= 2).
    Packing: int = 0
    # extension: label columns.  0 and 1 = the reference's single-label query;
    # 2..64 = T binary models over the same features in one query: the DPs'
    # labels are [N, T], level 1 is sent once per target (target-major) and
    # level 2, whose weight y - y(-1)^2 - 1 = -1 does not depend on the label,
    # once for all of them (K <= 2).  Travels as SurveyQuery.LRTargets on the wire.
    NbrTargets: int = 0


@dataclass
class KMeansParameters:
    """extension: one round of a k-means query (``drynx_amd.kmeans``, the
    operation ``kmeans``).  The records have NbrInput = d columns over
    [QueryMin, QueryMax]; ``Centroids`` are the K * d coordinates the round
    assigns by, cluster-major, integers in units of 1 / ``Scale``; ``Round`` of
    ``Rounds`` counts from 0.  ``SearchID`` is the id the rounds of one run
    share: generated records are seeded from it, so every round sees the same
    data."""
    K: int = 0
    Scale: int = 1
    Round: int = 0
    Rounds: int = 1
    Centroids: list = field(default_factory=list)
    SearchID: str = ""


@dataclass
class Operation:
    NameOp: str = ""
    NbrInput: int = 0
    NbrOutput: int = 0
    QueryMin: int = 0
    QueryMax: int = 0
    LRParameters: LogisticRegressionParameters = field(default_factory=LogisticRegressionParameters)
    KMeans: Optional[KMeansParameters] = None  # set for the operation "kmeans" only


@dataclass
class WhereClear:
    """One term of a WHERE clause (structs.go WhereQueryAttributeClear): column
    ``Name`` == int(``Value``), or the atom ``Name`` OP int(``Value``) that
    ``QuerySQL.Predicate`` makes of it."""
    Name: str = ""
    Value: str = ""


@dataclass
class QuerySQL:
    """structs.go:168-193 QuerySQL ("if real DB at data providers").  The
    reference declares it and never reads it; the semantics are ours:

    * a column name is ``c<k>``, the zero-based column k < 64 of a DP's record table;
    * ``Select``: the NbrInput columns the operation reads, in its input order
      (empty: c0 .. c{NbrInput-1});
    * ``Where``: at most 8 terms (column, int(Value)).  With an empty
      ``Predicate`` a record passes if every column equals its value (the
      conjunction of equalities);
    * ``Predicate``: a formula in the UnLynx syntax over the Where terms, where
      ``v{2i}`` names the column of ``Where[i]`` and ``v{2i+1}`` its value.  An
      atom is ``v{2i} OP v{2i+1}`` with OP one of ``== != < <= > >=`` (signed
      int64, exact at both ends); atoms combine with ``!``, ``&&`` (binds
      tighter), ``||`` and parentheses, ASCII spaces allowed, at most 256
      characters and 16 nested parentheses.  Every Where term appears in exactly
      one atom (a column compared twice is listed twice), and a record passes
      if the formula holds for it: ``v0 >= v1 && v2 < v3`` with Where = [(c4,
      40), (c4, 65)] is 40 <= c4 < 65;
    * ``GroupBy``: at most 4 columns; ``DPDataGen.GroupByValues[i]`` is the
      cardinality V_i of ``GroupBy[i]`` (product at most 4096), a record belongs
      to the group of its values in those columns, in ``all_possible_groups``
      order, and a record with a value outside [0, V_i) is dropped;
    * ``Where`` without ``GroupBy``: the filtered answer is replicated over the
      groups of ``GroupByValues`` as an unfiltered one is;
    * ``logistic regression``: one model per cell (cohort).  The columns are
      those of a DP's key table K [N, width] int64, row i the keys of record i
      of its float features; ``Select`` must stay empty; LRParameters has K = 2
      (level 2's first entry carries the cell's record count, with which the
      querier descends) and global Means and StandardDeviations; an empty cell
      decodes to NaN weights;
    * iterative rounds (``SurveyQuery.IterBase`` with ``min``, ``max`` or
      ``frequencyCount``): one search per cell, cell g under
      ``SurveyQuery.IterPrefixes[g]``; a cell's records are those of its group
      that pass ``Where``, lie in [QueryMin, QueryMax] and under its prefix.

    All empty = the query without SQL, in every respect."""
    Select: list = field(default_factory=list)
    Where: list = field(default_factory=list)
    Predicate: str = ""
    GroupBy: list = field(default_factory=list)

    def __bool__(self):
        return bool(self.Select or self.Where or self.Predicate or self.GroupBy)


SQL_MAX_COLUMNS = 64
SQL_MAX_WHERE = 8
SQL_MAX_GROUP_BY = 4
SQL_MAX_GROUPS = 4096
SQL_OPERATIONS = ("sum", "mean", "variance", "cosim", "lin_reg", "MLeval", "frequencyCount", "union", "inter", "min",
                  "max")


def sql_column(name) -> int:
    """Index k of the column name ``c<k>``; ValueError for anything else."""
    if not isinstance(name, str) or len(name) < 2 or name[0] != "c" or not name[1:].isdigit() \
            or not name[1:].isascii() or (len(name) > 2 and name[1] == "0"):
        raise ValueError(f"malformed column name {name!r} (c<k>)")
    k = int(name[1:])
    if k >= SQL_MAX_COLUMNS:
        raise ValueError(f"column {name} outside c0..c{SQL_MAX_COLUMNS - 1}")
    return k


SQL_MAX_PREDICATE_CHARS = 256
SQL_MAX_PREDICATE_DEPTH = 16
SQL_COMPARISONS = ("==", "!=", "<", "<=", ">", ">=")  # native.GROUP_OPS
_NO_PREDICATE = "without a predicate only the conjunction of the Where equalities is defined"


def _predicate_tokens(text: str) -> list:
    """The tokens of a predicate formula: ("v", k), a comparison, "!", "&&",
    "||", "(" or ")".  ValueError (the complaint alone) for anything else."""
    out, i = [], 0
    while i < len(text):
        c = text[i]
        if c == " ":
            i += 1
        elif c == "v":
            j = i + 1
            while j < len(text) and text[j] in "0123456789":
                j += 1
            digits = text[i + 1:j]
            if not digits or (len(digits) > 1 and digits[0] == "0") or len(digits) > 3:
                raise ValueError(f"has the malformed variable {text[i:j]!r} (v<k>, no leading zeros)")
            out.append(("v", int(digits)))
            i = j
        elif text[i:i + 2] in ("==", "!=", "<=", ">=", "&&", "||"):
            out.append(text[i:i + 2])
            i += 2
        elif c in "<>!()":
            out.append(c)
            i += 1
        else:
            raise ValueError(f"has the unknown token {text[i:i + 2].strip()!r}")
    return out


def parse_predicate(text: str, n_terms: int) -> tuple:
    """``QuerySQL.Predicate`` over ``n_terms`` Where terms -> (ops, table): the
    operator of every term's atom ``v{2i} OP v{2i+1}`` and the formula's truth
    table over the atom bits (atom i is bit i of the index) as an int below
    2^(2^n_terms).  ``&&`` binds tighter than ``||``; ``!`` applies to an atom,
    a parenthesis or another ``!``.  Raises ValueError with the complaint alone
    (``sql_plan`` words the refusal).  The formula is not trusted: its length
    and its nesting are capped before anything is built, and the parser keeps
    its own stack."""
    if n_terms < 1:
        raise ValueError("set with no Where term to compare")
    if len(text) > SQL_MAX_PREDICATE_CHARS:
        raise ValueError(f"is longer than {SQL_MAX_PREDICATE_CHARS} characters")
    if not text.isascii():
        raise ValueError("has a character outside ASCII")
    toks = _predicate_tokens(text)
    full = (1 << (1 << n_terms)) - 1
    ops = [None] * n_terms
    # one frame per open parenthesis: [pending negations, the || operands so far, the && operands of the last one]
    stack = [[0, [], []]]
    i, want_operand = 0, True

    def operand(t):
        frame = stack[-1]
        frame[2].append(full ^ t if frame[0] & 1 else t)
        frame[0] = 0

    def close(frame):
        conj = full
        for t in frame[2]:
            conj &= t
        return frame[1] + [conj]

    while i < len(toks):
        t = toks[i]
        if want_operand:
            if t == "!":
                stack[-1][0] += 1
                i += 1
            elif t == "(":
                if len(stack) > SQL_MAX_PREDICATE_DEPTH:
                    raise ValueError(f"nests deeper than {SQL_MAX_PREDICATE_DEPTH} parentheses")
                stack.append([0, [], []])
                i += 1
            elif isinstance(t, tuple):
                a, op, b = t[1], toks[i + 1] if i + 1 < len(toks) else None, toks[i + 2] if i + 2 < len(toks) else None
                if op not in SQL_COMPARISONS or not isinstance(b, tuple) or a % 2 or b[1] != a + 1:
                    raise ValueError(f"has an atom at v{a} that is not v{{2i}} OP v{{2i+1}} with OP one of "
                                     f"{' '.join(SQL_COMPARISONS)}")
                k = a // 2
                if k >= n_terms:
                    raise ValueError(f"names v{a}, Where has {n_terms} terms")
                if ops[k] is not None:
                    raise ValueError(f"uses the Where term {k} (v{a}) twice")
                ops[k] = op
                operand(sum(1 << m for m in range(1 << n_terms) if m >> k & 1))
                i += 3
                want_operand = False
            else:
                raise ValueError(f"has {t!r} where an atom, ! or ( is expected")
        elif t == "&&":
            i, want_operand = i + 1, True
        elif t == "||":
            frame = stack[-1]
            frame[1], frame[2] = close(frame), []
            i, want_operand = i + 1, True
        elif t == ")":
            if len(stack) == 1:
                raise ValueError("has unbalanced parentheses: a ) without its (")
            disj = 0
            for d in close(stack.pop()):
                disj |= d
            operand(disj)
            i += 1
        else:
            raise ValueError(f"has {t if isinstance(t, str) else 'v%d' % t[1]!r} where &&, || or ) is expected")
    if want_operand:
        raise ValueError("is empty" if not toks else "ends where an atom is expected")
    if len(stack) != 1:
        raise ValueError("has unbalanced parentheses: a ( is never closed")
    never = [k for k, op in enumerate(ops) if op is None]
    if never:
        raise ValueError(f"never uses the Where term {never[0]} (v{2 * never[0]})")
    table = 0
    for d in close(stack[0]):
        table |= d
    return tuple(ops), table


@dataclass
class SQLPlan:
    """A checked QuerySQL in column indices: ``select`` (the operation's input
    columns; none for a logistic regression), ``where`` [(column, value)],
    ``group_by`` [(column, cardinality)] and the table ``width`` (1 + the
    largest referenced column).  ``predicate``: None -- a record passes if it
    equals every ``where`` value -- or ``(ops, table)`` of ``parse_predicate``:
    term i is the atom ``column ops[i] value`` and a record passes if bit
    ``sum(atom_i << i)`` of ``table`` is set.  The plain conjunction of
    equalities is always None."""
    select: list
    where: list
    group_by: list
    width: int
    predicate: Optional[tuple] = None


def sql_plan(q: "Query") -> Optional[SQLPlan]:
    """The plan of a query's SQL part, None when it has none.  Raises
    ValueError with the violated rule (``check_parameters`` reports it)."""
    sql = q.SQL
    if not sql:
        return None
    n_in = max(1, q.Operation.NbrInput)
    if q.Operation.NameOp == "logistic regression":
        # the columns are those of a DP's key table, beside its float features
        if sql.Select:
            raise ValueError("SQL select with logistic regression: the features are the DP's float matrix, "
                             "not table columns")
        select = []
    else:
        select = [sql_column(n) for n in sql.Select] if sql.Select else list(range(n_in))
        if len(select) != n_in:
            raise ValueError(f"SQL select lists {len(select)} columns, the operation reads {n_in}")
    if len(sql.Where) > SQL_MAX_WHERE:
        raise ValueError(f"SQL where has more than {SQL_MAX_WHERE} terms")
    where = []
    for w in sql.Where:
        col = sql_column(w.Name)
        v = str(w.Value).strip()
        if not (v[1:] if v[:1] in "+-" else v).isdigit() or not v.isascii():
            raise ValueError(f"SQL where value {w.Value!r} is not an integer")
        if not -(1 << 63) <= int(v) < 1 << 63:
            raise ValueError(f"SQL where value {w.Value!r} is not an int64")
        where.append((col, int(v)))
    predicate = None
    if sql.Predicate:
        try:
            ops, table = parse_predicate(str(sql.Predicate), len(where))
        except ValueError as e:
            raise ValueError(f"SQL predicate {e}; {_NO_PREDICATE}") from None
        if any(op != "==" for op in ops) or table != 1 << ((1 << len(where)) - 1):
            predicate = (ops, table)  # the plain conjunction stays None: the plan of the query without a predicate
    group_by = []
    if sql.GroupBy:
        if len(sql.GroupBy) > SQL_MAX_GROUP_BY:
            raise ValueError(f"SQL group by has more than {SQL_MAX_GROUP_BY} columns")
        cards = list(q.DPDataGen.GroupByValues or [])
        if len(cards) != len(sql.GroupBy):
            raise ValueError("GroupByValues does not give one cardinality per SQL group-by column")
        total = 1
        for name, v in zip(sql.GroupBy, cards):
            if not isinstance(v, int) or isinstance(v, bool) or v < 1:
                raise ValueError("a SQL group-by cardinality below 1")
            total *= v
            group_by.append((sql_column(name), v))
        if total > SQL_MAX_GROUPS:
            raise ValueError(f"SQL group by over {total} groups (at most {SQL_MAX_GROUPS})")
    width = 1 + max(select + [c for c, _ in where] + [c for c, _ in group_by])
    return SQLPlan(select, where, group_by, width, predicate)


@dataclass
class Query:
    Operation: Operation = field(default_factory=Operation)
    Ranges: Optional[list] = None  # list of [u, l] (optionally [u, l, offset])
    Proofs: int = 0
    Obfuscation: bool = False
    DiffP: QueryDiffP = field(default_factory=QueryDiffP)
    DPDataGen: QueryDPDataGen = field(default_factory=QueryDPDataGen)
    IVSigs: QueryIVSigs = field(default_factory=QueryIVSigs)
    RosterVNs: Optional[Roster] = None
    CuttingFactor: int = 0
    SQL: QuerySQL = field(default_factory=QuerySQL)


@dataclass
class SurveyQuery:
    SurveyID: str = ""
    RosterServers: Roster = field(default_factory=Roster)
    ClientPubKey: Optional[tuple] = None
    IntraMessage: bool = False
    ServerToDP: dict = field(default_factory=dict)  # CN id -> [DP ServerIdentity]
    Query: Query = field(default_factory=Query)
    IDtoPublic: dict = field(default_factory=dict)
    Threshold: float = 0.0
    AggregationProofThreshold: float = 0.0
    ObfuscationProofThreshold: float = 0.0
    RangeProofThreshold: float = 0.0
    KeySwitchingProofThreshold: float = 0.0
    # extension: >0 -> each proof request is verified by exactly this many VNs
    # (deterministic sharding of the verification work across GPUs); 0 -> the
    # reference's random sampling with probability Threshold.
    VerificationSharding: int = 0
    # extension: range-proof verification mode.  0 = the reference
    # (RangeProofVerification trusts the proof's challenge, range_proof.go:
    # 504-565); 1 = strict: the VN recomputes c = SHA3-512(B||C||sum y) and
    # checks every V_ij in G2; 2 = strict with the v2 transcript, whose
    # challenge also binds D and every V_ij, a_ij (range_proof.go:350-374 omits them).
    RangeProofMode: int = 0
    # extension: iterative min/max.  IterBase b > 0 makes the query ONE round of
    # a digit-by-digit search: the DPs answer with the unary encoding (b
    # outputs) of the IterRound-th base-b digit of their extreme, most
    # significant first, if its leading digits equal IterPrefix, and with the
    # neutral value otherwise (csrc/kernels/dx_iter_round.hip).  IterSurveyID is
    # the id the rounds of one search share: generated records are seeded from
    # it, so every round sees the same data.  0 = the reference's one-shot query.
    # A frequencyCount round (the rounds of a quantile search) answers with the
    # b counts of that digit among the DP's in-domain records under the prefix
    # (the same kernel file).
    # With a non-empty Query.SQL the round is one round of G simultaneous
    # searches, one per cell of the SQL plan (G = the product of the GROUP BY
    # cardinalities, 1 with WHERE only; cells in all_possible_groups order):
    # IterPrefix stays 0 and IterPrefixes[g] is cell g's prefix, exactly G
    # entries in every round, all zero in round 0.  Cell g's answer is the
    # round's b values over the records of its group that pass the WHERE
    # conjunction, lie in the domain and under IterPrefixes[g]; min / max are the
    # unary rows of the first / last occupied digit (all zero without a record).
    # Without SQL the list is empty, and an empty list is not sent.
    IterBase: int = 0
    IterRound: int = 0
    IterPrefix: int = 0
    IterSurveyID: str = ""
    IterPrefixes: list = field(default_factory=list)

    # -------------------------------------------------------------- helpers
    def all_dps(self):
        out = []
        for cn in self.RosterServers.list:
            out += list(self.ServerToDP.get(cn.id) or [])
        return out

    def to_dict(self) -> dict:
        return _to_jsonable(self)

    @staticmethod
    def from_dict(d: dict) -> "SurveyQuery":
        return _survey_from_dict(d)


_digest_memo: dict = {}


def ivsigs_digest(sigs) -> str:
    """sha256 over a signature set (memoised per list object: the same CN
    input-validation keys serve many surveys)."""
    if not sigs:
        return ""
    hit = _digest_memo.get(id(sigs))
    if hit is not None and hit[0] is sigs:
        return hit[1]
    h = hashlib.sha256()
    for row in sigs:
        h.update(len(row).to_bytes(4, "little"))
        for s in row:
            h.update(s.Public)
            h.update(s.Signature)
    d = h.hexdigest()
    if len(_digest_memo) > 16:
        _digest_memo.clear()
    _digest_memo[id(sigs)] = (sigs, d)
    return d


def _to_jsonable(obj):
    if isinstance(obj, (ServerIdentity, Roster, PublishSignatureBytes)):
        return obj.to_dict()
    if is_dataclass(obj):
        out = {}
        for f in fields(obj):
            v = getattr(obj, f.name)
            if f.name == "ClientPubKey":
                out[f.name] = O.g1_to_bytes(v).hex() if v is not None else None
            elif f.name == "IDtoPublic":
                out[f.name] = {k: O.g1_to_bytes(p).hex() for k, p in v.items()}
            elif f.name == "ServerToDP":
                out[f.name] = {k: ([s.to_dict() for s in lst] if lst is not None else None) for k, lst in v.items()}
            elif f.name == "InputValidationSigs":
                out[f.name] = None if v is None else [[s.to_dict() for s in row] for row in v]
            elif isinstance(v, QuerySQL) and not v:
                continue  # an empty SQL is the dict of a query without the field
            elif f.name == "IterPrefixes" and not v:
                continue  # likewise: the dict of every survey without cell prefixes is unchanged
            elif f.name == "KMeans" and v is None:
                continue  # and the dict of every operation but k-means
            else:
                out[f.name] = _to_jsonable(v)
        return out
    if isinstance(obj, (list, tuple)):
        return [_to_jsonable(x) for x in obj]
    if isinstance(obj, dict):
        return {k: _to_jsonable(v) for k, v in obj.items()}
    return obj


def sql_from_dict(d) -> QuerySQL:
    """QuerySQL of its dict (JSON control plane or decoded wire message); a
    peer without the field (None, {}) reads as the empty SQL."""
    d = d or {}
    return QuerySQL(Select=[str(s) for s in d.get("Select") or []],
                    Where=[WhereClear(str(w.get("Name", "")), str(w.get("Value", ""))) for w in d.get("Where") or []],
                    Predicate=str(d.get("Predicate") or ""),
                    GroupBy=[str(s) for s in d.get("GroupBy") or []])


def kmeans_from_dict(d) -> Optional[KMeansParameters]:
    """KMeansParameters of their dict (JSON control plane or decoded wire
    message); a peer without the block (None) reads as no k-means."""
    if d is None:
        return None
    return KMeansParameters(K=int(d.get("K") or 0), Scale=int(d.get("Scale") or 0), Round=int(d.get("Round") or 0),
                            Rounds=int(d.get("Rounds") or 0), Centroids=[int(c) for c in d.get("Centroids") or []],
                            SearchID=str(d.get("SearchID") or ""))


def _survey_from_dict(d: dict) -> SurveyQuery:
    q = d["Query"]
    op = dict(q["Operation"])
    op["LRParameters"] = LogisticRegressionParameters(**op.get("LRParameters", {}))
    op["KMeans"] = kmeans_from_dict(op.get("KMeans"))
    ivs = dict(q.get("IVSigs") or {})
    if ivs.get("InputValidationSigs") is not None:
        ivs["InputValidationSigs"] = [[PublishSignatureBytes.from_dict(s) for s in row]
                                      for row in ivs["InputValidationSigs"]]
    query = Query(
        Operation=Operation(**op),
        Ranges=q.get("Ranges"),
        Proofs=q.get("Proofs", 0),
        Obfuscation=q.get("Obfuscation", False),
        DiffP=QueryDiffP(**q.get("DiffP", {})),
        DPDataGen=QueryDPDataGen(**q.get("DPDataGen", {})),
        IVSigs=QueryIVSigs(**ivs),
        RosterVNs=Roster.from_dict(q["RosterVNs"]) if q.get("RosterVNs") is not None else None,
        CuttingFactor=q.get("CuttingFactor", 0),
        SQL=sql_from_dict(q.get("SQL")),
    )
    return SurveyQuery(
        SurveyID=d.get("SurveyID", ""),
        RosterServers=Roster.from_dict(d.get("RosterServers")),
        ClientPubKey=O.g1_from_bytes(bytes.fromhex(d["ClientPubKey"])) if d.get("ClientPubKey") else None,
        IntraMessage=d.get("IntraMessage", False),
        ServerToDP={k: ([ServerIdentity.from_dict(s) for s in v] if v is not None else None)
                    for k, v in (d.get("ServerToDP") or {}).items()},
        Query=query,
        IDtoPublic={k: O.g1_from_bytes(bytes.fromhex(v)) for k, v in (d.get("IDtoPublic") or {}).items()},
        Threshold=d.get("Threshold", 0.0),
        AggregationProofThreshold=d.get("AggregationProofThreshold", 0.0),
        ObfuscationProofThreshold=d.get("ObfuscationProofThreshold", 0.0),
        RangeProofThreshold=d.get("RangeProofThreshold", 0.0),
        KeySwitchingProofThreshold=d.get("KeySwitchingProofThreshold", 0.0),
        VerificationSharding=d.get("VerificationSharding", 0),
        RangeProofMode=d.get("RangeProofMode", 0),
        IterBase=d.get("IterBase", 0),
        IterRound=d.get("IterRound", 0),
        IterPrefix=d.get("IterPrefix", 0),
        IterSurveyID=d.get("IterSurveyID", ""),
        IterPrefixes=list(d.get("IterPrefixes") or []),
    )


# ----------------------------------------------------------------------------- planning / validation
def add_diff_p(qdf: QueryDiffP) -> bool:
    """structs.go:423 — differential privacy is requested iff any parameter is set."""
    return not (qdf.LapMean == 0.0 and qdf.LapScale == 0.0 and qdf.NoiseListSize == 0 and qdf.Quanta == 0.0
                and qdf.Scale == 0 and qdf.Limit == 0)


def _ranges_zeros(ranges) -> bool:
    return all(r[0] == 0 and r[1] == 0 for r in ranges)


def _ranges_bits(ranges) -> bool:
    return all(r[0] == 2 and r[1] == 1 for r in ranges)


def check_parameters(sq: SurveyQuery, diffp: bool) -> bool:
    """structs.go:446-533 consistency rules; logs every violated rule."""
    msg = []
    q = sq.Query
    bool_ops = ("bool_AND", "bool_OR", "min", "max", "union", "inter")
    if q.Proofs == 1:
        if q.Obfuscation:
            if sq.ObfuscationProofThreshold == 0:
                msg.append("obfuscation threshold is 0 while obfuscation is true")
            if q.Operation.NameOp not in bool_ops:
                msg.append("obfuscation threshold for a non accepted operation")
            if q.Ranges is None or not _ranges_bits(q.Ranges):
                msg.append("obfuscation and proofs but ranges not for 0,1")
        elif sq.ObfuscationProofThreshold != 0:
            msg.append("obfuscation threshold is set and there is no Obfuscation")
        if q.Ranges is None:
            msg.append("proofs but no range")
        else:
            sigs = q.IVSigs.InputValidationSigs
            if sigs is None and not _ranges_zeros(q.Ranges):
                msg.append("proofs but no signatures")
            if _ranges_zeros(q.Ranges) and sigs is not None:
                msg.append("ranges to 0 but signatures also set")
            if sigs is not None:
                if q.Operation.NbrOutput != len(sigs[0]) or q.Operation.NbrOutput != len(q.Ranges):
                    msg.append("ranges or signatures length do not match with nbr output")
    elif q.Proofs == 0:
        if sq.KeySwitchingProofThreshold != 0 or sq.ObfuscationProofThreshold != 0 or sq.RangeProofThreshold != 0 \
                or sq.Threshold != 0:
            msg.append("no proofs and one of the threshold not 0")
        if q.Ranges is not None or q.IVSigs.InputValidationSigs is not None:
            msg.append("no proofs and some ranges or signatures")
        if q.RosterVNs is not None:
            msg.append("no proofs but VN roster")
    else:
        msg.append("unsupported proof type")
    d = q.DiffP
    if not diffp:
        if add_diff_p(d):
            msg.append("no diffP but parameters not to 0")
    else:
        if (d.Limit == 0.0 and d.Quanta == 0.0) or d.Scale == 0.0 or d.NoiseListSize == 0 or d.LapScale == 0.0:
            msg.append("diffP but parameters are 0")
    if q.Operation.NameOp == "logistic regression" and q.Operation.LRParameters is not None:
        lrp = q.Operation.LRParameters
        if lrp.Packing not in (0, 1):
            msg.append("logistic regression packing is neither 0 (cartesian) nor 1 (distinct)")
        elif lrp.Packing == 1 and lrp.K > 2:
            msg.append("distinct packing is defined for K <= 2 only")
        nt = lrp.NbrTargets
        if not isinstance(nt, int) or not 0 <= nt <= MAX_LR_TARGETS:
            msg.append(f"logistic regression targets outside 0..{MAX_LR_TARGETS}")
        else:
            if nt > 1 and lrp.K > 2:
                msg.append("several targets share level 2 only: K <= 2 (level 3's weight depends on the label)")
            D = lrp.NbrFeatures + 1
            if len(lrp.InitialWeights or []) not in (0, D, max(1, nt) * D):
                msg.append("initial weights are neither empty, one vector of d + 1 nor one per target")
    msg += _check_iterative(sq)
    msg += _check_sql(sq)
    msg += _check_kmeans(sq)
    if q.Operation.QueryMin != q.DPDataGen.GenerateDataMin or q.Operation.QueryMax != q.DPDataGen.GenerateDataMax:
        msg.append("min or max are inconsistent at DP and operations")
    for m in msg:
        log.warning(m)
    return not msg


def _check_iterative(sq: SurveyQuery) -> list:
    """Rules of the iterative min/max extension (IterBase > 0); nothing when it is off."""
    b = sq.IterBase
    q = sq.Query
    if b == 0:
        if sq.IterRound or sq.IterPrefix or sq.IterPrefixes:
            return ["iterative round or prefix without a base"]
        return []
    if sq.IterPrefixes and not q.SQL:
        return ["iterative cell prefixes (IterPrefixes) without a SQL part"]
    op = q.Operation
    msg = []
    hist = op.NameOp == "frequencyCount"
    # (over SQL cells every operation is derived from the digit's counts)
    top = ITER_MAX_HIST_BASE if hist or q.SQL else ITER_MAX_BASE
    if not isinstance(b, int) or isinstance(b, bool) or not 2 <= b <= top:
        return [f"iterative base outside 2..{top}"]
    if op.NameOp not in ITER_OPERATIONS:
        msg.append("iterative rounds are defined for min, max and frequencyCount only")
    if q.CuttingFactor != 0:
        msg.append("iterative rounds with a cutting factor")
    if add_diff_p(q.DiffP):
        msg.append("iterative rounds with differential privacy")
    R = op.QueryMax - op.QueryMin + 1
    if not 1 <= R <= ITER_MAX_RANGE:
        msg.append(f"iterative rounds over {R} values (1..2^40)")
    else:
        L = iter_rounds(op.QueryMin, op.QueryMax, b)
        if not isinstance(sq.IterRound, int) or not 0 <= sq.IterRound < L:
            msg.append(f"iterative round outside 0..{L - 1}")
        elif not isinstance(sq.IterPrefix, int) or not 0 <= sq.IterPrefix < b ** sq.IterRound:
            msg.append("iterative prefix is not a number of IterRound digits")
    if op.NbrOutput != b:
        msg.append("an iterative round has exactly IterBase outputs")
    if hist:
        # counts, not bits: any range wide enough for a DP's records, one per output
        if q.Proofs and (q.Ranges is None or len(q.Ranges) < b):
            msg.append("an iterative frequencyCount round with proofs needs IterBase ranges")
        elif q.Proofs and not _ranges_zeros(q.Ranges) and any(r[0] == 0 and r[1] == 0 for r in q.Ranges):
            msg.append("an iterative frequencyCount round with (0, 0) among other ranges")
    elif q.Proofs and (q.Ranges is None or not _ranges_bits(q.Ranges)):
        msg.append("iterative rounds with proofs need (2, 1) ranges")
    return msg


def _check_kmeans(sq: SurveyQuery) -> list:
    """Rules of a round of a k-means query (``Operation.KMeans``); nothing for
    every other operation without the block."""
    q = sq.Query
    op = q.Operation
    p = op.KMeans
    if op.NameOp != "kmeans":
        return [] if p is None else [f"k-means parameters with the operation {op.NameOp}"]
    if p is None:
        return ["k-means without its parameters (Operation.KMeans)"]
    try:
        km.check(p.K, op.NbrInput, op.QueryMin, op.QueryMax, p.Scale,
                 p.Centroids if isinstance(p.Centroids, (list, tuple)) else None)
        if not isinstance(p.Centroids, (list, tuple)):
            raise ValueError("k-means: the centroids are not a list")
        km.check_rounds(p.Rounds, p.Round)
    except ValueError as e:
        return [str(e)]
    msg = []
    n_out = p.K * (op.NbrInput + 2)
    if op.NbrOutput != n_out:
        msg.append(f"a k-means round has exactly K * (d + 2) = {n_out} outputs")
    if sq.IterBase:
        msg.append("k-means with iterative digits (IterBase): its rounds are KMeans.Round")
    if q.CuttingFactor != 0:
        msg.append("k-means with a cutting factor")
    if add_diff_p(q.DiffP):
        msg.append("k-means with differential privacy")
    if q.Obfuscation:
        msg.append("k-means with obfuscation")
    # counts and sums, not bits: any range wide enough for a DP's records, one per output
    if q.Proofs and (q.Ranges is None or len(q.Ranges) != n_out):
        msg.append(f"a k-means round with proofs needs one range per output ({n_out})")
    elif q.Proofs and any(r[0] == 0 and r[1] == 0 for r in q.Ranges):
        msg.append("a k-means round with a (0, 0) range")
    return msg


def _check_sql(sq: SurveyQuery) -> list:
    """Rules of a non-empty ``Query.SQL`` (see QuerySQL); nothing when it is empty."""
    q = sq.Query
    if not q.SQL:
        return []
    msg = []
    name = q.Operation.NameOp
    if name in ("bool_AND", "bool_OR"):
        msg.append(f"SQL with {name}: a DP's bit is its first record, not a statistic of its records")
    elif name == "logistic regression":
        lrp = q.Operation.LRParameters
        if lrp is None:
            msg.append("SQL with logistic regression: no LRParameters")
            return msg
        if lrp.K == 1:
            msg.append("SQL with logistic regression: K = 1 carries no record count, an empty cell cannot be told "
                       "from a real one")
        elif lrp.K != 2:
            msg.append(f"SQL with logistic regression: K = {lrp.K} has no fused encoder (K = 2 only)")
        if not (lrp.Means and lrp.StandardDeviations):
            msg.append("SQL with logistic regression: Means and StandardDeviations must be set (the "
                       "standardisation is global; one per cell is not defined)")
    elif name not in SQL_OPERATIONS:
        msg.append(f"SQL with the operation {name}")
    if sq.IterBase and name not in ITER_OPERATIONS:
        msg.append("SQL with iterative rounds")  # no operation with rounds: there are no searches per cell
    if q.CuttingFactor != 0:
        msg.append("SQL with a cutting factor")
    try:
        plan = sql_plan(q)
    except ValueError as e:
        msg.append(str(e))
        return msg
    if sq.IterBase and name in ITER_OPERATIONS:
        bad = _check_cell_prefixes(sq, plan)
        if bad:
            msg.append(f"SQL with iterative rounds: {bad}")
    return msg


def sql_cells(plan: SQLPlan) -> int:
    """G, the cells of a SQL plan: the product of the GROUP BY cardinalities, 1 with WHERE only."""
    G = 1
    for _, v in plan.group_by:
        G *= v
    return G


def _check_cell_prefixes(sq: SurveyQuery, plan: SQLPlan) -> str:
    """The violated rule of a round of G simultaneous searches (SQL with
    IterBase), "" when there is none; the base, the round and the domain are
    ``_check_iterative``'s to refuse."""
    b, k, G = sq.IterBase, sq.IterRound, sql_cells(plan)
    if not isinstance(b, int) or isinstance(b, bool) or not 2 <= b <= ITER_MAX_HIST_BASE:
        return ""
    if G * b > ITER_MAX_CELL_OUTPUTS:
        return f"{G} cells of {b} outputs (at most {ITER_MAX_CELL_OUTPUTS})"
    if sq.IterPrefix != 0:
        return "IterPrefix must stay 0, the cells' prefixes travel in IterPrefixes"
    ps = sq.IterPrefixes
    if not isinstance(ps, (list, tuple)) or len(ps) != G:
        return f"IterPrefixes needs one entry per cell ({G})"
    # the power below is taken for a round of the domain only: IterRound comes off the wire
    op = sq.Query.Operation
    if not 1 <= op.QueryMax - op.QueryMin + 1 <= ITER_MAX_RANGE:
        return ""
    if not isinstance(k, int) or isinstance(k, bool) or not 0 <= k < iter_rounds(op.QueryMin, op.QueryMax, b):
        return ""
    top = b ** k
    if any(not isinstance(p, int) or isinstance(p, bool) or not 0 <= p < top for p in ps):
        return "an entry of IterPrefixes is not a number of IterRound digits" if k else \
            "IterPrefixes must be all zero in round 0"
    return ""


def query_to_proofs_nbrs(sq: SurveyQuery) -> list:
    """structs.go:536-568: expected proofs [range, shuffle, aggregation, obfuscation, keyswitch]."""
    nbr_dps = sum(len(v) for v in sq.ServerToDP.values() if v is not None)
    nbr_servers = len(sq.RosterServers.list)
    prf_range = nbr_dps
    if sq.Query.Proofs == 0:
        nbr_servers = 0
    prf_aggr = nbr_servers
    prf_obf = nbr_servers if sq.Query.Obfuscation else 0
    prf_shuffle = nbr_servers if add_diff_p(sq.Query.DiffP) else 0
    prf_ks = nbr_servers
    return [prf_range, prf_shuffle, prf_aggr, prf_obf, prf_ks]


def choose_operation(name: str, query_min: int, query_max: int, d: int, cutting_factor: int) -> Operation:
    """structs.go:591-642."""
    op = Operation(NameOp=name, NbrInput=0, NbrOutput=0, QueryMin=int(query_min), QueryMax=int(query_max))
    if name == "sum":
        op.NbrInput, op.NbrOutput = 1, 1
    elif name == "mean":
        op.NbrInput, op.NbrOutput = 1, 2
    elif name == "variance":
        op.NbrInput, op.NbrOutput = 1, 3
    elif name == "cosim":
        op.NbrInput, op.NbrOutput = 2, 5
    elif name in ("frequencyCount", "min", "max", "union", "inter"):
        op.NbrInput, op.NbrOutput = 1, int(query_max - query_min + 1)
    elif name in ("bool_OR", "bool_AND"):
        op.NbrInput, op.NbrOutput = 1, 1
    elif name == "lin_reg":
        op.NbrInput, op.NbrOutput = d + 1, (d * d + 5 * d + 4) // 2
    elif name == "logistic regression":
        pass
    elif name == "MLeval":
        # reachable here (the reference log.Fatal's, structs.go:633-635): [N, sum y, sum y^2, SSE]
        op.NbrInput, op.NbrOutput = 2, 4
    else:
        raise ValueError(f"Operation: <{name}> does not exist")
    if cutting_factor != 0:
        op.NbrOutput = op.NbrOutput * cutting_factor
    return op


def iter_operation(name: str, query_min: int, query_max: int, base: int) -> Operation:
    """The operation of one round of an iterative query (extension): the full
    domain stays in QueryMin/QueryMax, the DPs send ``base`` outputs (unary
    bits for min/max, the digit's counts for frequencyCount)."""
    if name not in ITER_OPERATIONS:
        raise ValueError(f"Operation: <{name}> has no iterative rounds")
    iter_rounds(query_min, query_max, base)
    return Operation(NameOp=name, NbrInput=1, NbrOutput=int(base), QueryMin=int(query_min), QueryMax=int(query_max))


def kmeans_operation(query_min: int, query_max: int, d: int, k: int) -> Operation:
    """The operation of one round of a k-means query (extension): ``d`` input
    columns over [query_min, query_max], k * (d + 2) outputs (per cluster the
    count, the d coordinate sums and the sum of squares).  The round's
    parameters (``Operation.KMeans``) are the sender's to set."""
    d, k = int(d), int(k)
    if not 1 <= d <= km.KMEANS_MAX_DIMS or not 1 <= k <= km.max_clusters(d):
        raise ValueError(f"Operation: <kmeans> over {d} columns has no {k} clusters")
    return Operation(NameOp="kmeans", NbrInput=d, NbrOutput=k * (d + 2), QueryMin=int(query_min),
                     QueryMax=int(query_max))


MAX_LR_TARGETS = 64


def lr_nbr_outputs(d: int, k: int, packing: int = 0, targets: int = 1) -> int:
    """getTotalNumberApproxCoefficients (logistic_regression.go:306): sum_j (d+1)^(j+1).
    ``packing`` 1 (extension, k <= 2): level 2 is sent as the D(D+1)/2 distinct
    entries (i <= j) of the symmetric matrix, D = d + 1.  ``targets`` T > 1
    (extension, k <= 2): T level-1 vectors and ONE level 2, T*D + D^2 or
    T*D + D(D+1)/2; 0 and 1 are the single-label count."""
    t = int(targets)
    if not 0 <= t <= MAX_LR_TARGETS:
        raise ValueError(f"no {targets} targets")
    if t > 1 and k > 2:
        raise ValueError(f"{targets} targets for k = {k}: level 3 depends on the label")
    extra = (max(1, t) - 1) * (d + 1)
    if packing == 0:
        return extra + sum((d + 1) ** (j + 1) for j in range(k))
    if packing != 1 or k > 2:
        raise ValueError(f"no packing {packing} for k = {k}")
    D = d + 1
    return extra + (D if k == 1 else D + D * (D + 1) // 2)


def new_survey_id() -> str:
    return str(uuid.uuid4())


def clone(sq: SurveyQuery) -> SurveyQuery:
    return copy.deepcopy(sq)
