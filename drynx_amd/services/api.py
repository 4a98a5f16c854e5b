"""Querier/client API.

Reference: services/api.go (``NewDrynxClient`` :39 — keypair + decryption
table of 10000 entries; ``GenerateSurveyQuery`` :58-102; ``SendSurveyQuery``
:105-133) and services/api_skipchain.go (``SendSurveyQueryToVNs`` :16,
``SendEndVerification`` :30, ``SendGetLatestBlock`` :44, ``SendGetGenesis``
:61, ``SendGetBlock`` :71, ``SendGetProofs`` :86, ``SendCloseDB`` :98).

The client talks to an entry point: an in-process ``DrynxNode`` (rank 0 of a
local cluster) or a ``RemoteNode`` (TCP control plane to a running server,
see services/server.py).
"""
from __future__ import annotations

import copy

from ..crypto import elgamal as eg
from ..ops import encoding as enc
from ..query import (LogisticRegressionParameters, Operation, Query, QueryDiffP, QueryDPDataGen, QueryIVSigs, Roster,
                     SurveyQuery, check_parameters, iter_operation, iter_rounds, new_survey_id)
from ..utils import timers


class DrynxClient:
    def __init__(self, entry_point, keypair: eg.KeyPair | None = None, decrypt_bound: int = 10000, device="cpu"):
        self.entry = entry_point
        self.keypair = keypair or eg.KeyPair.generate()
        self.public = self.keypair.public
        self.device = device
        self.decrypt_bound = decrypt_bound
        self._table = None
        self.last_plaintexts: list = []  # the decrypted aggregate of the last logistic-regression query, per group

    @property
    def table(self) -> eg.DecryptionTable:
        """CreateDecryptionTable(limit) — built lazily on the client's device."""
        if self._table is None or self._table.bound != self.decrypt_bound:
            self._table = eg.decryption_table(self.decrypt_bound, self.device)
        return self._table

    # ------------------------------------------------------------------ query building
    def generate_survey_query(self, roster_servers: Roster, roster_vns: Roster | None, dp_to_server: dict,
                              id_to_public: dict, survey_id: str | None, operation: Operation, ranges, ps,
                              proofs: int, obfuscation: bool, thresholds, diffp: QueryDiffP | None = None,
                              dpdatagen: QueryDPDataGen | None = None, cutting_factor: int = 0,
                              verification_sharding: int = 0, range_proof_mode: int = 0) -> SurveyQuery:
        """GenerateSurveyQuery; thresholds = [general, aggregation, range, obfuscation, keyswitch] (api.go:79-83)."""
        sq = SurveyQuery(
            SurveyID=survey_id or new_survey_id(),
            RosterServers=roster_servers,
            ClientPubKey=self.public,
            IntraMessage=False,
            ServerToDP=dp_to_server,
            Query=Query(Operation=operation, Ranges=ranges, Proofs=proofs, Obfuscation=obfuscation,
                        DiffP=diffp or QueryDiffP(), DPDataGen=dpdatagen or QueryDPDataGen(),
                        IVSigs=QueryIVSigs(InputValidationSigs=ps,
                                           InputValidationSize1=len(ps) if ps else 0,
                                           InputValidationSize2=len(ps[0]) if ps else 0),
                        RosterVNs=roster_vns, CuttingFactor=cutting_factor),
            IDtoPublic=id_to_public,
            Threshold=thresholds[0], AggregationProofThreshold=thresholds[1], RangeProofThreshold=thresholds[2],
            ObfuscationProofThreshold=thresholds[3], KeySwitchingProofThreshold=thresholds[4],
            VerificationSharding=verification_sharding,
            RangeProofMode=range_proof_mode,
        )
        return sq

    # ------------------------------------------------------------------ execution
    def send_survey_query(self, sq: SurveyQuery):
        """SendSurveyQuery: run the survey, decode every group.  Returns
        (group keys, list of decoded float vectors, SurveyResult).  The key of
        group g is ``str(g)``; with a SQL GROUP BY it is the group's column
        values as the reference prints them (fmt.Sprint of a slice, "[0 1]"),
        in ``all_possible_groups`` order."""
        op = sq.Query.Operation
        keys = None
        if sq.Query.SQL.GroupBy:
            from ..protocols.data_collection import all_possible_groups

            keys = ["[" + " ".join(str(v) for v in g) + "]"
                    for g in all_possible_groups(sq.Query.DPDataGen.GroupByValues)]

        def decode_all(partial):
            groups, values = [], []
            self.last_plaintexts = []
            with timers.timed("Decode"):
                for g, cv in enumerate(partial.groups()):
                    groups.append(keys[g] if keys is not None else str(g))
                    values.append(self.decode(cv.to(self.device), op, cohort=bool(sq.Query.SQL)))
            return groups, values

        # decoding overlaps the VNs' proof verification (own thread + stream)
        res = self.entry.run_survey(sq, on_result=decode_all)
        groups, values = res.client_out
        return groups, values, res

    def decode(self, cv: eg.CipherVector, op: Operation, cohort: bool = False):
        """``cohort``: the aggregate of one cell of a query with SQL (a logistic
        regression then descends with the cell's own record count)."""
        if op.NameOp == "logistic regression":
            with timers.timed("Decryption"):
                vals = [int(v) for v in eg.decrypt_auto(self.keypair.secret, cv, self.decrypt_bound).cpu().tolist()]
            self.last_plaintexts.append(vals)
            from ..models.logistic_regression import decode_logistic_regression_values

            return decode_logistic_regression_values(vals, op.LRParameters, cohort)
        return enc.decode(cv, self.keypair.secret, op, self.table)

    # ------------------------------------------------------------------ iterative min / max
    def iterative_round_query(self, sq: SurveyQuery, base: int, k: int, prefix: int, iter_id: str) -> SurveyQuery:
        """Round ``k`` of the iterative search ``iter_id`` as a survey of its own:
        a copy of ``sq`` (a ``min``/``max``/``frequencyCount`` survey over the full
        domain) with ``base`` outputs, the first ``base`` columns of its ranges and
        input-validation signatures (the same objects every round, so the
        provers' and verifiers' tables built for round 0 serve the others) and
        a survey id derived from ``iter_id``."""
        op = sq.Query.Operation
        rq = copy.copy(sq)
        rq.Query = copy.copy(sq.Query)
        rq.Query.Operation = iter_operation(op.NameOp, op.QueryMin, op.QueryMax, base)
        q = rq.Query
        if q.Ranges is not None:
            if len(q.Ranges) < base:
                raise ValueError(f"{len(q.Ranges)} ranges for {base} outputs per round")
            q.Ranges = self._iter_columns(sq.Query.Ranges, base)
        sigs = q.IVSigs.InputValidationSigs
        if sigs is not None:
            if any(len(row) < base for row in sigs):
                raise ValueError(f"input-validation signatures for fewer than {base} outputs per round")
            cut = self._iter_columns(sigs, base, per_cn=True)
            q.IVSigs = QueryIVSigs(InputValidationSigs=cut, InputValidationSize1=len(cut), InputValidationSize2=base)
        rq.IterBase, rq.IterRound, rq.IterPrefix, rq.IterSurveyID = int(base), int(k), int(prefix), iter_id
        rq.SurveyID = f"{iter_id}.r{k}"  # no '/': ledger buckets and proof keys are '<survey id>/<kind>/...'
        return rq

    def _iter_columns(self, cols, base: int, per_cn: bool = False):
        """The first ``base`` columns of a survey's ranges or signature rows, cut
        once per search (memoised on the source object: the digest cache of
        the signature broadcast keys on the list's identity)."""
        if (all(len(row) == base for row in cols) if per_cn else len(cols) == base):
            return cols
        memo = getattr(self, "_iter_memo", None)
        if memo is None:
            memo = self._iter_memo = {}
        hit = memo.get((id(cols), base))
        if hit is not None and hit[0] is cols:
            return hit[1]
        cut = [row[:base] for row in cols] if per_cn else [list(r) for r in cols[:base]]
        if len(memo) > 8:
            memo.clear()
        memo[(id(cols), base)] = (cols, cut)
        return cut

    def _iterative_walk(self, sq: SurveyQuery, base: int, what: str, decoder, rule, on_round):
        """The rounds of one iterative search over ``sq``: round k's query carries
        the k digits found so far, ``decoder`` turns its aggregate into
        ``client_out`` (one entry per group) and ``rule(k, prefix, client_out)``
        into ``(digit, failed, empty)``: the round's digit, a message when the
        answers contradict an earlier round or each other, or that there is
        nothing to search.  Returns ``(prefix, empty, rounds, iter_id)``;
        raises the first failure."""
        op = sq.Query.Operation
        L = iter_rounds(op.QueryMin, op.QueryMax, base)
        iter_id = sq.SurveyID or new_survey_id()
        collective = getattr(getattr(self.entry, "comm", None), "world", 1) > 1
        # With several ranks the others serve exactly L rounds (``serve_iterative``):
        # a search that has failed, or found nothing to search, still runs them all.
        prefix, rounds, failed, empty = 0, [], None, False
        for k in range(L):
            rq = self.iterative_round_query(sq, base, k, prefix, iter_id)
            if k == 0 and not check_parameters(rq, False):
                raise ValueError("the iterative query fails CheckParameters")
            res = self.entry.run_survey(rq, on_result=decoder)
            rounds.append(res)
            digit = 0
            if failed is None and not empty:
                digit, failed, empty = rule(k, prefix, res.client_out)
            if (failed is not None or empty) and not collective:
                break
            if on_round is not None:
                on_round(k, digit, res)
            prefix = prefix * base + digit
        if failed is not None:
            raise RuntimeError(f"iterative {what} {iter_id}: {failed}")
        return prefix, empty, rounds, iter_id

    def send_iterative_extreme(self, sq: SurveyQuery, base: int, on_round=None):
        """Iterative min/max (extension): the result of the ``min``/``max`` survey
        ``sq`` found one base-``base`` digit per round, most significant first,
        instead of one output per value of the domain.  Every round is an
        ordinary verifiable query with ``base`` unary outputs (its own survey
        id, proofs and block); round k's query carries the k digits found so
        far in clear.  Returns ``(value, rounds)``: the decoded extreme and
        every round's SurveyResult.  ``on_round(k, digit, result)`` is called
        after each round.  Raises when the DPs' answers contradict an earlier
        round (a ``min`` round nobody matches) or the groups disagree."""
        op = sq.Query.Operation
        is_max = op.NameOp == "max"

        def digits(partial):
            """Per group the first zero (max) / non-zero (min) aggregate of the round, None without one."""
            out = []
            with timers.timed("Decode"):
                for cv in partial.groups():
                    nz = eg.decrypt_check_zero(self.keypair.secret, cv.to(self.device)).cpu().tolist()
                    out.append(next((i for i, b in enumerate(nz) if (b == 0) == is_max), None))
            return out

        def rule(k, prefix, ds):
            digit, failed = ds[0], None
            if any(d != digit for d in ds):
                failed = f"round {k}: the groups disagree on the digit ({ds})"
            elif digit is None and is_max:
                failed = f"round {k}: no zero aggregate (the last output of a max round is always zero)"
            elif digit is None and k > 0:
                failed = f"round {k}: no DP matches the prefix {prefix}: an answer changed between rounds"
            # min, round 0, no digit: no DP has records -> QueryMin, as the one-shot decode returns
            return digit or 0, failed, digit is None and failed is None

        prefix, empty, rounds, _ = self._iterative_walk(sq, base, op.NameOp, digits, rule, on_round)
        return float(op.QueryMin + (0 if empty else prefix)), rounds

    # ------------------------------------------------------------------ iterative quantiles
    def send_iterative_quantile(self, sq: SurveyQuery, base: int, num: int, den: int, on_round=None):
        """Iterative quantile (extension): the ``num/den`` nearest-rank quantile of
        the records the ``frequencyCount`` survey ``sq`` counts, found one
        base-``base`` digit per round, most significant first.  Every round is
        an ordinary verifiable query whose ``base`` outputs are the counts of
        that digit among the records under the prefix found so far (its own
        survey id, proofs and block).  Round 0 gives the number N of records in
        the domain and the target rank t = max(1, ceil(num * N / den)): 0/1 is
        the minimum, 1/1 the maximum, 1/2 the lower median.  Each round takes
        the first digit whose cumulative count reaches t and carries the rest
        of the rank into the chosen bin.  Returns ``(value, rounds)``: the
        quantile and every round's SurveyResult (``client_out`` = the counts
        per group).  ``on_round(k, digit, result)`` is called after each round.
        Raises when a round's total is not the count of the bin chosen in the
        round before, the groups disagree, or no DP has a record in the domain."""
        num, den = int(num), int(den)
        if den < 1 or not 0 <= num <= den:
            raise ValueError(f"no quantile {num}/{den}")
        op = sq.Query.Operation
        if op.NameOp != "frequencyCount":
            raise ValueError(f"an iterative quantile runs on a frequencyCount survey, not {op.NameOp}")
        round_op = iter_operation(op.NameOp, op.QueryMin, op.QueryMax, base)

        def counts(partial):
            """Per group the round's aggregate counts, decoded as the one-shot frequencyCount's."""
            with timers.timed("Decode"):
                return [[int(round(v)) for v in self.decode(cv.to(self.device), round_op)] for cv in partial.groups()]

        t, chosen = 0, 0  # the rank still to walk, the count of the bin chosen in the round before

        def rule(k, prefix, cs):
            nonlocal t, chosen
            c = cs[0]
            total = sum(c)
            if any(x != c for x in cs):
                return 0, f"round {k}: the groups disagree on the counts", False
            if k == 0 and total == 0:
                return 0, None, True
            if k == 0:
                t = max(1, (num * total + den - 1) // den)
            elif total != chosen:
                return 0, (f"round {k}: {total} records under the prefix {prefix}, round {k - 1} counted "
                           f"{chosen}: an answer changed between rounds"), False
            below = 0
            for digit, x in enumerate(c):  # the smallest digit whose cumulative count reaches t
                if below + x >= t:
                    break
                below += x
            t -= below
            chosen = c[digit]
            return digit, None, False

        prefix, empty, rounds, iter_id = self._iterative_walk(sq, base, "quantile", counts, rule, on_round)
        if empty:
            raise RuntimeError(f"iterative quantile {iter_id}: no records in the domain")
        return float(op.QueryMin + prefix), rounds

    # ------------------------------------------------------------------ VN / skipchain calls
    def send_survey_query_to_vns(self, sq: SurveyQuery):
        """SendSurveyQueryToVNs (api_skipchain.go:16): announce the survey to the
        VNs before running it (expected proof counts, ledger, chain)."""
        return self.entry.register_vn_survey(sq)

    def send_end_verification(self, vn_id: str, survey_id: str, timeout: float | None = 3600.0):
        """SendEndVerification (api_skipchain.go:30): blocks until the VNs have
        verified every proof of the survey and the root VN appended its block
        (EndVerificationChannel, service_skipchain.go:158-166); returns it, or
        None on timeout.  Callable before or while the survey runs."""
        return self.entry.wait_end_verification(survey_id, timeout)

    def send_get_latest_block(self, vn_id: str, sb=None):
        """SendGetLatestBlock (api_skipchain.go:44): the VN's head, or -- given a
        known block ``sb`` -- the end of the verified update chain from it."""
        return self.entry.get_latest_block(vn_id, sb) if sb is not None else self.entry.get_latest_block(vn_id)

    def send_get_genesis(self, vn_id: str):
        return self.entry.get_genesis(vn_id)

    def send_get_block(self, vn_id: str, survey_id: str):
        return self.entry.get_block(vn_id, survey_id)

    def send_get_proofs(self, vn_id: str, survey_id: str) -> dict:
        return self.entry.get_proofs(vn_id, survey_id)

    def send_close_db(self, vn_id: str, remove: bool = False):
        return self.entry.close_db(vn_id, remove)


def serve_iterative(node) -> list:
    """A rank without the querier serves one iterative search (min/max digits or
    the count rounds of a quantile): one
    ``run_survey(None)`` per round, the number of rounds derived from the
    first round's query.  Returns the rounds' SurveyResults."""
    res = node.run_survey(None)
    sq = node.surveys[res.survey_id]
    if not sq.IterBase:
        raise RuntimeError(f"survey {res.survey_id} is not a round of an iterative query")
    op = sq.Query.Operation
    L = iter_rounds(op.QueryMin, op.QueryMax, sq.IterBase)
    return [res] + [node.run_survey(None) for _ in range(L - 1)]


def lr_parameters(**kw) -> LogisticRegressionParameters:
    return LogisticRegressionParameters(**kw)
