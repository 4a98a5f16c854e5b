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
from dataclasses import dataclass, field

from .. import kmeans as km
from ..crypto import elgamal as eg
from ..ops import encoding as enc
from ..query import (KMeansParameters, LogisticRegressionParameters, Operation, Query, QueryDiffP, QueryDPDataGen,
                     QueryIVSigs, Roster, SurveyQuery, check_parameters, iter_operation, iter_rounds, new_survey_id,
                     sql_cells, sql_plan)
from ..utils import timers


@dataclass
class KMeansResult:
    """What ``DrynxClient.send_kmeans`` returns.  ``centroids``: the final K * d
    scaled coordinates (the update of the last round run), ``points`` the same
    as K lists of d Fractions in record units.  ``assigned``: the centroids the
    last round assigned by, which ``counts`` [K], ``sums`` [K][d] (of offsets
    x - QueryMin), ``sq_sums`` [K] and ``sse`` (a Fraction, record units) refer
    to.  ``converged_at``: the first round whose update changed nothing, None
    when every update moved a centroid.  ``rounds``: the rounds' SurveyResults."""
    centroids: list
    points: list
    assigned: list
    counts: list
    sums: list
    sq_sums: list
    sse: object
    converged_at: object = None
    rounds: list = field(default_factory=list)


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
    def iterative_round_query(self, sq: SurveyQuery, base: int, k: int, prefix, iter_id: str) -> SurveyQuery:
        """Round ``k`` of the iterative search ``iter_id`` as a survey of its own
        (``prefix``: the digits found so far, or for a survey with SQL the list of
        them, one per cell, which travels as IterPrefixes):
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
        if sq.Query.SQL:
            prefix, rq.IterPrefixes = 0, [int(p) for p in (prefix if isinstance(prefix, (list, tuple)) else [prefix])]
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

    @staticmethod
    def _iter_cells(sq: SurveyQuery):
        """The searches one walk over ``sq`` carries: None without SQL (one, its
        prefix travels as IterPrefix), with SQL the cells G of its plan (their
        prefixes travel as IterPrefixes; 1 with WHERE only)."""
        plan = sql_plan(sq.Query)
        return None if plan is None else sql_cells(plan)

    def _iterative_walk(self, sq: SurveyQuery, base: int, what: str, decoder, rule, on_round):
        """The rounds of one iterative search over ``sq``, or with SQL of the G
        searches of its cells side by side: round k's query carries the k
        digits found so far for every search (a list of prefixes, of length 1
        without SQL), ``decoder`` turns its aggregate into ``client_out`` (one
        entry per group) and ``rule(k, prefixes, client_out)`` into ``(digits,
        failed, empty)``: the round's digit of every search, a message when
        the answers contradict an earlier round or each other, or that there
        is nothing to search.  One ``run_survey`` per round, L rounds for every
        cell.  Returns ``(prefixes, empty, rounds, iter_id)``; raises the first
        failure.  ``on_round`` gets the digit without SQL, the list with."""
        op = sq.Query.Operation
        L = iter_rounds(op.QueryMin, op.QueryMax, base)
        iter_id = sq.SurveyID or new_survey_id()
        collective = getattr(getattr(self.entry, "comm", None), "world", 1) > 1
        cells = self._iter_cells(sq)
        n = 1 if cells is None else cells
        # With several ranks the others serve exactly L rounds (``serve_iterative``):
        # a search that has failed, or found nothing to search, still runs them all.
        prefixes, rounds, failed, empty = [0] * n, [], None, False
        for k in range(L):
            rq = self.iterative_round_query(sq, base, k, prefixes[0] if cells is None else prefixes, iter_id)
            if k == 0 and not check_parameters(rq, False):
                raise ValueError("the iterative query fails CheckParameters")
            res = self.entry.run_survey(rq, on_result=decoder)
            rounds.append(res)
            digits = [0] * n
            if failed is None and not empty:
                digits, failed, empty = rule(k, prefixes, res.client_out)
            if (failed is not None or empty) and not collective:
                break
            if on_round is not None:
                on_round(k, digits[0] if cells is None else list(digits), res)
            prefixes = [p * base + d for p, d in zip(prefixes, digits)]
        if failed is not None:
            raise RuntimeError(f"iterative {what} {iter_id}: {failed}")
        return prefixes, empty, rounds, iter_id

    @staticmethod
    def _cell_outs(k: int, cells: int, outs: list):
        """``(one decoded entry per cell, failure)`` of a round's ``client_out``:
        with GROUP BY the ciphertext groups are the cells; with WHERE only
        the one cell's answer is replicated over the groups of GroupByValues,
        which must agree."""
        if cells == 1:
            if any(x != outs[0] for x in outs):
                return None, f"round {k}: the groups disagree on the one cell's answer"
            return outs[:1], None
        if len(outs) != cells:
            return None, f"round {k}: {len(outs)} groups answered for {cells} cells"
        return outs, None

    def send_iterative_extreme(self, sq: SurveyQuery, base: int, on_round=None):
        """Iterative min/max (extension): the result of the ``min``/``max`` survey
        ``sq`` found one base-``base`` digit per round, most significant first,
        instead of one output per value of the domain.  Every round is an
        ordinary verifiable query with ``base`` unary outputs (its own survey
        id, proofs and block); round k's query carries the k digits found so
        far in clear.  Returns ``(value, rounds)``: the decoded extreme and
        every round's SurveyResult.  ``on_round(k, digit, result)`` is called
        after each round.  Raises when the DPs' answers contradict an earlier
        round (a ``min`` round nobody matches) or the groups disagree.

        A survey with SQL: one search per cell of its WHERE / GROUP BY, all in
        the same L rounds (``SurveyQuery.IterPrefixes``).  Returns ``([value per
        cell], rounds)``, a list of one with WHERE only; a cell without records
        decodes to QueryMin, as the one-shot SQL ``min`` / ``max`` decode it.
        Raises "round k, cell g: ... an answer changed between rounds" when a
        ``min`` cell's answers contradict an earlier round; ``on_round`` gets the
        list of the cells' digits."""
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

        def rule(k, prefixes, ds):
            digit, failed = ds[0], None
            if any(d != digit for d in ds):
                failed = f"round {k}: the groups disagree on the digit ({ds})"
            elif digit is None and is_max:
                failed = f"round {k}: no zero aggregate (the last output of a max round is always zero)"
            elif digit is None and k > 0:
                failed = f"round {k}: no DP matches the prefix {prefixes[0]}: an answer changed between rounds"
            # min, round 0, no digit: no DP has records -> QueryMin, as the one-shot decode returns
            return [digit or 0], failed, digit is None and failed is None

        cells = self._iter_cells(sq)
        vacant = set()  # min: the cells without a record in round 0

        def cell_rule(k, prefixes, ds):
            ds, failed = self._cell_outs(k, cells, ds)
            if failed is not None:
                return [0] * cells, failed, False
            for g, d in enumerate(ds):
                if is_max:
                    if d is None:
                        failed = f"round {k}, cell {g}: no zero aggregate (the last output of a max round is zero)"
                elif k == 0:
                    if d is None:  # no record in the cell -> QueryMin, as the one-shot decode returns
                        vacant.add(g)
                elif d is None and g not in vacant:
                    failed = (f"round {k}, cell {g}: no DP matches the prefix {prefixes[g]}: an answer changed "
                              "between rounds")
                elif d is not None and g in vacant:
                    failed = (f"round {k}, cell {g}: a record in a cell that had none in round 0: an answer changed "
                              "between rounds")
                if failed is not None:
                    break
            return [d or 0 for d in ds], failed, False

        prefixes, empty, rounds, _ = self._iterative_walk(sq, base, op.NameOp, digits,
                                                          rule if cells is None else cell_rule, on_round)
        if cells is not None:
            return [float(op.QueryMin + p) for p in prefixes], rounds
        return float(op.QueryMin + (0 if empty else prefixes[0])), rounds

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
        round before, the groups disagree, or no DP has a record in the domain.

        A survey with SQL (``SELECT median(x) ... WHERE ... GROUP BY ...``): one
        search per cell, all in the same L rounds; every cell has its own rank
        from its own round-0 total and its own consistency check ("round k,
        cell g: ... an answer changed between rounds").  Returns ``([value per
        cell], rounds)``, a list of one with WHERE only.  A cell without records
        in round 0 yields NaN (what the logistic-regression cohorts return for
        an empty cell); it keeps prefix 0 and must total 0 in every later
        round.  Empty cells do not raise; ``on_round`` gets the list of digits."""
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

        def step(c, t):
            """``(digit, the rank left inside it)``: the smallest digit whose cumulative count reaches t."""
            below = 0
            for digit, x in enumerate(c):
                if below + x >= t:
                    break
                below += x
            return digit, t - below

        t, chosen = 0, 0  # the rank still to walk, the count of the bin chosen in the round before

        def rule(k, prefixes, cs):
            nonlocal t, chosen
            c = cs[0]
            total = sum(c)
            if any(x != c for x in cs):
                return [0], f"round {k}: the groups disagree on the counts", False
            if k == 0 and total == 0:
                return [0], None, True
            if k == 0:
                t = max(1, (num * total + den - 1) // den)
            elif total != chosen:
                return [0], (f"round {k}: {total} records under the prefix {prefixes[0]}, round {k - 1} counted "
                             f"{chosen}: an answer changed between rounds"), False
            digit, t = step(c, t)
            chosen = c[digit]
            return [digit], None, False

        cells = self._iter_cells(sq)
        ts, chosens = [0] * (cells or 0), [0] * (cells or 0)  # per cell; a cell empty in round 0 keeps (0, 0)

        def cell_rule(k, prefixes, cs):
            cs, failed = self._cell_outs(k, cells, cs)
            if failed is not None:
                return [0] * cells, failed, False
            digits = [0] * cells
            for g, c in enumerate(cs):
                total = sum(c)
                if k == 0:
                    ts[g] = max(1, (num * total + den - 1) // den) if total else 0
                elif total != chosens[g]:
                    return digits, (f"round {k}, cell {g}: {total} records under the prefix {prefixes[g]}, round "
                                    f"{k - 1} counted {chosens[g]}: an answer changed between rounds"), False
                if ts[g]:
                    digits[g], ts[g] = step(c, ts[g])
                    chosens[g] = c[digits[g]]
            return digits, None, False

        prefixes, empty, rounds, iter_id = self._iterative_walk(sq, base, "quantile", counts,
                                                                rule if cells is None else cell_rule, on_round)
        if cells is not None:
            return [float(op.QueryMin + p) if ts[g] else float("nan") for g, p in enumerate(prefixes)], rounds
        if empty:
            raise RuntimeError(f"iterative quantile {iter_id}: no records in the domain")
        return float(op.QueryMin + prefixes[0]), rounds

    # ------------------------------------------------------------------ k-means
    def kmeans_round_query(self, sq: SurveyQuery, r: int, centroids, search_id: str) -> SurveyQuery:
        """Round ``r`` of the k-means run ``search_id`` as a survey of its own: a
        copy of the ``kmeans`` survey ``sq`` whose ``Operation.KMeans`` carries the
        round and the centroids it assigns by, with the survey's ranges and
        input-validation signatures (the same objects every round, so the
        provers' and verifiers' tables built for round 0 serve the others) and
        a survey id derived from ``search_id``."""
        op = sq.Query.Operation
        if op.NameOp != "kmeans" or op.KMeans is None:
            raise ValueError(f"a k-means run needs a kmeans survey, not {op.NameOp}")
        rq = copy.copy(sq)
        rq.Query = copy.copy(sq.Query)
        rq.Query.Operation = copy.copy(op)
        p = op.KMeans
        rq.Query.Operation.KMeans = KMeansParameters(K=p.K, Scale=p.Scale, Round=int(r), Rounds=p.Rounds,
                                                     Centroids=[int(c) for c in centroids], SearchID=search_id)
        rq.SurveyID = f"{search_id}.r{r}"  # no '/': ledger buckets and proof keys are '<survey id>/<kind>/...'
        return rq

    def send_kmeans(self, sq: SurveyQuery, centroids, on_round=None, stop_when_converged=False) -> KMeansResult:
        """K-means clustering (extension) of the records the ``kmeans`` survey
        ``sq`` reads (``make_kmeans_survey``), from the K * d scaled start
        ``centroids``: ``KMeans.Rounds`` Lloyd rounds, every one an ordinary
        verifiable query (its own survey id, proofs and block) whose K * (d +
        2) outputs are the per-cluster counts, coordinate sums and sums of
        squares under the centroids the round carries in clear; the querier
        moves the centroids with ``kmeans.update`` (exact, half up; an empty
        cluster stays).  ``on_round(r, answer, result)`` is called after each
        round with the decrypted aggregate.  Exactly ``Rounds`` rounds run,
        unless ``stop_when_converged`` ends the run after the first round whose
        update changed nothing -- with a single rank only: the other ranks of a
        ``comm`` serve a fixed count (``serve_kmeans``).  Replicated groups
        (``GroupByValues``) must agree.  Returns a ``KMeansResult``."""
        op = sq.Query.Operation
        if op.NameOp != "kmeans" or op.KMeans is None:
            raise ValueError(f"a k-means run needs a kmeans survey, not {op.NameOp}")
        p, d = op.KMeans, op.NbrInput
        cur = [int(c) for c in centroids]
        km.check(p.K, d, op.QueryMin, op.QueryMax, p.Scale, cur)
        km.check_rounds(p.Rounds)
        collective = getattr(getattr(self.entry, "comm", None), "world", 1) > 1
        if stop_when_converged and collective:
            raise ValueError("stop_when_converged with several ranks: the other ranks serve exactly Rounds rounds")
        search_id = sq.SurveyID or new_survey_id()

        def answers(partial):
            """Per group the round's aggregate, decrypted as integers."""
            with timers.timed("Decode"):
                return [[int(v) for v in eg.decrypt_auto(self.keypair.secret, cv.to(self.device),
                                                         self.decrypt_bound).cpu().tolist()]
                        for cv in partial.groups()]

        rounds, failed, converged_at, answer, assigned = [], None, None, None, cur
        for r in range(p.Rounds):
            rq = self.kmeans_round_query(sq, r, cur, search_id)
            if r == 0 and not check_parameters(rq, False):
                raise ValueError("the k-means query fails CheckParameters")
            res = self.entry.run_survey(rq, on_result=answers)
            rounds.append(res)
            if failed is None:
                outs = res.client_out
                if not outs or any(x != outs[0] for x in outs):
                    failed = f"round {r}: the groups disagree on the clusters' sums"
                else:
                    answer, assigned = outs[0], cur
                    cur = km.update(assigned, answer, p.K, d, p.Scale)
                    if cur == assigned and converged_at is None:
                        converged_at = r
                    if on_round is not None:
                        on_round(r, answer, res)
            # With several ranks the others serve exactly Rounds rounds: a failed run still runs them all.
            if failed is not None and not collective:
                break
            if stop_when_converged and converged_at is not None:
                break
        if failed is not None:
            raise RuntimeError(f"k-means {search_id}: {failed}")
        counts, sums, sq_sums = km.split(answer, p.K, d)
        return KMeansResult(cur, km.points(cur, p.K, d, op.QueryMin, p.Scale), assigned, counts, sums, sq_sums,
                            km.sse(answer, p.K, d), converged_at, rounds)

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


def serve_kmeans(node) -> list:
    """A rank without the querier serves one k-means run: one
    ``run_survey(None)`` per round, the number of rounds read from the first
    round's query.  Returns the rounds' SurveyResults."""
    res = node.run_survey(None)
    op = node.surveys[res.survey_id].Query.Operation
    if op.NameOp != "kmeans" or op.KMeans is None:
        raise RuntimeError(f"survey {res.survey_id} is not a round of a k-means query")
    return [res] + [node.run_survey(None) for _ in range(op.KMeans.Rounds - 1)]


def lr_parameters(**kw) -> LogisticRegressionParameters:
    return LogisticRegressionParameters(**kw)
