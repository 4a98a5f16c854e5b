"""Privacy-preserving logistic regression (the reference's flagship "model").

Reference: lib/encoding/logistic_regression.go.
  * DP side (EncodeLogisticRegression[WithProofs], :46-215): standardise with
    global (or local) mean/std, augment with a column of ones, compute the
    polynomial-approximation coefficients of the log-loss per record
    (level 1: x*(2y-1); level j>=2: ypart * x^{(x)j}, ypart = y - y(-1)^j - 1),
    sum over records, scale by PrecisionApproxCoefficients, round to int64 and
    encrypt.  Packing: level j at offset sum_{i<j}(d+1)^(i+1) (== the
    reference's j*(d+1)^j for k<=2, :96-111).
  * Querier side (DecodeLogisticRegression :217, FindMinimumWeights :693):
    decrypt, unpack, rescale, gradient descent on the approximated loss with
    the exact reference Cost (including its level-accumulation quirk, :526)
    and Gradient (:564) — here vectorised O((d+1)^2) instead of re-enumerating
    cartesian products each iteration.

MI355X design: the per-record coefficient sums are one tall-skinny fp64
GEMM  X^T diag(w) X  over N records (K13) — the HIP MFMA kernels
``lr_encode`` / ``lr_moments`` in csrc/kernels/dx_lr.hip (v_mfma_f64_16x16x4f64,
a grid of up to 3x3-tile output blocks, so any number of features: the
reference's 100-feature BC and GSE datasets included) when the DP's records
live on a GPU; the CPU path uses torch float64 matmul.
"""
from __future__ import annotations

import math
import time

import torch

from .. import native as nt
from ..crypto import elgamal as eg
from ..query import LogisticRegressionParameters, lr_nbr_outputs
from ..utils import timers
from ..utils.log import get_logger

log = get_logger("logreg")

TAYLOR_COEFFICIENTS = [-math.log(2), -0.5, -0.125, 0, 0.0052]
MIN_AREA_COEFFICIENTS = [-0.714761, -0.5, -0.0976419]
POLY_APPROX_COEFFICIENTS = MIN_AREA_COEFFICIENTS
NUM_DPS = 10


# ----------------------------------------------------------------------------- data utilities
def standardise_with(X: torch.Tensor, means, sds) -> torch.Tensor:
    m = torch.as_tensor(means, dtype=torch.float64, device=X.device)
    s = torch.as_tensor(sds, dtype=torch.float64, device=X.device)
    return (X - m) / s


def compute_means_sds(X: torch.Tensor):
    """population mean / std per column (montanaflynn/stats StandardDeviation)."""
    return X.mean(0), X.std(0, unbiased=False)


def standardise(X: torch.Tensor) -> torch.Tensor:
    m, s = compute_means_sds(X)
    return (X - m) / s


def standardise_with_train(X_test: torch.Tensor, X_train: torch.Tensor) -> torch.Tensor:
    """StandardiseWithTrain (logistic_regression.go:943-965): the test matrix
    standardised with the TRAINING matrix's column means and (population)
    standard deviations."""
    m, s = compute_means_sds(X_train.to(torch.float64))
    return (X_test.to(torch.float64) - m) / s


def normalize(X: torch.Tensor) -> torch.Tensor:
    """Normalize (:985): column-wise min-max scaling with the matrix's own range."""
    return normalize_with(X, X)


def normalize_with(X_test: torch.Tensor, X_train: torch.Tensor) -> torch.Tensor:
    """NormalizeWith (:990-1012): the test matrix min-max scaled with the
    training matrix's column minima and maxima."""
    tr = X_train.to(torch.float64)
    mn, mx = tr.min(0).values, tr.max(0).values
    return (X_test.to(torch.float64) - mn) / (mx - mn)


def partition_dataset(X: torch.Tensor, y: torch.Tensor, ratio: float, shuffle: bool = False, seed: int = 0):
    """PartitionDataset (:1389-1420): the first int(n * ratio) records (after an
    optional seeded shuffle) for training, the rest for testing.  -> (X_train,
    y_train, X_test, y_test).  The shuffle order comes from numpy's seeded
    generator, not Go's math/rand (parity of the order itself is unpinned; the
    split sizes and the no-shuffle split are the reference's)."""
    import numpy as np

    n = X.shape[0]
    n_train = int(float(n) * ratio)
    idx = np.arange(n)
    if shuffle:
        idx = np.random.RandomState(seed).permutation(n)
    tr = torch.as_tensor(idx[:n_train], dtype=torch.long, device=X.device)
    te = torch.as_tensor(idx[n_train:], dtype=torch.long, device=X.device)
    return X.index_select(0, tr), y.index_select(0, tr.to(y.device)), X.index_select(0, te), \
        y.index_select(0, te.to(y.device))


def augment(X: torch.Tensor) -> torch.Tensor:
    return torch.cat([torch.ones((X.shape[0], 1), dtype=X.dtype, device=X.device), X], dim=1)


def n_coeffs(d: int, k: int, packing: int = 0, targets: int = 1) -> int:
    """Values a DP sends: cartesian sum_j (d+1)^(j+1), or with distinct packing
    (1, k <= 2) D + D(D+1)/2 with D = d + 1; with T > 1 targets (k <= 2) T
    level-1 vectors and one level 2."""
    return lr_nbr_outputs(d, k, packing, targets)


def n_targets(params) -> int:
    """Label columns of a query: NbrTargets 0 and 1 are the single-label query."""
    return max(1, int(getattr(params, "NbrTargets", 0) or 0))


def _label_columns(y: torch.Tensor, T: int) -> list:
    """The T label columns of ``y`` ([N] or [N, 1] for T = 1, [N, T] beyond)."""
    if y.dim() == 1 and T == 1:
        return [y]
    if y.dim() != 2 or y.shape[1] != T:
        raise ValueError(f"labels of shape {tuple(y.shape)} for a query with {T} target(s)")
    return [y[:, t] for t in range(T)]


# ----------------------------------------------------------------------------- distinct-coefficient packing
# Query extension (LogisticRegressionParameters.Packing = 1, K <= 2): level 2,
# the symmetric matrix sum_i w_i xa_i xa_i^T, travels as its row-major upper
# triangle (0,0),(0,1),..,(0,d),(1,1),..,(d,d).  The values are the cartesian
# ones at those positions (ComputeAllApproxCoefficients semantics, weight
# ypart_2), NOT the reference's ComputeDistinctApproxCoefficients, which
# carries the level-1 sign into level 2 (``distinct_approx_coefficients``).
def packed_index(i: int, j: int, D: int) -> int:
    """Position of entry (i, j), i <= j, in the packed level 2."""
    assert 0 <= i <= j < D
    return i * D - i * (i - 1) // 2 + (j - i)


_triu_memo: dict = {}


def _triu_flat(D: int) -> torch.Tensor:
    """Flat cartesian positions i * D + j of the packed level-2 entries, in packed order."""
    t = _triu_memo.get(D)
    if t is None:
        iu = torch.triu_indices(D, D)  # row-major: (0,0),(0,1),..,(0,D-1),(1,1),..
        t = _triu_memo[D] = iu[0] * D + iu[1]
    return t


def pack(vals, d: int, k: int):
    """Cartesian vector [level 1, level 2 (D*D)] -> the distinct layout (a
    tensor for a tensor, a list otherwise)."""
    D = d + 1
    if k == 1:
        return vals
    if k != 2:
        raise ValueError("distinct packing is defined for K <= 2 only")
    idx = _triu_flat(D)
    n1 = (vals.shape[-1] if isinstance(vals, torch.Tensor) else len(vals)) - D * D  # T*D level-1 values
    if isinstance(vals, torch.Tensor):
        return torch.cat([vals[..., :n1], vals[..., n1:].index_select(-1, idx.to(vals.device))], -1)
    vals = list(vals)
    return vals[:n1] + [vals[n1 + e] for e in idx.tolist()]


# ----------------------------------------------------------------------------- approximation coefficients
def approx_coefficients(Xa: torch.Tensor, y: torch.Tensor, k: int) -> list:
    """Aggregated (summed over records) approximation coefficients per level.

    Xa: [N, d+1] standardised+augmented float64; y: [N] in {0,1}.
    Level 1: sum_i (2y_i-1) x_i ; level j: sum_i ypart_j(y_i) * x_i^{(x)j}
    flattened in cartesian (row-major) order.
    y: [N, T], T > 1 (k <= 2): level 1 is the T single-label vectors
    concatenated (each computed as for y[:, t] alone, so the values are the
    single-label ones), level 2 the one matrix they share (weight -1)."""
    if y.dim() == 2:
        cols = _label_columns(y, y.shape[1])
        if len(cols) > 1 and k > 2:
            raise ValueError("several targets share level 2 only: K <= 2")
        per = [approx_coefficients(Xa, c, k) for c in cols[:1]]
        per += [approx_coefficients(Xa, c, 1) for c in cols[1:]]
        return [torch.cat([lv[0] for lv in per])] + per[0][1:]
    y = y.to(torch.float64)
    out = [Xa.T @ (2 * y - 1)]
    for j in range(2, k + 1):
        ypart = y - y * ((-1.0) ** j) - 1.0
        if j == 2:
            out.append(lr_moment_gemm(Xa, ypart).reshape(-1))
        elif j == 3:
            out.append(torch.einsum("n,na,nb,nc->abc", ypart, Xa, Xa, Xa).reshape(-1))
        else:
            raise NotImplementedError("k > 3 is not supported (the reference packing is only valid for k <= 2)")
    return out


def distinct_approx_coefficients(x, y: int, k: int) -> list:
    """ComputeDistinctApproxCoefficients (lib/encoding/logistic_regression.go:
    322-363) for ONE (augmented) record: level j holds the products over the
    multisets i_1 <= ... <= i_j of the record's entries, in lexicographic
    order, times the level's sign -- (2y - 1) for level 1, then the previous
    level's sign times ypart = y - y (-1)^(j+1) - 1.  The cartesian layout of
    ``approx_coefficients`` is the same values with every ordering repeated."""
    import itertools

    xs = [float(v) for v in x]
    sign = 2.0 * float(y) - 1.0
    out = []
    for j in range(1, k + 1):
        if j > 1:
            sign *= float(y) - float(y) * (-1.0) ** j - 1.0
        lvl = []
        for combo in itertools.combinations_with_replacement(range(len(xs)), j):
            prod = 1.0
            for i in combo:
                prod *= xs[i]
            lvl.append(prod * sign + 0.0)  # + 0.0: no negative zeros
        out.append(lvl)
    return out


def lr_moment_gemm(Xa: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """sum_i w_i x_i x_i^T (K13).  On GPU: the native fp64-MFMA kernel."""
    if Xa.is_cuda:
        return nt.lr_moments(Xa.contiguous(), w.contiguous())
    return (Xa * w[:, None]).T @ Xa


def round_precision(v: torch.Tensor, precision: float) -> torch.Tensor:
    """int64(math.Round(x * precision)) — Go rounds half away from zero."""
    x = v * precision
    return (torch.sign(x) * torch.floor(torch.abs(x) + 0.5)).to(torch.int64)


def _standardisation(params: LogisticRegressionParameters, X: torch.Tensor):
    """(means, sds): the query's global ones, or without them the records' own."""
    if params.Means and params.StandardDeviations:
        return params.Means, params.StandardDeviations
    return compute_means_sds(X)


def _gpu_coefficients_int(Xs: list, ys: list, params: LogisticRegressionParameters, Ks=None, plan=None):
    """``encode_coefficients_int`` of a batch of DPs on the fused fp64-MFMA
    encoder (K <= 2) -> [n, n_coeffs] int64; with the DPs' key tables ``Ks`` and
    a SQL ``plan``, per cell -> [n, G, n_coeffs].  Xs: float64 records on one
    GPU with unit column stride, ys: ``_label_matrix``.  A single DP is a batch
    of one: the batch reducers give a DP the same bits alone or batched.
    Level-2 weight: ypart = y - y*(-1)^2 - 1 = 0*y - 1."""
    T = n_targets(params)
    D = Xs[0].shape[1] + 1
    m, s = _standardisation(params, Xs[0])
    precision = params.PrecisionApproxCoefficients
    if plan is not None:
        keys, filters, predicate = _cohort_terms(params, plan)
    if params.Packing == 1:
        # distinct layout: the upper launch plan, then one reduce + pack + round launch
        packed = nt.lr_encode_packed_many(Xs, ys, m, s, 0.0, -1.0, precision) if plan is None else \
            nt.lr_encode_cells_packed_many(Xs, ys, Ks, m, s, -1.0, keys, filters, precision,
                                           predicate=predicate)
        return packed[..., :T * D] if params.K == 1 else packed
    tot = nt.lr_encode_many(Xs, ys, m, s, 0.0, -1.0) if plan is None else \
        nt.lr_encode_cells_many(Xs, ys, Ks, m, s, -1.0, keys, filters, predicate=predicate)
    lv = tot[..., D:D + T, :D].flatten(-2)  # target-major level 1
    if params.K == 2:
        lv = torch.cat([lv, tot[..., :D, :D].flatten(-2)], -1)
    return round_precision(lv, precision)


def encode_coefficients_int_many(Xs: list, ys: list, params: LogisticRegressionParameters):
    """``encode_coefficients_int`` of several DPs' records as one fused batch
    (one encoder launch per DP, one reduction, one rounding pass: the same
    values as DP by DP) -> [n_dp, n_coeffs] int64, or None when the batch
    does not fit the fused GPU encoder (the caller then encodes per DP)."""
    if not Xs or params.K > 2 or not (params.Means and params.StandardDeviations):
        return None
    d = Xs[0].shape[1] if Xs[0] is not None and Xs[0].dim() == 2 else -1
    if d < 1 or any(X is None or not X.is_cuda or X.dim() != 2 or X.shape[1] != d or len(X) == 0 for X in Xs):
        return None
    ys = [_label_matrix(y, n_targets(params)) for y in ys]
    Xs = [X.to(torch.float64) for X in Xs]
    return _gpu_coefficients_int(Xs if params.Packing == 1 else [X.contiguous() for X in Xs], ys, params)


# ----------------------------------------------------------------------------- cohorts (SQL WHERE / GROUP BY)
def cell_ids(K: torch.Tensor, plan) -> tuple:
    """The cell of every record under a query's SQL plan, from the DP's key
    table K [N, >= plan.width] int64 -> ([N] int64, G): the ``row_group`` rule
    of the grouped moments in torch.  A record failing the WHERE (a Where
    equality, or ``plan.predicate`` over the terms' atoms) or with a GroupBy
    value outside [0, V_i) gets G (dropped); otherwise the mixed-radix
    number of its GroupBy values, first column most significant
    (``all_possible_groups`` order); without GroupBy the one cell 0."""
    keep = torch.ones(K.shape[0], dtype=torch.bool, device=K.device)
    if plan.predicate is None:
        for col, val in plan.where:
            keep &= K[:, col] == val
    else:
        ops, table = plan.predicate
        cmp = {"==": torch.eq, "!=": torch.ne, "<": torch.lt, "<=": torch.le, ">": torch.gt, ">=": torch.ge}
        idx = torch.zeros(K.shape[0], dtype=torch.int64, device=K.device)
        for i, ((col, val), op) in enumerate(zip(plan.where, ops)):
            idx |= cmp[op](K[:, col], val).to(torch.int64) << i
        bits = torch.tensor([table >> i & 1 for i in range(1 << len(ops))], dtype=torch.bool, device=K.device)
        keep = bits[idx]
    key = torch.zeros(K.shape[0], dtype=torch.int64, device=K.device)
    G = 1
    for col, card in plan.group_by:
        v = K[:, col]
        keep &= (v >= 0) & (v < card)
        key = key * card + v
        G *= card
    return torch.where(keep, key, torch.full_like(key, G)), G


def _cohort_terms(params, plan):
    """(keys, filters, predicate) of the native grouped ops for a SQL plan, after the cohort rules."""
    if params.K != 2 or not (params.Means and params.StandardDeviations):
        raise ValueError("logistic regression over SQL cohorts needs K = 2 and global Means and StandardDeviations")
    return [(c, 0, v) for c, v in plan.group_by], list(plan.where), plan.predicate


def _key_table(K, n: int, plan, device) -> torch.Tensor:
    if K is None:
        raise ValueError("records without a key table for a query with SQL")
    K = torch.as_tensor(K, device=device)
    if K.dim() != 2 or K.dtype != torch.int64 or K.shape[0] != n:
        raise ValueError(f"key table of shape {tuple(K.shape)} ({K.dtype}) for {n} records: [N, width] int64")
    if K.shape[1] < plan.width:
        raise ValueError(f"key table has {K.shape[1]} columns, the SQL query reads {plan.width}")
    return K if K.shape[1] <= 1 or K.stride(1) == 1 else K.contiguous()


def encode_coefficients_int_cells_many(Xs: list, ys: list, Ks: list, params: LogisticRegressionParameters, plan):
    """``encode_coefficients_int`` per cell of the query's WHERE / GROUP BY, for
    several DPs -> [n_dp, G, n_coeffs] int64 (G = the product of the GroupBy
    cardinalities, 1 without GroupBy).  ``Ks[i]`` [N_i, width] int64 is DP i's
    key table, row r the key columns of record r of (Xs[i], ys[i]); cell
    membership is ``cell_ids``.  Standardisation is the query's global Means /
    StandardDeviations, K = 2; an empty cell (and a DP without records) is all
    zeros.  Records on a GPU: the grouped fp64-MFMA encoder
    (``native.lr_encode_cells_many`` / ``..._packed_many``), one batch for the
    DPs.  Host: ``cell_ids``, then ``approx_coefficients`` on each cell's
    records -- the model the kernels are tested against."""
    _cohort_terms(params, plan)  # the cohort rules
    T = n_targets(params)
    d = params.NbrFeatures
    D = d + 1
    n_out = n_coeffs(d, 2, params.Packing, params.NbrTargets)
    G = 1
    for _, v in plan.group_by:
        G *= v
    live = [i for i, X in enumerate(Xs) if X is not None and len(X) > 0]
    dev = Xs[live[0]].device if live else torch.device("cpu")
    out = torch.zeros((len(Xs), G, n_out), dtype=torch.int64, device=dev)
    if not live:
        return out
    lX = [Xs[i].to(torch.float64) for i in live]
    lX = [X if X.dim() != 2 or X.stride(1) == 1 else X.contiguous() for X in lX]
    ly = [_label_matrix(torch.as_tensor(ys[i], device=dev), T) for i in live]
    lK = [_key_table(Ks[i], lX[j].shape[0], plan, dev) for j, i in enumerate(live)]
    if any(X.dim() != 2 or X.shape[1] != d for X in lX):
        raise ValueError(f"records of another width than the query's {d} features")
    if dev.type == "cuda":
        out[torch.as_tensor(live, device=dev)] = _gpu_coefficients_int(lX, ly, params, lK, plan)
        return out
    for X, y, K, i in zip(lX, ly, lK, live):
        ids, _ = cell_ids(K, plan)
        for c in ids.unique().tolist():
            if c < G:
                rows = (ids == c).nonzero().reshape(-1)
                out[i, c] = encode_coefficients_int(X.index_select(0, rows), y.index_select(0, rows), params)
    return out


def encode_coefficients_int_cells(X: torch.Tensor, y: torch.Tensor, K: torch.Tensor,
                                  params: LogisticRegressionParameters, plan) -> torch.Tensor:
    """One DP's ``encode_coefficients_int_cells_many`` -> [G, n_coeffs] int64."""
    return encode_coefficients_int_cells_many([X], [y], [K], params, plan)[0]


def _label_matrix(y: torch.Tensor, T: int) -> torch.Tensor:
    """Labels as the fused encoder takes them: [N] for one target, [N, T] for several."""
    if T == 1:
        return _label_columns(y, 1)[0]
    _label_columns(y, T)  # shape check
    return y


def encode_coefficients_int(X: torch.Tensor, y: torch.Tensor, params: LogisticRegressionParameters) -> torch.Tensor:
    """The packed int64 vector the DP encrypts (before encryption)."""
    X = X.to(torch.float64)
    T = n_targets(params)
    if T > 1 and params.K > 2:
        raise ValueError("several targets share level 2 only: K <= 2")
    y = _label_matrix(y, T)
    if params.Packing == 1:
        return _encode_coefficients_int_packed(X, y, params)
    if X.is_cuda and params.K <= 2:
        return _gpu_coefficients_int([X.contiguous()], [y], params)[0]
    levels = approx_coefficients(augment(standardise_with(X, *_standardisation(params, X))), y, params.K)
    return torch.cat([round_precision(lv, params.PrecisionApproxCoefficients) for lv in levels])


def _encode_coefficients_int_packed(X: torch.Tensor, y: torch.Tensor, params) -> torch.Tensor:
    """``encode_coefficients_int`` in the distinct layout (Packing = 1)."""
    if params.K > 2:
        raise ValueError("distinct packing is defined for K <= 2 only")
    if X.is_cuda:
        return _gpu_coefficients_int([X], [y], params)[0]
    # host: the cartesian levels as for Packing = 0, then the upper triangle
    levels = approx_coefficients(augment(standardise_with(X, *_standardisation(params, X))), y, params.K)
    cart = torch.cat([round_precision(lv, params.PrecisionApproxCoefficients) for lv in levels])
    return pack(cart, X.shape[1], params.K)


def encode_logistic_regression(X, y, params: LogisticRegressionParameters, pk: eg.PublicKeyTable,
                               with_proofs: bool = False, ranges=None):
    from ..ops.encoding import _encrypt_with_proofs

    d = params.NbrFeatures
    n = n_coeffs(d, params.K, params.Packing, params.NbrTargets)
    if X is None or len(X) == 0:
        vals = [0] * n
    else:
        vals = encode_coefficients_int(torch.as_tensor(X, device=pk.device), torch.as_tensor(y, device=pk.device),
                                       params).cpu().tolist()
        assert len(vals) == n, (len(vals), n)
    return _encrypt_with_proofs(pk, vals, with_proofs, ranges)


# ----------------------------------------------------------------------------- querier: gradient descent
def mirror_upper(upper: torch.Tensor, D: int) -> torch.Tensor:
    """The D(D+1)/2 packed level-2 values -> the flattened symmetric [D, D] matrix."""
    assert upper.numel() == D * (D + 1) // 2, (upper.numel(), D)
    iu = torch.triu_indices(D, D)
    A2 = torch.zeros((D, D), dtype=upper.dtype)
    A2[iu[0], iu[1]] = upper
    return (A2 + torch.triu(A2, 1).T).reshape(-1)


def unpack(vals, d: int, k: int, packing: int = 0, targets: int = 1) -> list:
    """Per-level float64 tensors in the cartesian layout.  ``packing`` 1: the
    D(D+1)/2 distinct level-2 values are mirrored into the symmetric [D, D]
    matrix (on the host), so the descent below is the same for both layouts.
    ``targets`` T > 1 (k <= 2): [the T level-1 vectors as one [T, D] tensor]
    and, for k = 2, the one level-2 matrix they share."""
    if targets > 1:
        if k > 2:
            raise ValueError("several targets share level 2 only: K <= 2")
        D = d + 1
        vals = list(vals)
        shared = unpack(vals[(targets - 1) * D:], d, k, packing)  # the last target's level 1, then level 2
        return [torch.tensor(vals[:targets * D], dtype=torch.float64).reshape(targets, D)] + shared[1:]
    if packing == 1:
        if k > 2:
            raise ValueError("distinct packing is defined for K <= 2 only")
        D = d + 1
        out = [torch.tensor(vals[:D], dtype=torch.float64)]
        if k == 2:
            out.append(mirror_upper(torch.tensor(vals[D: D + D * (D + 1) // 2], dtype=torch.float64), D))
        return out
    if packing != 0:
        raise ValueError(f"unknown packing {packing}")
    out, off = [], 0
    for j in range(k):
        m = (d + 1) ** (j + 1)
        out.append(torch.tensor(vals[off: off + m], dtype=torch.float64))
        off += m
    return out


def cost(weights: torch.Tensor, approx: list, N: int, lam: float) -> float:
    """logistic_regression.go:526 Cost, replicated exactly (the running sum is
    multiplied by each level's polynomial coefficient in turn)."""
    k = len(approx)
    d = approx[0].numel() - 1
    c = 0.0
    w = weights
    outer = w
    for j in range(k):
        if j == 0:
            term = float((w * approx[0]).sum())
        else:
            outer = torch.einsum("...a,b->...ab", outer, w) if j >= 1 else w
            term = float((outer.reshape(-1) * approx[j]).sum())
        c += term
        c *= POLY_APPROX_COEFFICIENTS[j + 1]
    c = c / N - POLY_APPROX_COEFFICIENTS[0]
    reg = float((weights[1:d + 1] ** 2).sum())
    return c + (lam / (2 * N)) * reg


def gradient(weights: torch.Tensor, approx: list, N: int, lam: float) -> torch.Tensor:
    """logistic_regression.go:564 Gradient, closed form for k <= 3."""
    k = len(approx)
    d1 = approx[0].numel()
    g = POLY_APPROX_COEFFICIENTS[1] * approx[0].clone()
    if k >= 2:
        A2 = approx[1].reshape(d1, d1)
        g += POLY_APPROX_COEFFICIENTS[2] * ((A2 + A2.T) @ weights)
    if k >= 3:
        A3 = approx[2].reshape(d1, d1, d1)
        S = A3 + A3.permute(1, 0, 2) + A3.permute(1, 2, 0)
        g += POLY_APPROX_COEFFICIENTS[3] * torch.einsum("iab,a,b->i", S, weights, weights)
    g = g / N
    reg = (lam / N) * weights
    reg[0] = 0.0
    return g + reg


def find_minimum_weights(approx: list, initial_weights, N: int, lam: float, step: float, max_iter: int,
                         timeout_s: float = 180.0) -> list:
    """logistic_regression.go:693 FindMinimumWeights (k == 1 -> closed form :680)."""
    k = len(approx)
    if k == 1:
        return [float(-POLY_APPROX_COEFFICIENTS[1] * a / lam) for a in approx[0].tolist()]
    if k == 2:
        return _find_minimum_weights_k2(approx, initial_weights, N, lam, step, max_iter, timeout_s)
    w = torch.tensor(list(initial_weights), dtype=torch.float64)
    min_w = w.clone()
    t0 = time.time()
    for it in range(max_iter):
        c = cost(w, approx, N, lam)
        if c >= 0.0:
            min_w = w.clone()
        w = w - step * gradient(w, approx, N, lam)
        if time.time() - t0 > timeout_s - 2.0:
            break
    return min_w.tolist()


def _find_minimum_weights_k2(approx, initial_weights, N, lam, step, max_iter, timeout_s):
    """k = 2 fast path of FindMinimumWeights: Cost and Gradient reduce to one
    (d+1)x(d+1) mat-vec per iteration with S = A2 + A2^T (w^T A2 w = w^T S w / 2),
    in float64 on the host in native code (``dx_lr_gd_k2``: no GIL held, ~10x
    the numpy loop); same iteration, same quirky Cost accumulation and
    min-weights rule."""
    import numpy as np

    from .. import native as nt

    C0, C1, C2 = POLY_APPROX_COEFFICIENTS[0], POLY_APPROX_COEFFICIENTS[1], POLY_APPROX_COEFFICIENTS[2]
    a0 = approx[0].cpu().numpy().astype(np.float64)
    d1 = a0.shape[0]
    A2 = approx[1].cpu().numpy().astype(np.float64).reshape(d1, d1)
    S = A2 + A2.T
    w0 = np.asarray(list(initial_weights), dtype=np.float64)
    return nt.lr_gd_k2(a0, S, w0, N, lam, step, max_iter, (C0, C1, C2))


def find_minimum_weights_with_encryption(encrypted: list, secret: int, initial_weights, N: int, lam: float,
                                         step: float, max_iter: int, precision: float, packing: int = 0):
    """FindMinimumWeightsWithEncryption (:746-766): the client decrypts the
    encrypted approximation coefficients (one CipherVector per level, with
    negatives), rescales them by ``precision`` and runs FindMinimumWeights.
    ``packing`` 1: level 2 arrives as its D(D+1)/2 distinct values and is
    mirrored first.  -> (weights, approx coefficients as lists of floats,
    cartesian layout)."""
    approx = []
    for lvl, cv in enumerate(encrypted):
        vals = eg.decrypt_auto(secret, cv).cpu().to(torch.float64)
        if packing == 1 and lvl == 1:
            vals = mirror_upper(vals, approx[0].numel())
        elif packing not in (0, 1) or (packing == 1 and lvl > 1):
            raise ValueError(f"no packing {packing} for level {lvl + 1}")
        approx.append(vals / precision)
    w = find_minimum_weights(approx, initial_weights, N, lam, step, max_iter)
    return w, [a.tolist() for a in approx]


def cohort_records(vals, params: LogisticRegressionParameters) -> int:
    """Records behind the aggregate of one SQL cell: level 2's entry (0, 0) is
    sum (-1) * 1 * 1 = -n, the first level-2 value in both layouts, so
    n = round(-v / PrecisionApproxCoefficients)."""
    if params.K < 2:
        raise ValueError("K = 1 carries no record count")
    v = float(vals[n_targets(params) * (params.NbrFeatures + 1)])
    return int(round(-v / params.PrecisionApproxCoefficients))


def decode_logistic_regression_values(vals, params: LogisticRegressionParameters, cohort: bool = False) -> list:
    """The weights of the decrypted aggregate ``vals``.  ``cohort``: the
    aggregate of one cell of a query with SQL: the descent runs with the
    cell's own record count (``cohort_records``) in place of NbrRecords, and an
    empty cell decodes to NaN weights, as the other operations answer for an
    empty group."""
    with timers.timed("GradientDescent", sync=False):
        approx = [a / params.PrecisionApproxCoefficients
                  for a in unpack(vals, params.NbrFeatures, params.K, params.Packing, n_targets(params))]
        D = params.NbrFeatures + 1
        init = list(params.InitialWeights or [0.0] * D)
        T = n_targets(params)
        n_rec = params.NbrRecords
        if cohort:
            n_rec = cohort_records(vals, params)
            if n_rec == 0:
                return [float("nan")] * (T * D)
        if T == 1:
            return find_minimum_weights(approx, init, n_rec, params.Lambda, params.Step, params.MaxIterations)
        # one descent per target against the shared level 2; the weights target-major in one flat list
        if len(init) not in (D, T * D):
            raise ValueError(f"{len(init)} initial weights for {T} targets of {D} weights")
        out = []
        for t in range(T):
            w0 = init if len(init) == D else init[t * D:(t + 1) * D]
            out += list(find_minimum_weights([approx[0][t]] + approx[1:], w0, n_rec, params.Lambda, params.Step,
                                             params.MaxIterations))
        return out


# ----------------------------------------------------------------------------- prediction & metrics
def predict(X: torch.Tensor, weights, means=None, sds=None) -> torch.Tensor:
    X = X.to(torch.float64)
    if means is not None and sds is not None:
        X = standardise_with(X, means, sds)
    Xa = augment(X)
    w = torch.as_tensor(weights, dtype=torch.float64, device=X.device)
    return torch.sigmoid(Xa @ w)


def split_targets(weights, T: int) -> list:
    """The flat target-major weight list of a T-target query -> T lists of d + 1 weights."""
    w = list(weights)
    T = max(1, int(T))
    if len(w) % T:
        raise ValueError(f"{len(w)} weights do not split into {T} targets")
    D = len(w) // T
    return [w[t * D:(t + 1) * D] for t in range(T)]


def predict_targets(X: torch.Tensor, weights, T: int, means=None, sds=None) -> torch.Tensor:
    """[n, T] probabilities: column t is ``predict`` with target t's weights."""
    return torch.stack([predict(X, w, means, sds) for w in split_targets(weights, T)], dim=1)


def predict_class(X: torch.Tensor, weights, T: int, means=None, sds=None) -> torch.Tensor:
    """One-vs-rest: the target with the largest probability per record -> [n] int64."""
    return predict_targets(X, weights, T, means, sds).argmax(dim=1)


def predict_in_clear(x, weights) -> float:
    """PredictInClear (:808-817): sigmoid(w0 + sum_i w_{i+1} x_i) for one record."""
    s_ = sum(float(w) * float(v) for w, v in zip(list(weights)[1:], x))
    return 1.0 / (1.0 + math.exp(-float(weights[0]) - s_))


def predict_encrypted(encrypted_data: eg.CipherVector, weights, secret: int, precision_weights: float,
                      precision_data: float) -> float:
    """Predict (:820-852) for ONE encrypted record (Enc(round(x_i *
    precision_data)) per feature): the weighted sum with integer weights
    round(w_{i+1} * precision_weights) is evaluated homomorphically (the
    reference adds the ciphertext |w| times; here one scalar multiplication
    per feature, negatives as r - |w|, and one K5 reduction), decrypted with
    negatives, rescaled, and the sigmoid taken with the clear bias w0."""
    from ..crypto import bn254 as bn

    wi = [int(round_precision(torch.tensor([float(w)], dtype=torch.float64), precision_weights)[0])
          for w in list(weights)[1:]]
    n = len(encrypted_data)
    if n != len(wi):
        raise ValueError(f"{n} encrypted features for {len(wi)} weights")
    dev = encrypted_data.device
    sc = bn.scalars_tensor([w % bn.R for w in wi], dev)
    prod = encrypted_data.mul_scalars(sc)
    tot = eg.CipherVector(nt.g1_sum(prod.K.view(n, 1, 24)), nt.g1_sum(prod.C.view(n, 1, 24)))
    bound = sum(abs(w) for w in wi) * int(precision_data * 1e3 + 1) + 1
    dot = int(eg.decrypt_auto(secret, tot, bound=min(bound, 1 << 20)).cpu()[0])
    val = dot / (precision_weights * precision_data)
    return 1.0 / (1.0 + math.exp(-float(weights[0]) - val))


def logistic_regression_cost(weights, X: torch.Tensor, y: torch.Tensor, N: int, lam: float) -> float:
    """LogisticRegressionCost (:769-794) on clear data, including the
    reference's regulariser precedence (lambda / 2 * N, not lambda / (2N);
    a test-only helper)."""
    w = torch.as_tensor(weights, dtype=torch.float64)
    s1 = X.to(torch.float64) @ w
    cost = float((torch.log1p(torch.exp(s1)) - y.to(torch.float64) * s1).sum())
    return cost + float((w * w).sum()) * (lam / 2 * float(N))


def logistic_regression_gradient(weights, X: torch.Tensor, y: torch.Tensor, N: int, lam: float) -> list:
    """LogisticRegressionGradient (:797-817) on clear data."""
    w = torch.as_tensor(weights, dtype=torch.float64)
    X = X.to(torch.float64)
    g = X.T @ (torch.sigmoid(X @ w) - y.to(torch.float64)) + (lam / float(N)) * w
    return g.tolist()


def predict_homomorphic(X: torch.Tensor, weights, pk: eg.PublicKeyTable, secret: int, precision: float = 1e2):
    """Score encrypted features (logistic_regression.go PredictHomomorphic): the
    linear term is evaluated homomorphically on Enc(round(x*precision)) with
    integer weights round(w*precision), decrypted, then the sigmoid applied."""
    from ..crypto import bn254 as bn

    Xa = augment(X.to(torch.float64))
    xi = round_precision(Xa.reshape(-1), precision)
    cv, _ = eg.encrypt_ints(pk, xi)
    wi = round_precision(torch.as_tensor(weights, dtype=torch.float64), precision)
    N, d1 = Xa.shape
    ws = [int(v) for v in wi.repeat(N).tolist()]
    sc = bn.scalars_tensor([v % bn.R for v in ws], pk.device)
    prod = cv.mul_scalars(sc)
    K = nt.g1_sum(prod.K.view(N, d1, 24).transpose(0, 1).contiguous())
    C = nt.g1_sum(prod.C.view(N, d1, 24).transpose(0, 1).contiguous())
    bound = int(abs(xi).max()) * int(abs(wi).max() + 1) * d1 + 1
    dots = eg.DecryptionTable(bound, pk.device).decrypt(secret, eg.CipherVector(K, C))
    return torch.sigmoid(dots.to(torch.float64) / (precision * precision))


def metrics(pred: torch.Tensor, y: torch.Tensor, threshold: float = 0.5) -> dict:
    """Accuracy / precision / recall / F-score / AUC (logistic_regression.go:1103-1164)."""
    y = y.to(torch.float64)
    yhat = (pred >= threshold).to(torch.float64)
    tp = float(((yhat == 1) & (y == 1)).sum())
    tn = float(((yhat == 0) & (y == 0)).sum())
    fp = float(((yhat == 1) & (y == 0)).sum())
    fn = float(((yhat == 0) & (y == 1)).sum())
    n = max(1.0, float(y.numel()))
    precision = tp / (tp + fp) if tp + fp else 0.0
    recall = tp / (tp + fn) if tp + fn else 0.0
    f = 2 * precision * recall / (precision + recall) if precision + recall else 0.0
    # AUC via the rank statistic
    order = torch.argsort(pred)
    ranks = torch.empty_like(pred)
    ranks[order] = torch.arange(1, pred.numel() + 1, dtype=pred.dtype, device=pred.device)
    npos, nneg = float((y == 1).sum()), float((y == 0).sum())
    auc = (float(ranks[y == 1].sum()) - npos * (npos + 1) / 2) / (npos * nneg) if npos and nneg else 0.0
    return {"accuracy": (tp + tn) / n, "precision": precision, "recall": recall, "fscore": f, "auc": auc}


def partition_for_dp(X: torch.Tensor, y: torch.Tensor, dp_index: int, n_dps: int = NUM_DPS):
    """Deterministic per-DP split (the reference slices by a character of the
    DP's ServerIdentity string, logistic_regression.go:1427-1448; here by index)."""
    n = X.shape[0]
    per = n // n_dps
    s = dp_index * per
    e = n if dp_index == n_dps - 1 else s + per
    return X[s:e], y[s:e]


def load_csv_dataset(path: str, label_col: int = 0, drop_cols=(), targets: int = 1):
    """Dataset loader: CSV with the label in column 0 (logistic_regression.go GetDataForDataProvider).
    ``targets`` T > 1: ``label_0,..,label_{T-1},f1,..,fd`` per line -> (X [n, d], y [n, T])."""
    import numpy as np

    if targets > 1:
        data = np.loadtxt(path, delimiter=",", ndmin=2)
        if label_col != 0 or data.shape[1] <= targets:
            raise ValueError(f"{path}: {targets} label columns lead each record, then the features")
        keep = [c for c in range(targets, data.shape[1]) if c not in drop_cols]
        return torch.tensor(data[:, keep], dtype=torch.float64), torch.tensor(data[:, :targets], dtype=torch.int64)
    data = np.loadtxt(path, delimiter=",")
    keep = [c for c in range(data.shape[1]) if c != label_col and c not in drop_cols]
    X = torch.tensor(data[:, keep], dtype=torch.float64)
    y = torch.tensor(data[:, label_col], dtype=torch.int64)
    return X, y
