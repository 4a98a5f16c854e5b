"""The arithmetic of a k-means query: one Lloyd round at a DP, the querier's update.

A k-means query clusters records of ``d`` integer columns over the domain
[QueryMin, QueryMax] (R = QueryMax - QueryMin + 1 values per column) into ``k``
clusters in ``Rounds`` rounds, every round an ordinary verifiable survey.  A
record's coordinates are the offsets o_j = x_j - QueryMin.  ``S >= 1`` is the
query's Scale: centroids travel as integers c[c][j] in units of 1/S, the point
is QueryMin + c[c][j] / S, and 0 <= c[c][j] <= (R - 1) * S.

One round, at every DP (``round_model``; csrc/kernels/dx_kmeans.hip computes
the same numbers and checks the same limits below the binding):

* a row with any of its d coordinates outside [QueryMin, QueryMax] is DROPPED
  (the frequencyCount rule);
* a kept row is assigned to the cluster with the smallest
  D(c) = sum_j (S * o_j - c[c][j])^2, ties to the lowest cluster index;
* the answer is k * (d + 2) non-negative integers, cluster-major:
  [n_c, s_c0 .. s_c(d-1), q_c] with n_c the rows assigned, s_cj = sum o_j and
  q_c = sum over the rows of sum_j o_j^2.  (The encoders add in int64 modulo
  2^64, like every moment here; the ranges of a query with proofs bound what a
  DP may answer.)

The querier sums the DPs' answers and moves the centroids (``update``):
c'[c][j] = floor((2 * S * s_cj + n_c) / (2 * n_c)), the mean in units of 1/S
rounded half up; a cluster without rows keeps its centroid.  ``sse`` is the
within-cluster sum of squared distances to the clusters' exact means, in
record units.

No torch, no native import.
"""
from __future__ import annotations

import hashlib
from fractions import Fraction

KMEANS_MAX_DIMS = 32
KMEANS_MAX_CLUSTERS = 512
KMEANS_MAX_CELLS = 3072  # k * (d + 2): one 64-bit LDS accumulator per output (csrc/kernels/dx_kmeans.hip kMaxCells)
KMEANS_MAX_COORD = 1 << 31  # (R - 1) * S stays below: a difference fits 32 bits
KMEANS_MAX_DIST = 1 << 63  # d * ((R - 1) * S)^2 stays below: a distance never wraps
KMEANS_MAX_ROUNDS = 64


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def max_clusters(d: int) -> int:
    """The largest k the limits allow for ``d`` columns."""
    return min(KMEANS_MAX_CLUSTERS, KMEANS_MAX_CELLS // (int(d) + 2))


def check(k, d, qmin, qmax, scale, centroids=None) -> None:
    """Raises ValueError naming the violated rule of a k-means query: the
    limits above, and for ``centroids`` (None: not checked) their number k * d
    and their bounds."""
    if not all(_is_int(v) for v in (k, d, qmin, qmax, scale)):
        raise ValueError("k-means: k, d, the domain and the scale are integers")
    if not 1 <= d <= KMEANS_MAX_DIMS:
        raise ValueError(f"k-means: {d} columns outside 1..{KMEANS_MAX_DIMS}")
    if not 1 <= k <= KMEANS_MAX_CLUSTERS:
        raise ValueError(f"k-means: {k} clusters outside 1..{KMEANS_MAX_CLUSTERS}")
    if k * (d + 2) > KMEANS_MAX_CELLS:
        raise ValueError(f"k-means: {k} clusters of {d} columns are {k * (d + 2)} outputs (at most "
                         f"{KMEANS_MAX_CELLS})")
    if scale < 1:
        raise ValueError(f"k-means: scale {scale} below 1")
    if qmax < qmin:
        raise ValueError(f"k-means: an empty domain [{qmin}, {qmax}]")
    if qmin < -(1 << 63) or qmax >= 1 << 63:
        raise ValueError(f"k-means: the domain [{qmin}, {qmax}] is not one of int64 records")
    top = (qmax - qmin) * scale
    if top >= KMEANS_MAX_COORD:
        raise ValueError(f"k-means: (R - 1) * scale = {top} does not stay below 2^31")
    if d * top * top >= KMEANS_MAX_DIST:
        raise ValueError(f"k-means: d * ((R - 1) * scale)^2 = {d * top * top} does not stay below 2^63")
    if centroids is None:
        return
    if not isinstance(centroids, (list, tuple)) or len(centroids) != k * d:
        n = len(centroids) if isinstance(centroids, (list, tuple)) else "no list of"
        raise ValueError(f"k-means: {n} centroid coordinates for {k} clusters of {d} columns")
    if any(not _is_int(c) or not 0 <= c <= top for c in centroids):
        raise ValueError(f"k-means: a centroid coordinate outside 0..(R - 1) * scale = {top}")


def check_rounds(rounds, rnd=0) -> None:
    """Raises ValueError unless 1 <= rounds <= 64 and 0 <= rnd < rounds."""
    if not _is_int(rounds) or not 1 <= rounds <= KMEANS_MAX_ROUNDS:
        raise ValueError(f"k-means: {rounds} rounds outside 1..{KMEANS_MAX_ROUNDS}")
    if not _is_int(rnd) or not 0 <= rnd < rounds:
        raise ValueError(f"k-means: round {rnd} outside 0..{rounds - 1}")


def assign(offsets, k: int, d: int, scale: int, centroids) -> int:
    """The cluster of a kept row with the offsets ``offsets``: the smallest D, the lowest index among equals."""
    best, best_d = 0, None
    for c in range(k):
        dist = sum((scale * offsets[j] - centroids[c * d + j]) ** 2 for j in range(d))
        if best_d is None or dist < best_d:
            best, best_d = c, dist
    return best


def round_model(rows, k: int, d: int, qmin: int, qmax: int, scale: int, centroids) -> list:
    """The golden model of one DP's answer: ``rows`` are its records (the first
    ``d`` values of each are read) -> the k * (d + 2) integers of the round."""
    check(k, d, qmin, qmax, scale, list(centroids))
    out = [0] * (k * (d + 2))
    for row in rows:
        x = [int(v) for v in row[:d]]
        if len(x) != d:
            raise ValueError(f"k-means: a record of {len(x)} values, the query reads {d}")
        if any(v < qmin or v > qmax for v in x):
            continue
        o = [v - qmin for v in x]
        at = assign(o, k, d, scale, centroids) * (d + 2)
        out[at] += 1
        for j in range(d):
            out[at + 1 + j] += o[j]
            out[at + 1 + d] += o[j] * o[j]
    return out


def split(answer, k: int, d: int) -> tuple:
    """``(counts [k], sums [k][d], sq_sums [k])`` of an answer of k * (d + 2) integers."""
    if len(answer) != k * (d + 2):
        raise ValueError(f"k-means: an answer of {len(answer)} values for {k} clusters of {d} columns")
    a = [int(v) for v in answer]
    W = d + 2
    return [a[c * W] for c in range(k)], [a[c * W + 1: c * W + 1 + d] for c in range(k)], \
        [a[c * W + 1 + d] for c in range(k)]


def update(centroids, answer, k: int, d: int, scale: int) -> list:
    """The next centroids from the summed answers of a round: the clusters'
    means in units of 1 / scale, rounded half up; an empty cluster keeps its
    centroid.  Exact integer arithmetic."""
    counts, sums, _ = split(answer, k, d)
    out = [int(c) for c in centroids]
    for c in range(k):
        n = counts[c]
        if n > 0:
            for j in range(d):
                out[c * d + j] = (2 * scale * sums[c][j] + n) // (2 * n)
    return out


def sse(answer, k: int, d: int) -> Fraction:
    """The within-cluster sum of squared distances to the clusters' exact means,
    in record units: sum over the non-empty clusters of q_c - |s_c|^2 / n_c."""
    counts, sums, sqs = split(answer, k, d)
    total = Fraction(0)
    for c in range(k):
        if counts[c] > 0:
            total += sqs[c] - Fraction(sum(s * s for s in sums[c]), counts[c])
    return total


def points(centroids, k: int, d: int, qmin: int, scale: int) -> list:
    """The centroids in record units: k lists of d Fractions QueryMin + c / scale."""
    return [[qmin + Fraction(int(centroids[c * d + j]), scale) for j in range(d)] for c in range(k)]


def random_centroids(k: int, d: int, R: int, scale: int, seed) -> list:
    """k * d start coordinates, uniform over 0 .. (R - 1) * scale, a function of
    ``seed`` (an int or a string) alone: SHA-256 in counter mode, the same on
    every platform."""
    top = (int(R) - 1) * int(scale)
    out = []
    for i in range(int(k) * int(d)):
        h = hashlib.sha256(f"kmeans/{seed}/{i}".encode()).digest()
        out.append(int.from_bytes(h[:16], "big") % (top + 1))
    return out
