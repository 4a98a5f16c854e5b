"""The arithmetic of one round of an iterative (digit-by-digit) query.

An iterative ``min``, ``max`` or ``frequencyCount`` over [QueryMin, QueryMax]
in base b has R = QueryMax - QueryMin + 1 values and L rounds, L the smallest
integer with b^L >= R.  Round k (0 <= k < L) carries the prefix of the k digits
found so far, 0 <= prefix < b^k, and looks at the digit (o div lo) mod b of an
offset o = x - QueryMin with o div hi == prefix, where lo = b^(L-1-k) and
hi = b * lo.  The query rules, the native binding and the tools all read the
limits and the round from here (csrc/kernels/dx_iter_round.hip checks the same
rule below the binding).  No torch, no native import.
"""
from __future__ import annotations

ITER_OPERATIONS = ("min", "max", "frequencyCount")
ITER_MAX_BASE = 65536
ITER_MAX_HIST_BASE = 4096  # frequencyCount rounds: one LDS counter per output (csrc/kernels/dx_iter_round.hip)
ITER_MAX_RANGE = 1 << 40  # every power of the base a round divides by stays far inside int64
# rounds over the G cells of a SQL plan (one search per cell, SurveyQuery.IterPrefixes): G * base outputs per DP
# (csrc/kernels/dx_iter_round.hip dx_iter_round_cells checks the same number); every operation counts, so the
# base is at most ITER_MAX_HIST_BASE
ITER_MAX_CELL_OUTPUTS = 1 << 20


def max_base(name: str) -> int:
    """The largest base of an iterative ``name`` query."""
    if name not in ITER_OPERATIONS:
        raise ValueError(f"Operation: <{name}> has no iterative rounds")
    return ITER_MAX_HIST_BASE if name == "frequencyCount" else ITER_MAX_BASE


def iter_rounds(qmin: int, qmax: int, base: int) -> int:
    """Rounds L of the iterative min/max over [qmin, qmax] in base ``base``: the
    smallest integer with base^L >= qmax - qmin + 1 (integer products, no log)."""
    R = int(qmax) - int(qmin) + 1
    base = int(base)
    if base < 2 or R < 1:
        raise ValueError(f"no iterative rounds for base {base} over {R} values")
    L, p = 1, base
    while p < R:
        p *= base
        L += 1
    return L


def iter_round(name: str, qmin: int, qmax: int, base: int, k: int, prefix: int) -> tuple:
    """``(L, lo)`` of round ``k`` of the iterative ``name`` query over [qmin,
    qmax] in base ``base`` under ``prefix``, lo = base^(L-1-k); ValueError for
    an operation without rounds, a base or a domain outside the limits, a
    round outside 0..L-1 or a prefix that is not a number of k digits."""
    qmin, qmax, base, k, prefix = int(qmin), int(qmax), int(base), int(k), int(prefix)
    R = qmax - qmin + 1
    if not 2 <= base <= max_base(name) or not 1 <= R <= ITER_MAX_RANGE:
        raise ValueError(f"iterative {name}: base {base}, {R} values")
    L = iter_rounds(qmin, qmax, base)
    if not 0 <= k < L or not 0 <= prefix < base ** k:
        raise ValueError(f"iterative {name}: round {k} of {L}, prefix {prefix}")
    return L, base ** (L - 1 - k)


def iter_round_cells(name: str, qmin: int, qmax: int, base: int, k: int, prefixes, n_cells: int) -> tuple:
    """``(L, lo)`` of round ``k`` of ``n_cells`` simultaneous iterative ``name``
    searches, one per cell of a SQL plan, cell g under ``prefixes[g]``: the
    round of ``iter_round`` with the counting base limit (min / max are derived
    from the counts) for every distinct prefix, exactly ``n_cells`` prefixes
    and ``n_cells * base`` at most ITER_MAX_CELL_OUTPUTS."""
    if name not in ITER_OPERATIONS:
        raise ValueError(f"Operation: <{name}> has no iterative rounds")
    prefixes = [int(p) for p in prefixes]
    if n_cells < 1 or len(prefixes) != n_cells:
        raise ValueError(f"iterative {name}: {len(prefixes)} prefixes for {n_cells} cells")
    if n_cells * int(base) > ITER_MAX_CELL_OUTPUTS:
        raise ValueError(f"iterative {name}: {n_cells} cells of {base} outputs (at most {ITER_MAX_CELL_OUTPUTS})")
    out = None
    for p in sorted(set(prefixes)):
        out = iter_round("frequencyCount", qmin, qmax, base, k, p)
    return out
