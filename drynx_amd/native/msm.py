"""Bucket plans of the verifier's three multi-scalar products: the GT
multi-exponentiation, the G1 MSM of the D-check and the G2 MSM of the R side
(csrc/kernels/dx_rpmsm.hip, dx_plan.hip).  One pipeline, each stage once:

  runs     ``_runs``: bucket keys of every (entry, window), sorted, and every
           bucket's run in the sorted entries;
  plan     ``CountedPlan`` (one host sync, arbitrary groups) or the cached
           ``DeviceLayout`` (shape-derived, no sync): the sorted ids of the
           buckets that carry a value, the slice passes that reduce the sorted
           entries to one row per such bucket (``_reduce``, given the group's
           two slice operations) and the weights record, built with the plan;
  weights  digit times bucket, summed per (group, window), the same stage for
           either plan: ``DigitWeights`` (G1) or ``ChunkWeights`` (G2, GT);
  finish   Horner over the windows of a ``Handle``.

``drynx_amd.native`` re-exports the public names.
"""
from __future__ import annotations

import threading
from dataclasses import dataclass, field, fields
from functools import partial

import numpy as np

import torch

from . import (_call, _ctx, _pow2_scalar, _ptr, _raw_call, _rows, _upload, g1_mul, gt_mul, gt_one, gt_pi, gt_pow,
               gt_prod)

_ME_SLICE = 8      # entries per thread in each segmented-product pass
# entries per lane pair in the first pass over torus images (gt_beta_slice_prod): the first factor of a
# slice is free and a step costs two Fp6 products, so longer slices pay (profiles/me_torus/README.md)
_ME_TORUS_SLICE = 32
G2_CHUNK = 32      # digit range of one running-sum chunk of Pippenger buckets


# ----------------------------------------------------------------------------- slice and chunk kernels
def gt_slice_prod(src: torch.Tensor, idx, start: torch.Tensor, length: torch.Tensor) -> torch.Tensor:
    """out[s] = prod_k src[idx[start[s] + k]] (or src[start[s] + k]), k < length[s].
    (A latency-hidden 1-wave/SIMD variant with the gathers issued one
    product ahead measured the same, 3.62 vs 3.71 ms on 3.4M factors, and
    was dropped.)"""
    n = start.numel()
    out = torch.empty((n, 96), dtype=torch.int32, device=src.device)
    g, s = _ctx(src, idx, start, length)
    _call("dx_gt_slice_prod", g, s, _ptr(src), _ptr(idx), _ptr(start), _ptr(length), _ptr(out), n)
    return out


def gt_beta_slice_prod(beta: torch.Tensor, idx, start: torch.Tensor, length: torch.Tensor) -> torch.Tensor:
    """out[s] = a numerator (gt_torus.h) of prod_k pi(beta[idx[start[s] + k]] + w)
    (or beta[start[s] + k]), k < length[s], over torus images beta [., 48]: the
    first row of a slice is free, every further one costs two Fp6 products.
    All-zero rows are skipped; an empty slice gives 1.  ``gt_pi`` of the result
    is ``gt_slice_prod`` over the elements the rows are images of."""
    n = start.numel()
    assert beta.shape[-1] == 48 and (idx is None or idx.dtype == torch.int64)
    assert start.dtype == torch.int64 and length.dtype == torch.int32
    out = torch.empty((n, 96), dtype=torch.int32, device=beta.device)
    g, s = _ctx(beta, idx, start, length)
    _call("dx_gt_beta_slice_prod", g, s, _ptr(beta), _ptr(idx), _ptr(start), _ptr(length), _ptr(out), n)
    return out


def g1_slice_sum(src: torch.Tensor, idx, start: torch.Tensor, length: torch.Tensor) -> torch.Tensor:
    """out[s] = sum_k src[idx[start[s] + k]] (or src[start[s] + k]), k < length[s] (Jacobian)."""
    n = start.numel()
    out = torch.empty((n, 24), dtype=torch.int32, device=src.device)
    g, s = _ctx(src, idx, start, length)
    _call("dx_g1_slice_sum", g, s, _ptr(src), _ptr(idx), _ptr(start), _ptr(length), _ptr(out), n)
    return out


def g2_slice_sum(src: torch.Tensor, idx, start: torch.Tensor, length: torch.Tensor, src_aff: bool,
                 idx_mod: int = 0) -> torch.Tensor:
    """out[s] = sum_k src[idx[start[s] + k] % idx_mod] (or src[start[s] + k]),
    k < length[s], from affine (mixed additions) or Jacobian G2 rows -> Jacobian [n, 48]."""
    n = start.numel()
    assert src.shape[-1] == (32 if src_aff else 48) and (idx is None or idx.dtype == torch.int32)
    assert start.dtype == torch.int64 and length.dtype == torch.int32
    out = torch.empty((n, 48), dtype=torch.int32, device=src.device)
    g, s = _ctx(src, idx, start, length)
    _call("dx_g2_slice_sum", g, s, _ptr(src), _ptr(idx), _ptr(start), _ptr(length), _ptr(out), n, int(src_aff),
          int(idx_mod))
    return out


_g2_jac_sum = partial(g2_slice_sum, src_aff=False)      # over Jacobian rows: every level but the first


def gt_chunk_weight(B: torch.Tensor, d: torch.Tensor, start: torch.Tensor, length: torch.Tensor,
                    base: torch.Tensor) -> torch.Tensor:
    """out[ch] = prod_{i in chunk ch} B[i]^d[i] over digit-sorted GT buckets
    (chunk: start/length rows whose digits lie in [base, base + L)) -- running
    products instead of one power per bucket."""
    n = start.numel()
    out = torch.empty((n, 96), dtype=torch.int32, device=B.device)
    g, s = _ctx(B, d, start, length, base)
    _call("dx_gt_chunk_weight", g, s, _ptr(B.contiguous()), _ptr(d.contiguous()), _ptr(start), _ptr(length),
          _ptr(base), _ptr(out), n)
    return out


def g2_chunk_weight(B_jac: torch.Tensor, d: torch.Tensor, start: torch.Tensor, length: torch.Tensor,
                    base: torch.Tensor) -> torch.Tensor:
    """out[ch] = sum_{i in chunk ch} d[i] B[i] over digit-sorted Jacobian
    buckets (chunk: start/length rows whose digits lie in [base, base +
    G2_CHUNK)) -- running sums instead of one multiplication per bucket."""
    n = start.numel()
    assert B_jac.shape[-1] == 48 and d.dtype == torch.int32 and start.dtype == torch.int64
    assert length.dtype == torch.int32 and base.dtype == torch.int32 and base.numel() == n
    out = torch.empty((n, 48), dtype=torch.int32, device=B_jac.device)
    g, s = _ctx(B_jac, d, start, length, base)
    _call("dx_g2_chunk_weight", g, s, _ptr(B_jac.contiguous()), _ptr(d.contiguous()), _ptr(start), _ptr(length),
          _ptr(base), _ptr(out), n)
    return out


# The two slice operations of each group, for ``_reduce``: ``first(start, len)`` reads the source rows through the
# sorted item index, ``next(cur, None, start, len)`` (the group's slice kernel) the level before.  The groups' index
# types and row periods stay in here.
def _gt_ops(a: torch.Tensor, items: torch.Tensor, item_split: tuple | None = None):
    """Entry i reads a[i % n] (n = rows of a); with ``item_split`` = (s, q)
    entry i >= s reads a[(i - s) % q].  The kernel takes int64 premapped rows.
    ``a`` is [n, 96] Fp12 rows or [n, 48] torus images (``gt_beta_rows``): with
    images the first pass leaves numerators, which are ordinary Fp12 values,
    so every later pass is the same generic product."""
    n = a.shape[0]
    first = gt_beta_slice_prod if a.shape[-1] == 48 else gt_slice_prod
    it = items.to(torch.int64)
    if item_split is not None:
        sp, q = item_split
        it = torch.where(it < sp, it % n, (it - sp) % q)
    else:
        it = it % n
    it = it.contiguous()
    return (lambda st, ln: first(a, it, st, ln)), gt_slice_prod


def _g1_ops(P_jac: torch.Tensor, items: torch.Tensor):
    P_jac, it = P_jac.contiguous(), items.to(torch.int64)
    return (lambda st, ln: g1_slice_sum(P_jac, it, st, ln)), g1_slice_sum


def _g2_ops(P_aff: torch.Tensor, items: torch.Tensor, m: int):
    """Entry i reads the affine row P[i % m] (int32 index, modulus in the kernel)."""
    return (lambda st, ln: g2_slice_sum(P_aff, items, st, ln, True, m)), _g2_jac_sum


# ----------------------------------------------------------------------------- runs
def _group_arg(group, n: int, dev):
    """(explicit int32 group tensor or None, group stride): an int ``group``
    means entry t belongs to group t // group (no per-entry tensor)."""
    if group is None:
        return None, 0
    if isinstance(group, int):
        return None, group
    assert group.numel() == n
    return group.to(device=dev, dtype=torch.int32).contiguous(), 0


def _runs(k: torch.Tensor, group, n_groups: int, W: int, c: int):
    """Bucket keys of a multi-scalar product over the low W c-bit windows of
    the scalars k [n, 8]: window w, digit d of an entry of group g -> bucket
    (g W + w) 2^c + d, built by one kernel (zero digits get a sentinel that
    sorts last); the entries sorted by key (torch's onesweep radix sort: on
    gfx950 faster than a direct rocPRIM pairs sort over the keys' bits, and it
    interferes least with the kernels running beside the plan,
    profiles/r4/ab_plan_sort.txt; an atomic counting sort measured +22 ms on a
    1-GPU inbox's 60M entries) and every bucket's run in them
    (csrc/kernels/dx_plan.hip) -> (items sorted by key, first[nb], end[nb]) on
    the device (empty buckets: first = end = 0)."""
    dev = k.device
    n = k.shape[0]
    nb = (W << c) * n_groups
    assert n * W < 2 ** 31 and nb < 2 ** 31 - 1
    keys = torch.empty(n * W, dtype=torch.int32, device=dev)
    items = torch.empty(n * W, dtype=torch.int32, device=dev)
    grp, gstride = _group_arg(group, n, dev)
    g, s = _ctx(k, keys)
    _call("dx_msm_keys", g, s, _ptr(k.contiguous()), _ptr(grp), gstride, n, c, W, _ptr(keys), _ptr(items))
    k2, order = torch.sort(keys)
    items = items.index_select(0, order)
    bounds = torch.zeros((2, nb), dtype=torch.int64, device=dev)
    g, s = _ctx(k2)
    _call("dx_bucket_bounds", g, s, _ptr(k2), keys.numel(), nb, _ptr(bounds[0]), _ptr(bounds[1]))
    return items, bounds[0], bounds[1]


# ----------------------------------------------------------------------------- plans
def _segment_passes(counts, first=None):
    """Slice plans that reduce contiguous runs of `counts` entries to one
    value per run, <= _ME_SLICE entries per thread per pass (a lone GPU lane
    runs an Fp12 chain latency-bound, so chains stay short and each pass is
    wide).  ``first``: where each run starts in the first pass's source
    (default: the runs are packed).  Returns [(start, len), ...] numpy arrays
    per pass."""
    passes = []
    c = np.asarray(counts, dtype=np.int64)
    while c.size and c.max() > 1:
        n_sl = (c + _ME_SLICE - 1) // _ME_SLICE
        if first is None:
            first = np.cumsum(c) - c
        b = np.repeat(np.arange(c.size), n_sl)
        k = np.arange(b.size) - (np.cumsum(n_sl) - n_sl)[b]
        passes.append((first[b] + k * _ME_SLICE, np.minimum(c[b] - k * _ME_SLICE, _ME_SLICE)))
        c, first = n_sl, None
    return passes


def _segment_passes_dev(counts, dev, first_slice: int | None = None):
    """``_segment_passes`` with the per-slice (start, len) arrays written on
    the device by one thread per bucket (csrc/kernels/dx_plan.hip
    dx_slice_plan): only the per-bucket counts (at most a few hundred
    thousand) go through the host; the millions of slice descriptors of a wide
    multi-exponentiation are never built by numpy or torch index kernels.
    ``first_slice``: entries per thread in the first pass (later passes use
    _ME_SLICE)."""
    passes = []
    c = np.asarray(counts, dtype=np.int64)
    while c.size and c.max() > 1:
        sl = first_slice if (first_slice and not passes) else _ME_SLICE
        n_sl = (c + sl - 1) // sl
        total = int(n_sl.sum())
        meta = np.stack([np.cumsum(c) - c, c, np.cumsum(n_sl) - n_sl])
        m_dev = _upload(meta, dev)
        start = torch.empty(total, dtype=torch.int64, device=dev)
        ln = torch.empty(total, dtype=torch.int32, device=dev)
        g, s = _ctx(m_dev)
        _call("dx_slice_desc", g, s, _ptr(m_dev[0]), _ptr(m_dev[1]), _ptr(m_dev[2]), sl, c.size, total, _ptr(start),
              _ptr(ln))
        passes.append((start, ln))
        c = n_sl
    return passes


class _Record:
    """Base of the records: a field is also read by name, ``r["W"]`` (the spelling of the dicts they
    replace, which tests and tools outside this module still use), and each knows its tensors."""

    def __getitem__(self, name: str):
        return getattr(self, name)

    def tensors(self, x=None):
        """Every tensor the record reaches: its fields, through lists, tuples and nested records."""
        for y in [getattr(self, f.name) for f in fields(self)] if x is None else x:
            if isinstance(y, torch.Tensor):
                yield y
            elif isinstance(y, (list, tuple, _Record)):
                yield from y.tensors() if isinstance(y, _Record) else self.tensors(y)


@dataclass
class CountedPlan(_Record):
    """Plan from the buckets' actual counts (``_counted_plan``)."""
    item: torch.Tensor                  # the sorted entries without the zero-digit sentinels
    bk: np.ndarray                      # sorted ids of the non-empty buckets (host)
    passes: list                        # segmented slices down to one value per such bucket (``_reduce``)
    G: int
    W: int
    c: int
    weights: DigitWeights | ChunkWeights | None    # None: no bucket holds an entry


def _counted_plan(k: torch.Tensor, group, n_groups: int, W: int, c: int, weights: type,
                  first_slice: int | None = None) -> CountedPlan:
    """ONE host sync (the counts), any grouping; ``weights``: the record class of its weights."""
    dev = k.device
    items, first, end = _runs(k, group, n_groups, W, c)
    counts = (end - first).cpu().numpy().astype(np.int64)               # the plan's one device-to-host copy
    bk = np.flatnonzero(counts)
    passes = _segment_passes_dev(counts[bk], dev, first_slice)
    if bk.size and not passes:  # every bucket holds one entry
        passes = [(torch.arange(bk.size, device=dev), torch.ones(bk.size, dtype=torch.int32, device=dev))]
    return CountedPlan(items[: int(counts.sum())], bk, passes, n_groups, W, c,
                       weights.build(bk, c, dev) if bk.size else None)


_DPLANS = {}       # (shape, device, weights record class) -> DeviceLayout, in the order built
_PLAN_LIMIT = 32


@dataclass
class DeviceLayout(_Record):
    """A counted plan takes ONE host sync (the per-bucket counts decide the
    slice passes).  A device-resident plan fixes its layout from the plan's
    SHAPE instead: every bucket owns a number of lanes set by its window's
    expected run (uniform digits: the batch weights are uniform), each lane
    takes an equal share of the bucket's actual run (csrc/kernels/dx_plan.hip
    dx_lane_slices), the multi-lane buckets reduce by a fixed tree and the
    bucket weighting runs over a fixed set of buckets.  Nothing goes through
    the host, so every pass is queued at once behind the sort."""
    n_lanes: int
    used: np.ndarray                    # sorted ids of the buckets of the declared widths (host)
    lane_bucket: torch.Tensor           # per lane: its bucket, and its rank among the bucket's lanes
    lane_j: torch.Tensor
    lanes: torch.Tensor                 # per bucket: its lane count, and its first lane
    first_lane: torch.Tensor
    multi: torch.Tensor                 # the buckets with several lanes
    passes: list                        # the tree over their lanes
    used_t: torch.Tensor
    unused_t: torch.Tensor
    weights: DigitWeights | ChunkWeights
    _streams: set = field(default_factory=set)      # ids of the streams recorded on ``tensors()`` (``_mark_use``)


def _mark_use(lay: DeviceLayout, dev):
    """A cached layout is read by kernels of whatever stream the caller is on;
    its tensors were allocated on the stream that built it.  Every new user
    stream is recorded on them (``record_stream``), so when the cache evicts
    the layout the caching allocator hands its blocks out again only after
    every such stream has passed its last use -- without this an eviction
    while another stream's kernels still read the layout let the building
    stream reuse the memory under them (profiles/r6/graph_fault.md).  A HIP
    graph being captured keeps the layout itself (``capture_keep``): a
    captured launch reads it at every replay, long after any eviction."""
    keep = getattr(_CAPTURE, "keep", None)
    if keep is not None:
        keep.append(lay)
    s = torch.cuda.current_stream(dev) if dev.type == "cuda" else None
    if s is not None and s.stream_id not in lay._streams:
        lay._streams.add(s.stream_id)
        for t in lay.tensors():
            t.record_stream(s)


_CAPTURE = threading.local()


class capture_keep:
    """Inside a HIP graph capture on this thread: collects every cached device
    object the captured launches read (``_mark_use``) into ``self.items``;
    the graph must hold them for its lifetime."""

    def __enter__(self):
        self.prev = getattr(_CAPTURE, "keep", None)
        self.items = []
        _CAPTURE.keep = self.items
        return self

    def __exit__(self, *a):
        _CAPTURE.keep = self.prev
        return False


def _device_layout(groups: tuple, W: int, c: int, sl: int, dev, weights: type | None = None) -> DeviceLayout:
    """The layout of a shape, cached per shape and ``weights`` record class (default ``ChunkWeights``).
    ``groups`` = ((entries, scalar bits), ...) per group.  Window w of a group
    with b = min(c, bits - w c) > 0 bits uses the buckets of digits 1 .. 2^b - 1,
    each with ceil(entries / (2^b sl)) lanes; every other bucket keeps one lane
    and must stay empty (``overflow`` counts entries that land there)."""
    dev, weights = torch.device(dev), weights or ChunkWeights
    key = (groups, W, c, sl, str(dev), weights)
    lay = _DPLANS.get(key)
    if lay is not None:
        _mark_use(lay, dev)
        return lay
    D = 1 << c
    nb = len(groups) * W * D
    lanes = np.ones(nb, dtype=np.int64)
    used = np.zeros(nb, dtype=bool)
    for g, (rows, bits) in enumerate(groups):
        for w in range(W):
            bw = min(c, int(bits) - w * c)
            if bw <= 0:
                continue
            base, hi = (g * W + w) * D, 1 << bw
            used[base + 1: base + hi] = True
            lanes[base + 1: base + hi] = max(1, -(-int(rows) // (hi * sl)))
    off = np.cumsum(lanes) - lanes
    L = int(lanes.sum())
    lane_bucket = np.repeat(np.arange(nb), lanes)
    lane_j = np.arange(L) - off[lane_bucket]
    multi = np.flatnonzero(lanes > 1)
    # the tree over the multi-lane buckets' lanes: its first level reads them in
    # place in the lane array, the next ones the compacted results
    passes = _segment_passes(lanes[multi], off[multi])
    up = lambda a, dt: _upload(np.asarray(a).astype(dt), dev)  # noqa: E731
    ubk = np.flatnonzero(used)
    lay = DeviceLayout(L, ubk, lane_bucket=up(lane_bucket, np.int32), lane_j=up(lane_j, np.int32),
                       lanes=up(lanes, np.int32), first_lane=up(off, np.int64), multi=up(multi, np.int64),
                       passes=[(up(st, np.int64), up(ln, np.int32)) for st, ln in passes],
                       used_t=up(ubk, np.int64), unused_t=up(np.flatnonzero(~used), np.int64),
                       weights=weights.build(ubk, c, dev))
    if dev.type == "cuda":  # uploaded on this stream, weights included; readers on others must not see it half-copied
        torch.cuda.current_stream(dev).synchronize()
    while len(_DPLANS) > _PLAN_LIMIT:  # least recently built first (see ``_mark_use`` for why that is safe)
        _DPLANS.pop(next(iter(_DPLANS)))
    _DPLANS[key] = lay
    _mark_use(lay, dev)
    return lay


def _lane_slices(first: torch.Tensor, end: torch.Tensor, lay: DeviceLayout):
    """Every lane's equal share of its bucket's run: the layout's first pass."""
    L = lay.n_lanes
    st = torch.empty(L, dtype=torch.int64, device=first.device)
    ln = torch.empty(L, dtype=torch.int32, device=first.device)
    g, s = _ctx(first, st)
    _call("dx_lane_slices", g, s, _ptr(first), _ptr(end), _ptr(lay.lane_bucket), _ptr(lay.lane_j),
          _ptr(lay.lanes), L, _ptr(st), _ptr(ln))
    return st, ln


def _reduce(passes: list, ops: tuple, lay: DeviceLayout | None = None) -> torch.Tensor:
    """Sorted entries -> one row per bucket that carries a value.  ``ops`` =
    (first, next): passes[0] reads the source through the item index, every
    later pass the level before.  A counted plan's passes end at one row per
    bucket of ``bk``.  With a layout the first pass leaves one row per lane: a
    single-lane bucket's is its value, the later passes are the tree over the
    multi-lane buckets' lanes -> one row per USED bucket (``lay.used`` order)."""
    first_op, next_op = ops
    cur = first_op(*passes[0])
    B = cur.index_select(0, lay.first_lane) if lay is not None else None
    for st, ln in passes[1:]:
        cur = next_op(cur, None, st, ln)
    if lay is None:
        return cur
    if len(passes) > 1:
        B.index_copy_(0, lay.multi, cur)
    return B.index_select(0, lay.used_t)


def _device_buckets(k: torch.Tensor, group, groups: tuple, W: int, c: int, sl: int, weights: type, ops):
    """Runs, shape-derived layout (``sl`` entries per lane, ``weights`` record)
    and reduction, all queued without a host sync; ``ops(items)`` gives the
    group's slice operations -> (one row per used bucket, layout, overflow:
    the entries in buckets outside the layout, i.e. scalars wider than
    declared, as a device scalar for ``check_overflow``)."""
    items, first, end = _runs(k, group, len(groups), W, c)
    lay = _device_layout(tuple(groups), W, c, sl, k.device, weights)
    B = _reduce([_lane_slices(first, end, lay)] + lay.passes, ops(items), lay)
    return B, lay, (end - first).index_select(0, lay.unused_t).sum()


@dataclass
class Handle(_Record):
    """What a launched product leaves for its finisher."""
    G: int
    W: int
    c: int
    rows: torch.Tensor | None = None    # per-window rows (G2 hands its window sums over beside the handle)
    gws: np.ndarray | None = None       # the (group, window) g W + w of every row; None: all G W, in order
    overflow: torch.Tensor | None = None    # a device plan's entries outside the declared widths
    torus: bool = False                 # GT rows are numerators of torus images


def check_overflow(h: Handle):
    """Raise if a device-resident plan dropped entries (checked once the results are read back: no extra host sync)."""
    if h.overflow is not None and int(h.overflow) != 0:
        raise RuntimeError(f"device bucket plan: {int(h.overflow)} entries fell outside the declared scalar widths")


# ----------------------------------------------------------------------------- weights
@dataclass
class DigitWeights(_Record):
    """G1: the digit scalars of d * B_{g,w,d}, then per-(group, window) sums -- the sorted
    bucket keys are (g W + w) 2^c + d, so each (group, window) is a contiguous run."""
    sc: torch.Tensor                    # [buckets, 8] digit scalars
    gws: np.ndarray                     # the (group, window) of every summed row (host)
    passes: list

    @classmethod
    def build(cls, bk, c: int, dev) -> DigitWeights:
        sc = np.zeros((bk.size, 8), dtype=np.int32)
        sc[:, 0] = bk & ((1 << c) - 1)
        gws, counts = np.unique(bk >> c, return_counts=True)
        return cls(_upload(sc, dev), gws,
                   [(_upload(st, dev), _upload(ln.astype("int32"), dev)) for st, ln in _segment_passes(counts)])

    def weigh(self, B: torch.Tensor) -> tuple:
        """Bucket sums -> d * B_{g,w,d} (one short variable-base launch) ->
        per-(group, window) sums on the device -> (one row per ``gws``, ``gws``)."""
        cur = g1_mul(B, self.sc)
        for st, ln in self.passes:
            cur = g1_slice_sum(cur, None, st, ln)
        return cur, self.gws


@dataclass
class ChunkWeights(_Record):
    """G2 and GT: running sums / running products over chunks of an aligned
    digit range (csrc/kernels/dx_rpmsm.hip chunk_weight_one, dx_range.hip
    gt_chunk_weight_coop), then per-(group, window) sums of the chunk results."""
    d: torch.Tensor                     # every bucket's digit
    chunks: tuple                       # (first bucket, buckets, digit base) of every chunk
    gws: torch.Tensor                   # the (group, window) of every summed row
    passes: list

    @classmethod
    def build(cls, bk, c: int, dev) -> ChunkWeights:
        # digit range of a chunk: 32 (about two additions per bucket) while that still gives ~16k chunk lanes,
        # shorter for a small plan (a 1/8 pool slice: 8, i.e. 4x the lanes with a third of the chain)
        chunk = G2_CHUNK
        while chunk > 4 and bk.size // chunk < 16384:
            chunk //= 2
        dig = bk & ((1 << c) - 1)
        gw = bk >> c
        ck = gw * ((1 << c) // chunk + 1) + dig // chunk
        first = np.flatnonzero(np.r_[True, ck[1:] != ck[:-1]])
        clen = np.diff(np.r_[first, bk.size])
        gwf = gw[first]                                  # sorted: run lengths instead of np.unique's sort
        gstart = np.flatnonzero(np.r_[True, gwf[1:] != gwf[:-1]])
        gws, gcounts = gwf[gstart], np.diff(np.r_[gstart, gwf.size])
        return cls(_upload(dig.astype("int32"), dev),
                   (_upload(first.astype(np.int64), dev), _upload(clen.astype(np.int32), dev),
                    _upload(((dig[first] // chunk) * chunk).astype(np.int32), dev)),
                   _upload(gws.astype(np.int64), dev), _segment_passes_dev(gcounts, dev))

    def weigh(self, B: torch.Tensor, chunk_op, slice_op, out: torch.Tensor) -> torch.Tensor:
        """One row per bucket -> ``out`` [G W, .] (neutral rows) with the row of every window that holds a bucket."""
        cur = chunk_op(B, self.d, *self.chunks)
        for st, ln in self.passes:
            cur = slice_op(cur, None, st, ln)
        return out.index_copy_(0, self.gws, cur)


# ----------------------------------------------------------------------------- GT multi-exponentiation
def me_window(groups: tuple, lo: int = 8, hi: int = 16) -> tuple:
    """(W, c) of a GT multi-exponentiation over ``groups`` = ((entries,
    exponent bits), ...): c minimises the bucket products (entries x windows)
    plus ~3 products per bucket for the running-product weights -> 16-bit
    windows for a whole 1-GPU inbox (2 windows per 32-bit GLV half instead of
    3), 11 bits for a pool slice."""
    def cost(c):
        return sum(r * -(-b // c) for r, b in groups) + 3 * sum(-(-b // c) for _, b in groups) * (1 << c)
    c = min(range(lo, hi + 1), key=cost)
    return max(-(-b // c) for _, b in groups), c


def multi_exp_plan(k: torch.Tensor, group, n_groups: int, W: int = 8, c: int = 8):
    """The bucket plan of ``multi_exp_grouped`` alone (its one host sync)."""
    return _counted_plan(k, group, n_groups, W, c, ChunkWeights)


def _gt_windows(B: torch.Tensor, wp: ChunkWeights, G: int, W: int) -> torch.Tensor:
    """One row per bucket -> the dense [1, G W, 96] window rows; a window without a bucket is one."""
    return wp.weigh(B, gt_chunk_weight, gt_slice_prod, gt_one(B.device).repeat(G * W, 1)).view(1, G * W, 96)


def multi_exp_grouped(a: torch.Tensor, k: torch.Tensor, group, n_groups: int, W: int = 8, c: int = 8,
                      plan: CountedPlan | None = None) -> Handle:
    """Launch G independent multi-exponentiations prod_{i: group_i = g} a[i % n]^k_i
    (n = rows of a, k [m, 8] with m a multiple of n, low W c-bit windows of
    each exponent; ``group`` an int32 tensor or an int stride) as ONE bucket
    plan (one host sync for all groups, e.g. the batch weights of several
    verifying nodes, unless ``plan`` comes from ``multi_exp_plan``).  Returns a
    handle for ``multi_exp_grouped_finish``; device passes are queued on the
    current stream."""
    plan = plan or multi_exp_plan(k, group, n_groups, W, c)
    h = Handle(n_groups, W, c)
    if plan.weights is not None:
        h.rows = _gt_windows(_reduce(plan.passes, _gt_ops(a, plan.item)), plan.weights, n_groups, W)
    return h


def multi_exp_device(a: torch.Tensor, k: torch.Tensor, group, groups: tuple, W: int | None = None,
                     c: int | None = None, item_split: tuple | None = None, first_slice: int | None = None) -> Handle:
    """``multi_exp_grouped`` with a device-resident plan (no host sync):
    ``groups`` = ((entries, exponent bits), ...) per group (window from
    ``me_window`` unless given).  -> the handle of ``multi_exp_grouped_finish``.
    ``item_split`` = (s, q): entry i < s uses a[i % n], entry i >= s uses
    a[(i - s) % q] (two exponent blocks over different row periods).
    ``a`` [n, 48]: torus images of the rows (``gt_beta_rows``) -- the first
    pass then runs on numerators (``gt_beta_slice_prod``, ``first_slice``
    entries per lane, default ``_ME_TORUS_SLICE``), the later passes are
    unchanged, and ``multi_exp_grouped_finish`` maps the per-window rows back
    by ``gt_pi``: the same results, bit for bit."""
    torus = a.shape[-1] == 48
    sl = first_slice or (_ME_TORUS_SLICE if torus else _ME_SLICE)
    G = len(groups)
    if c is None:
        W, c = me_window(tuple(groups))
    B, lay, overflow = _device_buckets(k, group, groups, W, c, sl, ChunkWeights,
                                       lambda items: _gt_ops(a, items, item_split))
    return Handle(G, W, c, _gt_windows(B, lay.weights, G, W), overflow=overflow, torus=torus)


def multi_exp_grouped_finish(h: Handle) -> torch.Tensor:
    """[G, 96] host results: the Horner steps over the window rows on the host."""
    G, W = h.G, h.W
    if h.rows is None:
        return gt_one("cpu").repeat(G, 1)
    S_w = gt_prod(h.rows.cpu(), chunk=64)                   # [1, G W, 96] -> [G W, 96]
    if h.torus:                                             # numerators -> the canonical unitary values
        S_w = gt_pi(S_w)
    S_w = S_w.view(G, W, 96)
    acc = S_w[:, W - 1].contiguous()
    sh = _pow2_scalar(h.c).expand(G, 8).contiguous()
    for w in range(W - 2, -1, -1):
        acc = gt_mul(gt_pow(acc, sh), S_w[:, w].contiguous())
    return acc


# ----------------------------------------------------------------------------- G1 MSM (the D-check)
def g1_msm(P_jac: torch.Tensor, k: torch.Tensor, bits: int = 256) -> torch.Tensor:
    """sum_i k_i P_i (Pippenger bucket method, 8-bit windows) -> [1, 24] HOST
    Jacobian point.  Buckets accumulate in wide segmented passes on the device
    (no per-point 256-step doubling chain: the cost is ~bits/8 additions per
    point), bucket weights d*B_{w,d} are one short variable-base launch, and
    the 32-window Horner combination runs on the host pool."""
    return g1_msm_grouped(P_jac, k, None, 1, bits)


def g1_msm_grouped(P_jac: torch.Tensor, k: torch.Tensor, group: torch.Tensor | None, n_groups: int,
                   bits: int = 256) -> torch.Tensor:
    """G independent MSMs in one bucket pass: out[g] = sum_{i: group_i = g}
    k_i P_i -> [n_groups, 24] HOST Jacobian points.  Only non-zero 8-bit
    digits enter a bucket, so a 64-bit weight costs 8 bucket additions, not
    32: batch verifiers keep the short random weights in their own group and
    apply the shared full-size factor (a challenge) to the group's sum on the
    host, instead of multiplying it into every per-element scalar."""
    return g1_msm_finish(g1_msm_launch(P_jac, k, group, n_groups, bits))


def g1_msm_plan(k: torch.Tensor, group, n_groups: int, bits: int = 256):
    """The bucket plan of ``g1_msm_launch`` alone (its one host sync), so a
    caller can take every plan's sync before queueing any heavy pass."""
    return _counted_plan(k, group, n_groups, (bits + 7) // 8, 8, DigitWeights) if k.shape[0] else None


def g1_msm_launch(P_jac: torch.Tensor, k: torch.Tensor, group: torch.Tensor | None, n_groups: int,
                  bits: int = 256, plan: CountedPlan | None = None) -> Handle:
    """First half of g1_msm_grouped: the bucket plan (one host sync on k,
    unless ``plan`` comes from ``g1_msm_plan``) and every device pass, queued
    on the current stream.  g1_msm_finish waits for them and runs the Horner
    steps on the host."""
    assert P_jac.shape[0] == k.shape[0]
    assert group is None or isinstance(group, int) or group.numel() == k.shape[0]
    plan = plan or g1_msm_plan(k, group, n_groups, bits)
    if plan is None or plan.weights is None:
        return Handle(n_groups, (bits + 7) // 8, 8)
    return Handle(n_groups, plan.W, 8, *plan.weights.weigh(_reduce(plan.passes, _g1_ops(P_jac, plan.item))))


def g1_msm_device(P_jac: torch.Tensor, k: torch.Tensor, group, groups: tuple, bits: int = 256) -> Handle:
    """``g1_msm_launch`` with a device-resident plan (8-bit windows, no host
    sync) -> the handle of ``g1_msm_finish``."""
    W = (bits + 7) // 8
    B, lay, overflow = _device_buckets(k, group, groups, W, 8, _ME_SLICE, DigitWeights,
                                       lambda items: _g1_ops(P_jac, items))
    return Handle(len(groups), W, 8, *lay.weights.weigh(B), overflow)


def g1_msm_finish(h: Handle) -> torch.Tensor:
    from ..crypto.bn254 import g1_infinity_jac

    G, W, gws = h.G, h.W, h.gws
    if h.rows is None:
        return g1_infinity_jac(G, "cpu")
    S_w = h.rows.cpu()                                                   # [len(gws), 24]
    # Horner over the windows, all groups at once: acc = 2^8 acc + S_{g,w}.
    # ~8 doublings per window and group, instead of one up-to-248-doubling
    # multiplication 2^{8w} S_{g,w} per (group, window)
    rows = g1_infinity_jac(G * W, "cpu")
    rows[torch.from_numpy(gws.astype(np.int64))] = S_w
    rows = rows.view(G, W, 24)
    top = int((gws % W).max())
    out = torch.empty((G, 24), dtype=torch.int32)
    src = rows[:, : top + 1].contiguous()  # held: the host call reads it
    rc = _raw_call("dx_g1_horner_host", _ptr(src), _ptr(out), G, top + 1, 8)
    if rc:
        raise RuntimeError(f"dx_g1_horner_host failed rc={rc}")
    return out


# ----------------------------------------------------------------------------- G2 MSM (verifier mode "msm")
# csrc/kernels/dx_rpmsm.hip: range-proof batch verification by bilinearity
def g2_msm_launch(P_aff: torch.Tensor, k: torch.Tensor, group: torch.Tensor | None, n_groups: int,
                  c: int = 13, bits: int = 254, first_slice: int = 32) -> CountedPlan:
    """Bucket plan of G independent G2 MSMs out[g] = sum_{t: group_t = g}
    k_t P[t % m] (m = rows of P_aff, k [n, 8] with n a multiple of m; group:
    int32 tensor, or an int stride s meaning group_t = t // s) over c-bit
    windows, with its bucket weights -- ONE host sync (the counts).
    ``g2_msm_run`` queues the device passes."""
    assert k.shape[0] % _rows(P_aff, 32) == 0
    return _counted_plan(k, group, n_groups, -(-bits // c), c, ChunkWeights, first_slice)


def g2_msm_run(P_aff: torch.Tensor, h: CountedPlan) -> torch.Tensor:
    """Device passes of a ``g2_msm_launch`` plan, queued on the current stream:
    bucket sums, weights d B_d, per-(group, window) sums -> [G * W, 48]
    Jacobian window sums (``g2_msm_finish`` combines them)."""
    S = torch.zeros((h.G * h.W, 48), dtype=torch.int32, device=P_aff.device)     # Jacobian infinity = Z 0
    if h.weights is not None:
        B = _reduce(h.passes, _g2_ops(P_aff, h.item, _rows(P_aff, 32)))
        h.weights.weigh(B, g2_chunk_weight, _g2_jac_sum, S)
    return S


def g2_msm_device(P_aff: torch.Tensor, k: torch.Tensor, group, groups: tuple, c: int = 13,
                  bits: int = 254) -> tuple:
    """``g2_msm_launch`` + ``g2_msm_run`` with a device-resident plan (no host
    sync): out[g] = sum_{t: group_t = g} k_t P[t % m] -> ([G * W, 48] window
    sums, handle for ``g2_msm_finish``)."""
    G = len(groups)
    W = -(-bits // c)
    B, lay, overflow = _device_buckets(k, group, groups, W, c, 32, ChunkWeights,
                                       lambda items: _g2_ops(P_aff, items, _rows(P_aff, 32)))
    S = torch.zeros((G * W, 48), dtype=torch.int32, device=P_aff.device)
    return lay.weights.weigh(B, g2_chunk_weight, _g2_jac_sum, S), Handle(G, W, c, overflow=overflow)


def g2_msm_finish(S: torch.Tensor, h: CountedPlan | Handle, out_aff: torch.Tensor | None = None, stride: int = 1,
                  offset: int = 0) -> torch.Tensor:
    """Horner over the windows, one lane per group (W*c doublings), on the
    tensor's device: out_aff[g * stride + offset] = affine(out[g]).  On the
    host (CPU tensors) a core runs this serial chain ~5x faster than one GPU lane."""
    G, W, c = h.G, h.W, h.c
    if out_aff is None:
        out_aff = torch.zeros((G, 32), dtype=torch.int32, device=S.device)
    g, s = _ctx(S, out_aff)
    _call("dx_g2_horner", g, s, _ptr(S.contiguous()), _ptr(out_aff), G, W, c, stride, offset)
    return out_aff


def rp_msm_uv(Y_jac: torch.Tensor, UV: torch.Tensor, n_groups: int, G: int, pad: int) -> torch.Tensor:
    """UV[v*pad + q] = (x/y, 1/y) of -Y_q (q < n_groups) and of B (q = n_groups)."""
    assert _rows(Y_jac, 24) == n_groups and _rows(UV, 16) >= (G - 1) * pad + n_groups + 1 and pad > n_groups
    g, s = _ctx(Y_jac, UV)
    _call("dx_rp_msm_uv", g, s, _ptr(Y_jac.contiguous()), _ptr(UV), n_groups, G, pad)
    return UV
