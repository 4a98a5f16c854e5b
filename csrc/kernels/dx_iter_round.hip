// K14b / K14c: one round of an iterative (digit-by-digit) query -- min, max or
// frequencyCount -- all DPs of a rank in two launches.
//
// The one-shot encodings send one value per element of the domain [QueryMin,
// QueryMax].  The iterative query asks for the result one base-b digit at a
// time: with R = QueryMax - QueryMin + 1 and L the smallest integer with
// b^L >= R, round k carries the prefix p of the k digits found so far.  With
// lo = b^(L-1-k) and hi = b^(L-k) = b * lo, an offset o = x - QueryMin lies
// under the prefix iff o div hi == p, and its digit is (o div lo) mod b.  One
// division decides both: q = o div lo lies in [p*b, p*b + b) iff o div hi == p,
// and then q - p*b is the digit (round_digit below).
//
// min / max (K14b): a DP whose extreme e, CLAMPED to the domain, lies under
// the prefix answers with its digit v, every other DP (and a DP without
// records) with the neutral value (0 for max, b for min), and the b values it
// encrypts are the unary encoding of v over [0, b-1]:
//
//     max: out[i] = [i < v]        min: out[i] = [i >= v]
//
// frequencyCount (K14c, the rounds of a quantile search): a DP answers with
// the b counts
//
//     out[d] = #{ records x in the domain under the prefix with digit d }.
//
// Records outside the domain are DROPPED (not clamped), as the one-shot
// histogram drops them.
//
// The records of every DP of the rank are stacked in one int64 matrix Z (DP g
// owns a row range; only column 0 is read, row stride ldz).
//
// Stage 1: one 256-thread workgroup per tile of the host-made plan (a row
// range of one DP, as K14's), streaming the tile's records with coalesced
// 64-bit loads.  min / max: reduce across the 64 lanes of a wave with
// __shfl_xor, across the four waves through LDS, and store ONE partial per
// tile.  Counts: tiles have at least max(64, b) rows but for a DP's last tile,
// so the partials are never larger than the records they summarise; the
// workgroup zeroes b 32-bit counters in LDS, adds every matching record to its
// counter with one LDS atomic, and after a barrier stores the b counters as
// int64 to partial[tile][0..b), coalesced.
// Stage 2, min / max: one workgroup per DP reduces the DP's partials (its tile
// range), clamps, takes the round's digit, applies match / neutral and writes
// the b-value row coalesced.  Counts: grid (G, ceil(b / 256)), one thread per
// (DP, bin) sums the bin over the DP's consecutive tiles and writes out[g][bin].
// The hand-off between the stages is the launch boundary: no global atomics,
// no counters, no fences, no zeroed state.  Host path: the same two stages on
// the thread pool.
//
// K14e (dx_iter_round_cells): the counts of a round per cell of a SQL WHERE /
// GROUP BY, every cell under a prefix of its own (G simultaneous searches):
//
//     out[dp][g][d] = #{ rows i of DP dp : row_group(i) == g, qmin <= x_i <= qmax,
//                        (x_i - qmin) div hi == prefix[g], d == ((x_i - qmin) div lo) mod b }
//
// row_group is K14d's membership rule, the very function (group_terms.h: the
// conjunction of equalities or a predicate over compared atoms, then the key); x_i
// is column xcol of the key matrix K [rows][CK], read in place through its row
// stride.  GPU: one 256-thread workgroup per tile of the host-made plan, the
// tile's rows streamed with coalesced 64-bit loads, a row's group computed
// once.  The counters live in LDS, one 32-bit counter per (group of the
// window, digit): a launch covers the window [g0, g0 + gw) of consecutive
// groups with gw * b <= kMaxCounters and ignores rows whose group falls outside
// it (the binding loops over the windows, as K14d's does).  kMaxCounters is
// half of a CU's 160 KiB of LDS, so two workgroups stay resident; the LDS is
// sized per launch, so a small window leaves room for more.  A counted row
// costs one LDS atomic.  The window's prefixes are READ THROUGH THE CACHE, one
// 64-bit load per row that has a group and lies in the domain: staged in LDS
// they would take 8 bytes beside the 4 * b bytes of a group's counters and
// halve the window at small bases, while the at most 80 KiB of a window's
// prefixes are read-only, shared by every workgroup and stay in L2.  After a
// barrier the non-zero counters go to the caller-zeroed out with one 64-bit
// global (vector) atomic each, as in K14d: a per-tile slab of gw * b partials
// would be larger than the records it summarises, so K14c's second stage does
// not carry over; integer adds do not depend on the order of tiles or atomics,
// and there is no global state beyond out.  The binding's tiles stream at least
// min(min(G, gw) * b, 2048) rows, so zeroing and flushing never outweigh the
// records, and a tile stays below 2^31 rows for the 32-bit counters.
// Memory safety does not depend on the prefixes, which the entry cannot read on
// the device: a prefix is only ever COMPARED with the quotient o div hi, and the
// counter index is g * b + (q - (q div b) * b) with q = o div lo, inside
// [0, gw * b) whatever the prefix holds.  Host path: the same tiles on the
// thread pool, adding to out with relaxed atomic adds -- bit-identical.
#include "exec.h"
#include "group_terms.h"

namespace {
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int64_t kMaxBase = 65536;
constexpr int64_t kMaxHistBase = 4096;  // 16 KiB of LDS counters
constexpr int64_t kMaxRange = (int64_t)1 << 40;
enum Kind { kKindMin = 0, kKindMax = 1, kKindCounts = 2 };

struct RoundArgs {
  const int64_t *Z;
  int64_t ldz;
  const int64_t *tiles;     // [n_tiles][3] = (dp, row0, row1)
  const int64_t *dp_first;  // [G + 1]: DP g owns tiles dp_first[g] .. dp_first[g + 1]
  int64_t *partial;         // min / max: [n_tiles]; counts: [n_tiles][base]
  int64_t *out;             // [G][base]
  int64_t qmin, qmax, base, lo, pb;  // lo = b^(L-1-k), pb = prefix * b
};

// The digit of the in-domain offset o (0 .. R-1 < 2^40) in this round, -1 if o
// is not under the prefix.
__host__ __device__ inline int64_t round_digit(const RoundArgs &a, uint64_t o) {
  const int64_t d = (int64_t)(o / (uint64_t)a.lo) - a.pb;
  return d >= 0 && d < a.base ? d : -1;
}

// ---------------------------------------------------------------- min / max
template <bool kMax>
__host__ __device__ inline int64_t ext_identity() {
  return kMax ? INT64_MIN : INT64_MAX;
}

template <bool kMax>
__host__ __device__ inline int64_t ext_pick(int64_t a, int64_t b) {
  return kMax ? (a > b ? a : b) : (a < b ? a : b);
}

// The round value of a DP whose extreme over its records is e (has = it has records).
template <bool kMax>
__host__ __device__ inline int64_t round_value(const RoundArgs &a, bool has, int64_t e) {
  const int64_t neutral = kMax ? 0 : a.base;
  if (!has) return neutral;
  e = e < a.qmin ? a.qmin : (e > a.qmax ? a.qmax : e);
  const int64_t d = round_digit(a, (uint64_t)e - (uint64_t)a.qmin);
  return d < 0 ? neutral : d;
}

template <bool kMax>
__host__ __device__ inline int64_t unary_bit(int64_t i, int64_t v) {
  return kMax ? (int64_t)(i < v) : (int64_t)(i >= v);
}

// All 256 threads call it; the result is valid in every thread.
template <bool kMax>
__device__ inline int64_t block_reduce(int64_t x, int64_t *lds) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = ext_pick<kMax>(x, (int64_t)__shfl_xor((long long)x, m, 64));
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
  __syncthreads();
  int64_t r = lds[0];
#pragma unroll
  for (int w = 1; w < kWaves; w++) r = ext_pick<kMax>(r, lds[w]);
  return r;
}

template <bool kMax>
__global__ void __launch_bounds__(kThreads) extreme_tiles_kernel(RoundArgs a) {
  __shared__ int64_t lds[kWaves];
  const int64_t r0 = a.tiles[3 * (int64_t)blockIdx.x + 1], r1 = a.tiles[3 * (int64_t)blockIdx.x + 2];
  int64_t x = ext_identity<kMax>();
  for (int64_t r = r0 + threadIdx.x; r < r1; r += kThreads) x = ext_pick<kMax>(x, a.Z[r * a.ldz]);
  x = block_reduce<kMax>(x, lds);
  if (threadIdx.x == 0) a.partial[blockIdx.x] = x;
}

template <bool kMax>
__global__ void __launch_bounds__(kThreads) extreme_rows_kernel(RoundArgs a) {
  __shared__ int64_t lds[kWaves];
  const int64_t g = blockIdx.x;
  const int64_t t0 = a.dp_first[g], t1 = a.dp_first[g + 1];
  int64_t x = ext_identity<kMax>();
  for (int64_t t = t0 + threadIdx.x; t < t1; t += kThreads) x = ext_pick<kMax>(x, a.partial[t]);
  x = block_reduce<kMax>(x, lds);
  const int64_t v = round_value<kMax>(a, t1 > t0, x);
  int64_t *row = a.out + g * a.base;
  for (int64_t i = threadIdx.x; i < a.base; i += kThreads) row[i] = unary_bit<kMax>(i, v);
}

template <bool kMax>
void host_extreme(const RoundArgs &a, int64_t n_tiles, int64_t G) {
  dx::host_for_each(n_tiles, [=](int64_t t) {
    int64_t x = ext_identity<kMax>();
    for (int64_t r = a.tiles[3 * t + 1]; r < a.tiles[3 * t + 2]; r++) x = ext_pick<kMax>(x, a.Z[r * a.ldz]);
    a.partial[t] = x;
  });
  dx::host_for_each(G, [=](int64_t g) {
    const int64_t t0 = a.dp_first[g], t1 = a.dp_first[g + 1];
    int64_t x = ext_identity<kMax>();
    for (int64_t t = t0; t < t1; t++) x = ext_pick<kMax>(x, a.partial[t]);
    const int64_t v = round_value<kMax>(a, t1 > t0, x);
    int64_t *row = a.out + g * a.base;
    for (int64_t i = 0; i < a.base; i++) row[i] = unary_bit<kMax>(i, v);
  });
}

// ---------------------------------------------------------------- counts
// The bin of record x in this round, -1 if it does not count.
__host__ __device__ inline int64_t hist_bin(const RoundArgs &a, int64_t x) {
  if (x < a.qmin || x > a.qmax) return -1;
  return round_digit(a, (uint64_t)x - (uint64_t)a.qmin);
}

__global__ void __launch_bounds__(kThreads) hist_tiles_kernel(RoundArgs a) {
  __shared__ unsigned int cnt[kMaxHistBase];
  const int b = (int)a.base;
  for (int i = threadIdx.x; i < b; i += kThreads) cnt[i] = 0;
  __syncthreads();
  const int64_t r0 = a.tiles[3 * (int64_t)blockIdx.x + 1], r1 = a.tiles[3 * (int64_t)blockIdx.x + 2];
  for (int64_t r = r0 + threadIdx.x; r < r1; r += kThreads) {
    const int64_t d = hist_bin(a, a.Z[r * a.ldz]);
    if (d >= 0) atomicAdd(&cnt[d], 1u);
  }
  __syncthreads();
  int64_t *row = a.partial + (int64_t)blockIdx.x * a.base;
  for (int i = threadIdx.x; i < b; i += kThreads) row[i] = (int64_t)cnt[i];
}

__global__ void __launch_bounds__(kThreads) hist_rows_kernel(RoundArgs a) {
  const int64_t g = blockIdx.x;
  const int64_t bin = (int64_t)blockIdx.y * kThreads + threadIdx.x;
  if (bin >= a.base) return;
  int64_t s = 0;
  for (int64_t t = a.dp_first[g]; t < a.dp_first[g + 1]; t++) s += a.partial[t * a.base + bin];
  a.out[g * a.base + bin] = s;
}

void host_hist(const RoundArgs &a, int64_t n_tiles, int64_t G) {
  dx::host_for_each(n_tiles, [=](int64_t t) {
    int64_t *row = a.partial + t * a.base;
    for (int64_t i = 0; i < a.base; i++) row[i] = 0;
    for (int64_t r = a.tiles[3 * t + 1]; r < a.tiles[3 * t + 2]; r++) {
      const int64_t d = hist_bin(a, a.Z[r * a.ldz]);
      if (d >= 0) row[d]++;
    }
  });
  dx::host_for_each(G, [=](int64_t g) {
    int64_t *row = a.out + g * a.base;
    for (int64_t i = 0; i < a.base; i++) row[i] = 0;
    for (int64_t t = a.dp_first[g]; t < a.dp_first[g + 1]; t++)
      for (int64_t i = 0; i < a.base; i++) row[i] += a.partial[t * a.base + i];
  });
}

// ---------------------------------------------------------------- both
// The two launches of a round: `tiles` over the plan's tiles (none for a plan
// without tiles), then `rows` over `rows_grid`.
template <class Tiles, class Rows>
int launch_round(void *stream, const RoundArgs &a, int64_t n_tiles, Tiles tiles, const char *tiles_name, Rows rows,
                 dim3 rows_grid, const char *rows_name) {
  hipStream_t s = (hipStream_t)stream;
  if (n_tiles > 0) {
    hipLaunchKernelGGL(tiles, dim3((unsigned)n_tiles), dim3(kThreads), 0, s, a);
    if (int rc = dx::check_hip(hipGetLastError(), tiles_name)) return rc;
  }
  hipLaunchKernelGGL(rows, rows_grid, dim3(kThreads), 0, s, a);
  return dx::check_hip(hipGetLastError(), rows_name);
}

template <bool kMax>
int run_extreme(int on_gpu, void *stream, const RoundArgs &a, int64_t n_tiles, int64_t G) {
  if (on_gpu)
    return launch_round(stream, a, n_tiles, extreme_tiles_kernel<kMax>, "extreme_tiles", extreme_rows_kernel<kMax>,
                        dim3((unsigned)G), "extreme_rows");
  host_extreme<kMax>(a, n_tiles, G);
  return 0;
}

int run_hist(int on_gpu, void *stream, const RoundArgs &a, int64_t n_tiles, int64_t G) {
  if (on_gpu)
    return launch_round(stream, a, n_tiles, hist_tiles_kernel, "digit_hist_tiles", hist_rows_kernel,
                        dim3((unsigned)G, (unsigned)((a.base + kThreads - 1) / kThreads)), "digit_hist_rows");
  host_hist(a, n_tiles, G);
  return 0;
}

// Is (base, lo, prefix) a round of the domain [qmin, qmax] for this kind, and
// are the counts within the grid limits?
bool is_round(int kind, int64_t n_tiles, int64_t G, int64_t qmin, int64_t qmax, int64_t base, int64_t lo,
              int64_t prefix) {
  if (kind < kKindMin || kind > kKindCounts) return false;
  if (G < 0 || n_tiles < 0 || n_tiles > 0x7fffffff || G > 0x7fffffff || qmax < qmin) return false;
  if (base < 2 || base > (kind == kKindCounts ? kMaxHistBase : kMaxBase)) return false;
  const uint64_t R = (uint64_t)qmax - (uint64_t)qmin + 1;
  if (R < 1 || R > (uint64_t)kMaxRange) return false;
  int64_t top = base;  // b^L <= b * 2^40 = 2^56
  while ((uint64_t)top < R) top *= base;
  // lo = b^(L-1-k) for some 0 <= k < L, 0 <= prefix < b^k = b^L / (b * lo)
  bool found = false;
  for (int64_t pw = 1; pw < top; pw *= base) found = found || pw == lo;
  return found && prefix >= 0 && prefix < top / (lo * base);
}
}  // namespace

// kind 0 = min, 1 = max, 2 = counts.  tiles [n_tiles][3] and dp_first [G + 1]
// describe the same plan: the tiles of DP g are consecutive.  partial is
// scratch ([n_tiles] for min / max, [n_tiles][base] for counts), out [G][base]
// the rows.  lo is b^(L-1-k) of round k: the entry recovers k from it and
// refuses anything that is not a round of this domain, for every kind.  For
// counts a host plan is also checked for the tile length the 32-bit counters
// allow (a plan in device memory is the binding's to check).
extern "C" int dx_iter_round(int on_gpu, void *stream, const int64_t *Z, int64_t ldz, const int64_t *tiles,
                             int64_t n_tiles, const int64_t *dp_first, int64_t G, int kind, int64_t qmin,
                             int64_t qmax, int64_t base, int64_t lo, int64_t prefix, int64_t *partial, int64_t *out) {
  if (!is_round(kind, n_tiles, G, qmin, qmax, base, lo, prefix)) return -2;
  if (kind == kKindCounts && !on_gpu)
    for (int64_t t = 0; t < n_tiles; t++)
      if (tiles[3 * t + 2] - tiles[3 * t + 1] > 0x7fffffff) return -2;
  if (G == 0) return 0;
  RoundArgs a{Z, ldz, tiles, dp_first, partial, out, qmin, qmax, base, lo, prefix * base};
  if (kind == kKindCounts) return run_hist(on_gpu, stream, a, n_tiles, G);
  return kind == kKindMax ? run_extreme<true>(on_gpu, stream, a, n_tiles, G)
                          : run_extreme<false>(on_gpu, stream, a, n_tiles, G);
}

// ---------------------------------------------------------------- cells (K14e)
namespace {
constexpr int kLdsPerCU = 160 * 1024;
constexpr int kMaxCounters = kLdsPerCU / 2 / 4;  // 20480 32-bit counters of one launch
constexpr int64_t kMaxCellOutputs = (int64_t)1 << 20;  // G * b of a query (rounds.ITER_MAX_CELL_OUTPUTS)
static_assert(kMaxCounters >= kMaxHistBase, "one group of the largest base fits a window");
static_assert(kMaxCounters * 4 <= kLdsPerCU / 2, "two workgroups per CU");

struct CellArgs : dx::GroupTerms {  // G groups: out is [n_dp][G][base], zeroed by the caller
  const int64_t *K;
  int64_t ldk;
  int xcol;
  const int64_t *tiles;   // [n_tiles][3] = (dp, row0, row1)
  const int64_t *prefix;  // [G], in the memory K lives in; never trusted
  int64_t qmin, qmax, base, lo;
  int64_t *out;
};

// The counter (window-relative group * base + digit) of the row whose columns
// are krow and whose group (row_group) is g, -1 if the row does not count.
__host__ __device__ inline int cell_counter(const CellArgs &a, const int64_t *krow, int g) {
  if (g < 0) return -1;
  const int64_t x = krow[a.xcol];
  if (x < a.qmin || x > a.qmax) return -1;
  const uint64_t q = ((uint64_t)x - (uint64_t)a.qmin) / (uint64_t)a.lo;  // o div lo
  const uint64_t p = q / (uint64_t)a.base;                                // o div hi, hi = lo * b
  if ((int64_t)p != a.prefix[a.g0 + g]) return -1;                        // p < 2^40: a compare, no arithmetic
  return g * (int)a.base + (int)(q - p * (uint64_t)a.base);
}

template <bool General>  // a.general: the WHERE is a predicate (group_terms.h)
__global__ void __launch_bounds__(kThreads) cell_hist_kernel(CellArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned int cell_cnt[];  // [gw][base]
  const int n = a.gw * (int)a.base;
  for (int i = threadIdx.x; i < n; i += kThreads) cell_cnt[i] = 0;
  __syncthreads();
  const int64_t dp = a.tiles[3 * (int64_t)blockIdx.x], r0 = a.tiles[3 * (int64_t)blockIdx.x + 1],
                r1 = a.tiles[3 * (int64_t)blockIdx.x + 2];
  for (int64_t r = r0 + threadIdx.x; r < r1; r += kThreads) {
    const int64_t *krow = a.K + r * a.ldk;
    const int c = cell_counter(a, krow, dx::row_group<General>(a, krow));
    if (c >= 0) atomicAdd(&cell_cnt[c], 1u);
  }
  __syncthreads();
  unsigned long long *o = reinterpret_cast<unsigned long long *>(a.out) + (dp * a.G + a.g0) * a.base;
  for (int i = threadIdx.x; i < n; i += kThreads)
    if (cell_cnt[i]) atomicAdd(o + i, (unsigned long long)cell_cnt[i]);
}

void host_cell_hist(const CellArgs &a, int64_t n_tiles) {
  dx::host_for_each(n_tiles, [=](int64_t t) {
    const int64_t dp = a.tiles[3 * t], r0 = a.tiles[3 * t + 1], r1 = a.tiles[3 * t + 2];
    uint64_t *o = reinterpret_cast<uint64_t *>(a.out) + (dp * a.G + a.g0) * a.base;
    for (int64_t r = r0; r < r1; r++) {
      const int64_t *krow = a.K + r * a.ldk;
      const int c = cell_counter(a, krow, dx::row_group(a, krow));
      if (c >= 0) __atomic_fetch_add(o + c, (uint64_t)1, __ATOMIC_RELAXED);
    }
  });
}

// One window on the device.  The LDS limit of a kernel is raised once, to the
// largest window, not per launch.
template <bool General>
int launch_cell_hist(const CellArgs &a, int64_t n_tiles, size_t bytes, void *stream) {
  static const int lds_rc = dx::check_hip(
      hipFuncSetAttribute(reinterpret_cast<const void *>(cell_hist_kernel<General>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, kMaxCounters * 4),
      "iter_round_cells (LDS size)");
  if (lds_rc) return lds_rc;
  hipLaunchKernelGGL(cell_hist_kernel<General>, dim3((unsigned)n_tiles), dim3(kThreads), bytes, (hipStream_t)stream, a);
  return dx::check_hip(hipGetLastError(), "iter_round_cells");
}
}  // namespace

extern "C" int dx_iter_round_max_counters() { return kMaxCounters; }

// One window of the grouped counts of a round.  keys [n_keys][3], filters
// [n_filters][2] and pred (NULL or the operators and the truth table) are
// K14d's HOST arrays over K [rows][CK] (at most 4 keys: the counted column
// xcol is not one of them), prefix [G] lives with K.  out
// [n_dp][G][base] is zeroed by the caller before the first window; this call
// adds the groups [g0, g0 + gw).  lo is b^(L-1-k) of round k, as dx_iter_round
// takes it.  Everything that can be checked without reading device memory is
// checked here -- the terms (the shared checker), xcol, the round, G * base, the
// window, the counts, and on a host plan the tile length the 32-bit counters
// allow: an argument that does not fit returns -2 and launches nothing.
extern "C" int dx_iter_round_cells_pred(int on_gpu, void *stream, const int64_t *K, int64_t ldk, int CK,
                                        int64_t xcol, const int64_t *tiles, int64_t n_tiles, const int64_t *keys,
                                        int n_keys, const int64_t *filters, int n_filters, int64_t qmin, int64_t qmax,
                                        int64_t base, int64_t lo, const int64_t *prefix, int64_t g0, int64_t gw,
                                        int64_t *out, const int64_t *pred) {
  CellArgs a{};
  if (n_keys >= dx::kMaxKeys || !dx::set_terms(a, CK, keys, n_keys, filters, n_filters, pred)) return -2;
  if (xcol < 0 || xcol >= CK) return -2;
  if (!is_round(kKindCounts, n_tiles, 0, qmin, qmax, base, lo, 0)) return -2;
  if (a.G * base > kMaxCellOutputs) return -2;
  if (g0 < 0 || gw < 1 || g0 + gw > a.G || gw * base > kMaxCounters) return -2;
  if (!on_gpu)
    for (int64_t t = 0; t < n_tiles; t++)
      if (tiles[3 * t + 2] - tiles[3 * t + 1] > 0x7fffffff) return -2;
  if (n_tiles == 0) return 0;
  a.K = K, a.ldk = ldk, a.xcol = (int)xcol, a.tiles = tiles, a.prefix = prefix;
  a.qmin = qmin, a.qmax = qmax, a.base = base, a.lo = lo, a.g0 = g0, a.gw = (int)gw, a.out = out;
  if (!on_gpu) {
    host_cell_hist(a, n_tiles);
    return 0;
  }
  const size_t bytes = (size_t)gw * (size_t)base * 4;
  return a.general ? launch_cell_hist<true>(a, n_tiles, bytes, stream)
                   : launch_cell_hist<false>(a, n_tiles, bytes, stream);
}

// pred == NULL under the signature the entry had before predicates
extern "C" int dx_iter_round_cells(int on_gpu, void *stream, const int64_t *K, int64_t ldk, int CK, int64_t xcol,
                                   const int64_t *tiles, int64_t n_tiles, const int64_t *keys, int n_keys,
                                   const int64_t *filters, int n_filters, int64_t qmin, int64_t qmax, int64_t base,
                                   int64_t lo, const int64_t *prefix, int64_t g0, int64_t gw, int64_t *out) {
  return dx_iter_round_cells_pred(on_gpu, stream, K, ldk, CK, xcol, tiles, n_tiles, keys, n_keys, filters, n_filters,
                                  qmin, qmax, base, lo, prefix, g0, gw, out, nullptr);
}
