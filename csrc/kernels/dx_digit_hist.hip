// K14c: one round of the iterative (digit-by-digit) frequencyCount query, all
// DPs of a rank in two launches.
//
// The one-shot frequencyCount sends one count per element of the domain
// [QueryMin, QueryMax].  A quantile search asks for the histogram one base-b
// digit at a time: with R = QueryMax - QueryMin + 1 and L the smallest integer
// with b^L >= R, round k carries the prefix p of the k digits found so far and
// a DP answers with the b counts
//
//     out[d] = #{ records x in the domain : o div b^(L-k) == p and
//                                           (o div b^(L-1-k)) mod b == d },  o = x - QueryMin.
//
// Records outside the domain are dropped (not clamped), as the one-shot
// histogram drops them.  With hi = b^(L-k) = b * lo one division decides both
// conditions: q = o div lo lies in [p*b, p*b + b) iff o div hi == p, and then
// q - p*b is the digit.
//
// The records of every DP of the rank are stacked in one int64 matrix Z (DP g
// owns a row range; only column 0 is read, row stride ldz).
//
// Stage 1: one 256-thread workgroup per tile of the host-made plan (a row
// range of one DP, as K14b's, of at least max(64, b) rows but for a DP's last
// tile, so the partials are never larger than the records they summarise).
// The workgroup zeroes b 32-bit counters in LDS, streams the tile's records
// with coalesced 64-bit loads, adds every matching record to its counter with
// one LDS atomic, and after a barrier stores the b counters as int64 to
// partial[tile][0..b), coalesced.  Stage 2: grid (G, ceil(b / 256)), one
// thread per (DP, bin) sums the bin over the DP's consecutive tiles and writes
// out[g][bin].  The hand-off between the stages is the launch boundary: no
// global atomics, no counters, no fences, no zeroed state.  Host path: the
// same two stages on the thread pool.
#include "exec.h"

namespace {
constexpr int kThreads = 256;
constexpr int64_t kMaxBase = 4096;  // 16 KiB of LDS counters
constexpr int64_t kMaxRange = (int64_t)1 << 40;

struct HistArgs {
  const int64_t *Z;
  int64_t ldz;
  const int64_t *tiles;     // [n_tiles][3] = (dp, row0, row1)
  const int64_t *dp_first;  // [G + 1]: DP g owns tiles dp_first[g] .. dp_first[g + 1]
  int64_t *partial;         // [n_tiles][base]
  int64_t *out;             // [G][base]
  int64_t qmin, qmax, base, lo, pb;  // lo = b^(L-1-k), pb = prefix * b
};

// The bin of record x in this round, -1 if it does not count.
__host__ __device__ inline int64_t hist_bin(const HistArgs &a, int64_t x) {
  if (x < a.qmin || x > a.qmax) return -1;
  const uint64_t o = (uint64_t)x - (uint64_t)a.qmin;  // 0 .. R-1 < 2^40
  const int64_t d = (int64_t)(o / (uint64_t)a.lo) - a.pb;
  return d >= 0 && d < a.base ? d : -1;
}

__global__ void __launch_bounds__(kThreads) hist_tiles_kernel(HistArgs a) {
  __shared__ unsigned int cnt[kMaxBase];
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

__global__ void __launch_bounds__(kThreads) hist_rows_kernel(HistArgs a) {
  const int64_t g = blockIdx.x;
  const int64_t bin = (int64_t)blockIdx.y * kThreads + threadIdx.x;
  if (bin >= a.base) return;
  int64_t s = 0;
  for (int64_t t = a.dp_first[g]; t < a.dp_first[g + 1]; t++) s += a.partial[t * a.base + bin];
  a.out[g * a.base + bin] = s;
}

int run_hist(int on_gpu, void *stream, const HistArgs &a, int64_t n_tiles, int64_t G) {
  if (on_gpu) {
    hipStream_t s = (hipStream_t)stream;
    if (n_tiles > 0) {
      hipLaunchKernelGGL(hist_tiles_kernel, dim3((unsigned)n_tiles), dim3(kThreads), 0, s, a);
      if (int rc = dx::check_hip(hipGetLastError(), "digit_hist_tiles")) return rc;
    }
    const unsigned by = (unsigned)((a.base + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(hist_rows_kernel, dim3((unsigned)G, by), dim3(kThreads), 0, s, a);
    return dx::check_hip(hipGetLastError(), "digit_hist_rows");
  }
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
  return 0;
}
}  // namespace

// tiles [n_tiles][3] and dp_first [G + 1] describe the same plan: the tiles of
// DP g are consecutive.  partial [n_tiles][base] is scratch, out [G][base] the
// rows.  hi and lo are b^(L-k) and b^(L-1-k) of round k: the entry recovers k
// from them and refuses anything that is not a round of this domain.  A host
// plan is also checked for the tile length the 32-bit counters allow (a plan
// in device memory is the binding's to check).
extern "C" int dx_digit_histogram(int on_gpu, void *stream, const int64_t *Z, int64_t ldz, const int64_t *tiles,
                                  int64_t n_tiles, const int64_t *dp_first, int64_t G, int64_t qmin, int64_t qmax,
                                  int64_t base, int64_t hi, int64_t lo, int64_t prefix, int64_t *partial,
                                  int64_t *out) {
  if (G < 0 || n_tiles < 0 || n_tiles > 0x7fffffff || G > 0x7fffffff || base < 2 || base > kMaxBase || qmax < qmin)
    return -2;
  const uint64_t R = (uint64_t)qmax - (uint64_t)qmin + 1;
  if (R < 1 || R > (uint64_t)kMaxRange) return -2;
  int64_t top = base;  // b^L <= b * 2^40 = 2^52
  while ((uint64_t)top < R) top *= base;
  // lo = b^(L-1-k) for some 0 <= k < L, hi = b * lo, 0 <= prefix < b^k = b^L / hi
  bool is_round = false;
  for (int64_t pw = 1; pw < top; pw *= base) is_round = is_round || pw == lo;
  if (!is_round || hi != lo * base || prefix < 0 || prefix >= top / hi) return -2;
  if (!on_gpu)
    for (int64_t t = 0; t < n_tiles; t++)
      if (tiles[3 * t + 2] - tiles[3 * t + 1] > 0x7fffffff) return -2;
  if (G == 0) return 0;
  HistArgs a{Z, ldz, tiles, dp_first, partial, out, qmin, qmax, base, lo, prefix * base};
  return run_hist(on_gpu, stream, a, n_tiles, G);
}
