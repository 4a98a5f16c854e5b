// K14b: one round of the iterative (digit-by-digit) min/max query, all DPs of
// a rank in two launches.
//
// The unary min/max encoding sends one value per element of the domain
// [QueryMin, QueryMax].  The iterative query asks for the result one base-b
// digit at a time: with R = QueryMax - QueryMin + 1 and L the smallest integer
// with b^L >= R, round k carries the prefix p of the k digits found so far.  A
// DP whose clamped extreme e has o = e - QueryMin with o div b^(L-k) == p
// answers with its digit v = (o div b^(L-1-k)) mod b, every other DP (and a DP
// without records) with the neutral value (0 for max, b for min), and the b
// values it encrypts are the unary encoding of v over [0, b-1]:
//
//     max: out[i] = [i < v]        min: out[i] = [i >= v]
//
// The records of every DP of the rank are stacked in one int64 matrix Z (DP g
// owns a row range; only column 0 is read, row stride ldz).
//
// Stage 1: one 256-thread workgroup per tile of the host-made plan (a row
// range of one DP, as K14's).  The threads stream the tile's records with
// coalesced 64-bit loads, reduce across the 64 lanes of a wave with
// __shfl_xor, across the four waves through LDS, and store ONE partial per
// tile.  Stage 2: one workgroup per DP reduces the DP's partials (its tile
// range), clamps, takes the two quotients by the host-computed powers, applies
// match / neutral and writes the b-value row coalesced.  The hand-off between
// the stages is the launch boundary: no counters, no fences, no zeroed state.
// Host path: the same two stages on the thread pool.
#include "exec.h"

namespace {
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

struct ExtArgs {
  const int64_t *Z;
  int64_t ldz;
  const int64_t *tiles;     // [n_tiles][3] = (dp, row0, row1)
  const int64_t *dp_first;  // [G + 1]: DP g owns tiles dp_first[g] .. dp_first[g + 1]
  int64_t *partial;         // [n_tiles]
  int64_t *out;             // [G][base]
  int64_t qmin, qmax, base, hi, lo, prefix;  // hi = b^(L-k), lo = b^(L-1-k)
};

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
__host__ __device__ inline int64_t round_value(const ExtArgs &a, bool has, int64_t e) {
  const int64_t neutral = kMax ? 0 : a.base;
  if (!has) return neutral;
  e = e < a.qmin ? a.qmin : (e > a.qmax ? a.qmax : e);
  const int64_t o = (int64_t)((uint64_t)e - (uint64_t)a.qmin);  // 0 .. R-1 <= 2^40
  if (o / a.hi != a.prefix) return neutral;
  return (o / a.lo) % a.base;
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
__global__ void __launch_bounds__(kThreads) extreme_tiles_kernel(ExtArgs a) {
  __shared__ int64_t lds[kWaves];
  const int64_t r0 = a.tiles[3 * (int64_t)blockIdx.x + 1], r1 = a.tiles[3 * (int64_t)blockIdx.x + 2];
  int64_t x = ext_identity<kMax>();
  for (int64_t r = r0 + threadIdx.x; r < r1; r += kThreads) x = ext_pick<kMax>(x, a.Z[r * a.ldz]);
  x = block_reduce<kMax>(x, lds);
  if (threadIdx.x == 0) a.partial[blockIdx.x] = x;
}

template <bool kMax>
__global__ void __launch_bounds__(kThreads) extreme_rows_kernel(ExtArgs a) {
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
int run_extreme(int on_gpu, void *stream, const ExtArgs &a, int64_t n_tiles, int64_t G) {
  if (on_gpu) {
    hipStream_t s = (hipStream_t)stream;
    if (n_tiles > 0) {
      hipLaunchKernelGGL(extreme_tiles_kernel<kMax>, dim3((unsigned)n_tiles), dim3(kThreads), 0, s, a);
      if (int rc = dx::check_hip(hipGetLastError(), "extreme_tiles")) return rc;
    }
    hipLaunchKernelGGL(extreme_rows_kernel<kMax>, dim3((unsigned)G), dim3(kThreads), 0, s, a);
    return dx::check_hip(hipGetLastError(), "extreme_rows");
  }
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
  return 0;
}
}  // namespace

// tiles [n_tiles][3] and dp_first [G + 1] describe the same plan: the tiles of
// DP g are consecutive.  partial [n_tiles] is scratch, out [G][base] the rows.
extern "C" int dx_extreme_digit_bits(int on_gpu, void *stream, const int64_t *Z, int64_t ldz, const int64_t *tiles,
                                     int64_t n_tiles, const int64_t *dp_first, int64_t G, int is_max, int64_t qmin,
                                     int64_t qmax, int64_t base, int64_t hi, int64_t lo, int64_t prefix,
                                     int64_t *partial, int64_t *out) {
  if (G < 0 || n_tiles < 0 || n_tiles > 0x7fffffff || G > 0x7fffffff || base < 2 || base > 65536 || qmax < qmin ||
      lo < 1 || hi < lo || prefix < 0)
    return -2;
  if (G == 0) return 0;
  ExtArgs a{Z, ldz, tiles, dp_first, partial, out, qmin, qmax, base, hi, lo, prefix};
  return is_max ? run_extreme<true>(on_gpu, stream, a, n_tiles, G) : run_extreme<false>(on_gpu, stream, a, n_tiles, G);
}
