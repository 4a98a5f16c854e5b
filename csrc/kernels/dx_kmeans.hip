// K14f: one Lloyd round of a k-means query -- the nearest centroid of every
// record, then a count, a coordinate sum per column and a sum of squares per
// cluster -- all DPs of a rank in one launch.
//
// A query clusters records of d integer columns over the domain [qmin, qmax]
// (R = qmax - qmin + 1 values per column) into k clusters.  A record's
// coordinates are the offsets o_j = x_j - qmin; the centroids travel as
// integers c[c][j] in units of 1/S (S >= 1, the query's Scale), 0 <= c[c][j] <=
// (R - 1) * S.  For every DP:
//
//   * a row with a coordinate outside [qmin, qmax] is DROPPED (the
//     frequencyCount rule, not clamped);
//   * a kept row goes to the cluster with the smallest
//         D(c) = sum_j (S * o_j - c[c][j])^2,
//     ties to the LOWEST cluster index: the clusters are walked in order and a
//     later one wins only with a strictly smaller D (unsigned compare);
//   * out[dp][c] = [n_c, s_c0 .. s_c(d-1), q_c]: the rows assigned, s_cj = sum
//     o_j and q_c = sum over the rows of sum_j o_j^2 (mod 2^64, like K14).
//
// Limits (drynx_amd/kmeans.py holds the same numbers; the entry checks them
// again and returns -2): 1 <= d <= 32, 1 <= k <= 512, k * (d + 2) <= 3072 cells,
// M = (R - 1) * S < 2^31 -- a difference fits 32 bits and its square is one
// 32 x 32 -> 64 multiply-add -- and d * M^2 < 2^63, so D never wraps.
//
// The records of every DP of the rank are stacked in one int64 matrix Z (DP g
// owns a row range; columns 0 .. d-1 are read in place through the row stride
// ldz).
//
// GPU: one 256-thread workgroup per tile of K14's host-made plan (a row range
// of one DP).  LDS holds, per workgroup,
//   * the accumulators, one 64-bit cell per (cluster, output): k * (d + 2) <= 3072;
//   * a copy of the centroids as 32-bit words, [k][DT] with DT = d rounded up
//     to a power of two and the padding zero, so a cluster's row is read with
//     wide, wave-uniform (broadcast) LDS reads;
//   * the staging area of 256 rows: the tile's rows are loaded 256 at a time
//     with coalesced 64-bit loads by all threads (element e of the chunk is row
//     e / d, column e mod d), reduced to 32-bit offsets -- a coordinate outside
//     the domain becomes kDropped, which no offset equals since o <= M < 2^31 --
//     and stored with an odd row stride, so that the 32-bit reads of
//     consecutive rows fall into different banks.
// Then one thread per row: it takes its offsets into registers (padded to DT
// with zeros: padding adds (0 - 0)^2 to every D), walks the k clusters, and
// keeps register accumulators (n, s_0 .. s_(d-1), q) for the run of equal
// clusters along its rows (rows t, t + 256, ... of the tile), which it flushes
// with d + 2 64-bit LDS atomics (fewer where a sum is zero) when the cluster
// changes and at the tile's end -- K14d's run rule.  After a barrier the
// non-zero cells go to the caller-zeroed out with one 64-bit global (vector)
// atomic each, as K14d flushes.  Integer adds do not depend on the order of
// tiles or atomics; there is no global state beyond out and there are no fences.
// The three LDS areas stay within half a CU's 160 KiB for every (k, d) the
// limits allow (static_assert below): two workgroups stay resident.  The LDS
// is sized per launch, so a small query leaves room for more.
//
// Memory safety does not depend on the centroids, which the entry cannot read
// on the device: a centroid is only SUBTRACTED AND COMPARED, the cell index is
// argmin * (d + 2) + j with argmin in [0, k) whatever the centroids hold, and
// both paths read a centroid as its low 32 bits.
// Host path: the same tiles on the thread pool, every tile summed locally and
// added to out with relaxed atomic adds -- bit-identical to the device.
#include "exec.h"

namespace {
constexpr int kThreads = 256;
constexpr int kMaxDims = 32;
constexpr int kMaxClusters = 512;
constexpr int kMaxCells = 3072;
constexpr uint32_t kDropped = 0xffffffffu;
constexpr int kLdsPerCU = 160 * 1024;

constexpr int padded_dims(int d) {
  int p = 1;
  while (p < d) p *= 2;
  return p;
}
constexpr int stage_stride(int dt) { return dt | 1; }
constexpr int max_clusters(int d) { return kMaxCells / (d + 2) < kMaxClusters ? kMaxCells / (d + 2) : kMaxClusters; }
// Bytes of LDS of a launch: the cells (an even number of them, so the centroid
// rows that follow stay 16-byte aligned), the centroid copy, the staging area.
constexpr size_t lds_bytes(int k, int d) {
  return (size_t)((k * (d + 2) + 1) & ~1) * 8 + (size_t)k * padded_dims(d) * 4 +
         (size_t)kThreads * stage_stride(padded_dims(d)) * 4;
}
constexpr size_t max_lds_bytes() {
  size_t m = 0;
  for (int d = 1; d <= kMaxDims; d++)
    if (lds_bytes(max_clusters(d), d) > m) m = lds_bytes(max_clusters(d), d);
  return m;
}
static_assert(max_lds_bytes() <= kLdsPerCU / 2, "accumulators + centroids + staging: two workgroups per CU");

struct KMeansArgs {
  const int64_t *Z;
  int64_t ldz;
  const int64_t *tiles;  // [n_tiles][3] = (dp, row0, row1)
  const int64_t *cen;    // [k][d], in the memory Z lives in; never trusted
  int k, d;
  uint32_t scale;
  int64_t qmin, qmax;
  int64_t *out;  // [n_dp][k][d + 2], zeroed by the caller
};

// The 32-bit offset of a coordinate, kDropped outside the domain.
__host__ __device__ inline uint32_t offset_of(const KMeansArgs &a, int64_t x) {
  return x < a.qmin || x > a.qmax ? kDropped : (uint32_t)((uint64_t)x - (uint64_t)a.qmin);
}

__host__ __device__ inline uint64_t sq_diff(uint32_t so, uint32_t c) {
  const uint32_t ad = so > c ? so - c : c - so;
  return (uint64_t)ad * ad;
}

// DT consecutive centroid words of LDS, 16-byte aligned when DT >= 4.
template <int DT>
__device__ inline void load_centroid(const uint32_t *row, uint32_t (&c)[DT]) {
  if constexpr (DT >= 4) {
#pragma unroll
    for (int j = 0; j < DT; j += 4) {
      const uint4 v = *reinterpret_cast<const uint4 *>(row + j);
      c[j] = v.x, c[j + 1] = v.y, c[j + 2] = v.z, c[j + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < DT; j++) c[j] = row[j];
  }
}

template <int DT>
__global__ void __launch_bounds__(kThreads) kmeans_kernel(KMeansArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  constexpr int S = stage_stride(DT);
  const int d = a.d, k = a.k, W = d + 2, cells = k * W;
  unsigned long long *cell = reinterpret_cast<unsigned long long *>(lds);    // [k][d + 2]
  uint32_t *cen = reinterpret_cast<uint32_t *>(cell + ((cells + 1) & ~1));  // [k][DT]
  uint32_t *st = cen + k * DT;                                              // [kThreads][S]
  const int64_t dp = a.tiles[3 * (int64_t)blockIdx.x], r0 = a.tiles[3 * (int64_t)blockIdx.x + 1],
                r1 = a.tiles[3 * (int64_t)blockIdx.x + 2];
  for (int i = threadIdx.x; i < cells; i += kThreads) cell[i] = 0;
  for (int i = threadIdx.x; i < k * DT; i += kThreads) {
    const int c = i / DT, j = i - c * DT;
    cen[i] = j < d ? (uint32_t)a.cen[c * d + j] : 0u;
  }

  // the run of equal clusters along this thread's rows
  int cur = 0;
  uint64_t n = 0, q = 0, s[DT];
#pragma unroll
  for (int j = 0; j < DT; j++) s[j] = 0;
  auto flush = [&] {
    unsigned long long *o = cell + cur * W;
    if (n) atomicAdd(o, (unsigned long long)n);
#pragma unroll
    for (int j = 0; j < DT; j++)
      if (j < d && s[j]) atomicAdd(o + 1 + j, (unsigned long long)s[j]);
    if (q) atomicAdd(o + 1 + d, (unsigned long long)q);
    n = 0, q = 0;
#pragma unroll
    for (int j = 0; j < DT; j++) s[j] = 0;
  };

  for (int64_t base = r0; base < r1; base += kThreads) {
    const int nr = (int)(r1 - base < kThreads ? r1 - base : kThreads);
    __syncthreads();  // the cells and centroids are set; the last chunk is consumed
    for (int e = threadIdx.x; e < nr * d; e += kThreads) {
      const int r = e / d, c = e - r * d;
      st[r * S + c] = offset_of(a, a.Z[(base + r) * a.ldz + c]);
    }
    __syncthreads();
    if ((int)threadIdx.x < nr) {
      uint32_t o[DT], so[DT];
      bool keep = true;
#pragma unroll
      for (int j = 0; j < DT; j++) {
        o[j] = j < d ? st[threadIdx.x * S + j] : 0u;
        keep = keep && o[j] != kDropped;
        so[j] = o[j] * a.scale;
      }
      if (keep) {
        int best = 0;
        uint64_t best_d = 0;
        for (int c = 0; c < k; c++) {
          uint32_t cc[DT];
          load_centroid<DT>(cen + c * DT, cc);
          uint64_t D = 0;
#pragma unroll
          for (int j = 0; j < DT; j++) D += sq_diff(so[j], cc[j]);
          if (c == 0 || D < best_d) best = c, best_d = D;
        }
        if (best != cur) {
          flush();
          cur = best;
        }
        n++;
#pragma unroll
        for (int j = 0; j < DT; j++) {
          s[j] += o[j];
          q += (uint64_t)o[j] * o[j];
        }
      }
    }
  }
  flush();
  __syncthreads();
  unsigned long long *o = reinterpret_cast<unsigned long long *>(a.out) + dp * cells;
  for (int i = threadIdx.x; i < cells; i += kThreads)
    if (cell[i]) atomicAdd(o + i, cell[i]);
}

void host_kmeans(const KMeansArgs &a, int64_t n_tiles) {
  const int d = a.d, k = a.k, W = d + 2, cells = k * W;
  dx::host_for_each(n_tiles, [=](int64_t t) {
    const int64_t dp = a.tiles[3 * t], r0 = a.tiles[3 * t + 1], r1 = a.tiles[3 * t + 2];
    std::vector<uint64_t> acc((size_t)cells, 0);
    uint32_t o[kMaxDims];
    for (int64_t r = r0; r < r1; r++) {
      bool keep = true;
      for (int j = 0; j < d; j++) {
        o[j] = offset_of(a, a.Z[r * a.ldz + j]);
        keep = keep && o[j] != kDropped;
      }
      if (!keep) continue;
      int best = 0;
      uint64_t best_d = 0;
      for (int c = 0; c < k; c++) {
        uint64_t D = 0;
        for (int j = 0; j < d; j++) D += sq_diff(o[j] * a.scale, (uint32_t)a.cen[c * d + j]);
        if (c == 0 || D < best_d) best = c, best_d = D;
      }
      uint64_t *row = acc.data() + (size_t)best * W;
      row[0]++;
      for (int j = 0; j < d; j++) {
        row[1 + j] += o[j];
        row[1 + d] += (uint64_t)o[j] * o[j];
      }
    }
    uint64_t *out = reinterpret_cast<uint64_t *>(a.out) + dp * cells;
    for (int i = 0; i < cells; i++)
      if (acc[i]) __atomic_fetch_add(out + i, acc[i], __ATOMIC_RELAXED);
  });
}

template <int DT>
int launch_kmeans(const KMeansArgs &a, int64_t n_tiles, void *stream) {
  static const int lds_rc =
      dx::check_hip(hipFuncSetAttribute(reinterpret_cast<const void *>(kmeans_kernel<DT>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_lds_bytes()),
                    "kmeans_round (LDS size)");
  if (lds_rc) return lds_rc;
  hipLaunchKernelGGL(kmeans_kernel<DT>, dim3((unsigned)n_tiles), dim3(kThreads), lds_bytes(a.k, a.d),
                     (hipStream_t)stream, a);
  return dx::check_hip(hipGetLastError(), "kmeans_round");
}

// The limits of a query: d, k, the cells, S >= 1, M = (R - 1) * S < 2^31 and d * M^2 < 2^63.
bool is_query(int64_t k, int64_t d, int64_t scale, int64_t qmin, int64_t qmax) {
  if (d < 1 || d > kMaxDims || k < 1 || k > kMaxClusters || k * (d + 2) > kMaxCells) return false;
  if (scale < 1 || qmax < qmin) return false;
  const uint64_t R1 = (uint64_t)qmax - (uint64_t)qmin, lim = (uint64_t)1 << 31;
  if (R1 >= lim) return false;
  if (R1 == 0) return true;  // one value: every offset and every centroid is 0
  if ((uint64_t)scale >= lim || R1 * (uint64_t)scale >= lim) return false;
  const uint64_t M = R1 * (uint64_t)scale;
  return M * M <= (((uint64_t)1 << 63) - 1) / (uint64_t)d;
}
}  // namespace

extern "C" int dx_kmeans_max_cells() { return kMaxCells; }

// One round for every DP of a batch.  Z [rows][>= d] with row stride ldz, tiles
// [n_tiles][3] = (dp, row0, row1) with dp < n_dp, cen [k][d] (with Z: host or
// device memory), out [n_dp][k][d + 2] zeroed by the caller.  Everything that
// can be checked without reading device memory is checked here -- the limits
// and the counts; on the host path also the plan (dp, ordered rows) and the
// centroid bounds -- and an argument that does not fit returns -2 and launches
// nothing.
extern "C" int dx_kmeans_round(int on_gpu, void *stream, const int64_t *Z, int64_t ldz, const int64_t *tiles,
                               int64_t n_tiles, int64_t n_dp, const int64_t *cen, int64_t k, int64_t d,
                               int64_t scale, int64_t qmin, int64_t qmax, int64_t *out) {
  if (!is_query(k, d, scale, qmin, qmax)) return -2;
  if (n_tiles < 0 || n_tiles > 0x7fffffff || n_dp < 0 || ldz < 0) return -2;
  if (n_tiles == 0) return 0;
  const uint64_t R1 = (uint64_t)qmax - (uint64_t)qmin;
  if (!on_gpu) {
    for (int64_t t = 0; t < n_tiles; t++)
      if (tiles[3 * t] < 0 || tiles[3 * t] >= n_dp || tiles[3 * t + 1] < 0 || tiles[3 * t + 2] < tiles[3 * t + 1])
        return -2;
    for (int64_t i = 0; i < k * d; i++)
      if (cen[i] < 0 || (uint64_t)cen[i] > R1 * (uint64_t)scale) return -2;
  }
  // (R - 1 = 0: the scale multiplies offsets that are all 0, any 32 bits of it do)
  KMeansArgs a{Z, ldz, tiles, cen, (int)k, (int)d, (uint32_t)scale, qmin, qmax, out};
  if (!on_gpu) {
    host_kmeans(a, n_tiles);
    return 0;
  }
  switch (padded_dims((int)d)) {
    case 1: return launch_kmeans<1>(a, n_tiles, stream);
    case 2: return launch_kmeans<2>(a, n_tiles, stream);
    case 4: return launch_kmeans<4>(a, n_tiles, stream);
    case 8: return launch_kmeans<8>(a, n_tiles, stream);
    case 16: return launch_kmeans<16>(a, n_tiles, stream);
    default: return launch_kmeans<32>(a, n_tiles, stream);
  }
}
