// K14d: K14's exact int64 moments, filtered and grouped (SQL WHERE / GROUP BY
// over the DPs' records), all DPs of a rank in one launch per group window.
//
//     out[dp][g][p] = sum over rows i of DP dp with where(i) and key(i) == g
//                     of Z[i][a_p] * Z[i][b_p]                  (mod 2^64, like Go)
//
// Z [rows][C] is K14's value matrix (column C = constant 1, the pair list is
// K14's).  A second matrix K [rows][CK] (its own row stride) holds the columns
// the query filters and groups by:
//
//   where(i) : K[i][fcol_f] == fval_f for every filter term f (at most 8) or,
//              with a predicate, a formula of !, && and || over the atoms
//              K[i][fcol_f] OP_f fval_f (== != < <= > >=, signed), and
//   key(i)   : the mixed-radix number of the digits K[i][kcol_j] - koff_j over
//              the cardinalities kcard_j, first column most significant (at
//              most 4 columns and the counted one below); a row with a digit
//              outside [0, kcard_j) has no key and is DROPPED, as the
//              histogram drops out-of-domain records.
//
// The rule (the terms, row_group and their checker) lives in group_terms.h,
// which the grouped rounds of an iterative query (dx_iter_round.hip) share.
//
// No key column: one group.  A frequency count is the same reduction: the pair
// list is the single pair (C, C) and the counted column is one more innermost
// key column (x, QueryMin, R), so a (group, bin) cell is a group.
//
// GPU: one 256-thread workgroup per tile of K14's host-made plan.  The
// accumulators live in LDS, one 64-bit cell per (group of the window, pair);
// a launch covers the window [g0, g0 + gw) of consecutive groups with
// gw * P <= kMaxCells and ignores rows whose key falls outside it (the binding
// loops over the windows).  kMaxCells is sized so that a workgroup never takes
// more than half of a CU's 160 KiB of LDS: two workgroups stay resident.  The
// tile's rows are staged 64 at a time (values with the constant column
// appended, and each row's window-relative key, -1 for a row that does not
// count); the threads split the (pair, row-lane) space as in K14.  Each thread
// keeps a register accumulator for the run of equal keys along its row lane and
// flushes it with one 64-bit LDS atomic when the key changes and at the tile's
// end; after a barrier the non-zero cells go to the output with one global
// (vector) 64-bit atomic each.  Integer addition is associative and
// commutative, so the result does not depend on the order of tiles or atomics.
// Host path: the same tiles on the thread pool, adding to the output with
// relaxed atomic adds -- bit-identical to the device.
#include "exec.h"
#include "group_terms.h"

namespace {
using dx::GroupTerms;
using dx::row_group;
using dx::set_terms;
constexpr int kRows = 64;
constexpr int kMaxCols = 64;                                   // data columns (+ the constant one)
constexpr int kMaxPairs = (kMaxCols + 1) * (kMaxCols + 2) / 2;  // 2145
constexpr int kThreads = 256;
constexpr int kMaxUnits = (kMaxPairs + kThreads - 1) / kThreads;
constexpr int kLdsPerCU = 160 * 1024;
constexpr int kStageBytes = kRows * (kMaxCols + 2) * 8 + kRows * 4;  // widest staging area + the keys
// cells of one launch: what half a CU's LDS leaves beside the widest staging
// area, rounded down to a multiple of 256
constexpr int kMaxCells = (kLdsPerCU / 2 - kStageBytes) / 8 / 256 * 256;  // 5888
static_assert(kMaxCells >= kMaxPairs, "one group of the widest pair list fits a window");
static_assert(kMaxCells * 8 + kStageBytes <= kLdsPerCU / 2, "two workgroups per CU");

struct GroupArgs : GroupTerms {  // G groups: out is [n_dp][G][P], zeroed by the caller
  const int64_t *Z;
  int64_t ldz;
  int C;
  const int64_t *K;
  int64_t ldk;
  const int64_t *tiles;  // [n_tiles][3] = (dp, row0, row1)
  const int16_t *pairs;  // [P][2], column index C = constant 1
  int P;
  int L;  // row lanes per pair
  int64_t *out;
};

// Row stride of the staging area in int64: odd, so the 64-bit reads of
// consecutive rows fall into different banks.
__host__ __device__ inline int stage_stride(int C) { return (C + 1) | 1; }

inline size_t lds_bytes(int C, int cells) {
  return (size_t)cells * 8 + (size_t)kRows * stage_stride(C) * 8 + (size_t)kRows * 4;
}

template <bool General>  // a.general: the WHERE is a predicate
__global__ void __launch_bounds__(kThreads) group_moments_kernel(GroupArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int cells = a.gw * a.P;
  const int W = a.C + 1, S = stage_stride(a.C);
  unsigned long long *cell = reinterpret_cast<unsigned long long *>(lds);  // [gw][P]
  int64_t *z = reinterpret_cast<int64_t *>(lds) + cells;                   // [kRows][S]
  int *grp = reinterpret_cast<int *>(z + kRows * S);                       // [kRows]
  const int64_t dp = a.tiles[3 * (int64_t)blockIdx.x], r0 = a.tiles[3 * (int64_t)blockIdx.x + 1],
                r1 = a.tiles[3 * (int64_t)blockIdx.x + 2];
  for (int c = threadIdx.x; c < cells; c += kThreads) cell[c] = 0;

  const int units = a.P * a.L;
  uint64_t acc[kMaxUnits];
  int cur[kMaxUnits], pp[kMaxUnits], ca[kMaxUnits], cb[kMaxUnits], lane[kMaxUnits];
#pragma unroll
  for (int k = 0; k < kMaxUnits; k++) {
    const int e = threadIdx.x + k * kThreads;
    acc[k] = 0;
    cur[k] = 0;
    pp[k] = e < units ? e / a.L : 0;
    ca[k] = a.pairs[2 * pp[k]];
    cb[k] = a.pairs[2 * pp[k] + 1];
    lane[k] = e % a.L;
  }

  for (int64_t base = r0; base < r1; base += kRows) {
    const int nr = (int)(r1 - base < kRows ? r1 - base : kRows);
    __syncthreads();
    for (int e = threadIdx.x; e < kRows * W; e += kThreads) {
      const int r = e / W, c = e - r * W;
      z[r * S + c] = r < nr ? (c < a.C ? a.Z[(base + r) * a.ldz + c] : 1) : 0;
    }
    if (threadIdx.x < kRows) {
      const int r = threadIdx.x;
      grp[r] = r < nr ? row_group<General>(a, a.K + (base + r) * a.ldk) : -1;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kMaxUnits; k++) {
      if (threadIdx.x + k * kThreads < units) {
        uint64_t s = acc[k];
        int g = cur[k];
        for (int r = lane[k]; r < nr; r += a.L) {
          const int gr = grp[r];
          if (gr < 0) continue;
          if (gr != g) {  // the run of equal keys ends: one LDS atomic
            if (s) atomicAdd(&cell[g * a.P + pp[k]], (unsigned long long)s);
            s = 0;
            g = gr;
          }
          s += (uint64_t)z[r * S + ca[k]] * (uint64_t)z[r * S + cb[k]];
        }
        acc[k] = s;
        cur[k] = g;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kMaxUnits; k++)
    if (threadIdx.x + k * kThreads < units && acc[k])
      atomicAdd(&cell[cur[k] * a.P + pp[k]], (unsigned long long)acc[k]);
  __syncthreads();
  unsigned long long *o = reinterpret_cast<unsigned long long *>(a.out) + (dp * a.G + a.g0) * a.P;
  for (int c = threadIdx.x; c < cells; c += kThreads)
    if (cell[c]) atomicAdd(o + c, cell[c]);
}

void host_group_moments(const GroupArgs &a, int64_t n_tiles) {
  dx::host_for_each(n_tiles, [=](int64_t t) {
    const int64_t dp = a.tiles[3 * t], r0 = a.tiles[3 * t + 1], r1 = a.tiles[3 * t + 2];
    uint64_t *o = reinterpret_cast<uint64_t *>(a.out) + (dp * a.G + a.g0) * a.P;
    for (int64_t i = r0; i < r1; i++) {
      const int g = row_group(a, a.K + i * a.ldk);
      if (g < 0) continue;
      const int64_t *zi = a.Z + i * a.ldz;
      for (int p = 0; p < a.P; p++) {
        const int ia = a.pairs[2 * p], ib = a.pairs[2 * p + 1];
        const uint64_t x = ia < a.C ? (uint64_t)zi[ia] : 1u, y = ib < a.C ? (uint64_t)zi[ib] : 1u;
        __atomic_fetch_add(o + (int64_t)g * a.P + p, x * y, __ATOMIC_RELAXED);
      }
    }
  });
}
}  // namespace

extern "C" int dx_group_moments_max_cells() { return kMaxCells; }

// keys [n_keys][3] = (column of K, offset, cardinality), filters
// [n_filters][2] = (column of K, value) and pred (NULL: the conjunction of the
// equalities; else n_filters operator codes and the four words of the truth
// table, group_terms.h) are HOST arrays; K has CK columns.  out
// [n_dp][G][P] with G the product of the cardinalities (1 without keys) is
// zeroed by the caller before the first window; this call adds the groups
// [g0, g0 + gw).  Every count, cardinality, column index and the cell cap is
// checked here: an argument that does not fit returns -2 and launches nothing.
namespace {
// cell[i] = the group of row i among all G, G for a row that is dropped
template <bool General>
struct RowCells {
  GroupArgs a;  // g0 = 0, gw = G: the window is every group; a.general == General
  int64_t *cell;
  __host__ __device__ void operator()(int64_t i) const {
    const int g = row_group<General>(a, a.K + i * a.ldk);
    cell[i] = g < 0 ? a.G : (int64_t)g;
  }
};

template <bool General>
int run_cells(int on_gpu, void *stream, const GroupArgs &a, int64_t rows, int64_t *cell) {
  return dx::run(on_gpu, stream, rows, RowCells<General>{a, cell}, false, "group_cells");
}
}  // namespace

// The cell plan of a grouped encoder over other records than K14's (the
// logistic-regression cohorts): cell[i] = the group of row i of K [rows][CK] by
// the membership rule above (row_group, the very function of the moments), G =
// the product of the cardinalities for a row that the WHERE or an out-of-range
// key digit drops.  keys, filters and pred as below.
extern "C" int dx_group_cells_pred(int on_gpu, void *stream, const int64_t *K, int64_t ldk, int CK, int64_t rows,
                                   const int64_t *keys, int n_keys, const int64_t *filters, int n_filters,
                                   int64_t *cell, const int64_t *pred) {
  GroupArgs a{};
  if (rows < 0 || !set_terms(a, CK, keys, n_keys, filters, n_filters, pred)) return -2;
  a.K = K, a.ldk = ldk, a.g0 = 0, a.gw = (int)a.G;
  return a.general ? run_cells<true>(on_gpu, stream, a, rows, cell) : run_cells<false>(on_gpu, stream, a, rows, cell);
}

// pred == NULL under the signature the entry had before predicates
extern "C" int dx_group_cells(int on_gpu, void *stream, const int64_t *K, int64_t ldk, int CK, int64_t rows,
                              const int64_t *keys, int n_keys, const int64_t *filters, int n_filters,
                              int64_t *cell) {
  return dx_group_cells_pred(on_gpu, stream, K, ldk, CK, rows, keys, n_keys, filters, n_filters, cell, nullptr);
}

extern "C" int dx_group_moments_pred(int on_gpu, void *stream, const int64_t *Z, int64_t ldz, int C,
                                     const int64_t *K, int64_t ldk, int CK, const int64_t *tiles, int64_t n_tiles,
                                     const int16_t *pairs, int P, const int64_t *keys, int n_keys,
                                     const int64_t *filters, int n_filters, int64_t g0, int64_t gw, int64_t *out,
                                     const int64_t *pred) {
  if (C < 0 || C > kMaxCols || P <= 0 || P > kMaxPairs || n_tiles < 0 || n_tiles > 0x7fffffff) return -2;
  GroupArgs a{};
  if (!set_terms(a, CK, keys, n_keys, filters, n_filters, pred)) return -2;
  const int64_t G = a.G;
  if (g0 < 0 || gw < 1 || g0 + gw > G || gw * P > kMaxCells) return -2;
  if (n_tiles == 0) return 0;
  a.Z = Z, a.ldz = ldz, a.C = C, a.K = K, a.ldk = ldk, a.tiles = tiles, a.pairs = pairs, a.P = P;
  a.n_keys = n_keys, a.n_filters = n_filters, a.G = G, a.g0 = g0, a.gw = (int)gw, a.out = out;
  if (!on_gpu) {
    host_group_moments(a, n_tiles);
    return 0;
  }
  a.L = 1;
  while (a.L < kRows && P * a.L * 2 <= kThreads) a.L *= 2;
  const size_t bytes = lds_bytes(C, (int)(gw * P));
  void (*const kernel)(GroupArgs) = a.general ? group_moments_kernel<true> : group_moments_kernel<false>;
  if (bytes > 48 * 1024)
    if (int rc = dx::check_hip(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes),
                               "group_moments (LDS size)"))
      return rc;
  hipLaunchKernelGGL(kernel, dim3((unsigned)n_tiles), dim3(kThreads), bytes, (hipStream_t)stream, a);
  return dx::check_hip(hipGetLastError(), "group_moments");
}

// pred == NULL under the signature the entry had before predicates
extern "C" int dx_group_moments(int on_gpu, void *stream, const int64_t *Z, int64_t ldz, int C, const int64_t *K,
                                int64_t ldk, int CK, const int64_t *tiles, int64_t n_tiles, const int16_t *pairs,
                                int P, const int64_t *keys, int n_keys, const int64_t *filters, int n_filters,
                                int64_t g0, int64_t gw, int64_t *out) {
  return dx_group_moments_pred(on_gpu, stream, Z, ldz, C, K, ldk, CK, tiles, n_tiles, pairs, P, keys, n_keys, filters,
                               n_filters, g0, gw, out, nullptr);
}
