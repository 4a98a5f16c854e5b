// The membership rule of the grouped reductions (SQL WHERE / GROUP BY over the
// DPs' record tables): which group a row of the key matrix K belongs to.  K14d
// (dx_group_moments.hip), the cell plan of the grouped LR encoder
// (dx_group_cells, same file) and the grouped rounds of an iterative query
// (dx_iter_round.hip, dx_iter_round_cells) all include this one definition.
//
//   where(i) : K[i][fcol_f] == fval_f for every filter term f (at most 8), and
//   key(i)   : the mixed-radix number of the digits K[i][kcol_j] - koff_j over
//              the cardinalities kcard_j, first column most significant (at
//              most 4 columns and the counted one of a frequency count); a row
//              with a digit outside [0, kcard_j) has no key and is DROPPED.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace dx {
constexpr int kMaxKeys = 5;  // 4 group-by columns and the counted column of a frequency count
constexpr int kMaxFilters = 8;
constexpr int64_t kMaxGroups = (int64_t)1 << 24;

struct GroupTerms {
  int n_keys, n_filters;
  int kcol[kMaxKeys];
  int64_t koff[kMaxKeys], kcard[kMaxKeys];
  int fcol[kMaxFilters];
  int64_t fval[kMaxFilters];
  int64_t G;   // groups of the query: the product of the cardinalities, 1 without keys
  int64_t g0;  // the window [g0, g0 + gw)
  int gw;
};

// The window-relative group of the row whose key / filter columns are krow,
// -1 if the row does not pass the filter, has no key or lies outside the window.
__host__ __device__ inline int row_group(const GroupTerms &a, const int64_t *krow) {
#pragma unroll
  for (int f = 0; f < kMaxFilters; f++)
    if (f < a.n_filters && krow[a.fcol[f]] != a.fval[f]) return -1;
  uint64_t key = 0;
#pragma unroll
  for (int j = 0; j < kMaxKeys; j++) {
    if (j < a.n_keys) {
      const uint64_t v = (uint64_t)krow[a.kcol[j]] - (uint64_t)a.koff[j];
      if (v >= (uint64_t)a.kcard[j]) return -1;
      key = key * (uint64_t)a.kcard[j] + v;
    }
  }
  const uint64_t rel = key - (uint64_t)a.g0;  // key < G <= 2^24
  return rel < (uint64_t)a.gw ? (int)rel : -1;
}

// The key and filter terms of a call into a: keys [n_keys][3] = (column of K,
// offset, cardinality) and filters [n_filters][2] = (column of K, value) are
// HOST arrays, K has CK columns.  false if a count, a column index or a
// cardinality does not fit (nothing of a is then to be used).
inline bool set_terms(GroupTerms &a, int CK, const int64_t *keys, int n_keys, const int64_t *filters,
                      int n_filters) {
  if (n_keys < 0 || n_keys > kMaxKeys || n_filters < 0 || n_filters > kMaxFilters || CK < 0) return false;
  int64_t G = 1;
  for (int j = 0; j < n_keys; j++) {
    const int64_t col = keys[3 * j], card = keys[3 * j + 2];
    if (col < 0 || col >= CK || card < 1 || card > kMaxGroups) return false;
    G *= card;
    if (G > kMaxGroups) return false;
    a.kcol[j] = (int)col;
    a.koff[j] = keys[3 * j + 1];
    a.kcard[j] = card;
  }
  for (int f = 0; f < n_filters; f++) {
    const int64_t col = filters[2 * f];
    if (col < 0 || col >= CK) return false;
    a.fcol[f] = (int)col;
    a.fval[f] = filters[2 * f + 1];
  }
  a.n_keys = n_keys, a.n_filters = n_filters, a.G = G;
  return true;
}
}  // namespace dx
