// The membership rule of the grouped reductions (SQL WHERE / GROUP BY over the
// DPs' record tables): which group a row of the key matrix K belongs to.  K14d
// (dx_group_moments.hip), the cell plan of the grouped LR encoder
// (dx_group_cells, same file) and the grouped rounds of an iterative query
// (dx_iter_round.hip, dx_iter_round_cells) all include this one definition.
//
//   where(i) : without a predicate, K[i][fcol_f] == fval_f for every filter term
//              f (at most 8).  With a predicate, term f is the atom
//              K[i][fcol_f] OP_f fval_f, OP_f one of == != < <= > >= over signed
//              int64, and the row passes iff bit (sum of atom_f(i) << f) of the
//              predicate's truth table (2^n bits for n terms, at most 256) is
//              set: any formula of !, && and || over the atoms; and
//   key(i)   : the mixed-radix number of the digits K[i][kcol_j] - koff_j over
//              the cardinalities kcard_j, first column most significant (at
//              most 4 columns and the counted one of a frequency count); a row
//              with a digit outside [0, kcard_j) has no key and is DROPPED.
//
// The two forms of where are two INSTANTIATIONS of the rule and of every kernel
// that calls it, chosen at the launch by the flag general: the conjunction of
// equalities keeps its early-exit loop in a kernel that holds nothing of the
// predicate (one kernel with the flag as an argument, a uniform branch, was
// measured 3 - 7 % slower on the equality path: the second path's registers).
// The host twins take the flag at run time.  On the general path every atom is an
// interval test (uint64)(x - lo) <= (uint64)(hi - lo), negated or not, with lo,
// the span hi - lo and the negate bit made by set_terms on the host:
//
//   == c : [c, c]      != c : not [c, c]
//   <= c : [MIN, c]    >  c : not [MIN, c]
//   >= c : [c, MAX]    <  c : not [c, MAX]
//
// exact at both ends of int64 (< MIN holds for no row, <= MAX for every row),
// branch-free and without an early exit, so the lanes of a wave stay together.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace dx {
constexpr int kMaxKeys = 5;  // 4 group-by columns and the counted column of a frequency count
constexpr int kMaxFilters = 8;
constexpr int64_t kMaxGroups = (int64_t)1 << 24;
// operator codes of a predicate's atoms (native.GROUP_OPS, in this order)
enum : int64_t { kOpEq = 0, kOpNe, kOpLt, kOpLe, kOpGt, kOpGe, kOps };

struct GroupTerms {
  int n_keys, n_filters;
  int kcol[kMaxKeys];
  int64_t koff[kMaxKeys], kcard[kMaxKeys];
  int fcol[kMaxFilters];
  int64_t fval[kMaxFilters];  // the constant of an equality; lo of an atom's interval on the general path
  int64_t G;   // groups of the query: the product of the cardinalities, 1 without keys
  int64_t g0;  // the window [g0, g0 + gw)
  int gw;
  // the general path (a predicate): interval spans, negate bits (bit f: term f) and the truth table
  int general;
  unsigned fneg;
  uint64_t fspan[kMaxFilters];
  uint64_t table[4];
};

// where(i) under a predicate: every atom evaluated, one bit of the table decides.
__host__ __device__ inline bool row_passes(const GroupTerms &a, const int64_t *krow) {
  unsigned idx = 0;
#pragma unroll
  for (int f = 0; f < kMaxFilters; f++)
    if (f < a.n_filters) {  // uniform: n_filters is an argument
      const uint64_t d = (uint64_t)krow[a.fcol[f]] - (uint64_t)a.fval[f];
      idx |= ((unsigned)(d <= a.fspan[f]) ^ ((a.fneg >> f) & 1u)) << f;
    }
  // the word by selects on the two high index bits: no lane-varying subscript into the argument struct
  const uint64_t w01 = idx & 64u ? a.table[1] : a.table[0], w23 = idx & 64u ? a.table[3] : a.table[2];
  return (((idx & 128u ? w23 : w01) >> (idx & 63u)) & 1u) != 0;
}

// The window-relative group of the row whose key / filter columns are krow,
// -1 if the row does not pass the filter, has no key or lies outside the window.
// General must be a.general.
template <bool General>
__host__ __device__ inline int row_group(const GroupTerms &a, const int64_t *krow) {
  if constexpr (General) {
    if (!row_passes(a, krow)) return -1;
  } else {
#pragma unroll
    for (int f = 0; f < kMaxFilters; f++)
      if (f < a.n_filters && krow[a.fcol[f]] != a.fval[f]) return -1;
  }
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

// The same with the flag read at run time (the host twins).
__host__ __device__ inline int row_group(const GroupTerms &a, const int64_t *krow) {
  return a.general ? row_group<true>(a, krow) : row_group<false>(a, krow);
}

// The key and filter terms of a call into a: keys [n_keys][3] = (column of K,
// offset, cardinality), filters [n_filters][2] = (column of K, value) and pred
// are HOST arrays, K has CK columns.  pred == NULL: the conjunction of the
// equalities.  Otherwise pred holds n_filters operator codes followed by the
// four 64-bit words of the truth table, low word first.  false if a count, a
// column index, a cardinality or an operator code does not fit, if a table bit
// at or above 2^(2^n_filters) is set or if a predicate comes without a filter
// term (nothing of a is then to be used).
inline bool set_terms(GroupTerms &a, int CK, const int64_t *keys, int n_keys, const int64_t *filters,
                      int n_filters, const int64_t *pred) {
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
  a.general = 0, a.fneg = 0;
  if (pred) {
    if (n_filters < 1) return false;
    for (int f = 0; f < n_filters; f++) {
      const int64_t op = pred[f], c = filters[2 * f + 1];
      if (op < 0 || op >= kOps) return false;
      const bool below = op == kOpLe || op == kOpGt, above = op == kOpGe || op == kOpLt;
      const int64_t lo = below ? INT64_MIN : c, hi = above ? INT64_MAX : c;
      a.fval[f] = lo;
      a.fspan[f] = (uint64_t)hi - (uint64_t)lo;
      if (op == kOpNe || op == kOpGt || op == kOpLt) a.fneg |= 1u << f;
    }
    const int bits = 1 << n_filters;  // of the table: 2 .. 256
    for (int w = 0; w < 4; w++) {
      const uint64_t word = (uint64_t)pred[n_filters + w];
      const int have = bits - 64 * w;  // table bits that fall into this word
      if (have < 64 && (have <= 0 ? word : word >> have)) return false;
      a.table[w] = word;
    }
    a.general = 1;
  }
  a.n_keys = n_keys, a.n_filters = n_filters, a.G = G;
  return true;
}
}  // namespace dx
