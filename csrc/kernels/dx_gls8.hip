// GLS-2 fixed-base tables with SIGNED 8-bit windows (prover table mode 7;
// K6/K7 of the range-proof prover, lib/range/range_proof.go:452-469).
//
// The prover's per-item work is V = v A_phi (G2) and e(B, A_phi)^(-s v) (GT)
// with per-signature bases.  Both groups carry an endomorphism with eigenvalue
// lambda2 = 6u^2 = p (mod r), a ~127-bit number: psi on G2 (curve.h) and the
// Frobenius x -> x^p on GT.  Any scalar k < r splits as k = k0 + k1 lambda2
// with k0 < lambda2 and k1 < 2^128 by one long division (no lattice: lambda2 ~
// sqrt r), so k Q = k0 Q + psi(k1 Q) and x^k = x^k0 * frob(x^k1): two
// fixed-base evaluations over 128-bit exponents from ONE table per base.  Each
// half is recoded LSB-first into 17 signed digits in [-127, 128] (a byte plus
// the carry of the previous window), so one table per base holds
// d 2^(8w) Q for d = 1..128, w < 17 (2176 entries: 272 KiB on G2, 408 KiB on
// GT), and a negative digit uses the negated entry -- y -> -y on G2,
// beta -> -beta on GT.  An evaluation costs 34 mixed additions / GT steps
// instead of the 64 of the 4-bit 256-bit comb.  For the reference's random
// per-CN, per-column keys (99,360 points for a SPECTF-shaped query) the tables
// take ~70 GB of the 288 GB of HBM.
//
// The GT side runs on torus images (gt_torus.h): a table entry is the Fp6
// element beta = (1 + g) / h of E^(d 2^(8w)) = g + h w, a chain multiplies a
// numerator y by (+-beta + w) -- two Fp6 products per step on a lane pair --
// and the canonical Fp12 value pi(y) = y / conj(y) is taken once per item at
// the end (gt_finish_kernel, one Fp6 inversion per chunk of items).
//
// Every body is force-inlined into an explicit __global__ kernel (no device
// calls: see dx_rpmsm.hip on branch relaxation in out-of-line callees).
#define DX_NI __host__ __device__ __forceinline__
#include "common.h"
#include "../bn254/gt_coop.h"
#include "../bn254/gt_torus.h"

using namespace dxk;

namespace {
constexpr int kBits = 8;
constexpr int kHalf = 1 << (kBits - 1);   // 128 entries per window
constexpr int kWin = 17;                  // 16 bytes + the final carry
constexpr int kEnt = kWin * kHalf;        // 2176
constexpr int kWG = 64;

// k (8 limbs) = k0 + k1 * lambda2, k0 < lambda2 (4 limbs), k1 < 2^128: binary
// long division by the 127-bit constant.
DX_HD void split_lambda2(const uint32_t *k, uint32_t *k0, uint32_t *k1) {
  uint32_t rem[5] = {0, 0, 0, 0, 0}, q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int bit = 255; bit >= 0; bit--) {
#pragma unroll
    for (int i = 4; i > 0; i--) rem[i] = (rem[i] << 1) | (rem[i - 1] >> 31);
    rem[0] = (rem[0] << 1) | ((k[bit >> 5] >> (bit & 31)) & 1u);
    uint32_t d[5], br = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) d[i] = subb32(rem[i], i < 4 ? SIX_U2[i] : 0u, br);
    if (!br) {
#pragma unroll
      for (int i = 0; i < 5; i++) rem[i] = d[i];
      q[bit >> 5] |= 1u << (bit & 31);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; i++) k0[i] = rem[i];
  k0[4] = 0;
#pragma unroll
  for (int i = 0; i < 5; i++) k1[i] = q[i];
}

// signed digit of byte window w (LSB first), carry in / out
DX_HD int sdigit(const uint32_t *k5, int w, uint32_t &carry) {
  const int bit = w * kBits;
  const uint32_t v = ((k5[bit >> 5] >> (bit & 31)) & 0xFFu) + carry;
  carry = v > (uint32_t)kHalf ? 1u : 0u;
  return carry ? (int)v - 256 : (int)v;
}

DX_HD void g2_half(G2J &a, const G2A *T, const uint32_t *k5) {
  uint32_t c = 0;
  for (int w = 0; w < kWin; w++) {
    const int d = sdigit(k5, w, c);
    if (d) {
      G2A q = T[w * kHalf + (d > 0 ? d : -d) - 1];
      if (d < 0) q.y = neg(q.y);
      a = jadd_mixed(a, q);
    }
  }
}

DX_HD G2J g2_gls8_eval(const G2A *T, const uint32_t *k) {
  uint32_t k0[5], k1[5];
  split_lambda2(k, k0, k1);
  G2J a = G2J::inf();
  g2_half(a, T, k1);
  a = psi(a);
  g2_half(a, T, k0);
  return a;
}

// the table row of an entry that is 1 (beta_chunk): no step
DX_HD bool is_unit_row(const Fp6 &b) { return b.c0.c0.v[7] == 0xFFFFFFFFu; }

// y <- y * prod (+-beta + w) over the signed windows of one 128-bit half
DX_HD void gt_half(Fp12 &y, const Fp6 *T, const uint32_t *k5) {
  uint32_t c = 0;
  for (int w = 0; w < kWin; w++) {
    const int d = sdigit(k5, w, c);
    if (!d) continue;
    const Fp6 &b = T[w * kHalf + (d > 0 ? d : -d) - 1];
    if (!is_unit_row(b)) torus::mul_beta(y, b, d < 0);
  }
}

// a numerator of E^k from the beta table of E
DX_HD Fp12 gt_gls8_eval(const Fp6 *T, const uint32_t *k) {
  uint32_t k0[5], k1[5];
  split_lambda2(k, k0, k1);
  Fp12 y = Fp12::one();
  gt_half(y, T, k1);
  y = frob<1>(y);
  gt_half(y, T, k0);
  return y;
}

// ---- table construction: work[b*17 + w] = 2^(8w) base; entry = d * work
DX_HD void g2_pow_one(const uint32_t *bases_aff, uint32_t *work, int64_t b) {
  G2J acc = G2J::from_aff(at<G2A>(bases_aff, b));
  for (int w = 0; w < kWin; w++) {
    at<G2J>(work, b * kWin + w) = acc;
    for (int i = 0; i < kBits; i++) acc = jdbl(acc);
  }
}
DX_HD void gt_pow_one(const uint32_t *bases, uint32_t *work, int64_t b) {
  Fp12 acc = at<Fp12>(bases, b);
  for (int w = 0; w < kWin; w++) {
    at<Fp12>(work, b * kWin + w) = acc;
    for (int i = 0; i < kBits; i++) acc = cyclotomic_sqr(acc);
  }
}
// Entries by chunks of kCh consecutive digits d0 .. d0 + kCh - 1 of one
// window: the first by double-and-add from the window's base, each next one
// by one more addition / product -- ~1/7 of the per-entry double-and-add
// (setup: ~3.4 s of table building for a 3-CN SPECTF-shaped set).
constexpr int kCh = 16;
constexpr int kChunks = kEnt / kCh;  // 136 per base (kHalf = 128 is a multiple of kCh)

DX_HD void g2_entry_chunk_one(const uint32_t *work, uint32_t *table, int64_t t) {
  const int64_t b = t / kChunks, c = t % kChunks;
  const int w = (int)(c / (kHalf / kCh)), d0 = (int)(c % (kHalf / kCh)) * kCh + 1;
  const int64_t qi = b * kWin + w;  // q re-read per addition: no register copy to spill
  G2J acc = G2J::inf();
  for (int bit = kBits - 1; bit >= 0; bit--) {
    acc = jdbl(acc);
    if ((d0 >> bit) & 1) acc = jadd(acc, at<G2J>(work, qi));
  }
  const int64_t e0 = b * kEnt + (int64_t)w * kHalf + d0 - 1;
  for (int j = 0; j < kCh; j++) {
    at<G2A>(table, e0 + j) = to_affine(acc);
    if (j + 1 < kCh) acc = jadd(acc, at<G2J>(work, qi));
  }
}

// beta[j] = (1 + g_j) / h_j of the kCh unitary f[j] = g_j + h_j w with ONE Fp6
// inversion (Montgomery's trick; the prefix products are parked in the output
// rows).  f_j = 1 has no image (beta would be infinite): its row is the unit
// mark, all words 0xFFFFFFFF -- no canonical limb -- and the chains skip such a
// row (a signature set pads with the point at infinity, whose E is 1).
// false when some f_j = g + 0 w is not 1.
DX_HD bool beta_chunk(const Fp12 *f, Fp6 *beta) {
  Fp6 acc = Fp6::one();
  bool ok = true;
  for (int j = 0; j < kCh; j++) {
    beta[j] = acc;
    if (!(f[j].c1 == Fp6::zero())) acc = torus::mul6(acc, f[j].c1);
  }
  Fp6 inv_all = inv(acc);
  for (int j = kCh - 1; j >= 0; j--) {
    if (f[j].c1 == Fp6::zero()) {
      ok = ok && f[j].c0 == Fp6::one();
      uint32_t *row = &beta[j].c0.c0.v[0];
      for (int i = 0; i < 48; i++) row[i] = 0xFFFFFFFFu;
      continue;
    }
    const Fp6 hi = torus::mul6(inv_all, beta[j]);
    inv_all = torus::mul6(inv_all, f[j].c1);
    beta[j] = torus::mul6(add(Fp6::one(), f[j].c0), hi);
  }
  return ok;
}

DX_HD bool gt_entry_chunk_one(const uint32_t *work, uint32_t *table, int64_t t) {
  const int64_t b = t / kChunks, c = t % kChunks;
  const int w = (int)(c / (kHalf / kCh)), d0 = (int)(c % (kHalf / kCh)) * kCh + 1;
  const Fp12 q = at<Fp12>(work, b * kWin + w);
  Fp12 f[kCh];
  Fp12 acc = Fp12::one();
  for (int bit = kBits - 1; bit >= 0; bit--) {
    acc = cyclotomic_sqr(acc);
    if ((d0 >> bit) & 1) acc = mul(acc, q);
  }
  for (int j = 0; j < kCh; j++) {
    f[j] = acc;
    if (j + 1 < kCh) acc = mul(acc, q);
  }
  return beta_chunk(f, &at<Fp6>(table, b * kEnt + (int64_t)w * kHalf + d0 - 1));
}

// the GT chunks on three lanes per chunk (gt_coop.h: no Fp12 spills): the
// Fp12 powers, [n_bases * 2176, 96], which gt_beta_chunk_kernel normalises
__global__ void __launch_bounds__(64) DX_OCC gt_entry_chunk_coop(const uint32_t *work, uint32_t *table, int64_t n) {
  const coop::Role R = coop::role();
  const int64_t t = (int64_t)blockIdx.x * coop::kTriples + R.g;
  if (R.g >= coop::kTriples || t >= n) return;  // whole triples leave together
  const int64_t b = t / kChunks, c = t % kChunks;
  const int w = (int)(c / (kHalf / kCh)), d0 = (int)(c % (kHalf / kCh)) * kCh + 1;
  const Fp12 *Q = &at<Fp12>(work, b * kWin + w);  // re-read per product (L1 / L2): no register copy to spill
  Fp6 acc = coop::one(R);
  for (int bit = kBits - 1; bit >= 0; bit--) {
    coop::mul(acc, acc, R);
    if ((d0 >> bit) & 1) coop::mul(acc, coop::load(Q, false, R), R);
  }
  const int64_t e0 = b * kEnt + (int64_t)w * kHalf + d0 - 1;
  for (int j = 0; j < kCh; j++) {
    coop::store(&at<Fp12>(table, e0 + j), acc, R);
    if (j + 1 < kCh) coop::mul(acc, coop::load(Q, false, R), R);
  }
}

DX_HD void g2_mul_one(const uint32_t *tables, const int32_t *tab_idx, const uint32_t *scalars, uint32_t *out_aff,
                      int64_t i) {
  const G2A *T = reinterpret_cast<const G2A *>(tables) + (int64_t)(tab_idx ? tab_idx[i] : 0) * kEnt;
  at<G2A>(out_aff, i) = to_affine(g2_gls8_eval(T, scalars + 8 * i));
}

// ---- gT with signed 16-bit windows: T16[w*32768 + d-1] = gT^(d 2^(16w)),
// d = 1..32768, w < 17 (214 MB, one table per device): 17 products per
// exponentiation instead of the 32 of the 8-bit comb
constexpr int kB16 = 16, kH16 = 1 << 15, kW16 = 17;
// beta rows of the kCh consecutive digits of chunk t (host)
DX_HD bool gt16_entry_chunk_one(const uint32_t *pow2, uint32_t *table, int64_t t) {
  const int w = (int)(t / (kH16 / kCh)), d0 = (int)(t % (kH16 / kCh)) * kCh + 1;
  const Fp12 q = at<Fp12>(pow2, w);
  Fp12 f[kCh];
  Fp12 acc = Fp12::one();
  for (int bit = kB16 - 1; bit >= 0; bit--) {  // d <= 2^15
    acc = cyclotomic_sqr(acc);
    if ((d0 >> bit) & 1) acc = mul(acc, q);
  }
  for (int j = 0; j < kCh; j++) {
    f[j] = acc;
    if (j + 1 < kCh) acc = mul(acc, q);
  }
  return beta_chunk(f, &at<Fp6>(table, (int64_t)w * kH16 + d0 - 1));
}
// signed 16-bit digit of window w (LSB first), carry in / out
DX_HD int sdigit16(const uint32_t *k, int w, uint32_t &carry) {
  const uint32_t raw = w < 16 ? (k[w >> 1] >> (16 * (w & 1))) & 0xFFFFu : 0u;
  const uint32_t v = raw + carry;
  carry = v > (uint32_t)kH16 ? 1u : 0u;
  return carry ? (int)v - 65536 : (int)v;
}
// a numerator of gT^k from the 16-bit beta table
DX_HD Fp12 gt16_pow(const Fp6 *T, const uint32_t *k) {
  Fp12 y = Fp12::one();
  uint32_t carry = 0;
  for (int w = 0; w < kW16; w++) {
    const int d = sdigit16(k, w, carry);
    if (d) torus::mul_beta(y, T[w * kH16 + (d > 0 ? d : -d) - 1], d < 0);
  }
  return y;
}

// prover pass 1: a[p*S*L + j] = a numerator of gT^(t[p*L + j]) (shared by the
// S servers); t16: gt_table is the signed 16-bit beta table instead of the
// 8-bit Fp12 comb
DX_HD void prove_t_one(const uint32_t *t_sc, const uint32_t *gt_table, uint32_t *a_out, int S, int L, int t16,
                       int64_t pj) {
  const int64_t p = pj / L, j = pj % L;
  at<Fp12>(a_out, p * S * L + j) =
      t16 ? gt16_pow(reinterpret_cast<const Fp6 *>(gt_table), t_sc + 8 * pj)
          : torus::num_of(gt_fixed_pow(reinterpret_cast<const Fp12 *>(gt_table), t_sc + 8 * pj));
}
// prover pass 2 over the items of one server range [i_lo, i_hi): a[it] = a
// numerator of E^(e[it]) * pi(a[p*S*L + j]); pass 3 (finish) maps every row by pi
DX_HD void prove_e_one(const uint32_t *gphi_tables, const int32_t *tab_idx, const uint32_t *e_sc, uint32_t *a_out,
                       int S, int L, int i_lo, int i_hi, int64_t k) {
  const int64_t per = (int64_t)(i_hi - i_lo) * L;
  const int64_t p = k / per, r = k % per;
  const int64_t i = i_lo + r / L, j = r % L;
  const int64_t it = (p * S + i) * L + j;
  const Fp6 *T = reinterpret_cast<const Fp6 *>(gphi_tables) + (int64_t)tab_idx[it] * kEnt;
  at<Fp12>(a_out, it) = mul(gt_gls8_eval(T, e_sc + 8 * it), at<Fp12>(a_out, p * S * L + j));
}

// ---- the prover passes on the GPU: a lane pair per item (gt_torus.h)
namespace tp = torus::pair;
// x <- x * prod (+-beta + w) over the signed 8-bit windows of one 128-bit half
__device__ __forceinline__ void gt_half_pair(Fp6 &x, const Fp6 *T, const uint32_t *k5, const tp::Role &R) {
  uint32_t c = 0;
  for (int w = 0; w < kWin; w++) {
    const int d = sdigit(k5, w, c);
    if (!d) continue;  // both lanes of a pair: the same d and the same row
    const Fp6 &b = T[w * kHalf + (d > 0 ? d : -d) - 1];
    if (!is_unit_row(b)) tp::mul_beta(x, b, d < 0, R);
  }
}

__global__ void __launch_bounds__(kWG) DX_OCC prove_t_pair(const uint32_t *t_sc, const uint32_t *gt16, uint32_t *a_out,
                                                          int S, int L, int64_t n_pj) {
  const tp::Role R = tp::role();
  const int64_t pj = (int64_t)blockIdx.x * tp::kPairs + R.g;
  if (pj >= n_pj) return;  // whole pairs leave together
  const Fp6 *T = reinterpret_cast<const Fp6 *>(gt16);
  const uint32_t *k = t_sc + 8 * pj;
  Fp6 x = tp::one(R);
  uint32_t carry = 0;
  for (int w = 0; w < kW16; w++) {
    const int d = sdigit16(k, w, carry);
    if (d) tp::mul_beta(x, T[w * kH16 + (d > 0 ? d : -d) - 1], d < 0, R);
  }
  const int64_t p = pj / L, j = pj % L;
  tp::store(&at<Fp12>(a_out, p * S * L + j), x, R);
}

// server range [i_lo, i_hi): a[it] = a numerator of E_phi(it)^(e[it]) * pi(a[p*S*L + j])
__global__ void __launch_bounds__(kWG) DX_OCC prove_e_pair(const uint32_t *gphi, const int32_t *tab_idx,
                                                          const uint32_t *e_sc, uint32_t *a_out, int S, int L,
                                                          int i_lo, int i_hi, int64_t n) {
  const tp::Role R = tp::role();
  const int64_t kk = (int64_t)blockIdx.x * tp::kPairs + R.g;
  if (kk >= n) return;
  const int64_t per = (int64_t)(i_hi - i_lo) * L;
  const int64_t p = kk / per, rr = kk % per;
  const int64_t i = i_lo + rr / L, j = rr % L;
  const int64_t it = (p * S + i) * L + j;
  const Fp6 *T = reinterpret_cast<const Fp6 *>(gphi) + (int64_t)tab_idx[it] * kEnt;
  uint32_t k0[5], k1[5];
  split_lambda2(e_sc + 8 * it, k0, k1);
  Fp6 x = tp::one(R);
  gt_half_pair(x, T, k1, R);
  tp::frob1(x, R);
  gt_half_pair(x, T, k0, R);
  tp::mul_full(x, &at<Fp12>(a_out, p * S * L + j), R);  // both lanes have read the shared slot before either store
  tp::store(&at<Fp12>(a_out, it), x, R);
}

// pass 3: a[i] <- pi(a[i]), one lane per chunk of k rows (one Fp6 inversion per chunk)
__global__ void __launch_bounds__(kWG) DX_OCC gt_finish_kernel(uint32_t *a, uint32_t *tmp, int64_t n, int64_t k) {
  const int64_t t = (int64_t)blockIdx.x * kWG + threadIdx.x;
  const int64_t i0 = t * k, i1 = i0 + k < n ? i0 + k : n;
  if (i0 < n) torus::finish_chunk(reinterpret_cast<Fp12 *>(a), reinterpret_cast<Fp12 *>(tmp), i0, i1);
}

// beta rows of chunk t of the Fp12 powers f [n * kCh, 96] -> table [n * kCh, 48]; *bad |= 1 on an h = 0
__global__ void __launch_bounds__(kWG) DX_OCC gt_beta_chunk_kernel(const uint32_t *f, uint32_t *table, uint32_t *bad,
                                                                  int64_t n) {
  const int64_t t = (int64_t)blockIdx.x * kWG + threadIdx.x;
  if (t >= n) return;
  if (!beta_chunk(&at<Fp12>(f, t * kCh), &at<Fp6>(table, t * kCh))) atomicOr(bad, 1u);
}

#define DX_TID() const int64_t i = (int64_t)blockIdx.x * kWG + threadIdx.x
__global__ void __launch_bounds__(kWG) DX_OCC g2_pow_kernel(const uint32_t *b, uint32_t *w, int64_t n) {
  DX_TID();
  if (i < n) g2_pow_one(b, w, i);
}
__global__ void __launch_bounds__(kWG) DX_OCC g2_entry_chunk_kernel(const uint32_t *w, uint32_t *t, int64_t n) {
  DX_TID();
  if (i < n) g2_entry_chunk_one(w, t, i);
}
__global__ void __launch_bounds__(kWG) DX_OCC gt_pow_kernel(const uint32_t *b, uint32_t *w, int64_t n) {
  DX_TID();
  if (i < n) gt_pow_one(b, w, i);
}

__global__ void __launch_bounds__(kWG) DX_OCC g2_mul_kernel(const uint32_t *tables, const int32_t *tab_idx,
                                                           const uint32_t *sc, uint32_t *out, int64_t n) {
  DX_TID();
  if (i < n) g2_mul_one(tables, tab_idx, sc, out, i);
}
// chunks of kCh consecutive digits per lane triple (as gt_entry_chunk_coop)
__global__ void __launch_bounds__(64) DX_OCC gt16_entry_chunk_coop(const uint32_t *pow2, uint32_t *table, int64_t n) {
  const coop::Role R = coop::role();
  const int64_t t = (int64_t)blockIdx.x * coop::kTriples + R.g;
  if (R.g >= coop::kTriples || t >= n) return;
  const int w = (int)(t / (kH16 / kCh)), d0 = (int)(t % (kH16 / kCh)) * kCh + 1;
  const Fp12 *Q = &at<Fp12>(pow2, w);
  Fp6 acc = coop::one(R);
  for (int bit = kB16 - 1; bit >= 0; bit--) {
    coop::mul(acc, acc, R);
    if ((d0 >> bit) & 1) coop::mul(acc, coop::load(Q, false, R), R);
  }
  const int64_t e0 = (int64_t)w * kH16 + d0 - 1;
  for (int j = 0; j < kCh; j++) {
    coop::store(&at<Fp12>(table, e0 + j), acc, R);
    if (j + 1 < kCh) coop::mul(acc, coop::load(Q, false, R), R);
  }
}
#undef DX_TID

inline dim3 grid_of(int64_t n) { return dim3((unsigned)((n + kWG - 1) / kWG)); }
inline dim3 grid_coop(int64_t n) { return dim3((unsigned)((n + coop::kTriples - 1) / coop::kTriples)); }
inline dim3 grid_pair(int64_t n) { return dim3((unsigned)((n + tp::kPairs - 1) / tp::kPairs)); }

// Rows per inversion of the finish pass: up to 4, but no more than keeps
// >= 2 waves per SIMD busy (as t2_chunk of dx_gt_t2.hip).  Measured at
// 993,600 rows (tools/gt_torus_bench.hip): 3.7 ms at 1, 2.6 ms at 4, 2.5 ms at 8.
inline int64_t finish_chunk_len(int64_t n) {
  const int64_t c = n / (1024 * 64 * 2);
  return c < 1 ? 1 : (c > 4 ? 4 : c);
}

// the builders' device flag, read once the stream has drained (set-up code: the sync is not on a query's path)
inline int read_flag(hipStream_t s, const uint32_t *flag, const char *what) {
  uint32_t h = 0;
  if (check_hip(hipGetLastError(), what)) return -1;
  if (check_hip(hipMemcpyAsync(&h, flag, 4, hipMemcpyDeviceToHost, s), what)) return -1;
  if (check_hip(hipStreamSynchronize(s), what)) return -1;
  return h ? 2 : 0;
}

}  // namespace

extern "C" {
int dx_gls8_entries() { return kEnt; }
int dx_gt16_entries() { return kW16 * kH16; }

// pow2[w] = gT^(2^(16w)) for w < 17 (host-computed), table [17*32768, 48] of
// beta rows; tmp (GPU path) [17*32768 + 1, 96]: the Fp12 powers and a flag
// row.  2: an entry is +-1 (gT is not a generator of the order-r group).
int dx_gt16_table(int on_gpu, void *stream, const uint32_t *pow2, uint32_t *table, uint32_t *tmp) {
  const int64_t n = (int64_t)kW16 * kH16;
  if (!on_gpu) {
    std::atomic<int> bad{0};
    host_for_each(n / kCh, [&](int64_t t) {
      if (!gt16_entry_chunk_one(pow2, table, t)) bad = 1;
    });
    return bad ? 2 : 0;
  }
  hipStream_t s = (hipStream_t)stream;
  uint32_t *flag = tmp + n * 96;
  if (check_hip(hipMemsetAsync(flag, 0, 4, s), "gt16_table")) return -1;
  hipLaunchKernelGGL(gt16_entry_chunk_coop, grid_coop(n / kCh), dim3(kWG), 0, s, pow2, tmp, n / kCh);
  hipLaunchKernelGGL(gt_beta_chunk_kernel, grid_of(n / kCh), dim3(kWG), 0, s, tmp, table, flag, n / kCh);
  return read_flag(s, flag, "gt16_table");
}

// table[b*2176 + w*128 + d-1] = d 2^(8w) A_b (affine); work [nb*17] Jacobian
int dx_g2_gls8_table(int on_gpu, void *stream, const uint32_t *bases_aff, uint32_t *work, uint32_t *table,
                     int64_t n_bases) {
  if (n_bases <= 0) return 0;
  if (!on_gpu) {
    host_for_each(n_bases, [=](int64_t b) { g2_pow_one(bases_aff, work, b); });
    host_for_each(n_bases * kChunks, [=](int64_t t) { g2_entry_chunk_one(work, table, t); });
    return 0;
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(g2_pow_kernel, grid_of(n_bases), dim3(kWG), 0, s, bases_aff, work, n_bases);
  hipLaunchKernelGGL(g2_entry_chunk_kernel, grid_of(n_bases * kChunks), dim3(kWG), 0, s, work, table,
                     n_bases * kChunks);
  return check_hip(hipGetLastError(), "g2_gls8_table");
}

// table[b*2176 + w*128 + d-1] = the beta image of E_b^(d 2^(8w)), [nb*2176, 48];
// work [nb*17, 96].  GPU path: the Fp12 powers of tmp_bases bases at a time go
// through tmp [tmp_bases*2176 + 1, 96] (the last row holds a flag).
// A base 1 gets unit-mark rows; 2: an entry g + 0 w is not 1 (only a base -1,
// or one that is not in the order-r group, has such an entry).
int dx_gt_gls8_table(int on_gpu, void *stream, const uint32_t *bases, uint32_t *work, uint32_t *table,
                     int64_t n_bases, uint32_t *tmp, int64_t tmp_bases) {
  if (n_bases <= 0) return 0;
  if (!on_gpu) {
    std::atomic<int> bad{0};
    host_for_each(n_bases, [=](int64_t b) { gt_pow_one(bases, work, b); });
    host_for_each(n_bases * kChunks, [&](int64_t t) {
      if (!gt_entry_chunk_one(work, table, t)) bad = 1;
    });
    return bad ? 2 : 0;
  }
  if (tmp_bases <= 0) return check_hip(hipErrorInvalidValue, "gt_gls8_table (no room for the Fp12 powers)");
  hipStream_t s = (hipStream_t)stream;
  uint32_t *flag = tmp + tmp_bases * kEnt * 96;
  if (check_hip(hipMemsetAsync(flag, 0, 4, s), "gt_gls8_table")) return -1;
  hipLaunchKernelGGL(gt_pow_kernel, grid_of(n_bases), dim3(kWG), 0, s, bases, work, n_bases);
  for (int64_t b0 = 0; b0 < n_bases; b0 += tmp_bases) {
    const int64_t nb = n_bases - b0 < tmp_bases ? n_bases - b0 : tmp_bases;
    hipLaunchKernelGGL(gt_entry_chunk_coop, grid_coop(nb * kChunks), dim3(kWG), 0, s, work + b0 * kWin * 96, tmp,
                       nb * kChunks);
    hipLaunchKernelGGL(gt_beta_chunk_kernel, grid_of(nb * kChunks), dim3(kWG), 0, s, tmp, table + b0 * kEnt * 48,
                       flag, nb * kChunks);
  }
  return read_flag(s, flag, "gt_gls8_table");
}

int dx_g2_gls8_mul(int on_gpu, void *stream, const uint32_t *tables, const int32_t *tab_idx, const uint32_t *scalars,
                   uint32_t *out_aff, int64_t n) {
  if (n <= 0) return 0;
  if (!on_gpu) {
    host_for_each(n, [=](int64_t i) { g2_mul_one(tables, tab_idx, scalars, out_aff, i); });
    return 0;
  }
  hipLaunchKernelGGL(g2_mul_kernel, grid_of(n), dim3(kWG), 0, (hipStream_t)stream, tables, tab_idx, scalars, out_aff,
                     n);
  return check_hip(hipGetLastError(), "g2_gls8_mul");
}

// a[it] = E_phi(it)^(e[it]) * gT^(t[p, j]): a numerator of the gT^t part once
// per (p, j), then the servers i >= 1 and server 0 in two launches (server 0's
// slot holds the gT^t numerator until its own launch overwrites it last), then
// every row's numerator to its canonical Fp12 value.  tmp (GPU path): [n_items, 96].
int dx_rp_prove_a_gls8(int on_gpu, void *stream, const uint32_t *gphi_tables, const int32_t *tab_idx,
                       const uint32_t *e_sc, const uint32_t *t_sc, const uint32_t *gt_table, uint32_t *a_out,
                       int64_t n_items, int S, int L, int t16, uint32_t *tmp) {
  if (n_items <= 0) return 0;
  const int64_t n_pj = n_items / S, n_p = n_pj / L;
  const int ranges[2][2] = {{1, S}, {0, 1}};
  if (!on_gpu) {
    host_for_each(n_pj, [=](int64_t pj) { prove_t_one(t_sc, gt_table, a_out, S, L, t16, pj); });
    for (auto &rg : ranges) {
      const int lo = rg[0], hi = rg[1];
      if (hi <= lo) continue;
      host_for_each(n_p * (hi - lo) * L,
                    [=](int64_t k) { prove_e_one(gphi_tables, tab_idx, e_sc, a_out, S, L, lo, hi, k); });
    }
    host_for_each(n_items, [=](int64_t i) { at<Fp12>(a_out, i) = torus::finish(at<Fp12>(a_out, i)); });
    return 0;
  }
  hipStream_t s = (hipStream_t)stream;
  if (!t16) return check_hip(hipErrorInvalidValue, "rp_prove_a_gls8 (the GPU path takes the 16-bit gT table)");
  hipLaunchKernelGGL(prove_t_pair, grid_pair(n_pj), dim3(kWG), 0, s, t_sc, gt_table, a_out, S, L, n_pj);
  for (auto &rg : ranges) {
    const int lo = rg[0], hi = rg[1];
    if (hi <= lo) continue;
    const int64_t n = n_p * (hi - lo) * L;
    hipLaunchKernelGGL(prove_e_pair, grid_pair(n), dim3(kWG), 0, s, gphi_tables, tab_idx, e_sc, a_out, S, L, lo, hi,
                       n);
  }
  const int64_t k = finish_chunk_len(n_items);
  hipLaunchKernelGGL(gt_finish_kernel, grid_of((n_items + k - 1) / k), dim3(kWG), 0, s, a_out, tmp, n_items, k);
  return check_hip(hipGetLastError(), "rp_prove_a_gls8");
}
}  // extern "C"
