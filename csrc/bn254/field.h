// BN254 prime-field arithmetic (Fp and Fr), stored as 8 x 32-bit limbs in
// Montgomery form (R = 2^256).
//
// CDNA4 mapping: additions and subtractions run on the 32-bit words with the
// carry in VCC; a product unpacks its operands into nine 29-bit limbs, so that
// a whole column of limb products fits one 64-bit accumulator, and every limb
// product is one `v_mad_u64_u32` (32x32+64 -> 64) with nothing beside it (see
// "Montgomery products on nine 29-bit limbs" below).  Both moduli are below
// 2^254, which is what the bounds of that core rest on.
// One thread owns one field element (8 VGPRs); kernels are thread-per-item.
//
// The same inline functions are compiled for the host (CPU batch path used by
// the control plane and the CPU test-suite) and for gfx950 device kernels.
// Replaces kyber's bn256 gfP (reference: lib/suite.go:10, external kyber).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>
#include "constants.h"

#define DX_HD __host__ __device__ __forceinline__
// DX_NI: out-of-line tower/curve functions (small code, shared by the kernels
// of a translation unit).  A TU may predefine it as force-inline to get one
// register-allocated body per kernel instead (dx_fold.hip, dx_check_inl.hip).
#ifndef DX_NI
#define DX_NI __host__ __device__ __noinline__ inline
#endif
// The Montgomery multiply is force-inlined into device code (register
// allocation across a whole Fp2/Fp6 product) but kept out-of-line on the host,
// where x86 instruction selection of thousands of unrolled 64-bit MACs would
// otherwise dominate build time.
#ifdef __HIP_DEVICE_COMPILE__
#define DX_MUL DX_HD
#else
#define DX_MUL __host__ __device__ __noinline__ inline
#endif

namespace dx {

// Limb add/subtract with carry.  The clang builtins lower to one
// v_add_co/v_addc_co (v_sub_co/v_subb_co) per limb with the carry kept in
// VCC/an SGPR pair; the equivalent 64-bit C++ arithmetic was lowered to ~5
// VALU instructions per limb on gfx950 (materialised 0/1 carries, 64-bit
// adds, s_nop), which made the modular additions cost as much as the
// Montgomery products around them.
DX_HD uint32_t addc32(uint32_t a, uint32_t b, uint32_t &carry) {
  unsigned co;
  const uint32_t r = __builtin_addc(a, b, carry, &co);
  carry = co;
  return r;
}
DX_HD uint32_t subb32(uint32_t a, uint32_t b, uint32_t &borrow) {
  unsigned bo;
  const uint32_t r = __builtin_subc(a, b, borrow, &bo);
  borrow = bo;
  return r;
}

template <class PR>
struct FieldT {
  uint32_t v[8];

  static DX_HD FieldT zero() {
    FieldT r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = 0;
    return r;
  }
  static DX_HD FieldT one() {
    FieldT r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = PR::ONE[i];
    return r;
  }
  static DX_HD FieldT from_limbs(const uint32_t *p) {
    FieldT r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = p[i];
    return r;
  }
  DX_HD bool is_zero() const {
    uint32_t acc = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) acc |= v[i];
    return acc == 0;
  }
  DX_HD bool operator==(const FieldT &o) const {
    uint32_t acc = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) acc |= v[i] ^ o.v[i];
    return acc == 0;
  }
  DX_HD bool operator!=(const FieldT &o) const { return !(*this == o); }
};

// r = a if borrow==0 after t-MOD else t (i.e. conditional subtract of the modulus)
template <class PR>
DX_HD void cond_sub_mod(uint32_t *t) {
  uint32_t s[8];
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) s[i] = subb32(t[i], PR::MOD[i], borrow);
  // borrow==1 -> t < MOD -> keep t
#pragma unroll
  for (int i = 0; i < 8; i++) t[i] = borrow ? t[i] : s[i];
}

template <class PR>
DX_HD FieldT<PR> fadd(const FieldT<PR> &a, const FieldT<PR> &b) {
  FieldT<PR> r;
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = addc32(a.v[i], b.v[i], c);
  cond_sub_mod<PR>(r.v);
  return r;
}

template <class PR>
DX_HD FieldT<PR> fsub(const FieldT<PR> &a, const FieldT<PR> &b) {
  FieldT<PR> r;
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = subb32(a.v[i], b.v[i], br);
  uint32_t mask = 0u - br;
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = addc32(r.v[i], PR::MOD[i] & mask, c);
  return r;
}

template <class PR>
DX_HD FieldT<PR> fneg(const FieldT<PR> &a) {
  return fsub(FieldT<PR>::zero(), a);
}

template <class PR>
DX_HD FieldT<PR> fdbl(const FieldT<PR> &a) {
  return fadd(a, a);
}

// ---------------------------------------------------------------------------
// Montgomery products on nine 29-bit limbs.
//
// Storage stays 8 x 32 bits and the Montgomery constant stays R = 2^256.  A
// product unpacks its operands into nine 29-bit limbs, runs a product-scanning
// REDC with R' = 2^261 (nine uniform 29-bit digits) on (a << 5) * b, and packs
// the result back: ((a << 5) b + m p) / 2^261 = (a b + m' p) / 2^256 mod p.
// A limb product is below 2^58, so a whole column (up to 27 of them plus the
// carry of the previous column) fits one uint64_t: there is no carry word, no
// add-with-carry per limb product and no inline asm, and the host runs the
// same code.  Each `acc += (uint64_t)x * y` is one v_mad_u64_u32 on gfx950.
namespace l29 {
constexpr uint32_t M29 = (1u << 29) - 1;

// bits [29 k, 29 k + 29) of a little-endian 8 x 32-bit integer (compile time)
constexpr uint32_t climb(const uint32_t (&w)[8], int k) {
  uint32_t r = 0;
  for (int b = 0; b < 29; b++) {
    const int bit = 29 * k + b;
    if (bit < 256 && ((w[bit / 32] >> (bit % 32)) & 1u)) r |= 1u << b;
  }
  return r;
}

// Limbs of the modulus and -MOD^-1 mod 2^29 (the low 29 bits of the 32-bit
// Montgomery constant).  MOD < 2^254, so P[8] < 2^22.
template <class PR>
struct Mod {
  static constexpr uint32_t P[9] = {climb(PR::MOD, 0), climb(PR::MOD, 1), climb(PR::MOD, 2),
                                    climb(PR::MOD, 3), climb(PR::MOD, 4), climb(PR::MOD, 5),
                                    climb(PR::MOD, 6), climb(PR::MOD, 7), climb(PR::MOD, 8)};
  static constexpr uint32_t NINV = PR::INV & M29;
};

// L[k] = bits [29 k, 29 k + 29) of (w << SH), SH in {0, 5}, for any w < 2^256.
// Out: L[0..8] < 2^29; for SH = 0, L[8] < 2^24.  Every shift count is a
// compile-time constant in [0, 31]: the low limb of a pre-shifted value is a
// left shift of word 0 alone, a limb that starts at bit s <= 3 of its word
// needs no second word, and limb 8 ends in word 7.
template <int SH>
DX_HD void unpack(const uint32_t *w, uint32_t *L) {
  static_assert(SH == 0 || SH == 5, "pre-shift is 0 or 5 bits");
#pragma unroll
  for (int k = 0; k < 9; k++) {
    const int lo = 29 * k - SH;  // first bit of w in limb k
    if (lo < 0) {
      L[k] = (w[0] << SH) & M29;
    } else {
      const int j = lo / 32, s = lo % 32;
      uint32_t x = w[j] >> s;
      if (s > 3 && j + 1 < 8) x |= w[j + 1] << (32 - s);
      L[k] = x & M29;
    }
  }
}

// The column loop: REDC_{2^261}(A B [+ C D]) on limbs.
// In : A, C < 2^29 per limb (a value << 5); B, D < 2^29 per limb, values
//      below 2^256.
// Col: at most 9 (A B) + 9 (C D) + 9 (m P) products below 2^58 plus a carry
//      below 2^36: < 27 * 2^58 + 2^36 < 2^63.
// Out: u[0..7] < 2^29 and u[8], the value ((a << 5) b [+ (c << 5) d] + m p)
//      / 2^261 < (a b [+ c d]) / 2^256 + p.  For a, c < 2^256 and b, d < p
//      that is below 2 p [3 p], so u[8] < 2^24 and pack() is exact; for
//      a, b, c, d < p it is below 1.2 p [1.4 p].
template <class PR, bool TWO>
DX_HD void redc_cols(const uint32_t *A, const uint32_t *B, const uint32_t *C, const uint32_t *D, uint32_t *u) {
  using MP = Mod<PR>;
  uint32_t m[9];
  uint64_t acc = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) {
#pragma unroll
    for (int j = 0; j <= i; j++) {
      acc += (uint64_t)A[j] * B[i - j];
      if (TWO) acc += (uint64_t)C[j] * D[i - j];
      if (j < i) acc += (uint64_t)m[j] * MP::P[i - j];
    }
    m[i] = ((uint32_t)acc * MP::NINV) & M29;
    acc += (uint64_t)m[i] * MP::P[0];
    acc >>= 29;
  }
#pragma unroll
  for (int i = 9; i < 17; i++) {
#pragma unroll
    for (int j = i - 8; j < 9; j++) {
      acc += (uint64_t)A[j] * B[i - j];
      if (TWO) acc += (uint64_t)C[j] * D[i - j];
      acc += (uint64_t)m[j] * MP::P[i - j];
    }
    u[i - 9] = (uint32_t)acc & M29;
    acc >>= 29;
  }
  u[8] = (uint32_t)acc;
}

// Nine limbs (u[0..7] < 2^29, u[8] < 2^24) of a value below 2 MOD -> canonical
// 8 x 32.  Word k starts at bit s = 32 k - 29 j of limb j = 32 k / 29; s is
// one of 0, 3, .., 21, so both shift counts (s and 29 - s) stay in [0, 29].
template <class PR>
DX_HD FieldT<PR> pack(const uint32_t *u) {
  uint32_t t[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int j = (32 * k) / 29, s = 32 * k - 29 * j;
    t[k] = (u[j] >> s) | (u[j + 1] << (29 - s));
  }
  cond_sub_mod<PR>(t);
  FieldT<PR> r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = t[i];
  return r;
}
}  // namespace l29

// Montgomery product a b 2^-256 mod MOD, canonical.  In: a < 2^256, b < MOD
// (or the other way round).  Before the conditional subtraction the value is
// below 2 MOD (below 1.2 MOD for a, b < MOD).
template <class PR>
DX_MUL FieldT<PR> fmul29(const FieldT<PR> &a, const FieldT<PR> &b) {
  uint32_t A[9], B[9], u[9];
  l29::unpack<5>(a.v, A);
  l29::unpack<0>(b.v, B);
  l29::redc_cols<PR, false>(A, B, A, B, u);
  return l29::pack<PR>(u);
}

// Sum of two products (a b + c d) 2^-256 mod MOD, canonical, in one reduced
// column chain.  In: a, b, c, d <= MOD.  Before the conditional subtraction
// the value is below MOD (1 + 2 MOD / 2^256) < 1.4 MOD.
template <class PR>
DX_MUL FieldT<PR> fmul2_29(const FieldT<PR> &a, const FieldT<PR> &b, const FieldT<PR> &c, const FieldT<PR> &d) {
  uint32_t A[9], B[9], C[9], D[9], u[9];
  l29::unpack<5>(a.v, A);
  l29::unpack<0>(b.v, B);
  l29::unpack<5>(c.v, C);
  l29::unpack<0>(d.v, D);
  l29::redc_cols<PR, true>(A, B, C, D, u);
  return l29::pack<PR>(u);
}

// MOD - a for a < MOD: in (0, MOD], a valid operand of the products above
// (not canonical for a = 0).
template <class PR>
DX_HD FieldT<PR> mod_minus(const FieldT<PR> &a) {
  FieldT<PR> r;
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = subb32(PR::MOD[i], a.v[i], br);
  return r;
}

template <class PR>
DX_HD FieldT<PR> fmul(const FieldT<PR> &a, const FieldT<PR> &b) {
  return fmul29(a, b);
}
// (a b + c d) 2^-256 mod MOD for a, b, c, d <= MOD
template <class PR>
DX_HD FieldT<PR> fmul2(const FieldT<PR> &a, const FieldT<PR> &b, const FieldT<PR> &c, const FieldT<PR> &d) {
  return fmul2_29(a, b, c, d);
}

template <class PR>
DX_HD FieldT<PR> fsqr(const FieldT<PR> &a) {
  return fmul(a, a);
}

// a^e for a little-endian 8-limb exponent (square-and-multiply, MSB first).
template <class PR>
DX_NI FieldT<PR> fpow(const FieldT<PR> &a, const uint32_t *e) {
  FieldT<PR> r = FieldT<PR>::one();
  for (int i = 7; i >= 0; i--) {
    for (int b = 31; b >= 0; b--) {
      r = fsqr(r);
      if ((e[i] >> b) & 1u) r = fmul(r, a);
    }
  }
  return r;
}

// Inverse of a Montgomery-form element (a = xR -> x^-1 R), constant time:
// Bernstein-Yang "safegcd" with half-delta divsteps (the variant and the
// 10 x 59 = 590-step bound for 256-bit moduli of libsecp256k1's modinv64;
// written here from the published algorithm).  The divsteps run on the low
// 64 bits of (f, g) alone, 59 at a time, accumulating a 2x2 transition
// matrix scaled by 2^62; each batch then applies the matrix to the full
// 5 x 62-bit signed limbs of f, g and of the Bezout tracker (d, e) (mod p,
// with a p multiple that clears the low 62 bits before the shift).  Starting
// e at R^2 mod p makes d = R^2 (xR)^-1 = x^-1 R directly.  ~590 x 16 simple
// 64-bit ops plus 10 x 44 64x64 products: ~4x fewer VALU instructions than
// the bitwise binary GCD it replaces (510 steps over 8-limb values).
namespace inv62 {
using i64 = int64_t;
using u64 = uint64_t;
using i128 = __int128;
constexpr u64 M62 = ~0ull >> 2;

// bits [62 k, 62 k + 62) of a little-endian 8 x 32-bit integer
constexpr i64 limb(const uint32_t (&w)[8], int k) {
  u64 r = 0;
  for (int b = 0; b < 62; b++) {
    const int bit = 62 * k + b;
    if (bit < 256 && ((w[bit / 32] >> (bit % 32)) & 1u)) r |= 1ull << b;
  }
  return (i64)r;
}
// p^-1 mod 2^62 (Newton: each step doubles the correct low bits; p odd)
constexpr u64 inv_mod62(const uint32_t (&w)[8]) {
  const u64 p0 = (u64)w[0] | ((u64)w[1] << 32);
  u64 x = p0;  // correct mod 2^3 for odd p
  for (int i = 0; i < 6; i++) x *= 2 - p0 * x;
  return x & M62;
}

DX_HD i64 divsteps59(i64 zeta, u64 f, u64 g, i64 &tu, i64 &tv, i64 &tq, i64 &tr) {
  u64 u = 8, v = 0, q = 0, r = 8;  // identity x 2^3: 59 steps later the matrix carries 2^62
  for (int i = 3; i < 62; i++) {
    u64 m1 = (u64)(zeta >> 63);    // zeta < 0
    const u64 m2 = 0 - (g & 1);    // g odd
    const u64 x = (f ^ m1) - m1, y = (u ^ m1) - m1, z = (v ^ m1) - m1;
    g += x & m2;
    q += y & m2;
    r += z & m2;
    m1 &= m2;                      // zeta < 0 and g odd: swap (f <- g, zeta <- -zeta - 2)
    zeta = (zeta ^ (i64)m1) - 1;
    f += g & m1;
    u += q & m1;
    v += r & m1;
    g >>= 1;
    u <<= 1;
    v <<= 1;
  }
  tu = (i64)u;
  tv = (i64)v;
  tq = (i64)q;
  tr = (i64)r;
  return zeta;
}

// [f, g] <- t [f, g] / 2^62 (exact)
DX_HD void update_fg(i64 *f, i64 *g, i64 u, i64 v, i64 q, i64 r) {
  i128 cf = (i128)u * f[0] + (i128)v * g[0];
  i128 cg = (i128)q * f[0] + (i128)r * g[0];
  cf >>= 62;
  cg >>= 62;
#pragma unroll
  for (int k = 1; k < 5; k++) {
    cf += (i128)u * f[k] + (i128)v * g[k];
    cg += (i128)q * f[k] + (i128)r * g[k];
    f[k - 1] = (i64)((u64)cf & M62);
    g[k - 1] = (i64)((u64)cg & M62);
    cf >>= 62;
    cg >>= 62;
  }
  f[4] = (i64)cf;
  g[4] = (i64)cg;
}

// [d, e] <- (t [d, e] + p [md, me]) / 2^62, md / me chosen so the division is exact
// and d, e stay in (-2p, p)
DX_HD void update_de(i64 *d, i64 *e, i64 u, i64 v, i64 q, i64 r, const i64 *P, u64 pinv) {
  const i64 sd = d[4] >> 63, se = e[4] >> 63;
  i64 md = (u & sd) + (v & se);
  i64 me = (q & sd) + (r & se);
  i128 cd = (i128)u * d[0] + (i128)v * e[0];
  i128 ce = (i128)q * d[0] + (i128)r * e[0];
  md -= (i64)((pinv * (u64)cd + (u64)md) & M62);
  me -= (i64)((pinv * (u64)ce + (u64)me) & M62);
  cd += (i128)P[0] * md;
  ce += (i128)P[0] * me;
  cd >>= 62;
  ce >>= 62;
#pragma unroll
  for (int k = 1; k < 5; k++) {
    cd += (i128)u * d[k] + (i128)v * e[k] + (i128)P[k] * md;
    ce += (i128)q * d[k] + (i128)r * e[k] + (i128)P[k] * me;
    d[k - 1] = (i64)((u64)cd & M62);
    e[k - 1] = (i64)((u64)ce & M62);
    cd >>= 62;
    ce >>= 62;
  }
  d[4] = (i64)cd;
  e[4] = (i64)ce;
}

// d in (-2p, p), negated if sign < 0 -> [0, p)
DX_HD void normalize(i64 *d, i64 sign, const i64 *P) {
  i64 c = d[4] >> 63;
#pragma unroll
  for (int k = 0; k < 5; k++) d[k] += P[k] & c;
  const i64 n = sign >> 63;
#pragma unroll
  for (int k = 0; k < 5; k++) d[k] = (d[k] ^ n) - n;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    d[k + 1] += d[k] >> 62;
    d[k] &= (i64)M62;
  }
  c = d[4] >> 63;
#pragma unroll
  for (int k = 0; k < 5; k++) d[k] += P[k] & c;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    d[k + 1] += d[k] >> 62;
    d[k] &= (i64)M62;
  }
}
}  // namespace inv62

template <class PR>
DX_NI FieldT<PR> finv(const FieldT<PR> &a) {
  using namespace inv62;
  constexpr i64 P0 = limb(PR::MOD, 0), P1 = limb(PR::MOD, 1), P2 = limb(PR::MOD, 2), P3 = limb(PR::MOD, 3),
                P4 = limb(PR::MOD, 4);
  constexpr i64 E0 = limb(PR::R2, 0), E1 = limb(PR::R2, 1), E2 = limb(PR::R2, 2), E3 = limb(PR::R2, 3),
                E4 = limb(PR::R2, 4);
  constexpr u64 PINV = inv_mod62(PR::MOD);
  const i64 P[5] = {P0, P1, P2, P3, P4};
  i64 f[5] = {P0, P1, P2, P3, P4};
  i64 e[5] = {E0, E1, E2, E3, E4};
  i64 d[5] = {0, 0, 0, 0, 0};
  i64 g[5];
  const uint32_t *w = a.v;
  g[0] = (i64)(((u64)w[0] | ((u64)w[1] << 32)) & M62);
  g[1] = (i64)((((u64)w[1] >> 30) | ((u64)w[2] << 2) | ((u64)w[3] << 34)) & M62);
  g[2] = (i64)((((u64)w[3] >> 28) | ((u64)w[4] << 4) | ((u64)w[5] << 36)) & M62);
  g[3] = (i64)((((u64)w[5] >> 26) | ((u64)w[6] << 6) | ((u64)w[7] << 38)) & M62);
  g[4] = (i64)((u64)w[7] >> 24);
  i64 zeta = -1;  // -(delta + 1/2), delta = 1/2
  for (int it = 0; it < 10; it++) {
    i64 u, v, q, r;
    zeta = divsteps59(zeta, (u64)f[0], (u64)g[0], u, v, q, r);
    update_de(d, e, u, v, q, r, P, PINV);
    update_fg(f, g, u, v, q, r);
  }
  normalize(d, f[4], P);  // g = 0, f = +-1: d = +- R^2 a^-1
  FieldT<PR> out;
  out.v[0] = (uint32_t)d[0];
  out.v[1] = (uint32_t)(((u64)d[0] >> 32) | ((u64)d[1] << 30));
  out.v[2] = (uint32_t)((u64)d[1] >> 2);
  out.v[3] = (uint32_t)(((u64)d[1] >> 34) | ((u64)d[2] << 28));
  out.v[4] = (uint32_t)((u64)d[2] >> 4);
  out.v[5] = (uint32_t)(((u64)d[2] >> 36) | ((u64)d[3] << 26));
  out.v[6] = (uint32_t)((u64)d[3] >> 6);
  out.v[7] = (uint32_t)(((u64)d[3] >> 38) | ((u64)d[4] << 24));
  return out;
}

// canonical integer (limbs, little endian) <-> Montgomery
template <class PR>
DX_HD FieldT<PR> to_mont(const FieldT<PR> &a) {
  return fmul(a, FieldT<PR>::from_limbs(PR::R2));
}
template <class PR>
DX_HD FieldT<PR> from_mont(const FieldT<PR> &a) {
  FieldT<PR> one = FieldT<PR>::zero();
  one.v[0] = 1;
  return fmul(a, one);
}

// Reduce an arbitrary 256-bit integer (little-endian limbs) below MOD.
// Inputs are < 2^256 < 6*MOD, so at most 5 subtractions are needed.
template <class PR>
DX_HD FieldT<PR> reduce_256(const uint32_t *x) {
  FieldT<PR> r = FieldT<PR>::from_limbs(x);
  for (int k = 0; k < 5; k++) cond_sub_mod<PR>(r.v);
  return r;
}

using Fp = FieldT<FpParams>;
using Fr = FieldT<FrParams>;

}  // namespace dx
