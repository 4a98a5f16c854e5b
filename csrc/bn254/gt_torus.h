// GT product chains on torus (T2) images: TWO Fp6 products per step.
//
// A unitary f = g + h w (h != 0) is (beta + w) / (beta - w) with
// beta = (1 + g) / h in Fp6 -- the image dx_gt_t2.hip stores in the ledger.
// For any non-zero y = N + D w in Fp12 let pi(y) = y / conj(y).  pi is
// multiplicative, commutes with the Frobenius, ignores a non-zero Fp6 factor
// of y (conj fixes Fp6), and pi(beta + w) = f.  So a chain prod f_k runs on
// numerators,
//   y <- y (beta_k + w):   N' = N beta + v D,   D' = D beta + N,
// two Fp6 products by the SAME beta instead of Karatsuba's three, and pi is
// taken once at the end: pi(y) = y^2 / (N^2 - v D^2), one Fp6 inversion.
// f^-1 is beta -> -beta.  A valid state never becomes 0 (that needs
// beta^2 = v, a non-square), and it is an ordinary Fp12 value: generic Fp12
// products of numerators are numerators of the product.
//
// Host code and one-lane device code work on y as an Fp12 (num_of, mul_beta,
// finish, finish_chunk); the chain kernels put one item on a PAIR
// of lanes (pair::), lane 2g: N, lane 2g + 1: D, 32 items per 64-lane wave.
// One step is one Fp6 product per lane, one 48-dword exchange inside the pair
// (DPP quad_perm: no LDS traffic), mul_v on the N lane and an Fp6 addition.
// The two lanes of a pair must take every exchange together: kernels drop or
// keep whole pairs.
#pragma once
#include "tower.h"

namespace dx {
namespace torus {

// tower.h's Karatsuba Fp6 product, force-inlined whatever DX_NI is in the
// including translation unit (as coop::mul6)
__host__ __device__ __forceinline__ Fp6 mul6(const Fp6 &a, const Fp6 &b) {
  Fp2 t0 = dx::mul(a.c0, b.c0), t1 = dx::mul(a.c1, b.c1), t2 = dx::mul(a.c2, b.c2);
  Fp2 c0 = add(t0, mul_xi(sub(sub(dx::mul(add(a.c1, a.c2), add(b.c1, b.c2)), t1), t2)));
  Fp2 c1 = add(sub(sub(dx::mul(add(a.c0, a.c1), add(b.c0, b.c1)), t0), t1), mul_xi(t2));
  Fp2 c2 = add(sub(sub(dx::mul(add(a.c0, a.c2), add(b.c0, b.c2)), t0), t2), t1);
  return {c0, c1, c2};
}

// ---- whole numerators (host, one-lane device code)
// a numerator of the unitary f (any f but -1; f = 1 gives the Fp6 element 2)
DX_HD Fp12 num_of(const Fp12 &f) { return {add(Fp6::one(), f.c0), f.c1}; }

// y <- y (beta + w), or y (-beta + w): a numerator of pi(y) / f
DX_HD void mul_beta(Fp12 &y, const Fp6 &beta, bool negate) {
  const Fp6 n = mul6(y.c0, beta), d = mul6(y.c1, beta);
  const Fp6 vd = mul_v(y.c1);
  y = negate ? Fp12{sub(vd, n), sub(y.c0, d)} : Fp12{add(n, vd), add(d, y.c0)};
}

DX_HD Fp6 norm_of(const Fp12 &y) { return sub(sqr(y.c0), mul_v(sqr(y.c1))); }

// pi(y) from 1 / norm:  (N^2 + v D^2 + 2 N D w) / norm = 1 + 2 v D q + 2 N q w,
// q = D / norm -- exactly Fp12::one() for D = 0
DX_HD Fp12 pi_from(const Fp12 &y, const Fp6 &norm_inv) {
  const Fp6 q = mul6(y.c1, norm_inv);
  const Fp6 a = mul_v(mul6(y.c1, q)), b = mul6(y.c0, q);
  return {add(Fp6::one(), add(a, a)), add(b, b)};
}

// canonical value of pi(y), optionally times T
DX_HD Fp12 finish(const Fp12 &y) { return pi_from(y, inv(norm_of(y))); }
DX_HD Fp12 finish(const Fp12 &y, const Fp12 &T) { return mul(finish(y), T); }

// a[i] <- pi(a[i]) for a chunk [i0, i1) with ONE Fp6 inversion (Montgomery's
// trick).  tmp[i] (an Fp12 per row) parks the prefix product and the row's
// norm between the two passes: a lane keeps no per-chunk arrays.
DX_HD void finish_chunk(Fp12 *a, Fp12 *tmp, int64_t i0, int64_t i1) {
  Fp6 acc = Fp6::one();
  for (int64_t i = i0; i < i1; i++) {
    const Fp6 n = norm_of(a[i]);
    tmp[i].c0 = acc;
    tmp[i].c1 = n;
    acc = mul6(acc, n);
  }
  Fp6 inv_all = inv(acc);
  for (int64_t i = i1 - 1; i >= i0; i--) {
    const Fp6 ni = mul6(inv_all, tmp[i].c0);
    inv_all = mul6(inv_all, tmp[i].c1);
    a[i] = pi_from(a[i], ni);
  }
}

#ifdef __HIPCC__
// ---- one item on a pair of lanes (device code)
namespace pair {

constexpr int kPairs = 32;  // items per 64-lane wave

struct Role {
  int r;  // 0: holds N, 1: holds D
  int g;  // pair index in the wave (0..31)
};

__device__ __forceinline__ Role role() {
  const int lane = threadIdx.x & 63;
  return {lane & 1, lane >> 1};
}

// value of `a` in the other lane of the pair
__device__ __forceinline__ Fp6 swap6(const Fp6 &a) {
  Fp6 out;
  const uint32_t *pa = &a.c0.c0.v[0];
  uint32_t *po = &out.c0.c0.v[0];
#pragma unroll
  for (int i = 0; i < 48; i++)
    po[i] = (uint32_t)__builtin_amdgcn_update_dpp((int)pa[i], (int)pa[i], 0xB1 /* quad_perm [1,0,3,2] */, 0xF, 0xF, false);
  return out;
}

// word-wise select: v_cndmask, never a branch (a ternary on whole Fp6 values
// becomes divergent control flow and costs the chain kernels ~230 B of scratch)
__device__ __forceinline__ Fp6 sel6(bool c, const Fp6 &a, const Fp6 &b) {
  Fp6 out;
  const uint32_t *pa = &a.c0.c0.v[0], *pb = &b.c0.c0.v[0];
  uint32_t *po = &out.c0.c0.v[0];
#pragma unroll
  for (int i = 0; i < 48; i++) po[i] = c ? pa[i] : pb[i];
  return out;
}

// role half of the numerator 1
__device__ __forceinline__ Fp6 one(const Role &R) { return R.r ? Fp6::zero() : Fp6::one(); }

// role half of *y
__device__ __forceinline__ Fp6 load(const Fp12 *y, const Role &R) { return R.r ? y->c1 : y->c0; }

// x <- role half of y (beta + w) (negate: of y (-beta + w)); both lanes pass the same beta
__device__ __forceinline__ void mul_beta(Fp6 &x, const Fp6 &beta, bool negate, const Role &R) {
  const Fp6 t = mul6(x, sel6(negate, neg(beta), beta));
  const Fp6 o = swap6(x);  // N lane: D ; D lane: N
  x = add(t, sel6(R.r != 0, o, mul_v(o)));
}

// x <- role half of y * b for a whole numerator (or any Fp12) b in memory:
// N' = N b0 + v D b1,  D' = D b0 + N b1 -- four Fp6 products, two per lane
__device__ __forceinline__ void mul_full(Fp6 &x, const Fp12 *b, const Role &R) {
  const Fp6 u = mul6(swap6(x), b->c1);
  x = add(mul6(x, b->c0), sel6(R.r != 0, u, mul_v(u)));
}

// x <- role half of frob<1>(y): conjugation times gamma_1[e], e the
// w-exponent -- even on the N lane, odd on the D lane (coop::frob1's rule)
__device__ __forceinline__ void frob1(Fp6 &x, const Role &R) {
  auto f = [&](const Fp2 &a, int e) { return dx::mul(conj(a), Fp2::from_limbs(Frob::G1[e])); };
  x = {f(x.c0, R.r), f(x.c1, 2 + R.r), f(x.c2, 4 + R.r)};
}

// the whole numerator (each lane writes its half)
__device__ __forceinline__ void store(Fp12 *out, const Fp6 &x, const Role &R) {
  if (R.r) out->c1 = x;
  else out->c0 = x;
}

}  // namespace pair
#endif

}  // namespace torus
}  // namespace dx
