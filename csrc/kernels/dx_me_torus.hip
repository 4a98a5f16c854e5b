// First pass of the range verifier's GT multi-exponentiation on torus images
// (gt_torus.h).
//
// The bucket products of prod a_ij^rho multiply a running value by a SOURCE
// element a_ij every time, and the a_ij are unitary (validate_list requires
// the cyclotomic subgroup).  With beta = (1 + g) / h of a = g + h w, a bucket's
// product runs on numerators, y <- y (beta + w): two Fp6 products on a lane
// pair instead of Karatsuba's three on a lane triple, over 192-byte rows
// instead of 384-byte ones, and the first factor of a slice is free
// (y = beta + w).  The slice results are ordinary Fp12 values -- numerators of
// the bucket products -- so every later pass of the multi-exponentiation (the
// tree over the lanes, the running-product weights, the per-window products)
// keeps the generic Fp12 kernels, and pi is taken once per (group, window) row
// at the end (dx_gt_pi).
//
//   dx_gt_beta_rows        a [m, 96] -> beta2 [2m, 48]: the images of a_i and
//                          of frob^8(a_i), one Fp6 inversion per chunk of rows
//   dx_gt_beta_slice_prod  numerators of the slice products over beta rows
//   dx_gt_pi               numerators -> canonical unitary Fp12 values
//
// The all-zero row is the skip mark: beta = 0 needs g = -1, which forces
// h = 0, so no element with an image has it; a = 1 is the only element
// validate_list accepts that has no image, and skipping it multiplies by 1.
//
// Every body is force-inlined into an explicit __global__ kernel (as
// dx_gls8.hip); host paths through host_for_each / run().
#define DX_NI __host__ __device__ __forceinline__
#include "common.h"
#include "../bn254/gt_torus.h"

using namespace dxk;

namespace {
constexpr int kWG = 64;
namespace tp = torus::pair;

// h with canonical limbs.  The kernel makes no validity test of its rows
// (validate_list does, on the same rows, and its verdict gates every use of
// the result), but a row it rejects must not spoil its neighbours: a
// non-canonical encoding of h = 0 that entered the shared inversion would zero
// the whole chunk, rows of other proofs included.  On canonical limbs this is
// the identity.
DX_HD Fp6 canon6(const Fp6 &h) {
  auto c2 = [](const Fp2 &a) { return Fp2{reduce_256<FpParams>(a.c0.v), reduce_256<FpParams>(a.c1.v)}; };
  return {c2(h.c0), c2(h.c1), c2(h.c2)};
}

// Image of frob^8(a) from the image beta of a.  frob^8 multiplies the
// coefficient of w^e by zeta^(4e), zeta = gamma_2[1] of order 6: on
// a = g + h w that is g -> phi(g), h -> zeta^4 phi(h) with phi the
// coefficient-wise map x_j -> zeta^(8j) x_j of Fp6 (a ring automorphism), so
// beta -> phi(beta) / zeta^4 (zeta^4 = w^(p^8 - 1)): coefficient j times
// zeta^(8j - 4) = zeta^2, zeta^4, 1.
DX_HD Fp6 frob8_image(const Fp6 &b) {
  return {dx::mul(b.c0, Fp2::from_limbs(Frob::G2[2])), dx::mul(b.c1, Fp2::from_limbs(Frob::G2[4])), b.c2};
}

DX_HD bool is_skip_row(const Fp6 &b) {
  const uint32_t *w = &b.c0.c0.v[0];
  uint32_t acc = 0;
#pragma unroll
  for (int i = 0; i < 48; i++) acc |= w[i];
  return acc == 0;
}

// beta2[i] = (1 + g_i) / h_i and beta2[m + i] = its frob^8 image for the rows
// [i0, i1) with ONE Fp6 inversion; the prefix products of Montgomery's trick
// are parked in the rows' own output slots (as compress_chunk of
// dx_gt_t2.hip): a lane keeps no per-chunk arrays.  Rows with h = 0 stay out
// of the chain and get the skip mark in both halves.
DX_HD void beta_rows_chunk(const uint32_t *a, uint32_t *beta2, int64_t m, int64_t i0, int64_t i1) {
  Fp6 acc = Fp6::one();
  for (int64_t i = i0; i < i1; i++) {
    const Fp6 h = canon6(at<Fp12>(a, i).c1);
    at<Fp6>(beta2, i) = acc;
    if (!(h == Fp6::zero())) acc = torus::mul6(acc, h);
  }
  Fp6 inv_all = inv(acc);
  for (int64_t i = i1 - 1; i >= i0; i--) {
    const Fp6 h = canon6(at<Fp12>(a, i).c1);
    if (h == Fp6::zero()) {
      at<Fp6>(beta2, i) = Fp6::zero();
      at<Fp6>(beta2, m + i) = Fp6::zero();
      continue;
    }
    const Fp6 hi = torus::mul6(inv_all, at<Fp6>(beta2, i));
    inv_all = torus::mul6(inv_all, h);
    const Fp6 b = torus::mul6(add(Fp6::one(), at<Fp12>(a, i).c0), hi);
    at<Fp6>(beta2, i) = b;
    at<Fp6>(beta2, m + i) = frob8_image(b);
  }
}

__global__ void __launch_bounds__(kWG) DX_OCC gt_beta_rows_kernel(const uint32_t *a, uint32_t *beta2, int64_t m,
                                                                 int64_t k, int64_t chunks) {
  const int64_t t = (int64_t)blockIdx.x * kWG + threadIdx.x;
  if (t >= chunks) return;
  const int64_t i0 = t * k, i1 = i0 + k < m ? i0 + k : m;
  beta_rows_chunk(a, beta2, m, i0, i1);
}

// One slice per lane pair, 32 slices per wave.  Both lanes of a pair read the
// same start, len and rows, so they take every branch -- and every DPP
// exchange of mul_beta -- together; pairs of different lengths or skip
// patterns diverge from each other only.
__global__ void __launch_bounds__(kWG) DX_OCC gt_beta_slice_prod_pair(const uint32_t *beta, const int64_t *idx,
                                                                     const int64_t *start, const int32_t *len,
                                                                     uint32_t *out, int64_t n_slices) {
  const tp::Role R = tp::role();
  const int64_t s = (int64_t)blockIdx.x * tp::kPairs + R.g;
  if (s >= n_slices) return;  // whole pairs leave together
  const int64_t b = start[s];
  const int n = len[s];
  const Fp6 *T = reinterpret_cast<const Fp6 *>(beta);
  Fp6 x = tp::one(R);
  int k = 0;
  for (; k < n; k++) {  // the first factor is free: y = beta + w
    const Fp6 bt = T[idx ? idx[b + k] : b + k];
    if (is_skip_row(bt)) continue;
    x = tp::sel6(R.r != 0, Fp6::one(), bt);
    k++;
    break;
  }
  for (; k < n; k++) {
    const Fp6 bt = T[idx ? idx[b + k] : b + k];
    if (!is_skip_row(bt)) tp::mul_beta(x, bt, false, R);
  }
  tp::store(&at<Fp12>(out, s), x, R);
}

inline dim3 grid_of(int64_t n) { return dim3((unsigned)((n + kWG - 1) / kWG)); }
inline dim3 grid_pair(int64_t n) { return dim3((unsigned)((n + tp::kPairs - 1) / tp::kPairs)); }
}  // namespace

extern "C" {
// a [m, 96] GT elements -> beta2 [2m, 48]: row i the image of a_i, row m + i
// the image of frob^8(a_i); rows_per_inv rows share one Fp6 inversion
int dx_gt_beta_rows(int on_gpu, void *stream, const uint32_t *a, uint32_t *beta2, int64_t m, int64_t rows_per_inv) {
  if (m <= 0) return 0;
  const int64_t k = rows_per_inv < 1 ? 1 : rows_per_inv;
  const int64_t chunks = (m + k - 1) / k;
  if (!on_gpu) {
    host_for_each(chunks, [=](int64_t t) {
      const int64_t i0 = t * k, i1 = i0 + k < m ? i0 + k : m;
      beta_rows_chunk(a, beta2, m, i0, i1);
    }, 2);
    return 0;
  }
  hipLaunchKernelGGL(gt_beta_rows_kernel, grid_of(chunks), dim3(kWG), 0, (hipStream_t)stream, a, beta2, m, k, chunks);
  return check_hip(hipGetLastError(), "gt_beta_rows");
}

// out[s] = a numerator of prod_k pi(beta[r_k] + w), r_k = idx ? idx[start[s] + k] : start[s] + k,
// k < len[s]; skip rows left out, Fp12::one() for an empty or all-skipped slice
int dx_gt_beta_slice_prod(int on_gpu, void *stream, const uint32_t *beta, const int64_t *idx, const int64_t *start,
                          const int32_t *len, uint32_t *out, int64_t n_slices) {
  if (n_slices <= 0) return 0;
  if (!on_gpu) {
    host_for_each(n_slices, [=](int64_t s) {
      const int64_t b = start[s];
      const int n = len[s];
      Fp12 y = Fp12::one();
      bool have = false;
      for (int k = 0; k < n; k++) {
        const Fp6 bt = at<Fp6>(beta, idx ? idx[b + k] : b + k);
        if (is_skip_row(bt)) continue;
        if (have) {
          torus::mul_beta(y, bt, false);
        } else {
          y = Fp12{bt, Fp6::one()};
          have = true;
        }
      }
      at<Fp12>(out, s) = y;
    });
    return 0;
  }
  hipLaunchKernelGGL(gt_beta_slice_prod_pair, grid_pair(n_slices), dim3(kWG), 0, (hipStream_t)stream, beta, idx,
                     start, len, out, n_slices);
  return check_hip(hipGetLastError(), "gt_beta_slice_prod");
}

// out[i] = pi(y[i]) = y / conj(y): the canonical unitary value of a numerator
int dx_gt_pi(int on_gpu, void *stream, const uint32_t *y, uint32_t *out, int64_t n) {
  auto op = [=] __host__ __device__(int64_t i) { at<Fp12>(out, i) = torus::finish(at<Fp12>(y, i)); };
  return run(on_gpu, stream, n, op, true, "gt_pi");
}
}  // extern "C"
