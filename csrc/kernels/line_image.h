// The raw line-coefficient image of the U-side fold, written by
// rp_coeffs_kernel (dx_fold.hip) and read by ufold_coop_raw_kernel
// (dx_ufold_coop.hip): per Miller step s < kMillerSteps and item it < n the
// three Fp2 coefficients (c0, c1, c3) of the step's line, which at P = (x, y)
// is c0 y + (c1 x) w + c3 w^3.  Layout [step][12][n] uint4: word q (0..11) of
// step s, item it at img[(s * 12 + q) * n + it] (192 B per step and item, every
// uint4 access of a wave contiguous).
#pragma once
#include "common.h"

namespace dxk {

__device__ __forceinline__ void store_line(uint4 *img, int64_t n, int s, int64_t it, const Fp2 &c0, const Fp2 &c1,
                                           const Fp2 &c3) {
  const Fp2 *src[3] = {&c0, &c1, &c3};
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(src[c]);
#pragma unroll
    for (int q = 0; q < 4; q++)
      img[((int64_t)s * 12 + c * 4 + q) * n + it] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
  }
}

__device__ __forceinline__ void load_line(const uint4 *__restrict__ img, int64_t n, int s, int64_t it, Fp2 &c0,
                                          Fp2 &c1, Fp2 &c3) {
  Fp2 *dst[3] = {&c0, &c1, &c3};
#pragma unroll
  for (int c = 0; c < 3; c++) {
    uint32_t *w = reinterpret_cast<uint32_t *>(dst[c]);
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const uint4 v = img[((int64_t)s * 12 + c * 4 + q) * n + it];
      w[4 * q] = v.x;
      w[4 * q + 1] = v.y;
      w[4 * q + 2] = v.z;
      w[4 * q + 3] = v.w;
    }
  }
}

}  // namespace dxk
