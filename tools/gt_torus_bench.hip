// Microbenchmark: the range prover's GT chains on torus images
// (csrc/bn254/gt_torus.h) against the three-lane Fp12 chain (gt_coop.h).
//
//   B3:  three lanes per item, f <- f * T[e] (or * conj(T[e])) on Fp12 entries
//   P2:  a lane pair per item, y <- y * (+-beta[e] + w) on Fp6 images
//   FIN: a[i] <- pi(a[i]), one lane per chunk of items, one inversion per chunk
//
// The P2 result of a sample of items is checked on the host against the plain
// Fp12 product of the decompressed entries.
//
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -I csrc tools/gt_torus_bench.hip -o build/gt_torus_bench
// Run:   build/gt_torus_bench [items] [products] [table_entries]
#define DX_NI __host__ __device__ __forceinline__
#include "kernels/common.h"
#include "bn254/gt_coop.h"
#include "bn254/gt_torus.h"

#include <random>
#include <vector>

namespace {
constexpr int kWG = 64;
namespace tp = dx::torus::pair;

__global__ void __launch_bounds__(kWG) DX_OCC chain_b3(const Fp12 *T, const uint32_t *idx, Fp12 *out, int64_t n, int K) {
  const coop::Role R = coop::role();
  const int64_t i = (int64_t)blockIdx.x * coop::kTriples + R.g;
  if (R.g >= coop::kTriples || i >= n) return;
  Fp6 x = coop::one(R);
  for (int k = 0; k < K; k++) {
    const uint32_t e = idx[i * K + k];
    coop::mul(x, coop::load(T + (e >> 1), e & 1, R), R);
  }
  coop::store(out + i, x, R);
}

__global__ void __launch_bounds__(kWG) DX_OCC chain_p2(const Fp6 *B, const uint32_t *idx, Fp12 *out, int64_t n, int K) {
  const tp::Role R = tp::role();
  const int64_t i = (int64_t)blockIdx.x * tp::kPairs + R.g;
  if (i >= n) return;
  Fp6 x = tp::one(R);
  for (int k = 0; k < K; k++) {
    const uint32_t e = idx[i * K + k];
    tp::mul_beta(x, B[e >> 1], e & 1, R);
  }
  tp::store(out + i, x, R);
}

__global__ void __launch_bounds__(kWG) DX_OCC finish_k(Fp12 *a, Fp12 *tmp, int64_t n, int64_t k) {
  const int64_t t = (int64_t)blockIdx.x * kWG + threadIdx.x;
  const int64_t i0 = t * k, i1 = i0 + k < n ? i0 + k : n;
  if (i0 < n) torus::finish_chunk(a, tmp, i0, i1);
}

void check(hipError_t e, const char *w) {
  if (e != hipSuccess) {
    fprintf(stderr, "%s: %s\n", w, hipGetErrorString(e));
    exit(1);
  }
}

template <class F>
float best_of(int reps, F launch) {
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  float best = 1e30f;
  for (int rep = 0; rep < reps; rep++) {
    hipEventRecord(e0);
    launch();
    hipEventRecord(e1);
    check(hipEventSynchronize(e1), "sync");
    float ms;
    hipEventElapsedTime(&ms, e0, e1);
    if (ms < best) best = ms;
  }
  return best;
}
}  // namespace

int main(int argc, char **argv) {
  const int64_t n = argc > 1 ? atoll(argv[1]) : 993600;
  const int K = argc > 2 ? atoi(argv[2]) : 34;
  const int64_t nt = argc > 3 ? atoll(argv[3]) : (1 << 20);
  std::mt19937_64 rng(7);
  std::vector<Fp6> B(nt);
  for (auto &t : B) {
    uint32_t *p = &t.c0.c0.v[0];
    for (int i = 0; i < 48; i++) p[i] = (uint32_t)rng();
    for (int c = 0; c < 6; c++) p[8 * c + 7] &= 0x0fffffffu;  // < p
  }
  std::vector<Fp12> T(nt);  // B3 operands: timing only (any canonical limbs)
  for (int64_t i = 0; i < nt; i++) T[i] = {B[i], B[(i + 1) % nt]};
  std::vector<uint32_t> idx((size_t)n * K);
  for (auto &v : idx) v = (uint32_t)(rng() % (uint64_t)(2 * nt));
  Fp12 *dT, *dO, *dTmp;
  Fp6 *dB;
  uint32_t *dI;
  check(hipMalloc(&dT, nt * sizeof(Fp12)), "malloc");
  check(hipMalloc(&dB, nt * sizeof(Fp6)), "malloc");
  check(hipMalloc(&dO, n * sizeof(Fp12)), "malloc");
  check(hipMalloc(&dTmp, n * sizeof(Fp12)), "malloc");
  check(hipMalloc(&dI, idx.size() * 4), "malloc");
  check(hipMemcpy(dT, T.data(), nt * sizeof(Fp12), hipMemcpyHostToDevice), "h2d");
  check(hipMemcpy(dB, B.data(), nt * sizeof(Fp6), hipMemcpyHostToDevice), "h2d");
  check(hipMemcpy(dI, idx.data(), idx.size() * 4, hipMemcpyHostToDevice), "h2d");
  const dim3 g3((unsigned)((n + coop::kTriples - 1) / coop::kTriples)), g2((unsigned)((n + tp::kPairs - 1) / tp::kPairs));
  auto report = [&](const char *name, float ms, double work) {
    printf("{\"variant\": \"%s\", \"items\": %lld, \"products\": %d, \"table\": %lld, \"ms\": %.3f, \"Mop_per_s\": %.1f}\n",
           name, (long long)n, K, (long long)nt, ms, work / ms / 1e3);
    fflush(stdout);
  };
  report("B3_fp12", best_of(4, [&] { hipLaunchKernelGGL(chain_b3, g3, dim3(kWG), 0, 0, dT, dI, dO, n, K); }),
         (double)n * K);
  report("P2_beta", best_of(4, [&] { hipLaunchKernelGGL(chain_p2, g2, dim3(kWG), 0, 0, dB, dI, dO, n, K); }),
         (double)n * K);
  std::vector<Fp12> y(n), f(n);
  check(hipMemcpy(y.data(), dO, n * sizeof(Fp12), hipMemcpyDeviceToHost), "d2h");
  for (int64_t k : {1, 4, 7, 8}) {
    // the chain's numerators again each time: finish works in place
    check(hipMemcpy(dO, y.data(), n * sizeof(Fp12), hipMemcpyHostToDevice), "h2d");
    const int64_t lanes = (n + k - 1) / k;
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    hipEventRecord(e0);
    hipLaunchKernelGGL(finish_k, dim3((unsigned)((lanes + kWG - 1) / kWG)), dim3(kWG), 0, 0, dO, dTmp, n, k);
    hipEventRecord(e1);
    check(hipEventSynchronize(e1), "sync");
    float ms;
    hipEventElapsedTime(&ms, e0, e1);
    char name[32];
    snprintf(name, sizeof name, "FIN_chunk%lld", (long long)k);
    report(name, ms, (double)n);
  }
  check(hipMemcpy(f.data(), dO, n * sizeof(Fp12), hipMemcpyDeviceToHost), "d2h");
  // host check on a sample: the plain Fp12 product of the decompressed entries
  int64_t bad = 0;
  const int64_t step = n > 64 ? n / 64 : 1;
  for (int64_t i = 0; i < n; i += step) {
    Fp12 ref = Fp12::one(), yh = Fp12::one();
    for (int k = 0; k < K; k++) {
      const uint32_t e = idx[i * K + k];
      const Fp12 fe = torus::finish(Fp12{B[e >> 1], Fp6::one()});
      ref = mul(ref, (e & 1) ? conj(fe) : fe);
      torus::mul_beta(yh, B[e >> 1], e & 1);
    }
    bad += !(yh == y[i]) + !(ref == f[i]) + !(torus::finish(yh) == ref);
  }
  printf("{\"mismatches\": %lld}\n", (long long)bad);
  return bad ? 2 : 0;
}
