// Host check of the 9 x 29-bit-limb Montgomery core (csrc/bn254/field.h,
// tower.h) for a sanitizer build: the fixed edge vectors of
// tests/test_field29.py, every pairing, through fmul / fsqr / fmul2 for Fp and
// Fr and through the Fp2 product, against a schoolbook Montgomery product on
// 4 x 64-bit words with unsigned __int128.  Host code only; needs no GPU.
//
// Build: hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=undefined,address \
//          -Xarch_host -fno-sanitize-recover=undefined -I csrc tools/field29_check.hip -o tools/bin/field29_check
// Run:   tools/bin/field29_check
#include "bn254/tower.h"

#include <cstdio>
#include <vector>

using namespace dx;
typedef unsigned __int128 u128;

namespace {
struct U256 {
  uint64_t w[4];
};

template <class PR>
U256 modulus() {
  U256 r;
  for (int i = 0; i < 4; i++) r.w[i] = (uint64_t)PR::MOD[2 * i] | ((uint64_t)PR::MOD[2 * i + 1] << 32);
  return r;
}
template <class PR>
U256 from_field(const FieldT<PR> &a) {
  U256 r;
  for (int i = 0; i < 4; i++) r.w[i] = (uint64_t)a.v[2 * i] | ((uint64_t)a.v[2 * i + 1] << 32);
  return r;
}
template <class PR>
FieldT<PR> to_field(const U256 &a) {
  FieldT<PR> r;
  for (int i = 0; i < 4; i++) {
    r.v[2 * i] = (uint32_t)a.w[i];
    r.v[2 * i + 1] = (uint32_t)(a.w[i] >> 32);
  }
  return r;
}
bool geq(const U256 &a, const U256 &b) {
  for (int i = 3; i >= 0; i--) {
    if (a.w[i] != b.w[i]) return a.w[i] > b.w[i];
  }
  return true;
}
U256 add(const U256 &a, const U256 &b, uint64_t &carry) {
  U256 r;
  u128 c = 0;
  for (int i = 0; i < 4; i++) {
    c += (u128)a.w[i] + b.w[i];
    r.w[i] = (uint64_t)c;
    c >>= 64;
  }
  carry = (uint64_t)c;
  return r;
}
U256 sub(const U256 &a, const U256 &b) {
  U256 r;
  uint64_t br = 0;
  for (int i = 0; i < 4; i++) {
    const u128 d = (u128)a.w[i] - b.w[i] - br;
    r.w[i] = (uint64_t)d;
    br = (uint64_t)(d >> 64) & 1;
  }
  return r;
}
U256 pow2(int k) {
  U256 r = {{0, 0, 0, 0}};
  r.w[k / 64] = 1ull << (k % 64);
  return r;
}
U256 small(uint64_t x) { return {{x, 0, 0, 0}}; }

// (sum of the 512-bit schoolbook products a_i b_i) * 2^-256 mod p, word-serial REDC
U256 ref_mont(const U256 &p, const std::vector<std::pair<U256, U256>> &prods) {
  uint64_t t[10] = {0};
  for (const auto &ab : prods) {
    for (int i = 0; i < 4; i++) {
      u128 c = 0;
      for (int j = 0; j < 4; j++) {
        c += (u128)ab.first.w[i] * ab.second.w[j] + t[i + j];
        t[i + j] = (uint64_t)c;
        c >>= 64;
      }
      for (int k = i + 4; c != 0 && k < 10; k++) {
        c += t[k];
        t[k] = (uint64_t)c;
        c >>= 64;
      }
    }
  }
  uint64_t ninv = 1;  // -p^-1 mod 2^64 by Newton
  for (int i = 0; i < 6; i++) ninv *= 2 - p.w[0] * ninv;
  ninv = 0 - ninv;
  for (int i = 0; i < 4; i++) {
    const uint64_t m = t[i] * ninv;
    u128 c = 0;
    for (int j = 0; j < 4; j++) {
      c += (u128)m * p.w[j] + t[i + j];
      t[i + j] = (uint64_t)c;
      c >>= 64;
    }
    for (int k = i + 4; c != 0 && k < 10; k++) {
      c += t[k];
      t[k] = (uint64_t)c;
      c >>= 64;
    }
  }
  U256 r = {{t[4], t[5], t[6], t[7]}};
  uint64_t hi = t[8];
  while (hi != 0 || geq(r, p)) {  // below 3 p: at most two rounds
    const bool borrow = !geq(r, p);
    r = sub(r, p);
    if (borrow) hi--;
  }
  return r;
}

template <class PR>
std::vector<U256> operands() {
  const U256 p = modulus<PR>();
  uint64_t cy;
  std::vector<U256> v = {small(0), small(1), sub(p, small(1)), sub(p, small(2)), from_field(FieldT<PR>::one()),
                         from_field(FieldT<PR>::from_limbs(PR::R2))};
  for (int k = 1; k <= 8; k++) {
    v.push_back(sub(pow2(29 * k), small(1)));
    v.push_back(pow2(29 * k));
    v.push_back(add(pow2(29 * k), small(1), cy));
  }
  for (int k = 1; k <= 7; k++) {
    v.push_back(sub(pow2(32 * k), small(1)));
    v.push_back(add(pow2(32 * k), small(1), cy));
  }
  for (int k = 1; k <= 8; k++) v.push_back(sub(p, pow2(29 * k)));
  return v;
}

template <class PR>
bool same(const FieldT<PR> &got, const U256 &want) {
  return got == to_field<PR>(want);
}

template <class PR>
long check_field(const char *name) {
  const U256 p = modulus<PR>();
  const std::vector<U256> v = operands<PR>();
  long bad = 0, n = 0;
  for (const U256 &x : v) {
    for (const U256 &y : v) {
      const FieldT<PR> a = to_field<PR>(x), b = to_field<PR>(y);
      bad += !same(fmul(a, b), ref_mont(p, {{x, y}}));
      bad += !same(fsqr(a), ref_mont(p, {{x, x}}));
      // fmul2 with the mirrored pair and with the operand MOD - y (in (0, MOD])
      bad += !same(fmul2(a, b, b, a), ref_mont(p, {{x, y}, {y, x}}));
      bad += !same(fmul2(a, a, b, mod_minus(b)), ref_mont(p, {{x, x}, {y, sub(p, y)}}));
      n += 4;
    }
  }
  printf("%s: %ld results, %ld wrong\n", name, n, bad);
  return bad;
}

long check_fp2() {
  const U256 p = modulus<FpParams>();
  const std::vector<U256> v = operands<FpParams>();
  const size_t nv = v.size();
  long bad = 0, n = 0;
  for (size_t i = 0; i < nv; i++) {
    for (size_t j = 0; j < nv; j++) {
      const U256 &a0 = v[i], &a1 = v[(i + 1) % nv], &b0 = v[j], &b1 = v[(j + 1) % nv];
      const Fp2 a = {to_field<FpParams>(a0), to_field<FpParams>(a1)}, b = {to_field<FpParams>(b0), to_field<FpParams>(b1)};
      const Fp2 c = mul(a, b);
      bad += !same(c.c0, ref_mont(p, {{a0, b0}, {a1, sub(p, b1)}}));
      bad += !same(c.c1, ref_mont(p, {{a0, b1}, {a1, b0}}));
      const Fp2 s = sqr(a);
      bad += !same(s.c0, ref_mont(p, {{a0, a0}, {a1, sub(p, a1)}}));
      bad += !same(s.c1, ref_mont(p, {{a0, a1}, {a1, a0}}));
      const Fp2 f = mul_fp(a, b.c0);
      bad += !same(f.c0, ref_mont(p, {{a0, b0}}));
      bad += !same(f.c1, ref_mont(p, {{a1, b0}}));
      n += 6;
    }
  }
  printf("Fp2: %ld results, %ld wrong\n", n, bad);
  return bad;
}
}  // namespace

int main() {
  const long bad = check_field<FpParams>("Fp") + check_field<FrParams>("Fr") + check_fp2();
  printf(bad ? "FAILED\n" : "field29_check: all results match\n");
  return bad ? 1 : 0;
}
