// ray_perm.hpp — the epoch permutation of the ray loaders: a stateless bijection of [0, N) keyed by (seed, epoch).
// Position p of epoch e is a pure function of (N, seed, e, p): no N-sized table, no host RNG, any thread of any rank
// computes it.  One definition for the device (k_ray_batch, raydata.hip) and the host (fsn_ray_perm_host); the tests
// restate it in NumPy (tests/raydata_ref.py).
//
// Construction: a balanced 4-round Feistel network over 2k bits, 2k the smallest even width >= 2 with 2^(2k) >= N
// (so the domain D = 2^(2k) is below 4N for N >= 2), round function = k bits of a splitmix64 finaliser of
// (half ^ round key), and cycle walking: apply the network again while the value is >= N.
//   * a Feistel network is a bijection of [0, D) whatever its round function is;
//   * cycle walking ends: x -> E(x) moves along the cycle of the permutation E that contains the start p < N; the
//     cycle is finite and returns to p itself, so a value < N is met after at most D - N + 1 applications (in
//     expectation D / N < 4).  The map p -> first value < N on p's cycle is then a bijection of [0, N) (the
//     permutation E restricted to the subset by skipping the elements outside it).
// N up to 2^62 (k <= 31).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#define FSN_HD __host__ __device__ __forceinline__

namespace fsn {

constexpr int kRayPermRounds = 4;

struct RayPerm {
  uint64_t n;                    // size of the index set
  uint64_t key[kRayPermRounds];  // round keys
  uint32_t half_bits;            // k
  uint32_t half_mask;            // 2^k - 1
};

// splitmix64's output function (Steele, Lea, Flood 2014) on z + golden gamma
FSN_HD uint64_t ray_perm_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

FSN_HD RayPerm ray_perm_make(uint64_t n, uint64_t seed, uint64_t epoch) {
  RayPerm p;
  p.n = n;
  uint32_t k = 1;
  while (k < 31 && (1ull << (2 * k)) < n) ++k;
  p.half_bits = k;
  p.half_mask = (uint32_t)((1ull << k) - 1ull);
  const uint64_t base = ray_perm_mix(seed ^ ray_perm_mix(epoch));
  for (int r = 0; r < kRayPermRounds; ++r) p.key[r] = ray_perm_mix(base + (uint64_t)r);
  return p;
}

// one application of the network to x in [0, 2^(2k))
FSN_HD uint64_t ray_perm_feistel(const RayPerm& p, uint64_t x) {
  uint32_t l = (uint32_t)(x >> p.half_bits) & p.half_mask, r = (uint32_t)x & p.half_mask;
#pragma unroll
  for (int i = 0; i < kRayPermRounds; ++i) {
    const uint32_t f = (uint32_t)(ray_perm_mix((uint64_t)r ^ p.key[i]) >> 32) & p.half_mask;
    const uint32_t t = l ^ f;
    l = r;
    r = t;
  }
  return ((uint64_t)l << p.half_bits) | (uint64_t)r;
}

// element `pos` (< n) of the permutation.  The loop ends after at most D - N + 1 turns (see above).
FSN_HD uint64_t ray_perm_at(const RayPerm& p, uint64_t pos) {
  uint64_t x = pos;
  do {
    x = ray_perm_feistel(p, x);
  } while (x >= p.n);
  return x;
}

}  // namespace fsn
