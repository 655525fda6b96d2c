// The dropout mask of v0.19.0 (dropout.hip: the six attended features; fusion.hip: the epilogue of m): a stateless counter RNG,
// Philox-4x32-10.  Element i belongs to block i >> 2, word i & 3, and the block is a pure function of (block, step, seed):
// nothing of a mask is stored, a backward regenerates the forward's from the same three numbers.  Element i is kept when its
// word is >= thr = floor(p 2^32), and then scaled by 1 / (1 - p).  tests/_dropout.keep is the definition both users are held to.
#pragma once
#include "common.h"

namespace {

constexpr unsigned kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u, kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
struct u32x4 { unsigned x, y, z, w; };

__device__ __forceinline__ u32x4 philox4x32_10(u32x4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(kM0, c.x), lo0 = kM0 * c.x;
    const unsigned hi1 = __umulhi(kM1, c.z), lo1 = kM1 * c.z;
    c = u32x4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += kW0;
    k1 += kW1;
  }
  return c;
}

// a mask's three numbers but the block: the seed, the step, and what p makes of a word
struct Drop { unsigned k0, k1, s0, s1, thr; float scale; };
// the state words are seed lo, hi, step lo, hi; `next`: step + 1, the mask a training forward draws and then stores
__device__ __forceinline__ unsigned long long drop_step(const unsigned* state, int next) {
  return ((unsigned long long)state[2] | ((unsigned long long)state[3] << 32)) + (unsigned long long)(next != 0);
}
__device__ __forceinline__ Drop drop_load(const unsigned* state, unsigned thr, float scale, int next) {
  const unsigned long long step = drop_step(state, next);
  return Drop{state[0], state[1], (unsigned)step, (unsigned)(step >> 32), thr, scale};
}
__device__ __forceinline__ u32x4 drop_block(const Drop& d, unsigned long long j) {
  return philox4x32_10(u32x4{(unsigned)j, (unsigned)(j >> 32), d.s0, d.s1}, d.k0, d.k1);
}
__device__ __forceinline__ float drop_word(const Drop& d, unsigned r) { return r >= d.thr ? d.scale : 0.0f; }
// the factor of element i alone
__device__ __forceinline__ float drop_factor(const Drop& d, unsigned i) {
  const u32x4 c = drop_block(d, i >> 2);
  const unsigned w = i & 3u;
  return drop_word(d, w == 0u ? c.x : (w == 1u ? c.y : (w == 2u ? c.z : c.w)));
}

struct DropHost { unsigned thr; float scale; };
inline DropHost drop_host(float p) {                          // (floor: the product is exact and below 2^32)
  return DropHost{(unsigned)(unsigned long long)((double)p * 4294967296.0), (float)(1.0 / (1.0 - (double)p))};
}

}  // namespace
