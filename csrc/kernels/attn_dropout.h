#pragma once
// Attention dropout: the one definition of the keep-mask (mirrored in Python by
// flexflow_amd.kernels.attn_dropout_keep_ref, the oracle of the tests).
//
// Whether attention probability (b, h, q, k) of a layer is kept in a training step is a pure
// function of (seed, layer_id, step, b, h, q, k), b and h being GLOBAL batch / head indices: no tile
// shape, kernel variant, launch geometry or sharding enters, so every shard and every kernel draws
// the mask a 1-GPU run draws. Counter-based, no state:
//
//   rng_seed = mix64(seed * 0x9E3779B97F4A7C15 + layer_id)          host, once per layer
//   head_key = mix64(mix64(rng_seed + step * 0xD1B54A32D192ED03)    wave-uniform (scalar unit)
//                    + (b * H_total + h) * 0x9E3779B97F4A7C15)
//   row_key  = high 32 bits of mix64(head_key + q * 0x9E3779B97F4A7C15)   once per query row
//   word     = fmix32(row_key + (k >> 2) * 0x9E3779B1)              4 threshold bytes: keys 4j..4j+3
//   keep     = ((word >> 8 (k & 3)) & 255) >= thr,  thr = round(256 p)
//
// mix64 is the splitmix64 finaliser (init.hip, elementwise.hip), fmix32 the murmur3 one. The 8-bit
// threshold makes the effective rate p_eff = thr / 256; the 1 / (1 - p_eff) scale uses p_eff. The
// 64-bit multiplies are per row; an element costs at most the 32-bit fmix32 (the forward, whose
// lanes hold 4 consecutive keys of one row per register quad, pays it once per 4 elements; the
// backward, whose lanes hold one key and 4 consecutive queries, once per element).
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ffk {

__device__ __forceinline__ uint64_t adrop_mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ uint32_t adrop_fmix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  return x ^ (x >> 16);
}

constexpr uint32_t ADROP_KMUL = 0x9E3779B1u;

// bh = global batch index * H_total + global head index
__device__ __forceinline__ uint64_t attn_dropout_head_key(uint64_t rng_seed, int64_t step, int64_t bh) {
  const uint64_t s = adrop_mix64(rng_seed + (uint64_t)step * 0xD1B54A32D192ED03ull);
  return adrop_mix64(s + (uint64_t)bh * 0x9E3779B97F4A7C15ull);
}

__device__ __forceinline__ uint32_t attn_dropout_row_key(uint64_t head_key, int q) {
  return (uint32_t)(adrop_mix64(head_key + (uint64_t)(uint32_t)q * 0x9E3779B97F4A7C15ull) >> 32);
}

// the threshold bytes of keys 4 kq .. 4 kq + 3 of a row; kq_mul = kq * ADROP_KMUL
__device__ __forceinline__ uint32_t attn_dropout_word(uint32_t row_key, uint32_t kq_mul) {
  return adrop_fmix32(row_key + kq_mul);
}

__device__ __forceinline__ bool attn_dropout_keep(uint64_t rng_seed, int64_t step, int64_t bh, int q, int k,
                                                  uint32_t thr) {
  const uint32_t w = attn_dropout_word(attn_dropout_row_key(attn_dropout_head_key(rng_seed, step, bh), q),
                                       (uint32_t)(k >> 2) * ADROP_KMUL);
  return ((w >> (8 * (k & 3))) & 255u) >= thr;
}

}  // namespace ffk
