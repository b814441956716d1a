#pragma once
// Device helpers shared by the flash attention kernels (attention.hip) and the score-bias gradient
// kernel (attn_dbias.hip): the swizzled [rows][D] bf16 LDS tile image, its register and LDS-DMA
// stagers, the bare exp2 and the per-sample key limit.
#include "common.h"
#include "attention.h"

namespace ffk {

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

template <int D>
__device__ __forceinline__ int aswz(int row) {
  if (D == 64) return (((row >> 1) & 1) << 2) | ((row >> 3) & 1) | (((row >> 4) & 1) << 1);
  else return ((row & 3) << 2) | ((row >> 2) & 3);
}
// byte offset of element (row, col) of a [rows][D] bf16 tile image
template <int D>
__device__ __forceinline__ int aoff(int row, int col) {
  const int ch = col >> 3;
  return row * (D * 2) + ((ch ^ aswz<D>(row)) << 4) + ((col & 7) << 1);
}

// 2^x as the bare v_exp_f32. exp2f() lowers to v_exp_f32 wrapped in a denormal range fix-up
// (v_cmp + 2 v_cndmask + v_add + v_ldexp: six VALU ops per score element instead of one); softmax
// probabilities below 2^-126 are irrelevant (they flush to 0, exp2(-inf) stays 0).
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

typedef short v4s __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16x4 tr_read(const char* lds, int off) {
  v4s v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(lds + off));
  return __builtin_bit_cast(bf16x4, v);
}

// Stage a [ROWS][D] bf16 tile (rows r0.., clamp at rlim) from global (row stride ss) into regs.
template <int D, int ROWS, int NTH>
struct TileStage {
  static constexpr int CH = ROWS * D / 8 / NTH;  // 16-B chunks per thread
  uint4 r[CH];
  __device__ __forceinline__ void load(const bf16_t* g, int64_t ss, int r0, int rlim, int tid) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int id = tid + i * NTH;
      const int row = id / (D / 8), c = id % (D / 8);
      if (r0 + row < rlim) r[i] = *reinterpret_cast<const uint4*>(g + (int64_t)(r0 + row) * ss + c * 8);
      else r[i] = make_uint4(0, 0, 0, 0);
    }
  }
  __device__ __forceinline__ void store(char* lds, int tid) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int id = tid + i * NTH;
      const int row = id / (D / 8), c = id % (D / 8);
      *reinterpret_cast<uint4*>(lds + aoff<D>(row, c * 8)) = r[i];
    }
  }
  template <class F>
  __device__ __forceinline__ void store(char* lds, int tid, F off) {  // image given by off(row, col)
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int id = tid + i * NTH;
      const int row = id / (D / 8), c = id % (D / 8);
      *reinterpret_cast<uint4*>(lds + off(row, c * 8)) = r[i];
    }
  }
};

typedef __attribute__((address_space(3))) void* lds_ptr_t;

// Same [64][D] tile image as TileStage::store, written by the LDS-DMA path (buffer_load ... lds):
// no staging registers, so the forward needs 32 fewer VGPRs (4 workgroups per CU instead of 3 at
// D = 64). Each wave instruction fills one 1-KiB piece, lane l landing at piece + 16 l; the XOR
// swizzle is applied on the global side (lane l of slot s fetches chunk (s % CPR) ^ aswz(row)).
// Rows past the sequence end read as zero (buffer range check), like TileStage's clamp.
template <int D, int NWAVES>
__device__ __forceinline__ void dma_tile(__amdgpu_buffer_rsrc_t rs, char* lds_tile, int64_t ss, int r0, int wave,
                                         int lane) {
  constexpr int PIECES = 64 * D * 2 / 1024, CPR = D / 8;
#pragma unroll
  for (int i = 0; i < PIECES / NWAVES; ++i) {
    const int piece = i * NWAVES + wave;
    const int slot = piece * 64 + lane;
    const int row = slot / CPR;
    const int ch = (slot % CPR) ^ aswz<D>(row);
    const int off = (int)(((int64_t)(r0 + row) * ss + ch * 8) * 2);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)(lds_tile + piece * 1024), 16, off, 0, 0, 0);
  }
}

// Keys of sample b that take part: clamp(key_lens[b], 0, Sk), or Sk without lengths. One scalar
// load per workgroup (b is wave-uniform); only the MASK = true instantiations look at it.
template <bool MASK>
__device__ __forceinline__ int key_limit(const AttnArgs& a, int b) {
  if constexpr (MASK) {
    if (a.key_lens) return __builtin_amdgcn_readfirstlane(min(max(a.key_lens[b], 0), a.Sk));
  }
  return a.Sk;
}

}  // namespace ffk
