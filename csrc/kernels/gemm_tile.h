// What the tiled bf16 MFMA GEMMs share on the device (gemm.hip 128x128, gemm_big.hip 256x128,
// gemm256_tile.h / gemm256.hip 256-row, gemm_pp.hip persistent ping-pong): the LDS image swizzles,
// the 16x32 fragment read and the tile order. One copy: a fix to a swizzle is made here once. (The
// scattered epilogue they share is gemm_scatter_epilogue.h.) Each kernel compiles to the instruction
// stream it had with its own copies (profiles/gemm_dedup_isa.txt).
#pragma once
#include <type_traits>
#include "common.h"
#include "gemm.h"

namespace ffk {
namespace gtile {

typedef __attribute__((address_space(3))) void* lds_ptr_t;

// 16-B chunk swizzle of a K-contiguous row of BK bf16 (64-B rows: 4 chunks, 128-B rows: 8 chunks)
template <int BK>
__device__ __forceinline__ int swz_k(int row) {
  if constexpr (BK == 32) return ((row >> 2) & 1) << 1;
  else return row & 7;
}
// 16-B chunk swizzle of a 256-B MN-contiguous k-row (T10 image (b))
__device__ __forceinline__ int swz_mn(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }

// 16 (rows along M or N) x 32 (k, sub-step kk of the K-tile) fragment for mfma_f32_16x16x32_bf16:
// lane holds row r0 + (l & 15), k = 32 kk + 8 (l >> 4) + j, j = 0..7. K-contiguous image: 2 BK-byte
// rows, one ds_read_b128. MN-contiguous image: 128-wide halves of 256-B k-rows (half r0 >> 7; a
// 128-wide tile only has half 0), two ds_read_b64_tr_b16 so the hardware does the transpose.
template <bool KCONT, int BK, bool HALVES = true>
__device__ __forceinline__ bf16x8 frag(const char* tile, int r0, int kk, int lane) {
  if (KCONT) {
    const int row = r0 + (lane & 15);
    const int c = kk * 4 + (lane >> 4);
    return *reinterpret_cast<const bf16x8*>(tile + row * (BK * 2) + ((c ^ swz_k<BK>(row)) << 4));
  } else {
    const char* hl = HALVES ? tile + (r0 >> 7) * (BK * 256) : tile;
    const int rr = HALVES ? r0 & 127 : r0;
    const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
    const int chunk = (rr >> 3) + (p >> 1);
    bf16x8 out;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const int krow = 32 * kk + 8 * g + 4 * hf + q;
      const int off = krow * 256 + ((chunk ^ swz_mn(krow)) << 4) + 8 * (p & 1);
      typedef short v4s __attribute__((ext_vector_type(4)));
      v4s v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(hl + off));
      bf16x4 b = __builtin_bit_cast(bf16x4, v);
      out[4 * hf + 0] = b[0];
      out[4 * hf + 1] = b[1];
      out[4 * hf + 2] = b[2];
      out[4 * hf + 3] = b[3];
    }
    return out;
  }
}

// Block id -> output tile: XCD-aware bijective remap (T1), then groups of GROUP_M = 8 row tiles
// walked column by column for L2 reuse.
__device__ __forceinline__ void tile_coords(int bid, int tm, int tn, int& tile_m, int& tile_n) {
  const int nwg = tm * tn;
  bid = xcd_remap(bid, nwg);
  constexpr int GM = 8;
  const int per_group = GM * tn;
  const int group = bid / per_group;
  const int first_m = group * GM;
  const int gsize = min(tm - first_m, GM);
  const int in_g = bid % per_group;
  tile_m = first_m + in_g % gsize;
  tile_n = in_g / gsize;
}

}  // namespace gtile
}  // namespace ffk
