// Large-tile bf16 MFMA GEMM (256x128x64, 8 waves) with direct global->LDS DMA staging.
//
// Same math / layouts / epilogue contract as gemm.hip (A_K / B_K operand orientations, fused
// bias + activation + pre-activation store, beta accumulate, fp32 split-K partials), but built for
// the MI355X regime where the 128x128 register-staged kernel is L2-bandwidth bound
// (64 B/clk/CU of operand traffic at full MFMA rate vs ~47 here):
//   * tile 256(M) x 128(N) x 64(K), 512 threads = 8 waves as 4(M) x 2(N), 64x64 per wave
//     (4x4 mfma_f32_16x16x32_bf16 fragments, operands swapped so lanes own 4 output columns);
//     M = 8192-token BERT GEMMs with N = 1024 give exactly 256 tiles = one per CU;
//   * operands land in LDS by buffer_load ... lds (LDS-DMA, 16 B/lane, 1 KiB per wave
//     instruction): no staging VGPRs, hardware range check (num_records) zero-fills reads past
//     the end of the buffer so edge tiles never fault;
//   * conflict-free images written through the SOURCE address (rule 21: linear LDS destination,
//     inverse-swizzled global source, same XOR on the read): K-contiguous tiles as 128-B rows with
//     chunk ^ (row & 7) read by ds_read_b128; MN-contiguous tiles as 128-wide halves of 256-B
//     rows with the T10 image (b) XOR read by ds_read_b64_tr_b16;
//   * 3-stage LDS ring (3 x 48 KiB), counted `s_waitcnt vmcnt(6)` + raw s_barrier so the next
//     tile's DMA stays in flight across the barrier (cdna_hip_programming.md §5 "Pipelining
//     across barriers"; never __syncthreads in the loop, all LDS in one __shared__ array);
//   * XCD-aware bijective block remap + GROUP_M=8 ordering for L2 reuse; s_setprio around the
//     MFMA clusters (T5).
// Requires: 16-B aligned operand rows, K % 64 == 0 (a K tile never straddles rows), operands
// < 2 GiB. Anything else goes to gemm.hip.
// Both LDS images and their fragment read and the tile order are the ones of gemm_tile.h, the
// scattered epilogue is gemm_scatter_epilogue.h (all shared with gemm.hip and the 256-row
// kernels); this file is the DMA issue and the 3-stage loop around them.
#include "gemm_tile.h"

namespace ffk {
namespace big {
using namespace gtile;

constexpr int BM = 256, BN = 128, BK = 64, NT = 512;
constexpr int A_BYTES = BM * BK * 2;   // 32 KiB
constexpr int B_BYTES = BN * BK * 2;   // 16 KiB
constexpr int STAGE = A_BYTES + B_BYTES;
constexpr int NSTAGE = 3;

// Issue the LDS-DMA loads of one operand tile. ROWS = extent along M (or N).
// K-contiguous: image [ROWS][64] with 128-B rows, piece = 8 rows.
// MN-contiguous: image [ROWS/128][64][128] (256-B rows), piece = 4 rows of one half.
// Own copy: a loop over g256::dma_piece<KCONT, 64> is the same arithmetic but changes every
// instruction stream here, up to +26 instructions (docs/PERFORMANCE.md, "GEMM sources: one copy ...").
template <bool KCONT, int ROWS>
__device__ __forceinline__ void dma_tile(__amdgpu_buffer_rsrc_t rsrc, char* lds, int64_t ld, int mn0, int k0,
                                         int wave, int lane) {
  constexpr int PIECES = ROWS * BK * 2 / 1024;
  constexpr int PER_WAVE = PIECES / 8;
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int piece = wave * PER_WAVE + i;
    int64_t elem;
    if (KCONT) {
      const int row = piece * 8 + (lane >> 3);
      const int pc = lane & 7;
      const int c = pc ^ (row & 7);
      elem = (int64_t)(mn0 + row) * ld + k0 + c * 8;
    } else {
      const int half = piece / 16;          // 16 pieces (64 rows x 256 B) per 128-wide half
      const int row = (piece % 16) * 4 + (lane >> 4);
      const int pc = lane & 15;
      const int c = pc ^ swz_mn(row);
      elem = (int64_t)(k0 + row) * ld + mn0 + half * 128 + c * 8;
    }
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_ptr_t)(lds + piece * 1024), 16, (int)(elem * 2), 0, 0, 0);
  }
}

template <bool A_K, bool B_K, int OUT_MODE>
__global__ void __launch_bounds__(NT, 1) gemm_big_kernel(GemmArgs p, int64_t a_bytes, int64_t b_bytes) {
  __shared__ __attribute__((aligned(16))) char smem[NSTAGE * STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int tm = (p.M + BM - 1) / BM, tn = (p.N + BN - 1) / BN;
  int tile_m, tile_n;
  tile_coords(blockIdx.x, tm, tn, tile_m, tile_n);
  const int z = blockIdx.y;
  const int b = z / p.splitk, ks = z % p.splitk;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int kbeg = ks * p.kchunk;
  const int kend = min(p.K, kbeg + p.kchunk);
  const int nk = (kend - kbeg + BK - 1) / BK;

  const bf16_t* Ab = p.A + (int64_t)b * p.sA;
  const bf16_t* Bb = p.B + (int64_t)b * p.sB;
  // range-checked descriptors over the rest of each operand buffer (reads past it return 0)
  const int64_t a_rem = a_bytes - (int64_t)b * p.sA * 2;
  const int64_t b_rem = b_bytes - (int64_t)b * p.sB * 2;
  __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)Ab, (short)0, (int)min(a_rem, (int64_t)0x7fffffff), 0x00020000);
  __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)Bb, (short)0, (int)min(b_rem, (int64_t)0x7fffffff), 0x00020000);

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto issue = [&](int t) {
    char* st = smem + (t % NSTAGE) * STAGE;
    const int k0 = kbeg + t * BK;
    dma_tile<A_K, BM>(ra, st, p.lda, m0, k0, wave, lane);
    dma_tile<B_K, BN>(rb, st + A_BYTES, p.ldb, n0, k0, wave, lane);
  };
  if (nk > 0) issue(0);
  if (nk > 1) issue(1);
  for (int t = 0; t < nk; ++t) {
    if (t + 1 < nk) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (t + 2 < nk) issue(t + 2);
    const char* cur = smem + (t % NSTAGE) * STAGE;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) bfr[j] = frag<B_K, BK>(cur + A_BYTES, wn * 64 + j * 16, kk, lane);
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = frag<A_K, BK>(cur, wm * 64 + i * 16, kk, lane);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
  }

  const int mrow = m0 + wm * 64 + (lane & 15);
  const int ncol = n0 + wn * 64 + (lane >> 4) * 4;
  constexpr int NI = 4, NJ = 4;
#include "gemm_scatter_epilogue.h"
}

template <int MODE>
static void launch(const GemmArgs& p, dim3 grid, hipStream_t s, int64_t ab, int64_t bb) {
  gemm_with_layout(p.a_kcontig, p.b_kcontig, [&](auto ak, auto bk) {
    hipLaunchKernelGGL((gemm_big_kernel<decltype(ak)::value, decltype(bk)::value, MODE>), grid, dim3(NT), 0, s, p, ab, bb);
  });
}

}  // namespace big

// Returns false if the shape/alignment is not eligible (caller uses the 128x128 kernel).
bool gemm_big_bf16(const GemmArgs& p0, int64_t a_bytes, int64_t b_bytes, hipStream_t stream) {
  using namespace big;
  GemmArgs p = p0;
  if (p.K % BK != 0 || p.sA % 8 || p.sB % 8 || !gemm_dma_operands_ok(p, a_bytes, b_bytes)) return false;
  const int tm = (p.M + BM - 1) / BM, tn = (p.N + BN - 1) / BN;
  if ((int64_t)tm * tn * p.batch * p.splitk < 128) return false;  // too few tiles: 128x128 kernel fills better
  if (p.splitk > 1 && p.ws != nullptr) {
    p.kchunk = gemm_kchunk(p.K, p.splitk, BK);
    dim3 grid(tm * tn, p.batch * p.splitk);
    launch<2>(p, grid, stream, a_bytes, b_bytes);
    return true;  // caller runs the reduction
  }
  p.splitk = 1;
  p.kchunk = p.K;
  dim3 grid(tm * tn, p.batch);
  if (p.out_f32) launch<1>(p, grid, stream, a_bytes, b_bytes);
  else launch<0>(p, grid, stream, a_bytes, b_bytes);
  return true;
}

}  // namespace ffk
