// Grouped bf16 MFMA GEMMs for the Linears of a mixture of experts: all n experts of a layer in ONE
// launch per direction, each expert computing only the rows the router gave it.
//
// Expert e owns X_e [cap][K] (group_by's output: n separate tensors, reached through a pointer table
// passed by value, nothing is copied into a slab), W_e [N][K] of the stacked weight [n][N][K], and
// r_e = min(max(load[e], 0), cap) live rows, read from the router's device-side load[] (no host
// synchronisation: the grid depends on (n, cap, N, K) only, so a step captures into a hipGraph).
//
//   forward        Y_e[r, :]  = act(X_e[r, :] . W_e^T + b_e)        r < r_e     (bf16, optional Z = pre-act)
//   input gradient dX_e[r, :] = dZ_e[r, :] . W_e                    r < r_e     (bf16)
//   weight gradient dW_e     += sum_{r < r_e} dZ_e[r, :]^T X_e[r, :]            (fp32, beta = 1)
//                   db_e     += sum_{r < r_e} dZ_e[r, :]
//   act backward   dZ_e[r, :] = dY_e[r, :] * act'(Z_e[r, :])        r < r_e     (elementwise, one launch)
//
// Rows >= r_e of Y / Z / dX are written as exact zeros; rows >= r_e of X_e / dY_e / dZ_e are never
// loaded (a masked chunk is SELECTED to zero in the staging registers, it is not multiplied by
// zero), so NaN in the padding cannot reach any result.
//
// Design. One workgroup = 4 waves (2 x 2) = one output tile of one expert, blockIdx.y = e.
//   * forward / input gradient (experts_rows_kernel): BM x 128 x 64 tiles, BM = 128 (each wave 64 x 64,
//     4 x 4 mfma_f32_16x16x32_bf16 fragments) or BM = 64 (each wave 32 x 64). A tile wholly at or beyond
//     r_e loads nothing, issues no MFMA and stores zeros; the block ids of an expert are dealt to its
//     live tiles first, so these spread over all XCDs at any load. The 64-row variant is chosen for cap <= 512:
//     the rows a partial last tile wastes are BM / 2 per expert on average, which at such capacities is
//     more than a tenth of the live rows, while the W tile (re-read once per M-tile) is small against
//     them; above that the 128-row tile halves the W traffic per output row. The input gradient reads
//     W_e N-major through the transposed LDS image (frag<false>, ds_read_b64_tr_b16).
//   * weight gradient (experts_wgrad_kernel): one workgroup owns one 128 x 128 tile of dW_e and walks the
//     whole reduction of ceil(r_e / 64) steps: no split-K, no atomics, no finishing pass, the same bits
//     on every run. Both operands are read row-major over the reduction (MN-contiguous images). The
//     workgroups of K-tile 0 also sum db from the dZ chunks they stage (fp32 per thread, then a fixed-
//     order fold of the 16 row groups through LDS). r_e = 0 leaves dW_e / db_e untouched.
//   * staging: global_load_dwordx4 into registers for tile t + 1 issued before the MFMAs of tile t,
//     ds_write after them, double-buffered LDS, one barrier per K-tile; LDS images, fragment reads and
//     tile order are gemm_tile.h's (shared with gemm.hip), the masked staging is this kernel's own.
//   * gated experts (experts_glu_rows_kernel, experts_glu_bwd_kernel): W_e [2F][K] holds F gate rows, then F
//     up rows. H_e = act(X_e Wg_e^T + bg_e) * (X_e Wu_e^T + bu_e) from one BM x 64 tile per workgroup whose
//     B stage is the 64 gate rows and the 64 up rows of its output columns: both fp32 sums of an element
//     sit in the same lane and the product is the epilogue (optional Z = (zg | zu) [cap][2F] for the
//     backward), written through LDS as whole 16-B row chunks. The gate backward is one elementwise launch
//     over the live rows into dZ [cap][2F], which the two gradient kernels above take with N = 2F.
// Launchers refuse (return false) K % 8, N % 8, more than kMoeMaxExperts experts or a base that is not
// 16-B aligned; the caller then runs its per-expert fallback.
#include "gemm_tile.h"
#include "glu_act.h"
#include "ops.h"

namespace ffk {
using namespace gtile;

namespace {

constexpr int BN = 128, BK = 64, NT = 256;

struct ExpertPtrs {
  const bf16_t* p[kMoeMaxExperts];
};

__device__ __forceinline__ int live_rows(const int* __restrict__ load, int e, int cap) {
  return min(max(load[e], 0), cap);
}

// Register staging of one operand tile: ROWS x 64 K-contiguous (ROWS = 64 or 128) or 64 x 128
// MN-contiguous. Chunks (8 bf16, 16 B) outside [mn_lim) x [k_lim) are selected to zero, not loaded:
// k_lim / mn_lim carry the expert's live row count where rows are the masked extent.
template <bool KCONT, int ROWS>
struct Stage {
  static constexpr int NL = KCONT ? ROWS / 32 : 4;
  uint4 r[NL];
  __device__ __forceinline__ void load(const bf16_t* __restrict__ g, int64_t ld, int mn0, int k0, int mn_lim,
                                       int k_lim, int tid) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int id = tid + i * NT;
      int mn, kk;
      if (KCONT) { mn = id >> 3; kk = (id & 7) * 8; }
      else { kk = id >> 4; mn = (id & 15) * 8; }
      const int gm = mn0 + mn, gk = k0 + kk;
      if (gm < mn_lim && gk < k_lim) {
        const bf16_t* q = KCONT ? g + (int64_t)gm * ld + gk : g + (int64_t)gk * ld + gm;
        r[i] = *reinterpret_cast<const uint4*>(q);
      } else {
        r[i] = make_uint4(0, 0, 0, 0);
      }
    }
  }
  // The B stage of the gated forward (K-contiguous, 128 rows): rows 0..63 are the gate rows n0 .. n0 + 63
  // of W_e [2F][K], rows 64..127 its up rows F + n0 .. F + n0 + 63; a row whose column n0 + (row & 63) is at
  // or beyond F is selected to zero, so an up tile never reads into the next expert and a gate tile never
  // reads up rows.
  __device__ __forceinline__ void load_glu(const bf16_t* __restrict__ g, int64_t ld, int n0, int k0, int F, int k_lim,
                                           int tid) {
    static_assert(KCONT && ROWS == 128, "the gated stage is the K-contiguous 128-row one");
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int id = tid + i * NT;
      const int row = id >> 3, gn = n0 + (row & 63), gk = k0 + (id & 7) * 8;
      if (gn < F && gk < k_lim) {
        r[i] = *reinterpret_cast<const uint4*>(g + (int64_t)((row >> 6) * F + gn) * ld + gk);
      } else {
        r[i] = make_uint4(0, 0, 0, 0);
      }
    }
  }
  __device__ __forceinline__ void store(char* lds, int tid) const {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int id = tid + i * NT;
      int off;
      if (KCONT) {
        const int row = id >> 3, c = id & 7;
        off = row * 128 + ((c ^ swz_k<BK>(row)) << 4);
      } else {
        const int row = id >> 4, c = id & 15;
        off = row * 256 + ((c ^ swz_mn(row)) << 4);
      }
      *reinterpret_cast<uint4*>(lds + off) = r[i];
    }
  }
  // MN-contiguous only: every chunk of a thread covers the same 8 columns ((tid & 15) * 8 ..), so
  // their fp32 sums over the staged k-rows accumulate in 8 registers
  __device__ __forceinline__ void add_cols(float* s) const {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const uint32_t w[4] = {r[i].x, r[i].y, r[i].z, r[i].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s[2 * j] += __uint_as_float(w[j] << 16);
        s[2 * j + 1] += __uint_as_float(w[j] & 0xffff0000u);
      }
    }
  }
};

// Block id -> tile of expert e with `rows` live rows: the first tm_live * tn block ids take the live
// tiles, in gemm_tile.h's order over the live rows only; the others take the empty tiles behind them.
// Consecutive block ids go to consecutive XCDs, so the live tiles spread over all of them whatever
// share of the capacity is filled (the tile order over all cap rows put them on the first XCDs only:
// 2x the time at half load).
template <int BM>
__device__ __forceinline__ void deal_tile(int bid, int rows, int tn, int& tile_m, int& tile_n) {
  const int tm_live = (rows + BM - 1) / BM, n_live = tm_live * tn;
  if (bid < n_live) {
    tile_coords(bid, tm_live, tn, tile_m, tile_n);
  } else {
    tile_m = tm_live + (bid - n_live) / tn;
    tile_n = (bid - n_live) % tn;
  }
}

// The K loop of the gated forward, experts_rows_kernel's with the gated B stage: acc += X_e[m0 .. m0 + BM)[K]
// . (gate rows | up rows)^T over double-buffered LDS stages (A: BM x 64, rows at or beyond `rows` selected
// to zero; B: 128 x 64), the loads of tile t + 1 issued before the MFMAs of tile t and written to LDS
// after them, one barrier per K-tile. Wave (wm, wn) takes A rows wm * BM/2 + 16 i and, for accumulator
// slot j, B rows wn * 32 + 16 j (gate, j < 2) or 64 + wn * 32 + 16 (j - 2) (up): slots j and j + 2 of a lane
// hold the gate and the up value of the same output element. On return every wave has passed the last
// barrier: the LDS is free. (Kept apart from experts_rows_kernel's loop: one template for both changed
// that kernel's scalar registers and argument loads.)
template <int BM>
__device__ __forceinline__ void glu_mainloop(char* smem, const bf16_t* __restrict__ A, const bf16_t* __restrict__ W,
                                             int K, int F, int m0, int n0, int rows, int tid, int lane, int wm, int wn,
                                             f32x4 (&acc)[BM / 32][4]) {
  constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2, STAGE_BYTES = A_BYTES + B_BYTES;
  constexpr int MI = BM / 32;
  const int nk = (K + BK - 1) / BK;
  Stage<true, BM> sa;
  Stage<true, BN> sb;
  sa.load(A, K, m0, 0, rows, K, tid);
  sb.load_glu(W, K, n0, 0, F, K, tid);
  sa.store(smem, tid);
  sb.store(smem + A_BYTES, tid);
  __syncthreads();
  for (int t = 0; t < nk; ++t) {
    char* cur = smem + (t & 1) * STAGE_BYTES;
    char* nxt = smem + ((t + 1) & 1) * STAGE_BYTES;
    const bool more = (t + 1) < nk;
    if (more) {
      sa.load(A, K, m0, (t + 1) * BK, rows, K, tid);
      sb.load_glu(W, K, n0, (t + 1) * BK, F, K, tid);
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[MI], bfr[4];
#pragma unroll
      for (int i = 0; i < MI; ++i) af[i] = frag<true, BK, false>(cur, wm * (BM / 2) + i * 16, kk, lane);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        bfr[j] = frag<true, BK, false>(cur + A_BYTES, (j >> 1) * 64 + wn * 32 + (j & 1) * 16, kk, lane);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    if (more) {
      sa.store(nxt, tid);
      sb.store(nxt + A_BYTES, tid);
    }
    __syncthreads();
  }
}

struct RowsArgs {
  ExpertPtrs a;       // X_e (forward) or dZ_e (input gradient): [cap][KR]
  const bf16_t* w;    // [n][N][K]; read [NO][KR] K-contiguous (forward) or [KR][NO] (input gradient)
  const void* bias;   // forward only: [n][NO], bf16 or fp32
  bf16_t* y;          // [n][cap][NO]
  bf16_t* z;          // optional pre-activation, same layout
  const int* load;
  int64_t w_stride;   // N * K
  int cap, NO, KR, ldw, act, bias_bf16;
};

template <int BM, bool B_K>
__global__ void __launch_bounds__(NT, 2) experts_rows_kernel(RowsArgs p) {
  constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2, STAGE_BYTES = A_BYTES + B_BYTES;
  constexpr int MI = BM / 32;
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int e = blockIdx.y;
  const int tn = (p.NO + BN - 1) / BN;
  const bf16_t* A = p.a.p[e];
  const int rows = A ? live_rows(p.load, e, p.cap) : 0;
  int tile_m, tile_n;
  deal_tile<BM>(blockIdx.x, rows, tn, tile_m, tile_n);
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  bf16_t* Y = p.y + (int64_t)e * p.cap * p.NO;
  bf16_t* Z = p.z ? p.z + (int64_t)e * p.cap * p.NO : nullptr;

  if (m0 >= rows) {  // nothing routed here: no operand load, no MFMA, the tile is zeros
    for (int id = tid; id < BM * (BN / 8); id += NT) {
      const int m = m0 + (id >> 4), n = n0 + (id & 15) * 8;
      if (m < p.cap && n < p.NO) {
        const int64_t o = (int64_t)m * p.NO + n;
        *reinterpret_cast<uint4*>(Y + o) = make_uint4(0, 0, 0, 0);
        if (Z) *reinterpret_cast<uint4*>(Z + o) = make_uint4(0, 0, 0, 0);
      }
    }
    return;
  }

  const bf16_t* W = p.w + (int64_t)e * p.w_stride;
  const int nk = (p.KR + BK - 1) / BK;
  Stage<true, BM> sa;
  Stage<B_K, BN> sb;
  f32x4 acc[MI][4];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  sa.load(A, p.KR, m0, 0, rows, p.KR, tid);
  sb.load(W, p.ldw, n0, 0, p.NO, p.KR, tid);
  sa.store(smem, tid);
  sb.store(smem + A_BYTES, tid);
  __syncthreads();
  for (int t = 0; t < nk; ++t) {
    char* cur = smem + (t & 1) * STAGE_BYTES;
    char* nxt = smem + ((t + 1) & 1) * STAGE_BYTES;
    const bool more = (t + 1) < nk;
    if (more) {
      sa.load(A, p.KR, m0, (t + 1) * BK, rows, p.KR, tid);
      sb.load(W, p.ldw, n0, (t + 1) * BK, p.NO, p.KR, tid);
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[MI], bfr[4];
#pragma unroll
      for (int i = 0; i < MI; ++i) af[i] = frag<true, BK, false>(cur, wm * (BM / 2) + i * 16, kk, lane);
#pragma unroll
      for (int j = 0; j < 4; ++j) bfr[j] = frag<B_K, BK, false>(cur + A_BYTES, wn * 64 + j * 16, kk, lane);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    if (more) {
      sa.store(nxt, tid);
      sb.store(nxt + A_BYTES, tid);
    }
    __syncthreads();
  }

  // lane holds C[m][n .. n + 3], m = m0 + wm * BM/2 + 16 i + (lane & 15), n = n0 + wn * 64 + 16 j +
  // 4 (lane >> 4); NO % 8 == 0 keeps every quad whole. Rows in [rows, cap) of a partial tile: zeros.
  const int mrow = m0 + wm * (BM / 2) + (lane & 15);
  const int ncol = n0 + wn * 64 + (lane >> 4) * 4;
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int m = mrow + i * 16;
    if (m >= p.cap) continue;
    const bool live = m < rows;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = ncol + j * 16;
      if (n >= p.NO) continue;
      ushort4 yo = make_ushort4(0, 0, 0, 0), zo = yo;
      if (live) {
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float x = acc[i][j][q];
          if (p.bias) {
            const int64_t bi = (int64_t)e * p.NO + n + q;
            x += p.bias_bf16 ? bf2f(((const bf16_t*)p.bias)[bi]) : ((const float*)p.bias)[bi];
          }
          v[q] = x;
        }
        zo = make_ushort4(f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3]));
        if (p.act != ACT_NONE) {
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = act_fwd(p.act, v[q]);
        }
        yo = make_ushort4(f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3]));
      }
      const int64_t o = (int64_t)m * p.NO + n;
      *reinterpret_cast<ushort4*>(Y + o) = yo;
      if (Z) *reinterpret_cast<ushort4*>(Z + o) = zo;
    }
  }
}

struct GluRowsArgs {
  ExpertPtrs a;       // X_e [cap][K]
  const bf16_t* w;    // [n][2F][K]: F gate rows, then F up rows, per expert
  const void* bias;   // optional [n][2F] in the same order, bf16 or fp32
  bf16_t* h;          // [n][cap][F]
  bf16_t* z;          // optional [n][cap][2F] = (zg | zu)
  const int* load;
  int cap, F, K, act, bias_bf16;
};

// Gated forward: one workgroup owns a BM x 64 tile of H_e. Its B stage holds the 64 gate rows and the 64
// up rows of those output columns, so accumulator slots j and j + 2 of a lane are zg and zu of the same
// element and act(zg) * zu is taken in registers from the fp32 sums. STAGED: the bf16 H tile and the two
// Z half tiles go through the LDS the K loop has left free (row r at r * 128 B, its eight 16-B chunks
// swizzled by r & 7: the lanes' 8-B writes and the 16-B reads both run without bank conflicts) and leave
// as whole 16-B row chunks, eight consecutive lanes to a 128-B row segment; otherwise each lane stores
// its 8-B quads straight from the accumulators.
template <int BM, bool STAGED>
__global__ void __launch_bounds__(NT, 2) experts_glu_rows_kernel(GluRowsArgs p) {
  constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2, STAGE_BYTES = A_BYTES + B_BYTES;
  constexpr int MI = BM / 32, BNH = 64, OUT_BYTES = BM * BNH * 2;
  static_assert(3 * OUT_BYTES <= 2 * STAGE_BYTES, "H and the two Z halves fit the K loop's LDS");
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int e = blockIdx.y;
  const int F = p.F, tn = (F + BNH - 1) / BNH;
  const bf16_t* A = p.a.p[e];
  const int rows = A ? live_rows(p.load, e, p.cap) : 0;
  int tile_m, tile_n;
  deal_tile<BM>(blockIdx.x, rows, tn, tile_m, tile_n);
  const int m0 = tile_m * BM, n0 = tile_n * BNH;
  bf16_t* H = p.h + (int64_t)e * p.cap * F;
  bf16_t* Z = p.z ? p.z + (int64_t)e * p.cap * 2 * F : nullptr;

  if (m0 >= rows) {  // nothing routed here: no operand load, no MFMA, the tile is zeros
    for (int id = tid; id < BM * (BNH / 8); id += NT) {
      const int m = m0 + (id >> 3), n = n0 + (id & 7) * 8;
      if (m < p.cap && n < F) {
        *reinterpret_cast<uint4*>(H + (int64_t)m * F + n) = make_uint4(0, 0, 0, 0);
        if (Z) {
          *reinterpret_cast<uint4*>(Z + (int64_t)m * 2 * F + n) = make_uint4(0, 0, 0, 0);
          *reinterpret_cast<uint4*>(Z + (int64_t)m * 2 * F + F + n) = make_uint4(0, 0, 0, 0);
        }
      }
    }
    return;
  }

  const bf16_t* W = p.w + (int64_t)e * 2 * F * p.K;
  f32x4 acc[MI][4];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  glu_mainloop<BM>(smem, A, W, p.K, F, m0, n0, rows, tid, lane, wm, wn, acc);

  // lane holds zg = acc[i][j], zu = acc[i][j + 2] of H[m][n .. n + 3], m = m0 + r, r = wm * BM/2 + 16 i +
  // (lane & 15), n = n0 + c, c = wn * 32 + 16 j + 4 (lane >> 4); F % 8 == 0 keeps every quad whole. Rows
  // in [rows, cap) of a partial tile: zeros. Columns at or beyond F have no bias and are not stored.
  const int r0 = wm * (BM / 2) + (lane & 15);
  const int c0 = wn * 32 + (lane >> 4) * 4;
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int r = r0 + i * 16, m = m0 + r;
    if (!STAGED && m >= p.cap) continue;
    const bool live = m < rows;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = c0 + j * 16, n = n0 + c;
      if (n >= F) continue;
      ushort4 ho = make_ushort4(0, 0, 0, 0), go = ho, uo = ho;
      if (live) {
        float g[4], u[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          g[q] = acc[i][j][q];
          u[q] = acc[i][j + 2][q];
          if (p.bias) {
            const int64_t bi = (int64_t)e * 2 * F + n + q;
            g[q] += p.bias_bf16 ? bf2f(((const bf16_t*)p.bias)[bi]) : ((const float*)p.bias)[bi];
            u[q] += p.bias_bf16 ? bf2f(((const bf16_t*)p.bias)[bi + F]) : ((const float*)p.bias)[bi + F];
          }
        }
        go = make_ushort4(f2bf(g[0]), f2bf(g[1]), f2bf(g[2]), f2bf(g[3]));
        uo = make_ushort4(f2bf(u[0]), f2bf(u[1]), f2bf(u[2]), f2bf(u[3]));
#pragma unroll
        for (int q = 0; q < 4; ++q) g[q] = glu_act(p.act, g[q]) * u[q];
        ho = make_ushort4(f2bf(g[0]), f2bf(g[1]), f2bf(g[2]), f2bf(g[3]));
      }
      if (STAGED) {
        char* q = smem + r * (BNH * 2) + (((c >> 3) ^ (r & 7)) << 4) + (c & 7) * 2;
        *reinterpret_cast<ushort4*>(q) = ho;
        if (Z) {
          *reinterpret_cast<ushort4*>(q + OUT_BYTES) = go;
          *reinterpret_cast<ushort4*>(q + 2 * OUT_BYTES) = uo;
        }
      } else {
        *reinterpret_cast<ushort4*>(H + (int64_t)m * F + n) = ho;
        if (Z) {
          *reinterpret_cast<ushort4*>(Z + (int64_t)m * 2 * F + n) = go;
          *reinterpret_cast<ushort4*>(Z + (int64_t)m * 2 * F + F + n) = uo;
        }
      }
    }
  }
  if (STAGED) {
    __syncthreads();
    for (int id = tid; id < BM * (BNH / 8); id += NT) {
      const int r = id >> 3, c8 = id & 7;
      const int m = m0 + r, n = n0 + c8 * 8;
      if (m < p.cap && n < F) {
        const char* q = smem + r * (BNH * 2) + ((c8 ^ (r & 7)) << 4);
        *reinterpret_cast<uint4*>(H + (int64_t)m * F + n) = *reinterpret_cast<const uint4*>(q);
        if (Z) {
          *reinterpret_cast<uint4*>(Z + (int64_t)m * 2 * F + n) = *reinterpret_cast<const uint4*>(q + OUT_BYTES);
          *reinterpret_cast<uint4*>(Z + (int64_t)m * 2 * F + F + n) = *reinterpret_cast<const uint4*>(q + 2 * OUT_BYTES);
        }
      }
    }
  }
}

struct WgradArgs {
  ExpertPtrs dz, x;  // [cap][N], [cap][K]
  const int* load;
  float* dw;         // [n][N][K], +=
  float* db;         // optional [n][N], +=
  int cap, N, K;
};

__global__ void __launch_bounds__(NT, 2) experts_wgrad_kernel(WgradArgs p) {
  constexpr int TILE_BYTES = BN * BK * 2, STAGE_BYTES = 2 * TILE_BYTES;
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int e = blockIdx.y;
  const bf16_t* A = p.dz.p[e];
  const bf16_t* B = p.x.p[e];
  const int rows = (A && B) ? live_rows(p.load, e, p.cap) : 0;
  if (rows == 0) return;  // the gradient is left alone
  const int tm = (p.N + 127) / 128, tn = (p.K + BN - 1) / BN;
  int tile_m, tile_n;
  tile_coords(blockIdx.x, tm, tn, tile_m, tile_n);
  const int m0 = tile_m * 128, n0 = tile_n * BN;
  const int nk = (rows + BK - 1) / BK;
  const bool do_db = p.db != nullptr && tile_n == 0;

  Stage<false, 128> sa, sb;
  float bsum[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) bsum[j] = 0.f;
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the reduction index is the row: k_lim = rows selects the rows of the last step at or beyond r_e to zero
  sa.load(A, p.N, m0, 0, p.N, rows, tid);
  sb.load(B, p.K, n0, 0, p.K, rows, tid);
  sa.store(smem, tid);
  sb.store(smem + TILE_BYTES, tid);
  if (do_db) sa.add_cols(bsum);
  __syncthreads();
  for (int t = 0; t < nk; ++t) {
    char* cur = smem + (t & 1) * STAGE_BYTES;
    char* nxt = smem + ((t + 1) & 1) * STAGE_BYTES;
    const bool more = (t + 1) < nk;
    if (more) {
      sa.load(A, p.N, m0, (t + 1) * BK, p.N, rows, tid);
      sb.load(B, p.K, n0, (t + 1) * BK, p.K, rows, tid);
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = frag<false, BK, false>(cur, wm * 64 + i * 16, kk, lane);
#pragma unroll
      for (int j = 0; j < 4; ++j) bfr[j] = frag<false, BK, false>(cur + TILE_BYTES, wn * 64 + j * 16, kk, lane);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    if (more) {
      sa.store(nxt, tid);
      sb.store(nxt + TILE_BYTES, tid);
      if (do_db) sa.add_cols(bsum);
    }
    __syncthreads();
  }

  const int mrow = m0 + wm * 64 + (lane & 15);
  const int ncol = n0 + wn * 64 + (lane >> 4) * 4;
  float* DW = p.dw + (int64_t)e * p.N * p.K;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = mrow + i * 16;
    if (m >= p.N) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = ncol + j * 16;
      if (n >= p.K) continue;
      float4* dst = reinterpret_cast<float4*>(DW + (int64_t)m * p.K + n);
      float4 c = *dst;
      c.x += acc[i][j][0]; c.y += acc[i][j][1]; c.z += acc[i][j][2]; c.w += acc[i][j][3];
      *dst = c;
    }
  }
  if (do_db) {  // block-uniform; the loop's last barrier freed the LDS
    float* red = reinterpret_cast<float*>(smem);  // [16 row groups][128 columns]
#pragma unroll
    for (int j = 0; j < 8; ++j) red[(tid >> 4) * 128 + (tid & 15) * 8 + j] = bsum[j];
    __syncthreads();
    if (tid < 128 && m0 + tid < p.N) {
      float s = 0.f;
#pragma unroll
      for (int g = 0; g < 16; ++g) s += red[g * 128 + tid];
      p.db[(int64_t)e * p.N + m0 + tid] += s;
    }
  }
}

// dZ_e[r, :] = dY_e[r, :] * act'(Z_e[r, :]) for r < r_e, 8 elements per thread and step; rows >= r_e
// of the dZ slab are not written (no grouped kernel reads them)
__global__ void __launch_bounds__(NT) experts_dact_kernel(ExpertPtrs dy, const bf16_t* __restrict__ z,
                                                         bf16_t* __restrict__ dz, const int* __restrict__ load,
                                                         int cap, int N, int act) {
  const int e = blockIdx.y;
  const bf16_t* g = dy.p[e];
  if (!g) return;
  const int64_t live = (int64_t)live_rows(load, e, cap) * N;
  const int64_t base = (int64_t)e * cap * N;
  for (int64_t i = ((int64_t)blockIdx.x * NT + threadIdx.x) * 8; i < live; i += (int64_t)gridDim.x * NT * 8) {
    float a[8], b[8];
    load16(g + i, a);
    load16(z + base + i, b);
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] *= act_grad(act, b[j]);
    store16(dz + base + i, a);
  }
}

// Gate backward over the live rows of every expert, one 16-B chunk of dH (8 columns) per thread and step:
// dZ_e[r, c] = dH_e[r, c] * Zu * act'(Zg), dZ_e[r, F + c] = dH_e[r, c] * act(Zg), act and act' from one
// glu_act_grad. Rows >= r_e of the dZ slab are not written (no grouped kernel reads them).
__global__ void __launch_bounds__(NT) experts_glu_bwd_kernel(ExpertPtrs dh, const bf16_t* __restrict__ z,
                                                            bf16_t* __restrict__ dz, const int* __restrict__ load,
                                                            int cap, int F, int act) {
  const int e = blockIdx.y;
  const bf16_t* g = dh.p[e];
  if (!g) return;
  const int f8 = F >> 3;
  const int64_t live = (int64_t)live_rows(load, e, cap) * f8;
  const int64_t base = (int64_t)e * cap * 2 * F;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < live; i += (int64_t)gridDim.x * NT) {
    const int64_t r = i / f8;
    const int c = (int)(i - r * f8) * 8;
    const int64_t o = base + r * 2 * F + c;
    float d[8], a[8], b[8];
    load16(g + r * F + c, d);
    load16(z + o, a);
    load16(z + o + F, b);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float y, dy;
      glu_act_grad(act, a[j], y, dy);
      a[j] = d[j] * b[j] * dy;
      b[j] = d[j] * y;
    }
    store16(dz + o, a);
    store16(dz + o + F, b);
  }
}

bool al16(const void* q) { return ((uintptr_t)q & 15) == 0; }

// pointer table of n experts; false when one is misaligned (null = an expert without rows)
bool fill_table(ExpertPtrs& t, const void* const* ptrs, int n) {
  for (int i = 0; i < kMoeMaxExperts; ++i) {
    t.p[i] = i < n ? reinterpret_cast<const bf16_t*>(ptrs[i]) : nullptr;
    if (!al16(t.p[i])) return false;
  }
  return true;
}

bool shape_ok(int n, int cap, int N, int K) {
  return n >= 1 && n <= kMoeMaxExperts && cap >= 1 && N >= 8 && K >= 8 && N % 8 == 0 && K % 8 == 0;
}

template <bool B_K>
void launch_rows(const RowsArgs& p, int n, int tile_m, hipStream_t st) {
  const bool small = tile_m == 64 || (tile_m == 0 && experts_tile_m(p.cap) == 64);
  const int bm = small ? 64 : 128;
  dim3 grid(((p.cap + bm - 1) / bm) * ((p.NO + BN - 1) / BN), n);
  if (small) hipLaunchKernelGGL((experts_rows_kernel<64, B_K>), grid, dim3(NT), 0, st, p);
  else hipLaunchKernelGGL((experts_rows_kernel<128, B_K>), grid, dim3(NT), 0, st, p);
}

}  // namespace

int experts_tile_m(int cap) { return cap <= 512 ? 64 : 128; }

bool experts_fwd(const void* const* xs, int n, const void* w, const void* bias, int bias_bf16, const int* load,
                 void* y, void* z, int cap, int N, int K, int act, int tile_m, hipStream_t st) {
  RowsArgs p;
  if (!shape_ok(n, cap, N, K) || !fill_table(p.a, xs, n) || !al16(w) || !al16(y) || !al16(z)) return false;
  p.w = reinterpret_cast<const bf16_t*>(w);
  p.bias = bias;
  p.bias_bf16 = bias_bf16;
  p.y = reinterpret_cast<bf16_t*>(y);
  p.z = reinterpret_cast<bf16_t*>(z);
  p.load = load;
  p.w_stride = (int64_t)N * K;
  p.cap = cap; p.NO = N; p.KR = K; p.ldw = K; p.act = act;
  launch_rows<true>(p, n, tile_m, st);
  return true;
}

bool experts_bwd_data(const void* const* dzs, int n, const void* w, const int* load, void* dx, int cap, int N, int K,
                      int tile_m, hipStream_t st) {
  RowsArgs p;
  if (!shape_ok(n, cap, N, K) || !fill_table(p.a, dzs, n) || !al16(w) || !al16(dx)) return false;
  p.w = reinterpret_cast<const bf16_t*>(w);
  p.bias = nullptr;
  p.bias_bf16 = 0;
  p.y = reinterpret_cast<bf16_t*>(dx);
  p.z = nullptr;
  p.load = load;
  p.w_stride = (int64_t)N * K;
  p.cap = cap; p.NO = K; p.KR = N; p.ldw = K; p.act = ACT_NONE;
  launch_rows<false>(p, n, tile_m, st);
  return true;
}

bool experts_bwd_weight(const void* const* dzs, const void* const* xs, int n, const int* load, float* dw, float* db,
                        int cap, int N, int K, hipStream_t st) {
  WgradArgs p;
  if (!shape_ok(n, cap, N, K) || !fill_table(p.dz, dzs, n) || !fill_table(p.x, xs, n) || !al16(dw)) return false;
  p.load = load;
  p.dw = dw;
  p.db = db;
  p.cap = cap; p.N = N; p.K = K;
  dim3 grid(((N + 127) / 128) * ((K + BN - 1) / BN), n);
  hipLaunchKernelGGL(experts_wgrad_kernel, grid, dim3(NT), 0, st, p);
  return true;
}

bool experts_act_bwd(const void* const* dys, int n, const void* z, void* dz, const int* load, int cap, int N, int act,
                     hipStream_t st) {
  ExpertPtrs t;
  if (!shape_ok(n, cap, N, 8) || !fill_table(t, dys, n) || !al16(z) || !al16(dz)) return false;
  const int64_t chunks = ((int64_t)cap * N / 8 + NT - 1) / NT;
  const int gx = (int)std::max<int64_t>(1, std::min<int64_t>(chunks, 2048 / n));
  hipLaunchKernelGGL(experts_dact_kernel, dim3(gx, n), dim3(NT), 0, st, t, reinterpret_cast<const bf16_t*>(z),
                     reinterpret_cast<bf16_t*>(dz), load, cap, N, act);
  return true;
}

namespace {

// The default epilogue of the gated forward (docs/PERFORMANCE.md, 'Gated expert GEMMs')
constexpr bool kGluStagedEpilogue = true;

template <bool STAGED>
void launch_glu_rows(const GluRowsArgs& p, int n, int tile_m, hipStream_t st) {
  const bool small = tile_m == 64 || (tile_m == 0 && experts_tile_m(p.cap) == 64);
  const int bm = small ? 64 : 128;
  dim3 grid(((p.cap + bm - 1) / bm) * ((p.F + 63) / 64), n);
  if (small) hipLaunchKernelGGL((experts_glu_rows_kernel<64, STAGED>), grid, dim3(NT), 0, st, p);
  else hipLaunchKernelGGL((experts_glu_rows_kernel<128, STAGED>), grid, dim3(NT), 0, st, p);
}

}  // namespace

bool experts_glu_fwd(const void* const* xs, int n, const void* w, const void* bias, int bias_bf16, const int* load,
                     void* h, void* z, int cap, int F, int K, int act, int tile_m, int epilogue, hipStream_t st) {
  GluRowsArgs p;
  if (!shape_ok(n, cap, F, K) || !fill_table(p.a, xs, n) || !al16(w) || !al16(h) || !al16(z)) return false;
  p.w = reinterpret_cast<const bf16_t*>(w);
  p.bias = bias;
  p.bias_bf16 = bias_bf16;
  p.h = reinterpret_cast<bf16_t*>(h);
  p.z = reinterpret_cast<bf16_t*>(z);
  p.load = load;
  p.cap = cap; p.F = F; p.K = K; p.act = act;
  if (epilogue == 1 || (epilogue == 0 && kGluStagedEpilogue)) launch_glu_rows<true>(p, n, tile_m, st);
  else launch_glu_rows<false>(p, n, tile_m, st);
  return true;
}

bool experts_glu_bwd(const void* const* dhs, int n, const void* z, void* dz, const int* load, int cap, int F, int act,
                     hipStream_t st) {
  ExpertPtrs t;
  if (!shape_ok(n, cap, F, 8) || !fill_table(t, dhs, n) || !al16(z) || !al16(dz)) return false;
  const int64_t chunks = ((int64_t)cap * F / 8 + NT - 1) / NT;
  const int gx = (int)std::max<int64_t>(1, std::min<int64_t>(chunks, 2048 / n));
  hipLaunchKernelGGL(experts_glu_bwd_kernel, dim3(gx, n), dim3(NT), 0, st, t, reinterpret_cast<const bf16_t*>(z),
                     reinterpret_cast<bf16_t*>(dz), load, cap, F, act);
  return true;
}

}  // namespace ffk
