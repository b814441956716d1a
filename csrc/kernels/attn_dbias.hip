// Gradient of the attention score bias (AttnArgs.dsbias), bf16 operands, fp32 result, gfx950 MFMA
// 32x32x16.
//
//   dsbias[bb][hb][q][k] = sum_{b in R(bb)} sum_{h in R(hb)} P0 (dP' - delta)        (no factor scale)
//   P0  = exp2(scale log2e q.k + bias log2e - lse2), 0 where the forward removed the key
//   dP' = dO.V^T, keep ? dP drop_scale : 0 with dropout
//
// R(bb) is every batch index when the bias has batch extent 1 and {bb} otherwise, R(hb) the same over
// heads. The flash backward (attention.hip) forms the same dS per key block and drops it; summing it
// over the batch there would take atomics or [B][H][Sq][Sk] slabs. Here the work is split by the
// OUTPUT instead:
//
//  * One workgroup owns one (bb, hb, TM query x TM key) tile of dsbias and walks its reduction set, b
//    ascending and h ascending inside it, with the tile's dS sum in fp32 MFMA accumulators from the
//    first step to the last. Every element is written once, by one lane, after one fixed order of
//    additions: no atomics, no intermediate, no finishing pass, the same bits on every run.
//  * 4 waves as 2 x 2, each owning a (TM/2) x (TM/2) corner as 32 x 32 blocks. The MFMA runs
//    transposed, S^T = K.Q^T and dP^T = V.dO^T (K / V rows as the A operand), so that a lane owns ONE
//    query row and, per register quad, 4 CONSECUTIVE keys: lse2 / delta / the dropout row key are one
//    value per lane and block row, a quad's dropout bytes are one hash, the bias comes in and the
//    result leaves as 16-B vectors along a bias row (4-B predicated accesses where Sk % 4 != 0 or a
//    base is not 16-B aligned). Nothing is read or written at or past Sq / Sk.
//  * What does not change along the reduction lives in registers for the whole loop: the reduction
//    runs over broadcast dims only, so the tile's bias is the same at every step. It is loaded once,
//    premultiplied by log2e, and the causal diagonal and the keys past Sk are folded into it as -inf.
//    Only the per-sample key length is tested per step, on the blocks that cross it.
//  * Per step the [TM][D] Q, dO, K and V tiles and the lse2 / delta rows of (b, h) go global -> LDS by
//    LDS-DMA into the swizzled images of attn_tile.h, double-buffered: step i + 1 is requested right
//    behind the barrier that opens step i, and is waited for at the barrier that opens step i + 1.
//    One barrier per step. D = 64: TM = 128 (2 x 65 KiB of the 160 KiB LDS). D = 128: four
//    double-buffered 128-row tiles would take 256 KiB, so TM = 64 there (the same 2 x 65 KiB), each
//    wave one 32 x 32 block.
//  * A wave reads every fragment of its Q / dO / K / V rows once per step, all at the top of the step
//    (128 registers; the workgroup has a CU to itself, so a wave may use 512), and the next step's DMA
//    is requested behind those reads: no LDS read is issued while a DMA is in flight, which hipcc
//    would guard with a wait for the DMA. S and dP of one 32 x 32 block are the only transient
//    accumulators.
//  * A tile wholly above the causal diagonal writes zeros and loads nothing; a key tile wholly past
//    key_lens[b] skips b's steps; blocks above the diagonal or past the length skip their MFMAs.
//  * 1-D grid through xcd_remap with the tiles of one (bb, hb) adjacent: the workgroups that read one
//    head's Q / dO / K / V share an XCD and its L2.
//  * Operands whose rows are not 16-B aligned (or lie past the 2 GiB a buffer offset reaches) take the
//    DMA = false form: the same step staged through registers (TileStage), single-buffered.
//
// The kernel is bound by L2 -> LDS traffic, not by the matrix core: a step moves 64 KiB for
// 2 x 2 TM^2 D flops (64 flop / B at D = 64), see docs/PERFORMANCE.md 'Score-bias gradient'.
#include "common.h"
#include "attention.h"
#include "attn_tile.h"
#include "attn_dropout.h"
#include <utility>

namespace ffk {

template <int D, bool DROP, bool DMA>
__global__ void __launch_bounds__(256, 1) attn_dbias_kernel(AttnArgs a) {
  constexpr int TM = D == 64 ? 128 : 64;  // tile edge (queries and keys)
  constexpr int WT = TM / 2;              // a wave's edge
  constexpr int NB = WT / 32;             // its 32 x 32 blocks per dim
  constexpr int TB = TM * D * 2;          // bytes of one operand tile
  constexpr int BUF = 4 * TB + 2 * TM * 4;  // Q, dO, K, V, lse2, delta
  constexpr int NBUF = DMA ? 2 : 1;
  __shared__ __attribute__((aligned(16))) char smem[NBUF * BUF];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h2 = lane >> 5, l31 = lane & 31;
  const int wq = wave >> 1, wk = wave & 1;
  const int ntq = (a.Sq + TM - 1) / TM, ntk = (a.Sk + TM - 1) / TM;
  const int Bb = a.sbias_sb ? a.B : 1, Hb = a.sbias_sh ? a.H : 1;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int tile = lid % (ntq * ntk), slab = lid / (ntq * ntk);
  const int bb = slab / Hb, hb = slab % Hb;
  const int q0 = (tile / ntk) * TM, k0 = (tile % ntk) * TM;
  const int b_lo = Bb > 1 ? bb : 0, b_hi = Bb > 1 ? bb + 1 : a.B;
  const int h_lo = Hb > 1 ? hb : 0, h_hi = Hb > 1 ? hb + 1 : a.H;

  // the lane's rows and key quads; element r of block (qb, kb) is query qrow[qb], key
  // kblk(kb) + 4 h2 + (r & 3) + 8 (r >> 2)
  int qrow[NB];
#pragma unroll
  for (int qb = 0; qb < NB; ++qb) qrow[qb] = q0 + wq * WT + 32 * qb + l31;
  auto kblk = [&](int kb) __attribute__((always_inline)) { return k0 + wk * WT + 32 * kb; };

  const int64_t slab_off = (int64_t)bb * a.sbias_sb + (int64_t)hb * a.sbias_sh;
  float* out = a.dsbias + slab_off;
  const bool dvec = (((uintptr_t)a.dsbias | (uintptr_t)(a.sbias_sb * 4) | (uintptr_t)(a.sbias_sh * 4) | (uintptr_t)(a.Sk * 4)) & 15) == 0;
  f32x16 acc[NB][NB];
#pragma unroll
  for (int qb = 0; qb < NB; ++qb)
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) acc[qb][kb] = f32x16{};

  auto store_out = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int qb = 0; qb < NB; ++qb) {
      if (qrow[qb] >= a.Sq) continue;
      float* orow = out + (int64_t)qrow[qb] * a.Sk;
#pragma unroll
      for (int kb = 0; kb < NB; ++kb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int key = kblk(kb) + 4 * h2 + 8 * g;
          const f32x16& c = acc[qb][kb];
          if (dvec && key < a.Sk) {  // Sk % 4 == 0 and key % 4 == 0: the quad ends inside the row
            *reinterpret_cast<float4*>(orow + key) = make_float4(c[4 * g], c[4 * g + 1], c[4 * g + 2], c[4 * g + 3]);
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (key + j < a.Sk) orow[key + j] = c[4 * g + j];
          }
        }
    }
  };

  // wholly above the causal diagonal (smallest key > largest query): zeros, nothing loaded
  if (a.causal && k0 > q0 + TM - 1) {
    store_out();
    return;
  }

  // the tile's bias in log2 units, constant along the reduction; -inf: the causal diagonal, keys
  // past Sk, and what the bias itself removes (-inf, or a product that overflows)
  float bl[NB][NB][16];
  {
    const float* bias = a.sbias + slab_off;
    const bool bvec = (((uintptr_t)a.sbias | (uintptr_t)(a.sbias_sb * 4) | (uintptr_t)(a.sbias_sh * 4) | (uintptr_t)(a.Sk * 4)) & 15) == 0;
#pragma unroll
    for (int qb = 0; qb < NB; ++qb) {
      const float* brow = bias + (int64_t)min(qrow[qb], a.Sq - 1) * a.Sk;
#pragma unroll
      for (int kb = 0; kb < NB; ++kb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int key = kblk(kb) + 4 * h2 + 8 * g;
          float v[4];
          if (bvec && key < a.Sk) {
            const float4 q4 = *reinterpret_cast<const float4*>(brow + key);
            v[0] = q4.x; v[1] = q4.y; v[2] = q4.z; v[3] = q4.w;
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = key + j < a.Sk ? brow[key + j] : 0.f;
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const bool off = key + j >= a.Sk || (a.causal && key + j > qrow[qb]);
            bl[qb][kb][4 * g + j] = off ? -INFINITY : v[j] * LOG2E;
          }
        }
    }
  }

  const float sl2 = a.scale * LOG2E;
  const int64_t rstep = DROP ? (a.rng_step ? *a.rng_step : 0) : 0;  // uniform: one scalar load

  // the reduction set in its order, without the samples whose keys end at or before this key tile
  auto live_b = [&](int b) __attribute__((always_inline)) { return key_limit<true>(a, b) > k0; };
  int b = b_lo, h = h_lo;
  while (b < b_hi && !live_b(b)) ++b;
  bool live = b < b_hi;
  auto next = [&](int& nb, int& nh) __attribute__((always_inline)) {
    if (++nh < h_hi) return true;
    nh = h_lo;
    do ++nb; while (nb < b_hi && !live_b(nb));
    return nb < b_hi;
  };

  // step (sb, sh) into a buffer: LDS-DMA, rows past Sq / Sk read as zero (buffer range check)
  auto dma_step = [&](char* buf, int sb, int sh) __attribute__((always_inline)) {
    const int hk = a.G == 1 ? sh : sh / a.G;  // grouped-query attention: the KV head of query head sh
    const bf16_t* Q = a.q + (int64_t)sb * a.q_sb + (int64_t)sh * a.q_sh;
    const bf16_t* dO = a.dout + (int64_t)sb * a.do_sb + (int64_t)sh * a.do_sh;
    const bf16_t* K = a.k + (int64_t)sb * a.k_sb + (int64_t)hk * a.k_sh;
    const bf16_t* V = a.v + (int64_t)sb * a.v_sb + (int64_t)hk * a.v_sh;
    auto rsrc = [](const void* p, int64_t bytes) {
      return __builtin_amdgcn_make_buffer_rsrc((void*)p, (short)0, (int)min((int64_t)0x7fffffff, bytes), 0x00020000);
    };
    const __amdgpu_buffer_rsrc_t rq = rsrc(Q, ((int64_t)(a.Sq - 1) * a.q_ss + D) * 2);
    const __amdgpu_buffer_rsrc_t rd = rsrc(dO, ((int64_t)(a.Sq - 1) * a.do_ss + D) * 2);
    const __amdgpu_buffer_rsrc_t rk = rsrc(K, ((int64_t)(a.Sk - 1) * a.k_ss + D) * 2);
    const __amdgpu_buffer_rsrc_t rv = rsrc(V, ((int64_t)(a.Sk - 1) * a.v_ss + D) * 2);
#pragma unroll
    for (int j = 0; j < TM / 64; ++j) {
      dma_tile<D, 4>(rq, buf + j * 64 * D * 2, a.q_ss, q0 + 64 * j, wave, lane);
      dma_tile<D, 4>(rd, buf + TB + j * 64 * D * 2, a.do_ss, q0 + 64 * j, wave, lane);
      dma_tile<D, 4>(rk, buf + 2 * TB + j * 64 * D * 2, a.k_ss, k0 + 64 * j, wave, lane);
      dma_tile<D, 4>(rv, buf + 3 * TB + j * 64 * D * 2, a.v_ss, k0 + 64 * j, wave, lane);
    }
    // lse2 then delta, 64 rows per wave instruction
    const int64_t row0 = ((int64_t)sb * a.H + sh) * a.Sq;
    if (wave < 2 * (TM / 64)) {
      const int which = wave / (TM / 64), piece = wave % (TM / 64);
      const __amdgpu_buffer_rsrc_t rr = rsrc((which ? a.delta : a.lse2) + row0, (int64_t)a.Sq * 4);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rr, (lds_ptr_t)(buf + 4 * TB + which * TM * 4 + piece * 256), 4,
                                               (q0 + 64 * piece + lane) * 4, 0, 0, 0);
    }
  };
  // the same through registers, one operand at a time
  auto stage_step = [&](char* buf, int sb, int sh) __attribute__((always_inline)) {
    const int hk = a.G == 1 ? sh : sh / a.G;
    TileStage<D, TM, 256> st;
    st.load(a.q + (int64_t)sb * a.q_sb + (int64_t)sh * a.q_sh, a.q_ss, q0, a.Sq, tid);
    st.store(buf, tid);
    st.load(a.dout + (int64_t)sb * a.do_sb + (int64_t)sh * a.do_sh, a.do_ss, q0, a.Sq, tid);
    st.store(buf + TB, tid);
    st.load(a.k + (int64_t)sb * a.k_sb + (int64_t)hk * a.k_sh, a.k_ss, k0, a.Sk, tid);
    st.store(buf + 2 * TB, tid);
    st.load(a.v + (int64_t)sb * a.v_sb + (int64_t)hk * a.v_sh, a.v_ss, k0, a.Sk, tid);
    st.store(buf + 3 * TB, tid);
    if (tid < 2 * TM) {
      const int which = tid / TM, r = tid % TM;
      const float* src = (which ? a.delta : a.lse2) + ((int64_t)sb * a.H + sh) * a.Sq;
      reinterpret_cast<float*>(buf + 4 * TB)[tid] = q0 + r < a.Sq ? src[q0 + r] : 0.f;
    }
  };

  // a step's operands, read from LDS in one go at the top of the step: the next step's LDS-DMA is
  // requested behind these reads and nothing reads LDS while it is in flight (hipcc waits for every
  // outstanding LDS-DMA in front of an LDS read it cannot tell apart from the DMA's target)
  bf16x8 qf[NB][D / 16], df[NB][D / 16], kf[NB][D / 16], vf[NB][D / 16];
  float l2[NB], dl[NB];
  auto read_frags = [&](const char* buf) __attribute__((always_inline)) {
    const float* lse_l = reinterpret_cast<const float*>(buf + 4 * TB);
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int qr = wq * WT + 32 * i + l31, kr = wk * WT + 32 * i + l31;
      l2[i] = lse_l[qr];
      dl[i] = lse_l[TM + qr];
#pragma unroll
      for (int s = 0; s < D / 16; ++s) {
        qf[i][s] = *reinterpret_cast<const bf16x8*>(buf + aoff<D>(qr, 16 * s + 8 * h2));
        df[i][s] = *reinterpret_cast<const bf16x8*>(buf + TB + aoff<D>(qr, 16 * s + 8 * h2));
        kf[i][s] = *reinterpret_cast<const bf16x8*>(buf + 2 * TB + aoff<D>(kr, 16 * s + 8 * h2));
        vf[i][s] = *reinterpret_cast<const bf16x8*>(buf + 3 * TB + aoff<D>(kr, 16 * s + 8 * h2));
      }
    }
  };

  auto compute = [&](int sb, int sh) __attribute__((always_inline)) {
    const int klim = key_limit<true>(a, sb);
    uint64_t hkey = 0;
    if constexpr (DROP) hkey = attn_dropout_head_key(a.rng_seed, rstep, (int64_t)(a.b0 + sb) * a.H_total + a.h0 + sh);
    uint32_t rkey[NB];
#pragma unroll
    for (int qb = 0; qb < NB; ++qb) rkey[qb] = DROP ? attn_dropout_row_key(hkey, qrow[qb]) : 0u;
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
      const int kbase = kblk(kb);
      if (kbase >= klim) continue;  // past the sample's keys: P = 0 (also covers keys past Sk)
      const bool cut = kbase + 32 > klim;  // the length ends inside the block (wave-uniform)
#pragma unroll
      for (int qb = 0; qb < NB; ++qb) {
        if (a.causal && kbase > q0 + wq * WT + 32 * qb + 31) continue;  // the block lies above the diagonal
        // S^T[key][q] and dP^T[key][q]: the lane's query column, keys down the registers
        f32x16 sacc = f32x16{}, pacc = f32x16{};
#pragma unroll
        for (int s = 0; s < D / 16; ++s) {
          sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kb][s], qf[qb][s], sacc, 0, 0, 0);
          pacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[kb][s], df[qb][s], pacc, 0, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int key = kbase + 4 * h2 + 8 * g;
          uint32_t w = 0;
          if constexpr (DROP) w = attn_dropout_word(rkey[qb], (uint32_t)(key >> 2) * ADROP_KMUL);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int r = 4 * g + j;
            // -inf from the bias, or lse2 = +inf of a dead row, gives exp2(-inf) = 0, never NaN
            float p = fast_exp2(__builtin_fmaf(sacc[r], sl2, bl[qb][kb][r]) - l2[qb]);
            if (cut && key + j >= klim) p = 0.f;
            float dp = pacc[r];
            if constexpr (DROP) dp = ((w >> (8 * j)) & 255u) >= a.drop_thr ? dp * a.drop_scale : 0.f;
            acc[qb][kb][r] = __builtin_fmaf(p, dp - dl[qb], acc[qb][kb][r]);
          }
        }
      }
    }
  };

  if constexpr (DMA) {
    if (live) dma_step(smem, b, h);
  }
  // one step; the buffer index is a compile-time constant (the loop is unrolled by two)
  auto body = [&](auto par) __attribute__((always_inline)) {
    constexpr int P = DMA ? decltype(par)::value : 0;
    char* cur = smem + P * BUF;
    int nb = b, nh = h;
    const bool more = next(nb, nh);
    if constexpr (DMA) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();  // this step's tiles are in; every wave is done with the other buffer
      read_frags(cur);
      if (more) dma_step(smem + (P ^ 1) * BUF, nb, nh);
    } else {
      __syncthreads();
      stage_step(cur, b, h);
      __syncthreads();
      read_frags(cur);
    }
    compute(b, h);
    b = nb;
    h = nh;
    live = more;
  };
  while (live) {
    body(std::integral_constant<int, 0>{});
    if (!live) break;
    body(std::integral_constant<int, 1>{});
  }
  store_out();
}

// LDS-DMA staging of a [rows][D] operand: 16-B aligned rows, buffer offsets below 2 GiB one tile past
// the last row included
static bool dbias_dma_ok(const void* p, int64_t sb, int64_t sh, int64_t ss, int rows) {
  return ((uintptr_t)p & 15) == 0 && sb % 8 == 0 && sh % 8 == 0 && ss % 8 == 0 && (int64_t)(rows + 128) * ss * 2 < 0x7fffffffLL;
}

void attn_dbias(const AttnArgs& a, hipStream_t st) {
  if (!a.dsbias || !a.sbias || (a.D != 64 && a.D != 128) || a.B <= 0 || a.H <= 0 || a.Sq <= 0 || a.Sk <= 0) return;
  const int TM = a.D == 64 ? 128 : 64;
  const int64_t tiles = (int64_t)((a.Sq + TM - 1) / TM) * ((a.Sk + TM - 1) / TM);
  const dim3 grid((unsigned)(tiles * (a.sbias_sb ? a.B : 1) * (a.sbias_sh ? a.H : 1)));
  const bool dma = dbias_dma_ok(a.q, a.q_sb, a.q_sh, a.q_ss, a.Sq) && dbias_dma_ok(a.dout, a.do_sb, a.do_sh, a.do_ss, a.Sq) &&
                   dbias_dma_ok(a.k, a.k_sb, a.k_sh, a.k_ss, a.Sk) && dbias_dma_ok(a.v, a.v_sb, a.v_sh, a.v_ss, a.Sk);
  const bool drop = a.drop_thr > 0;
  auto go = [&](auto d) {
    constexpr int D = decltype(d)::value;
    if (drop && dma) hipLaunchKernelGGL((attn_dbias_kernel<D, true, true>), grid, dim3(256), 0, st, a);
    else if (drop) hipLaunchKernelGGL((attn_dbias_kernel<D, true, false>), grid, dim3(256), 0, st, a);
    else if (dma) hipLaunchKernelGGL((attn_dbias_kernel<D, false, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((attn_dbias_kernel<D, false, false>), grid, dim3(256), 0, st, a);
  };
  if (a.D == 64) go(std::integral_constant<int, 64>{});
  else go(std::integral_constant<int, 128>{});
}

}  // namespace ffk
