// QK-norm fused with rotary: per-head RMSNorm of the projected Q and K head rows with a learned [D]
// weight each, then the rotation of rope.hip on the unrounded result, in ONE memory-bound launch per
// direction (ops.h QkNormArgs has the definition). The forward is out of place (the pre-norm heads
// are what the backward needs), the backward writes dx over dz where the flash kernel left it.
//
// Work split. A head row is short (D <= 256), so it belongs to LPR = D / 16 adjacent lanes, not to a
// wave: lane c of the group holds two 8-element chunks of the row in registers, chosen so that the
// rotation pair is lane-local:
//   half-split, c < rd/16   chunks [8c, 8c + 8) and [rd/2 + 8c, rd/2 + 8c + 8): pairs (i, i + rd/2)
//   interleaved, 16c < rd   chunks [16c, 16c + 8) and [16c + 8, 16c + 16): pairs (2k, 2k + 1)
//   behind the rotated part the same 16 contiguous columns, not rotated.
// Either way the lane reads table[p][8c .. 8c + 8): four float4. The sum of squares (forward) and
// sum(g w xhat) (backward) cross the group in log2(LPR) __shfl_xor steps: no LDS, no barrier.
// A 256-thread workgroup is G = 256 / LPR such groups and owns a fixed, contiguous range of tokens;
// group g takes tokens g, g + G, ... of it. A lane fetches its token's (cos, sin) and its slices of
// wq / wk once and reuses them over the token's H + Hkv head rows, which it walks in batches of
// QKN_ROWS rows whose loads are all issued before the first store. Small problems spread the row
// batches over blockIdx.y as well (qkn_plan), large ones keep them in one workgroup.
// dw: a lane adds g * xhat of its 16 columns over all of its rows in registers; at the end the
// workgroup folds its G groups through LDS in a fixed order and stores one fp32 row per weight into
// the slab [2][groups][D]; col_reduce_add2 folds the slab rows in a fixed order. No float atomics:
// dw has the same bits every run.
// The general form (fp32, D not 32 / 64 / 128 / 256, rd % 16 != 0, strides or pointers that do not
// fit 16-byte accesses) works at pair granularity: a wave owns a token, lane l the pairs l and
// l + 64 of each of its head rows, the workgroup's four waves fold dw through LDS the same way.
// Tails (tokens past the last full workgroup, head rows past a multiple of the batch, rows of the
// shorter tensor) are bounds-checked, not padded.
#include "common.h"
#include "ops.h"

namespace ffk {

namespace {

constexpr int QKN_BLOCK = 256;
constexpr int QKN_ROWS = 4;      // head rows whose loads are in flight together: 8 x 16 B a lane
constexpr int QKN_ROWS_BWD = 2;  // the backward loads x and dz: the same 8 x 16 B, half the registers
constexpr int QKN_TARGET_WG = 1024;  // workgroups wanted before tokens are stacked: 4 per CU

// how a launch is cut: gx workgroups of tpw contiguous tokens each, times gy slices of the row batches
struct QknPlan {
  int64_t tokens;
  int smax, tpw, gx, gy;
  int nbq, nb;  // row batches of the first tensor / of both
};

QknPlan qkn_plan(int64_t tokens, int H0, int H1, int G, int rows_per_batch) {
  QknPlan p;
  p.tokens = tokens;
  p.smax = 0;
  p.nbq = ceil_div(H0, rows_per_batch);
  p.nb = p.nbq + ceil_div(H1, rows_per_batch);
  p.tpw = G;
  int64_t gx = ceil_div64(tokens, G);
  int gy = std::max(p.nb, 1);
  while (gx * gy > QKN_TARGET_WG && gy > 1) gy = ceil_div(gy, 2);
  if (gx * gy > QKN_TARGET_WG) {
    p.tpw = G * (int)ceil_div64(gx, QKN_TARGET_WG);
    gx = ceil_div64(tokens, p.tpw);
  }
  p.gx = (int)std::max<int64_t>(gx, 1);
  p.gy = gy;
  return p;
}
QknPlan qkn_plan_vec(int64_t tokens, int H0, int H1, int D, bool bwd) {
  return qkn_plan(tokens, H0, H1, QKN_BLOCK / (D / 16), bwd ? QKN_ROWS_BWD : QKN_ROWS);
}
// the general form walks all rows of a token in one wave: one "batch" per tensor, gy = 1
QknPlan qkn_plan_gen(int64_t tokens, int H0, int H1) {
  QknPlan p = qkn_plan(tokens, H0 ? 1 : 0, H1 ? 1 : 0, QKN_BLOCK / 64, 1);
  if (p.gy > 1) p.gy = 1;
  return p;
}
bool qkn_vec_dim(int D) { return D == 32 || D == 64 || D == 128 || D == 256; }

__device__ __forceinline__ float wload(const void* w, int wdt, int e) {
  return wdt == DT_BF16 ? bf2f(static_cast<const bf16_t*>(w)[e]) : static_cast<const float*>(w)[e];
}

__device__ __forceinline__ int qkn_pos(const QkNormArgs& a, int b, int s, int smax) {
  const int p = a.pos ? a.pos[(int64_t)b * smax + s] : s;
  return min(max(p, 0), a.max_pos - 1);
}

// ------------------------------------------------------------------------------ 16-byte form (bf16)
// the lane's two chunks and whether they rotate
__device__ __forceinline__ void qkn_cols(int rd, int inter, int c, int& e1, int& e2, bool& rot) {
  rot = 16 * c < rd;
  if (rot && !inter) e1 = 8 * c, e2 = (rd >> 1) + 8 * c;
  else e1 = 16 * c, e2 = 16 * c + 8;
}

__device__ __forceinline__ void qkn_unpack(const uint4& r1, const uint4& r2, float* x) {
  const bf16_t* a = reinterpret_cast<const bf16_t*>(&r1);
  const bf16_t* b = reinterpret_cast<const bf16_t*>(&r2);
#pragma unroll
  for (int i = 0; i < 8; ++i) x[i] = bf2f(a[i]), x[8 + i] = bf2f(b[i]);
}

// y <- R(y) in registers; sn already carries the direction's sign
__device__ __forceinline__ void qkn_rotate(float* y, const float* cs, const float* sn, int inter) {
  if (inter) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float a = y[2 * k], b = y[2 * k + 1];
      y[2 * k] = a * cs[k] - b * sn[k];
      y[2 * k + 1] = b * cs[k] + a * sn[k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float a = y[k], b = y[8 + k];
      y[k] = a * cs[k] - b * sn[k];
      y[8 + k] = b * cs[k] + a * sn[k];
    }
  }
}

__device__ __forceinline__ void qkn_table(const QkNormArgs& a, int p, int c, bool inverse, float* cs, float* sn) {
  const float4* tp = reinterpret_cast<const float4*>(a.table + ((int64_t)p * (a.rd >> 1) + 8 * c) * 2);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float4 t = tp[k];
    cs[2 * k] = t.x, cs[2 * k + 1] = t.z;
    sn[2 * k] = inverse ? -t.y : t.y, sn[2 * k + 1] = inverse ? -t.w : t.w;
  }
}

template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

template <int LPR>
__global__ __launch_bounds__(QKN_BLOCK) void qkn_fwd_vec(QkNormArgs a, QknPlan p) {
  constexpr int G = QKN_BLOCK / LPR, R = QKN_ROWS;
  const int c = threadIdx.x % LPR, g = threadIdx.x / LPR;
  int e1, e2;
  bool rot;
  qkn_cols(a.rd, a.interleaved, c, e1, e2, rot);
  float w[2][16];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) w[t][i] = t < a.nt ? wload(a.t[t].w, a.wdt, i < 8 ? e1 + i : e2 + i - 8) : 0.f;
  const float inv_d = 1.f / (float)a.D;
  const int64_t t0 = (int64_t)blockIdx.x * p.tpw, t1 = min(t0 + p.tpw, p.tokens);
  for (int64_t tok = t0 + g; tok < t1; tok += G) {
    const int b = (int)(tok / p.smax), s = (int)(tok - (int64_t)b * p.smax);
    float cs[8], sn[8];
    if (rot) qkn_table(a, qkn_pos(a, b, s, p.smax), c, false, cs, sn);
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {  // unrolled: w[ti] / dw[ti] stay in registers
      if (ti >= a.nt) continue;
      const QkNormTensor& t = a.t[ti];
      if (s >= t.S) continue;
      // batch bb of tensor ti is batch ti * nbq + bb of the launch, which slice that % gridDim.y takes
      const int nbt = ti ? p.nb - p.nbq : p.nbq, gy = gridDim.y;
      for (int bb = ti ? (blockIdx.y + gy - p.nbq % gy) % gy : blockIdx.y; bb < nbt; bb += gy) {
        const int h0 = bb * R;
        const bf16_t* in = static_cast<const bf16_t*>(t.x) + b * t.xsb + s * t.xss;
        bf16_t* out = static_cast<bf16_t*>(t.y) + b * t.ysb + s * t.yss;
        uint4 raw[R][2];
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (h0 + r < t.H) {
            const bf16_t* row = in + (h0 + r) * t.xsh;
            raw[r][0] = *reinterpret_cast<const uint4*>(row + e1);
            raw[r][1] = *reinterpret_cast<const uint4*>(row + e2);
          }
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (h0 + r >= t.H) continue;
          float x[16];
          qkn_unpack(raw[r][0], raw[r][1], x);
          float ss = 0.f;
#pragma unroll
          for (int i = 0; i < 16; ++i) ss += x[i] * x[i];
          const float rs = rsqrtf(group_sum<LPR>(ss) * inv_d + a.eps);
          if (c == 0) t.rstd[((int64_t)b * t.S + s) * t.H + h0 + r] = rs;
#pragma unroll
          for (int i = 0; i < 16; ++i) x[i] = x[i] * rs * w[ti][i];
          if (rot) qkn_rotate(x, cs, sn, a.interleaved);
          bf16_t* row = out + (h0 + r) * t.ysh;
          store16(row + e1, x);
          store16(row + e2, x + 8);
        }
      }
    }
  }
}

// The workgroup's fold of the lanes' dw registers (threadIdx.x * 16 + i, padded to 17) into one row
// of D columns: 256 / D column sets add 16 groups each, then the sets are added in order.
template <int LPR>
__device__ __forceinline__ void qkn_fold_vec(const float* dw, float* red, float* part, float* slab_row, const QkNormArgs& a) {
  constexpr int G = QKN_BLOCK / LPR, D = 16 * LPR, NQ = QKN_BLOCK / D;
#pragma unroll
  for (int i = 0; i < 16; ++i) red[threadIdx.x * 17 + i] = dw[i];
  __syncthreads();
  const int j = threadIdx.x % D, q = threadIdx.x / D;
  const int c = j / 16, i = j % 16;
  float acc = 0.f;
  for (int g = q * (G / NQ); g < (q + 1) * (G / NQ); ++g) acc += red[(g * LPR + c) * 17 + i];
  part[q * D + j] = acc;
  __syncthreads();
  if (q == 0) {
    for (int k = 1; k < NQ; ++k) acc += part[k * D + j];
    int e1, e2;
    bool rot;
    qkn_cols(a.rd, a.interleaved, c, e1, e2, rot);
    slab_row[i < 8 ? e1 + i : e2 + i - 8] = acc;
  }
  __syncthreads();
}

template <int LPR>
__global__ __launch_bounds__(QKN_BLOCK) void qkn_bwd_vec(QkNormArgs a, QknPlan p) {
  constexpr int G = QKN_BLOCK / LPR, R = QKN_ROWS_BWD, D = 16 * LPR;
  __shared__ float red[QKN_BLOCK * 17];
  __shared__ float part[QKN_BLOCK];
  const int c = threadIdx.x % LPR, g = threadIdx.x / LPR;
  int e1, e2;
  bool rot;
  qkn_cols(a.rd, a.interleaved, c, e1, e2, rot);
  float w[2][16], dw[2][16];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      w[t][i] = t < a.nt ? wload(a.t[t].w, a.wdt, i < 8 ? e1 + i : e2 + i - 8) : 0.f;
      dw[t][i] = 0.f;
    }
  const float inv_d = 1.f / (float)a.D;
  const int64_t t0 = (int64_t)blockIdx.x * p.tpw, t1 = min(t0 + p.tpw, p.tokens);
  for (int64_t tok = t0 + g; tok < t1; tok += G) {
    const int b = (int)(tok / p.smax), s = (int)(tok - (int64_t)b * p.smax);
    float cs[8], sn[8];
    if (rot) qkn_table(a, qkn_pos(a, b, s, p.smax), c, true, cs, sn);
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {  // unrolled: w[ti] / dw[ti] stay in registers
      if (ti >= a.nt) continue;
      const QkNormTensor& t = a.t[ti];
      if (s >= t.S) continue;
      // batch bb of tensor ti is batch ti * nbq + bb of the launch, which slice that % gridDim.y takes
      const int nbt = ti ? p.nb - p.nbq : p.nbq, gy = gridDim.y;
      for (int bb = ti ? (blockIdx.y + gy - p.nbq % gy) % gy : blockIdx.y; bb < nbt; bb += gy) {
        const int h0 = bb * R;
        const bf16_t* xin = static_cast<const bf16_t*>(t.x) + b * t.xsb + s * t.xss;
        bf16_t* gio = static_cast<bf16_t*>(t.y) + b * t.ysb + s * t.yss;
        const float* rsp = t.rstd + ((int64_t)b * t.S + s) * t.H;
        uint4 xr[R][2], gr[R][2];
        float rs[R];
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (h0 + r < t.H) {
            const bf16_t* xrow = xin + (h0 + r) * t.xsh;
            const bf16_t* grow = gio + (h0 + r) * t.ysh;
            xr[r][0] = *reinterpret_cast<const uint4*>(xrow + e1);
            xr[r][1] = *reinterpret_cast<const uint4*>(xrow + e2);
            gr[r][0] = *reinterpret_cast<const uint4*>(grow + e1);
            gr[r][1] = *reinterpret_cast<const uint4*>(grow + e2);
            rs[r] = rsp[h0 + r];
          }
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (h0 + r >= t.H) continue;
          float xh[16], gv[16];
          qkn_unpack(xr[r][0], xr[r][1], xh);
          qkn_unpack(gr[r][0], gr[r][1], gv);
          if (rot) qkn_rotate(gv, cs, sn, a.interleaved);  // g = R^-1 dz
          float dot = 0.f;
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            xh[i] *= rs[r];
            dw[ti][i] += gv[i] * xh[i];
            gv[i] *= w[ti][i];
            dot += gv[i] * xh[i];
          }
          const float m = group_sum<LPR>(dot) * inv_d;
#pragma unroll
          for (int i = 0; i < 16; ++i) gv[i] = rs[r] * (gv[i] - xh[i] * m);
          bf16_t* grow = gio + (h0 + r) * t.ysh;
          store16(grow + e1, gv);
          store16(grow + e2, gv + 8);
        }
      }
    }
  }
  if (a.slab) {  // a workgroup without rows stores its zeros: the fold reads every slab row
    const int64_t group = (int64_t)blockIdx.y * gridDim.x + blockIdx.x, groups = (int64_t)gridDim.x * gridDim.y;
#pragma unroll
    for (int t = 0; t < 2; ++t)
      if (t < a.nt) qkn_fold_vec<LPR>(dw[t], red, part, a.slab + (t * groups + group) * D, a);
  }
}

// ------------------------------------------------------------------------------ general form
// pair i of a head row: the rotated pairs first, then the columns behind them two by two
__device__ __forceinline__ void qkn_pair(int rd, int inter, int i, int& e1, int& e2) {
  if (!inter && 2 * i < rd) e1 = i, e2 = i + (rd >> 1);
  else e1 = 2 * i, e2 = 2 * i + 1;
}

template <typename T, bool BWD>
__global__ __launch_bounds__(QKN_BLOCK) void qkn_gen(QkNormArgs a, QknPlan p) {
  constexpr int NP = 2;  // pairs a lane holds: D <= 256
  __shared__ float red[QKN_BLOCK / 64][256];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int np = a.D >> 1, half = a.rd >> 1;
  int e1[NP], e2[NP];
  float w[2][NP][2], dw[2][NP][2];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int i = lane + 64 * k;
    qkn_pair(a.rd, a.interleaved, i, e1[k], e2[k]);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const bool ok = i < np && t < a.nt;
      w[t][k][0] = ok ? wload(a.t[t].w, a.wdt, e1[k]) : 0.f;
      w[t][k][1] = ok ? wload(a.t[t].w, a.wdt, e2[k]) : 0.f;
      dw[t][k][0] = dw[t][k][1] = 0.f;
    }
  }
  const float inv_d = 1.f / (float)a.D;
  const int64_t t0 = (int64_t)blockIdx.x * p.tpw, t1 = min(t0 + p.tpw, p.tokens);
  for (int64_t tok = t0 + wv; tok < t1; tok += QKN_BLOCK / 64) {
    const int b = (int)(tok / p.smax), s = (int)(tok - (int64_t)b * p.smax);
    float cs[NP], sn[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int i = lane + 64 * k;
      cs[k] = 1.f, sn[k] = 0.f;  // the pairs behind the rotated part turn by nothing
      if (i < half) {
        const float* tp = a.table + ((int64_t)qkn_pos(a, b, s, p.smax) * half + i) * 2;
        cs[k] = tp[0], sn[k] = BWD ? -tp[1] : tp[1];
      }
    }
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
      if (ti >= a.nt) continue;
      const QkNormTensor& t = a.t[ti];
      if (s >= t.S) continue;
      for (int h = 0; h < t.H; ++h) {
        const T* xrow = static_cast<const T*>(t.x) + b * t.xsb + h * t.xsh + s * t.xss;
        T* yrow = static_cast<T*>(t.y) + b * t.ysb + h * t.ysh + s * t.yss;
        float* rsp = t.rstd + ((int64_t)b * t.S + s) * t.H + h;
        float x[NP][2], gv[NP][2];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
          const bool ok = lane + 64 * k < np;
          x[k][0] = ok ? Cvt<T>::to_f(xrow[e1[k]]) : 0.f;
          x[k][1] = ok ? Cvt<T>::to_f(xrow[e2[k]]) : 0.f;
          if (BWD) {
            gv[k][0] = ok ? Cvt<T>::to_f(yrow[e1[k]]) : 0.f;
            gv[k][1] = ok ? Cvt<T>::to_f(yrow[e2[k]]) : 0.f;
          }
        }
        if constexpr (!BWD) {
          float ss = 0.f;
#pragma unroll
          for (int k = 0; k < NP; ++k) ss += x[k][0] * x[k][0] + x[k][1] * x[k][1];
          const float rs = rsqrtf(wave_sum(ss) * inv_d + a.eps);
          if (lane == 0) *rsp = rs;
#pragma unroll
          for (int k = 0; k < NP; ++k) {
            if (lane + 64 * k >= np) continue;
            const float y1 = x[k][0] * rs * w[ti][k][0], y2 = x[k][1] * rs * w[ti][k][1];
            yrow[e1[k]] = Cvt<T>::from_f(y1 * cs[k] - y2 * sn[k]);
            yrow[e2[k]] = Cvt<T>::from_f(y2 * cs[k] + y1 * sn[k]);
          }
        } else {
          const float rs = *rsp;
          float dot = 0.f;
#pragma unroll
          for (int k = 0; k < NP; ++k) {
            const float g1 = gv[k][0] * cs[k] - gv[k][1] * sn[k], g2 = gv[k][1] * cs[k] + gv[k][0] * sn[k];
            x[k][0] *= rs, x[k][1] *= rs;
            dw[ti][k][0] += g1 * x[k][0], dw[ti][k][1] += g2 * x[k][1];
            gv[k][0] = g1 * w[ti][k][0], gv[k][1] = g2 * w[ti][k][1];
            dot += gv[k][0] * x[k][0] + gv[k][1] * x[k][1];
          }
          const float m = wave_sum(dot) * inv_d;
#pragma unroll
          for (int k = 0; k < NP; ++k) {
            if (lane + 64 * k >= np) continue;
            yrow[e1[k]] = Cvt<T>::from_f(rs * (gv[k][0] - x[k][0] * m));
            yrow[e2[k]] = Cvt<T>::from_f(rs * (gv[k][1] - x[k][1] * m));
          }
        }
      }
    }
  }
  if (BWD && a.slab) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (t >= a.nt) continue;
#pragma unroll
      for (int k = 0; k < NP; ++k)
        if (lane + 64 * k < np) red[wv][e1[k]] = dw[t][k][0], red[wv][e2[k]] = dw[t][k][1];
      __syncthreads();
      if ((int)threadIdx.x < a.D) {
        float acc = red[0][threadIdx.x];
        for (int v = 1; v < QKN_BLOCK / 64; ++v) acc += red[v][threadIdx.x];
        a.slab[((int64_t)t * gridDim.x + blockIdx.x) * a.D + threadIdx.x] = acc;
      }
      __syncthreads();
    }
  }
}

// ------------------------------------------------------------------------------------ launch
bool qkn_args_ok(const QkNormArgs& a, bool bwd) {
  bool ok = (a.nt == 1 || a.nt == 2) && a.B >= 0 && a.D >= 2 && a.D % 2 == 0 && a.D <= 256 && a.rd >= 0 &&
            a.rd % 2 == 0 && a.rd <= a.D && (a.dt == DT_BF16 || a.dt == DT_F32) && (a.wdt == DT_BF16 || a.wdt == DT_F32) &&
            (a.rd == 0 || (a.table && a.max_pos >= 1)) && (bwd || a.eps > 0.f);
  for (int i = 0; ok && i < a.nt; ++i) {
    const QkNormTensor& t = a.t[i];
    ok = t.x && t.y && t.w && t.rstd && t.H >= 0 && t.S >= 0 && t.xsb >= 0 && t.xsh >= 0 && t.xss >= 0 && t.ysb >= 0 &&
         t.ysh >= 0 && t.yss >= 0 && (bwd || t.x != t.y);
  }
  if (ok && a.pos && a.nt == 2) ok = a.t[0].S == a.t[1].S;  // one [B][S] id tensor for both
  return ok;
}

bool qkn_vec_ok(const QkNormArgs& a) {
  bool vec = a.dt == DT_BF16 && qkn_vec_dim(a.D) && a.rd % 16 == 0 && reinterpret_cast<uintptr_t>(a.table) % 16 == 0;
  for (int i = 0; i < a.nt; ++i) {
    const QkNormTensor& t = a.t[i];
    vec = vec && t.xsb % 8 == 0 && t.xsh % 8 == 0 && t.xss % 8 == 0 && t.ysb % 8 == 0 && t.ysh % 8 == 0 && t.yss % 8 == 0 &&
          reinterpret_cast<uintptr_t>(t.x) % 16 == 0 && reinterpret_cast<uintptr_t>(t.y) % 16 == 0;
  }
  return vec;
}

// launches the direction's kernel; returns the slab rows per weight it filled
template <bool BWD>
int qkn_launch(const QkNormArgs& a, hipStream_t st) {
  const int smax = a.nt > 1 ? std::max(a.t[0].S, a.t[1].S) : a.t[0].S;
  const int H0 = a.t[0].H, H1 = a.nt > 1 ? a.t[1].H : 0;
  const int64_t tokens = (int64_t)a.B * smax;
  if (tokens == 0 || H0 + H1 == 0) return 0;
  if (qkn_vec_ok(a)) {
    QknPlan p = qkn_plan_vec(tokens, H0, H1, a.D, BWD);
    p.smax = smax;
    const dim3 grid(p.gx, p.gy);
#define QKN_V(L)                                                                                     \
  do {                                                                                               \
    if (BWD) hipLaunchKernelGGL(qkn_bwd_vec<L>, grid, dim3(QKN_BLOCK), 0, st, a, p);                  \
    else hipLaunchKernelGGL(qkn_fwd_vec<L>, grid, dim3(QKN_BLOCK), 0, st, a, p);                      \
  } while (0)
    switch (a.D / 16) {
      case 2: QKN_V(2); break;
      case 4: QKN_V(4); break;
      case 8: QKN_V(8); break;
      default: QKN_V(16); break;
    }
#undef QKN_V
    return p.gx * p.gy;
  }
  QknPlan p = qkn_plan_gen(tokens, H0, H1);
  p.smax = smax;
  if (a.dt == DT_BF16) hipLaunchKernelGGL((qkn_gen<bf16_t, BWD>), dim3(p.gx), dim3(QKN_BLOCK), 0, st, a, p);
  else hipLaunchKernelGGL((qkn_gen<float, BWD>), dim3(p.gx), dim3(QKN_BLOCK), 0, st, a, p);
  return p.gx;
}

}  // namespace

int qk_norm_groups(int64_t tokens, int H0, int H1, int D) {
  int g = qkn_plan_gen(tokens, H0, H1).gx;
  if (qkn_vec_dim(D)) {
    const QknPlan p = qkn_plan_vec(tokens, H0, H1, D, true);
    g = std::max(g, p.gx * p.gy);
  }
  return g;
}

void qk_norm_rope_fwd(const QkNormArgs& a, hipStream_t st) {
  if (!qkn_args_ok(a, false)) {
    fprintf(stderr, "ffk::qk_norm_rope_fwd: invalid arguments (nt %d, D %d, rd %d)\n", a.nt, a.D, a.rd);
    abort();
  }
  QkNormArgs f = a;
  f.slab = nullptr;
  qkn_launch<false>(f, st);
}

void qk_norm_rope_bwd(const QkNormArgs& a, hipStream_t st) {
  if (!qkn_args_ok(a, true)) {
    fprintf(stderr, "ffk::qk_norm_rope_bwd: invalid arguments (nt %d, D %d, rd %d)\n", a.nt, a.D, a.rd);
    abort();
  }
  QkNormArgs f = a;
  const bool want = a.t[0].dw || (a.nt > 1 && a.t[1].dw);
  if (!want) f.slab = nullptr;
  const int groups = qkn_launch<true>(f, st);
  if (f.slab && groups > 0)  // slab [2][groups][D]: each weight's rows in a fixed order
    col_reduce_add2(f.slab, a.t[0].dw, a.nt > 1 ? a.t[1].dw : nullptr, groups, a.D, st);
}

}  // namespace ffk
