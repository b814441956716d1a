// RMSNorm with the residual add in front of it fused in (the pre-norm decoder's `add` + `rms_norm`):
//   s = T(x + res),   y = s * rsqrt(mean(s^2) + eps) * w          -> s, y, rstd
//   dx = r g - r^3 s mean(g s) + ds  with g = dy w,   dw += sum_rows dy s r
// s is an output (the residual stream goes on to the next block), so the forward moves exactly two
// row reads and two row writes, and the backward reads s, dy (and ds, the gradient that arrives on
// the sum) and writes dx, which is the gradient of x and of res alike.
//
// Layout. A row is cut into chunks of 64 lanes x 16 B (512 bf16 / 256 fp32 columns); a *group* of
// WPR waves owns a row at a time and wave w of the group holds chunks w, w + WPR, ... (NCH of them)
// in VGPRs from the statistics to the stores:
//   WPR = 1  one wave per row, four independent rows per 256-thread workgroup, no LDS, no barrier
//            (up to ARN_NCH chunks: 2048 bf16 / 1024 fp32 columns);
//   WPR = 4  the workgroup's four waves share the row: each reduces its chunks with the wave
//            butterfly, the four partial sums cross one double-buffered LDS slot and one barrier per
//            row, and every wave adds them in the same order (up to 8192 bf16 / 4096 fp32 columns);
//   WPR = 8  the same with a 512-thread workgroup (fp32 up to 8192 columns).
// The cut at ARN_NCH = 4 chunks per wave is from the compiled register counts (hipcc -O3, gfx950,
// -Rpass-analysis=kernel-resource-usage): at 4 chunks the bf16 backward (the row of s, the row of g,
// the dw partials, w and the raw loads) takes 212 VGPRs and no scratch, two waves a SIMD, which is
// what ARN_MAX_WAVES puts there; the forward takes 127. Twice the chunks would leave one wave a SIMD
// with nothing to cover its loads.
// Every 16-byte load of a row is issued before the first use. w is read once per wave and stays in
// registers over the wave's rows.
// dw: each wave keeps fp32 partials of its columns over its rows and stores them once, as row
// `group` of an fp32 slab [groups][d] that col_reduce_add folds in a fixed order. Groups, and which
// rows a group takes (group, group + groups, ...), follow from (rows, d, element size) alone and
// nothing is added atomically: dw has the same bits every run.
// Rows that are no multiple of 16 bytes, or operands that are not 16-byte aligned, take the
// element form: one wave per row with scalar accesses, dw by a column-owning kernel into the same slab.
#include "common.h"
#include "ops.h"

namespace ffk {

constexpr int ARN_NCH = 4;         // chunks a wave keeps in registers
constexpr int ARN_MAX_WAVES = 2048;  // waves in flight: 8 per CU; a group takes >= 4 rows

template <typename T>
__device__ __forceinline__ void unpack16(const uint4& raw, float* out) {
  constexpr int N = 16 / sizeof(T);
  const T* e = reinterpret_cast<const T*>(&raw);
#pragma unroll
  for (int i = 0; i < N; ++i) out[i] = Cvt<T>::to_f(e[i]);
}
__device__ __forceinline__ uint4 ldraw(const void* p) { return *reinterpret_cast<const uint4*>(p); }

// Sum over the row's group: the wave butterfly (every lane ends with the same bits), then for a
// shared row one LDS slot per wave and one barrier; slot `par` alternates row by row, so a wave that
// runs ahead writes the other slot and the barrier of the next row orders the reuse. One wave per
// row (WPR = 1) has no LDS and no barrier at all.
template <int WPR>
__device__ __forceinline__ float group_sum(float v, int& par) {
  v = wave_sum(v);
  if constexpr (WPR > 1) {
    __shared__ float sh[2][WPR];
    if ((threadIdx.x & 63) == 0) sh[par][threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < WPR; ++i) t += sh[par][i];
    par ^= 1;
    v = t;
  }
  return v;
}

template <typename T, int NCH, int WPR>
__global__ void __launch_bounds__(WPR == 1 ? 256 : 64 * WPR)
    arn_fwd_kernel(const T* __restrict__ x, const T* __restrict__ res, const T* __restrict__ w, T* __restrict__ s_out,
                   T* __restrict__ y, float* __restrict__ rstd, int rows, int d, float eps) {
  constexpr int V = 16 / sizeof(T);
  int par = 0;
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
  const int group = WPR == 1 ? blockIdx.x * 4 + wib : blockIdx.x;
  const int groups = WPR == 1 ? gridDim.x * 4 : gridDim.x;
  const int sub = WPR == 1 ? 0 : wib;
  int col[NCH];
  uint4 wr[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    col[c] = ((c * WPR + sub) * 64 + lane) * V;
    wr[c] = col[c] < d ? ldraw(w + col[c]) : uint4{0, 0, 0, 0};
  }
  const float inv_d = 1.f / (float)d;
  for (int row = group; row < rows; row += groups) {
    const int64_t base = (int64_t)row * d;
    uint4 xr[NCH], rr[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      if (col[c] < d) {
        xr[c] = ldraw(x + base + col[c]);
        rr[c] = ldraw(res + base + col[c]);
      }
    float sv[NCH][V];
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (col[c] < d) {
        float a[V], b[V];
        unpack16<T>(xr[c], a);
        unpack16<T>(rr[c], b);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          sv[c][j] = Cvt<T>::to_f(Cvt<T>::from_f(a[j] + b[j]));  // the statistics see the rounded sum
          ss += sv[c][j] * sv[c][j];
        }
        store16(s_out + base + col[c], sv[c]);
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) sv[c][j] = 0.f;
      }
    }
    const float r = rsqrtf(group_sum<WPR>(ss, par) * inv_d + eps);
    if (lane == 0 && sub == 0) rstd[row] = r;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      if (col[c] < d) {
        float wf[V], o[V];
        unpack16<T>(wr[c], wf);
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = sv[c][j] * r * wf[j];
        store16(y + base + col[c], o);
      }
  }
}

template <typename T, int NCH, int WPR, bool DS>
__global__ void __launch_bounds__(WPR == 1 ? 256 : 64 * WPR)
    arn_bwd_kernel(const T* __restrict__ s, const T* __restrict__ w, const float* __restrict__ rstd,
                   const T* __restrict__ dy, const T* __restrict__ ds, T* __restrict__ dx, float* __restrict__ slab,
                   int rows, int d) {
  constexpr int V = 16 / sizeof(T);
  int par = 0;
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
  const int group = WPR == 1 ? blockIdx.x * 4 + wib : blockIdx.x;
  const int groups = WPR == 1 ? gridDim.x * 4 : gridDim.x;
  const int sub = WPR == 1 ? 0 : wib;
  int col[NCH];
  uint4 wr[NCH];
  float pw[NCH][V];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    col[c] = ((c * WPR + sub) * 64 + lane) * V;
    wr[c] = col[c] < d ? ldraw(w + col[c]) : uint4{0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < V; ++j) pw[c][j] = 0.f;
  }
  const float inv_d = 1.f / (float)d;
  for (int row = group; row < rows; row += groups) {
    const int64_t base = (int64_t)row * d;
    const float r = rstd[row];
    uint4 sr[NCH], dr[NCH], ar[DS ? NCH : 1];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      if (col[c] < d) {
        sr[c] = ldraw(s + base + col[c]);
        dr[c] = ldraw(dy + base + col[c]);
        if (DS) ar[DS ? c : 0] = ldraw(ds + base + col[c]);
      }
    float sv[NCH][V], g[NCH][V];
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (col[c] < d) {
        float dv[V], wf[V];
        unpack16<T>(sr[c], sv[c]);
        unpack16<T>(dr[c], dv);
        unpack16<T>(wr[c], wf);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          pw[c][j] += dv[j] * sv[c][j] * r;
          g[c][j] = dv[j] * wf[j];
          dot += g[c][j] * sv[c][j];
        }
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) { sv[c][j] = 0.f; g[c][j] = 0.f; }
      }
    }
    const float k = r * r * r * (group_sum<WPR>(dot, par) * inv_d);
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      if (col[c] < d) {
        float o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = r * g[c][j] - k * sv[c][j];
        if (DS) {
          float a[V];
          unpack16<T>(ar[DS ? c : 0], a);
#pragma unroll
          for (int j = 0; j < V; ++j) o[j] += a[j];
        }
        store16(dx + base + col[c], o);
      }
  }
  if (slab) {  // a group without rows stores its zeros: the fold reads every slab row
    float* prow = slab + (int64_t)group * d;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      if (col[c] < d) {
#pragma unroll
        for (int j = 0; j < V; j += 4)
          *reinterpret_cast<float4*>(prow + col[c] + j) = float4{pw[c][j], pw[c][j + 1], pw[c][j + 2], pw[c][j + 3]};
      }
  }
}

// ------------------------------------------------------------------------------ element form
// Any width and alignment: one wave per row, lane l takes columns l, l + 64, ...; the sum is formed
// again in the later passes (the same bits) instead of being kept.
template <typename T>
__global__ void __launch_bounds__(256)
    arn_fwd_elem(const T* __restrict__ x, const T* __restrict__ res, const T* __restrict__ w, T* __restrict__ s_out,
                 T* __restrict__ y, float* __restrict__ rstd, int rows, int d, float eps) {
  const int lane = threadIdx.x & 63;
  const int group = blockIdx.x * 4 + (threadIdx.x >> 6), groups = gridDim.x * 4;
  for (int row = group; row < rows; row += groups) {
    const int64_t base = (int64_t)row * d;
    float ss = 0.f;
    for (int c = lane; c < d; c += 64) {
      const T st = Cvt<T>::from_f(Cvt<T>::to_f(x[base + c]) + Cvt<T>::to_f(res[base + c]));
      s_out[base + c] = st;
      const float v = Cvt<T>::to_f(st);
      ss += v * v;
    }
    const float r = rsqrtf(wave_sum(ss) / (float)d + eps);
    if (lane == 0) rstd[row] = r;
    for (int c = lane; c < d; c += 64) {
      const float v = Cvt<T>::to_f(Cvt<T>::from_f(Cvt<T>::to_f(x[base + c]) + Cvt<T>::to_f(res[base + c])));
      y[base + c] = Cvt<T>::from_f(v * r * Cvt<T>::to_f(w[c]));
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(256)
    arn_bwd_elem(const T* __restrict__ s, const T* __restrict__ w, const float* __restrict__ rstd,
                 const T* __restrict__ dy, const T* __restrict__ ds, T* __restrict__ dx, int rows, int d) {
  const int lane = threadIdx.x & 63;
  const int group = blockIdx.x * 4 + (threadIdx.x >> 6), groups = gridDim.x * 4;
  for (int row = group; row < rows; row += groups) {
    const int64_t base = (int64_t)row * d;
    const float r = rstd[row];
    float dot = 0.f;
    for (int c = lane; c < d; c += 64)
      dot += Cvt<T>::to_f(dy[base + c]) * Cvt<T>::to_f(w[c]) * Cvt<T>::to_f(s[base + c]);
    const float k = r * r * r * (wave_sum(dot) / (float)d);
    for (int c = lane; c < d; c += 64) {
      float o = r * (Cvt<T>::to_f(dy[base + c]) * Cvt<T>::to_f(w[c])) - k * Cvt<T>::to_f(s[base + c]);
      if (ds) o += Cvt<T>::to_f(ds[base + c]);
      dx[base + c] = Cvt<T>::from_f(o);
    }
  }
}

// dw partials of the element form: a thread owns a column, blockIdx.y is the group; rows group,
// group + groups, ... in that order into slab[group][column].
template <typename T>
__global__ void __launch_bounds__(256)
    arn_dw_elem(const T* __restrict__ s, const float* __restrict__ rstd, const T* __restrict__ dy,
                float* __restrict__ slab, int rows, int d) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= d) return;
  float acc = 0.f;
  for (int row = blockIdx.y; row < rows; row += gridDim.y) {
    const int64_t i = (int64_t)row * d + c;
    acc += Cvt<T>::to_f(dy[i]) * Cvt<T>::to_f(s[i]) * rstd[row];
  }
  slab[(int64_t)blockIdx.y * d + c] = acc;
}

// ------------------------------------------------------------------------------------ launch
static bool arn_a16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// waves that share a row of d columns (a function of d and the element size alone)
static int arn_wpr(int d, int esz) {
  const int n = ceil_div(d, 64 * (16 / esz));
  return n <= ARN_NCH ? 1 : (n <= 4 * ARN_NCH ? 4 : 8);
}

// Groups launched = slab rows: about four rows a group, at most ARN_MAX_WAVES waves; with one wave
// per row whole workgroups of four, and the waves past the last row store zeros.
int add_rmsnorm_groups(int rows, int d, int esz) {
  const int wpr = arn_wpr(d, esz);
  const int g = std::max(1, std::min(ceil_div(rows, 4), ARN_MAX_WAVES / wpr));
  return wpr == 1 ? 4 * ceil_div(g, 4) : g;
}

// F(NCH, WPR) is expanded with the chunk count and the sharing the width asks for
#define ARN_DISPATCH(F)                                                         \
  do {                                                                          \
    if (wpr == 1) { if (n <= 1) F(1, 1); else if (n <= 2) F(2, 1); else F(4, 1); } \
    else if (wpr == 4) { if (n <= 8) F(2, 4); else F(4, 4); }                    \
    else F(4, 8);                                                               \
  } while (0)

template <typename T>
static void arn_fwd_t(const T* x, const T* res, const T* w, T* s, T* y, float* rstd, int rows, int d, float eps,
                      hipStream_t st) {
  constexpr int V = 16 / sizeof(T);
  const int wpr = arn_wpr(d, sizeof(T)), n = ceil_div(d, 64 * V);
  const int groups = add_rmsnorm_groups(rows, d, sizeof(T));
  const bool vec = d % V == 0 && n <= 8 * ARN_NCH && arn_a16(x) && arn_a16(res) && arn_a16(w) && arn_a16(s) && arn_a16(y);
  if (!vec) {
    hipLaunchKernelGGL(arn_fwd_elem<T>, dim3(ceil_div(groups, 4)), dim3(256), 0, st, x, res, w, s, y, rstd, rows, d, eps);
    return;
  }
  const dim3 grid(wpr == 1 ? groups / 4 : groups), block(wpr == 1 ? 256 : 64 * wpr);
#define ARN_F(N, W) hipLaunchKernelGGL((arn_fwd_kernel<T, N, W>), grid, block, 0, st, x, res, w, s, y, rstd, rows, d, eps)
  ARN_DISPATCH(ARN_F);
#undef ARN_F
}

template <typename T>
static void arn_bwd_t(const T* s, const T* w, const float* rstd, const T* dy, const T* ds, T* dx, float* dw,
                      float* slab, int rows, int d, hipStream_t st) {
  constexpr int V = 16 / sizeof(T);
  const int wpr = arn_wpr(d, sizeof(T)), n = ceil_div(d, 64 * V);
  const int groups = add_rmsnorm_groups(rows, d, sizeof(T));
  float* part = dw ? slab : nullptr;
  const bool vec = d % V == 0 && n <= 8 * ARN_NCH && arn_a16(s) && arn_a16(w) && arn_a16(dy) && arn_a16(dx) &&
                   (!ds || arn_a16(ds)) && (!part || arn_a16(part));
  if (!vec) {
    hipLaunchKernelGGL(arn_bwd_elem<T>, dim3(ceil_div(groups, 4)), dim3(256), 0, st, s, w, rstd, dy, ds, dx, rows, d);
    if (part) hipLaunchKernelGGL(arn_dw_elem<T>, dim3(ceil_div(d, 256), groups), dim3(256), 0, st, s, rstd, dy, part, rows, d);
  } else {
    const dim3 grid(wpr == 1 ? groups / 4 : groups), block(wpr == 1 ? 256 : 64 * wpr);
#define ARN_B(N, W)                                                                                                   \
  do {                                                                                                                \
    if (ds) hipLaunchKernelGGL((arn_bwd_kernel<T, N, W, true>), grid, block, 0, st, s, w, rstd, dy, ds, dx, part, rows, d); \
    else hipLaunchKernelGGL((arn_bwd_kernel<T, N, W, false>), grid, block, 0, st, s, w, rstd, dy, ds, dx, part, rows, d);   \
  } while (0)
    ARN_DISPATCH(ARN_B);
#undef ARN_B
  }
  if (part) col_reduce_add(part, dw, groups, d, st);
}

void add_rmsnorm_fwd(int dt, const void* x, const void* res, const void* w, void* s, void* y, float* rstd, int rows,
                     int d, float eps, hipStream_t st) {
  if (rows == 0) return;
  if (dt == DT_BF16)
    arn_fwd_t<bf16_t>((const bf16_t*)x, (const bf16_t*)res, (const bf16_t*)w, (bf16_t*)s, (bf16_t*)y, rstd, rows, d, eps, st);
  else
    arn_fwd_t<float>((const float*)x, (const float*)res, (const float*)w, (float*)s, (float*)y, rstd, rows, d, eps, st);
}

void add_rmsnorm_bwd(int dt, const void* s, const void* w, const float* rstd, const void* dy, const void* ds, void* dx,
                     float* dw, float* slab, int rows, int d, hipStream_t st) {
  if (rows == 0) return;
  if (dt == DT_BF16)
    arn_bwd_t<bf16_t>((const bf16_t*)s, (const bf16_t*)w, rstd, (const bf16_t*)dy, (const bf16_t*)ds, (bf16_t*)dx, dw,
                      slab, rows, d, st);
  else
    arn_bwd_t<float>((const float*)s, (const float*)w, rstd, (const float*)dy, (const float*)ds, (float*)dx, dw, slab,
                     rows, d, st);
}

}  // namespace ffk
