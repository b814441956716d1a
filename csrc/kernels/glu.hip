// Gated linear units (SwiGLU / GeGLU / ReGLU / GLU): y = act(g) * u and its backward, one launch each
// (ops.h GluArgs has the definition). Memory-bound: 16 B per lane where the widths, row strides and
// base pointers allow (Guideline 13), grid-stride over a capped grid (Guideline 11), 64-bit offsets.
//
// Every operand is a [rows][F] view with its own row stride, so two tensors, the two halves of one
// packed [T][2F] buffer and views into wider buffers are the same launch. A lane owns one 16-byte
// chunk of a row (VEC) or one element (the columns past the last whole chunk of a row, or every
// column when an operand is off a 16-byte boundary: VEC = false); it walks its (row, column) items
// by a per-launch step, so the loop holds no division. Only columns < F of rows < rows are written.
// The backward recomputes act(g) and act'(g) from g (glu_act.h: one exponential / erf for both).
// No LDS, no atomics.
#include "common.h"
#include "glu_act.h"
#include "ops.h"

namespace ffk {

namespace {

constexpr int kGluBlock = 256;

// items first, first + step, ... of a [rows][w] index space as (r, c)
struct GluWalk {
  int64_t r, c, dr, dc, w;
  __device__ __forceinline__ GluWalk(int64_t first, int64_t step, int64_t w_) : w(w_) {
    r = first / w, c = first - r * w;
    dr = step / w, dc = step - dr * w;
  }
  __device__ __forceinline__ void next() {
    r += dr, c += dc;
    if (c >= w) c -= w, ++r;
  }
};

// ACT >= 0: the activation as a compile-time constant, -1: the run-time a.act
template <typename T, int ACT, bool VEC>
__global__ __launch_bounds__(kGluBlock) void glu_fwd_kernel(GluArgs a) {
  const int act = ACT >= 0 ? ACT : a.act;
  constexpr int V = 16 / sizeof(T);
  const T* __restrict__ g = static_cast<const T*>(a.g);
  const T* __restrict__ u = static_cast<const T*>(a.u);
  T* __restrict__ y = static_cast<T*>(a.y);
  const int64_t first = (int64_t)blockIdx.x * kGluBlock + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * kGluBlock;
  const int64_t nvr = VEC ? a.F / V : 0;  // whole 16-byte chunks per row
  if (VEC && nvr > 0) {
    for (GluWalk w(first, step, nvr); w.r < a.rows; w.next()) {
      const int64_t c = w.c * V;
      float gv[V], uv[V];
      load16(g + w.r * a.sg + c, gv);
      load16(u + w.r * a.su + c, uv);
#pragma unroll
      for (int j = 0; j < V; ++j) gv[j] = glu_act(act, gv[j]) * uv[j];
      store16(y + w.r * a.sy + c, gv);
    }
  }
  const int64_t c0 = nvr * V, tail = a.F - c0;
  if (tail > 0) {
    for (GluWalk w(first, step, tail); w.r < a.rows; w.next()) {
      const int64_t c = c0 + w.c;
      const float gf = Cvt<T>::to_f(g[w.r * a.sg + c]), uf = Cvt<T>::to_f(u[w.r * a.su + c]);
      y[w.r * a.sy + c] = Cvt<T>::from_f(glu_act(act, gf) * uf);
    }
  }
}

template <typename T, int ACT, bool VEC>
__global__ __launch_bounds__(kGluBlock) void glu_bwd_kernel(GluArgs a) {
  const int act = ACT >= 0 ? ACT : a.act;
  constexpr int V = 16 / sizeof(T);
  const T* __restrict__ g = static_cast<const T*>(a.g);
  const T* __restrict__ u = static_cast<const T*>(a.u);
  const T* __restrict__ dy = static_cast<const T*>(a.dy);
  T* __restrict__ dg = static_cast<T*>(a.dg);
  T* __restrict__ du = static_cast<T*>(a.du);
  const int64_t first = (int64_t)blockIdx.x * kGluBlock + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * kGluBlock;
  const int64_t nvr = VEC ? a.F / V : 0;
  if (VEC && nvr > 0) {
    for (GluWalk w(first, step, nvr); w.r < a.rows; w.next()) {
      const int64_t c = w.c * V;
      float gv[V], uv[V], dv[V];
      load16(g + w.r * a.sg + c, gv);
      load16(u + w.r * a.su + c, uv);
      load16(dy + w.r * a.sdy + c, dv);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float f, d;
        glu_act_grad(act, gv[j], f, d);
        gv[j] = dv[j] * uv[j] * d;
        uv[j] = dv[j] * f;
      }
      store16(dg + w.r * a.sdg + c, gv);
      store16(du + w.r * a.sdu + c, uv);
    }
  }
  const int64_t c0 = nvr * V, tail = a.F - c0;
  if (tail > 0) {
    for (GluWalk w(first, step, tail); w.r < a.rows; w.next()) {
      const int64_t c = c0 + w.c;
      const float gf = Cvt<T>::to_f(g[w.r * a.sg + c]), uf = Cvt<T>::to_f(u[w.r * a.su + c]);
      const float df = Cvt<T>::to_f(dy[w.r * a.sdy + c]);
      float f, d;
      glu_act_grad(act, gf, f, d);
      dg[w.r * a.sdg + c] = Cvt<T>::from_f(df * uf * d);
      du[w.r * a.sdu + c] = Cvt<T>::from_f(df * f);
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the launch's own copy of the arguments: row-contiguous operands collapse into one flat row, and
// `vec` says whether every access of the 16-byte path would be aligned
GluArgs glu_plan(const GluArgs& in, bool bwd, int V, bool& vec) {
  GluArgs a = in;
  const int64_t st[6] = {a.sg, a.su, a.sy, a.sdy, a.sdg, a.sdu};
  const void* p[6] = {a.g, a.u, a.y, a.dy, a.dg, a.du};
  bool flat = true, bases = true, strides = true;
  for (int i = 0; i < 6; ++i) {
    if (bwd ? i == 2 : i >= 3) continue;  // not an operand of this direction
    flat = flat && (a.rows == 1 || st[i] == a.F);
    bases = bases && aligned16(p[i]);
    strides = strides && st[i] % V == 0;
  }
  if (flat) {
    a.F *= a.rows;
    a.rows = 1;
  }
  vec = bases && (flat || strides);
  return a;
}

int glu_grid(const GluArgs& a, bool vec, int V, int max_blocks) {
  const int64_t nvr = vec ? a.F / V : 0;
  const int64_t items = a.rows * std::max<int64_t>(nvr, a.F - nvr * V);
  int grid = ew_grid(items, kGluBlock);
  if (max_blocks > 0) grid = std::min(grid, max_blocks);
  return grid;
}

void glu_check(const GluArgs& a, bool bwd, const char* fn) {
  bool ok = a.rows >= 0 && a.F >= 0 && a.act >= 0 && a.act < GLU_NACT && (a.dt == DT_BF16 || a.dt == DT_F32) && a.g &&
            a.u && a.sg >= 0 && a.su >= 0;
  if (bwd) ok = ok && a.dy && a.dg && a.du && a.sdy >= 0 && (a.rows <= 1 || (a.sdg >= a.F && a.sdu >= a.F));
  else ok = ok && a.y && (a.rows <= 1 || a.sy >= a.F);
  if (!ok) {
    fprintf(stderr, "ffk::%s: invalid arguments (rows %lld, F %lld, act %d, dt %d)\n", fn, (long long)a.rows,
            (long long)a.F, a.act, a.dt);
    abort();
  }
}

#define FFK_GLU_LAUNCH(KERNEL, T, VECB)                                                                \
  do {                                                                                                 \
    if (a.act == GLU_SILU)                                                                             \
      hipLaunchKernelGGL((KERNEL<T, GLU_SILU, VECB>), dim3(grid), dim3(kGluBlock), 0, st, a);          \
    else if (a.act == GLU_GELU_TANH)                                                                   \
      hipLaunchKernelGGL((KERNEL<T, GLU_GELU_TANH, VECB>), dim3(grid), dim3(kGluBlock), 0, st, a);     \
    else                                                                                               \
      hipLaunchKernelGGL((KERNEL<T, -1, VECB>), dim3(grid), dim3(kGluBlock), 0, st, a);                \
  } while (0)

template <typename T>
void glu_launch(const GluArgs& in, bool bwd, hipStream_t st, int max_blocks) {
  constexpr int V = 16 / sizeof(T);
  bool vec;
  const GluArgs a = glu_plan(in, bwd, V, vec);
  const int grid = glu_grid(a, vec, V, max_blocks);
  if (bwd) {
    if (vec) FFK_GLU_LAUNCH(glu_bwd_kernel, T, true);
    else FFK_GLU_LAUNCH(glu_bwd_kernel, T, false);
  } else {
    if (vec) FFK_GLU_LAUNCH(glu_fwd_kernel, T, true);
    else FFK_GLU_LAUNCH(glu_fwd_kernel, T, false);
  }
}

}  // namespace

void glu_fwd(const GluArgs& a, hipStream_t st, int max_blocks) {
  glu_check(a, false, "glu_fwd");
  if (a.rows == 0 || a.F == 0) return;
  if (a.dt == DT_BF16) glu_launch<bf16_t>(a, false, st, max_blocks);
  else glu_launch<float>(a, false, st, max_blocks);
}

void glu_bwd(const GluArgs& a, hipStream_t st, int max_blocks) {
  glu_check(a, true, "glu_bwd");
  if (a.rows == 0 || a.F == 0) return;
  if (a.dt == DT_BF16) glu_launch<bf16_t>(a, true, st, max_blocks);
  else glu_launch<float>(a, true, st, max_blocks);
}

}  // namespace ffk
