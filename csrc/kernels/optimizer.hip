// Fused multi-tensor optimizers over flat parameter arenas.
// All trainable weights of one dtype live in ONE contiguous fp32 master buffer (plus an optional
// bf16 compute copy), gradients in ONE fp32 buffer: a single launch updates the whole model and
// writes the bf16 copy in the same pass (no separate cast kernel).
// Semantics follow reference src/runtime/optimizer_kernel.cu (sgd_update: momentum/nesterov/
// weight-decay; adam_update with bias-corrected alpha_t computed on the host, optimizer.cc:371).
#include "common.h"
#include "ops.h"

namespace ffk {

// four updated floats -> the float4 group i of the bf16 copy, as one 8-byte store
__device__ __forceinline__ void store_bf16x4(bf16_t* wl, int64_t i, const float* wp) {
  ushort4 o;
  o.x = f2bf(wp[0]); o.y = f2bf(wp[1]); o.z = f2bf(wp[2]); o.w = f2bf(wp[3]);
  reinterpret_cast<ushort4*>(wl)[i] = o;
}

__global__ void sgd_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ v,
                           bf16_t* __restrict__ wl, int64_t n, float lr, float momentum, int nesterov, float wd,
                           float gscale, const float* __restrict__ gscale_dev) {
  if (gscale_dev) gscale *= *gscale_dev;
  const int64_t nv = n / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
    float4 wv = reinterpret_cast<float4*>(w)[i];
    float4 gv = reinterpret_cast<const float4*>(g)[i];
    float* wp = &wv.x;
    float* gp = &gv.x;
    float4 vv = make_float4(0, 0, 0, 0);
    if (momentum > 0.f) vv = reinterpret_cast<float4*>(v)[i];
    float* vp = &vv.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float gt = gp[j] * gscale + wd * wp[j];
      if (momentum > 0.f) {
        vp[j] = vp[j] * momentum + gt;
        gt = nesterov ? gt + momentum * vp[j] : vp[j];
      }
      wp[j] -= lr * gt;
    }
    reinterpret_cast<float4*>(w)[i] = wv;
    if (momentum > 0.f) reinterpret_cast<float4*>(v)[i] = vv;
    if (wl) store_bf16x4(wl, i, wp);
  }
  for (int64_t i = nv * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float gt = g[i] * gscale + wd * w[i];
    if (momentum > 0.f) {
      v[i] = v[i] * momentum + gt;
      gt = nesterov ? gt + momentum * v[i] : v[i];
    }
    w[i] -= lr * gt;
    if (wl) wl[i] = f2bf(w[i]);
  }
}

// alpha_dev: the step size read from device memory instead of the argument (a captured hipGraph
// of the whole training step replays one launch whose alpha_t changes every step)
// gscale_dev (both kernels): a device factor multiplied into gscale, the clipping coefficient
// clip_coef leaves on the device; the weight-decay term wd * w is not scaled by it
__global__ void adam_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, bf16_t* __restrict__ wl, int64_t n, float alpha_t, float b1,
                            float b2, float wd, float eps, float gscale, const float* __restrict__ alpha_dev,
                            const float* __restrict__ gscale_dev) {
  if (alpha_dev) alpha_t = *alpha_dev;
  if (gscale_dev) gscale *= *gscale_dev;
  const int64_t nv = n / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
    float4 wv = reinterpret_cast<float4*>(w)[i];
    float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float* wp = &wv.x; float* gp = &gv.x; float* mp = &mv.x; float* vp = &vv.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gt = gp[j] * gscale + wd * wp[j];
      mp[j] = b1 * mp[j] + (1.f - b1) * gt;
      vp[j] = b2 * vp[j] + (1.f - b2) * gt * gt;
      wp[j] -= alpha_t * mp[j] / (sqrtf(vp[j]) + eps);
    }
    reinterpret_cast<float4*>(w)[i] = wv;
    reinterpret_cast<float4*>(m)[i] = mv;
    reinterpret_cast<float4*>(v)[i] = vv;
    if (wl) store_bf16x4(wl, i, wp);
  }
  for (int64_t i = nv * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float gt = g[i] * gscale + wd * w[i];
    m[i] = b1 * m[i] + (1.f - b1) * gt;
    v[i] = b2 * v[i] + (1.f - b2) * gt * gt;
    w[i] -= alpha_t * m[i] / (sqrtf(v[i]) + eps);
    if (wl) wl[i] = f2bf(w[i]);
  }
}

// Row-sparse SGD for embedding tables (momentum 0, no weight decay: a row no id touched has a zero
// gradient, so skipping it is exact). Two passes, no sort: every occurrence i of row r stores i
// into mark[r] (one store wins), then only the occurrence that won applies w -= lr * g to the row
// (and refreshes its bf16 copy) — each touched row is updated exactly once whatever the
// duplicates, and clears the row's gradient (so zero_gradients can skip the table: only touched
// rows were ever non-zero). mark needs no clearing: pass 1 rewrites every row this step touches.
__global__ void sparse_rows_mark_kernel(const int64_t* __restrict__ idx, int n, int64_t rows, int* __restrict__ mark) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const int64_t r = idx[i];
    if (r >= 0 && r < rows) mark[r] = i;
  }
}
__global__ void sparse_rows_sgd_kernel(const int64_t* __restrict__ idx, int n, int64_t rows, int dim,
                                       const int* __restrict__ mark, float* __restrict__ w,
                                       float* __restrict__ g, bf16_t* __restrict__ wl, float lr) {
  // one wave per occurrence, lanes over the row's columns
  const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= n) return;
  const int64_t r = idx[i];
  if (r < 0 || r >= rows || mark[r] != i) return;
  float* wr = w + r * dim;
  float* gr = g + r * dim;
  for (int d = lane; d < dim; d += 64) {
    const float v = wr[d] - lr * gr[d];
    wr[d] = v;
    gr[d] = 0.f;
    if (wl) wl[r * dim + d] = f2bf(v);
  }
}
void sgd_sparse_rows(const int64_t* idx, int n, int64_t rows, int dim, int* mark, float* master, float* grad,
                     void* lowp, float lr, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(sparse_rows_mark_kernel, dim3((n + 255) / 256), dim3(256), 0, st, idx, n, rows, mark);
  hipLaunchKernelGGL(sparse_rows_sgd_kernel, dim3((n + 3) / 4), dim3(256), 0, st, idx, n, rows, dim, mark, master,
                     grad, (bf16_t*)lowp, lr);
}

// max_blocks > 0 caps the grid (an update overlapped with the backward on a side stream leaves CU
// slots to the compute stream's kernels; the grid-stride loops keep enough bytes in flight).
// max_blocks < 0: short-lived workgroups instead of a grid-stride sweep — each thread updates about
// -max_blocks float4 groups and exits, so the CU slots of an overlapped update are handed back to
// the compute stream every few microseconds (a 2048-block sweep held every wave slot of every CU
// for its whole ~95 us and starved the backward's small-grid kernels, ~1.4 ms/step of BERT-Large).
static int opt_grid(int64_t n, int max_blocks) {
  if (max_blocks < 0) {
    const int64_t per = 256 * (int64_t)(-max_blocks);
    return (int)std::max<int64_t>(1, std::min<int64_t>((n / 4 + per - 1) / per, 1 << 30));
  }
  const int g = ew_grid(n / 4 + 1, 256);
  return max_blocks > 0 ? std::min(g, max_blocks) : g;
}
void sgd_update(float* master, const float* grad, float* mom, void* param_lowp, int64_t n, float lr, float momentum,
                int nesterov, float wd, float gscale, hipStream_t st, int max_blocks, const float* gscale_dev) {
  if (n == 0) return;
  hipLaunchKernelGGL(sgd_kernel, dim3(opt_grid(n, max_blocks)), dim3(256), 0, st, master, grad, mom,
                     (bf16_t*)param_lowp, n, lr, momentum, nesterov, wd, gscale, gscale_dev);
}
void adam_update(float* master, const float* grad, float* m, float* v, void* param_lowp, int64_t n, float alpha_t,
                 float beta1, float beta2, float wd, float eps, float gscale, hipStream_t st, int max_blocks,
                 const float* alpha_dev, const float* gscale_dev) {
  if (n == 0) return;
  hipLaunchKernelGGL(adam_kernel, dim3(opt_grid(n, max_blocks)), dim3(256), 0, st, master, grad, m, v,
                     (bf16_t*)param_lowp, n, alpha_t, beta1, beta2, wd, eps, gscale, alpha_dev, gscale_dev);
}

// ---------------------------------------------------------------- gradient clipping by global norm
// grad_sumsq: sum of x[i]^2 over a contiguous, 16-byte aligned fp32 range into one device scalar,
// with no float atomics: the result is a pure function of the values and n (same bits every run,
// whatever the device or the launch order).
//   nv = n / 4 float4 groups; G = clamp(ceil(nv / (256 * 8)), 1, 2048) workgroups of 256 threads
//   (G = 0 when nv = 0), T = 256 * G threads, iters = ceil(nv / T).
//   pass 1: thread t takes groups t + k * T (k < iters) into four float4 accumulators (k mod 4, one
//     fma per element: the square is not rounded on its own), adds the four accumulators pairwise,
//     their four components pairwise, then block_sum<256> (6 butterfly steps in the wave, 4 adds
//     over the waves' LDS slots) -> partial[block].
//   pass 2 (one workgroup): thread t adds partial[t + 256 * j] (j < pf = ceil(G / 256)) in order,
//     block_sum<256> again; thread 0 then folds in the n % 4 tail elements and adds the result to
//     *out (accumulate) or stores it.
// Longest chain of fp32 additions any element passes through:
//   d(n) = ceil(iters / 4) + 2 + 2 + 10 + pf + 10 + 3 + 1
// (10 = 6 + 4 of one block_sum, 3 = tail, 1 = the accumulate into *out); d(2^22 + 3) = 32, and
// d = 76 for the 335 M elements of BERT-Large. The relative error of the sum is at most about
// d * 2^-24 (every term is non-negative, so there is no cancellation).
constexpr int kSumsqMaxBlocks = 2048;
static int sumsq_grid(int64_t n) {
  const int64_t nv = n / 4;
  if (nv == 0) return 0;
  return (int)std::min<int64_t>((nv + 256 * 8 - 1) / (256 * 8), kSumsqMaxBlocks);
}
int grad_sumsq_partials() { return kSumsqMaxBlocks; }

__global__ void __launch_bounds__(256) grad_sumsq_kernel(const float* __restrict__ x, int64_t nv, int64_t iters,
                                                         float* __restrict__ partial) {
  __shared__ float red[4];
  const int64_t T = (int64_t)gridDim.x * 256;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const float4* xv = reinterpret_cast<const float4*>(x);
  float4 a[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) a[u] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t k = 0; k < iters; k += 4) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {  // four 16-byte loads in flight per lane
      const int64_t i = t + (k + u) * T;
      v[u] = (k + u < iters && i < nv) ? xv[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a[u].x = fmaf(v[u].x, v[u].x, a[u].x);
      a[u].y = fmaf(v[u].y, v[u].y, a[u].y);
      a[u].z = fmaf(v[u].z, v[u].z, a[u].z);
      a[u].w = fmaf(v[u].w, v[u].w, a[u].w);
    }
  }
  float4 s;
  s.x = (a[0].x + a[1].x) + (a[2].x + a[3].x);
  s.y = (a[0].y + a[1].y) + (a[2].y + a[3].y);
  s.z = (a[0].z + a[1].z) + (a[2].z + a[3].z);
  s.w = (a[0].w + a[1].w) + (a[2].w + a[3].w);
  const float r = block_sum<256>((s.x + s.y) + (s.z + s.w), red);
  if (threadIdx.x == 0) partial[blockIdx.x] = r;
}
__global__ void __launch_bounds__(256) grad_sumsq_final_kernel(const float* __restrict__ partial, int npart,
                                                               const float* __restrict__ x, int64_t n,
                                                               float* __restrict__ out, int accumulate) {
  __shared__ float red[4];
  float s = 0.f;
  for (int j = threadIdx.x; j < npart; j += 256) s += partial[j];
  s = block_sum<256>(s, red);
  if (threadIdx.x == 0) {
    for (int64_t i = n / 4 * 4; i < n; ++i) s = fmaf(x[i], x[i], s);
    *out = accumulate ? *out + s : s;
  }
}
void grad_sumsq(const float* x, int64_t n, float* partial, float* out, int accumulate, hipStream_t st) {
  const int g = sumsq_grid(n);
  if (g > 0) {
    const int64_t nv = n / 4, T = (int64_t)g * 256;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(g), dim3(256), 0, st, x, nv, (nv + T - 1) / T, partial);
  }
  hipLaunchKernelGGL(grad_sumsq_final_kernel, dim3(1), dim3(256), 0, st, partial, g, x, n, out, accumulate);
}

// norm = sqrt(sumsq), coef = min(1, max_norm / (norm + eps)): torch's clip_grad_norm_ coefficient,
// left on the device for the update kernels' gscale_dev (no host sync; a NaN norm gives a NaN coef)
__global__ void clip_coef_kernel(const float* __restrict__ sumsq, float max_norm, float eps, float* __restrict__ norm,
                                 float* __restrict__ coef) {
  const float nr = sqrtf(*sumsq);
  const float c = max_norm / (nr + eps);
  *norm = nr;
  *coef = c < 1.f ? c : (c >= 1.f ? 1.f : c);  // NaN stays NaN (fminf would drop it)
}
void clip_coef(const float* sumsq, float max_norm, float eps, float* norm, float* coef, hipStream_t st) {
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(1), 0, st, sumsq, max_norm, eps, norm, coef);
}

// -------------------------------------------------------------------------------------------- LAMB
// (You et al., "Large Batch Optimization for Deep Learning", ICLR 2020.) Adam moments, decoupled
// weight decay and one trust ratio per logical weight:
//   g' = c g;  m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2;  u = m rc1 / (sqrt(v rc2) + eps) + lam_p w
//   r_p = |w_p| / |u_p| (1 when the weight is excluded or either norm is not > 0);  w -= lr r_p u
// The norms run over whole weights, which a flat range [lo, hi) cannot express, so the launches
// are driven by a chunk table the host builds once (kernels.lamb_table): every piece (an arena
// entry cut by an update range) is split into chunks of at most kLambChunk elements with a 16-byte
// aligned start; the padding between entries belongs to no chunk and is never touched.
//   lamb_moments (one workgroup per chunk): m, v updated, u formed, sum w^2 and sum u^2 -> partials
//   lamb_norms   (one workgroup per weight): the weight's chunk partials, in index order -> norms
//   (the caller all-reduces norms over the world)
//   lamb_apply   (one workgroup per chunk): r_p from norms, u recomputed from the stored m, v, w by
//     the same lamb_u as stage 1 (no arena-sized u buffer), w and its bf16 copy written
// No float atomics anywhere: the same input gives the same bits. hyper = {lr, rc1, rc2} on the
// device (rc = 1 / (1 - beta^t), or 1 without bias correction), gscale_dev = the clipping
// coefficient or null.
// Longest chain of fp32 additions an element's square passes through, for a weight of cc chunks:
//   lamb_moments: thread t takes float4 groups t + 256 k (k < kLambChunk / 1024 = 8) into one float4
//     accumulator (one fma per element): 8; its components pairwise: 2; one of the <= 3 tail
//     elements of the chunk: 1; block_sum<256>: 6 + 4 = 10
//   lamb_norms: thread t adds partial[first + t + 256 j] (j < ceil(cc / 256)) in order, then
//     block_sum<256>: 10
//   d(cc) = 8 + 2 + 1 + 10 + ceil(cc / 256) + 10 = 31 + ceil(cc / 256)
// (d = 32 up to 2 M elements; the 31 M-element embedding table of BERT-Large: cc = 3816, d = 46.)
// Every term is non-negative, so the relative error of a sum is at most about d * 2^-24.
constexpr int kLambChunk = 8192;
int lamb_chunk() { return kLambChunk; }

struct LambChunk {  // 16 bytes, as kernels.lamb_table packs them
  int64_t start;    // first element, a multiple of 4
  int len;          // 1 .. kLambChunk
  int weight;       // row of the weight table
};
struct LambWeight {  // 16 bytes
  float lambda;      // decoupled weight decay of this weight (0 when excluded)
  int flags;         // bit 0: adapt (trust ratio applies); bit 1: this table owns the row
  int first, count;  // the weight's chunks are [first, first + count) of this table
};

__device__ __forceinline__ float lamb_u(float m, float v, float w, float rc1, float rc2, float eps, float lambda) {
  return fmaf(lambda, w, (m * rc1) / (sqrtf(v * rc2) + eps));
}

// a chunk the table's builder would not have produced is skipped, never followed out of bounds
__device__ __forceinline__ bool lamb_chunk_ok(const LambChunk& c, int64_t n, int n_weights) {
  return c.start >= 0 && (c.start & 3) == 0 && c.len > 0 && c.len <= kLambChunk && c.start + c.len <= n &&
         c.weight >= 0 && c.weight < n_weights;
}

// the Adam moments of one element from its (scaled) gradient; c = 1 - b (one_minus)
__device__ __forceinline__ void adam_moments(float& m, float& v, float gt, float b1, float c1, float b2, float c2) {
  m = fmaf(b1, m, c1 * gt);
  v = fmaf(b2, v, c2 * gt * gt);
}

// One workgroup of 256 threads over one chunk: body4(i) for each float4 group i of the chunk
// (counted from c.start, which is 16-byte aligned), between() once in every thread, then tail(t)
// for each of the chunk's len % 4 last elements (t an index into the arena). The callers' lambdas
// capture by value where they can: by reference the compiler orders the address arithmetic and
// the loads differently (same results, other instructions).
template <class Body4, class Between, class Tail>
__device__ __forceinline__ void walk_chunk(const LambChunk& c, Body4 body4, Between between, Tail tail) {
  const int nv = c.len >> 2;
#pragma unroll 2
  for (int i = threadIdx.x; i < nv; i += 256) body4(i);
  between();
  const int64_t t = c.start + (nv << 2) + threadIdx.x;
  if ((int)threadIdx.x < (c.len & 3)) tail(t);
}

__global__ void __launch_bounds__(256)
lamb_moments_kernel(const float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                    float* __restrict__ v, int64_t n, const LambChunk* __restrict__ chunks,
                    const LambWeight* __restrict__ wtab, int n_weights, const float* __restrict__ hyper,
                    const float* __restrict__ gscale_dev, float b1, float c1, float b2, float c2, float eps,
                    float* __restrict__ partial) {
  __shared__ float red_w[4], red_u[4];
  const LambChunk c = chunks[blockIdx.x];
  const bool ok = lamb_chunk_ok(c, n, n_weights);  // uniform over the workgroup
  float4 aw = make_float4(0.f, 0.f, 0.f, 0.f), au = aw;
  float sw = 0.f, su = 0.f;
  if (ok) {
    const float gs = gscale_dev ? *gscale_dev : 1.f;
    const float rc1 = hyper[1], rc2 = hyper[2];
    const float lambda = wtab[c.weight].lambda;
    const float4* wv4 = reinterpret_cast<const float4*>(w + c.start);
    const float4* gv4 = reinterpret_cast<const float4*>(g + c.start);
    float4* mv4 = reinterpret_cast<float4*>(m + c.start);
    float4* vv4 = reinterpret_cast<float4*>(v + c.start);
    walk_chunk(c, [&](int i) {
      const float4 wv = wv4[i];
      const float4 gv = gv4[i];
      float4 mv = mv4[i];
      float4 vv = vv4[i];
      const float* wp = &wv.x; const float* gp = &gv.x;
      float* mp = &mv.x; float* vp = &vv.x; float* awp = &aw.x; float* aup = &au.x;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        adam_moments(mp[j], vp[j], gp[j] * gs, b1, c1, b2, c2);
        const float u = lamb_u(mp[j], vp[j], wp[j], rc1, rc2, eps, lambda);
        awp[j] = fmaf(wp[j], wp[j], awp[j]);
        aup[j] = fmaf(u, u, aup[j]);
      }
      mv4[i] = mv;
      vv4[i] = vv;
    }, [&] {  // the tail element is added to the sum of the accumulators
      sw = (aw.x + aw.y) + (aw.z + aw.w);
      su = (au.x + au.y) + (au.z + au.w);
    }, [=, &sw, &su](int64_t t) {
      float mt = m[t], vt = v[t];
      adam_moments(mt, vt, g[t] * gs, b1, c1, b2, c2);
      const float wt = w[t];
      const float u = lamb_u(mt, vt, wt, rc1, rc2, eps, lambda);
      m[t] = mt;
      v[t] = vt;
      sw = fmaf(wt, wt, sw);
      su = fmaf(u, u, su);
    });
  }
  sw = block_sum<256>(sw, red_w);
  su = block_sum<256>(su, red_u);
  if (threadIdx.x == 0) {
    partial[2 * (int64_t)blockIdx.x] = sw;
    partial[2 * (int64_t)blockIdx.x + 1] = su;
  }
}

// count = 0: this rank must not count the arena (a replica another rank counts): zeros
__global__ void __launch_bounds__(256)
lamb_norms_kernel(const float* __restrict__ partial, int n_chunks, const LambWeight* __restrict__ wtab, int count,
                  float* __restrict__ norms) {
  __shared__ float red_w[4], red_u[4];
  const LambWeight e = wtab[blockIdx.x];
  if (!(e.flags & 2)) return;  // another arena's weight (uniform over the workgroup)
  float sw = 0.f, su = 0.f;
  if (count && e.first >= 0 && e.count > 0 && e.first <= n_chunks - e.count) {
    for (int j = threadIdx.x; j < e.count; j += 256) {
      sw += partial[2 * (int64_t)(e.first + j)];
      su += partial[2 * (int64_t)(e.first + j) + 1];
    }
  }
  sw = block_sum<256>(sw, red_w);
  su = block_sum<256>(su, red_u);
  if (threadIdx.x == 0) {
    norms[2 * blockIdx.x] = sw;
    norms[2 * blockIdx.x + 1] = su;
  }
}

__global__ void __launch_bounds__(256)
lamb_apply_kernel(float* __restrict__ w, const float* __restrict__ m, const float* __restrict__ v,
                  bf16_t* __restrict__ wl, int64_t n, const LambChunk* __restrict__ chunks,
                  const LambWeight* __restrict__ wtab, int n_weights, const float* __restrict__ hyper, float eps,
                  const float* __restrict__ norms) {
  const LambChunk c = chunks[blockIdx.x];
  if (!lamb_chunk_ok(c, n, n_weights)) return;
  const LambWeight e = wtab[c.weight];
  const float rc1 = hyper[1], rc2 = hyper[2];
  const float wn = sqrtf(norms[2 * c.weight]), un = sqrtf(norms[2 * c.weight + 1]);
  const float step = hyper[0] * (((e.flags & 1) && wn > 0.f && un > 0.f) ? wn / un : 1.f);
  float4* wv4 = reinterpret_cast<float4*>(w + c.start);
  const float4* mv4 = reinterpret_cast<const float4*>(m + c.start);
  const float4* vv4 = reinterpret_cast<const float4*>(v + c.start);
  walk_chunk(c, [=](int i) {
    float4 wv = wv4[i];
    const float4 mv = mv4[i];
    const float4 vv = vv4[i];
    float* wp = &wv.x; const float* mp = &mv.x; const float* vp = &vv.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) wp[j] -= step * lamb_u(mp[j], vp[j], wp[j], rc1, rc2, eps, e.lambda);
    wv4[i] = wv;
    if (wl) store_bf16x4(wl + c.start, i, wp);
  }, [] {}, [=](int64_t t) {
    const float wt = w[t] - step * lamb_u(m[t], v[t], w[t], rc1, rc2, eps, e.lambda);
    w[t] = wt;
    if (wl) wl[t] = f2bf(wt);
  });
}

// ------------------------------------------------------------------------------------------- AdamW
// (Loshchilov & Hutter, "Decoupled Weight Decay Regularization", ICLR 2019.) LAMB with a trust ratio
// of 1, in one pass: the moments as lamb_moments forms them, u by the same lamb_u, w -= lr u and
// the bf16 copy, over the chunks [c0, c1) of a LAMB chunk table. lambda is per weight (the table's
// row), so biases and norm gains can go undecayed; the padding between entries is in no chunk.
// No reduction, no LDS, no atomics: the same input gives the same bits. One workgroup per chunk
// (at most kLambChunk elements, 8 float4 groups per thread): the short-lived workgroups the
// overlapped update wants (opt_grid, max_blocks < 0); a capped grid strides over the chunks.
__global__ void __launch_bounds__(256)
adamw_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
             bf16_t* __restrict__ wl, int64_t n, const LambChunk* __restrict__ chunks, int c0, int c1,
             const LambWeight* __restrict__ wtab, int n_weights, const float* __restrict__ hyper,
             const float* __restrict__ gscale_dev, float b1, float c1m, float b2, float c2m, float eps) {
  const float gs = gscale_dev ? *gscale_dev : 1.f;
  const float lr = hyper[0], rc1 = hyper[1], rc2 = hyper[2];
  for (int ci = c0 + (int)blockIdx.x; ci < c1; ci += (int)gridDim.x) {
    const LambChunk c = chunks[ci];
    if (!lamb_chunk_ok(c, n, n_weights)) continue;  // uniform over the workgroup
    const float lambda = wtab[c.weight].lambda;
    float4* wv4 = reinterpret_cast<float4*>(w + c.start);
    const float4* gv4 = reinterpret_cast<const float4*>(g + c.start);
    float4* mv4 = reinterpret_cast<float4*>(m + c.start);
    float4* vv4 = reinterpret_cast<float4*>(v + c.start);
    walk_chunk(c, [=](int i) {
      float4 wv = wv4[i];
      const float4 gv = gv4[i];
      float4 mv = mv4[i];
      float4 vv = vv4[i];
      float* wp = &wv.x; const float* gp = &gv.x; float* mp = &mv.x; float* vp = &vv.x;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        adam_moments(mp[j], vp[j], gp[j] * gs, b1, c1m, b2, c2m);
        wp[j] -= lr * lamb_u(mp[j], vp[j], wp[j], rc1, rc2, eps, lambda);
      }
      wv4[i] = wv;
      mv4[i] = mv;
      vv4[i] = vv;
      if (wl) store_bf16x4(wl + c.start, i, wp);
    }, [] {}, [=](int64_t t) {
      float mt = m[t], vt = v[t];
      adam_moments(mt, vt, g[t] * gs, b1, c1m, b2, c2m);
      const float wt = w[t] - lr * lamb_u(mt, vt, w[t], rc1, rc2, eps, lambda);
      m[t] = mt;
      v[t] = vt;
      w[t] = wt;
      if (wl) wl[t] = f2bf(wt);
    });
  }
}

// 1 - beta as the moment kernels take it: rounded once from double (1.f - 0.999f is 4.7e-5 off 0.001)
static float one_minus(double beta) { return (float)(1.0 - beta); }

void adamw_update(float* master, const float* grad, float* m, float* v, void* param_lowp, int64_t n,
                  const void* chunks, int c0, int c1, const void* wtab, int n_weights, const float* hyper,
                  const float* gscale_dev, double beta1, double beta2, float eps, hipStream_t st, int max_blocks) {
  if (c1 <= c0) return;
  const int grid = max_blocks > 0 ? std::min(c1 - c0, max_blocks) : c1 - c0;
  hipLaunchKernelGGL(adamw_kernel, dim3(grid), dim3(256), 0, st, master, grad, m, v, (bf16_t*)param_lowp, n,
                     (const LambChunk*)chunks, c0, c1, (const LambWeight*)wtab, n_weights, hyper, gscale_dev,
                     (float)beta1, one_minus(beta1), (float)beta2, one_minus(beta2), eps);
}

void lamb_moments(const float* master, const float* grad, float* m, float* v, int64_t n, const void* chunks,
                  int n_chunks, const void* wtab, int n_weights, const float* hyper, const float* gscale_dev,
                  double beta1, double beta2, float eps, float* partial, hipStream_t st) {
  if (n_chunks <= 0) return;
  hipLaunchKernelGGL(lamb_moments_kernel, dim3(n_chunks), dim3(256), 0, st, master, grad, m, v, n,
                     (const LambChunk*)chunks, (const LambWeight*)wtab, n_weights, hyper, gscale_dev, (float)beta1,
                     one_minus(beta1), (float)beta2, one_minus(beta2), eps, partial);
}
void lamb_norms(const float* partial, int n_chunks, const void* wtab, int n_weights, int count, float* norms,
                hipStream_t st) {
  if (n_weights <= 0) return;
  hipLaunchKernelGGL(lamb_norms_kernel, dim3(n_weights), dim3(256), 0, st, partial, n_chunks,
                     (const LambWeight*)wtab, count, norms);
}
void lamb_apply(float* master, const float* m, const float* v, void* param_lowp, int64_t n, const void* chunks,
                int n_chunks, const void* wtab, int n_weights, const float* hyper, float eps, const float* norms,
                hipStream_t st) {
  if (n_chunks <= 0) return;
  hipLaunchKernelGGL(lamb_apply_kernel, dim3(n_chunks), dim3(256), 0, st, master, m, v, (bf16_t*)param_lowp, n,
                     (const LambChunk*)chunks, (const LambWeight*)wtab, n_weights, hyper, eps, norms);
}

}  // namespace ffk
