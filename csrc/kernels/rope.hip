// Rotary position embedding (RoPE): one memory-bound pass that rotates the projected Q and K heads by
// their positions, in place or out of place, forward or inverse (ops.h RopeArgs has the definition).
//
// No trigonometry on the device: per-element sinf / cosf would make the pass VALU-bound (kernel guide,
// appendix B 'Element-wise'), so (cos, sin) come from a host-built fp32 table [max_pos][rd/2][2] that
// stays in L2. A lane owns one 16-byte chunk of a token's rotated columns (8 bf16 / 4 fp32; two
// chunks, i and i + rd/2, in the half-split pairing), fetches that token's cos / sin once and keeps
// them in registers across kRopeRows of the token's H + Hkv head rows (blockIdx.y picks which): all of
// those rows' loads are issued before the first store, so up to 16 x 16 B are in flight per lane. Rows
// whose extents or alignment do not fit 16-byte accesses take the element-pair kernel, one lane per
// (token, pair). Neither uses LDS; the tail (tokens x chunks past a multiple of the block, head rows
// past a multiple of kRopeRows, rows of the shorter tensor) is bounds-checked, not padded.
#include "common.h"
#include "ops.h"

namespace ffk {

namespace {

constexpr int kRopeBlock = 256;
constexpr int kRopeRows = 8;  // head rows per lane: one table fetch serves them all

template <typename T>
__device__ __forceinline__ void unpack16(const uint4& raw, float* out) {
  constexpr int N = 16 / sizeof(T);
  const T* e = reinterpret_cast<const T*>(&raw);
#pragma unroll
  for (int i = 0; i < N; ++i) out[i] = Cvt<T>::to_f(e[i]);
}
template <typename T>
__device__ __forceinline__ uint4 pack16(const float* in) {
  constexpr int N = 16 / sizeof(T);
  uint4 raw;
  T* e = reinterpret_cast<T*>(&raw);
#pragma unroll
  for (int i = 0; i < N; ++i) e[i] = Cvt<T>::from_f(in[i]);
  return raw;
}

// the position of row s of sample b, clamped into the table
__device__ __forceinline__ int rope_pos(const RopeArgs& a, int b, int s, int smax) {
  const int p = a.pos ? a.pos[(int64_t)b * smax + s] : s;
  return min(max(p, 0), a.max_pos - 1);
}

// head row j of the launch (the first tensor's heads, then the second's) for token (b, s): its buffers,
// its element offset, and whether the row exists for this token
struct RopeRow {
  const void* in;
  void* out;
  int64_t off;
  bool ok;
};
__device__ __forceinline__ RopeRow rope_row_of(const RopeArgs& a, int j, int b, int s) {
  const int H0 = a.t[0].H;
  const int nrows = H0 + (a.nt > 1 ? a.t[1].H : 0);
  const bool second = j >= H0;  // uniform over the block
  const int h = second ? j - H0 : j;
  RopeRow r;
  r.in = second ? a.t[1].in : a.t[0].in;
  r.out = second ? a.t[1].out : a.t[0].out;
  const int64_t sb = second ? a.t[1].sb : a.t[0].sb, sh = second ? a.t[1].sh : a.t[0].sh,
                ss = second ? a.t[1].ss : a.t[0].ss;
  r.ok = j < nrows && s < (second ? a.t[1].S : a.t[0].S);
  r.off = b * sb + h * sh + s * ss;
  return r;
}

// 16-byte path. lpr: lanes per token (chunks of its rotated columns); total = B * smax * lpr.
template <typename T, bool INTER>
__global__ __launch_bounds__(kRopeBlock) void rope_vec_kernel(RopeArgs a, int lpr, int smax, int64_t total) {
  constexpr int V = 16 / sizeof(T);
  constexpr int NP = INTER ? V / 2 : V;  // pairs per lane
  constexpr int NL = INTER ? 1 : 2;      // 16-byte chunks per lane and row
  const int64_t idx = (int64_t)blockIdx.x * kRopeBlock + threadIdx.x;
  if (idx >= total) return;
  const int64_t tok = idx / lpr;
  const int c = (int)(idx - tok * lpr);
  const int b = (int)(tok / smax), s = (int)(tok - (int64_t)b * smax);
  const int half = a.rd >> 1;
  const int p = rope_pos(a, b, s, smax);
  float cs[NP], sn[NP];
  {
    const float4* tp = reinterpret_cast<const float4*>(a.table + ((int64_t)p * half + (int64_t)c * NP) * 2);
#pragma unroll
    for (int k = 0; k < NP / 2; ++k) {
      const float4 t = tp[k];
      cs[2 * k] = t.x, cs[2 * k + 1] = t.z;
      sn[2 * k] = a.inverse ? -t.y : t.y, sn[2 * k + 1] = a.inverse ? -t.w : t.w;
    }
  }
  const int j0 = blockIdx.y * kRopeRows;
  const int e1 = c * V, e2 = half + c * V;  // the lane's chunks (e2: half-split only)
  RopeRow row[kRopeRows];
  uint4 raw[kRopeRows][NL];
#pragma unroll
  for (int r = 0; r < kRopeRows; ++r) {
    row[r] = rope_row_of(a, j0 + r, b, s);
    if (row[r].ok) {
      const T* in = static_cast<const T*>(row[r].in) + row[r].off;
      raw[r][0] = *reinterpret_cast<const uint4*>(in + e1);
      if (NL == 2) raw[r][NL - 1] = *reinterpret_cast<const uint4*>(in + e2);
    }
  }
#pragma unroll
  for (int r = 0; r < kRopeRows; ++r) {
    if (!row[r].ok) continue;
    T* out = static_cast<T*>(row[r].out) + row[r].off;
    if constexpr (INTER) {
      float x[V], y[V];
      unpack16<T>(raw[r][0], x);
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        y[2 * k] = x[2 * k] * cs[k] - x[2 * k + 1] * sn[k];
        y[2 * k + 1] = x[2 * k + 1] * cs[k] + x[2 * k] * sn[k];
      }
      *reinterpret_cast<uint4*>(out + e1) = pack16<T>(y);
    } else {
      float x1[V], x2[V], y1[V], y2[V];
      unpack16<T>(raw[r][0], x1);
      unpack16<T>(raw[r][NL - 1], x2);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        y1[k] = x1[k] * cs[k] - x2[k] * sn[k];
        y2[k] = x2[k] * cs[k] + x1[k] * sn[k];
      }
      *reinterpret_cast<uint4*>(out + e1) = pack16<T>(y1);
      *reinterpret_cast<uint4*>(out + e2) = pack16<T>(y2);
    }
    const T* in = static_cast<const T*>(row[r].in) + row[r].off;
    if (in != out && a.rd < a.D) {  // out of place: the columns behind the rotated ones, bit for bit
      if ((a.D - a.rd) % V == 0) {
        for (int e = a.rd + c * V; e < a.D; e += lpr * V)
          *reinterpret_cast<uint4*>(out + e) = *reinterpret_cast<const uint4*>(in + e);
      } else {
        for (int e = a.rd + c; e < a.D; e += lpr) out[e] = in[e];
      }
    }
  }
}

// element-pair path: one lane per (token, pair); total = B * smax * (rd / 2)
template <typename T, bool INTER>
__global__ __launch_bounds__(kRopeBlock) void rope_pair_kernel(RopeArgs a, int smax, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * kRopeBlock + threadIdx.x;
  if (idx >= total) return;
  const int half = a.rd >> 1;
  const int64_t tok = idx / half;
  const int i = (int)(idx - tok * half);
  const int b = (int)(tok / smax), s = (int)(tok - (int64_t)b * smax);
  const int p = rope_pos(a, b, s, smax);
  const float* tp = a.table + ((int64_t)p * half + i) * 2;
  const float cs = tp[0], sn = a.inverse ? -tp[1] : tp[1];
  const int j0 = blockIdx.y * kRopeRows;
  const int e1 = INTER ? 2 * i : i, e2 = INTER ? 2 * i + 1 : i + half;
  RopeRow row[kRopeRows];
  T r1[kRopeRows], r2[kRopeRows];
#pragma unroll
  for (int r = 0; r < kRopeRows; ++r) {
    row[r] = rope_row_of(a, j0 + r, b, s);
    if (row[r].ok) {
      const T* in = static_cast<const T*>(row[r].in) + row[r].off;
      r1[r] = in[e1], r2[r] = in[e2];
    }
  }
#pragma unroll
  for (int r = 0; r < kRopeRows; ++r) {
    if (!row[r].ok) continue;
    const T* in = static_cast<const T*>(row[r].in) + row[r].off;
    T* out = static_cast<T*>(row[r].out) + row[r].off;
    const float x1 = Cvt<T>::to_f(r1[r]), x2 = Cvt<T>::to_f(r2[r]);
    out[e1] = Cvt<T>::from_f(x1 * cs - x2 * sn);
    out[e2] = Cvt<T>::from_f(x2 * cs + x1 * sn);
    if (in != out)
      for (int e = a.rd + i; e < a.D; e += half) out[e] = in[e];
  }
}

template <typename T>
void rope_launch(const RopeArgs& a, hipStream_t st) {
  constexpr int V = 16 / sizeof(T);
  const int half = a.rd / 2;
  const int smax = a.nt > 1 ? std::max(a.t[0].S, a.t[1].S) : a.t[0].S;
  const int nrows = a.t[0].H + (a.nt > 1 ? a.t[1].H : 0);
  if ((int64_t)a.B * smax * nrows == 0) return;
  bool vec = (a.interleaved ? a.rd : half) % V == 0;
  for (int i = 0; i < a.nt; ++i) {
    const RopeTensor& t = a.t[i];
    vec = vec && t.sb % V == 0 && t.sh % V == 0 && t.ss % V == 0 &&
          reinterpret_cast<uintptr_t>(t.in) % 16 == 0 && reinterpret_cast<uintptr_t>(t.out) % 16 == 0;
  }
  const int lpr = vec ? (a.interleaved ? a.rd : half) / V : half;
  const int64_t total = (int64_t)a.B * smax * lpr;
  const dim3 grid((unsigned)ceil_div64(total, kRopeBlock), (unsigned)ceil_div(nrows, kRopeRows));
  if (vec) {
    if (a.interleaved)
      hipLaunchKernelGGL((rope_vec_kernel<T, true>), grid, dim3(kRopeBlock), 0, st, a, lpr, smax, total);
    else
      hipLaunchKernelGGL((rope_vec_kernel<T, false>), grid, dim3(kRopeBlock), 0, st, a, lpr, smax, total);
  } else {
    if (a.interleaved)
      hipLaunchKernelGGL((rope_pair_kernel<T, true>), grid, dim3(kRopeBlock), 0, st, a, smax, total);
    else
      hipLaunchKernelGGL((rope_pair_kernel<T, false>), grid, dim3(kRopeBlock), 0, st, a, smax, total);
  }
}

}  // namespace

void rope(const RopeArgs& a, hipStream_t st) {
  bool ok = (a.nt == 1 || a.nt == 2) && a.B >= 0 && a.rd >= 2 && a.rd % 2 == 0 && a.rd <= a.D && a.table &&
            a.max_pos >= 1 && (a.dt == DT_BF16 || a.dt == DT_F32);
  for (int i = 0; ok && i < a.nt; ++i)
    ok = a.t[i].in && a.t[i].out && a.t[i].H >= 0 && a.t[i].S >= 0 && a.t[i].sb >= 0 && a.t[i].sh >= 0 &&
         a.t[i].ss >= 0;
  if (ok && a.pos && a.nt == 2) ok = a.t[0].S == a.t[1].S;  // one [B][S] id tensor for both
  if (!ok) {
    fprintf(stderr, "ffk::rope: invalid arguments (nt %d, D %d, rd %d, max_pos %d)\n", a.nt, a.D, a.rd, a.max_pos);
    abort();
  }
  if (a.dt == DT_BF16) rope_launch<bf16_t>(a, st);
  else rope_launch<float>(a, st);
}

}  // namespace ffk
