#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ffk {

// Strided [B][H][S][D] views (element strides; D is contiguous). All pointers bf16.
struct AttnArgs {
  const uint16_t* q = nullptr; int64_t q_sb = 0, q_sh = 0, q_ss = 0;
  const uint16_t* k = nullptr; int64_t k_sb = 0, k_sh = 0, k_ss = 0;
  const uint16_t* v = nullptr; int64_t v_sb = 0, v_sh = 0, v_ss = 0;
  uint16_t* o = nullptr; int64_t o_sb = 0, o_sh = 0, o_ss = 0;
  float* lse = nullptr;  // [B*H][Sq]
  // backward
  const uint16_t* dout = nullptr; int64_t do_sb = 0, do_sh = 0, do_ss = 0;
  uint16_t* dq = nullptr; int64_t dq_sb = 0, dq_sh = 0, dq_ss = 0;
  uint16_t* dk = nullptr; int64_t dk_sb = 0, dk_sh = 0, dk_ss = 0;
  uint16_t* dv = nullptr; int64_t dv_sb = 0, dv_sh = 0, dv_ss = 0;
  float* dq_acc = nullptr;  // [ceil(Sk/128)][B*H][Sq][D] partials
  float* delta = nullptr;   // [B*H][Sq]
  float* lse2 = nullptr;    // [B*H][Sq] lse * log2(e) (attn_bwd_pre_kernel)
  // fused bias gradient of the [B,S,3,H,D] QKV projection: dbias [3][H][D] += column sums of dq /
  // dk / dv (attn_bwd1b_kernel partials in dbp, folded by attn_bias_fold_kernel); attn_bwd returns
  // whether it did, else the caller sums the bias gradient itself
  float* dbp = nullptr;
  float* dbias = nullptr;
  int B = 0, H = 0, Sq = 0, Sk = 0, D = 64;
  float scale = 1.f;
  int causal = 0;
  float rescale_thr = 8.f;  // forward: deferred-max threshold, log2 units (attn_set_rescale_thr)
  int stagger = 0;  // backward (attn_bwd1b_kernel): waves 4-7 run each dQ chunk after the softmax
  // per-sample key lengths [B] (device int32) of a right-padded batch, or null: key j of sample b
  // takes part iff j < clamp(key_lens[b], 0, Sk). Read on the device only; selects the MASK = true
  // instantiations, which bound their mask tests and tile / key-block loops by it (memory bounds
  // stay on Sk). A sample of length 0 gives o = 0, lse = +inf and zero gradients.
  const int* key_lens = nullptr;
  // attention dropout (attn_dropout.h): drop_thr = round(256 p) > 0 selects the DROP = true
  // instantiations of attn_fwd_kernel / attn_bwd_kernel (always MASK = true; attn_fwd2_kernel and
  // attn_bwd1b_kernel have none, so attn_bwd then leaves the fused bias gradient to the caller).
  // rng_step is a one-element device counter read by the kernels (one scalar load per workgroup), so
  // a captured step draws a new mask at every replay; rng_seed has seed and layer id folded in;
  // drop_scale = 1 / (1 - drop_thr / 256); b0 / h0 are the shard's first global batch / head index
  // and H_total the global head count. lse is that of the undropped softmax.
  const int64_t* rng_step = nullptr;
  uint64_t rng_seed = 0;
  uint32_t drop_thr = 0;
  float drop_scale = 1.f;
  int b0 = 0, h0 = 0, H_total = 0;
  // score bias, fp32 [Bb][Hb][Sq][Sk] (rows contiguous: row stride Sk), or null: scores are
  // s = scale q.k + sbias[b][h][q][k] in the forward and in the backward's recompute of P. sbias_sb /
  // sbias_sh are element strides over batch and head, 0 = broadcast. Selects the BIAS = true
  // instantiations of attn_fwd_kernel / attn_bwd_kernel (always MASK = true; attn_fwd2_kernel and
  // attn_bwd1b_kernel have none, so attn_bwd then leaves the fused bias gradient to the caller).
  // An element of -inf, or one so negative that sbias * log2(e) overflows fp32 (finfo.min masks),
  // removes that key; a query row with no key left gives o = 0, lse = +inf and zero gradients. +inf
  // and NaN are the caller's problem. The score bias takes no gradient.
  const float* sbias = nullptr;
  int64_t sbias_sb = 0, sbias_sh = 0;
  // packed sequences: the run [seg_lo[b][i], seg_hi[b][i]) that position i of row b belongs to,
  // int32 [B][S] each as attn_seg_bounds writes them (both non-decreasing along a row, an empty run
  // anchored at i for padding), or null. Query i sees key j iff j lies in i's run; the relation is
  // symmetric, so it needs Sq == Sk. Selects the SEG = true instantiations of attn_fwd_kernel /
  // attn_bwd_kernel (always MASK = true, never with sbias or key_lens; attn_fwd2_kernel and
  // attn_bwd1b_kernel have none, so attn_bwd then leaves the fused bias gradient to the caller).
  // They bound their mask tests and tile loops by the runs; memory bounds stay on Sq / Sk. A padding
  // position gives o = 0, lse = +inf and zero dq / dk / dv rows.
  //
  // The kernels know no segments, only row intervals: query i sees the keys [seg_lo[b][i],
  // seg_hi[b][i]) and key j is seen by the queries [seg_klo[b][j], seg_khi[b][j]). The contract:
  //  * all four arrays are int32 [B][S] and non-decreasing along a row;
  //  * the key side is the transpose of the query side: j in [lo[i], hi[i]) <=> i in [klo[j], khi[j]);
  //  * an empty interval is anchored at its own index (lo[i] = hi[i] = i, klo[j] = khi[j] = j).
  // seg_klo / seg_khi null (both) means the query-side arrays: a symmetric relation, which runs are.
  // Half a pair, or a key side without the query side, is an error: attn_bwd launches nothing.
  // A sliding window (attn_band_bounds: the band [i - left, i + right], alone or cut to the runs) is
  // such a family with a key side of its own, [j - right, j + left]. The forward reads the query side
  // only; the backward takes a lane's mask test from the key side and its query-tile ranges and dQ
  // chains from the query side. The causal bound is applied on top by both.
  const int* seg_lo = nullptr;
  const int* seg_hi = nullptr;
  const int* seg_klo = nullptr;
  const int* seg_khi = nullptr;
  // grouped-query / multi-query attention: Hkv key / value heads under H query heads, query head h
  // reading KV head h / G with G = H / Hkv (torch's enable_gqa, repeat_interleave(G) over heads). 0 or
  // H: every head has its own K / V, what the kernels did before. With 0 < Hkv < H the strides k_s*,
  // v_s*, dk_s*, dv_s* run over the Hkv KV heads; everything else (lse, delta, dq, the dropout
  // stream, the score bias, the dQ workspace) stays indexed by the query head. G is filled in by
  // attn_fwd / attn_bwd. The backward then has every query head write its dK / dV contribution to
  // kv_part ([2][B][H][Sk][D] bf16 in the workspace, behind the bias-gradient partials) and
  // attn_kv_group_sum_kernel adds each group's G rows in fp32 into the caller's dk / dv; the fused
  // bias gradient (dbp / dbias, laid out for [3][H][D]) is left to the caller.
  int Hkv = 0;
  int G = 1;
  uint16_t* kv_part = nullptr;
};

// lo / hi [B][S] (int32) from segment ids [B][S]: a segment is a maximal run of equal ids >= 0 and
// [lo[i], hi[i]) is the run of position i; a padding position (id < 0) gets lo = hi = i. One
// workgroup per row, nothing read on the host.
void attn_seg_bounds(const int* ids, int* lo, int* hi, int B, int S, hipStream_t st);
// Sliding window: lo / hi (query side) and klo / khi (key side), int32 [B][S] each, of the band
// i - left <= j <= i + right (left / right < 0: unbounded on that side), cut to the runs seg_lo /
// seg_hi of attn_seg_bounds when those are given (both or neither; [B][S]):
//   lo[i] = max(seg_lo[i], i - left)    hi[i] = min(seg_hi[i], i + right + 1)
//   klo[j] = max(seg_lo[j], j - right)  khi[j] = min(seg_hi[j], j + left + 1)
// with 0 / S for the run without segments; a padding position (seg_lo == seg_hi) keeps its empty
// interval on both sides. Element-wise, nothing read on the host. The outputs may not alias the inputs.
void attn_band_bounds(int left, int right, const int* seg_lo, const int* seg_hi, int* lo, int* hi, int* klo, int* khi,
                      int B, int S, hipStream_t st);
// scores [H][Sq][Sk] (fp32) of one sample: -inf outside the query's run (rows lo / hi of that sample)
void segment_mask_f32(float* s, int H, int Sq, int Sk, const int* lo, const int* hi, hipStream_t st);

// out[h][q][k] = keep(b, h0 + h, q, k) ? x[h][q][k] * drop_scale : 0 over an fp32 [H][Sq][Sk] slab of
// global sample b (the fp32 device path: P[b] after the softmax, dP in the backward); out may be x
void attn_dropout_f32(const float* x, float* out, int H, int Sq, int Sk, int b, int h0, int H_total,
                      const int64_t* rng_step, uint64_t rng_seed, uint32_t drop_thr, float drop_scale, hipStream_t st);
// the keep-mask itself as bytes [B][H][Sq][Sk] (tests, debugging)
void attn_dropout_mask(uint8_t* out, int B, int H, int Sq, int Sk, int b0, int h0, int H_total,
                       const int64_t* rng_step, uint64_t rng_seed, uint32_t drop_thr, hipStream_t st);

void attn_fwd(AttnArgs a, hipStream_t st);
bool attn_bwd(AttnArgs a, hipStream_t st);
// Hkv (0 or H: none) adds the two expanded dK / dV buffers of grouped-query attention
int64_t attn_bwd_workspace_floats(int B, int H, int Sq, int Sk, int D, int Hkv = 0);
int64_t attn_bwd_slab_floats(int B, int H, int Sq, int Sk, int D);  // offset of delta in the workspace
int64_t attn_bwd_kv_part_floats(int B, int H, int Sq, int Sk, int D);  // offset of kv_part (16-B aligned)
int attn_bwd_variant();
void attn_set_bwd_variant(int v);
int attn_fwd_variant();
void attn_set_fwd_variant(int v);
float attn_rescale_thr();
int attn_stagger();
void attn_set_stagger(int v);
void attn_set_rescale_thr(float t);

}  // namespace ffk
