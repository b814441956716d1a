// The gate activations of glu.hip (and SiLU for elementwise.hip): value and derivative from one shared
// exponential / erf, formulated so that every finite input gives finite results.
#pragma once
#include "common.h"

namespace ffk {

// s = sigmoid(x) and 1 - s from e = exp(-|x|) in (0, 1]: one v_exp, one v_rcp, and nothing that
// overflows (1 / (1 + exp(-x)) passes through inf for x < -88, and '1 - s' cancels for large x).
__device__ __forceinline__ void sigmoid_pair(float x, float& s, float& oms) {
  const float e = fast_expe(-fabsf(x));
  const float r = fast_rcp(1.f + e);
  const float er = e * r;
  s = x >= 0.f ? r : er;
  oms = x >= 0.f ? er : r;
}

__device__ __forceinline__ float silu_f(float x) {
  float s, oms;
  sigmoid_pair(x, s, oms);
  return x * s;
}
// d silu / dx = s + x s (1 - s)
__device__ __forceinline__ float silu_df(float x) {
  float s, oms;
  sigmoid_pair(x, s, oms);
  return __builtin_fmaf(x * s, oms, s);
}

enum GluAct : int { GLU_SILU = 0, GLU_GELU = 1, GLU_GELU_TANH = 2, GLU_RELU = 3, GLU_SIGMOID = 4, GLU_NACT = 5 };

// y = act(x), d = act'(x)
__device__ __forceinline__ void glu_act_grad(int act, float x, float& y, float& d) {
  switch (act) {
    case GLU_SILU: {
      float s, oms;
      sigmoid_pair(x, s, oms);
      y = x * s;
      d = __builtin_fmaf(y, oms, s);
      return;
    }
    case GLU_GELU: act_fwd_grad(ACT_GELU, x, y, d); return;
    case GLU_GELU_TANH: {
      // 0.5 (1 + tanh z) = sigmoid(2 z), z = sqrt(2/pi) (x + 0.044715 x^3); the polynomial is taken of
      // x clamped to +-32 (sigmoid(2 z) is exactly 0 or 1 in fp32 from |x| = 10 on), so x^3 stays finite
      const float xc = fminf(fmaxf(x, -32.f), 32.f);
      const float x2 = xc * xc;
      const float z2 = 1.5957691216057308f * xc * __builtin_fmaf(0.044715f, x2, 1.f);  // 2 z
      const float dz2 = 1.5957691216057308f * __builtin_fmaf(0.134145f, x2, 1.f);      // d (2 z) / dx
      float s, oms;
      sigmoid_pair(z2, s, oms);
      y = x * s;
      d = __builtin_fmaf(y * oms, dz2, s);
      return;
    }
    case GLU_RELU: y = fmaxf(x, 0.f); d = x > 0.f ? 1.f : 0.f; return;
    case GLU_SIGMOID: {
      float s, oms;
      sigmoid_pair(x, s, oms);
      y = s;
      d = s * oms;
      return;
    }
    default: y = x; d = 1.f; return;
  }
}
__device__ __forceinline__ float glu_act(int act, float x) {
  float y, d;
  glu_act_grad(act, x, y, d);  // d is dead here: the compiler drops its arithmetic
  return y;
}

}  // namespace ffk
