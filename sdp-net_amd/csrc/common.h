// Shared device helpers for the SdP-Net gfx950 kernels.
// Storage types: float (fp32 path) and bf16 (uint16 bit pattern, bf16 path).
// All arithmetic is fp32; bf16 is storage only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "sdpnet_hip.h"

typedef uint16_t bf16_t;
typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) short bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

#define SDP_DEV __device__ __forceinline__
#define AS1 __attribute__((address_space(1)))
#define AS3 __attribute__((address_space(3)))

SDP_DEV float bf2f(bf16_t u) { return __uint_as_float(((uint32_t)u) << 16); }
SDP_DEV bf16_t f2bf(float f) { return __builtin_bit_cast(bf16_t, (__bf16)f); }

template <typename T> SDP_DEV float to_f(T v);
template <> SDP_DEV float to_f<float>(float v) { return v; }
template <> SDP_DEV float to_f<bf16_t>(bf16_t v) { return bf2f(v); }

template <typename T> SDP_DEV T from_f(float v);
template <> SDP_DEV float from_f<float>(float v) { return v; }
template <> SDP_DEV bf16_t from_f<bf16_t>(float v) { return f2bf(v); }

// ---- activations: model.py:13-24 registry, training_utilities.py:91-92 (KeLu)
enum SdpAct {
  ACT_NONE = 0, ACT_GELU = 1, ACT_RELU = 2, ACT_TANH = 3, ACT_SIGMOID = 4,
  ACT_LEAKY_RELU = 5, ACT_SELU = 6, ACT_KELU = 7
};

// Hot-epilogue GELU: the tanh form x * sigmoid(sqrt(2/pi) (x + 0.044715 x^3))
// = x / (1 + exp2(x (k + k2 x^2))), one v_exp_f32 + one v_rcp_f32 per element.
// Max |err| vs the exact erf GELU (nn.GELU(), layers.py:88) is 4.7e-4 absolute /
// 0.22 % relative (|y| > 0.05), i.e. at most one bf16 rounding of the output,
// which the bf16 path applies anyway.  The generic path keeps the erf form (gelu_erf below).
// gelu_fast (scalar) and gelu_fast2 (packed) perform the same fused operations in
// the same order, so every epilogue path gives bit-identical results.
typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr float GELU_K = -2.3022081983f;          // -sqrt(2/pi) * log2(e)
constexpr float GELU_K2 = -0.10294324471f;        // GELU_K * 0.044715
SDP_DEV float gelu_fast(float x) {
  const float a = fmaf(x * x, GELU_K2, GELU_K);
  const float t = __builtin_amdgcn_exp2f(x * a);
  return x * __builtin_amdgcn_rcpf(t + 1.0f);
}
SDP_DEV f32x2 gelu_fast2(f32x2 x) {
  const f32x2 a = (x * x) * GELU_K2 + GELU_K;
  const f32x2 u = x * a;
  const f32x2 t = {__builtin_amdgcn_exp2f(u.x), __builtin_amdgcn_exp2f(u.y)};
  const f32x2 d = t + 1.0f;
  return x * f32x2{__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
}

// Phi(x) = P(N(0,1) <= x) and e = exp(-x^2 / 2), branch-free: erfc(|x| / sqrt 2) by Abramowitz &
// Stegun 7.1.26 (t = 1 / (1 + p z), erfc(z) = t (a1 + .. + a5 t^4) exp(-z^2), |error| <= 1.5e-7),
// sharing its exp(-z^2) with GELU's derivative.  Measured over [-12, 12] against double-precision
// erf: |d Phi| <= 3.0e-7, |d gelu| <= 4.2e-7, |d gelu'| <= 3.0e-7 -- the fp32 formula
// 0.5 x (1 + erff(x / sqrt 2)) is itself off by up to 4.5e-7.  2 transcendental + 12 VALU per
// element, against ~35 (two erff branches + a full-range expf) before.  Every product / sum is
// an explicit mul or fma, so no path can contract it differently (all kernels agree bit for bit).
SDP_DEV float norm_cdf(float x, float& e) {
  const float z = fabsf(x) * 0.70710678118654752f;
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
  float y = fmaf(t, 1.061405429f, -1.453152027f);
  y = fmaf(t, y, 1.421413741f);
  y = fmaf(t, y, -0.284496736f);
  y = fmaf(t, y, 0.254829592f);
  y = y * t;
  const float x2 = x * x;
  e = __builtin_amdgcn_exp2f(x2 * -0.72134752044448170f);  // exp(-x^2 / 2)
  const float h = y * e;                                     // erfc(|x| / sqrt 2)
  return x >= 0.f ? fmaf(-0.5f, h, 1.0f) : 0.5f * h;
}
SDP_DEV float gelu_erf(float x) {
  float e;
  return x * norm_cdf(x, e);
}
SDP_DEV float gelu_erf_grad(float x) {  // Phi(x) + x phi(x)
  float e;
  const float cdf = norm_cdf(x, e);
  return fmaf(x * e, 0.39894228040143268f, cdf);
}

SDP_DEV float apply_act(int act, float x) {
  switch (act) {
    case ACT_GELU: return gelu_erf(x);  // erf GELU (nn.GELU())
    case ACT_RELU: return x < 0.0f ? 0.0f : x;  // (not fmaxf: a NaN stays a NaN, as torch's relu)
    case ACT_TANH: return tanhf(x);
    case ACT_SIGMOID: return 1.0f / (1.0f + expf(-x));
    case ACT_LEAKY_RELU: return x >= 0.0f ? x : 0.01f * x;
    case ACT_SELU: {
      const float alpha = 1.6732632423543772848f, scale = 1.0507009873554804934f;
      // expm1f: expf(x) - 1 loses every digit of a small negative x to the rounding of expf at 1
      return scale * (x > 0.0f ? x : alpha * expm1f(x));
    }
    case ACT_KELU: {
      const float a = 3.5f;
      if (x < -a) return 0.0f;
      if (x > a) return x;
      return 0.5f * x * (1.0f + x / a + 0.31830988618379067f * sinf(x * 3.14159265358979323846f / a));
    }
    default: return x;
  }
}

// ---------------------------------------------------------------------------
// counter-hash RNG for dropout / drop-path masks: keep(seed, idx) = u(seed, idx) >= p
// ---------------------------------------------------------------------------
SDP_DEV uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352dU;
  x ^= x >> 15;
  x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}
SDP_DEV float uniform01(uint64_t seed, uint64_t idx) {
  const uint32_t h = mix32((uint32_t)idx ^ mix32((uint32_t)seed ^ mix32((uint32_t)(idx >> 32) + (uint32_t)(seed >> 32) * 0x9e3779b9U)));
  return (float)(h >> 8) * (1.0f / 16777216.0f);
}

// uniform01(seed, idx) >= p in two parts, for runs of consecutive indices: drop_key depends only on
// the upper 32 index bits (shared by any 8-aligned run of 8), drop_keep is one mix32 per element.
// Bit-identical to the uniform01 test: (h >> 8) * 2^-24 >= p  <=>  h >= ceil(p * 2^24) << 8 (both
// sides exact in fp32; p < 1 keeps the threshold below 2^32).
SDP_DEV uint32_t drop_key(uint64_t seed, uint64_t idx) {
  return mix32((uint32_t)seed ^ mix32((uint32_t)(idx >> 32) + (uint32_t)(seed >> 32) * 0x9e3779b9U));
}
SDP_DEV uint32_t drop_thresh(float p) { return (uint32_t)ceilf(p * 16777216.0f) << 8; }
SDP_DEV bool drop_keep(uint32_t key, uint32_t idx_lo, uint32_t thr) { return mix32(idx_lo ^ key) >= thr; }

// act'(x) of apply_act (training backward; erf-form GELU).
SDP_DEV float act_grad(int act, float x) {
  switch (act) {
    case ACT_GELU: return gelu_erf_grad(x);
    case ACT_RELU: return x > 0.0f ? 1.0f : 0.0f;
    case ACT_TANH: { const float t = tanhf(x); return 1.0f - t * t; }
    case ACT_SIGMOID: { const float s = 1.0f / (1.0f + expf(-x)); return s * (1.0f - s); }
    case ACT_LEAKY_RELU: return x > 0.0f ? 1.0f : 0.01f;
    case ACT_SELU: {
      const float alpha = 1.6732632423543772848f, scale = 1.0507009873554804934f;
      return x > 0.0f ? scale : scale * alpha * expf(x);
    }
    case ACT_KELU: {
      const float a = 3.5f, k = 3.14159265358979323846f / a;
      if (x < -a) return 0.0f;
      if (x > a) return 1.0f;
      return 0.5f * (1.0f + 2.0f * x / a + 0.31830988618379067f * sinf(k * x) + x * cosf(k * x) / a);
    }
    default: return 1.0f;
  }
}

// Grouped row map: logical row m -> physical row (m / grp) * gstride + off + (m % grp).
// Lets one kernel address the image rows of a [B, R+P, C] token buffer (grp=P,
// gstride=R+P, off=R), a plain dense matrix (grp=huge, gstride=0, off=0), or a
// table broadcast over the batch (grp=P, gstride=0, off=0).
// Logical rows are < 2^31 and grp > 0 (every constructor maps "dense" to grp = INT_MAX), so the
// division runs in 32 bits: a 64-bit division is a ~40-instruction sequence (plus a branch to its
// 32-bit fast path) per call, which per-row kernels paid once per operand and row.
struct RowMap {
  int grp;
  int off;
  int64_t gstride;
  SDP_DEV int64_t operator()(int64_t m) const {
    const uint32_t mm = (uint32_t)m, g = (uint32_t)grp;
    const uint32_t q = mm / g;
    return (int64_t)q * gstride + off + (int64_t)(mm - q * g);
  }
};

SDP_DEV float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
SDP_DEV float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// (fp64: the loss kernels and the fp32 softmax backward form their gradients, differences that
// cancel, in double and round once)
SDP_DEV double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

#define SDP_CHECK_LAUNCH() (int)hipGetLastError()

// Kernel skipping for timing experiments (tools/r4_skip.sh): compiled in only by the diagnostic
// build (`make stamps`, -DSDP_DIAG, a separate library the product never loads).  In the product
// library every skip test is the constant 0, so no entry point can return without its launch.
#ifdef SDP_DIAG
extern int g_sdp_debug_skip;
#define SDP_DIAG_SKIP(bit) (g_sdp_debug_skip & (bit))
#else
#define SDP_DIAG_SKIP(bit) 0
#endif
