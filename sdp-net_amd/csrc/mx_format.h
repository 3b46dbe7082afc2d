// MX (block-scaled) FP8 operand format of sdp_mx_quant_rows / sdp_gemm_mx: the scale and element
// rules of include/sdpnet_hip.h ("MX operand format"), as plain integer / fp32 code that compiles
// for the device and for the host alike.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MX_HD __host__ __device__ inline
#else
#define MX_HD inline
#endif

constexpr int MX_BLOCK = 32;           // K elements per scale
constexpr uint32_t MX_NAN_BYTE = 0x7f; // e4m3fn NaN
constexpr int MX_NAN_CODE = -1;        // mx_scale_code: the block holds a NaN or an Inf

MX_HD uint32_t mx_bits(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  return u;
}

// E8M0 code of a block from the bits of its largest magnitude (sign cleared): amax = m 2^E with
// m in [1, 2) read from the exponent field (a subnormal amax reads E = -127 and clamps to code 0);
// e = E - 8 for m <= 1.75, else E - 7: the smallest e with amax 2^-e <= 448.  No clamping of
// elements, no log2f.  A zero block gives 127, a non-finite one MX_NAN_CODE.
MX_HD int mx_scale_code(uint32_t amax_bits) {
  if (amax_bits >= 0x7f800000u) return MX_NAN_CODE;
  if (amax_bits == 0) return 127;
  const int E = (int)(amax_bits >> 23) - 127;
  const int e = (amax_bits & 0x7fffffu) <= 0x600000u ? E - 8 : E - 7;
  const int code = e + 127;
  return code < 0 ? 0 : (code > 254 ? 254 : code);
}

// e4m3fn byte of v 2^-(code - 127), rounded to nearest even on the e4m3 grid (subnormals, spacing
// 2^-9, included).  The scaled value is exact in fp32 wherever it is not below the grid's first
// tie, and at most 448 by the scale rule, so nothing saturates.  The sign survives, also on zero.
MX_HD uint32_t mx_e4m3(float v, int code) {
  const float y = ldexpf(v, 127 - code);
  const uint32_t u = mx_bits(y), sign = (u >> 24) & 0x80u;
  uint32_t a = u & 0x7fffffffu;
  if (a < 0x3c800000u) {  // |y| < 2^-6: subnormal grid, 0 .. 8 steps of 2^-9 (8 = the first normal)
    float ay;
    memcpy(&ay, &a, 4);
    return sign | (uint32_t)(int)rintf(ay * 512.0f);
  }
  a += 0x7ffffu + ((a >> 20) & 1u);  // nearest even at 3 mantissa bits
  return sign | ((((a >> 23) - 120u) << 3) | ((a >> 20) & 7u));
}
