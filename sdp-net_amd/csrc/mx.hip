// MXFP8 inference path (opt-in; sdp_gemm never routes here): block-scaled e4m3 operands on
// v_mfma_scale_f32_16x16x128_f8f6f4, fp32 accumulation.  Format and rounding points:
// include/sdpnet_hip.h, "MX operand format"; the scale / element rules are mx_format.h.
//  * mx::quant_rows — one streaming pass: rows (bf16 / fp32, row map, optional LayerNorm
//    statistics) -> e4m3 bytes Q[M][K] + E8M0 scales S[M][K/32].
//  * mx::gemm_mx — 128 x 128 x 128 tiles, 4 waves (2 along M x 2 along N, 64 x 64 each), both
//    operands HBM -> registers -> ds_write_b128 into the XOR-swizzled [row][128 B] image of the
//    bf16 kernels (a 128-element e4m3 K-tile has the bytes of their 64-element bf16 K-tile),
//    double buffered, one barrier per K-tile.  The MFMA is issued swapped (A = W rows, B = X
//    rows) as in gemm.hip, so the accumulator holds D[n][m] with 4 consecutive n per lane, and the
//    epilogue runs from registers: a lane owns 16 columns of a row's 64-column chunk, the 4 lanes
//    l, l + 16, l + 32, l + 48 the whole chunk.
// Operand lane map of the scaled MFMA (confirmed with exact integer data by
// tests/test_gpu_gemm_mx.py; profiles/mx_fp8.md): lane l, g = l / 16, holds row / column l % 16
// and TWO 16-element runs of K: 16 g .. 16 g + 15 in registers 0-3 and 64 + 16 g .. 64 + 16 g + 15
// in registers 4-7 (lds_frag: 16-B chunks g and g + 4 of the 128-B row).  Byte 0 of its scale
// register (opsel 0) is the scale of the 32-element block g, K 32 g .. 32 g + 31 -- which lies in
// the lanes of groups 2 (g % 2) and 2 (g % 2) + 1, not in lane l.  Holding 32 consecutive K per
// lane instead pairs A and B correctly and applies the wrong blocks' scales.
#include "common.h"
#include "mx_format.h"

extern int g_exact_gelu;  // gemm.hip: sdp_gemm_set_exact_gelu

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

namespace mx {
constexpr int NTHREADS = 256;

// ---------------------------------------------------------------------------
// Quantiser: thread -> 8 consecutive elements, 4 threads a 32-element block, 16 threads the four
// blocks whose scales make one 32-bit store.  K % 128 == 0, so a 16-lane group never leaves its row.
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(NTHREADS) void quant_rows(const T* __restrict__ X, int64_t ldx, RowMap xmap,
                                                       const float* __restrict__ stats, uint8_t* __restrict__ Q,
                                                       int64_t ldq, uint8_t* __restrict__ S, int64_t lds, int M,
                                                       int K) {
  const int per_row = K >> 3;
  const int64_t idx = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (idx >= (int64_t)M * per_row) return;  // whole 16-lane groups leave together
  const int m = (int)(idx / per_row), c = (int)(idx - (int64_t)m * per_row);
  const T* xp = X + xmap(m) * ldx + c * 8;
  float v[8];
  if constexpr (sizeof(T) == 2) {
    const bf16x8 r = *(const bf16x8*)xp;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = bf2f((bf16_t)r[i]);
  } else {
    const f32x4 a = *(const f32x4*)xp, b = *(const f32x4*)(xp + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = a[i];
      v[4 + i] = b[i];
    }
  }
  if (stats) {  // LayerNorm without affine: exactly (x - mean) * rstd, two fp32 operations
    const float2 st = *(const float2*)(stats + 2 * (int64_t)m);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (v[i] - st.x) * st.y;
  }
  uint32_t amax = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) amax = max(amax, mx_bits(v[i]) & 0x7fffffffu);
  amax = max(amax, (uint32_t)__shfl_xor((int)amax, 1, 64));
  amax = max(amax, (uint32_t)__shfl_xor((int)amax, 2, 64));
  const int code = mx_scale_code(amax);
  uint32_t w[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    w[h] = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      w[h] |= (code == MX_NAN_CODE ? MX_NAN_BYTE : mx_e4m3(v[4 * h + i], code)) << (8 * i);
  }
  *(u32x2*)(Q + (int64_t)m * ldq + c * 8) = u32x2{w[0], w[1]};
  const uint32_t sc = code == MX_NAN_CODE ? 127u : (uint32_t)code;
  const int base = threadIdx.x & 48;  // first lane of the 16-lane group
  uint32_t sw = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) sw |= (uint32_t)__shfl((int)sc, base + 4 * b, 64) << (8 * b);
  if ((threadIdx.x & 15) == 0) *(uint32_t*)(S + (int64_t)m * lds + (c >> 2)) = sw;
}

// ---------------------------------------------------------------------------
// GEMM
// ---------------------------------------------------------------------------
constexpr int BM = 128, BN = 128, BK = 128;  // BK in e4m3 elements = bytes
constexpr int XT = BM * BK, STAGE = XT + BN * BK;

struct Epi {
  const float* bias;     // [N] or null
  const bf16_t* resid;   // or null (bf16 output only)
  int64_t ldr;
  RowMap rmap;
  bf16_t* out;           // bf16 output, or null
  int64_t ldc;
  RowMap cmap;
  uint8_t* outq;         // MX output: e4m3 bytes [M][N] and scales [M][N/32], or null
  int64_t ldq;
  uint8_t* outs;
  int64_t lds;
  int act;
  int resid_pre;
  int fast_gelu;
  float* part;           // {mean, M2} per stored row and 64-column chunk, or null
};

SDP_DEV i32x8 lds_frag(const char* tile, int r, int fq) {
  const i32x4 lo = *(const i32x4*)(tile + r * 128 + (fq ^ ((r >> 1) & 7)) * 16);
  const i32x4 hi = *(const i32x4*)(tile + r * 128 + ((fq + 4) ^ ((r >> 1) & 7)) * 16);
  return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// One logical row m of a wave's 64-column chunk: the lane's columns n_c + 16 i + r (i, r < 4),
// n_c = chunk base + 4 (lane / 16).  One rounding on the bf16 output, bf16(act(acc + b [+ R]) [+ R])
// (fast GEMM 9's model); the MX output quantises the fp32 act(acc + b) in 32-column blocks
// (i = 0, 1 and i = 2, 3 of the 4 lanes).  Rows past M come in clamped with row_ok = false: they
// take part in the shuffles and store nothing.  Columns past N (N % 32 == 0: whole blocks) too.
SDP_DEV void row_epilogue(const Epi& e, int m, bool row_ok, int n_c, int N, const f32x4 (&acc)[4]) {
  float v[4][4];
  bool col_ok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n_c + 16 * i;
    col_ok[i] = n < N;
    const f32x4 bv = (e.bias && col_ok[i]) ? *(const f32x4*)(e.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
    float rv[4] = {0.f, 0.f, 0.f, 0.f};
    if (e.resid && col_ok[i]) {
      const bf16x4 rr = *(const bf16x4*)(e.resid + e.rmap(m) * e.ldr + n);
#pragma unroll
      for (int r = 0; r < 4; ++r) rv[r] = bf2f((bf16_t)rr[r]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float t = acc[i][r] + bv[r];
      if (e.resid && e.resid_pre) t += rv[r];
      if (e.act != ACT_NONE) t = e.fast_gelu ? gelu_fast(t) : apply_act(e.act, t);
      if (e.resid && !e.resid_pre) t += rv[r];
      v[i][r] = t;
    }
  }
  if (e.out) {
    const int64_t prow = e.cmap(m);
    float f[4][4], sum = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bf16x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        o[r] = (short)f2bf(v[i][r]);
        f[i][r] = bf2f((bf16_t)o[r]);
        sum += f[i][r];
      }
      if (row_ok && col_ok[i]) *(bf16x4*)(e.out + prow * e.ldc + n_c + 16 * i) = o;
    }
    if (e.part && col_ok[0]) {  // N % 64 == 0 here: a chunk is whole or (wave-uniformly) past N
      sum += __shfl_xor(sum, 16, 64);
      sum += __shfl_xor(sum, 32, 64);
      const float mean = sum * (1.0f / 64.0f);
      float m2 = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) m2 = fmaf(f[i][r] - mean, f[i][r] - mean, m2);
      m2 += __shfl_xor(m2, 16, 64);
      m2 += __shfl_xor(m2, 32, 64);
      if (row_ok && (threadIdx.x & 63) < 16)
        *(float2*)(e.part + (prow * (N >> 6) + (n_c >> 6)) * 2) = float2{mean, m2};
    }
    return;
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {  // the 32-column block of i = 2h, 2h + 1
    uint32_t amax = 0;
#pragma unroll
    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
      for (int r = 0; r < 4; ++r) amax = max(amax, mx_bits(v[2 * h + ii][r]) & 0x7fffffffu);
    amax = max(amax, (uint32_t)__shfl_xor((int)amax, 16, 64));
    amax = max(amax, (uint32_t)__shfl_xor((int)amax, 32, 64));
    const int code = mx_scale_code(amax);
#pragma unroll
    for (int ii = 0; ii < 2; ++ii) {
      const int i = 2 * h + ii;
      uint32_t w = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) w |= (code == MX_NAN_CODE ? MX_NAN_BYTE : mx_e4m3(v[i][r], code)) << (8 * r);
      if (row_ok && col_ok[i]) *(uint32_t*)(e.outq + (int64_t)m * e.ldq + n_c + 16 * i) = w;
    }
    const int nb = (n_c & ~63) + 32 * h;
    if (row_ok && nb < N && (threadIdx.x & 63) < 16)
      e.outs[(int64_t)m * e.lds + (nb >> 5)] = (uint8_t)(code == MX_NAN_CODE ? 127 : code);
  }
}

__global__ __launch_bounds__(NTHREADS) void gemm_mx(const uint8_t* __restrict__ Xq, int64_t ldxq,
                                                    const uint8_t* __restrict__ Xs, int64_t ldxs,
                                                    const uint8_t* __restrict__ Wq, int64_t ldwq,
                                                    const uint8_t* __restrict__ Ws, int64_t ldws, Epi epi, int M, int N,
                                                    int K) {
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, fr = lane & 15, fq = lane >> 4;
  const int nt = K / BK;

  // loads: thread -> 16-B chunk lc of rows lr + 32 i (8 lanes cover a row's 128 B).  Rows past M / N
  // re-read the last row (their results are never stored).
  const int lc = tid & 7, lr = tid >> 3;
  const uint8_t* xp[4];
  const uint8_t* wp[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    xp[i] = Xq + (int64_t)min(m0 + lr + 32 * i, M - 1) * ldxq + lc * 16;
    wp[i] = Wq + (int64_t)min(n0 + lr + 32 * i, N - 1) * ldwq + lc * 16;
  }
  // scales: one 32-bit word per row and K-tile, byte fq is this lane's block
  const uint8_t* xsp[4];
  const uint8_t* wsp[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    xsp[i] = Xs + (int64_t)min(m0 + wm * 64 + i * 16 + fr, M - 1) * ldxs;
    wsp[i] = Ws + (int64_t)min(n0 + wn * 64 + i * 16 + fr, N - 1) * ldws;
  }
  i32x4 xr[4], wr[4];
  uint32_t xs[4], ws[4];
  auto gload = [&](int t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      xr[i] = *(const i32x4*)(xp[i] + (int64_t)t * BK);
      wr[i] = *(const i32x4*)(wp[i] + (int64_t)t * BK);
    }
  };
  auto sload = [&](int t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      xs[i] = *(const uint32_t*)(xsp[i] + 4 * t);
      ws[i] = *(const uint32_t*)(wsp[i] + 4 * t);
    }
  };
  auto lstore = [&](char* st) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = lr + 32 * i;
      const int o = r * 128 + (lc ^ ((r >> 1) & 7)) * 16;
      *(i32x4*)(st + o) = xr[i];
      *(i32x4*)(st + XT + o) = wr[i];
    }
  };

  f32x4 acc[4][4];  // [i: 16 columns of n][j: 16 rows of m]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  gload(0);
  sload(0);
  lstore(lds);
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const char* st = lds + (t & 1) * STAGE;
    int sa[4], sb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sa[i] = (int)((ws[i] >> (8 * fq)) & 0xffu);
      sb[i] = (int)((xs[i] >> (8 * fq)) & 0xffu);
    }
    if (t + 1 < nt) {
      gload(t + 1);
      sload(t + 1);
    }
    i32x8 aw[4], bx[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      aw[i] = lds_frag(st + XT, wn * 64 + i * 16 + fr, fq);
      bx[i] = lds_frag(st, wm * 64 + i * 16 + fr, fq);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(aw[i], bx[j], acc[i][j], 0, 0, 0, sa[i], 0, sb[j]);
    // the other stage was last read in iteration t - 1, which every wave left through the barrier
    if (t + 1 < nt) lstore(lds + ((t + 1) & 1) * STAGE);
    __syncthreads();
  }

  // D[n][m]: the lane holds n = .. + 16 i + 4 fq + r, m = .. + 16 j + fr
  // (four calls, not a loop: the body is too large for the unroller, and a rolled loop would index
  // the accumulators at run time)
  auto rows = [&](int j, const f32x4 (&row)[4]) {
    const int m = m0 + wm * 64 + j * 16 + fr;
    row_epilogue(epi, min(m, M - 1), m < M, n0 + wn * 64 + fq * 4, N, row);
  };
  rows(0, {acc[0][0], acc[1][0], acc[2][0], acc[3][0]});
  rows(1, {acc[0][1], acc[1][1], acc[2][1], acc[3][1]});
  rows(2, {acc[0][2], acc[1][2], acc[2][2], acc[3][2]});
  rows(3, {acc[0][3], acc[1][3], acc[2][3], acc[3][3]});
}
}  // namespace mx

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
static RowMap mx_map(int grp, int64_t gstride, int off) {
  RowMap r;
  r.grp = grp > 0 ? grp : 0x7fffffff;
  r.gstride = grp > 0 ? gstride : 0;
  r.off = grp > 0 ? off : 0;
  return r;
}

static bool mx_al(const void* p, uintptr_t a) { return (uintptr_t)p % a == 0; }

extern "C" int sdp_mx_quant_rows(int dtype, const void* X, int64_t ldx, int x_grp, int64_t x_gstride, int x_off,
                                 const float* stats, void* Q, int64_t ldq, void* S, int64_t lds, int M, int K,
                                 void* stream) {
  if ((dtype != 0 && dtype != 1) || !X || !Q || !S || M < 0 || K <= 0 || K % 128) return (int)hipErrorInvalidValue;
  if (ldx < K || ldq < K || ldq % 16 || lds < K / 32 || lds % 4) return (int)hipErrorInvalidValue;
  // 16-B input vectors, 8-B byte stores, 4-B scale words
  if (!mx_al(X, 16) || ldx % (dtype == 1 ? 8 : 4) || !mx_al(Q, 16) || !mx_al(S, 4) || (stats && !mx_al(stats, 8)))
    return (int)hipErrorInvalidValue;
  if (M == 0) return 0;
  const int64_t threads = (int64_t)M * (K / 8);
  const int64_t blocks = (threads + mx::NTHREADS - 1) / mx::NTHREADS;
  if (blocks > 0x7fffffff) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const RowMap xm = mx_map(x_grp, x_gstride, x_off);
  if (dtype == 1)
    hipLaunchKernelGGL(mx::quant_rows<bf16_t>, dim3((unsigned)blocks), dim3(mx::NTHREADS), 0, s, (const bf16_t*)X, ldx,
                       xm, stats, (uint8_t*)Q, ldq, (uint8_t*)S, lds, M, K);
  else
    hipLaunchKernelGGL(mx::quant_rows<float>, dim3((unsigned)blocks), dim3(mx::NTHREADS), 0, s, (const float*)X, ldx,
                       xm, stats, (uint8_t*)Q, ldq, (uint8_t*)S, lds, M, K);
  return SDP_CHECK_LAUNCH();
}

extern "C" int sdp_gemm_mx_applies(int M, int N, int K, int out_is_mx) {
  (void)out_is_mx;  // both outputs work in whole 32-column blocks
  return M >= 1 && N >= 32 && N % 32 == 0 && K >= 128 && K % 128 == 0;
}

extern "C" int sdp_gemm_mx(const void* Xq, int64_t ldxq, const void* Xs, int64_t ldxs, const void* Wq, int64_t ldwq,
                           const void* Ws, int64_t ldws, const float* bias, const void* R, int64_t ldr, int r_grp,
                           int64_t r_gstride, int r_off, void* Y, int64_t ldy, int y_grp, int64_t y_gstride, int y_off,
                           void* Yq, int64_t ldyq, void* Ys, int64_t ldys, int M, int N, int K, int act, int resid_pre,
                           float* part, void* stream) {
  if (!Xq || !Xs || !Wq || !Ws || M < 0 || N <= 0 || K <= 0 || act < 0 || act > ACT_KELU)
    return (int)hipErrorInvalidValue;
  const bool out_mx = Yq != nullptr;
  if ((Y != nullptr) == out_mx || (out_mx && !Ys)) return (int)hipErrorInvalidValue;  // exactly one output
  if (!sdp_gemm_mx_applies(M > 0 ? M : 1, N, K, out_mx)) return (int)hipErrorInvalidValue;
  if (out_mx && (R || part)) return (int)hipErrorInvalidValue;
  if (part && N % 64) return (int)hipErrorInvalidValue;
  if (ldxq < K || ldwq < K || ldxq % 16 || ldwq % 16 || !mx_al(Xq, 16) || !mx_al(Wq, 16) || ldxs < K / 32 ||
      ldws < K / 32 || ldxs % 4 || ldws % 4 || !mx_al(Xs, 4) || !mx_al(Ws, 4) || (bias && !mx_al(bias, 16)))
    return (int)hipErrorInvalidValue;
  if (out_mx ? (ldyq < N || ldyq % 4 || !mx_al(Yq, 4) || ldys < N / 32)
             : (ldy < N || ldy % 4 || !mx_al(Y, 8) || (R && (ldr < N || ldr % 4 || !mx_al(R, 8))) ||
                (part && !mx_al(part, 8))))
    return (int)hipErrorInvalidValue;
  if ((N + mx::BN - 1) / mx::BN > 65535) return (int)hipErrorInvalidValue;
  if (M == 0) return 0;
  mx::Epi e{bias, (const bf16_t*)R, ldr, mx_map(r_grp, r_gstride, r_off), (bf16_t*)Y, ldy,
            mx_map(y_grp, y_gstride, y_off), (uint8_t*)Yq, ldyq, (uint8_t*)Ys, ldys, act, resid_pre,
            (act == ACT_GELU && !g_exact_gelu) ? 1 : 0, part};
  const dim3 grid((M + mx::BM - 1) / mx::BM, (N + mx::BN - 1) / mx::BN);
  hipLaunchKernelGGL(mx::gemm_mx, grid, dim3(mx::NTHREADS), 0, (hipStream_t)stream, (const uint8_t*)Xq, ldxq,
                     (const uint8_t*)Xs, ldxs, (const uint8_t*)Wq, ldwq, (const uint8_t*)Ws, ldws, e, M, N, K);
  return SDP_CHECK_LAUNCH();
}
