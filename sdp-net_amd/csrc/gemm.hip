// Dense contractions of the SdP-Net forward on gfx950 MFMA.
//
// Every GEMM on the hot path has the nn.Linear / 1x1-conv form
//     Y[m, n] = epilogue( sum_k X[m, k] * W[n, k] )
// with W stored [N][K] (K contiguous) exactly as torch keeps Linear weights and
// 1x1-conv weights ([out, in, 1, 1]).  Call sites: layers.py:79-91 (1x1 convs of
// ConvMixer), layers.py:242-249 / :282-284 / :301 / :308 (q/k/v/o projections and
// FFN of EncoderLayer), layers.py:34-42 (patch conv as a GEMM over im2col rows),
// layers.py:449-454 (classification head).
//
// Epilogue (fused, fp32):  v = acc + bias[n];  if (resid_pre) v += R[m,n];
//                          v = act(v);         if (!resid_pre) v += R[m,n];
// covers  act(conv)+x  (ConvMixer), x + FFN (+bias) (Encoder), pos-emb add +
// embedding activation (EmbeddingLayer), Tanh (head).
//
// Kernels (bf16 fast path selected by sdp_gemm_set_fast_kernel, default 14):
//  * gemm_bf16_8ph — the hot kernel: 256x256x64 tiles, 8 waves (2 along M x
//    4 along N, 128x64 per wave), v_mfma_f32_16x16x32_bf16, both operands staged
//    HBM->LDS by global_load_lds_dwordx4 into an XOR-swizzled [row][64] image
//    (conflict-free ds_read_b128), 4 phases per K-tile with the two wave groups
//    ping-ponging MFMA against LDS traffic, XCD-aware tile order.  Epilogue 14 =
//    whole-line LDS-staged stores (default), 9 = register epilogue (fallback).
//    Requires K % 64 == 0; any M, N (clamped loads, masked stores).
//  * gemm_generic<T> — correctness path for fp32 (exact f32 MFMA
//    v_mfma_f32_16x16x4_f32) and for odd bf16 shapes; fully masked.
//  * small::gemm_bf16_splitk + small::splitk_reduce — opt-in small-M path (sdp_gemm_splitk
//    only; sdp_gemm never routes to it): BM x 64 tiles over K-slices, fp32 slabs.
//
// The MFMA is issued "swapped" (A-operand = W rows, B-operand = X rows) so the
// accumulator holds D[n][m] with 4 consecutive n per lane: every epilogue
// access (bias, residual, output) is an 8/16-byte vector per lane.
#include "common.h"
#include <mutex>
#include <type_traits>


template <typename T>
struct Epi {
  const float* bias;   // [N] or null
  const T* resid;      // or null
  int64_t ldr;
  RowMap rmap;
  T* out;
  int64_t ldc;
  RowMap cmap;
  int act;
  int resid_pre;
  // LayerNorm folded into this GEMM (W = W_orig * gamma, bias = beta . W_orig^T + b):
  // v = rstd_m * acc - rstd_m * mean_m * lnsum[n] + bias[n], (mean, rstd) = lnst[m]
  const float* lnst;   // float2 per logical row, or null
  const float* lnsum;  // [N] column sums of the folded weight
  // Per-row partial statistics of the stored outputs, 64-column chunks:
  // part[(cmap(m) * (N/64) + n/64) * 2 + {0,1}] = {mean, M2} (whole-line epilogue only)
  float* part;
  int nt_store = 0;  // whole-line epilogue: non-temporal (streaming) output stores
  int group_m = 1;   // 8ph tile raster: M-blocks per group (1 = row-major tiles)
  // training epilogues (EPI 5 / 6 of the 8-phase kernel, dense rows), act2 / p2 / seed2 as
  // sdp_act_fwd / sdp_act_bwd (mask index m * N + n):
  //   EPI 5: out = z (pre-activation), out2[m * ld2 + n] = dropout(act2(z))
  //   EPI 6: out = dropout(acc) * act2'(resid)       (resid = the stored pre-activation z)
  // launch timeline (bench.py's roofline inside graph replay): {min start, max end} in
  // s_memrealtime ticks (100 MHz), or null
  unsigned long long* tline = nullptr;
  // byte extents of out / resid / part (tile_epilogue_fl's buffer descriptors; < 2 GiB)
  uint32_t out_bytes = 0, res_bytes = 0, part_bytes = 0;
  T* out2 = nullptr;
  int64_t ld2 = 0;
  int act2 = 0;
  float p2 = 0.f;
  uint64_t seed2 = 0;
};

// fold: v = r * acc + (b - r * mu * s) for one element (generic paths)
SDP_DEV float ln_fold(float acc, float r, float rmu, float s, float b) { return fmaf(r, acc, fmaf(-rmu, s, b)); }

// Apply the epilogue to 4 consecutive columns n..n+3 of logical row m.  FAST_GELU: GELU in the
// fast kernel's tanh form (its ragged tiles; the generic kernel keeps the erf form).
template <typename T, bool FAST_GELU = false>
SDP_DEV void epi_store4(const Epi<T>& e, int64_t m, int n, int N, f32x4 acc) {
  float v[4] = {acc[0], acc[1], acc[2], acc[3]};
  const bool full = (n + 3 < N);
  if (e.lnst) {
    // two floats, not one float2: this is the path a 4-B aligned lnst falls to
    const float2 st = float2{e.lnst[2 * m], e.lnst[2 * m + 1]};
    const float rmu = st.y * st.x;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (full || n + r < N) v[r] = ln_fold(v[r], st.y, rmu, e.lnsum[n + r], e.bias ? e.bias[n + r] : 0.f);
  } else if (e.bias) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += (full || n + r < N) ? e.bias[n + r] : 0.f;
  }
  float rv[4] = {0.f, 0.f, 0.f, 0.f};
  if (e.resid) {
    const T* rp = e.resid + e.rmap(m) * e.ldr + n;
    if constexpr (sizeof(T) == 2) {
      if (full && ((((uintptr_t)rp) & 7) == 0)) {
        bf16x4 rr = *(const bf16x4*)rp;
#pragma unroll
        for (int r = 0; r < 4; ++r) rv[r] = bf2f((bf16_t)rr[r]);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) if (n + r < N) rv[r] = to_f<T>(rp[r]);
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) if (n + r < N) rv[r] = to_f<T>(rp[r]);
    }
  }
  if (e.resid && e.resid_pre) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += rv[r];
  }
  if (e.act != ACT_NONE) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = FAST_GELU ? gelu_fast(v[r]) : apply_act(e.act, v[r]);
  }
  if (e.resid && !e.resid_pre) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += rv[r];
  }
  T* op = e.out + e.cmap(m) * e.ldc + n;
  if constexpr (sizeof(T) == 2) {
    if (full && ((((uintptr_t)op) & 7) == 0)) {
      bf16x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = (short)f2bf(v[r]);
      *(bf16x4*)op = o;
      return;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) if (n + r < N) op[r] = from_f<T>(v[r]);
}

// ---------------------------------------------------------------------------
// Hot kernel: bf16, 256x256x64 tiles, LDS-DMA double buffer (gemm_bf16_8ph below).
// ---------------------------------------------------------------------------
namespace fast {
constexpr int BM = 256, BN = 256, BK = 64;
constexpr int TILE_BYTES = BM * BK * 2;       // 32 KiB per operand per stage
constexpr int NTHREADS = 512;

// LDS image of one operand tile: [256 rows][64 bf16] = 128 B per row, 16-B chunk
// c of row r stored at chunk position c ^ ((r >> 1) & 7): a 16-lane ds_read_b128
// group reading one logical chunk of 16 consecutive rows hits 16 distinct 4-bank
// slots (conflict-free).
SDP_DEV int swz(int r, int c) { return c ^ ((r >> 1) & 7); }

SDP_DEV bf16x8 lds_frag(const char* lds_tile, int r, int c) {
  return *(const bf16x8*)(lds_tile + r * 128 + swz(r, c) * 16);
}

// Epilogue activation is a template parameter: ACT_NONE, ACT_GELU (fast erf) or -1
// (runtime code through apply_act).
template <int ACT>
SDP_DEV float epi_act(int code, float v) {
  if constexpr (ACT == ACT_NONE) return v;
  else if constexpr (ACT == ACT_GELU) return gelu_fast(v);
  else if constexpr (ACT == ACT_TANH) return tanhf(v);
  else return apply_act(code, v);
}

// Epilogue of one tile held as acc[4 n-tiles][8 m-tiles] per wave (wave's n base:
// n0 + wn*64, m base: m0 + wm*128).
template <int ACT>
SDP_DEV void tile_epilogue(const Epi<bf16_t>& epi, f32x4 (&acc)[4][8], int m0, int n0, int M, int N, int wm, int wn,
                           int fr, int fq) {
  // D[n][m]: lane holds n = base + 4*fq + r, m = base + fr.
  const bool full_n = (n0 + BN <= N);
  if (!full_n) {
    // the same activation form as the full tiles: a column's result must not depend on where
    // the tile boundaries fall (epi_store4's own GELU is the generic kernel's erf form)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int m = m0 + wm * 128 + j * 16 + fr;
      if (m >= M) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int n = n0 + wn * 64 + i * 16 + fq * 4;
        if (n < N) epi_store4<bf16_t, ACT == ACT_GELU>(epi, m, n, N, acc[i][j]);
      }
    }
    return;
  }
  f32x4 bv[4], sv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + wn * 64 + i * 16 + fq * 4;
    bv[i] = epi.bias ? *(const f32x4*)(epi.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
    sv[i] = epi.lnst ? *(const f32x4*)(epi.lnsum + n) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int m = m0 + wm * 128 + j * 16 + fr;
    if (m >= M) continue;
    float lr = 1.f, lrmu = 0.f;
    if (epi.lnst) {
      const float2 st = *(const float2*)(epi.lnst + 2 * (int64_t)m);
      lr = st.y;
      lrmu = st.y * st.x;
    }
    const int nb = n0 + wn * 64 + fq * 4;
    bf16x4 rr[4];
    if (epi.resid) {
      const bf16_t* rp = epi.resid + epi.rmap(m) * epi.ldr + nb;
#pragma unroll
      for (int i = 0; i < 4; ++i) rr[i] = *(const bf16x4*)(rp + i * 16);
    }
    bf16_t* op = epi.out + epi.cmap(m) * epi.ldc + nb;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bf16x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = epi.lnst ? ln_fold(acc[i][j][r], lr, lrmu, sv[i][r], bv[i][r]) : acc[i][j][r] + bv[i][r];
        if (epi.resid && epi.resid_pre) v += bf2f((bf16_t)rr[i][r]);
        v = epi_act<ACT>(epi.act, v);
        if (epi.resid && !epi.resid_pre) v += bf2f((bf16_t)rr[i][r]);
        o[r] = (short)f2bf(v);
      }
      *(bf16x4*)(op + i * 16) = o;
    }
  }
}

// Same epilogue with 16-byte stores: v_permlane16_swap pairs the 4-column chunks of
// n-tiles (2p, 2p+1) held by lanes l and l+16, so each lane ends up with 8
// contiguous columns (col0 = 32p + {0,16,8,24}[fq]); residual loads / output
// stores become one 16-B access per lane per pair (half the store instructions).
SDP_DEV int pair_col0(int fq) { return 8 * (((fq & 1) << 1) | (fq >> 1)); }

template <int ACT, int TBN = BN, int JB = 8, bool FULL = false>
SDP_DEV void tile_epilogue16(const Epi<bf16_t>& epi, f32x4 (&acc)[4][8], int m0, int n0, int M, int N, int wm,
                             int wn, int fr, int fq) {
  // FULL: the caller guarantees m0 + 256 <= M and n0 + TBN <= N (no row checks, so
  // every residual load is consumed on every path)
  if (!FULL && n0 + TBN > N) {  // ragged N: generic per-4 path
    tile_epilogue<ACT>(epi, acc, m0, n0, M, N, wm, wn, fr, fq);
    return;
  }
  const int cbase = n0 + wn * 64 + pair_col0(fq);
  f32x4 bv[2][2], sv[2][2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    if (epi.bias) {
      bv[p][0] = *(const f32x4*)(epi.bias + cbase + 32 * p);
      bv[p][1] = *(const f32x4*)(epi.bias + cbase + 32 * p + 4);
    } else {
      bv[p][0] = bv[p][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (epi.lnst) {
      sv[p][0] = *(const f32x4*)(epi.lnsum + cbase + 32 * p);
      sv[p][1] = *(const f32x4*)(epi.lnsum + cbase + 32 * p + 4);
    } else {
      sv[p][0] = sv[p][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  // Residual loads are issued JB row groups at a time (one 16-B load per lane per
  // (row group, pair)) ahead of their use, so a tile waits on memory 8 / JB times
  // instead of once per row group.
#pragma unroll
  for (int j0 = 0; j0 < 8; j0 += JB) {
    bf16x8 rres[JB][2];
    if (epi.resid) {
#pragma unroll
      for (int jj = 0; jj < JB; ++jj) {
        int m = m0 + wm * 128 + (j0 + jj) * 16 + fr;
        if (!FULL) m = m < M ? m : M - 1;
        const bf16_t* rp = epi.resid + epi.rmap(m) * epi.ldr + cbase;
#pragma unroll
        for (int p = 0; p < 2; ++p) rres[jj][p] = *(const bf16x8*)(rp + 32 * p);
      }
    }
#pragma unroll
    for (int jj = 0; jj < JB; ++jj) {
      const int j = j0 + jj;
      const int m = m0 + wm * 128 + j * 16 + fr;
      if (!FULL && m >= M) continue;
      const bf16x8* rr = rres[jj];
      bf16_t* op = epi.out + epi.cmap(m) * epi.ldc + cbase;
      float lr = 1.f, lrmu = 0.f;
      if (epi.lnst) {
        const float2 st = *(const float2*)(epi.lnst + 2 * (int64_t)m);
        lr = st.y;
        lrmu = st.y * st.x;
      }
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        float v[8];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[2 * p][j][r]),
                                                     __float_as_uint(acc[2 * p + 1][j][r]), false, false);
          v[r] = __uint_as_float(sw[0]);
          v[4 + r] = __uint_as_float(sw[1]);
        }
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float x = epi.lnst ? ln_fold(v[e], lr, lrmu, sv[p][e >> 2][e & 3], bv[p][e >> 2][e & 3])
                             : v[e] + bv[p][e >> 2][e & 3];
          if (epi.resid && epi.resid_pre) x += bf2f((bf16_t)rr[p][e]);
          x = epi_act<ACT>(epi.act, x);
          if (epi.resid && !epi.resid_pre) x += bf2f((bf16_t)rr[p][e]);
          o[e] = (short)f2bf(x);
        }
        *(bf16x8*)(op + 32 * p) = o;
      }
    }
  }
}

// Full-tile epilogue with whole-line memory accesses.  A wave's 16-row x 64-col
// slice (row group j) is packed to bf16 in the MFMA layout (row fr, 8 columns per
// lane after the permlane16 pairing), written to the wave's private 2 KiB LDS slot
// (XOR-swizzled 16-B chunks), and read back so that lane l owns row (l>>3) + 8q,
// chunk l&7: each 16-B store (and residual load) instruction then covers 8 full
// 128-B rows instead of 16 half rows.  The residual is added after the staging
// (v = bf16(act(acc + b)) + R, rounded again), i.e. resid_pre = 0 semantics; the
// caller routes resid_pre with an activation elsewhere.  Same-wave LDS accesses
// execute in order, so the slot needs no barrier.
// Physical rows of a lane's logical rows m, m + 8, m + 16, ... through a RowMap without a
// division per row: (g, r) = divmod(m, grp) once, then r += 8 with a carry into g.
struct RowWalk {
  int g, r, grp, off;
  int64_t gstride;
  SDP_DEV RowWalk(const RowMap& rm, int m) : grp(rm.grp), off(rm.off), gstride(rm.gstride) {
    g = (int)((unsigned)m / (unsigned)rm.grp);
    r = m - g * rm.grp;
  }
  SDP_DEV int64_t phys() const { return (int64_t)g * gstride + off + r; }
  SDP_DEV void step8() {
    r += 8;
    while (r >= grp) {  // one pass unless grp < 8
      r -= grp;
      ++g;
    }
  }
};

// f(std::integral_constant<int, I>) for I = B .. E-1, unrolled by construction (a plain
// `#pragma unroll` gives up once the body is large, and the arrays it indexes go to scratch).
template <int B, int E, typename F>
SDP_DEV void static_for(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, E>(f);
  }
}

// TRN 1 / 2 (training epilogues, EPI 5 / 6): rows are staged without an activation and ACT is
// the activation of the training epilogue (-1: epi.act2 at run time).
template <int ACT, int JB = 4, bool ALL = false, int TRN = 0>
SDP_DEV void tile_epilogue_rows(const Epi<bf16_t>& epi, f32x4 (&acc)[4][8], int m0, int n0, int M, int N, int wm,
                                int wn, int lane, int fr, int fq, char* stg) {
  // Ragged tiles take the same arithmetic with masked rows / 8-column chunks
  // (host guarantees N % 8 == 0 and 16-B aligned rows), so a row's result never
  // depends on where the tile boundaries fall (batch invariance).
  const int cbase = n0 + wn * 64 + pair_col0(fq);
  f32x4 bv[2][2], sv[2][2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int c0 = min(cbase + 32 * p, N - 8);
    if (epi.bias) {
      bv[p][0] = *(const f32x4*)(epi.bias + c0);
      bv[p][1] = *(const f32x4*)(epi.bias + c0 + 4);
    } else {
      bv[p][0] = bv[p][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (epi.lnst) {
      sv[p][0] = *(const f32x4*)(epi.lnsum + c0);
      sv[p][1] = *(const f32x4*)(epi.lnsum + c0 + 4);
    } else {
      sv[p][0] = sv[p][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  const int rlo = lane >> 3, ch = lane & 7;
  const int col = n0 + wn * 64 + ch * 8;
  const bool col_ok = col < N;
  const int lcol = col_ok ? col : N - 8;
  const int wchunk0 = ((fq & 1) << 1) | (fq >> 1);  // 16-B chunk of pair 0 (pair 1: +4)
  // the lane's 16 drain rows are mb + 8 i, i = 2 j + q
  const int mb = m0 + wm * 128 + rlo;
  // stage(j): row group j through the permlane pairing, bias / LN fold / activation, bf16
  // pack, into its LDS slot; drain(j, rr): read the slot back in whole-line order, add the
  // residual, store, emit the row partials.  ALL: every row group gets its own 2 KiB
  // slot (stg spans 16 KiB per wave), all eight are staged before the first drain, so the
  // wave pays one LDS round trip instead of eight and issues its 16 stores back to back.
  auto slot = [&](int j) { return ALL ? stg + j * 2048 : stg; };
  auto stage = [&](int j) {
    char* sl = slot(j);
    f32x2 lr2 = {1.f, 1.f}, lm2 = {0.f, 0.f};  // rstd, -rstd * mean of this lane's row (MFMA layout)
    if (epi.lnst) {
      const int mrow = min(m0 + wm * 128 + j * 16 + fr, M - 1);
      const float2 st = *(const float2*)(epi.lnst + 2 * (int64_t)mrow);
      lr2 = f32x2{st.y, st.y};
      lm2 = f32x2{-st.y * st.x, -st.y * st.x};
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      float v[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[2 * p][j][r]),
                                                   __float_as_uint(acc[2 * p + 1][j][r]), false, false);
        v[r] = __uint_as_float(sw[0]);
        v[4 + r] = __uint_as_float(sw[1]);
      }
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; e += 2) {
        const f32x2 b2 = {bv[p][e >> 2][e & 3], bv[p][e >> 2][(e & 3) + 1]};
        f32x2 x2;
        if (epi.lnst) {  // r * acc + (b - r * mean * s)
          const f32x2 s2 = {sv[p][e >> 2][e & 3], sv[p][e >> 2][(e & 3) + 1]};
          x2 = f32x2{v[e], v[e + 1]} * lr2 + (s2 * lm2 + b2);
        } else {
          x2 = f32x2{v[e], v[e + 1]} + b2;
        }
        if constexpr (TRN != 0) {
          // stored pre-activation z: no activation in the staging
        } else if constexpr (ACT == ACT_GELU) {
          x2 = gelu_fast2(x2);
        } else {
          x2.x = epi_act<ACT>(epi.act, x2.x);
          x2.y = epi_act<ACT>(epi.act, x2.y);
        }
        o[e] = (short)f2bf(x2.x);
        o[e + 1] = (short)f2bf(x2.y);
      }
      *(bf16x8*)(sl + fr * 128 + (((4 * p + wchunk0) ^ (fr & 7)) << 4)) = o;
    }
  };
  RowWalk ow(epi.cmap, mb);
  const int64_t part_col = (n0 + wn * 64) >> 6;
  auto drain = [&](int j, const bf16x8(&rr)[2]) {
    const char* sl = slot(j);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int r = rlo + 8 * q;
      bf16x8 o = *(const bf16x8*)(sl + r * 128 + ((ch ^ (r & 7)) << 4));
      const int m = mb + j * 16 + 8 * q;
      if constexpr (TRN == 2) {  // dz = dropout(bf16 dh) * act'(z): sdp_act_bwd's arithmetic on the stored dh
        const float inv = epi.p2 > 0.f ? 1.0f / (1.0f - epi.p2) : 1.0f;
        const uint32_t thr = drop_thresh(epi.p2), key = drop_key(epi.seed2, (uint64_t)m * N + col);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float d = bf2f((bf16_t)o[e]);
          if (epi.p2 > 0.f) d = drop_keep(key, (uint32_t)((uint64_t)m * N + col) + e, thr) ? d * inv : 0.f;
          const int a2 = ACT >= 0 ? ACT : epi.act2;
          o[e] = (short)f2bf(a2 == ACT_NONE ? d : d * act_grad(a2, bf2f((bf16_t)rr[q][e])));
        }
      } else if (epi.resid) {
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (short)f2bf(bf2f((bf16_t)o[e]) + bf2f((bf16_t)rr[q][e]));
      }
      const int64_t prow = ow.phys();
      ow.step8();
      if (m < M && col_ok) {
        bf16x8* dst = (bf16x8*)(epi.out + (uint64_t)prow * (uint32_t)epi.ldc + col);
#ifdef SDP_DIAG
        if (epi.nt_store) __builtin_nontemporal_store(o, dst);  // store-policy experiment (diagnostic build)
        else
#endif
        *dst = o;
      }
      if constexpr (TRN == 1) {  // h = dropout(act(z)) from the stored z: sdp_act_fwd's arithmetic
        const float inv = epi.p2 > 0.f ? 1.0f / (1.0f - epi.p2) : 1.0f;
        const uint32_t thr = drop_thresh(epi.p2), key = drop_key(epi.seed2, (uint64_t)m * N + col);
        bf16x8 h;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float v = apply_act(ACT >= 0 ? ACT : epi.act2, bf2f((bf16_t)o[e]));
          if (epi.p2 > 0.f) v = drop_keep(key, (uint32_t)((uint64_t)m * N + col) + e, thr) ? v * inv : 0.f;
          h[e] = (short)f2bf(v);
        }
        if (m < M && col_ok) *(bf16x8*)(epi.out2 + (uint64_t)m * (uint64_t)epi.ld2 + col) = h;
      }
      if (epi.part) {  // {mean, M2} of the row's 64 stored columns (8 lanes x 8)
        float f[8], sum = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          f[e] = bf2f((bf16_t)o[e]);
          sum += f[e];
        }
        sum += __shfl_xor(sum, 1, 64);
        sum += __shfl_xor(sum, 2, 64);
        sum += __shfl_xor(sum, 4, 64);
        const float mean = sum * (1.0f / 64.0f);
        float m2 = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) m2 = fmaf(f[e] - mean, f[e] - mean, m2);
        m2 += __shfl_xor(m2, 1, 64);
        m2 += __shfl_xor(m2, 2, 64);
        m2 += __shfl_xor(m2, 4, 64);
        if (ch == 0 && m < M && col_ok)
          *(float2*)(epi.part + (prow * (N >> 6) + part_col) * 2) = float2{mean, m2};
      }
    }
  };
  // residual rows: loads for every row group issued before any staging (ALL), so their
  // latency runs under the staging arithmetic; rows past M re-read the last valid row
  bf16x8 rres[ALL ? 8 : JB][2];
  RowWalk rw(epi.rmap, mb);
  int64_t rlast = 0;
  if (epi.resid) {
    const RowWalk rl(epi.rmap, M - 1);
    rlast = rl.phys();
  }
  auto load_res = [&](int jj, int j) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int m = mb + j * 16 + 8 * q;
      const int64_t prow = m < M ? rw.phys() : rlast;
      rw.step8();
      rres[jj][q] = *(const bf16x8*)(epi.resid + (uint64_t)prow * (uint32_t)epi.ldr + lcol);
    }
  };
  if constexpr (ALL) {
    if (epi.resid) static_for<0, 8>([&](auto j) { load_res(j, j); });
    static_for<0, 8>([&](auto j) { stage(j); });
    static_for<0, 8>([&](auto j) { drain(j, rres[j]); });
  } else {
#pragma unroll
    for (int j0 = 0; j0 < 8; j0 += JB) {
      if (epi.resid) {
#pragma unroll
        for (int jj = 0; jj < JB; ++jj) load_res(jj, j0 + jj);
      }
#pragma unroll
      for (int jj = 0; jj < JB; ++jj) {
        stage(j0 + jj);
        drain(j0 + jj, rres[jj]);
      }
    }
  }
}

// Whole-line epilogue of the model's GEMMs with the epilogue flags fixed at compile time
// (FL: EF_BIAS | EF_LN | EF_RESID | EF_PART; same staging and drain order as
// tile_epilogue_rows<ACT, 4, true>).  Differences, all in instruction count: no run-time flag
// branches; output / residual / partial accesses are buffer instructions with 32-bit byte
// offsets walked incrementally per row (the host guarantees every operand's extent < 2 GiB,
// Epi::*_bytes) and rows past M or columns past N get an offset beyond the descriptor's range,
// so the hardware drops those stores instead of a branch per row; the residual add works on
// packed bf16 pairs; the row partials come from the stored bf16 values in two passes (the
// chunk sum by v_dot2c_f32_bf16, then the squared deviations from its mean by packed FMAs),
// each reduced over the row's 8 lanes with DPP adds.  Stored outputs are bit-identical to
// tile_epilogue_rows; the partials agree to fp32 rounding.
enum { EF_BIAS = 1, EF_LN = 2, EF_RESID = 4, EF_PART = 8 };
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2n;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) int i32x2v;
typedef __attribute__((ext_vector_type(4))) int i32x4v;
constexpr uint32_t OFF_DROP = 0x80000000u;  // >= every descriptor range used below

SDP_DEV float dpp_sum8(float v) {  // sum over the 8-lane group (lane & ~7), result in every lane
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, false));
  return v;
}

SDP_DEV uint32_t pack_bf16x2(float lo, float hi) {
  return __builtin_bit_cast(uint32_t, bf16x2n{(__bf16)lo, (__bf16)hi});
}

// o := bf16(o + r) elementwise (8 bf16), in packed fp32 pairs
SDP_DEV u32x4 add_bf16x8(u32x4 ou, u32x4 ru) {
  u32x4 res;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2 a = {__uint_as_float(ou[i] << 16), __uint_as_float(ou[i] & 0xffff0000u)};
    const f32x2 b = {__uint_as_float(ru[i] << 16), __uint_as_float(ru[i] & 0xffff0000u)};
    const f32x2 sm = a + b;
    res[i] = pack_bf16x2(sm.x, sm.y);
  }
  return res;
}

#ifdef SDP_GEMM_STAMPS
// Diagnostic build only (tools/gemm_stamps.py, a separate library): wall-clock stamps of
// workgroup events, 64 per workgroup; stamp = event code << 56 | s_memrealtime (100 MHz).
__device__ unsigned long long g_gemm_stamps[8192 * 64];
__device__ int g_gemm_dephase;  // experiment: first-round workgroup b waits ((b >> 3) & 3) * this many 10-ns ticks
// phase timeline of workgroup 0: waves 0 (group 0) and 4 (group 1), s_memtime (shader clock) at
// each MFMA section's start (after its barrier + lgkmcnt wait) and after its last MFMA issue
__device__ unsigned long long g_phase_stamps[2 * 2 * 64];  // [s_memtime x 2 groups][s_memrealtime x 2 groups]
#define SDP_STAMP(code)                                                                            \
  do {                                                                                             \
    if (tid == 0 && nstamp < 64)                                                                   \
      g_gemm_stamps[(int64_t)b * 64 + nstamp++] =                                                  \
          ((unsigned long long)(code) << 56) | (__builtin_amdgcn_s_memrealtime() & 0xffffffffffffffull); \
  } while (0)
// epilogue sub-phases: slots 40 + code of the workgroup's row, wave 0 only; g_epi_wait = 1 drains
// the wave's memory counters before each stamp (serialises the parts so each one is timed alone)
__device__ int g_epi_wait;
#define SDP_ESTAMP(code)                                                                               \
  do {                                                                                                 \
    if (g_epi_wait) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                        \
    if (threadIdx.x == 0)                                                                              \
      g_gemm_stamps[(int64_t)blockIdx.x * 64 + 40 + (code)] =                                          \
          ((unsigned long long)(0x20 + (code)) << 56) | (__builtin_amdgcn_s_memrealtime() & 0xffffffffffffffull); \
  } while (0)
#else
#define SDP_STAMP(code) do {} while (0)
#define SDP_ESTAMP(code) do {} while (0)
#endif

// byte offset of a lane's rows m, m + 8, m + 16, ... through a RowMap (see RowWalk), 32-bit
struct RowOff {
  uint32_t off, step, wrap;
  int r, grp;
  SDP_DEV RowOff(const RowMap& rm, int m, uint32_t ldb) : grp(rm.grp) {
    const int g = (int)((unsigned)m / (unsigned)rm.grp);
    r = m - g * rm.grp;
    off = (uint32_t)(((int64_t)g * rm.gstride + rm.off + r) * (int64_t)ldb);
    step = 8u * ldb;
    wrap = (uint32_t)((rm.gstride - (int64_t)rm.grp) * (int64_t)ldb);
  }
  SDP_DEV void step8() {  // the host guarantees grp >= 8 (at most one carry per step): branch-free
    r += 8;
    off += step;
    const bool c = r >= grp;
    r = c ? r - grp : r;
    off = c ? off + wrap : off;
  }
};

template <int ACT, int FL>
SDP_DEV void tile_epilogue_fl(const Epi<bf16_t>& epi, f32x4 (&acc)[4][8], int m0, int n0, int M, int N, int wm,
                              int wn, int lane, int fr, int fq, char* stg) {
  constexpr bool HB = FL & EF_BIAS, HL = FL & EF_LN, HR = FL & EF_RESID, HP = FL & EF_PART;
  const int cbase = n0 + wn * 64 + pair_col0(fq);
  f32x4 bv[2][2], sv[2][2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int c0 = min(cbase + 32 * p, N - 8);
    if constexpr (HB || HL) {
      if (epi.bias) {
        bv[p][0] = *(const f32x4*)(epi.bias + c0);
        bv[p][1] = *(const f32x4*)(epi.bias + c0 + 4);
      } else {
        bv[p][0] = bv[p][1] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    if constexpr (HL) {
      sv[p][0] = *(const f32x4*)(epi.lnsum + c0);
      sv[p][1] = *(const f32x4*)(epi.lnsum + c0 + 4);
    }
  }
  const int rlo = lane >> 3, ch = lane & 7;
  const int col = n0 + wn * 64 + ch * 8;
  const bool col_ok = col < N;
  const int wchunk0 = ((fq & 1) << 1) | (fq >> 1);
  const int mb = m0 + wm * 128 + rlo;
  auto stage = [&](int j) {
    char* sl = stg + j * 2048;
    f32x2 lr2 = {1.f, 1.f}, lm2 = {0.f, 0.f};
    if constexpr (HL) {
      const int mrow = min(m0 + wm * 128 + j * 16 + fr, M - 1);
      const float2 st = *(const float2*)(epi.lnst + 2 * (int64_t)mrow);
      lr2 = f32x2{st.y, st.y};
      lm2 = f32x2{-st.y * st.x, -st.y * st.x};
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      float v[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[2 * p][j][r]),
                                                   __float_as_uint(acc[2 * p + 1][j][r]), false, false);
        v[r] = __uint_as_float(sw[0]);
        v[4 + r] = __uint_as_float(sw[1]);
      }
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 8; e += 2) {
        f32x2 x2 = {v[e], v[e + 1]};
        if constexpr (HL) {
          const f32x2 b2 = {bv[p][e >> 2][e & 3], bv[p][e >> 2][(e & 3) + 1]};
          const f32x2 s2 = {sv[p][e >> 2][e & 3], sv[p][e >> 2][(e & 3) + 1]};
          x2 = x2 * lr2 + (s2 * lm2 + b2);
        } else if constexpr (HB) {
          x2 = x2 + f32x2{bv[p][e >> 2][e & 3], bv[p][e >> 2][(e & 3) + 1]};
        }
        if constexpr (ACT == ACT_GELU) {
          x2 = gelu_fast2(x2);
        } else if constexpr (ACT != ACT_NONE) {
          x2.x = epi_act<ACT>(epi.act, x2.x);
          x2.y = epi_act<ACT>(epi.act, x2.y);
        }
        o[e >> 1] = pack_bf16x2(x2.x, x2.y);
      }
      *(u32x4*)(sl + fr * 128 + (((4 * p + wchunk0) ^ (fr & 7)) << 4)) = o;
    }
  };
  const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(epi.out, 0, (int)epi.out_bytes, 0x00020000);
  RowOff ow(epi.cmap, mb, (uint32_t)epi.ldc * 2u);
  const uint32_t colb = (uint32_t)col * 2u;
  [[maybe_unused]] __amdgpu_buffer_rsrc_t prs;
  [[maybe_unused]] uint32_t pcolb = 0;
  RowOff pw(epi.cmap, mb, (uint32_t)(N >> 6) * 8u);  // bytes per physical row of partials
  if constexpr (HP) {
    prs = __builtin_amdgcn_make_buffer_rsrc(epi.part, 0, (int)epi.part_bytes, 0x00020000);
    pcolb = (uint32_t)((n0 + wn * 64) >> 6) * 8u;
  }
  auto drain = [&](int j, const u32x4(&rr)[2], const u32x4(&ov)[2]) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      u32x4 o = ov[q];
      const int m = mb + j * 16 + 8 * q;
      if constexpr (HR) o = add_bf16x8(o, rr[q]);
      const bool ok = m < M && col_ok;
      const uint32_t rowoff = ow.off;
      ow.step8();
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4v, o), ors, ok ? rowoff + colb : OFF_DROP, 0, 0);
      if constexpr (HP) {
        // two passes over the 8 values the lane holds: the chunk mean first (dot2 sum, 8-lane DPP
        // reduction), then the sum of squared deviations -- no sumsq - sum * mean cancellation when
        // a row's |mean| is far above its spread
        const bf16x2n one = {(__bf16)1.0f, (__bf16)1.0f};
        float sm = 0.f;
        uint32_t uv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          // opaque copy: hipcc (ROCm 7.2) miscompiles bit_cast<bf16x2>(u32 vector element) feeding
          // v_dot2c_f32_bf16 (every i reads element 0); a register the compiler cannot see through
          // keeps the element
          uint32_t u = o[i];
          asm volatile("" : "+v"(u));
          uv[i] = u;
          sm = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2n, u), one, sm, false);
        }
        sm = dpp_sum8(sm);
        const float mean = sm * (1.0f / 64.0f);
        const f32x2 mu2 = {mean, mean};
        f32x2 q2 = {0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const f32x2 d = f32x2{__uint_as_float(uv[i] << 16), __uint_as_float(uv[i] & 0xffff0000u)} - mu2;
          q2 = d * d + q2;
        }
        const float m2 = dpp_sum8(q2.x + q2.y);
        // the partials are addressed by the output's physical row (walk pw, nch * 8 B per row)
        const uint32_t poff = pw.off;
        pw.step8();
        // every lane stores (no divergent branch); only the row's first lane has an in-range offset
        __builtin_amdgcn_raw_buffer_store_b64(i32x2v{__float_as_int(mean), __float_as_int(m2)}, prs,
                                              (ok && ch == 0) ? poff + pcolb : OFF_DROP, 0, 0);
      }
    }
  };
  SDP_ESTAMP(0);
  // residual rows j loaded just before stage(j): a wave that issues all 16 loads at once stalls at
  // issue for as long as the memory pipeline takes to accept them (~3.7 us per tile with every CU
  // in its epilogue, tools/gemm_stamps.py); interleaved, the staging VALU runs in that time
  u32x4 rres[8][2];
  [[maybe_unused]] __amdgpu_buffer_rsrc_t rrs;
  RowOff rw(epi.rmap, mb, (uint32_t)epi.ldr * 2u);
  if constexpr (HR) rrs = __builtin_amdgcn_make_buffer_rsrc((void*)epi.resid, 0, (int)epi.res_bytes, 0x00020000);
  static_for<0, 8>([&](auto j) {
    if constexpr (HR) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int m = mb + j * 16 + 8 * q;
        const uint32_t ro = rw.off;
        rw.step8();
        rres[j][q] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rrs, (m < M && col_ok) ? ro + colb : OFF_DROP, 0, 0));
      }
    }
    stage(j);
    if constexpr (HR) __builtin_amdgcn_sched_barrier(0);  // keep each row group's loads before its staging
  });
  SDP_ESTAMP(1);
  SDP_ESTAMP(2);
  // read every staged row back before the first store: one LDS round trip per wave instead of one
  // per row (hipcc keeps an LDS read below any earlier buffer store, which it cannot prove
  // disjoint, so reads placed inside the drain loop wait for the previous row's store)
  u32x4 ov[8][2];
  static_for<0, 8>([&](auto j) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int r = rlo + 8 * q;
      ov[j][q] = *(const u32x4*)(stg + j * 2048 + r * 128 + ((ch ^ (r & 7)) << 4));
    }
  });
  SDP_ESTAMP(3);
  static_for<0, 8>([&](auto j) { drain(j, rres[j], ov[j]); });
#ifdef SDP_GEMM_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  SDP_ESTAMP(4);
}

// EPI: 0 = 8-B stores, 1 = permlane-paired 16-B stores, 2 = no stores (timing probe only)
// ---------------------------------------------------------------------------
// 8-phase ping-pong kernel: 256x256x64 tiles, 8 waves (2 along M x 4 along N,
// 128x64 per wave), two LDS buffers of one K-tile each (X + W = 64 KiB).
//
// A K-tile is consumed in 4 phases, one 64(m) x 32(n) C-quadrant x K=64 each
// (16 MFMAs): Q(m0,n0), Q(m0,n1), Q(m1,n1), Q(m1,n0), so a phase reads 12, 4, 8
// or 0 fragments.  Each phase is
//     ds_read fragments ; issue LDS-DMA ; [counted vmcnt] ; s_barrier ;
//     lgkmcnt(0) ; setprio(1) ; 16 MFMA ; setprio(0) ; s_barrier
// and the wave group wm=1 runs one barrier behind wm=0, so on every SIMD one
// wave is in its MFMA burst while the other issues its LDS reads / DMA.
//
// The K-tile's LDS image is filled in three sub-stages, ordered by first use:
//   S1 = X rows of m-half 0 of both wave groups + W rows of n-half 0 of all waves
//        (read in phase 0; 4 DMA per wave), S2 = W rows of n-half 1 (phase 1; 2),
//   S3 = X rows of m-half 1 (phase 2; 2).
// Schedule (tile t): phase 0 issues S3(t+1), phase 2 S1(t+2), phase 3 S2(t+2).
// With the staggered groups a DMA'd region may be read in phase p only after
// every wave's vmcnt wait in phase p-1, and overwritten in phase p only if its
// last read was in phase <= p-2; the schedule meets both with 5 phases
// (about one K-tile of MFMA time) between issue and retirement:
//   phase 0: vmcnt(10) retires S2(t); phase 1: vmcnt(8) retires S3(t);
//   phase 3: vmcnt(10) retires S1(t+1)   (smaller counts at the K tail).
// ---------------------------------------------------------------------------
constexpr int BUF8 = 2 * TILE_BYTES;

#define SDP_VMCNT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")

// tile index -> (tm, tn).  group_m > 1: indices run down a group of group_m M-blocks
// before moving to the next N-tile, so the tiles an XCD holds at once span ~group_m
// X blocks x 32/group_m W slices instead of 32/tiles_n X blocks x every W slice.
SDP_DEV void tile_coords(int t, int tiles_m, int tiles_n, int group_m, int& tm, int& tn) {
  if (group_m > 1) {
    const int gsz_full = group_m * tiles_n;
    const int g = t / gsz_full, r = t - g * gsz_full;
    const int first = g * group_m;
    const int gm = min(tiles_m - first, group_m);
    tm = first + r % gm;
    tn = r / gm;
  } else {
    tm = t / tiles_n;
    tn = t % tiles_n;
  }
}


// EPI: 1 = permlane-paired register epilogue, 4 = whole-line LDS-staged epilogue.
// PH2 = true: the same K-tile in 2 phases of 32 MFMAs per wave group instead of 4 of 16 (half the
// group-to-group hand-overs; see the k-loop below).
template <int ACT, int EPI, bool PH2 = false>
__global__ __launch_bounds__(NTHREADS) void gemm_bf16_8ph(const bf16_t* __restrict__ X, int64_t ldx, RowMap xmap,
                                                         const bf16_t* __restrict__ W, int64_t ldw, Epi<bf16_t> epi,
                                                         int M, int N, int K, int tiles_m, int tiles_n) {
  // 2 K-tile buffers
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF8];
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  const int fr = lane & 15, fq = lane >> 4;
  const int nk = K / BK;
#ifdef SDP_GEMM_STAMPS
  int nstamp = 0;
#endif
  SDP_STAMP(0);
  if (epi.tline && tid == 0) atomicMin(epi.tline, (unsigned long long)__builtin_amdgcn_s_memrealtime());
#ifdef SDP_GEMM_STAMPS
  if (g_gemm_dephase > 0 && b < 256) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    const unsigned long long w = (unsigned long long)(((b >> 3) & 3) * g_gemm_dephase);
    while (__builtin_amdgcn_s_memrealtime() - t0 < w) __builtin_amdgcn_s_sleep(8);
  }
#endif

  // XCD-aware tile order: consecutive blocks b, b + 8, ... share an XCD (round-robin dispatch), so
  // XCD x = b % 8 takes a contiguous run of the raster (bijective for any tile count)
  int tile;
  {
    const int nwg = tiles_m * tiles_n;
    const int xcd = b & 7, q = nwg >> 3, rem = nwg & 7;
    tile = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (b >> 3);
  }
  const int kb = 0, kn = nk;
  SDP_STAMP(0x10);
  int tm, tn;
  tile_coords(tile, tiles_m, tiles_n, epi.group_m, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;

  // The wave's 8 DMA pieces per K-tile (8 rows x 128 B each): [0,1] S1-X,
  // [2,3] S1-W, [4,5] S2-W, [6,7] S3-X.  Source pointers advance by BK per tile.
  const bf16_t* src[8];
  int loff[8];
  {
    const int rr = lane >> 3, pc = lane & 7;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int idx = wave * 2 + (s & 1);  // 0..15
      int piece;
      bool isx;
      if (s < 2) { piece = idx < 8 ? idx : idx + 8; isx = true; }
      else if (s < 4) { piece = (idx >> 2) * 8 + (idx & 3); isx = false; }
      else if (s < 6) { piece = (idx >> 2) * 8 + 4 + (idx & 3); isx = false; }
      else { piece = idx < 8 ? idx + 8 : idx + 16; isx = true; }
      const int r = piece * 8 + rr;
      const int c = swz(r, pc);
      if (isx) {
        int g = m0 + r;
        g = g < M ? g : M - 1;
        src[s] = X + xmap(g) * ldx + kb * BK + c * 8;
        loff[s] = piece * 1024;
      } else {
        int g = n0 + r;
        g = g < N ? g : N - 1;
        src[s] = W + (int64_t)g * ldw + kb * BK + c * 8;
        loff[s] = TILE_BYTES + piece * 1024;
      }
    }
  }
  auto dma = [&](int s, int kt) {
    __builtin_amdgcn_global_load_lds((const AS1 void*)(src[s] + (int64_t)kt * BK),
                                     (AS3 void*)(smem + (kt & 1) * BUF8 + loff[s]), 16, 0, 0);
  };
  auto S1 = [&](int kt) { dma(0, kt); dma(1, kt); dma(2, kt); dma(3, kt); };
  auto S2 = [&](int kt) { dma(4, kt); dma(5, kt); };
  auto S3 = [&](int kt) { dma(6, kt); dma(7, kt); };

  f32x4 acc[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  bf16x8 xf[8], w0[4], w1[4];
  auto read_x = [&](const char* xt, int jm) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) xf[j * 2 + ks] = lds_frag(xt, wm * 128 + jm * 64 + j * 16 + fr, ks * 4 + fq);
  };
  auto read_w = [&](const char* wt, int in, bf16x8(&wf)[4]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) wf[i * 2 + ks] = lds_frag(wt, wn * 64 + in * 32 + i * 16 + fr, ks * 4 + fq);
  };
  // ks outermost: the two K-halves of one accumulator are 8 MFMAs apart, so no MFMA
  // waits on its predecessor's result (ks innermost made 8 dependent back-to-back pairs)
  auto quad = [&](int jm, int in, const bf16x8(&wf)[4]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[in * 2 + i][jm * 4 + j] =
              __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i * 2 + ks], xf[j * 2 + ks], acc[in * 2 + i][jm * 4 + j], 0, 0, 0);
  };
#ifdef SDP_GEMM_STAMPS
  int pst = 0;
  auto pstamp = [&]() {
    if (b == 0 && (wave & 3) == 0 && lane == 0 && pst < 64)
    {
      g_phase_stamps[(wave >> 2) * 64 + pst] = __builtin_amdgcn_s_memtime();
      if (pst == 0 || pst == 31) g_phase_stamps[128 + (wave >> 2) * 64 + pst] = __builtin_amdgcn_s_memrealtime();
      ++pst;
    }
  };
#else
  auto pstamp = [&]() {};
#endif
  auto mfma_section = [&](auto&& body) {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    pstamp();
    __builtin_amdgcn_s_setprio(1);
    body();
    __builtin_amdgcn_s_setprio(0);
    pstamp();
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };

  if constexpr (PH2) {
    // 2 phases per K-tile: P0 = Q(m0, n0) + Q(m0, n1) (reads w0, w1, xf(m-half 0)), P1 = Q(m1, n1) +
    // Q(m1, n0) (reads xf(m-half 1)), 32 MFMAs per section.  A wave retires its fragment reads
    // (lgkmcnt(0)) BEFORE the section's first barrier, so a region read in phase p may be
    // re-staged from phase p + 1.  Schedule (tile t): P0 issues S3(t+1), P1 issues S1(t+2) S2(t+2);
    // P0 waits vmcnt(8) = retires S3(t) (read in P1), P1 waits vmcnt(8) = retires S1(t+1) S2(t+1)
    // (read in P0 of t+1): two phases (~one K-tile of MFMA) between issue and retirement.
#ifndef SDP_PH2_PRIO
// 1 (default): static priority for wave group 1 (the younger half, the arbitration loser on every
// segment), no per-section flips: M forward 10,099 / 10,107 -> 10,158 / 10,162 img/s over
// per-section flips (0); no s_setprio at all (2) 10,074 / 10,101 (interleaved, tools/r4_prio.sh)
#define SDP_PH2_PRIO 1
#endif
    if (SDP_PH2_PRIO == 1 && __builtin_amdgcn_readfirstlane(wm) == 1) __builtin_amdgcn_s_setprio(1);
    auto section = [&](auto&& body) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      pstamp();
      if (SDP_PH2_PRIO == 0) __builtin_amdgcn_s_setprio(1);
      body();
      if (SDP_PH2_PRIO == 0) __builtin_amdgcn_s_setprio(0);
      pstamp();
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    };
    S1(0); S2(0); S3(0);
    if (kn > 1) { S1(1); S2(1); SDP_VMCNT(8); }
    else SDP_VMCNT(2);
    __builtin_amdgcn_s_barrier();
    if (wm == 1) __builtin_amdgcn_s_barrier();  // stagger group 1 by one barrier
    SDP_STAMP(4);
    __builtin_amdgcn_sched_barrier(0);
    for (int t = 0; t < kn; ++t) {
      const char* xt = smem + (t & 1) * BUF8;
      const char* wt = xt + TILE_BYTES;
      const bool more1 = t + 1 < kn, more2 = t + 2 < kn;
      read_w(wt, 0, w0);
      read_w(wt, 1, w1);
      read_x(xt, 0);
      if (more1) { S3(t + 1); SDP_VMCNT(8); } else SDP_VMCNT(0);
      section([&] { quad(0, 0, w0); quad(0, 1, w1); });
      read_x(xt, 1);
      if (more2) { S1(t + 2); S2(t + 2); SDP_VMCNT(8); }
      else if (more1) SDP_VMCNT(2);
      section([&] { quad(1, 1, w1); quad(1, 0, w0); });
    }
  } else {
  // prologue: S1(0) S2(0) S3(0) [S1(1) S2(1)]; retire S1(0)
  S1(0); S2(0); S3(0);
  if (kn > 1) { S1(1); S2(1); SDP_VMCNT(10); }
  else SDP_VMCNT(4);
  __builtin_amdgcn_s_barrier();
  if (wm == 1) __builtin_amdgcn_s_barrier();  // stagger group 1 by one barrier
  SDP_STAMP(4);
  __builtin_amdgcn_sched_barrier(0);

  for (int t = 0; t < kn; ++t) {
    const char* xt = smem + (t & 1) * BUF8;
    const char* wt = xt + TILE_BYTES;
    const bool more1 = t + 1 < kn, more2 = t + 2 < kn;
    // phase 0: Q(m0, n0)
    read_w(wt, 0, w0);
    read_x(xt, 0);
    if (more1) { S3(t + 1); SDP_VMCNT(10); } else SDP_VMCNT(2);
    mfma_section([&] { quad(0, 0, w0); });
    // phase 1: Q(m0, n1)
    read_w(wt, 1, w1);
    if (more1) SDP_VMCNT(8); else SDP_VMCNT(0);
    mfma_section([&] { quad(0, 1, w1); });
    // phase 2: Q(m1, n1)
    read_x(xt, 1);
    if (more2) S1(t + 2);
    mfma_section([&] { quad(1, 1, w1); });
    // phase 3: Q(m1, n0)
    if (more2) { S2(t + 2); SDP_VMCNT(10); }
    else if (more1) SDP_VMCNT(4);
    mfma_section([&] { quad(1, 0, w0); });
  }
  }  // !PH2
  if (wm == 0) __builtin_amdgcn_s_barrier();  // balance the stagger
  SDP_STAMP(5);
  if constexpr (EPI == 4) {  // whole-line epilogue, all eight row groups staged first (16 KiB
    // per wave: both K buffers, free once the balancing barrier above has passed); the host
    // routes resid_pre-with-activation and unaligned calls to EPI 1
    tile_epilogue_rows<ACT, 4, true>(epi, acc, m0, n0, M, N, wm, wn, lane, fr, fq, smem + wave * 16384);
  } else if constexpr (EPI >= 16) {  // whole-line epilogue with compile-time flags (EPI - 16)
    tile_epilogue_fl<ACT, EPI - 16>(epi, acc, m0, n0, M, N, wm, wn, lane, fr, fq, smem + wave * 16384);
  } else if constexpr (EPI == 5 || EPI == 6) {  // training epilogues (same staging)
    tile_epilogue_rows<ACT, 4, true, EPI - 4>(epi, acc, m0, n0, M, N, wm, wn, lane, fr, fq, smem + wave * 16384);
  } else {
    tile_epilogue16<ACT>(epi, acc, m0, n0, M, N, wm, wn, fr, fq);
  }
  SDP_STAMP(6);
  if (epi.tline) {  // end of this workgroup: its stores have left (timeline runs only)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (tid == 0) atomicMax(epi.tline + 1, (unsigned long long)__builtin_amdgcn_s_memrealtime());
  }
}

#ifdef SDP_DIAG  // measured slower than gemm_bf16_8ph (round 6): diagnostic build only
// ---------------------------------------------------------------------------
// Cross-tile kernel (gemm_bf16_ct): the two 4-wave groups of a 512-thread workgroup own DIFFERENT
// output tiles and run half a tile period apart, so one group's epilogue (GELU / LN fold / residual
// / stores / LN partials) executes while the other group issues MFMAs on the same SIMDs.
// gemm_bf16_8ph's two groups share one 256 x 256 tile and reach its epilogue together: every CU's
// matrix pipes idle for the whole epilogue (4.5-11 us of a ~28-33 us K = 768 tile, round-5 stamps).
//
// Workgroup = a run of T consecutive 256 x 256 "pair" tiles of the raster; group g computes the
// 128 x 256 half [m0 + 128 g, m0 + 128 g + 128) of each (gemm_bf16_8ph's wave-group split), wave
// wn = 0..3 its 128 x 64 column slice (same acc[4][8] layout, same MFMA, same per-accumulator k
// order, same epilogue arithmetic: outputs are bit-identical to gemm_bf16_8ph).  Splitting M keeps
// the large operand X read once per pair tile; only the small weight panel is staged twice (a
// 256 x 128 split doubled the X traffic and ran the K = 3072 shapes at half speed).  Each group
// streams its operands through its own 3-slot LDS ring of 32-deep K-steps (X 128 x 32 + W 256 x 32
// bf16 = 24 KiB per slot, 2 x 72 KiB in all), two steps ahead across tile boundaries, so the next
// tile's first K-steps land during the epilogue (no prologue on the critical path).
//
// Schedule: every K-step of a group is  [load phase: fragment reads of step g, DMA of step g + 2,
// vmcnt retiring step g + 1] [section: barrier, 32 MFMAs, barrier]; group 1 runs one barrier behind
// group 0 (as in gemm_bf16_8ph), so one group's load phase lies under the other's MFMA section.  An
// epilogue step keeps that barrier pattern: its VALU-heavy half (residual loads, staging through LDS
// with bias / LN fold / activation) lies under the partner's MFMA section, its store half under the
// partner's load phase.  Group 1 additionally starts E steps (one epilogue) late and group 0 pads its
// end by the same amount, so their epilogues alternate.  Both groups execute the same barrier count
// (2 + 2 E + 2 T (S + E)), all control flow is wave-uniform.
//
// LDS ring slot: [128 X rows][32 bf16] then [256 W rows][32 bf16], 64-B rows; 16-B chunk c of row r
// stored at c ^ h((r >> 2) & 3), h = {0, 2, 3, 1}: each 16-lane group of a ds_read_b128 fragment
// read hits 16 distinct 16-B bank slots.  One LDS-DMA instruction fills 16 rows (1 KiB).
// ---------------------------------------------------------------------------
namespace ctk {
constexpr int GBM = 128, CBN = 256, CBK = 32;
constexpr int XSB = GBM * CBK * 2;  // 8 KiB
constexpr int WSB = CBN * CBK * 2;  // 16 KiB
constexpr int SLOT = XSB + WSB;    // 24 KiB
constexpr int RING = 3 * SLOT;     // 72 KiB per group
SDP_DEV int hsw(int r) { return (0x78 >> (2 * ((r >> 2) & 3))) & 3; }
}  // namespace ctk

template <int ACT, int FL, int RE>
__global__ __launch_bounds__(NTHREADS) void gemm_bf16_ct(const bf16_t* __restrict__ X, int64_t ldx, RowMap xmap,
                                                        const bf16_t* __restrict__ W, int64_t ldw, Epi<bf16_t> epi,
                                                        int M, int N, int K, int tiles_m, int tiles_n, int T) {
  using namespace ctk;
  constexpr bool HB = FL & EF_BIAS, HL = FL & EF_LN, HR = FL & EF_RESID, HP = FL & EF_PART;
  constexpr int E = 8 / RE;  // epilogue steps per tile
  static_assert(8 % RE == 0 && RE * 2048 * 4 <= SLOT, "epilogue staging must fit one ring slot");
  __shared__ __attribute__((aligned(16))) char smem[2 * RING];
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wave >> 2, w4 = wave & 3, wn = w4;
  constexpr int wm = 0;  // a group's 128 rows are one wave row
  const int fr = lane & 15, fq = lane >> 4;
  char* const ring = smem + grp * RING;
  if (epi.tline && tid == 0) atomicMin(epi.tline, (unsigned long long)__builtin_amdgcn_s_memrealtime());

  // this workgroup's run of pair tiles (XCD-aware: blocks b, b + 8, ... share an XCD and take a
  // contiguous stretch of runs)
  int wgi;
  {
    const int nwg = gridDim.x, xcd = b & 7, q = nwg >> 3, rem = nwg & 7;
    wgi = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (b >> 3);
  }
  const int p0 = wgi * T;
  const int Tw = min(T, tiles_m * tiles_n - p0);  // >= 1 (host: grid = ceil(pairs / T))
  const int S = K / CBK;                          // K-steps per tile (>= 2)
  const int nsteps = Tw * S;
  // group 1's offset: E steps is the least that puts every epilogue of one group beside K-steps of the
  // other (group 0's tile-t epilogue beside group 1's last E K-steps of tile t, group 1's beside group
  // 0's first E K-steps of tile t + 1); a larger offset only lengthens the workgroup's unpaired start
  // and end
  const int padB = E;
  auto tile_origin = [&](int p, int& m0, int& n0) {
    int tm, tn;
    tile_coords(p, tiles_m, tiles_n, epi.group_m, tm, tn);
    m0 = tm * (2 * GBM) + grp * GBM;
    n0 = tn * CBN;
  };

  // ---- LDS-DMA: per wave 2 X pieces (rows 16 (w4 + 4 i) ..) and 4 W pieces per K-step
  const int prow = lane >> 2;
  const int pcol = ((lane & 3) ^ hsw(prow)) * 8;  // logical element offset this lane loads
  const bf16_t* xsrc[2];
  const bf16_t* wsrc[4];
  int f_ks = 0, f_tile = 0, f_slot = 0;  // fetch cursor: K-step in tile, tile index, ring slot
  auto fetch = [&]() {
    if (f_ks == 0) {
      int m0, n0;
      tile_origin(p0 + f_tile, m0, n0);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int r = min(m0 + (w4 + 4 * i) * 16 + prow, M - 1);
        xsrc[i] = X + xmap(r) * ldx + pcol;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = min(n0 + (w4 + 4 * i) * 16 + prow, N - 1);
        wsrc[i] = W + (int64_t)r * ldw + pcol;
      }
    }
    char* slot = ring + f_slot * SLOT;
    const int64_t ko = (int64_t)f_ks * CBK;
#pragma unroll
    for (int i = 0; i < 2; ++i)
      __builtin_amdgcn_global_load_lds((const AS1 void*)(xsrc[i] + ko), (AS3 void*)(slot + (w4 + 4 * i) * 1024), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_global_load_lds((const AS1 void*)(wsrc[i] + ko), (AS3 void*)(slot + XSB + (w4 + 4 * i) * 1024),
                                       16, 0, 0);
    if (++f_ks == S) { f_ks = 0; ++f_tile; }
    f_slot = f_slot == 2 ? 0 : f_slot + 1;
  };

  // ---- fragments and MFMAs (gemm_bf16_8ph's D[n][m] layout: A = W rows, B = X rows)
  const int loff = fr * 64 + ((fq ^ hsw(fr)) << 4);
  f32x4 acc[4][8];
  bf16x8 xf[8], wf[4];
  auto read_frags = [&](const char* slot) {
#pragma unroll
    for (int i = 0; i < 4; ++i) wf[i] = *(const bf16x8*)(slot + XSB + (wn * 64 + i * 16) * 64 + loff);
#pragma unroll
    for (int j = 0; j < 8; ++j) xf[j] = *(const bf16x8*)(slot + (j * 16) * 64 + loff);
  };
  auto bar = [] {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };

  // group 1 is the younger half of every SIMD pair: static priority (gemm_bf16_8ph, SDP_PH2_PRIO 1)
  if (grp == 1) __builtin_amdgcn_s_setprio(1);

  // prologue: K-steps 0 and 1 of the first tile; retire step 0
  fetch();
  fetch();
  SDP_VMCNT(6);
  bar();
  if (grp == 1) {  // one barrier behind, and half a tile period late
    bar();
    for (int i = 0; i < padB; ++i) { bar(); bar(); }
  }
  int fetched = 2, cslot = 0;
  for (int t = 0; t < Tw; ++t) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < S; ++ks) {
      // load phase: DMA of step g + 2 (into the slot step g - 1 used), fragment reads of step g
      const bool more = fetched < nsteps;
      if (more) {
        fetch();
        ++fetched;
      }
      read_frags(ring + cslot * SLOT);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      bar();
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i], xf[j], acc[i][j], 0, 0, 0);
      // retire step g + 1 (the next load phase reads it) behind the MFMAs: its DMA had the whole load
      // phase and section of step g to land; the closing barrier then publishes it to the group
      __builtin_amdgcn_sched_barrier(0);
      if (more) SDP_VMCNT(6);
      else SDP_VMCNT(0);
      bar();
      cslot = cslot == 2 ? 0 : cslot + 1;
    }

    // ---- epilogue of this tile (tile_epilogue_fl's arithmetic, RE row groups per step); the
    // staging area is the ring slot of the tile's last K-step, free once its section ended
    char* const stg = ring + (cslot == 0 ? 2 : cslot - 1) * SLOT + w4 * (RE * 2048);
    int m0, n0;
    tile_origin(p0 + t, m0, n0);
    const int cbase = n0 + wn * 64 + pair_col0(fq);
    f32x4 bv[2][2], sv[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int c0 = min(cbase + 32 * p, N - 8);
      if constexpr (HB || HL) {
        if (epi.bias) {
          bv[p][0] = *(const f32x4*)(epi.bias + c0);
          bv[p][1] = *(const f32x4*)(epi.bias + c0 + 4);
        } else {
          bv[p][0] = bv[p][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
      if constexpr (HL) {
        sv[p][0] = *(const f32x4*)(epi.lnsum + c0);
        sv[p][1] = *(const f32x4*)(epi.lnsum + c0 + 4);
      }
    }
    const int rlo = lane >> 3, ch = lane & 7;
    const int col = n0 + wn * 64 + ch * 8;
    const bool col_ok = col < N;
    const int wchunk0 = ((fq & 1) << 1) | (fq >> 1);
    const int mb = m0 + wm * 128 + rlo;
    const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(epi.out, 0, (int)epi.out_bytes, 0x00020000);
    RowOff ow(epi.cmap, mb, (uint32_t)epi.ldc * 2u);
    const uint32_t colb = (uint32_t)col * 2u;
    [[maybe_unused]] __amdgpu_buffer_rsrc_t prs;
    [[maybe_unused]] uint32_t pcolb = 0;
    RowOff pw(epi.cmap, mb, (uint32_t)(N >> 6) * 8u);
    if constexpr (HP) {
      prs = __builtin_amdgcn_make_buffer_rsrc(epi.part, 0, (int)epi.part_bytes, 0x00020000);
      pcolb = (uint32_t)((n0 + wn * 64) >> 6) * 8u;
    }
    [[maybe_unused]] __amdgpu_buffer_rsrc_t rrs;
    RowOff rw(epi.rmap, mb, (uint32_t)epi.ldr * 2u);
    if constexpr (HR) rrs = __builtin_amdgcn_make_buffer_rsrc((void*)epi.resid, 0, (int)epi.res_bytes, 0x00020000);
    u32x4 rres[RE][2];
    static_for<0, E>([&](auto e) {
      // half 1 (under the partner group's MFMA section): residual loads, staging
      static_for<0, RE>([&](auto jj) {
        constexpr int j = decltype(e)::value * RE + decltype(jj)::value;
        if constexpr (HR) {
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const int m = mb + j * 16 + 8 * q;
            const uint32_t ro = rw.off;
            rw.step8();
            rres[jj][q] = __builtin_bit_cast(
                u32x4, __builtin_amdgcn_raw_buffer_load_b128(rrs, (m < M && col_ok) ? ro + colb : OFF_DROP, 0, 0));
          }
        }
        char* sl = stg + jj * 2048;
        f32x2 lr2 = {1.f, 1.f}, lm2 = {0.f, 0.f};
        if constexpr (HL) {
          const int mrow = min(m0 + wm * 128 + j * 16 + fr, M - 1);
          const float2 st = *(const float2*)(epi.lnst + 2 * (int64_t)mrow);
          lr2 = f32x2{st.y, st.y};
          lm2 = f32x2{-st.y * st.x, -st.y * st.x};
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          float v[8];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[2 * p][j][r]),
                                                       __float_as_uint(acc[2 * p + 1][j][r]), false, false);
            v[r] = __uint_as_float(sw[0]);
            v[4 + r] = __uint_as_float(sw[1]);
          }
          u32x4 o;
#pragma unroll
          for (int e2 = 0; e2 < 8; e2 += 2) {
            f32x2 x2 = {v[e2], v[e2 + 1]};
            if constexpr (HL) {
              const f32x2 b2 = {bv[p][e2 >> 2][e2 & 3], bv[p][e2 >> 2][(e2 & 3) + 1]};
              const f32x2 s2 = {sv[p][e2 >> 2][e2 & 3], sv[p][e2 >> 2][(e2 & 3) + 1]};
              x2 = x2 * lr2 + (s2 * lm2 + b2);
            } else if constexpr (HB) {
              x2 = x2 + f32x2{bv[p][e2 >> 2][e2 & 3], bv[p][e2 >> 2][(e2 & 3) + 1]};
            }
            if constexpr (ACT == ACT_GELU) {
              x2 = gelu_fast2(x2);
            } else if constexpr (ACT != ACT_NONE) {
              x2.x = epi_act<ACT>(epi.act, x2.x);
              x2.y = epi_act<ACT>(epi.act, x2.y);
            }
            o[e2 >> 1] = pack_bf16x2(x2.x, x2.y);
          }
          *(u32x4*)(sl + fr * 128 + (((4 * p + wchunk0) ^ (fr & 7)) << 4)) = o;
        }
      });
      bar();
      // half 2 (under the partner's load phase): read back whole lines, residual add, stores, partials
      static_for<0, RE>([&](auto jj) {
        constexpr int j = decltype(e)::value * RE + decltype(jj)::value;
        const char* sl = stg + jj * 2048;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int r = rlo + 8 * q;
          u32x4 o = *(const u32x4*)(sl + r * 128 + ((ch ^ (r & 7)) << 4));
          const int m = mb + j * 16 + 8 * q;
          if constexpr (HR) o = add_bf16x8(o, rres[jj][q]);
          const bool ok = m < M && col_ok;
          const uint32_t rowoff = ow.off;
          ow.step8();
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4v, o), ors, ok ? rowoff + colb : OFF_DROP, 0, 0);
          if constexpr (HP) {
            const bf16x2n one = {(__bf16)1.0f, (__bf16)1.0f};
            float sm = 0.f;
            uint32_t uv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              uint32_t u = o[i];
              asm volatile("" : "+v"(u));  // see tile_epilogue_fl (hipcc dot2 operand miscompile)
              uv[i] = u;
              sm = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2n, u), one, sm, false);
            }
            sm = dpp_sum8(sm);
            const float mean = sm * (1.0f / 64.0f);
            const f32x2 mu2 = {mean, mean};
            f32x2 q2 = {0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const f32x2 d = f32x2{__uint_as_float(uv[i] << 16), __uint_as_float(uv[i] & 0xffff0000u)} - mu2;
              q2 = d * d + q2;
            }
            const float m2 = dpp_sum8(q2.x + q2.y);
            const uint32_t poff = pw.off;
            pw.step8();
            __builtin_amdgcn_raw_buffer_store_b64(i32x2v{__float_as_int(mean), __float_as_int(m2)}, prs,
                                                  (ok && ch == 0) ? poff + pcolb : OFF_DROP, 0, 0);
          }
        }
      });
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      bar();
    });
  }
  if (grp == 0) {  // the same barrier count as group 1
    bar();
    for (int i = 0; i < padB; ++i) { bar(); bar(); }
  }
  if (epi.tline) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (tid == 0) atomicMax(epi.tline + 1, (unsigned long long)__builtin_amdgcn_s_memrealtime());
  }
}

#endif  // SDP_DIAG (gemm_bf16_ct)

#undef SDP_VMCNT

}  // namespace fast

// ---------------------------------------------------------------------------
// Generic masked kernel (fp32 exact-MFMA path and odd bf16 shapes).
// 64x64 tile, BK=32, 4 waves (2x2, 32x32 each), register-staged LDS.
// ---------------------------------------------------------------------------
namespace gen {
constexpr int BM = 64, BN = 64, BK = 32, PAD = 8, LDK = BK + PAD;

template <typename T>
__global__ __launch_bounds__(256) void gemm_generic(const T* __restrict__ X, int64_t ldx, RowMap xmap,
                                                    const T* __restrict__ W, int64_t ldw, Epi<T> epi,
                                                    int M, int N, int K) {
  __shared__ __attribute__((aligned(16))) T xs[BM * LDK];
  __shared__ __attribute__((aligned(16))) T ws[BN * LDK];
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < K; k0 += BK) {
#pragma unroll
    for (int it = 0; it < (BM * BK) / 256; ++it) {
      const int idx = tid + it * 256;
      const int r = idx / BK, c = idx % BK;
      const int gm = m0 + r, gn = n0 + r, gk = k0 + c;
      T xv = from_f<T>(0.f), wv = from_f<T>(0.f);
      if (gm < M && gk < K) xv = X[xmap(gm) * ldx + gk];
      if (gn < N && gk < K) wv = W[(int64_t)gn * ldw + gk];
      xs[r * LDK + c] = xv;
      ws[r * LDK + c] = wv;
    }
    __syncthreads();
    if constexpr (sizeof(T) == 2) {
      bf16x8 bx[2], aw[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) bx[j] = *(const bf16x8*)&xs[(wm * 32 + j * 16 + fr) * LDK + fq * 8];
#pragma unroll
      for (int i = 0; i < 2; ++i) aw[i] = *(const bf16x8*)&ws[(wn * 32 + i * 16 + fr) * LDK + fq * 8];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw[i], bx[j], acc[i][j], 0, 0, 0);
    } else {
#pragma unroll
      for (int kk = 0; kk < BK; kk += 4) {
        float bx[2], aw[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) bx[j] = xs[(wm * 32 + j * 16 + fr) * LDK + kk + fq];
#pragma unroll
        for (int i = 0; i < 2; ++i) aw[i] = ws[(wn * 32 + i * 16 + fr) * LDK + kk + fq];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[i], bx[j], acc[i][j], 0, 0, 0);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = m0 + wm * 32 + j * 16 + fr;
    if (m >= M) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int n = n0 + wn * 32 + i * 16 + fq * 4;
      if (n < N) epi_store4<T>(epi, m, n, N, acc[i][j]);
    }
  }
}
}  // namespace gen

// ---------------------------------------------------------------------------
// Small-M kernel (opt-in, sdp_gemm_splitk): bf16, BM x 64 x 64 tiles over one K-slice.
// The 256x256 kernel gives a 196-row GEMM 3..12 workgroups, each walking the whole K; here the
// grid is ceil(M/BM) x N/64 x S, every workgroup a BM x 64 output tile over one of S slices of
// whole 64-wide K-tiles (slice sizes differ by at most one tile).  4 waves (2 along M x 2 along
// N), v_mfma_f32_16x16x32_bf16 issued swapped as above; both operands go HBM -> registers ->
// ds_write_b128 into the XOR-swizzled [row][64] image of the hot kernel (full 128-B rows per 8
// lanes), double buffered, one barrier per K-tile, the next tile's global loads in flight under
// the current tile's MFMAs.
// S == 1: the fp32 tile goes through LDS to the row epilogue below.  S > 1: every slice stores
// its fp32 slab ws[s][m][n] and splitk_reduce (a second launch: nothing inside a launch waits on
// another workgroup) sums the slabs in slice order and runs the same epilogue, so the result
// does not depend on the order workgroups run in.
// ---------------------------------------------------------------------------
namespace small {
constexpr int BN = 64, BK = 64, NTHREADS = 256;
constexpr int TLD = BN + 4;  // fp32 tile row stride in LDS (floats; rows stay 16-B aligned)

// Epilogue of 4 consecutive columns n..n+3 of logical row m; the 16 lanes l..l+15 (l % 16 == 0) of
// a wave hold the row's 64-column chunk.  One rounding: bf16(act(acc + b [+ R]) [+ R]) (kernel 9's
// arithmetic).  part: {mean, M2} of the 64 stored bf16 values in two passes (sum, then squared
// deviations from its mean), the whole-line epilogue's layout.  Rows past M come in clamped with
// row_ok = false: they take part in the shuffles and store nothing.
SDP_DEV void row_epilogue(const Epi<bf16_t>& e, int m, bool row_ok, int n, int N, f32x4 acc, int fast_gelu) {
  float v[4] = {acc[0], acc[1], acc[2], acc[3]};
  const f32x4 bv = e.bias ? *(const f32x4*)(e.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
  if (e.lnst) {
    const float2 st = *(const float2*)(e.lnst + 2 * (int64_t)m);
    const float rmu = st.y * st.x;
    const f32x4 sv = *(const f32x4*)(e.lnsum + n);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = ln_fold(v[r], st.y, rmu, sv[r], bv[r]);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += bv[r];
  }
  float rv[4] = {0.f, 0.f, 0.f, 0.f};
  if (e.resid) {
    const bf16x4 rr = *(const bf16x4*)(e.resid + e.rmap(m) * e.ldr + n);
#pragma unroll
    for (int r = 0; r < 4; ++r) rv[r] = bf2f((bf16_t)rr[r]);
  }
  if (e.resid && e.resid_pre) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += rv[r];
  }
  if (e.act != ACT_NONE) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = fast_gelu ? gelu_fast(v[r]) : apply_act(e.act, v[r]);
  }
  if (e.resid && !e.resid_pre) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += rv[r];
  }
  bf16x4 o;
#pragma unroll
  for (int r = 0; r < 4; ++r) o[r] = (short)f2bf(v[r]);
  const int64_t prow = e.cmap(m);
  if (row_ok) *(bf16x4*)(e.out + prow * e.ldc + n) = o;
  if (e.part) {
    float f[4], sum = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      f[r] = bf2f((bf16_t)o[r]);
      sum += f[r];
    }
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) sum += __shfl_xor(sum, d, 64);
    const float mean = sum * (1.0f / 64.0f);
    float m2 = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) m2 = fmaf(f[r] - mean, f[r] - mean, m2);
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) m2 += __shfl_xor(m2, d, 64);
    if (row_ok && (threadIdx.x & 15) == 0)
      *(float2*)(e.part + (prow * (N >> 6) + (n >> 6)) * 2) = float2{mean, m2};
  }
}

template <int BM>
__global__ __launch_bounds__(NTHREADS) void gemm_bf16_splitk(const bf16_t* __restrict__ X, int64_t ldx, RowMap xmap,
                                                             const bf16_t* __restrict__ W, int64_t ldw,
                                                             Epi<bf16_t> epi, float* __restrict__ ws, int M, int N,
                                                             int K, int S, int fast_gelu) {
  constexpr int MT = BM / 32;  // 16-row m-tiles per wave = 32-row load passes per workgroup
  constexpr int XT = BM * 128, STAGE = XT + BN * 128;
  static_assert(BM * TLD * 4 <= 2 * STAGE, "the fp32 tile reuses the operand stages");
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN, sl = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, fr = lane & 15, fq = lane >> 4;
  // this slice's K-tiles: [t0, t0 + nt)
  const int kt = K / BK, tb = kt / S, trem = kt % S;
  const int t0 = sl * tb + min(sl, trem), nt = tb + (sl < trem ? 1 : 0);

  // loads: thread -> 16-B chunk lc of rows lr + 32 i (8 lanes cover a row's 128 B); rows past M
  // re-read row M - 1 (their results are never stored)
  const int lc = tid & 7, lr = tid >> 3;
  const bf16_t* xp[MT];
  const bf16_t* wp[2];
#pragma unroll
  for (int i = 0; i < MT; ++i) xp[i] = X + xmap(min(m0 + lr + 32 * i, M - 1)) * ldx + (int64_t)t0 * BK + lc * 8;
#pragma unroll
  for (int i = 0; i < 2; ++i) wp[i] = W + (int64_t)(n0 + lr + 32 * i) * ldw + (int64_t)t0 * BK + lc * 8;
  bf16x8 xr[MT], wr[2];
  auto gload = [&](int t) {
#pragma unroll
    for (int i = 0; i < MT; ++i) xr[i] = *(const bf16x8*)(xp[i] + t * BK);
#pragma unroll
    for (int i = 0; i < 2; ++i) wr[i] = *(const bf16x8*)(wp[i] + t * BK);
  };
  auto lstore = [&](char* st) {
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int r = lr + 32 * i;
      *(bf16x8*)(st + r * 128 + fast::swz(r, lc) * 16) = xr[i];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = lr + 32 * i;
      *(bf16x8*)(st + XT + r * 128 + fast::swz(r, lc) * 16) = wr[i];
    }
  };

  f32x4 acc[2][MT];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  gload(0);
  lstore(lds);
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const char* st = lds + (t & 1) * STAGE;
    if (t + 1 < nt) gload(t + 1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 aw[2], bx[MT];
#pragma unroll
      for (int i = 0; i < 2; ++i) aw[i] = fast::lds_frag(st + XT, wn * 32 + i * 16 + fr, kk * 4 + fq);
#pragma unroll
      for (int j = 0; j < MT; ++j) bx[j] = fast::lds_frag(st, wm * (BM / 2) + j * 16 + fr, kk * 4 + fq);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw[i], bx[j], acc[i][j], 0, 0, 0);
    }
    // the other stage was last read in iteration t - 1, which every wave left through the barrier
    if (t + 1 < nt) lstore(lds + ((t + 1) & 1) * STAGE);
    __syncthreads();
  }

  // D[n][m]: the lane holds n = .. + 4 fq + r, m = .. + fr
  if (S > 1) {
    float* slab = ws + (int64_t)sl * M * N;
#pragma unroll
    for (int j = 0; j < MT; ++j) {
      const int m = m0 + wm * (BM / 2) + j * 16 + fr;
      if (m >= M) continue;
#pragma unroll
      for (int i = 0; i < 2; ++i)
        *(f32x4*)(slab + (int64_t)m * N + n0 + wn * 32 + i * 16 + fq * 4) = acc[i][j];
    }
    return;
  }
  float* tile = (float*)lds;  // every wave is past the K-loop's last barrier
#pragma unroll
  for (int j = 0; j < MT; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i)
      *(f32x4*)(tile + (wm * (BM / 2) + j * 16 + fr) * TLD + wn * 32 + i * 16 + fq * 4) = acc[i][j];
  __syncthreads();
  const int g = tid >> 4, l = tid & 15;
  for (int p = 0; p < BM / 16; ++p) {
    const int row = p * 16 + g, m = m0 + row;
    row_epilogue(epi, min(m, M - 1), m < M, n0 + l * 4, N, *(const f32x4*)(tile + row * TLD + l * 4), fast_gelu);
  }
}

// Sum of the S slabs in slice order 0 .. S-1 (fp32), then the row epilogue: 16 rows x one
// 64-column chunk per workgroup, 16 lanes x 4 columns per row.
__global__ __launch_bounds__(NTHREADS) void splitk_reduce(const float* __restrict__ ws, Epi<bf16_t> epi, int M, int N,
                                                          int S, int fast_gelu) {
  const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
  const int m = blockIdx.x * 16 + g, n = blockIdx.y * BN + l * 4;
  const int mc = min(m, M - 1);
  const float* p = ws + (int64_t)mc * N + n;
  const int64_t slab = (int64_t)M * N;
  f32x4 a = *(const f32x4*)p;
  for (int s = 1; s < S; ++s) a += *(const f32x4*)(p + s * slab);
  row_epilogue(epi, mc, m < M, n, N, a, fast_gelu);
}
}  // namespace small

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
static RowMap mk_map(int grp, int64_t gstride, int off) {
  RowMap r;
  r.grp = grp > 0 ? grp : 0x7fffffff;
  r.gstride = grp > 0 ? gstride : 0;
  r.off = grp > 0 ? off : 0;
  return r;
}

// Returns the kernel variant chosen for the shape (for tests / profiling).
extern "C" int sdp_gemm_variant(int dtype, int M, int N, int K) {
  if (dtype == 1 && K % fast::BK == 0 && K >= fast::BK && M >= 128 && N >= 128) return 1;
  return 0;
}

static int g_force_generic = 0;
extern "C" int sdp_gemm_force_generic(int on) {
  int old = g_force_generic;
  g_force_generic = on;
  return old;
}

// bf16 fast-kernel selection: 14 (default) = 8-phase ping-pong 256x256 with the whole-line
// LDS-staged epilogue (every row group staged before the first store); 9 = the same main
// loop with the permlane-paired 16-B register epilogue (also the fallback for unaligned /
// resid_pre-with-activation calls).
static int g_fast_kernel = 14;
extern "C" int sdp_gemm_set_fast_kernel(int k) {  // 0 queries; an unknown id returns -1
  const int old = g_fast_kernel;
  if (k == 0) return old;
  if (k != 9 && k != 14) return -1;
  g_fast_kernel = k;
  return old;
}

// -1 = auto: groups of 2 M-blocks below 9 N-tiles (N = 768), 4 from 9 (round 6: against 8 from 12
// N-tiles and row-major below, 4 everywhere gave the M forward +0.4 % and the XL forward +1.4 %, then
// 2 for the narrow shapes another +0.4 % over five interleaved pairs; profiles/r06_gemm_raster_ab.md)
static int g_group_m = -1;
static inline int auto_group_m(int tiles_n) { return tiles_n < 9 ? 2 : 4; }
extern "C" int sdp_gemm_set_group_m(int gm) {
  int old = g_group_m;
  g_group_m = gm;
  return old;
}

int g_exact_gelu = 0;  // also read by mx.hip
extern "C" int sdp_gemm_set_exact_gelu(int on) {
  int old = g_exact_gelu;
  g_exact_gelu = on ? 1 : 0;
  return old;
}

// Launch timeline (bench.py): while a buffer is set, fast-GEMM launch i gets slot i of it
// ({start, end} u64 pair) until `slots` run out; launches past that are not timed.
static unsigned long long* g_tl_buf = nullptr;
static int g_tl_slots = 0, g_tl_next = 0;
static std::mutex g_tl_mu;
extern "C" int sdp_gemm_set_timeline(void* buf, int slots) {
  std::lock_guard<std::mutex> lk(g_tl_mu);
  const int used = g_tl_next;
  g_tl_buf = (unsigned long long*)buf;
  g_tl_slots = buf ? slots : 0;
  g_tl_next = 0;
  return used;
}
extern "C" int sdp_gemm_timeline_count(void) {
  std::lock_guard<std::mutex> lk(g_tl_mu);
  return g_tl_next;
}
static unsigned long long* tl_take() {
  std::lock_guard<std::mutex> lk(g_tl_mu);
  if (!g_tl_buf || g_tl_next >= g_tl_slots) return nullptr;
  return g_tl_buf + 2 * (g_tl_next++);
}

// Phases per K-tile of the 8-phase kernel's main loop: 2 (32 MFMAs per wave-group section, half the
// group-to-group hand-overs: 3.2k vs 4.3k cycles per K-tile, profiles/r04_gemm_ph2.md).  The 4-phase
// loop (16 MFMAs per section), the run-time-flag epilogue for the model's flag combinations
// (EPI_SPEC=0) and the non-temporal store policy are A/B arms of earlier rounds: they are compiled
// only into the diagnostic library (make stamps, -DSDP_DIAG).  In the product the setters accept
// only the product value (0 = query) and return -1 for anything else, so a stale selection fails
// loudly instead of silently running the default.
#ifdef SDP_DIAG
static int g_kloop_phases = 2, g_epi_spec = 1, g_nt_store = 0;
#else
static constexpr int g_kloop_phases = 2, g_epi_spec = 1, g_nt_store = 0;
#endif
extern "C" int sdp_gemm_set_kloop_phases(int n) {
  const int old = g_kloop_phases;
  if (n == 0 || n == g_kloop_phases) return old;
#ifdef SDP_DIAG
  if (n == 2 || n == 4) { g_kloop_phases = n; return old; }
#endif
  return -1;
}

// 1: the model's epilogue flag combinations take tile_epilogue_fl (product); 0: the run-time flag
// epilogue for every call (diagnostic build only)
extern "C" int sdp_gemm_set_epi_spec(int on) {
  const int old = g_epi_spec;
  if ((on ? 1 : 0) == g_epi_spec) return old;
#ifdef SDP_DIAG
  g_epi_spec = on ? 1 : 0;
  return old;
#else
  return -1;
#endif
}

extern "C" int sdp_gemm_set_store_policy(int nt) {
  const int old = g_nt_store;
  if ((nt ? 1 : 0) == g_nt_store) return old;
#ifdef SDP_DIAG
  g_nt_store = nt ? 1 : 0;
  return old;
#else
  return -1;
#endif
}

// Cross-tile kernel (gemm_bf16_ct): pair tiles per workgroup (0 = off: gemm_bf16_8ph everywhere;
// -1 = one whole row of pair tiles, i.e. tiles_n) and row groups per epilogue step (1 or 2); applied
// to the specialised-epilogue calls with K <= g_ct_kmax and N <= g_ct_nmax.
static int g_ct_tiles = 0, g_ct_re = 2, g_ct_kmax = 1024, g_ct_nmax = 1 << 30;
extern "C" int sdp_gemm_set_ct(int tiles, int re, int kmax, int nmax) {
  const int old = g_ct_tiles;
#ifndef SDP_DIAG
  // the product library does not contain the cross-tile kernel (profiles/r06_ct_gemm.md): only "off"
  (void)re, (void)kmax, (void)nmax;
  return tiles == 0 ? old : -2;
#endif
  if (tiles < -1 || tiles > 64 || (re != 1 && re != 2) || kmax < 64 || nmax < 8) return -2;
  g_ct_tiles = tiles;
  g_ct_re = re;
  g_ct_kmax = kmax;
  g_ct_nmax = nmax;
  return old;
}

#ifdef SDP_GEMM_STAMPS
extern "C" int sdp_gemm_phase_stamps(void* dst) {
  hipError_t rc = hipDeviceSynchronize();
  if (rc == hipSuccess) rc = hipMemcpyFromSymbol(dst, HIP_SYMBOL(fast::g_phase_stamps), sizeof(fast::g_phase_stamps));
  return (int)rc;
}
extern "C" int sdp_gemm_set_epi_wait(int on) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(fast::g_epi_wait), &on, sizeof(int));
}
extern "C" int sdp_gemm_set_dephase(int ticks) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(fast::g_gemm_dephase), &ticks, sizeof(int));
}
extern "C" int sdp_gemm_stamps(void* dst, int64_t bytes, int clear) {
  hipError_t rc = hipDeviceSynchronize();
  if (rc == hipSuccess && dst) rc = hipMemcpyFromSymbol(dst, HIP_SYMBOL(fast::g_gemm_stamps), std::min<int64_t>(bytes, sizeof(fast::g_gemm_stamps)));
  if (rc == hipSuccess && clear) {
    void* p = nullptr;
    rc = hipGetSymbolAddress(&p, HIP_SYMBOL(fast::g_gemm_stamps));
    if (rc == hipSuccess) rc = hipMemset(p, 0, sizeof(fast::g_gemm_stamps));
  }
  return (int)rc;
}
#endif

int sdp_row_partials(int dtype, const void* X, int64_t ldx, int x_grp, int64_t x_gstride, int x_off, int M, int C,
                     float* part, void* stream);

static int gemm_impl(int dtype, const void* X, int64_t ldx, int x_grp, int64_t x_gstride, int x_off,
                     const void* W, int64_t ldw, const float* bias, const void* R, int64_t ldr,
                     int r_grp, int64_t r_gstride, int r_off, void* Y, int64_t ldy, int y_grp,
                     int64_t y_gstride, int y_off, int M, int N, int K, int act, int resid_pre,
                     const float* ln_stats, const float* ln_colsum, float* part, bool* part_done, void* stream);

extern "C" int sdp_gemm(int dtype, const void* X, int64_t ldx, int x_grp, int64_t x_gstride, int x_off,
                        const void* W, int64_t ldw, const float* bias, const void* R, int64_t ldr,
                        int r_grp, int64_t r_gstride, int r_off, void* Y, int64_t ldy, int y_grp,
                        int64_t y_gstride, int y_off, int M, int N, int K, int act, int resid_pre,
                        void* stream) {
  return gemm_impl(dtype, X, ldx, x_grp, x_gstride, x_off, W, ldw, bias, R, ldr, r_grp, r_gstride, r_off, Y, ldy,
                   y_grp, y_gstride, y_off, M, N, K, act, resid_pre, nullptr, nullptr, nullptr, nullptr, stream);
}

// Training GEMM epilogues on the 8-phase kernel (bf16, dense rows).  mode 1: Y = X W^T + bias
// and Y2 = dropout(act(Y)) (sdp_act_fwd fused: the activation input is not re-read);
// mode 2: Y = dropout(X W^T) * act'(Z) (sdp_act_bwd fused into the input-gradient GEMM; no
// bias).  hipErrorNotSupported when the fast kernel does not take the shape / alignment (the
// caller then runs the GEMM and the activation kernel separately).
extern "C" int sdp_gemm_train_epi(int mode, const void* X, int64_t ldx, const void* W, int64_t ldw,
                                  const float* bias, const void* Z, int64_t ldz, void* Y, int64_t ldy, void* Y2,
                                  int64_t ldy2, int M, int N, int K, int act, float p, uint64_t seed,
                                  void* stream) {
  if (M < 0 || N <= 0 || K <= 0 || !X || !W || !Y || act < 0 || act > ACT_KELU || p < 0.f || p >= 1.f)
    return (int)hipErrorInvalidValue;
  if ((mode == 1 && (!Y2 || Z)) || (mode == 2 && (!Z || Y2 || bias)) || (mode != 1 && mode != 2))
    return (int)hipErrorInvalidValue;
  if (M == 0) return 0;
  auto a16 = [](const void* q) { return (uintptr_t)q % 16 == 0; };
  const bool ok = !g_force_generic && sdp_gemm_variant(1, M, N, K) == 1 && N % 8 == 0 && ldx % 8 == 0 &&
                  ldw % 8 == 0 && ldy % 8 == 0 && a16(X) && a16(W) && a16(Y) && (!bias || a16(bias)) &&
                  (mode != 1 || (ldy2 % 8 == 0 && a16(Y2))) && (mode != 2 || (ldz % 8 == 0 && a16(Z)));
  if (!ok) return (int)hipErrorNotSupported;
  const RowMap dm = mk_map(0, 0, 0);
  Epi<bf16_t> e{bias, (const bf16_t*)Z, ldz, dm, (bf16_t*)Y, ldy, dm, ACT_NONE, 0, nullptr, nullptr, nullptr};
  e.nt_store = g_nt_store;
  const int tm = (M + fast::BM - 1) / fast::BM, tn = (N + fast::BN - 1) / fast::BN;
  e.group_m = g_group_m >= 1 ? g_group_m : auto_group_m(tn);
  e.out2 = (bf16_t*)Y2;
  e.ld2 = ldy2;
  e.act2 = act;
  e.p2 = p;
  e.seed2 = seed;
  hipStream_t s = (hipStream_t)stream;
  // the model's activations get their own instantiation (the activation folds at compile
  // time); any other code goes through the run-time switch on epi.act2
#define SDP_TRN(A, E)                                                                                           \
  hipLaunchKernelGGL((fast::gemm_bf16_8ph<A, E, true>), dim3(tm * tn), dim3(fast::NTHREADS), 0, s,              \
                     (const bf16_t*)X, ldx, dm, (const bf16_t*)W, ldw, e, M, N, K, tm, tn)
  if (mode == 1) {
    if (act == ACT_GELU) SDP_TRN(ACT_GELU, 5);
    else if (act == ACT_RELU) SDP_TRN(ACT_RELU, 5);
    else SDP_TRN(-1, 5);
  } else {
    if (act == ACT_GELU) SDP_TRN(ACT_GELU, 6);
    else if (act == ACT_RELU) SDP_TRN(ACT_RELU, 6);
    else SDP_TRN(-1, 6);
  }
#undef SDP_TRN
  return SDP_CHECK_LAUNCH();
}

extern "C" int sdp_gemm_ln(int dtype, const void* X, int64_t ldx, int x_grp, int64_t x_gstride, int x_off,
                           const void* W, int64_t ldw, const float* bias, const void* R, int64_t ldr,
                           int r_grp, int64_t r_gstride, int r_off, void* Y, int64_t ldy, int y_grp,
                           int64_t y_gstride, int y_off, int M, int N, int K, int act, int resid_pre,
                           const float* ln_stats, const float* ln_colsum, float* part, void* stream) {
  if ((ln_stats != nullptr) != (ln_colsum != nullptr)) return (int)hipErrorInvalidValue;
  bool done = false;
  const int rc = gemm_impl(dtype, X, ldx, x_grp, x_gstride, x_off, W, ldw, bias, R, ldr, r_grp, r_gstride, r_off, Y,
                           ldy, y_grp, y_gstride, y_off, M, N, K, act, resid_pre, ln_stats, ln_colsum, part, &done,
                           stream);
  if (rc || !part || done || M == 0) return rc;
  // the kernel taken could not emit the partials: compute them from the stored rows
  return sdp_row_partials(dtype, Y, ldy, y_grp, y_gstride, y_off, M, N, part, stream);
}

static int gemm_impl(int dtype, const void* X, int64_t ldx, int x_grp, int64_t x_gstride, int x_off,
                     const void* W, int64_t ldw, const float* bias, const void* R, int64_t ldr,
                     int r_grp, int64_t r_gstride, int r_off, void* Y, int64_t ldy, int y_grp,
                     int64_t y_gstride, int y_off, int M, int N, int K, int act, int resid_pre,
                     const float* ln_stats, const float* ln_colsum, float* part, bool* part_done, void* stream) {
  if (M < 0 || N <= 0 || K <= 0 || !X || !W || !Y) return (int)hipErrorInvalidValue;
  if (M == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const RowMap xm = mk_map(x_grp, x_gstride, x_off);
  const RowMap rm = mk_map(r_grp, r_gstride, r_off);
  const RowMap ym = mk_map(y_grp, y_gstride, y_off);
  if (ln_colsum && (uintptr_t)ln_colsum % 16) return (int)hipErrorInvalidValue;
  if (dtype == 1) {
    Epi<bf16_t> e{bias, (const bf16_t*)R, ldr, rm, (bf16_t*)Y, ldy, ym, act, resid_pre, ln_stats, ln_colsum, nullptr};
    e.nt_store = g_nt_store;
    {
      // auto raster: groups of 2 / 4 M-blocks (round 6, auto_group_m above; round 2 chose
      // row-major up to 9 N-tiles and groups of 8 from 12 on the solo L2-miss count,
      // tools/raster_traffic.py, profiles/r02_gemm_probes.md -- the two-stream model prefers 4)
      e.group_m = g_group_m >= 1 ? g_group_m : auto_group_m((N + fast::BN - 1) / fast::BN);
    }
    const bool aligned = (ldy % 4 == 0) && ((uintptr_t)Y % 8 == 0) && (!R || ((ldr % 4 == 0) && ((uintptr_t)R % 8 == 0))) &&
                         (!bias || ((uintptr_t)bias % 16 == 0)) && (ldx % 8 == 0) && ((uintptr_t)X % 16 == 0) &&
                         (ldw % 8 == 0) && ((uintptr_t)W % 16 == 0) &&
                         (!ln_stats || ((uintptr_t)ln_stats % 8 == 0));  // the fast epilogues read (mean, rstd) as float2
    if (!g_force_generic && aligned && sdp_gemm_variant(dtype, M, N, K) == 1) {
      const int tm = (M + fast::BM - 1) / fast::BM, tn = (N + fast::BN - 1) / fast::BN;
      e.tline = g_tl_buf ? tl_take() : nullptr;
      // the whole-line epilogue needs 16-B aligned output / residual rows and N % 8 == 0,
      // and implements resid_pre only without an activation
      const bool rows_ok = (N % 8 == 0) && (ldy % 8 == 0) && ((uintptr_t)Y % 16 == 0) &&
                           (!R || ((ldr % 8 == 0) && ((uintptr_t)R % 16 == 0))) && !(R && resid_pre && act != ACT_NONE);
      const int fk = rows_ok ? g_fast_kernel : 9;
      // the whole-line epilogue emits the row partial statistics (float2 stores: an 8-B aligned
      // buffer; otherwise sdp_gemm_ln computes them from the stored rows)
      if (fk == 14 && part && N % 64 == 0 && (uintptr_t)part % 8 == 0) {
        e.part = part;
        if (part_done) *part_done = true;
      }
#ifdef SDP_DIAG
#define SDP_8PH(A, E)                                                                                               \
  do {                                                                                                              \
    if (g_kloop_phases == 2)                                                                                        \
      hipLaunchKernelGGL((fast::gemm_bf16_8ph<A, E, true>), dim3(tm * tn), dim3(fast::NTHREADS), 0, s,              \
                         (const bf16_t*)X, ldx, xm, (const bf16_t*)W, ldw, e, M, N, K, tm, tn);                     \
    else                                                                                                            \
      hipLaunchKernelGGL((fast::gemm_bf16_8ph<A, E, false>), dim3(tm * tn), dim3(fast::NTHREADS), 0, s,             \
                         (const bf16_t*)X, ldx, xm, (const bf16_t*)W, ldw, e, M, N, K, tm, tn);                     \
  } while (0)
#else
#define SDP_8PH(A, E)                                                                                               \
  hipLaunchKernelGGL((fast::gemm_bf16_8ph<A, E, true>), dim3(tm * tn), dim3(fast::NTHREADS), 0, s,                  \
                     (const bf16_t*)X, ldx, xm, (const bf16_t*)W, ldw, e, M, N, K, tm, tn)
#endif
      // erf-form GELU goes through the runtime-activation epilogue (apply_act)
      const int ak = (act == ACT_GELU && g_exact_gelu) ? -1 : act;
      // the model's epilogue combinations get compile-time flags (tile_epilogue_fl)
      const int fl = (bias ? fast::EF_BIAS : 0) | (ln_stats ? fast::EF_LN : 0) | (R ? fast::EF_RESID : 0) |
                     (e.part ? fast::EF_PART : 0);
      // byte extents of the operands the specialised epilogue addresses with 32-bit offsets
      auto extent = [M](const RowMap& rm, int64_t row_bytes) -> int64_t {
        const int64_t last = (int64_t)((M - 1) / rm.grp) * rm.gstride + rm.off + (M - 1) % rm.grp;
        int64_t mx = last;
        if ((M - 1) / rm.grp > 0) mx = std::max(mx, (int64_t)((M - 1) / rm.grp - 1) * rm.gstride + rm.off + rm.grp - 1);
        return (mx + 1) * row_bytes;
      };
      const int64_t ob = extent(ym, ldy * 2), rb = R ? extent(rm, ldr * 2) : 0, pb = e.part ? extent(ym, (N / 64) * 8) : 0;
      const bool small = ob < (1ll << 31) && rb < (1ll << 31) && pb < (1ll << 31) && ym.grp >= 8 && rm.grp >= 8;
      e.out_bytes = (uint32_t)ob;
      e.res_bytes = (uint32_t)rb;
      e.part_bytes = (uint32_t)pb;
      const bool spec = g_epi_spec && fk == 14 && small && !e.nt_store && (ak == ACT_NONE || ak == ACT_GELU) &&
                        (fl == 0 || fl == fast::EF_BIAS || fl == (fast::EF_BIAS | fast::EF_LN) ||
                         fl == (fast::EF_RESID | fast::EF_PART) || fl == (fast::EF_BIAS | fast::EF_RESID | fast::EF_PART));
#ifdef SDP_DIAG
      if (spec && g_ct_tiles != 0 && K <= g_ct_kmax && N <= g_ct_nmax) {
        const int pairs = tm * tn;
        const int ctt = g_ct_tiles > 0 ? g_ct_tiles : tn;
        const int grid = (pairs + ctt - 1) / ctt;
#define SDP_CT(A, F)                                                                                              \
  do {                                                                                                            \
    if (g_ct_re == 2)                                                                                             \
      hipLaunchKernelGGL((fast::gemm_bf16_ct<A, F, 2>), dim3(grid), dim3(fast::NTHREADS), 0, s, (const bf16_t*)X, \
                         ldx, xm, (const bf16_t*)W, ldw, e, M, N, K, tm, tn, ctt);                               \
    else                                                                                                          \
      hipLaunchKernelGGL((fast::gemm_bf16_ct<A, F, 1>), dim3(grid), dim3(fast::NTHREADS), 0, s, (const bf16_t*)X, \
                         ldx, xm, (const bf16_t*)W, ldw, e, M, N, K, tm, tn, ctt);                               \
  } while (0)
#define SDP_CT_FL(A)                                                            \
  do {                                                                          \
    if (fl == (fast::EF_BIAS | fast::EF_LN)) SDP_CT(A, 3);                      \
    else if (fl == (fast::EF_RESID | fast::EF_PART)) SDP_CT(A, 12);             \
    else if (fl == 0) SDP_CT(A, 0);                                             \
    else if (fl == fast::EF_BIAS) SDP_CT(A, 1);                                 \
    else SDP_CT(A, 13);                                                         \
  } while (0)
        if (ak == ACT_NONE) SDP_CT_FL(ACT_NONE);
        else SDP_CT_FL(ACT_GELU);
#undef SDP_CT_FL
#undef SDP_CT
      } else
#endif
      if (spec) {
#define SDP_8PH_FL(A)                                                           \
  do {                                                                          \
    if (fl == (fast::EF_BIAS | fast::EF_LN)) SDP_8PH(A, 16 + 3);                \
    else if (fl == (fast::EF_RESID | fast::EF_PART)) SDP_8PH(A, 16 + 12);       \
    else if (fl == 0) SDP_8PH(A, 16 + 0);                                       \
    else if (fl == fast::EF_BIAS) SDP_8PH(A, 16 + 1);                           \
    else SDP_8PH(A, 16 + 13);                                                   \
  } while (0)
        if (ak == ACT_NONE) SDP_8PH_FL(ACT_NONE);
        else SDP_8PH_FL(ACT_GELU);
#undef SDP_8PH_FL
      } else if (fk == 14) {
        if (ak == ACT_NONE) SDP_8PH(ACT_NONE, 4);
        else if (ak == ACT_GELU) SDP_8PH(ACT_GELU, 4);
        else if (ak == ACT_TANH) SDP_8PH(ACT_TANH, 4);
        else SDP_8PH(-1, 4);
      } else {
        if (ak == ACT_NONE) SDP_8PH(ACT_NONE, 1);
        else if (ak == ACT_GELU) SDP_8PH(ACT_GELU, 1);
        else if (ak == ACT_TANH) SDP_8PH(ACT_TANH, 1);
        else SDP_8PH(-1, 1);
      }
#undef SDP_8PH
    } else {
      dim3 grid((M + gen::BM - 1) / gen::BM, (N + gen::BN - 1) / gen::BN);
      hipLaunchKernelGGL(gen::gemm_generic<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)X, ldx, xm,
                         (const bf16_t*)W, ldw, e, M, N, K);
    }
  } else if (dtype == 0) {
    Epi<float> e{bias, (const float*)R, ldr, rm, (float*)Y, ldy, ym, act, resid_pre, ln_stats, ln_colsum, nullptr};
    dim3 grid((M + gen::BM - 1) / gen::BM, (N + gen::BN - 1) / gen::BN);
    hipLaunchKernelGGL(gen::gemm_generic<float>, grid, dim3(256), 0, s, (const float*)X, ldx, xm,
                       (const float*)W, ldw, e, M, N, K);
  } else {
    return (int)hipErrorInvalidValue;
  }
  return SDP_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------
// Split-K small-M GEMM (opt-in; sdp_gemm / sdp_gemm_ln never route here).  bf16 only.  The
// library keeps no state for it: the caller chooses bm / splits and owns the workspace.
// ---------------------------------------------------------------------------
extern "C" int64_t sdp_gemm_splitk_ws_bytes(int M, int N, int bm, int splits) {
  if (M < 0 || N <= 0 || (bm != 64 && bm != 128) || splits < 1) return -1;
  return splits > 1 ? (int64_t)splits * M * N * 4 : 0;
}

extern "C" int sdp_gemm_splitk(int dtype, const void* X, int64_t ldx, int x_grp, int64_t x_gstride, int x_off,
                               const void* W, int64_t ldw, const float* bias, const void* R, int64_t ldr,
                               int r_grp, int64_t r_gstride, int r_off, void* Y, int64_t ldy, int y_grp,
                               int64_t y_gstride, int y_off, int M, int N, int K, int act, int resid_pre,
                               const float* ln_stats, const float* ln_colsum, float* part, int bm, int splits,
                               void* ws, int64_t ws_bytes, void* stream) {
  if (dtype != 1 || M < 0 || N <= 0 || K <= 0 || !X || !W || !Y || act < 0 || act > ACT_KELU)
    return (int)hipErrorInvalidValue;
  if ((ln_stats != nullptr) != (ln_colsum != nullptr)) return (int)hipErrorInvalidValue;
  if ((bm != 64 && bm != 128) || N % small::BN || K % small::BK || splits < 1 || splits > K / small::BK)
    return (int)hipErrorInvalidValue;
  if (N / small::BN > 65535 || splits > 65535) return (int)hipErrorInvalidValue;
  const int64_t need = sdp_gemm_splitk_ws_bytes(M, N, bm, splits);
  if (need > 0 && (!ws || ws_bytes < need || (uintptr_t)ws % 16)) return (int)hipErrorInvalidValue;
  // 16-B operand chunks, 8-B output / residual vectors, 16-B bias / column-sum vectors
  auto al = [](const void* p, uintptr_t a) { return (uintptr_t)p % a == 0; };
  if (ldx % 8 || ldw % 8 || !al(X, 16) || !al(W, 16) || ldy % 4 || !al(Y, 8) || (R && (ldr % 4 || !al(R, 8))) ||
      (bias && !al(bias, 16)) || (ln_colsum && !al(ln_colsum, 16)) || (ln_stats && !al(ln_stats, 8)) ||
      (part && !al(part, 8)))
    return (int)hipErrorInvalidValue;
  if (M == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const RowMap xm = mk_map(x_grp, x_gstride, x_off);
  Epi<bf16_t> e{bias, (const bf16_t*)R, ldr, mk_map(r_grp, r_gstride, r_off), (bf16_t*)Y, ldy,
                mk_map(y_grp, y_gstride, y_off), act, resid_pre, ln_stats, ln_colsum, part};
  // GELU in the fast kernel's form (tanh unless sdp_gemm_set_exact_gelu(1)): the activation
  // function must not change with the batch size
  const int fast_gelu = (act == ACT_GELU && !g_exact_gelu) ? 1 : 0;
  const dim3 grid((M + bm - 1) / bm, N / small::BN, splits);
  if (bm == 64)
    hipLaunchKernelGGL(small::gemm_bf16_splitk<64>, grid, dim3(small::NTHREADS), 0, s, (const bf16_t*)X, ldx, xm,
                       (const bf16_t*)W, ldw, e, (float*)ws, M, N, K, splits, fast_gelu);
  else
    hipLaunchKernelGGL(small::gemm_bf16_splitk<128>, grid, dim3(small::NTHREADS), 0, s, (const bf16_t*)X, ldx, xm,
                       (const bf16_t*)W, ldw, e, (float*)ws, M, N, K, splits, fast_gelu);
  if (splits > 1) {
    const int rc = SDP_CHECK_LAUNCH();
    if (rc) return rc;
    hipLaunchKernelGGL(small::splitk_reduce, dim3((M + 15) / 16, N / small::BN), dim3(small::NTHREADS), 0, s,
                       (const float*)ws, e, M, N, splits, fast_gelu);
  }
  return SDP_CHECK_LAUNCH();
}
