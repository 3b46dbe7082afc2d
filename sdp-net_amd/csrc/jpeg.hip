// Device half of the hybrid JPEG decoder: sdp_jpeg_reconstruct.
//
// The host (jpeg_host.h) has done the serial Huffman decode; what is left is data-parallel and runs
// here for a batch of images of different sizes and modes, in two passes:
//   jpeg_idct_k    dequantise + 8x8 inverse DCT (13-bit fixed-point Loeffler / Ligtenberg /
//                  Moschytz, columns first) of every block into planar uint8 samples over the
//                  padded block grid (the workspace);
//   jpeg_colour_k  2:1 "fancy" chroma upsampling with the edges of the component's true size,
//                  YCbCr -> RGB in 16-bit fixed point, HWC uint8 into the packed pix buffer that
//                  sdp_val_preprocess and sdp_resized_crop read.
// The arithmetic is libjpeg's integer decoder restated, so the pixels equal Pillow's bit for bit
// wherever the signed 32-bit computation does not overflow (every stream an 8-bit encoder writes);
// sums and products wrap as unsigned 32-bit, so no coefficient or table can cause undefined
// behaviour.  Descriptor layout: include/sdpnet_hip.h.
#include "common.h"

namespace jpg {
constexpr int DESC = 64;  // int32 words per image
constexpr int D_W = 0, D_H = 1, D_NCOMP = 2, D_MODE = 3, D_MCUX = 4, D_MCUY = 5, D_COEF = 6, D_WS = 8, D_PIX = 10,
              D_QT = 16;

struct Img {
  int W, H, nc, mode, mcux, mcuy, bw0, bh0;
  int64_t coef, ws, pix;
};

template <typename P>
__host__ SDP_DEV Img image(P q) {
  Img g;
  g.W = q[D_W], g.H = q[D_H], g.nc = q[D_NCOMP], g.mode = q[D_MODE], g.mcux = q[D_MCUX], g.mcuy = q[D_MCUY];
  g.bw0 = g.mcux * (g.nc == 3 && g.mode >= 1 ? 2 : 1);
  g.bh0 = g.mcuy * (g.nc == 3 && g.mode == 2 ? 2 : 1);
  g.coef = (int64_t)((uint64_t)(uint32_t)q[D_COEF] | ((uint64_t)(uint32_t)q[D_COEF + 1] << 32));
  g.ws = (int64_t)((uint64_t)(uint32_t)q[D_WS] | ((uint64_t)(uint32_t)q[D_WS + 1] << 32));
  g.pix = (int64_t)((uint64_t)(uint32_t)q[D_PIX] | ((uint64_t)(uint32_t)q[D_PIX + 1] << 32));
  return g;
}

SDP_DEV int32_t descale(uint32_t x, int n) { return (int32_t)(x + (1u << (n - 1))) >> n; }

// One pass of the inverse DCT over v[0..7]; out[k] = DESCALE(.., shift).  Unsigned arithmetic wraps.
SDP_DEV void idct8(const uint32_t* v, int shift, int32_t* out) {
  uint32_t z2 = v[2], z3 = v[6];
  uint32_t z1 = (z2 + z3) * 4433u;
  uint32_t t2 = z1 - z3 * 15137u;
  uint32_t t3 = z1 + z2 * 6270u;
  uint32_t t0 = (v[0] + v[4]) << 13;
  uint32_t t1 = (v[0] - v[4]) << 13;
  const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  t0 = v[7], t1 = v[5], t2 = v[3], t3 = v[1];
  z1 = t0 + t3, z2 = t1 + t2, z3 = t0 + t2;
  uint32_t z4 = t1 + t3;
  const uint32_t z5 = (z3 + z4) * 9633u;
  t0 *= 2446u, t1 *= 16819u, t2 *= 25172u, t3 *= 12299u;
  z1 *= (uint32_t)-7373, z2 *= (uint32_t)-20995;
  z3 = z3 * (uint32_t)-16069 + z5;
  z4 = z4 * (uint32_t)-3196 + z5;
  t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4;
  out[0] = descale(t10 + t3, shift), out[7] = descale(t10 - t3, shift);
  out[1] = descale(t11 + t2, shift), out[6] = descale(t11 - t2, shift);
  out[2] = descale(t12 + t1, shift), out[5] = descale(t12 - t1, shift);
  out[3] = descale(t13 + t0, shift), out[4] = descale(t13 - t0, shift);
}

SDP_DEV int clamp255(int v) { return min(max(v, 0), 255); }

// 8 lanes per block, 32 blocks per workgroup.  Lane j loads coefficient row j (16 bytes), the block
// is transposed through LDS (rows padded to 9 words: both the column and the row access are free of
// bank conflicts), lane j runs column j, then row j, and stores row j's 8 samples with one store.
constexpr int BLOCKS_PER_WG = 32;
__global__ __launch_bounds__(256) void jpeg_idct_k(const int16_t* __restrict__ coef, const int32_t* __restrict__ desc,
                                                   uint8_t* __restrict__ ws) {
  __shared__ int32_t sm[BLOCKS_PER_WG][8][9];
  const int32_t* q = desc + (int64_t)blockIdx.y * DESC;
  const Img g = image(q);
  const int64_t n0 = (int64_t)g.bw0 * g.bh0, nc1 = (int64_t)g.mcux * g.mcuy;
  const int64_t nblk = n0 + (g.nc == 3 ? 2 * nc1 : 0);
  if ((int64_t)blockIdx.x * BLOCKS_PER_WG >= nblk) return;  // uniform over the workgroup
  const int slot = threadIdx.x >> 3, j = threadIdx.x & 7;
  const int64_t blk = (int64_t)blockIdx.x * BLOCKS_PER_WG + slot;
  const bool live = blk < nblk;
  int comp = 0, bw = g.bw0;
  int64_t rel = blk, plane = 0;
  if (blk >= n0) {
    comp = blk >= n0 + nc1 ? 2 : 1;
    rel = blk - n0 - (comp == 2 ? nc1 : 0);
    bw = g.mcux;
    plane = 64 * (n0 + (comp == 2 ? nc1 : 0));
  }
  if (live) {
    const uint4 raw = *(const uint4*)(coef + g.coef + blk * 64 + j * 8);
    const uint32_t qa = (uint32_t)q[D_QT + comp * 16 + j * 2], qb = (uint32_t)q[D_QT + comp * 16 + j * 2 + 1];
    const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int cv = (int16_t)(w[c >> 1] >> (16 * (c & 1)));
      const int qv = (int)(((c < 4 ? qa : qb) >> (8 * (c & 3))) & 255u);
      sm[slot][j][c] = cv * qv;
    }
  }
  __syncthreads();
  if (live) {
    uint32_t v[8];
    int32_t o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (uint32_t)sm[slot][k][j];
    idct8(v, 11, o);
#pragma unroll
    for (int k = 0; k < 8; ++k) sm[slot][k][j] = o[k];
  }
  __syncthreads();
  if (live) {
    uint32_t v[8];
    int32_t o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (uint32_t)sm[slot][j][k];
    idct8(v, 18, o);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      lo |= (uint32_t)clamp255(o[k] + 128) << (8 * k);
      hi |= (uint32_t)clamp255(o[k + 4] + 128) << (8 * k);
    }
    const int64_t by = rel / bw, bx = rel - by * bw;
    *(uint2*)(ws + g.ws + plane + (by * 8 + j) * ((int64_t)bw * 8) + bx * 8) = make_uint2(lo, hi);
  }
}

SDP_DEV void store_rgb(uint8_t* p, int y, int cb, int cr) {
  cb -= 128, cr -= 128;
  p[0] = (uint8_t)clamp255(y + ((91881 * cr + 32768) >> 16));
  p[1] = (uint8_t)clamp255(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  p[2] = (uint8_t)clamp255(y + ((116130 * cb + 32768) >> 16));
}

// One lane per pair of output pixels (2i, 2i + 1) of a row: they share chroma column i.
__global__ __launch_bounds__(256) void jpeg_colour_k(const uint8_t* __restrict__ ws, const int32_t* __restrict__ desc,
                                                     uint8_t* __restrict__ pix) {
  const Img g = image(desc + (int64_t)blockIdx.y * DESC);
  const int pw = (g.W + 1) >> 1;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)pw * g.H) return;
  const int y = (int)(t / pw), i = (int)(t - (int64_t)y * pw);
  const int x0 = 2 * i;
  const bool two = x0 + 1 < g.W;
  const int64_t ys = (int64_t)g.bw0 * 8;
  const uint8_t* Y = ws + g.ws + y * ys + x0;
  uint8_t* out = pix + g.pix + ((int64_t)y * g.W + x0) * 3;
  const int y0 = Y[0], y1 = Y[1];  // column x0 + 1 <= W lies inside the padded plane when W is odd
  if (g.nc == 1) {
    out[0] = out[1] = out[2] = (uint8_t)y0;
    if (two) out[3] = out[4] = out[5] = (uint8_t)y1;
    return;
  }
  const int64_t cs = (int64_t)g.mcux * 8, csize = cs * g.mcuy * 8;
  const uint8_t* Cb = ws + g.ws + ys * g.bh0 * 8;
  int cb0, cb1, cr0, cr1;
  if (g.mode == 0) {
    const uint8_t* p = Cb + y * cs + x0;
    cb0 = p[0], cb1 = p[1], cr0 = p[csize], cr1 = p[csize + 1];
  } else {
    const int cw = pw;  // the chroma component's true width, ceil(W / 2)
    const int il = max(i - 1, 0), ir = min(i + 1, cw - 1);
    if (g.mode == 1) {
      const uint8_t* p = Cb + y * cs;
      if (cw <= 2) {
        cb0 = cb1 = p[i], cr0 = cr1 = p[csize + i];
      } else {
        const int sb = p[i], sr = p[csize + i];
        cb0 = i == 0 ? sb : (3 * sb + p[il] + 1) >> 2;
        cr0 = i == 0 ? sr : (3 * sr + p[csize + il] + 1) >> 2;
        cb1 = i == cw - 1 ? sb : (3 * sb + p[ir] + 2) >> 2;
        cr1 = i == cw - 1 ? sr : (3 * sr + p[csize + ir] + 2) >> 2;
      }
    } else {
      const int ch = (g.H + 1) >> 1, r = y >> 1;
      const int rn = (y & 1) ? min(r + 1, ch - 1) : max(r - 1, 0);
      const uint8_t* p = Cb + r * cs;
      const uint8_t* n = Cb + rn * cs;
      if (cw <= 2) {
        cb0 = cb1 = p[i], cr0 = cr1 = p[csize + i];
      } else {
        const int b = 3 * p[i] + n[i], bl = 3 * p[il] + n[il], br = 3 * p[ir] + n[ir];
        const int c = 3 * p[csize + i] + n[csize + i], cl = 3 * p[csize + il] + n[csize + il],
                  cr = 3 * p[csize + ir] + n[csize + ir];
        cb0 = i == 0 ? (4 * b + 8) >> 4 : (3 * b + bl + 8) >> 4;
        cr0 = i == 0 ? (4 * c + 8) >> 4 : (3 * c + cl + 8) >> 4;
        cb1 = i == cw - 1 ? (4 * b + 7) >> 4 : (3 * b + br + 7) >> 4;
        cr1 = i == cw - 1 ? (4 * c + 7) >> 4 : (3 * c + cr + 7) >> 4;
      }
    }
  }
  store_rgb(out, y0, cb0, cr0);
  if (two) store_rgb(out + 3, y1, cb1, cr1);
}
}  // namespace jpg

extern "C" int sdp_jpeg_reconstruct(const int16_t* coef, int64_t coef_elems, const int32_t* desc_host,
                                    const int32_t* desc_dev, int B, uint8_t* ws, int64_t ws_bytes, uint8_t* pix,
                                    int64_t pix_bytes, void* stream) {
  if (B < 0 || B > 65535 || coef_elems < 0 || ws_bytes < 0 || pix_bytes < 0) return (int)hipErrorInvalidValue;
  if (B == 0) return 0;
  if (!coef || !desc_host || !desc_dev || !ws || !pix) return (int)hipErrorInvalidValue;
  if (((uintptr_t)coef & 15) || ((uintptr_t)ws & 7) || ((uintptr_t)desc_dev & 3)) return (int)hipErrorInvalidValue;
  int64_t max_blocks = 0, max_pairs = 0;
  for (int b = 0; b < B; ++b) {
    const int32_t* q = desc_host + (int64_t)b * jpg::DESC;
    const jpg::Img g = jpg::image(q);
    if (g.W < 1 || g.W > 65535 || g.H < 1 || g.H > 65535 || (g.nc != 1 && g.nc != 3) || g.mode < 0 || g.mode > 2 ||
        (g.nc == 1 && g.mode != 0))
      return (int)hipErrorInvalidValue;
    const int hs = g.nc == 3 && g.mode >= 1 ? 2 : 1, vs = g.nc == 3 && g.mode == 2 ? 2 : 1;
    if (g.mcux != (g.W + 8 * hs - 1) / (8 * hs) || g.mcuy != (g.H + 8 * vs - 1) / (8 * vs))
      return (int)hipErrorInvalidValue;
    const int64_t blocks = (int64_t)g.bw0 * g.bh0 + (g.nc == 3 ? 2 * (int64_t)g.mcux * g.mcuy : 0);
    const int64_t n = 64 * blocks;  // coefficients, and bytes of planar samples
    if (g.coef < 0 || (g.coef & 7) || g.coef > coef_elems || n > coef_elems - g.coef) return (int)hipErrorInvalidValue;
    if (g.ws < 0 || (g.ws & 7) || g.ws > ws_bytes || n > ws_bytes - g.ws) return (int)hipErrorInvalidValue;
    const int64_t out = (int64_t)g.W * g.H * 3;
    if (g.pix < 0 || g.pix > pix_bytes || out > pix_bytes - g.pix) return (int)hipErrorInvalidValue;
    max_blocks = std::max(max_blocks, blocks);
    max_pairs = std::max(max_pairs, (int64_t)((g.W + 1) / 2) * g.H);
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(jpg::jpeg_idct_k, dim3((unsigned)((max_blocks + jpg::BLOCKS_PER_WG - 1) / jpg::BLOCKS_PER_WG), B),
                     dim3(256), 0, s, coef, desc_dev, ws);
  hipLaunchKernelGGL(jpg::jpeg_colour_k, dim3((unsigned)((max_pairs + 255) / 256), B), dim3(256), 0, s,
                     (const uint8_t*)ws, desc_dev, pix);
  return SDP_CHECK_LAUNCH();
}
