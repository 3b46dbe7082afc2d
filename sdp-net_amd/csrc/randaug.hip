// RandAugment on the device: num_ops ops in sequence on every image of a uint8 [B][H][W][3] batch.
//
// The reference's train_transforms (hf_dataset_generator.py:43-57) runs torchvision's
// RandAugment() on PIL images between RandomResizedCrop / flip and the tensor conversion, i.e.
// through Pillow.  sdp_randaugment restates Pillow 12.2.0's arithmetic bit for bit, in integers
// and fp32 only: Image.transform's 16.16 fixed-point nearest path (Geometry.c affine_fixed),
// ImagingBlend's fp32 interpolation (Blend.c), ImageFilter.SMOOTH's interior / copied border,
// ImageOps.autocontrast / equalize tables, the L conversion (19595 R + 38470 G + 7471 B + 0x8000)
// >> 16.  Every random decision and every double-precision parameter is taken on the host and
// arrives in the plan; plan words are compared or used in arithmetic whose result is range-checked
// before it addresses anything, so no plan can reach outside image b.
//
// Plan (int32, one host copy): [B][num_ops][8] = {op, p1 .. p7}:
//   0 Identity
//   1..5 ShearX, ShearY, TranslateX, TranslateY, Rotate: p1..p6 = a0..a5, the 16.16 words of the
//        output -> input matrix; xin = (a2 + a0 x + a1 y) >> 16, yin = (a5 + a3 x + a4 y) >> 16,
//        a source pixel outside the image gives 0
//   6..9 Brightness, Color, Contrast, Sharpness: p1 = bits of the fp32 factor f;
//        out = blend(degenerate, in, f)
//   10 Posterize: p1 = mask;  11 Solarize: p1 = the first inverted value
//   12 AutoContrast;  13 Equalize
// Any other op code is Identity.
//
// One workgroup per image.  An image of at most 224 x 224 x 3 bytes lives in LDS for the whole
// sequence (150,528 B + 3.8 KiB of histogram / table space of the CU's 160 KiB): pointwise and
// histogram ops rewrite the LDS copy in place, the gather ops (affine, Sharpness) read it and
// write the image's scratch slice, which is then read back, with workgroup barriers between the
// phases.  A larger image takes the same code with the output slice in global memory as the
// working copy.
#include "common.h"

namespace ra {
constexpr int PER = 8;                      // plan words per op
constexpr int LDS_IMAGE = 224 * 224 * 3;    // bytes of the largest image kept in LDS
constexpr int HDR = 3072 + 768 + 16;        // histogram counters, byte tables, the luma sum
constexpr int MAX_THREADS = 1024;

// ImagingBlend: (UINT8)((int)d + f * ((int)s - (int)d)) in fp32, one rounded product and one
// rounded sum (no contraction); outside 0 <= f <= 1 the value is clamped to [0, 255] first.
SDP_DEV uint8_t blend(int d, int s, float f, bool inside) {
#pragma clang fp contract(off)
  const float p = f * (float)(s - d);
  float t = (float)d + p;
  if (!inside) t = t <= 0.f ? 0.f : (t >= 255.f ? 255.f : t);
  return (uint8_t)(int)t;
}
SDP_DEV int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// 16 bytes per lane when both ends allow it (the caller says so), bytes otherwise and for the tail
SDP_DEV void copy_bytes(uint8_t* dst, const uint8_t* src, int n, bool wide) {
  int done = 0;
  if (wide) {
    const int n16 = n >> 4;
    for (int i = threadIdx.x; i < n16; i += blockDim.x) ((uint4*)dst)[i] = ((const uint4*)src)[i];
    done = n16 << 4;
  }
  for (int i = done + threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}
SDP_DEV bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// out[y][x] = cur[yin][xin] or 0: Geometry.c affine_fixed (the host keeps the plan inside the
// range where int32 does not wrap; 64-bit here, so a bad word only fails the range test)
SDP_DEV void affine(const uint8_t* cur, uint8_t* dst, const int* q, int H, int W) {
  const int64_t a0 = q[1], a1 = q[2], a2 = q[3], a3 = q[4], a4 = q[5], a5 = q[6];
  const int npix = H * W;
  for (int p = threadIdx.x; p < npix; p += blockDim.x) {
    const int y = p / W, x = p - y * W;
    const int64_t xin = (a2 + a0 * x + a1 * y) >> 16, yin = (a5 + a3 * x + a4 * y) >> 16;
    uint8_t r = 0, g = 0, b = 0;
    if (xin >= 0 && xin < W && yin >= 0 && yin < H) {
      const uint8_t* s = cur + ((int)yin * W + (int)xin) * 3;
      r = s[0];
      g = s[1];
      b = s[2];
    }
    dst[p * 3 + 0] = r;
    dst[p * 3 + 1] = g;
    dst[p * 3 + 2] = b;
  }
}

// blend(SMOOTH(cur), cur, f): (1 1 1; 1 5 1; 1 1 1) / 13 rounded half up inside, the one-pixel
// border copied (every pixel of an image with H < 3 or W < 3 is border)
SDP_DEV void sharpness(const uint8_t* cur, uint8_t* dst, float f, bool inside, int H, int W) {
  const int npix = H * W;
  for (int p = threadIdx.x; p < npix; p += blockDim.x) {
    const int y = p / W, x = p - y * W;
    const bool interior = x > 0 && y > 0 && x < W - 1 && y < H - 1;
    const uint8_t* s = cur + p * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int v = s[c];
      int d = v;
      if (interior) {
        int sum = 4 * v;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) sum += s[(dy * W + dx) * 3 + c];
        d = min((2 * sum + 13) / 26, 255);
      }
      dst[p * 3 + c] = blend(d, v, f, inside);
    }
  }
}

// ImageOps.autocontrast (cutoff 0) table of one channel
SDP_DEV void autocontrast_table(const uint32_t* h, uint8_t* lut) {
#pragma clang fp contract(off)
  int lo = 0, hi = 255;
  while (lo < 256 && h[lo] == 0) ++lo;
  while (hi >= 0 && h[hi] == 0) --hi;
  if (hi <= lo) {
    for (int i = 0; i < 256; ++i) lut[i] = (uint8_t)i;
    return;
  }
  const double scale = 255.0 / (hi - lo);
  const double offset = -lo * scale;
  for (int i = 0; i < 256; ++i) {
    const double m = i * scale;
    const int v = (int)(m + offset);
    lut[i] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
  }
}

// ImageOps.equalize table of one channel
SDP_DEV void equalize_table(const uint32_t* h, uint8_t* lut, int npix) {
  int nonzero = 0, last = 0;
  for (int i = 0; i < 256; ++i)
    if (h[i]) {
      ++nonzero;
      last = (int)h[i];
    }
  const int step = (npix - last) / 255;
  if (nonzero <= 1 || step == 0) {
    for (int i = 0; i < 256; ++i) lut[i] = (uint8_t)i;
    return;
  }
  int64_t n = step / 2;
  for (int i = 0; i < 256; ++i) {
    lut[i] = (uint8_t)min(n / step, (int64_t)255);
    n += h[i];
  }
}

template <bool LDS>
__global__ __launch_bounds__(MAX_THREADS) void randaug_k(const uint8_t* in, uint8_t* out, uint8_t* scratch,
                                                         const int* __restrict__ plan, int H, int W, int num_ops) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint32_t* hist = (uint32_t*)smem;                                 // [3][256]
  uint8_t* lut = smem + 3072;                                       // [3][256]
  unsigned long long* lsum = (unsigned long long*)(smem + 3840);
  const int b = blockIdx.x;
  const int npix = H * W, n = npix * 3;  // the entry point keeps n below 2^31
  const uint8_t* src = in + (int64_t)b * n;
  uint8_t* dst = out + (int64_t)b * n;
  uint8_t* alt = scratch + (int64_t)b * n;
  uint8_t* cur = LDS ? smem + HDR : dst;
  if (LDS || src != dst) copy_bytes(cur, src, n, aligned16(src) && (LDS || aligned16(dst)));
  __syncthreads();
  for (int k = 0; k < num_ops; ++k) {
    const int* q = plan + ((int64_t)b * num_ops + k) * PER;
    const int op = __builtin_amdgcn_readfirstlane(q[0]);
    const float f = __int_as_float(q[1]);
    const bool inside = f >= 0.f && f <= 1.f;
    if ((op >= 1 && op <= 5) || op == 9) {
      if (op == 9)
        sharpness(cur, alt, f, inside, H, W);
      else
        affine(cur, alt, q, H, W);
      __syncthreads();
      copy_bytes(cur, alt, n, aligned16(alt) && (LDS || aligned16(dst)));
    } else if (op == 6) {
      for (int i = threadIdx.x; i < n; i += blockDim.x) cur[i] = blend(0, cur[i], f, inside);
    } else if (op == 7) {
      for (int p = threadIdx.x; p < npix; p += blockDim.x) {
        uint8_t* s = cur + p * 3;
        const int r = s[0], g = s[1], bl = s[2];
        const int L = luma(r, g, bl);
        s[0] = blend(L, r, f, inside);
        s[1] = blend(L, g, f, inside);
        s[2] = blend(L, bl, f, inside);
      }
    } else if (op == 8) {
      if (threadIdx.x == 0) *lsum = 0ull;
      __syncthreads();
      unsigned long long part = 0;
      for (int p = threadIdx.x; p < npix; p += blockDim.x) {
        const uint8_t* s = cur + p * 3;
        part += (unsigned)luma(s[0], s[1], s[2]);
      }
      for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
      if ((threadIdx.x & 63) == 0) atomicAdd(lsum, part);
      __syncthreads();
      // int(mean + 0.5) with the mean an integer sum divided in double precision (ImageStat)
      const int mean = (int)((double)*lsum / (double)npix + 0.5);
      for (int i = threadIdx.x; i < n; i += blockDim.x) cur[i] = blend(mean, cur[i], f, inside);
    } else if (op == 10) {
      const int mask = q[1] & 0xff;
      for (int i = threadIdx.x; i < n; i += blockDim.x) cur[i] = (uint8_t)(cur[i] & mask);
    } else if (op == 11) {
      const int thr = q[1];
      for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int v = cur[i];
        cur[i] = (uint8_t)(v >= thr ? 255 - v : v);
      }
    } else if (op == 12 || op == 13) {
      for (int i = threadIdx.x; i < 768; i += blockDim.x) hist[i] = 0u;
      __syncthreads();
      for (int p = threadIdx.x; p < npix; p += blockDim.x) {
        const uint8_t* s = cur + p * 3;
        atomicAdd(&hist[s[0]], 1u);
        atomicAdd(&hist[256 + s[1]], 1u);
        atomicAdd(&hist[512 + s[2]], 1u);
      }
      __syncthreads();
      if (threadIdx.x < 3) {
        if (op == 12)
          autocontrast_table(hist + 256 * threadIdx.x, lut + 256 * threadIdx.x);
        else
          equalize_table(hist + 256 * threadIdx.x, lut + 256 * threadIdx.x, npix);
      }
      __syncthreads();
      for (int p = threadIdx.x; p < npix; p += blockDim.x) {
        uint8_t* s = cur + p * 3;
        s[0] = lut[s[0]];
        s[1] = lut[256 + s[1]];
        s[2] = lut[512 + s[2]];
      }
    }
    __syncthreads();
  }
  if (LDS) copy_bytes(dst, cur, n, aligned16(dst));
}
}  // namespace ra

extern "C" int sdp_randaugment(const uint8_t* in, uint8_t* out, const int32_t* plan, int B, int H, int W,
                               int num_ops, uint8_t* scratch, void* stream) {
  if (B < 0 || H <= 0 || W <= 0 || num_ops < 1 || num_ops > 4 || (int64_t)H * W * 3 >= (int64_t)1 << 31)
    return (int)hipErrorInvalidValue;
  if (B == 0) return 0;
  if (!in || !out || !plan || !scratch) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const int n = H * W * 3;
  const int threads = H * W >= 16384 ? ra::MAX_THREADS : 256;
  if (n <= ra::LDS_IMAGE) {
    const size_t lds = ra::HDR + (size_t)((n + 15) & ~15);
    if (lds > 65536) {
      static bool raised = false;
      if (!raised) {
        (void)hipFuncSetAttribute((const void*)ra::randaug_k<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  160 * 1024);
        raised = true;
      }
    }
    hipLaunchKernelGGL(ra::randaug_k<true>, dim3(B), dim3(threads), lds, s, in, out, scratch, plan, H, W, num_ops);
  } else {
    hipLaunchKernelGGL(ra::randaug_k<false>, dim3(B), dim3(threads), ra::HDR, s, in, out, scratch, plan, H, W,
                       num_ops);
  }
  return SDP_CHECK_LAUNCH();
}
