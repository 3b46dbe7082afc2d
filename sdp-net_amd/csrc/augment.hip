// Batch-level tail of the reference's training input pipeline, on the device.
//
// The reference ends every training sample with ToImage -> ToDtype(float32, scale=True) ->
// Normalize -> RandomErasing(p=0.25) (hf_dataset_generator.py:43-57) and collates the batch
// through RandomChoice([CutMix(), MixUp(alpha=0.8)]) with the labels expanded to [B, 1000] float
// rows (hf_dataset_generator.py:325-336, dataset_generator.py:105-110), all in fp32 on the
// loader's CPU.  sdp_train_batch_aug does the same arithmetic on a uint8 batch: one streaming pass
// that writes the model's NCHW input (fp32 or bf16) and, when the batch is mixed, the dense
// target rows.  Every random decision is taken on the host and arrives as the plan (one int32
// device buffer); nothing in the plan is ever used as an index, so no plan can address memory
// outside the operands.
//
// Plan layout (int32 words): header {mode, bits(wa), bits(wp), x1, y1, x2, y2, 0}, then per image
// {flip, top, left, h, w, 0, 0, 0}.
#include "common.h"

namespace aug {
constexpr int HDR = 8;   // header words
constexpr int PER = 8;   // words per image

struct Img {  // per-image plan
  int flip, top, left, h, w;
};
SDP_DEV Img img_plan(const int* __restrict__ plan, int i) {
  const int* q = plan + HDR + (int64_t)i * PER;
  return Img{q[0], q[1], q[2], q[3], q[4]};
}
// unsigned compare: v in [lo, lo + n) for n >= 0 without overflow on hostile plans
SDP_DEV bool in_range(int v, int lo, int n) { return n > 0 && v >= lo && (int64_t)v < (int64_t)lo + n; }
SDP_DEV bool erased(const Img& g, int y, int x) { return in_range(y, g.top, g.h) && in_range(x, g.left, g.w); }

// fl(fl(vp * wp) + fl(vb * wa)): x.roll(1, 0).mul(1 - lam).add_(x.mul(lam)).  The pragma keeps
// the compiler from contracting a product into the sum (HIP's __fmul_rn / __fadd_rn are plain
// operators and would be fused): two rounded products, one rounded sum, as torch computes them.
SDP_DEV float mix(float vp, float wp, float vb, float wa) {
#pragma clang fp contract(off)
  const float a = vp * wp;
  const float b = vb * wa;
  return a + b;
}

// ---- generic path: one output element per thread, any W, either input layout ----
template <typename TO>
__global__ __launch_bounds__(256) void generic_k(const uint8_t* __restrict__ images, int nhwc,
                                                 const float* __restrict__ lut, const int* __restrict__ plan, int B,
                                                 int H, int W, TO* __restrict__ out) {
  __shared__ float tab[3 * 256];
  for (int i = threadIdx.x; i < 3 * 256; i += blockDim.x) tab[i] = lut[i];
  __syncthreads();
  const int mode = plan[0];
  const float wa = __int_as_float(plan[1]), wp = __int_as_float(plan[2]);
  const int x1 = plan[3], y1 = plan[4], x2 = plan[5], y2 = plan[6];
  const int64_t total = (int64_t)B * 3 * H * W;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(idx % W);
    const int64_t r = idx / W;
    const int y = (int)(r % H);
    const int pc = (int)(r / H);
    const int b = pc / 3, c = pc - 3 * b;
    auto value = [&](int i) -> float {
      const Img g = img_plan(plan, i);
      if (erased(g, y, x)) return 0.f;
      const int sx = g.flip ? W - 1 - x : x;
      const int64_t at = nhwc ? (((int64_t)i * H + y) * W + sx) * 3 + c : (((int64_t)i * 3 + c) * H + y) * W + sx;
      return tab[c * 256 + images[at]];
    };
    const int p = b == 0 ? B - 1 : b - 1;
    float v;
    if (mode == 1)
      v = mix(value(p), wp, value(b), wa);
    else if (mode == 2 && y >= y1 && y < y2 && x >= x1 && x < x2)
      v = value(p);
    else
      v = value(b);
    out[idx] = from_f<TO>(v);
  }
}

// ---- fast path: NCHW, W % 8 == 0, 8-byte aligned input, 16-byte aligned output ----
// A workgroup owns a slice of one (image, channel) plane, so its LUT is the 256 entries of one
// channel (1 KiB of LDS).  A lane takes groups of 8 consecutive pixels of a row: one 8-byte load
// per source image, one (bf16) or two (fp32) 16-byte stores per group.
// A flipped row reads the mirrored group and reverses its bytes, so that byte j of the result is
// output pixel x0 + j either way.
SDP_DEV uint2 load8(const uint8_t* __restrict__ row, int W, int x0, const Img& g) {
  const uint2 r = *reinterpret_cast<const uint2*>(row + (g.flip ? W - 8 - x0 : x0));
  return g.flip ? uint2{__builtin_bswap32(r.y), __builtin_bswap32(r.x)} : r;
}
SDP_DEV void decode8(uint2 raw, int x0, const Img& g, int y, const float* tab, float (&v)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = tab[((j < 4 ? raw.x : raw.y) >> (8 * (j & 3))) & 0xffu];
  if (in_range(y, g.top, g.h)) {  // few rows of few images: keep the column tests off the common path
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = in_range(x0 + j, g.left, g.w) ? 0.f : v[j];
  }
}

template <typename TO> SDP_DEV void store8(TO* dst, const float (&v)[8]);
template <> SDP_DEV void store8<float>(float* dst, const float (&v)[8]) {
  reinterpret_cast<f32x4*>(dst)[0] = f32x4{v[0], v[1], v[2], v[3]};
  reinterpret_cast<f32x4*>(dst)[1] = f32x4{v[4], v[5], v[6], v[7]};
}
template <> SDP_DEV void store8<bf16_t>(bf16_t* dst, const float (&v)[8]) {
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (short)f2bf(v[j]);
  *reinterpret_cast<bf16x8*>(dst) = o;
}

// Measured at B = 120, 224 x 224 (tools/aug_bench.py): two groups per lane with both loads issued
// before either is used, and as many workgroups per plane as give every lane one such round,
// beat one or four groups per lane and a grid-stride loop over 8 workgroups per plane.
constexpr int UNROLL = 2;       // 8-pixel groups per lane whose loads are issued together
constexpr int MAX_CHUNKS = 64;  // workgroups per (image, channel) plane; larger planes loop

template <typename TO>
__global__ __launch_bounds__(256) void plane_k(const uint8_t* __restrict__ images, const float* __restrict__ lut,
                                               const int* __restrict__ plan, int B, int H, int W, int chunks,
                                               TO* __restrict__ out) {
  __shared__ float tab[256];
  const int pc = blockIdx.x / chunks, chunk = blockIdx.x - pc * chunks;
  const int b = pc / 3, c = pc - 3 * b;
  tab[threadIdx.x] = lut[c * 256 + threadIdx.x];  // blockDim.x == 256
  __syncthreads();
  const int mode = plan[0];
  const float wa = __int_as_float(plan[1]), wp = __int_as_float(plan[2]);
  const int x1 = plan[3], y1 = plan[4], x2 = plan[5], y2 = plan[6];
  const int p = b == 0 ? B - 1 : b - 1;
  const Img gb = img_plan(plan, b), gp = img_plan(plan, p);
  const int64_t plane = (int64_t)H * W;
  const uint8_t* src_b = images + ((int64_t)b * 3 + c) * plane;
  const uint8_t* src_p = images + ((int64_t)p * 3 + c) * plane;
  TO* dst = out + (int64_t)pc * plane;
  const int W8 = W >> 3;
  const int items = H * W8;  // the entry point keeps H * W below 2^31
  for (int base = chunk * 256 * UNROLL; base < items; base += chunks * 256 * UNROLL) {
    // all the loads of this round first, so that each lane has UNROLL (x 2 when mixing) in flight
    uint2 rb[UNROLL], rp[UNROLL];
    int ys[UNROLL], xs[UNROLL];
    bool ok[UNROLL], partner[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int it = base + u * 256 + threadIdx.x;
      ok[u] = it < items;
      const int y = it / W8, x0 = (it - y * W8) << 3;
      ys[u] = y;
      xs[u] = x0;
      partner[u] = ok[u] && (mode == 1 || (mode == 2 && y >= y1 && y < y2 && x0 < x2 && x0 + 8 > x1));
      rb[u] = rp[u] = uint2{0u, 0u};
      if (ok[u]) rb[u] = load8(src_b + (int64_t)y * W, W, x0, gb);
      if (partner[u]) rp[u] = load8(src_p + (int64_t)y * W, W, x0, gp);
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      if (!ok[u]) continue;
      const int y = ys[u], x0 = xs[u];
      float v[8];
      decode8(rb[u], x0, gb, y, tab, v);
      if (partner[u]) {
        float q[8];
        decode8(rp[u], x0, gp, y, tab, q);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          v[j] = mode == 1 ? mix(q[j], wp, v[j], wa) : ((x0 + j >= x1 && x0 + j < x2) ? q[j] : v[j]);
      }
      store8<TO>(dst + (int64_t)y * W + x0, v);
    }
  }
}

// t[b][k] = fl(fl(wp * [k == labels[p]]) + fl(wa * [k == labels[b]])): the labels are compared,
// never used as an index.  Written only when the plan's mode mixes.
__global__ __launch_bounds__(256) void targets_k(const int64_t* __restrict__ labels, const int* __restrict__ plan,
                                                 int B, int K, float* __restrict__ t, int64_t ldt) {
  if (plan[0] == 0) return;
  const float wa = __int_as_float(plan[1]), wp = __int_as_float(plan[2]);
  const int64_t total = (int64_t)B * K;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(idx / K), k = (int)(idx - (int64_t)b * K);
    const int p = b == 0 ? B - 1 : b - 1;
    const float hp = labels[p] == k ? 1.f : 0.f, hb = labels[b] == k ? 1.f : 0.f;
    t[(int64_t)b * ldt + k] = mix(hp, wp, hb, wa);
  }
}

template <typename TO>
void launch(const uint8_t* images, int nhwc, const float* lut, const int* plan, int B, int H, int W, TO* out,
            hipStream_t s) {
  const bool fast = !nhwc && W % 8 == 0 && (int64_t)H * W < (int64_t)1 << 31 && (uintptr_t)images % 8 == 0 &&
                    (uintptr_t)out % 16 == 0 && (int64_t)B * 3 * 8 < (int64_t)1 << 31;
  if (fast) {
    const int items = H * (W / 8);
    const int per = 256 * UNROLL;
    const int chunks = std::min(std::max((items + per - 1) / per, 1), MAX_CHUNKS);
    hipLaunchKernelGGL(plane_k<TO>, dim3(B * 3 * chunks), dim3(256), 0, s, images, lut, plan, B, H, W, chunks, out);
  } else {
    const int64_t total = (int64_t)B * 3 * H * W;
    const int grid = (int)std::min<int64_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(generic_k<TO>, dim3(grid), dim3(256), 0, s, images, nhwc, lut, plan, B, H, W, out);
  }
}
}  // namespace aug

extern "C" int sdp_train_batch_aug(const uint8_t* images, int nhwc, const int64_t* labels, const float* lut,
                                   const int32_t* plan, int B, int H, int W, int dtype_out, void* out, float* targets,
                                   int64_t ldt, int K, void* stream) {
  if (B < 0 || H <= 0 || W <= 0 || (dtype_out != 0 && dtype_out != 1)) return (int)hipErrorInvalidValue;
  if (targets && (K <= 0 || ldt < K)) return (int)hipErrorInvalidValue;
  if (B == 0) return 0;
  if (!images || !lut || !plan || !out || (targets && !labels)) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  if (dtype_out == 0)
    aug::launch<float>(images, nhwc, lut, plan, B, H, W, (float*)out, s);
  else
    aug::launch<bf16_t>(images, nhwc, lut, plan, B, H, W, (bf16_t*)out, s);
  if (targets) {
    const int grid = (int)std::min<int64_t>(((int64_t)B * K + 255) / 256, 2048);
    hipLaunchKernelGGL(aug::targets_k, dim3(grid), dim3(256), 0, s, labels, plan, B, K, targets, ldt);
  }
  return SDP_CHECK_LAUNCH();
}
