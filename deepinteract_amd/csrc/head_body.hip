// The contact head's body from one C call (include/deepinteract_amd.h, "the whole contact-head body in
// one call").
//
// di_head_body_batch is a host loop and nothing else: per ResNet the initial projection, per bottleneck
// block the statistics / fold / convolution / SE launches of ResNet._forward_hipconv_batch (head.py), in
// its order, on its buffers, through the same *_batch entry points -- so an image gets the bits the
// Python loop gives it. It gives the C ABI the head, and takes the interpreter out from between the 598
// launches of a forward (5.9 us of host time per launch instead of ~12; the device, at ~11 us per
// kernel on a small image, is the floor either way: DESIGN.md section 8). Everything that could be
// refused is checked before the first launch; after it the only possible failure is a launch error,
// returned as it is.
//
// k_head_logits is the one kernel: phase2_conv(ELU(x)), 128 channels -> 2 classes per pixel. It reads
// 256 B and writes 4 B per pixel and is shaped for the read (measured: 2.3 TB/s at 1000 x 1000, where
// its 128 ELUs per pixel and not HBM set the time): a thread owns 8
// consecutive pixels and walks the 128 channel planes, one 16-B vector of each, 8 planes in flight, the
// two weights of a plane wave-uniform. The reduction runs over planes for a fixed pixel, so -- unlike
// the plane passes of head_ops.hip, where a plane's vectors can simply start at its first aligned
// element -- every plane must be read at the SAME pixels, and plane c starts at element c * hw of a
// 16-B aligned item: aligned only when hw is a multiple of 8. Otherwise a thread loads the two aligned
// vectors its 8 pixels straddle and shifts the 8 elements out of the pair; the shift (c * hw) & 7 is
// the same for every thread. The second vector is loaded only where a needed element lies in it, which
// keeps every load inside the item (its end is 16-B aligned). A wave per block: 512 pixels, so a
// 64 x 64 image still spreads over 8 CUs; no barrier, no LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"
#include "../../include/deepinteract_amd.h"
#include "head_batch.h"

namespace di {

constexpr int HL_THREADS = 64;
constexpr int HL_PX = 8;                      // pixels per thread = one 16-B vector of a plane
constexpr int HL_TILE = HL_THREADS * HL_PX;   // pixels per block
constexpr int HL_C = 128;                     // input channels
constexpr int HL_U = 8;                       // planes in flight per thread

typedef unsigned int u32x4b __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float hl_round(float v) {
  return __builtin_bit_cast(float, (pack_bf16x2(v, 0.f) & 0xffffu) << 16);
}

// One block's 512 pixels of one item: x the item's [128, hw] image, y its [2, hw] logits.
template <bool ALIGNED>
__device__ __forceinline__ void head_logits_body(const u16* __restrict__ x, const int64_t hw,
                                                 const float* __restrict__ w, const float* __restrict__ bias,
                                                 u16* __restrict__ y, const int64_t bx) {
  const int64_t p0 = bx * HL_TILE + (int64_t)threadIdx.x * HL_PX;
  if (p0 >= hw) return;
  const int nv = hw - p0 < HL_PX ? (int)(hw - p0) : HL_PX;  // this thread's pixels inside the image
  float acc0[HL_PX], acc1[HL_PX];
#pragma unroll
  for (int k = 0; k < HL_PX; ++k) acc0[k] = acc1[k] = 0.f;

  for (int c0 = 0; c0 < HL_C; c0 += HL_U) {
    uint64_t q[HL_U][4];
#pragma unroll
    for (int u = 0; u < HL_U; ++u) {
      const int64_t e0 = (int64_t)(c0 + u) * hw;
      const int s = ALIGNED ? 0 : (int)(e0 & 7);
      const u32x4b* v = reinterpret_cast<const u32x4b*>(x + (e0 - s + p0));
      const u32x4b lo = __builtin_nontemporal_load(v);
      u32x4b hi = {0u, 0u, 0u, 0u};
      if (!ALIGNED && s + nv > HL_PX) hi = __builtin_nontemporal_load(v + 1);
      q[u][0] = ((uint64_t)lo[1] << 32) | lo[0];
      q[u][1] = ((uint64_t)lo[3] << 32) | lo[2];
      q[u][2] = ((uint64_t)hi[1] << 32) | hi[0];
      q[u][3] = ((uint64_t)hi[3] << 32) | hi[2];
    }
#pragma unroll
    for (int u = 0; u < HL_U; ++u) {
      const int c = c0 + u;
      uint64_t r0 = q[u][0], r1 = q[u][1];
      if constexpr (!ALIGNED) {  // elements s .. s + 7 of the pair's 16
        const int s = (int)(((int64_t)c * hw) & 7);
        const uint64_t a = s & 4 ? q[u][1] : q[u][0], b = s & 4 ? q[u][2] : q[u][1], d = s & 4 ? q[u][3] : q[u][2];
        const int bs = (s & 3) * 16;
        r0 = bs ? (a >> bs) | (b << (64 - bs)) : a;
        r1 = bs ? (b >> bs) | (d << (64 - bs)) : b;
      }
      const float w0 = w[c], w1 = w[HL_C + c];
#pragma unroll
      for (int k = 0; k < HL_PX; ++k) {
        const uint32_t bits = (uint32_t)((k < 4 ? r0 : r1) >> (16 * (k & 3))) & 0xffffu;
        const float a = hl_round(hc_elu(__builtin_bit_cast(float, bits << 16)));
        acc0[k] = fmaf(w0, a, acc0[k]);
        acc1[k] = fmaf(w1, a, acc1[k]);
      }
    }
  }
  const float b0 = bias ? bias[0] : 0.f, b1 = bias ? bias[1] : 0.f;
#pragma unroll
  for (int k = 0; k < HL_PX; ++k)
    if (k < nv) {
      y[p0 + k] = (u16)(pack_bf16x2(acc0[k] + b0, 0.f) & 0xffffu);
      y[hw + p0 + k] = (u16)(pack_bf16x2(acc1[k] + b1, 0.f) & 0xffffu);
    }
}

// The batch idiom of k_head_conv: blockIdx.z names the item, the x grid is the largest item's, and a
// block past its own item's tiles leaves at once.
__global__ __launch_bounds__(HL_THREADS) void k_head_logits(const u16* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, u16* __restrict__ y,
                                                            const di_head_item* __restrict__ items) {
  const di_head_item it = items[blockIdx.z];
  const int64_t hw = (int64_t)it.h * it.w;
  if ((int64_t)blockIdx.x * HL_TILE >= hw) return;
  x += (int64_t)HL_C * it.px_off;
  y += 2 * it.px_off;
  if ((hw & 7) == 0) head_logits_body<true>(x, hw, w, bias, y, blockIdx.x);
  else head_logits_body<false>(x, hw, w, bias, y, blockIdx.x);
}

static bool hbd_aligned(const void* p, uintptr_t a) { return p && ((uintptr_t)p & (a - 1)) == 0; }

static int hbd_check_block(const di_head_block& b) {
  if (!hbd_aligned(b.w1, 2) || !hbd_aligned(b.w2, 2) || !hbd_aligned(b.w3, 2)) return DI_EINVAL;
  const int norms = !!b.gamma1 + !!b.beta1 + !!b.gamma2 + !!b.beta2 + !!b.gamma3 + !!b.beta3;
  if (norms != 0 && norms != 6) return DI_EINVAL;
  if (!b.se_w1 || !b.se_b1 || !b.se_w2 || !b.se_b2) return DI_EINVAL;
  if (!(b.eps >= 0.f)) return DI_EINVAL;
  if (b.dilation < 1 || b.dilation > 8) return DI_EINVAL;
  return DI_OK;
}

// Everything a launch of the loop below could be refused for (the *_batch entry points' own checks
// included: the item table, and every item's sizes against both kernel sizes' grid limits).
static int hbd_check(di_dtype dt, const di_head_net* nets, int32_t num_nets, const di_head_arena* a) {
  if (dt != DI_BF16 || !nets || !a || num_nets < 1) return DI_EINVAL;
  const void* packed[4] = {a->wide0, a->wide1, a->half0, a->half1};
  for (int i = 0; i < 4; ++i) {
    if (!hbd_aligned(packed[i], 16)) return DI_EINVAL;
    for (int j = 0; j < i; ++j)
      if (packed[i] == packed[j]) return DI_EINVAL;
  }
  if (!hbd_aligned(a->stats, 8) || !hbd_aligned(a->rows, 4)) return DI_EINVAL;
  int rc = hb_check_items(a->items, a->items_dev, a->count);
  if (rc != DI_OK) return rc;
  di_head_conv_args one = {};
  one.x = a->wide0, one.weight = a->wide0, one.y = a->wide1;
  one.cin = 128, one.cout = 64, one.dilation = 1;
  for (int32_t i = 0; i < a->count; ++i)
    for (int ks = 1; ks <= 3; ks += 2) {
      one.h = a->items[i].h, one.w = a->items[i].w, one.ksize = ks;
      rc = di_head_conv_check(dt, &one);
      if (rc != DI_OK) return rc;
    }
  for (int32_t n = 0; n < num_nets; ++n) {
    const di_head_net& net = nets[n];
    if (!net.blocks || net.num_blocks < 1) return DI_EINVAL;
    if (net.proj_w ? !hbd_aligned(net.proj_w, 2) : net.in_elu != 0) return DI_EINVAL;
    for (int32_t b = 0; b < net.num_blocks; ++b) {
      rc = hbd_check_block(net.blocks[b]);
      if (rc != DI_OK) return rc;
    }
  }
  return DI_OK;
}

// the launches of one forward; stops at the first error
struct HeadBodyRun {
  const di_head_arena& a;
  void* stream;
  float *scale, *shift, *mean, *gate;
  int rc = DI_OK;

  HeadBodyRun(const di_head_arena& arena, void* s) : a(arena), stream(s) {
    const int64_t row = (int64_t)a.count * 128;
    scale = a.rows, shift = a.rows + row, mean = a.rows + 2 * row, gate = a.rows + 3 * row;
  }
  bool ok() const { return rc == DI_OK; }
  void conv(const void* x, void* y, const void* w, int cin, int cout, int ks, int dil, bool rows, const float* bias,
            bool elu, bool stats) {
    if (!ok()) return;
    di_head_conv_args k = {};
    k.x = x, k.weight = w, k.y = y;
    k.in_scale = rows ? scale : nullptr, k.in_shift = rows ? shift : nullptr;
    k.bias = bias;
    k.stats = stats ? a.stats : nullptr;
    k.cin = cin, k.cout = cout, k.ksize = ks, k.dilation = dil, k.in_elu = elu ? 1 : 0;
    rc = di_head_conv_batch(DI_BF16, &k, a.items, a.items_dev, a.count, stream);
  }
  void plane_stats(const void* x) {
    if (ok()) rc = di_plane_stats_batch(DI_BF16, x, 128, a.items, a.items_dev, a.count, a.stats, stream);
  }
  void fold_norm(int c, const float* gamma, const float* beta, float eps) {
    if (ok())
      rc = di_head_norm_fold_batch(a.stats, c, a.items, a.items_dev, a.count, gamma, beta, eps, nullptr, scale, shift,
                                   nullptr, stream);
  }
  void fold_mean(const float* bias) {
    if (ok())
      rc = di_head_norm_fold_batch(a.stats, 128, a.items, a.items_dev, a.count, nullptr, nullptr, 0.f, bias, nullptr,
                                   nullptr, mean, stream);
  }
  void se(const di_head_block& b, void* y, const void* res) {
    if (ok()) rc = di_se_gate(mean, b.se_w1, b.se_b1, b.se_w2, b.se_b2, a.count, 128, 8, gate, stream);
    if (ok())
      rc = di_se_scale_add_batch(DI_BF16, y, gate, b.bias3, res, 128, a.items, a.items_dev, a.count, y, stream);
  }
};

}  // namespace di

using namespace di;

extern "C" int di_head_body_batch_check(di_dtype dt, const di_head_net* nets, int32_t num_nets,
                                        const di_head_arena* arena) {
  return hbd_check(dt, nets, num_nets, arena);
}

extern "C" int di_head_body_batch(di_dtype dt, const di_head_net* nets, int32_t num_nets, const di_head_arena* arena,
                                  int32_t* result, void* stream) {
  if (!result) return DI_EINVAL;
  const int rc = hbd_check(dt, nets, num_nets, arena);
  if (rc != DI_OK) return rc;
  HeadBodyRun run(*arena, stream);
  void* wide[2] = {arena->wide0, arena->wide1};
  void *h1 = arena->half0, *h2 = arena->half1;
  int xi = 0;  // wide[xi]: the residual stream; wide[xi ^ 1]: the spare buffer
  for (int32_t n = 0; n < num_nets && run.ok(); ++n) {
    const di_head_net& net = nets[n];
    if (net.proj_w) {
      run.conv(wide[xi], wide[xi ^ 1], net.proj_w, 128, 128, 1, 1, false, net.proj_b, net.in_elu != 0, false);
      xi ^= 1;
    }
    for (int32_t i = 0; i < net.num_blocks && run.ok(); ++i) {
      const di_head_block& b = net.blocks[i];
      void *x = wide[xi], *spare = wide[xi ^ 1];
      if (b.gamma1) {
        run.plane_stats(x);
        run.fold_norm(128, b.gamma1, b.beta1, b.eps);
        run.conv(x, h1, b.w1, 128, 64, 1, 1, true, nullptr, true, true);
        run.fold_norm(64, b.gamma2, b.beta2, b.eps);
        run.conv(h1, h2, b.w2, 64, 64, 3, b.dilation, true, nullptr, true, true);
        run.fold_norm(64, b.gamma3, b.beta3, b.eps);
        run.conv(h2, spare, b.w3, 64, 128, 1, 1, true, nullptr, true, true);
      } else {
        run.conv(x, h1, b.w1, 128, 64, 1, 1, false, b.bias1, true, false);
        run.conv(h1, h2, b.w2, 64, 64, 3, b.dilation, false, b.bias2, true, false);
        run.conv(h2, spare, b.w3, 64, 128, 1, 1, false, nullptr, true, true);
      }
      run.fold_mean(b.bias3);
      run.se(b, spare, x);
      xi ^= 1;
    }
  }
  if (run.ok()) *result = xi;
  return run.rc;
}

extern "C" int di_head_logits_batch(di_dtype dt, const void* x, const float* weight, const float* bias,
                                    const di_head_item* items, const di_head_item* items_dev, int32_t count, void* y,
                                    void* stream) {
  if (dt != DI_BF16 || !hbd_aligned(x, 16) || !hbd_aligned(weight, 4) || !hbd_aligned(y, 2) || y == x) return DI_EINVAL;
  if (((uintptr_t)bias & 3) != 0) return DI_EINVAL;
  const int rc = hb_check_items(items, items_dev, count);
  if (rc != DI_OK) return rc;
  int64_t gx = 1;
  for (int32_t i = 0; i < count; ++i) {
    const int64_t n = ((int64_t)items[i].h * items[i].w + HL_TILE - 1) / HL_TILE;
    if (n > INT32_MAX) return DI_ERANGE;  // grid.x
    gx = n > gx ? n : gx;
  }
  hipLaunchKernelGGL(k_head_logits, dim3((unsigned)gx, 1, (unsigned)count), dim3(HL_THREADS), 0, (hipStream_t)stream,
                     (const u16*)x, weight, bias, (u16*)y, items_dev);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DI_OK : (int)e;
}
