// The ragged batch of head images (include/deepinteract_amd.h, di_head_item): the layout the helper
// fills and the validation every *_batch entry point runs on the host table before it launches; and
// the ELU the head's fused kernels share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/deepinteract_amd.h"

namespace di {

constexpr int64_t HB_MAX_PX = (int64_t)1 << 40;

// an item's room in the batch's statistics buffer: what either convolution or di_plane_stats writes
// for up to 128 channels, rounded to 16 B
static inline int64_t hb_stats_room(int32_t h, int32_t w) {
  return (di_head_conv_stats_bytes(128, h, w) + 15) / 16 * 16;
}

// DI_OK when items[0 .. count) carry the offsets di_head_batch_layout gives their h and w
static inline int hb_check_items(const di_head_item* items, const di_head_item* items_dev, int32_t count) {
  if (count < 1 || !items || !items_dev) return DI_EINVAL;
  if (count > DI_BATCH_MAX) return DI_ERANGE;
  int64_t px = 0, st = 0;
  for (int32_t i = 0; i < count; ++i) {
    if (items[i].h < 1 || items[i].w < 1) return DI_EINVAL;
    if (items[i].px_off != px || items[i].stats_off != st) return DI_EINVAL;
    px += (int64_t)items[i].h * items[i].w;
    st += hb_stats_room(items[i].h, items[i].w);
    if (px > HB_MAX_PX) return DI_ERANGE;
  }
  return DI_OK;
}

// ELU. The negative branch expm1(z) to ~1e-6 relative in a dozen VALU operations (libm's expm1f, at
// several times that, was a quarter of the fused kernels' time): the degree-6 Taylor polynomial for
// z > -0.25 (remainder z^6 / 5040 < 5e-8 relative) and exp(z) - 1 with the hardware exponential below
// it (|result| >= 0.22, so the absolute ~1e-7 is ~5e-7 relative). The value is rounded to bf16
// (2^-9 relative) next.
__device__ __forceinline__ float hc_elu(float z) {
  float p = fmaf(z, 1.f / 720.f, 1.f / 120.f);
  p = fmaf(z, p, 1.f / 24.f);
  p = fmaf(z, p, 1.f / 6.f);
  p = fmaf(z, p, 0.5f);
  p = fmaf(z, p, 1.f);
  p *= z;
  const float e = __expf(z) - 1.f;
  return z > 0.f ? z : (z > -0.25f ? p : e);
}

// v + (v of the lane a DPP pattern pairs this one with), for the reduction over a row of 16 lanes:
// quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror in turn leave every lane of
// the row with the row's sum (after each step the lanes of a quad / half hold one value, and the next
// pattern pairs each lane with one of the other quad / half). Both lanes of a pair add the same two
// numbers, so every lane gets the same bits. Called with all 64 lanes active.
template <int CTRL>
__device__ __forceinline__ double hc_dpp_add(double v) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, CTRL, 0xf, 0xf, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), CTRL, 0xf, 0xf, false);
  return v + __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double hc_row_sum(double v) {
  v = hc_dpp_add<0xB1>(v);
  v = hc_dpp_add<0x4E>(v);
  v = hc_dpp_add<0x141>(v);
  return hc_dpp_add<0x140>(v);
}

}  // namespace di
