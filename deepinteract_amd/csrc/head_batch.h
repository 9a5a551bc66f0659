// The ragged batch of head images (include/deepinteract_amd.h, di_head_item): the layout the helper
// fills and the validation every *_batch entry point runs on the host table before it launches.
#pragma once
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

}  // namespace di
