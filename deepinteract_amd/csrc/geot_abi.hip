// GeoT C ABI, host only: the ABI version and the size / fragment layout of the packed weight blobs
// (csrc/layout.h). The launching entry points are in their stage's file (geot.h).
#include "geot.h"

using namespace di;

extern "C" int di_abi_version(void) { return DI_ABI_VERSION; }

extern "C" int64_t di_blob_bytes(int kind, di_dtype dtype, int vec) {
  if (!dtype_ok(dtype)) return -1;
  const int64_t esz = dtype == DI_BF16 ? 2 : 4;
  int64_t blk = 0, nvec = 0;
  switch (kind) {
    case 0: blk = EM_NBLK; nvec = EMV_N; break;
    case 1: blk = IE_NBLK; nvec = IEV_N; break;
    case 2: blk = EL_NBLK; nvec = ELV_N; break;
    case 3: blk = EL_NBLK_FINAL; nvec = ELV_N_FINAL; break;
    case 4: blk = NL_NBLK; nvec = NLV_N; break;
    case 5: blk = NL_NBLK_FINAL; nvec = NLV_N_FINAL; break;
    case 6: blk = EL_NBLK_CONF; nvec = ELV_N_CONF; break;
    default: return -1;
  }
  return vec ? nvec * 4 : blk * BLK * esz;
}

extern "C" int di_blob_layout(int kind, di_dtype dtype) {
  if (!dtype_ok(dtype) || kind < 0 || kind > 6) return -1;
  if (dtype != DI_BF16) return 16;
  if (kind == 1 || kind == 2 || kind == 3) return 32;  // k_init_x32 / k_init_res_x32 / k_edge_x32_ring
  return 16;
}
