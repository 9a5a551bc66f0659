// Shared by the kernels that ask "do two residues have atoms within a cutoff" for ragged CSR chains
// (contact_interface.hip between two chains, residue_env.hip within one): the bit-fixed fp32 squared
// distance, the bounding-sphere record and the cull's margin. The soundness argument of the cull is in
// contact_interface.hip's header comment; it is written for `d2 <= c2`, and a pair that cannot pass `<=`
// cannot pass `<` either.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace di {

constexpr int32_t IF_MAX_ATOMS = 1 << 24;
constexpr float IF_MARGIN = 1.0f + 0x1p-18f;     // see the soundness argument in contact_interface.hip

// A residue's bounding sphere as both kernels store it in their workspace: float4 (cx, cy, cz, r), the
// centre c = fp32 mean of the atoms, the radius r = the largest COMPUTED distance of an atom from that
// COMPUTED centre.
typedef float4 if_sphere;

// (dx * dx + dy * dy) + dz * dz in fp32, every operation rounded on its own
__device__ __forceinline__ float if_dist2(float x0, float y0, float z0, float x1, float y1, float z1) {
#pragma clang fp contract(off)
  const float dx = x0 - x1, dy = y0 - y1, dz = z0 - z1;
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const float xy = xx + yy;
  return xy + zz;
}

__device__ __forceinline__ int if_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__device__ __forceinline__ bool if_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }   // false for NaN

// true unless the two spheres prove that no atom pair of the residues is within `cutoff`; NaN: examined
__device__ __forceinline__ bool if_may_touch(const if_sphere& si, const if_sphere& sj, float cutoff) {
  const float dist = sqrtf(if_dist2(si.x, si.y, si.z, sj.x, sj.y, sj.z));
  const float reach = ((cutoff + si.w) + sj.w) * IF_MARGIN;
  return !(dist > reach);
}

}  // namespace di
