// Interface label maps from atom coordinates (di_interface_labels_batch): what the reference gets from
// DIPS' pos_idx (deepinteract_utils.py:567-582, 612: neighbor_def='non_heavy_res', cutoff=6), computed
// from its definition for every complex of a ragged batch with one memset and TWO launches whatever the
// number of complexes. Residue i of chain 0 and residue j of chain 1 interact iff some heavy atom of i
// lies within `cutoff` (<=) of some heavy atom of j:
//
//   labels[i * l2 + j] = 1 iff some atom pair has d2 <= c2, uint8, the map ContactRankOp / ContactAucOp take
//
// The pair test is fixed to the last bit, so that numpy reproduces it: dx = x0 - x1 (likewise dy, dz) and
// d2 = (dx * dx + dy * dy) + dz * dz, every operation rounded to fp32 and none contracted into an fma
// (hipcc contracts device code by default and its __fmul_rn is a plain `*`: if_dist2 switches contraction
// off for its own body), contact iff d2 <= c2 with c2 = (float)((double)cutoff * cutoff) from the host. A
// comparison against NaN is false.
//
// Stage 1 (k_interface_spheres, one thread per residue of either chain) validates res_off and stores a
// bounding sphere per residue as float4 in `work`: the centre c = fp32 mean of the atoms, the radius r =
// the largest COMPUTED distance of an atom from that COMPUTED centre.
// Stage 2 (k_interface_labels, a block per 16 x 64 tile of the map, a wave's lanes along j) skips a pair,
// and labels it 0, only when its spheres prove that no atom pair can pass the test:
//
//     D^ > ((cutoff + r_i) + r_j) * (1 + 2^-18),   D^ = the computed distance of the two centres
//
// Why that is sound (u = 2^-24; the centres are fp32 POINTS, whatever rounding produced them, and the
// radii are measured from those points, so the rounding of the mean does not enter):
//   * a computed squared distance is the true one times (1 + e), |e| <= 5u (a rounded difference, a rounded
//     product and at most two rounded sums of non-negative terms per component; an fma only removes a
//     rounding), and its rounded square root adds at most 2u more: computed distance = true * (1 +- 5u).
//     So every atom is within R = r (1 + 5u) of its centre, and the centres are D >= D^ (1 - 5u) apart.
//   * every atom pair is then at least D - R_i - R_j apart, and a pair whose true distance exceeds
//     cutoff (1 + 4u) fails the test: its computed d2 >= d^2 (1 - 5u) > cutoff^2 (1 + 8u)(1 - 5u) >
//     cutoff^2 (1 + u) >= c2.
//   * so skipping is safe when D^ (1 - 5u) > (cutoff + r_i + r_j)(1 + 5u); the computed sum is within 2u of
//     the true one and its product with the margin within u: (1 + 5u)(1 + 3u) / (1 - 5u) < 1 + 14u, and the
//     margin is 1 + 64u. (Squared distances below the fp32 normal range lose relative accuracy, by less
//     than 1e-19 A in absolute terms.) A NaN anywhere makes the comparison false: the pair is examined.
// Survivors run the atom loop with an early exit, the j side's atoms staged in LDS (a tile's 64 residues
// are one contiguous range of the chain's CSR, taken IF_CAP atoms at a time, so a residue may have any
// number of atoms); a tile none of whose pairs survives stages nothing. No [A0, A1] array is formed.
// Every byte of every map is written exactly once with a plain store, a wave writing 64 consecutive
// bytes of a row: the map takes no memset and no atomics.
//
// Stats (di_interface_stats, the first `count` 16-byte records of `work`, cleared by the call's memset):
// num_pos is a sum of integers (one agent-scope atomic add per wave at most: ballot, then popcount) and
// flags an OR of constants (one atomicOr per wave at most), so both are functions of the input alone,
// whatever the schedule. Every residue's atom range is clamped into [0, A] before use: malformed offsets
// set DI_IF_OFFSETS and read nothing outside xyz; a flagged complex's map is unspecified, but every write
// stays inside it, and its neighbours are not affected.
// Grid (the batch's largest block count, count): block (x, y) works on complex y, whose descriptor it
// reads from the device table, and returns at once when x is past that complex's own block count.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "atom_pairs.h"   // if_dist2, the sphere record, IF_MARGIN, IF_MAX_ATOMS
#include "common.h"
#include "../../include/deepinteract_amd.h"

namespace di {

constexpr int IF_THREADS = 256;
constexpr int IF_WAVES = IF_THREADS / 64;
constexpr int IF_TJ = 64;                        // j residues of a tile: one per lane
constexpr int IF_ROWS = 4;                       // i rows of a tile per wave
constexpr int IF_TI = IF_WAVES * IF_ROWS;        // i residues of a tile
constexpr int IF_CAP = 2048;                     // j-side atoms staged in LDS at a time (24 KiB)
constexpr int64_t IF_MAX_PAIRS = (int64_t)1 << 29;

__global__ __launch_bounds__(IF_THREADS) void k_interface_spheres(const di_interface_item* __restrict__ items,
                                                                  char* __restrict__ work) {
  const di_interface_item& it = items[blockIdx.y];
  const int l1 = it.l1, l2 = it.l2;               // l1 + l2 <= l1 * l2 + 1 <= 2^29
  if ((int64_t)blockIdx.x * IF_THREADS >= (int64_t)l1 + l2) return;
  const int r = (int)blockIdx.x * IF_THREADS + (int)threadIdx.x;
  int f = 0;
  if (r < l1 + l2) {
    const bool second = r >= l1;
    const int res = second ? r - l1 : r, L = second ? l2 : l1, A = second ? it.a1 : it.a0;
    const float* __restrict__ xyz = second ? it.xyz1 : it.xyz0;
    const int32_t* __restrict__ off = second ? it.res_off1 : it.res_off0;
    const int lo_raw = off[res], hi_raw = off[res + 1];
    if ((res == 0 && lo_raw != 0) || hi_raw < lo_raw || (res == L - 1 && hi_raw != A)) f |= DI_IF_OFFSETS;
    const int lo = if_clamp(lo_raw, A);
    int hi = if_clamp(hi_raw, A);
    hi = hi < lo ? lo : hi;
    if (hi_raw == lo_raw) f |= DI_IF_EMPTY;       // a range that clamping emptied is DI_IF_OFFSETS' already
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    bool finite = true;
    for (int a = lo; a < hi; ++a) {
      const float x = xyz[3 * a], y = xyz[3 * a + 1], z = xyz[3 * a + 2];
      finite = finite && if_finite(x) && if_finite(y) && if_finite(z);
      sx += x, sy += y, sz += z;
    }
    if (!finite) f |= DI_IF_NONFINITE;
    const float n = (float)(hi > lo ? hi - lo : 1);
    const float cx = sx / n, cy = sy / n, cz = sz / n;
    float r2 = 0.0f;
    for (int a = lo; a < hi; ++a) r2 = fmaxf(r2, if_dist2(xyz[3 * a], xyz[3 * a + 1], xyz[3 * a + 2], cx, cy, cz));
    reinterpret_cast<float4*>(work + it.work_off)[r] = make_float4(cx, cy, cz, sqrtf(r2));   // sqrt is monotone
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) f |= __shfl_xor(f, m);
  if ((threadIdx.x & 63) == 0 && f) atomicOr(&reinterpret_cast<di_interface_stats*>(work)[blockIdx.y].flags, f);
}

__global__ __launch_bounds__(IF_THREADS) void k_interface_labels(const di_interface_item* __restrict__ items,
                                                                 char* __restrict__ work, float cutoff, float c2) {
  __shared__ float s_xyz[3 * IF_CAP];
  const di_interface_item& it = items[blockIdx.y];
  const int l1 = it.l1, l2 = it.l2, a0 = it.a0, a1 = it.a1;
  const int tiles_j = (l2 + IF_TJ - 1) / IF_TJ;
  if ((int64_t)blockIdx.x >= (int64_t)((l1 + IF_TI - 1) / IF_TI) * tiles_j) return;
  const int ti = (int)blockIdx.x / tiles_j, tj = (int)blockIdx.x - ti * tiles_j;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const float* __restrict__ xyz0 = it.xyz0;
  const float* __restrict__ xyz1 = it.xyz1;
  const int32_t* __restrict__ off0 = it.res_off0;
  const int32_t* __restrict__ off1 = it.res_off1;
  const float4* __restrict__ sph0 = reinterpret_cast<const float4*>(work + it.work_off);
  const float4* __restrict__ sph1 = sph0 + l1;

  const int j_first = tj * IF_TJ, j_end = j_first + IF_TJ < l2 ? j_first + IF_TJ : l2;
  const int j = j_first + lane;
  const bool have_j = j < l2;
  float4 sj = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  int jlo = 0, jhi = 0;                             // this lane's residue: atoms [jlo, jhi) of chain 1
  if (have_j) {
    sj = sph1[j];
    jlo = if_clamp(off1[j], a1), jhi = if_clamp(off1[j + 1], a1);
    jhi = jhi < jlo ? jlo : jhi;
  }
  // the tile's atoms: one range of the CSR (well-formed offsets put every [jlo, jhi) inside it)
  const int t_lo = if_clamp(off1[j_first], a1);
  int t_hi = if_clamp(off1[j_end], a1);
  t_hi = t_hi < t_lo ? t_lo : t_hi;

  const int i_base = ti * IF_TI + wave * IF_ROWS;
  unsigned live = 0;                                // bit s: row i_base + s is past the cull, no contact yet
#pragma unroll
  for (int s = 0; s < IF_ROWS; ++s) {
    const int i = i_base + s;
    if (i < l1 && have_j) {
      const float4 si = sph0[i];
      if (if_may_touch(si, sj, cutoff)) live |= 1u << s;   // NaN: not provably apart
    }
  }
  unsigned hit = 0;
  if (__syncthreads_or((int)live)) {
    for (int base = t_lo; base < t_hi; base += IF_CAP) {     // the same trip count in every thread
      const int n = t_hi - base < IF_CAP ? t_hi - base : IF_CAP;
      __syncthreads();                              // the readers of the chunk before
      for (int k = threadIdx.x; k < 3 * n; k += IF_THREADS) s_xyz[k] = xyz1[3 * (int64_t)base + k];
      __syncthreads();
      const int clo = (jlo > base ? jlo : base) - base;            // >= 0
      const int chi = (jhi < base + n ? jhi : base + n) - base;    // <= n
      if (clo < chi) {
#pragma unroll
        for (int s = 0; s < IF_ROWS; ++s) {
          if (!((live >> s) & 1u)) continue;
          const int i = i_base + s;                 // < l1: live
          const int ilo = if_clamp(off0[i], a0);
          int ihi = if_clamp(off0[i + 1], a0);
          ihi = ihi < ilo ? ilo : ihi;
          bool found = false;
          for (int a = ilo; a < ihi && !found; ++a) {
            const float x0 = xyz0[3 * a], y0 = xyz0[3 * a + 1], z0 = xyz0[3 * a + 2];
            for (int b = clo; b < chi; ++b) {
              if (if_dist2(x0, y0, z0, s_xyz[3 * b], s_xyz[3 * b + 1], s_xyz[3 * b + 2]) <= c2) {
                found = true;
                break;
              }
            }
          }
          if (found) hit |= 1u << s, live &= ~(1u << s);
        }
      }
    }
  }
  int pos = 0;
#pragma unroll
  for (int s = 0; s < IF_ROWS; ++s) {
    const int i = i_base + s;
    if (i >= l1) break;                             // the same in every lane of the wave
    const bool one = (hit >> s) & 1u;
    if (have_j) it.labels[(int64_t)i * l2 + j] = one ? 1 : 0;
    pos += __popcll(__ballot(have_j && one));
  }
  if (lane == 0 && pos)
    __hip_atomic_fetch_add(&reinterpret_cast<di_interface_stats*>(work)[blockIdx.y].num_pos, (int64_t)pos,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

static int64_t if_stats_bytes(int64_t count) { return count * (int64_t)sizeof(di_interface_stats); }

// The workspace from the items' sizes: the stats records of every complex first, then each complex's
// spheres (l1 of chain 0, then l2 of chain 1). off[i] = work_off of item i where off is given; the
// total, or the code of the first item refused.
static int64_t if_layout(const di_interface_item* items, int32_t count, int64_t* off) {
  int64_t at = if_stats_bytes(count);
  for (int32_t i = 0; i < count; ++i) {
    const di_interface_item& it = items[i];
    if (it.l1 < 1 || it.l2 < 1 || it.a0 < 1 || it.a1 < 1) return DI_EINVAL;
    if ((int64_t)it.l1 * (int64_t)it.l2 >= IF_MAX_PAIRS) return DI_ERANGE;
    if (it.a0 >= IF_MAX_ATOMS || it.a1 >= IF_MAX_ATOMS) return DI_ERANGE;
    if (off) off[i] = at;
    at += ((int64_t)it.l1 + (int64_t)it.l2) * (int64_t)sizeof(float4);
  }
  return at;
}

}  // namespace di

using namespace di;

static_assert(sizeof(di_interface_stats) == 16, "the stats records are 16-byte words of the workspace");

extern "C" int64_t di_interface_work_bytes(di_interface_item* items, int32_t count) {
  if (!items || count < 1) return DI_EINVAL;
  if (count > DI_BATCH_MAX) return DI_ERANGE;
  int64_t off[DI_BATCH_MAX];
  const int64_t total = if_layout(items, count, off);
  if (total < 0) return total;
  for (int32_t i = 0; i < count; ++i) items[i].work_off = off[i];
  return total;
}

extern "C" int di_interface_labels_batch_check(const di_interface_item* items, const di_interface_item* items_dev,
                                               int32_t count, float cutoff, const void* work) {
  if (count < 1 || !items || !items_dev || !work) return DI_EINVAL;
  if (count > DI_BATCH_MAX) return DI_ERANGE;
  if (!(cutoff > 0.0f) || !(cutoff <= 3.402823466e+38f)) return DI_EINVAL;   // NaN, Inf, zero, negative
  if ((uintptr_t)work & 15) return DI_EINVAL;
  for (int32_t i = 0; i < count; ++i) {
    const di_interface_item& it = items[i];
    if (!it.xyz0 || !it.res_off0 || !it.xyz1 || !it.res_off1 || !it.labels) return DI_EINVAL;
    if (((uintptr_t)it.xyz0 | (uintptr_t)it.xyz1 | (uintptr_t)it.res_off0 | (uintptr_t)it.res_off1) & 3)
      return DI_EINVAL;
  }
  int64_t off[DI_BATCH_MAX];
  const int64_t total = if_layout(items, count, off);
  if (total < 0) return (int)total;
  for (int32_t i = 0; i < count; ++i)
    if (items[i].work_off != off[i]) return DI_EINVAL;   // not the helper's
  return DI_OK;
}

extern "C" int di_interface_labels_batch(const di_interface_item* items, const di_interface_item* items_dev,
                                         int32_t count, float cutoff, void* work, void* stream) {
  const int rc = di_interface_labels_batch_check(items, items_dev, count, cutoff, work);
  if (rc != DI_OK) return rc;
  int64_t max_res = 1, max_tiles = 1;
  for (int32_t i = 0; i < count; ++i) {
    const int64_t res = (int64_t)items[i].l1 + items[i].l2;
    const int64_t tiles = (int64_t)((items[i].l1 + IF_TI - 1) / IF_TI) * (int64_t)((items[i].l2 + IF_TJ - 1) / IF_TJ);
    max_res = res > max_res ? res : max_res;
    max_tiles = tiles > max_tiles ? tiles : max_tiles;    // < 2^29 / 16 + 2^29 / 64 + 1
  }
  const float c2 = (float)((double)cutoff * (double)cutoff);
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(work, 0, (size_t)if_stats_bytes(count), s);
  if (e != hipSuccess) return (int)e;
  const dim3 block(IF_THREADS);
  hipLaunchKernelGGL(k_interface_spheres, dim3((unsigned)((max_res + IF_THREADS - 1) / IF_THREADS), count), block, 0,
                     s, items_dev, (char*)work);
  e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_interface_labels, dim3((unsigned)max_tiles, count), block, 0, s, items_dev, (char*)work,
                     cutoff, c2);
  e = hipGetLastError();
  return e == hipSuccess ? DI_OK : (int)e;
}
