// Structure-derived DIPS-Plus node features from a chain's atoms (di_residue_env_batch): the residue
// one-hot, the half-sphere amino-acid composition (HSAAC, get_hsacc dips_plus_utils.py:118-161), the
// coordination number (get_similarity_matrix :84-115, min-max normalised per chain :569) and the amide
// normals (:356-374), for every chain of a ragged batch with one memset and THREE launches whatever the
// number of chains. The definitions, column by column, are in include/deepinteract_amd.h.
//
// The search is contact_interface.hip's -- "do two residues have atoms within a cutoff", a bounding-sphere
// cull, then the atom loop with an early exit and the j side staged in LDS -- within ONE chain and with
// another epilogue. The pair test is if_dist2(...) < c2, STRICT (the reference tests exp(-d2 / 8) > 1e-3).
// The cull takes a length: the host passes cutoff = the smallest fp32 whose fp64 square is >= c2, so cutoff
// >= sqrt(c2) and contact_interface.hip's soundness argument holds as written (a pair farther apart than
// cutoff (1 + 4u) has a computed d2 > cutoff^2 (1 + u) >= c2 and fails `<=`, hence `<`).
//
// Stage 1 (k_env_residues, one thread per residue) validates res_off, role, aa and resname, and stores
//   per residue in `work` three float4: the bounding sphere, (CA, -) and (u, -); it writes the one-hot
//   columns, the amide normal and the [4, 3] backbone row.
// Stage 2 (k_env_pairs, a block per ENV_TI = 16 rows, a wave's lanes along j) walks the chain's 64-residue
//   column tiles; a tile none of whose pairs survives the cull stages nothing. A neighbour j != i is up
//   iff dot(u_i, CA_j - CA_i) > 0 (evaluated uncontracted; zero or NaN: down); i itself is a neighbour
//   whatever its coordinates, and down. Per row 21 up and 21 down counters by amino-acid type in LDS
//   (integer atomic adds) and UN / DN (ballot + popcount): sums of integers, so the result does not
//   depend on the schedule, and there are no float atomics. The 42 quotients of a row are then written
//   with lanes along the columns, cn_raw as int32, and the chain's max CN and max (l - CN) folded into
//   its stats record with one integer atomicMax each per block (the record is cleared by the call's
//   memset, and both values are >= 0).
// Stage 3 (k_env_cn, one thread per residue) writes column 78 from cn_raw and the chain's min and max.
// LDS of stage 2: 24 KiB of staged atoms + 16 x 44 counters + 16 aa codes = 26.8 KiB a block.
//
// Every residue's atom range is clamped into [0, a] before use: malformed offsets set DI_ENV_OFFSETS and
// read nothing outside xyz / role; every write is indexed by a residue < l. Only plain vector stores.
// Grid (the batch's largest block count, count): block (x, y) works on chain y, whose descriptor it
// reads from the device table, and returns at once when x is past that chain's own block count.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "atom_pairs.h"
#include "common.h"
#include "../../include/deepinteract_amd.h"

namespace di {

constexpr int ENV_THREADS = 256;
constexpr int ENV_WAVES = ENV_THREADS / 64;
constexpr int ENV_TJ = 64;                        // j residues of a tile: one per lane
constexpr int ENV_ROWS = 4;                       // i rows per wave
constexpr int ENV_TI = ENV_WAVES * ENV_ROWS;      // i rows per block
constexpr int ENV_CAP = 2048;                     // j-side atoms staged in LDS at a time (24 KiB)
constexpr int ENV_NAA = 21;                       // 'ACDEFGHIKLMNPQRSTVWY-'
constexpr int ENV_CNT = 2 * ENV_NAA + 2;          // up[21], down[21], UN, DN
constexpr int ENV_REC = 3;                        // float4 per residue in work: sphere, CA, u
constexpr int DIPS_W = 106, COL_HSAAC = 36, COL_CN = 78;

struct env_vec {
  float x, y, z;
};

__device__ __forceinline__ env_vec env_sub(env_vec a, env_vec b) {
#pragma clang fp contract(off)
  return {a.x - b.x, a.y - b.y, a.z - b.z};
}

// (a.x * b.x + a.y * b.y) + a.z * b.z, every operation rounded on its own
__device__ __forceinline__ float env_dot(env_vec a, env_vec b) {
#pragma clang fp contract(off)
  const float xx = a.x * b.x, yy = a.y * b.y, zz = a.z * b.z;
  const float xy = xx + yy;
  return xy + zz;
}

__device__ __forceinline__ env_vec env_unit(env_vec v) {
  const float n = sqrtf(env_dot(v, v));
  return {v.x / n, v.y / n, v.z / n};             // the zero vector: NaN, and every dot with it is down
}

// cross(a, b), every operation rounded to fp32 and none contracted: numpy fp32 reproduces the bits
__device__ __forceinline__ env_vec env_cross(env_vec a, env_vec b) {
#pragma clang fp contract(off)
  const float x0 = a.y * b.z, x1 = a.z * b.y;
  const float y0 = a.z * b.x, y1 = a.x * b.z;
  const float z0 = a.x * b.y, z1 = a.y * b.x;
  return {x0 - x1, y0 - y1, z0 - z1};
}

__global__ __launch_bounds__(ENV_THREADS) void k_env_residues(const di_env_item* __restrict__ items,
                                                              char* __restrict__ work) {
  const di_env_item& it = items[blockIdx.y];
  const int L = it.l, A = it.a;
  if ((int64_t)blockIdx.x * ENV_THREADS >= (int64_t)L) return;
  const int res = (int)blockIdx.x * ENV_THREADS + (int)threadIdx.x;
  int f = 0;
  if (res < L) {
    const float* __restrict__ xyz = it.xyz;
    const uint8_t* __restrict__ role = it.role;
    const int lo_raw = it.res_off[res], hi_raw = it.res_off[res + 1];
    if ((res == 0 && lo_raw != 0) || hi_raw < lo_raw || (res == L - 1 && hi_raw != A)) f |= DI_ENV_OFFSETS;
    const int lo = if_clamp(lo_raw, A);
    int hi = if_clamp(hi_raw, A);
    hi = hi < lo ? lo : hi;
    if (hi_raw == lo_raw) f |= DI_ENV_EMPTY;      // a range that clamping emptied is DI_ENV_OFFSETS' already
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    bool finite = true, roles_ok = true;
    env_vec at[6] = {};                           // the last atom seen of every role (at[0] unused)
    int seen[6] = {};
    for (int a = lo; a < hi; ++a) {
      const float x = xyz[3 * (int64_t)a], y = xyz[3 * (int64_t)a + 1], z = xyz[3 * (int64_t)a + 2];
      finite = finite && if_finite(x) && if_finite(y) && if_finite(z);
      sx += x, sy += y, sz += z;
      const int r = role[a];
      roles_ok = roles_ok && r <= DI_ROLE_CB;
#pragma unroll
      for (int q = 1; q <= DI_ROLE_CB; ++q)
        if (r == q) at[q] = {x, y, z}, ++seen[q];
    }
    if (!finite) f |= DI_ENV_NONFINITE;
    const int aa = it.aa[res], col = it.resname[res];
    if (!roles_ok || aa >= ENV_NAA || col >= 20 || seen[DI_ROLE_N] != 1 || seen[DI_ROLE_CA] != 1 ||
        seen[DI_ROLE_C] != 1 || seen[DI_ROLE_O] != 1 || seen[DI_ROLE_CB] > 1)
      f |= DI_ENV_BACKBONE;
    const float n = (float)(hi > lo ? hi - lo : 1);
    const float cx = sx / n, cy = sy / n, cz = sz / n;
    const env_vec ca = at[DI_ROLE_CA];
    float r2 = 0.0f;
    env_vec u = {0.0f, 0.0f, 0.0f};
    int side = 0;
    for (int a = lo; a < hi; ++a) {
      const float x = xyz[3 * (int64_t)a], y = xyz[3 * (int64_t)a + 1], z = xyz[3 * (int64_t)a + 2];
      r2 = fmaxf(r2, if_dist2(x, y, z, cx, cy, cz));
      const int r = role[a];
      if (r == DI_ROLE_OTHER || r >= DI_ROLE_CB) {
        const env_vec e = env_unit(env_sub({x, y, z}, ca));
        u.x += e.x, u.y += e.y, u.z += e.z;
        ++side;
      }
    }
    if (side) {
      const float m = (float)side;
      u = {u.x / m, u.y / m, u.z / m};
    } else {
      const env_vec e0 = env_unit(env_sub(ca, at[DI_ROLE_C])), e1 = env_unit(env_sub(ca, at[DI_ROLE_N]));
      u = {0.5f * (e0.x + e1.x), 0.5f * (e0.y + e1.y), 0.5f * (e0.z + e1.z)};
    }
    float4* __restrict__ rec = reinterpret_cast<float4*>(work + it.work_off) + (int64_t)ENV_REC * res;
    rec[0] = make_float4(cx, cy, cz, sqrtf(r2));  // sqrt is monotone
    rec[1] = make_float4(ca.x, ca.y, ca.z, 0.0f);
    rec[2] = make_float4(u.x, u.y, u.z, 0.0f);
    env_vec am = {0.0f, 0.0f, 0.0f};
    if (seen[DI_ROLE_CB]) am = env_cross(env_sub(ca, at[DI_ROLE_CB]), env_sub(at[DI_ROLE_CB], at[DI_ROLE_N]));
    float* __restrict__ an = it.amide_norm + 3 * (int64_t)res;
    an[0] = am.x, an[1] = am.y, an[2] = am.z;
    float* __restrict__ bb = it.backbone + 12 * (int64_t)res;
#pragma unroll
    for (int q = 0; q < 4; ++q) bb[3 * q] = at[q + 1].x, bb[3 * q + 1] = at[q + 1].y, bb[3 * q + 2] = at[q + 1].z;
    float* __restrict__ dp = it.dips + DIPS_W * (int64_t)res;
    for (int c = 0; c < 20; ++c) dp[c] = c == col ? 1.0f : 0.0f;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) f |= __shfl_xor(f, m);
  if ((threadIdx.x & 63) == 0 && f) atomicOr(&reinterpret_cast<di_env_stats*>(work)[blockIdx.y].flags, f);
}

__global__ __launch_bounds__(ENV_THREADS) void k_env_pairs(const di_env_item* __restrict__ items,
                                                           char* __restrict__ work, float cutoff, float c2) {
  __shared__ float s_xyz[3 * ENV_CAP];
  __shared__ int s_cnt[ENV_TI][ENV_CNT];
  __shared__ int s_aa[ENV_TI];
  const di_env_item& it = items[blockIdx.y];
  const int l = it.l, na = it.a;
  if ((int64_t)blockIdx.x * ENV_TI >= (int64_t)l) return;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const float* __restrict__ xyz = it.xyz;
  const int32_t* __restrict__ off = it.res_off;
  const uint8_t* __restrict__ aa = it.aa;
  const float4* __restrict__ rec = reinterpret_cast<const float4*>(work + it.work_off);
  const int i0 = (int)blockIdx.x * ENV_TI;

  for (int k = threadIdx.x; k < ENV_TI * ENV_CNT; k += ENV_THREADS) (&s_cnt[0][0])[k] = 0;
  if (threadIdx.x < ENV_TI) {
    const int i = i0 + (int)threadIdx.x;
    const int t = i < l ? aa[i] : 0;
    s_aa[threadIdx.x] = t < ENV_NAA ? t : ENV_NAA - 1;
  }
  __syncthreads();

  // this wave's rows: the same in every lane
  const int i_base = i0 + wave * ENV_ROWS;
  float4 sph_i[ENV_ROWS];
  env_vec ca_i[ENV_ROWS], u_i[ENV_ROWS];
  int ilo[ENV_ROWS], ihi[ENV_ROWS];
#pragma unroll
  for (int s = 0; s < ENV_ROWS; ++s) {
    const int i = i_base + s < l ? i_base + s : l - 1;
    sph_i[s] = rec[(int64_t)ENV_REC * i];
    const float4 c = rec[(int64_t)ENV_REC * i + 1], u = rec[(int64_t)ENV_REC * i + 2];
    ca_i[s] = {c.x, c.y, c.z}, u_i[s] = {u.x, u.y, u.z};
    ilo[s] = if_clamp(off[i], na), ihi[s] = if_clamp(off[i + 1], na);
    ihi[s] = ihi[s] < ilo[s] ? ilo[s] : ihi[s];
  }

  const int tiles_j = (l + ENV_TJ - 1) / ENV_TJ;
  for (int tj = 0; tj < tiles_j; ++tj) {           // the same trip count in every thread
    const int j_first = tj * ENV_TJ, j_end = j_first + ENV_TJ < l ? j_first + ENV_TJ : l;
    const int j = j_first + lane;
    const bool have_j = j < l;
    float4 sj = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int jlo = 0, jhi = 0;                           // this lane's residue: atoms [jlo, jhi)
    if (have_j) {
      sj = rec[(int64_t)ENV_REC * j];
      jlo = if_clamp(off[j], na), jhi = if_clamp(off[j + 1], na);
      jhi = jhi < jlo ? jlo : jhi;
    }
    // the tile's atoms: one range of the CSR (well-formed offsets put every [jlo, jhi) inside it)
    const int t_lo = if_clamp(off[j_first], na);
    int t_hi = if_clamp(off[j_end], na);
    t_hi = t_hi < t_lo ? t_lo : t_hi;

    unsigned live = 0, hit = 0;                     // bit s: row i_base + s past the cull / a neighbour
#pragma unroll
    for (int s = 0; s < ENV_ROWS; ++s) {
      const int i = i_base + s;
      if (i < l && have_j) {
        if (i == j) hit |= 1u << s;                 // nb(i, i) whatever the coordinates
        else if (if_may_touch(sph_i[s], sj, cutoff)) live |= 1u << s;   // NaN: not provably apart
      }
    }
    if (__syncthreads_or((int)live)) {
      for (int base = t_lo; base < t_hi; base += ENV_CAP) {    // the same trip count in every thread
        const int n = t_hi - base < ENV_CAP ? t_hi - base : ENV_CAP;
        __syncthreads();                            // the readers of the chunk before
        for (int k = threadIdx.x; k < 3 * n; k += ENV_THREADS) s_xyz[k] = xyz[3 * (int64_t)base + k];
        __syncthreads();
        const int clo = (jlo > base ? jlo : base) - base;            // >= 0
        const int chi = (jhi < base + n ? jhi : base + n) - base;    // <= n
        if (clo < chi) {
#pragma unroll
          for (int s = 0; s < ENV_ROWS; ++s) {
            if (!((live >> s) & 1u)) continue;
            bool found = false;
            for (int a = ilo[s]; a < ihi[s] && !found; ++a) {
              const float x0 = xyz[3 * (int64_t)a], y0 = xyz[3 * (int64_t)a + 1], z0 = xyz[3 * (int64_t)a + 2];
              for (int b = clo; b < chi; ++b) {
                if (if_dist2(x0, y0, z0, s_xyz[3 * b], s_xyz[3 * b + 1], s_xyz[3 * b + 2]) < c2) {
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
    // classify this tile's neighbours: up or down, by the amino-acid type of j
    env_vec ca_j = {0.0f, 0.0f, 0.0f};
    int aa_j = 0;
    if (hit) {
      const float4 c = rec[(int64_t)ENV_REC * j + 1];
      ca_j = {c.x, c.y, c.z};
      aa_j = aa[j];
      aa_j = aa_j < ENV_NAA ? aa_j : ENV_NAA - 1;
    }
#pragma unroll
    for (int s = 0; s < ENV_ROWS; ++s) {
      const int i = i_base + s;
      if (i >= l) break;                            // the same in every lane of the wave
      const bool nb = (hit >> s) & 1u;
      const bool up = nb && i != j && env_dot(u_i[s], env_sub(ca_j, ca_i[s])) > 0.0f;
      int* cnt = s_cnt[wave * ENV_ROWS + s];
      if (nb) atomicAdd(&cnt[(up ? 0 : ENV_NAA) + aa_j], 1);
      const int ups = __popcll(__ballot(up)), all = __popcll(__ballot(nb));
      if (lane == 0) cnt[2 * ENV_NAA] += ups, cnt[2 * ENV_NAA + 1] += all - ups;   // this wave's rows only
    }
  }
  __syncthreads();

  for (int k = threadIdx.x; k < ENV_TI * 2 * ENV_NAA; k += ENV_THREADS) {     // lanes along the columns
    const int r = k / (2 * ENV_NAA), c = k - r * (2 * ENV_NAA);
    const int i = i0 + r;
    if (i >= l) break;
    const int half = c >= ENV_NAA, t = c - half * ENV_NAA;
    const int num = s_cnt[r][c] + (t == s_aa[r] ? 1 : 0), den = 1 + s_cnt[r][2 * ENV_NAA + half];
    it.dips[DIPS_W * (int64_t)i + COL_HSAAC + c] = (float)num / (float)den;
  }
  if (wave == 0) {
    int cn = 0, gap = 0;
    if (lane < ENV_TI && i0 + lane < l) {
      cn = s_cnt[lane][2 * ENV_NAA] + s_cnt[lane][2 * ENV_NAA + 1];     // 1 <= cn <= l
      gap = l - cn;
      it.cn_raw[i0 + lane] = cn;
    }
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) {
      const int c2m = __shfl_xor(cn, m), g2m = __shfl_xor(gap, m);
      cn = cn > c2m ? cn : c2m, gap = gap > g2m ? gap : g2m;
    }
    if (lane == 0) {
      di_env_stats* st = &reinterpret_cast<di_env_stats*>(work)[blockIdx.y];
      atomicMax(&st->cn_max, cn);
      if (gap) atomicMax(&st->cn_min_gap, gap);
    }
  }
}

__global__ __launch_bounds__(ENV_THREADS) void k_env_cn(const di_env_item* __restrict__ items,
                                                        const char* __restrict__ work) {
  const di_env_item& it = items[blockIdx.y];
  const int l = it.l;
  if ((int64_t)blockIdx.x * ENV_THREADS >= (int64_t)l) return;
  const int i = (int)blockIdx.x * ENV_THREADS + (int)threadIdx.x;
  if (i >= l) return;
  const di_env_stats& st = reinterpret_cast<const di_env_stats*>(work)[blockIdx.y];
  const int mx = st.cn_max, mn = l - st.cn_min_gap;
  const int cn = it.cn_raw[i];
  it.dips[DIPS_W * (int64_t)i + COL_CN] = mx == mn ? 0.0f : (float)(cn - mn) / (float)(mx - mn);
}

static int64_t env_stats_bytes(int64_t count) { return count * (int64_t)sizeof(di_env_stats); }

// The workspace from the items' sizes: the stats records of every chain first, then each chain's
// ENV_REC float4 per residue. off[i] = work_off of item i where off is given; the total, or the code
// of the first item refused.
static int64_t env_layout(const di_env_item* items, int32_t count, int64_t* off) {
  int64_t at = env_stats_bytes(count);
  for (int32_t i = 0; i < count; ++i) {
    const di_env_item& it = items[i];
    if (it.l < 1 || it.a < 1) return DI_EINVAL;
    if (it.a >= IF_MAX_ATOMS || it.l >= IF_MAX_ATOMS) return DI_ERANGE;
    if (off) off[i] = at;
    at += (int64_t)it.l * ENV_REC * (int64_t)sizeof(float4);
  }
  return at;
}

}  // namespace di

using namespace di;

static_assert(sizeof(di_env_stats) == 16, "the stats records are 16-byte words of the workspace");

extern "C" int64_t di_residue_env_work_bytes(di_env_item* items, int32_t count) {
  if (!items || count < 1) return DI_EINVAL;
  if (count > DI_BATCH_MAX) return DI_ERANGE;
  int64_t off[DI_BATCH_MAX];
  const int64_t total = env_layout(items, count, off);
  if (total < 0) return total;
  for (int32_t i = 0; i < count; ++i) items[i].work_off = off[i];
  return total;
}

extern "C" int di_residue_env_batch_check(const di_env_item* items, const di_env_item* items_dev, int32_t count,
                                          float c2, const void* work) {
  if (count < 1 || !items || !items_dev || !work) return DI_EINVAL;
  if (count > DI_BATCH_MAX) return DI_ERANGE;
  if (!(c2 > 0.0f) || !(c2 <= 3.402823466e+38f)) return DI_EINVAL;   // NaN, Inf, zero, negative
  if ((uintptr_t)work & 15) return DI_EINVAL;
  for (int32_t i = 0; i < count; ++i) {
    const di_env_item& it = items[i];
    if (!it.xyz || !it.res_off || !it.role || !it.aa || !it.resname || !it.dips || !it.amide_norm ||
        !it.backbone || !it.cn_raw)
      return DI_EINVAL;
    if (((uintptr_t)it.xyz | (uintptr_t)it.res_off | (uintptr_t)it.dips | (uintptr_t)it.amide_norm |
         (uintptr_t)it.backbone | (uintptr_t)it.cn_raw) & 3)
      return DI_EINVAL;
  }
  int64_t off[DI_BATCH_MAX];
  const int64_t total = env_layout(items, count, off);
  if (total < 0) return (int)total;
  for (int32_t i = 0; i < count; ++i)
    if (items[i].work_off != off[i]) return DI_EINVAL;   // not the helper's
  return DI_OK;
}

extern "C" int di_residue_env_batch(const di_env_item* items, const di_env_item* items_dev, int32_t count, float c2,
                                    void* work, void* stream) {
  const int rc = di_residue_env_batch_check(items, items_dev, count, c2, work);
  if (rc != DI_OK) return rc;
  int64_t max_l = 1;
  for (int32_t i = 0; i < count; ++i) max_l = items[i].l > max_l ? items[i].l : max_l;   // < 2^24
  // the cull's length: the smallest fp32 whose square is >= c2 (sqrt of a finite fp32 is far from overflow)
  float cutoff = (float)sqrt((double)c2);
  if ((double)cutoff * (double)cutoff < (double)c2) cutoff = nextafterf(cutoff, INFINITY);
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(work, 0, (size_t)env_stats_bytes(count), s);
  if (e != hipSuccess) return (int)e;
  const dim3 block(ENV_THREADS), per_res((unsigned)((max_l + ENV_THREADS - 1) / ENV_THREADS), count);
  hipLaunchKernelGGL(k_env_residues, per_res, block, 0, s, items_dev, (char*)work);
  e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_env_pairs, dim3((unsigned)((max_l + ENV_TI - 1) / ENV_TI), count), block, 0, s, items_dev,
                     (char*)work, cutoff, c2);
  e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_env_cn, per_res, block, 0, s, items_dev, (const char*)work);
  e = hipGetLastError();
  return e == hipSuccess ? DI_OK : (int)e;
}
