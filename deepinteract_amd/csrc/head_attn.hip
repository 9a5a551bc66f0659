// The contact head's regional attention (MultiHeadRegionalAttention, deepinteract_modules.py:1109-1152;
// MHA2D_1 / MHA2D_2 of ResNet2DInputWithOptAttention :1206-1216, :1236-1244) without the reference's
// ninefold Conv3d stretch of q, k and v. For one [128, h, w] image a, 4 heads of 32 channels, d_k 16,
// a 3 x 3 region:
//   q = Wq a, k = Wk a (16 channels each), v = Wv a, per pixel
//   s[hd, p] = 1/4 sum_{j = 4 hd .. 4 hd + 3} q[j, p] k[j, p]              (a pixel's score: its own q.k)
//   out[c, p] = sum over the 9 taps d of softmax_d(s[c / 32, p + d]) v[c, p + d]
// where a tap outside the image has score 0 and value 0 and STAYS in the softmax's denominator.
//  * di_region_scores: x -> s. One lane owns pixels and keeps their 16 + 16 q / k sums in fp32 registers
//    over one pass of the 128 planes (x is read once); the weights are read at wave-uniform addresses
//    (scalar loads). q, k and s stay fp32: they feed an exponential.
//  * di_region_mix: v, s -> out. A block owns a run of pixels (flat, row-major) of one head: every lane
//    forms its pixels' nine weights once -- e_d = exp(s_d - m), m the maximum over the nine taps (outside
//    taps' 0 included), 1 / sum e_d -- and keeps them in registers over the head's 32 planes.
//    v is a torch / di_head_conv convolution: no GEMM here.
// Two geometries, chosen per image by ra_scores_vec / ra_mix_vec from its sizes and pointers alone (so a
// batch item takes the single call's):
//    vector   hw a multiple of the lane's pixels (4 scores, 8 mix) and 16-B aligned pointers (every plane
//             then starts 16-B aligned): 16-B accesses per lane (8 B for the bf16 x of the scores, whose
//             32 accumulators per pixel bound a lane at 4 pixels). The mix stages its run of a plane plus
//             one row and one pixel on either side in LDS (zeros outside the plane), 16 B per lane, and
//             takes the taps from there: v is read once per block, a run's halo a second time by its
//             neighbours, and y is written once with 16-B stores. The next plane's window is in flight
//             (registers, then the other of two LDS windows) while a plane's taps are taken. Needs
//             w <= RM_WMAX (the LDS windows); wider images take the element geometry.
//    element  anything else (an odd hw puts planes on 2-B / 4-B boundaries): one pixel per lane and slot,
//             consecutive lanes on consecutive pixels, element accesses; the mix takes its taps through
//             the cache.
// Both give a pixel the same fp32 operations in the same order. No atomics; no allocation; planes at
// 64-bit offsets. A tap outside the image is read as a finite stand-in and multiplied by a weight of
// exactly 0, so v must be finite.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "common.h"
#include "../../include/deepinteract_amd.h"
#include "head_batch.h"

namespace di {

constexpr int RA_C = 128;       // channels
constexpr int RA_HEADS = 4;
constexpr int RA_DK = 16;       // q / k channels
constexpr int RA_CPH = RA_C / RA_HEADS;
constexpr int RA_THREADS = 256;
constexpr int RS_PX = 4;        // scores: pixels per lane
constexpr int RM_PX = 8;        // mix, vector geometry: pixels per lane
constexpr int RM_NV = 4;        // mix, vector geometry: 16-B vectors of a window per lane, at most
constexpr int RM_WMAX = 2048;   // mix, vector geometry: widest image (two fp32 windows: 48 KiB of LDS)

__host__ __device__ static inline bool ra_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

__host__ __device__ static inline bool ra_scores_vec(const void* x, const float* s, int64_t hw) {
  return (hw % RS_PX) == 0 && ra_al16(x) && ra_al16(s);
}
__host__ __device__ static inline bool ra_mix_vec(const void* v, const void* y, int32_t w, int64_t hw) {
  return (hw % RM_PX) == 0 && w <= RM_WMAX && ra_al16(v) && ra_al16(y);
}
__host__ __device__ static inline int64_t ra_scores_blocks(int64_t hw) {
  const int64_t per = RA_THREADS * RS_PX;   // either geometry: 4 pixels per lane
  return (hw + per - 1) / per;
}
__host__ __device__ static inline int64_t ra_mix_blocks(bool vec, int64_t hw) {
  const int64_t per = RA_THREADS * (vec ? RM_PX : 1);
  return (hw + per - 1) / per;
}
// elements of the mix's LDS window: the run, and a row and a pixel (rounded to a vector) on either side
__host__ __device__ static inline int ra_mix_pad(int32_t w) { return (w + 1 + RM_PX - 1) / RM_PX * RM_PX; }
__host__ __device__ static inline int ra_mix_window(int32_t w) { return RA_THREADS * RM_PX + 2 * ra_mix_pad(w); }
static_assert(RA_THREADS * RM_PX + 2 * ((RM_WMAX + RM_PX) / RM_PX * RM_PX) <= RM_NV * RA_THREADS * RM_PX,
              "a lane stages at most RM_NV vectors of the widest window");
// LDS of a launch: two windows, one being read while the other is filled
static inline size_t ra_mix_lds(int32_t w, size_t es) { return 2 * (size_t)ra_mix_window(w) * es; }

__device__ __forceinline__ float ra_ld(const float* p) { return *p; }
__device__ __forceinline__ float ra_ld(const u16* p) { return __builtin_bit_cast(float, (uint32_t)*p << 16); }
__device__ __forceinline__ void ra_st(float* p, float v) { *p = v; }
__device__ __forceinline__ void ra_st(u16* p, float v) { *p = (u16)(pack_bf16x2(v, 0.f) & 0xffffu); }

typedef unsigned int ra_u32x4 __attribute__((ext_vector_type(4)));

// 8 consecutive elements, 16-B aligned, as raw bits on their way from global memory to LDS
template <typename T>
struct RaRaw;
template <>
struct RaRaw<u16> {
  ra_u32x4 a;
  __device__ __forceinline__ void load(const u16* p) { a = *reinterpret_cast<const ra_u32x4*>(p); }
  __device__ __forceinline__ void zero() { a = (ra_u32x4){0u, 0u, 0u, 0u}; }
  __device__ __forceinline__ void store(u16* p) const { *reinterpret_cast<ra_u32x4*>(p) = a; }
};
template <>
struct RaRaw<float> {
  floatx4 a, b;
  __device__ __forceinline__ void load(const float* p) { a = ld4(p), b = ld4(p + 4); }
  __device__ __forceinline__ void zero() { a = b = (floatx4){0.f, 0.f, 0.f, 0.f}; }
  __device__ __forceinline__ void store(float* p) const { st4(p, a), st4(p + 4, b); }
};
// store of 8 fp32 values
__device__ __forceinline__ void ra_store8(u16* p, const float* v) {
  ra_u32x4 u;
#pragma unroll
  for (int q = 0; q < 4; ++q) u[q] = pack_bf16x2(v[2 * q], v[2 * q + 1]);
  *reinterpret_cast<ra_u32x4*>(p) = u;
}
__device__ __forceinline__ void ra_store8(float* p, const float* v) {
  st4(p, (floatx4){v[0], v[1], v[2], v[3]});
  st4(p + 4, (floatx4){v[4], v[5], v[6], v[7]});
}

// ------------------------------------------------------------------------------------------ scores
// Tile bx of 1024 pixels. VEC: lane t owns pixels 4 t .. 4 t + 3 of the tile (one 16-B / 8-B load per
// plane); element: pixels t, t + 256, t + 512, t + 768 (coalesced element loads). q[j] and k[j] are
// fused multiply-add chains over c = 0 .. 127 from 0; s = 0.25 * (chain over the head's 4 products).
template <typename T, bool VEC, bool ELU>
__device__ __forceinline__ void region_scores_body(const T* __restrict__ x, const float* __restrict__ wq,
                                                   const float* __restrict__ wk, float* __restrict__ s,
                                                   const int64_t hw, const int64_t bx) {
  const int64_t tile0 = bx * (RA_THREADS * RS_PX);
  int64_t p[RS_PX];
#pragma unroll
  for (int k = 0; k < RS_PX; ++k)
    p[k] = VEC ? tile0 + (int64_t)threadIdx.x * RS_PX + k : tile0 + (int64_t)k * RA_THREADS + threadIdx.x;
  if (VEC && p[0] >= hw) return;   // hw is a multiple of 4: a lane's pixels are all inside or all outside
  float q[RS_PX][RA_DK], kk[RS_PX][RA_DK];
#pragma unroll
  for (int k = 0; k < RS_PX; ++k)
#pragma unroll
    for (int j = 0; j < RA_DK; ++j) q[k][j] = kk[k][j] = 0.f;
#pragma unroll 2
  for (int c = 0; c < RA_C; ++c) {
    const T* plane = x + (int64_t)c * hw;
    float a[RS_PX];
    if constexpr (VEC) {
      const floatx4 t = ld4(plane + p[0]);
#pragma unroll
      for (int k = 0; k < RS_PX; ++k) a[k] = t[k];
    } else {
#pragma unroll
      for (int k = 0; k < RS_PX; ++k) a[k] = p[k] < hw ? ra_ld(plane + p[k]) : 0.f;
    }
    if constexpr (ELU) {
#pragma unroll
      for (int k = 0; k < RS_PX; ++k) a[k] = hc_elu(a[k]);
    }
#pragma unroll
    for (int j = 0; j < RA_DK; ++j) {
      const float wqj = wq[j * RA_C + c], wkj = wk[j * RA_C + c];   // wave-uniform
#pragma unroll
      for (int k = 0; k < RS_PX; ++k) {
        q[k][j] = fmaf(wqj, a[k], q[k][j]);
        kk[k][j] = fmaf(wkj, a[k], kk[k][j]);
      }
    }
  }
#pragma unroll
  for (int hd = 0; hd < RA_HEADS; ++hd) {
    float r[RS_PX];
#pragma unroll
    for (int k = 0; k < RS_PX; ++k) {
      float t = 0.f;
#pragma unroll
      for (int j = 0; j < RA_DK / RA_HEADS; ++j) t = fmaf(q[k][4 * hd + j], kk[k][4 * hd + j], t);
      r[k] = 0.25f * t;
    }
    float* out = s + (int64_t)hd * hw;
    if constexpr (VEC) {
      st4(out + p[0], (floatx4){r[0], r[1], r[2], r[3]});
    } else {
#pragma unroll
      for (int k = 0; k < RS_PX; ++k)
        if (p[k] < hw) out[p[k]] = r[k];
    }
  }
}

// One kernel for the single call and the batch (TABLE: blockIdx.z names the item, the x grid is the
// largest item's, a block past its own item's tiles leaves at once; the idiom of k_head_conv).
template <typename T, bool ELU, bool TABLE>
__global__ __launch_bounds__(RA_THREADS) void k_region_scores(const T* __restrict__ x, const float* __restrict__ wq,
                                                              const float* __restrict__ wk, float* __restrict__ s,
                                                              int64_t hw, const di_head_item* __restrict__ items) {
  if constexpr (TABLE) {
    const di_head_item it = items[blockIdx.z];
    hw = (int64_t)it.h * it.w;
    x += (int64_t)RA_C * it.px_off;
    s += (int64_t)RA_HEADS * it.px_off;
  }
  const bool vec = ra_scores_vec(x, s, hw);
  if (TABLE && (int64_t)blockIdx.x >= ra_scores_blocks(hw)) return;
  if (vec) region_scores_body<T, true, ELU>(x, wq, wk, s, hw, blockIdx.x);
  else region_scores_body<T, false, ELU>(x, wq, wk, s, hw, blockIdx.x);
}

// --------------------------------------------------------------------------------------------- mix
// Run bx of one head: pixels [F0, F0 + 256 P) in flat order, lane t owns P consecutive ones (P = 8:
// vector geometry, taps from the LDS window; P = 1: element geometry, taps from global memory). The
// window holds flat pixels [F0 - pad, F0 + 256 P + pad) of the current plane, zeros outside the plane.
template <typename T, bool VEC>
__device__ __forceinline__ void region_mix_body(const T* __restrict__ v, const float* __restrict__ sc,
                                                T* __restrict__ y, const int32_t h, const int32_t w,
                                                const int64_t hw, const int head, const int64_t bx, T* lds) {
  constexpr int P = VEC ? RM_PX : 1;
  const int64_t F0 = bx * (RA_THREADS * P);
  const int64_t f0 = F0 + (int64_t)threadIdx.x * P;
  const bool active = f0 < hw;   // vector geometry: hw is a multiple of 8, all of a lane's pixels or none
  float wt[P][9], inv[P];
  int64_t center_off[9];         // element geometry: a tap's offset from its pixel, 0 when outside
#pragma unroll
  for (int t = 0; t < 9; ++t) center_off[t] = 0;
  if (active) {
    const float* sp = sc + (int64_t)head * hw;
    int64_t row = f0 / w;
    int32_t col = (int32_t)(f0 - row * w);
#pragma unroll
    for (int k = 0; k < P; ++k) {
      const int64_t f = f0 + k;
      float st[9];
      bool ok[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int dy = t / 3 - 1, dx = t % 3 - 1;
        ok[t] = row + dy >= 0 && row + dy < h && col + dx >= 0 && col + dx < w;
        st[t] = ok[t] ? sp[f + (int64_t)dy * w + dx] : 0.f;
        if (!VEC) center_off[t] = ok[t] ? (int64_t)dy * w + dx : 0;
      }
      float m = st[0];
#pragma unroll
      for (int t = 1; t < 9; ++t) m = fmaxf(m, st[t]);   // an outside tap's 0 is among them
      float den = 0.f;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const float e = expf(st[t] - m);
        den += e;                                        // outside taps stay in the denominator
        wt[k][t] = ok[t] ? e : 0.f;
      }
      inv[k] = 1.f / den;
      if (++col == w) col = 0, ++row;
    }
  }
  const int c0 = head * RA_CPH;
  if constexpr (VEC) {
    const int pad = ra_mix_pad(w);
    const int window = ra_mix_window(w);
    const int nvec = window / RM_PX;           // <= RM_NV * RA_THREADS (w <= RM_WMAX)
    const int64_t lo = F0 - pad;
    const int base = (int)(f0 - lo);          // this lane's first pixel in the window
    // The next plane's window is loaded into registers while this plane's taps are taken, and the two
    // windows alternate: one barrier per plane, and the loads' latency lies under the arithmetic.
    RaRaw<T> reg[RM_NV];
    auto fetch = [&](const int c) {
      const T* plane = v + (int64_t)c * hw;
#pragma unroll
      for (int j = 0; j < RM_NV; ++j) {
        const int i = threadIdx.x + j * RA_THREADS;
        const int64_t f = lo + (int64_t)i * RM_PX;
        if (i < nvec && f >= 0 && f < hw) reg[j].load(plane + f);
        else reg[j].zero();
      }
    };
    fetch(c0);
    for (int c = c0, cur = 0; c < c0 + RA_CPH; ++c, cur ^= 1) {
      T* win = lds + cur * window;
#pragma unroll
      for (int j = 0; j < RM_NV; ++j) {
        const int i = threadIdx.x + j * RA_THREADS;
        if (i < nvec) reg[j].store(win + i * RM_PX);
      }
      // also orders this write after every lane's reads of the same window two planes ago: those come
      // before the previous plane's barrier in program order
      __syncthreads();
      if (c + 1 < c0 + RA_CPH) fetch(c + 1);
      if (active) {
        float val[3][P + 2];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int i = 0; i < P + 2; ++i) val[r][i] = ra_ld(win + base + (r - 1) * w + i - 1);
        float out[P];
#pragma unroll
        for (int k = 0; k < P; ++k) {
          float acc = 0.f;
#pragma unroll
          for (int t = 0; t < 9; ++t) acc = fmaf(wt[k][t], val[t / 3][k + t % 3], acc);
          out[k] = acc * inv[k];
        }
        ra_store8(y + (int64_t)c * hw + f0, out);
      }
    }
  } else {
    if (!active) return;
    for (int c = c0; c < c0 + RA_CPH; ++c) {
      const T* at = v + (int64_t)c * hw + f0;
      float acc = 0.f;
#pragma unroll
      for (int t = 0; t < 9; ++t) acc = fmaf(wt[0][t], ra_ld(at + center_off[t]), acc);
      ra_st(y + (int64_t)c * hw + f0, acc * inv[0]);
    }
  }
}

template <typename T, bool TABLE>
__global__ __launch_bounds__(RA_THREADS) void k_region_mix(const T* __restrict__ v, const float* __restrict__ sc,
                                                           T* __restrict__ y, int32_t h, int32_t w,
                                                           const di_head_item* __restrict__ items) {
  extern __shared__ __attribute__((aligned(16))) char ra_smem[];
  if constexpr (TABLE) {
    const di_head_item it = items[blockIdx.z];
    h = it.h, w = it.w;
    v += (int64_t)RA_C * it.px_off;
    y += (int64_t)RA_C * it.px_off;
    sc += (int64_t)RA_HEADS * it.px_off;
  }
  const int64_t hw = (int64_t)h * w;
  const bool vec = ra_mix_vec(v, y, w, hw);
  if (TABLE && (int64_t)blockIdx.x >= ra_mix_blocks(vec, hw)) return;
  if (vec) region_mix_body<T, true>(v, sc, y, h, w, hw, blockIdx.y, blockIdx.x, reinterpret_cast<T*>(ra_smem));
  else region_mix_body<T, false>(v, sc, y, h, w, hw, blockIdx.y, blockIdx.x, nullptr);
}

// --------------------------------------------------------------------------------------- host side
enum { RA_SCORES = 1, RA_MIX = 2 };

static int ra_check(di_dtype dt, const di_region_attn_args* a, int stages) {
  if (!a || (dt != DI_F32 && dt != DI_BF16)) return DI_EINVAL;
  if (a->h < 1 || a->w < 1) return DI_EINVAL;
  const uintptr_t em = dt == DI_BF16 ? 1 : 3;
  if (!a->scores || ((uintptr_t)a->scores & 3) != 0) return DI_EINVAL;
  if (stages & RA_SCORES) {
    if (!a->x || !a->wq || !a->wk) return DI_EINVAL;
    if (((uintptr_t)a->x & em) != 0 || (((uintptr_t)a->wq | (uintptr_t)a->wk) & 3) != 0) return DI_EINVAL;
  }
  if (stages & RA_MIX) {
    if (!a->v || !a->y || a->y == a->v) return DI_EINVAL;
    if ((((uintptr_t)a->v | (uintptr_t)a->y) & em) != 0) return DI_EINVAL;
  }
  const int64_t hw = (int64_t)a->h * a->w;
  if ((hw + RA_THREADS - 1) / RA_THREADS > INT32_MAX) return DI_ERANGE;   // grid.x of the element geometry
  return DI_OK;
}

// the batch's checks and grid: every item on its own sizes and rebased pointers, as the single call
static int ra_batch(di_dtype dt, const di_region_attn_args* args, const di_head_item* items,
                    const di_head_item* items_dev, int32_t count, int stages, unsigned* gx, size_t* lds) {
  if (!args) return DI_EINVAL;
  int rc = hb_check_items(items, items_dev, count);
  if (rc != DI_OK) return rc;
  const int64_t es = dt == DI_BF16 ? 2 : 4;
  *gx = 1, *lds = 0;
  for (int32_t i = 0; i < count; ++i) {
    di_region_attn_args one = *args;
    one.h = items[i].h, one.w = items[i].w;
    const int64_t off = (int64_t)RA_C * items[i].px_off * es;
    if (one.x) one.x = (const char*)one.x + off;
    if (one.v) one.v = (const char*)one.v + off;
    if (one.y) one.y = (char*)one.y + off;
    if (one.scores) one.scores += (int64_t)RA_HEADS * items[i].px_off;
    rc = ra_check(dt, &one, stages);
    if (rc != DI_OK) return rc;
    const int64_t hw = (int64_t)one.h * one.w;
    int64_t n;
    if (stages == RA_SCORES) {
      n = ra_scores_blocks(hw);
    } else {
      const bool vec = ra_mix_vec(one.v, one.y, one.w, hw);
      n = ra_mix_blocks(vec, hw);
      const size_t b = vec ? ra_mix_lds(one.w, (size_t)es) : 0;
      *lds = b > *lds ? b : *lds;
    }
    *gx = (unsigned)n > *gx ? (unsigned)n : *gx;
  }
  return DI_OK;
}

template <bool TABLE>
static void ra_launch_scores(di_dtype dt, const di_region_attn_args* a, dim3 grid, hipStream_t s,
                             const di_head_item* items) {
  const int64_t hw = TABLE ? 0 : (int64_t)a->h * a->w;
  if (dt == DI_BF16) {
    if (a->in_elu)
      hipLaunchKernelGGL((k_region_scores<u16, true, TABLE>), grid, dim3(RA_THREADS), 0, s, (const u16*)a->x, a->wq,
                         a->wk, a->scores, hw, items);
    else
      hipLaunchKernelGGL((k_region_scores<u16, false, TABLE>), grid, dim3(RA_THREADS), 0, s, (const u16*)a->x, a->wq,
                         a->wk, a->scores, hw, items);
  } else {
    if (a->in_elu)
      hipLaunchKernelGGL((k_region_scores<float, true, TABLE>), grid, dim3(RA_THREADS), 0, s, (const float*)a->x,
                         a->wq, a->wk, a->scores, hw, items);
    else
      hipLaunchKernelGGL((k_region_scores<float, false, TABLE>), grid, dim3(RA_THREADS), 0, s, (const float*)a->x,
                         a->wq, a->wk, a->scores, hw, items);
  }
}

template <bool TABLE>
static void ra_launch_mix(di_dtype dt, const di_region_attn_args* a, dim3 grid, size_t lds, hipStream_t s,
                          const di_head_item* items) {
  if (dt == DI_BF16)
    hipLaunchKernelGGL((k_region_mix<u16, TABLE>), grid, dim3(RA_THREADS), lds, s, (const u16*)a->v,
                       (const float*)a->scores, (u16*)a->y, a->h, a->w, items);
  else
    hipLaunchKernelGGL((k_region_mix<float, TABLE>), grid, dim3(RA_THREADS), lds, s, (const float*)a->v,
                       (const float*)a->scores, (float*)a->y, a->h, a->w, items);
}

static int ra_last_error() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DI_OK : (int)e;
}

}  // namespace di

using namespace di;

extern "C" int di_region_attn_check(di_dtype dt, const di_region_attn_args* args) {
  return ra_check(dt, args, RA_SCORES | RA_MIX);
}

extern "C" int di_region_scores(di_dtype dt, const di_region_attn_args* args, void* stream) {
  const int rc = ra_check(dt, args, RA_SCORES);
  if (rc != DI_OK) return rc;
  const int64_t hw = (int64_t)args->h * args->w;
  const int64_t n = ra_scores_blocks(hw);
  ra_launch_scores<false>(dt, args, dim3((unsigned)n), (hipStream_t)stream, nullptr);
  return ra_last_error();
}

extern "C" int di_region_mix(di_dtype dt, const di_region_attn_args* args, void* stream) {
  const int rc = ra_check(dt, args, RA_MIX);
  if (rc != DI_OK) return rc;
  const int64_t hw = (int64_t)args->h * args->w;
  const bool vec = ra_mix_vec(args->v, args->y, args->w, hw);
  const size_t lds = vec ? ra_mix_lds(args->w, dt == DI_BF16 ? 2 : 4) : 0;
  ra_launch_mix<false>(dt, args, dim3((unsigned)ra_mix_blocks(vec, hw), RA_HEADS), lds, (hipStream_t)stream, nullptr);
  return ra_last_error();
}

extern "C" int di_region_scores_batch(di_dtype dt, const di_region_attn_args* args, const di_head_item* items,
                                      const di_head_item* items_dev, int32_t count, void* stream) {
  unsigned gx;
  size_t lds;
  const int rc = ra_batch(dt, args, items, items_dev, count, RA_SCORES, &gx, &lds);
  if (rc != DI_OK) return rc;
  ra_launch_scores<true>(dt, args, dim3(gx, 1, (unsigned)count), (hipStream_t)stream, items_dev);
  return ra_last_error();
}

extern "C" int di_region_mix_batch(di_dtype dt, const di_region_attn_args* args, const di_head_item* items,
                                   const di_head_item* items_dev, int32_t count, void* stream) {
  unsigned gx;
  size_t lds;
  const int rc = ra_batch(dt, args, items, items_dev, count, RA_MIX, &gx, &lds);
  if (rc != DI_OK) return rc;
  ra_launch_mix<true>(dt, args, dim3(gx, RA_HEADS, (unsigned)count), lds, (hipStream_t)stream, items_dev);
  return ra_last_error();
}
