// Contact-head convolutions: the 1x1 and dilated 3x3 convolutions of the
// dilated-ResNet head (ResNet.forward, deepinteract_modules.py:1075-1095) as an implicit GEMM on
// v_mfma_f32_16x16x32_bf16, for one [Cin, H, W] NCHW bf16 image, with the norm + ELU in front of the
// convolution and the statistics of the norm behind it fused in:
//
//   y[co] = bias[co] + sum over (ci, tap) of w[co][ci][tap] * a[ci][pixel + tap offset]
//   a     = in_elu ? ELU(x * in_scale[ci] + in_shift[ci]) : x * in_scale[ci] + in_shift[ci]
//
// a is computed in fp32 and rounded to bf16 (RNE) as it enters LDS -- the rounding the unfused path
// has when di_inorm_elu stores its output -- and a tap outside the image contributes 0 (the zero
// padding applies AFTER the transform). fp32 accumulation, one RNE rounding at the store.
//
// Shape of the product: D[co][pixel] = W[co][k] . A[k][pixel], the weights as the MFMA's A operand
// (row = co = lane & 15), the pixels as its B operand (col = pixel = lane & 15), k = 32 input channels
// per step: lane l holds W[co][8 (l >> 4) + j] and A[8 (l >> 4) + j][pixel] (cdna_hip_programming.md §3).
// In NCHW the k index (the channel) is the strided one, so the LDS fill transposes: a thread gathers 8
// channels of one pixel (8 loads, each coalesced over the wave's pixels), transforms, packs and writes
// one 16-B LDS vector; a B fragment is then one 16-B LDS read and the wave's 64 reads are one
// contiguous KiB. Weights come as the module's [Cout, Cin, k, k] tensor; the LDS fill puts them in
// fragment order.
//
// A block of 4 waves owns 256 output pixels x all Cout channels (wave: 4 groups of 16 pixels x Cout / 16
// blocks = 16 or 32 accumulator tiles) and loops over Cin in chunks of 32:
//   1x1: the image is a flat run of hw pixels; the tile is 256 consecutive ones.
//   3x3: the tile is 16 x 16 pixels; LDS holds its (16 + 2 d)^2 halo, and tap (ty, tx) is the 1x1
//        product over the halo shifted by (ty d, tx d): a dilated 3x3 is nine shifted 1x1 products.
//        Three instantiations by LDS size (d <= 2, <= 4, <= 8: 63 / 74 / 102 KiB for Cout = 64).
// Plane offsets (channel * hw) are 64-bit. Ordinary launches; no block waits for another.
// di_head_conv_batch runs the same kernel over a packed ragged batch of images in one launch (given the
// batch's item table, a block of k_head_conv rebases its pointers and takes h / w from its item; the
// layout and the item table: include/deepinteract_amd.h).
//
// Statistics (optional): per output channel (sum y, sum y^2) of the values AS STORED (after the bf16
// rounding). A thread sums its 4 pixels in fp32 (as k_inorm_stats sums a vector's elements); from
// there on everything is fp64: 16 lanes by DPP row exchanges, 4 waves through LDS in wave order, one partial
// per block and channel. No atomics: di_head_norm_fold adds the partials in a fixed order, so two runs
// give the same bits. Layout of the statistics buffer: see include/deepinteract_amd.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "common.h"
#include "../../include/deepinteract_amd.h"
#include "head_batch.h"

namespace di {

constexpr int HC_THREADS = 256;
constexpr int HC_TILE = 16;   // 3x3: the output tile is HC_TILE x HC_TILE pixels
constexpr int HC_PIX = 256;   // output pixels per block (both kernel sizes)
constexpr int HC_KC = 32;     // input channels per chunk = one MFMA k-step
constexpr int HC_MAX_CIN = 256;

struct HcArgs {
  const u16* x;
  const u16* w;
  const float* in_scale;
  const float* in_shift;
  const float* bias;
  u16* y;
  double* stats;  // NULL, or the statistics buffer (2 header doubles, then the partials)
  int64_t hw;
  int32_t cin, h, wd, dil, in_elu;
};

// hc_elu (the fused ELU): head_batch.h, shared with the logits kernel of head_body.hip
// hc_row_sum (the statistics' sum over a row of 16 lanes): head_batch.h, shared with head_conv_f32.hip
__device__ __forceinline__ float hc_f32(u16 b) { return __builtin_bit_cast(float, (uint32_t)b << 16); }

// blocks per CU the register budget is set for: what the LDS tile leaves room for, at most 2
constexpr int hc_blocks_per_cu(int ks, int cout, int dmax) {
  return ks == 1 || (cout == 64 && dmax <= 4) ? 2 : 1;
}

// One block's work, for block (bx, by) of an image's own gx x gy grid (1x1: gy = 1). A single call and a
// batch both run exactly this, so an image's output and statistics partials do not depend on which of
// the two launched it.
template <int KS, int COUT, int DMAX>
__device__ __forceinline__ void head_conv_body(const HcArgs& a, const int bx, const int by, const int gx,
                                               const int gy) {
  constexpr int TAPS = KS * KS;
  constexpr int NCB = COUT / 16;
  constexpr int HALO = HC_TILE + 2 * DMAX;
  constexpr int NPX = KS == 3 ? HALO * HALO : HC_PIX;
  constexpr int NW_ELEMS = COUT * HC_KC * TAPS;  // weight elements of a chunk
  constexpr int WB = KS == 3 ? 24 : 8;           // weight loads in flight per thread
  constexpr int XB = 4;                          // pixel items (8 loads each) in flight per thread
  static_assert(NW_ELEMS % (HC_THREADS * WB) == 0, "whole weight batches");
  static_assert(NPX * HC_KC * 2 >= 4 * COUT * 2 * 8, "the statistics' wave partials reuse the pixel tile");
  __shared__ __attribute__((aligned(16))) u16 wl[TAPS * COUT * HC_KC];  // [tap][cout block][lane][8]
  __shared__ __attribute__((aligned(16))) u16 xl[NPX * HC_KC];         // [pixel][32 channels]
  __shared__ float tr[2][HC_MAX_CIN];                                    // in_scale, in_shift
  __shared__ float bl[COUT];                                             // bias

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p = lane & 15, g = lane >> 4;
  const int d = KS == 3 ? a.dil : 0;
  const int halo = HC_TILE + 2 * d;               // <= HALO: the host picks DMAX >= d
  const int npx = KS == 3 ? halo * halo : HC_PIX;
  const int y0 = by * HC_TILE, x0 = bx * HC_TILE;  // 3x3
  const int64_t base = (int64_t)bx * HC_PIX;  // 1x1
  const int64_t hw = a.hw;

  for (int c = tid; c < a.cin; c += HC_THREADS) {
    tr[0][c] = a.in_scale ? a.in_scale[c] : 1.f;
    tr[1][c] = a.in_shift ? a.in_shift[c] : 0.f;
  }
  // from LDS in the epilogue: a global load between the stores would wait for every store before it
  if (tid < COUT) bl[tid] = a.bias ? a.bias[tid] : 0.f;

  floatx4 acc[4][NCB];
#pragma unroll
  for (int pb = 0; pb < 4; ++pb)
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) acc[pb][cb] = (floatx4){0.f, 0.f, 0.f, 0.f};

  for (int c0 = 0; c0 < a.cin; c0 += HC_KC) {
    __syncthreads();  // the previous chunk's fragments are read (first pass: tr is written)
    // weights of this chunk in fragment order: for one co the chunk's 32 x TAPS elements are
    // contiguous. Loads in batches of WB with all of a batch in flight before its LDS writes.
    for (int e0 = tid; e0 < NW_ELEMS; e0 += HC_THREADS * WB) {
      u16 v[WB];
#pragma unroll
      for (int u = 0; u < WB; ++u) {
        const int e = e0 + u * HC_THREADS;
        const int co = e / (HC_KC * TAPS), r = e % (HC_KC * TAPS);
        v[u] = a.w[((int64_t)co * a.cin + c0) * TAPS + r];
      }
#pragma unroll
      for (int u = 0; u < WB; ++u) {
        const int e = e0 + u * HC_THREADS;
        const int co = e / (HC_KC * TAPS), r = e % (HC_KC * TAPS), ci = r / TAPS, t = r % TAPS;
        wl[(((t * NCB + (co >> 4)) * 64) + (co & 15) + 16 * (ci >> 3)) * 8 + (ci & 7)] = v[u];
      }
    }
    // pixels: item (channel group gq of 8, pixel px); consecutive lanes take consecutive pixels.
    // XB items per pass, their 8 XB loads issued together (an item outside the image or past the
    // tile loads pixel 0 instead and is zeroed / dropped afterwards, so no load sits behind a branch)
    const int total = 4 * npx;
    for (int i0 = tid; i0 < total; i0 += HC_THREADS * XB) {
      u16 raw[XB][8];
      bool valid[XB];
      int gqs[XB], pxs[XB];
#pragma unroll
      for (int u = 0; u < XB; ++u) {
        const int i = i0 + u * HC_THREADS;
        const int ii = i < total ? i : 0;
        const int gq = ii / npx, px = ii - gq * npx;
        int64_t gp;
        if constexpr (KS == 3) {
          const int hy = px / halo, hx = px - hy * halo;
          const int gy = y0 - d + hy, gx = x0 - d + hx;
          valid[u] = gy >= 0 && gy < a.h && gx >= 0 && gx < a.wd;
          gp = (int64_t)gy * a.wd + gx;
        } else {
          gp = base + px;
          valid[u] = gp < hw;
        }
        gp = valid[u] ? gp : 0;
        gqs[u] = gq;
        pxs[u] = px;
#pragma unroll
        for (int j = 0; j < 8; ++j) raw[u][j] = a.x[(int64_t)(c0 + 8 * gq + j) * hw + gp];
      }
#pragma unroll
      for (int u = 0; u < XB; ++u) {
        float f[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int c = c0 + 8 * gqs[u] + j;
          const float z = fmaf(hc_f32(raw[u][j]), tr[0][c], tr[1][c]);
          f[j] = a.in_elu ? hc_elu(z) : z;
        }
        uint4 pk = {0u, 0u, 0u, 0u};  // outside the image: zero AFTER the transform
        if (valid[u])
          pk = (uint4){pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]),
                       pack_bf16x2(f[6], f[7])};
        if (i0 + u * HC_THREADS < total) *reinterpret_cast<uint4*>(xl + pxs[u] * HC_KC + gqs[u] * 8) = pk;
      }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < TAPS; ++t) {
      bf16x8 bf[4];
#pragma unroll
      for (int pb = 0; pb < 4; ++pb) {
        const int rb = wave * 4 + pb;
        const int px = KS == 3 ? (rb + (t / 3) * d) * halo + (t % 3) * d + p : rb * 16 + p;
        bf[pb] = *reinterpret_cast<const bf16x8*>(xl + px * HC_KC + g * 8);
      }
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        const bf16x8 af = *reinterpret_cast<const bf16x8*>(wl + ((t * NCB + cb) * 64 + lane) * 8);
#pragma unroll
        for (int pb = 0; pb < 4; ++pb)
          acc[pb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf[pb], acc[pb][cb], 0, 0, 0);
      }
    }
  }

  // epilogue: accumulator tile (pb, cb), register r = channel 16 cb + 4 g + r at pixel p of group pb
  bool valid[4];
  int64_t gp[4];
#pragma unroll
  for (int pb = 0; pb < 4; ++pb) {
    const int rb = wave * 4 + pb;
    if constexpr (KS == 3) {
      const int gy = y0 + rb, gx = x0 + p;
      valid[pb] = gy < a.h && gx < a.wd;
      gp[pb] = (int64_t)gy * a.wd + gx;
    } else {
      gp[pb] = base + rb * 16 + p;
      valid[pb] = gp[pb] < hw;
    }
  }
  const bool stats = a.stats != nullptr;
  double* red = reinterpret_cast<double*>(xl);  // [wave][COUT][2]
  if (stats) __syncthreads();                   // every wave is done reading xl
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = 16 * cb + 4 * g + r;
      const float bc = bl[co];
      float fs = 0.f, fss = 0.f;  // this thread's 4 pixels in fp32, then fp64
#pragma unroll
      for (int pb = 0; pb < 4; ++pb) {
        const uint32_t bits = pack_bf16x2(acc[pb][cb][r] + bc, 0.f) & 0xffffu;
        if (valid[pb]) {
          a.y[(int64_t)co * hw + gp[pb]] = (u16)bits;
          const float v = __builtin_bit_cast(float, bits << 16);
          fs += v;
          fss = fmaf(v, v, fss);
        }
      }
      if (stats) {
        const double s = hc_row_sum((double)fs), ss = hc_row_sum((double)fss);  // the channel's 16 lanes (pixels)
        if (p == 0) {
          red[(wave * COUT + co) * 2 + 0] = s;
          red[(wave * COUT + co) * 2 + 1] = ss;
        }
      }
    }
  if (stats) {
    __syncthreads();
    const int64_t nblk = (int64_t)gx * gy;
    const int64_t blk = (int64_t)by * gx + bx;
    double* part = a.stats + 2;
    if (tid < COUT) {
      double s = 0.0, ss = 0.0;
      for (int w = 0; w < HC_THREADS / 64; ++w) {
        s += red[(w * COUT + tid) * 2 + 0];
        ss += red[(w * COUT + tid) * 2 + 1];
      }
      part[((int64_t)tid * nblk + blk) * 2 + 0] = s;
      part[((int64_t)tid * nblk + blk) * 2 + 1] = ss;
    }
    if (blk == 0 && tid == 0) {
      reinterpret_cast<int64_t*>(a.stats)[0] = nblk;
      reinterpret_cast<int64_t*>(a.stats)[1] = 0;
    }
  }
}

// One kernel serves the single call and the batch. For a single call (TABLE = false, items unused) it
// uses `a` as the host filled it. For a batch, blockIdx.z names the item: a.x, a.y, a.stats, a.in_scale
// and a.in_shift are the packed buffers' bases, which the block rebases to its item, and h, wd, hw come
// from the item; the x / y grid is the largest item's, and a block past its own item's tile count leaves
// at once -- as a whole, before any barrier. (The project's idiom, as the rank / AUC batches: against a
// prefix table of tiles it needs no second table and no search per block, and a block that only reads
// its item and leaves costs far less than the launch it saves; a batch of one large and many small
// images starts at most (count - 1) x the large one's tiles of them.) The image's own grid gx x gy comes
// from h / wd / hw in both cases (in a single call it is the launch's grid, so no block leaves).
// TABLE is a template parameter -- the call kind is known where the launch is written -- and not a test
// of `items`: behind such a test the single call loads its arguments in two dependent rounds (the
// table pointer, a branch, then the rest), and the whole head at 1000 x 1000 measured 0.1 - 0.2 % slower,
// just outside the window of the kernels before the merge.
template <int KS, int COUT, int DMAX, bool TABLE>
__global__ __launch_bounds__(HC_THREADS, hc_blocks_per_cu(KS, COUT, DMAX)) void k_head_conv(
    HcArgs a, const di_head_item* __restrict__ items) {
  if constexpr (TABLE) {
    const int z = blockIdx.z;
    const int64_t px = items[z].px_off;
    a.h = items[z].h;
    a.wd = items[z].w;
    a.hw = (int64_t)a.h * a.wd;
    a.x += (int64_t)a.cin * px;
    a.y += (int64_t)COUT * px;
    a.stats = a.stats ? reinterpret_cast<double*>(reinterpret_cast<char*>(a.stats) + items[z].stats_off) : nullptr;
    a.in_scale = a.in_scale ? a.in_scale + (int64_t)z * a.cin : nullptr;
    a.in_shift = a.in_shift ? a.in_shift + (int64_t)z * a.cin : nullptr;
  }
  int gx, gy;
  if constexpr (KS == 3) {
    gx = (a.wd + HC_TILE - 1) / HC_TILE;
    gy = (a.h + HC_TILE - 1) / HC_TILE;
  } else {
    gx = (int)((a.hw + HC_PIX - 1) / HC_PIX);
    gy = 1;
  }
  if (TABLE && ((int)blockIdx.x >= gx || (int)blockIdx.y >= gy)) return;
  head_conv_body<KS, COUT, DMAX>(a, blockIdx.x, blockIdx.y, gx, gy);
}

// blocks of a launch = partials per channel
static int64_t hc_blocks(int ksize, int64_t h, int64_t w) {
  if (ksize == 3) return ((h + HC_TILE - 1) / HC_TILE) * ((w + HC_TILE - 1) / HC_TILE);
  return (h * w + HC_PIX - 1) / HC_PIX;
}

static int hc_check(di_dtype dt, const di_head_conv_args* a) {
  if (!a || dt != DI_BF16) return DI_EINVAL;
  if (!a->x || !a->weight || !a->y || a->y == a->x) return DI_EINVAL;
  if (a->cin != 64 && a->cin != 128 && a->cin != 256) return DI_EINVAL;
  if (a->cout != 64 && a->cout != 128) return DI_EINVAL;
  if (a->ksize != 1 && a->ksize != 3) return DI_EINVAL;
  if (a->dilation < 1 || a->dilation > 8) return DI_EINVAL;
  if (a->h < 1 || a->w < 1) return DI_EINVAL;
  if ((((uintptr_t)a->x | (uintptr_t)a->weight | (uintptr_t)a->y) & 1) != 0) return DI_EINVAL;
  if (((uintptr_t)a->stats & 7) != 0) return DI_EINVAL;
  if (a->ksize == 3 && ((a->h + HC_TILE - 1) / HC_TILE) > 65535) return DI_ERANGE;  // grid.y
  if (a->ksize == 1 && hc_blocks(1, a->h, a->w) > INT32_MAX) return DI_ERANGE;      // grid.x
  return DI_OK;
}

template <int KS, int COUT, int DMAX, bool TABLE>
static void hc_launch(const HcArgs& k, dim3 grid, hipStream_t s, const di_head_item* items) {
  hipLaunchKernelGGL((k_head_conv<KS, COUT, DMAX, TABLE>), grid, dim3(HC_THREADS), 0, s, k, items);
}

// the kernel's arguments from the call's, for an image of h x w pixels (a batch: 0 x 0, every block
// takes its item's)
static HcArgs hc_args(const di_head_conv_args* args, int32_t h, int32_t w) {
  HcArgs k;
  k.x = (const u16*)args->x;
  k.w = (const u16*)args->weight;
  k.in_scale = args->in_scale;
  k.in_shift = args->in_shift;
  k.bias = args->bias;
  k.y = (u16*)args->y;
  k.stats = (double*)args->stats;
  k.hw = (int64_t)h * w;
  k.cin = args->cin;
  k.h = h;
  k.wd = w;
  k.dil = args->dilation;
  k.in_elu = args->in_elu ? 1 : 0;
  return k;
}

// the instantiation for (ksize, cout, dilation); items: the batch's device table (TABLE), or NULL
template <bool TABLE>
static void hc_dispatch(const HcArgs& k, int ksize, int cout, int d, dim3 grid, hipStream_t s,
                        const di_head_item* items) {
  const bool wide = cout == 128;
  if (ksize == 1) {
    if (wide) hc_launch<1, 128, 0, TABLE>(k, grid, s, items);
    else hc_launch<1, 64, 0, TABLE>(k, grid, s, items);
  } else if (d <= 2) {
    if (wide) hc_launch<3, 128, 2, TABLE>(k, grid, s, items);
    else hc_launch<3, 64, 2, TABLE>(k, grid, s, items);
  } else if (d <= 4) {
    if (wide) hc_launch<3, 128, 4, TABLE>(k, grid, s, items);
    else hc_launch<3, 64, 4, TABLE>(k, grid, s, items);
  } else {
    if (wide) hc_launch<3, 128, 8, TABLE>(k, grid, s, items);
    else hc_launch<3, 64, 8, TABLE>(k, grid, s, items);
  }
}

}  // namespace di

using namespace di;

extern "C" int di_head_conv_check(di_dtype dt, const di_head_conv_args* args) { return hc_check(dt, args); }

extern "C" int64_t di_head_conv_stats_bytes(int32_t cout, int32_t h, int32_t w) {
  if (cout < 1 || h < 1 || w < 1) return DI_EINVAL;
  // either kernel size's block count, and never under what di_plane_stats writes
  int64_t n = hc_blocks(1, h, w);
  const int64_t n3 = hc_blocks(3, h, w);
  n = n > n3 ? n : n3;
  n = n > 64 ? n : 64;
  return 16 + (int64_t)cout * n * 2 * (int64_t)sizeof(double);
}

extern "C" int di_head_conv(di_dtype dt, const di_head_conv_args* args, void* stream) {
  const int rc = hc_check(dt, args);
  if (rc != DI_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid = args->ksize == 1 ? dim3((unsigned)hc_blocks(1, args->h, args->w))
                                     : dim3((args->w + HC_TILE - 1) / HC_TILE, (args->h + HC_TILE - 1) / HC_TILE);
  hc_dispatch<false>(hc_args(args, args->h, args->w), args->ksize, args->cout, args->dilation, grid, s, nullptr);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DI_OK : (int)e;
}

extern "C" int di_head_batch_layout(di_head_item* items, int32_t count, int64_t* total_px, int64_t* stats_bytes) {
  if (!items || !total_px || !stats_bytes || count < 1) return DI_EINVAL;
  if (count > DI_BATCH_MAX) return DI_ERANGE;
  int64_t px = 0, st = 0;
  for (int32_t i = 0; i < count; ++i) {
    if (items[i].h < 1 || items[i].w < 1) return DI_EINVAL;
    px += (int64_t)items[i].h * items[i].w;
    if (px > HB_MAX_PX) return DI_ERANGE;
  }
  px = 0;
  for (int32_t i = 0; i < count; ++i) {
    items[i].px_off = px;
    items[i].stats_off = st;
    px += (int64_t)items[i].h * items[i].w;
    st += hb_stats_room(items[i].h, items[i].w);
  }
  *total_px = px;
  *stats_bytes = st;
  return DI_OK;
}

extern "C" int di_head_conv_batch(di_dtype dt, const di_head_conv_args* args, const di_head_item* items,
                                  const di_head_item* items_dev, int32_t count, void* stream) {
  if (!args) return DI_EINVAL;
  int rc = hb_check_items(items, items_dev, count);
  if (rc != DI_OK) return rc;
  unsigned gx = 1, gy = 1;
  di_head_conv_args one = *args;
  for (int32_t i = 0; i < count; ++i) {  // the single call's checks, on every item's own sizes
    one.h = items[i].h;
    one.w = items[i].w;
    rc = hc_check(dt, &one);
    if (rc != DI_OK) return rc;
    const unsigned ix = args->ksize == 1 ? (unsigned)hc_blocks(1, one.h, one.w) : (unsigned)((one.w + HC_TILE - 1) / HC_TILE);
    const unsigned iy = args->ksize == 1 ? 1u : (unsigned)((one.h + HC_TILE - 1) / HC_TILE);
    gx = ix > gx ? ix : gx;
    gy = iy > gy ? iy : gy;
  }
  hc_dispatch<true>(hc_args(args, 0, 0), args->ksize, args->cout, args->dilation, dim3(gx, gy, (unsigned)count),
              (hipStream_t)stream, items_dev);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DI_OK : (int)e;
}
