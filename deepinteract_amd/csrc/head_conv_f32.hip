// Contact-head convolutions in fp32 (di_head_conv_f32): di_head_conv's contract (head_conv.hip) with
// fp32 storage, fp32 weights and v_mfma_f32_16x16x4_f32, for the parity head (LitGINI head_convs="hip_f32"):
//
//   y[co] = bias[co] + sum over (ci, tap) of w[co][ci][tap] * a[ci][pixel + tap offset]
//   a     = in_elu ? ELU(x * in_scale[ci] + in_shift[ci]) : x * in_scale[ci] + in_shift[ci]
//
// a is computed in fp32 (one fmaf, then the ELU) and enters LDS as it is; a tap outside the image
// contributes 0 (the zero padding applies AFTER the transform). The f32-input MFMA is a k-ordered fmaf
// chain with one rounding per term (cdna_hip_programming.md section 3, "FP32-input MFMA"), so nothing
// is rounded but by fp32's own arithmetic, and the bias is added to the finished sum.
//
// ELU: the negative branch is libm's expm1f (about 1 ulp), not hc_elu of the bf16 kernels. hc_elu's
// ~1e-6 relative was chosen against a bf16 rounding of 2^-9 behind it and is four times the fp32
// rounding it would stand beside here, in the one configuration whose reason to exist is the
// reference's numbers; and its price is small in this kernel: an f32 MFMA does 1/16 of the bf16 MFMA's
// work per cycle, so per transformed value the matrix pipe is busy 16 times as long and the ~30 VALU
// operations of expm1f hide behind it (3x3, d = 1: 20 values per thread and chunk against 576 MFMAs).
//
// Shape of the product: as the bf16 kernel, D[co][pixel] = W[co][k] . A[k][pixel] with the weights as the
// MFMA's A operand (row = co = lane & 15) and the pixels as its B operand (col = pixel = lane & 15), but
// one k-step is 4 channels and a lane's operand ONE float: lane l holds W[co][k = l >> 4] and
// A[k = l >> 4][pixel]. So the LDS pixel tile is [channel][pixel], a straight copy of the NCHW planes (no
// transposing fill: consecutive lanes load consecutive pixels of one channel and write consecutive LDS
// words), and a B fragment read is four 16-pixel rows of four consecutive channels. The channel stride
// is the instantiation's largest pixel count rounded up to 16 mod 64 words (a constant: a fragment's
// channel offset is its read's immediate), which puts those four rows on four distinct groups of 16
// banks (64 banks x 4 B). Weights sit in LDS in fragment order, four k-steps to a 16-B vector:
// [tap][cout block][k quad][lane][4], element j of lane (co, g) = channel 16 quad + 4 j + g, so one
// ds_read_b128 feeds four MFMAs.
//
// A block of 4 waves owns 256 output pixels x all Cout channels, as the bf16 kernel (1x1: 256 consecutive
// pixels; 3x3: a 16 x 16 tile with its (16 + 2 d)^2 halo in LDS, nine shifted 1x1 products), so the
// block count, the statistics layout and di_head_conv_stats_bytes are the same. fp32 doubles every LDS
// byte, so the channel chunk is chosen per instantiation (f32_kc): 32 channels for 1x1 with Cout 64
// (34 + 8 KiB), 16 for 1x1 with Cout 128 (its 128 accumulator registers leave room for 16 channels of
// prefetched pixels, not 32) and for 3x3 -- pixels 26 / 37 / 65 KiB at d <= 2 / 4 / 8, weights 36 KiB (Cout 64) or 72 KiB (128) --
// which keeps two blocks per CU exactly where the bf16 kernel has them (1x1; 3x3 with Cout 64, d <= 4).
//
// A thread fixes its pixels' plane offsets once (no division inside the chunk loop). A chunk's pixel
// loads and its first batch of weight loads are issued before the previous chunk's MFMAs and wait in
// registers under them, so the fill between two barriers is the transform, the LDS writes and the
// weights' remaining batches. Plane offsets are 64-bit.
//
// Statistics: as head_conv.hip, of the fp32 values as stored -- a thread's 4 pixels in fp32, then fp64:
// 16 lanes by DPP row exchanges (hc_row_sum, head_batch.h), 4 waves through LDS in wave order, one
// partial per block and channel; no atomics.
//
// di_head_conv_f32_batch runs the same kernel over a packed ragged batch of fp32 images in one launch, as
// di_head_conv_batch does for bf16 (head_conv.hip; the layout and the item table: include/deepinteract_amd.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "common.h"
#include "../../include/deepinteract_amd.h"
#include "head_batch.h"

namespace di {

constexpr int F32_THREADS = 256;
constexpr int F32_TILE = 16;   // 3x3: the output tile is F32_TILE x F32_TILE pixels
constexpr int F32_PIX = 256;   // output pixels per block (both kernel sizes)
constexpr int F32_MAX_CIN = 256;

struct HcArgsF32 {
  const float* x;
  const float* w;
  const float* in_scale;
  const float* in_shift;
  const float* bias;
  float* y;
  double* stats;  // NULL, or the statistics buffer (2 header doubles, then the partials)
  int64_t hw;
  int32_t cin, h, wd, dil, in_elu;
};

// input channels per chunk
constexpr int f32_kc(int ks, int cout) { return ks == 1 && cout == 64 ? 32 : 16; }
// the channel stride of a tile of npx pixels: the least count >= npx that is 16 mod 64
constexpr int f32_stride(int npx) { return (npx + 47) / 64 * 64 + 16; }
// blocks per CU the register budget is set for: the bf16 kernel's (hc_blocks_per_cu)
constexpr int f32_blocks_per_cu(int ks, int cout, int dmax) {
  return ks == 1 || (cout == 64 && dmax <= 4) ? 2 : 1;
}

__device__ __forceinline__ float f32_elu(float z) { return z > 0.f ? z : expm1f(z); }

// an image's own grid from its sizes (1x1: gy = 1): what a single call launches
template <int KS>
__device__ __forceinline__ void f32_item_grid(const HcArgsF32& a, int& gx, int& gy) {
  if constexpr (KS == 3) {
    gx = (a.wd + F32_TILE - 1) / F32_TILE;
    gy = (a.h + F32_TILE - 1) / F32_TILE;
  } else {
    gx = (int)((a.hw + F32_PIX - 1) / F32_PIX);
    gy = 1;
  }
}

// One kernel serves the single call and the batch, as k_head_conv (head_conv.hip, where the form and the
// reason for a template parameter are written out). A single call (TABLE = false, items unused) uses `a`
// as the host filled it, and its launch's grid is the image's own. For a batch, blockIdx.z names the
// item: a.x, a.y, a.stats, a.in_scale and a.in_shift are the packed buffers' bases, which the block
// rebases to its item (fp32: item i of a C-channel buffer at element C * px_off_i), h, wd, hw come from the
// item, the x / y grid is the largest item's, and a block past its own item's tile count leaves at once
// -- as a whole, before any barrier. The statistics then count and number the ITEM's blocks, not the
// launch's.
template <int KS, int COUT, int DMAX, bool TABLE>
__global__ __launch_bounds__(F32_THREADS, f32_blocks_per_cu(KS, COUT, DMAX)) void k_head_conv_f32(
    HcArgsF32 a, const di_head_item* __restrict__ items) {
  if constexpr (TABLE) {
    const int z = blockIdx.z;
    const int64_t px = items[z].px_off;
    a.h = items[z].h;
    a.wd = items[z].w;
    a.hw = (int64_t)a.h * a.wd;
    int gx, gy;
    f32_item_grid<KS>(a, gx, gy);
    if ((int)blockIdx.x >= gx || (int)blockIdx.y >= gy) return;
    a.x += (int64_t)a.cin * px;
    a.y += (int64_t)COUT * px;
    a.stats = a.stats ? reinterpret_cast<double*>(reinterpret_cast<char*>(a.stats) + items[z].stats_off) : nullptr;
    a.in_scale = a.in_scale ? a.in_scale + (int64_t)z * a.cin : nullptr;
    a.in_shift = a.in_shift ? a.in_shift + (int64_t)z * a.cin : nullptr;
  }
  constexpr int TAPS = KS * KS;
  constexpr int NCB = COUT / 16;
  constexpr int KC = f32_kc(KS, COUT);
  constexpr int NKQ = KC / 16;
  constexpr int HALO = F32_TILE + 2 * DMAX;
  constexpr int NPX = KS == 3 ? HALO * HALO : F32_PIX;
  constexpr int STRIDE = f32_stride(NPX);
  constexpr int NJ = (NPX + F32_THREADS - 1) / F32_THREADS;  // pixels of the tile per thread
  constexpr int NW_ELEMS = COUT * KC * TAPS;                 // weight elements of a chunk
  constexpr int WB = KS == 3 ? 9 : 8;                        // weight loads in flight per thread
  // a tap's weights in LDS, 4 floats more than their COUT x KC: consecutive elements of the module's
  // tensor are the 9 taps of one (co, ci), and the skew spreads their writes over 9 groups of banks
  constexpr int WTAP = COUT * KC + 4;
  // channels of a chunk whose pixel loads are issued a chunk ahead: all, but half of them where two
  // blocks share a CU's registers and a thread has 3 pixels (3x3, Cout 64, d 3 .. 4: all 16 spill)
  constexpr int PRE = f32_blocks_per_cu(KS, COUT, DMAX) == 2 && NJ == 3 ? KC / 2 : KC;
  static_assert(NW_ELEMS % (F32_THREADS * WB) == 0, "whole weight batches");
  static_assert(KC % 16 == 0, "whole k quads");
  static_assert(KC * STRIDE * 4 >= 4 * COUT * 2 * 8, "the statistics' wave partials reuse the pixel tile");
  static_assert((TAPS * WTAP + KC * STRIDE + 2 * F32_MAX_CIN + COUT) * 4 * f32_blocks_per_cu(KS, COUT, DMAX) <=
                    160 * 1024, "the blocks of a CU fit its LDS");
  __shared__ __attribute__((aligned(16))) float wl[TAPS * WTAP];  // [tap][cout block][k quad][lane][4]
  __shared__ __attribute__((aligned(16))) float xl[KC * STRIDE];       // [channel][pixel]
  __shared__ float tr[2][F32_MAX_CIN];                                  // in_scale, in_shift
  __shared__ float bl[COUT];                                            // bias

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p = lane & 15, g = lane >> 4;
  const int d = KS == 3 ? a.dil : 0;
  const int halo = F32_TILE + 2 * d;  // <= HALO: the host picks DMAX >= d
  const int npx = KS == 3 ? halo * halo : F32_PIX;
  const int bx = blockIdx.x, by = blockIdx.y;
  const int y0 = by * F32_TILE, x0 = bx * F32_TILE;  // 3x3
  const int64_t base = (int64_t)bx * F32_PIX;        // 1x1
  const int64_t hw = a.hw;

  for (int c = tid; c < a.cin; c += F32_THREADS) {
    tr[0][c] = a.in_scale ? a.in_scale[c] : 1.f;
    tr[1][c] = a.in_shift ? a.in_shift[c] : 0.f;
  }
  if (tid < COUT) bl[tid] = a.bias ? a.bias[tid] : 0.f;

  // this thread's pixels of the tile: slot j is tile pixel tid + 256 j; its plane offset, or -1 outside
  // the image (loaded from offset 0 and zeroed after the transform, so no load sits behind a branch)
  int64_t goff[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int px = tid + j * F32_THREADS;
    int64_t gp;
    bool valid;
    if constexpr (KS == 3) {
      const int hy = px / halo, hx = px - hy * halo;
      const int gy = y0 - d + hy, gx = x0 - d + hx;
      valid = px < npx && gy >= 0 && gy < a.h && gx >= 0 && gx < a.wd;
      gp = (int64_t)gy * a.wd + gx;
    } else {
      gp = base + px;
      valid = gp < hw;
    }
    goff[j] = valid ? gp : -1;
  }

  floatx4 acc[4][NCB];
#pragma unroll
  for (int pb = 0; pb < 4; ++pb)
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) acc[pb][cb] = (floatx4){0.f, 0.f, 0.f, 0.f};

  // A chunk's global loads are issued one chunk ahead, before the previous chunk's MFMAs, and held in
  // registers under them: its pixels (PRE x NJ values) and the first batch of its weights.
  float raw[PRE][NJ];
  float wv[WB];
  auto prefetch = [&](const int c0) {
#pragma unroll
    for (int u = 0; u < WB; ++u) {
      const int e = tid + u * F32_THREADS;
      const int co = e / (KC * TAPS), r = e % (KC * TAPS);
      wv[u] = a.w[((int64_t)co * a.cin + c0) * TAPS + r];
    }
#pragma unroll
    for (int u = 0; u < PRE; ++u)
#pragma unroll
      for (int j = 0; j < NJ; ++j) raw[u][j] = a.x[(int64_t)(c0 + u) * hw + (goff[j] < 0 ? 0 : goff[j])];
  };
  // channel u of the chunk at c0: transformed as it enters LDS
  auto put_x = [&](const int c0, const int u, const float (&v)[NJ]) {
    const float sc = tr[0][c0 + u], sh = tr[1][c0 + u];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int px = tid + j * F32_THREADS;
      const float z = fmaf(v[j], sc, sh);
      const float f = a.in_elu ? f32_elu(z) : z;
      if (px < npx) xl[u * STRIDE + px] = goff[j] < 0 ? 0.f : f;  // zero AFTER the transform
    }
  };
  // element e of a chunk's weights (for one co the chunk's KC x TAPS elements are contiguous) to its
  // place in fragment order
  auto put_w = [&](const int e, const float v) {
    const int co = e / (KC * TAPS), r = e % (KC * TAPS), ci = r / TAPS, t = r % TAPS;
    wl[t * WTAP + ((((co >> 4) * NKQ + (ci >> 4)) * 64) + (co & 15) + 16 * (ci & 3)) * 4 + ((ci >> 2) & 3)] = v;
  };
  prefetch(0);

  for (int c0 = 0; c0 < a.cin; c0 += KC) {
    __syncthreads();  // the previous chunk's fragments are read (first pass: tr is written)
#pragma unroll
    for (int u = 0; u < WB; ++u) put_w(tid + u * F32_THREADS, wv[u]);
#pragma unroll
    for (int u = 0; u < PRE; ++u) put_x(c0, u, raw[u]);
    if constexpr (PRE < KC) {  // the channels that were not prefetched, in one batch
      float rest[KC - PRE][NJ];
#pragma unroll
      for (int u = 0; u < KC - PRE; ++u)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          rest[u][j] = a.x[(int64_t)(c0 + PRE + u) * hw + (goff[j] < 0 ? 0 : goff[j])];
#pragma unroll
      for (int u = 0; u < KC - PRE; ++u) put_x(c0, PRE + u, rest[u]);
    }
    // the weights' other batches
    for (int e0 = tid + F32_THREADS * WB; e0 < NW_ELEMS; e0 += F32_THREADS * WB) {
      float v[WB];
#pragma unroll
      for (int u = 0; u < WB; ++u) {
        const int e = e0 + u * F32_THREADS;
        const int co = e / (KC * TAPS), r = e % (KC * TAPS);
        v[u] = a.w[((int64_t)co * a.cin + c0) * TAPS + r];
      }
#pragma unroll
      for (int u = 0; u < WB; ++u) put_w(e0 + u * F32_THREADS, v[u]);
    }
    __syncthreads();
    // the next chunk's loads (the last chunk loads itself again: no branch around the loads), pinned
    // in front of the MFMAs
    prefetch(c0 + KC < a.cin ? c0 + KC : c0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < TAPS; ++t) {
      int pxo[4];
#pragma unroll
      for (int pb = 0; pb < 4; ++pb) {
        const int rb = wave * 4 + pb;
        pxo[pb] = g * STRIDE + (KS == 3 ? (rb + (t / 3) * d) * halo + (t % 3) * d + p : rb * 16 + p);
      }
#pragma unroll
      for (int kq = 0; kq < NKQ; ++kq) {
        floatx4 af[NCB];
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
          af[cb] = *reinterpret_cast<const floatx4*>(wl + t * WTAP + ((cb * NKQ + kq) * 64 + lane) * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float bf[4];
#pragma unroll
          for (int pb = 0; pb < 4; ++pb) bf[pb] = xl[(16 * kq + 4 * j) * STRIDE + pxo[pb]];
#pragma unroll
          for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int pb = 0; pb < 4; ++pb)
              acc[pb][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[cb][j], bf[pb], acc[pb][cb], 0, 0, 0);
        }
        // one (tap, k quad) group -- NCB + 16 LDS reads, 16 NCB MFMAs -- at a time: without the fence
        // the compiler hoists every tap's fragment reads and the Cout = 64 3x3 kernels spill at their
        // 256 registers; the reads' latency at a group's head is the other wave's MFMA time
        __builtin_amdgcn_sched_barrier(0);
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
        const float v = acc[pb][cb][r] + bc;
        if (valid[pb]) {
          a.y[(int64_t)co * hw + gp[pb]] = v;
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
    int gx = gridDim.x, gy = gridDim.y;  // a single call's grid is the image's
    if constexpr (TABLE) f32_item_grid<KS>(a, gx, gy);
    const int64_t nblk = (int64_t)gx * gy;
    const int64_t blk = (int64_t)by * gx + bx;
    double* part = a.stats + 2;
    if (tid < COUT) {
      double s = 0.0, ss = 0.0;
      for (int w = 0; w < F32_THREADS / 64; ++w) {
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

// blocks of a launch = partials per channel: the bf16 kernel's counts, which di_head_conv_stats_bytes sizes
static int64_t f32_blocks(int ksize, int64_t h, int64_t w) {
  if (ksize == 3) return ((h + F32_TILE - 1) / F32_TILE) * ((w + F32_TILE - 1) / F32_TILE);
  return (h * w + F32_PIX - 1) / F32_PIX;
}

// hc_check's refusals (head_conv.hip) with fp32's alignment
static int f32_check(const di_head_conv_args* a) {
  if (!a) return DI_EINVAL;
  if (!a->x || !a->weight || !a->y || a->y == a->x) return DI_EINVAL;
  if (a->cin != 64 && a->cin != 128 && a->cin != 256) return DI_EINVAL;
  if (a->cout != 64 && a->cout != 128) return DI_EINVAL;
  if (a->ksize != 1 && a->ksize != 3) return DI_EINVAL;
  if (a->dilation < 1 || a->dilation > 8) return DI_EINVAL;
  if (a->h < 1 || a->w < 1) return DI_EINVAL;
  if ((((uintptr_t)a->x | (uintptr_t)a->weight | (uintptr_t)a->y) & 3) != 0) return DI_EINVAL;
  if (((uintptr_t)a->stats & 7) != 0) return DI_EINVAL;
  if (a->ksize == 3 && ((a->h + F32_TILE - 1) / F32_TILE) > 65535) return DI_ERANGE;  // grid.y
  if (a->ksize == 1 && f32_blocks(1, a->h, a->w) > INT32_MAX) return DI_ERANGE;       // grid.x
  return DI_OK;
}

template <int KS, int COUT, int DMAX, bool TABLE>
static void f32_launch(const HcArgsF32& k, dim3 grid, hipStream_t s, const di_head_item* items) {
  hipLaunchKernelGGL((k_head_conv_f32<KS, COUT, DMAX, TABLE>), grid, dim3(F32_THREADS), 0, s, k, items);
}

// the kernel's arguments from the call's, for an image of h x w pixels (a batch: 0 x 0, every block
// takes its item's)
static HcArgsF32 f32_args(const di_head_conv_args* args, int32_t h, int32_t w) {
  HcArgsF32 k;
  k.x = (const float*)args->x;
  k.w = (const float*)args->weight;
  k.in_scale = args->in_scale;
  k.in_shift = args->in_shift;
  k.bias = args->bias;
  k.y = (float*)args->y;
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
static void f32_dispatch(const HcArgsF32& k, int ksize, int cout, int d, dim3 grid, hipStream_t s,
                         const di_head_item* items) {
  const bool wide = cout == 128;
  if (ksize == 1) {
    if (wide) f32_launch<1, 128, 0, TABLE>(k, grid, s, items);
    else f32_launch<1, 64, 0, TABLE>(k, grid, s, items);
  } else if (d <= 2) {
    if (wide) f32_launch<3, 128, 2, TABLE>(k, grid, s, items);
    else f32_launch<3, 64, 2, TABLE>(k, grid, s, items);
  } else if (d <= 4) {
    if (wide) f32_launch<3, 128, 4, TABLE>(k, grid, s, items);
    else f32_launch<3, 64, 4, TABLE>(k, grid, s, items);
  } else {
    if (wide) f32_launch<3, 128, 8, TABLE>(k, grid, s, items);
    else f32_launch<3, 64, 8, TABLE>(k, grid, s, items);
  }
}

// The batch's validation: the table, then the single call's checks on every item's own sizes. On DI_OK
// *grid is the launch's: (the largest item's gx, the largest item's gy, count).
static int f32_batch_check(const di_head_conv_args* args, const di_head_item* items, const di_head_item* items_dev,
                           int32_t count, dim3* grid) {
  if (!args) return DI_EINVAL;
  int rc = hb_check_items(items, items_dev, count);
  if (rc != DI_OK) return rc;
  unsigned gx = 1, gy = 1;
  di_head_conv_args one = *args;
  for (int32_t i = 0; i < count; ++i) {
    one.h = items[i].h;
    one.w = items[i].w;
    rc = f32_check(&one);
    if (rc != DI_OK) return rc;
    const unsigned ix = args->ksize == 1 ? (unsigned)f32_blocks(1, one.h, one.w) : (unsigned)((one.w + F32_TILE - 1) / F32_TILE);
    const unsigned iy = args->ksize == 1 ? 1u : (unsigned)((one.h + F32_TILE - 1) / F32_TILE);
    gx = ix > gx ? ix : gx;
    gy = iy > gy ? iy : gy;
  }
  *grid = dim3(gx, gy, (unsigned)count);
  return DI_OK;
}

}  // namespace di

using namespace di;

extern "C" int di_head_conv_f32_check(const di_head_conv_args* args) { return f32_check(args); }

extern "C" int di_head_conv_f32(const di_head_conv_args* args, void* stream) {
  const int rc = f32_check(args);
  if (rc != DI_OK) return rc;
  const dim3 grid = args->ksize == 1 ? dim3((unsigned)f32_blocks(1, args->h, args->w))
                                     : dim3((args->w + F32_TILE - 1) / F32_TILE, (args->h + F32_TILE - 1) / F32_TILE);
  f32_dispatch<false>(f32_args(args, args->h, args->w), args->ksize, args->cout, args->dilation, grid,
                      (hipStream_t)stream, nullptr);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DI_OK : (int)e;
}

extern "C" int di_head_conv_f32_batch_check(const di_head_conv_args* args, const di_head_item* items,
                                            const di_head_item* items_dev, int32_t count) {
  dim3 grid;
  return f32_batch_check(args, items, items_dev, count, &grid);
}

extern "C" int di_head_conv_f32_batch(const di_head_conv_args* args, const di_head_item* items,
                                      const di_head_item* items_dev, int32_t count, void* stream) {
  dim3 grid;
  const int rc = f32_batch_check(args, items, items_dev, count, &grid);
  if (rc != DI_OK) return rc;
  f32_dispatch<true>(f32_args(args, 0, 0), args->ksize, args->cout, args->dilation, grid, (hipStream_t)stream,
                     items_dev);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DI_OK : (int)e;
}
