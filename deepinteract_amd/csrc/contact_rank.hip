// Contact ranking (di_contact_rank): what a user does with the head's logits of one complex --
// the contact-probability map, its K best contacts in a fixed order, and, given labels, the
// counters LitGINI.test_step's metrics are made of (deepinteract_modules.py:2018-2101, top-k
// precision / recall deepinteract_utils.py:977-995) -- without sorting the n = L1 * L2 map.
//
//   p = softmax(logits)[1] = 1 / (1 + exp(l0 - l1))            (contact_prob: the only producer of p)
//   order: p descending, equal p by ascending flat index i * L2 + j, NaN above every number
//          (torch.sort(descending=True, stable=True) of the stored map)
//   key(p) = the bits of p (monotone: p >= 0), NaN -> all ones; the K-th largest key T is found by a
//   radix select over 11 / 11 / 10 key bits, so exactly K elements have key > T or are among the
//   lowest-index elements with key == T.
//
// Launch sequence on the caller's stream (no block waits for another; every stage is a kernel):
//   memset           the header (histograms, label counters)
//   k_rank_probs     logits -> probs (fp32), histogram of key bits 31..21 (LDS-private, one flush
//                    per block); with labels: tp / fp / fn / tn counters (integer atomics) and one
//                    fp64 cross-entropy partial per block
//   k_rank_hist<1>   select (every block, from the finished histogram: the bin holding rank K ->
//                    prefix, ranks still to take inside it), then probs -> histogram of bits 20..10
//                    under the prefix
//   k_rank_hist<2>   select, then probs -> histogram of bits 9..0 under the prefix
//   k_rank_count     select -> T and how many elements equal to T to take; probs -> per WAVE (a
//                    contiguous slice each) the elements > T and == T
//   k_rank_compact   blocks holding a candidate sum the counts of the waves before them, re-read
//                    their slices and write (key, index) at its position (wave-ballot ranks: index
//                    order, no atomics); the others return
//   k_rank_finish    one block: bitonic sort of the K candidates by (key desc, index asc) in LDS,
//                    top_ids / top_scores, prefix sums of labels[top_ids], the loss partials folded
//                    in a fixed order, the metrics record
// Algorithmic bytes per element (fp32 / bf16 logits): 8 / 4 read + 4 written by k_rank_probs (+ 1
// with labels), then 3 x 4 read of the map (two histograms, the count): 24 / 20 B; the compaction
// re-reads only slices that hold a candidate.
// di_contact_rank_batch runs the same sequence once for many complexes (grid y = complex; "the batch"
// below): the same kernel bodies on the same per-complex geometry, so the same bits per complex.
// Elements are handled as 4-element vectors of the (16-B aligned) map; the class planes of the
// logits start at any element alignment (n odd), so they are read with unaligned 16-B / 8-B loads.
#include <float.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "common.h"
#include "../../include/deepinteract_amd.h"

namespace di {

constexpr int RK_THREADS = 256;
constexpr int RK_WAVES = RK_THREADS / 64;
constexpr int RK_MAX_BLOCKS = 1024;
constexpr int RK_MAX_WAVES = RK_MAX_BLOCKS * RK_WAVES;
constexpr int RK_ONE_THREADS = 1024;  // the single-block stage (finish)
constexpr int64_t RK_MAX_N = (int64_t)1 << 29;  // the fp32 map stays under 2^31 bytes

// cleared by the launch sequence before every run
struct RankHdr {
  uint32_t hist[3][2048];     // pass 2 uses 1024 bins
  unsigned long long cnt[5];  // num_pos, tp, fp, fn, tn
  uint32_t sel[3][2];         // after select step i: {key bits fixed so far, ranks to take under them};
                              // sel[2]: {the threshold key T, elements equal to T to take}
};
static_assert(sizeof(RankHdr) % 16 == 0, "the arrays behind the header stay 16-B aligned");

// workspace behind the header
struct RankWork {
  RankHdr* hdr;
  uint32_t *wave_eq, *wave_gt;  // [RK_MAX_WAVES] each
  double* ce_part;              // [RK_MAX_BLOCKS]
  unsigned long long* cand;     // [k]: (~key << 32) | index
};
constexpr int64_t RK_FIXED_BYTES =
    (int64_t)sizeof(RankHdr) + 2 * RK_MAX_WAVES * (int64_t)sizeof(uint32_t) + RK_MAX_BLOCKS * (int64_t)sizeof(double);

// hdr: the cleared header; rest: everything else (directly behind the header in a single call's
// workspace; in a batch the headers of all complexes are contiguous, so that one memset clears them)
__host__ __device__ static inline RankWork rank_work(void* hdr, void* rest) {
  RankWork w;
  w.hdr = reinterpret_cast<RankHdr*>(hdr);
  w.wave_eq = reinterpret_cast<uint32_t*>(rest);
  w.wave_gt = w.wave_eq + RK_MAX_WAVES;
  w.ce_part = reinterpret_cast<double*>(w.wave_gt + RK_MAX_WAVES);
  w.cand = reinterpret_cast<unsigned long long*>(w.ce_part + RK_MAX_BLOCKS);
  return w;
}

// nv 4-element vectors over nb blocks of RK_WAVES waves; wave w owns vectors [w * per, (w + 1) * per)
// (per a multiple of 64). A function of n alone: the loss partials fold the same way on every run.
struct RankGeo {
  int nv, nb, nw, per;
};
__host__ __device__ static inline RankGeo rank_geo(int64_t n) {
  RankGeo g;
  g.nv = (int)((n + 3) / 4);
  const int64_t want = (g.nv + RK_THREADS * 4 - 1) / (RK_THREADS * 4);  // >= 4 vectors per lane
  g.nb = (int)(want < 1 ? 1 : (want > RK_MAX_BLOCKS ? RK_MAX_BLOCKS : want));
  g.nw = g.nb * RK_WAVES;
  g.per = ((g.nv + g.nw - 1) / g.nw + 63) / 64 * 64;
  return g;
}

// ---------------------------------------------------------------- the value and its key
// A NaN is stored as the one positive quiet NaN, whatever sign and payload the logits' NaN carried:
// sorts that order floats by their bits then rank it above every number too.
__device__ __forceinline__ float contact_prob(float l0, float l1) {
  const float p = 1.0f / (1.0f + expf(l0 - l1));
  return p != p ? __uint_as_float(0x7fc00000u) : p;
}

__device__ __forceinline__ uint32_t rank_key(float p) { return p != p ? 0xffffffffu : __float_as_uint(p); }

// -log softmax(l0, l1)[label] = softplus(+-(l0 - l1)), in fp64 (the difference of two fp32 is exact there)
__device__ __forceinline__ double ce_term(float l0, float l1, bool pos) {
  const double x = pos ? (double)l0 - (double)l1 : (double)l1 - (double)l0;
  return fmax(x, 0.0) + log1p(exp(-fabs(x)));
}

template <typename T>
struct Logit;
template <>
struct Logit<float> {
  __device__ static void ld4(const float* p, float* v) {
    floatx4 a;
    __builtin_memcpy(&a, p, 16);  // element-aligned only
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = a[q];
  }
  __device__ static float ld1(const float* p) { return *p; }
};
template <>
struct Logit<u16> {
  __device__ static void ld4(const u16* p, float* v) {
    uint2 u;
    __builtin_memcpy(&u, p, 8);
    v[0] = __builtin_bit_cast(float, u.x << 16);
    v[1] = __builtin_bit_cast(float, u.x & 0xffff0000u);
    v[2] = __builtin_bit_cast(float, u.y << 16);
    v[3] = __builtin_bit_cast(float, u.y & 0xffff0000u);
  }
  __device__ static float ld1(const u16* p) { return __builtin_bit_cast(float, (uint32_t)*p << 16); }
};

// the stored probabilities of vector v; returns how many of its 4 elements lie inside the map
__device__ __forceinline__ int load_probs4(const float* __restrict__ probs, int v, int n, float* p) {
  const int e = 4 * v;
  if (e + 4 <= n) {
    const floatx4 a = *reinterpret_cast<const floatx4*>(probs + e);
#pragma unroll
    for (int q = 0; q < 4; ++q) p[q] = a[q];
    return 4;
  }
  const int m = n - e;
#pragma unroll
  for (int q = 0; q < 4; ++q) p[q] = q < m ? probs[e + q] : 0.f;
  return m;
}

__device__ __forceinline__ void lds_hist_clear(uint32_t* h, int bins) {
  for (int i = threadIdx.x; i < bins; i += RK_THREADS) h[i] = 0;
  __syncthreads();
}
__device__ __forceinline__ void lds_hist_flush(const uint32_t* h, int bins, uint32_t* g) {
  __syncthreads();
  for (int i = threadIdx.x; i < bins; i += RK_THREADS)
    if (h[i]) atomicAdd(&g[i], h[i]);
}

// ---------------------------------------------------------------- pass 1
// Every stage is a __device__ body behind two thin entry points: k_x for one complex and k_x_b for a
// batch, where the grid's y index names the complex (see "the batch" below). bx is the block's index
// inside its complex.
template <typename T, bool LAB>
__device__ __forceinline__ void rank_probs_body(const int bx, const T* __restrict__ logits, int n, int nv, int per,
                                                const uint8_t* __restrict__ labels, float threshold,
                                                float* __restrict__ probs, RankHdr* __restrict__ hdr,
                                                double* __restrict__ ce_part) {
  __shared__ uint32_t h[2048];
  lds_hist_clear(h, 2048);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lo = (bx * RK_WAVES + wave) * per;
  const int hi = lo + per < nv ? lo + per : nv;
  const T* __restrict__ l0 = logits;
  const T* __restrict__ l1 = logits + n;
  double ce = 0.0;
  uint32_t c_tp = 0, c_fp = 0, c_fn = 0, c_tn = 0;
  for (int v = lo + lane; v < hi; v += 64) {
    const int e = 4 * v;
    const int m = n - e < 4 ? n - e : 4;
    float a[4], b[4], p[4];
    uint32_t lab4 = 0;
    if (m == 4) {
      Logit<T>::ld4(l0 + e, a);
      Logit<T>::ld4(l1 + e, b);
      if constexpr (LAB) __builtin_memcpy(&lab4, labels + e, 4);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        a[q] = q < m ? Logit<T>::ld1(l0 + e + q) : 0.f;
        b[q] = q < m ? Logit<T>::ld1(l1 + e + q) : 0.f;
        if constexpr (LAB) lab4 |= q < m ? (uint32_t)labels[e + q] << (8 * q) : 0u;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) p[q] = contact_prob(a[q], b[q]);
    if (m == 4) {
      *reinterpret_cast<floatx4*>(probs + e) = (floatx4){p[0], p[1], p[2], p[3]};
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q < m) probs[e + q] = p[q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q < m) {
        atomicAdd(&h[rank_key(p[q]) >> 21], 1u);
        if constexpr (LAB) {
          const bool pos = ((lab4 >> (8 * q)) & 0xffu) != 0, pred = p[q] >= threshold;
          c_tp += pred && pos;
          c_fp += pred && !pos;
          c_fn += !pred && pos;
          c_tn += !pred && !pos;
          ce += ce_term(a[q], b[q], pos);
        }
      }
    }
  }
  lds_hist_flush(h, 2048, hdr->hist[0]);
  if constexpr (LAB) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      ce += __shfl_xor(ce, off);
      c_tp += __shfl_xor(c_tp, off);
      c_fp += __shfl_xor(c_fp, off);
      c_fn += __shfl_xor(c_fn, off);
      c_tn += __shfl_xor(c_tn, off);
    }
    __shared__ double red_ce[RK_WAVES];
    __shared__ uint32_t red_c[4][RK_WAVES];
    if (lane == 0) {
      red_ce[wave] = ce;
      red_c[0][wave] = c_tp, red_c[1][wave] = c_fp, red_c[2][wave] = c_fn, red_c[3][wave] = c_tn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double s = 0.0;
      unsigned long long c[4] = {0, 0, 0, 0};
      for (int w = 0; w < RK_WAVES; ++w) {
        s += red_ce[w];
        for (int j = 0; j < 4; ++j) c[j] += red_c[j][w];
      }
      ce_part[bx] = s;  // folded in block order by k_rank_finish
      if (c[0] + c[2]) atomicAdd(&hdr->cnt[0], c[0] + c[2]);
      for (int j = 0; j < 4; ++j)
        if (c[j]) atomicAdd(&hdr->cnt[1 + j], c[j]);
    }
  }
}

// ---------------------------------------------------------------- radix select
// exclusive prefix sum of v over the block's threads (whole waves, at most 16); s: 16 words of LDS
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* s) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(inc, off);
    if (lane >= off) inc += t;
  }
  __syncthreads();  // s is free of an earlier scan's readers
  if (lane == 63) s[wave] = inc;
  __syncthreads();
  uint32_t base = 0;
  for (int i = 0; i < wave; ++i) base += s[i];
  return base + inc - v;
}

// Select step STEP, by every block of the kernel that needs its result (a launch less than a
// one-block kernel, and the histogram is complete: the previous kernel filled it): the bin, from the
// top, that holds rank krem of histogram STEP extends the prefix; the elements above it come off
// krem. Requires krem <= the histogram's total. Block 0 records the result as hdr->sel[STEP] for the
// kernels after this one (nothing in this kernel reads that slot).
struct RankSel {
  uint32_t prefix, krem;
};
template <int STEP>
__device__ __forceinline__ RankSel rank_select(const int bx, RankHdr* __restrict__ hdr, uint32_t k) {
  constexpr int BINS = STEP == 2 ? 1024 : 2048;
  constexpr int BITS = STEP == 2 ? 10 : 11;
  constexpr int PER = BINS / RK_THREADS;
  __shared__ uint32_t s[16], res[2];
  const uint32_t prefix = STEP == 0 ? 0u : hdr->sel[STEP - 1][0];
  const uint32_t krem = STEP == 0 ? k : hdr->sel[STEP - 1][1];
  const uint32_t* __restrict__ h = hdr->hist[STEP];
  const int t = threadIdx.x;
  uint32_t c[PER], sum = 0;  // thread t: bins BINS-1 - PER t downwards
#pragma unroll
  for (int j = 0; j < PER; ++j) sum += c[j] = h[BINS - 1 - (PER * t + j)];
  uint32_t above = block_excl_scan(sum, s);
  if (t == 0) res[0] = prefix << BITS, res[1] = 1u;  // kept only if krem exceeds the total (never)
  __syncthreads();
  if (above < krem && krem <= above + sum) {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      if (krem <= above + c[j]) {
        res[0] = (prefix << BITS) | (uint32_t)(BINS - 1 - (PER * t + j));
        res[1] = krem - above;
        break;
      }
      above += c[j];
    }
  }
  __syncthreads();
  const RankSel r = {res[0], res[1]};
  if (bx == 0 && t == 0) hdr->sel[STEP][0] = r.prefix, hdr->sel[STEP][1] = r.krem;
  return r;
}

// PASS 1: bits 20..10 of the keys whose bits 31..21 equal the prefix; PASS 2: bits 9..0 of those whose
// bits 31..10 do
template <int PASS>
__device__ __forceinline__ void rank_hist_body(const int bx, const float* __restrict__ probs, int n, int nv, int per,
                                               uint32_t k, RankHdr* __restrict__ hdr) {
  constexpr int BINS = PASS == 1 ? 2048 : 1024;
  constexpr int SHIFT = PASS == 1 ? 21 : 10;
  __shared__ uint32_t h[BINS];
  lds_hist_clear(h, BINS);
  const uint32_t prefix = rank_select<PASS - 1>(bx, hdr, k).prefix;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lo = (bx * RK_WAVES + wave) * per;
  const int hi = lo + per < nv ? lo + per : nv;
#pragma unroll 2
  for (int v = lo + lane; v < hi; v += 64) {
    float p[4];
    const int m = load_probs4(probs, v, n, p);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t key = rank_key(p[q]);
      if (q < m && (key >> SHIFT) == prefix) atomicAdd(&h[PASS == 1 ? (key >> 10) & 0x7ffu : key & 0x3ffu], 1u);
    }
  }
  lds_hist_flush(h, BINS, hdr->hist[PASS]);
}

// ---------------------------------------------------------------- ordered compaction
// the last select fixes the threshold key T (hdr->sel[2]: T, and how many elements equal to T to take)
__device__ __forceinline__ void rank_count_body(const int bx, const float* __restrict__ probs, int n, int nv, int per,
                                                uint32_t k, RankHdr* __restrict__ hdr,
                                                uint32_t* __restrict__ wave_eq, uint32_t* __restrict__ wave_gt) {
  const uint32_t T = rank_select<2>(bx, hdr, k).prefix;
  const int lane = threadIdx.x & 63, w = bx * RK_WAVES + (threadIdx.x >> 6);
  const int lo = w * per;
  const int hi = lo + per < nv ? lo + per : nv;
  uint32_t eq = 0, gt = 0;
#pragma unroll 2
  for (int v = lo + lane; v < hi; v += 64) {
    float p[4];
    const int m = load_probs4(probs, v, n, p);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t key = rank_key(p[q]);
      eq += q < m && key == T;
      gt += q < m && key > T;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    eq += __shfl_xor(eq, off);
    gt += __shfl_xor(gt, off);
  }
  if (lane == 0) {
    wave_eq[w] = eq;
    wave_gt[w] = gt;
  }
}

// Candidates in index order: the elements above T at cand[0 .. k - need), the first `need` elements
// equal to T behind them. A block without a candidate returns at once; the others sum the counts of
// the waves before them (the scan across blocks, without a launch of its own). A wave's rank inside
// its 64-vector tile comes from ballots: lanes below it, then its own earlier elements.
__device__ __forceinline__ void rank_compact_body(const int bx, const float* __restrict__ probs, int n, int nv,
                                                  int per, int k, const RankHdr* __restrict__ hdr,
                                                  const uint32_t* __restrict__ wave_eq,
                                                  const uint32_t* __restrict__ wave_gt,
                                                  unsigned long long* __restrict__ cand) {
  const uint32_t T = hdr->sel[2][0];
  const uint32_t need = hdr->sel[2][1] < (uint32_t)k ? hdr->sel[2][1] : (uint32_t)k;  // 1 .. k: slots stay below k
  const uint32_t ngt = (uint32_t)k - need;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int w0 = bx * RK_WAVES, w = w0 + wave;
  uint32_t ceq[RK_WAVES], cgt[RK_WAVES], any = 0;
#pragma unroll
  for (int i = 0; i < RK_WAVES; ++i) any |= (ceq[i] = wave_eq[w0 + i]) | (cgt[i] = wave_gt[w0 + i]);
  if (any == 0) return;  // block-uniform
  uint32_t oe = 0, og = 0;
  for (int i = threadIdx.x; i < w0; i += RK_THREADS) oe += wave_eq[i], og += wave_gt[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) oe += __shfl_xor(oe, off), og += __shfl_xor(og, off);
  __shared__ uint32_t red[2][RK_WAVES];
  if (lane == 0) red[0][wave] = oe, red[1][wave] = og;
  __syncthreads();
  oe = og = 0;
#pragma unroll
  for (int i = 0; i < RK_WAVES; ++i) {
    oe += red[0][i] + (i < wave ? ceq[i] : 0u);
    og += red[1][i] + (i < wave ? cgt[i] : 0u);
  }
  if (cgt[wave] == 0 && (ceq[wave] == 0 || oe >= need)) return;  // wave-uniform, after the block's barrier
  const int lo = w * per;
  const int hi = lo + per < nv ? lo + per : nv;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int v0 = lo; v0 < hi; v0 += 64) {
    const int v = v0 + lane;
    float p[4] = {0.f, 0.f, 0.f, 0.f};
    const int m = v < hi ? load_probs4(probs, v, n, p) : 0;
    uint32_t key[4], fe = 0, fg = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      key[q] = rank_key(p[q]);
      fe |= (uint32_t)(q < m && key[q] == T) << q;
      fg |= (uint32_t)(q < m && key[q] > T) << q;
    }
    if (__ballot((fe | fg) != 0) == 0ull) continue;
    uint32_t pe = 0, pg = 0, te = 0, tg = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned long long be = __ballot((fe >> q) & 1u), bg = __ballot((fg >> q) & 1u);
      pe += __popcll(be & below), te += __popcll(be);
      pg += __popcll(bg & below), tg += __popcll(bg);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t idx = (uint32_t)(4 * v + q);
      if ((fe >> q) & 1u) {
        const uint32_t r = oe + pe + __popc(fe & ((1u << q) - 1u));
        if (r < need) cand[ngt + r] = ((unsigned long long)(~T) << 32) | idx;
      }
      if ((fg >> q) & 1u) {
        const uint32_t r = og + pg + __popc(fg & ((1u << q) - 1u));
        if (r < ngt) cand[r] = ((unsigned long long)(~key[q]) << 32) | idx;
      }
    }
    oe += te;
    og += tg;
  }
}

// ---------------------------------------------------------------- sort and outputs
// One block per complex. kp: k rounded up to a power of two (<= DI_RANK_MAX_K).
__device__ __forceinline__ void rank_finish_body(
    const float* __restrict__ probs, const uint8_t* __restrict__ labels, int n, int k, int kp,
    const unsigned long long* __restrict__ cand, const RankHdr* __restrict__ hdr, const double* __restrict__ ce_part,
    int nb, int32_t* __restrict__ top_ids, float* __restrict__ top_scores, int32_t* __restrict__ top_hits,
    di_rank_metrics* __restrict__ metrics) {
  static_assert(DI_RANK_MAX_K <= 4 * RK_ONE_THREADS, "4 ranks per thread");
  __shared__ unsigned long long s[DI_RANK_MAX_K];
  __shared__ double sd[RK_ONE_THREADS];
  __shared__ uint32_t sc[16];
  const int t = threadIdx.x;
  for (int i = t; i < kp; i += RK_ONE_THREADS) s[i] = i < k ? cand[i] : ~0ull;
  __syncthreads();
  // ascending (~key, index) = key descending, index ascending; the all-ones padding stays behind
  for (int size = 2; size <= kp; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = t; i < (kp >> 1); i += RK_ONE_THREADS) {
        const int a = 2 * i - (i & (stride - 1)), b = a + stride;
        const unsigned long long x = s[a], y = s[b];
        if ((x > y) == ((a & size) == 0)) s[a] = y, s[b] = x;
      }
      __syncthreads();
    }
  }
  uint32_t id[4], lab[4] = {0, 0, 0, 0}, mine = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = 4 * t + j;
    if (r < k) {
      id[j] = (uint32_t)s[r];
      if (id[j] >= (uint32_t)n) id[j] = (uint32_t)n - 1;  // never taken: keeps every gather inside the map
      top_ids[r] = (int32_t)id[j];
      top_scores[r] = probs[id[j]];
      if (labels) mine += lab[j] = labels[id[j]] != 0;
    }
  }
  if (labels) {  // kernel argument: uniform
    uint32_t run = block_excl_scan(mine, sc);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = 4 * t + j;
      run += lab[j];
      if (r < k) top_hits[r] = (int32_t)run;
    }
    // the blocks' loss partials, always folded in this order
    double acc = 0.0;
    for (int i = t; i < nb; i += RK_ONE_THREADS) acc += ce_part[i];
    sd[t] = acc;
    __syncthreads();
    for (int off = RK_ONE_THREADS / 2; off > 0; off >>= 1) {
      if (t < off) sd[t] += sd[t + off];
      __syncthreads();
    }
    if (t == 0) {
      metrics->num_pos = (int64_t)hdr->cnt[0];
      metrics->tp = (int64_t)hdr->cnt[1];
      metrics->fp = (int64_t)hdr->cnt[2];
      metrics->fn = (int64_t)hdr->cnt[3];
      metrics->tn = (int64_t)hdr->cnt[4];
      metrics->ce_sum = sd[0];
    }
  }
}

// ---------------------------------------------------------------- entry points: one complex
template <typename T, bool LAB>
__global__ __launch_bounds__(RK_THREADS) void k_rank_probs(const T* __restrict__ logits, int n, int nv, int per,
                                                           const uint8_t* __restrict__ labels, float threshold,
                                                           float* __restrict__ probs, RankHdr* __restrict__ hdr,
                                                           double* __restrict__ ce_part) {
  rank_probs_body<T, LAB>(blockIdx.x, logits, n, nv, per, labels, threshold, probs, hdr, ce_part);
}
template <int PASS>
__global__ __launch_bounds__(RK_THREADS) void k_rank_hist(const float* __restrict__ probs, int n, int nv, int per,
                                                          uint32_t k, RankHdr* __restrict__ hdr) {
  rank_hist_body<PASS>(blockIdx.x, probs, n, nv, per, k, hdr);
}
__global__ __launch_bounds__(RK_THREADS) void k_rank_count(const float* __restrict__ probs, int n, int nv, int per,
                                                           uint32_t k, RankHdr* __restrict__ hdr,
                                                           uint32_t* __restrict__ wave_eq,
                                                           uint32_t* __restrict__ wave_gt) {
  rank_count_body(blockIdx.x, probs, n, nv, per, k, hdr, wave_eq, wave_gt);
}
__global__ __launch_bounds__(RK_THREADS) void k_rank_compact(const float* __restrict__ probs, int n, int nv, int per,
                                                             int k, const RankHdr* __restrict__ hdr,
                                                             const uint32_t* __restrict__ wave_eq,
                                                             const uint32_t* __restrict__ wave_gt,
                                                             unsigned long long* __restrict__ cand) {
  rank_compact_body(blockIdx.x, probs, n, nv, per, k, hdr, wave_eq, wave_gt, cand);
}
__global__ __launch_bounds__(RK_ONE_THREADS) void k_rank_finish(
    const float* __restrict__ probs, const uint8_t* __restrict__ labels, int n, int k, int kp,
    const unsigned long long* __restrict__ cand, const RankHdr* __restrict__ hdr, const double* __restrict__ ce_part,
    int nb, int32_t* __restrict__ top_ids, float* __restrict__ top_scores, int32_t* __restrict__ top_hits,
    di_rank_metrics* __restrict__ metrics) {
  rank_finish_body(probs, labels, n, k, kp, cand, hdr, ce_part, nb, top_ids, top_scores, top_hits, metrics);
}

// ---------------------------------------------------------------- entry points: the batch
// Grid (the batch's largest block count, count): block (x, y) works on complex y, whose descriptor it
// reads from the device table, and returns at once when x is past that complex's own block count. The
// geometry is rank_geo of that complex's n, as in the single call, so every output has the single
// call's bits. Workspace: the RankHdr of every complex first, contiguous (item i's at
// i * sizeof(RankHdr): one memset), then each complex's wave counts, loss partials and candidates.
struct RankCtx {
  int n;
  RankGeo g;
  RankWork w;
};
__device__ __forceinline__ RankCtx rank_ctx(const di_rank_item& it, char* __restrict__ work) {
  RankCtx c;
  c.n = it.l1 * it.l2;
  c.g = rank_geo(c.n);
  c.w = rank_work(work + it.hdr_off, work + it.work_off);
  return c;
}

template <typename T, bool LAB>
__global__ __launch_bounds__(RK_THREADS) void k_rank_probs_b(const di_rank_item* __restrict__ items,
                                                             char* __restrict__ work, float threshold) {
  const di_rank_item& it = items[blockIdx.y];
  const RankCtx c = rank_ctx(it, work);
  if ((int)blockIdx.x >= c.g.nb) return;
  rank_probs_body<T, LAB>(blockIdx.x, (const T*)it.logits, c.n, c.g.nv, c.g.per, it.labels, threshold, it.probs,
                          c.w.hdr, c.w.ce_part);
}
template <int PASS>
__global__ __launch_bounds__(RK_THREADS) void k_rank_hist_b(const di_rank_item* __restrict__ items,
                                                            char* __restrict__ work) {
  const di_rank_item& it = items[blockIdx.y];
  const RankCtx c = rank_ctx(it, work);
  if ((int)blockIdx.x >= c.g.nb) return;
  rank_hist_body<PASS>(blockIdx.x, it.probs, c.n, c.g.nv, c.g.per, (uint32_t)it.k, c.w.hdr);
}
__global__ __launch_bounds__(RK_THREADS) void k_rank_count_b(const di_rank_item* __restrict__ items,
                                                             char* __restrict__ work) {
  const di_rank_item& it = items[blockIdx.y];
  const RankCtx c = rank_ctx(it, work);
  if ((int)blockIdx.x >= c.g.nb) return;
  rank_count_body(blockIdx.x, it.probs, c.n, c.g.nv, c.g.per, (uint32_t)it.k, c.w.hdr, c.w.wave_eq, c.w.wave_gt);
}
__global__ __launch_bounds__(RK_THREADS) void k_rank_compact_b(const di_rank_item* __restrict__ items,
                                                               char* __restrict__ work) {
  const di_rank_item& it = items[blockIdx.y];
  const RankCtx c = rank_ctx(it, work);
  if ((int)blockIdx.x >= c.g.nb) return;
  rank_compact_body(blockIdx.x, it.probs, c.n, c.g.nv, c.g.per, it.k, c.w.hdr, c.w.wave_eq, c.w.wave_gt, c.w.cand);
}
__global__ __launch_bounds__(RK_ONE_THREADS) void k_rank_finish_b(const di_rank_item* __restrict__ items,
                                                                  char* __restrict__ work) {
  const di_rank_item& it = items[blockIdx.y];
  const RankCtx c = rank_ctx(it, work);
  int kp = 1;
  while (kp < it.k) kp <<= 1;
  rank_finish_body(it.probs, it.labels, c.n, it.k, kp, c.w.cand, c.w.hdr, c.w.ce_part, c.g.nb, it.top_ids,
                   it.top_scores, it.top_hits, it.metrics);
}

static int rank_check_sizes(int64_t n, int64_t k) {
  if (n < 1 || k < 1 || k > n) return DI_EINVAL;
  if (k > DI_RANK_MAX_K || n >= RK_MAX_N) return DI_ERANGE;
  return DI_OK;
}

// every refusal of di_contact_rank, for one complex
static int rank_check_call(int32_t dtype, const void* logits, int32_t l1, int32_t l2, int32_t k, const uint8_t* labels,
                           float threshold, const float* probs, const int32_t* top_ids, const float* top_scores,
                           const int32_t* top_hits, const di_rank_metrics* metrics, const void* work) {
  if (l1 < 1 || l2 < 1) return DI_EINVAL;
  const int64_t n64 = (int64_t)l1 * (int64_t)l2;  // < 2^62
  if (k < 1 || k > n64) return DI_EINVAL;
  if (dtype != DI_F32 && dtype != DI_BF16) return DI_EINVAL;
  if (!logits || !probs || !top_ids || !top_scores || !work) return DI_EINVAL;
  const int with = (labels != nullptr) + (top_hits != nullptr) + (metrics != nullptr);
  if (with != 0 && with != 3) return DI_EINVAL;
  if (threshold != threshold) return DI_EINVAL;
  if (((uintptr_t)probs & 15) || ((uintptr_t)work & 15)) return DI_EINVAL;
  return rank_check_sizes(n64, k);
}

template <typename T>
static void launch_probs(const RankGeo& g, const void* logits, int n, const uint8_t* labels, float threshold,
                         float* probs, const RankWork& w, hipStream_t s) {
  if (labels)
    hipLaunchKernelGGL((k_rank_probs<T, true>), dim3(g.nb), dim3(RK_THREADS), 0, s, (const T*)logits, n, g.nv, g.per,
                       labels, threshold, probs, w.hdr, w.ce_part);
  else
    hipLaunchKernelGGL((k_rank_probs<T, false>), dim3(g.nb), dim3(RK_THREADS), 0, s, (const T*)logits, n, g.nv,
                       g.per, labels, threshold, probs, w.hdr, w.ce_part);
}

template <typename T>
static void launch_probs_b(dim3 grid, bool lab, const di_rank_item* items_dev, char* work, float threshold,
                           hipStream_t s) {
  if (lab)
    hipLaunchKernelGGL((k_rank_probs_b<T, true>), grid, dim3(RK_THREADS), 0, s, items_dev, work, threshold);
  else
    hipLaunchKernelGGL((k_rank_probs_b<T, false>), grid, dim3(RK_THREADS), 0, s, items_dev, work, threshold);
}

// what lies behind the headers for one complex, a multiple of 16 B
static int64_t rank_rest_bytes(int64_t k) {
  const int64_t b = RK_FIXED_BYTES - (int64_t)sizeof(RankHdr) + k * (int64_t)sizeof(unsigned long long);
  return (b + 15) / 16 * 16;
}

// The batch workspace's layout from the items' sizes: off[i] = {hdr_off, work_off} of item i where off
// is given; the total, or the code of the first item whose sizes the single call would refuse.
static int64_t rank_batch_layout(const di_rank_item* items, int32_t count, int64_t (*off)[2]) {
  int64_t at = (int64_t)count * (int64_t)sizeof(RankHdr);
  for (int32_t i = 0; i < count; ++i) {
    if (items[i].l1 < 1 || items[i].l2 < 1) return DI_EINVAL;
    const int rc = rank_check_sizes((int64_t)items[i].l1 * (int64_t)items[i].l2, items[i].k);
    if (rc != DI_OK) return rc;
    if (off) off[i][0] = (int64_t)i * (int64_t)sizeof(RankHdr), off[i][1] = at;
    at += rank_rest_bytes(items[i].k);
  }
  return at;
}

}  // namespace di

using namespace di;

extern "C" int64_t di_contact_rank_work_bytes(int64_t n, int32_t k) {
  const int rc = rank_check_sizes(n, k);
  if (rc != DI_OK) return rc;
  return RK_FIXED_BYTES + (int64_t)k * (int64_t)sizeof(unsigned long long);
}

// The wire record of one complex's ranking: ids | scores | hits | pad to 8 | di_rank_metrics |
// di_auc_metrics | pad to 16 (the last three and hits only with labels). Host arithmetic only.
extern "C" int64_t di_rank_record_bytes(int32_t l1, int32_t l2, int32_t k, int32_t with_labels, int64_t* offsets) {
  if (l1 < 1 || l2 < 1 || (with_labels != 0 && with_labels != 1)) return DI_EINVAL;
  const int rc = rank_check_sizes((int64_t)l1 * (int64_t)l2, k);
  if (rc != DI_OK) return rc;
  const int64_t k4 = (int64_t)k * 4;  // <= 16 KiB
  int64_t off[5] = {0, k4, -1, -1, -1};
  int64_t at = 2 * k4;
  if (with_labels) {
    off[2] = at;
    at = (at + k4 + 7) / 8 * 8;
    off[3] = at;
    at += (int64_t)sizeof(di_rank_metrics);
    off[4] = at;
    at += (int64_t)sizeof(di_auc_metrics);
  }
  if (offsets)
    for (int i = 0; i < 5; ++i) offsets[i] = off[i];
  return (at + 15) / 16 * 16;
}

extern "C" int di_contact_rank(int32_t dtype, const void* logits, int32_t l1, int32_t l2, int32_t k,
                               const uint8_t* labels, float threshold, float* probs, int32_t* top_ids,
                               float* top_scores, int32_t* top_hits, di_rank_metrics* metrics, void* work,
                               void* stream) {
  const int rc = rank_check_call(dtype, logits, l1, l2, k, labels, threshold, probs, top_ids, top_scores, top_hits,
                                 metrics, work);
  if (rc != DI_OK) return rc;

  const int n = l1 * l2;
  const RankGeo g = rank_geo(n);
  const RankWork w = rank_work(work, reinterpret_cast<char*>(work) + sizeof(RankHdr));
  int kp = 1;
  while (kp < k) kp <<= 1;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(w.hdr, 0, sizeof(RankHdr), s);
  if (e != hipSuccess) return (int)e;
  if (dtype == DI_BF16)
    launch_probs<u16>(g, logits, n, labels, threshold, probs, w, s);
  else
    launch_probs<float>(g, logits, n, labels, threshold, probs, w, s);
  const dim3 grid(g.nb), block(RK_THREADS);
  hipLaunchKernelGGL(k_rank_hist<1>, grid, block, 0, s, probs, n, g.nv, g.per, (uint32_t)k, w.hdr);
  hipLaunchKernelGGL(k_rank_hist<2>, grid, block, 0, s, probs, n, g.nv, g.per, (uint32_t)k, w.hdr);
  hipLaunchKernelGGL(k_rank_count, grid, block, 0, s, probs, n, g.nv, g.per, (uint32_t)k, w.hdr, w.wave_eq,
                     w.wave_gt);
  hipLaunchKernelGGL(k_rank_compact, grid, block, 0, s, probs, n, g.nv, g.per, (int)k, w.hdr, w.wave_eq, w.wave_gt,
                     w.cand);
  hipLaunchKernelGGL(k_rank_finish, dim3(1), dim3(RK_ONE_THREADS), 0, s, probs, labels, n, (int)k, kp, w.cand, w.hdr,
                     w.ce_part, g.nb, top_ids, top_scores, top_hits, metrics);
  e = hipGetLastError();
  return e == hipSuccess ? DI_OK : (int)e;
}

extern "C" int64_t di_contact_rank_batch_work_bytes(di_rank_item* items, int32_t count) {
  if (!items || count < 1) return DI_EINVAL;
  if (count > DI_BATCH_MAX) return DI_ERANGE;
  int64_t off[DI_BATCH_MAX][2];
  const int64_t total = rank_batch_layout(items, count, off);
  if (total < 0) return total;
  for (int32_t i = 0; i < count; ++i) items[i].hdr_off = off[i][0], items[i].work_off = off[i][1];
  return total;
}

extern "C" int di_contact_rank_batch(int32_t dtype, const di_rank_item* items, const di_rank_item* items_dev,
                                     int32_t count, float threshold, void* work, void* stream) {
  if (count < 1 || !items || !items_dev) return DI_EINVAL;
  if (count > DI_BATCH_MAX) return DI_ERANGE;
  int max_nb = 1;
  for (int32_t i = 0; i < count; ++i) {
    const di_rank_item& it = items[i];
    const int rc = rank_check_call(dtype, it.logits, it.l1, it.l2, it.k, it.labels, threshold, it.probs, it.top_ids,
                                   it.top_scores, it.top_hits, it.metrics, work);
    if (rc != DI_OK) return rc;
    // one kernel variant serves the batch: labels for every complex or for none
    if ((it.labels != nullptr) != (items[0].labels != nullptr)) return DI_EINVAL;
    const int nb = rank_geo((int64_t)it.l1 * it.l2).nb;
    max_nb = nb > max_nb ? nb : max_nb;
  }
  // the offsets are those di_contact_rank_batch_work_bytes fills (every item's sizes passed above)
  int64_t off[DI_BATCH_MAX][2];
  if (rank_batch_layout(items, count, off) < 0) return DI_EINVAL;
  for (int32_t i = 0; i < count; ++i)
    if (items[i].hdr_off != off[i][0] || items[i].work_off != off[i][1]) return DI_EINVAL;

  hipStream_t s = (hipStream_t)stream;
  char* w = reinterpret_cast<char*>(work);
  hipError_t e = hipMemsetAsync(w, 0, (size_t)count * sizeof(RankHdr), s);
  if (e != hipSuccess) return (int)e;
  const dim3 grid(max_nb, count), block(RK_THREADS);
  if (dtype == DI_BF16)
    launch_probs_b<u16>(grid, items[0].labels != nullptr, items_dev, w, threshold, s);
  else
    launch_probs_b<float>(grid, items[0].labels != nullptr, items_dev, w, threshold, s);
  hipLaunchKernelGGL(k_rank_hist_b<1>, grid, block, 0, s, items_dev, w);
  hipLaunchKernelGGL(k_rank_hist_b<2>, grid, block, 0, s, items_dev, w);
  hipLaunchKernelGGL(k_rank_count_b, grid, block, 0, s, items_dev, w);
  hipLaunchKernelGGL(k_rank_compact_b, grid, block, 0, s, items_dev, w);
  hipLaunchKernelGGL(k_rank_finish_b, dim3(1, count), dim3(RK_ONE_THREADS), 0, s, items_dev, w);
  e = hipGetLastError();
  return e == hipSuccess ? DI_OK : (int)e;
}

