// Exact per-complex AUROC and average precision of class 1 (di_contact_auc): LitGINI.test_step's
// test_auroc / test_auprc (deepinteract_modules.py:2018-2101) from the fp32 map di_contact_rank stored
// and its uint8 labels, without sorting the n = L1 * L2 map. Contact labels are sparse, and both
// figures are determined by the sorted POSITIVE scores plus a histogram of the negatives over the
// gaps between them.
//
//   key(p) = the bits of p (monotone: p >= 0), NaN -> all ones; kernels carry ik = ~key, so that
//   ascending ik is descending p. P / N = positives / negatives by label. The positives' distinct
//   keys, descending: groups g = 0 .. U-1, c_g elements each, TP_g = c_0 + .. + c_g; FP_g = negatives
//   with key >= key_g.
//     u2    = sum_g c_g (2 (N - FP_g) + E_g), E_g = negatives with key == key_g   (exact, < 2^59)
//     auroc = u2 / (2 P N)                    (one correctly rounded fp64 quotient)
//     auprc = sum_g c_g TP_g / (P (TP_g + FP_g))       (fp64 terms, summed in an order fixed by U)
//
// Launch sequence on the caller's stream (no block waits for another; every stage is a kernel; the
// stages after the first read P from the header and return at once where they have nothing to do):
//   memset          the header and the negatives' bins
//   k_auc_collect   one pass over map and labels: num_pos / num_neg / num_nan; the positives' ik
//                   into a max_pos-element buffer. A wave stages its positives in LDS (ballot ranks)
//                   and takes slots with one returning atomic per flush, never one per element; a
//                   slot at or past max_pos is not written (overflow = P > max_pos)
//   P <= 4096:      k_auc_small, one block: bitonic sort in LDS, head flags, scan -> uk, upos, U
//   P  > 4096:      4 x (k_auc_rhist, k_auc_rscan, k_auc_rscatter): stable LSD radix sort, 8 bits a
//                   pass, keys only; every wave owns a contiguous slice, its 256 digit counts are
//                   scanned over the waves (one block per digit) and over the digits, and it scatters
//                   its slice in order with ballot-matched ranks (no atomics). Then k_auc_heads / k_auc_uniq: head flags per
//                   wave, the waves before a block summed by the block -> uk, upos, U
//                   (uk[g] = ik of group g, upos[g] = its first rank: c_g = upos[g+1] - upos[g],
//                   TP_g = upos[g+1])
//   k_auc_bin       second pass over the map: a negative below every positive (most of them) counts
//                   nowhere; one at or above the largest, or equal to the smallest positive is counted
//                   in registers (one atomic per wave and kernel: the bins a saturated map fills); any
//                   other binary-searches uk (10 steps in an LDS table of every stride-th key, the
//                   rest in L2) and adds 1 to eq[g] or gap[g] (integer atomics)
//   k_auc_tiles     the negatives in the bins of every 1024 groups
//   k_auc_terms     per 1024 groups: the tiles before summed, a scan inside -> FP_g; the tile's share of
//                   u2 and of the fp64 sum (group order per thread, a fixed tree per block)
//   k_auc_finish    one block: the tiles' shares in a fixed order, the record
// Algorithmic bytes per element: 2 x (4 + 1) read = 10 B; the sort touches O(P) words.
// di_contact_auc_batch runs the same sequence once for many complexes (grid y = complex; "the batch"
// below): the same kernel bodies on the same per-complex geometry, so the same bits per complex.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "common.h"
#include "../../include/deepinteract_amd.h"

namespace di {

constexpr int AU_THREADS = 256;
constexpr int AU_WAVES = AU_THREADS / 64;
constexpr int AU_MAX_BLOCKS = 1024;
constexpr int AU_ONE_THREADS = 1024;             // the single-block stages
constexpr int AU_SMALL = 4096;                   // positives one block sorts in LDS
constexpr int AU_STAGE = 512;                    // a wave's LDS staging slots in k_auc_collect
constexpr int AU_SORT_MAX_WAVES = 1024;          // slices of the radix sort
constexpr int AU_SORT_KEYS_PER_WAVE = 1024;      // at max_pos keys
constexpr int AU_SAMPLES = 1024;                 // k_auc_bin's LDS table of every stride-th positive key
constexpr int AU_TILE = 4 * AU_THREADS;          // groups per block of k_auc_tiles / k_auc_terms
constexpr int64_t AU_MAX_N = (int64_t)1 << 29;   // as di_contact_rank

// cleared by the launch sequence before every run
struct AucHdr {
  unsigned long long pos, neg, nan;  // by label; NaN scores of either label
  uint32_t slots;                    // slot allocator of the positives' buffer
  uint32_t U;                        // distinct keys among the positives
  uint32_t top_gt, top_eq;           // negatives above / equal to the largest positive key
  uint32_t bot_eq;                   // negatives equal to the smallest positive key (U > 1)
  uint32_t pad[1];
};
static_assert(sizeof(AucHdr) % 16 == 0, "the arrays behind the header stay 16-B aligned");

struct AucWork {
  AucHdr* hdr;
  uint32_t *eq, *gap;        // [A] each, cleared with the header: negatives == key_g / between key_{g-1} and key_g
  uint32_t *keys_a, *keys_b; // [A] the positives' ik, radix ping-pong
  uint32_t *uk, *upos;       // [A] group g's ik and first rank; upos[U] = P
  uint32_t* whist;           // [256][nws] digit-major wave histograms / offsets
  uint32_t* wheads;          // [nws]
  uint32_t* dtot;            // [256] keys per digit
  uint32_t* tsum;            // [tiles] negatives in the bins of each AU_TILE groups
  unsigned long long* part_u2;  // [tiles]
  double* part_ap;              // [tiles]
  int64_t a;                 // max_pos + 1 rounded up to 4 elements
  int nws;                   // waves of the sort grid (a multiple of AU_WAVES)
  int64_t tiles;             // ceil(max_pos / AU_TILE) rounded up to 4
  int64_t clear_bytes, bytes;
};

// work: the cleared part (header, eq, gap); rest: everything else (directly behind it in a single call's
// workspace; in a batch the cleared parts of all complexes are contiguous, so that one memset clears
// them). A function of max_pos alone, on host and device.
__host__ __device__ static inline AucWork auc_work(void* work, void* rest, int64_t max_pos) {
  AucWork w;
  w.a = (max_pos + 1 + 3) / 4 * 4;
  int64_t nws = (max_pos + AU_SORT_KEYS_PER_WAVE - 1) / AU_SORT_KEYS_PER_WAVE;
  nws = (nws + AU_WAVES - 1) / AU_WAVES * AU_WAVES;
  w.nws = (int)(nws > AU_SORT_MAX_WAVES ? AU_SORT_MAX_WAVES : nws);
  w.clear_bytes = (int64_t)sizeof(AucHdr) + 2 * w.a * (int64_t)sizeof(uint32_t);
  w.tiles = ((max_pos + AU_TILE - 1) / AU_TILE + 3) / 4 * 4;
  w.bytes = (int64_t)sizeof(AucHdr) + (6 * w.a + 257 * (int64_t)w.nws + 256 + w.tiles) * (int64_t)sizeof(uint32_t) +
            w.tiles * (int64_t)(sizeof(unsigned long long) + sizeof(double));
  w.hdr = nullptr;
  if (!work) return w;  // sizes only
  char* p = reinterpret_cast<char*>(work);
  w.hdr = reinterpret_cast<AucHdr*>(p);
  w.eq = reinterpret_cast<uint32_t*>(p + sizeof(AucHdr));
  w.gap = w.eq + w.a;
  w.keys_a = reinterpret_cast<uint32_t*>(rest);
  w.keys_b = w.keys_a + w.a;
  w.uk = w.keys_b + w.a;
  w.upos = w.uk + w.a;
  w.whist = w.upos + w.a;
  w.wheads = w.whist + 256 * (int64_t)w.nws;
  w.dtot = w.wheads + w.nws;
  w.tsum = w.dtot + 256;
  w.part_u2 = reinterpret_cast<unsigned long long*>(w.tsum + w.tiles);  // an even count of words behind the header
  w.part_ap = reinterpret_cast<double*>(w.part_u2 + w.tiles);
  return w;
}

// the map passes: nv 4-element vectors over nb blocks of AU_WAVES waves; wave w owns vectors
// [w * per, (w + 1) * per), per a multiple of 64
struct AucGeo {
  int nv, nb, per;
};
__host__ __device__ static inline AucGeo auc_geo(int64_t n) {
  AucGeo g;
  g.nv = (int)((n + 3) / 4);
  const int64_t want = (g.nv + AU_THREADS * 4 - 1) / (AU_THREADS * 4);
  g.nb = (int)(want < 1 ? 1 : (want > AU_MAX_BLOCKS ? AU_MAX_BLOCKS : want));
  const int nw = g.nb * AU_WAVES;
  g.per = ((g.nv + nw - 1) / nw + 63) / 64 * 64;
  return g;
}

__device__ __forceinline__ uint32_t auc_ikey(float p) { return p != p ? 0u : ~__float_as_uint(p); }

// nothing to sort, bin or sum: overflow, a NaN score, or one class empty (k_auc_finish writes NaN)
__device__ __forceinline__ bool auc_idle(const AucHdr* __restrict__ hdr, uint32_t max_pos) {
  return hdr->pos > max_pos || hdr->pos == 0 || hdr->neg == 0 || hdr->nan != 0;
}

// the stored scores and labels of vector v; returns how many of its 4 elements lie inside the map
__device__ __forceinline__ int auc_load4(const float* __restrict__ probs, const uint8_t* __restrict__ labels, int v,
                                         int n, float* p, uint32_t& lab4) {
  const int e = 4 * v;
  if (e + 4 <= n) {
    const floatx4 a = *reinterpret_cast<const floatx4*>(probs + e);
#pragma unroll
    for (int q = 0; q < 4; ++q) p[q] = a[q];
    __builtin_memcpy(&lab4, labels + e, 4);  // byte-aligned only
    return 4;
  }
  const int m = n - e;
  lab4 = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    p[q] = q < m ? probs[e + q] : 0.f;
    lab4 |= q < m ? (uint32_t)labels[e + q] << (8 * q) : 0u;
  }
  return m;
}

// exclusive prefix sum of v over the block's threads (whole waves, at most 16); s: 16 words of LDS
__device__ __forceinline__ uint32_t auc_excl_scan(uint32_t v, uint32_t* s) {
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

// ---------------------------------------------------------------- pass 1: counts, positives
// Every stage is a __device__ body behind two thin entry points: k_x for one complex and k_x_b for a
// batch, where the grid's y index names the complex (see "the batch" below). bx is the block's index
// inside its complex.
__device__ __forceinline__ void auc_collect_body(const int bx, const float* __restrict__ probs,
                                                 const uint8_t* __restrict__ labels, int n, int nv, int per,
                                                 uint32_t max_pos, AucHdr* __restrict__ hdr,
                                                 uint32_t* __restrict__ keys) {
  __shared__ uint32_t stage_all[AU_WAVES][AU_STAGE];
  __shared__ uint32_t red[3][AU_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  volatile uint32_t* stage = stage_all[wave];  // written and read back by this wave only, in program order
  const int lo = (bx * AU_WAVES + wave) * per;
  const int hi = lo + per < nv ? lo + per : nv;
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t c_pos = 0, c_neg = 0, c_nan = 0;
  uint32_t staged = 0;  // wave-uniform (sums of ballot counts)
  auto flush = [&]() {
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&hdr->slots, staged);
    base = __shfl(base, 0);
    for (uint32_t i = lane; i < staged; i += 64)
      if (base + i < max_pos) keys[base + i] = stage[i];  // slot order is free: the sort canonicalises it
    staged = 0;
  };
  for (int v0 = lo; v0 < hi; v0 += 64) {
    const int v = v0 + lane;
    float p[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t lab4 = 0;
    const int m = v < hi ? auc_load4(probs, labels, v, n, p, lab4) : 0;
    uint32_t posm = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool in = q < m, pos = in && ((lab4 >> (8 * q)) & 0xffu) != 0;
      c_pos += pos;
      c_neg += in && !pos;
      c_nan += in && p[q] != p[q];
      posm |= (uint32_t)pos << q;
    }
    if (__ballot(posm != 0) != 0ull) {
      uint32_t before = 0, total = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const unsigned long long b = __ballot((posm >> q) & 1u);
        before += __popcll(b & below);
        total += __popcll(b);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if ((posm >> q) & 1u) stage[staged + before + __popc(posm & ((1u << q) - 1u))] = auc_ikey(p[q]);
      staged += total;
      if (staged > AU_STAGE - 256) flush();  // the next 64 vectors add at most 256
    }
  }
  if (staged) flush();
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    c_pos += __shfl_xor(c_pos, off);
    c_neg += __shfl_xor(c_neg, off);
    c_nan += __shfl_xor(c_nan, off);
  }
  if (lane == 0) red[0][wave] = c_pos, red[1][wave] = c_neg, red[2][wave] = c_nan;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long c[3] = {0, 0, 0};
    for (int w = 0; w < AU_WAVES; ++w)
      for (int j = 0; j < 3; ++j) c[j] += red[j][w];
    if (c[0]) atomicAdd(&hdr->pos, c[0]);
    if (c[1]) atomicAdd(&hdr->neg, c[1]);
    if (c[2]) atomicAdd(&hdr->nan, c[2]);
  }
}

// ---------------------------------------------------------------- P <= AU_SMALL: one block
__device__ __forceinline__ void auc_small_body(AucHdr* __restrict__ hdr, uint32_t max_pos,
                                               const uint32_t* __restrict__ keys, uint32_t* __restrict__ uk,
                                               uint32_t* __restrict__ upos) {
  static_assert(AU_SMALL == 4 * AU_ONE_THREADS, "4 ranks per thread");
  __shared__ uint32_t s[AU_SMALL];
  __shared__ uint32_t sc[16];
  if (auc_idle(hdr, max_pos) || hdr->pos > (unsigned long long)AU_SMALL) return;  // block-uniform
  const int P = (int)hdr->pos, t = threadIdx.x;
  int kp = 2;
  while (kp < P) kp <<= 1;
  // the all-ones padding is the ik of +0.0: it ties with such positives and stays behind rank P
  for (int i = t; i < kp; i += AU_ONE_THREADS) s[i] = i < P ? keys[i] : 0xffffffffu;
  __syncthreads();
  for (int size = 2; size <= kp; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = t; i < (kp >> 1); i += AU_ONE_THREADS) {
        const int a = 2 * i - (i & (stride - 1)), b = a + stride;
        const uint32_t x = s[a], y = s[b];
        if ((x > y) == ((a & size) == 0)) s[a] = y, s[b] = x;
      }
      __syncthreads();
    }
  }
  uint32_t head = 0, mine = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = 4 * t + j;
    if (r < P && (r == 0 || s[r] != s[r - 1])) head |= 1u << j, ++mine;
  }
  uint32_t g = auc_excl_scan(mine, sc);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if ((head >> j) & 1u) {
      uk[g] = s[4 * t + j];
      upos[g] = (uint32_t)(4 * t + j);
      ++g;
    }
  if (t == AU_ONE_THREADS - 1) {
    hdr->U = g;
    upos[g] = (uint32_t)P;
  }
}

// ---------------------------------------------------------------- P > AU_SMALL: radix sort
// wave w of the sort grid owns ranks [w * per, (w + 1) * per) of the P keys
struct AucSlice {
  uint32_t lo, hi;
};
__device__ __forceinline__ AucSlice auc_slice(uint32_t P, int nws, int w) {
  const uint32_t per = ((P + nws - 1) / nws + 63u) / 64u * 64u;
  const unsigned long long lo = (unsigned long long)w * per, hi = lo + per;
  AucSlice s;
  s.lo = (uint32_t)(lo < P ? lo : P);
  s.hi = (uint32_t)(hi < P ? hi : P);
  return s;
}
__device__ __forceinline__ bool auc_sorted_by_block(const AucHdr* __restrict__ hdr, uint32_t max_pos) {
  return auc_idle(hdr, max_pos) || hdr->pos <= (unsigned long long)AU_SMALL;
}

__device__ __forceinline__ void auc_rhist_body(const int bx, const AucHdr* __restrict__ hdr, uint32_t max_pos, int nws,
                                               int shift, const uint32_t* __restrict__ src,
                                               uint32_t* __restrict__ whist) {
  __shared__ uint32_t h[AU_WAVES][256];
  if (auc_sorted_by_block(hdr, max_pos)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, w = bx * AU_WAVES + wave;
  for (int i = lane; i < 256; i += 64) h[wave][i] = 0;
  __syncthreads();
  const AucSlice sl = auc_slice((uint32_t)hdr->pos, nws, w);
  for (uint32_t i = sl.lo + lane; i < sl.hi; i += 64) atomicAdd(&h[wave][(src[i] >> shift) & 255u], 1u);
  __syncthreads();
  for (int d = lane; d < 256; d += 64) whist[(size_t)d * nws + w] = h[wave][d];
}

// block d: exclusive prefix sum of digit d's counts over the waves (a coalesced row of the table), and
// the digit's total
__device__ __forceinline__ void auc_rscan_body(const int bx, const AucHdr* __restrict__ hdr, uint32_t max_pos, int nws,
                                               uint32_t* __restrict__ whist, uint32_t* __restrict__ dtot) {
  static_assert(AU_SORT_MAX_WAVES <= 4 * AU_THREADS, "4 waves' counts per thread");
  __shared__ uint32_t sc[16];
  if (auc_sorted_by_block(hdr, max_pos)) return;
  uint32_t* __restrict__ row = whist + (size_t)bx * nws;
  const int i0 = 4 * threadIdx.x;
  uint32_t c[4], sum = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) sum += c[j] = i0 + j < nws ? row[i0 + j] : 0u;
  uint32_t run = auc_excl_scan(sum, sc);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (i0 + j < nws) row[i0 + j] = run;
    run += c[j];
  }
  if (threadIdx.x == AU_THREADS - 1) dtot[bx] = run;
}

__device__ __forceinline__ void auc_rscatter_body(const int bx, const AucHdr* __restrict__ hdr, uint32_t max_pos,
                                                  int nws, int shift, const uint32_t* __restrict__ src,
                                                  const uint32_t* __restrict__ whist,
                                                  const uint32_t* __restrict__ dtot, uint32_t* __restrict__ dst) {
  static_assert(AU_THREADS == 256, "one thread per digit");
  __shared__ uint32_t off_all[AU_WAVES][256];
  __shared__ uint32_t dbase[256], sc[16];
  if (auc_sorted_by_block(hdr, max_pos)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, w = bx * AU_WAVES + wave;
  dbase[threadIdx.x] = auc_excl_scan(dtot[threadIdx.x], sc);  // the keys with a smaller digit
  __syncthreads();
  volatile uint32_t* off = off_all[wave];  // this wave's running offsets, read and advanced in program order
  for (int d = lane; d < 256; d += 64) off[d] = dbase[d] + whist[(size_t)d * nws + w];
  __syncthreads();
  const uint32_t P = (uint32_t)hdr->pos;
  const AucSlice sl = auc_slice(P, nws, w);
  const unsigned long long below = (1ull << lane) - 1ull;
  for (uint32_t i0 = sl.lo; i0 < sl.hi; i0 += 64) {
    const uint32_t i = i0 + lane;
    const bool in = i < sl.hi;
    const uint32_t k = in ? src[i] : 0u, d = (k >> shift) & 255u;
    unsigned long long same = __ballot(in);  // the lanes holding this lane's digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const unsigned long long bb = __ballot((d >> b) & 1u);
      same &= (d >> b) & 1u ? bb : ~bb;
    }
    if (in) {
      const uint32_t at = off[d] + (uint32_t)__popcll(same & below);
      if (at < P && at < max_pos) dst[at] = k;  // always true for a consistent histogram
    }
    __builtin_amdgcn_wave_barrier();
    if (in && (same >> lane) == 1ull) off[d] += (uint32_t)__popcll(same);  // the digit's last lane
    __builtin_amdgcn_wave_barrier();
  }
}

// head flags of the sorted keys: how many groups start in each wave's slice
__device__ __forceinline__ void auc_heads_body(const int bx, const AucHdr* __restrict__ hdr, uint32_t max_pos, int nws,
                                               const uint32_t* __restrict__ keys, uint32_t* __restrict__ wheads) {
  if (auc_sorted_by_block(hdr, max_pos)) return;
  const int lane = threadIdx.x & 63, w = bx * AU_WAVES + (threadIdx.x >> 6);
  const AucSlice sl = auc_slice((uint32_t)hdr->pos, nws, w);
  uint32_t c = 0;
  for (uint32_t i = sl.lo + lane; i < sl.hi; i += 64) c += i == 0 || keys[i] != keys[i - 1];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if (lane == 0) wheads[w] = c;
}

__device__ __forceinline__ void auc_uniq_body(const int bx, AucHdr* __restrict__ hdr, uint32_t max_pos, int nws,
                                              const uint32_t* __restrict__ keys, const uint32_t* __restrict__ wheads,
                                              uint32_t* __restrict__ uk, uint32_t* __restrict__ upos) {
  __shared__ uint32_t red[AU_WAVES];
  if (auc_sorted_by_block(hdr, max_pos)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int w0 = bx * AU_WAVES, w = w0 + wave;
  uint32_t g = 0;  // the groups that start in the waves before this block
  for (int i = threadIdx.x; i < w0; i += AU_THREADS) g += wheads[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) g += __shfl_xor(g, off);
  if (lane == 0) red[wave] = g;
  __syncthreads();
  g = 0;
#pragma unroll
  for (int i = 0; i < AU_WAVES; ++i) g += red[i] + (i < wave ? wheads[w0 + i] : 0u);
  const uint32_t P = (uint32_t)hdr->pos;
  const AucSlice sl = auc_slice(P, nws, w);
  const unsigned long long below = (1ull << lane) - 1ull;
  for (uint32_t i0 = sl.lo; i0 < sl.hi; i0 += 64) {
    const uint32_t i = i0 + lane;
    const uint32_t k = i < sl.hi ? keys[i] : 0u;
    const bool head = i < sl.hi && (i == 0 || k != keys[i - 1]);
    const unsigned long long b = __ballot(head);
    if (head) {
      const uint32_t at = g + (uint32_t)__popcll(b & below);
      if (at < max_pos) uk[at] = k, upos[at] = i;  // at < U <= P <= max_pos
    }
    g += (uint32_t)__popcll(b);
  }
  if (w == nws - 1 && lane == 0) {  // the last slice ends at P: g is now U
    hdr->U = g;
    if (g <= max_pos) upos[g] = P;
  }
}

// ---------------------------------------------------------------- pass 2: the negatives' bins
__device__ __forceinline__ void auc_bin_body(const int bx, const float* __restrict__ probs,
                                             const uint8_t* __restrict__ labels, int n, int nv, int per,
                                             uint32_t max_pos, AucHdr* __restrict__ hdr,
                                             const uint32_t* __restrict__ uk, uint32_t* __restrict__ eq,
                                             uint32_t* __restrict__ gap) {
  if (auc_idle(hdr, max_pos)) return;
  const uint32_t U = hdr->U;
  if (U == 0 || U > max_pos) return;  // never: P > 0
  const uint32_t k_top = uk[0], k_bot = uk[U - 1];  // ik: k_top <= k_bot
  // every stride-th key in LDS: the first 10 steps of a search stay on chip
  __shared__ uint32_t samp[AU_SAMPLES];
  const uint32_t stride = (U + AU_SAMPLES - 1) / AU_SAMPLES;
  for (uint32_t i = threadIdx.x; i < AU_SAMPLES; i += AU_THREADS) {
    const unsigned long long g = (unsigned long long)i * stride;
    samp[i] = g < U - 1 ? uk[g] : k_bot;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lo = (bx * AU_WAVES + wave) * per;
  const int hi = lo + per < nv ? lo + per : nv;
  uint32_t c_tgt = 0, c_teq = 0, c_beq = 0;
  for (int v = lo + lane; v < hi; v += 64) {
    float p[4];
    uint32_t lab4;
    const int m = auc_load4(probs, labels, v, n, p, lab4);
    uint32_t k[4], a[4], b[4];  // the search range [a, b] inside 1 .. U-1 of a negative between two positives
    bool mid[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool neg = q < m && ((lab4 >> (8 * q)) & 0xffu) == 0;
      k[q] = auc_ikey(p[q]);
      c_tgt += neg && k[q] < k_top;
      c_teq += neg && k[q] == k_top;
      c_beq += neg && k[q] == k_bot && k_bot != k_top;
      mid[q] = neg && k[q] > k_top && k[q] < k_bot;
      // the last sample below k (samp[0] = k_top is): the first g with uk[g] >= k lies behind it, at or
      // before the next sample (or U - 1: uk[U-1] = k_bot > k)
      uint32_t i = 0;
#pragma unroll
      for (uint32_t step = AU_SAMPLES / 2; step > 0; step >>= 1)
        if (samp[i + step] < k[q]) i += step;
      const unsigned long long first = (unsigned long long)i * stride + 1u, last = first - 1u + stride;
      a[q] = mid[q] ? (uint32_t)first : 1u;
      b[q] = mid[q] ? (uint32_t)(last < U - 1 ? last : U - 1) : 1u;
    }
    while ((a[0] < b[0]) | (a[1] < b[1]) | (a[2] < b[2]) | (a[3] < b[3])) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (a[q] < b[q]) {
          const uint32_t c = (a[q] + b[q]) >> 1;
          if (uk[c] >= k[q]) b[q] = c;
          else a[q] = c + 1u;
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (mid[q]) atomicAdd(uk[a[q]] == k[q] ? &eq[a[q]] : &gap[a[q]], 1u);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    c_tgt += __shfl_xor(c_tgt, off);
    c_teq += __shfl_xor(c_teq, off);
    c_beq += __shfl_xor(c_beq, off);
  }
  if (lane == 0) {
    if (c_tgt) atomicAdd(&hdr->top_gt, c_tgt);
    if (c_teq) atomicAdd(&hdr->top_eq, c_teq);
    if (c_beq) atomicAdd(&hdr->bot_eq, c_beq);
  }
}

// ---------------------------------------------------------------- the record
// a / b for 0 <= a, 0 < b < 2^62, correctly rounded but for a second-order term: the two integers'
// conversion errors and the quotient's remainder are folded back in
__device__ __forceinline__ double auc_ratio(unsigned long long a, unsigned long long b) {
  const double ah = (double)a, bh = (double)b;
  const double ar = (double)(long long)(a - (unsigned long long)ah);
  const double br = (double)(long long)(b - (unsigned long long)bh);
  const double q = ah / bh;
  const double rem = fma(-q, bh, ah) + (ar - q * br);
  return q + rem / bh;
}

// The sum over the groups, in three stages. Block b of k_auc_tiles / k_auc_terms owns groups
// [b * AU_TILE, (b + 1) * AU_TILE), thread t four consecutive ones; blocks past U return. The fp64 terms
// are summed in group order per thread, then in fixed trees over the threads of a block and over the
// blocks: an order that is a function of U alone.
struct AucBins {
  const uint32_t *eq, *gap;
  uint32_t U, top_gt, top_eq, bot_eq;
  __device__ __forceinline__ uint32_t eqv(uint32_t g) const {
    return eq[g] + (g == 0 ? top_eq : 0u) + (g == U - 1 ? bot_eq : 0u);
  }
  __device__ __forceinline__ uint32_t gapv(uint32_t g) const { return gap[g] + (g == 0 ? top_gt : 0u); }
};
__device__ __forceinline__ AucBins auc_bins(const AucHdr* __restrict__ hdr, const uint32_t* __restrict__ eq,
                                            const uint32_t* __restrict__ gap) {
  return AucBins{eq, gap, hdr->U, hdr->top_gt, hdr->top_eq, hdr->bot_eq};
}

// tsum[b] = negatives in the bins of tile b
__device__ __forceinline__ void auc_tiles_body(const int bx, const AucHdr* __restrict__ hdr, uint32_t max_pos,
                                               const uint32_t* __restrict__ eq, const uint32_t* __restrict__ gap,
                                               uint32_t* __restrict__ tsum) {
  __shared__ uint32_t red[AU_WAVES];
  if (auc_idle(hdr, max_pos)) return;
  const AucBins bins = auc_bins(hdr, eq, gap);
  const unsigned long long t0 = (unsigned long long)bx * AU_TILE;
  if (bins.U > max_pos || t0 >= bins.U) return;  // block-uniform
  const uint32_t g0 = (uint32_t)t0 + 4u * threadIdx.x;
  uint32_t sum = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j)
    if (g0 + j < bins.U) sum += bins.eqv(g0 + j) + bins.gapv(g0 + j);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) tsum[bx] = red[0] + red[1] + red[2] + red[3];
}

// FP_g from the tiles before this one and a scan inside it; the tile's share of u2 and of the fp64 sum
__device__ __forceinline__ void auc_terms_body(const int bx, const AucHdr* __restrict__ hdr, uint32_t max_pos,
                                               const uint32_t* __restrict__ upos, const uint32_t* __restrict__ eq,
                                               const uint32_t* __restrict__ gap, const uint32_t* __restrict__ tsum,
                                               unsigned long long* __restrict__ part_u2,
                                               double* __restrict__ part_ap) {
  static_assert(AU_WAVES == 4, "red[]");
  __shared__ uint32_t red[AU_WAVES], sc[16];
  __shared__ double sd[AU_THREADS];
  __shared__ unsigned long long su[AU_THREADS];
  if (auc_idle(hdr, max_pos)) return;
  const AucBins bins = auc_bins(hdr, eq, gap);
  const unsigned long long t0 = (unsigned long long)bx * AU_TILE;
  if (bins.U > max_pos || t0 >= bins.U) return;  // block-uniform
  const int t = threadIdx.x;
  const unsigned long long P = hdr->pos, N = hdr->neg;
  uint32_t before = 0;  // the negatives of the tiles before this one
  for (uint32_t i = t; i < (uint32_t)bx; i += AU_THREADS) before += tsum[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off);
  if ((t & 63) == 0) red[t >> 6] = before;
  __syncthreads();
  before = red[0] + red[1] + red[2] + red[3];
  const uint32_t g0 = (uint32_t)t0 + 4u * t;
  uint32_t e[4], gp[4], sum = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    const bool in = g0 + j < bins.U;
    e[j] = in ? bins.eqv(g0 + j) : 0u;
    gp[j] = in ? bins.gapv(g0 + j) : 0u;
    sum += e[j] + gp[j];
  }
  uint32_t fp = before + auc_excl_scan(sum, sc);  // negatives above key_g0
  unsigned long long u2 = 0;
  double ap = 0.0;
  uint32_t tp_prev = g0 < bins.U ? upos[g0] : 0u;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j)
    if (g0 + j < bins.U) {
      const uint32_t tp = upos[g0 + j + 1], c = tp - tp_prev;
      fp += gp[j] + e[j];  // FP_g
      u2 += (unsigned long long)c * (2ull * (N - fp) + e[j]);
      // c TP / (P (TP + FP)): one division of two integers (exact in fp64 while under 2^53)
      ap += (double)((unsigned long long)c * tp) / (double)(P * ((unsigned long long)tp + fp));
      tp_prev = tp;
    }
  sd[t] = ap;
  su[t] = u2;
  __syncthreads();
  for (int off = AU_THREADS / 2; off > 0; off >>= 1) {
    if (t < off) sd[t] += sd[t + off], su[t] += su[t + off];
    __syncthreads();
  }
  if (t == 0) part_ap[bx] = sd[0], part_u2[bx] = su[0];
}

// One block per complex: the tiles' shares folded (thread t: tiles t, t + 1024, .. in order, then a fixed tree),
// the record
__device__ __forceinline__ void auc_finish_body(const AucHdr* __restrict__ hdr, uint32_t max_pos,
                                                const unsigned long long* __restrict__ part_u2,
                                                const double* __restrict__ part_ap,
                                                di_auc_metrics* __restrict__ out) {
  __shared__ double sd[AU_ONE_THREADS];
  __shared__ unsigned long long su[AU_ONE_THREADS];
  const int t = threadIdx.x;
  const unsigned long long P = hdr->pos, N = hdr->neg;
  const uint32_t U = hdr->U;
  if (auc_idle(hdr, max_pos) || U == 0 || U > max_pos) {  // block-uniform
    if (t == 0) {
      out->num_pos = (int64_t)P, out->num_neg = (int64_t)N, out->num_nan = (int64_t)hdr->nan;
      out->pos_distinct = 0;
      out->u2 = 0;
      out->auroc = out->auprc = __longlong_as_double(0x7ff8000000000000ll);
      out->overflow = P > max_pos, out->pad = 0;
    }
    return;
  }
  const uint32_t tiles = (U + AU_TILE - 1) / AU_TILE;
  unsigned long long u2 = 0;
  double ap = 0.0;
  for (uint32_t i = t; i < tiles; i += AU_ONE_THREADS) u2 += part_u2[i], ap += part_ap[i];
  sd[t] = ap;
  su[t] = u2;
  __syncthreads();
  for (int off = AU_ONE_THREADS / 2; off > 0; off >>= 1) {
    if (t < off) sd[t] += sd[t + off], su[t] += su[t + off];
    __syncthreads();
  }
  if (t == 0) {
    out->num_pos = (int64_t)P, out->num_neg = (int64_t)N, out->num_nan = 0;
    out->pos_distinct = (int64_t)U;
    out->u2 = su[0];
    out->auroc = auc_ratio(su[0], 2ull * P * N);
    out->auprc = sd[0];
    out->overflow = 0, out->pad = 0;
  }
}

// ---------------------------------------------------------------- entry points: one complex
__global__ __launch_bounds__(AU_THREADS) void k_auc_collect(const float* __restrict__ probs,
                                                            const uint8_t* __restrict__ labels, int n, int nv, int per,
                                                            uint32_t max_pos, AucHdr* __restrict__ hdr,
                                                            uint32_t* __restrict__ keys) {
  auc_collect_body(blockIdx.x, probs, labels, n, nv, per, max_pos, hdr, keys);
}
__global__ __launch_bounds__(AU_ONE_THREADS) void k_auc_small(AucHdr* __restrict__ hdr, uint32_t max_pos,
                                                              const uint32_t* __restrict__ keys,
                                                              uint32_t* __restrict__ uk, uint32_t* __restrict__ upos) {
  auc_small_body(hdr, max_pos, keys, uk, upos);
}
__global__ __launch_bounds__(AU_THREADS) void k_auc_rhist(const AucHdr* __restrict__ hdr, uint32_t max_pos, int nws,
                                                          int shift, const uint32_t* __restrict__ src,
                                                          uint32_t* __restrict__ whist) {
  auc_rhist_body(blockIdx.x, hdr, max_pos, nws, shift, src, whist);
}
__global__ __launch_bounds__(AU_THREADS) void k_auc_rscan(const AucHdr* __restrict__ hdr, uint32_t max_pos, int nws,
                                                          uint32_t* __restrict__ whist, uint32_t* __restrict__ dtot) {
  auc_rscan_body(blockIdx.x, hdr, max_pos, nws, whist, dtot);
}
__global__ __launch_bounds__(AU_THREADS) void k_auc_rscatter(const AucHdr* __restrict__ hdr, uint32_t max_pos, int nws,
                                                             int shift, const uint32_t* __restrict__ src,
                                                             const uint32_t* __restrict__ whist,
                                                             const uint32_t* __restrict__ dtot,
                                                             uint32_t* __restrict__ dst) {
  auc_rscatter_body(blockIdx.x, hdr, max_pos, nws, shift, src, whist, dtot, dst);
}
__global__ __launch_bounds__(AU_THREADS) void k_auc_heads(const AucHdr* __restrict__ hdr, uint32_t max_pos, int nws,
                                                          const uint32_t* __restrict__ keys,
                                                          uint32_t* __restrict__ wheads) {
  auc_heads_body(blockIdx.x, hdr, max_pos, nws, keys, wheads);
}
__global__ __launch_bounds__(AU_THREADS) void k_auc_uniq(AucHdr* __restrict__ hdr, uint32_t max_pos, int nws,
                                                         const uint32_t* __restrict__ keys,
                                                         const uint32_t* __restrict__ wheads, uint32_t* __restrict__ uk,
                                                         uint32_t* __restrict__ upos) {
  auc_uniq_body(blockIdx.x, hdr, max_pos, nws, keys, wheads, uk, upos);
}
__global__ __launch_bounds__(AU_THREADS) void k_auc_bin(const float* __restrict__ probs,
                                                        const uint8_t* __restrict__ labels, int n, int nv, int per,
                                                        uint32_t max_pos, AucHdr* __restrict__ hdr,
                                                        const uint32_t* __restrict__ uk, uint32_t* __restrict__ eq,
                                                        uint32_t* __restrict__ gap) {
  auc_bin_body(blockIdx.x, probs, labels, n, nv, per, max_pos, hdr, uk, eq, gap);
}
__global__ __launch_bounds__(AU_THREADS) void k_auc_tiles(const AucHdr* __restrict__ hdr, uint32_t max_pos,
                                                          const uint32_t* __restrict__ eq,
                                                          const uint32_t* __restrict__ gap,
                                                          uint32_t* __restrict__ tsum) {
  auc_tiles_body(blockIdx.x, hdr, max_pos, eq, gap, tsum);
}
__global__ __launch_bounds__(AU_THREADS) void k_auc_terms(const AucHdr* __restrict__ hdr, uint32_t max_pos,
                                                          const uint32_t* __restrict__ upos,
                                                          const uint32_t* __restrict__ eq,
                                                          const uint32_t* __restrict__ gap,
                                                          const uint32_t* __restrict__ tsum,
                                                          unsigned long long* __restrict__ part_u2,
                                                          double* __restrict__ part_ap) {
  auc_terms_body(blockIdx.x, hdr, max_pos, upos, eq, gap, tsum, part_u2, part_ap);
}
__global__ __launch_bounds__(AU_ONE_THREADS) void k_auc_finish(const AucHdr* __restrict__ hdr, uint32_t max_pos,
                                                               const unsigned long long* __restrict__ part_u2,
                                                               const double* __restrict__ part_ap,
                                                               di_auc_metrics* __restrict__ out) {
  auc_finish_body(hdr, max_pos, part_u2, part_ap, out);
}

// ---------------------------------------------------------------- entry points: the batch
// Grid (the batch's largest block count of the stage, count): block (x, y) works on complex y, whose
// descriptor it reads from the device table, and returns at once when x is past that complex's own
// block count for the stage (the map passes: auc_geo(n).nb; the sort: nws / AU_WAVES; the sums:
// auc_tile_blocks(max_pos)). Geometry and workspace arrays are auc_geo / auc_work of that complex's n
// and max_pos, as in the single call, so every output has the single call's bits. Workspace: the
// cleared part (AucHdr, eq, gap) of every complex first, contiguous: one memset; then each complex's
// remaining arrays.
__host__ __device__ static inline int auc_tile_blocks(int64_t max_pos) {
  return (int)((max_pos + AU_TILE - 1) / AU_TILE);
}
struct AucCtx {
  int n;
  uint32_t max_pos;
  AucGeo g;
  AucWork w;
};
__device__ __forceinline__ AucCtx auc_ctx(const di_auc_item& it, char* __restrict__ work) {
  AucCtx c;
  c.n = (int)it.n;
  c.max_pos = (uint32_t)it.max_pos;
  c.g = auc_geo(it.n);
  c.w = auc_work(work + it.hdr_off, work + it.work_off, it.max_pos);
  return c;
}

__global__ __launch_bounds__(AU_THREADS) void k_auc_collect_b(const di_auc_item* __restrict__ items,
                                                              char* __restrict__ work) {
  const di_auc_item& it = items[blockIdx.y];
  const AucCtx c = auc_ctx(it, work);
  if ((int)blockIdx.x >= c.g.nb) return;
  auc_collect_body(blockIdx.x, it.probs, it.labels, c.n, c.g.nv, c.g.per, c.max_pos, c.w.hdr, c.w.keys_a);
}
__global__ __launch_bounds__(AU_ONE_THREADS) void k_auc_small_b(const di_auc_item* __restrict__ items,
                                                                char* __restrict__ work) {
  const AucCtx c = auc_ctx(items[blockIdx.y], work);
  auc_small_body(c.w.hdr, c.max_pos, c.w.keys_a, c.w.uk, c.w.upos);
}
// flip: the pass reads keys_b and writes keys_a (passes 1 and 3)
__global__ __launch_bounds__(AU_THREADS) void k_auc_rhist_b(const di_auc_item* __restrict__ items,
                                                            char* __restrict__ work, int shift, int flip) {
  const AucCtx c = auc_ctx(items[blockIdx.y], work);
  if ((int)blockIdx.x >= c.w.nws / AU_WAVES) return;
  auc_rhist_body(blockIdx.x, c.w.hdr, c.max_pos, c.w.nws, shift, flip ? c.w.keys_b : c.w.keys_a, c.w.whist);
}
__global__ __launch_bounds__(AU_THREADS) void k_auc_rscan_b(const di_auc_item* __restrict__ items,
                                                            char* __restrict__ work) {
  const AucCtx c = auc_ctx(items[blockIdx.y], work);
  auc_rscan_body(blockIdx.x, c.w.hdr, c.max_pos, c.w.nws, c.w.whist, c.w.dtot);
}
__global__ __launch_bounds__(AU_THREADS) void k_auc_rscatter_b(const di_auc_item* __restrict__ items,
                                                               char* __restrict__ work, int shift, int flip) {
  const AucCtx c = auc_ctx(items[blockIdx.y], work);
  if ((int)blockIdx.x >= c.w.nws / AU_WAVES) return;
  auc_rscatter_body(blockIdx.x, c.w.hdr, c.max_pos, c.w.nws, shift, flip ? c.w.keys_b : c.w.keys_a, c.w.whist,
                    c.w.dtot, flip ? c.w.keys_a : c.w.keys_b);
}
__global__ __launch_bounds__(AU_THREADS) void k_auc_heads_b(const di_auc_item* __restrict__ items,
                                                            char* __restrict__ work) {
  const AucCtx c = auc_ctx(items[blockIdx.y], work);
  if ((int)blockIdx.x >= c.w.nws / AU_WAVES) return;
  auc_heads_body(blockIdx.x, c.w.hdr, c.max_pos, c.w.nws, c.w.keys_a, c.w.wheads);
}
__global__ __launch_bounds__(AU_THREADS) void k_auc_uniq_b(const di_auc_item* __restrict__ items,
                                                           char* __restrict__ work) {
  const AucCtx c = auc_ctx(items[blockIdx.y], work);
  if ((int)blockIdx.x >= c.w.nws / AU_WAVES) return;
  auc_uniq_body(blockIdx.x, c.w.hdr, c.max_pos, c.w.nws, c.w.keys_a, c.w.wheads, c.w.uk, c.w.upos);
}
__global__ __launch_bounds__(AU_THREADS) void k_auc_bin_b(const di_auc_item* __restrict__ items,
                                                          char* __restrict__ work) {
  const di_auc_item& it = items[blockIdx.y];
  const AucCtx c = auc_ctx(it, work);
  if ((int)blockIdx.x >= c.g.nb) return;
  auc_bin_body(blockIdx.x, it.probs, it.labels, c.n, c.g.nv, c.g.per, c.max_pos, c.w.hdr, c.w.uk, c.w.eq, c.w.gap);
}
__global__ __launch_bounds__(AU_THREADS) void k_auc_tiles_b(const di_auc_item* __restrict__ items,
                                                            char* __restrict__ work) {
  const di_auc_item& it = items[blockIdx.y];
  const AucCtx c = auc_ctx(it, work);
  if ((int)blockIdx.x >= auc_tile_blocks(it.max_pos)) return;
  auc_tiles_body(blockIdx.x, c.w.hdr, c.max_pos, c.w.eq, c.w.gap, c.w.tsum);
}
__global__ __launch_bounds__(AU_THREADS) void k_auc_terms_b(const di_auc_item* __restrict__ items,
                                                            char* __restrict__ work) {
  const di_auc_item& it = items[blockIdx.y];
  const AucCtx c = auc_ctx(it, work);
  if ((int)blockIdx.x >= auc_tile_blocks(it.max_pos)) return;
  auc_terms_body(blockIdx.x, c.w.hdr, c.max_pos, c.w.upos, c.w.eq, c.w.gap, c.w.tsum, c.w.part_u2, c.w.part_ap);
}
__global__ __launch_bounds__(AU_ONE_THREADS) void k_auc_finish_b(const di_auc_item* __restrict__ items,
                                                                 char* __restrict__ work) {
  const di_auc_item& it = items[blockIdx.y];
  const AucCtx c = auc_ctx(it, work);
  auc_finish_body(c.w.hdr, c.max_pos, c.w.part_u2, c.w.part_ap, it.out);
}

static int auc_check_sizes(int64_t n, int64_t max_pos) {
  if (n < 1 || max_pos < 1 || max_pos > n) return DI_EINVAL;
  if (n >= AU_MAX_N) return DI_ERANGE;
  return DI_OK;
}

// every refusal of di_contact_auc, for one complex
static int auc_check_call(const float* probs, const uint8_t* labels, int64_t n, int64_t max_pos,
                          const di_auc_metrics* out, const void* work) {
  const int rc = auc_check_sizes(n, max_pos);
  if (rc != DI_OK) return rc;
  if (!probs || !labels || !out || !work) return DI_EINVAL;
  if (((uintptr_t)probs & 15) || ((uintptr_t)work & 15)) return DI_EINVAL;
  return DI_OK;
}

// The batch workspace's layout from the items' sizes: off[i] = {hdr_off, work_off} of item i where off
// is given; *clear = the bytes at the front that the call clears; the total, or the code of the first
// item whose sizes the single call would refuse. Every part is a multiple of 16 B.
static int64_t auc_batch_layout(const di_auc_item* items, int32_t count, int64_t (*off)[2], int64_t* clear) {
  int64_t at = 0;
  for (int32_t i = 0; i < count; ++i) {
    const int rc = auc_check_sizes(items[i].n, items[i].max_pos);
    if (rc != DI_OK) return rc;
    if (off) off[i][0] = at;
    at += auc_work(nullptr, nullptr, items[i].max_pos).clear_bytes;
  }
  if (clear) *clear = at;
  for (int32_t i = 0; i < count; ++i) {
    const AucWork w = auc_work(nullptr, nullptr, items[i].max_pos);
    if (off) off[i][1] = at;
    at += w.bytes - w.clear_bytes;
  }
  return at;
}

}  // namespace di

using namespace di;

extern "C" int64_t di_contact_auc_work_bytes(int64_t n, int64_t max_pos) {
  const int rc = auc_check_sizes(n, max_pos);
  if (rc != DI_OK) return rc;
  return auc_work(nullptr, nullptr, max_pos).bytes;
}

extern "C" int di_contact_auc(const float* probs, const uint8_t* labels, int64_t n64, int64_t max_pos64,
                              di_auc_metrics* out, void* work, void* stream) {
  const int rc = auc_check_call(probs, labels, n64, max_pos64, out, work);
  if (rc != DI_OK) return rc;

  const int n = (int)n64;
  const uint32_t max_pos = (uint32_t)max_pos64;
  const AucGeo g = auc_geo(n);
  const int64_t clear_bytes = auc_work(nullptr, nullptr, max_pos64).clear_bytes;
  const AucWork w = auc_work(work, reinterpret_cast<char*>(work) + clear_bytes, max_pos64);
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(w.hdr, 0, (size_t)w.clear_bytes, s);
  if (e != hipSuccess) return (int)e;
  const dim3 grid(g.nb), block(AU_THREADS), one(1), wide(AU_ONE_THREADS), sgrid(w.nws / AU_WAVES);
  const dim3 tgrid((unsigned)auc_tile_blocks(max_pos64));
  hipLaunchKernelGGL(k_auc_collect, grid, block, 0, s, probs, labels, n, g.nv, g.per, max_pos, w.hdr, w.keys_a);
  hipLaunchKernelGGL(k_auc_small, one, wide, 0, s, w.hdr, max_pos, w.keys_a, w.uk, w.upos);
  uint32_t *src = w.keys_a, *dst = w.keys_b;
  for (int shift = 0; shift < 32; shift += 8) {
    hipLaunchKernelGGL(k_auc_rhist, sgrid, block, 0, s, w.hdr, max_pos, w.nws, shift, src, w.whist);
    hipLaunchKernelGGL(k_auc_rscan, dim3(256), block, 0, s, w.hdr, max_pos, w.nws, w.whist, w.dtot);
    hipLaunchKernelGGL(k_auc_rscatter, sgrid, block, 0, s, w.hdr, max_pos, w.nws, shift, src, w.whist, w.dtot,
                       dst);
    uint32_t* t = src;
    src = dst, dst = t;
  }
  // four passes: the sorted keys are back in keys_a
  hipLaunchKernelGGL(k_auc_heads, sgrid, block, 0, s, w.hdr, max_pos, w.nws, w.keys_a, w.wheads);
  hipLaunchKernelGGL(k_auc_uniq, sgrid, block, 0, s, w.hdr, max_pos, w.nws, w.keys_a, w.wheads, w.uk, w.upos);
  hipLaunchKernelGGL(k_auc_bin, grid, block, 0, s, probs, labels, n, g.nv, g.per, max_pos, w.hdr, w.uk, w.eq, w.gap);
  hipLaunchKernelGGL(k_auc_tiles, tgrid, block, 0, s, w.hdr, max_pos, w.eq, w.gap, w.tsum);
  hipLaunchKernelGGL(k_auc_terms, tgrid, block, 0, s, w.hdr, max_pos, w.upos, w.eq, w.gap, w.tsum, w.part_u2,
                     w.part_ap);
  hipLaunchKernelGGL(k_auc_finish, one, wide, 0, s, w.hdr, max_pos, w.part_u2, w.part_ap, out);
  e = hipGetLastError();
  return e == hipSuccess ? DI_OK : (int)e;
}

extern "C" int64_t di_contact_auc_batch_work_bytes(di_auc_item* items, int32_t count) {
  if (!items || count < 1) return DI_EINVAL;
  if (count > DI_BATCH_MAX) return DI_ERANGE;
  int64_t off[DI_BATCH_MAX][2];
  const int64_t total = auc_batch_layout(items, count, off, nullptr);
  if (total < 0) return total;
  for (int32_t i = 0; i < count; ++i) items[i].hdr_off = off[i][0], items[i].work_off = off[i][1];
  return total;
}

extern "C" int di_contact_auc_batch(const di_auc_item* items, const di_auc_item* items_dev, int32_t count,
                                    void* work, void* stream) {
  if (count < 1 || !items || !items_dev) return DI_EINVAL;
  if (count > DI_BATCH_MAX) return DI_ERANGE;
  int max_nb = 1, max_sort = 1, max_tiles = 1;
  for (int32_t i = 0; i < count; ++i) {
    const di_auc_item& it = items[i];
    const int rc = auc_check_call(it.probs, it.labels, it.n, it.max_pos, it.out, work);
    if (rc != DI_OK) return rc;
    const int nb = auc_geo(it.n).nb, sort = auc_work(nullptr, nullptr, it.max_pos).nws / AU_WAVES;
    const int tiles = auc_tile_blocks(it.max_pos);
    max_nb = nb > max_nb ? nb : max_nb;
    max_sort = sort > max_sort ? sort : max_sort;
    max_tiles = tiles > max_tiles ? tiles : max_tiles;
  }
  // the offsets are those di_contact_auc_batch_work_bytes fills (every item's sizes passed above)
  int64_t off[DI_BATCH_MAX][2], clear_bytes = 0;
  if (auc_batch_layout(items, count, off, &clear_bytes) < 0) return DI_EINVAL;
  for (int32_t i = 0; i < count; ++i)
    if (items[i].hdr_off != off[i][0] || items[i].work_off != off[i][1]) return DI_EINVAL;

  hipStream_t s = (hipStream_t)stream;
  char* w = reinterpret_cast<char*>(work);
  hipError_t e = hipMemsetAsync(w, 0, (size_t)clear_bytes, s);
  if (e != hipSuccess) return (int)e;
  const dim3 block(AU_THREADS), wide(AU_ONE_THREADS), one(1, count);
  const dim3 grid(max_nb, count), sgrid(max_sort, count), dgrid(256, count), tgrid(max_tiles, count);
  hipLaunchKernelGGL(k_auc_collect_b, grid, block, 0, s, items_dev, w);
  hipLaunchKernelGGL(k_auc_small_b, one, wide, 0, s, items_dev, w);
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(k_auc_rhist_b, sgrid, block, 0, s, items_dev, w, 8 * pass, pass & 1);
    hipLaunchKernelGGL(k_auc_rscan_b, dgrid, block, 0, s, items_dev, w);
    hipLaunchKernelGGL(k_auc_rscatter_b, sgrid, block, 0, s, items_dev, w, 8 * pass, pass & 1);
  }
  // four passes: the sorted keys are back in keys_a
  hipLaunchKernelGGL(k_auc_heads_b, sgrid, block, 0, s, items_dev, w);
  hipLaunchKernelGGL(k_auc_uniq_b, sgrid, block, 0, s, items_dev, w);
  hipLaunchKernelGGL(k_auc_bin_b, grid, block, 0, s, items_dev, w);
  hipLaunchKernelGGL(k_auc_tiles_b, tgrid, block, 0, s, items_dev, w);
  hipLaunchKernelGGL(k_auc_terms_b, tgrid, block, 0, s, items_dev, w);
  hipLaunchKernelGGL(k_auc_finish_b, one, wide, 0, s, items_dev, w);
  e = hipGetLastError();
  return e == hipSuccess ? DI_OK : (int)e;
}

