// Example lists on the device (di_examples_labels_batch, di_examples_gather_batch): the reference's
// `examples` [n, 3] = (i, j, label) rows of each complex of a ragged batch, turned into what the
// ranking and AUC ops take, in ONE launch (plus one memset) whatever the number of complexes.
//
//   labels   a complete list (every pair exactly once): labels[i * l2 + j] = label, uint8
//   gather   a sampled list (any count, any order, repeats allowed), as LitGINI.validation_step reads
//            it (deepinteract_modules.py:1915-1982): pool_logits[c * total + out_off + r] =
//            logits[c, i_r, j_r] and pool_labels[out_off + r] = label_r, where a pool is the
//            reference's torch.cat over the complexes of one validation batch
//
// Both leave one int32 flag word per complex: DI_EX_OUTSIDE (an index outside the complex),
// DI_EX_LABEL (a label other than 0 / 1), DI_EX_TWICE (labels only: a pair listed twice). With
// n == l1 * l2, no DI_EX_OUTSIDE and no DI_EX_TWICE every pair is covered, so "missing" needs no
// second pass.
//
// A pair listed twice is found with a 1-bit-per-pair bitmap (cleared by the call's memset) and
// atomicOr at agent scope, which RETURNS the word as it was: of two rows naming one pair, whichever
// the memory system orders second sees the bit the first set. Which one that is depends on
// scheduling; that ONE of them sees it does not, and the flag is an idempotent atomicOr of a
// constant, so the flag word is a function of the list alone. A plain read-modify-write of the word
// would not do: two waves on different XCDs may both read the old word from their own L2.
// Rows of a sorted list put up to 32 consecutive lanes on one bitmap word. When the rows a wave holds
// are consecutive pairs (flat index = the first lane's + lane: checked, never assumed) the first lane
// on each word ORs in the mask of all of them, 2-3 atomics a wave instead of 64; such a mask cannot
// name a pair twice itself, and an overlap with any other row's bit or mask shows in the returned
// word exactly as above. Any other wave takes one atomic a row. (One atomic a row on every wave
// measured 1.3-8x slower on sorted lists and the same on shuffled ones: DESIGN.md section 8.)
//
// Indices are compared in their own width (int64 or int32) before anything is narrowed: 2^40 or -1 is
// "outside", not a wrapped 32-bit value. A row that is outside touches no memory but its flag.
// Grid (the batch's largest block count, count): block (x, y) works on complex y, whose descriptor it
// reads from the device table, and returns at once when x is past that complex's own block count.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"
#include "../../include/deepinteract_amd.h"

namespace di {

constexpr int EX_THREADS = 256;
constexpr int EX_PER = 4;                             // rows per thread
constexpr int EX_BLOCK_ROWS = EX_THREADS * EX_PER;    // DI_EX_BLOCK_ROWS
constexpr int64_t EX_MAX_N = (int64_t)1 << 29;        // pairs of one complex: the maps' limit
constexpr int64_t EX_MAX_TOTAL = (int64_t)1 << 31;    // rows of one pool / one sampled list
static_assert(EX_BLOCK_ROWS == DI_EX_BLOCK_ROWS, "the header's constant");

// OR over the wave, flushed by one lane: at most one atomic per wave and flag word
__device__ __forceinline__ void flag_flush(int f, int32_t* __restrict__ flag) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) f |= __shfl_xor(f, m);
  if ((threadIdx.x & 63) == 0 && f) atomicOr(flag, f);
}

// the word as it was, at agent scope: one answer for the waves of every XCD
__device__ __forceinline__ uint32_t fetch_or(uint32_t* p, uint32_t v) {
  return __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename I>
struct ExRow {
  I i, j, lab;
};
template <typename I>
__device__ __forceinline__ ExRow<I> ex_load(const I* __restrict__ ex, int64_t r) {
  ExRow<I> row;
  row.i = ex[3 * r], row.j = ex[3 * r + 1], row.lab = ex[3 * r + 2];
  return row;
}
// flag bits of a row; `inside` says whether its indices may be used
template <typename I>
__device__ __forceinline__ int ex_flags(const ExRow<I>& row, int l1, int l2, bool& inside) {
  inside = row.i >= (I)0 && row.i < (I)l1 && row.j >= (I)0 && row.j < (I)l2;   // in I's width
  return (inside ? 0 : DI_EX_OUTSIDE) | ((row.lab == (I)0 || row.lab == (I)1) ? 0 : DI_EX_LABEL);
}

template <typename I>
__global__ __launch_bounds__(EX_THREADS) void k_examples_labels(const di_examples_item* __restrict__ items,
                                                                char* __restrict__ work) {
  const di_examples_item& it = items[blockIdx.y];
  const int64_t n = it.n;
  const int64_t first = (int64_t)blockIdx.x * EX_BLOCK_ROWS;
  if (first >= n) return;
  const I* __restrict__ ex = (const I*)it.examples;
  const int l1 = it.l1, l2 = it.l2;
  uint8_t* __restrict__ labels = it.labels;
  uint32_t* __restrict__ bits = reinterpret_cast<uint32_t*>(work + it.work_off);
  const int lane = threadIdx.x & 63;
  int f = 0;
#pragma unroll
  for (int s = 0; s < EX_PER; ++s) {
    const int64_t r = first + s * EX_THREADS + threadIdx.x;   // a wave holds 64 consecutive rows
    const bool have = r < n;
    bool inside = false;
    int flat = -1;
    if (have) {
      const ExRow<I> row = ex_load(ex, r);
      f |= ex_flags(row, l1, l2, inside);
      if (inside) {
        flat = (int)row.i * l2 + (int)row.j;   // < l1 * l2 < 2^29
        labels[flat] = (uint8_t)row.lab;
      }
    }
    // the wave's rows are consecutive pairs: every lane that has a row is inside and at flat0 + lane
    // (rows past n are the wave's last lanes)
    const int flat0 = __shfl(flat, 0);
    const bool run = __all(!have || (inside && flat == flat0 + lane)) && flat0 >= 0;
    if (run) {
      const int nact = __popcll(__ballot(have));
      const int bit = flat & 31;
      if (have && (lane == 0 || bit == 0)) {
        const int left = nact - lane, room = 32 - bit;
        const int cnt = left < room ? left : room;
        const uint32_t mask = (cnt == 32 ? 0xffffffffu : ((1u << cnt) - 1u)) << bit;
        if (fetch_or(&bits[flat >> 5], mask) & mask) f |= DI_EX_TWICE;
      }
    } else if (inside) {
      const uint32_t mask = 1u << (flat & 31);
      if (fetch_or(&bits[flat >> 5], mask) & mask) f |= DI_EX_TWICE;
    }
  }
  flag_flush(f, reinterpret_cast<int32_t*>(work) + blockIdx.y);
}

template <typename T, typename I>
__global__ __launch_bounds__(EX_THREADS) void k_examples_gather(const di_examples_item* __restrict__ items,
                                                                int32_t* __restrict__ flags) {
  const di_examples_item& it = items[blockIdx.y];
  const int64_t n = it.n;
  const int64_t first = (int64_t)blockIdx.x * EX_BLOCK_ROWS;
  if (first >= n) return;
  const I* __restrict__ ex = (const I*)it.examples;
  const T* __restrict__ logits = (const T*)it.logits;
  const int l1 = it.l1, l2 = it.l2;
  const int64_t plane = (int64_t)l1 * l2, total = it.total;
  T* __restrict__ out = (T*)it.pool_logits + it.out_off;
  uint8_t* __restrict__ out_lab = it.pool_labels + it.out_off;
  int f = 0;
#pragma unroll
  for (int s = 0; s < EX_PER; ++s) {
    const int64_t r = first + s * EX_THREADS + threadIdx.x;
    if (r < n) {
      const ExRow<I> row = ex_load(ex, r);
      bool inside;
      f |= ex_flags(row, l1, l2, inside);
      if (inside) {
        const int64_t flat = (int64_t)row.i * l2 + (int64_t)row.j;
        out[r] = logits[flat];
        out[total + r] = logits[plane + flat];
        out_lab[r] = (uint8_t)row.lab;
      }
    }
  }
  flag_flush(f, flags + blockIdx.y);
}

static int64_t ex_blocks(int64_t n) { return (n + EX_BLOCK_ROWS - 1) / EX_BLOCK_ROWS; }
static int64_t ex_flag_bytes(int64_t count) { return (count * 4 + 15) / 16 * 16; }
static int64_t ex_bitmap_bytes(int64_t n) { return ((n + 31) / 32 * 4 + 15) / 16 * 16; }

// what both modes ask of one item
static int ex_check_item(const di_examples_item& it, int32_t idx_dtype) {
  if (!it.examples || it.n < 1 || it.l1 < 1 || it.l2 < 1) return DI_EINVAL;
  if ((uintptr_t)it.examples & (idx_dtype == DI_I64 ? 7 : 3)) return DI_EINVAL;
  return DI_OK;
}

// The labels workspace from the items' sizes: the flag words of every complex first, then each
// complex's bitmap (all of it cleared by one memset). off[i] = work_off of item i where off is given;
// the total, or the code of the first item refused.
static int64_t ex_labels_layout(const di_examples_item* items, int32_t count, int64_t* off) {
  int64_t at = ex_flag_bytes(count);
  for (int32_t i = 0; i < count; ++i) {
    const di_examples_item& it = items[i];
    if (it.n < 1 || it.l1 < 1 || it.l2 < 1) return DI_EINVAL;
    const int64_t pairs = (int64_t)it.l1 * (int64_t)it.l2;
    if (it.n != pairs) return DI_EINVAL;
    if (pairs >= EX_MAX_N) return DI_ERANGE;
    if (off) off[i] = at;
    at += ex_bitmap_bytes(pairs);
  }
  return at;
}

}  // namespace di

using namespace di;

extern "C" int64_t di_examples_labels_work_bytes(di_examples_item* items, int32_t count) {
  if (!items || count < 1) return DI_EINVAL;
  if (count > DI_BATCH_MAX) return DI_ERANGE;
  int64_t off[DI_BATCH_MAX];
  const int64_t total = ex_labels_layout(items, count, off);
  if (total < 0) return total;
  for (int32_t i = 0; i < count; ++i) items[i].work_off = off[i];
  return total;
}

extern "C" int di_examples_labels_batch_check(int32_t idx_dtype, const di_examples_item* items,
                                              const di_examples_item* items_dev, int32_t count, const void* work) {
  if (count < 1 || !items || !items_dev || !work) return DI_EINVAL;
  if (count > DI_BATCH_MAX) return DI_ERANGE;
  if (idx_dtype != DI_I64 && idx_dtype != DI_I32) return DI_EINVAL;
  if ((uintptr_t)work & 15) return DI_EINVAL;
  for (int32_t i = 0; i < count; ++i) {
    const int rc = ex_check_item(items[i], idx_dtype);
    if (rc != DI_OK) return rc;
    if (!items[i].labels) return DI_EINVAL;
  }
  int64_t off[DI_BATCH_MAX];
  const int64_t total = ex_labels_layout(items, count, off);
  if (total < 0) return (int)total;
  for (int32_t i = 0; i < count; ++i)
    if (items[i].work_off != off[i]) return DI_EINVAL;   // not the helper's
  return DI_OK;
}

extern "C" int di_examples_labels_batch(int32_t idx_dtype, const di_examples_item* items,
                                        const di_examples_item* items_dev, int32_t count, void* work,
                                        void* stream) {
  const int rc = di_examples_labels_batch_check(idx_dtype, items, items_dev, count, work);
  if (rc != DI_OK) return rc;
  int64_t max_nb = 1;
  for (int32_t i = 0; i < count; ++i) {
    const int64_t nb = ex_blocks(items[i].n);
    max_nb = nb > max_nb ? nb : max_nb;
  }
  const int64_t clear = ex_labels_layout(items, count, nullptr);
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(work, 0, (size_t)clear, s);
  if (e != hipSuccess) return (int)e;
  const dim3 grid((unsigned)max_nb, count), block(EX_THREADS);
  if (idx_dtype == DI_I64)
    hipLaunchKernelGGL(k_examples_labels<int64_t>, grid, block, 0, s, items_dev, (char*)work);
  else
    hipLaunchKernelGGL(k_examples_labels<int32_t>, grid, block, 0, s, items_dev, (char*)work);
  e = hipGetLastError();
  return e == hipSuccess ? DI_OK : (int)e;
}

extern "C" int di_examples_gather_batch_check(int32_t dtype, int32_t idx_dtype, const di_examples_item* items,
                                              const di_examples_item* items_dev, int32_t count,
                                              const int32_t* flags) {
  if (count < 1 || !items || !items_dev || !flags) return DI_EINVAL;
  if (count > DI_BATCH_MAX) return DI_ERANGE;
  if (dtype != DI_F32 && dtype != DI_BF16) return DI_EINVAL;
  if (idx_dtype != DI_I64 && idx_dtype != DI_I32) return DI_EINVAL;
  if ((uintptr_t)flags & 3) return DI_EINVAL;
  const uintptr_t elem = dtype == DI_F32 ? 3 : 1;
  for (int32_t i = 0; i < count; ++i) {
    const di_examples_item& it = items[i];
    const int rc = ex_check_item(it, idx_dtype);
    if (rc != DI_OK) return rc;
    if (!it.logits || !it.pool_logits || !it.pool_labels) return DI_EINVAL;
    if (((uintptr_t)it.logits & elem) || ((uintptr_t)it.pool_logits & elem)) return DI_EINVAL;
    // the item's rows lie inside its pool
    if (it.total < 1 || it.out_off < 0 || it.out_off > it.total || it.n > it.total - it.out_off) return DI_EINVAL;
    if ((int64_t)it.l1 * (int64_t)it.l2 >= EX_MAX_N || it.total >= EX_MAX_TOTAL) return DI_ERANGE;
  }
  return DI_OK;
}

extern "C" int di_examples_gather_batch(int32_t dtype, int32_t idx_dtype, const di_examples_item* items,
                                        const di_examples_item* items_dev, int32_t count, int32_t* flags,
                                        void* stream) {
  const int rc = di_examples_gather_batch_check(dtype, idx_dtype, items, items_dev, count, flags);
  if (rc != DI_OK) return rc;
  int64_t max_nb = 1;
  for (int32_t i = 0; i < count; ++i) {
    const int64_t nb = ex_blocks(items[i].n);
    max_nb = nb > max_nb ? nb : max_nb;
  }
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(flags, 0, (size_t)count * sizeof(int32_t), s);
  if (e != hipSuccess) return (int)e;
  const dim3 grid((unsigned)max_nb, count), block(EX_THREADS);
  const bool wide = idx_dtype == DI_I64;
  if (dtype == DI_BF16) {
    if (wide) hipLaunchKernelGGL((k_examples_gather<u16, int64_t>), grid, block, 0, s, items_dev, flags);
    else hipLaunchKernelGGL((k_examples_gather<u16, int32_t>), grid, block, 0, s, items_dev, flags);
  } else {
    if (wide) hipLaunchKernelGGL((k_examples_gather<float, int64_t>), grid, block, 0, s, items_dev, flags);
    else hipLaunchKernelGGL((k_examples_gather<float, int32_t>), grid, block, 0, s, items_dev, flags);
  }
  e = hipGetLastError();
  return e == hipSuccess ? DI_OK : (int)e;
}
