// GeoT forward kernels for gfx950 (MI355X), one translation unit per stage: node embedding and
// InitEdge (geot_init.hip), fused edge layer (geot_edge.hip), fused node layer (geot_node.hip); the
// blob / version queries of the C ABI are geot_abi.hip. This header holds what more than one stage
// uses: the kernel argument structs, lane / row indexing, the launch geometry, the attention fold's
// tile constants and the host launch helpers. Device engine: common.h ("row-on-lane" transposed
// activations, MFMA 16x16 chains with weights streamed through LDS by LDS-DMA).
//
// Reference semantics (paths relative to the reference project's project/utils/):
//   node embedding            deepinteract_modules.py:1541-1543, 1663-1664
//   InitEdgeModule            deepinteract_modules.py:198-264
//   ConformationModule        deepinteract_modules.py:373-455 (+ ResBlock :458-497)
//   attention edge UDFs       deepinteract_modules.py:76-96, graph_utils.py:21-63
//   GT layer residual / FFN   deepinteract_modules.py:669-727 (intermediate), :892-946 (final)
// Algebraic rewrites (exact in real arithmetic, fp32-rounding-level differences only):
//   * eval BatchNorm folded into the following/preceding linear (host packing);
//   * nbr_linear applied once per edge (Fn = F W^T + b) and gathered, instead of per gathered row;
//   * two-stage geometric embeddings (W1 . W0 . g) pre-multiplied on the host;
//   * InitEdge's emb[src]/emb[dst] slots of combined_linear_0 precomputed per node position
//     (pos tables [2304,128]); the 4 final gates summed before multiplying (a*x+b*x = (a+b)*x).
#pragma once
#include "common.h"
#include "layout.h"
#include "../../include/deepinteract_amd.h"

namespace di {

struct EmbedArgs {
  int Nt;
  int in_dim;
  const float* node_f;
  const void* wmat;
  const float* wvec;
  void* h_out;
  void* qkv_out;
  uint32_t* sig_q;  // optional pair queue: raise its READY to sig_job + 1 at launch start (pair_queue.h)
  int sig_job;
};

struct InitArgs {
  int Et;
  const float* edge_f;
  const int* src;
  const int* dst;
  const int* node_pos;
  const void* wmat;
  const float* wvec;
  const float* pos_src;
  const float* pos_dst;
  void* f_out;
  void* fn_out;
};

struct EdgeArgs {
  int Et;
  const float* edge_f;
  const int* src;
  const int* dst;
  const int* nbr;
  const void* f_in;
  const void* fn_in;
  const void* qkv;
  const void* wmat;
  const float* wvec;
  float* alpha_out;
  void* f_out;
  void* fn_out;
  // di_edge_layer_attn (bf16): the attention aggregation folded into the epilogue (edge_attn_fold)
  float* attn_out = nullptr;
  float* attn_parts = nullptr;
  const int* in_ptr = nullptr;
  // di_edge_layer_z (bf16 layer 0): f_in holds z0 rows; the InitEdge blob whose combined_linear_2
  // blocks rebuild F0 from them
  const void* init_wmat = nullptr;
};

struct NodeArgs {
  int Nt;
  const float* attn;  // optional [Nt, 128] aggregated attention rows (k_node_aggr); null: gather here
  void* hT_out;  // optional [128, Nt] transposed copy of h_out (pair-tensor input)
  const int* src;
  const int* in_ptr;
  const float* alpha;
  const void* h_in;
  const void* qkv;
  const void* wmat;
  const float* wvec;
  void* h_out;
  void* qkv_out;
  // with attn: di_edge_layer_attn's partial sums of the destinations split over edge tiles
  // (attn_row; in_ptr is then the CSR row pointer)
  const float* attn_parts = nullptr;
};

struct AggrArgs {
  int Nt;
  const int* src;
  const int* in_ptr;
  const float* alpha;
  const void* qkv;
  float* attn;
};

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
// A bijection of [0, n) that turns slot j, run on XCD j mod 8 (blocks are dealt round-robin over
// the 8 XCDs: b and b + 8 share one -- speed only, correct under any placement), into
// base(j mod 8) + j / 8: the slots of one XCD cover one contiguous range, so neighbouring rows
// (a destination range's gathered K / Q / V rows) stay in that XCD's L2.
// (n = 8q + r: XCD y holds q + [y < r] slots, so base(x) = x q + min(x, r))
__device__ __forceinline__ int xcd_slot(int j, int n) {
  const int x = j & 7;
  return x * (n >> 3) + min(x, n & 7) + (j >> 3);
}
template <int NW>
__device__ __forceinline__ int row_id() {
  return blockIdx.x * (NW * ROWS_PER_WAVE) + (threadIdx.x >> 6) * ROWS_PER_WAVE + (threadIdx.x & 15);
}

// Launch geometry of k_edge_layer per storage dtype: 4-wave blocks, two per CU (<= 240 VGPRs each).
// Two independent blocks per CU matter: the waves of ONE block meet at every stage barrier in
// lockstep, so only waves of the other block can fill a SIMD's MFMA pipe while these run their SiLU
// VALU work (and vice versa). bf16 (di_conformation) double-buffers its weight stages (2 x 36.5 KiB
// per block) so the LDS-DMA of layer i+1 runs under layer i's MFMAs; fp32 (stages twice as large,
// 72.5 KiB) stages synchronously through one slot.
template <class DT>
struct Geo : KernelGeo<4> {
  static constexpr bool DBUF = DT::kBF16;
};

// The edge's own input row F: bf16 path keeps it in registers as a packed MFMA operand (its
// stored values are bf16, so unpacking is exact); fp32 path re-reads it (L2) where needed.
template <class DT>
struct FRow;
template <>
struct FRow<BF16T> {
  Op<BF16T, 4> op;
  // the raw row IS the packed operand: op.f[s] = {u[2s].x, u[2s].y, u[2s+1].x, u[2s+1].y}
  __device__ void set_raw(const RawRow<u16>& r) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      op.f[k] = __builtin_bit_cast(bf16x8, (uint4){r.u[2 * k].x, r.u[2 * k].y, r.u[2 * k + 1].x, r.u[2 * k + 1].y});
  }
  __device__ void act(Act<8>& a, const u16*, int) const { unpack_op(a, op); }
  __device__ const Op<BF16T, 4>& operand(const u16*, int) const { return op; }
};
template <>
struct FRow<F32T> {
  Op<F32T, 4> tmp;
  __device__ void act(Act<8>& a, const float* row, int g) const { load_row(a, row, g); }
  __device__ const Op<F32T, 4>& operand(const float* row, int g) {
    Act<8> a;
    load_row(a, row, g);
    make_op(tmp, a);
    return tmp;
  }
};

// Tiles of the attention fold (geot_edge.hip edge_attn_fold writes attn_parts, geot_node.hip attn_row
// adds them, di_attn_parts_bytes sizes them)
constexpr int FOLD_ROWS = 32;   // edges per tile of attn_parts (one wave's rows)
constexpr int FOLD_PART = 132;  // floats per partial: 128 wV, then z of the 4 heads

// ================================================================ host launch helpers
// grid / block of a launch, both from the kernel's geometry struct
template <class Geom>
static inline dim3 grid_of(int n) { return dim3((unsigned)((n + Geom::ROWS - 1) / Geom::ROWS)); }
template <class Geom>
static inline dim3 block_of() { return dim3(Geom::THREADS); }

// grid of a persistent launch (blocks walk the tiles): n rows in tiles of `rows`, one block per CU
// and never more blocks than tiles
struct PersistentGrid {
  int ntiles;
  dim3 grid;
};
static inline PersistentGrid persistent_grid(int n, int rows) {
  const int ntiles = (n + rows - 1) / rows;
  const int cus = device_cus();
  return {ntiles, dim3((unsigned)(ntiles < cus ? ntiles : cus))};
}

static inline int launch_status() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? DI_OK : (int)e;
}

static inline bool dtype_ok(di_dtype dt) { return dt == DI_BF16 || dt == DI_F32; }

}  // namespace di
