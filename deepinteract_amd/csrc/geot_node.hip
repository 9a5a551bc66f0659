// GeoT, node layer: the CSR attention aggregation, the node update on its weight ring, the
// weight-stationary bf16 node layer, the fused node layer, and their entry points (reference
// semantics: geot.h).
#include "geot.h"

namespace di {

// ================================================================ node aggregation (CSR segment sum)
// h_attn[v] = sum_{e in in(v)} alpha[e, head] * V[src e]  /  (sum_e alpha[e, head] + 1e-6)
// (send_and_recv(u_mul_e('V_h','score'), sum) and (copy_e('score'), sum), then wV / (z + 1e-6):
// deepinteract_modules.py:93-96, 116). Edges are destination-major (CSR in_ptr), so a node's
// in-edges are one contiguous range.
// 16 lanes per destination, 8 features (16 B of bf16) per lane: a gathered V row is one coalesced
// 256-B access. In-edges go in chunks of U: the chunk's source ids arrive with ONE coalesced load
// (lane j of the node's 16 reads src[e0 + j], broadcast by ds_bpermute) and the next chunk's ids are
// in flight while this chunk's alphas and V rows land, so a chunk costs one memory latency; U rows
// per lane in flight and 16 nodes per 256-thread block (grid = Nt / 16, several blocks per CU) hide
// it. The products are added one edge at a time in edge order with the same fused multiply-adds as
// the fused node kernels (fp32: k_node_layer's node_gather; bf16: k_node_ws's seg_sum16), so h_attn is
// bit-identical to what they compute internally.
constexpr int AGG_NODES = 16;  // destinations per block (16 lanes each)
template <class DT>
struct AggrCfg {
  static constexpr int U = DT::kBF16 ? 16 : 8;  // in-edges per chunk (V bytes in flight per lane: U x 16/32)
};

template <class DT>
__global__ __launch_bounds__(16 * AGG_NODES) void k_node_aggr(AggrArgs a) {
  using T = typename DT::T;
  constexpr int U = AggrCfg<DT>::U;
  constexpr int FPL = 8;  // features per lane
  const int j = threadIdx.x & 15;
  const int v = blockIdx.x * AGG_NODES + (threadIdx.x >> 4);
  if (v >= a.Nt) return;  // whole 16-lane groups exit together (shuffles stay within a group)
  const int head = (FPL * j) >> 5;
  const T* vbase = reinterpret_cast<const T*>(a.qkv) + 2 * HID + FPL * j;
  const int e0 = a.in_ptr[v], e1 = a.in_ptr[v + 1];
  float acc[FPL];
#pragma unroll
  for (int f = 0; f < FPL; ++f) acc[f] = 0.f;
  float z = 0.f;
  const int lane_base = threadIdx.x & 48;  // first lane of this node's 16 (within the wave)
  int id_next = e0 + j < e1 ? a.src[e0 + j] : 0;
#pragma unroll 1
  for (int c = e0; c < e1; c += U) {
    const int n = min(U, e1 - c);
    // this chunk's ids (lanes 0..n-1 of the group hold them) and alphas / V rows in flight
    const int id_cur = id_next;
    int ids[U];
#pragma unroll
    for (int u = 0; u < U; ++u) ids[u] = __shfl(id_cur, lane_base + (u & 15), 64);
    float al[U];
    T vv[U][FPL];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u < n) {
        al[u] = a.alpha[(int64_t)(c + u) * 4 + head];
        const T* row = vbase + (int64_t)ids[u] * 3 * HID;
        if constexpr (DT::kBF16) {
          *reinterpret_cast<uint4*>(vv[u]) = *reinterpret_cast<const uint4*>(row);
        } else {
          *reinterpret_cast<float4*>(vv[u]) = *reinterpret_cast<const float4*>(row);
          *reinterpret_cast<float4*>(vv[u] + 4) = *reinterpret_cast<const float4*>(row + 4);
        }
      }
    }
    // ids of the next chunk (U <= 16 lanes of the group)
    if (c + U < e1) id_next = c + U + j < e1 && j < U ? a.src[c + U + j] : 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u < n) {
#pragma unroll
        for (int f = 0; f < FPL; ++f) {
          float x;
          if constexpr (DT::kBF16) x = __builtin_bit_cast(float, (uint32_t)vv[u][f] << 16);
          else x = vv[u][f];
          acc[f] = __builtin_fmaf(al[u], x, acc[f]);
        }
        z += al[u];
      }
    }
  }
  const float d = z + 1e-6f;
  float4 o0, o1;
  o0.x = acc[0] / d; o0.y = acc[1] / d; o0.z = acc[2] / d; o0.w = acc[3] / d;
  o1.x = acc[4] / d; o1.y = acc[5] / d; o1.z = acc[6] / d; o1.w = acc[7] / d;
  float* out = a.attn + (int64_t)v * HID + FPL * j;
  *reinterpret_cast<float4*>(out) = o0;
  *reinterpret_cast<float4*>(out + 4) = o1;
}

// The attention row of node v from precomputed aggregates: di_node_aggregate's rows, or
// di_edge_layer_attn's (attn_parts != null): complete rows for destinations whose in-edges lie in
// one fold tile, partial sums for the others (edge_attn_fold), zero for a node without in-edges
// (wV / (z + 1e-6) = 0 there).
__device__ __forceinline__ void attn_row(Act<8>& wv, const NodeArgs& a, int v, int g) {
  if (a.attn_parts == nullptr) {
    load_row(wv, a.attn + (int64_t)v * HID, g);
    return;
  }
  const int e0 = a.in_ptr[v], e1 = a.in_ptr[v + 1];
  const int t0 = e0 / FOLD_ROWS, t1 = (e1 - 1) / FOLD_ROWS;
  if (e1 <= e0) {
    zero(wv);
  } else if (t0 == t1) {
    load_row(wv, a.attn + (int64_t)v * HID, g);
  } else {
    const float* p = a.attn_parts + ((int64_t)t0 * 2 + 1) * FOLD_PART;
    load_row(wv, p, g);
    floatx4 z = ld4(p + HID);
#pragma unroll 1
    for (int t = t0 + 1; t <= t1; ++t) {
      p = a.attn_parts + (int64_t)t * 2 * FOLD_PART;
      add_row(wv, p, g);
      z += ld4(p + HID);
    }
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const float d = z[b >> 1] + 1e-6f;
#pragma unroll
      for (int q = 0; q < 4; ++q) wv.v[b][q] = wv.v[b][q] / d;
    }
  }
}

// The CSR segment sum of one node held in the MFMA layout (wv[b][q] = feature 16b + 4g + q of node
// v): wV / (z + 1e-6) with wV = sum alpha * V[src], z = sum alpha over v's in-edges
// (deepinteract_modules.py:93-96, 116). The fp32 fused node layer's gather (k_node_layer with
// attn == NULL); k_node_aggr computes the same products in the same order.
__device__ __forceinline__ void node_gather(Act<8>& wv, const NodeArgs& a, int v, int g) {
  const float* qkv = reinterpret_cast<const float*>(a.qkv);
  zero(wv);
  floatx4 z = {0.f, 0.f, 0.f, 0.f};
  // In-edges in groups of UNR: the group's source ids, alphas and V[src] rows are all in flight
  // before the first product (one latency per group instead of two dependent ones per edge); the
  // products are still added one edge at a time in edge order (the reference's summation order).
  constexpr int UNR = 2;
  const int e0 = a.in_ptr[v], e1 = a.in_ptr[v + 1];
  int e = e0;
#pragma unroll 1
  for (; e + UNR <= e1; e += UNR) {
    int sid[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) sid[u] = a.src[e + u];
    floatx4 al[UNR];
    RawRow<float> vr[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      al[u] = ld4(a.alpha + (int64_t)(e + u) * 4);
      vr[u].load(qkv + (int64_t)sid[u] * 3 * HID + 2 * HID, g);
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      Act<8> vv;
      vr[u].to_act(vv);
#pragma unroll
      for (int b = 0; b < 8; ++b) wv.v[b] = __builtin_elementwise_fma((floatx4)al[u][b >> 1], vv.v[b], wv.v[b]);
      z += al[u];
    }
  }
#pragma unroll 1
  for (; e < e1; ++e) {
    const floatx4 al = ld4(a.alpha + (int64_t)e * 4);
    Act<8> vv;
    load_row(vv, qkv + (int64_t)a.src[e] * 3 * HID + 2 * HID, g);
#pragma unroll
    for (int b = 0; b < 8; ++b) wv.v[b] = __builtin_elementwise_fma((floatx4)al[b >> 1], vv.v[b], wv.v[b]);
    z += al;
  }
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const float d = z[b >> 1] + 1e-6f;
#pragma unroll
    for (int q = 0; q < 4; ++q) wv.v[b][q] = wv.v[b][q] / d;
  }
}

// ================================================================ node update (bf16), 4-slot weight ring
// O_node + residual + FFN (+ next layer's Q/K/V, + hT) from the aggregated rows of k_node_aggr.
// Nt / 64 blocks is one block per CU, so a stage's 32 MFMAs per wave (~0.3 us) are far shorter than
// an LDS-DMA stage's landing latency (~1 us): a double-buffered WPipe would wait on
// every stage. Here ALL the layer's biases land once at entry and the 32-KiB stages stream through
// a 4-slot ring, three stages ahead: entering stage s the wave waits only for its own pieces of
// stage s (s_waitcnt vmcnt(8 x stages issued after it): each wave issues exactly 8 one-KiB pieces
// per stage, and every other vector-memory operation is older than them: outputs are held in
// registers and stored at the end), then a barrier publishes the stage and frees the slot of
// stage s-1 for stage s+3. With k_node_aggr's rows it is bit-identical to k_node_ws
// (tests/test_gpu_node_aggr.py).
constexpr int NU_SLOTS = 4;
constexpr int NU_STAGE = MAT128;  // blocks per stage
__device__ __forceinline__ void nu_wait_younger(int n_stages_younger) {
  // vmcnt takes an immediate: the three counts this ring can need
  if (n_stages_younger >= 2) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  else if (n_stages_younger == 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// each of the 4 waves issues exactly NU_STAGE * BLK * 2 / 1024 / 4 = 8 one-KiB pieces per stage:
// the vmcnt immediates of nu_wait_younger assume that split
using NodeRingGeo = KernelGeo<4>;
static_assert(NU_STAGE * BLK * 2 / 1024 / NodeRingGeo::NW == 8, "nu_wait_younger counts 8 pieces per wave");
template <bool FINAL>
__global__ __launch_bounds__(NodeRingGeo::THREADS, 1) void k_node_update_ring(NodeArgs a) {
  constexpr int NS = FINAL ? 5 : 8;
  constexpr int NVEC = FINAL ? NLV_N_FINAL : NLV_N;
  // one LDS object: [4 ring slots | all biases]
  __shared__ __attribute__((aligned(16))) char lds[NU_SLOTS * NU_STAGE * BLK * 2 + NLV_N * 4];
  u16* wring = reinterpret_cast<u16*>(lds);
  float* vlds = reinterpret_cast<float*>(lds + NU_SLOTS * NU_STAGE * BLK * 2);
  const int lane = lane_id(), g = lane >> 4;
  const int r = row_id<NodeRingGeo::NW>();
  const bool valid = r < a.Nt;
  const int v = valid ? r : a.Nt - 1;
  const u16* W = reinterpret_cast<const u16*>(a.wmat);
  // stage s -> first packed block
  auto stage_blk = [](int s) {
    return s == 0 ? NL_ON : (s == 1 ? NL_F1 : (s == 2 ? NL_F2 : (s == 3 ? NL_F1 + MAT128 : (s == 4 ? NL_F2 + MAT128 : NL_Q + MAT128 * (s - 5)))));
  };
  auto issue = [&](int s) { dma_blocks<NodeRingGeo::NW>(wring + (s % NU_SLOTS) * NU_STAGE * BLK, W + stage_blk(s) * BLK, NU_STAGE); };
  // biases and stage 0, then this node's rows, landed here (the compiler cannot count the DMA
  // loops, so a row used later would make it wait for every stage in flight), then stages 1-2
  dma_vec<NodeRingGeo::NW>(vlds, a.wvec, NVEC / 128);
  issue(0);
  RawRow<u16> hin;
  hin.load(reinterpret_cast<const u16*>(a.h_in) + (int64_t)v * HID, g);
  Act<8> wv;
  attn_row(wv, a, v, g);
  settle(hin);
#pragma unroll
  for (int b = 0; b < 8; ++b) asm volatile("" ::"v"(wv.v[b]));
  issue(1);
  issue(2);
  auto enter = [&](int s) -> const u16* {
    nu_wait_younger(min(2, NS - 1 - s));
    // a bare s_barrier: __syncthreads()' workgroup fence would wait for every outstanding
    // vector-memory operation, i.e. also for the stages in flight behind this one
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (s + 3 < NS) issue(s + 3);
    return wring + (s % NU_SLOTS) * NU_STAGE * BLK;
  };
  // n = in1 + O_node(h)
  const u16* w = enter(0);
  Act<8> n;
  init_vec_lds(n, vlds + NLV_ON, g);
  {
    Act<8> hv;
    hin.to_act(hv);
    add_(n, hv);
  }
  linear<BF16T, 8, 4>(n, wv, w, lane);
  // n = n + W2 silu(W1 BN2(n))
  Act<8> o;
  zero(o);
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    w = enter(1 + 2 * half);
    Act<8> t;
    init_vec_lds(t, vlds + NLV_F1 + 128 * half, g);
    linear<BF16T, 8, 4>(t, n, w, lane);
    silu2_<8, true>(t);
    w = enter(2 + 2 * half);
    linear<BF16T, 8, 4>(o, t, w, lane);
  }
  add_(n, o);
  if constexpr (FINAL) {
    if (valid) store_row(n, reinterpret_cast<u16*>(a.h_out) + (int64_t)v * HID, g);
    if (a.hT_out != nullptr && valid) {
      u16* hT = reinterpret_cast<u16*>(a.hT_out);
#pragma unroll
      for (int b = 0; b < 8; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          hT[(int64_t)(16 * b + 4 * g + q) * a.Nt + v] = (u16)(pack_bf16x2(n.v[b][q], 0.f) & 0xffffu);
    }
  } else {
    Op<BF16T, 4> nop;
    make_op(nop, n);  // bf16 bits of n: the h_out row and the Q/K/V operand
    Op<BF16T, 4> qkv_rows[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      w = enter(5 + q);
      Act<8> t;
      init_vec_lds(t, vlds + NLV_Q + 128 * q, g);
      mma<8, 4>(t, nop, w, lane);
      make_op(qkv_rows[q], t);
    }
    if (valid) {
      // packed operand -> row-major bf16: f[s] = {blk 2s regs 0-3, blk 2s+1 regs 0-3} = 4+4 features
      auto store_op = [&](const Op<BF16T, 4>& op, u16* row) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const uint4 u = __builtin_bit_cast(uint4, op.f[s]);
          *reinterpret_cast<uint2*>(row + 16 * (2 * s) + 4 * g) = (uint2){u.x, u.y};
          *reinterpret_cast<uint2*>(row + 16 * (2 * s + 1) + 4 * g) = (uint2){u.z, u.w};
        }
      };
      store_op(nop, reinterpret_cast<u16*>(a.h_out) + (int64_t)v * HID);
      u16* qo = reinterpret_cast<u16*>(a.qkv_out) + (int64_t)v * 3 * HID;
#pragma unroll
      for (int q = 0; q < 3; ++q) store_op(qkv_rows[q], qo + q * HID);
    }
  }
}

// The CSR segment sum of ONE destination by its 16-lane group (lane j: features 8j .. 8j + 7, head
// j / 4): acc = sum_e alpha[e, head] * V[src e], z = sum_e alpha[e, head] over e in [e0, e1), edge by
// edge in order -- k_node_aggr's products and order, so the row is bit-identical to it for any chunk
// size U. Every product is added with an explicit fused multiply-add (here, in k_node_aggr and in
// node_gather): a plain a += w * x is llvm.fmuladd, which the backend may fuse in one kernel and split
// into a multiply and an add in another (round 6: a build with specialised aggregation waves differed
// from the split form by one bf16 ulp on 1 row in 96 until its sums were explicit FMAs). Every load of a chunk is issued unconditionally (a slot past e1 re-reads edge c's alpha and
// a valid V row and adds it with weight 0, which is exact), so a chunk is one batch of buffer loads
// (32-bit offsets from SGPR descriptors) and one wait, with no per-edge branch. A chunk's source ids
// arrive as two per-lane registers (lane j of the group: src[c + j] and src[c + 16 + j], 0 past e1),
// loaded one chunk ahead; on entry (ida, idb) hold chunk e0's.
template <int U>
__device__ __forceinline__ void seg_ids(const int* __restrict__ src, int c, int e1, int j, int& ida, int& idb) {
  ida = c + j < e1 && j < U ? src[c + j] : 0;
  if constexpr (U > 16) idb = c + 16 + j < e1 && 16 + j < U ? src[c + 16 + j] : 0;
}
template <int U>
__device__ __forceinline__ void seg_sum16(__amdgpu_buffer_rsrc_t vr, __amdgpu_buffer_rsrc_t ar, const int* __restrict__ src,
                                          int e0, int e1, int j, int lane_base, int ida, int idb, float (&acc)[8],
                                          float& z) {
  static_assert(U >= 1 && U <= 32, "a chunk's ids come from two registers of the group's 16 lanes");
  const int head = j >> 2;
#pragma unroll 1
  for (int c = e0; c < e1; c += U) {
    const int n = min(U, e1 - c);
    const int id_a = ida, id_b = idb;
    float al[U];
    uint4 vv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int id = __shfl(u < 16 ? id_a : id_b, lane_base + (u & 15), 64);
      const int eu = u < n ? c + u : c;
      al[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ar, (eu * 4 + head) * 4, 0, 0));
      vv[u] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(vr, id * (3 * HID * 2) + 16 * j, 0, 0));
    }
    if (c + U < e1) seg_ids<U>(src, c + U, e1, j, ida, idb);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float w = u < n ? al[u] : 0.f;
      const uint32_t x[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
#pragma unroll
      for (int f = 0; f < 8; ++f) {
        const uint32_t b = f & 1 ? (x[f >> 1] & 0xffff0000u) : (x[f >> 1] << 16);
        acc[f] = __builtin_fmaf(w, __builtin_bit_cast(float, b), acc[f]);
      }
      z += w;
    }
  }
}

// k_node_ws: chunks of 10 (k = 20 in-edges are two chunks). One chunk of 20 (one memory latency per
// tile) spills 5 VGPRs at the 240 cap and measured slower: node layers beside the pair stream
// 47 / 27-29 vs 43 / 26-29 us, 7953 / 7918 vs 8038 / 7993 complexes/s (round 6,
// tools/sessions/r6_05_wsu.sh)
constexpr int SEG_U_WS = 10;
// LDS row strides of the node kernels' exchange buffers, padded for the banking of the instructions
// that touch them (MI355X_MICROARCH.md §LDS): the fp32 aggregated rows are read by ds_read_b128 (four
// 16-lane groups, bank = word mod 64) -- a 136-word stride puts every group's 16 lanes (rows r, lane
// groups g) on distinct bank quads; the bf16 operand rows are read by ds_read2_b64 and written by
// ds_write_b64 (16 contiguous lanes per access, bank = word mod 32, 2 words per lane) -- 66 / 130-word
// strides put 16 rows on 32 distinct banks. Unpadded (128 / 64 / 128 words) every row starts on bank
// 0: 16-way conflicts on each exchange access (round 6, first k_node_ws build: 2x slower).
constexpr int LDS_ATTN = HID + 8;       // fp32 aggregated rows: 136 words
constexpr int LDS_N = HID + 4;          // bf16 n / h rows: 66 words
constexpr int LDS_T = 2 * HID + 4;      // bf16 FFN-hidden rows: 130 words

// ================================================================ node layer, weights stationary (bf16)
// The bf16 di_node_layer since round 6. Round 5's kernel (deleted) streamed the whole
// layer's weights (256 KiB) from L2 into every 16-destination block: 1000 blocks, 256 MB of L2 -> CU
// fragment traffic per C3 micro-batch, each wave's chain waiting on its fragment loads, beside a pair
// stream that pushes ~4 TB/s of stores through the same L2s. Here the weights are loaded ONCE per CU
// and stay:
//   * one persistent 8-wave block per CU (two waves per SIMD) walks tiles of 32 destinations
//     (XCD-contiguous tile order, as the edge ring);
//   * wave w keeps its slice of O (output block w), the FFN hidden layer (blocks 2w, 2w+1 of 16) and
//     the FFN output (block w, both K halves) in registers for the whole launch (80 VGPRs), and the
//     next layer's Q|K|V (96 KiB) sits in LDS, DMA'd once at entry (wave w: blocks 3w..3w+2 of 24);
//   * per tile: (1) the CSR segment sum, 16 lanes per destination (seg_sum16: k_node_aggr's products
//     in k_node_aggr's order and its division: bit-identical rows) into LDS -- 32 destinations x 16
//     lanes = the block;
//     (2) O_node + residual, FFN, Q|K|V as two 16-destination MFMA column groups, every register
//     fragment feeding both groups, activations exchanged through LDS as bf16 operands.
// Per output element the arithmetic is that of k_node_aggr + k_node_update_ring (the same bias +
// residual initial value, the same k-steps in the same order, the same bf16 operands): h / Q,K,V / hT
// are bit-identical to the split pair (tests/test_gpu_node_aggr.py::
// test_node_layer_ragged_csr_matches_split).
constexpr int NWS_NW = 8;        // waves per block
constexpr int NWS_TILE = 32;     // destinations per tile (2 MFMA column groups of 16)
static_assert(NWS_TILE * 16 == 64 * NWS_NW, "16 aggregation lanes per destination of a tile");
// <= 240 VGPRs (amdgpu_num_vgpr counts register pairs): two waves per SIMD leave a pair-stream wave
// (32 VGPRs) room beside them, as the edge ring
template <bool FINAL>
__global__ __attribute__((amdgpu_flat_work_group_size(1, 64 * NWS_NW), amdgpu_waves_per_eu(2, 2),
                          amdgpu_num_vgpr(120)))
void k_node_ws(NodeArgs a, int ntiles) {
  constexpr int NG = NWS_TILE / 16;
  __shared__ __attribute__((aligned(16))) float s_attn[NWS_TILE * LDS_ATTN];  // aggregated rows (fp32), 16 KiB
  __shared__ __attribute__((aligned(16))) u16 s_n[NWS_TILE * LDS_N];       // n / new h as a bf16 operand, 8 KiB
  __shared__ __attribute__((aligned(16))) u16 s_t[NWS_TILE * LDS_T];   // FFN hidden (bf16), 16 KiB
  __shared__ __attribute__((aligned(16))) u16 s_q[FINAL ? 8 : 3 * MAT128 * BLK];  // Q|K|V weights, 96 KiB
  const int lane = lane_id(), g = lane >> 4, r = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const u16* W = reinterpret_cast<const u16*>(a.wmat);
  const float* V = a.wvec;
  if constexpr (!FINAL) dma_blocks<NWS_NW>(s_q, W + NL_Q * BLK, 3 * MAT128);
  // this wave's register-resident weights (A fragments: output block bo, k-step s of a 128x128 matrix)
  auto frag = [&](int m, int bo, int s) {
    return *reinterpret_cast<const bf16x8*>(W + (m + bo * 4 + s) * BLK + lane * 8);
  };
  bf16x8 fo[4], f1[2][4], f2[2][4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    fo[s] = frag(NL_ON, w, s);
#pragma unroll
    for (int b = 0; b < 2; ++b) f1[b][s] = frag(NL_F1 + MAT128 * ((2 * w + b) >> 3), (2 * w + b) & 7, s);
#pragma unroll
    for (int h = 0; h < 2; ++h) f2[h][s] = frag(NL_F2 + MAT128 * h, w, s);
  }
  auto lds_op = [&](const u16* rows, int stride, int q, int f0) {
    Op<BF16T, 4> o;
    const u16* row = rows + (q * 16 + r) * stride + f0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const uint2 lo = *reinterpret_cast<const uint2*>(row + 32 * s + 4 * g);
      const uint2 hi = *reinterpret_cast<const uint2*>(row + 32 * s + 16 + 4 * g);
      o.f[s] = __builtin_bit_cast(bf16x8, (uint4){lo.x, lo.y, hi.x, hi.y});
    }
    return o;
  };
  auto put_slice = [&](u16* rows, int stride, int q, int f, floatx4 x) {
    *reinterpret_cast<uint2*>(rows + (q * 16 + r) * stride + f + 4 * g) =
        (uint2){pack_bf16x2(x[0], x[1]), pack_bf16x2(x[2], x[3])};
  };
  bool qkv_landed = FINAL;
  const int j = threadIdx.x & 15, nl = threadIdx.x >> 4;  // aggregation: destination nl of the tile, lane j
  auto tile_of = [&](int i) { return (gridDim.x & 7) == 0 ? xcd_slot(i, ntiles) : i; };
  // this lane's CSR range and first source id of a tile's destination (issued a tile ahead)
  int e0 = 0, e1 = 0, ida = 0, idb = 0;
  auto seg_head = [&](int i) {
    const int v = tile_of(i) * NWS_TILE + nl;
    e0 = e1 = 0;
    if (i < ntiles && v < a.Nt) {
      e0 = a.in_ptr[v];
      e1 = a.in_ptr[v + 1];
    }
  };
  auto seg_id0 = [&]() { seg_ids<SEG_U_WS>(a.src, e0, e1, j, ida, idb); };
  seg_head((int)blockIdx.x);
  seg_id0();
#pragma unroll 1
  for (int i = (int)blockIdx.x; i < ntiles; i += (int)gridDim.x) {
    const int vb = tile_of(i) * NWS_TILE;
    // ---- 1. wV / (z + 1e-6), 16 lanes per destination (k_node_aggr's sums)
    {
      constexpr int FPL = 8;
      float acc[FPL];
#pragma unroll
      for (int f = 0; f < FPL; ++f) acc[f] = 0.f;
      float z = 0.f;
      // empty past Nt (e0 == e1): the shuffles stay inside the 16-lane group
      seg_sum16<SEG_U_WS>(buf_rsrc(reinterpret_cast<const u16*>(a.qkv) + 2 * HID), buf_rsrc(a.alpha), a.src, e0, e1, j,
                          threadIdx.x & 48, ida, idb, acc, z);
      seg_head(i + (int)gridDim.x);  // the next tile's CSR range, in flight under this tile's update
      const float d = z + 1e-6f;
      float* out = s_attn + nl * LDS_ATTN + FPL * j;
      st4(out, (floatx4){acc[0] / d, acc[1] / d, acc[2] / d, acc[3] / d});
      st4(out + 4, (floatx4){acc[4] / d, acc[5] / d, acc[6] / d, acc[7] / d});
    }
    // ---- 2. the update: wave w's output blocks for both column groups
    int vq[NG];
    bool valid[NG];
    Act<1> n[NG];
#pragma unroll
    for (int q = 0; q < NG; ++q) {
      vq[q] = vb + q * 16 + r;
      valid[q] = vq[q] < a.Nt;
      const int vc = valid[q] ? vq[q] : a.Nt - 1;
      n[q].v[0] = ld4(V + NLV_ON + 16 * w + 4 * g) + ld4(reinterpret_cast<const u16*>(a.h_in) + (int64_t)vc * HID + 16 * w + 4 * g);
    }
    __syncthreads();  // the aggregated rows (and, tile > 0, every wave past the previous tile's reads)
    // n = b_O + h_in + O(attn)
#pragma unroll
    for (int q = 0; q < NG; ++q) {
      Act<8> wv;
#pragma unroll
      for (int b = 0; b < 8; ++b)
        wv.v[b] = *reinterpret_cast<const floatx4*>(s_attn + (q * 16 + r) * LDS_ATTN + 16 * b + 4 * g);
      Op<BF16T, 4> op;
      make_op(op, wv);
#pragma unroll
      for (int s = 0; s < 4; ++s) n[q].v[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fo[s], op.f[s], n[q].v[0], 0, 0, 0);
      put_slice(s_n, LDS_N, q, 16 * w, n[q].v[0]);
    }
    floatx4 b1[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) b1[b] = ld4(V + NLV_F1 + 16 * (2 * w + b) + 4 * g);
    seg_id0();  // the next tile's first source ids
    __syncthreads();  // n, all 128 features of both groups
    // FFN hidden: blocks 2w, 2w + 1 of the 16
#pragma unroll
    for (int q = 0; q < NG; ++q) {
      const Op<BF16T, 4> nop = lds_op(s_n, LDS_N, q, 0);
      Act<2> tq;
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        tq.v[b] = b1[b];
#pragma unroll
        for (int s = 0; s < 4; ++s) tq.v[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f1[b][s], nop.f[s], tq.v[b], 0, 0, 0);
      }
      silu2_<2, true>(tq);
#pragma unroll
      for (int b = 0; b < 2; ++b) put_slice(s_t, LDS_T, q, 16 * (2 * w + b), tq.v[b]);
    }
    __syncthreads();  // the hidden layer, all 256 features (and every wave is past its n operands)
    // FFN output block w: both hidden halves in order, as k_node_update_ring
#pragma unroll
    for (int q = 0; q < NG; ++q) {
      Act<1> o;
      zero(o);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const Op<BF16T, 4> top = lds_op(s_t, LDS_T, q, HID * h);
#pragma unroll
        for (int s = 0; s < 4; ++s) o.v[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f2[h][s], top.f[s], o.v[0], 0, 0, 0);
      }
      add_(n[q], o);
      if (valid[q]) st4(reinterpret_cast<u16*>(a.h_out) + (int64_t)vq[q] * HID + 16 * w + 4 * g, n[q].v[0]);
      if constexpr (FINAL) {
        if (a.hT_out != nullptr && valid[q]) {
          u16* hT = reinterpret_cast<u16*>(a.hT_out);
#pragma unroll
          for (int k = 0; k < 4; ++k)
            hT[(int64_t)(16 * w + 4 * g + k) * a.Nt + vq[q]] = (u16)(pack_bf16x2(n[q].v[0][k], 0.f) & 0xffffu);
        }
      } else {
        put_slice(s_n, LDS_N, q, 16 * w, n[q].v[0]);
      }
    }
    if constexpr (!FINAL) {
      floatx4 bq[3];
#pragma unroll
      for (int b = 0; b < 3; ++b) bq[b] = ld4(V + NLV_Q + 16 * (3 * w + b) + 4 * g);
      if (!qkv_landed) {  // first tile only: this wave's pieces of the Q|K|V weights, before the barrier
        lds_dma_wait();
        qkv_landed = true;
      }
      __syncthreads();  // the new h, all 128 features (s_n's previous readers finished before the last barrier)
      // next layer's Q | K | V: blocks 3w .. 3w + 2 of the 24 (Q 0-7, K 8-15, V 16-23)
      bf16x8 fq[3][4];
#pragma unroll
      for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int ob = 3 * w + b;
          fq[b][s] = *reinterpret_cast<const bf16x8*>(s_q + (MAT128 * (ob >> 3) + (ob & 7) * 4 + s) * BLK + lane * 8);
        }
#pragma unroll
      for (int q = 0; q < NG; ++q) {
        const Op<BF16T, 4> hop = lds_op(s_n, LDS_N, q, 0);
        u16* qo = reinterpret_cast<u16*>(a.qkv_out) + (int64_t)vq[q] * 3 * HID;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          floatx4 x = bq[b];
#pragma unroll
          for (int s = 0; s < 4; ++s) x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fq[b][s], hop.f[s], x, 0, 0, 0);
          if (valid[q]) st4(qo + 16 * (3 * w + b) + 4 * g, x);
        }
      }
    }
  }
}

// ================================================================ fused node layer (fp32)
// The fp32 di_node_layer and di_node_update (the reference's precision; bf16: k_node_ws,
// k_node_update_ring): each 64-KiB stage is DMA'd synchronously into ONE slot (pipe.next() issues
// the stage, waits and publishes it). Every bias vector rides in its stage's slot (init_vec_lds),
// and the node's own input row is loaded before the first stage and settled right after it, so no
// later stage wait stands between the load and its use.
// Launch geometry of k_node_layer: DI_NODE_NW waves (16 nodes each) per block. Round 2's 2-wave
// build faulted (code 719) because di_node_update's fp32 launch kept a hard-coded 256-thread block
// while the kernel had been compiled for 128 (__launch_bounds__(64 * 2)): every launch site now
// takes its shape from NodeGeo. 4 waves is the default; the 2-wave build of the fp32 node layer is
// a tested variant (tools/build_variants.py "node2").
#ifndef DI_NODE_NW
#define DI_NODE_NW 4
#endif
using NodeGeo = KernelGeo<DI_NODE_NW>;
template <bool FINAL>
__global__ __launch_bounds__(NodeGeo::THREADS, 2) void k_node_layer(NodeArgs a) {
  using Pipe = WPipe<float, NodeGeo::NW, false, MAT128, 128>;
  __shared__ __attribute__((aligned(16))) char lds[Pipe::SLOT_BYTES];
  const int lane = lane_id(), g = lane >> 4;
  const int r = row_id<NodeGeo::NW>();
  const bool valid = r < a.Nt;
  const int v = valid ? r : a.Nt - 1;
  const float* W = reinterpret_cast<const float*>(a.wmat);
  const float* V = a.wvec;
  Pipe pipe(lds);
  pipe.issue(W + NL_ON * BLK, MAT128, V + NLV_ON, 128);
  RawRow<float> hin;  // in1 of the residual, consumed after the O stage barrier
  hin.load(reinterpret_cast<const float*>(a.h_in) + (int64_t)v * HID, g);

  // send_and_recv(u_mul_e('V_h','score'), sum) and (copy_e('score'), sum); h = wV / (z + 1e-6)
  Act<8> wv;
  if (a.attn != nullptr) attn_row(wv, a, v, g);  // k_node_aggr (same products, order, division) or the fold
  else node_gather(wv, a, v, g);
  // n = in1 + O_node(h)
  const float* w = pipe.next();
  settle(hin);  // landed with the O stage (its wait drained vmcnt)
  pipe.issue(W + NL_F1 * BLK, MAT128, V + NLV_F1, 128);
  Act<8> n;
  init_vec_lds(n, pipe.v(), g);
  {
    Act<8> hv;
    hin.to_act(hv);
    add_(n, hv);
  }
  linear<F32T, 8, 4>(n, wv, w, lane);
  // n = n + W2 silu(W1 BN2(n))
  Act<8> o;
  zero(o);
#pragma unroll 1
  for (int half = 0; half < 2; ++half) {
    w = pipe.next();
    pipe.issue(W + (NL_F2 + MAT128 * half) * BLK, MAT128);
    Act<8> t;
    init_vec_lds(t, pipe.v(), g);
    linear<F32T, 8, 4>(t, n, w, lane);
    silu_<8, false>(t);
    w = pipe.next();
    if (half == 0) pipe.issue(W + (NL_F1 + MAT128) * BLK, MAT128, V + NLV_F1 + 128, 128);
    else if (!FINAL) pipe.issue(W + NL_Q * BLK, MAT128, V + NLV_Q, 128);
    linear<F32T, 8, 4>(o, t, w, lane);
  }
  add_(n, o);
  if (valid) store_row(n, reinterpret_cast<float*>(a.h_out) + (int64_t)v * HID, g);
  if (a.hT_out != nullptr && valid) {  // 16 lanes (nodes) store 64 contiguous bytes per feature
    float* hT = reinterpret_cast<float*>(a.hT_out);
#pragma unroll
    for (int b = 0; b < 8; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) hT[(int64_t)(16 * b + 4 * g + q) * a.Nt + v] = n.v[b][q];
  }
  if constexpr (!FINAL) {
    float* qo = reinterpret_cast<float*>(a.qkv_out);
#pragma unroll 1
    for (int q = 0; q < 3; ++q) {
      w = pipe.next();
      if (q < 2) pipe.issue(W + (NL_Q + MAT128 * (q + 1)) * BLK, MAT128, V + NLV_Q + 128 * (q + 1), 128);
      Act<8> t;
      init_vec_lds(t, pipe.v(), g);
      linear<F32T, 8, 4>(t, n, w, lane);
      if (valid) store_row(t, qo + (int64_t)v * 3 * HID + q * HID, g);
    }
  }
}

}  // namespace di

// ================================================================ C ABI
using namespace di;

extern "C" int di_node_layer(const di_graph* g, di_dtype dt, int final_layer, const float* alpha,
                             const void* h_in, const void* qkv, const void* wmat, const float* wvec,
                             void* h_out, void* qkv_out, void* hT_out, void* stream) {
  if (!g || !alpha || !h_in || !qkv || !wmat || !wvec || !h_out || g->num_nodes <= 0 || !dtype_ok(dt))
    return DI_EINVAL;
  if (!final_layer && !qkv_out) return DI_EINVAL;
  NodeArgs a{g->num_nodes, nullptr, hT_out, g->src, g->in_ptr, alpha, h_in, qkv, wmat, wvec, h_out, qkv_out};
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid = grid_of<NodeGeo>(a.Nt), block = block_of<NodeGeo>();
  if (dt == DI_BF16) {
    // persistent weight-stationary blocks, one per CU, 32-destination tiles (k_node_ws)
    if (!g->src || !g->in_ptr) return DI_EINVAL;
    // the segment sums address V rows and alphas by 32-bit buffer offsets
    if ((int64_t)a.Nt * 3 * HID * 2 >= (1LL << 31) || (int64_t)g->num_edges * 16 >= (1LL << 31)) return DI_ERANGE;
    const PersistentGrid p = persistent_grid(a.Nt, NWS_TILE);
    const dim3 bw(64 * NWS_NW);
    if (final_layer) hipLaunchKernelGGL((k_node_ws<true>), p.grid, bw, 0, s, a, p.ntiles);
    else hipLaunchKernelGGL((k_node_ws<false>), p.grid, bw, 0, s, a, p.ntiles);
  } else {
    if (final_layer) hipLaunchKernelGGL((k_node_layer<true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_node_layer<false>), grid, block, 0, s, a);
  }
  return launch_status();
}

extern "C" int di_node_aggregate(const di_graph* g, di_dtype dt, const float* alpha, const void* qkv, float* attn_out,
                                 void* stream) {
  if (!g || !alpha || !qkv || !attn_out || !g->src || !g->in_ptr || g->num_nodes <= 0 || !dtype_ok(dt))
    return DI_EINVAL;
  AggrArgs a{g->num_nodes, g->src, g->in_ptr, alpha, qkv, attn_out};
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((a.Nt + AGG_NODES - 1) / AGG_NODES)), block(16 * AGG_NODES);
  if (dt == DI_BF16) hipLaunchKernelGGL(k_node_aggr<BF16T>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(k_node_aggr<F32T>, grid, block, 0, s, a);
  return launch_status();
}

static int node_update(const di_graph* g, di_dtype dt, int final_layer, const float* attn, const float* attn_parts,
                       const void* h_in, const void* wmat, const float* wvec, void* h_out, void* qkv_out, void* hT_out,
                       void* stream) {
  if (!g || !attn || !h_in || !wmat || !wvec || !h_out || g->num_nodes <= 0 || !dtype_ok(dt)) return DI_EINVAL;
  if (!final_layer && !qkv_out) return DI_EINVAL;
  if (attn_parts && !g->in_ptr) return DI_EINVAL;
  NodeArgs a{g->num_nodes, attn, hT_out, nullptr, attn_parts ? g->in_ptr : nullptr, nullptr, h_in, nullptr, wmat,
             wvec, h_out, qkv_out, attn_parts};
  hipStream_t s = (hipStream_t)stream;
  if (dt == DI_BF16) {
    const dim3 grid = grid_of<NodeRingGeo>(a.Nt), block = block_of<NodeRingGeo>();
    if (final_layer) hipLaunchKernelGGL((k_node_update_ring<true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_node_update_ring<false>), grid, block, 0, s, a);
  } else {
    const dim3 grid = grid_of<NodeGeo>(a.Nt), block = block_of<NodeGeo>();
    if (final_layer) hipLaunchKernelGGL((k_node_layer<true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_node_layer<false>), grid, block, 0, s, a);
  }
  return launch_status();
}

extern "C" int di_node_update(const di_graph* g, di_dtype dt, int final_layer, const float* attn, const void* h_in,
                              const void* wmat, const float* wvec, void* h_out, void* qkv_out, void* hT_out,
                              void* stream) {
  return node_update(g, dt, final_layer, attn, nullptr, h_in, wmat, wvec, h_out, qkv_out, hT_out, stream);
}

extern "C" int di_node_update_folded(const di_graph* g, di_dtype dt, int final_layer, const float* attn,
                                     const float* attn_parts, const void* h_in, const void* wmat, const float* wvec,
                                     void* h_out, void* qkv_out, void* hT_out, void* stream) {
  if (!attn_parts) return DI_EINVAL;
  return node_update(g, dt, final_layer, attn, attn_parts, h_in, wmat, wvec, h_out, qkv_out, hT_out, stream);
}
