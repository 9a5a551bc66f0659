// GeoT, embedding and InitEdge stage: the node embedding (+ layer-0 Q/K/V), InitEdgeModule on 16x16
// and 32x32 MFMA, its LDS-resident form, and their entry points (reference semantics: geot.h).
#include "geot.h"
#include "mfma32.h"
#include "pair_queue.h"

namespace di {

// ================================================================ node embedding (+ Q/K/V of layer 0)
using EmbedGeo = KernelGeo<4>;
template <class DT>
__global__ __launch_bounds__(EmbedGeo::THREADS) void k_node_embed(EmbedArgs a) {
  pq_signal_at_start(a.sig_q, a.sig_job);
  using T = typename DT::T;
  __shared__ __attribute__((aligned(16))) T lds[2 * MAT128 * BLK];
  const int lane = lane_id(), g = lane >> 4;
  const int r = row_id<EmbedGeo::NW>();
  const bool valid = r < a.Nt;
  const int v = valid ? r : a.Nt - 1;
  const T* W = reinterpret_cast<const T*>(a.wmat);
  WPipe<T, EmbedGeo::NW, true, MAT128> pipe(lds);
  pipe.issue(W + EM_EMB * BLK, MAT128);

  Act<8> x;  // in_dim (113 raw DIPS-Plus + geometric features) input columns, zero padded to 128
  const float* row = a.node_f + (int64_t)v * a.in_dim;
#pragma unroll
  for (int b = 0; b < 8; ++b)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int f = 16 * b + 4 * g + q;
      x.v[b][q] = f < a.in_dim ? row[f] : 0.f;
    }
  const T* w = pipe.next();
  pipe.issue(W + EM_Q * BLK, MAT128);
  Act<8> h;
  zero(h);
  linear<DT, 8, 4>(h, x, w, lane);
  if (valid) store_row(h, reinterpret_cast<T*>(a.h_out) + (int64_t)v * HID, g);
  T* qkv = reinterpret_cast<T*>(a.qkv_out);
#pragma unroll 1
  for (int q = 0; q < 3; ++q) {
    w = pipe.next();
    if (q < 2) pipe.issue(W + (EM_Q + MAT128 * (q + 1)) * BLK, MAT128);
    Act<8> t;
    init_vec(t, a.wvec + EMV_Q + 128 * q, g);
    linear<DT, 8, 4>(t, h, w, lane);
    if (valid) store_row(t, qkv + (int64_t)v * 3 * HID + q * HID, g);
  }
}

// ================================================================ InitEdgeModule (+ layer-0 nbr_linear)
// GC (DI_GRAPH_GEO_REF batches): the direction terms silu(dir_linear_{0,1}(0)) = 0 are skipped and
// the orientation terms are the packed constants IEV_ORC / IEV_OGATE; the layer-0
// silu(nbr_linear(F)) rows are only computed when fn_out is given (the grouped edge kernel does
// not gather them for such batches).
// Both InitEdge kernels (k_init_edge: fp32 on 16x16 MFMA, k_init_x32: bf16 on 32x32) stage their
// weights synchronously through ONE slot of INIT_CAP blocks per block, so several blocks share a CU
// and cover each other's stage waits (measured shapes: DESIGN.md §8).
constexpr int INIT_CAP = 40;  // blocks of the weight-stage slot (the largest phase: a geometric term)
// k_init_edge's launch geometry: 4-wave blocks of 64 edges, two per CU (an 80-KiB fp32 slot each)
struct InitGeo : KernelGeo<4> {
  static constexpr int WPE = 2;  // blocks (waves per SIMD) per CU
};
// The node embedding (+ layer-0 Q/K/V) as the first `embed_blocks` blocks of an InitEdge launch
// (di_embed_init_edge): same stages and arithmetic as k_node_embed<DT> through InitEdge's single
// 40-block LDS slot, so the two run side by side inside one launch instead of the embedding on a
// side stream (whose blocks find no LDS beside InitEdge's until its tail). Instantiated for both
// hosts: <F32T, InitGeo::NW> in k_init_edge, <BF16T, InitX32Geo::NW> in k_init_x32.
// (NW: the launch's waves per block, 16 rows each)
template <class DT, int NW>
__device__ __forceinline__ void embed_block(const EmbedArgs& ea, WPipe<typename DT::T, NW, false, INIT_CAP>& pipe,
                                            int blk, int lane, int g) {
  using T = typename DT::T;
  const int r = blk * ROWS_PER_WAVE * NW + (threadIdx.x >> 6) * ROWS_PER_WAVE + (lane & 15);
  const bool valid = r < ea.Nt;
  const int v = valid ? r : ea.Nt - 1;
  const T* W = reinterpret_cast<const T*>(ea.wmat);
  pipe.issue(W + EM_EMB * BLK, MAT128);
  Act<8> x;
  const float* row = ea.node_f + (int64_t)v * ea.in_dim;
#pragma unroll
  for (int b = 0; b < 8; ++b)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int f = 16 * b + 4 * g + q;
      x.v[b][q] = f < ea.in_dim ? row[f] : 0.f;
    }
  const T* w = pipe.next();
  Act<8> h;
  zero(h);
  // bf16: the fragment ring; fp32: the 16x16x4 chain of k_node_embed<F32T> (same operands, same order)
  auto mm = [&](Act<8>& out, const Op<DT, 4>& op, const T* wm) {
    if constexpr (DT::kBF16) mma_ring<8, 4>(out, op, wm, lane);
    else mma<8, 4>(out, op, wm, lane);
  };
  {
    Op<DT, 4> xop;
    make_op(xop, x);
    mm(h, xop, w);
  }
  if (valid) store_row(h, reinterpret_cast<T*>(ea.h_out) + (int64_t)v * HID, g);
  Op<DT, 4> hop;
  make_op(hop, h);
  T* qkv = reinterpret_cast<T*>(ea.qkv_out);
#pragma unroll 1
  for (int q = 0; q < 3; ++q) {
    pipe.issue(W + (EM_Q + MAT128 * q) * BLK, MAT128);
    w = pipe.next();
    Act<8> t;
    init_vec(t, ea.wvec + EMV_Q + 128 * q, g);
    mm(t, hop, w);
    if (valid) store_row(t, qkv + (int64_t)v * 3 * HID + q * HID, g);
  }
}

// The fp32 InitEdge (the reference's precision: plain SiLU, unscaled weights); bf16 is k_init_x32.
template <bool GC>
__global__ __attribute__((amdgpu_flat_work_group_size(1, InitGeo::THREADS),
                          amdgpu_waves_per_eu(InitGeo::WPE, InitGeo::WPE)))
void k_init_edge(InitArgs a, EmbedArgs ea, int embed_blocks) {
  pq_signal_at_start(ea.sig_q, ea.sig_job);
  __shared__ __attribute__((aligned(16))) float lds[INIT_CAP * BLK];
  const int lane = lane_id(), g = lane >> 4;
  if constexpr (GC) {
    if ((int)blockIdx.x < embed_blocks) {  // uniform per block
      WPipe<float, InitGeo::NW, false, INIT_CAP> epipe(lds);
      embed_block<F32T, InitGeo::NW>(ea, epipe, blockIdx.x, lane, g);
      return;
    }
  }
  const int r = ((int)blockIdx.x - embed_blocks) * InitGeo::ROWS + (threadIdx.x >> 6) * ROWS_PER_WAVE + (lane & 15);
  const bool valid = r < a.Et;
  const int e = valid ? r : a.Et - 1;
  const float* W = reinterpret_cast<const float*>(a.wmat);
  WPipe<float, InitGeo::NW, false, INIT_CAP> pipe(lds);
  pipe.issue(W + IE_T0 * BLK, 8);  // stage 0: the collapsed edge-message map (8 blocks)

  Act<2> geo;
  load_edge_geo(geo, a.edge_f + (int64_t)e * NFEAT_E, g);
  Op<F32T, 1> gop;
  make_op(gop, geo);

  // combined_linear_0 over [emb[src], emb[dst], em0, silu(d0), silu(r0), silu(o0), silu(a0)]
  Act<8> acc;
  load_row(acc, a.pos_src + (int64_t)a.node_pos[a.src[e]] * HID, g);
  add_row(acc, a.pos_dst + (int64_t)a.node_pos[a.dst[e]] * HID, g);
  if constexpr (GC) add_vec(acc, a.wvec + IEV_ORC, g);  // orientation term (constant)
  // geometric terms t = 1..4 (dist, dir, orient, amide); GC: dist and amide only
  constexpr int NT = GC ? 2 : 4;
  auto geo_t = [](int i) { return GC ? (i == 0 ? 1 : 4) : i + 1; };
  {
    // t = 0: edge_messages_linear_0 and its combined_linear_0 slice, collapsed on the host into one
    // [128, 2] map of the message columns (no activation between them, :237-241)
    const float* w = pipe.next();
    pipe.issue(W + (IE_T0 + 40 * geo_t(0)) * BLK, 40);
    mma<8, 1>(acc, gop, w, lane);
  }
#pragma unroll 1
  for (int i = 0; i < NT; ++i) {
    const float* w = pipe.next();
    if (i + 1 < NT) pipe.issue(W + (IE_T0 + 40 * geo_t(i + 1)) * BLK, 40);
    else pipe.issue(W + IE_GEO1 * BLK, 40);
    Act<8> y;
    zero(y);
    mma<8, 1>(y, gop, w, lane);
    silu_<8, false>(y);
    linear<F32T, 8, 4>(acc, y, w + 8 * BLK, lane);
  }
  silu_<8, false>(acc);  // combined_edge_logits
  // gating: (em1 + silu(d1) + silu(r1) + silu(o1) + silu(a1)) * c
  {
    const float* w = pipe.next();
    pipe.issue(W + IE_C1 * BLK, 16);
    Act<8> gs;
    if constexpr (GC) init_vec(gs, a.wvec + IEV_OGATE, g);  // silu(o1): constant; silu(r1) = 0
    else zero(gs);
#pragma unroll 1
    for (int t = 0; t < 5; ++t) {
      if (GC && (t == 2 || t == 3)) continue;
      Act<8> y;
      zero(y);
      mma<8, 1>(y, gop, w + 8 * t * BLK, lane);
      if (t > 0) silu_<8, false>(y);
      add_(gs, y);
    }
    mul_(acc, gs);
  }
  const bool with_fn = a.fn_out != nullptr;  // uniform
  // combined_linear_2(combined_linear_1(.)) : 128 -> 28 (padded 32) -> 128
  Act<8> f;
  {
    const float* w = pipe.next();
    if (with_fn) pipe.issue(W + IE_NBR * BLK, MAT128);
    Act<2> z;
    zero(z);
    linear<F32T, 2, 4>(z, acc, w, lane);
    zero(f);
    linear<F32T, 8, 1>(f, z, w + 8 * BLK, lane);
  }
  if (valid) store_edge_row(f, reinterpret_cast<float*>(a.f_out) + (int64_t)e * HID, g);
  if (!with_fn) return;
  // layer-0 silu(nbr_linear(F)), applied once per edge and gathered by the conformation module
  // (silu(nbr_linear(F[ids])) == silu(nbr_linear(F))[ids], deepinteract_modules.py:386-390)
  {
    const float* w = pipe.next();
    Act<8> fn;
    init_vec(fn, a.wvec + IEV_NBR, g);
    linear<F32T, 8, 4>(fn, f, w, lane);
    silu_<8, false>(fn);
    if (valid) store_edge_row(fn, reinterpret_cast<float*>(a.fn_out) + (int64_t)e * HID, g);
  }
}

// Resident InitEdge weights (k_init_res_x32): the 128 weight blocks the GEO_REF path reads, at these
// block offsets of the LDS copy
constexpr int IR_NBLK = 128;  // resident weight blocks
constexpr int IR_T0 = 0, IR_DIST = 8, IR_AMIDE = 48, IR_GATE = 88, IR_C = 112;

// ================================================================ InitEdgeModule on 32x32x16 MFMA (bf16)
// The bf16 InitEdge: k_init_edge's phases on 32-row tiles (csrc/mfma32.h) with bf16 operands and
// log2-unit SiLUs (silu2_blk: the host packing scales the neighbouring weights). Every 128-wide stage is
// half the MFMAs of a 16x16 chain, so half the MFMA hold on the SIMD's vector issue the SiLU-heavy
// InitEdge is bound by (640 SiLU values per edge against 65,536 MAC). The bf16 init blob (kind 1) is
// packed in the 32x32 fragment order (di_blob_layout(1, bf16) == 32). Geometric terms and gates are
// produced one 32-feature block at a time (16 registers) and packed / multiplied straight away, so
// a 32-row tile fits three waves per SIMD (<= 168 VGPRs).
// Weight phases of one tile (GC: DI_GRAPH_GEO_REF batches):
//   T0 (collapsed edge-message map, [128x32] 8 blk) -> geometric terms (dist, [dir, orient,] amide:
//   [128x32] W_t0 + [128x128] combined_linear_0 slice, 40 blk each) -> gates (em1, dist1, [dir1,
//   orient1,] amide1: [128x32] each) -> combined_linear_1/2 (8 + 8 blk) -> [layer-0 nbr_linear, 32 blk]
constexpr int INIT_X32_NW = 4;  // waves per block (three waves per SIMD: 12 / NW blocks per CU)
struct InitX32Geo {
  static constexpr int NW = INIT_X32_NW, THREADS = 64 * NW, ROWS_PER_WAVE = 32, ROWS = ROWS_PER_WAVE * NW;
  static constexpr int EMBED_ROWS = 16 * NW;  // node rows of one embedding block of the same launch
};

// one 32-row tile of InitEdge; wt(phase) returns the phase's weight blocks (LDS) and gate_off(t) the
// block offset of gate t (0 em, 1 dist, 2 dir, 3 orient, 4 amide) inside the gates phase.
// acc enters holding emb[src] + emb[dst] slots (+ the orientation constant for GC).
// init_tile_x32_z stops at zop, combined_linear_1's 32-wide output as a packed operand, and returns
// the last phase's weights (combined_linear_1 at 0, combined_linear_2 at 8 blocks); init_tile_x32
// goes on to f = combined_linear_2(zop).
template <bool GC, class WT, class GO>
__device__ __forceinline__ const u16* init_tile_x32_z(X32<4>& acc, const P32<2>& gop, const float* wvec, int lane,
                                                      int h, WT&& wt, GO&& gate_off, P32<2>& zop) {
  mma32<4, 2>(acc, gop, wt(0), lane);  // t = 0: the collapsed [128, 2] edge-message map
  constexpr int NT = GC ? 2 : 4;
#pragma unroll 1
  for (int i = 0; i < NT; ++i) {
    const u16* w = wt(1 + i);
    // y = silu2(W_t0 . g), one 32-feature block at a time, packed as combined_linear_0's operand
    P32<8> yop;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      lean_fence();  // block by block: one block's fragments and values live at a time
      floatx16 y = {};
      y = mfma32(afrag(w, 2 * b, lane), gop.f[0], y);
      y = mfma32(afrag(w, 2 * b + 1, lane), gop.f[1], y);
      silu2_blk(y);
      pack_blk(yop.f[2 * b], yop.f[2 * b + 1], y);
      asm volatile("" : "+v"(yop.f[2 * b]), "+v"(yop.f[2 * b + 1]));
    }
    mma32<4, 8>(acc, yop, w + 8 * BLK, lane);
    pin(acc);
  }
#pragma unroll
  for (int b = 0; b < 4; ++b) silu2_blk(acc.v[b]);  // combined_edge_logits (log2 units)
  pin(acc);  // computed here: sunk to their uses, x and rcp(1 + 2^-x) would both stay live
  // gating: (em1 + silu(d1) + silu(r1) + silu(o1) + silu(a1)) * c, block by block
  {
    const u16* w = wt(1 + NT);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      lean_fence();
      floatx16 gs = {};
      if constexpr (GC) {  // silu(o1): the packed constant IEV_OGATE (silu(r1) = 0)
#pragma unroll
        for (int q = 0; q < 4; ++q) set_quad(gs, q, ld4(wvec + IEV_OGATE + 32 * b + 8 * q + 4 * h));
      }
#pragma unroll
      for (int t = 0; t < 5; ++t) {
        if (GC && (t == 2 || t == 3)) continue;
        __builtin_amdgcn_sched_barrier(0);
        floatx16 y = {};
        const u16* wg = w + gate_off(t) * BLK;
        y = mfma32(afrag(wg, 2 * b, lane), gop.f[0], y);
        y = mfma32(afrag(wg, 2 * b + 1, lane), gop.f[1], y);
        if (t > 0) silu2_blk(y);
        gs += y;
      }
      acc.v[b] *= gs;
      asm volatile("" : "+v"(acc.v[b]));  // computed here (not sunk past the next stage barrier)
    }
  }
  // combined_linear_1 : 128 -> 28 (padded 32)
  const u16* w = wt(2 + NT);
  P32<8> aop;
  make_op32(aop, acc);
  X32<1> z;
  zero(z);
  mma32<1, 8>(z, aop, w, lane);
  make_op32(zop, z);
  return w;
}
template <bool GC, class WT, class GO>
__device__ __forceinline__ void init_tile_x32(X32<4>& acc, const P32<2>& gop, const float* wvec, int lane, int h,
                                              WT&& wt, GO&& gate_off, X32<4>& f) {
  P32<2> zop;
  const u16* w = init_tile_x32_z<GC>(acc, gop, wvec, lane, h, wt, gate_off, zop);
  // combined_linear_2 : 32 -> 128
  zero(f);
  mma32<4, 2>(f, zop, w + 8 * BLK, lane);
}

// acc = pos_src[node_pos[src]] + pos_dst[node_pos[dst]] (the orientation constant of GEO_REF batches
// arrives through the collapsed message map: geo_op32<true>)
__device__ __forceinline__ void init_acc_x32(X32<4>& acc, const InitArgs& a, int ps, int pd, int h) {
  const float* rs = a.pos_src + (int64_t)ps * HID;
  const float* rd = a.pos_dst + (int64_t)pd * HID;
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int f = 32 * b + 8 * q + 4 * h;
      set_quad(acc.v[b], q, ld4(rs + f) + ld4(rd + f));
    }
}

// the edge's geometric features [28] as a 32-feature operand; ONE: features 28 and 29 = 1 (the
// bf16 hi / lo columns of the orientation constant in the 32x32 init blob's message map), else 0
template <bool ONE = false>
__device__ __forceinline__ void geo_op32(P32<2>& gop, const float* edge_f, int e, int h) {
  const float* grow = edge_f + (int64_t)e * NFEAT_E;
  X32<1> geo;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int f = 8 * q + 4 * h;
    set_quad(geo.v[0], q, f < NFEAT_E ? ld4(grow + f) : (ONE ? (floatx4){1.f, 1.f, 0.f, 0.f} : (floatx4){0.f, 0.f, 0.f, 0.f}));
  }
  make_op32(gop, geo);
}

// staged weights (one INIT_CAP-block slot per block, three blocks per CU); the first
// embed_blocks blocks run the node embedding (16x16 k_node_embed arithmetic, kind-0 blob)
// <= 160 VGPRs (amdgpu_num_vgpr counts register pairs): three waves per SIMD hold 480 of the 512
// registers, leaving exactly one 32-register pair-tensor wave room beside them. At 161 (168 allocated)
// the pair kernel's persistent blocks found no SIMD with room while InitEdge ran and the overlapped
// pair tensor slowed from ~1050 to ~1540 us per micro-batch (round 4)
// Z (GC, no Fn): the tile stops at combined_linear_1's output and stores it as the 64-B z0 row
// (mfma32.h) in a.f_out's place; combined_linear_2 is applied by layer 0's edge kernel
// (k_edge_x32_ring<0, true, true>), so the 256-B F0 row is never written
template <bool GC, bool Z = false>
__global__ __attribute__((amdgpu_flat_work_group_size(1, InitX32Geo::THREADS), amdgpu_waves_per_eu(3, 3),
                          amdgpu_num_vgpr(80)))
void k_init_x32(InitArgs a, EmbedArgs ea, int embed_blocks) {
  static_assert(GC || !Z, "the z0 form is the DI_GRAPH_GEO_REF path");
  pq_signal_at_start(ea.sig_q, ea.sig_job);
  constexpr int NW = InitX32Geo::NW;
  __shared__ __attribute__((aligned(16))) u16 lds[INIT_CAP * BLK];
  const int lane = lane_id();
  if ((int)blockIdx.x < embed_blocks) {  // uniform per block
    WPipe<u16, NW, false, INIT_CAP> epipe(lds);
    embed_block<BF16T, NW>(ea, epipe, blockIdx.x, lane, lane >> 4);
    return;
  }
  const int h = lane >> 5;
  const int r = ((int)blockIdx.x - embed_blocks) * InitX32Geo::ROWS + (threadIdx.x >> 6) * InitX32Geo::ROWS_PER_WAVE +
                (lane & 31);
  const bool valid = r < a.Et;
  const int e = valid ? r : a.Et - 1;
  const u16* W = reinterpret_cast<const u16*>(a.wmat);
  WPipe<u16, NW, false, INIT_CAP> pipe(lds);
  pipe.issue(W + IE_T0 * BLK, 8);
  P32<2> gop;
  geo_op32<GC>(gop, a.edge_f, e, h);
  X32<4> acc;
  init_acc_x32(acc, a, a.node_pos[a.src[e]], a.node_pos[a.dst[e]], h);
  const bool with_fn = a.fn_out != nullptr;  // uniform
  constexpr int NT = GC ? 2 : 4;
  auto geo_t = [](int i) { return GC ? (i == 0 ? 1 : 4) : i + 1; };
  // phase p's weights: wait for its stage, issue the next one
  auto wt = [&](int p) -> const u16* {
    const u16* w = pipe.next();
    if (p == 0) pipe.issue(W + (IE_T0 + 40 * geo_t(0)) * BLK, 40);
    else if (p < NT) pipe.issue(W + (IE_T0 + 40 * geo_t(p)) * BLK, 40);
    else if (p == NT) {
      if constexpr (GC) {  // em1, dist1 and amide1 only: dir1 / orient1 (blocks 16-31) are never read
        pipe.issue(W + IE_GEO1 * BLK, 16);
        pipe.issue2(W + (IE_GEO1 + 32) * BLK, 8);
      } else {
        pipe.issue(W + IE_GEO1 * BLK, 40);
      }
    }
    else if (p == NT + 1) pipe.issue(W + IE_C1 * BLK, Z ? 8 : 16);
    else if (with_fn) pipe.issue(W + IE_NBR * BLK, MAT128);
    return w;
  };
  // block offset of gate t in the gates phase (GC: the three gates fetched, back to back)
  auto gate_off = [](int t) { return GC ? (t == 0 ? 0 : (t == 1 ? 8 : 16)) : 8 * t; };
  if constexpr (Z) {
    P32<2> zop;
    init_tile_x32_z<GC>(acc, gop, a.wvec, lane, h, wt, gate_off, zop);
    if (valid) store_z0(zop, reinterpret_cast<u16*>(a.f_out), e, h);
    return;
  }
  // The F / Fn stores take the lane half and the row predicate from a lane id read afresh
  // (v_mbcnt): held live from the top of the kernel for the 16-B stores they cost the registers the
  // 160 cap does not have (scratch)
  auto store_f = [&](const X32<4>& t, void* out) {
    int l = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    asm volatile("" : "+v"(l));
    const int rr = ((int)blockIdx.x - embed_blocks) * InitX32Geo::ROWS + (threadIdx.x >> 6) * InitX32Geo::ROWS_PER_WAVE +
                   (l & 31);
    store_row32(t, reinterpret_cast<u16*>(out) + (int64_t)e * HID, l >> 5, rr < a.Et);
  };
  X32<4> f;
  init_tile_x32<GC>(acc, gop, a.wvec, lane, h, wt, gate_off, f);
  store_f(f, a.f_out);
  if (!with_fn) return;
  // layer-0 silu(nbr_linear(F)), applied once per edge and gathered by the conformation module
  const u16* w = pipe.next();
  P32<8> fop;
  make_op32(fop, f);
  X32<4> fn;
  init_vec32(fn, a.wvec + IEV_NBR, h);
  mma32<4, 8>(fn, fop, w, lane);
#pragma unroll
  for (int b = 0; b < 4; ++b) silu_blk(fn.v[b]);
  store_f(fn, a.fn_out);
}

// resident weights (DI_GRAPH_GEO_REF, no Fn): the path's 128 blocks loaded once per CU into LDS
// (block offsets IR_*), one 12-wave block per CU, waves striding over 32-edge tiles with the
// next tile's src/dst -> node_pos chain issued a tile ahead
constexpr int IRX_NW = 12;
__global__ __attribute__((amdgpu_flat_work_group_size(1, 64 * IRX_NW), amdgpu_waves_per_eu(IRX_NW / 4, IRX_NW / 4)))
void k_init_res_x32(InitArgs a, int ntiles) {
  __shared__ __attribute__((aligned(16))) u16 w[IR_NBLK * BLK];
  const u16* W = reinterpret_cast<const u16*>(a.wmat);
  dma_blocks<IRX_NW>(w + IR_T0 * BLK, W + IE_T0 * BLK, 8);
  dma_blocks<IRX_NW>(w + IR_DIST * BLK, W + (IE_T0 + 40 * 1) * BLK, 40);
  dma_blocks<IRX_NW>(w + IR_AMIDE * BLK, W + (IE_T0 + 40 * 4) * BLK, 40);
  dma_blocks<IRX_NW>(w + IR_GATE * BLK, W + IE_GEO1 * BLK, 16);               // em1, dist1
  dma_blocks<IRX_NW>(w + (IR_GATE + 16) * BLK, W + (IE_GEO1 + 32) * BLK, 8);  // amide1
  dma_blocks<IRX_NW>(w + IR_C * BLK, W + IE_C1 * BLK, 16);                    // combined_linear_1, _2
  lds_dma_wait();
  __syncthreads();
  const int lane = lane_id(), h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int stride = gridDim.x * IRX_NW;
  auto edge_of = [&](int t) {
    const int r = t * 32 + (lane & 31);
    return r < a.Et ? r : a.Et - 1;
  };
  int tile = blockIdx.x * IRX_NW + wave;
  int ps = 0, pd = 0;
  if (tile < ntiles) {
    const int e = edge_of(tile);
    ps = a.node_pos[a.src[e]];
    pd = a.node_pos[a.dst[e]];
  }
  auto wt = [&](int p) -> const u16* {
    return w + (p == 0 ? IR_T0 : p == 1 ? IR_DIST : p == 2 ? IR_AMIDE : p == 3 ? IR_GATE : IR_C) * BLK;
  };
  auto gate_off = [](int t) { return t == 0 ? 0 : (t == 1 ? 8 : 16); };  // em1, dist1, amide1
#pragma unroll 1
  for (; tile < ntiles; tile += stride) {
    const int r = tile * 32 + (lane & 31);
    const bool valid = r < a.Et;
    const int e = valid ? r : a.Et - 1;
    P32<2> gop;
    geo_op32<true>(gop, a.edge_f, e, h);
    X32<4> acc;
    init_acc_x32(acc, a, ps, pd, h);
    const bool more = tile + stride < ntiles;  // uniform
    if (more) {  // the next tile's positional-row indices
      const int en = edge_of(tile + stride);
      ps = a.node_pos[a.src[en]];
      pd = a.node_pos[a.dst[en]];
    }
    X32<4> f;
    init_tile_x32<true>(acc, gop, a.wvec, lane, h, wt, gate_off, f);
    store_row32(f, reinterpret_cast<u16*>(a.f_out) + (int64_t)e * HID, h, valid);
  }
}

}  // namespace di

// ================================================================ C ABI
using namespace di;

extern "C" int di_node_embed(const di_graph* g, di_dtype dt, int32_t in_dim, const float* node_f, const void* wmat,
                             const float* wvec, void* h_out, void* qkv_out, void* queue, int32_t signal_job,
                             void* stream) {
  if (!g || !node_f || !wmat || !wvec || !h_out || !qkv_out || g->num_nodes <= 0 || in_dim <= 0 || in_dim > HID ||
      !dtype_ok(dt))
    return DI_EINVAL;
  EmbedArgs a{g->num_nodes, in_dim, node_f, wmat, wvec, h_out, qkv_out, (uint32_t*)queue, signal_job};
  hipStream_t s = (hipStream_t)stream;
  if (dt == DI_BF16)
    hipLaunchKernelGGL(k_node_embed<BF16T>, grid_of<EmbedGeo>(a.Nt), block_of<EmbedGeo>(), 0, s, a);
  else
    hipLaunchKernelGGL(k_node_embed<F32T>, grid_of<EmbedGeo>(a.Nt), block_of<EmbedGeo>(), 0, s, a);
  return launch_status();
}

extern "C" int di_init_edge(const di_graph* g, di_dtype dt, const float* edge_f, const void* wmat,
                            const float* wvec, const float* pos_src_tab, const float* pos_dst_tab,
                            void* f_out, void* fn_out, void* stream) {
  const bool gc = (g ? g->flags : 0) & DI_GRAPH_GEO_REF;
  if (!g || !edge_f || !wmat || !wvec || !pos_src_tab || !pos_dst_tab || !f_out || (!fn_out && !gc) ||
      g->num_edges <= 0 || !dtype_ok(dt))
    return DI_EINVAL;
  InitArgs a{g->num_edges, edge_f, g->src, g->dst, g->node_pos, wmat, wvec, pos_src_tab, pos_dst_tab,
             f_out, fn_out};
  hipStream_t s = (hipStream_t)stream;
  const dim3 gf = grid_of<InitGeo>(a.Et), bf = block_of<InitGeo>();
  const EmbedArgs ne{};
  const dim3 gx((unsigned)((a.Et + InitX32Geo::ROWS - 1) / InitX32Geo::ROWS)), bx(InitX32Geo::THREADS);
  if (dt == DI_BF16 && gc) hipLaunchKernelGGL((k_init_x32<true>), gx, bx, 0, s, a, ne, 0);
  else if (dt == DI_BF16) hipLaunchKernelGGL((k_init_x32<false>), gx, bx, 0, s, a, ne, 0);
  else if (gc) hipLaunchKernelGGL((k_init_edge<true>), gf, bf, 0, s, a, ne, 0);
  else hipLaunchKernelGGL((k_init_edge<false>), gf, bf, 0, s, a, ne, 0);
  return launch_status();
}

// The embedding blocks, then the InitEdge blocks, in one launch (Z: the bf16 z0 form)
template <class DT, bool Z = false>
static void launch_embed_init(const InitArgs& a, const EmbedArgs& ea, hipStream_t s) {
  if constexpr (DT::kBF16) {
    const int eb = (ea.Nt + InitX32Geo::EMBED_ROWS - 1) / InitX32Geo::EMBED_ROWS;
    const int ib = (a.Et + InitX32Geo::ROWS - 1) / InitX32Geo::ROWS;
    hipLaunchKernelGGL((k_init_x32<true, Z>), dim3((unsigned)(eb + ib)), dim3(InitX32Geo::THREADS), 0, s, a, ea, eb);
  } else {
    const int eb = (ea.Nt + InitGeo::ROWS - 1) / InitGeo::ROWS;
    const int ib = (a.Et + InitGeo::ROWS - 1) / InitGeo::ROWS;
    hipLaunchKernelGGL((k_init_edge<true>), dim3((unsigned)(eb + ib)), block_of<InitGeo>(), 0, s, a, ea, eb);
  }
}

// di_embed_init_edge and its z form: one argument check, one launch. z: `out` takes z0 rows in the
// F rows' place (k_init_x32<true, true>), bf16 only.
static int embed_init_edge(bool z, const di_graph* g, di_dtype dt, int32_t in_dim, const float* node_f,
                           const void* embed_wmat, const float* embed_wvec, void* h_out, void* qkv_out,
                           const float* edge_f, const void* init_wmat, const float* init_wvec,
                           const float* pos_src_tab, const float* pos_dst_tab, void* out, void* queue,
                           int32_t signal_job, void* stream) {
  if (!g || !(g->flags & DI_GRAPH_GEO_REF) || !g->src || !g->dst || !g->node_pos || g->num_nodes <= 0 ||
      g->num_edges <= 0 || in_dim <= 0 || in_dim > HID || !node_f || !embed_wmat || !embed_wvec || !h_out ||
      !qkv_out || !edge_f || !init_wmat || !init_wvec || !pos_src_tab || !pos_dst_tab || !out ||
      (z ? dt != DI_BF16 : !dtype_ok(dt)))
    return DI_EINVAL;
  EmbedArgs ea{g->num_nodes, in_dim, node_f, embed_wmat, embed_wvec, h_out, qkv_out, (uint32_t*)queue, signal_job};
  InitArgs a{g->num_edges, edge_f, g->src, g->dst, g->node_pos, init_wmat, init_wvec, pos_src_tab, pos_dst_tab,
             out, nullptr};
  hipStream_t s = (hipStream_t)stream;
  if (z) launch_embed_init<BF16T, true>(a, ea, s);
  else if (dt == DI_BF16) launch_embed_init<BF16T>(a, ea, s);
  else launch_embed_init<F32T>(a, ea, s);
  return launch_status();
}

extern "C" int di_embed_init_edge(const di_graph* g, di_dtype dt, int32_t in_dim, const float* node_f,
                                  const void* embed_wmat, const float* embed_wvec, void* h_out, void* qkv_out,
                                  const float* edge_f, const void* init_wmat, const float* init_wvec,
                                  const float* pos_src_tab, const float* pos_dst_tab, void* f_out, void* queue,
                                  int32_t signal_job, void* stream) {
  return embed_init_edge(false, g, dt, in_dim, node_f, embed_wmat, embed_wvec, h_out, qkv_out, edge_f, init_wmat,
                         init_wvec, pos_src_tab, pos_dst_tab, f_out, queue, signal_job, stream);
}

extern "C" int di_embed_init_edge_z(const di_graph* g, di_dtype dt, int32_t in_dim, const float* node_f,
                                    const void* embed_wmat, const float* embed_wvec, void* h_out, void* qkv_out,
                                    const float* edge_f, const void* init_wmat, const float* init_wvec,
                                    const float* pos_src_tab, const float* pos_dst_tab, void* z_out, void* queue,
                                    int32_t signal_job, void* stream) {
  return embed_init_edge(true, g, dt, in_dim, node_f, embed_wmat, embed_wvec, h_out, qkv_out, edge_f, init_wmat,
                         init_wvec, pos_src_tab, pos_dst_tab, z_out, queue, signal_job, stream);
}

extern "C" int di_init_edge_resident(const di_graph* g, const float* edge_f, const void* wmat, const float* wvec,
                                     const float* pos_src_tab, const float* pos_dst_tab, void* f_out, void* stream) {
  if (!g || !(g->flags & DI_GRAPH_GEO_REF) || !g->src || !g->dst || !g->node_pos || !edge_f || !wmat || !wvec ||
      !pos_src_tab || !pos_dst_tab || !f_out || g->num_edges <= 0)
    return DI_EINVAL;
  InitArgs a{g->num_edges, edge_f, g->src, g->dst, g->node_pos, wmat, wvec, pos_src_tab, pos_dst_tab, f_out, nullptr};
  // one block per CU holding the path's weights; never more blocks than the 32-edge tiles need at one
  // per wave
  const int ntiles = (a.Et + 31) / 32;
  hipLaunchKernelGGL(k_init_res_x32, persistent_grid(ntiles, IRX_NW).grid, dim3(64 * IRX_NW), 0,
                     (hipStream_t)stream, a, ntiles);
  return launch_status();
}
