// GeoT, edge layer: the fused edge layer on 16x16 MFMA (fp32 layers, the conformation module alone),
// the bf16 layers on 32x32 MFMA over the 8-wave weight ring with the attention fold, and their entry
// points (reference semantics: geot.h).
#include "geot.h"
#include "mfma32.h"

namespace di {

// ================================================================ fused edge layer
// Weight stage order of the edge layer: block offsets / sizes (csrc/layout.h) and the fp32
// vector (bias) staged with each layer (-1: none).
__constant__ int EL_ORDER[25] = {
    EL_S0, EL_UP, EL_OM,
    EL_RES + 0 * MAT128, EL_RES + 1 * MAT128, EL_RES + 2 * MAT128,
    EL_RES + 3 * MAT128, EL_RES + 4 * MAT128, EL_RES + 5 * MAT128,
    EL_RC,
    EL_RES + 6 * MAT128, EL_RES + 7 * MAT128, EL_RES + 8 * MAT128,
    EL_RES + 9 * MAT128, EL_RES + 10 * MAT128, EL_RES + 11 * MAT128,
    EL_FG, EL_F, EL_P,
    EL_OE, EL_F1, EL_F2, EL_F1 + MAT128, EL_F2 + MAT128, EL_NN};
__constant__ int EL_SIZE[25] = {36, 16, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32,
                                32, 32, 32, 8, 32, 32, 32, 32, 32, 32, 32, 32};
__constant__ int EL_VEC[25] = {-1, ELV_OM, -1,
                               ELV_RES + 0 * 128, ELV_RES + 1 * 128, ELV_RES + 2 * 128,
                               ELV_RES + 3 * 128, ELV_RES + 4 * 128, ELV_RES + 5 * 128,
                               ELV_RC,
                               ELV_RES + 6 * 128, ELV_RES + 7 * 128, ELV_RES + 8 * 128,
                               ELV_RES + 9 * 128, ELV_RES + 10 * 128, ELV_RES + 11 * 128,
                               -1, ELV_F, ELV_P,
                               ELV_OE, ELV_F1, -1, ELV_F1 + 128, -1, ELV_NN};
constexpr int EL_NSTAGE_CONF = 18, EL_NSTAGE_FINAL = 19, EL_NSTAGE = 25;
constexpr int EL_CAP = 36;

// k_edge_layer: 16 rows per wave, 4-wave blocks, two blocks per CU: the fp32 edge layers (the
// reference's precision; the bf16 layers are k_edge_x32_ring below) and the conformation module
// alone (di_conformation, both dtypes).
template <class DT>
using EdgePipe = WPipe<typename DT::T, Geo<DT>::NW, Geo<DT>::DBUF, EL_CAP, 128>;

// MODE: 0 intermediate layer, 1 final layer, 2 conformation module alone (di_conformation)
template <int MODE>
constexpr int edge_nstage() { return MODE == 2 ? EL_NSTAGE_CONF : (MODE == 1 ? EL_NSTAGE_FINAL : EL_NSTAGE); }

// The weight-stage sequence of one tile: next() makes the next stage current (its weights w(),
// its bias vector v()) and issues the DMA of the one after it.
// GC (DI_GRAPH_GEO_REF batches, layer modes 0/1): the sequence starts at orig_msg_linear, which
// then carries the orig_msg_linear bias, and (intermediate layers) ends before nbr_linear
template <class DT, int MODE, bool GC = false>
struct EdgeStages {
  using T = typename DT::T;
  static constexpr int NS = edge_nstage<MODE>() - (GC ? (MODE == 1 ? 2 : 3) : 0);
  EdgePipe<DT>& pipe;
  const T* W;
  const float* V;
  int gi;  // index of the next stage to make current
  __device__ void issue(int s0) {
    const int s = GC ? s0 + 2 : s0;
    const int vo = (GC && s0 == 0) ? ELV_OM : EL_VEC[s];
    pipe.issue(W + EL_ORDER[s] * BLK, EL_SIZE[s], vo >= 0 ? V + vo : nullptr, 128);
  }
  __device__ void begin() { issue(0); }
  __device__ const T* next() {
    const int i = gi++;
    const T* w = pipe.next();
    if (i + 1 < NS) issue(i + 1);
    return w;
  }
  __device__ const float* v() const { return pipe.v(); }
};

template <class DT, int MODE, bool GC>
__device__ __forceinline__ void res_block(Act<8>& x, EdgeStages<DT, MODE, GC>& st, int lane, int g) {
  constexpr bool FAST = DT::kBF16;
  Act<8> y = x;
#pragma unroll 1
  for (int l = 0; l < 3; ++l) {
    const typename DT::T* w = st.next();
    Act<8> t;
    init_vec_lds(t, st.v(), g);
    linear<DT, 8, 4>(t, y, w, lane);
    silu2_<8, FAST>(t);  // log2 units: folded into the next linear / the residual fma
    y = t;
  }
  add_scaled_(x, y, silu2_unit<FAST>());
}

// Two 4-wave blocks per CU, each wave capped at 240 VGPRs (amdgpu_num_vgpr counts the unified
// VGPR+AGPR file in pairs on gfx950): 2 x 240 + 32 = 512 leaves one pair-tensor wave per SIMD
// co-resident. One 64-row tile per block.
// GC (DI_GRAPH_GEO_REF, modes 0/1): the neighbour-message stages are skipped (exactly zero) and no
// silu(nbr_linear(F)) rows are gathered or written.
template <class DT, int MODE, bool GC = false>
__global__ __attribute__((amdgpu_flat_work_group_size(1, Geo<DT>::THREADS), amdgpu_waves_per_eu(2, 2),
                          amdgpu_num_vgpr(120)))
void k_edge_layer(EdgeArgs a) {
  constexpr bool FINAL = MODE == 1, CONF = MODE == 2;
  using T = typename DT::T;
  using G = Geo<DT>;
  constexpr bool FAST = DT::kBF16;
  static_assert(!DT::kBF16 || MODE == 2, "the bf16 layers are k_edge_x32_ring's; bf16 here is di_conformation only");
  __shared__ __attribute__((aligned(16))) char lds[(G::DBUF ? 2 : 1) * EdgePipe<DT>::SLOT_BYTES];
  const int lane = lane_id(), g = lane >> 4;
  const int r = row_id<G::NW>();
  const bool valid = r < a.Et;
  const int e = valid ? r : a.Et - 1;
  const T* W = reinterpret_cast<const T*>(a.wmat);
  const T* fn_in = reinterpret_cast<const T*>(a.fn_in);
  const T* qkv = reinterpret_cast<const T*>(a.qkv);
  const T* f_row = reinterpret_cast<const T*>(a.f_in) + (int64_t)e * HID;

  EdgePipe<DT> pipe(lds);
  EdgeStages<DT, MODE, GC> st{pipe, W, a.wvec, 0};
  st.begin();
  int4 nb = {0, 0, 0, 0};
  if constexpr (!GC) nb = *reinterpret_cast<const int4*>(a.nbr + (int64_t)e * 4);
  Op<DT, 1> gop;
  {
    Act<2> geo;
    load_edge_geo(geo, a.edge_f + (int64_t)e * NFEAT_E, g);
    make_op(gop, geo);
  }
  FRow<DT> fr;
  if constexpr (DT::kBF16) {
    RawRow<T> fraw;
    fraw.load(f_row, g);
    fr.set_raw(fraw);
  }

  const T* w;
  Act<8> x;
  if constexpr (GC) {
    // DI_GRAPH_GEO_REF: the neighbour messages are multiplied by dir_linear_1(dir_linear_0(0)) = 0
    // (:408): x = orig_msg_linear(F) + b exactly
    w = st.next();  // orig_msg_linear (+ its bias)
    init_vec_lds(x, st.v(), g);
  } else {
    // ---- neighbour-edge messages (conformation_module_message_func :384-418)
    RawRow<T> xn;
    xn.load(fn_in + (int64_t)nb.x * HID, g);
    w = st.next();  // stage 0: geometric gates + downward_proj
    Act<4> gate;    // dir . orient . amide embeddings (64)
    {
      Act<4> t1;
      zero(gate);
      mma<4, 1>(gate, gop, w + 8 * BLK, lane);
      zero(t1);
      mma<4, 1>(t1, gop, w + 12 * BLK, lane);
      mul_(gate, t1);
      zero(t1);
      mma<4, 1>(t1, gop, w + 16 * BLK, lane);
      mul_(gate, t1);
    }
    Act<4> s;
    zero(s);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      Act<8> xa;
      xn.to_act(xa);
      if (j < 3) {  // prefetch the next neighbour row under this one's MFMAs
        const int nx = j == 0 ? nb.y : (j == 1 ? nb.z : nb.w);
        xn.load(fn_in + (int64_t)nx * HID, g);
      }
      // dist_linear_1(dist_linear_0(dist)), recomputed per neighbour (8 MFMAs) rather than held
      // live across the loop: the memory clobber stops the compiler from hoisting it (32 VGPRs)
      asm volatile("" ::: "memory");
      Act<8> dg;
      zero(dg);
      mma<8, 1>(dg, gop, w, lane);
#pragma unroll
      for (int b = 0; b < 8; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) xa.v[b][q] *= dg.v[b][q];  // gathered rows are silu(nbr_linear(F))
      Act<4> y;
      zero(y);
      linear<DT, 4, 4>(y, xa, w + 20 * BLK, lane);  // downward_proj
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) s.v[b][q] += silu2<FAST>(y.v[b][q]) * gate.v[b][q];
    }
    w = st.next();  // stage 1: upward_proj (+ orig_msg_linear bias)
    zero(x);
    linear<DT, 8, 2>(x, s, w, lane);
    silu2_<8, FAST>(x);
    {
      Act<8> bo;
      init_vec_lds(bo, st.v(), g);
#pragma unroll
      for (int b = 0; b < 8; ++b) x.v[b] = silu2_unit<FAST>() * x.v[b] + bo.v[b];
    }
    w = st.next();  // stage 2: orig_msg_linear(res) + nbr
  }
  mma<8, 4>(x, fr.operand(f_row, g), w, lane);
  res_block<DT, MODE, GC>(x, st, lane, g);
  res_block<DT, MODE, GC>(x, st, lane, g);
  {
    w = st.next();  // res_connect_linear
    Act<8> y;
    init_vec_lds(y, st.v(), g);
    linear<DT, 8, 4>(y, x, w, lane);
    silu2_<8, FAST>(y);
    fr.act(x, f_row, g);
    add_scaled_(x, y, silu2_unit<FAST>());
  }
  res_block<DT, MODE, GC>(x, st, lane, g);
  res_block<DT, MODE, GC>(x, st, lane, g);
  {
    w = st.next();  // final geometric gate
    Act<8> fg;
    zero(fg);
    mma<8, 1>(fg, gop, w, lane);
    mul_(x, fg);
    w = st.next();  // final_linear
    Act<8> y;
    init_vec_lds(y, st.v(), g);
    linear<DT, 8, 4>(y, x, w, lane);
    silu2_<8, FAST>(y);
    fr.act(x, f_row, g);
    add_scaled_(x, y, silu2_unit<FAST>());  // conformation output
  }
  if constexpr (CONF) {
    if (valid) store_row(x, reinterpret_cast<T*>(a.f_out) + (int64_t)e * HID, g);
    return;
  } else {
    // ---- attention scores (propagate_attention :76-91)
    const int sn = a.src[e], dn = a.dst[e];
    RawRow<T> kr, qr;  // K[src], Q[dst] in flight under the projection's MFMAs
    kr.load(qkv + (int64_t)sn * 3 * HID + HID, g);
    qr.load(qkv + (int64_t)dn * 3 * HID, g);
    w = st.next();  // edge_feats_projection(BN1e(conf))
    Act<8> p;
    init_vec_lds(p, st.v(), g);
    linear<DT, 8, 4>(p, x, w, lane);
    {
      Act<8> kq, qd;
      kr.to_act(kq);
      qr.to_act(qd);
      const float scale = 5.656854249492381f;  // np.sqrt(32)
#pragma unroll
      for (int b = 0; b < 8; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float sc = (kq.v[b][q] * qd.v[b][q]) / scale;
          sc = fminf(fmaxf(sc, -5.f), 5.f);
          p.v[b][q] = sc * p.v[b][q];  // score = e_out
        }
    }
    floatx4 al;
#pragma unroll
    for (int h = 0; h < 4; ++h) al[h] = expf(fminf(fmaxf(head_sum(p, h), -5.f), 5.f));
    if (valid && g == 0) st4(a.alpha_out + (int64_t)e * 4, al);

    if constexpr (!FINAL) {
      // ---- edge output: e = in + O_e(e_out); e = e + FFN(BN2e(e)) (:697-724)
      w = st.next();  // O_edge_feats
      Act<8> e1;
      init_vec_lds(e1, st.v(), g);
      linear<DT, 8, 4>(e1, p, w, lane);
      {
        Act<8> fa;
        fr.act(fa, f_row, g);
        add_(e1, fa);
      }
      Act<8> o;
      zero(o);
#pragma unroll 1
      for (int half = 0; half < 2; ++half) {
        w = st.next();  // edge_feats_MLP.0 (BN2e folded), hidden half
        Act<8> t;
        init_vec_lds(t, st.v(), g);
        linear<DT, 8, 4>(t, e1, w, lane);
        silu_<8, false>(t);
        w = st.next();  // edge_feats_MLP.3, input half
        linear<DT, 8, 4>(o, t, w, lane);
      }
      add_(e1, o);
      if (valid) store_edge_row(e1, reinterpret_cast<T*>(a.f_out) + (int64_t)e * HID, g);
      if constexpr (GC) return;  // no silu(nbr_linear(F)) rows for the next layer
      w = st.next();  // next layer's silu(nbr_linear(.))
      Act<8> fn;
      init_vec_lds(fn, st.v(), g);
      linear<DT, 8, 4>(fn, e1, w, lane);
      silu_<8, false>(fn);
      if (valid) store_edge_row(fn, reinterpret_cast<T*>(a.fn_out) + (int64_t)e * HID, g);
    }
  }
}

// ================================================================ fused edge layer on 32x32x16 MFMA (bf16)
// The bf16 edge layers: k_edge_layer's stage sequence (EL_ORDER / EL_SIZE / EL_VEC) with the log2-unit
// SiLUs, the reciprocal score scale and __expf of the bf16 product, each wave's 32 rows as ONE 32x32
// tile (csrc/mfma32.h): a 128x128 linear is 32 v_mfma_f32_32x32x16_bf16 per wave. The weight stages
// arrive on an 8-wave LDS ring (k_edge_x32_ring below); the weight blobs are packed in the 32x32
// fragment order (packing.pack_matrix32, di_blob_layout() == 32). Pinned to the fp64 oracle by
// tests/test_gpu_geot_edge_shapes.py.

// x through one ResBlock: two silu2(W . + b) layers packed as the next operand, then x += ln2 * silu2(W . + b)
template <class ST>
__device__ __forceinline__ void x32_res_block(X32<4>& x, ST& st, int lane, int h) {
  P32<8> op;
  make_op32(op, x);
#pragma unroll 1
  for (int l = 0; l < 2; ++l) {
    const u16* w = st.next();
    X32<4> t;
    P32<8> opn;
    lin32_pipe<8>(t, op, w, st.v(), lane, h, [&](int b) {
      silu2_blk(t.v[b]);
      pack_blk(opn.f[2 * b], opn.f[2 * b + 1], t.v[b]);
    });
    op = opn;
    pin(op);
  }
  const u16* w = st.next();
  X32<4> t;
  lin32_pipe<8>(t, op, w, st.v(), lane, h, [&](int b) {
    silu2_blk(t.v[b]);
    x.v[b] += silu2_unit<true>() * t.v[b];
  });
  pin(x);
}

// x = F + ln2 * silu2(W x + b)  (res_connect_linear / final_linear residual; F the edge's bf16 row)
__device__ __forceinline__ void x32_f_residual(X32<4>& x, const u16* w, const float* v, const R32<4>& fr, int lane,
                                               int h) {
  P32<8> op;
  make_op32(op, x);
  X32<4> y;
  lin32_pipe<8>(y, op, w, v, lane, h, [&](int b) {
    silu2_blk(y.v[b]);
#pragma unroll
    for (int q = 0; q < 4; ++q) set_quad(x.v[b], q, unpack4(fr.u[4 * b + q]) + silu2_unit<true>() * quad(y.v[b], q));
  });
  pin(x);
}
// the same with F taken block by block from fblk(b) (an R32<1>: the z0 form rebuilds F0's blocks)
template <class FB>
__device__ __forceinline__ void x32_f_residual_blk(X32<4>& x, const u16* w, const float* v, FB&& fblk, int lane, int h) {
  P32<8> op;
  make_op32(op, x);
  X32<4> y;
  lin32_pipe<8>(y, op, w, v, lane, h, [&](int b) {
    silu2_blk(y.v[b]);
    const R32<1> fr = fblk(b);
#pragma unroll
    for (int q = 0; q < 4; ++q) set_quad(x.v[b], q, unpack4(fr.u[q]) + silu2_unit<true>() * quad(y.v[b], q));
  });
  pin(x);
}

// ---- the node layer's attention aggregation folded into the edge layer (di_edge_layer_attn)
// h_attn[v] = sum_{e in in(v)} alpha[e, head] * V[src e] / (sum_e alpha[e, head] + 1e-6)
// (send_and_recv(u_mul_e('V_h','score'), sum), (copy_e('score'), sum), wV / (z + 1e-6):
// deepinteract_modules.py:93-96, 116). Edges are destination-major, so a destination's in-edges are
// consecutive rows: a wave's 32 rows hold whole destinations plus at most one continuing from the
// previous 32-row tile and one continuing into the next. Each lane forms alpha * V[src] for its row
// (the 64 features of its lane half, in the accumulator quads) and alpha itself; a segmented
// inclusive scan over the 32 rows -- DPP row shifts by 1, 2, 4, 8 inside each 16-lane row, then the
// first row's last lane broadcast into the second -- leaves every destination's sums in the lane of
// its last row here. That lane writes attn[v] = wV / (z + 1e-6) when all of v's in-edges are in this
// tile, else the partial sums to attn_parts[tile][slot] (slot 1: v continues into the next tile;
// slot 0: v continues from the previous one); attn_row (the node update) adds a split
// destination's partials. Summation order: a tree over each tile's rows, then tile by tile.
// (FOLD_ROWS / FOLD_PART, a tile's rows and a partial's floats: geot.h)

// one scan step: lanes whose DPP source row has the same destination add its sums
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void fold_step(X32<4>& s, floatx4& z, int d) {
  const bool same = __builtin_amdgcn_update_dpp(-2, d, CTRL, ROW_MASK, 0xf, false) == d;
  auto mv = [](float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, ROW_MASK, 0xf,
                                                                  false));
  };
#pragma unroll
  for (int b = 0; b < 4; ++b) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const float t = mv(s.v[b][k]);
      s.v[b][k] += same ? t : 0.f;
    }
    const float t = mv(z[b]);
    z[b] += same ? t : 0.f;
  }
}

// d: the row's destination, vr: its V[src] row, ip: in_ptr[d], in_ptr[d + 1] (loaded with K / Q)
__device__ __forceinline__ void edge_attn_fold(const EdgeArgs& a, int e, bool valid, int lane, int h, floatx4 al,
                                               int d, const R32<4>& vr, int2 ip) {
  if (!valid) {  // rows past the end: their own (empty) segment
    d = -1;
    al = (floatx4){0.f, 0.f, 0.f, 0.f};
  }
  X32<4> s;
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int q = 0; q < 4; ++q) set_quad(s.v[b], q, al[b] * unpack4(vr.u[4 * b + q]));
  floatx4 z = al;
  fold_step<0x111, 0xf>(s, z, d);  // row_shr:1
  fold_step<0x112, 0xf>(s, z, d);  // row_shr:2
  fold_step<0x114, 0xf>(s, z, d);  // row_shr:4
  fold_step<0x118, 0xf>(s, z, d);  // row_shr:8
  fold_step<0x142, 0xa>(s, z, d);  // row_bcast:15 into rows 1 and 3 (each lane half's second 16 rows)
  const int dnext = __shfl_down(d, 1, 32);
  if (!valid || ((lane & 31) != 31 && dnext == d)) return;
  const int t = e / FOLD_ROWS, t0 = ip.x / FOLD_ROWS, t1 = (ip.y - 1) / FOLD_ROWS;
  if (t0 == t1) {
    float* row = a.attn_out + (int64_t)d * HID;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const float den = z[b] + 1e-6f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const floatx4 x = quad(s.v[b], q);
        st4(row + 32 * b + 8 * q + 4 * h, (floatx4){x[0] / den, x[1] / den, x[2] / den, x[3] / den});
      }
    }
  } else {
    float* p = a.attn_parts + ((int64_t)t * 2 + (t == t0 ? 1 : 0)) * FOLD_PART;
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) st4(p + 32 * b + 8 * q + 4 * h, quad(s.v[b], q));
    if (h == 0) st4(p + HID, z);
  }
}

// One 32-row tile per wave through the whole edge layer: the stage sequence `st` (the 8-wave ring's
// RingStages) hands out each weight stage in order (next(): its weights, v(): its bias).
// Z0 (layer 0 after k_init_x32<true, true>): a.f_in holds z0 rows (mfma32.h) and wc2 the 8 packed
// blocks of InitEdge's combined_linear_2 in LDS. The row's z0 operand stays in 8 registers for the
// whole tile and each 32-feature block of F0 is rebuilt from it where F is used (f0_blk: the MFMAs
// and the rounding InitEdge applies), one block live at a time, instead of four reads of the F row.
template <int MODE, bool GC, bool Z0, class ST>
__device__ __forceinline__ void edge_x32_tile(const EdgeArgs& a, ST& st, int e, bool valid, int lane, int h,
                                              const u16* wc2) {
  constexpr bool FINAL = MODE == 1;
  static_assert(!Z0 || (GC && !FINAL), "the z0 form is the non-final DI_GRAPH_GEO_REF layer 0");
  // the lane half is opaque per tile: the bf16 rows' 16-B accesses and the fp32 rows share the byte
  // offset 16 h, and the compiler otherwise keeps (array base + 16 h) of every array in a register
  // pair across the block's tile loop -- past the 240 cap in the <0, true, false> form (scratch)
  asm volatile("" : "+v"(h));
  const u16* f_row = reinterpret_cast<const u16*>(a.f_in) + (int64_t)e * HID;
  const u16* qkv = reinterpret_cast<const u16*>(a.qkv);

  // the edge's geometric features [28] (fp32 row) as a 32-feature operand, features 28..31 = 0
  P32<2> gop;
  {
    const float* grow = a.edge_f + (int64_t)e * NFEAT_E;
    X32<1> geo;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int f = 8 * q + 4 * h;
      set_quad(geo.v[0], q, f < NFEAT_E ? ld4(grow + f) : (floatx4){0.f, 0.f, 0.f, 0.f});
    }
    make_op32(gop, geo);
  }
  X32<4> x;
  R32<4> fr;  // the edge's own row F, re-read (L2) before each use: the stages have no room to hold it
  P32<2> zop;  // Z0: the row's z0 operand instead
  auto f0 = [&](int b) { return f0_blk(wc2, zop, b, lane); };
  (void)f0;
  const u16* w;
  if constexpr (Z0) {
    load_z0(zop, reinterpret_cast<const u16*>(a.f_in), e, h);
    w = st.next([&] { asm volatile("" ::"v"(zop.f[0]), "v"(zop.f[1])); });  // orig_msg_linear (+ its bias)
    init_vec32_lds(x, st.v(), h);
  } else if constexpr (GC) {
    // DI_GRAPH_GEO_REF: the neighbour messages are multiplied by dir_linear_1(dir_linear_0(0)) = 0
    // (:408), so x = orig_msg_linear(F) + b exactly; no gathered rows, no stages 0-1
    fr.load(f_row, h);
    w = st.next([&] { settle(fr); });  // orig_msg_linear (+ its bias)
    init_vec32_lds(x, st.v(), h);
  } else {
    // ---- neighbour-edge messages (conformation_module_message_func :384-418)
    const u16* fn_in = reinterpret_cast<const u16*>(a.fn_in);
    const int4 nb = *reinterpret_cast<const int4*>(a.nbr + (int64_t)e * 4);
    R32<4> xn;  // the gathered silu(nbr_linear(F)) row in flight
    xn.load(fn_in + (int64_t)nb.x * HID, h);
    w = st.next();  // stage 0: geometric gates (dist [4x2] blocks 0-7, dir / orient / amide [2x2] at 8 / 12 / 16)
                    // + downward_proj [2x8] at 20
    X32<2> gate;
    {
      X32<2> t1;
      zero(gate);
      mma32<2, 2>(gate, gop, w + 8 * BLK, lane);
      zero(t1);
      mma32<2, 2>(t1, gop, w + 12 * BLK, lane);
#pragma unroll
      for (int b = 0; b < 2; ++b) gate.v[b] *= t1.v[b];
      zero(t1);
      mma32<2, 2>(t1, gop, w + 16 * BLK, lane);
#pragma unroll
      for (int b = 0; b < 2; ++b) gate.v[b] *= t1.v[b];
      pin(gate);
    }
    X32<2> s;
    zero(s);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      // x = silu(nbr_linear(F))[nbr_j] * dist gate, packed block by block (the dist gate recomputed
      // per neighbour: 2 MFMAs per block instead of 64 live registers)
      P32<8> xop;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        asm volatile("" ::: "memory");
        xn.unswz_blk(b);  // no settle for the gathered row: block by block at its use, as its waits
        floatx16 dg = {};
        dg = mfma32(afrag(w, 2 * b, lane), gop.f[0], dg);
        dg = mfma32(afrag(w, 2 * b + 1, lane), gop.f[1], dg);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          asm volatile("" : "+v"(xn.u[4 * b + 2 * t]), "+v"(xn.u[4 * b + 2 * t + 1]));
          const floatx4 lo = unpack4(xn.u[4 * b + 2 * t]) * quad(dg, 2 * t);
          const floatx4 hi = unpack4(xn.u[4 * b + 2 * t + 1]) * quad(dg, 2 * t + 1);
          const uint4 u = {pack_bf16x2(lo[0], lo[1]), pack_bf16x2(lo[2], lo[3]), pack_bf16x2(hi[0], hi[1]),
                           pack_bf16x2(hi[2], hi[3])};
          xop.f[2 * b + t] = __builtin_bit_cast(bf16x8, u);
        }
      }
      if (j < 3) {  // the next gathered row, in flight under this one's downward_proj
        const int nx = j == 0 ? nb.y : (j == 1 ? nb.z : nb.w);
        xn.load(fn_in + (int64_t)nx * HID, h);
      }
      X32<2> y;
      zero(y);
      mma32<2, 8>(y, xop, w + 20 * BLK, lane);  // downward_proj
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int k = 0; k < 16; ++k) s.v[b][k] += silu2<true>(y.v[b][k]) * gate.v[b][k];
      pin(s);
    }
    w = st.next();  // stage 1: upward_proj [4x4] (+ orig_msg_linear bias)
    {
      P32<4> sop;
      make_op32(sop, s);
      zero(x);
      mma32<4, 4>(x, sop, w, lane);
      X32<4> bo;
      init_vec32_lds(bo, st.v(), h);
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        silu2_blk(x.v[b]);
        x.v[b] = silu2_unit<true>() * x.v[b] + bo.v[b];
      }
      pin(x);
    }
    fr.load(f_row, h);
    w = st.next([&] { settle(fr); });  // stage 2: orig_msg_linear(res) + nbr
  }
  {
    P32<8> fop;
    if constexpr (Z0) {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        lean_fence();  // block by block: one rebuilt block live at a time
        P32<2> o;
        raw_op32(o, f0(b));
        fop.f[2 * b] = o.f[0];
        fop.f[2 * b + 1] = o.f[1];
        asm volatile("" : "+v"(fop.f[2 * b]), "+v"(fop.f[2 * b + 1]));
      }
    } else {
      raw_op32(fop, fr);
    }
    mma32<4, 8>(x, fop, w, lane);
    pin(x);
  }
  x32_res_block(x, st, lane, h);
  x32_res_block(x, st, lane, h);
  // F rows are loaded BEFORE the stage's barrier and DMA issue: vmcnt retires in order, so a load
  // issued after the stage's LDS-DMA pieces would make its use wait for the whole weight stage
  if constexpr (!Z0) fr.load(f_row, h);
  w = st.next([&] { if constexpr (!Z0) settle(fr); });  // res_connect_linear: x = F + silu(rc(x))
  if constexpr (Z0) x32_f_residual_blk(x, w, st.v(), f0, lane, h);
  else x32_f_residual(x, w, st.v(), fr, lane, h);
  x32_res_block(x, st, lane, h);
  x32_res_block(x, st, lane, h);
  w = st.next();  // final geometric gate [4x2]
  {
    X32<4> fg;
    zero(fg);
    mma32<4, 2>(fg, gop, w, lane);
#pragma unroll
    for (int b = 0; b < 4; ++b) x.v[b] *= fg.v[b];
    pin(x);
  }
  if constexpr (!Z0) fr.load(f_row, h);
  w = st.next([&] { if constexpr (!Z0) settle(fr); });  // final_linear: x = F + silu(final(x)) = conformation output
  if constexpr (Z0) x32_f_residual_blk(x, w, st.v(), f0, lane, h);
  else x32_f_residual(x, w, st.v(), fr, lane, h);

  // ---- attention scores (propagate_attention :76-91): head hd = features 32 hd .. 32 hd + 31 = block hd
  R32<4> kr, qr;  // K[src], Q[dst], issued before the stage barrier
  const int sn = a.src[e], dn = a.dst[e];
  kr.load(qkv + (int64_t)sn * 3 * HID + HID, h);
  qr.load(qkv + (int64_t)dn * 3 * HID, h);
  // the fold's V[src] row and the destination's in-edge range, in flight with K / Q (GEO_REF kernels;
  // the general path's extra live rows leave no room: loaded at the fold)
  const bool fold = !Z0 && a.attn_out != nullptr;  // uniform (there is no fold form of the z0 layer)
  R32<4> vr;
  int2 ip = {0, 0};
  auto fold_loads = [&] {
    vr.load(qkv + (int64_t)sn * 3 * HID + 2 * HID, h);
    ip = *reinterpret_cast<const int2*>(a.in_ptr + dn);
  };
  if (GC && fold) fold_loads();
  w = st.next([&] {
    settle(kr);
    settle(qr);
    if (GC && fold) {
      settle(vr);
      asm volatile("" ::"v"(ip.x), "v"(ip.y));
    }
  });  // edge_feats_projection(BN1e(conf))
  X32<4> p;
  {
    P32<8> xop;
    make_op32(xop, x);
    init_vec32_lds(p, st.v(), h);
    mma32<4, 8>(p, xop, w, lane);
  }
  floatx4 al;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const floatx4 kq = unpack4(kr.u[4 * b + q]), qd = unpack4(qr.u[4 * b + q]);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float sc = (kq[i] * qd[i]) * (1.0f / 5.656854249492381f);  // / np.sqrt(32)
        sc = fminf(fmaxf(sc, -5.f), 5.f);
        const float pv = sc * p.v[b][4 * q + i];  // score = e_out
        p.v[b][4 * q + i] = pv;
        sum += pv;
      }
    }
    sum += __shfl_xor(sum, 32);  // the head's other 16 features: the same row in the other lane half
    al[b] = expf_<true>(fminf(fmaxf(sum, -5.f), 5.f));
  }
  if (valid && h == 0 && a.alpha_out != nullptr) st4(a.alpha_out + (int64_t)e * 4, al);
  if (!GC && fold) fold_loads();
  // the general path's V row has no settle(): its layout is restored at the fold, its first use
  auto attn_fold = [&] {
    if (!GC) vr.unswz();
    edge_attn_fold(a, e, valid, lane, h, al, dn, vr, ip);
  };
  if constexpr (FINAL) {
    if (fold) attn_fold();
  } else {
    // ---- edge output: e = in + O_e(e_out); e = e + FFN(BN2e(e)) (:697-724)
    P32<8> pop;
    make_op32(pop, p);
    pin(pop);
    if (fold) attn_fold();  // p is packed: room for the scan
    if constexpr (!Z0) fr.load(f_row, h);                    // O_edge: re-read
    w = st.next([&] { if constexpr (!Z0) settle(fr); });  // O_edge_feats
    X32<4> e1;
    init_vec32_lds(e1, st.v(), h);
    mma32<4, 8>(e1, pop, w, lane);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      R32<1> fb;
      if constexpr (Z0) {
        lean_fence();
        fb = f0(b);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) fb.u[q] = fr.u[4 * b + q];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) set_quad(e1.v[b], q, quad(e1.v[b], q) + unpack4(fb.u[q]));
    }
    pin(e1);
    P32<8> eop;
    make_op32(eop, e1);
    pin(eop);
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
      w = st.next();  // edge_feats_MLP.0 (BN2e folded), hidden half
      X32<4> t;
      P32<8> top;
      lin32_pipe<8>(t, eop, w, st.v(), lane, h, [&](int b) {
        silu2_blk(t.v[b]);
        pack_blk(top.f[2 * b], top.f[2 * b + 1], t.v[b]);
      });
      pin(top);
      w = st.next();  // edge_feats_MLP.3, input half: accumulated into the residual
      mma32<4, 8>(e1, top, w, lane);
      pin(e1);
    }
    store_row32(e1, reinterpret_cast<u16*>(a.f_out) + (int64_t)e * HID, h, valid);
    if constexpr (GC) return;  // the next layer gathers no silu(nbr_linear(F)) rows
    make_op32(eop, e1);
    w = st.next();  // next layer's silu(nbr_linear(.))
    X32<4> fn;
    init_vec32_lds(fn, st.v(), h);
    mma32<4, 8>(fn, eop, w, lane);
#pragma unroll
    for (int b = 0; b < 4; ++b) silu_blk(fn.v[b]);
    store_row32(fn, reinterpret_cast<u16*>(a.fn_out) + (int64_t)e * HID, h, valid);
  }
}

// ================================================================ the bf16 edge layers on an 8-wave weight ring
// One persistent 8-wave block per CU (2 waves per SIMD, <= 240 VGPRs), a 4-slot ring of
// 36-block weight stages in LDS (150 KB): every stage is DMA'd ONCE per 256 edges (8 waves x 32 rows)
// instead of once per 128 -- half the L2 -> LDS weight stream of round 4's two 4-wave blocks per CU,
// the traffic that competes with the pair-tensor stores beside it -- and there is no
// block-wide barrier per stage. Per slot two LDS counters, both monotonic: FULL counts publications of
// the slot's stages (the owner waits its vmcnt, then adds), FREE the waves done reading it. A wave entering global stage g (stages run on across the block's tiles, so the
// next tile's first stages are in flight under the current tile's last ones):
//   releases stage g - 1 (FREE += 1); if it owns a stage it issued earlier (stage s is loaded by wave
//   s % 8), waits for its own loads (vmcnt(0)) and publishes it (FULL += 1); if it owns stage g + 2,
//   issues it into the slot of stage g - 2 once all 8 waves have released that one; then waits until
//   stage g is published. No block-wide barrier: a wave waits only for the owner of the stage it needs
//   and, once in 8 stages, for the slowest wave two stages back.
constexpr int RING_NW = 8, RING_SLOTS = 4, RING_AHEAD = 2;
using RingSlot = WPipe<u16, RING_NW, true, EL_CAP, 128>;  // slot geometry only (SLOT_BYTES)
struct EdgeRingGeo {
  static constexpr int NW = RING_NW, THREADS = 64 * NW, ROWS_PER_WAVE = 32, ROWS = ROWS_PER_WAVE * NW;
};
static_assert(EdgeRingGeo::ROWS_PER_WAVE == FOLD_ROWS, "a fold tile is one wave's rows");

// The ring's LDS counters are read and added with explicit ds_ instructions: through C++ atomics the
// compiler cannot tell them from the weight slots the in-flight LDS-DMA writes and puts an
// s_waitcnt vmcnt(0) in front of every poll, which would drain the prefetch at every stage.
__device__ __forceinline__ uint32_t lds_off(const uint32_t* p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint32_t*)p;
}
__device__ __forceinline__ uint32_t lds_ld(const uint32_t* p) {
  uint32_t v;
  asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(lds_off(p)) : "memory");
  return v;
}
// +1 per WAVE (one lane; LDS operations of a wave execute in order, so the add follows the wave's
// earlier reads of the slot)
__device__ __forceinline__ void lds_add(uint32_t* p) {
  asm volatile(
      "s_mov_b64 s[0:1], exec\n\t"
      "s_mov_b64 exec, 1\n\t"
      "ds_add_u32 %0, %1\n\t"
      "s_mov_b64 exec, s[0:1]" ::"v"(lds_off(p)), "v"(1u)
      : "memory", "s0", "s1");
}
// spin until *p >= v (s_sleep between LDS polls)
__device__ __forceinline__ void lds_wait_ge(const uint32_t* p, uint32_t v) {
  while (lds_ld(p) < v) __builtin_amdgcn_s_sleep(1);
}

// raw buffer descriptor (as buf_rsrc: stride 0, num_records 0x7fffffff, DATA_FORMAT 32) in SGPRs
typedef uint32_t rsrc4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ rsrc4 rsrc_of(const void* p) {
  const uint64_t a = (uint64_t)(uintptr_t)p;
  return (rsrc4){(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a),
                 (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32)) & 0xffffu, 0x7fffffffu,
                 (uint32_t)BUF_RSRC_W3};
}
// one 1-KiB LDS-DMA piece: 16 B per lane from rsrc + voff + soff to LDS byte address lds + 16 * lane
__device__ __forceinline__ void dma_piece(rsrc4 r, uint32_t lds, int voff, int soff) {
  asm volatile(
      "s_mov_b32 m0, %0\n\t"
      "s_nop 0\n\t"
      "buffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(__builtin_amdgcn_readfirstlane((int)lds)),
      "v"(voff), "s"(r), "s"(__builtin_amdgcn_readfirstlane(soff))
      : "memory", "m0");
}

// The bf16 edge layer's stage sequence on the ring. One stage is one run of packed 512-element blocks
// of the layer's blob (EL_ORDER / EL_SIZE: first block, block count) and an optional bias vector
// (EL_VEC: 128 floats, after the slot's blocks); global stage gs is stage gs % NS of the layer.
// GC: as EdgeStages, the sequence starts at orig_msg_linear, which then carries ELV_OM.
template <int NS, bool GC>
struct RingStages {
  char* base;          // RING_SLOTS x RingSlot::SLOT_BYTES
  uint32_t* full;      // [RING_SLOTS]: stage uses published (1 per use)
  uint32_t* freec;     // [RING_SLOTS]: wave releases (RING_NW per use)
  const u16* W;        // the layer's weight blob
  const float* V;      // its bias vectors
  int wave;
  int total;           // global stages of this block
  int g = 0;           // next stage to consume
  int issued = 0;      // stages [0, issued) are issued (by their owners)
  int pending = -1;    // a stage this wave issued and has not published yet
  int cur = 0;         // slot of the stage being consumed
  __device__ u16* slot_w(int sl) const { return reinterpret_cast<u16*>(base + sl * RingSlot::SLOT_BYTES); }
  __device__ float* slot_v(int sl) const {
    return reinterpret_cast<float*>(base + sl * RingSlot::SLOT_BYTES + EL_CAP * BLK * 2);
  }
  // global stage gs is loaded and published by ONE wave, gs % RING_NW (its owner): all its 1-KiB
  // LDS-DMA pieces and the bias vector. Issued by inline asm: the compiler's waitcnt pass cannot tell a
  // ring slot (runtime index) from the one being read and would wait for every piece before the next
  // ds_read -- completion is what FULL tracks (the owner's vmcnt(0), then its publish).
  __device__ void issue_one(int gs) {
    const int s = gs % NS;
    const int si = GC ? s + 2 : s;
    const int vo = (GC && s == 0) ? ELV_OM : EL_VEC[si];
    const int off = EL_ORDER[si], n = EL_SIZE[si];  // the stage's run: first block, block count
    const float* v = vo >= 0 ? V + vo : nullptr;    // its bias vector
    const int sl = gs % RING_SLOTS;
    const uint32_t dst = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)slot_w(sl);
    const int loff = (threadIdx.x & 63) * 16;
    const rsrc4 r = rsrc_of(W + off * BLK);
    for (int i = 0; i < n; ++i) dma_piece(r, dst + i * 1024, loff, i * 1024);  // 1 KiB per block
    if (v && (threadIdx.x & 63) < 32)
      dma_piece(rsrc_of(v), (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)slot_v(sl), loff, 0);
    pending = gs;
  }
  // stages issued ahead of the one consumed, owners' slots permitting
  __device__ void issue_ahead() {
    for (; issued <= g + RING_AHEAD && issued < total; ++issued) {
      if (issued % RING_NW != wave) continue;
      const int prev = issued - RING_SLOTS;  // the stage that used this slot last
      if (prev >= 0) lds_wait_ge(freec + issued % RING_SLOTS, (uint32_t)(RING_NW * (prev / RING_SLOTS + 1)));
      issue_one(issued);
    }
  }
  __device__ void fill() {
    for (; issued < RING_AHEAD && issued < total; ++issued)
      if (issued % RING_NW == wave) issue_one(issued);
  }
  // settle(): an empty asm reading the rows the caller loaded just before this call (F rows, K / Q):
  // the compiler then waits for them HERE, after the vmcnt(0) that has landed them anyway -- not after
  // the asm-issued DMA below, which it cannot see and would otherwise wait for at their first use
  template <class F>
  __device__ const u16* next(F&& settle) {
    asm volatile("" ::: "memory");
    if (g > 0) lds_add(freec + (g - 1) % RING_SLOTS);  // done reading stage g - 1 (its reads are in order before)
    lds_dma_wait();  // this wave's loads (rows, and the pieces of a stage it owns) have landed
    settle();
    if (pending >= 0) {
      lds_add(full + pending % RING_SLOTS);
      pending = -1;
    }
    issue_ahead();
    lds_wait_ge(full + g % RING_SLOTS, (uint32_t)(g / RING_SLOTS + 1));
    asm volatile("" ::: "memory");
    cur = g % RING_SLOTS;
    ++g;
    return slot_w(cur);
  }
  __device__ const u16* next() {
    return next([] {});
  }
  __device__ const float* v() const { return slot_v(cur); }
};

// Z0 (di_edge_layer_z): layer 0 on z0 rows; InitEdge's combined_linear_2 (8 packed blocks, 8 KiB of
// the kind-1 blob at IE_C1 + 8) stays in LDS beside the ring for the block's lifetime
constexpr int Z0_WC2_BLOCKS = 8;
static_assert(RING_SLOTS * RingSlot::SLOT_BYTES + 2 * RING_SLOTS * (int)sizeof(uint32_t) + Z0_WC2_BLOCKS * BLK * 2 <=
                  160 * 1024,
              "ring slots + counters + combined_linear_2 fit the CU's LDS (the pair stream uses none)");
static_assert(Z0_WC2_BLOCKS == RING_NW, "one 1-KiB LDS-DMA piece of combined_linear_2 per wave");
template <int MODE, bool GC, bool Z0 = false>
__global__ __attribute__((amdgpu_flat_work_group_size(1, EdgeRingGeo::THREADS), amdgpu_waves_per_eu(2, 2),
                          amdgpu_num_vgpr(120)))
void k_edge_x32_ring(EdgeArgs a, int ntiles) {
  constexpr bool FINAL = MODE == 1;
  constexpr int NS = (FINAL ? EL_NSTAGE_FINAL : EL_NSTAGE) - (GC ? (FINAL ? 2 : 3) : 0);
  __shared__ __attribute__((aligned(16))) char lds[RING_SLOTS * RingSlot::SLOT_BYTES];
  __shared__ uint32_t counters[2 * RING_SLOTS];
  const int lane = lane_id(), h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int my_tiles = ((int)blockIdx.x < ntiles) ? (ntiles - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;
  if (threadIdx.x < 2 * RING_SLOTS) counters[threadIdx.x] = 0;
  const u16* wc2 = nullptr;
  if constexpr (Z0) {
    __shared__ __attribute__((aligned(16))) u16 wc2_lds[Z0_WC2_BLOCKS * BLK];
    dma_piece(rsrc_of(reinterpret_cast<const u16*>(a.init_wmat) + (IE_C1 + 8) * BLK),
              (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)wc2_lds + wave * 1024, lane * 16,
              wave * 1024);
    lds_dma_wait();  // the barrier below does not wait for LDS-DMA
    wc2 = wc2_lds;
  }
  __syncthreads();
  RingStages<NS, GC> st{lds, counters, counters + RING_SLOTS, reinterpret_cast<const u16*>(a.wmat), a.wvec, wave,
                        my_tiles * NS};
  st.fill();
#pragma unroll 1
  for (int i = 0; i < my_tiles; ++i) {
    // slot j = b + i G: with G a multiple of 8, slot j runs on block b's XCD (j mod 8), and
    // xcd_slot gives each XCD one contiguous eighth of the edges (every block keeps its tile count)
    const int j = (int)blockIdx.x + i * (int)gridDim.x;
    const int tile = (gridDim.x & 7) == 0 ? xcd_slot(j, ntiles) : j;
    const int r = tile * EdgeRingGeo::ROWS + wave * EdgeRingGeo::ROWS_PER_WAVE + (lane & 31);
    const bool valid = r < a.Et;
    const int e = valid ? r : a.Et - 1;
    edge_x32_tile<MODE, GC, Z0>(a, st, e, valid, lane, h, wc2);
  }
}

}  // namespace di

// ================================================================ C ABI
using namespace di;

// persistent 8-wave blocks on the weight ring, one per CU (k_edge_x32_ring)
template <int MODE, bool GC, bool Z0 = false>
static void launch_edge_ring(EdgeArgs a, hipStream_t s) {
  const PersistentGrid p = persistent_grid(a.Et, EdgeRingGeo::ROWS);
  hipLaunchKernelGGL((k_edge_x32_ring<MODE, GC, Z0>), p.grid, dim3(EdgeRingGeo::THREADS), 0, s, a, p.ntiles);
}

static int edge_layer(const di_graph* g, di_dtype dt, int final_layer, const float* edge_f, const void* f_in,
                      const void* fn_in, const void* qkv, const void* wmat, const float* wvec, float* alpha_out,
                      void* f_out, void* fn_out, float* attn_out, float* attn_parts, void* stream) {
  // DI_GRAPH_GEO_REF: the neighbour-message branch is skipped (exactly zero), fn_in is not read and
  // fn_out not written (every edge-layer kernel; di_conformation computes the branch)
  const bool gc = g && (g->flags & DI_GRAPH_GEO_REF);
  const bool fold = attn_out != nullptr;
  if (!g || !edge_f || !f_in || (!fn_in && !gc) || !qkv || !wmat || !wvec || (!alpha_out && !fold) ||
      g->num_edges <= 0 || !dtype_ok(dt))
    return DI_EINVAL;
  if (fold && (dt != DI_BF16 || !attn_parts || !g->in_ptr || !g->src || !g->dst)) return DI_EINVAL;
  if (!final_layer && (!f_out || (!fn_out && !gc))) return DI_EINVAL;
  EdgeArgs a{g->num_edges, edge_f, g->src, g->dst, g->nbr, f_in, fn_in, qkv, wmat, wvec, alpha_out,
             f_out, fn_out, attn_out, attn_parts, g->in_ptr};
  hipStream_t s = (hipStream_t)stream;
  if (dt == DI_BF16) {
    if (final_layer && gc) launch_edge_ring<1, true>(a, s);
    else if (final_layer) launch_edge_ring<1, false>(a, s);
    else if (gc) launch_edge_ring<0, true>(a, s);
    else launch_edge_ring<0, false>(a, s);
  } else {
    const dim3 grid = grid_of<Geo<F32T>>(a.Et), block = block_of<Geo<F32T>>();
    if (final_layer && gc) hipLaunchKernelGGL((k_edge_layer<F32T, 1, true>), grid, block, 0, s, a);
    else if (final_layer) hipLaunchKernelGGL((k_edge_layer<F32T, 1>), grid, block, 0, s, a);
    else if (gc) hipLaunchKernelGGL((k_edge_layer<F32T, 0, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_edge_layer<F32T, 0>), grid, block, 0, s, a);
  }
  return launch_status();
}

extern "C" int di_edge_layer(const di_graph* g, di_dtype dt, int final_layer, const float* edge_f,
                             const void* f_in, const void* fn_in, const void* qkv, const void* wmat,
                             const float* wvec, float* alpha_out, void* f_out, void* fn_out,
                             void* stream) {
  return edge_layer(g, dt, final_layer, edge_f, f_in, fn_in, qkv, wmat, wvec, alpha_out, f_out, fn_out, nullptr,
                    nullptr, stream);
}

extern "C" int di_edge_layer_z(const di_graph* g, di_dtype dt, const float* edge_f, const void* z_in,
                               const void* init_wmat, const void* qkv, const void* wmat, const float* wvec,
                               float* alpha_out, void* f_out, void* stream) {
  // the non-final bf16 DI_GRAPH_GEO_REF layer 0 of edge_layer(), F0 rebuilt from z0 rows
  if (!g || !(g->flags & DI_GRAPH_GEO_REF) || !edge_f || !z_in || !init_wmat || !qkv || !wmat || !wvec || !f_out ||
      !g->src || !g->dst || g->num_edges <= 0 || dt != DI_BF16)
    return DI_EINVAL;
  EdgeArgs a{g->num_edges, edge_f, g->src, g->dst, g->nbr, z_in, nullptr, qkv, wmat, wvec, alpha_out,
             f_out, nullptr, nullptr, nullptr, g->in_ptr, init_wmat};
  launch_edge_ring<0, true, true>(a, (hipStream_t)stream);
  return launch_status();
}

extern "C" int64_t di_attn_parts_bytes(int32_t num_edges) {
  if (num_edges <= 0) return DI_EINVAL;
  return (int64_t)((num_edges + FOLD_ROWS - 1) / FOLD_ROWS) * 2 * FOLD_PART * (int64_t)sizeof(float);
}

extern "C" int di_edge_layer_attn(const di_graph* g, di_dtype dt, int final_layer, const float* edge_f,
                                  const void* f_in, const void* fn_in, const void* qkv, const void* wmat,
                                  const float* wvec, float* alpha_out, void* f_out, void* fn_out, float* attn_out,
                                  float* attn_parts, void* stream) {
  if (!attn_out) return DI_EINVAL;
  return edge_layer(g, dt, final_layer, edge_f, f_in, fn_in, qkv, wmat, wvec, alpha_out, f_out, fn_out, attn_out,
                    attn_parts, stream);
}

extern "C" int di_conformation(const di_graph* g, di_dtype dt, const float* edge_f, const void* f_in,
                               const void* fn_in, const void* wmat, const float* wvec, void* conf_out,
                               void* stream) {
  if (!g || !edge_f || !f_in || !fn_in || !wmat || !wvec || !conf_out || g->num_edges <= 0 || !dtype_ok(dt))
    return DI_EINVAL;
  EdgeArgs a{g->num_edges, edge_f, g->src, g->dst, g->nbr, f_in, fn_in, nullptr, wmat, wvec, nullptr,
             conf_out, nullptr};
  hipStream_t s = (hipStream_t)stream;
  if (dt == DI_BF16)
    hipLaunchKernelGGL((k_edge_layer<BF16T, 2>), grid_of<Geo<BF16T>>(a.Et), block_of<Geo<BF16T>>(), 0, s, a);
  else
    hipLaunchKernelGGL((k_edge_layer<F32T, 2>), grid_of<Geo<F32T>>(a.Et), block_of<Geo<F32T>>(), 0, s, a);
  return launch_status();
}
