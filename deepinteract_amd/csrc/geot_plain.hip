// GeoT with disable_geometric_mode: the plain Graph Transformer baseline's edge side (the node side is
// geot_node.hip's, unchanged). Reference semantics (project/utils/deepinteract_modules.py):
//   InitEdge          nn.Linear(30, H, bias=False) on cat(pos_enc, weight, edata['f'])        :1349-1351, :1444-1451
//   intermediate      no conformation module: BN1e / attention scores / O_edge / FFN on F     :584, :676, :697-724
//   final layer       nn.Linear(30, H, bias=False) on cat(F[:,0], F[:,1], orig edge feats),    :819-821, :897-904
//                     F the HIDDEN edge features by then (columns 0 / 1 of the previous layer's
//                     output, not the raw positional encoding and weight); then BN1e / scores
// Two kernels on common.h's 16x16 row-on-lane engine with Geo<DT>'s geometry (4-wave blocks, 64 rows,
// two blocks per CU), one tile per block: no persistent loop, no weight ring, no device-side wait, no
// inline assembly. Weight stages go through a WPipe of 32-block slots (bf16 double-buffered).
//
// k_edge_plain restates k_edge_layer's attention / FFN tail (geot_edge.hip, about 60 lines: score,
// clamp, alpha, O_edge + residual, the two FFN halves). That is the price of leaving k_edge_layer and
// k_edge_x32_ring untouched: neither can skip its conformation module, and the ring sits at 230-240
// VGPRs, a budget this mode is not worth putting at risk.
//
// Arithmetic: fp32 is k_edge_layer's (score / sqrt(32), expf, common.h's SiLU), so a DI_F32_FAST_SILU=0
// build follows. bf16 takes the ring kernel's reciprocal scale and __expf; its SiLU is common.h's plain
// hardware form -- the blobs carry no log2-unit scaling in either dtype (packing.edge_blob_plain).
// Host folds (packing.py): InitEdge's doubled columns 0 / 1 added into one [128, 28 -> 32] map; the
// final layer's W_c reordered to the operand [G (28), F[:,0], F[:,1], 0, 0]; BN1e / BN2e folded.
#include "geot.h"

namespace di {

struct PlainArgs {
  int Et;
  const float* edge_f;
  const int* src;
  const int* dst;
  const void* f_in;
  const void* qkv;
  const void* wmat;
  const float* wvec;
  float* alpha_out;
  void* f_out;
};

// F0 = W' . G: one K = 32 product per row (8 blocks, staged once per block)
template <class DT>
__global__ __attribute__((amdgpu_flat_work_group_size(1, Geo<DT>::THREADS)))
void k_init_plain(PlainArgs a) {
  using T = typename DT::T;
  using G = Geo<DT>;
  using Pipe = WPipe<T, G::NW, false, PI_NBLK>;
  __shared__ __attribute__((aligned(16))) char lds[Pipe::SLOT_BYTES];
  const int lane = lane_id(), g = lane >> 4;
  const int r = row_id<G::NW>();
  const bool valid = r < a.Et;
  const int e = valid ? r : a.Et - 1;
  Pipe pipe(lds);
  pipe.issue(reinterpret_cast<const T*>(a.wmat), PI_NBLK);
  Op<DT, 1> gop;
  {
    Act<2> geo;
    load_edge_geo(geo, a.edge_f + (int64_t)e * NFEAT_E, g);
    make_op(gop, geo);
  }
  const T* w = pipe.next();
  Act<8> x;
  zero(x);
  mma<8, 1>(x, gop, w, lane);
  if (valid) store_edge_row(x, reinterpret_cast<T*>(a.f_out) + (int64_t)e * HID, g);
}

template <class DT>
using PlainPipe = WPipe<typename DT::T, Geo<DT>::NW, Geo<DT>::DBUF, MAT128, 128>;

template <class DT, bool FINAL>
__global__ __attribute__((amdgpu_flat_work_group_size(1, Geo<DT>::THREADS), amdgpu_waves_per_eu(2, 2),
                          amdgpu_num_vgpr(120)))
void k_edge_plain(PlainArgs a) {
  using T = typename DT::T;
  using G = Geo<DT>;
  constexpr bool FAST = DT::kBF16;
  __shared__ __attribute__((aligned(16))) char lds[(G::DBUF ? 2 : 1) * PlainPipe<DT>::SLOT_BYTES];
  const int lane = lane_id(), g = lane >> 4;
  const int r = row_id<G::NW>();
  const bool valid = r < a.Et;
  const int e = valid ? r : a.Et - 1;  // tail rows recompute the last edge; their stores are guarded
  const T* W = reinterpret_cast<const T*>(a.wmat);
  const T* qkv = reinterpret_cast<const T*>(a.qkv);
  const T* f_row = reinterpret_cast<const T*>(a.f_in) + (int64_t)e * HID;

  PlainPipe<DT> pipe(lds);
  // a stage: `n` blocks at block offset `off`, with the 128-float bias at `vo` (-1: none)
  auto issue = [&](int off, int n, int vo) { pipe.issue(W + off * BLK, n, vo >= 0 ? a.wvec + vo : nullptr, 128); };
  const T* w;
  Act<8> x;  // the projection's input: F, or the final layer's 30-wide product
  if constexpr (FINAL) {
    issue(PF_WC, 8, -1);
    Op<DT, 1> cop;
    {
      // [G (28), F[e,0], F[e,1], 0, 0]: features 28 / 29 are registers 0 / 1 of block 1 in lane group 3
      Act<2> c;
      load_edge_geo(c, a.edge_f + (int64_t)e * NFEAT_E, g);
      Act<1> f01;
      load_row(f01, f_row, 0);  // hidden columns 0 .. 3 of the row
      if (g == 3) {
        c.v[1][0] = f01.v[0][0];
        c.v[1][1] = f01.v[0][1];
      }
      make_op(cop, c);
    }
    w = pipe.next();  // W_c
    issue(PF_P, MAT128, PFV_P);
    zero(x);
    mma<8, 1>(x, cop, w, lane);
  } else {
    issue(PL_P, MAT128, PLV_P);
    load_row(x, f_row, g);
  }
  // ---- attention scores (propagate_attention :76-91), as k_edge_layer's tail
  const int sn = a.src[e], dn = a.dst[e];
  RawRow<T> kr, qr;  // K[src], Q[dst] in flight under the projection's MFMAs
  kr.load(qkv + (int64_t)sn * 3 * HID + HID, g);
  qr.load(qkv + (int64_t)dn * 3 * HID, g);
  w = pipe.next();  // edge_feats_projection(BN1e(.))
  if constexpr (!FINAL) issue(PL_OE, MAT128, PLV_OE);
  Act<8> p;
  init_vec_lds(p, pipe.v(), g);
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
        float sc = kq.v[b][q] * qd.v[b][q];
        sc = FAST ? sc * (1.0f / scale) : sc / scale;
        sc = fminf(fmaxf(sc, -5.f), 5.f);
        p.v[b][q] = sc * p.v[b][q];  // score = e_out
      }
  }
  floatx4 al;
#pragma unroll
  for (int h = 0; h < 4; ++h) al[h] = expf_<FAST>(fminf(fmaxf(head_sum(p, h), -5.f), 5.f));
  if (valid && g == 0) st4(a.alpha_out + (int64_t)e * 4, al);

  if constexpr (!FINAL) {
    // ---- edge output: e = in + O_e(e_out); e = e + FFN(BN2e(e)) (:697-724)
    w = pipe.next();  // O_edge_feats
    issue(PL_F1, MAT128, PLV_F1);
    Act<8> e1;
    init_vec_lds(e1, pipe.v(), g);
    linear<DT, 8, 4>(e1, p, w, lane);
    add_row(e1, f_row, g);  // the row again (L2) instead of 32 registers held across the projection
    Act<8> o;
    zero(o);
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
      w = pipe.next();  // edge_feats_MLP.0 (BN2e folded), hidden half
      issue(PL_F2 + half * MAT128, MAT128, -1);
      Act<8> t;
      init_vec_lds(t, pipe.v(), g);
      linear<DT, 8, 4>(t, e1, w, lane);
      silu_<8, FAST>(t);
      w = pipe.next();  // edge_feats_MLP.3, input half
      if (half == 0) issue(PL_F1 + MAT128, MAT128, PLV_F1 + 128);
      linear<DT, 8, 4>(o, t, w, lane);
    }
    add_(e1, o);
    if (valid) store_edge_row(e1, reinterpret_cast<T*>(a.f_out) + (int64_t)e * HID, g);
  }
}

}  // namespace di

// ================================================================ C ABI
using namespace di;

extern "C" int64_t di_plain_blob_bytes(int kind, di_dtype dtype, int vec) {
  if (!dtype_ok(dtype)) return -1;
  const int64_t esz = dtype == DI_BF16 ? 2 : 4;
  int64_t blk = 0, nvec = 0;
  switch (kind) {
    case 0: blk = PI_NBLK; nvec = 0; break;
    case 1: blk = PL_NBLK; nvec = PLV_N; break;
    case 2: blk = PF_NBLK; nvec = PFV_N; break;
    default: return -1;
  }
  return vec ? nvec * 4 : blk * BLK * esz;
}

extern "C" int di_init_edge_plain(const di_graph* g, di_dtype dt, const float* edge_f, const void* wmat, void* f_out,
                                  void* stream) {
  if (!g || !edge_f || !wmat || !f_out || g->num_edges <= 0 || !dtype_ok(dt)) return DI_EINVAL;
  PlainArgs a{g->num_edges, edge_f, nullptr, nullptr, nullptr, nullptr, wmat, nullptr, nullptr, f_out};
  hipStream_t s = (hipStream_t)stream;
  if (dt == DI_BF16)
    hipLaunchKernelGGL((k_init_plain<BF16T>), grid_of<Geo<BF16T>>(a.Et), block_of<Geo<BF16T>>(), 0, s, a);
  else
    hipLaunchKernelGGL((k_init_plain<F32T>), grid_of<Geo<F32T>>(a.Et), block_of<Geo<F32T>>(), 0, s, a);
  return launch_status();
}

extern "C" int di_edge_layer_plain(const di_graph* g, di_dtype dt, int final_layer, const float* edge_f,
                                   const void* f_in, const void* qkv, const void* wmat, const float* wvec,
                                   float* alpha_out, void* f_out, void* stream) {
  if (!g || !edge_f || !f_in || !qkv || !wmat || !wvec || !alpha_out || !g->src || !g->dst || g->num_edges <= 0 ||
      !dtype_ok(dt))
    return DI_EINVAL;
  if (!final_layer && !f_out) return DI_EINVAL;
  PlainArgs a{g->num_edges, edge_f, g->src, g->dst, f_in, qkv, wmat, wvec, alpha_out, f_out};
  hipStream_t s = (hipStream_t)stream;
  if (dt == DI_BF16) {
    const dim3 grid = grid_of<Geo<BF16T>>(a.Et), block = block_of<Geo<BF16T>>();
    if (final_layer) hipLaunchKernelGGL((k_edge_plain<BF16T, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_edge_plain<BF16T, false>), grid, block, 0, s, a);
  } else {
    const dim3 grid = grid_of<Geo<F32T>>(a.Et), block = block_of<Geo<F32T>>();
    if (final_layer) hipLaunchKernelGGL((k_edge_plain<F32T, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_edge_plain<F32T, false>), grid, block, 0, s, a);
  }
  return launch_status();
}
