/*
 * deepinteract_amd — C ABI of the MI355X (gfx950) GeoT hot path.
 *
 * Plain pointers and sizes only: every pointer argument is a DEVICE pointer unless stated;
 * every call is asynchronous on `stream` (a hipStream_t passed as void*); no call allocates
 * device memory; every call returns 0 or a hipError_t code (>0) or a negative DI_E* code.
 *
 * Each entry point replaces one piece of the reference's DGL/ATen hot path (file:line cited
 * relative to /root/reference/project/utils/):
 *
 *   di_node_embed   LitGINI.gnn_forward node_in_embedding            deepinteract_modules.py:1663-1664
 *                   + layer-0 Q/K/V of MultiHeadGeometricAttention   deepinteract_modules.py:101-103
 *   di_init_edge    InitEdgeModule.forward / message UDF             deepinteract_modules.py:198-264
 *   di_edge_layer   ConformationModule (:373-455) + attention edge UDFs (:76-91, graph_utils.py:21-63)
 *                   + O_edge/edge FFN of GeometricTransformerModule  deepinteract_modules.py:669-727
 *   di_node_layer   send_and_recv(u_mul_e/copy_e, sum) gSpMM         deepinteract_modules.py:93-96,116
 *   di_edge_layer_attn / di_node_update_folded: the same gSpMM folded into the edge layer (bf16)
 *                   + O_node / node FFN                               deepinteract_modules.py:696-723, 923-943
 *   di_pair_tensor  construct_interact_tensor (pad=False)            deepinteract_utils.py:158-172
 *   di_pair_stream / di_pair_help / di_pair_signal: the same, per micro-batch, as a device queue beside
 *                   the GeoT stream (lit_model_predict.py:236 calls it once per complex)
 *   di_head_prologue  ELU(inorm_1(conv2d_1(T))) of the head, T never materialised
 *                                                                    deepinteract_modules.py:1181-1184, 1228-1232
 *   di_inorm_elu    ELU(InstanceNorm2d(x)) of the head's ResNet blocks deepinteract_modules.py:1016-1030,1075-1095
 *   di_se_scale_add conv bias + SEBlock gate + residual add          deepinteract_modules.py:954-970, 1095
 *   di_channel_mean SEBlock squeeze (channel mean)                   deepinteract_modules.py:966
 *   di_head_body_batch  the head's two ResNets for a batch of complexes deepinteract_modules.py:1234-1241
 *   di_head_logits_batch  phase2_conv(ELU(x)) for the batch           deepinteract_modules.py:1241, 1247
 *   di_knn_topk     dgl.knn_graph + topk(pairwise_squared_distance)  graph_utils.py:107-108
 *   di_knn_graph    knn_graph's edge list / in-edge CSR (src, dst)   graph_utils.py:107, deepinteract_utils.py:442-443
 *   di_geo_feats    GeometricProteinFeatures('full') + edge/node feature assembly
 *                                                                    protein_feature_utils.py:322-377,
 *                                                                    deepinteract_utils.py:474-530
 *   di_build_nbr_ids  per-edge neighbour-edge ids                    deepinteract_utils.py:534-553
 *   di_build_nbr_ids_torch  the same, bit-exact with torch.randperm  deepinteract_utils.py:539-546
 *   di_contact_rank  LitGINI.test_step's softmax, ranking and counters deepinteract_modules.py:2018-2101,
 *                                                                    deepinteract_utils.py:977-995
 *   di_contact_auc   test_step's exact per-complex test_auroc / test_auprc (class 1)
 *                                                                    deepinteract_modules.py:2018-2101
 *   di_contact_rank_batch / di_contact_auc_batch  both over many complexes in one launch sequence
 *   di_examples_labels_batch / di_examples_gather_batch  a batch's example lists as label maps, or
 *                     as validation_step's pooled logits and labels  deepinteract_modules.py:1915-1982
 *   di_interface_labels_batch  a batch's label maps from the chains' heavy-atom coordinates
 *                     (what build_examples_tensor reads from pos_idx)  deepinteract_utils.py:567-582, 612
 *   di_residue_env_batch  a batch's structure-derived DIPS-Plus columns (residue one-hot, HSAAC, CN)
 *                     and amide normals from the chains' atoms        dips_plus_utils.py:84-161, 356-374
 *
 * Module-at-a-time entry points (deepinteract_amd/layers.py; same math as the fused kernels):
 *   di_conformation   ConformationModule.forward                      deepinteract_modules.py:373-455
 *   di_gemm_bias_act  nn.Linear (+ folded BatchNorm, + SiLU, + residual) of the GeoT modules
 *                                                                    deepinteract_modules.py:99-104, 696-723
 *   di_geo_attention  MultiHeadGeometricAttentionLayer.propagate_attention + h = wV/(z+1e-6)
 *                                                                    deepinteract_modules.py:76-121
 */
#ifndef DEEPINTERACT_AMD_H
#define DEEPINTERACT_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DI_ABI_VERSION 8

/* activation / weight storage type of the GeoT kernels (accumulation is always fp32). A plain
 * int32 (not a C enum type): a foreign caller may pass any value, and every entry point refuses
 * values other than DI_F32 / DI_BF16 with DI_EINVAL (a C++ enum holding 5 would be undefined
 * behaviour before the check could run; found by the host UBSan build). */
enum { DI_F32 = 0, DI_BF16 = 1 };
typedef int32_t di_dtype;

enum {
  DI_OK = 0,
  DI_EINVAL = -1,   /* bad shape / null pointer / unsupported config */
  DI_ERANGE = -2,   /* a size beyond the kernels' index range (see each entry point) */
};

/* A batch of residue graphs (one graph per chain, concatenated). Edges are destination-major:
 * the in-edges of node v are edge ids in_ptr[v] .. in_ptr[v+1]-1. All ids are GLOBAL to the batch. */
typedef struct {
  int32_t num_nodes;        /* Nt */
  int32_t num_edges;        /* Et */
  const int32_t* src;       /* [Et] source node of each edge */
  const int32_t* dst;       /* [Et] destination node of each edge */
  const int32_t* nbr;       /* [Et,4] src_nbr_e_ids[0:2], dst_nbr_e_ids[0:2] */
  const int32_t* node_pos;  /* [Nt] node index inside its chain (positional-embedding row) */
  const int32_t* in_ptr;    /* [Nt+1] CSR row pointer of in-edges by destination */
  int32_t flags;            /* DI_GRAPH_* properties of the batch's edge features (0: none known) */
} di_graph;

/* di_graph.flags bit: every edge's direction columns edge_f[:, 20:23] are 0 and its orientation
 * columns edge_f[:, 23:27] are (0, 0, 0, 1) -- what the reference featuriser produces for every
 * kNN graph (GeometricProteinFeatures is called with E_idx = the destination node itself,
 * deepinteract_utils.py:474-477, so dU = normalize(0) = 0 and the relative rotation is the
 * identity quaternion). With all direction features zero, the conformation module's neighbour
 * messages are multiplied by dir_linear_1(dir_linear_0(0)) = 0 (both bias-free,
 * deepinteract_modules.py:301-302, :408), so that branch is exactly zero and the gathered
 * silu(nbr_linear(F)) rows are never needed; InitEdge's direction terms are silu(0) = 0 and its
 * orientation terms are per-model constants. With this flag:
 *   di_init_edge  skips the direction terms, adds the orientation terms as packed constants, and
 *                 writes fn_out only when fn_out != NULL;
 *   di_edge_layer skips the neighbour-message branch: fn_in is not read and fn_out is not
 *                 written (both may be NULL).
 * di_conformation ignores the flag (it computes the branch, which is exactly zero). */
#define DI_GRAPH_GEO_REF 1

/* one complex of a pair-tensor launch (host-built array copied to the device) */
typedef struct {
  int64_t h1_row;   /* first node row of chain 1 in the node-feature matrix */
  int64_t h2_row;   /* first node row of chain 2 */
  int64_t out_off;  /* element offset of this complex's [2H, L1, L2] block in `out` */
  int32_t l1, l2;
} di_pair_desc;

int di_abi_version(void);
/* bytes of the packed weight blobs a kernel expects: kind = 0 embed, 1 init_edge,
 * 2 edge_layer(non-final), 3 edge_layer(final), 4 node_layer(non-final), 5 node_layer(final).
 * `vec` selects the fp32 vector blob (biases) instead of the matrix blob. */
int64_t di_blob_bytes(int kind, di_dtype dtype, int vec);
/* MFMA fragment order of a kind's matrix blob (ABI 5): 16 = blocks of 16 output rows x 32 input
 * features (v_mfma_f32_16x16x32_bf16 / 16x16x4_f32 A fragments), 32 = blocks of 32 output rows x 16
 * input features (v_mfma_f32_32x32x16_bf16: the bf16 InitEdge and edge-layer blobs, kinds 1, 2 and 3;
 * the kind-1 32 order also carries the DI_GRAPH_GEO_REF orientation constant as a bf16 hi/lo pair in
 * columns 28/29 of the collapsed message map); -1 for an unknown kind or dtype. Both orders hold the
 * same number of 512-element blocks at the same block offsets (deepinteract_amd/packing.py:
 * pack_matrix / pack_matrix32, init_blob / edge_blob with layout = di_blob_layout(kind, dtype)). */
int di_blob_layout(int kind, di_dtype dtype);

/* in_dim: width of node_f rows (113 for LitGINI's raw node features; 128 with an identity
 * embedding when DGLGeometricTransformer is used standalone on already-embedded features).
 * queue / signal_job (ABI 6; NULL / -1: none): a pair-queue signal carried by this launch -- at its
 * start it marks job signal_job ready, i.e. what di_pair_signal(queue, signal_job) issued just before
 * it on `stream` would do, without that launch (the producer of signal_job's hT must precede this
 * launch on `stream`). Same pair on di_embed_init_edge and di_pair_help. */
int di_node_embed(const di_graph* g, di_dtype dt, int32_t in_dim, const float* node_f /*[Nt,in_dim]*/,
                  const void* wmat, const float* wvec,
                  void* h_out /*[Nt,128]*/, void* qkv_out /*[Nt,384]*/, void* queue, int32_t signal_job,
                  void* stream);

int di_init_edge(const di_graph* g, di_dtype dt, const float* edge_f /*[Et,28]*/,
                 const void* wmat, const float* wvec,
                 const float* pos_src_tab /*[2304,128]*/, const float* pos_dst_tab /*[2304,128]*/,
                 void* f_out /*[Et,128]*/, void* fn_out /*[Et,128]*/, void* stream);
/* The same InitEdge for bf16 DI_GRAPH_GEO_REF batches without layer-0 Fn rows, with the 128 KiB of
 * weight blocks that path reads resident in LDS (one block per CU; waves stride over 16-edge tiles):
 * F bit-identical to di_init_edge. A scheduling choice of this build: faster alone, but its block
 * holds 128 KiB of a CU's 160 KiB LDS, so LDS-staged kernels of other streams (the node embedding)
 * cannot run beside it. DI_EINVAL for batches without DI_GRAPH_GEO_REF. */
int di_init_edge_resident(const di_graph* g, const float* edge_f /*[Et,28]*/, const void* wmat /*bf16 blob*/,
                          const float* wvec, const float* pos_src_tab, const float* pos_dst_tab,
                          void* f_out /*[Et,128] bf16*/, void* stream);
/* di_node_embed + di_init_edge (DI_GRAPH_GEO_REF, no Fn) as ONE launch: the embedding runs as the
 * launch's first blocks, beside InitEdge's, through the same LDS slot -- instead of on a side
 * stream. h_out / qkv_out / f_out bit-identical to the two separate calls. 0 < in_dim <= 128.
 * ABI 5: any dtype (fp32 added: the embedding of the reference's precision inside the launch). */
int di_embed_init_edge(const di_graph* g, di_dtype dt, int32_t in_dim, const float* node_f /*[Nt,in_dim]*/,
                       const void* embed_wmat, const float* embed_wvec, void* h_out /*[Nt,128]*/,
                       void* qkv_out /*[Nt,384]*/, const float* edge_f, const void* init_wmat, const float* init_wvec,
                       const float* pos_src_tab, const float* pos_dst_tab, void* f_out /*[Et,128]*/, void* queue,
                       int32_t signal_job, void* stream);

int di_edge_layer(const di_graph* g, di_dtype dt, int final_layer, const float* edge_f,
                  const void* f_in, const void* fn_in, const void* qkv,
                  const void* wmat, const float* wvec,
                  float* alpha_out /*[Et,4]*/, void* f_out, void* fn_out, void* stream);
/* The bf16 DI_GRAPH_GEO_REF pair InitEdge -> non-final layer 0 without the [Et,128] row F0 between
 * them (an addition to ABI 8). F0 = combined_linear_2(z0) with z0 InitEdge's 32-wide
 * combined_linear_1 output, so:
 *   di_embed_init_edge_z = di_embed_init_edge (queue / signal_job included) storing z0 instead of F0:
 *     z_out is [Et,32] bf16 (64 B per edge, a quarter of the F0 row) in the kernels' packed operand
 *     order -- element 16 h + 8 s + j of a row is z0 feature 16 s + 8 (j >> 2) + 4 h + (j & 3), for
 *     h, s in {0,1}, j < 8; features 28..31 are zero padding. Private to this pair of entry points.
 *   di_edge_layer_z = di_edge_layer(final_layer = 0) reading z_in (those rows) and init_wmat (the
 *     kind-1 bf16 blob InitEdge ran with) instead of f_in: each 32-feature block of F0 is rebuilt in
 *     registers where the layer uses it -- the MFMAs and the bf16 rounding InitEdge applies -- so
 *     alpha_out and f_out are bit-identical to di_embed_init_edge + di_edge_layer. alpha_out may be
 *     NULL (not written).
 * DI_EINVAL unless dt == DI_BF16 and the graph has DI_GRAPH_GEO_REF. There is no di_edge_layer_attn
 * form. */
int di_embed_init_edge_z(const di_graph* g, di_dtype dt, int32_t in_dim, const float* node_f /*[Nt,in_dim]*/,
                         const void* embed_wmat, const float* embed_wvec, void* h_out /*[Nt,128]*/,
                         void* qkv_out /*[Nt,384]*/, const float* edge_f, const void* init_wmat,
                         const float* init_wvec, const float* pos_src_tab, const float* pos_dst_tab,
                         void* z_out /*[Et,32] bf16*/, void* queue, int32_t signal_job, void* stream);
int di_edge_layer_z(const di_graph* g, di_dtype dt, const float* edge_f, const void* z_in /*[Et,32] bf16*/,
                    const void* init_wmat /*kind-1 bf16 blob*/, const void* qkv, const void* wmat,
                    const float* wvec, float* alpha_out /*[Et,4]*/, void* f_out /*[Et,128]*/, void* stream);

/* disable_geometric_mode (an addition to ABI 8): the edge side of the reference's plain Graph
 * Transformer baseline (deepinteract_modules.py:1349-1351, :1444-1451, :584, :676, :819-821, :897-904);
 * the node side is di_node_aggregate + di_node_update / di_node_layer, unchanged. The graph's nbr,
 * node_pos and flags are not read.
 *   di_plain_blob_bytes  bytes of the packed blobs (packing.init_blob_plain / edge_blob_plain): kind
 *                        0 InitEdge (no vector blob: 0 bytes), 1 intermediate layer, 2 final layer;
 *                        -1 for any other kind or a bad dtype. Always the 16x16 fragment order.
 *   di_init_edge_plain   F0 = W_i . cat(edge_f[:,0], edge_f[:,1], edge_f), bias-free.
 *   di_edge_layer_plain  intermediate (final_layer = 0): c = f_in; alpha_out from BN1e / projection /
 *                        K[src] . Q[dst] as di_edge_layer; f_out = f_in + O_edge(score) + FFN(BN2e(.)).
 *                        final: c = W_c . cat(f_in[:,0], f_in[:,1], edge_f) -- columns 0 / 1 of the HIDDEN
 *                        edge features, as the reference computes it -- then alpha_out; f_out is not written.
 * DI_EINVAL, before any launch: a NULL argument (f_out may be NULL on the final layer only; stream may
 * be NULL), g->src / g->dst NULL for the layer, num_edges <= 0, a bad dtype. */
int64_t di_plain_blob_bytes(int kind, di_dtype dtype, int vec);
int di_init_edge_plain(const di_graph* g, di_dtype dt, const float* edge_f /*[Et,28]*/, const void* wmat,
                       void* f_out /*[Et,128]*/, void* stream);
int di_edge_layer_plain(const di_graph* g, di_dtype dt, int final_layer, const float* edge_f /*[Et,28]*/,
                        const void* f_in /*[Et,128]*/, const void* qkv /*[Nt,384]*/, const void* wmat,
                        const float* wvec, float* alpha_out /*[Et,4]*/, void* f_out /*[Et,128]*/, void* stream);

/* hT_out (optional, may be NULL): also write h_out transposed, [128, Nt] (pair-tensor input).
 * bf16: DI_ERANGE when Nt * 768 or Et * 16 reaches 2^31 (the segment sums use 32-bit byte offsets;
 * split such a batch, or use di_node_aggregate + di_node_update). */
int di_node_layer(const di_graph* g, di_dtype dt, int final_layer, const float* alpha,
                  const void* h_in, const void* qkv, const void* wmat, const float* wvec,
                  void* h_out, void* qkv_out, void* hT_out, void* stream);
/* The node layer in two launches (what GeoTEngine runs): the attention aggregation as a CSR
 * segment reduction over each node's in-edges (replaces send_and_recv(u_mul_e, sum) +
 * (copy_e, sum) + wV / (z + 1e-6), deepinteract_modules.py:93-96, 116):
 *   attn_out[v, :] = sum_{e: dst(e) = v} alpha[e, head] * V[src(e), :] / (sum_e alpha[e, head] + 1e-6)
 * (fp32 [Nt, 128]; V = columns 256..383 of qkv), then O_node + residual + FFN (+ next layer's
 * Q/K/V, + optional transposed copy) from those rows. Bit-identical to di_node_layer: the same
 * products added one in-edge at a time in edge order (16 lanes per destination). */
int di_node_aggregate(const di_graph* g, di_dtype dt, const float* alpha /*[Et,4]*/, const void* qkv /*[Nt,384]*/,
                      float* attn_out /*[Nt,128]*/, void* stream);
int di_node_update(const di_graph* g, di_dtype dt, int final_layer, const float* attn /*[Nt,128]*/,
                   const void* h_in, const void* wmat, const float* wvec, void* h_out, void* qkv_out,
                   void* hT_out, void* stream);
/* ABI 7: the same aggregation folded into the bf16 edge layer's epilogue (no alpha round trip, no
 * gather launch). di_edge_layer_attn = di_edge_layer (alpha_out may be NULL: not written) + the
 * segment sums of its edges: the kernel's waves each hold 32 consecutive (destination-major) edges,
 * "fold tile" t = edges 32t .. 32t+31; for every destination v
 *   all in-edges in one fold tile:  attn_out[v, :] = wV / (z + 1e-6)  (fp32 [Nt,128], as di_node_aggregate)
 *   in-edges over tiles t0 < .. < t1: attn_parts[t0][1] holds tile t0's partial sums (wV[128], z[4]),
 *                                     attn_parts[t][0] tile t's for t0 < t <= t1
 * attn_parts: di_attn_parts_bytes(num_edges) bytes (fp32 [ceil(Et/32)][2][132]); rows of nodes
 * without in-edges are not written. dt must be DI_BF16 and g->in_ptr set (DI_EINVAL otherwise).
 * Summation order: a tree over a tile's rows, then tile by tile (di_node_aggregate adds in edge
 * order; both within the bf16 path's bound). di_node_update_folded = di_node_update on those
 * outputs: split destinations add their partials, nodes without in-edges get 0. */
int64_t di_attn_parts_bytes(int32_t num_edges);
int di_edge_layer_attn(const di_graph* g, di_dtype dt, int final_layer, const float* edge_f,
                       const void* f_in, const void* fn_in, const void* qkv, const void* wmat, const float* wvec,
                       float* alpha_out, void* f_out, void* fn_out, float* attn_out /*[Nt,128]*/,
                       float* attn_parts, void* stream);
int di_node_update_folded(const di_graph* g, di_dtype dt, int final_layer, const float* attn,
                          const float* attn_parts, const void* h_in, const void* wmat, const float* wvec,
                          void* h_out, void* qkv_out, void* hT_out, void* stream);

/* Pair-tensor kernel of a di_pair_tensor call (di_pair_launch.kernel). Scheduling choice of this
 * build, not a reference interface; every kernel writes the same bytes. */
enum {
  DI_PAIR_AUTO = 0,    /* ROWS for aligned >= 1, the generic kernel otherwise */
  DI_PAIR_ROWS = 1,    /* a wave streams 64 whole rows (needs aligned >= 1) */
  DI_PAIR_VECTOR = 2,  /* one 16-B load per 16-B store over flat plane positions (aligned >= 1) */
  DI_PAIR_LINES = 3,   /* every store writes whole 128-B lines (aligned == 2) */
};
/* Launch of one di_pair_tensor call (host struct; NULL = all defaults). */
typedef struct {
  int32_t kernel;           /* DI_PAIR_* */
  int32_t blocks;           /* resident blocks of the persistent grid; 0 = one per CU */
  int32_t waves_per_block;  /* ROWS / LINES: 1..16 waves per block; 0 = 4 */
  int32_t beside;           /* 1: the schedule beside a concurrent GeoT stream: at most 3 stores in
                               flight per wave (its loads do not queue behind a store backlog) and
                               non-temporal stores; 0: plain stores, unbounded */
} di_pair_launch;

/* h [Nt, hidden] node features; hT (optional for aligned == 0) the same transposed [hidden, Nt]
 * (di_node_layer's hT_out), which turns chain-2 column reads into 16-B vector loads.
 * aligned: 0 none; 1 promises every L2, out_off and h2_row is a multiple of 16 bytes worth of
 * elements and `out` is 16-B aligned (vector stores); 2 additionally promises every channel plane
 * starts on a 128-B line (out 128-B aligned, out_off * elem and L1 * L2 * elem multiples of 128).
 * Limits: L1 * L2 * elem < 2^31 bytes per plane, L1 <= 2^20 (di_pair_tensor_check). */
int di_pair_tensor(di_dtype dt, const di_pair_desc* descs /*device [B]*/, int32_t num_complexes,
                   int32_t max_l1, int32_t max_l2, int32_t hidden, int32_t aligned, const void* h,
                   const void* hT, int32_t num_rows, const di_pair_launch* launch, void* out, void* stream);
/* The shape / launch validation di_pair_tensor applies before launching (host only): DI_OK,
 * DI_EINVAL or DI_ERANGE. elem_bytes: 2 (bf16) or 4 (fp32). */
int di_pair_tensor_check(int32_t num_complexes, int32_t max_l1, int32_t max_l2, int32_t hidden, int32_t elem_bytes,
                         const di_pair_launch* launch);

/* ---- pair-tensor queue (ABI 6): the overlapped schedule's pair stream -----------------------------
 * A job is one micro-batch's pair tensors (construct_interact_tensor of each complex,
 * deepinteract_utils.py:158-172), produced by the GeoT stream in job order. The producer stream signals
 * each job after its final node layer (hT written): with di_pair_signal, or carried by its next launch
 * (the signal_job argument of di_node_embed / di_embed_init_edge / di_pair_help); it calls
 * di_pair_help before it reuses a job's hT buffer and once at the end of a run (drain). di_pair_stream is one persistent launch
 * on its own stream over a range of jobs, beside the producer: its waves wait for each job's signal and
 * take the job's items (complex, channel, 64-row block) from the queue's per-job ticket counter, with
 * the bounded non-temporal stores of di_pair_launch.beside. di_pair_help takes the remaining items of
 * its jobs with plain stores on the whole chip and returns (on the device) once every item of them is
 * done, whoever took it: a wave counts its items DONE only after its stores have completed, so every
 * launch ordered after a help launch on its stream reads the jobs' final bytes. Completion never depends on di_pair_stream running concurrently: a stream
 * wave that waits longer than patience_ms for a signal gives up and the help launches do the rest. The
 * bytes written are those of di_pair_tensor(aligned = 1) for the same descriptors.
 * Preconditions (the kernels cannot check device-resident jobs): every job's descs are 16-B aligned
 * planes (L2 and out_off multiples of 16 bytes of the dtype, h2_row too), hT 16-B aligned, items =
 * di_pair_job_items(num_complexes, max_l1, hidden), and max_l1 >= every descs[i].l1. */
typedef struct {
  const void* hT;             /* [hidden, num_rows] transposed final node features (di_node_layer hT_out) */
  const di_pair_desc* descs;  /* [num_complexes] (device) */
  void* out;                  /* base of the job's pair tensors (descs[i].out_off elements from here) */
  int32_t num_rows;           /* columns of hT: node rows of the micro-batch */
  int32_t num_complexes;
  int32_t max_l1;             /* largest chain-1 length of the job */
  int32_t items;              /* di_pair_job_items(num_complexes, max_l1, hidden) */
} di_pair_job;
/* device bytes of a queue for jobs 0 .. num_jobs-1 (zero it before first use; -1 for num_jobs <= 0).
 * Words (uint32): [0] jobs signalled, [32] error bits (1: a help launch's completion wait timed out,
 * 2: a stream wave read a non-increasing ticket),
 * [33] stream waves that gave up waiting, [40..41] / [42..43] bytes written by stream / help launches
 * (uint64), then 256 B per job (ticket, arrive, done; csrc/pair_queue.h). */
int64_t di_pair_queue_bytes(int32_t num_jobs);
/* items of a job: num_complexes * 2 * hidden * ceil(max_l1 / 64); DI_EINVAL / DI_ERANGE */
int32_t di_pair_job_items(int32_t num_complexes, int32_t max_l1, int32_t hidden);
/* the job's hT is complete (stream order of `stream`): raises the queue's signalled count to job + 1 */
int di_pair_signal(void* queue, int32_t job, void* stream);
/* persistent pair stream over jobs [job_begin, job_end) (jobs: device array indexed by job number);
 * launch: blocks (0: one per CU; fp32: half the CUs), waves_per_block (0: 2; fp32: 4); always the beside
 * store policy */
int di_pair_stream(di_dtype dt, const di_pair_job* jobs, int32_t job_begin, int32_t job_end, int32_t hidden,
                   void* queue, const di_pair_launch* launch, float patience_ms, void* stream);
/* complete jobs [first_job, last_job] (all produced before this call in `stream` order); launch:
 * blocks (0: one per CU), waves_per_block (0: 8); signal_job >= 0: also marks that job ready at the
 * launch's start (as di_node_embed's signal) */
int di_pair_help(di_dtype dt, const di_pair_job* jobs, int32_t first_job, int32_t last_job, int32_t hidden,
                 void* queue, const di_pair_launch* launch, int32_t signal_job, void* stream);

/* ---- streams of the overlapped schedule (ABI 8; host calls, synchronous) ---------------------------
 * di_pair_stream waits on the device for signals that launches on the producer's stream raise, so the
 * two streams must reach the GPU through DIFFERENT hardware queues. HIP multiplexes a process's
 * streams onto at most GPU_MAX_HW_QUEUES in-order queues per priority (least-used first once the pool
 * is full), so which queue an ordinary stream gets depends on every stream created before it (an RCCL
 * communicator creates several); two streams on one queue run one after the other and every stream
 * wave waits out its patience.
 * di_stream_create_dedicated: a normal-priority stream whose CU mask covers every CU -- the runtime
 * gives each CU-masked stream a hardware queue of its own, never shared with another stream. Like every
 * stream created with default flags it synchronises with the legacy NULL stream: issue nothing on the
 * NULL stream while a pair-stream launch is in flight.
 * di_streams_concurrent: measures the property: a one-wave kernel on `a` waits (at most patience_ms,
 * <= 10000) for a word that a kernel on `b`, issued after it, raises; *concurrent (host) = 1 if it saw
 * it, else 0. work: >= 256 device bytes, overwritten. Synchronises both streams. */
int di_stream_create_dedicated(void** stream);
int di_stream_destroy(void* stream);
int di_streams_concurrent(void* a, void* b, void* work, float patience_ms, int32_t* concurrent);

/* Fused head prologue: x = ELU(InstanceNorm2d(conv2d_1(T))) of the contact
 * head (ResNet2DInputWithOptAttention.forward, deepinteract_modules.py:1181-1184, 1228-1232) for a
 * batch of complexes WITHOUT materialising the pair tensor T: the 1x1 conv of the outer concat
 * separates into W[:, :H] h1[i] + W[:, H:] h2[j] + b and the InstanceNorm statistics of that
 * separable sum are analytic. h: [rows, hidden] node features in `dt` (16-B aligned, hidden a
 * multiple of 8, <= 256); conv_w [channels, 2*hidden], conv_b, in_gamma, in_beta [channels] fp32;
 * work: device scratch of di_head_prologue_work_bytes() bytes; out: per complex [channels, L1, L2]
 * in `dt` at descs[i].out_off (elements). aligned16: every L2 and out_off a multiple of 16 bytes
 * of `dt` (row-streaming store kernel). */
int di_head_prologue(di_dtype dt, const di_pair_desc* descs /*device [B]*/, int32_t num_complexes, int32_t max_l1,
                     int32_t max_l2, int32_t hidden, int32_t channels, int32_t aligned16, const void* h,
                     const float* conv_w, const float* conv_b, const float* in_gamma, const float* in_beta,
                     float eps, float* work, void* out, void* stream);
int64_t di_head_prologue_work_bytes(int32_t num_complexes, int32_t max_l1, int32_t max_l2, int32_t channels);

/* ---- contact-head body (convolutions stay on MIOpen) --------------------- */
/* y = ELU(InstanceNorm2d(x)) of one [channels, hw] NCHW image (batch 1): biased variance, eps,
 * affine gamma/beta [channels] fp32; fp64 statistics. Replaces the `inorm_i` + `F.elu` pair of
 * every inorm ResNet block (ResNet.forward, deepinteract_modules.py:1075-1095; the modules
 * :1016-1030) and of the head prologue (:1231-1232). x, y: 16-B aligned, `dt` storage (y may
 * alias x); work: di_inorm_work_bytes() bytes of device scratch. */
int di_inorm_elu(di_dtype dt, const void* x, int32_t channels, int64_t hw, const float* gamma,
                 const float* beta, float eps, void* work, void* y, void* stream);
int64_t di_inorm_work_bytes(int32_t channels, int64_t hw);
/* y = (x + bias[c]) * scale[c] + res: the ResNet block's last conv bias (nullable), SEBlock's
 * channel gate (deepinteract_modules.py:954-970) and the block's residual add (:1095); each step
 * is rounded to `dt`, as torch's separate kernels do. x, res, y: [channels, hw], 16-B aligned (y
 * may alias x or res); scale, bias [channels] fp32. */
int di_se_scale_add(di_dtype dt, const void* x, const float* scale, const float* bias, const void* res,
                    int32_t channels, int64_t hw, void* y, void* stream);
/* mean[c] = mean over hw of x[c] (+ bias[c], nullable): SEBlock's x.mean(dim=(2, 3))
 * (:966) of a conv output whose bias is deferred to di_se_scale_add. fp64 accumulation;
 * work: di_inorm_work_bytes() bytes. */
int di_channel_mean(di_dtype dt, const void* x, int32_t channels, int64_t hw, const float* bias, void* work,
                    float* mean, void* stream);

/* ---- contact-head convolutions with fused norm + ELU (an addition to ABI 8) -----------------
 * di_head_conv: one 1x1 or dilated 3x3 convolution (stride 1, padding = dilation) of one NCHW image,
 * bf16 storage, fp32 accumulation on the matrix cores:
 *   a = in_elu ? ELU(x * in_scale[ci] + in_shift[ci]) : x * in_scale[ci] + in_shift[ci]
 *       in fp32, rounded to bf16 (RNE); NULL in_scale / in_shift mean 1 / 0. The zero padding applies
 *       AFTER the transform: a tap outside the image contributes 0.
 *   y = conv(a, weight) (+ bias[co], nullable), rounded to bf16 (RNE) once.
 * x [cin, h, w], y [cout, h, w]: bf16, any 2-byte alignment, planes at 64-bit offsets (h * w may be odd
 * and cin * h * w may pass 2^31); y must not alias x. weight: [cout, cin, ksize, ksize] contiguous bf16
 * (the module's own tensor). in_scale, in_shift [cin], bias [cout]: fp32. cin 64 / 128 / 256, cout
 * 64 / 128, ksize 1 or 3, dilation 1 .. 8 (ignored by ksize 1), h, w >= 1.
 * stats (nullable; 8-B aligned, di_head_conv_stats_bytes(cout, h, w) bytes): per output channel the
 * (sum y, sum y^2) of the values as stored, one fp64 partial pair per block and channel, no atomics
 * (bit-reproducible). Layout: int64 n (partials per channel), int64 0, then double [channels][n][2].
 * di_head_conv_check: the same validation on the host, without a launch. DI_EINVAL: dt other than
 * DI_BF16, an unsupported cin / cout / ksize / dilation, h or w < 1, NULL x / weight / y, y == x, a
 * misaligned pointer. DI_ERANGE: more than 2^31 - 1 tiles of 256 pixels (ksize 1), h > 16 * 65535
 * (ksize 3).
 * di_plane_stats: the same partials from a stored [channels, hw] image (fp32 or bf16, 16-B aligned) in
 * one read pass; stats as above (di_head_conv_stats_bytes bytes suffice).
 * di_head_norm_fold: adds a statistics buffer's partials in a fixed order and writes, per channel,
 *   scale = gamma / sqrt(var + eps), shift = beta - mean * scale   (InstanceNorm2d as an affine map:
 *           biased variance, fp64 inside; NULL gamma / beta mean 1 / 0)
 *   mean  = mean (+ bias[c], nullable)                             (the SE squeeze, as di_channel_mean)
 * as fp32 [channels]; any of the three outputs may be NULL. hw = h * w of the image.
 * di_head_conv_f32: di_head_conv with fp32 storage (x, weight, y: fp32, 4-byte aligned), the same
 * arguments and shapes: a in fp32 with no rounding of its own (the ELU's negative branch is expm1f),
 * the sum on the f32-input matrix instructions (a k-ordered fp32 fmaf chain), bias added to the finished
 * sum. stats: as above, of the fp32 values as stored, the same layout and di_head_conv_stats_bytes
 * bytes; di_plane_stats(DI_F32, ...) and di_head_norm_fold take it unchanged. No atomics.
 * di_head_conv_f32_check: its validation on the host, without a launch: di_head_conv_check's refusals
 * but the dtype's, with 4-byte alignment. */
typedef struct {
  const void* x; const void* weight; const float* in_scale; const float* in_shift; const float* bias;
  void* y; void* stats;
  int32_t cin, cout, h, w, ksize, dilation, in_elu;
} di_head_conv_args;
int di_head_conv(di_dtype dt, const di_head_conv_args* args, void* stream);
int di_head_conv_check(di_dtype dt, const di_head_conv_args* args);
int di_head_conv_f32(const di_head_conv_args* args, void* stream);
int di_head_conv_f32_check(const di_head_conv_args* args);
int64_t di_head_conv_stats_bytes(int32_t cout, int32_t h, int32_t w);
int di_plane_stats(di_dtype dt, const void* x, int32_t channels, int64_t hw, void* stats, void* stream);
int di_head_norm_fold(const void* stats, int32_t channels, int64_t hw, const float* gamma, const float* beta,
                      float eps, const float* bias, float* scale, float* shift, float* mean, void* stream);

/* ---- the contact-head body over a ragged batch of images (an addition to ABI 8) -------------
 * `count` images of different shapes go through each head kernel in ONE launch, whatever count is.
 * Packed ragged image: a batch of [C, h_i, w_i] bf16 images in one buffer, item i a contiguous NCHW
 * image at element offset C * px_off_i, px_off_i = sum over j < i of h_j * w_j (64-bit). The head's C
 * are multiples of 64, so with a 128-B aligned buffer every item starts 128-B aligned.
 * di_head_batch_layout fills px_off and stats_off (the item's byte offset in the batch's statistics
 * buffer: 16-B aligned, room for di_head_conv_stats_bytes(128, h, w)) from h and w, and returns the
 * pixel total and the statistics buffer's bytes through total_px / stats_bytes. One table serves every
 * launch of a forward:
 *   items      host array [count]: validated, and used for grid sizes; may be freed on return
 *   items_dev  a copy of it in device memory, made by the caller (in stream order before the call;
 *              it must stay unchanged until the call's kernels have run)
 * The grid's z index names the item; a block reads its item from the device table, leaves as a whole
 * (before any barrier) when its x / y index lies past that item's own tile or slice count, and
 * otherwise runs the single call's code on that item's sizes alone: every output of an item (the
 * statistics partials included) has the bits the single call gives on that image.
 * di_head_conv_batch: args as di_head_conv with x, y and stats packed buffers (stats nullable),
 * in_scale / in_shift [count, cin] fp32 rows (nullable), weight and bias shared; args->h and args->w
 * are ignored. di_plane_stats_batch: bf16 only, x 16-B aligned, channels a multiple of 8 (items start
 * 16-B aligned) and <= 128 (an item's room in stats). di_head_norm_fold_batch: channels <= 128; gamma,
 * beta, bias [channels] shared; scale / shift / mean [count, channels] rows, each nullable.
 * di_se_scale_add_batch: scale [count, channels], bias [channels] (nullable); bf16, 16-B aligned,
 * channels a multiple of 8; y may alias x or res.
 * di_se_gate: gate[i][c] = sigmoid(relu(b2[c] + sum_j w2[c][j] * relu(b1[j] + sum_k w1[j][k] *
 * mean[i][k]))) -- SEBlock's two linears (deepinteract_modules.py:954-970) on [count, channels] fp32
 * means, all fp32, each sum taken in index order by fused multiply-adds starting from the bias, so a
 * row's bits depend on nothing but that row. w1 [hidden, channels], w2 [channels, hidden] row-major.
 * channels 1 .. 1024, hidden 1 .. 64, count >= 1. One launch.
 * The fp32 batch (the parity head, di_head_conv_f32's storage): packed ragged fp32 images, item i of a
 * C-channel buffer at element offset C * px_off_i, with the same table, the same statistics buffer and
 * the same rows. The bf16 entry points above keep refusing DI_F32; the fp32 forms are entry points of
 * their own, as di_head_conv_f32 is:
 *   di_head_conv_f32_batch     di_head_conv_batch's contract with fp32 x, weight and y (4-byte aligned);
 *                              every item has the bits di_head_conv_f32 gives on that image
 *   di_head_conv_f32_batch_check  its validation on the host, without a launch
 *   di_plane_stats_f32_batch   di_plane_stats_batch for fp32: x 16-B aligned, channels a multiple of 4
 *                              (items start 16-B aligned) and <= 128; the bits of di_plane_stats(DI_F32)
 *   di_se_scale_add_f32_batch  di_se_scale_add_batch for fp32: 16-B aligned, channels a multiple of 4;
 *                              the bits of di_se_scale_add(DI_F32)
 * di_head_norm_fold_batch and di_se_gate hold no image dtype and serve both; di_region_scores_batch /
 * di_region_mix_batch take DI_F32.
 * Asynchronous, no allocation, every refusal before any launch. DI_EINVAL: count < 1, a NULL table,
 * h or w < 1, offsets that the helper did not fill, or anything the single call refuses with
 * DI_EINVAL; DI_ERANGE: count > DI_BATCH_MAX, more than 2^40 pixels in all, or an item the single
 * call refuses with DI_ERANGE. */
typedef struct { int64_t px_off, stats_off; int32_t h, w; } di_head_item;
int di_head_batch_layout(di_head_item* items, int32_t count, int64_t* total_px, int64_t* stats_bytes);
int di_head_conv_batch(di_dtype dt, const di_head_conv_args* args, const di_head_item* items,
                       const di_head_item* items_dev, int32_t count, void* stream);
int di_plane_stats_batch(di_dtype dt, const void* x, int32_t channels, const di_head_item* items,
                         const di_head_item* items_dev, int32_t count, void* stats, void* stream);
int di_head_norm_fold_batch(const void* stats, int32_t channels, const di_head_item* items,
                            const di_head_item* items_dev, int32_t count, const float* gamma, const float* beta,
                            float eps, const float* bias, float* scale, float* shift, float* mean, void* stream);
int di_se_scale_add_batch(di_dtype dt, const void* x, const float* scale, const float* bias, const void* res,
                          int32_t channels, const di_head_item* items, const di_head_item* items_dev,
                          int32_t count, void* y, void* stream);
int di_se_gate(const float* mean, const float* w1, const float* b1, const float* w2, const float* b2,
               int32_t count, int32_t channels, int32_t hidden, float* gate, void* stream);
int di_head_conv_f32_batch(const di_head_conv_args* args, const di_head_item* items,
                           const di_head_item* items_dev, int32_t count, void* stream);
int di_head_conv_f32_batch_check(const di_head_conv_args* args, const di_head_item* items,
                                 const di_head_item* items_dev, int32_t count);
int di_plane_stats_f32_batch(const void* x, int32_t channels, const di_head_item* items,
                             const di_head_item* items_dev, int32_t count, void* stats, void* stream);
int di_se_scale_add_f32_batch(const void* x, const float* scale, const float* bias, const void* res,
                              int32_t channels, const di_head_item* items, const di_head_item* items_dev,
                              int32_t count, void* y, void* stream);

/* ---- the whole contact-head body in one call (an addition to ABI 8) -------------------------
 * di_head_body_batch: everything between the prologue ELU(inorm_1(conv2d_1(T))) and phase2_conv
 * (ResNet2DInputWithOptAttention.forward, deepinteract_modules.py:1234-1247) for a ragged batch of
 * images -- the model's two dilated ResNets, 56 + 6 bottleneck blocks (ResNet.forward :1075-1095) --
 * as one host loop over the *_batch entry points above. It adds no kernel and no arithmetic: per net
 *   init_proj (if given):  conv 1x1 128 -> 128 (+ proj_b), ELU on its load when in_elu
 * and per block, with x the 128-channel residual stream and `spare` the other wide buffer,
 *   norms given:   plane_stats(x); fold(gamma1, beta1) -> conv 1x1 128 -> 64 into half0 (stats);
 *                  fold(gamma2, beta2) -> conv 3x3 `dilation` 64 -> 64 into half1 (stats);
 *                  fold(gamma3, beta3) -> conv 1x1 64 -> 128 into spare (stats)
 *   no norms:      conv 1x1 (+ bias1) into half0; conv 3x3 (+ bias2) into half1; conv 1x1 into spare
 *                  (stats); each with ELU on its load
 *   then           fold(bias3) -> mean; di_se_gate -> gate; spare = (spare + bias3) * gate + x;
 *                  x and spare swap
 * -- one launch each on `stream`, whatever count is: 10 per normed block, 6 per block without norms, 1
 * per init_proj (598 for the model). The scale / shift / mean / gate rows are rows[0 .. 3] of the
 * arena; a 64-channel fold writes [count, 64] rows at the start of its [count, 128] room.
 *   di_head_block  device pointers: w1 [64, 128, 1, 1], w2 [64, 64, 3, 3], w3 [128, 64, 1, 1] bf16 (the
 *                  modules' own tensors, as di_head_conv takes them); gamma / beta 1 .. 3 fp32 [128],
 *                  [64], [64], all six given or all six NULL; bias1, bias2 [64] fp32 (nullable; read
 *                  only without norms: in front of a norm a bias cancels), bias3 [128] fp32 (nullable);
 *                  the SE block's w1 [8, 128], b1 [8], w2 [128, 8], b2 [128] fp32; eps of the three
 *                  norms; dilation 1 .. 8 of w2.
 *   di_head_net    proj_w [128, 128, 1, 1] bf16 (NULL: no initial projection) and proj_b [128] fp32
 *                  (nullable); blocks: HOST array [num_blocks], num_blocks >= 1; in_elu: the ELU in
 *                  front of this net, applied by init_proj's load (so it needs proj_w).
 *   di_head_arena  the batch's buffers: wide0 (holds the input), wide1 [128 * pixels] and half0, half1
 *                  [64 * pixels] bf16, 16-B aligned, all different; stats (8-B aligned, stats_bytes of
 *                  di_head_batch_layout); rows fp32 [4][count][128]; items / items_dev / count as above.
 * nets: HOST array [num_nets] run in order. *result (host): 0 when wide0 holds the output, 1 for wide1.
 * Same kernels on the same geometry as a caller issuing the launches itself: the same bits.
 * Asynchronous: no allocation, no synchronisation, no graph capture; every refusal comes before the
 * first launch, and the first launch error (hipGetLastError after each) is returned as it is.
 * di_head_body_batch_check: the same validation on the host, without a launch. DI_EINVAL: dt other than
 * DI_BF16, NULL nets / arena / result, num_nets or num_blocks < 1, a NULL weight or SE vector, norms
 * partly given, in_elu without proj_w, eps < 0 or NaN, dilation outside 1 .. 8, a NULL, misaligned or
 * repeated arena buffer, or a table the *_batch calls refuse; DI_ERANGE as they return it.
 *
 * di_head_logits_batch: phase2_conv(ELU(x)) (:1241, 1247) for every item of a packed 128-channel bf16
 * buffer in one launch (the one kernel this section adds): per pixel a_c = bf16(ELU(x_c)), ELU in fp32
 * as di_head_conv's; y_o = bf16(sum over c of w[o][c] * a_c + b[o]) for o = 0, 1, the sum in fp32 in
 * channel order by fused multiply-adds from 0, one rounding (RNE) at the store. weight [2, 128] fp32
 * row-major (the 1x1 kernel's values), bias [2] fp32 (nullable). x 16-B aligned. y: packed [2 * pixels]
 * bf16, item i a contiguous [2, h, w] image at element offset 2 * px_off_i, any 2-byte alignment (what
 * di_contact_rank takes); y must not alias x. Errors as the *_batch calls. */
typedef struct {
  const void* w1; const void* w2; const void* w3;
  const float* gamma1; const float* beta1; const float* gamma2; const float* beta2;
  const float* gamma3; const float* beta3;
  const float* bias1; const float* bias2; const float* bias3;
  const float* se_w1; const float* se_b1; const float* se_w2; const float* se_b2;
  float eps; int32_t dilation;
} di_head_block;
typedef struct {
  const void* proj_w; const float* proj_b; const di_head_block* blocks;
  int32_t num_blocks, in_elu;
} di_head_net;
typedef struct {
  void* wide0; void* wide1; void* half0; void* half1; void* stats; float* rows;
  const di_head_item* items; const di_head_item* items_dev;
  int32_t count;
} di_head_arena;
int di_head_body_batch(di_dtype dt, const di_head_net* nets, int32_t num_nets, const di_head_arena* arena,
                       int32_t* result, void* stream);
int di_head_body_batch_check(di_dtype dt, const di_head_net* nets, int32_t num_nets, const di_head_arena* arena);
int di_head_logits_batch(di_dtype dt, const void* x, const float* weight, const float* bias,
                         const di_head_item* items, const di_head_item* items_dev, int32_t count, void* y,
                         void* stream);

/* ---- the head's regional attention (an addition to ABI 8) -----------------------------------
 * MultiHeadRegionalAttention (deepinteract_modules.py:1109-1152; MHA2D_1 / MHA2D_2 of the head with
 * use_interact_attention, :1206-1216, :1236-1244) for one [128, h, w] NCHW image, fixed at 128
 * channels, 4 heads of 32 channels, d_k 16 and a 3 x 3 region, without the reference's ninefold
 * stretch of q, k and v. dt: DI_F32 or DI_BF16 storage of x, v and y.
 *   di_region_scores  a = in_elu ? ELU(x) : x in fp32 (di_head_conv's ELU); q = wq a, k = wk a per
 *                     pixel, fused multiply-add chains over the channels in order from 0;
 *                     scores[hd, p] = 0.25 * sum_{j = 4 hd .. 4 hd + 3} q[j, p] k[j, p]. q, k and the
 *                     scores are fp32 throughout. wq, wk: [16, 128] fp32 row-major (the 1x1 kernels'
 *                     values). scores: [4, h, w] fp32. x is read once.
 *   di_region_mix     y[c, p] = sum over the 9 taps d of e_d v[c, p + d] / sum over the 9 taps of e_d,
 *                     e_d = exp(s_d - m), s_d = scores[c / 32, p + d], m = max over the 9 taps of s_d.
 *                     A tap outside the image has s_d = 0 and v = 0 and stays in m and in the
 *                     denominator (a 1 x 1 image gives v e^s / (e^s + 8)). fp32 arithmetic, taps in
 *                     row-major order, one rounding (RNE) at the store. v must be finite (an outside
 *                     tap is a finite stand-in times a weight of exactly 0).
 * Pointers need their element's alignment only (h * w may be odd, so planes may start on any 2-B / 4-B
 * boundary); with 16-B aligned pointers and h * w a multiple of 4 (scores) / 8 (mix, and w <= 2048) the
 * kernels use 16-B accesses per lane. Planes sit at 64-bit offsets. y may alias x; y must not alias v.
 * No atomics: two runs give the same bits. Asynchronous on `stream`, nothing allocated.
 * di_region_scores reads x, wq, wk, in_elu and writes scores; di_region_mix reads v, scores and writes y;
 * each ignores the other's pointers. di_region_attn_check: the validation of both on the host, without
 * a launch. DI_EINVAL: dt other than the two, h or w < 1, a NULL pointer the call reads or writes,
 * y == v, a pointer off its element's alignment (fp32 for wq, wk, scores). DI_ERANGE: more than
 * 2^31 - 1 tiles of 256 pixels.
 * The *_batch forms: every item of a di_head_item table in one launch; x, v, y are packed
 * [128 * pixels] buffers (item i at element 128 * px_off_i), scores [4 * pixels] fp32 (item i at
 * 4 * px_off_i), h and w of the arguments are ignored. An item gets the single call's kernel body on
 * the single call's geometry for its own sizes and pointers: the same bits. Errors as the other
 * *_batch calls, and any item the single call refuses. */
typedef struct {
  const void* x; const float* wq; const float* wk;
  float* scores;
  const void* v; void* y;
  int32_t h, w, in_elu;
} di_region_attn_args;
int di_region_scores(di_dtype dt, const di_region_attn_args* args, void* stream);
int di_region_mix(di_dtype dt, const di_region_attn_args* args, void* stream);
int di_region_attn_check(di_dtype dt, const di_region_attn_args* args);
int di_region_scores_batch(di_dtype dt, const di_region_attn_args* args, const di_head_item* items,
                           const di_head_item* items_dev, int32_t count, void* stream);
int di_region_mix_batch(di_dtype dt, const di_region_attn_args* args, const di_head_item* items,
                        const di_head_item* items_dev, int32_t count, void* stream);

/* ---- contact ranking (an addition to ABI 8) ------------------------------------------------
 * What LitGINI.test_step does with one complex's logits (deepinteract_modules.py:2018-2101; top-k
 * precision / recall deepinteract_utils.py:977-995), without sorting the map. logits: [1, 2, l1, l2]
 * contiguous NCHW in `dtype`, n = l1 * l2 (the class-1 plane starts at element n, any alignment).
 *   probs [n] fp32       p = softmax(logits)[1] = 1 / (1 + exp(l0 - l1)), computed in fp32 (values
 *                        below FLT_MIN may be flushed to 0; a NaN is stored as the positive quiet
 *                        NaN 0x7fc00000); 16-B aligned
 *   top_ids [k] int32    flat indices i * l2 + j of the k best contacts: p descending, equal p by
 *                        ascending index, NaN above every number (what torch.sort(descending=True,
 *                        stable=True) of probs gives); top_scores [k] fp32 their p
 * labels [n] uint8 0/1 (NULL: none; then top_hits and metrics are NULL too):
 *   top_hits [k] int32   positives among ranks 0 .. r
 *   metrics (device)     num_pos and the confusion counts of (p >= threshold) against the labels;
 *                        ce_sum = sum over all elements of -log softmax(logits)[label] in fp64
 *                        (nn.CrossEntropyLoss in sum form; mean = ce_sum / n)
 * work: di_contact_rank_work_bytes bytes, 16-B aligned; cleared in-stream by the call, so calls
 * that share it need only stream order. Outputs are bit-reproducible from run to run.
 * DI_EINVAL: n < 1, k < 1, k > n, bad dtype, a NULL required pointer, labels / top_hits / metrics
 * not all NULL or all set, threshold NaN, probs or work not 16-B aligned. DI_ERANGE:
 * k > DI_RANK_MAX_K, n >= 2^29 (the fp32 map stays under 2^31 bytes, as the pair tensor's planes).
 * di_contact_rank_work_bytes returns the same -1 / -2. */
typedef struct { int64_t num_pos, tp, fp, fn, tn; double ce_sum; } di_rank_metrics;
#define DI_RANK_MAX_K 4096   /* the model's chain limit: the reference's largest k is l = min(L1, L2) */
int64_t di_contact_rank_work_bytes(int64_t n, int32_t k);
int di_contact_rank(int32_t dtype, const void* logits, int32_t l1, int32_t l2, int32_t k,
                    const uint8_t* labels, float threshold, float* probs, int32_t* top_ids,
                    float* top_scores, int32_t* top_hits, di_rank_metrics* metrics,
                    void* work, void* stream);

/* ---- exact per-complex AUROC / AUPRC (an addition to ABI 8) ---------------------------------
 * test_auroc / test_auprc of LitGINI.test_step (deepinteract_modules.py:2018-2101) for class 1 of one
 * complex: roc_curve + trapezoid and average precision over the distinct thresholds (torchmetrics'
 * exact mode, scikit-learn), without sorting the map. probs [n] fp32 in [0, 1] or NaN, 16-B aligned
 * (the map di_contact_rank stored); labels [n] uint8, non-zero = positive.
 * key = bits of p (monotone for p >= 0). P = num_pos, N = num_neg. Positives grouped by distinct key,
 * descending: groups g = 0 .. U-1 with counts c_g, TP_g = c_0 + .. + c_g, FP_g = negatives with
 * key >= key_g.
 *   u2     sum over (pos, neg) pairs of 2 [p_pos > p_neg] + [p_pos == p_neg], an exact integer
 *   auroc  u2 / (2 P N), one correctly rounded fp64 quotient of the exact integers
 *   auprc  (1 / P) sum_g c_g TP_g / (TP_g + FP_g), terms in fp64, summed in an order that is a
 *          function of U alone
 * num_pos, num_neg (by label) and num_nan (NaN scores of either label) are always filled. With
 * P = 0, N = 0 or num_nan > 0 both figures are NaN and u2 = pos_distinct = 0. overflow = 1 when
 * num_pos > max_pos (the positives' buffer, never written past): then too nothing but the three
 * counts is valid and both figures are NaN; call again with max_pos >= num_pos.
 * work: di_contact_auc_work_bytes bytes, 16-B aligned; cleared in-stream by the call, so calls that
 * share it need only stream order. The call is asynchronous on `stream` and allocates nothing; out
 * is device memory. Outputs are bit-reproducible from run to run (integer atomics only).
 * DI_EINVAL: n < 1, max_pos < 1, max_pos > n, a NULL pointer, probs or work not 16-B aligned.
 * DI_ERANGE: n >= 2^29. di_contact_auc_work_bytes returns the same -1 / -2. */
typedef struct {
  int64_t num_pos, num_neg, num_nan;
  int64_t pos_distinct;
  uint64_t u2;
  double auroc, auprc;
  int32_t overflow, pad;
} di_auc_metrics;
int64_t di_contact_auc_work_bytes(int64_t n, int64_t max_pos);
int di_contact_auc(const float* probs, const uint8_t* labels, int64_t n, int64_t max_pos,
                   di_auc_metrics* out, void* work, void* stream);

/* ---- both of the above over a ragged batch (an addition to ABI 8) ---------------------------
 * `count` complexes of different shapes in ONE launch sequence, whatever count is: one memset + 6
 * launches (rank), one memset + 19 launches (AUC). One item per complex holds the single call's
 * arguments. The grid's y index names the complex; a block reads its item from the DEVICE copy of the
 * table and derives its geometry from that complex's sizes alone, by the single call's functions, so
 * every output of a complex has the bits the single call gives on the same inputs (ce_sum, auroc and
 * auprc included), whatever its neighbours hold.
 *   items      host array [count]: validated, and used for grid sizes and offsets; may be freed on
 *              return
 *   items_dev  a copy of it in device memory, made by the caller (in stream order before the call;
 *              it must stay unchanged until the call's kernels have run)
 * hdr_off / work_off: the complex's places in `work`, filled by the *_batch_work_bytes call (16-B
 * aligned; all that the call clears lies contiguous at the front: every complex's header, for the AUC
 * with its bins); the batch call refuses other values. work: that many bytes, 16-B aligned.
 * One dtype and one threshold serve a rank batch, and its items carry labels / top_hits / metrics
 * either all or none. The AUC overflow rule holds per complex (overflow = 1, only the three counts
 * valid), and leaves the neighbours alone.
 * Asynchronous, no allocation, every refusal before any launch. DI_EINVAL: count < 1, a NULL table,
 * offsets that the helper did not fill, or any item the single call refuses with DI_EINVAL;
 * DI_ERANGE: count > DI_BATCH_MAX, or an item the single call refuses with DI_ERANGE. The
 * *_batch_work_bytes helpers return the same codes for the sizes. */
#define DI_BATCH_MAX 1024
typedef struct {
  const void* logits;
  const uint8_t* labels;
  float* probs;
  int32_t* top_ids;
  float* top_scores;
  int32_t* top_hits;
  di_rank_metrics* metrics;
  int64_t hdr_off, work_off;
  int32_t l1, l2, k, pad;
} di_rank_item;
typedef struct {
  const float* probs;
  const uint8_t* labels;
  di_auc_metrics* out;
  int64_t n, max_pos;
  int64_t hdr_off, work_off;
} di_auc_item;
int64_t di_contact_rank_batch_work_bytes(di_rank_item* items, int32_t count);
int di_contact_rank_batch(int32_t dtype, const di_rank_item* items, const di_rank_item* items_dev,
                          int32_t count, float threshold, void* work, void* stream);
int64_t di_contact_auc_batch_work_bytes(di_auc_item* items, int32_t count);
int di_contact_auc_batch(const di_auc_item* items, const di_auc_item* items_dev, int32_t count,
                         void* work, void* stream);

/* ---- one complex's ranking as a wire record (an addition to ABI 8) ----------------------------
 * What a rank sends of a complex instead of its map (distributed.predict_sharded, gather="topk"):
 * the outputs of di_contact_rank(_batch) and di_contact_auc(_batch) laid side by side, so that the
 * items' top_ids / top_scores / top_hits / metrics / out pointers can name the collective's send
 * buffer and no pack, cast or copy runs between the ops and the send. For a complex of shape
 * (l1, l2) with k kept ranks:
 *   offsets[0]  top_ids     int32[k]
 *   offsets[1]  top_scores  float[k]
 *   offsets[2]  top_hits    int32[k]          with labels only
 *               (pad to 8 B)
 *   offsets[3]  di_rank_metrics               with labels only
 *   offsets[4]  di_auc_metrics                with labels only
 *               (pad to 16 B)
 * Every field is made of 4- or 8-byte words and starts on its word size, given a record that starts
 * 16-B aligned; records laid end to end stay 16-B aligned. Returns the record's bytes and, where
 * offsets is not NULL, the five byte offsets from its start (-1 for a field the record does not
 * have). Host arithmetic only: nothing is launched, no device is touched.
 * DI_EINVAL: l1 or l2 < 1, k < 1, k > l1 * l2, with_labels other than 0 / 1. DI_ERANGE:
 * k > DI_RANK_MAX_K, l1 * l2 >= 2^29 (the sizes di_contact_rank refuses, with its codes). */
int64_t di_rank_record_bytes(int32_t l1, int32_t l2, int32_t k, int32_t with_labels,
                             int64_t* offsets /* 5 field offsets, may be NULL */);

/* ---- example lists of a ragged batch (an addition to ABI 8) ---------------------------------
 * The reference's `examples` [n, 3] = (i, j, label) rows of `count` complexes, contiguous, int64
 * (DI_I64) or int32 (DI_I32; one width per call), turned into what the two ops above take: one memset
 * and ONE launch, whatever count is. Tables and grid as for di_contact_rank_batch (host items
 * validated and used for grid sizes; items_dev the caller's device copy).
 *   di_examples_labels_batch  complete lists (n == l1 * l2, every pair exactly once):
 *                             labels[i * l2 + j] = label, uint8 [l1 * l2]
 *   di_examples_gather_batch  sampled lists as LitGINI.validation_step reads them
 *                             (deepinteract_modules.py:1915-1982; n >= 1, any order, repeats allowed):
 *                             pool_logits[c * total + out_off + r] = logits[c, i_r, j_r] (c = 0, 1;
 *                             logits [2, l1, l2] in `dtype`, copied bit for bit) and
 *                             pool_labels[out_off + r] = label_r (uint8). A pool is the reference's
 *                             torch.cat over the complexes of one validation batch: its items carry
 *                             the pool's base pointers and row count `total`, and their own place
 *                             out_off in it. Any number of pools per call.
 * Flags, one int32 per complex, device memory, cleared by the call: DI_EX_OUTSIDE an index outside
 * the complex; DI_EX_LABEL a label other than 0 / 1; DI_EX_TWICE (labels only) a pair listed twice.
 * With n == l1 * l2, no DI_EX_OUTSIDE and no DI_EX_TWICE every pair is covered. The flags are a
 * function of the lists alone (agent-scope atomicOr on a 1-bit-per-pair bitmap, the returned word
 * tested; see csrc/contact_examples.hip). Indices are compared in their own width: 2^40 or -1 is
 * outside. A row that is outside touches no memory but its flag, and writes nothing; a flagged
 * complex's outputs are unspecified, its neighbours' are not affected.
 *   labels: flags are the first `count` words of `work` (di_examples_labels_work_bytes bytes, 16-B
 *   aligned, cleared in-stream by the call); the helper fills work_off (the complex's bitmap), and the
 *   call refuses other values. gather: flags [count] is the caller's.
 * Asynchronous, no allocation, every refusal before any launch; the *_check forms do the same
 * validation on the host, without a launch. DI_EINVAL: count < 1, a NULL table / work / flags, a bad
 * dtype or index width, an item with a NULL pointer its mode uses, n < 1, l1 or l2 < 1, a pointer off
 * its element's alignment, labels with n != l1 * l2 or a work_off the helper did not fill, gather
 * with total < 1 or rows outside the pool (out_off < 0, out_off + n > total). DI_ERANGE:
 * count > DI_BATCH_MAX, l1 * l2 >= 2^29, total >= 2^31. */
enum { DI_I64 = 0, DI_I32 = 1 };
enum { DI_EX_OUTSIDE = 1, DI_EX_LABEL = 2, DI_EX_TWICE = 4 };
#define DI_EX_BLOCK_ROWS 1024   /* rows of one list a block takes (a wave: 64 consecutive rows at a time) */
typedef struct {
  const void* examples;
  const void* logits;
  uint8_t* labels;
  void* pool_logits;
  uint8_t* pool_labels;
  int64_t n, out_off, total, work_off;
  int32_t l1, l2;
} di_examples_item;
int64_t di_examples_labels_work_bytes(di_examples_item* items, int32_t count);
int di_examples_labels_batch(int32_t idx_dtype, const di_examples_item* items, const di_examples_item* items_dev,
                             int32_t count, void* work, void* stream);
int di_examples_labels_batch_check(int32_t idx_dtype, const di_examples_item* items,
                                   const di_examples_item* items_dev, int32_t count, const void* work);
int di_examples_gather_batch(int32_t dtype, int32_t idx_dtype, const di_examples_item* items,
                             const di_examples_item* items_dev, int32_t count, int32_t* flags, void* stream);
int di_examples_gather_batch_check(int32_t dtype, int32_t idx_dtype, const di_examples_item* items,
                                   const di_examples_item* items_dev, int32_t count, const int32_t* flags);

/* ---- interface label maps from atom coordinates (an addition to ABI 8) -----------------------
 * The label map of each of `count` bound complexes from its two chains' heavy atoms, by the
 * definition behind DIPS' pos_idx (deepinteract_utils.py:612: neighbor_def='non_heavy_res',
 * cutoff=6): labels[i * l2 + j] = 1 iff some atom of residue i of chain 0 lies within `cutoff` (<=)
 * of some atom of residue j of chain 1, uint8 [l1 * l2], the map di_contact_rank / di_contact_auc
 * take and di_examples_labels_batch writes. One memset (the stats) and TWO launches, whatever count
 * is. Tables and grid as for di_contact_rank_batch (host items validated and used for grid sizes;
 * items_dev the caller's device copy).
 *   per chain: xyz [a, 3] fp32 heavy-atom coordinates grouped by residue; res_off [l + 1] int32 CSR
 *   offsets into xyz (res_off[0] = 0, non-decreasing, res_off[l] = a).
 * The pair test, to the bit: dx = x0 - x1 (likewise dy, dz), d2 = (dx * dx + dy * dy) + dz * dz,
 * every operation rounded to fp32 and none contracted; contact iff d2 <= c2, c2 =
 * (float)((double)cutoff * (double)cutoff); a comparison against NaN is false. Residue pairs whose
 * bounding spheres (computed centre, largest computed distance from it) are provably farther apart
 * than cutoff are not examined; the margin argument is in csrc/contact_interface.hip. Every byte of
 * every map is written exactly once (no memset of the maps, no atomics on them).
 * work: di_interface_work_bytes bytes, 16-B aligned. Its first `count` 16-byte records are the
 * di_interface_stats of the complexes (cleared in-stream by the call): num_pos = the map's positives,
 * flags = DI_IF_OFFSETS (res_off[0] != 0, a decreasing pair, or res_off[l] != a; every residue's range
 * is clamped into [0, a] before use, so nothing outside xyz is read), DI_IF_EMPTY (a residue with no
 * atoms), DI_IF_NONFINITE (a NaN or Inf coordinate). Both are functions of the input alone (integer
 * adds, ORs of constants). A flagged complex's map is unspecified, but every write stays inside it;
 * its neighbours are not affected. The helper fills work_off (the complex's spheres, after the
 * stats), and the call refuses other values.
 * Asynchronous, no allocation, every refusal before any launch; the _check form does the same
 * validation on the host, without a launch. DI_EINVAL: count < 1, a NULL table / work / item pointer,
 * l1, l2, a0 or a1 < 1, cutoff not finite or not positive, work not 16-B aligned, xyz or res_off not
 * 4-B aligned, a work_off the helper did not fill. DI_ERANGE: count > DI_BATCH_MAX,
 * l1 * l2 >= 2^29, a chain of 2^24 atoms or more. */
enum { DI_IF_OFFSETS = 1, DI_IF_EMPTY = 2, DI_IF_NONFINITE = 4 };
typedef struct {
  const float* xyz0;
  const int32_t* res_off0;
  const float* xyz1;
  const int32_t* res_off1;
  uint8_t* labels;
  int32_t l1, l2, a0, a1;
  int64_t work_off;
} di_interface_item;
typedef struct {
  int64_t num_pos;
  int32_t flags;
  int32_t pad;
} di_interface_stats;
int64_t di_interface_work_bytes(di_interface_item* items, int32_t count);
int di_interface_labels_batch(const di_interface_item* items, const di_interface_item* items_dev, int32_t count,
                              float cutoff, void* work, void* stream);
int di_interface_labels_batch_check(const di_interface_item* items, const di_interface_item* items_dev,
                                    int32_t count, float cutoff, const void* work);

/* ---- residue environment features from atoms (an addition to ABI 8) --------------------------
 * The DIPS-Plus node-feature columns that are functions of a chain's atoms alone, and its amide
 * normals and backbone rows, for each of `count` chains of a ragged batch: one memset (the stats)
 * and THREE launches, whatever count is. Tables and grid as for di_interface_labels_batch.
 *   per chain: xyz [a, 3] fp32 coordinates of ALL atoms grouped by residue (hydrogens too where the
 *   file has them); res_off [l + 1] int32 CSR offsets; role [a] uint8 per atom (DI_ROLE_*); aa [l]
 *   uint8, the index into "ACDEFGHIKLMNPQRSTVWY-" ('-' = 20: not one of the standard twenty);
 *   resname [l] uint8, the one-hot column 0..19 (TRP PHE LYS PRO ASP ALA ARG CYS VAL THR GLY SER
 *   HIS LEU GLU TYR ILE ASN MET GLN; an unknown residue goes to the last).
 * Every residue holds exactly one N, CA, C and O and at most one CB (DI_ENV_BACKBONE otherwise).
 *   nb(i, j): some atom of i and some atom of j have d2 < c2 (STRICT; d2 as in
 *     di_interface_labels_batch, fp32, every operation rounded, none contracted); nb(i, i) always.
 *     The default c2 is DI_ENV_C2 = (float)(8 ln 1000): exp(-d2 / 8) > 1e-3.
 *   CN_i = #{j : nb(i, j)}, self included -> cn_raw [l] int32.
 *   u_i = the mean of the unit vectors from CA to the atoms whose role is not N, CA, C or O; without
 *     such atoms 1/2 [(CA - C) / |CA - C| + (CA - N) / |CA - N|]. fp32; only signs of dot products
 *     with it are used.
 *   j != i with nb(i, j) is UP iff dot(u_i, CA_j - CA_i) > 0, else DOWN (a zero or NaN dot: down);
 *     i itself counts as DOWN. UN_i = #up, DN_i = CN_i - UN_i.
 *   dips [l, 106] fp32, row stride 106; the call writes ONLY these columns and leaves the others:
 *     0:20   the one-hot of resname
 *     36:57  UC[t] = ([t == aa_i] + #{up j: aa_j = t}) / (1 + UN_i), t = 0..20
 *     57:78  DC[t] = ([t == aa_i] + #{down j, i included: aa_j = t}) / (1 + DN_i)
 *     78     (CN_i - min) / (max - min) over the chain, 0 when max == min
 *     every value the fp32 quotient of two integers.
 *   amide_norm [l, 3]: cross(CA - CB, CB - N), every operation rounded to fp32 and none contracted;
 *     zeros without a CB. backbone [l, 4, 3]: the N, CA, C, O coordinates.
 * All counts are integers accumulated with integer adds, so every output is a function of the input
 * alone, whatever the schedule. Residue pairs whose bounding spheres are provably farther apart than
 * sqrt(c2) are not examined (csrc/atom_pairs.h, the argument in csrc/contact_interface.hip).
 * work: di_residue_env_work_bytes bytes, 16-B aligned. Its first `count` 16-byte records are the
 * di_env_stats of the chains (cleared in-stream by the call): flags = DI_ENV_OFFSETS / DI_ENV_EMPTY
 * / DI_ENV_NONFINITE as DI_IF_* (ranges are clamped into [0, a] before use: nothing outside the
 * chain's arrays is read), DI_ENV_BACKBONE (a role > 5, an aa > 20, a resname > 19, or a residue
 * without exactly one N, CA, C, O and at most one CB); cn_max = max CN; cn_min_gap = l - min CN.
 * A flagged chain's outputs are unspecified but every write stays inside its own buffers; its
 * neighbours in the batch are not affected. The helper fills work_off, and the call refuses others.
 * Asynchronous, no allocation, every refusal before any launch; the _check form validates on the
 * host without a launch. DI_EINVAL: count < 1, a NULL table / work / item pointer, l or a < 1, c2 not
 * finite or not positive, work not 16-B aligned, xyz / res_off / dips / amide_norm / backbone /
 * cn_raw not 4-B aligned, a work_off the helper did not fill. DI_ERANGE: count > DI_BATCH_MAX, a
 * chain of 2^24 atoms or residues or more. */
#define DI_ENV_C2 55.262043f
enum { DI_ROLE_OTHER = 0, DI_ROLE_N = 1, DI_ROLE_CA = 2, DI_ROLE_C = 3, DI_ROLE_O = 4, DI_ROLE_CB = 5 };
enum { DI_ENV_OFFSETS = 1, DI_ENV_EMPTY = 2, DI_ENV_NONFINITE = 4, DI_ENV_BACKBONE = 8 };
typedef struct {
  const float* xyz;
  const int32_t* res_off;
  const uint8_t* role;
  const uint8_t* aa;
  const uint8_t* resname;
  float* dips;
  float* amide_norm;
  float* backbone;
  int32_t* cn_raw;
  int32_t l, a;
  int64_t work_off;
} di_env_item;
typedef struct {
  int32_t flags;
  int32_t cn_max;
  int32_t cn_min_gap;
  int32_t pad;
} di_env_stats;
int64_t di_residue_env_work_bytes(di_env_item* items, int32_t count);
int di_residue_env_batch(const di_env_item* items, const di_env_item* items_dev, int32_t count, float c2,
                         void* work, void* stream);
int di_residue_env_batch_check(const di_env_item* items, const di_env_item* items_dev, int32_t count, float c2,
                               const void* work);

/* ---- graph builder ----------------------------------------------------------------------- */
/* Cα kNN per chain: idx_out [Nt,k] chain-local neighbour ids (ascending squared distance,
 * self first), d2_out [Nt,k] the expansion-formula squared distances. node_off [G+1] device. */
int di_knn_topk(int32_t num_graphs, const int32_t* node_off, const float* ca /*[Nt,3]*/, int32_t k,
                int32_t max_nodes, int32_t* idx_out, float* d2_out, void* stream);

/* kNN graph topology of every chain from di_knn_topk's idx ([DGL-ASSUMPTION] DGL 0.6 knn_graph
 * edge order, graph_utils.py:107): edge e = v*k + r has src = idx[v,r] + node_off[g] and dst = v
 * (global ids); in_ptr_out [Nt+1] = v*k; node_pos_out [Nt] = v - node_off[g]. */
int di_knn_graph(int32_t num_graphs, const int32_t* node_off, int32_t k, const int32_t* knn_idx,
                 int32_t num_nodes, int32_t* src_out, int32_t* dst_out, int32_t* in_ptr_out,
                 int32_t* node_pos_out, void* stream);

typedef struct {
  int32_t num_graphs, k, max_nodes;
  const int32_t* node_off;   /* [G+1] */
  const float* backbone;     /* [Nt,4,3] N, CA, C, O */
  const float* amide_norm;   /* [Nt,3] */
  const float* dips;         /* [Nt,106] DIPS-Plus residue features */
  const int32_t* knn_idx;    /* [Nt,k] chain-local (di_knn_topk) */
  const float* knn_d2;       /* [Nt,k] */
  float* node_f;             /* out [Nt,113] */
  float* edge_f;             /* out [Nt*k,28] */
  float* stats;              /* workspace [G,4] */
} di_geo_args;
int di_geo_feats(const di_geo_args* args, void* stream);

/* neighbour-edge ids: 2 distinct in-edges of src(e) and of dst(e), uniform, counter-based RNG
 * (seed, e); nbr_out [Et,4] global edge ids in the di_graph.nbr layout. */
int di_build_nbr_ids(int32_t num_edges, const int32_t* src, const int32_t* dst, const int32_t* in_ptr,
                     uint64_t seed, int32_t* nbr_out, void* stream);

/* neighbour-edge ids bit-exact with the reference's torch.randperm draws
 * (deepinteract_utils.py:539-546): chain g's ids are those convert_df_to_dgl_graph produces right
 * after torch.manual_seed(seeds[g]) (torch CPU generator = mt19937; randperm = Fisher-Yates, E src
 * calls then E dst calls). kNN graphs only (uniform in-degree k, dst-major edges, k >= 3).
 * node_off [G+1], seeds [G] (device); num_nodes = node_off[G]; src/dst [Et = num_nodes*k] global
 * node ids; nbr_out [Et,4] global ids. Two launches: the per-chain mt19937 streams (one wave per
 * chain) write the kept in-edge positions, then every id gets its endpoint's in-edge base.
 * DI_ERANGE when 2 * num_nodes * k * (k-1) exceeds INT32_MAX (a chain's draw count is int32). */
int di_build_nbr_ids_torch(int32_t num_graphs, const int32_t* node_off, int32_t k, const uint64_t* seeds,
                           int32_t num_nodes, const int32_t* src, const int32_t* dst, int32_t* nbr_out, void* stream);

/* ---- module-at-a-time API ---------------------------------------------------------------- */
/* ConformationModule alone (kind-6 blob): conf_out [Et,128] = F + SiLU(final_linear(...)), from the
 * current edge features f_in [Et,128] and fn_in = SiLU(nbr_linear(f_in)) [Et,128]. */
int di_conformation(const di_graph* g, di_dtype dt, const float* edge_f /*[Et,28]*/, const void* f_in,
                    const void* fn_in, const void* wmat, const float* wvec, void* conf_out, void* stream);

/* y[r,:] = res[r,:] + act(W x[r,:] + bias) for r < rows; W packed in the natural-k fragment order
 * (packing.pack_matrix_natural: out_dim % 16 == 0, in_dim padded to 32). act: 0 none, 1 SiLU.
 * bias / res may be NULL. x, res, y in the storage dtype; bias fp32. */
int di_gemm_bias_act(di_dtype dt, int32_t rows, int32_t in_dim, int32_t out_dim, const void* x, int32_t x_ld,
                     const void* w_packed, const float* bias, int32_t act, const void* res, int32_t res_ld,
                     void* y, int32_t y_ld, void* stream);

/* qkv [Nt,384] = Q|K|V, proj_e [Et,128]: e_out [Et,128] (NULL: not produced), alpha_out [Et,4]
 * (fp32, exp(clamp(sum score))), h_out [Nt,128] = sum alpha V[src] / (sum alpha + 1e-6). */
int di_geo_attention(const di_graph* g, di_dtype dt, const void* qkv, const void* proj_e, void* e_out,
                     float* alpha_out, void* h_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DEEPINTERACT_AMD_H */
