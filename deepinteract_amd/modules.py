"""Reference-interface modules over the HIP kernels.

Mirrors the Python API the reference's hot path exposes (deepinteract_modules.py):

* ``DGLGeometricTransformer.forward(graph) -> graph`` (:1426-1466): reads ndata['f'] [N,128],
  edata['f'] [E,28], edata['src_nbr_e_ids'|'dst_nbr_e_ids'] [E,2]; writes ndata['f'] [N,128]
  and edata['f'] [E,128] (the last intermediate layer's edges) in place, keeps batch_num_*.
* ``LitGINI`` (:1478): ``gnn_forward`` (:1660-1679), ``shared_step`` (:1687-1745),
  ``predict_step`` (:2178-2184), ``test_step`` (:2018-2101), plus ``predict_batch`` (the batched
  entry the benchmark and the distributed driver use), ``predict_contacts`` (the same with each
  complex's ranked contacts), ``test_batch`` (test_step's figures for many complexes at once),
  ``test_epoch_end`` (:2103-2165, the medians and the top-k CSV), ``validation_step`` (:1915-1982, the
  same figures on sampled example lists, a batch's complexes pooled), ``validation_batch`` (one such
  dict per complex at once) and ``validation_epoch_end`` (:1984-2016, the medians).

Graphs may be ``deepinteract_amd.graph.ResidueGraph`` or real ``dgl.DGLGraph`` objects.
Batched graphs get per-chain semantics (each chain as the reference computes it at batch size 1).
Weights come from a reference-keyed state dict (``load_reference_state_dict``); the GeoT part
is packed once into device blobs, the head is a regular torch module.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .config import GeoTConfig, NODE_COUNT_LIMIT, RESIDUE_COUNT_LIMIT
from .engine import GeoTEngine, HeadPrologueOp, PairTensorOp, gpu_device
from .graph import GraphBatch, ResidueGraph, batch as batch_graphs, unbatch
from .head import HeadBatch, HeadConvOps, HeadNormOps, ResNet2DInputWithOptAttention, contact_probs
from ._lib import DI_RANK_MAX_K
from .ranking import (ContactAucOp, ContactRankOp, ExamplesOp, InterfaceOp, confusion_metrics, labels_from_examples,
                      labels_from_examples_batch, pooled_topk_metrics, topk_metrics)


def _identity_embedding_sd(sd, cfg: GeoTConfig):
    """Standalone DGLGeometricTransformer: node features arrive already embedded (128-d);
    reuse the fused embed kernel with an identity node_in_embedding."""
    out = {k: v for k, v in sd.items()}
    out["node_in_embedding.weight"] = torch.eye(cfg.num_gnn_hidden_channels)
    return out


def _graph_list(graph):
    if hasattr(graph, "batch_num_nodes") and len(graph.batch_num_nodes()) > 1:
        return unbatch(graph) if isinstance(graph, ResidueGraph) else __import__("dgl").unbatch(graph)
    return [graph]


class DGLGeometricTransformer(nn.Module):
    """Drop-in for deepinteract_modules.DGLGeometricTransformer (eval-mode forward)."""

    def __init__(self, node_count_limit=NODE_COUNT_LIMIT, num_hidden_channels=128, num_attention_heads=4,
                 knn=20, num_layers=4, dtype="f32", disable_geometric_mode=False, **kwargs):
        super().__init__()
        self.cfg = GeoTConfig(num_gnn_layers=num_layers, num_gnn_hidden_channels=num_hidden_channels,
                              num_gnn_attention_heads=num_attention_heads, knn=knn,
                              node_count_limit=node_count_limit, num_node_input_feats=num_hidden_channels,
                              disable_geometric_mode=bool(disable_geometric_mode))
        if num_hidden_channels != 128 or num_attention_heads != 4:
            raise NotImplementedError("kernels are specialised for 128 hidden channels, 4 heads")
        if node_count_limit <= 0:
            raise ValueError("max_num_graph_nodes must be positive")
        self.dtype = dtype
        self.engine = None

    def load_reference_state_dict(self, sd, prefix="gnn_module.0."):
        """Keys as in LitGINI's state dict; prefix strips to this module's own keys."""
        full = {("gnn_module.0." + k[len(prefix):]) if k.startswith(prefix) else k: v for k, v in sd.items()}
        self.engine = GeoTEngine(_identity_embedding_sd(full, self.cfg), self.dtype, self.cfg)
        return self

    def forward(self, graph):
        if self.engine is None:
            raise RuntimeError("load_reference_state_dict() first")
        bnn, bne = graph.batch_num_nodes(), graph.batch_num_edges()
        gb = GraphBatch.from_graphs(_graph_list(graph), device=self.engine.device,
                                     node_count_limit=self.cfg.node_count_limit)
        h, e = self.engine.forward(gb)
        graph.ndata["f"] = h.to(torch.float32) if self.dtype == "f32" else h
        graph.edata["f"] = e.to(torch.float32) if self.dtype == "f32" else e
        graph.set_batch_num_nodes(bnn)
        graph.set_batch_num_edges(bne)
        return graph


class LitGINI(nn.Module):
    """Inference-side drop-in for LitGINI (GeoT on HIP kernels, dilated-ResNet head on torch)."""

    def __init__(self, num_node_input_feats=113, num_gnn_layers=2, num_gnn_hidden_channels=128,
                 num_gnn_attention_heads=4, knn=20, num_interact_layers=14, num_interact_hidden_channels=128,
                 num_classes=2, max_num_graph_nodes=NODE_COUNT_LIMIT, max_num_residues=RESIDUE_COUNT_LIMIT,
                 dtype="f32", head_dtype=torch.float32, precise_head=False, fuse_head_prologue=False,
                 head_channels_last=False, head_hip_ops=True, head_convs="torch", pos_prob_threshold=0.5,
                 head_batch=0, head_batch_pixels=2 ** 22, head_body="python", use_interact_attention=False,
                 num_interact_attention_heads=4, disable_geometric_mode=False, head_batch_f32=0, **kwargs):
        super().__init__()
        # disable_geometric_mode (the reference's --disable_geometric_mode): the plain Graph Transformer
        # baseline in the GeoT's place, on its own HIP edge kernels (GeoTConfig, csrc/geot_plain.hip)
        # use_interact_attention / num_interact_attention_heads (the reference's --use_interact_attention,
        # --num_interact_attention_heads): a MultiHeadRegionalAttention block behind each of the head's two
        # ResNets (MHA2D_1, MHA2D_2), on HIP with head_hip_ops (head.HeadAttnOps) and on torch otherwise
        use_interact_attention = bool(use_interact_attention)
        if use_interact_attention and int(num_interact_attention_heads) != 4:
            # q / k / v are 16- / 16- / 128-channel convolutions whatever the head count, so a checkpoint
            # trained with another head count would load and silently compute 4-head attention
            raise NotImplementedError("the head's regional attention is specialised for 4 heads")
        if use_interact_attention and head_body == "native":
            raise ValueError('head_body="native" does not run the regional attention (di_head_body_batch has no '
                             'attention stage); use head_body="python"')
        if num_gnn_hidden_channels != 128 or num_gnn_attention_heads != 4:
            # Q/K/V are Linear(H, H) whatever the head count, so a checkpoint trained with another
            # head count would load and silently compute 4-head attention
            raise NotImplementedError("the GeoT kernels are specialised for 128 hidden channels, 4 heads")
        if max_num_graph_nodes <= 0:
            # the GeoT kernels need only node_pos < max_num_graph_nodes (the positional table's rows);
            # the on-device graph builder's own chain limit (4096) is enforced where it is used
            raise ValueError("max_num_graph_nodes must be positive")
        self.cfg = GeoTConfig(num_node_input_feats=num_node_input_feats, num_gnn_layers=num_gnn_layers,
                              num_gnn_hidden_channels=num_gnn_hidden_channels,
                              num_gnn_attention_heads=num_gnn_attention_heads, knn=knn,
                              node_count_limit=max_num_graph_nodes,
                              num_interact_layers=num_interact_layers,
                              num_interact_hidden_channels=num_interact_hidden_channels, num_classes=num_classes,
                              use_interact_attention=use_interact_attention,
                              num_interact_attention_heads=int(num_interact_attention_heads),
                              disable_geometric_mode=bool(disable_geometric_mode))
        self.dtype = dtype
        self.head_dtype = head_dtype
        # precise_head: run the head's convolutions without MIOpen's fast algorithms (Winograd /
        # FFT variants drift ~1e-3 relative over the 58 residual blocks); GEMM-based fp32 convs
        # keep logits within 1e-4 of the reference CPU path.
        self.precise_head = precise_head
        # fuse_head_prologue: ELU(inorm_1(conv2d_1(T))) straight from the node features on HIP
        # (di_head_prologue), never materialising the [2H, L1, L2] pair tensor T
        self.fuse_head_prologue = fuse_head_prologue
        # head_dtype / head_channels_last: the dilated-ResNet head's parameters and activations in
        # head_dtype (bf16: MIOpen bf16 convolutions, fp32 accumulation) and NHWC memory layout
        # (SURVEY §8f-3); the fp32 NCHW default is the parity configuration
        self.head_channels_last = head_channels_last
        # head_hip_ops: the head's InstanceNorm+ELU and SE-gate+residual passes on HIP
        # (head.HeadNormOps; NCHW only, so not with head_channels_last)
        self.head_hip_ops = head_hip_ops and not head_channels_last
        # head_convs: "torch" (MIOpen), or the ResNets' 1x1 / dilated 3x3 convolutions on the matrix cores
        # with the norm + ELU fused into their loads (head.HeadConvOps), NCHW only: "hip" for the bf16 head
        # (di_head_conv), "hip_f32" for the fp32 one (di_head_conv_f32: fp32 storage, f32-input MFMA; one
        # complex at a time, or in chunks with head_batch_f32 -- head_batch and the native body are bf16 only).
        if head_convs not in ("torch", "hip", "hip_f32"):
            raise ValueError(f'head_convs must be "torch", "hip" or "hip_f32", got {head_convs!r}')
        if head_convs == "hip" and (head_dtype != torch.bfloat16 or not head_hip_ops or head_channels_last):
            raise ValueError('head_convs="hip" needs head_dtype=torch.bfloat16, head_hip_ops=True and no '
                             "head_channels_last")
        if head_convs == "hip_f32" and (head_dtype != torch.float32 or not head_hip_ops or head_channels_last):
            raise ValueError('head_convs="hip_f32" needs head_dtype=torch.float32, head_hip_ops=True and no '
                             "head_channels_last")
        if head_convs == "hip_f32" and (int(head_batch) > 0 or head_body == "native"):
            raise ValueError('head_convs="hip_f32" runs one complex at a time: head_batch > 0 and '
                             'head_body="native" are the bf16-only batch (head_convs="hip")')
        self.head_convs = head_convs
        # head_batch: N > 0 sends _forward_batch's complexes through the head's blocks in chunks of at
        # most N complexes and at most head_batch_pixels pixels (L1 * L2 summed), every head kernel
        # launched once per chunk (head.HeadBatch, body_batch). The chunk's arena takes 768 B per
        # pixel, so the default cap keeps it at 3 GiB; a complex larger than the cap goes alone.
        head_batch, head_batch_pixels = int(head_batch), int(head_batch_pixels)
        if head_batch < 0 or head_batch_pixels < 1:
            raise ValueError("head_batch must be >= 0 and head_batch_pixels >= 1")
        if head_batch > 0 and head_convs != "hip":
            raise ValueError('head_batch > 0 needs head_convs="hip" (the batched head runs on the HIP convolutions)')
        self.head_batch, self.head_batch_pixels = head_batch, head_batch_pixels
        # head_batch_f32: head_batch for the fp32 parity head (head_convs="hip_f32"): N > 0 sends
        # _forward_batch's complexes through the fp32 head's blocks in chunks of at most N complexes and at
        # most head_batch_pixels pixels, every head kernel launched once per chunk (di_head_conv_f32_batch,
        # di_plane_stats_f32_batch, di_se_scale_add_f32_batch). The fp32 arena takes 1536 B per pixel, so
        # the default head_batch_pixels = 2**22 means 6 GiB: lower it where that is too much. A complex's
        # logits are the same bits whatever else its chunk holds; they differ from head_batch_f32=0's in
        # the last bits (the SE gate comes from di_se_gate's fp32 fmaf chain, not torch's fp32 linears).
        head_batch_f32 = int(head_batch_f32)
        if head_batch_f32 < 0:
            raise ValueError("head_batch_f32 must be >= 0")
        if head_batch_f32 > 0 and head_convs != "hip_f32":
            raise ValueError('head_batch_f32 > 0 needs head_convs="hip_f32" (the batched fp32 head runs on the fp32 '
                             'HIP convolutions; the bf16 head takes head_batch)')
        self.head_batch_f32 = head_batch_f32
        # head_body: "python" issues the batched head's launches from ResNet._forward_hipconv_batch;
        # "native" issues the same launches from one C call per chunk (di_head_body_batch) and takes the
        # logits from one HIP launch (di_head_logits_batch). Same bits up to phase2_conv's input; it takes
        # the interpreter out from between the ~600 launches, which is worth 9 % on one 64 x 64 complex and
        # about nothing from 145 x 145 up, where the kernels' own time is the floor.
        # With head_batch=0 every complex goes through as a chunk of one.
        if head_body not in ("python", "native"):
            raise ValueError(f'head_body must be "python" or "native", got {head_body!r}')
        if head_body == "native" and head_convs != "hip":
            raise ValueError('head_body="native" needs head_convs="hip" (it runs the HIP convolutions\' launches)')
        self.head_body = head_body
        self.max_num_residues = max_num_residues
        # pos_prob_threshold: a contact is predicted where its probability reaches it (test_step's
        # rounded predictions and confusion counts; the reference's default)
        self.pos_prob_threshold = float(pos_prob_threshold)
        self.interact_module = ResNet2DInputWithOptAttention(num_interact_layers, 2 * num_gnn_hidden_channels,
                                                             num_interact_hidden_channels, num_classes,
                                                             use_attention=use_interact_attention,
                                                             n_head=int(num_interact_attention_heads))
        self._geot_sd = None     # GeoT part of the reference state dict (host copy)
        self._prologue_w = None  # fp32 host copies of conv2d_1 / inorm_1 (fused head prologue)
        self._dev_ops = None     # (device, GeoTEngine, PairTensorOp, HeadPrologueOp | None)
        self._rank_op = None     # ContactRankOp on the model's device
        self._auc_op = None      # ContactAucOp on the model's device
        self._examples_op = None  # ExamplesOp on the model's device
        self._interface_op = None  # InterfaceOp on the model's device

    def load_reference_state_dict(self, sd):
        """Reference-keyed LitGINI state dict. The head loads into this nn.Module; the GeoT
        weights are kept on the host and packed for the GPU the model lives on at first use
        (so ``load`` on the CPU followed by ``.cuda()``, as lit_model_predict.py:214 does, works)."""
        head = {k[len("interact_module."):]: v for k, v in sd.items() if k.startswith("interact_module.")}
        self.interact_module.load_state_dict(head)
        self._geot_sd = {k: v.detach().to("cpu", copy=True) for k, v in sd.items()
                         if not k.startswith("interact_module.")}
        m = self.interact_module
        self._prologue_w = tuple(t.detach().to("cpu", torch.float32, copy=True) for t in
                                 (m.conv2d_1.weight, m.conv2d_1.bias, m.inorm_1.weight, m.inorm_1.bias))
        self._prologue_eps = m.inorm_1.eps
        self.interact_module.to(dtype=self.head_dtype)
        if self.head_channels_last:
            self.interact_module.to(memory_format=torch.channels_last)
        self._dev_ops = None
        return self

    def _ops(self):
        """(GeoTEngine, PairTensorOp, HeadPrologueOp | None) on the device of the model's
        parameters, (re)built when the model has moved. A model on the CPU raises: the kernels
        take device pointers only (no CPU fallback)."""
        if self._geot_sd is None:
            raise RuntimeError("load_reference_state_dict() / load_from_checkpoint() first")
        dev = gpu_device(next(self.interact_module.parameters()).device)
        if self._dev_ops is None or self._dev_ops[0] != dev:
            self._dev_ops = None
            eng = GeoTEngine(self._geot_sd, self.dtype, self.cfg, device=dev)
            pair = PairTensorOp(dev)
            pro = HeadPrologueOp(*self._prologue_w, self._prologue_eps, dev) if self.fuse_head_prologue else None
            self.interact_module.use_hip_norm_ops(HeadNormOps(dev) if self.head_hip_ops else None)
            self.interact_module.use_hip_convs(HeadConvOps(dev) if self.head_convs in ("hip", "hip_f32") else None)
            self._dev_ops = (dev, eng, pair, pro)
        return self._dev_ops[1:]

    @property
    def engine(self):
        return self._ops()[0]

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, map_location=None, strict=True, safe_globals=None, **kwargs):
        """LightningModule.load_from_checkpoint as lit_model_predict.py:214-219 calls it: build the
        network from the checkpoint's hyper-parameters (shapes inferred from the state dict where
        absent) and load its ``state_dict``. ``kwargs`` override hyper-parameters; the reference's
        training-only overrides (use_wandb_logger, batch_size, lr, weight_decay, dropout_rate) are
        accepted and have no effect on inference. The file is read with ``torch.load(weights_only=
        True)`` (``weights.read_checkpoint``). strict: every key this build needs must be present
        with its shape; keys outside node_in_embedding / gnn_module / interact_module are ignored."""
        from .weights import check_state_dict, infer_config, read_checkpoint
        sd, arch = read_checkpoint(checkpoint_path, safe_globals=safe_globals)
        net_prefixes = ("node_in_embedding.", "gnn_module.", "interact_module.")
        sd = type(sd)((k, v) for k, v in sd.items() if k.startswith(net_prefixes))
        arch.update({k: v for k, v in kwargs.items() if k in arch or k.startswith("num_") or k in ("knn", "use_interact_attention", "disable_geometric_mode")})
        cfg = infer_config(sd, **arch)
        problems = check_state_dict(sd, cfg)
        if strict and problems:
            raise RuntimeError(f"{checkpoint_path}: state dict does not match LitGINI ({len(problems)} problems): "
                               + "; ".join(problems[:8]))
        opts = {k: kwargs[k] for k in ("dtype", "head_dtype", "precise_head", "fuse_head_prologue",
                                       "head_channels_last", "head_hip_ops", "head_convs", "head_batch",
                                       "head_batch_pixels", "head_body", "head_batch_f32") if k in kwargs}
        model = cls(num_node_input_feats=cfg.num_node_input_feats, num_gnn_layers=cfg.num_gnn_layers,
                    num_gnn_hidden_channels=cfg.num_gnn_hidden_channels,
                    num_gnn_attention_heads=cfg.num_gnn_attention_heads, knn=cfg.knn,
                    num_interact_layers=cfg.num_interact_layers,
                    num_interact_hidden_channels=cfg.num_interact_hidden_channels, num_classes=cfg.num_classes,
                    max_num_graph_nodes=cfg.node_count_limit,
                    use_interact_attention=cfg.use_interact_attention,
                    num_interact_attention_heads=cfg.num_interact_attention_heads,
                    disable_geometric_mode=cfg.disable_geometric_mode,
                    max_num_residues=int(arch.get("max_num_residues", RESIDUE_COUNT_LIMIT)), **opts)
        if map_location is not None:
            model = model.to(map_location)
        return model.eval().load_reference_state_dict(sd)

    def freeze(self):
        """LightningModule.freeze (lit_model_predict.py:220): eval mode, no gradients."""
        for p in self.parameters():
            p.requires_grad_(False)
        return self.eval()

    # --- reference API ------------------------------------------------------------------
    def gnn_forward(self, graph):
        """node_in_embedding + GeoT for a (batched) graph; returns per-graph node features and
        writes ndata['f'] / edata['f'] like the reference (:1660-1679)."""
        graphs = _graph_list(graph)
        eng = self.engine
        gb = GraphBatch.from_graphs(graphs, device=eng.device, node_count_limit=self.cfg.node_count_limit)
        h, e = eng.forward(gb)
        graph.ndata["f"], graph.edata["f"] = h, e
        return [h[a:b] for a, b in zip(gb.node_off[:-1], gb.node_off[1:])]

    def interact_forward(self, interact_tensor, prologue_done=False):
        """Head on an interaction tensor; prologue_done: the input is already
        ELU(inorm_1(conv2d_1(T))) (HeadPrologueOp)."""
        x = interact_tensor.to(self.head_dtype)
        if self.head_channels_last:
            x = x.contiguous(memory_format=torch.channels_last)
        fn = self.interact_module.body if prologue_done else self.interact_module
        if self.precise_head:
            with torch.backends.cudnn.flags(enabled=False):
                return fn(x)
        return fn(x)

    def shared_step(self, graph1, graph2, return_representations=False):
        g1s, g2s = _graph_list(graph1), _graph_list(graph2)
        gb = GraphBatch.from_graphs(g1s + g2s, device=self.engine.device,
                                     node_count_limit=self.cfg.node_count_limit)
        logits_list, h, e = self._forward_batch(gb, [(i, len(g1s) + i) for i in range(len(g1s))])
        n1 = gb.node_off[len(g1s)]
        e1 = gb.edge_off[len(g1s)]
        graph1.ndata["f"], graph1.edata["f"] = h[:n1], e[:e1]
        graph2.ndata["f"], graph2.edata["f"] = h[n1:], e[e1:]
        if return_representations:
            np_ = lambda t: t.detach().float().cpu().numpy()  # noqa: E731
            return logits_list, np_(h[:n1]), np_(e[:e1]), np_(h[n1:]), np_(e[e1:])
        return logits_list

    def predict_step(self, batch, batch_idx=0, dataloader_idx=None):
        graph1, graph2 = batch[0], batch[1]
        return self.shared_step(graph1, graph2, return_representations=True)

    # --- batched entry ------------------------------------------------------------------
    def _forward_batch(self, gb: GraphBatch, pairs):
        eng, pair_op, prologue_op = self._ops()
        h, e = eng.forward(gb)
        off = gb.node_off
        h1r = [off[a] for a, _ in pairs]
        h2r = [off[b] for _, b in pairs]
        l1 = [gb.nodes_per_graph[a] for a, _ in pairs]
        l2 = [gb.nodes_per_graph[b] for _, b in pairs]
        batched = self.head_batch > 0 or self.head_batch_f32 > 0 or self.head_body == "native"
        if prologue_op is not None and self.head_body == "native" and h.dtype == torch.bfloat16:
            logits = self._head_native_fused(prologue_op, h, h1r, h2r, l1, l2)
        elif prologue_op is not None:
            _, views = prologue_op(h, h1r, h2r, l1, l2)
            logits = self._head_batched(views, True) if batched else \
                [self.interact_forward(v, prologue_done=True) for v in views]
        else:
            _, views = pair_op(h, h1r, h2r, l1, l2, hT=eng.last_hT)
            logits = self._head_batched(views, False) if batched else \
                [self.interact_forward(v) for v in views]
        return logits, h, e

    def _head_chunks(self, shapes):
        """Consecutive complexes in chunks of at most head_batch (an fp32 head: head_batch_f32) complexes and
        head_batch_pixels pixels."""
        chunks, cur, px = [], [], 0
        # head_batch=0 with head_body="native": chunks of one; at most one of the two counts is set
        most = max(1, self.head_batch, self.head_batch_f32)
        for i, (a, b) in enumerate(shapes):
            if cur and (len(cur) == most or px + a * b > self.head_batch_pixels):
                chunks.append(cur)
                cur, px = [], 0
            cur.append(i)
            px += a * b
        if cur:
            chunks.append(cur)
        return chunks

    def _head_batched(self, views, prologue_done):
        """The head over the complexes' views chunk by chunk (head_batch / head_batch_f32 > 0): the prologue per
        complex, written straight into the chunk's arena, then the blocks once for the whole chunk."""
        import contextlib
        im = self.interact_module
        logits = []
        # precise_head: conv2d_1 and phase2_conv (the two convolutions left on torch) as interact_forward
        with torch.backends.cudnn.flags(enabled=False) if self.precise_head else contextlib.nullcontext():
            for chunk in self._head_chunks([tuple(v.shape[2:]) for v in views]):
                hb = HeadBatch([views[i].shape[2:] for i in chunk], views[chunk[0]].device, dtype=self.head_dtype)
                for slot, i in enumerate(chunk):
                    if prologue_done:
                        hb.input(slot).copy_(views[i])
                    else:
                        im.ops.inorm_elu(im.conv2d_1(views[i].to(self.head_dtype)), im.inorm_1, out=hb.input(slot))
                logits += im.body_batch(hb, native=self.head_body == "native")
        return logits

    def _head_native_fused(self, prologue_op, h, h1r, h2r, l1, l2):
        """head_body="native" behind the fused prologue on bf16 node features: HeadPrologueOp writes a
        whole chunk straight into its arena's input buffer (its packed C * L1 * L2 offsets are the
        HeadBatch layout), so a chunk is three C calls and no per-complex launch or copy."""
        im = self.interact_module
        logits = []
        for chunk in self._head_chunks(list(zip(l1, l2))):
            hb = HeadBatch([(l1[i], l2[i]) for i in chunk], h.device)
            prologue_op(h, *([v[i] for i in chunk] for v in (h1r, h2r, l1, l2)), out=hb.wide[0])
            logits += im.body_batch(hb, native=True)
        return logits

    def predict_batch(self, gb: GraphBatch, pairs):
        """pairs: (chain-1 graph index, chain-2 graph index) per complex -> (logits, probs)."""
        logits, _, _ = self._forward_batch(gb, pairs)
        return logits, [contact_probs(lg) for lg in logits]

    def _ranker(self):
        dev = self.engine.device
        if self._rank_op is None or self._rank_op.device != dev:
            self._rank_op = ContactRankOp(dev)
        return self._rank_op

    def _auc(self):
        dev = self.engine.device
        if self._auc_op is None or self._auc_op.device != dev:
            self._auc_op = ContactAucOp(dev)
        return self._auc_op

    def predict_contacts(self, gb: GraphBatch, pairs, k=None):
        """predict_batch with each complex's ranked contacts: (logits, [ranking.ContactRanking]) --
        the probability map, the k best contacts (default k = min(L1, L2)) as flat ids, (i, j) pairs
        and scores; probability descending, ties by ascending index, NaN first (ranking.py)."""
        logits, _, _ = self._forward_batch(gb, pairs)
        rank = self._ranker()
        return logits, [rank(lg.contiguous(), k=k) for lg in logits]

    def test_step(self, batch, batch_idx=0):
        """LitGINI.test_step (deepinteract_modules.py:2018-2101). batch = (graph1, graph2,
        examples_list, filepaths); examples_list[i] is complex i's [L1 * L2, 3] (i, j, label) rows,
        every pair exactly once. As in the reference, the figures are those of one complex per batch;
        for a batch of several this returns the first complex's top-k figures and maps, and loss and
        confusion over all of them.

        Returns the reference's keys this build computes: loss (mean cross-entropy), top_10_prec,
        top_l_by_10_prec, top_l_by_5_prec, top_l_recall, top_l_by_2_recall, top_l_by_5_recall
        (l = min(L1, L2); float('nan') where the reference would divide by zero, ranking.topk_metrics),
        test_preds / test_preds_rounded / test_labels as [L1, L2] numpy arrays, target,
        confusion = {tp, fp, fn, tn} at pos_prob_threshold, test_auroc / test_auprc (the first complex's
        exact class-1 AUROC and average precision of test_preds against test_labels,
        ranking.ContactAucOp; float('nan') when a class is empty or a score is NaN), and test_acc /
        test_prec / test_recall / test_f1 from the summed confusion counts (torchmetrics' class-1
        definitions restated, ranking.confusion_metrics)."""
        import os
        graph1, graph2, examples_list, filepaths = batch[0], batch[1], batch[2], batch[3]
        logits_list = self.shared_step(graph1, graph2)
        if len(examples_list) != len(logits_list):
            raise ValueError("test_step: one examples tensor per complex")
        rank = self._ranker()
        results = []
        for logits, examples in zip(logits_list, examples_list):
            l1, l2 = int(logits.shape[2]), int(logits.shape[3])
            labels = labels_from_examples(examples.to(rank.device), l1, l2)
            results.append((rank(logits.contiguous(), k=min(l1, l2), labels=labels,
                                 threshold=self.pos_prob_threshold), labels, l1, l2))
        r0, labels0, l1, l2 = results[0]
        auc = self._auc()(r0.probs, labels0)   # the map the ranking judged
        n_all = sum(a * b for _, _, a, b in results)
        confusion = {f: sum(getattr(r, f) for r, _, _, _ in results) for f in ("tp", "fp", "fn", "tn")}
        out = {"loss": sum(r.ce_sum for r, _, _, _ in results) / n_all}
        out.update(topk_metrics(r0.hits.cpu(), r0.num_pos, min(l1, l2)))
        preds = r0.probs
        out["test_preds"] = preds.cpu().numpy()
        out["test_preds_rounded"] = (preds >= self.pos_prob_threshold).float().cpu().numpy()
        out["test_labels"] = labels0.view(l1, l2).float().cpu().numpy()
        out["target"] = str(filepaths[0]).split(os.sep)[-1][:4]
        out["confusion"] = confusion
        out["test_auroc"], out["test_auprc"] = auc.auroc, auc.auprc
        out.update(confusion_metrics(**confusion))
        return out

    def test_batch(self, gb: GraphBatch, pairs, examples_list, filepaths, keep_maps=None):
        """test_step for many complexes at once: one forward (``_forward_batch``), one batched ranking
        call and one batched AUC call (ranking.ContactRankOp.batch / ContactAucOp.batch), whatever
        the number of complexes. pairs as in ``predict_batch``; examples_list[i] / filepaths[i] belong
        to complex i.

        Returns one dict per complex with exactly test_step's keys, every figure that complex's own:
        loss (its mean cross-entropy), the six top_* figures, confusion, test_auroc / test_auprc,
        test_acc .. test_f1 from its confusion counts, target. test_preds / test_preds_rounded /
        test_labels are copied to the host only for the first ``keep_maps`` complexes (None: all; the
        reference keeps 55 of an epoch); the other dicts hold None there. The host reads the device
        once for the labels' validation, once per metrics table and once for all top_hits."""
        if not (len(pairs) == len(examples_list) == len(filepaths)):
            raise ValueError("test_batch: one examples tensor and one file path per complex")
        logits_list, _, _ = self._forward_batch(gb, pairs)
        shapes = [(int(lg.shape[2]), int(lg.shape[3])) for lg in logits_list]
        labels = labels_from_examples_batch([ex.to(self._ranker().device) for ex in examples_list], shapes)
        return self._test_batch_dicts(logits_list, shapes, labels, filepaths, keep_maps)

    def _test_batch_dicts(self, logits_list, shapes, labels, filepaths, keep_maps):
        """test_batch's tail: the batched ranking and AUC calls over the logits and their uint8 label
        maps, and one test_step dict per complex."""
        import os
        rank, auc_op = self._ranker(), self._auc()
        ranks = rank.batch([lg.contiguous() for lg in logits_list], labels_list=labels,
                           threshold=self.pos_prob_threshold)
        aucs = auc_op.batch([r.probs for r in ranks], labels)   # the maps the ranking judged
        hits = ranks.hits.cpu()
        keep = len(ranks) if keep_maps is None else int(keep_maps)
        outs = []
        for i, (r, a, (l1, l2)) in enumerate(zip(ranks, aucs, shapes)):
            k = min(l1, l2)
            confusion = {f: getattr(r, f) for f in ("tp", "fp", "fn", "tn")}
            out = {"loss": r.ce_sum / (l1 * l2)}
            out.update(topk_metrics(hits[ranks.hits_off[i]:ranks.hits_off[i] + k], r.num_pos, k))
            if i < keep:
                out["test_preds"] = r.probs.cpu().numpy()
                out["test_preds_rounded"] = (r.probs >= self.pos_prob_threshold).float().cpu().numpy()
                out["test_labels"] = labels[i].view(l1, l2).float().cpu().numpy()
            else:
                out["test_preds"] = out["test_preds_rounded"] = out["test_labels"] = None
            out["target"] = str(filepaths[i]).split(os.sep)[-1][:4]
            out["confusion"] = confusion
            out["test_auroc"], out["test_auprc"] = a.auroc, a.auprc
            out.update(confusion_metrics(**confusion))
            outs.append(out)
        return outs

    def _interface(self):
        dev = self.engine.device
        if self._interface_op is None or self._interface_op.device != dev:
            self._interface_op = InterfaceOp(dev)
        return self._interface_op

    def test_batch_structures(self, gb: GraphBatch, pairs, structures, filepaths, keep_maps=None, cutoff=6.0):
        """``test_batch`` from structures instead of example lists: structures[i] = ((xyz0, res_off0),
        (xyz1, res_off1)), complex i's heavy atoms per chain as ``ranking.interface_atoms`` groups them
        (numpy arrays or tensors on the model's GPU). The label maps come from ``ranking.InterfaceOp``
        (residues interact iff two of their heavy atoms lie within ``cutoff``, 6 A in DIPS); everything
        after them is test_batch's, and so are the dicts. A chain whose residue count differs from its
        graph's node count raises ValueError before any launch."""
        if not (len(pairs) == len(structures) == len(filepaths)):
            raise ValueError("test_batch_structures: one structure and one file path per complex")
        for i, ((a, b), (c0, c1)) in enumerate(zip(pairs, structures)):
            want = (gb.nodes_per_graph[a], gb.nodes_per_graph[b])
            got = (int(c0[1].shape[0]) - 1, int(c1[1].shape[0]) - 1)
            if got != want:
                raise ValueError(f"test_batch_structures: complex {i}'s chains have {got} residues, "
                                 f"its graphs {want} nodes")
        logits_list, _, _ = self._forward_batch(gb, pairs)
        shapes = [(int(lg.shape[2]), int(lg.shape[3])) for lg in logits_list]
        labels = self._interface().labels([s[0] for s in structures], [s[1] for s in structures], cutoff=cutoff)
        return self._test_batch_dicts(logits_list, shapes, labels, filepaths, keep_maps)

    def test_sharded(self, complexes, examples_list, filepaths, micro_batch=8, k=20, seed=0, group=None,
                     device=None, structures=None, cutoff=6.0):
        """test_step over a test set sharded across a process group (``distributed.test_sharded``):
        every rank ranks and scores its shard on the device, ONE all-gather moves a KB-sized record
        per complex, and every rank returns every complex's test_batch dict (maps None; ``top_ids`` /
        ``top_scores`` added), ready for ``test_epoch_end(outs)`` without a group. The labels come from
        ``examples_list`` or, with ``examples_list=None``, from ``structures`` (as
        ``test_batch_structures`` takes them; ``cutoff`` in A): exactly one of the two."""
        from .distributed import test_sharded
        return test_sharded(self, complexes, examples_list, filepaths, micro_batch=micro_batch, k=k, seed=seed,
                            group=group, device=device, structures=structures, cutoff=cutoff)

    def _examples(self):
        dev = self.engine.device
        if self._examples_op is None or self._examples_op.device != dev:
            self._examples_op = ExamplesOp(dev)
        return self._examples_op

    @staticmethod
    def _validation_k(l: int, n: int) -> int:
        """Ranks kept of a pool of n rows: the largest k of the six figures that the pool and the
        ranking's limit allow (l, or 10 for chains of fewer than 10 residues in all)."""
        return min(max(l, 10), n, DI_RANK_MAX_K)

    @staticmethod
    def _validation_output(r, a, hits, l: int, n: int) -> dict:
        """validation_step's dict from a pool's ranking (its counters), AUC record and host hits."""
        confusion = {f: getattr(r, f) for f in ("tp", "fp", "fn", "tn")}
        out = {"loss": r.ce_sum / n}
        out.update({"val_" + name[5:]: v for name, v in confusion_metrics(**confusion).items()})
        out["val_auroc"], out["val_auprc"] = a.auroc, a.auprc
        out["confusion"] = confusion
        out.update({"val_" + name: v for name, v in pooled_topk_metrics(hits, r.num_pos, l, n).items()})
        return out

    def validation_step(self, batch, batch_idx=0):
        """LitGINI.validation_step (deepinteract_modules.py:1915-1982). batch = (graph1, graph2,
        examples_list, filepaths); examples_list[i] is complex i's sampled [n_i, 3] (i, j, label)
        rows: any count >= 1, any order, repeats allowed. As in the reference only the listed pairs
        are judged, and the complexes of a batch are pooled: their rows, one complex after another,
        form one list of N rows (ranking.ExamplesOp.gather), ranked and scored as one.

        Returns loss (the mean cross-entropy over the N rows), val_acc / val_prec / val_recall /
        val_f1 (ranking.confusion_metrics on the pool's counts at pos_prob_threshold), val_auroc /
        val_auprc (ranking.ContactAucOp on the pool's probabilities; float('nan') when a class is
        empty), confusion = {tp, fp, fn, tn}, and the six figures the reference logs:
        val_top_10_prec, val_top_l_by_10_prec, val_top_l_by_5_prec, val_top_l_recall,
        val_top_l_by_2_recall, val_top_l_by_5_recall with l = graph1.num_nodes() +
        graph2.num_nodes() (ranking.pooled_topk_metrics: a k past the pool takes all N rows and
        precision still divides by k; float('nan') where the reference would divide by zero, and
        where k and N both exceed DI_RANK_MAX_K).

        Equal probabilities rank by their position in the pooled list (the ranking op's stable
        order); the reference's ``argsort`` leaves their order undefined."""
        graph1, graph2, examples_list = batch[0], batch[1], batch[2]
        logits_list = self.shared_step(graph1, graph2)
        if len(examples_list) != len(logits_list):
            raise ValueError("validation_step: one examples tensor per complex")
        ex_op, rank = self._examples(), self._ranker()
        (pool_logits, pool_labels), = ex_op.gather([lg.contiguous() for lg in logits_list],
                                                   [ex.to(rank.device) for ex in examples_list],
                                                   pools=[list(range(len(logits_list)))])
        n = int(pool_labels.numel())
        l = int(graph1.num_nodes()) + int(graph2.num_nodes())
        r = rank(pool_logits, k=self._validation_k(l, n), labels=pool_labels, threshold=self.pos_prob_threshold)
        a = self._auc()(r.probs, pool_labels)   # the map the ranking judged
        return self._validation_output(r, a, r.hits.cpu(), l, n)

    def validation_batch(self, gb: GraphBatch, pairs, examples_list):
        """validation_step for many complexes at once, each complex its own pool and its own
        l = L1 + L2: one forward (``_forward_batch``), one gather (ranking.ExamplesOp.gather), one
        batched ranking call and one batched AUC call, whatever the number of complexes. pairs as in
        ``predict_batch``; examples_list[i] belongs to complex i. Returns one validation_step dict per
        complex, with the bits validation_step gives on that complex alone. The host reads the
        device once for the lists' validation, once per metrics table and once for all top_hits."""
        if len(pairs) != len(examples_list):
            raise ValueError("validation_batch: one examples tensor per complex")
        logits_list, _, _ = self._forward_batch(gb, pairs)
        ex_op, rank, auc_op = self._examples(), self._ranker(), self._auc()
        pooled = ex_op.gather([lg.contiguous() for lg in logits_list], [ex.to(rank.device) for ex in examples_list])
        ls = [int(lg.shape[2]) + int(lg.shape[3]) for lg in logits_list]
        ns = [int(lab.numel()) for _, lab in pooled]
        ranks = rank.batch([lg for lg, _ in pooled], k=[self._validation_k(l, n) for l, n in zip(ls, ns)],
                           labels_list=[lab for _, lab in pooled], threshold=self.pos_prob_threshold)
        aucs = auc_op.batch([r.probs for r in ranks], [lab for _, lab in pooled])
        hits = ranks.hits.cpu()
        return [self._validation_output(r, a, hits[ranks.hits_off[i]:ranks.hits_off[i] + r.ids.numel()], l, n)
                for i, (r, a, l, n) in enumerate(zip(ranks, aucs, ls, ns))]

    _VAL_MEDIANS = ("val_acc", "val_prec", "val_recall", "val_f1", "val_auroc", "val_auprc")

    def validation_epoch_end(self, outputs, group=None):
        """LitGINI.validation_epoch_end (deepinteract_modules.py:1984-2016) without the loggers:
        med_val_acc / prec / recall / f1 / auroc / auprc over the dicts of validation_step /
        validation_batch, as ``test_epoch_end`` gives med_test_* (``torch.median``; with a process
        ``group`` over every rank's values)."""
        return self._epoch_medians(outputs, self._VAL_MEDIANS, group, "validation_epoch_end")

    @staticmethod
    def _epoch_medians(outputs, names, group, what) -> dict:
        """med_<name> of this rank's outputs, or of every rank's (all-gathered; ranks may hold
        different counts) with a process group."""
        vals = [[float(o[name]) for name in names] for o in outputs]
        if group is not None:
            import torch.distributed as dist
            gathered = [None] * dist.get_world_size(group)
            dist.all_gather_object(gathered, vals, group=group)
            vals = [row for part in gathered for row in part]
        if not vals:
            raise ValueError(f"{what}: no outputs")
        table = torch.tensor(vals, dtype=torch.float64)
        return {"med_" + name: float(torch.median(table[:, c])) for c, name in enumerate(names)}

    _MEDIANS = ("test_acc", "test_prec", "test_recall", "test_f1", "test_auroc", "test_auprc")
    _CSV_COLUMNS = ("top_10_prec", "top_l_by_10_prec", "top_l_by_5_prec", "top_l_recall", "top_l_by_2_recall",
                    "top_l_by_5_recall", "target")

    def test_epoch_end(self, outputs, csv_path=None, group=None):
        """LitGINI.test_epoch_end (deepinteract_modules.py:2103-2165) without the loggers. outputs: the
        dicts of test_step / test_batch of this rank.

        Returns med_test_acc / prec / recall / f1 / auroc / auprc: ``torch.median`` over all complexes
        (the lower middle value of an even count; NaN if any value is NaN). With a process ``group``
        every rank's per-complex values are all-gathered first (ranks may hold different counts), so
        every rank returns the medians of all of them. With ``csv_path`` the six top-k columns plus
        ``target`` are written, one row per complex of THIS rank's outputs, in the layout
        ``DataFrame.to_csv`` writes (a leading unnamed index column; NaN as an empty field)."""
        out = self._epoch_medians(outputs, self._MEDIANS, group, "test_epoch_end")
        if csv_path is not None:
            import csv
            with open(csv_path, "w", newline="") as fh:
                wr = csv.writer(fh, lineterminator="\n")
                wr.writerow(("",) + self._CSV_COLUMNS)
                for i, o in enumerate(outputs):
                    row = [o[c] for c in self._CSV_COLUMNS]
                    wr.writerow([i] + ["" if isinstance(v, float) and v != v else v for v in row])
        return out


def construct_interact_tensor(graph1_feats, graph2_feats, pad=False, max_len=256):
    """deepinteract_utils.py:158-172 on the HIP pair-tensor kernel (pad=False path)."""
    if pad:
        raise NotImplementedError("pad=True (subsequencing) is disabled in the reference (:1699)")
    h = torch.cat([graph1_feats, graph2_feats]).contiguous()
    l1, l2 = graph1_feats.shape[0], graph2_feats.shape[0]
    _, views = PairTensorOp(h.device)(h, [0], [l1], [l1], [l2])
    return views[0]


__all__ = ["DGLGeometricTransformer", "LitGINI", "construct_interact_tensor", "batch_graphs", "unbatch"]
