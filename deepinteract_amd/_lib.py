"""ctypes binding of the C ABI in include/deepinteract_amd.h.

The product path has no fallback: if the HIP library cannot be loaded every op raises.
"""
from __future__ import annotations

import ctypes
import os

from . import build as _build

DI_F32, DI_BF16 = 0, 1


class DiGraph(ctypes.Structure):
    _fields_ = [("num_nodes", ctypes.c_int32), ("num_edges", ctypes.c_int32),
                ("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("nbr", ctypes.c_void_p),
                ("node_pos", ctypes.c_void_p), ("in_ptr", ctypes.c_void_p), ("flags", ctypes.c_int32)]


DI_GRAPH_GEO_REF = 1


class DiGeoArgs(ctypes.Structure):
    _fields_ = [("num_graphs", ctypes.c_int32), ("k", ctypes.c_int32), ("max_nodes", ctypes.c_int32),
                ("node_off", ctypes.c_void_p), ("backbone", ctypes.c_void_p), ("amide_norm", ctypes.c_void_p),
                ("dips", ctypes.c_void_p), ("knn_idx", ctypes.c_void_p), ("knn_d2", ctypes.c_void_p),
                ("node_f", ctypes.c_void_p), ("edge_f", ctypes.c_void_p), ("stats", ctypes.c_void_p)]


class DiPairDesc(ctypes.Structure):
    _fields_ = [("h1_row", ctypes.c_int64), ("h2_row", ctypes.c_int64), ("out_off", ctypes.c_int64),
                ("l1", ctypes.c_int32), ("l2", ctypes.c_int32)]


class DiPairLaunch(ctypes.Structure):
    _fields_ = [("kernel", ctypes.c_int32), ("blocks", ctypes.c_int32), ("waves_per_block", ctypes.c_int32),
                ("beside", ctypes.c_int32)]


DI_PAIR_AUTO, DI_PAIR_ROWS, DI_PAIR_VECTOR, DI_PAIR_LINES = 0, 1, 2, 3
ABI_VERSION = 8


class DiPairJob(ctypes.Structure):
    _fields_ = [("hT", ctypes.c_void_p), ("descs", ctypes.c_void_p), ("out", ctypes.c_void_p),
                ("num_rows", ctypes.c_int32), ("num_complexes", ctypes.c_int32), ("max_l1", ctypes.c_int32),
                ("items", ctypes.c_int32)]


class DiRankMetrics(ctypes.Structure):
    _fields_ = [("num_pos", ctypes.c_int64), ("tp", ctypes.c_int64), ("fp", ctypes.c_int64),
                ("fn", ctypes.c_int64), ("tn", ctypes.c_int64), ("ce_sum", ctypes.c_double)]


DI_RANK_MAX_K = 4096


class DiAucMetrics(ctypes.Structure):
    _fields_ = [("num_pos", ctypes.c_int64), ("num_neg", ctypes.c_int64), ("num_nan", ctypes.c_int64),
                ("pos_distinct", ctypes.c_int64), ("u2", ctypes.c_uint64), ("auroc", ctypes.c_double),
                ("auprc", ctypes.c_double), ("overflow", ctypes.c_int32), ("pad", ctypes.c_int32)]


DI_BATCH_MAX = 1024


class DiRankItem(ctypes.Structure):
    _fields_ = [("logits", ctypes.c_void_p), ("labels", ctypes.c_void_p), ("probs", ctypes.c_void_p),
                ("top_ids", ctypes.c_void_p), ("top_scores", ctypes.c_void_p), ("top_hits", ctypes.c_void_p),
                ("metrics", ctypes.c_void_p), ("hdr_off", ctypes.c_int64), ("work_off", ctypes.c_int64),
                ("l1", ctypes.c_int32), ("l2", ctypes.c_int32), ("k", ctypes.c_int32), ("pad", ctypes.c_int32)]


class DiAucItem(ctypes.Structure):
    _fields_ = [("probs", ctypes.c_void_p), ("labels", ctypes.c_void_p), ("out", ctypes.c_void_p),
                ("n", ctypes.c_int64), ("max_pos", ctypes.c_int64), ("hdr_off", ctypes.c_int64),
                ("work_off", ctypes.c_int64)]


DI_I64, DI_I32 = 0, 1
DI_EX_OUTSIDE, DI_EX_LABEL, DI_EX_TWICE = 1, 2, 4
DI_EX_BLOCK_ROWS = 1024


class DiExamplesItem(ctypes.Structure):
    _fields_ = [("examples", ctypes.c_void_p), ("logits", ctypes.c_void_p), ("labels", ctypes.c_void_p),
                ("pool_logits", ctypes.c_void_p), ("pool_labels", ctypes.c_void_p), ("n", ctypes.c_int64),
                ("out_off", ctypes.c_int64), ("total", ctypes.c_int64), ("work_off", ctypes.c_int64),
                ("l1", ctypes.c_int32), ("l2", ctypes.c_int32)]


DI_IF_OFFSETS, DI_IF_EMPTY, DI_IF_NONFINITE = 1, 2, 4


class DiInterfaceItem(ctypes.Structure):
    _fields_ = [("xyz0", ctypes.c_void_p), ("res_off0", ctypes.c_void_p), ("xyz1", ctypes.c_void_p),
                ("res_off1", ctypes.c_void_p), ("labels", ctypes.c_void_p), ("l1", ctypes.c_int32),
                ("l2", ctypes.c_int32), ("a0", ctypes.c_int32), ("a1", ctypes.c_int32), ("work_off", ctypes.c_int64)]


class DiInterfaceStats(ctypes.Structure):
    _fields_ = [("num_pos", ctypes.c_int64), ("flags", ctypes.c_int32), ("pad", ctypes.c_int32)]


DI_ENV_OFFSETS, DI_ENV_EMPTY, DI_ENV_NONFINITE, DI_ENV_BACKBONE = 1, 2, 4, 8
DI_ROLE_OTHER, DI_ROLE_N, DI_ROLE_CA, DI_ROLE_C, DI_ROLE_O, DI_ROLE_CB = range(6)
DI_ENV_C2 = 55.262043       # (float)(8 ln 1000): exp(-d2 / 8) > 1e-3


class DiEnvItem(ctypes.Structure):
    _fields_ = [("xyz", ctypes.c_void_p), ("res_off", ctypes.c_void_p), ("role", ctypes.c_void_p),
                ("aa", ctypes.c_void_p), ("resname", ctypes.c_void_p), ("dips", ctypes.c_void_p),
                ("amide_norm", ctypes.c_void_p), ("backbone", ctypes.c_void_p), ("cn_raw", ctypes.c_void_p),
                ("l", ctypes.c_int32), ("a", ctypes.c_int32), ("work_off", ctypes.c_int64)]


class DiEnvStats(ctypes.Structure):
    _fields_ = [("flags", ctypes.c_int32), ("cn_max", ctypes.c_int32), ("cn_min_gap", ctypes.c_int32),
                ("pad", ctypes.c_int32)]


class DiHeadConvArgs(ctypes.Structure):
    _fields_ = [("x", ctypes.c_void_p), ("weight", ctypes.c_void_p), ("in_scale", ctypes.c_void_p),
                ("in_shift", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("y", ctypes.c_void_p),
                ("stats", ctypes.c_void_p), ("cin", ctypes.c_int32), ("cout", ctypes.c_int32),
                ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("ksize", ctypes.c_int32),
                ("dilation", ctypes.c_int32), ("in_elu", ctypes.c_int32)]


class DiHeadItem(ctypes.Structure):
    _fields_ = [("px_off", ctypes.c_int64), ("stats_off", ctypes.c_int64), ("h", ctypes.c_int32),
                ("w", ctypes.c_int32)]


class DiHeadBlock(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in
                ("w1", "w2", "w3", "gamma1", "beta1", "gamma2", "beta2", "gamma3", "beta3", "bias1", "bias2",
                 "bias3", "se_w1", "se_b1", "se_w2", "se_b2")] + [("eps", ctypes.c_float), ("dilation", ctypes.c_int32)]


class DiHeadNet(ctypes.Structure):
    _fields_ = [("proj_w", ctypes.c_void_p), ("proj_b", ctypes.c_void_p), ("blocks", ctypes.POINTER(DiHeadBlock)),
                ("num_blocks", ctypes.c_int32), ("in_elu", ctypes.c_int32)]


class DiHeadArena(ctypes.Structure):
    _fields_ = [("wide0", ctypes.c_void_p), ("wide1", ctypes.c_void_p), ("half0", ctypes.c_void_p),
                ("half1", ctypes.c_void_p), ("stats", ctypes.c_void_p), ("rows", ctypes.c_void_p),
                ("items", ctypes.c_void_p), ("items_dev", ctypes.c_void_p), ("count", ctypes.c_int32)]


class DiRegionAttnArgs(ctypes.Structure):
    _fields_ = [("x", ctypes.c_void_p), ("wq", ctypes.c_void_p), ("wk", ctypes.c_void_p),
                ("scores", ctypes.c_void_p), ("v", ctypes.c_void_p), ("y", ctypes.c_void_p),
                ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("in_elu", ctypes.c_int32)]


# pair-queue words(include/deepinteract_amd.h, di_pair_queue_bytes)
PQ_READY, PQ_ERROR, PQ_GAVE_UP, PQ_SBYTES, PQ_HBYTES = 0, 32, 33, 40, 42


_P = ctypes.c_void_p
_I = ctypes.c_int32
_SIGS = {
    "di_abi_version": ([], ctypes.c_int),
    "di_blob_bytes": ([ctypes.c_int, ctypes.c_int, ctypes.c_int], ctypes.c_int64),
    "di_blob_layout": ([ctypes.c_int, ctypes.c_int], ctypes.c_int),
    "di_node_embed": ([ctypes.POINTER(DiGraph), _I, _I, _P, _P, _P, _P, _P, _P, _I, _P], ctypes.c_int),
    "di_init_edge": ([ctypes.POINTER(DiGraph), _I, _P, _P, _P, _P, _P, _P, _P, _P], ctypes.c_int),
    "di_init_edge_resident": ([ctypes.POINTER(DiGraph), _P, _P, _P, _P, _P, _P, _P], ctypes.c_int),
    "di_embed_init_edge": ([ctypes.POINTER(DiGraph), _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P],
                           ctypes.c_int),
    "di_edge_layer": ([ctypes.POINTER(DiGraph), _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
                      ctypes.c_int),
    "di_embed_init_edge_z": ([ctypes.POINTER(DiGraph), _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P],
                             ctypes.c_int),
    "di_edge_layer_z": ([ctypes.POINTER(DiGraph), _I, _P, _P, _P, _P, _P, _P, _P, _P, _P], ctypes.c_int),
    "di_plain_blob_bytes": ([ctypes.c_int, ctypes.c_int, ctypes.c_int], ctypes.c_int64),
    "di_init_edge_plain": ([ctypes.POINTER(DiGraph), _I, _P, _P, _P, _P], ctypes.c_int),
    "di_edge_layer_plain": ([ctypes.POINTER(DiGraph), _I, _I, _P, _P, _P, _P, _P, _P, _P, _P], ctypes.c_int),
    "di_node_layer": ([ctypes.POINTER(DiGraph), _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P], ctypes.c_int),
    "di_node_aggregate": ([ctypes.POINTER(DiGraph), _I, _P, _P, _P, _P], ctypes.c_int),
    "di_node_update": ([ctypes.POINTER(DiGraph), _I, _I, _P, _P, _P, _P, _P, _P, _P, _P], ctypes.c_int),
    "di_attn_parts_bytes": ([_I], ctypes.c_int64),
    "di_edge_layer_attn": ([ctypes.POINTER(DiGraph), _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
                           ctypes.c_int),
    "di_node_update_folded": ([ctypes.POINTER(DiGraph), _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P], ctypes.c_int),
    "di_pair_tensor": ([_I, _P, _I, _I, _I, _I, _I, _P, _P, _I, ctypes.POINTER(DiPairLaunch), _P, _P], ctypes.c_int),
    "di_pair_tensor_check": ([_I, _I, _I, _I, _I, ctypes.POINTER(DiPairLaunch)], ctypes.c_int),
    "di_pair_queue_bytes": ([_I], ctypes.c_int64),
    "di_pair_job_items": ([_I, _I, _I], ctypes.c_int32),
    "di_pair_signal": ([_P, _I, _P], ctypes.c_int),
    "di_pair_stream": ([_I, _P, _I, _I, _I, _P, ctypes.POINTER(DiPairLaunch), ctypes.c_float, _P], ctypes.c_int),
    "di_pair_help": ([_I, _P, _I, _I, _I, _P, ctypes.POINTER(DiPairLaunch), _I, _P], ctypes.c_int),
    "di_stream_create_dedicated": ([ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "di_stream_destroy": ([_P], ctypes.c_int),
    "di_streams_concurrent": ([_P, _P, _P, ctypes.c_float, ctypes.POINTER(ctypes.c_int32)], ctypes.c_int),
    "di_head_prologue": ([_I, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, ctypes.c_float, _P, _P, _P],
                         ctypes.c_int),
    "di_head_prologue_work_bytes": ([_I, _I, _I, _I], ctypes.c_int64),
    "di_inorm_elu": ([_I, _P, _I, ctypes.c_int64, _P, _P, ctypes.c_float, _P, _P, _P], ctypes.c_int),
    "di_inorm_work_bytes": ([_I, ctypes.c_int64], ctypes.c_int64),
    "di_se_scale_add": ([_I, _P, _P, _P, _P, _I, ctypes.c_int64, _P, _P], ctypes.c_int),
    "di_channel_mean": ([_I, _P, _I, ctypes.c_int64, _P, _P, _P, _P], ctypes.c_int),
    "di_head_conv": ([_I, ctypes.POINTER(DiHeadConvArgs), _P], ctypes.c_int),
    "di_head_conv_check": ([_I, ctypes.POINTER(DiHeadConvArgs)], ctypes.c_int),
    "di_head_conv_f32": ([ctypes.POINTER(DiHeadConvArgs), _P], ctypes.c_int),
    "di_head_conv_f32_check": ([ctypes.POINTER(DiHeadConvArgs)], ctypes.c_int),
    "di_head_conv_stats_bytes": ([_I, _I, _I], ctypes.c_int64),
    "di_plane_stats": ([_I, _P, _I, ctypes.c_int64, _P, _P], ctypes.c_int),
    "di_head_norm_fold": ([_P, _I, ctypes.c_int64, _P, _P, ctypes.c_float, _P, _P, _P, _P, _P], ctypes.c_int),
    "di_head_batch_layout": ([_P, _I, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)], ctypes.c_int),
    "di_head_conv_batch": ([_I, ctypes.POINTER(DiHeadConvArgs), _P, _P, _I, _P], ctypes.c_int),
    "di_plane_stats_batch": ([_I, _P, _I, _P, _P, _I, _P, _P], ctypes.c_int),
    "di_head_norm_fold_batch": ([_P, _I, _P, _P, _I, _P, _P, ctypes.c_float, _P, _P, _P, _P, _P], ctypes.c_int),
    "di_se_scale_add_batch": ([_I, _P, _P, _P, _P, _I, _P, _P, _I, _P, _P], ctypes.c_int),
    "di_se_gate": ([_P, _P, _P, _P, _P, _I, _I, _I, _P, _P], ctypes.c_int),
    "di_head_conv_f32_batch": ([ctypes.POINTER(DiHeadConvArgs), _P, _P, _I, _P], ctypes.c_int),
    "di_head_conv_f32_batch_check": ([ctypes.POINTER(DiHeadConvArgs), _P, _P, _I], ctypes.c_int),
    "di_plane_stats_f32_batch": ([_P, _I, _P, _P, _I, _P, _P], ctypes.c_int),
    "di_se_scale_add_f32_batch": ([_P, _P, _P, _P, _I, _P, _P, _I, _P, _P], ctypes.c_int),
    "di_head_body_batch": ([_I, ctypes.POINTER(DiHeadNet), _I, ctypes.POINTER(DiHeadArena),
                            ctypes.POINTER(ctypes.c_int32), _P], ctypes.c_int),
    "di_head_body_batch_check": ([_I, ctypes.POINTER(DiHeadNet), _I, ctypes.POINTER(DiHeadArena)], ctypes.c_int),
    "di_head_logits_batch": ([_I, _P, _P, _P, _P, _P, _I, _P, _P], ctypes.c_int),
    "di_region_scores": ([_I, ctypes.POINTER(DiRegionAttnArgs), _P], ctypes.c_int),
    "di_region_mix": ([_I, ctypes.POINTER(DiRegionAttnArgs), _P], ctypes.c_int),
    "di_region_attn_check": ([_I, ctypes.POINTER(DiRegionAttnArgs)], ctypes.c_int),
    "di_region_scores_batch": ([_I, ctypes.POINTER(DiRegionAttnArgs), _P, _P, _I, _P], ctypes.c_int),
    "di_region_mix_batch": ([_I, ctypes.POINTER(DiRegionAttnArgs), _P, _P, _I, _P], ctypes.c_int),
    "di_contact_rank_work_bytes": ([ctypes.c_int64, _I], ctypes.c_int64),
    "di_contact_rank": ([_I, _P, _I, _I, _I, _P, ctypes.c_float, _P, _P, _P, _P, _P, _P, _P], ctypes.c_int),
    "di_contact_auc_work_bytes": ([ctypes.c_int64, ctypes.c_int64], ctypes.c_int64),
    "di_contact_auc": ([_P, _P, ctypes.c_int64, ctypes.c_int64, _P, _P, _P], ctypes.c_int),
    "di_contact_rank_batch_work_bytes": ([_P, _I], ctypes.c_int64),
    "di_contact_rank_batch": ([_I, _P, _P, _I, ctypes.c_float, _P, _P], ctypes.c_int),
    "di_contact_auc_batch_work_bytes": ([_P, _I], ctypes.c_int64),
    "di_contact_auc_batch": ([_P, _P, _I, _P, _P], ctypes.c_int),
    "di_rank_record_bytes": ([_I, _I, _I, _I, ctypes.POINTER(ctypes.c_int64)], ctypes.c_int64),
    "di_examples_labels_work_bytes": ([_P, _I], ctypes.c_int64),
    "di_examples_labels_batch": ([_I, _P, _P, _I, _P, _P], ctypes.c_int),
    "di_examples_labels_batch_check": ([_I, _P, _P, _I, _P], ctypes.c_int),
    "di_examples_gather_batch": ([_I, _I, _P, _P, _I, _P, _P], ctypes.c_int),
    "di_examples_gather_batch_check": ([_I, _I, _P, _P, _I, _P], ctypes.c_int),
    "di_interface_work_bytes": ([_P, _I], ctypes.c_int64),
    "di_interface_labels_batch": ([_P, _P, _I, ctypes.c_float, _P, _P], ctypes.c_int),
    "di_interface_labels_batch_check": ([_P, _P, _I, ctypes.c_float, _P], ctypes.c_int),
    "di_residue_env_work_bytes": ([_P, _I], ctypes.c_int64),
    "di_residue_env_batch": ([_P, _P, _I, ctypes.c_float, _P, _P], ctypes.c_int),
    "di_residue_env_batch_check": ([_P, _P, _I, ctypes.c_float, _P], ctypes.c_int),
    "di_knn_topk": ([_I, _P, _P, _I, _I, _P, _P, _P], ctypes.c_int),
    "di_geo_feats": ([ctypes.POINTER(DiGeoArgs), _P], ctypes.c_int),
    "di_build_nbr_ids": ([_I, _P, _P, _P, ctypes.c_uint64, _P, _P], ctypes.c_int),
    "di_build_nbr_ids_torch": ([_I, _P, _I, _P, _I, _P, _P, _P, _P], ctypes.c_int),
    "di_knn_graph": ([_I, _P, _I, _P, _I, _P, _P, _P, _P, _P], ctypes.c_int),
    "di_conformation": ([ctypes.POINTER(DiGraph), _I, _P, _P, _P, _P, _P, _P, _P], ctypes.c_int),
    "di_gemm_bias_act": ([_I, _I, _I, _I, _P, _I, _P, _P, _I, _P, _I, _P, _I, _P], ctypes.c_int),
    "di_geo_attention": ([ctypes.POINTER(DiGraph), _I, _P, _P, _P, _P, _P, _P], ctypes.c_int),
}

_lib = None


def library_path() -> str:
    return _build.LIB


def _bind(path: str):
    lib = ctypes.CDLL(path)
    for name, (argtypes, restype) in _SIGS.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = restype
    if lib.di_abi_version() != ABI_VERSION:
        raise RuntimeError("deepinteract_amd ABI version mismatch")
    return lib


def load(build_if_missing: bool = True):
    """Load (building first if needed) the in-tree HIP library; raises if it is unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own libamdhip64.so.7: load it first so this library binds to the SAME HIP
    # runtime (same SONAME) instead of pulling /opt/rocm's copy into the process.
    import torch  # noqa: F401
    if not os.path.exists(_build.LIB) or (build_if_missing and not _build.up_to_date()):
        if not build_if_missing:
            raise RuntimeError(f"deepinteract_amd HIP library missing: {_build.LIB}")
        _build.build()
    _lib = _bind(_build.LIB)
    return _lib


def load_variant(path: str):
    """Tuning only (bench.py --lib): bind a launch-shape variant of the library built by
    build.build_variant() instead of the in-tree one. Must run before any other load()."""
    global _lib
    if _lib is not None:
        raise RuntimeError("the HIP library is already loaded")
    import torch  # noqa: F401
    if not os.path.exists(path):
        raise RuntimeError(f"variant library {path} does not exist")
    _lib = _bind(path)
    return _lib


RECORD_FIELDS = ("ids", "scores", "hits", "metrics", "auc")


def rank_record_layout(l1: int, l2: int, k: int, with_labels: bool):
    """``di_rank_record_bytes``: (the record's bytes, {field: byte offset} of RECORD_FIELDS; a field the
    record does not have is absent). The layout is the C function's alone. ValueError where it refuses."""
    offs = (ctypes.c_int64 * 5)()
    nb = load().di_rank_record_bytes(int(l1), int(l2), int(k), int(bool(with_labels)), offs)
    if nb < 0:
        raise ValueError(f"ranking record of a {l1} x {l2} complex, k = {k}: code {nb} "
                         f"(1 <= k <= min(L1 * L2, {DI_RANK_MAX_K}), L1 * L2 < 2^29)")
    return int(nb), {f: int(o) for f, o in zip(RECORD_FIELDS, offs) if o >= 0}


def check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what} failed with code {rc}")
