"""The batched fp32 contact head without a GPU: the refusals of di_head_conv_f32_batch,
di_plane_stats_f32_batch and di_se_scale_add_f32_batch before a launch (dummy pointers are never
dereferenced), di_head_conv_f32_batch_check's verdicts, and LitGINI's ``head_batch_f32`` option. The table
helpers are those of test_head_batch_host.py."""
import ctypes

import pytest
import torch

from deepinteract_amd import _lib
from test_capi import _declared_arg_counts
from test_head_batch_host import BATCH, MID, _setter, head_items, layout

EINVAL, ERANGE = -1, -2
P, Q = 16 * 1024, 32 * 1024      # dummy non-NULL, 16-B aligned pointers


def conv_args(**kw):
    a = _lib.DiHeadConvArgs(P, P, None, None, None, Q, None, 64, 64, 0, 0, 3, 2, 1)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def good_items(shapes=BATCH):
    items = head_items(shapes)
    assert layout(items)[0] == 0
    return items


def test_signatures_and_abi():
    decl = _declared_arg_counts()
    for name, n in (("di_head_conv_f32_batch", 5), ("di_head_conv_f32_batch_check", 4),
                    ("di_plane_stats_f32_batch", 7), ("di_se_scale_add_f32_batch", 10)):
        assert decl[name] == n == len(_lib._SIGS[name][0]), name
    assert _lib.load().di_abi_version() == _lib.ABI_VERSION == 8     # additions: the version stays


def _calls():
    """name -> callable(items, items_dev, count) for each fp32 batch entry point with good shared arguments."""
    lib = _lib.load()
    p, q = ctypes.c_void_p(P), ctypes.c_void_p(Q)
    return {
        "conv": lambda it, dev, n: lib.di_head_conv_f32_batch(ctypes.byref(conv_args()), it, dev, n, None),
        "conv_check": lambda it, dev, n: lib.di_head_conv_f32_batch_check(ctypes.byref(conv_args()), it, dev, n),
        "stats": lambda it, dev, n: lib.di_plane_stats_f32_batch(p, 128, it, dev, n, q, None),
        "se": lambda it, dev, n: lib.di_se_scale_add_f32_batch(p, p, p, p, 128, it, dev, n, q, None),
    }


@pytest.mark.parametrize("name", ["conv", "conv_check", "stats", "se"])
def test_item_table_refusals_without_gpu(name):
    """A bad, unfilled or NULL table, count 0 and count > DI_BATCH_MAX: refused before any launch (there is
    no GPU here)."""
    fn = _calls()[name]
    p = ctypes.c_void_p(P)

    def call(edit=None, count=None, host=True, dev=p, at=MID):
        items = good_items()
        if edit:
            edit(items[at])
        return fn(items if host else None, dev, len(items) if count is None else count)

    assert call(count=0) == EINVAL and call(count=-2) == EINVAL
    assert call(host=False) == EINVAL and call(dev=None) == EINVAL
    many = head_items([(8, 8)] * (_lib.DI_BATCH_MAX + 1))
    assert layout(many, _lib.DI_BATCH_MAX)[0] == 0
    assert fn(many, p, _lib.DI_BATCH_MAX + 1) == ERANGE
    for kw in (dict(h=0), dict(w=0), dict(h=-4), dict(w=-1)):
        assert call(_setter(**kw)) == EINVAL, kw
    assert call(_setter(px_off=0)) == EINVAL and call(_setter(stats_off=16)) == EINVAL
    assert call(_setter(px_off=1), at=0) == EINVAL and call(_setter(stats_off=8), at=0) == EINVAL
    assert call(_setter(h=144)) == EINVAL and call(_setter(w=146)) == EINVAL   # sizes changed after the layout
    fresh = head_items(BATCH)                                                 # never laid out
    assert fn(fresh, p, len(fresh)) == EINVAL


def test_conv_f32_batch_check_accepts_what_the_single_call_accepts():
    lib = _lib.load()
    p = ctypes.c_void_p(P)
    items = good_items()
    for kw in (dict(), dict(ksize=1, dilation=1, cin=128, cout=64), dict(ksize=1, dilation=1, cin=64, cout=128),
               dict(ksize=1, dilation=1, cin=256, cout=128), dict(dilation=8), dict(cout=128, dilation=4),
               dict(in_scale=P, in_shift=P, bias=P, stats=Q + 8), dict(x=P + 4, weight=P + 4, y=Q + 4), dict(in_elu=0)):
        assert lib.di_head_conv_f32_batch_check(ctypes.byref(conv_args(**kw)), items, p, len(items)) == 0, kw
    one = good_items([(33, 70)])
    assert lib.di_head_conv_f32_batch_check(ctypes.byref(conv_args()), one, p, 1) == 0


def test_conv_f32_batch_shared_argument_refusals_without_gpu():
    """Every DI_EINVAL of di_head_conv_f32_check on the shared arguments, with a good table: the batch's
    verdict is the single call's on an item's sizes."""
    lib = _lib.load()
    p = ctypes.c_void_p(P)
    items = good_items()

    def call(**kw):
        a, single = conv_args(**kw), conv_args(**kw)
        single.h, single.w = 145, 145
        rc = lib.di_head_conv_f32_batch(ctypes.byref(a), items, p, len(items), None)
        assert rc == lib.di_head_conv_f32_batch_check(ctypes.byref(a), items, p, len(items)), kw
        assert rc == lib.di_head_conv_f32_check(ctypes.byref(single)), kw
        return rc

    assert lib.di_head_conv_f32_batch(None, items, p, len(items), None) == EINVAL
    assert lib.di_head_conv_f32_batch_check(None, items, p, len(items)) == EINVAL
    for name in ("x", "weight", "y"):
        assert call(**{name: None}) == EINVAL, name
    assert call(y=P) == EINVAL                                  # y == x
    for kw in (dict(cin=32), dict(cin=96), dict(cin=0), dict(cin=512), dict(cout=32), dict(cout=256), dict(cout=2),
               dict(ksize=2), dict(ksize=5), dict(ksize=0), dict(dilation=0), dict(dilation=9), dict(dilation=-1),
               dict(x=P + 1), dict(x=P + 2), dict(weight=P + 2), dict(y=Q + 2), dict(y=Q + 3), dict(stats=Q + 4)):
        assert call(**kw) == EINVAL, kw
    # args->h and args->w are ignored
    assert lib.di_head_conv_f32_batch_check(ctypes.byref(conv_args(h=-5, w=0)), items, p, len(items)) == 0
    # a range refusal of the single call, on one item's own sizes
    tall = good_items(BATCH[:2] + [(16 * 65535 + 1, 1)] + BATCH[2:])
    assert lib.di_head_conv_f32_batch(ctypes.byref(conv_args()), tall, p, len(tall), None) == ERANGE
    assert lib.di_head_conv_f32_batch_check(ctypes.byref(conv_args()), tall, p, len(tall)) == ERANGE
    # ... which a 1x1 over the same table does not have
    assert lib.di_head_conv_f32_batch_check(ctypes.byref(conv_args(ksize=1, dilation=1)), tall, p, len(tall)) == 0
    # the bf16 batch keeps refusing fp32
    assert lib.di_head_conv_batch(_lib.DI_F32, ctypes.byref(conv_args()), items, p, len(items), None) == EINVAL


def test_norm_f32_batch_refusals_without_gpu():
    lib = _lib.load()
    p, q = ctypes.c_void_p(P), ctypes.c_void_p(Q)
    odd4, odd8 = ctypes.c_void_p(P + 4), ctypes.c_void_p(P + 8)      # 4- and 8-byte aligned only: no 16-B vectors
    items = good_items()
    n = len(items)
    assert lib.di_plane_stats_f32_batch(None, 128, items, p, n, q, None) == EINVAL
    assert lib.di_plane_stats_f32_batch(p, 128, items, p, n, None, None) == EINVAL
    assert lib.di_plane_stats_f32_batch(odd4, 128, items, p, n, q, None) == EINVAL
    assert lib.di_plane_stats_f32_batch(odd8, 128, items, p, n, q, None) == EINVAL
    assert lib.di_plane_stats_f32_batch(p, 128, items, p, n, odd4, None) == EINVAL      # stats: 8-byte aligned
    # items must start 16-B aligned (a multiple of 4 channels); the statistics room is for <= 128 channels
    for ch in (0, -1, 1, 2, 6, 99, 130, 132, 256):
        assert lib.di_plane_stats_f32_batch(p, ch, items, p, n, q, None) == EINVAL, ch
    for args in ((None, p, p, p, q), (p, None, p, p, q), (p, p, p, None, q), (p, p, p, p, None),
                 (odd4, p, p, p, q), (odd8, p, p, p, q), (p, p, p, odd8, q), (p, p, p, p, odd8), (p, p, p, p, odd4)):
        x, s, b, r, y = args
        assert lib.di_se_scale_add_f32_batch(x, s, b, r, 128, items, p, n, y, None) == EINVAL
    for ch in (0, -8, 1, 2, 6, 99, 65536):
        assert lib.di_se_scale_add_f32_batch(p, p, p, p, ch, items, p, n, q, None) == EINVAL, ch
    # the bf16 entry points keep refusing fp32
    assert lib.di_plane_stats_batch(_lib.DI_F32, p, 128, items, p, n, q, None) == EINVAL
    assert lib.di_se_scale_add_batch(_lib.DI_F32, p, p, p, p, 128, items, p, n, q, None) == EINVAL


def test_model_option_validation():
    from deepinteract_amd.modules import LitGINI
    assert LitGINI().head_batch_f32 == 0 and LitGINI(head_convs="hip_f32").head_batch_f32 == 0
    m = LitGINI(head_convs="hip_f32", head_batch_f32=4)
    assert m.head_batch_f32 == 4 and m.head_batch == 0 and m.head_batch_pixels == 2 ** 22
    assert m.head_dtype == torch.float32 and m.head_body == "python"
    m = LitGINI(head_convs="hip_f32", head_batch_f32=4, fuse_head_prologue=True, use_interact_attention=True)
    assert m.head_batch_f32 == 4 and m.fuse_head_prologue and m.interact_module.use_attention
    for kw in (dict(head_convs="hip", head_dtype=torch.bfloat16), dict(head_convs="torch"), dict()):
        with pytest.raises(ValueError, match="head_batch_f32"):
            LitGINI(head_batch_f32=4, **kw)
    with pytest.raises(ValueError):
        LitGINI(head_convs="hip_f32", head_batch_f32=4, head_body="native")
    with pytest.raises(ValueError):
        LitGINI(head_convs="hip_f32", head_batch_f32=-1)
    with pytest.raises(ValueError):
        LitGINI(head_convs="hip_f32", head_batch_f32=4, head_batch_pixels=0)
    # head_batch stays the bf16 option
    with pytest.raises(ValueError, match="bf16-only batch"):
        LitGINI(head_convs="hip_f32", head_batch=4)
    # head_batch's chunking, with the fp32 count
    m = LitGINI(head_convs="hip_f32", head_batch_f32=3, head_batch_pixels=100)
    assert m._head_chunks([(5, 5), (5, 5), (9, 9), (20, 20), (1, 1), (1, 1), (1, 1), (1, 1)]) == \
        [[0, 1], [2], [3], [4, 5, 6], [7]]
