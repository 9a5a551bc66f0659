"""The batched contact head without a GPU: di_head_item against the header, the layout
di_head_batch_layout fills, every refusal of the *_batch entry points and di_se_gate before a launch
(dummy pointers are never dereferenced), and the model option's validation."""
import ctypes

import pytest

from deepinteract_amd import _lib
from test_capi import _declared_arg_counts, _declared_struct_fields

EINVAL, ERANGE = -1, -2
P, Q = 16 * 1024, 32 * 1024      # dummy non-NULL, 16-B aligned pointers
SHAPES = [(1, 1), (3, 5), (145, 145), (16, 16), (17, 9), (33, 70), (1000, 1000), (7, 4096)]


def head_items(shapes):
    items = (_lib.DiHeadItem * len(shapes))()
    for it, (h, w) in zip(items, shapes):
        it.h, it.w = h, w
    return items


def layout(items, count=None):
    px, nb = ctypes.c_int64(-7), ctypes.c_int64(-7)
    rc = _lib.load().di_head_batch_layout(items, len(items) if count is None else count, ctypes.byref(px),
                                          ctypes.byref(nb))
    return rc, px.value, nb.value


def test_item_layout_and_signatures():
    assert [f for f, _ in _lib.DiHeadItem._fields_] == _declared_struct_fields("di_head_item")
    assert [t for _, t in _lib.DiHeadItem._fields_] == [ctypes.c_int64] * 2 + [ctypes.c_int32] * 2
    assert ctypes.sizeof(_lib.DiHeadItem) == 24
    decl = _declared_arg_counts()
    for name, n in (("di_head_batch_layout", 4), ("di_head_conv_batch", 6), ("di_plane_stats_batch", 8),
                    ("di_head_norm_fold_batch", 13), ("di_se_scale_add_batch", 11), ("di_se_gate", 10)):
        assert decl[name] == n == len(_lib._SIGS[name][0]), name
    assert _lib.load().di_abi_version() == _lib.ABI_VERSION == 8


def test_layout_offsets_and_sizes():
    lib = _lib.load()
    items = head_items(SHAPES)
    rc, px, nb = layout(items)
    assert rc == 0
    at_px = at_st = 0
    for it, (h, w) in zip(items, SHAPES):
        assert it.px_off == at_px and it.stats_off == at_st        # prefix sums, in order
        assert it.stats_off % 16 == 0
        at_px += h * w
        at_st += (max(lib.di_head_conv_stats_bytes(c, h, w) for c in (64, 128)) + 15) // 16 * 16
    assert px == at_px == sum(h * w for h, w in SHAPES) and nb == at_st
    # every item's room holds either channel count's single-call buffer
    ends = [it.stats_off for it in items[1:]] + [nb]
    for it, end, (h, w) in zip(items, ends, SHAPES):
        for c in (64, 128):
            assert end - it.stats_off >= lib.di_head_conv_stats_bytes(c, h, w) > 0
    # a batch of one
    one = head_items([(145, 145)])
    assert layout(one) == (0, 145 * 145, (lib.di_head_conv_stats_bytes(128, 145, 145) + 15) // 16 * 16)
    assert one[0].px_off == 0 and one[0].stats_off == 0
    # refusals leave the outputs alone
    assert layout(items, 0) == (EINVAL, -7, -7) and layout(items, -1)[0] == EINVAL
    many = head_items([(8, 8)] * (_lib.DI_BATCH_MAX + 1))
    assert layout(many)[0] == ERANGE and layout(many, _lib.DI_BATCH_MAX)[0] == 0
    px, nb = ctypes.c_int64(), ctypes.c_int64()
    assert lib.di_head_batch_layout(None, 1, ctypes.byref(px), ctypes.byref(nb)) == EINVAL
    assert lib.di_head_batch_layout(items, len(items), None, ctypes.byref(nb)) == EINVAL
    assert lib.di_head_batch_layout(items, len(items), ctypes.byref(px), None) == EINVAL
    for bad in ((0, 5), (5, 0), (-1, 5), (5, -3)):
        assert layout(head_items(SHAPES[:3] + [bad] + SHAPES[3:]))[0] == EINVAL, bad
    big = head_items([((1 << 31) - 1, (1 << 31) - 1)])
    assert layout(big)[0] == ERANGE


def _setter(**kw):
    def edit(obj):
        for k, v in kw.items():
            setattr(obj, k, v)
    return edit


def conv_args(**kw):
    a = _lib.DiHeadConvArgs(P, P, None, None, None, Q, None, 64, 64, 0, 0, 3, 2, 1)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


BATCH = SHAPES[:6]
MID = 2


def _calls():
    """name -> callable(items, items_dev, count) for each batch entry point with good shared arguments."""
    lib = _lib.load()
    p, q, f = ctypes.c_void_p(P), ctypes.c_void_p(Q), ctypes.c_float(1e-6)
    return {
        "conv": lambda it, dev, n: lib.di_head_conv_batch(_lib.DI_BF16, ctypes.byref(conv_args()), it, dev, n, None),
        "stats": lambda it, dev, n: lib.di_plane_stats_batch(_lib.DI_BF16, p, 128, it, dev, n, q, None),
        "fold": lambda it, dev, n: lib.di_head_norm_fold_batch(p, 128, it, dev, n, p, p, f, p, q, q, q, None),
        "se": lambda it, dev, n: lib.di_se_scale_add_batch(_lib.DI_BF16, p, p, p, p, 128, it, dev, n, q, None),
    }


@pytest.mark.parametrize("name", ["conv", "stats", "fold", "se"])
def test_item_table_refusals_without_gpu(name):
    """Every refusal happens before any launch: there is no GPU here, and no pointer is dereferenced."""
    fn = _calls()[name]
    p = ctypes.c_void_p(P)

    def call(edit=None, count=None, host=True, dev=p, at=MID):
        items = head_items(BATCH)
        assert layout(items)[0] == 0
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
    # offsets the helper did not fill
    assert call(_setter(px_off=0)) == EINVAL and call(_setter(stats_off=16)) == EINVAL
    assert call(_setter(px_off=1), at=0) == EINVAL and call(_setter(stats_off=8), at=0) == EINVAL
    assert call(_setter(h=144)) == EINVAL and call(_setter(w=146)) == EINVAL   # sizes changed after the layout
    fresh = head_items(BATCH)                                                 # never laid out
    assert fn(fresh, p, len(fresh)) == EINVAL


def test_conv_batch_shared_argument_refusals_without_gpu():
    """Every refusal of di_head_conv_check on the shared arguments, with a good table."""
    lib = _lib.load()
    p = ctypes.c_void_p(P)
    items = head_items(BATCH)
    assert layout(items)[0] == 0

    def call(dt=_lib.DI_BF16, **kw):
        a = conv_args(**kw)
        single = conv_args(**kw)
        single.h, single.w = 145, 145
        rc = lib.di_head_conv_batch(dt, ctypes.byref(a), items, p, len(items), None)
        assert rc == lib.di_head_conv_check(dt, ctypes.byref(single)), kw     # the single call's verdict
        return rc

    assert lib.di_head_conv_batch(_lib.DI_BF16, None, items, p, len(items), None) == EINVAL
    assert call(dt=_lib.DI_F32) == EINVAL and call(dt=5) == EINVAL
    for name in ("x", "weight", "y"):
        assert call(**{name: None}) == EINVAL, name
    assert call(y=P) == EINVAL                                  # y == x
    for kw in (dict(cin=96), dict(cin=0), dict(cin=512), dict(cout=32), dict(cout=256), dict(ksize=2),
               dict(ksize=5), dict(dilation=0), dict(dilation=9), dict(x=P + 1), dict(weight=P + 1),
               dict(y=Q + 1), dict(stats=Q + 4)):
        assert call(**kw) == EINVAL, kw
    # a range refusal of the single call, on one item's own sizes
    tall = head_items(BATCH[:2] + [(16 * 65535 + 1, 1)] + BATCH[2:])
    assert layout(tall)[0] == 0
    assert lib.di_head_conv_batch(_lib.DI_BF16, ctypes.byref(conv_args()), tall, p, len(tall), None) == ERANGE


def test_norm_batch_and_gate_refusals_without_gpu():
    lib = _lib.load()
    p, q, f = ctypes.c_void_p(P), ctypes.c_void_p(Q), ctypes.c_float(1e-6)
    odd, odd8 = ctypes.c_void_p(P + 8), ctypes.c_void_p(P + 4)
    items = head_items(BATCH)
    assert layout(items)[0] == 0
    n = len(items)
    bf = _lib.DI_BF16
    assert lib.di_plane_stats_batch(_lib.DI_F32, p, 128, items, p, n, q, None) == EINVAL     # bf16 only
    assert lib.di_plane_stats_batch(bf, None, 128, items, p, n, q, None) == EINVAL
    assert lib.di_plane_stats_batch(bf, p, 128, items, p, n, None, None) == EINVAL
    assert lib.di_plane_stats_batch(bf, odd, 128, items, p, n, q, None) == EINVAL
    assert lib.di_plane_stats_batch(bf, p, 128, items, p, n, odd8, None) == EINVAL
    for ch in (0, -1, 100, 256):      # items must start 16-B aligned; the statistics room is for <= 128 channels
        assert lib.di_plane_stats_batch(bf, p, ch, items, p, n, q, None) == EINVAL, ch
    assert lib.di_head_norm_fold_batch(None, 128, items, p, n, p, p, f, p, q, q, q, None) == EINVAL
    assert lib.di_head_norm_fold_batch(odd8, 128, items, p, n, p, p, f, p, q, q, q, None) == EINVAL
    assert lib.di_head_norm_fold_batch(p, 0, items, p, n, p, p, f, p, q, q, q, None) == EINVAL
    assert lib.di_head_norm_fold_batch(p, 129, items, p, n, p, p, f, p, q, q, q, None) == EINVAL
    assert lib.di_head_norm_fold_batch(p, 128, items, p, n, p, p, ctypes.c_float(-1.0), p, q, q, q, None) == EINVAL
    assert lib.di_head_norm_fold_batch(p, 128, items, p, n, p, p, ctypes.c_float(float("nan")), p, q, q, q,
                                       None) == EINVAL
    assert lib.di_se_scale_add_batch(_lib.DI_F32, p, p, p, p, 128, items, p, n, q, None) == EINVAL
    for args in ((None, p, p, p, q), (p, None, p, p, q), (p, p, p, None, q), (p, p, p, p, None),
                 (odd, p, p, p, q), (p, p, p, odd, q), (p, p, p, p, odd)):
        x, s, b, r, y = args
        assert lib.di_se_scale_add_batch(bf, x, s, b, r, 128, items, p, n, y, None) == EINVAL
    for ch in (0, -8, 100):
        assert lib.di_se_scale_add_batch(bf, p, p, p, p, ch, items, p, n, q, None) == EINVAL, ch
    # di_se_gate
    for i in range(5):
        ptrs = [p] * 5
        ptrs[i] = None
        assert lib.di_se_gate(*ptrs, 4, 128, 8, q, None) == EINVAL
    assert lib.di_se_gate(p, p, p, p, p, 4, 128, 8, None, None) == EINVAL
    for count, ch, hid in ((0, 128, 8), (-1, 128, 8), (4, 0, 8), (4, 1025, 8), (4, 128, 0), (4, 128, 65)):
        assert lib.di_se_gate(p, p, p, p, p, count, ch, hid, q, None) == EINVAL, (count, ch, hid)


def test_model_option_validation():
    import torch
    from deepinteract_amd.modules import LitGINI
    assert LitGINI().head_batch == 0
    with pytest.raises(ValueError):
        LitGINI(head_batch=4)
    with pytest.raises(ValueError):
        LitGINI(head_batch=4, head_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        LitGINI(head_batch=-1)
    with pytest.raises(ValueError):
        LitGINI(head_dtype=torch.bfloat16, head_convs="hip", head_batch=4, head_batch_pixels=0)
    m = LitGINI(head_dtype=torch.bfloat16, head_convs="hip", head_batch=4)
    assert m.head_batch == 4 and m.head_batch_pixels == 2 ** 22
    m = LitGINI(head_dtype=torch.bfloat16, head_convs="hip", head_batch=3, head_batch_pixels=100)
    assert m._head_chunks([(5, 5), (5, 5), (9, 9), (20, 20), (1, 1), (1, 1), (1, 1), (1, 1)]) == \
        [[0, 1], [2], [3], [4, 5, 6], [7]]
    # without the option nothing is chunked
    assert LitGINI(head_dtype=torch.bfloat16, head_convs="hip").head_batch == 0
