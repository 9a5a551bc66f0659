"""Host side of the head convolutions (csrc/head_conv.hip): di_head_conv_check's refusals, the
statistics buffer's size and LitGINI's ``head_convs`` option. No GPU: the check is host-only, so the
pointers are dummies that are never dereferenced."""
import ctypes
import os
import re

import pytest
import torch

from deepinteract_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DI_EINVAL = -1


def _args(**kw):
    a = dict(x=0x1000, weight=0x2000, in_scale=0x3000, in_shift=0x4000, bias=0x5000, y=0x6000, stats=0x7000,
             cin=64, cout=64, h=33, w=70, ksize=3, dilation=2, in_elu=1)
    a.update(kw)
    return _lib.DiHeadConvArgs(**a)


def _check(dt=_lib.DI_BF16, **kw):
    return _lib.load().di_head_conv_check(dt, ctypes.byref(_args(**kw)))


def test_valid_sets_pass():
    assert _check() == 0
    assert _check(in_scale=None, in_shift=None, bias=None, stats=None, in_elu=0) == 0
    for cin in (64, 128, 256):
        for cout in (64, 128):
            assert _check(cin=cin, cout=cout, ksize=1, dilation=1) == 0
    for d in range(1, 9):
        assert _check(dilation=d) == 0
    assert _check(h=1, w=1) == 0
    assert _check(h=4100, w=4100, dilation=8) == 0


@pytest.mark.parametrize("kw", [
    dict(dt=_lib.DI_F32), dict(dt=5), dict(cin=32), dict(cin=96), dict(cin=512), dict(cout=32), dict(cout=256),
    dict(cout=2), dict(ksize=2), dict(ksize=5), dict(ksize=0), dict(dilation=0), dict(dilation=9), dict(dilation=-1),
    dict(x=None), dict(weight=None), dict(y=None), dict(y=0x1000), dict(h=0), dict(w=0), dict(x=0x1001),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_each_refusal(kw):
    assert _check(**kw) == DI_EINVAL


def test_null_args_refused():
    lib = _lib.load()
    assert lib.di_head_conv_check(_lib.DI_BF16, None) == DI_EINVAL
    assert lib.di_head_conv(_lib.DI_BF16, None, None) == DI_EINVAL
    # di_head_conv validates before any launch: the dummy pointers are never touched
    assert lib.di_head_conv(_lib.DI_F32, ctypes.byref(_args()), None) == DI_EINVAL
    assert lib.di_head_conv(_lib.DI_BF16, ctypes.byref(_args(y=0x1000)), None) == DI_EINVAL
    assert lib.di_plane_stats(_lib.DI_BF16, None, 64, 100, ctypes.c_void_p(0x1000), None) == DI_EINVAL
    assert lib.di_plane_stats(_lib.DI_BF16, ctypes.c_void_p(0x1000), 64, 0, ctypes.c_void_p(0x1000), None) == DI_EINVAL
    assert lib.di_head_norm_fold(None, 64, 100, None, None, 1e-6, None, None, None, None, None) == DI_EINVAL
    assert lib.di_head_norm_fold(ctypes.c_void_p(0x1000), 0, 100, None, None, 1e-6, None, None, None, None,
                                 None) == DI_EINVAL


def test_stats_bytes_positive_and_monotone_in_cout():
    lib = _lib.load()
    for h, w in ((1, 1), (3, 5), (145, 145), (1000, 1000), (4100, 4100)):
        b = [lib.di_head_conv_stats_bytes(c, h, w) for c in (1, 7, 64, 128)]
        assert b[0] > 0 and all(x < y for x, y in zip(b, b[1:])), (h, w, b)
        # one fp64 pair per 16 x 16 tile / 256-pixel run and channel fits
        tiles = max(-(-h // 16) * -(-w // 16), -(-h * w // 256))
        assert b[2] >= 16 + 64 * tiles * 16
    assert lib.di_head_conv_stats_bytes(0, 10, 10) < 0
    assert lib.di_head_conv_stats_bytes(64, 0, 10) < 0


def test_ctypes_struct_matches_header():
    src = open(os.path.join(ROOT, "include", "deepinteract_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*di_head_conv_args;", src).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [f.strip().lstrip("*") for f in decl.split(None, 1)[1].split(",")] if "," in decl \
                else [decl.split()[-1].lstrip("*")]
    assert [f for f, _ in _lib.DiHeadConvArgs._fields_] == fields
    assert ctypes.sizeof(_lib.DiHeadConvArgs) == 7 * 8 + 7 * 4 + 4


def test_litgini_head_convs_option():
    from deepinteract_amd.modules import LitGINI
    with pytest.raises(ValueError):
        LitGINI(head_convs="hip")  # the default head_dtype is fp32
    with pytest.raises(ValueError):
        LitGINI(head_convs="hip", head_dtype=torch.bfloat16, head_hip_ops=False)
    with pytest.raises(ValueError):
        LitGINI(head_convs="hip", head_dtype=torch.bfloat16, head_channels_last=True)
    with pytest.raises(ValueError):
        LitGINI(head_convs="miopen")
    m = LitGINI(head_convs="hip", head_dtype=torch.bfloat16)
    assert m.head_convs == "hip"
    assert LitGINI().head_convs == "torch"
