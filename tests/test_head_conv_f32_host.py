"""Host side of the fp32 head convolutions (csrc/head_conv_f32.hip): di_head_conv_f32_check's refusals
-- those of di_head_conv_check (test_head_conv_host.py) but the dtype's, with 4-byte alignment -- and
LitGINI's ``head_convs="hip_f32"``. No GPU: the check is host-only, so the pointers are dummies that are
never dereferenced."""
import ctypes

import pytest
import torch

from deepinteract_amd import _lib

DI_EINVAL = -1


def _args(**kw):
    a = dict(x=0x1000, weight=0x2000, in_scale=0x3000, in_shift=0x4000, bias=0x5000, y=0x6000, stats=0x7000,
             cin=64, cout=64, h=33, w=70, ksize=3, dilation=2, in_elu=1)
    a.update(kw)
    return _lib.DiHeadConvArgs(**a)


def _check(**kw):
    return _lib.load().di_head_conv_f32_check(ctypes.byref(_args(**kw)))


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
    dict(cin=32), dict(cin=96), dict(cin=512), dict(cout=32), dict(cout=256),
    dict(cout=2), dict(ksize=2), dict(ksize=5), dict(ksize=0), dict(dilation=0), dict(dilation=9), dict(dilation=-1),
    dict(x=None), dict(weight=None), dict(y=None), dict(y=0x1000), dict(h=0), dict(w=0), dict(x=0x1001),
    dict(x=0x1002), dict(weight=0x2002), dict(y=0x6002), dict(stats=0x7004),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_each_refusal(kw):
    assert _check(**kw) == DI_EINVAL


def test_ranges_refused():
    assert _check(h=16 * 65535 + 1, w=1) == -2                    # ksize 3: grid.y
    assert _check(h=2 ** 31 - 1, w=2 ** 10, ksize=1) == -2        # ksize 1: grid.x


def test_null_args_refused_and_no_launch():
    lib = _lib.load()
    assert lib.di_head_conv_f32_check(None) == DI_EINVAL
    assert lib.di_head_conv_f32(None, None) == DI_EINVAL
    # di_head_conv_f32 validates before any launch: the dummy pointers are never touched
    assert lib.di_head_conv_f32(ctypes.byref(_args(y=0x1000)), None) == DI_EINVAL
    assert lib.di_head_conv_f32(ctypes.byref(_args(x=0x1002)), None) == DI_EINVAL
    assert lib.di_head_conv_f32(ctypes.byref(_args(cin=96)), None) == DI_EINVAL
    # the bf16 entry point keeps refusing fp32
    assert lib.di_head_conv_check(_lib.DI_F32, ctypes.byref(_args())) == DI_EINVAL


def test_litgini_head_convs_hip_f32_option():
    from deepinteract_amd.modules import LitGINI
    m = LitGINI(head_convs="hip_f32")
    assert m.head_convs == "hip_f32" and m.head_dtype == torch.float32 and m.head_batch == 0
    assert LitGINI(head_convs="hip_f32", fuse_head_prologue=True, use_interact_attention=True).head_convs == "hip_f32"
    for kw in (dict(head_dtype=torch.bfloat16), dict(head_hip_ops=False), dict(head_channels_last=True)):
        with pytest.raises(ValueError):
            LitGINI(head_convs="hip_f32", **kw)
    for kw in (dict(head_batch=4), dict(head_body="native")):
        with pytest.raises(ValueError, match="bf16-only batch"):
            LitGINI(head_convs="hip_f32", **kw)
    with pytest.raises(ValueError):
        LitGINI(head_convs="hip")  # still bf16 only
    assert LitGINI().head_convs == "torch"
