"""Dilated-ResNet contact head — on PyTorch-ROCm (MIOpen convolutions) by default, as north_star
specifies; opt-in, the head's convolutions run on HIP (HeadConvOps: csrc/head_conv.hip for the bf16 head,
csrc/head_conv_f32.hip for the fp32 one), for one complex at a time or for a ragged batch of
complexes with one launch per pass (HeadBatch, body_batch; bf16 or fp32). Module/parameter names match the reference's ``interact_module`` so reference
state dicts load unchanged: ResNet2DInputWithOptAttention (deepinteract_modules.py:1155-1248),
ResNet (:973-1106), SEBlock (:954-970), MultiHeadRegionalAttention (:1109-1152). The optional regional
attention (``use_interact_attention``: MHA2D_1 / MHA2D_2 behind the two ResNets) runs its scores and its
3x3 softmax-weighted mix on HIP (HeadAttnOps, csrc/head_attn.hip) wherever the HIP norm passes run, and as
plain torch otherwise; neither forms the reference's ninefold stretch of q, k and v.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from .engine import _ptr, _stream


class HeadNormOps:
    """The head's HBM-bound passes on HIP (csrc/head_ops.hip): ELU(InstanceNorm2d(x))
    in 3 plane passes instead of torch's 5, and SEBlock gate + residual add in 3 instead of 5.
    Inputs: one [1, C, H, W] NCHW-contiguous image, fp32 or bf16, on the GPU. No CPU fallback:
    constructing it without the HIP library / a GPU raises."""

    def __init__(self, device):
        from . import _lib
        if not torch.cuda.is_available():
            raise RuntimeError("HeadNormOps needs a ROCm GPU (no CPU fallback)")
        self._lib = _lib
        self.lib = _lib.load()
        self.device = torch.device(device)
        self._work = None
        self._f32 = {}  # fp32 copies of (bf16) per-channel parameters, made once per parameter

    def f32(self, p):
        """fp32 contiguous copy of a (possibly bf16) per-channel parameter, cached."""
        if p is None:
            return None
        hit = self._f32.get(id(p))
        # the entry holds p itself, so its id cannot be reused by another tensor while cached
        if hit is None or hit[0] is not p or hit[1] != p._version:
            hit = self._f32[id(p)] = (p, p._version, p.detach().float().contiguous())
        return hit[2]

    def work(self, C, hw, device):
        nb = self.lib.di_inorm_work_bytes(C, hw)
        if self._work is None or self._work.numel() * 8 < nb:
            self._work = torch.empty((nb + 7) // 8, dtype=torch.float64, device=device)
        return self._work

    def _dt(self, x):
        if x.dtype == torch.float32:
            return self._lib.DI_F32
        if x.dtype == torch.bfloat16:
            return self._lib.DI_BF16
        raise TypeError(f"head ops take fp32 / bf16, got {x.dtype}")

    @staticmethod
    def _check(x):
        if x.dim() != 4 or x.shape[0] != 1 or not x.is_contiguous() or not x.is_cuda:
            raise ValueError("head ops take one contiguous NCHW [1, C, H, W] GPU image")

    def inorm_elu(self, x, norm: nn.InstanceNorm2d, out=None):
        """F.elu(norm(x)); out may be x (in place)."""
        self._check(x)
        C, hw = x.shape[1], x.shape[2] * x.shape[3]
        y = torch.empty_like(x) if out is None else out
        w = self.work(C, hw, x.device)
        g, b = self.f32(norm.weight), self.f32(norm.bias)
        self._lib.check(self.lib.di_inorm_elu(self._dt(x), _ptr(x), C, hw, _ptr(g), _ptr(b), ctypes.c_float(norm.eps),
                                              _ptr(w), _ptr(y), _stream()), "di_inorm_elu")
        return y

    def channel_mean(self, x, bias=None):
        """x.mean(dim=(2, 3)) (+ bias) as fp32 [1, C]."""
        self._check(x)
        C, hw = x.shape[1], x.shape[2] * x.shape[3]
        w = self.work(C, hw, x.device)
        m = torch.empty(1, C, dtype=torch.float32, device=x.device)
        b = self.f32(bias)
        self._lib.check(self.lib.di_channel_mean(self._dt(x), _ptr(x), C, hw, _ptr(b), _ptr(w), _ptr(m), _stream()),
                        "di_channel_mean")
        return m

    def se_scale_add(self, x, scale, res, out=None, bias=None):
        """(x + bias[None, :, None, None]) * scale[None, :, None, None] + res; out may be x or res."""
        self._check(x)
        self._check(res)
        C, hw = x.shape[1], x.shape[2] * x.shape[3]
        s = scale.detach().reshape(-1).float().contiguous()
        b = self.f32(bias)
        y = torch.empty_like(x) if out is None else out
        self._lib.check(self.lib.di_se_scale_add(self._dt(x), _ptr(x), _ptr(s), _ptr(b), _ptr(res), C, hw, _ptr(y),
                                                 _stream()), "di_se_scale_add")
        return y


    def se_scale_add_batch(self, hb, x, scale, res, out=None, bias=None):
        """se_scale_add for every image of a HeadBatch in one launch: x, res, out packed [C * pixels]
        buffers of the batch's dtype (out may be x or res; None: a new buffer), scale [count, C] fp32 rows,
        bias [C] shared. bf16: di_se_scale_add_batch; fp32: di_se_scale_add_f32_batch."""
        C = scale.shape[1]
        hb.check_packed(x, C), hb.check_packed(res, C)
        if scale.dtype != torch.float32 or not scale.is_contiguous() or scale.shape[0] != hb.count:
            raise ValueError("the batch's gates are contiguous fp32 [count, C] rows")
        b = self.f32(bias)
        y = torch.empty_like(x) if out is None else out
        hb.check_packed(y, C)
        if hb.dtype == torch.float32:
            self._lib.check(self.lib.di_se_scale_add_f32_batch(_ptr(x), _ptr(scale), _ptr(b), _ptr(res), C, hb.items,
                                                               hb.items_ptr, hb.count, _ptr(y), _stream()),
                            "di_se_scale_add_f32_batch")
        else:
            self._lib.check(self.lib.di_se_scale_add_batch(self._lib.DI_BF16, _ptr(x), _ptr(scale), _ptr(b), _ptr(res),
                                                           C, hb.items, hb.items_ptr, hb.count, _ptr(y), _stream()),
                            "di_se_scale_add_batch")
        return y

    def se_gate(self, se, mean, out=None):
        """SEBlock's gate sigmoid(relu(linear2(relu(linear1(mean))))) for [count, C] fp32 means, all in
        fp32 with a fixed accumulation order (di_se_gate; one launch): fp32 [count, C]."""
        if mean.dtype != torch.float32 or mean.dim() != 2 or not mean.is_contiguous() or not mean.is_cuda:
            raise ValueError("se_gate takes contiguous fp32 [count, C] GPU means")
        count, C = mean.shape
        w1, b1, w2, b2 = (self.f32(t) for t in (se.linear1.weight, se.linear1.bias, se.linear2.weight,
                                                 se.linear2.bias))
        hidden = w1.shape[0]
        if tuple(w1.shape) != (hidden, C) or tuple(w2.shape) != (C, hidden):
            raise ValueError(f"the SE block takes {w1.shape[1]} channels, the means have {C}")
        g = torch.empty_like(mean) if out is None else out
        self._lib.check(self.lib.di_se_gate(*(_ptr(t) for t in (mean, w1, b1, w2, b2)), count, C, hidden, _ptr(g),
                                            _stream()), "di_se_gate")
        return g


class HeadBatch:
    """A ragged batch of head images for the batched HIP head (di_head_item, include/deepinteract_amd.h):
    built once from the images' (h, w), it owns the device copy of the item table, the statistics
    buffer, the per-item fp32 rows (scale, shift, mean, gate) and the arena every layer of a forward
    works in -- two 128-channel packed buffers (the residual stream and a block's output, swapping
    roles from block to block) and two 64-channel ones: 768 B per pixel in bf16 (the default), 1536 B per
    pixel with dtype=torch.float32 (the fp32 parity head). Nothing is allocated per layer and nothing is
    copied to the device after construction.

    Item i of a packed [C * pixels] buffer is the contiguous NCHW image ``view(buf, C, i)``. Fill
    ``input(i)`` (a [1, 128, h, w] view of the residual stream) with ELU(inorm_1(conv2d_1(T_i))) for
    every i, then call ``ResNet2DInputWithOptAttention.body_batch(batch)``."""

    CHANNELS = 128

    def __init__(self, shapes, device, dtype=torch.bfloat16):
        from . import _lib
        from .ranking import _table_to_device
        if dtype not in (torch.bfloat16, torch.float32):
            raise TypeError(f"a head batch holds bf16 or fp32 images, got {dtype}")
        self.dtype = dtype
        shapes = [(int(h), int(w)) for h, w in shapes]
        self.shapes, self.count = shapes, len(shapes)
        if not 1 <= self.count <= _lib.DI_BATCH_MAX:
            raise ValueError(f"a head batch holds 1 .. {_lib.DI_BATCH_MAX} images, got {self.count}")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.items = (_lib.DiHeadItem * self.count)()
        for it, (h, w) in zip(self.items, shapes):
            it.h, it.w = h, w
        px, nb = ctypes.c_int64(), ctypes.c_int64()
        rc = _lib.load().di_head_batch_layout(self.items, self.count, ctypes.byref(px), ctypes.byref(nb))
        if rc != 0:
            raise ValueError(f"head batch of shapes {shapes}: code {rc}")
        self.pixels, self.stats_bytes = px.value, nb.value
        self.px_off = [it.px_off for it in self.items]
        self.stats_off = [it.stats_off for it in self.items]
        self.items_dev = _table_to_device(self.items, self.device)
        self.items_ptr = _ptr(self.items_dev)
        C = self.CHANNELS
        kw = dict(dtype=dtype, device=self.device)
        self.wide = [torch.empty(C * self.pixels, **kw) for _ in range(2)]
        self.half = [torch.empty(C // 2 * self.pixels, **kw) for _ in range(2)]
        self.stats = torch.empty(self.stats_bytes // 8, dtype=torch.float64, device=self.device)
        self.rows = torch.empty(4, self.count, C, dtype=torch.float32, device=self.device)

    def check_packed(self, buf, C):
        if buf.dtype != self.dtype or not buf.is_contiguous() or buf.numel() != C * self.pixels \
                or buf.device != self.device:
            raise ValueError(f"a packed buffer of this batch holds {C} x {self.pixels} {self.dtype} elements on "
                             f"{self.device}")

    def view(self, buf, C, i):
        """Item i of a packed C-channel buffer as a [1, C, h, w] view."""
        h, w = self.shapes[i]
        return buf[C * self.px_off[i]:C * (self.px_off[i] + h * w)].view(1, C, h, w)

    def pack(self, images):
        """A new packed buffer holding the [1, C, h, w] images (tests and tools)."""
        C = images[0].shape[1]
        buf = torch.empty(C * self.pixels, dtype=self.dtype, device=self.device)
        for i, im in enumerate(images):
            self.view(buf, C, i).copy_(im)
        return buf

    def input(self, i):
        return self.view(self.wide[0], self.CHANNELS, i)

    def item_stats(self, st, i, C):
        """Item i's header and partials of a batch statistics buffer, as the single call lays them out."""
        at = self.stats_off[i] // 8
        n = int(st[at:at + 1].view(torch.int64).item())
        return st[at:at + 2 + C * n * 2]


class HeadConvOps:
    """The head's convolutions on HIP (csrc/head_conv.hip, csrc/head_conv_f32.hip): 1x1 and dilated 3x3
    on the matrix cores, NCHW, with the InstanceNorm + ELU in front of a convolution applied as it loads
    its input (``ELU(x * scale + shift)``) and the next norm's statistics left by its epilogue. One
    [1, C, H, W] contiguous GPU image per call, bf16 with bf16 weights (di_head_conv) or fp32 with fp32
    weights (di_head_conv_f32); the batch passes take a HeadBatch of either dtype (di_head_conv_batch /
    di_head_conv_f32_batch, di_plane_stats_batch / di_plane_stats_f32_batch). No CPU fallback: constructing it without
    the HIP library / a GPU raises."""

    def __init__(self, device):
        from . import _lib
        if not torch.cuda.is_available():
            raise RuntimeError("HeadConvOps needs a ROCm GPU (no CPU fallback)")
        self._lib = _lib
        self.lib = _lib.load()
        self.device = torch.device(device)
        self._stats = None

    @staticmethod
    def _check(x):
        if x.dim() != 4 or x.shape[0] != 1 or not x.is_contiguous() or not x.is_cuda \
                or x.dtype not in (torch.bfloat16, torch.float32):
            raise ValueError("head convolutions take one contiguous NCHW [1, C, H, W] bf16 or fp32 GPU image")

    @staticmethod
    def _check_params(weight=None, vectors=(), dtype=torch.bfloat16):
        """The checks conv and conv_batch share: the weight tensor (if given; of the image's dtype) and fp32
        per-channel vectors."""
        if weight is not None and (weight.dtype != dtype or not weight.is_contiguous() or weight.dim() != 4):
            raise ValueError(f"head conv weights are the module's contiguous [Cout, Cin, k, k] tensor in the image's "
                             f"dtype ({dtype})")
        for v in vectors:
            if v is not None and (v.dtype != torch.float32 or not v.is_contiguous()):
                raise ValueError("per-channel vectors are contiguous fp32")

    def stats_buffer(self, C, H, W, device):
        """The statistics buffer the next conv / plane_stats writes and the next fold reads (one,
        reused: stream order keeps a fold ahead of the launch that overwrites its input)."""
        nb = self.lib.di_head_conv_stats_bytes(C, H, W)
        if self._stats is None or self._stats.numel() * 8 < nb or self._stats.device != device:
            self._stats = torch.empty((nb + 7) // 8, dtype=torch.float64, device=device)
        return self._stats

    def conv(self, x, weight, bias=None, in_scale=None, in_shift=None, in_elu=False, dilation=1, stats=False):
        """conv2d(T(x), weight, bias, padding=dilation, dilation=dilation) with
        T(x) = ELU?(x * in_scale + in_shift) per channel, zero padding after T. weight: the module's
        [Cout, Cin, k, k] tensor in x's dtype (bf16, or fp32: di_head_conv_f32); bias, in_scale, in_shift: fp32
        per-channel vectors or None. Returns y, or (y, stats buffer) with stats=True."""
        self._check(x)
        self._check_params(weight, (bias, in_scale, in_shift), dtype=x.dtype)
        _, C, H, W = x.shape
        cout, cin, k, _ = weight.shape
        if cin != C:
            raise ValueError(f"weight takes {cin} channels, the image has {C}")
        y = torch.empty(1, cout, H, W, dtype=x.dtype, device=x.device)
        st = self.stats_buffer(cout, H, W, x.device) if stats else None
        args = self._lib.DiHeadConvArgs(x.data_ptr(), weight.data_ptr(), _ptr(in_scale).value,
                                        _ptr(in_shift).value, _ptr(bias).value, y.data_ptr(),
                                        _ptr(st).value, C, cout, H, W, k, int(dilation), int(bool(in_elu)))
        if x.dtype == torch.float32:
            self._lib.check(self.lib.di_head_conv_f32(ctypes.byref(args), _stream()), "di_head_conv_f32")
        else:
            self._lib.check(self.lib.di_head_conv(self._lib.DI_BF16, ctypes.byref(args), _stream()), "di_head_conv")
        return (y, st) if stats else y

    def plane_stats(self, x):
        """The statistics buffer of a stored image (one read pass)."""
        self._check(x)
        _, C, H, W = x.shape
        st = self.stats_buffer(C, H, W, x.device)
        dt = self._lib.DI_F32 if x.dtype == torch.float32 else self._lib.DI_BF16
        self._lib.check(self.lib.di_plane_stats(dt, _ptr(x), C, H * W, _ptr(st), _stream()), "di_plane_stats")
        return st

    def fold(self, st, C, hw, gamma=None, beta=None, eps=0.0, bias=None, want=("scale", "shift")):
        """Fold a statistics buffer into fp32 [C] vectors: scale = gamma / sqrt(var + eps),
        shift = beta - mean * scale, mean = mean (+ bias). Returns the ones named in ``want``, in order."""
        out = {k: torch.empty(C, dtype=torch.float32, device=st.device) for k in want}
        self._lib.check(self.lib.di_head_norm_fold(_ptr(st), C, hw, _ptr(gamma), _ptr(beta),
                                                   ctypes.c_float(eps), _ptr(bias), _ptr(out.get("scale")),
                                                   _ptr(out.get("shift")), _ptr(out.get("mean")),
                                                   _stream()), "di_head_norm_fold")
        return tuple(out[k] for k in want)


    # ---- the same passes over a HeadBatch: one launch each, whatever the number of images ----
    def conv_batch(self, hb, x, weight, y=None, bias=None, in_scale=None, in_shift=None, in_elu=False, dilation=1,
                   stats=False):
        """conv for every image of a HeadBatch: x a packed [Cin * pixels] buffer, y the packed output
        (None: a new buffer), in_scale / in_shift [count, Cin] fp32 rows or None, weight / bias shared.
        With stats=True the batch's statistics buffer is written (every item at its stats_off).
        Buffers and weight in the batch's dtype: bf16 (di_head_conv_batch) or fp32 (di_head_conv_f32_batch).
        Returns y, or (y, hb.stats)."""
        self._check_params(weight, dtype=hb.dtype)
        cout, cin, k, _ = weight.shape
        hb.check_packed(x, cin)
        for v in (in_scale, in_shift):
            if v is not None and (v.dtype != torch.float32 or not v.is_contiguous()
                                  or tuple(v.shape) != (hb.count, cin)):
                raise ValueError("the batch's scale / shift are contiguous fp32 [count, Cin] rows")
        self._check_params(vectors=(bias,))
        if y is None:
            y = torch.empty(cout * hb.pixels, dtype=hb.dtype, device=x.device)
        hb.check_packed(y, cout)
        args = self._lib.DiHeadConvArgs(x.data_ptr(), weight.data_ptr(), _ptr(in_scale).value,
                                        _ptr(in_shift).value, _ptr(bias).value, y.data_ptr(),
                                        hb.stats.data_ptr() if stats else None, cin, cout, 0, 0, k, int(dilation),
                                        int(bool(in_elu)))
        if hb.dtype == torch.float32:
            self._lib.check(self.lib.di_head_conv_f32_batch(ctypes.byref(args), hb.items, hb.items_ptr, hb.count,
                                                            _stream()), "di_head_conv_f32_batch")
        else:
            self._lib.check(self.lib.di_head_conv_batch(self._lib.DI_BF16, ctypes.byref(args), hb.items, hb.items_ptr,
                                                        hb.count, _stream()), "di_head_conv_batch")
        return (y, hb.stats) if stats else y

    def plane_stats_batch(self, hb, x, C):
        """The batch's statistics buffer of a packed C-channel buffer (one read pass)."""
        hb.check_packed(x, C)
        if hb.dtype == torch.float32:
            self._lib.check(self.lib.di_plane_stats_f32_batch(_ptr(x), C, hb.items, hb.items_ptr, hb.count,
                                                              _ptr(hb.stats), _stream()), "di_plane_stats_f32_batch")
        else:
            self._lib.check(self.lib.di_plane_stats_batch(self._lib.DI_BF16, _ptr(x), C, hb.items, hb.items_ptr,
                                                          hb.count, _ptr(hb.stats), _stream()),
                            "di_plane_stats_batch")
        return hb.stats

    def fold_batch(self, hb, st, C, gamma=None, beta=None, eps=0.0, bias=None, want=("scale", "shift"), out=None):
        """fold for every item of a batch statistics buffer: fp32 [count, C] rows. out: a dict of
        preallocated rows by name (None: new tensors)."""
        out = {k: (out[k] if out is not None else torch.empty(hb.count, C, dtype=torch.float32, device=st.device))
               for k in want}
        self._lib.check(self.lib.di_head_norm_fold_batch(_ptr(st), C, hb.items, hb.items_ptr, hb.count,
                                                         _ptr(gamma), _ptr(beta), ctypes.c_float(eps),
                                                         _ptr(bias), _ptr(out.get("scale")),
                                                         _ptr(out.get("shift")), _ptr(out.get("mean")),
                                                         _stream()), "di_head_norm_fold_batch")
        return tuple(out[k] for k in want)


class HeadAttnOps:
    """The head's regional attention on HIP (csrc/head_attn.hip): the per-pixel scores of a
    [1, 128, H, W] image and the 3x3 softmax-weighted mix of its values, fp32 or bf16 storage, for one
    image or for every image of a HeadBatch in one launch each. The value convolution is the caller's
    (torch, or HeadConvOps.conv). No CPU fallback: constructing it without the HIP library / a GPU
    raises."""

    CHANNELS, HEADS, DK = 128, 4, 16

    def __init__(self, device):
        from . import _lib
        if not torch.cuda.is_available():
            raise RuntimeError("HeadAttnOps needs a ROCm GPU (no CPU fallback)")
        self._lib = _lib
        self.lib = _lib.load()
        self.device = torch.device(device)

    def _dt(self, x):
        if x.dtype == torch.float32:
            return self._lib.DI_F32
        if x.dtype == torch.bfloat16:
            return self._lib.DI_BF16
        raise TypeError(f"the regional attention takes fp32 / bf16 images, got {x.dtype}")

    def _check_image(self, x):
        if x.dim() != 4 or x.shape[0] != 1 or x.shape[1] != self.CHANNELS or not x.is_contiguous() or not x.is_cuda:
            raise ValueError("the regional attention takes one contiguous NCHW [1, 128, H, W] GPU image")

    def _check_qk(self, wq, wk):
        for t in (wq, wk):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != self.DK * self.CHANNELS \
                    or t.shape[0] != self.DK or not t.is_cuda:
                raise ValueError("wq / wk are contiguous fp32 [16, 128] GPU tensors (the 1x1 kernels' values)")

    def _check_scores(self, s, px):
        if s.dtype != torch.float32 or not s.is_contiguous() or s.numel() != self.HEADS * px or not s.is_cuda:
            raise ValueError(f"the scores are a contiguous fp32 GPU tensor of 4 x {px} elements")

    def scores(self, x, wq, wk, in_elu=False, out=None):
        """fp32 [4, H, W] scores of x (ELU(x) with in_elu): a pixel's own q.k per head, over sqrt(16)."""
        self._check_image(x)
        self._check_qk(wq, wk)
        _, _, H, W = x.shape
        s = torch.empty(self.HEADS, H, W, dtype=torch.float32, device=x.device) if out is None else out
        self._check_scores(s, H * W)
        args = self._lib.DiRegionAttnArgs(x.data_ptr(), wq.data_ptr(), wk.data_ptr(), s.data_ptr(), None, None,
                                          H, W, int(bool(in_elu)))
        self._lib.check(self.lib.di_region_scores(self._dt(x), ctypes.byref(args), _stream()), "di_region_scores")
        return s

    def mix(self, v, scores, out=None):
        """The softmax over each pixel's 3x3 region of scores (taps outside the image: score 0, value 0,
        kept in the denominator) applied to v's channels of that head. out: None (a new image) or any
        image but v -- the scores' input may be overwritten."""
        self._check_image(v)
        _, _, H, W = v.shape
        self._check_scores(scores, H * W)
        y = torch.empty_like(v) if out is None else out
        self._check_image(y)
        if y.dtype != v.dtype or y.shape != v.shape or y.data_ptr() == v.data_ptr():
            raise ValueError("mix writes an image of v's shape and dtype that is not v")
        args = self._lib.DiRegionAttnArgs(None, None, None, scores.data_ptr(), v.data_ptr(), y.data_ptr(), H, W, 0)
        self._lib.check(self.lib.di_region_mix(self._dt(v), ctypes.byref(args), _stream()), "di_region_mix")
        return y

    # ---- the same over a HeadBatch: one launch each ----
    @staticmethod
    def batch_scores_buffer(hb):
        """The batch's [4 * pixels] fp32 scores in the arena: the front of hb.half[0] (16 of its 128 B per
        pixel in bf16, of its 256 B in fp32), free between two ResNets."""
        half = hb.half[0] if hb.dtype == torch.float32 else hb.half[0].view(torch.float32)
        return half[:HeadAttnOps.HEADS * hb.pixels]

    def scores_batch(self, hb, x, wq, wk, in_elu=False, out=None):
        """scores for every image of a HeadBatch: x a packed [128 * pixels] buffer; returns the packed
        [4 * pixels] fp32 scores (item i at 4 * px_off_i; out: None takes batch_scores_buffer)."""
        hb.check_packed(x, self.CHANNELS)
        self._check_qk(wq, wk)
        s = self.batch_scores_buffer(hb) if out is None else out
        self._check_scores(s, hb.pixels)
        args = self._lib.DiRegionAttnArgs(x.data_ptr(), wq.data_ptr(), wk.data_ptr(), s.data_ptr(), None, None,
                                          0, 0, int(bool(in_elu)))
        self._lib.check(self.lib.di_region_scores_batch(self._dt(x), ctypes.byref(args), hb.items, hb.items_ptr,
                                                        hb.count, _stream()), "di_region_scores_batch")
        return s

    def mix_batch(self, hb, v, scores, y):
        """mix for every image of a HeadBatch: v, y packed [128 * pixels] buffers (y is not v)."""
        hb.check_packed(v, self.CHANNELS), hb.check_packed(y, self.CHANNELS)
        self._check_scores(scores, hb.pixels)
        if y.data_ptr() == v.data_ptr():
            raise ValueError("mix_batch writes a buffer that is not v")
        args = self._lib.DiRegionAttnArgs(None, None, None, scores.data_ptr(), v.data_ptr(), y.data_ptr(), 0, 0, 0)
        self._lib.check(self.lib.di_region_mix_batch(self._dt(v), ctypes.byref(args), hb.items, hb.items_ptr,
                                                     hb.count, _stream()), "di_region_mix_batch")
        return y


class _StretchWeight(nn.Module):
    """The reference's ``stretch_layer`` (a bias-free Conv3d whose fixed one-hot weight copies tap (i, j)
    of the 3x3 region into channel 3 i + j): only its weight is kept, so that a reference state dict
    loads unchanged, and checked on load -- the region it encodes is what forward and the kernels
    compute."""

    def __init__(self, region=3):
        super().__init__()
        from .weights import stretch_weight
        self.region = region
        self.weight = nn.Parameter(stretch_weight(region), requires_grad=False)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        from .weights import stretch_weight
        w = state_dict.get(prefix + "weight")
        want = stretch_weight(self.region)
        if w is not None and tuple(w.shape) == tuple(want.shape) and \
                not torch.equal(w.detach().to("cpu", torch.float32), want):
            raise ValueError(f"{prefix}weight is not the reference's fixed one-hot stretch pattern: the regional "
                             "attention hard-wires it")
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


class MultiHeadRegionalAttention(nn.Module):
    """deepinteract_modules.py:1109-1152 with the head's arguments (d_k 16, d_v = in_dim, output_score=True),
    restated without the ninefold stretch of q, k and v: a pixel's score is its own q.k per head over
    ``temper``; the output is the softmax over the 3x3 region's scores applied to the region's values,
    a tap outside the image counting with score 0 and value 0. Dropout is the identity (inference).
    Plain torch, any device: the path of the CPU head, of ``head_hip_ops=False`` and of a channels-last
    head; HeadAttnOps runs the same on HIP. Returns (out, attention scores [B * n_head, 9, H, W])."""

    def __init__(self, in_dim=128, region_size=3, d_k=16, d_v=128, n_head=4):
        super().__init__()
        if region_size != 3:
            raise NotImplementedError("the regional attention is built for a 3x3 region")
        self.temper = int(d_k ** 0.5)
        self.n_head, self.dk_per_head, self.dv_per_head = n_head, d_k // n_head, d_v // n_head
        self.q_layer = nn.Conv2d(in_dim, d_k, 1, bias=False)
        self.k_layer = nn.Conv2d(in_dim, d_k, 1, bias=False)
        self.v_layer = nn.Conv2d(in_dim, d_v, 1, bias=False)
        self.stretch_layer = _StretchWeight(region_size)

    def forward(self, x):
        B, _, H, W = x.shape
        q, k, v = self.q_layer(x), self.k_layer(x), self.v_layer(x)
        s = (q * k).reshape(B, self.n_head, self.dk_per_head, H, W).sum(2) / self.temper
        sp, vp = F.pad(s, (1, 1, 1, 1)), F.pad(v, (1, 1, 1, 1))
        taps = [(i, j) for i in range(3) for j in range(3)]
        att = torch.softmax(torch.stack([sp[:, :, i:i + H, j:j + W] for i, j in taps], 2), 2)   # [B, n_head, 9, H, W]
        out = None
        for n, (i, j) in enumerate(taps):
            term = att[:, :, n, None] * vp[:, :, i:i + H, j:j + W].reshape(B, self.n_head, self.dv_per_head, H, W)
            out = term if out is None else out + term
        return out.reshape(B, -1, H, W), att.reshape(B * self.n_head, 9, H, W)


class SEBlock(nn.Module):
    def __init__(self, ch, ratio=16):
        super().__init__()
        self.linear1 = nn.Linear(ch, ch // ratio)
        self.linear2 = nn.Linear(ch // ratio, ch)

    def gate(self, x):
        return self.gate_from_mean(x.mean(dim=(2, 3)))

    def gate_from_mean(self, s):
        s = s.to(self.linear1.weight.dtype)
        return torch.sigmoid(F.relu(self.linear2(F.relu(self.linear1(s)))))

    def forward(self, x):
        return x * self.gate(x)[:, :, None, None]


class ResNet(nn.Module):
    def __init__(self, num_channels, num_chunks, module_name, inorm=False, initial_projection=False,
                 extra_blocks=False, dilation_cycle=(1, 2, 4, 8)):
        super().__init__()
        self.module_name, self.inorm = module_name, inorm
        self.initial_projection = initial_projection
        self.ops = None  # HeadNormOps: fused norm/ELU and SE/residual passes on HIP
        self.cops = None  # HeadConvOps: the convolutions on HIP, norm + ELU fused into their loads
        C = num_channels
        self.blocks = []
        if initial_projection:
            self.add_module(f"resnet_{module_name}_init_proj", nn.Conv2d(C, C, 1))
        names = [(f"{i}_{d}", d) for i in range(num_chunks) for d in dilation_cycle]
        if extra_blocks:
            names += [("extra0", 1), ("extra1", 1)]
        for b, d in names:
            r = f"resnet_{module_name}_{b}"
            if inorm:
                self.add_module(f"{r}_inorm_1", nn.InstanceNorm2d(C, eps=1e-06, affine=True))
                self.add_module(f"{r}_inorm_2", nn.InstanceNorm2d(C // 2, eps=1e-06, affine=True))
                self.add_module(f"{r}_inorm_3", nn.InstanceNorm2d(C // 2, eps=1e-06, affine=True))
            self.add_module(f"{r}_conv2d_1", nn.Conv2d(C, C // 2, 1))
            self.add_module(f"{r}_conv2d_2", nn.Conv2d(C // 2, C // 2, 3, dilation=d, padding=d))
            self.add_module(f"{r}_conv2d_3", nn.Conv2d(C // 2, C, 1))
            self.add_module(f"{r}_se_block", SEBlock(C, 16))
            self.blocks.append(r)

    def forward(self, x):
        m = self._modules
        if self.cops is not None:
            if self.ops is None:
                raise RuntimeError("the HIP convolutions need the HIP norm passes (use_hip_norm_ops) too")
            return self._forward_hipconv(x, self.ops, self.cops)
        if self.initial_projection:
            x = m[f"resnet_{self.module_name}_init_proj"](x)
        ops = self.ops
        if ops is not None:
            return self._forward_hip(x, ops)
        for r in self.blocks:
            res = x
            for i in (1, 2, 3):
                if self.inorm:
                    x = m[f"{r}_inorm_{i}"](x)
                x = m[f"{r}_conv2d_{i}"](F.elu(x))
            x = m[f"{r}_se_block"](x) + res
        return x

    def _forward_hip(self, x, ops):
        """Same blocks with the norm / bias / SE passes on HIP (HeadNormOps). A conv that feeds an
        InstanceNorm runs without its bias (a per-channel constant cancels in the normalisation);
        the last conv's bias is applied inside the SE gate + residual pass, and the SE squeeze
        (channel mean) adds it analytically."""
        m = self._modules
        for r in self.blocks:
            res = x
            for i in (1, 2, 3):
                conv = m[f"{r}_conv2d_{i}"]
                if self.inorm:
                    x = ops.inorm_elu(x, m[f"{r}_inorm_{i}"], out=None if i == 1 else x)
                else:
                    x = F.elu(x)
                keep_bias = not self.inorm and i < 3
                x = F.conv2d(x, conv.weight, conv.bias if keep_bias else None, conv.stride, conv.padding,
                             conv.dilation)
            conv3, se = m[f"{r}_conv2d_3"], m[f"{r}_se_block"]
            gate = se.gate_from_mean(ops.channel_mean(x, conv3.bias))
            x = ops.se_scale_add(x, gate, res, out=x, bias=conv3.bias)
        return x


    def _forward_hipconv(self, x, ops, cops, in_elu=False):
        """The blocks with their convolutions on HIP too (HeadConvOps). An InstanceNorm + ELU in
        front of a convolution never makes a pass of its own: the statistics of the convolution's
        input -- left by the convolution that produced it, or one read pass over the residual
        stream for inorm_1 -- are folded to a per-channel scale / shift that the convolution applies
        as it loads. Biases as in _forward_hip. in_elu: the caller's F.elu in front of this ResNet,
        applied by init_proj's load."""
        m = self._modules
        if self.initial_projection:
            proj = m[f"resnet_{self.module_name}_init_proj"]
            x = cops.conv(x, proj.weight, bias=ops.f32(proj.bias), in_elu=in_elu)
        elif in_elu:
            x = F.elu(x)
        _, C, H, W = x.shape
        hw = H * W
        for r in self.blocks:
            res = x
            st = cops.plane_stats(x) if self.inorm else None
            for i in (1, 2, 3):
                conv = m[f"{r}_conv2d_{i}"]
                if self.inorm:
                    norm = m[f"{r}_inorm_{i}"]
                    sc, sh = cops.fold(st, x.shape[1], hw, ops.f32(norm.weight), ops.f32(norm.bias), norm.eps)
                    x, st = cops.conv(x, conv.weight, in_scale=sc, in_shift=sh, in_elu=True,
                                      dilation=conv.dilation[0], stats=True)
                elif i < 3:
                    x = cops.conv(x, conv.weight, bias=ops.f32(conv.bias), in_elu=True, dilation=conv.dilation[0])
                else:
                    x, st = cops.conv(x, conv.weight, in_elu=True, stats=True)
            conv3, se = m[f"{r}_conv2d_3"], m[f"{r}_se_block"]
            (mean,) = cops.fold(st, C, hw, bias=ops.f32(conv3.bias), want=("mean",))
            gate = se.gate_from_mean(mean[None])
            x = ops.se_scale_add(x, gate, res, out=x, bias=conv3.bias)
        return x


    def _forward_hipconv_batch(self, hb, x, spare, ops, cops, in_elu=False):
        """_forward_hipconv for every image of a HeadBatch at once: each pass is one launch over the
        packed buffers, the SE gate one di_se_gate launch in fp32 (the single path's gate goes through
        torch's linears in the head's dtype). The buffers are bf16 or fp32, as the batch is. x: the packed residual stream; spare: the other 128-channel buffer.
        Returns (the buffer holding the result, the free one)."""
        m = self._modules
        C = hb.CHANNELS
        h1, h2 = hb.half
        rows = dict(scale=hb.rows[0], shift=hb.rows[1], mean=hb.rows[2])
        gate = hb.rows[3]
        if self.initial_projection:
            proj = m[f"resnet_{self.module_name}_init_proj"]
            cops.conv_batch(hb, x, proj.weight, y=spare, bias=ops.f32(proj.bias), in_elu=in_elu)
            x, spare = spare, x
        elif in_elu:
            raise NotImplementedError("a batched ResNet applies the caller's ELU in its initial projection")
        for r in self.blocks:
            st = cops.plane_stats_batch(hb, x, C) if self.inorm else None
            t = x
            for i, y in ((1, h1), (2, h2), (3, spare)):
                conv = m[f"{r}_conv2d_{i}"]
                cin = conv.weight.shape[1]
                if self.inorm:
                    norm = m[f"{r}_inorm_{i}"]
                    # [count, cin] rows: contiguous views of the batch's [count, C] storage
                    out = {k: rows[k].view(-1)[:hb.count * cin].view(hb.count, cin) for k in ("scale", "shift")}
                    sc, sh = cops.fold_batch(hb, st, cin, ops.f32(norm.weight), ops.f32(norm.bias), norm.eps, out=out)
                    _, st = cops.conv_batch(hb, t, conv.weight, y=y, in_scale=sc, in_shift=sh, in_elu=True,
                                            dilation=conv.dilation[0], stats=True)
                elif i < 3:
                    cops.conv_batch(hb, t, conv.weight, y=y, bias=ops.f32(conv.bias), in_elu=True,
                                    dilation=conv.dilation[0])
                else:
                    _, st = cops.conv_batch(hb, t, conv.weight, y=y, in_elu=True, stats=True)
                t = y
            conv3, se = m[f"{r}_conv2d_3"], m[f"{r}_se_block"]
            (mean,) = cops.fold_batch(hb, st, C, bias=ops.f32(conv3.bias), want=("mean",), out=rows)
            ops.se_gate(se, mean, out=gate)
            ops.se_scale_add_batch(hb, spare, gate, x, out=spare, bias=conv3.bias)
            x, spare = spare, x
        return x, spare


class ResNet2DInputWithOptAttention(nn.Module):
    def __init__(self, num_chunks=14, init_channels=256, num_channels=128, num_classes=2, use_attention=False,
                 n_head=4):
        super().__init__()
        if use_attention and n_head != 4:
            raise NotImplementedError("the head's regional attention is specialised for 4 heads")
        self.use_attention = bool(use_attention)
        self.conv2d_1 = nn.Conv2d(init_channels, num_channels, 1)
        self.inorm_1 = nn.InstanceNorm2d(num_channels, eps=1e-06, affine=True)
        self.base_resnet = ResNet(num_channels, num_chunks, "base_resnet", inorm=True, initial_projection=True)
        self.phase2_resnet = ResNet(num_channels, 1, "bin_resnet", inorm=False, initial_projection=True,
                                    extra_blocks=True)
        self.phase2_conv = nn.Conv2d(num_channels, num_classes, 1)
        if self.use_attention:   # registered last, as the reference does (:1206-1216)
            self.MHA2D_1 = MultiHeadRegionalAttention(num_channels, d_v=num_channels, n_head=n_head)
            self.MHA2D_2 = MultiHeadRegionalAttention(num_channels, d_v=num_channels, n_head=n_head)
        self.ops = None
        self.cops = None
        self.aops = None  # HeadAttnOps: the regional attention on HIP, in place with the HIP norm passes

    def use_hip_norm_ops(self, ops):
        """Route the InstanceNorm+ELU and SE+residual passes through HeadNormOps (or None: torch)."""
        self.ops = self.base_resnet.ops = self.phase2_resnet.ops = ops
        self.aops = HeadAttnOps(ops.device) if ops is not None and self.use_attention else None
        return self

    def use_hip_convs(self, cops):
        """Route the ResNets' convolutions through HeadConvOps (or None: torch / MIOpen). A bf16 or an
        fp32 NCHW head, with the HIP norm passes (use_hip_norm_ops) in place. conv2d_1 and phase2_conv
        stay on torch."""
        self.cops = self.base_resnet.cops = self.phase2_resnet.cops = cops
        return self

    def forward(self, t):
        x = self.conv2d_1(t)
        if getattr(self, "ops", None) is not None:
            return self.body(self.ops.inorm_elu(x, self.inorm_1, out=x))
        return self.body(F.elu(self.inorm_1(x)))

    def body(self, x):
        """Everything after the prologue ELU(inorm_1(conv2d_1(t))) (which HeadPrologueOp fuses
        with the pair tensor on HIP)."""
        if getattr(self, "cops", None) is not None:
            if self.ops is None:
                raise RuntimeError("the HIP convolutions need the HIP norm passes (use_hip_norm_ops) too")
            x = self.base_resnet._forward_hipconv(x, self.ops, self.cops)
            if self.use_attention:
                x = self._attention_hipconv(self.MHA2D_1, x)
            x = self.phase2_resnet._forward_hipconv(x, self.ops, self.cops, in_elu=True)
            if self.use_attention:
                x = self._attention_hipconv(self.MHA2D_2, x)
            return self.phase2_conv(F.elu(x))
        x = F.elu(self.base_resnet(x))
        if self.use_attention:
            x = F.elu(self._attention(self.MHA2D_1, x))
        x = F.elu(self.phase2_resnet(x))
        if self.use_attention:
            x = F.elu(self._attention(self.MHA2D_2, x))
        return self.phase2_conv(x)

    def _qk(self, mha):
        """The block's q / k weights as HeadAttnOps takes them: fp32 [16, 128] (cached copies for a bf16 head)."""
        return (self.ops.f32(mha.q_layer.weight).view(HeadAttnOps.DK, -1),
                self.ops.f32(mha.k_layer.weight).view(HeadAttnOps.DK, -1))

    def _attention(self, mha, x):
        """mha(x)[0] with torch convolutions: scores and mix on HIP (the value convolution on torch) where the
        HIP norm passes are in place and x is one NCHW image on the GPU; the module's torch path otherwise
        (the CPU, head_hip_ops=False, a channels-last head)."""
        aops = getattr(self, "aops", None)
        if aops is None or not x.is_cuda or not x.is_contiguous() or x.shape[0] != 1 \
                or x.shape[1] != HeadAttnOps.CHANNELS:
            return mha(x)[0]
        s = aops.scores(x, *self._qk(mha))
        v = mha.v_layer(x)
        if not v.is_contiguous():
            v = v.contiguous()
        return aops.mix(v, s, out=x)   # x is this forward's own ELU output: overwritten

    def _attention_hipconv(self, mha, x):
        """The same behind a ResNet whose stored output is pre-ELU (HIP convolutions): the ELU is applied
        as the scores and the value convolution load x; the result, pre-ELU again, overwrites x."""
        if self.aops is None:
            raise RuntimeError("the regional attention behind the HIP convolutions needs the HIP norm passes")
        s = self.aops.scores(x, *self._qk(mha), in_elu=True)
        v = self.cops.conv(x, mha.v_layer.weight, in_elu=True)
        return self.aops.mix(v, s, out=x)

    def _attention_batch(self, mha, hb, x, spare):
        """_attention_hipconv for every image of a HeadBatch, inside its arena: the scores in the front of
        hb.half[0] (fp32), the values in the spare wide buffer, the result back over x."""
        s = self.aops.scores_batch(hb, x, *self._qk(mha), in_elu=True)
        self.cops.conv_batch(hb, x, mha.v_layer.weight, y=spare, in_elu=True)
        self.aops.mix_batch(hb, spare, s, x)
        return x, spare


    def plan(self, check="all"):
        """This head's HeadBodyPlan, rebuilt when a parameter it points into was replaced or written
        (HeadBodyPlan.stale; check="head": only those the first launches read)."""
        plan = getattr(self, "_plan", None)
        if plan is None or plan.ops is not self.ops or plan.stale(check):
            plan = self._plan = HeadBodyPlan(self, self.ops)
        return plan

    def body_batch(self, xs, native=False):
        """body for several images in one launch sequence (HIP convolutions; a bf16 or an fp32 head): xs is a list of
        [1, 128, h, w] prologue outputs, or a HeadBatch whose ``input(i)`` views hold them. Returns
        the list of logits. Each image's logits are the same bits whatever else the batch holds.
        native: the same launches issued from C (di_head_body_batch, called on the plan's two parts) and
        phase2_conv(ELU(x)) of all images by one HIP launch (di_head_logits_batch) instead of two torch
        kernels per image; the logits are views of one packed buffer; bf16 only. With the regional attention
        (use_attention) only native=False: its two blocks run inside the arena (_attention_batch)."""
        if native and self.use_attention:
            raise RuntimeError("body_batch(native=True) does not run the regional attention: di_head_body_batch "
                               "has no attention stage (use native=False)")
        if getattr(self, "cops", None) is None or self.ops is None:
            raise RuntimeError("body_batch needs the HIP convolutions and norm passes (use_hip_convs, "
                               "use_hip_norm_ops)")
        dtype = self.phase2_conv.weight.dtype
        if isinstance(xs, HeadBatch):
            hb = xs
        else:
            hb = HeadBatch([x.shape[2:] for x in xs], xs[0].device, dtype=dtype)
            for i, x in enumerate(xs):
                hb.input(i).copy_(x)
        if hb.dtype != dtype:
            raise ValueError(f"a {dtype} head takes a HeadBatch of that dtype, got {hb.dtype}")
        if native and dtype != torch.bfloat16:
            raise RuntimeError("body_batch(native=True) is bf16 only (di_head_body_batch, di_head_logits_batch); "
                               "an fp32 head runs native=False")
        if native:
            # the staleness check reads ~850 parameters' pointers and versions (~0.25 ms): only those of the
            # first launches are checked before anything runs, the rest while the GPU works on these
            plan = self.plan(check="head")
            which = plan.body(hb, part=0)
            plan = self.plan()
            return plan.logits(hb, hb.wide[plan.body(hb, part=1, start=which)])
        x, spare = self.base_resnet._forward_hipconv_batch(hb, hb.wide[0], hb.wide[1], self.ops, self.cops)
        if self.use_attention:
            x, spare = self._attention_batch(self.MHA2D_1, hb, x, spare)
        x, spare = self.phase2_resnet._forward_hipconv_batch(hb, x, spare, self.ops, self.cops, in_elu=True)
        if self.use_attention:
            x, spare = self._attention_batch(self.MHA2D_2, hb, x, spare)
        return [self.phase2_conv(F.elu(hb.view(x, hb.CHANNELS, i))) for i in range(hb.count)]


class HeadBodyPlan:
    """The head's body as di_head_body_batch takes it (include/deepinteract_amd.h): one di_head_net per
    ResNet with its host array of di_head_block, every pointer into the module's own bf16 tensors or into
    HeadNormOps.f32's cached fp32 copies, plus phase2_conv as di_head_logits_batch's fp32 [2, 128] rows.
    Built once from a ResNet2DInputWithOptAttention and rebuilt by ``ResNet2DInputWithOptAttention.plan()``
    when ``stale()``: a parameter's storage or ``_version`` changed (a reload, a dtype or device move).
    ``nets`` is the table a C caller would pass; ``parts`` cuts the same blocks after the first HEAD of
    them, so that a forward can start on part 0 and check the other parameters meanwhile.
    No GPU is needed to build one (``ops`` None: the fp32 copies are made here); running it needs the
    bf16 head on the GPU."""

    HEAD = 3   # blocks of part 0: ~30 launches, what the full check's ~0.25 ms hide behind

    def __init__(self, head, ops=None):
        from . import _lib
        self._lib, self.ops = _lib, ops
        f32 = ops.f32 if ops is not None else (lambda p: None if p is None else p.detach().float().contiguous())
        self._params, self._keep, self._weights = [], [], []
        self.blocks, self.dilations = [], []
        nets, parts = [], []
        for net, in_elu in ((head.base_resnet, False), (head.phase2_resnet, True)):
            m = net._modules
            proj = m[f"resnet_{net.module_name}_init_proj"] if net.initial_projection else None
            if in_elu and proj is None:
                raise NotImplementedError("a batched ResNet applies the caller's ELU in its initial projection")
            pw = self._own(proj.weight) if proj is not None else None
            pb = self._vec(proj.bias, f32) if proj is not None else None
            arr = (_lib.DiHeadBlock * len(net.blocks))()
            for at, (blk, r) in enumerate(zip(arr, net.blocks)):
                if not nets and at == self.HEAD:
                    self._n_head = len(self._params)
                convs = [m[f"{r}_conv2d_{i}"] for i in (1, 2, 3)]
                se = m[f"{r}_se_block"]
                C = convs[0].weight.shape[1]
                hidden = se.linear1.weight.shape[0]
                want = [(C // 2, C, 1, 1), (C // 2, C // 2, 3, 3), (C, C // 2, 1, 1)]
                if C != HeadBatch.CHANNELS or hidden != 8 or [tuple(c.weight.shape) for c in convs] != want:
                    raise ValueError(f"{r}: di_head_body_batch runs 128-channel bottleneck blocks with an 8-unit SE")
                blk.w1, blk.w2, blk.w3 = (self._own(c.weight) for c in convs)
                if net.inorm:
                    norms = [m[f"{r}_inorm_{i}"] for i in (1, 2, 3)]
                    if len({n.eps for n in norms}) != 1:
                        raise ValueError(f"{r}: one eps per block")
                    blk.eps = norms[0].eps
                    for i, n in enumerate(norms, 1):
                        setattr(blk, f"gamma{i}", self._vec(n.weight, f32))
                        setattr(blk, f"beta{i}", self._vec(n.bias, f32))
                else:
                    blk.eps = 0.0
                    blk.bias1, blk.bias2 = self._vec(convs[0].bias, f32), self._vec(convs[1].bias, f32)
                blk.bias3 = self._vec(convs[2].bias, f32)
                blk.se_w1, blk.se_b1, blk.se_w2, blk.se_b2 = (self._vec(p, f32) for p in (
                    se.linear1.weight, se.linear1.bias, se.linear2.weight, se.linear2.bias))
                blk.dilation = convs[1].dilation[0]
                self.dilations.append(blk.dilation)
            self.blocks.append(arr)
            if not nets and len(arr) > self.HEAD:   # the first net in two parts: [0, HEAD) and the rest
                rest = ctypes.cast(ctypes.byref(arr, self.HEAD * ctypes.sizeof(_lib.DiHeadBlock)),
                                   ctypes.POINTER(_lib.DiHeadBlock))
                parts += [_lib.DiHeadNet(pw, pb, arr, self.HEAD, int(in_elu)),
                          _lib.DiHeadNet(None, None, rest, len(arr) - self.HEAD, 0)]
            else:
                if not nets:
                    self._n_head = len(self._params)
                parts.append(_lib.DiHeadNet(pw, pb, arr, len(arr), int(in_elu)))
            nets.append(_lib.DiHeadNet(pw, pb, arr, len(arr), int(in_elu)))
        self.nets = (_lib.DiHeadNet * len(nets))(*nets)
        self.parts = ((_lib.DiHeadNet * 1)(parts[0]), (_lib.DiHeadNet * (len(parts) - 1))(*parts[1:]))
        p2 = head.phase2_conv
        if tuple(p2.weight.shape) != (2, HeadBatch.CHANNELS, 1, 1):
            raise ValueError("di_head_logits_batch computes 2 classes from 128 channels")
        self.logit_w, self.logit_b = self._vec(p2.weight, f32), self._vec(p2.bias, f32)
        self.num_blocks = len(self.dilations)
        w = self._weights
        self.device = w[0].device
        self.runnable = all(t.dtype == torch.bfloat16 and t.is_contiguous() and t.device == self.device for t in w)
        self._sig = self._signature(len(self._params))

    def __deepcopy__(self, memo):
        return None   # raw pointers: a copied or unpickled module builds its own plan

    def __reduce__(self):
        return (type(None), ())

    def _own(self, p):
        """A pointer into the module's own tensor."""
        self._params.append(p)
        self._weights.append(p)
        return p.data_ptr()

    def _vec(self, p, f32):
        """A pointer to the fp32 copy of a parameter (None: NULL)."""
        if p is None:
            return None
        self._params.append(p)
        t = f32(p)
        self._keep.append(t)
        return t.data_ptr()

    def _signature(self, n):
        ps = self._params[:n]
        return [p.data_ptr() for p in ps], [p._version for p in ps]

    def stale(self, check="all"):
        """Whether a parameter the tables point into (check="head": into part 0's) has another storage
        or version than when the plan was built."""
        n = self._n_head if check == "head" else len(self._params)
        ptrs, versions = self._signature(n)
        return ptrs != self._sig[0][:n] or versions != self._sig[1][:n]

    def arena(self, hb, start=0):
        """The batch's buffers, with hb.wide[start] as the input."""
        return self._lib.DiHeadArena(hb.wide[start].data_ptr(), hb.wide[start ^ 1].data_ptr(), hb.half[0].data_ptr(),
                                     hb.half[1].data_ptr(), hb.stats.data_ptr(), hb.rows.data_ptr(),
                                     ctypes.addressof(hb.items), hb.items_ptr.value, hb.count)

    def body(self, hb, part=None, start=0):
        """di_head_body_batch over a HeadBatch whose wide[start] holds the input -- the whole body, or
        part 0 / part 1 of it: the index of the hb.wide buffer holding the result."""
        _lib = self._lib
        if not self.runnable or hb.device != self.device:
            raise ValueError("di_head_body_batch takes the modules' contiguous bf16 weights on the batch's device")
        nets = self.nets if part is None else self.parts[part]
        arena, which = self.arena(hb, start), ctypes.c_int32(-1)
        _lib.check(_lib.load().di_head_body_batch(_lib.DI_BF16, nets, len(nets), ctypes.byref(arena),
                                                  ctypes.byref(which), _stream()), "di_head_body_batch")
        return start ^ which.value

    def logits(self, hb, x):
        """phase2_conv(ELU(x)) of a packed 128-channel buffer (di_head_logits_batch): the [1, 2, h, w]
        views of one new packed bf16 buffer."""
        _lib = self._lib
        hb.check_packed(x, hb.CHANNELS)
        y = torch.empty(2 * hb.pixels, dtype=torch.bfloat16, device=hb.device)
        _lib.check(_lib.load().di_head_logits_batch(_lib.DI_BF16, _ptr(x), self.logit_w, self.logit_b, hb.items,
                                                    hb.items_ptr, hb.count, _ptr(y), _stream()),
                   "di_head_logits_batch")
        return [hb.view(y, 2, i) for i in range(hb.count)]

    def run(self, hb):
        """The body, then the logits: two C calls and one allocation, whatever the batch holds."""
        return self.logits(hb, hb.wide[self.body(hb)])


def contact_probs(logits):
    """lit_model_predict.py:236-239: softmax over classes, positive class, [L1, L2]."""
    return torch.softmax(logits.squeeze(0), dim=0)[1]
