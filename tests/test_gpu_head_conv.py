"""GPU tests of the head convolutions (csrc/head_conv.hip, head.HeadConvOps): di_head_conv,
di_plane_stats and di_head_norm_fold, then the whole head and the model with ``head_convs="hip"``.

Exact cases: inputs and weights are integers in [-4, 4] stored as bf16, so every product and every
partial sum is an integer of magnitude <= 16 K <= 9216 < 2^24, exact in fp32 in any order, and the only
rounding is the bf16 store: the output must equal torch's GEMM convolution (fp32, MIOpen's fast
algorithms off) rounded to bf16, bit for bit. The stored values are integers too, so their fp64 sums
are exact in any order, and a thread's fp32 sum of 4 squares is exact while |y| < 2048 (4 * 2^22 =
2^24; the tests assert it): the statistics partials must add up to the fp64 sums of the stored y
exactly.

Transform cases: against ref = conv(ELU(x s + b), w) in fp64 on the unrounded transform, with
S the same convolution of absolute values: |y - ref| <= 2^-8 |ref| + (2^-8 + K 2^-24) S (one bf16
rounding of each input -- the weights are bf16 already --, fp32 accumulation of K terms, one output
rounding). A transform applied to the padding, a missing ELU or swapped scale / shift is O(S).

Fold cases: 1e-6 relative (+1e-7) against fp64, the bound of test_gpu_head_ops.test_channel_mean.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_common import chain_item, load_case, rel_max

pytestmark = pytest.mark.gpu

SHAPES_3 = [(1, 1), (3, 5), (17, 9), (33, 70), (64, 64), (145, 145), (70, 257)]
SHAPES_1 = [(3, 5), (33, 70), (145, 145)]
CH_1 = [(128, 64), (64, 128), (128, 128), (256, 128)]


@pytest.fixture(scope="module")
def cops():
    from deepinteract_amd.head import HeadConvOps
    return HeadConvOps("cuda")


def _ints(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, shape, generator=g).to(torch.bfloat16).cuda()


def _x(C, H, W, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    # per-channel offsets and scales so the statistics are non-trivial (as test_gpu_head_ops._x)
    x = torch.randn(1, C, H, W, generator=g) * (0.5 + torch.rand(C, generator=g))[None, :, None, None] \
        + 3 * torch.randn(C, generator=g)[None, :, None, None]
    return x.cuda().to(dtype)


def _ref_f32(x, w, d, bias=None):
    with torch.backends.cudnn.flags(enabled=False):
        return F.conv2d(x.float(), w.float(), bias, padding=d if w.shape[-1] == 3 else 0, dilation=d)


def _conv64(a, w, d):
    """fp64 convolution as the sum of the taps' shifted 1x1 products (zero padding = d for 3x3)."""
    k = w.shape[-1]
    _, _, H, W = a.shape
    if k == 1:
        return torch.einsum("oc,bchw->bohw", w[:, :, 0, 0], a)
    ap = F.pad(a, (d, d, d, d))
    out = torch.zeros(1, w.shape[0], H, W, dtype=torch.float64, device=a.device)
    for ty in range(3):
        for tx in range(3):
            out += torch.einsum("oc,bchw->bohw", w[:, :, ty, tx], ap[:, :, ty * d:ty * d + H, tx * d:tx * d + W])
    return out


def _partials(st, C):
    """(sum y, sum y^2) per channel from a statistics buffer, added in fp64 on the host side."""
    n = int(st[:1].view(torch.int64).item())
    p = st[2:2 + C * n * 2].view(C, n, 2)
    return p[:, :, 0].sum(dim=1), p[:, :, 1].sum(dim=1)


def _check_exact(cops, cin, cout, k, d, H, W, bias=False, seed=0):
    x = _ints((1, cin, H, W), 100 + seed)
    w = _ints((cout, cin, k, k), 200 + seed)
    b = _ints((cout,), 300 + seed).float() if bias else None
    ref = _ref_f32(x, w, d, b)
    y, st = cops.conv(x, w, bias=b, dilation=d, stats=True)
    assert y.shape == ref.shape and y.dtype == torch.bfloat16
    assert torch.equal(y, ref.to(torch.bfloat16)), f"max |diff| {float((y.float() - ref).abs().max())}"
    assert float(y.float().abs().max()) < 2048  # the exactness argument for the fp32 sums of 4 squares
    s, ss = _partials(st, cout)
    yd = y.double()
    assert torch.equal(s, yd.sum(dim=(0, 2, 3))) and torch.equal(ss, (yd * yd).sum(dim=(0, 2, 3)))
    # ... and the folded mean is their one correctly rounded quotient
    (mean,) = cops.fold(st, cout, H * W, want=("mean",))
    assert torch.equal(mean, (yd.sum(dim=(0, 2, 3)) / (H * W)).float())


@pytest.mark.parametrize("shape", SHAPES_3, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("d", [1, 2, 4, 8])
def test_exact_3x3(cops, shape, d):
    _check_exact(cops, 64, 64, 3, d, *shape, seed=d)


@pytest.mark.parametrize("shape", SHAPES_1, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("ch", CH_1, ids=lambda c: f"{c[0]}to{c[1]}")
def test_exact_1x1(cops, ch, shape):
    _check_exact(cops, ch[0], ch[1], 1, 1, *shape)


@pytest.mark.parametrize("cin,cout,k,d,shape", [(64, 64, 3, 2, (33, 70)), (64, 64, 3, 8, (17, 9)),
                                                (128, 128, 1, 1, (33, 70)), (128, 64, 1, 1, (145, 145))])
def test_exact_with_integer_bias(cops, cin, cout, k, d, shape):
    _check_exact(cops, cin, cout, k, d, *shape, bias=True, seed=7)


def test_other_supported_shapes_exact(cops):
    """Shapes the head does not use but the entry point accepts: 3x3 with 128 / 256 input channels
    and 128 output channels, and the odd dilations (each LDS-size instantiation's largest)."""
    _check_exact(cops, 128, 128, 3, 3, 21, 37, seed=11)
    _check_exact(cops, 256, 64, 3, 5, 19, 18, seed=12)
    _check_exact(cops, 64, 128, 3, 7, 40, 23, seed=13)
    _check_exact(cops, 64, 64, 3, 6, 16, 16, seed=14)


def _band_ref(x, w, d, rows):
    """Reference for the first and last `rows` output rows from cropped bands: d extra rows towards
    the image's inside, padding only at the true image edge (the conv's own padding on the cropped
    side lands in rows that are dropped)."""
    H = x.shape[2]
    e = d if w.shape[-1] == 3 else 0
    top = _ref_f32(x[:, :, :rows + e], w, d)[:, :, :rows]
    bot = _ref_f32(x[:, :, H - rows - e:], w, d)[:, :, -rows:]
    return top, bot


@pytest.mark.parametrize("cin,cout,k,d,L", [(128, 64, 1, 1, 2900), (64, 64, 3, 8, 4100)],
                         ids=["1x1_2900", "3x3_d8_4100"])
def test_exact_past_2gb(cops, cin, cout, k, d, L):
    """Plane offsets past 2^31 bytes: a 2.15-GB input; the first and last 24 rows, exact."""
    g = torch.Generator(device="cuda").manual_seed(L)
    x = torch.randint(-4, 5, (1, cin, L, L), generator=g, device="cuda", dtype=torch.int8).to(torch.bfloat16)
    assert x.numel() * 2 > 2 ** 31
    w = _ints((cout, cin, k, k), 400 + L)
    y, st = cops.conv(x, w, dilation=d, stats=True)
    top, bot = _band_ref(x, w, d, 24)
    assert torch.equal(y[:, :, :24], top.to(torch.bfloat16))
    assert torch.equal(y[:, :, -24:], bot.to(torch.bfloat16))
    assert float(y[:, :, -24:].float().abs().max()) > 0
    s, _ = _partials(st, cout)
    assert torch.equal(s, y.sum(dim=(0, 2, 3), dtype=torch.float64))


TRANSFORM_CASES = [(64, 64, 3, 2, (33, 70)), (64, 64, 3, 8, (33, 70)), (128, 64, 1, 1, (145, 145))]


def _transform_inputs(cin, cout, k, shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = _x(cin, *shape, seed, torch.bfloat16)
    w = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).to(torch.bfloat16).cuda()
    s = (1 + 0.3 * torch.randn(cin, generator=g)).cuda()
    b = (0.3 * torch.randn(cin, generator=g)).cuda()
    return x, w, s, b


@pytest.mark.parametrize("cin,cout,k,d,shape", TRANSFORM_CASES)
def test_transform(cops, cin, cout, k, d, shape):
    x, w, s, b = _transform_inputs(cin, cout, k, shape, 21)
    y = cops.conv(x, w, in_scale=s, in_shift=b, in_elu=True, dilation=d).double()
    a = F.elu(x.double() * s.double()[None, :, None, None] + b.double()[None, :, None, None])
    ref = _conv64(a, w.double(), d)
    S = _conv64(a.abs(), w.double().abs(), d)
    K = cin * k * k
    bound = 2.0 ** -8 * ref.abs() + (2.0 ** -8 + K * 2.0 ** -24) * S
    ratio = float(((y - ref).abs() / bound).max())
    print(f"transform {cin}->{cout} k{k} d{d} {shape}: max |y - ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    # the affine form without ELU, and scale / shift each alone (NULL means 1 / 0)
    for kw, fn in ((dict(in_scale=s, in_shift=b), lambda v: v * s.double()[None, :, None, None]
                    + b.double()[None, :, None, None]),
                   (dict(in_scale=s), lambda v: v * s.double()[None, :, None, None]),
                   (dict(in_shift=b, in_elu=True), lambda v: F.elu(v + b.double()[None, :, None, None]))):
        a2 = fn(x.double())
        r2, S2 = _conv64(a2, w.double(), d), _conv64(a2.abs(), w.double().abs(), d)
        y2 = cops.conv(x, w, dilation=d, **kw).double()
        assert bool(((y2 - r2).abs() <= 2.0 ** -8 * r2.abs() + (2.0 ** -8 + K * 2.0 ** -24) * S2).all()), kw


def _fold64(x, gamma, beta, eps, bias):
    xd = x.double()
    m = xd.mean(dim=(0, 2, 3))
    var = (xd * xd).mean(dim=(0, 2, 3)) - m * m
    sc = gamma.double() / torch.sqrt(var + eps)
    return sc, beta.double() - m * sc, m + bias.double()


def _close(a, ref):
    return float((a.double() - ref).abs().max()) < 1e-6 * float(ref.abs().max()) + 1e-7


@pytest.mark.parametrize("shape", [(7, 3, 3), (64, 145, 145), (128, 64, 64)])
def test_plane_stats_and_fold(cops, shape):
    C, H, W = shape
    x = _x(C, H, W, 9, torch.bfloat16)
    g = torch.Generator().manual_seed(10)
    gamma, beta, bias = ((1 + 0.3 * torch.randn(C, generator=g)).cuda(), (0.3 * torch.randn(C, generator=g)).cuda(),
                         torch.randn(C, generator=g).cuda())
    st = cops.plane_stats(x)
    sc, sh, mean = cops.fold(st, C, H * W, gamma, beta, 1e-6, bias, want=("scale", "shift", "mean"))
    rsc, rsh, rmean = _fold64(x, gamma, beta, 1e-6, bias)
    assert _close(sc, rsc) and _close(sh, rsh) and _close(mean, rmean)
    # NULL gamma / beta / bias mean 1 / 0 / 0; outputs may be left out
    (sc1,) = cops.fold(st, C, H * W, eps=1e-6, want=("scale",))
    one, zero = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    assert _close(sc1, _fold64(x, one, zero, 1e-6, zero)[0])


@pytest.mark.parametrize("cin,cout,k,d,shape", TRANSFORM_CASES)
def test_conv_stats_match_plane_stats(cops, cin, cout, k, d, shape):
    x, w, s, b = _transform_inputs(cin, cout, k, shape, 31)
    g = torch.Generator().manual_seed(32)
    gamma, beta, bias = ((1 + 0.3 * torch.randn(cout, generator=g)).cuda(),
                         (0.3 * torch.randn(cout, generator=g)).cuda(), torch.randn(cout, generator=g).cuda())
    hw = shape[0] * shape[1]
    y, st = cops.conv(x, w, in_scale=s, in_shift=b, in_elu=True, dilation=d, stats=True)
    own = cops.fold(st, cout, hw, gamma, beta, 1e-6, bias, want=("scale", "shift", "mean"))
    own = [t.clone() for t in own]
    plane = cops.fold(cops.plane_stats(y), cout, hw, gamma, beta, 1e-6, bias, want=("scale", "shift", "mean"))
    ref = _fold64(y, gamma, beta, 1e-6, bias)
    for a, p, r in zip(own, plane, ref):
        assert _close(a, r) and _close(p, r) and _close(a, p.double())


@pytest.mark.parametrize("cin,cout,k,d,shape", TRANSFORM_CASES + [(256, 128, 1, 1, (70, 257))])
def test_deterministic(cops, cin, cout, k, d, shape):
    x, w, s, b = _transform_inputs(cin, cout, k, shape, 41)
    hw = shape[0] * shape[1]
    outs = []
    for _ in range(2):
        y, st = cops.conv(x, w, in_scale=s, in_shift=b, in_elu=True, dilation=d, stats=True)
        f = cops.fold(st, cout, hw, eps=1e-6, want=("scale", "shift", "mean"))
        outs.append((y.clone(), st[:2 + cout * int(st[:1].view(torch.int64).item()) * 2].clone(),
                     [t.clone() for t in f]))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1].view(torch.int64), outs[1][1].view(torch.int64))
    for a, c in zip(outs[0][2], outs[1][2]):
        assert torch.equal(a.view(torch.int32), c.view(torch.int32))


def test_refusals_on_device(cops):
    x = _ints((1, 64, 8, 8), 1)
    w = _ints((64, 64, 3, 3), 2)
    with pytest.raises(ValueError):
        cops.conv(x.float(), w)
    with pytest.raises(ValueError):
        cops.conv(x, w.float())
    with pytest.raises(RuntimeError):
        cops.conv(x, w, dilation=9)
    with pytest.raises(RuntimeError):
        cops.conv(_ints((1, 96, 8, 8), 3), _ints((64, 96, 1, 1), 4))


def _head(dtype):
    from deepinteract_amd.head import ResNet2DInputWithOptAttention
    from deepinteract_amd.weights import seeded_state_dict
    sd = seeded_state_dict(0)
    hsd = {k[len("interact_module."):]: v for k, v in sd.items() if k.startswith("interact_module.")}
    m = ResNet2DInputWithOptAttention().cuda().eval()
    m.load_state_dict(hsd)
    return m.to(dtype=dtype)


def test_whole_head_no_worse_than_miopen_bf16(cops):
    """58 + 4 ResNet blocks on the seeded weights: the logits' error against the fp32 torch head,
    e_hip (HIP convolutions) against e_mi (bf16 MIOpen convolutions + HIP norm passes). Both round to
    bf16 at the same points; the factor 2 covers two different accumulation orders of the same
    roundings."""
    from deepinteract_amd.head import HeadNormOps
    t = torch.randn(1, 256, 48, 40, generator=torch.Generator().manual_seed(0)).cuda()
    with torch.no_grad():
        with torch.backends.cudnn.flags(enabled=False):
            ref = _head(torch.float32)(t)
        mi = _head(torch.bfloat16).use_hip_norm_ops(HeadNormOps("cuda"))
        y_mi = mi(t.to(torch.bfloat16)).float()
        hip = _head(torch.bfloat16).use_hip_norm_ops(HeadNormOps("cuda")).use_hip_convs(cops)
        y_hip = hip(t.to(torch.bfloat16)).float()
    e_mi = float((y_mi - ref).abs().max() / ref.abs().max())
    e_hip = float((y_hip - ref).abs().max() / ref.abs().max())
    print(f"whole head 48x40: e_hip = {e_hip:.3e}, e_mi = {e_mi:.3e}")
    assert y_hip.shape == ref.shape and bool(torch.isfinite(y_hip).all())
    assert e_hip <= 2 * e_mi


def test_model_head_convs_hip_on_tiny_fixture():
    """LitGINI(head_convs="hip") against the fixture's golden logits, beside the bf16 torch-conv model."""
    from deepinteract_amd.graph import GraphBatch
    from deepinteract_amd.modules import LitGINI
    from deepinteract_amd.weights import seeded_state_dict
    sd = seeded_state_dict(0)
    z = load_case("tiny")
    gb = GraphBatch.from_arrays([chain_item(z, "g1"), chain_item(z, "g2")], "cuda")
    err = {}
    for convs in ("torch", "hip"):
        model = LitGINI(dtype="bf16", head_dtype=torch.bfloat16, head_convs=convs).cuda().eval() \
            .load_reference_state_dict(sd)
        with torch.no_grad():
            logits, probs = model.predict_batch(gb, [(0, 1)])
        torch.cuda.synchronize()
        lg = logits[0].detach().float().cpu().numpy()
        assert np.isfinite(lg).all() and lg.shape == z["logits"].shape
        err[convs] = rel_max(lg, z["logits"])
    print(f"tiny: logits rel err vs golden: head_convs=hip {err['hip']:.3e}, torch {err['torch']:.3e}")
    assert err["hip"] <= 2 * err["torch"]
