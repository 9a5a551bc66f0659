"""GPU tests of the fp32 head convolutions (csrc/head_conv_f32.hip, head.HeadConvOps on fp32 images):
di_head_conv_f32 with di_plane_stats / di_head_norm_fold, then the whole head and the model with
``head_convs="hip_f32"``. The helpers are those of test_gpu_head_conv.py with fp32 storage.

Exact cases: inputs and weights are integers in [-4, 4] stored as fp32, so every product and every
partial sum is an integer of magnitude <= 16 K <= 36864 < 2^24, exact in fp32 in any order: the output
must equal the fp64 tap-sum convolution cast to fp32, bit for bit. The stored values are integers too,
so their fp64 sums are exact in any order, and a thread's fp32 sum of 4 squares is exact while
|y| < 2048 (4 * 2^22 = 2^24; asserted on the reference): the statistics partials must add up to the fp64
sums of y and y^2 exactly.

Transform cases: against ref = conv(ELU(x s + b), w) in fp64, with S the same convolution of absolute
values: |y - ref| <= ((K + 4) 2^-24 + e_elu) S -- one fp32 rounding in the affine step and one per
accumulated term, and the ELU's relative error, e_elu = 2^-22 for the kernel's expm1f. A transform
applied to the padding, a missing ELU or swapped scale / shift is O(S).
Measured on MI355X: the worst |y - ref| / bound over the cases and forms is 0.047.

Fold cases: 1e-6 relative (+1e-7) against fp64, the bound of test_gpu_head_conv.py.

Whole head, 48 x 40 on the seeded weights, against the same module in float64 on the CPU:
e = max|y - ref64| / max|ref64| <= 1e-4, the project's fp32 bound. Measured on MI355X: 1.0e-6 for the
hip_f32 head and 7.4e-7 for the fp32 torch head (MIOpen's fast algorithms off).
"""
import pytest
import torch
import torch.nn.functional as F

from gpu_common import chain_item, close_elem, load_case, rel_elem, rel_max

pytestmark = pytest.mark.gpu

SHAPES_3 = [(1, 1), (3, 5), (17, 9), (33, 70), (64, 64), (145, 145), (70, 257)]
SHAPES_1 = [(3, 5), (33, 70), (145, 145)]
CH_1 = [(128, 64), (64, 128), (128, 128), (256, 128)]
E_ELU = 2.0 ** -22   # expm1f (the kernel's header comment)


@pytest.fixture(scope="module")
def cops():
    from deepinteract_amd.head import HeadConvOps
    return HeadConvOps("cuda")


def _ints(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, shape, generator=g).to(torch.float32).cuda()


def _x(C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    # per-channel offsets and scales so the statistics are non-trivial (as test_gpu_head_ops._x)
    x = torch.randn(1, C, H, W, generator=g) * (0.5 + torch.rand(C, generator=g))[None, :, None, None] \
        + 3 * torch.randn(C, generator=g)[None, :, None, None]
    return x.cuda()


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
    b = _ints((cout,), 300 + seed) if bias else None
    ref = _conv64(x.double(), w.double(), d)
    if bias:
        ref = ref + b.double()[None, :, None, None]
    assert float(ref.abs().max()) < 2048  # the exactness argument for the fp32 sums of 4 squares
    y, st = cops.conv(x, w, bias=b, dilation=d, stats=True)
    assert y.shape == ref.shape and y.dtype == torch.float32
    assert torch.equal(y, ref.float()), f"max |diff| {float((y.double() - ref).abs().max())}"
    s, ss = _partials(st, cout)
    assert torch.equal(s, ref.sum(dim=(0, 2, 3))) and torch.equal(ss, (ref * ref).sum(dim=(0, 2, 3)))
    # ... and the folded mean is their one correctly rounded quotient
    (mean,) = cops.fold(st, cout, H * W, want=("mean",))
    assert torch.equal(mean, (ref.sum(dim=(0, 2, 3)) / (H * W)).float())


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
    """fp64 reference for the first and last `rows` output rows from cropped bands: d extra rows towards
    the image's inside, padding only at the true image edge (the convolution's own padding on the
    cropped side lands in rows that are dropped)."""
    H = x.shape[2]
    top = _conv64(x[:, :, :rows + d].double(), w.double(), d)[:, :, :rows]
    bot = _conv64(x[:, :, H - rows - d:].double(), w.double(), d)[:, :, -rows:]
    return top, bot


def test_exact_past_2gb(cops):
    """Plane offsets past 2^31 bytes: 64 -> 64 3x3 d = 8 at 2900 x 2900 fp32 (2.15 GB in and out); the
    first and last 24 rows, exact."""
    L, d = 2900, 8
    g = torch.Generator(device="cuda").manual_seed(L)
    x = torch.randint(-4, 5, (1, 64, L, L), generator=g, device="cuda", dtype=torch.int8).to(torch.float32)
    assert x.numel() * 4 > 2 ** 31
    w = _ints((64, 64, 3, 3), 400 + L)
    y, st = cops.conv(x, w, dilation=d, stats=True)
    top, bot = _band_ref(x, w, d, 24)
    assert torch.equal(y[:, :, :24], top.float())
    assert torch.equal(y[:, :, -24:], bot.float())
    assert float(y[:, :, -24:].abs().max()) > 0
    s, _ = _partials(st, 64)
    assert torch.equal(s, y.sum(dim=(0, 2, 3), dtype=torch.float64))


TRANSFORM_CASES = [(64, 64, 3, 2, (33, 70)), (64, 64, 3, 8, (33, 70)), (128, 64, 1, 1, (145, 145))]


def _transform_inputs(cin, cout, k, shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = _x(cin, *shape, seed)
    w = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).cuda()
    s = (1 + 0.3 * torch.randn(cin, generator=g)).cuda()
    b = (0.3 * torch.randn(cin, generator=g)).cuda()
    return x, w, s, b


def _ratio(y, a, w, d, K):
    ref, S = _conv64(a, w.double(), d), _conv64(a.abs(), w.double().abs(), d)
    return float(((y.double() - ref).abs() / (((K + 4) * 2.0 ** -24 + E_ELU) * S)).max())


@pytest.mark.parametrize("cin,cout,k,d,shape", TRANSFORM_CASES)
def test_transform(cops, cin, cout, k, d, shape):
    x, w, s, b = _transform_inputs(cin, cout, k, shape, 21)
    K = cin * k * k
    sd, bd = s.double()[None, :, None, None], b.double()[None, :, None, None]
    y = cops.conv(x, w, in_scale=s, in_shift=b, in_elu=True, dilation=d)
    ratio = _ratio(y, F.elu(x.double() * sd + bd), w, d, K)
    print(f"transform {cin}->{cout} k{k} d{d} {shape}: max |y - ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    # the affine form without ELU, and scale / shift each alone (NULL means 1 / 0)
    for kw, fn in ((dict(in_scale=s, in_shift=b), lambda v: v * sd + bd),
                   (dict(in_scale=s), lambda v: v * sd),
                   (dict(in_shift=b, in_elu=True), lambda v: F.elu(v + bd))):
        r2 = _ratio(cops.conv(x, w, dilation=d, **kw), fn(x.double()), w, d, K)
        print(f"  {sorted(kw)}: {r2:.3f}")
        assert r2 <= 1.0, kw


def _fold64(x, gamma, beta, eps, bias):
    xd = x.double()
    m = xd.mean(dim=(0, 2, 3))
    var = (xd * xd).mean(dim=(0, 2, 3)) - m * m
    sc = gamma.double() / torch.sqrt(var + eps)
    return sc, beta.double() - m * sc, m + bias.double()


def _close(a, ref):
    return float((a.double() - ref).abs().max()) < 1e-6 * float(ref.abs().max()) + 1e-7


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
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
    assert torch.equal(outs[0][1].view(torch.int64), outs[1][1].view(torch.int64))
    for a, c in zip(outs[0][2], outs[1][2]):
        assert torch.equal(a.view(torch.int32), c.view(torch.int32))


def test_refusals_on_device(cops):
    x = _ints((1, 64, 8, 8), 1)
    w = _ints((64, 64, 3, 3), 2)
    with pytest.raises(ValueError):
        cops.conv(x, w.bfloat16())
    with pytest.raises(ValueError):
        cops.conv(x.bfloat16(), w)
    with pytest.raises(RuntimeError):
        cops.conv(x, w, dilation=9)
    with pytest.raises(RuntimeError):
        cops.conv(_ints((1, 96, 8, 8), 3), _ints((64, 96, 1, 1), 4))


def _head(dtype, device="cuda"):
    from deepinteract_amd.head import ResNet2DInputWithOptAttention
    from deepinteract_amd.weights import seeded_state_dict
    sd = seeded_state_dict(0)
    hsd = {k[len("interact_module."):]: v for k, v in sd.items() if k.startswith("interact_module.")}
    m = ResNet2DInputWithOptAttention().eval()
    m.load_state_dict(hsd)
    return m.to(device=device, dtype=dtype)


def test_whole_head_against_float64(cops):
    """58 + 4 ResNet blocks on the seeded weights against the same module in float64 on the CPU: the
    hip_f32 head within the project's fp32 bound, the fp32 torch head's error printed beside it."""
    from deepinteract_amd.head import HeadNormOps
    t = torch.randn(1, 256, 48, 40, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        ref = _head(torch.float64, "cpu")(t.double())
        with torch.backends.cudnn.flags(enabled=False):
            y_torch = _head(torch.float32)(t.cuda()).double().cpu()
            hip = _head(torch.float32).use_hip_norm_ops(HeadNormOps("cuda")).use_hip_convs(cops)
            y_hip = hip(t.cuda()).double().cpu()
    e_torch = float((y_torch - ref).abs().max() / ref.abs().max())
    e_hip = float((y_hip - ref).abs().max() / ref.abs().max())
    print(f"whole head 48x40 vs float64: e_hip_f32 = {e_hip:.3e}, e_torch_f32 = {e_torch:.3e}")
    assert y_hip.shape == ref.shape and bool(torch.isfinite(y_hip).all())
    assert e_hip <= 1e-4


def _residue_graph(z, tag):
    from deepinteract_amd.graph import ResidueGraph
    it = chain_item(z, tag)
    g = ResidueGraph(it["src"], it["dst"], it["num_nodes"])
    g.ndata["f"] = it["node_f"]
    g.edata["f"] = it["edge_f"]
    g.edata["src_nbr_e_ids"] = it["src_nbr"]
    g.edata["dst_nbr_e_ids"] = it["dst_nbr"]
    return g.to("cuda")


def _model(**kw):
    from deepinteract_amd.modules import LitGINI
    from deepinteract_amd.weights import seeded_state_dict
    return LitGINI(dtype="f32", head_convs="hip_f32", **kw).cuda().eval().load_reference_state_dict(seeded_state_dict(0))


@pytest.fixture(scope="module")
def model():
    return _model()


def _check_model(model, case):
    """The checks of test_gpu_api.py::test_shared_step_and_predict_step on the logits and probabilities."""
    from deepinteract_amd.head import HeadConvOps, contact_probs
    z = load_case(case)
    with torch.no_grad():
        logits = model.shared_step(_residue_graph(z, "g1"), _residue_graph(z, "g2"))
    assert isinstance(model.interact_module.cops, HeadConvOps)
    lg = logits[0].detach().float().cpu().numpy()
    assert len(logits) == 1 and lg.shape == tuple(z["logits"].shape)
    lc, pe = close_elem(lg, z["logits"]), rel_elem(contact_probs(logits[0]).detach().cpu().numpy(), z["probs"])
    print(f"{case} hip_f32: logits normwise {rel_max(lg, z['logits']):.3e}, allclose ratio {lc:.3f}, "
          f"probabilities elementwise relative {pe:.3e}")
    assert rel_max(lg, z["logits"]) < 1e-4 and lc <= 1.0 and pe < 1e-4


@pytest.mark.parametrize("case", ["tiny", "c1", "c2"])
def test_model_head_convs_hip_f32(model, case):
    _check_model(model, case)


def test_model_head_convs_hip_f32_fused_prologue():
    _check_model(_model(fuse_head_prologue=True), "tiny")


def test_whole_head_with_attention_against_the_fixture(cops):
    """use_interact_attention: the head with its regional attention on tests/golden/attn_head.npz's 11 x 19
    input against the reference's logits."""
    import attn_cases as A
    from deepinteract_amd.head import HeadNormOps
    fx = A.fixture()
    head = A.build_head().cuda().float().use_hip_norm_ops(HeadNormOps("cuda")).use_hip_convs(cops)
    assert head.aops is not None
    with torch.no_grad():
        y = head(fx["input"].cuda())
    torch.cuda.synchronize()
    ref = fx["logits"]
    err = float((y.cpu() - ref).abs().max() / ref.abs().max())
    print(f"whole hip_f32 head with attention vs the reference's logits: {err:.3e}")
    assert y.dtype == torch.float32 and err <= 1e-4
