"""GPU tests of the batched contact head (head.HeadBatch, the *_batch entry points of csrc/head_conv.hip
and csrc/head_ops.hip, di_se_gate, ResNet2DInputWithOptAttention.body_batch, LitGINI(head_batch=N)).

Per-item cases are bit-exact against the single calls: a batch kernel runs the single kernel's code on
the item's own sizes, so ``torch.equal`` on integer views is the bar, for the output, the statistics
header and every partial. The batches hold 1x1, 3x5, 16x16, 17x9, 33x70 beside 145x145 (most items
have far fewer tiles than the grid, so the early exit is exercised), largest first and largest last,
and a batch of one.

di_se_gate is checked against the same formula in fp64 with the bound of fp32 accumulation written
out in test_se_gate_against_fp64 (measured on MI355X: 0.005 of the bound).

Whole head against the fp32 torch head, measured on MI355X, e_batch / e_hip:
48x40 1.69e-2 / 1.94e-2, 17x9 2.01e-2 / 1.47e-2, 70x33 1.72e-2 / 1.78e-2; the model against the golden
logits, head_batch=4 / head_batch=0: tiny 2.20e-2 / 2.07e-2, c1 2.32e-2 / 2.31e-2.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_common import chain_item, load_case, rel_max

pytestmark = pytest.mark.gpu

SMALL = [(1, 1), (3, 5), (16, 16), (17, 9), (33, 70)]
BATCHES = {"largest_first": [(145, 145)] + SMALL, "largest_last": SMALL + [(145, 145)], "one": [(33, 70)]}
CONVS = [(3, 64, 64, 1), (3, 64, 64, 2), (3, 64, 64, 4), (3, 64, 64, 8), (1, 128, 64, 1), (1, 64, 128, 1),
         (1, 128, 128, 1)]


@pytest.fixture(scope="module")
def cops():
    from deepinteract_amd.head import HeadConvOps
    return HeadConvOps("cuda")


@pytest.fixture(scope="module")
def ops():
    from deepinteract_amd.head import HeadNormOps
    return HeadNormOps("cuda")


@pytest.fixture(scope="module", params=list(BATCHES))
def batch(request):
    """(HeadBatch, {C: images}) -- the images are made once per batch and never written."""
    from deepinteract_amd.head import HeadBatch
    shapes = BATCHES[request.param]
    hb = HeadBatch(shapes, "cuda")
    g = torch.Generator().manual_seed(len(shapes))
    images = {}
    for C in (64, 128):
        images[C] = [(torch.randn(1, C, h, w, generator=g) * (0.5 + torch.rand(C, generator=g))[None, :, None, None]
                      + torch.randn(C, generator=g)[None, :, None, None]).to(torch.bfloat16).cuda()
                     for h, w in shapes]
    return hb, images


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _single_stats(st, C):
    n = int(st[:1].view(torch.int64).item())
    return st[:2 + C * n * 2]


def test_layout_on_device(batch):
    hb, _ = batch
    assert hb.pixels == sum(h * w for h, w in hb.shapes)
    back = hb.items_dev.cpu().view(torch.int64).view(-1, 3)      # px_off, stats_off, (h, w)
    assert back[:, 0].tolist() == hb.px_off and back[:, 1].tolist() == hb.stats_off
    assert hb.input(hb.count - 1).shape == (1, 128) + tuple(hb.shapes[-1])


@pytest.mark.parametrize("k,cin,cout,d", CONVS, ids=lambda v: str(v))
def test_conv_batch_bit_exact_per_item(cops, batch, k, cin, cout, d):
    hb, images = batch
    g = torch.Generator().manual_seed(100 * k + d + cin)
    w = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).to(torch.bfloat16).cuda()
    s = (1 + 0.3 * torch.randn(hb.count, cin, generator=g)).cuda()
    b = (0.3 * torch.randn(hb.count, cin, generator=g)).cuda()
    bias = torch.randn(cout, generator=g).cuda()
    x = hb.pack(images[cin])
    # scale + shift + ELU with per-item rows; then bias and no transform
    for kw_b, kw_1 in ((dict(in_scale=s, in_shift=b, in_elu=True), lambda i: dict(in_scale=s[i], in_shift=b[i],
                                                                                    in_elu=True)),
                       (dict(bias=bias), lambda i: dict(bias=bias))):
        y, st = cops.conv_batch(hb, x, w, dilation=d, stats=True, **kw_b)
        y, st = y.clone(), st.clone()
        for i, im in enumerate(images[cin]):
            y1, st1 = cops.conv(im, w, dilation=d, stats=True, **kw_1(i))
            assert torch.equal(_bits(hb.view(y, cout, i)), _bits(y1)), (i, hb.shapes[i])
            assert torch.equal(_bits(hb.item_stats(st, i, cout)), _bits(_single_stats(st1, cout))), (i, hb.shapes[i])
    # without statistics the output is the same and the statistics buffer is left alone
    before = hb.stats.clone()
    y2 = cops.conv_batch(hb, x, w, dilation=d, bias=bias)
    assert torch.equal(_bits(y2), _bits(y)) and torch.equal(_bits(hb.stats), _bits(before))


@pytest.mark.parametrize("C", [64, 128])
def test_norm_passes_bit_exact_per_item(cops, ops, batch, C):
    hb, images = batch
    g = torch.Generator().manual_seed(C)
    gamma, beta, bias = ((1 + 0.3 * torch.randn(C, generator=g)).cuda(), (0.3 * torch.randn(C, generator=g)).cuda(),
                         torch.randn(C, generator=g).cuda())
    x = hb.pack(images[C])
    st = cops.plane_stats_batch(hb, x, C).clone()
    sc, sh, mean = cops.fold_batch(hb, st, C, gamma, beta, 1e-6, bias, want=("scale", "shift", "mean"))
    (mean_only,) = cops.fold_batch(hb, st, C, want=("mean",))
    for i, im in enumerate(images[C]):
        st1 = cops.plane_stats(im)
        assert torch.equal(_bits(hb.item_stats(st, i, C)), _bits(_single_stats(st1, C))), (i, hb.shapes[i])
        hw = im.shape[2] * im.shape[3]
        sc1, sh1, mean1 = cops.fold(st1, C, hw, gamma, beta, 1e-6, bias, want=("scale", "shift", "mean"))
        (m1,) = cops.fold(st1, C, hw, want=("mean",))
        for a, r in ((sc[i], sc1), (sh[i], sh1), (mean[i], mean1), (mean_only[i], m1)):
            assert torch.equal(_bits(a), _bits(r)), (i, hb.shapes[i])
    # SE gate + bias + residual: out of place, then in place into x's copy and into the residual's copy
    res_images = [torch.roll(im, 1, dims=1) for im in images[C]]
    res = hb.pack(res_images)
    gate = torch.rand(hb.count, C, generator=g).cuda()
    want = [ops.se_scale_add(im, gate[i], r, bias=bias) for i, (im, r) in enumerate(zip(images[C], res_images))]
    y = ops.se_scale_add_batch(hb, x, gate, res, bias=bias)
    xin, rin = x.clone(), res.clone()
    assert ops.se_scale_add_batch(hb, xin, gate, res, out=xin, bias=bias) is xin
    ops.se_scale_add_batch(hb, x, gate, rin, out=rin, bias=bias)
    nobias = ops.se_scale_add_batch(hb, x, gate, res)
    for i in range(hb.count):
        for got in (y, xin, rin):
            assert torch.equal(_bits(hb.view(got, C, i)), _bits(want[i])), (i, hb.shapes[i])
        assert torch.equal(_bits(hb.view(nobias, C, i)),
                           _bits(ops.se_scale_add(images[C][i], gate[i], res_images[i]))), (i, hb.shapes[i])


def test_se_gate_against_fp64(ops):
    """|g - ref| <= e2 / 4 + 2^-22 with e2_i = 9 2^-24 S2_i + sum_j |W2_ij| 129 2^-24 S1_j, S1 / S2 the
    absolute-value dot products including the bias: fp32 accumulation of 128 (+ bias) and 8 (+ bias)
    terms, ReLU 1-Lipschitz, sigmoid 1/4-Lipschitz, and a few ulp below 1 for the hardware exponential
    and reciprocal."""
    from deepinteract_amd.head import SEBlock
    torch.manual_seed(5)
    se = SEBlock(128, 16).cuda()
    with torch.no_grad():
        se.linear1.bias.normal_(0, 0.5)
        se.linear2.bias.normal_(0, 0.5)
        se.linear2.weight.mul_(3)
    g = torch.Generator().manual_seed(6)
    mean = (2 * torch.randn(6, 128, generator=g) + torch.randn(128, generator=g)).cuda()
    gate = ops.se_gate(se, mean)
    again = ops.se_gate(se, mean.clone())
    assert gate.shape == mean.shape and gate.dtype == torch.float32
    assert torch.equal(_bits(gate), _bits(again))                      # two runs, the same bits
    for rows in ([0], [3], [5, 1, 2]):                                 # a row does not depend on count
        sub = ops.se_gate(se, mean[rows].contiguous())
        assert torch.equal(_bits(sub), _bits(gate[rows]))
    w1, b1, w2, b2 = (t.detach().double() for t in (se.linear1.weight, se.linear1.bias, se.linear2.weight,
                                                     se.linear2.bias))
    m = mean.double()
    hid = F.relu(m @ w1.T + b1)
    ref = torch.sigmoid(F.relu(hid @ w2.T + b2))
    S1 = m.abs() @ w1.abs().T + b1.abs()
    S2 = hid.abs() @ w2.abs().T + b2.abs()
    e2 = 9 * 2.0 ** -24 * S2 + (129 * 2.0 ** -24 * S1) @ w2.abs().T
    ratio = float(((gate.double() - ref).abs() / (e2 / 4 + 2.0 ** -22)).max())
    print(f"se_gate: largest |g - ref| / bound = {ratio:.3f}")
    assert float(ref.min()) < 0.6 and float(ref.max()) > 0.9            # both ends of the gate's range
    assert ratio <= 1.0


# ---- whole head
HEAD_SHAPES = [(48, 40), (17, 9), (70, 33)]


def _head(dtype):
    from deepinteract_amd.head import ResNet2DInputWithOptAttention
    from deepinteract_amd.weights import seeded_state_dict
    sd = seeded_state_dict(0)
    hsd = {k[len("interact_module."):]: v for k, v in sd.items() if k.startswith("interact_module.")}
    m = ResNet2DInputWithOptAttention().cuda().eval()
    m.load_state_dict(hsd)
    return m.to(dtype=dtype)


@pytest.fixture(scope="module")
def whole_head(cops, ops):
    """The three inputs, the fp32 torch reference, the single-complex HIP path and the batch of three."""
    g = torch.Generator().manual_seed(0)
    ts = [torch.randn(1, 256, h, w, generator=g).cuda() for h, w in HEAD_SHAPES]
    with torch.no_grad():
        with torch.backends.cudnn.flags(enabled=False):
            f32 = _head(torch.float32)
            refs = [f32(t) for t in ts]
        hip = _head(torch.bfloat16).use_hip_norm_ops(ops).use_hip_convs(cops)
        single = [hip(t.to(torch.bfloat16)) for t in ts]
        pro = [ops.inorm_elu(hip.conv2d_1(t.to(torch.bfloat16)), hip.inorm_1) for t in ts]
        three = hip.body_batch(pro)
    return hip, pro, refs, single, three


def test_whole_head_batch_bits_do_not_depend_on_the_batch(whole_head):
    hip, pro, refs, _, three = whole_head
    with torch.no_grad():
        for i, x in enumerate(pro):
            (one,) = hip.body_batch([x])
            assert one.shape == refs[i].shape and torch.equal(_bits(one), _bits(three[i])), HEAD_SHAPES[i]
        order = [2, 0, 1]
        other = hip.body_batch([pro[i] for i in order])
        for slot, i in enumerate(order):
            assert torch.equal(_bits(other[slot]), _bits(three[i])), HEAD_SHAPES[i]


def test_whole_head_batch_no_worse_than_single(whole_head):
    """e_batch <= 2 e_hip per complex against the fp32 torch head: both paths round to bf16 at the same
    points; the batch differs from the single path only by its unrounded fp32 gate."""
    _, _, refs, single, three = whole_head
    for shape, ref, y1, yb in zip(HEAD_SHAPES, refs, single, three):
        e_hip = float((y1.float() - ref).abs().max() / ref.abs().max())
        e_batch = float((yb.float() - ref).abs().max() / ref.abs().max())
        print(f"whole head {shape[0]}x{shape[1]}: e_batch = {e_batch:.3e}, e_hip = {e_hip:.3e}")
        assert yb.shape == ref.shape and bool(torch.isfinite(yb).all())
        assert e_batch <= 2 * e_hip


# ---- model
@pytest.fixture(scope="module")
def model_case():
    from deepinteract_amd.graph import GraphBatch
    from deepinteract_amd.modules import LitGINI
    from deepinteract_amd.weights import seeded_state_dict
    sd = seeded_state_dict(0)
    zs = [load_case("tiny"), load_case("c1")]
    gb = GraphBatch.from_arrays([chain_item(z, tag) for z in zs for tag in ("g1", "g2")], "cuda")
    pairs = [(0, 1), (2, 3)]
    out = {}
    for n in (4, 0):
        model = LitGINI(dtype="bf16", head_dtype=torch.bfloat16, head_convs="hip", head_batch=n).cuda().eval() \
            .load_reference_state_dict(sd)
        with torch.no_grad():
            logits, probs = model.predict_batch(gb, pairs)
        torch.cuda.synchronize()
        out[n] = (model, [lg.detach().clone() for lg in logits], probs)
    return zs, gb, pairs, out


def test_model_head_batch_against_golden(model_case):
    zs, _, _, out = model_case
    for i, z in enumerate(zs):
        lg4 = out[4][1][i].float().cpu().numpy()
        lg0 = out[0][1][i].float().cpu().numpy()
        assert lg4.shape == lg0.shape == z["logits"].shape
        assert np.isfinite(lg4).all() and np.isfinite(lg0).all()
        assert out[4][2][i].shape == out[0][2][i].shape and bool(torch.isfinite(out[4][2][i]).all())
        e4, e0 = rel_max(lg4, z["logits"]), rel_max(lg0, z["logits"])
        print(f"complex {i}: logits rel err vs golden: head_batch=4 {e4:.3e}, head_batch=0 {e0:.3e}")
        assert e4 <= 2 * e0


def test_model_pixel_cap_gives_the_same_bits(model_case):
    _, gb, pairs, out = model_case
    model, one_chunk, _ = out[4]
    shapes = [tuple(lg.shape[2:]) for lg in one_chunk]
    assert model._head_chunks(shapes) == [[0, 1]]
    model.head_batch_pixels = 3000                      # 48 x 48 fits, 145 x 145 goes alone
    try:
        assert model._head_chunks(shapes) == [[0], [1]]
        with torch.no_grad():
            logits, _ = model.predict_batch(gb, pairs)
    finally:
        model.head_batch_pixels = 2 ** 22
    for a, b in zip(logits, one_chunk):
        assert torch.equal(_bits(a), _bits(b))
