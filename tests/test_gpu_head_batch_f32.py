"""GPU tests of the batched fp32 contact head (head.HeadBatch(dtype=torch.float32), di_head_conv_f32_batch,
di_plane_stats_f32_batch, di_se_scale_add_f32_batch, ResNet2DInputWithOptAttention.body_batch on an fp32
head, LitGINI(head_convs="hip_f32", head_batch_f32=N)). It mirrors test_gpu_head_batch.py.

Per-item cases are bit-exact against the single calls (di_head_conv_f32, di_plane_stats(DI_F32),
di_se_scale_add(DI_F32)): a batch kernel runs the single kernel's code on the item's own sizes, so
``torch.equal`` on integer views is the bar, for the output, the statistics header and every partial. The
batches hold 1x1, 3x5, 16x16, 17x9, 33x70 beside 145x145 (most items have far fewer tiles than the grid,
so the early exit and the per-item numbering of the statistics' blocks are exercised), largest first and
largest last, and a batch of one.

One exact case guards against a batch that is merely consistently wrong: integer inputs and weights in
[-4, 4] (test_gpu_head_conv_f32.py's argument: every product and partial sum is an integer below 2^24,
|ref| < 2048 asserted), every item equal to the fp64 tap-sum convolution bit for bit.

Whole head (58 + 4 blocks, seeded weights) against the same module in float64 on the CPU, the bound and
the reference of test_gpu_head_conv_f32.py::test_whole_head_against_float64 (e <= 1e-4). The batched path
takes its SE gate from di_se_gate (an fp32 fmaf chain in index order), the single path from torch's fp32
linears, so the two are not the same bits; measured on MI355X, e_batch / e_single /
largest |batch - single| over max |ref|:
48x40 1.056e-6 / 1.006e-6 / 9.17e-7, 17x9 8.52e-7 / 6.69e-7 / 8.20e-7, 70x33 8.67e-7 / 1.005e-6 / 7.65e-7
(measurements, not bars). With attention (the 11x19 fixture beside a 16x16 filler): 5.26e-7 of the
reference's logits. The model against the golden logits with head_batch_f32=4, tiny / c1 / c2: normwise
2.3e-6 / 2.6e-6 / 2.6e-6, allclose ratio 0.14 / 0.21 / 0.23, probabilities 5.8e-6 / 6.6e-6 / 6.7e-6.
"""
import numpy as np
import pytest
import torch

from gpu_common import chain_item, close_elem, load_case, rel_elem, rel_max
from test_gpu_head_conv_f32 import _conv64, _head, _ints, _partials

pytestmark = pytest.mark.gpu

SMALL = [(1, 1), (3, 5), (16, 16), (17, 9), (33, 70)]
BATCHES = {"largest_first": [(145, 145)] + SMALL, "largest_last": SMALL + [(145, 145)], "one": [(33, 70)]}
# 3x3 64 -> 64 at d = 1, 2, 4, 8: each DMAX instantiation and both blocks-per-CU settings; the three 1x1 shapes
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
    """(fp32 HeadBatch, {C: images}) -- the images are made once per batch and never written."""
    from deepinteract_amd.head import HeadBatch
    shapes = BATCHES[request.param]
    hb = HeadBatch(shapes, "cuda", dtype=torch.float32)
    g = torch.Generator().manual_seed(len(shapes))
    images = {}
    for C in (64, 128):
        images[C] = [(torch.randn(1, C, h, w, generator=g) * (0.5 + torch.rand(C, generator=g))[None, :, None, None]
                      + torch.randn(C, generator=g)[None, :, None, None]).cuda()
                     for h, w in shapes]
    return hb, images


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _single_stats(st, C):
    n = int(st[:1].view(torch.int64).item())
    return st[:2 + C * n * 2]


def test_fp32_arena(batch):
    from deepinteract_amd.head import HeadAttnOps
    hb, images = batch
    assert hb.dtype == torch.float32 and hb.pixels == sum(h * w for h, w in hb.shapes)
    assert all(t.dtype == torch.float32 for t in hb.wide + hb.half)
    assert sum(t.numel() * t.element_size() for t in hb.wide + hb.half) == 1536 * hb.pixels
    assert hb.input(hb.count - 1).shape == (1, 128) + tuple(hb.shapes[-1])
    s = HeadAttnOps.batch_scores_buffer(hb)
    assert s.dtype == torch.float32 and s.numel() == 4 * hb.pixels and s.data_ptr() == hb.half[0].data_ptr()
    with pytest.raises(ValueError):
        hb.check_packed(hb.wide[0].bfloat16(), 128)
    x = hb.pack(images[64])
    assert x.dtype == torch.float32 and torch.equal(hb.view(x, 64, hb.count - 1), images[64][-1])


@pytest.mark.parametrize("k,cin,cout,d", CONVS, ids=lambda v: str(v))
def test_conv_batch_bit_exact_per_item(cops, batch, k, cin, cout, d):
    hb, images = batch
    g = torch.Generator().manual_seed(100 * k + d + cin)
    w = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).cuda()
    s = (1 + 0.3 * torch.randn(hb.count, cin, generator=g)).cuda()
    b = (0.3 * torch.randn(hb.count, cin, generator=g)).cuda()
    bias = torch.randn(cout, generator=g).cuda()
    x = hb.pack(images[cin])
    # scale + shift + ELU with per-item rows; then bias and no transform
    for kw_b, kw_1 in ((dict(in_scale=s, in_shift=b, in_elu=True), lambda i: dict(in_scale=s[i], in_shift=b[i],
                                                                                    in_elu=True)),
                       (dict(bias=bias), lambda i: dict(bias=bias))):
        y, st = cops.conv_batch(hb, x, w, dilation=d, stats=True, **kw_b)
        assert y.dtype == torch.float32
        y, st = y.clone(), st.clone()
        for i, im in enumerate(images[cin]):
            y1, st1 = cops.conv(im, w, dilation=d, stats=True, **kw_1(i))
            assert torch.equal(_bits(hb.view(y, cout, i)), _bits(y1)), (i, hb.shapes[i])
            assert torch.equal(_bits(hb.item_stats(st, i, cout)), _bits(_single_stats(st1, cout))), (i, hb.shapes[i])
    # without statistics the output is the same and the statistics buffer is left alone
    before = hb.stats.clone()
    y2 = cops.conv_batch(hb, x, w, dilation=d, bias=bias)
    assert torch.equal(_bits(y2), _bits(y)) and torch.equal(_bits(hb.stats), _bits(before))


def test_conv_batch_exact_against_fp64():
    """Integers in [-4, 4]: every item of the batch equals the fp64 tap-sum convolution (+ integer bias) bit
    for bit, and its statistics partials add up to the fp64 sums of y and y^2 exactly."""
    from deepinteract_amd.head import HeadBatch, HeadConvOps
    cops = HeadConvOps("cuda")
    shapes, d = BATCHES["largest_first"], 4
    hb = HeadBatch(shapes, "cuda", dtype=torch.float32)
    images = [_ints((1, 64, h, w), 500 + i) for i, (h, w) in enumerate(shapes)]
    w, b = _ints((64, 64, 3, 3), 600), _ints((64,), 601)
    y, st = cops.conv_batch(hb, hb.pack(images), w, bias=b, dilation=d, stats=True)
    for i, im in enumerate(images):
        ref = _conv64(im.double(), w.double(), d) + b.double()[None, :, None, None]
        assert float(ref.abs().max()) < 2048  # the exactness argument for the fp32 sums of 4 squares
        assert torch.equal(hb.view(y, 64, i), ref.float()), (i, shapes[i])
        s, ss = _partials(hb.item_stats(st, i, 64), 64)
        assert torch.equal(s, ref.sum(dim=(0, 2, 3))) and torch.equal(ss, (ref * ref).sum(dim=(0, 2, 3))), shapes[i]
    assert float(hb.view(y, 64, 0).abs().max()) > 0


@pytest.mark.parametrize("C", [64, 128])
def test_norm_passes_bit_exact_per_item(cops, ops, batch, C):
    hb, images = batch
    g = torch.Generator().manual_seed(C)
    gamma, beta, bias = ((1 + 0.3 * torch.randn(C, generator=g)).cuda(), (0.3 * torch.randn(C, generator=g)).cuda(),
                         torch.randn(C, generator=g).cuda())
    x = hb.pack(images[C])
    st = cops.plane_stats_batch(hb, x, C).clone()
    sc, sh, mean = cops.fold_batch(hb, st, C, gamma, beta, 1e-6, bias, want=("scale", "shift", "mean"))
    for i, im in enumerate(images[C]):
        st1 = cops.plane_stats(im)
        assert torch.equal(_bits(hb.item_stats(st, i, C)), _bits(_single_stats(st1, C))), (i, hb.shapes[i])
        hw = im.shape[2] * im.shape[3]
        sc1, sh1, mean1 = cops.fold(st1, C, hw, gamma, beta, 1e-6, bias, want=("scale", "shift", "mean"))
        for a, r in ((sc[i], sc1), (sh[i], sh1), (mean[i], mean1)):
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
    assert y.dtype == torch.float32
    for i in range(hb.count):
        for got in (y, xin, rin):
            assert torch.equal(_bits(hb.view(got, C, i)), _bits(want[i])), (i, hb.shapes[i])
        assert torch.equal(_bits(hb.view(nobias, C, i)),
                           _bits(ops.se_scale_add(images[C][i], gate[i], res_images[i]))), (i, hb.shapes[i])


# ---- whole head
HEAD_SHAPES = [(48, 40), (17, 9), (70, 33)]


@pytest.fixture(scope="module")
def whole_head(cops, ops):
    """The three inputs' float64 CPU references, the single hip_f32 head's logits, the prologue outputs and the
    batch of three."""
    g = torch.Generator().manual_seed(0)
    ts = [torch.randn(1, 256, h, w, generator=g) for h, w in HEAD_SHAPES]
    with torch.no_grad():
        f64 = _head(torch.float64, "cpu")
        refs = [f64(t.double()) for t in ts]
        with torch.backends.cudnn.flags(enabled=False):
            hip = _head(torch.float32).use_hip_norm_ops(ops).use_hip_convs(cops)
            single = [hip(t.cuda()) for t in ts]
            pro = [ops.inorm_elu(hip.conv2d_1(t.cuda()), hip.inorm_1) for t in ts]
            three = hip.body_batch(pro)
    torch.cuda.synchronize()
    return hip, pro, refs, single, three


def test_whole_head_batch_bits_do_not_depend_on_the_batch(whole_head):
    hip, pro, refs, _, three = whole_head
    dot = torch.randn(1, 128, 1, 1, generator=torch.Generator().manual_seed(9)).cuda()
    order = [2, 0, None, 1]        # another order, a 1 x 1 image between them
    with torch.no_grad(), torch.backends.cudnn.flags(enabled=False):
        other = hip.body_batch([dot if i is None else pro[i] for i in order])
        with pytest.raises(RuntimeError, match="bf16 only"):
            hip.body_batch(pro, native=True)
    assert other[2].shape == (1, 2, 1, 1) and bool(torch.isfinite(other[2]).all())
    for slot, i in enumerate(order):
        if i is not None:
            assert three[i].dtype == torch.float32 and three[i].shape == refs[i].shape
            assert torch.equal(_bits(other[slot]), _bits(three[i])), HEAD_SHAPES[i]


def test_whole_head_batch_against_float64(whole_head):
    """e = max|y - ref64| / max|ref64| <= 1e-4 per image, the project's fp32 bound; the single hip_f32 head's e
    and the largest batched-vs-single difference are printed beside it (measurements, not bars)."""
    _, _, refs, single, three = whole_head
    for shape, ref, y1, yb in zip(HEAD_SHAPES, refs, single, three):
        top = float(ref.abs().max())
        e_single = float((y1.double().cpu() - ref).abs().max()) / top
        e_batch = float((yb.double().cpu() - ref).abs().max()) / top
        diff = float((yb.double() - y1.double()).abs().max()) / top
        print(f"whole fp32 head {shape[0]}x{shape[1]} vs float64: e_batch = {e_batch:.3e}, e_single = {e_single:.3e}, "
              f"max |batch - single| / max |ref| = {diff:.3e}")
        assert yb.shape == ref.shape and bool(torch.isfinite(yb).all())
        assert e_batch <= 1e-4


def test_whole_head_batch_with_attention_against_the_fixture(cops, ops):
    """use_interact_attention inside the fp32 arena (_attention_batch): tests/golden/attn_head.npz's 11 x 19
    input beside a 16 x 16 filler, against the reference's logits, in either slot."""
    import attn_cases as A
    fx = A.fixture()
    head = A.build_head().cuda().float().use_hip_norm_ops(ops).use_hip_convs(cops)
    assert head.aops is not None
    filler = torch.randn(1, 128, 16, 16, generator=torch.Generator().manual_seed(3)).cuda()
    with torch.no_grad():
        pro = ops.inorm_elu(head.conv2d_1(fx["input"].cuda()), head.inorm_1)
        y = head.body_batch([pro, filler])[0]
        y_last = head.body_batch([filler, pro])[1]
    torch.cuda.synchronize()
    ref = fx["logits"]
    err = float((y.cpu() - ref).abs().max() / ref.abs().max())
    print(f"batched hip_f32 head with attention vs the reference's logits: {err:.3e}")
    assert y.dtype == torch.float32 and y.shape == ref.shape and err <= 1e-4
    assert torch.equal(_bits(y), _bits(y_last))


# ---- model
CASES = ["tiny", "c1", "c2"]


def _model(**kw):
    from deepinteract_amd.modules import LitGINI
    from deepinteract_amd.weights import seeded_state_dict
    return LitGINI(dtype="f32", head_convs="hip_f32", **kw).cuda().eval().load_reference_state_dict(seeded_state_dict(0))


def _graph_batch(zs):
    from deepinteract_amd.graph import GraphBatch
    gb = GraphBatch.from_arrays([chain_item(z, tag) for z in zs for tag in ("g1", "g2")], "cuda")
    return gb, [(2 * i, 2 * i + 1) for i in range(len(zs))]


def _check_logits(tag, logits, z):
    """_check_model's three assertions of test_gpu_head_conv_f32.py."""
    from deepinteract_amd.head import contact_probs
    lg = logits.detach().float().cpu().numpy()
    assert lg.shape == tuple(z["logits"].shape)
    lc, pe = close_elem(lg, z["logits"]), rel_elem(contact_probs(logits).detach().cpu().numpy(), z["probs"])
    print(f"{tag}: logits normwise {rel_max(lg, z['logits']):.3e}, allclose ratio {lc:.3f}, "
          f"probabilities elementwise relative {pe:.3e}")
    assert rel_max(lg, z["logits"]) < 1e-4 and lc <= 1.0 and pe < 1e-4


@pytest.fixture(scope="module")
def model_run():
    zs = [load_case(c) for c in CASES]
    gb, pairs = _graph_batch(zs)
    model = _model(head_batch_f32=4)
    with torch.no_grad():
        logits, probs = model.predict_batch(gb, pairs)
    torch.cuda.synchronize()
    return zs, gb, pairs, model, [lg.detach().clone() for lg in logits], probs


def test_model_head_batch_f32_against_golden(model_run):
    zs, _, _, model, logits, probs = model_run
    assert model._head_chunks([tuple(lg.shape[2:]) for lg in logits]) == [[0, 1, 2]]
    for case, z, lg, pr in zip(CASES, zs, logits, probs):
        assert lg.dtype == torch.float32 and pr.shape == lg.shape[2:]
        _check_logits(f"{case} head_batch_f32=4", lg, z)


def test_model_head_batch_f32_fused_prologue():
    z = load_case("tiny")
    gb, pairs = _graph_batch([z])
    with torch.no_grad():
        logits, _ = _model(head_batch_f32=4, fuse_head_prologue=True).predict_batch(gb, pairs)
    _check_logits("tiny head_batch_f32=4 fused prologue", logits[0], z)


def test_model_chunk_boundary_gives_the_same_bits(model_run):
    _, gb, pairs, _, one_chunk, _ = model_run
    model = _model(head_batch_f32=2)
    assert model._head_chunks([tuple(lg.shape[2:]) for lg in one_chunk]) == [[0, 1], [2]]
    with torch.no_grad():
        logits, _ = model.predict_batch(gb, pairs)
    for a, b in zip(logits, one_chunk):
        assert torch.equal(_bits(a), _bits(b))


def test_test_batch_agrees_with_the_single_head():
    """test_batch on two complexes: head_batch_f32=4 returns head_batch_f32=0's keys, and loss and test_auroc
    agree to the project's fp32 bound, 1e-4: the logits of the two paths differ by fp32 rounding in the SE
    gate alone (far below the bound, printed by test_whole_head_batch_against_float64), the loss is a mean of
    log-softmax values, 1-Lipschitz in the logits, and the AUROC moves only where that difference reorders
    two of a complex's probabilities, by 1 / (positives x negatives) a pair."""
    zs = [load_case("tiny"), load_case("c1")]
    gb, pairs = _graph_batch(zs)
    g = torch.Generator().manual_seed(50)
    examples = []
    for z in zs:
        l1, l2 = int(z["logits"].shape[2]), int(z["logits"].shape[3])
        i, j = torch.meshgrid(torch.arange(l1), torch.arange(l2), indexing="ij")
        examples.append(torch.stack((i.flatten(), j.flatten(), (torch.rand(l1 * l2, generator=g) < 0.05).long()), dim=1))
    paths = ["/data/test/4heq_l_u.dill", "/data/test/1abc_r_b.dill"]
    outs = {}
    for n in (4, 0):
        with torch.no_grad():
            outs[n] = _model(head_batch_f32=n).test_batch(gb, pairs, examples, paths, keep_maps=0)
    assert len(outs[4]) == len(outs[0]) == 2
    for a, b in zip(outs[4], outs[0]):
        assert list(a) == list(b) and a["target"] == b["target"]
        print(f"{a['target']}: loss {a['loss']:.9f} / {b['loss']:.9f}, auroc {a['test_auroc']:.9f} / {b['test_auroc']:.9f}")
        assert np.isfinite(a["loss"]) and np.isfinite(a["test_auroc"])
        assert abs(a["loss"] - b["loss"]) <= 1e-4 * abs(b["loss"])
        assert abs(a["test_auroc"] - b["test_auroc"]) <= 1e-4 * abs(b["test_auroc"])
