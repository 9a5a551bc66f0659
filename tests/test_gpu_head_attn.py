"""The head's regional attention on the MI355X (csrc/head_attn.hip, head.HeadAttnOps,
ResNet2DInputWithOptAttention(use_attention=True), LitGINI(use_interact_attention=True)) against the
float64 restatement of attn_cases and the reference's fixture tests/golden/attn_head.npz.

Every kernel case runs in fp32 and bf16 on attn_cases.SHAPES: 1x1, strips, an odd plane, several blocks,
and a pixel count on each side of every edge the kernels have (4 / 8 pixels per lane, the scores' 1024-pixel
tile, the mix's 2048-pixel run and 256-pixel element block), so both geometries of both kernels run.

Bounds. Scores: the fp32 dot products' own bound (attn_cases.scores_bound; measured on the MI355X: 0.001 of it
at worst, scores of std 1.33 and |s| up to 9.8). Mix, fp32: 1e-4 normwise, the project's fp32 figure (measured:
4.1e-7 at worst over both score scales). Mix, bf16 (bf16-representable v, the kernel's own scores):
MIX_BF16_BOUND = 6.7e-3, twice the largest figure measured on the MI355X over every shape and both score scales
(3.32e-3, at 16 x the scores; the x1 cases reach 3.1e-3). That figure is the one RNE rounding of the store --
bf16 keeps 8 significant bits, so a value just above a power of two is off by up to 2^-8 = 3.9e-3 of itself --
the fp32 arithmetic in front of it contributes under 1e-6. Far under the project's module bound of 1.6e-2.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attn_cases as A
from gpu_common import chain_item, load_case

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
MIX_F32_BOUND = 1e-4
MIX_BF16_BOUND = 6.7e-3
MODULE_BF16_BOUND = 1.6e-2   # a bf16 module against fp32


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _ids(s):
    return f"{s[0]}x{s[1]}"


@pytest.fixture(scope="module")
def aops():
    from deepinteract_amd.head import HeadAttnOps
    return HeadAttnOps("cuda")


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Per shape, made once on the CPU and left unchanged: x and v (bf16-representable, so both dtypes see
    the same values), wq / wk uniform +-0.25, and the float64 scores with and without the ELU."""
    g = torch.Generator().manual_seed(1000 * shape[0] + shape[1])
    x = torch.randn(128, *shape, generator=g).bfloat16().float()
    v = torch.randn(128, *shape, generator=g).bfloat16().float()
    wq, wk = (torch.rand(16, 128, generator=g) * 0.5 - 0.25 for _ in range(2))
    out = dict(x=x, v=v, wq=wq, wk=wk)
    for elu in (False, True):
        a = F.elu(x.double()) if elu else x.double()
        out["s64", elu] = A.scores64(a, wq.double(), wk.double())
        out["bound", elu] = A.scores_bound(a, wq.double(), wk.double())
    return out


def _img(t, dtype):
    return t[None].to("cuda", dtype).contiguous()


# ---- 1. the border rule ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", A.SHAPES, ids=_ids)
def test_border_rule_counts_the_taps_inside(aops, shape, dtype):
    """scores 0, v = 9: every tap weighs 1/9 and an outside tap brings 0, so y = the number of taps inside
    the image (a kernel that renormalises over the taps inside gives 9 everywhere)."""
    H, W = shape
    v = torch.full((1, 128, H, W), 9.0, dtype=dtype, device="cuda")
    y = aops.mix(v, torch.zeros(4, H, W, device="cuda"))
    torch.cuda.synchronize()
    rows = torch.minimum(torch.arange(H) + 1, torch.tensor(H - 1)) - torch.clamp(torch.arange(H) - 1, min=0) + 1
    cols = torch.minimum(torch.arange(W) + 1, torch.tensor(W - 1)) - torch.clamp(torch.arange(W) - 1, min=0) + 1
    want = (rows[:, None] * cols[None, :]).float()
    assert want.max() <= 9 and want[0, 0] == (1 if H == 1 else 2) * (1 if W == 1 else 2)
    if min(H, W) >= 3:
        assert want[0, 0] == 4 and want[0, 1] == 6 and want[1, 1] == 9
    got = y[0].float().cpu()
    assert float(((got - want[None]).abs() / want[None]).max()) <= 1e-6


# ---- 2. geometry, exact ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 3), (6, 9), (48, 51), (18, 255), (24, 96)], ids=_ids)
def test_geometry_exact(aops, shape, dtype):
    """+200 on the lattice (3i+1, 3j+1), 0 elsewhere: every other tap's exp(-200) is exactly 0 in fp32, so
    y[c, y, x] is v at its 3x3 cell's centre, bit for bit. (24x96: the vector geometry too.)"""
    H, W = shape
    g = torch.Generator().manual_seed(7)
    v = _img(torch.randn(128, H, W, generator=g), dtype)
    s = torch.zeros(4, H, W)
    s[:, 1::3, 1::3] = 200.0
    y = aops.mix(v, s.cuda())
    torch.cuda.synchronize()
    yy, xx = 3 * (torch.arange(H) // 3) + 1, 3 * (torch.arange(W) // 3) + 1
    want = v[0].cpu()[:, yy][:, :, xx]
    assert torch.equal(y[0].cpu(), want)


# ---- 3. scores ------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_elu", [False, True], ids=["plain", "elu"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", A.SHAPES, ids=_ids)
def test_scores_within_the_fp32_bound(aops, shape, dtype, in_elu):
    c = _case(shape)
    s = aops.scores(_img(c["x"], dtype), c["wq"].cuda(), c["wk"].cuda(), in_elu=in_elu)
    torch.cuda.synchronize()
    assert s.shape == (4, *shape) and s.dtype == torch.float32
    err = (s.cpu().double() - c["s64", in_elu]).abs()
    frac = float((err / c["bound", in_elu]).max())
    print(f"scores {shape} {dtype} elu={in_elu}: std {float(c['s64', in_elu].std()) if s.numel() > 4 else 0:.2f}, "
          f"absmax {float(c['s64', in_elu].abs().max()):.2f}, worst error / bound {frac:.3f}")
    assert frac <= 1.0


# ---- 4. mix against float64, fed the kernel's own scores -------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 16.0], ids=["x1", "x16"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", A.SHAPES, ids=_ids)
def test_mix_against_float64(aops, shape, dtype, scale):
    c = _case(shape)
    s = aops.scores(_img(c["x"], dtype), c["wq"].cuda(), c["wk"].cuda()) * scale
    y = aops.mix(_img(c["v"], dtype), s)
    torch.cuda.synchronize()
    want = A.mix64(c["v"].double(), s.cpu().double())
    assert y.dtype == dtype and bool(torch.isfinite(y).all())
    err = float((y[0].cpu().double() - want).abs().max() / want.abs().max())
    bound = MIX_F32_BOUND if dtype == torch.float32 else MIX_BF16_BOUND
    print(f"mix {shape} {dtype} scores x{scale:g} (absmax {float(s.abs().max()):.1f}): normwise {err:.3e}, bound {bound:.3e}")
    assert err <= bound


# ---- 5. the composed block, the batch forms, determinism, a side stream ------------------------------
def _block(aops, a, wq, wk, wv, dtype):
    """scores, v, mix on one block input a [1, 128, H, W] (CPU fp32) in dtype."""
    x = a.to("cuda", dtype).contiguous()
    s = aops.scores(x, wq.cuda().contiguous(), wk.cuda().contiguous())
    v = torch.einsum("oc,bchw->bohw", wv.to("cuda", dtype), x).contiguous()
    return aops.mix(v, s, out=x), s


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("i", [1, 2])
def test_composed_block_against_the_fixture(aops, i, dtype):
    fx = A.fixture()
    y, s = _block(aops, fx[f"block{i}_in"], *A.block_weights(i), dtype)
    torch.cuda.synchronize()
    ref = fx[f"block{i}_out"]
    err = float((y.float().cpu() - ref).abs().max() / ref.abs().max())
    att = A.weights64(s.cpu().double()).permute(1, 0, 2, 3)
    e_att = float((att - fx[f"block{i}_scores"].double()).abs().max())
    print(f"composed block {i} {dtype}: out normwise {err:.3e}, attention weights abs {e_att:.3e}")
    assert err <= (1e-4 if dtype == torch.float32 else MODULE_BF16_BOUND)
    assert e_att <= (1e-4 if dtype == torch.float32 else MODULE_BF16_BOUND)


RAGGED = [(1, 1), (3, 5), (17, 33), (48, 51), (145, 145), (32, 64)]   # both geometries; odd offsets in between


def _batch_raw(aops, hb, dt, es, x, wq, wk, s, v, y, in_elu, stream=None):
    """The two batch calls on packed buffers of either dtype (HeadAttnOps' batch forms take the bf16 arena)."""
    from deepinteract_amd import _lib
    from deepinteract_amd.engine import _stream
    args = _lib.DiRegionAttnArgs(x.data_ptr(), wq.data_ptr(), wk.data_ptr(), s.data_ptr(), v.data_ptr(), y.data_ptr(),
                                 0, 0, int(in_elu))
    st = _stream()
    _lib.check(aops.lib.di_region_scores_batch(dt, ctypes.byref(args), hb.items, hb.items_ptr, hb.count, st), "scores")
    _lib.check(aops.lib.di_region_mix_batch(dt, ctypes.byref(args), hb.items, hb.items_ptr, hb.count, st), "mix")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_batch_forms_equal_the_single_calls(aops, dtype):
    from deepinteract_amd import _lib
    from deepinteract_amd.head import HeadBatch
    dt = _lib.DI_F32 if dtype == torch.float32 else _lib.DI_BF16
    wq, wk = _case((3, 5))["wq"].cuda(), _case((3, 5))["wk"].cuda()
    single = {}
    for shape in RAGGED:
        c = _case(shape) if shape in A.SHAPES else None
        g = torch.Generator().manual_seed(shape[0] * 7 + shape[1])
        x = _img(c["x"] if c else torch.randn(128, *shape, generator=g), dtype)
        v = _img(c["v"] if c else torch.randn(128, *shape, generator=g), dtype)
        s = aops.scores(x, wq, wk, in_elu=True)
        y = aops.mix(v, s)
        s2 = aops.scores(x.clone(), wq, wk, in_elu=True)          # two runs: the same bits
        y2 = aops.mix(v.clone(), s2)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                             # and on a side stream
            s3 = aops.scores(x, wq, wk, in_elu=True)
            y3 = aops.mix(v, s3)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        assert torch.equal(_bits(s), _bits(s2)) and torch.equal(_bits(y), _bits(y2)), shape
        assert torch.equal(_bits(s), _bits(s3)) and torch.equal(_bits(y), _bits(y3)), shape
        single[shape] = (x, v, s, y)
    for order in (RAGGED, RAGGED[::-1]):
        hb = HeadBatch(order, "cuda")
        px = hb.pixels
        xb, vb, yb = (torch.empty(128 * px, dtype=dtype, device="cuda") for _ in range(3))
        sb = torch.empty(4 * px, dtype=torch.float32, device="cuda")
        for i, shape in enumerate(order):
            lo, n = hb.px_off[i], shape[0] * shape[1]
            xb[128 * lo:128 * (lo + n)] = single[shape][0].reshape(-1)
            vb[128 * lo:128 * (lo + n)] = single[shape][1].reshape(-1)
        _batch_raw(aops, hb, dt, xb.element_size(), xb, wq, wk, sb, vb, yb, True)
        if dtype == torch.bfloat16:   # HeadAttnOps' own batch forms, the result written over x
            s_own = aops.scores_batch(hb, xb, wq, wk, in_elu=True, out=torch.empty_like(sb))
            y_own = aops.mix_batch(hb, vb, s_own, xb)
        torch.cuda.synchronize()
        for i, shape in enumerate(order):
            lo, n = hb.px_off[i], shape[0] * shape[1]
            _, _, s1, y1 = single[shape]
            assert torch.equal(_bits(sb[4 * lo:4 * (lo + n)]), _bits(s1.reshape(-1))), (shape, "scores")
            assert torch.equal(_bits(yb[128 * lo:128 * (lo + n)]), _bits(y1.reshape(-1))), (shape, "mix")
            if dtype == torch.bfloat16:
                assert torch.equal(_bits(s_own[4 * lo:4 * (lo + n)]), _bits(s1.reshape(-1))), (shape, "scores_batch")
                assert torch.equal(_bits(y_own[128 * lo:128 * (lo + n)]), _bits(y1.reshape(-1))), (shape, "mix_batch")


def test_ops_refuse_bad_arguments(aops):
    x = torch.zeros(1, 128, 4, 4, device="cuda")
    wq = torch.zeros(16, 128, device="cuda")
    s = torch.zeros(4, 4, 4, device="cuda")
    with pytest.raises(ValueError):
        aops.scores(x[:, :64].contiguous(), wq, wq)
    with pytest.raises(ValueError):
        aops.scores(x, wq.bfloat16(), wq)
    with pytest.raises(TypeError):
        aops.scores(x.half(), wq, wq)
    with pytest.raises(ValueError):
        aops.mix(x, s, out=x)
    with pytest.raises(ValueError):
        aops.mix(x, s[:2].contiguous())
    with pytest.raises(ValueError):
        aops.mix(x.cpu(), s)


# ---- 6. large offsets -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4100, 4100), (8208, 2048)], ids=_ids)
def test_mix_large_offsets_bf16_sampled(aops, shape):
    """128 h w > 2^31 elements (4100x4100: the element geometry, wider than the LDS windows; 8208x2048: the
    vector geometry): ~1000 pixels of the first and last rows and channels against the restatement on their
    3x3 crops (the output depends on nothing else)."""
    H, W = shape
    g = torch.Generator(device="cuda").manual_seed(3)
    v = torch.randn(1, 128, H, W, generator=g, device="cuda", dtype=torch.bfloat16)
    s = torch.randn(4, H, W, generator=g, device="cuda") * 1.3
    y = aops.mix(v, s)
    torch.cuda.synchronize()
    cg = torch.Generator().manual_seed(4)
    n = 1024
    ch = torch.tensor([0, 1, 31, 32, 96, 126, 127])[torch.randint(0, 7, (n,), generator=cg)]
    row = torch.tensor([0, 1, 2, H - 3, H - 2, H - 1])[torch.randint(0, 6, (n,), generator=cg)]
    col = torch.randint(0, W, (n,), generator=cg)
    col[:64] = torch.tensor([0, 1, W - 2, W - 1]).repeat(16)
    ch[:8], row[:8] = torch.tensor([0, 0, 0, 0, 127, 127, 127, 127]), torch.tensor([0, 0, H - 1, H - 1] * 2)
    sc, vc = torch.zeros(n, 9, dtype=torch.float64), torch.zeros(n, 9, dtype=torch.float64)
    chd, hd = ch.cuda(), (ch // 32).cuda()
    for t, (i, j) in enumerate(A.TAPS):
        rr, cc = row + i - 1, col + j - 1
        ok = (rr >= 0) & (rr < H) & (cc >= 0) & (cc < W)
        rc, ccc = rr.clamp(0, H - 1).cuda(), cc.clamp(0, W - 1).cuda()
        sc[:, t] = torch.where(ok, s[hd, rc, ccc].cpu().double(), torch.zeros(()).double())
        vc[:, t] = torch.where(ok, v[0, chd, rc, ccc].cpu().double(), torch.zeros(()).double())
    want = (torch.softmax(sc, 1) * vc).sum(1)
    got = y[0, chd, row.cuda(), col.cuda()].cpu().double()
    err = float((got - want).abs().max() / want.abs().max())
    print(f"mix {H}x{W} bf16, {n} sampled pixels: normwise {err:.3e}")
    assert bool(torch.isfinite(got).all()) and err <= MIX_BF16_BOUND


# ---- 7. the whole head on the fixture's input -------------------------------------------------------
def _head(dtype):
    return A.build_head().cuda().to(dtype)


def test_whole_head_f32_hip_ops_against_the_fixture():
    from deepinteract_amd.head import HeadNormOps
    fx = A.fixture()
    head = _head(torch.float32).use_hip_norm_ops(HeadNormOps("cuda"))
    assert head.aops is not None
    with torch.no_grad(), torch.backends.cudnn.flags(enabled=False):
        y = head(fx["input"].cuda())
    torch.cuda.synchronize()
    ref = fx["logits"]
    err = float((y.cpu() - ref).abs().max() / ref.abs().max())
    print(f"whole fp32 head with attention on HIP vs the reference's logits: {err:.3e}")
    assert err <= 1e-4


def test_whole_head_bf16_hip_no_worse_than_miopen():
    """e_hip <= 2 e_mi against the fp32 head (the form and factor of test_whole_head_no_worse_than_miopen_bf16),
    and e_mi < 0.1: without that the comparison proves nothing (7e-3 on the CPU)."""
    from deepinteract_amd.head import HeadConvOps, HeadNormOps
    fx = A.fixture()
    t = fx["input"].cuda()
    with torch.no_grad():
        with torch.backends.cudnn.flags(enabled=False):
            ref = _head(torch.float32)(t)
        mi = _head(torch.bfloat16).use_hip_norm_ops(HeadNormOps("cuda"))
        y_mi = mi(t.bfloat16()).float()
        hip = _head(torch.bfloat16).use_hip_norm_ops(HeadNormOps("cuda")).use_hip_convs(HeadConvOps("cuda"))
        y_hip = hip(t.bfloat16()).float()
    torch.cuda.synchronize()
    assert float((ref.cpu() - fx["logits"]).abs().max() / fx["logits"].abs().max()) <= 1e-4
    e_mi = float((y_mi - ref).abs().max() / ref.abs().max())
    e_hip = float((y_hip - ref).abs().max() / ref.abs().max())
    print(f"whole bf16 head with attention 11x19: e_hip = {e_hip:.3e}, e_mi = {e_mi:.3e}")
    assert bool(torch.isfinite(y_hip).all()) and e_mi < 0.1
    assert e_hip <= 2 * e_mi


# ---- 8. body_batch ----------------------------------------------------------------------------------
def test_body_batch_with_attention():
    """Three ragged images: an image's logits do not depend on the batch, and against the fp32 torch head the
    batch is no worse than twice the single path (the batched head's fp32 SE gate is its one difference)."""
    from deepinteract_amd.head import HeadConvOps, HeadNormOps
    shapes = [(24, 20), (17, 9), (40, 33)]
    g = torch.Generator().manual_seed(0)
    ts = [torch.randn(1, 256, h, w, generator=g).cuda() for h, w in shapes]
    ops = HeadNormOps("cuda")
    with torch.no_grad():
        with torch.backends.cudnn.flags(enabled=False):
            f32 = _head(torch.float32)
            refs = [f32(t) for t in ts]
        hip = _head(torch.bfloat16).use_hip_norm_ops(ops).use_hip_convs(HeadConvOps("cuda"))
        single = [hip(t.bfloat16()) for t in ts]
        pro = [ops.inorm_elu(hip.conv2d_1(t.bfloat16()), hip.inorm_1) for t in ts]
        three = hip.body_batch(pro)
        ones = [hip.body_batch([x])[0] for x in pro]
        other = hip.body_batch([pro[i] for i in (2, 0, 1)])
        with pytest.raises(RuntimeError, match="native"):
            hip.body_batch(pro, native=True)
    torch.cuda.synchronize()
    for i, (shape, ref) in enumerate(zip(shapes, refs)):
        assert torch.equal(_bits(ones[i]), _bits(three[i])) and torch.equal(_bits(other[(2, 0, 1).index(i)]),
                                                                          _bits(three[i])), shape
        e_hip = float((single[i].float() - ref).abs().max() / ref.abs().max())
        e_batch = float((three[i].float() - ref).abs().max() / ref.abs().max())
        print(f"attention head {shape}: e_batch = {e_batch:.3e}, e_hip = {e_hip:.3e}")
        assert three[i].shape == ref.shape and bool(torch.isfinite(three[i]).all())
        assert e_batch <= 2 * e_hip


# ---- 9. end to end on tiny --------------------------------------------------------------------------
def _residue_graph(z, tag):
    from deepinteract_amd.graph import ResidueGraph
    it = chain_item(z, tag)
    g = ResidueGraph(it["src"], it["dst"], it["num_nodes"])
    g.ndata["f"], g.edata["f"] = it["node_f"], it["edge_f"]
    g.edata["src_nbr_e_ids"], g.edata["dst_nbr_e_ids"] = it["src_nbr"], it["dst_nbr"]
    return g.to("cuda")


def test_model_with_attention_end_to_end_on_tiny():
    """LitGINI(use_interact_attention=True, precise_head=True): the logits against the CPU torch head (pinned
    to the reference by test_head_attn_host.py) run on the model's own pair tensor; test_step's keys."""
    from deepinteract_amd.modules import LitGINI, construct_interact_tensor
    sd = A.attention_state_dict()
    z = load_case("tiny")
    model = LitGINI(use_interact_attention=True, precise_head=True).cuda().eval().load_reference_state_dict(sd)
    with torch.no_grad():
        logits_list, n1, _, n2, _ = model.shared_step(_residue_graph(z, "g1"), _residue_graph(z, "g2"),
                                                      return_representations=True)
        t = construct_interact_tensor(torch.as_tensor(n1).cuda(), torch.as_tensor(n2).cuda())
        want = A.build_head()(t.float().cpu())
    torch.cuda.synchronize()
    got = logits_list[0].float().cpu()
    assert got.shape == want.shape
    worst = float(((got - want).abs() / (1e-4 * want.abs() + 1e-5 * want.abs().max())).max())
    print(f"tiny with attention: worst |got - want| / (1e-4 |want| + 1e-5 max|want|) = {worst:.3f}")
    assert worst <= 1.0
    # not the no-attention network
    assert float((got - torch.as_tensor(z["logits"])).abs().max()) > 1e-2 * float(want.abs().max())
    l1, l2 = got.shape[2:]
    lab = (torch.rand(l1 * l2, generator=torch.Generator().manual_seed(9)) < 0.05).long()
    i, j = torch.meshgrid(torch.arange(l1), torch.arange(l2), indexing="ij")
    examples = torch.stack((i.flatten(), j.flatten(), lab), dim=1)
    with torch.no_grad():
        out = model.test_step((_residue_graph(z, "g1"), _residue_graph(z, "g2"), [examples],
                               ["/data/test/tiny_l_u.dill"]), 0)
    for key in ("loss", "top_10_prec", "top_l_by_10_prec", "top_l_by_5_prec", "top_l_recall", "top_l_by_2_recall",
                "top_l_by_5_recall", "test_preds", "test_preds_rounded", "test_labels", "target", "confusion",
                "test_auroc", "test_auprc", "test_acc", "test_prec", "test_recall", "test_f1"):
        assert key in out, key
    assert np.isfinite(out["test_preds"]).all() and out["test_preds"].shape == (l1, l2)
