"""GPU tests of the native head body (di_head_body_batch, di_head_logits_batch, head.HeadBodyPlan,
ResNet2DInputWithOptAttention.body_batch(native=True), LitGINI(head_body="native")).

The body is the Python loop's launches issued from C, so its bar is ``torch.equal`` on the arena buffer
it names. The logits kernel is new arithmetic: exact on integer inputs (every product and partial sum an
integer below 2^8, which bf16 and fp32 hold), and within 2^-8 (sum |w ELU(x)| + |b|) of fp64 on random
inputs -- each a_c = bf16(ELU(x_c)) carries one rounding of 2^-9 relative, the stored result another;
the fp32 sum of 128 terms (<= 128 2^-24 of the same sum) and hc_elu's 1e-6 are far below the
remaining 2^-9. Whole head and model: against the fp32 torch head and the golden logits, with the
Python-issued path as the yardstick and the margin of test_gpu_head_batch.py.

Measured on MI355X: logits kernel 0.375 of its bound; whole head e_native / e_python
48x40 1.650e-2 / 1.650e-2, 17x9 2.013e-2 / 2.013e-2, 70x33 1.720e-2 / 1.720e-2; the model against the golden
logits, native / python: tiny 2.199e-2 / 2.199e-2, c1 2.417e-2 / 2.322e-2.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_common import chain_item, load_case, rel_max

pytestmark = pytest.mark.gpu

BODY_BATCH = [(48, 40), (1, 1), (17, 9), (3, 5), (70, 33)]
LOGIT_BATCH = [(1, 1), (3, 5), (17, 9), (33, 70), (145, 145)]
HEAD_SHAPES = [(48, 40), (17, 9), (70, 33)]


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _head(dtype):
    from deepinteract_amd.head import ResNet2DInputWithOptAttention
    from deepinteract_amd.weights import seeded_state_dict
    sd = seeded_state_dict(0)
    hsd = {k[len("interact_module."):]: v for k, v in sd.items() if k.startswith("interact_module.")}
    m = ResNet2DInputWithOptAttention().cuda().eval()
    m.load_state_dict(hsd)
    return m.to(dtype=dtype)


@pytest.fixture(scope="module")
def hip():
    from deepinteract_amd.head import HeadConvOps, HeadNormOps
    return _head(torch.bfloat16).use_hip_norm_ops(HeadNormOps("cuda")).use_hip_convs(HeadConvOps("cuda"))


@pytest.fixture(scope="module")
def body_inputs():
    g = torch.Generator().manual_seed(11)
    return {s: F.elu(torch.randn(1, 128, *s, generator=g)).to(torch.bfloat16).cuda() for s in BODY_BATCH}


def _python_body(hip, hb):
    x, spare = hip.base_resnet._forward_hipconv_batch(hb, hb.wide[0], hb.wide[1], hip.ops, hip.cops)
    x, _ = hip.phase2_resnet._forward_hipconv_batch(hb, x, spare, hip.ops, hip.cops, in_elu=True)
    return x


# ---- 1. the body's bits
@pytest.fixture(scope="module")
def body_of_five(hip, body_inputs):
    from deepinteract_amd.head import HeadBatch
    hb = HeadBatch(BODY_BATCH, "cuda")
    for i, s in enumerate(BODY_BATCH):
        hb.input(i).copy_(body_inputs[s])
    with torch.no_grad():
        x = _python_body(hip, hb)
    return hb, [hb.view(x, 128, i).clone() for i in range(hb.count)], [w is x for w in hb.wide].index(True)


@pytest.mark.parametrize("order", ["as_listed", "reversed", "one"])
def test_body_bits_equal_the_python_loop(hip, body_inputs, body_of_five, order):
    from deepinteract_amd.head import HeadBatch
    _, want, want_index = body_of_five
    ids = {"as_listed": [0, 1, 2, 3, 4], "reversed": [4, 3, 2, 1, 0], "one": [4]}[order]
    hb = HeadBatch([BODY_BATCH[i] for i in ids], "cuda")
    for buf in (hb.wide[1], hb.half[0], hb.half[1]):     # everything the call must write before it reads
        buf.fill_(float("nan"))
    for slot, i in enumerate(ids):
        hb.input(slot).copy_(body_inputs[BODY_BATCH[i]])
    which = hip.plan().body(hb)
    torch.cuda.synchronize()
    assert which == want_index
    for slot, i in enumerate(ids):
        got = hb.view(hb.wide[which], 128, slot)
        assert bool(torch.isfinite(got.float()).all()), BODY_BATCH[i]
        assert torch.equal(_bits(got), _bits(want[i])), (order, BODY_BATCH[i])
    if order == "as_listed":   # the same batch: the whole packed buffer
        ref_hb = body_of_five[0]
        assert torch.equal(_bits(hb.wide[which]), _bits(ref_hb.wide[want_index]))


# ---- 2. / 3. the logits kernel
def _logits_call(hb, x, w, b, y):
    from deepinteract_amd import _lib
    from deepinteract_amd.engine import _ptr, _stream
    _lib.check(_lib.load().di_head_logits_batch(_lib.DI_BF16, _ptr(x), _ptr(w), _ptr(b), hb.items, hb.items_ptr,
                                                hb.count, y.data_ptr(), _stream()), "di_head_logits_batch")


@pytest.mark.parametrize("shapes", [LOGIT_BATCH, LOGIT_BATCH[::-1]], ids=["largest_last", "largest_first"])
def test_logits_exact_on_integers(shapes):
    from deepinteract_amd.head import HeadBatch
    hb = HeadBatch(shapes, "cuda")
    g = torch.Generator().manual_seed(len(shapes) + shapes[0][0])
    images = [torch.randint(0, 3, (1, 128, h, w), generator=g).to(torch.bfloat16).cuda() for h, w in shapes]
    x = hb.pack(images)
    w = torch.randint(-1, 2, (2, 128), generator=g).float().cuda()
    b = torch.zeros(2).cuda()
    guard = 64
    y = torch.full((2 * hb.pixels + guard,), -7.0, dtype=torch.bfloat16, device="cuda")
    _logits_call(hb, x, w, b, y)
    torch.cuda.synchronize()
    assert torch.equal(y[2 * hb.pixels:], torch.full((guard,), -7.0, dtype=torch.bfloat16, device="cuda"))
    for i, im in enumerate(images):
        want = torch.einsum("oc,chw->ohw", w.double(), im[0].double())
        assert float(want.abs().max()) <= 256
        got = hb.view(y[:2 * hb.pixels], 2, i)[0].double()
        assert torch.equal(got, want), shapes[i]


def test_logits_within_bf16_rounding_of_fp64(hip):
    from deepinteract_amd.head import HeadBatch
    hb = HeadBatch(LOGIT_BATCH, "cuda")
    g = torch.Generator().manual_seed(3)
    images = [(2 * torch.randn(1, 128, h, w, generator=g)).to(torch.bfloat16).cuda() for h, w in LOGIT_BATCH]
    x = hb.pack(images)
    got = hip.plan().logits(hb, x)
    # a second output at an odd 2-byte alignment: the same bits
    y2 = torch.zeros(2 * hb.pixels + 1, dtype=torch.bfloat16, device="cuda")
    plan = hip.plan()
    from deepinteract_amd import _lib
    from deepinteract_amd.engine import _ptr, _stream
    _lib.check(_lib.load().di_head_logits_batch(_lib.DI_BF16, _ptr(x), plan.logit_w, plan.logit_b, hb.items,
                                                hb.items_ptr, hb.count, y2.data_ptr() + 2, _stream()), "logits")
    torch.cuda.synchronize()
    w = hip.phase2_conv.weight.detach().double().view(2, 128)
    b = hip.phase2_conv.bias.detach().double()
    worst = 0.0
    for i, im in enumerate(images):
        a = im[0].double()
        a = torch.where(a > 0, a, torch.expm1(a))                       # ELU, unrounded
        want = torch.einsum("oc,chw->ohw", w, a) + b[:, None, None]
        bound = 2.0 ** -8 * (torch.einsum("oc,chw->ohw", w.abs(), a.abs()) + b.abs()[:, None, None])
        assert got[i].shape == (1, 2) + tuple(LOGIT_BATCH[i]) and got[i].dtype == torch.bfloat16
        ratio = float(((got[i][0].double() - want).abs() / bound).max())
        worst = max(worst, ratio)
        assert torch.equal(_bits(hb.view(y2[1:], 2, i)), _bits(got[i])), LOGIT_BATCH[i]
    print(f"logits kernel: largest |y - y64| / bound = {worst:.3f}")
    assert worst <= 1.0


# ---- 4. the whole body
def test_whole_head_native_no_worse_than_python(hip):
    """e_native <= 2 e_python per complex against the fp32 torch head: the two differ by the logits'
    last step alone (hc_elu and one fp32 sum instead of torch's ELU and MIOpen's bf16 convolution)."""
    g = torch.Generator().manual_seed(0)
    ts = [torch.randn(1, 256, h, w, generator=g).cuda() for h, w in HEAD_SHAPES]
    with torch.no_grad():
        with torch.backends.cudnn.flags(enabled=False):
            f32 = _head(torch.float32)
            refs = [f32(t) for t in ts]
        pro = [hip.ops.inorm_elu(hip.conv2d_1(t.to(torch.bfloat16)), hip.inorm_1) for t in ts]
        python = hip.body_batch(pro)
        native = hip.body_batch(pro, native=True)
    for shape, ref, yp, yn in zip(HEAD_SHAPES, refs, python, native):
        e_python = float((yp.float() - ref).abs().max() / ref.abs().max())
        e_native = float((yn.float() - ref).abs().max() / ref.abs().max())
        print(f"whole head {shape[0]}x{shape[1]}: e_native = {e_native:.3e}, e_python = {e_python:.3e}")
        assert yn.shape == ref.shape and yn.dtype == yp.dtype and bool(torch.isfinite(yn).all())
        assert e_native <= 2 * e_python


# ---- 5. - 7. the model
def _model(sd, **kw):
    from deepinteract_amd.modules import LitGINI
    return LitGINI(dtype="bf16", head_dtype=torch.bfloat16, head_convs="hip", **kw).cuda().eval() \
        .load_reference_state_dict(sd)


def _predict(model, gb, pairs):
    with torch.no_grad():
        logits, _ = model.predict_batch(gb, pairs)
    torch.cuda.synchronize()
    return [lg.detach().clone() for lg in logits]


@pytest.fixture(scope="module")
def model_case():
    from deepinteract_amd.graph import GraphBatch
    from deepinteract_amd.weights import seeded_state_dict
    sd = seeded_state_dict(0)
    zs = [load_case("tiny"), load_case("c1")]
    gb = GraphBatch.from_arrays([chain_item(z, tag) for z in zs for tag in ("g1", "g2")], "cuda")
    pairs = [(0, 1), (2, 3)]
    native = _model(sd, head_batch=4, head_body="native")
    return zs, gb, pairs, native, _predict(native, gb, pairs)


def test_model_native_against_golden(model_case):
    from deepinteract_amd.weights import seeded_state_dict
    zs, gb, pairs, _, native = model_case
    python = _predict(_model(seeded_state_dict(0), head_batch=4, head_body="python"), gb, pairs)
    for i, z in enumerate(zs):
        ln, lp = native[i].float().cpu().numpy(), python[i].float().cpu().numpy()
        assert ln.shape == lp.shape == z["logits"].shape and np.isfinite(ln).all()
        e_native, e_python = rel_max(ln, z["logits"]), rel_max(lp, z["logits"])
        print(f"complex {i}: logits rel err vs golden: native {e_native:.3e}, python {e_python:.3e}")
        assert e_native <= 2 * e_python


def test_model_native_bits_do_not_depend_on_the_chunks(model_case):
    from deepinteract_amd.weights import seeded_state_dict
    _, gb, pairs, model, native = model_case
    one_by_one = _predict(_model(seeded_state_dict(0), head_batch=0, head_body="native"), gb, pairs)
    shapes = [tuple(lg.shape[2:]) for lg in native]
    assert model._head_chunks(shapes) == [[0, 1]]
    model.head_batch_pixels = 3000                      # 48 x 48 fits, 145 x 145 goes alone
    try:
        assert model._head_chunks(shapes) == [[0], [1]]
        capped = _predict(model, gb, pairs)
    finally:
        model.head_batch_pixels = 2 ** 22
    for a, b, c in zip(native, one_by_one, capped):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(c))


def test_model_native_fused_prologue_writes_the_arena(model_case):
    """fuse_head_prologue=True: HeadPrologueOp writes the chunk into the arena's input buffer; the same
    call into a private buffer, copied into the arena, gives the same logits bit for bit."""
    from deepinteract_amd.head import HeadBatch
    from deepinteract_amd.weights import seeded_state_dict
    zs, gb, pairs, _, _ = model_case
    model = _model(seeded_state_dict(0), head_batch=4, head_body="native", fuse_head_prologue=True)
    got = _predict(model, gb, pairs)
    with torch.no_grad():
        eng, _, pro = model._ops()
        h, _ = eng.forward(gb)
        assert h.dtype == torch.bfloat16
        off, n = gb.node_off, gb.nodes_per_graph
        rows = [[off[a] for a, _ in pairs], [off[b] for _, b in pairs], [n[a] for a, _ in pairs],
                [n[b] for _, b in pairs]]
        buf, _ = pro(h, *rows)
        hb = HeadBatch(list(zip(rows[2], rows[3])), "cuda")
        assert buf.numel() == hb.wide[0].numel()
        hb.wide[0].copy_(buf)
        want = model.interact_module.body_batch(hb, native=True)
    torch.cuda.synchronize()
    for i, z in enumerate(zs):
        assert got[i].shape == z["logits"].shape and bool(torch.isfinite(got[i]).all())
        assert torch.equal(_bits(got[i]), _bits(want[i])), i


def test_model_native_reload_rebuilds_the_plan(model_case):
    from deepinteract_amd.weights import seeded_state_dict
    _, gb, pairs, model, native = model_case
    sd1 = seeded_state_dict(1)
    fresh = _predict(_model(sd1, head_batch=4, head_body="native"), gb, pairs)
    try:
        again = _predict(model.load_reference_state_dict(sd1), gb, pairs)
    finally:
        model.load_reference_state_dict(seeded_state_dict(0))
    for a, b, c in zip(again, fresh, native):
        assert torch.equal(_bits(a), _bits(b))
        assert not torch.equal(_bits(a), _bits(c))          # other weights, other logits
    for a, c in zip(_predict(model, gb, pairs), native):    # and back
        assert torch.equal(_bits(a), _bits(c))


def test_model_native_test_batch_figures(model_case):
    """test_batch on the native logits (views of one packed buffer, 2-byte aligned): every top_* figure
    and the confusion counts equal those of the single ContactRankOp on the logits it judged."""
    from deepinteract_amd.ranking import ContactRankOp, topk_metrics
    zs, gb, pairs, model, native = model_case
    g = torch.Generator().manual_seed(50)
    examples = []
    for lg in native:
        l1, l2 = int(lg.shape[2]), int(lg.shape[3])
        i, j = torch.meshgrid(torch.arange(l1), torch.arange(l2), indexing="ij")
        lab = (torch.rand(l1 * l2, generator=g) < 0.05).long()
        examples.append(torch.stack((i.flatten(), j.flatten(), lab), dim=1))
    seen, forward = [], model._forward_batch

    def spy(*args):                  # the logits test_batch judged
        out = forward(*args)
        seen.extend(lg.clone() for lg in out[0])
        return out

    model._forward_batch = spy
    try:
        with torch.no_grad():
            outs = model.test_batch(gb, pairs, examples, ["/data/test/4heq_l_u.dill", "/data/test/1abc_r_b.dill"])
    finally:
        del model._forward_batch
    torch.cuda.synchronize()
    rank = ContactRankOp("cuda")
    assert len(outs) == len(seen) == 2
    for out, lg, ex in zip(outs, seen, examples):
        l1, l2 = int(lg.shape[2]), int(lg.shape[3])
        r = rank(lg.contiguous(), k=min(l1, l2), labels=ex[:, 2].to(torch.uint8).cuda(),
                 threshold=model.pos_prob_threshold)
        want = topk_metrics(r.hits.cpu(), r.num_pos, min(l1, l2))
        assert {k for k in out if k.startswith("top_")} == set(want) and len(want) == 6
        for k, v in want.items():
            assert out[k] == v or (out[k] != out[k] and v != v), k
        assert out["confusion"] == {f: getattr(r, f) for f in ("tp", "fp", "fn", "tn")}
        assert np.array_equal(out["test_preds"], r.probs.cpu().numpy())
