"""Example lists on the GPU (csrc/contact_examples.hip, ranking.ExamplesOp, LitGINI.validation_step /
validation_batch, and the routing of labels_from_examples_batch).

Yardsticks, computed here:
* labels: ranking.labels_from_examples_batch_torch on the same device tensors: equal bytes for good
  lists (and no flag raised), the same ValueError text for bad ones;
* gather: torch indexing ``logits[0][:, i, j]`` on the device, bit for bit, and the reference's own
  index line from tests/golden/val_step.npz;
* validation_step: torch.sort(stable=True, descending=True) of the pool's stored map for the ranking,
  ranking.pooled_topk_metrics on that order (pinned to the reference's functions in
  test_examples_host.py), F.cross_entropy in fp64 for the loss within test_gpu_contact_rank's bound,
  test_gpu_contact_auc.against_ref for the two AUCs.
"""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_common import load_case
from test_gpu_contact_auc import against_ref
from test_gpu_contact_rank import ULP, _residue_graph

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
OUTSIDE = "examples: a pair index outside the complex"
LABEL = "examples: labels must be 0 or 1"
TWICE = "examples: a pair is missing or listed twice"


@pytest.fixture(scope="module")
def op():
    from deepinteract_amd.ranking import ExamplesOp
    return ExamplesOp("cuda")


def full_list(l1, l2, seed, order="row", dtype=torch.int64):
    """Every pair of an l1 x l2 complex once, 20 % positives; rows row-major, reversed or shuffled."""
    g = torch.Generator().manual_seed(seed)
    i, j = torch.meshgrid(torch.arange(l1), torch.arange(l2), indexing="ij")
    lab = (torch.rand(l1 * l2, generator=g) < 0.2).long()
    ex = torch.stack((i.flatten(), j.flatten(), lab), dim=1)
    if order == "rev":
        ex = ex.flip(0)
    elif order == "shuf":
        ex = ex[torch.randperm(l1 * l2, generator=g)]
    return ex.to(dtype).contiguous().cuda()


def torch_body(exs, shapes):
    from deepinteract_amd.ranking import labels_from_examples_batch_torch
    return labels_from_examples_batch_torch(exs, shapes)


# the rows one block takes are DI_EX_BLOCK_ROWS = 1024 (1023 = 11 x 93, 1025 = 25 x 41), the rows a wave takes
# at a time 64 (63 = 7 x 9, 65 = 5 x 13)
SHAPES = [(1, 1), (3, 5), (7, 400), (145, 145), (256, 257), (11, 93), (32, 32), (25, 41), (7, 9), (8, 8), (5, 13)]
VARIANTS = [(o, d) for o in ("row", "rev", "shuf") for d in (torch.int64, torch.int32)]


def test_block_and_wave_rows_are_what_the_shapes_assume():
    from deepinteract_amd import _lib
    assert _lib.DI_EX_BLOCK_ROWS == 1024 == 32 * 32 and 11 * 93 == 1023 and 25 * 41 == 1025


@pytest.mark.parametrize("l1,l2", SHAPES)
def test_labels_one_complex_equals_the_torch_body(op, l1, l2):
    for v, (order, dtype) in enumerate(VARIANTS):
        ex = full_list(l1, l2, 10 + v, order, dtype)
        (got,), (want,) = op.labels([ex], [(l1, l2)]), torch_body([ex], [(l1, l2)])   # count = 1
        assert got.dtype == torch.uint8 and tuple(got.shape) == (l1 * l2,)
        assert torch.equal(got, want), (order, dtype)
        assert int(got.sum()) == int(ex[:, 2].sum())
        out, flags, intact = raw_labels(ex, l1, l2)
        assert flags == 0 and intact and torch.equal(out, want), (order, dtype)


def test_labels_mixed_batch(op):
    shapes, exs = [], []
    for s, (l1, l2) in enumerate(SHAPES):
        for v, (order, dtype) in enumerate(VARIANTS):
            shapes.append((l1, l2))
            exs.append(full_list(l1, l2, 100 * s + v, order, dtype))
    want = torch_body(exs, shapes)
    for lists in (exs, [e.int() for e in exs], [e.long() for e in exs], [e.double() for e in exs]):
        got = op.labels(lists, shapes)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert torch.equal(g, w)
            assert g.data_ptr() % 16 == 0 and g.untyped_storage().data_ptr() == got[0].untyped_storage().data_ptr()
    # a strided list is converted first
    wide = torch.zeros(15, 5, dtype=torch.int64, device="cuda")
    wide[:, :3] = exs[6]
    assert not wide[:, :3].is_contiguous()
    assert torch.equal(op.labels([wide[:, :3]], [(3, 5)])[0], want[6])


def test_more_complexes_than_one_launch_takes(op):
    from deepinteract_amd import _lib
    count = _lib.DI_BATCH_MAX + 6
    base = full_list(2, 3, 5, "shuf")
    exs = []
    for c in range(count):
        ex = base.clone()
        ex[:, 2] = (torch.arange(6, device="cuda") + c) % 2
        exs.append(ex)
    got = op.labels(exs, [(2, 3)] * count)
    for c in (0, 1, _lib.DI_BATCH_MAX - 1, _lib.DI_BATCH_MAX, count - 1):
        want = torch.zeros(6, dtype=torch.uint8, device="cuda")
        want[exs[c][:, 0] * 3 + exs[c][:, 1]] = exs[c][:, 2].to(torch.uint8)
        assert torch.equal(got[c], want), c
    exs[count - 2] = exs[count - 2].clone()
    exs[count - 2][0, 2] = 2                  # a fault in the second launch is seen too
    with pytest.raises(ValueError, match=LABEL):
        op.labels(exs, [(2, 3)] * count)


# ---- bad lists
def raw_labels(ex, l1, l2):
    """di_examples_labels_batch on one list, with the map and the workspace each between two 4-KiB
    guard regions of 0xA5: (the map, the flag word, guards intact)."""
    from deepinteract_amd import _lib
    from deepinteract_amd.ranking import _table_to_device
    lib, n, guard = _lib.load(), l1 * l2, 4096
    items = (_lib.DiExamplesItem * 1)()
    it = items[0]
    it.n, it.l1, it.l2 = ex.shape[0], l1, l2
    nb = lib.di_examples_labels_work_bytes(items, 1)
    assert nb > 0 and nb % 16 == 0
    pad = (n + 15) // 16 * 16
    maps = torch.full((guard + pad + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    work = torch.full((guard + nb + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    it.examples, it.labels = ex.data_ptr(), maps.data_ptr() + guard
    idt = {torch.int64: _lib.DI_I64, torch.int32: _lib.DI_I32}[ex.dtype]
    dev = _table_to_device(items, torch.device("cuda", torch.cuda.current_device()))
    rc = lib.di_examples_labels_batch(idt, items, ctypes.c_void_p(dev.data_ptr()), 1,
                                      ctypes.c_void_p(work.data_ptr() + guard),
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    intact = all(bool((t == 0xA5).all()) for t in (maps[:guard], maps[guard + n:], work[:guard], work[guard + nb:]))
    flags = int(work[guard:guard + 4].view(torch.int32)[0])
    return maps[guard:guard + n].clone(), flags, intact


def bad_lists(dtype=torch.int64):
    """name -> (a 7 x 40 list with one fault or two, the flag bits, the message). Every index, wrapped
    to 32 bits or used as it is, stays within 4 KiB of the map and of the bitmap."""
    l1, l2 = 7, 40
    good = full_list(l1, l2, 77, "shuf", dtype)
    row = full_list(l1, l2, 78, "row", dtype)
    cases = {}

    def case(name, base, edits, flags, msg):
        ex = base.clone()
        for r, c, v in edits:
            ex[r, c] = v
        cases[name] = (ex, flags, msg)

    dup = row.clone()
    dup[1, :2] = dup[0, :2]                                # rows 0 and 1 both name pair (0, 0): one bitmap word
    cases["same-word duplicate"] = (dup, 4, TWICE)
    dup = row.clone()
    dup[279, :2] = dup[0, :2]                              # the first and the last row
    cases["far-apart duplicate"] = (dup, 4, TWICE)
    dup = good.clone()
    dup[200, :2] = dup[3, :2]
    cases["shuffled duplicate"] = (dup, 4, TWICE)
    case("i = -1", good, [(5, 0, -1)], 1, OUTSIDE)
    case("i = l1", good, [(5, 0, l1)], 1, OUTSIDE)
    case("j = l2", good, [(5, 1, l2)], 1, OUTSIDE)
    case("j = -1 in a sorted list", row, [(64, 1, -1)], 1, OUTSIDE)
    if dtype == torch.int64:
        case("i = 2**40", good, [(5, 0, 2 ** 40)], 1, OUTSIDE)
        case("j = 2**32 + 1", good, [(9, 1, 2 ** 32 + 1)], 1, OUTSIDE)
    case("label 2", good, [(0, 2, 2)], 2, LABEL)
    case("label -1", good, [(279, 2, -1)], 2, LABEL)
    case("label 256", row, [(100, 2, 256)], 2, LABEL)
    case("outside and label", good, [(5, 0, -1), (6, 2, 2)], 3, OUTSIDE)
    dup = good.clone()
    dup[200, :2] = dup[3, :2]
    dup[7, 2] = 3
    cases["label and duplicate"] = (dup, 6, LABEL)
    return (l1, l2), cases


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_bad_lists_raise_the_torch_bodys_message(op, dtype):
    (l1, l2), cases = bad_lists(dtype)
    before, after = full_list(3, 5, 1, "shuf", dtype), full_list(145, 145, 2, "row", dtype)
    for name, (ex, flags, msg) in cases.items():
        with pytest.raises(ValueError) as want:
            torch_body([ex], [(l1, l2)])
        assert str(want.value) == msg, name
        for lists, shapes in (([ex], [(l1, l2)]), ([before, ex, after], [(3, 5), (l1, l2), (145, 145)])):
            with pytest.raises(ValueError) as got:        # good complexes around it do not mask it
                op.labels(lists, shapes)
            assert str(got.value) == msg, name
    # complexes in order: the first faulty one speaks
    with pytest.raises(ValueError, match=TWICE):
        op.labels([cases["far-apart duplicate"][0], cases["label 2"][0]], [(l1, l2)] * 2)
    with pytest.raises(ValueError, match=LABEL):
        op.labels([cases["label 2"][0], before, cases["i = -1"][0]], [(l1, l2), (3, 5), (l1, l2)])


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_flag_bits_and_outside_rows_touch_nothing(dtype):
    (l1, l2), cases = bad_lists(dtype)
    for name, (ex, flags, _) in cases.items():
        out, got, intact = raw_labels(ex, l1, l2)
        assert got == flags, (name, got)
        assert intact, name
        if flags & 1 and not flags & 4:        # the pair the outside row should have named stays unwritten
            assert int((out == 0xA5).sum()) == 1, name
    # the flags do not depend on the run
    ex = cases["label and duplicate"][0]
    assert {raw_labels(ex, l1, l2)[1] for _ in range(5)} == {6}


def test_argument_errors(op):
    ex = full_list(3, 5, 1)
    with pytest.raises(ValueError, match="tensor on cpu"):
        op.labels([ex.cpu()], [(3, 5)])
    with pytest.raises(ValueError, match=r"\[n, 3\] rows"):
        op.labels([ex[:, :2]], [(3, 5)])
    with pytest.raises(ValueError, match="14 rows for 3 x 5 = 15 pairs"):
        op.labels([ex[:14]], [(3, 5)])
    with pytest.raises(ValueError, match="one \\(l1, l2\\) per complex"):
        op.labels([ex], [])
    lg = torch.zeros(1, 2, 3, 5, device="cuda")
    with pytest.raises(ValueError, match="tensor on cpu"):
        op.gather([lg.cpu()], [ex])
    with pytest.raises(ValueError, match="tensor on cpu"):
        op.gather([lg], [ex.cpu()])
    with pytest.raises(TypeError):
        op.gather([lg.half()], [ex])
    with pytest.raises(TypeError):
        op.gather([lg, lg.bfloat16()], [ex, ex])
    with pytest.raises(ValueError, match="at least one row"):
        op.gather([lg], [ex[:0]])
    with pytest.raises(ValueError, match="exactly one non-empty pool"):
        op.gather([lg, lg], [ex, ex], pools=[[0], [0]])
    with pytest.raises(ValueError, match=OUTSIDE):
        bad = ex.clone()
        bad[3, 1] = 5
        op.gather([lg, lg], [ex, bad])
    with pytest.raises(ValueError, match=LABEL):
        bad = ex.clone()
        bad[3, 2] = 7
        op.gather([lg, lg], [bad, ex])


# ---- gather
def sampled(l1, l2, rows, seed, dtype=torch.int64, repeats=True):
    g = torch.Generator().manual_seed(seed)
    flat = torch.randint(0, l1 * l2, (rows,), generator=g) if repeats else torch.randperm(l1 * l2, generator=g)[:rows]
    lab = (torch.rand(rows, generator=g) < 0.3).long()
    return torch.stack((flat // l2, flat % l2, lab), dim=1).to(dtype).cuda()


def logits_of(l1, l2, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return (4.0 * torch.randn(1, 2, l1, l2, generator=g)).to(dtype).cuda()


def pool_ref(lgs, exs):
    """torch indexing, one complex after another: ([2, N] logits, [N] labels)."""
    cols = [lg[0][:, ex[:, 0].long(), ex[:, 1].long()] for lg, ex in zip(lgs, exs)]
    return torch.cat(cols, dim=1), torch.cat([ex[:, 2] for ex in exs]).to(torch.uint8)


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("idx", [torch.int64, torch.int32])
def test_gather_sampling_rates_of_145(op, dtype, idx):
    lg = logits_of(145, 145, 3, dtype)
    n = 145 * 145
    lists = [sampled(145, 145, rows, 40 + s, idx) for s, rows in enumerate((1, n // 100, n // 10, n, 1023, 1025))]
    lists.append(full_list(145, 145, 9, "row", idx))              # 100 %, every pair once
    got = op.gather([lg] * len(lists), lists)                     # default: one pool per complex
    assert len(got) == len(lists)
    for (pl, lab), ex in zip(got, lists):
        want_lg, want_lab = pool_ref([lg], [ex])
        assert pl.dtype == dtype and tuple(pl.shape) == (1, 2, ex.shape[0], 1) and pl.is_contiguous()
        assert lab.dtype == torch.uint8 and tuple(lab.shape) == (ex.shape[0],)
        assert torch.equal(bits(pl.view(2, -1)), bits(want_lg)) and torch.equal(lab, want_lab)
        assert pl.data_ptr() % 16 == 0 and lab.data_ptr() % 16 == 0
    assert len({tuple(r) for r in lists[3][:, :2].tolist()}) < n   # repeated rows were among them


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gather_pools_of_different_shapes(op, dtype):
    shapes = [(7, 400), (1, 1), (145, 145), (3, 5), (256, 257), (8, 8)]
    rows = [500, 3, 2000, 40, 1, 64]
    lgs = [logits_of(l1, l2, 60 + s, dtype) for s, (l1, l2) in enumerate(shapes)]
    exs = [sampled(l1, l2, r, 70 + s) for s, ((l1, l2), r) in enumerate(zip(shapes, rows))]
    pools = [[4], [2, 0, 3], [5, 1]]                               # three pools in one call, one of three complexes
    got = op.gather(lgs, exs, pools=pools)
    assert len(got) == 3
    for (pl, lab), members in zip(got, pools):
        want_lg, want_lab = pool_ref([lgs[i] for i in members], [exs[i] for i in members])
        assert tuple(pl.shape) == (1, 2, want_lab.numel(), 1)
        assert torch.equal(bits(pl.view(2, -1)), bits(want_lg)) and torch.equal(lab, want_lab)
    # mixed index widths and a float list are converted first
    mixed = [exs[0].int(), exs[1], exs[2].double(), exs[3], exs[4], exs[5]]
    for (pl, lab), (pl2, lab2) in zip(got, op.gather(lgs, mixed, pools=pools)):
        assert torch.equal(bits(pl), bits(pl2)) and torch.equal(lab, lab2)


def test_gather_equals_the_references_index_line(op):
    z = np.load(os.path.join(HERE, "golden", "val_step.npz"))
    lgs, exs, want = [], [], []
    for c in (0, 1):
        l1, l2 = (int(v) for v in z[f"c_{c}_shape"])
        lg = logits_of(l1, l2, 80 + c, torch.float32)
        flat = torch.flatten(lg.squeeze(), start_dim=1)            # the step's own lines, on its own index
        want.append(flat[:, torch.from_numpy(z[f"c_{c}_index"]).cuda()])
        lgs.append(lg)
        exs.append(torch.from_numpy(z[f"c_{c}_examples"]).cuda())
    (pl, lab), = op.gather(lgs, exs, pools=[[0, 1]])
    assert torch.equal(pl.view(2, -1), torch.cat(want, dim=1))
    assert torch.equal(lab.long().cpu(), torch.from_numpy(z["c_labels"]))


def test_pooled_outputs_go_straight_into_the_ranking_and_auc_ops(op):
    from deepinteract_amd.ranking import ContactAucOp, ContactRankOp
    lg, ex = logits_of(145, 145, 5, torch.float32), sampled(145, 145, 3000, 6)
    (pl, lab), = op.gather([lg], [ex])
    r = ContactRankOp("cuda")(pl, k=100, labels=lab)
    idx = torch.sort(r.probs.flatten(), descending=True, stable=True)[1]
    assert tuple(r.probs.shape) == (3000, 1) and torch.equal(r.ids.long(), idx[:100])
    assert r.num_pos == int(ex[:, 2].sum())
    against_ref(ContactAucOp("cuda")(r.probs, lab), r.probs, lab, "a pooled list")


# ---- LitGINI.validation_step / validation_batch
FIGURES = ("top_10_prec", "top_l_by_10_prec", "top_l_by_5_prec", "top_l_recall", "top_l_by_2_recall",
           "top_l_by_5_recall")
KEYS = {"loss", "val_acc", "val_prec", "val_recall", "val_f1", "val_auroc", "val_auprc", "confusion"} | \
    {"val_" + f for f in FIGURES}


@pytest.fixture(scope="module")
def val_run():
    """One model, the c1 and c2 complexes, 2000 sampled rows each (repeats among them, ~5 % positives),
    the logits every call judged, and the outputs of validation_step on c1, on the batch of both, and
    of validation_batch."""
    from deepinteract_amd.graph import GraphBatch, batch as batch_graphs
    from deepinteract_amd.modules import LitGINI
    from deepinteract_amd.weights import seeded_state_dict
    zs = [load_case("c1"), load_case("c2")]
    model = LitGINI(dtype="f32", precise_head=True).cuda().eval().load_reference_state_dict(seeded_state_dict(0))
    exs = []
    for s, z in enumerate(zs):
        l1, l2 = int(z["logits"].shape[2]), int(z["logits"].shape[3])
        ex = sampled(l1, l2, 2000, 90 + s).cpu()
        ex[:, 2] = (torch.rand(2000, generator=torch.Generator().manual_seed(95 + s)) < 0.05).long()
        assert int(ex[:, 2].sum()) >= 10
        exs.append(ex)
    seen, forward = [], model._forward_batch

    def spy(gb, pairs):
        out = forward(gb, pairs)
        seen.append([lg.clone() for lg in out[0]])
        return out

    model._forward_batch = spy
    g = lambda c, tag: _residue_graph(zs[c], tag)   # noqa: E731
    with torch.no_grad():
        one = model.validation_step((g(0, "g1"), g(0, "g2"), [exs[0]], ["/data/val/4heq_l_u.dill"]), 0)
        both = model.validation_step((batch_graphs([g(0, "g1"), g(1, "g1")]), batch_graphs([g(0, "g2"), g(1, "g2")]),
                                      list(exs), ["a", "b"]), 1)
        gb = GraphBatch.from_graphs([g(c, tag) for c in (0, 1) for tag in ("g1", "g2")], device=model.engine.device,
                                    node_count_limit=model.cfg.node_count_limit)
        batched = model.validation_batch(gb, [(0, 1), (2, 3)], exs)
    torch.cuda.synchronize()
    model._forward_batch = forward
    return model, zs, exs, seen, one, both, batched


def check_step(out, lgs, exs, l, model):
    """A validation_step dict against the yardsticks, from the logits the step judged."""
    from deepinteract_amd import _lib
    from deepinteract_amd.ranking import ContactAucOp, ContactRankOp, ExamplesOp, confusion_metrics, pooled_topk_metrics
    assert set(out) == KEYS
    exs = [ex.cuda() for ex in exs]
    want_lg, labels = pool_ref(lgs, exs)
    n = labels.numel()
    (pl, lab), = ExamplesOp("cuda").gather([lg.contiguous() for lg in lgs], exs, pools=[list(range(len(lgs)))])
    assert torch.equal(bits(pl.view(2, -1)), bits(want_lg)) and torch.equal(lab, labels)
    k = min(l, n, _lib.DI_RANK_MAX_K)
    assert l >= 10
    r = ContactRankOp("cuda")(pl, k=k, labels=lab, threshold=model.pos_prob_threshold)
    vals, idx = torch.sort(r.probs.flatten(), descending=True, stable=True)
    assert torch.equal(r.ids.long(), idx[:k])                       # ties by position in the pooled list
    assert torch.equal(r.scores.view(torch.int32), vals[:k].view(torch.int32))
    hits = torch.cumsum(labels[idx[:k]].long(), 0).cpu()
    num_pos = int(labels.sum())
    for name, v in pooled_topk_metrics(hits, num_pos, l, n).items():
        assert out["val_" + name] == v and not math.isnan(v), (name, out["val_" + name], v)
    ce_ref = float(F.cross_entropy(want_lg.double().t(), labels.long(), reduction="mean"))
    dmax = float((want_lg[0].double() - want_lg[1].double()).abs().max())
    err = abs(out["loss"] - ce_ref) / ce_ref
    print(f"validation loss over {n} rows: relative error {err:.3e}, bound {(4 + dmax) * ULP:.3e}")
    assert err <= (4.0 + dmax) * ULP
    pred, pos = r.probs.flatten() >= model.pos_prob_threshold, labels.bool()
    confusion = {"tp": int((pred & pos).sum()), "fp": int((pred & ~pos).sum()), "fn": int((~pred & pos).sum()),
                 "tn": int((~pred & ~pos).sum())}
    assert out["confusion"] == confusion
    for name, v in confusion_metrics(**confusion).items():
        assert out["val_" + name[5:]] == v
    a = ContactAucOp("cuda")(r.probs, lab)
    against_ref(a, r.probs, lab, f"a pool of {n} rows")
    assert (out["val_auroc"], out["val_auprc"]) == (a.auroc, a.auprc)


def test_validation_step_on_c1(val_run):
    model, zs, exs, seen, one, _, _ = val_run
    l1, l2 = (int(v) for v in zs[0]["logits"].shape[2:])
    assert len(seen[0]) == 1 and tuple(seen[0][0].shape) == (1, 2, l1, l2)
    assert len({tuple(r) for r in exs[0][:, :2].tolist()}) < 2000      # repeated rows
    check_step(one, seen[0], exs[:1], l1 + l2, model)


def test_validation_step_pools_a_batch_of_two(val_run):
    model, zs, exs, seen, one, both, _ = val_run
    l = sum(int(v) for z in zs for v in z["logits"].shape[2:])          # graph1.num_nodes() + graph2.num_nodes()
    assert len(seen[1]) == 2
    check_step(both, seen[1], exs, l, model)
    assert sum(both["confusion"].values()) == 4000 and sum(one["confusion"].values()) == 2000


def same(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    if isinstance(a, float):
        return np.float64(a).tobytes() == np.float64(b).tobytes()
    return a == b


def test_validation_batch_equals_validation_step_on_each_complex(val_run):
    model, zs, exs, seen, _, _, batched = val_run
    assert len(batched) == 2 and len(seen[2]) == 2
    for c, out in enumerate(batched):
        l1, l2 = (int(v) for v in zs[c]["logits"].shape[2:])
        check_step(out, [seen[2][c]], [exs[c]], l1 + l2, model)
        # validation_step on that complex alone, on the logits validation_batch judged
        shared = model.shared_step
        model.shared_step = lambda g1, g2, c=c: [seen[2][c]]
        try:
            alone = model.validation_step((_residue_graph(zs[c], "g1"), _residue_graph(zs[c], "g2"), [exs[c]], ["x"]), 0)
        finally:
            model.shared_step = shared
        assert same(out, alone), c
    medians = model.validation_epoch_end(batched)
    assert medians["med_val_auroc"] == min(o["val_auroc"] for o in batched)


# ---- routing
def test_test_batch_gives_the_same_dicts_with_the_op_as_with_the_torch_body(val_run, monkeypatch):
    from deepinteract_amd import modules, ranking
    from deepinteract_amd.graph import GraphBatch
    model, zs = val_run[0], val_run[1]
    shapes = [tuple(int(v) for v in z["logits"].shape[2:]) for z in zs]
    exs = [full_list(l1, l2, 120 + s, "shuf" if s else "row").cpu() for s, (l1, l2) in enumerate(shapes)]
    graphs = [_residue_graph(z, tag) for z in zs for tag in ("g1", "g2")]
    fresh = lambda tag: _residue_graph(zs[0], tag)   # noqa: E731  (shared_step writes its features into the graphs)
    calls = []
    labels = ranking.ExamplesOp.labels
    monkeypatch.setattr(ranking.ExamplesOp, "labels", lambda self, e, s: calls.append(len(e)) or labels(self, e, s))
    with torch.no_grad():
        gb = GraphBatch.from_graphs(graphs, device=model.engine.device, node_count_limit=model.cfg.node_count_limit)
        with_op = model.test_batch(gb, [(0, 1), (2, 3)], exs, ["/d/4heq_l_u.dill", "/d/1abc_r_b.dill"])
        step_op = model.test_step((fresh("g1"), fresh("g2"), [exs[0]], ["/d/4heq_l_u.dill"]), 0)
        assert calls == [2, 1]                                   # both went through the op
        monkeypatch.setattr(modules, "labels_from_examples_batch", ranking.labels_from_examples_batch_torch)
        monkeypatch.setattr(ranking, "labels_from_examples_batch", ranking.labels_from_examples_batch_torch)
        with_torch = model.test_batch(gb, [(0, 1), (2, 3)], exs, ["/d/4heq_l_u.dill", "/d/1abc_r_b.dill"])
        step_torch = model.test_step((fresh("g1"), fresh("g2"), [exs[0]], ["/d/4heq_l_u.dill"]), 0)
        assert calls == [2, 1]                                   # and these did not
    assert len(with_op) == len(with_torch) == 2
    for a, b in zip(with_op + [step_op], with_torch + [step_torch]):
        assert same(a, b)
    assert with_op[0]["test_labels"].sum() == float(exs[0][:, 2].sum())
