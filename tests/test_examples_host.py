"""Example lists without a GPU: the item struct and signatures against the header, every refusal of
di_examples_labels_batch / di_examples_gather_batch before a launch, ranking.pooled_topk_metrics
against the reference's own functions (tests/golden/val_step.npz, made by make_val_golden.py),
LitGINI.validation_epoch_end's medians (also over a two-rank gloo group), and the routing of
labels_from_examples_batch for host tensors."""
import ctypes
import math
import multiprocessing as mp
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

from deepinteract_amd import _lib, ranking
from test_capi import _declared_arg_counts, _declared_struct_fields
from test_distributed import _free_port

EINVAL, ERANGE = -1, -2
P = 16 * 1024            # a dummy non-NULL, 16-B aligned pointer: never dereferenced
HERE = os.path.dirname(os.path.abspath(__file__))
FIGURES = ("top_10_prec", "top_l_by_10_prec", "top_l_by_5_prec", "top_l_recall", "top_l_by_2_recall",
           "top_l_by_5_recall")


def test_item_layout_and_signatures():
    assert [f for f, _ in _lib.DiExamplesItem._fields_] == _declared_struct_fields("di_examples_item")
    assert [t for _, t in _lib.DiExamplesItem._fields_] == \
        [ctypes.c_void_p] * 5 + [ctypes.c_int64] * 4 + [ctypes.c_int32] * 2
    assert ctypes.sizeof(_lib.DiExamplesItem) == 5 * 8 + 4 * 8 + 2 * 4
    decl = _declared_arg_counts()
    for name, n in (("di_examples_labels_work_bytes", 2), ("di_examples_labels_batch", 6),
                    ("di_examples_labels_batch_check", 5), ("di_examples_gather_batch", 7),
                    ("di_examples_gather_batch_check", 6)):
        assert decl[name] == n == len(_lib._SIGS[name][0]), name
    src = open(os.path.join(os.path.dirname(HERE), "include", "deepinteract_amd.h")).read()
    assert "enum { DI_I64 = 0, DI_I32 = 1 };" in src and (_lib.DI_I64, _lib.DI_I32) == (0, 1)
    assert "enum { DI_EX_OUTSIDE = 1, DI_EX_LABEL = 2, DI_EX_TWICE = 4 };" in src
    assert (_lib.DI_EX_OUTSIDE, _lib.DI_EX_LABEL, _lib.DI_EX_TWICE) == (1, 2, 4)
    assert f"#define DI_EX_BLOCK_ROWS {_lib.DI_EX_BLOCK_ROWS} " in src
    assert _lib.load().di_abi_version() == _lib.ABI_VERSION == 8


def label_items(shapes):
    """Good labels-mode items with dummy pointers; shapes: (l1, l2) per complex."""
    items = (_lib.DiExamplesItem * len(shapes))()
    for it, (l1, l2) in zip(items, shapes):
        it.examples = it.labels = P
        it.n, it.l1, it.l2 = l1 * l2, l1, l2
    return items


def gather_items(specs):
    """Good gather-mode items with dummy pointers; specs: (l1, l2, n) per complex, one pool each."""
    items = (_lib.DiExamplesItem * len(specs))()
    for it, (l1, l2, n) in zip(items, specs):
        it.examples = it.logits = it.pool_logits = it.pool_labels = P
        it.n, it.l1, it.l2, it.out_off, it.total = n, l1, l2, 0, n
    return items


def setter(**kw):
    def edit(it):
        for k, v in kw.items():
            setattr(it, k, v)
    return edit


SHAPES = [(1, 1), (3, 5), (145, 145), (7, 400), (300, 300)]
MID = 2


def test_labels_work_bytes_layout():
    lib = _lib.load()
    items = label_items(SHAPES)
    total = lib.di_examples_labels_work_bytes(items, len(items))
    at = (len(SHAPES) * 4 + 15) // 16 * 16          # the flag words, then one bit per pair
    for it, (l1, l2) in zip(items, SHAPES):
        assert it.work_off == at and at % 16 == 0
        at += ((l1 * l2 + 31) // 32 * 4 + 15) // 16 * 16
    assert total == at
    assert lib.di_examples_labels_work_bytes(None, 1) == EINVAL
    assert lib.di_examples_labels_work_bytes(items, 0) == EINVAL
    many = label_items([(2, 2)] * (_lib.DI_BATCH_MAX + 1))
    assert lib.di_examples_labels_work_bytes(many, _lib.DI_BATCH_MAX + 1) == ERANGE
    assert lib.di_examples_labels_work_bytes(many, _lib.DI_BATCH_MAX) > 0
    for edit, rc in ((setter(l1=0), EINVAL), (setter(l2=-1), EINVAL), (setter(n=0), EINVAL),
                     (setter(n=145 * 145 - 1), EINVAL), (setter(l1=1 << 15, l2=1 << 14, n=1 << 29), ERANGE)):
        items = label_items(SHAPES)
        edit(items[MID])
        assert lib.di_examples_labels_work_bytes(items, len(items)) == rc


def test_labels_refusals_without_gpu():
    """Every refusal happens before any launch: the dummy pointers are never dereferenced. The entry
    point and its _check form refuse alike."""
    lib = _lib.load()
    p = ctypes.c_void_p(P)

    def call(edit=None, idt=_lib.DI_I64, count=None, host=True, dev=p, work=p, shapes=SHAPES):
        items = label_items(shapes)
        assert lib.di_examples_labels_work_bytes(items, len(items)) > 0
        if edit:
            edit(items[MID])
        args = (idt, items if host else None, dev, len(items) if count is None else count, work)
        rc = lib.di_examples_labels_batch_check(*args)
        if rc != 0:      # a good call would launch
            assert lib.di_examples_labels_batch(*args, None) == rc
        return rc

    assert call() == 0 and call(idt=_lib.DI_I32) == 0
    assert call(count=0) == EINVAL and call(count=-2) == EINVAL
    assert call(host=False) == EINVAL and call(dev=None) == EINVAL and call(work=None) == EINVAL
    assert call(work=ctypes.c_void_p(P + 8)) == EINVAL
    many = label_items([(2, 2)] * (_lib.DI_BATCH_MAX + 1))
    assert lib.di_examples_labels_batch_check(_lib.DI_I64, many, p, _lib.DI_BATCH_MAX + 1, p) == ERANGE
    assert lib.di_examples_labels_batch(_lib.DI_I64, many, p, _lib.DI_BATCH_MAX + 1, p, None) == ERANGE
    assert call(idt=2) == EINVAL and call(idt=-1) == EINVAL
    for kw in (dict(examples=None), dict(labels=None), dict(n=0), dict(n=-5), dict(l1=0), dict(l2=0), dict(l1=-3),
               dict(n=145 * 145 - 1), dict(n=145 * 145 + 1), dict(l1=144)):
        assert call(setter(**kw)) == EINVAL, kw
    # examples off the index width's alignment
    assert call(setter(examples=P + 4)) == EINVAL and call(setter(examples=P + 4), idt=_lib.DI_I32) == 0
    assert call(setter(examples=P + 2), idt=_lib.DI_I32) == EINVAL
    assert call(setter(l1=1 << 15, l2=1 << 14, n=1 << 29)) == ERANGE
    assert call(setter(l1=(1 << 31) - 1, l2=(1 << 31) - 1, n=((1 << 31) - 1) ** 2)) == ERANGE
    # offsets the helper did not fill
    assert call(setter(work_off=0)) == EINVAL and call(setter(work_off=1 << 20)) == EINVAL
    assert call(setter(l1=29, l2=725, n=145 * 145)) == 0          # the same pair count: the same layout
    assert call(setter(l1=100, l2=100, n=10000)) == EINVAL         # sizes changed after the layout was made


def test_gather_refusals_without_gpu():
    lib = _lib.load()
    p = ctypes.c_void_p(P)
    specs = [(1, 1, 1), (3, 5, 40), (145, 145, 2000), (7, 400, 1), (300, 300, 90000)]

    def call(edit=None, dt=_lib.DI_F32, idt=_lib.DI_I64, count=None, host=True, dev=p, flags=p):
        items = gather_items(specs)
        if edit:
            edit(items[MID])
        args = (dt, idt, items if host else None, dev, len(items) if count is None else count, flags)
        rc = lib.di_examples_gather_batch_check(*args)
        if rc != 0:
            assert lib.di_examples_gather_batch(*args, None) == rc
        return rc

    assert call() == 0 and call(dt=_lib.DI_BF16, idt=_lib.DI_I32) == 0
    assert call(count=0) == EINVAL and call(count=-1) == EINVAL
    assert call(host=False) == EINVAL and call(dev=None) == EINVAL and call(flags=None) == EINVAL
    assert call(flags=ctypes.c_void_p(P + 2)) == EINVAL
    many = gather_items([(2, 2, 3)] * (_lib.DI_BATCH_MAX + 1))
    assert lib.di_examples_gather_batch_check(_lib.DI_F32, _lib.DI_I64, many, p, _lib.DI_BATCH_MAX + 1, p) == ERANGE
    assert lib.di_examples_gather_batch(_lib.DI_F32, _lib.DI_I64, many, p, _lib.DI_BATCH_MAX + 1, p, None) == ERANGE
    assert call(dt=2) == EINVAL and call(dt=-1) == EINVAL and call(idt=2) == EINVAL and call(idt=-1) == EINVAL
    for name in ("examples", "logits", "pool_logits", "pool_labels"):
        assert call(setter(**{name: None})) == EINVAL, name
    for kw in (dict(n=0), dict(n=-1), dict(l1=0), dict(l2=0), dict(l2=-7)):
        assert call(setter(**kw)) == EINVAL, kw
    assert call(setter(logits=P + 2)) == EINVAL and call(setter(logits=P + 2), dt=_lib.DI_BF16) == 0
    assert call(setter(pool_logits=P + 1), dt=_lib.DI_BF16) == EINVAL
    assert call(setter(examples=P + 4)) == EINVAL
    # rows outside the pool
    for kw in (dict(out_off=-1), dict(out_off=1), dict(total=1999), dict(total=0), dict(out_off=5000, total=6999),
               dict(out_off=1 << 40, total=2000)):
        assert call(setter(**kw)) == EINVAL, kw
    assert call(setter(out_off=5000, total=7000)) == 0 and call(setter(total=1 << 20)) == 0
    assert call(setter(l1=1 << 15, l2=1 << 14)) == ERANGE
    assert call(setter(total=1 << 31)) == ERANGE and call(setter(out_off=(1 << 31) - 2000, total=1 << 31)) == ERANGE


# ---- the top-k arithmetic of validation_step
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "val_step.npz"))


def pool_of(z, name):
    scores, labels, l = torch.from_numpy(z[f"{name}_scores"]), torch.from_numpy(z[f"{name}_labels"]), int(z[f"{name}_l"])
    return scores, labels, l, z[f"{name}_figures"]


def hits_of(scores, labels, k):
    order = torch.sort(scores, descending=True, stable=True)[1]
    return torch.cumsum(labels[order[:k]], 0)


def same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def test_pooled_topk_metrics_against_the_reference(golden):
    names = [str(n) for n in golden["pools"]]
    assert names == ["a", "b", "c", "d", "e"]
    for name in names:
        scores, labels, l, want = pool_of(golden, name)
        n = scores.numel()
        assert len(set(scores.tolist())) == n            # no ties: the reference's order is defined
        k = min(max(l, 10), n, _lib.DI_RANK_MAX_K)       # the ranks validation_step keeps
        got = ranking.pooled_topk_metrics(hits_of(scores, labels, k), int(labels.sum()), l, n)
        assert tuple(got) == FIGURES
        for fig, w in zip(FIGURES, want):
            assert same(got[fig], float(w)), (name, fig, got[fig], float(w))
    # what the pools are there for
    _, labels, l, want = pool_of(golden, "b")
    assert l // 10 == 0 and math.isnan(want[1]) and labels.numel() < 10 and labels.numel() < l
    assert want[0] == int(labels.sum()) / 10             # k > N: all rows taken, precision still divides by k
    assert want[3] == 1.0                                # k = l > N: every positive is in the slice
    _, labels, _, want = pool_of(golden, "d")
    assert int(labels.sum()) == 0 and all(math.isnan(w) for w in want[3:]) and want[0] == 0.0
    assert len(golden["c_0_examples"]) + len(golden["c_1_examples"]) == len(golden["c_labels"])
    for c in (0, 1):                                     # repeated rows, and the step's index line
        ex, (l1, l2) = golden[f"c_{c}_examples"], golden[f"c_{c}_shape"]
        assert len({(i, j) for i, j, _ in ex.tolist()}) < len(ex)
        assert np.array_equal(golden[f"c_{c}_index"], ex[:, 0] * l2 + ex[:, 1]) and ex[:, 0].max() < l1


def test_pooled_topk_metrics_edges():
    m = ranking.pooled_topk_metrics
    hits = [0, 1, 1, 2]
    got = m(hits, 2, 4, 4)                 # 10 > N = 4: all four rows, over 10; l // 10 = l // 5 = 0
    assert got["top_10_prec"] == 2 / 10 and math.isnan(got["top_l_by_10_prec"]) and math.isnan(got["top_l_by_5_prec"])
    assert got["top_l_recall"] == 1.0 and got["top_l_by_2_recall"] == 0.5 and math.isnan(got["top_l_by_5_recall"])
    got = m([0] * 10, 0, 20, 50)           # no positives: recalls NaN, precisions 0
    assert got["top_10_prec"] == 0.0 and got["top_l_by_10_prec"] == 0.0
    assert all(math.isnan(got[f]) for f in FIGURES[3:])
    # the ranking is cut at DI_RANK_MAX_K = 4096: k and N both past it give NaN, k alone past it takes all rows
    K = _lib.DI_RANK_MAX_K
    hits = list(range(1, K + 1))
    got = m(hits, 5000, 5 * (K + 1), 6000)
    assert math.isnan(got["top_l_recall"]) and math.isnan(got["top_l_by_2_recall"]) and math.isnan(got["top_l_by_5_prec"])
    assert got["top_l_by_10_prec"] == 1.0 and got["top_10_prec"] == 1.0      # l // 10 = 2048 <= K
    got = m(hits, K, 5 * (K + 1), K)       # N = K: the slice takes the whole pool
    assert got["top_l_recall"] == 1.0 and got["top_l_by_5_prec"] == K / (K + 1)
    got = m(hits, 5000, K, 6000)           # k = K exactly is still ranked
    assert got["top_l_recall"] == K / 5000
    got = m(hits[:5], 9, 40, 100)          # fewer ranks kept than k asks for
    assert math.isnan(got["top_10_prec"]) and got["top_l_by_10_prec"] == 4 / 4 and math.isnan(got["top_l_recall"])


# ---- validation_epoch_end
NAMES = ("val_acc", "val_prec", "val_recall", "val_f1", "val_auroc", "val_auprc")


def hand_outputs(count, seed):
    g = torch.Generator().manual_seed(seed)
    return [dict(zip(NAMES, torch.rand(6, generator=g, dtype=torch.float64).tolist()), loss=0.5) for _ in range(count)]


@pytest.fixture(scope="module")
def model():
    from deepinteract_amd.modules import LitGINI
    return LitGINI(num_interact_layers=1)


@pytest.mark.parametrize("count", [1, 4, 5])
def test_validation_epoch_end_medians(model, count):
    outs = hand_outputs(count, count)
    got = model.validation_epoch_end(outs)
    assert set(got) == {"med_" + n for n in NAMES}
    for n in NAMES:
        vals = [o[n] for o in outs]
        assert got["med_" + n] == float(torch.median(torch.tensor(vals, dtype=torch.float64)))
        assert got["med_" + n] == sorted(vals)[(count - 1) // 2]       # the lower middle value
    outs[0]["val_auroc"] = float("nan")
    got = model.validation_epoch_end(outs)
    assert math.isnan(got["med_val_auroc"]) and not math.isnan(got["med_val_auprc"])
    with pytest.raises(ValueError, match="validation_epoch_end"):
        model.validation_epoch_end([])
    with pytest.raises(ValueError, match="test_epoch_end"):
        model.test_epoch_end([])


def _worker_epoch_end(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from deepinteract_amd.modules import LitGINI
        outs = hand_outputs(4, 21)
        mine = outs[:3] if rank == 0 else outs[3:]
        q.put((rank, LitGINI(num_interact_layers=1).validation_epoch_end(mine, group=dist.group.WORLD)))
    finally:
        dist.destroy_process_group()


def test_validation_epoch_end_two_rank_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_epoch_end, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    outs = hand_outputs(4, 21)
    want = {"med_" + n: float(torch.median(torch.tensor([o[n] for o in outs], dtype=torch.float64))) for n in NAMES}
    assert res[0] == want and res[1] == want


# ---- routing
def test_host_lists_take_the_torch_body(monkeypatch):
    def boom(self, device="cuda"):
        raise AssertionError("ExamplesOp built for host tensors")

    monkeypatch.setattr(ranking.ExamplesOp, "__init__", boom)
    i, j = torch.meshgrid(torch.arange(5), torch.arange(7), indexing="ij")
    lab = (torch.arange(35) % 4 == 0).long()
    ex = torch.stack((i.flatten(), j.flatten(), lab), dim=1)[torch.randperm(35, generator=torch.Generator().manual_seed(1))]
    got = ranking.labels_from_examples_batch([ex, ex.int()], [(5, 7), (5, 7)])
    want = ranking.labels_from_examples_batch_torch([ex, ex.int()], [(5, 7), (5, 7)])
    assert all(torch.equal(a, b) and a.dtype == torch.uint8 for a, b in zip(got, want))
    assert torch.equal(got[0].view(5, 7), lab.view(5, 7).to(torch.uint8))
    assert torch.equal(ranking.labels_from_examples(ex, 5, 7), got[0])
    assert ranking.labels_from_examples_batch([], []) == []
    dup = ex.clone()
    dup[1] = dup[0]
    with pytest.raises(ValueError, match="missing or listed twice"):
        ranking.labels_from_examples_batch([ex, dup], [(5, 7), (5, 7)])
