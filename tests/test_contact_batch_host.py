"""Batched contact ranking / AUC without a GPU: the item structs against the header, the layout the
*_batch_work_bytes helpers fill, every refusal of di_contact_rank_batch / di_contact_auc_batch before
a launch, LitGINI.test_epoch_end's medians and CSV (also over a two-rank gloo group), and
ranking.labels_from_examples_batch against the single function."""
import ctypes
import math
import multiprocessing as mp
import os

import pytest
import torch
import torch.distributed as dist

from deepinteract_amd import _lib
from test_capi import _declared_arg_counts, _declared_struct_fields
from test_distributed import _free_port

EINVAL, ERANGE = -1, -2
P = 16 * 1024            # a dummy non-NULL, 16-B aligned pointer: never dereferenced
RANK_HDR = 3 * 2048 * 4 + 5 * 8 + 3 * 2 * 4    # csrc/contact_rank.hip RankHdr


def test_item_layouts_and_signatures():
    assert [f for f, _ in _lib.DiRankItem._fields_] == _declared_struct_fields("di_rank_item")
    assert [f for f, _ in _lib.DiAucItem._fields_] == _declared_struct_fields("di_auc_item")
    assert ctypes.sizeof(_lib.DiRankItem) == 7 * 8 + 2 * 8 + 4 * 4
    assert ctypes.sizeof(_lib.DiAucItem) == 3 * 8 + 4 * 8
    assert [t for _, t in _lib.DiRankItem._fields_] == [ctypes.c_void_p] * 7 + [ctypes.c_int64] * 2 + [ctypes.c_int32] * 4
    assert [t for _, t in _lib.DiAucItem._fields_] == [ctypes.c_void_p] * 3 + [ctypes.c_int64] * 4
    decl = _declared_arg_counts()
    for name, n in (("di_contact_rank_batch", 7), ("di_contact_rank_batch_work_bytes", 2),
                    ("di_contact_auc_batch", 5), ("di_contact_auc_batch_work_bytes", 2)):
        assert decl[name] == n == len(_lib._SIGS[name][0]), name
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                            "deepinteract_amd.h")).read()
    assert "#define DI_BATCH_MAX 1024" in src and _lib.DI_BATCH_MAX == 1024
    assert _lib.load().di_abi_version() == _lib.ABI_VERSION == 8


def rank_items(shapes, labels=False):
    """Good items with dummy pointers; shapes: (l1, l2, k) per complex."""
    items = (_lib.DiRankItem * len(shapes))()
    for it, (l1, l2, k) in zip(items, shapes):
        it.logits = it.probs = it.top_ids = it.top_scores = P
        if labels:
            it.labels = it.top_hits = it.metrics = P
        it.l1, it.l2, it.k = l1, l2, k
    return items


def auc_items(sizes):
    """Good items with dummy pointers; sizes: (n, max_pos) per complex."""
    items = (_lib.DiAucItem * len(sizes))()
    for it, (n, max_pos) in zip(items, sizes):
        it.probs = it.labels = it.out = P
        it.n, it.max_pos = n, max_pos
    return items


RANK_SHAPES = [(1, 1, 1), (3, 5, 15), (145, 145, 145), (7, 400, 7), (300, 300, 300), (4096, 4096, 4096)]
AUC_SIZES = [(1, 1), (15, 15), (145 * 145, 145 * 145), (90000, 65536), (90000, 4097), (4096 * 4096, 1 << 20)]


def test_rank_batch_work_bytes_layout():
    lib = _lib.load()
    items = rank_items(RANK_SHAPES)
    total = lib.di_contact_rank_batch_work_bytes(items, len(items))
    single = [lib.di_contact_rank_work_bytes(l1 * l2, k) for l1, l2, k in RANK_SHAPES]
    assert total >= sum(single) > 0
    spans = []
    for i, (it, nb) in enumerate(zip(items, single)):
        assert it.hdr_off % 16 == 0 and it.work_off % 16 == 0
        assert it.hdr_off == i * RANK_HDR              # the cleared headers: contiguous at the front
        spans += [(it.hdr_off, it.hdr_off + RANK_HDR), (it.work_off, it.work_off + nb - RANK_HDR)]
    spans.sort()
    assert spans[0][0] == 0 and spans[-1][1] <= total
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    # a batch of one is the single call's size (rounded up to 16 B)
    one = rank_items([(145, 145, 145)])
    assert lib.di_contact_rank_batch_work_bytes(one, 1) == (single[2] + 15) // 16 * 16
    # refusals
    assert lib.di_contact_rank_batch_work_bytes(None, 1) == EINVAL
    assert lib.di_contact_rank_batch_work_bytes(items, 0) == EINVAL
    assert lib.di_contact_rank_batch_work_bytes(items, -1) == EINVAL
    many = rank_items([(8, 8, 8)] * (_lib.DI_BATCH_MAX + 1))
    assert lib.di_contact_rank_batch_work_bytes(many, _lib.DI_BATCH_MAX + 1) == ERANGE
    assert lib.di_contact_rank_batch_work_bytes(many, _lib.DI_BATCH_MAX) > 0
    for bad, rc in (((0, 5, 1), EINVAL), ((5, -1, 1), EINVAL), ((5, 5, 0), EINVAL), ((3, 3, 10), EINVAL),
                    ((100, 100, 4097), ERANGE), ((1 << 15, 1 << 14, 10), ERANGE)):
        shapes = RANK_SHAPES[:3] + [bad] + RANK_SHAPES[3:]
        assert lib.di_contact_rank_batch_work_bytes(rank_items(shapes), len(shapes)) == rc, bad


def test_auc_batch_work_bytes_layout():
    lib = _lib.load()
    items = auc_items(AUC_SIZES)
    total = lib.di_contact_auc_batch_work_bytes(items, len(items))
    single = [lib.di_contact_auc_work_bytes(n, m) for n, m in AUC_SIZES]
    assert total >= sum(single) > 0
    clear = [48 + 2 * 4 * ((m + 1 + 3) // 4 * 4) for _, m in AUC_SIZES]     # AucHdr + eq + gap
    spans, at = [], 0
    for it, nb, cb in zip(items, single, clear):
        assert it.hdr_off % 16 == 0 and it.work_off % 16 == 0
        assert it.hdr_off == at                        # the cleared parts: contiguous at the front
        at += cb
        spans += [(it.hdr_off, it.hdr_off + cb), (it.work_off, it.work_off + nb - cb)]
    assert min(it.work_off for it in items) == at
    spans.sort()
    assert spans[0][0] == 0 and spans[-1][1] <= total
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert lib.di_contact_auc_batch_work_bytes(auc_items([(90000, 4097)]), 1) == single[4]
    assert lib.di_contact_auc_batch_work_bytes(None, 1) == EINVAL
    assert lib.di_contact_auc_batch_work_bytes(items, 0) == EINVAL
    many = auc_items([(64, 64)] * (_lib.DI_BATCH_MAX + 1))
    assert lib.di_contact_auc_batch_work_bytes(many, _lib.DI_BATCH_MAX + 1) == ERANGE
    assert lib.di_contact_auc_batch_work_bytes(many, _lib.DI_BATCH_MAX) > 0
    for bad, rc in (((0, 1), EINVAL), ((10, 0), EINVAL), ((10, 11), EINVAL), ((1 << 29, 10), ERANGE)):
        sizes = AUC_SIZES[:3] + [bad] + AUC_SIZES[3:]
        assert lib.di_contact_auc_batch_work_bytes(auc_items(sizes), len(sizes)) == rc, bad


def test_rank_batch_refusals_without_gpu():
    """Every refusal happens before any launch: the dummy pointers are never dereferenced."""
    lib = _lib.load()
    thr, p, odd = ctypes.c_float(0.5), ctypes.c_void_p(P), ctypes.c_void_p(P + 8)
    shapes = RANK_SHAPES[:5]
    mid = 2

    def call(edit=None, labels=False, dtype=_lib.DI_F32, count=None, host=True, dev=p, threshold=thr, work=p,
             shapes=shapes):
        items = rank_items(shapes, labels)
        assert lib.di_contact_rank_batch_work_bytes(items, len(items)) > 0
        if edit:
            edit(items[mid])
        return lib.di_contact_rank_batch(dtype, items if host else None, dev, len(items) if count is None else count,
                                         threshold, work, None)

    def setter(**kw):
        def edit(it):
            for k, v in kw.items():
                setattr(it, k, v)
        return edit

    assert call(count=0) == EINVAL and call(count=-2) == EINVAL
    assert call(host=False) == EINVAL and call(dev=None) == EINVAL
    many = rank_items([(8, 8, 8)] * (_lib.DI_BATCH_MAX + 1))
    assert lib.di_contact_rank_batch(_lib.DI_F32, many, p, _lib.DI_BATCH_MAX + 1, thr, p, None) == ERANGE
    # one bad item in the middle of good ones, for each refusal of the single call
    for kw in (dict(l1=0), dict(l2=0), dict(l1=-3), dict(k=0), dict(k=-1), dict(l1=3, l2=3, k=10)):
        assert call(setter(**kw)) == EINVAL, kw
    assert call(dtype=2) == EINVAL and call(dtype=-1) == EINVAL
    for name in ("logits", "probs", "top_ids", "top_scores"):
        assert call(setter(**{name: None})) == EINVAL, name
    assert call(work=None) == EINVAL
    for kw in (dict(labels=P), dict(top_hits=P), dict(metrics=P), dict(labels=P, top_hits=P),
               dict(labels=P, metrics=P), dict(top_hits=P, metrics=P)):
        assert call(setter(**kw)) == EINVAL, kw
    for name in ("labels", "top_hits", "metrics"):
        assert call(setter(**{name: None}), labels=True) == EINVAL, name
    # labels for every complex or for none: one kernel variant serves the batch
    assert call(setter(labels=None, top_hits=None, metrics=None), labels=True) == EINVAL
    assert call(setter(labels=P, top_hits=P, metrics=P)) == EINVAL
    assert call(threshold=ctypes.c_float(float("nan"))) == EINVAL
    assert call(setter(probs=P + 8)) == EINVAL and call(work=odd) == EINVAL
    assert call(setter(l1=100, l2=100, k=4097)) == ERANGE
    assert call(setter(l1=1 << 15, l2=1 << 14)) == ERANGE
    assert call(setter(l1=(1 << 31) - 1, l2=(1 << 31) - 1)) == ERANGE
    assert call(setter(l1=10, l2=10, k=5000)) == EINVAL
    # offsets the helper did not fill
    assert call(setter(hdr_off=0)) == EINVAL and call(setter(work_off=16)) == EINVAL
    assert call(setter(k=100)) == EINVAL           # sizes changed after the layout was made


def test_auc_batch_refusals_without_gpu():
    lib = _lib.load()
    p, odd = ctypes.c_void_p(P), ctypes.c_void_p(P + 8)
    sizes = AUC_SIZES[:5]
    mid = 2

    def call(edit=None, count=None, host=True, dev=p, work=p):
        items = auc_items(sizes)
        assert lib.di_contact_auc_batch_work_bytes(items, len(items)) > 0
        if edit:
            edit(items[mid])
        return lib.di_contact_auc_batch(items if host else None, dev, len(items) if count is None else count, work,
                                        None)

    def setter(**kw):
        def edit(it):
            for k, v in kw.items():
                setattr(it, k, v)
        return edit

    assert call(count=0) == EINVAL and call(count=-1) == EINVAL
    assert call(host=False) == EINVAL and call(dev=None) == EINVAL
    many = auc_items([(64, 64)] * (_lib.DI_BATCH_MAX + 1))
    assert lib.di_contact_auc_batch(many, p, _lib.DI_BATCH_MAX + 1, p, None) == ERANGE
    for kw in (dict(n=0), dict(n=-1), dict(max_pos=0), dict(max_pos=145 * 145 + 1)):
        assert call(setter(**kw)) == EINVAL, kw
    for name in ("probs", "labels", "out"):
        assert call(setter(**{name: None})) == EINVAL, name
    assert call(work=None) == EINVAL
    assert call(setter(probs=P + 8)) == EINVAL and call(work=odd) == EINVAL
    assert call(setter(n=1 << 29)) == ERANGE
    assert call(setter(hdr_off=16)) == EINVAL and call(setter(work_off=0)) == EINVAL
    assert call(setter(max_pos=100)) == EINVAL     # sizes changed after the layout was made


# ---- test_epoch_end
NAMES = ("test_acc", "test_prec", "test_recall", "test_f1", "test_auroc", "test_auprc")
TOPK = ("top_10_prec", "top_l_by_10_prec", "top_l_by_5_prec", "top_l_recall", "top_l_by_2_recall",
        "top_l_by_5_recall")


def hand_outputs(count, seed, first=0):
    g = torch.Generator().manual_seed(seed)
    outs = []
    for i in range(count):
        vals = torch.rand(12, generator=g, dtype=torch.float64).tolist()
        out = dict(zip(NAMES + TOPK, vals))
        out["target"] = f"t{first + i:03d}"
        out["test_preds"] = None
        outs.append(out)
    return outs


@pytest.fixture(scope="module")
def model():
    from deepinteract_amd.modules import LitGINI
    return LitGINI(num_interact_layers=1)


@pytest.mark.parametrize("count", [1, 4, 5])
def test_epoch_end_medians_are_torch_median(model, count):
    outs = hand_outputs(count, count)
    got = model.test_epoch_end(outs)
    assert set(got) == {"med_" + n for n in NAMES}
    for n in NAMES:
        vals = [o[n] for o in outs]
        assert got["med_" + n] == float(torch.median(torch.tensor(vals, dtype=torch.float64)))
        if count == 4:
            assert got["med_" + n] == sorted(vals)[1]       # the lower middle value
        if count == 5:
            assert got["med_" + n] == sorted(vals)[2]


def test_epoch_end_nan_propagates(model):
    outs = hand_outputs(5, 7)
    outs[3]["test_auroc"] = float("nan")
    got = model.test_epoch_end(outs)
    assert math.isnan(got["med_test_auroc"])
    assert got["med_test_auprc"] == sorted(o["test_auprc"] for o in outs)[2]
    with pytest.raises(ValueError):
        model.test_epoch_end([])


def test_epoch_end_csv(model, tmp_path):
    outs = hand_outputs(3, 11)
    outs[1]["top_l_by_10_prec"] = float("nan")
    outs[2]["top_10_prec"] = 0.5
    path = tmp_path / "top_metrics.csv"
    model.test_epoch_end(outs, csv_path=str(path))
    lines = path.read_text().split("\n")
    assert lines[-1] == "" and len(lines) == 5
    assert lines[0] == "," + ",".join(TOPK + ("target",))      # DataFrame.to_csv: an unnamed index column
    for i, (line, o) in enumerate(zip(lines[1:4], outs)):
        cells = line.split(",")
        assert cells[0] == str(i) and cells[-1] == o["target"] and len(cells) == 8
        for cell, name in zip(cells[1:7], TOPK):
            if math.isnan(o[name]):
                assert cell == ""
            else:
                assert float(cell) == o[name] and cell == repr(o[name])
    assert lines[3].split(",")[1] == "0.5"


def _worker_epoch_end(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from deepinteract_amd.modules import LitGINI
        outs = hand_outputs(4, 21)
        mine = outs[:3] if rank == 0 else outs[3:]
        got = LitGINI(num_interact_layers=1).test_epoch_end(mine, group=dist.group.WORLD)
        q.put((rank, got))
    finally:
        dist.destroy_process_group()


def test_epoch_end_two_rank_gloo_gathers_uneven_counts():
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


# ---- labels_from_examples_batch
def _examples(l1, l2, seed):
    g = torch.Generator().manual_seed(seed)
    i, j = torch.meshgrid(torch.arange(l1), torch.arange(l2), indexing="ij")
    lab = (torch.rand(l1 * l2, generator=g) < 0.2).long()
    ex = torch.stack((i.flatten(), j.flatten(), lab), dim=1)
    return ex[torch.randperm(l1 * l2, generator=g)]


def test_labels_from_examples_batch_equals_single_and_refuses():
    from deepinteract_amd.ranking import labels_from_examples, labels_from_examples_batch
    shapes = [(5, 7), (1, 1), (12, 3)]
    exs = [_examples(l1, l2, s) for s, (l1, l2) in enumerate(shapes)]
    exs[2] = exs[2].float()                       # the reference's examples may be float
    got = labels_from_examples_batch(exs, shapes)
    assert len(got) == 3
    for out, ex, (l1, l2) in zip(got, exs, shapes):
        want = labels_from_examples(ex, l1, l2)
        assert out.dtype == torch.uint8 and torch.equal(out, want)
    assert labels_from_examples_batch([], []) == []

    def bad_batch(ex):
        return [exs[0], ex, exs[2]], [shapes[0], (5, 7), shapes[2]]

    ex = _examples(5, 7, 9)
    cases = [ex[:-1], ex[:, :2]]
    dup = ex.clone()
    dup[3] = dup[4]
    cases.append(dup)
    for col, val in ((0, 5), (1, 7), (0, -1)):
        bad = ex.clone()
        bad[0, col] = val
        cases.append(bad)
    bad = ex.clone()
    bad[2, 2] = 2
    cases.append(bad)
    for case in cases:
        with pytest.raises(ValueError) as single:
            labels_from_examples(case, 5, 7)
        with pytest.raises(ValueError) as batched:
            labels_from_examples_batch(*bad_batch(case))
        assert str(single.value) == str(batched.value)
    with pytest.raises(ValueError):
        labels_from_examples_batch(exs, shapes[:2])
