"""``predict_sharded(gather="topk")`` without a GPU (gloo, worlds of 1, 2 and 3): ranked-contact
records instead of maps. The forward is a fake that ranks a closed-form map per complex id with
``torch.sort(descending=True, stable=True)`` and writes into the record slots it is handed, so what is
tested is the driver: the record layout (``di_rank_record_bytes``, the only place it is defined), the
plan of records, the single collective, and that every rank ends with every complex's record, equal
to the unsharded computation."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from deepinteract_amd import _lib
from deepinteract_amd.distributed import RecordPlan, local_order, predict_sharded, shard
from deepinteract_amd.ranking import GatheredRanking, RecordSlot, record_k
from test_distributed import _free_port

EINVAL, ERANGE = -1, -2
SIZES = [(5, 7), (7, 5), (1, 9), (12, 12), (3, 3)]
KS = (None, 4, 100)             # 100 > L1 * L2 for most: clamps to L1 * L2
MICRO = (1, 2, 8)
RANK_FIELDS = ("num_pos", "tp", "fp", "fn", "tn", "ce_sum")
AUC_FIELDS = ("num_pos", "num_neg", "num_nan", "pos_distinct", "u2", "auroc", "auprc", "overflow")


def _complexes(sizes):
    return [({"backbone": np.zeros((a, 4, 3), np.float32)}, {"backbone": np.zeros((b, 4, 3), np.float32)})
            for a, b in sizes]


def _map_of(i, l1, l2):
    """A closed-form map with exact ties (the value repeats every 5 elements) in [0, 1)."""
    flat = torch.arange(l1 * l2, dtype=torch.float32)
    return ((flat * (3 + i)) % 5) / 8 + i / 64


def _labels_of(i, l1, l2):
    return ((torch.arange(l1 * l2) + i) % 3 == 0).to(torch.int64)


def _expected(i, l1, l2, k, with_labels):
    """The unsharded computation of complex i's record fields."""
    probs = _map_of(i, l1, l2)
    scores, order = torch.sort(probs, descending=True, stable=True)
    want = {"ids": order[:k].to(torch.int32), "scores": scores[:k]}
    if with_labels:
        lab = _labels_of(i, l1, l2)
        pred = (probs >= 0.5).to(torch.int64)
        want["hits"] = torch.cumsum(lab[order[:k]], 0).to(torch.int32)
        want["metrics"] = dict(zip(RANK_FIELDS, (int(lab.sum()), int((pred * lab).sum()), int((pred * (1 - lab)).sum()),
                                                 int(((1 - pred) * lab).sum()), int(((1 - pred) * (1 - lab)).sum()),
                                                 float(probs.double().sum()) + 0.125 * i)))
        want["auc"] = dict(zip(AUC_FIELDS, (int(lab.sum()), int((1 - lab).sum()), 0, i, 7 * i + 1,
                                            1.0 / (i + 3), float("nan") if i == 2 else 0.25 * i, 0)))
    return want


def _fake_forward(batch, ids, out):
    """Writes every complex's expected fields into its slot, as the ops would."""
    for (c1, c2), i, slot in zip(batch, ids, out):
        l1, l2 = len(c1["backbone"]), len(c2["backbone"])
        assert (slot.l1, slot.l2) == (l1, l2)
        want = _expected(i, l1, l2, slot.k, slot.with_labels)
        slot.ids.copy_(want["ids"])
        slot.scores.copy_(want["scores"])
        if slot.with_labels:
            slot.hits.copy_(want["hits"])
            m = _lib.DiRankMetrics(*[want["metrics"][f] for f in RANK_FIELDS])
            slot.metrics.copy_(torch.frombuffer(bytearray(bytes(m)), dtype=torch.int64))
            a = _lib.DiAucMetrics(*[want["auc"][f] for f in AUC_FIELDS], 0)
            slot.auc.copy_(torch.frombuffer(bytearray(bytes(a)), dtype=torch.int64))
    return out


def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and a != a and b != b)


def _check_records(recs, sizes, k, with_labels):
    """Every gathered record against the unsharded computation; returns the records' bytes."""
    raw = []
    for i, (rec, (l1, l2)) in enumerate(zip(recs, sizes)):
        kk = record_k(l1, l2, k)
        want = _expected(i, l1, l2, kk, with_labels)
        assert rec.probs is None and rec.ids.dtype == torch.int32 and rec.scores.dtype == torch.float32
        assert torch.equal(rec.ids, want["ids"]) and torch.equal(rec.scores, want["scores"])
        assert rec.pairs.tolist() == [list(divmod(int(f), l2)) for f in want["ids"]]
        if with_labels:
            assert torch.equal(rec.hits, want["hits"])
            assert all(_same(rec.metrics()[f], want["metrics"][f]) for f in RANK_FIELDS), rec.metrics()
            assert all(_same(rec.auc()[f], want["auc"][f]) for f in AUC_FIELDS), rec.auc()
            assert rec.tp == want["metrics"]["tp"] and rec.ce_sum == want["metrics"]["ce_sum"]
            assert rec.num_pos == want["metrics"]["num_pos"] and _same(rec.auprc, want["auc"]["auprc"])
            assert np.array_equal(rec.host_array("hits"), want["hits"].numpy())
        else:
            assert rec.hits is None and rec.tp is None
            with pytest.raises(ValueError):
                rec.metrics()
        assert rec.byte_off % 16 == 0
        raw.append(bytes(rec.buffer[rec.byte_off // 4:(rec.byte_off + rec.nbytes) // 4].numpy().tobytes()))
    return raw


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        calls = []
        real = dist.all_gather_into_tensor

        def counting(*args, **kwargs):
            calls.append(1)
            return real(*args, **kwargs)

        dist.all_gather_into_tensor = counting
        got = {}
        cases = [(SIZES, mb) for mb in MICRO] + [(SIZES[:2], 2)]     # world 3 over 2 complexes: an empty rank
        for sizes, mb in cases:
            cx = _complexes(sizes)
            for k in KS:
                for with_labels in (False, True):
                    before = len(calls)
                    recs, plan = predict_sharded(cx, _fake_forward, micro_batch=mb, gather="topk", k=k,
                                                 with_labels=with_labels)
                    assert len(calls) - before == 1, "exactly one all-gather per call"
                    assert plan == shard(sizes, world) and len(recs) == len(sizes)
                    raw = _check_records(recs, sizes, k, with_labels)
                    per_rank = [sum(_lib.rank_record_layout(*sizes[i], record_k(*sizes[i], k), with_labels)[0]
                                    for i in p) for p in plan]
                    assert recs[0].buffer.numel() * 4 == world * max(per_rank)
                    assert recs[0].buffer.dtype == torch.int32 and all(r.buffer is recs[0].buffer for r in recs)
                    got[(len(sizes), mb, k, with_labels)] = (raw, recs[0].buffer.numpy().tobytes())
        # a K beyond DI_RANK_MAX_K: ValueError on every rank, before any collective (no hang)
        big = _complexes([(5, 7), (_lib.DI_RANK_MAX_K + 1, _lib.DI_RANK_MAX_K + 4)])
        before = len(calls)
        refused = []
        for k in (None, _lib.DI_RANK_MAX_K + 1):
            try:
                predict_sharded(big, _fake_forward, micro_batch=2, gather="topk", k=k)
                refused.append(False)
            except ValueError:
                refused.append(True)
        assert refused == [True, True] and len(calls) == before
        recs, _ = predict_sharded(big, _fake_forward, micro_batch=2, gather="topk", k=_lib.DI_RANK_MAX_K)
        assert [r.ids.numel() for r in recs] == [35, _lib.DI_RANK_MAX_K]
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, got, None))
    except Exception as exc:      # reported to the parent instead of hanging it
        import traceback
        q.put((rank, None, traceback.format_exc() + repr(exc)))


@pytest.mark.parametrize("world", [1, 2, 3])
def test_topk_records_equal_unsharded_on_every_rank(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted((q.get(timeout=180) for _ in procs), key=lambda t: t[0])
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for rank, got, err in res:
        assert err is None, f"rank {rank}: {err}"
    first = res[0][1]
    assert len(first) == (len(MICRO) + 1) * len(KS) * 2
    for rank, got, _ in res[1:]:
        assert got == first, f"rank {rank} holds other bytes than rank 0"
    # the records' bytes do not depend on the micro-batch size either
    for k in KS:
        for with_labels in (False, True):
            assert len({tuple(first[(len(SIZES), mb, k, with_labels)][0]) for mb in MICRO}) == 1
    assert [p.exitcode for p in procs] == [0] * world


def test_record_layout_is_the_c_functions():
    lib = _lib.load()
    offs = (ctypes.c_int64 * 5)()
    for l1, l2 in SIZES + [(1, 1), (145, 40), (1000, 1000), (4096, 4096)]:
        for k in sorted({1, min(l1 * l2, 2), min(l1 * l2, 3), min(l1, l2), min(l1 * l2, 37),
                             min(l1 * l2, _lib.DI_RANK_MAX_K)}):
            for with_labels in (0, 1):
                nb = lib.di_rank_record_bytes(l1, l2, k, with_labels, offs)
                assert nb == lib.di_rank_record_bytes(l1, l2, k, with_labels, None) > 0
                assert nb % 16 == 0
                ids, scores, hits, metrics, auc = list(offs)
                assert (ids, scores) == (0, 4 * k)
                if with_labels:
                    assert hits == 8 * k and metrics == (12 * k + 7) // 8 * 8
                    assert auc == metrics + ctypes.sizeof(_lib.DiRankMetrics)
                    assert metrics % 8 == 0 and auc % 8 == 0 and hits % 4 == 0
                    assert nb == (auc + ctypes.sizeof(_lib.DiAucMetrics) + 15) // 16 * 16
                else:
                    assert (hits, metrics, auc) == (-1, -1, -1) and nb == (8 * k + 15) // 16 * 16
                # what Python sees is the C function's answer
                pnb, poffs = _lib.rank_record_layout(l1, l2, k, bool(with_labels))
                assert pnb == nb and poffs == {f: o for f, o in zip(_lib.RECORD_FIELDS, offs) if o >= 0}
                buf = torch.zeros(nb // 4 + 8, dtype=torch.int32)
                slot = RecordSlot(buf, 16, l1, l2, k, bool(with_labels))
                assert slot.nbytes == nb and slot.ids.numel() == slot.scores.numel() == k
                assert slot.ids.data_ptr() == buf.data_ptr() + 16 and slot.scores.data_ptr() == buf.data_ptr() + 16 + scores
                if with_labels:
                    assert slot.metrics.dtype == torch.int64 and slot.metrics.numel() == 6 and slot.auc.numel() == 8
                    assert slot.metrics.data_ptr() == buf.data_ptr() + 16 + metrics
                    assert slot.auc.data_ptr() == buf.data_ptr() + 16 + auc
                    assert slot.hits.data_ptr() == buf.data_ptr() + 16 + hits
    # 1000 x 1000 with labels: about 12 KB against a 4 MB map
    assert lib.di_rank_record_bytes(1000, 1000, 1000, 1, None) == 12112


def test_record_bytes_refusals():
    lib = _lib.load()
    offs = (ctypes.c_int64 * 5)(*[77] * 5)
    for args, rc in (((0, 5, 1, 0), EINVAL), ((5, 0, 1, 0), EINVAL), ((-3, 5, 1, 1), EINVAL), ((5, -1, 1, 1), EINVAL),
                     ((5, 5, 0, 0), EINVAL), ((5, 5, -1, 1), EINVAL), ((5, 5, 26, 0), EINVAL), ((3, 3, 10, 1), EINVAL),
                     ((5, 5, 5, 2), EINVAL), ((5, 5, 5, -1), EINVAL),
                     ((100, 100, _lib.DI_RANK_MAX_K + 1, 0), ERANGE), ((1 << 15, 1 << 14, 10, 1), ERANGE),
                     (((1 << 31) - 1, (1 << 31) - 1, 10, 0), ERANGE), ((10, 10, 5000, 0), EINVAL)):
        assert lib.di_rank_record_bytes(*args, offs) == rc, args
        assert list(offs) == [77] * 5           # a refusal writes nothing
        if args[3] in (0, 1):
            with pytest.raises(ValueError):
                _lib.rank_record_layout(*args)
    assert lib.di_rank_record_bytes(4096, 4096, _lib.DI_RANK_MAX_K, 1, None) > 0


def test_record_k_and_plan():
    assert record_k(5, 7) == 5 and record_k(5, 7, 4) == 4 and record_k(5, 7, 100) == 35
    for bad in ((5, 7, 0), (5, 7, -2), (5000, 4097, None), (100, 100, _lib.DI_RANK_MAX_K + 1)):
        with pytest.raises(ValueError):
            record_k(*bad)
    for world in (1, 2, 3, 8):
        plan = shard(SIZES, world)
        for with_labels in (False, True):
            rp = RecordPlan(SIZES, plan, None, with_labels)
            spans = {}
            for r, p in enumerate(plan):
                at = 0
                for i in local_order(SIZES, p):       # a micro-batch's records are contiguous
                    assert rp.place[i] == (r, at)
                    at += _lib.rank_record_layout(*SIZES[i], rp.ks[i], with_labels)[0]
                spans[r] = at
            assert rp.rank_bytes == [spans[r] for r in range(world)]
            assert rp.width == max(rp.rank_bytes) and rp.recv_bytes == world * rp.width
    assert RecordPlan([], [[], []]).width == 16


def test_slot_and_gathered_record_refuse_bad_buffers():
    buf = torch.zeros(64, dtype=torch.int32)
    RecordSlot(buf, 0, 5, 7, 5, True)
    for bad in (4, 8, -16):
        with pytest.raises(ValueError):
            RecordSlot(buf, bad, 5, 7, 5, True)                       # records start 16-B aligned
    with pytest.raises(ValueError):
        RecordSlot(buf, 96, 5, 7, 5, True)                            # 176 bytes do not fit behind byte 96
    with pytest.raises(ValueError):
        RecordSlot(buf.to(torch.int64), 0, 5, 7, 5, True)
    with pytest.raises(ValueError):
        RecordSlot(buf.view(8, 8), 0, 5, 7, 5, True)
    with pytest.raises(ValueError):
        RecordSlot(buf[::2], 0, 5, 7, 5, False)
    with pytest.raises(ValueError):
        GatheredRanking(buf, 0, 5, 7, 36, False)                      # k > L1 * L2
