"""Ranked-contact records on the GPU: ``ContactRankOp.batch(out=...)`` / ``ContactAucOp.batch(out=...)``
writing into one shared buffer laid out by ``di_rank_record_bytes``, and the sharded driver over them
(``predict_sharded(gather="topk")``, ``ranked_forward``, ``test_sharded``) with the real HIP forward.

Op level: with ``out`` every output has the bits it has without, and nothing else in the buffer
changes. Driver level, two gloo ranks sharing cuda:0 and one RCCL rank, ``LitGINI(dtype="f32",
precise_head=True)`` (bit-stable across micro-batching, tests/test_gpu_c4.py): every rank's ids and
scores equal a single-process ``predict_contacts`` over the whole batch, every ``test_sharded`` figure
equals a single-process ``test_batch`` (floats by exact equality, NaN matching NaN), and a complex
that overflows ``auc_max_pos`` is finished by its owner before the collective."""
import os
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_gpu_c4 import _free_port, _model

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
SIZES = [(20, 20), (21, 64), (64, 21), (33, 47), (145, 40)]     # chains hold >= k = 20 residues
SEED = 0


def _same(a, b):
    """Exact equality, NaN matching NaN, through dicts."""
    if isinstance(a, float) and isinstance(b, float):
        return a == b or (a != a and b != b)
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    return type(a) is type(b) and a == b


# ---- op level -------------------------------------------------------------------------------------
def _op_cases():
    """(fp32 logits [1, 2, L1, L2], uint8 labels [n], k) on the device: exact ties (K = n over a map of
    one value), a NaN and a tie group, a map saturated to 1.0."""
    g = torch.Generator().manual_seed(3)
    ties = torch.full((1, 2, 1, 9), 0.25)
    nan = 6.0 * torch.randn(1, 2, 37, 64, generator=g)
    nan.view(2, -1)[1, 1000] = float("nan")
    nan.view(2, -1)[:, 64:128] = 0.5                       # one row of equal probabilities
    sat = 30.0 * torch.randn(1, 2, 145, 40, generator=g)   # saturates to exactly 1.0 and 0.0
    cases = []
    for lg, share, k in ((ties, 0.4, 9), (nan, 0.05, None), (sat, 0.03, None)):
        n = lg.shape[2] * lg.shape[3]
        cases.append((lg.cuda().contiguous(), (torch.rand(n, generator=g) < share).to(torch.uint8).cuda(), k))
    return cases


def _layout(cases, with_labels, lead=16, tail=32):
    from deepinteract_amd import _lib
    from deepinteract_amd.ranking import record_k
    at, places = lead, []
    for lg, _, k in cases:
        l1, l2 = int(lg.shape[2]), int(lg.shape[3])
        kk = record_k(l1, l2, k)
        nb, offs = _lib.rank_record_layout(l1, l2, kk, with_labels)
        places.append((at, l1, l2, kk, nb, offs))
        at += nb
    return places, at + tail


@pytest.mark.parametrize("with_labels", [False, True])
def test_ops_write_the_record_with_the_bits_of_the_plain_call(with_labels):
    from deepinteract_amd import _lib
    from deepinteract_amd.ranking import ContactAucOp, ContactRankOp, RecordSlot
    rank, auc = ContactRankOp("cuda"), ContactAucOp("cuda")
    cases = _op_cases()
    logits, labels, ks = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    plain = rank.batch(logits, k=ks, labels_list=labels if with_labels else None)
    plain_auc = auc.batch([r.probs for r in plain], labels) if with_labels else None
    assert float(plain[2].probs.max()) == 1.0 and bool(torch.isnan(plain[1].scores[0]))

    places, total = _layout(cases, with_labels)
    buf = torch.full((total // 4,), FILL, dtype=torch.int32, device="cuda")
    slots = [RecordSlot(buf, at, l1, l2, kk, with_labels) for at, l1, l2, kk, _, _ in places]
    got = rank.batch(logits, k=ks, labels_list=labels if with_labels else None, out=slots)
    if with_labels:
        got_auc = auc.batch([r.probs for r in got], labels, out=slots)
    torch.cuda.synchronize()
    host = buf.cpu().numpy().view(np.uint8)
    covered = np.zeros(host.shape, dtype=bool)
    for slot, r, p, (at, l1, l2, kk, nb, offs) in zip(slots, got, plain, places):
        assert r.ids.data_ptr() == slot.ids.data_ptr() == buf.data_ptr() + at + offs["ids"]
        assert r.scores.data_ptr() == slot.scores.data_ptr() == buf.data_ptr() + at + offs["scores"]
        assert torch.equal(slot.ids, p.ids) and p.ids.numel() == kk
        assert slot.scores.cpu().numpy().tobytes() == p.scores.cpu().numpy().tobytes()
        assert r.probs.cpu().numpy().tobytes() == p.probs.cpu().numpy().tobytes()
        assert torch.equal(r.pairs, p.pairs)
        covered[at + offs["ids"]:at + offs["ids"] + 4 * kk] = True
        covered[at + offs["scores"]:at + offs["scores"] + 4 * kk] = True
        if with_labels:
            assert r.hits.data_ptr() == buf.data_ptr() + at + offs["hits"]
            assert torch.equal(slot.hits, p.hits)
            assert torch.equal(slot.metrics, p._metrics_dev) and _same(r.metrics(), p.metrics())
            covered[at + offs["hits"]:at + offs["hits"] + 4 * kk] = True
            covered[at + offs["metrics"]:at + offs["metrics"] + 48] = True
            covered[at + offs["auc"]:at + offs["auc"] + 64] = True
    if with_labels:
        for slot, a, p in zip(slots, got_auc, plain_auc):
            assert torch.equal(slot.auc, p._metrics_dev)
            assert _same(a.metrics(), p.metrics())
    # lead, tail and the records' padding keep the fill pattern
    assert covered.sum() < covered.size
    assert np.array_equal(host[~covered], np.full(int((~covered).sum()), 0x5A, dtype=np.uint8))
    # a received record reads the same buffer
    from deepinteract_amd.ranking import GatheredRanking
    at, l1, l2, kk, _, _ = places[1]
    rec = GatheredRanking(buf, at, l1, l2, kk, with_labels)
    assert rec.probs is None and torch.equal(rec.ids, plain[1].ids)
    assert rec.pairs.tolist() == [list(divmod(int(i), l2)) for i in plain[1].ids.cpu()]
    if with_labels:
        assert _same(rec.metrics(), plain[1].metrics()) and rec.tp == plain[1].tp
        assert _same(rec.ce_sum, plain[1].ce_sum) and _same(rec.auc(), plain_auc[1].metrics())
        assert rec.auc()["num_pos"] == plain_auc[1].num_pos and rec.auc()["u2"] == plain_auc[1].u2
        assert np.array_equal(rec.host_array("hits"), plain[1].hits.cpu().numpy())
    assert _lib.DI_RANK_MAX_K == 4096


def test_bad_slots_raise_before_any_launch():
    from deepinteract_amd.ranking import ContactAucOp, ContactRankOp, RecordSlot
    rank, auc = ContactRankOp("cuda"), ContactAucOp("cuda")
    cases = _op_cases()
    logits, labels, ks = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    places, total = _layout(cases, True)
    buf = torch.full((total // 4,), FILL, dtype=torch.int32, device="cuda")
    at, l1, l2, kk, nb, _ = places[1]
    for bad in (at + 4, at + 8):                                # misaligned
        with pytest.raises(ValueError):
            RecordSlot(buf, bad, l1, l2, kk, True)
    with pytest.raises(ValueError):                             # short: the last record does not fit
        RecordSlot(buf[:(places[2][0] + places[2][4]) // 4 - 4], places[2][0], *places[2][1:4], True)
    good = [RecordSlot(buf, p[0], p[1], p[2], p[3], True) for p in places]

    def edited(**kw):
        fields = {f: getattr(good[1], f) for f in ("ids", "scores", "hits", "metrics", "auc")}
        fields.update(kw)
        return [good[0], types.SimpleNamespace(**fields), good[2]]

    wrong = [dict(ids=good[1].ids[:-1]), dict(scores=good[1].scores[:-1]), dict(hits=good[1].hits[:-1]),
             dict(ids=good[1].scores), dict(scores=good[1].ids), dict(hits=None),
             dict(metrics=good[1].metrics.view(torch.int32)), dict(metrics=good[1].metrics[:5]),
             dict(ids=buf[0:2 * kk:2]), dict(ids=good[1].ids.cpu()), dict(metrics=good[1].metrics.cpu())]
    for kw in wrong:
        with pytest.raises(ValueError):
            rank.batch(logits, k=ks, labels_list=labels, out=edited(**kw))
    with pytest.raises(ValueError):
        rank.batch(logits, k=ks, labels_list=labels, out=good[:2])
    with pytest.raises(ValueError):                             # a slot made for another k
        rank.batch(logits, k=[9, 5, None], labels_list=labels, out=good)
    probs = [torch.rand(int(lg.shape[2]), int(lg.shape[3]), device="cuda") for lg in logits]
    for kw in (dict(auc=good[1].auc[:7]), dict(auc=good[1].auc.view(torch.float64)), dict(auc=good[1].auc.cpu())):
        with pytest.raises(ValueError):
            auc.batch(probs, labels, out=edited(**kw))
    with pytest.raises(ValueError):
        auc.batch(probs, labels, out=good[:1])
    torch.cuda.synchronize()
    assert bool((buf == FILL).all())                            # every refusal came before a launch


# ---- driver level ---------------------------------------------------------------------------------
def _complexes():
    from deepinteract_amd import synth
    return [synth.synthetic_complex(700 + i, a, b) for i, (a, b) in enumerate(SIZES)]


def _examples():
    """Complete example lists in shuffled row order: complex 0 without a positive (AUROC NaN), complex 1
    dense, the others about 5 % positives."""
    g = torch.Generator().manual_seed(11)
    out = []
    for c, (l1, l2) in enumerate(SIZES):
        i, j = torch.meshgrid(torch.arange(l1), torch.arange(l2), indexing="ij")
        share = (0.0, 0.6)[c] if c < 2 else 0.05
        lab = (torch.rand(l1 * l2, generator=g) < share).long()
        ex = torch.stack((i.flatten(), j.flatten(), lab), dim=1)
        out.append(ex[torch.randperm(l1 * l2, generator=g)].contiguous())
    return out


FILEPATHS = [os.path.join("data", "final", f"{chr(97 + i)}{i}xy_complex.dill") for i in range(len(SIZES))]
K_EXTRA = 30      # an explicit k: beyond min(L1, L2) of the smallest complexes, below every L1 * L2


def _plain(o):
    """A test_step dict as picklable host values."""
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in o.items()}


def _worker(backend, rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    try:
        torch.cuda.set_device(0)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        from deepinteract_amd.builder import build_graph_batch
        from deepinteract_amd.distributed import predict_sharded, ranked_forward, test_sharded
        model = _model()
        cx, examples = _complexes(), _examples()
        device = "cuda" if backend == "nccl" else "cuda:0"
        res = {"backend": dist.get_backend()}
        for k in (None, K_EXTRA):
            recs, plan = predict_sharded(cx, ranked_forward(model, k=20, seed=SEED), micro_batch=2, device=device,
                                         gather="topk", k=k)
            torch.cuda.synchronize()
            res[("ranked", k)] = [(r.ids.is_cuda, r.ids.cpu().numpy().tobytes(), r.scores.cpu().numpy().tobytes(),
                                   r.pairs.cpu().tolist(), r.probs is None and r.hits is None) for r in recs]
            res["plan"] = [len(p) for p in plan]
        outs = model.test_sharded(cx, examples, FILEPATHS, micro_batch=2, k=20, seed=SEED, device=device)
        res["outs"] = [_plain(o) for o in outs]
        res["medians"] = model.test_epoch_end(outs)
        tight = test_sharded(model, cx, examples, FILEPATHS, micro_batch=2, k=20, seed=SEED, device=device,
                             auc_max_pos=4)
        res["outs_max_pos_4"] = [_plain(o) for o in tight]
        if rank == 0:       # the single-process yardstick, computed once per test
            chains = [c for pair in cx for c in pair]
            gb = build_graph_batch(chains, k=20, device="cuda:0", node_count_limit=model.cfg.node_count_limit,
                                   nbr_seeds=[SEED + 2 * i + s for i in range(len(cx)) for s in (0, 1)])
            pairs = [(2 * j, 2 * j + 1) for j in range(len(cx))]
            with torch.no_grad():
                for k in (None, K_EXTRA):
                    _, ranks = model.predict_contacts(gb, pairs, k=k)
                    res[("ref_ranked", k)] = [(r.ids.cpu().numpy().tobytes(), r.scores.cpu().numpy().tobytes())
                                              for r in ranks]
                ref = model.test_batch(gb, pairs, examples, FILEPATHS, keep_maps=0)
            res["ref_outs"] = [_plain(o) for o in ref]
            res["ref_medians"] = model.test_epoch_end(ref)
        if backend == "gloo":
            dist.barrier()
        dist.destroy_process_group()
        q.put((rank, res, None))
    except Exception as exc:      # reported to the parent instead of hanging it
        import traceback
        q.put((rank, None, traceback.format_exc() + repr(exc)))


def _run(backend, world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(backend, r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted((q.get(timeout=300) for _ in procs), key=lambda t: t[0])
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for rank, got, err in res:
        assert err is None, f"rank {rank}: {err}"
    assert [p.exitcode for p in procs] == [0] * world
    return [got for _, got, _ in res]


def _check(results, backend, world):
    ref = results[0]
    assert sum(ref["plan"]) == len(SIZES) and min(ref["plan"]) >= 1
    dense = [c for c, o in enumerate(ref["ref_outs"]) if o["confusion"]["tp"] + o["confusion"]["fn"] >= 10]
    assert 1 in dense and len(dense) >= 2           # auc_max_pos = 4 overflows on these
    assert ref["ref_outs"][0]["test_auroc"] != ref["ref_outs"][0]["test_auroc"]        # no positive: NaN
    for rank, got in enumerate(results):
        assert got["backend"] == backend
        for k in (None, K_EXTRA):
            for c, ((on_dev, ids, scores, pairs, bare), (ref_ids, ref_scores), (l1, l2)) in enumerate(
                    zip(got[("ranked", k)], ref[("ref_ranked", k)], SIZES)):
                kk = min(l1, l2) if k is None else min(k, l1 * l2)
                assert on_dev and bare and len(ids) == 4 * kk
                assert ids == ref_ids and scores == ref_scores, (rank, k, c)
                assert pairs == [list(divmod(int(i), l2)) for i in np.frombuffer(ids, dtype=np.int32)]
        for name in ("outs", "outs_max_pos_4"):
            assert len(got[name]) == len(SIZES)
            for c, (o, want, (l1, l2)) in enumerate(zip(got[name], ref["ref_outs"], SIZES)):
                for key, v in want.items():             # every key of test_batch
                    assert key in o and _same(o[key], v), (rank, name, c, key, o[key], v)
                assert o["test_preds"] is None and o["test_preds_rounded"] is None and o["test_labels"] is None
                assert o["target"] == FILEPATHS[c].split(os.sep)[-1][:4]
                ref_ids, ref_scores = ref[("ref_ranked", None)][c]
                assert np.asarray(o["top_ids"], dtype=np.int32).tobytes() == ref_ids
                assert np.asarray(o["top_scores"], dtype=np.float32).tobytes() == ref_scores
        assert _same(got["medians"], ref["ref_medians"]), (rank, got["medians"], ref["ref_medians"])


def test_two_gloo_ranks_on_one_gpu_equal_single_process():
    _check(_run("gloo", 2), "gloo", 2)


def test_one_rccl_rank_equals_single_process():
    _check(_run("nccl", 1), "nccl", 1)
