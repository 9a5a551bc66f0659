"""Contact ranking on the GPU (csrc/contact_rank.hip, ranking.ContactRankOp, LitGINI.test_step).

References, computed here:
* order: torch.sort(probs.flatten(), descending=True, stable=True) of the op's OWN stored map must
  give ids and scores exactly (ties by ascending index, NaN first);
* map: torch.softmax(logits.double(), 0)[1] on the stored-dtype logits; relative error per element
  <= (4 + |l1 - l0|) 2^-23 (the subtraction's rounding is amplified by |d| through the exponential,
  plus a few ulp for exp, the add and the reciprocal); elements with |d| > 80 absolutely, to 2e-38
  (values under FLT_MIN may be flushed). torch.softmax in fp32 on the CPU is first shown to stay
  inside the same bound on the same inputs;
* counters: torch's counts on the op's stored map (exact); ce_sum against F.cross_entropy(sum) in
  fp64 within (4 + max|d|) 2^-23 relative (a sum of non-negative terms each within that).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_common import chain_item, load_case

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def op():
    from deepinteract_amd.ranking import ContactRankOp
    return ContactRankOp("cuda")


def randn_logits(l1, l2, seed, dtype=torch.float32):
    """6 randn, class 1 shifted by -7: saturates to exact 1.0 ties and to flushed zeros."""
    g = torch.Generator().manual_seed(seed)
    lg = 6.0 * torch.randn(1, 2, l1, l2, generator=g)
    lg[:, 1] -= 7.0
    return lg.to(dtype).cuda()


def check_map(probs, logits):
    """The stored map against fp64 softmax; returns the worst error / bound ratio."""
    lg = logits.squeeze(0)
    ref = torch.softmax(lg.double(), 0)[1]
    d = (lg[1].double() - lg[0].double()).abs()
    bound = (4.0 + d) * ULP
    finite = ~torch.isnan(ref)
    rel_zone = finite & (d <= 80.0)
    abs_zone = finite & (d > 80.0)

    def ratio(p):
        p = p.double()
        r = ((p - ref).abs() / ref / bound)[rel_zone]
        return float(r.max()) if r.numel() else 0.0

    # the yardstick itself: torch's fp32 softmax on the CPU stays inside the bound on these inputs
    cpu32 = torch.softmax(lg.float().cpu(), 0)[1].cuda()
    r_torch = ratio(cpu32)
    assert r_torch <= 1.0, r_torch
    r_op = ratio(probs)
    print(f"map {tuple(probs.shape)} {logits.dtype}: worst error / bound {r_op:.3f} (torch fp32 on the CPU {r_torch:.3f})")
    assert r_op <= 1.0, r_op
    if bool(abs_zone.any()):
        assert float((probs.double() - ref).abs()[abs_zone].max()) <= 2e-38
    assert bool(torch.isnan(probs[~finite]).all())
    return r_op


def check_order(r, k):
    vals, idx = torch.sort(r.probs.flatten(), descending=True, stable=True)
    assert r.ids.dtype == torch.int32 and tuple(r.ids.shape) == (k,)
    assert torch.equal(r.ids.long(), idx[:k])
    # bit equality (NaN scores compare equal to themselves this way)
    assert torch.equal(r.scores.view(torch.int32), vals[:k].view(torch.int32))
    l2 = r.probs.shape[1]
    assert torch.equal(r.pairs[:, 0].long() * l2 + r.pairs[:, 1].long(), idx[:k])


def run(op, logits, k, **kw):
    r = op(logits, k=k, **kw)
    torch.cuda.synchronize()
    assert r.probs.dtype == torch.float32 and tuple(r.probs.shape) == tuple(logits.shape[2:])
    return r


@pytest.mark.parametrize("l1,l2", [(1, 1), (3, 5)])
def test_planes_shorter_than_a_block(op, l1, l2):
    lg = randn_logits(l1, l2, 11)
    r = run(op, lg, l1 * l2)
    check_map(r.probs, lg)
    check_order(r, l1 * l2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_c1_golden_logits_odd_plane(op, dtype):
    """145 x 145: n is odd, so the class-1 plane is not 16-B aligned."""
    z = load_case("c1")
    lg = torch.as_tensor(z["logits"]).to(dtype).cuda().contiguous()
    assert lg.shape[2] * lg.shape[3] % 2 == 1
    r = run(op, lg, None)
    assert r.ids.numel() == min(lg.shape[2], lg.shape[3])
    check_map(r.probs, lg)
    check_order(r, r.ids.numel())


@pytest.mark.parametrize("l1,l2", [(7, 4000), (4000, 7)])
def test_non_square(op, l1, l2):
    lg = randn_logits(l1, l2, 5)
    r = run(op, lg, None)
    assert r.ids.numel() == 7
    check_map(r.probs, lg)
    check_order(r, 7)
    r = run(op, lg, 4000)
    check_order(r, 4000)


def test_all_equal_ties_span_every_block(op):
    lg = torch.full((1, 2, 256, 257), 0.25, device="cuda")
    r = run(op, lg, 256)
    assert torch.equal(r.ids, torch.arange(256, dtype=torch.int32, device="cuda"))
    assert bool((r.scores == 0.5).all())
    check_order(r, 256)


def test_tie_group_straddles_k(op):
    """100 high positions, the rest equal, K = 256: the 100 in index order, then the 156 lowest-index others."""
    g = torch.Generator().manual_seed(3)
    n = 300 * 300
    high = torch.randperm(n, generator=g)[:100].sort().values
    l1 = torch.full((n,), -1.0)
    l1[high] = 3.0
    lg = torch.stack((torch.zeros(n), l1)).view(1, 2, 300, 300).cuda()
    r = run(op, lg, 256)
    is_high = torch.zeros(n, dtype=torch.bool)
    is_high[high] = True
    others = torch.nonzero(~is_high).flatten()[:156]
    assert torch.equal(r.ids.cpu().long(), torch.cat((high, others)))
    check_order(r, 256)
    check_map(r.probs, lg)


def test_only_the_last_radix_pass_separates(op):
    """d within +-2^-10 of 0: p differs in its low mantissa bits only."""
    g = torch.Generator().manual_seed(8)
    d = (torch.rand(512 * 512, generator=g) * 2 - 1) * 2.0 ** -10
    lg = torch.stack((torch.zeros_like(d), d)).view(1, 2, 512, 512).cuda()
    r = run(op, lg, 512)
    top = r.probs.flatten().view(torch.int32) >> 10
    assert int(top.max() - top.min()) <= 1 << 5   # the upper 22 key bits barely move
    check_order(r, 512)
    check_map(r.probs, lg)


@pytest.fixture(scope="module")
def big_f32():
    return randn_logits(1000, 1000, 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_saturated_map_1000(op, big_f32, dtype):
    lg = big_f32.to(dtype).contiguous()
    r = run(op, lg, 1000)
    assert int((r.probs == 1.0).sum()) > 1000   # exact-1.0 ties fill the whole list and more
    check_map(r.probs, lg)
    check_order(r, 1000)
    assert bool((r.scores == 1.0).all())
    assert bool((r.ids[1:] > r.ids[:-1]).all())


def test_nan_logits_rank_first(op, big_f32):
    lg = big_f32.clone()
    g = torch.Generator().manual_seed(21)
    pos = torch.randperm(10 ** 6, generator=g)[:3].sort().values
    flat = lg.view(2, -1)
    flat[0, int(pos[0])] = float("nan")
    flat[1, int(pos[1])] = float("nan")
    flat[:, int(pos[2])] = float("nan")
    r = run(op, lg, 1000)
    assert torch.equal(r.ids[:3].cpu().long(), pos)
    assert bool(torch.isnan(r.scores[:3]).all()) and not bool(torch.isnan(r.scores[3:]).any())
    check_order(r, 1000)
    check_map(r.probs, lg)


def test_model_limit_4096_bf16(op):
    g = torch.Generator(device="cuda").manual_seed(4)
    lg = 6.0 * torch.randn(1, 2, 4096, 4096, generator=g, device="cuda")
    lg[:, 1] -= 7.0
    lg = lg.to(torch.bfloat16).contiguous()
    from deepinteract_amd import _lib
    r = run(op, lg, _lib.DI_RANK_MAX_K)
    check_map(r.probs, lg)
    check_order(r, 4096)


@pytest.mark.parametrize("k", [1, 4096])
def test_k_edges(op, big_f32, k):
    lg = big_f32 * 0.01   # no saturation: distinct values
    r = run(op, lg, k)
    check_order(r, k)
    with pytest.raises(ValueError):
        op(lg, k=4097)
    with pytest.raises(ValueError):
        op(lg, k=0)


# ---- call patterns
def _outputs(r):
    return [r.probs.clone(), r.ids.clone(), r.scores.clone()] + ([r.hits.clone()] if r.hits is not None else [])


def test_repeat_is_bit_identical_and_back_to_back_calls(op, big_f32):
    g = torch.Generator().manual_seed(2)
    labels = (torch.rand(10 ** 6, generator=g) < 0.01).to(torch.uint8).cuda()
    other = randn_logits(1000, 1000, 77)
    a = op(big_f32, k=1000, labels=labels)
    b = op(other, k=500)                        # same workspace, no host sync in between
    c = op(big_f32, k=1000, labels=labels)
    torch.cuda.synchronize()
    for x, y in zip(_outputs(a), _outputs(c)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert a.metrics() == c.metrics()
    assert a.ce_sum == c.ce_sum and a.ce_sum > 0
    check_order(a, 1000)
    check_order(b, 500)
    check_map(b.probs, other)


def test_non_default_stream_and_probs_out(op, big_f32):
    out = torch.full((1000, 1000), -1.0, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        r = op(big_f32, k=100, probs_out=out)
    s.synchronize()
    assert r.probs.data_ptr() == out.data_ptr()
    assert bool((out >= 0).all())
    check_order(r, 100)
    check_map(out, big_f32)
    with pytest.raises(ValueError):
        op(big_f32, probs_out=torch.empty(1000, 999, device="cuda"))
    with pytest.raises(ValueError):
        op(big_f32.cpu())


# ---- labels
def check_labels(op, lg, labels, k):
    n = labels.numel()
    lg2 = lg.view(2, n)
    ce_ref = float(F.cross_entropy(lg2.double().t(), labels.long(), reduction="sum"))
    dmax = float((lg2[0].double() - lg2[1].double()).abs().max())
    for thr in (0.5, 0.9):
        r = run(op, lg, k, labels=labels, threshold=thr)
        check_order(r, k)
        assert torch.equal(r.hits.long(), torch.cumsum(labels[r.ids.long()].long(), 0))
        pred, pos = r.probs.flatten() >= thr, labels.bool()
        want = {"num_pos": int(pos.sum()), "tp": int((pred & pos).sum()), "fp": int((pred & ~pos).sum()),
                "fn": int((~pred & pos).sum()), "tn": int((~pred & ~pos).sum())}
        got = r.metrics()
        assert {f: got[f] for f in want} == want
        assert (r.num_pos, r.tp, r.fp, r.fn, r.tn) == tuple(want.values())
        err = abs(r.ce_sum - ce_ref) / ce_ref
        print(f"ce_sum {tuple(lg.shape[2:])} {lg.dtype}: relative error {err:.3e}, bound {(4 + dmax) * ULP:.3e}")
        assert err <= (4.0 + dmax) * ULP


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("positives", [True, False])
def test_label_counters_and_loss(op, big_f32, dtype, positives):
    g = torch.Generator().manual_seed(31)
    labels = (torch.rand(10 ** 6, generator=g) < (0.01 if positives else -1.0)).to(torch.uint8).cuda()
    assert bool(labels.any()) == positives
    check_labels(op, big_f32.to(dtype).contiguous(), labels, 1000)


def test_label_counters_odd_plane(op):
    z = load_case("c1")
    lg = torch.as_tensor(z["logits"]).cuda().contiguous()
    n = lg.shape[2] * lg.shape[3]
    g = torch.Generator().manual_seed(32)
    labels = (torch.rand(n, generator=g) < 0.01).to(torch.uint8).cuda()
    check_labels(op, lg, labels, min(lg.shape[2:]))


def test_without_labels_there_are_no_metrics(op):
    lg = randn_logits(3, 5, 1)
    r = op(lg)
    assert r.hits is None and r.num_pos is None
    with pytest.raises(ValueError):
        r.metrics()
    with pytest.raises(ValueError):
        op(lg, labels=torch.zeros(15, dtype=torch.int64, device="cuda"))


# ---- end to end
def _residue_graph(z, tag):
    from deepinteract_amd.graph import ResidueGraph
    it = chain_item(z, tag)
    g = ResidueGraph(it["src"], it["dst"], it["num_nodes"])
    g.ndata["f"], g.edata["f"] = it["node_f"], it["edge_f"]
    g.edata["src_nbr_e_ids"], g.edata["dst_nbr_e_ids"] = it["src_nbr"], it["dst_nbr"]
    return g.to("cuda")


def test_litgini_test_step_end_to_end():
    from deepinteract_amd.graph import GraphBatch
    from deepinteract_amd.modules import LitGINI
    from deepinteract_amd.weights import seeded_state_dict
    z = load_case("c1")
    model = LitGINI(dtype="f32", precise_head=True).cuda().eval().load_reference_state_dict(seeded_state_dict(0))
    assert model.pos_prob_threshold == 0.5
    l1, l2 = int(z["logits"].shape[2]), int(z["logits"].shape[3])
    n, l = l1 * l2, min(l1, l2)
    g = torch.Generator().manual_seed(9)
    lab = (torch.rand(n, generator=g) < 0.05).long()
    i, j = torch.meshgrid(torch.arange(l1), torch.arange(l2), indexing="ij")
    examples = torch.stack((i.flatten(), j.flatten(), lab), dim=1)   # row-major
    with torch.no_grad():
        out = model.test_step((_residue_graph(z, "g1"), _residue_graph(z, "g2"), [examples],
                               ["/data/test/4heq_l_u.dill"]), 0)
        gb = GraphBatch.from_graphs([_residue_graph(z, "g1"), _residue_graph(z, "g2")], device=model.engine.device,
                                    node_count_limit=model.cfg.node_count_limit)   # as shared_step batches them
        logits, _ = model.predict_batch(gb, [(0, 1)])
        _, ranked = model.predict_contacts(gb, [(0, 1)])
    torch.cuda.synchronize()
    lg = logits[0].contiguous()
    assert out["target"] == "4heq"
    # the references above, applied to predict_batch's logits
    probs = torch.from_numpy(out["test_preds"]).cuda()
    assert tuple(probs.shape) == (l1, l2)
    check_map(probs, lg)
    vals, idx = torch.sort(probs.flatten(), descending=True, stable=True)
    labels = lab.cuda()
    hits = torch.cumsum(labels[idx[:l]], 0).cpu()
    num_pos = int(lab.sum())
    want = {"top_10_prec": int(hits[9]) / 10, "top_l_by_10_prec": int(hits[l // 10 - 1]) / (l // 10),
            "top_l_by_5_prec": int(hits[l // 5 - 1]) / (l // 5), "top_l_recall": int(hits[l - 1]) / num_pos,
            "top_l_by_2_recall": int(hits[l // 2 - 1]) / num_pos, "top_l_by_5_recall": int(hits[l // 5 - 1]) / num_pos}
    for name, v in want.items():
        assert out[name] == v, (name, out[name], v)
    pred, pos = probs.flatten() >= 0.5, labels.bool()
    assert out["confusion"] == {"tp": int((pred & pos).sum()), "fp": int((pred & ~pos).sum()),
                                "fn": int((~pred & pos).sum()), "tn": int((~pred & ~pos).sum())}
    ce_ref = float(F.cross_entropy(lg.view(2, n).double().t(), labels, reduction="mean"))
    dmax = float((lg.view(2, n)[0].double() - lg.view(2, n)[1].double()).abs().max())
    assert abs(out["loss"] - ce_ref) / ce_ref <= (4.0 + dmax) * ULP
    assert np.array_equal(out["test_labels"], lab.view(l1, l2).float().numpy())
    assert np.array_equal(out["test_preds_rounded"], (out["test_preds"] >= 0.5).astype(np.float32))
    assert float(np.abs(out["test_preds"] - z["probs"]).max()) <= 1e-4
    # predict_contacts: the same ranking without labels
    assert len(ranked) == 1 and ranked[0].hits is None
    assert torch.equal(ranked[0].ids.long(), idx[:l])
    assert torch.equal(ranked[0].probs, probs)
