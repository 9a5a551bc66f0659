"""Exact per-complex AUROC / AUPRC on the GPU (csrc/contact_auc.hip, ranking.ContactAucOp,
LitGINI.test_step's test_auroc / test_auprc).

Reference, computed here on the op's OWN input map: test_contact_auc_host.ref_auc (sort of the whole
map, tie groups, exact integers, extended-precision sum; pinned to scikit-learn in that module).
* num_pos, num_neg, num_nan, pos_distinct and u2 are EQUAL to the reference's;
* auroc within 2^-52 relative: one fp64 quotient of the exact integers u2 and 2 P N;
* auprc within (U + 2) 2^-53 relative: a sum of U positive fp64 terms, each a few roundings from exact.
"""
import math

import pytest
import torch

from gpu_common import chain_item, load_case
from test_contact_auc_host import ref_auc

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def op():
    from deepinteract_amd.ranking import ContactAucOp
    return ContactAucOp("cuda")


@pytest.fixture(scope="module")
def rank():
    from deepinteract_amd.ranking import ContactRankOp
    return ContactRankOp("cuda")


def bernoulli(n, share, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, generator=g) < share).to(torch.uint8).cuda()


def exactly(n, num_pos, seed):
    g = torch.Generator().manual_seed(seed)
    lab = torch.zeros(n, dtype=torch.uint8)
    lab[torch.randperm(n, generator=g)[:num_pos]] = 1
    return lab.cuda()


def uniform_map(l1, l2, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(l1, l2, generator=g).cuda()


def against_ref(res, probs, labels, what=""):
    """The record of one op call against ref_auc of the same map; returns the reference."""
    torch.cuda.synchronize()
    u2, auroc, auprc, (P, N, nan, U) = ref_auc(probs.cpu().numpy(), labels.cpu().numpy())
    got = res.metrics()
    assert (got["num_pos"], got["num_neg"], got["num_nan"], got["pos_distinct"]) == (P, N, nan, U), (what, got)
    assert got["u2"] == u2, (what, got["u2"], u2)
    assert got["overflow"] == 0
    if math.isnan(auroc):
        assert math.isnan(got["auroc"]) and math.isnan(got["auprc"]), (what, got)
        return u2, auroc, auprc, (P, N, nan, U)
    e_roc, e_ap = abs(got["auroc"] - auroc) / auroc if auroc else abs(got["auroc"]), abs(got["auprc"] - auprc) / auprc
    print(f"auc {what or tuple(probs.shape)}: P = {P}, U = {U}, auroc {got['auroc']:.17g} rel. error {e_roc:.2e}, "
          f"auprc {got['auprc']:.17g} rel. error {e_ap:.2e} (bound {(U + 2) * EPS:.2e})")
    assert e_roc <= 2 * EPS, (what, got["auroc"], auroc)
    assert e_ap <= (U + 2) * EPS, (what, got["auprc"], auprc)
    return u2, auroc, auprc, (P, N, nan, U)


@pytest.mark.parametrize("label", [1, 0])
def test_one_element(op, label):
    probs = torch.full((1, 1), 0.25, device="cuda")
    res = op(probs, torch.full((1,), label, dtype=torch.uint8, device="cuda"))
    _, auroc, _, counts = against_ref(res, probs, torch.tensor([label]))
    assert math.isnan(auroc) and counts == (label, 1 - label, 0, 0)
    assert math.isnan(res.auroc) and math.isnan(res.auprc)


def test_3x5_one_positive(op):
    probs = uniform_map(3, 5, 1)
    labels = exactly(15, 1, 2)
    u2, auroc, auprc, _ = against_ref(op(probs, labels), probs, labels)
    below = int((probs.flatten() < probs.flatten()[labels.bool()]).sum())
    assert u2 == 2 * below and auroc == below / 14 and auprc == pytest.approx(1 / (15 - below), rel=4 * EPS)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_c1_golden_logits_odd_plane(op, rank, dtype):
    """145 x 145 through ContactRankOp: the map ranking and AUC both judge; n is odd."""
    z = load_case("c1")
    lg = torch.as_tensor(z["logits"]).to(dtype).cuda().contiguous()
    n = lg.shape[2] * lg.shape[3]
    assert n % 2 == 1
    labels = bernoulli(n, 0.01, 5)
    r = rank(lg, labels=labels)
    against_ref(op(r.probs, labels), r.probs, labels, f"c1 {dtype}")


def test_all_scores_equal(op):
    probs = torch.full((256, 257), 0.5, device="cuda")
    labels = bernoulli(256 * 257, 0.01, 6)
    res = op(probs, labels)
    _, _, _, (P, N, _, U) = against_ref(res, probs, labels)
    assert U == 1 and res.u2 == P * N
    assert res.auroc == 0.5 and res.auprc == P / (256 * 257)


@pytest.mark.parametrize("l1,l2", [(7, 4000), (4000, 7)])
def test_non_square(op, l1, l2):
    probs = uniform_map(l1, l2, 7)
    labels = bernoulli(l1 * l2, 0.01, 8)
    against_ref(op(probs, labels), probs, labels)


@pytest.fixture(scope="module")
def saturated(rank):
    """1000 x 1000 of 30 randn logits: about a quarter of the map is exactly 1.0, some of it exactly 0."""
    g = torch.Generator().manual_seed(0)
    lg = 30.0 * torch.randn(1, 2, 1000, 1000, generator=g)
    probs = rank(lg.cuda(), k=10).probs
    torch.cuda.synchronize()
    assert int((probs == 1.0).sum()) > 10 ** 5 and int((probs == 0.0).sum()) > 100
    return probs, bernoulli(10 ** 6, 0.002, 9)


def test_saturated_map_1000(op, saturated):
    probs, labels = saturated
    _, _, _, (P, _, _, U) = against_ref(op(probs, labels), probs, labels, "saturated 1000 x 1000")
    assert U < P                                   # the positives at exactly 1.0 are one group
    assert bool((probs.flatten()[labels.bool()] == 0.0).any())    # and the smallest positive key ties with negatives


def test_tie_group_of_positives_and_negatives_inside_the_map(op, saturated):
    probs, labels = saturated
    probs = probs.clone()
    flat, lab = probs.view(-1), labels.bool()
    flat[torch.nonzero(lab).flatten()[100:140]] = 0.37      # 40 positives and 60 negatives share one score
    flat[torch.nonzero(~lab).flatten()[5000:5060]] = 0.37   # strictly between other positives' scores
    pos_scores = flat[lab]
    assert bool((pos_scores > 0.37).any()) and bool(((pos_scores < 0.37) & (pos_scores > 0)).any())
    against_ref(op(probs, labels), probs, labels, "mid-map tie group")


@pytest.mark.parametrize("num_pos", [4096, 4097])
def test_one_block_and_global_sort_boundary(op, num_pos):
    probs = uniform_map(300, 300, 10)
    labels = exactly(90000, num_pos, 11)
    _, _, _, (P, _, _, _) = against_ref(op(probs, labels), probs, labels, f"P = {num_pos}")
    assert P == num_pos


def test_half_positives_64(op):
    probs = uniform_map(64, 64, 12)
    labels = bernoulli(4096, 0.5, 13)
    against_ref(op(probs, labels), probs, labels)


@pytest.mark.parametrize("label", [1, 0])
def test_one_class_only(op, label):
    probs = uniform_map(64, 65, 14)
    labels = torch.full((64 * 65,), label, dtype=torch.uint8, device="cuda")
    _, auroc, _, counts = against_ref(op(probs, labels), probs, labels)
    assert math.isnan(auroc) and counts == (64 * 65 * label, 64 * 65 * (1 - label), 0, 0)


@pytest.mark.parametrize("on_positive", [True, False])
def test_one_nan_score(op, on_positive):
    probs = uniform_map(300, 300, 15)
    labels = bernoulli(90000, 0.01, 16)
    at = int(torch.nonzero(labels.bool() == on_positive).flatten()[17])
    probs.view(-1)[at] = float("nan")
    res = op(probs, labels)
    against_ref(res, probs, labels)
    assert res.num_nan == 1 and math.isnan(res.auroc) and math.isnan(res.auprc)
    assert res.num_pos == int(labels.sum()) and res.num_pos + res.num_neg == 90000


def test_overflow_is_reported_and_nothing_is_written_past_the_workspace():
    """max_pos below the positives, given to the C entry point: overflow = 1, the counts stay right, and
    the bytes behind di_contact_auc_work_bytes(n, max_pos) keep their pattern."""
    from deepinteract_amd import _lib
    from deepinteract_amd.engine import _ptr, _stream
    lib = _lib.load()
    probs = uniform_map(300, 300, 17)
    labels = bernoulli(90000, 0.3, 18)
    n, num_pos = 90000, int(labels.sum())
    for max_pos in (1, 1000, 4097, num_pos - 1):
        nb = lib.di_contact_auc_work_bytes(n, max_pos)
        assert nb > 0 and nb % 4 == 0
        guard = 4096
        buf = torch.full((nb + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        out = torch.zeros(8, dtype=torch.int64, device="cuda")
        rc = lib.di_contact_auc(_ptr(probs), _ptr(labels), n, max_pos, _ptr(out), _ptr(buf), _stream())
        assert rc == 0
        torch.cuda.synchronize()
        m = _lib.DiAucMetrics.from_buffer_copy(out.cpu().numpy().tobytes())
        assert m.overflow == 1 and (m.num_pos, m.num_neg, m.num_nan) == (num_pos, n - num_pos, 0)
        assert math.isnan(m.auroc) and math.isnan(m.auprc) and m.u2 == 0 and m.pos_distinct == 0
        assert bool((buf[nb:] == 0xA5).all()), max_pos
    # exactly enough room: no overflow
    nb = lib.di_contact_auc_work_bytes(n, num_pos)
    buf = torch.full((nb + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.zeros(8, dtype=torch.int64, device="cuda")
    assert lib.di_contact_auc(_ptr(probs), _ptr(labels), n, num_pos, _ptr(out), _ptr(buf), _stream()) == 0
    torch.cuda.synchronize()
    m = _lib.DiAucMetrics.from_buffer_copy(out.cpu().numpy().tobytes())
    u2, auroc, _, _ = ref_auc(probs.cpu().numpy(), labels.cpu().numpy())
    assert m.overflow == 0 and m.u2 == u2 and abs(m.auroc - auroc) <= 2 * EPS * auroc
    assert bool((buf[nb:] == 0xA5).all())


@pytest.mark.parametrize("share,max_pos", [(0.3, None), (0.3, 1000), (0.8, None)])
def test_rerun_after_overflow(share, max_pos):
    """300 x 300: the default max_pos is 65536, which 30 % positives fit and 80 % do not; an explicit
    max_pos = 1000 overflows at 30 % too. The op then runs once more with max_pos = num_pos."""
    from deepinteract_amd.ranking import ContactAucOp
    op = ContactAucOp("cuda")                      # its own workspace: the rerun has to grow it
    probs = uniform_map(300, 300, 19)
    labels = bernoulli(90000, share, 20)
    res = op(probs, labels, max_pos=max_pos)
    first = res.max_pos
    assert first == (65536 if max_pos is None else max_pos)
    _, _, _, (P, _, _, _) = against_ref(res, probs, labels, f"{share:.0%} positives, max_pos {max_pos}")
    assert res.max_pos == (P if P > first else first)
    assert (share, max_pos) == (0.3, None) or res.max_pos == P


def test_many_blocks_2048x2047(op):
    probs = uniform_map(2048, 2047, 21)
    probs = (probs * 65536).floor() / 65536            # 2^16 levels: tie groups of positives and negatives
    labels = bernoulli(2048 * 2047, 0.02, 22)
    _, _, _, (P, _, _, U) = against_ref(op(probs, labels), probs, labels, "2048 x 2047")
    assert P > 80000 and U > 4096


def _raw(res):
    torch.cuda.synchronize()
    return res._metrics_dev.cpu().numpy().tobytes()


def test_repeat_is_bit_identical_and_back_to_back_calls(op, saturated):
    probs, labels = saturated
    other = uniform_map(700, 900, 23)
    other_labels = bernoulli(700 * 900, 0.05, 24)      # 31 k positives: the global sort
    a = op(probs, labels)
    b = op(other, other_labels)                        # same workspace, no host sync in between
    c = op(probs, labels)
    d = op(other, other_labels)
    assert _raw(a) == _raw(c) and _raw(b) == _raw(d)
    against_ref(a, probs, labels)
    against_ref(b, other, other_labels)
    assert b.num_pos > 4096 >= a.num_pos


def test_non_default_stream(op):
    probs = uniform_map(500, 501, 25)
    labels = bernoulli(500 * 501, 0.03, 26)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        res = op(probs, labels)
    s.synchronize()
    against_ref(res, probs, labels)
    with pytest.raises(ValueError):
        op(probs.cpu(), labels)
    with pytest.raises(ValueError):
        op(probs, labels.cpu())
    with pytest.raises(ValueError):
        op(probs, labels[:-1])


# ---- end to end
def _residue_graph(z, tag):
    from deepinteract_amd.graph import ResidueGraph
    it = chain_item(z, tag)
    g = ResidueGraph(it["src"], it["dst"], it["num_nodes"])
    g.ndata["f"], g.edata["f"] = it["node_f"], it["edge_f"]
    g.edata["src_nbr_e_ids"], g.edata["dst_nbr_e_ids"] = it["src_nbr"], it["dst_nbr"]
    return g.to("cuda")


def test_litgini_test_step_end_to_end():
    from deepinteract_amd.modules import LitGINI
    from deepinteract_amd.ranking import confusion_metrics
    from deepinteract_amd.weights import seeded_state_dict
    z = load_case("c1")
    model = LitGINI(dtype="f32", precise_head=True).cuda().eval().load_reference_state_dict(seeded_state_dict(0))
    l1, l2 = int(z["logits"].shape[2]), int(z["logits"].shape[3])
    g = torch.Generator().manual_seed(9)
    lab = (torch.rand(l1 * l2, generator=g) < 0.05).long()
    i, j = torch.meshgrid(torch.arange(l1), torch.arange(l2), indexing="ij")
    examples = torch.stack((i.flatten(), j.flatten(), lab), dim=1)   # row-major
    with torch.no_grad():
        out = model.test_step((_residue_graph(z, "g1"), _residue_graph(z, "g2"), [examples],
                               ["/data/test/4heq_l_u.dill"]), 0)
    torch.cuda.synchronize()
    u2, auroc, auprc, (P, N, nan, U) = ref_auc(out["test_preds"], out["test_labels"])
    assert P == int(lab.sum()) and nan == 0 and U > 0
    print(f"test_step: test_auroc {out['test_auroc']:.17g} (ref {auroc:.17g}), "
          f"test_auprc {out['test_auprc']:.17g} (ref {auprc:.17g}), U = {U}")
    assert abs(out["test_auroc"] - auroc) <= 2 * EPS * auroc
    assert abs(out["test_auprc"] - auprc) <= (U + 2) * EPS * auprc
    assert {k: out[k] for k in ("test_acc", "test_prec", "test_recall", "test_f1")} == \
        confusion_metrics(**out["confusion"])
    c = out["confusion"]
    assert c["tp"] + c["fn"] == P and sum(c.values()) == l1 * l2
    assert out["test_recall"] == (c["tp"] / P) == out["test_acc"]
    for key in ("loss", "top_10_prec", "top_l_by_10_prec", "top_l_by_5_prec", "top_l_recall", "top_l_by_2_recall",
                "top_l_by_5_recall", "test_preds", "test_preds_rounded", "test_labels", "target", "confusion"):
        assert key in out, key
