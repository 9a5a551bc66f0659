"""Contact ranking without a GPU: di_contact_rank's host contract (sizes, every refusal before a
launch), the DiRankMetrics layout, ranking.topk_metrics against a restatement of the reference's
calculate_top_k_prec / calculate_top_k_recall (deepinteract_utils.py:977-995), and the validation of
ranking.labels_from_examples."""
import ctypes
import math

import pytest
import torch

from deepinteract_amd import _lib
from test_capi import _declared_arg_counts, _declared_struct_fields

EINVAL, ERANGE = -1, -2


def test_work_bytes_contract():
    lib = _lib.load()
    wb = lib.di_contact_rank_work_bytes
    last = 0
    for n in (1, 15, 145 * 145, 10 ** 6, 4096 * 4096, (1 << 29) - 1):
        b = wb(n, 1)
        assert b > 0 and b >= last, (n, b, last)
        last = b
    assert wb(4096 * 4096, 4096) >= wb(4096 * 4096, 1) > 0
    assert wb(0, 1) == EINVAL and wb(10, 0) == EINVAL and wb(10, 11) == EINVAL
    assert wb(-5, 1) == EINVAL and wb(10, -1) == EINVAL
    assert wb(1 << 20, 4097) == ERANGE
    assert wb(1 << 29, 10) == ERANGE
    assert wb(1 << 62, 10) == ERANGE


def test_contact_rank_refusals_without_gpu():
    """Every refusal happens before any launch: the dummy non-NULL pointers are never dereferenced."""
    lib = _lib.load()
    p, odd = ctypes.c_void_p(16), ctypes.c_void_p(24)
    thr = ctypes.c_float(0.5)

    def call(dtype=_lib.DI_F32, logits=p, l1=64, l2=64, k=10, labels=None, threshold=thr, probs=p, ids=p,
             scores=p, hits=None, metrics=None, work=p):
        return lib.di_contact_rank(dtype, logits, l1, l2, k, labels, threshold, probs, ids, scores, hits, metrics,
                                   work, None)

    assert call(l1=0) == EINVAL and call(l2=0) == EINVAL and call(l1=-3) == EINVAL
    assert call(k=0) == EINVAL and call(k=-1) == EINVAL
    assert call(l1=3, l2=3, k=10) == EINVAL                      # k > n
    assert call(dtype=2) == EINVAL and call(dtype=-1) == EINVAL
    for name in ("logits", "probs", "ids", "scores", "work"):
        assert call(**{name: None}) == EINVAL, name
    for labels, hits, metrics in ((p, None, None), (None, p, None), (None, None, p), (p, p, None), (p, None, p),
                                  (None, p, p)):
        assert call(labels=labels, hits=hits, metrics=metrics) == EINVAL
    assert call(threshold=ctypes.c_float(float("nan"))) == EINVAL
    assert call(probs=odd) == EINVAL and call(work=odd) == EINVAL
    assert call(l1=100, l2=100, k=4097) == ERANGE
    assert call(l1=1 << 15, l2=1 << 14) == ERANGE                # n = 2^29
    assert call(l1=(1 << 31) - 1, l2=(1 << 31) - 1) == ERANGE    # the product stays inside int64
    # k > n is a bad argument even when k is also over the limit
    assert call(l1=10, l2=10, k=5000) == EINVAL


def test_rank_metrics_layout_and_signatures():
    assert ctypes.sizeof(_lib.DiRankMetrics) == 48
    assert [f for f, _ in _lib.DiRankMetrics._fields_] == _declared_struct_fields("di_rank_metrics")
    assert [t for _, t in _lib.DiRankMetrics._fields_] == [ctypes.c_int64] * 5 + [ctypes.c_double]
    decl = _declared_arg_counts()
    assert decl["di_contact_rank"] == 14 == len(_lib._SIGS["di_contact_rank"][0])
    assert decl["di_contact_rank_work_bytes"] == 2 == len(_lib._SIGS["di_contact_rank_work_bytes"][0])
    assert _lib.DI_RANK_MAX_K == 4096
    assert _lib.load().di_abi_version() == 8


# ---- the reference's arithmetic, restated (deepinteract_utils.py:977-995)
def ref_top_k_prec(sorted_pred_indices, labels, k):
    return torch.sum(labels[sorted_pred_indices[:k]]).item() / k


def ref_top_k_recall(sorted_pred_indices, labels, k):
    return torch.sum(labels[sorted_pred_indices[:k]]).item() / torch.sum(labels).item()


def _hand_ranking(l, seed, positives=True):
    """A ranking of l * l elements cut at K = l (the op's default) and its labels."""
    g = torch.Generator().manual_seed(seed)
    n = l * l
    labels = (torch.rand(n, generator=g) < 0.3).long() if positives else torch.zeros(n, dtype=torch.long)
    order = torch.randperm(n, generator=g)
    hits = torch.cumsum(labels[order[:l]], 0)
    return order, labels, hits


@pytest.mark.parametrize("l", [7, 10, 145, 4096])
def test_topk_metrics_matches_reference_arithmetic(l):
    from deepinteract_amd.ranking import topk_metrics
    ln = min(l, 200)  # the map's side: the figures depend on the ranking's first l entries only
    g = torch.Generator().manual_seed(l)
    n = max(ln * ln, l)
    labels = (torch.rand(n, generator=g) < 0.3).long()
    order = torch.randperm(n, generator=g)
    hits = torch.cumsum(labels[order[:l]], 0)
    got = topk_metrics(hits, int(labels.sum()), l)
    want = {"top_10_prec": (ref_top_k_prec, 10), "top_l_by_10_prec": (ref_top_k_prec, l // 10),
            "top_l_by_5_prec": (ref_top_k_prec, l // 5), "top_l_recall": (ref_top_k_recall, l),
            "top_l_by_2_recall": (ref_top_k_recall, l // 2), "top_l_by_5_recall": (ref_top_k_recall, l // 5)}
    assert set(got) == set(want)
    for name, (fn, k) in want.items():
        if k == 0 or k > l:
            # the reference: ZeroDivisionError (k = 0), or a slice longer than this ranking (k > K)
            assert math.isnan(got[name]), (name, got[name])
        else:
            assert got[name] == fn(order, labels, k), (name, k)
    if l == 7:
        assert math.isnan(got["top_10_prec"]) and math.isnan(got["top_l_by_10_prec"])
        assert not math.isnan(got["top_l_by_5_prec"]) and not math.isnan(got["top_l_recall"])
    # the same from a list and a numpy array
    assert topk_metrics(hits.tolist(), int(labels.sum()), l) == pytest.approx(got, nan_ok=True)
    assert topk_metrics(hits.numpy(), int(labels.sum()), l) == pytest.approx(got, nan_ok=True)


def test_topk_metrics_without_positives():
    from deepinteract_amd.ranking import topk_metrics
    order, labels, hits = _hand_ranking(145, 3, positives=False)
    got = topk_metrics(hits, 0, 145)
    for name in ("top_l_recall", "top_l_by_2_recall", "top_l_by_5_recall"):
        assert math.isnan(got[name])          # the reference: ZeroDivisionError
    for name, k in (("top_10_prec", 10), ("top_l_by_10_prec", 14), ("top_l_by_5_prec", 29)):
        assert got[name] == 0.0 == ref_top_k_prec(order, labels, k)


def _examples(l1, l2, seed=0):
    g = torch.Generator().manual_seed(seed)
    i, j = torch.meshgrid(torch.arange(l1), torch.arange(l2), indexing="ij")
    lab = (torch.rand(l1 * l2, generator=g) < 0.2).long()
    ex = torch.stack((i.flatten(), j.flatten(), lab), dim=1)
    return ex[torch.randperm(l1 * l2, generator=g)], lab   # any row order


def test_labels_from_examples_scatter_and_refusals():
    from deepinteract_amd.ranking import labels_from_examples
    ex, lab = _examples(5, 7)
    out = labels_from_examples(ex, 5, 7)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (35,)
    assert torch.equal(out.long(), lab)
    assert torch.equal(labels_from_examples(ex.float(), 5, 7), out)   # the reference's examples may be float
    with pytest.raises(ValueError):
        labels_from_examples(ex[:-1], 5, 7)                  # a missing pair
    dup = ex.clone()
    dup[3] = dup[4]
    with pytest.raises(ValueError):
        labels_from_examples(dup, 5, 7)                      # a duplicate (and so a missing) pair
    for col, val in ((0, 5), (1, 7), (0, -1)):
        bad = ex.clone()
        bad[0, col] = val
        with pytest.raises(ValueError):
            labels_from_examples(bad, 5, 7)                  # index out of range
    bad = ex.clone()
    bad[2, 2] = 2
    with pytest.raises(ValueError):
        labels_from_examples(bad, 5, 7)                      # a label of 2
    with pytest.raises(ValueError):
        labels_from_examples(ex[:, :2], 5, 7)
