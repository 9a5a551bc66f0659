"""Exact per-complex AUROC / AUPRC without a GPU: ``ref_auc``, the yardstick of the GPU tests, pinned to
scikit-learn; di_contact_auc's host contract (sizes, every refusal before a launch, the DiAucMetrics
layout); ranking.confusion_metrics; ContactAucOp's argument checks.

``ref_auc`` restates the definitions of include/deepinteract_amd.h by sorting the whole map and
grouping ties (the device sorts only the positives and bins the negatives): with the positives grouped
by distinct score, descending, c_g per group, TP_g = c_0 + .. + c_g and FP_g = negatives scoring at
least group g's score,
    u2 = sum_g c_g (2 (N - FP_g) + E_g)     E_g = negatives scoring exactly group g's score
    auroc = u2 / (2 P N)                    Python's int / int: the correctly rounded quotient
    auprc = (1 / P) sum_g c_g TP_g / (TP_g + FP_g)
The auprc terms are formed and summed in numpy's extended precision (64-bit significand on x86), so
the yardstick's own error stays far under the bounds the tests apply to the device's fp64 sum.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from deepinteract_amd import _lib
from gpu_common import load_case
from test_capi import _declared_arg_counts, _declared_struct_fields

EINVAL, ERANGE = -1, -2
EPS = 2.0 ** -53


def ref_auc(probs, labels):
    """(u2, auroc, auprc, (num_pos, num_neg, num_nan, pos_distinct)) of a score map and its labels
    (arrays of any shape; non-zero label = positive). NaN figures, u2 = pos_distinct = 0 when a class
    is empty or a score is NaN."""
    p = np.asarray(probs, dtype=np.float64).ravel()
    pos = np.asarray(labels).ravel() != 0
    P, N, nan = int(pos.sum()), int((~pos).sum()), int(np.isnan(p).sum())
    if P == 0 or N == 0 or nan:
        return 0, float("nan"), float("nan"), (P, N, nan, 0)
    order = np.argsort(-p, kind="stable")
    ps, ys = p[order], pos[order]
    last = np.flatnonzero(np.append(ps[1:] != ps[:-1], True))     # last element of every tie group
    tp_all = np.cumsum(ys)[last]                                   # positives scoring >= the group's score
    fp_all = np.cumsum(~ys)[last]
    c_all = np.diff(tp_all, prepend=0)
    e_all = np.diff(fp_all, prepend=0)
    has_pos = c_all > 0
    c, tp, fp, e = (a[has_pos] for a in (c_all, tp_all, fp_all, e_all))
    u2 = int((c.astype(np.int64) * (2 * (N - fp.astype(np.int64)) + e)).sum())    # <= 2 P N < 2^59: exact
    ld = np.longdouble
    ap = float((c.astype(ld) * tp.astype(ld) / (tp + fp).astype(ld)).sum() / ld(P))
    return u2, u2 / (2 * P * N), ap, (P, N, 0, int(has_pos.sum()))


def bernoulli(n, share, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, generator=g) < share).numpy().astype(np.uint8)


def _sklearn_cases():
    z = load_case("c1")
    c1 = np.asarray(z["probs"], dtype=np.float32).reshape(-1)
    yield "c1 golden, 1 % positives", c1, bernoulli(c1.size, 0.01, 1)
    g = torch.Generator().manual_seed(2)
    q = (torch.rand(300 * 300, generator=g).pow(3) * 29).round() / 29      # ~30 distinct values
    yield "300 x 300, 30 distinct values", q.numpy().astype(np.float32), bernoulli(q.numel(), 0.02, 3)
    d = torch.rand(64 * 64, generator=g).numpy().astype(np.float32)
    yield "64 x 64, 50 % positives", d, bernoulli(d.size, 0.5, 4)


def test_ref_auc_is_scikit_learns():
    metrics = pytest.importorskip("sklearn.metrics")
    for name, p, y in _sklearn_cases():
        u2, auroc, auprc, (P, N, nan, U) = ref_auc(p, y)
        assert P > 0 and N > 0 and nan == 0 and P + N == p.size and 0 < U <= P
        roc = float(metrics.roc_auc_score(y, p.astype(np.float64)))
        ap = float(metrics.average_precision_score(y, p.astype(np.float64)))
        e_roc, e_ap = abs(auroc - roc) / roc, abs(auprc - ap) / ap
        print(f"{name}: P = {P}, U = {U}, auroc {auroc:.17g} (rel. diff {e_roc:.2e}), "
              f"auprc {auprc:.17g} (rel. diff {e_ap:.2e})")
        assert e_roc <= 4 * EPS and e_ap <= 4 * EPS


def test_ref_auc_by_hand():
    # scores 0.9+ 0.8- 0.8+ 0.3- 0.1+ : pairs (pos, neg): 0.9>0.8, 0.9>0.3, 0.8=0.8, 0.8>0.3, 0.1<both
    u2, auroc, auprc, counts = ref_auc([0.9, 0.8, 0.8, 0.3, 0.1], [1, 0, 1, 0, 1])
    assert u2 == 2 + 2 + 1 + 2 and auroc == 7 / 12 and counts == (3, 2, 0, 3)
    assert auprc == pytest.approx((1 / 1 + 2 / 3 + 3 / 5) / 3, rel=4 * EPS)
    assert ref_auc([0.5, 0.5, 0.5], [1, 0, 0])[1:3] == (0.5, 1 / 3)
    for p, y, counts in (([0.5], [1], (1, 0, 0, 0)), ([0.5], [0], (0, 1, 0, 0)),
                         ([0.5, float("nan")], [1, 0], (1, 1, 1, 0))):
        u2, auroc, auprc, got = ref_auc(p, y)
        assert u2 == 0 and math.isnan(auroc) and math.isnan(auprc) and got == counts


def test_work_bytes_contract():
    lib = _lib.load()
    wb = lib.di_contact_auc_work_bytes
    assert wb(0, 1) == EINVAL and wb(-4, 1) == EINVAL
    assert wb(10, 0) == EINVAL and wb(10, -1) == EINVAL and wb(10, 11) == EINVAL
    assert wb(1 << 29, 10) == ERANGE and wb(1 << 62, 10) == ERANGE
    assert wb(1, 1) > 0 and wb((1 << 29) - 1, (1 << 29) - 1) > 0
    last = 0
    for max_pos in (1, 4096, 4097, 65536, 10 ** 6):
        b = wb(10 ** 6, max_pos)
        assert b > last and b % 4 == 0
        last = b
    assert wb(4096 * 4096, 10) == wb(10 ** 6, 10)      # the positives' buffers, not the map, size it


def test_contact_auc_refusals_without_gpu():
    """Every refusal happens before any launch: the dummy non-NULL pointers are never dereferenced."""
    lib = _lib.load()
    p, odd = ctypes.c_void_p(16), ctypes.c_void_p(24)

    def call(probs=p, labels=p, n=4096, max_pos=100, out=p, work=p):
        return lib.di_contact_auc(probs, labels, n, max_pos, out, work, None)

    assert call(n=0) == EINVAL and call(n=-1) == EINVAL
    assert call(max_pos=0) == EINVAL and call(max_pos=4097) == EINVAL
    for name in ("probs", "labels", "out", "work"):
        assert call(**{name: None}) == EINVAL, name
    assert call(probs=odd) == EINVAL and call(work=odd) == EINVAL
    assert call(n=1 << 29) == ERANGE


def test_auc_metrics_layout_and_signatures():
    assert ctypes.sizeof(_lib.DiAucMetrics) == 64
    assert [f for f, _ in _lib.DiAucMetrics._fields_] == _declared_struct_fields("di_auc_metrics")
    assert [t for _, t in _lib.DiAucMetrics._fields_] == \
        [ctypes.c_int64] * 4 + [ctypes.c_uint64] + [ctypes.c_double] * 2 + [ctypes.c_int32] * 2
    decl = _declared_arg_counts()
    assert decl["di_contact_auc"] == 7 == len(_lib._SIGS["di_contact_auc"][0])
    assert decl["di_contact_auc_work_bytes"] == 2 == len(_lib._SIGS["di_contact_auc_work_bytes"][0])
    assert _lib.load().di_abi_version() == _lib.ABI_VERSION == 8


def test_confusion_metrics():
    from deepinteract_amd.ranking import confusion_metrics
    m = confusion_metrics(tp=30, fp=10, fn=20, tn=940)
    assert m == {"test_acc": 30 / 50, "test_prec": 30 / 40, "test_recall": 30 / 50, "test_f1": 60 / 90}
    assert confusion_metrics(0, 0, 0, 0) == {"test_acc": 0.0, "test_prec": 0.0, "test_recall": 0.0, "test_f1": 0.0}
    assert confusion_metrics(0, 0, 0, 100) == confusion_metrics(0, 0, 0, 0)      # tn enters none of them
    assert confusion_metrics(0, 5, 0, 0) == {"test_acc": 0.0, "test_prec": 0.0, "test_recall": 0.0, "test_f1": 0.0}
    assert confusion_metrics(0, 0, 5, 0)["test_recall"] == 0.0
    assert confusion_metrics(7, 0, 0, 0) == {"test_acc": 1.0, "test_prec": 1.0, "test_recall": 1.0, "test_f1": 1.0}
    t = confusion_metrics(torch.tensor(3), torch.tensor(1), torch.tensor(2), torch.tensor(4))   # counts of any int type
    assert t == confusion_metrics(3, 1, 2, 4) and all(type(v) is float for v in t.values())


def test_auc_op_argument_errors():
    from deepinteract_amd.ranking import ContactAucOp
    assert ContactAucOp.default_max_pos(15) == 15
    assert ContactAucOp.default_max_pos(10 ** 6) == 65536
    assert ContactAucOp.default_max_pos(4096 * 4096) == 1 << 20
    probs, labels = torch.rand(5, 7), torch.zeros(35, dtype=torch.uint8)
    assert ContactAucOp.check_args(probs, labels) == 35
    assert ContactAucOp.check_args(probs, labels.view(5, 7), max_pos=3) == 3
    for bad_probs in (probs.double(), probs.flatten(), probs.t(), torch.empty(0, 7)):
        with pytest.raises(ValueError):
            ContactAucOp.check_args(bad_probs, labels)
    for bad_labels in (labels.long(), labels[:-1], torch.zeros(70, dtype=torch.uint8)[::2]):
        with pytest.raises(ValueError):
            ContactAucOp.check_args(probs, bad_labels)
    for bad in (0, -1, 36):
        with pytest.raises(ValueError):
            ContactAucOp.check_args(probs, labels, max_pos=bad)
    with pytest.raises(RuntimeError):
        ContactAucOp("cpu")                       # no CPU fallback
