"""Ranked contacts and LitGINI.test_step's top-k metrics from the head's logits.

The reference judges a prediction through its ranked contacts: top-10 / top-L/10 / top-L/5 precision
and top-L / L/2 / L/5 recall of ``LitGINI.test_step`` (deepinteract_modules.py:2018-2101,
``calculate_top_k_prec`` / ``calculate_top_k_recall`` deepinteract_utils.py:977-995), with
L = min(L1, L2). ``ContactRankOp`` produces, on the device and without sorting the L1 * L2 map, the
contact-probability map, its K best contacts and -- given labels -- the counters those metrics are
made of (csrc/contact_rank.hip, ``di_contact_rank``).

Order: probability descending, equal probabilities by ascending flat index ``i * L2 + j``, NaN above
every number -- ``torch.sort(descending=True, stable=True)`` of the stored map. The maps saturate to
exactly 1.0, so ties are common; ``argsort`` / ``topk`` leave their order undefined.

``ContactAucOp`` gives the same step's exact per-complex ``test_auroc`` / ``test_auprc`` (class 1:
roc_curve + trapezoid and average precision over the distinct thresholds, what torchmetrics' exact
mode and scikit-learn compute) from that stored map and its labels, again without sorting the map
(csrc/contact_auc.hip, ``di_contact_auc``): the sorted positive scores plus a histogram of the
negatives over the gaps between them determine both. ``confusion_metrics`` restates torchmetrics'
test_acc / test_prec / test_recall / test_f1 from ``tp, fp, fn, tn``.

Out of scope: sending top-k lists instead of maps through ``predict_sharded``.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .engine import _ptr, _stream, check_on, gpu_device


class ContactRanking:
    """Result of one ``ContactRankOp`` call (device tensors; label fields None without labels).

    probs [L1, L2] fp32; ids [K] int32 flat indices in rank order; pairs [K, 2] their (i, j);
    scores [K] fp32; hits [K] int32, hits[r] = positives among ranks 0..r. ``num_pos, tp, fp, fn,
    tn, ce_sum`` are host numbers, read from the device on first use with one copy (which waits for
    the stream the op ran on)."""

    _FIELDS = tuple(f for f, _ in _lib.DiRankMetrics._fields_)

    def __init__(self, probs, ids, scores, hits, metrics_dev, l2):
        self.probs, self.ids, self.scores, self.hits = probs, ids, scores, hits
        self._metrics_dev, self._metrics, self._l2 = metrics_dev, None, l2

    @property
    def pairs(self):
        i = torch.div(self.ids, self._l2, rounding_mode="floor")
        return torch.stack((i, self.ids - i * self._l2), dim=1)

    def metrics(self) -> dict:
        if self._metrics_dev is None:
            raise ValueError("the ranking was computed without labels")
        if self._metrics is None:
            raw = self._metrics_dev.cpu().numpy().tobytes()
            m = _lib.DiRankMetrics.from_buffer_copy(raw)
            self._metrics = {f: getattr(m, f) for f in self._FIELDS}
        return self._metrics

    def __getattr__(self, name):
        if name in ContactRanking._FIELDS:
            return None if self._metrics_dev is None else self.metrics()[name]
        raise AttributeError(name)


class ContactRankOp:
    """softmax(logits)[1], its K best contacts and test_step's counters for one complex on HIP.

    logits: [1, 2, L1, L2] contiguous, fp32 or bf16, on the op's GPU. No CPU fallback. The workspace
    is reused between calls; calls on one stream need no synchronisation between them."""

    def __init__(self, device="cuda"):
        self.device = gpu_device(device)
        self.lib = _lib.load()
        self._work = None

    def _workspace(self, n, k):
        nb = self.lib.di_contact_rank_work_bytes(n, k)
        if nb < 0:
            raise ValueError(f"contact ranking of {n} elements, k = {k}: code {nb} "
                             f"(1 <= k <= min(n, {_lib.DI_RANK_MAX_K}), n < 2^29)")
        if self._work is None or self._work.numel() * 8 < nb:
            self._work = torch.empty((nb + 7) // 8, dtype=torch.int64, device=self.device)
        return self._work

    def __call__(self, logits, k=None, labels=None, threshold=0.5, probs_out=None):
        if logits.dim() != 4 or logits.shape[0] != 1 or logits.shape[1] != 2 or not logits.is_contiguous():
            raise ValueError("contact ranking takes one contiguous [1, 2, L1, L2] logits tensor")
        if logits.dtype == torch.float32:
            dt = _lib.DI_F32
        elif logits.dtype == torch.bfloat16:
            dt = _lib.DI_BF16
        else:
            raise TypeError(f"contact ranking takes fp32 / bf16 logits, got {logits.dtype}")
        l1, l2 = int(logits.shape[2]), int(logits.shape[3])
        n = l1 * l2
        k = min(l1, l2) if k is None else int(k)
        check_on(self.device, "ContactRankOp", logits, labels, probs_out)
        if labels is not None:
            if labels.dtype != torch.uint8 or labels.numel() != n or not labels.is_contiguous():
                raise ValueError("labels: a contiguous uint8 tensor of L1 * L2 elements")
        if probs_out is None:
            probs = torch.empty(l1, l2, dtype=torch.float32, device=self.device)
        else:
            probs = probs_out
            if probs.dtype != torch.float32 or tuple(probs.shape) != (l1, l2) or not probs.is_contiguous():
                raise ValueError("probs_out: a contiguous fp32 [L1, L2] tensor")
        work = self._workspace(n, k)
        ids = torch.empty(k, dtype=torch.int32, device=self.device)
        scores = torch.empty(k, dtype=torch.float32, device=self.device)
        hits = metrics = None
        if labels is not None:
            hits = torch.empty(k, dtype=torch.int32, device=self.device)
            metrics = torch.empty(ctypes.sizeof(_lib.DiRankMetrics) // 8, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.di_contact_rank(dt, _ptr(logits), l1, l2, k, _ptr(labels), ctypes.c_float(threshold),
                                            _ptr(probs), _ptr(ids), _ptr(scores), _ptr(hits), _ptr(metrics),
                                            _ptr(work), _stream()), "di_contact_rank")
        return ContactRanking(probs, ids, scores, hits, metrics, l2)


class ContactAuc:
    """Result of one ``ContactAucOp`` call. ``num_pos, num_neg, num_nan, pos_distinct, u2, auroc,
    auprc, overflow`` are host numbers, read from the device on first use with one copy (which waits
    for the stream the op ran on). u2 = sum over (positive, negative) pairs of 2 [p_pos > p_neg] +
    [p_pos == p_neg]; auroc = u2 / (2 num_pos num_neg); both figures are float('nan') when a class is
    empty or a score is NaN (then u2 = pos_distinct = 0). ``rerun(num_pos)``, if given, runs the op
    again with room for every positive: used once, on that first read, if this run overflowed."""

    _FIELDS = tuple(f for f, _ in _lib.DiAucMetrics._fields_ if f != "pad")

    def __init__(self, metrics_dev, max_pos, rerun=None):
        self._metrics_dev, self._metrics, self.max_pos, self._rerun = metrics_dev, None, max_pos, rerun

    def _read(self) -> dict:
        m = _lib.DiAucMetrics.from_buffer_copy(self._metrics_dev.cpu().numpy().tobytes())
        return {f: getattr(m, f) for f in self._FIELDS}

    def metrics(self) -> dict:
        if self._metrics is None:
            m = self._read()
            if m["overflow"] and self._rerun is not None:
                again = self._rerun(m["num_pos"])
                self._metrics_dev, self.max_pos = again._metrics_dev, again.max_pos
                m = self._read()
            self._metrics, self._rerun = m, None
        return self._metrics

    def __getattr__(self, name):
        if name in ContactAuc._FIELDS:
            return self.metrics()[name]
        raise AttributeError(name)


class ContactAucOp:
    """Exact AUROC and average precision of class 1 for one complex on HIP, from the fp32 map
    ``ContactRankOp`` stored (values in [0, 1] or NaN) and its uint8 labels, so that ranking and AUC
    judge the same numbers. No CPU fallback. The workspace is reused between calls; calls on one
    stream need no synchronisation between them.

    ``max_pos`` sizes the positives' buffer (default ``min(n, max(65536, n // 16))``: contact labels
    are sparse). If a map holds more positives the op runs once more with ``max_pos = num_pos`` when
    the metrics are first read, so any label density works and the common case keeps a small
    workspace; the result keeps ``probs`` and ``labels`` alive until then, and they must not be
    overwritten before the metrics are read."""

    def __init__(self, device="cuda"):
        self.device = gpu_device(device)
        self.lib = _lib.load()
        self._work = None

    @staticmethod
    def default_max_pos(n: int) -> int:
        return min(n, max(65536, n // 16))

    @staticmethod
    def check_args(probs, labels, max_pos=None) -> int:
        """Raises on arguments di_contact_auc cannot take; returns max_pos (the default if None)."""
        if probs.dtype != torch.float32 or probs.dim() != 2 or not probs.is_contiguous():
            raise ValueError("contact AUC takes one contiguous fp32 [L1, L2] probability map")
        n = probs.numel()
        if n < 1:
            raise ValueError("contact AUC: an empty map")
        if labels.dtype != torch.uint8 or labels.numel() != n or not labels.is_contiguous():
            raise ValueError("labels: a contiguous uint8 tensor of L1 * L2 elements")
        max_pos = ContactAucOp.default_max_pos(n) if max_pos is None else int(max_pos)
        if max_pos < 1 or max_pos > n:
            raise ValueError(f"max_pos = {max_pos}: 1 <= max_pos <= n = {n}")
        return max_pos

    def _workspace(self, n, max_pos):
        nb = self.lib.di_contact_auc_work_bytes(n, max_pos)
        if nb < 0:
            raise ValueError(f"contact AUC of {n} elements, max_pos = {max_pos}: code {nb} "
                             "(1 <= max_pos <= n < 2^29)")
        if self._work is None or self._work.numel() * 8 < nb:
            self._work = torch.empty((nb + 7) // 8, dtype=torch.int64, device=self.device)
        return self._work

    def _run(self, probs, labels, max_pos):
        n = probs.numel()
        work = self._workspace(n, max_pos)
        out = torch.empty(ctypes.sizeof(_lib.DiAucMetrics) // 8, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.di_contact_auc(_ptr(probs), _ptr(labels), n, max_pos, _ptr(out), _ptr(work), _stream()),
                   "di_contact_auc")
        return ContactAuc(out, max_pos)

    def __call__(self, probs, labels, max_pos=None):
        max_pos = self.check_args(probs, labels, max_pos)
        check_on(self.device, "ContactAucOp", probs, labels)
        res = self._run(probs, labels, max_pos)
        res._rerun = lambda num_pos: self._run(probs, labels, num_pos)   # keeps probs and labels alive
        return res


def confusion_metrics(tp, fp, fn, tn) -> dict:
    """test_acc / test_prec / test_recall / test_f1 of LitGINI.test_step from the confusion counts at
    pos_prob_threshold, as torchmetrics' multiclass (num_classes=2, average=None) metrics define them
    for class 1: precision tp / (tp + fp), recall tp / (tp + fn), F1 2 tp / (2 tp + fp + fn), and the
    per-class accuracy, which for class 1 is tp / (tp + fn) too; a zero denominator gives 0.0
    (torchmetrics' ``_safe_divide``). ``tn`` enters none of the four. Restated from the published
    definitions, not executed: torchmetrics is not a dependency of this package or of its tests."""
    tp, fp, fn, tn = int(tp), int(fp), int(fn), int(tn)

    def div(a, b):
        return a / b if b else 0.0

    return {"test_acc": div(tp, tp + fn), "test_prec": div(tp, tp + fp), "test_recall": div(tp, tp + fn),
            "test_f1": div(2 * tp, 2 * tp + fp + fn)}


def labels_from_examples(examples, l1: int, l2: int):
    """The reference's ``examples`` [n, 3] = (i, j, label) rows of one complex as a uint8 [l1 * l2]
    label map on the device of ``examples``. Raises ValueError unless the rows cover every pair
    exactly once with indices in range and labels in {0, 1}."""
    if examples.dim() != 2 or examples.shape[1] != 3:
        raise ValueError("examples: [n, 3] rows of (i, j, label)")
    n = l1 * l2
    if examples.shape[0] != n:
        raise ValueError(f"examples: {examples.shape[0]} rows for {l1} x {l2} = {n} pairs "
                         "(every pair exactly once)")
    ex = examples.to(torch.int64)
    i, j, lab = ex[:, 0], ex[:, 1], ex[:, 2]
    if bool(((i < 0) | (i >= l1) | (j < 0) | (j >= l2)).any()):
        raise ValueError("examples: a pair index outside the complex")
    if bool(((lab != 0) & (lab != 1)).any()):
        raise ValueError("examples: labels must be 0 or 1")
    flat = i * l2 + j
    seen = torch.zeros(n, dtype=torch.int32, device=examples.device)
    seen.index_add_(0, flat, torch.ones(n, dtype=torch.int32, device=examples.device))
    if bool((seen != 1).any()):
        raise ValueError("examples: a pair is missing or listed twice")
    out = torch.zeros(n, dtype=torch.uint8, device=examples.device)
    out[flat] = lab.to(torch.uint8)
    return out


def topk_metrics(hits, num_pos, l: int) -> dict:
    """The six top-k figures of LitGINI.test_step from ``hits`` (hits[r] = positives among ranks
    0..r; a tensor, array or list) with the reference's arithmetic (deepinteract_utils.py:977-995):
    precision = positives among the first k / k for k in (10, l // 10, l // 5); recall = positives
    among the first k / num_pos for k in (l, l // 2, l // 5).

    Where the reference divides by zero or slices past the ranking the figure is float('nan'):
    k = 0 (l < 10 for l // 10, l < 5 for l // 5, l < 2 for l // 2), num_pos = 0 (recall), and
    k > len(hits) (the ranking was cut shorter than k)."""
    K = len(hits)
    num_pos = int(num_pos)

    def top(k):
        return None if k < 1 or k > K else int(hits[k - 1])

    def prec(k):
        h = top(k)
        return float("nan") if h is None else h / k

    def recall(k):
        h = top(k)
        return float("nan") if h is None or num_pos == 0 else h / num_pos

    return {"top_10_prec": prec(10), "top_l_by_10_prec": prec(l // 10), "top_l_by_5_prec": prec(l // 5),
            "top_l_recall": recall(l), "top_l_by_2_recall": recall(l // 2), "top_l_by_5_recall": recall(l // 5)}


__all__ = ["ContactRankOp", "ContactRanking", "ContactAucOp", "ContactAuc", "confusion_metrics",
           "labels_from_examples", "topk_metrics"]
