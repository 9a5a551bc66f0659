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

``ContactRankOp.batch`` / ``ContactAucOp.batch`` run either op over many complexes of different shapes
with one launch sequence (``di_contact_rank_batch`` / ``di_contact_auc_batch``) and give every complex
the bits of the single call; ``labels_from_examples_batch`` validates a batch's labels with one host
read. ``ExamplesOp`` reads the example lists on the device (csrc/contact_examples.hip): complete lists
as label maps, sampled lists as ``LitGINI.validation_step``'s pooled logits and labels;
``pooled_topk_metrics`` is that step's top-k arithmetic. ``InterfaceOp`` builds the label maps from the
two chains' heavy-atom coordinates instead (csrc/contact_interface.hip; ``interface_atoms`` groups a
chain's atoms for it), so a prediction can be scored from a structure, without example lists.

Across ranks: ``ContactRankOp.batch(out=...)`` / ``ContactAucOp.batch(out=...)`` write a complex's
ranked contacts and metrics into caller memory -- ``RecordSlot``, the views of one wire record
(``di_rank_record_bytes`` lays it out) in a collective's send buffer -- with the bits they have
without ``out``; ``GatheredRanking`` reads a received record. ``distributed.predict_sharded(gather=
"topk")`` sends these records instead of the maps.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .engine import _ptr, _stream, check_on, gpu_device


class _MetricsTable:
    """The metrics records of one batch, [count, words] int64 on the device: read with one copy (which
    waits for the stream the batch ran on) when the first result asks for a number."""

    def __init__(self, dev):
        self.dev, self._host = dev, None

    def row(self, i: int) -> bytes:
        if self._host is None:
            self._host = self.dev.cpu().numpy()
        return self._host[i].tobytes()


class ContactRankingBatch(list):
    """``ContactRankOp.batch``'s list of ``ContactRanking``, plus the packed buffers its elements are
    views of: ``hits`` (all complexes' top_hits, int32; None without labels) and ``hits_off`` (complex
    i's start in it), so that a caller can bring every complex's hits to the host with one copy."""

    hits = None
    hits_off = ()


class ContactRanking:
    """Result of one ``ContactRankOp`` call (device tensors; label fields None without labels).

    probs [L1, L2] fp32; ids [K] int32 flat indices in rank order; pairs [K, 2] their (i, j);
    scores [K] fp32; hits [K] int32, hits[r] = positives among ranks 0..r. ``num_pos, tp, fp, fn,
    tn, ce_sum`` are host numbers, read from the device on first use with one copy (which waits for
    the stream the op ran on); the results of one ``batch`` call share that copy (``table``, ``index``:
    the batch's metrics table and this complex's row)."""

    _FIELDS = tuple(f for f, _ in _lib.DiRankMetrics._fields_)

    def __init__(self, probs, ids, scores, hits, metrics_dev, l2, table=None, index=0):
        self.probs, self.ids, self.scores, self.hits = probs, ids, scores, hits
        self._metrics_dev, self._metrics, self._l2 = metrics_dev, None, l2
        self._table, self._index = table, index

    @property
    def pairs(self):
        i = torch.div(self.ids, self._l2, rounding_mode="floor")
        return torch.stack((i, self.ids - i * self._l2), dim=1)

    def metrics(self) -> dict:
        if self._metrics_dev is None:
            raise ValueError("the ranking was computed without labels")
        if self._metrics is None:
            raw = self._metrics_dev.cpu().numpy().tobytes() if self._table is None else self._table.row(self._index)
            m = _lib.DiRankMetrics.from_buffer_copy(raw)
            self._metrics = {f: getattr(m, f) for f in self._FIELDS}
        return self._metrics

    def __getattr__(self, name):
        if name in ContactRanking._FIELDS:
            return None if self._metrics_dev is None else self.metrics()[name]
        raise AttributeError(name)


def record_k(l1: int, l2: int, k=None) -> int:
    """Ranks a wire record keeps of an (l1, l2) complex: min(l1, l2) for k = None (test_step's
    l), else min(k, l1 * l2). A function of the sizes and the caller's k alone, so every rank of a
    process group computes every record's size. ValueError for k < 1 or a result beyond DI_RANK_MAX_K."""
    kk = min(int(l1), int(l2)) if k is None else min(int(k), int(l1) * int(l2))
    if kk < 1 or kk > _lib.DI_RANK_MAX_K:
        raise ValueError(f"a {l1} x {l2} complex with k = {k} keeps {kk} ranks: 1 <= ranks <= {_lib.DI_RANK_MAX_K}")
    return kk


_WORDS = {"metrics": ctypes.sizeof(_lib.DiRankMetrics) // 4, "auc": ctypes.sizeof(_lib.DiAucMetrics) // 4}


class RecordSlot:
    """The fields of one wire record (``_lib.rank_record_layout``: ``di_rank_record_bytes``) as views of
    ``buffer``, a contiguous 1-D int32 tensor, starting ``byte_off`` bytes into it: ``ids`` int32 [k],
    ``scores`` fp32 [k] and, with labels, ``hits`` int32 [k], ``metrics`` int64 [6] (di_rank_metrics)
    and ``auc`` int64 [8] (di_auc_metrics); None without labels. These are what ``ContactRankOp.batch``
    and ``ContactAucOp.batch`` take as ``out``. ValueError for a buffer of another dtype or layout, a
    record that does not start 16-B aligned or does not fit."""

    def __init__(self, buffer, byte_off: int, l1: int, l2: int, k: int, with_labels: bool):
        if buffer.dtype != torch.int32 or buffer.dim() != 1 or not buffer.is_contiguous():
            raise ValueError("record buffer: a contiguous 1-D int32 tensor")
        self.nbytes, self.offsets = _lib.rank_record_layout(l1, l2, k, with_labels)
        byte_off = int(byte_off)
        if byte_off < 0 or (buffer.data_ptr() + byte_off) % 16:
            raise ValueError(f"record at byte {byte_off}: records start 16-B aligned")
        if byte_off + self.nbytes > buffer.numel() * 4:
            raise ValueError(f"record of {self.nbytes} bytes at byte {byte_off} does not fit "
                             f"a buffer of {buffer.numel() * 4} bytes")
        self.buffer, self.byte_off, self.l1, self.l2, self.k = buffer, byte_off, int(l1), int(l2), int(k)
        self.with_labels = bool(with_labels)

        def words(field, count):
            if field not in self.offsets:
                return None
            at = (byte_off + self.offsets[field]) // 4
            return buffer[at:at + count]

        self.ids = words("ids", k)
        self.scores = words("scores", k).view(torch.float32)
        self.hits = words("hits", k)
        self.metrics, self.auc = (None if w is None else w.view(torch.int64)
                                  for w in (words(f, _WORDS[f]) for f in ("metrics", "auc")))


class _HostCopy:
    """A gathered record buffer, brought to the host once (which waits for the stream it was written on)
    when the first record asks for a number."""

    def __init__(self, buffer):
        self.buffer, self._host = buffer, None

    def bytes(self, lo: int, hi: int) -> bytes:
        if self._host is None:
            import numpy as np
            self._host = self.buffer.cpu().numpy().view(np.uint8)
        return self._host[lo:hi].tobytes()


class GatheredRanking:
    """One complex's received wire record (``distributed.predict_sharded(gather="topk")``): ``ids``
    [K] int32 flat indices in rank order, ``scores`` [K] fp32, ``pairs`` [K, 2] their (i, j), ``hits``
    [K] int32 (None without labels), all views of the receive buffer on its device; ``probs`` is None
    (maps are not sent). ``metrics()`` / ``auc()`` decode the record's di_rank_metrics /
    di_auc_metrics, and ContactRanking's names (``num_pos, tp, fp, fn, tn, ce_sum``) and ``auroc`` /
    ``auprc`` read them; the records of one call share one host copy of the buffer (``host``)."""

    probs = None
    _FIELDS = ContactRanking._FIELDS
    _AUC_FIELDS = tuple(f for f, _ in _lib.DiAucMetrics._fields_ if f != "pad")

    def __init__(self, buffer, byte_off, l1, l2, k, with_labels, host=None):
        slot = RecordSlot(buffer, byte_off, l1, l2, k, with_labels)
        self.ids, self.scores, self.hits = slot.ids, slot.scores, slot.hits
        self.buffer, self.byte_off, self.nbytes = buffer, slot.byte_off, slot.nbytes
        self.l1, self.l2, self.with_labels = slot.l1, slot.l2, slot.with_labels
        self._at = {f: byte_off + o for f, o in slot.offsets.items()}
        self._host = _HostCopy(buffer) if host is None else host
        self._decoded = {}

    @property
    def pairs(self):
        i = torch.div(self.ids, self.l2, rounding_mode="floor")
        return torch.stack((i, self.ids - i * self.l2), dim=1)

    def _struct(self, field, ctype, names):
        if not self.with_labels:
            raise ValueError("the record was sent without labels")
        if field not in self._decoded:
            lo = self._at[field]
            m = ctype.from_buffer_copy(self._host.bytes(lo, lo + ctypes.sizeof(ctype)))
            self._decoded[field] = {f: getattr(m, f) for f in names}
        return self._decoded[field]

    def host_array(self, field):
        """ids / scores / hits as a numpy array, from the shared host copy."""
        import numpy as np
        k = self.ids.numel()
        lo = self._at[field]
        return np.frombuffer(self._host.bytes(lo, lo + 4 * k),
                             dtype=np.float32 if field == "scores" else np.int32).copy()

    def metrics(self) -> dict:
        return self._struct("metrics", _lib.DiRankMetrics, self._FIELDS)

    def auc(self) -> dict:
        return self._struct("auc", _lib.DiAucMetrics, self._AUC_FIELDS)

    def __getattr__(self, name):
        if name in GatheredRanking._FIELDS:
            return self.metrics()[name] if self.with_labels else None
        if name in ("auroc", "auprc"):
            return self.auc()[name] if self.with_labels else None
        raise AttributeError(name)


def _check_out(what, t, dtype, length, align, device):
    """An output handed in by the caller is what the op would have allocated itself."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"out: {what} is missing")
    if t.dtype != dtype or t.dim() != 1 or t.numel() != length or not t.is_contiguous():
        raise ValueError(f"out: {what} is a contiguous {dtype} tensor of {length} elements, "
                         f"got {t.dtype} {tuple(t.shape)}")
    if t.device != device:
        raise ValueError(f"out: {what} on {t.device}, the kernels run on {device}")
    if t.data_ptr() % align:
        raise ValueError(f"out: {what} is not {align}-B aligned")
    return t


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
        return _grow(self, nb)

    def _check(self, logits, k, labels):
        """The argument checks of one complex: (dtype code, l1, l2, k)."""
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
        check_on(self.device, "ContactRankOp", logits, labels)
        if labels is not None:
            if labels.dtype != torch.uint8 or labels.numel() != n or not labels.is_contiguous():
                raise ValueError("labels: a contiguous uint8 tensor of L1 * L2 elements")
        return dt, l1, l2, k

    def __call__(self, logits, k=None, labels=None, threshold=0.5, probs_out=None):
        dt, l1, l2, k = self._check(logits, k, labels)
        n = l1 * l2
        check_on(self.device, "ContactRankOp", probs_out)
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

    def batch(self, logits_list, k=None, labels_list=None, threshold=0.5, out=None):
        """The op over many complexes of different shapes with ONE launch sequence per DI_BATCH_MAX
        complexes (``di_contact_rank_batch``): a ``ContactRankingBatch`` (a list) of ``ContactRanking``,
        each with the bits the single call gives on the same inputs. logits_list: [1, 2, L1, L2]
        tensors of one dtype (mixed: TypeError); k: None (min(L1, L2) per complex), one int, or one
        per complex; labels_list: None, or one uint8 label tensor per complex. The argument checks are
        the single op's, applied to every element. The outputs are views of packed buffers (one
        allocation per kind; every map starts 16-B aligned); the descriptor table goes to the device
        with one pinned, non-blocking copy on the current stream; the results share one metrics
        table, read from the device once, on first use.

        out (optional): one slot per complex (``RecordSlot``, or anything with these attributes) whose
        ``ids`` int32 [k], ``scores`` fp32 [k] and, with labels, ``hits`` int32 [k] and ``metrics``
        int64 [6] (8-B aligned) tensors receive the outputs instead of the op's own buffers: the item
        table's top_ids / top_scores / top_hits / metrics pointers name them, the kernels and every
        output bit are those of the call without ``out``, and nothing is packed or copied afterwards.
        Another dtype, length, device, layout or alignment raises ValueError before any launch. The
        maps stay the op's own allocation; the batch's packed ``hits`` is None, and each result reads
        its own metrics record."""
        count = len(logits_list)
        if count < 1:
            raise ValueError("contact ranking: an empty batch")
        if out is not None and len(out) != count:
            raise ValueError("contact ranking: one out slot per complex")
        ks = list(k) if isinstance(k, (list, tuple)) else [k] * count
        if labels_list is not None and len(labels_list) != count or len(ks) != count:
            raise ValueError("contact ranking: one k and one labels tensor per complex")
        with_labels = labels_list is not None
        checked = [self._check(lg, ks[i], labels_list[i] if with_labels else None) for i, lg in enumerate(logits_list)]
        if any(c[0] != checked[0][0] for c in checked):
            raise TypeError("contact ranking: one batch takes logits of one dtype")
        dt = checked[0][0]
        for _, l1, l2, kk in checked:   # sizes only: raises as the single op does
            if self.lib.di_contact_rank_work_bytes(l1 * l2, kk) < 0:
                self._workspace(l1 * l2, kk)
        map_off, k_off, at_map, at_k = [], [], 0, 0
        for _, l1, l2, kk in checked:
            map_off.append(at_map)
            k_off.append(at_k)
            at_map += (l1 * l2 + 3) // 4 * 4
            at_k += kk
        dev = self.device
        words = ctypes.sizeof(_lib.DiRankMetrics) // 8
        if out is not None:     # the caller's memory: checked against what is allocated below
            for slot, (_, _, _, kk) in zip(out, checked):
                _check_out("ids", slot.ids, torch.int32, kk, 4, dev)
                _check_out("scores", slot.scores, torch.float32, kk, 4, dev)
                if with_labels:
                    _check_out("hits", slot.hits, torch.int32, kk, 4, dev)
                    _check_out("metrics", slot.metrics, torch.int64, words, 8, dev)
        probs = torch.empty(at_map, dtype=torch.float32, device=dev)
        ids = scores = hits = metrics = table = None
        if out is None:
            ids = torch.empty(at_k, dtype=torch.int32, device=dev)
            scores = torch.empty(at_k, dtype=torch.float32, device=dev)
            hits = torch.empty(at_k, dtype=torch.int32, device=dev) if with_labels else None
            metrics = torch.empty(count, words, dtype=torch.int64, device=dev) if with_labels else None
            table = _MetricsTable(metrics) if with_labels else None
        res = ContactRankingBatch()
        res.hits, res.hits_off = hits, tuple(k_off)
        items = (_lib.DiRankItem * count)()
        for i, (lg, (_, l1, l2, kk)) in enumerate(zip(logits_list, checked)):
            n = l1 * l2
            if out is None:
                mine = (ids[k_off[i]:k_off[i] + kk], scores[k_off[i]:k_off[i] + kk],
                        hits[k_off[i]:k_off[i] + kk] if with_labels else None, metrics[i] if with_labels else None)
            else:
                mine = (out[i].ids, out[i].scores, out[i].hits if with_labels else None,
                        out[i].metrics if with_labels else None)
            r = ContactRanking(probs[map_off[i]:map_off[i] + n].view(l1, l2), *mine, l2, table, i)
            res.append(r)
            it = items[i]
            it.logits, it.probs, it.top_ids, it.top_scores = (t.data_ptr() for t in (lg, r.probs, r.ids, r.scores))
            if with_labels:
                it.labels, it.top_hits, it.metrics = labels_list[i].data_ptr(), r.hits.data_ptr(), mine[3].data_ptr()
            it.l1, it.l2, it.k = l1, l2, kk
        for lo in range(0, count, _lib.DI_BATCH_MAX):
            m = min(_lib.DI_BATCH_MAX, count - lo)
            part = (_lib.DiRankItem * m).from_buffer(items, lo * ctypes.sizeof(_lib.DiRankItem))
            nb = self.lib.di_contact_rank_batch_work_bytes(part, m)
            if nb < 0:
                raise ValueError(f"contact ranking of a batch of {m}: code {nb}")
            work, part_dev = _grow(self, nb), _table_to_device(part, dev)
            _lib.check(self.lib.di_contact_rank_batch(dt, part, _ptr(part_dev), m, ctypes.c_float(threshold),
                                                      _ptr(work), _stream()), "di_contact_rank_batch")
        return res


def _grow(op, nbytes):
    """The op's workspace, grown to nbytes (shared by its single and batched calls: stream order)."""
    if op._work is None or op._work.numel() * 8 < nbytes:
        op._work = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=op.device)
    return op._work


def _table_to_device(items, device):
    """A ctypes array of descriptors as a device tensor: staged in a fresh pinned buffer (the host
    allocator keeps it until the copy has run) and copied without blocking on the current stream."""
    nbytes = ctypes.sizeof(items)
    pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    ctypes.memmove(pinned.data_ptr(), ctypes.addressof(items), nbytes)
    return pinned.to(device, non_blocking=True)


class ContactAuc:
    """Result of one ``ContactAucOp`` call. ``num_pos, num_neg, num_nan, pos_distinct, u2, auroc,
    auprc, overflow`` are host numbers, read from the device on first use with one copy (which waits
    for the stream the op ran on). u2 = sum over (positive, negative) pairs of 2 [p_pos > p_neg] +
    [p_pos == p_neg]; auroc = u2 / (2 num_pos num_neg); both figures are float('nan') when a class is
    empty or a score is NaN (then u2 = pos_distinct = 0). ``rerun(num_pos)``, if given, runs the op
    again with room for every positive: used once, on that first read, if this run overflowed. The
    results of one ``batch`` call share one copy of their records (``table``, ``index``: the batch's
    metrics table and this complex's row); one that overflowed is rerun alone."""

    _FIELDS = tuple(f for f, _ in _lib.DiAucMetrics._fields_ if f != "pad")

    def __init__(self, metrics_dev, max_pos, rerun=None, table=None, index=0):
        self._metrics_dev, self._metrics, self.max_pos, self._rerun = metrics_dev, None, max_pos, rerun
        self._table, self._index = table, index

    def _read(self) -> dict:
        raw = self._metrics_dev.cpu().numpy().tobytes() if self._table is None else self._table.row(self._index)
        m = _lib.DiAucMetrics.from_buffer_copy(raw)
        return {f: getattr(m, f) for f in self._FIELDS}

    def metrics(self) -> dict:
        if self._metrics is None:
            m = self._read()
            if m["overflow"] and self._rerun is not None:
                again = self._rerun(m["num_pos"])
                self._metrics_dev, self.max_pos, self._table = again._metrics_dev, again.max_pos, None
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
        return _grow(self, nb)

    def _run(self, probs, labels, max_pos, out=None):
        """One complex through di_contact_auc; out (optional): the int64 [8] record to write."""
        n = probs.numel()
        work = self._workspace(n, max_pos)
        words = ctypes.sizeof(_lib.DiAucMetrics) // 8
        if out is None:
            out = torch.empty(words, dtype=torch.int64, device=self.device)
        else:
            _check_out("auc", out, torch.int64, words, 8, self.device)
        _lib.check(self.lib.di_contact_auc(_ptr(probs), _ptr(labels), n, max_pos, _ptr(out), _ptr(work), _stream()),
                   "di_contact_auc")
        return ContactAuc(out, max_pos)

    def __call__(self, probs, labels, max_pos=None):
        max_pos = self.check_args(probs, labels, max_pos)
        check_on(self.device, "ContactAucOp", probs, labels)
        res = self._run(probs, labels, max_pos)
        res._rerun = lambda num_pos: self._run(probs, labels, num_pos)   # keeps probs and labels alive
        return res

    def batch(self, probs_list, labels_list, max_pos=None, out=None):
        """The op over many complexes of different shapes with ONE launch sequence per DI_BATCH_MAX
        complexes (``di_contact_auc_batch``): a list of ``ContactAuc``, each with the bits the single
        call gives on the same inputs. max_pos: None (the default per complex), one int, or one per
        complex. The argument checks are the single op's, applied to every element. The descriptor
        table goes to the device with one pinned, non-blocking copy on the current stream; the results
        share one metrics table, read from the device once, on first use; a complex that overflowed
        its max_pos is rerun alone through the single op on that read, and leaves its neighbours'
        figures as they are.

        out (optional): per complex the int64 [8], 8-B aligned tensor (or a ``RecordSlot``, whose
        ``auc`` is one) that receives its di_auc_metrics instead of a row of the op's table: the items'
        out pointers name them, with the bits of the call without ``out``. Another dtype, length,
        device, layout or alignment raises ValueError before any launch. Each result then reads its
        own record; a rerun after an overflow still writes a buffer of the op's (the caller that must
        have the rerun's figures in its memory calls ``_run(..., out=...)``, as
        ``distributed.ranked_forward`` does)."""
        count = len(probs_list)
        if count < 1:
            raise ValueError("contact AUC: an empty batch")
        if out is not None and len(out) != count:
            raise ValueError("contact AUC: one out record per complex")
        mps = list(max_pos) if isinstance(max_pos, (list, tuple)) else [max_pos] * count
        if len(labels_list) != count or len(mps) != count:
            raise ValueError("contact AUC: one labels tensor and one max_pos per complex")
        for i in range(count):
            mps[i] = self.check_args(probs_list[i], labels_list[i], mps[i])
            check_on(self.device, "ContactAucOp", probs_list[i], labels_list[i])
            if self.lib.di_contact_auc_work_bytes(probs_list[i].numel(), mps[i]) < 0:
                self._workspace(probs_list[i].numel(), mps[i])    # raises as the single op does
        words = ctypes.sizeof(_lib.DiAucMetrics) // 8
        if out is None:
            metrics = torch.empty(count, words, dtype=torch.int64, device=self.device)
            table = _MetricsTable(metrics)
        else:
            metrics = [_check_out("auc", getattr(o, "auc", o), torch.int64, words, 8, self.device) for o in out]
            table = None
        items = (_lib.DiAucItem * count)()
        results = []
        for i, (probs, labels) in enumerate(zip(probs_list, labels_list)):
            it = items[i]
            it.probs, it.labels, it.out = probs.data_ptr(), labels.data_ptr(), metrics[i].data_ptr()
            it.n, it.max_pos = probs.numel(), mps[i]
            res = ContactAuc(metrics[i], mps[i], None, table, i)
            res._rerun = lambda num_pos, p=probs, y=labels: self._run(p, y, num_pos)   # keeps both alive
            results.append(res)
        for lo in range(0, count, _lib.DI_BATCH_MAX):
            m = min(_lib.DI_BATCH_MAX, count - lo)
            part = (_lib.DiAucItem * m).from_buffer(items, lo * ctypes.sizeof(_lib.DiAucItem))
            nb = self.lib.di_contact_auc_batch_work_bytes(part, m)
            if nb < 0:
                raise ValueError(f"contact AUC of a batch of {m}: code {nb}")
            work, part_dev = _grow(self, nb), _table_to_device(part, self.device)
            _lib.check(self.lib.di_contact_auc_batch(part, _ptr(part_dev), m, _ptr(work), _stream()),
                       "di_contact_auc_batch")
        return results


_EX_OUTSIDE = "examples: a pair index outside the complex"
_EX_LABEL = "examples: labels must be 0 or 1"
_EX_TWICE = "examples: a pair is missing or listed twice"


class ExamplesOp:
    """The reference's ``examples`` lists ([n, 3] rows of (i, j, label)) of a ragged batch on HIP
    (csrc/contact_examples.hip): ``labels`` turns complete lists into the uint8 label maps the ranking
    and AUC ops take, ``gather`` turns sampled lists into ``LitGINI.validation_step``'s pooled logits
    and labels. One memset and one launch per DI_BATCH_MAX complexes, one host read (the flag words)
    per call. No CPU fallback. Lists of int64 or int32 are read as they are when the whole batch has
    one of the two widths; any other dtype, a mixed batch or a non-contiguous list is converted to
    contiguous int64 first (a float list is truncated, as ``Tensor.to(torch.int64)`` does)."""

    def __init__(self, device="cuda"):
        self.device = gpu_device(device)
        self.lib = _lib.load()

    def _lists(self, examples_list):
        """(index-width code, the lists as the kernels read them)."""
        check_on(self.device, "ExamplesOp", *examples_list)
        for ex in examples_list:
            if ex.dim() != 2 or ex.shape[1] != 3:
                raise ValueError("examples: [n, 3] rows of (i, j, label)")
        if all(ex.dtype == torch.int32 for ex in examples_list):
            return _lib.DI_I32, [ex.contiguous() for ex in examples_list]
        return _lib.DI_I64, [ex.to(torch.int64).contiguous() for ex in examples_list]

    @staticmethod
    def _raise(flags, twice=True):
        """The first complex with a flag raises; within it outside, then labels, then twice."""
        for f in flags:
            if f & _lib.DI_EX_OUTSIDE:
                raise ValueError(_EX_OUTSIDE)
            if f & _lib.DI_EX_LABEL:
                raise ValueError(_EX_LABEL)
            if twice and f & _lib.DI_EX_TWICE:
                raise ValueError(_EX_TWICE)

    def labels(self, examples_list, shapes):
        """Complete lists (every pair of the complex exactly once) -> one uint8 [l1 * l2] map per
        complex, views of one packed buffer that each start 16-B aligned. shapes[i] = (l1, l2).
        Raises ``labels_from_examples_batch_torch``'s ValueErrors: a list of another shape or row
        count; then, for the first complex that has a fault, an index outside it, a label other
        than 0 / 1, a pair missing or listed twice, in this order."""
        count = len(examples_list)
        if count != len(shapes):
            raise ValueError("examples: one (l1, l2) per complex")
        if count < 1:
            raise ValueError("examples: an empty batch")
        idt, lists = self._lists(examples_list)
        off, at = [], 0
        for ex, (l1, l2) in zip(lists, shapes):
            n = int(l1) * int(l2)
            if n < 1:
                raise ValueError(f"examples: an empty complex ({l1} x {l2})")
            if ex.shape[0] != n:
                raise ValueError(f"examples: {ex.shape[0]} rows for {l1} x {l2} = {n} pairs "
                                 "(every pair exactly once)")
            off.append(at)
            at += (n + 15) // 16 * 16
        maps = torch.empty(at, dtype=torch.uint8, device=self.device)
        outs = [maps[o:o + int(l1) * int(l2)] for o, (l1, l2) in zip(off, shapes)]
        items = (_lib.DiExamplesItem * count)()
        for it, ex, out, (l1, l2) in zip(items, lists, outs, shapes):
            it.examples, it.labels, it.n, it.l1, it.l2 = ex.data_ptr(), out.data_ptr(), ex.shape[0], l1, l2
        flags = []
        for lo in range(0, count, _lib.DI_BATCH_MAX):
            m = min(_lib.DI_BATCH_MAX, count - lo)
            part = (_lib.DiExamplesItem * m).from_buffer(items, lo * ctypes.sizeof(_lib.DiExamplesItem))
            nb = self.lib.di_examples_labels_work_bytes(part, m)
            if nb < 0:
                raise ValueError(f"examples of a batch of {m}: code {nb} (l1 * l2 < 2^29)")
            # its own workspace per launch: the flag words at its front are read after the last one
            work = torch.empty(nb // 4, dtype=torch.int32, device=self.device)
            part_dev = _table_to_device(part, self.device)
            _lib.check(self.lib.di_examples_labels_batch(idt, part, _ptr(part_dev), m, _ptr(work), _stream()),
                       "di_examples_labels_batch")
            flags.append(work[:m])
        self._raise((flags[0] if len(flags) == 1 else torch.cat(flags)).cpu().tolist())
        return outs

    def gather(self, logits_list, examples_list, pools=None):
        """Sampled lists (any row count >= 1, any order, repeats allowed) -> per pool
        ``(logits [1, 2, N, 1], labels [N] uint8)``: logits[0, c, r, 0] = the complex's
        logits[0, c, i_r, j_r], bit for bit in the logits' dtype, and labels[r] = label_r, the rows of
        the pool's complexes one after another (the reference's ``torch.cat``,
        deepinteract_modules.py:1923-1932). Both go straight into ``ContactRankOp`` /
        ``ContactAucOp``, which take the pooled list as an N x 1 map. logits_list: contiguous
        [1, 2, L1, L2] tensors of one dtype (fp32 or bf16). pools: the complexes (indices into the
        lists) that form each pool, every complex in exactly one; default: one pool per complex.
        Raises ValueError for an index outside a complex or a label other than 0 / 1 (the first
        complex with a fault, in this order)."""
        count = len(logits_list)
        if count < 1 or len(examples_list) != count:
            raise ValueError("examples: one non-empty list of logits and one examples tensor per complex")
        pools = [[i] for i in range(count)] if pools is None else [list(p) for p in pools]
        if sorted(i for p in pools for i in p) != list(range(count)) or any(not p for p in pools):
            raise ValueError("examples: every complex belongs to exactly one non-empty pool")
        check_on(self.device, "ExamplesOp", *logits_list)
        idt, lists = self._lists(examples_list)
        dtype = logits_list[0].dtype
        if dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"examples: fp32 / bf16 logits, got {dtype}")
        for lg, ex in zip(logits_list, lists):
            if lg.dim() != 4 or lg.shape[0] != 1 or lg.shape[1] != 2 or not lg.is_contiguous() or lg.numel() < 1:
                raise ValueError("examples: one contiguous [1, 2, L1, L2] logits tensor per complex")
            if lg.dtype != dtype:
                raise TypeError("examples: one batch takes logits of one dtype")
            if ex.shape[0] < 1:
                raise ValueError("examples: a sampled list holds at least one row")
        totals = [sum(lists[i].shape[0] for i in p) for p in pools]
        lg_off, lab_off, at_lg, at_lab = [], [], 0, 0
        for total in totals:      # every pool starts 16-B aligned in both buffers
            lg_off.append(at_lg)
            lab_off.append(at_lab)
            at_lg += (2 * total + 7) // 8 * 8
            at_lab += (total + 15) // 16 * 16
        pool_logits = torch.empty(at_lg, dtype=dtype, device=self.device)
        pool_labels = torch.empty(at_lab, dtype=torch.uint8, device=self.device)
        out = [(pool_logits[a:a + 2 * t].view(1, 2, t, 1), pool_labels[b:b + t])
               for a, b, t in zip(lg_off, lab_off, totals)]
        items = (_lib.DiExamplesItem * count)()
        for (plg, plab), members, total in zip(out, pools, totals):
            at = 0
            for i in members:
                it, lg, ex = items[i], logits_list[i], lists[i]
                it.examples, it.logits, it.pool_logits, it.pool_labels = (t.data_ptr() for t in (ex, lg, plg, plab))
                it.n, it.out_off, it.total, it.l1, it.l2 = ex.shape[0], at, total, lg.shape[2], lg.shape[3]
                at += ex.shape[0]
        flags = torch.empty(count, dtype=torch.int32, device=self.device)
        dt = _lib.DI_F32 if dtype == torch.float32 else _lib.DI_BF16
        for lo in range(0, count, _lib.DI_BATCH_MAX):
            m = min(_lib.DI_BATCH_MAX, count - lo)
            part = (_lib.DiExamplesItem * m).from_buffer(items, lo * ctypes.sizeof(_lib.DiExamplesItem))
            rc = self.lib.di_examples_gather_batch_check(dt, idt, part, ctypes.c_void_p(16), m, _ptr(flags[lo:]))
            if rc < 0:
                raise ValueError(f"examples of a batch of {m}: code {rc} (l1 * l2 < 2^29, a pool's rows < 2^31)")
            part_dev = _table_to_device(part, self.device)
            _lib.check(self.lib.di_examples_gather_batch(dt, idt, part, _ptr(part_dev), m, _ptr(flags[lo:]),
                                                         _stream()), "di_examples_gather_batch")
        self._raise(flags.cpu().tolist(), twice=False)
        return out


def interface_atoms(xyz, residue_index, element=None):
    """One chain's atoms as ``InterfaceOp`` takes them: ``(xyz float32 [A, 3], res_off int32 [L + 1])``,
    the heavy atoms grouped by residue with CSR offsets. Host, numpy. xyz: [N, 3] coordinates;
    residue_index: one entry per atom ([N] of any dtype, or [N, m] rows such as (number, insertion
    code)) -- atoms of one residue follow each other, and residues are numbered in order of first
    appearance; element (optional): one symbol per atom, atoms whose symbol is 'H' (any case, spaces
    ignored) are dropped. ValueError for arrays of other shapes, a chain left without atoms, or a
    residue index that reappears after another one."""
    import numpy as np
    xyz = np.asarray(xyz)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError("interface atoms: xyz is [N, 3]")
    res = np.asarray(residue_index)
    if res.ndim == 1:
        res = res[:, None]
    if res.ndim != 2 or res.shape[0] != xyz.shape[0]:
        raise ValueError("interface atoms: one residue index per atom")
    if element is not None:
        el = np.char.upper(np.char.strip(np.asarray(element, dtype=str)))
        if el.shape != (xyz.shape[0],):
            raise ValueError("interface atoms: one element symbol per atom")
        xyz, res = xyz[el != "H"], res[el != "H"]
    if xyz.shape[0] < 1:
        raise ValueError("interface atoms: the chain has no heavy atoms")
    starts = np.concatenate(([0], np.flatnonzero((res[1:] != res[:-1]).any(axis=1)) + 1))
    if len(np.unique(res[starts], axis=0)) != len(starts):
        raise ValueError("interface atoms: a residue index reappears after another residue "
                         "(the atoms of one residue follow each other)")
    res_off = np.concatenate((starts, [xyz.shape[0]])).astype(np.int32)
    return np.ascontiguousarray(xyz, dtype=np.float32), res_off


_IF_OFFSETS = "interface: residue offsets do not start at 0, decrease, or do not end at the atom count"
_IF_EMPTY = "interface: a residue without atoms"
_IF_NONFINITE = "interface: a NaN or Inf coordinate"


class InterfaceOp:
    """The label maps of bound complexes from their chains' heavy-atom coordinates on HIP
    (csrc/contact_interface.hip, ``di_interface_labels_batch``): residue i of chain 0 and residue j of
    chain 1 interact iff some atom of i lies within ``cutoff`` (<=) of some atom of j -- the definition
    behind DIPS' pos_idx (deepinteract_utils.py:612: non-hydrogen atoms, 6 A), from which the reference's
    ``build_examples_tensor`` makes its example lists. One memset and two launches per DI_BATCH_MAX
    complexes, one host read (the stats) per call. No CPU fallback."""

    def __init__(self, device="cuda"):
        self.device = gpu_device(device)
        self.lib = _lib.load()
        self.num_pos = []

    def labels(self, chains0, chains1, cutoff=6.0):
        """chains0[i] / chains1[i]: complex i's ``(xyz [A, 3], res_off [L + 1])`` per chain
        (``interface_atoms``), numpy arrays or tensors on the op's GPU -> one uint8 [l1 * l2] map per
        complex, views of one packed buffer that each start 16-B aligned, as ``ExamplesOp.labels``
        returns them. The pair test is fp32 and fixed to the bit: d2 = (dx * dx + dy * dy) + dz * dz
        <= (float)(cutoff * cutoff). All host arrays of a call go to the device in ONE pinned packed
        copy on the current stream; device tensors are read where they are (converted to contiguous
        fp32 / int32 if they are not). ``num_pos`` keeps the call's positives per complex (ints).
        Raises ValueError for arrays of other shapes or a cutoff that is not finite and positive, before
        any launch; then, for the first complex that has a fault, malformed offsets, a residue without
        atoms, a NaN or Inf coordinate, in this order."""
        import math

        import numpy as np
        count = len(chains0)
        if count < 1 or len(chains1) != count:
            raise ValueError("interface: one non-empty list of chains per side, of one length")
        cutoff = float(cutoff)
        as_f32 = ctypes.c_float(cutoff).value       # what the kernels get
        if not math.isfinite(as_f32) or as_f32 <= 0:
            raise ValueError(f"interface: cutoff = {cutoff}: finite and positive")
        host, words = [], 0       # (array, word offset in the packed copy)
        chains = []               # per complex and side: [xyz, res_off], a tensor or an index into host

        def take(a, dtype, tdtype):
            nonlocal words
            if isinstance(a, torch.Tensor):
                check_on(self.device, "InterfaceOp", a)
                return a.to(tdtype).contiguous()
            a = np.ascontiguousarray(a, dtype=dtype)
            host.append((a, words))
            words += a.size
            return len(host) - 1

        shapes = []
        for pair in zip(chains0, chains1):
            sizes = []
            for xyz, off in pair:
                if len(xyz.shape) != 2 or xyz.shape[1] != 3 or len(off.shape) != 1:
                    raise ValueError("interface: a chain is (xyz [A, 3], res_off [L + 1])")
                a, l = int(xyz.shape[0]), int(off.shape[0]) - 1
                if a < 1 or l < 1:
                    raise ValueError("interface: a chain has at least one residue and one atom")
                chains.append([take(xyz, np.float32, torch.float32), take(off, np.int32, torch.int32)])
                sizes.append((l, a))
            shapes.append(sizes)
        if host:
            pinned = torch.empty(words, dtype=torch.int32, pin_memory=True)
            flat = pinned.numpy()
            for a, at in host:
                flat[at:at + a.size] = a.reshape(-1).view(np.int32)
            packed = pinned.to(self.device, non_blocking=True)
            for c in chains:
                for s, tdtype in ((0, torch.float32), (1, torch.int32)):
                    if not isinstance(c[s], torch.Tensor):
                        a, at = host[c[s]]
                        c[s] = packed[at:at + a.size].view(tdtype)
        off_map, at = [], 0
        for (l1, _), (l2, _) in shapes:
            off_map.append(at)
            at += (l1 * l2 + 15) // 16 * 16
        maps = torch.empty(at, dtype=torch.uint8, device=self.device)
        outs = [maps[o:o + s[0][0] * s[1][0]] for o, s in zip(off_map, shapes)]
        items = (_lib.DiInterfaceItem * count)()
        for i, (it, out, ((l1, a0), (l2, a1))) in enumerate(zip(items, outs, shapes)):
            (x0, o0), (x1, o1) = chains[2 * i], chains[2 * i + 1]
            it.xyz0, it.res_off0, it.xyz1, it.res_off1 = (t.data_ptr() for t in (x0, o0, x1, o1))
            it.labels, it.l1, it.l2, it.a0, it.a1 = out.data_ptr(), l1, l2, a0, a1
        stats = []
        for lo in range(0, count, _lib.DI_BATCH_MAX):
            m = min(_lib.DI_BATCH_MAX, count - lo)
            part = (_lib.DiInterfaceItem * m).from_buffer(items, lo * ctypes.sizeof(_lib.DiInterfaceItem))
            nb = self.lib.di_interface_work_bytes(part, m)
            if nb < 0:
                raise ValueError(f"interface of a batch of {m}: code {nb} (l1 * l2 < 2^29, a chain's atoms < 2^24)")
            # its own workspace per launch: the stats at its front are read after the last one
            work = torch.empty(nb // 8, dtype=torch.int64, device=self.device)
            part_dev = _table_to_device(part, self.device)
            _lib.check(self.lib.di_interface_labels_batch(part, _ptr(part_dev), m, ctypes.c_float(cutoff), _ptr(work),
                                                          _stream()), "di_interface_labels_batch")
            stats.append(work[:2 * m])
        rows =(stats[0] if len(stats) == 1 else torch.cat(stats)).cpu().view(count, 2).tolist()
        for _, word in rows:
            f = word & 0xffffffff
            for bit, text in ((_lib.DI_IF_OFFSETS, _IF_OFFSETS), (_lib.DI_IF_EMPTY, _IF_EMPTY),
                              (_lib.DI_IF_NONFINITE, _IF_NONFINITE)):
                if f & bit:
                    raise ValueError(text)
        self.num_pos = [int(n) for n, _ in rows]
        return outs


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
    return labels_from_examples_batch([examples], [(l1, l2)])[0]


_examples_ops = {}   # device -> ExamplesOp, for labels_from_examples_batch


def labels_from_examples_batch(examples_list, shapes):
    """``labels_from_examples`` for many complexes: shapes[i] = (l1, l2) of examples_list[i]. The same
    validation and the same result per complex, with ONE host read for the whole batch. Lists that
    all lie on one GPU go through ``ExamplesOp.labels`` (one memset and one launch per DI_BATCH_MAX
    complexes); anything else -- host tensors, an empty batch, an empty complex -- takes
    ``labels_from_examples_batch_torch``. Results and errors are the same either way."""
    devices = {ex.device for ex in examples_list}
    if len(devices) == 1 and len(examples_list) == len(shapes) and all(a * b > 0 for a, b in shapes):
        dev = next(iter(devices))
        if dev.type == "cuda":
            if dev not in _examples_ops:
                _examples_ops[dev] = ExamplesOp(dev)
            return _examples_ops[dev].labels(examples_list, shapes)
    return labels_from_examples_batch_torch(examples_list, shapes)


def labels_from_examples_batch_torch(examples_list, shapes):
    """``labels_from_examples_batch`` in torch operations, on whatever device the lists are on: the
    path of host tensors, and the yardstick ``ExamplesOp.labels`` is tested and measured against."""
    if len(examples_list) != len(shapes):
        raise ValueError("examples: one (l1, l2) per complex")
    flags, outs = [], []
    for examples, (l1, l2) in zip(examples_list, shapes):
        if examples.dim() != 2 or examples.shape[1] != 3:
            raise ValueError("examples: [n, 3] rows of (i, j, label)")
        n = l1 * l2
        if examples.shape[0] != n:
            raise ValueError(f"examples: {examples.shape[0]} rows for {l1} x {l2} = {n} pairs "
                             "(every pair exactly once)")
        ex = examples.to(torch.int64)
        i, j, lab = ex[:, 0], ex[:, 1], ex[:, 2]
        outside = (i < 0) | (i >= l1) | (j < 0) | (j >= l2)
        flat = torch.where(outside, torch.zeros_like(i), i * l2 + j)    # a bad row scatters nowhere new
        seen = torch.zeros(n, dtype=torch.int32, device=examples.device)
        seen.index_add_(0, flat, torch.ones(n, dtype=torch.int32, device=examples.device))
        flags.append(torch.stack((outside.any(), ((lab != 0) & (lab != 1)).any(), (seen != 1).any())))
        out = torch.zeros(n, dtype=torch.uint8, device=examples.device)
        out[flat] = lab.to(torch.uint8)
        outs.append(out)
    if flags:
        devices = {f.device for f in flags}
        host = (torch.stack(flags) if len(devices) == 1 else torch.stack([f.cpu() for f in flags])).cpu()
        for bad in host.tolist():
            if bad[0]:
                raise ValueError("examples: a pair index outside the complex")
            if bad[1]:
                raise ValueError("examples: labels must be 0 or 1")
            if bad[2]:
                raise ValueError("examples: a pair is missing or listed twice")
    return outs


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


def pooled_topk_metrics(hits, num_pos, l: int, n: int) -> dict:
    """The six top-k figures of LitGINI.validation_step (``top_10_prec`` .. ``top_l_by_5_recall``; the
    step logs them as ``val_`` + name) for a pooled list of ``n`` sampled rows, from ``hits`` (hits[r] =
    positives among ranks 0..r of the pool, as many ranks as were kept) with the reference's
    arithmetic (deepinteract_utils.py:977-995) and its k's: 10, l // 10, l // 5 (precision), l,
    l // 2, l // 5 (recall), l = graph1.num_nodes() + graph2.num_nodes(). Unlike test_step's maps a
    pool may be shorter than k: the reference's slice ``[:k]`` then takes all n rows (num_pos
    positives), and precision still divides by k.

    A figure is float('nan') where the reference would divide by zero (k = 0; num_pos = 0 for a
    recall), where k and n both exceed DI_RANK_MAX_K (the ranking is cut there), and where fewer than
    min(k, n) ranks were kept."""
    K, num_pos, n = len(hits), int(num_pos), int(n)

    def top(k):
        if k < 1 or (k > _lib.DI_RANK_MAX_K and n > _lib.DI_RANK_MAX_K):
            return None
        if k >= n:
            return num_pos
        return None if k > K else int(hits[k - 1])

    def prec(k):
        h = top(k)
        return float("nan") if h is None else h / k

    def recall(k):
        h = top(k)
        return float("nan") if h is None or num_pos == 0 else h / num_pos

    return {"top_10_prec": prec(10), "top_l_by_10_prec": prec(l // 10), "top_l_by_5_prec": prec(l // 5),
            "top_l_recall": recall(l), "top_l_by_2_recall": recall(l // 2), "top_l_by_5_recall": recall(l // 5)}


__all__ = ["ContactRankOp", "ContactRanking", "ContactRankingBatch", "ContactAucOp", "ContactAuc",
           "ExamplesOp", "InterfaceOp", "interface_atoms", "GatheredRanking", "RecordSlot", "record_k", "confusion_metrics", "labels_from_examples", "labels_from_examples_batch",
           "labels_from_examples_batch_torch", "pooled_topk_metrics", "topk_metrics"]
