"""Shared cases for the overlapped schedule at small ragged shapes (tests/test_schedule_cases_host.py
on the CPU, tests/test_gpu_schedule_small.py on the GPU). No tests here.

* Layouts (``LAYOUTS``): the per-complex (l1, l2) list every micro-batch of a schedule shares.
    ragged8  [(24, 136), (72, 40), (136, 24)]  every length a multiple of 8 (bf16 and fp32); max(l1) = 136
             is three 64-row blocks, the last of 8 rows, and the two shorter complexes leave empty items
    ragged4  [(28, 36), (68, 44)]              every length a multiple of 4 and none of 8: fp32 only (a
             16-byte vector is 4 fp32 or 8 bf16 elements)
  ``descriptors`` gives the rows and lengths the schedule is constructed with, ``aligned`` restates the
  constructor's alignment rule (node rows, every h2 row, every l2).
* Micro-batches: ``N_MB`` distinct ones per layout. "knn": synth.synthetic_chain chains of the layout's
  lengths (seed ``chain_seed``), k = 20, one fixed neighbour seed per chain position; built on the device
  (``device_batch``; reference-featurised, so gb.geo_ref holds) or on the CPU (``knn_host_item``).
  "general": hand-made chains of the ragged8 lengths (``general_item``: in-degrees 0 .. 12 behind a fixed
  head, src uniform over the chain, random direction and normalised quaternion columns, as
  geot_cases.ragged_item's "general" form), so gb.geo_ref is False and the live-gather kernels run.
* ``pair_reference`` / ``pair_views``: the flat sink of one job (construct_interact_tensor of every
  complex at the schedule's offsets) built with torch indexing, and its per-complex views.
* ``check_pairs``: every pair tensor bit-equal (compared as integers, so a NaN, a sign of zero or one
  mantissa bit counts) to the outer concat of h, both halves; the error names the first bad
  (job, complex, half).
* ``Checked``: an OverlappedSchedule that verifies an epoch at the rollover's own drain.
"""
import torch

from deepinteract_amd.pipeline import OverlappedSchedule
from oracle import geot_oracle as O

LAYOUTS = {"ragged8": [(24, 136), (72, 40), (136, 24)], "ragged4": [(28, 36), (68, 44)]}
DTYPES = {"ragged8": ("bf16", "f32"), "ragged4": ("f32",)}
VEC = {"bf16": 8, "f32": 4}  # elements of a 16-byte vector
TORCH_DT = {"bf16": torch.bfloat16, "f32": torch.float32}
K, N_MB, H, L = 20, 3, 128, 2
# (layout, featurisation) of every batch family the GPU file runs
FAMILIES = (("ragged8", "knn"), ("ragged4", "knn"), ("ragged8", "general"))
# in-degrees of the first nodes of every hand-made chain (an empty destination, one edge, one past a
# 16-edge segment, one past a 32-edge wave); the rest uniform in 0 .. GENERAL_MAX_DEG
GENERAL_HEAD, GENERAL_MAX_DEG = (0, 1, 17, 40), 12

_items = {}


def chain_sizes(layout):
    return [n for pair in LAYOUTS[layout] for n in pair]


def descriptors(layout):
    """(h1r, h2r, l1, l2, n_rows) of a layout: chain 1 then chain 2 of each complex, concatenated."""
    off, h1r, h2r = 0, [], []
    for a, b in LAYOUTS[layout]:
        h1r.append(off)
        h2r.append(off + a)
        off += a + b
    return h1r, h2r, [a for a, _ in LAYOUTS[layout]], [b for _, b in LAYOUTS[layout]], off


def aligned(layout, vec):
    """OverlappedSchedule's rule: node rows, every h2 row and every l2 a multiple of `vec` elements."""
    _, h2r, _, l2, n_rows = descriptors(layout)
    return n_rows % vec == 0 and all(r % vec == 0 for r in h2r) and all(b % vec == 0 for b in l2)


def numel(layout):
    return sum(2 * H * a * b for a, b in LAYOUTS[layout])


def chain_seed(layout, mb, g):
    return 9000 + 1000 * list(LAYOUTS).index(layout) + 100 * mb + g


def nbr_seeds(layout):
    return list(range(1, len(chain_sizes(layout)) + 1))


def knn_chains(layout, mb):
    from deepinteract_amd import synth
    return [synth.synthetic_chain(n, chain_seed(layout, mb, g)) for g, n in enumerate(chain_sizes(layout))]


def knn_host_item(layout, mb, g):
    """Chain g of a kNN micro-batch featurised on the CPU (oracle.build_graph, the same neighbour seed)."""
    key = (layout, "knn", mb, g)
    if key not in _items:
        from deepinteract_amd import synth
        chain = synth.synthetic_chain(chain_sizes(layout)[g], chain_seed(layout, mb, g))
        it = O.build_graph(chain, k=K, seed=nbr_seeds(layout)[g])
        _items[key] = {k: it[k] for k in ("num_nodes", "src", "dst", "src_nbr", "dst_nbr", "node_f", "edge_f")}
    return _items[key]


def general_item(layout, mb, g):
    """Hand-made chain g of a general-featurised micro-batch (cached; treat as read-only)."""
    key = (layout, "general", mb, g)
    if key not in _items:
        n = chain_sizes(layout)[g]
        gen = torch.Generator().manual_seed(chain_seed(layout, mb, g) + 50)
        deg = torch.randint(0, GENERAL_MAX_DEG + 1, (n,), generator=gen)
        deg[:len(GENERAL_HEAD)] = torch.tensor(GENERAL_HEAD)
        E = int(deg.sum())
        edge_f = torch.rand(E, 28, generator=gen)
        edge_f[:, 20:23] = torch.randn(E, 3, generator=gen)
        edge_f[:, 23:27] = torch.nn.functional.normalize(torch.randn(E, 4, generator=gen), dim=1)
        _items[key] = {"num_nodes": n, "src": torch.randint(0, n, (E,), generator=gen),
                       "dst": torch.repeat_interleave(torch.arange(n), deg),
                       "src_nbr": torch.randint(0, E, (E, 2), generator=gen),
                       "dst_nbr": torch.randint(0, E, (E, 2), generator=gen),
                       "node_f": torch.rand(n, 113, generator=gen), "edge_f": edge_f}
    return _items[key]


def host_item(layout, feats, mb, g):
    return knn_host_item(layout, mb, g) if feats == "knn" else general_item(layout, mb, g)


def device_batch(layout, feats, mb):
    """Micro-batch `mb` of a family as a GraphBatch on the GPU."""
    if feats == "knn":
        from deepinteract_amd.builder import build_graph_batch
        return build_graph_batch(knn_chains(layout, mb), k=K, nbr_seeds=nbr_seeds(layout))
    from deepinteract_amd.graph import GraphBatch
    return GraphBatch.from_arrays([general_item(layout, mb, g) for g in range(len(chain_sizes(layout)))], "cuda")


# ---- the pair tensors of one job --------------------------------------------------------------------
def pair_views(buf, l1, l2):
    """Per-complex [1, 2H, l1, l2] views of a flat sink (the schedule's offsets: complexes back to back)."""
    out, off = [], 0
    for a, b in zip(l1, l2):
        out.append(buf[off:off + 2 * H * a * b].view(1, 2 * H, a, b))
        off += 2 * H * a * b
    return out


def pair_reference(h, h1r, h2r, l1, l2):
    """Flat sink holding construct_interact_tensor (deepinteract_utils.py:158-172) of every complex of
    h [rows, H], by torch indexing."""
    parts = []
    for r1, r2, a, b in zip(h1r, h2r, l1, l2):
        t = torch.cat([h[r1:r1 + a].t().unsqueeze(2).expand(H, a, b), h[r2:r2 + b].t().unsqueeze(1).expand(H, a, b)])
        parts.append(t.reshape(-1))
    return torch.cat(parts)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def check_pairs(views, h, h1r, h2r, l1, l2, job=None):
    """Every view bit-equal to the outer concat of h's rows: channels [:H] chain 1's features along
    dim 2, channels [H:] chain 2's along dim 3. AssertionError names the first bad (job, complex, half)."""
    assert len(views) == len(l1) == len(l2) == len(h1r) == len(h2r), (len(views), len(l1))
    hb = _bits(h)
    for cx, (t, r1, r2, a, b) in enumerate(zip(views, h1r, h2r, l1, l2)):
        assert t.shape == (1, 2 * H, a, b) and t.dtype == h.dtype, (job, cx, tuple(t.shape), t.dtype)
        tb = _bits(t[0])
        want = (hb[r1:r1 + a].t().unsqueeze(2).expand(H, a, b), hb[r2:r2 + b].t().unsqueeze(1).expand(H, a, b))
        for half in (0, 1):
            bad = tb[half * H:(half + 1) * H] != want[half]
            if bool(bad.any()):
                c, i, j = bad.nonzero()[0].tolist()
                raise AssertionError(f"pair tensor differs from its node features: job {job}, complex {cx}, half {half} "
                                     f"({int(bad.sum())} elements; first at channel {half * H + c}, row {i}, column {j})")


# ---- a schedule that checks itself at the rollover ------------------------------------------------------
COUNTERS = ("signalled", "error", "gave_up", "stream_bytes", "help_bytes")


class Checked(OverlappedSchedule):
    """OverlappedSchedule whose rollover is observed: when job numbering wraps, the device has just been
    drained by _rollover itself (the harness never calls finish() before it), so every sink of the epoch
    must be complete there. on_epoch_end(schedule, epoch, jobs): called at that point, to verify the
    epoch's sinks against the epoch's taps. Afterwards the queue's state must be all zero, the sinks are
    refilled with NaN, and the epoch's counters (as check() read them, before the reset) are added to
    ``total``. ``epoch`` counts the wraps so far; close() adds the last, partial epoch's counters."""

    def __init__(self, *args, on_epoch_end=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.on_epoch_end = on_epoch_end
        self.epoch, self.epoch_jobs = 0, []
        self.total = dict.fromkeys(COUNTERS, 0)
        self.last_counters = None

    def check(self, *args, **kwargs):
        self.last_counters = None
        self.last_counters = c = super().check(*args, **kwargs)
        return c

    def _add(self, c):
        for k in COUNTERS:
            self.total[k] += c[k]

    def _rollover(self):
        before, self.last_counters = self.next_job, None
        super()._rollover()
        if not (before > 0 and self.next_job == 0):
            return
        assert self.last_counters is not None, "the rollover did not check the queue"
        self._add(self.last_counters)
        assert not bool(self.queue.state.any()), "queue state survives the rollover"
        assert (self.helped, self.pending) == (0, -1)
        if self.on_epoch_end is not None:
            self.on_epoch_end(self, self.epoch, before)
        for s in self.sinks:
            s.fill_(float("nan"))
        torch.cuda.synchronize(self.eng.device)
        self.epoch_jobs.append(before)
        self.epoch += 1

    def close(self, allow_gave_up=None):
        """finish(), drain, and the sum of every epoch's counters (the last epoch's included)."""
        self.finish()
        torch.cuda.synchronize(self.eng.device)
        kw = {} if allow_gave_up is None else {"allow_gave_up": allow_gave_up}
        self._add(self.check(**kw))
        self.epoch_jobs.append(self.next_job)
        return dict(self.total)


def set_word(sch, word, value):
    """Write one word of the queue's state (_lib.PQ_GAVE_UP, _lib.PQ_ERROR) from the host, on the GeoT
    stream (the NULL stream would wait for a pair-stream launch in flight), and drain."""
    with torch.cuda.stream(sch.s_geot):
        sch.queue.state[word] = int(value)
    torch.cuda.synchronize(sch.eng.device)
