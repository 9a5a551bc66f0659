"""Complex-sharded data parallelism over torch.distributed (RCCL on ROCm, gloo in CPU tests).

SURVEY.md §8e: complexes are independent (eval-mode BatchNorm, replicated weights), so the
forward shards by complex with no exchange; the only collective is ONE all-gather of the
contact maps after the head (the reference has no multi-GPU inference; its predict path is
single-node DP, lit_model_predict_docker.py:183, producing per-complex maps as
lit_model_predict.py:236-239 does).

* ``shard`` — contiguous shards: rank r owns complexes [b_r, b_{r+1}), the boundaries chosen so
  every rank's summed cost (L1*L2 pair work + (L1+L2)*k edge work) is as even as a contiguous
  split allows; every rank computes the same plan from the sizes alone.
* ``local_order`` — a rank's complexes in size-sorted order, so micro-batches group similar
  sizes (varlen work balanced inside each launch).
* ``all_gather_maps`` — packs each rank's [L1,L2] maps into one flat buffer (padded to the
  largest rank's element count) and issues a single ``all_gather_into_tensor``; on xGMI one big
  collective beats many small ones (7 point-to-point links per GPU). dtype and device are
  arguments every rank passes identically, so a rank that owns no complex still sends a
  buffer of the agreed type.
* ``predict_sharded`` — the C4 driver: shard -> micro-batched forward (graph build, GeoT,
  pair tensor / head prologue, head, contact probabilities) -> the maps on every rank, gathered
  either chunked (default, SURVEY.md §8e: round c gathers every rank's c-th micro-batch of maps
  with an asynchronous ``all_gather_into_tensor`` issued as soon as they exist, so the collective
  of round c runs on the process group's stream while round c+1 computes) or ONCE after the last
  micro-batch (``all_gather_maps``). Both return bit-identical maps.
* ``predict_sharded(gather="topk")`` -- a third wire format: per complex one fixed-layout record
  (``di_rank_record_bytes``: its K best contacts and, with labels, test_step's counters and AUC
  figures) instead of its L1 * L2 map; ``ranked_forward`` is its HIP forward, whose ranking and AUC
  kernels write the records straight into the send buffer, and ``RecordPlan`` their places in it.
  ONE all-gather moves them. ``test_sharded`` builds ``LitGINI.test_step``'s dict for every complex
  on every rank from them (the reference gathers per-step results the same way,
  deepinteract_modules.py:2114-2119).
"""
from __future__ import annotations

from typing import Callable, Sequence

import torch
import torch.distributed as dist


def complex_cost(l1: int, l2: int, k: int = 20) -> int:
    return l1 * l2 + k * (l1 + l2)


def shard(sizes: Sequence[tuple], world: int, k: int = 20):
    """sizes: (L1, L2) per complex -> per rank, the contiguous list of its complex indices.

    Boundary b_r is the first index whose cost prefix reaches r/world of the total, so each
    shard's cost is within one complex of the even share."""
    n = len(sizes)
    cost = [complex_cost(a, b, k) for a, b in sizes]
    total = float(sum(cost))
    bounds, acc, i = [0], 0.0, 0
    for r in range(1, world):
        target = total * r / world
        while i < n and acc + cost[i] / 2.0 <= target:
            acc += cost[i]
            i += 1
        bounds.append(i)
    bounds.append(n)
    return [list(range(bounds[r], bounds[r + 1])) for r in range(world)]


def local_order(sizes: Sequence[tuple], indices: Sequence[int]):
    """A rank's complexes, largest first (stable), for size-grouped micro-batches."""
    return sorted(indices, key=lambda i: (-(sizes[i][0] * sizes[i][1]), i))


def all_gather_maps(local_maps: Sequence[torch.Tensor], plan, sizes, dtype: torch.dtype,
                    device, group=None):
    """Gather every rank's contact maps; returns the maps of ALL complexes in global order.

    local_maps: this rank's maps in the order of plan[rank]; dtype / device: the wire format,
    identical on every rank (RCCL needs matching dtypes and sizes on all ranks)."""
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    if len(plan) != world:
        raise ValueError(f"plan has {len(plan)} shards for a world of {world}")
    counts = [sum(sizes[i][0] * sizes[i][1] for i in p) for p in plan]
    width = max(max(counts), 1)
    send = torch.zeros(width, dtype=dtype, device=device)
    if len(local_maps) != len(plan[rank]):
        raise ValueError(f"rank {rank}: {len(local_maps)} maps for {len(plan[rank])} planned complexes")
    if len(local_maps):
        flat = torch.cat([m.reshape(-1).to(device=device, dtype=dtype) for m in local_maps])
        if flat.numel() != counts[rank]:
            raise ValueError(f"rank {rank}: maps hold {flat.numel()} elements, plan says {counts[rank]}")
        send[:flat.numel()] = flat
    recv = torch.empty(world * width, dtype=dtype, device=device)
    dist.all_gather_into_tensor(recv, send, group=group)
    out = [None] * len(sizes)
    for r, p in enumerate(plan):
        off = r * width
        for i in p:
            l1, l2 = sizes[i]
            out[i] = recv[off:off + l1 * l2].view(l1, l2)
            off += l1 * l2
    return out


def gpu_forward(model, k: int = 20, seed: int = 0):
    """The per-micro-batch forward of ``predict_sharded`` on the HIP path: on-device graph build
    (deepinteract_amd.builder) -> LitGINI.predict_batch -> contact probabilities. Complex i's
    chains draw their neighbour-edge ids as torch.manual_seed(seed + 2i + s) would (s = 0, 1), so
    the maps do not depend on how the complexes are sharded or micro-batched. out (optional): one
    [L1, L2] tensor per complex -- the chunked gather's send slices -- that receive the maps (the
    softmax output written straight into the collective's buffer, in its wire dtype)."""
    from .builder import build_graph_batch

    def fn(complexes, ids, out=None):
        chains = [c for pair in complexes for c in pair]
        dev = model.engine.device
        gb = build_graph_batch(chains, k=k, device=dev, node_count_limit=model.cfg.node_count_limit,
                               nbr_seeds=[seed + 2 * i + s for i in ids for s in (0, 1)])
        with torch.no_grad():
            _, probs = model.predict_batch(gb, [(2 * j, 2 * j + 1) for j in range(len(complexes))])
            if out is not None:
                for dst, p in zip(out, probs):
                    dst.copy_(p)
                return out
        return probs

    return fn


def gather_rounds(sizes: Sequence[tuple], plan, micro_batch: int):
    """The chunked all-gather's schedule, computed by every rank from the sizes alone: round c holds
    micro-batch c of every rank (its size-sorted local order cut into micro_batch-sized pieces; a
    rank with fewer micro-batches contributes nothing to the later rounds). Returns per round
    (per-rank complex lists, the round's per-rank buffer width in elements)."""
    mbs = []
    for p in plan:
        order = local_order(sizes, p)
        mbs.append([order[s:s + micro_batch] for s in range(0, len(order), micro_batch)])
    rounds = []
    for c in range(max((len(m) for m in mbs), default=0)):
        members = [m[c] if c < len(m) else [] for m in mbs]
        width = max(max(sum(sizes[i][0] * sizes[i][1] for i in ids) for ids in members), 1)
        rounds.append((members, width))
    return rounds


class ChunkedGather:
    """Round-by-round asynchronous all-gather of contact maps (chunked and overlapped
    with compute). Every round's send and receive buffers are allocated up front (sizes are known
    from the plan), and ``slots(c)`` hands out this rank's [L1, L2] slices of round c's send buffer
    for the forward to write its maps into (gpu_forward's ``out``): the compute stream runs no pack,
    pad or cast kernels. ``put(c)`` issues ``all_gather_into_tensor(..., async_op=True)`` -- on
    RCCL it runs on the process group's own stream, which waits for the work already queued on the
    current stream (one event), so the next micro-batch's kernels, issued right after, overlap it;
    ``finish()`` waits for every round and returns the maps of all complexes in global order (views
    of the rounds' receive buffers)."""

    def __init__(self, sizes, plan, micro_batch, dtype, device, group=None):
        self.sizes, self.dtype, self.device, self.group = sizes, dtype, device, group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self.rounds = gather_rounds(sizes, plan, micro_batch)
        # padding of a round's send buffer is never read by a receiver; zeroed once for determinism
        self.send = [torch.zeros(width, dtype=dtype, device=device) for _, width in self.rounds]
        self.recv = [torch.empty(self.world * width, dtype=dtype, device=device) for _, width in self.rounds]
        self.pending = []

    def slots(self, c):
        """This rank's maps of round c as [L1, L2] views of the round's send buffer (member order)."""
        views, off = [], 0
        for i in self.rounds[c][0][self.rank]:
            l1, l2 = self.sizes[i]
            views.append(self.send[c][off:off + l1 * l2].view(l1, l2))
            off += l1 * l2
        return views

    def put(self, c, maps=None):
        """Issue round c's collective. maps (optional): this rank's maps of the round, copied into the
        send slices (for a forward that did not write them there itself)."""
        mine = self.rounds[c][0][self.rank]
        if maps is not None:
            if len(maps) != len(mine):
                raise ValueError(f"rank {self.rank}: {len(maps)} maps for round {c}'s {len(mine)} complexes")
            for dst, m in zip(self.slots(c), maps):
                if dst.data_ptr() != m.data_ptr():
                    dst.copy_(m)
        self._issue(c)

    def _issue(self, c):
        work = dist.all_gather_into_tensor(self.recv[c], self.send[c], group=self.group, async_op=True)
        self.pending.append((c, self.recv[c], self.send[c], work))

    def finish(self):
        # rounds in which this rank has no micro-batch still take part (every rank issues every round)
        done = {c for c, *_ in self.pending}
        for c in range(len(self.rounds)):
            if c not in done:
                self._issue(c)
        out = [None] * len(self.sizes)
        for c, recv, _send, work in sorted(self.pending, key=lambda t: t[0]):
            work.wait()
            members, width = self.rounds[c]
            for r, ids in enumerate(members):
                off = r * width
                for i in ids:
                    l1, l2 = self.sizes[i]
                    out[i] = recv[off:off + l1 * l2].view(l1, l2)
                    off += l1 * l2
        self.pending = []
        return out


class RecordPlan:
    """Where every complex's wire record lies, computed by every rank from the sizes, the plan and k
    alone (no communication): rank r's records follow each other in its size-sorted local order (so
    a micro-batch's records are contiguous), each ``di_rank_record_bytes`` long, and every rank's
    part of the receive buffer is as wide as the largest rank's. ``ks[i]`` = ``ranking.record_k`` of
    complex i; a K beyond DI_RANK_MAX_K raises ValueError here, on every rank alike, before any
    collective. ``place[i]`` = (owner rank, byte offset in the owner's send buffer);
    ``rank_bytes[r]``; ``width`` = bytes of one rank's part (>= 16); ``send_bytes`` / ``recv_bytes``
    = what one rank sends and holds."""

    def __init__(self, sizes, plan, k=None, with_labels=False):
        from . import _lib
        from .ranking import record_k
        self.sizes, self.plan, self.with_labels = list(sizes), plan, bool(with_labels)
        self.ks = [record_k(l1, l2, k) for l1, l2 in self.sizes]
        self.place, self.rank_bytes = [None] * len(self.sizes), []
        for r, p in enumerate(plan):
            at = 0
            for i in local_order(self.sizes, p):
                self.place[i] = (r, at)
                at += _lib.rank_record_layout(*self.sizes[i], self.ks[i], self.with_labels)[0]
            self.rank_bytes.append(at)
        self.width = max(max(self.rank_bytes, default=0), 16)
        self.send_bytes, self.recv_bytes = self.width, len(plan) * self.width


def _predict_topk(complexes, forward, sizes, plan, micro_batch, device, group, k, with_labels):
    from .ranking import GatheredRanking, RecordSlot, _HostCopy
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    rp = RecordPlan(sizes, plan, k, with_labels)      # raises on every rank alike, before any collective
    # zero-filled once: padding, and the buffer of a rank that owns nothing, are deterministic
    send = torch.zeros(rp.width // 4, dtype=torch.int32, device=device)
    recv = torch.empty(world * rp.width // 4, dtype=torch.int32, device=device)
    mine = local_order(sizes, plan[rank])
    for s in range(0, len(mine), micro_batch):
        ids = mine[s:s + micro_batch]
        slots = [RecordSlot(send, rp.place[i][1], *sizes[i], rp.ks[i], with_labels) for i in ids]
        forward([complexes[i] for i in ids], ids, out=slots)
    if send.is_cuda and dist.get_backend(group) == "gloo":
        # gloo is a host transport: the finished buffer crosses to the host and back, still one collective
        host = torch.empty(recv.shape, dtype=recv.dtype)
        dist.all_gather_into_tensor(host, send.cpu(), group=group)
        recv.copy_(host)
    else:
        dist.all_gather_into_tensor(recv, send, group=group)
    table = _HostCopy(recv)
    return [GatheredRanking(recv, r * rp.width + off, *sizes[i], rp.ks[i], with_labels, table)
            for i, (r, off) in enumerate(rp.place)], plan


def predict_sharded(complexes: Sequence, forward: Callable, micro_batch: int = 8, dtype=torch.float32,
                    device=None, group=None, gather: str = "chunked", k=None, with_labels: bool = False):
    """C4 driver: every rank runs ``forward`` over its contiguous shard of
    ``complexes`` in size-sorted micro-batches; every complex's contact map ends on every rank.

    complexes: per complex a (chain1, chain2) pair of builder inputs (dicts with backbone
    [N,4,3], amide_norm [N,3], dips [N,106]); forward(batch, ids) -> list of [L1, L2] maps for
    the complexes ``batch`` (global indices ``ids``); a forward that takes ``out=`` (gpu_forward)
    writes them straight into the chunked gather's send slices.
    gather: "chunked" (default) -- one asynchronous all-gather per micro-batch round, overlapped
    with the next round's compute (ChunkedGather); "once" -- ONE all-gather after the last
    micro-batch (all_gather_maps); "none" -- no collective, this rank's maps only (timing the
    compute alone). Returns the maps (global order; None for other ranks' complexes with "none")
    and the plan.

    gather="topk": ranked contacts and metrics instead of maps. Sharding, micro-batches and plan are
    the same; what crosses the wire is one record per complex (``RecordPlan``; ``k``: ranks kept,
    None = min(L1, L2), an int = min(k, L1 * L2); ``with_labels``: the records also carry top_hits,
    di_rank_metrics and di_auc_metrics). One int32 send buffer for the whole call and the receive
    buffer are allocated up front on ``device``; the forward is called as ``forward(batch, ids,
    out=slots)`` with ``slots`` the complexes' ``ranking.RecordSlot`` views of the send buffer, which it
    must fill (``ranked_forward``); ``dtype`` is not used. After the last micro-batch exactly ONE
    ``all_gather_into_tensor`` is issued for the call, not one per round: a record is a few KB
    (12 KB at 1000 x 1000 with labels against a 4 MB map), so per-round collectives would be bound by
    their latency, not by bytes, and there is nothing worth overlapping. Returns one
    ``ranking.GatheredRanking`` per complex in global order, views of the receive buffer on ``device``,
    and the plan. A K beyond DI_RANK_MAX_K raises ValueError on every rank before any collective."""
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    sizes = [(int(len(c[0]["backbone"])), int(len(c[1]["backbone"]))) for c in complexes]
    plan = shard(sizes, world)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) == "nccl" \
            else torch.device("cpu")
    if gather not in ("chunked", "once", "none", "topk"):
        raise ValueError(f"gather {gather!r}: one of chunked, once, none, topk")
    if gather == "topk":
        return _predict_topk(complexes, forward, sizes, plan, micro_batch, torch.device(device), group, k,
                             with_labels)
    chunks = ChunkedGather(sizes, plan, micro_batch, dtype, device, group) if gather == "chunked" else None
    mine = local_order(sizes, plan[rank])
    maps = {}
    import inspect
    takes_out = "out" in inspect.signature(forward).parameters
    for c, s in enumerate(range(0, len(mine), micro_batch)):
        ids = mine[s:s + micro_batch]
        if chunks is not None and takes_out:
            got = list(forward([complexes[i] for i in ids], ids, out=chunks.slots(c)))
        else:
            got = list(forward([complexes[i] for i in ids], ids))
        for i, m in zip(ids, got):
            if tuple(m.shape) != sizes[i]:
                raise ValueError(f"complex {i}: map {tuple(m.shape)} != {sizes[i]}")
            maps[i] = m
        if chunks is not None:
            chunks.put(c, got)
    if gather == "chunked":
        return chunks.finish(), plan
    if gather == "none":
        return [maps.get(i) for i in range(len(sizes))], plan
    return all_gather_maps([maps[i] for i in plan[rank]], plan, sizes, dtype, device, group), plan


def ranked_forward(model, k: int = 20, seed: int = 0, examples=None, filepaths=None, auc_max_pos=None,
                   structures=None, cutoff: float = 6.0):
    """The per-micro-batch forward of ``predict_sharded(gather="topk")`` on the HIP path: on-device
    graph build with ``gpu_forward``'s seeding rule (complex i's chains draw their neighbour-edge ids
    from seed + 2i + s; ``k`` is the graphs' neighbour count) -> the model's batched forward ->
    ``ContactRankOp.batch(out=slots)``, whose kernels write each complex's ids and scores -- with
    ``examples`` also top_hits and di_rank_metrics -- into its record in the send buffer. The ranks
    kept are the slots' (``RecordPlan.ks``).

    examples (optional): every complex's [L1 * L2, 3] example list, indexed by global id (filepaths
    likewise; the forward itself does not read them). Then ``labels_from_examples_batch`` goes first and
    ``ContactAucOp.batch(out=slots)`` follows, on the maps the ranking stored. A complex with more
    positives than ``auc_max_pos`` (None: the op's default) must be finished by its owner before the
    collective: the micro-batch's records are read once (one copy of their span of the send buffer),
    and every complex whose record says overflow is run again through the single op with
    max_pos = num_pos, writing the same record, in stream order before the send.

    structures (instead of examples; both: ValueError): every complex's ((xyz0, res_off0), (xyz1,
    res_off1)) heavy atoms, indexed by global id, as ``LitGINI.test_batch_structures`` takes them. The
    label maps then come from ``ranking.InterfaceOp`` (``cutoff`` in A) and everything after them is
    the same; only the micro-batch's own atoms go to this rank's device. A chain whose residue count
    differs from its complex's raises ValueError before the micro-batch's first launch."""
    import ctypes

    from . import _lib
    from .builder import build_graph_batch
    from .ranking import labels_from_examples_batch

    if examples is not None and structures is not None:
        raise ValueError("ranked_forward: labels from examples or from structures, not both")
    given = examples if examples is not None else structures
    if given is not None and filepaths is not None and len(given) != len(filepaths):
        raise ValueError("ranked_forward: one file path per examples tensor / structure")

    def fn(complexes, ids, out):
        if len(out) != len(ids):
            raise ValueError("ranked_forward: one record slot per complex")
        if any(slot.with_labels != (given is not None) for slot in out):
            raise ValueError("ranked_forward: records carry labels exactly when examples or structures are given")
        if structures is not None:
            for i, (c1, c2) in zip(ids, complexes):
                want = (len(c1["backbone"]), len(c2["backbone"]))
                got = tuple(int(chain[1].shape[0]) - 1 for chain in structures[i])
                if got != want:
                    raise ValueError(f"ranked_forward: complex {i}'s structure has {got} residues, "
                                     f"its chains {want}")
        chains = [c for pair in complexes for c in pair]
        dev = model.engine.device
        gb = build_graph_batch(chains, k=k, device=dev, node_count_limit=model.cfg.node_count_limit,
                               nbr_seeds=[seed + 2 * i + s for i in ids for s in (0, 1)])
        with torch.no_grad():
            logits, _, _ = model._forward_batch(gb, [(2 * j, 2 * j + 1) for j in range(len(complexes))])
            logits = [lg.contiguous() for lg in logits]
            rank = model._ranker()
            ks = [slot.k for slot in out]
            if given is None:
                rank.batch(logits, k=ks, threshold=model.pos_prob_threshold, out=out)
                return out
            shapes = [(int(lg.shape[2]), int(lg.shape[3])) for lg in logits]
            if examples is not None:
                labels = labels_from_examples_batch([examples[i].to(rank.device) for i in ids], shapes)
            else:
                labels = model._interface().labels([structures[i][0] for i in ids], [structures[i][1] for i in ids],
                                                   cutoff=cutoff)
            ranks = rank.batch(logits, k=ks, labels_list=labels, threshold=model.pos_prob_threshold, out=out)
            auc_op = model._auc()
            max_pos = None if auc_max_pos is None else [min(int(auc_max_pos), a * b) for a, b in shapes]
            auc_op.batch([r.probs for r in ranks], labels, max_pos=max_pos, out=out)
            # the owner finishes overflowed complexes: one read of the micro-batch's span of records
            buf = out[0].buffer
            lo = min(slot.byte_off for slot in out)
            hi = max(slot.byte_off + slot.nbytes for slot in out)
            host = buf[lo // 4:hi // 4].cpu().numpy().tobytes()
            for slot, r, lab in zip(out, ranks, labels):
                at = slot.byte_off - lo + slot.offsets["auc"]
                m = _lib.DiAucMetrics.from_buffer_copy(host[at:at + ctypes.sizeof(_lib.DiAucMetrics)])
                if m.overflow:
                    auc_op._run(r.probs, lab, int(m.num_pos), out=slot.auc)
        return out

    return fn


def test_sharded(model, complexes, examples_list, filepaths, micro_batch: int = 8, k: int = 20, seed: int = 0,
                 group=None, device=None, auc_max_pos=None, structures=None, cutoff: float = 6.0):
    """``LitGINI.test_step`` over a sharded test set: ``predict_sharded(gather="topk",
    with_labels=True)`` with ``ranked_forward`` (``k``: the graphs' neighbour count, ``seed`` its
    seeding), then one dict per complex, in global order, on EVERY rank, decoded from the gathered
    records with one host copy. The keys are ``LitGINI.test_batch``'s, from the same host arithmetic
    (``topk_metrics`` over the record's top_hits with l = min(L1, L2), ``confusion_metrics``,
    loss = ce_sum / (L1 * L2), the record's auroc / auprc), so every figure has the bits of a
    single-process ``test_batch``. ``test_preds`` / ``test_preds_rounded`` / ``test_labels`` are
    None: maps are not sent. ``top_ids`` / ``top_scores`` (numpy, the min(L1, L2) best contacts) are
    added. The list goes to ``model.test_epoch_end(outs)`` WITHOUT a group: every rank already holds
    every row. device: where the buffers live (default: the model's GPU).

    The labels come from ``examples_list`` or, with ``examples_list=None``, from ``structures``
    (``ranked_forward``; ``cutoff`` in A): exactly one of the two is not None (ValueError otherwise)."""
    import os

    from .ranking import confusion_metrics, topk_metrics
    if (examples_list is None) == (structures is None):
        raise ValueError("test_sharded: exactly one of examples_list and structures")
    if not (len(complexes) == len(examples_list if structures is None else structures) == len(filepaths)):
        raise ValueError("test_sharded: one examples tensor (or structure) and one file path per complex")
    if device is None:
        device = model.engine.device
    forward = ranked_forward(model, k=k, seed=seed, examples=examples_list, filepaths=filepaths,
                             auc_max_pos=auc_max_pos, structures=structures, cutoff=cutoff)
    recs, _ = predict_sharded(complexes, forward, micro_batch=micro_batch, device=device, group=group,
                              gather="topk", k=None, with_labels=True)
    outs = []
    for rec, path in zip(recs, filepaths):
        l = min(rec.l1, rec.l2)
        confusion = {f: getattr(rec, f) for f in ("tp", "fp", "fn", "tn")}
        out = {"loss": rec.ce_sum / (rec.l1 * rec.l2)}
        out.update(topk_metrics(rec.host_array("hits"), rec.num_pos, l))
        out["test_preds"] = out["test_preds_rounded"] = out["test_labels"] = None
        out["target"] = str(path).split(os.sep)[-1][:4]
        out["confusion"] = confusion
        out["test_auroc"], out["test_auprc"] = rec.auroc, rec.auprc
        out.update(confusion_metrics(**confusion))
        out["top_ids"], out["top_scores"] = rec.host_array("ids"), rec.host_array("scores")
        outs.append(out)
    return outs


test_sharded.__test__ = False    # a driver, not a pytest case
