"""pipeline.OverlappedSchedule in the modes tests/test_gpu_c3.py and tests/test_gpu_rccl_schedule.py do
not run, at chain lengths of 24 .. 136 residues (a job is a few hundred kB; cases, the pair checker and
the self-checking schedule in tests/schedule_cases.py, their premises in
tests/test_schedule_cases_host.py):

  a. every engine path as the schedule's producer: each signal carrier (di_embed_init_edge_z,
     di_embed_init_edge, di_node_embed) as the first launch of a forward that carries signal=, each hT
     writer (di_node_update, di_node_layer, di_node_update_folded) into the ring, bf16 and fp32,
     reference-featurised and general batches, on the ragged layout;
  b. fp32 on a layout aligned to 4 elements but not to 8, which a bf16 schedule refuses;
  c. "ordered" mode (one stream given twice): no pair stream, a help launch behind every forward;
  d. queue rollovers (capacity_steps = 2 over 5 steps), verified at the rollover's own drain;
  e. jobs_per_launch 1 and 2 with 3 micro-batches (the last launch covers one job);
  f. as many sinks as ring slots (sinks reused), and fewer (refused unless discard_outputs);
  g. no patience across a rollover with allow_gave_up: the help launches complete every job;
  h. the rollover's check and the constructor's allow_gave_up, with the queue's gave-up / error words
     set from the host.

Every test first runs each micro-batch alone through the engine (with the path's settings), then the
schedule. Per job: every pair tensor bit-equal to the outer concat of the node features the schedule
itself computed (its tap), the tap bit-equal to the standalone forward, and each chain of the tap within
geot_cases.TOL of its own float64 oracle run (fp32 1e-4, bf16 1.5e-2). Counters: error == 0, signalled ==
jobs, stream_bytes + help_bytes == the exact byte count, and gave_up == 0 wherever the mode is
overlapped -- a carrier that dropped its signal would still produce exact outputs (the help launches
complete every job) and only that counter would show it. Measured errors are printed with -s
(DESIGN.md section 2).
"""
import pytest
import torch

import geot_cases as C
import schedule_cases as S

pytestmark = pytest.mark.gpu

# (dtype, path) -> engine attributes that differ from the defaults
PATHS = {
    ("bf16", "default"): {},
    ("bf16", "f_form"): {"z_init": False},
    ("bf16", "unfused_staged"): {"fuse_embed_init": False, "resident_init": False},
    ("bf16", "fused_node"): {"split_node": False},
    ("bf16", "fold"): {"fold_attn": True},
    ("f32", "default"): {},
    ("f32", "unfused"): {"fuse_embed_init": False},
    ("f32", "fused_node"): {"split_node": False},
}
DEFAULTS = {"z_init": True, "fuse_embed_init": True, "resident_init": True, "split_node": True, "fold_attn": False}
MATRIX = [("bf16", "default", "knn"), ("bf16", "f_form", "knn"), ("bf16", "unfused_staged", "knn"),
          ("bf16", "fused_node", "knn"), ("bf16", "fold", "knn"), ("bf16", "default", "general"),
          ("f32", "default", "knn"), ("f32", "unfused", "knn"), ("f32", "fused_node", "knn"),
          ("f32", "default", "general")]
N_MAX, E_MAX = 432, 432 * S.K  # ragged8 built with k = 20, the largest batch here


@pytest.fixture(scope="module")
def batches():
    out = {}
    for layout, feats in S.FAMILIES:
        out[layout, feats] = mbs = [S.device_batch(layout, feats, mb) for mb in range(S.N_MB)]
        for gb in mbs:
            assert gb.geo_ref == (feats == "knn")
            assert gb.nodes_per_graph == S.chain_sizes(layout) and gb.num_nodes == S.descriptors(layout)[4]
            assert gb.num_nodes <= N_MAX and gb.num_edges <= E_MAX
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def engines():
    from deepinteract_amd.config import GeoTConfig
    from deepinteract_amd.engine import GeoTEngine
    made = {}

    def get(dtype):
        if dtype not in made:
            eng = GeoTEngine(C.state_dict(S.L), dtype, GeoTConfig(num_gnn_layers=S.L))
            assert {a: getattr(eng, a) for a in DEFAULTS} == DEFAULTS  # DI_INIT_Z=0 would hide the z path
            eng.workspace(N_MAX, E_MAX)  # one slot for every batch: never replaced while a schedule runs
            made[dtype] = eng
        return made[dtype]

    return get


class _Path:
    """Engine attributes of a path for the length of a with block."""

    def __init__(self, eng, path):
        self.eng, self.attrs = eng, PATHS[eng.dtype, path]

    def __enter__(self):
        for a, v in self.attrs.items():
            setattr(self.eng, a, v)
        return self.eng

    def __exit__(self, *exc):
        for a, v in DEFAULTS.items():
            setattr(self.eng, a, v)


class _Run:
    """One schedule over the micro-batches of a family: standalone forwards first (the warm-up and the
    bit-exact reference of every tap), then a schedule_cases.Checked with NaN-filled sinks."""

    def __init__(self, eng, batches, layout, feats="knn", *, n_sinks, ordered=False, ring=4, help_every=2,
                 patience_ms=200.0, events=None, **kw):
        from deepinteract_amd.pipeline import schedule_streams
        self.eng, self.layout, self.feats, self.mbs = eng, layout, feats, batches[layout, feats]
        self.h1r, self.h2r, self.l1, self.l2, _ = S.descriptors(layout)
        self.dt = S.TORCH_DT[eng.dtype]
        self.outs = [eng.forward(gb, events=events) for gb in self.mbs]
        torch.cuda.synchronize()
        self.sinks = [torch.full((S.numel(layout),), float("nan"), dtype=self.dt, device="cuda") for _ in range(n_sinks)]
        self.taps = {}
        if ordered:
            kw["s_geot"] = kw["s_pair"] = schedule_streams(eng.device)[0]
        # the launch geometry (stream_blocks / stream_waves / help_blocks / help_waves) stays the library's
        self.sch = S.Checked(eng, self.mbs, self.h1r, self.h2r, self.l1, self.l2, self.sinks, ring=ring,
                             help_every=help_every, patience_ms=patience_ms, tap=self._tap,
                             on_epoch_end=self._epoch_end, **kw)
        assert self.sch.mode == ("ordered" if ordered else "overlapped") and self.sch.concurrent == (not ordered)
        self.verified = []

    def _tap(self, j, h, e):
        self.taps[self.sch.epoch, j] = (h.clone(), e.clone())

    def _epoch_end(self, sch, epoch, jobs):
        # inside the rollover, behind its own drain: every job of the epoch that still owns its sink
        self.verify(range(max(0, jobs - len(self.sinks)), jobs), epoch)

    def steps(self, n):
        for _ in range(n):
            self.sch.step()
        return self

    def verify(self, jobs, epoch=None):
        """Pair tensors of `jobs` (of the current or a given epoch) against their taps, the taps against
        the standalone forwards."""
        epoch = self.sch.epoch if epoch is None else epoch
        for j in jobs:
            h, e = self.taps[epoch, j]
            S.check_pairs(self.sch.views(j), h, self.h1r, self.h2r, self.l1, self.l2, job=(epoch, j))
            ho, eo = self.outs[j % len(self.mbs)]
            assert torch.equal(h, ho) and torch.equal(e, eo), ("tap differs from the standalone forward", epoch, j)
            self.verified.append((epoch, j))

    def oracle(self, label):
        """Each chain of the last tap of every micro-batch against its own float64 oracle run."""
        worst = [0.0, 0.0]
        tol, failures = C.TOL[self.eng.dtype], []
        for m, gb in enumerate(self.mbs):
            key = max(k for k in self.taps if k[1] % len(self.mbs) == m)
            h, e = (t.float().cpu().numpy() for t in self.taps[key])
            for g in range(len(gb.nodes_per_graph)):
                rn, re = C.oracle64(C.state_dict(S.L), C.oracle_item(gb, g), S.L, key=("sched", self.layout, self.feats, m, g))
                n0, n1, e0, e1 = gb.node_off[g], gb.node_off[g + 1], gb.edge_off[g], gb.edge_off[g + 1]
                (en, rown), (ee, rowe) = C.check(h[n0:n1], rn), C.check(e[e0:e1], re)
                worst = [max(worst[0], en), max(worst[1], ee)]
                if not (en <= tol and ee <= tol):
                    failures.append(f"job {key} chain {g}: node {en:.3e} (row {rown}), edge {ee:.3e} (row {rowe})")
        print(f"schedule_small {label} {self.layout} {self.feats}: worst node {worst[0]:.3e} edge {worst[1]:.3e}")
        assert not failures, (tol, failures)

    def close(self, n_jobs, **kw):
        """Drain, then the counters every run must show; returns their sum over the epochs."""
        cnt = self.sch.close(**kw)
        print(f"counters {cnt} help launches {self.sch.help_launches} epochs {self.sch.epoch_jobs}")
        assert cnt["error"] == 0 and cnt["signalled"] == n_jobs == sum(self.sch.epoch_jobs), cnt
        assert cnt["stream_bytes"] + cnt["help_bytes"] == self.exact_bytes(n_jobs), (cnt, self.exact_bytes(n_jobs))
        return cnt

    def exact_bytes(self, n_jobs):
        return n_jobs * S.numel(self.layout) * torch.tensor([], dtype=self.dt).element_size()


def _overlapped_run(eng, batches, layout, feats, label, steps=2, **kw):
    """Test a's run and checks: `steps` steps, one sink per job, ring 4, a help launch every 2 jobs."""
    n_jobs = steps * S.N_MB
    run = _Run(eng, batches, layout, feats, n_sinks=n_jobs, **kw).steps(steps)
    cnt = run.close(n_jobs)
    assert cnt["gave_up"] == 0, cnt
    assert run.sch.epoch == 0
    run.verify(range(n_jobs))
    run.oracle(label)
    return run, cnt


# ---- a. path matrix --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path,feats", MATRIX, ids=[f"{d}-{p}-{f}" for d, p, f in MATRIX])
def test_path_matrix(engines, batches, dtype, path, feats):
    from deepinteract_amd.engine import uses_z_init
    with _Path(engines(dtype), path) as eng:
        # what the path table means, stated apart from the engine's own dispatch
        want_z = dtype == "bf16" and path in ("default", "fused_node") and feats == "knn"
        want_embed_launch = path.startswith("unfused") or feats == "general"
        want_split = path not in ("fused_node", "fold")
        assert all(uses_z_init(eng, gb) == want_z for gb in batches["ragged8", feats])
        before, events = eng.z_forwards, {}
        run, cnt = _overlapped_run(eng, batches, "ragged8", feats, f"{dtype} {path}", events=events)
        # 3 standalone forwards and 6 jobs: the z0 path on all of them or on none
        assert eng.z_forwards - before == int(want_z) * 3 * S.N_MB
        # the launches of the standalone forwards (the same dispatch): which kernel carries a signal
        # (node_embed when the embedding is a launch of its own, else the InitEdge launch) and which
        # writes hT (the split node update behind node_aggr, else the fused / folded node layer)
        assert ("node_embed" in events) == want_embed_launch, sorted(events)
        assert ("node_aggr" in events) == want_split, sorted(events)
        _carrier_signals(eng, batches["ragged8", feats][0])
    assert {a: getattr(eng, a) for a in DEFAULTS} == DEFAULTS


def _carrier_signals(eng, gb):
    """The path's signal carrier on its own, without timing. At these sizes gave_up == 0 cannot show a
    carrier that drops its signal_job: the signalled word is a running maximum, so the next help launch
    (which carries the pending signal itself) would release the waiting stream waves within a few
    forwards, far inside any patience. So: one forward with signal= on a zeroed queue must leave
    exactly job + 1 in the signalled word and touch no other word; a lower job never lowers it."""
    from deepinteract_amd.pipeline import PairQueue
    q = PairQueue(eng.device, 8)
    eng.forward(gb, clone=False)
    torch.cuda.synchronize()
    assert not bool(q.state.any())
    eng.forward(gb, clone=False, signal=(q.state, 4))
    torch.cuda.synchronize()
    assert q.counters()["signalled"] == 5 and int(q.state.count_nonzero()) == 1, q.counters()
    eng.forward(gb, clone=False, signal=(q.state, 2))
    torch.cuda.synchronize()
    assert q.counters()["signalled"] == 5 and int(q.state.count_nonzero()) == 1, q.counters()


# ---- b. a layout aligned to 4 elements only --------------------------------------------------------------
def test_ragged4_f32(engines, batches):
    _overlapped_run(engines("f32"), batches, "ragged4", "knn", "f32 default")


def test_ragged4_bf16_is_refused(engines, batches):
    from deepinteract_amd.pipeline import OverlappedSchedule
    h1r, h2r, l1, l2, _ = S.descriptors("ragged4")
    sinks = [torch.empty(S.numel("ragged4"), dtype=torch.bfloat16, device="cuda") for _ in range(S.N_MB)]
    with pytest.raises(ValueError, match="16-B aligned planes"):
        OverlappedSchedule(engines("bf16"), batches["ragged4", "knn"], h1r, h2r, l1, l2, sinks, ring=4, help_every=2)


# ---- c. ordered mode -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_ordered_mode(engines, batches, dtype):
    n_jobs = 2 * S.N_MB
    run = _Run(engines(dtype), batches, "ragged8", n_sinks=n_jobs, ordered=True).steps(2)
    assert run.sch.mode == "ordered" and not run.sch.concurrent
    cnt = run.close(n_jobs)
    assert cnt["stream_bytes"] == 0 and cnt["gave_up"] == 0 and cnt["help_bytes"] == run.exact_bytes(n_jobs), cnt
    assert run.sch.help_launches == n_jobs and cnt["signalled"] == n_jobs
    run.verify(range(n_jobs))
    run.oracle(f"{dtype} ordered")


# ---- d. rollover ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,ordered", [("bf16", False), ("f32", False), ("bf16", True)],
                         ids=["bf16-overlapped", "f32-overlapped", "bf16-ordered"])
def test_rollover(engines, batches, dtype, ordered):
    """5 steps of 3 jobs with room for 2 steps: two rollovers. Every epoch's 6 jobs are verified inside
    _rollover (Checked: behind the rollover's own drain, never a finish() of the test's), where the queue's
    state must be zero again; the help cadence (every 2 jobs, 3 jobs a step) falls differently in each step."""
    run = _Run(engines(dtype), batches, "ragged8", n_sinks=6, ordered=ordered, capacity_steps=2)
    assert run.sch.queue.capacity == 6
    run.steps(5)
    assert run.sch.epoch == 2 and run.verified == [(ep, j) for ep in (0, 1) for j in range(6)]
    cnt = run.close(15)
    assert run.sch.epoch_jobs == [6, 6, 3]
    run.verify(range(3))
    assert len(run.verified) == 15
    if ordered:
        assert cnt["stream_bytes"] == 0 and run.sch.help_launches == 15, cnt
    assert cnt["gave_up"] == 0, cnt
    run.oracle(f"{dtype} rollover {'ordered' if ordered else 'overlapped'}")


# ---- e. jobs_per_launch -----------------------------------------------------------------------------------
@pytest.mark.parametrize("jpl", [1, 2])
def test_jobs_per_launch(engines, batches, jpl):
    run, _ = _overlapped_run(engines("bf16"), batches, "ragged8", "knn", f"bf16 jobs_per_launch={jpl}", jobs_per_launch=jpl)
    assert run.sch.jobs_per_launch == jpl


# ---- f. sinks ---------------------------------------------------------------------------------------------
def test_as_many_sinks_as_ring_slots(engines, batches):
    run = _Run(engines("bf16"), batches, "ragged8", n_sinks=4).steps(2)
    assert len(run.sinks) == run.sch.ring == 4
    cnt = run.close(6)
    assert cnt["gave_up"] == 0, cnt
    run.verify(range(2, 6))  # jobs 4 and 5 reused the sinks of jobs 0 and 1


def test_fewer_sinks_than_ring_slots(engines, batches):
    run = _Run(engines("bf16"), batches, "ragged8", n_sinks=2)
    with pytest.raises(ValueError, match="2 sinks for up to 4 jobs in flight"):
        run.sch.step()
    assert run.sch.next_job == 0 and not run.taps  # refused before anything was issued
    # a benchmark that never reads them: the outputs race by design and are not compared
    run = _Run(engines("bf16"), batches, "ragged8", n_sinks=2, discard_outputs=True).steps(2)
    cnt = run.close(6)
    assert cnt["gave_up"] == 0, cnt


# ---- g. no patience ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_no_patience_across_a_rollover(engines, batches, dtype):
    """Stream waves that find their job unsignalled give up at once; the help launches (before a ring
    slot is reused, at the rollover's drain and at the end) complete every job all the same."""
    run = _Run(engines(dtype), batches, "ragged8", n_sinks=6, capacity_steps=2, patience_ms=1e-6, allow_gave_up=True)
    run.steps(3)
    assert run.sch.epoch == 1 and run.verified == [(0, j) for j in range(6)]
    cnt = run.close(9)  # close() checks with the constructor's allow_gave_up
    assert cnt["help_bytes"] > 0, cnt
    run.verify(range(3))


# ---- h. the rollover's check ----------------------------------------------------------------------------
def _one_epoch(engines, batches, **kw):
    """A schedule with room for one step, after one step and a drain that showed clean counters."""
    run = _Run(engines("bf16"), batches, "ragged8", n_sinks=4, capacity_steps=1, **kw).steps(1)
    run.sch.finish()
    torch.cuda.synchronize()
    cnt = run.sch.check()
    assert cnt["gave_up"] == 0 and cnt["error"] == 0 and cnt["signalled"] == S.N_MB, cnt
    return run


def test_rollover_raises_on_gave_up_by_default(engines, batches):
    from deepinteract_amd import _lib
    run = _one_epoch(engines, batches)
    assert run.sch.allow_gave_up is False
    S.set_word(run.sch, _lib.PQ_GAVE_UP, 1)
    with pytest.raises(RuntimeError, match="gave up waiting"):
        run.sch.step()
    assert run.sch.epoch == 0 and run.sch.next_job == S.N_MB  # nothing was reset or issued


def test_rollover_goes_on_with_allow_gave_up(engines, batches):
    from deepinteract_amd import _lib
    run = _one_epoch(engines, batches, allow_gave_up=True)
    S.set_word(run.sch, _lib.PQ_GAVE_UP, 1)
    run.sch.step()  # rolls over: Checked verifies epoch 0's sinks and that the queue's state is zero again
    assert run.sch.epoch == 1 and run.verified == [(0, j) for j in range(S.N_MB)]
    run.sch.finish()
    torch.cuda.synchronize()
    cnt = run.sch.check(allow_gave_up=False)  # the word was reset: the new epoch is clean by the strict check
    assert cnt["gave_up"] == 0 and cnt["signalled"] == S.N_MB, cnt
    total = run.close(2 * S.N_MB)
    assert total["gave_up"] == 1, total  # the epoch's count as the rollover read it
    run.verify(range(S.N_MB))


def test_rollover_raises_on_the_error_word_in_every_case(engines, batches):
    from deepinteract_amd import _lib
    run = _one_epoch(engines, batches, allow_gave_up=True)
    S.set_word(run.sch, _lib.PQ_ERROR, 1)
    with pytest.raises(RuntimeError, match="pair queue error"):
        run.sch.step()
    with pytest.raises(RuntimeError, match="pair queue error"):
        run.sch.check(allow_gave_up=True)
