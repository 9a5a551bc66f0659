"""The fused head prologue (csrc/head_prologue.hip) elementwise against float64 at its tiling edges, with
the two-stage oracle of tests/prologue_cases.py (premises: tests/test_prologue_cases_host.py).

di_head_prologue is called through ctypes, so the test owns the workspace and the descriptors' out_off:
Stage A reads a', b', e^a', e^b' and the flag words back from the workspace (prefilled with a NaN, a guard
region behind di_head_prologue_work_bytes); Stage B compares the WHOLE output buffer as integers against
values computed from the device's own tables: 4096 guard elements before the first and after the last
complex, gaps between the complexes (a multiple of the vector for the row kernel, odd for the flat
kernel), a NaN guard word no ELU output holds. A failure names (complex, channel, row, column) or "guard".
Every test prints the figures it measured (python -m pytest -s) before it asserts.
"""
import types

import numpy as np
import pytest
import torch

import prologue_cases as P

pytestmark = pytest.mark.gpu

TORCH_DT = {"bf16": torch.bfloat16, "f32": torch.float32}
INT_DT = {"bf16": torch.int16, "f32": torch.int32}
DI_ERANGE = -2      # include/deepinteract_amd.h


def _params(cases):
    return [pytest.param(c.name, dt, id=f"{c.name}-{dt}") for c in cases for dt in c.dtypes]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _guarded(n, dtype):
    return torch.full((n,), P.GUARD[dtype], dtype=INT_DT[dtype], device="cuda").view(TORCH_DT[dtype])


def _fresh_work(words):
    """`words` fp32 words of workspace and WORK_GUARD behind them, all holding the NaN WORK_FILL."""
    return torch.full((words + P.WORK_GUARD,), P.WORK_FILL, dtype=torch.int32, device="cuda").view(torch.float32)


def _bits(t):
    it = torch.int16 if t.element_size() == 2 else torch.int32
    return t.contiguous().view(it).cpu().numpy().view(np.uint16 if t.element_size() == 2 else np.uint32)


def _desc_table(descs):
    from deepinteract_amd import _lib
    arr = (_lib.DiPairDesc * len(descs))(*[_lib.DiPairDesc(*d) for d in descs])
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()


def _call(prob, h, work, base, aligned=None):
    """di_head_prologue on the problem's descriptors; returns its code (synchronised)."""
    from deepinteract_amd import _lib
    from deepinteract_amd.engine import _ptr, _stream
    lib = _lib.load()
    assert lib.di_head_prologue_work_bytes(len(prob.sizes), prob.m1, prob.m2, prob.C) == 4 * prob.work_words
    assert work.numel() == prob.work_words + P.WORK_GUARD and h.data_ptr() % 16 == 0
    d = _desc_table(prob.descs)
    par = [_dev(v) for v in (prob.w, prob.b, prob.gamma, prob.beta)]
    dt = _lib.DI_BF16 if prob.dtype == "bf16" else _lib.DI_F32
    rc = lib.di_head_prologue(dt, _ptr(d), len(prob.sizes), prob.m1, prob.m2, prob.H, prob.C,
                              prob.aligned if aligned is None else aligned, _ptr(h), *[_ptr(p) for p in par],
                              prob.eps, _ptr(work), _ptr(base), _stream())
    torch.cuda.synchronize()
    return rc


def _run(prob, work=None):
    """One call on a fresh guarded output (and, unless given, a fresh NaN workspace). Returns (out bits
    from the layout's base, workspace words); the words before the base and behind the workspace are
    checked here."""
    h = _dev(prob.h).to(TORCH_DT[prob.dtype])
    assert torch.equal(h.float().cpu(), torch.from_numpy(prob.h))
    alloc = _guarded(prob.out_shift + prob.total, prob.dtype)
    base = alloc[prob.out_shift:]
    if prob.aligned:
        assert base.data_ptr() % 16 == 0
    else:
        assert prob.out_shift == 0 or base.data_ptr() % 16 == prob.out_shift * P.ESZ[prob.dtype]
    work = _fresh_work(prob.work_words) if work is None else work
    assert _call(prob, h, work, base) == 0
    got, w = _bits(alloc), work.cpu().numpy()
    assert (got[:prob.out_shift] == P.GUARD[prob.dtype]).all(), "guard: wrote before the buffer"
    assert (w[prob.work_words:].view(np.uint32) == P.WORK_FILL).all(), "guard: wrote behind the workspace"
    return got[prob.out_shift:], w


def _check(prob, got, w, what):
    tabs, flags = P.read_work(w, prob)
    a = P.check_tables(prob, tabs, flags)
    b = P.check_stream(prob, tabs, flags, got)
    print(f"\n{what}: Stage A {a.figures}, Stage B {b.figures}")
    assert a.ok, f"{what}, Stage A (k_prologue_tables): {a}"
    assert b.ok, f"{what}, Stage B (k_prologue_{prob.kernel}): {b}"
    return a, b


def _case(name, dtype):
    prob = P.problem(name, dtype)
    got, w = _run(prob)
    _check(prob, got, w, f"{name} {dtype}")
    return prob, got, w


@pytest.mark.parametrize("name,dtype", _params(P.STREAM_CASES))
def test_stream_cases(name, dtype):
    """k_prologue_rows at 1, 2, 63 .. 65, 127 .. 129, 193 and 257 chunks per row and 1, 63 .. 65,
    255 .. 257 and 513 rows, ragged batches; "wrap": more work items than blocks."""
    _case(name, dtype)


@pytest.mark.parametrize("name,dtype", _params(P.CHANNEL_CASES))
def test_channel_cases(name, dtype):
    """k_prologue_tables' ragged last channel group (nc = 1, 2, 3) beside full groups, hidden 8 .. 256."""
    _case(name, dtype)


@pytest.mark.parametrize("name,dtype", _params(P.FLAT_CASES))
def test_flat_cases(name, dtype):
    """k_prologue_flat: odd L2, 1 x 1, one row of one vector, odd gaps, the base one element off the
    vector; "grid": a complex of more than 4096 * 256 elements."""
    _case(name, dtype)


@pytest.mark.parametrize("name,dtype", _params(P.STAT_CASES))
def test_stat_cases(name, dtype):
    """Chains of 1 .. 3, var ~ eps, a conv bias 1e4 x the spread, unequal chains in one batch."""
    _case(name, dtype)


@pytest.mark.parametrize("dtype", P.DTYPES)
def test_small_x(dtype):
    """Thousands of elements with 0 < |x| < 2^-12 on both sides of zero: the product path (bf16) stays
    within PROD_ABS of the float64 ELU and equals the host's med3 bit for bit."""
    prob, _, w = _case("smallx", dtype)
    _, flags = P.read_work(w, prob)
    assert flags[0, 0] == 0


def test_flag_cases_and_a_stale_workspace():
    """max|table| on 30, 59, 61, 80, 200 per channel (a'- and b'-dominated, mixed within a group of four).
    flagA on a NaN workspace, flagB (the opposite flag in every channel) on the workspace flagA left, flagA
    again on the workspace flagB left: the same bits as the first time, tables and flags included."""
    pa, pb = P.problem("flagA", "bf16"), P.problem("flagB", "bf16")
    work = _fresh_work(pa.work_words)
    got1, w1 = _run(pa, work)
    _check(pa, got1, w1, "flagA, fresh workspace")
    gotb, wb = _run(pb, work)
    _check(pb, gotb, wb, "flagB, flagA's workspace")
    got2, w2 = _run(pa, work)
    _check(pa, got2, w2, "flagA, flagB's workspace")
    fa, fb = P.read_work(w1, pa)[1], P.read_work(wb, pb)[1]
    assert np.array_equal(fa, np.array(pa.flag, dtype=np.int32)) and np.array_equal(fa, 1 - fb)
    assert np.array_equal(got1, got2), "a stale workspace changed the output"
    assert np.array_equal(w1.view(np.uint32), w2.view(np.uint32)), "a stale workspace changed the tables"


@pytest.mark.parametrize("name,dtype", [("s2", "bf16"), ("s2", "f32"), ("odd", "bf16"), ("odd", "f32"), ("c7-h64", "bf16")])
def test_two_runs_give_the_same_bits(name, dtype):
    prob = P.problem(name, dtype)
    got1, w1 = _run(prob)
    got2, w2 = _run(prob)
    assert np.array_equal(got1, got2) and np.array_equal(w1.view(np.uint32), w2.view(np.uint32))


# ---- through HeadPrologueOp ---------------------------------------------------------------------------------
def _op_run(prob, shift):
    """HeadPrologueOp on out = a guarded buffer's payload, `shift` elements further in. Returns the
    buffer's bits from the shifted base on (the problem's gap-free layout), the rest checked here."""
    from deepinteract_amd.engine import HeadPrologueOp
    op = HeadPrologueOp(_dev(prob.w).reshape(prob.C, 2 * prob.H, 1, 1), _dev(prob.b), _dev(prob.gamma), _dev(prob.beta),
                        prob.eps, "cuda")
    h = _dev(prob.h).to(TORCH_DT[prob.dtype])
    alloc = _guarded(shift + prob.total, prob.dtype)
    lo = shift + P.BAND
    out, views = op(h, prob.h1r, prob.h2r, [a for a, _ in prob.sizes], [b for _, b in prob.sizes],
                    out=alloc[lo:lo + prob.total - 2 * P.BAND])
    torch.cuda.synchronize()
    assert out.data_ptr() == alloc.data_ptr() + lo * P.ESZ[prob.dtype]
    assert [tuple(v.shape) for v in views] == [(1, prob.C, a, b) for a, b in prob.sizes]
    got = _bits(alloc)
    assert (got[:shift] == P.GUARD[prob.dtype]).all(), "guard: wrote before the buffer"
    return got[shift:]


@pytest.mark.parametrize("name,dtype", [("s1", "bf16"), ("s1", "f32"), ("c7-h64", "bf16"), ("c7-h64", "f32"),
                                        ("flagA", "bf16"), ("smallx", "bf16"), ("eps", "f32")])
def test_through_the_op(name, dtype):
    """The op allocates its own workspace, so the bar is per element against float64: bar_a'[c] +
    bar_b'[c] plus Stage B's term (prologue_cases.check_composite). With `out` 4 bytes off the vector the
    flat kernel runs: the row kernel's bits in fp32 and on flagged bf16 channels; on unflagged bf16
    channels within the product path's allowance (PROD_ABS and the two bf16 roundings, 2^-8 relative
    each)."""
    prob = P.problem(name, dtype, 0)
    assert prob.kernel == "rows"
    rows = _op_run(prob, 0)
    rep = P.check_composite(prob, rows)
    print(f"\n{name} {dtype} through the op, row kernel: {rep.figures}")
    assert rep.ok, str(rep)
    flat = _op_run(prob, 4 // P.ESZ[dtype])
    rep = P.check_composite(prob, flat)
    print(f"{name} {dtype} through the op, 4 bytes off the vector: {rep.figures}")
    assert rep.ok, str(rep)
    for n, (_, _, off, l1, l2) in enumerate(prob.descs):
        r, f = (g[off:off + prob.C * l1 * l2].reshape(prob.C, l1 * l2) for g in (rows, flat))
        for c in range(prob.C):
            if dtype == "f32" or prob.flag[n][c]:
                assert np.array_equal(r[c], f[c]), f"complex {n}, channel {c}: the flat kernel's bits differ"
            else:
                rv, fv = P.bf16_val(r[c]).astype(np.float64), P.bf16_val(f[c]).astype(np.float64)
                tol = P.PROD_ABS + 2.0 ** -7 * np.maximum(np.abs(rv), np.abs(fv))
                bad = ~(np.abs(rv - fv) <= tol)
                assert not bad.any(), (f"complex {n}, channel {c}, row {int(np.flatnonzero(bad)[0]) // l2}, column "
                                       f"{int(np.flatnonzero(bad)[0]) % l2}: rows {rv[bad][0]!r}, flat {fv[bad][0]!r}")


# ---- 32-bit row offsets at their limit --------------------------------------------------------------------
def _tall_problem(dtype, size):
    case = P.Case(f"tall-{dtype}", 1, 8, [(size[0], ("el", size[1]))], seed=13)
    return P.Problem(case, dtype)


@pytest.mark.parametrize("dtype", P.DTYPES)
def test_tall_plane(dtype):
    """One plane just under 2^31 bytes (32768 x 32760 bf16, 16384 x 32764 fp32; C = 1, hidden = 8): Stage
    A on the whole tables; Stage B on the first and last 24 rows and the rows either side of 256, 512, 768
    and 1024, gathered on the device and checked against the device's tables; every other element holds
    something other than the guard word, both guard bands hold it."""
    l1, l2 = P.TALL[dtype]
    prob = _tall_problem(dtype, (l1, l2))
    assert prob.total == 2 * P.BAND + l1 * l2 and l1 * l2 * P.ESZ[dtype] < 2 ** 31
    h = _dev(prob.h).to(TORCH_DT[dtype])
    alloc = _guarded(prob.total, dtype)
    work = _fresh_work(prob.work_words)
    assert _call(prob, h, work, alloc) == 0
    w = work.cpu().numpy()
    assert (w[prob.work_words:].view(np.uint32) == P.WORK_FILL).all(), "guard: wrote behind the workspace"
    tabs, flags = P.read_work(w, prob)
    a = P.check_tables(prob, tabs, flags)
    print(f"\ntall {dtype}: Stage A {a.figures}")
    assert a.ok, str(a)
    gi, g = alloc.view(INT_DT[dtype]), P.GUARD[dtype]
    assert bool((gi[:P.BAND] == g).all()) and bool((gi[-P.BAND:] == g).all()), "guard: a band was written"
    plane = gi[P.BAND:P.BAND + l1 * l2].view(l1, l2)
    left = int((plane == g).sum())
    assert left == 0, f"{left} elements of the plane keep the guard word"
    sel = [r for r in P.TALL_ROWS if r < l1 - 24] + list(range(l1 - 24, l1))
    idx = torch.tensor(sel, device="cuda")
    picked = plane.index_select(0, idx).reshape(-1)
    band = gi[:P.BAND]
    small = _bits(torch.cat([band, picked, band]).view(TORCH_DT[dtype]))
    sub = types.SimpleNamespace(dtype=dtype, C=1, kernel="rows", total=small.size,
                                descs=[(0, 0, P.BAND, len(sel), l2)])
    ta, tb, tea, teb = tabs[0]
    b = P.check_stream(sub, [(ta[:, sel], tb, tea[:, sel], teb)], flags, small)
    print(f"tall {dtype}: Stage B on rows {sel[:3]} .. {sel[-1]}: {b.figures}")
    assert b.ok, f"(row numbers index {sel}) {b}"
    del alloc, gi, plane, picked
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", P.DTYPES)
@pytest.mark.parametrize("aligned", [1, 0])
def test_a_plane_of_2_31_bytes_is_refused(dtype, aligned):
    """max_l1 * max_l2 * sizeof = 2^31: DI_ERANGE before any launch, output and workspace unwritten."""
    l1, l2 = P.TALL_REFUSED[dtype]
    prob = types.SimpleNamespace(sizes=[(l1, l2)], m1=l1, m2=l2, C=1, H=8, dtype=dtype, eps=P.EPS, aligned=aligned,
                                 work_words=2 * (l1 + l2) + 1, descs=[(0, l1, P.BAND, l1, l2)],
                                 w=np.ones((1, 16), np.float32), b=np.zeros(1, np.float32),
                                 gamma=np.ones(1, np.float32), beta=np.zeros(1, np.float32))
    h = torch.zeros(l1 + l2, 8, device="cuda", dtype=TORCH_DT[dtype])
    out = _guarded(2 * P.BAND, dtype)
    work = _fresh_work(prob.work_words)
    assert _call(prob, h, work, out) == DI_ERANGE
    assert bool((out.view(INT_DT[dtype]) == P.GUARD[dtype]).all()), "a refused call wrote to the output"
    assert bool((work.view(torch.int32) == P.WORK_FILL).all()), "a refused call wrote to the workspace"
