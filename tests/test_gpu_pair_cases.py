"""The pair-tensor kernels (csrc/pair_tensor.hip) against the byte-exact host oracle of
tests/pair_cases.py, at the edges of their index arithmetic.

Every assertion compares the WHOLE output buffer as integers with pair_cases.expand: the complexes, the
guard bands before and after them and the gaps between them. The buffer is prefilled with a guard word
no input holds, so an element a kernel did not write, a store outside a plane and a NaN payload, a sign
of zero or a subnormal that did not survive all count; a failure names the first differing flat index
as (complex, channel, row, column) or "guard". There is no tolerance: the operation is a copy.

* LINE_CASES: k_pair_lines at line periods 1, 2, 4 and 8 rows mixed in one batch, nt below, at, one past
  and several times its 64-row reload; ROW_CASES: pair_rows_item at 63 .. 65 and 127 .. 129 16-B chunks
  per row and row blocks of 64 w +- 1 rows; both through PairTensorOp for every kernel, 1 .. 16 waves per
  block, beside or alone, one block or one per CU, hidden 128 / 24 / 8 / 1, and through the C ABI with
  gaps between the complexes.
* FLAT_CASES: k_pair_flat on odd shapes off every vector boundary, with hT and with the strided read.
* TALL_CASES: plane_rc at 2^20 rows and at flat positions past 2^24.
* PairTensorOp's alignment classes, and the queue kernels (di_pair_stream / di_pair_help) at 1 and 16
  waves per block on jobs cut from ROW_CASES.
"""
import ctypes

import numpy as np
import pytest
import torch

import pair_cases as P

pytestmark = pytest.mark.gpu

TORCH_DT = {"bf16": torch.bfloat16, "f32": torch.float32}
INT_DT = {"bf16": torch.int16, "f32": torch.int32}


def _guard_int(dtype):
    """The guard word as the signed integer of the buffer's integer view."""
    return int(np.array(P.GUARD[dtype], dtype=P.BITS[dtype]).view(np.int16 if dtype == "bf16" else np.int32))


def _device_inputs(bits, dtype):
    """h [rows, H] and hT [H, rows] with exactly the bits of `bits` (transposed as integers)."""
    h = P.to_torch(bits, dtype, "cuda")
    hT = h.view(INT_DT[dtype]).t().contiguous().view(TORCH_DT[dtype])
    return h, hT


def _guarded(lay):
    """(allocation, base): lay.out_shift + lay.total elements of the guard word; base starts out_shift
    elements in (the buffer the layout's offsets count from)."""
    alloc = torch.full((lay.out_shift + lay.total,), _guard_int(lay.dtype), dtype=INT_DT[lay.dtype], device="cuda")
    alloc = alloc.view(TORCH_DT[lay.dtype])
    assert alloc.data_ptr() % 128 == 0
    return alloc, alloc[lay.out_shift:]


def _check(alloc, lay, want, what):
    got = P.to_bits(alloc)
    assert (got[:lay.out_shift] == P.GUARD[lay.dtype]).all(), f"{what}: wrote before the buffer"
    diff = P.first_difference(got[lay.out_shift:], want, lay.descs, lay.hidden)
    assert diff is None, f"{what}: {diff}"


def _run_op(lay, h, hT, kernel="auto", waves=0, beside=False, blocks=0):
    """PairTensorOp on out = base[band:] of a fresh guarded buffer (a layout without gaps: the op's own
    descriptors, complexes back to back from the start of `out`). Returns the allocation."""
    from deepinteract_amd.engine import PairTensorOp
    assert lay.gap == 0
    alloc, base = _guarded(lay)
    op = PairTensorOp(kernel=kernel, blocks=blocks, waves_per_block=waves, beside=beside)
    out, views = op(h, lay.h1r, lay.h2r, lay.l1s, lay.l2s, out=base[lay.band:], hT=hT)
    assert out.data_ptr() == base.data_ptr() + lay.band * P.ESZ[lay.dtype]
    assert [tuple(v.shape) for v in views] == [(1, 2 * lay.hidden, a, b) for a, b in lay.sizes]
    return alloc


def _desc_table(lay):
    from deepinteract_amd import _lib
    arr = (_lib.DiPairDesc * len(lay.descs))(*[_lib.DiPairDesc(*d) for d in lay.descs])
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()


def _run_capi(lay, h, hT, launch):
    """di_pair_tensor with hand-built descriptors (absolute out_off: bands and gaps) and the layout's own
    alignment class. launch: None or (kernel, waves, beside, blocks)."""
    from deepinteract_amd import _lib
    from deepinteract_amd.engine import _ptr, _stream
    lib = _lib.load()
    alloc, base = _guarded(lay)
    d = _desc_table(lay)
    cls = lay.aligned(with_hT=hT is not None)
    lp = None
    if launch is not None:
        kernel, waves, beside, blocks = launch
        need = {_lib.DI_PAIR_LINES: 2, _lib.DI_PAIR_ROWS: 1, _lib.DI_PAIR_VECTOR: 1}.get(kernel, 0)
        assert cls >= need, "the test would ask for a kernel the layout does not allow"
        lp = ctypes.byref(_lib.DiPairLaunch(kernel, blocks, waves, int(beside)))
    dt = _lib.DI_BF16 if lay.dtype == "bf16" else _lib.DI_F32
    _lib.check(lib.di_pair_tensor(dt, _ptr(d), len(lay.sizes), max(lay.l1s), max(lay.l2s), lay.hidden, cls, _ptr(h),
                                  _ptr(hT), lay.rows, lp, _ptr(base), _stream()), "di_pair_tensor")
    torch.cuda.synchronize()
    return alloc


def _label(launch):
    kernel, waves, beside = launch[:3]
    return f"{kernel}-w{waves}{'-beside' if beside else ''}" + (f"-b{launch[3]}" if len(launch) > 3 else "")


WAVE_LAUNCHES = lambda kernel: [(kernel, w, b) for w in P.ROW_WAVES for b in (False, True)]  # noqa: E731
ROW_LAUNCHES = WAVE_LAUNCHES("rows") + [("vector", 0, False), ("auto", 0, False)]
LINE_LAUNCHES = WAVE_LAUNCHES("lines") + [("rows", 4, False), ("rows", 16, True), ("vector", 0, False), ("auto", 0, False)]

LINE_PARAMS = [pytest.param(case, dtype, launch, id=f"{case['name']}-{dtype}-{_label(launch)}")
               for case in P.LINE_CASES for dtype in P.DTYPES for launch in LINE_LAUNCHES]
ROW_PARAMS = [pytest.param(case, dtype, launch, id=f"{case['name']}-{dtype}-{_label(launch)}")
              for case in P.ROW_CASES for dtype in P.DTYPES for launch in ROW_LAUNCHES]


@pytest.mark.parametrize("case,dtype,launch", LINE_PARAMS)
def test_line_cases(case, dtype, launch):
    """128-B aligned planes of every line period through every kernel that takes them."""
    sizes, hidden = case["sizes"][dtype], case["hidden"]
    lay, bits = P.inputs(sizes, dtype, hidden)
    assert lay.aligned() == 2
    h, hT = _device_inputs(bits, dtype)
    kernel, waves, beside = launch
    alloc = _run_op(lay, h, hT, kernel, waves, beside)
    _check(alloc, lay, P.expected(sizes, dtype, hidden), f"LINE_CASES {case['name']} {dtype} {_label(launch)}")


@pytest.mark.parametrize("case,dtype,launch", ROW_PARAMS)
def test_row_cases(case, dtype, launch):
    """16-B aligned planes at the row-segment and row-block edges through the row and vector kernels."""
    sizes, hidden = P.row_sizes(case, dtype), case["hidden"]
    lay, bits = P.inputs(sizes, dtype, hidden)
    assert lay.aligned() >= 1
    h, hT = _device_inputs(bits, dtype)
    kernel, waves, beside = launch
    alloc = _run_op(lay, h, hT, kernel, waves, beside)
    _check(alloc, lay, P.expected(sizes, dtype, hidden), f"ROW_CASES {case['name']} {dtype} {_label(launch)}")


ONE_BLOCK = [(P.LINE_CASES[0], P.LINE_CASES[0]["sizes"], launch)
             for launch in (("lines", 1, False), ("lines", 4, True), ("lines", 16, False), ("rows", 2, True), ("vector", 0, False))] + \
            [(case, None, launch) for case in (P.ROW_CASES[0], P.ROW_CASES[2])
             for launch in (("rows", 1, True), ("rows", 4, False), ("rows", 16, False), ("vector", 0, False), ("auto", 0, False))]


@pytest.mark.parametrize("dtype", P.DTYPES)
@pytest.mark.parametrize("case,sizes,launch", [pytest.param(c, s, l, id=f"{c['name']}-{_label(l)}") for c, s, l in ONE_BLOCK])
def test_one_block_walks_every_item(case, sizes, launch, dtype):
    """blocks = 1: a single block's persistent loop visits every work item, the empty ones included."""
    sizes = sizes[dtype] if sizes is not None else P.row_sizes(case, dtype)
    lay, bits = P.inputs(sizes, dtype, case["hidden"])
    h, hT = _device_inputs(bits, dtype)
    kernel, waves, beside = launch
    alloc = _run_op(lay, h, hT, kernel, waves, beside, blocks=1)
    _check(alloc, lay, P.expected(sizes, dtype, case["hidden"]), f"{case['name']} {dtype} {_label(launch)} blocks=1")


def _capi_launches(kind):
    from deepinteract_amd import _lib
    rows = [(_lib.DI_PAIR_ROWS, 1, True, 0), (_lib.DI_PAIR_ROWS, 8, False, 0), (_lib.DI_PAIR_ROWS, 16, False, 1),
            (_lib.DI_PAIR_VECTOR, 0, False, 0), (_lib.DI_PAIR_AUTO, 0, False, 0), None]
    lines = [(_lib.DI_PAIR_LINES, 1, False, 0), (_lib.DI_PAIR_LINES, 8, True, 0), (_lib.DI_PAIR_LINES, 16, False, 1)]
    return lines + rows[:1] + rows[3:] if kind == "line" else rows


GAPPED = [("line", c) for c in P.LINE_CASES] + [("row", c) for c in P.ROW_CASES]


@pytest.mark.parametrize("dtype", P.DTYPES)
@pytest.mark.parametrize("kind,case", [pytest.param(k, c, id=f"{k}-{c['name']}") for k, c in GAPPED])
def test_gapped_layouts_through_the_c_abi(kind, case, dtype):
    """out_off with guard gaps between the complexes (the C ABI allows them, PairTensorOp never makes
    them): no kernel writes into a gap, before the first or past the last complex. launch = NULL too."""
    sizes = case["sizes"][dtype] if kind == "line" else P.row_sizes(case, dtype)
    lay, bits = P.inputs(sizes, dtype, case["hidden"], gap=P.GAP)
    assert lay.aligned() == (2 if kind == "line" else P.Layout(sizes, dtype, case["hidden"]).aligned())
    h, hT = _device_inputs(bits, dtype)
    want = P.expected(sizes, dtype, case["hidden"], gap=P.GAP)
    for launch in _capi_launches(kind):
        alloc = _run_capi(lay, h, hT, launch)
        _check(alloc, lay, want, f"{kind} {case['name']} {dtype} gap={P.GAP} launch={launch}")
        del alloc


@pytest.mark.parametrize("with_hT", [True, False], ids=["hT", "strided"])
@pytest.mark.parametrize("dtype", P.DTYPES)
@pytest.mark.parametrize("case", P.FLAT_CASES, ids=[c["name"] for c in P.FLAT_CASES])
def test_flat_cases(case, dtype, with_hT):
    """k_pair_flat: odd L2, h2 rows off the vector, the output one element off a 16-B boundary, a plane
    of several 65536-element chunks; chain 2 read from hT and (hT = None) strided from h. Through
    PairTensorOp (auto must classify the batch generic) and through the C ABI with gaps."""
    lay, bits = P.inputs(case["sizes"], dtype, case["hidden"], h2_shift=1, out_shift=1)
    assert lay.aligned() == 0
    h, hT = _device_inputs(bits, dtype)
    alloc = _run_op(lay, h, hT if with_hT else None)
    assert alloc[1:].data_ptr() % 16 == P.ESZ[dtype]
    _check(alloc, lay, P.expected(case["sizes"], dtype, case["hidden"], h2_shift=1, out_shift=1),
           f"FLAT_CASES {case['name']} {dtype} hT={with_hT}")
    gapped, gbits = P.inputs(case["sizes"], dtype, case["hidden"], gap=P.GAP, h2_shift=1, out_shift=1)
    alloc = _run_capi(gapped, h, hT if with_hT else None, None)
    assert np.array_equal(gbits, bits)
    _check(alloc, gapped, P.expected(case["sizes"], dtype, case["hidden"], gap=P.GAP, h2_shift=1, out_shift=1),
           f"FLAT_CASES {case['name']} {dtype} hT={with_hT} gap={P.GAP}")


@pytest.mark.parametrize("dtype", P.DTYPES)
def test_every_choice_writes_the_same_bytes(dtype):
    """PairTensorOp's promise, asserted directly: one LINE_CASES batch through every kernel and launch
    shape gives identical buffers (bands included); a failure names the two choices."""
    case = P.LINE_CASES[0]
    sizes, hidden = case["sizes"][dtype], case["hidden"]
    lay, bits = P.inputs(sizes, dtype, hidden)
    h, hT = _device_inputs(bits, dtype)
    choices = [(k, w, b, blocks) for k in ("lines", "rows") for w in P.ROW_WAVES for b in (False, True) for blocks in (0, 1)]
    choices += [("vector", 0, False, 0), ("vector", 0, False, 1), ("auto", 0, False, 0), ("auto", 0, True, 0)]
    first = None
    for ch in choices:
        got = _run_op(lay, h, hT, *ch).view(INT_DT[dtype])
        if first is None:
            first = (ch, got)
            _check(got.view(TORCH_DT[dtype]), lay, P.expected(sizes, dtype, hidden), f"{_label(ch)}")
        elif not torch.equal(got, first[1]):
            i = int((got != first[1]).nonzero()[0])
            raise AssertionError(f"{_label(ch)} and {_label(first[0])} write different bytes; first at flat index {i} "
                                 f"= {P.locate(i, lay.descs, hidden)}")
    # the generic kernel on the same batch (hT withheld: class 0) writes them too
    got = _run_op(lay, h, None).view(INT_DT[dtype])
    assert torch.equal(got, first[1]), "flat and " + _label(first[0])


# ---- the fp32-quotient row index at its limit -----------------------------------------------------------
TALL = [pytest.param(size, dtype, kernel, id=f"{size[0]}x{size[1]}-{dtype}-{kernel}")
        for kernels, size in P.TALL_CASES for dtype in P.DTYPES
        for kernel in (kernels if kernels != ("flat",) else ("flat-hT", "flat-strided"))]


@pytest.mark.parametrize("size,dtype,kernel", TALL)
def test_tall_planes(size, dtype, kernel):
    """2^20 rows (PAIR_MAX_PLANE_ROWS, where plane_rc's fp32 quotient is documented exact), hidden = 1:
    every row of both planes, compared on the host."""
    lay = P.Layout([size], dtype, 1)
    bits = P.special_rows(dtype, lay.rows, 1, seed=7, spans=lay.spans)
    h, hT = _device_inputs(bits, dtype)
    if kernel.startswith("flat"):
        assert lay.aligned() == 0
        alloc = _run_op(lay, h, hT if kernel == "flat-hT" else None)
    else:
        assert lay.aligned() >= 1
        alloc = _run_op(lay, h, hT, kernel)
    want = P.expand(bits, lay.descs, 1, lay.total, P.GUARD[dtype])
    _check(alloc, lay, want, f"{size} {dtype} {kernel}")


@pytest.mark.parametrize("kernel", P.TALL_LARGE_Q[0])
def test_large_flat_positions(kernel):
    """(262144, 1000) bf16, hidden = 1: flat positions up to 2.6e8, where (float)q is no longer exact.
    1 GB, so planes and guard bands are compared on the device (as integers)."""
    dtype, (l1, l2) = "bf16", P.TALL_LARGE_Q[1]
    lay = P.Layout([(l1, l2)], dtype, 1)
    bits = P.special_rows(dtype, lay.rows, 1, seed=8, spans=lay.spans)
    h, hT = _device_inputs(bits, dtype)
    alloc = _run_op(lay, h, hT, kernel)
    torch.cuda.synchronize()
    gi, hb, g = alloc.view(torch.int16), h.view(torch.int16), _guard_int(dtype)
    assert bool((gi[:lay.band] == g).all()) and bool((gi[-lay.band:] == g).all()), "a guard band was written"
    t = gi[lay.band:lay.band + 2 * l1 * l2].view(2, l1, l2)
    assert lay.band + 2 * l1 * l2 + lay.band == gi.numel()
    want = (hb[lay.h1r[0]:lay.h1r[0] + l1, 0].unsqueeze(1).expand(l1, l2), hb[lay.h2r[0]:lay.h2r[0] + l2, 0].unsqueeze(0).expand(l1, l2))
    for c in (0, 1):
        bad = t[c] != want[c]
        if bool(bad.any()):
            i, j = bad.nonzero()[0].tolist()
            raise AssertionError(f"{kernel}: channel {c}, row {i}, column {j} (flat position {i * l2 + j}): "
                                 f"got {int(t[c, i, j]) & 0xffff:#x}, expected {int(want[c][i, j]) & 0xffff:#x}")
        del bad
    del alloc, gi, t
    torch.cuda.empty_cache()


# ---- PairTensorOp's alignment classes -------------------------------------------------------------------
@pytest.mark.parametrize("dtype", P.DTYPES)
def test_op_refuses_lines_off_the_line(dtype):
    """16-B but not 128-B aligned planes: "lines" raises before any launch, auto is exact."""
    case = P.ROW_CASES[0]
    sizes = P.row_sizes(case, dtype)
    lay, bits = P.inputs(sizes, dtype, case["hidden"])
    assert lay.aligned() == 1
    h, hT = _device_inputs(bits, dtype)
    with pytest.raises(ValueError):
        _run_op(lay, h, hT, "lines")
    _check(_run_op(lay, h, hT, "auto"), lay, P.expected(sizes, dtype, case["hidden"]), "auto on 16-B planes")


@pytest.mark.parametrize("how", ["out+8B", "odd-h2-row"])
@pytest.mark.parametrize("dtype", P.DTYPES)
def test_op_takes_the_generic_path_off_the_vector(dtype, how):
    """Vector-sized rows, but the output 8 bytes off a 16-B boundary, or every h2 row off the vector:
    auto must take the generic kernel (exact bytes), "rows" / "vector" / "lines" raise ValueError and
    leave the buffer untouched."""
    from deepinteract_amd.engine import PairTensorOp
    case = P.ROW_CASES[0]
    sizes, hidden = P.row_sizes(case, dtype), case["hidden"]
    kw = {"out_shift": 8 // P.ESZ[dtype]} if how == "out+8B" else {"h2_shift": 1}
    lay, bits = P.inputs(sizes, dtype, hidden, **kw)
    assert lay.aligned() == 0 and P.Layout(sizes, dtype, hidden).aligned() >= 1
    h, hT = _device_inputs(bits, dtype)
    want = P.expected(sizes, dtype, hidden, **kw)
    _check(_run_op(lay, h, hT, "auto"), lay, want, f"auto, {how}")
    alloc, base = _guarded(lay)
    if how == "out+8B":
        assert base[lay.band:].data_ptr() % 16 == 8
    for kernel in ("rows", "vector", "lines"):
        with pytest.raises(ValueError):
            PairTensorOp(kernel=kernel)(h, lay.h1r, lay.h2r, lay.l1s, lay.l2s, out=base[lay.band:], hT=hT)
    torch.cuda.synchronize()
    assert bool((alloc.view(INT_DT[dtype]) == _guard_int(dtype)).all()), "a refused call wrote to the buffer"


def test_op_refuses_a_short_buffer():
    from deepinteract_amd.engine import PairTensorOp
    lay, bits = P.inputs([(3, 8), (5, 16)], "bf16", 4)
    h, hT = _device_inputs(bits, "bf16")
    alloc, base = _guarded(lay)
    with pytest.raises(ValueError):
        PairTensorOp()(h, lay.h1r, lay.h2r, lay.l1s, lay.l2s, out=base[lay.band:lay.band + lay.payload - 1], hT=hT)
    torch.cuda.synchronize()
    assert bool((alloc.view(torch.int16) == _guard_int("bf16")).all())
    out, _ = PairTensorOp()(h, lay.h1r, lay.h2r, lay.l1s, lay.l2s, out=base[lay.band:lay.band + lay.payload], hT=hT)
    _check(alloc, lay, P.expected([(3, 8), (5, 16)], "bf16", 4), "an output of exactly the payload")


# ---- the queue kernels ----------------------------------------------------------------------------------
QUEUE_SHAPES = [("s1x1-h1", (1, 1), 1), ("s1x1-h16", (1, 1), 16), ("s16-h1", (0, 16), 1), ("s16-h16", (0, 16), 16)]


@pytest.mark.parametrize("name,stream_shape,help_waves", QUEUE_SHAPES, ids=[s[0] for s in QUEUE_SHAPES])
@pytest.mark.parametrize("case", P.ROW_CASES, ids=[c["name"] for c in P.ROW_CASES])
@pytest.mark.parametrize("dtype", P.DTYPES)
def test_queue_jobs(dtype, case, name, stream_shape, help_waves):
    """di_pair_signal / di_pair_stream / di_pair_help over three jobs cut from a ROW_CASES batch (one
    hidden per run: 128, 24, 1), gapped guarded outputs, special-value inputs; the stream kernel as one
    wave and as 16-wave blocks, the help kernel at 1 and 16 waves per block. Job 0's items have at most
    3 stores each (the stream kernel waits for its next ticket itself) and fewer items than a full launch
    has waves. Every job is signalled from the producer stream before the first help launch; nothing
    waits for a signal that is not sent."""
    from deepinteract_amd import _lib
    from deepinteract_amd.pipeline import PairQueue, schedule_streams
    lib = _lib.load()
    hidden = case["hidden"]
    jobs, keep = [], []
    for n, idx in enumerate(case["jobs"]):
        sizes = P.row_sizes(case, dtype, idx)
        lay, bits = P.inputs(sizes, dtype, hidden, gap=P.GAP, seed=10 + n)
        assert lay.aligned() >= 1 and lay.out_shift == 0
        h, hT = _device_inputs(bits, dtype)
        alloc, base = _guarded(lay)
        d = _desc_table(lay)
        items = lib.di_pair_job_items(len(sizes), max(lay.l1s), hidden)
        assert items == len(sizes) * 2 * hidden * -(-max(lay.l1s) // 64)
        jobs.append(_lib.DiPairJob(hT.data_ptr(), d.data_ptr(), base.data_ptr(), lay.rows, len(sizes), max(lay.l1s), items))
        keep.append((lay, sizes, 10 + n, hT, d, alloc))
    assert max(P.row_item_stores(a, n) for a, n in [case["sizes"][i] for i in case["jobs"][0]]) <= 3
    q = PairQueue(torch.device("cuda"), len(jobs))
    q.set_jobs(jobs)
    di = _lib.DI_BF16 if dtype == "bf16" else _lib.DI_F32
    main, side = schedule_streams()
    st = lambda s: ctypes.c_void_p(s.cuda_stream)  # noqa: E731
    qp, jp = ctypes.c_void_p(q.state.data_ptr()), ctypes.c_void_p(q.jobs.data_ptr())
    sl = _lib.DiPairLaunch(_lib.DI_PAIR_AUTO, stream_shape[0], stream_shape[1], 0)
    hl = _lib.DiPairLaunch(_lib.DI_PAIR_AUTO, 0, help_waves, 0)
    torch.cuda.synchronize()
    _lib.check(lib.di_pair_stream(di, jp, 0, len(jobs), hidden, qp, ctypes.byref(sl), 200.0, st(side)), "di_pair_stream")
    for j in range(len(jobs)):
        _lib.check(lib.di_pair_signal(qp, j, st(main)), "di_pair_signal")
    _lib.check(lib.di_pair_help(di, jp, 0, 1, hidden, qp, ctypes.byref(hl), -1, st(main)), "di_pair_help")
    _lib.check(lib.di_pair_help(di, jp, 2, len(jobs) - 1, hidden, qp, ctypes.byref(hl), -1, st(main)), "di_pair_help (drain)")
    torch.cuda.synchronize()
    cnt = q.counters()
    payload = sum(lay.payload for lay, *_ in keep) * P.ESZ[dtype]
    assert cnt["error"] == 0 and cnt["gave_up"] == 0 and cnt["signalled"] == len(jobs), cnt
    assert cnt["stream_bytes"] + cnt["help_bytes"] == payload, (cnt, payload)
    for n, (lay, sizes, seed, _, _, alloc) in enumerate(keep):
        _check(alloc, lay, P.expected(sizes, dtype, hidden, gap=P.GAP, seed=seed), f"{case['name']} {dtype} {name} job {n}")
