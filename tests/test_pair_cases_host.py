"""What tests/test_gpu_pair_cases.py rests on, checked without a GPU (tests/pair_cases.py):

* ``expand`` equals a plain triple loop over (c, i, j) on tiny ragged batches (gaps, hidden = 1), writes
  every element of every complex and leaves every guard element alone -- so a whole-buffer mismatch on
  the device is the kernel's;
* ``special_rows`` plants every special value in both chains of every complex that has room, gives every
  (row, channel) of a small case its own pattern, never produces the guard word, and its tensors carry
  the exact bits (signalling NaNs included);
* the layouts' alignment classes: 2 for every LINE_CASES batch, >= 1 for ROW_CASES, 0 for FLAT_CASES,
  and each term of the rule on its own;
* the tables hold what they are for: line periods 1, 2, 4, 8 in every LINE_CASES batch and dtype (the
  kernel's formula written out), nt < G, = G, = G + 1 and > 2 G for every period; 16-B chunks per row
  63 .. 65, 127 .. 129 and the row-block edges 64 w +- 1 in ROW_CASES; odd L2, h2 rows and an output off
  the vector, a plane of several chunks in FLAT_CASES;
* a numpy fp32 emulation of plane_rc gives (q // L2, q % L2) within +-2 of every row boundary of the
  TALL_CASES shapes and of (1048000, 1023) -- the margin the 2^20-row limit claims (the device test is
  test_gpu_pair_cases.py's);
* di_pair_tensor_check's range edge at 2^20 + 1 rows and di_pair_job_items at hidden 1 and 24.
"""
import numpy as np
import pytest
import torch

import pair_cases as P

TINY = [  # (sizes, hidden, gap)
    ([(2, 3), (1, 1), (3, 2)], 2, 0),
    ([(1, 4), (5, 1)], 1, 64),
    ([(3, 8), (2, 16), (1, 8)], 3, 128),
]


def _loop(bits, descs, hidden, total, guard):
    out = [guard] * total
    for r1, r2, off, l1, l2 in descs:
        for c in range(2 * hidden):
            for i in range(l1):
                for j in range(l2):
                    out[off + (c * l1 + i) * l2 + j] = int(bits[r1 + i, c] if c < hidden else bits[r2 + j, c - hidden])
    return out


@pytest.mark.parametrize("dtype", P.DTYPES)
@pytest.mark.parametrize("sizes,hidden,gap", TINY)
def test_expand_is_the_triple_loop(dtype, sizes, hidden, gap):
    lay, bits = P.inputs(sizes, dtype, hidden, gap=gap, seed=5)
    guard = P.GUARD[dtype]
    want = P.expand(bits, lay.descs, hidden, lay.total, guard)
    assert want.dtype == P.BITS[dtype] and want.shape == (lay.total,)
    assert want.tolist() == _loop(bits, lay.descs, hidden, lay.total, guard)
    # every element of every complex is written (no input holds the guard word), every guard element
    # -- both bands, every gap -- is left alone
    inside = np.zeros(lay.total, dtype=bool)
    for _, _, off, l1, l2 in lay.descs:
        assert not inside[off:off + 2 * hidden * l1 * l2].any()
        inside[off:off + 2 * hidden * l1 * l2] = True
    assert int(inside.sum()) == lay.payload and not (bits == guard).any()
    assert (want[inside] != guard).all() and (want[~inside] == guard).all()
    assert not inside[:P.BAND].any() and not inside[-P.BAND:].any()
    if gap:
        for (_, _, off, l1, l2), nxt in zip(lay.descs, lay.descs[1:]):
            assert nxt[2] - (off + 2 * hidden * l1 * l2) == gap
    # the error message decodes a flat index
    got = want.copy()
    _, _, off, l1, l2 = lay.descs[1]
    got[off + (1 * l1 + (l1 - 1)) * l2 + (l2 - 1)] ^= 1
    msg = P.first_difference(got, want, lay.descs, hidden)
    assert f"complex 1 ({l1} x {l2}), channel 1, row {l1 - 1}, column {l2 - 1}" in msg, msg
    got = want.copy()
    got[lay.descs[0][2] - 1] ^= 1
    assert "= guard" in P.first_difference(got, want, lay.descs, hidden)
    assert P.first_difference(want.copy(), want, lay.descs, hidden) is None


def _all_cases():
    for case in P.LINE_CASES:
        for dtype in P.DTYPES:
            yield "line", case["name"], dtype, case["sizes"][dtype], case["hidden"], {}
    for case in P.ROW_CASES:
        for dtype in P.DTYPES:
            yield "row", case["name"], dtype, P.row_sizes(case, dtype), case["hidden"], {}
    for case in P.FLAT_CASES:
        for dtype in P.DTYPES:
            yield "flat", case["name"], dtype, case["sizes"], case["hidden"], {"h2_shift": 1, "out_shift": 1}


@pytest.mark.parametrize("dtype", P.DTYPES)
def test_special_rows(dtype):
    sp = set(P.SPECIALS[dtype])
    assert len(sp) == 11
    expo, mant = (0x7F80, 0x007F) if dtype == "bf16" else (0x7F800000, 0x007FFFFF)
    quiet = (mant + 1) >> 1
    nans = [v for v in sp if v & expo == expo and v & mant]
    assert len([v for v in nans if v & quiet]) == 2 and len([v for v in nans if not v & quiet]) == 2
    assert len({v & mant for v in nans}) == 4 and {v >> (15 if dtype == "bf16" else 31) for v in nans} == {0, 1}
    assert {expo, expo | (mant + 1) << 8, 0, (mant + 1) << 8, 1, mant, expo - (mant + 1) | mant} <= sp
    for kind, name, dt, sizes, hidden, kw in _all_cases():
        if dt != dtype:
            continue
        lay, bits = P.inputs(sizes, dtype, hidden, **kw)
        assert bits.shape == (lay.rows, hidden) and bits.dtype == P.BITS[dtype]
        assert not (bits == P.GUARD[dtype]).any(), (kind, name)
        for (start, length) in lay.spans:
            have = sp & set(bits[start:start + length].reshape(-1).tolist())
            assert len(have) >= min(len(sp), length * hidden), (kind, name, start, length, len(have))
        if lay.rows * hidden <= P.DISTINCT_MAX:
            # every (row, channel) its own pattern, but for the planted specials
            # (and the one word that stands in for the guard word)
            plain = bits[~np.isin(bits, list(sp) + [P.GUARD[dtype] ^ 1])]
            assert plain.size >= bits.size - 2 * len(sp) * len(lay.spans) and np.unique(plain).size == plain.size, (kind, name)
    # the tensors hold exactly these bits: a reinterpreting view, signalling NaNs not quieted
    bits = P.special_rows(dtype, 9, 5, seed=1)
    t = P.to_torch(bits, dtype)
    assert t.dtype == (torch.bfloat16 if dtype == "bf16" else torch.float32) and t.shape == (9, 5)
    assert np.array_equal(P.to_bits(t), bits) and np.array_equal(P.to_bits(t.t()), bits.T)
    is_nan = ((bits & expo) == expo) & ((bits & mant) != 0)
    assert np.array_equal(torch.isnan(t).numpy(), is_nan) and int(is_nan.sum()) >= 4 and int(torch.isinf(t).sum()) >= 2
    # random finite base of the large cases: no NaN or inf but the planted ones
    big = P.special_rows(dtype, 1 << 14, 8, seed=2, spans=[(0, 1 << 14)])
    assert int(((big & expo) == expo).sum()) == 6 and not (big == P.GUARD[dtype]).any()


def test_alignment_classes():
    for kind, name, dtype, sizes, hidden, kw in _all_cases():
        lay, _ = P.inputs(sizes, dtype, hidden, **kw)
        cls = lay.aligned()
        assert cls == {"line": 2, "flat": 0}.get(kind, cls) and (kind != "row" or cls >= 1), (kind, name, dtype, cls)
        assert lay.aligned(with_hT=False) == 0
        if kind != "flat":
            gapped = P.Layout(sizes, dtype, hidden, gap=P.GAP)
            assert gapped.aligned() == cls and gapped.total == lay.total + P.GAP * (len(sizes) - 1)
    # each term on its own (bf16, 8-element vectors; 64 elements per 128-B line)
    L = lambda sizes, **kw: P.Layout(sizes, "bf16", 4, **kw).aligned()  # noqa: E731
    assert L([(8, 8), (8, 8)]) == 2
    assert L([(4, 8), (8, 8)]) == 1                       # a plane of 64 B: the next one is off the line
    assert L([(8, 8), (8, 8)], out_shift=8) == 1          # base 16 B into a line
    assert L([(8, 8), (8, 8)], out_shift=4) == 0          # base 8 B off the vector
    assert L([(8, 8), (8, 8)], out_shift=1) == 0
    assert L([(8, 8), (8, 8)], h2_shift=1) == 0           # odd h2 rows
    assert L([(8, 12), (8, 8)]) == 0                      # an L2 off the vector
    assert P.Layout([(8, 4), (8, 4)], "f32", 4).aligned() == 2 and P.Layout([(8, 4), (8, 4)], "bf16", 4).aligned() == 0
    lay = P.Layout([(3, 8), (5, 16)], "bf16", 2, gap=64)
    assert (lay.h1r, lay.h2r, lay.rows) == ([0, 16], [8, 24], 40)
    assert lay.offs == [4096, 4096 + 96 + 64] and lay.total == 4096 + 96 + 64 + 320 + 4096


def test_line_cases_cover_every_period():
    seen = {dt: {p: set() for p in (1, 2, 4, 8)} for dt in P.DTYPES}
    l2_seen = {dt: set() for dt in P.DTYPES}
    for case in P.LINE_CASES:
        assert case["hidden"] in (128, 8)
        for dtype in P.DTYPES:
            periods = set()
            for l1, l2 in case["sizes"][dtype]:
                R = l2 * P.ESZ[dtype]                                  # k_pair_lines' own arithmetic
                low = R & -R
                p = 128 // min(low, 128)
                assert p == P.line_period(l2, dtype) and R % 16 == 0 and l1 % p == 0
                assert l2 in P.LINE_L2[dtype][p] and l1 in (p, 64, 64 + p, 136, 520), (l1, l2)
                assert (l1 - l1 // p * p) * R >> 7 == 0              # the kernel's `tail`: always 0 here
                G, nt = 64 // p, l1 // p
                seen[dtype][p].add("<" if nt < G else "=" if nt == G else "+1" if nt == G + 1 else ">2" if nt > 2 * G else "")
                periods.add(p)
                l2_seen[dtype].add(l2)
            assert periods == {1, 2, 4, 8}, (case["name"], dtype, periods)
            lay, _ = P.inputs(case["sizes"][dtype], dtype, case["hidden"])
            assert lay.total * P.ESZ[dtype] <= 64 << 20
    for dtype in P.DTYPES:
        assert l2_seen[dtype] == {l2 for v in P.LINE_L2[dtype].values() for l2 in v}
        for p, kinds in seen[dtype].items():
            assert {"<", "=", "+1", ">2"} <= kinds, (dtype, p, kinds)
    assert P.LINE_L2["bf16"][1] == (64, 192, 448) and P.LINE_L2["bf16"][2] == (32, 96) and P.LINE_L2["bf16"][4] == (16, 48)


def test_row_cases_cover_the_segment_and_block_edges():
    assert {63, 64, 65, 127, 128, 129} < set(P.ROW_NCH) and P.ROW_WAVES == (1, 2, 4, 8, 16)
    nch_seen, l1_seen = set(), set()
    for case in P.ROW_CASES:
        l1s = [a for a, _ in case["sizes"]]
        assert len(set(-(-a // 64) for a in l1s)) > 1, "ragged L1: empty row blocks past the shorter complexes"
        nch_seen |= {n for _, n in case["sizes"]}
        l1_seen |= set(l1s)
        assert sorted(i for job in case["jobs"] for i in job) == list(range(len(case["sizes"]))) and len(case["jobs"]) == 3
        small = [case["sizes"][i] for i in case["jobs"][0]]
        assert all(P.row_item_stores(a, n) <= 3 for a, n in small) and max(a for a, _ in small) <= 64
        assert any(P.row_item_stores(a, n) > 3 for i in case["jobs"][1] for a, n in [case["sizes"][i]])
        for dtype in P.DTYPES:
            lay, _ = P.inputs(P.row_sizes(case, dtype), dtype, case["hidden"])
            assert lay.total * P.ESZ[dtype] <= 64 << 20 and all(b == P.VEC[dtype] * n for (_, b), (_, n) in
                                                                zip(lay.sizes, case["sizes"]))
    assert nch_seen == set(P.ROW_NCH) and l1_seen >= set(P.ROW_L1)
    assert {c["hidden"] for c in P.ROW_CASES} == {128, 24, 1}
    assert set(P.ROW_L1) >= {63, 65, 127, 129, 255, 257, 511, 513, 1023, 1025}
    # the store count the queue's waited branch depends on: one piece up to 64 chunks, two up to 128
    assert [P.row_item_stores(1, n) for n in (1, 64, 65, 128, 129, 192, 193, 257)] == [1, 1, 2, 2, 3, 3, 4, 5]


def test_flat_cases():
    l2s = set()
    for case in P.FLAT_CASES:
        l2s |= {b for _, b in case["sizes"]}
        for dtype in P.DTYPES:
            lay, _ = P.inputs(case["sizes"], dtype, case["hidden"], h2_shift=1, out_shift=1)
            assert all(r % P.VEC[dtype] == 1 for r in lay.h2r) and all(b % 2 for b in lay.l2s)
            assert lay.total * P.ESZ[dtype] <= 64 << 20
    assert l2s == set(P.FLAT_L2)
    assert any(a * b > 2 * P.PAIR_CHUNK and b % 2 for c in P.FLAT_CASES for a, b in c["sizes"])


def _plane_rc(q, l2):
    """plane_rc of csrc/pair_tensor.hip in numpy: the fp32 quotient, two corrections, 64-bit remainder."""
    inv = np.float32(1.0) / np.float32(l2)
    ii = (q.astype(np.float32) * inv).astype(np.int64)     # (float)q rounds to nearest; the cast truncates
    jj = q.astype(np.int64) - ii * l2
    lo = jj < 0
    ii, jj = ii - lo, jj + lo * l2
    hi = jj >= l2
    return ii + hi, jj - hi * l2


@pytest.mark.parametrize("l1,l2", [s for _, s in P.TALL_CASES] + [P.TALL_LARGE_Q[1], (1048000, 1023)])
def test_plane_rc_margin(l1, l2):
    assert l1 <= P.PAIR_MAX_PLANE_ROWS and l1 * l2 * 4 < 1 << 32
    q = (np.arange(l1 + 1, dtype=np.int64)[:, None] * l2 + np.arange(-2, 3)).reshape(-1)
    q = np.unique(q[(q >= 0) & (q < l1 * l2)]).astype(np.uint32)
    i, j = _plane_rc(q, l2)
    assert np.array_equal(i, q.astype(np.int64) // l2) and np.array_equal(j, q.astype(np.int64) % l2)


def test_tall_cases():
    assert [s for _, s in P.TALL_CASES] == [(1 << 20, 8), (1 << 20, 24), (1 << 20, 3), (1 << 20, 7)]
    assert all(l1 == P.PAIR_MAX_PLANE_ROWS for _, (l1, _) in P.TALL_CASES)
    l1, l2 = P.TALL_LARGE_Q[1]
    assert l1 * l2 > 1 << 24 and l1 * l2 * 2 < 1 << 31 and 2 * l1 * l2 * 2 > 10 ** 9


def test_host_range_checks():
    from deepinteract_amd import _lib
    lib = _lib.load()
    assert lib.di_pair_tensor_check(1, (1 << 20) + 1, 8, 1, 2, None) == -2   # DI_ERANGE: one row too many
    for l2 in (3, 7, 8, 24):
        for esz in (2, 4):
            assert lib.di_pair_tensor_check(1, 1 << 20, l2, 1, esz, None) == 0
    l1, l2 = P.TALL_LARGE_Q[1]
    assert lib.di_pair_tensor_check(1, l1, l2, 1, 2, None) == 0
    assert lib.di_pair_job_items(1, 1, 1) == 2 and lib.di_pair_job_items(3, 65, 1) == 3 * 2 * 2
    assert lib.di_pair_job_items(2, 64, 24) == 2 * 48 and lib.di_pair_job_items(5, 1025, 24) == 5 * 48 * 17
    assert lib.di_pair_job_items(1, 1, 0) == -1
    for case in P.ROW_CASES:
        for job in case["jobs"]:
            l1 = max(case["sizes"][i][0] for i in job)
            assert lib.di_pair_job_items(len(job), l1, case["hidden"]) == len(job) * 2 * case["hidden"] * -(-l1 // 64)
