"""Case tables and the byte-exact host oracle of the pair-tensor kernels (csrc/pair_tensor.hip), shared by
tests/test_pair_cases_host.py (CPU) and tests/test_gpu_pair_cases.py (GPU). No tests here; importable
without a GPU (numpy only; torch is imported where a tensor is made).

The operation is a copy: T[c, i, j] = h1[i, c] (c < H), h2[j, c - H] (c >= H). Its exact reference is an
integer expansion of the inputs' bit patterns (uint16 for bf16, uint32 for fp32), so everything here
works on bits: NaN payloads, signs of zero, infinities and subnormals are ordinary integers.

* ``expand``: the WHOLE expected output buffer -- guard word everywhere, every complex's [2H, L1, L2]
  block at its out_off -- so a compare against it also sees what a kernel wrote outside its planes
  (the bands before the first and after the last complex, the gaps between complexes) and what it did
  not write (the buffer is prefilled with the guard word, which no input holds).
* ``special_rows``: node features as bit patterns, special values planted in every chain.
* ``Layout``: rows (chain 2 on a 16-B vector), out_off (bands, optional gaps) and the alignment class
  (0 generic / 1 16-B planes / 2 128-B planes) of one list of (L1, L2), restated independently of
  PairTensorOp.
* ``LINE_CASES`` / ``ROW_CASES`` / ``FLAT_CASES`` / ``TALL_CASES``: fixed shapes at the edges of the
  kernels' index arithmetic (see each table).
"""
import functools

import numpy as np

DTYPES = ("bf16", "f32")
VEC = {"bf16": 8, "f32": 4}       # elements of a 16-byte vector
ESZ = {"bf16": 2, "f32": 4}
BITS = {"bf16": np.uint16, "f32": np.uint32}
# what the output holds before the kernel runs; special_rows never produces it
GUARD = {"bf16": 0xA5C3, "f32": 0xA5C3F00D}
BAND = 4096                       # guard elements before the first and after the last complex
GAP = 192                         # guard elements between complexes of a gapped layout (3 x 128 B in bf16)

# quiet NaNs (two payloads, both signs), signalling NaNs (quiet bit clear, two payloads, both signs),
# +-inf, +-0, the smallest and the largest subnormal, the largest finite value
SPECIALS = {
    "bf16": (0x7FC1, 0xFFC2, 0x7F81, 0xFFA3, 0x7F80, 0xFF80, 0x0000, 0x8000, 0x0001, 0x007F, 0x7F7F),
    "f32": (0x7FC00001, 0xFFC12345, 0x7F800001, 0xFFA00002, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000,
            0x00000001, 0x007FFFFF, 0x7F7FFFFF),
}
DISTINCT_MAX = 1 << 16            # rows * hidden up to which every (row, channel) gets its own pattern


# ---- the oracle ---------------------------------------------------------------------------------------
def expand(bits_h, descs, hidden, total, guard_word):
    """The expected output buffer of di_pair_tensor as bit patterns: `total` elements of bits_h's integer
    dtype, `guard_word` wherever no complex lies. bits_h: [rows, hidden] unsigned integers; descs: one
    (h1_row, h2_row, out_off, l1, l2) per complex. Integer indexing and broadcasting only."""
    assert bits_h.dtype in (np.uint16, np.uint32) and bits_h.ndim == 2 and bits_h.shape[1] == hidden
    out = np.full(total, guard_word, dtype=bits_h.dtype)
    for r1, r2, off, l1, l2 in descs:
        n = 2 * hidden * l1 * l2
        assert 0 <= off and off + n <= total, (off, n, total)
        blk = out[off:off + n].reshape(2 * hidden, l1, l2)
        blk[:hidden] = bits_h[r1:r1 + l1].T[:, :, None]
        blk[hidden:] = bits_h[r2:r2 + l2].T[:, None, :]
    return out


def locate(idx, descs, hidden):
    """Flat buffer index -> "complex n, channel c, row i, column j", or "guard" outside every complex."""
    for n, (_, _, off, l1, l2) in enumerate(descs):
        if off <= idx < off + 2 * hidden * l1 * l2:
            c, rest = divmod(idx - off, l1 * l2)
            return f"complex {n} ({l1} x {l2}), channel {c}, row {rest // l2}, column {rest % l2}"
    return "guard"


def first_difference(got, want, descs, hidden):
    """None when the two integer buffers are equal, else a message naming the first differing element."""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if np.array_equal(got, want):
        return None
    bad = np.flatnonzero(got != want)
    i = int(bad[0])
    return (f"{bad.size} of {got.size} elements differ; first at flat index {i} = {locate(i, descs, hidden)}: "
            f"got {int(got[i]):#x}, expected {int(want[i]):#x}")


# ---- inputs -------------------------------------------------------------------------------------------
def special_rows(dtype, rows, hidden, seed, spans=None, distinct=None):
    """[rows, hidden] node features as bit patterns (BITS[dtype]).

    Base: where rows * hidden <= DISTINCT_MAX (`distinct` None) every (row, channel) holds its own
    pattern, (row * hidden + c + 1) * an odd constant truncated to the element width (a bijection of the
    width's integers, so a transposed or shifted read meets a different word); otherwise random finite
    values (a random word whose all-ones exponent is cleared). Then every entry of SPECIALS[dtype] is
    planted at a random (row, channel) of each span (start row, rows) -- the chains of a Layout; where a
    span has fewer slots than specials it takes as many as fit, starting at a different special for each
    span. No element equals GUARD[dtype] (an element that would holds GUARD ^ 1 instead)."""
    rng = np.random.default_rng(seed)
    ut, width = BITS[dtype], 8 * ESZ[dtype]
    if distinct is None:
        distinct = rows * hidden <= DISTINCT_MAX
    if distinct:
        odd = 0x9E3779B1 if width == 32 else 0x9E37
        b = ((np.arange(1, rows * hidden + 1, dtype=np.uint64) * odd) & ((1 << width) - 1)).astype(ut)
    else:
        b = rng.integers(0, 1 << width, size=rows * hidden, dtype=np.uint64).astype(ut)
        expo, low = (0x7F80, 0x0080) if width == 16 else (0x7F800000, 0x00800000)
        b[(b & ut(expo)) == ut(expo)] &= ut(((1 << width) - 1) ^ low)   # exponent 0xFF -> 0xFE: finite
    b = b.reshape(rows, hidden)
    sp = SPECIALS[dtype]
    for n, (start, length) in enumerate(spans or [(0, rows)]):
        slots = length * hidden
        take = min(slots, len(sp))
        where = rng.choice(slots, size=take, replace=False)
        for k, w in enumerate(where):
            b[start + w // hidden, w % hidden] = sp[(n + k) % len(sp)]
    guard = ut(GUARD[dtype])
    b[b == guard] = guard ^ ut(1)
    return b


def to_torch(bits, dtype, device="cpu"):
    """A bf16 / fp32 tensor with exactly these bit patterns (a reinterpreting view: no float conversion)."""
    import torch
    signed = np.ascontiguousarray(bits).view(np.int16 if dtype == "bf16" else np.int32)
    return torch.from_numpy(signed.copy()).to(device).view(torch.bfloat16 if dtype == "bf16" else torch.float32)


def to_bits(t):
    """The bit patterns of a bf16 / fp32 tensor as a numpy array of BITS (synchronises)."""
    import torch
    it = torch.int16 if t.element_size() == 2 else torch.int32
    return t.contiguous().view(it).cpu().numpy().view(np.uint16 if t.element_size() == 2 else np.uint32)


# ---- layouts ------------------------------------------------------------------------------------------
class Layout:
    """Rows and output offsets of one list of (L1, L2) sizes.

    Rows: chain 1 of a complex starts where the previous complex ended; chain 2 starts on the next
    multiple of the 16-B vector, plus `h2_shift` rows (1: no h2 row on a vector); the row count is padded
    to the vector. Output: BAND guard elements (`band`), then the complexes with `gap` guard elements
    between them (a multiple of 64 elements, which keeps 128-B alignment in both dtypes), then the band
    again; `out_shift` elements move the buffer's base off its 128-B allocation boundary (a view that
    starts `out_shift` elements into an allocation). ``descs`` are absolute (the C ABI, base = the
    allocation + out_shift); ``rel_descs`` are relative to the first complex (what PairTensorOp builds
    for out = buffer[band:]) and exist when gap == 0."""

    def __init__(self, sizes, dtype, hidden, gap=0, band=BAND, h2_shift=0, out_shift=0):
        assert gap % 64 == 0 and band % 64 == 0 and band >= 4096
        vec = VEC[dtype]
        self.sizes, self.dtype, self.hidden, self.gap, self.band = list(sizes), dtype, hidden, gap, band
        self.h2_shift, self.out_shift = h2_shift, out_shift
        self.h1r, self.h2r, self.offs = [], [], []
        r, off = 0, band
        for a, b in sizes:
            self.h1r.append(r)
            r2 = -(-(r + a) // vec) * vec + h2_shift
            self.h2r.append(r2)
            r = r2 + b
            self.offs.append(off)
            off += 2 * hidden * a * b + gap
        self.rows = -(-r // vec) * vec
        self.total = off - gap + band
        self.l1s, self.l2s = [a for a, _ in sizes], [b for _, b in sizes]
        self.descs = [(r1, r2, o, a, b) for r1, r2, o, (a, b) in zip(self.h1r, self.h2r, self.offs, sizes)]
        self.payload = sum(2 * hidden * a * b for a, b in sizes)   # elements the kernels must write

    @property
    def spans(self):
        return [s for r1, r2, (a, b) in zip(self.h1r, self.h2r, self.sizes) for s in ((r1, a), (r2, b))]

    def aligned(self, with_hT=True):
        """The alignment class di_pair_tensor is told: 1 when hT is given and every 16-B access of the
        row / vector kernels is aligned (the row count hT is strided by, every h2 row, every L2, every
        out_off and the base), 2 when also every channel plane starts on a 128-B line (base, out_off
        and L1 * L2 bytes), else 0. The base is a 128-B aligned allocation plus out_shift elements."""
        vec, esz = VEC[self.dtype], ESZ[self.dtype]
        base = self.out_shift * esz
        if not (with_hT and self.rows % vec == 0 and base % 16 == 0 and all(b % vec == 0 for b in self.l2s)
                and all(o % vec == 0 for o in self.offs) and all(r % vec == 0 for r in self.h2r)):
            return 0
        if base % 128 == 0 and all(o * esz % 128 == 0 for o in self.offs) \
                and all(a * b * esz % 128 == 0 for a, b in self.sizes):
            return 2
        return 1


def line_period(l2, dtype):
    """Rows after which a channel plane's 128-B lines repeat: 128 / gcd(row bytes, 128)."""
    return 128 // np.gcd(l2 * ESZ[dtype], 128)


@functools.lru_cache(maxsize=None)
def _inputs(sizes, dtype, hidden, gap, h2_shift, out_shift, seed):
    lay = Layout(sizes, dtype, hidden, gap=gap, h2_shift=h2_shift, out_shift=out_shift)
    bits = special_rows(dtype, lay.rows, hidden, seed, spans=lay.spans)
    bits.setflags(write=False)
    return lay, bits


def inputs(sizes, dtype, hidden, gap=0, h2_shift=0, out_shift=0, seed=0):
    """(Layout, node-feature bits) of a case, computed once and shared (read-only)."""
    return _inputs(tuple(sizes), dtype, hidden, gap, h2_shift, out_shift, seed)


@functools.lru_cache(maxsize=4)
def _expected(sizes, dtype, hidden, gap, h2_shift, out_shift, seed):
    lay, bits = _inputs(sizes, dtype, hidden, gap, h2_shift, out_shift, seed)
    want = expand(bits, lay.descs, hidden, lay.total, GUARD[dtype])
    want.setflags(write=False)
    return want


def expected(sizes, dtype, hidden, gap=0, h2_shift=0, out_shift=0, seed=0):
    """expand() of inputs(...) (the few latest are kept: the launch shapes of one case run in a row)."""
    return _expected(tuple(sizes), dtype, hidden, gap, h2_shift, out_shift, seed)


# ---- the tables ---------------------------------------------------------------------------------------
# k_pair_lines: p = 128 / gcd(row bytes, 128) rows per period, G = 64 / p repeats per 64 loaded chain-1
# rows, nt = L1 / p repeats per plane. Every plane is 128-B aligned (L1 a multiple of p). Each batch mixes
# all four periods (`groups` is sized for the largest one) and L1 from {p, 64, 64 + p, 136, 520}:
# nt < G, nt = G, nt = G + 1, several G.
#   bf16 L2: 64 192 448 -> p 1; 32 96 -> 2; 16 48 -> 4; 8 1000 -> 8
#   fp32 L2: 32 96 -> p 1; 16 48 -> 2; 8 1000 -> 4; 4 2052 -> 8
LINE_CASES = [
    {"name": "small", "hidden": 128, "sizes": {
        "bf16": [(1, 64), (2, 32), (4, 16), (8, 8), (64, 192), (66, 96), (68, 48), (72, 8)],
        "f32": [(1, 32), (2, 16), (4, 8), (8, 4), (64, 96), (66, 48), (68, 8), (72, 4)]}},
    {"name": "wide", "hidden": 8, "sizes": {
        "bf16": [(136, 448), (136, 96), (136, 48), (136, 1000), (520, 64), (520, 32), (520, 16), (520, 8),
                 (65, 192), (64, 1000), (8, 1000), (64, 32), (64, 48)],
        "f32": [(136, 96), (136, 48), (136, 1000), (136, 2052), (520, 32), (520, 16), (520, 8), (520, 4),
                (65, 32), (64, 2052), (8, 2052), (64, 48), (64, 8)]}},
]
LINE_L2 = {"bf16": {1: (64, 192, 448), 2: (32, 96), 4: (16, 48), 8: (8, 1000)},
           "f32": {1: (32, 96), 2: (16, 48), 4: (8, 1000), 8: (4, 2052)}}

# pair_rows_item (k_pair_rows, k_pair_stream, k_pair_help): nch 16-B chunks per row in segments of 128,
# `two = seg + 64 < nch`; k_pair_rows: 64 rows per wave, 64 * waves per block. "sizes" are (L1, nch),
# L2 = VEC * nch. Every batch is ragged in L1 (the shorter complexes leave empty row blocks); "edges"
# holds L1 = 64 w +- 1 for every waves-per-block w under test. "jobs" splits a batch into the three jobs
# of a queue run: the first job's items have at most 3 store instructions each (k_pair_stream must wait
# for its next ticket itself) and, with rblocks = 1, fewer items than a full launch has waves.
ROW_NCH = (1, 2, 63, 64, 65, 127, 128, 129, 193, 257)
ROW_WAVES = (1, 2, 4, 8, 16)
ROW_L1 = (1, 3, 4, 63, 64, 65, 127, 129) + tuple(64 * w + d for w in ROW_WAVES for d in (-1, 1))
ROW_CASES = [
    {"name": "h128", "hidden": 128,
     "sizes": [(1, 1), (3, 2), (4, 129), (63, 64), (65, 65), (64, 1), (2, 127), (1, 128)],
     "jobs": [[0, 1], [2, 3, 4], [5, 6, 7]]},
    {"name": "h24", "hidden": 24,
     "sizes": [(1, 63), (3, 64), (127, 128), (129, 129), (65, 127), (63, 193), (64, 257), (4, 65)],
     "jobs": [[0, 1], [2, 3, 4], [5, 6, 7]]},
    {"name": "edges", "hidden": 1,
     "sizes": [(3, 1), (1, 128), (255, 129), (257, 63), (511, 65), (513, 127), (1023, 128), (1025, 257), (127, 193),
               (129, 2), (63, 64), (1, 257)],
     "jobs": [[0, 1], [2, 3, 4, 5, 6], [7, 8, 9, 10, 11]]},
]


def row_sizes(case, dtype, idx=None):
    s = case["sizes"] if idx is None else [case["sizes"][i] for i in idx]
    return [(a, VEC[dtype] * n) for a, n in s]


def row_item_stores(l1, nch):
    """Store instructions of the largest item of a (L1, nch) complex: rows x pieces of every segment."""
    pieces = sum(2 if seg + 64 < nch else 1 for seg in range(0, nch, 128))
    return min(l1, 64) * pieces


# k_pair_flat: odd L2 (no 16-B vector anywhere), h2 rows off the vector (Layout h2_shift = 1), the
# output one element off a 16-B boundary (out_shift = 1), one plane of several PAIR_CHUNK (65536) items
FLAT_L2 = (1, 3, 7, 13, 31, 1001)
FLAT_CASES = [
    {"name": "odd", "hidden": 128, "sizes": [(7, 1), (20, 3), (33, 7), (5, 13), (64, 31), (1, 31), (65, 1)]},
    {"name": "chunks", "hidden": 3, "sizes": [(257, 1001), (3, 1001), (65, 13)]},
]
PAIR_CHUNK = 65536

# plane_rc's fp32-quotient row index at its documented limit, 2^20 rows (hidden = 1: two planes):
# (kernels, (L1, L2)); the last is the "large q" plane (flat positions far past 2^24), bf16 only, 1 GB,
# compared on the device
PAIR_MAX_PLANE_ROWS = 1 << 20
TALL_CASES = [
    (("rows", "vector"), (1 << 20, 8)),
    (("rows", "vector"), (1 << 20, 24)),
    (("flat",), (1 << 20, 3)),
    (("flat",), (1 << 20, 7)),
]
TALL_LARGE_Q = (("rows", "vector"), (262144, 1000))
