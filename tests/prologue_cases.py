"""Case tables, oracles and checkers of the fused head prologue (csrc/head_prologue.hip, di_head_prologue),
shared by tests/test_prologue_cases_host.py (CPU) and tests/test_gpu_prologue_cases.py (GPU). No tests
here; importable without a GPU (numpy; torch only for the fp32 matmul of the plain reference).

The oracle has two stages, so a failure names its kernel:

* Stage A (k_prologue_tables): the folded tables a', b' read back from the workspace against the float64
  evaluation of tests/test_head_prologue_math.py's formulas (``tables64``). The bar of a table of channel
  c is 4 * max(e32, 8 * 2^-24 * max|table_c|), e32 the worst error of the same formulas in plain fp32
  (torch matmul, two-pass variance) against float64: the reference's own fp32 behaviour, with a factor 4
  for another summation order (a premise the host file checks with the kernel's order). e^a', e^b'
  against exp of the device's own tables; the flag words by equality.
* Stage B (k_prologue_rows / k_prologue_flat): the whole output buffer, guard words included, against
  values computed from the DEVICE's tables. fp32: x > 0 bit for bit, x <= 0 within expm1f's margin.
  bf16: the RNE rounding of the host's med3(x, fma(ea, eb, -1), 0) (product path) or exact ELU (flagged
  channels, flat kernel), or the bf16 value across a rounding boundary the float64 value lies within
  2 * 2^-24 * max(1, |v|) of. The product path's value also stays within PROD_ABS of the float64 ELU.

``emulate_tables`` / ``emulate_stream`` restate the kernels' dataflow in numpy fp32 (with optional planted
defects); the host file runs them through the same checkers.
"""
import functools
import math

import numpy as np

f32, f64 = np.float32, np.float64
DTYPES = ("bf16", "f32")
VEC = {"bf16": 8, "f32": 4}
ESZ = {"bf16": 2, "f32": 4}
BITS = {"bf16": np.uint16, "f32": np.uint32}
# what output and workspace hold before a run: NaNs with a fixed payload. No ELU output is a NaN, and a
# NaN made by arithmetic carries the default payload (0x7FC0 / 0x7FC00000), not this one.
GUARD = {"bf16": 0x7FE5, "f32": 0x7FE5A3C1}
WORK_FILL = 0x7FD3B2A1            # workspace prefill and the guard behind di_head_prologue_work_bytes
WORK_GUARD = 1024                 # fp32 words behind the workspace
BAND = 4096                       # guard elements before the first and after the last complex
EPS = 1e-6                        # inorm_1.eps of the reference head
EXP_SAFE = 60.0                   # PRO_EXP_SAFE
PRO_SEG, PRO_TTHREADS, PRO_ROWS = 128, 512, 256

U = 2.0 ** -24                    # fp32 unit roundoff
FLOOR_ULPS = 8                    # bar floor: 8 * 2^-24 * max|table_c| (the issue's figure)
ORDER_FACTOR = 4                  # bar = 4 * max(e32, floor): another summation order (host premise)
# Relative accuracy granted to the device's expf and expm1f: 2 x the worst error measured on the MI355X
# over every value the cases produce: expf 8.15e-8 = 0.68 * 2^-23 over 2.3e5 table
# entries, expm1f 8.70e-8 = 0.73 * 2^-23 over 4.6e6 elements with x <= 0. ROCm's installed headers state
# no ulp figure for either; in ulps of the result the margins are at most 1.4 and 1.5 * 2 = 2.9.
EXPF_REL = 2 * 8.2e-8
EXPM1F_REL = 2 * 8.75e-8
# Product path, x <= 0: ea eb = e^x (1 + d1)(1 + d2), |d| <= EXPF_REL, e^x <= 1; the fma rounds once
# (2^-24); x = fl32(a' + b') moves e^x by |x| e^x 2^-24 <= 0.37 * 2^-24. For x > 0 med3 returns x unless
# the computed e^x - 1 fell below x, which takes e^x - 1 - x <= that error, so x < 2^-10 and e^x < 1.001.
PROD_ABS = (2 * EXPF_REL + 1.37 * U) * 1.001
NEIGHBOUR_WINDOW = 2 * U          # |v - boundary| <= 2 * 2^-24 * max(1, |v|)
NEIGHBOUR_SHARE = 0.01


# ---- number formats -----------------------------------------------------------------------------------
def bf16_rne(x):
    """float32 array -> bf16 bit patterns (uint16), round to nearest even."""
    u = np.ascontiguousarray(x, dtype=f32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_val(b):
    """bf16 bit patterns -> float32 values."""
    return (np.ascontiguousarray(b).astype(np.uint32) << 16).view(f32)


def round_to(x, dtype):
    """float array -> float32 values the dtype holds (bf16: RNE)."""
    x = np.asarray(x, dtype=f32)
    return bf16_val(bf16_rne(x)).reshape(x.shape) if dtype == "bf16" else x


def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding. The product of two fp32 is exact in float64; the sum is
    rounded to float64 (its error kept by TwoSum) and then to fp32; where the float64 sum sits exactly
    halfway between two fp32 and the kept error is not zero, the error decides."""
    a, b, c = (np.asarray(v, dtype=f32).astype(f64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        r = s.astype(f32)
        r64 = r.astype(f64)
        other = np.nextafter(r, np.where(s > r64, np.inf, -np.inf).astype(f32)).astype(f64)
        tie = np.isfinite(s) & (s != r64) & (np.abs(s - r64) == np.abs(other - s)) & (err != 0)
        move = tie & (np.sign(err) == np.sign(other - r64))
    return np.where(move, other, r64).astype(f32)


def med3(x, e, z):
    """The median of three (v_med3_f32 on numbers)."""
    return np.maximum(np.minimum(x, e), np.minimum(np.maximum(x, e), z))


def elu64(x):
    x = np.asarray(x, dtype=f64)
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))


# ---- cases --------------------------------------------------------------------------------------------
class Case:
    """One batch. sizes: (L1, n) with L2 = VEC * n ("rows": the row kernel's 16-B chunks; n = ("el", L2)
    gives L2 itself) or (L1, L2) as they are ("flat"). bias: the conv bias's size (None: 0.1 randn).
    gap: guard elements between complexes (a multiple of the vector for the row kernel, odd for the flat
    kernel). share: every complex reads the SAME node rows as complex 0."""

    def __init__(self, name, C, H, sizes, kernel="rows", seed=0, dtypes=DTYPES, w_scale=1.0, bias=None,
                 targets=None, small_x=False, share=False, out_shift=0):
        self.name, self.C, self.H, self.raw_sizes, self.kernel, self.seed = name, C, H, sizes, kernel, seed
        self.dtypes, self.w_scale, self.bias, self.targets, self.small_x = dtypes, w_scale, bias, targets, small_x
        self.share, self.out_shift = share, out_shift

    def sizes(self, dtype):
        if self.kernel != "rows":
            return list(self.raw_sizes)
        return [(a, n[1] if isinstance(n, tuple) else VEC[dtype] * n) for a, n in self.raw_sizes]

    def gap(self, dtype):
        return 3 * VEC[dtype] if self.kernel == "rows" else 7

    def __repr__(self):
        return self.name


# k_prologue_rows: nch 16-B chunks per row in segments of PRO_SEG = 128, `two = seg + 64 < nch`; a wave
# owns 64 rows, a work item 256. Every batch is ragged in both lengths (l1 < max_l1: the `r0 >= r1`
# skip; l2 < max_l2). "wrap": 40 * 5 * ceil(513 / 256) = 600 work items > the 512 blocks of the launch.
ROW_NCH = (1, 2, 63, 64, 65, 127, 128, 129, 193, 257)
ROW_L1 = (1, 63, 64, 65, 255, 256, 257, 513)
STREAM_CASES = [
    Case("s1", 2, 8, [(1, 1), (63, 2), (64, 63), (65, 64), (3, 65), (2, 127)], seed=1),
    Case("s2", 3, 8, [(255, 128), (5, 129), (256, 1), (4, 193), (257, 2), (2, 257)], seed=2),
    Case("s3", 1, 8, [(513, 1), (65, 257), (1, 193), (64, 129), (63, 65)], seed=3),
    Case("wrap", 5, 8, [(513, 1)] * 19 + [(257, 1), (1, 1)] + [(513, 1)] * 19, seed=4),
]
# k_prologue_tables: groups of PRO_CG = 4 channels, a second code path for nc = C % 4 in 1 .. 3; the
# weight rows of a group in LDS as wl[2 * hidden] (512 entries: full at hidden = 256). 515 rows and 520
# columns: the 512-thread loops over a chain take a second turn.
CHANNEL_C = (1, 2, 3, 5, 6, 7, 13)
CHANNEL_H = (8, 64, 128, 256)
CHANNEL_CASES = [Case(f"c{C}-h{H}", C, H, [(515, 1), (3, ("el", 520)), (70, 2)], seed=100 + 10 * C + H // 8)
                 for C in CHANNEL_C for H in CHANNEL_H]
# k_prologue_flat: odd L2 (never a vector), 1 x 1 (var = 0: a' = beta, b' = 0), L1 = 1 with L2 = one
# vector, the output one element off the vector; "grid": 5 * 459 * 459 = 1 053 405 > 4096 * 256 elements
# in one complex, so the flat grid's stride loop takes a second turn.
FLAT_L2 = (1, 3, 7, 13, 31, 1001)
FLAT_CASES = [
    Case("odd", 3, 8, [(1, 1), (7, 1), (20, 3), (33, 7), (5, 13), (64, 31), (3, 1001), (1, 8)], "flat", seed=5,
         out_shift=1),
    Case("grid", 5, 8, [(459, 459)], "flat", seed=6, dtypes=("bf16",), out_shift=1),
]
# statistics: chains of 2 and 3 (biased / unbiased variance differ by 2 and 1.5), var ~ eps (weights
# scaled until the conv's variance is about 1e-6), a conv bias 1e4 x the spread, unequal chains.
STAT_CASES = [
    Case("short", 5, 8, [(2, 3), (3, 2), (2, 2), (1, 2), (2, 1), (3, 3), (1, 3)], "flat", seed=7),
    Case("eps", 6, 16, [(37, 2), (9, 5)], seed=8, w_scale=4e-4),
    Case("bias", 5, 16, [(41, 3), (130, 1)], seed=9, bias=1e4),
    Case("chains", 3, 8, [(300, 1), (2, 40), (17, 3), (600, 2)], seed=10),
]
# the flag at |table| > 60: per-channel gamma from the float64 reference puts max|table| on the target,
# channels 0 .. 4 dominated by a', 5 .. 9 by b' (beta = 0, so a table scales with gamma). Groups of four:
# (30 59 | 61 80), (200 | 30 59 | 61), ragged (80 200). Complex 1 reads complex 0's rows (one gamma
# cannot put two different complexes on a target). "flagB" has the opposite flag in every channel.
FLAG_TARGETS = (30.0, 59.0, 61.0, 80.0, 200.0)
_OPPOSITE = {30.0: 200.0, 59.0: 61.0, 61.0: 59.0, 80.0: 30.0, 200.0: 30.0}
FLAG_CASES = [
    Case("flagA", 10, 8, [(70, 9), (70, 9)], seed=11, dtypes=("bf16",), targets=FLAG_TARGETS * 2, share=True),
    Case("flagB", 10, 8, [(70, 9), (70, 9)], seed=11, dtypes=("bf16",),
         targets=tuple(_OPPOSITE[t] for t in FLAG_TARGETS * 2), share=True),
]
# small |x| on the product path: in channel 0 every 16th (i, j) has 0 < |a'_i + b'_j| < 2^-12, both signs
# (Problem._small_x). Two ordinary channels beside it: a bf16 value this small lies within the neighbour
# window of a rounding boundary a quarter to half of the time (spacing 2^-20 .. 2^-21 against a window of
# 2^-22), so channel 0 alone would exceed the 1 % cap the case must keep.
SMALL_X = Case("smallx", 3, 8, [(256, ("el", 256))], seed=12, small_x=True)
SMALL_X_BOUND = 2.0 ** -12
SMALL_X_COUNT = 1000              # on each side of zero
# 32-bit row offsets: planes just under 2^31 bytes, C = 1, hidden = 8
TALL = {"bf16": (32768, 32760), "f32": (16384, 32764)}
TALL_REFUSED = {"bf16": (32768, 32768), "f32": (16384, 32768)}
TALL_ROWS = sorted(set(range(24)) | {r for m in range(256, 1025, 256) for r in (m - 1, m)})

SMALL_CASES = STREAM_CASES + CHANNEL_CASES + FLAT_CASES + STAT_CASES + FLAG_CASES + [SMALL_X]
BY_NAME = {c.name: c for c in SMALL_CASES}


# ---- the float64 reference and its fp32 restatements ------------------------------------------------
def tables64(h1, h2, w, b, gamma, beta, eps):
    """a' [C, L1], b' [C, L2] in float64: test_head_prologue_math.fused_prologue's formulas up to the sum."""
    h1, h2, w, b, gamma, beta = (np.asarray(v, dtype=f64) for v in (h1, h2, w, b, gamma, beta))
    H = h1.shape[1]
    A = h1 @ w[:, :H].T
    B = h2 @ w[:, H:].T + b
    ma, mb = A.mean(0), B.mean(0)
    var = ((A - ma) ** 2).mean(0) + ((B - mb) ** 2).mean(0)
    s = gamma / np.sqrt(var + eps)
    return (s * (A - ma) + beta).T.copy(), (s * (B - mb)).T.copy()


def tables32_plain(h1, h2, w, b, gamma, beta, eps):
    """The same formulas in plain fp32: torch's matmul, numpy's fp32 mean, two-pass variance."""
    import torch
    H = h1.shape[1]
    mm = lambda x, y: torch.from_numpy(np.ascontiguousarray(x)).matmul(torch.from_numpy(np.ascontiguousarray(y)).t()).numpy()  # noqa: E731
    A = mm(h1, w[:, :H])
    B = mm(h2, w[:, H:]) + b
    ma, mb = A.mean(0, dtype=f32), B.mean(0, dtype=f32)
    var = ((A - ma) ** 2).mean(0, dtype=f32) + ((B - mb) ** 2).mean(0, dtype=f32)
    s = gamma / np.sqrt(var + f32(eps))
    return (s * (A - ma) + beta).T.copy(), (s * (B - mb)).T.copy()


def _block_sum(v):
    """k_prologue_tables' sum of one value per row over a 512-thread block, fp32: thread t adds rows t,
    t + 512, ... in order; a butterfly over each wave's 64 lanes; the 8 wave sums in order. v: [n, C]."""
    n, C = v.shape
    pad = -n % PRO_TTHREADS
    t = np.concatenate([v, np.zeros((pad, C), f32)]).reshape(-1, PRO_TTHREADS, C)
    acc = np.zeros((PRO_TTHREADS, C), f32)
    for m in range(t.shape[0]):
        acc = acc + t[m]
    acc = acc.reshape(8, 64, C)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ o]
    tot = np.zeros(C, f32)
    for wv in range(8):
        tot = tot + acc[wv, 0]
    return tot


def _dots(h, w):
    """A sequential fp32 fma chain in k order (pro_dots): [n, H] x [C, H] -> [n, C]."""
    acc = np.zeros((h.shape[0], w.shape[0]), f32)
    for k in range(h.shape[1]):
        acc = fma32(w[None, :, k], h[:, k, None], acc)
    return acc


TABLE_DEFECTS = ("unbiased", "eps_outside", "max_l1", "beta_b", "bias_both")
STREAM_DEFECTS = ("two_one", "seg_stop", "prod_flagged", "no_med3")


def tables32_kernel(h1, h2, w, b, gamma, beta, eps, max_l1=None, defect=None):
    """k_prologue_tables' dataflow in numpy fp32: fma chains in k order, block sums, two-pass variance.
    defect: one of TABLE_DEFECTS, the one-token slips the host file plants."""
    H = h1.shape[1]
    l1, l2 = h1.shape[0], h2.shape[0]
    A = _dots(h1, w[:, :H]) + (b if defect == "bias_both" else f32(0))
    B = _dots(h2, w[:, H:]) + b
    ma = _block_sum(A) / f32(max_l1 if defect == "max_l1" else l1)
    mb = _block_sum(B) / f32(l2)
    ta, tb = A - ma, B - mb
    d1, d2 = (max(l1 - 1, 1), max(l2 - 1, 1)) if defect == "unbiased" else (l1, l2)
    var = _block_sum(ta * ta) / f32(d1) + _block_sum(tb * tb) / f32(d2)
    s = gamma / (np.sqrt(var) + f32(eps)) if defect == "eps_outside" else gamma / np.sqrt(var + f32(eps))
    a = s * ta + beta
    bb = s * tb + (beta if defect == "beta_b" else f32(0))
    return a.T.astype(f32), bb.T.astype(f32)


class Problem:
    """Inputs, layout, float64 reference and bars of one (case, dtype)."""

    def __init__(self, case, dtype, gap=None):
        self.case, self.dtype, self.C, self.H, self.kernel = case, dtype, case.C, case.H, case.kernel
        self.sizes = case.sizes(dtype)
        C, H = case.C, case.H
        rng = np.random.default_rng(case.seed)
        self.w = (rng.normal(size=(C, 2 * H)) / math.sqrt(2 * H) * case.w_scale).astype(f32)
        self.b = (rng.normal(size=C) * 0.1 if case.bias is None else case.bias * (1 + 0.1 * rng.normal(size=C))).astype(f32)
        self.gamma = (1 + 0.2 * rng.normal(size=C)).astype(f32)
        self.beta = (0.2 * rng.normal(size=C)).astype(f32)
        self.eps = EPS
        # rows: chain 1, then chain 2, complex after complex (every row starts on a 16-B vector)
        self.h1r, self.h2r, r = [], [], 0
        for n, (a, b2) in enumerate(self.sizes):
            if case.share and n > 0:
                self.h1r.append(self.h1r[0]), self.h2r.append(self.h2r[0])
                continue
            self.h1r.append(r), self.h2r.append(r + a)
            r += a + b2
        self.rows = r
        self.h = round_to(rng.normal(size=(r, H)) * 2, dtype)
        if case.small_x:
            self._small_x(rng)
        if case.targets:
            self._targets()
        # output: band, complexes with gaps, band; base `out_shift` elements into the allocation
        gap = case.gap(dtype) if gap is None else gap
        self.offs, off = [], BAND
        for a, b2 in self.sizes:
            self.offs.append(off)
            off += C * a * b2 + gap
        self.total = off - gap + BAND
        self.out_shift = case.out_shift
        self.descs = [(r1, r2, o, a, b2) for r1, r2, o, (a, b2) in zip(self.h1r, self.h2r, self.offs, self.sizes)]
        self.m1, self.m2 = max(a for a, _ in self.sizes), max(b2 for _, b2 in self.sizes)
        self.aligned = int(self.kernel == "rows")
        if self.aligned:
            v = VEC[dtype]
            assert self.out_shift == 0 and all(b2 % v == 0 for _, b2 in self.sizes) and all(o % v == 0 for o in self.offs)
        # reference, plain-fp32 error, bars
        self.ref, self.bar_a, self.bar_b, self.big, self.flag = [], [], [], [], []
        for n in range(len(self.sizes)):
            h1, h2 = self.chains(n)
            a64, b64 = tables64(h1, h2, self.w, self.b, self.gamma, self.beta, self.eps)
            a32, b32 = tables32_plain(h1, h2, self.w, self.b, self.gamma, self.beta, self.eps)
            big = np.maximum(np.abs(a64).max(1), np.abs(b64).max(1))
            floor = FLOOR_ULPS * U * big
            self.ref.append((a64, b64))
            self.bar_a.append(ORDER_FACTOR * np.maximum(np.abs(a32 - a64).max(1), floor))
            self.bar_b.append(ORDER_FACTOR * np.maximum(np.abs(b32 - b64).max(1), floor))
            self.big.append(big)
            self.flag.append(big > EXP_SAFE)

    def chains(self, n):
        a, b2 = self.sizes[n]
        return self.h[self.h1r[n]:self.h1r[n] + a], self.h[self.h2r[n]:self.h2r[n] + b2]

    def in_window(self, n):
        """Channels whose float64 max|table| is within a Stage-A bar of the flag's threshold."""
        return np.abs(self.big[n] - EXP_SAFE) <= np.maximum(self.bar_a[n], self.bar_b[n])

    def _small_x(self, rng):
        """SMALL_X's rows: s (v, t) with v one of 8 base vectors, t in [2^-14, 2^-13] in feature 0 and the
        sign s = +-1 in antisymmetric pairs; channel 0 weighs v with opposite signs on the two chains and t
        with 1 on both, and has beta = 0: where both chains drew the same s v, x = scale * s (t_i + t_j)."""
        H, (l1, l2) = self.H, self.sizes[0]
        base = round_to(rng.normal(size=(8, H)), self.dtype)
        base[:, 0] = 0
        for start, length in ((0, l1), (l1, l2)):
            for m in range(length // 2):
                row = base[rng.integers(8)].copy()
                row[0] = round_to(np.array([rng.uniform(2.0 ** -14, 2.0 ** -13)]), self.dtype)[0]
                sign = rng.choice([-1, 1])
                self.h[start + 2 * m], self.h[start + 2 * m + 1] = sign * row, -sign * row
        self.w[0, H:] = -self.w[0, :H]
        self.w[0, 0] = self.w[0, H] = 1.0
        self.beta[0] = 0
        self.gamma[0] = 0.45       # scale = gamma / sqrt(var) is about 0.95: |x| in 0.95 * [2^-13, 2^-12]

    def _targets(self):
        """FLAG_CASES' gamma: channels 0 .. C/2 - 1 dominated by a' (chain-1 weights x 1.25, chain-2 / 1.25: the
        other table still reaches about two thirds of the target, so at 200 e^a' e^b' meets inf * 0), the others by b'; beta = 0; gamma_c = target_c / max|table_c| of the float64 reference at gamma = 1."""
        C, H = self.C, self.H
        self.w[:C // 2, :H] *= 1.25
        self.w[:C // 2, H:] /= 1.25
        self.w[C // 2:, :H] /= 1.25
        self.w[C // 2:, H:] *= 1.25
        self.beta[:] = 0
        a, b2 = self.sizes[0]
        h1, h2 = self.h[self.h1r[0]:self.h1r[0] + a], self.h[self.h2r[0]:self.h2r[0] + b2]
        for _ in range(20):        # a channel whose draw still favours the other table: once more
            a64, b64 = tables64(h1, h2, self.w, self.b, np.ones(C), self.beta, self.eps)
            ma, mb = np.abs(a64).max(1), np.abs(b64).max(1)
            wrong = np.where(np.arange(C) < C // 2, ma <= 1.02 * mb, mb <= 1.02 * ma)
            if not wrong.any():
                break
            for c in np.flatnonzero(wrong):
                lo, hi = (slice(H, None), slice(0, H)) if c < C // 2 else (slice(0, H), slice(H, None))
                self.w[c, hi] *= 1.25
                self.w[c, lo] /= 1.25
        big = np.maximum(ma, mb)
        self.gamma = (np.array(self.case.targets) / big).astype(f32)

    # -- layout of the workspace (pro_table_stride, di_head_prologue_work_bytes) --
    @property
    def stride(self):
        return 2 * (self.m1 + self.m2)

    @property
    def work_words(self):
        return len(self.sizes) * self.C * (self.stride + 1)

    def locate(self, idx):
        for n, (_, _, off, l1, l2) in enumerate(self.descs):
            if off <= idx < off + self.C * l1 * l2:
                c, rest = divmod(idx - off, l1 * l2)
                return f"complex {n} ({l1} x {l2}), channel {c}, row {rest // l2}, column {rest % l2}"
        return "guard"


@functools.lru_cache(maxsize=None)
def problem(name, dtype, gap=None):
    """The Problem of a named case, made once and shared (gap = 0: the layout HeadPrologueOp builds)."""
    return Problem(BY_NAME[name], dtype, gap)


def read_work(work, prob):
    """The workspace (fp32 words, at least prob.work_words of them) as per-complex tables
    [(a' [C, l1], b' [C, l2], e^a', e^b')] and the flag words [complexes, C] (int32)."""
    C, st, m1, m2 = prob.C, prob.stride, prob.m1, prob.m2
    ncpx = len(prob.sizes)
    t = work[:ncpx * C * st].reshape(ncpx, C, st)
    tabs = [(t[n, :, :l1], t[n, :, m1:m1 + l2], t[n, :, m1 + m2:m1 + m2 + l1], t[n, :, 2 * m1 + m2:2 * m1 + m2 + l2])
            for n, (l1, l2) in enumerate(prob.sizes)]
    flags = work[ncpx * C * st:ncpx * C * (st + 1)].view(np.int32).reshape(ncpx, C)
    return tabs, flags


# ---- the checkers ---------------------------------------------------------------------------------------
class Report:
    """Failures (messages) and the figures a check measured."""

    def __init__(self):
        self.failures, self.figures = [], {}

    def fail(self, msg):
        if len(self.failures) < 8:
            self.failures.append(msg)

    def peak(self, key, value):
        value = float(value)
        if value == value:
            self.figures[key] = max(self.figures.get(key, 0.0), value)

    @property
    def ok(self):
        return not self.failures

    def __str__(self):
        return "; ".join(self.failures) or "ok"


def _ratio(err, bar):
    """err / bar per channel, with 0 / 0 = 0 and x / 0 = inf."""
    with np.errstate(all="ignore"):
        return np.where(err == 0, 0.0, np.where(bar > 0, err / np.where(bar > 0, bar, 1), np.inf))


def _exp_check(rep, what, e_dev, t_dev):
    """e_dev = expf(t_dev) within EXPF_REL where exp is a normal fp32; past the format's ends: inf (or the
    largest values) above, at most 2^-125 below."""
    want = np.exp(t_dev.astype(f64))
    e = e_dev.astype(f64)
    normal = (want >= 2.0 ** -126) & (want <= 3.4028234e38)
    with np.errstate(all="ignore"):
        rel = np.abs(e - want) / want
    if normal.any():
        rep.peak("expf_rel", rel[normal].max())
    bad = (normal & ~(rel <= EXPF_REL)) | ((want > 3.4028234e38) & ~(e >= 3.4028234e38 * (1 - EXPF_REL))) | \
        ((want < 2.0 ** -126) & ~((e >= 0) & (e <= 2.0 ** -125)))
    if bad.any():
        c, i = np.argwhere(bad)[0]
        rep.fail(f"{what}, channel {c}, entry {i}: expf({t_dev[c, i]!r}) gave {e_dev[c, i]!r}, exp is {want[c, i]!r}")


def check_tables(prob, tabs, flags):
    """Stage A on the workspace's tables and flag words."""
    rep = Report()
    for n, (a, b2, ea, eb) in enumerate(tabs):
        a64, b64 = prob.ref[n]
        for name, got, ref, bar in (("a'", a, a64, prob.bar_a[n]), ("b'", b2, b64, prob.bar_b[n])):
            err = np.abs(got.astype(f64) - ref)
            err[~np.isfinite(err)] = np.inf
            ratio = _ratio(err.max(1), bar)
            rep.peak("table_ratio", ratio.max())
            for c in np.flatnonzero(~(ratio <= 1)):
                i = int(err[c].argmax())
                rep.fail(f"complex {n} {prob.sizes[n]}, channel {c}, {name}[{i}]: got {got[c, i]!r}, float64 "
                         f"{ref[c, i]!r}, error {err[c, i]:.3e} = {ratio[c]:.2f} x the bar {bar[c]:.3e}")
        _exp_check(rep, f"complex {n}, e^a'", ea, a)
        _exp_check(rep, f"complex {n}, e^b'", eb, b2)
        for c in range(prob.C):
            if flags[n, c] not in (0, 1):
                rep.fail(f"complex {n}, channel {c}: flag word {int(flags[n, c]):#x}")
            elif not prob.in_window(n)[c] and bool(flags[n, c]) != bool(prob.flag[n][c]):
                rep.fail(f"complex {n}, channel {c}: flag {int(flags[n, c])}, max|table| {prob.big[n][c]:.6g}")
    return rep


def _bf16_ok(y, hv, v64, rep):
    """bf16 words y against the host's fp32 value hv: its RNE rounding (zeros of either sign equal), or
    the adjacent bf16 value where the float64 value v64 is within the window of the boundary between the
    two. Returns the elementwise verdict; counts the allowance's uses."""
    hb = bf16_rne(hv)
    same = (y == hb) | (((y | hb) & 0x7FFF) == 0)
    if same.all():
        return same
    yv, hbv = bf16_val(y).astype(f64), bf16_val(hb).astype(f64)
    key = lambda b: np.where(b & 0x8000, -(b & 0x7FFF).astype(np.int32), (b & 0x7FFF).astype(np.int32))  # noqa: E731
    adjacent = np.abs(key(y) - key(hb)) == 1
    with np.errstate(all="ignore"):
        near = np.abs(v64 - (yv + hbv) / 2) <= NEIGHBOUR_WINDOW * np.maximum(1, np.abs(v64))
    used = ~same & adjacent & near & ((y & 0x7F80) != 0x7F80)
    rep.figures["neighbour_used"] = rep.figures.get("neighbour_used", 0) + int(used.sum())
    return same | used


def check_stream(prob, tabs, flags, got, kernel=None):
    """Stage B: the WHOLE output buffer `got` (bit patterns, prob.total elements from the layout's base)
    against values computed from the tables `tabs` / `flags` (the device's own)."""
    rep, dtype, C = Report(), prob.dtype, prob.C
    kernel = kernel or prob.kernel
    assert got.dtype == BITS[dtype] and got.shape == (prob.total,), (got.dtype, got.shape, prob.total)
    outside = np.ones(prob.total, dtype=bool)
    for _, _, off, l1, l2 in prob.descs:
        outside[off:off + C * l1 * l2] = False
    bad = np.flatnonzero(outside & (got != GUARD[dtype]))
    if bad.size:
        rep.fail(f"guard: {bad.size} words written outside every complex, first at flat index {int(bad[0])}")
    elements = 0
    for n, (_, _, off, l1, l2) in enumerate(prob.descs):
        a, b2, ea, eb = tabs[n]
        blk = got[off:off + C * l1 * l2].reshape(C, l1, l2)
        for c in range(C):
            x = a[c][:, None] + b2[c][None, :]            # fl32(a' + b'), one IEEE add
            x64 = x.astype(f64)
            v64 = elu64(x64)
            y = blk[c]
            elements += y.size
            if dtype == "f32":
                yv = y.view(f32).astype(f64)
                pos = x > 0
                err = np.abs(yv - v64)
                with np.errstate(all="ignore"):
                    rel = err / np.abs(v64)
                m = ~pos & (np.abs(v64) >= 2.0 ** -126)
                if m.any():
                    rep.peak("expm1f_rel", rel[m].max() if np.isfinite(rel[m]).all() else np.inf)
                ok = np.where(pos, y == x.view(np.uint32), err <= EXPM1F_REL * np.abs(v64) + 2.0 ** -149)
            else:
                if kernel == "rows" and flags[n, c] == 0:
                    hv = med3(x, fma32(ea[c][:, None], eb[c][None, :], f32(-1)), f32(0))
                    perr = np.abs(hv.astype(f64) - v64)
                    perr[~np.isfinite(perr)] = np.inf
                    rep.peak("prod_abs", perr.max())
                    ok = _bf16_ok(y, hv, v64, rep) & (perr <= PROD_ABS)
                else:
                    ok = _bf16_ok(y, v64.astype(f32), v64, rep)
            if not ok.all():
                i, j = np.argwhere(~ok)[0]
                what = "guard word left" if y[i, j] == GUARD[dtype] else f"got {int(y[i, j]):#x}"
                rep.fail(f"complex {n} ({l1} x {l2}), channel {c}, row {i}, column {j}: {what}, x = {x[i, j]!r}, "
                         f"float64 ELU {v64[i, j]!r}" + (f", flag {int(flags[n, c])}" if dtype == "bf16" else ""))
    share = rep.figures.get("neighbour_used", 0) / max(elements, 1)
    rep.figures["neighbour_share"] = share
    if share > NEIGHBOUR_SHARE:
        rep.fail(f"{share:.2%} of the elements used the neighbour allowance (cap {NEIGHBOUR_SHARE:.0%})")
    return rep


def check_composite(prob, got):
    """Through HeadPrologueOp (its own workspace: no device tables to read): every element of the WHOLE
    buffer against the float64 ELU(a' + b') within bar_a'[c] + bar_b'[c] (ELU is 1-Lipschitz) plus Stage
    B's term on the float64 value: fl32's rounding of x, then expm1f's margin (fp32) or the product
    path's absolute bound and half a bf16 ulp, 2^-8 relative (bf16)."""
    rep, dtype, C = Report(), prob.dtype, prob.C
    assert got.dtype == BITS[dtype] and got.shape == (prob.total,), (got.dtype, got.shape, prob.total)
    outside = np.ones(prob.total, dtype=bool)
    for _, _, off, l1, l2 in prob.descs:
        outside[off:off + C * l1 * l2] = False
    bad = np.flatnonzero(outside & (got != GUARD[dtype]))
    if bad.size:
        rep.fail(f"guard: {bad.size} words written outside every complex, first at flat index {int(bad[0])}")
    for n, (_, _, off, l1, l2) in enumerate(prob.descs):
        a64, b64 = prob.ref[n]
        blk = got[off:off + C * l1 * l2].reshape(C, l1, l2)
        for c in range(C):
            x64 = a64[c][:, None] + b64[c][None, :]
            v64 = elu64(x64)
            tol = prob.bar_a[n][c] + prob.bar_b[n][c] + U * np.abs(x64)
            if dtype == "f32":
                yv = blk[c].view(f32).astype(f64)
                tol = tol + EXPM1F_REL * np.abs(v64) + 2.0 ** -149
            else:
                yv = bf16_val(blk[c]).astype(f64)
                tol = tol + PROD_ABS
                tol = tol + 2.0 ** -8 * (np.abs(v64) + tol) + 2.0 ** -134
            err = np.abs(yv - v64)
            with np.errstate(all="ignore"):
                rep.peak("composite_ratio", np.where(np.isfinite(err), err / tol, np.inf).max())
            ok = err <= tol
            if not ok.all():
                i, j = np.argwhere(~ok)[0]
                rep.fail(f"complex {n} ({l1} x {l2}), channel {c}, row {i}, column {j}: got {yv[i, j]!r}, float64 ELU "
                         f"{v64[i, j]!r}, bar {tol[i, j]:.3e}")
    return rep


def boundary_share(prob):
    """Host premise: the share of float64 reference values within the neighbour window of a bf16 rounding
    boundary (the elements that MAY use the neighbour allowance)."""
    near = total = 0
    for n, (a64, b64) in enumerate(prob.ref):
        for c in range(prob.C):
            v = elu64(a64[c][:, None] + b64[c][None, :])
            lo = (v.astype(f32).view(np.uint32) & 0xFFFF0000).view(f32).astype(f64)     # toward zero
            ulp = 2.0 ** np.floor(np.log2(np.maximum(np.abs(lo), 2.0 ** -126))) * 2.0 ** -7
            mid = lo + np.sign(v) * ulp / 2
            near += int((np.abs(v - mid) <= NEIGHBOUR_WINDOW * np.maximum(1, np.abs(v))).sum())
            total += v.size
    return near / total


# ---- the kernels' dataflow in numpy fp32 ----------------------------------------------------------------
def emulate_tables(prob, defect=None):
    """A workspace (fp32 words) as k_prologue_tables fills it; unwritten words keep WORK_FILL."""
    work = np.full(prob.work_words + WORK_GUARD, WORK_FILL, dtype=np.uint32).view(f32)
    tabs, flags = read_work(work, prob)
    for n in range(len(prob.sizes)):
        h1, h2 = prob.chains(n)
        a, b2 = tables32_kernel(h1, h2, prob.w, prob.b, prob.gamma, prob.beta, prob.eps, prob.m1, defect)
        with np.errstate(all="ignore"):
            tabs[n][0][:], tabs[n][1][:] = a, b2
            tabs[n][2][:], tabs[n][3][:] = np.exp(a.astype(f64)).astype(f32), np.exp(b2.astype(f64)).astype(f32)
        flags[n] = np.maximum(np.abs(a).max(1), np.abs(b2).max(1)) > f32(EXP_SAFE)
    return work


def emulate_stream(prob, work, kernel=None, defect=None):
    """The output buffer (bit patterns) as k_prologue_rows / k_prologue_flat fill it from `work`: the
    guard word everywhere else, the row kernel's chunk walk (segments of 128, `two`) restated."""
    dtype, C, vec = prob.dtype, prob.C, VEC[prob.dtype]
    kernel = kernel or prob.kernel
    tabs, flags = read_work(work, prob)
    out = np.full(prob.total, GUARD[dtype], dtype=BITS[dtype])
    for n, (_, _, off, l1, l2) in enumerate(prob.descs):
        a, b2, ea, eb = tabs[n]
        cols = np.ones(l2, dtype=bool)
        if kernel == "rows":
            nch, chunk = l2 // vec, np.zeros(l2 // vec, dtype=bool)
            for seg in range(0, nch, PRO_SEG):
                chunk[seg:min(seg + 64, nch)] = True
                if seg + (65 if defect == "two_one" else 64) < nch:
                    chunk[seg + 64:min(seg + 128, nch)] = True
                if defect == "seg_stop":
                    break
            cols = np.repeat(chunk, vec)
        blk = out[off:off + C * l1 * l2].reshape(C, l1, l2)
        for c in range(C):
            x = a[c][:, None] + b2[c][None, :]
            with np.errstate(all="ignore"):
                exact = np.where(x > 0, x, np.expm1(np.minimum(x, 0).astype(f64)).astype(f32))
                if dtype == "bf16" and kernel == "rows" and (flags[n, c] == 0 or defect == "prod_flagged"):
                    e = fma32(ea[c][:, None], eb[c][None, :], f32(-1))
                    y = np.where(x > 0, e, med3(x, e, f32(0))) if defect == "no_med3" else med3(x, e, f32(0))
                else:
                    y = exact
            bits = bf16_rne(y) if dtype == "bf16" else y.astype(f32).view(np.uint32)
            blk[c][:, cols] = bits.reshape(l1, l2)[:, cols]
    return out
