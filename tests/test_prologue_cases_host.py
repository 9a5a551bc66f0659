"""CPU premises of tests/prologue_cases.py (the oracle of tests/test_gpu_prologue_cases.py): the float64
restatement against the materialised-T oracle, the 4x summation-order premise of the Stage-A bar, the
neighbour-share cap, the FLAG_CASES margins, the SMALL_X count, the case tables' coverage, a numpy fp32
emulation of the kernels' dataflow through the same checkers, and the planted defects each checker must
catch by at least 2x its bar."""
import numpy as np
import pytest
import torch

import prologue_cases as P
from test_head_prologue_math import fused_prologue

ALL = [pytest.param(c.name, dt, id=f"{c.name}-{dt}") for c in P.SMALL_CASES for dt in c.dtypes]


def _materialised(prob, n):
    from oracle import geot_oracle as O
    h1, h2 = prob.chains(n)
    C, H = prob.C, prob.H
    sd = {"interact_module.conv2d_1.weight": torch.tensor(prob.w.astype(np.float64)).reshape(C, 2 * H, 1, 1),
          "interact_module.conv2d_1.bias": torch.tensor(prob.b.astype(np.float64)),
          "interact_module.inorm_1.weight": torch.tensor(prob.gamma.astype(np.float64)),
          "interact_module.inorm_1.bias": torch.tensor(prob.beta.astype(np.float64))}
    with torch.no_grad():
        return O.head_prologue(sd, O.pair_tensor(torch.tensor(h1.astype(np.float64)), torch.tensor(h2.astype(np.float64))))[0].numpy()


@pytest.mark.parametrize("name", ["s1", "odd", "short", "eps", "chains", "c3-h8", "c13-h256"])
def test_float64_restatement_equals_the_materialised_oracle(name):
    """tables64 is fused_prologue's formulas (the same bits after the sum and the ELU), and
    fused_prologue equals ELU(inorm_1(conv2d_1(T))) on the materialised T at 1e-10 of the channel's
    scale, on the degenerate shapes too: 1 x 1 (var = 0), chains of 1, 2 and 3, var ~ eps."""
    from oracle import geot_oracle as O
    assert O.IN_EPS == P.EPS
    prob = P.problem(name, "f32")
    for n, (l1, l2) in enumerate(prob.sizes):
        if l1 * l2 > 40000:
            continue
        h1, h2 = (v.astype(np.float64) for v in prob.chains(n))
        args = [v.astype(np.float64) for v in (prob.w, prob.b, prob.gamma, prob.beta)]
        fused = fused_prologue(h1, h2, *args, prob.eps)
        a64, b64 = prob.ref[n]
        assert np.array_equal(P.elu64(a64[:, :, None] + b64[:, None, :]), fused)
        if l1 * l2 == 1:    # torch's instance_norm refuses a single element; the formulas give ELU(beta)
            continue
        np.testing.assert_allclose(fused, _materialised(prob, n), rtol=0, atol=1e-10 * max(1.0, prob.big[n].max()))
    if name == "odd":       # 1 x 1: var = 0, a' = beta, b' = 0
        assert prob.sizes[0] == (1, 1)
        assert np.array_equal(prob.ref[0][0][:, 0], prob.beta.astype(np.float64)) and not prob.ref[0][1].any()


def test_case_tables_reach_every_branch():
    for dt in P.DTYPES:
        sizes = [s for c in P.STREAM_CASES for s in c.sizes(dt)]
        assert {b // P.VEC[dt] for _, b in sizes} >= set(P.ROW_NCH) and {a for a, _ in sizes} >= set(P.ROW_L1)
        for c in P.STREAM_CASES:
            s = c.sizes(dt)
            assert min(a for a, _ in s) < max(a for a, _ in s) and c.gap(dt) % P.VEC[dt] == 0
        wrap = P.problem("wrap", dt)
        assert len(wrap.sizes) * wrap.C * -(-wrap.m1 // P.PRO_ROWS) > 512
    assert {c.C % 4 for c in P.CHANNEL_CASES} == {1, 2, 3} and {c.C for c in P.CHANNEL_CASES} == set(P.CHANNEL_C)
    assert {c.H for c in P.CHANNEL_CASES} == set(P.CHANNEL_H) and len(P.CHANNEL_CASES) == 28
    flat = [s for c in P.FLAT_CASES for s in c.sizes("bf16")]
    assert {b for _, b in flat} >= set(P.FLAT_L2) and (1, 1) in flat and (1, 8) in flat
    assert all(b % 2 == 1 or a == 1 for a, b in flat) and all(c.gap("bf16") % 2 == 1 for c in P.FLAT_CASES)
    assert 5 * 459 * 459 > 4096 * 256
    for dt, (a, b) in P.TALL.items():
        assert a * b * P.ESZ[dt] < 2 ** 31 <= P.TALL_REFUSED[dt][0] * P.TALL_REFUSED[dt][1] * P.ESZ[dt]
        assert (a - 1) * b * P.ESZ[dt] + b * P.ESZ[dt] < 2 ** 31 and b % P.VEC[dt] == 0
    assert P.TALL["bf16"][0] * P.TALL["bf16"][1] == 1073479680 and P.TALL["f32"][0] * P.TALL["f32"][1] == 536805376


def test_stat_cases_are_what_they_claim():
    eps = P.problem("eps", "f32")
    for n in range(len(eps.sizes)):        # var_c within [eps / 4, 4 eps]: gamma / s = sqrt(var + eps)
        h1, h2 = (v.astype(np.float64) for v in eps.chains(n))
        w, H = eps.w.astype(np.float64), eps.H
        var = (h1 @ w[:, :H].T).var(0) + (h2 @ w[:, H:].T).var(0)
        assert ((var > P.EPS / 4) & (var < 4 * P.EPS)).all(), var
    bias = P.problem("bias", "f32")
    h1, h2 = (v.astype(np.float64) for v in bias.chains(0))
    spread = (h2 @ bias.w.astype(np.float64)[:, bias.H:].T).std(0)
    assert (np.abs(bias.b) > 3e3 * spread).all() and (np.abs(bias.b) < 3e4 * spread).all()
    assert {a for a, _ in P.problem("short", "f32").sizes} == {1, 2, 3}


@pytest.mark.parametrize("name,dtype", ALL)
def test_two_fp32_orders_stay_within_the_factor(name, dtype):
    """The bar is 4 x max(plain fp32's error, the floor). Premise, asserted in every channel of every
    complex: the kernel's order (a sequential fma chain in k order, block sums) stays within the bar made
    from torch's matmul. The converse (torch's matmul within 4 x max(the kernel order's error, the floor))
    is printed: no bar rests on it, and it misses in one channel (eps-bf16, complex 1, channel 3: 4.34)."""
    prob = P.problem(name, dtype)
    for n in range(len(prob.sizes)):
        h1, h2 = prob.chains(n)
        a64, b64 = prob.ref[n]
        ak, bk = P.tables32_kernel(h1, h2, prob.w, prob.b, prob.gamma, prob.beta, prob.eps)
        ap, bp = P.tables32_plain(h1, h2, prob.w, prob.b, prob.gamma, prob.beta, prob.eps)
        floor = P.FLOOR_ULPS * P.U * prob.big[n]
        for got, other, ref, bar in ((ak, ap, a64, prob.bar_a[n]), (bk, bp, b64, prob.bar_b[n])):
            ek, ep = np.abs(got - ref).max(1), np.abs(other - ref).max(1)
            assert (ek <= bar).all(), (n, ek / bar)
            conv = ep / np.maximum(ek, floor)
            if (conv > P.ORDER_FACTOR).any():
                print(f"{name} {dtype} complex {n}: converse factor {conv.max():.2f} in channel {int(conv.argmax())}")


@pytest.mark.parametrize("name,dtype", ALL)
def test_no_channel_sits_in_the_flag_window(name, dtype):
    prob = P.problem(name, dtype)
    for n in range(len(prob.sizes)):
        assert not prob.in_window(n).any(), (n, prob.big[n])


def test_flag_cases_land_on_their_targets():
    for case in P.FLAG_CASES:
        prob = P.problem(case.name, "bf16")
        for n in range(len(prob.sizes)):
            a64, b64 = prob.ref[n]
            ma, mb = np.abs(a64).max(1), np.abs(b64).max(1)
            np.testing.assert_allclose(prob.big[n], case.targets, rtol=1e-6)
            assert (ma[:5] > mb[:5]).all() and (mb[5:] > ma[5:]).all()
            # the margin to 60 is thousands of bars wide
            assert (np.abs(prob.big[n] - P.EXP_SAFE) > 1e3 * np.maximum(prob.bar_a[n], prob.bar_b[n])).all()
        flags = prob.flag[0]
        for g in (flags[0:4], flags[4:8]):
            assert g.any() and not g.all()          # flagged and unflagged channels in one group of four
    assert (P.problem("flagA", "bf16").flag[0] != P.problem("flagB", "bf16").flag[0]).all()


@pytest.mark.parametrize("dtype", P.DTYPES)
def test_small_x_count(dtype):
    prob = P.problem("smallx", dtype)
    a64, b64 = prob.ref[0]
    x = a64[0][:, None] + b64[0][None, :]
    pos, neg = int(((x > 0) & (x < P.SMALL_X_BOUND)).sum()), int(((x < 0) & (x > -P.SMALL_X_BOUND)).sum())
    print(f"SMALL_X {dtype}: {pos} elements in (0, 2^-12), {neg} in (-2^-12, 0)")
    assert pos >= P.SMALL_X_COUNT and neg >= P.SMALL_X_COUNT
    assert not prob.flag[0][0]


@pytest.mark.parametrize("name", [c.name for c in P.SMALL_CASES if c.name not in ("grid", "wrap") and c not in P.CHANNEL_CASES]
                         + ["c13-h8", "c5-h256"])
def test_neighbour_share_cap_on_the_reference(name):
    """The share of float64 reference values within 2 * 2^-24 * max(1, |v|) of a bf16 rounding boundary
    (all that may ever use the neighbour allowance) is under the 1 % cap."""
    share = P.boundary_share(P.problem(name, "bf16"))
    print(f"{name}: {share:.4%} of the reference within the window of a bf16 boundary")
    assert share <= P.NEIGHBOUR_SHARE


EMULATED = [pytest.param(c.name, dt, id=f"{c.name}-{dt}") for c in P.SMALL_CASES for dt in c.dtypes
            if c.name != "grid" and (c not in P.CHANNEL_CASES or c.name in ("c1-h8", "c6-h64", "c7-h128", "c13-h256"))]


@pytest.mark.parametrize("name,dtype", EMULATED)
def test_emulation_passes_the_checkers(name, dtype):
    """A numpy fp32 restatement of the kernels' dataflow passes Stage A and Stage B on every case small
    enough to emulate (the flat grid case and most of the channel x hidden grid are left to the GPU)."""
    prob = P.problem(name, dtype)
    work = P.emulate_tables(prob)
    tabs, flags = P.read_work(work, prob)
    a = P.check_tables(prob, tabs, flags)
    assert a.ok, str(a)
    assert (work[prob.work_words:].view(np.uint32) == P.WORK_FILL).all()
    b = P.check_stream(prob, tabs, flags, P.emulate_stream(prob, work))
    assert b.ok, str(b)
    print(f"{name} {dtype}: emulation at {a.figures['table_ratio']:.3f} of the Stage-A bar, figures {b.figures}")
    if prob.kernel == "rows" and name in ("s1", "flagA", "smallx"):
        flat = P.check_stream(prob, tabs, flags, P.emulate_stream(prob, work, kernel="flat"), kernel="flat")
        assert flat.ok, str(flat)


# defect -> (case, dtype): the named case on which the checker must fail
PLANTED_TABLES = {"unbiased": ("short", "f32"), "eps_outside": ("eps", "f32"), "max_l1": ("chains", "f32"),
                  "beta_b": ("s1", "bf16"), "bias_both": ("bias", "f32")}
PLANTED_STREAM = {"two_one": ("s1", "bf16"), "seg_stop": ("s2", "f32"), "prod_flagged": ("flagA", "bf16"),
                  "no_med3": ("smallx", "bf16")}


@pytest.mark.parametrize("defect", P.TABLE_DEFECTS)
def test_planted_table_defects_fail_stage_a(defect):
    name, dtype = PLANTED_TABLES[defect]
    prob = P.problem(name, dtype)
    tabs, flags = P.read_work(P.emulate_tables(prob, defect), prob)
    rep = P.check_tables(prob, tabs, flags)
    print(f"{defect} on {name} {dtype}: {rep.figures['table_ratio']:.3g} x the Stage-A bar")
    assert not rep.ok and rep.figures["table_ratio"] >= 2


@pytest.mark.parametrize("defect", P.STREAM_DEFECTS)
def test_planted_stream_defects_fail_stage_b(defect):
    """Stage B compares bits, so a defect's size is counted in elements; where the defect is numeric
    (no_med3, prod_flagged) its worst error against the float64 ELU is at least 2 x PROD_ABS as well."""
    name, dtype = PLANTED_STREAM[defect]
    prob = P.problem(name, dtype)
    work = P.emulate_tables(prob)
    tabs, flags = P.read_work(work, prob)
    good = P.emulate_stream(prob, work)
    bad = P.emulate_stream(prob, work, defect=defect)
    rep = P.check_stream(prob, tabs, flags, bad)
    assert not rep.ok
    wrong = good != bad
    if defect in ("two_one", "seg_stop"):
        assert (bad[wrong] == P.GUARD[dtype]).all() and "guard word left" in str(rep)
        print(f"{defect} on {name} {dtype}: {int(wrong.sum())} elements keep the guard word")
    else:
        with np.errstate(all="ignore"):
            d = np.abs(P.bf16_val(good[wrong]).astype(np.float64) - P.bf16_val(bad[wrong]).astype(np.float64))
        worst = np.where(np.isnan(d), np.inf, d).max()
        print(f"{defect} on {name} {dtype}: {int(wrong.sum())} elements differ, worst by {worst:.3g} "
              f"= {worst / P.PROD_ABS:.3g} x PROD_ABS")
        assert worst >= 2 * P.PROD_ABS


def test_fma32_rounds_once():
    """fma32 against exact rational arithmetic on random operands and on constructed double-rounding ties."""
    from fractions import Fraction
    rng = np.random.default_rng(0)
    a = rng.normal(size=2000).astype(np.float32)
    b = rng.normal(size=2000).astype(np.float32)
    c = (-a.astype(np.float64) * b * (1 + rng.normal(size=2000) * 1e-3)).astype(np.float32)
    # ties: a * b + c = a representable fp32 + half an ulp + a bit far below
    a[:3], b[:3], c[:3] = np.float32(1 + 2.0 ** -23), np.float32(1 + 2.0 ** -23), np.float32([2.0 ** -24, -2.0 ** -24, 2.0 ** 23])
    got = P.fma32(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo, hi = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
        assert abs(Fraction(float(g)) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))
