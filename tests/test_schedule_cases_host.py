"""What tests/test_gpu_schedule_small.py rests on, checked without a GPU (tests/schedule_cases.py):

* the layouts meet the schedule's alignment rule (node rows, every h2 row, every l2 multiples of a
  16-byte vector) for the dtypes they are stated for, ragged4 fails it at 8 elements, ragged8's 136
  rows end in an 8-row block, and the micro-batches of a family have equal node counts but different
  numbers;
* check_pairs passes a pair tensor built on the CPU and fails, naming the (job, complex, half), on the
  mistakes a queue kernel or a descriptor table makes: the two halves swapped, complex 1's tensor at
  complex 2's offset, chain 1's rows shifted by one, the last 8-row block never written (NaN), one
  element's lowest mantissa bit flipped; in bf16 and fp32;
* the float64 oracle agrees with the fp32 oracle within 1e-5 on every chain of every micro-batch
  (tests/test_geot_cases_host.py's bound; reference against reference), and no reference row is below
  0.1 of its tensor's maximum, so the normwise bounds of the GPU file cannot hide a bad row.
"""
import numpy as np
import pytest
import torch

import geot_cases as C
import schedule_cases as S

CHAINS = [(lay, feats, mb, g) for lay, feats in S.FAMILIES for mb in range(S.N_MB) for g in range(len(S.chain_sizes(lay)))]


def test_layouts_meet_the_alignment_rule():
    assert S.LAYOUTS["ragged8"] == [(24, 136), (72, 40), (136, 24)] and S.LAYOUTS["ragged4"] == [(28, 36), (68, 44)]
    for layout, dtypes in S.DTYPES.items():
        for dtype in dtypes:
            assert S.aligned(layout, S.VEC[dtype]), (layout, dtype)
    assert S.DTYPES == {"ragged8": ("bf16", "f32"), "ragged4": ("f32",)}
    assert not S.aligned("ragged4", 8)
    assert all(n % 4 == 0 and n % 8 for n in S.chain_sizes("ragged4"))
    assert all(n % 8 == 0 for n in S.chain_sizes("ragged8"))
    # each term of the rule on its own: a layout that breaks only that term is refused
    h1r, h2r, l1, l2, n_rows = S.descriptors("ragged4")
    assert (h1r, h2r, l1, l2, n_rows) == ([0, 64], [28, 132], [28, 68], [36, 44], 176)
    assert n_rows % 8 == 0 and any(r % 8 for r in h2r) and any(b % 8 for b in l2)
    try:
        S.LAYOUTS["rows_only"] = [(8, 8), (8, 12)]      # l2 and n_rows off 8, h2 rows on it
        S.LAYOUTS["h2_only"] = [(12, 8), (12, 8)]       # h2 rows off 8 alone
        S.LAYOUTS["l2_only"] = [(8, 12), (12, 8)]       # one l2 off 8 alone (n_rows 40, h2 rows 8, 32)
        assert not S.aligned("rows_only", 8) and S.aligned("rows_only", 4)
        assert not S.aligned("h2_only", 8) and S.descriptors("h2_only")[4] % 8 == 0
        assert not S.aligned("l2_only", 8) and all(r % 8 == 0 for r in S.descriptors("l2_only")[1])
    finally:
        for k in ("rows_only", "h2_only", "l2_only"):
            S.LAYOUTS.pop(k, None)
    # ragged8: three 64-row blocks for max(l1), the last of 8 rows; the shorter complexes leave empty items
    _, _, l1, _, _ = S.descriptors("ragged8")
    assert max(l1) == 136 and -(-max(l1) // 64) == 3 and max(l1) - 128 == 8
    assert sorted(-(-a // 64) for a in l1) == [1, 2, 3]


def test_micro_batches_share_shape_not_numbers():
    for layout, feats in S.FAMILIES:
        sizes = S.chain_sizes(layout)
        first = [S.host_item(layout, feats, 0, g) for g in range(len(sizes))]
        for mb in range(S.N_MB):
            items = [S.host_item(layout, feats, mb, g) for g in range(len(sizes))]
            assert [it["num_nodes"] for it in items] == sizes
            assert sum(it["num_nodes"] for it in items) == S.descriptors(layout)[4]
            for it in items:
                E = it["src"].numel()
                assert it["node_f"].shape == (it["num_nodes"], 113) and it["edge_f"].shape == (E, 28)
                assert bool((it["dst"][1:] >= it["dst"][:-1]).all())
                assert 0 <= int(it["src"].min()) and int(it["src"].max()) < it["num_nodes"]
                assert 0 <= int(min(it["src_nbr"].min(), it["dst_nbr"].min()))
                assert int(max(it["src_nbr"].max(), it["dst_nbr"].max())) < E
                if feats == "knn":
                    assert E == S.K * it["num_nodes"]
            if mb:
                assert not any(torch.equal(a["node_f"], b["node_f"]) for a, b in zip(first, items))


def test_featurisations():
    from deepinteract_amd.graph import edge_feats_geo_ref
    for layout, feats, mb, g in CHAINS:
        it = S.host_item(layout, feats, mb, g)
        assert edge_feats_geo_ref(it["edge_f"]) == (feats == "knn"), (layout, feats, mb, g)
        if feats == "general":
            deg = torch.bincount(it["dst"], minlength=it["num_nodes"])
            assert deg[:4].tolist() == list(S.GENERAL_HEAD) and int(deg[4:].max()) <= S.GENERAL_MAX_DEG
            assert torch.allclose(it["edge_f"][:, 23:27].norm(dim=1), torch.ones(it["edge_f"].shape[0]))


# ---- check_pairs -------------------------------------------------------------------------------------
def _correct(dtype):
    h1r, h2r, l1, l2, n_rows = S.descriptors("ragged8")
    h = torch.randn(n_rows, S.H, generator=torch.Generator().manual_seed(3)).to(S.TORCH_DT[dtype])
    return h, (h1r, h2r, l1, l2), S.pair_reference(h, h1r, h2r, l1, l2)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_check_pairs_passes_the_reference(dtype):
    h, d, buf = _correct(dtype)
    assert buf.numel() == S.numel("ragged8") and buf.dtype == h.dtype
    S.check_pairs(S.pair_views(buf, d[2], d[3]), h, *d, job=0)
    # against the reference's own construction (oracle.pair_tensor) for one complex
    from oracle import geot_oracle as O
    t = O.pair_tensor(h[d[0][1]:d[0][1] + d[2][1]].float(), h[d[1][1]:d[1][1] + d[3][1]].float())
    assert torch.equal(S.pair_views(buf, d[2], d[3])[1].float(), t)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_check_pairs_catches_mutations(dtype):
    h, d, good = _correct(dtype)
    h1r, h2r, l1, l2 = d
    H = S.H
    offs = [0]
    for a, b in zip(l1, l2):
        offs.append(offs[-1] + 2 * H * a * b)

    def views_of(buf):
        return S.pair_views(buf, l1, l2)

    mutants = {}
    # the two halves of complex 1 swapped (l1 != l2 there: each half refilled from the other chain's
    # features would not even have the shape, so the channel blocks trade places)
    buf = good.clone()
    v = views_of(buf)[1]
    v.copy_(torch.cat([v[:, H:], v[:, :H]], 1))
    mutants["halves swapped"] = (buf, (1, 0))
    # complex 1's tensor written at complex 2's offset (a wrong out_off), complex 1 itself in place
    buf = good.clone()
    n1 = offs[2] - offs[1]
    assert n1 <= offs[3] - offs[2]
    buf[offs[2]:offs[2] + n1] = good[offs[1]:offs[2]]
    mutants["complex 1 at complex 2's offset"] = (buf, (2, 0))
    # chain 1's rows of complex 0 shifted by one (a wrong h1 row)
    buf = good.clone()
    v = views_of(buf)[0]
    v[:, :H] = torch.roll(v[:, :H], 1, dims=2)
    mutants["h1 rows shifted by one"] = (buf, (0, 0))
    # the last 8-row block (rows 128 .. 135 of the 136-row complex) never written; both halves miss it
    buf = good.clone()
    views_of(buf)[2][:, :, 128:] = float("nan")
    mutants["last 8-row block NaN"] = (buf, (2, 0))
    # the same block missing in chain 2's half alone is named half 1
    buf = good.clone()
    views_of(buf)[2][:, H:, 128:] = float("nan")
    mutants["last 8-row block NaN, half 1"] = (buf, (2, 1))
    # one element's lowest mantissa bit
    buf = good.clone()
    at = offs[1] + (H + 5) * l1[1] * l2[1] + 7 * l2[1] + 3  # complex 1, channel H + 5, row 7, column 3
    S._bits(buf)[at] ^= 1
    assert int((buf != good).sum()) == 1
    mutants["one mantissa bit"] = (buf, (1, 1))

    for what, (buf, (cx, half)) in mutants.items():
        with pytest.raises(AssertionError, match=f"job 7, complex {cx}, half {half} ") as exc:
            S.check_pairs(views_of(buf), h, *d, job=7)
        print(f"{dtype} {what}: {exc.value}")
    with pytest.raises(AssertionError, match="channel 133, row 7, column 3"):
        S.check_pairs(views_of(mutants["one mantissa bit"][0]), h, *d, job=7)
    S.check_pairs(views_of(good), h, *d, job=7)  # the source of every mutant still passes


def test_check_pairs_tells_the_signs_of_zero_apart():
    h, d, good = _correct("f32")
    h = h.clone()
    h[d[0][0], 0] = 0.0
    good = S.pair_reference(h, *d)
    S.check_pairs(S.pair_views(good, d[2], d[3]), h, *d)
    buf = good.clone()
    buf[0] = -0.0  # complex 0, channel 0, row 0, column 0: torch.equal would pass it
    with pytest.raises(AssertionError, match="complex 0, half 0 "):
        S.check_pairs(S.pair_views(buf, d[2], d[3]), h, *d)


# ---- the oracle on these chains ----------------------------------------------------------------------
def _ref(layout, feats, mb, g):
    return C.oracle64(C.state_dict(S.L), S.host_item(layout, feats, mb, g), S.L, key=("sched_host", layout, feats, mb, g))


@pytest.mark.parametrize("layout,feats,mb,g", CHAINS)
def test_oracle64_matches_oracle32(layout, feats, mb, g):
    n64, e64 = _ref(layout, feats, mb, g)
    n32, e32 = C.oracle32(C.state_dict(S.L), S.host_item(layout, feats, mb, g), S.L)
    assert n32.dtype == np.float32 and n64.dtype == np.float64
    en, ee = C.check(n32, n64)[0], C.check(e32, e64)[0]
    print(f"{layout} {feats} mb {mb} chain {g}: oracle32 vs oracle64 node {en:.2e} edge {ee:.2e}")
    assert max(en, ee) <= 1e-5, (en, ee)


@pytest.mark.parametrize("layout,feats,mb,g", CHAINS)
def test_no_small_reference_row(layout, feats, mb, g):
    for what, ref in zip(("node", "edge"), _ref(layout, feats, mb, g)):
        ratio = np.abs(ref).max(axis=1) / np.abs(ref).max()
        print(f"{layout} {feats} mb {mb} chain {g} {what}: smallest row max / tensor max {ratio.min():.3f}")
        assert ratio.min() >= 0.1, (what, int(ratio.argmin()), float(ratio.min()))
