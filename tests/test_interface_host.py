"""The interface labels without a GPU: the yardsticks of tests/interface_cases.py against each other and
against the independent oracle stored in tests/golden/4heq_interface.npz (scipy's cKDTree over the fp64
coordinates), ranking.interface_atoms, and the host contract of di_interface_work_bytes /
di_interface_labels_batch(_check): every refusal comes before any launch, so none needs a device."""
import ctypes

import numpy as np
import pytest

import interface_cases as ic
from gpu_common import load_case


def test_4heq_every_yardstick_agrees_with_the_kdtree_labels():
    z = load_case("4heq_interface")
    c0, c1 = (z["xyz0"], z["res_off0"]), (z["xyz1"], z["res_off1"])
    assert z["labels"].shape == (145, 145) and c0[0].shape == c1[0].shape == (1076, 3)
    assert int(z["labels"].sum()) == int(z["num_pos"]) == 80
    assert max(np.diff(c0[1]).max(), np.diff(c1[1]).max()) == 14
    assert np.array_equal(ic.ref_labels_f32(c0, c1), z["labels"])
    assert np.array_equal(ic.ref_labels_f64(c0, c1), z["labels"])
    assert len(ic.ambiguous(c0, c1)) == 0


@pytest.mark.parametrize("seed,l1,l2", ic.RANDOM_FLOAT)
def test_random_float_cases_have_no_ambiguous_pair(seed, l1, l2):
    """So the GPU test's comparison with the fp64 labels excludes nothing."""
    c0, c1 = ic.random_float_case(seed, l1, l2)
    assert len(ic.ambiguous(c0, c1)) == 0
    lab = ic.ref_labels_f32(c0, c1)
    assert np.array_equal(lab, ic.ref_labels_f64(c0, c1))
    assert 20 <= lab.sum() < lab.size // 10          # an interface, not an empty or a full map


def test_grid_exact_case_is_exact_and_has_ties():
    c0, c1 = ic.grid_exact_case()
    for xyz, off in (c0, c1):
        assert np.array_equal(xyz * 8, np.round(xyz * 8)) and np.abs(xyz).max() <= 64
        assert 1 <= np.diff(off).min() and np.diff(off).max() <= 20
    d32, d64 = ic._pair_d2(c0, c1, np.float32), ic._pair_d2(c0, c1, np.float64)
    assert np.array_equal(d32.astype(np.float64), d64)           # every fp32 operation was exact
    assert (d64 == 36.0).sum() >= 2
    assert np.array_equal(ic.ref_labels_f32(c0, c1), ic.ref_labels_f64(c0, c1))


def test_contraction_triples_split_the_unfused_and_the_fused_sum():
    triples = ic.contraction_triples()
    assert len(triples) == 3
    verdicts = set()
    for t in triples:
        u, f = ic.unfused_d2(t), ic.fused_d2(t)
        assert (u <= np.float32(36)) != (f <= np.float32(36)), (t, u, f)
        assert int(ic.ref_labels_f32(*ic.contraction_case(t))[0, 0]) == int(u <= np.float32(36))
        verdicts.add(bool(u <= np.float32(36)))
    assert verdicts == {True, False}
    # the example of the issue text
    t = np.array([4.4490314, 3.2312827, -2.4010274], dtype=np.float32)
    assert ic.unfused_d2(t) == np.float32(36.0) and ic.fused_d2(t) > np.float32(36.0)


def test_constructed_cases_are_what_they_claim():
    assert ic.ref_labels_f32(*ic.boundary_case(False)).tolist() == [[1]]
    assert ic.ref_labels_f32(*ic.boundary_case(True)).tolist() == [[0]]
    for counts in ic.STAGING_COUNTS:
        c0, c1 = ic.staging_case(counts)
        assert np.array_equal(ic.ref_labels_f32(c0, c1), np.eye(len(counts), dtype=np.uint8))
        d2 = ic._pair_d2(c0, c1, np.float64)
        last0, last1 = c0[1][1:] - 1, c1[1][1:] - 1
        assert (d2 <= 36.0).sum() == len(counts) and (d2[last0, last1] <= 36.0).all()
    assert sum(ic.STAGING_COUNTS[1]) > 2048 > sum(ic.STAGING_COUNTS[1][:10])     # crosses the staged chunk
    for diagonal in (False, True):
        for shift in ((0.0, 0.0, 0.0), ic.CULL_SHIFT):
            c0, c1 = ic.cull_case(diagonal, shift)
            centre0, centre1 = c0[0][:16].astype(np.float64).mean(0), c1[0][2:].astype(np.float64).mean(0)
            assert np.linalg.norm(centre0 - centre1) > 30.0
            if not diagonal:        # exact coordinates: the ends touch at exactly 6 A
                assert ic._pair_d2(c0, c1, np.float64)[15, 2] == 36.0
                assert ic.ref_labels_f32(c0, c1).tolist() == [[0, 1], [1, 0]]


# ---- interface_atoms ----------------------------------------------------------------------------------
def test_interface_atoms_groups_filters_and_refuses():
    from deepinteract_amd.ranking import interface_atoms
    xyz = np.arange(24, dtype=np.float64).reshape(8, 3) + 0.1
    res = [7, 7, 7, 3, 3, 9, 9, 9]
    got, off = interface_atoms(xyz, res)
    assert got.dtype == np.float32 and off.dtype == np.int32 and got.flags["C_CONTIGUOUS"]
    assert np.array_equal(got, xyz.astype(np.float32)) and off.tolist() == [0, 3, 5, 8]
    el = ["N", "H", "C", " h", "O", "H ", "H", "S"]
    got, off = interface_atoms(xyz, res, el)
    assert np.array_equal(got, xyz[[0, 2, 4, 7]].astype(np.float32)) and off.tolist() == [0, 2, 3, 4]
    # a residue all of whose atoms are hydrogen disappears; keys may be rows (chain, number, insertion code)
    keys = np.array([("A", " 10", " ")] * 2 + [("A", " 10", "A")] * 3 + [("A", " 11", " ")] * 3, dtype=str)
    got, off = interface_atoms(xyz, keys, ["C", "C", "H", "H", "H", "C", "N", "O"])
    assert off.tolist() == [0, 2, 5]
    with pytest.raises(ValueError, match="reappears"):
        interface_atoms(xyz, [1, 1, 2, 2, 1, 3, 3, 3])
    with pytest.raises(ValueError, match="no heavy atoms"):
        interface_atoms(xyz, res, ["H"] * 8)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        interface_atoms(np.zeros((8, 2)), res)
    with pytest.raises(ValueError, match="one residue index per atom"):
        interface_atoms(xyz, res[:-1])
    with pytest.raises(ValueError, match="one element symbol per atom"):
        interface_atoms(xyz, res, el[:-1])


# ---- the C contract -----------------------------------------------------------------------------------
P = 16 * 1024       # a 16-B aligned dummy address, never dereferenced


def _items(shapes):
    from deepinteract_amd import _lib
    items = (_lib.DiInterfaceItem * len(shapes))()
    for it, (l1, l2, a0, a1) in zip(items, shapes):
        it.xyz0 = it.res_off0 = it.xyz1 = it.res_off1 = it.labels = P
        it.l1, it.l2, it.a0, it.a1 = l1, l2, a0, a1
    return items


def _check(lib, items, count, cutoff=6.0, work=P, dev=P):
    return lib.di_interface_labels_batch_check(items, ctypes.c_void_p(dev), count, ctypes.c_float(cutoff),
                                               ctypes.c_void_p(work))


def test_struct_layouts_and_flag_values():
    from deepinteract_amd import _lib
    assert ctypes.sizeof(_lib.DiInterfaceItem) == 5 * 8 + 4 * 4 + 8
    assert ctypes.sizeof(_lib.DiInterfaceStats) == 16
    assert (_lib.DI_IF_OFFSETS, _lib.DI_IF_EMPTY, _lib.DI_IF_NONFINITE) == (1, 2, 4)
    assert _lib.load().di_abi_version() == 8


def test_work_bytes_layout_stats_first_then_spheres():
    from deepinteract_amd import _lib
    lib = _lib.load()
    shapes = [(1, 1, 1, 1), (3, 5, 20, 40), (145, 145, 1076, 1076), (7, 400, 90, 5000), (4096, 4096, 60000, 60000)]
    items = _items(shapes)
    nb = lib.di_interface_work_bytes(items, len(shapes))
    at = 16 * len(shapes)                       # the di_interface_stats records
    for it, (l1, l2, _, _) in zip(items, shapes):
        assert it.work_off == at and at % 16 == 0
        at += 16 * (l1 + l2)                    # one float4 per residue of either chain
    assert nb == at
    assert _check(lib, items, len(shapes)) == 0
    items[2].work_off += 16
    assert _check(lib, items, len(shapes)) == -1                  # not the helper's
    assert lib.di_interface_labels_batch(items, ctypes.c_void_p(P), len(shapes), ctypes.c_float(6.0),
                                         ctypes.c_void_p(P), None) == -1


def test_every_refusal():
    from deepinteract_amd import _lib
    lib = _lib.load()
    good = (3, 5, 20, 40)

    def ready(shape=good):
        items = _items([shape])
        assert lib.di_interface_work_bytes(items, 1) > 0
        return items

    assert _check(lib, ready(), 1) == 0
    # DI_EINVAL
    assert lib.di_interface_work_bytes(None, 1) == -1
    for count in (0, -1):
        assert lib.di_interface_work_bytes(ready(), count) == -1 and _check(lib, ready(), count) == -1
    assert _check(lib, None, 1) == -1 and _check(lib, ready(), 1, dev=0) == -1 and _check(lib, ready(), 1, work=0) == -1
    for field in ("xyz0", "res_off0", "xyz1", "res_off1", "labels"):
        items = ready()
        setattr(items[0], field, None)
        assert _check(lib, items, 1) == -1, field
    for k in range(4):
        for bad in (0, -1, -2 ** 31):
            shape = list(good)
            shape[k] = bad
            items = _items([tuple(shape)])
            assert lib.di_interface_work_bytes(items, 1) == -1, shape
            assert _check(lib, items, 1) == -1, shape
    for cutoff in (0.0, -6.0, float("nan"), float("inf"), -float("inf")):
        assert _check(lib, ready(), 1, cutoff=cutoff) == -1, cutoff
    assert _check(lib, ready(), 1, cutoff=1e-30) == 0
    for work in (P + 4, P + 8, P + 1):
        assert _check(lib, ready(), 1, work=work) == -1
    for field in ("xyz0", "xyz1", "res_off0", "res_off1"):
        for delta in (1, 2):
            items = ready()
            setattr(items[0], field, P + delta)
            assert _check(lib, items, 1) == -1, field
        items = ready()
        setattr(items[0], field, P + 4)          # 4-B aligned is enough
        assert _check(lib, items, 1) == 0, field
    items = ready()
    items[0].labels = P + 1                      # a map may start anywhere
    assert _check(lib, items, 1) == 0
    # DI_ERANGE
    for shape in ((1 << 15, 1 << 14, 9, 9), (1, 1 << 29, 9, 9), (2 ** 31 - 1, 2 ** 31 - 1, 9, 9),
                  (3, 5, 1 << 24, 40), (3, 5, 20, 1 << 24), (3, 5, 2 ** 31 - 1, 2 ** 31 - 1)):
        items = _items([shape])
        assert lib.di_interface_work_bytes(items, 1) == -2, shape
        assert _check(lib, items, 1) == -2, shape
    for shape in ((1 << 15, (1 << 14) - 1, 9, 9), (1, (1 << 29) - 1, 9, 9), (3, 5, (1 << 24) - 1, (1 << 24) - 1)):
        assert _check(lib, ready(shape), 1) == 0, shape
    # the refusing call launches nothing: the same codes from the launching entry point
    assert lib.di_interface_labels_batch(ready(), ctypes.c_void_p(P), 1, ctypes.c_float(0.0), ctypes.c_void_p(P),
                                         None) == -1
    assert lib.di_interface_labels_batch(_items([(1, 1 << 29, 9, 9)]), ctypes.c_void_p(P), 1, ctypes.c_float(6.0),
                                         ctypes.c_void_p(P), None) == -2


def test_batch_max_accepted_and_one_more_refused():
    from deepinteract_amd import _lib
    lib = _lib.load()
    n = _lib.DI_BATCH_MAX
    items = _items([(1 + i % 7, 1 + i % 5, 3, 4) for i in range(n + 1)])
    nb = lib.di_interface_work_bytes(items, n)
    assert nb == 16 * n + sum(16 * (2 + i % 7 + i % 5) for i in range(n))
    offs = [it.work_off for it in items[:n]]
    assert all(o % 16 == 0 for o in offs) and offs[0] == 16 * n
    ends = [o + 16 * (it.l1 + it.l2) for o, it in zip(offs, items)]
    assert offs[1:] == ends[:-1] and ends[-1] == nb          # back to back: no overlap, no gap
    assert _check(lib, items, n) == 0
    assert lib.di_interface_work_bytes(items, n + 1) == -2
    assert _check(lib, items, n + 1) == -2
    assert lib.di_interface_labels_batch(items, ctypes.c_void_p(P), n + 1, ctypes.c_float(6.0), ctypes.c_void_p(P),
                                         None) == -2
