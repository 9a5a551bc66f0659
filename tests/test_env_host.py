"""The residue-environment features without a GPU: structure.residue_atoms and structure.read_pdb, the host
contract of di_residue_env_work_bytes / di_residue_env_batch(_check) (every refusal comes before any
launch, so none needs a device), the two oracles of tests/env_cases.py against each other on every case
the GPU tests use, and the fixture tests/golden/4heq_env.npz against a fresh run of the fp64 oracle."""
import ctypes

import numpy as np
import pytest

import env_cases as ec
from gpu_common import load_case


# ---- residue_atoms ------------------------------------------------------------------------------------
def test_residue_atoms_groups_codes_and_refuses():
    from deepinteract_amd.structure import AA_LETTERS, residue_atoms
    from deepinteract_amd.synth import RESNAMES
    assert AA_LETTERS == ec.AA and RESNAMES == ec.ONE_HOT
    xyz = np.arange(36, dtype=np.float64).reshape(12, 3) + 0.1
    res = [7] * 5 + [3] * 4 + [9] * 3
    names = ["N", "CA", "C", "O", "CB", " n ", "ca", "C", "O", "CA", "HA", "CG1"]
    resname = ["TRP"] * 5 + ["gly"] * 4 + ["MSE"] * 3
    got, off, role, aa, col = residue_atoms(xyz, res, names, resname)
    assert got.dtype == np.float32 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, xyz.astype(np.float32))
    assert off.dtype == np.int32 and off.tolist() == [0, 5, 9, 12]
    assert role.dtype == aa.dtype == col.dtype == np.uint8
    assert role.tolist() == [1, 2, 3, 4, 5, 1, 2, 3, 4, 2, 0, 0]          # hydrogens are kept, as role 0
    # TRP -> 'W' and column 0; GLY -> 'G' and column 10; an unknown name -> '-' (20) and the GLN bin
    assert aa.tolist() == [ec.AA.index("W"), ec.AA.index("G"), 20] and col.tolist() == [0, 10, 19]
    assert [ec.column_of(t) for t in aa] == col.tolist()
    for letter in ec.AA[:20]:                                             # all twenty, both codes
        _, _, _, a1, c1 = residue_atoms(xyz[:1], [1], ["CA"], [ec.THREE[letter]])
        assert a1.tolist() == [ec.AA.index(letter)] and c1.tolist() == [ec.ONE_HOT.index(ec.THREE[letter])]
    # a real GLN shares the last bin with the unknowns but keeps its own aa code
    _, _, _, a1, c1 = residue_atoms(xyz[:1], [1], ["CA"], ["GLN"])
    assert a1.tolist() == [ec.AA.index("Q")] and c1.tolist() == [19]
    # keys may be rows (chain, number, insertion code)
    keys = np.array([("A", " 10", " ")] * 5 + [("A", " 10", "A")] * 4 + [("A", " 11", " ")] * 3, dtype=str)
    assert residue_atoms(xyz, keys, names, resname)[1].tolist() == [0, 5, 9, 12]
    with pytest.raises(ValueError, match="reappears"):
        residue_atoms(xyz, [1] * 5 + [2] * 4 + [1] * 3, names, resname)
    with pytest.raises(ValueError, match="no atoms"):
        residue_atoms(np.zeros((0, 3)), [], [], [])
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        residue_atoms(np.zeros((12, 2)), res, names, resname)
    with pytest.raises(ValueError, match="one residue index per atom"):
        residue_atoms(xyz, res[:-1], names, resname)
    with pytest.raises(ValueError, match="one atom name per atom"):
        residue_atoms(xyz, res, names[:-1], resname)
    with pytest.raises(ValueError, match="one residue name per atom"):
        residue_atoms(xyz, res, names, resname[:-1])


# ---- read_pdb -------------------------------------------------------------------------------------------
def _atom(serial, name, alt, resname, chain, num, icode, x, y, z, el, record="ATOM  "):
    name4 = name if len(name) == 4 else " " + name.ljust(3)
    return (f"{record}{serial:5d} {name4}{alt}{resname:>3} {chain}{num:4d}{icode}   {x:8.3f}{y:8.3f}{z:8.3f}"
            f"{1.0:6.2f}{0.0:6.2f}          {el:>2}\n")


PDB_TEXT = "".join([
    "HEADER    TEST\n", "MODEL        1\n",
    _atom(1, "N", " ", "ALA", "A", 1, " ", 1.0, 2.0, 3.0, "N"),
    _atom(2, "CA", " ", "ALA", "A", 1, " ", 1.5, 2.5, 3.5, "C"),
    _atom(3, "CB", "A", "ALA", "A", 1, " ", -11.125, 0.0, 99.999, "C"),
    _atom(4, "CB", "B", "ALA", "A", 1, " ", 7.0, 7.0, 7.0, "C"),
    _atom(5, "HB1", "A", "ALA", "A", 1, " ", 4.0, 4.0, 4.0, ""),
    _atom(6, "CA", "B", "SER", "A", 1, "A", 5.0, 5.0, 5.0, "C"),      # first altloc seen in ITS residue: B
    _atom(7, "CA", "A", "SER", "A", 1, "A", 6.0, 6.0, 6.0, "C"),
    _atom(8, "CA", " ", "CA", "A", 300, " ", 9.0, 9.0, 9.0, "CA", record="HETATM"),
    "TER\n",
    _atom(9, "CA", " ", "GLY", "B", 1, " ", 8.0, 8.0, 8.0, "C"),
    "ENDMDL\n", "MODEL        2\n",
    _atom(10, "CA", " ", "GLY", "A", 1, " ", 0.0, 0.0, 0.0, "C"),
    "ENDMDL\n", "END\n"])


def test_read_pdb_altloc_models_hetatm_and_chain_filter(tmp_path):
    from deepinteract_amd.structure import read_pdb, residue_atoms
    path = tmp_path / "t.pdb"
    path.write_text(PDB_TEXT)
    xyz, keys, names, resnames, elements = read_pdb(str(path))
    assert xyz.dtype == np.float64 and xyz.shape == (6, 3)
    assert names.tolist() == ["N", "CA", "CB", "HB1", "CA", "CA"]         # altloc B of ALA, A of SER, HETATM, model 2: gone
    assert xyz[2].tolist() == [-11.125, 0.0, 99.999] and xyz[4].tolist() == [5.0, 5.0, 5.0]
    assert resnames.tolist() == ["ALA"] * 4 + ["SER", "GLY"]
    assert elements.tolist() == ["N", "C", "C", "H", "C", "C"]            # an empty element column: from the name
    assert keys.tolist() == [["A", "   1", " "]] * 4 + [["A", "   1", "A"], ["B", "   1", " "]]
    _, off, role, aa, col = residue_atoms(xyz, keys, names, resnames)
    assert off.tolist() == [0, 4, 5, 6] and role.tolist() == [1, 2, 5, 0, 2, 2]
    only_b = read_pdb(str(path), chain="B")
    assert only_b[0].tolist() == [[8.0, 8.0, 8.0]] and only_b[3].tolist() == ["GLY"]
    assert read_pdb(str(path), chain="AB")[0].shape == (6, 3)
    with pytest.raises(ValueError, match="no ATOM record"):
        read_pdb(str(path), chain="C")


# ---- the C contract -------------------------------------------------------------------------------------
P = 16 * 1024       # a 16-B aligned dummy address, never dereferenced
POINTERS = ("xyz", "res_off", "role", "aa", "resname", "dips", "amide_norm", "backbone", "cn_raw")
ALIGNED = ("xyz", "res_off", "dips", "amide_norm", "backbone", "cn_raw")


def _items(shapes):
    from deepinteract_amd import _lib
    items = (_lib.DiEnvItem * len(shapes))()
    for it, (l, a) in zip(items, shapes):
        for f in POINTERS:
            setattr(it, f, P)
        it.l, it.a = l, a
    return items


def _check(lib, items, count, c2=ec.C2, work=P, dev=P):
    return lib.di_residue_env_batch_check(items, ctypes.c_void_p(dev), count, ctypes.c_float(c2),
                                          ctypes.c_void_p(work))


def test_struct_layouts_flag_values_and_the_default_c2():
    from deepinteract_amd import _lib, structure
    assert ctypes.sizeof(_lib.DiEnvItem) == 9 * 8 + 2 * 4 + 8
    assert ctypes.sizeof(_lib.DiEnvStats) == 16
    assert (_lib.DI_ENV_OFFSETS, _lib.DI_ENV_EMPTY, _lib.DI_ENV_NONFINITE, _lib.DI_ENV_BACKBONE) == (1, 2, 4, 8)
    assert (_lib.DI_ROLE_OTHER, _lib.DI_ROLE_N, _lib.DI_ROLE_CA, _lib.DI_ROLE_C, _lib.DI_ROLE_O,
            _lib.DI_ROLE_CB) == (ec.OTHER, ec.N, ec.CA, ec.C, ec.O, ec.CB)
    c2 = np.float32(8.0 * np.log(1000.0))                # sg = 2, thr = 1e-3: exp(-d2 / 8) > 1e-3
    assert np.float32(_lib.DI_ENV_C2) == np.float32(structure.ENV_C2) == np.float32(ec.C2) == c2
    assert c2 == np.float32(55.262043)
    assert structure.OWN_COLUMNS.tolist() == ec.OWN.tolist() and len(ec.OWN) == 63
    assert structure.EXTERN_COLUMNS.tolist() == ec.EXTERN.tolist() and len(ec.EXTERN) == 43
    assert _lib.load().di_abi_version() == 8


def test_work_bytes_layout_stats_first_then_three_float4_per_residue():
    from deepinteract_amd import _lib
    lib = _lib.load()
    shapes = [(1, 4), (3, 20), (145, 1076), (400, 5000), (4096, 60000)]
    items = _items(shapes)
    nb = lib.di_residue_env_work_bytes(items, len(shapes))
    at = 16 * len(shapes)                       # the di_env_stats records
    for it, (l, _) in zip(items, shapes):
        assert it.work_off == at and at % 16 == 0
        at += 48 * l                            # sphere, CA, u
    assert nb == at
    assert _check(lib, items, len(shapes)) == 0
    items[2].work_off += 16
    assert _check(lib, items, len(shapes)) == -1                  # not the helper's
    assert lib.di_residue_env_batch(items, ctypes.c_void_p(P), len(shapes), ctypes.c_float(ec.C2),
                                    ctypes.c_void_p(P), None) == -1


def test_every_refusal():
    from deepinteract_amd import _lib
    lib = _lib.load()

    def ready(shape=(3, 20)):
        items = _items([shape])
        assert lib.di_residue_env_work_bytes(items, 1) > 0
        return items

    assert _check(lib, ready(), 1) == 0
    # DI_EINVAL
    assert lib.di_residue_env_work_bytes(None, 1) == -1
    for count in (0, -1):
        assert lib.di_residue_env_work_bytes(ready(), count) == -1 and _check(lib, ready(), count) == -1
    assert _check(lib, None, 1) == -1 and _check(lib, ready(), 1, dev=0) == -1 and _check(lib, ready(), 1, work=0) == -1
    for field in POINTERS:
        items = ready()
        setattr(items[0], field, None)
        assert _check(lib, items, 1) == -1, field
    for k in range(2):
        for bad in (0, -1, -2 ** 31):
            shape = [3, 20]
            shape[k] = bad
            items = _items([tuple(shape)])
            assert lib.di_residue_env_work_bytes(items, 1) == -1, shape
            assert _check(lib, items, 1) == -1, shape
    for c2 in (0.0, -55.0, float("nan"), float("inf"), -float("inf")):
        assert _check(lib, ready(), 1, c2=c2) == -1, c2
    assert _check(lib, ready(), 1, c2=1e-30) == 0 and _check(lib, ready(), 1, c2=3e38) == 0
    for work in (P + 4, P + 8, P + 1):
        assert _check(lib, ready(), 1, work=work) == -1
    for field in ALIGNED:
        for delta in (1, 2):
            items = ready()
            setattr(items[0], field, P + delta)
            assert _check(lib, items, 1) == -1, field
        items = ready()
        setattr(items[0], field, P + 4)          # 4-B aligned is enough
        assert _check(lib, items, 1) == 0, field
    for field in ("role", "aa", "resname"):      # bytes may start anywhere
        items = ready()
        setattr(items[0], field, P + 1)
        assert _check(lib, items, 1) == 0, field
    # DI_ERANGE
    for shape in ((3, 1 << 24), (1 << 24, 20), (2 ** 31 - 1, 2 ** 31 - 1)):
        items = _items([shape])
        assert lib.di_residue_env_work_bytes(items, 1) == -2, shape
        assert _check(lib, items, 1) == -2, shape
    assert _check(lib, ready(((1 << 24) - 1, (1 << 24) - 1)), 1) == 0
    # the refusing call launches nothing: the same codes from the launching entry point
    assert lib.di_residue_env_batch(ready(), ctypes.c_void_p(P), 1, ctypes.c_float(0.0), ctypes.c_void_p(P),
                                    None) == -1
    assert lib.di_residue_env_batch(_items([(3, 1 << 24)]), ctypes.c_void_p(P), 1, ctypes.c_float(ec.C2),
                                    ctypes.c_void_p(P), None) == -2


def test_batch_max_accepted_and_one_more_refused():
    from deepinteract_amd import _lib
    lib = _lib.load()
    n = _lib.DI_BATCH_MAX
    items = _items([(1 + i % 7, 30) for i in range(n + 1)])
    nb = lib.di_residue_env_work_bytes(items, n)
    assert nb == 16 * n + sum(48 * (1 + i % 7) for i in range(n))
    offs = [it.work_off for it in items[:n]]
    assert all(o % 16 == 0 for o in offs) and offs[0] == 16 * n
    ends = [o + 48 * it.l for o, it in zip(offs, items)]
    assert offs[1:] == ends[:-1] and ends[-1] == nb          # back to back: no overlap, no gap
    assert _check(lib, items, n) == 0
    assert lib.di_residue_env_work_bytes(items, n + 1) == -2
    assert _check(lib, items, n + 1) == -2
    assert lib.di_residue_env_batch(items, ctypes.c_void_p(P), n + 1, ctypes.c_float(ec.C2), ctypes.c_void_p(P),
                                    None) == -2


# ---- the oracles on every case the GPU tests use -------------------------------------------------------
@pytest.mark.parametrize("seed,L", ec.RANDOM)
def test_random_cases_keep_both_margins_and_the_oracles_agree(seed, L):
    """So the GPU test's comparison with the fp64 oracle leaves out nothing: no residue pair's d2 within
    1e-4 relative of c2, no half-sphere |cos| below 1e-5 (fp32 moves either by a few 1e-7)."""
    case = ec.random_case(seed, L)
    counts = np.diff(case[1])
    assert len(counts) == L and counts.min() == 4 and counts.max() == 14
    rel, cos = ec.margins(case)
    assert rel > 1e-4 and cos > 1e-5, (rel, cos)
    o64, o32 = ec.oracle(case), ec.oracle(case, dtype=np.float32)
    assert ec.same(o64, o32, amide=False) == []
    assert np.abs(o64["amide"] - o32["amide"]).max() < 1e-5          # fp32 cross products of vectors of a few A
    assert o64["cn_raw"].min() < o64["cn_raw"].max() and o64["un"].max() > 0 and o64["dn"].min() >= 1
    assert (o64["amide"] == 0).all(axis=1).sum() >= (counts == 4).sum() > 0     # Gly, and residues without a CB


@pytest.mark.parametrize("L", ec.GRID_L)
def test_grid_cases_are_exact_and_hit_zero_dots(L):
    case = ec.grid_case(L)
    xyz = case[0]
    assert np.array_equal(xyz, np.round(xyz)) and np.abs(xyz).max() < 64
    o64, o32 = ec.oracle(case), ec.oracle(case, dtype=np.float32)
    assert ec.same(o64, o32) == []                                    # every fp32 operation was exact
    ca, u, _, _ = ec.geometry(case, np.float64)
    dots = ((ca[None] - ca[:, None]) * u[:, None]).sum(axis=2)
    nb = ec._per_residue(ec._pair_d2(xyz, np.float64) < ec.C2, case[1]) & ~np.eye(L, dtype=bool)
    assert (dots[nb] == 0).sum() > L                                  # exact zeros among the tests: down
    kinds = np.arange(L) % 7
    assert (u[kinds == 6] == 0).all() and (o64["un"][kinds == 6] == 0).all()      # cancelling unit vectors
    assert (o64["amide"][(kinds == 3) | (kinds == 5)] == 0).all()     # Gly; a side atom that is not a CB
    assert (np.abs(o64["amide"][kinds == 0]).sum(axis=1) > 0).any()   # (a CB on the N axis gives 0 too)
    assert (o64["un"] + o64["dn"] == o64["cn_raw"]).all() and o64["cn_raw"].min() < o64["cn_raw"].max()


def test_constructed_cases_are_what_they_claim():
    o = ec.oracle(ec.single_case(7))
    assert (o["cn_raw"], o["un"], o["dn"]) == (1, 0, 1) and o["cn"].tolist() == [0.0]
    assert o["hsaac"][0, 7] == 1 and o["hsaac"][0, 21 + 7] == 1 and o["hsaac"].sum() == 2
    for dtype in (np.float64, np.float32):
        assert ec.oracle(ec.boundary_case(False), ec.BOUNDARY_C2, dtype)["cn_raw"].tolist() == [1, 1]
        assert ec.oracle(ec.boundary_case(True), ec.BOUNDARY_C2, dtype)["cn_raw"].tolist() == [2, 2]
    x = ec.boundary_case(True)[0][:, 0]
    assert float(x[5]) == 7.0 - 2.0 ** -21 and np.nextafter(x[5], np.float32(8)) == np.float32(7.0)
    for diagonal in (False, True):
        for shift in ((0.0, 0.0, 0.0), ec.CULL_SHIFT):
            case = ec.cull_case(diagonal, shift)
            xyz = case[0].astype(np.float64)
            gap = np.linalg.norm(xyz[0:16].mean(0) - xyz[24:40].mean(0))
            assert abs(gap - 36.0) < 0.01                             # cutoff + both radii, to a few 1e-3
            for dtype in (np.float64, np.float32):
                assert ec.oracle(case, ec.CULL_C2, dtype)["cn_raw"].tolist() == [2, 1, 1, 2]
    for name, counts in ec.STAGING_COUNTS.items():
        case = ec.staging_case(counts)
        o64, o32 = ec.oracle(case), ec.oracle(case, dtype=np.float32)
        assert ec.same(o64, o32, amide=False) == [] and (o64["cn_raw"] == 2).all(), name
    c = ec.STAGING_COUNTS
    assert sum(c["two_chunks"]) > 2048 > sum(c["two_chunks"][:10]) and sum(c["two_chunks"][:11]) > 2048
    assert c["long_residue"][0] > 2048 and sum(c["tile_straddles"][:64]) > 2048 and len(c["tile_straddles"]) > 64


def test_minmax_scaler_equals_the_fp32_quotient_for_every_small_range():
    """The claim behind column 78: fp32 of sklearn's fp64 MinMaxScaler result IS the fp32 quotient."""
    from sklearn.preprocessing import MinMaxScaler
    for lo, hi in ((1, 2), (8, 36), (9, 38), (5, 109), (1, 4096), (3, 1000)):
        cn = np.arange(lo, hi + 1)
        ref = MinMaxScaler().fit_transform(cn.astype(np.float64).reshape(-1, 1)).reshape(-1).astype(np.float32)
        assert np.array_equal(ref, (cn - lo).astype(np.float32) / np.float32(hi - lo))


# ---- the fixture ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["l", "r"])
def test_4heq_fixture_equals_a_fresh_fp64_oracle_and_keeps_the_margins(tag):
    z = load_case("4heq_env")
    case = tuple(z[f"{tag}_{k}"] for k in ("xyz", "res_off", "role", "aa", "resname_idx"))
    assert case[0].shape == (1076, 3) and len(case[3]) == 145 and case[0].dtype == np.float32
    off, role = case[1], case[2]
    assert all(role[off[i]:off[i] + 4].tolist() == [1, 2, 3, 4] for i in range(145))
    o = ec.oracle(case)
    for k in ("cn_raw", "un", "dn", "hsaac", "cn", "onehot", "amide"):
        assert z[f"{tag}_{k}"].tobytes() == o[k].tobytes(), k
    assert (int(o["cn_raw"].min()), int(o["cn_raw"].max())) == {"l": (8, 36), "r": (9, 38)}[tag]
    rel, cos = ec.margins(case)
    assert rel > 1e-4 and cos > 1e-4, (rel, cos)
    o32 = ec.oracle(case, dtype=np.float32)
    assert ec.same(o, o32, amide=False) == []
    assert [ec.column_of(t) for t in case[3]] == case[4].tolist()
