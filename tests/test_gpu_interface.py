"""Interface label maps from atom coordinates on the GPU (csrc/contact_interface.hip,
ranking.InterfaceOp). Every map is compared byte for byte with tests/interface_cases.ref_labels_f32 -- numpy
brute force over every atom pair in the kernel's stated fp32 operation order -- and num_pos with its sum;
where fp32 is exact or nothing is near the boundary, also with the fp64 brute force, and on the 4HEQ pair
with the cKDTree labels stored in tests/golden/4heq_interface.npz. The cases are built on the CPU in
tests/interface_cases.py and checked there by tests/test_interface_host.py."""
import ctypes

import numpy as np
import pytest
import torch

import interface_cases as ic
from gpu_common import load_case

pytestmark = pytest.mark.gpu

OFFSETS = "interface: residue offsets do not start at 0, decrease, or do not end at the atom count"
EMPTY = "interface: a residue without atoms"
NONFINITE = "interface: a NaN or Inf coordinate"


@pytest.fixture(scope="module")
def op():
    from deepinteract_amd.ranking import InterfaceOp
    return InterfaceOp("cuda")


def run(op, cases, cutoff=6.0):
    """The op over `cases` in ONE call: its maps as [l1, l2] numpy arrays, and num_pos."""
    maps = op.labels([c[0] for c in cases], [c[1] for c in cases], cutoff=cutoff)
    out = []
    for m, (c0, c1) in zip(maps, cases):
        assert m.dtype == torch.uint8 and m.is_cuda and m.numel() == (len(c0[1]) - 1) * (len(c1[1]) - 1)
        assert m.data_ptr() % 16 == 0
        out.append(m.cpu().numpy().reshape(len(c0[1]) - 1, len(c1[1]) - 1))
    return out, list(op.num_pos)


def same_as_f32(op, cases):
    got, num_pos = run(op, cases)
    refs = [ic.ref_labels_f32(*c) for c in cases]
    for k, (g, r) in enumerate(zip(got, refs)):
        assert g.tobytes() == r.tobytes(), (k, np.argwhere(g != r)[:8].tolist())
    assert num_pos == [int(r.sum()) for r in refs]
    return got, refs


def test_boundary_is_inclusive_to_the_last_fp32_step(op):
    got, _ = same_as_f32(op, [ic.boundary_case(False), ic.boundary_case(True)])
    assert got[0].tolist() == [[1]] and got[1].tolist() == [[0]]


def test_the_sum_is_not_contracted(op):
    triples = ic.contraction_triples()
    got, _ = same_as_f32(op, [ic.contraction_case(t) for t in triples])
    for g, t in zip(got, triples):
        unfused, fused = ic.unfused_d2(t) <= np.float32(36), ic.fused_d2(t) <= np.float32(36)
        assert unfused != fused and int(g[0, 0]) == int(unfused), (t, g)


def test_ragged_shapes_every_row_alignment(op):
    cases = [ic.cloud_case(1000 * l1 + l2, l1, l2) for l1, l2 in ic.RAGGED_SHAPES]
    _, refs = same_as_f32(op, cases)
    assert all(r.sum() > 0 for r in refs)


@pytest.mark.parametrize("counts", ic.STAGING_COUNTS, ids=["one_chunk", "two_chunks"])
def test_atom_counts_across_the_staging_boundaries(op, counts):
    got, _ = same_as_f32(op, [ic.staging_case(counts)])
    assert np.array_equal(got[0], np.eye(len(counts), dtype=np.uint8))


@pytest.mark.parametrize("shift", [(0.0, 0.0, 0.0), ic.CULL_SHIFT], ids=["origin", "shifted_9000"])
@pytest.mark.parametrize("diagonal", [False, True], ids=["axis", "diagonal"])
def test_the_cull_keeps_spheres_that_touch_at_the_cutoff(op, diagonal, shift):
    case = ic.cull_case(diagonal, shift)
    got, _ = same_as_f32(op, [case])
    if not diagonal:
        assert got[0].tolist() == [[0, 1], [1, 0]]


def test_grid_exact_case_equals_fp64_ties_included(op):
    case = ic.grid_exact_case()
    got, _ = same_as_f32(op, [case])
    assert got[0].shape == (97, 131) and got[0].tobytes() == ic.ref_labels_f64(*case).tobytes()
    assert got[0][0, 0] == 1 and got[0][1, 1] == 1          # the exact ties


@pytest.mark.parametrize("seed,l1,l2", ic.RANDOM_FLOAT)
def test_random_float_case_equals_fp32_and_fp64(op, seed, l1, l2):
    case = ic.random_float_case(seed, l1, l2)
    got, _ = same_as_f32(op, [case])
    skip = ic.ambiguous(*case)              # proved empty on the CPU: nothing is excluded
    assert len(skip) == 0
    assert got[0].tobytes() == ic.ref_labels_f64(*case).tobytes()


def heq():
    z = load_case("4heq_interface")
    return ((z["xyz0"], z["res_off0"]), (z["xyz1"], z["res_off1"])), z["labels"]


def test_4heq_equals_the_kdtree_labels(op):
    case, want = heq()
    got, num_pos = run(op, [case])
    assert got[0].tobytes() == want.tobytes() and num_pos == [80]


def five_cases():
    return [ic.cloud_case(41, 24, 31), ic.staging_case(ic.STAGING_COUNTS[0]), heq()[0], ic.cloud_case(42, 1, 70),
            ic.grid_exact_case(9, 50, 17)]


def test_batch_gives_the_bytes_each_complex_gives_alone(op):
    cases = five_cases()
    together, num_pos = run(op, cases)
    for k, c in enumerate(cases):
        alone, n = run(op, [c])
        assert alone[0].tobytes() == together[k].tobytes() and n == [num_pos[k]]
        assert alone[0].tobytes() == ic.ref_labels_f32(*c).tobytes()


def test_1025_complexes_go_through_the_chunking(op):
    from deepinteract_amd import _lib
    rng = np.random.default_rng(3)
    n = _lib.DI_BATCH_MAX + 1
    cases = []
    for _ in range(n):
        a, b = rng.integers(1, 4, size=2)
        cases.append((ic.chain(rng.normal(scale=2.5, size=(a, 3)), [a]),
                      ic.chain(rng.normal(scale=2.5, size=(b, 3)) + (4.0, 0.0, 0.0), [b])))
    got, num_pos = run(op, cases)
    want = [int(ic.ref_labels_f32(*c)[0, 0]) for c in cases]
    assert [int(g[0, 0]) for g in got] == want == num_pos
    assert 0 < sum(want) < n and want[-1] == num_pos[-1]


def test_host_and_device_inputs_give_the_same_bytes(op):
    cases = five_cases()[:3]
    host, n_host = run(op, cases)
    dev = [tuple((torch.from_numpy(x).cuda(), torch.from_numpy(o).cuda()) for x, o in c) for c in cases]
    maps = op.labels([c[0] for c in dev], [c[1] for c in dev])
    assert [m.cpu().numpy().tobytes() for m in maps] == [h.tobytes() for h in host] and op.num_pos == n_host
    # mixed: one chain from the host, the other on the device; fp64 / int64 inputs are converted
    mixed = op.labels([(cases[0][0][0].astype(np.float64), cases[0][0][1].astype(np.int64))], [dev[0][1]])
    assert mixed[0].cpu().numpy().tobytes() == host[0].tobytes()


def test_another_cutoff(op):
    case = ic.cloud_case(77, 40, 33)
    for cutoff in (3.0, 8.5):
        got, num_pos = run(op, [case], cutoff=cutoff)
        ref = ic.ref_labels_f32(*case, cutoff=cutoff)
        assert got[0].tobytes() == ref.tobytes() and num_pos == [int(ref.sum())]


# ---- flags and refusals -------------------------------------------------------------------------------
def broken(kind):
    (x0, o0), (x1, o1) = ic.cloud_case(55, 9, 12, amin=2)
    x1, o1 = x1.copy(), o1.copy()
    if kind == "decreasing":
        o1[5] = o1[4] - 1
    elif kind == "first":
        o1[0] = 1
    elif kind == "last":
        o1[-1] -= 1
    elif kind == "beyond":
        o1[-1] += 1000                  # clamped into [0, A]: nothing outside xyz is read
    elif kind == "negative":
        o1[3] = -7
    elif kind == "empty":
        o1[5] = o1[4]
    elif kind == "nan":
        x1[7, 1] = np.nan
    elif kind == "inf":
        x1[0, 2] = -np.inf
    return (x0, o0), (x1, o1)


@pytest.mark.parametrize("kind,text", [("decreasing", OFFSETS), ("first", OFFSETS), ("last", OFFSETS),
                                       ("beyond", OFFSETS), ("negative", OFFSETS), ("empty", EMPTY),
                                       ("nan", NONFINITE), ("inf", NONFINITE)])
def test_flagged_complexes_raise(op, kind, text):
    good = ic.cloud_case(56, 5, 6)
    with pytest.raises(ValueError) as e:
        run(op, [good, broken(kind), good])
    assert str(e.value) == text
    # chain 0 is checked like chain 1
    c0, c1 = broken(kind)
    with pytest.raises(ValueError) as e:
        run(op, [(c1, c0)])
    assert str(e.value) == text


def test_flags_in_order_offsets_empty_nonfinite(op):
    (x0, o0), (x1, o1) = broken("empty")
    x1[0, 0] = np.nan
    with pytest.raises(ValueError) as e:
        run(op, [((x0, o0), (x1, o1))])
    assert str(e.value) == EMPTY
    o1[-1] -= 1
    with pytest.raises(ValueError) as e:
        run(op, [((x0, o0), (x1, o1))])
    assert str(e.value) == OFFSETS


def test_python_refusals_before_any_launch(op):
    c0, c1 = ic.cloud_case(57, 4, 5)
    for cutoff in (0.0, -1.0, float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="cutoff"):
            op.labels([c0], [c1], cutoff=cutoff)
    with pytest.raises(ValueError, match="of one length"):
        op.labels([c0], [c1, c1])
    with pytest.raises(ValueError, match="of one length"):
        op.labels([], [])
    with pytest.raises(ValueError, match=r"xyz \[A, 3\]"):
        op.labels([(c0[0][:, :2], c0[1])], [c1])
    with pytest.raises(ValueError, match="at least one residue"):
        op.labels([(c0[0], c0[1][:1])], [c1])
    with pytest.raises(ValueError, match="the kernels run on"):
        op.labels([(torch.from_numpy(c0[0]), torch.from_numpy(c0[1]))], [c1])      # a CPU tensor
    from deepinteract_amd.ranking import InterfaceOp
    with pytest.raises(RuntimeError):
        InterfaceOp("cpu")


def test_c_batch_flags_one_complex_and_leaves_its_neighbours_correct():
    """The C entry point directly: stats per complex, a flagged complex between two good ones."""
    from deepinteract_amd import _lib
    lib = _lib.load()
    cases = [ic.cloud_case(61, 20, 70), broken("decreasing"), broken("nan"), broken("empty"), ic.cloud_case(62, 33, 5)]
    dev, items = [], (_lib.DiInterfaceItem * len(cases))()
    for it, ((x0, o0), (x1, o1)) in zip(items, cases):
        t = [torch.from_numpy(a).cuda() for a in (x0, o0, x1, o1)]
        l1, l2 = len(o0) - 1, len(o1) - 1
        out = torch.full((l1 * l2 + 32,), 0xAB, dtype=torch.uint8, device="cuda")      # 16 guard bytes either side
        dev.append((t, out))
        it.xyz0, it.res_off0, it.xyz1, it.res_off1 = (a.data_ptr() for a in t)
        it.labels, it.l1, it.l2, it.a0, it.a1 = out.data_ptr() + 16, l1, l2, len(x0), len(x1)
    nb = lib.di_interface_work_bytes(items, len(cases))
    assert nb > 0
    work = torch.empty(nb // 8, dtype=torch.int64, device="cuda")
    table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).cuda()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):          # a second call on the same workspace: the stats are cleared, not added to
        rc = lib.di_interface_labels_batch(items, ctypes.c_void_p(table.data_ptr()), len(cases), ctypes.c_float(6.0),
                                           ctypes.c_void_p(work.data_ptr()), stream)
        assert rc == 0
    stats = work[:2 * len(cases)].cpu().view(len(cases), 2).tolist()
    flags = [w & 0xffffffff for _, w in stats]
    assert flags == [0, _lib.DI_IF_OFFSETS, _lib.DI_IF_NONFINITE, _lib.DI_IF_EMPTY, 0]
    for k, ((t, out), c) in enumerate(zip(dev, cases)):
        host = out.cpu().numpy()
        assert (host[:16] == 0xAB).all() and (host[-16:] == 0xAB).all(), k       # every write inside the map
        if flags[k] == 0:
            ref = ic.ref_labels_f32(*c)
            assert host[16:-16].tobytes() == ref.tobytes() and stats[k][0] == int(ref.sum())
        else:
            assert set(np.unique(host[16:-16]).tolist()) <= {0, 1}              # written, whatever it says
