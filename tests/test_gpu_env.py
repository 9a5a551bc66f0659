"""Structure-derived DIPS-Plus features on the GPU (csrc/residue_env.hip, structure.ResidueEnvOp,
builder.build_graph_batch_structures). Integers (cn_raw) and the HSAAC / CN / one-hot columns are compared
exactly -- they are fp32 quotients of integer counts -- with both oracles of tests/env_cases.py, the amide
normals and backbone rows bit for bit with the fp32 one; on the 4HEQ pair with the fixture
tests/golden/4heq_env.npz (the fp64 oracle, scipy + sklearn). The cases are built on the CPU in
tests/env_cases.py and checked there by tests/test_env_host.py, which also asserts the margins that make
the fp64 comparison leave nothing out."""
import ctypes

import numpy as np
import pytest
import torch

import env_cases as ec
from gpu_common import load_case

pytestmark = pytest.mark.gpu

OFFSETS = "residue env: residue offsets do not start at 0, decrease, or do not end at the atom count"
EMPTY = "residue env: a residue without atoms"
NONFINITE = "residue env: a NaN or Inf coordinate"
BACKBONE = "residue env: a role, aa or resname code out of range"


@pytest.fixture(scope="module")
def op():
    from deepinteract_amd.structure import ResidueEnvOp
    return ResidueEnvOp("cuda")


_REFS = {}


def refs(key, case, c2=ec.C2):
    """Both oracles of a case, computed once per module run."""
    if key not in _REFS:
        _REFS[key] = (ec.oracle(case, c2, np.float32), ec.oracle(case, c2, np.float64))
    return _REFS[key]


def run(op, cases, c2=ec.C2, extern=None):
    """The op over `cases` in ONE call: per chain a dict of numpy arrays."""
    res = op.features(cases, extern=extern, c2=c2)
    out = []
    for r, case in zip(res, cases):
        L = len(case[3])
        assert tuple(r["dips"].shape) == (L, 106) and tuple(r["amide_norm"].shape) == (L, 3)
        assert tuple(r["backbone"].shape) == (L, 4, 3) and tuple(r["cn_raw"].shape) == (L,)
        assert r["cn_raw"].dtype == torch.int32 and all(t.is_cuda for t in r.values())
        out.append({k: v.cpu().numpy() for k, v in r.items()})
    return out


def expect(got, o32, o64=None, extern=None):
    assert got["cn_raw"].tolist() == o32["cn_raw"].tolist()
    want = ec.dips_of(o32, extern)
    bad = np.argwhere(got["dips"].view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, bad[:8].tolist()
    assert got["amide_norm"].tobytes() == o32["amide"].tobytes()
    assert got["backbone"].tobytes() == o32["backbone"].tobytes()
    if o64 is not None:
        assert got["cn_raw"].tolist() == o64["cn_raw"].tolist()
        assert got["dips"][:, ec.OWN].tobytes() == ec.dips_of(o64)[:, ec.OWN].tobytes()


def test_one_residue(op):
    cases = [ec.single_case(aa) for aa in (0, 7, 20)]
    for got, case, aa in zip(run(op, cases), cases, (0, 7, 20)):
        assert got["cn_raw"].tolist() == [1]                          # CN = 1: UN = 0, DN = 1
        hs = got["dips"][0, 36:78]
        assert hs[aa] == 1.0 and hs[21 + aa] == 1.0 and hs.sum() == 2.0          # UC[aa] = 1 / 1, DC[aa] = 2 / 2
        assert got["dips"][0, 78] == 0.0                              # the range is zero
        assert got["dips"][0, :20].tolist() == np.eye(20)[ec.column_of(aa)].tolist()
        expect(got, *refs(("single", aa), case))


@pytest.mark.parametrize("L", ec.GRID_L)
def test_tile_tails_on_the_grid_exact_chain(op, L):
    case = ec.grid_case(L)
    o32, o64 = refs(("grid", L), case)
    got = run(op, [case])[0]
    expect(got, o32, o64)
    kinds = np.arange(L) % 7
    # u = 0 (kind 6): every neighbour is down, so UN = 0 and UC is the residue's own type alone, 1 / 1
    zero_u = np.flatnonzero(kinds == 6)
    assert (o64["un"][zero_u] == 0).all() and (got["dips"][zero_u, 36 + case[3][zero_u]] == 1.0).all()
    assert (got["amide_norm"][(kinds == 3) | (kinds == 5)] == 0).all()


def test_strict_boundary(op):
    cases = [ec.boundary_case(False), ec.boundary_case(True)]
    got = run(op, cases, c2=ec.BOUNDARY_C2)
    assert got[0]["cn_raw"].tolist() == [1, 1]                        # exactly 7 A: d2 == c2 is not < c2
    assert got[1]["cn_raw"].tolist() == [2, 2]                        # 7 - 2^-21 A
    for g, c, inside in zip(got, cases, (False, True)):
        expect(g, *refs(("boundary", inside), c, ec.BOUNDARY_C2))


@pytest.mark.parametrize("shift", [(0.0, 0.0, 0.0), ec.CULL_SHIFT], ids=["origin", "shifted_9000"])
@pytest.mark.parametrize("diagonal", [False, True], ids=["axis", "diagonal"])
def test_the_cull_keeps_spheres_that_touch_at_the_cutoff(op, diagonal, shift):
    case = ec.cull_case(diagonal, shift)
    o32, o64 = refs(("cull", diagonal, shift), case, ec.CULL_C2)
    got = run(op, [case], c2=ec.CULL_C2)[0]
    assert got["cn_raw"].tolist() == [2, 1, 1, 2]
    expect(got, o32, o64 if not diagonal else None)


@pytest.mark.parametrize("name", list(ec.STAGING_COUNTS))
def test_atom_counts_across_the_staging_boundaries(op, name):
    case = ec.staging_case(ec.STAGING_COUNTS[name])
    got = run(op, [case])[0]
    assert (got["cn_raw"] == 2).all()
    expect(got, *refs(("staging", name), case))


@pytest.mark.parametrize("seed,L", ec.RANDOM)
def test_random_float_chains_equal_both_oracles(op, seed, L):
    case = ec.random_case(seed, L)
    expect(run(op, [case])[0], *refs(("random", seed, L), case))


def fixture_chain(z, tag):
    return tuple(z[f"{tag}_{k}"] for k in ("xyz", "res_off", "role", "aa", "resname_idx"))


def test_4heq_equals_the_fixture(op):
    z = load_case("4heq_env")
    cases = [fixture_chain(z, "l"), fixture_chain(z, "r")]
    for got, case, tag in zip(run(op, cases), cases, ("l", "r")):
        assert got["cn_raw"].tobytes() == z[f"{tag}_cn_raw"].tobytes()
        assert got["dips"][:, 0:20].tobytes() == z[f"{tag}_onehot"].tobytes()
        assert got["dips"][:, 36:78].tobytes() == z[f"{tag}_hsaac"].tobytes()
        assert got["dips"][:, 78].tobytes() == z[f"{tag}_cn"].tobytes()
        assert (got["dips"][:, ec.EXTERN] == 0).all()
        # fp32 cross products of differences of a few A: 6 roundings of products below 8 A^2
        assert np.abs(got["amide_norm"] - z[f"{tag}_amide"]).max() < 1e-5
        expect(got, *refs(("4heq", tag), case))


def _ragged():
    return [ec.single_case(3), ec.grid_case(17), ec.random_case(*ec.RANDOM[0]),
            ec.staging_case(ec.STAGING_COUNTS["lanes"]), ec.grid_case(65)]


def _bytes(res):
    return [{k: v.tobytes() for k, v in r.items()} for r in res]


def test_ragged_batch_gives_each_chain_the_bytes_it_gets_alone(op):
    cases = _ragged()
    together = _bytes(run(op, cases))
    for k, case in enumerate(cases):
        assert _bytes(run(op, [case]))[0] == together[k], k
    # host and device inputs give the same bytes (the second chain stays on the host: a mixed call)
    dev = [tuple(torch.as_tensor(a).cuda() for a in c) if k != 1 else c for k, c in enumerate(cases)]
    assert _bytes(run(op, dev)) == together


def test_more_chains_than_one_call_takes(op):
    from deepinteract_amd import _lib
    n = _lib.DI_BATCH_MAX + 1
    cases = [ec.single_case(i % 21) for i in range(n)]
    got = run(op, cases)
    want = {aa: ec.dips_of(ec.oracle(ec.single_case(aa), dtype=np.float32)) for aa in range(21)}
    for i, g in enumerate(got):
        assert g["cn_raw"].tolist() == [1] and g["dips"].tobytes() == want[i % 21].tobytes(), i


def test_extern_columns_arrive_untouched_and_own_columns_ignore_them(op):
    cases = [ec.grid_case(17), ec.random_case(*ec.RANDOM[0]), ec.single_case(5)]
    rng = np.random.default_rng(3)
    ext = [rng.normal(size=(len(c[3]), 106)).astype(np.float32) for c in cases]
    ext[0][:, ec.OWN] = np.nan                                        # what it holds there is ignored
    for extern in ([ext[0], torch.as_tensor(ext[1]).cuda(), None], [ext[0], ext[1], None]):
        got = run(op, cases, extern=extern)
        for g, e, c, key in zip(got, (ext[0], ext[1], None), cases,
                                (("grid", 17), ("random",) + ec.RANDOM[0], ("single", 5))):
            o32, _ = refs(key, c)
            expect(g, o32, extern=e)
            want = np.zeros((len(c[3]), 43), np.float32) if e is None else e[:, ec.EXTERN]
            assert g["dips"][:, ec.EXTERN].tobytes() == want.tobytes()


def _broken(kind):
    xyz, off, role, aa, col = (a.copy() for a in ec.grid_case(17))
    if kind == "offsets":
        off[3] = off[2] - 1
    elif kind == "end":
        off[-1] += 1
    elif kind == "empty":
        off[3] = off[2]                    # residue 2 loses its atoms to nobody: still non-decreasing
    elif kind == "nan":
        xyz[7, 1] = np.nan
    elif kind == "inf":
        xyz[0, 0] = np.inf
    elif kind == "role":
        role[5] = 6
    elif kind == "two_ca":
        role[off[4]] = ec.CA               # the N of residue 4 becomes a second CA
    elif kind == "two_cb":
        role[off[6] + 5] = ec.CB           # residue 6 (kind 6) has a CB and another side atom
    elif kind == "aa":
        aa[2] = 21
    elif kind == "resname":
        col[16] = 20
    elif kind == "nan_and_role":
        xyz[7, 1], role[5] = np.nan, 6
    elif kind == "empty_and_nan":
        off[3], xyz[0, 0] = off[2], np.nan
    return xyz, off, role, aa, col


@pytest.mark.parametrize("kind,message", [
    ("offsets", OFFSETS), ("end", OFFSETS), ("empty", EMPTY), ("nan", NONFINITE), ("inf", NONFINITE),
    ("role", BACKBONE), ("two_ca", BACKBONE), ("two_cb", BACKBONE), ("aa", BACKBONE), ("resname", BACKBONE),
    ("nan_and_role", NONFINITE), ("empty_and_nan", EMPTY)])
def test_each_flag_raises_its_message_in_the_documented_order(op, kind, message):
    with pytest.raises(ValueError) as err:
        op.features([ec.single_case(1), _broken(kind)])
    assert str(err.value).startswith(message)


def test_bad_arguments_raise_before_any_launch(op):
    good = ec.single_case(1)
    for c2 in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError, match="c2"):
            op.features([good], c2=c2)
    with pytest.raises(ValueError, match="non-empty list"):
        op.features([])
    with pytest.raises(ValueError, match="a chain is"):
        op.features([good[:4]])
    with pytest.raises(ValueError, match="a chain is"):
        op.features([(good[0].reshape(-1), *good[1:])])
    with pytest.raises(ValueError, match=r"role is \[A\]"):
        op.features([(good[0], good[1], good[2][:-1], good[3], good[4])])
    with pytest.raises(ValueError, match="extern"):
        op.features([good], extern=[np.zeros((1, 105), np.float32)])
    with pytest.raises(ValueError, match="extern arrays"):
        op.features([good], extern=[None, None])
    with pytest.raises(ValueError, match="tensor on cpu"):
        op.features([tuple(torch.as_tensor(a) for a in good)])


def test_the_c_call_flags_one_chain_and_leaves_its_neighbours_correct():
    from deepinteract_amd import _lib
    lib = _lib.load()
    cases = [ec.grid_case(17), _broken("two_ca"), ec.grid_case(65)]
    keep, items = [], (_lib.DiEnvItem * 3)()
    outs = []
    for it, c in zip(items, cases):
        L, A = len(c[3]), c[0].shape[0]
        dev = [torch.as_tensor(a).cuda() for a in c]
        out = [torch.zeros(L, 106, device="cuda"), torch.empty(L, 3, device="cuda"),
               torch.empty(L, 4, 3, device="cuda"), torch.empty(L, dtype=torch.int32, device="cuda")]
        keep += dev + out
        outs.append(out)
        it.xyz, it.res_off, it.role, it.aa, it.resname = (t.data_ptr() for t in dev)
        it.dips, it.amide_norm, it.backbone, it.cn_raw = (t.data_ptr() for t in out)
        it.l, it.a = L, A
    nb = lib.di_residue_env_work_bytes(items, 3)
    assert nb == 3 * 16 + 48 * (17 + 17 + 65)
    work = torch.empty(nb // 8, dtype=torch.int64, device="cuda")
    table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).cuda()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.di_residue_env_batch(items, ctypes.c_void_p(table.data_ptr()), 3, ctypes.c_float(ec.C2),
                                    ctypes.c_void_p(work.data_ptr()), stream) == 0
    stats = work[:6].cpu().numpy().view(np.int32).reshape(3, 4)
    assert stats[:, 0].tolist() == [0, _lib.DI_ENV_BACKBONE, 0]
    for k, key in ((0, ("grid", 17)), (2, ("grid", 65))):
        o32, o64 = refs(key, cases[k])
        got = dict(zip(("dips", "amide_norm", "backbone", "cn_raw"), (t.cpu().numpy() for t in outs[k])))
        expect(got, o32, o64)
        assert stats[k, 1] == o64["cn_raw"].max() and stats[k, 2] == len(cases[k][3]) - o64["cn_raw"].min()


def test_end_to_end_graph_batch_from_the_4heq_structures():
    """build_graph_batch_structures on the fixture: the structure-derived node-feature columns equal the
    fixture, and EVERY tensor of the batch is bit-identical to build_graph_batch fed with the op's own
    dips, amide_norm and backbone copied to the host; model.predict_batch runs on it."""
    import plain_cases as P
    from deepinteract_amd.builder import build_graph_batch, build_graph_batch_structures
    from deepinteract_amd.modules import LitGINI
    from deepinteract_amd.weights import seeded_state_dict
    z = load_case("4heq_env")
    cases = [fixture_chain(z, "l"), fixture_chain(z, "r")]
    rng = np.random.default_rng(9)
    ext = [rng.random((145, 106)).astype(np.float32) for _ in cases]
    gb, aux = build_graph_batch_structures(cases, extern=ext, nbr_seeds=[5, 6], return_aux=True)
    node_f = gb.node_f.cpu().numpy()
    assert node_f.shape == (290, 113) and gb.nodes_per_graph == [145, 145]
    for g, tag in enumerate(("l", "r")):
        rows = node_f[145 * g:145 * (g + 1)]
        assert rows[:, 7:27].tobytes() == z[f"{tag}_onehot"].tobytes()
        assert rows[:, 43:85].tobytes() == z[f"{tag}_hsaac"].tobytes()
        assert rows[:, 85].tobytes() == z[f"{tag}_cn"].tobytes()
        assert rows[:, 7 + ec.EXTERN].tobytes() == ext[g][:, ec.EXTERN].tobytes()
    host = [{"backbone": e["backbone"].cpu().numpy(), "amide_norm": e["amide_norm"].cpu().numpy(),
             "dips": e["dips"].cpu().numpy()} for e in aux["env"]]
    gb2, aux2 = build_graph_batch(host, nbr_seeds=[5, 6], return_aux=True)
    for name in ("src", "dst", "nbr", "node_f", "edge_f", "in_ptr", "node_pos"):
        assert torch.equal(getattr(gb, name), getattr(gb2, name)), name
    assert torch.equal(aux["knn_idx"], aux2["knn_idx"]) and torch.equal(aux["knn_d2"], aux2["knn_d2"])
    assert gb.geo_ref == gb2.geo_ref and gb.edges_per_graph == gb2.edges_per_graph
    # the counter-based neighbour ids too
    assert torch.equal(build_graph_batch_structures(cases, extern=ext, seed=3).nbr, build_graph_batch(host, seed=3).nbr)
    cfg = P.plain_cfg(2, num_interact_layers=1)
    model = LitGINI(disable_geometric_mode=True, num_interact_layers=1, dtype="f32").cuda().eval()
    model.load_reference_state_dict(seeded_state_dict(0, cfg))
    with torch.no_grad():
        logits, probs = model.predict_batch(gb, [(0, 1)])
        logits2, _ = model.predict_batch(gb2, [(0, 1)])
    torch.cuda.synchronize()
    assert tuple(probs[0].shape) == (145, 145) and bool(torch.isfinite(logits[0]).all())
    assert torch.equal(logits[0], logits2[0])
    with pytest.raises(ValueError, match="fewer than k"):
        build_graph_batch_structures([ec.grid_case(17)])
    with pytest.raises(ValueError, match="neighbour seeds"):
        build_graph_batch_structures(cases, nbr_seeds=[1])
