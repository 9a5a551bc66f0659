"""Shared by the residue-environment tests (not collected): two numpy oracles of the definitions in
include/deepinteract_amd.h (di_residue_env_batch) and the seeded cases the CPU and GPU tests both use.

A chain is ``(xyz float32 [A, 3], res_off int32 [L + 1], role uint8 [A], aa uint8 [L], resname_idx uint8
[L])``, what ``structure.residue_atoms`` returns. The codes are restated here, not imported.

* ``oracle(chain, c2, np.float64)``: atom-pair squared distances from scipy's ``cdist(..., "sqeuclidean")``,
  neighbours iff d2 < c2, side-chain vectors and half-sphere tests in fp64, CN normalised by sklearn's
  ``MinMaxScaler`` and rounded to fp32 once.
* ``oracle(chain, c2, np.float32)``: d2 = (dx * dx + dy * dy) + dz * dz in fp32 in exactly the kernel's
  order (numpy rounds every elementwise operation on its own and never fuses two), the amide normal the
  same way -- both to the bit -- and the side-chain vectors in fp32.
* ``margins``: how far the case is from any decision fp32 could flip: the smallest |d2 - c2| / c2 over the
  residue pairs (d2 = the pair's smallest atom-pair value) and the smallest |cos| over the half-sphere
  tests, in fp64.

All counts are integers; given equal counts every output is determined to the bit: HSAAC and CN are fp32
quotients of two integers.
"""
import numpy as np

AA = "ACDEFGHIKLMNPQRSTVWY-"
ONE_HOT = ["TRP", "PHE", "LYS", "PRO", "ASP", "ALA", "ARG", "CYS", "VAL", "THR",
           "GLY", "SER", "HIS", "LEU", "GLU", "TYR", "ILE", "ASN", "MET", "GLN"]
THREE = {"A": "ALA", "C": "CYS", "D": "ASP", "E": "GLU", "F": "PHE", "G": "GLY", "H": "HIS", "I": "ILE", "K": "LYS",
         "L": "LEU", "M": "MET", "N": "ASN", "P": "PRO", "Q": "GLN", "R": "ARG", "S": "SER", "T": "THR", "V": "VAL",
         "W": "TRP", "Y": "TYR", "-": "UNK"}
OTHER, N, CA, C, O, CB = range(6)
C2 = float(np.float32(8.0 * np.log(1000.0)))          # 55.262043f, the default
OWN = np.r_[0:20, 36:79]
EXTERN = np.r_[20:36, 79:106]


def column_of(aa):
    """The one-hot column of an aa code: an unknown residue goes to the last bin (GLN)."""
    name = THREE[AA[aa]]
    return ONE_HOT.index(name) if name in ONE_HOT else len(ONE_HOT) - 1


def chain(xyz, counts, role, aa):
    counts = np.asarray(counts, dtype=np.int64)
    xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float64).reshape(-1, 3), dtype=np.float32)
    role = np.asarray(role, dtype=np.uint8)
    aa = np.asarray(aa, dtype=np.uint8)
    assert counts.sum() == xyz.shape[0] == role.shape[0] and len(aa) == len(counts)
    off = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    return xyz, off, role, aa, np.array([column_of(t) for t in aa], dtype=np.uint8)


# ---- the oracles --------------------------------------------------------------------------------------
def _pair_d2(x, dtype):
    if dtype == np.float64:
        from scipy.spatial.distance import cdist
        x = x.astype(np.float64)
        return cdist(x, x, "sqeuclidean")
    dx = x[:, None, 0] - x[None, :, 0]
    dy = x[:, None, 1] - x[None, :, 1]
    dz = x[:, None, 2] - x[None, :, 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == np.float32
    return d2


def _per_residue(mask, off, reduce=np.logical_or):
    off = np.asarray(off, dtype=np.int64)
    return reduce.reduceat(reduce.reduceat(mask, off[:-1], axis=0), off[:-1], axis=1)


def _unit(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def geometry(chain, dtype):
    """(ca [L, 3], u [L, 3], amide [L, 3], backbone [L, 4, 3]) in `dtype`."""
    xyz, off, role = chain[0].astype(dtype), chain[1], chain[2]
    L = len(off) - 1
    ca, u = np.zeros((L, 3), dtype), np.zeros((L, 3), dtype)
    amide, bb = np.zeros((L, 3), dtype), np.zeros((L, 4, 3), dtype)
    for i in range(L):
        at, r = xyz[off[i]:off[i + 1]], role[off[i]:off[i + 1]]
        for q in (N, CA, C, O):
            assert (r == q).sum() == 1
            bb[i, q - 1] = at[r == q][0]
        ca[i] = bb[i, 1]
        side = at[(r == OTHER) | (r == CB)]
        if len(side):
            u[i] = _unit(side - ca[i]).sum(axis=0) / dtype(len(side))
        else:
            u[i] = dtype(0.5) * (_unit(ca[i] - bb[i, 2]) + _unit(ca[i] - bb[i, 0]))
        if (r == CB).sum() == 1:
            cb = at[r == CB][0]
            a, b = ca[i] - cb, cb - bb[i, 0]
            amide[i] = (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
    assert u.dtype == dtype and amide.dtype == dtype
    return ca, u, amide, bb


def oracle(chain, c2=C2, dtype=np.float64):
    xyz, off, role, aa, col = chain
    L = len(off) - 1
    with np.errstate(invalid="ignore", over="ignore"):
        nb = _per_residue(_pair_d2(xyz, dtype) < dtype(c2), off)
    np.fill_diagonal(nb, True)
    ca, u, amide, bb = geometry(chain, dtype)
    with np.errstate(invalid="ignore"):
        dots = ((ca[None, :, :] - ca[:, None, :]) * u[:, None, :]).sum(axis=2)
        up = nb & ~np.eye(L, dtype=bool) & (dots > 0)
    down = nb & ~up                                    # self included
    kind = np.eye(21, dtype=np.int64)[aa]              # [L, 21]
    up_c, down_c = up.astype(np.int64) @ kind, down.astype(np.int64) @ kind
    un, dn = up.sum(axis=1), down.sum(axis=1)
    cn = nb.sum(axis=1)
    num = np.concatenate((up_c + kind, down_c + kind), axis=1)
    den = np.concatenate((np.repeat(1 + un[:, None], 21, 1), np.repeat(1 + dn[:, None], 21, 1)), axis=1)
    if dtype == np.float64:
        from sklearn.preprocessing import MinMaxScaler
        hsaac = (num.astype(np.float64) / den.astype(np.float64)).astype(np.float32)
        cn_n = MinMaxScaler().fit_transform(cn.astype(np.float64).reshape(-1, 1)).reshape(-1).astype(np.float32)
    else:
        hsaac = num.astype(np.float32) / den.astype(np.float32)
        rng = np.float32(cn.max() - cn.min())
        cn_n = (cn - cn.min()).astype(np.float32) / rng if rng else np.zeros(L, np.float32)
    onehot = np.eye(20, dtype=np.float32)[col]
    return {"cn_raw": cn.astype(np.int32), "un": un.astype(np.int32), "dn": dn.astype(np.int32),
            "up": up_c.astype(np.int32), "down": down_c.astype(np.int32), "hsaac": hsaac, "cn": cn_n,
            "onehot": onehot, "amide": amide.astype(np.float32), "backbone": bb.astype(np.float32)}


INTEGERS = ("cn_raw", "un", "dn", "up", "down")


def same(a, b, amide=True):
    """The fields in which two oracle results differ (amide normals compared bit for bit where asked)."""
    bad = [k for k in INTEGERS + ("hsaac", "cn", "onehot", "backbone") if a[k].tobytes() != b[k].tobytes()]
    if amide and a["amide"].tobytes() != b["amide"].tobytes():
        bad.append("amide")
    return bad


def dips_of(o, extern=None):
    """The op's dips [L, 106] from an oracle result: its own columns, `extern` (or zeros) in the others."""
    L = len(o["cn_raw"])
    d = np.zeros((L, 106), np.float32) if extern is None else np.array(extern, dtype=np.float32)
    d[:, 0:20], d[:, 36:78], d[:, 78] = o["onehot"], o["hsaac"], o["cn"]
    return d


def margins(chain, c2=C2):
    """(the smallest |d2(i, j) - c2| / c2 over the residue pairs, d2(i, j) the smallest squared distance
    between an atom of i and an atom of j -- the quantity the neighbour decision compares; the smallest
    |cos| over the half-sphere tests of neighbours j != i), in fp64. fp32 rounding moves a d2 by a few
    1e-7 relative and a cosine by about as much, so a case whose margins are above 1e-4 and 1e-5 has no
    decision fp32 could flip. A zero or NaN side-chain vector gives cos = NaN and is left out (such a
    residue is all down in every arithmetic)."""
    xyz, off = chain[0], chain[1]
    d2 = _per_residue(_pair_d2(xyz, np.float64), off, np.minimum)
    rel = float((np.abs(d2 - c2) / c2).min())
    nb = (d2 < c2) & ~np.eye(len(off) - 1, dtype=bool)
    ca, u, _, _ = geometry(chain, np.float64)
    v = ca[None, :, :] - ca[:, None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        cos = (v * u[:, None, :]).sum(axis=2) / (np.linalg.norm(v, axis=2) * np.linalg.norm(u, axis=1)[:, None])
    cos = np.abs(cos[nb])
    cos = cos[~np.isnan(cos)]
    return rel, float(cos.min()) if len(cos) else 1.0


# ---- one residue ---------------------------------------------------------------------------------------
def single_case(aa=7):
    xyz = [[0.0, 1.4, 0.0], [0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [2.0, 1.0, 0.0], [-0.5, -0.8, -1.2]]
    return chain(xyz, [5], [N, CA, C, O, CB], [aa])


# ---- grid-exact chains at the tile tails ------------------------------------------------------------------
GRID_L = [15, 16, 17, 63, 64, 65, 129]
_AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])


def grid_case(L):
    """Residue r's CA on a 4 x 4 x n integer grid of spacing 3; C = CA + x, N = CA + y, O = CA - z; one
    side atom on an axis (r % 6) at distance 1 or 2, so every unit vector, u and dot product is exact in
    fp32 and dots with grid neighbours across the axis are exactly 0 (down). r % 7 == 3: Gly (no side
    atom, u = -(x + y) / 2); r % 7 == 5: the side atom is not a CB (amide normal 0); r % 7 == 6: a CB at
    +axis * 1 and another atom at -axis * 2, whose unit vectors cancel (u = 0: everything down)."""
    xyz, counts, role, aa = [], [], [], []
    for r in range(L):
        ca = 3 * np.array([r % 4, (r // 4) % 4, r // 16])
        at, ro = [ca + (0, 1, 0), ca, ca + (1, 0, 0), ca - (0, 0, 1)], [N, CA, C, O]
        ax, kind = _AXES[r % 6], r % 7
        if kind == 6:
            at += [ca + ax, ca - 2 * ax]
            ro += [CB, OTHER]
        elif kind != 3:
            at.append(ca + (1 + r % 2) * ax)
            ro.append(OTHER if kind == 5 else CB)
        xyz += at
        role += ro
        counts.append(len(at))
        aa.append(r % 21)
    return chain(xyz, counts, role, aa)


# ---- the strict boundary ---------------------------------------------------------------------------------
BOUNDARY_C2 = 49.0


def boundary_case(inside: bool):
    """Two residues on the x axis whose closest atoms are exactly 7 A apart (d2 == 49: NOT neighbours under
    the strict test with c2 = 49) or 7 - 2^-21 A, one fp32 step of the coordinate less (neighbours)."""
    x1 = 7.0 - 2.0 ** -21 if inside else 7.0
    xs = [-1.0, 0.0, -2.0, -3.0, x1 + 1.0, x1, x1 + 2.0, x1 + 3.0]
    return chain([[x, 0.0, 0.0] for x in xs], [4, 4], [N, CA, C, O] * 2, [0, 19])


# ---- cull soundness --------------------------------------------------------------------------------------
CULL_C2 = 36.0
CULL_SHIFT = (9000.0, -9000.0, 9000.0)      # fp32 spacing 2^-10 A


def cull_case(diagonal: bool, shift=(0.0, 0.0, 0.0)):
    """Two residues of 16 atoms each on a 30 A line (2 A apart), end to end on one axis, 6 - 2^-9 A between
    their ends (neighbours under c2 = 36, by the last atom of one and the first of the other), while their
    centres are 36 - 2^-9 A apart = cutoff + both radii, to 2^-9: the pair the bounding spheres must not
    skip. Two small residues far away. diagonal: the axis is (1, 1, 1) / sqrt(3), so no coordinate is exact."""
    axis = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0) if diagonal else np.array([1.0, 0.0, 0.0])
    t0, t1 = np.arange(0.0, 31.0, 2.0), np.arange(36.0, 67.0, 2.0) - 2.0 ** -9
    far = np.array([[0.0, 300.0, 0.0], [1.0, 300.0, 0.5], [2.0, 300.0, 0.0], [1.0, 301.0, 0.0]])
    xyz = np.concatenate((t0[:, None] * axis, far, far + (0.0, 0.0, 40.0), t1[:, None] * axis)) + np.asarray(shift)
    line = [N, CA, C, O] + [OTHER] * 12
    return chain(xyz, [16, 4, 4, 16], line + [N, CA, C, O] * 2 + line, [1, 2, 3, 4])


# ---- atom counts across the staging boundaries ----------------------------------------------------------
STAGING_COUNTS = {"lanes": (4, 14, 15, 63, 64, 65, 200, 5),
                  "two_chunks": (200,) * 11 + (4, 14, 5),       # 2223 atoms: residue 10 straddles 2048
                  "long_residue": (2100, 6, 5, 4),              # one residue longer than the staged chunk
                  "tile_straddles": (40,) * 70}                 # the first 64-residue tile has 2560 atoms


def staging_case(counts):
    """Residues in pairs (2p, 2p + 1), 100 A between pairs: the only atom pair of a pair's two residues in
    range is the LAST atom of each (5 A apart); all their other atoms are 50 A and more from the other
    residue. So residue r has exactly two neighbours, itself and its partner."""
    xyz, role = [], []
    for r, n in enumerate(counts):
        sign = 1.0 if r % 2 else -1.0
        xyz += [[100.0 * (r // 2), 5.0 * (r % 2), sign * (50.0 + 0.5 * k)] for k in range(n - 1)]
        xyz.append([100.0 * (r // 2), 5.0 * (r % 2), 0.0])
        role += ([N, CA, C, O] + [OTHER] * (n - 4))
    return chain(xyz, counts, role, [r % 21 for r in range(len(counts))])


# ---- random float chains ---------------------------------------------------------------------------------
# (seed, residues): tests/test_env_host.py asserts the two margins for every one of them, so comparing the
# GPU with the fp64 oracle leaves nothing out
RANDOM = [(11, 37), (11, 100), (12, 145)]


def random_case(seed, L, amin=4, amax=14):
    """A self-avoiding CA walk (3.8 A steps, CAs at least 5 A apart, pulled towards the origin so the chain
    stays compact), 4-14 atoms per residue: N, CA, C, O about 1.5 A from CA, then -- 4 atoms: Gly -- a CB
    (left out for one residue in ten) and other side atoms, jittered around a point 2.5 A from CA."""
    rng = np.random.default_rng(seed)
    cas = [np.zeros(3)]
    while len(cas) < L:
        step = rng.normal(size=3) - 0.01 * cas[-1]
        p = cas[-1] + 3.8 * step / np.linalg.norm(step)
        if len(cas) < 2 or np.linalg.norm(np.array(cas[:-1]) - p, axis=1).min() >= 5.0 or rng.random() < 0.01:
            cas.append(p)
    xyz, counts, role, aa = [], [], [], []
    for ca in cas:
        n = int(rng.integers(amin, amax + 1))
        at = [ca + 1.5 * _unit(rng.normal(size=3)), ca] + [ca + 1.5 * _unit(rng.normal(size=3)) for _ in range(2)]
        ro = [N, CA, C, O]
        centre = ca + 2.5 * _unit(rng.normal(size=3))
        no_cb = rng.random() < 0.1
        for k in range(n - 4):
            at.append(centre + rng.normal(scale=0.9, size=3))
            ro.append(CB if k == 0 and not no_cb else OTHER)
        xyz += at
        role += ro
        counts.append(n)
        aa.append(int(rng.integers(0, 21)))
    return chain(xyz, counts, role, aa)


def flat(chain):
    """A chain's tuple for the fixture: field name -> array."""
    return dict(zip(("xyz", "res_off", "role", "aa", "resname_idx"), chain))
