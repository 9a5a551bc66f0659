"""Shared by the interface-label tests (not collected): the numpy yardsticks of csrc/contact_interface.hip
and the seeded cases the CPU and GPU tests both use.

A chain is ``(xyz float32 [A, 3], res_off int32 [L + 1])``; a case is ``(chain0, chain1)``.

* ``ref_labels_f32``: brute force over every atom pair in fp32 in exactly the kernel's stated order,
  dx = x0 - x1, d2 = (dx * dx + dy * dy) + dz * dz, contact iff d2 <= (float)(cutoff * cutoff). numpy rounds
  every elementwise operation to fp32 on its own and never fuses two, so this IS the specification.
* ``ref_labels_f64``: the same in fp64, d2 <= cutoff * cutoff.
* ``ambiguous``: the residue pairs that have an atom pair with |d64^2 - c^2| <= 1e-4 c^2, where fp32 and
  fp64 may legitimately disagree (fp32 rounding moves d2 by a few 1e-7 relative; 1e-4 is far outside).
"""
import numpy as np

CUTOFF = 6.0


def _pair_d2(chain0, chain1, dtype):
    a = np.asarray(chain0[0], dtype=dtype)
    b = np.asarray(chain1[0], dtype=dtype)
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == dtype
    return d2


def _per_residue(hit, off0, off1):
    """any() of an [A0, A1] atom-pair mask over every residue pair (no residue is empty)."""
    off0, off1 = np.asarray(off0, dtype=np.int64), np.asarray(off1, dtype=np.int64)
    assert (np.diff(off0) > 0).all() and (np.diff(off1) > 0).all()
    rows = np.logical_or.reduceat(hit, off0[:-1], axis=0)
    return np.logical_or.reduceat(rows, off1[:-1], axis=1)


def ref_labels_f32(chain0, chain1, cutoff=CUTOFF):
    c2 = np.float32(np.float64(cutoff) * np.float64(cutoff))
    with np.errstate(invalid="ignore", over="ignore"):
        hit = _pair_d2(chain0, chain1, np.float32) <= c2
    return _per_residue(hit, chain0[1], chain1[1]).astype(np.uint8)


def ref_labels_f64(chain0, chain1, cutoff=CUTOFF):
    hit = _pair_d2(chain0, chain1, np.float64) <= np.float64(cutoff) * np.float64(cutoff)
    return _per_residue(hit, chain0[1], chain1[1]).astype(np.uint8)


def ambiguous(chain0, chain1, cutoff=CUTOFF, rel=1e-4):
    """[n, 2] (i, j) residue pairs with an atom pair whose fp64 d2 is within rel * c2 of c2."""
    c2 = np.float64(cutoff) * np.float64(cutoff)
    near = np.abs(_pair_d2(chain0, chain1, np.float64) - c2) <= rel * c2
    return np.argwhere(_per_residue(near, chain0[1], chain1[1]))


def chain(xyz, counts):
    counts = np.asarray(counts, dtype=np.int64)
    xyz = np.ascontiguousarray(np.asarray(xyz).reshape(-1, 3), dtype=np.float32)
    assert counts.sum() == xyz.shape[0]
    return xyz, np.concatenate(([0], np.cumsum(counts))).astype(np.int32)


# ---- boundary ---------------------------------------------------------------------------------------
def boundary_case(beyond: bool):
    """1 x 1 residue, one atom each, 6 A apart exactly (-> 1) or one fp32 step beyond (-> 0)."""
    x = np.nextafter(np.float32(6.0), np.float32(np.inf)) if beyond else np.float32(6.0)
    return chain([[0.0, 0.0, 0.0]], [1]), chain([[x, 0.0, 0.0]], [1])


# ---- contraction ------------------------------------------------------------------------------------
def unfused_d2(t):
    t = np.asarray(t, dtype=np.float32)
    return (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]


def fused_d2(t):
    """The sum as a contracting compiler may form it: fma(dz, dz, fma(dy, dy, dx * dx)), each fma rounded
    once. The products of two fp32 are exact in fp64, so the fp64 sum rounded to fp32 is the fma up to
    a double rounding that none of the chosen triples is near."""
    t = np.asarray(t, dtype=np.float32).astype(np.float64)
    s = np.float32(t[0] * t[0])
    s = np.float32(t[1] * t[1] + np.float64(s))
    return np.float32(t[2] * t[2] + np.float64(s))


def contraction_triples(count=3, seed=5):
    """fp32 (dx, dy, dz) of length about 6 whose unfused and fma-contracted sums fall on different sides
    of 36: the first `count` found by a seeded search, both directions present. About 7 % of random
    directions qualify."""
    rng = np.random.default_rng(seed)
    c2 = np.float32(36.0)
    found = []                        # (triple, the unfused verdict: the specified one)
    while len(found) < count or len({inside for _, inside in found}) < 2:
        v = rng.normal(size=3)
        t = (v / np.linalg.norm(v) * 6.0).astype(np.float32)
        u, f = unfused_d2(t), fused_d2(t)
        if (u <= c2) != (f <= c2):
            found.append((t, bool(u <= c2)))
    first_in = next(t for t, inside in found if inside)
    first_out = next(t for t, inside in found if not inside)
    rest = [t for t, _ in found if t is not first_in and t is not first_out]
    return ([first_in, first_out] + rest)[:count]


def contraction_case(t):
    return chain([[0.0, 0.0, 0.0]], [1]), chain([t], [1])


# ---- random clouds ----------------------------------------------------------------------------------
RAGGED_SHAPES = [(1, 257), (65, 3), (7, 1), (33, 64)]


def cloud_case(seed, l1, l2, amin=1, amax=14, gap=3.0, side=None):
    """Two chains laid face to face: residue centres uniform in two slabs `gap` apart along z, atoms
    jittered around them (sigma 1.2 A). Float coordinates."""
    rng = np.random.default_rng(seed)
    side = 5.0 * (l1 * l2) ** 0.25 + 4.0 if side is None else side
    out = []
    for s, l in enumerate((l1, l2)):
        counts = rng.integers(amin, amax + 1, size=l)
        centre = rng.uniform(0.0, 1.0, size=(l, 3)) * (side, side, 8.0)
        centre[:, 2] = centre[:, 2] + gap if s else -centre[:, 2]
        xyz = np.repeat(centre, counts, axis=0) + rng.normal(scale=1.2, size=(counts.sum(), 3))
        out.append(chain(xyz, counts))
    return tuple(out)


# the two seeded random-float cases of the GPU test: tests/test_interface_host.py proves ambiguous()
# empty for both, so comparing with the fp64 labels hides no pair
RANDOM_FLOAT = [(104, 120, 90), (102, 118, 93)]


def random_float_case(seed, l1, l2):
    return cloud_case(seed, l1, l2, amin=4, amax=14, gap=3.5)


def grid_exact_case(seed=7, l1=97, l2=131):
    """1-20 atoms per residue, every coordinate a multiple of 1/8 A within +-64: differences are
    multiples of 1/8 below 128, their squares multiples of 1/64 below 2^14 and the sums below 2^16, all
    exact in fp32's 24 bits. fp32 and fp64 then agree on every pair, exact ties (d2 == 36) included."""
    rng = np.random.default_rng(seed)
    out = []
    for s, l in enumerate((l1, l2)):
        counts = rng.integers(1, 21, size=l)
        centre = rng.integers(-20 * 8, 20 * 8 + 1, size=(l, 3))
        atoms = np.repeat(centre, counts, axis=0) + rng.integers(-2 * 8, 2 * 8 + 1, size=(counts.sum(), 3))
        out.append((atoms, counts))
    (a0, c0), (a1, c1) = out
    # exact ties: the first atoms of chain 1's residues 0 and 1 lie exactly 6 A from chain 0's, (6, 0, 0) and (4, 4, 2)
    a1[0] = a0[0] + np.array([6, 0, 0]) * 8
    a1[c1[0]] = a0[c0[0]] + np.array([4, 4, 2]) * 8
    assert np.abs(a0).max() <= 64 * 8 and np.abs(a1).max() <= 64 * 8
    return chain(a0 / 8.0, c0), chain(a1 / 8.0, c1)


# ---- atom counts across the staging boundaries --------------------------------------------------------
STAGING_COUNTS = [(1, 14, 15, 63, 64, 65, 200),     # a wave's lanes, one staging chunk
                  (200,) * 11 + (1, 14)]            # 2215 atoms: past the 2048 atoms staged at a time,
#                                                     residue 10 straddles the chunk boundary


def staging_case(counts):
    """Residue r of either chain has counts[r] atoms; the only atom pair in range of residue pair (r, r)
    is the LAST atom of each (5 A apart); every other atom is 50 A and more away, and residues r != r'
    are 100 A apart. The map is the identity."""
    xyz = [[], []]
    for r, n in enumerate(counts):
        for s in (0, 1):
            sign = 1.0 if s else -1.0
            far = [[100.0 * r, 5.0 * s, sign * (50.0 + 0.5 * k)] for k in range(n - 1)]
            xyz[s] += far + [[100.0 * r, 5.0 * s, 0.0]]
    return chain(xyz[0], counts), chain(xyz[1], counts)


# ---- cull soundness ---------------------------------------------------------------------------------
def cull_case(diagonal: bool, shift=(0.0, 0.0, 0.0)):
    """Per chain one residue of 16 atoms on a 30 A line (2 A apart) and one residue far away. The two
    lines lie end to end on one axis and touch at exactly the cutoff (t = 30 and t = 36), while their
    centres are 36 A apart = cutoff + both radii: the pair the bounding spheres must not skip.
    diagonal: the axis is (1, 1, 1) / sqrt(3) instead of x, so no coordinate is exact. shift: added in
    fp64 before rounding to fp32 (every yardstick sees the same fp32 inputs)."""
    axis = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0) if diagonal else np.array([1.0, 0.0, 0.0])
    t0, t1 = np.arange(0.0, 31.0, 2.0), np.arange(36.0, 67.0, 2.0)
    far = np.array([[0.0, 300.0, 0.0], [1.0, 300.0, 0.5]])
    shift = np.asarray(shift, dtype=np.float64)
    c0 = np.concatenate((t0[:, None] * axis, far)) + shift
    c1 = np.concatenate((far + (0.0, 0.0, 4.0), t1[:, None] * axis)) + shift
    return chain(c0, [16, 2]), chain(c1, [2, 16])


CULL_SHIFT = (9000.0, -9000.0, 9000.0)      # fp32 spacing 2^-10 A: the coarsest of PDB-range coordinates


# ---- face-to-face complexes for the loop tests --------------------------------------------------------
def structure_for(l1, l2, seed):
    """A small complex with positives, as test_batch_structures takes it."""
    return cloud_case(seed, l1, l2, amin=4, amax=14, gap=3.0)


def examples_from_labels(labels, l1, l2):
    """The reference's complete example list [l1 * l2, 3] int64 (i, j, label), row-major."""
    i, j = np.divmod(np.arange(l1 * l2, dtype=np.int64), l2)
    return np.stack((i, j, np.asarray(labels, dtype=np.int64).reshape(-1)), axis=1)
