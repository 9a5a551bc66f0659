"""Fixture for the interface labels: ``4heq_interface.npz``.

The reference's bundled unbound pair (project/test_data/4heq_l_u.pdb, 4heq_r_u.pdb; chain 0 = l, chain
1 = r) as ``ranking.InterfaceOp`` takes it, and the labels an independent oracle gives it:

  xyz0, xyz1          [A, 3] float32, the ATOM / HETATM records that are not hydrogen, in file order
  res_off0, res_off1  [L + 1] int32 CSR offsets (``ranking.interface_atoms`` over chain id, residue
                      number and insertion code)
  labels              [L1, L2] uint8: residues i and j have heavy atoms within 6 A (<=), from scipy's
                      ``cKDTree.query_ball_point(r=6)`` over the fp64 coordinates the file prints
  num_pos             labels.sum()

This is the definition behind DIPS' pos_idx (deepinteract_utils.py:612: neighbor_def='non_heavy_res',
cutoff=6). The PDB's three decimals are exact multiples of 1e-3 in fp64 as parsed; the fp32 arrays are
those values rounded once. The closest atom pair to the 6 A boundary is 1.2e-3 A from it, far outside
anything fp32 rounding moves (tests/test_interface_host.py checks that nothing is ambiguous).

Usage (build container only; the fixture is committed):  python tests/golden/make_interface_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import refshim  # noqa: E402


def read_pdb(path):
    """(xyz fp64 [N, 3], residue keys [N, 3] str, element [N] str) of the first model's atoms."""
    xyz, keys, element = [], [], []
    with open(path) as fh:
        for line in fh:
            if line.startswith("ENDMDL"):
                break
            if not line.startswith(("ATOM  ", "HETATM")):
                continue
            xyz.append((float(line[30:38]), float(line[38:46]), float(line[46:54])))
            keys.append((line[21], line[22:26], line[26]))
            el = line[76:78].strip()
            element.append(el if el else line[12:16].strip().lstrip("0123456789")[:1])
    return np.array(xyz, dtype=np.float64), np.array(keys, dtype=str), np.array(element, dtype=str)


def main():
    from scipy.spatial import cKDTree

    from deepinteract_amd.ranking import interface_atoms
    data = os.path.join(refshim.REFERENCE_ROOT, "project", "test_data")
    chains, exact = [], []
    for name in ("4heq_l_u.pdb", "4heq_r_u.pdb"):
        xyz, keys, element = read_pdb(os.path.join(data, name))
        xyz32, off = interface_atoms(xyz, keys, element)
        heavy = np.char.upper(np.char.strip(element)) != "H"
        assert xyz32.shape[0] == heavy.sum()
        chains.append((xyz32, off))
        exact.append(xyz[heavy])
    (x0, o0), (x1, o1) = chains
    res0 = np.repeat(np.arange(len(o0) - 1), np.diff(o0))
    res1 = np.repeat(np.arange(len(o1) - 1), np.diff(o1))
    labels = np.zeros((len(o0) - 1, len(o1) - 1), dtype=np.uint8)
    near = cKDTree(exact[1]).query_ball_point(exact[0], r=6.0)
    for a, hits in enumerate(near):
        labels[res0[a], res1[hits]] = 1
    out = os.path.join(HERE, "4heq_interface.npz")
    np.savez_compressed(out, xyz0=x0, res_off0=o0, xyz1=x1, res_off1=o1, labels=labels,
                        num_pos=np.int64(labels.sum()))
    print(f"{out}: {labels.shape[0]} x {labels.shape[1]} residues, {x0.shape[0]} + {x1.shape[0]} heavy atoms, "
          f"at most {max(np.diff(o0).max(), np.diff(o1).max())} per residue, {int(labels.sum())} positives, "
          f"{os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
