"""Fixture for the residue-environment features: ``4heq_env.npz``.

The reference's bundled unbound pair (project/test_data/4heq_l_u.pdb, 4heq_r_u.pdb; tag ``l`` / ``r``) as
``structure.ResidueEnvOp`` takes it, and what the fp64 oracle of tests/env_cases.py gives it:

  {tag}_xyz, _res_off, _role, _aa, _resname_idx   the chain as ``structure.residue_atoms`` returns it
                                                  (``structure.read_pdb``: ATOM records, all atoms)
  {tag}_cn_raw, _un, _dn [L] int32                coordination number (self included), up / down counts
  {tag}_hsaac [L, 42], _cn [L], _onehot [L, 20]   fp32: dips columns 36:78, 78 (sklearn's MinMaxScaler over
                                                  cn_raw, rounded once), 0:20
  {tag}_amide [L, 3]                              fp32 of the fp64 cross(CA - CB, CB - N)

The generator prints the figures the tests rely on: sizes, whether every residue starts N, CA, C, O,
the CN range, and the two margins (tests/env_cases.margins), which must be far outside what fp32
rounding moves (tests/test_env_host.py asserts them).

Usage (build container only; the fixture is committed):  python tests/golden/make_env_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import refshim  # noqa: E402


def main():
    import env_cases as ec
    from deepinteract_amd.structure import read_pdb, residue_atoms
    data = os.path.join(refshim.REFERENCE_ROOT, "project", "test_data")
    out = {}
    for tag in ("l", "r"):
        path = os.path.join(data, f"4heq_{tag}_u.pdb")
        xyz, keys, names, resnames, elements = read_pdb(path)
        altlocs = {line[16] for line in open(path) if line.startswith("ATOM  ")}
        chain = residue_atoms(xyz, keys, names, resnames)
        o = ec.oracle(chain)
        off, role = chain[1], chain[2]
        first4 = all(role[off[i]:off[i] + 4].tolist() == [ec.N, ec.CA, ec.C, ec.O] for i in range(len(off) - 1))
        d2 = ec._per_residue(ec._pair_d2(chain[0], np.float64), off, np.minimum)
        rel, cos = ec.margins(chain)
        print(f"4heq_{tag}: {len(off) - 1} residues, {chain[0].shape[0]} atoms, hydrogens "
              f"{int((np.char.upper(elements) == 'H').sum())}, altlocs {sorted(altlocs)}, first four N CA C O: {first4}, "
              f"CN {o['cn_raw'].min()}-{o['cn_raw'].max()}, closest d2 to c2 {np.abs(d2 - ec.C2).min():.2e} A^2 "
              f"(relative {rel:.2e}), smallest |cos| {cos:.2e}, unknown residues {int((chain[3] == 20).sum())}")
        for k, v in ec.flat(chain).items():
            out[f"{tag}_{k}"] = v
        for k in ("cn_raw", "un", "dn", "hsaac", "cn", "onehot", "amide"):
            out[f"{tag}_{k}"] = o[k]
    path = os.path.join(HERE, "4heq_env.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
