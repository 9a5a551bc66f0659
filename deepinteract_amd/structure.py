"""DIPS-Plus's structure-derived node features from a chain's atoms, on HIP.

Of the 106 DIPS-Plus columns (``synth.py`` lists them) 63 are functions of the chain's atoms alone, and
so are the amide normals and the backbone rows the graph builder takes. ``ResidueEnvOp`` computes them
on the device (csrc/residue_env.hip, ``di_residue_env_batch``) for a ragged batch of chains:

====================  =====================  ==========================================================
``dips`` columns      node-feature columns   what
====================  =====================  ==========================================================
0:20                  7:27                   residue type one-hot (graph_utils.py:113-126)
36:78                 43:85                  HSAAC, half-sphere amino-acid composition
                                             (get_hsacc, dips_plus_utils.py:118-161)
78                    85                     coordination number, min-max normalised per chain
                                             (get_similarity_matrix :84-115, :569)
(``amide_norm``)                             cross(CA - CB, CB - N), zero without a CB (:356-374, :908-911)
====================  =====================  ==========================================================

The other 43 columns need external programs -- DSSP (20:28, 28), MSMS (29), PSAIA (30:36), HH-suite
(79:106) -- and stay the caller's to supply (``extern``).

Definitions (include/deepinteract_amd.h states them to the bit). A chain is L residues, each a run of
atoms (ALL atoms of the residue, hydrogens too when the file has them: the reference's ``get_coords``
takes ``r.get_list()``); every atom has a role (other, N, CA, C, O, CB), every residue an ``aa`` index
into ``'ACDEFGHIKLMNPQRSTVWY-'``. Residues i and j are neighbours iff some atom pair has fp32
``d2 < c2`` (strict; ``ENV_C2 = float32(8 ln 1000)``: the reference's ``exp(-d2 / 8) > 1e-3``); a residue
is its own neighbour. CN counts the neighbours, self included. The side-chain vector ``u_i`` is the mean
of the unit vectors from CA to the atoms whose ROLE is not N, CA, C or O (the reference takes
``get_unpacked_list()[4:]``, the same set whenever a residue's first four atoms are N, CA, C, O; the role
is what this module goes by); without such atoms it is 1/2 [(CA - C)/|CA - C| + (CA - N)/|CA - N|].
A neighbour j != i is *up* iff ``dot(u_i, CA_j - CA_i) > 0``, otherwise -- a zero or NaN dot included --
*down*.

The residue itself counts as down. That follows Biopython's ``Vector.angle``: for the zero vector it forms
0/0 = nan, then ``min(nan, 1) = nan`` and ``max(-1, nan) = -1``, so the angle is pi and ``angle < pi/2``
fails. This was derived by reading Biopython's code; Biopython is not installed where this was written,
so it was not executed.

Every residue must hold exactly one N, CA, C and O and at most one CB -- the residues the graph builder
accepts anyway. The reference's NaN-then-impute path for residues without a CA is deliberately NOT
reproduced: such a chain is refused (``ValueError``).
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib
from .synth import RESNAMES

AA_LETTERS = "ACDEFGHIKLMNPQRSTVWY-"
THREE_TO_ONE = {"ALA": "A", "CYS": "C", "ASP": "D", "GLU": "E", "PHE": "F", "GLY": "G", "HIS": "H", "ILE": "I",
                "LYS": "K", "LEU": "L", "MET": "M", "ASN": "N", "PRO": "P", "GLN": "Q", "ARG": "R", "SER": "S",
                "THR": "T", "VAL": "V", "TRP": "W", "TYR": "Y"}
ROLES = {"N": _lib.DI_ROLE_N, "CA": _lib.DI_ROLE_CA, "C": _lib.DI_ROLE_C, "O": _lib.DI_ROLE_O,
         "CB": _lib.DI_ROLE_CB}
ENV_C2 = float(np.float32(8.0 * math.log(1000.0)))     # 55.262043
OWN_COLUMNS = np.r_[0:20, 36:79]                       # the dips columns the op writes
EXTERN_COLUMNS = np.r_[20:36, 79:106]                  # the 43 it leaves to the caller


def read_pdb(path, chain=None):
    """The atoms of a PDB file by its fixed columns: the ``ATOM`` records (no ``HETATM``) of the first
    model, of every chain or of the chain id(s) given (a string of one-letter ids). Of alternate
    locations, an atom is kept when its altloc is blank or is the first non-blank one seen in its residue.

    Returns ``(xyz float64 [N, 3], residue_key str [N, 3] (chain id, residue number, insertion code),
    atom_name str [N], resname str [N], element str [N])`` in file order -- what ``residue_atoms`` and
    ``ranking.interface_atoms`` take. ValueError when no atom is left."""
    xyz, keys, names, resnames, elements = [], [], [], [], []
    altloc_of = {}
    with open(path) as fh:
        for line in fh:
            if line.startswith("ENDMDL"):
                break
            if not line.startswith("ATOM  "):
                continue
            if chain is not None and line[21] not in chain:
                continue
            key = (line[21], line[22:26], line[26])
            alt = line[16]
            if alt != " " and altloc_of.setdefault(key, alt) != alt:
                continue
            name = line[12:16].strip()
            el = line[76:78].strip()
            xyz.append((float(line[30:38]), float(line[38:46]), float(line[46:54])))
            keys.append(key)
            names.append(name)
            resnames.append(line[17:20].strip())
            elements.append(el if el else name.lstrip("0123456789")[:1])
    if not xyz:
        raise ValueError(f"read_pdb: no ATOM record{'' if chain is None else ' of chain ' + repr(chain)} in {path}")
    return (np.array(xyz, dtype=np.float64), np.array(keys, dtype=str), np.array(names, dtype=str),
            np.array(resnames, dtype=str), np.array(elements, dtype=str))


def residue_atoms(xyz, residue_index, atom_name, resname):
    """One chain's atoms as ``ResidueEnvOp`` takes them: ``(xyz float32 [A, 3], res_off int32 [L + 1],
    role uint8 [A], aa uint8 [L], resname_idx uint8 [L])``. Host, numpy. Atoms are grouped as
    ``ranking.interface_atoms`` groups them (residue_index: one entry or row per atom; atoms of one
    residue follow each other; residues are numbered in order of first appearance), but ALL atoms are
    kept, hydrogens too. role: 1..5 for the atoms named N, CA, C, O, CB, else 0. aa: the index of the
    residue's one-letter code in ``AA_LETTERS``, 20 ('-') when its name (that of its first atom) is not
    one of the standard twenty; resname_idx: its column of the residue one-hot (``synth.RESNAMES``), an
    unknown name going to the last (GLN), as in the reference. ValueError for arrays of other shapes, a
    chain without atoms, or a residue index that reappears after another one."""
    xyz = np.asarray(xyz)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError("residue atoms: xyz is [N, 3]")
    res = np.asarray(residue_index)
    if res.ndim == 1:
        res = res[:, None]
    if res.ndim != 2 or res.shape[0] != xyz.shape[0]:
        raise ValueError("residue atoms: one residue index per atom")
    names = np.char.upper(np.char.strip(np.asarray(atom_name, dtype=str)))
    if names.shape != (xyz.shape[0],):
        raise ValueError("residue atoms: one atom name per atom")
    rn = np.char.upper(np.char.strip(np.asarray(resname, dtype=str)))
    if rn.shape != (xyz.shape[0],):
        raise ValueError("residue atoms: one residue name per atom")
    if xyz.shape[0] < 1:
        raise ValueError("residue atoms: the chain has no atoms")
    starts = np.concatenate(([0], np.flatnonzero((res[1:] != res[:-1]).any(axis=1)) + 1))
    if len(np.unique(res[starts], axis=0)) != len(starts):
        raise ValueError("residue atoms: a residue index reappears after another residue "
                         "(the atoms of one residue follow each other)")
    res_off = np.concatenate((starts, [xyz.shape[0]])).astype(np.int32)
    role = np.zeros(xyz.shape[0], dtype=np.uint8)
    for name, code in ROLES.items():
        role[names == name] = code
    aa = np.array([AA_LETTERS.index(THREE_TO_ONE.get(n, "-")) for n in rn[starts]], dtype=np.uint8)
    col = np.array([RESNAMES.index(n) if n in RESNAMES else len(RESNAMES) - 1 for n in rn[starts]], dtype=np.uint8)
    return np.ascontiguousarray(xyz, dtype=np.float32), res_off, role, aa, col


_ENV_MESSAGES = (
    (_lib.DI_ENV_OFFSETS, "residue env: residue offsets do not start at 0, decrease, or do not end at the atom count"),
    (_lib.DI_ENV_EMPTY, "residue env: a residue without atoms"),
    (_lib.DI_ENV_NONFINITE, "residue env: a NaN or Inf coordinate"),
    (_lib.DI_ENV_BACKBONE, "residue env: a role, aa or resname code out of range, or a residue without exactly one "
                           "N, CA, C and O and at most one CB"),
)


class EnvFeatures(list):
    """``ResidueEnvOp.features``' result: one dict of views per chain, and ``packed``, the buffers they
    are views of (``dips [Lt, 106]``, ``amide_norm [Lt, 3]``, ``backbone [Lt, 4, 3]``, ``cn_raw [Lt]``,
    chains back to back) with ``sizes``, the chains' residue counts."""
    packed = None
    sizes = None


class ResidueEnvOp:
    """The structure-derived DIPS-Plus columns, amide normals and backbone rows of a batch of chains on
    HIP (csrc/residue_env.hip, ``di_residue_env_batch``; the module docstring has the definitions). One
    memset and three launches per DI_BATCH_MAX chains, one host read (the flags) per call. No CPU
    fallback."""

    def __init__(self, device="cuda"):
        from .engine import gpu_device
        self.device = gpu_device(device)
        self.lib = _lib.load()

    def features(self, chains, extern=None, c2=ENV_C2):
        """chains[i]: ``(xyz [A, 3], res_off [L + 1], role [A], aa [L], resname_idx [L])``
        (``residue_atoms``), numpy arrays or tensors on the op's GPU. extern[i] (optional, or None for
        a chain): ``[L, 106]`` supplying the 43 columns this op does not own (``EXTERN_COLUMNS``); what
        it holds in the op's own columns is ignored; absent, those 43 columns are zeros.

        Returns an ``EnvFeatures``: per chain ``{"dips": [L, 106], "amide_norm": [L, 3], "backbone":
        [L, 4, 3], "cn_raw": [L] int32}``, views of packed device buffers. All host arrays of a call go to
        the device in ONE pinned packed copy on the current stream; device tensors are read where they
        are (converted to the kernel's dtype and made contiguous if they are not).
        Raises ValueError for arrays of other shapes or a c2 that is not finite and positive, before any
        launch; then, for the first chain that has a fault: malformed offsets, a residue without atoms,
        a NaN or Inf coordinate, a bad code or backbone, in this order."""
        from .engine import _ptr, _stream, check_on
        from .ranking import _table_to_device
        count = len(chains)
        if count < 1:
            raise ValueError("residue env: a non-empty list of chains")
        if extern is not None and len(extern) != count:
            raise ValueError(f"residue env: {len(extern)} extern arrays for {count} chains")
        c2 = float(c2)
        as_f32 = ctypes.c_float(c2).value           # what the kernels get
        if not math.isfinite(as_f32) or as_f32 <= 0:
            raise ValueError(f"residue env: c2 = {c2}: finite and positive")
        host, nbytes = [], 0      # (array, byte offset in the packed copy), every array 16-B aligned

        def take(a, dtype, tdtype):
            nonlocal nbytes
            if isinstance(a, torch.Tensor):
                check_on(self.device, "ResidueEnvOp", a)
                return a.to(tdtype).contiguous()
            a = np.ascontiguousarray(a, dtype=dtype)
            host.append((a, nbytes))
            nbytes += (a.nbytes + 15) // 16 * 16
            return len(host) - 1

        kinds = ((np.float32, torch.float32), (np.int32, torch.int32), (np.uint8, torch.uint8),
                 (np.uint8, torch.uint8), (np.uint8, torch.uint8))
        fields, sizes, atoms = [], [], []
        for ci, chain in enumerate(chains):
            if len(chain) != 5:
                raise ValueError("residue env: a chain is (xyz [A, 3], res_off [L + 1], role [A], aa [L], resname_idx [L])")
            xyz, off, role, aa, col = chain
            if len(xyz.shape) != 2 or xyz.shape[1] != 3 or any(len(t.shape) != 1 for t in (off, role, aa, col)):
                raise ValueError("residue env: a chain is (xyz [A, 3], res_off [L + 1], role [A], aa [L], resname_idx [L])")
            a, l = int(xyz.shape[0]), int(off.shape[0]) - 1
            if a < 1 or l < 1:
                raise ValueError("residue env: a chain has at least one residue and one atom")
            if int(role.shape[0]) != a or int(aa.shape[0]) != l or int(col.shape[0]) != l:
                raise ValueError("residue env: role is [A], aa and resname_idx are [L]")
            ext = extern[ci] if extern is not None else None
            if ext is not None and tuple(ext.shape) != (l, 106):
                raise ValueError(f"residue env: extern of a chain of {l} residues is [{l}, 106]")
            row = [take(t, *kd) for t, kd in zip(chain, kinds)]
            row.append(None if ext is None else take(ext, np.float32, torch.float32))
            fields.append(row)
            sizes.append(l)
            atoms.append(a)
        if host:
            pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
            flat = pinned.numpy()
            for a, at in host:
                flat[at:at + a.nbytes] = a.reshape(-1).view(np.uint8)
            packed = pinned.to(self.device, non_blocking=True)
            for row in fields:
                for s, tdtype in enumerate((torch.float32, torch.int32, torch.uint8, torch.uint8, torch.uint8,
                                            torch.float32)):
                    if row[s] is not None and not isinstance(row[s], torch.Tensor):
                        a, at = host[row[s]]
                        row[s] = packed[at:at + a.nbytes].view(tdtype)
        lt = sum(sizes)
        dips = torch.zeros(lt, 106, dtype=torch.float32, device=self.device)
        amide = torch.empty(lt, 3, dtype=torch.float32, device=self.device)
        bb = torch.empty(lt, 4, 3, dtype=torch.float32, device=self.device)
        cn_raw = torch.empty(lt, dtype=torch.int32, device=self.device)
        out = EnvFeatures()
        items = (_lib.DiEnvItem * count)()
        lo = 0
        for it, row, l, a in zip(items, fields, sizes, atoms):
            view = {"dips": dips[lo:lo + l], "amide_norm": amide[lo:lo + l], "backbone": bb[lo:lo + l],
                    "cn_raw": cn_raw[lo:lo + l]}
            if row[5] is not None:
                view["dips"].copy_(row[5].view(l, 106))
            it.xyz, it.res_off, it.role, it.aa, it.resname = (t.data_ptr() for t in row[:5])
            it.dips, it.amide_norm, it.backbone, it.cn_raw = (view[f].data_ptr() for f in
                                                              ("dips", "amide_norm", "backbone", "cn_raw"))
            it.l, it.a = l, a
            out.append(view)
            lo += l
        stats = []
        for lo in range(0, count, _lib.DI_BATCH_MAX):
            m = min(_lib.DI_BATCH_MAX, count - lo)
            part = (_lib.DiEnvItem * m).from_buffer(items, lo * ctypes.sizeof(_lib.DiEnvItem))
            nb = self.lib.di_residue_env_work_bytes(part, m)
            if nb < 0:
                raise ValueError(f"residue env of a batch of {m}: code {nb} (a chain's atoms and residues < 2^24)")
            # its own workspace per launch: the stats at its front are read after the last one
            work = torch.empty(nb // 8, dtype=torch.int64, device=self.device)
            part_dev = _table_to_device(part, self.device)
            _lib.check(self.lib.di_residue_env_batch(part, _ptr(part_dev), m, ctypes.c_float(c2), _ptr(work),
                                                     _stream()), "di_residue_env_batch")
            stats.append(work[:2 * m])
        rows = (stats[0] if len(stats) == 1 else torch.cat(stats)).cpu().view(count, 2).tolist()
        for word, _ in rows:
            f = word & 0xffffffff
            for bit, text in _ENV_MESSAGES:
                if f & bit:
                    raise ValueError(text)
        out.packed = {"dips": dips, "amide_norm": amide, "backbone": bb, "cn_raw": cn_raw}
        out.sizes = sizes
        out._keep = fields        # the inputs the launches read
        return out
