"""Bond-length constraints for batched molecular dynamics (newtonnet_amd/dynamics.py, csrc/rattle.hip): what the host does once, at
construction -- checking the pairs, colouring every molecule's constraint graph, sorting the constraints by (molecule, colour) and
laying out the tables nnhip_md_step_constrained reads (include/newtonnet_hip.h has the layout).

Colouring: greedy edge colouring in input order -- a constraint takes the smallest colour neither of its atoms has used yet.  No
two constraints of a colour share an atom, so the lanes of a wave can take a colour's constraints side by side; a constraint sees
at most (deg_i - 1) + (deg_j - 1) taken colours, hence at most 2 max_degree - 1 colours per molecule."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch


class Prepared(NamedTuple):
    """Constraints sorted by (molecule, colour, input order), as numpy arrays:
    order [C] (position in the input of every sorted constraint), pairs [C,2] int64 (global atom indices, sorted), local [C,2] int32
    (atoms counted within their molecule), colour [C], mol_col_ptr int32 [B+1], col_ptr int32 [K+1], per_mol int64 [B] (C_b)"""
    order: np.ndarray
    pairs: np.ndarray
    local: np.ndarray
    colour: np.ndarray
    mol_col_ptr: np.ndarray
    col_ptr: np.ndarray
    per_mol: np.ndarray


def greedy_edge_colouring(pairs) -> np.ndarray:
    """colour [C] of the constraints `pairs` [C,2] of one molecule (or of several: colours are per connected atoms anyway), greedy
    in input order"""
    used = {}
    colour = np.zeros(len(pairs), dtype=np.int64)
    for c, (i, j) in enumerate(np.asarray(pairs, dtype=np.int64).reshape(-1, 2).tolist()):
        taken = used.setdefault(i, set()) | used.setdefault(j, set())
        k = 0
        while k in taken:
            k += 1
        colour[c] = k
        used[i].add(k)
        used[j].add(k)
    return colour


def prepare(pairs, lengths, batch, n_mol: int, fixed=None, max_atoms: Optional[int] = None) -> Prepared:
    """Check and sort constraints on the host.  pairs: int64 [C,2] global atom indices; lengths: [C] or None; batch: [N] sorted
    molecule index of every atom; fixed: bool [N] or None (numpy arrays or host tensors).  Raises ValueError for a pair across
    molecules, i == j, duplicate pairs, a pair of two fixed atoms, an index outside 0 .. N - 1, a length <= 0 and a constrained
    molecule above max_atoms."""
    pairs = np.asarray(pairs)
    if pairs.dtype != np.int64 or pairs.ndim != 2 or pairs.shape[1] != 2:
        raise ValueError(f'constraints: pairs int64 [C,2] expected (got {pairs.dtype} {tuple(pairs.shape)})')
    batch = np.asarray(batch).astype(np.int64).reshape(-1)
    N, C = batch.size, pairs.shape[0]
    if lengths is not None:
        lengths = np.asarray(lengths)
        if lengths.dtype != np.float32 or lengths.shape != (C,):
            raise ValueError(f'constraints: lengths float32 [{C}] or None expected (got {lengths.dtype} {tuple(lengths.shape)})')
        if not bool(np.all(np.isfinite(lengths) & (lengths > 0))):
            raise ValueError('constraints: every length must be finite and > 0')
    if C and (pairs.min() < 0 or pairs.max() >= N):
        raise ValueError(f'constraints: atom indices in 0 .. {N - 1} expected')
    i, j = pairs[:, 0], pairs[:, 1]
    if np.any(i == j):
        raise ValueError(f'constraints: constraint {int(np.argmax(i == j))} joins an atom to itself')
    mol = batch[i] if C else np.zeros(0, dtype=np.int64)
    if C and np.any(mol != batch[j]):
        c = int(np.argmax(mol != batch[j]))
        raise ValueError(f'constraints: constraint {c} joins atoms of two molecules ({int(batch[i[c]])} and {int(batch[j[c]])})')
    key = np.minimum(i, j) * max(N, 1) + np.maximum(i, j)
    if np.unique(key).size != C:
        raise ValueError('constraints: duplicate pairs')
    if fixed is not None and C:
        fixed = np.asarray(fixed).astype(bool).reshape(-1)
        if np.any(fixed[i] & fixed[j]):
            raise ValueError(f'constraints: constraint {int(np.argmax(fixed[i] & fixed[j]))} joins two fixed atoms')
    counts = np.bincount(batch, minlength=n_mol) if N else np.zeros(n_mol, dtype=np.int64)
    per_mol = np.bincount(mol, minlength=n_mol) if C else np.zeros(n_mol, dtype=np.int64)
    if max_atoms is not None and np.any((per_mol > 0) & (counts > max_atoms)):
        b = int(np.argmax((per_mol > 0) & (counts > max_atoms)))
        raise ValueError(f'constraints: molecule {b} has {int(counts[b])} atoms, above the {max_atoms} a constrained molecule may '
                         'have (one wave works on one molecule, its state in LDS)')
    first = np.concatenate([[0], np.cumsum(counts)])[:-1]
    colour = greedy_edge_colouring(pairs)          # (constraints of different molecules share no atom: one pass colours them all)
    order = np.lexsort((np.arange(C), colour, mol)) if C else np.zeros(0, dtype=np.int64)
    s_pairs, s_mol, s_col = pairs[order], mol[order], colour[order]
    n_colours = np.zeros(n_mol, dtype=np.int64)
    if C:
        np.maximum.at(n_colours, s_mol, s_col + 1)
    mol_col_ptr = np.concatenate([[0], np.cumsum(n_colours)]).astype(np.int32)
    slot = mol_col_ptr[s_mol].astype(np.int64) + s_col if C else np.zeros(0, dtype=np.int64)      # the global colour of each
    col_ptr = np.concatenate([[0], np.cumsum(np.bincount(slot, minlength=int(mol_col_ptr[-1])))]).astype(np.int32)
    local = (s_pairs - first[s_mol][:, None]).astype(np.int32) if C else np.zeros((0, 2), dtype=np.int32)
    return Prepared(order, s_pairs, local, s_col, mol_col_ptr, col_ptr, per_mol)


def hydrogen_constraints(z: torch.Tensor, pos: torch.Tensor, batch: torch.Tensor, max_length: float = 1.3):
    """(pairs int64 [C,2], lengths fp32 [C]) on the device of pos: every hydrogen paired with its nearest non-hydrogen atom of the
    same molecule, (heavy atom, hydrogen), at the present distance -- on the positions as stored, no minimum image (the convention
    newtonnet_amd/metadynamics.py uses for its collective variables).  Raises ValueError when a hydrogen has no partner within
    max_length (Angstrom)."""
    zz = z.detach().cpu().numpy().astype(np.int64).reshape(-1)
    x = pos.detach().cpu().double().numpy().reshape(-1, 3)
    bb = batch.detach().cpu().numpy().astype(np.int64).reshape(-1)
    if not (zz.size == bb.size == x.shape[0]):
        raise ValueError('hydrogen_constraints: z [N], pos [N,3] and batch [N] expected')
    pairs, lengths = [], []
    bounds = np.flatnonzero(np.diff(bb)) + 1 if bb.size else np.zeros(0, dtype=np.int64)
    for a0, a1 in zip(np.concatenate([[0], bounds]), np.concatenate([bounds, [bb.size]])):
        h = np.flatnonzero(zz[a0:a1] == 1) + a0
        heavy = np.flatnonzero(zz[a0:a1] != 1) + a0
        if h.size == 0:
            continue
        if heavy.size == 0:
            raise ValueError(f'hydrogen_constraints: atom {int(h[0])} (H) has no non-hydrogen atom in its molecule')
        d = np.linalg.norm(x[h][:, None, :] - x[heavy][None, :, :], axis=-1)
        near = d.argmin(axis=1)
        dist = d[np.arange(h.size), near]
        if np.any(dist > max_length):
            k = int(np.argmax(dist > max_length))
            raise ValueError(f'hydrogen_constraints: atom {int(h[k])} (H) has no non-hydrogen partner within {max_length} A (the '
                             f'nearest is {dist[k]:.3f} A away)')
        pairs += [np.stack([heavy[near], h], axis=1)]
        lengths += [dist]
    pairs = np.concatenate(pairs) if pairs else np.zeros((0, 2), dtype=np.int64)
    lengths = np.concatenate(lengths) if lengths else np.zeros(0)
    return (torch.from_numpy(pairs.astype(np.int64)).to(pos.device), torch.from_numpy(lengths.astype(np.float32)).to(pos.device))


def device_tables(prep: Prepared, d2: np.ndarray, mol_ptr: torch.Tensor):
    """hip.ConstraintTables of prepared constraints: d2 fp32 [C] in SORTED order, mol_ptr int32 [B+1] on the device"""
    from newtonnet_amd import hip
    dev = mol_ptr.device
    mcp, cp = torch.from_numpy(prep.mol_col_ptr.copy()), torch.from_numpy(prep.col_ptr.copy())
    return hip.ConstraintTables(mol_ptr, mol_ptr.cpu(), mcp.to(dev), mcp, cp.to(dev), cp,
                                torch.from_numpy(np.ascontiguousarray(prep.local)).to(dev).contiguous(),
                                torch.from_numpy(np.ascontiguousarray(d2, dtype=np.float32)).to(dev))
