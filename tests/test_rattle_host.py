"""Bond-length constraints, the parts that run anywhere: the colouring and the checks of newtonnet_amd/constraints.py,
hydrogen_constraints on the MD fixtures, the fp64 reference of tests/rattle_ref.py against the properties a RATTLE step must have,
the ABI of the new entry points and the degrees of freedom of a constrained trajectory."""
import ctypes
import os

import numpy as np
import pytest
import torch

from newtonnet_amd import abi
from newtonnet_amd import constraints as con
from tests import rattle_ref as rr
from tests import util


def _batch(sizes):
    return np.repeat(np.arange(len(sizes)), sizes)


def _is_matching(pairs):
    atoms = np.asarray(pairs).reshape(-1)
    return np.unique(atoms).size == atoms.size


CH4 = [[0, 1], [0, 2], [0, 3], [0, 4]]
TRIANGLE = [[0, 1], [0, 2], [1, 2]]
PAIRS70 = [[2 * k, 2 * k + 1] for k in range(70)]


@pytest.mark.parametrize('pairs, n_atoms, n_colours', [(CH4, 5, 4), (TRIANGLE, 3, 3), (PAIRS70, 140, 1), ([], 0, 0)])
def test_every_colour_is_a_matching_and_greedy_stays_within_two_delta_minus_one(pairs, n_atoms, n_colours):
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    colour = con.greedy_edge_colouring(p)
    assert (int(colour.max()) + 1 if len(pairs) else 0) == n_colours
    for k in range(n_colours):
        assert _is_matching(p[colour == k])
    if len(pairs):
        delta = np.bincount(p.reshape(-1)).max()
        assert n_colours <= 2 * delta - 1
    prep = con.prepare(p, None, _batch([n_atoms]), 1)
    assert prep.mol_col_ptr.tolist() == [0, n_colours] and prep.col_ptr[-1] == len(pairs) and prep.per_mol.tolist() == [len(pairs)]


def test_prepare_sorts_by_molecule_and_colour_and_counts_within_the_molecule():
    rng = np.random.default_rng(0)
    sizes = [3, 0, 5, 3, 140]
    first = np.concatenate([[0], np.cumsum(sizes)])
    pairs = np.concatenate([np.array(TRIANGLE) + first[0], np.array(CH4) + first[2], np.array(PAIRS70) + first[4]])
    perm = rng.permutation(len(pairs))
    prep = con.prepare(pairs[perm], None, _batch(sizes), 5)
    assert prep.mol_col_ptr.tolist() == [0, 3, 3, 7, 7, 8] and prep.per_mol.tolist() == [3, 0, 4, 0, 70]
    assert np.array_equal(prep.pairs, pairs[perm][prep.order])
    for k in range(8):                               # every colour: a matching inside ONE molecule, local indices inside it
        sl = slice(prep.col_ptr[k], prep.col_ptr[k + 1])
        assert _is_matching(prep.pairs[sl]) and sl.stop > sl.start
        b = int(np.searchsorted(prep.mol_col_ptr, k, side='right') - 1)
        assert np.all(_batch(sizes)[prep.pairs[sl]] == b)
        assert np.array_equal(prep.local[sl], prep.pairs[sl] - first[b]) and prep.local[sl].max() < sizes[b]
    degree = np.bincount(pairs.reshape(-1))
    assert prep.mol_col_ptr[-1] <= sum(2 * degree[first[b]:first[b + 1]].max() - 1 for b in (0, 2, 4))


def test_every_refusal_by_message():
    batch = _batch([3, 3])
    ok = np.array([[0, 1], [3, 4]], dtype=np.int64)
    con.prepare(ok, np.array([1.0, 1.0], dtype=np.float32), batch, 2)
    for pairs, lengths, fixed, max_atoms, msg in (
            (np.array([[0, 3]]), None, None, None, 'two molecules'),
            (np.array([[1, 1]]), None, None, None, 'itself'),
            (np.array([[0, 1], [1, 0]]), None, None, None, 'duplicate'),
            (np.array([[0, 1]]), None, np.array([1, 1, 0, 0, 0, 0], dtype=bool), None, 'two fixed'),
            (np.array([[0, 1]]), np.array([0.0], dtype=np.float32), None, None, 'length'),
            (np.array([[0, 1]]), np.array([-1.0], dtype=np.float32), None, None, 'length'),
            (np.array([[0, 1]]), np.array([1.0]), None, None, 'float32'),
            (np.array([[0, 1]], dtype=np.int32), None, None, None, 'int64'),
            (np.array([[0, 6]]), None, None, None, 'indices'),
            (np.array([[0, 1]]), None, None, 2, 'above the 2')):
        with pytest.raises(ValueError, match=msg):
            con.prepare(pairs, lengths, batch, 2, fixed, max_atoms)
    con.prepare(np.array([[300, 301]]), None, _batch([300, 3]), 2, None, 256)      # a large molecule WITHOUT constraints is fine


def test_dynamics_refuses_bad_constraint_arguments_without_a_device():
    from newtonnet_amd import dynamics as dyn
    cpu = torch.device('cpu')
    pairs = torch.tensor([[0, 1]])
    for bad, kw, msg in (('bonds', {}, 'h-bonds'), ((pairs,), {}, 'h-bonds'), ((pairs.int(), None), {}, 'int64'),
                         ((pairs, torch.ones(1, dtype=torch.float64)), {}, 'float32'), ((pairs, torch.ones(2)), {}, 'float32'),
                         ((pairs, None), dict(tolerance=0.0), 'constraint_tolerance'),
                         ((pairs, None), dict(max_iter=0), 'constraint_max_iter')):
        with pytest.raises(ValueError, match=msg):
            dyn._check_constraint_arguments(bad, kw.get('tolerance', 1e-5), kw.get('max_iter', 150), cpu)
    dyn._check_constraint_arguments(None, -1.0, 0, cpu)                         # nothing is looked at without constraints
    dyn._check_constraint_arguments('h-bonds', 1e-5, 150, cpu)


@pytest.mark.parametrize('case, per_molecule', [('aspirin8_rand', [8] * 8), ('ethanol_and_aspirin', [6, 8])])
def test_hydrogen_constraints_on_the_md_fixtures(case, per_molecule):
    """(the ethanol is molecule 0 of ethanol4_rand, the one hessian_ref.ethanol_and_aspirin and mixed_rand use: the fixture's
    geometries are jittered by 0.1 A per coordinate, and in another of its four molecules one O-H is 1.46 A long, which the
    default max_length = 1.3 A rightly refuses)"""
    if case == 'ethanol_and_aspirin':
        from tests import hessian_ref as hr
        z, pos, cell, batch = hr.ethanol_and_aspirin()
    else:
        z, pos, cell, batch, _ = util.case_inputs(case, torch.float32)
    pairs, lengths = con.hydrogen_constraints(z, pos, batch)
    B = cell.shape[0]
    assert pairs.dtype == torch.int64 and lengths.dtype == torch.float32 and pairs.shape == (sum(per_molecule), 2)
    hydrogens = torch.nonzero(z == 1).reshape(-1)
    assert torch.equal(torch.sort(pairs[:, 1]).values, hydrogens)                # each H once
    assert bool((z[pairs[:, 0]] != 1).all()) and torch.equal(batch[pairs[:, 0]], batch[pairs[:, 1]])
    d = (pos[pairs[:, 0]] - pos[pairs[:, 1]]).double().norm(dim=1)
    assert torch.allclose(d, lengths.double(), rtol=1e-6) and float(lengths.max()) <= 1.3 and float(lengths.min()) > 0.8
    assert np.bincount(batch[pairs[:, 0]].numpy(), minlength=B).tolist() == per_molecule
    with pytest.raises(ValueError, match='no non-hydrogen partner within 0.5'):
        con.hydrogen_constraints(z, pos, batch, max_length=0.5)
    con.prepare(pairs.numpy(), lengths.numpy(), batch.numpy(), B, None, 256)


def test_hydrogen_constraints_on_the_whole_ethanol_fixture():
    """ethanol4_rand as it is: the default max_length refuses its 1.46 A O-H and says which atom; a larger one gives 6 pairs for
    each of the four molecules, every H once"""
    z, pos, cell, batch, _ = util.case_inputs('ethanol4_rand', torch.float32)
    with pytest.raises(ValueError, match=r'\(H\) has no non-hydrogen partner within 1.3 A \(the nearest is 1.46'):
        con.hydrogen_constraints(z, pos, batch)
    pairs, lengths = con.hydrogen_constraints(z, pos, batch, max_length=1.6)
    assert pairs.shape == (24, 2) and np.bincount(batch[pairs[:, 0]].numpy()).tolist() == [6] * 4
    assert torch.equal(torch.sort(pairs[:, 1]).values, torch.nonzero(z == 1).reshape(-1)) and float(lengths.max()) > 1.45


@pytest.mark.parametrize('name', ['water', 'mixed', 'water_fixed'])
@pytest.mark.parametrize('noise', [False, True])
def test_the_fp64_reference_keeps_constraints_and_momentum(name, noise):
    d = rr.case(name)
    T = d['T']
    ref = rr.run(d, rr.FINISH | rr.BEGIN, noise)
    assert not ref['failed'].any()
    x, v = ref['x'], ref['v']
    r, u = x[T.gi] - x[T.gj], v[T.gi] - v[T.gj]
    d2 = T.d2.astype(np.float64)
    assert np.all(np.abs((r * r).sum(1) - d2) <= 1e-12 * d2)
    assert np.all(np.abs((r * u).sum(1)) * d['dth'] <= 1e-12 * d2)
    if not noise and not d['fixed'].any():
        # constraint forces are internal: the momentum of a molecule changes by the two kicks alone.  The solver's masses are
        # 1 / w (w is the fp32 inverse mass it is given), so that is the mass the conserved sum is taken with
        m = 1.0 / d['w'].astype(np.float64)[:, None]
        dp = np.zeros((T.n_mol, 3))
        np.add.at(dp, d['batch'], m * (v - d['v'] - 2.0 * d['hk'].astype(np.float64)[:, None] * d['F']))
        scale = np.zeros(T.n_mol)
        np.add.at(scale, d['batch'], (m * np.abs(v)).sum(1))
        assert np.all(np.abs(dp).max(1) <= 1e-12 * np.maximum(scale, 1.0)), np.abs(dp).max()


def test_a_diatomic_with_velocity_along_the_bond_ends_with_none_of_it_along_the_bond():
    d = rr.case('diatomic')
    bond = (d['x'][1] - d['x'][0]).astype(np.float64)
    d['v'] = np.stack([-0.1 * bond, 0.3 * bond]).astype(np.float32)
    for flags, F in ((rr.PROJECT, None), (rr.FINISH, 0.0)):
        dd = dict(d, F=d['F'] * 0 if F is not None else d['F'])
        ref = rr.run(dd, flags, False)
        x = ref['x'] if ref['x'] is not None else d['x'].astype(np.float64)
        r, u = x[1] - x[0], ref['v'][1] - ref['v'][0]
        assert abs(r @ u) <= 1e-12 and not ref['failed'].any()
        # the centre-of-mass velocity is what is left of a motion purely along the bond
        m = d['m'].astype(np.float64)
        vcm = (m[:, None] * d['v']).sum(0) / m.sum()
        assert np.allclose(ref['v'], np.stack([vcm, vcm]), atol=1e-9)


def test_the_emulation_agrees_with_the_fp64_reference_within_the_bound():
    """the yardstick itself: the ratios written in rattle_ref are those the emulation gives (one case; the whole table is printed
    by `python -m tests.rattle_ref`)"""
    d = rr.case('ch4')
    for flags in (rr.FINISH, rr.BEGIN | rr.FINISH, rr.PROJECT):
        ref = rr.run(d, flags, False, bound_tol=rr.TOL)
        emu = rr.run(d, flags, False, fp32=True, tol=rr.TOL, max_iter=rr.MAX_ITER)
        raw, rel = rr.ratios(emu, ref, d['T'], flags, False)
        print(f'ch4 flags {flags}: emulation ratio to the summed response {raw}, err / bound {rel}')
        assert max(raw.values()) <= max(rr.EMULATION_RATIOS.values()) and max(rel.values()) <= 0.25 + 1e-9
        p_err, p_bound, v_err, v_bound = rr.stored_residuals(d['T'], emu['x'] if emu['x'] is not None else d['x'], emu['v'], rr.TOL, d['dth'])
        if flags != rr.FINISH:
            assert np.all(p_err <= p_bound)
        assert np.all(v_err <= v_bound)


def test_the_header_declares_the_entry_points_and_the_library_exports_them():
    from newtonnet_amd import hip
    for name in ('nnhip_md_step_constrained', 'nnhip_md_constrained_max_atoms'):
        assert name in abi.FUNCTIONS and name in hip.EXPORTED_SYMBOLS
    restype, argtypes = abi.FUNCTIONS['nnhip_md_step_constrained']
    assert restype is ctypes.c_int32 and len(argtypes) == 30
    assert [k for k, t in enumerate(argtypes) if t is ctypes.c_float] == [8, 9, 10, 23]
    assert abi.FUNCTIONS['nnhip_md_constrained_max_atoms'] == (ctypes.c_int32, [])
    for name, value in (('NNHIP_MDC_PROJECT', 4), ('NNHIP_MDC_MAX_ATOMS', 256)):
        assert abi.CONSTANTS[name] == value
    assert (hip.MDC_PROJECT, hip.MD_FINISH, hip.MD_BEGIN) == (rr.PROJECT, rr.FINISH, rr.BEGIN)
    assert os.path.exists(hip.LIB_PATH), 'build the library first (__graft_entry__.build())'
    lib = ctypes.CDLL(hip.LIB_PATH)
    assert hasattr(lib, 'nnhip_md_step_constrained') and lib.nnhip_md_constrained_max_atoms() == 256


def test_temperature_of_a_constrained_trajectory_uses_3n_minus_c():
    from newtonnet_amd.dynamics import K_BOLTZMANN, Trajectory
    ke = torch.tensor([[0.3, 0.5]])
    counts = torch.tensor([21, 9])
    traj = Trajectory(torch.zeros(1, dtype=torch.int64), None, None, torch.zeros(1, 2), ke, counts)
    assert torch.allclose(traj.temperature, 2.0 * ke / (3.0 * K_BOLTZMANN * counts.float()))             # as before
    traj._dof = (3 * counts - torch.tensor([8, 6])).float()
    assert torch.allclose(traj.temperature, 2.0 * ke / (K_BOLTZMANN * torch.tensor([55.0, 21.0])))
