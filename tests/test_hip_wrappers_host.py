"""CPU-side checks of the argument checks of the dynamics wrappers of newtonnet_amd/hip.py (md_step, npt_barostat, npt_step,
md_step_constrained, lbfgs_step, neb_step, remd_exchange, pimd_step, bias_step): every refusal of a tensor happens in Python, before
the library is touched, with the exception type callers rely on and the offending argument's name at the head of the message.

Each case starts from one valid set of CPU arguments and spoils exactly one of them: a tensor the kernel writes (wrong dtype, not
contiguous, wrong number of values, wrong device -- a `meta` tensor), a float32 input (float64) or an int32 offset table (wrong
dtype; a host copy of another length or off the CPU).  The library is replaced by a function that fails the test."""
import pytest
import torch

from newtonnet_amd import hip

N, B, G, M, P, CAP = 8, 4, 2, 2, 2, 3       # atoms, molecules, groups (bands, ladders), L-BFGS memory, beads, hill capacity


def _f(*shape):
    return torch.zeros(*shape)


def _i(*shape):
    return torch.zeros(*shape, dtype=torch.int32)


def _ptr(*values):
    return torch.tensor(values, dtype=torch.int32)


MOL_PTR = (0, 2, 4, 6, 8)
GROUP_PTR = (0, 2, 4)


def _md_args():
    return dict(pos_in=_f(N, 3), vel=_f(N, 3), force=_f(N, 3), hk=_f(N), dth=0.1, c1=1.0, flags=3, pos_out=_f(N, 3), mass=_f(N),
                sigma=_f(N), noise=_f(N, 3), ke_out=_f(N))


def _constrained_call(d):
    d = dict(d)
    tables = hip.ConstraintTables(*(d.pop(k) for k in hip.ConstraintTables._fields))
    return hip.md_step_constrained(tables=tables, **d)


# name: (call, valid arguments, written tensors, the argument the device is taken from, float32 inputs, (table, host copy) pairs)
WRAPPERS = {
    'md_step': (
        lambda d: hip.md_step(**d), _md_args,
        ('vel', 'pos_out', 'ke_out'), 'vel', ('pos_in', 'force', 'hk', 'mass', 'sigma', 'noise'), ()),
    'npt_barostat': (
        lambda d: hip.npt_barostat(**d),
        lambda: dict(vel=_f(N, 3), mass=_f(N), mol_ptr=_ptr(*MOL_PTR), cell_in=_f(B, 3, 3), virial=_f(B, 3, 3), a=_f(B), p0=_f(B),
                     cell_out=_f(B, 3, 3), mu=_f(B), inv_mu=_f(B), ke=_f(B), pressure=_f(B), volume=_f(B), deps=_f(B),
                     force=_f(N, 3), hk=_f(N), s2=_f(B), noise=_f(B)),
        ('cell_out', 'mu', 'inv_mu', 'ke', 'pressure', 'volume', 'deps'), 'vel',
        ('vel', 'mass', 'cell_in', 'virial', 'a', 'p0', 'force', 'hk', 's2', 'noise'), (('mol_ptr', None),)),
    'npt_step': (
        lambda d: hip.npt_step(**d),
        lambda: dict(_md_args(), mu=_f(B), inv_mu=_f(B), mol_of_atom=_i(N)),
        ('vel', 'pos_out', 'ke_out'), 'vel', ('pos_in', 'force', 'hk', 'mass', 'sigma', 'noise', 'mu', 'inv_mu'),
        (('mol_of_atom', None),)),
    'md_step_constrained': (
        _constrained_call,
        lambda: dict(pos_in=_f(N, 3), vel=_f(N, 3), force=_f(N, 3), hk=_f(N), inv_mass=_f(N), dth=0.1, inv_dth=10.0, c1=1.0, flags=3,
                     mol_ptr=_ptr(*MOL_PTR), mol_ptr_host=_ptr(*MOL_PTR), mol_col_ptr=_ptr(0, 1, 2, 2, 2),
                     mol_col_ptr_host=_ptr(0, 1, 2, 2, 2), col_ptr=_ptr(0, 1, 2), col_ptr_host=_ptr(0, 1, 2), con_pair=_i(2, 2),
                     con_d2=_f(2), tol=1e-6, max_iter=10, n_failed=_i(B), n_sweeps=_i(B), pos_out=_f(N, 3), mass=_f(N), sigma=_f(N),
                     noise=_f(N, 3), ke_out=_f(N)),
        ('vel', 'pos_out', 'ke_out', 'n_failed', 'n_sweeps'), 'vel', ('pos_in', 'force', 'hk', 'mass', 'inv_mass', 'sigma', 'noise'),
        (('mol_ptr', 'mol_ptr_host'), ('mol_col_ptr', 'mol_col_ptr_host'), ('col_ptr', 'col_ptr_host'))),
    'lbfgs_step': (
        lambda d: hip.lbfgs_step(**d),
        lambda: dict(pos_in=_f(N, 3), force=_f(N, 3), free=torch.ones(N, dtype=torch.bool), mol_ptr=_ptr(*MOL_PTR), memory=M,
                     tol2=1e-4, alpha=70.0, maxstep=0.2, flags=0, converged=_i(B), n_steps=_i(B), n_pairs=_i(B), head=_i(B),
                     S=_f(M, N, 3), Y=_f(M, N, 3), rho=_f(B, M), f_prev=_f(N, 3), work=_f(N, 3), pos_out=_f(N, 3), fmax_out=_f(B)),
        ('converged', 'n_steps', 'n_pairs', 'head', 'S', 'Y', 'rho', 'f_prev', 'work', 'pos_out', 'fmax_out'), 'mol_ptr',
        ('pos_in', 'force'), (('mol_ptr', None),)),
    'neb_step': (
        lambda d: hip.neb_step(**d),
        lambda: dict(pos_in=_f(N, 3), force=_f(N, 3), energy=_f(B), free=None, mol_ptr=_ptr(*MOL_PTR), band_ptr=_ptr(*GROUP_PTR),
                     band_ptr_host=_ptr(*GROUP_PTR), spring=0.1, tol2=1e-4, climb2=1e-2, fire=hip.NEB_FIRE_DEFAULTS, flags=0,
                     converged=_i(G), climbing=_i(G), n_steps=_i(G), n_pos=_i(G), dt=_f(G), a=_f(G), vel=_f(N, 3), pos_out=_f(N, 3),
                     neb_force_out=_f(N, 3), tangent_out=_f(N, 3), fmax_out=_f(G), saddle_out=_i(G)),
        ('converged', 'climbing', 'n_steps', 'n_pos', 'dt', 'a', 'vel', 'pos_out', 'neb_force_out', 'tangent_out', 'fmax_out',
         'saddle_out'), 'mol_ptr', ('pos_in', 'force', 'energy'), (('mol_ptr', None), ('band_ptr', 'band_ptr_host'))),
    'remd_exchange': (
        lambda d: hip.remd_exchange(**d),
        lambda: dict(energy=_f(B), mol_ptr=_ptr(*MOL_PTR), mol_ptr_host=_ptr(*MOL_PTR), ladder_ptr=_ptr(*GROUP_PTR),
                     ladder_ptr_host=_ptr(*GROUP_PTR), stream_id=_i(G), dbeta=_f(B), scale_up=_f(B), scale_down=_f(B),
                     sigma_table=_f(2, N), rank_of_slot=_i(B), slot_of_rank=_i(B), vel=_f(N, 3), sigma=_f(N), n_attempt=_i(B),
                     n_accept=_i(B), attempt=0, seed=1, delta_out=_f(B), u_out=_f(B), accepted_out=_i(B)),
        ('rank_of_slot', 'slot_of_rank', 'n_attempt', 'n_accept', 'vel', 'sigma', 'delta_out', 'u_out', 'accepted_out'), 'mol_ptr',
        ('energy', 'dbeta', 'scale_up', 'scale_down', 'sigma_table'),
        (('mol_ptr', 'mol_ptr_host'), ('ladder_ptr', 'ladder_ptr_host'))),
    'pimd_step': (
        lambda d: hip.pimd_step(**d),
        lambda: dict(u=_f(N, 3), w=_f(N, 3), force=_f(N, 3), ctab=_f(P, P), mode_tab=_f(B, 5), hk=_f(N), mol_ptr=_ptr(*MOL_PTR),
                     mol_ptr_host=_ptr(*MOL_PTR), n_beads=P, flags=3, pos_out=_f(N, 3), pos_pending=_f(N, 3), mass=_f(N),
                     sigma=_f(N), noise=_f(N, 3), est_out=_f(N, 4)),
        ('u', 'w', 'pos_out', 'est_out'), 'u', ('force', 'ctab', 'mode_tab', 'hk', 'mass', 'sigma', 'noise', 'pos_pending'),
        (('mol_ptr', 'mol_ptr_host'),)),
    'bias_step': (
        lambda d: hip.bias_step(**d),
        lambda: dict(pos=_f(N, 3), force_in=_f(N, 3), mol_ptr=_ptr(*MOL_PTR), mol_ptr_host=_ptr(*MOL_PTR),
                     group_ptr=_ptr(*GROUP_PTR), group_ptr_host=_ptr(*GROUP_PTR), cv_def=_i(B, hip.BIAS_MAX_CVS, 5),
                     restraint=_f(B, hip.BIAS_MAX_CVS, 2), hill_par=_f(G, 4), hills=_f(G, CAP, 4), n_deposits=0, flags=0,
                     force_out=_f(N, 3), cv_out=_f(B, 2), bias_out=_f(B, 2), status_out=_i(B)),
        ('hills', 'force_out', 'cv_out', 'bias_out', 'status_out'), 'mol_ptr', ('pos', 'force_in', 'restraint', 'hill_par'),
        (('mol_ptr', 'mol_ptr_host'), ('group_ptr', 'group_ptr_host'))),
}


def _wider(t):
    """the same leading shape with one more value per row: another number of values, whichever argument the sizes are read from"""
    return torch.zeros(t.shape[:-1] + (t.shape[-1] + 1,), dtype=t.dtype)


def _strided(t):
    s = torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype)[..., ::2]
    assert s.shape == t.shape and not s.is_contiguous()
    return s


def _other_dtype(t):
    return t.to(torch.float64 if t.dtype == torch.float32 else torch.int64)


def _on_meta(t):
    return torch.empty_like(t, device='meta')


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    def reached():
        raise AssertionError('the wrapper reached the library: a refusal in Python was expected before')
    monkeypatch.setattr(hip, 'lib', reached)


def _refused(wrapper, name, spoil, error):
    call, make = WRAPPERS[wrapper][:2]
    d = make()
    d[name] = spoil(d[name])
    with pytest.raises(error, match=rf'^{name}\b'):
        call(d)


@pytest.mark.parametrize('wrapper', WRAPPERS)
def test_written_tensors(wrapper):
    written, device_from = WRAPPERS[wrapper][2:4]
    for name in written:
        for spoil in (_other_dtype, _strided, _wider):
            _refused(wrapper, name, spoil, ValueError)
        if name != device_from:
            _refused(wrapper, name, _on_meta, ValueError)


@pytest.mark.parametrize('wrapper', WRAPPERS)
def test_float64_inputs(wrapper):
    for name in WRAPPERS[wrapper][4]:
        _refused(wrapper, name, _other_dtype, NotImplementedError)


@pytest.mark.parametrize('wrapper', WRAPPERS)
def test_offset_tables(wrapper):
    for table, host in WRAPPERS[wrapper][5]:
        _refused(wrapper, table, _other_dtype, ValueError)
        if host is not None:
            _refused(wrapper, host, _other_dtype, ValueError)
            _refused(wrapper, host, _wider, ValueError)
            _refused(wrapper, host, _on_meta, ValueError)


@pytest.mark.parametrize('wrapper', WRAPPERS)
def test_valid_arguments_reach_the_library(wrapper):
    """the unspoiled arguments pass every check: each refusal above is the spoiled argument's"""
    call, make = WRAPPERS[wrapper][:2]
    with pytest.raises(AssertionError, match='reached the library'):
        call(make())
