"""Batched nudged-elastic-band saddle search on the HIP path: every image of every band is one molecule of ONE model() call, and
one launch (nnhip_neb_step, csrc/neb.hip) per step forms the tangents and the NEB forces of all bands and moves each band by one
FIRE step, with no host round trip of positions, forces or energies.

The reference leaves path searches to an outside driver that calls its calculator once per image per step.  Here
`Band` owns the positions and the FIRE state of K bands as device tensors.  The method is the improved-tangent NEB of Henkelman and
Jonsson (2000) with one spring constant and the climbing image of Henkelman, Uberuaga and Jonsson (2000), optimised by FIRE as
ase.optimize.FIRE states it (mass 1, ASE's constants, one step length per band).  The climbing image is switched on per band when
the band's NEB fmax falls below `climb_below` and a band converges when it falls below `fmax` with the climbing image on; both
flags are sticky.  A converged band is frozen -- later launches leave every bit of it alone -- but model() keeps evaluating it
with the rest of the batch, endpoints included.

Not done here: removal of rotation / translation of free molecules, IDPP interpolation, minimum-image tangents (a periodic path
must be given unwrapped and continuous), variable springs, the dimer method or any Hessian-based refinement.

The barrier a BandResult reports is a difference of two fp32 energies: it is resolved to one fp32 ulp of |E|, 2 meV for aspirin with
the shipped per-element shifts (|E| = 1.76e4 eV).  The kernel itself uses the energies only in comparisons and in differences of
neighbouring images, so the search is not affected.

Units: positions in Angstrom, energies in eV, forces and fmax in eV / Angstrom, spring in eV / Angstrom^2."""
from __future__ import annotations

import math

import numpy as np
import torch

from newtonnet_amd import hip
from newtonnet_amd.dynamics import _mol_ptr
from newtonnet_amd.relax import check_inputs
from newtonnet_amd.stepper import Stepper

FIRE_N_MIN, FIRE_F_INC, FIRE_F_DEC, FIRE_A_START, FIRE_F_A = hip.NEB_FIRE_DEFAULTS[2:7]


class BandResult:
    """What Band.run returns, as device tensors (B images, K bands, N atoms):

    pos         fp32 [N,3]   positions after the last step;   energy fp32 [B]: the model's energy of every image there
    neb_force, tangent  fp32 [N,3]   the NEB force and the unit tangent of every image there (endpoints: 0)
    fmax        fp32 [K]     the largest NEB force norm on a free atom of an interior image
    converged, climbing  bool [K]   the sticky flags;   n_steps int64 [K]: FIRE steps taken
    saddle_image  int64 [K]  molecule index of the interior image of highest energy (the climbing image)
    barrier_forward, barrier_reverse  fp32 [K]   its fp32 energy minus that of the band's first / last image
    traj_*      only with record_every > 0, over the R recorded steps: traj_step int64 [R], traj_pos and traj_force fp32 [R,N,3]
                (the model's forces at those positions), traj_energy fp32 [R,B], traj_dt fp32 [R,K] (each band's FIRE step length
                after that step)
    """

    def __init__(self, **kw):
        self.traj_step = self.traj_pos = self.traj_force = self.traj_energy = self.traj_dt = None
        self.__dict__.update(kw)


def band_counts(n_images, n_mol):
    """images per band as a list of ints, refused without touching the device: an int (every band that many) or one per band"""
    if isinstance(n_images, (int, np.integer)) and not isinstance(n_images, bool):
        if n_images < 3 or n_mol % int(n_images):
            raise ValueError(f'n_images: {n_mol} molecules do not split into bands of {n_images} images (at least 3 each)')
        counts = [int(n_images)] * (n_mol // int(n_images))
    else:
        try:
            counts = [int(c) for c in n_images]
            exact = all(c == v for c, v in zip(counts, n_images))
        except (TypeError, ValueError):
            raise ValueError(f'n_images: an int or one int per band expected (got {n_images!r})') from None
        if not exact or not counts or sum(counts) != n_mol:
            raise ValueError(f'n_images: integer counts that add up to the {n_mol} molecules of the batch expected (got {n_images!r})')
    for c in counts:
        if not 3 <= c <= hip.NEB_MAX_IMAGES:
            raise ValueError(f'n_images: 3 .. {hip.NEB_MAX_IMAGES} images per band expected (got {c})')
    return counts


def check_arguments(spring, fmax, climb_below, dt, dt_max, maxstep):
    """the method's numbers, refused without touching the device; returns them as floats (climb_below None: 5 fmax)"""
    out = []
    for name, v in (('spring', spring), ('fmax', fmax), ('climb_below', climb_below), ('dt', dt), ('dt_max', dt_max),
                    ('maxstep', maxstep)):
        if name == 'climb_below' and v is None:
            v = 5.0 * out[1]
        try:
            v = float(v)
        except (TypeError, ValueError):
            raise ValueError(f'{name}: a number expected (got {v!r})') from None
        if not (v > 0.0 and math.isfinite(v)):
            raise ValueError(f'{name}: a finite value > 0 expected (got {v!r})')
        out.append(v)
    if out[3] > out[4]:
        raise ValueError(f'dt: at most dt_max = {out[4]} expected (got {out[3]})')
    return tuple(out)


def interpolate(pos_a: torch.Tensor, pos_b: torch.Tensor, n_images: int) -> torch.Tensor:
    """Linear images between two geometries, on their device: [n_images, n, 3] with image 0 = pos_a and the last = pos_b, both
    bitwise.  No minimum image is taken: give a periodic pair unwrapped."""
    if not isinstance(pos_a, torch.Tensor) or not isinstance(pos_b, torch.Tensor) or pos_a.shape != pos_b.shape \
            or pos_a.dim() != 2 or pos_a.shape[1] != 3:
        raise ValueError('interpolate: two [n,3] tensors of the same shape expected')
    if int(n_images) != n_images or not 3 <= n_images <= hip.NEB_MAX_IMAGES:
        raise ValueError(f'n_images: an integer in 3 .. {hip.NEB_MAX_IMAGES} expected (got {n_images!r})')
    n_images = int(n_images)
    w = torch.arange(n_images, dtype=pos_a.dtype, device=pos_a.device).view(-1, 1, 1) / (n_images - 1)
    out = pos_a.unsqueeze(0) + w * (pos_b - pos_a).unsqueeze(0)
    out[0], out[-1] = pos_a, pos_b
    return out


class Band(Stepper):
    """K bands optimised together on the device.

    model: a NewtonNet in eval mode with the 'energy' and 'gradient_force' heads.  z, pos, cell, batch: as for model(...), on the
    device, the images of a band being consecutive molecules in path order; none of them is modified.  n_images: images per band,
    an int or one per band (3 .. hip.NEB_MAX_IMAGES; the first and last image of a band are its fixed endpoints).  spring: the
    spring constant.  fmax: a band has converged when the largest NEB force norm on a free atom of its interior images is below
    it (compared as squares in fp32).  climb: use a climbing image, switched on below climb_below (None: 5 fmax).  fixed: bool
    [N], atoms that never move.  dt, dt_max, maxstep: FIRE's first and largest step length and the cap on the length of a band's
    step; its other constants are ASE's."""
    NOUN, CHECK_ONLY = 'band searches', hip.NEB_CHECK_ONLY
    TRAJ = (('pos', ('n_atoms', 3), torch.float32), ('force', ('n_atoms', 3), torch.float32), ('energy', ('n_mol',), torch.float32),
            ('dt', ('n_bands',), torch.float32))

    def __init__(self, model, z, pos, cell, batch, n_images, spring=0.1, fmax=0.05, climb=True, climb_below=None, fixed=None,
                 dt=0.1, dt_max=1.0, maxstep=0.2):
        # ---- everything that can be refused without touching the device
        N, B = check_inputs(model, 'Band', z, pos, cell, batch, fixed)
        counts = band_counts(n_images, B)
        spring, fmax, climb_below, dt, dt_max, maxstep = check_arguments(spring, fmax, climb_below, dt, dt_max, maxstep)
        dev = self._check_device(pos, z=z, cell=cell, batch=batch, fixed=fixed)
        # ---- state
        self.model, self.z, self.cell, self.batch = model, z, cell, batch
        self.n_atoms, self.n_mol, self.n_bands = N, B, len(counts)
        self.fmax, self.climb_below, self.spring, self.climb = fmax, climb_below, spring, bool(climb)
        f32 = np.float32
        # the numbers the kernel gets, as the Python floats of their fp32 values
        self._spring, self._tol2, self._climb2 = float(f32(spring)), float(f32(fmax * fmax)), float(f32(climb_below * climb_below))
        self._fire = (float(f32(dt)), float(f32(dt_max)), int(FIRE_N_MIN), float(f32(FIRE_F_INC)), float(f32(FIRE_F_DEC)),
                      float(f32(FIRE_A_START)), float(f32(FIRE_F_A)), float(f32(maxstep)))
        self._flags = hip.NEB_CLIMB if climb else 0
        K = self.n_bands
        with torch.no_grad():
            self._band_ptr_host = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)
            self._band_ptr = self._band_ptr_host.to(dev)
            self._mol_ptr = _mol_ptr(batch, B)
            sizes = np.diff(self._mol_ptr.cpu().numpy())
            for k in range(K):
                s = sizes[int(self._band_ptr_host[k]):int(self._band_ptr_host[k + 1])]
                if (s != s[0]).any():
                    raise ValueError(f'band {k}: its images have different atom counts ({s.tolist()})')
            self._free = None if fixed is None else (~fixed).contiguous()
            self._init_buffers(pos.detach().clone().contiguous())

            def ints():
                return torch.zeros(K, dtype=torch.int32, device=dev)
            self._converged, self._climbing, self._n_steps, self._n_pos, self._saddle = ints(), ints(), ints(), ints(), ints()
            self._active = self._converged
            self._dt = torch.zeros(K, dtype=torch.float32, device=dev)
            self._a = torch.zeros(K, dtype=torch.float32, device=dev)
            self._vel = torch.zeros(N, 3, dtype=torch.float32, device=dev)
            self._neb_force = torch.zeros(N, 3, dtype=torch.float32, device=dev)
            self._tangent = torch.zeros(N, 3, dtype=torch.float32, device=dev)
            self._fmax = torch.zeros(K, dtype=torch.float32, device=dev)

    # ------------------------------------------------------------------------------------------
    def _launch(self, flags=0):
        """one launch: reads the current buffer, forces and energies, writes the other buffer, and the buffers swap"""
        other = 1 - self._cur
        hip.neb_step(self._pos[self._cur], self._force, self._energy, self._free, self._mol_ptr, self._band_ptr, self._band_ptr_host,
                     self._spring, self._tol2, self._climb2, self._fire, self._flags | flags, self._converged, self._climbing,
                     self._n_steps, self._n_pos, self._dt, self._a, self._vel, self._pos[other], self._neb_force, self._tangent,
                     self._fmax, self._saddle)
        self._cur = other

    # ------------------------------------------------------------------------------------------
    # run (Stepper.run): FIRE steps of every band that has not converged; the check-only launch forms the NEB forces, the tangents
    # and fmax at the positions reached, moves nothing and sets no flag
    def _frame(self):
        return self._pos[self._cur].clone(), self._force.clone(), self._energy.clone(), self._dt.clone()

    def _result(self):
        saddle = self._saddle.long()
        first, last = self._band_ptr[:-1].long(), self._band_ptr[1:].long() - 1
        e = self._energy
        return BandResult(pos=self._pos[self._cur].clone(), energy=e.clone(), neb_force=self._neb_force.clone(),
                          tangent=self._tangent.clone(), fmax=self._fmax.clone(), converged=self._converged != 0,
                          climbing=self._climbing != 0, n_steps=self._n_steps.long(), saddle_image=saddle,
                          barrier_forward=e[saddle] - e[first], barrier_reverse=e[saddle] - e[last])
