"""Mode Grueneisen parameters and thermal expansion of crystals on the HIP path: the first anharmonic quantities of the phonon line.

gamma_k(q, s) = -(1 / (2 lambda)) d lambda / d eta_k, the logarithmic slope of the frequency of mode s at wave vector q along the strain
parameter eta_k (ln V for strain='volume', the six Voigt components for strain='voigt').  By Hellmann-Feynman
d lambda / d eta_k = e^H (dD / d eta_k) e, and D is linear in the force constants, so dD / d eta_k is D's own sum over a plane
dPhi / d eta_k of force-constant derivatives: ONE launch of nnhip_phonon_strain_slopes (csrc/phonon_gruneisen.hip) takes the slopes of
every mode of every (crystal, q) problem and every plane from the modes either solver left on the device, with degenerate
perturbation theory inside groups of (nearly) equal eigenvalues along a split plane sum_k w_k dPhi / d eta_k.

dPhi / d eta_k needs the third derivative of the energy, which no pass of the library gives: it is a CENTRAL DIFFERENCE of the analytic
force constants at two strained cells, dfc_k = (Phi(+delta) - Phi(-delta)) / (2 delta), formed in fp64 and rounded once to fp32.
The central crystal's image table serves every plane: in units of the lattice vectors it does not move under affine strain, and a tie
that strain breaks is shared among the central images, which is the first-order statement.

From the slopes: GruneisenMesh.mean(T), the thermodynamic Grueneisen parameter sum c_v gamma / sum c_v, and
GruneisenMesh.thermal_expansion(T, elastic), alpha_V = sum c_v gamma / (Q V B) (volume form) or alpha_I = (1 / (Q V)) sum_J S_IJ sum c_v
gamma_J (Voigt form) with the bulk modulus / compliance of an elastic.ElasticConstants, in 1 / K.

Limits, as they are.  The derivative is a central difference in strain of analytic force constants: its error is O(delta^2) plus the
fp32 noise of the force constants divided by delta.  The ions follow the strain affinely: exact for crystals whose atoms sit on
symmetry-fixed sites, otherwise the clamped-ion value; Gruneisen.from_phonons, fed with Phonons of cells whose ions were relaxed at
each strain, is the way to relaxed ions.  Not built: the full quasi-harmonic volume scan, third-order force constants and lifetimes.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from newtonnet_amd import elastic as _el
from newtonnet_amd import hip
from newtonnet_amd import phonons as _ph
from newtonnet_amd import vibrations as _v

MAX_PLANES = 6          # strain planes one launch of nnhip_phonon_strain_slopes takes
EPS32 = _ph.EPS32


# ---- host helpers (numpy, fp64) ----------------------------------------------------------------------------------------------

def _check_delta(delta) -> float:
    if not (isinstance(delta, (int, float, np.floating, np.integer)) and math.isfinite(float(delta)) and float(delta) > 0.0):
        raise ValueError(f'delta: a finite strain step > 0 expected (got {delta!r})')
    return float(delta)


def strain_matrices(strain) -> np.ndarray:
    """fp64 [K, 3, 3]: the symmetric strain directions of `strain` -- 'volume': I / 3 (eta = ln V); 'voigt': the six unit Voigt
    strains of elastic.voigt_matrices (engineering shears); an array [K, 3, 3] (or [3, 3]) of symmetric matrices, K <= 6."""
    if isinstance(strain, str):
        if strain == 'volume':
            return np.eye(3)[None] / 3.0
        if strain == 'voigt':
            return _el.voigt_matrices(np.eye(6))
        raise ValueError(f"strain: 'volume', 'voigt' or symmetric matrices [K, 3, 3] expected (got {strain!r})")
    e = strain.detach().double().cpu().numpy() if isinstance(strain, torch.Tensor) else np.asarray(strain, dtype=np.float64)
    if e.shape == (3, 3):
        e = e[None]
    if e.ndim != 3 or e.shape[1:] != (3, 3) or e.shape[0] < 1 or not np.isfinite(e).all():
        raise ValueError(f"strain: 'volume', 'voigt' or finite symmetric matrices [K, 3, 3] expected (got shape {tuple(e.shape)})")
    if e.shape[0] > MAX_PLANES:
        raise ValueError(f'strain: at most {MAX_PLANES} strains in one call (got {e.shape[0]})')
    for k in range(len(e)):
        if np.abs(e[k] - e[k].T).max() > 1e-12 * max(np.abs(e[k]).max(), 1e-300):
            raise ValueError(f'strain: matrix {k} is not symmetric')
    return np.ascontiguousarray(e)


def _form(strain) -> str:
    return strain if isinstance(strain, str) else 'custom'


def strained_crystals(pos, cell, batch, strain='volume', delta: float = 0.01, dtype=torch.float32):
    """The 2 K strained copies of B crystals (pos [N, 3], cell [B, 3, 3], batch [N]; tensors or arrays).  Host, fp64, rounded once
    to `dtype` (fp32, what the model takes; torch.float64 keeps the construction as it is).  Returns (strains fp64 [K, 3, 3], copies):
    copies[k] = ((pos-, cell-, Q-), (pos+, cell+, Q+)), pos and cell tensors on the device of pos (CPU for arrays), Q fp64 numpy
    [B, 3, 3] the rotation back.
      'volume' (default): F = exp(+-delta / 3) I, pos' = pos F, cell' = cell F: ln V moves by exactly +-delta, a symmetric cell stays
        symmetric, Q = I.
      'voigt' / explicit matrices: F = I +- delta eps_k.  cell F is in general not symmetric, which phonons() requires, so the
        strained crystal is rotated with phonons.symmetric_cell: cell' = cell F Q^T, pos' = pos F Q^T.  Force constants computed in the
        rotated frame go back per 3 x 3 block as Phi = Q^T Phi_rot Q (rotate_back)."""
    delta = _check_delta(delta)
    eps = strain_matrices(strain)
    dev = pos.device if isinstance(pos, torch.Tensor) else torch.device('cpu')
    pos_h = pos.detach().double().cpu().numpy() if isinstance(pos, torch.Tensor) else np.asarray(pos, dtype=np.float64)
    cell_h = cell.detach().double().cpu().numpy() if isinstance(cell, torch.Tensor) else np.asarray(cell, dtype=np.float64)
    b_h = batch.detach().cpu().numpy() if isinstance(batch, torch.Tensor) else np.asarray(batch)
    pos_h, cell_h, b_h = pos_h.reshape(-1, 3), cell_h.reshape(-1, 3, 3), b_h.reshape(-1).astype(np.int64)
    B = len(cell_h)
    volume = isinstance(strain, str) and strain == 'volume'
    copies = []
    for k in range(len(eps)):
        pair = []
        for sign in (-1.0, 1.0):
            F = math.exp(sign * delta / 3.0) * np.eye(3) if volume else np.eye(3) + sign * delta * eps[k]
            p, c, Q = np.empty_like(pos_h), np.empty_like(cell_h), np.tile(np.eye(3), (B, 1, 1))
            for b in range(B):
                sel = b_h == b
                if volume:
                    p[sel], c[b] = pos_h[sel] @ F, cell_h[b] @ F
                else:
                    cs = cell_h[b] @ F
                    p[sel], c[b] = _ph.symmetric_cell(pos_h[sel] @ F, cs)
                    u, _, vh = np.linalg.svd(cs)
                    Q[b] = u @ vh
            pair.append((torch.tensor(p, dtype=dtype).to(dev), torch.tensor(c, dtype=dtype).to(dev), Q))
        copies.append(tuple(pair))
    return eps, copies


def rotate_back(fc: torch.Tensor, Q, counts, sc_counts) -> torch.Tensor:
    """fp64, packed like fc: Phi = Q_b^T Phi_rot Q_b on every 3 x 3 block of crystal b (fc packed [n_b, 3, N_b, 3] per crystal, computed
    in the frame r' = r Q_b^T)."""
    out, o = [], 0
    for b, (n, N) in enumerate(zip(counts, sc_counts)):
        q = torch.tensor(np.asarray(Q[b], dtype=np.float64), dtype=torch.float64).to(fc.device)
        phi = fc[o:o + 9 * n * N].double().view(n, 3, N, 3)
        out.append(torch.einsum('ca,icJd,db->iaJb', q, phi, q).reshape(-1))
        o += 9 * n * N
    return torch.cat(out) if out else fc.double()


def _split_weights(w, K: int) -> np.ndarray:
    w = np.ones(K) if w is None else np.asarray(w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else w, dtype=np.float64)
    if w.shape != (K,) or not np.isfinite(w).all() or not (np.linalg.norm(w) > 0.0):
        raise ValueError(f'split_weights: {K} finite weights, not all zero, expected (got {w!r})')
    return w / np.linalg.norm(w)


def _heat_capacity(ev: torch.Tensor, live: torch.Tensor, T: float) -> torch.Tensor:
    """fp64 per mode, eV / K: the harmonic c_v of the live modes (zero elsewhere), the formula of PhononMesh.transport_tensor"""
    if T == 0.0:
        return torch.zeros_like(ev)
    eps = _v.EV_PER_SQRT_EIGENVALUE * torch.where(live, ev, torch.ones_like(ev)).sqrt()
    x = (eps / (_v.K_BOLTZMANN * T)).clamp(max=100.0)
    em, om = torch.exp(-x), -torch.expm1(-x)
    return torch.where(live, _v.K_BOLTZMANN * x * x * em / (om * om), torch.zeros_like(ev))


# ---- results -------------------------------------------------------------------------------------------------------------------

class GruneisenBands(_ph.PhononBands):
    """A PhononBands (bitwise what Phonons.frequencies returns) with, for K strain planes:

    gruneisen                    fp32 [Q sum d_b, K]  gamma_k = -(d lambda / d eta_k) / (2 lambda); 0 where not defined
    eigenvalue_strain_gradients  fp32 [Q sum d_b, K]  d lambda / d eta_k, eV / (A^2 amu) per unit strain parameter (also for a zero mode;
                                 zero for a group above MAX_DEGENERATE)
    gruneisen_defined            bool [Q sum d_b]     False for |lambda| <= the zero tolerance (the acoustic modes at Gamma) and for the
                                 modes of a group above phonons.MAX_DEGENERATE (status bit 3)
    degenerate_group             int32 [Q sum d_b]    per mode, the index of the first mode of its group
    Modes whose eigenvalues lie within the degeneracy tolerance of each other are rotated so that the split plane's perturbation is
    diagonal (ascending); inside a subgroup it leaves degenerate only the sum over the subgroup is defined."""

    def __init__(self, **kw):
        self.gruneisen = None
        self.eigenvalue_strain_gradients = None
        self.gruneisen_defined = None
        super().__init__(**kw)

    def gruneisen_parameters(self, b: int):
        """(gamma [Q, d, K], defined [Q, d]) of crystal b: views."""
        if self.gruneisen is None:
            raise ValueError('no gruneisen parameters: these bands were not made by a Gruneisen object')
        Q, d, o = len(self.q), self._dims[b], self._offsets[b]
        K = self.gruneisen.shape[1]
        return self.gruneisen[Q * o:Q * (o + d)].view(Q, d, K), self.gruneisen_defined[Q * o:Q * (o + d)].view(Q, d)

    def strain_gradients(self, b: int):
        """d lambda / d eta [Q, d, K] of crystal b: a view."""
        if self.eigenvalue_strain_gradients is None:
            raise ValueError('no gruneisen parameters: these bands were not made by a Gruneisen object')
        Q, d, o = len(self.q), self._dims[b], self._offsets[b]
        return self.eigenvalue_strain_gradients[Q * o:Q * (o + d)].view(Q, d, -1)


class GruneisenMesh(_ph.PhononMesh):
    """The spectra and mode Grueneisen parameters of a regular mesh (Gruneisen.mesh): a PhononMesh (dos, thermochemistry, threshold)
    whose `bands` is a GruneisenBands.  `form`: 'volume', 'voigt' or 'custom' (what the K planes are)."""

    def __init__(self, bands, phonons, form: str = 'custom'):
        super().__init__(bands, phonons)
        self.form = form

    def _sums(self, T: float, tol_zero):
        """(sum c_v gamma_k fp64 [B, K], sum c_v fp64 [B]) over the live (lambda > threshold) and defined modes of the mesh"""
        bands, ph = self.bands, self._ph
        if getattr(bands, 'gruneisen', None) is None:
            raise ValueError('gruneisen: this mesh holds no Grueneisen parameters: make it with Gruneisen.mesh')
        thr = self.threshold(tol_zero)
        K, dev = bands.gruneisen.shape[1], bands.eigenvalues.device
        num, den = [], []
        for b in range(len(ph.counts)):
            ev = bands.crystal(b)[0].reshape(-1).double()
            gam, ok = bands.gruneisen_parameters(b)
            live = (ev > thr[b]) & ok.reshape(-1)
            cv = _heat_capacity(ev, live, T)
            num.append((cv[:, None] * gam.reshape(-1, K).double()).sum(dim=0))
            den.append(cv.sum())
        if not num:
            return torch.zeros(0, K, dtype=torch.float64, device=dev), torch.zeros(0, dtype=torch.float64, device=dev)
        return torch.stack(num), torch.stack(den)

    def mean(self, temperature: float, tol_zero: Optional[float] = None) -> torch.Tensor:
        """fp32 [B, K]: the thermodynamic Grueneisen parameter gamma_k(T) = sum c_v gamma_k / sum c_v over the live modes (lambda >
        threshold(tol_zero)) whose gamma is defined.  fp64 torch ops on the device.  T = 0 has no heat capacity to weigh with:
        ValueError."""
        T = _v._temperature(temperature)
        if T == 0.0:
            raise ValueError('temperature: the mean Grueneisen parameter is a ratio of heat capacities, which vanish at T = 0')
        num, den = self._sums(T, tol_zero)
        return (num / den[:, None]).float()

    def thermal_expansion(self, temperature: float, elastic=None, tol_zero: Optional[float] = None) -> torch.Tensor:
        """The thermal expansion coefficient in 1 / K at `temperature` (K), fp64 torch ops on the device.
        form 'volume': fp32 [B], alpha_V = sum c_v gamma / (Q V B_Voigt), B_Voigt = elastic.bulk_modulus()[0], the second derivative
        of the energy under uniform scaling.  form 'voigt': fp32 [B, 6], alpha_I = (1 / (Q V)) sum_J S_IJ sum c_v gamma_J with S =
        elastic.compliance() (engineering shears; alpha_V = alpha_1 + alpha_2 + alpha_3).  elastic: an elastic.ElasticConstants or a
        [B, 6, 6] tensor of C in eV / A^3."""
        T = _v._temperature(temperature)
        if self.form not in ('volume', 'voigt'):
            raise ValueError("thermal_expansion: needs a Gruneisen made with strain='volume' or strain='voigt'")
        if elastic is None:
            raise ValueError('elastic: the elastic constants (an ElasticConstants or C [B, 6, 6] in eV / A^3) are needed')
        ph = self._ph
        B = len(ph.counts)
        c = elastic.C.detach().double().cpu() if isinstance(elastic, _el.ElasticConstants) else torch.as_tensor(elastic).detach().double().cpu()
        if tuple(c.shape) != (B, 6, 6):
            raise ValueError(f'elastic: C of shape [{B}, 6, 6] expected (got {tuple(c.shape)})')
        num, _ = self._sums(T, tol_zero)
        dev = num.device
        Q = max(len(self.bands.q), 1)
        vol = torch.tensor(np.abs(np.linalg.det(np.asarray(ph._cells, dtype=np.float64).reshape(B, 3, 3))), dtype=torch.float64).to(dev)
        if self.form == 'volume':
            kv = (c[:, 0, 0] + c[:, 1, 1] + c[:, 2, 2] + 2.0 * (c[:, 0, 1] + c[:, 0, 2] + c[:, 1, 2])) / 9.0
            return (num[:, 0] / (Q * vol * kv.to(dev))).float()
        S = torch.linalg.inv(c).to(dev)
        return (torch.einsum('bij,bj->bi', S, num) / (Q * vol)[:, None]).float()


class Gruneisen:
    """Force-constant derivatives of B crystals along K strains, ready for any number of wave vectors.

    phonons        the central Phonons (force constants, image table, masses)
    dfc            fp32 [K, n_fc]: plane k = d Phi / d eta_k, each laid out as phonons.fc
    strains        fp64 numpy [K, 3, 3] (None: from_phonons), delta: the strain step, form: 'volume' | 'voigt' | 'custom'
    split_weights  fp64 numpy [K], unit norm (default: all equal): degenerate groups are split along dfc_split = sum_k w_k dfc_k; for
                   K = 1 that is the plane itself, the same memory
    """

    def __init__(self, phonons, dfc, strains, delta, form='custom', split_weights=None):
        self.phonons, self.dfc, self.strains, self.delta, self.form = phonons, dfc.contiguous(), strains, delta, form
        self.set_split_weights(split_weights)

    def set_split_weights(self, w=None):
        K = self.dfc.shape[0]
        self.split_weights = _split_weights(w, K)
        if K == 1:
            self.dfc_split = self.dfc[0]
        else:
            wt = torch.tensor(self.split_weights, dtype=torch.float32).to(self.dfc.device)
            self.dfc_split = (wt[:, None] * self.dfc).sum(dim=0).contiguous()

    @classmethod
    def from_phonons(cls, ph0, ph_minus, ph_plus, step: float, form: str = 'volume') -> 'Gruneisen':
        """One plane from three Phonons the caller made: dfc = (ph_plus.fc - ph_minus.fc) / (2 step), formed in fp64.  For ions relaxed
        at each volume, or force constants from elsewhere (Phonons.from_force_constants).  step: the strain parameter's step (ln V
        for form='volume', which thermal_expansion then takes).  Counts and supercells must agree (ValueError).
        ph0's image table and masses serve all three.  That is legitimate: the table lists, per pair, the lattice translations of the
        nearest images in units of the lattice vectors, and another assignment of the atomic positions in the phases multiplies row i
        and column j of D by unit phases -- a diagonal unitary change of D and of every dD alike, which changes no eigenvalue and no
        e^H dD e inside a group."""
        step = _check_delta(step)
        for name, p in (('ph_minus', ph_minus), ('ph_plus', ph_plus)):
            if list(p.counts) != list(ph0.counts) or list(p.sc_counts) != list(ph0.sc_counts) or \
                    not np.array_equal(np.asarray(p.supercell), np.asarray(ph0.supercell)):
                raise ValueError(f'{name}: built for other crystals or another supercell than ph0')
        dfc = ((ph_plus.fc.double() - ph_minus.fc.double().to(ph_plus.fc.device)) / (2.0 * step)).float().to(ph0.fc.device)
        return cls(ph0, dfc[None], None, step, form)

    # ---- wave vectors ---------------------------------------------------------------------------------------------------------
    def frequencies(self, q, solver: Optional[str] = None, degeneracy_tol: Optional[float] = None, modes: bool = False) -> GruneisenBands:
        """The spectra at the wave vectors q with the mode Grueneisen parameters: the central Phonons' frequencies(q, modes=True) and
        then ONE launch of nnhip_phonon_strain_slopes, whichever solver wrote the modes (dropped again unless modes=True).  Everything
        else of the result is bitwise what Phonons.frequencies returns.  degeneracy_tol and the zero tolerance: as
        Phonons.frequencies(velocities=True) forms them, per crystal, relative to max |lambda| of the call."""
        degeneracy_tol = _ph._check_degeneracy_tol(degeneracy_tol)
        ph = self.phonons
        base = ph.frequencies(q, modes=True, solver=solver)
        dev, B, Q, K = ph.fc.device, len(ph.counts), len(base.q), self.dfc.shape[0]
        n_val = 3 * sum(ph.counts)
        evals = base.eigenvalues
        dlam, gamma = (torch.zeros(Q * n_val, K, dtype=torch.float32, device=dev) for _ in range(2))
        group = torch.zeros(Q * n_val, dtype=torch.int32, device=dev)
        defined = torch.zeros(Q * n_val, dtype=torch.uint8, device=dev)
        gstatus = torch.zeros(B, Q, dtype=torch.int32, device=dev)
        if B and Q and n_val:
            lengths = torch.tensor([Q * d for d in ph._dims], dtype=torch.int64).to(dev)
            scale = torch.segment_reduce(evals.abs(), 'max', lengths=lengths, unsafe=True).clamp_min(0.0)
            default = torch.tensor([8.0 * EPS32 * 2 * d for d in ph._dims], dtype=torch.float32, device=dev)
            zero_tol = (default * scale).contiguous()
            deg_tol = zero_tol if degeneracy_tol is None else (degeneracy_tol * scale).contiguous()
            q_dev = torch.tensor(base.q, dtype=torch.float64).to(dev)
            vec = torch.view_as_real(base.modes)
            rc = hip.lib().nnhip_phonon_strain_slopes(
                hip._ptr(self.dfc), K, self.dfc.stride(0), hip._ptr(self.dfc_split), hip._ptr(ph.fc_ptr), hip._ptr(ph.cry_ptr),
                ph._cry_host.data_ptr(), hip._ptr(ph.sc_atoms), hip._ptr(ph.img_ptr), hip._ptr(ph.img_start), hip._ptr(ph.img_off),
                hip._ptr(ph.masses), hip._ptr(ph.out_ptr), B, hip._ptr(q_dev), Q, hip._ptr(evals), hip._ptr(vec), hip._ptr(deg_tol),
                hip._ptr(zero_tol), hip._ptr(dlam), hip._ptr(gamma), hip._ptr(group), hip._ptr(defined), hip._ptr(gstatus),
                hip._stream(dev))
            if rc == 2:
                raise NotImplementedError(hip.lib().nnhip_last_error().decode())
            hip._check(rc, 'nnhip_phonon_strain_slopes')
            base.status |= gstatus
        return GruneisenBands(eigenvalues=evals, frequencies=base.frequencies, modes=base.modes if modes else None,
                              dynamical_matrix=None, sweeps=base.sweeps, status=base.status, q=base.q, _dims=ph._dims,
                              _offsets=ph._offsets, _sq_offsets=ph._sq_offsets, gruneisen=gamma, eigenvalue_strain_gradients=dlam,
                              gruneisen_defined=defined.bool(), degenerate_group=group)

    def band_structure(self, points, n_per_segment: int = 20, solver: Optional[str] = None) -> GruneisenBands:
        """frequencies() along the piecewise-linear path through `points` (phonons.band_path), with `path` and `ticks`."""
        q, ticks = _ph.band_path(points, n_per_segment)
        bands = self.frequencies(q, solver=solver)
        cells = self.phonons._cells
        bands.path = np.stack([_ph.path_length(q, c) for c in cells]) if len(cells) else np.zeros((0, len(q)))
        bands.ticks = ticks
        return bands

    def mesh(self, n1: int, n2: int, n3: int, shift: bool = False, solver: Optional[str] = None) -> GruneisenMesh:
        """The spectra and mode Grueneisen parameters on the full n1 x n2 x n3 grid of phonons.monkhorst_pack."""
        return GruneisenMesh(self.frequencies(_ph.monkhorst_pack(n1, n2, n3, shift), solver=solver), self.phonons, self.form)


# ---- from a model ----------------------------------------------------------------------------------------------------------------

def gruneisen(model, z, pos, cell, batch, supercell, strain='volume', delta: float = 0.01, masses: Optional[torch.Tensor] = None,
              asr: bool = True, solver: str = 'lds', phonons=None, split_weights=None) -> Gruneisen:
    """Force-constant derivatives of every crystal of the batch along `strain` ('volume': one plane d Phi / d ln V; 'voigt': the six Voigt
    strains, the convention of elastic.ElasticConstants; or symmetric matrices [K, 3, 3], K <= 6) as a central difference of the
    analytic force constants at the cells strained by +-delta (see the module text and strained_crystals).  z, pos, cell, batch,
    supercell, masses, asr, solver: as phonons.phonons takes them; its checks (phonons._checked_crystals: symmetric cell, supercell
    widths against the cutoff) are applied to every strained copy as well.  The acoustic sum rule is imposed on Phi(+-delta) as on the
    central force constants, so the planes obey it.  phonons: the central Phonons of this call's crystals and supercell (None computes
    one).  The strained force constants themselves are not kept."""
    delta = _check_delta(delta)
    eps = strain_matrices(strain)
    w = _split_weights(split_weights, len(eps))
    _ph._check_solver(solver)
    cells, S, counts = _ph._checked_crystals(model, z, pos, cell, batch, supercell, lambda c: _ph._check_bound(c, solver))
    if masses is not None and masses.numel() != pos.shape[0]:
        raise ValueError(f'masses: {masses.numel()} values for {pos.shape[0]} atoms')
    if phonons is not None and (list(phonons.counts) != list(counts) or not np.array_equal(np.asarray(phonons.supercell), S)):
        raise ValueError('phonons: built for other crystals or another supercell than this call')
    _, copies = strained_crystals(pos, cell, batch, strain, delta)
    checked = [[_ph._checked_crystals(model, z, p, c, batch, supercell, None) for p, c, _ in pair] for pair in copies]
    if not pos.is_cuda:
        raise RuntimeError('newtonnet_amd phonons run on an MI355X (ROCm) device only: move the model and the inputs to "cuda"')
    dev = pos.device
    ph0 = phonons if phonons is not None else _ph.phonons(model, z, pos, cell, batch, supercell, masses=masses, asr=asr, solver=solver)
    rotated = not (isinstance(strain, str) and strain == 'volume')
    planes = []
    for pair, chk in zip(copies, checked):
        phi = []
        for (p, c, Q), (cells_s, S_s, counts_s) in zip(pair, chk):
            fc, sc_counts = _ph._force_constants(model, z, p, cells_s, S_s, counts_s, asr, dev)
            phi.append(rotate_back(fc, Q, counts, sc_counts) if rotated else fc.double())
        planes.append(((phi[1] - phi[0]) / (2.0 * delta)).float())
        del phi
    return Gruneisen(ph0, torch.stack(planes), eps, delta, _form(strain), w)
