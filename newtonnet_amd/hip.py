"""ctypes binding of libnewtonnet_hip.so (C ABI: include/newtonnet_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every kernel is
in the shared library.  There is no fallback: if the library is missing or a
call fails, this module raises.  The structs, the constants and every function's
argtypes / restype are derived from the header (newtonnet_amd/abi.py); the wrappers
below add validation and tensor plumbing.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import NamedTuple, Optional

import torch

from . import abi
from .abi import HipLibraryError  # noqa: F401  (raised here and by every caller as hip.HipLibraryError)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'lib', os.environ.get('NNHIP_LIB_NAME', 'libnewtonnet_hip.so'))  # env: tooling only
BUILD_SCRIPT = os.path.join(_HERE, 'csrc', 'build.sh')

_K = abi.CONSTANTS
NNHIP_F, NNHIP_NB, NNHIP_MAX_NB, NNHIP_MAX_LAYERS = _K['NNHIP_F'], _K['NNHIP_NB'], _K['NNHIP_MAX_NB'], _K['NNHIP_MAX_LAYERS']
# activation ids of include/newtonnet_hip.h, keyed by the reference's factory names (activations.py:5-30)
ACTIVATION_IDS = {name: _K['NNHIP_ACT_' + ('SILU' if name == 'swish' else name.upper())]
                  for name in ('swish', 'silu', 'relu', 'elu', 'leaky_relu', 'tanh', 'sigmoid', 'softplus', 'gelu', 'ssp')}
N_TIMER_CLASSES = _K['NNHIP_N_TIMER_CLASSES']
TIMER_CLASSES = ('edge_all', 'linear_mfma', 'other', 'edge_msg_fwd', 'edge_force_fwd', 'edge_force_bwd',
                 'edge_msg_bwd', 'graph', 'mlp128', 'lin128', 'wgrad', 'mlp_onepass', 'mol_fwd', 'mol_bwd')

# the structs of the header (generated: abi.parse): every pointer member is a c_void_p, callers assign data_ptr() integers
(LayerParams, Model, WsLayout, StepLayout, StepDev, MlpDesc, WgradProblem, ColsumProblem, TrainWs, HvpWs) = (
    abi.STRUCTS['nnhip_' + name] for name in ('layer_params', 'model', 'ws_layout', 'step_layout', 'step_dev', 'mlp_desc',
                                              'wgrad_problem', 'colsum_problem', 'train_ws', 'hvp_ws'))

MODE_FWD, MODE_BWD, MODE_TAN, MODE_TAN2 = 0, 1, 2, 3
LOSS_MODES = {name: _K['NNHIP_LOSS_' + name.upper()] for name in ('mse', 'mae', 'huber')}   # newtonnet/train/loss.py:53-103
WG_PLAIN, WG_ACT, WG_TDACT = 0, 1, 2


_lib = None


def build(verbose: bool = False, force: bool = False) -> str:
    """Compile the HIP sources for gfx950 into newtonnet_amd/lib/libnewtonnet_hip.so (force: every source, not only the
    stale ones)."""
    r = subprocess.run(['bash', BUILD_SCRIPT] + (['--force'] if force else []), capture_output=True, text=True)
    if r.returncode != 0:
        raise HipLibraryError(f'hipcc build failed:\n{r.stdout}\n{r.stderr}')
    if verbose:
        print(r.stdout.strip())
    return LIB_PATH


def lib():
    """The loaded library.  Fails loudly when it is absent (no CPU path exists in this package)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(
            f'{LIB_PATH} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            f'or `bash {BUILD_SCRIPT}`.  newtonnet_amd has no CPU fallback.')
    L = C.CDLL(LIB_PATH)
    abi.bind(L, ('nnhip_version', 'nnhip_build_flags'))
    if L.nnhip_build_flags() & 1 and os.environ.get('NNHIP_ALLOW_TOOLING_LIB') != '1':
        raise HipLibraryError(f'{LIB_PATH} is a TOOLING build (compiled with extra flags such as an ablation switch: its results '
                              'may be wrong).  Rebuild with `bash newtonnet_amd/csrc/build.sh --force`, or set '
                              'NNHIP_ALLOW_TOOLING_LIB=1 for measurements.')
    abi.bind(L)
    _lib = L
    return L


EXPORTED_SYMBOLS = tuple(abi.FUNCTIONS)     # every entry point the header declares


def _check(rc: int, what: str):
    if rc != 0:
        raise HipLibraryError(f'{what} failed (code {rc}): {lib().nnhip_last_error().decode()}')


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _f32c(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise NotImplementedError(f'{name}: the HIP path computes in float32 (got {t.dtype})')
    return t.contiguous()


CELL_LIST_MIN_ATOMS = 2048   # below this the all-pairs kernel is at least as fast


_EDGE_FIELDS = ('col', 'rev', 'disp', 'edge_index', 'geo', 'rbf', 'drbf', 'xg', 'pid')


class Graph:
    """Neighbor list + edge embedding of one batch (device tensors).  The per-edge arrays (`col`, `rev`, `pid`, `xg`, `geo`,
    `disp`, `rbf`, `drbf`, `edge_index`) are views into three allocations; they are created on first access -- the host time
    between the edge-count read-back and the first launch behind it is on the step's critical path, and a dozen view
    constructions are ~15 us of it -- and `edge_ptr(name)` gives the raw device address without creating one."""
    __slots__ = ('n_atoms', 'n_mol', 'n_edges', 'mol_ptr', 'row_ptr', 'col', 'rev', 'disp', 'edge_index', 'geo',
                 'rbf', 'drbf', 'xg', 'pid', 'pair_ptr', '_train_eg', 'envelope', 'status', '_arrays', '_cap', '_nb', '_want_rbf',
                 '_meta')

    def __getattr__(self, name):   # (only reached when the slot is still empty)
        if name in _EDGE_FIELDS and self._bind():
            return object.__getattribute__(self, name)
        raise AttributeError(name)

    def _bind(self) -> bool:
        try:
            ints, flts, ei = object.__getattribute__(self, '_arrays')
        except AttributeError:
            return False
        cap, E, nb = self._cap, self.n_edges, self._nb
        self.xg, self.col = ints[:2 * cap].view(cap, 2)[:E], ints[2 * cap:2 * cap + E]
        self.rev, self.pid = ints[3 * cap:3 * cap + E], ints[4 * cap:4 * cap + E]
        self.geo, self.disp = flts[:4 * cap].view(cap, 4)[:E], flts[4 * cap:7 * cap].view(cap, 3)[:E]
        want_rbf = self._want_rbf
        self.rbf = flts[7 * cap:(7 + nb) * cap].view(cap, nb)[:E] if want_rbf else None     # dist_edge (tests / API)
        self.drbf = flts[(7 + nb) * cap:].view(cap, nb)[:E] if want_rbf else None
        self.edge_index = ei[:2 * E].view(2, E) if ei is not None else None   # (its rows were written at stride E)
        return True

    def edge_ptr(self, name: str):
        """Device address of a per-edge array (None when absent), without materialising the view."""
        try:
            ints, flts, ei = object.__getattribute__(self, '_arrays')
        except AttributeError:
            return _ptr(getattr(self, name))
        cap, nb = self._cap, self._nb
        if cap == 0:
            return None
        off = {'xg': (ints, 0), 'col': (ints, 8 * cap), 'rev': (ints, 12 * cap), 'pid': (ints, 16 * cap), 'geo': (flts, 0),
               'disp': (flts, 16 * cap)}
        if name in off:
            base, o = off[name]
            return C.c_void_p(base.data_ptr() + o)
        if name == 'edge_index':
            return _ptr(ei)
        if not self._want_rbf:
            return None
        return C.c_void_p(flts.data_ptr() + (28 * cap if name == 'rbf' else (28 + 4 * nb) * cap))


def prepare(model: Model, device, block: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fill a prepared block (nnhip_prepare) for `model` on the current stream and return it (a new one unless `block`)."""
    L = lib()
    n = L.nnhip_prepared_bytes(model.n_layers)
    buf = block if block is not None else torch.empty(max(n, 256), dtype=torch.uint8, device=device)
    _check(L.nnhip_prepare(C.byref(model), _ptr(buf), buf.numel(), _stream(buf.device)), 'nnhip_prepare')
    return buf


STATUS_BIG_MOLECULE = 8     # bit of the graph status word: a molecule of more than NNHIP_MOL_STAGE_MAX atoms (informational)
STATUS_PARAMS_CHANGED = 4   # bit of the graph status word: nnhip_prepare_check found a parameter that differs from its snapshot


def prepare_check(model: Model, block: torch.Tensor, status: torch.Tensor):
    """Queue the exact parameters-vs-snapshot comparison of `block` (nnhip_prepare_check); STATUS_PARAMS_CHANGED is OR-ed into
    the device int32 `status[0]` when a parameter changed since the previous check of this block."""
    _check(lib().nnhip_prepare_check(C.byref(model), _ptr(block), block.numel(), _ptr(status), STATUS_PARAMS_CHANGED,
                                     _stream(block.device)), 'nnhip_prepare_check')


def _orthorhombic_box(cell: torch.Tensor, cutoff: float, cell_host=None):
    """Box lengths (3 floats) when `cell` ([1,3,3]) is an axis-aligned periodic box of at least 3 cutoffs per side -- the
    precondition of the O(N) cell-list kernels -- else None.  The CURRENT contents of the cell decide, every call: a device
    tensor is read back (36 bytes, one round trip of ~30 us on a step that takes milliseconds at the >= 2048-atom sizes this
    path serves); callers that hold the cell on the host (the ASE calculator) pass it in and skip the round trip.  Nothing is
    cached on tensor identity: a fresh cell tensor per NPT frame reuses the allocator's block and its version counter."""
    if cell_host is not None:
        c = torch.as_tensor(cell_host, dtype=torch.float32).reshape(3, 3)
    else:
        c = cell.reshape(3, 3).cpu()
    diag = torch.diagonal(c)
    ok = bool((c - torch.diag(diag) == 0).all()) and bool((diag >= 3.0003 * cutoff).all())
    ok = ok and bool((diag <= 2.0 * CELL_LIST_MAX_COORD * cutoff).all())
    return tuple(float(v) for v in diag) if ok else None


# The cell list bins fp32 coordinates in fp32, and its bins are only 1.0001 cutoffs wide: far from the origin the rounding of the
# bin boundaries (and, across periodic images, of the pair predicate itself) eats that margin and a pair two bins apart can pass the
# predicate -- a neighbor the all-pairs list has and the cell list would lose (first seen near 2500 cutoffs).  Up to 128 cutoffs
# from the origin, in a box of at most 256 cutoffs, it cannot happen (tests/graph_ref.py); beyond that
# range -- unwrapped coordinates of a long MD run -- the all-pairs builder serves the system.
CELL_LIST_MAX_COORD = 128.0


def _cell_list_in_range(pos: torch.Tensor, cutoff: float) -> bool:
    """every |coordinate| <= CELL_LIST_MAX_COORD cutoffs (one 4-byte read-back, on the >= 2048-atom periodic path only)"""
    return bool(pos.abs().max() <= CELL_LIST_MAX_COORD * cutoff)


def build_graph(pos: torch.Tensor, cell: torch.Tensor, batch: torch.Tensor, cutoff: float,
                frequencies: torch.Tensor, want_edge_index: bool = True, want_rbf: bool = False,
                while_waiting=None, z: Optional[torch.Tensor] = None, cell_host=None, envelope: int = 9,
                before_sync=None, edge_capacity: int = 0) -> Graph:
    """RadiusGraph + ScaledNorm + envelope x Bessel (representations.py:20-43) on the GPU.
    `while_waiting`: callable run after the counting kernels are queued and before the host waits for the edge count --
    work it launches on the stream fills the GPU's idle time during that round trip (NewtonNet.forward passes
    nnhip_prepare here).  `z` (int64, optional): species, range-checked on the device in the same round trip (the
    reference raises IndexError for z outside 0..118).  `cell_host`: the cell as a host array, when the caller has it.
    `before_sync(status)`: callable that may queue kernels OR-ing further bits (>= 4) into the device status word before it is
    read back with the edge count; the word comes back as `graph.status`.
    `edge_capacity` > 0 (with `while_waiting`; all-pairs builder): the edge arrays are allocated for that many edges and
    nnhip_graph_finish_early is queued BEFORE the host waits for the count -- the kernels read it on the device; when the
    count turns out larger than the capacity they have written nothing and the ordinary path runs after the wait."""
    L = lib()
    dev = pos.device
    pos = _f32c(pos, 'pos')
    cell = _f32c(cell, 'cell')
    batch = batch.contiguous()
    if batch.dtype != torch.int64:
        batch = batch.long()
    N, B = pos.shape[0], cell.shape[0]
    g = Graph()
    g.n_atoms, g.n_mol, g.envelope = N, B, int(envelope)
    n_scan = (N + 1023) // 1024 + 1
    # one int32 block: mol_ptr [B+1] | row_ptr [N+1] | status + scan scratch [1 + n_scan] | pair_ptr [N+1] | its scan scratch
    meta = torch.empty(B + 1 + N + 1 + 1 + n_scan + N + 1 + n_scan, dtype=torch.int32, device=dev)
    g.mol_ptr, g.row_ptr, status = meta[:B + 1], meta[B + 1:B + N + 2], meta[B + N + 2:B + N + 3 + n_scan]
    o_pp = B + N + 3 + n_scan
    g.pair_ptr, pair_scan = meta[o_pp:o_pp + N + 1], meta[o_pp + N + 1:]
    st = _stream(dev)
    # One big orthorhombic periodic box -> O(N) cell-list kernels (bit-identical output to the all-pairs kernels).
    box = None
    if B == 1 and N >= CELL_LIST_MIN_ATOMS:
        lengths = _orthorhombic_box(cell, cutoff, cell_host)
        if lengths is not None and _cell_list_in_range(pos, cutoff):
            box = (C.c_float * 3)(*lengths)
    if box is not None:
        scratch = torch.empty(L.nnhip_graph_cells_scratch_bytes(N, box, float(cutoff)), dtype=torch.uint8, device=dev)
        status[:1].zero_()
        _check(L.nnhip_graph_count_cells_pairs(_ptr(pos), _ptr(cell), N, float(cutoff), box, _ptr(scratch), _ptr(g.mol_ptr),
                                               _ptr(g.row_ptr), _ptr(g.pair_ptr), st), 'nnhip_graph_count_cells_pairs')
    else:   # (the count pass also takes the per-row pair counts: the pair ids then need no pass of their own after the sync)
        _check(L.nnhip_graph_count_pairs(_ptr(pos), _ptr(cell), _ptr(batch), N, B, float(cutoff), _ptr(g.mol_ptr),
                                         _ptr(g.row_ptr), _ptr(status), _ptr(g.pair_ptr), st), 'nnhip_graph_count_pairs')
    if z is not None:
        if z.dtype != torch.int64 or not z.is_contiguous():
            z = z.long().contiguous()
        _check(L.nnhip_check_species(_ptr(z), N, _ptr(status), st), 'nnhip_check_species')
    if before_sync is not None:
        before_sync(status[:1])
    tail_dev = meta[B + N + 1:B + N + 3]
    nb = frequencies.numel()
    freq = _f32c(frequencies, 'frequencies')

    def edge_arrays(cap):
        # everything sized by the edge count in three allocations (the host time between the sync and the first launch is on the
        # step's critical path): int32 [xg 2 cap | col | rev | pid], float32 [geo 4 cap | disp 3 cap | rbf, drbf nb cap each], edge_index
        ints = torch.empty(5 * cap, dtype=torch.int32, device=dev)
        flts = torch.empty((7 + (2 * nb if want_rbf else 0)) * cap, dtype=torch.float32, device=dev)
        ei = torch.empty(2 * cap, dtype=torch.int64, device=dev) if want_edge_index else None
        return ints, flts, ei

    def bind(arrays, cap, E):   # (views of the first E edges: made on first access, Graph._bind)
        g._arrays, g._cap, g._nb, g._want_rbf = arrays, cap, nb, bool(want_rbf)

    def finish_args(arrays, cap):
        ints, flts, ei = arrays
        return (_ptr(pos), _ptr(cell), _ptr(batch), _ptr(g.mol_ptr), _ptr(g.row_ptr), _ptr(g.pair_ptr), N, B, cap, float(cutoff),
                C.c_void_p(ints.data_ptr() + 8 * cap), C.c_void_p(ints.data_ptr() + 12 * cap), C.c_void_p(ints.data_ptr() + 16 * cap),
                C.c_void_p(flts.data_ptr() + 16 * cap), _ptr(ei), _ptr(freq), nb, _ptr(flts),
                C.c_void_p(flts.data_ptr() + 28 * cap) if want_rbf else None,
                C.c_void_p(flts.data_ptr() + (28 + 4 * nb) * cap) if want_rbf else None, _ptr(ints), g.envelope, st)

    early = None
    if while_waiting is not None:
        tail_host = torch.empty(2, dtype=torch.int32, pin_memory=True)
        tail_host.copy_(tail_dev, non_blocking=True)          # queue the read-back first ...
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        # ... then work that does not need the edge count on the host: the pair scan,
        _check(L.nnhip_graph_pair_scan(_ptr(g.pair_ptr), N, _ptr(pair_scan), st), 'nnhip_graph_pair_scan')
        if edge_capacity > 0 and box is None:                  # the fill itself, into arrays of the caller's capacity,
            early = edge_arrays(int(edge_capacity))
            _check(L.nnhip_graph_finish_early(*finish_args(early, int(edge_capacity))), 'nnhip_graph_finish_early')
        while_waiting()                                        # the caller's (allocations), then wait for the copy only
        ev.synchronize()
        tail = tail_host.tolist()
    else:
        _check(L.nnhip_graph_pair_scan(_ptr(g.pair_ptr), N, _ptr(pair_scan), st), 'nnhip_graph_pair_scan')
        tail = tail_dev.tolist()  # (E, status): the one device->host sync of the path
    E, bad = int(tail[0]), int(tail[1])
    if bad & 1:
        raise ValueError('batch must be non-decreasing with values in [0, cell.shape[0]) (PyG collation order)')
    if bad & 2:
        raise IndexError('atomic numbers z must lie in [0, 118] (rows of node_embedding / scale / shift)')
    g.n_edges = E
    g.status = bad | (STATUS_BIG_MOLECULE if box is not None else 0)   # (the cell-list builder serves ONE large system)
    if early is not None and E <= int(edge_capacity):          # the early launch has done the work
        bind(early, int(edge_capacity), E)
        if E == 0:
            g.pair_ptr.zero_()
        return g
    arrays = edge_arrays(E)
    bind(arrays, E, E)
    if box is None:
        _check(L.nnhip_graph_finish(*finish_args(arrays, E)), 'nnhip_graph_finish')
        if E == 0:
            g.pair_ptr.zero_()
    else:
        _check(L.nnhip_graph_finish_cells(_ptr(pos), _ptr(cell), N, E, float(cutoff), box, _ptr(scratch), _ptr(g.row_ptr),
                                          _ptr(g.pair_ptr), _ptr(g.col), _ptr(g.rev), _ptr(g.pid), _ptr(g.disp), _ptr(g.edge_index),
                                          _ptr(freq), nb, _ptr(g.geo), _ptr(g.rbf), _ptr(g.drbf), _ptr(g.xg), g.envelope, st),
               'nnhip_graph_finish_cells')
    return g


def refresh_graph(g: Graph, pos: torch.Tensor, cell: torch.Tensor, batch: torch.Tensor, cutoff: float,
                  frequencies: torch.Tensor) -> Graph:
    """Re-evaluate the geometry of an existing (candidate) list at new positions, in place and without any host sync:
    disp, geo and the filter-table positions xg.  `g` must have been built with want_edge_index=True and a cutoff of at
    least `cutoff` (cutoff + skin for Verlet reuse); candidates outside `cutoff` get all-zero filter rows."""
    L = lib()
    if g.edge_index is None:
        raise ValueError('refresh_graph needs a graph built with want_edge_index=True')
    st = _stream(g.row_ptr.device)     # (pos may be a pinned HOST array read in place by the kernels: the MD loop's zero-copy input)
    pos, cell = _f32c(pos, 'pos'), _f32c(cell, 'cell')
    if batch.dtype != torch.int64 or not batch.is_contiguous():
        batch = batch.long().contiguous()
    E = g.n_edges
    _check(L.nnhip_edge_refresh(_ptr(pos), _ptr(cell), _ptr(batch), _ptr(g.edge_index), E, float(cutoff),
                                _ptr(_f32c(frequencies, 'frequencies')), frequencies.numel(), _ptr(g.disp), _ptr(g.geo), _ptr(g.rbf),
                                _ptr(g.drbf), _ptr(g.xg), g.envelope, st), 'nnhip_edge_refresh')
    return g


_step_layouts = {}


def step_layout(N: int, B: int, cap: int) -> StepLayout:
    key = (N, B, cap)
    lay = _step_layouts.get(key)
    if lay is None:
        lay = StepLayout()
        _check(lib().nnhip_step_layout_of(N, B, cap, C.byref(lay)), 'nnhip_step_layout_of')
        if len(_step_layouts) > 256:
            _step_layouts.clear()
        _step_layouts[key] = lay
    return lay


class DevStep:
    """Arenas of one deferred step (nnhip_forward_dev) and lazily made views of what a caller may look at.  Quacks like the
    result dict of energy_forces (`step[name]`) and like a Graph as far as NewtonNet.forward needs one (`edge_index`,
    `n_edges`, `status`).  `n_edges` is None until the caller has read the count."""
    __slots__ = ('N', 'B', 'cap', 'lay', 'i32', 'f32', 'ei', 'atom_node', 'force_node', 'workspace', 'n_edges', 'status',
                 'want_forces', 'want_virial', '_views')

    def __getitem__(self, name):
        v = self._views.get(name)
        if v is None:
            lay, N, B = self.lay, self.N, self.B
            if name == 'energy':
                v = self.f32[lay.energy:lay.energy + B]
            elif name == 'forces':
                v = self.f32[lay.forces:lay.forces + 3 * N].view(N, 3) if self.want_forces else None
            elif name == 'virial':
                v = self.f32[lay.virial:lay.virial + 9 * B].view(B, 3, 3) if (self.want_forces and self.want_virial) else None
            elif name == 'atom_energy':
                v = self.f32[lay.atom_energy:lay.atom_energy + N]
            elif name == 'atom_node':
                v = self.atom_node
            elif name == 'force_node':
                v = self.force_node
            elif name == 'workspace':
                v = self.workspace
            else:
                raise KeyError(name)
            self._views[name] = v
        return v

    @property
    def row_ptr(self):
        return self.i32[self.lay.row_ptr:self.lay.row_ptr + self.N + 1]

    @property
    def col(self):
        return self.i32[self.lay.col:self.lay.col + self.n_edges]

    @property
    def edge_index(self):
        # RadiusGraph's [2][E] array, made when a caller asks for it (most evaluation steps never do): receiver = the row of the
        # edge, sender = col (nnhip_edge_index_from_csr)
        if self.ei is None:
            E, lay = self.n_edges, self.lay
            self.ei = torch.empty(2 * E, dtype=torch.int64, device=self.i32.device)
            _check(lib().nnhip_edge_index_from_csr(_ptr(self.i32[lay.row_ptr:]), _ptr(self.i32[lay.col:]), self.N, E, _ptr(self.ei),
                                                   None, _stream(self.i32.device)), 'nnhip_edge_index_from_csr')
        E = self.n_edges
        return self.ei[:2 * E].view(2, E)


def forward_dev(model: Model, z, pos, cell, batch, cap: int, prepared: torch.Tensor, tail_host_ptr: int, seq: int,
                want_forces: bool, want_virial: bool, workspace: Optional[torch.Tensor], event_handle: int = 0,
                small_molecules: bool = False) -> DevStep:
    """The whole deferred step in one C call (nnhip_forward_dev): neighbor list into arrays of `cap` edges, the (count, status)
    words stored into the pinned slot `tail_host_ptr` by the last neighbor-list kernel, `seq` behind them; energy / forces pipeline.
    Four allocations per step (two arenas, the two node states); `edge_index` is made on demand (DevStep.edge_index)."""
    L = lib()
    dev = pos.device
    N, B = pos.shape[0], cell.shape[0]
    lay = step_layout(N, B, cap)
    st = DevStep()
    st.N, st.B, st.cap, st.lay, st.n_edges, st.status, st._views = N, B, cap, lay, None, 0, {}
    st.want_forces, st.want_virial = want_forces, want_virial
    st.i32 = torch.empty(lay.i32_count, dtype=torch.int32, device=dev)
    st.f32 = torch.empty(lay.f32_count, dtype=torch.float32, device=dev)
    st.ei = None
    st.atom_node = torch.empty(N, NNHIP_F, dtype=torch.float32, device=dev)
    st.force_node = torch.empty(N, 3, NNHIP_F, dtype=torch.float32, device=dev)
    need = L.nnhip_workspace_bytes(N, cap, B, model.n_layers)
    if workspace is None or workspace.numel() < need or workspace.device != dev:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
    st.workspace = workspace
    a = StepDev()
    a.z, a.pos, a.cell, a.batch = z.data_ptr(), pos.data_ptr(), cell.data_ptr(), batch.data_ptr()
    a.n_atoms, a.n_mol, a.capacity, a.want_forces, a.want_virial = N, B, cap, int(want_forces), int(want_virial)
    a.i32, a.f32, a.edge_index = st.i32.data_ptr(), st.f32.data_ptr(), None
    a.atom_node, a.force_node = st.atom_node.data_ptr(), st.force_node.data_ptr()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel()
    a.prepared, a.prepared_bytes = prepared.data_ptr(), prepared.numel()
    a.tail_host, a.event, a.seq, a.flags = tail_host_ptr, (event_handle or None), seq, (1 if small_molecules else 0)
    _check(L.nnhip_forward_dev(C.byref(model), C.byref(a), _stream(dev)), 'nnhip_forward_dev')
    return st


def spatial_order(pos: torch.Tensor, z: torch.Tensor, cutoff: float):
    """(perm, inv, z_perm, pos_perm): the atoms of ONE big system in Morton order of cells (nnhip_spatial_order; int32 perm / inv on
    pos.device, no host round trip, deterministic: by cell, then by input index)."""
    L = lib()
    pos = _f32c(pos, 'pos')
    N, dev = pos.shape[0], pos.device
    perm = torch.empty(N, dtype=torch.int32, device=dev)
    inv = torch.empty(N, dtype=torch.int32, device=dev)
    z_out, pos_out = torch.empty_like(z), torch.empty_like(pos)
    scratch = torch.empty(L.nnhip_spatial_order_scratch_bytes(N), dtype=torch.uint8, device=dev)
    _check(L.nnhip_spatial_order(_ptr(pos), _ptr(z), N, float(cutoff), _ptr(perm), _ptr(inv), _ptr(z_out), _ptr(pos_out),
                                 _ptr(scratch), _stream(dev)), 'nnhip_spatial_order')
    return perm, inv, z_out, pos_out


def permute_rows(x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """out[k] = x[idx[k]] over dim 0 (idx int32): the per-atom results of a permuted step in the caller's order."""
    L = lib()
    x = _f32c(x, 'x')
    width = 1
    for d in x.shape[1:]:
        width *= int(d)
    out = torch.empty_like(x)
    _check(L.nnhip_permute_rows(_ptr(x), _ptr(idx), x.shape[0], width, _ptr(out), _stream(x.device)), 'nnhip_permute_rows')
    return out


def edge_index_unpermute(row_ptr, col, perm, inv, n_atoms: int, n_edges: int) -> torch.Tensor:
    """The [2][E] int64 neighbor list of a permuted step in the reference's order for the caller's atom order."""
    L = lib()
    dev = perm.device
    ei = torch.empty(2, n_edges, dtype=torch.int64, device=dev)
    scratch = torch.empty(n_atoms + 1 + n_atoms // 1024 + 2, dtype=torch.int32, device=dev)
    _check(L.nnhip_edge_index_unpermute(_ptr(row_ptr), _ptr(col), _ptr(perm), _ptr(inv), n_atoms, n_edges, _ptr(ei), _ptr(scratch),
                                        _stream(dev)), 'nnhip_edge_index_unpermute')
    return ei


def bf16_mlp_launches() -> int:
    """Edge-MLP launches that took the bf16 compute mode (training under torch.autocast(bfloat16)) since the library was loaded."""
    return int(lib().nnhip_bf16_mlp_launches())


def mlp_forms() -> dict:
    """Which forms the fused edge-MLP launches of a large batch take (nnhip_mlp_forms): what bench.py's byte model asks."""
    v = lib().nnhip_mlp_forms()
    return {'split': bool(v & 1), 'regw_bwd': bool(v & 2), 'regw_fwd': bool(v & 4), 'regw_single_bwd': bool(v & 8),
            'regw_single_fwd': bool(v & 16)}


def config() -> dict:
    """Every form choice the library makes in this process (nnhip_config), as a dict."""
    import json
    L = lib()
    buf = C.create_string_buffer(4096)
    _check(L.nnhip_config(buf, 4096), 'nnhip_config')
    return json.loads(buf.value.decode())


def workspace_layout(N: int, E: int, B: int, n_layers: int) -> WsLayout:
    out = WsLayout()
    _check(lib().nnhip_workspace_layout(N, E, B, n_layers, C.byref(out)), 'nnhip_workspace_layout')
    return out


def alloc_outputs(N: int, B: int, dev, want_forces: bool = True, want_virial: bool = False, want_nodes: bool = True) -> dict:
    """The output tensors of one energy_forces call (they depend on N and B only: NewtonNet.forward allocates them while the
    host waits for the edge count)."""
    out = dict()
    out['energy'] = torch.empty(B, dtype=torch.float32, device=dev)
    out['forces'] = torch.empty(N, 3, dtype=torch.float32, device=dev) if want_forces else None
    out['virial'] = torch.empty(B, 3, 3, dtype=torch.float32, device=dev) if (want_virial and want_forces) else None
    out['atom_energy'] = torch.empty(N, dtype=torch.float32, device=dev)
    out['atom_node'] = torch.empty(N, NNHIP_F, dtype=torch.float32, device=dev) if want_nodes else None
    out['force_node'] = torch.empty(N, 3, NNHIP_F, dtype=torch.float32, device=dev) if want_nodes else None
    return out


def energy_forces(model: Model, z: torch.Tensor, pos: torch.Tensor, cell: torch.Tensor, g: Graph, want_forces: bool = True,
                  want_virial: bool = False, want_nodes: bool = True, workspace: Optional[torch.Tensor] = None,
                  out: Optional[dict] = None, prepared: Optional[torch.Tensor] = None):
    """Run the whole hot path.  Returns dict(energy, forces, virial, atom_energy, atom_node, force_node, workspace).
    `out` = the dict of a previous call with the same sizes: its tensors are reused (static addresses for graph capture)."""
    L = lib()
    dev = z.device
    N, E, B = g.n_atoms, g.n_edges, g.n_mol
    need = L.nnhip_workspace_bytes(N, E, B, model.n_layers)
    if workspace is None or workspace.numel() < need or workspace.device != dev:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
    if out is None:
        out = alloc_outputs(N, B, dev, want_forces, want_virial, want_nodes)
    out['workspace'] = workspace
    pos, cell = _f32c(pos, 'pos'), _f32c(cell, 'cell')
    pair_ptr = getattr(g, 'pair_ptr', None)
    if pair_ptr is not None and E > 0:
        # the same step through the entry point that also takes the per-row pair counts: the row kernels then split a row into the
        # pairs it owns and the others with two scalar loads instead of a ballot over its cols
        _check(L.nnhip_energy_forces_pp(C.byref(model), _ptr(z), _ptr(pos), _ptr(cell), _ptr(g.mol_ptr), _ptr(g.row_ptr),
                                        g.edge_ptr('col'), g.edge_ptr('rev'), g.edge_ptr('pid'), g.edge_ptr('geo'), g.edge_ptr('xg'),
                                        g.edge_ptr('disp'), N, E, B, _ptr(workspace), workspace.numel(), _ptr(out['energy']),
                                        _ptr(out['forces']), _ptr(out['virial']), _ptr(out['atom_energy']), _ptr(out['atom_node']),
                                        _ptr(out['force_node']), _ptr(prepared), _ptr(pair_ptr),
                                        0 if (g.status & STATUS_BIG_MOLECULE) else 1, _stream(dev)),
               'nnhip_energy_forces_pp')
        return out
    _check(L.nnhip_energy_forces(C.byref(model), _ptr(z), _ptr(pos), _ptr(cell), _ptr(g.mol_ptr), _ptr(g.row_ptr), g.edge_ptr('col'),
                                 g.edge_ptr('rev'), g.edge_ptr('pid'), g.edge_ptr('geo'), g.edge_ptr('xg'), g.edge_ptr('disp'), N, E, B,
                                 _ptr(workspace), workspace.numel(), _ptr(out['energy']), _ptr(out['forces']),
                                 _ptr(out['virial']), _ptr(out['atom_energy']), _ptr(out['atom_node']),
                                 _ptr(out['force_node']), _ptr(prepared), _stream(dev)), 'nnhip_energy_forces')
    return out


PRO_NONE, PRO_SILU = 0, 1
EPI_STORE, EPI_BIAS, EPI_DSILU, EPI_ACC = 0, 1, 2, 3


def linear128(A: torch.Tensor, W: torch.Tensor, out: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
              H: Optional[torch.Tensor] = None, prologue: int = PRO_NONE, epilogue: int = EPI_STORE) -> torch.Tensor:
    """C = epilogue(prologue(A) @ W.T) for [M,128] x [128,128] on the fp32 matrix cores (csrc/lin128.hip).
    A / out / H may be row-strided views (last dim contiguous)."""
    assert A.dim() == 2 and A.shape[1] == NNHIP_F and A.stride(1) == 1 and A.dtype == torch.float32
    assert W.shape == (NNHIP_F, NNHIP_F) and W.is_contiguous() and W.dtype == torch.float32
    M = A.shape[0]
    if out is None:
        out = torch.empty(M, NNHIP_F, dtype=torch.float32, device=A.device)
    assert out.shape == A.shape and out.stride(1) == 1
    ldh = H.stride(0) if H is not None else 0
    _check(lib().nnhip_linear128(_ptr(A), A.stride(0) if M > 1 else NNHIP_F, _ptr(W), _ptr(out),
                                 out.stride(0) if M > 1 else NNHIP_F, _ptr(bias), _ptr(H), ldh, M, prologue, epilogue,
                                 _stream(A.device)), 'nnhip_linear128')
    return out


def mlp128(X: torch.Tensor, W1: torch.Tensor, W2: torch.Tensor, H: torch.Tensor, Y: torch.Tensor, mode: int = 0,
           accumulate: bool = False) -> torch.Tensor:
    """Fused Linear->SiLU->Linear (mode 0: writes H, Y) or its adjoint (mode 1: reads H); csrc/mlp128.hip."""
    M = X.shape[0]
    _check(lib().nnhip_mlp128(_ptr(X), X.stride(0), _ptr(W1), _ptr(W2), _ptr(H), H.stride(0), _ptr(Y), Y.stride(0), M,
                              mode, 1 if accumulate else 0, _stream(X.device)), 'nnhip_mlp128')
    return Y


def direct_force(atom_node: torch.Tensor, force_node: torch.Tensor, z: torch.Tensor, head, scale,
                 activation: int = 0) -> torch.Tensor:
    """direct_force head (output.py:115-132): head = nn.Sequential(Linear, act, Linear, act, Linear); scale [119,1] or None;
    activation = ACTIVATION_IDS[name]."""
    N = atom_node.shape[0]
    out = torch.empty(N, 3, dtype=torch.float32, device=atom_node.device)
    scratch = torch.empty(3 * max(N, 1) * NNHIP_F, dtype=torch.float32, device=atom_node.device)
    _check(lib().nnhip_direct_force(_ptr(atom_node), _ptr(force_node), _ptr(z), _ptr(head[0].weight), _ptr(head[0].bias),
                                    _ptr(head[2].weight), _ptr(head[2].bias), _ptr(head[4].weight), _ptr(head[4].bias),
                                    _ptr(scale), int(activation), N, _ptr(scratch), _ptr(out), _stream(atom_node.device)),
           'nnhip_direct_force')
    return out


def segment_sum(x: torch.Tensor, row_ptr: torch.Tensor, n_rows: int) -> torch.Tensor:
    """out[i] = sum of x[row_ptr[i]:row_ptr[i+1]] over dim 0 (deterministic CSR scatter-sum)."""
    x = _f32c(x, 'x')
    width = x[0].numel() if x.shape[0] else int(torch.tensor(x.shape[1:]).prod())
    out = torch.empty((n_rows,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    _check(lib().nnhip_segment_sum(_ptr(x), _ptr(row_ptr), n_rows, width, _ptr(out), _stream(x.device)),
           'nnhip_segment_sum')
    return out


def _written(dev, optional=(), **tensors):
    """tensors a kernel writes in place, name=(tensor, numel) or (tensor, numel, dtype), float32 unless stated: contiguous, of
    exactly that dtype, on `dev` (a copy would take the result away); None only under the names in `optional`"""
    for name, (t, numel, *dtype) in tensors.items():
        if t is None and name in optional:
            continue
        dtype = dtype[0] if dtype else torch.float32
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f'{name}: a contiguous {str(dtype)[6:]} tensor expected (it is written in place)')
        if t.numel() != numel or t.device != dev:
            raise ValueError(f'{name}: {numel} values on {dev} expected (got {t.numel()} on {t.device})')


def _read(dev, **tensors):
    """tensors a kernel reads: float32 (made contiguous) with the stated number of values on `dev`; None stays None"""
    out = []
    for name, (t, numel) in tensors.items():
        if t is not None:
            t = _f32c(t, name)
            if t.numel() != numel or t.device != dev:
                raise ValueError(f'{name}: {numel} values on {dev} expected (got {t.numel()} on {t.device})')
        out.append(t)
    return out


def _offsets(name, t, dev=None, host=False) -> int:
    """an int32 offset table [n+1]: contiguous, at least one value, on `dev` when one is given; `host`, unless False: its copy on
    the CPU, of the same length.  Returns n."""
    for label, x in ((name, t),) if host is False else ((name, t), (name + '_host', host)):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.int32 or not x.is_contiguous() or x.numel() < 1:
            raise ValueError(f'{label}: a contiguous int32 tensor [n+1] expected')
    if dev is not None and t.device != dev:
        raise ValueError(f'{name}: on {dev} expected (it is on {t.device})')
    if host is not False and (host.device.type != 'cpu' or host.numel() != t.numel()):
        raise ValueError(f'{name}_host: the host copy of {name} expected')
    return t.numel() - 1


MD_FINISH, MD_BEGIN = _K['NNHIP_MD_FINISH'], _K['NNHIP_MD_BEGIN']      # flags of nnhip_md_step


def md_step(pos_in: Optional[torch.Tensor], vel: torch.Tensor, force: torch.Tensor, hk: torch.Tensor, dth: float, c1: float,
            flags: int, pos_out: Optional[torch.Tensor] = None, mass: Optional[torch.Tensor] = None,
            sigma: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None, ke_out: Optional[torch.Tensor] = None):
    """One launch of the integrator (nnhip_md_step, csrc/md.hip) on the current stream: MD_FINISH = the second half kick with
    `force` (and the per-atom kinetic energies into `ke_out`), MD_BEGIN = half kick, half drift, the exact Ornstein-Uhlenbeck
    step v = c1 v + sigma noise (only with `noise`), half drift.  `vel` is updated in place and `pos_out` written: both must be
    contiguous float32 (a copy would take the result away); `pos_out` may not overlap `pos_in`."""
    N, dev = vel.shape[0], vel.device
    _written(dev, optional=('pos_out', 'ke_out'), vel=(vel, 3 * N), pos_out=(pos_out, 3 * N), ke_out=(ke_out, N))
    pos_in, force, hk, mass, sigma, noise = _read(dev, pos_in=(pos_in, 3 * N), force=(force, 3 * N), hk=(hk, N), mass=(mass, N),
                                                  sigma=(sigma, N), noise=(noise, 3 * N))
    _check(lib().nnhip_md_step(_ptr(pos_in), _ptr(vel), _ptr(force), _ptr(hk), _ptr(mass), _ptr(sigma), _ptr(noise), float(dth),
                               float(c1), int(flags), N, _ptr(pos_out), _ptr(ke_out), _stream(dev)), 'nnhip_md_step')


def md_kinetic(ke: torch.Tensor, mol_ptr: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[b] = sum of ke[mol_ptr[b]:mol_ptr[b+1]] (mol_ptr int32 [B+1]): the deterministic per-molecule sum of nnhip_md_kinetic."""
    ke = _f32c(ke, 'ke')
    if mol_ptr.dtype != torch.int32 or not mol_ptr.is_contiguous() or mol_ptr.numel() < 1:
        raise ValueError('mol_ptr: contiguous int32 [B+1] expected')
    B = mol_ptr.numel() - 1
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=ke.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != B:
        raise ValueError(f'out: contiguous float32 [{B}] expected')
    if ke.numel() == 0:
        return out.zero_()
    _check(lib().nnhip_md_kinetic(_ptr(ke), _ptr(mol_ptr), B, _ptr(out), _stream(ke.device)), 'nnhip_md_kinetic')
    return out


def npt_barostat(vel: torch.Tensor, mass: torch.Tensor, mol_ptr: torch.Tensor, cell_in: torch.Tensor, virial: torch.Tensor,
                 a: torch.Tensor, p0: torch.Tensor, cell_out: torch.Tensor, mu: torch.Tensor, inv_mu: torch.Tensor,
                 ke: torch.Tensor, pressure: torch.Tensor, volume: torch.Tensor, deps: torch.Tensor,
                 force: Optional[torch.Tensor] = None, hk: Optional[torch.Tensor] = None, s2: Optional[torch.Tensor] = None,
                 noise: Optional[torch.Tensor] = None):
    """One launch of the barostat of constant-pressure dynamics (nnhip_npt_barostat, csrc/npt.hip; the chain is written out in
    include/newtonnet_hip.h) on the current stream: per system the kinetic energy of the full-step velocities (`vel` with the
    pending half kick hk x force, or `vel` itself without `force`), V = det(cell_in), P = (2 K + tr virial) / (3 V), the step
    deps = -a (p0 - P) + sqrt(s2 / V) noise of ln V and mu = exp(deps / 3).  Writes cell_out = mu cell_in [B,3,3], mu, inv_mu and
    the records ke, pressure, volume, deps [B]: all contiguous float32; `cell_out` may not overlap `cell_in`.  mol_ptr int32 [B+1]."""
    N, dev = vel.shape[0], vel.device
    B = _offsets('mol_ptr', mol_ptr, dev)
    _written(dev, cell_out=(cell_out, 9 * B), mu=(mu, B), inv_mu=(inv_mu, B), ke=(ke, B), pressure=(pressure, B),
             volume=(volume, B), deps=(deps, B))
    vel, force, hk, mass, cell_in, virial, a, p0, s2, noise = _read(
        dev, vel=(vel, 3 * N), force=(force, 3 * N), hk=(hk, N), mass=(mass, N), cell_in=(cell_in, 9 * B), virial=(virial, 9 * B),
        a=(a, B), p0=(p0, B), s2=(s2, B), noise=(noise, B))
    _check(lib().nnhip_npt_barostat(_ptr(vel), _ptr(force), _ptr(hk), _ptr(mass), _ptr(mol_ptr), B, N, _ptr(cell_in), _ptr(virial),
                                    _ptr(a), _ptr(p0), _ptr(s2), _ptr(noise), _ptr(cell_out), _ptr(mu), _ptr(inv_mu), _ptr(ke),
                                    _ptr(pressure), _ptr(volume), _ptr(deps), _stream(dev)), 'nnhip_npt_barostat')


def npt_step(pos_in: Optional[torch.Tensor], vel: torch.Tensor, force: torch.Tensor, hk: torch.Tensor, dth: float, c1: float,
             flags: int, mu: Optional[torch.Tensor] = None, inv_mu: Optional[torch.Tensor] = None,
             mol_of_atom: Optional[torch.Tensor] = None, pos_out: Optional[torch.Tensor] = None,
             mass: Optional[torch.Tensor] = None, sigma: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
             ke_out: Optional[torch.Tensor] = None):
    """One launch of the constant-pressure integrator (nnhip_npt_step, csrc/md.hip) on the current stream: md_step's flags and
    chain with the rescale  x = mu_b x, v = inv_mu_b v  of the atom's system b = mol_of_atom[i] (int32 [N]) between the MD_BEGIN kick
    and the first half drift.  mu, inv_mu: float32 [B] as nnhip_npt_barostat wrote them.  `vel` is updated in place and `pos_out`
    written: both contiguous float32; `pos_out` may not overlap `pos_in`."""
    N, dev = vel.shape[0], vel.device
    _written(dev, optional=('pos_out', 'ke_out'), vel=(vel, 3 * N), pos_out=(pos_out, 3 * N), ke_out=(ke_out, N))
    n_mol = 0
    if mu is not None or inv_mu is not None:
        if mu is None or inv_mu is None or mu.numel() != inv_mu.numel():
            raise ValueError('mu and inv_mu: two float32 tensors [B] expected')
        n_mol = mu.numel()
    if mol_of_atom is not None and (mol_of_atom.dtype != torch.int32 or not mol_of_atom.is_contiguous() or mol_of_atom.numel() != N
                                    or mol_of_atom.device != dev):
        raise ValueError(f'mol_of_atom: contiguous int32 [{N}] on {dev} expected')
    pos_in, force, hk, mass, sigma, noise, mu, inv_mu = _read(
        dev, pos_in=(pos_in, 3 * N), force=(force, 3 * N), hk=(hk, N), mass=(mass, N), sigma=(sigma, N), noise=(noise, 3 * N),
        mu=(mu, n_mol), inv_mu=(inv_mu, n_mol))
    _check(lib().nnhip_npt_step(_ptr(pos_in), _ptr(vel), _ptr(force), _ptr(hk), _ptr(mass), _ptr(sigma), _ptr(noise), _ptr(mu),
                                _ptr(inv_mu), _ptr(mol_of_atom), n_mol, float(dth), float(c1), int(flags), N, _ptr(pos_out),
                                _ptr(ke_out), _stream(dev)), 'nnhip_npt_step')


MDC_PROJECT, MDC_MAX_ATOMS = _K['NNHIP_MDC_PROJECT'], _K['NNHIP_MDC_MAX_ATOMS']      # of nnhip_md_step_constrained


class ConstraintTables(NamedTuple):
    """The constraint tables of nnhip_md_step_constrained (the layout is in include/newtonnet_hip.h): int32 offset tables on the
    device with their host copies, con_pair int32 [C,2] (atoms counted within their molecule) and con_d2 fp32 [C] on the device."""
    mol_ptr: torch.Tensor
    mol_ptr_host: torch.Tensor
    mol_col_ptr: torch.Tensor
    mol_col_ptr_host: torch.Tensor
    col_ptr: torch.Tensor
    col_ptr_host: torch.Tensor
    con_pair: torch.Tensor
    con_d2: torch.Tensor


def md_constrained_max_atoms() -> int:
    """the largest molecule with constraints nnhip_md_step_constrained takes"""
    return int(lib().nnhip_md_constrained_max_atoms())


def md_step_constrained(pos_in: torch.Tensor, vel: torch.Tensor, force: Optional[torch.Tensor], hk: Optional[torch.Tensor],
                        inv_mass: torch.Tensor, dth: float, inv_dth: float, c1: float, flags: int, tables: ConstraintTables,
                        tol: float, max_iter: int, n_failed: torch.Tensor, n_sweeps: torch.Tensor,
                        pos_out: Optional[torch.Tensor] = None, mass: Optional[torch.Tensor] = None,
                        sigma: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                        ke_out: Optional[torch.Tensor] = None):
    """One launch of the constrained integrator (nnhip_md_step_constrained, csrc/rattle.hip; the contract is in
    include/newtonnet_hip.h) on the current stream: md_step's flags MD_FINISH and MD_BEGIN with SHAKE / RATTLE on the constraints
    of `tables`, or MDC_PROJECT alone (the constraints imposed on pos_in and vel).  pos_in is always read.  `vel` is updated in
    place, `pos_out`, `ke_out` are written and `n_failed`, `n_sweeps` (int32 [B]) updated: all of these must be contiguous tensors
    of exactly that type (a copy would take the result away); `pos_out` may not overlap `pos_in`."""
    N, dev = vel.shape[0], vel.device
    B = _offsets('mol_ptr', tables.mol_ptr, dev, tables.mol_ptr_host)
    if _offsets('mol_col_ptr', tables.mol_col_ptr, dev, tables.mol_col_ptr_host) != B:
        raise ValueError(f'mol_col_ptr: int32 [{B + 1}] expected')
    K = _offsets('col_ptr', tables.col_ptr, dev, tables.col_ptr_host)
    C_ = int(tables.col_ptr_host[K])
    pair, d2 = tables.con_pair, tables.con_d2
    if (pair.dtype != torch.int32 or not pair.is_contiguous() or pair.device != dev or d2.dtype != torch.float32
            or not d2.is_contiguous() or d2.device != dev or pair.numel() < 2 * C_ or d2.numel() < C_):
        raise ValueError(f'con_pair: contiguous int32 [{C_},2] and con_d2: contiguous float32 [{C_}] on {dev} expected')
    _written(dev, optional=('pos_out', 'ke_out'), vel=(vel, 3 * N), pos_out=(pos_out, 3 * N), ke_out=(ke_out, N),
             n_failed=(n_failed, B, torch.int32), n_sweeps=(n_sweeps, B, torch.int32))
    pos_in, force, hk, mass, inv_mass, sigma, noise = _read(
        dev, pos_in=(pos_in, 3 * N), force=(force, 3 * N), hk=(hk, N), mass=(mass, N), inv_mass=(inv_mass, N), sigma=(sigma, N),
        noise=(noise, 3 * N))
    _check(lib().nnhip_md_step_constrained(
        _ptr(pos_in), _ptr(vel), _ptr(force), _ptr(hk), _ptr(mass), _ptr(inv_mass), _ptr(sigma), _ptr(noise), float(dth),
        float(inv_dth), float(c1), int(flags), N, _ptr(tables.mol_ptr), _ptr(tables.mol_ptr_host), B, _ptr(pair), _ptr(d2),
        _ptr(tables.mol_col_ptr), _ptr(tables.mol_col_ptr_host), _ptr(tables.col_ptr), _ptr(tables.col_ptr_host), K, float(tol),
        int(max_iter), _ptr(pos_out), _ptr(ke_out), _ptr(n_failed), _ptr(n_sweeps), _stream(dev)), 'nnhip_md_step_constrained')


LBFGS_CHECK_ONLY = _K['NNHIP_LBFGS_CHECK_ONLY']             # flag of nnhip_lbfgs_step
LBFGS_MAX_MEMORY = _K['NNHIP_LBFGS_MAX_MEMORY']
LBFGS_CURVATURE_MIN = 1e-4       # a pair enters the history iff y.s > 0 and cos(y, s) > this (include/newtonnet_hip.h)
LBFGS_WG_THREADS = _K['NNHIP_LBFGS_WG_THREADS']             # threads of the workgroup-per-system form (nnhip_lbfgs_step_wg)


def _wg_min_atoms(wg_min_atoms):
    if (isinstance(wg_min_atoms, bool) or not hasattr(wg_min_atoms, '__index__') or
            not -2 ** 31 <= int(wg_min_atoms) < 2 ** 31):
        raise ValueError(f'wg_min_atoms: None or an int32 expected (got {wg_min_atoms!r})')
    return int(wg_min_atoms)


def _n_rows3(pos_out) -> int:
    """N of the pos_out [N,3] of an optimiser step, refused when it is not of that form"""
    if pos_out.dim() != 2 or pos_out.shape[1] != 3:
        raise ValueError(f'pos_out: [N,3] expected (got {tuple(pos_out.shape)})')
    return pos_out.shape[0]


def _free_mask(free, N: int, dev):
    """the `free` argument of an optimiser step as the kernel reads it: None, or N contiguous bytes on dev"""
    if free is None:
        return None
    if free.dtype not in (torch.bool, torch.uint8) or free.numel() != N or free.device != dev:
        raise ValueError(f'free: a bool or uint8 tensor of {N} values on {dev} expected')
    return free.contiguous()


def lbfgs_step(pos_in: torch.Tensor, force: torch.Tensor, free: Optional[torch.Tensor], mol_ptr: torch.Tensor, memory: int,
               tol2: float, alpha: float, maxstep: float, flags: int, converged: torch.Tensor, n_steps: torch.Tensor,
               n_pairs: torch.Tensor, head: torch.Tensor, S: torch.Tensor, Y: torch.Tensor, rho: torch.Tensor,
               f_prev: torch.Tensor, work: Optional[torch.Tensor], pos_out: torch.Tensor, fmax_out: torch.Tensor,
               wg_min_atoms: Optional[int] = None):
    """One launch of the L-BFGS step (nnhip_lbfgs_step, csrc/relax.hip; the contract is in include/newtonnet_hip.h) on the
    current stream, for the B molecules mol_ptr (int32 [B+1]) delimits.  pos_in, force [N,3] are read; free: bool / uint8 [N]
    (False = fixed atom) or None; the state (converged, n_steps, n_pairs, head int32 [B]; S, Y fp32 [memory,N,3]; rho fp32
    [B,memory]; f_prev fp32 [N,3]) is updated in place, pos_out [N,3] and fmax_out [B] are written: all of these must be contiguous
    tensors of exactly that type (a copy would take the result away).  work: fp32 [N,3] scratch, needed when N > 64.  pos_out may
    not overlap pos_in.  wg_min_atoms: None = nnhip_lbfgs_step (one wave64 per molecule); an int = nnhip_lbfgs_step_wg, which
    gives the molecules of at least that many atoms one workgroup of LBFGS_WG_THREADS threads each (<= 0: every molecule)."""
    if wg_min_atoms is not None:
        wg_min_atoms = _wg_min_atoms(wg_min_atoms)
    B, dev, m, i32 = _offsets('mol_ptr', mol_ptr), mol_ptr.device, int(memory), torch.int32
    N, rows = _n_rows3(pos_out), max(m, 0)
    _written(dev, optional=('work',), converged=(converged, B, i32), n_steps=(n_steps, B, i32), n_pairs=(n_pairs, B, i32),
             head=(head, B, i32), S=(S, rows * N * 3), Y=(Y, rows * N * 3), rho=(rho, B * rows), f_prev=(f_prev, 3 * N),
             work=(work, 3 * N), pos_out=(pos_out, 3 * N), fmax_out=(fmax_out, B))
    free = _free_mask(free, N, dev)
    pos_in, force = _read(dev, pos_in=(pos_in, 3 * N), force=(force, 3 * N))
    L = lib()
    head_args = (_ptr(pos_in), _ptr(force), _ptr(free), _ptr(mol_ptr), B, N, m, float(tol2), float(alpha), float(maxstep))
    tail_args = (int(flags), _ptr(converged), _ptr(n_steps), _ptr(n_pairs), _ptr(head), _ptr(S), _ptr(Y), _ptr(rho), _ptr(f_prev),
                 _ptr(work), _ptr(pos_out), _ptr(fmax_out), _stream(dev))
    if wg_min_atoms is None:
        _check(L.nnhip_lbfgs_step(*head_args, *tail_args), 'nnhip_lbfgs_step')
    else:
        _check(L.nnhip_lbfgs_step_wg(*head_args, wg_min_atoms, *tail_args), 'nnhip_lbfgs_step_wg')


# flags of nnhip_cell_lbfgs_step
CELL_LBFGS_CHECK_ONLY, CELL_LBFGS_HYDROSTATIC, CELL_LBFGS_CONSTANT_VOLUME = (
    _K['NNHIP_CELL_LBFGS_' + name] for name in ('CHECK_ONLY', 'HYDROSTATIC', 'CONSTANT_VOLUME'))
CELL_LBFGS_MASK_ALL = 63         # strain_mask with all six Voigt components (xx, yy, zz, yz, xz, xy) free


def cell_lbfgs_step(x_in: torch.Tensor, pos_in: torch.Tensor, force: torch.Tensor, virial: torch.Tensor, cell_in: torch.Tensor,
                    h0: torch.Tensor, free: Optional[torch.Tensor], mol_ptr: torch.Tensor, pressure: torch.Tensor,
                    cell_factor: torch.Tensor, memory: int, tol2: float, alpha: float, maxstep: float, strain_mask: int, flags: int,
                    converged: torch.Tensor, n_steps: torch.Tensor, n_pairs: torch.Tensor, head: torch.Tensor, S: torch.Tensor,
                    Y: torch.Tensor, rho: torch.Tensor, g_prev: torch.Tensor, work: Optional[torch.Tensor], G: torch.Tensor,
                    x_out: torch.Tensor, pos_out: torch.Tensor, cell_out: torch.Tensor, fmax_out: torch.Tensor,
                    wg_min_atoms: Optional[int] = None):
    """One launch of the variable-cell L-BFGS step (nnhip_cell_lbfgs_step, csrc/cellrelax.hip; the contract is in
    include/newtonnet_hip.h) on the current stream, for the B periodic systems mol_ptr (int32 [B+1]) delimits.  With R = N + 3 B
    generalised rows (system b: its atom rows, then the three rows of cell_factor x F): x_in [R,3], pos_in, force [N,3], virial,
    cell_in, h0 [B,3,3], pressure (eV / Angstrom^3) and cell_factor [B] are read; free: bool / uint8 [N] (False = fixed atom) or
    None; strain_mask: bit k frees the Voigt component k; the state (converged, n_steps, n_pairs, head int32 [B]; S, Y fp32
    [memory,R,3]; rho fp32 [B,memory]; g_prev fp32 [R,3]) is updated in place, G and x_out [R,3], pos_out [N,3], cell_out [B,3,3]
    and fmax_out [B] are written: all of these must be contiguous tensors of exactly that type (a copy would take the result
    away).  work: fp32 [R,3] scratch, needed when R > 64.  x_out, pos_out, cell_out may not overlap x_in, pos_in, cell_in.
    wg_min_atoms: None = nnhip_cell_lbfgs_step (one wave64 per system); an int = nnhip_cell_lbfgs_step_wg, which gives the systems
    of at least that many atoms one workgroup of LBFGS_WG_THREADS threads each (<= 0: every system)."""
    if wg_min_atoms is not None:
        wg_min_atoms = _wg_min_atoms(wg_min_atoms)
    B, dev, m, i32 = _offsets('mol_ptr', mol_ptr), mol_ptr.device, int(memory), torch.int32
    N, slots = _n_rows3(pos_out), max(m, 0)
    R = N + 3 * B
    _written(dev, optional=('work',), converged=(converged, B, i32), n_steps=(n_steps, B, i32), n_pairs=(n_pairs, B, i32),
             head=(head, B, i32), S=(S, slots * R * 3), Y=(Y, slots * R * 3), rho=(rho, B * slots), g_prev=(g_prev, 3 * R),
             work=(work, 3 * R), G=(G, 3 * R), x_out=(x_out, 3 * R), pos_out=(pos_out, 3 * N), cell_out=(cell_out, 9 * B),
             fmax_out=(fmax_out, B))
    free = _free_mask(free, N, dev)
    x_in, pos_in, force, virial, cell_in, h0, pressure, cell_factor = _read(
        dev, x_in=(x_in, 3 * R), pos_in=(pos_in, 3 * N), force=(force, 3 * N), virial=(virial, 9 * B), cell_in=(cell_in, 9 * B),
        h0=(h0, 9 * B), pressure=(pressure, B), cell_factor=(cell_factor, B))
    L = lib()
    head_args = (_ptr(x_in), _ptr(pos_in), _ptr(force), _ptr(virial), _ptr(cell_in), _ptr(h0), _ptr(free), _ptr(mol_ptr),
                 _ptr(pressure), _ptr(cell_factor), B, N, m, float(tol2), float(alpha), float(maxstep), int(strain_mask))
    tail_args = (int(flags), _ptr(converged), _ptr(n_steps), _ptr(n_pairs), _ptr(head), _ptr(S), _ptr(Y), _ptr(rho), _ptr(g_prev),
                 _ptr(work), _ptr(G), _ptr(x_out), _ptr(pos_out), _ptr(cell_out), _ptr(fmax_out), _stream(dev))
    if wg_min_atoms is None:
        _check(L.nnhip_cell_lbfgs_step(*head_args, *tail_args), 'nnhip_cell_lbfgs_step')
    else:
        _check(L.nnhip_cell_lbfgs_step_wg(*head_args, wg_min_atoms, *tail_args), 'nnhip_cell_lbfgs_step_wg')


NEB_CHECK_ONLY, NEB_CLIMB =_K['NNHIP_NEB_CHECK_ONLY'], _K['NNHIP_NEB_CLIMB']      # flags of nnhip_neb_step
NEB_MAX_IMAGES = _K['NNHIP_NEB_MAX_IMAGES']
# ase.optimize.FIRE's defaults, in the order nnhip_neb_step takes them: dt, dt_max, n_min, f_inc, f_dec, a_start, f_a, maxstep
NEB_FIRE_DEFAULTS = (0.1, 1.0, 5, 1.1, 0.5, 0.1, 0.99, 0.2)


def neb_step(pos_in: torch.Tensor, force: torch.Tensor, energy: torch.Tensor, free: Optional[torch.Tensor], mol_ptr: torch.Tensor,
             band_ptr: torch.Tensor, band_ptr_host: torch.Tensor, spring: float, tol2: float, climb2: float, fire, flags: int,
             converged: torch.Tensor, climbing: torch.Tensor, n_steps: torch.Tensor, n_pos: torch.Tensor, dt: torch.Tensor,
             a: torch.Tensor, vel: torch.Tensor, pos_out: torch.Tensor, neb_force_out: torch.Tensor, tangent_out: torch.Tensor,
             fmax_out: torch.Tensor, saddle_out: torch.Tensor):
    """One launch of the nudged-elastic-band step (nnhip_neb_step, csrc/neb.hip; the contract is in include/newtonnet_hip.h) on
    the current stream, for the K bands band_ptr (int32 [K+1], device; band_ptr_host: the same on the host) delimits among the B
    molecules of mol_ptr (int32 [B+1]).  pos_in, force [N,3] and energy [B] are read; free: bool / uint8 [N] (False = fixed atom)
    or None; fire = (dt, dt_max, n_min, f_inc, f_dec, a_start, f_a, maxstep).  The state (converged, climbing, n_steps, n_pos int32
    [K]; dt, a fp32 [K]; vel fp32 [N,3]) is updated in place, pos_out, neb_force_out, tangent_out [N,3], fmax_out [K] and saddle_out
    (int32 [K]) are written: all of these must be contiguous tensors of exactly that type (a copy would take the result away).
    pos_out may not overlap pos_in."""
    B, dev, i32 = _offsets('mol_ptr', mol_ptr), mol_ptr.device, torch.int32
    K = _offsets('band_ptr', band_ptr, dev, band_ptr_host)
    N = _n_rows3(pos_out)
    _written(dev, converged=(converged, K, i32), climbing=(climbing, K, i32), n_steps=(n_steps, K, i32), n_pos=(n_pos, K, i32),
             dt=(dt, K), a=(a, K), vel=(vel, 3 * N), pos_out=(pos_out, 3 * N), neb_force_out=(neb_force_out, 3 * N),
             tangent_out=(tangent_out, 3 * N), fmax_out=(fmax_out, K), saddle_out=(saddle_out, K, i32))
    free = _free_mask(free, N, dev)
    pos_in, force, energy = _read(dev, pos_in=(pos_in, 3 * N), force=(force, 3 * N), energy=(energy, B))
    dt0, dt_max, n_min, f_inc, f_dec, a_start, f_a, maxstep = fire
    _check(lib().nnhip_neb_step(_ptr(pos_in), _ptr(force), _ptr(energy), _ptr(free), _ptr(mol_ptr), _ptr(band_ptr),
                                _ptr(band_ptr_host), K, B, N, float(spring), float(tol2), float(climb2), float(dt0), float(dt_max),
                                int(n_min), float(f_inc), float(f_dec), float(a_start), float(f_a), float(maxstep), int(flags),
                                _ptr(converged), _ptr(climbing), _ptr(n_steps), _ptr(n_pos), _ptr(dt), _ptr(a), _ptr(vel),
                                _ptr(pos_out), _ptr(neb_force_out), _ptr(tangent_out), _ptr(fmax_out), _ptr(saddle_out),
                                _stream(dev)), 'nnhip_neb_step')


IRC_CHECK_ONLY = _K['NNHIP_IRC_CHECK_ONLY']                 # flag of nnhip_irc_step
IRC_ACCEL = 0.00964853322        # eV / (Angstrom amu) in Angstrom / fs^2: NNHIP_IRC_ACCEL (include/newtonnet_hip.h), dynamics.FS^2


def irc_step(pos_in: torch.Tensor, force: torch.Tensor, free: Optional[torch.Tensor], masses: torch.Tensor, mol_ptr: torch.Tensor,
             v0: float, delta0: float, dt_min: float, dt_max: float, tol2: float, flags: int, status: torch.Tensor,
             armed: torch.Tensor, n_steps: torch.Tensor, dt: torch.Tensor, dt_prev: torch.Tensor, arc: torch.Tensor,
             vel: torch.Tensor, x_prev: torch.Tensor, v_prev: torch.Tensor, a_prev: torch.Tensor, pos_out: torch.Tensor,
             fmax_out: torch.Tensor):
    """One launch of the reaction-path step (nnhip_irc_step, csrc/irc.hip; the contract is in include/newtonnet_hip.h) on the
    current stream, for the B molecules mol_ptr (int32 [B+1]) delimits.  pos_in, force [N,3] and masses [N] are read; free: bool /
    uint8 [N] (False = fixed atom) or None; the state (status, armed, n_steps int32 [B]; dt, dt_prev, arc fp32 [B]; vel, x_prev,
    v_prev, a_prev fp32 [N,3]) is updated in place, pos_out [N,3] and fmax_out [B] are written: all of these must be contiguous
    tensors of exactly that type (a copy would take the result away).  pos_out may not overlap pos_in."""
    B, dev, i32 = _offsets('mol_ptr', mol_ptr), mol_ptr.device, torch.int32
    N = _n_rows3(pos_out)
    _written(dev, status=(status, B, i32), armed=(armed, B, i32), n_steps=(n_steps, B, i32), dt=(dt, B), dt_prev=(dt_prev, B),
             arc=(arc, B), vel=(vel, 3 * N), x_prev=(x_prev, 3 * N), v_prev=(v_prev, 3 * N), a_prev=(a_prev, 3 * N),
             pos_out=(pos_out, 3 * N), fmax_out=(fmax_out, B))
    free = _free_mask(free, N, dev)
    pos_in, force, masses = _read(dev, pos_in=(pos_in, 3 * N), force=(force, 3 * N), masses=(masses, N))
    _check(lib().nnhip_irc_step(_ptr(pos_in), _ptr(force), _ptr(free), _ptr(masses), _ptr(mol_ptr), B, N, float(v0), float(delta0),
                                float(dt_min), float(dt_max), float(tol2), int(flags), _ptr(status), _ptr(armed), _ptr(n_steps),
                                _ptr(dt), _ptr(dt_prev), _ptr(arc), _ptr(vel), _ptr(x_prev), _ptr(v_prev), _ptr(a_prev),
                                _ptr(pos_out), _ptr(fmax_out), _stream(dev)), 'nnhip_irc_step')


DIMER_CHECK_ONLY = _K['NNHIP_DIMER_CHECK_ONLY']             # flag of nnhip_dimer_step
# rows of its state blocks istate [DIMER_N_INT, B], fstate [DIMER_N_FLOAT, B] and vstate [DIMER_N_VEC, N, 3]
DIMER_N_INT, DIMER_N_FLOAT, DIMER_N_VEC = _K['NNHIP_DIMER_N_INT'], _K['NNHIP_DIMER_N_FLOAT'], _K['NNHIP_DIMER_N_VEC']
DIMER_I = {k[len('NNHIP_DIMER_I_'):].lower(): v for k, v in _K.items() if k.startswith('NNHIP_DIMER_I_')}
DIMER_F = {k[len('NNHIP_DIMER_F_'):].lower(): v for k, v in _K.items() if k.startswith('NNHIP_DIMER_F_')}
DIMER_V = {k[len('NNHIP_DIMER_V_'):].lower(): v for k, v in _K.items() if k.startswith('NNHIP_DIMER_V_')}


def dimer_step(pos_in: torch.Tensor, force: torch.Tensor, energy: Optional[torch.Tensor], free: Optional[torch.Tensor],
               mol_ptr: torch.Tensor, memory: int, delta: float, rot_tol: float, max_rotations: int, tol2: float, alpha: float,
               maxstep: float, flags: int, istate: torch.Tensor, fstate: torch.Tensor, vstate: torch.Tensor, S: torch.Tensor,
               Y: torch.Tensor, rho: torch.Tensor, work: Optional[torch.Tensor], pos_out: torch.Tensor, fmax_out: torch.Tensor,
               energy_out: Optional[torch.Tensor] = None):
    """One launch of the dimer-method step (nnhip_dimer_step, csrc/dimer.hip; the contract is in include/newtonnet_hip.h) on the
    current stream, for the B molecules mol_ptr (int32 [B+1]) delimits.  pos_in (the probes), force [N,3] and energy [B] (or None)
    are read; free: bool / uint8 [N] (False = fixed atom) or None; the state (istate int32 [DIMER_N_INT,B]; fstate fp32
    [DIMER_N_FLOAT,B]; vstate fp32 [DIMER_N_VEC,N,3]; S, Y fp32 [memory,N,3]; rho fp32 [B,memory]) is updated in place, pos_out
    [N,3] (the next probes), fmax_out [B] and energy_out [B] (or None) are written: all of these must be contiguous tensors of
    exactly that type (a copy would take the result away).  work: fp32 [N,3] scratch, needed when N > 64.  pos_out may not overlap
    pos_in."""
    B, dev, m, i32 = _offsets('mol_ptr', mol_ptr), mol_ptr.device, int(memory), torch.int32
    N, rows = _n_rows3(pos_out), max(m, 0)
    _written(dev, optional=('work', 'energy_out'), istate=(istate, DIMER_N_INT * B, i32), fstate=(fstate, DIMER_N_FLOAT * B),
             vstate=(vstate, DIMER_N_VEC * N * 3), S=(S, rows * N * 3), Y=(Y, rows * N * 3), rho=(rho, B * rows), work=(work, 3 * N),
             pos_out=(pos_out, 3 * N), fmax_out=(fmax_out, B), energy_out=(energy_out, B))
    free = _free_mask(free, N, dev)
    pos_in, force, energy = _read(dev, pos_in=(pos_in, 3 * N), force=(force, 3 * N), energy=(energy, B))
    _check(lib().nnhip_dimer_step(_ptr(pos_in), _ptr(force), _ptr(energy), _ptr(free), _ptr(mol_ptr), B, N, m, float(delta),
                                  float(rot_tol), int(max_rotations), float(tol2), float(alpha), float(maxstep), int(flags),
                                  _ptr(istate), _ptr(fstate), _ptr(vstate), _ptr(S), _ptr(Y), _ptr(rho), _ptr(work), _ptr(pos_out),
                                  _ptr(fmax_out), _ptr(energy_out), _stream(dev)), 'nnhip_dimer_step')


REMD_MAX_REPLICAS = _K['NNHIP_REMD_MAX_REPLICAS']


def remd_exchange(energy: torch.Tensor, mol_ptr: torch.Tensor, mol_ptr_host: torch.Tensor, ladder_ptr: torch.Tensor,
                  ladder_ptr_host: torch.Tensor, stream_id: torch.Tensor, dbeta: torch.Tensor, scale_up: torch.Tensor,
                  scale_down: torch.Tensor, sigma_table: torch.Tensor, rank_of_slot: torch.Tensor, slot_of_rank: torch.Tensor,
                  vel: torch.Tensor, sigma: torch.Tensor, n_attempt: torch.Tensor, n_accept: torch.Tensor, attempt: int, seed: int,
                  delta_out: Optional[torch.Tensor] = None, u_out: Optional[torch.Tensor] = None,
                  accepted_out: Optional[torch.Tensor] = None):
    """One launch of the replica-exchange attempt (nnhip_remd_exchange, csrc/remd.hip; the contract is in
    include/newtonnet_hip.h) on the current stream, for the G ladders ladder_ptr (int32 [G+1], device; ladder_ptr_host and
    mol_ptr_host: the same arrays on the host) delimits among the B molecules of mol_ptr (int32 [B+1]).  energy [B], stream_id
    (int32 [G]), dbeta, scale_up, scale_down [B] and sigma_table [n_rows,N] are read; rank_of_slot, slot_of_rank, n_attempt,
    n_accept (int32 [B]), vel [N,3] and sigma [N] are updated in place, delta_out, u_out (fp32 [B]) and accepted_out (int32 [B]) are
    written when given: all of these must be contiguous tensors of exactly that type (a copy would take the result away).
    attempt: the attempt number (its low bit is the parity), an int in 0 .. 2^32 - 1; seed: an int in 0 .. 2^64 - 1."""
    B, dev, i32 = _offsets('mol_ptr', mol_ptr, host=mol_ptr_host), mol_ptr.device, torch.int32
    G = _offsets('ladder_ptr', ladder_ptr, dev, ladder_ptr_host)
    if int(attempt) != attempt or not 0 <= attempt < 2 ** 32 or int(seed) != seed or not 0 <= seed < 2 ** 64:
        raise ValueError(f'attempt: an integer in 0 .. 2^32 - 1 and seed: one in 0 .. 2^64 - 1 expected (got {attempt!r}, {seed!r})')
    if vel.dim() != 2 or vel.shape[1] != 3:
        raise ValueError(f'vel: [N,3] expected (got {tuple(vel.shape)})')
    N = vel.shape[0]
    if sigma_table.dim() != 2 or sigma_table.shape[1] != N:
        raise ValueError(f'sigma_table: [n_rows,{N}] expected (got {tuple(sigma_table.shape)})')
    n_rows = sigma_table.shape[0]
    _written(dev, optional=('delta_out', 'u_out', 'accepted_out'), rank_of_slot=(rank_of_slot, B, i32),
             slot_of_rank=(slot_of_rank, B, i32), n_attempt=(n_attempt, B, i32), n_accept=(n_accept, B, i32), vel=(vel, 3 * N),
             sigma=(sigma, N), delta_out=(delta_out, B), u_out=(u_out, B), accepted_out=(accepted_out, B, i32))
    energy, dbeta, scale_up, scale_down, sigma_table = _read(
        dev, energy=(energy, B), dbeta=(dbeta, B), scale_up=(scale_up, B), scale_down=(scale_down, B),
        sigma_table=(sigma_table, n_rows * N))
    if stream_id.dtype != torch.int32 or stream_id.numel() != G or stream_id.device != dev:
        raise ValueError(f'stream_id: int32 (the bits of a uint32), {G} values on {dev} expected')
    stream_id = stream_id.contiguous()
    attempt, seed = int(attempt), int(seed)
    # (the C ABI has signed scalars only: the same bits)
    _check(lib().nnhip_remd_exchange(_ptr(energy), _ptr(mol_ptr), _ptr(mol_ptr_host), _ptr(ladder_ptr), _ptr(ladder_ptr_host),
                                     _ptr(stream_id), _ptr(dbeta), _ptr(scale_up), _ptr(scale_down), _ptr(sigma_table),
                                     _ptr(rank_of_slot), _ptr(slot_of_rank), _ptr(vel), _ptr(sigma), _ptr(n_attempt), _ptr(n_accept),
                                     _ptr(delta_out), _ptr(u_out), _ptr(accepted_out),
                                     attempt - 2 ** 32 if attempt >= 2 ** 31 else attempt, seed - 2 ** 64 if seed >= 2 ** 63 else seed,
                                     G, B, N, n_rows, _stream(dev)), 'nnhip_remd_exchange')


PIMD_FINISH, PIMD_BEGIN = _K['NNHIP_PIMD_FINISH'], _K['NNHIP_PIMD_BEGIN']      # flags of nnhip_pimd_step
PIMD_MAX_BEADS = _K['NNHIP_PIMD_MAX_BEADS']


def pimd_tile_atoms(n_beads: int) -> int:
    """atoms of one system a workgroup of nnhip_pimd_step handles: every (slot, atom) of the tile has a thread"""
    return _K['NNHIP_PIMD_THREADS'] // int(n_beads)


def pimd_step(u: torch.Tensor, w: torch.Tensor, force: torch.Tensor, ctab: torch.Tensor, mode_tab: torch.Tensor, hk: torch.Tensor,
              mol_ptr: torch.Tensor, mol_ptr_host: torch.Tensor, n_beads: int, flags: int, pos_out: Optional[torch.Tensor] = None,
              pos_pending: Optional[torch.Tensor] = None, mass: Optional[torch.Tensor] = None,
              sigma: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None, est_out: Optional[torch.Tensor] = None):
    """One launch of the path-integral integrator (nnhip_pimd_step, csrc/pimd.hip; the contract is in include/newtonnet_hip.h) on
    the current stream, for the G = B / n_beads ring polymers among the B molecules of mol_ptr (int32 [B+1]; mol_ptr_host: the same
    array on the host).  PIMD_FINISH = the second half kick with the mode forces of `force` (and the estimator terms into
    `est_out` [N,4]), PIMD_BEGIN = half kick, exact free-ring-polymer half step, the PILE step w = c1 w + sigma noise (only with
    `noise`), half step, and the bead positions into `pos_out`.  `u`, `w` [N,3] (mode positions and velocities) are updated in
    place and `pos_out`, `est_out` written: these must be contiguous float32 (a copy would take the result away).  ctab [P,P],
    mode_tab [B,5], hk, mass, sigma [N], noise [N,3] are read.  `pos_out` may not overlap `pos_pending`, the positions the pending
    forward call read."""
    if isinstance(n_beads, bool) or int(n_beads) != n_beads:
        raise ValueError(f'n_beads: an integer expected (got {n_beads!r})')
    if u.dim() != 2 or u.shape[1] != 3:
        raise ValueError(f'u: [N,3] expected (got {tuple(u.shape)})')
    P, N, dev = int(n_beads), u.shape[0], u.device
    B = _offsets('mol_ptr', mol_ptr, dev, mol_ptr_host)
    _written(dev, optional=('pos_out', 'est_out'), u=(u, 3 * N), w=(w, 3 * N), pos_out=(pos_out, 3 * N), est_out=(est_out, 4 * N))
    force, ctab, mode_tab, hk, mass, sigma, noise, pos_pending = _read(
        dev, force=(force, 3 * N), ctab=(ctab, max(P, 0) ** 2), mode_tab=(mode_tab, 5 * B), hk=(hk, N), mass=(mass, N),
        sigma=(sigma, N), noise=(noise, 3 * N), pos_pending=(pos_pending, 3 * N))
    _check(lib().nnhip_pimd_step(_ptr(u), _ptr(w), _ptr(force), _ptr(ctab), _ptr(mode_tab), _ptr(hk), _ptr(mass), _ptr(sigma),
                                 _ptr(noise), _ptr(mol_ptr), _ptr(mol_ptr_host), _ptr(pos_pending), int(flags), P, B, N,
                                 _ptr(pos_out), _ptr(est_out), _stream(dev)), 'nnhip_pimd_step')


BIAS_MAX_CVS, BIAS_THREADS = _K['NNHIP_BIAS_MAX_CVS'], _K['NNHIP_BIAS_THREADS']
BIAS_DISTANCE, BIAS_ANGLE, BIAS_TORSION = _K['NNHIP_BIAS_DISTANCE'], _K['NNHIP_BIAS_ANGLE'], _K['NNHIP_BIAS_TORSION']   # kinds
BIAS_DEPOSIT = _K['NNHIP_BIAS_DEPOSIT']                         # flag of nnhip_bias_step
BIAS_STATUS_INVALID = _K['NNHIP_BIAS_STATUS_INVALID']           # status bit; bits 0 and 1: variable 0 / 1 has no gradient here


def bias_step(pos: torch.Tensor, force_in: torch.Tensor, mol_ptr: torch.Tensor, mol_ptr_host: torch.Tensor, group_ptr: torch.Tensor,
              group_ptr_host: torch.Tensor, cv_def: torch.Tensor, restraint: torch.Tensor, hill_par: torch.Tensor,
              hills: torch.Tensor, n_deposits: int, flags: int, force_out: torch.Tensor, cv_out: torch.Tensor,
              bias_out: torch.Tensor, status_out: torch.Tensor):
    """One launch of the bias on collective variables (nnhip_bias_step, csrc/bias.hip; the contract is in
    include/newtonnet_hip.h) on the current stream, for the G groups group_ptr (int32 [G+1], device; group_ptr_host and
    mol_ptr_host: the same arrays on the host) delimits among the B molecules of mol_ptr (int32 [B+1]).  pos, force_in [N,3], cv_def
    (int32 [B,2,5]), restraint [B,2,2] and hill_par [G,4] are read; hills [G,capacity,4] is read below row n_deposits W and, with
    BIAS_DEPOSIT, written at the W rows from there; force_out [N,3], cv_out, bias_out [B,2] and status_out (int32 [B]) are
    written: these must be contiguous tensors of exactly that type (a copy would take the result away).  force_out may overlap
    neither force_in nor pos."""
    B, dev = _offsets('mol_ptr', mol_ptr, host=mol_ptr_host), mol_ptr.device
    G = _offsets('group_ptr', group_ptr, dev, group_ptr_host)
    if isinstance(n_deposits, bool) or int(n_deposits) != n_deposits or not 0 <= n_deposits < 2 ** 31:
        raise ValueError(f'n_deposits: an integer in 0 .. 2^31 - 1 expected (got {n_deposits!r})')
    if isinstance(flags, bool) or int(flags) != flags or not 0 <= flags < 2 ** 31:
        raise ValueError(f'flags: an integer >= 0 expected (got {flags!r})')
    if not isinstance(force_out, torch.Tensor) or force_out.dim() != 2 or force_out.shape[1] != 3:
        raise ValueError('force_out: a tensor [N,3] expected')
    N = force_out.shape[0]
    if not isinstance(hills, torch.Tensor) or hills.dim() != 3 or hills.shape[0] != G or hills.shape[2] != 4:
        raise ValueError(f'hills: [{G},capacity,4] expected')
    capacity = hills.shape[1]
    _written(dev, hills=(hills, G * capacity * 4), force_out=(force_out, 3 * N), cv_out=(cv_out, 2 * B), bias_out=(bias_out, 2 * B),
             status_out=(status_out, B, torch.int32))
    pos, force_in, restraint, hill_par = _read(dev, pos=(pos, 3 * N), force_in=(force_in, 3 * N),
                                               restraint=(restraint, B * BIAS_MAX_CVS * 2), hill_par=(hill_par, G * 4))
    if cv_def.dtype != torch.int32 or cv_def.numel() != B * BIAS_MAX_CVS * 5 or cv_def.device != dev:
        raise ValueError(f'cv_def: int32, {B * BIAS_MAX_CVS * 5} values on {dev} expected')
    cv_def = cv_def.contiguous()
    _check(lib().nnhip_bias_step(_ptr(pos), _ptr(force_in), _ptr(mol_ptr), _ptr(mol_ptr_host), _ptr(group_ptr), _ptr(group_ptr_host),
                                 _ptr(cv_def), _ptr(restraint), _ptr(hill_par), _ptr(hills), capacity, int(n_deposits), int(flags), G,
                                 B, N, _ptr(force_out), _ptr(cv_out), _ptr(bias_out), _ptr(status_out), _stream(dev)),
           'nnhip_bias_step')


def bias_eval(hills: torch.Tensor, hill_par: torch.Tensor, group: int, n_hills: int, points: torch.Tensor, periods=(0.0, 0.0)):
    """V of group `group` at points [M,2] over the first n_hills rows of its hill list (nnhip_bias_eval, csrc/bias.hip: the hill
    sum of nnhip_bias_step, one workgroup per point); periods: the period of each coordinate as an fp32 value (0: none).
    Returns fp32 [M]."""
    if not isinstance(hills, torch.Tensor) or hills.dim() != 3 or hills.shape[2] != 4:
        raise ValueError('hills: [G,capacity,4] expected')
    G, capacity = hills.shape[0], hills.shape[1]
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 2:
        raise ValueError('points: a tensor [M,2] expected')
    for name, v in (('group', group), ('n_hills', n_hills)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f'{name}: an integer expected (got {v!r})')
    if not 0 <= group < G or not 0 <= n_hills <= capacity:
        raise ValueError(f'group in 0 .. {G - 1} and n_hills in 0 .. {capacity} expected (got {group}, {n_hills})')
    hills, hill_par, points = _f32c(hills, 'hills'), _f32c(hill_par, 'hill_par'), _f32c(points, 'points')
    dev = hills.device
    if hill_par.numel() != 4 * G or hill_par.device != dev or points.device != dev:
        raise ValueError(f'hill_par: {4 * G} values, and points, on {dev} expected')
    p0, p1 = (float(p) for p in periods)
    out = torch.empty(points.shape[0], dtype=torch.float32, device=dev)
    if points.shape[0] == 0:
        return out
    _check(lib().nnhip_bias_eval(_ptr(hills), _ptr(hill_par), _ptr(points), p0, p1, int(group), capacity, int(n_hills),
                                 points.shape[0], G, _ptr(out), _stream(dev)), 'nnhip_bias_eval')
    return out


RDF_MAX_KINDS, RDF_MAX_BINS, RDF_MAX_COUNTERS = _K['NNHIP_RDF_MAX_KINDS'], _K['NNHIP_RDF_MAX_BINS'], _K['NNHIP_RDF_MAX_COUNTERS']


def check_histogram_size(n_kinds: int, n_bins: int):
    """the LDS histogram of nnhip_rdf_accumulate: refused here as the library refuses it, without touching the device"""
    n_kinds, n_bins = int(n_kinds), int(n_bins)
    if not (1 <= n_kinds <= RDF_MAX_KINDS and 1 <= n_bins <= RDF_MAX_BINS and n_kinds * (n_kinds + 1) // 2 * n_bins <= RDF_MAX_COUNTERS):
        raise ValueError(f'{n_kinds} kinds and {n_bins} bins are outside the histogram kernel: at most {RDF_MAX_KINDS} kinds, '
                         f'{RDF_MAX_BINS} bins and n_kinds (n_kinds + 1) / 2 * n_bins <= {RDF_MAX_COUNTERS}')


def _frames(name, t, dev=None):
    """a block of frames [F,N,3]: float32, on `dev` when given, each frame contiguous (the frame stride is free); returns (F, N, stride)"""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f'{name}: a float32 tensor [F,N,3] expected')
    F, N = t.shape[0], t.shape[1]
    if N and (t.stride(2) != 1 or t.stride(1) != 3 or (F > 1 and t.stride(0) < 3 * N)):
        raise ValueError(f'{name}: contiguous frames expected (strides {tuple(t.stride())})')
    if dev is not None and t.device != dev:
        raise ValueError(f'{name}: on {dev} expected (it is on {t.device})')
    return F, N, (t.stride(0) if F > 1 else 3 * N)


def _kinds(kind, N, dev):
    if not isinstance(kind, torch.Tensor) or kind.dtype != torch.int32 or not kind.is_contiguous() or kind.numel() != N or kind.device != dev:
        raise ValueError(f'kind: a contiguous int32 tensor [{N}] on {dev} expected')


def rdf_accumulate(pos: torch.Tensor, cell: torch.Tensor, mol_ptr: torch.Tensor, kind: torch.Tensor, n_kinds: int,
                   edge2: torch.Tensor, counts: torch.Tensor, max_atoms: int):
    """Add the pair-distance histogram of the frames pos [F,N,3] to counts, int64 [B, n_kinds (n_kinds + 1) / 2, n_bins]
    (nnhip_rdf_accumulate, csrc/observables.hip; include/newtonnet_hip.h states which pair lands where).  cell: [B,3,3] (every frame)
    or [F,B,3,3]; mol_ptr int32 [B+1]; kind int32 [N] (0 .. n_kinds - 1, -1 = ignored); edge2 fp32 [n_bins + 1]: the bin edges as
    thresholds on r2; max_atoms: the size of the largest system."""
    dev = pos.device if isinstance(pos, torch.Tensor) else None
    F, N, stride = _frames('pos', pos)
    B = _offsets('mol_ptr', mol_ptr, dev)
    _kinds(kind, N, dev)
    if not isinstance(edge2, torch.Tensor) or edge2.dtype != torch.float32 or not edge2.is_contiguous() or edge2.dim() != 1 \
            or edge2.numel() < 2 or edge2.device != dev:
        raise ValueError(f'edge2: a contiguous float32 tensor [n_bins + 1] on {dev} expected')
    n_bins, n_kinds = edge2.numel() - 1, int(n_kinds)
    check_histogram_size(n_kinds, n_bins)
    _written(dev, counts=(counts, B * (n_kinds * (n_kinds + 1) // 2) * n_bins, torch.int64))
    if not isinstance(cell, torch.Tensor) or cell.dtype != torch.float32 or not cell.is_contiguous() or cell.device != dev \
            or tuple(cell.shape) not in ((B, 3, 3), (F, B, 3, 3)):
        raise ValueError(f'cell: a contiguous float32 tensor [{B},3,3] or [{F},{B},3,3] on {dev} expected')
    cell_stride = 9 * B if cell.dim() == 4 else 0
    if not 0 <= int(max_atoms) <= N:
        raise ValueError(f'max_atoms: 0 .. {N} expected (got {max_atoms})')
    _check(lib().nnhip_rdf_accumulate(_ptr(pos), stride, F, _ptr(cell), cell_stride, _ptr(mol_ptr), B, N, int(max_atoms), _ptr(kind),
                                      n_kinds, _ptr(edge2), n_bins, _ptr(counts), _stream(dev)), 'nnhip_rdf_accumulate')


TC_PRODUCT, TC_DISPLACEMENT = 0, 1          # modes of nnhip_time_correlation


def check_correlation(n_frames: int, max_lag, origin_every, mode=TC_PRODUCT):
    """the arguments nnhip_time_correlation refuses, refused here without touching the device; returns (max_lag, origin_every)"""
    if int(max_lag) != max_lag or not 0 <= max_lag < n_frames:
        raise ValueError(f'max_lag: an integer in 0 .. n_frames - 1 = {n_frames - 1} expected (got {max_lag!r}): a lag needs two '
                         f'frames that far apart')
    if int(origin_every) != origin_every or origin_every < 1:
        raise ValueError(f'origin_every: an integer >= 1 expected (got {origin_every!r})')
    if mode not in (TC_PRODUCT, TC_DISPLACEMENT):
        raise ValueError(f'mode: {TC_PRODUCT} (product) or {TC_DISPLACEMENT} (squared displacement) expected (got {mode!r})')
    return int(max_lag), int(origin_every)


def time_correlation(x: torch.Tensor, mol_ptr: torch.Tensor, kind: torch.Tensor, n_kinds: int, mode: int, max_lag: int,
                     sums: torch.Tensor, origin_every: int = 1, weight: Optional[torch.Tensor] = None):
    """Add the lagged correlation of the frames x [F,N,3] to sums, fp64 [B, n_kinds, max_lag + 1] (nnhip_time_correlation,
    csrc/observables.hip): per system, kind and lag the sum over origins 0, origin_every, ... and atoms of x(t0) . x(t0 + l)
    (TC_PRODUCT) or |x(t0 + l) - x(t0)|^2 (TC_DISPLACEMENT), times weight [N] when given.  fp32 terms, fp64 sums in a fixed order."""
    dev = x.device if isinstance(x, torch.Tensor) else None
    F, N, stride = _frames('x', x)
    max_lag, origin_every = check_correlation(F, max_lag, origin_every, mode)
    B = _offsets('mol_ptr', mol_ptr, dev)
    _kinds(kind, N, dev)
    n_kinds = int(n_kinds)
    if not 1 <= n_kinds <= RDF_MAX_KINDS:
        raise ValueError(f'n_kinds: 1 .. {RDF_MAX_KINDS} expected (got {n_kinds})')
    _written(dev, sums=(sums, B * n_kinds * (max_lag + 1), torch.float64))
    weight, = _read(dev, weight=(weight, N))
    _check(lib().nnhip_time_correlation(_ptr(x), stride, F, _ptr(mol_ptr), B, N, _ptr(kind), n_kinds, _ptr(weight), int(mode),
                                        max_lag, origin_every, _ptr(sums), _stream(dev)), 'nnhip_time_correlation')


def gather_rows(x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """out[e] = x[idx[e]] (idx int32)."""
    x = _f32c(x, 'x')
    width = int(torch.tensor(x.shape[1:]).prod())
    out = torch.empty((idx.numel(),) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    _check(lib().nnhip_gather_rows(_ptr(x), _ptr(idx), idx.numel(), width, _ptr(out), _stream(x.device)),
           'nnhip_gather_rows')
    return out


def timers_enable(on, classes=None):
    """Event timers of the library on / off.  `classes` (names of TIMER_CLASSES): only those classes record events."""
    if on and classes:
        mask = 0
        for name in classes:
            mask |= 1 << (TIMER_CLASSES.index(name) + 1)
        _check(lib().nnhip_timers_enable(mask), 'nnhip_timers_enable')
    else:
        _check(lib().nnhip_timers_enable(1 if on else 0), 'nnhip_timers_enable')


def split_products() -> bool:
    """True when the dense kernels use the split-f16 product form (default; NNHIP_MLP_SPLIT=0 selects fp32 MFMA)."""
    return bool(lib().nnhip_split_products())


def timers_read(reset: bool = True):
    ms = (C.c_double * N_TIMER_CLASSES)()
    cnt = (C.c_int64 * N_TIMER_CLASSES)()
    _check(lib().nnhip_timers_read(ms, cnt, 1 if reset else 0), 'nnhip_timers_read')
    return {name: (ms[k], cnt[k]) for k, name in enumerate(TIMER_CLASSES)}
