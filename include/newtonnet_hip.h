/*
 * newtonnet_hip.h -- C ABI of libnewtonnet_hip.so (gfx950 / MI355X).
 *
 * The reference (THGLab/NewtonNet v2.1.0) is pure Python: the hot path has no
 * FFI of its own.  The entry points below are the operations its model forward
 * dispatches through PyTorch, cut where a maintainer would bind a native
 * extension (INTEGRATION.md shows the ctypes stub).  Each one cites the
 * reference code it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - all floating-point data is fp32, row-major, contiguous; indices are
 *     int32 inside the library and int64 where the reference API exposes them;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *     nothing synchronises the device except where stated;
 *   - the library never allocates device memory: callers own every buffer
 *     (PyTorch does, in the shipped host code);
 *   - return value 0 = success, anything else = error; nnhip_last_error()
 *     returns a static description for the calling thread.
 *   - F = n_features must be 128 (the reference's default, scripts/config.yml:30-36); nb = n_basis may be
 *     1..NNHIP_MAX_NB (default 20); other sizes return NNHIP_E_UNSUPPORTED.
 */
#ifndef NEWTONNET_HIP_H
#define NEWTONNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NNHIP_F 128
#define NNHIP_NB 20        /* the reference's default n_basis */
#define NNHIP_MAX_NB 32    /* any 1 <= n_basis <= 32 runs: only the radial-filter table builder sees the basis */
#define NNHIP_MAX_LAYERS 8
#define NNHIP_MOL_STAGE_MAX 24 /* atoms of a molecule whose node rows the molecule-resident edge kernels stage in LDS */
#define NNHIP_N_ELEMENTS 119 /* rows of node_embedding / scale / shift (z = 0..118) */
/* cutoff envelope of the edge embedding: a positive value p = PolynomialCutoff(p) (representations.py:138-171; the model
 * uses p = 9, :17; 0 means 9), NNHIP_ENVELOPE_COSINE = CosineCutoff (representations.py:177-203) */
#define NNHIP_ENVELOPE_COSINE (-1)

/* activation ids (newtonnet/layers/activations.py:5-30); 'swish' and 'silu' are both NNHIP_ACT_SILU */
enum {
  NNHIP_ACT_SILU = 0,
  NNHIP_ACT_RELU = 1,
  NNHIP_ACT_ELU = 2,
  NNHIP_ACT_LEAKY_RELU = 3,
  NNHIP_ACT_TANH = 4,
  NNHIP_ACT_SIGMOID = 5,
  NNHIP_ACT_SOFTPLUS = 6,
  NNHIP_ACT_GELU = 7,
  NNHIP_ACT_SSP = 8
};

enum {
  NNHIP_OK = 0,
  NNHIP_E_INVALID = 1,      /* bad argument */
  NNHIP_E_UNSUPPORTED = 2,  /* n_features / n_basis / n_layers outside the built kernels */
  NNHIP_E_WORKSPACE = 3,    /* workspace too small */
  NNHIP_E_HIP = 4           /* a HIP runtime call or kernel launch failed */
};

int nnhip_version(void);
/* bit 0: tooling build (compiled with extra flags, e.g. an ablation switch that changes results); the Python package refuses
 * to load such a library unless NNHIP_ALLOW_TOOLING_LIB=1 */
int nnhip_build_flags(void);
const char* nnhip_last_error(void);

/* --------------------------------------------------------------------------
 * Parameters of one model, in the reference's state_dict layout
 * (nn.Linear weights are [out][in] row-major).
 * Replaces: the nn.Module parameter storage of
 *   newtonnet/models/newtonnet.py:116-205 and newtonnet/models/output.py:88-96,
 *   newtonnet/layers/scalers.py:42-45.
 * ------------------------------------------------------------------------ */
typedef struct {
  const float* node0_w;  /* interaction_layers.l.message_nodepart.0.weight [F][F] */
  const float* node0_b;  /* ...message_nodepart.0.bias   [F] */
  const float* node2_w;  /* ...message_nodepart.2.weight [F][F] */
  const float* node2_b;  /* ...message_nodepart.2.bias   [F] */
  const float* edge_w;   /* ...message_edgepart.weight   [F][nb] */
  const float* eq1_0_w;  /* ...equiv_message1.0.weight   [F][F] */
  const float* eq1_2_w;  /* ...equiv_message1.2.weight   [F][F] */
  const float* eq2_0_w;  /* ...equiv_message2.0.weight   [F][F] */
  const float* eq2_2_w;  /* ...equiv_message2.2.weight   [F][F] */
  const float* update_w; /* ...equiv_update.weight       [F][F] */
  const float* ln_w;     /* ...layer_norm.weight         [F]  (NULL with ln_b: layer_norm=False, newtonnet.py:202-205) */
  const float* ln_b;     /* ...layer_norm.bias           [F] */
} nnhip_layer_params;

typedef struct {
  int32_t n_features; /* 128 */
  int32_t n_basis;    /* 1..NNHIP_MAX_NB (20 in the reference's configs) */
  int32_t n_layers;   /* 1..NNHIP_MAX_LAYERS */
  float cutoff;       /* Angstrom */
  const float* node_embedding; /* embedding_layers.node_embedding.weight [119][F] */
  const float* frequencies;    /* embedding_layers.edge_embedding.embedding.frequencies [nb] */
  nnhip_layer_params layer[NNHIP_MAX_LAYERS];
  const float* head0_w; /* output_layers.k.layers.0.weight [F][F] */
  const float* head0_b; /* [F] */
  const float* head2_w; /* output_layers.k.layers.2.weight [F][F] */
  const float* head2_b; /* [F] */
  const float* head4_w; /* output_layers.k.layers.4.weight [1][F] */
  const float* head4_b; /* [1] */
  const float* scale;   /* scalers.k.scale.weight [119] (NULL = 1) */
  const float* shift;   /* scalers.k.shift.weight [119] (NULL = 0) */
  int32_t activation;   /* NNHIP_ACT_* of every MLP of the model (constructor argument `activation`, newtonnet.py:30) */
  int32_t envelope;     /* cutoff envelope (see NNHIP_ENVELOPE_COSINE); 0 = the model's PolynomialCutoff(9) */
} nnhip_model;

/* --------------------------------------------------------------------------
 * Neighbor list.
 * Replaces: RadiusGraph.forward, newtonnet/layers/representations.py:57-100
 *   (all ordered pairs inside a molecule, i != j, optional single-image
 *   minimum-image shift d -= cell @ round(solve(cell^T, d)), strict ||d|| < r).
 * Contract: `batch` is non-decreasing (PyG collation order).  Edges come out
 * sorted by (molecule, i, j) -- the reference's order -- so the list is a CSR
 * over the RECEIVER i = edge_index[0].
 *
 * nnhip_graph_count: writes row_ptr[N+1] (exclusive scan of the in-degree) and
 *   mol_ptr[B+1].  status is int32[1 + ceil(n_atoms/1024)]: status[0] gets bit 1 if `batch` is not sorted (an error) and
 *   bit 8 if a molecule has more than NNHIP_MOL_STAGE_MAX atoms (information for the choice of edge kernels, not an error);
 *   the rest is scratch of the prefix scan.
 *   The caller reads E = row_ptr[N] (a device->host copy; the only sync).
 * nnhip_graph_fill: writes col[E] (sender j), rev[E] (index of the reverse
 *   edge (j,i); the edge set is symmetric), disp[E][3] = pos_i - pos_j (after
 *   the image shift) and, if non-NULL, edge_index[2][E] int64 (reference API).
 * ------------------------------------------------------------------------ */
int nnhip_graph_count(const float* pos, const float* cell, const int64_t* batch, int32_t n_atoms, int32_t n_mol,
                      float cutoff, int32_t* mol_ptr, int32_t* row_ptr, int32_t* status, void* stream);

int nnhip_graph_fill(const float* pos, const float* cell, const int64_t* batch, const int32_t* mol_ptr,
                     const int32_t* row_ptr, int32_t n_atoms, int32_t n_mol, int32_t n_edges, float cutoff,
                     int32_t* col, int32_t* rev, float* disp, int64_t* edge_index, void* stream);
/* The same neighbor list with fewer launches behind the host's edge-count round trip (the path NewtonNet.forward takes):
 * nnhip_graph_count_pairs also leaves, per row, the number of neighbors ABOVE the row's atom (the undirected pairs the row owns)
 * in pair_cnt[0 .. N); nnhip_graph_pair_scan turns them into pair_ptr[0 .. N] (exclusive scan, in place; it can run while the
 * host waits for the edge count); nnhip_graph_finish = nnhip_graph_fill + nnhip_graph_pairs' pid + nnhip_edge_embed in two
 * launches (fill; then one thread per edge: reverse edge, pair id, geometry / radial basis / table position).  Bit-identical
 * outputs to the separate entry points. */
int nnhip_graph_count_pairs(const float* pos, const float* cell, const int64_t* batch, int32_t n_atoms, int32_t n_mol,
                            float cutoff, int32_t* mol_ptr, int32_t* row_ptr, int32_t* status, int32_t* pair_cnt, void* stream);
int nnhip_graph_pair_scan(int32_t* pair_ptr, int32_t n_atoms, int32_t* scan_scratch, void* stream);
int nnhip_graph_finish(const float* pos, const float* cell, const int64_t* batch, const int32_t* mol_ptr,
                       const int32_t* row_ptr, const int32_t* pair_ptr, int32_t n_atoms, int32_t n_mol, int32_t n_edges,
                       float cutoff, int32_t* col, int32_t* rev, int32_t* pid, float* disp, int64_t* edge_index,
                       const float* frequencies, int32_t n_basis, float* geo, float* rbf, float* drbf, int32_t* xg,
                       int32_t envelope, void* stream);
/* The same two launches BEFORE the host has read the edge count: every array holds `capacity` edges (edge_index 2 x capacity
 * int64; its rows are written at the true stride, so the first 2 E entries are the contiguous [2][E] result), the kernels take the
 * count from row_ptr[n_atoms] on the device and write nothing when it exceeds `capacity` -- the caller, who learns E from its
 * read-back, then calls nnhip_graph_finish.  Fills the GPU's idle time behind the edge-count round trip. */
int nnhip_graph_finish_early(const float* pos, const float* cell, const int64_t* batch, const int32_t* mol_ptr,
                             const int32_t* row_ptr, const int32_t* pair_ptr, int32_t n_atoms, int32_t n_mol, int32_t capacity,
                             float cutoff, int32_t* col, int32_t* rev, int32_t* pid, float* disp, int64_t* edge_index,
                             const float* frequencies, int32_t n_basis, float* geo, float* rbf, float* drbf, int32_t* xg,
                             int32_t envelope, void* stream);

/* --------------------------------------------------------------------------
 * Undirected pairs.  msg = (W_e rbf) * m[i] * m[j] (newtonnet.py:211) is symmetric under i <-> j, and so is everything
 * equiv_message1/2 compute from it (newtonnet.py:218,222): nnhip_energy_forces evaluates msg / hidden / phi once per
 * undirected pair.  pid[e] = pair row of directed edge e (pairs numbered in CSR order of their i < j edge);
 * pair_ptr[N+1] = first pair owned by each row.  n_edges must be even (symmetric edge set).
 * ------------------------------------------------------------------------ */
int nnhip_graph_pairs(const int32_t* row_ptr, const int32_t* col, const int32_t* rev, int32_t n_atoms, int32_t n_edges,
                      int32_t* pair_ptr, int32_t* pid, int32_t* scan_scratch /* int32[ceil(n_atoms/1024)] */, void* stream);

/* --------------------------------------------------------------------------
 * O(N) variant of the neighbor list for ONE large orthorhombic periodic box (BASELINE config 5; the reference's
 * all-pairs build, representations.py:74-85, needs O(N^2) memory and cannot run it).  Bit-identical output to
 * nnhip_graph_count/fill (same predicate, same displacement arithmetic, same edge order); candidates are pruned
 * with a grid of cells >= cutoff wide.  box_len_host = the three diagonal cell entries (HOST pointer); every
 * length must be >= 3 x cutoff (else NNHIP_E_UNSUPPORTED: use the all-pairs entry points).
 * scratch: nnhip_graph_cells_scratch_bytes() bytes, kept between the count and fill calls.
 * ------------------------------------------------------------------------ */
size_t nnhip_graph_cells_scratch_bytes(int32_t n_atoms, const float* box_len_host, float cutoff);
int nnhip_graph_count_cells(const float* pos, const float* cell, int32_t n_atoms, float cutoff,
                            const float* box_len_host, void* scratch, int32_t* mol_ptr, int32_t* row_ptr, void* stream);
int nnhip_graph_fill_cells(const float* pos, const float* cell, int32_t n_atoms, int32_t n_edges, float cutoff,
                           const float* box_len_host, void* scratch, const int32_t* row_ptr, int32_t* col, int32_t* rev,
                           float* disp, int64_t* edge_index, void* stream);
/* The cell-list counterparts of nnhip_graph_count_pairs / nnhip_graph_finish (same outputs as the separate entry points) */
int nnhip_graph_count_cells_pairs(const float* pos, const float* cell, int32_t n_atoms, float cutoff, const float* box_len_host,
                                  void* scratch, int32_t* mol_ptr, int32_t* row_ptr, int32_t* pair_cnt, void* stream);
int nnhip_graph_finish_cells(const float* pos, const float* cell, int32_t n_atoms, int32_t n_edges, float cutoff,
                             const float* box_len_host, void* scratch, const int32_t* row_ptr, const int32_t* pair_ptr,
                             int32_t* col, int32_t* rev, int32_t* pid, float* disp, int64_t* edge_index,
                             const float* frequencies, int32_t n_basis, float* geo, float* rbf, float* drbf, int32_t* xg,
                             int32_t envelope, void* stream);

/* --------------------------------------------------------------------------
 * Verlet-skin reuse of a neighbor list in an MD loop (caller: MLAseCalculator.calculate,
 * newtonnet/utils/ase_interface.py:52-81, which rebuilds the O(N^2) graph every step).
 * nnhip_edge_disp: disp[e] = pos_i - pos_j (+ the reference's single-image shift) for the edges of a list built
 *   earlier with cutoff + skin (edge_index[2][E] int64 from nnhip_graph_fill).  nnhip_edge_embed with the real cutoff
 *   then points candidates with r >= cutoff at all-zero filter rows, so they contribute exactly nothing.
 * ------------------------------------------------------------------------ */
int nnhip_edge_disp(const float* pos, const float* cell, const int64_t* batch, const int64_t* edge_index, int32_t n_edges,
                    float* disp, void* stream);
/* nnhip_edge_disp followed by nnhip_edge_embed, in one launch (the per-step refresh of a reused candidate list) */
int nnhip_edge_refresh(const float* pos, const float* cell, const int64_t* batch, const int64_t* edge_index, int32_t n_edges,
                       float cutoff, const float* frequencies, int32_t n_basis, float* disp, float* geo, float* rbf, float* drbf,
                       int32_t* xg, int32_t envelope, void* stream);

/* --------------------------------------------------------------------------
 * Species check.  The reference indexes nn.Embedding(119, F) / the scale and shift tables with z and raises
 * IndexError for z outside 0..118 (newtonnet.py:142, scalers.py:55-58); the kernels would read out of bounds.
 * ORs 2 into status[0] (the word nnhip_graph_count ORs 1 into for a bad batch vector; the host reads it back
 * together with the edge count) when any z[i] is outside [0, NNHIP_N_ELEMENTS).
 * ------------------------------------------------------------------------ */
int nnhip_check_species(const int64_t* z, int32_t n_atoms, int32_t* status, void* stream);

/* --------------------------------------------------------------------------
 * Edge embedding.
 * Replaces: ScaledNorm.forward (representations.py:118-133), PolynomialCutoff
 *   p=9 (:155-171), RadialBesselLayer.forward (:223-235) and their product (:41).
 * geo[E][4]  = (ux, uy, uz, r)    dir_edge and |disp|
 * rbf[E][nb] = env(x) * sin(w_n x)/x,  x = r/cutoff        (= dist_edge; may be NULL)
 * drbf[E][nb]= d rbf / d x                                  (may be NULL)
 * xg[E][2]   = (g0, bits of u): x = (g0 + u) / FT_G, the position of the edge on the radial-filter table that
 *              nnhip_energy_forces interpolates instead of contracting rbf with message_edgepart.weight per edge
 *              (may be NULL).  A candidate that fails the neighbor predicate `|disp| < cutoff` (fp32, as
 *              representations.py:96) gets the all-zero filter row and is masked out of the force kernels.
 * ------------------------------------------------------------------------ */
int nnhip_edge_embed(const float* disp, int32_t n_edges, float cutoff, const float* frequencies, int32_t n_basis,
                     float* geo, float* rbf, float* drbf, int32_t* xg, int32_t envelope, void* stream);

/* --------------------------------------------------------------------------
 * Whole hot path: energy and forces (= -dE/dpos) for a batch.
 * Replaces: NewtonNet.forward after the graph build, i.e.
 *   EmbeddingNet.forward newtonnet/models/newtonnet.py:139-161 (node part),
 *   InteractionNet.forward :207-231 for every layer,
 *   EnergyOutput.forward output.py:98-100, ScaleShift.forward scalers.py:47-59,
 *   EnergyAggregator.forward output.py:245-247,
 *   and the reverse sweep torch.autograd.grad performs for
 *   GradientForceOutput (output.py:66-73,109-113), written out analytically.
 *
 * workspace: nnhip_workspace_bytes(...) bytes, 256-byte aligned.  Per-layer
 * intermediates stay in it after the call; nnhip_workspace_layout() reports
 * where (used by the parity tests).
 * Optional outputs (may be NULL): atom_energy[N], atom_node[N][F],
 * force_node[N][3][F], virial[B][3][3] (= -dE/d strain, output.py:154-165).
 * forces may be NULL (energy only: forward sweep only).  pos / cell are read only for the virial (may be NULL
 * otherwise); with periodic cells the virial follows the reference's own strain formula, including the
 * `cell @ n` image shift of representations.py:93.
 * ------------------------------------------------------------------------ */
size_t nnhip_workspace_bytes(int32_t n_atoms, int32_t n_edges, int32_t n_mol, int32_t n_layers);

typedef struct {
  /* byte offsets into the workspace; per-layer arrays indexed by layer */
  size_t m[NNHIP_MAX_LAYERS];      /* [N][F]   message_nodepart output */
  size_t hn[NNHIP_MAX_LAYERS];     /* [N][F]   message_nodepart hidden pre-activation */
  size_t msg[NNHIP_MAX_LAYERS];    /* [P][F]   message, one row per undirected pair (P = E/2, row pid[e]) */
  size_t h12[NNHIP_MAX_LAYERS];    /* 2 x [pad32(P)][F] scratch between the equiv_message{1,2} forward and its adjoint, private to
                                      the MLP kernels: the hidden pre-activations h, row-major, up to 26 624 pair rows; above that
                                      silu'(h) in MFMA-fragment order (all the adjoint needs of h) */
  size_t phi1[NNHIP_MAX_LAYERS];   /* [P][F] */
  size_t phi2[NNHIP_MAX_LAYERS];   /* [P][F] */
  size_t a_mid[NNHIP_MAX_LAYERS];  /* [N][F]   atom_node after the invariant update */
  /* hn[0] is not written: layer 0's message_nodepart is evaluated per element (its adjoint is never needed) */
  size_t a_out[NNHIP_MAX_LAYERS];  /* [N][F]   atom_node after the layer (last layer: only when atom_node == NULL) */
  size_t f_out[NNHIP_MAX_LAYERS];  /* [N][3][F] force_node after the layer (last layer: only when force_node == NULL) */
  size_t q[NNHIP_MAX_LAYERS];      /* [N][3][F] equiv_update(force_node) */
  size_t a0;                       /* [N][F]   embedded atom_node */
  size_t e1, e2;                   /* [N][F]   head hidden pre-activations */
  size_t g_x;                      /* [L][E]   dE/dx per layer */
  size_t g_u;                      /* [L][E][3] dE/d dir per layer (only [E][4] rows: gx,guy..) */
  size_t g_a;                      /* [N][F]   running dE/d atom_node */
  size_t g_f;                      /* [N][3][F] running dE/d force_node */
  size_t total;
} nnhip_ws_layout;

int nnhip_workspace_layout(int32_t n_atoms, int32_t n_edges, int32_t n_mol, int32_t n_layers, nnhip_ws_layout* out);

int nnhip_energy_forces(const nnhip_model* model, const int64_t* z, const float* pos, const float* cell,
                        const int32_t* mol_ptr,
                        const int32_t* row_ptr, const int32_t* col, const int32_t* rev, const int32_t* pid, const float* geo,
                        const int32_t* xg, const float* disp, int32_t n_atoms, int32_t n_edges,
                        int32_t n_mol, void* workspace, size_t workspace_bytes, float* energy, float* forces,
                        float* virial, float* atom_energy, float* atom_node, float* force_node,
                        const void* prepared, void* stream);

/* The same step queued BEFORE the host knows the edge count: no device->host round trip inside a step, so a slow host costs
 * nothing (the reference has no counterpart: RadiusGraph.forward, representations.py:57-100, is synchronous by construction;
 * the caller it serves is still NewtonNet.forward, newtonnet.py:74-104).
 *   nnhip_graph_finish_dev   = nnhip_graph_finish_early into arrays of `capacity` edges (even, > 0) + a guard: when the count
 *       (row_ptr[n_atoms]) exceeds the capacity nothing was filled and the guard EMPTIES the graph on the device
 *       (every row becomes [count, count), pair_ptr all zero; graph.hip:graph_guard_kernel), so that the step below runs on zero edges, inside the arrays; likewise when the status word
 *       of nnhip_graph_count_pairs / nnhip_check_species carries bit 1 or 2 (the synchronous path raises on those BEFORE it
 *       runs the step: a broken batch vector can give an edge set without reverse edges).
 *   nnhip_energy_forces_dev  = nnhip_energy_forces with n_edges := capacity (array / workspace sizes,
 *       nnhip_workspace_bytes(n_atoms, capacity, ...)) and the true number of undirected pairs read on the device from
 *       *n_pairs_dev (= &pair_ptr[n_atoms]).
 * The host copies (row_ptr[n_atoms], status) out asynchronously BEFORE nnhip_graph_finish_dev and looks at them whenever it
 * likes (NewtonNet.forward: when a result of the call is first touched, or when the next call starts): count > capacity or a
 * stale prepared block => repeat the step the ordinary way; status bits 1 / 2 => the reference's ValueError / IndexError.
 * Species outside [0, 118] never index a table (the kernels clamp them; the status bit reports them). */
/* nnhip_graph_count_pairs with the species check of nnhip_check_species riding in its molecule-extent kernel (z may be NULL) and
 * pair_ptr scanned in the same two launches as row_ptr (pair_scan_scratch: n_atoms / 1024 + 1 ints) -- what the deferred step
 * uses instead of nnhip_graph_count_pairs + nnhip_check_species + nnhip_graph_pair_scan (three launches less). */
int nnhip_graph_count_pairs_z(const float* pos, const float* cell, const int64_t* batch, const int64_t* z, int32_t n_atoms,
                              int32_t n_mol, float cutoff, int32_t* mol_ptr, int32_t* row_ptr, int32_t* status,
                              int32_t* pair_ptr, int32_t* pair_scan_scratch, void* stream);
int nnhip_graph_finish_dev(const float* pos, const float* cell, const int64_t* batch, const int32_t* mol_ptr,
                           int32_t* row_ptr, int32_t* pair_ptr, int32_t n_atoms, int32_t n_mol, int32_t capacity,
                           float cutoff, int32_t* col, int32_t* rev, int32_t* pid, float* disp, int64_t* edge_index,
                           const float* frequencies, int32_t n_basis, float* geo, float* rbf, float* drbf, int32_t* xg,
                           int32_t envelope, const int32_t* status, int32_t* tail_host /* 4 ints, pinned host memory, or NULL */,
                           const int32_t* changes /* nnhip_prepare_check_counter's counter, or NULL */,
                           int32_t seq /* stored into tail_host[3] after the three words */, void* stream);
int nnhip_energy_forces_dev(const nnhip_model* model, const int64_t* z, const float* pos, const float* cell,
                            const int32_t* mol_ptr,
                            const int32_t* row_ptr, const int32_t* col, const int32_t* rev, const int32_t* pid, const float* geo,
                            const int32_t* xg, const float* disp, int32_t n_atoms, int32_t capacity,
                            int32_t n_mol, void* workspace, size_t workspace_bytes, float* energy, float* forces,
                            float* virial, float* atom_energy, float* atom_node, float* force_node,
                            const void* prepared, const int32_t* n_pairs_dev, void* stream);

/* The neighbor list of a small system (1 .. 1024 atoms; nnhip_forward_dev uses it up to nnhip_graph_small_max_atoms() = 128, where one
 * workgroup still beats fourteen parallel launches) in ONE launch: everything nnhip_graph_count_pairs,
 * nnhip_check_species, nnhip_graph_pair_scan and nnhip_graph_finish_dev do, as the phases of one workgroup (same list, bit for
 * bit).  tail[0] = the true edge count, tail[1] = the status bits, tail[2] = *changes; when the count exceeds `capacity` or a status bit 1 / 2 is
 * set, row_ptr / pair_ptr come back all-zero (an emptied graph, as nnhip_graph_finish_dev leaves one).  Used by nnhip_forward_dev. */
int nnhip_graph_small_dev(const float* pos, const float* cell, const int64_t* batch, const int64_t* z, int32_t n_atoms,
                          int32_t n_mol, int32_t capacity, float cutoff, int32_t* mol_ptr, int32_t* row_ptr,
                          int32_t* pair_ptr, int32_t* tail /* 4 ints; may be pinned host memory */,
                          const int32_t* changes /* or NULL */, int32_t seq /* -> tail[3], last */, int32_t* col, int32_t* rev, int32_t* pid, float* disp,
                          int64_t* edge_index, const float* frequencies, int32_t n_basis, float* geo, int32_t* xg,
                          int32_t envelope, void* stream);
int nnhip_graph_small_max_atoms(void);

/* The neighbor list of a batch of small molecules, one workgroup per molecule (graph.hip:graph_mol_count_kernel,
 * graph_mol_fill_kernel): what nnhip_graph_count_pairs_z + nnhip_graph_finish_dev do in eight launches, in five (init, molecule
 * extents + species check, counts, fill, the guard; four with initialised != 0: the caller has zeroed status[0] and
 * mol_ptr[0 .. n_mol]).  Serves molecules of up to 1024 atoms; nnhip_forward_dev uses it when flags bit 0 says the batch holds small
 * molecules only.  status: one int32 (bits 1 / 2 as nnhip_graph_count / nnhip_check_species; 8: a molecule above
 * NNHIP_MOL_STAGE_MAX atoms; 16: a molecule above 1024 atoms -- the graph is emptied).  scratch: 2 n_mol + n_mol / 1024 + 4 ints
 * (any content).  tail_host / changes / seq, the emptied graph and the list itself: as nnhip_graph_finish_dev (bit for bit the
 * same list; geo / xg as nnhip_edge_embed without rbf). */
int nnhip_graph_mol_dev(const float* pos, const float* cell, const int64_t* batch, const int64_t* z, int32_t n_atoms,
                        int32_t n_mol, int32_t capacity, float cutoff, int32_t* mol_ptr, int32_t* row_ptr, int32_t* pair_ptr,
                        int32_t* status, int32_t* scratch, int32_t initialised, int32_t* tail_host, const int32_t* changes,
                        int32_t seq, int32_t* col, int32_t* rev, int32_t* pid, float* disp, float* geo, int32_t* xg, void* stream);
/* edge_index [2][n_edges] int64 (RadiusGraph's API array, representations.py:98-100) from the CSR list: row 0 = the receiver of
 * each edge, row 1 = col.  n_edges_dev (optional): the count is read on the device, n_edges is then the capacity of the grid. */
int nnhip_edge_index_from_csr(const int32_t* row_ptr, const int32_t* col, int32_t n_atoms, int32_t n_edges,
                              int64_t* edge_index, const int32_t* n_edges_dev, void* stream);

/* The whole deferred step in ONE call (what NewtonNet.forward issues in its steady state: the ~8 host calls of the pieces above
 * cost a small molecule more than its kernels): nnhip_prepare_check_counter, the neighbor list (nnhip_graph_count_pairs_z +
 * nnhip_graph_finish_dev, or nnhip_graph_small_dev for small systems) whose last kernel stores (edge count, status, change counter,
 * seq) into tail_host[4] (pinned host memory; the caller polls tail_host[3] for its seq, or waits on the optional `event`), and
 * nnhip_energy_forces_dev.  Everything per-step lives in caller-allocated arenas laid out by nnhip_step_layout. */
typedef struct {
  size_t i32_count, f32_count;   /* elements of the two arenas (int32 / float32, both 256-byte aligned by the caller) */
  /* int32 arena */
  size_t mol_ptr, row_ptr, status, pair_ptr, pair_scan, tail /* 2 ints */, mol_scratch /* 2 n_mol + n_mol / 1024 + 4 ints */, xg, col, rev, pid;
  /* float32 arena: edge geometry, then the small outputs */
  size_t geo, disp, energy, forces, virial, atom_energy;
} nnhip_step_layout;
int nnhip_step_layout_of(int32_t n_atoms, int32_t n_mol, int32_t capacity, nnhip_step_layout* out);
typedef struct {
  const int64_t* z;        /* [N] */
  const float* pos;        /* [N][3] */
  const float* cell;       /* [B][3][3] */
  const int64_t* batch;    /* [N] */
  int32_t n_atoms, n_mol, capacity /* even, > 0 */, want_forces, want_virial;
  int32_t seq;             /* the caller's sequence number of this step: stored into tail_host[3] AFTER the three words */
  int32_t flags, pad_;     /* bit 0: every molecule of the batch is expected to have at most NNHIP_MOL_STAGE_MAX atoms (the status
                              word of the previous batch of this shape had bit 8 clear): the molecule-resident edge kernels may run */
  int32_t* i32;            /* arena of nnhip_step_layout.i32_count ints */
  float* f32;              /* arena of nnhip_step_layout.f32_count floats */
  int64_t* edge_index;     /* [2 * capacity] or NULL (what newtonnet_amd/hip.py passes: it calls nnhip_edge_index_from_csr when a
                              caller asks for the array); rows at stride = the TRUE edge count */
  float* atom_node;        /* [N][F] */
  float* force_node;       /* [N][3][F] */
  void* workspace;         /* nnhip_workspace_bytes(N, capacity, B, L) */
  size_t workspace_bytes;
  void* prepared;          /* nnhip_prepared_bytes(L), filled by nnhip_prepare */
  size_t prepared_bytes;
  int32_t* tail_host;      /* pinned host memory, 4 ints: (edge count, status, change counter of the prepared block: non-zero =
                              a parameter changed since nnhip_prepare, seq) -- written by a kernel's own stores (zero-copy), seq
                              last with release semantics: a host that reads tail_host[3] == seq may read the other three */
  void* event;             /* optional hipEvent_t recorded behind that kernel (NULL: none -- a record is a marker packet in the
                              stream, ~6 us of bubble per step; NewtonNet.forward polls tail_host[3] instead) */
} nnhip_step_dev;
int nnhip_forward_dev(const nnhip_model* model, const nnhip_step_dev* step, void* stream);

/* nnhip_energy_forces for a caller that kept pair_ptr[n_atoms + 1] (the scan of the per-row pair counts): the row kernels then
 * find the split of a row into "pairs the other endpoint owns | pairs this row owns" with two scalar loads instead of a ballot
 * over its cols.  Same results.  flags bit 0: no molecule of the batch has more than NNHIP_MOL_STAGE_MAX atoms (bit 8 of the
 * status word nnhip_graph_count* left is clear): large batches then run force_fwd one workgroup per molecule with the molecule's
 * node rows staged in LDS (edge.hip:force_fwd_mol_kernel; same sums in a different order than the row form, ~1e-7 relative). */
int nnhip_energy_forces_pp(const nnhip_model* model, const int64_t* z, const float* pos, const float* cell,
                           const int32_t* mol_ptr,
                           const int32_t* row_ptr, const int32_t* col, const int32_t* rev, const int32_t* pid, const float* geo,
                           const int32_t* xg, const float* disp, int32_t n_atoms, int32_t n_edges,
                           int32_t n_mol, void* workspace, size_t workspace_bytes, float* energy, float* forces,
                           float* virial, float* atom_energy, float* atom_node, float* force_node,
                           const void* prepared, const int32_t* pair_ptr, int32_t flags, void* stream);

/* Parameter-only preparation (transposed weights for the reverse sweep, radial-filter tables, layer 0's
 * message_nodepart per element): what the reference gets for free from nn.Module state.  `prepared` is a caller-owned
 * 256-byte-aligned block of nnhip_prepared_bytes(n_layers); fill it with nnhip_prepare whenever the parameters may have
 * changed (the Python mirror does it on every forward, on the stream, while the host waits for the edge count) and pass it
 * to nnhip_energy_forces.  prepared == NULL: nnhip_energy_forces rebuilds the block inside its workspace on every call. */
size_t nnhip_prepared_bytes(int32_t n_layers);
int nnhip_prepare(const nnhip_model* model, void* prepared, size_t prepared_bytes, void* stream);
/* Has any parameter changed since `prepared` was last FILLED?  One launch: every parameter tensor of `model` is compared bit for
 * bit with the snapshot nnhip_prepare took when it filled the block, and `bit` is OR-ed into *status (device int32) when
 * something differs.  Compare only: the snapshot moves in nnhip_prepare alone, so a change stays visible until the block has
 * really been refilled (a caller that fails between the check and the refill cannot lose it).  A caller that keeps one block
 * per model runs this every call and calls nnhip_prepare only when the bit comes back set.  Replaces nothing in the
 * reference: torch modules keep no derived state. */
int nnhip_prepare_check(const nnhip_model* model, void* prepared, size_t prepared_bytes, int32_t* status, int32_t bit,
                        void* stream);
/* The same comparison reporting through an int32 counter INSIDE the block: zero after nnhip_prepare, one or more up for every
 * check that finds a difference (so it stays non-zero until the block is refilled).  Nothing of the caller's has to be
 * initialised for it.  *counter (optional) receives the counter's device address: the deferred step hands the value to the host
 * next to the edge count (nnhip_graph_finish_dev / nnhip_graph_small_dev, `changes`). */
int nnhip_prepare_check_counter(const nnhip_model* model, void* prepared, size_t prepared_bytes, const int32_t** counter,
                                void* stream);

/* --------------------------------------------------------------------------
 * One dense 128 -> 128 linear on the matrix cores (fp32 MFMA, exact fp32):
 *   C[M][128] = epilogue( prologue(A)[M][128] . W^T ),   W = [128 out][128 in] (nn.Linear layout)
 * Replaces: torch.nn.functional.linear for the F x F layers of the path
 *   (message_nodepart newtonnet.py:181-185, equiv_message1/2 :188-197, equiv_update :199,
 *   EnergyOutput.layers output.py:90-95) and the x W products of their adjoints (pass W^T).
 * prologue: 0 none, 1 A <- silu(A).   epilogue: 0 store, 1 + bias[n], 2 * silu'(H[m][n]), 3 C += result.
 * lda/ldc/ldh are row strides in floats (>= 128).  C may alias A only exactly (same pointer, ldc == lda).
 * ------------------------------------------------------------------------ */
int nnhip_linear128(const float* A, int32_t lda, const float* W, float* C, int32_t ldc, const float* bias,
                    const float* H, int32_t ldh, int32_t M, int32_t prologue, int32_t epilogue, void* stream);

/* --------------------------------------------------------------------------
 * Fused two-layer edge MLP (Linear -> SiLU -> Linear, no bias) and its adjoint; the hidden tile stays in registers.
 * Replaces: equiv_message1 / equiv_message2 (newtonnet.py:188-197, called at :218,:222) -- ~87 % of the FLOPs.
 *   mode 0 (forward):  H = X W1^T (written: the adjoint needs it),  Y = silu(H) W2^T
 *   mode 1 (adjoint):  G = (X W1^T) * silu'(H) (H read),            Y = G W2^T   (accumulate != 0: Y += ...)
 *                      call with X = g_phi, W1 = V2^T, W2 = V1^T to get Y = g_msg.
 * W1, W2: [128][128] row-major.  ldx / ldh / ldy: row strides in floats (>= 128, multiples of 4).
 * ------------------------------------------------------------------------ */
int nnhip_mlp128(const float* X, int32_t ldx, const float* W1, const float* W2, float* H, int32_t ldh, float* Y,
                 int32_t ldy, int32_t M, int32_t mode, int32_t accumulate, void* stream);

/* --------------------------------------------------------------------------
 * direct_force head.
 * Replaces: DirectForceOutput.forward (newtonnet/models/output.py:115-132) + ScaleShift (scalers.py:55-56):
 *   d = Linear(silu(Linear(silu(Linear(atom_node)))));  out[i][k] = scale[z_i] * < d[i], force_node[i][k] >
 * w0/w2/w4: output_layers.k.layers.{0,2,4}.weight [F][F], b0/b2/b4 biases [F]; scale: scalers.k.scale.weight [119]
 * (NULL = 1).  atom_node [N][F] and force_node [N][3][F] are the outputs of nnhip_energy_forces.
 * scratch: 3 * n_atoms * F floats.
 * ------------------------------------------------------------------------ */
int nnhip_direct_force(const float* atom_node, const float* force_node, const int64_t* z, const float* w0, const float* b0,
                       const float* w2, const float* b2, const float* w4, const float* b4, const float* scale,
                       int32_t activation, int32_t n_atoms, float* scratch, float* out, void* stream);

/* --------------------------------------------------------------------------
 * Differentiable building blocks of the train-mode forward (both are linear maps and each other's adjoints, so
 * torch.autograd can differentiate through them twice: force-loss training, output.py:66-73 + trainer.py:307-309).
 * Replaces: torch_geometric.utils.scatter(..., reduce='sum') (newtonnet.py:214,226; output.py:246) and the
 *   index gathers m[edge_index[k]], force_node[edge_index[1]] (newtonnet.py:211,223).
 *   segment_sum: out[i][:] = sum_{e in [row_ptr[i], row_ptr[i+1])} x[e][:]   (CSR rows; deterministic, no atomics)
 *   gather_rows: out[e][:] = x[idx[e]][:]
 * width = floats per row (even).
 * ------------------------------------------------------------------------ */
int nnhip_segment_sum(const float* x, const int32_t* row_ptr, int32_t n_rows, int32_t width, float* out, void* stream);
int nnhip_gather_rows(const float* x, const int32_t* idx, int32_t n_out, int32_t width, float* out, void* stream);

/* ==========================================================================
 * Per-stage entry points (last row) and TRAINING.
 *
 * The stages nnhip_energy_forces runs internally, exported one by one, plus the kernels that differentiate them
 * once more.  Training (newtonnet/train/trainer.py:299-313: loss.backward() through the autograd force of
 * newtonnet/models/output.py:66-73, create_graph=True) is evaluated as "tangent over reverse": with c_b = dL/dE_b and
 * d = dL/dF,   dL/dtheta = sum_b c_b dE_b/dtheta - D_d[grad_theta E_tot],   i.e. the reverse sweep is differentiated in
 * forward (tangent) mode along v = -d with the reverse seed carried as the dual number 1 + eps c_b.  Every stage below has a
 * value form (*_fwd / *_bwd = its adjoint) and a tangent form (*_tan_fwd / *_tan_bwd); all are deterministic (segmented
 * sums over the receiver CSR, pair rows written by the lower endpoint, no float atomics).  The host side that strings
 * them together is newtonnet_amd/train_fused.py; tests/tangent_ref.py states the same sweeps in fp64.
 * Shapes: N atoms, E directed edges, P = E/2 pairs (row pid[e]); node rows [N][F], [N][3][F]; pair rows [P][F].
 * ========================================================================== */

/* atom_node = Embedding[z]  (newtonnet.py:142) */
int nnhip_embed(const int64_t* z, const float* table, int32_t n_atoms, float* out, void* stream);

/* Radial-filter tables of `n_layers` layers (message_edgepart applied to the Bessel basis, newtonnet.py:186,210): for each
 * layer three planes of FT_ROWS rows of F floats over the nodes x_g = g / FT_G (FT_G = 3072 intervals of x = r/cutoff; row =
 * g + 1) -- value, secant slope to the next node (differenced in fp64), d/dx; tables[l] needs nnhip_filter_table_bytes() bytes.
 * The message kernels interpolate (value: 4-point Lagrange on the value plane; value and derivative: cubic Hermite from four
 * rows) instead of contracting rbf per edge. */
size_t nnhip_filter_table_bytes(void);
int nnhip_filter_tables(const float* const* edge_w_host_array, float* const* tables_host_array, int32_t n_layers,
                        const float* frequencies, int32_t n_basis, int32_t envelope, void* stream);

/* out[k] = in[k]^T for `count` <= 40 [128][128] matrices (weights for the adjoint products) */
int nnhip_transpose128(const float* const* src_host_array, float* const* dst_host_array, int32_t count, void* stream);

/* K1: message + invariant aggregation (newtonnet.py:210-215) and its adjoint.
 *   fwd: msg[p] = eps(x_e) m_i m_j;  a_mid[i] = a_in[i] + sum_{e in row i} msg
 *   bwd: G = g_msg[p] + g_a[i] + g_a[j];  g_m[i] = sum_e G eps m_j;  g_x[e] = <G m_i m_j, d eps/dx> (pair owner's edge) */
int nnhip_message_fwd(const float* m, const int32_t* xg, const float* table, const int32_t* row_ptr, const int32_t* col,
                      const int32_t* pid, const float* a_in, float* msg, float* a_mid, int32_t n_atoms, void* stream);
int nnhip_message_bwd(const float* g_msg, const float* g_a, const float* m, const int32_t* xg, const float* table,
                      const int32_t* row_ptr, const int32_t* col, const int32_t* pid, float* g_m, float* g_x,
                      int32_t n_atoms, int32_t need_gm, void* stream);

/* K2: equivariant messages + aggregation (newtonnet.py:219-227) and its adjoint.  f_in NULL = first layer (force_node == 0).
 *   fwd: f_out[i][k] = f_in[i][k] + sum_e phi1[p] u_e[k] + phi2[p] f_in[j][k]
 *   bwd: g_h12[p] = (g_phi1 | g_phi2) (both directions summed), g_u[e][k] = <gf_i[k], phi1[p]>,
 *        g_fin[i][k] = gf[i][k] + sum_e phi2[p] gf[j][k] */
int nnhip_force_message_fwd(const float* phi1, const float* phi2, const float* geo, const int32_t* xg,
                            const int32_t* row_ptr, const int32_t* col, const int32_t* pid, const float* f_in,
                            float* f_out, int32_t n_atoms, void* stream);
int nnhip_force_message_bwd(const float* gf, const float* phi1, const float* phi2, const float* geo, const int32_t* xg,
                            const int32_t* row_ptr, const int32_t* col, const int32_t* pid, const float* f_in,
                            float* g_h12, float* g_u, float* g_fin, int32_t n_atoms, void* stream);

/* Adjoint of the edge embedding: g_x[L][E], g_u[L][E][4] of all layers -> g_d[E][4] -> forces[N][3] (= -dE/dpos) and,
 * optionally, virial[B][3][3] (output.py:154-165; needs disp / pos / cell / mol_ptr). */
int nnhip_edge_embed_bwd(const float* g_x, const float* g_u, const float* geo, const float* disp, const float* pos,
                         const float* cell, const int32_t* row_ptr, const int32_t* col, const int32_t* rev,
                         const int32_t* mol_ptr, int32_t n_atoms, int32_t n_edges, int32_t n_mol, int32_t n_layers,
                         float cutoff, float* g_d, float* forces, float* virial, void* stream);

/* Row-local node stages between two edge phases (newtonnet.py:229-231 and, for the next layer, :181-185,209).
 *   node_fwd: q_k = f_k Wu^T; a_out = a_mid + sum_k f_k q_k; [hn = a_out W0^T + b0; m = act(hn) W2^T + b2 when W0 != NULL]
 *   node_bwd: [g_hn = (g_top W2T^T) act'(h_top); g_a (+)= g_hn W0T^T when W2T != NULL];
 *             [gf_k = G_f,k + g_a q_k + (g_a f_k) WuT^T when WuT != NULL]     (W*T = transposed weights) */
int nnhip_node_fwd(const float* f, const float* a_mid, const float* Wu, float* q, float* a_out, const float* W0,
                   const float* b0, const float* W2, const float* b2, float* hn, float* m, int32_t n_atoms,
                   int32_t activation, void* stream);
int nnhip_node_bwd(const float* g_top, const float* h_top, const float* W2T, const float* W0T, float* g_a,
                   int32_t accumulate_ga, const float* f, const float* q, const float* G_f, const float* WuT, float* gf,
                   int32_t n_atoms, int32_t activation, void* stream);

/* The same two stages, their fused turn-around and their tangent forms in every form the pipelines launch.
 *   nnhip_node_images   split-f16 images (nnhip_weight_images) of Wu, W0, W2 and of their transposes; NULL member = absent.
 *   images == NULL      (node_fwd_ex / node_bwd_ex only) the fp32 kernels, any activation: what nnhip_node_fwd / _bwd run.
 *   images != NULL      the split-f16 kernels: SiLU only; the products read the IMAGES, and the fp32 weight pointers only say which
 *                       part runs (W0: next message_nodepart / head; W2T: MLP adjoint; WuT: update adjoint) and may be any non-NULL.
 *   node_bwd_ex         T [N][F] (may be NULL, images only): receives t = g_top W2 before the act' factor; g_a_in (may be NULL, images
 *                       only): with accumulate_ga the running g_a is read from it instead of from g_a.  q == NULL with WuT: q is
 *                       formed again from f and images->Wu (refused without that image).
 *   node_turn           node_fwd into the head, the head tail ( atom_energy = (<silu(e2), w4> + b4) scale[z] + shift[z],
 *                       g_e2 = scale w4 silu'(e2) ), the head adjoint and the update adjoint with G_f = 0, in one launch; all six
 *                       images; scale / shift may be NULL (1 / 0).  Outputs a_out, atom_energy [N], g_a, gf: the bits of
 *                       nnhip_node_fwd_ex -> nnhip_head_out -> nnhip_node_bwd_ex.
 *   node_tan_fwd        dq_k = df_k Wu^T; da_out = da_mid + sum_k (df_k q_k + f_k dq_k); T = da_out W0^T; Y = (T silu'(hn)) W2^T
 *   node_tan_bwd        part A (g_top != NULL): dT = g_top W2; G = dT silu'(h_top) + t2_top silu''(h_top) hd_top (t2 / hd NULL = 0);
 *                       dga (+)= G W0.  Part B (f != NULL): gq_k = ga f_k; dgq_k = dga f_k + ga df_k;
 *                       dgf_k = dgf_in,k + dga q_k + ga dq_k + dgq_k Wu  (dgf_in may be NULL).  Without part A dga is an input.
 * Every entry point refuses (NNHIP_E_INVALID, nothing launched) a negative n_atoms, an activation out of range, a missing image or
 * pointer of the chosen form; n_atoms == 0 returns NNHIP_OK. */
typedef struct {
  const void* Wu; const void* W0; const void* W2;
  const void* W2T; const void* W0T; const void* WuT;
} nnhip_node_images;
int nnhip_node_fwd_ex(const float* f, const float* a_mid, const float* Wu, float* q, float* a_out, const float* W0,
                      const float* b0, const float* W2, const float* b2, float* hn, float* m, int32_t n_atoms,
                      int32_t activation, const nnhip_node_images* images, void* stream);
int nnhip_node_bwd_ex(const float* g_top, const float* h_top, const float* W2T, const float* W0T, float* g_a,
                      int32_t accumulate_ga, const float* f, const float* q, const float* G_f, const float* WuT, float* gf,
                      float* T, const float* g_a_in, int32_t n_atoms, int32_t activation, const nnhip_node_images* images,
                      void* stream);
int nnhip_node_turn(const float* f, const float* a_mid, float* a_out, const float* b0, const float* b2, const float* w4,
                    const float* b4, const float* scale, const float* shift, const int64_t* z, float* atom_energy, float* g_a,
                    float* gf, int32_t n_atoms, const nnhip_node_images* images, void* stream);
int nnhip_node_tan_fwd(const float* df, const float* f, const float* q, const float* da_mid, const float* hn, float* dq,
                       float* da_out, float* T, float* Y, int32_t n_atoms, const nnhip_node_images* images, void* stream);
int nnhip_node_tan_bwd(const float* g_top, const float* h_top, const float* t2_top, const float* hd_top, float* G, float* dga,
                       int32_t accumulate_dga, const float* ga, const float* f, const float* df, const float* q, const float* dq,
                       const float* dgf_in, float* gq, float* dgq, float* dgf, int32_t n_atoms, const nnhip_node_images* images,
                       void* stream);

/* LayerNorm over the F features of atom_node (eps 1e-5), one wave per row, and its adjoint and tangents:
 *   fwd      in place: xhat = (x - mean) rstd, rstd = 1 / sqrt(var + eps) ([N]); a = xhat gamma + beta
 *   bwd      in place: g_a = rstd (g' - mean(g') - xhat mean(g' xhat)),  g' = g_a gamma
 *   tan_fwd  in place: s = mean(xhat dx); dxhat = rstd (dx - mean(dx) - xhat s); drstd = -rstd^2 s ([N]); da = gamma dxhat
 *   tan_bwd  in place on dga (in dg_y, out dg_x = drstd A + rstd dA, A as in bwd, dA its tangent); row_w = dg_y xhat + g_y dxhat;
 *            row_b = dg_y  (the rows whose column sums are the tangent parts of dL/dgamma, dL/dbeta) */
int nnhip_layer_norm_fwd(float* a, const float* gamma, const float* beta, int32_t n_atoms, float* xhat, float* rstd, void* stream);
int nnhip_layer_norm_bwd(float* g_a, const float* gamma, const float* xhat, const float* rstd, int32_t n_atoms, void* stream);
int nnhip_layer_norm_tan_fwd(float* da, const float* xhat, const float* rstd, const float* gamma, int32_t n_atoms, float* dxhat,
                             float* drstd, void* stream);
int nnhip_layer_norm_tan_bwd(const float* gy, float* dga, const float* xhat, const float* rstd, const float* dxhat,
                             const float* drstd, const float* gamma, int32_t n_atoms, float* row_w, float* row_b, void* stream);

/* Energy head tail (output.py:98-100 last linear, scalers.py:55-58, output.py:246) and the reverse seed:
 *   atom_energy[i] = (<act(e2_i), w4> + b4) scale[z_i] + shift[z_i];  energy[b] = sum;  g_e2[i] = scale w4 act'(e2)  (may be NULL) */
int nnhip_head_out(const float* e2, const float* w4, const float* b4, const float* scale, const float* shift,
                   const int64_t* z, const int32_t* mol_ptr, int32_t n_atoms, int32_t n_mol, int32_t activation,
                   float* atom_energy, float* g_e2, float* energy, void* stream);

/* The same stages with what nnhip_energy_forces hands its launchers besides the arrays above, so that every kernel form the
 * pipeline runs can be called (and tested) on its own.  A NULL member / zero means "as the plain entry point":
 *   pair_ptr [N + 1]  exclusive scan of the number of pairs a row owns (its upper edges, the last ones of the row): the rows
 *                     take their split from it instead of a ballot over col
 *   rev [E]           reverse edge: force_message_bwd then lets the pair's owner write g_u of both directions
 *   mol_ptr [n_mol+1] molecule offsets: batches that pay (edge_kernels_from_molecules <= n_mol, 8 n_mol <= N <=
 *                     NNHIP_MOL_STAGE_MAX n_mol, see nnhip_config "molecule_forms") take the molecule-resident kernels of
 *                     message_bwd and force_message_fwd; no edge may join two molecules
 *   small_molecules   edge_embed_bwd / head_out: the batch may take their molecule-resident kernels (mol_ptr / n_mol are
 *                     arguments of those two entry points).  nnhip_edge_embed_bwd_ex refuses g_d == NULL where g_d is written:
 *                     with a virial, and with more than 2^20 edges
 *   tail_*            message_bwd with need_gm = 0 only: the molecule-resident kernel goes on with the geometry adjoint and writes
 *                     tail_forces [N][3] from g_x (the head of a [tail_n_layers][tail_n_edges] array whose first row this
 *                     launch writes), tail_g_u [L][E][4], tail_geo and rev, as nnhip_edge_embed_bwd would have.  *tail_done
 *                     says whether it did (1) or the forces are still to be formed (0: another form served the launch). */
typedef struct {
  const int32_t* pair_ptr; const int32_t* rev; const int32_t* mol_ptr;
  int32_t n_mol, small_molecules;
  const float* tail_g_u; const float* tail_geo; float* tail_forces;
  int32_t tail_n_edges, tail_n_layers;
  float tail_cutoff; int32_t pad_;
} nnhip_stage_opts;
int nnhip_message_bwd_ex(const float* g_msg, const float* g_a, const float* m, const int32_t* xg, const float* table,
                         const int32_t* row_ptr, const int32_t* col, const int32_t* pid, float* g_m, float* g_x,
                         int32_t n_atoms, int32_t need_gm, const nnhip_stage_opts* opts, int32_t* tail_done, void* stream);
int nnhip_force_message_fwd_ex(const float* phi1, const float* phi2, const float* geo, const int32_t* xg,
                               const int32_t* row_ptr, const int32_t* col, const int32_t* pid, const float* f_in,
                               float* f_out, int32_t n_atoms, const nnhip_stage_opts* opts, void* stream);
int nnhip_force_message_bwd_ex(const float* gf, const float* phi1, const float* phi2, const float* geo, const int32_t* xg,
                               const int32_t* row_ptr, const int32_t* col, const int32_t* pid, const float* f_in,
                               float* g_h12, float* g_u, float* g_fin, int32_t n_atoms, const nnhip_stage_opts* opts,
                               void* stream);
int nnhip_edge_embed_bwd_ex(const float* g_x, const float* g_u, const float* geo, const float* disp, const float* pos,
                            const float* cell, const int32_t* row_ptr, const int32_t* col, const int32_t* rev,
                            const int32_t* mol_ptr, int32_t n_atoms, int32_t n_edges, int32_t n_mol, int32_t n_layers,
                            float cutoff, float* g_d, float* forces, float* virial, const nnhip_stage_opts* opts,
                            void* stream);
int nnhip_head_out_ex(const float* e2, const float* w4, const float* b4, const float* scale, const float* shift,
                      const int64_t* z, const int32_t* mol_ptr, int32_t n_atoms, int32_t n_mol, int32_t activation,
                      float* atom_energy, float* g_e2, float* energy, const nnhip_stage_opts* opts, void* stream);

/* Fused Linear -> act -> Linear with every option (nnhip_mlp128 is the plain subset):
 *   mode 0 FWD : H = X W1^T + b1 (stored);  Y = act(H) W2^T + b2
 *   mode 1 BWD : T = X W1^T;  Y (+)= (T act'(H)) W2^T
 *   mode 2 TAN : as BWD, and T is stored            -- tangent of FWD (X = dX: T = dH, Y = dY), or BWD keeping its hidden product
 *   mode 3 TAN2: dT = X W1^T;  G = dT act'(H) + T2 act''(H) Hd (stored);  Y (+)= G W2^T      -- tangent of BWD
 * H / T / T2 / Hd / G share the row pitch ldh. */
typedef struct {
  const float* X; int32_t ldx;
  const float* W1; const float* W2; const float* b1; const float* b2;
  float* H; int32_t ldh;
  float* Y; int32_t ldy;
  int32_t M, mode, accumulate, activation;
  float* T; const float* T2; const float* Hd; float* G;
  /* optional: split-f16 images of W1 / W2 (nnhip_weight_images; both or neither).  With them the row-local form of the kernel
   * (M <= 49 152 rows) takes the split-f16 product form instead of v_mfma_f32_32x32x2_f32; results agree to fp32 rounding. */
  const void* W1_image; const void* W2_image;
  /* 0: fp32-grade products (the default).  1: the bf16 compute mode of training under torch.autocast(bfloat16) (BASELINE configs[2];
   * the reference has no bf16, newtonnet/layers/precision.py:3-13): both operands of every product rounded to bf16, ONE
   * v_mfma_f32_32x32x16_bf16 per 16 k-values instead of three f16 ones, fp32 accumulation, fp32 inputs / outputs; bias-free SiLU
   * MLPs whose images were written by nnhip_weight_images_bf16. */
  int32_t precision; int32_t pad_;
} nnhip_mlp_desc;
int nnhip_mlp128_ex(const nnhip_mlp_desc* desc, void* stream);
/* Split-f16 image of a [128][128] fp32 matrix (rows = output features): two f16 planes (hi, lo) of the matrix scaled by a power
 * of two into the f16 range and stored fragment by fragment (1 KiB per (output block, MFMA step), lane-linear: the image is opaque to
 * the caller), then the inverse scale (csrc/node128s.hip).  `count` matrices in
 * one launch; each image takes nnhip_weight_image_bytes() bytes, 256-byte aligned. */
size_t nnhip_weight_image_bytes(void);
int nnhip_weight_images(const float* const* src, void* const* images, int32_t count, void* stream);
/* the same images in the bf16 format (first plane = the matrix rounded to bf16, unscaled; a format word behind the inverse scale tells
 * the kernels which form an image has): operands of nnhip_mlp_desc.precision = 1 */
int nnhip_weight_images_bf16(const float* const* src, void* const* images, int32_t count, void* stream);
/* how many nnhip_mlp128_ex / nnhip_mlp128_pair_ex calls have taken the bf16 compute mode since the library was loaded */
int64_t nnhip_bf16_mlp_launches(void);
/* two MLPs over the same M rows in one launch (same mode / activation; only the second may accumulate) */
int nnhip_mlp128_pair_ex(const nnhip_mlp_desc* desc0, const nnhip_mlp_desc* desc1, void* stream);

/* ---- tangent kernels (sweeps 3 and 4) ---- */
/* tgeo[e] = (du_e, dx_e): tangent of (dir, x = r/cutoff) along the position direction sign * v[N][3]
 * (training passes v = dL/dF with sign = -1) */
int nnhip_edge_tangent_geom(const float* v, float sign, const int64_t* edge_index, const float* geo, int32_t n_edges,
                            float cutoff, float* tgeo, void* stream);
/* dmsg[p] = deps dx m_i m_j + eps (dm_i m_j + m_i dm_j);  da_mid = da_in + sum_e dmsg   (dm = da_in = NULL: first layer) */
int nnhip_message_tan_fwd(const float* m, const float* dm, const int32_t* xg, const float* tgeo, const float* table,
                          const int32_t* row_ptr, const int32_t* col, const int32_t* pid, const float* da_in, float* dmsg,
                          float* da_mid, int32_t n_atoms, void* stream);
/* df_out = df_in + sum_e dphi1 u + phi1 du + dphi2 f_j + phi2 df_j   (f_in = df_in = NULL: first layer) */
int nnhip_force_message_tan_fwd(const float* phi1, const float* dphi1, const float* phi2, const float* dphi2,
                                const float* geo, const float* tgeo, const int32_t* xg, const int32_t* row_ptr,
                                const int32_t* col, const int32_t* pid, const float* f_in, const float* df_in,
                                float* df_out, int32_t n_atoms, void* stream);
/* dg_h12[p] = (dg_phi1 | dg_phi2),  dg_fin = dgf + sum_e dphi2 gf_j + phi2 dgf_j */
int nnhip_force_message_tan_bwd(const float* gf, const float* dgf, const float* phi2, const float* dphi2, const float* geo,
                                const float* tgeo, const int32_t* xg, const int32_t* row_ptr, const int32_t* col,
                                const int32_t* pid, const float* f_in, const float* df_in, float* dg_h12, float* dg_fin,
                                int32_t n_atoms, void* stream);
/* dg_m[i] = sum_e dG eps m_j + G deps dx m_j + G eps dm_j;  g_eps[p] = G m_i m_j;  dg_eps[p] = dG m_i m_j + G (dm_i m_j + m_i dm_j) */
int nnhip_message_tan_bwd(const float* g_msg, const float* dg_msg, const float* ga, const float* dga, const float* m,
                          const float* dm, const int32_t* xg, const float* tgeo, const float* table,
                          const int32_t* row_ptr, const int32_t* col, const int32_t* pid, float* dg_m, float* g_eps,
                          float* dg_eps, int32_t n_atoms, void* stream);
/* da_out = da_mid + sum_k df_k q_k + f_k dq_k */
int nnhip_update_tan_fwd(const float* da_mid, const float* f, const float* df, const float* q, const float* dq,
                         int32_t n_atoms, float* da_out, void* stream);
/* gq_k = GA f_k;  dgq_k = dGA f_k + GA df_k;  dgf_k = dgf_in,k + dGA q_k + GA dq_k   (the W_u product follows as a linear) */
int nnhip_update_tan_bwd(const float* ga, const float* dga, const float* f, const float* df, const float* q,
                         const float* dq, const float* dgf_in, int32_t n_atoms, float* gq, float* dgq, float* dgf,
                         void* stream);
/* seed of the tangent reverse sweep at the energy head, see csrc/train.hip:head_seed_tan_kernel */
int nnhip_head_seed_tan(const float* e2, const float* de2, const float* w4, const float* b4, const float* scale,
                        const int64_t* z, const int64_t* batch, const float* g_energy, int32_t n_atoms, int32_t activation,
                        float* dg_e2, float* w4row, float* scal, void* stream);
/* rb[p][0:nb] = rbf_e, rb[p][32:32+nb] = drbf_e dx_e for the owner edge of pair p ([P][64], zero padded) */
int nnhip_pair_rbf(const float* rbf, const float* drbf, const float* tgeo, const int64_t* edge_index, const int32_t* pid,
                   int32_t n_edges, int32_t n_basis, float* rb, void* stream);
/* ---- the last stage of "tangent over reverse" (csrc/hessian.hip; the strain seed and sum: csrc/elastic.hip), as nnhip_hessian_vp,
 * nnhip_hessian_blocks and nnhip_strain_vp run them.  Each call checks its arguments before any launch (a refused call writes
 * nothing); a zero size is NNHIP_OK without a launch. ---- */
/* dg_u[e] = (< dgf[i][k], phi1[p] > + < gf[i][k], dphi1[p] >, 0) for every directed edge e of receiver i, p = pid[e]; zeros for a
 * masked candidate (xg[e].x == the table's zero row; xg NULL: nothing is masked) */
int nnhip_hvp_dgu(const float* gf, const float* dgf, const float* phi1, const float* dphi1, const int32_t* row_ptr,
                  const int32_t* pid, const int32_t* xg, int32_t n_atoms, float* dg_u, void* stream);
/* dg_x[e] = sum_f dg_eps[p][f] eps'_f(x) + g_eps[p][f] eps''_f(x) tgeo[e][3] on the owner edge (edge_index[0][e] < edge_index[1][e])
 * of an unmasked pair with x = geo[e][3] / cutoff < 1, else 0; eps_f = sum_n edge_w[f][n] env(x) sin(freq_n x) / x evaluated
 * analytically in fp64.  n_basis outside 1..NNHIP_MAX_NB: NNHIP_E_UNSUPPORTED. */
int nnhip_hvp_dgx(const int64_t* edge_index, const int32_t* pid, const float* geo, const float* tgeo, const int32_t* xg,
                  const float* g_eps, const float* dg_eps, const float* edge_w, const float* freq, int32_t n_basis, int32_t envelope,
                  float cutoff, int32_t n_edges, float* dg_x, void* stream);
/* dg_d[e] = the tangent of g_d = a u + g_u / r, a = g_x / cutoff - (g_u . u) / r (g_x [L][E], g_u [L][E][4] and their tangents summed
 * over the n_layers layers) along tgeo = (du, dx = dr / cutoff), fourth component 0;  hv[i] = sum_{e in row i} dg_d[e] - dg_d[rev e] */
int nnhip_hvp_out(const float* g_x, const float* g_u, const float* dg_x, const float* dg_u, const float* geo, const float* tgeo,
                  const int32_t* row_ptr, const int32_t* rev, int32_t n_atoms, int32_t n_edges, int32_t n_layers, float cutoff,
                  float* dg_d, float* hv, void* stream);
/* pass k of nnhip_hessian_blocks: v[i] = e_(dir % 3) where atom i is local atom dir / 3 of its molecule b and dir < 3 n_b, else 0,
 * dir = k n_rep + b / n_mol0;  blocks[blk_ptr[b % n_mol0] + (3 a + c) 3 n_b + dir] = hv[i][c] (nothing where dir >= 3 n_b) */
int nnhip_hess_dirs(const int64_t* batch, const int32_t* mol_ptr, int32_t n_atoms, int32_t k, int32_t n_rep, int32_t n_mol0, float* v,
                    void* stream);
int nnhip_hess_scatter(const float* hv, const int64_t* batch, const int32_t* mol_ptr, const int64_t* blk_ptr, int32_t n_atoms,
                       int32_t k, int32_t n_rep, int32_t n_mol0, float* blocks, void* stream);
/* the seed of nnhip_strain_vp: tgeo[e] = (du, dx) of dd = eta (r u), eta = the strain eta6[batch[edge_index[0][e]]] as a matrix */
int nnhip_strain_tan_geom(const int64_t* edge_index, const int64_t* batch, const float* geo, const float* eta6, int32_t n_edges,
                          float cutoff, float* tgeo, void* stream);
/* d2[b][I] = sum_ab (d eps_ab / d e_I) S_ab, S_ab = sum_e dg_d[e]_a r_e u_e,b over the edges of system b's rows (fp64 sums) */
int nnhip_strain_born(const float* dg_d, const float* geo, const int32_t* row_ptr, const int32_t* mol_ptr, int32_t n_mol, float* d2,
                      void* stream);
/* Per-element sums of the first `width` (<= 128) columns of x[N][ldx], two deterministic passes through `scratch`
 * (nnhip_species_scratch_bytes(width)).  Up to two outputs, each a column range of the element table, and a plain total:
 *   out_k[zz][0:cols_k] (pitch ldo_k) = sum_{i: z_i = zz} x[i][c_k : c_k + cols_k];   total[0] = sum_i x[i][c_total]
 * (node_embedding / scale / shift gradients and dL/d b4). */
size_t nnhip_species_scratch_bytes(int32_t width);
int nnhip_species_sum(const float* x, int32_t ldx, int32_t width, const int64_t* z, int32_t n_atoms, float* scratch,
                      float* out0, int32_t c0, int32_t cols0, int32_t ldo0, float* out1, int32_t c1, int32_t cols1,
                      int32_t ldo1, float* total, int32_t c_total, void* stream);

/* Weight gradients dW[o][i] = sum_r A1[r][o] B1[r][i] + A2[r][o] B2[r][i] over M rows, batched; split-K on the fp32 matrix
 * cores with per-workgroup slabs and an ordered final sum.  type 0: operands as stored; 1: B1 = act(hB), B2 = act'(hB) dhB;
 * 2: A2 = A2 * act'(hA).  A2/B2 NULL: one product.  b_cols32: B rows are 32 wide (radial basis).  ld* = 0 means 128.
 * The problem table is DEVICE memory. */
typedef struct {
  const float* A1; const float* B1; const float* A2; const float* B2;
  const float* hA; const float* hB; const float* dhB;
  float* out;
  int32_t M, lda1, lda2, ldb1, ldb2, ldh, type, b_cols32, activation, ldo, ncols, pad_;
} nnhip_wgrad_problem;
size_t nnhip_wgrad_slab_bytes(int32_t n_problems, int32_t chunks);
/* bf16_operands: 0 = fp32 MFMA (v_mfma_f32_32x32x2_f32); 1 = operands rounded to bf16 after their fp32 prologue, fp32
 * accumulation (v_mfma_f32_32x32x16_bf16; torch.autocast(bfloat16)); 2 = fp32-GRADE products from three bf16 pieces per operand
 * (six MFMAs per 16 rows, 24 significant bits, no scaling: the default of fp32 training).
 * pair_rows: the row count of the problems whose M is negative (pair-level problems of a table built for a capacity: the
 * number of pairs changes from batch to batch, the table does not) */
int nnhip_wgrad_batch(const nnhip_wgrad_problem* problems_dev, int32_t n_problems, int32_t chunks, float* slabs,
                      int32_t bf16_operands, int32_t pair_rows, void* stream);
/* Training objective of the reference (newtonnet/train/loss.py:5-50 factory, :53-103 BaseLoss with nn.MSELoss / nn.L1Loss /
 * nn.HuberLoss(delta), mean reduction; scripts/config.yml:45-51) and its gradient:
 *   loss = w[0] sum l_E(E - E*) + w[1] sum l_F(F - F*);  g_energy = w[0] l_E'(E - E*);  g_forces = w[1] l_F'(F - F*)
 * weights_dev[2] = (w_E / n_E, w_F / n_F) lives in DEVICE memory (a data-parallel run refreshes the global counts there).
 * `forces` is whichever force the loss is on (gradient_force, or direct_force for DirectForceLoss, loss.py:41-47). */
enum { NNHIP_LOSS_MSE = 0, NNHIP_LOSS_MAE = 1, NNHIP_LOSS_HUBER = 2 };
int nnhip_loss_grad(const float* energy, const float* energy_label, int32_t n_energy, const float* forces,
                    const float* force_label, int32_t n_force, const float* weights_dev, int32_t mode_energy, int32_t mode_force,
                    float delta_energy, float delta_force, float* loss, float* g_energy, float* g_forces, void* stream);
/* the 'mse' / 'mse' case of nnhip_loss_grad */
int nnhip_mse_loss_grad(const float* energy, const float* energy_label, int32_t n_energy, const float* forces,
                        const float* force_label, int32_t n_force, const float* weights_dev, float* loss, float* g_energy,
                        float* g_forces, void* stream);
/* clip_grad_norm_(max_norm) + torch.optim.Adam step (trainer.py:311-313; no weight decay / amsgrad) on flat buffers of n
 * floats.  state[2] (device) = (step count, last gradient norm); scratch: nnhip_clip_adam_scratch_bytes().  max_norm <= 0:
 * no clipping.
 * nnhip_clip_adam_dev: the hyper-parameters (lr, beta1, beta2, eps, max_norm) are read from DEVICE memory at run time -- a
 * captured HIP graph then follows a learning-rate schedule (trainer.py:190,254: ReduceLROnPlateau on optimizer.param_groups) --
 * and mask_dev (n bytes, optional) marks frozen elements (0 = requires_grad False, newtonnet_train.py:69-81 freeze_*): they
 * stay out of the norm and are not updated. */
size_t nnhip_clip_adam_scratch_bytes(void);
int nnhip_clip_adam(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float* scratch,
                    float* state, float lr, float beta1, float beta2, float eps, float max_norm, void* stream);
int nnhip_clip_adam_dev(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float* scratch,
                        float* state, const float* hyper_dev, const uint8_t* mask_dev, void* stream);
/* out[c] = sum_r src[r][c] for [rows][128] arrays (bias gradients); device table */
typedef struct { const float* src; float* out; int32_t rows; int32_t pad_; } nnhip_colsum_problem;
size_t nnhip_colsum_scratch_bytes(int32_t n);
int nnhip_colsum_batch(const nnhip_colsum_problem* problems_dev, int32_t n, float* scratch, void* stream);

/* --------------------------------------------------------------------------
 * The two halves of a training step as single calls (what newtonnet_amd/train_fused.py:FusedEnergyForces runs in its forward
 * and backward): the stages above in order, on one stream, nothing else.  `ws` holds DEVICE pointers to every buffer of the
 * step (per-layer arrays indexed by layer; sizes as in the stage declarations; the host side owns and sizes them:
 * newtonnet_amd/train_fused.py:TrainWorkspace).  Replaces: the forward + torch.autograd.grad(create_graph=True) of
 * newtonnet/models/newtonnet.py:74-104 / output.py:66-73 (values), and loss.backward() through it, trainer.py:309 (grads).
 *   nnhip_train_values: parameter-only preparation (transposes, filter tables), forward sweep, reverse sweep -> energy[B],
 *                       forces[N][3], every intermediate kept in `ws`.
 *   nnhip_train_grads : given g_energy[B] = dL/dE and g_forces[N][3] = dL/dF: tangent forward, tangent reverse, the batched
 *                       weight-gradient / column-sum / per-element-sum launches; the parameter gradients land where the tables
 *                       (ws->probs, ws->sums) and the g_* pointers say.
 * ------------------------------------------------------------------------ */
typedef struct {
  int32_t n_atoms, n_edges, n_mol, n_layers, n_basis, envelope, bf16_wgrad;
  int32_t flags; /* bit 0: no molecule of the batch has more than NNHIP_MOL_STAGE_MAX atoms (bit 8 of the list's status word is
                    clear): with pair_ptr below, the value sweeps take the molecule-resident force_fwd / msg_bwd forms */
  /* batch + graph (nnhip_graph_* / nnhip_edge_embed outputs; rbf / drbf are required) */
  const int64_t* z; const float* pos; const float* cell; const int64_t* batch;
  const int32_t* mol_ptr; const int32_t* row_ptr; const int32_t* col; const int32_t* rev; const int32_t* pid;
  const int64_t* edge_index; const float* geo; const float* disp; const float* rbf; const float* drbf; const int32_t* xg;
  /* parameter-only data rebuilt by nnhip_train_values */
  float* wT[NNHIP_MAX_LAYERS][7]; float* headT[2]; float* ftab[NNHIP_MAX_LAYERS];
  /* split-f16 images (nnhip_weight_images) of, per layer: update, node0, node2, their transposes, eq1_0, eq1_2, eq2_0, eq2_2,
   * their transposes; of head0, head2 and their transposes */
  void* wimg[NNHIP_MAX_LAYERS][14]; void* himg[4];
  /* values, forward */
  float* a0; float* hn[NNHIP_MAX_LAYERS]; float* m[NNHIP_MAX_LAYERS]; float* msg[NNHIP_MAX_LAYERS];
  float* h1[NNHIP_MAX_LAYERS]; float* h2[NNHIP_MAX_LAYERS]; float* phi1[NNHIP_MAX_LAYERS]; float* phi2[NNHIP_MAX_LAYERS];
  float* a_mid[NNHIP_MAX_LAYERS]; float* a_out[NNHIP_MAX_LAYERS]; float* f_out[NNHIP_MAX_LAYERS]; float* q[NNHIP_MAX_LAYERS];
  float* e1; float* e2; float* g_e2; float* atom_energy; float* energy; float* forces;
  /* values, reverse */
  float* t_e1; float* GA[NNHIP_MAX_LAYERS]; float* gf[NNHIP_MAX_LAYERS]; float* Gf[2]; float* g_h12[NNHIP_MAX_LAYERS];
  float* t1[NNHIP_MAX_LAYERS]; float* t2[NNHIP_MAX_LAYERS]; float* g_msg[NNHIP_MAX_LAYERS]; float* g_m[NNHIP_MAX_LAYERS];
  float* t_n[NNHIP_MAX_LAYERS]; float* g_x; float* g_u; float* g_d;
  /* tangents, forward */
  float* tgeo; float* da_mid; float* da_out[NNHIP_MAX_LAYERS]; float* dhn[NNHIP_MAX_LAYERS]; float* dm[NNHIP_MAX_LAYERS];
  float* dmsg[NNHIP_MAX_LAYERS]; float* dh1[NNHIP_MAX_LAYERS]; float* dh2[NNHIP_MAX_LAYERS]; float* dphi1[NNHIP_MAX_LAYERS];
  float* dphi2[NNHIP_MAX_LAYERS]; float* df_out[NNHIP_MAX_LAYERS]; float* dq[NNHIP_MAX_LAYERS]; float* de1; float* de2;
  /* tangents, reverse */
  float* dg_e2; float* w4row; float* scal; float* dg_e1; float* dGA; float* dgf; float* dGf[2];
  float* gq[NNHIP_MAX_LAYERS]; float* dgq[NNHIP_MAX_LAYERS]; float* dg_h12[NNHIP_MAX_LAYERS]; float* dg_h1[NNHIP_MAX_LAYERS];
  float* dg_h2[NNHIP_MAX_LAYERS]; float* dg_msg; float* g_eps[NNHIP_MAX_LAYERS]; float* dg_eps[NNHIP_MAX_LAYERS];
  float* dg_m[NNHIP_MAX_LAYERS]; float* dg_hn[NNHIP_MAX_LAYERS]; float* rb; const float* zeros_nf;
  /* batched gradient launches and the outputs they do not cover */
  const nnhip_wgrad_problem* probs; const nnhip_colsum_problem* sums; float* slabs; float* cs_scratch; float* sp_scratch;
  int32_t n_probs, chunks, n_sums, pad2_;
  float* g_embedding; float* g_scale; float* g_shift; float* g_head4_b;
  /* layer_norm=True only (NULL otherwise): x_hat [N][F] and 1/sigma [N] of the value sweep, their tangents, the gradient at the
   * LayerNorm OUTPUT kept by the value reverse sweep, and the rows whose column sums are d gamma / d beta */
  float* ln_xhat[NNHIP_MAX_LAYERS]; float* ln_rstd[NNHIP_MAX_LAYERS]; float* ln_dxhat[NNHIP_MAX_LAYERS];
  float* ln_drstd[NNHIP_MAX_LAYERS]; float* ln_gy[NNHIP_MAX_LAYERS]; float* ln_row_w[NNHIP_MAX_LAYERS];
  float* ln_row_b[NNHIP_MAX_LAYERS];
  /* optional (NULL: the row kernels find a row's own pairs by a ballot): pair_ptr[N+1] of nnhip_graph_count_pairs -- the value sweeps
   * then run the forms the inference step runs (round 6) */
  const int32_t* pair_ptr;
} nnhip_train_ws;
size_t nnhip_train_ws_bytes(void); /* sizeof(nnhip_train_ws) of this build (bindings check their mirror against it) */
int nnhip_train_values(const nnhip_model* model, const nnhip_train_ws* ws, void* stream);
int nnhip_train_grads(const nnhip_model* model, const nnhip_train_ws* ws, const float* g_energy, const float* g_forces,
                      void* stream);
/* The same with adjoint seeds at the final node states: seed_a [N][F] = dL/d atom_node, seed_f [N][3][F] = dL/d force_node of
 * loss terms that read them directly (the direct_force head below; either may be NULL).  With g_forces = 0 and no seeds this is
 * plain back-propagation of an energy-only loss (output_properties ['energy'], trainer.py:299-313). */
int nnhip_train_grads_seeded(const nnhip_model* model, const nnhip_train_ws* ws, const float* g_energy, const float* g_forces,
                             const float* seed_a, const float* seed_f, void* stream);
/* First-order adjoint of the direct_force head (output.py:115-132, scalers.py:55-56; DirectForceLoss loss.py:41-47), given
 * g_out [N][3] = dL/d direct_force.  keep: the scratch of the forward nnhip_direct_force call, left untouched by the caller
 * ([3][N][F]: pre-activations of the first two linears, output of the third).  work
 * (nnhip_direct_force_bwd_work_floats(N) floats) receives g_d3 | g_pre2 | t1 | g_pre1 ([N][F] each, in this order): the rows of
 * the head's weight-gradient products  dW4 = g_d3^T act(pre2), dW2 = g_pre2^T act(pre1), dW0 = g_pre1^T atom_node  and of its
 * bias column sums, which the caller's nnhip_wgrad_batch / nnhip_colsum_batch tables reference.  seed_a / seed_f: outputs for
 * nnhip_train_grads_seeded.  g_scale [119] (NULL without a scale): gradient of scalers.k.scale.weight; sc4 [N][4] and
 * sp_scratch (nnhip_species_scratch_bytes(4)): scratch. */
size_t nnhip_direct_force_bwd_work_floats(int32_t n_atoms);
int nnhip_direct_force_bwd(const float* g_out, const float* force_node, const int64_t* z, const float* w0, const float* w2,
                           const float* w4, const float* scale, int32_t activation, int32_t n_atoms, const float* keep,
                           float* work, float* seed_a, float* seed_f, float* sc4, float* sp_scratch, float* g_scale,
                           void* stream);

/* --------------------------------------------------------------------------
 * Analytic Hessians of the energy with respect to the positions (cell fixed): HessianOutput, newtonnet/models/output.py:134-152
 * (H = d^2E/dpos^2 = -d gradient_force / dpos; MLAseCalculator 'hessian', utils/ase_interface.py:19,75-77).  Tangent over reverse:
 * sweeps 3-4 of the training step run along a position direction v with sign +1 and the reverse seed 1 + eps 0, plus three stages
 * the training step has no use for -- the tangents of g_u (force-message adjoint), of g_x (radial adjoint, second derivative of
 * the Bessel x envelope basis in fp64) and of the geometric adjoint -- and the force gather (csrc/hessian.hip).  No weight-gradient,
 * column-sum or per-element-sum launches; fp32-grade products (train_ws->bf16_wgrad must be 0); no float atomics.
 * Both calls need a prior nnhip_train_values on the same train_ws (the values and value adjoints of the batch).
 *   nnhip_hessian_vp    : hv[N][3] = H v for v[N][3] (device pointers; H is block-diagonal over the molecules).
 *   nnhip_hessian_blocks: ceil(n_dirs / n_rep) passes of the above with one-hot directions built on the device.  The batch of
 *                         train_ws is n_rep replicas of an original batch of n_mol0 molecules (molecule b = replica b / n_mol0 of
 *                         molecule b % n_mol0; n_rep = 1: the batch itself).  Pass k gives replica r the direction dir = k n_rep + r:
 *                         coordinate dir % 3 of local atom dir / 3 of every molecule (none where dir >= 3 n_b), and writes the
 *                         column H e_dir of each molecule into its packed block: blocks + blk_ptr[b] is [n_b][3][n_b][3],
 *                         blk_ptr[b] = sum_{b' < b} 9 n_b'^2 (int64, device).  n_dirs = 3 max n_b fills every block.
 * ------------------------------------------------------------------------ */
typedef struct {
  float* dg_x;            /* [L][E]     tangent of g_x (owner edges; 0 on the other direction) */
  float* dg_u;            /* [L][E][4]  tangent of g_u */
  float* dg_d;            /* [E][4]     tangent of the geometric adjoint g_d */
  float* v;               /* [N][3]     direction scratch of nnhip_hessian_blocks */
  float* hv;              /* [N][3]     column scratch of nnhip_hessian_blocks */
  const float* zeros_b;   /* [n_mol]    zeros: the tangent of the reverse seed */
  const int64_t* blk_ptr; /* [n_mol0]   block offsets (nnhip_hessian_blocks only) */
  int32_t n_rep, n_mol0;  /* replicas in the batch, molecules of the original batch (nnhip_hessian_blocks only) */
} nnhip_hvp_ws;
size_t nnhip_hvp_ws_bytes(void); /* sizeof(nnhip_hvp_ws) of this build */
int nnhip_hessian_vp(const nnhip_model* model, const nnhip_train_ws* train_ws, const nnhip_hvp_ws* hvp_ws, const float* v, float* hv,
                     void* stream);
int nnhip_hessian_blocks(const nnhip_model* model, const nnhip_train_ws* train_ws, const nnhip_hvp_ws* hvp_ws, int32_t n_dirs,
                         float* blocks, void* stream);

/* --------------------------------------------------------------------------
 * Batched normal-mode analysis on the packed Hessian blocks (csrc/eig.hip): what a user of HessianOutput does next with
 * numpy / LAPACK on the host, one molecule at a time.  One workgroup per molecule, ONE launch per batch, everything in LDS:
 *   A = (H + H^T)/2 mass-weighted, A[ia][jb] = H[ia][jb] / sqrt(m_i m_j)   (masses [N] fp32 in amu; null: unit masses)
 *   flags & NNHIP_EIG_PROJECT: A <- P A P, P = I - sum_k d_k d_k^T over the orthonormalised translations and rotations of the
 *     molecule about its centre of mass (fp64 Gram-Schmidt; a vector whose remainder is not above 1e-5 of its norm is dropped);
 *     a molecule with a non-zero cell row projects the translations only.  n_proj[b] = vectors projected (6, 5, 3 or 0).
 *   cyclic Jacobi, round-robin ordering, A and the eigenvectors in LDS in fp32, until off(A) <= 2^-24 ||A||_F or 30 sweeps:
 *     sweeps[b] = sweeps used, status[b] bit 0 (NNHIP_EIG_STATUS_SWEEPS) = the cap was hit (a block with a
 *     NaN or an Inf never counts as converged: it runs to the cap and says so).
 *   status[b] bit 1 (NNHIP_EIG_STATUS_SIZE): mol_ptr gives the molecule more atoms than mol_ptr_host did (see below); bit 2
 *     (NNHIP_EIG_STATUS_MASS): one of its masses is not positive and finite.  Such a molecule is not computed: its evals / modes keep
 *     what the caller put there.
 *   evals [3 N]: ascending per molecule, packed at 3 mol_ptr[b].  modes (may be null: eigenvalues only, bitwise the same ones):
 *     packed like the blocks at blk_ptr[b], ROW k = mode k ([3 n_b][n_b][3]), mass-weighted coordinates, unit norm, the component
 *     of largest magnitude (lowest index on a tie) positive.
 * blocks / blk_ptr: as nnhip_hessian_blocks writes them.  mol_ptr: int32 [n_mol + 1] atom offsets on the device; mol_ptr_host: the
 * same numbers on the host, which MUST be identical (a molecule that is larger by mol_ptr than by mol_ptr_host is skipped with
 * status bit 1, never computed in too little LDS) -- the dimension bound is checked from them BEFORE any launch (NNHIP_E_UNSUPPORTED, the message names
 * the bound and the molecule) and the launch's LDS is sized by the largest molecule.  pos [N][3] / cell [n_mol][3][3] are read with
 * NNHIP_EIG_PROJECT only.  A molecule of 0 atoms writes nothing; no float atomics, fixed summation order (bitwise repeatable).
 *   nnhip_eig_max_dim: the largest 3 n_b served (126: 42 atoms).
 * ------------------------------------------------------------------------ */
#define NNHIP_EIG_PROJECT 1
#define NNHIP_EIG_STATUS_SWEEPS 1
#define NNHIP_EIG_STATUS_SIZE 2
#define NNHIP_EIG_STATUS_MASS 4
int nnhip_eig_max_dim(void);
int nnhip_eig_blocks(const float* blocks, const int64_t* blk_ptr, const int32_t* mol_ptr, const int32_t* mol_ptr_host, int32_t n_mol,
                     const float* pos, const float* cell, const float* masses, int32_t flags, float* evals, float* modes,
                     int32_t* n_proj, int32_t* sweeps, int32_t* status, void* stream);

/* --------------------------------------------------------------------------
 * The same analysis above nnhip_eig_max_dim (csrc/eig_large.hip), opt-in: a two-sided BLOCK Jacobi spread over many workgroups by
 * ordinary launches, A and the eigenvectors in the caller's workspace in fp32.  Blocks of 32 coordinates on the round-robin ordering
 * of nnhip_eig_blocks, the order padded to a multiple of 64; per block step two launches (one workgroup per block pair diagonalises
 * its 64 x 64 sub-problem in LDS with the cyclic Jacobi of nnhip_eig_blocks; one workgroup per 64 x 64 tile forms Qt_k T Qt_l^T and
 * writes the tile and its mirror image, the eigenvector rows take Qt_k in the same launch), per sweep one launch that sums off(A)^2
 * and ||A||_F^2 per molecule in fp64 and ONE read-back of the per-molecule done flags by the host (the call synchronises `stream`
 * once per sweep: this is not the steady-state inference step).  Symmetrisation, mass-weighting, projection (flags, n_proj), the
 * stopping rule off(A) <= 2^-24 ||A||_F, the cap of 30 sweeps (sweeps[b] counts OUTER sweeps here), the status bits, the sorting and
 * the sign rule are those of nnhip_eig_blocks, and so are all arguments up to `status`; the outputs go to the same packed places.
 *   select_host [n_mol] (host; null: all): nonzero = this molecule is solved here.  The outputs of an unselected molecule are not
 *     touched, so nnhip_eig_blocks on the small molecules and this call on the others fill one set of arrays.
 *   ws / ws_bytes: device workspace, 256-byte aligned, at least nnhip_eig_large_ws_bytes(mol_ptr_host', n', modes != null) for the
 *     offsets mol_ptr_host' of the SELECTED molecules in their order (the size depends on their atom counts only; the offsets of
 *     all molecules give an upper bound): about 8 Mp^2 bytes per molecule with modes, 4 Mp^2 without (NNHIP_E_WORKSPACE).
 * Checked from mol_ptr_host BEFORE any launch, for the selected molecules: NNHIP_E_UNSUPPORTED above nnhip_eig_large_max_dim (the
 * message names the bound and the molecule).  A selected molecule to which mol_ptr gives more atoms than mol_ptr_host did is skipped
 * with status bit 1.  No float atomics, fixed summation orders: bitwise repeatable, the eigenvalues bitwise the same with and without
 * modes, and a molecule's result does not depend on the rest of the batch.
 *   nnhip_eig_large_max_dim: the largest 3 n_b served (1536: 512 atoms) -- the range the accuracy bound has been verified in and
 *     what the one-workgroup-per-molecule prepare / converge / finish kernels are sized for (the sort scratch of 3 x 1536 words is LDS).
 * ------------------------------------------------------------------------ */
int nnhip_eig_large_max_dim(void);
size_t nnhip_eig_large_ws_bytes(const int32_t* mol_ptr_host, int32_t n_mol, int32_t want_modes);
int nnhip_eig_blocks_large(const float* blocks, const int64_t* blk_ptr, const int32_t* mol_ptr, const int32_t* mol_ptr_host,
                           int32_t n_mol, const float* pos, const float* cell, const float* masses, int32_t flags, float* evals,
                           float* modes, int32_t* n_proj, int32_t* sweeps, int32_t* status, const uint8_t* select_host, void* ws,
                           size_t ws_bytes, void* stream);

/* --------------------------------------------------------------------------
 * Normal-mode sampling on the packed spectra of nnhip_eig_blocks (csrc/sample.hip): n_samples displaced geometries per molecule
 * drawn from its harmonic distribution at `temperature` (K), one workgroup per (molecule, tile of 32 samples), the mode matrix in LDS.
 *   modes / evals / blk_ptr / mol_ptr / mol_ptr_host / masses: as nnhip_eig_blocks writes / takes them (masses null: unit masses).
 *   thr [n_mol]: mode k of molecule b is LIVE iff evals > thr[b]; every other mode (projected, zero, imaginary) gets amplitude 0.
 *     n_skipped [n_mol] (int32): modes with evals < -thr[b] (-1: mol_ptr gives the molecule more atoms than mol_ptr_host did; it is
 *     not computed).
 *   classical (quantum = 0): sigma_k^2 = k_B T / lambda_k;  quantum: sigma_k^2 = (eps / 2 lambda) coth(eps / 2 k_B T), eps = hbar omega
 *     (T = 0: the ground state, eps / 2 lambda);  k_B = 8.617333262e-5 eV / K.
 *   xi: standard-normal draws, fp32, S x [3 n_b] per molecule at 3 S mol_ptr[b] (sample-major).  q = sigma xi ->
 *     amplitudes (same layout; may be null),  pos_out (same layout, as [n_b][3] per sample) = pos_i + sum_k q_k L[k][i] / sqrt(m_i),
 *     energy [n_mol x S] = 1/2 sum_k lambda_k q_k^2 (eV).  The samples of molecule b are molecules b S .. b S + S - 1 of the new batch.
 * The dimension bound is nnhip_eig_max_dim, checked from mol_ptr_host BEFORE any launch (NNHIP_E_UNSUPPORTED).  No float atomics, a
 * fixed summation order over k: bitwise repeatable, and a sample does not depend on n_samples or on its tile.
 * ------------------------------------------------------------------------ */
int nnhip_mode_sample(const float* modes, const float* evals, const int64_t* blk_ptr, const int32_t* mol_ptr,
                      const int32_t* mol_ptr_host, int32_t n_mol, const float* masses, const float* pos, const float* thr,
                      double temperature, int32_t quantum, int32_t n_samples, const float* xi, float* pos_out, float* energy,
                      float* amplitudes, int32_t* n_skipped, void* stream);

/* --------------------------------------------------------------------------
 * The same sampling above nnhip_eig_max_dim (csrc/sample_large.hip), opt-in: the mode matrix stays in HBM.  Two ordinary launches on
 * `stream` -- one workgroup per (molecule, tile of 32 samples) forms the amplitudes and the harmonic energies, one per (molecule,
 * tile of 32 samples, tile of 256 coordinates) the displacements -- no float atomics, no workspace.  The arguments up to n_skipped,
 * the formulas and the order of every sum over k are those of nnhip_mode_sample: a molecule both entries serve gets the same bits
 * from either, repeats are bitwise identical and a sample does not depend on n_samples, its tile or the rest of the batch.
 * Differences from nnhip_mode_sample:
 *   min_dim: the call serves the molecules with 3 n_b >= min_dim (decided from mol_ptr on the device; a molecule without atoms is
 *     never served).  No output of any other molecule is touched, so nnhip_mode_sample on the small molecules and this call with
 *     min_dim = nnhip_eig_max_dim() + 1 fill one set of arrays.  min_dim <= 1: every molecule.
 *   amplitudes is REQUIRED (the displacement kernel reads it): null gives NNHIP_E_INVALID.
 *   The bound is nnhip_mode_sample_large_max_dim (= nnhip_eig_large_max_dim: 1536, 512 atoms), checked from mol_ptr_host BEFORE any
 *     launch for the molecules min_dim selects: NNHIP_E_UNSUPPORTED, the message names the bound and the molecule.  A served
 *     molecule to which mol_ptr gives more coordinates than the largest served one of mol_ptr_host is not computed: n_skipped = -1.
 * Every other check is that of nnhip_mode_sample (decreasing mol_ptr_host, negative counts, a temperature that is not finite and
 * >= 0, more than 65535 x 32 samples).
 * ------------------------------------------------------------------------ */
int nnhip_mode_sample_large_max_dim(void);
int nnhip_mode_sample_large(const float* modes, const float* evals, const int64_t* blk_ptr, const int32_t* mol_ptr,
                            const int32_t* mol_ptr_host, int32_t n_mol, const float* masses, const float* pos, const float* thr,
                            double temperature, int32_t quantum, int32_t n_samples, const float* xi, float* pos_out, float* energy,
                            float* amplitudes, int32_t* n_skipped, int32_t min_dim, void* stream);

/* --------------------------------------------------------------------------
 * Molecular dynamics on the device (csrc/md.hip): ONE launch on `stream` integrates every atom of a batch between two force
 * evaluations.  The scheme is BAOAB with the O step exact; c1 = 1 with sigma = noise = NULL is velocity Verlet.  Per atom i and
 * coordinate k, all in fp32, every multiply-add one fma and every lone product one rounding (tests/md_ref.py restates the chain):
 *   finish (NNHIP_MD_FINISH):  v = fma(hk_i, F_ik, v)                         the second half kick of the step just evaluated
 *                              ke_out[i] = (0.5 mass_i) (vx vx + vy vy + vz vz)  only when ke_out != NULL (summed x, y, z by fma)
 *   begin  (NNHIP_MD_BEGIN):   v = fma(hk_i, F_ik, v);  x = fma(dth, v, pos_in);  v = fma(sigma_i, noise_ik, c1 v) [skipped when
 *                              noise == NULL];  pos_out = fma(dth, v, x)
 * flags = FINISH | BEGIN does both in that order with the same forces.  pos_in, force, noise [N,3]; vel [N,3] is updated in place;
 * hk [N] = dt / (2 m_i); mass [N] (read only for ke_out); sigma [N] and noise are both given or both NULL; dth = dt / 2.
 * pos_out [N,3] may NOT overlap pos_in (NNHIP_E_INVALID, nothing is launched): the caller of a deferred forward step must be able
 * to repeat that step from the positions it was queued with.  With FINISH alone pos_in / pos_out are not touched and may be NULL.
 * ke_out needs FINISH and mass.  n_atoms == 0: success, nothing is launched.  An atom with hk = sigma = 0 and v = 0 keeps its
 * position bit for bit (x = fma(dth, 0, x) twice).
 *   nnhip_md_kinetic: out[b] = sum of ke[mol_ptr[b] .. mol_ptr[b+1] - 1], one wave64 per molecule, lane l adds the atoms l, l + 64,
 *   ... in that order and the 64 partial sums meet in a fixed butterfly: no float atomics, bitwise repeatable, any molecule size.
 * ------------------------------------------------------------------------ */
#define NNHIP_MD_FINISH 1
#define NNHIP_MD_BEGIN 2
int nnhip_md_step(const float* pos_in, float* vel, const float* force, const float* hk, const float* mass, const float* sigma,
                  const float* noise, float dth, float c1, int32_t flags, int32_t n_atoms, float* pos_out, float* ke_out,
                  void* stream);
int nnhip_md_kinetic(const float* ke, const int32_t* mol_ptr, int32_t n_mol, float* out, void* stream);

/* --------------------------------------------------------------------------
 * Molecular dynamics with bond-length constraints on the device (csrc/rattle.hip): nnhip_md_step's launch for molecules whose
 * constrained distances |x_i - x_j| = d_c are kept by SHAKE / RATTLE.  Constrained BAOAB ("g-BAOAB", Leimkuhler & Matthews 2016,
 * one RATTLE per half drift); c1 = 1 with sigma = noise = NULL is velocity-Verlet RATTLE in two half drifts.  All in fp32, every
 * operation one rounding (tests/rattle_ref.py restates the chain in fp64 and emulates it in fp32).
 *
 * Tables (device, with host copies of the three offset tables; the caller keeps them equal):
 *   mol_ptr      int32 [B+1]   atom offsets of the molecules
 *   mol_col_ptr  int32 [B+1]   molecule b owns the colours mol_col_ptr[b] .. mol_col_ptr[b+1] - 1 (none: an unconstrained molecule)
 *   col_ptr      int32 [K+1]   colour k owns the constraints col_ptr[k] .. col_ptr[k+1] - 1; K = n_col; C = col_ptr[K]
 *   con_pair     int32 [C,2]   the two atoms of a constraint, counted from the first atom of its molecule (0 .. n_b - 1)
 *   con_d2       fp32  [C]     d_c^2
 * Constraints are thus sorted by molecule and, within one, by colour.  No two constraints of a colour may share an atom (the
 * caller's colouring; the lanes of a wave take a colour's constraints side by side).  The offset tables are checked on their host
 * copies; the kernel skips a constraint whose atoms lie outside its molecule (the molecule counts as failed) and never reads or
 * writes outside the arrays whatever the device tables hold.
 *
 * One launch, for a molecule WITH constraints.  x_first is the INPUT position of its first atom, y = fl32(x - x_first) per
 * coordinate, w = inv_mass (0 for a fixed atom, whose hk, sigma and velocity are 0 as well):
 *   NNHIP_MD_FINISH:    v = fma(hk_i, F, v);  PROJECT v at y;  ke_out[i] = (0.5 mass_i)(vx vx + vy vy + vz vz) as nnhip_md_step
 *   NNHIP_MD_BEGIN:     v = fma(hk_i, F, v);  PROJECT v at y;  DRIFT;  [v = fma(sigma_i, noise, c1 v);  PROJECT v at y]  DRIFT
 *                       (the bracket is skipped when noise == NULL)
 *     DRIFT:            r = y;  y = fma(dth, v, r);  D = 0;  SHAKE y along r;  v = fma(D, inv_dth, v);  PROJECT v at y
 *                       D_i is the sum of the updates SHAKE applied to atom i (= y'' - y'), accumulated by the same fmas as y: the
 *                       difference of the two positions would carry 2^-24 |y| / dth per update into the velocities
 *   NNHIP_MDC_PROJECT:  r = y;  SHAKE y along r;  PROJECT v at y          (valid alone: imposes the constraints on a start state)
 *   pos_out = fl32(x_first + y) with BEGIN or PROJECT -- but an atom with inv_mass = 0 gets pos_in bit for bit; vel in place.
 * FINISH | BEGIN performs exactly the operations of FINISH followed by BEGIN with the same forces.
 *   SHAKE, constraint (i, j, d2):  s = y_i - y_j;  q = r_i - r_j;  e = d2 - s.s;  applied iff |e| > tol d2:
 *                                  g = e / ((2 (w_i + w_j)) (s.q));  y_i = fma(g w_i, q, y_i);  y_j = fma(-(g w_j), q, y_j);
 *                                  D_i = fma(g w_i, q, D_i);  D_j = fma(-(g w_j), q, D_j)
 *   PROJECT, constraint (i, j, d2): q = y_i - y_j;  p = q.(v_i - v_j);  applied iff |p| dth > tol d2:
 *                                  g = p / ((w_i + w_j) d2);  v_i = fma(-(g w_i), q, v_i);  v_j = fma(g w_j, q, v_j)
 *   (dot products: fma(az, bz, fma(ay, by, ax bx)).)  Both are Gauss-Seidel sweeps over the molecule's constraints in colour order;
 *   a solve ends when a whole sweep applied no update, or after max_iter sweeps.  Breakdown guard: a SHAKE constraint with
 *   s.q <= NNHIP_MDC_GUARD d2 (the bond turned by almost a right angle within half a step), and any constraint with w_i + w_j <= 0,
 *   d2 <= 0, i == j or an atom outside its molecule, is SKIPPED -- nothing divides by a vanishing number: a failed solve may leave
 *   a wrong geometry, never a non-finite store that finite inputs did not hold.
 *   n_failed[b] (sticky, zeroed by the caller) is incremented ONCE per launch in which a solve of molecule b ended at max_iter with
 *   its last sweep still updating, or skipped a constraint;  n_sweeps[b] = the largest sweep count of this launch's solves (the
 *   closing sweep without an update counts; 0 for an unconstrained molecule).
 * The result does not depend on which lane takes which constraint: bitwise repeatable, a molecule's outputs are independent of the
 * rest of the batch and of its place in it.  The molecule-relative y makes convergence independent of where a molecule sits
 * (unwrapped periodic positions drift far from the origin); what the STORED positions can show is tol plus the rounding of the
 * stored coordinates.
 * A molecule WITHOUT constraints takes nnhip_md_step's chain bit for bit (PROJECT: pos_out = pos_in, vel untouched).
 *
 * One wave64 per molecule, its y, r, v, D, w in LDS (13 floats per atom): a molecule with constraints has at most nnhip_md_constrained_max_atoms() =
 * NNHIP_MDC_MAX_ATOMS atoms -- a kernel for batches of molecules, not for one large system.
 * NNHIP_E_INVALID, nothing launched and nothing written: pos_out overlapping pos_in (the reason is given at nnhip_md_step), a
 * constrained molecule above the bound, NULL mandatory pointers or tables, offset tables (host copies) that do not start at 0,
 * decrease, or do not end at n_atoms / n_col, n_mol < 1 with n_atoms > 0, tol <= 0 (or NaN), max_iter < 1, flags other than FINISH,
 * BEGIN, FINISH | BEGIN or PROJECT, sigma without noise or the reverse, ke_out without mass and FINISH.  force and hk may be NULL
 * with PROJECT, pos_out with FINISH alone.  n_atoms == 0 is success without a launch.
 * ------------------------------------------------------------------------ */
#define NNHIP_MDC_PROJECT 4
#define NNHIP_MDC_MAX_ATOMS 256
#define NNHIP_MDC_GUARD 0.1f
int nnhip_md_constrained_max_atoms(void);
int nnhip_md_step_constrained(const float* pos_in, float* vel, const float* force, const float* hk, const float* mass,
                              const float* inv_mass, const float* sigma, const float* noise, float dth, float inv_dth, float c1,
                              int32_t flags, int32_t n_atoms, const int32_t* mol_ptr, const int32_t* mol_ptr_host, int32_t n_mol,
                              const int32_t* con_pair, const float* con_d2, const int32_t* mol_col_ptr,
                              const int32_t* mol_col_ptr_host, const int32_t* col_ptr, const int32_t* col_ptr_host, int32_t n_col,
                              float tol, int32_t max_iter, float* pos_out, float* ke_out, int32_t* n_failed, int32_t* n_sweeps,
                              void* stream);

/* --------------------------------------------------------------------------
 * Geometry relaxation on the device (csrc/relax.hip): ONE launch on `stream` moves every molecule of a batch by one L-BFGS step
 * from the forces just evaluated.  L-BFGS without line search in ASE's convention (fixed H0 = 1 / alpha, the longest atomic
 * displacement capped at maxstep); every molecule has its own history, one wave64 works on one molecule, every reduction is a
 * lane-local sum / max in atom order and a fixed butterfly: no float atomics, a molecule's outputs are bitwise independent of the
 * rest of the batch and of its place in it.  All arithmetic in fp32, every operation one rounding (tests/relax_ref.py restates it).
 *
 * State of molecule b (device arrays of the caller, zero before the first step; memory = m, 1 <= m <= NNHIP_LBFGS_MAX_MEMORY):
 *   converged[b] (sticky), n_steps[b], n_pairs[b] (<= m), head[b] (the slot of the pending pair)      int32 [B] each
 *   S, Y   fp32 [m][N][3], slot-major: displacements s and force differences y of the stored pairs
 *   rho    fp32 [B][m] = 1 / (y.s) per slot;      f_prev  fp32 [N][3]: the (masked) forces of the previous step
 * Per launch: pos_in, force [N,3]; free_mask uint8 [N] (0 = fixed atom) or NULL (all free); mol_ptr int32 [B+1] atom offsets;
 * tol2 = fl32(fmax^2); alpha; maxstep; flags; work [N,3] scratch (the two-loop vector of molecules above 64 atoms; may be NULL when
 * n_atoms <= 64); outputs pos_out [N,3] and fmax_out [B].
 *
 * One step for molecule b:
 *   1. f_i = F_i for free atoms and exactly 0 for fixed ones.
 *   2. fmax2 = max_i |f_i|^2;  fmax_out[b] = sqrt(fmax2).
 *   3. Frozen when converged[b] is set, or fmax2 < tol2 (an empty molecule always), or flags has NNHIP_LBFGS_CHECK_ONLY:
 *      converged[b] is set in the first two cases only, pos_out = pos_in bitwise, every other state word is left untouched.
 *   4. Otherwise, when n_steps[b] > 0, the pending pair in slot `head` is completed:  y = f_prev - f,  s = S[head];  it is ACCEPTED
 *      iff  y.s > 0  and  (y.s)^2 > NNHIP_LBFGS_CURVATURE_MIN^2 (y.y)(s.s)  -- then Y[head] = y, rho[head] = 1 / y.s,
 *      n_pairs = min(n_pairs + 1, m), head = (head + 1) % m -- and otherwise the slot is reused; a rejection with n_pairs == m
 *      sets n_pairs = m - 1, because the pending s had taken the place of the oldest pair's in the ring.  This is a deviation from ASE,
 *      which takes every pair: below cos(y, s) = 1e-4 the curvature along s is not distinguishable from the fp32 rounding of the
 *      forces, and one pair with y.s <= 0 makes the inverse Hessian indefinite.
 *   5. Two-loop recursion over the n_pairs newest pairs:  q = -f;  newest first  a_i = rho_i (s_i.q), q -= a_i y_i;  z = q / alpha;
 *      oldest first  z += s_i (a_i - rho_i (y_i.z)).
 *   6. p = -z;  longest = max_i |p_i|;  when longest >= maxstep:  p *= maxstep / longest.
 *   7. pos_out = pos_in + p (a fixed atom keeps its bits);  S[head] = pos_out - pos_in, in fp32 on the stored values;  f_prev = f;
 *      n_steps[b] += 1.
 * pos_out may NOT overlap pos_in (NNHIP_E_INVALID, nothing is launched), for the reason given at nnhip_md_step.  NULL mandatory
 * pointers, memory outside 1 .. NNHIP_LBFGS_MAX_MEMORY, unknown flag bits, tol2 < 0, alpha <= 0 or maxstep <= 0 (or NaN) are
 * refused likewise.  n_mol == 0 is success without a launch; n_atoms == 0 marks every molecule converged.  A molecule whose state
 * words are impossible (head outside 0 .. m-1, n_pairs outside 0 .. m, n_steps < 0, atom offsets outside 0 .. n_atoms) is not
 * touched and gets fmax_out = NaN.
 * Cost: a molecule of n atoms takes about 2 m ceil(n / 64) dependent sweeps of ONE wave -- a kernel for batches of molecules.
 * ------------------------------------------------------------------------ */
#define NNHIP_LBFGS_CHECK_ONLY 1
#define NNHIP_LBFGS_MAX_MEMORY 64
#define NNHIP_LBFGS_CURVATURE_MIN 1e-4f
int nnhip_lbfgs_step(const float* pos_in, const float* force, const uint8_t* free_mask, const int32_t* mol_ptr, int32_t n_mol,
                     int32_t n_atoms, int32_t memory, float tol2, float alpha, float maxstep, int32_t flags, int32_t* converged,
                     int32_t* n_steps, int32_t* n_pairs, int32_t* head, float* S, float* Y, float* rho, float* f_prev, float* work,
                     float* pos_out, float* fmax_out, void* stream);

/* The workgroup-per-system form of nnhip_lbfgs_step, for large systems: the same step, state, arguments, checks and refusals (work
 * is mandatory when n_atoms > 64, as there), with ONE WORKGROUP of NNHIP_LBFGS_WG_THREADS = 1024 threads (16 waves) working on a
 * system instead of one wave64.  wg_min_atoms routes each system on the device, from mol_ptr, without a host read:
 *   wg_min_atoms <= 0   every system (empty ones included) is stepped by the workgroup kernel; the wave kernel is not launched
 *   wg_min_atoms >  0   a system of n >= wg_min_atoms atoms is stepped by the workgroup kernel, a smaller one by the wave kernel of
 *                       nnhip_lbfgs_step (and gets exactly the bits that call gives it); both kernels are launched on `stream`,
 *                       they own disjoint systems and neither touches a word of the other's, so their order does not matter.  (A
 *                       system whose atom offsets leave 0 .. n_atoms has no atom count: the wave kernel marks it, fmax_out = NaN.)
 * The workgroup kernel: thread t owns the atoms t, t + 1024, ... of its system in every sweep; the two-loop work vector is three
 * registers up to 1024 atoms, the thread's rows of `work` above.  A reduction is the thread-local sum (max) in atom order, the
 * butterfly 32 .. 1 within each wave, the 16 wave results through LDS and one barrier, and a fixed pairwise fold
 * (p[i] += p[i + d], d = 8, 4, 2, 1) that every thread does itself -- so a dot product over n atoms passes through
 * 3 + ceil(n / 1024) + 6 + 4 roundings instead of 3 + ceil(n / 64) + 6.  No float atomics, no communication between workgroups: a
 * system's outputs are bitwise independent of the rest of the batch and of its place in it, frozen systems keep their bits, refused
 * calls write nothing -- every per-system property of nnhip_lbfgs_step.  Because the order of the reductions differs, THE BITS OF
 * THE TWO FORMS DIFFER from each other above 64 atoms (up to 64, fifteen of the sixteen wave results are exact zeros and the bits
 * are the wave form's; y and S[head], single rounded operations, are the same function of their inputs in both at every size);
 * both satisfy the same fp64 restatement with their own depth.  One workgroup serves a system whatever its size; grid-stride over
 * the systems with at most 2048 workgroups.
 * Cost: about 2 m ceil(n / 1024) dependent sweeps of one workgroup, each reduction one barrier. */
#define NNHIP_LBFGS_WG_THREADS 1024
int nnhip_lbfgs_step_wg(const float* pos_in, const float* force, const uint8_t* free_mask, const int32_t* mol_ptr, int32_t n_mol,
                        int32_t n_atoms, int32_t memory, float tol2, float alpha, float maxstep, int32_t wg_min_atoms, int32_t flags,
                        int32_t* converged, int32_t* n_steps, int32_t* n_pairs, int32_t* head, float* S, float* Y, float* rho,
                        float* f_prev, float* work, float* pos_out, float* fmax_out, void* stream);

/* --------------------------------------------------------------------------
 * Variable-cell geometry relaxation on the device (csrc/cellrelax.hip): ONE launch on `stream` moves the atoms and the cell of
 * every periodic system of a batch by one L-BFGS step from the forces and the virial just evaluated.  The method is ASE's
 * UnitCellFilter under nnhip_lbfgs_step's recursion (one text: csrc/lbfgs_chain.h).  Per system b with n atoms: h the cell (rows
 * are lattice vectors), h0 the cell at the start, F the deformation gradient, q the reference-frame positions:
 *   h = h0 F^T,   x = q F^T,   generalised coordinates X = [q ; c F]  (n + 3 rows of 3),   generalised forces G = [f F ; Wc / c]
 *   Wc = (W - p V I) F^-T   with W the virial (minus the strain derivative of the energy, eV), V = det h, p = pressure[b] in
 *   eV / Angstrom^3 and c = cell_factor[b]; G is minus the gradient of the enthalpy E + p V with respect to X.
 * Launch shape and rounding discipline are nnhip_lbfgs_step's (one wave64 per system, fixed reductions, no float atomics, every
 * operation one fp32 rounding; a system's bits do not depend on the rest of the batch).  tests/cellrelax_ref.py restates it.
 *
 * Row layout: x_in, x_out, G, g_prev, work and every slot of S and Y have R = n_atoms + 3 n_mol rows of 3; system b owns the rows
 * [mol_ptr[b] + 3 b, mol_ptr[b+1] + 3 b + 3): its atom rows, then its three cell rows (c F, row by row).  Before the first step
 * the caller fills x_in with q = pos and c I (F = I, cell_in = h0) and zeroes the state.
 * State of system b (memory = m): converged, n_steps, n_pairs, head int32 [B]; S, Y fp32 [m][R][3]; rho fp32 [B][m]; g_prev fp32
 * [R][3] (the generalised forces of the previous step) -- as nnhip_lbfgs_step's, over generalised rows.
 * Per launch: x_in [R,3]; pos_in, force [N,3]; virial, cell_in, h0 [B,3,3]; free_mask uint8 [N] or NULL; mol_ptr int32 [B+1];
 * pressure, cell_factor fp32 [B]; tol2 = fl32(fmax^2); alpha; maxstep; strain_mask: bit k frees the Voigt component k (xx, yy, zz,
 * yz, xz, xy), 63 = all; flags; work [R,3] scratch (may be NULL when R <= 64).  Outputs: G [R,3] (written for the systems that
 * step), x_out [R,3], pos_out [N,3], cell_out [B,3,3], fmax_out [B].
 *
 * One step for system b (dot3(a, b) = fma(a2, b2, fma(a1, b1, a0 b0)); cof(A): rows A1 x A2, A2 x A0, A0 x A1 with
 * (u x v)_0 = fma(u1, v2, -(u2 v1)) and cyclic; det(A) = dot3(A0, cof(A)0)):
 *   1. F_jk = x_in[n + j][k] / c;  V = det(cell_in);  FinvT = cof(F) / det(F).
 *      The system is SKIPPED (nothing written but fmax_out[b] = NaN) when det F <= 0, when F, det F, V, p or c is not finite, when
 *      c <= 0, or when its state words are impossible (as nnhip_lbfgs_step).
 *   2. Wp = W with p V subtracted on the diagonal;  Wc_ij = fma(Wp_i2, FinvT_2j, fma(Wp_i1, FinvT_1j, Wp_i0 FinvT_0j));  then, in this
 *      order:  NNHIP_CELL_LBFGS_HYDROSTATIC  Wc = (((Wc_00 + Wc_11) + Wc_22) / 3) I;   strain_mask  the masked components are +0;
 *      NNHIP_CELL_LBFGS_CONSTANT_VOLUME  Wc_ii -= ((Wc_00 + Wc_11) + Wc_22) / 3.
 *   3. G: cell row i = Wc_i / c;  atom row a, component j = fma(f_a2, F_2j, fma(f_a1, F_1j, f_a0 F_0j)), exactly 0 for a fixed atom
 *      (its q is frozen: it rides with the cell).
 *   4. fmax2 = max over all n + 3 rows of |G_row|^2;  fmax_out[b] = sqrt(fmax2).
 *   5. Frozen when converged[b] is set, or fmax2 < tol2, or flags has NNHIP_CELL_LBFGS_CHECK_ONLY: converged[b] is set in the first
 *      two cases only; x_out, pos_out, cell_out = x_in, pos_in, cell_in bitwise; nothing else is touched (G included).
 *   6. Otherwise steps 4 to 7 of nnhip_lbfgs_step on (X, G) over the n + 3 rows (the clamp takes the longest ROW, cell rows
 *      included; the work vector is in registers up to 64 rows), G_prev = G, n_steps[b] += 1.
 *   7. F'_jk = x_out[n + j][k] / c;  cell_out_ij = dot3_k(h0_ik, F'_jk);  pos_out_aj = dot3_k(q_ak, F'_jk) with q = x_out's atom rows.
 * x_out, pos_out and cell_out may NOT overlap x_in, pos_in and cell_in (NNHIP_E_INVALID, nothing is launched), for the reason
 * given at nnhip_md_step.  NULL mandatory pointers, memory outside 1 .. NNHIP_LBFGS_MAX_MEMORY, unknown flag bits, strain_mask
 * outside 0 .. 63, tol2 < 0, alpha or maxstep that are not finite and > 0 are refused likewise; cell_factor lives on the device,
 * so a value that is not finite and > 0 skips its system (step 1).  n_mol == 0 is success without a launch.
 * Cost: a system of n atoms takes about 2 m ceil((n + 3) / 64) dependent sweeps of ONE wave.
 * ------------------------------------------------------------------------ */
#define NNHIP_CELL_LBFGS_CHECK_ONLY 1
#define NNHIP_CELL_LBFGS_HYDROSTATIC 2
#define NNHIP_CELL_LBFGS_CONSTANT_VOLUME 4
int nnhip_cell_lbfgs_step(const float* x_in, const float* pos_in, const float* force, const float* virial, const float* cell_in,
                          const float* h0, const uint8_t* free_mask, const int32_t* mol_ptr, const float* pressure,
                          const float* cell_factor, int32_t n_mol, int32_t n_atoms, int32_t memory, float tol2, float alpha,
                          float maxstep, int32_t strain_mask, int32_t flags, int32_t* converged, int32_t* n_steps, int32_t* n_pairs,
                          int32_t* head, float* S, float* Y, float* rho, float* g_prev, float* work, float* G, float* x_out,
                          float* pos_out, float* cell_out, float* fmax_out, void* stream);

/* The workgroup-per-system form of nnhip_cell_lbfgs_step: the same step, state, arguments, checks and refusals (work is mandatory
 * when n_atoms + 3 n_mol > 64, as there), with one workgroup of NNHIP_LBFGS_WG_THREADS threads per system, as nnhip_lbfgs_step_wg
 * has it.  wg_min_atoms routes a system by its ATOM count n (the chain walks n + 3 rows): <= 0 sends every system to the workgroup
 * kernel alone; > 0 sends the systems of n >= wg_min_atoms atoms there and leaves the others to the wave kernel of
 * nnhip_cell_lbfgs_step with exactly that call's bits.  Thread t owns the generalised rows t, t + 1024, ... of its system; the 3x3
 * quantities of the prologue are formed by every thread from the same loads; the cell rows of G are stored by the threads that own
 * them; the three new cell rows of x_out reach all threads through LDS and a barrier.  The work vector is in registers up to 1024
 * rows.  The bits of the two forms differ from each other (the order of the reductions differs). */
int nnhip_cell_lbfgs_step_wg(const float* x_in, const float* pos_in, const float* force, const float* virial, const float* cell_in,
                             const float* h0, const uint8_t* free_mask, const int32_t* mol_ptr, const float* pressure,
                             const float* cell_factor, int32_t n_mol, int32_t n_atoms, int32_t memory, float tol2, float alpha,
                             float maxstep, int32_t strain_mask, int32_t wg_min_atoms, int32_t flags, int32_t* converged,
                             int32_t* n_steps, int32_t* n_pairs, int32_t* head, float* S, float* Y, float* rho, float* g_prev,
                             float* work, float* G, float* x_out, float* pos_out, float* cell_out, float* fmax_out, void* stream);

/* --------------------------------------------------------------------------
 * Intrinsic-reaction-coordinate following on the device (csrc/irc.hip): ONE launch on `stream` moves every path of a batch by one
 * step of the damped velocity Verlet scheme (after Hratchian and Schlegel, J. Phys. Chem. A 106, 165 (2002)) from the forces just
 * evaluated.  The path is a trajectory whose speed is reset to the constant v0 after every step: with a = c F / m
 * (c = NNHIP_IRC_ACCEL: eV / (Angstrom amu) in Angstrom / fs^2, the square of dynamics.FS) it moves along M^-1 F, steepest descent in
 * mass-weighted coordinates, on one gradient per step.  One wave64 works on one molecule, every reduction is a lane-local sum / max
 * in atom order and a fixed butterfly: no float atomics, a molecule's outputs are bitwise independent of the rest of the batch and
 * of its place in it.  All arithmetic in fp32, every operation one rounding (tests/irc_ref.py restates it); the square roots and
 * the cube root are taken as good to 2 ulp.
 *
 * State of molecule b (device arrays of the caller):
 *   status[b] (sticky: 0 running, 1 minimum reached, 2 turned), armed[b] (sticky), n_steps[b]      int32 [B] each
 *   dt[b] (fs, inside [dt_min, dt_max]), dt_prev[b], arc[b] (amu^1/2 Angstrom)                     fp32 [B] each
 *   vel (Angstrom / fs; the caller's start velocity of norm v0 before the first step), x_prev, v_prev, a_prev      fp32 [N][3] each
 * Per launch: pos_in = x_n, force = F_n [N,3]; free_mask uint8 [N] (0 = fixed atom) or NULL (all free); masses fp32 [N] (amu);
 * mol_ptr int32 [B+1] atom offsets; v0 (Angstrom / fs); delta0 (Angstrom, the error target); dt_min, dt_max (fs); tol2 =
 * fl32(fmax^2); flags; outputs pos_out = x_{n+1} [N,3] and fmax_out [B].  A fixed atom is in no sum and never moves; |.| is the
 * Euclidean norm over the molecule's free atoms.
 *
 * One launch for molecule b:
 *   1. f_i = F_i for free atoms and exactly 0 for fixed ones.  fmax2 = max_i |f_i|^2;  fmax_out[b] = sqrt(fmax2).  armed[b] is set
 *      when fmax2 >= tol2 (only while status[b] == 0: a stopped molecule keeps every bit).
 *   2. Stop tests, never with NNHIP_IRC_CHECK_ONLY and never for status[b] != 0:  when n_steps >= 1 and P = sum_i f_i.vel_i < 0
 *      (vel: the damped velocity the previous launch stored -- the last step passed the minimum along the path): status = 2;
 *      otherwise, when armed[b] and fmax2 < tol2: status = 1.  (The force AT a saddle is below the threshold too: it counts only
 *      once the path has left that region.)
 *   3. Frozen when status[b] != 0 (before or now), when the molecule has no atoms, or with NNHIP_IRC_CHECK_ONLY:  pos_out = pos_in
 *      bitwise and no other state word is touched.
 *   4. Otherwise  a_n = (c f) / m,  and when n_steps >= 1:  v = fma(0.5 (a_prev + a_n), dt_prev, vel), then v = v (v0 / |v|) -- but
 *      with |v| == 0 nothing divides and v = vel as stored.  n_steps == 0:  v = vel.
 *   5. x_{n+1} = fma(a_n, (0.5 dt) dt, fma(v, dt, x_n)).
 *   6. arc[b] += sqrt(sum_i m_i |x_{n+1,i} - x_{n,i}|^2), the differences in fp32 on the stored values (a lane adds an atom by
 *      fma(m_i, |d_i|^2, acc)).
 *   7. When n_steps >= 1, with T = dt_prev + dt:  x' = fma(a_prev, (0.5 T) T, fma(v_prev, T, x_prev)),  Delta = |x_{n+1} - x'|,
 *      dt_next = dt cbrt(delta0 / Delta) clamped into [dt / 2, 2 dt] and then into [dt_min, dt_max].  Delta == 0 or n_steps == 0:
 *      dt_next = dt.
 *   8. x_prev = x_n, v_prev = vel = v, a_prev = a_n, dt_prev = dt, dt = dt_next, n_steps += 1.
 * pos_out may NOT overlap pos_in (NNHIP_E_INVALID, nothing is launched), for the reason given at nnhip_md_step.  NULL mandatory
 * pointers, unknown flag bits, v0, delta0 or dt_min that are not finite and > 0, dt_max < dt_min (or not finite) and tol2 < 0 are
 * refused likewise.  n_mol == 0 is success without a launch.  A molecule whose state words are impossible (status outside 0 .. 2,
 * n_steps < 0, dt outside [dt_min, dt_max] or NaN, atom offsets outside 0 .. n_atoms) is not touched and gets fmax_out = NaN; so
 * does a molecule with a free atom whose mass is not finite and > 0 -- the masses live on the device, where a launch function that
 * may not wait for it cannot read them; the driver refuses such masses when it is made.
 * Forces are taken as finite: a NaN component is passed over by the max in fmax2 (fmaxf returns its other operand)
 * and goes into the positions of its molecule, and of no other; the model's own input checks are the guard.
 * ------------------------------------------------------------------------ */
#define NNHIP_IRC_CHECK_ONLY 1
#define NNHIP_IRC_ACCEL 0.00964853322f
int nnhip_irc_step(const float* pos_in, const float* force, const uint8_t* free_mask, const float* masses, const int32_t* mol_ptr,
                   int32_t n_mol, int32_t n_atoms, float v0, float delta0, float dt_min, float dt_max, float tol2, int32_t flags,
                   int32_t* status, int32_t* armed, int32_t* n_steps, float* dt, float* dt_prev, float* arc, float* vel,
                   float* x_prev, float* v_prev, float* a_prev, float* pos_out, float* fmax_out, void* stream);

/* --------------------------------------------------------------------------
 * Dimer-method saddle search on the device (csrc/dimer.hip): ONE launch on `stream` advances the dimer of every molecule of a batch
 * by one move, from the forces just evaluated at each molecule's PROBE geometry.  Min-mode following after Henkelman and Jonsson
 * (1999) with the one-evaluation rotations of Heyden, Bell and Keil (2005) and Kaestner and Sherwood (2008): conjugate-gradient
 * rotation directions, the rotated endpoint's force interpolated, an L-BFGS translation (nnhip_lbfgs_step's recursion, one text:
 * csrc/lbfgs_chain.h).  A molecule's probe is its dimer's centre (phase 0), the endpoint centre + delta N (phase 1) or a trial
 * endpoint (phase 2), so a step of a batch is always one force evaluation of B geometries and the centre's force F0 is never
 * evaluated twice.  One wave64 works on one molecule, every reduction is a lane-local sum / max in atom order and a fixed
 * butterfly: no float atomics, a molecule's outputs are bitwise independent of the rest of the batch and of its place in it.  All
 * arithmetic in fp32, every operation one rounding, and only sums, products, quotients and square roots: no atan, sin or cos
 * (tests/dimer_ref.py restates the chain).
 *
 * State of molecule b (device arrays of the caller, zero before the first launch except the row MODE):
 *   istate  int32 [NNHIP_DIMER_N_INT][B]: rows STATUS (0 running, 1 converged, sticky), PHASE (0 centre, 1 endpoint, 2 trial), STEPS
 *           (translations), EVALS, ROT (rotations of this cycle), ROT_TOTAL, PAIRS, HEAD (the L-BFGS ring, as nnhip_lbfgs_step),
 *           PENDING (1: slot HEAD and F_PREV hold the pending pair of a translation made with C < 0)
 *   fstate  fp32 [NNHIP_DIMER_N_FLOAT][B]: rows CURVATURE C (eV / Angstrom^2), SLOPE b1, C2 and S2 (cosine and sine of twice the trial
 *           angle), DNORM (the norm of the rotation direction before it was normalised)
 *   vstate  fp32 [NNHIP_DIMER_N_VEC][N][3]: rows CENTER, MODE (N: a unit vector per molecule, zero on fixed atoms -- the caller's
 *           start direction), F0, F1 (forces at the centre and at the endpoint), THETA (the unit rotation direction), THETA_ROT
 *           (THETA carried into the rotated plane), G_OLD, X_PREV (the centre before the last translation), F_PREV
 *   S, Y    fp32 [m][N][3], rho fp32 [B][m]: the translation's L-BFGS history, laid out as nnhip_lbfgs_step's
 * Per launch: pos_in [N,3] the probes, force [N,3] and energy [B] (may be NULL) the model's results there; free_mask uint8 [N]
 * (0 = fixed atom) or NULL; mol_ptr int32 [B+1]; delta (Angstrom, the dimer's half length); rot_tol = tan(2 x the rotation
 * tolerance); max_rotations; tol2 = fl32(fmax^2); alpha, maxstep as nnhip_lbfgs_step; work [N,3] scratch when n_atoms > 64; outputs
 * pos_out [N,3] (the next probes), fmax_out [B] and energy_out [B] (may be NULL): the largest force norm and the energy at the
 * centre, written by every launch whose probe IS the centre (phase 0) and by no other.  A fixed atom has f = 0, reads as 0 in
 * every state vector, is in no sum and never moves.  sum(a, b) is the sum of a_i . b_i over the molecule's atoms.
 *
 * One launch for molecule b.  Frozen when STATUS != 0, when the molecule has no atoms, or with NNHIP_DIMER_CHECK_ONLY: pos_out =
 * pos_in bitwise and no state word is touched.  Otherwise EVALS += 1 and, by PHASE:
 *   0  F0 = f (the first launch also sets CENTER = pos_in).  When STEPS >= 1, max_i |f_i|^2 < tol2 and C < 0: STATUS = 1, pos_out =
 *      pos_in.  Otherwise pos_out = CENTER + delta N, PHASE = 1, ROT = 0.
 *   1  F1 = f; then ASSESS.
 *   2  (f is the force at CENTER + delta N*, N* = c1 N + s1 THETA with c1 = sqrt((1 + C2) / 2), s1 = S2 / (2 c1), formed as the
 *      launch before formed them.)  C* = sum(F0 - f, N*) / delta;  a1 = (C - C* + b1 S2) / (1 - C2);  the angle phi that minimises the
 *      fitted curvature a0 / 2 + a1 cos 2 phi + b1 sin 2 phi has (cos 2 phi, sin 2 phi) = -(a1, b1) / sqrt(a1^2 + b1^2) (phi = 0 when
 *      that root is 0 or not finite);  cos phi = sqrt((1 + cos 2 phi) / 2), sin phi = sign(sin 2 phi) sqrt((1 - cos 2 phi) / 2)
 *      -- of these two roots the one that does not cancel is taken and the other formed from sin 2 phi = 2 sin phi cos phi, and
 *      1 - C2 is formed as 2 s1^2;
 *      F1 = [(s1 cos phi - c1 sin phi) / s1] F1 + [sin phi / s1] f + [1 - cos phi - sin phi s1 / (1 + c1)] F0;
 *      THETA_ROT = -sin phi N + cos phi THETA;  N = (cos phi N + sin phi THETA) / |...|;  ROT += 1, ROT_TOTAL += 1; then ASSESS.
 *   ASSESS     g = F1 - F0;  C = -sum(g, N) / delta;  G = g - sum(g, N) N.  Direction D: after phase 1, D = G; after phase 2,
 *              beta = max(0, sum(G, G - G_OLD) / sum(G_OLD, G_OLD)) (0 when the divisor is 0), D = G + beta DNORM THETA_ROT,
 *              D -= sum(D, N) N, and D = G unless sum(D, G) > 0.  DNORM = |D|;  THETA = D / DNORM;  b1 = -sum(g, THETA) / delta;
 *              r = -b1 / |C|;  C2 = 1 / sqrt(1 + r^2), S2 = r C2 (C == 0, or 1 + r^2 not finite: C2 = 0, S2 = 1, r = +inf).
 *              The rotation is done when DNORM == 0, r < rot_tol or ROT >= max_rotations: TRANSLATE.  Otherwise G_OLD = G,
 *              pos_out = CENTER + delta N*, PHASE = 2.
 *   TRANSLATE  p = sum(F0, N);  F+ = F0 - 2 p N when C < 0, else -p N.  One step of nnhip_lbfgs_step's recursion on (CENTER, F+):
 *              its pending pair and acceptance rule, H0 = 1 / alpha, the maxstep cap.  The history holds pairs of translations
 *              made with C < 0 alone: with C >= 0 the step is the plain F+ / alpha (capped), PAIRS = 0 and PENDING = 0 -- -p N is
 *              no gradient, it turns with N, and a pair formed from it describes that rotation and not the surface; with C < 0
 *              the pending pair is completed only when PENDING is set, and PENDING = 1 afterwards.
 *              X_PREV = CENTER;  CENTER = pos_out = the new centre;  F_PREV = F+;  STEPS += 1;  PHASE = 0.
 * pos_out may NOT overlap pos_in (NNHIP_E_INVALID, nothing is launched), for the reason given at nnhip_md_step.  NULL mandatory
 * pointers, memory outside 1 .. NNHIP_LBFGS_MAX_MEMORY, unknown flag bits, delta, rot_tol, alpha or maxstep that are not finite and
 * > 0, tol2 < 0 (or NaN) and max_rotations < 0 are refused likewise.  n_mol == 0 is success without a launch.  A molecule whose
 * state words are impossible (STATUS outside 0 .. 1, PHASE outside 0 .. 2, a negative count, HEAD outside 0 .. m-1, PAIRS outside
 * 0 .. m, PENDING outside 0 .. 1, EVALS == 0 with PHASE != 0, a C that is not finite once STEPS >= 1 or PHASE == 2, atom offsets outside 0 .. n_atoms) is
 * not touched and gets fmax_out = NaN.
 * Cost: a translate launch walks the history (about 2 m ceil(n / 64) dependent sweeps of one wave), a rotate launch about ten
 * sweeps -- a kernel for batches of molecules.
 * ------------------------------------------------------------------------ */
#define NNHIP_DIMER_CHECK_ONLY 1
#define NNHIP_DIMER_N_INT 9
#define NNHIP_DIMER_I_STATUS 0
#define NNHIP_DIMER_I_PHASE 1
#define NNHIP_DIMER_I_STEPS 2
#define NNHIP_DIMER_I_EVALS 3
#define NNHIP_DIMER_I_ROT 4
#define NNHIP_DIMER_I_ROT_TOTAL 5
#define NNHIP_DIMER_I_PAIRS 6
#define NNHIP_DIMER_I_HEAD 7
#define NNHIP_DIMER_I_PENDING 8
#define NNHIP_DIMER_N_FLOAT 5
#define NNHIP_DIMER_F_CURVATURE 0
#define NNHIP_DIMER_F_SLOPE 1
#define NNHIP_DIMER_F_C2 2
#define NNHIP_DIMER_F_S2 3
#define NNHIP_DIMER_F_DNORM 4
#define NNHIP_DIMER_N_VEC 9
#define NNHIP_DIMER_V_CENTER 0
#define NNHIP_DIMER_V_MODE 1
#define NNHIP_DIMER_V_F0 2
#define NNHIP_DIMER_V_F1 3
#define NNHIP_DIMER_V_THETA 4
#define NNHIP_DIMER_V_THETA_ROT 5
#define NNHIP_DIMER_V_G_OLD 6
#define NNHIP_DIMER_V_X_PREV 7
#define NNHIP_DIMER_V_F_PREV 8
int nnhip_dimer_step(const float* pos_in, const float* force, const float* energy, const uint8_t* free_mask, const int32_t* mol_ptr,
                     int32_t n_mol, int32_t n_atoms, int32_t memory, float delta, float rot_tol, int32_t max_rotations, float tol2,
                     float alpha, float maxstep, int32_t flags, int32_t* istate, float* fstate, float* vstate, float* S, float* Y,
                     float* rho, float* work, float* pos_out, float* fmax_out, float* energy_out, void* stream);

/* --------------------------------------------------------------------------
 * Nudged elastic band on the device (csrc/neb.hip): ONE launch on `stream` moves every band of a batch by one FIRE step on its NEB
 * forces, from the forces and energies just evaluated.  Improved tangent (Henkelman and Jonsson 2000), one spring constant,
 * climbing image (Henkelman, Uberuaga and Jonsson 2000), FIRE as ase.optimize.FIRE states it (mass 1, one step length per band).
 * One workgroup per band, its images dealt to the waves; per-image sums are lane-local in atom order plus a fixed butterfly, band
 * sums go through one LDS slot per image and are added in image order: no float atomics, a band's outputs are bitwise independent
 * of the rest of the batch and of its place in it.  All arithmetic in fp32, every operation one rounding (tests/neb_ref.py).
 *
 * Layout: band k owns the consecutive molecules band_ptr[k] .. band_ptr[k+1] - 1, its images in path order (int32 [K+1], on the
 * device; band_ptr_host is the same array in host memory, for the checks below); mol_ptr int32 [B+1] gives each image's atoms.  All
 * images of a band have the same atom count; bands may differ in atom count and in image count (3 .. NNHIP_NEB_MAX_IMAGES).  The
 * first and the last image of a band are endpoints and never move.
 * State of band k (device arrays of the caller, zero before the first step):  converged[k], climbing[k] (both sticky), n_steps[k],
 * n_pos[k]  int32 [K] each;  dt[k], a[k]  fp32 [K] (set from dt_start / a_start in the band's first step);  vel fp32 [N][3].
 * Per launch: pos_in, force [N,3]; energy [B]; free_mask uint8 [N] (0 = fixed atom) or NULL; spring (eV/A^2); tol2 = fl32(fmax^2);
 * climb2 = fl32(climb_below^2); the FIRE constants dt_start, dt_max, n_min, f_inc, f_dec, a_start, f_a, maxstep (ASE: 0.1, 1.0, 5,
 * 1.1, 0.5, 0.1, 0.99, 0.2); flags.  Outputs: pos_out, neb_force_out, tangent_out [N,3]; fmax_out [K]; saddle_out int32 [K].
 *
 * One launch for band k (f = force of free atoms, exactly 0 for fixed ones; a fixed atom is in no sum and never moves):
 *   1. Tangent of interior image i:  t+ = R_{i+1} - R_i,  t- = R_i - R_{i-1}  (fp32 differences of the stored positions, no minimum
 *      image).  E_{i+1} > E_i > E_{i-1}: tau = t+;  E_{i+1} < E_i < E_{i-1}: tau = t-;  otherwise, with a = max(|E_{i+1} - E_i|,
 *      |E_{i-1} - E_i|) and b the min:  tau = a t+ + b t-  if E_{i+1} > E_{i-1}, else  b t+ + a t-.  that = tau / |tau| (0 when
 *      tau.tau == 0: the image gets its plain force).  tangent_out = that (endpoints: 0).
 *   2. NEB force  F_i = f_i - (f_i.that) that + spring (|t+| - |t-|) that.  The climbing image is the interior image of highest
 *      energy, the lowest index at a tie; saddle_out[k] = its molecule index.  When climbing[k] was set BEFORE the launch it gets
 *      F = f - 2 (f.that) that instead.  neb_force_out = F (endpoints: 0).  fmax_out[k] = sqrt(fmax2), fmax2 = max |F|^2 over the
 *      free atoms of the interior images.
 *   3. Flags (never with NNHIP_NEB_CHECK_ONLY, never for a band converged before):  with NNHIP_NEB_CLIMB, climbing[k] is set when
 *      fmax2 < climb2 and takes effect from the next launch;  converged[k] is set when fmax2 < tol2 and either NNHIP_NEB_CLIMB is
 *      absent or climbing[k] was set before this launch.
 *   4. Frozen when converged before, converging now, or NNHIP_NEB_CHECK_ONLY:  pos_out = pos_in bitwise; vel, dt, a, n_pos, n_steps
 *      untouched.
 *   5. Otherwise one FIRE step over the whole band.  First step (n_steps == 0): v = 0, dt = dt_start, a = a_start, n_pos = 0 and P
 *      is not tested.  Else P = sum F.v;  P > 0:  v = (1 - a) v + a |v| F / |F|, then if n_pos > n_min: dt = min(dt f_inc, dt_max),
 *      a = a f_a;  n_pos += 1.   P <= 0:  v = 0, a = a_start, dt = dt f_dec, n_pos = 0.   Then v += dt F;  dr = dt v;  if |dr| over
 *      the band > maxstep:  dr *= maxstep / |dr|;  pos_out = pos_in + dr (endpoints and fixed atoms: pos_in bitwise); n_steps += 1.
 * The energies enter only comparisons and differences of neighbouring images, so their absolute size costs no precision here.
 * A band whose images differ in atom count, whose offsets leave the arrays or whose state words no step can have left behind
 * (n_steps < 0; after the first step n_pos < 0, dt <= 0 or a <= 0, or NaN) is not touched and gets fmax_out = NaN.
 * NNHIP_E_INVALID, nothing launched: pos_out overlapping pos_in (the reason is given at nnhip_md_step), NULL mandatory pointers,
 * unknown flag bits, a band of fewer than 3 or more than NNHIP_NEB_MAX_IMAGES images (from band_ptr_host, which must run from 0 to
 * n_mol), n_min < 0, any other parameter <= 0 or NaN.  n_bands == 0 is success without a launch.
 * ------------------------------------------------------------------------ */
#define NNHIP_NEB_CHECK_ONLY 1
#define NNHIP_NEB_CLIMB 2
#define NNHIP_NEB_MAX_IMAGES 64
int nnhip_neb_step(const float* pos_in, const float* force, const float* energy, const uint8_t* free_mask, const int32_t* mol_ptr,
                   const int32_t* band_ptr, const int32_t* band_ptr_host, int32_t n_bands, int32_t n_mol, int32_t n_atoms,
                   float spring, float tol2, float climb2, float dt_start, float dt_max, int32_t n_min, float f_inc, float f_dec,
                   float a_start, float f_a, float maxstep, int32_t flags, int32_t* converged, int32_t* climbing, int32_t* n_steps,
                   int32_t* n_pos, float* dt, float* a, float* vel, float* pos_out, float* neb_force_out, float* tangent_out,
                   float* fmax_out, int32_t* saddle_out, void* stream);

/* --------------------------------------------------------------------------
 * Replica exchange (parallel tempering) on the device (csrc/remd.hip): ONE launch on `stream` attempts every neighbouring pair of
 * one parity in every temperature ladder of a batch, from the energies just evaluated, and swaps the temperatures of an accepted
 * pair in place.  One workgroup of four waves per ladder, the ladders by a grid-stride loop; thread k decides pair k and posts the
 * new rank and velocity scale of its two slots in LDS, one barrier reached by every thread follows (a skipped ladder skips the
 * work, never the barrier), then all 256 threads walk the ladder's atoms.  No float atomics, no communication between workgroups: a
 * ladder's outputs are bitwise independent of the rest of the batch and of its place in it.  Every float operation is one
 * rounding (tests/remd_ref.py restates the launch bitwise).
 *
 * Layout: ladder g owns the consecutive molecules ladder_ptr[g] .. ladder_ptr[g+1] - 1, its SLOTS: replicas of one system, all of
 * the same atom count (int32 [G+1], on the device; ladder_ptr_host and mol_ptr_host are the same arrays in host memory, for the
 * checks below); mol_ptr int32 [B+1] gives each slot's atoms.  Ladders may differ in atom count and in length R_g
 * (2 .. NNHIP_REMD_MAX_REPLICAS).  Every per-slot and per-pair array has B entries; entry ladder_ptr[g] + k belongs to slot k, rank
 * k or pair (k, k + 1) of ladder g, and the last per-pair entry of a ladder is unused.
 * State (device arrays of the caller):  rank_of_slot, slot_of_rank int32 [B], relative to the ladder and inverse permutations of
 * each other (rank = index into the ladder's temperatures; both the identity at the start);  vel fp32 [N][3];  sigma fp32 [N], the
 * Langevin sigma nnhip_md_step reads;  n_attempt, n_accept int32 [B], per pair, accumulated.
 * Per launch:  energy fp32 [B] (read only);  stream_id int32 [G], the bits of a uint32: the ladder's identity for the random
 * stream, NOT its position in the batch;  dbeta fp32 [B] = fl32(1 / (k_B T_k) - 1 / (k_B T_{k+1}));  scale_up, scale_down fp32 [B]
 * = fl32(sqrt(T_{k+1} / T_k)), fl32(sqrt(T_k / T_{k+1})) (all three formed in fp64 on the host and rounded once);  sigma_table fp32
 * [n_rows][N]: row k holds every atom's sigma at rank k of its ladder (fixed atoms: 0 in every row);  attempt, the bits of a
 * uint32, and seed, the bits of a uint64 (the header's vocabulary has signed scalars only).  Optional outputs (NULL: not written)
 * delta_out, u_out fp32 [B] and accepted_out int32 [B], per pair.
 *
 * One launch for ladder g of R slots:
 *   1. Pairs attempted: with p = attempt & 1, the pairs (k, k + 1) for k = p, p + 2, ... < R - 1.  They are disjoint: no two
 *      decisions touch the same slot.
 *   2. Pair k, with a = slot_of_rank[k] and b = slot_of_rank[k + 1]:  dE = E_a - E_b and delta = dbeta_k dE, one rounding each.
 *   3. (w0, w1, w2, w3) = Philox4x32-10 with counter (attempt, stream_id[g], k, 0) and key (seed low word, seed high word);
 *      u = float(w0 >> 8) 2^-24: exact in fp32, in [0, 1).
 *   4. Accepted iff  delta >= 0 || u < expf(delta).  A NaN delta rejects, a tie (delta == 0) accepts.  n_attempt[k] += 1 and
 *      n_accept[k] += accepted;  delta_out[k] = delta, u_out[k] = u, accepted_out[k] = 0 / 1.  The entries of pairs NOT attempted in
 *      this launch (the other parity, the unused last entry) get 0 in all three.
 *   5. Accepted:  rank_of_slot[a] = k + 1, rank_of_slot[b] = k, slot_of_rank[k] = b, slot_of_rank[k + 1] = a;  every vel component
 *      of slot a is multiplied by scale_up_k and every one of slot b by scale_down_k, one rounded product each;  sigma[i] =
 *      sigma_table[new rank][i] for the atoms of both slots: a copy, so sigma never drifts.  positions and forces are not arguments.
 *   6. A slot that is not swapped keeps every bit of its vel, sigma and map entries.
 * Skipped on the device: a ladder whose rank maps are not inverse permutations of each other (or whose slots differ in atom count
 * in mol_ptr) gets delta_out = NaN and accepted_out = 0 in all its entries and nothing else of it is written (u_out neither); a
 * ladder whose device offsets leave the arrays is not touched at all.
 * NNHIP_E_INVALID, nothing launched: NULL mandatory pointers (everything but the three optional outputs), negative counts,
 * ladder_ptr_host not running from 0 to n_mol (or a ladder leaving the batch on the way) or mol_ptr_host not from 0 to n_atoms, a
 * ladder of fewer than 2 or more than NNHIP_REMD_MAX_REPLICAS slots, n_rows below the longest ladder, slots of one ladder with
 * unequal atom counts.  n_ladders == 0 with n_mol == 0 is success without a launch.
 * The energies enter one difference of two slots of one ladder: delta is resolved to one fp32 ulp of |E| times dbeta.
 * ------------------------------------------------------------------------ */
#define NNHIP_REMD_MAX_REPLICAS 64
int nnhip_remd_exchange(const float* energy, const int32_t* mol_ptr, const int32_t* mol_ptr_host, const int32_t* ladder_ptr,
                        const int32_t* ladder_ptr_host, const int32_t* stream_id, const float* dbeta, const float* scale_up,
                        const float* scale_down, const float* sigma_table, int32_t* rank_of_slot, int32_t* slot_of_rank, float* vel,
                        float* sigma, int32_t* n_attempt, int32_t* n_accept, float* delta_out, float* u_out, int32_t* accepted_out,
                        int32_t attempt, int64_t seed, int32_t n_ladders, int32_t n_mol, int32_t n_atoms, int32_t n_rows,
                        void* stream);

/* --------------------------------------------------------------------------
 * Path-integral molecular dynamics on the device (csrc/pimd.hip): one launch advances every ring polymer of a batch by the second
 * half kick of one step and / or the first half of the next, in ring-polymer normal-mode coordinates.  The scheme is BAOAB with
 * the A step exact for the free ring polymer and the O step the PILE thermostat (Ceriotti, Parrinello, Markland and Manolopoulos
 * 2010); the driver is newtonnet_amd/pimd.py, a step of it  model(beads) -> nnhip_pimd_step(finish | begin).
 *
 * Layout: system g owns the n_beads = P consecutive molecules g P .. g P + P - 1 of mol_ptr (int32 [n_mol + 1], on the device;
 * mol_ptr_host: the same array in host memory, for the checks below), its SLOTS, all of one atom count n_g; n_mol = G P.  In force
 * and pos_out (fp32 [N][3], the buffers of the model) slot s holds bead s; in the state arrays u, w (fp32 [N][3], mode positions
 * and mode velocities, updated in place) slot k holds normal mode k.  Row r = mol_ptr[g P + k] + i is (slot k, atom i).
 * Tables, all formed in fp64 on the host and rounded once -- the kernel evaluates no transcendental:
 *   ctab fp32 [P][P], the orthonormal transform:  C[0][s] = 1 / sqrt(P);  C[k][s] = sqrt(2 / P) cos(2 pi s k / P) for 0 < k < P / 2;
 *     C[P/2][s] = (-1)^s / sqrt(P) (P even);  C[k][s] = sqrt(2 / P) sin(2 pi s k / P) for k > P / 2.
 *   mode_tab fp32 [n_mol][5], per (g, k), with omega_k = 2 omega_P sin(k pi / P) and h = dt / 2:
 *     a = cos(omega_k h),  b = sin(omega_k h) / omega_k (dt / 2 for k = 0),  d = -omega_k sin(omega_k h),  c1 = exp(-gamma_k dt),
 *     half_w2 = omega_k^2 / 2.
 *   hk fp32 [N] = dt / (2 m_i);  mass fp32 [N] (with est_out only);  sigma fp32 [N] = sqrt((1 - c1^2) k_B P T_g / m_i), per row;
 *   noise fp32 [N][3], standard normal, in mode space (sigma and noise: both or neither).
 *
 * Per row (mode k, atom i) and coordinate, every operation in fp32 and one rounding (tests/pimd_ref.py restates it in fp64):
 *   f_k = C[k][0] F_0;  f_k = fma(C[k][s], F_s, f_k) for s = 1 .. P - 1 ascending           (the mode force; once per launch)
 *   finish (NNHIP_PIMD_FINISH):  w = fma(hk, f_k, w);  est_out[r] = (kinetic, spring, virial, 0) when est_out != NULL:
 *     kinetic = (0.5 m) fma(wz, wz, fma(wy, wy, wx wx)),  spring = (m half_w2) fma(uz, uz, fma(uy, uy, ux ux)),
 *     virial = fma(uz, fz, fma(uy, fy, ux fx)) for k > 0 and 0 for k = 0
 *   begin (NNHIP_PIMD_BEGIN):  w = fma(hk, f_k, w);  A: (u, w) <- (fma(b, w, a u), fma(d, u, a w)), both from the old pair;
 *     O: w = fma(sigma, noise, c1 w), skipped entirely when noise == NULL;  A again;  u and w are stored;
 *     x_s = C[0][s] u_0;  x_s = fma(C[k][s], u_k, x_s) for k = 1 .. P - 1 ascending  ->  pos_out, bead s
 * With P = 1 (C = [1], a = 1, b = dth, d = 0) this is nnhip_md_step's chain, bit for bit.  finish alone writes neither u nor
 * pos_out.  est_out fp32 [N][4] is reduced per slot with nnhip_segment_sum (width 4).
 *
 * One workgroup of NNHIP_PIMD_THREADS threads per (system, tile of atoms); a tile holds NNHIP_PIMD_THREADS / P atoms (rounded down).
 * No float atomics, no communication between workgroups: a system's outputs are bitwise independent of the rest of the batch.
 * A system whose DEVICE offsets leave the arrays is not touched.
 * NNHIP_E_INVALID, nothing launched: flags outside 1 .. 3, negative counts, n_beads outside 1 .. NNHIP_PIMD_MAX_BEADS or not
 * dividing n_mol, sigma without noise or noise without sigma, est_out without finish (or without mass), mol_ptr_host not running
 * from 0 to n_atoms, slots of one system with unequal atom counts, NULL mandatory pointers (u, w, force, ctab, mode_tab, hk,
 * mol_ptr, mol_ptr_host; pos_out with begin), pos_out overlapping pos_pending -- the positions the forward call still pending read
 * (NULL: none is pending), for the reason given at nnhip_md_step.  n_atoms == 0 is success without a launch.
 * ------------------------------------------------------------------------ */
#define NNHIP_PIMD_FINISH 1
#define NNHIP_PIMD_BEGIN 2
#define NNHIP_PIMD_MAX_BEADS 64
#define NNHIP_PIMD_THREADS 256
int nnhip_pimd_step(float* u, float* w, const float* force, const float* ctab, const float* mode_tab, const float* hk,
                    const float* mass, const float* sigma, const float* noise, const int32_t* mol_ptr, const int32_t* mol_ptr_host,
                    const float* pos_pending, int32_t flags, int32_t n_beads, int32_t n_mol, int32_t n_atoms, float* pos_out,
                    float* est_out, void* stream);

/* --------------------------------------------------------------------------
 * Bias potentials on collective variables, on the device (csrc/bias.hip): ONE launch on `stream` turns the model's forces into the
 * forces of the biased potential for every molecule of a batch -- static harmonic restraints (umbrella windows) and a sum of
 * Gaussian hills shared by the walkers of a group (multiple-walker metadynamics, Raiteri et al. 2006; well-tempered heights,
 * Barducci, Bussi and Parrinello 2008) -- and, with NNHIP_BIAS_DEPOSIT, adds one hill per walker.  The driver is
 * newtonnet_amd/metadynamics.py, a step of it  model(pos) -> nnhip_bias_step -> nnhip_md_step.
 *
 * Layout: group g owns the consecutive molecules group_ptr[g] .. group_ptr[g+1] - 1, its W_g WALKERS: copies of one system, all of
 * one atom count (int32 [G+1], on the device; group_ptr_host and mol_ptr_host are the same arrays in host memory, for the checks
 * below); mol_ptr int32 [B+1] gives each walker's atoms.  Groups may differ in atom count and in W_g >= 1.
 * Tables, all formed in fp64 on the host and rounded once:
 *   cv_def int32 [B][NNHIP_BIAS_MAX_CVS][5] = (kind, a, b, c, d): the variable's kind (0 = unused) and its atoms, LOCAL to the
 *     molecule; entries beyond the kind's arity are ignored.  A group's walkers normally share their definitions.
 *   restraint fp32 [B][NNHIP_BIAS_MAX_CVS][2] = (kappa, s0): U = sum_d kappa_d (s_d - s0_d)^2 / 2; kappa = 0: none.
 *   hill_par fp32 [G][4] = (1 / sigma_0^2, 1 / sigma_1^2, w0, 1 / (k_B dT)): 1 / sigma_d^2 = 0 for an unused variable, the last
 *     entry 0 for plain metadynamics.
 *   hills fp32 [G][capacity][4], rows (c_0, c_1, height, 0), 16-byte aligned: rows 0 .. n_deposits W_g - 1 of group g are its hills.
 * Collective variables, on the positions AS STORED (unwrapped; no minimum image is taken), every operation in fp32 and one rounding
 * (tests/bias_ref.py restates the launch in fp64 with a bound):
 *   NNHIP_BIAS_DISTANCE (i, j):   s = |x_j - x_i|
 *   NNHIP_BIAS_ANGLE (i, j, k):   a = x_i - x_j, b = x_k - x_j, c = a x b;  s = atan2f(|c|, a.b) in [0, pi];
 *                                 ds/dx_i = (a x c) / (|a|^2 |c|), ds/dx_k = (c x b) / (|b|^2 |c|), ds/dx_j = -(their sum)
 *   NNHIP_BIAS_TORSION (i, j, k, l):  b1 = x_j - x_i, b2 = x_k - x_j, b3 = x_l - x_k, n1 = b1 x b2, n2 = b2 x b3;
 *                                 s = atan2f(|b2| b1.n2, n1.n2) in (-pi, pi];  Blondel and Karplus 1996:  g_i = -|b2| n1 / |n1|^2,
 *                                 g_l = |b2| n2 / |n2|^2,  with p = b1.b2 / |b2|^2, q = b3.b2 / |b2|^2 and t = q g_l - p g_i:
 *                                 g_j = t - g_i,  g_k = -(t + g_l).  A DIFFERENCE of a torsion is wrapped: delta <- delta - P rint(
 *                                 delta / P) with P = fl32(2 pi).
 *   An unused variable has s = 0 and no gradient.  Where a gradient is undefined (|r| = 0, |a x b| = 0, |n1| = 0 or |n2| = 0, or any
 *   row of it not finite) the variable contributes NO force and bit d of status_out[b] is set; its value still enters V and U.
 * One launch for molecule b = walker j of group g, with H = n_deposits W_g:
 *   1. delta_hd = s_d - c_hd (wrapped for a torsion);  a_hd = delta_hd / sigma_d^2;  e_h = a_h0 delta_h0 + a_h1 delta_h1;
 *      t_h = height_h expf(-e_h / 2);  V = sum_{h < H} t_h,  G_d = sum_h t_h a_hd  (= -dV/ds_d).  Thread t adds the hills t, t + 256,
 *      ... in ascending order; the partial sums go through a fixed tree (wave butterfly, then the four waves in order).
 *   2. r_d = s_d - s0_d (wrapped for a torsion);  U = sum_d (kappa_d r_d) r_d / 2;  c_d = kappa_d r_d - G_d.
 *   3. force_out[a] = force_in[a] - sum_d c_d ds_d/dx_a.  An atom in no variable, and any component whose bias part is exactly 0,
 *      is a bitwise copy of force_in; a molecule without variables is a pure copy.
 *   4. cv_out[b] = (s_0, s_1);  bias_out[b] = (V, U);  status_out[b] = the bits above.
 *   5. With NNHIP_BIAS_DEPOSIT: hills[g][H + j] = (s_0, s_1, w0 expf(-V / (k_B dT)), 0), V the bias BEFORE any deposit of this
 *      launch.  The rows written are exactly the rows no workgroup reads in this launch, and the count is a host integer: no
 *      race, no counter on the device, no atomics, no host read.
 * One workgroup of NNHIP_BIAS_THREADS threads per molecule, the molecules by a grid-stride loop; every thread forms the variables
 * and their gradient rows itself (the same bits in every thread, no communication).  No float atomics: a group's outputs depend
 * neither on the other groups of the batch nor on the group's place in it.
 * State words no driver can leave behind -- a kind outside 0 .. 3, an atom index outside the molecule, hills that would leave the
 * capacity by the DEVICE's group_ptr -- make the kernel copy that molecule's forces unchanged and set NNHIP_BIAS_STATUS_INVALID
 * (cv_out and bias_out get 0, no hill is written); a molecule whose device offsets leave the arrays is not touched at all.
 * NNHIP_E_INVALID, nothing launched: NULL mandatory pointers (everything but stream), force_out overlapping force_in or pos, hills
 * not 16-byte aligned, negative counts, group_ptr_host not running from 0 to n_mol or mol_ptr_host not from 0 to n_atoms, an empty
 * group, walkers of one group with unequal atom counts, n_deposits < 0, (n_deposits + (deposit ? 1 : 0)) W_g > capacity, unknown
 * flag bits.  n_mol == 0 is success without a launch.
 *
 * nnhip_bias_eval: V of group `group` at n_points given points (fp32 [n_points][2]), through the same hill sum as step 1 (one
 * workgroup per point), over the first n_hills rows; period0 / period1: the period of each coordinate (fl32(2 pi) for a torsion,
 * 0 for none).  v_out fp32 [n_points].  Refused: NULL pointers, negative counts, group outside 0 .. n_groups - 1, n_hills > capacity,
 * a negative or non-finite period.
 * ------------------------------------------------------------------------ */
#define NNHIP_BIAS_MAX_CVS 2
#define NNHIP_BIAS_DISTANCE 1
#define NNHIP_BIAS_ANGLE 2
#define NNHIP_BIAS_TORSION 3
#define NNHIP_BIAS_DEPOSIT 1
#define NNHIP_BIAS_THREADS 256
#define NNHIP_BIAS_STATUS_INVALID 4
int nnhip_bias_step(const float* pos, const float* force_in, const int32_t* mol_ptr, const int32_t* mol_ptr_host,
                    const int32_t* group_ptr, const int32_t* group_ptr_host, const int32_t* cv_def, const float* restraint,
                    const float* hill_par, float* hills, int32_t capacity, int32_t n_deposits, int32_t flags, int32_t n_groups,
                    int32_t n_mol, int32_t n_atoms, float* force_out, float* cv_out, float* bias_out, int32_t* status_out,
                    void* stream);
int nnhip_bias_eval(const float* hills, const float* hill_par, const float* points, float period0, float period1, int32_t group,
                    int32_t capacity, int32_t n_hills, int32_t n_points, int32_t n_groups, float* v_out, void* stream);

/* --------------------------------------------------------------------------
 * Product form of the dense kernels.  1 (default): the 128x128 linears of the hot path (edge MLPs, node MLPs, equiv_update
 * and their adjoints / tangents, SiLU models) form each fp32 product from two scaled f16 pieces per operand on
 * v_mfma_f32_32x32x16_f16 with fp32 accumulation (csrc/mlp128s.hip, node128s.hip); 0 (environment NNHIP_MLP_SPLIT=0,
 * read once per process): v_mfma_f32_32x32x2_f32 everywhere.  Inputs, outputs and accumulators are fp32 either way.
 * ------------------------------------------------------------------------ */
int nnhip_split_products(void);
/* Which forms the fused edge-MLP launches of a large batch take (what bench.py prices its byte model with):
 *   bit 0  split-f16 products (nnhip_split_products)
 *   bit 1  the two-MLP adjoint launches run in the one-pass register-weights kernel (mlp_regw_kernel)
 *   bit 2  ... the two-MLP forward launches too
 *   bit 3  the single-MLP adjoint (layer 0) runs in mlp_regw_kernel        bit 4  ... the single-MLP forward too */
int nnhip_mlp_forms(void);
/* Every form choice the library makes in this process -- neighbor-list builder thresholds, waves per receiver row, the
 * molecule-per-workgroup forms and their thresholds, the edge-MLP forms, the fused edge phase -- as one JSON object written into
 * buf (NUL-terminated; NNHIP_E_INVALID when n is too small: 2048 bytes are plenty), with the NNHIP_* environment switches that are
 * set.  For bench lines and for tests that pin non-default forms; the reference has no counterpart (one eager path,
 * newtonnet/models/newtonnet.py:74-104). */
int nnhip_config(char* buf, size_t n);

/* --------------------------------------------------------------------------
 * Internal spatial order of ONE big system (csrc/graph.hip, round 6).  The reference evaluates the atoms in the caller's order
 * (newtonnet/layers/representations.py:74-98 over one molecule); the step of a molecule of >= 16 384 atoms runs on the atoms in Morton
 * order of cells of max(cutoff, extent / 64) and hands everything back in the caller's order (newtonnet_amd/models/newtonnet.py).
 *   nnhip_spatial_order: perm[k] = input index of the atom at position k, inv = its inverse (int32 [N] each), and -- optional -- z / pos
 *     gathered through perm; deterministic (by cell key, then by input index); scratch of nnhip_spatial_order_scratch_bytes(N).
 *   nnhip_permute_rows: out[k] = x[idx[k]] for rows of `width` floats (per-atom results back: idx = inv).
 *   nnhip_edge_index_unpermute: the [2][E] int64 list of the permuted CSR (row_ptr_p, col_p) as the reference lists it for the caller's
 *     order -- rows by ascending i, neighbors by ascending j; scratch of (N + 1 + N / 1024 + 2) ints.
 * ------------------------------------------------------------------------ */
size_t nnhip_spatial_order_scratch_bytes(int32_t n_atoms);
int nnhip_spatial_order(const float* pos, const int64_t* z, int32_t n_atoms, float cutoff, int32_t* perm, int32_t* inv,
                        int64_t* z_out, float* pos_out, void* scratch, void* stream);
int nnhip_permute_rows(const float* x, const int32_t* idx, int32_t n_rows, int32_t width, float* out, void* stream);
int nnhip_edge_index_unpermute(const int32_t* row_ptr_p, const int32_t* col_p, const int32_t* perm, const int32_t* inv,
                               int32_t n_atoms, int32_t n_edges, int64_t* edge_index, int32_t* scratch, void* stream);

/* --------------------------------------------------------------------------
 * Constant-pressure molecular dynamics on the device (csrc/npt.hip): isotropic stochastic cell rescaling (Bernetti & Bussi, J. Chem.
 * Phys. 153, 114107 (2020)) as a first-order (Euler) step S for eps = ln V inside nnhip_md_step's BAOAB step:
 *   B(F_k) [full-step v, KE] B(F_k) S A O A,   then the model at the new positions with the new cell.
 * TWO launches on `stream` between two force evaluations: nnhip_npt_barostat forms every system's scale factor, nnhip_npt_step is
 * nnhip_md_step with S applied.  All in fp32; every line below is ONE rounding to nearest (an fma rounds once) unless it says
 * otherwise (tests/npt_ref.py restates both chains in fp64):
 *
 * nnhip_npt_barostat: one 256-thread workgroup per system b = 0 .. n_mol - 1, atoms mol_ptr[b] .. mol_ptr[b+1] - 1 (int32 [n_mol+1],
 * clamped to [0, n_atoms]).  Thread t takes the atoms t, t + 256, ... of the system in that order:
 *     v'   = fma(hk_i, F_ik, v_ik)          the pending second half kick;  force == NULL: none is pending, v' = v (no rounding).
 *                                           v' is NOT stored: nnhip_npt_step's finish forms the same bits
 *     s    = vx' vx';  s = fma(vy', vy', s);  s = fma(vz', vz', s);  ke_i = (0.5 mass_i) s     nnhip_md_step's ke_out chain
 *     acc  = acc + ke_i                                                                        (acc = 0 at the start)
 *   The 256 partial sums meet in a fixed LDS tree: for d = 128, 64, ..., 1 thread t < d adds the partial of t + d to its own.  No
 *   float atomics: K_b is bitwise repeatable for any system size, 0 (K = 0) and > 256 included.  Then one thread, with c = cell_in[b]
 *   (row-major [3][3]) and W = virial[b] (= -dE/d strain at the current geometry):
 *     m0   = fma(c11, c22, -(c12 c21));  m1 = fma(c10, c22, -(c12 c20));  m2 = fma(c10, c21, -(c11 c20))     (each product one rounding)
 *     V    = fma(c02, m2, fma(-c01, m1, c00 m0))                                               = det(cell)
 *     P    = fma(2, K, (W00 + W11) + W22) / (3 V)                                              two sums, the fma, 3 V, the quotient
 *     deps = fma(-a_b, P0_b - P, sqrt(s2_b / V) noise_b)                                       with noise: quotient, root, product, fma
 *     deps = (-a_b) (P0_b - P)                                                                 noise == NULL (s2 == NULL too)
 *            a_b == 0 with noise == NULL: system b is not coupled, deps = +0 whatever P is (a cell of zeros included)
 *     e    = deps fl32(1/3);  mu = expf(e);  inv_mu = expf(-e);  cell_out[b] = mu c            (nine products)
 *   a_b = beta_T dt / tau_p (per pressure unit), P0_b the target pressure, s2_b = 2 k_B T_b beta_T dt / tau_p (energy), noise_b ~
 *   N(0,1); pressures in energy / length^3.  Written: cell_out [n_mol][3][3], mu, inv_mu, and the records ke (= K), pressure (= P),
 *   volume (= V), deps, all [n_mol].  expf(+-0) = 1 exactly, and a product with 1.0f is exact: a_b = 0 without noise gives
 *   mu = inv_mu = 1.0f and cell_out[b] == cell_in[b] bit for bit.
 *   Roundings that are NOT half an ulp: expf, 2 ulp taken (0.836 ulp measured on an MI355X over 2^22 arguments, tools/probes/
 *   math_ulp_probe.hip; |e| < 1 here); the root, 2 ulp taken (gfx950 has no correctly rounded fp32 root:
 *   0.916 ulp measured, same probe).  The quotients are correctly rounded (0.5 ulp measured, same probe).
 *   cell_out may NOT overlap cell_in (NNHIP_E_INVALID, nothing is launched), for the reason given at nnhip_md_step: the deferred
 *   forward call queued on cell_in may have to be repeated from it.  NULL vel, mass, mol_ptr, cell_in, virial, a, p0 or any output,
 *   force without hk, or s2 and noise not both given / both NULL: NNHIP_E_INVALID.  n_mol == 0: success, nothing is launched.
 *
 * nnhip_npt_step: nnhip_md_step's launch shape, flags and chain with S between the begin kick and the first half drift; b =
 * mol_of_atom[i] (int32 [N], read with BEGIN only):
 *   finish (NNHIP_MD_FINISH):  v = fma(hk_i, F_ik, v);  ke_out[i] as nnhip_md_step                       [only when ke_out != NULL]
 *   begin  (NNHIP_MD_BEGIN):   v = fma(hk_i, F_ik, v);  x = mu_b pos_in;  v = inv_mu_b v;  x = fma(dth, v, x);
 *                              v = fma(sigma_i, noise_ik, c1 v) [skipped when noise == NULL];  pos_out = fma(dth, v, x)
 *   With every mu = inv_mu = 1 these are nnhip_md_step's bits (a product with 1.0f is exact).  Same aliasing rule (pos_out may NOT
 *   overlap pos_in), same NULL rules (plus mu, inv_mu [n_mol] and mol_of_atom with BEGIN), sigma and noise both given or both NULL,
 *   ke_out needs FINISH and mass, n_atoms == 0: success without a launch.  An atom whose mol_of_atom lies outside [0, n_mol) is
 *   left untouched by a BEGIN launch (no table is read outside its bounds).
 * ------------------------------------------------------------------------ */
int nnhip_npt_barostat(const float* vel, const float* force, const float* hk, const float* mass, const int32_t* mol_ptr,
                       int32_t n_mol, int32_t n_atoms, const float* cell_in, const float* virial, const float* a, const float* p0,
                       const float* s2, const float* noise, float* cell_out, float* mu, float* inv_mu, float* ke, float* pressure,
                       float* volume, float* deps, void* stream);
int nnhip_npt_step(const float* pos_in, float* vel, const float* force, const float* hk, const float* mass, const float* sigma,
                   const float* noise, const float* mu, const float* inv_mu, const int32_t* mol_of_atom, int32_t n_mol, float dth,
                   float c1, int32_t flags, int32_t n_atoms, float* pos_out, float* ke_out, void* stream);

/* --------------------------------------------------------------------------
 * Batched phonon dispersion of crystals (csrc/phonon.hip): the dynamical matrix D(q) of every (crystal, wave vector) pair
 * assembled and diagonalised in ONE launch; a problem has d = 3 n_b coordinates (n_b atoms of the primitive cell).
 *   fc / fc_ptr [n_cry]: force constants Phi(i, J) = d^2 E / d r_i d r_J of the home atoms i against the N_b atoms J of a
 *     supercell, fp32 [n_b][3][N_b][3] per crystal at fc + fc_ptr[b]; J = R n_b + j is copy R of home atom j, the home cell first.
 *   cry_ptr [n_cry + 1] (device) / cry_ptr_host (host, identical): home-atom offsets; sc_atoms [n_cry]: N_b (a multiple of n_b).
 *   img_ptr [n_cry], img_start, img_off: the image table.  Pair (i, J) of crystal b owns the rows
 *     img_start[img_ptr[b] + i N_b + J] .. img_start[img_ptr[b] + i N_b + J + 1] - 1 of img_off [.][3] (fp64): the m_iJ equally near
 *     supercell-lattice images of J seen from i, each as r_J + T - r_i in units of the PRIMITIVE lattice vectors.
 *   masses [n_home] (amu; null: unit masses), q [n_q][3] fp64: wave vectors in units of the primitive reciprocal vectors, shared
 *     by all crystals.  out_ptr [n_cry]: sum of d^2 over the crystals before b.
 *   D_ij(q) = (m_i m_j)^-1/2 sum_J Phi(i, J) (1 / m_iJ) sum_T exp(2 pi i q . x_T), J over the copies of j, then (D + D^H) / 2.  The
 *     phase product is formed in fp64 and reduced to [-1/2, 1/2] before the sine and cosine; every sum has a fixed order.
 *   Complex Hermitian cyclic Jacobi in LDS, round-robin ordering, until off(A) <= 2^-24 ||A||_F or 30 sweeps (the rule and the
 *     status bits of nnhip_eig_blocks: bit 0 sweep cap, bit 1 cry_ptr gives the crystal more atoms than cry_ptr_host did, bit 2 a
 *     mass that is not positive and finite; with bit 1 or 2 nothing of the problem is written).
 *   evals: [n_q][d] per crystal at n_q 3 cry_ptr[b], ascending per (b, q).  modes (may be null: the eigenvalues keep every bit):
 *     complex64 (re, im) [n_q][d][d] per crystal at 2 n_q out_ptr[b] floats, ROW k = mode k, unit norm, the component of largest
 *     magnitude real and positive (lowest index on a tie).  dmat (may be null): D(q) itself, laid out like modes.
 *     sweeps / status: [n_cry][n_q].
 * A crystal with d <= 32 gives each problem one wave (four problems per workgroup), a larger one a whole workgroup; the result of
 * a (b, q) does not depend on that, nor on the other problems of the launch.  No float atomics: bitwise repeatable.
 * Checked from cry_ptr_host BEFORE any launch: NNHIP_E_UNSUPPORTED above nnhip_phonon_max_dim (96: 32 atoms; A and the modes of a
 * problem take 16 d (d + 1) bytes of the 160 KiB of LDS), the message names the bound and the crystal; nnhip_phonon_bands_large
 * below serves larger crystals.
 *   nnhip_phonon_dos: density of states of values [val_ptr[b], val_ptr[b + 1]) per crystal over n_bins equal bins of [lo, hi]: one
 *     thread per bin walks the values in order.  counts (int32 [n_cry][n_bins], may be null): the histogram, integers only
 *     (a value equal to hi falls into the last bin, values outside are not counted).  density (fp32 [n_cry][n_bins], may be null;
 *     needs width > 0): sum over the values of the unit Gaussian of standard deviation `width` at the bin centre, summed in fp64.
 * ------------------------------------------------------------------------ */
int nnhip_phonon_max_dim(void);
int nnhip_phonon_bands(const float* fc, const int64_t* fc_ptr, const int32_t* cry_ptr, const int32_t* cry_ptr_host,
                       const int32_t* sc_atoms, const int64_t* img_ptr, const int32_t* img_start, const double* img_off,
                       const float* masses, const int64_t* out_ptr, int32_t n_cry, const double* q, int32_t n_q, float* evals,
                       float* modes, float* dmat, int32_t* sweeps, int32_t* status, void* stream);
int nnhip_phonon_dos(const float* values, const int64_t* val_ptr, int32_t n_cry, float lo, float hi, int32_t n_bins, float width,
                     int32_t* counts, float* density, void* stream);

/* --------------------------------------------------------------------------
 * The same dispersion above nnhip_phonon_max_dim (csrc/phonon_large.hip), opt-in: a two-sided BLOCK Jacobi for the complex Hermitian
 * D(q) spread over many workgroups by kernel boundaries (no cooperative launch, no grid barrier, no spin-wait), D(q) and the modes of
 * every (crystal, q) problem in the caller's workspace.  Arguments, layouts, stopping rule and status bits as nnhip_phonon_bands; an
 * element of D(q) is formed by the same device functions, so dmat is bitwise that of nnhip_phonon_bands where both serve a crystal.
 *   select_host [n_cry] (host, may be null = all): the crystals to compute; nothing of another crystal is touched in any output.
 *   ws / ws_bytes: device workspace, 256-byte aligned, at least nnhip_phonon_large_ws_bytes(cry_ptr_host, n_cry, n_q, modes != null,
 *     select_host): about 16 Mp^2 bytes per problem with modes, 8 Mp^2 without, Mp = d rounded up to a multiple of 64
 *     (NNHIP_E_WORKSPACE).  A caller short of memory splits the wave vectors over several calls: a problem's result does not depend
 *     on the other problems of the call.
 * Checked from cry_ptr_host BEFORE any launch, for the selected crystals: NNHIP_E_UNSUPPORTED above nnhip_phonon_large_max_dim (768:
 * 256 atoms -- the size the accuracy bound has been verified at), the message names the bound and the crystal.  The host reads one
 * done flag per problem once per sweep (a stream synchronisation per sweep).  No float atomics: bitwise repeatable; modes == null
 * leaves the eigenvalues bitwise the same.
 * ------------------------------------------------------------------------ */
int nnhip_phonon_large_max_dim(void);
size_t nnhip_phonon_large_ws_bytes(const int32_t* cry_ptr_host, int32_t n_cry, int32_t n_q, int32_t want_modes,
                                   const uint8_t* select_host);
int nnhip_phonon_bands_large(const float* fc, const int64_t* fc_ptr, const int32_t* cry_ptr, const int32_t* cry_ptr_host,
                             const int32_t* sc_atoms, const int64_t* img_ptr, const int32_t* img_start, const double* img_off,
                             const float* masses, const int64_t* out_ptr, int32_t n_cry, const double* q, int32_t n_q, float* evals,
                             float* modes, float* dmat, int32_t* sweeps, int32_t* status, const uint8_t* select_host, void* ws,
                             size_t ws_bytes, void* stream);

/* --------------------------------------------------------------------------
 * Phonon group velocities (csrc/phonon_velocity.hip): d lambda / d q_cart and the velocity of every mode of every (crystal, q) problem
 * in ONE launch, from the eigenpairs nnhip_phonon_bands / nnhip_phonon_bands_large wrote (either: the layouts are the same).
 *   fc .. out_ptr, n_cry, q, n_q: as nnhip_phonon_bands takes them.  cells [n_cry][3][3] fp64 (device): the primitive lattice vectors
 *     as rows, A.  direction [n_q][3] fp64 (device, may be null): the unit Cartesian direction n of each q, shared by all crystals;
 *     null: q_cart / |q_cart| of each crystal, q_cart = 2 pi q @ inv(cell)^T, and (1, 0, 0) at q = 0.
 *   evals, modes: inputs, as nnhip_phonon_bands writes them.  deg_tol, zero_tol [n_cry]: absolute, eV/(A^2 amu).
 *   G_a,ij = dD_ij/dq_cart,a = (m_i m_j)^-1/2 sum_J Phi(i, J) (1 / m_iJ) sum_T (i r_a) exp(2 pi i q . x_T), r = x_T @ cell, then
 *     (G_a + G_a^H) / 2: D's own sums (fp64 phase, copies ascending, fmaf) with one more factor per image.
 *   Consecutive eigenvalues no more than deg_tol[b] apart form a group.  A group of one: dlam_a = Re e^H G_a e.  A group of g <= 16:
 *     M_a = V^H G_a V, M_n = sum_a n_a M_a diagonalised (the Jacobi of nnhip_phonon_bands, eigenvalues ascending), and the group's
 *     modes, in that order, take dlam_a = Re diag(U^H M_a U).  Inside a subgroup M_n leaves degenerate only the trace is invariant.
 *   vel [.][3], laid out like evals x 3: dlam_a / (2 sqrt|lambda|), the derivative of sign(lambda) sqrt|lambda|, in sqrt(eV/amu)
 *     (x 98.227 = A/ps); zero where |lambda| <= zero_tol[b] (defined = 0: the limit depends on the direction).  dlam (may be null):
 *     d lambda / d q_cart, eV/(A amu).  group (may be null): per mode, the index of the first mode of its group.  defined: per mode.
 *   status [n_cry][n_q]: bits 1 and 2 of nnhip_phonon_bands (nothing else of the problem is written); bit 3
 *     (NNHIP_PHONON_STATUS_GROUP): a group above 16 modes -- its modes get zero, defined = 0; bit 4 (NNHIP_PHONON_STATUS_NONFINITE): a
 *     non-finite eigenvalue or mode -- nothing of the problem is written beyond defined = 0.
 * One workgroup per (crystal, q, tile of modes: all of them up to d = 96, 64 above); no workspace; every d up to
 * nnhip_phonon_large_max_dim, checked from cry_ptr_host BEFORE any launch (NNHIP_E_UNSUPPORTED).  Every sum has a fixed order, no float
 * atomics, one writer per output: a problem's result is bitwise repeatable and does not depend on the rest of the launch.
 * Measured against fp64 (tests/test_hip_phonon_velocities.py): see DESIGN.md section 23b.
 * ------------------------------------------------------------------------ */
#define NNHIP_PHONON_STATUS_GROUP 8
#define NNHIP_PHONON_STATUS_NONFINITE 16
int nnhip_phonon_velocities(const float* fc, const int64_t* fc_ptr, const int32_t* cry_ptr, const int32_t* cry_ptr_host,
                            const int32_t* sc_atoms, const int64_t* img_ptr, const int32_t* img_start, const double* img_off,
                            const float* masses, const int64_t* out_ptr, int32_t n_cry, const double* cells, const double* q,
                            int32_t n_q, const double* direction, const float* evals, const float* modes, const float* deg_tol,
                            const float* zero_tol, float* vel, float* dlam, int32_t* group, uint8_t* defined, int32_t* status,
                            void* stream);

/* --------------------------------------------------------------------------
 * Strain slopes of phonon eigenvalues and mode Grueneisen parameters (csrc/phonon_gruneisen.hip): d lambda / d eta_k = e^H (dD/d eta_k) e
 * of every mode of every (crystal, q) problem and every strain plane k in ONE launch, from the eigenpairs nnhip_phonon_bands /
 * nnhip_phonon_bands_large wrote.
 *   fc_ptr .. out_ptr, n_cry, q, n_q, evals, modes, deg_tol, zero_tol: as nnhip_phonon_velocities takes them (cells and direction are
 *     not taken).  In place of fc: dfc, fp32, n_planes planes (1 .. 6) of d Phi / d eta_k; plane k starts at dfc + k plane_stride
 *     (elements) and is laid out exactly as fc under fc_ptr.  dfc_split: one such plane, the perturbation along which degenerate groups
 *     are split; it may be the same pointer as a plane of dfc (that plane is then streamed once).
 *   dD_k,ij = (m_i m_j)^-1/2 sum_J dPhi_k(i, J) (1 / m_iJ) sum_T exp(2 pi i q . x_T), then (dD_k + dD_k^H) / 2: D's own sums (fp64
 *     phase, copies ascending, fmaf) applied to plane k, so fc itself handed in as a plane assembles D(q) as the solvers do.
 *   Groups as in nnhip_phonon_velocities.  A group of one: dlam_k = Re e^H dD_k e.  A group of g <= 16: M_s = V^H dD_split V is
 *     diagonalised (eigenvalues ascending, ties by index) and the group's modes, in that order, take dlam_k = Re diag(U^H M_k U).
 *   dlam [.][n_planes], laid out like evals x n_planes: d lambda / d eta_k, eV/(A^2 amu) per unit of the strain parameter.
 *     gamma [.][n_planes] = -dlam / (2 lambda) where |lambda| > zero_tol[b], else 0.  group (may be null): per mode, the first mode of
 *     its group.  defined: per mode, 0 for |lambda| <= zero_tol[b] and for the modes of a group above 16.
 *   status [n_cry][n_q]: the bits of nnhip_phonon_velocities with the same meaning -- 1 and 2 (size, mass: nothing else of the problem
 *     is written), NNHIP_PHONON_STATUS_GROUP (dlam = gamma = 0, defined = 0 for the group's modes), NNHIP_PHONON_STATUS_NONFINITE
 *     (nothing of the problem is written beyond defined = 0).
 * One workgroup per (crystal, q, tile of modes, plane): grid (n_q, tiles x n_planes, n_cry); a workgroup streams the split plane and its
 * own, so plane k's result does not depend on n_planes.  No workspace, no float atomics, one writer per output: bitwise repeatable and
 * independent of the rest of the launch.  Checked BEFORE any launch: null pointers, n_planes outside 1 .. 6, cry_ptr_host decreasing
 * (NNHIP_E_INVALID); a crystal above nnhip_phonon_large_max_dim, more than 65535 crystals (NNHIP_E_UNSUPPORTED).
 * Measured against fp64 (tests/test_hip_gruneisen.py): see DESIGN.md section 23c.
 * ------------------------------------------------------------------------ */
int nnhip_phonon_strain_slopes(const float* dfc, int32_t n_planes, int64_t plane_stride, const float* dfc_split, const int64_t* fc_ptr,
                               const int32_t* cry_ptr, const int32_t* cry_ptr_host, const int32_t* sc_atoms, const int64_t* img_ptr,
                               const int32_t* img_start, const double* img_off, const float* masses, const int64_t* out_ptr,
                               int32_t n_cry, const double* q, int32_t n_q, const float* evals, const float* modes,
                               const float* deg_tol, const float* zero_tol, float* dlam, float* gamma, int32_t* group,
                               uint8_t* defined, int32_t* status, void* stream);

/* --------------------------------------------------------------------------
 * Analytic elastic constants of crystals.  The kernels, nnhip_elastic_fold and nnhip_elastic_relax are in csrc/elastic.hip;
 * nnhip_strain_vp is implemented in csrc/train_step.hip, next to the static tangent sweeps it drives.
 *   nnhip_strain_vp: the tangent-over-reverse pass of nnhip_hessian_vp seeded with a homogeneous strain instead of a position
 *     direction.  eta6 [n_mol][6] (device): the strain of every system of the batch in Voigt components with engineering shears,
 *     eps = [[e1, e6/2, e5/2], [e6/2, e2, e4/2], [e5/2, e4/2, e3]]; x -> (1 + eps) x moves every displacement vector of the graph by
 *     dd_e = eps d_e (periodic shifts included).  dgrad [N][3] = d(dE/dpos)/d eps along eta; d2 [n_mol][6]: d2[b][I] =
 *     d/d eta (dE/d e_I) = sum_ab (d eps_ab / d e_I) sum_e dg_d[e]_a d_e,b over the edges of system b (fp64 sums, fixed order).
 *     Needs what nnhip_hessian_vp needs (a prior nnhip_train_values on train_ws, train_ws->bf16_wgrad == 0) plus train_ws->batch
 *     and train_ws->mol_ptr.  The six unit strains give the clamped-ion (Born) matrix d^2E/de_I de_J column by column.
 *   nnhip_elastic_fold: Phi0[i a][j b] = sum over the supercell copies J of j of fc[i][a][J][b], then (Phi0 + Phi0^T) / 2: the force
 *     constants at Gamma of every crystal, from fc / fc_ptr / cry_ptr / sc_atoms as nnhip_phonon_bands takes them, written as
 *     [n_b][3][n_b][3] at phi0 + out_ptr[b] (out_ptr[b] = sum of 9 n_b'^2 before b: the blocks of nnhip_eig_blocks).  status [n_cry]:
 *     0, or NNHIP_ELASTIC_STATUS_SIZE where sc_atoms[b] is no multiple of the crystal's atoms (nothing of that crystal is written).
 *   nnhip_elastic_relax: R_IJ = sum_m (q_m . Lambda_I)(q_m . Lambda_J) / lambda_m of every crystal, one wave each, over the
 *     eigenpairs of Phi0 (evals [3 n] at 3 cry_ptr[b], modes at blk_ptr[b] with ROW m = mode m, as nnhip_eig_blocks writes them with
 *     unit masses) with |lambda_m| > threshold[b], ascending in lambda, fp64 sums.  lambda [3 n][6]: d(dE/dpos)/d e_I of the home
 *     atoms.  relax [n_cry][6][6] (symmetric).  n_zero / n_negative [n_cry]: modes left out / below -threshold; status [n_cry]:
 *     NNHIP_ELASTIC_STATUS_ZERO = n_zero != 3, NNHIP_ELASTIC_STATUS_NEGATIVE = a negative mode entered the sum (the geometry is no
 *     minimum: R is the formula's value, not a physical relaxation).
 * No float atomics, one writer per output: bitwise repeatable.
 * ------------------------------------------------------------------------ */
#define NNHIP_ELASTIC_STATUS_ZERO 1
#define NNHIP_ELASTIC_STATUS_NEGATIVE 2
#define NNHIP_ELASTIC_STATUS_SIZE 8
int nnhip_strain_vp(const nnhip_model* model, const nnhip_train_ws* train_ws, const nnhip_hvp_ws* hvp_ws, const float* eta6,
                    float* dgrad, float* d2, void* stream);
int nnhip_elastic_fold(const float* fc, const int64_t* fc_ptr, const int32_t* cry_ptr, const int32_t* sc_atoms,
                       const int64_t* out_ptr, int32_t n_cry, float* phi0, int32_t* status, void* stream);
int nnhip_elastic_relax(const float* evals, const float* modes, const int64_t* blk_ptr, const int32_t* cry_ptr, const float* lambda,
                        const float* threshold, int32_t n_cry, float* relax, int32_t* n_zero, int32_t* n_negative, int32_t* status,
                        void* stream);

/* --------------------------------------------------------------------------
 * Observables of recorded trajectories (csrc/observables.hip): the pair-distance histogram behind the radial distribution function and
 * lagged time correlations (mean squared displacement, velocity autocorrelation).  Frames are [n_frames][n_atoms][3] fp32 with a frame
 * stride in floats (>= 3 n_atoms); mol_ptr int32 [n_mol + 1] as everywhere; kind int32 [n_atoms]: the species index 0 .. n_kinds - 1
 * of an atom, any other value (-1) = the atom is ignored.  tests/observables_ref.py restates both.
 *
 *   nnhip_rdf_accumulate: counts [n_mol][P][n_bins] int64, P = n_kinds (n_kinds + 1) / 2, is ADDED TO.  Of every frame and system,
 *     every unordered pair i < j of counted atoms adds 1 to counts[b][p][k] where
 *       r2 = pair_disp(pos_i, pos_j) of the neighbour list (csrc/pair_disp.h; bit for bit: fp32, no contraction, d = pos_i - pos_j,
 *            for a periodic system f = d / L (diagonal cell, exact division) or the product with the fp32 image of the fp64 inverse,
 *            n = rintf(f), d -= (c0 n0 + c1 n1) + c2 n2, r2 = fma(dz, dz, fma(dy, dy, dx dx)): a single image; positions may be
 *            unwrapped),
 *       k:   edge2[k] <= r2 < edge2[k+1]   (edge2 fp32 [n_bins + 1], non-decreasing, edge2[0] = 0; r2 >= edge2[n_bins] is not counted),
 *       p:   the pair kind (a, c) = (min, max) of the two kinds, p = a n_kinds - a (a - 1) / 2 + (c - a): (0,0), (0,1), .., (1,1), ...
 *     The bin edges are thresholds on r2: the caller forms edge2[k] = the smallest float T with sqrt_rn(T) >= r_k on the host (the
 *     cut2_of construction of the neighbour list), so that bin k holds exactly the pairs with r_k <= sqrt_rn(r2) < r_{k+1}; the kernel
 *     takes a square root only to propose a bin, the table decides.
 *     cell: [n_frames][n_mol][3][3] with cell_frame_stride (floats) >= 9 n_mol, or [n_mol][3][3] with cell_frame_stride = 0 (the same
 *     cells for every frame); an all-zero cell = that system is not periodic.  max_atoms: the size of the largest system (it sizes
 *     the grid; a larger value costs idle workgroups, max_atoms < 2 = no pair: nothing is launched).
 *     One workgroup = (system, tile of 64 atoms i, chunk of frames): uint32 counters in LDS, flushed with 64-bit integer atomics before
 *     any of them can wrap.  Integer counts: the result does not depend on scheduling, on the grid or on how frames are split into calls.
 *     Checked BEFORE any launch: n_kinds > NNHIP_RDF_MAX_KINDS, n_bins > NNHIP_RDF_MAX_BINS or P n_bins > NNHIP_RDF_MAX_COUNTERS (the LDS histogram; NNHIP_E_INVALID with a message);
 *     more than 2^26 atoms or 65535 systems (NNHIP_E_UNSUPPORTED).
 *
 *   nnhip_time_correlation: sums [n_mol][n_kinds][max_lag + 1] fp64 is ADDED TO (one writer per element).  For lag l,
 *       sums[b][s][l] += sum over origins t0 = 0, origin_every, 2 origin_every, ... with t0 + l < n_frames, and over the atoms i of
 *                        system b with kind s, of term(i, t0, l), with a = x_i(t0), c = x_i(t0 + l), all fp32, no contraction:
 *         mode 0:  v = fma(a_z, c_z, fma(a_y, c_y, a_x c_x))                                          (x(t0) . x(t0 + l))
 *         mode 1:  d = c - a (three roundings);  v = fma(d_z, d_z, fma(d_y, d_y, d_x d_x))            (|x(t0 + l) - x(t0)|^2)
 *         term = v, or weight_i v (one more rounding) when weight [n_atoms] is given.
 *     Every term is converted to fp64 and every sum is in fp64, in this order: atoms in tiles of 16 (from the system's first atom),
 *     origins in blocks of 64 frames; wave p of 4 takes the atoms p, p + 4, .. of a tile; per (atom, block) the terms are added
 *     ascending in t0 to a subtotal, the subtotal to the accumulator of the atom's kind; at the end (p0 + p1) + (p2 + p3).  No float
 *     atomics, no workspace: two identical calls give identical bits and the result does not depend on the grid.  Direct evaluation,
 *     O(n_frames max_lag n_atoms): a workgroup = (system, 64 lags) stages the frames of an origin block and of the lags it meets in LDS.
 *     Checked BEFORE any launch: max_lag outside 0 .. n_frames - 1, origin_every < 1, mode other than 0 / 1, n_kinds outside 1 .. 8
 *     (NNHIP_E_INVALID); more than 65535 systems (NNHIP_E_UNSUPPORTED).
 * ------------------------------------------------------------------------ */
#define NNHIP_RDF_MAX_KINDS 8
#define NNHIP_RDF_MAX_BINS 4096
#define NNHIP_RDF_MAX_COUNTERS 16384
int nnhip_rdf_accumulate(const float* pos, int64_t pos_frame_stride, int32_t n_frames, const float* cell, int64_t cell_frame_stride,
                         const int32_t* mol_ptr, int32_t n_mol, int32_t n_atoms, int32_t max_atoms, const int32_t* kind,
                         int32_t n_kinds, const float* edge2, int32_t n_bins, int64_t* counts, void* stream);
int nnhip_time_correlation(const float* x, int64_t frame_stride, int32_t n_frames, const int32_t* mol_ptr, int32_t n_mol,
                           int32_t n_atoms, const int32_t* kind, int32_t n_kinds, const float* weight, int32_t mode, int32_t max_lag,
                           int32_t origin_every, double* sums, void* stream);

/* --------------------------------------------------------------------------
 * Timing hook for bench.py: wraps the kernels of one nnhip_energy_forces call
 * in HIP events on `stream` and accumulates per-kernel-class milliseconds.
 * classes: 0 = edge kernels (message/force fwd+adjoint), 1 = all dense MFMA kernels, 2 = everything else,
 *          3-6 = msg_fwd / force_fwd / force_bwd / msg_bwd, 7 = graph build, 8 = fused edge-MLP kernel (mlp128),
 *          9 = single linears (lin128), 10 = the batched weight-gradient kernel of training (wgrad_kernel, without its
 *          slab reduction), 11 = the one-pass register-weights form of the two edge MLPs (mlp_regw_kernel; its launches are
 *          counted in class 8 as well), 12 / 13 = unused (the molecule-resident fused edge phase of rounds 5-6,
 *          removed: slower than the row kernels, profiles/r06_fused_persistent_ab.txt).  Disabled (0) by default.  on = 1: every class; any other non-zero value is a mask,
 *          bit (k + 1) = class k: only those classes record events (bench.py times each class in a pass of its own, so that a
 *          kernel's duration is not stretched by the events of the kernels around it).
 * ------------------------------------------------------------------------ */
#define NNHIP_N_TIMER_CLASSES 14
int nnhip_timers_enable(int32_t on);
int nnhip_timers_read(double* ms_per_class, int64_t* launches_per_class, int32_t reset);

#ifdef __cplusplus
}
#endif
#endif /* NEWTONNET_HIP_H */
