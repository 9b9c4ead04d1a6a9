// The NNHIP_* environment switches of the library: ONE table.  To add a switch: a line here, a predicate where it is used, a line in
// tools/README.md (tests/test_switches_host.py holds the three together).  Every switch is read once per process, on the first
// call of switches(); nothing else under csrc/ calls getenv.  What the library does with them: nnhip_config (pipeline.hip).
#pragma once
#include <stdlib.h>

// Small systems (the one-molecule MD step, small training batches) are bound by the latency chain of a row, not by traffic or
// occupancy: up to this many rows every edge kernel gives a row four waves.  Back-to-back aspirin batches, us per step with /
// without: 1008 atoms 389 / 404, 2016: 303 / 304, 3024: 390 / 383, 5376: 574 / 568 (profiles/r04_small_thresholds.txt).
#ifndef EDGE_SMALL_ATOMS
#define EDGE_SMALL_ATOMS 2048
#endif

// X(type, kind, field, name, default).  kind: flag = on unless set to something atoi reads as 0 (so garbage is OFF);
// num / lnum = atoi / atol of the value, the default when unset.
#define NNHIP_SWITCH_TABLE(X)                                                                                                      \
  X(long, lnum, edge_lds, "NNHIP_EDGE_LDS", 0)                        /* tooling: bytes of unused dynamic LDS on the edge kernels (caps occupancy) */ \
  X(int, num, edge_small_atoms, "NNHIP_EDGE_SMALL_ATOMS", EDGE_SMALL_ATOMS) /* four waves per edge row up to this many atoms (0 = never) */ \
  X(int, num, edge_wpr, "NNHIP_EDGE_WPR", 0)                          /* 1|2|4: that split for every row kernel at every size (tests reach the non-default forms); else 0 */ \
  X(int, flag, force_bwd_owner_gu, "NNHIP_FORCE_BWD_OWNER_GU", 1)     /* A/B: 0 = every force_bwd row computes its own g_u */ \
  X(int, flag, force_direct_mol, "NNHIP_FORCE_DIRECT_MOL", 1)         /* 0: never force_direct_mol_kernel */ \
  X(int, flag, force_fwd_mol, "NNHIP_FORCE_FWD_MOL", 1)               /* 0: never force_fwd_mol_kernel */ \
  X(int, flag, graph_mol, "NNHIP_GRAPH_MOL", 1)                       /* 0: never the per-molecule neighbor list in the deferred step */ \
  X(int, num, graph_small_atoms, "NNHIP_GRAPH_SMALL_ATOMS", 128)      /* single-launch neighbor list up to this many atoms (graph.hip clamps to what the kernel serves; profiles/r04_small_thresholds.txt) */ \
  X(int, flag, head_out_mol, "NNHIP_HEAD_OUT_MOL", 1)                 /* 0: never head_out_mol_kernel */ \
  X(int, num, lin_blocks, "NNHIP_LIN_BLOCKS", 512)                    /* tuning knob (tools/bench_lin.py): workgroup cap of lin128_kernel, 2 per CU x 256 CUs */ \
  X(int, num, mlp_regw, "NNHIP_MLP_REGW", 1)                          /* register-weights edge MLPs: 0 off, 1 the adjoint launches (106 vs 121 us), 2 the forward too (108 vs 106 us) */ \
  X(int, num, mlp_regw_single, "NNHIP_MLP_REGW_SINGLE", 1)            /* the same for the one MLP of layer 0: 0 off, 1 the adjoint, 2 the forward too */ \
  X(int, flag, mlp_regw_train, "NNHIP_MLP_REGW_TRAIN", 1)             /* 0: the training sweeps keep the two-phase form */ \
  X(int, flag, mlp_split, "NNHIP_MLP_SPLIT", 1)                       /* 0: fp32 MFMA instead of split-f16 products everywhere (tooling, A/B) */ \
  X(int, num, mlp_wide_tiles, "NNHIP_MLP_WIDE_TILES", -1)             /* row-local MLP form up to this many 32-row tiles; below 0 = the built-in threshold */ \
  X(int, num, mol_kernels_min, "NNHIP_MOL_KERNELS_MIN", 640)          /* molecule-resident edge kernels from this many molecules (profiles/r04_mol_kernels_crossover.txt) */ \
  X(int, flag, msg_bwd_force, "NNHIP_MSG_BWD_FORCE", 1)               /* 0: layer 0's msg_bwd_mol_kernel never goes on with the forces */ \
  X(int, flag, msg_bwd_mol, "NNHIP_MSG_BWD_MOL", 1)                   /* 0: never msg_bwd_mol_kernel */ \
  X(int, flag, node_bwd_q, "NNHIP_NODE_BWD_Q", 1)                     /* 0: node_fwd stores q = f W_u^T and node_bwd reads it back, instead of forming it again */ \
  X(int, flag, node_turn, "NNHIP_NODE_TURN", 1)                       /* 0: the turn-around as its three launches (node_fwd, head_out, node_bwd) */

struct Switches {
#define X(type, kind, field, name, dflt) type field;
  NNHIP_SWITCH_TABLE(X)
#undef X
};

// the names, for the "env" echo of nnhip_config; and the switches that the Python package reads, echoed only
inline const char* const kSwitchNames[] = {
#define X(type, kind, field, name, dflt) name,
    NNHIP_SWITCH_TABLE(X)
#undef X
};
inline const char* const kPythonSwitchNames[] = {"NNHIP_TRAIN_BF16", "NNHIP_WGRAD_FORM", "NNHIP_WGRAD_RPC"};

inline const char* switch_text(const char* name) { return getenv(name); }   // NULL = not set
inline int switch_flag(const char* v, int) { return (v && atoi(v) == 0) ? 0 : 1; }
inline int switch_num(const char* v, int dflt) { return v ? atoi(v) : dflt; }
inline long switch_lnum(const char* v, long dflt) { return v ? atol(v) : dflt; }

inline const Switches& switches() {
  static const Switches sw = [] {   // (a function-local static: filled once, also with concurrent host threads)
    Switches s;
#define X(type, kind, field, name, dflt) s.field = switch_##kind(switch_text(name), dflt);
    NNHIP_SWITCH_TABLE(X)
#undef X
    if (s.edge_wpr != 1 && s.edge_wpr != 2 && s.edge_wpr != 4) s.edge_wpr = 0;
    if (s.mlp_wide_tiles < 0) s.mlp_wide_tiles = -1;
    return s;
  }();
  return sw;
}
