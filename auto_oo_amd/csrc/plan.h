// The plan of one batched CAS evaluation (cas.hip): everything the host decides for a call -- which of the six
// paths runs, which stage-1 kernel, where the workspace blocks lie, where the circuit goes -- as plain data computed
// once by oovqe_eval_plan from the shape, the symmetry flags, what the caller holds, the option values and the CU
// count.  The entry points build it; cas_eval_batched and oovqe_oo_eval_batched_impl only launch from it.
#pragma once
#include "internal.h"

enum EvalPath {
    PATH_PACKED_TAIL = 0,     // packed triangle J, then q -> x, p -> n, Fock columns and assembly in ONE launch per call
    PATH_PACKED_SPLIT,        // packed triangle J, then sym_gm, panel and final launches
    PATH_PACKED_TWO_STEP,     // packed triangle J (row-major), q -> x kernel, K1 p -> n, panel, final (options only)
    PATH_FUSED,               // stage 1 + q -> x in one persistent kernel, K1 p -> n, panel, final
    PATH_COLUMN,              // T2, K1 p -> n, column kernel (q -> x and stage 3 per general index), final
    PATH_STAGED               // T2, then per geometry: K1 q -> x, p -> n, h_mo, Fock kernels on g_mo in memory
};
enum CircuitPlace {
    CIRCUIT_NONE = 0,         // the RDM sets are given
    CIRCUIT_RIDES,            // its workgroups ride along the p -> n launch (K1 or sym_gm)
    CIRCUIT_OWN               // a launch of its own, ahead of stage 1
};
enum Stage1Kernel {
    S1_HALF, S1_STREAM, S1_TILES,     // T2: one slab per wave (N <= 48) | persistent streaming | tile-packed copy (N > 48)
    S1_FUSED,                         // T3 of the fused path
    S1_TRI, S1_TRI_REG,               // packed triangle J from the full | the packed integrals
    S1_FROM_T2                        // packed triangle J from the caller's T2 (no sweep over the integrals)
};
// profile labels of the launches of an evaluation (ops.PROFILE_LABELS)
enum { LABEL_STAGE1 = 0, LABEL_CIRCUIT, LABEL_P_TO_N, LABEL_COLUMN, LABEL_FINAL, LABEL_Q_TO_X, LABEL_COUNT };
// blocks of the CAS workspace (each stacked over the batch)
enum WorkBlock { WB_JP = 0, WB_T3, WB_GMW, WB_CDUP, WB_T2, WB_U, WB_FCOL, WB_EPART, WB_CPART, WB_COUNT };

// The stage-1 kernels for N <= 48 are built for four slab shapes: kch k-steps per register chunk (the whole row),
// nrb 16-column tiles; npc: 1 KB pieces of a packed slab; ks: k-steps of the q -> x kernels (sym_q_contract, sym_gm,
// cas_tail), which have no build for 11.
struct Stage1Variant {
    int kch, nrb, npc, ks;
};

struct Stage1 {
    Stage1Kernel kernel;
    Stage1Variant v;                  // N <= 48
    int zt, sym;                      // S1_HALF, S1_STREAM, S1_TILES: 16-wide tiles of M; slabs read / layout written (SYM_*)
    int tiled;                        // S1_TRI, S1_TRI_REG: layout of J (see stage1_tri)
    int skch;                         // S1_STREAM: k-steps per chunk
    bool rs;                          // S1_STREAM: upper r <= s triangle of every slab only
    char name[64];                    // as oovqe_last_stage1_kernel reports it ("" for S1_FROM_T2: no sweep of its own)
};

// fused stage-1 + q -> x kernel for `batch` geometries: number of q chunks, slots per chunk, LDS ring
struct FusedPlan {
    int nchunk, qc, nbuf, ldb, wpg;
    size_t lds_bytes;
};

// the option values a plan depends on (common.h: oovqe_option_t)
struct EvalOpts {
    int fused_chunks, no_ride;
    bool cas_unfused, sym_no_rs, sym_mirror, sym_simple, sym_two_step, panel_no_w, tail_split;
    ContractOpts k1;
};
EvalOpts oovqe_eval_opts();           // as set now

struct EvalShape {
    int N, n_occ, ncas, nrdm, n_kappa, batch;
    unsigned eri_flags;
    bool packed;                      // the caller holds the packed copy of the integrals
    bool t2_ready;                    // ... stage 1's result T2
    bool extras;                      // Fock / gradient matrices or MO integrals are asked for beyond the packed outputs
    int n_qubits, n_gates;            // the circuit that produces the nrdm RDM sets (n_qubits == 0: they are given)
    int n_cu;
    EvalOpts opt;
};

struct EvalPlan {
    EvalPath path;
    Stage1 stage1;
    FusedPlan fused;                  // PATH_FUSED
    CircuitPlace circuit;
    bool circuit_small;               // the one-workgroup circuit + RDM kernel serves
    bool w;                           // the circuit's own launch leaves W = C^T h_ao [G][N][N] in block WB_T3
    bool rs;                          // the r <-> s flag is set and used
    int tail_nc;                      // PATH_PACKED_TAIL: kept entries of g_mo[n]
    size_t tail_lds;                  // ... and LDS bytes of cas_tail_kernel
    bool staged_rows;                 // PATH_STAGED: the rows kernels serve stage 3 (else the one-workgroup fock_kernel)
    size_t off[WB_COUNT], len[WB_COUNT];   // workspace blocks in doubles (len 0: not used by this path)
    int labels[LABEL_COUNT];          // bracketed launches by profile label
    long launches;                    // kernel launches of the call
};

// 0, or OOVQE_ERR_ARG with the error set (a shape no kernel serves)
int oovqe_eval_plan(const EvalShape& s, EvalPlan* plan);

// What the launch code of a path decides below the plan, as plain arithmetic on the shape, the option values and the
// CU count (cas.hip: the launch functions call these, oovqe_oo_eval_plan_describe reports them).
// cas_panel_kernel: general indices per workgroup, the LDS limit of that number, RDM sets per LDS chunk
struct PanelGeom {
    int npan, npan_max, rdm_chunk;
    size_t lds_bytes;
};
// cas_column_kernel: RDM sets per LDS chunk, workgroups per general index that share the chunks
struct ColumnGeom {
    int rdm_chunk, zsplit;
    size_t lds_bytes;
};
// w: the kernel reads the ready-made W = C^T h_ao; panel_rows: option panel_rows (0: chosen here).  false: no room in LDS
bool oovqe_panel_geom(int N, int n_occ, int ncas, int nrdm, int batch, bool w, int panel_rows, PanelGeom* g);
bool oovqe_column_geom(int N, int n_occ, int ncas, int nrdm, int batch, int n_cu, ColumnGeom* g);
// the 1-D grid that keeps the workgroups of a geometry on one XCD (sym_gm_kernel, cas_panel_kernel): the batch rounded
// up to a multiple of 8; plain_grid: option gm_plain_grid
inline bool oovqe_xcd_grid(int batch, bool plain_grid) { return batch > 1 && !plain_grid; }
