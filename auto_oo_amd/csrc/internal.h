// Functions of liboovqe_hip.so that cross translation units without being part of the C ABI
// (include/oovqe.h): each is declared here once, with its default arguments.
#pragma once
#include "common.h"

// ---- contract.hip: out = T x_mode Cm (the K1 contraction kernels) ----------------------------------------
int oovqe_mode_contract_impl(const double* T, const double* Cm, double* out, long A, int K, int J,
                             long B, int ldc, int last, hipStream_t st);
// the same for `batch` independent problems (strides in doubles), the batch index a grid dimension; cj: the
// small-circuit evaluations whose workgroups ride along the launch (a shape oovqe_contract_hosts_circuit accepts)
int oovqe_mode_contract_batched(const double* T, const double* Cm, double* out, long A, int K, int J,
                                long B, int ldc, int last, int batch, long t_bs, long c_bs, long o_bs,
                                hipStream_t st, const oovqe_circuit_job_t* cj = nullptr);
// the test / measurement options that bear on the choice of a contraction's kernel (common.h: k1_*), as values
struct ContractOpts {
    int force_nt;
    bool force_wide, no_pair;
};
ContractOpts oovqe_contract_opts();   // as set now
// can the launch for this shape host circuit workgroups?
int oovqe_contract_hosts_circuit(long A, int K, int J, long B, int last, int batch, const ContractOpts& o);

// ---- contract_pair.hip: two 16-wide strips per wave ------------------------------------------------------
int oovqe_contract_pair_ok(const double* T, const double* out, long A, long B, int nt, int ngroups, int batch,
                           long t_bs, long o_bs);
int oovqe_contract_pair_grid(long A, long B, int ngroups, int batch, long* n_items, long* grid_x);
int oovqe_contract_pair_launch(const double* T, const double* Cm, double* out, long A, int K, int J, long B,
                               int ldc, int nt, int ngroups, int deep, int batch, long t_bs, long c_bs,
                               long o_bs, hipStream_t st);

// ---- circuit.hip -----------------------------------------------------------------------------------------
// oovqe_circuit_rdms with W = C^T h_ao [batch][N][N] of every geometry formed by extra workgroups of the launch
// (Wpre non-null: small circuits only, N <= 48, batch <= 32767)
int oovqe_circuit_rdms_w(const double* theta, int n_theta, const oovqe_gate_t* gates, int n_gates, int n_qubits,
                         int ncas, uint32_t init_index, int want_tangents, int batch, double* psi, double* dpsi,
                         double* gamma, double* Gamma, double* work, const double* h_ao, const double* C, int N,
                         double* Wpre, oovqe_stream_t stream);
// batch elements stacked: theta [batch][n_theta]; c1 / c2 of element b at c1 + b * c1_bs, c2 + b * c2_bs;
// H element (j,k) of b at H[b * h_bs + j * ldh + k]; work: batch * oovqe_circuit_hessian_work_size()
int oovqe_circuit_hessian_batched_impl(const double* theta, int n_theta, const oovqe_gate_t* gates,
                                       int n_gates, int n_qubits, int ncas, uint32_t init_index,
                                       const double* c1, const double* c2, long c1_bs, long c2_bs,
                                       const int32_t* pairs, int n_pairs, int batch, double* work, double* H,
                                       long ldh, long h_bs, oovqe_stream_t stream);

// ---- cas.hip ---------------------------------------------------------------------------------------------
// the packed output of one geometry: [c0 | E | dE (max(nvec-1,1)) | gvec (nvec x n_kappa) | c1 (a^2) | c2 (a^4)]
struct OutSlab {
    double *c0, *E, *dE, *gvec, *c1, *c2;
};
inline OutSlab out_layout(double* out, int nvec, int n_kappa, int ncas)
{
    OutSlab o;
    o.c0 = out;
    o.E = out + 1;
    o.dE = out + 2;
    o.gvec = o.dE + (nvec > 1 ? nvec - 1 : 1);
    o.c1 = o.gvec + (size_t)nvec * n_kappa;
    o.c2 = o.c1 + (size_t)ncas * ncas;
    return o;
}

// Batched CAS path: `batch` geometries of identical shape, every per-geometry array stacked.
struct CasEvalArgs {
    const double *g_ao, *h_ao, *C;          // [G][N^4], [G][N^2], [G][N^2]
    const double *gamma, *Gamma;            // [G][nrdm][a^2], [G][nrdm][a^4]
    int nrdm;
    double nuc;                             // every geometry's nuclear repulsion, unless nuc_arr [G] is given
    const double* nuc_arr;
    int N, n_occ, ncas;
    const int32_t *kap_row, *kap_col;
    int n_kappa;
    double* work;                           // G * oovqe_cas_eval_work_size()
    OutSlab out;                            // outputs of geometry 0; those of geometry g at pointer + g * out_stride
    size_t out_stride;
    double *fock, *gmat, *Gm, *hmo;         // optional extra outputs [G][N][N], [G][N][N], [G][N][M^3], [G][N][M]
    int batch;
    oovqe_stream_t stream;
    unsigned eri_flags;
    const double* g_packed;                 // the packed copy of the integrals (oovqe_eri_pack) or null
    const double* T2_ready;                 // [G][N][N][M][M]: stage 1's result, when the caller has it in memory
    const oovqe_circuit_job_t* cj;          // the evaluations that produce gamma / Gamma, when they ride along (plan.h)
    hipEvent_t rdm_event;                   // recorded on the stream where gamma / Gamma are complete, or null
};

// One OO-VQE evaluation for each of `batch` geometries (same circuit, same shapes): circuit (+ tangents) -> RDM
// sets -> CAS path.  The RDM sets stay at the head of `work` (gamma [G][nvec][a^2], then Gamma [G][nvec][a^4]).
struct OoEvalArgs {
    const double* theta;             // [G][n_theta]
    int n_theta;
    const oovqe_gate_t* gates;
    int n_gates, n_qubits;
    uint32_t init_index;
    int derivatives;
    double* work;                    // G * oovqe_oo_eval_work_size()
    double* out;                     // [G][oovqe_oo_eval_out_size()], see out_layout
    CasEvalArgs cas;                 // integrals, shape, index tables, flags, stream, optional buffers; the RDM sets,
                                     // work, out and cj are filled in by the callee
};
int oovqe_oo_eval_batched_impl(const OoEvalArgs& a);

// stage 1 (T2[p,q,y,z]) for a stack of geometries, reading only the slabs p <= q when the flags vouch for the
// p<->q symmetry.  Vk_tri [G][N(N+1)/2][N][M] (optional; p <-> q symmetric integrals, N <= 48): the first product
// of every slab as well, see half_transform_kernel
int oovqe_half_transform_batched_impl(const double* g_ao, const double* C, int N, int M, double* T2,
                                      int batch, unsigned eri_flags, oovqe_stream_t stream,
                                      double* Vk_tri = nullptr);

// ---- newton_chol.hip -------------------------------------------------------------------------------------
int oovqe_newton_chol_launch(const double* hessian, const double* gradient, int n, int batch, double lambda_min,
                             double* work, double* dp, double* shift, double* info, hipStream_t st);
size_t oovqe_newton_chol_work(int n, int batch);
int oovqe_newton_chol_max_n(void);
