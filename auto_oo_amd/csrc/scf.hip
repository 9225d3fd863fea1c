// Batched closed-shell restricted Hartree-Fock for a stack of geometries (gfx950), the algorithm of the host
// gaussian.rhf iterate for iterate: core-Hamiltonian guess, F = h + J - K / 2, E = 1/2 sum D (h + F), DIIS on
// e = F D S - S D F over the last 8 Fock matrices, diagonalisation in the S^-1/2 basis, aufbau occupation.
//
//   scf_fock_jk_kernel  J[p,q] = sum_rs g[p,q,r,s] D[r,s], K[p,q] = sum_rs g[p,r,q,s] D[r,s]: ONE pass over the tensor,
//                       no symmetry assumed.  One workgroup per (geometry, p), one wave per slab g[p,q,:,:]: the slab
//                       goes through LDS once, J[p,q] = <slab, D> on the way in, the partial row slab . D[q,:] of K[p,:]
//                       on the way out; the partial rows of the waves are summed through LDS in a fixed order.  No
//                       floating-point atomics, every output written once: the result of a geometry does not depend on
//                       the stack around it.
//   sym_eig_kernel      eigenvalues ascending, eigenvectors in columns (largest component positive), one wave per
//                       matrix, on sym_jacobi_wave (jacobi.h) -- the iteration of the S^-1/2 kernel.
//   scf_step_kernel     one workgroup per geometry: everything of size N^2 and N^3 between two Fock contractions
//                       (F, E, commutator, DIIS history / system / solve, X F X, the eigensolver on wave 0, C = X c,
//                       D = 2 C_occ C_occ^T, the convergence test).  A geometry that has finished is frozen: both
//                       kernels leave at once for it and none of its outputs is touched again.
//
// LDS of the step kernel: three matrices [n][n | 1] + 512 doubles = 101.9 KB at n = 64 (limit 160 KB); of the Fock
// kernel: four slabs [n][n | 1] = 130 KB at n = 64, 59 KB at n = 43 (two workgroups per CU).
#include "common.h"
#include "jacobi.h"
#include <math.h>

#define SCF_NT 256
#define SCF_NW (SCF_NT / 64)
#define SCF_HIST 8              // Fock matrices the DIIS keeps (gaussian.rhf: fs[-8:])
#define SCF_CHECK_EVERY 4       // iterations between two looks of the host at the count of finished geometries

// per-geometry block of the work buffer, in doubles
#define SCF_SCAL 8              // [0] previous energy
__host__ __device__ static inline size_t scf_geom_doubles(int n)
{
    return (size_t)(3 + 2 * SCF_HIST) * n * n + SCF_HIST * SCF_HIST + SCF_SCAL;
}

// ---- Fock contraction ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SCF_NT) void scf_fock_jk_kernel(const double* __restrict__ g, const double* __restrict__ D,
                                                             size_t d_stride, int n, const int* __restrict__ status,
                                                             double* __restrict__ J, double* __restrict__ K,
                                                             size_t jk_stride)
{
    extern __shared__ double lds[];
    const int p = blockIdx.x, b = blockIdx.y;
    if (status != nullptr && status[b] != 0) return;
    const int ld = n | 1, nn = n * n;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double* slab = lds + (size_t)wave * n * ld;
    const double* Db = D + (size_t)b * d_stride;
    const double* gp = g + ((size_t)b * n + p) * (size_t)n * nn;
    const int dq = 64 / n, dr = 64 - dq * n;              // a step of 64 elements in (row, column)
    const int r0 = lane / n, c0 = lane - r0 * n;
    double kacc = 0.0;
    for (int q = wave; q < n; q += SCF_NW) {
        const double* sl = gp + (size_t)q * nn;
        double jacc = 0.0;
        int r = r0, c = c0;
        for (int k0 = lane; k0 < nn; k0 += 4 * 64) {
            double v[4], d[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + 64 * j;
                v[j] = (k < nn) ? sl[k] : 0.0;
                d[j] = (k < nn) ? Db[k] : 0.0;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (k0 + 64 * j < nn) {
                    slab[r * ld + c] = v[j];
                    jacc += v[j] * d[j];
                }
                c += dr; r += dq;
                if (c >= n) { c -= n; ++r; }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) jacc += __shfl_xor(jacc, o, 64);
        if (lane == 0) J[(size_t)b * jk_stride + (size_t)p * n + q] = jacc;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        if (lane < n) {
            const double* drow = Db + (size_t)q * n;
            double acc = 0.0;
            for (int s = 0; s < n; ++s) acc += slab[lane * ld + s] * drow[s];
            kacc += acc;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
    __syncthreads();                                       // every slab is consumed: the partial rows take their place
    lds[wave * 64 + lane] = (lane < n) ? kacc : 0.0;
    __syncthreads();
    const int t = threadIdx.x;
    if (t < n) {
        double x = lds[t];
#pragma unroll
        for (int w = 1; w < SCF_NW; ++w) x += lds[w * 64 + t];
        K[(size_t)b * jk_stride + (size_t)p * n + t] = x;
    }
}

static size_t scf_fock_lds(int n)
{
    const size_t a = (size_t)SCF_NW * n * (n | 1), b = (size_t)SCF_NW * 64;
    return (a > b ? a : b) * sizeof(double);
}

static int scf_launch_fock(const double* g, const double* D, size_t d_stride, int n, int batch, const int* status,
                           double* J, double* K, size_t jk_stride, hipStream_t st)
{
    const size_t lds = scf_fock_lds(n);
    if (oovqe_ensure_dynamic_lds(reinterpret_cast<const void*>(&scf_fock_jk_kernel), lds) != 0) return OOVQE_ERR_HIP;
    for (int b0 = 0; b0 < batch; b0 += 65535) {            // (grid.y limit)
        const int nb = batch - b0 < 65535 ? batch - b0 : 65535;
        hipLaunchKernelGGL(scf_fock_jk_kernel, dim3(n, nb), dim3(SCF_NT), lds, st,
                           g + (size_t)b0 * n * n * n * n, D + (size_t)b0 * d_stride, d_stride, n,
                           status ? status + b0 : nullptr, J + (size_t)b0 * jk_stride, K + (size_t)b0 * jk_stride,
                           jk_stride);
        OOVQE_CHECK_LAUNCH("scf_fock_jk_kernel");
    }
    return 0;
}

extern "C" int oovqe_fock_jk_batch(const double* g, const double* d, int n, int batch, double* j, double* k,
                                   oovqe_stream_t stream)
{
    const char* who = "oovqe_fock_jk_batch";
    OOVQE_REQUIRE(n >= 1 && n <= OOVQE_INVSQRT_MAX_N, "%s: n = %d (1 .. %d)", who, n, OOVQE_INVSQRT_MAX_N);
    OOVQE_REQUIRE(batch >= 0, "%s: batch = %d", who, batch);
    OOVQE_REQUIRE(g && d && j && k, "%s: null pointer", who);
    if (batch == 0) return 0;
    return scf_launch_fock(g, d, (size_t)n * n, n, batch, nullptr, j, k, (size_t)n * n, (hipStream_t)stream);
}

// ---- eigensolver --------------------------------------------------------------------------------------------------
// After sym_jacobi_wave: eigenvalues ascending (equal ones in the order of their columns) to w[0 .. n), the
// eigenvectors, each with its component of largest magnitude positive (the first one on ties), to the columns of
// v [n][ldv] and, if given, v2 [n][ldv2].  One wave; lane j carries column j.
__device__ __forceinline__ void scf_eig_sorted(const double* A, const double* U, int n, int ld, int lane, double* w,
                                               double* v, int ldv, double* v2, int ldv2)
{
    if (lane < n) {
        const double wj = A[lane * ld + lane];
        int rank = 0;
        double best = -1.0, sgn = 1.0;
        for (int i = 0; i < n; ++i) {
            const double wi = A[i * ld + i];
            rank += (wi < wj || (wi == wj && i < lane)) ? 1 : 0;
            const double u = U[i * ld + lane];
            if (fabs(u) > best) { best = fabs(u); sgn = (u < 0.0) ? -1.0 : 1.0; }
        }
        w[rank] = wj;
        for (int i = 0; i < n; ++i) {
            const double x = sgn * U[i * ld + lane];
            v[i * ldv + rank] = x;
            if (v2 != nullptr) v2[i * ldv2 + rank] = x;
        }
    }
}

__global__ __launch_bounds__(JACOBI_NT) void sym_eig_kernel(const double* __restrict__ Ain, int n,
                                                            double* __restrict__ W, double* __restrict__ V,
                                                            int* __restrict__ info)
{
    extern __shared__ double lds[];
    const int ld = n | 1;
    double* A = lds;
    double* U = lds + (size_t)n * ld;
    double* cs = U + (size_t)n * ld;
    int* pq = reinterpret_cast<int*>(cs + JACOBI_NT);
    const int lane = threadIdx.x, b = blockIdx.x;
    const double* Ab = Ain + (size_t)b * n * n;
    bool bad = false;
    for (int k = lane; k < n * n; k += JACOBI_NT) {
        const int r = k / n, c = k - r * n;
        const double x = (r >= c) ? Ab[r * n + c] : Ab[c * n + r];     // (the lower triangle is read)
        bad = bad || !isfinite(x);
        A[r * ld + c] = x;
        U[r * ld + c] = (r == c) ? 1.0 : 0.0;
    }
    const bool any_bad = __any(bad);
    if (lane == 0) info[b] = any_bad ? -3 : 0;
    if (any_bad) {
        for (int k = lane; k < n * n; k += JACOBI_NT) V[(size_t)b * n * n + k] = __builtin_nan("");
        if (lane < n) W[(size_t)b * n + lane] = __builtin_nan("");
        return;
    }
    sym_jacobi_wave(A, U, cs, pq, n, ld, lane);
    scf_eig_sorted(A, U, n, ld, lane, W + (size_t)b * n, V + (size_t)b * n * n, n, nullptr, 0);
}

extern "C" int oovqe_sym_eig_batch(const double* a, int n, int batch, double* w, double* v, int* info,
                                   oovqe_stream_t stream)
{
    const char* who = "oovqe_sym_eig_batch";
    OOVQE_REQUIRE(n >= 1 && n <= OOVQE_INVSQRT_MAX_N, "%s: n = %d (1 .. %d)", who, n, OOVQE_INVSQRT_MAX_N);
    OOVQE_REQUIRE(batch >= 0, "%s: batch = %d", who, batch);
    OOVQE_REQUIRE(a && w && v && info, "%s: null pointer", who);
    if (batch == 0) return 0;
    const size_t lds = (2 * (size_t)n * (n | 1) + 2 * JACOBI_NT) * sizeof(double);
    if (oovqe_ensure_dynamic_lds(reinterpret_cast<const void*>(&sym_eig_kernel), lds) != 0) return OOVQE_ERR_HIP;
    hipLaunchKernelGGL(sym_eig_kernel, dim3(batch), dim3(JACOBI_NT), lds, (hipStream_t)stream, a, n, w, v, info);
    OOVQE_CHECK_LAUNCH("sym_eig_kernel");
    return 0;
}

// ---- SCF step -----------------------------------------------------------------------------------------------------
struct scf_step_t {
    const double* h; const double* s;      // [batch][n][n]
    const double* x;                       // S^-1/2 [batch][n][n]: the caller's, or the one made in `work`
    const int* x_info;                     // info of the S^-1/2 kernel [batch]; null when x is the caller's
    double* work;                          // per geometry: D, J, K, F history, e history, B, scalars
    int* status;                           // [batch] 0 running, 1 frozen
    int* done;                             // count of frozen geometries
    double* mo_coeff; double* oao_mo_coeff; double* mo_energy; double* e_elec; double* diis_error;
    int* iterations; int* info;
    double conv_tol, err_tol;
    int n, n_occ, it, max_cycle;           // it = -1: the core-Hamiltonian guess
};

// sum / maximum over the workgroup, the same bits in every thread (butterfly inside a wave, waves in order)
__device__ __forceinline__ double scf_block_sum(double v, double* red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double x = red[0];
#pragma unroll
    for (int w = 1; w < SCF_NW; ++w) x += red[w];
    return x;
}

__device__ __forceinline__ double scf_block_max(double v, double* red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double x = red[0];
#pragma unroll
    for (int w = 1; w < SCF_NW; ++w) x = fmax(x, red[w]);
    return x;
}

// the geometry ends with a failure code: every output NaN, frozen
__device__ void scf_fail(const scf_step_t& a, int b, int code, int iterations)
{
    const int n = a.n, nn = n * n;
    const double nan = __builtin_nan("");
    for (int e = threadIdx.x; e < nn; e += SCF_NT) {
        a.mo_coeff[(size_t)b * nn + e] = nan;
        a.oao_mo_coeff[(size_t)b * nn + e] = nan;
    }
    for (int e = threadIdx.x; e < n; e += SCF_NT) a.mo_energy[(size_t)b * n + e] = nan;
    if (threadIdx.x == 0) {
        a.e_elec[b] = nan;
        a.diis_error[b] = nan;
        a.iterations[b] = iterations;
        a.info[b] = code;
        a.status[b] = 1;
        atomicAdd(a.done, 1);
    }
}

__global__ __launch_bounds__(SCF_NT) void scf_step_kernel(const scf_step_t a)
{
    extern __shared__ double lds[];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (a.status[b] != 0) return;
    const int n = a.n, nn = n * n, ld = n | 1, it = a.it;
    double* T0 = lds;
    double* T1 = T0 + (size_t)n * ld;
    double* T2 = T1 + (size_t)n * ld;
    double* red = T2 + (size_t)n * ld;                 // [8] reductions
    double* wts = red + 8;                             // [SCF_HIST] DIIS weights, [SCF_HIST] = 1 when they are valid
    double* sys = wts + SCF_HIST + 8;                  // [SCF_HIST + 1][SCF_HIST + 2] augmented DIIS system
    double* cs = sys + (SCF_HIST + 1) * (SCF_HIST + 2) + 6;     // Jacobi: rotations and index pairs of a round
    int* pq = reinterpret_cast<int*>(cs + JACOBI_NT);

    double* wk = a.work + (size_t)b * scf_geom_doubles(n);
    double* D = wk;
    const double* J = wk + (size_t)nn;
    const double* K = wk + (size_t)2 * nn;
    const double* X = a.x + (size_t)b * nn;
    double* Fh = wk + (size_t)3 * nn;
    double* Eh = Fh + (size_t)SCF_HIST * nn;
    double* Bm = Eh + (size_t)SCF_HIST * nn;
    double* scal = Bm + SCF_HIST * SCF_HIST;
    const double* h = a.h + (size_t)b * nn;
    const double* S = a.s + (size_t)b * nn;

    double energy = 0.0, maxerr = 0.0;
    if (it < 0) {
        // ---- start: inputs finite, S^-1/2 exists; the matrix to diagonalise is h ----
        double bad = 0.0;
        for (int e = tid; e < nn; e += SCF_NT) {
            const double hv = h[e];
            if (!isfinite(hv) || !isfinite(S[e]) || (a.x_info == nullptr && !isfinite(X[e]))) bad = 1.0;
            const int r = e / n, c = e - r * n;
            T0[r * ld + c] = hv;
        }
        bad = scf_block_max(bad, red);
        if (bad != 0.0) { scf_fail(a, b, -3, 0); return; }
        if (a.x_info != nullptr && a.x_info[b] != 0) { scf_fail(a, b, -1, 0); return; }
        if (tid == 0) scal[0] = 0.0;
    } else {
        // ---- F = h + J - K / 2, E = 1/2 sum D (h + F) ----
        const int slot = it % SCF_HIST, m = (it + 1 < SCF_HIST) ? it + 1 : SCF_HIST;
        double* Fs = Fh + (size_t)slot * nn;
        double* Es = Eh + (size_t)slot * nn;
        double esum = 0.0, bad = 0.0;
        for (int e = tid; e < nn; e += SCF_NT) {
            const double hv = h[e], dv = D[e];
            const double f = hv + J[e] - 0.5 * K[e];
            if (!isfinite(f)) bad = 1.0;
            esum += dv * (hv + f);
            const int r = e / n, c = e - r * n;
            T0[r * ld + c] = f;
            T1[r * ld + c] = dv;
            Fs[e] = f;
        }
        bad = scf_block_max(bad, red);
        if (bad != 0.0) { scf_fail(a, b, -3, it + 1); return; }     // (NaN or Inf in the two-electron integrals)
        energy = 0.5 * scf_block_sum(esum, red);
        // ---- e = F D S - S D F ----
        __syncthreads();
        for (int e = tid; e < nn; e += SCF_NT) {               // T2 = D S
            const int r = e / n, c = e - r * n;
            double x = 0.0;
            for (int k = 0; k < n; ++k) x += T1[r * ld + k] * S[k * n + c];
            T2[r * ld + c] = x;
        }
        __syncthreads();
        for (int e = tid; e < nn; e += SCF_NT) {               // F D S
            const int r = e / n, c = e - r * n;
            double x = 0.0;
            for (int k = 0; k < n; ++k) x += T0[r * ld + k] * T2[k * ld + c];
            Es[e] = x;
        }
        __syncthreads();
        for (int e = tid; e < nn; e += SCF_NT) {               // T2 = D F
            const int r = e / n, c = e - r * n;
            double x = 0.0;
            for (int k = 0; k < n; ++k) x += T1[r * ld + k] * T0[k * ld + c];
            T2[r * ld + c] = x;
        }
        __syncthreads();
        for (int e = tid; e < nn; e += SCF_NT) {               // e = F D S - S (D F)
            const int r = e / n, c = e - r * n;
            double x = 0.0;
            for (int k = 0; k < n; ++k) x += S[r * n + k] * T2[k * ld + c];
            const double ev = Es[e] - x;
            Es[e] = ev;
            maxerr = fmax(maxerr, fabs(ev));
        }
        maxerr = scf_block_max(maxerr, red);                   // (its barriers make the new e visible to the block)
        // ---- DIIS: B[slot][j] = <e_slot, e_j> over the history, the bordered system, its solve ----
        {
            double part[SCF_HIST];
#pragma unroll
            for (int j = 0; j < SCF_HIST; ++j) part[j] = 0.0;
            for (int e = tid; e < nn; e += SCF_NT) {
                const double ev = Es[e];
#pragma unroll
                for (int j = 0; j < SCF_HIST; ++j)
                    if (j < m) part[j] += ev * Eh[(size_t)j * nn + e];
            }
#pragma unroll
            for (int j = 0; j < SCF_HIST; ++j) {
                if (j < m) {
                    const double x = scf_block_sum(part[j], red);
                    if (tid == 0) { Bm[slot * SCF_HIST + j] = x; Bm[j * SCF_HIST + slot] = x; }
                }
            }
        }
        if (m > 1) {                                           // (the first iteration has nothing to extrapolate from)
            __syncthreads();
            if (tid == 0) {
                // rows / columns oldest to newest, the constraint last (gaussian.rhf); Gaussian elimination with
                // partial pivoting; an exactly singular system (numpy's LinAlgError) keeps the plain F
                const int w = m + 2;
                for (int i = 0; i < m; ++i) {
                    const int si = (it - m + 1 + i) % SCF_HIST;
                    for (int j = 0; j < m; ++j) sys[i * w + j] = Bm[si * SCF_HIST + (it - m + 1 + j) % SCF_HIST];
                    sys[i * w + m] = -1.0;
                    sys[m * w + i] = -1.0;
                    sys[i * w + m + 1] = 0.0;
                }
                sys[m * w + m] = 0.0;
                sys[m * w + m + 1] = -1.0;
                bool ok = true;
                for (int c = 0; c <= m && ok; ++c) {
                    int piv = c;
                    for (int r = c + 1; r <= m; ++r)
                        if (fabs(sys[r * w + c]) > fabs(sys[piv * w + c])) piv = r;
                    if (!(fabs(sys[piv * w + c]) > 0.0)) { ok = false; break; }
                    if (piv != c)
                        for (int j = c; j < w; ++j) {
                            const double t = sys[c * w + j]; sys[c * w + j] = sys[piv * w + j]; sys[piv * w + j] = t;
                        }
                    for (int r = c + 1; r <= m; ++r) {
                        const double f = sys[r * w + c] / sys[c * w + c];
                        for (int j = c; j < w; ++j) sys[r * w + j] -= f * sys[c * w + j];
                    }
                }
                if (ok) {
                    for (int r = m; r >= 0; --r) {
                        double x = sys[r * w + m + 1];
                        for (int j = r + 1; j <= m; ++j) x -= sys[r * w + j] * sys[j * w + m + 1];
                        x /= sys[r * w + r];
                        sys[r * w + m + 1] = x;
                        if (!isfinite(x)) ok = false;
                    }
                }
                for (int i = 0; i < m; ++i) wts[i] = ok ? sys[i * w + m + 1] : 0.0;
                wts[SCF_HIST] = ok ? 1.0 : 0.0;
            }
            __syncthreads();
            if (wts[SCF_HIST] != 0.0) {
                for (int e = tid; e < nn; e += SCF_NT) {
                    double x = 0.0;
                    for (int i = 0; i < m; ++i) x += wts[i] * Fh[(size_t)((it - m + 1 + i) % SCF_HIST) * nn + e];
                    const int r = e / n, c = e - r * n;
                    T0[r * ld + c] = x;
                }
            }
        }
    }
    // ---- A = X^T F X (lower triangle, mirrored: exactly symmetric), its eigenvectors c, C = X c ----
    __syncthreads();
    for (int e = tid; e < nn; e += SCF_NT) {                   // T1 = F X
        const int r = e / n, c = e - r * n;
        double x = 0.0;
        for (int k = 0; k < n; ++k) x += T0[r * ld + k] * X[k * n + c];
        T1[r * ld + c] = x;
    }
    __syncthreads();
    for (int e = tid; e < nn; e += SCF_NT) {
        const int r = e / n, c = e - r * n;
        if (r >= c) {
            double x = 0.0;
            for (int k = 0; k < n; ++k) x += X[k * n + r] * T1[k * ld + c];
            T2[r * ld + c] = x;
            T2[c * ld + r] = x;
        }
        T0[r * ld + c] = (r == c) ? 1.0 : 0.0;
    }
    __syncthreads();
    if (tid < JACOBI_NT) {                                     // (wave 0)
        sym_jacobi_wave(T2, T0, cs, pq, n, ld, tid);
        scf_eig_sorted(T2, T0, n, ld, tid, a.mo_energy + (size_t)b * n, T1, ld, a.oao_mo_coeff + (size_t)b * nn, n);
    }
    __syncthreads();
    for (int e = tid; e < nn; e += SCF_NT) {                   // C = X c
        const int r = e / n, c = e - r * n;
        double x = 0.0;
        for (int k = 0; k < n; ++k) x += X[r * n + k] * T1[k * ld + c];
        T2[r * ld + c] = x;
        a.mo_coeff[(size_t)b * nn + e] = x;
    }
    __syncthreads();
    for (int e = tid; e < nn; e += SCF_NT) {                   // D = 2 C_occ C_occ^T
        const int r = e / n, c = e - r * n;
        double x = 0.0;
        for (int o = 0; o < a.n_occ; ++o) x += T2[r * ld + o] * T2[c * ld + o];
        D[e] = 2.0 * x;
    }
    if (tid == 0 && it >= 0) {
        const bool conv = fabs(energy - scal[0]) < a.conv_tol && maxerr < a.err_tol;
        scal[0] = energy;
        a.e_elec[b] = energy;
        a.diis_error[b] = maxerr;
        a.iterations[b] = it + 1;
        if (conv || it + 1 >= a.max_cycle) {
            a.info[b] = conv ? 0 : 1;
            a.status[b] = 1;
            atomicAdd(a.done, 1);
        }
    }
}

static size_t scf_step_lds(int n) { return (3 * (size_t)n * (n | 1) + 512) * sizeof(double); }

static int scf_check_sizes(const char* who, int n, int batch)
{
    OOVQE_REQUIRE(n >= 2 && n <= OOVQE_INVSQRT_MAX_N, "%s: n = %d (2 .. %d)", who, n, OOVQE_INVSQRT_MAX_N);
    OOVQE_REQUIRE(batch >= 1, "%s: batch = %d", who, batch);
    return 0;
}

extern "C" int64_t oovqe_rhf_work_size(int n, int batch)
{
    if (scf_check_sizes("oovqe_rhf_work_size", n, batch) != 0) return OOVQE_ERR_ARG;
    return (int64_t)batch * ((int64_t)scf_geom_doubles(n) + (int64_t)n * n) + (2 * (int64_t)batch + 2 + 1) / 2;
}

extern "C" int oovqe_rhf_batch(const double* h, const double* g, const double* s, const double* x, int n, int n_occ,
                               int batch, double conv_tol, double err_tol, int max_cycle, double* mo_coeff,
                               double* oao_mo_coeff, double* mo_energy, double* e_elec, double* diis_error,
                               int* iterations, int* info, double* work, int* verdict_host, oovqe_stream_t stream)
{
    const char* who = "oovqe_rhf_batch";
    if (scf_check_sizes(who, n, batch) != 0) return OOVQE_ERR_ARG;
    OOVQE_REQUIRE(n_occ >= 1 && n_occ < n, "%s: n_occ = %d (1 .. n - 1 = %d)", who, n_occ, n - 1);
    OOVQE_REQUIRE(max_cycle >= 1, "%s: max_cycle = %d", who, max_cycle);
    OOVQE_REQUIRE(conv_tol > 0.0 && err_tol > 0.0, "%s: conv_tol and err_tol must be positive", who);
    OOVQE_REQUIRE(h && g && s && mo_coeff && oao_mo_coeff && mo_energy && e_elec && diis_error && iterations && info
                  && work, "%s: null pointer", who);
    hipStream_t st = (hipStream_t)stream;
    const size_t nn = (size_t)n * n, per = scf_geom_doubles(n);
    double* xw = work + (size_t)batch * per;              // S^-1/2 [batch][n][n] when the caller gives none
    int* ints = reinterpret_cast<int*>(xw + (size_t)batch * nn);
    int* status = ints;
    int* x_info = ints + batch;
    int* done = ints + 2 * (size_t)batch;
    OOVQE_CHECK_HIP(hipMemsetAsync(ints, 0, (2 * (size_t)batch + 2) * sizeof(int), st), who);
    OOVQE_CHECK_HIP(hipMemsetAsync(iterations, 0, (size_t)batch * sizeof(int), st), who);
    if (x == nullptr) {
        const int rc = oovqe_sym_invsqrt_batch(s, n, batch, xw, x_info, stream);
        if (rc != 0) return rc;
    }
    scf_step_t a;
    a.h = h; a.s = s; a.x = x ? x : xw; a.x_info = x ? nullptr : x_info; a.work = work; a.status = status;
    a.done = done; a.mo_coeff = mo_coeff; a.oao_mo_coeff = oao_mo_coeff; a.mo_energy = mo_energy; a.e_elec = e_elec;
    a.diis_error = diis_error; a.iterations = iterations; a.info = info;
    a.conv_tol = conv_tol; a.err_tol = err_tol; a.n = n; a.n_occ = n_occ; a.max_cycle = max_cycle;
    const size_t lds = scf_step_lds(n);
    if (oovqe_ensure_dynamic_lds(reinterpret_cast<const void*>(&scf_step_kernel), lds) != 0) return OOVQE_ERR_HIP;
    a.it = -1;
    hipLaunchKernelGGL(scf_step_kernel, dim3(batch), dim3(SCF_NT), lds, st, a);
    OOVQE_CHECK_LAUNCH("scf_step_kernel");

    // The loop runs SCF_CHECK_EVERY iterations ahead of the host's look at the count of finished geometries: the count
    // after block i is read (pinned memory, one event) once block i + 1 is enqueued, so the queue never drains; the
    // extra launches find every geometry frozen and leave at once.
    hipEvent_t ev[2] = {nullptr, nullptr};
    int local[2] = {0, 0};
    int* verdict = verdict_host ? verdict_host : local;
    if (verdict_host) {
        OOVQE_CHECK_HIP(hipEventCreateWithFlags(&ev[0], hipEventDisableTiming), who);
        OOVQE_CHECK_HIP(hipEventCreateWithFlags(&ev[1], hipEventDisableTiming), who);
    }
    int rc = 0, it = 0, slot = 0;
    bool pending = false, recorded[2] = {false, false};
    while (it < max_cycle && rc == 0) {
        const int end = it + SCF_CHECK_EVERY < max_cycle ? it + SCF_CHECK_EVERY : max_cycle;
        for (; it < end && rc == 0; ++it) {
            rc = scf_launch_fock(g, work, per, n, batch, status, work + nn, work + 2 * nn, per, st);
            if (rc != 0) break;
            a.it = it;
            hipLaunchKernelGGL(scf_step_kernel, dim3(batch), dim3(SCF_NT), lds, st, a);
            if (hipGetLastError() != hipSuccess) { oovqe_set_error("%s: scf_step_kernel launch failed", who); rc = OOVQE_ERR_HIP; }
        }
        if (rc != 0) break;
        if (verdict_host) {
            if (hipMemcpyAsync(&verdict[slot], done, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipEventRecord(ev[slot], st) != hipSuccess) { oovqe_set_error("%s: verdict copy failed", who); rc = OOVQE_ERR_HIP; break; }
            recorded[slot] = true;
            if (pending) {
                if (hipEventSynchronize(ev[slot ^ 1]) != hipSuccess) { oovqe_set_error("%s: event wait failed", who); rc = OOVQE_ERR_HIP; break; }
                if (verdict[slot ^ 1] >= batch) break;
            }
            pending = true;
            slot ^= 1;
        } else {
            if (hipMemcpyAsync(&local[0], done, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess) { oovqe_set_error("%s: verdict copy failed", who); rc = OOVQE_ERR_HIP; break; }
            if (local[0] >= batch) break;
        }
    }
    if (verdict_host) {
        // the last copy into the caller's pinned words must have landed before they can be reused
        for (int k = 0; k < 2; ++k)
            if (recorded[k] && hipEventSynchronize(ev[k]) != hipSuccess && rc == 0) {
                oovqe_set_error("%s: event wait failed", who);
                rc = OOVQE_ERR_HIP;
            }
        (void)hipEventDestroy(ev[0]);
        (void)hipEventDestroy(ev[1]);
    }
    return rc;
}
