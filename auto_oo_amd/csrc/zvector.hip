// Orbital response of CASCI states on canonical RHF orbitals for a stack of geometries (gfx950): the Z-vector
// (Handy-Schaefer) solve  A z = b,  (A k)_ai = (eps_a - eps_i) k_ai + [C^T G[dD(k)] C]_ai,  G[D] = J[D] - K[D] / 2,
// dD(k) = 2 (C_v k C_o^T + C_o k^T C_v^T),  by conjugate gradients preconditioned with 1 / (eps_a - eps_i), nset
// right-hand sides per geometry.
//
//   fock_jk_sets_kernel   J and K of nset densities per geometry in ONE pass over the tensor, the scheme of
//                         scf_fock_jk_kernel (scf.hip): one workgroup per (geometry, p), one wave per slab g[p,q,:,:].
//                         The slab goes through LDS once; on the way in every live set takes its J[p,q] = <slab, D_s>,
//                         on the way out its partial row slab . D_s[q,:] of K[p,:]; the partial rows of the waves are
//                         summed through LDS in a fixed order.  The sums of a set are carried in registers of their own
//                         (the number of sets is a template parameter) and run over the same elements in the same
//                         order whatever nset, so a set has the same bits alone, among others and at any place.  No
//                         floating-point atomics, every output written once.
//   zvector_step_kernel   one workgroup per (geometry, set): everything between two Fock contractions of an iteration
//                         (A p from J and K, alpha, x, r, the convergence test, the preconditioner, beta, the new
//                         direction and its AO trial density).  A set that has finished is frozen: both kernels leave at
//                         once for it and none of its outputs is touched again.
//   response_d2_kernel    D2 -= sym8[2 Z_pq D0_rs - Z_pr D0_qs] in place: a thread takes one canonical quadruple
//                         (p >= q, r >= s, pq >= rs), reads its element once and stores the result to its (up to 8)
//                         places, as cas_ao_densities_kernel does.
//
// LDS at n = 64: the Fock kernel four slabs [n][n | 1] = 130 KB; the step kernel three matrices [n][n | 1] and two
// vectors of n_occ n_virt <= 1024 doubles = 113.6 KB; the density kernel two matrices [n][n] = 64 KB (limit 160 KB).
#include "common.h"
#include <math.h>

#define ZV_NT 256
#define ZV_NW (ZV_NT / 64)
#define ZV_MAX_SETS 10          // OOVQE_ZVECTOR_MAX_SETS
#define ZV_CHECK_EVERY 4        // iterations between two looks of the host at the count of finished sets
#define ZV_SCAL 8               // per (geometry, set): [0] r . M^-1 r

// ---- Fock contraction of several densities ----------------------------------------------------------------------------
// NS: the sets of the call, a compile-time count, so that a set's sums live in registers and a call pays for its own
// sets only; the arithmetic of a set is the same in every instantiation.
template <int NS>
__global__ __launch_bounds__(ZV_NT) void fock_jk_sets_kernel(const double* __restrict__ g, const double* __restrict__ D,
                                                             int n, const int* __restrict__ status,
                                                             double* __restrict__ J, double* __restrict__ K)
{
    extern __shared__ double lds[];
    const int p = blockIdx.x, b = blockIdx.y;
    unsigned live = (1u << NS) - 1u;
    if (status != nullptr) {
        live = 0;
#pragma unroll
        for (int s = 0; s < NS; ++s)
            if (status[(size_t)b * NS + s] == 0) live |= 1u << s;
        live = __builtin_amdgcn_readfirstlane(live);
        if (live == 0) return;
    }
    const int ld = n | 1, nn = n * n;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double* slab = lds + (size_t)wave * n * ld;
    const double* Db = D + (size_t)b * NS * nn;
    const double* gp = g + ((size_t)b * n + p) * (size_t)n * nn;
    const int dq = 64 / n, dr = 64 - dq * n;              // a step of 64 elements in (row, column)
    const int r0 = lane / n, c0 = lane - r0 * n;
    double kacc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) kacc[s] = 0.0;
    for (int q = wave; q < n; q += ZV_NW) {
        const double* sl = gp + (size_t)q * nn;
        double jacc[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) jacc[s] = 0.0;
        int r = r0, c = c0;
        for (int k0 = lane; k0 < nn; k0 += 4 * 64) {
            double v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + 64 * j;
                v[j] = (k < nn) ? sl[k] : 0.0;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + 64 * j;
                if (k < nn) {
                    slab[r * ld + c] = v[j];
#pragma unroll
                    for (int s = 0; s < NS; ++s) jacc[s] += v[j] * Db[s * nn + k];
                }
                c += dr; r += dq;
                if (c >= n) { c -= n; ++r; }
            }
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            double x = jacc[s];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
            if (lane == 0 && (live & (1u << s))) J[((size_t)b * NS + s) * nn + (size_t)p * n + q] = x;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        if (lane < n) {
            const double* drow = Db + (size_t)q * n;
            for (int t = 0; t < n; ++t) {
                const double x = slab[lane * ld + t];
#pragma unroll
                for (int s = 0; s < NS; ++s) kacc[s] += x * drow[s * nn + t];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
    __syncthreads();                                       // every slab is consumed: the partial rows take their place
#pragma unroll
    for (int s = 0; s < NS; ++s) lds[(s * ZV_NW + wave) * 64 + lane] = (lane < n) ? kacc[s] : 0.0;
    __syncthreads();
    const int t = threadIdx.x;
    if (t < n) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            double x = lds[(s * ZV_NW) * 64 + t];
#pragma unroll
            for (int w = 1; w < ZV_NW; ++w) x += lds[(s * ZV_NW + w) * 64 + t];
            if (live & (1u << s)) K[((size_t)b * NS + s) * nn + (size_t)p * n + t] = x;
        }
    }
}

static size_t zv_fock_lds(int n, int nset)
{
    const size_t a = (size_t)ZV_NW * n * (n | 1), b = (size_t)nset * ZV_NW * 64;
    return (a > b ? a : b) * sizeof(double);
}

template <int NS>
static int zv_launch_fock_ns(const double* g, const double* D, int n, int batch, const int* status, double* J, double* K,
                             hipStream_t st)
{
    const size_t lds = zv_fock_lds(n, NS), nn = (size_t)n * n;
    if (oovqe_ensure_dynamic_lds(reinterpret_cast<const void*>(&fock_jk_sets_kernel<NS>), lds) != 0) return OOVQE_ERR_HIP;
    for (int b0 = 0; b0 < batch; b0 += 65535) {            // (grid.y limit)
        const int nb = batch - b0 < 65535 ? batch - b0 : 65535;
        hipLaunchKernelGGL(fock_jk_sets_kernel<NS>, dim3(n, nb), dim3(ZV_NT), lds, st, g + (size_t)b0 * nn * nn,
                           D + (size_t)b0 * NS * nn, n, status ? status + (size_t)b0 * NS : nullptr,
                           J + (size_t)b0 * NS * nn, K + (size_t)b0 * NS * nn);
        OOVQE_CHECK_LAUNCH("fock_jk_sets_kernel");
    }
    return 0;
}

static int zv_launch_fock(const double* g, const double* D, int n, int nset, int batch, const int* status, double* J,
                          double* K, hipStream_t st)
{
    switch (nset) {
#define ZV_CASE(NS) case NS: return zv_launch_fock_ns<NS>(g, D, n, batch, status, J, K, st);
        ZV_CASE(1) ZV_CASE(2) ZV_CASE(3) ZV_CASE(4) ZV_CASE(5) ZV_CASE(6) ZV_CASE(7) ZV_CASE(8) ZV_CASE(9) ZV_CASE(10)
#undef ZV_CASE
    }
    return OOVQE_ERR_ARG;
}

extern "C" int oovqe_fock_jk_sets_batch(const double* g, const double* d, int n, int nset, int batch, double* j,
                                        double* k, oovqe_stream_t stream)
{
    const char* who = "oovqe_fock_jk_sets_batch";
    OOVQE_REQUIRE(n >= 1 && n <= OOVQE_INVSQRT_MAX_N, "%s: n = %d (1 .. %d)", who, n, OOVQE_INVSQRT_MAX_N);
    OOVQE_REQUIRE(nset >= 1 && nset <= ZV_MAX_SETS, "%s: nset = %d (1 .. %d)", who, nset, ZV_MAX_SETS);
    OOVQE_REQUIRE(batch >= 0, "%s: batch = %d", who, batch);
    OOVQE_REQUIRE(g && d && j && k, "%s: null pointer", who);
    if (batch == 0) return 0;
    return zv_launch_fock(g, d, n, nset, batch, nullptr, j, k, (hipStream_t)stream);
}

// ---- conjugate-gradient step ------------------------------------------------------------------------------------------
struct zv_step_t {
    const double* mo_coeff;                // [batch][n][n] AO x MO, the first n_occ columns doubly occupied
    const double* mo_energy;               // [batch][n]
    const double* b;                       // [batch][nset][n_virt][n_occ]
    double *dt, *j, *k;                    // trial density and its J, K [batch][nset][n][n]
    double* vec;                           // per (geometry, set): r, p [n_virt n_occ] each, ZV_SCAL scalars
    int* status;                           // [batch][nset] 0 running, 1 frozen
    int* done;                             // count of frozen sets
    double* z; double* resid; int* iterations; int* info;
    double tol;
    int n, n_occ, nset, it, max_iter;      // it = -1: the start
};

__host__ __device__ static inline size_t zv_vec_doubles(int n, int n_occ)
{
    return 2 * (size_t)n_occ * (n - n_occ) + ZV_SCAL;
}

// sum / maximum over the workgroup, the same bits in every thread (butterfly inside a wave, waves in order)
__device__ __forceinline__ double zv_block_sum(double v, double* red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double x = red[0];
#pragma unroll
    for (int w = 1; w < ZV_NW; ++w) x += red[w];
    return x;
}

__device__ __forceinline__ double zv_block_max(double v, double* red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double x = red[0];
#pragma unroll
    for (int w = 1; w < ZV_NW; ++w) x = fmax(x, red[w]);
    return x;
}

// the set ends: with a failure code every output NaN; frozen
__device__ void zv_finish(const zv_step_t& a, int e, int code, int iterations, double resid)
{
    const int nvo = a.n_occ * (a.n - a.n_occ);
    if (code < 0) {
        const double nan = __builtin_nan("");
        for (int k = threadIdx.x; k < nvo; k += ZV_NT) a.z[(size_t)e * nvo + k] = nan;
        resid = nan;
    }
    if (threadIdx.x == 0) {
        a.resid[e] = resid;
        a.iterations[e] = iterations;
        a.info[e] = code;
        a.status[e] = 1;
        atomicAdd(a.done, 1);
    }
}

__global__ __launch_bounds__(ZV_NT) void zvector_step_kernel(const zv_step_t a)
{
    extern __shared__ double lds[];
    const int e = blockIdx.x, tid = threadIdx.x;
    if (a.status[e] != 0) return;
    const int n = a.n, nn = n * n, ld = n | 1, no = a.n_occ, nv = n - no, nvo = no * nv, it = a.it;
    const int b = e / a.nset;
    double* Cs = lds;                                  // C [n][ld]
    double* M = Cs + (size_t)n * ld;                   // J - K / 2 [n][ld]
    double* T1 = M + (size_t)n * ld;                   // [n][ld], n_occ columns used
    double* pl = T1 + (size_t)n * ld;                  // direction [n_virt][n_occ]
    double* ap = pl + nvo;                             // A p
    double* red = ap + nvo;                            // [8] reductions
    const double* C = a.mo_coeff + (size_t)b * nn;
    const double* eps = a.mo_energy + (size_t)b * n;
    const double* rhs = a.b + (size_t)e * nvo;
    double* x = a.z + (size_t)e * nvo;
    double* r = a.vec + (size_t)e * zv_vec_doubles(n, no);
    double* pg = r + nvo;
    double* scal = pg + nvo;
    double* Dt = a.dt + (size_t)e * nn;

    double bad = 0.0;
    for (int k = tid; k < nn; k += ZV_NT) {
        const double c = C[k];
        if (!isfinite(c)) bad = 1.0;
        const int rr = k / n, cc = k - rr * n;
        Cs[rr * ld + cc] = c;
    }
    double rz_new, rnorm;
    if (it < 0) {
        // ---- start: inputs finite, every eps_a - eps_i positive; x = 0, r = b, p = M^-1 r ----
        double gap = 0.0, rr = 0.0, rz = 0.0;
        for (int k = tid; k < n; k += ZV_NT)
            if (!isfinite(eps[k])) bad = 1.0;
        for (int k = tid; k < nvo; k += ZV_NT) {
            const int av = k / no, i = k - av * no;
            const double d = eps[no + av] - eps[i], bv = rhs[k];
            if (!isfinite(bv)) bad = 1.0;
            if (!(d > 0.0)) gap = 1.0;
            const double zz = bv / d;
            x[k] = 0.0;
            r[k] = bv;
            pg[k] = zz;
            pl[k] = zz;
            rr += bv * bv;
            rz += bv * zz;
        }
        bad = zv_block_max(bad, red);
        if (bad != 0.0) { zv_finish(a, e, -3, 0, 0.0); return; }
        gap = zv_block_max(gap, red);
        if (gap != 0.0) { zv_finish(a, e, -2, 0, 0.0); return; }       // (an occupied orbital above a virtual one)
        rnorm = sqrt(zv_block_sum(rr, red));
        rz_new = zv_block_sum(rz, red);
        if (rnorm <= a.tol) { zv_finish(a, e, 0, 0, rnorm); return; }
    } else {
        // ---- A p = (eps_a - eps_i) p + C_v^T (J - K / 2) C_o ----
        const double* J = a.j + (size_t)e * nn;
        const double* K = a.k + (size_t)e * nn;
        for (int k = tid; k < nn; k += ZV_NT) {
            const double m = J[k] - 0.5 * K[k];
            if (!isfinite(m)) bad = 1.0;
            const int rr = k / n, cc = k - rr * n;
            M[rr * ld + cc] = m;
        }
        for (int k = tid; k < nvo; k += ZV_NT) pl[k] = pg[k];
        bad = zv_block_max(bad, red);
        if (bad != 0.0) { zv_finish(a, e, -3, it + 1, 0.0); return; }   // (NaN or Inf in the two-electron integrals)
        for (int k = tid; k < n * no; k += ZV_NT) {                     // T1 = M C_o
            const int rr = k / no, i = k - rr * no;
            double s = 0.0;
            for (int c = 0; c < n; ++c) s += M[rr * ld + c] * Cs[c * ld + i];
            T1[rr * ld + i] = s;
        }
        __syncthreads();
        double pap = 0.0;
        for (int k = tid; k < nvo; k += ZV_NT) {
            const int av = k / no, i = k - av * no;
            double s = 0.0;
            for (int c = 0; c < n; ++c) s += Cs[c * ld + no + av] * T1[c * ld + i];
            const double v = (eps[no + av] - eps[i]) * pl[k] + s;
            ap[k] = v;
            pap += pl[k] * v;
        }
        pap = zv_block_sum(pap, red);
        const double rz = scal[0];
        if (!isfinite(pap)) { zv_finish(a, e, -3, it + 1, 0.0); return; }
        if (!(pap > 0.0)) { zv_finish(a, e, -2, it + 1, 0.0); return; }     // (A is not positive definite)
        const double alpha = rz / pap;
        double rr = 0.0, rzn = 0.0;
        for (int k = tid; k < nvo; k += ZV_NT) {
            const int av = k / no, i = k - av * no;
            x[k] += alpha * pl[k];
            const double rv = r[k] - alpha * ap[k];
            r[k] = rv;
            const double zz = rv / (eps[no + av] - eps[i]);
            ap[k] = zz;                                                 // (A p is consumed: M^-1 r takes its place)
            rr += rv * rv;
            rzn += rv * zz;
        }
        rnorm = sqrt(zv_block_sum(rr, red));
        rz_new = zv_block_sum(rzn, red);
        if (!isfinite(rnorm)) { zv_finish(a, e, -3, it + 1, 0.0); return; }
        if (rnorm <= a.tol || it + 1 >= a.max_iter) { zv_finish(a, e, rnorm <= a.tol ? 0 : 1, it + 1, rnorm); return; }
        const double beta = rz_new / rz;
        for (int k = tid; k < nvo; k += ZV_NT) {
            const double pv = ap[k] + beta * pl[k];
            pl[k] = pv;
            pg[k] = pv;
        }
    }
    // ---- the trial density dD(p) = 2 (C_v p C_o^T + C_o p^T C_v^T) ----
    __syncthreads();
    for (int k = tid; k < n * no; k += ZV_NT) {                         // T1 = C_v p
        const int rr = k / no, i = k - rr * no;
        double s = 0.0;
        for (int av = 0; av < nv; ++av) s += Cs[rr * ld + no + av] * pl[av * no + i];
        T1[rr * ld + i] = s;
    }
    __syncthreads();
    for (int k = tid; k < nn; k += ZV_NT) {
        const int rr = k / n, cc = k - rr * n;
        double s = 0.0;
        for (int i = 0; i < no; ++i) s += T1[rr * ld + i] * Cs[cc * ld + i] + Cs[rr * ld + i] * T1[cc * ld + i];
        Dt[k] = 2.0 * s;
    }
    if (tid == 0) {
        scal[0] = rz_new;
        a.resid[e] = rnorm;
        a.iterations[e] = it + 1;
    }
}

static size_t zv_step_lds(int n, int n_occ)
{
    return (3 * (size_t)n * (n | 1) + 2 * (size_t)n_occ * (n - n_occ) + 8) * sizeof(double);
}

static int zv_check_sizes(const char* who, int n, int n_occ, int nset, int batch)
{
    OOVQE_REQUIRE(n >= 2 && n <= OOVQE_INVSQRT_MAX_N, "%s: n = %d (2 .. %d)", who, n, OOVQE_INVSQRT_MAX_N);
    OOVQE_REQUIRE(n_occ >= 1 && n_occ < n, "%s: n_occ = %d (1 .. n - 1 = %d)", who, n_occ, n - 1);
    OOVQE_REQUIRE(nset >= 1 && nset <= ZV_MAX_SETS, "%s: nset = %d (1 .. %d)", who, nset, ZV_MAX_SETS);
    OOVQE_REQUIRE(batch >= 1 && (int64_t)batch * nset < (int64_t)1 << 30, "%s: batch = %d", who, batch);
    return 0;
}

extern "C" int64_t oovqe_zvector_work_size(int n, int n_occ, int nset, int batch)
{
    if (zv_check_sizes("oovqe_zvector_work_size", n, n_occ, nset, batch) != 0) return OOVQE_ERR_ARG;
    const int64_t sets = (int64_t)batch * nset;
    return sets * (3 * (int64_t)n * n + (int64_t)zv_vec_doubles(n, n_occ)) + (sets + 2 + 1) / 2;
}

extern "C" int oovqe_zvector_solve_batch(const double* g, const double* mo_coeff, const double* mo_energy, int n,
                                         int n_occ, int nset, int batch, const double* b, double tol, int max_iter,
                                         double* z, double* resid, int* iterations, int* info, double* work,
                                         int* verdict_host, oovqe_stream_t stream)
{
    const char* who = "oovqe_zvector_solve_batch";
    if (zv_check_sizes(who, n, n_occ, nset, batch) != 0) return OOVQE_ERR_ARG;
    OOVQE_REQUIRE(max_iter >= 1, "%s: max_iter = %d", who, max_iter);
    OOVQE_REQUIRE(tol > 0.0, "%s: tol must be positive", who);
    OOVQE_REQUIRE(g && mo_coeff && mo_energy && b && z && resid && iterations && info && work, "%s: null pointer", who);
    hipStream_t st = (hipStream_t)stream;
    const size_t nn = (size_t)n * n, sets = (size_t)batch * nset;
    zv_step_t a;
    a.mo_coeff = mo_coeff; a.mo_energy = mo_energy; a.b = b;
    a.dt = work; a.j = work + sets * nn; a.k = work + 2 * sets * nn; a.vec = work + 3 * sets * nn;
    int* ints = reinterpret_cast<int*>(a.vec + sets * zv_vec_doubles(n, n_occ));
    a.status = ints; a.done = ints + sets;
    a.z = z; a.resid = resid; a.iterations = iterations; a.info = info;
    a.tol = tol; a.n = n; a.n_occ = n_occ; a.nset = nset; a.max_iter = max_iter;
    OOVQE_CHECK_HIP(hipMemsetAsync(ints, 0, (sets + 2) * sizeof(int), st), who);
    OOVQE_CHECK_HIP(hipMemsetAsync(iterations, 0, sets * sizeof(int), st), who);
    const size_t lds = zv_step_lds(n, n_occ);
    if (oovqe_ensure_dynamic_lds(reinterpret_cast<const void*>(&zvector_step_kernel), lds) != 0) return OOVQE_ERR_HIP;
    a.it = -1;
    hipLaunchKernelGGL(zvector_step_kernel, dim3((unsigned)sets), dim3(ZV_NT), lds, st, a);
    OOVQE_CHECK_LAUNCH("zvector_step_kernel");

    // As oovqe_rhf_batch: the loop runs ZV_CHECK_EVERY iterations ahead of the host's look at the count of finished
    // sets (pinned memory, one event), so the queue never drains; the extra launches find every set frozen.
    hipEvent_t ev[2] = {nullptr, nullptr};
    int local[2] = {0, 0};
    int* verdict = verdict_host ? verdict_host : local;
    if (verdict_host) {
        OOVQE_CHECK_HIP(hipEventCreateWithFlags(&ev[0], hipEventDisableTiming), who);
        OOVQE_CHECK_HIP(hipEventCreateWithFlags(&ev[1], hipEventDisableTiming), who);
    }
    int rc = 0, it = 0, slot = 0;
    bool pending = false, recorded[2] = {false, false};
    while (it < max_iter && rc == 0) {
        const int end = it + ZV_CHECK_EVERY < max_iter ? it + ZV_CHECK_EVERY : max_iter;
        for (; it < end && rc == 0; ++it) {
            rc = zv_launch_fock(g, a.dt, n, nset, batch, a.status, a.j, a.k, st);
            if (rc != 0) break;
            a.it = it;
            hipLaunchKernelGGL(zvector_step_kernel, dim3((unsigned)sets), dim3(ZV_NT), lds, st, a);
            if (hipGetLastError() != hipSuccess) { oovqe_set_error("%s: zvector_step_kernel launch failed", who); rc = OOVQE_ERR_HIP; }
        }
        if (rc != 0) break;
        if (verdict_host) {
            if (hipMemcpyAsync(&verdict[slot], a.done, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipEventRecord(ev[slot], st) != hipSuccess) { oovqe_set_error("%s: verdict copy failed", who); rc = OOVQE_ERR_HIP; break; }
            recorded[slot] = true;
            if (pending) {
                if (hipEventSynchronize(ev[slot ^ 1]) != hipSuccess) { oovqe_set_error("%s: event wait failed", who); rc = OOVQE_ERR_HIP; break; }
                if (verdict[slot ^ 1] >= (int)sets) break;
            }
            pending = true;
            slot ^= 1;
        } else {
            if (hipMemcpyAsync(&local[0], a.done, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess) { oovqe_set_error("%s: verdict copy failed", who); rc = OOVQE_ERR_HIP; break; }
            if (local[0] >= (int)sets) break;
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

// ---- the Lagrangian's part of the AO two-particle density -------------------------------------------------------------
// One workgroup per (p, row): the pairs (p, q <= p) one after the other, the threads over the pairs rs <= pq.
__global__ __launch_bounds__(ZV_NT) void response_d2_kernel(const double* __restrict__ Zm, const double* __restrict__ D0m,
                                                            int n, double* __restrict__ d2m, size_t row_stride)
{
    extern __shared__ double lds[];
    double* Z = lds;                         // [n][n]
    double* D = Z + (size_t)n * n;           // [n][n]
    const int p = blockIdx.x, row = blockIdx.y, t = threadIdx.x;
    for (int k = t; k < n * n; k += ZV_NT) {
        Z[k] = Zm[(size_t)row * n * n + k];
        D[k] = D0m[(size_t)row * n * n + k];
    }
    __syncthreads();
    const size_t n1 = (size_t)n, n2 = n1 * n1, n3 = n2 * n1;
    double* out = d2m + (size_t)row * row_stride;
    for (int q = 0; q <= p; ++q) {
        const int pq = p * (p + 1) / 2 + q;
        for (int rs = t; rs <= pq; rs += ZV_NT) {
            int r = (int)((sqrt(8.0 * (double)rs + 1.0) - 1.0) * 0.5);
            while ((r + 1) * (r + 2) / 2 <= rs) ++r;
            while (r * (r + 1) / 2 > rs) --r;
            const int s = rs - r * (r + 1) / 2;
            const double v = (Z[p * n + q] * D[r * n + s] + Z[r * n + s] * D[p * n + q])
                             - 0.25 * ((Z[p * n + r] * D[q * n + s] + Z[q * n + r] * D[p * n + s])
                                       + (Z[p * n + s] * D[q * n + r] + Z[q * n + s] * D[p * n + r]));
            const double x = out[p * n3 + q * n2 + r * n1 + s] - v;
            out[p * n3 + q * n2 + r * n1 + s] = x;
            out[q * n3 + p * n2 + r * n1 + s] = x;
            out[p * n3 + q * n2 + s * n1 + r] = x;
            out[q * n3 + p * n2 + s * n1 + r] = x;
            out[r * n3 + s * n2 + p * n1 + q] = x;
            out[s * n3 + r * n2 + p * n1 + q] = x;
            out[r * n3 + s * n2 + q * n1 + p] = x;
            out[s * n3 + r * n2 + q * n1 + p] = x;
        }
    }
}

extern "C" int oovqe_response_d2_batch(const double* z, const double* d0, int n, int64_t rows, double* d2,
                                       int64_t row_stride, oovqe_stream_t stream)
{
    const char* who = "oovqe_response_d2_batch";
    OOVQE_REQUIRE(n >= 1 && n <= OOVQE_INVSQRT_MAX_N, "%s: n = %d (1 .. %d)", who, n, OOVQE_INVSQRT_MAX_N);
    OOVQE_REQUIRE(rows >= 0, "%s: rows = %lld", who, (long long)rows);
    OOVQE_REQUIRE(z && d0 && d2, "%s: null pointer", who);
    const size_t lds = 2 * (size_t)n * n * sizeof(double), nn = (size_t)n * n;
    OOVQE_REQUIRE(row_stride >= (int64_t)(nn * nn), "%s: row_stride = %lld < n^4", who, (long long)row_stride);
    if (rows == 0) return 0;
    if (oovqe_ensure_dynamic_lds(reinterpret_cast<const void*>(&response_d2_kernel), lds) != 0) return OOVQE_ERR_HIP;
    for (int64_t r0 = 0; r0 < rows; r0 += 65535) {           // (grid.y limit)
        const int64_t nr = rows - r0 < 65535 ? rows - r0 : 65535;
        hipLaunchKernelGGL(response_d2_kernel, dim3(n, (unsigned)nr), dim3(ZV_NT), lds, (hipStream_t)stream,
                           z + (size_t)r0 * nn, d0 + (size_t)r0 * nn, n, d2 + (size_t)r0 * row_stride, (size_t)row_stride);
        OOVQE_CHECK_LAUNCH("response_d2_kernel");
    }
    return 0;
}
