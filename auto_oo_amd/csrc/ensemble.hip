// State-averaged OO-VQE: several orthonormal initial states through ONE circuit U(theta), the
// weighted RDM sets of the ensemble and its theta-theta Hessian, for a stack of parameter rows.
//
// Three kernels, dense register only (n_qubits <= OOVQE_ENSEMBLE_MAX_QUBITS: every vector is LDS-resident, D <= 1024
// amplitudes), 1 <= nstate <= OOVQE_ENSEMBLE_MAX_STATES:
//
//   ensemble_states_kernel    one workgroup per (row, state, vector): U(theta) psi0_I, its tangents and its second
//                             tangents, from an initial vector that is a superposition (the kernels of circuit.hip
//                             start from one basis state).  LDS: working vector + sum, 2 D doubles (16 KiB).
//   ensemble_rdms_kernel      one workgroup per (row, RDM set): the vectors of ALL states of the set in LDS
//                             (2 nstate D doubles <= 64 KiB), one wave per RDM element, E_pq applied on the fly by bit
//                             operations (no V[pq][x] staging: a^2 D doubles do not fit LDS at 10 qubits), every lane
//                             adding its terms of the states in the order I = 0, 1, ..., then a butterfly over the wave.
//   ensemble_hessian_kernel   one workgroup per (row, pair j <= k): psi, tau_j, tau_k, psi_jk of all states in LDS
//                             (4 nstate D doubles <= 128 KiB), the four transition sets of the definition
//                             (oovqe_circuit_hessian_assemble) element by element, contracted with c1 | c2 as they are
//                             formed, one tree reduction over the workgroup.
//
// No atomics, no reduction whose order depends on the grid: a row has the same bits wherever it stands in the stack and
// whatever the batch size; a state of weight 0 is skipped, so it contributes exactly nothing.
#include "internal.h"
#include "circuit_small.h"

namespace {

constexpr int ENS_THREADS = 256;
constexpr size_t ENS_LDS_LIMIT = 150 * 1024;

// One gate on `st` (LDS), D = 2^n amplitudes.  mode 0: the gate, 1: d/dtheta, 2: d^2/dtheta^2 = -(1/4) of the gate's
// block; a differentiated gate annihilates the amplitudes it leaves alone (apply_gate / apply_gate_mode of circuit.hip).
__device__ void ens_apply_gate(double* st, uint32_t D, const oovqe_gate_t& g, double c, double s, int mode)
{
    const uint32_t fm = g.mask_hi | g.mask_lo;
    const uint32_t npairs = D >> g.nfix;
    const double h = 0.5 * (double)g.sign;
    for (uint32_t t = threadIdx.x; t < npairs; t += ENS_THREADS) {
        const uint32_t x = deposit(t, g) | g.mask_hi;
        const uint32_t y = x ^ fm;
        if (x >= D || y >= D) continue;       // (a table made for another register never leaves the vector)
        const double pi = (__popc(x & g.mask_par) & 1) ? -1.0 : 1.0;
        const double ax = st[x], ay = st[y];
        const double nx = c * ax + pi * s * ay, ny = c * ay - pi * s * ax;
        if (mode == 0) {
            st[x] = nx;
            st[y] = ny;
        } else if (mode == 1) {
            st[x] = h * (-s * ax + pi * c * ay);
            st[y] = h * (-s * ay - pi * c * ax);
        } else {
            st[x] = -0.25 * nx;
            st[y] = -0.25 * ny;
        }
    }
    if (mode != 0) {
        for (uint32_t x = threadIdx.x; x < D; x += ENS_THREADS) {
            const uint32_t f = x & fm;
            if (f != g.mask_hi && f != g.mask_lo) st[x] = 0.0;
        }
    }
}

// w = (circuit with the gates g1 and g2 differentiated; -1: none; g1 == g2: that gate twice) psi0
__device__ void ens_run(double* w, uint32_t D, const double* __restrict__ psi0, const double* __restrict__ th,
                        int n_theta, const oovqe_gate_t* __restrict__ gates, int n_gates, int g1, int g2)
{
    for (uint32_t x = threadIdx.x; x < D; x += ENS_THREADS) w[x] = psi0[x];
    __syncthreads();
    for (int g = 0; g < n_gates; ++g) {
        const oovqe_gate_t gt = gates[g];
        if (gt.theta_idx < 0 || gt.theta_idx >= n_theta) continue;      // fixed zero angle: identity
        double s, c;
        sincos(0.5 * (double)gt.sign * th[gt.theta_idx], &s, &c);
        ens_apply_gate(w, D, gt, c, s, (g == g1) + (g == g2));
        __syncthreads();
    }
}

// grid = batch * nstate * nvec, nvec = 1 + n_theta + n_pairs; vecs [batch][nstate][nvec][D]
__global__ __launch_bounds__(ENS_THREADS)
void ensemble_states_kernel(const double* __restrict__ theta, int n_theta, const oovqe_gate_t* __restrict__ gates,
                            int n_gates, int n_qubits, const double* __restrict__ psi0, int nstate,
                            const int32_t* __restrict__ pairs, int n_pairs, double* __restrict__ vecs)
{
    extern __shared__ double ens_lds[];
    const uint32_t D = 1u << n_qubits;
    const int nvec = 1 + n_theta + n_pairs;
    const int v = (int)(blockIdx.x % (unsigned)nvec);
    const int I = (int)((blockIdx.x / (unsigned)nvec) % (unsigned)nstate);
    const size_t b = blockIdx.x / ((unsigned)nvec * (unsigned)nstate);
    const double* th = theta + b * n_theta;
    const double* p0 = psi0 + (size_t)I * D;
    double* dst = vecs + (size_t)blockIdx.x * D;
    double* w = ens_lds;          // [D] the circuit in flight
    double* acc = ens_lds + D;    // [D] the sum over the gates a parameter drives
    if (v == 0) {
        ens_run(w, D, p0, th, n_theta, gates, n_gates, -1, -1);
        for (uint32_t x = threadIdx.x; x < D; x += ENS_THREADS) dst[x] = w[x];
        return;
    }
    int j, k;
    if (v <= n_theta) {
        j = v - 1;
        k = -1;
    } else {
        j = pairs[2 * (v - 1 - n_theta)];
        k = pairs[2 * (v - 1 - n_theta) + 1];
        if (j < 0 || j >= n_theta || k < 0 || k >= n_theta) j = k = -2;       // no gate carries these: a zero vector
    }
    for (uint32_t x = threadIdx.x; x < D; x += ENS_THREADS) acc[x] = 0.0;
    for (int g1 = 0; g1 < n_gates; ++g1) {
        if (gates[g1].theta_idx != j) continue;
        if (k == -1) {
            ens_run(w, D, p0, th, n_theta, gates, n_gates, g1, -1);
            for (uint32_t x = threadIdx.x; x < D; x += ENS_THREADS) acc[x] += w[x];
            continue;
        }
        for (int g2 = 0; g2 < n_gates; ++g2) {
            if (gates[g2].theta_idx != k) continue;
            ens_run(w, D, p0, th, n_theta, gates, n_gates, g1, g2);
            for (uint32_t x = threadIdx.x; x < D; x += ENS_THREADS) acc[x] += w[x];
        }
    }
    // (every thread adds and stores the x it owns: no barrier is needed between the sums and the store)
    for (uint32_t x = threadIdx.x; x < D; x += ENS_THREADS) dst[x] = acc[x];
}

// ---- RDM elements from LDS-resident vectors ---------------------------------------------------------------------
// (E_pq v)[x], E_pq = a+_{2p} a_{2q} + a+_{2p+1} a_{2q+1}, Jordan-Wigner: spin orbital j = wire j = bit n-1-j
__device__ __forceinline__ double ens_epq(const double* v, uint32_t x, int p, int q, int n)
{
    double acc = 0.0;
#pragma unroll
    for (int sp = 0; sp < 2; ++sp) {
        const uint32_t bP = 1u << (n - 1 - (2 * p + sp)), bQ = 1u << (n - 1 - (2 * q + sp));
        if (p == q) {
            if (x & bP) acc += v[x];
        } else if ((x & bP) && !(x & bQ)) {
            const uint32_t hi = bP > bQ ? bP : bQ, lo = bP > bQ ? bQ : bP;
            const uint32_t between = (hi - 1u) & ~((lo << 1) - 1u);
            const double sgn = (__popc(x & between) & 1) ? -1.0 : 1.0;
            acc += sgn * v[x ^ (bP | bQ)];
        }
    }
    return acc;
}

// element e of the transition set T(bra, ket) WITHOUT the delta term: e < a^2: gamma[pq] = bra . E_pq ket;
// e >= a^2: (E_qp bra) . (E_rs ket) of Gamma[pqrs]; the terms x = x0, x0 + dx, ... of the sum over the register
__device__ double ens_element(const double* bra, const double* ket, uint32_t D, int n, int ncas, int e,
                              uint32_t x0 = 0, uint32_t dx = 1)
{
    const int na2 = ncas * ncas;
    double s = 0.0;
    if (e < na2) {
        const int p = e / ncas, q = e - p * ncas;
        for (uint32_t x = x0; x < D; x += dx) s += bra[x] * ens_epq(ket, x, p, q, n);
    } else {
        const int pq = (e - na2) / na2, rs = (e - na2) - pq * na2;
        const int p = pq / ncas, q = pq - p * ncas, r = rs / ncas, t = rs - r * ncas;
        for (uint32_t x = x0; x < D; x += dx) s += ens_epq(bra, x, q, p, n) * ens_epq(ket, x, r, t, n);
    }
    return s;
}

// grid = batch * per, per = n_sets + (with_st ? nstate^2 : 0).  Workgroup u of a row: u < n_sets: set u of the
// ensemble (0: sum_I w_I T(psi_I, psi_I); k: sum_I w_I (T(tau_Ik, psi_I) + T(psi_I, tau_Ik))); else the state /
// transition set [I][J] = T(psi_I, psi_J).  vecs [batch][nstate][nvec][D].
__global__ __launch_bounds__(ENS_THREADS)
void ensemble_rdms_kernel(const double* __restrict__ vecs, int nvec, const double* __restrict__ weights, int n_qubits,
                          int ncas, int nstate, int n_sets, int with_st, double* __restrict__ gamma_sa,
                          double* __restrict__ Gamma_sa, double* __restrict__ gamma_st, double* __restrict__ Gamma_st)
{
    extern __shared__ double ens_lds[];
    const uint32_t D = 1u << n_qubits;
    const int na2 = ncas * ncas, na4 = na2 * na2;
    const int per = n_sets + (with_st ? nstate * nstate : 0);
    const int u = (int)(blockIdx.x % (unsigned)per);
    const size_t b = blockIdx.x / (unsigned)per;
    const double* row = vecs + b * nstate * nvec * D;
    double* A = ens_lds;                           // [nterm][D] bras
    double* B = ens_lds + (size_t)nstate * D;      // [nterm][D] kets
    double* gam = B + (size_t)nstate * D;          // [a^2] the set's gamma, for the delta term
    int nterm, sym;
    double* g1;
    double* g2;
    if (u < n_sets) {
        nterm = nstate;
        sym = u > 0;
        for (uint32_t i = threadIdx.x; i < (uint32_t)nstate * D; i += ENS_THREADS) {
            const uint32_t I = i >> n_qubits, x = i & (D - 1);
            const double* vs = row + (size_t)I * nvec * D;
            A[i] = vs[(size_t)u * D + x];
            B[i] = vs[x];
        }
        g1 = gamma_sa + (b * n_sets + u) * na2;
        g2 = Gamma_sa + (b * n_sets + u) * na4;
    } else {
        const int IJ = u - n_sets, I = IJ / nstate, J = IJ - I * nstate;
        nterm = 1;
        sym = 0;
        for (uint32_t x = threadIdx.x; x < D; x += ENS_THREADS) {
            A[x] = row[(size_t)I * nvec * D + x];
            B[x] = row[(size_t)J * nvec * D + x];
        }
        g1 = gamma_st + (b * nstate * nstate + IJ) * na2;
        g2 = Gamma_st + (b * nstate * nstate + IJ) * na4;
    }
    __syncthreads();
    // two rounds: the one-body elements (kept in LDS for the delta term), then the two-body ones.  One WAVE per element:
    // lane l adds the terms x = l, l + 64, ... of every state in the order I = 0, 1, ..., a butterfly adds the 64
    // partial sums in a fixed order
    const uint32_t lane = threadIdx.x & 63;
    for (int round = 0; round < 2; ++round) {
        const int e0 = round ? na2 : 0, e1 = round ? na2 + na4 : na2;
        for (int e = e0 + (int)(threadIdx.x >> 6); e < e1; e += ENS_THREADS / 64) {
            double val = 0.0;
            for (int t = 0; t < nterm; ++t) {
                const double w = (u < n_sets) ? weights[t] : 1.0;
                if (w == 0.0) continue;                 // a state of weight 0 contributes exactly nothing
                const double* bra = A + (size_t)t * D;
                const double* ket = B + (size_t)t * D;
                double s = ens_element(bra, ket, D, n_qubits, ncas, e, lane, 64);
                if (sym) s += ens_element(ket, bra, D, n_qubits, ncas, e, lane, 64);
                val += w * s;
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) val += __shfl_xor(val, o, 64);
            if (lane != 0) continue;
            if (round == 0) {
                gam[e] = val;
                g1[e] = val;
            } else {
                const int pq = (e - na2) / na2, rs = (e - na2) - pq * na2;
                const int p = pq / ncas, q = pq - p * ncas, r = rs / ncas, t2 = rs - r * ncas;
                g2[e - na2] = val - (q == r ? gam[p * ncas + t2] : 0.0);
            }
        }
        __syncthreads();
    }
}

// grid = batch * n_pairs.  H[b][j][k] = H[b][k][j] = sum_I w_I sum over the four sets T(psi_I,jk, psi_I),
// T(psi_I,j, psi_I,k), T(psi_I,k, psi_I,j), T(psi_I, psi_I,jk) of c1 . gamma + c2 . Gamma.  The delta term of Gamma is
// folded into the coefficient of the one-body element: sum_pqrs c2[pqrs] (-delta_qr gamma[ps]) = -sum_ps gamma[ps]
// sum_q c2[pqqs].
__global__ __launch_bounds__(ENS_THREADS)
void ensemble_hessian_kernel(const double* __restrict__ vecs, const double* __restrict__ weights, int n_qubits,
                             int ncas, int nstate, int n_theta, const int32_t* __restrict__ pairs, int n_pairs,
                             const double* __restrict__ c1, const double* __restrict__ c2, long c_stride,
                             double* __restrict__ H)
{
    extern __shared__ double ens_lds[];
    __shared__ double red[ENS_THREADS];
    const uint32_t D = 1u << n_qubits;
    const int na2 = ncas * ncas, na4 = na2 * na2;
    const int nvec = 1 + n_theta + n_pairs;
    const int pr = (int)(blockIdx.x % (unsigned)n_pairs);
    const size_t b = blockIdx.x / (unsigned)n_pairs;
    const int j = pairs[2 * pr], k = pairs[2 * pr + 1];
    if (j < 0 || j >= n_theta || k < 0 || k >= n_theta) return;       // (uniform: no element of H belongs to the pair)
    const double* row = vecs + b * nstate * nvec * D;
    const double* cc1 = c1 + b * c_stride;
    const double* cc2 = c2 + b * c_stride;
    const size_t SD = (size_t)nstate * D;
    double* P0 = ens_lds;            // [nstate][D] psi_I
    double* Pj = P0 + SD;            //             tau_I,j
    double* Pk = Pj + SD;            //             tau_I,k
    double* P2 = Pk + SD;            //             psi_I,jk
    for (uint32_t i = threadIdx.x; i < (uint32_t)SD; i += ENS_THREADS) {
        const uint32_t I = i >> n_qubits, x = i & (D - 1);
        const double* vs = row + (size_t)I * nvec * D;
        P0[i] = vs[x];
        Pj[i] = vs[(size_t)(1 + j) * D + x];
        Pk[i] = vs[(size_t)(1 + k) * D + x];
        P2[i] = vs[(size_t)(1 + n_theta + pr) * D + x];
    }
    __syncthreads();
    double acc = 0.0;
    for (int e = (int)threadIdx.x; e < na2 + na4; e += ENS_THREADS) {
        double coef;
        if (e < na2) {
            const int p = e / ncas, s = e - p * ncas;
            double d = 0.0;
            for (int q = 0; q < ncas; ++q) d += cc2[((p * ncas + q) * ncas + q) * ncas + s];
            coef = cc1[e] - d;
        } else {
            coef = cc2[e - na2];
        }
        double val = 0.0;
        for (int I = 0; I < nstate; ++I) {
            const double w = weights[I];
            if (w == 0.0) continue;
            const double* p0 = P0 + (size_t)I * D;
            const double* pj = Pj + (size_t)I * D;
            const double* pk = Pk + (size_t)I * D;
            const double* p2 = P2 + (size_t)I * D;
            double s = ens_element(p2, p0, D, n_qubits, ncas, e);
            s += ens_element(pj, pk, D, n_qubits, ncas, e);
            s += ens_element(pk, pj, D, n_qubits, ncas, e);
            s += ens_element(p0, p2, D, n_qubits, ncas, e);
            val += w * s;
        }
        acc += coef * val;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = ENS_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double* Hb = H + b * n_theta * n_theta;
        Hb[(size_t)j * n_theta + k] = red[0];
        Hb[(size_t)k * n_theta + j] = red[0];
    }
}

}  // namespace

// the scope shared by the four entry points; refuses before anything is launched
static int ensemble_scope(const char* who, int n_qubits, int nstate, int n_theta, int n_pairs, int batch)
{
    OOVQE_REQUIRE(n_qubits >= 2 && n_qubits <= OOVQE_ENSEMBLE_MAX_QUBITS,
                  "%s: n_qubits = %d (dense register only: 2 .. OOVQE_ENSEMBLE_MAX_QUBITS = %d)", who, n_qubits,
                  OOVQE_ENSEMBLE_MAX_QUBITS);
    OOVQE_REQUIRE(nstate >= 1 && nstate <= OOVQE_ENSEMBLE_MAX_STATES,
                  "%s: nstate = %d (1 .. OOVQE_ENSEMBLE_MAX_STATES = %d)", who, nstate, OOVQE_ENSEMBLE_MAX_STATES);
    OOVQE_REQUIRE(n_theta >= 1 && n_pairs >= 0 && batch >= 1, "%s: n_theta = %d, n_pairs = %d, batch = %d", who,
                  n_theta, n_pairs, batch);
    OOVQE_REQUIRE((int64_t)batch * nstate * (1 + (int64_t)n_theta + n_pairs) <= 0x7fffffffLL,
                  "%s: %lld workgroups (at most 2^31 - 1)", who,
                  (long long)batch * nstate * (1 + (long long)n_theta + n_pairs));
    return 0;
}

extern "C" int64_t oovqe_ensemble_work_size(int n_theta, int n_qubits, int nstate, int n_pairs, int batch)
{
    if (int rc = ensemble_scope("ensemble_work_size", n_qubits, nstate, n_theta, n_pairs, batch)) return rc;
    return (int64_t)batch * nstate * (1 + (int64_t)n_theta + n_pairs) * ((int64_t)1 << n_qubits);
}

extern "C" int oovqe_ensemble_states(const double* theta, int n_theta, const oovqe_gate_t* gates, int n_gates,
                                     int n_qubits, const double* psi0, int nstate, const int32_t* pairs, int n_pairs,
                                     int batch, double* vecs, oovqe_stream_t stream)
{
    if (int rc = ensemble_scope("ensemble_states", n_qubits, nstate, n_theta, n_pairs, batch)) return rc;
    OOVQE_REQUIRE(theta && gates && psi0 && vecs && (pairs || n_pairs == 0), "ensemble_states: null pointer");
    OOVQE_REQUIRE(n_gates >= 1, "ensemble_states: n_gates = %d", n_gates);
    const size_t D = (size_t)1 << n_qubits;
    const unsigned grid = (unsigned)((int64_t)batch * nstate * (1 + n_theta + n_pairs));
    hipLaunchKernelGGL(ensemble_states_kernel, dim3(grid), dim3(ENS_THREADS), 2 * D * sizeof(double),
                       (hipStream_t)stream, theta, n_theta, gates, n_gates, n_qubits, psi0, nstate, pairs, n_pairs, vecs);
    OOVQE_CHECK_LAUNCH("ensemble_states");
    return 0;
}

extern "C" int oovqe_ensemble_rdms(const double* vecs, int nvec, const double* weights, int n_qubits, int ncas,
                                   int nstate, int n_tan, int batch, double* gamma_sa, double* Gamma_sa,
                                   double* gamma_st, double* Gamma_st, oovqe_stream_t stream)
{
    if (int rc = ensemble_scope("ensemble_rdms", n_qubits, nstate, nvec >= 1 ? nvec : 1, 0, batch)) return rc;
    OOVQE_REQUIRE(vecs && weights && gamma_sa && Gamma_sa, "ensemble_rdms: null pointer");
    OOVQE_REQUIRE(!gamma_st == !Gamma_st, "ensemble_rdms: gamma_st and Gamma_st come together");
    OOVQE_REQUIRE(n_qubits == 2 * ncas, "ensemble_rdms: n_qubits = %d, ncas = %d", n_qubits, ncas);
    OOVQE_REQUIRE(nvec >= 1 && n_tan >= 0 && n_tan < nvec, "ensemble_rdms: %d derivative sets of %d vectors a state",
                  n_tan, nvec);
    const size_t D = (size_t)1 << n_qubits;
    const int na2 = ncas * ncas;
    const int per = 1 + n_tan + (gamma_st ? nstate * nstate : 0);
    OOVQE_REQUIRE((int64_t)batch * per <= 0x7fffffffLL, "ensemble_rdms: %lld workgroups (at most 2^31 - 1)",
                  (long long)batch * per);
    const size_t lds = (2 * (size_t)nstate * D + na2) * sizeof(double);
    OOVQE_REQUIRE(lds <= ENS_LDS_LIMIT, "ensemble_rdms: %zu bytes of LDS (limit %zu)", lds, ENS_LDS_LIMIT);
    if (lds > 64 * 1024)
        if (int rc = oovqe_ensure_dynamic_lds((const void*)ensemble_rdms_kernel, ENS_LDS_LIMIT)) return rc;
    hipLaunchKernelGGL(ensemble_rdms_kernel, dim3((unsigned)((int64_t)batch * per)), dim3(ENS_THREADS), lds,
                       (hipStream_t)stream, vecs, nvec, weights, n_qubits, ncas, nstate, 1 + n_tan, gamma_st ? 1 : 0,
                       gamma_sa, Gamma_sa, gamma_st, Gamma_st);
    OOVQE_CHECK_LAUNCH("ensemble_rdms");
    return 0;
}

extern "C" int oovqe_ensemble_circuit_hessian_batch(const double* vecs, const double* weights, int n_qubits, int ncas,
                                                    int nstate, int n_theta, const int32_t* pairs, int n_pairs,
                                                    int batch, const double* c1, const double* c2, int64_t c_stride,
                                                    double* H, oovqe_stream_t stream)
{
    if (int rc = ensemble_scope("ensemble_circuit_hessian", n_qubits, nstate, n_theta, n_pairs, batch)) return rc;
    OOVQE_REQUIRE(vecs && weights && pairs && c1 && c2 && H, "ensemble_circuit_hessian: null pointer");
    OOVQE_REQUIRE(n_qubits == 2 * ncas, "ensemble_circuit_hessian: n_qubits = %d, ncas = %d", n_qubits, ncas);
    OOVQE_REQUIRE(n_pairs >= 1 && (batch == 1 || c_stride > 0), "ensemble_circuit_hessian: n_pairs = %d, stride %ld",
                  n_pairs, (long)c_stride);
    const size_t D = (size_t)1 << n_qubits;
    const size_t lds = 4 * (size_t)nstate * D * sizeof(double);
    OOVQE_REQUIRE(lds <= ENS_LDS_LIMIT, "ensemble_circuit_hessian: %zu bytes of LDS (limit %zu)", lds, ENS_LDS_LIMIT);
    if (lds > 64 * 1024)
        if (int rc = oovqe_ensure_dynamic_lds((const void*)ensemble_hessian_kernel, ENS_LDS_LIMIT)) return rc;
    hipLaunchKernelGGL(ensemble_hessian_kernel, dim3((unsigned)((int64_t)batch * n_pairs)), dim3(ENS_THREADS), lds,
                       (hipStream_t)stream, vecs, weights, n_qubits, ncas, nstate, n_theta, pairs, n_pairs, c1, c2,
                       (long)c_stride, H);
    OOVQE_CHECK_LAUNCH("ensemble_circuit_hessian");
    return 0;
}
