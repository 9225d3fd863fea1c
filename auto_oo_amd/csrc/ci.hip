// Batched determinant-space CI: block Davidson-Liu for the lowest roots of the active-space Hamiltonian
//   H = c0 + sum_pq c1_pq E_pq + sum_pqrs c2_pqrs (E_pq E_rs - delta_qr E_ps)       (c2 = g / 2)
// in the (N_alpha = N_beta) sector, one workgroup per problem, every iteration inside ONE launch.
//
// Basis.  The kernel works in the determinant basis |ia, ib> = A(ia)^+ B(ib)^+ |0> (all alpha creators, then
// all beta creators) where an excitation E^alpha_pq acts on the alpha string only and E^beta_pq on the beta
// string only, each with the parity of its own electrons strictly between p and q (sector.hip, the comment
// over sector_gmat_kernel).  The sector layout of the circuit engine (spin orbitals interleaved, 2p = alpha_p)
// differs from it by the sign sigma(ia, ib) of sorting one operator order into the other; the CI vectors
// leave the kernel in the sector layout c = ia * nb + ib with that sign applied.  The strings are those of
// sector.string_tables: ascending by value, orbital p at bit ncas - 1 - p.
//
// Sigma.  With C the na x nb matrix of the vector and Ga the na x na matrix of the one-spin part
//   Ga = sum_pq c1'_pq A_pq + sum_pqrs c2_pqrs A_pq A_rs,     c1'_pq = c1_pq - sum_r c2_prrq
// (the same matrix for beta, the strings being the same), the sigma vector is
//   (H - c0) C = Ga C + C Ga^T + sum_{pq,rs} M[pq][rs] A_pq C B_rs^T,    M[pq][rs] = 2 c2_pqrs (- lambda S^2 part)
// The mixed term is formed one target alpha string ia at a time: the rows C[src_pq(ia)] of the nv excitations
// pq that reach ia are gathered into X [nv, nb] (LDS), Y = M^T X [a^2, nb] is a small dense product, and
// sigma(ia, ib) = sum_rs sign * Y[rs][src_rs(ib)] gathers Y with the beta excitations.
//
// Spin.  S^2 = S_- S_+ at Ms = 0, S_- S_+ = N_beta - sum_pq A_qp B_pq: with a spin shift lambda > 0 the sigma is
// that of H + lambda S^2, whose lowest roots are the lowest of { E + lambda S (S + 1) }, and the energy reported is
// <H> = theta - lambda <S^2>, <S^2> from the same sigma routine with the S^2 coefficients.  A state of spin S is
// lifted by lambda S (S + 1) and no further: whether the roots ARE singlets is for the caller to read off <S^2> and,
// where they are not, to solve again with a larger shift (ci.casci_packed does).  The residual norms reported are
// those of H + lambda S^2 at theta.
//
// Guess.  Unit vectors on the 2 nroots + 2 lowest diagonal elements, and one more vector with a nonzero component on
// every other determinant (a fixed hash of its index).  |ia, ib> and |ib, ia> have the same diagonal element, so the
// unit vectors span whole classes of the alpha/beta-swap symmetry (and of any point group that maps determinants
// onto determinants); corrections never leave the classes of the Ritz vectors they come from, and without the hash
// vector an eigenvector of a class the unit vectors miss is never reached while every residual goes below tol.
//
// Coefficients are symmetrised on load over the symmetries every real state's RDMs have (gamma_pq = gamma_qp,
// Gamma_pqrs = Gamma_rspq = Gamma_qpsr = Gamma_srqp), so c0 + c1.gamma + c2.Gamma is unchanged and H is symmetric.
#include "common.h"

namespace {

constexpr int CI_NT = 256;                // threads per workgroup
constexpr int CI_NW = CI_NT / 64;
constexpr int CI_MAXA = 8;
constexpr int CI_MAXSTR = 70;             // C(8, 4)
constexpr int CI_MAXDC = CI_MAXSTR * CI_MAXSTR;
constexpr int CI_MAXSUB = 24;             // Davidson subspace
constexpr int CI_MAXR = 4;                // roots
constexpr int CI_MAXKEEP = 2 * CI_MAXR + 2;   // Ritz vectors kept when the subspace is collapsed
constexpr int CI_MAXREJECT = 3;           // refusals of a solve on the residual of H before it gives up
constexpr int CI_YREG = (CI_MAXA * CI_MAXA * CI_MAXSTR + CI_NT - 1) / CI_NT;
constexpr double CI_SPIN_SHIFT = 1.0;        // the shift of oovqe_ci_davidson_batch (fix_singlet != 0)

__host__ __device__ inline int ci_binom(int n, int k)
{
    if (k < 0 || k > n) return 0;
    long r = 1;
    for (int i = 1; i <= k; ++i) r = r * (n - k + i) / i;
    return (int)r;
}

__host__ __device__ inline int ci_maxsub(int Dc) { return Dc < CI_MAXSUB ? Dc : CI_MAXSUB; }
__host__ __device__ inline int ci_nguess(int Dc, int nroots)
{
    int g = 2 * nroots + 2;
    const int ms = ci_maxsub(Dc);
    return g < ms ? g : ms;
}

// per-problem global scratch (doubles): V [ms][Dc] | W [ms][Dc] | T [nroots][Dc] | Hd [Dc] | Ga [na][na] | Sx [Dc]
inline size_t ci_work_per_problem(int na, int nroots)
{
    const int Dc = na * na;
    return (size_t)(2 * ci_maxsub(Dc) + nroots + 3) * Dc;
}

struct CiLds {
    double *Cv, *M, *XY, *Hs, *U, *theta, *dots, *red, *part, *c1p, *scal;
    int *pql, *ints, *rank, *chosen;
    uint32_t* unrank;
    uint16_t* tab;
};

// X / Y buffer: max(a^2, na) rows of nb (also Ga while it is built, and the Rayleigh-Ritz matrix's copy)
__host__ __device__ inline int ci_xy_doubles(int a, int na)
{
    const int xr = a * a > na ? a * a : na;
    return xr * na > CI_MAXSUB * CI_MAXSUB ? xr * na : CI_MAXSUB * CI_MAXSUB;
}

__host__ __device__ inline size_t ci_lds_doubles(int a, int na)
{
    const int a2 = a * a, Dc = na * na;
    return (size_t)Dc + (size_t)a2 * a2 + ci_xy_doubles(a, na) + 2 * CI_MAXSUB * CI_MAXSUB + 2 * CI_MAXSUB
           + CI_NW * CI_MAXSUB + CI_NT + a2 + 8;
}

inline size_t ci_lds_bytes(int a, int na)
{
    const size_t ints = (size_t)a * a + 8 + (1u << a) + 16 + na;           // pql, ints, rank, chosen, unrank
    const size_t tab = ((size_t)a * a * na * 2 + 7) / 8;
    return (ci_lds_doubles(a, na) + (ints + 1) / 2 + tab) * sizeof(double);
}

__device__ inline CiLds ci_carve(double* lds, int a, int na)
{
    const int a2 = a * a, Dc = na * na;
    CiLds L;
    double* p = lds;
    L.Cv = p; p += Dc;
    L.M = p; p += a2 * a2;
    L.XY = p; p += ci_xy_doubles(a, na);
    L.Hs = p; p += CI_MAXSUB * CI_MAXSUB;
    L.U = p; p += CI_MAXSUB * CI_MAXSUB;
    L.theta = p; p += CI_MAXSUB;
    L.dots = p; p += CI_MAXSUB;
    L.red = p; p += CI_NW * CI_MAXSUB;
    L.part = p; p += CI_NT;
    L.c1p = p; p += a2;
    L.scal = p; p += 8;
    int* q = reinterpret_cast<int*>(p);
    L.pql = q; q += a2;
    L.ints = q; q += 8;
    L.rank = q; q += 1 << a;
    L.chosen = q; q += 16;
    L.unrank = reinterpret_cast<uint32_t*>(q); q += na;
    const size_t ints = (size_t)a2 + 8 + (1u << a) + 16 + na;
    L.tab = reinterpret_cast<uint16_t*>(p + (ints + 1) / 2);
    return L;
}

__device__ __forceinline__ double ci_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ uint32_t ci_orb_mask(int a, int r1, int r2)     // orbitals r1 .. r2 of a string
{
    return r2 < r1 ? 0u : (((1u << (r2 - r1 + 1)) - 1u) << (a - 1 - r2));
}

// out[j] = x . V_j for j < m (x, V_j in global memory, V_j = V + j * ld); out in LDS, valid after the call
__device__ void ci_dots(const double* __restrict__ x, const double* __restrict__ V, size_t ld, int m, int Dc,
                        double* out, double* red)
{
    double acc[CI_MAXSUB];
#pragma unroll
    for (int j = 0; j < CI_MAXSUB; ++j) acc[j] = 0.0;
    for (int I = threadIdx.x; I < Dc; I += CI_NT) {
        const double xv = x[I];
#pragma unroll
        for (int j = 0; j < CI_MAXSUB; ++j)
            if (j < m) acc[j] += xv * V[j * ld + I];
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < CI_MAXSUB; ++j) {
        if (j < m) {
            const double s = ci_wave_sum(acc[j]);
            if (lane == 0) red[w * CI_MAXSUB + j] = s;
        }
    }
    __syncthreads();
    if (threadIdx.x < m) {
        double s = 0.0;
        for (int k = 0; k < CI_NW; ++k) s += red[k * CI_MAXSUB + threadIdx.x];
        out[threadIdx.x] = s;
    }
    __syncthreads();
}

// component I of the last guess vector: a fixed hash of the index in (-1/2, 1/2), never zero
__device__ __forceinline__ double ci_guess_hash(int I)
{
    uint32_t h = (uint32_t)I * 2654435761u + 0x9e3779b9u;
    h ^= h >> 15;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    return ((double)((h >> 8) & 0xffffu) + 0.5) / 65536.0 - 0.5;
}

// the lowest value of v (global) whose index is not in excl[0 .. nex); (value, index) order, ties by index
__device__ int ci_argmin(const double* __restrict__ v, int Dc, const int* excl, int nex, double* red, int* ints)
{
    double best = 1.0e308;
    int bi = 0x7fffffff;
    for (int I = threadIdx.x; I < Dc; I += CI_NT) {
        bool skip = false;
        for (int e = 0; e < nex; ++e) skip |= excl[e] == I;
        const double x = v[I];
        if (!skip && (x < best || (x == best && I < bi))) { best = x; bi = I; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { red[w] = best; ints[w] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double b = red[0];
        int i = ints[0];
        for (int k = 1; k < CI_NW; ++k)
            if (red[k] < b || (red[k] == b && ints[k] < i)) { b = red[k]; i = ints[k]; }
        ints[4] = i;
    }
    __syncthreads();
    const int r = ints[4];
    __syncthreads();
    return r;
}

// out = shift * C + [Ga C + C Ga^T] + sum M[pq][rs] A_pq C B_rs^T for the vector C in L.Cv (LDS); out global.
// Ga (global, na x na) is skipped when null.
__device__ void ci_sigma(const CiLds& L, int a, int na, const double* __restrict__ Ga, double shift,
                         double* __restrict__ out)
{
    const int a2 = a * a, nb = na, tid = threadIdx.x;
    const int ngrp = CI_NT / nb, g = tid / nb, ibt = tid - g * nb;
    for (int ia = 0; ia < na; ++ia) {
        // 1. the excitations pq that reach string ia (a^2 <= 64: one wave)
        if (tid < 64) {
            const bool v = tid < a2 && ((L.tab[tid * na + ia] >> 11) & 1u);
            const unsigned long long mk = __ballot(v);
            if (v) L.pql[__popcll(mk & ((1ull << tid) - 1ull))] = tid;
            if (tid == 0) L.ints[0] = __popcll(mk);
        }
        __syncthreads();
        const int nv = L.ints[0];
        // 2. X[k][ib] = sign * C[src_pq(ia)][ib]
        for (int o = tid; o < nv * nb; o += CI_NT) {
            const int k = o / nb, ib = o - k * nb;
            const uint16_t w = L.tab[L.pql[k] * na + ia];
            const double x = L.Cv[(w & 2047u) * nb + ib];
            L.XY[o] = ((w >> 12) & 1u) ? -x : x;
        }
        __syncthreads();
        // 3. Y[rs][ib] = sum_k M[pq_k][rs] X[k][ib] (registers, then over X)
        double yr[CI_YREG];
#pragma unroll
        for (int j = 0; j < CI_YREG; ++j) {
            const int o = tid + j * CI_NT;
            yr[j] = 0.0;
            if (o < a2 * nb) {
                const int rs = o / nb, ib = o - rs * nb;
                double acc = 0.0;
                for (int k = 0; k < nv; ++k) acc += L.M[L.pql[k] * a2 + rs] * L.XY[k * nb + ib];
                yr[j] = acc;
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < CI_YREG; ++j) {
            const int o = tid + j * CI_NT;
            if (o < a2 * nb) L.XY[o] = yr[j];
        }
        __syncthreads();
        // 4. beta gather of Y and the one-spin terms, split over ngrp groups of nb threads (fixed order)
        if (g < ngrp) {
            double acc = 0.0;
            for (int rs = g; rs < a2; rs += ngrp) {
                const uint16_t w = L.tab[rs * na + ibt];
                if ((w >> 11) & 1u) {
                    const double y = L.XY[rs * nb + (w & 2047u)];
                    acc += ((w >> 12) & 1u) ? -y : y;
                }
            }
            if (Ga) {
                for (int j = g; j < na; j += ngrp) acc += Ga[ia * na + j] * L.Cv[j * nb + ibt];
                for (int j = g; j < nb; j += ngrp) acc += Ga[ibt * na + j] * L.Cv[ia * nb + j];
            }
            L.part[tid] = acc;
        }
        __syncthreads();
        if (tid < nb) {
            double s = shift * L.Cv[ia * nb + tid];
            for (int k = 0; k < ngrp; ++k) s += L.part[k * nb + tid];
            out[ia * nb + tid] = s;
        }
        // (the next row writes pql / X only after its first barrier; part after three)
    }
    __syncthreads();
}

// eigen-decomposition of the symmetric m x m matrix Hs (LDS, pitch CI_MAXSUB) by cyclic Jacobi on wave 0:
// theta ascending, U[:, k] the eigenvectors.  Hs is overwritten.
__device__ void ci_jacobi(double* A, double* U, double* theta, int m)
{
    const int lane = threadIdx.x;
    if (threadIdx.x < 64) {
        for (int k = lane; k < m * CI_MAXSUB; k += 64) {
            const int r = k / CI_MAXSUB, c = k - r * CI_MAXSUB;
            U[k] = (r == c) ? 1.0 : 0.0;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        for (int sweep = 0; sweep < 60; ++sweep) {
            double off = 0.0, dg = 0.0;
            if (lane < m) {
                for (int c = 0; c < m; ++c) {
                    const double x = fabs(A[lane * CI_MAXSUB + c]);
                    if (c == lane) dg = fmax(dg, x); else off = fmax(off, x);
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                off = fmax(off, __shfl_xor(off, o, 64));
                dg = fmax(dg, __shfl_xor(dg, o, 64));
            }
            if (off <= 1e-15 * fmax(dg, 1e-300) || off == 0.0) break;
            for (int p = 0; p < m - 1; ++p) {
                for (int q = p + 1; q < m; ++q) {
                    const double apq = A[p * CI_MAXSUB + q];
                    if (fabs(apq) <= 1e-300) continue;
                    const double app = A[p * CI_MAXSUB + p], aqq = A[q * CI_MAXSUB + q];
                    const double tau = (aqq - app) / (2.0 * apq);
                    const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                    const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
                    double akp = 0.0, akq = 0.0, ukp = 0.0, ukq = 0.0;
                    if (lane < m) {
                        akp = A[lane * CI_MAXSUB + p]; akq = A[lane * CI_MAXSUB + q];
                        ukp = U[lane * CI_MAXSUB + p]; ukq = U[lane * CI_MAXSUB + q];
                    }
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                    if (lane < m) {
                        U[lane * CI_MAXSUB + p] = c * ukp - s * ukq;
                        U[lane * CI_MAXSUB + q] = s * ukp + c * ukq;
                        if (lane != p && lane != q) {
                            const double np_ = c * akp - s * akq, nq_ = s * akp + c * akq;
                            A[lane * CI_MAXSUB + p] = np_; A[p * CI_MAXSUB + lane] = np_;
                            A[lane * CI_MAXSUB + q] = nq_; A[q * CI_MAXSUB + lane] = nq_;
                        } else if (lane == p) {
                            A[p * CI_MAXSUB + p] = app - t * apq;
                            A[q * CI_MAXSUB + q] = aqq + t * apq;
                            A[p * CI_MAXSUB + q] = 0.0;
                            A[q * CI_MAXSUB + p] = 0.0;
                        }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                }
            }
        }
        // ascending order (selection by one lane, columns of U moved by all)
        for (int k = 0; k < m; ++k) {
            int best = k;
            double bv = A[k * CI_MAXSUB + k];
            for (int j = k + 1; j < m; ++j)
                if (A[j * CI_MAXSUB + j] < bv) { bv = A[j * CI_MAXSUB + j]; best = j; }
            if (best != k) {
                if (lane < m) {
                    const double t0 = U[lane * CI_MAXSUB + k];
                    U[lane * CI_MAXSUB + k] = U[lane * CI_MAXSUB + best];
                    U[lane * CI_MAXSUB + best] = t0;
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                if (lane == 0) {
                    const double t0 = A[k * CI_MAXSUB + k];
                    A[k * CI_MAXSUB + k] = A[best * CI_MAXSUB + best];
                    A[best * CI_MAXSUB + best] = t0;
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            }
            if (lane == 0) theta[k] = A[k * CI_MAXSUB + k];
        }
    }
    __syncthreads();
}

// M[pq][rs] = 2 c2s_pqrs - lam delta_ps delta_qr (lam = 0 and c2 = null: no two-body part; s2_only: -delta delta)
__device__ void ci_load_m(double* M, const double* __restrict__ c2, int a, double lam, bool s2_only)
{
    const int a2 = a * a, a3 = a2 * a;
    for (int o = threadIdx.x; o < a2 * a2; o += CI_NT) {
        const int p = o / a3, q = (o / a2) % a, r = (o / a) % a, s = o % a;
        double v = 0.0;
        if (!s2_only)
            v = 0.5 * (c2[((p * a + q) * a + r) * a + s] + c2[((r * a + s) * a + p) * a + q]
                       + c2[((q * a + p) * a + s) * a + r] + c2[((s * a + r) * a + q) * a + p]);
        if (p == s && q == r) v -= lam;
        M[o] = v;
    }
}

__global__ __launch_bounds__(CI_NT)
void ci_davidson_kernel(int a, int n, int nroots, const double* __restrict__ c0g, const double* __restrict__ c1g,
                        const double* __restrict__ c2g, long c_stride, double lam, double tol, int max_iter,
                        double* __restrict__ energies, double* __restrict__ ci, double* __restrict__ s2out,
                        double* __restrict__ rnorm, int* __restrict__ info, double* __restrict__ work,
                        size_t per_problem)
{
    extern __shared__ double lds[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int na = ci_binom(a, n), nb = na, Dc = na * nb, a2 = a * a;
    CiLds L = ci_carve(lds, a, na);
    const int ms = ci_maxsub(Dc);
    double* V = work + (size_t)b * per_problem;
    double* W = V + (size_t)ms * Dc;
    double* T = W + (size_t)ms * Dc;
    double* Hd = T + (size_t)nroots * Dc;
    double* Ga = Hd + Dc;
    double* Sx = Ga + Dc;                           // S^2 x_k of one Ritz vector
    const double* c1 = c1g + (size_t)b * c_stride;
    const double* c2 = c2g + (size_t)b * c_stride;

    // ---- strings, excitation table, coefficients ------------------------------------------------------------
    if (tid == 0) {
        int k = 0;
        for (int mk = 0; mk < (1 << a); ++mk) {
            if (__popc(mk) == n) { L.unrank[k] = (uint32_t)mk; L.rank[mk] = k++; }
            else L.rank[mk] = -1;
        }
    }
    ci_load_m(L.M, c2, a, lam, false);
    __syncthreads();
    for (int idx = tid; idx < na * a2; idx += CI_NT) {
        const int pq = idx / na, is = idx - pq * na, p = pq / a, q = pq - p * a;
        const uint32_t st = L.unrank[is];
        const uint32_t bp = 1u << (a - 1 - p), bq = 1u << (a - 1 - q);
        const int lo = p < q ? p : q, hi = p < q ? q : p;
        uint32_t valid, src;
        if (p == q) { valid = (st & bp) ? 1u : 0u; src = (uint32_t)is; }
        else {
            valid = ((st & bp) && !(st & bq)) ? 1u : 0u;
            src = valid ? (uint32_t)L.rank[(st & ~bp) | bq] : 0u;
        }
        const uint32_t own = __popc(st & ci_orb_mask(a, lo + 1, hi - 1)) & 1u;
        L.tab[pq * na + is] = (uint16_t)(src | (valid << 11) | (own << 12));
    }
    // c1'_pq = c1s_pq - sum_r c2s_prrq   (c2s = (M + lam delta delta) / 2)
    for (int pq = tid; pq < a2; pq += CI_NT) {
        const int p = pq / a, q = pq - p * a;
        double v = 0.5 * (c1[p * a + q] + c1[q * a + p]);
        for (int r = 0; r < a; ++r) {
            const int o = (p * a + r) * a2 + r * a + q;
            v -= 0.5 * (L.M[o] + ((p == q) ? lam : 0.0));
        }
        L.c1p[pq] = v;
    }
    __syncthreads();
    // Ga, one row per thread, accumulated in LDS (the X buffer), then copied to global
    for (int o = tid; o < na * na; o += CI_NT) L.XY[o] = 0.0;
    __syncthreads();
    if (tid < na) {
        double* Gi = L.XY + tid * na;
        for (int pq = 0; pq < a2; ++pq) {
            const uint16_t w = L.tab[pq * na + tid];
            if (!((w >> 11) & 1u)) continue;
            const int k = w & 2047u;
            const double s1 = ((w >> 12) & 1u) ? -1.0 : 1.0;
            Gi[k] += s1 * L.c1p[pq];
            const int p = pq / a, q = pq - p * a;
            for (int rs = 0; rs < a2; ++rs) {
                const uint16_t w2 = L.tab[rs * na + k];
                if (!((w2 >> 11) & 1u)) continue;
                const int r = rs / a, s = rs - r * a;
                const double c2s = 0.5 * (L.M[pq * a2 + rs] + ((p == s && q == r) ? lam : 0.0));
                Gi[w2 & 2047u] += (((w2 >> 12) & 1u) ? -s1 : s1) * c2s;
            }
        }
    }
    __syncthreads();
    for (int o = tid; o < na * na; o += CI_NT) Ga[o] = L.XY[o];
    // diagonal (the preconditioner and the guess)
    const double shift = lam * n;
    for (int I = tid; I < Dc; I += CI_NT) {
        const int ia = I / nb, ib = I - ia * nb;
        const uint32_t sa = L.unrank[ia], sb = L.unrank[ib];
        double d = L.XY[ia * na + ia] + L.XY[ib * na + ib] + shift;
        for (int p = 0; p < a; ++p) {
            if (!(sa & (1u << (a - 1 - p)))) continue;
            for (int r = 0; r < a; ++r)
                if (sb & (1u << (a - 1 - r))) d += L.M[(p * a + p) * a2 + r * a + r];
        }
        Hd[I] = d;
        // the guess is chosen on the diagonal of H alone (T is free until the first residual): the S^2 penalty
        // would rank every open-shell determinant lambda higher and can leave whole symmetries out of the guess
        int closed = 0;
        for (int p = 0; p < a; ++p) closed += ((sa & sb) >> (a - 1 - p)) & 1u;
        T[I] = d - lam * (n - closed);
    }
    __syncthreads();

    // ---- guess: unit vectors on the lowest diagonal elements, and the hash vector orthogonal to them -----------
    const int ng = ci_nguess(Dc, nroots);
    for (int k = 0; k < ng; ++k) {
        const int I = ci_argmin(T, Dc, L.chosen, k, L.red, L.ints);
        if (tid == 0) L.chosen[k] = I;
        for (int J = tid; J < Dc; J += CI_NT) V[(size_t)k * Dc + J] = (J == I) ? 1.0 : 0.0;
        __syncthreads();
    }
    int m = ng;
    if (ng < ms) {                                   // (so Dc > ng: some determinant is not a unit guess)
        double* t = V + (size_t)ng * Dc;
        for (int J = tid; J < Dc; J += CI_NT) {
            bool unit = false;
            for (int k = 0; k < ng; ++k) unit |= L.chosen[k] == J;
            t[J] = unit ? 0.0 : ci_guess_hash(J);
        }
        __syncthreads();
        ci_dots(t, t, 0, 1, Dc, L.dots, L.red);
        const double inv = 1.0 / sqrt(L.dots[0]);
        for (int J = tid; J < Dc; J += CI_NT) t[J] *= inv;
        __syncthreads();
        m = ng + 1;
    }

    // ---- Davidson iterations ------------------------------------------------------------------------------------
    int mold = 0, iters = 0, conv_all = 0, nreject = 0;
    bool have_s2 = false;                // L.scal holds <S^2> of the current Ritz vectors
    double* rn = L.scal + CI_MAXR;       // residual norms
    if (tid < CI_MAXR) rn[tid] = 0.0;
    __syncthreads();
    for (int it = 0; it < max_iter; ++it) {
        iters = it + 1;
        have_s2 = false;
        for (int i = mold; i < m; ++i) {
            for (int J = tid; J < Dc; J += CI_NT) L.Cv[J] = V[(size_t)i * Dc + J];
            __syncthreads();
            ci_sigma(L, a, na, Ga, shift, W + (size_t)i * Dc);
        }
        for (int i = mold; i < m; ++i) {
            ci_dots(W + (size_t)i * Dc, V, Dc, i + 1, Dc, L.dots, L.red);
            if (tid <= i) { L.Hs[i * CI_MAXSUB + tid] = L.dots[tid]; L.Hs[tid * CI_MAXSUB + i] = L.dots[tid]; }
            __syncthreads();
        }
        // Rayleigh-Ritz on a copy of Hs (the Jacobi routine overwrites its input; XY is free here)
        double* A = L.XY;
        for (int o = tid; o < CI_MAXSUB * CI_MAXSUB; o += CI_NT) A[o] = L.Hs[o];
        __syncthreads();
        ci_jacobi(A, L.U, L.theta, m);
        // residuals r_k = sum_j U_jk (W_j - theta_k V_j) -> T_k
        const int nr = nroots;
        for (int I = tid; I < Dc; I += CI_NT) {
            double r[CI_MAXR];
#pragma unroll
            for (int k = 0; k < CI_MAXR; ++k) r[k] = 0.0;
            for (int j = 0; j < m; ++j) {
                const double w = W[(size_t)j * Dc + I], v = V[(size_t)j * Dc + I];
#pragma unroll
                for (int k = 0; k < CI_MAXR; ++k)
                    if (k < nr) r[k] += L.U[j * CI_MAXSUB + k] * (w - L.theta[k] * v);
            }
#pragma unroll
            for (int k = 0; k < CI_MAXR; ++k)
                if (k < nr) T[(size_t)k * Dc + I] = r[k];
        }
        __syncthreads();
        int nunc = 0;
#pragma unroll
        for (int k = 0; k < CI_MAXR; ++k) {
            if (k < nr) {
                ci_dots(T + (size_t)k * Dc, T + (size_t)k * Dc, 0, 1, Dc, L.dots, L.red);
                const double r = sqrt(fmax(L.dots[0], 0.0));
                if (tid == 0) rn[k] = r;
                nunc += (r < tol) ? 0 : 1;              // (NaN counts as not converged)
            }
        }
        __syncthreads();
        // With a spin shift the residuals above are those of H + lam S^2.  A component of spin S along an eigenvector
        // of H at E enters them with E + lam S (S + 1) - theta, and the residual of H with E - <H>, which is the larger
        // one for a state of higher spin below the root.  So a solve is accepted only when the residuals of H,
        // r_k - lam (S^2 x_k - <S^2> x_k), are below tol as well; the norms reported are the larger of the two.
        // Iterating on drives both down together, unless a lifted state lies at a root: the Ritz vector then mixes
        // the two spins whatever the residual of H + lam S^2.  After CI_MAXREJECT refusals the solve stops as not
        // converged (info < max_iter) and the caller's remedy is another shift.
        if (nunc == 0 && lam > 0.0) {
            ci_load_m(L.M, nullptr, a, 1.0, true);
            __syncthreads();
#pragma unroll
            for (int k = 0; k < CI_MAXR; ++k) {
                if (k < nr) {
                    for (int J = tid; J < Dc; J += CI_NT) {
                        double x = 0.0;
                        for (int j = 0; j < m; ++j) x += L.U[j * CI_MAXSUB + k] * V[(size_t)j * Dc + J];
                        L.Cv[J] = x;
                    }
                    __syncthreads();
                    ci_sigma(L, a, na, nullptr, (double)n, Sx);
                    ci_dots(Sx, L.Cv, 0, 1, Dc, L.dots, L.red);
                    const double s2 = L.dots[0];
                    for (int J = tid; J < Dc; J += CI_NT)
                        Sx[J] = T[(size_t)k * Dc + J] - lam * (Sx[J] - s2 * L.Cv[J]);
                    __syncthreads();
                    ci_dots(Sx, Sx, 0, 1, Dc, L.dots, L.red);
                    if (tid == 0) L.scal[k] = s2;          // (read in the output stage, many barriers on)
                    const double r = fmax(rn[k], sqrt(fmax(L.dots[0], 0.0)));
                    nunc += (r < tol) ? 0 : 1;
                    __syncthreads();                       // (every thread has read rn[k])
                    if (tid == 0) rn[k] = r;
                }
            }
            have_s2 = true;
            __syncthreads();
        }
        if (nunc == 0) { conv_all = 1; break; }
        if (it == max_iter - 1) break;
        if (have_s2 && ++nreject >= CI_MAXREJECT) break;
        if (have_s2) {                                 // (M held the S^2 coefficients for the check)
            ci_load_m(L.M, c2, a, lam, false);
            __syncthreads();
        }
        // collapse when the new directions do not fit: onto the lowest 2 nroots + 2 Ritz vectors (those above the
        // roots carry what the subspace has learnt about the next eigenvalues, which sets the rate of the last root)
        if (m + nunc > ms) {
            int nk = 2 * nr + 2;
            if (nk > ms - nunc) nk = ms - nunc;
            if (nk < nr) nk = nr;
            for (int pass = 0; pass < 2; ++pass) {      // V, then W (each element is read before it is written)
                double* Z = pass ? W : V;
                for (int I = tid; I < Dc; I += CI_NT) {
                    double x[CI_MAXKEEP];
#pragma unroll
                    for (int k = 0; k < CI_MAXKEEP; ++k) x[k] = 0.0;
                    for (int j = 0; j < m; ++j) {
                        const double z = Z[(size_t)j * Dc + I];
#pragma unroll
                        for (int k = 0; k < CI_MAXKEEP; ++k)
                            if (k < nk) x[k] += L.U[j * CI_MAXSUB + k] * z;
                    }
#pragma unroll
                    for (int k = 0; k < CI_MAXKEEP; ++k)
                        if (k < nk) Z[(size_t)k * Dc + I] = x[k];
                }
            }
            __syncthreads();                           // (every thread has read U before it is reset)
            for (int o = tid; o < CI_MAXSUB * CI_MAXSUB; o += CI_NT) {
                const int r = o / CI_MAXSUB, c = o - r * CI_MAXSUB;
                L.Hs[o] = (r == c && r < nk) ? L.theta[r] : 0.0;
                L.U[o] = (r == c) ? 1.0 : 0.0;         // (the Ritz vectors are now V_0 .. V_nk-1)
            }
            m = nk;
            __syncthreads();
        }
        // corrections t_k = r_k / (theta_k - Hd), orthonormalised against V (twice), appended
        mold = m;
#pragma unroll
        for (int k = 0; k < CI_MAXR; ++k) {
            if (k >= nr || m >= ms || rn[k] < tol) continue;
            double* t = V + (size_t)m * Dc;
            const double th = L.theta[k];
            for (int I = tid; I < Dc; I += CI_NT) {
                double d = th - Hd[I];
                if (fabs(d) < 1e-4) d = d < 0.0 ? -1e-4 : 1e-4;
                t[I] = T[(size_t)k * Dc + I] / d;
            }
            __syncthreads();
            ci_dots(t, t, 0, 1, Dc, L.dots, L.red);
            const double n0 = sqrt(L.dots[0]);
            for (int pass = 0; pass < 2; ++pass) {
                ci_dots(t, V, Dc, m, Dc, L.dots, L.red);
                for (int I = tid; I < Dc; I += CI_NT) {
                    double x = t[I];
                    for (int j = 0; j < m; ++j) x -= L.dots[j] * V[(size_t)j * Dc + I];
                    t[I] = x;
                }
                __syncthreads();
            }
            ci_dots(t, t, 0, 1, Dc, L.dots, L.red);
            const double n1 = sqrt(L.dots[0]);
            if (!(n1 > 1e-8 * n0) || !(n1 > 1e-300)) continue;          // (linearly dependent: dropped)
            const double inv = 1.0 / n1;
            for (int I = tid; I < Dc; I += CI_NT) t[I] *= inv;
            __syncthreads();
            ++m;
        }
        if (m == mold) break;                                           // no new direction: stagnated
    }

    // ---- Ritz vectors, <S^2>, <H>, sector sign, output ---------------------------------------------------------
    for (int I = tid; I < Dc; I += CI_NT) {
        double x[CI_MAXR];
#pragma unroll
        for (int k = 0; k < CI_MAXR; ++k) x[k] = 0.0;
        for (int j = 0; j < m; ++j) {
            const double v = V[(size_t)j * Dc + I];
#pragma unroll
            for (int k = 0; k < CI_MAXR; ++k)
                if (k < nroots) x[k] += L.U[j * CI_MAXSUB + k] * v;
        }
#pragma unroll
        for (int k = 0; k < CI_MAXR; ++k)
            if (k < nroots) T[(size_t)k * Dc + I] = x[k];
    }
    if (!have_s2) ci_load_m(L.M, nullptr, a, 1.0, true);
    __syncthreads();
    for (int k = 0; k < nroots; ++k) {
        double s2 = have_s2 ? L.scal[k] : 0.0;
        if (!have_s2) {
            for (int J = tid; J < Dc; J += CI_NT) L.Cv[J] = T[(size_t)k * Dc + J];
            __syncthreads();
            ci_sigma(L, a, na, nullptr, (double)n, Sx);
            ci_dots(Sx, T + (size_t)k * Dc, 0, 1, Dc, L.dots, L.red);
            s2 = L.dots[0];
        }
        // sign: the largest |component| (first on ties) positive, in the sector layout
        double best = -1.0;
        int bi = 0x7fffffff;
        for (int I = tid; I < Dc; I += CI_NT) {
            const int ia = I / nb, ib = I - ia * nb;
            const uint32_t sa = L.unrank[ia], sb = L.unrank[ib];
            uint32_t par = 0;
            for (int i = 1; i < a; ++i)
                if (sa & (1u << (a - 1 - i))) par ^= __popc(sb & ci_orb_mask(a, 0, i - 1)) & 1u;
            const double x = par ? -T[(size_t)k * Dc + I] : T[(size_t)k * Dc + I];
            T[(size_t)k * Dc + I] = x;
            const double ax = fabs(x);
            if (ax > best || (ax == best && I < bi)) { best = ax; bi = I; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        if ((tid & 63) == 0) { L.part[tid >> 6] = best; L.ints[tid >> 6] = bi; }
        __syncthreads();
        if (tid == 0) {
            double bb = L.part[0];
            int ii = L.ints[0];
            for (int w = 1; w < CI_NW; ++w)
                if (L.part[w] > bb || (L.part[w] == bb && L.ints[w] < ii)) { bb = L.part[w]; ii = L.ints[w]; }
            L.ints[4] = ii;
        }
        __syncthreads();
        const double sg = T[(size_t)k * Dc + L.ints[4]] < 0.0 ? -1.0 : 1.0;
        double* out = ci + ((size_t)b * nroots + k) * Dc;
        for (int I = tid; I < Dc; I += CI_NT) out[I] = sg * T[(size_t)k * Dc + I];
        if (tid == 0) {
            energies[b * nroots + k] = c0g[(size_t)b * c_stride] + L.theta[k] - lam * s2;
            s2out[b * nroots + k] = s2;
            rnorm[b * nroots + k] = rn[k];
        }
        __syncthreads();
    }
    if (tid == 0) info[b] = conv_all ? 0 : iters;
}

}  // namespace

// the shape of a problem, or a negative code with the message set
static int ci_shape(int ncas, int nelecas, int nroots, int* na_out)
{
    OOVQE_REQUIRE(ncas >= 1 && ncas <= CI_MAXA, "oovqe_ci: ncas = %d outside 1..%d", ncas, CI_MAXA);
    OOVQE_REQUIRE(nelecas >= 0 && nelecas <= 2 * ncas && nelecas % 2 == 0,
                  "oovqe_ci: nelecas = %d must be even and in 0..2 ncas (N_alpha = N_beta)", nelecas);
    const int na = ci_binom(ncas, nelecas / 2), Dc = na * na;
    OOVQE_REQUIRE(Dc <= CI_MAXDC, "oovqe_ci: %d determinants > %d", Dc, CI_MAXDC);
    const int rmax = Dc < CI_MAXR ? Dc : CI_MAXR;
    OOVQE_REQUIRE(nroots >= 1 && nroots <= rmax, "oovqe_ci: nroots = %d outside 1..%d", nroots, rmax);
    *na_out = na;
    return 0;
}

extern "C" int64_t oovqe_ci_work_size(int ncas, int nelecas, int nroots, int batch)
{
    int na = 0;
    const int rc = ci_shape(ncas, nelecas, nroots, &na);
    if (rc != 0) return rc;
    if (batch < 0) { oovqe_set_error("oovqe_ci_work_size: batch = %d", batch); return OOVQE_ERR_ARG; }
    return (int64_t)ci_work_per_problem(na, nroots) * batch;
}

extern "C" int oovqe_ci_davidson_shift_batch(int ncas, int nelecas, int nroots, int batch, const double* c0,
                                             const double* c1, const double* c2, int64_t c_stride,
                                             double spin_shift, double tol, int max_iter, double* energies,
                                             double* ci, double* s2, double* rnorm, int* info, double* work,
                                             oovqe_stream_t stream)
{
    int na = 0;
    const int rc = ci_shape(ncas, nelecas, nroots, &na);
    if (rc != 0) return rc;
    OOVQE_REQUIRE(batch >= 0, "oovqe_ci_davidson_batch: batch = %d", batch);
    if (batch == 0) return 0;
    OOVQE_REQUIRE(c0 && c1 && c2 && energies && ci && s2 && rnorm && info && work,
                  "oovqe_ci_davidson_batch: null pointer");
    OOVQE_REQUIRE(c_stride >= 0, "oovqe_ci_davidson_batch: c_stride = %lld", (long long)c_stride);
    OOVQE_REQUIRE(tol > 0.0 && max_iter >= 1, "oovqe_ci_davidson_batch: tol = %g, max_iter = %d", tol, max_iter);
    OOVQE_REQUIRE(spin_shift >= 0.0 && spin_shift <= 1e6, "oovqe_ci_davidson_batch: spin_shift = %g", spin_shift);
    const size_t lds = ci_lds_bytes(ncas, na);
    OOVQE_REQUIRE(lds <= 160 * 1024, "oovqe_ci_davidson_batch: %zu bytes of LDS", lds);
    if (oovqe_ensure_dynamic_lds(reinterpret_cast<const void*>(&ci_davidson_kernel), lds) != 0)
        return OOVQE_ERR_HIP;
    hipLaunchKernelGGL(ci_davidson_kernel, dim3(batch), dim3(CI_NT), lds, (hipStream_t)stream, ncas, nelecas / 2,
                       nroots, c0, c1, c2, (long)c_stride, spin_shift, tol, max_iter, energies, ci, s2, rnorm,
                       info, work, ci_work_per_problem(na, nroots));
    OOVQE_CHECK_LAUNCH("ci_davidson_kernel");
    return 0;
}

extern "C" int oovqe_ci_davidson_batch(int ncas, int nelecas, int nroots, int batch, const double* c0,
                                       const double* c1, const double* c2, int64_t c_stride, int fix_singlet,
                                       double tol, int max_iter, double* energies, double* ci, double* s2,
                                       double* rnorm, int* info, double* work, oovqe_stream_t stream)
{
    return oovqe_ci_davidson_shift_batch(ncas, nelecas, nroots, batch, c0, c1, c2, c_stride,
                                         fix_singlet ? CI_SPIN_SHIFT : 0.0, tol, max_iter, energies, ci, s2, rnorm,
                                         info, work, stream);
}
