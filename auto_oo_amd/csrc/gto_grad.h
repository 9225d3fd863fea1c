// Shared by the nuclear-derivative kernels of gto_grad.hip and gto_grad_sets.hip: the record of a pair / quartet, the
// small sums over Hermite indices, derivative coefficients, and the count of records of a call; and the host code the
// derivative entries (those two, gto_connection.hip) share: the nset check, the fork onto the internal stream, the split
// of the sets into tiles and the ladder over the quartet classes and their sides.
#pragma once
#include "gto.h"

#define GRAD_REC 16
#define GRAD_RT 256              // threads of the reduction

// ---- small sums over Hermite indices (all bounds compile-time) ------------------------------------------------------
// sum_{t <= N0, u <= N1, w <= N2} (-1)^(t+u+w) c0[t] c1[u] c2[w] R[T + t][U + u][W + w]
template <int T, int U, int W, int N0, int N1, int N2, int M, int DIM>
__device__ __forceinline__ double gto_ket_sum(const double (&c0)[M], const double (&c1)[M], const double (&c2)[M],
                                              const double (&R)[DIM][DIM][DIM])
{
    // (nested, innermost factor first: no product of coefficients alone exists that could be kept across a loop)
    double x = 0.0;
#pragma unroll
    for (int t = 0; t <= N0; ++t) {
        double xu = 0.0;
#pragma unroll
        for (int u = 0; u <= N1; ++u) {
            double xw = 0.0;
#pragma unroll
            for (int w = 0; w <= N2; ++w) xw += ((w & 1) ? -c2[w] : c2[w]) * R[T + t][U + u][W + w];
            xu += ((u & 1) ? -c1[u] : c1[u]) * xw;
        }
        x += ((t & 1) ? -c0[t] : c0[t]) * xu;
    }
    return x;
}

// sum_{t <= N0, u <= N1, w <= N2} c0[t] c1[u] c2[w] X[t + S0][u + S1][w + S2]
template <int N0, int N1, int N2, int S0, int S1, int S2, int M, int DIM>
__device__ __forceinline__ double gto_bra_sum(const double (&c0)[M], const double (&c1)[M], const double (&c2)[M],
                                              const double (&X)[DIM][DIM][DIM])
{
    double v = 0.0;
#pragma unroll
    for (int t = 0; t <= N0; ++t) {
        double vu = 0.0;
#pragma unroll
        for (int u = 0; u <= N1; ++u) {
            double vw = 0.0;
#pragma unroll
            for (int w = 0; w <= N2; ++w) vw += c2[w] * X[t + S0][u + S1][w + S2];
            vu += c1[u] * vw;
        }
        v += c0[t] * vu;
    }
    return v;
}

// derivative coefficients with respect to the FIRST centre: dE[i][j][t] = 2a E[i+1][j][t] - i E[i-1][j][t], t <= i+j+1
template <int LA, int LB>
__device__ __forceinline__ void gto_herm_deriv(double (&dE)[LA + 1][LB + 1][LA + LB + 2],
                                               const double (&E)[LA + 2][LB + 1][LA + LB + 2], double a)
{
#pragma unroll
    for (int i = 0; i <= LA; ++i)
#pragma unroll
        for (int j = 0; j <= LB; ++j)
#pragma unroll
            for (int t = 0; t <= LA + LB + 1; ++t) {
                double v = 2.0 * a * E[i + 1][j][t];
                if (i >= 1) v -= (double)i * E[i >= 1 ? i - 1 : 0][j][t];
                dE[i][j][t] = v;
            }
}

// kinetic factor of one dimension, powers (I, J): -2 b^2 S(I, J+2) + b (2J+1) S(I, J) - J (J-1) / 2 S(I, J-2)
template <int I, int J, int NI, int NJ, int NT>
__device__ __forceinline__ double gto_kin1(const double (&E)[NI][NJ][NT], double b)
{
    if constexpr (I < 0) {
        return 0.0;
    } else {
        double v = -2.0 * b * b * E[I][J + 2][0] + b * (double)(2 * J + 1) * E[I][J][0];
        if constexpr (J >= 2) v -= 0.5 * (double)(J * (J - 1)) * E[I][J - 2][0];
        return v;
    }
}
template <int I, int J, int NI, int NJ, int NT>
__device__ __forceinline__ double gto_ovl1(const double (&E)[NI][NJ][NT])
{
    if constexpr (I < 0) return 0.0;
    else return E[I][J][0];
}

__device__ __forceinline__ void grad_store(double* __restrict__ rec, int a0, int a1, int a2, int a3,
                                           const double (&v)[12])
{
    d2* o = reinterpret_cast<d2*>(rec);
#pragma unroll
    for (int k = 0; k < 6; ++k) { d2 x; x.x = v[2 * k]; x.y = v[2 * k + 1]; o[k] = x; }
    d2 x;
    x.x = (double)a0; x.y = (double)a1; o[6] = x;
    x.x = (double)a2; x.y = (double)a3; o[7] = x;
}

// ---- records of a call ----------------------------------------------------------------------------------------------------
static inline int64_t grad_records(int nshell, int natm)
{
    const int64_t npair = (int64_t)nshell * (nshell + 1) / 2;
    return npair * (natm + 1) + npair * (npair + 1) * 3;     // (at most: every quartet (pp|pp))
}

// gto_grad_reduce_kernel (gto_grad.hip) for `rows` stacks of nrec records each, stack r to grad[r][natm][3]; with_nuc
// adds the nuclear repulsion of coords[r]
int gto_grad_reduce_launch(const double* rec, long nrec, const double* charges, int natm, const double* coords,
                           int with_nuc, long rows, double* grad, hipStream_t st);

// records per quartet: two sides; (pp|pp) in three launches per side (GRAD_PPPP_PARTS)
#define GRAD_PPPP_PARTS 3
template <int LA, int LB, int LC, int LD> constexpr int grad_parts()
{
    return (LA + LB + LC + LD == 4) ? GRAD_PPPP_PARTS : 1;
}

// ---- host side shared by the derivative entries -----------------------------------------------------------------------
static inline int grad_check_nset(const char* who, int nset)
{
    OOVQE_REQUIRE(nset >= 1 && nset <= OOVQE_GTO_GRAD_MAX_SETS, "%s: nset = %d (1 .. %d)", who, nset,
                  OOVQE_GTO_GRAD_MAX_SETS);
    return 0;
}

// the records of the terms asked for, one-electron pairs first
static inline long grad_nrec(const gto_prep_t& p, bool one, bool two)
{
    const long npair = p.npair(), npp = p.cnt[gto_cls(1, 1)];
    return (one ? npair * (p.natm + 1) : 0) + (two ? npair * (npair + 1) + (GRAD_PPPP_PARTS - 1) * npp * (npp + 1) : 0);
}

// The launches of a call are independent of each other up to the reduction, and each lasts as long as one lane's chain
// of primitive quartets while filling a fraction of the chip: the second sides of the quartets run on the library's
// internal stream, forked from the caller's stream behind the pair data and joined in front of the reduction.  Every
// launch writes its own records, so the result does not depend on how they overlap.
// fork() leaves side = st where no fork is wanted or the library has no second stream; join() is called on the one way
// out of the launches, whatever they returned, and the destructor joins on any other: the caller's stream never runs
// ahead of the fork.  (gto_grad.hip)
struct grad_fork_t {
    const char* who = nullptr;
    hipStream_t st = nullptr, side = nullptr;
    hipEvent_t ev_join = nullptr;
    int fork(const char* who, hipStream_t st, bool wanted);
    int join();
    ~grad_fork_t() { (void)join(); }
};

// the sets spread evenly over the fewest tiles of at most `tile`: 10 -> 5 + 5, 6 -> 3 + 3 (a set's bits do not depend on
// the split); f(k0, nk) for every tile, up to the first return code that is not 0
template <class F> int grad_for_tiles(int nset, int tile, F&& f)
{
    const int ntile = (nset + tile - 1) / tile;
    int rc = 0;
    for (int t = 0, k0 = 0; t < ntile && rc == 0; ++t) {
        const int nk = (nset - k0 + (ntile - t) - 1) / (ntile - t);
        rc = f(k0, nk);
        k0 += nk;
    }
    return rc;
}

// One side of the quartets of a bra class and a ket class of the enumeration, the other side's first shell restricted
// to component PART of NPART, as a value (gto_cls_t): the launcher of an entry deduces its kernel from it.
template <int LA, int LB, int LC, int LD, bool SWAP, int PART, int NPART> struct grad_side_t {};

// both sides of the quartets of bra class (LA, LB) and ket class (LC, LD): side(grad_side_t, grid, nbra, nket, nq, off)
// launches one
template <int LA, int LB, int LC, int LD, class S>
int grad_launch_eri(gto_cls_t<LA, LB, LC, LD>, const gto_prep_t& p, long& off, S&& side)
{
    const int nbra = p.cnt[gto_cls(LA, LB)], nket = p.cnt[gto_cls(LC, LD)];
    const long nq = gto_quartets(LA == LC && LB == LD, nbra, nket);
    if (nq == 0) return 0;
    constexpr int NP = grad_parts<LA, LB, LC, LD>();
    unsigned grid;
    int rc = gto_grid_split(p.who, nq * p.batch, &grid);
    static_for<NP>([&](auto part) {
        if (rc == 0) rc = side(grad_side_t<LA, LB, LC, LD, false, decltype(part)::value, NP>{}, grid, nbra, nket, nq, off);
    });
    static_for<NP>([&](auto part) {
        if (rc == 0) rc = side(grad_side_t<LC, LD, LA, LB, true, decltype(part)::value, NP>{}, grid, nbra, nket, nq, off);
    });
    if (rc == 0) off += 2 * nq * NP;
    return rc;
}

// The launches of one call (of one tile of sets): the quartets (`two`) through side(...) as above, the long threads of
// (pp|pp) first, as in oovqe_gto_integrals_batch; their records lie behind the pairs'.  Then the pairs (`one`) through
// pair(gto_cls_t, off), which launches a class and advances off by its records.
template <class S, class O> int grad_launch_all(const gto_prep_t& p, bool one, bool two, long nrec, S&& side, O&& pair)
{
    long off = 0;
    int rc = 0;
    if (two) {
        off = one ? p.npair() * (p.natm + 1) : 0;
        rc = gto_sp_quartets([&](auto c) { return grad_launch_eri(c, p, off, side); });
        if (rc == 0 && off != nrec) {
            oovqe_set_error("%s: %ld quartet records of %ld", p.who, off, nrec);
            rc = OOVQE_ERR_SIZE;
        }
    }
    if (one && rc == 0) {
        off = 0;
        rc = gto_sp_pairs([&](auto c) { return pair(c, off); });
    }
    return rc;
}
