// Shared by the nuclear-derivative kernels of gto_grad.hip and gto_grad_sets.hip: the record of a pair / quartet, the
// small sums over Hermite indices, derivative coefficients, and the count of records of a call.
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
