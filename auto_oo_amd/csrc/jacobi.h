// Cyclic Jacobi for a symmetric matrix on ONE wave (gfx950), shared by the S^-1/2 kernel (gto.hip) and the
// eigensolver of the SCF kernels (scf.hip).
#pragma once
#include "common.h"

#define JACOBI_NT 64            // lanes of the wave that runs sym_jacobi_wave

// pair k of round r of the round-robin schedule over n2 (even) indices: index n2 - 1 stays, the others rotate
__device__ __forceinline__ void invsqrt_pair(int k, int r, int n2, int& p, int& q)
{
    const int a = (k == 0) ? r : (r + k) % (n2 - 1), b = (k == 0) ? n2 - 1 : (r - k + n2 - 1) % (n2 - 1);
    p = a < b ? a : b;
    q = a < b ? b : a;
}

// Parallel (round-robin) ordering: the rotations of the n / 2 disjoint pairs of a round are computed by n / 2 lanes at
// once and applied in two passes (lane = row, then lane = column).  On entry A [n][ld] (LDS) is exactly symmetric and
// U [n][ld] (LDS) is the identity; on return the diagonal of A holds the eigenvalues (unordered) and the columns of U
// the eigenvectors.  cs: JACOBI_NT doubles, pq: JACOBI_NT ints of LDS (the (cos, sin) and index pairs of a round).
// Every lane of the wave calls it; a NaN in A leaves after the first test.
__device__ __forceinline__ void sym_jacobi_wave(double* A, double* U, double* cs, int* pq, int n, int ld, int lane)
{
    const int n2 = n + (n & 1), m = n2 / 2;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, dg = 0.0;
        if (lane < n) {
            for (int c = 0; c < n; ++c) {
                const double x = fabs(A[lane * ld + c]);
                if (c == lane) dg = fmax(dg, x); else off = fmax(off, x);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            off = fmax(off, __shfl_xor(off, o, 64));
            dg = fmax(dg, __shfl_xor(dg, o, 64));
        }
        if (!(off > 1e-15 * fmax(dg, 1e-300))) break;      // (also leaves on NaN)
        // one sweep = n2 - 1 rounds of the round-robin schedule: the n2 / 2 pairs of a round are disjoint, so their
        // rotations J commute; A <- J^T A J as a column pass (lane = row) and a row pass (lane = column)
        for (int r = 0; r < n2 - 1; ++r) {
            int p = 0, q = n;
            double c = 1.0, s = 0.0;
            if (lane < m) {
                invsqrt_pair(lane, r, n2, p, q);
                if (q < n) {
                    const double apq = A[p * ld + q];
                    if (fabs(apq) > 1e-300) {
                        const double tau = (A[q * ld + q] - A[p * ld + p]) / (2.0 * apq);
                        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                        c = 1.0 / sqrt(1.0 + t * t);
                        s = t * c;
                    }
                }
                cs[2 * lane] = c;
                cs[2 * lane + 1] = (q < n) ? s : 0.0;
                pq[2 * lane] = p;
                pq[2 * lane + 1] = (q < n) ? q : p;           // (an idle pair has s = 0 and is skipped)
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            // the pairs of a round are disjoint: four at a time, all loads of a group before its stores (the compiler
            // cannot know that the stores of one pair leave the loads of the next alone; one pair at a time was a
            // chain of LDS round trips)
            if (lane < n) {
                for (int k0 = 0; k0 < m; k0 += 4) {
                    double ap[4], aq[4], up[4], uq[4], ck[4], sk[4];
                    int pk[4], qk[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int k = (k0 + j < m) ? k0 + j : 0;
                        pk[j] = pq[2 * k]; qk[j] = pq[2 * k + 1];
                        ck[j] = cs[2 * k]; sk[j] = (k0 + j < m) ? cs[2 * k + 1] : 0.0;
                        ap[j] = A[lane * ld + pk[j]]; aq[j] = A[lane * ld + qk[j]];
                        up[j] = U[lane * ld + pk[j]]; uq[j] = U[lane * ld + qk[j]];
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (sk[j] != 0.0) {
                            A[lane * ld + pk[j]] = ck[j] * ap[j] - sk[j] * aq[j];
                            A[lane * ld + qk[j]] = sk[j] * ap[j] + ck[j] * aq[j];
                            U[lane * ld + pk[j]] = ck[j] * up[j] - sk[j] * uq[j];
                            U[lane * ld + qk[j]] = sk[j] * up[j] + ck[j] * uq[j];
                        }
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            if (lane < n) {
                for (int k0 = 0; k0 < m; k0 += 4) {
                    double ap[4], aq[4], ck[4], sk[4];
                    int pk[4], qk[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int k = (k0 + j < m) ? k0 + j : 0;
                        pk[j] = pq[2 * k]; qk[j] = pq[2 * k + 1];
                        ck[j] = cs[2 * k]; sk[j] = (k0 + j < m) ? cs[2 * k + 1] : 0.0;
                        ap[j] = A[pk[j] * ld + lane]; aq[j] = A[qk[j] * ld + lane];
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (sk[j] != 0.0) {
                            A[pk[j] * ld + lane] = ck[j] * ap[j] - sk[j] * aq[j];
                            A[qk[j] * ld + lane] = sk[j] * ap[j] + ck[j] * aq[j];
                        }
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            if (lane < m && q < n && s != 0.0) {
                A[p * ld + q] = 0.0;               // (annihilated up to rounding: made exact)
                A[q * ld + p] = 0.0;
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        }
    }
}
