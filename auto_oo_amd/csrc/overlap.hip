// Overlaps of sector vectors over non-orthogonal orbitals (gfx950): one launch, one workgroup per pair.
//
//   out[p][i][j] = sum_{J, I} bra_i[Ja, Jb] det U[occ(Ja), occ(Ia)] det U[occ(Jb), occ(Ib)] ket_j[Ia, Ib]
//
// for the (N_alpha, N_beta) sector of ncas orbitals, vectors in the layout c[ia * nb + ib] of the sector engine (strings
// ascending by value, orbital p at bit ncas - 1 - p).  Rows of U go with the bra, columns with the ket.  U is made from
// s[p] [m][m], m = n_core + ncas, the overlap of the occupied-plus-active orbitals of the bra geometry (rows) with those
// of the ket geometry (columns):
//
//   core fold    Gaussian elimination of the first n_core columns of s in LDS, pivoting among the core rows only:
//                core_det = det(s_cc) and the trailing block is U = s_aa - s_ac s_cc^-1 s_ca.  det of the whole occupied
//                block of one spin = det(s_cc) det(U[occ, occ]), so the all-electron overlap is core_det^2 out.
//   mode 1       U is replaced by the Q factor of U = Q R with a positive diagonal of R (modified Gram-Schmidt with a
//                second projection pass, one lane, at most 8 x 8)
//   minors       MT[I][J] = det U[occ(J), occ(I)] for the alpha and the beta strings, one determinant per lane at a
//                time: the order is a template parameter, the matrix lives in registers, rows are exchanged by selects
//                (partial pivoting: a permutation matrix is a legitimate U), a zero pivot column gives 0.  When N_alpha =
//                N_beta the strings and U coincide and one table serves both spins.
//   contraction  per ket:  K = ket (gathered, signed) -> T[Ja][Ib] = sum_Ia MT_a[Ia][Ja] K[Ia][Ib] -> W[Ja][Jb] =
//                sum_Ib T[Ja][Ib] MT_b[Ib][Jb], weighted at once with every bra (read from memory) into one partial sum
//                per lane and bra; a tree in LDS adds the lanes.
//
// LDS (doubles): m^2 + 64 + na^2 + (N_alpha != N_beta) nb^2 + 2 na nb + 256, at most 145 KB (ncas = 8, (4, 3)) and
// 136 KB for CAS(8e,8o): above 64 KB through the dynamic-LDS attribute.  Every sum has a fixed order that depends on the
// pair alone.  No atomics, no scratch, no MFMA: about 1.4 MFLOP per pair, the call is latency-bound and parallel over
// pairs.
#include "common.h"

#define OVL_NT 256
#define OVL_US 8                 // row stride of U

// sign of moving every alpha creation operator in front of the beta ones (berry.sector_tables)
__host__ __device__ __forceinline__ double ovl_sign(unsigned ma, unsigned mb)
{
    int n = 0;
    while (ma) {
        const int b = __builtin_ffs((int)ma) - 1;
        n += __builtin_popcount(mb >> (b + 1));
        ma &= ma - 1;
    }
    return (n & 1) ? -1.0 : 1.0;
}

// det U[occ(mj), occ(mi)] of order K: occupied orbitals ascending = set bits descending
template <int K>
__host__ __device__ __forceinline__ double ovl_minor(const double* __restrict__ U, int ncas, unsigned mj,
                                                     unsigned mi)
{
    if constexpr (K == 0) {
        return 1.0;
    } else {
        int rj[K], ci[K];
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const int hj = 31 - (mj ? __builtin_clz(mj) : 32), hi = 31 - (mi ? __builtin_clz(mi) : 32);
            rj[r] = (ncas - 1 - hj) * OVL_US;
            ci[r] = ncas - 1 - hi;
            mj &= ~(1u << hj);
            mi &= ~(1u << hi);
        }
        double a[K][K];
#pragma unroll
        for (int r = 0; r < K; ++r)
#pragma unroll
            for (int c = 0; c < K; ++c) a[r][c] = U[rj[r] + ci[c]];
        double det = 1.0;
#pragma unroll
        for (int c = 0; c < K; ++c) {
            int piv = c;
            double best = fabs(a[c][c]);
#pragma unroll
            for (int r = c + 1; r < K; ++r) {
                const double v = fabs(a[r][c]);
                const bool up = v > best;
                best = up ? v : best;
                piv = up ? r : piv;
            }
#pragma unroll
            for (int r = c + 1; r < K; ++r) {
                const bool sw = piv == r;
#pragma unroll
                for (int j = c; j < K; ++j) {
                    const double x = a[c][j], y = a[r][j];
                    a[c][j] = sw ? y : x;
                    a[r][j] = sw ? x : y;
                }
            }
            const double pv = a[c][c];
            det = piv != c ? -det : det;
            det *= pv;
            const double inv = pv != 0.0 ? 1.0 / pv : 0.0;
#pragma unroll
            for (int r = c + 1; r < K; ++r) {
                const double l = a[r][c] * inv;
#pragma unroll
                for (int j = c + 1; j < K; ++j) a[r][j] -= l * a[c][j];
            }
        }
        return det;
    }
}

#ifndef OVERLAP_BODIES_ONLY
template <int K>
__device__ __forceinline__ void ovl_minors(double* __restrict__ MT, const double* __restrict__ U, int ncas,
                                           const int* __restrict__ str, int n, int t)
{
    for (int e = t; e < n * n; e += OVL_NT) {
        const int I = e / n, J = e - I * n;
        MT[e] = ovl_minor<K>(U, ncas, (unsigned)str[J], (unsigned)str[I]);
    }
}

__device__ __forceinline__ void ovl_minors_of(int k, double* MT, const double* U, int ncas, const int* str, int n, int t)
{
    switch (k) {
        case 0: ovl_minors<0>(MT, U, ncas, str, n, t); break;
        case 1: ovl_minors<1>(MT, U, ncas, str, n, t); break;
        case 2: ovl_minors<2>(MT, U, ncas, str, n, t); break;
        case 3: ovl_minors<3>(MT, U, ncas, str, n, t); break;
        case 4: ovl_minors<4>(MT, U, ncas, str, n, t); break;
        case 5: ovl_minors<5>(MT, U, ncas, str, n, t); break;
        case 6: ovl_minors<6>(MT, U, ncas, str, n, t); break;
        case 7: ovl_minors<7>(MT, U, ncas, str, n, t); break;
        default: ovl_minors<8>(MT, U, ncas, str, n, t); break;
    }
}

struct ovl_args_t {
    const double* s; const double* bra; const double* ket; const int32_t* index; double* out; double* core_det;
    long ld;
    int m, n_core, ncas, n_alpha, n_beta, na, nb, rb, rk, mode, sgn;
};

__global__ __launch_bounds__(OVL_NT) void sector_overlap_kernel(const ovl_args_t a)
{
    extern __shared__ double lds[];
    __shared__ int strA[70], strB[70];
    __shared__ int sh_piv;
    const int t = threadIdx.x, p = blockIdx.x;
    const int m = a.m, nc = a.n_core, ncas = a.ncas, na = a.na, nb = a.nb, D = na * nb;
    const bool shared = a.n_alpha == a.n_beta;
    double* S = lds;
    double* U = S + m * m;
    double* MTa = U + OVL_US * OVL_US;
    double* MTb = shared ? MTa : MTa + na * na;
    double* K = MTb + nb * nb;
    double* T = K + D;
    double* red = T + D;

    // strings ascending by value, one lane per spin
    if (t == 0 || t == 64) {
        int* str = t == 0 ? strA : strB;
        const int want = t == 0 ? a.n_alpha : a.n_beta, lim = t == 0 ? na : nb;
        int n = 0;
        for (int v = 0; v < (1 << ncas); ++v)
            if (__popc(v) == want && n < lim) str[n++] = v;
    }
    const double* sp = a.s + (size_t)p * m * m;
    for (int i = t; i < m * m; i += OVL_NT) S[i] = sp[i];
    __syncthreads();

    // ---- core fold -------------------------------------------------------------------------------------------------
    double det = 1.0;                       // (lane 0)
    bool singular = false;
    for (int c = 0; c < nc; ++c) {
        if (t == 0) {
            int piv = c;
            double best = fabs(S[c * m + c]);
            for (int r = c + 1; r < nc; ++r) {
                const double v = fabs(S[r * m + c]);
                if (v > best) { best = v; piv = r; }
            }
            sh_piv = piv;
            det *= S[piv * m + c];
            if (piv != c) det = -det;
        }
        __syncthreads();
        const int piv = sh_piv;
        if (piv != c)
            for (int j = t; j < m; j += OVL_NT) {
                const double x = S[c * m + j];
                S[c * m + j] = S[piv * m + j];
                S[piv * m + j] = x;
            }
        __syncthreads();
        const double pv = S[c * m + c];
        if (pv == 0.0 || pv != pv) { singular = true; break; }       // (the same in every lane)
        const int w = m - c - 1;
        for (int e = t; e < w * w; e += OVL_NT) {
            const int r = c + 1 + e / w, j = c + 1 + e % w;
            S[r * m + j] -= S[r * m + c] / pv * S[c * m + j];
        }
        __syncthreads();
    }
    if (t == 0) a.core_det[p] = singular ? 0.0 : det;
    if (t < OVL_US * OVL_US) {
        const int i = t / OVL_US, j = t % OVL_US;
        double u = 0.0;
        if (i < ncas && j < ncas) u = singular ? __builtin_nan("") : S[(nc + i) * m + nc + j];
        U[t] = u;
    }
    __syncthreads();

    // ---- Q factor of U (positive diagonal of R) -----------------------------------------------------------------------
    if (a.mode == 1) {
        if (t == 0) {
            for (int k = 0; k < ncas; ++k) {
                for (int pass = 0; pass < 2; ++pass)
                    for (int j = 0; j < k; ++j) {
                        double r = 0.0;
                        for (int i = 0; i < ncas; ++i) r += U[i * OVL_US + j] * U[i * OVL_US + k];
                        for (int i = 0; i < ncas; ++i) U[i * OVL_US + k] -= r * U[i * OVL_US + j];
                    }
                double n2 = 0.0;
                for (int i = 0; i < ncas; ++i) n2 += U[i * OVL_US + k] * U[i * OVL_US + k];
                const double nrm = sqrt(n2);
                for (int i = 0; i < ncas; ++i) U[i * OVL_US + k] = U[i * OVL_US + k] / nrm;
            }
        }
        __syncthreads();
    }

    // ---- minors ----------------------------------------------------------------------------------------------------
    ovl_minors_of(a.n_alpha, MTa, U, ncas, strA, na, t);
    if (!shared) ovl_minors_of(a.n_beta, MTb, U, ncas, strB, nb, t);
    __syncthreads();

    // ---- contraction -------------------------------------------------------------------------------------------------
    const unsigned long ld = (unsigned long)a.ld;
    const double* brap = a.bra + (size_t)p * a.rb * a.ld;
    const double* ketp = a.ket + (size_t)p * a.rk * a.ld;
    for (int j = 0; j < a.rk; ++j) {
        const double* kv = ketp + (size_t)j * a.ld;
        for (int e = t; e < D; e += OVL_NT) {
            const int ia = e / nb, ib = e - ia * nb;
            const unsigned long x = a.index ? (unsigned long)(long)a.index[e] : (unsigned long)e;
            double v = x < ld ? kv[x] : 0.0;
            if (a.sgn) v *= ovl_sign((unsigned)strA[ia], (unsigned)strB[ib]);
            K[e] = v;
        }
        __syncthreads();
        for (int e = t; e < D; e += OVL_NT) {
            const int ja = e / nb, ib = e - ja * nb;
            double v = 0.0;
            for (int ia = 0; ia < na; ++ia) v += MTa[ia * na + ja] * K[ia * nb + ib];
            T[e] = v;
        }
        __syncthreads();
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int e = t; e < D; e += OVL_NT) {
            const int ja = e / nb, jb = e - ja * nb;
            double w = 0.0;
            for (int ib = 0; ib < nb; ++ib) w += T[ja * nb + ib] * MTb[ib * nb + jb];
            if (a.sgn) w *= ovl_sign((unsigned)strA[ja], (unsigned)strB[jb]);
            const unsigned long x = a.index ? (unsigned long)(long)a.index[e] : (unsigned long)e;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < a.rb) acc[i] += (x < ld ? brap[(size_t)i * a.ld + x] : 0.0) * w;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < a.rb) {                 // (the same in every lane)
                red[t] = acc[i];
                __syncthreads();
                for (int o = OVL_NT / 2; o > 0; o >>= 1) {
                    if (t < o) red[t] += red[t + o];
                    __syncthreads();
                }
                if (t == 0) a.out[((size_t)p * a.rb + i) * a.rk + j] = red[0];
                __syncthreads();
            }
        }
    }
}

static int ovl_binomial(int n, int k)
{
    long c = 1;
    for (int i = 1; i <= k; ++i) c = c * (n - k + i) / i;
    return (int)c;
}

extern "C" int oovqe_sector_overlap_batch(const double* s, int m, int n_core, int ncas, int n_alpha, int n_beta,
                                          int npair, const double* bra, int rb, const double* ket, int rk,
                                          const int32_t* index, int64_t ld, int mode, int with_signs, double* out,
                                          double* core_det, oovqe_stream_t stream)
{
    const char* who = "oovqe_sector_overlap_batch";
    static_assert(OOVQE_OVERLAP_MAX_ROOTS == 4 && OOVQE_OVERLAP_MAX_NCAS == 8, "the kernel's register arrays");
    OOVQE_REQUIRE(ncas >= 1 && ncas <= OOVQE_OVERLAP_MAX_NCAS, "%s: ncas = %d (1 .. %d)", who, ncas,
                  OOVQE_OVERLAP_MAX_NCAS);
    OOVQE_REQUIRE(n_core >= 0 && m == n_core + ncas && m <= OOVQE_OVERLAP_MAX_M,
                  "%s: m = %d, n_core = %d, ncas = %d (m = n_core + ncas <= %d)", who, m, n_core, ncas,
                  OOVQE_OVERLAP_MAX_M);
    OOVQE_REQUIRE(n_alpha >= 0 && n_alpha <= ncas && n_beta >= 0 && n_beta <= ncas,
                  "%s: (N_alpha, N_beta) = (%d, %d) in %d orbitals", who, n_alpha, n_beta, ncas);
    const int na = ovl_binomial(ncas, n_alpha), nb = ovl_binomial(ncas, n_beta);
    OOVQE_REQUIRE(na <= OOVQE_OVERLAP_MAX_STRINGS && nb <= OOVQE_OVERLAP_MAX_STRINGS, "%s: %d x %d strings (<= %d)", who,
                  na, nb, OOVQE_OVERLAP_MAX_STRINGS);
    OOVQE_REQUIRE(rb >= 1 && rb <= OOVQE_OVERLAP_MAX_ROOTS && rk >= 1 && rk <= OOVQE_OVERLAP_MAX_ROOTS,
                  "%s: %d bra and %d ket vectors per pair (1 .. %d)", who, rb, rk, OOVQE_OVERLAP_MAX_ROOTS);
    OOVQE_REQUIRE(mode == 0 || mode == 1, "%s: mode = %d (0: U as it is, 1: its Q factor)", who, mode);
    OOVQE_REQUIRE(npair >= 0, "%s: npair = %d", who, npair);
    OOVQE_REQUIRE(index ? ld >= 1 : ld >= (int64_t)na * nb, "%s: ld = %lld (%s)", who, (long long)ld,
                  index ? "at least 1 with an index table" : "at least na nb without one");
    if (npair == 0) return 0;
    OOVQE_REQUIRE(s && bra && ket && out && core_det, "%s: null pointer", who);
    const size_t doubles = (size_t)m * m + OVL_US * OVL_US + (size_t)na * na + (n_alpha == n_beta ? 0 : (size_t)nb * nb) +
                           2 * (size_t)na * nb + OVL_NT;
    const size_t bytes = doubles * sizeof(double);
    OOVQE_REQUIRE(bytes <= 160 * 1024 - 1024, "%s: %zu bytes of LDS", who, bytes);
    int rc = oovqe_ensure_dynamic_lds(reinterpret_cast<const void*>(sector_overlap_kernel), bytes);
    if (rc != 0) return rc;
    const ovl_args_t a = {s, bra, ket, index, out, core_det, (long)ld, m, n_core, ncas, n_alpha, n_beta, na, nb, rb, rk,
                          mode, with_signs != 0};
    hipLaunchKernelGGL(sector_overlap_kernel, dim3((unsigned)npair), dim3(OVL_NT), bytes, (hipStream_t)stream, a);
    OOVQE_CHECK_LAUNCH("sector_overlap_kernel");
    return 0;
}
#endif  // OVERLAP_BODIES_ONLY
