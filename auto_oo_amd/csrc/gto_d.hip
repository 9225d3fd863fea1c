// Integral classes that contain a d shell (gfx950): ds, dp, dd one-electron pairs and the 15 quartet classes from
// (ds|ss) to (dd|dd).  The s/p kernels of gto.hip keep a whole quartet in one lane's registers; (dd|dd) would need 1296
// accumulators and 165 R_tuv per lane.  Here a WORKGROUP owns one (geometry, shell pair / quartet) and everything that
// is indexed by a component lives in LDS:
//
//   per primitive quartet, in order (bra primitive pair outer, ket primitive pair inner -- a fixed summation order):
//     1. lanes 0..2 build the Hermite coefficients of one dimension each in registers (gto_herm) and put them to LDS;
//        every lane evaluates the Boys function (the same bits in every lane), lanes 0..L put (-2 alpha)^n F_n to LDS
//     2. R^n_tuv level by level (t + u + v = 1 .. L), the entries of a level dealt out over the lanes, in LDS
//     3. X[ket component pair][t u v of the bra] = sum E^cd R, one entry per lane and pass
//     4. acc[bra component pair][ket component pair] += sum E^ab X, every accumulator owned by one lane (no atomics)
//   then the normalisation of the d components (sqrt 3 for xy, xz, yz) or the 6 -> 5 contraction to real solid
//   harmonics, one index after the other, in place in LDS, and the stores: every unique value to its (up to 8) places
//   from one register, by the rules of gto_eri_kernel.
//
// Every phase is a loop "for (i = lane; i < count; i += nlane)" followed by a barrier, so the bodies are
// __host__ __device__ functions of (workgroup index, lane, number of lanes): a CPU build runs them with lane = 0,
// nlane = 1 and no barrier.  All loops have run-time bounds (nothing is unrolled over components): the 15 + 3
// instantiations compile in seconds, and no per-thread array is indexed at run time (no scratch).
#include "gto.h"

// (t, u, v), t + u + v <= L, packed: t ascending, then u, then v
__host__ __device__ constexpr int gto_tet(int k) { return k * (k + 1) * (k + 2) / 6; }
__host__ __device__ __forceinline__ int gto_ridx(int L, int t, int u, int v)
{
    const int M = L - t;
    return gto_tet(L + 1) - gto_tet(M + 1) + u * (M + 1) - u * (u - 1) / 2 + v;
}
// the inverse, t | u << 8 | v << 16, for every packed index (once per workgroup)
__host__ __device__ __forceinline__ void gto_decode_fill(int* dec, int L, int lane, int nlane)
{
    const int n = gto_tet(L + 1);
    for (int i = lane; i < n; i += nlane) {
        int t = 0, u = 0;
        while (gto_ridx(L, t + 1, 0, 0) <= i) ++t;
        while (u + 1 <= L - t && gto_ridx(L, t, u + 1, 0) <= i) ++u;
        dec[i] = t | (u << 8) | ((i - gto_ridx(L, t, u, 0)) << 16);
    }
}

// R^n_tuv in LDS, Rn[n * NR + packed(t, u, v)], from Rn[n * NR] = (-2 alpha)^n F_n: level m needs levels m - 1 and
// m - 2 at n + 1.  The recursion goes down in t first, then u, then v, as gto_R does.  Ends with a barrier.
__host__ __device__ __forceinline__ void gto_R_build(double* Rn, const int* dec, int L, double X, double Y, double Z,
                                                     int lane, int nlane)
{
    const int NR = gto_tet(L + 1);
    for (int m = 1; m <= L; ++m) {
        for (int i = lane; i < NR; i += nlane) {
            const int t = dec[i] & 255, u = (dec[i] >> 8) & 255, v = dec[i] >> 16;
            if (t + u + v != m) continue;
            double x;
            int i1, i2, c;
            if (t > 0) {
                x = X; c = t - 1; i1 = gto_ridx(L, t - 1, u, v); i2 = c > 0 ? gto_ridx(L, t - 2, u, v) : 0;
            } else if (u > 0) {
                x = Y; c = u - 1; i1 = gto_ridx(L, 0, u - 1, v); i2 = c > 0 ? gto_ridx(L, 0, u - 2, v) : 0;
            } else {
                x = Z; c = v - 1; i1 = gto_ridx(L, 0, 0, v - 1); i2 = c > 0 ? gto_ridx(L, 0, 0, v - 2) : 0;
            }
            for (int n = 0; n <= L - m; ++n) {
                double val = x * Rn[(n + 1) * NR + i1];
                if (c > 0) val += (double)c * Rn[(n + 1) * NR + i2];
                Rn[n * NR + i] = val;
            }
        }
        gto_sync();
    }
}

// ---- one-electron integrals of the pair classes ds, dp, dd -----------------------------------------------------------
template <int LA, int LB> struct gto_d1_lds_t {
    static constexpr int L = LA + LB, NR = gto_tet(L + 1), NAB = gto_ncomp(LA) * gto_ncomp(LB);
    double S[NAB], T[NAB], V[NAB];
    double E[3][LA + 1][LB + 3][LA + LB + 3];
    double Rn[(L + 1) * NR];
    int dec[NR];
};
#define GTO_D1_NT 64

template <int LA, int LB>
__host__ __device__ __forceinline__ void gto_d_one_body(long grp, int lane, int nlane, gto_d1_lds_t<LA, LB>& s,
                                                        const int* __restrict__ iw, const int* __restrict__ shells,
                                                        int nshell, int count, const double* __restrict__ charges,
                                                        int natm, const double* __restrict__ coords, int batch,
                                                        const double* __restrict__ pairs, int kp, int nao,
                                                        double* __restrict__ overlap, double* __restrict__ h_ao)
{
    using lds_t = gto_d1_lds_t<LA, LB>;
    constexpr int NB = gto_ncomp(LB), NAB = lds_t::NAB, L = lds_t::L, NR = lds_t::NR;
    if (grp >= (long)count * batch) return;
    const int g = (int)(grp / count), k = (int)(grp - (long)g * count);
    const long npair = (long)nshell * (nshell + 1) / 2;
    const double* xyz = coords + (size_t)g * natm * 3;
    const gto_pair_ref_t ab = gto_pair_ref(iw + nshell, gto_cls(LA, LB), k, npair, iw, shells, xyz,
                                           pairs + (size_t)g * npair * kp * GTO_PW, kp);
    for (int c = lane; c < NAB; c += nlane) { s.S[c] = 0.0; s.T[c] = 0.0; s.V[c] = 0.0; }
    gto_decode_fill(s.dec, L, lane, nlane);
    gto_sync();
    for (int kab = 0; kab < ab.nprim; ++kab) {
        const gto_prim_t pr = gto_load_prim(ab.data + (size_t)kab * GTO_PW, ab.swapped);
        for (int d = lane; d < 3; d += nlane) {
            double E[LA + 1][LB + 3][LA + LB + 3];
            const double q = gto_pick(ab.AB, d);
            gto_herm<LA, LB + 2>(E, -pr.fb * q, pr.fa * q, pr.oo2p);
#pragma unroll
            for (int i = 0; i <= LA; ++i)
#pragma unroll
                for (int j = 0; j <= LB + 2; ++j)
#pragma unroll
                    for (int t = 0; t <= LA + LB + 2; ++t) s.E[d][i][j][t] = E[i][j][t];
        }
        gto_sync();
        const double b = pr.fb * pr.p;
        const double pop = GTO_PI / pr.p;
        const double fS = pr.cck * pop * sqrt(pop);
        for (int c = lane; c < NAB; c += nlane) {
            const int ca = c / NB, cb = c - ca * NB;
            double s1[3], t1[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const int i = gto_pow(LA, ca, d), j = gto_pow(LB, cb, d);
                s1[d] = s.E[d][i][j][0];
                double td = -2.0 * b * b * s.E[d][i][j + 2][0] + b * (double)(2 * j + 1) * s1[d];
                if (j >= 2) td -= 0.5 * (double)(j * (j - 1)) * s.E[d][i][j - 2][0];
                t1[d] = td;
            }
            s.S[c] += fS * (s1[0] * s1[1] * s1[2]);
            s.T[c] += fS * (t1[0] * s1[1] * s1[2] + s1[0] * t1[1] * s1[2] + s1[0] * s1[1] * t1[2]);
        }
        if (h_ao) {
            const double fV = -2.0 * GTO_PI / pr.p * pr.cck;
            for (int c = 0; c < natm; ++c) {
                const double X = pr.P[0] - xyz[3 * c], Y = pr.P[1] - xyz[3 * c + 1], Z = pr.P[2] - xyz[3 * c + 2];
                double F[L + 1];
                gto_boys<L>(pr.p * (X * X + Y * Y + Z * Z), F);
                double sc = fV * charges[c];
                static_for<L + 1>([&](auto nc) {
                    constexpr int n = decltype(nc)::value;
                    if (gto_mine(n, lane, nlane)) s.Rn[n * NR] = sc * F[n];
                    sc *= -2.0 * pr.p;
                });
                gto_sync();
                gto_R_build(s.Rn, s.dec, L, X, Y, Z, lane, nlane);
                for (int cc = lane; cc < NAB; cc += nlane) {
                    const int ca = cc / NB, cb = cc - ca * NB;
                    const int ix = gto_pow(LA, ca, 0), jx = gto_pow(LB, cb, 0), iy = gto_pow(LA, ca, 1),
                              jy = gto_pow(LB, cb, 1), iz = gto_pow(LA, ca, 2), jz = gto_pow(LB, cb, 2);
                    double v = 0.0;
                    for (int t = 0; t <= ix + jx; ++t)
                        for (int u = 0; u <= iy + jy; ++u)
                            for (int w = 0; w <= iz + jz; ++w)
                                v += s.E[0][ix][jx][t] * s.E[1][iy][jy][u] * s.E[2][iz][jz][w] *
                                     s.Rn[gto_ridx(L, t, u, w)];
                    s.V[cc] += v;
                }
                gto_sync();
            }
        }
        gto_sync();
    }
    // the form of the d shells (the flag of the l field), one index after the other
    const int fa = shells[4 * ab.sa + 1], fb = shells[4 * ab.sb + 1];
    int na = gto_ncomp(LA), nb = NB;
    if (LA == 2) {
        const bool cart = (fa & OOVQE_GTO_CARTESIAN) != 0;
        gto_d_pass(s.S, NAB, NB, cart, lane, nlane);
        gto_d_pass(s.T, NAB, NB, cart, lane, nlane);
        gto_d_pass(s.V, NAB, NB, cart, lane, nlane);
        na = cart ? 6 : 5;
    }
    if (LB == 2) {
        const bool cart = (fb & OOVQE_GTO_CARTESIAN) != 0;
        gto_d_pass(s.S, NAB, 1, cart, lane, nlane);
        gto_d_pass(s.T, NAB, 1, cart, lane, nlane);
        gto_d_pass(s.V, NAB, 1, cart, lane, nlane);
        nb = cart ? 6 : 5;
    }
    const bool same = ab.sa == ab.sb;
    for (int c = lane; c < NAB; c += nlane) {
        const int ca = c / NB, cb = c - ca * NB;
        if (ca >= na || cb >= nb) continue;
        const int mu = ab.oa + ca, nu = ab.ob + cb;
        if ((!same || mu >= nu) && mu < nao && nu < nao) {
            if (overlap) {
                const double x = s.S[c];
                overlap[((size_t)g * nao + mu) * nao + nu] = x;
                overlap[((size_t)g * nao + nu) * nao + mu] = x;
            }
            if (h_ao) {
                const double h = s.T[c] + s.V[c];
                h_ao[((size_t)g * nao + mu) * nao + nu] = h;
                h_ao[((size_t)g * nao + nu) * nao + mu] = h;
            }
        }
    }
}

#ifndef GTO_BODIES_ONLY
template <int LA, int LB>
__global__ __launch_bounds__(GTO_D1_NT) void gto_d_one_kernel(const int* __restrict__ iw,
                                                              const int* __restrict__ shells, int nshell, int count,
                                                              const double* __restrict__ charges, int natm,
                                                              const double* __restrict__ coords, int batch,
                                                              const double* __restrict__ pairs, int kp, int nao,
                                                              double* __restrict__ overlap, double* __restrict__ h_ao)
{
    __shared__ gto_d1_lds_t<LA, LB> s;
    gto_d_one_body<LA, LB>((long)blockIdx.x, (int)threadIdx.x, GTO_D1_NT, s, iw, shells, nshell, count, charges, natm,
                           coords, batch, pairs, kp, nao, overlap, h_ao);
}
#endif

// ---- two-electron integrals of the 15 quartet classes with a d shell -------------------------------------------------
template <int LA, int LB, int LC, int LD> struct gto_dq_lds_t {
    static constexpr int L = LA + LB + LC + LD, LAB = LA + LB, LCD = LC + LD;
    static constexpr int NR = gto_tet(L + 1), NRB = gto_tet(LAB + 1);
    static constexpr int NAB = gto_ncomp(LA) * gto_ncomp(LB), NCD = gto_ncomp(LC) * gto_ncomp(LD);
    // lanes of the workgroup: one wave, or four where a phase has more than 256 entries
    static constexpr int NT = (NCD * NRB > 256 || NAB * NCD > 256) ? 256 : 64;
    double acc[NAB * NCD];
    double Rn[(L + 1) * NR];
    double Xh[NCD * NRB];
    double Eb[3][LA + 1][LB + 1][LAB + 1];
    double Ek[3][LC + 1][LD + 1][LCD + 1];
    int dec[NR];
    int decb[NRB];
};

template <int LA, int LB, int LC, int LD>
__host__ __device__ __forceinline__ void gto_d_eri_body(long grp, int lane, int nlane,
                                                        gto_dq_lds_t<LA, LB, LC, LD>& s, const int* __restrict__ iw,
                                                        const int* __restrict__ shells, int nshell, int nbra,
                                                        int nket, long nquart, const double* __restrict__ coords,
                                                        int natm, int batch, const double* __restrict__ pairs, int kp,
                                                        int nao, double* __restrict__ g_ao)
{
    using lds_t = gto_dq_lds_t<LA, LB, LC, LD>;
    constexpr int NB = gto_ncomp(LB), NC = gto_ncomp(LC), ND = gto_ncomp(LD);
    constexpr int L = lds_t::L, LAB = lds_t::LAB, NR = lds_t::NR, NRB = lds_t::NRB, NAB = lds_t::NAB,
                  NCD = lds_t::NCD;
    constexpr bool same_cls = (LA == LC && LB == LD);
    if (grp >= nquart * batch) return;
    const int g = (int)(grp / nquart);
    const long r = grp - (long)g * nquart;
    int k1, k2;
    if (same_cls) {              // unique pairs of pairs k1 >= k2
        k1 = (int)((sqrt(8.0 * (double)r + 1.0) - 1.0) * 0.5);
        while ((long)(k1 + 1) * (k1 + 2) / 2 <= r) ++k1;
        while ((long)k1 * (k1 + 1) / 2 > r) --k1;
        k2 = (int)(r - (long)k1 * (k1 + 1) / 2);
    } else {
        k1 = (int)(r / nket);
        k2 = (int)(r - (long)k1 * nket);
    }
    if (k1 >= nbra || k2 >= nket) return;
    const long npair = (long)nshell * (nshell + 1) / 2;
    const double* xyz = coords + (size_t)g * natm * 3;
    const double* pairs_g = pairs + (size_t)g * npair * kp * GTO_PW;
    const gto_pair_ref_t ab = gto_pair_ref(iw + nshell, gto_cls(LA, LB), k1, npair, iw, shells, xyz, pairs_g, kp);
    const gto_pair_ref_t cd = gto_pair_ref(iw + nshell, gto_cls(LC, LD), k2, npair, iw, shells, xyz, pairs_g, kp);

    for (int c = lane; c < NAB * NCD; c += nlane) s.acc[c] = 0.0;
    gto_decode_fill(s.dec, L, lane, nlane);
    gto_decode_fill(s.decb, LAB, lane, nlane);
    gto_sync();
    for (int kab = 0; kab < ab.nprim; ++kab) {
        const gto_prim_t pb = gto_load_prim(ab.data + (size_t)kab * GTO_PW, ab.swapped);
        for (int d = lane; d < 3; d += nlane) {
            double E[LA + 1][LB + 1][LA + LB + 1];
            const double q = gto_pick(ab.AB, d);
            gto_herm<LA, LB>(E, -pb.fb * q, pb.fa * q, pb.oo2p);
#pragma unroll
            for (int i = 0; i <= LA; ++i)
#pragma unroll
                for (int j = 0; j <= LB; ++j)
#pragma unroll
                    for (int t = 0; t <= LA + LB; ++t) s.Eb[d][i][j][t] = E[i][j][t];
        }
        for (int kcd = 0; kcd < cd.nprim; ++kcd) {
            const gto_prim_t pk = gto_load_prim(cd.data + (size_t)kcd * GTO_PW, cd.swapped);
            for (int d = lane; d < 3; d += nlane) {
                double E[LC + 1][LD + 1][LC + LD + 1];
                const double q = gto_pick(cd.AB, d);
                gto_herm<LC, LD>(E, -pk.fb * q, pk.fa * q, pk.oo2p);
#pragma unroll
                for (int i = 0; i <= LC; ++i)
#pragma unroll
                    for (int j = 0; j <= LD; ++j)
#pragma unroll
                        for (int t = 0; t <= LC + LD; ++t) s.Ek[d][i][j][t] = E[i][j][t];
            }
            const double sum = pb.p + pk.p, alpha = pb.p * pk.p / sum;
            const double X = pb.P[0] - pk.P[0], Y = pb.P[1] - pk.P[1], Z = pb.P[2] - pk.P[2];
            double F[L + 1];
            gto_boys<L>(alpha * (X * X + Y * Y + Z * Z), F);
            // 2 pi^(5/2) / (p q sqrt(p + q)) and the two pair factors
            double sc = 34.98683665524972497 / (pb.p * pk.p * sqrt(sum)) * (pb.cck * pk.cck);
            static_for<L + 1>([&](auto nc) {
                constexpr int n = decltype(nc)::value;
                if (gto_mine(n, lane, nlane)) s.Rn[n * NR] = sc * F[n];
                sc *= -2.0 * alpha;
            });
            gto_sync();
            gto_R_build(s.Rn, s.dec, L, X, Y, Z, lane, nlane);
            // ket side first: X_tuv = sum_t'u'v' (-1)^(t'+u'+v') E^cd_t'u'v' R_(t+t', u+u', v+v') of a ket component pair
            for (int it = lane; it < NCD * NRB; it += nlane) {
                const int ccd = it / NRB, ib = it - ccd * NRB;
                const int t = s.decb[ib] & 255, u = (s.decb[ib] >> 8) & 255, w = s.decb[ib] >> 16;
                const int cc = ccd / ND, cd_ = ccd - cc * ND;
                const int kx = gto_pow(LC, cc, 0), lx = gto_pow(LD, cd_, 0), ky = gto_pow(LC, cc, 1),
                          ly = gto_pow(LD, cd_, 1), kz = gto_pow(LC, cc, 2), lz = gto_pow(LD, cd_, 2);
                double x = 0.0;
                for (int t2 = 0; t2 <= kx + lx; ++t2)
                    for (int u2 = 0; u2 <= ky + ly; ++u2) {
                        const double e2 = s.Ek[0][kx][lx][t2] * s.Ek[1][ky][ly][u2];
                        for (int w2 = 0; w2 <= kz + lz; ++w2) {
                            const double ek = e2 * s.Ek[2][kz][lz][w2];
                            const double sg = ((t2 + u2 + w2) & 1) ? -1.0 : 1.0;
                            x += sg * ek * s.Rn[gto_ridx(L, t + t2, u + u2, w + w2)];
                        }
                    }
                s.Xh[it] = x;
            }
            gto_sync();
            // then every bra component pair takes its few E^ab_tuv X_tuv
            for (int it = lane; it < NAB * NCD; it += nlane) {
                const int cab = it / NCD, ccd = it - cab * NCD;
                const int ca = cab / NB, cb = cab - ca * NB;
                const int ix = gto_pow(LA, ca, 0), jx = gto_pow(LB, cb, 0), iy = gto_pow(LA, ca, 1),
                          jy = gto_pow(LB, cb, 1), iz = gto_pow(LA, ca, 2), jz = gto_pow(LB, cb, 2);
                double v = 0.0;
                for (int t = 0; t <= ix + jx; ++t)
                    for (int u = 0; u <= iy + jy; ++u) {
                        const double e2 = s.Eb[0][ix][jx][t] * s.Eb[1][iy][jy][u];
                        for (int w = 0; w <= iz + jz; ++w)
                            v += e2 * s.Eb[2][iz][jz][w] * s.Xh[ccd * NRB + gto_ridx(LAB, t, u, w)];
                    }
                s.acc[it] += v;
            }
            gto_sync();
        }
    }
    // the form of the d shells, one index after the other (strides of the Cartesian layout [NA][NB][NC][ND])
    int nf[4] = {gto_ncomp(LA), NB, NC, ND};
    static_for<4>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        constexpr int lq = q == 0 ? LA : (q == 1 ? LB : (q == 2 ? LC : LD));
        constexpr int stride = q == 0 ? NB * NCD : (q == 1 ? NCD : (q == 2 ? ND : 1));
        if constexpr (lq == 2) {
            const int sh = q == 0 ? ab.sa : (q == 1 ? ab.sb : (q == 2 ? cd.sa : cd.sb));
            const bool cart = (shells[4 * sh + 1] & OOVQE_GTO_CARTESIAN) != 0;
            gto_d_pass(s.acc, NAB * NCD, stride, cart, lane, nlane);
            nf[q] = cart ? 6 : 5;
        }
    });
    // every unique value to its (up to 8) places, from one register; a value two components both stand for (same
    // shell twice in a pair, same pair twice in the quartet) is stored by one of them only
    const bool same_ab = ab.sa == ab.sb, same_cd = cd.sa == cd.sb;
    const bool same_pair = same_cls && ab.sa == cd.sa && ab.sb == cd.sb;
    double* out = g_ao + (size_t)g * nao * nao * nao * nao;
    const size_t n1 = (size_t)nao, n2 = n1 * n1, n3 = n2 * n1;
    for (int it = lane; it < NAB * NCD; it += nlane) {
        const int cab = it / NCD, ccd = it - cab * NCD;
        const int ca = cab / NB, cb = cab - ca * NB, cc = ccd / ND, cd_ = ccd - cc * ND;
        if (ca >= nf[0] || cb >= nf[1] || cc >= nf[2] || cd_ >= nf[3]) continue;
        const size_t mu = ab.oa + ca, nu = ab.ob + cb, la = cd.oa + cc, si = cd.ob + cd_;
        const size_t m1 = mu > nu ? mu : nu, m0 = mu > nu ? nu : mu, l1 = la > si ? la : si, l0 = la > si ? si : la;
        bool keep = m1 < n1 && l1 < n1;
        if (same_ab && mu < nu) keep = false;
        if (same_cd && la < si) keep = false;
        if (same_pair && m1 * (m1 + 1) / 2 + m0 < l1 * (l1 + 1) / 2 + l0) keep = false;
        if (keep) {
            const double x = s.acc[it];
            out[mu * n3 + nu * n2 + la * n1 + si] = x;
            out[nu * n3 + mu * n2 + la * n1 + si] = x;
            out[mu * n3 + nu * n2 + si * n1 + la] = x;
            out[nu * n3 + mu * n2 + si * n1 + la] = x;
            out[la * n3 + si * n2 + mu * n1 + nu] = x;
            out[si * n3 + la * n2 + mu * n1 + nu] = x;
            out[la * n3 + si * n2 + nu * n1 + mu] = x;
            out[si * n3 + la * n2 + nu * n1 + mu] = x;
        }
    }
}

#ifndef GTO_BODIES_ONLY
template <int LA, int LB, int LC, int LD>
__global__ __launch_bounds__((gto_dq_lds_t<LA, LB, LC, LD>::NT)) void gto_d_eri_kernel(
    const int* __restrict__ iw, const int* __restrict__ shells, int nshell, int nbra, int nket, long nquart,
    const double* __restrict__ coords, int natm, int batch, const double* __restrict__ pairs, int kp, int nao,
    double* __restrict__ g_ao)
{
    __shared__ gto_dq_lds_t<LA, LB, LC, LD> s;
    gto_d_eri_body<LA, LB, LC, LD>((long)blockIdx.x, (int)threadIdx.x, gto_dq_lds_t<LA, LB, LC, LD>::NT, s, iw, shells,
                                   nshell, nbra, nket, nquart, coords, natm, batch, pairs, kp, nao, g_ao);
}

// ---- host side ----------------------------------------------------------------------------------------------------
namespace {
template <int LA, int LB> int gto_d_launch_one(gto_cls_t<LA, LB>, const gto_prep_t& p, double* overlap, double* h_ao)
{
    const int count = p.cnt[gto_cls(LA, LB)];
    if (count == 0) return 0;
    unsigned grid;
    if (const int rc = gto_grid_wg(p.who, (long)count * p.batch, &grid)) return rc;
    hipLaunchKernelGGL((gto_d_one_kernel<LA, LB>), dim3(grid), dim3(GTO_D1_NT), 0, p.st, p.iw, p.shells, p.nshell, count,
                       p.charges, p.natm, p.coords, p.batch, p.pairs, p.kp, p.nao, overlap, h_ao);
    OOVQE_CHECK_LAUNCH("gto_d_one_kernel");
    return 0;
}

template <int LA, int LB, int LC, int LD> int gto_d_launch_eri(const gto_prep_t& p, double* g_ao)
{
    const int nbra = p.cnt[gto_cls(LA, LB)], nket = p.cnt[gto_cls(LC, LD)];
    const long nq = gto_quartets(LA == LC && LB == LD, nbra, nket);
    if (nq == 0) return 0;
    unsigned grid;
    if (const int rc = gto_grid_wg(p.who, nq * p.batch, &grid)) return rc;
    hipLaunchKernelGGL((gto_d_eri_kernel<LA, LB, LC, LD>), dim3(grid), dim3(gto_dq_lds_t<LA, LB, LC, LD>::NT), 0, p.st,
                       p.iw, p.shells, p.nshell, nbra, nket, nq, p.coords, p.natm, p.batch, p.pairs, p.kp, p.nao, g_ao);
    OOVQE_CHECK_LAUNCH("gto_d_eri_kernel");
    return 0;
}
}  // namespace

int gto_d_launch_one_electron(const gto_prep_t& p, double* overlap, double* h_ao)
{
    return gto_d_pairs([&](auto c) { return gto_d_launch_one(c, p, overlap, h_ao); });
}

// bra class >= ket class, the longest workgroups first
int gto_d_launch_two_electron(const gto_prep_t& p, double* g_ao)
{
    int rc;
#define GTO_D_ERI(la, lb, lc, ld) \
    if ((rc = gto_d_launch_eri<la, lb, lc, ld>(p, g_ao)) != 0) return rc
    GTO_D_ERI(2, 2, 2, 2); GTO_D_ERI(2, 2, 2, 1); GTO_D_ERI(2, 2, 2, 0); GTO_D_ERI(2, 2, 1, 1); GTO_D_ERI(2, 2, 1, 0);
    GTO_D_ERI(2, 2, 0, 0);
    GTO_D_ERI(2, 1, 2, 1); GTO_D_ERI(2, 1, 2, 0); GTO_D_ERI(2, 1, 1, 1); GTO_D_ERI(2, 1, 1, 0); GTO_D_ERI(2, 1, 0, 0);
    GTO_D_ERI(2, 0, 2, 0); GTO_D_ERI(2, 0, 1, 1); GTO_D_ERI(2, 0, 1, 0); GTO_D_ERI(2, 0, 0, 0);
#undef GTO_D_ERI
    return 0;
}
#endif  // GTO_BODIES_ONLY
