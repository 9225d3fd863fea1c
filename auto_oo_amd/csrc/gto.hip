// Batched Gaussian integrals over a stack of geometries (gfx950): contracted s, p and d shells (d as 5 real solid
// harmonics or 6 Cartesian functions), McMurchie-Davidson.  The kernels of this file serve the classes of s and p
// shells; every class with a d shell is served by the workgroup-per-quartet kernels of gto_d.hip.  One basis description (shell table, exponents, normalised contraction coefficients,
// charges) is shared by all geometries; the geometry index is a grid dimension of every kernel.
//
//   gto_setup_kernel   AO offset of every shell and the shell pairs i >= j sorted into classes (la >= lb: ss, ps, pp,
//                      ds, dp, dd)
//   gto_pair_kernel    per geometry and primitive pair: p, P, c_a c_b exp(-mu |AB|^2), 1/(2p), a/p, b/p
//                      (8 doubles, in the work buffer) and the nuclear repulsion of the geometry.  The Hermite
//                      coefficients E_t^{ij} per dimension are polynomials in (P - A, P - B, 1/2p) times the
//                      exponential kept here: the consumers rebuild them in registers from these 8 doubles
//                      (a table of all E_t^{ij} would be 29 doubles per primitive pair read 81 times per quartet).
//   gto_one_kernel     <la, lb>: S, T, V of one shell pair per group of GTO_SPLIT lanes, all components together
//   gto_eri_kernel     <la, lb, lc, ld>: one unique shell quartet per group of GTO_SPLIT lanes (the primitive pairs of
//                      the bra dealt out over the lanes), all components together: Boys values and R_tuv once per
//                      primitive quartet; every unique value goes to its (up to 8) places from one register
//   sym_invsqrt_kernel S^-1/2 by cyclic Jacobi (round-robin ordering), one wave per matrix, matrix and vectors in LDS
//
// The device helpers (Boys function, Hermite coefficients, R_tuv, the readers of the pair data) live in gto.h, shared
// with the nuclear-derivative kernels of gto_grad.hip.
// l is a template parameter everywhere; these kernels are instantiated for l <= 1 (the component tables gto_ncomp /
// gto_pow are written for l <= GTO_LMAX = 2).  Every per-thread array is indexed by compile-time constants
// (static_for / fully unrolled loops of constant trip count), so none of them lives in scratch.
#include "gto.h"

__host__ __device__ inline void gto_setup_body(const int* __restrict__ shells, int nshell, int* __restrict__ iw)
{
    const int npair = nshell * (nshell + 1) / 2;
    int off = 0;
    for (int s = 0; s < nshell; ++s) {
        iw[s] = off;
        off += gto_nfunc(shells[4 * s + 1]);
    }
    int cnt[GTO_NCLS];
#pragma unroll
    for (int c = 0; c < GTO_NCLS; ++c) cnt[c] = 0;
    int* lists = iw + nshell;
    for (int i = 0; i < nshell; ++i) {
        for (int j = 0; j <= i; ++j) {
            const int li = gto_l_of(shells[4 * i + 1]), lj = gto_l_of(shells[4 * j + 1]);
            const int hi = (li >= lj) ? i : j, lo = (li >= lj) ? j : i;
            const int cls = gto_cls(li >= lj ? li : lj, li >= lj ? lj : li);
#pragma unroll
            for (int c = 0; c < GTO_NCLS; ++c) {          // (static index into cnt)
                if (c == cls) {
                    lists[((long)c * npair + cnt[c]) * 2 + 0] = hi;
                    lists[((long)c * npair + cnt[c]) * 2 + 1] = lo;
                    cnt[c] += 1;
                }
            }
        }
    }
}

#ifndef GTO_BODIES_ONLY
__global__ void gto_setup_kernel(const int* __restrict__ shells, int nshell, int* __restrict__ iw)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) gto_setup_body(shells, nshell, iw);
}
#endif

__host__ __device__ __forceinline__ void gto_pair_body(long tid, const int* __restrict__ shells, int nshell,
                                                       const double* __restrict__ exps,
                                                       const double* __restrict__ coefs,
                                                       const double* __restrict__ charges, int natm,
                                                       const double* __restrict__ coords, int batch, int kp,
                                                       double* __restrict__ pairs, double* __restrict__ nuc)
{
    const long npair = (long)nshell * (nshell + 1) / 2;
    const long per = npair * kp;
    if (tid >= per * batch) return;
    const int g = (int)(tid / per);
    const long r = tid - (long)g * per;
    const int pidx = (int)(r / kp), k = (int)(r - (long)pidx * kp);
    const double* xyz = coords + (size_t)g * natm * 3;
    if (r == 0 && nuc) {
        // the order of the host sum (gaussian.Moldata_sto3g): i ascending, j < i ascending
        double e = 0.0;
        for (int i = 0; i < natm; ++i) {
            for (int j = 0; j < i; ++j) {
                const double dx = xyz[3 * i] - xyz[3 * j], dy = xyz[3 * i + 1] - xyz[3 * j + 1],
                             dz = xyz[3 * i + 2] - xyz[3 * j + 2];
                e += charges[i] * charges[j] / sqrt(dx * dx + dy * dy + dz * dz);
            }
        }
        nuc[g] = e;
    }
    int i = (int)((sqrt(8.0 * (double)pidx + 1.0) - 1.0) * 0.5);
    while ((long)(i + 1) * (i + 2) / 2 <= pidx) ++i;
    while ((long)i * (i + 1) / 2 > pidx) --i;
    const int j = pidx - i * (i + 1) / 2;
    const int ni = shells[4 * i + 2], nj = shells[4 * j + 2];
    if (k >= ni * nj) return;
    const int ka = k / nj, kb = k - ka * nj;
    const double a = exps[shells[4 * i + 3] + ka], b = exps[shells[4 * j + 3] + kb];
    const double ca = coefs[shells[4 * i + 3] + ka], cb = coefs[shells[4 * j + 3] + kb];
    const double* A = xyz + 3 * shells[4 * i];
    const double* B = xyz + 3 * shells[4 * j];
    const double p = a + b, mu = a * b / p;
    const double qx = A[0] - B[0], qy = A[1] - B[1], qz = A[2] - B[2];
    double* o = pairs + ((size_t)g * npair + pidx) * kp * GTO_PW + (size_t)k * GTO_PW;
    d2* o2 = reinterpret_cast<d2*>(o);
    d2 v;
    v.x = p; v.y = (a * A[0] + b * B[0]) / p; o2[0] = v;
    v.x = (a * A[1] + b * B[1]) / p; v.y = (a * A[2] + b * B[2]) / p; o2[1] = v;
    v.x = ca * cb * exp(-mu * (qx * qx + qy * qy + qz * qz)); v.y = 0.5 / p; o2[2] = v;
    v.x = a / p; v.y = b / p; o2[3] = v;
}

#ifndef GTO_BODIES_ONLY
__global__ __launch_bounds__(256) void gto_pair_kernel(const int* __restrict__ shells, int nshell,
                                                       const double* __restrict__ exps,
                                                       const double* __restrict__ coefs,
                                                       const double* __restrict__ charges, int natm,
                                                       const double* __restrict__ coords, int batch, int kp,
                                                       double* __restrict__ pairs, double* __restrict__ nuc)
{
    gto_pair_body((long)blockIdx.x * blockDim.x + threadIdx.x, shells, nshell, exps, coefs, charges, natm, coords,
                  batch, kp, pairs, nuc);
}
#endif

// ---- one-electron integrals ---------------------------------------------------------------------------------------
// (the bodies of the integral kernels are __host__ __device__ functions of the thread index: a CPU build of this file
// -- GTO_BODIES_ONLY: no kernel, no entry point; tools/gto_host.hip -- runs them in a loop, under a host debugger or
// sanitizer if need be)
template <int LA, int LB, int SPLIT>
__host__ __device__ __forceinline__ void gto_one_body(long tid, const int* __restrict__ iw,
                                                      const int* __restrict__ shells, int nshell, int count,
                                                      const double* __restrict__ charges, int natm,
                                                      const double* __restrict__ coords, int batch,
                                                      const double* __restrict__ pairs, int kp, int nao,
                                                      double* __restrict__ overlap, double* __restrict__ h_ao)
{
    constexpr int NA = gto_ncomp(LA), NB = gto_ncomp(LB), L = LA + LB;
    const int sub = (int)(tid % SPLIT);
    tid /= SPLIT;
    if (tid >= (long)count * batch) return;
    const int g = (int)(tid / count), k = (int)(tid - (long)g * count);
    const long npair = (long)nshell * (nshell + 1) / 2;
    const double* xyz = coords + (size_t)g * natm * 3;
    const gto_pair_ref_t ab = gto_pair_ref(iw + nshell, gto_cls(LA, LB), k, npair, iw, shells, xyz,
                                           pairs + (size_t)g * npair * kp * GTO_PW, kp);
    double accS[NA * NB], accT[NA * NB], accV[NA * NB];
#pragma unroll
    for (int c = 0; c < NA * NB; ++c) { accS[c] = 0.0; accT[c] = 0.0; accV[c] = 0.0; }
    for (int kab = sub; kab < ab.nprim; kab += SPLIT) {
        const gto_prim_t pr = gto_load_prim(ab.data + (size_t)kab * GTO_PW, ab.swapped);
        double E[3][LA + 1][LB + 3][LA + LB + 3];
#pragma unroll
        for (int d = 0; d < 3; ++d) gto_herm<LA, LB + 2>(E[d], -pr.fb * ab.AB[d], pr.fa * ab.AB[d], pr.oo2p);
        const double b = pr.fb * pr.p;
        const double pop = GTO_PI / pr.p;
        const double fS = pr.cck * pop * sqrt(pop);
        static_for<NA>([&](auto cac) {
            static_for<NB>([&](auto cbc) {
                constexpr int ca = decltype(cac)::value, cb = decltype(cbc)::value;
                double s1[3], t1[3];
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const int i = gto_pow(LA, ca, d), j = gto_pow(LB, cb, d);
                    s1[d] = E[d][i][j][0];
                    double td = -2.0 * b * b * E[d][i][j + 2][0] + b * (double)(2 * j + 1) * s1[d];
                    if (j >= 2) td -= 0.5 * (double)(j * (j - 1)) * E[d][i][j >= 2 ? j - 2 : 0][0];
                    t1[d] = td;
                }
                accS[ca * NB + cb] += fS * (s1[0] * s1[1] * s1[2]);
                accT[ca * NB + cb] += fS * (t1[0] * s1[1] * s1[2] + s1[0] * t1[1] * s1[2] + s1[0] * s1[1] * t1[2]);
            });
        });
        if (h_ao) {
            const double fV = -2.0 * GTO_PI / pr.p * pr.cck;
            for (int c = 0; c < natm; ++c) {
                const double X = pr.P[0] - xyz[3 * c], Y = pr.P[1] - xyz[3 * c + 1], Z = pr.P[2] - xyz[3 * c + 2];
                double F[L + 1], Fs[L + 1], R[L + 1][L + 1][L + 1];
                gto_boys<L>(pr.p * (X * X + Y * Y + Z * Z), F);
                double sc = fV * charges[c];
#pragma unroll
                for (int n = 0; n <= L; ++n) { Fs[n] = sc * F[n]; sc *= -2.0 * pr.p; }
                gto_R_fill<L>(R, Fs, X, Y, Z);
                static_for<NA>([&](auto cac) {
                    static_for<NB>([&](auto cbc) {
                        constexpr int ca = decltype(cac)::value, cb = decltype(cbc)::value;
                        constexpr int ix = gto_pow(LA, ca, 0), jx = gto_pow(LB, cb, 0), iy = gto_pow(LA, ca, 1),
                                      jy = gto_pow(LB, cb, 1), iz = gto_pow(LA, ca, 2), jz = gto_pow(LB, cb, 2);
                        double v = 0.0;
#pragma unroll
                        for (int t = 0; t <= ix + jx; ++t)
#pragma unroll
                            for (int u = 0; u <= iy + jy; ++u)
#pragma unroll
                                for (int w = 0; w <= iz + jz; ++w)
                                    v += E[0][ix][jx][t] * E[1][iy][jy][u] * E[2][iz][jz][w] * R[t][u][w];
                        accV[ca * NB + cb] += v;
                    });
                });
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NA * NB; ++c) {
        accS[c] = gto_group_sum<SPLIT>(accS[c]);
        accT[c] = gto_group_sum<SPLIT>(accT[c]);
        accV[c] = gto_group_sum<SPLIT>(accV[c]);
    }
    const bool same = ab.sa == ab.sb;
    static_for<NA>([&](auto cac) {
        static_for<NB>([&](auto cbc) {
            constexpr int ca = decltype(cac)::value, cb = decltype(cbc)::value;
            const int mu = ab.oa + ca, nu = ab.ob + cb;
            if ((ca * NB + cb) % SPLIT == sub && (!same || mu >= nu) && mu < nao && nu < nao) {
                if (overlap) {
                    const double s = accS[ca * NB + cb];
                    overlap[((size_t)g * nao + mu) * nao + nu] = s;
                    overlap[((size_t)g * nao + nu) * nao + mu] = s;
                }
                if (h_ao) {
                    const double h = accT[ca * NB + cb] + accV[ca * NB + cb];
                    h_ao[((size_t)g * nao + mu) * nao + nu] = h;
                    h_ao[((size_t)g * nao + nu) * nao + mu] = h;
                }
            }
        });
    });
}

#ifndef GTO_BODIES_ONLY
template <int LA, int LB>
__global__ __launch_bounds__(GTO_NT) void gto_one_kernel(const int* __restrict__ iw, const int* __restrict__ shells,
                                                         int nshell, int count, const double* __restrict__ charges,
                                                         int natm, const double* __restrict__ coords, int batch,
                                                         const double* __restrict__ pairs, int kp, int nao,
                                                         double* __restrict__ overlap, double* __restrict__ h_ao)
{
    gto_one_body<LA, LB, GTO_SPLIT>((long)blockIdx.x * GTO_NT + threadIdx.x, iw, shells, nshell, count, charges, natm, coords,
                         batch, pairs, kp, nao, overlap, h_ao);
}
#endif

// ---- two-electron integrals ---------------------------------------------------------------------------------------
template <int LA, int LB, int LC, int LD, int SPLIT>
__host__ __device__ __forceinline__ void gto_eri_body(long tid, const int* __restrict__ iw,
                                                      const int* __restrict__ shells, int nshell, int nbra, int nket,
                                                      long nquart, const double* __restrict__ coords, int natm,
                                                      int batch, const double* __restrict__ pairs, int kp, int nao,
                                                      double* __restrict__ g_ao)
{
    constexpr int NA = gto_ncomp(LA), NB = gto_ncomp(LB), NC = gto_ncomp(LC), ND = gto_ncomp(LD);
    constexpr int L = LA + LB + LC + LD;
    constexpr bool same_cls = (LA == LC && LB == LD);
    const int sub = (int)(tid % SPLIT);
    tid /= SPLIT;
    if (tid >= nquart * batch) return;
    const int g = (int)(tid / nquart);
    const long r = tid - (long)g * nquart;
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

    double acc[NA * NB * NC * ND];
#pragma unroll
    for (int c = 0; c < NA * NB * NC * ND; ++c) acc[c] = 0.0;
    for (int kab = sub; kab < ab.nprim; kab += SPLIT) {
        const gto_prim_t pb = gto_load_prim(ab.data + (size_t)kab * GTO_PW, ab.swapped);
        double Eb[3][LA + 1][LB + 1][LA + LB + 1];
#pragma unroll
        for (int d = 0; d < 3; ++d) gto_herm<LA, LB>(Eb[d], -pb.fb * ab.AB[d], pb.fa * ab.AB[d], pb.oo2p);
        for (int kcd = 0; kcd < cd.nprim; ++kcd) {
            const gto_prim_t pk = gto_load_prim(cd.data + (size_t)kcd * GTO_PW, cd.swapped);
            double Ek[3][LC + 1][LD + 1][LC + LD + 1];
#pragma unroll
            for (int d = 0; d < 3; ++d) gto_herm<LC, LD>(Ek[d], -pk.fb * cd.AB[d], pk.fa * cd.AB[d], pk.oo2p);
            const double s = pb.p + pk.p, alpha = pb.p * pk.p / s;
            const double X = pb.P[0] - pk.P[0], Y = pb.P[1] - pk.P[1], Z = pb.P[2] - pk.P[2];
            double F[L + 1], Fs[L + 1], R[L + 1][L + 1][L + 1];
            gto_boys<L>(alpha * (X * X + Y * Y + Z * Z), F);
            // 2 pi^(5/2) / (p q sqrt(p + q)) and the two pair factors
            double sc = 34.98683665524972497 / (pb.p * pk.p * sqrt(s)) * (pb.cck * pk.cck);
#pragma unroll
            for (int n = 0; n <= L; ++n) { Fs[n] = sc * F[n]; sc *= -2.0 * alpha; }
            gto_R_fill<L>(R, Fs, X, Y, Z);
            // ket side first: X_tuv = sum_t'u'v' (-1)^(t'+u'+v') E^cd_t'u'v' R_(t+t', u+u', v+v') of one ket component,
            // then every bra component takes its few E^ab_tuv X_tuv
            static_for<NC * ND>([&](auto ccdc) {
                constexpr int ccd = decltype(ccdc)::value, cc = ccd / ND, cd_ = ccd % ND;
                constexpr int kx = gto_pow(LC, cc, 0), lx = gto_pow(LD, cd_, 0), ky = gto_pow(LC, cc, 1),
                              ly = gto_pow(LD, cd_, 1), kz = gto_pow(LC, cc, 2), lz = gto_pow(LD, cd_, 2);
                constexpr int LAB = LA + LB;
                double Xh[LAB + 1][LAB + 1][LAB + 1];
                static_for<(LAB + 1) * (LAB + 1) * (LAB + 1)>([&](auto tuvc) {
                    constexpr int tuv = decltype(tuvc)::value, t = tuv / ((LAB + 1) * (LAB + 1)),
                                  u = (tuv / (LAB + 1)) % (LAB + 1), w = tuv % (LAB + 1);
                    if constexpr (t + u + w <= LAB) {
                        double x = 0.0;
#pragma unroll
                        for (int t2 = 0; t2 <= kx + lx; ++t2)
#pragma unroll
                            for (int u2 = 0; u2 <= ky + ly; ++u2)
#pragma unroll
                                for (int w2 = 0; w2 <= kz + lz; ++w2) {
                                    const double ek = Ek[0][kx][lx][t2] * Ek[1][ky][ly][u2] * Ek[2][kz][lz][w2];
                                    const double sg = ((t2 + u2 + w2) & 1) ? -1.0 : 1.0;
                                    x += sg * ek * R[t + t2][u + u2][w + w2];
                                }
                        Xh[t][u][w] = x;
                    }
                });
                static_for<NA * NB>([&](auto cabc) {
                    constexpr int cab = decltype(cabc)::value, ca = cab / NB, cb = cab % NB;
                    constexpr int ix = gto_pow(LA, ca, 0), jx = gto_pow(LB, cb, 0), iy = gto_pow(LA, ca, 1),
                                  jy = gto_pow(LB, cb, 1), iz = gto_pow(LA, ca, 2), jz = gto_pow(LB, cb, 2);
                    double v = 0.0;
#pragma unroll
                    for (int t = 0; t <= ix + jx; ++t)
#pragma unroll
                        for (int u = 0; u <= iy + jy; ++u)
#pragma unroll
                            for (int w = 0; w <= iz + jz; ++w)
                                v += Eb[0][ix][jx][t] * Eb[1][iy][jy][u] * Eb[2][iz][jz][w] * Xh[t][u][w];
                    acc[cab * (NC * ND) + ccd] += v;
                });
            });
        }
    }
#pragma unroll
    for (int c = 0; c < NA * NB * NC * ND; ++c) acc[c] = gto_group_sum<SPLIT>(acc[c]);
    // (after the butterfly every lane of the group holds every value: lane `sub` stores every SPLIT-th component)
    // every unique value to its (up to 8) places, from one register; a value two components of this thread both
    // stand for (same shell twice in a pair, same pair twice in the quartet) is stored by one of them only
    const bool same_ab = ab.sa == ab.sb, same_cd = cd.sa == cd.sb;
    const bool same_pair = same_cls && ab.sa == cd.sa && ab.sb == cd.sb;
    double* out = g_ao + (size_t)g * nao * nao * nao * nao;
    const size_t n1 = (size_t)nao, n2 = n1 * n1, n3 = n2 * n1;
    static_for<NA * NB>([&](auto cabc) {
        constexpr int cab = decltype(cabc)::value, ca = cab / NB, cb = cab % NB;
        static_for<NC * ND>([&](auto ccdc) {
            constexpr int ccd = decltype(ccdc)::value, cc = ccd / ND, cd_ = ccd % ND;
            const size_t mu = ab.oa + ca, nu = ab.ob + cb, la = cd.oa + cc, si = cd.ob + cd_;
            const size_t m1 = mu > nu ? mu : nu, m0 = mu > nu ? nu : mu, l1 = la > si ? la : si,
                         l0 = la > si ? si : la;
            bool keep = m1 < n1 && l1 < n1 && (cab * (NC * ND) + ccd) % SPLIT == sub;
            if (same_ab && mu < nu) keep = false;
            if (same_cd && la < si) keep = false;
            if (same_pair && m1 * (m1 + 1) / 2 + m0 < l1 * (l1 + 1) / 2 + l0) keep = false;
            if (keep) {
                const double x = acc[cab * (NC * ND) + ccd];
                out[mu * n3 + nu * n2 + la * n1 + si] = x;
                out[nu * n3 + mu * n2 + la * n1 + si] = x;
                out[mu * n3 + nu * n2 + si * n1 + la] = x;
                out[nu * n3 + mu * n2 + si * n1 + la] = x;
                out[la * n3 + si * n2 + mu * n1 + nu] = x;
                out[si * n3 + la * n2 + mu * n1 + nu] = x;
                out[la * n3 + si * n2 + nu * n1 + mu] = x;
                out[si * n3 + la * n2 + nu * n1 + mu] = x;
            }
        });
    });
}

#ifndef GTO_BODIES_ONLY
template <int LA, int LB, int LC, int LD>
__global__ __launch_bounds__(GTO_NT) void gto_eri_kernel(const int* __restrict__ iw, const int* __restrict__ shells,
                                                         int nshell, int nbra, int nket, long nquart,
                                                         const double* __restrict__ coords, int natm, int batch,
                                                         const double* __restrict__ pairs, int kp, int nao,
                                                         double* __restrict__ g_ao)
{
    gto_eri_body<LA, LB, LC, LD, GTO_SPLIT>((long)blockIdx.x * GTO_NT + threadIdx.x, iw, shells, nshell, nbra, nket, nquart,
                                 coords, natm, batch, pairs, kp, nao, g_ao);
}
#endif

#ifndef GTO_BODIES_ONLY
// ---- Boys function on its own (the accuracy test) ----------------------------------------------------------------
template <int L>
__global__ void gto_boys_kernel(const double* __restrict__ T, long count, double* __restrict__ F)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    double f[L + 1];
    gto_boys<L>(T[i], f);
#pragma unroll
    for (int n = 0; n <= L; ++n) F[i * (L + 1) + n] = f[n];
}

// ---- S^-1/2 -------------------------------------------------------------------------------------------------------
// One wave per matrix: cyclic Jacobi on A in the parallel (round-robin) ordering -- the rotations of the n / 2 disjoint
// pairs of a round are computed by n / 2 lanes at once and applied in two passes; with one rotation at a time (the
// order of ci_jacobi) the chain of divisions and square roots of 78 rotations per sweep took 0.27 ms at n = 13 --
// then X = U diag(w^-1/2) U^T, each element of the lower triangle once, stored to both places.
// LDS: A and U, leading dimension n | 1, and the (cos, sin) and index pairs of a round.  The iteration itself is
// sym_jacobi_wave (jacobi.h), shared with the eigensolver of the SCF kernels.
__global__ __launch_bounds__(INVSQRT_NT) void sym_invsqrt_kernel(const double* __restrict__ S, int n, double min_eig,
                                                                 double* __restrict__ Xout, int* __restrict__ info)
{
    extern __shared__ double lds[];
    const int ld = n | 1;
    double* A = lds;
    double* U = lds + (size_t)n * ld;
    double* cs = U + (size_t)n * ld;                // (cos, sin) of the rotations of a round
    int* pq = reinterpret_cast<int*>(cs + INVSQRT_NT);   // and their index pairs
    const int lane = threadIdx.x, g = blockIdx.x;
    const double* Sg = S + (size_t)g * n * n;
    double* Xg = Xout + (size_t)g * n * n;
    for (int k = lane; k < n * n; k += INVSQRT_NT) {
        const int r = k / n, c = k - r * n;
        // (the upper triangle is taken from the lower one: the iteration works on an exactly symmetric matrix)
        A[r * ld + c] = (r >= c) ? Sg[r * n + c] : Sg[c * n + r];
        U[r * ld + c] = (r == c) ? 1.0 : 0.0;
    }
    sym_jacobi_wave(A, U, cs, pq, n, ld, lane);
    double w = INFINITY;
    bool bad = false;
    if (lane < n) { w = A[lane * ld + lane]; bad = !(w >= min_eig); }     // (NaN is bad)
    const bool any_bad = __any(bad);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    if (lane < n) A[lane * ld + lane] = any_bad ? 0.0 : 1.0 / sqrt(w);     // the diagonal now holds w^-1/2
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    if (lane == 0) info[g] = any_bad ? -1 : 0;
    if (lane < n) {
        for (int c = 0; c <= lane; ++c) {
            double x = 0.0;
            for (int k = 0; k < n; ++k) x += U[lane * ld + k] * A[k * ld + k] * U[c * ld + k];
            if (any_bad) x = __builtin_nan("");
            Xg[lane * n + c] = x;
            Xg[c * n + lane] = x;
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------
extern "C" int64_t oovqe_gto_work_size(int nshell, int max_nprim, int batch)
{
    if (gto_check_sizes("oovqe_gto_work_size", nshell, max_nprim, batch) != 0) return OOVQE_ERR_ARG;
    return gto_work_base(nshell, max_nprim, batch);
}

namespace {
template <int LA, int LB> int gto_launch_one(gto_cls_t<LA, LB>, const gto_prep_t& p, double* overlap, double* h_ao)
{
    const int count = p.cnt[gto_cls(LA, LB)];
    if (count == 0) return 0;
    unsigned grid;
    if (const int rc = gto_grid_split(p.who, (long)count * p.batch, &grid)) return rc;
    hipLaunchKernelGGL((gto_one_kernel<LA, LB>), dim3(grid), dim3(GTO_NT), 0, p.st, p.iw, p.shells, p.nshell, count,
                       p.charges, p.natm, p.coords, p.batch, p.pairs, p.kp, p.nao, overlap, h_ao);
    OOVQE_CHECK_LAUNCH("gto_one_kernel");
    return 0;
}

template <int LA, int LB, int LC, int LD>
int gto_launch_eri(gto_cls_t<LA, LB, LC, LD>, const gto_prep_t& p, double* g_ao)
{
    const int nbra = p.cnt[gto_cls(LA, LB)], nket = p.cnt[gto_cls(LC, LD)];
    const long nq = gto_quartets(LA == LC && LB == LD, nbra, nket);
    if (nq == 0) return 0;
    unsigned grid;
    if (const int rc = gto_grid_split(p.who, nq * p.batch, &grid)) return rc;
    hipLaunchKernelGGL((gto_eri_kernel<LA, LB, LC, LD>), dim3(grid), dim3(GTO_NT), 0, p.st, p.iw, p.shells, p.nshell,
                       nbra, nket, nq, p.coords, p.natm, p.batch, p.pairs, p.kp, p.nao, g_ao);
    OOVQE_CHECK_LAUNCH("gto_eri_kernel");
    return 0;
}
}  // namespace

int gto_read_shells(const char* who, int max_l, int nshell, const int32_t* shells, int nprim_total, int natm, int nao,
                    hipStream_t st, std::vector<int32_t>* table)
{
    // the shell table is read back once per call (16 bytes per shell): the limits below are enforced here, with a
    // return code, and the launches are sized from it
    std::vector<int32_t>& tab = *table;
    tab.resize((size_t)nshell * 4);
    OOVQE_CHECK_HIP(hipMemcpyAsync(tab.data(), shells, tab.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st), who);
    OOVQE_CHECK_HIP(hipStreamSynchronize(st), who);
    int ao = 0;
    for (int s = 0; s < nshell; ++s) {
        const int atom = tab[4 * s], field = tab[4 * s + 1], np = tab[4 * s + 2], off = tab[4 * s + 3];
        const int l = gto_l_of(field);
        OOVQE_REQUIRE(field >= 0 && l <= OOVQE_GTO_MAX_L && (field == l || (l == 2 && field == (2 | OOVQE_GTO_CARTESIAN))),
                      "%s: shell %d has the l field %d (l <= %d; OOVQE_GTO_CARTESIAN on a d shell only)", who, s, field,
                      OOVQE_GTO_MAX_L);
        OOVQE_REQUIRE(l <= max_l, "%s: shell %d has l = %d: this entry serves s and p shells only (l <= %d)", who, s, l,
                      max_l);
        OOVQE_REQUIRE(np >= 1 && np <= OOVQE_GTO_MAX_PRIM, "%s: shell %d has %d primitives (1 .. %d)", who, s, np,
                      OOVQE_GTO_MAX_PRIM);
        OOVQE_REQUIRE(atom >= 0 && atom < natm, "%s: shell %d sits on atom %d of %d", who, s, atom, natm);
        OOVQE_REQUIRE(off >= 0 && off + np <= nprim_total, "%s: shell %d reads primitives %d .. %d of %d", who, s,
                      off, off + np - 1, nprim_total);
        ao += gto_nfunc(field);
    }
    OOVQE_REQUIRE(ao == nao, "%s: the shell table has %d functions, nao = %d", who, ao, nao);
    return 0;
}

// What every entry point that consumes pair data does first: the shell table is checked against the limits, the pair
// classes counted, ao_off / class lists (gto_setup_kernel) and the pair data of every geometry (gto_pair_kernel; nuc
// may be null) written into `work`.  batch = 0 leaves p->batch = 0 and launches nothing.
int gto_prepare(const char* who, int max_l, int nshell, const int32_t* shells, int nprim_total, const double* exps,
                const double* coefs, int natm, const double* charges, int batch, const double* coords, int nao,
                double* nuc, double* work, hipStream_t st, gto_prep_t* p)
{
    OOVQE_REQUIRE(nshell >= 1 && nshell <= OOVQE_GTO_MAX_SHELL, "%s: nshell = %d (1 .. %d)", who, nshell,
                  OOVQE_GTO_MAX_SHELL);
    OOVQE_REQUIRE(batch >= 0 && natm >= 1 && nprim_total >= 1, "%s: batch = %d, natm = %d, nprim_total = %d", who,
                  batch, natm, nprim_total);
    p->batch = batch;
    if (batch == 0) return 0;
    OOVQE_REQUIRE(shells && exps && coefs && charges && coords && work, "%s: null pointer", who);
    std::vector<int32_t> tab;
    const int rc = gto_read_shells(who, max_l, nshell, shells, nprim_total, natm, nao, st, &tab);
    if (rc != 0) return rc;
    int* cnt = p->cnt;
    for (int c = 0; c < GTO_NCLS; ++c) cnt[c] = 0;
    int kp = 0;
    for (int i = 0; i < nshell; ++i) {
        kp = tab[4 * i + 2] > kp ? tab[4 * i + 2] : kp;
        for (int j = 0; j <= i; ++j) {
            const int li = gto_l_of(tab[4 * i + 1]), lj = gto_l_of(tab[4 * j + 1]);
            cnt[gto_cls(li >= lj ? li : lj, li >= lj ? lj : li)] += 1;
        }
    }
    kp *= kp;
    const long npair = (long)nshell * (nshell + 1) / 2;
    // the layout of the work buffer: int part | pair data of the stack | the entry's own records
    int* iw = p->iw = reinterpret_cast<int*>(work);
    double* pairs = p->pairs = work + gto_int_doubles(nshell);
    p->rec = pairs + (size_t)batch * npair * kp * GTO_PW;
    p->kp = kp;
    p->who = who; p->shells = shells; p->nshell = nshell; p->charges = charges; p->natm = natm; p->coords = coords;
    p->nao = nao; p->st = st;
    hipLaunchKernelGGL(gto_setup_kernel, dim3(1), dim3(64), 0, st, shells, nshell, iw);
    OOVQE_CHECK_LAUNCH("gto_setup_kernel");
    const long pt = npair * kp * batch;
    OOVQE_REQUIRE((pt + 255) / 256 < (1L << 31), "%s: %ld primitive pairs", who, pt);
    hipLaunchKernelGGL(gto_pair_kernel, dim3((unsigned)((pt + 255) / 256)), dim3(256), 0, st, shells, nshell, exps,
                       coefs, charges, natm, coords, batch, kp, pairs, nuc);
    OOVQE_CHECK_LAUNCH("gto_pair_kernel");
    return 0;
}

extern "C" int oovqe_gto_integrals_batch(int nshell, const int32_t* shells, int nprim_total, const double* exps,
                                         const double* coefs, int natm, const double* charges, int batch,
                                         const double* coords, int nao, double* overlap, double* h_ao, double* g_ao,
                                         double* nuc, double* work, oovqe_stream_t stream)
{
    hipStream_t st = (hipStream_t)stream;
    gto_prep_t p;
    int rc = gto_prepare("oovqe_gto_integrals_batch", OOVQE_GTO_MAX_L, nshell, shells, nprim_total, exps, coefs, natm, charges, batch,
                         coords, nao, nuc, work, st, &p);
    if (rc != 0 || batch == 0) return rc;
    if (overlap || h_ao) {
        if ((rc = gto_d_launch_one_electron(p, overlap, h_ao)) != 0) return rc;
        if ((rc = gto_sp_pairs([&](auto c) { return gto_launch_one(c, p, overlap, h_ao); })) != 0) return rc;
    }
    if (g_ao) {
        // bra class >= ket class; the most numerous (and cheapest) classes last, behind the classes with a d shell
        // (gto_d.hip) and the long threads of (pp|pp)
        if ((rc = gto_d_launch_two_electron(p, g_ao)) != 0) return rc;
        if ((rc = gto_sp_quartets([&](auto c) { return gto_launch_eri(c, p, g_ao); })) != 0) return rc;
    }
    return 0;
}

extern "C" int oovqe_sym_invsqrt_batch(const double* s, int n, int batch, double* x, int* info,
                                       oovqe_stream_t stream)
{
    const char* who = "oovqe_sym_invsqrt_batch";
    OOVQE_REQUIRE(n >= 1 && n <= OOVQE_INVSQRT_MAX_N, "%s: n = %d (1 .. %d)", who, n, OOVQE_INVSQRT_MAX_N);
    OOVQE_REQUIRE(batch >= 0, "%s: batch = %d", who, batch);
    if (batch == 0) return 0;
    OOVQE_REQUIRE(s && x && info, "%s: null pointer", who);
    const size_t lds = (2 * (size_t)n * (n | 1) + 2 * INVSQRT_NT) * sizeof(double);
    if (oovqe_ensure_dynamic_lds(reinterpret_cast<const void*>(&sym_invsqrt_kernel), lds) != 0) return OOVQE_ERR_HIP;
    hipLaunchKernelGGL(sym_invsqrt_kernel, dim3(batch), dim3(INVSQRT_NT), lds, (hipStream_t)stream, s, n,
                       (double)OOVQE_INVSQRT_MIN_EIG, x, info);
    OOVQE_CHECK_LAUNCH("sym_invsqrt_kernel");
    return 0;
}

extern "C" int oovqe_boys(int nmax, const double* t, int64_t count, double* f, oovqe_stream_t stream)
{
    OOVQE_REQUIRE(nmax >= 0 && nmax <= 4 * OOVQE_GTO_MAX_L, "oovqe_boys: nmax = %d (0 .. %d)", nmax,
                  4 * OOVQE_GTO_MAX_L);
    OOVQE_REQUIRE(count >= 0, "oovqe_boys: count = %lld", (long long)count);
    if (count == 0) return 0;
    OOVQE_REQUIRE(t && f, "oovqe_boys: null pointer");
    const dim3 grid((unsigned)((count + 255) / 256)), block(256);
    hipStream_t st = (hipStream_t)stream;
    switch (nmax) {
    case 0: hipLaunchKernelGGL(gto_boys_kernel<0>, grid, block, 0, st, t, (long)count, f); break;
    case 1: hipLaunchKernelGGL(gto_boys_kernel<1>, grid, block, 0, st, t, (long)count, f); break;
    case 2: hipLaunchKernelGGL(gto_boys_kernel<2>, grid, block, 0, st, t, (long)count, f); break;
    case 3: hipLaunchKernelGGL(gto_boys_kernel<3>, grid, block, 0, st, t, (long)count, f); break;
    case 4: hipLaunchKernelGGL(gto_boys_kernel<4>, grid, block, 0, st, t, (long)count, f); break;
    case 5: hipLaunchKernelGGL(gto_boys_kernel<5>, grid, block, 0, st, t, (long)count, f); break;
    case 6: hipLaunchKernelGGL(gto_boys_kernel<6>, grid, block, 0, st, t, (long)count, f); break;
    case 7: hipLaunchKernelGGL(gto_boys_kernel<7>, grid, block, 0, st, t, (long)count, f); break;
    default: hipLaunchKernelGGL(gto_boys_kernel<8>, grid, block, 0, st, t, (long)count, f); break;
    }
    OOVQE_CHECK_LAUNCH("gto_boys_kernel");
    return 0;
}
#endif  // GTO_BODIES_ONLY
