// Nuclear gradients of a stack of geometries (gfx950): the derivatives of the AO integrals of gto.hip with respect to
// the nuclear coordinates, contracted on the fly with densities -- no derivative integral is ever stored.
//
//   grad[g, A, :] = sum_pq D1[g,p,q] dh[p,q]/dR_A + sum_pq WQ[g,p,q] dS[p,q]/dR_A
//                 + 1/2 sum_pqrs D2[g,p,q,r,s] d(pq|rs)/dR_A + dE_nuc/dR_A
//
//   gto_grad_one_kernel  <la, lb>: one shell pair per group of GTO_SPLIT lanes: D1 . d(T + V) and WQ . dS
//   gto_grad_eri_kernel  <la, lb, lc, ld, swap>: one unique shell quartet per group of GTO_SPLIT lanes (the enumeration
//                        and the lane groups of gto_eri_kernel), ONE side of it differentiated per launch; the quartet's
//                        block of D2 (at most 81 values, weighted with the degeneracy of the quartet) is loaded once
//                        into LDS and contracted inside the primitive loop
//   gto_grad_reduce_kernel  one workgroup per (atom, geometry): the records of the geometry summed in a fixed order,
//                        the derivative of the nuclear repulsion added
//   cas_ao_densities_kernel  D1 and the 8-fold symmetric D2 of a CAS wave function from orbitals and active RDMs
//
// The derivative of a Cartesian Gaussian with respect to its centre is 2a times the function one l higher minus l times
// the function one l lower, so the Hermite coefficients are made one order higher on the differentiated centre
// (gto_herm<L + 1, .>), the Boys function and R_tuv one order higher (t + u + v <= 5 for (pp|pp)).  Per pair or quartet
// only SCALARS per centre are accumulated: 3 numbers for the first centre of a pair (derivative coefficients) and 3 for
// the sum of both centres (d/dP: R_tuv -> R_t+1,uv, the coefficients depend on A - B only); the second centre is the
// difference.  The last centre follows from translational invariance: for a pair and a nucleus it is minus d/dP, for a
// quartet d/dQ = -d/dP is what the launch of the other side accumulates (in its own order of summation).  One-centre
// pairs and quartets contribute exactly zero and are skipped.
//
// No floating-point atomics: every pair / quartet writes one record of GRAD_REC doubles (4 centres x 3 components and
// the 4 atom indices, -1 = nothing) at a place that depends on the geometry and the quartet only, and the reduction
// adds the records of a geometry in a fixed order: a geometry's gradient has the same bits whatever stack it is in.
#include "gto_grad.h"

// ---- one-electron terms ---------------------------------------------------------------------------------------------
// records of pair k of the class: [natm + 1]: c < natm the attraction of nucleus c (centres A, B, c), natm: S and T
template <int LA, int LB>
__global__ __launch_bounds__(GTO_NT) void gto_grad_one_kernel(const int* __restrict__ iw, const int* __restrict__ shells,
                                                              int nshell, int count, const double* __restrict__ charges,
                                                              int natm, const double* __restrict__ coords, int batch,
                                                              const double* __restrict__ pairs, int kp, int nao,
                                                              const double* __restrict__ d1, const double* __restrict__ wq,
                                                              double* __restrict__ rec, long rec_off, long nrec)
{
    constexpr int NA = gto_ncomp(LA), NB = gto_ncomp(LB), L = LA + LB;
    long tid = (long)blockIdx.x * GTO_NT + threadIdx.x;
    const int sub = (int)(tid % GTO_SPLIT);
    tid /= GTO_SPLIT;
    if (tid >= (long)count * batch) return;
    const int g = (int)(tid / count), k = (int)(tid - (long)g * count);
    const long npair = (long)nshell * (nshell + 1) / 2;
    const double* xyz = coords + (size_t)g * natm * 3;
    const gto_pair_ref_t ab = gto_pair_ref(iw + nshell, gto_cls(LA, LB), k, npair, iw, shells, xyz,
                                           pairs + (size_t)g * npair * kp * GTO_PW, kp);
    const int atA = shells[4 * ab.sa], atB = shells[4 * ab.sb];
    double* out = rec + ((size_t)g * nrec + rec_off + (size_t)k * (natm + 1)) * GRAD_REC;
    const double deg = (ab.sa == ab.sb) ? 1.0 : 2.0;
    double w1[NA * NB], ws[NA * NB];
#pragma unroll
    for (int c = 0; c < NA * NB; ++c) {
        const size_t idx = ((size_t)g * nao + (ab.oa + c / NB)) * nao + (ab.ob + c % NB);
        w1[c] = d1 ? deg * d1[idx] : 0.0;
        ws[c] = wq ? deg * wq[idx] : 0.0;
    }
    // overlap and kinetic energy: two centres, B = -A
    {
        double gA[3] = {0.0, 0.0, 0.0};
        if (atA != atB) {
            for (int kab = sub; kab < ab.nprim; kab += GTO_SPLIT) {
                const gto_prim_t pr = gto_load_prim(ab.data + (size_t)kab * GTO_PW, ab.swapped);
                double E[3][LA + 2][LB + 3][LA + LB + 4];
#pragma unroll
                for (int d = 0; d < 3; ++d) gto_herm<LA + 1, LB + 2>(E[d], -pr.fb * ab.AB[d], pr.fa * ab.AB[d], pr.oo2p);
                const double a = pr.fa * pr.p, b = pr.fb * pr.p;
                const double pop = GTO_PI / pr.p;
                const double fS = pr.cck * pop * sqrt(pop);
                static_for<NA * NB>([&](auto cc) {
                    constexpr int c = decltype(cc)::value, ca = c / NB, cb = c % NB;
                    double s1[3], t1[3], ds[3], dt[3];
                    static_for<3>([&](auto dc) {
                        constexpr int d = decltype(dc)::value;
                        constexpr int i = gto_pow(LA, ca, d), j = gto_pow(LB, cb, d);
                        s1[d] = gto_ovl1<i, j>(E[d]);
                        t1[d] = gto_kin1<i, j>(E[d], b);
                        ds[d] = 2.0 * a * gto_ovl1<i + 1, j>(E[d]) - (double)i * gto_ovl1<i - 1, j>(E[d]);
                        dt[d] = 2.0 * a * gto_kin1<i + 1, j>(E[d], b) - (double)i * gto_kin1<i - 1, j>(E[d], b);
                    });
                    static_for<3>([&](auto dc) {
                        constexpr int d = decltype(dc)::value, e = (d + 1) % 3, f = (d + 2) % 3;
                        const double dS = ds[d] * s1[e] * s1[f];
                        const double dT = dt[d] * s1[e] * s1[f] + ds[d] * (t1[e] * s1[f] + s1[e] * t1[f]);
                        gA[d] += fS * (ws[c] * dS + w1[c] * dT);
                    });
                });
            }
        }
        double v[12];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double x = gto_group_sum<GTO_SPLIT>(gA[d]);
            v[d] = x; v[3 + d] = -x; v[6 + d] = 0.0; v[9 + d] = 0.0;
        }
        if (sub == 0) {
            if (atA != atB) grad_store(out + (size_t)natm * GRAD_REC, atA, atB, -1, -1, v);
            else grad_store(out + (size_t)natm * GRAD_REC, -1, -1, -1, -1, v);
        }
    }
    // nuclear attraction: the basis functions on A and B and the operator on every nucleus c
    for (int c = 0; c < natm; ++c) {
        double vA[3] = {0.0, 0.0, 0.0}, vP[3] = {0.0, 0.0, 0.0};
        const bool live = d1 && !(atA == atB && atA == c);
        if (live) {
            const double zc = charges[c];
            for (int kab = sub; kab < ab.nprim; kab += GTO_SPLIT) {
                const gto_prim_t pr = gto_load_prim(ab.data + (size_t)kab * GTO_PW, ab.swapped);
                double E[3][LA + 2][LB + 1][L + 2], dE[3][LA + 1][LB + 1][L + 2];
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    gto_herm<LA + 1, LB>(E[d], -pr.fb * ab.AB[d], pr.fa * ab.AB[d], pr.oo2p);
                    gto_herm_deriv<LA, LB>(dE[d], E[d], pr.fa * pr.p);
                }
                const double X = pr.P[0] - xyz[3 * c], Y = pr.P[1] - xyz[3 * c + 1], Z = pr.P[2] - xyz[3 * c + 2];
                double F[L + 2], Fs[L + 2], R[L + 2][L + 2][L + 2];
                gto_boys<L + 1>(pr.p * (X * X + Y * Y + Z * Z), F);
                double sc = -2.0 * GTO_PI / pr.p * pr.cck * zc;
#pragma unroll
                for (int n = 0; n <= L + 1; ++n) { Fs[n] = sc * F[n]; sc *= -2.0 * pr.p; }
                gto_R_fill<L + 1>(R, Fs, X, Y, Z);
                static_for<NA * NB>([&](auto cc) {
                    constexpr int cm = decltype(cc)::value, ca = cm / NB, cb = cm % NB;
                    constexpr int ix = gto_pow(LA, ca, 0), jx = gto_pow(LB, cb, 0), iy = gto_pow(LA, ca, 1),
                                  jy = gto_pow(LB, cb, 1), iz = gto_pow(LA, ca, 2), jz = gto_pow(LB, cb, 2);
                    const double w = w1[cm];
                    vA[0] += w * gto_bra_sum<ix + jx + 1, iy + jy, iz + jz, 0, 0, 0>(dE[0][ix][jx], E[1][iy][jy], E[2][iz][jz], R);
                    vA[1] += w * gto_bra_sum<ix + jx, iy + jy + 1, iz + jz, 0, 0, 0>(E[0][ix][jx], dE[1][iy][jy], E[2][iz][jz], R);
                    vA[2] += w * gto_bra_sum<ix + jx, iy + jy, iz + jz + 1, 0, 0, 0>(E[0][ix][jx], E[1][iy][jy], dE[2][iz][jz], R);
                    vP[0] += w * gto_bra_sum<ix + jx, iy + jy, iz + jz, 1, 0, 0>(E[0][ix][jx], E[1][iy][jy], E[2][iz][jz], R);
                    vP[1] += w * gto_bra_sum<ix + jx, iy + jy, iz + jz, 0, 1, 0>(E[0][ix][jx], E[1][iy][jy], E[2][iz][jz], R);
                    vP[2] += w * gto_bra_sum<ix + jx, iy + jy, iz + jz, 0, 0, 1>(E[0][ix][jx], E[1][iy][jy], E[2][iz][jz], R);
                });
            }
        }
        double v[12];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double xa = gto_group_sum<GTO_SPLIT>(vA[d]), xp = gto_group_sum<GTO_SPLIT>(vP[d]);
            v[d] = xa; v[3 + d] = xp - xa; v[6 + d] = -xp; v[9 + d] = 0.0;
        }
        if (sub == 0) {
            if (live) grad_store(out + (size_t)c * GRAD_REC, atA, atB, c, -1, v);
            else grad_store(out + (size_t)c * GRAD_REC, -1, -1, -1, -1, v);
        }
    }
}

// ---- two-electron term ------------------------------------------------------------------------------------------------
// One launch differentiates ONE side of every quartet: (LA, LB) is the side whose two centres this instantiation
// handles (derivative coefficients on its first centre, d/dP for the sum of both), (LC, LD) the other side, folded
// into R_tuv with its plain coefficients.  SWAP = false: the differentiated side is the bra of gto_eri_kernel's
// enumeration of unique quartets, SWAP = true: its ket; the two launches of a class pair write the two records of a
// quartet.  (Both sides in one kernel -- the ket's derivative coefficients beside the bra's -- needs R_tuv, four
// coefficient tables and two folded copies at once: 512 registers and 2.6 kB of scratch per lane for (pp|pp).  Split by
// side, each launch repeats the Boys function and R_tuv of a primitive quartet and nothing spills.)
template <int LA, int LB, int LC, int LD, bool SWAP, int PART, int NPART>
__global__ __launch_bounds__(GTO_NT) void gto_grad_eri_kernel(const int* __restrict__ iw, const int* __restrict__ shells,
                                                              int nshell, int nbra, int nket, long nquart,
                                                              const double* __restrict__ coords, int natm, int batch,
                                                              const double* __restrict__ pairs, int kp, int nao,
                                                              const double* __restrict__ d2m, double* __restrict__ rec,
                                                              long rec_off, long nrec)
{
    constexpr int NA = gto_ncomp(LA), NB = gto_ncomp(LB), NC = gto_ncomp(LC), ND = gto_ncomp(LD);
    constexpr int NAB = NA * NB, NCD = NC * ND, LAB = LA + LB, LCD = LC + LD;
    constexpr int L = LAB + LCD + 1;
    constexpr bool same_cls = (LA == LC && LB == LD);
    __shared__ double Dl[GTO_NT / GTO_SPLIT][NAB * NCD];
    long tid = (long)blockIdx.x * GTO_NT + threadIdx.x;
    const int sub = (int)(tid % GTO_SPLIT), grp = (int)(threadIdx.x / GTO_SPLIT);
    tid /= GTO_SPLIT;
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
    // ab: the differentiated side, cd: the other one
    const gto_pair_ref_t ab = gto_pair_ref(iw + nshell, gto_cls(LA, LB), SWAP ? k2 : k1, npair, iw, shells, xyz, pairs_g, kp);
    const gto_pair_ref_t cd = gto_pair_ref(iw + nshell, gto_cls(LC, LD), SWAP ? k1 : k2, npair, iw, shells, xyz, pairs_g, kp);
    const int atA = shells[4 * ab.sa], atB = shells[4 * ab.sb], atC = shells[4 * cd.sa], atD = shells[4 * cd.sb];
    double* out = rec + ((size_t)g * nrec + rec_off + (2 * r + (SWAP ? 1 : 0)) * NPART + PART) * GRAD_REC;
    double v[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) v[c] = 0.0;
    if (atA == atB && atA == atC && atA == atD) {          // one centre: exactly zero
        if (sub == 0) grad_store(out, -1, -1, -1, -1, v);
        return;
    }
    {
        // E_2 = 1/2 sum D2 (pq|rs) over ALL index quadruples: a unique quartet stands for up to 8 of them
        const double deg = 0.5 * (ab.sa == ab.sb ? 1.0 : 2.0) * (cd.sa == cd.sb ? 1.0 : 2.0)
                           * ((same_cls && k1 == k2) ? 1.0 : 2.0);
        const size_t n1 = (size_t)nao;
        const double* dg = d2m + (size_t)g * n1 * n1 * n1 * n1;
        for (int c = sub; c < NAB * NCD; c += GTO_SPLIT) {
            const int cab = c / NCD, ccd = c - cab * NCD;
            const size_t mu = ab.oa + cab / NB, nu = ab.ob + cab % NB, la = cd.oa + ccd / ND, si = cd.ob + ccd % ND;
            Dl[grp][c] = deg * dg[((mu * n1 + nu) * n1 + la) * n1 + si];
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();

    // (read as volatile: the 81 weights are loop invariant, and hoisted out of the primitive loops they would take the
    // 162 registers the LDS copy is there to save)
    const volatile double* wl = Dl[grp];
    double gA[3] = {0.0, 0.0, 0.0}, gP[3] = {0.0, 0.0, 0.0};
    for (int kab = sub; kab < ab.nprim; kab += GTO_SPLIT) {
        const gto_prim_t pb = gto_load_prim(ab.data + (size_t)kab * GTO_PW, ab.swapped);
        double Eb[3][LA + 2][LB + 1][LAB + 2], dEb[3][LA + 1][LB + 1][LAB + 2];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            gto_herm<LA + 1, LB>(Eb[d], -pb.fb * ab.AB[d], pb.fa * ab.AB[d], pb.oo2p);
            gto_herm_deriv<LA, LB>(dEb[d], Eb[d], pb.fa * pb.p);
        }
        for (int kcd = 0; kcd < cd.nprim; ++kcd) {
            const gto_prim_t pk = gto_load_prim(cd.data + (size_t)kcd * GTO_PW, cd.swapped);
            double Ek[3][LC + 1][LD + 1][LCD + 1];
#pragma unroll
            for (int d = 0; d < 3; ++d) gto_herm<LC, LD>(Ek[d], -pk.fb * cd.AB[d], pk.fa * cd.AB[d], pk.oo2p);
            const double s = pb.p + pk.p, alpha = pb.p * pk.p / s;
            const double X = pb.P[0] - pk.P[0], Y = pb.P[1] - pk.P[1], Z = pb.P[2] - pk.P[2];
            double F[L + 1], Fs[L + 1], R[L + 1][L + 1][L + 1];
            gto_boys<L>(alpha * (X * X + Y * Y + Z * Z), F);
            double sc = 34.98683665524972497 / (pb.p * pk.p * sqrt(s)) * (pb.cck * pk.cck);
#pragma unroll
            for (int n = 0; n <= L; ++n) { Fs[n] = sc * F[n]; sc *= -2.0 * alpha; }
            gto_R_fill<L>(R, Fs, X, Y, Z);
            static_for<NCD>([&](auto ccdc) {
                constexpr int ccd = decltype(ccdc)::value, cc = ccd / ND, cd_ = ccd % ND;
                constexpr int kx = gto_pow(LC, cc, 0), lx = gto_pow(LD, cd_, 0), ky = gto_pow(LC, cc, 1),
                              ly = gto_pow(LD, cd_, 1), kz = gto_pow(LC, cc, 2), lz = gto_pow(LD, cd_, 2);
                if constexpr (NPART > 1 && cc != PART) return;          // (this launch takes the components cc = PART)
                // the other side's component folded into R, t + u + w <= LAB + 1: this side takes its own derivative
                // and d/dP from it
                double X0[LAB + 2][LAB + 2][LAB + 2];
                static_for<(LAB + 2) * (LAB + 2) * (LAB + 2)>([&](auto tuvc) {
                    constexpr int tuv = decltype(tuvc)::value, t = tuv / ((LAB + 2) * (LAB + 2)),
                                  u = (tuv / (LAB + 2)) % (LAB + 2), w = tuv % (LAB + 2);
                    if constexpr (t + u + w <= LAB + 1)
                        X0[t][u][w] = gto_ket_sum<t, u, w, kx + lx, ky + ly, kz + lz>(Ek[0][kx][lx], Ek[1][ky][ly],
                                                                                      Ek[2][kz][lz], R);
                });
                static_for<NAB>([&](auto cabc) {
                    constexpr int cab = decltype(cabc)::value, ca = cab / NB, cb = cab % NB;
                    constexpr int ix = gto_pow(LA, ca, 0), jx = gto_pow(LB, cb, 0), iy = gto_pow(LA, ca, 1),
                                  jy = gto_pow(LB, cb, 1), iz = gto_pow(LA, ca, 2), jz = gto_pow(LB, cb, 2);
                    constexpr int nx = ix + jx, ny = iy + jy, nz = iz + jz;
                    const double w = wl[cab * NCD + ccd];
                    const double(&ex)[LAB + 2] = Eb[0][ix][jx];
                    const double(&ey)[LAB + 2] = Eb[1][iy][jy];
                    const double(&ez)[LAB + 2] = Eb[2][iz][jz];
                    gA[0] += w * gto_bra_sum<nx + 1, ny, nz, 0, 0, 0>(dEb[0][ix][jx], ey, ez, X0);
                    gA[1] += w * gto_bra_sum<nx, ny + 1, nz, 0, 0, 0>(ex, dEb[1][iy][jy], ez, X0);
                    gA[2] += w * gto_bra_sum<nx, ny, nz + 1, 0, 0, 0>(ex, ey, dEb[2][iz][jz], X0);
                    gP[0] += w * gto_bra_sum<nx, ny, nz, 1, 0, 0>(ex, ey, ez, X0);
                    gP[1] += w * gto_bra_sum<nx, ny, nz, 0, 1, 0>(ex, ey, ez, X0);
                    gP[2] += w * gto_bra_sum<nx, ny, nz, 0, 0, 1>(ex, ey, ez, X0);
                });
            });
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double xa = gto_group_sum<GTO_SPLIT>(gA[d]), xp = gto_group_sum<GTO_SPLIT>(gP[d]);
        v[d] = xa; v[3 + d] = xp - xa;
    }
    if (sub == 0) grad_store(out, atA, atB, -1, -1, v);
}

// ---- reduction: one workgroup per (atom, geometry), fixed order -----------------------------------------------------
__global__ __launch_bounds__(GRAD_RT) void gto_grad_reduce_kernel(const double* __restrict__ rec, long nrec,
                                                                  const double* __restrict__ charges, int natm,
                                                                  const double* __restrict__ coords, int with_nuc,
                                                                  double* __restrict__ grad)
{
    __shared__ double red[3][GRAD_RT];
    const int a = blockIdx.x, g = blockIdx.y, t = threadIdx.x;
    double s[3] = {0.0, 0.0, 0.0};
    const double* base = rec + (size_t)g * nrec * GRAD_REC;
    for (long r = t; r < nrec; r += GRAD_RT) {
        const d2* p = reinterpret_cast<const d2*>(base + (size_t)r * GRAD_REC);
        const d2 i01 = p[6], i23 = p[7];
        const int at[4] = {(int)i01.x, (int)i01.y, (int)i23.x, (int)i23.y};
        const double* v = base + (size_t)r * GRAD_REC;
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (at[c] == a) { s[0] += v[3 * c]; s[1] += v[3 * c + 1]; s[2] += v[3 * c + 2]; }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) red[d][t] = s[d];
    __syncthreads();
    for (int o = GRAD_RT / 2; o > 0; o >>= 1) {
        if (t < o) {
#pragma unroll
            for (int d = 0; d < 3; ++d) red[d][t] += red[d][t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        double e[3] = {red[0][0], red[1][0], red[2][0]};
        if (with_nuc) {
            const double* xyz = coords + (size_t)g * natm * 3;
            double n[3] = {0.0, 0.0, 0.0};
            for (int b = 0; b < natm; ++b) {
                if (b == a) continue;
                const double dx = xyz[3 * a] - xyz[3 * b], dy = xyz[3 * a + 1] - xyz[3 * b + 1],
                             dz = xyz[3 * a + 2] - xyz[3 * b + 2];
                const double r2 = dx * dx + dy * dy + dz * dz;
                const double f = -charges[a] * charges[b] / (r2 * sqrt(r2));
                n[0] += f * dx; n[1] += f * dy; n[2] += f * dz;
            }
#pragma unroll
            for (int d = 0; d < 3; ++d) e[d] += n[d];
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) grad[((size_t)g * natm + a) * 3 + d] = e[d];
    }
}

// the reduction for `rows` stacks of nrec records (gto_grad.h: for the kernels of other files); grad [rows][natm][3]
int gto_grad_reduce_launch(const double* rec, long nrec, const double* charges, int natm, const double* coords,
                           int with_nuc, long rows, double* grad, hipStream_t st)
{
    for (long r0 = 0; r0 < rows; r0 += 65535) {
        const long n = rows - r0 < 65535 ? rows - r0 : 65535;
        hipLaunchKernelGGL(gto_grad_reduce_kernel, dim3(natm, (unsigned)n), dim3(GRAD_RT), 0, st,
                           rec + (size_t)r0 * nrec * GRAD_REC, nrec, charges, natm,
                           coords ? coords + (size_t)r0 * natm * 3 : nullptr, with_nuc ? 1 : 0,
                           grad + (size_t)r0 * natm * 3);
        OOVQE_CHECK_LAUNCH("gto_grad_reduce_kernel");
    }
    return 0;
}

// ---- AO densities of a CAS wave function ----------------------------------------------------------------------------
// D1 = Dc + Da, Dc = 2 C_c C_c^T, Da = C_a sym(gamma) C_a^T, and (E_2 = 1/2 sum (pq|rs) D2_pqrs)
//   D2_pqrs = Dc_pq Dc_rs - (Dc_pr Dc_qs + Dc_ps Dc_qr) / 4 + Dc_pq Da_rs + Dc_rs Da_pq
//             - (Dc_pr Da_qs + Dc_qr Da_ps + Dc_ps Da_qr + Dc_qs Da_pr) / 4 + sum_tuvw Gs_tuvw C_pt C_qu C_rv C_sw,
// the average over the 8 index permutations of the integrals' symmetry of the expression in the header (Gs the same
// average of the active 2-RDM).  A thread computes the element of one canonical quadruple (p >= q, r >= s, pq >= rs)
// and stores it to its (up to 8) places: the symmetry of D2 is exact.  LDS: the M = n_core + ncas columns of C, Dc, Da, Gs.
#define DENS_NT 256
__global__ __launch_bounds__(DENS_NT) void cas_ao_densities_kernel(const double* __restrict__ mo, int n, int n_core,
                                                                   int ncas, const double* __restrict__ gamma,
                                                                   const double* __restrict__ Gamma, long ncanon,
                                                                   double* __restrict__ d1, double* __restrict__ d2m)
{
    extern __shared__ double lds[];
    const int M = n_core + ncas, a2 = ncas * ncas;
    double* C = lds;                         // [n][M]
    double* Dc = C + (size_t)n * M;          // [n][n]
    double* Da = Dc + (size_t)n * n;         // [n][n]
    double* Gs = Da + (size_t)n * n;         // [ncas]^4
    const int g = blockIdx.y, t = threadIdx.x;
    const double* Cg = mo + (size_t)g * n * n;
    for (int k = t; k < n * M; k += DENS_NT) C[k] = Cg[(size_t)(k / M) * n + (k % M)];
    if (ncas > 0) {
        const double* Gg = Gamma + (size_t)g * a2 * a2;
        for (int k = t; k < a2 * a2; k += DENS_NT) {
            const int p = k / (a2 * ncas), q = (k / a2) % ncas, r = (k / ncas) % ncas, s = k % ncas;
            auto at = [&](int i, int j, int kk, int l) { return Gg[((i * ncas + j) * ncas + kk) * ncas + l]; };
            Gs[k] = 0.125 * (((at(p, q, r, s) + at(q, p, r, s)) + (at(p, q, s, r) + at(q, p, s, r)))
                             + ((at(r, s, p, q) + at(s, r, p, q)) + (at(r, s, q, p) + at(s, r, q, p))));
        }
    }
    __syncthreads();
    const double* gam = gamma ? gamma + (size_t)g * a2 : nullptr;
    for (int k = t; k < n * n; k += DENS_NT) {
        const int p = k / n, q = k - p * n;
        if (p < q) continue;
        double c = 0.0, a = 0.0;
        for (int i = 0; i < n_core; ++i) c += C[p * M + i] * C[q * M + i];
        for (int x = 0; x < ncas; ++x) {
            double h = 0.0;
            for (int y = 0; y < ncas; ++y) h += 0.5 * (gam[x * ncas + y] + gam[y * ncas + x]) * C[q * M + n_core + y];
            a += C[p * M + n_core + x] * h;
        }
        c *= 2.0;
        Dc[p * n + q] = c; Dc[q * n + p] = c;
        Da[p * n + q] = a; Da[q * n + p] = a;
        if (blockIdx.x == 0 && d1) {
            d1[((size_t)g * n + p) * n + q] = c + a;
            d1[((size_t)g * n + q) * n + p] = c + a;
        }
    }
    __syncthreads();
    if (!d2m) return;
    const long id = (long)blockIdx.x * DENS_NT + t;
    if (id >= ncanon) return;
    long I = (long)((sqrt(8.0 * (double)id + 1.0) - 1.0) * 0.5);
    while ((I + 1) * (I + 2) / 2 <= id) ++I;
    while (I * (I + 1) / 2 > id) --I;
    const long J = id - I * (I + 1) / 2;
    auto split = [](long P, int& hi, int& lo) {
        int h = (int)((sqrt(8.0 * (double)P + 1.0) - 1.0) * 0.5);
        while ((long)(h + 1) * (h + 2) / 2 <= P) ++h;
        while ((long)h * (h + 1) / 2 > P) --h;
        hi = h; lo = (int)(P - (long)h * (h + 1) / 2);
    };
    int p, q, r, s;
    split(I, p, q);
    split(J, r, s);
    double x = Dc[p * n + q] * Dc[r * n + s] - 0.25 * (Dc[p * n + r] * Dc[q * n + s] + Dc[p * n + s] * Dc[q * n + r]);
    if (ncas > 0) {
        x += Dc[p * n + q] * Da[r * n + s] + Dc[r * n + s] * Da[p * n + q];
        x -= 0.25 * ((Dc[p * n + r] * Da[q * n + s] + Dc[q * n + r] * Da[p * n + s])
                     + (Dc[p * n + s] * Da[q * n + r] + Dc[q * n + s] * Da[p * n + r]));
        const double *cp = C + p * M + n_core, *cq = C + q * M + n_core, *cr = C + r * M + n_core,
                     *cs = C + s * M + n_core;
        double A = 0.0;
        for (int i = 0; i < ncas; ++i) {
            double ai = 0.0;
            for (int j = 0; j < ncas; ++j) {
                double aj = 0.0;
                for (int k = 0; k < ncas; ++k) {
                    double ak = 0.0;
                    for (int l = 0; l < ncas; ++l) ak += Gs[((i * ncas + j) * ncas + k) * ncas + l] * cs[l];
                    aj += ak * cr[k];
                }
                ai += aj * cq[j];
            }
            A += ai * cp[i];
        }
        x += A;
    }
    const size_t n1 = (size_t)n, n2 = n1 * n1, n3 = n2 * n1;
    double* out = d2m + (size_t)g * n3 * n1;
    out[p * n3 + q * n2 + r * n1 + s] = x;
    out[q * n3 + p * n2 + r * n1 + s] = x;
    out[p * n3 + q * n2 + s * n1 + r] = x;
    out[q * n3 + p * n2 + s * n1 + r] = x;
    out[r * n3 + s * n2 + p * n1 + q] = x;
    out[s * n3 + r * n2 + p * n1 + q] = x;
    out[r * n3 + s * n2 + q * n1 + p] = x;
    out[s * n3 + r * n2 + q * n1 + p] = x;
}

// ---- host side --------------------------------------------------------------------------------------------------------

extern "C" int64_t oovqe_gto_gradient_work_size(int nshell, int max_nprim, int natm, int batch)
{
    const char* who = "oovqe_gto_gradient_work_size";
    if (gto_check_sizes(who, nshell, max_nprim, batch) != 0) return OOVQE_ERR_ARG;
    OOVQE_REQUIRE(natm >= 1, "%s: natm = %d", who, natm);
    return gto_work_base(nshell, max_nprim, batch) + (int64_t)batch * grad_records(nshell, natm) * GRAD_REC;
}

int grad_fork_t::fork(const char* who_, hipStream_t st_, bool wanted)
{
    who = who_;
    st = side = st_;
    if (!wanted) return 0;
    hipStream_t si = oovqe_internal_stream(0);
    hipEvent_t ev_fork = oovqe_internal_event();
    ev_join = oovqe_internal_event();
    if (si && si != st && ev_fork && ev_join) {
        OOVQE_CHECK_HIP(hipEventRecord(ev_fork, st), who);
        OOVQE_CHECK_HIP(hipStreamWaitEvent(si, ev_fork, 0), who);
        side = si;
    }
    return 0;
}

int grad_fork_t::join()
{
    if (side == st) return 0;
    hipStream_t forked = side;
    side = st;
    OOVQE_CHECK_HIP(hipEventRecord(ev_join, forked), who);
    OOVQE_CHECK_HIP(hipStreamWaitEvent(st, ev_join, 0), who);
    return 0;
}

namespace {
struct grad_args_t {
    const double* d1; const double* wq; const double* d2; long nrec;
    hipStream_t side;           // the launches of the quartets' second sides (grad_fork_t)
};

template <int LA, int LB> int grad_launch_one(gto_cls_t<LA, LB>, const gto_prep_t& p, const grad_args_t& a, long& off)
{
    const int count = p.cnt[gto_cls(LA, LB)];
    if (count == 0) return 0;
    unsigned grid;
    if (const int rc = gto_grid_split(p.who, (long)count * p.batch, &grid)) return rc;
    hipLaunchKernelGGL((gto_grad_one_kernel<LA, LB>), dim3(grid), dim3(GTO_NT), 0, p.st, p.iw, p.shells, p.nshell, count,
                       p.charges, p.natm, p.coords, p.batch, p.pairs, p.kp, p.nao, a.d1, a.wq, p.rec, off, a.nrec);
    OOVQE_CHECK_LAUNCH("gto_grad_one_kernel");
    off += (long)count * (p.natm + 1);
    return 0;
}

template <int LA, int LB, int LC, int LD, bool SWAP, int PART, int NPART>
int grad_launch_side(grad_side_t<LA, LB, LC, LD, SWAP, PART, NPART>, const gto_prep_t& p, const grad_args_t& a,
                     unsigned grid, int nbra, int nket, long nq, long off)
{
    hipLaunchKernelGGL((gto_grad_eri_kernel<LA, LB, LC, LD, SWAP, PART, NPART>), dim3(grid), dim3(GTO_NT), 0,
                       SWAP ? a.side : p.st, p.iw, p.shells, p.nshell, nbra, nket, nq, p.coords, p.natm, p.batch, p.pairs,
                       p.kp, p.nao, a.d2, p.rec, off, a.nrec);
    OOVQE_CHECK_LAUNCH("gto_grad_eri_kernel");
    return 0;
}
}  // namespace

extern "C" int oovqe_gto_gradient_batch(int nshell, const int32_t* shells, int nprim_total, const double* exps,
                                        const double* coefs, int natm, const double* charges, int batch,
                                        const double* coords, int nao, const double* d1, const double* wq,
                                        const double* d2, int with_nuc, double* grad, double* work,
                                        oovqe_stream_t stream)
{
    const char* who = "oovqe_gto_gradient_batch";
    hipStream_t st = (hipStream_t)stream;
    gto_prep_t p;
    OOVQE_REQUIRE(batch <= 65535, "%s: batch = %d (at most 65535 geometries per call)", who, batch);
    // (derivatives of d shells need f-type intermediates: a table with l = 2 is refused, before any launch)
    int rc = gto_prepare(who, 1, nshell, shells, nprim_total, exps, coefs, natm, charges, batch, coords, nao, nullptr, work,
                         st, &p);
    if (rc != 0 || batch == 0) return rc;
    OOVQE_REQUIRE(grad, "%s: null pointer", who);
    const bool one = d1 || wq, two = d2 != nullptr;
    grad_fork_t fk;
    if ((rc = fk.fork(who, st, two)) != 0) return rc;
    const grad_args_t a = {d1, wq, d2, grad_nrec(p, one, two), fk.side};
    rc = grad_launch_all(
        p, one, two, a.nrec,
        [&](auto s, unsigned grid, int nbra, int nket, long nq, long off) {
            return grad_launch_side(s, p, a, grid, nbra, nket, nq, off);
        },
        [&](auto c, long& off) { return grad_launch_one(c, p, a, off); });
    if (const int rj = fk.join()) return rj;        // (joined whatever happened above)
    if (rc != 0) return rc;
    return gto_grad_reduce_launch(p.rec, a.nrec, charges, natm, coords, with_nuc, batch, grad, st);
}

extern "C" int oovqe_cas_ao_densities_batch(const double* mo_coeff, int n, int n_core, int ncas, const double* gamma,
                                            const double* Gamma, int batch, double* d1, double* d2,
                                            oovqe_stream_t stream)
{
    const char* who = "oovqe_cas_ao_densities_batch";
    OOVQE_REQUIRE(n >= 1 && n <= OOVQE_INVSQRT_MAX_N, "%s: n = %d (1 .. %d)", who, n, OOVQE_INVSQRT_MAX_N);
    OOVQE_REQUIRE(n_core >= 0 && ncas >= 0 && ncas <= 8 && n_core + ncas <= n,
                  "%s: n_core = %d, ncas = %d (ncas <= 8, n_core + ncas <= n = %d)", who, n_core, ncas, n);
    OOVQE_REQUIRE(batch >= 0 && batch <= 65535, "%s: batch = %d (0 .. 65535)", who, batch);
    if (batch == 0 || (!d1 && !d2)) return 0;
    OOVQE_REQUIRE(mo_coeff && (ncas == 0 || (gamma && Gamma)), "%s: null pointer", who);
    const int M = n_core + ncas;
    const size_t lds = ((size_t)n * M + 2 * (size_t)n * n + (size_t)ncas * ncas * ncas * ncas) * sizeof(double);
    if (oovqe_ensure_dynamic_lds(reinterpret_cast<const void*>(&cas_ao_densities_kernel), lds) != 0) return OOVQE_ERR_HIP;
    const long np = (long)n * (n + 1) / 2, ncanon = np * (np + 1) / 2;
    const long blocks = d2 ? (ncanon + DENS_NT - 1) / DENS_NT : 1;
    hipLaunchKernelGGL(cas_ao_densities_kernel, dim3((unsigned)blocks, batch), dim3(DENS_NT), lds, (hipStream_t)stream,
                       mo_coeff, n, n_core, ncas, gamma, Gamma, ncanon, d1, d2);
    OOVQE_CHECK_LAUNCH("cas_ao_densities_kernel");
    return 0;
}
