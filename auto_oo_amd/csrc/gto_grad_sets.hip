// Nuclear gradients of a stack of geometries for SEVERAL density sets per geometry (gfx950): one pass over the
// derivative integrals of gto_grad.hip, contracted with nset sets (D1, WQ, D2) at once.
//
//   grad[g, k, A, :] = sum_pq D1[g,k,p,q] dh[p,q]/dR_A + sum_pq WQ[g,k,p,q] dS[p,q]/dR_A
//                    + 1/2 sum_pqrs D2[g,k,p,q,r,s] d(pq|rs)/dR_A + (bit k of nuc_mask) dE_nuc/dR_A
//
// In gto_grad_eri_kernel a weight enters in the last line only, gA[d] += w * gto_bra_sum(...): the Boys function,
// R_tuv, the fold X0 of the other side and the six bra sums of a term do not depend on the density.  The kernels here
// are those of gto_grad.hip -- pair data, class lists, quartet enumeration, GTO_SPLIT lane groups, one side per launch,
// (pp|pp) in three launches per side -- with that last line replaced by a loop over the sets of a TILE:
//
//   - the weight blocks of the tile's sets lie in LDS (per lane group and set: the NAB x NCD / NPART weights this launch
//     reads, at most 27);
//   - the six accumulators of a lane per set lie in LDS as well ([set][6][lane]: consecutive lanes, consecutive doubles),
//     updated by a read-modify-write per term.  Registers would hold 6 x 3 doubles at most beside the 256 + 216 of
//     (pp|pp); LDS holds GRAD_SETS_TILE = 5 sets in 24 KB per wave, so that as many waves fit a CU as the registers of
//     (pp|pp) allow (4);
//   - a call with more sets than one tile runs the launches once per tile, the sets spread evenly over the tiles.
//
// The sets of a tile are handled by a loop with a run-time count, each set with accumulators of its own: the sequence of
// operations that makes a set's numbers does not depend on how many sets share its tile nor on its place among them,
// so neither do its bits.  Records go to [geometry][set][record] -- for one set the layout of gto_grad.hip -- and the
// reduction adds the records of a (geometry, set) in the fixed order of gto_grad_reduce_kernel.  No floating-point
// atomics.
#include "gto_grad.h"

#define GRAD_SETS_TILE OOVQE_GTO_GRAD_SETS_TILE         // sets per pass over the integrals (5)

// the accumulators of one lane: a[(k * 6 + d) * GTO_NT], lane = threadIdx.x
__device__ __forceinline__ void sets_zero(double* a, int nk, int nd)
{
    for (int k = 0; k < nk; ++k)
        for (int d = 0; d < nd; ++d) a[(k * 6 + d) * GTO_NT] = 0.0;
}

// ---- one-electron terms ---------------------------------------------------------------------------------------------
// records of pair k of the class, per set: [natm + 1]: c < natm the attraction of nucleus c, natm: S and T
template <int LA, int LB>
__global__ __launch_bounds__(GTO_NT) void gto_grad_sets_one_kernel(
    const int* __restrict__ iw, const int* __restrict__ shells, int nshell, int count,
    const double* __restrict__ charges, int natm, const double* __restrict__ coords, int batch,
    const double* __restrict__ pairs, int kp, int nao, int nset, int k0, int nk, const double* __restrict__ d1,
    const double* __restrict__ wq, double* __restrict__ rec, long rec_off, long nrec)
{
    constexpr int NA = gto_ncomp(LA), NB = gto_ncomp(LB), NAB = NA * NB, L = LA + LB;
    __shared__ double Wl[GTO_NT / GTO_SPLIT][GRAD_SETS_TILE][2][NAB];      // [.][set][0: D1, 1: WQ][component]
    __shared__ double Al[GRAD_SETS_TILE * 6 * GTO_NT];
    long tid = (long)blockIdx.x * GTO_NT + threadIdx.x;
    const int sub = (int)(tid % GTO_SPLIT), grp = (int)(threadIdx.x / GTO_SPLIT);
    tid /= GTO_SPLIT;
    if (tid >= (long)count * batch) return;
    const int g = (int)(tid / count), k = (int)(tid - (long)g * count);
    const long npair = (long)nshell * (nshell + 1) / 2;
    const double* xyz = coords + (size_t)g * natm * 3;
    const gto_pair_ref_t ab = gto_pair_ref(iw + nshell, gto_cls(LA, LB), k, npair, iw, shells, xyz,
                                           pairs + (size_t)g * npair * kp * GTO_PW, kp);
    const int atA = shells[4 * ab.sa], atB = shells[4 * ab.sb];
    // record c of set ks of this pair
    auto out = [&](int ks, int c) {
        return rec + (((size_t)g * nset + k0 + ks) * nrec + rec_off + (size_t)k * (natm + 1) + c) * GRAD_REC;
    };
    const double deg = (ab.sa == ab.sb) ? 1.0 : 2.0;
    for (int c = sub; c < nk * NAB; c += GTO_SPLIT) {
        const int ks = c / NAB, cm = c - ks * NAB;
        const size_t idx = (((size_t)g * nset + k0 + ks) * nao + (ab.oa + cm / NB)) * nao + (ab.ob + cm % NB);
        Wl[grp][ks][0][cm] = d1 ? deg * d1[idx] : 0.0;
        Wl[grp][ks][1][cm] = wq ? deg * wq[idx] : 0.0;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const volatile double* wl = &Wl[grp][0][0][0];
    double* acc = Al + threadIdx.x;
    // overlap and kinetic energy: two centres, B = -A
    {
        sets_zero(acc, nk, 3);
        if (atA != atB) {
            for (int kab = sub; kab < ab.nprim; kab += GTO_SPLIT) {
                const gto_prim_t pr = gto_load_prim(ab.data + (size_t)kab * GTO_PW, ab.swapped);
                double E[3][LA + 2][LB + 3][LA + LB + 4];
#pragma unroll
                for (int d = 0; d < 3; ++d) gto_herm<LA + 1, LB + 2>(E[d], -pr.fb * ab.AB[d], pr.fa * ab.AB[d], pr.oo2p);
                const double a = pr.fa * pr.p, b = pr.fb * pr.p;
                const double pop = GTO_PI / pr.p;
                const double fS = pr.cck * pop * sqrt(pop);
                static_for<NAB>([&](auto cc) {
                    constexpr int c = decltype(cc)::value, ca = c / NB, cb = c % NB;
                    double s1[3], t1[3], ds[3], dt[3], dS[3], dT[3];
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
                        dS[d] = ds[d] * s1[e] * s1[f];
                        dT[d] = dt[d] * s1[e] * s1[f] + ds[d] * (t1[e] * s1[f] + s1[e] * t1[f]);
                    });
#pragma nounroll
                    for (int ks = 0; ks < nk; ++ks) {
                        const double w1 = wl[(ks * 2 + 0) * NAB + c], ws = wl[(ks * 2 + 1) * NAB + c];
#pragma unroll
                        for (int d = 0; d < 3; ++d) acc[(ks * 6 + d) * GTO_NT] += fS * (ws * dS[d] + w1 * dT[d]);
                    }
                });
            }
        }
        for (int ks = 0; ks < nk; ++ks) {
            double v[12];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double x = gto_group_sum<GTO_SPLIT>(acc[(ks * 6 + d) * GTO_NT]);
                v[d] = x; v[3 + d] = -x; v[6 + d] = 0.0; v[9 + d] = 0.0;
            }
            if (sub == 0) {
                if (atA != atB) grad_store(out(ks, natm), atA, atB, -1, -1, v);
                else grad_store(out(ks, natm), -1, -1, -1, -1, v);
            }
        }
    }
    // nuclear attraction: the basis functions on A and B and the operator on every nucleus c
    for (int c = 0; c < natm; ++c) {
        sets_zero(acc, nk, 6);
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
                static_for<NAB>([&](auto cc) {
                    constexpr int cm = decltype(cc)::value, ca = cm / NB, cb = cm % NB;
                    constexpr int ix = gto_pow(LA, ca, 0), jx = gto_pow(LB, cb, 0), iy = gto_pow(LA, ca, 1),
                                  jy = gto_pow(LB, cb, 1), iz = gto_pow(LA, ca, 2), jz = gto_pow(LB, cb, 2);
                    double t[6];
                    t[0] = gto_bra_sum<ix + jx + 1, iy + jy, iz + jz, 0, 0, 0>(dE[0][ix][jx], E[1][iy][jy], E[2][iz][jz], R);
                    t[1] = gto_bra_sum<ix + jx, iy + jy + 1, iz + jz, 0, 0, 0>(E[0][ix][jx], dE[1][iy][jy], E[2][iz][jz], R);
                    t[2] = gto_bra_sum<ix + jx, iy + jy, iz + jz + 1, 0, 0, 0>(E[0][ix][jx], E[1][iy][jy], dE[2][iz][jz], R);
                    t[3] = gto_bra_sum<ix + jx, iy + jy, iz + jz, 1, 0, 0>(E[0][ix][jx], E[1][iy][jy], E[2][iz][jz], R);
                    t[4] = gto_bra_sum<ix + jx, iy + jy, iz + jz, 0, 1, 0>(E[0][ix][jx], E[1][iy][jy], E[2][iz][jz], R);
                    t[5] = gto_bra_sum<ix + jx, iy + jy, iz + jz, 0, 0, 1>(E[0][ix][jx], E[1][iy][jy], E[2][iz][jz], R);
#pragma nounroll
                    for (int ks = 0; ks < nk; ++ks) {
                        const double w = wl[(ks * 2 + 0) * NAB + cm];
#pragma unroll
                        for (int d = 0; d < 6; ++d) acc[(ks * 6 + d) * GTO_NT] += w * t[d];
                    }
                });
            }
        }
        for (int ks = 0; ks < nk; ++ks) {
            double v[12];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double xa = gto_group_sum<GTO_SPLIT>(acc[(ks * 6 + d) * GTO_NT]),
                             xp = gto_group_sum<GTO_SPLIT>(acc[(ks * 6 + 3 + d) * GTO_NT]);
                v[d] = xa; v[3 + d] = xp - xa; v[6 + d] = -xp; v[9 + d] = 0.0;
            }
            if (sub == 0) {
                if (live) grad_store(out(ks, c), atA, atB, c, -1, v);
                else grad_store(out(ks, c), -1, -1, -1, -1, v);
            }
        }
    }
}

// ---- two-electron term ------------------------------------------------------------------------------------------------
// gto_grad_eri_kernel (one side of every quartet per launch, see there) for the sets k0 .. k0 + nk - 1 of every geometry.
template <int LA, int LB, int LC, int LD, bool SWAP, int PART, int NPART>
__global__ __launch_bounds__(GTO_NT) void gto_grad_sets_eri_kernel(
    const int* __restrict__ iw, const int* __restrict__ shells, int nshell, int nbra, int nket, long nquart,
    const double* __restrict__ coords, int natm, int batch, const double* __restrict__ pairs, int kp, int nao, int nset,
    int k0, int nk, const double* __restrict__ d2m, double* __restrict__ rec, long rec_off, long nrec)
{
    constexpr int NA = gto_ncomp(LA), NB = gto_ncomp(LB), NC = gto_ncomp(LC), ND = gto_ncomp(LD);
    constexpr int NAB = NA * NB, NCD = NC * ND, LAB = LA + LB, LCD = LC + LD;
    constexpr int L = LAB + LCD + 1;
    constexpr bool same_cls = (LA == LC && LB == LD);
    // the components of the other side this launch takes: cc = PART of NPART, i.e. ccd = CD0 .. CD0 + NCDL - 1
    constexpr int NCDL = NCD / NPART, CD0 = (NPART > 1) ? PART * ND : 0;
    constexpr int NW = NAB * NCDL;
    static_assert(NPART == 1 || NPART == NC, "the parts are the components of the other side's first shell");
    __shared__ double Dl[GTO_NT / GTO_SPLIT][GRAD_SETS_TILE][NW];
    __shared__ double Al[GRAD_SETS_TILE * 6 * GTO_NT];
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
    auto out = [&](int ks) {
        return rec + (((size_t)g * nset + k0 + ks) * nrec + rec_off + (2 * r + (SWAP ? 1 : 0)) * NPART + PART) * GRAD_REC;
    };
    double v[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) v[c] = 0.0;
    if (atA == atB && atA == atC && atA == atD) {          // one centre: exactly zero
        if (sub == 0)
            for (int ks = 0; ks < nk; ++ks) grad_store(out(ks), -1, -1, -1, -1, v);
        return;
    }
    {
        // E_2 = 1/2 sum D2 (pq|rs) over ALL index quadruples: a unique quartet stands for up to 8 of them
        const double deg = 0.5 * (ab.sa == ab.sb ? 1.0 : 2.0) * (cd.sa == cd.sb ? 1.0 : 2.0)
                           * ((same_cls && k1 == k2) ? 1.0 : 2.0);
        const size_t n1 = (size_t)nao;
        for (int c = sub; c < nk * NW; c += GTO_SPLIT) {
            const int ks = c / NW, cw = c - ks * NW;
            const int cab = cw / NCDL, ccd = CD0 + (cw - cab * NCDL);
            const double* dg = d2m + ((size_t)g * nset + k0 + ks) * n1 * n1 * n1 * n1;
            const size_t mu = ab.oa + cab / NB, nu = ab.ob + cab % NB, la = cd.oa + ccd / ND, si = cd.ob + ccd % ND;
            Dl[grp][ks][cw] = deg * dg[((mu * n1 + nu) * n1 + la) * n1 + si];
        }
    }
    double* acc = Al + threadIdx.x;
    sets_zero(acc, nk, 6);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();

    // (read as volatile: the weights are loop invariant, see gto_grad_eri_kernel)
    const volatile double* wl = &Dl[grp][0][0];
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
            static_for<NCDL>([&](auto ccdc) {
                constexpr int cl = decltype(ccdc)::value, ccd = CD0 + cl, cc = ccd / ND, cd_ = ccd % ND;
                constexpr int kx = gto_pow(LC, cc, 0), lx = gto_pow(LD, cd_, 0), ky = gto_pow(LC, cc, 1),
                              ly = gto_pow(LD, cd_, 1), kz = gto_pow(LC, cc, 2), lz = gto_pow(LD, cd_, 2);
                // the other side's component folded into R, t + u + w <= LAB + 1
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
                    const double(&ex)[LAB + 2] = Eb[0][ix][jx];
                    const double(&ey)[LAB + 2] = Eb[1][iy][jy];
                    const double(&ez)[LAB + 2] = Eb[2][iz][jz];
                    // the six values of this term, once for all sets
                    double t[6];
                    t[0] = gto_bra_sum<nx + 1, ny, nz, 0, 0, 0>(dEb[0][ix][jx], ey, ez, X0);
                    t[1] = gto_bra_sum<nx, ny + 1, nz, 0, 0, 0>(ex, dEb[1][iy][jy], ez, X0);
                    t[2] = gto_bra_sum<nx, ny, nz + 1, 0, 0, 0>(ex, ey, dEb[2][iz][jz], X0);
                    t[3] = gto_bra_sum<nx, ny, nz, 1, 0, 0>(ex, ey, ez, X0);
                    t[4] = gto_bra_sum<nx, ny, nz, 0, 1, 0>(ex, ey, ez, X0);
                    t[5] = gto_bra_sum<nx, ny, nz, 0, 0, 1>(ex, ey, ez, X0);
#pragma nounroll
                    for (int ks = 0; ks < nk; ++ks) {
                        const double w = wl[ks * NW + cab * NCDL + cl];
#pragma unroll
                        for (int d = 0; d < 6; ++d) acc[(ks * 6 + d) * GTO_NT] += w * t[d];
                    }
                });
            });
        }
    }
    for (int ks = 0; ks < nk; ++ks) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double xa = gto_group_sum<GTO_SPLIT>(acc[(ks * 6 + d) * GTO_NT]),
                         xp = gto_group_sum<GTO_SPLIT>(acc[(ks * 6 + 3 + d) * GTO_NT]);
            v[d] = xa; v[3 + d] = xp - xa;
        }
        if (sub == 0) grad_store(out(ks), atA, atB, -1, -1, v);
    }
}

// ---- reduction: one workgroup per (atom, geometry, set), the order of gto_grad_reduce_kernel ----------------------------
__global__ __launch_bounds__(GRAD_RT) void gto_grad_sets_reduce_kernel(const double* __restrict__ rec, long nrec,
                                                                       const double* __restrict__ charges, int natm,
                                                                       const double* __restrict__ coords, int nset,
                                                                       unsigned nuc_mask, double* __restrict__ grad)
{
    __shared__ double red[3][GRAD_RT];
    const int a = blockIdx.x, g = blockIdx.y, ks = blockIdx.z, t = threadIdx.x;
    double s[3] = {0.0, 0.0, 0.0};
    const double* base = rec + ((size_t)g * nset + ks) * nrec * GRAD_REC;
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
        if ((nuc_mask >> ks) & 1u) {
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
        for (int d = 0; d < 3; ++d) grad[(((size_t)g * nset + ks) * natm + a) * 3 + d] = e[d];
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------
// (for nset = 1 the size of oovqe_gto_gradient_work_size: the records of a set are those of the single-set entry)
extern "C" int64_t oovqe_gto_gradient_sets_work_size(int nshell, int max_nprim, int natm, int batch, int nset)
{
    const char* who = "oovqe_gto_gradient_sets_work_size";
    if (gto_check_sizes(who, nshell, max_nprim, batch) != 0) return OOVQE_ERR_ARG;
    OOVQE_REQUIRE(natm >= 1, "%s: natm = %d", who, natm);
    if (grad_check_nset(who, nset) != 0) return OOVQE_ERR_ARG;
    return gto_work_base(nshell, max_nprim, batch) + (int64_t)batch * nset * grad_records(nshell, natm) * GRAD_REC;
}

namespace {
struct sets_args_t {
    int nset; int k0; int nk; const double* d1; const double* wq; const double* d2; long nrec;
    hipStream_t side;           // the launches of the quartets' second sides (grad_fork_t)
};

template <int LA, int LB> int sets_launch_one(gto_cls_t<LA, LB>, const gto_prep_t& p, const sets_args_t& a, long& off)
{
    const int count = p.cnt[gto_cls(LA, LB)];
    if (count == 0) return 0;
    unsigned grid;
    if (const int rc = gto_grid_split(p.who, (long)count * p.batch, &grid)) return rc;
    hipLaunchKernelGGL((gto_grad_sets_one_kernel<LA, LB>), dim3(grid), dim3(GTO_NT), 0, p.st, p.iw, p.shells, p.nshell,
                       count, p.charges, p.natm, p.coords, p.batch, p.pairs, p.kp, p.nao, a.nset, a.k0, a.nk, a.d1, a.wq,
                       p.rec, off, a.nrec);
    OOVQE_CHECK_LAUNCH("gto_grad_sets_one_kernel");
    off += (long)count * (p.natm + 1);
    return 0;
}

template <int LA, int LB, int LC, int LD, bool SWAP, int PART, int NPART>
int sets_launch_side(grad_side_t<LA, LB, LC, LD, SWAP, PART, NPART>, const gto_prep_t& p, const sets_args_t& a,
                     unsigned grid, int nbra, int nket, long nq, long off)
{
    hipLaunchKernelGGL((gto_grad_sets_eri_kernel<LA, LB, LC, LD, SWAP, PART, NPART>), dim3(grid), dim3(GTO_NT), 0,
                       SWAP ? a.side : p.st, p.iw, p.shells, p.nshell, nbra, nket, nq, p.coords, p.natm, p.batch, p.pairs,
                       p.kp, p.nao, a.nset, a.k0, a.nk, a.d2, p.rec, off, a.nrec);
    OOVQE_CHECK_LAUNCH("gto_grad_sets_eri_kernel");
    return 0;
}
}  // namespace

extern "C" int oovqe_gto_gradient_sets_batch(int nshell, const int32_t* shells, int nprim_total, const double* exps,
                                             const double* coefs, int natm, const double* charges, int batch,
                                             const double* coords, int nao, int nset, const double* d1,
                                             const double* wq, const double* d2, unsigned nuc_mask, double* grad,
                                             double* work, oovqe_stream_t stream)
{
    const char* who = "oovqe_gto_gradient_sets_batch";
    hipStream_t st = (hipStream_t)stream;
    gto_prep_t p;
    if (grad_check_nset(who, nset) != 0) return OOVQE_ERR_ARG;
    OOVQE_REQUIRE(batch <= 65535, "%s: batch = %d (at most 65535 geometries per call)", who, batch);
    // (a table with l = 2 is refused here, before any launch, as by oovqe_gto_gradient_batch)
    int rc = gto_prepare(who, 1, nshell, shells, nprim_total, exps, coefs, natm, charges, batch, coords, nao, nullptr, work,
                         st, &p);
    if (rc != 0 || batch == 0) return rc;
    OOVQE_REQUIRE(grad, "%s: null pointer", who);
    const bool one = d1 || wq, two = d2 != nullptr;
    const long nrec = grad_nrec(p, one, two);
    // second sides on the library's internal stream, as in oovqe_gto_gradient_batch
    grad_fork_t fk;
    if ((rc = fk.fork(who, st, two)) != 0) return rc;
    rc = grad_for_tiles(nset, GRAD_SETS_TILE, [&](int k0, int nk) {
        const sets_args_t a = {nset, k0, nk, d1, wq, d2, nrec, fk.side};
        return grad_launch_all(
            p, one, two, nrec,
            [&](auto s, unsigned grid, int nbra, int nket, long nq, long off) {
                return sets_launch_side(s, p, a, grid, nbra, nket, nq, off);
            },
            [&](auto c, long& off) { return sets_launch_one(c, p, a, off); });
    });
    if (const int rj = fk.join()) return rj;        // (joined whatever happened above)
    if (rc != 0) return rc;
    hipLaunchKernelGGL(gto_grad_sets_reduce_kernel, dim3(natm, batch, nset), dim3(GRAD_RT), 0, st, p.rec, nrec, charges,
                       natm, coords, nset, nuc_mask, grad);
    OOVQE_CHECK_LAUNCH("gto_grad_sets_reduce_kernel");
    return 0;
}
