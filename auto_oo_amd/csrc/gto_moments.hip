// Dipole and second-moment integrals of a stack of geometries and their contraction with densities (gfx950).
//
//   M^c_{mu nu} = <mu| (x - Ox)^ex (y - Oy)^ey (z - Oz)^ez |nu>,  c = x, y, z | xx, xy, xz, yy, yz, zz
//
// over the basis functions of `overlap` (gto.hip / gto_d.hip: the same shell tables, pair data, class lists, order and
// normalisation).  Per primitive pair and dimension, with the Hermite coefficients E^ij_t of gto_herm, X = P - O and
// everything in units of sqrt(pi / p):
//
//   S^0_ij = E_0,   S^1_ij = X E_0 + E_1,   S^2_ij = (X^2 + 1/2p) E_0 + 2 X E_1 + 2 E_2
//
// and the integral is the product of the three dimensions times c_a c_b exp(-mu |AB|^2) (pi / p)^(3/2).  No Boys
// function.
//
//   gto_mom_kernel     <la, lb>, la, lb <= 1: one shell pair per group of GTO_SPLIT lanes, everything in registers (the
//                      style of gto_one_kernel)
//   gto_mom_d_kernel   <2, lb>: a workgroup owns one (geometry, shell pair); E of one dimension per lane, kept in LDS;
//                      every accumulator is owned by one lane and adds its primitive pairs in their stored order; the d
//                      components are finished in LDS by gto_d_pass before the stores (the style of gto_d_one_kernel)
//   gto_mom_expect_kernel  out[g][k][c] = -sum_pq dens[g][k][p][q] M^c[g][p][q] + (with_nuc[k]) sum_A Z_A (R_A - O)^c:
//                      one workgroup per (geometry, density), strided partial sums and a tree in LDS (fixed order)
//
// All nine components are accumulated by the same instructions whatever `order` asks for; order 1 stores the first
// three.  Every unique element is computed once and stored to both places.  No atomics, no scratch.
// The bodies are __host__ __device__ functions: a CPU build (GTO_MOMENTS_BODIES_ONLY: no kernel, no entry point) runs
// them with one lane per workgroup, or with the lanes as host threads and GTO_HOST_BARRIER as the barrier.
#include "gto.h"

#define GTO_MOM_NC 9             // x, y, z, xx, xy, xz, yy, yz, zz
#define GTO_MOM_NT 64            // lanes of a workgroup of the d classes
#define GTO_MOM_RT 256           // lanes of the contraction

// power of coordinate d in moment component c (one hexadecimal digit per component, c = 0 the lowest)
__host__ __device__ constexpr int gto_mom_pow(int c, int d)
{
    return (int)(((d == 0 ? 0x000112001ULL : (d == 1 ? 0x012010010ULL : 0x210100100ULL)) >> (4 * c)) & 15);
}
// sum_t E_t M^e_t of one dimension in units of sqrt(pi / p); e0, e1, e2 = E_0, E_1, E_2 (zero beyond i + j)
__host__ __device__ __forceinline__ double gto_mom_1d(int e, double X, double oo2p, double e0, double e1, double e2)
{
    return e == 0 ? e0 : (e == 1 ? X * e0 + e1 : (X * X + oo2p) * e0 + 2.0 * X * e1 + 2.0 * e2);
}
__host__ __device__ __forceinline__ void gto_mom_origin(const double* __restrict__ origin, int g, double (&O)[3])
{
#pragma unroll
    for (int d = 0; d < 3; ++d) O[d] = origin ? origin[(size_t)3 * g + d] : 0.0;
}

// ---- classes ss, ps, pp ----------------------------------------------------------------------------------------------
template <int LA, int LB, int SPLIT>
__host__ __device__ __forceinline__ void gto_mom_body(long tid, const int* __restrict__ iw,
                                                      const int* __restrict__ shells, int nshell, int count,
                                                      const double* __restrict__ coords, int natm, int batch,
                                                      const double* __restrict__ pairs, int kp, int nao, int ncomp,
                                                      const double* __restrict__ origin, double* __restrict__ moments)
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
    double O[3];
    gto_mom_origin(origin, g, O);
    double acc[GTO_MOM_NC][NA * NB];
#pragma unroll
    for (int c = 0; c < GTO_MOM_NC; ++c)
#pragma unroll
        for (int i = 0; i < NA * NB; ++i) acc[c][i] = 0.0;
    for (int kab = sub; kab < ab.nprim; kab += SPLIT) {
        const gto_prim_t pr = gto_load_prim(ab.data + (size_t)kab * GTO_PW, ab.swapped);
        double E[3][LA + 1][LB + 1][L + 1];
#pragma unroll
        for (int d = 0; d < 3; ++d) gto_herm<LA, LB>(E[d], -pr.fb * ab.AB[d], pr.fa * ab.AB[d], pr.oo2p);
        const double pop = GTO_PI / pr.p;
        const double fS = pr.cck * pop * sqrt(pop);
        // the three 1-D moments of every (i, j) of every dimension, once per primitive pair
        double m[3][LA + 1][LB + 1][3];
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int i = 0; i <= LA; ++i)
#pragma unroll
                for (int j = 0; j <= LB; ++j) {
                    const double e0 = E[d][i][j][0], e1 = L >= 1 ? E[d][i][j][L >= 1 ? 1 : 0] : 0.0,
                                 e2 = L >= 2 ? E[d][i][j][L >= 2 ? 2 : 0] : 0.0;
#pragma unroll
                    for (int e = 0; e < 3; ++e) m[d][i][j][e] = gto_mom_1d(e, pr.P[d] - O[d], pr.oo2p, e0, e1, e2);
                }
        static_for<GTO_MOM_NC>([&](auto cc) {
            static_for<NA * NB>([&](auto cabc) {
                constexpr int c = decltype(cc)::value, cab = decltype(cabc)::value, ca = cab / NB, cb = cab % NB;
                acc[c][cab] += fS * (m[0][gto_pow(LA, ca, 0)][gto_pow(LB, cb, 0)][gto_mom_pow(c, 0)] *
                                     m[1][gto_pow(LA, ca, 1)][gto_pow(LB, cb, 1)][gto_mom_pow(c, 1)] *
                                     m[2][gto_pow(LA, ca, 2)][gto_pow(LB, cb, 2)][gto_mom_pow(c, 2)]);
            });
        });
    }
#pragma unroll
    for (int c = 0; c < GTO_MOM_NC; ++c)
#pragma unroll
        for (int i = 0; i < NA * NB; ++i) acc[c][i] = gto_group_sum<SPLIT>(acc[c][i]);
    // (after the butterfly every lane of the group holds every value: lane `sub` stores every SPLIT-th of them)
    const bool same = ab.sa == ab.sb;
    static_for<GTO_MOM_NC>([&](auto cc) {
        static_for<NA * NB>([&](auto cabc) {
            constexpr int c = decltype(cc)::value, cab = decltype(cabc)::value, ca = cab / NB, cb = cab % NB;
            const int mu = ab.oa + ca, nu = ab.ob + cb;
            if (c < ncomp && (c * NA * NB + cab) % SPLIT == sub && (!same || mu >= nu) && mu < nao && nu < nao) {
                double* out = moments + ((size_t)g * ncomp + c) * nao * nao;
                const double x = acc[c][cab];
                out[(size_t)mu * nao + nu] = x;
                out[(size_t)nu * nao + mu] = x;
            }
        });
    });
}

// ---- classes ds, dp, dd ----------------------------------------------------------------------------------------------
template <int LA, int LB> struct gto_mom_lds_t {
    static constexpr int NAB = gto_ncomp(LA) * gto_ncomp(LB);
    double acc[GTO_MOM_NC * NAB];                  // [component][ca][cb]
    double E[3][LA + 1][LB + 1][LA + LB + 1];
};

template <int LA, int LB>
__host__ __device__ __forceinline__ void gto_mom_d_body(long grp, int lane, int nlane, gto_mom_lds_t<LA, LB>& s,
                                                        const int* __restrict__ iw, const int* __restrict__ shells,
                                                        int nshell, int count, const double* __restrict__ coords,
                                                        int natm, int batch, const double* __restrict__ pairs, int kp,
                                                        int nao, int ncomp, const double* __restrict__ origin,
                                                        double* __restrict__ moments)
{
    static_assert(LA == 2 && LB <= 2, "the classes with a d shell");
    constexpr int NB = gto_ncomp(LB), NAB = gto_mom_lds_t<LA, LB>::NAB;
    if (grp >= (long)count * batch) return;
    const int g = (int)(grp / count), k = (int)(grp - (long)g * count);
    const long npair = (long)nshell * (nshell + 1) / 2;
    const double* xyz = coords + (size_t)g * natm * 3;
    const gto_pair_ref_t ab = gto_pair_ref(iw + nshell, gto_cls(LA, LB), k, npair, iw, shells, xyz,
                                           pairs + (size_t)g * npair * kp * GTO_PW, kp);
    double O[3];
    gto_mom_origin(origin, g, O);
    const int total = ncomp * NAB;
    for (int it = lane; it < total; it += nlane) s.acc[it] = 0.0;
    gto_sync();
    for (int kab = 0; kab < ab.nprim; ++kab) {
        const gto_prim_t pr = gto_load_prim(ab.data + (size_t)kab * GTO_PW, ab.swapped);
        for (int d = lane; d < 3; d += nlane) {
            double E[LA + 1][LB + 1][LA + LB + 1];
            const double q = gto_pick(ab.AB, d);
            gto_herm<LA, LB>(E, -pr.fb * q, pr.fa * q, pr.oo2p);
#pragma unroll
            for (int i = 0; i <= LA; ++i)
#pragma unroll
                for (int j = 0; j <= LB; ++j)
#pragma unroll
                    for (int t = 0; t <= LA + LB; ++t) s.E[d][i][j][t] = E[i][j][t];
        }
        gto_sync();
        const double pop = GTO_PI / pr.p;
        const double fS = pr.cck * pop * sqrt(pop);
        for (int it = lane; it < total; it += nlane) {
            const int c = it / NAB, cab = it - c * NAB, ca = cab / NB, cb = cab - ca * NB;
            double m[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double* e = s.E[d][gto_pow(LA, ca, d)][gto_pow(LB, cb, d)];      // (LA + LB >= 2: E_2 exists)
                m[d] = gto_mom_1d(gto_mom_pow(c, d), gto_pick(pr.P, d) - gto_pick(O, d), pr.oo2p, e[0], e[1], e[2]);
            }
            s.acc[it] += fS * (m[0] * m[1] * m[2]);
        }
        gto_sync();
    }
    // the form of the d shells (the flag of the l field), one index after the other
    int na = gto_ncomp(LA), nb = NB;
    {
        const bool cart = (shells[4 * ab.sa + 1] & OOVQE_GTO_CARTESIAN) != 0;
        gto_d_pass(s.acc, total, NB, cart, lane, nlane);
        na = cart ? 6 : 5;
    }
    if (LB == 2) {
        const bool cart = (shells[4 * ab.sb + 1] & OOVQE_GTO_CARTESIAN) != 0;
        gto_d_pass(s.acc, total, 1, cart, lane, nlane);
        nb = cart ? 6 : 5;
    }
    const bool same = ab.sa == ab.sb;
    for (int it = lane; it < total; it += nlane) {
        const int c = it / NAB, cab = it - c * NAB, ca = cab / NB, cb = cab - ca * NB;
        if (ca >= na || cb >= nb) continue;
        const int mu = ab.oa + ca, nu = ab.ob + cb;
        if ((!same || mu >= nu) && mu < nao && nu < nao) {
            double* out = moments + ((size_t)g * ncomp + c) * nao * nao;
            const double x = s.acc[it];
            out[(size_t)mu * nao + nu] = x;
            out[(size_t)nu * nao + mu] = x;
        }
    }
}

#ifndef GTO_MOMENTS_BODIES_ONLY
template <int LA, int LB>
__global__ __launch_bounds__(GTO_NT) void gto_mom_kernel(const int* __restrict__ iw, const int* __restrict__ shells,
                                                         int nshell, int count, const double* __restrict__ coords,
                                                         int natm, int batch, const double* __restrict__ pairs, int kp,
                                                         int nao, int ncomp, const double* __restrict__ origin,
                                                         double* __restrict__ moments)
{
    gto_mom_body<LA, LB, GTO_SPLIT>((long)blockIdx.x * GTO_NT + threadIdx.x, iw, shells, nshell, count, coords, natm,
                                    batch, pairs, kp, nao, ncomp, origin, moments);
}

template <int LA, int LB>
__global__ __launch_bounds__(GTO_MOM_NT) void gto_mom_d_kernel(const int* __restrict__ iw,
                                                               const int* __restrict__ shells, int nshell, int count,
                                                               const double* __restrict__ coords, int natm, int batch,
                                                               const double* __restrict__ pairs, int kp, int nao,
                                                               int ncomp, const double* __restrict__ origin,
                                                               double* __restrict__ moments)
{
    __shared__ gto_mom_lds_t<LA, LB> s;
    gto_mom_d_body<LA, LB>((long)blockIdx.x, (int)threadIdx.x, GTO_MOM_NT, s, iw, shells, nshell, count, coords, natm,
                           batch, pairs, kp, nao, ncomp, origin, moments);
}

// ---- contraction: one workgroup per (density, geometry), fixed order -------------------------------------------------
__global__ __launch_bounds__(GTO_MOM_RT) void gto_mom_expect_kernel(const double* __restrict__ moments, int ncomp,
                                                                    int nao, const double* __restrict__ dens, int nd,
                                                                    int natm, const double* __restrict__ charges,
                                                                    const double* __restrict__ coords,
                                                                    const double* __restrict__ origin,
                                                                    const int* __restrict__ with_nuc,
                                                                    double* __restrict__ out)
{
    __shared__ double red[GTO_MOM_NC][GTO_MOM_RT];
    const int k = blockIdx.x, g = blockIdx.y, t = threadIdx.x;
    const long nn = (long)nao * nao;
    const double* D = dens + ((size_t)g * nd + k) * nn;
    const double* M = moments + (size_t)g * ncomp * nn;
    double s[GTO_MOM_NC];
#pragma unroll
    for (int c = 0; c < GTO_MOM_NC; ++c) s[c] = 0.0;
    for (long i = t; i < nn; i += GTO_MOM_RT) {
        const double d = D[i];
#pragma unroll
        for (int c = 0; c < GTO_MOM_NC; ++c)
            if (c < ncomp) s[c] += d * M[(size_t)c * nn + i];
    }
#pragma unroll
    for (int c = 0; c < GTO_MOM_NC; ++c) red[c][t] = s[c];
    __syncthreads();
    for (int o = GTO_MOM_RT / 2; o > 0; o >>= 1) {
        if (t < o) {
#pragma unroll
            for (int c = 0; c < GTO_MOM_NC; ++c) red[c][t] += red[c][t + o];
        }
        __syncthreads();
    }
    if (t < ncomp) {
        // component t: the electrons count negative; the nuclei in the order of the atoms
        double e = -red[t][0];
        if (with_nuc && with_nuc[k]) {
            const double* xyz = coords + (size_t)g * natm * 3;
            double O[3];
            gto_mom_origin(origin, g, O);
            const int px = gto_mom_pow(t, 0), py = gto_mom_pow(t, 1), pz = gto_mom_pow(t, 2);
            double n = 0.0;
            for (int a = 0; a < natm; ++a) {
                const double x = xyz[3 * a] - O[0], y = xyz[3 * a + 1] - O[1], z = xyz[3 * a + 2] - O[2];
                const double fx = px == 0 ? 1.0 : (px == 1 ? x : x * x), fy = py == 0 ? 1.0 : (py == 1 ? y : y * y),
                             fz = pz == 0 ? 1.0 : (pz == 1 ? z : z * z);
                n += charges[a] * (fx * fy * fz);
            }
            e += n;
        }
        out[((size_t)g * nd + k) * ncomp + t] = e;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------
namespace {
template <int LA, int LB>
int gto_mom_launch(gto_cls_t<LA, LB>, const gto_prep_t& p, int ncomp, const double* origin, double* moments)
{
    const int count = p.cnt[gto_cls(LA, LB)];
    if (count == 0) return 0;
    unsigned grid;
    if constexpr (LA == 2) {
        if (const int rc = gto_grid_wg(p.who, (long)count * p.batch, &grid)) return rc;
        hipLaunchKernelGGL((gto_mom_d_kernel<LA, LB>), dim3(grid), dim3(GTO_MOM_NT), 0, p.st, p.iw, p.shells, p.nshell,
                           count, p.coords, p.natm, p.batch, p.pairs, p.kp, p.nao, ncomp, origin, moments);
        OOVQE_CHECK_LAUNCH("gto_mom_d_kernel");
    } else {
        if (const int rc = gto_grid_split(p.who, (long)count * p.batch, &grid)) return rc;
        hipLaunchKernelGGL((gto_mom_kernel<LA, LB>), dim3(grid), dim3(GTO_NT), 0, p.st, p.iw, p.shells, p.nshell, count,
                           p.coords, p.natm, p.batch, p.pairs, p.kp, p.nao, ncomp, origin, moments);
        OOVQE_CHECK_LAUNCH("gto_mom_kernel");
    }
    return 0;
}
}  // namespace

extern "C" int oovqe_gto_moments_batch(int nshell, const int32_t* shells, int nprim_total, const double* exps,
                                       const double* coefs, int natm, const double* charges, int batch,
                                       const double* coords, int nao, int order, const double* origin,
                                       double* moments, double* work, oovqe_stream_t stream)
{
    const char* who = "oovqe_gto_moments_batch";
    OOVQE_REQUIRE(order >= 1 && order <= OOVQE_GTO_MAX_MOMENT, "%s: order = %d (1 .. %d)", who, order,
                  OOVQE_GTO_MAX_MOMENT);
    hipStream_t st = (hipStream_t)stream;
    gto_prep_t p;
    int rc = gto_prepare(who, OOVQE_GTO_MAX_L, nshell, shells, nprim_total, exps, coefs, natm, charges, batch, coords,
                         nao, nullptr, work, st, &p);
    if (rc != 0 || batch == 0) return rc;
    OOVQE_REQUIRE(moments, "%s: null pointer", who);
    const int ncomp = order == 1 ? 3 : GTO_MOM_NC;
    return gto_pairs_d_first([&](auto c) { return gto_mom_launch(c, p, ncomp, origin, moments); });
}

extern "C" int oovqe_gto_moments_expect_batch(const double* moments, int ncomp, int nao, int batch, const double* dens,
                                              int nd, int natm, const double* charges, const double* coords,
                                              const double* origin, const int32_t* with_nuc, double* out,
                                              oovqe_stream_t stream)
{
    const char* who = "oovqe_gto_moments_expect_batch";
    OOVQE_REQUIRE(ncomp == 3 || ncomp == GTO_MOM_NC, "%s: ncomp = %d (3 or %d)", who, ncomp, GTO_MOM_NC);
    OOVQE_REQUIRE(nao >= 1 && natm >= 1, "%s: nao = %d, natm = %d", who, nao, natm);
    OOVQE_REQUIRE(batch >= 0 && batch <= 65535 && nd >= 0, "%s: batch = %d (0 .. 65535), nd = %d", who, batch, nd);
    if (batch == 0 || nd == 0) return 0;
    OOVQE_REQUIRE(moments && dens && out && (!with_nuc || (charges && coords)), "%s: null pointer", who);
    hipLaunchKernelGGL(gto_mom_expect_kernel, dim3((unsigned)nd, (unsigned)batch), dim3(GTO_MOM_RT), 0,
                       (hipStream_t)stream, moments, ncomp, nao, dens, nd, natm, charges, coords, origin, with_nuc,
                       out);
    OOVQE_CHECK_LAUNCH("gto_mom_expect_kernel");
    return 0;
}
#endif  // GTO_MOMENTS_BODIES_ONLY
