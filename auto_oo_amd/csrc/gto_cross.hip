// AO overlap between two geometries of a stack (gfx950).
//
//   S_ab[p][mu][nu] = <chi_mu at R_a(p) | chi_nu at R_b(p)>,   p = 0 .. npair - 1
//
// over the basis functions of `overlap` (gto.hip / gto_d.hip: the same shell tables, order and normalisation).  The
// matrix is not symmetric, so every one of the nshell^2 ordered shell pairs (i of the bra geometry, j of the ket
// geometry) is an item of its own, a shell paired with its own displaced copy included.  The centres of a pair come
// from two geometries, so the pair data of gto_pair_kernel do not apply: p, P, c_a c_b exp(-mu |AB|^2) are formed here,
// by the same expressions.  Per primitive pair and dimension the overlap is E_0 of gto_herm (the order-0 term of
// gto_moments.hip) in units of sqrt(pi / p).  No Boys function, no atomics, no scratch, no work buffer.
//
// An item is computed with the shell of higher l first (ties: the bra shell first), as the kernels of a single geometry
// do, and stored transposed when that is the ket shell: six templates serve the nine ordered classes.  Every launch
// runs over all items and an item whose class is not the launch's leaves at once.
//
//   gto_cross_kernel   <la, lb>, la, lb <= 1: one item per group of GTO_SPLIT lanes, everything in registers (the style
//                      of gto_mom_kernel); the partial sums are added by a butterfly
//   gto_cross_d_kernel <2, lb>: a workgroup owns one item; E of one dimension per lane, kept in LDS; every accumulator is
//                      owned by one lane and adds its primitive pairs in their stored order; the d components are
//                      finished in LDS by gto_d_pass before the stores (the style of gto_mom_d_kernel)
//
// The order of every sum is fixed by the item alone: a pair has the same bits wherever it stands in the list, alone, or
// on another stream.  The bodies are __host__ __device__ functions: a CPU build (GTO_CROSS_BODIES_ONLY: no kernel, no
// entry point) runs them with one lane per group / workgroup.
#include "gto.h"

#define GTO_CROSS_NT 64          // lanes of a workgroup of the d classes

struct gto_cross_ref_t {
    int oa, ob;                 // AO offsets of the first and the second shell
    int pa, pb;                 // their first primitives
    int na, nb;                 // their numbers of primitives
    int fa, fb;                 // their l fields
    bool bra_first;             // the first shell is the bra's (row index); else the result is stored transposed
    double AB[3];               // A - B
};

// item (p, i, j) of the launch <LA, LB>: false when the ordered pair (i, j) belongs to another class
template <int LA, int LB>
__host__ __device__ __forceinline__ bool gto_cross_item(long item, const int* __restrict__ shells, int nshell,
                                                        const double* __restrict__ coords_a,
                                                        const double* __restrict__ coords_b, int natm,
                                                        gto_cross_ref_t& r, int& p)
{
    const long per = (long)nshell * nshell;
    p = (int)(item / per);
    const int ij = (int)(item - (long)p * per), i = ij / nshell, j = ij - i * nshell;
    const int li = gto_l_of(shells[4 * i + 1]), lj = gto_l_of(shells[4 * j + 1]);
    r.bra_first = li >= lj;
    const int sa = r.bra_first ? i : j, sb = r.bra_first ? j : i;
    r.fa = shells[4 * sa + 1];
    r.fb = shells[4 * sb + 1];
    if (gto_l_of(r.fa) != LA || gto_l_of(r.fb) != LB) return false;
    r.na = shells[4 * sa + 2]; r.pa = shells[4 * sa + 3];
    r.nb = shells[4 * sb + 2]; r.pb = shells[4 * sb + 3];
    int oa = 0, ob = 0;
    for (int s = 0; s < nshell; ++s) {
        const int nf = gto_nfunc(shells[4 * s + 1]);
        oa += s < sa ? nf : 0;
        ob += s < sb ? nf : 0;
    }
    r.oa = oa; r.ob = ob;
    const double* xa = coords_a + (size_t)p * natm * 3;
    const double* xb = coords_b + (size_t)p * natm * 3;
    const double* A = (r.bra_first ? xa : xb) + 3 * shells[4 * sa];
    const double* B = (r.bra_first ? xb : xa) + 3 * shells[4 * sb];
#pragma unroll
    for (int d = 0; d < 3; ++d) r.AB[d] = A[d] - B[d];
    return true;
}

// primitive pair k of an item, by the expressions of gto_pair_body
__host__ __device__ __forceinline__ gto_prim_t gto_cross_prim(const gto_cross_ref_t& r, int k,
                                                              const double* __restrict__ exps,
                                                              const double* __restrict__ coefs)
{
    const int ka = k / r.nb, kb = k - ka * r.nb;
    const double a = exps[r.pa + ka], b = exps[r.pb + kb];
    const double ca = coefs[r.pa + ka], cb = coefs[r.pb + kb];
    gto_prim_t q;
    q.p = a + b;
    const double mu = a * b / q.p;
    q.P[0] = q.P[1] = q.P[2] = 0.0;             // (the centre of the product is not read by the overlap)
    q.cck = ca * cb * exp(-mu * (r.AB[0] * r.AB[0] + r.AB[1] * r.AB[1] + r.AB[2] * r.AB[2]));
    q.oo2p = 0.5 / q.p;
    q.fa = a / q.p;
    q.fb = b / q.p;
    return q;
}

__host__ __device__ __forceinline__ void gto_cross_store(double* __restrict__ out, int nao, const gto_cross_ref_t& r,
                                                         int ca, int cb, double x)
{
    const int mu = r.oa + ca, nu = r.ob + cb;
    if (mu < nao && nu < nao) out[r.bra_first ? (size_t)mu * nao + nu : (size_t)nu * nao + mu] = x;
}

// ---- classes ss, ps, pp ----------------------------------------------------------------------------------------------
template <int LA, int LB, int SPLIT>
__host__ __device__ __forceinline__ void gto_cross_body(long tid, const int* __restrict__ shells, int nshell,
                                                        const double* __restrict__ exps,
                                                        const double* __restrict__ coefs, int natm, int npair,
                                                        const double* __restrict__ coords_a,
                                                        const double* __restrict__ coords_b, int nao,
                                                        double* __restrict__ out)
{
    constexpr int NA = gto_ncomp(LA), NB = gto_ncomp(LB);
    const int sub = (int)(tid % SPLIT);
    tid /= SPLIT;
    if (tid >= (long)npair * nshell * nshell) return;
    gto_cross_ref_t r;
    int p;
    if (!gto_cross_item<LA, LB>(tid, shells, nshell, coords_a, coords_b, natm, r, p)) return;
    double acc[NA * NB];
#pragma unroll
    for (int i = 0; i < NA * NB; ++i) acc[i] = 0.0;
    const int nprim = r.na * r.nb;
    for (int k = sub; k < nprim; k += SPLIT) {
        const gto_prim_t pr = gto_cross_prim(r, k, exps, coefs);
        double E[3][LA + 1][LB + 1][LA + LB + 1];
#pragma unroll
        for (int d = 0; d < 3; ++d) gto_herm<LA, LB>(E[d], -pr.fb * r.AB[d], pr.fa * r.AB[d], pr.oo2p);
        const double pop = GTO_PI / pr.p;
        const double fS = pr.cck * pop * sqrt(pop);
        static_for<NA * NB>([&](auto cabc) {
            constexpr int cab = decltype(cabc)::value, ca = cab / NB, cb = cab % NB;
            acc[cab] += fS * (E[0][gto_pow(LA, ca, 0)][gto_pow(LB, cb, 0)][0] *
                              E[1][gto_pow(LA, ca, 1)][gto_pow(LB, cb, 1)][0] *
                              E[2][gto_pow(LA, ca, 2)][gto_pow(LB, cb, 2)][0]);
        });
    }
#pragma unroll
    for (int i = 0; i < NA * NB; ++i) acc[i] = gto_group_sum<SPLIT>(acc[i]);
    // (after the butterfly every lane of the group holds every value: lane `sub` stores every SPLIT-th of them)
    double* o = out + (size_t)p * nao * nao;
    static_for<NA * NB>([&](auto cabc) {
        constexpr int cab = decltype(cabc)::value, ca = cab / NB, cb = cab % NB;
        if (cab % SPLIT == sub) gto_cross_store(o, nao, r, ca, cb, acc[cab]);
    });
}

// ---- classes ds, dp, dd ----------------------------------------------------------------------------------------------
template <int LA, int LB> struct gto_cross_lds_t {
    static constexpr int NAB = gto_ncomp(LA) * gto_ncomp(LB);
    double acc[NAB];                               // [ca][cb]
    double E[3][LA + 1][LB + 1][LA + LB + 1];
};

template <int LA, int LB>
__host__ __device__ __forceinline__ void gto_cross_d_body(long grp, int lane, int nlane, gto_cross_lds_t<LA, LB>& s,
                                                          const int* __restrict__ shells, int nshell,
                                                          const double* __restrict__ exps,
                                                          const double* __restrict__ coefs, int natm, int npair,
                                                          const double* __restrict__ coords_a,
                                                          const double* __restrict__ coords_b, int nao,
                                                          double* __restrict__ out)
{
    static_assert(LA == 2 && LB <= 2, "the classes with a d shell");
    constexpr int NB = gto_ncomp(LB), NAB = gto_cross_lds_t<LA, LB>::NAB;
    if (grp >= (long)npair * nshell * nshell) return;
    gto_cross_ref_t r;
    int p;
    // (the same answer in every lane of the workgroup: nobody waits at a barrier for a lane that has left)
    if (!gto_cross_item<LA, LB>(grp, shells, nshell, coords_a, coords_b, natm, r, p)) return;
    for (int it = lane; it < NAB; it += nlane) s.acc[it] = 0.0;
    gto_sync();
    const int nprim = r.na * r.nb;
    for (int k = 0; k < nprim; ++k) {
        const gto_prim_t pr = gto_cross_prim(r, k, exps, coefs);
        for (int d = lane; d < 3; d += nlane) {
            double E[LA + 1][LB + 1][LA + LB + 1];
            const double q = gto_pick(r.AB, d);
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
        for (int it = lane; it < NAB; it += nlane) {
            const int ca = it / NB, cb = it - ca * NB;
            s.acc[it] += fS * (s.E[0][gto_pow(LA, ca, 0)][gto_pow(LB, cb, 0)][0] *
                               s.E[1][gto_pow(LA, ca, 1)][gto_pow(LB, cb, 1)][0] *
                               s.E[2][gto_pow(LA, ca, 2)][gto_pow(LB, cb, 2)][0]);
        }
        gto_sync();
    }
    // the form of the d shells (the flag of the l field), one index after the other
    int na = gto_ncomp(LA), nb = NB;
    {
        const bool cart = (r.fa & OOVQE_GTO_CARTESIAN) != 0;
        gto_d_pass(s.acc, NAB, NB, cart, lane, nlane);
        na = cart ? 6 : 5;
    }
    if (LB == 2) {
        const bool cart = (r.fb & OOVQE_GTO_CARTESIAN) != 0;
        gto_d_pass(s.acc, NAB, 1, cart, lane, nlane);
        nb = cart ? 6 : 5;
    }
    double* o = out + (size_t)p * nao * nao;
    for (int it = lane; it < NAB; it += nlane) {
        const int ca = it / NB, cb = it - ca * NB;
        if (ca < na && cb < nb) gto_cross_store(o, nao, r, ca, cb, s.acc[it]);
    }
}

#ifndef GTO_CROSS_BODIES_ONLY
template <int LA, int LB>
__global__ __launch_bounds__(GTO_NT) void gto_cross_kernel(const int* __restrict__ shells, int nshell,
                                                           const double* __restrict__ exps,
                                                           const double* __restrict__ coefs, int natm, int npair,
                                                           const double* __restrict__ coords_a,
                                                           const double* __restrict__ coords_b, int nao,
                                                           double* __restrict__ out)
{
    gto_cross_body<LA, LB, GTO_SPLIT>((long)blockIdx.x * GTO_NT + threadIdx.x, shells, nshell, exps, coefs, natm, npair,
                                      coords_a, coords_b, nao, out);
}

template <int LA, int LB>
__global__ __launch_bounds__(GTO_CROSS_NT) void gto_cross_d_kernel(const int* __restrict__ shells, int nshell,
                                                                   const double* __restrict__ exps,
                                                                   const double* __restrict__ coefs, int natm,
                                                                   int npair, const double* __restrict__ coords_a,
                                                                   const double* __restrict__ coords_b, int nao,
                                                                   double* __restrict__ out)
{
    __shared__ gto_cross_lds_t<LA, LB> s;
    gto_cross_d_body<LA, LB>((long)blockIdx.x, (int)threadIdx.x, GTO_CROSS_NT, s, shells, nshell, exps, coefs, natm,
                             npair, coords_a, coords_b, nao, out);
}

// ---- host side ----------------------------------------------------------------------------------------------------
namespace {
struct gto_cross_launch_t {
    const char* who; const int* shells; int nshell; const int* cnt; const double* exps; const double* coefs; int natm;
    int npair; const double* coords_a; const double* coords_b; int nao; double* out; hipStream_t st;
};

template <int LA, int LB> int gto_cross_launch(gto_cls_t<LA, LB>, const gto_cross_launch_t& a)
{
    if (a.cnt[gto_cls(LA, LB)] == 0) return 0;
    const long items = (long)a.npair * a.nshell * a.nshell;
    unsigned grid;
    if constexpr (LA == 2) {
        if (const int rc = gto_grid_wg(a.who, items, &grid)) return rc;
        hipLaunchKernelGGL((gto_cross_d_kernel<LA, LB>), dim3(grid), dim3(GTO_CROSS_NT), 0, a.st, a.shells, a.nshell,
                           a.exps, a.coefs, a.natm, a.npair, a.coords_a, a.coords_b, a.nao, a.out);
        OOVQE_CHECK_LAUNCH("gto_cross_d_kernel");
    } else {
        if (const int rc = gto_grid_split(a.who, items, &grid)) return rc;
        hipLaunchKernelGGL((gto_cross_kernel<LA, LB>), dim3(grid), dim3(GTO_NT), 0, a.st, a.shells, a.nshell, a.exps,
                           a.coefs, a.natm, a.npair, a.coords_a, a.coords_b, a.nao, a.out);
        OOVQE_CHECK_LAUNCH("gto_cross_kernel");
    }
    return 0;
}
}  // namespace

extern "C" int oovqe_gto_cross_overlap_batch(int nshell, const int32_t* shells, int nprim_total, const double* exps,
                                             const double* coefs, int natm, int npair, const double* coords_a,
                                             const double* coords_b, int nao, double* out, oovqe_stream_t stream)
{
    const char* who = "oovqe_gto_cross_overlap_batch";
    hipStream_t st = (hipStream_t)stream;
    OOVQE_REQUIRE(nshell >= 1 && nshell <= OOVQE_GTO_MAX_SHELL, "%s: nshell = %d (1 .. %d)", who, nshell,
                  OOVQE_GTO_MAX_SHELL);
    OOVQE_REQUIRE(npair >= 0 && natm >= 1 && nprim_total >= 1, "%s: npair = %d, natm = %d, nprim_total = %d", who,
                  npair, natm, nprim_total);
    if (npair == 0) return 0;
    OOVQE_REQUIRE(shells && exps && coefs && coords_a && coords_b && out, "%s: null pointer", who);
    // the shell table is read back and checked as gto_prepare does it (every l this library has is served here): the
    // limits are enforced with a return code, before anything is launched
    std::vector<int32_t> tab;
    const int rc = gto_read_shells(who, OOVQE_GTO_MAX_L, nshell, shells, nprim_total, natm, nao, st, &tab);
    if (rc != 0) return rc;
    int cnt[GTO_NCLS], nl[GTO_LMAX + 1] = {0, 0, 0};
    for (int s = 0; s < nshell; ++s) nl[gto_l_of(tab[4 * s + 1])] += 1;
    for (int la = 0; la <= GTO_LMAX; ++la)
        for (int lb = 0; lb <= la; ++lb) cnt[gto_cls(la, lb)] = nl[la] * nl[lb];
    const gto_cross_launch_t a = {who, shells, nshell, cnt, exps, coefs, natm, npair, coords_a, coords_b, nao, out, st};
    return gto_pairs_d_first([&](auto c) { return gto_cross_launch(c, a); });
}
#endif  // GTO_CROSS_BODIES_ONLY
