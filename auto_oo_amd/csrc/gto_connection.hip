// One-sided overlap-derivative contraction of a stack of geometries for SEVERAL matrices per geometry (gfx950):
//
//   out[g, k, A, :] = sum over mu, and nu on atom A, of D[g,k,mu,nu] <chi_mu | grad_A chi_nu>
//
// the orbital-connection term of a derivative coupling, Da . T^A with T^A[mu,nu] = <chi_mu | d chi_nu / dR_A>.  D is
// a general matrix: both D[mu,nu] and D[nu,mu] are read.
//
// The kernel is gto_grad_sets_one_kernel reduced to its overlap part -- the same pair data, class lists, GTO_SPLIT lane
// groups, per-set accumulators in LDS ([set][6][lane]), one record per (pair, set), the reduction of
// gto_grad_reduce_kernel, no floating-point atomics -- and what it forms per component is that kernel's dS[d], the
// derivative of the pair overlap <mu|nu> with respect to the centre of the FIRST shell, dS[d] = <d_A mu | nu>.  What
// is new is where it goes.  For the shell pair (a on A, b on B), mu in a, nu in b:
//
//   <mu | grad_B nu> = -dS      (the overlap depends on A - B only)   -> atom B receives  -sum D[mu,nu] dS[mu,nu]
//   <nu | grad_A mu> = +dS                                            -> atom A receives  +sum D[nu,mu] dS[mu,nu]
//
// Pairs on ONE atom are not skipped: dS is the derivative with respect to the centre of mu alone, which does not
// vanish at A = B (<s | d p> on one centre), and both contributions land on that atom.  A shell paired with itself
// holds every ordered (mu, nu) in its first sum already; the second is left out.
//
// The sets of a tile are handled by a loop with a run-time count, each set with accumulators of its own, so a set's
// bits depend neither on how many sets share its tile nor on its place among them.
#include "gto_grad.h"

#define CONN_SETS_TILE OOVQE_GTO_GRAD_SETS_TILE

// records: [geometry][set][pair of the class lists, ss | ps | pp]
template <int LA, int LB>
__global__ __launch_bounds__(GTO_NT) void gto_connection_kernel(
    const int* __restrict__ iw, const int* __restrict__ shells, int nshell, int count, int natm,
    const double* __restrict__ coords, int batch, const double* __restrict__ pairs, int kp, int nao, int nset, int k0,
    int nk, const double* __restrict__ dm, double* __restrict__ rec, long rec_off, long nrec)
{
    constexpr int NA = gto_ncomp(LA), NB = gto_ncomp(LB), NAB = NA * NB;
    __shared__ double Wl[GTO_NT / GTO_SPLIT][CONN_SETS_TILE][2][NAB];      // [.][set][0: D[mu,nu], 1: D[nu,mu]][component]
    __shared__ double Al[CONN_SETS_TILE * 6 * GTO_NT];
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
    const double second = (ab.sa == ab.sb) ? 0.0 : 1.0;
    for (int c = sub; c < nk * NAB; c += GTO_SPLIT) {
        const int ks = c / NAB, cm = c - ks * NAB;
        const size_t base = ((size_t)g * nset + k0 + ks) * nao * nao;
        const size_t mu = ab.oa + cm / NB, nu = ab.ob + cm % NB;
        Wl[grp][ks][0][cm] = dm[base + mu * nao + nu];
        Wl[grp][ks][1][cm] = second * dm[base + nu * nao + mu];
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const volatile double* wl = &Wl[grp][0][0][0];
    double* acc = Al + threadIdx.x;
    for (int ks = 0; ks < nk; ++ks)
        for (int d = 0; d < 6; ++d) acc[(ks * 6 + d) * GTO_NT] = 0.0;
    for (int kab = sub; kab < ab.nprim; kab += GTO_SPLIT) {
        const gto_prim_t pr = gto_load_prim(ab.data + (size_t)kab * GTO_PW, ab.swapped);
        double E[3][LA + 2][LB + 1][LA + LB + 2];
#pragma unroll
        for (int d = 0; d < 3; ++d) gto_herm<LA + 1, LB>(E[d], -pr.fb * ab.AB[d], pr.fa * ab.AB[d], pr.oo2p);
        const double a = pr.fa * pr.p;
        const double pop = GTO_PI / pr.p;
        const double fS = pr.cck * pop * sqrt(pop);
        static_for<NAB>([&](auto cc) {
            constexpr int c = decltype(cc)::value, ca = c / NB, cb = c % NB;
            double s1[3], ds[3], dS[3];
            static_for<3>([&](auto dc) {
                constexpr int d = decltype(dc)::value;
                constexpr int i = gto_pow(LA, ca, d), j = gto_pow(LB, cb, d);
                s1[d] = gto_ovl1<i, j>(E[d]);
                ds[d] = 2.0 * a * gto_ovl1<i + 1, j>(E[d]) - (double)i * gto_ovl1<i - 1, j>(E[d]);
            });
            static_for<3>([&](auto dc) {
                constexpr int d = decltype(dc)::value, e = (d + 1) % 3, f = (d + 2) % 3;
                dS[d] = fS * (ds[d] * s1[e] * s1[f]);
            });
#pragma nounroll
            for (int ks = 0; ks < nk; ++ks) {
                const double wb = wl[(ks * 2 + 0) * NAB + c], wa = wl[(ks * 2 + 1) * NAB + c];
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    acc[(ks * 6 + d) * GTO_NT] += wa * dS[d];
                    acc[(ks * 6 + 3 + d) * GTO_NT] -= wb * dS[d];
                }
            }
        });
    }
    for (int ks = 0; ks < nk; ++ks) {
        double v[12];
#pragma unroll
        for (int d = 0; d < 6; ++d) {
            v[d] = gto_group_sum<GTO_SPLIT>(acc[(ks * 6 + d) * GTO_NT]);
            v[6 + d] = 0.0;
        }
        if (sub == 0)
            grad_store(rec + (((size_t)g * nset + k0 + ks) * nrec + rec_off + k) * GRAD_REC, atA, atB, -1, -1, v);
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------
extern "C" int64_t oovqe_gto_overlap_connection_work_size(int nshell, int max_nprim, int natm, int batch, int nset)
{
    const char* who = "oovqe_gto_overlap_connection_work_size";
    if (gto_check_sizes(who, nshell, max_nprim, batch) != 0) return OOVQE_ERR_ARG;
    OOVQE_REQUIRE(natm >= 1, "%s: natm = %d", who, natm);
    if (grad_check_nset(who, nset) != 0) return OOVQE_ERR_ARG;
    const int64_t npair = (int64_t)nshell * (nshell + 1) / 2;
    return gto_work_base(nshell, max_nprim, batch) + (int64_t)batch * nset * npair * GRAD_REC;
}

namespace {
template <int LA, int LB>
int conn_launch(gto_cls_t<LA, LB>, const gto_prep_t& p, int nset, int k0, int nk, const double* dm, long& off)
{
    const int count = p.cnt[gto_cls(LA, LB)];
    if (count == 0) return 0;
    unsigned grid;
    if (const int rc = gto_grid_split(p.who, (long)count * p.batch, &grid)) return rc;
    hipLaunchKernelGGL((gto_connection_kernel<LA, LB>), dim3(grid), dim3(GTO_NT), 0, p.st, p.iw, p.shells, p.nshell, count,
                       p.natm, p.coords, p.batch, p.pairs, p.kp, p.nao, nset, k0, nk, dm, p.rec, off, p.npair());
    OOVQE_CHECK_LAUNCH("gto_connection_kernel");
    off += count;
    return 0;
}
}  // namespace

extern "C" int oovqe_gto_overlap_connection_batch(int nshell, const int32_t* shells, int nprim_total, const double* exps,
                                                  const double* coefs, int natm, const double* charges, int batch,
                                                  const double* coords, int nao, int nset, const double* dm,
                                                  double* out, double* work, oovqe_stream_t stream)
{
    const char* who = "oovqe_gto_overlap_connection_batch";
    hipStream_t st = (hipStream_t)stream;
    gto_prep_t p;
    if (grad_check_nset(who, nset) != 0) return OOVQE_ERR_ARG;
    OOVQE_REQUIRE(batch <= 65535, "%s: batch = %d (at most 65535 geometries per call)", who, batch);
    // (a table with l = 2 is refused here, before any launch, as by oovqe_gto_gradient_batch)
    int rc = gto_prepare(who, 1, nshell, shells, nprim_total, exps, coefs, natm, charges, batch, coords, nao, nullptr, work,
                         st, &p);
    if (rc != 0 || batch == 0) return rc;
    OOVQE_REQUIRE(dm && out, "%s: null pointer", who);
    const long npair = p.npair();
    // the sets spread evenly over the fewest tiles, as in oovqe_gto_gradient_sets_batch
    rc = grad_for_tiles(nset, CONN_SETS_TILE, [&](int k0, int nk) {
        long off = 0;
        const int rt = gto_sp_pairs([&](auto c) { return conn_launch(c, p, nset, k0, nk, dm, off); });
        if (rt == 0 && off != npair) {
            oovqe_set_error("%s: %ld pair records of %ld", who, off, npair);
            return (int)OOVQE_ERR_SIZE;
        }
        return rt;
    });
    if (rc != 0) return rc;
    // every (geometry, set) is a row of gto_grad_reduce_kernel: its records summed in that kernel's fixed order
    return gto_grad_reduce_launch(p.rec, npair, charges, natm, coords, 0, (long)batch * nset, out, st);
}
