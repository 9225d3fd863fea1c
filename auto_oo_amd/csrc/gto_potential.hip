// Electrostatic potential and field of a stack of geometries at arbitrary points (gfx950): every geometry g has its own
// M points r[g, m] and K density matrices D[g, k] (general: both (mu, nu) and (nu, mu) are read),
//
//   phi[g, k, m]  = (nuc_k) sum_A Z_A / |R_A - r_m|  -  sum_{mu nu} D[g, k, mu, nu] <mu| 1 / |r - r_m| |nu>
//   F[g, k, m, :] = - d phi[g, k, m] / d r_m                                                     (optional)
//
// over the functions of the integral kernels (s, p and d shells, both d forms).  The points are the parallel dimension,
// as the charges are in gto_charges.hip, and the pair data of gto_prepare is uniform across them.
//
//   gto_potential_kernel <field>   one workgroup of POT_NT lanes per (geometry, chunk of POT_NT points); a lane owns one
//       point.  The workgroup walks the pair classes ss, ps, pp, ds, dp, dd and their shell pairs in the order of the
//       class lists.  Per shell pair the K blocks of D (+ their transposes for two different shells) go to LDS once, and
//       the form of the d shells is folded into them there (sqrt 3, or the 5 -> 6 back-transform: the transpose of
//       gto_d_pass), so nothing per point ever meets a coefficient of a component.  Per primitive pair the lanes build
//       the Hermite densities rho^k_tuv = sum_ab D^k_ab E^ab_tuv in LDS together (an element is made by one lane, in
//       the order of the components); after a barrier every lane makes the Boys values and R_tuv(P - r) of ITS point in
//       registers, to order L (potential) or L + 1 (field: d/dr R_tuv = -R_{t+1,u,v}), and dots them with the K
//       densities.  The sums of a lane live in its own column of LDS [K][1 or 4][POT_NT], so no per-thread array is
//       indexed at run time; nobody else touches that column.  The nuclei are added last, in the order of the atoms.
//
// No atomics, no scratch, no records in the work buffer (it holds the pair data only).  A value depends on the shell
// table, its geometry, its density and its point alone: every product that meets a sum is written as an explicit fma, so
// the two instantiations round alike, and the Boys values come from order L + 1 in both.  Hence a (geometry, set, point)
// has the same bits wherever it stands in the stack, among the points and among the sets, on any stream, with or without
// the field.
// The bodies are __host__ __device__ functions of (chunk, geometry, lane, nlane): a CPU build
// (GTO_POTENTIAL_BODIES_ONLY: no kernel, no entry point) runs them with one lane per workgroup (chunks of one point), or
// with the lanes as host threads and GTO_HOST_BARRIER as the barrier.
#include "gto.h"

#define POT_NT 64                // lanes of a workgroup = points of a chunk (one wave)
#define POT_MAX 65535            // points per geometry
#define POT_KMAX OOVQE_GTO_GRAD_MAX_SETS
#define POT_NAB 36               // components of a dd pair
#define POT_NR 125               // (L + 1)^3 of a dd pair: the cube t, u, v <= L, of which t + u + v <= L is used

struct gto_pot_lds_t {
    double W[POT_KMAX * POT_NAB];           // [set][ca][cb] of the current shell pair
    double E[3 * 3 * 3 * 5];                // [dimension][i][j][t] of the current primitive pair
    double rho[POT_KMAX * POT_NR];          // [set][t][u][v]
};

// the transpose of gto_d_pass along one index of the weights of a shell pair: the weights of the functions of a d shell
// (5 real solid harmonics in the first 5 places of a fibre of 6, or 6 normalised Cartesian functions) become the weights
// of the 6 Cartesian components xx, xy, xz, yy, yz, zz with the radial part normalised for xx
__host__ __device__ __forceinline__ void gto_pot_d_back(double* a, int total, int stride, bool cartesian, int lane,
                                                        int nlane)
{
    const double r3 = 1.7320508075688772935;
    for (int i = lane; i < total; i += nlane) {
        if ((i / stride) % 6 != 0) continue;
        if (cartesian) {
            a[i + stride] *= r3;
            a[i + 2 * stride] *= r3;
            a[i + 4 * stride] *= r3;
        } else {
            const double w0 = a[i], w1 = a[i + stride], w2 = a[i + 2 * stride], w3 = a[i + 3 * stride],
                         w4 = a[i + 4 * stride];
            const double h = (0.5 * r3) * w4;
            a[i] = h - 0.5 * w2;                   // xx
            a[i + stride] = r3 * w0;               // xy
            a[i + 2 * stride] = r3 * w3;           // xz
            a[i + 3 * stride] = -0.5 * w2 - h;     // yy
            a[i + 4 * stride] = r3 * w1;           // yz
            a[i + 5 * stride] = w2;                // zz
        }
    }
    gto_sync();
}

// R^N_TUV as gto_R makes it, every product that meets a sum an explicit fma
template <int T, int U, int V, int N, int NF>
__host__ __device__ __forceinline__ double gto_pot_R(const double (&Fs)[NF], double X, double Y, double Z)
{
    if constexpr (T < 0 || U < 0 || V < 0) {
        return 0.0;
    } else if constexpr (T == 0 && U == 0 && V == 0) {
        return Fs[N];
    } else if constexpr (T == 0 && U == 0) {
        if constexpr (V > 1)
            return fma(Z, gto_pot_R<0, 0, V - 1, N + 1>(Fs, X, Y, Z), (double)(V - 1) * gto_pot_R<0, 0, V - 2, N + 1>(Fs, X, Y, Z));
        else
            return Z * gto_pot_R<0, 0, V - 1, N + 1>(Fs, X, Y, Z);
    } else if constexpr (T == 0) {
        if constexpr (U > 1)
            return fma(Y, gto_pot_R<0, U - 1, V, N + 1>(Fs, X, Y, Z), (double)(U - 1) * gto_pot_R<0, U - 2, V, N + 1>(Fs, X, Y, Z));
        else
            return Y * gto_pot_R<0, U - 1, V, N + 1>(Fs, X, Y, Z);
    } else {
        if constexpr (T > 1)
            return fma(X, gto_pot_R<T - 1, U, V, N + 1>(Fs, X, Y, Z), (double)(T - 1) * gto_pot_R<T - 2, U, V, N + 1>(Fs, X, Y, Z));
        else
            return X * gto_pot_R<T - 1, U, V, N + 1>(Fs, X, Y, Z);
    }
}

// the shell pairs of class (LA, LB) for the point (rx, ry, rz) of this lane: column `lane` of acc [nset][NC][nlane]
// receives - sum D <mu| 1 / |r - r_m| |nu> and, FIELD, minus its derivative in the point
template <int LA, int LB, bool FIELD>
__host__ __device__ __forceinline__ void gto_pot_class(int lane, int nlane, gto_pot_lds_t& s, double* __restrict__ acc,
                                                       const int* __restrict__ iw, const int* __restrict__ shells,
                                                       int nshell, int count, const double* __restrict__ xyz,
                                                       const double* __restrict__ pairs_g, int kp, int nao, int nset,
                                                       const double* __restrict__ dm_g, double rx, double ry, double rz)
{
    constexpr int NA = gto_ncomp(LA), NB = gto_ncomp(LB), NAB = NA * NB, L = LA + LB, D = L + 1, NR = D * D * D;
    constexpr int LR = L + (FIELD ? 1 : 0), NC = FIELD ? 4 : 1;
    constexpr int EJ = L + 1, EI = (LB + 1) * EJ, ED = (LA + 1) * EI;       // strides of s.E [3][LA + 1][LB + 1][L + 1]
    const long npair = (long)nshell * (nshell + 1) / 2;
    const size_t nn = (size_t)nao * nao;
    for (int k = 0; k < count; ++k) {
        const gto_pair_ref_t ab = gto_pair_ref(iw + nshell, gto_cls(LA, LB), k, npair, iw, shells, xyz, pairs_g, kp);
        // the weights of the pair of every set: D_ab + D_ba (one shell with itself: its block as it stands)
        const bool same = ab.sa == ab.sb;
        const int na = gto_nfunc(shells[4 * ab.sa + 1]), nb = gto_nfunc(shells[4 * ab.sb + 1]);
        for (int i = lane; i < nset * NAB; i += nlane) {
            const int ks = i / NAB, c = i - ks * NAB, ca = c / NB, cb = c - ca * NB;
            double w = 0.0;
            if (ca < na && cb < nb) {
                const double* d = dm_g + (size_t)ks * nn;
                const size_t mu = ab.oa + ca, nu = ab.ob + cb;
                w = same ? d[mu * nao + nu] : d[mu * nao + nu] + d[nu * nao + mu];
            }
            s.W[i] = w;
        }
        gto_sync();
        if (LA == 2) gto_pot_d_back(s.W, nset * NAB, NB, (shells[4 * ab.sa + 1] & OOVQE_GTO_CARTESIAN) != 0, lane, nlane);
        if (LB == 2) gto_pot_d_back(s.W, nset * NAB, 1, (shells[4 * ab.sb + 1] & OOVQE_GTO_CARTESIAN) != 0, lane, nlane);
        for (int kab = 0; kab < ab.nprim; ++kab) {
            const gto_prim_t pr = gto_load_prim(ab.data + (size_t)kab * GTO_PW, ab.swapped);
            for (int d = lane; d < 3; d += nlane) {
                double E[LA + 1][LB + 1][L + 1];
                const double q = gto_pick(ab.AB, d);
                gto_herm<LA, LB>(E, -pr.fb * q, pr.fa * q, pr.oo2p);
#pragma unroll
                for (int i = 0; i <= LA; ++i)
#pragma unroll
                    for (int j = 0; j <= LB; ++j)
#pragma unroll
                        for (int t = 0; t <= L; ++t) s.E[d * ED + i * EI + j * EJ + t] = E[i][j][t];
            }
            gto_sync();
            // rho^k_tuv = sum_ab W^k_ab E^ab_t E^ab_u E^ab_v: one lane per element, the components in their order
            for (int i = lane; i < nset * NR; i += nlane) {
                const int ks = i / NR, r = i - ks * NR, t = r / (D * D), u = (r / D) % D, v = r % D;
                if (t + u + v > L) continue;
                const double* w = s.W + ks * NAB;
                double x = 0.0;
                for (int c = 0; c < NAB; ++c) {
                    const int ca = c / NB, cb = c - ca * NB;
                    const double e = s.E[gto_pow(LA, ca, 0) * EI + gto_pow(LB, cb, 0) * EJ + t] *
                                     s.E[ED + gto_pow(LA, ca, 1) * EI + gto_pow(LB, cb, 1) * EJ + u] *
                                     s.E[2 * ED + gto_pow(LA, ca, 2) * EI + gto_pow(LB, cb, 2) * EJ + v];
                    x = fma(w[c], e, x);
                }
                s.rho[i] = x;
            }
            gto_sync();
            // this lane's point: Boys values from order L + 1 in both instantiations, R_tuv to order L or L + 1
            const double X = pr.P[0] - rx, Y = pr.P[1] - ry, Z = pr.P[2] - rz;
            double F[L + 2], Fs[LR + 1], R[LR + 1][LR + 1][LR + 1];
            gto_boys<L + 1>(pr.p * fma(X, X, fma(Y, Y, Z * Z)), F);
            double sc = -2.0 * GTO_PI / pr.p * pr.cck;
#pragma unroll
            for (int n = 0; n <= LR; ++n) { Fs[n] = sc * F[n]; sc *= -2.0 * pr.p; }
            static_for<(LR + 1) * (LR + 1) * (LR + 1)>([&](auto ic) {
                constexpr int i = decltype(ic)::value, t = i / ((LR + 1) * (LR + 1)), u = (i / (LR + 1)) % (LR + 1),
                              v = i % (LR + 1);
                if constexpr (t + u + v <= LR) R[t][u][v] = gto_pot_R<t, u, v, 0>(Fs, X, Y, Z);
            });
            for (int ks = 0; ks < nset; ++ks) {
                const double* rho = s.rho + ks * NR;
                double a0 = 0.0, ax = 0.0, ay = 0.0, az = 0.0;
                static_for<NR>([&](auto ic) {
                    constexpr int i = decltype(ic)::value, t = i / (D * D), u = (i / D) % D, v = i % D;
                    if constexpr (t + u + v <= L) {
                        const double x = rho[i];
                        a0 = fma(x, R[t][u][v], a0);
                        if constexpr (FIELD) {
                            ax = fma(x, R[t + 1][u][v], ax);
                            ay = fma(x, R[t][u + 1][v], ay);
                            az = fma(x, R[t][u][v + 1], az);
                        }
                    }
                });
                double* col = acc + (size_t)ks * NC * nlane + lane;
                col[0] += a0;
                if constexpr (FIELD) {
                    col[nlane] += ax;
                    col[2 * nlane] += ay;
                    col[3 * nlane] += az;
                }
            }
        }
        // (the weights of the next pair are written while slow lanes still read rho, never W: the last barrier above
        // is behind every read of W)
    }
}

// cnt: shell pairs per class (gto_prep_t::cnt); acc [nset][1 or 4][nlane]
template <bool FIELD>
__host__ __device__ __forceinline__ void gto_pot_body(int chunk, int g, int lane, int nlane, gto_pot_lds_t& s,
                                                      double* __restrict__ acc, const int* __restrict__ iw,
                                                      const int* __restrict__ shells, int nshell, int n_ss, int n_ps,
                                                      int n_pp, int n_ds, int n_dp, int n_dd,
                                                      const double* __restrict__ zat, int natm,
                                                      const double* __restrict__ coords,
                                                      const double* __restrict__ pairs, int kp, int nao, int nset,
                                                      const double* __restrict__ dm, int npoint,
                                                      const double* __restrict__ points, unsigned nuc_mask,
                                                      double* __restrict__ phi, double* __restrict__ field)
{
    constexpr int NC = FIELD ? 4 : 1;
    const long npair = (long)nshell * (nshell + 1) / 2;
    const double* xyz = coords + (size_t)g * natm * 3;
    const double* pairs_g = pairs + (size_t)g * npair * kp * GTO_PW;
    const double* dm_g = dm + (size_t)g * nset * nao * nao;
    // (a lane beyond the last point runs along with point zero and stores nothing)
    const int m = chunk * nlane + lane;
    const bool mine = m < npoint;
    const double* r = points + ((size_t)g * npoint + (mine ? m : 0)) * 3;
    const double rx = r[0], ry = r[1], rz = r[2];
    for (int i = 0; i < nset * NC; ++i) acc[(size_t)i * nlane + lane] = 0.0;
    gto_pot_class<0, 0, FIELD>(lane, nlane, s, acc, iw, shells, nshell, n_ss, xyz, pairs_g, kp, nao, nset, dm_g, rx, ry, rz);
    gto_pot_class<1, 0, FIELD>(lane, nlane, s, acc, iw, shells, nshell, n_ps, xyz, pairs_g, kp, nao, nset, dm_g, rx, ry, rz);
    gto_pot_class<1, 1, FIELD>(lane, nlane, s, acc, iw, shells, nshell, n_pp, xyz, pairs_g, kp, nao, nset, dm_g, rx, ry, rz);
    gto_pot_class<2, 0, FIELD>(lane, nlane, s, acc, iw, shells, nshell, n_ds, xyz, pairs_g, kp, nao, nset, dm_g, rx, ry, rz);
    gto_pot_class<2, 1, FIELD>(lane, nlane, s, acc, iw, shells, nshell, n_dp, xyz, pairs_g, kp, nao, nset, dm_g, rx, ry, rz);
    gto_pot_class<2, 2, FIELD>(lane, nlane, s, acc, iw, shells, nshell, n_dd, xyz, pairs_g, kp, nao, nset, dm_g, rx, ry, rz);
    if (!mine) return;
    // the nuclei in the order of the atoms (a point ON a nucleus: inf, and NaN in the field)
    double pn = 0.0, fx = 0.0, fy = 0.0, fz = 0.0;
    if (nuc_mask != 0u) {
        for (int a = 0; a < natm; ++a) {
            const double dx = rx - xyz[3 * a], dy = ry - xyz[3 * a + 1], dz = rz - xyz[3 * a + 2];
            const double r2 = fma(dx, dx, fma(dy, dy, dz * dz));
            const double d = sqrt(r2);
            pn += zat[a] / d;
            if constexpr (FIELD) {
                const double f = zat[a] / (r2 * d);
                fx = fma(f, dx, fx); fy = fma(f, dy, fy); fz = fma(f, dz, fz);
            }
        }
    }
    for (int ks = 0; ks < nset; ++ks) {
        const bool nuc = (nuc_mask >> ks) & 1u;
        const double* col = acc + (size_t)ks * NC * nlane + lane;
        const size_t o = ((size_t)g * nset + ks) * npoint + m;
        phi[o] = nuc ? pn + col[0] : col[0];
        if constexpr (FIELD) {
            field[3 * o] = nuc ? fx + col[nlane] : col[nlane];
            field[3 * o + 1] = nuc ? fy + col[2 * nlane] : col[2 * nlane];
            field[3 * o + 2] = nuc ? fz + col[3 * nlane] : col[3 * nlane];
        }
    }
}

#ifndef GTO_POTENTIAL_BODIES_ONLY
template <bool FIELD>
__global__ __launch_bounds__(POT_NT) void gto_potential_kernel(const int* __restrict__ iw, const int* __restrict__ shells,
                                                               int nshell, int n_ss, int n_ps, int n_pp, int n_ds,
                                                               int n_dp, int n_dd, const double* __restrict__ zat,
                                                               int natm, const double* __restrict__ coords,
                                                               const double* __restrict__ pairs, int kp, int nao,
                                                               int nset, const double* __restrict__ dm, int npoint,
                                                               const double* __restrict__ points, unsigned nuc_mask,
                                                               double* __restrict__ phi, double* __restrict__ field)
{
    __shared__ gto_pot_lds_t s;
    extern __shared__ double acc[];             // [nset][1 or 4][POT_NT]: a lane reads and writes its own column only
    gto_pot_body<FIELD>((int)blockIdx.x, (int)blockIdx.y, (int)threadIdx.x, POT_NT, s, acc, iw, shells, nshell, n_ss, n_ps,
                        n_pp, n_ds, n_dp, n_dd, zat, natm, coords, pairs, kp, nao, nset, dm, npoint, points, nuc_mask,
                        phi, field);
}

// ---- host side --------------------------------------------------------------------------------------------------------
namespace {
int pot_check(const char* who, int batch, int nset)
{
    OOVQE_REQUIRE(batch >= 0 && batch <= 65535, "%s: batch = %d (at most 65535 geometries per call)", who, batch);
    OOVQE_REQUIRE(nset >= 1 && nset <= POT_KMAX, "%s: nset = %d (1 .. %d density sets per geometry)", who, nset, POT_KMAX);
    return 0;
}
}  // namespace

extern "C" int64_t oovqe_gto_potential_work_size(int nshell, int max_nprim, int natm, int batch, int nset)
{
    const char* who = "oovqe_gto_potential_work_size";
    if (gto_check_sizes(who, nshell, max_nprim, batch) != 0) return OOVQE_ERR_ARG;
    OOVQE_REQUIRE(natm >= 1, "%s: natm = %d", who, natm);
    if (pot_check(who, batch, nset) != 0) return OOVQE_ERR_ARG;
    return gto_work_base(nshell, max_nprim, batch);
}

extern "C" int oovqe_gto_potential_batch(int nshell, const int32_t* shells, int nprim_total, const double* exps,
                                         const double* coefs, int natm, const double* charges, int batch,
                                         const double* coords, int nao, int nset, const double* dm, int npoint,
                                         const double* points, unsigned nuc_mask, double* phi, double* field,
                                         double* work, oovqe_stream_t stream)
{
    const char* who = "oovqe_gto_potential_batch";
    hipStream_t st = (hipStream_t)stream;
    int rc = pot_check(who, batch, nset);
    if (rc != 0) return rc;
    OOVQE_REQUIRE(npoint >= 1 && npoint <= POT_MAX, "%s: npoint = %d (1 .. %d points per geometry)", who, npoint, POT_MAX);
    OOVQE_REQUIRE((nuc_mask >> nset) == 0u,"%s: nuc_mask = 0x%x has bits beyond the %d sets", who, nuc_mask,
                  nset);
    OOVQE_REQUIRE(batch == 0 || (dm && points && phi), "%s: null pointer", who);
    gto_prep_t p;
    rc = gto_prepare(who, OOVQE_GTO_MAX_L, nshell, shells, nprim_total, exps, coefs, natm, charges, batch, coords, nao,
                     nullptr, work, st, &p);
    if (rc != 0 || batch == 0) return rc;
    const int nchunk = (npoint + POT_NT - 1) / POT_NT;
    const size_t lds = (size_t)nset * (field ? 4 : 1) * POT_NT * sizeof(double);
    const dim3 grid((unsigned)nchunk, (unsigned)batch);
    if (field) {
        hipLaunchKernelGGL(gto_potential_kernel<true>, grid, dim3(POT_NT), lds, st, p.iw, shells, nshell,
                           p.cnt[gto_cls(0, 0)], p.cnt[gto_cls(1, 0)], p.cnt[gto_cls(1, 1)], p.cnt[gto_cls(2, 0)],
                           p.cnt[gto_cls(2, 1)], p.cnt[gto_cls(2, 2)], charges, natm, coords, p.pairs, p.kp, nao, nset,
                           dm, npoint, points, nuc_mask, phi, field);
    } else {
        hipLaunchKernelGGL(gto_potential_kernel<false>, grid, dim3(POT_NT), lds, st, p.iw, shells, nshell,
                           p.cnt[gto_cls(0, 0)], p.cnt[gto_cls(1, 0)], p.cnt[gto_cls(1, 1)], p.cnt[gto_cls(2, 0)],
                           p.cnt[gto_cls(2, 1)], p.cnt[gto_cls(2, 2)], charges, natm, coords, p.pairs, p.kp, nao, nset,
                           dm, npoint, points, nuc_mask, phi, field);
    }
    OOVQE_CHECK_LAUNCH("gto_potential_kernel");
    return 0;
}
#endif  // GTO_POTENTIAL_BODIES_ONLY
