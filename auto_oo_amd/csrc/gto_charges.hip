// Point-charge embedding of a stack of geometries (gfx950): every geometry g has its own cloud of M classical charges
// q[g, k] at r[g, k].  Two things are computed, both with the charges as the parallel dimension and the pair data of
// gto_prepare uniform across them:
//
//   V_ext[g, mu, nu] = - sum_k q[g, k] <mu| 1 / |r - r[g, k]| |nu>                 (all pair classes ss .. dd)
//   gA[g, A, :] = sum D[g] . dV_ext / dR_A,   gQ[g, k, :] = sum D[g] . dV_ext / dr_k      (s and p shells)
//
//   gto_charge_op_kernel <la, lb>   one workgroup of CHG_NT lanes per (geometry, shell pair).  The operator is linear
//       in the Hermite Coulomb integrals, V = sum_tuv E_tuv sum_k q_k R_tuv(P - r_k), so a lane only ever makes the
//       Boys values and R_tuv of ITS charges (k = lane, lane + CHG_NT, ...) and adds them up in registers, per
//       primitive pair.  The lanes' sums are added by a butterfly inside each wave and in a fixed order over the
//       waves; the Hermite coefficients meet the sum once per primitive pair, the d forms (sqrt 3, 6 -> 5) once
//       per shell pair.  Nothing per charge is ever multiplied with a coefficient of a component.
//   gto_charge_grad_kernel          one wave per (geometry, chunk of CHG_GL charges).  A lane owns one charge and walks
//       the shell pairs ss, ps, pp in their fixed order; per (primitive pair, charge) it forms what
//       gto_grad_one_kernel forms for a nucleus: the derivative coefficients on the first centre and d/dP for the sum
//       of both.  The charge's own share, minus d/dP, stays in three registers and is final (no other lane touches
//       that charge); the atoms' shares go to the lane's own column of LDS [natm][3][CHG_GL] and are added over the
//       lanes by a butterfly at the end: one record of natm x 3 doubles per (geometry, chunk).
//   gto_charge_grad_reduce_kernel   the records of a geometry added over the chunks, in ascending order.
//
// No floating-point atomics; every order of summation depends on (M, the shell table) only, so a geometry has the
// same bits wherever it stands in a stack.  The work buffer holds the pair data and batch x ceil(M / CHG_GL) x natm x 3
// doubles: it does not grow with npair x M.
#include "gto_grad.h"

#define CHG_NT 256               // lanes of the operator kernel (4 waves)
#define CHG_NW (CHG_NT / 64)
#define CHG_GL 64                // charges per chunk of the gradient kernel (one wave)
#define CHG_MAX 65535            // charges per geometry
#define CHG_LDS_MAX (160 * 1024) // bytes of LDS a workgroup of the gradient kernel may ask for: natm <= 106

// ---- operator ---------------------------------------------------------------------------------------------------------
template <int LA, int LB> struct gto_chg_lds_t {
    static constexpr int L = LA + LB, D = L + 1, NR = D * D * D, NAB = gto_ncomp(LA) * gto_ncomp(LB);
    double V[NAB];
    double E[3][LA + 1][LB + 1][L + 1];
    double part[CHG_NW][NR];
    double Rs[NR];
};

template <int LA, int LB>
__global__ __launch_bounds__(CHG_NT) void gto_charge_op_kernel(const int* __restrict__ iw, const int* __restrict__ shells,
                                                               int nshell, int count, int natm,
                                                               const double* __restrict__ coords, int batch,
                                                               const double* __restrict__ pairs, int kp, int nao,
                                                               int ncharge, const double* __restrict__ q,
                                                               const double* __restrict__ qxyz, double* __restrict__ vext)
{
    using lds_t = gto_chg_lds_t<LA, LB>;
    constexpr int NB = gto_ncomp(LB), NAB = lds_t::NAB, L = lds_t::L, D = lds_t::D, NR = lds_t::NR;
    __shared__ lds_t s;
    const long grp = blockIdx.x;
    const int lane = threadIdx.x, wave = lane >> 6;
    if (grp >= (long)count * batch) return;
    const int g = (int)(grp / count), k = (int)(grp - (long)g * count);
    const long npair = (long)nshell * (nshell + 1) / 2;
    const double* xyz = coords + (size_t)g * natm * 3;
    const gto_pair_ref_t ab = gto_pair_ref(iw + nshell, gto_cls(LA, LB), k, npair, iw, shells, xyz,
                                           pairs + (size_t)g * npair * kp * GTO_PW, kp);
    const double* qg = q + (size_t)g * ncharge;
    const double* rg = qxyz + (size_t)g * ncharge * 3;
    for (int c = lane; c < NAB; c += CHG_NT) s.V[c] = 0.0;
    for (int kab = 0; kab < ab.nprim; ++kab) {
        const gto_prim_t pr = gto_load_prim(ab.data + (size_t)kab * GTO_PW, ab.swapped);
        if (lane < 3) {
            double E[LA + 1][LB + 1][L + 1];
            const double d = gto_pick(ab.AB, lane);
            gto_herm<LA, LB>(E, -pr.fb * d, pr.fa * d, pr.oo2p);
#pragma unroll
            for (int i = 0; i <= LA; ++i)
#pragma unroll
                for (int j = 0; j <= LB; ++j)
#pragma unroll
                    for (int t = 0; t <= L; ++t) s.E[lane][i][j][t] = E[i][j][t];
        }
        // this lane's charges: sum_k q_k R_tuv(P - r_k), t + u + v <= L, in registers
        double Racc[D][D][D];
        static_for<NR>([&](auto ic) {
            constexpr int i = decltype(ic)::value, t = i / (D * D), u = (i / D) % D, v = i % D;
            if constexpr (t + u + v <= L) Racc[t][u][v] = 0.0;
        });
        const double fV = -2.0 * GTO_PI / pr.p * pr.cck;
        for (int kc = lane; kc < ncharge; kc += CHG_NT) {
            const double X = pr.P[0] - rg[3 * kc], Y = pr.P[1] - rg[3 * kc + 1], Z = pr.P[2] - rg[3 * kc + 2];
            double F[L + 1], Fs[L + 1], R[D][D][D];
            gto_boys<L>(pr.p * (X * X + Y * Y + Z * Z), F);
            double sc = fV * qg[kc];
#pragma unroll
            for (int n = 0; n <= L; ++n) { Fs[n] = sc * F[n]; sc *= -2.0 * pr.p; }
            gto_R_fill<L>(R, Fs, X, Y, Z);
            static_for<NR>([&](auto ic) {
                constexpr int i = decltype(ic)::value, t = i / (D * D), u = (i / D) % D, v = i % D;
                if constexpr (t + u + v <= L) Racc[t][u][v] += R[t][u][v];
            });
        }
        // over the lanes of a wave (butterfly), then over the waves in ascending order
        static_for<NR>([&](auto ic) {
            constexpr int i = decltype(ic)::value, t = i / (D * D), u = (i / D) % D, v = i % D;
            if constexpr (t + u + v <= L) {
                const double x = gto_group_sum<64>(Racc[t][u][v]);
                if ((lane & 63) == 0) s.part[wave][i] = x;
            }
        });
        __syncthreads();
        for (int i = lane; i < NR; i += CHG_NT) {
            const int t = i / (D * D), u = (i / D) % D, v = i % D;
            if (t + u + v > L) continue;
            double x = s.part[0][i];
#pragma unroll
            for (int w = 1; w < CHG_NW; ++w) x += s.part[w][i];
            s.Rs[i] = x;
        }
        __syncthreads();
        for (int c = lane; c < NAB; c += CHG_NT) {
            const int ca = c / NB, cb = c - ca * NB;
            const int ix = gto_pow(LA, ca, 0), jx = gto_pow(LB, cb, 0), iy = gto_pow(LA, ca, 1), jy = gto_pow(LB, cb, 1),
                      iz = gto_pow(LA, ca, 2), jz = gto_pow(LB, cb, 2);
            double v = 0.0;
            for (int t = 0; t <= ix + jx; ++t)
                for (int u = 0; u <= iy + jy; ++u)
                    for (int w = 0; w <= iz + jz; ++w)
                        v += s.E[0][ix][jx][t] * s.E[1][iy][jy][u] * s.E[2][iz][jz][w] * s.Rs[(t * D + u) * D + w];
            s.V[c] += v;
        }
        __syncthreads();
    }
    // the form of the d shells, once per shell pair, after the sum over the charges
    int na = gto_ncomp(LA), nb = NB;
    if (LA == 2) {
        const bool cart = (shells[4 * ab.sa + 1] & OOVQE_GTO_CARTESIAN) != 0;
        gto_d_pass(s.V, NAB, NB, cart, lane, CHG_NT);
        na = cart ? 6 : 5;
    }
    if (LB == 2) {
        const bool cart = (shells[4 * ab.sb + 1] & OOVQE_GTO_CARTESIAN) != 0;
        gto_d_pass(s.V, NAB, 1, cart, lane, CHG_NT);
        nb = cart ? 6 : 5;
    }
    const bool same = ab.sa == ab.sb;
    for (int c = lane; c < NAB; c += CHG_NT) {
        const int ca = c / NB, cb = c - ca * NB;
        if (ca >= na || cb >= nb) continue;
        const int mu = ab.oa + ca, nu = ab.ob + cb;
        if ((!same || mu >= nu) && mu < nao && nu < nao) {
            const double x = s.V[c];
            vext[((size_t)g * nao + mu) * nao + nu] = x;
            vext[((size_t)g * nao + nu) * nao + mu] = x;
        }
    }
}

// ---- gradient ---------------------------------------------------------------------------------------------------------
// the shell pairs of class (LA, LB) for the charge of this lane: gQ -= d/dP, the atoms' shares to column `lane` of at
template <int LA, int LB>
__device__ __forceinline__ void gto_charge_grad_class(const int* __restrict__ iw, const int* __restrict__ shells,
                                                      int nshell, int count, const double* __restrict__ xyz,
                                                      const double* __restrict__ pairs_g, int kp, int nao,
                                                      const double* __restrict__ d1g, double qk, double rx, double ry,
                                                      double rz, double (&gQ)[3], double* __restrict__ at, int lane)
{
    constexpr int NA = gto_ncomp(LA), NB = gto_ncomp(LB), L = LA + LB;
    const long npair = (long)nshell * (nshell + 1) / 2;
    for (int k = 0; k < count; ++k) {
        const gto_pair_ref_t ab = gto_pair_ref(iw + nshell, gto_cls(LA, LB), k, npair, iw, shells, xyz, pairs_g, kp);
        const int atA = shells[4 * ab.sa], atB = shells[4 * ab.sb];
        const double deg = (ab.sa == ab.sb) ? 1.0 : 2.0;
        double w1[NA * NB];
#pragma unroll
        for (int c = 0; c < NA * NB; ++c) w1[c] = deg * d1g[(size_t)(ab.oa + c / NB) * nao + (ab.ob + c % NB)];
        double vA[3] = {0.0, 0.0, 0.0}, vP[3] = {0.0, 0.0, 0.0};
        for (int kab = 0; kab < ab.nprim; ++kab) {
            const gto_prim_t pr = gto_load_prim(ab.data + (size_t)kab * GTO_PW, ab.swapped);
            double E[3][LA + 2][LB + 1][L + 2], dE[3][LA + 1][LB + 1][L + 2];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                gto_herm<LA + 1, LB>(E[d], -pr.fb * ab.AB[d], pr.fa * ab.AB[d], pr.oo2p);
                gto_herm_deriv<LA, LB>(dE[d], E[d], pr.fa * pr.p);
            }
            const double X = pr.P[0] - rx, Y = pr.P[1] - ry, Z = pr.P[2] - rz;
            double F[L + 2], Fs[L + 2], R[L + 2][L + 2][L + 2];
            gto_boys<L + 1>(pr.p * (X * X + Y * Y + Z * Z), F);
            double sc = -2.0 * GTO_PI / pr.p * pr.cck * qk;
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
        // first centre: its derivative coefficients; second: d/dP minus that; the charge: minus d/dP
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            gQ[d] -= vP[d];
            at[(atA * 3 + d) * CHG_GL + lane] += vA[d];
            at[(atB * 3 + d) * CHG_GL + lane] += vP[d] - vA[d];
        }
    }
}

__global__ __launch_bounds__(CHG_GL) void gto_charge_grad_kernel(const int* __restrict__ iw, const int* __restrict__ shells,
                                                                 int nshell, int n_ss, int n_ps, int n_pp,
                                                                 const double* __restrict__ zat, int natm,
                                                                 const double* __restrict__ coords,
                                                                 const double* __restrict__ pairs, int kp, int nao,
                                                                 int ncharge, const double* __restrict__ q,
                                                                 const double* __restrict__ qxyz,
                                                                 const double* __restrict__ d1, int with_nuc,
                                                                 double* __restrict__ gq, double* __restrict__ rec)
{
    extern __shared__ double at[];              // [natm][3][CHG_GL]: a lane reads and writes its own column only
    const int chunk = blockIdx.x, nchunk = gridDim.x, g = blockIdx.y, lane = threadIdx.x;
    const long npair = (long)nshell * (nshell + 1) / 2;
    const double* xyz = coords + (size_t)g * natm * 3;
    const double* pairs_g = pairs + (size_t)g * npair * kp * GTO_PW;
    const double* d1g = d1 + (size_t)g * nao * nao;
    // (a lane beyond the last charge runs along with charge zero of weight 0 and stores nothing of its own)
    const int kc = chunk * CHG_GL + lane;
    const bool mine = kc < ncharge;
    const size_t kr = (size_t)g * ncharge + (mine ? kc : 0);
    const double qk = mine ? q[kr] : 0.0;
    const double rx = qxyz[3 * kr], ry = qxyz[3 * kr + 1], rz = qxyz[3 * kr + 2];
    for (int a = 0; a < natm * 3; ++a) at[a * CHG_GL + lane] = 0.0;
    double gQ[3] = {0.0, 0.0, 0.0};
    gto_charge_grad_class<0, 0>(iw, shells, nshell, n_ss, xyz, pairs_g, kp, nao, d1g, qk, rx, ry, rz, gQ, at, lane);
    gto_charge_grad_class<1, 0>(iw, shells, nshell, n_ps, xyz, pairs_g, kp, nao, d1g, qk, rx, ry, rz, gQ, at, lane);
    gto_charge_grad_class<1, 1>(iw, shells, nshell, n_pp, xyz, pairs_g, kp, nao, d1g, qk, rx, ry, rz, gQ, at, lane);
    if (with_nuc && mine) {
        // d/dR_A and d/dr_k of sum_A Z_A q_k / |R_A - r_k| (a charge ON a nucleus has no such derivative: NaN)
        for (int a = 0; a < natm; ++a) {
            const double dx = xyz[3 * a] - rx, dy = xyz[3 * a + 1] - ry, dz = xyz[3 * a + 2] - rz;
            const double r2 = dx * dx + dy * dy + dz * dz;
            const double f = zat[a] * qk / (r2 * sqrt(r2));
            gQ[0] += f * dx; gQ[1] += f * dy; gQ[2] += f * dz;
            at[(a * 3 + 0) * CHG_GL + lane] -= f * dx;
            at[(a * 3 + 1) * CHG_GL + lane] -= f * dy;
            at[(a * 3 + 2) * CHG_GL + lane] -= f * dz;
        }
    }
    if (mine) {
#pragma unroll
        for (int d = 0; d < 3; ++d) gq[kr * 3 + d] = gQ[d];
    }
    double* out = rec + ((size_t)g * nchunk + chunk) * natm * 3;
    for (int a = 0; a < natm * 3; ++a) {
        const double x = gto_group_sum<CHG_GL>(at[a * CHG_GL + lane]);
        if (lane == 0) out[a] = x;
    }
}

__global__ __launch_bounds__(64) void gto_charge_grad_reduce_kernel(const double* __restrict__ rec, int nchunk, int n3,
                                                                    int batch, double* __restrict__ grad)
{
    const long tid = (long)blockIdx.x * 64 + threadIdx.x;
    if (tid >= (long)batch * n3) return;
    const int g = (int)(tid / n3), a = (int)(tid - (long)g * n3);
    const double* p = rec + (size_t)g * nchunk * n3 + a;
    double x = 0.0;
    for (int c = 0; c < nchunk; ++c) x += p[(size_t)c * n3];
    grad[tid] = x;
}

// ---- host side --------------------------------------------------------------------------------------------------------
namespace {
int chg_check(const char* who, int batch, int ncharge)
{
    OOVQE_REQUIRE(batch <= 65535, "%s: batch = %d (at most 65535 geometries per call)", who, batch);
    OOVQE_REQUIRE(ncharge >= 1 && ncharge <= CHG_MAX, "%s: ncharge = %d (1 .. %d point charges per geometry)", who,
                  ncharge, CHG_MAX);
    return 0;
}

// the gradient kernel keeps the atoms' shares of a chunk in dynamic LDS [natm][3][CHG_GL]: refused before anything is
// launched where that exceeds what a workgroup can have
int chg_check_atoms(const char* who, int natm)
{
    const size_t lds = (size_t)(natm > 0 ? natm : 0) * 3 * CHG_GL * sizeof(double);
    OOVQE_REQUIRE(lds <= CHG_LDS_MAX, "%s: natm = %d (the atoms' shares of a chunk need %zu bytes of LDS, at most %d)", who,
                  natm, lds, CHG_LDS_MAX);
    return 0;
}

template <int LA, int LB>
int chg_launch_op(gto_cls_t<LA, LB>, const gto_prep_t& p, int ncharge, const double* q, const double* qxyz, double* vext)
{
    const int count = p.cnt[gto_cls(LA, LB)];
    if (count == 0) return 0;
    unsigned grid;
    if (const int rc = gto_grid_wg(p.who, (long)count * p.batch, &grid)) return rc;
    hipLaunchKernelGGL((gto_charge_op_kernel<LA, LB>), dim3(grid), dim3(CHG_NT), 0, p.st, p.iw, p.shells, p.nshell, count,
                       p.natm, p.coords, p.batch, p.pairs, p.kp, p.nao, ncharge, q, qxyz, vext);
    OOVQE_CHECK_LAUNCH("gto_charge_op_kernel");
    return 0;
}
}  // namespace

extern "C" int oovqe_gto_point_charge_batch(int nshell, const int32_t* shells, int nprim_total, const double* exps,
                                            const double* coefs, int natm, const double* charges, int batch,
                                            const double* coords, int nao, int ncharge, const double* q,
                                            const double* qxyz, double* vext, double* work, oovqe_stream_t stream)
{
    const char* who = "oovqe_gto_point_charge_batch";
    hipStream_t st = (hipStream_t)stream;
    int rc = chg_check(who, batch, ncharge);
    if (rc != 0) return rc;
    gto_prep_t p;
    rc = gto_prepare(who, OOVQE_GTO_MAX_L, nshell, shells, nprim_total, exps, coefs, natm, charges, batch, coords, nao,
                     nullptr, work, st, &p);
    if (rc != 0 || batch == 0) return rc;
    OOVQE_REQUIRE(q && qxyz && vext, "%s: null pointer", who);
    return gto_pairs_descending([&](auto c) { return chg_launch_op(c, p, ncharge, q, qxyz, vext); });
}

extern "C" int64_t oovqe_gto_point_charge_gradient_work_size(int nshell, int max_nprim, int natm, int batch, int ncharge)
{
    const char* who = "oovqe_gto_point_charge_gradient_work_size";
    if (gto_check_sizes(who, nshell, max_nprim, batch) != 0) return OOVQE_ERR_ARG;
    OOVQE_REQUIRE(natm >= 1, "%s: natm = %d", who, natm);
    if (chg_check(who, batch, ncharge) != 0) return OOVQE_ERR_ARG;
    if (chg_check_atoms(who, natm) != 0) return OOVQE_ERR_ARG;
    const int64_t nchunk = (ncharge + CHG_GL - 1) / CHG_GL;
    return gto_work_base(nshell, max_nprim, batch) + (int64_t)batch * nchunk * natm * 3;
}

extern "C" int oovqe_gto_point_charge_gradient_batch(int nshell, const int32_t* shells, int nprim_total,
                                                     const double* exps, const double* coefs, int natm,
                                                     const double* charges, int batch, const double* coords, int nao,
                                                     int ncharge, const double* q, const double* qxyz, const double* d1,
                                                     int with_nuc, double* grad_atoms, double* grad_charges,
                                                     double* work, oovqe_stream_t stream)
{
    // (the name every message of gto_prepare starts with: its refusal of l = 2 then says what is refused)
    const char* who = "oovqe_gto_point_charge_gradient_batch (no derivatives of d shells)";
    hipStream_t st = (hipStream_t)stream;
    int rc = chg_check(who, batch, ncharge);
    if (rc != 0) return rc;
    if ((rc = chg_check_atoms(who, natm)) != 0) return rc;
    gto_prep_t p;
    rc = gto_prepare(who, 1, nshell, shells, nprim_total, exps, coefs, natm, charges, batch, coords, nao, nullptr, work,
                     st, &p);
    if (rc != 0 || batch == 0) return rc;
    OOVQE_REQUIRE(q && qxyz && d1 && grad_atoms && grad_charges, "%s: null pointer", who);
    const size_t lds = (size_t)natm * 3 * CHG_GL * sizeof(double);
    if (oovqe_ensure_dynamic_lds(reinterpret_cast<const void*>(&gto_charge_grad_kernel), lds) != 0) return OOVQE_ERR_HIP;
    const int nchunk = (ncharge + CHG_GL - 1) / CHG_GL;
    double* rec = p.rec;
    hipLaunchKernelGGL(gto_charge_grad_kernel, dim3(nchunk, batch), dim3(CHG_GL), lds, st, p.iw, shells, nshell,
                       p.cnt[gto_cls(0, 0)], p.cnt[gto_cls(1, 0)], p.cnt[gto_cls(1, 1)], charges, natm, coords, p.pairs,
                       p.kp, nao, ncharge, q, qxyz, d1, with_nuc ? 1 : 0, grad_charges, rec);
    OOVQE_CHECK_LAUNCH("gto_charge_grad_kernel");
    const long total = (long)batch * natm * 3;
    hipLaunchKernelGGL(gto_charge_grad_reduce_kernel, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, st, rec, nchunk,
                       natm * 3, batch, grad_atoms);
    OOVQE_CHECK_LAUNCH("gto_charge_grad_reduce_kernel");
    return 0;
}
