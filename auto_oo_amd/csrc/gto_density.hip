// Electron density, its gradient and orbital values of a stack of geometries at arbitrary points (gfx950): every geometry
// g has its own M points r[g, m], K density matrices D[g, k] (general: both (mu, nu) and (nu, mu) are read) or ncol
// coefficient columns C[g, :, i],
//
//   rho[g, k, m]     = sum_{mu nu} D[g, k, mu, nu] chi_mu(r_m) chi_nu(r_m)      drho[g, k, m, :] = d rho / d r_m (optional)
//   psi[g, i, m]     = sum_mu C[g, mu, i] chi_mu(r_m)                           dpsi[g, i, m, :] = d psi / d r_m (optional)
//
// over the functions of the integral kernels (s, p and d shells, both d forms).  The decomposition is that of
// gto_potential.hip: the points are the parallel dimension, one workgroup of DEN_NT lanes per (geometry, chunk of DEN_NT
// points), a lane owns one point.  There is no pair data and no work buffer: a Gaussian at a point needs the shell table
// and the geometry alone.
//
//   gto_density_kernel <grad>   first every lane makes, per shell, the radial sums of ITS point, R0 = sum_p c_p e^(-a_p
//       r^2) and (grad) R1 = sum_p -2 a_p c_p e^(-a_p r^2), into its own column of LDS [shell][1 or 2][DEN_NT]: once per
//       shell, not once per shell pair.  Then the workgroup walks the shell pairs i >= j in that order.  Per pair the K
//       blocks of D (+ their transposes for two different shells) go to LDS once, and the form of the d shells is folded
//       into them there (gto_pot_d_back: sqrt 3, or the 5 -> 6 back-transform), so nothing per point meets a coefficient
//       of a component.  A lane makes the Cartesian components chi_a, chi_b (and their derivatives) of the two shells at
//       its point in registers, u_a = sum_b W_ab chi_b, v_b = sum_a W_ab chi_a, and
//           rho += sum_a chi_a u_a,     drho += sum_a dchi_a u_a + sum_b dchi_b v_b.
//   gto_orbital_kernel <grad>   the same per shell: the rows of C of the shell go to LDS [column][component], the d form is
//       folded in, psi_i += sum_c W_ic chi_c.  The radial sums of a shell are used once, so they stay in registers.
//
// The sums of a lane live in its own column of LDS [K or ncol][1 or 4][DEN_NT]; no per-thread array is indexed at run
// time; nobody else touches a lane's columns.  No atomics, no scratch.  A value depends on the shell table, its geometry,
// its density (or column) and its point alone, and every product that meets a sum is an explicit fma, so the two
// instantiations round alike: a (geometry, set, point) has the same bits wherever it stands in the stack, among the points
// and among the sets, on any stream, with or without the gradient.
// x^0 is the literal 1 and the term l x^(l-1) of a derivative is not formed for l = 0: a point ON a nucleus has finite,
// exact values.  A coordinate of a point beyond +-DEN_CLAMP Bohr is taken as +-DEN_CLAMP: there every exponential of any
// exponent above 1e-147 is exactly zero and the polynomials in front of it are still finite, so the result is an exact
// zero and never 0 * inf.
// The bodies are __host__ __device__ functions of (chunk, geometry, lane, nlane): a CPU build (GTO_DENSITY_BODIES_ONLY:
// no kernel, no entry point; tools/gto_density_host.hip) runs them with one lane per workgroup (chunks of one point), or
// with the lanes as host threads and GTO_HOST_BARRIER as the barrier.
#define GTO_POTENTIAL_BODIES_ONLY        // gto_pot_d_back alone is taken from the potential kernel
#include "gto_potential.hip"
#undef GTO_POTENTIAL_BODIES_ONLY

#define DEN_NT 64                // lanes of a workgroup = points of a chunk (one wave)
#define DEN_MAX 65535            // points per geometry
#define DEN_KMAX OOVQE_GTO_GRAD_MAX_SETS
#define DEN_NAB 36               // components of a dd pair
#define DEN_CLAMP 1e75           // Bohr
#define DEN_LDS_MAX 65536        // bytes of LDS a workgroup may ask for (static + dynamic)

struct gto_den_lds_t {
    double W[DEN_KMAX * DEN_NAB];           // [set][ca][cb] of the current shell pair, or [column][c] of the current shell
    int off[OOVQE_GTO_MAX_SHELL];           // AO offset of every shell
};

template <int N> __host__ __device__ __forceinline__ double gto_den_pow(double x)
{
    if constexpr (N <= 0) return 1.0;
    else if constexpr (N == 1) return x;
    else return x * gto_den_pow<N - 1>(x);
}

// The Cartesian components x^i y^j z^k R0 of a shell of angular momentum L at the displacement (x, y, z) from its centre
// and, GRAD, their derivatives (i x^(i-1) y^j z^k) R0 + x (x^i y^j z^k) R1 ...: the first term only where i > 0.
// chi does not depend on GRAD.
template <int L, bool GRAD>
__host__ __device__ __forceinline__ void gto_den_shell(double x, double y, double z, double r0, double r1,
                                                       double (&chi)[gto_ncomp(L)], double (&dchi)[3][gto_ncomp(L)])
{
    static_for<gto_ncomp(L)>([&](auto cc) {
        constexpr int c = decltype(cc)::value, i = gto_pow(L, c, 0), j = gto_pow(L, c, 1), k = gto_pow(L, c, 2);
        const double px = gto_den_pow<i>(x), py = gto_den_pow<j>(y), pz = gto_den_pow<k>(z);
        const double poly = px * py * pz;
        chi[c] = poly * r0;
        if constexpr (GRAD) {
            const double pr1 = poly * r1;
            if constexpr (i > 0) dchi[0][c] = fma(x, pr1, ((double)i * gto_den_pow<i - 1>(x) * py * pz) * r0);
            else dchi[0][c] = x * pr1;
            if constexpr (j > 0) dchi[1][c] = fma(y, pr1, ((double)j * px * gto_den_pow<j - 1>(y) * pz) * r0);
            else dchi[1][c] = y * pr1;
            if constexpr (k > 0) dchi[2][c] = fma(z, pr1, ((double)k * px * py * gto_den_pow<k - 1>(z)) * r0);
            else dchi[2][c] = z * pr1;
        }
    });
}

// R0 = sum_p c_p e^(-a_p r^2) and, GRAD, R1 = sum_p -2 a_p c_p e^(-a_p r^2) of one shell, the primitives in their order
template <bool GRAD>
__host__ __device__ __forceinline__ void gto_den_radial(const int* __restrict__ sh, const double* __restrict__ exps,
                                                        const double* __restrict__ coefs, double r2, double& r0, double& r1)
{
    const int np = sh[2], po = sh[3];
    r0 = 0.0;
    r1 = 0.0;
    for (int p = 0; p < np; ++p) {
        const double a = exps[po + p], c = coefs[po + p];
        const double e = exp(-(a * r2));
        r0 = fma(c, e, r0);
        if constexpr (GRAD) r1 = fma((-2.0 * a) * c, e, r1);
    }
}

__host__ __device__ __forceinline__ double gto_den_clamp(double x)
{
    return x > DEN_CLAMP ? DEN_CLAMP : (x < -DEN_CLAMP ? -DEN_CLAMP : x);
}

// AO offsets of the shells into s.off (every lane needs all of them)
__host__ __device__ __forceinline__ void gto_den_offsets(int lane, int nlane, gto_den_lds_t& s,
                                                         const int* __restrict__ shells, int nshell)
{
    for (int i = lane; i < nshell; i += nlane) {
        int o = 0;
        for (int t = 0; t < i; ++t) o += gto_nfunc(shells[4 * t + 1]);
        s.off[i] = o;
    }
    gto_sync();
}

// the shell pair (sa, sb), l of sa = LA >= LB = l of sb, for the point of this lane: column `lane` of acc [nset][NC][nlane]
// receives sum D chi chi and, GRAD, its derivative in the point.  rad [nshell][NR][nlane]: the radial sums.
template <int LA, int LB, bool GRAD>
__host__ __device__ __forceinline__ void gto_den_pair(int lane, int nlane, gto_den_lds_t& s, double* __restrict__ acc,
                                                      const double* __restrict__ rad, int sa, int sb,
                                                      const int* __restrict__ shells, const double* __restrict__ xyz,
                                                      int nao, int nset, const double* __restrict__ dm_g, double rx,
                                                      double ry, double rz)
{
    constexpr int NA = gto_ncomp(LA), NB = gto_ncomp(LB), NAB = NA * NB, NC = GRAD ? 4 : 1, NR = GRAD ? 2 : 1;
    const size_t nn = (size_t)nao * nao;
    const bool same = sa == sb;
    const int fa = shells[4 * sa + 1], fb = shells[4 * sb + 1];
    const int na = gto_nfunc(fa), nb = gto_nfunc(fb), oa = s.off[sa], ob = s.off[sb];
    gto_sync();                                 // every lane has finished with the weights of the pair before
    // the weights of the pair of every set: D_ab + D_ba (one shell with itself: its block as it stands)
    for (int i = lane; i < nset * NAB; i += nlane) {
        const int ks = i / NAB, c = i - ks * NAB, ca = c / NB, cb = c - ca * NB;
        double w = 0.0;
        if (ca < na && cb < nb) {
            const double* d = dm_g + (size_t)ks * nn;
            const size_t mu = oa + ca, nu = ob + cb;
            w = same ? d[mu * nao + nu] : d[mu * nao + nu] + d[nu * nao + mu];
        }
        s.W[i] = w;
    }
    gto_sync();
    if (LA == 2) gto_pot_d_back(s.W, nset * NAB, NB, (fa & OOVQE_GTO_CARTESIAN) != 0, lane, nlane);
    if (LB == 2) gto_pot_d_back(s.W, nset * NAB, 1, (fb & OOVQE_GTO_CARTESIAN) != 0, lane, nlane);
    // this lane's point
    const double* A = xyz + 3 * shells[4 * sa];
    const double* B = xyz + 3 * shells[4 * sb];
    const double* ra = rad + (size_t)sa * NR * nlane + lane;
    const double* rb = rad + (size_t)sb * NR * nlane + lane;
    double ca[NA], da[3][NA], cb[NB], db[3][NB];
    gto_den_shell<LA, GRAD>(rx - A[0], ry - A[1], rz - A[2], ra[0], GRAD ? ra[nlane] : 0.0, ca, da);
    gto_den_shell<LB, GRAD>(rx - B[0], ry - B[1], rz - B[2], rb[0], GRAD ? rb[nlane] : 0.0, cb, db);
    for (int ks = 0; ks < nset; ++ks) {
        const double* w = s.W + ks * NAB;
        double a0 = 0.0, ax = 0.0, ay = 0.0, az = 0.0, v[NB];
        if constexpr (GRAD) static_for<NB>([&](auto bc) { v[decltype(bc)::value] = 0.0; });
        static_for<NA>([&](auto ac) {
            constexpr int a = decltype(ac)::value;
            double u = 0.0;
            static_for<NB>([&](auto bc) {
                constexpr int b = decltype(bc)::value;
                const double x = w[a * NB + b];
                u = fma(x, cb[b], u);
                if constexpr (GRAD) v[b] = fma(x, ca[a], v[b]);
            });
            a0 = fma(ca[a], u, a0);
            if constexpr (GRAD) {
                ax = fma(da[0][a], u, ax);
                ay = fma(da[1][a], u, ay);
                az = fma(da[2][a], u, az);
            }
        });
        if constexpr (GRAD)
            static_for<NB>([&](auto bc) {
                constexpr int b = decltype(bc)::value;
                ax = fma(db[0][b], v[b], ax);
                ay = fma(db[1][b], v[b], ay);
                az = fma(db[2][b], v[b], az);
            });
        double* col = acc + (size_t)ks * NC * nlane + lane;
        col[0] += a0;
        if constexpr (GRAD) {
            col[nlane] += ax;
            col[2 * nlane] += ay;
            col[3 * nlane] += az;
        }
    }
}

// acc [nset][1 or 4][nlane], rad [nshell][1 or 2][nlane]
template <bool GRAD>
__host__ __device__ __forceinline__ void gto_den_body(int chunk, int g, int lane, int nlane, gto_den_lds_t& s,
                                                      double* __restrict__ acc, double* __restrict__ rad,
                                                      const int* __restrict__ shells, int nshell,
                                                      const double* __restrict__ exps, const double* __restrict__ coefs,
                                                      int natm, const double* __restrict__ coords, int nao, int nset,
                                                      const double* __restrict__ dm, int npoint,
                                                      const double* __restrict__ points, double* __restrict__ rho,
                                                      double* __restrict__ drho)
{
    constexpr int NC = GRAD ? 4 : 1, NR = GRAD ? 2 : 1;
    const double* xyz = coords + (size_t)g * natm * 3;
    const double* dm_g = dm + (size_t)g * nset * nao * nao;
    // (a lane beyond the last point runs along with point zero and stores nothing)
    const int m = chunk * nlane + lane;
    const bool mine = m < npoint;
    const double* r = points + ((size_t)g * npoint + (mine ? m : 0)) * 3;
    const double rx = gto_den_clamp(r[0]), ry = gto_den_clamp(r[1]), rz = gto_den_clamp(r[2]);
    for (int i = 0; i < nset * NC; ++i) acc[(size_t)i * nlane + lane] = 0.0;
    for (int sh = 0; sh < nshell; ++sh) {
        const double* A = xyz + 3 * shells[4 * sh];
        const double dx = rx - A[0], dy = ry - A[1], dz = rz - A[2];
        double r0, r1;
        gto_den_radial<GRAD>(shells + 4 * sh, exps, coefs, fma(dx, dx, fma(dy, dy, dz * dz)), r0, r1);
        rad[(size_t)sh * NR * nlane + lane] = r0;
        if constexpr (GRAD) rad[((size_t)sh * NR + 1) * nlane + lane] = r1;
    }
    gto_den_offsets(lane, nlane, s, shells, nshell);
    for (int i = 0; i < nshell; ++i)
        for (int j = 0; j <= i; ++j) {
            const int li = gto_l_of(shells[4 * i + 1]), lj = gto_l_of(shells[4 * j + 1]);
            const int sa = li >= lj ? i : j, sb = li >= lj ? j : i;
            switch (gto_cls(li >= lj ? li : lj, li >= lj ? lj : li)) {
            case gto_cls(0, 0): gto_den_pair<0, 0, GRAD>(lane, nlane, s, acc, rad, sa, sb, shells, xyz, nao, nset, dm_g, rx, ry, rz); break;
            case gto_cls(1, 0): gto_den_pair<1, 0, GRAD>(lane, nlane, s, acc, rad, sa, sb, shells, xyz, nao, nset, dm_g, rx, ry, rz); break;
            case gto_cls(1, 1): gto_den_pair<1, 1, GRAD>(lane, nlane, s, acc, rad, sa, sb, shells, xyz, nao, nset, dm_g, rx, ry, rz); break;
            case gto_cls(2, 0): gto_den_pair<2, 0, GRAD>(lane, nlane, s, acc, rad, sa, sb, shells, xyz, nao, nset, dm_g, rx, ry, rz); break;
            case gto_cls(2, 1): gto_den_pair<2, 1, GRAD>(lane, nlane, s, acc, rad, sa, sb, shells, xyz, nao, nset, dm_g, rx, ry, rz); break;
            default: gto_den_pair<2, 2, GRAD>(lane, nlane, s, acc, rad, sa, sb, shells, xyz, nao, nset, dm_g, rx, ry, rz); break;
            }
        }
    if (!mine) return;
    for (int ks = 0; ks < nset; ++ks) {
        const double* col = acc + (size_t)ks * NC * nlane + lane;
        const size_t o = ((size_t)g * nset + ks) * npoint + m;
        rho[o] = col[0];
        if constexpr (GRAD) {
            drho[3 * o] = col[nlane];
            drho[3 * o + 1] = col[2 * nlane];
            drho[3 * o + 2] = col[3 * nlane];
        }
    }
}

// one shell of angular momentum L for the point of this lane: psi_i += sum_c C[oa + c, i] chi_c, i < ncol
template <int L, bool GRAD>
__host__ __device__ __forceinline__ void gto_orb_shell(int lane, int nlane, gto_den_lds_t& s, double* __restrict__ acc,
                                                       int sh, const int* __restrict__ shells,
                                                       const double* __restrict__ exps, const double* __restrict__ coefs,
                                                       const double* __restrict__ xyz, int ncol,
                                                       const double* __restrict__ c_g, double rx, double ry, double rz)
{
    constexpr int NA = gto_ncomp(L), NC = GRAD ? 4 : 1;
    const int fa = shells[4 * sh + 1], na = gto_nfunc(fa), oa = s.off[sh];
    gto_sync();                                 // every lane has finished with the weights of the shell before
    for (int i = lane; i < ncol * NA; i += nlane) {
        const int col = i / NA, c = i - col * NA;
        s.W[i] = c < na ? c_g[(size_t)(oa + c) * ncol + col] : 0.0;
    }
    gto_sync();
    if (L == 2) gto_pot_d_back(s.W, ncol * NA, 1, (fa & OOVQE_GTO_CARTESIAN) != 0, lane, nlane);
    const double* A = xyz + 3 * shells[4 * sh];
    const double dx = rx - A[0], dy = ry - A[1], dz = rz - A[2];
    double r0, r1, ca[NA], da[3][NA];
    gto_den_radial<GRAD>(shells + 4 * sh, exps, coefs, fma(dx, dx, fma(dy, dy, dz * dz)), r0, r1);
    gto_den_shell<L, GRAD>(dx, dy, dz, r0, r1, ca, da);
    for (int i = 0; i < ncol; ++i) {
        const double* w = s.W + i * NA;
        double a0 = 0.0, ax = 0.0, ay = 0.0, az = 0.0;
        static_for<NA>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            const double x = w[c];
            a0 = fma(x, ca[c], a0);
            if constexpr (GRAD) {
                ax = fma(x, da[0][c], ax);
                ay = fma(x, da[1][c], ay);
                az = fma(x, da[2][c], az);
            }
        });
        double* col = acc + (size_t)i * NC * nlane + lane;
        col[0] += a0;
        if constexpr (GRAD) {
            col[nlane] += ax;
            col[2 * nlane] += ay;
            col[3 * nlane] += az;
        }
    }
}

// acc [ncol][1 or 4][nlane]; cmat [batch][nao][ncol]
template <bool GRAD>
__host__ __device__ __forceinline__ void gto_orb_body(int chunk, int g, int lane, int nlane, gto_den_lds_t& s,
                                                      double* __restrict__ acc, const int* __restrict__ shells,
                                                      int nshell, const double* __restrict__ exps,
                                                      const double* __restrict__ coefs, int natm,
                                                      const double* __restrict__ coords, int nao, int ncol,
                                                      const double* __restrict__ cmat, int npoint,
                                                      const double* __restrict__ points, double* __restrict__ psi,
                                                      double* __restrict__ dpsi)
{
    constexpr int NC = GRAD ? 4 : 1;
    const double* xyz = coords + (size_t)g * natm * 3;
    const double* c_g = cmat + (size_t)g * nao * ncol;
    const int m = chunk * nlane + lane;
    const bool mine = m < npoint;
    const double* r = points + ((size_t)g * npoint + (mine ? m : 0)) * 3;
    const double rx = gto_den_clamp(r[0]), ry = gto_den_clamp(r[1]), rz = gto_den_clamp(r[2]);
    for (int i = 0; i < ncol * NC; ++i) acc[(size_t)i * nlane + lane] = 0.0;
    gto_den_offsets(lane, nlane, s, shells, nshell);
    for (int sh = 0; sh < nshell; ++sh) {
        switch (gto_l_of(shells[4 * sh + 1])) {
        case 0: gto_orb_shell<0, GRAD>(lane, nlane, s, acc, sh, shells, exps, coefs, xyz, ncol, c_g, rx, ry, rz); break;
        case 1: gto_orb_shell<1, GRAD>(lane, nlane, s, acc, sh, shells, exps, coefs, xyz, ncol, c_g, rx, ry, rz); break;
        default: gto_orb_shell<2, GRAD>(lane, nlane, s, acc, sh, shells, exps, coefs, xyz, ncol, c_g, rx, ry, rz); break;
        }
    }
    if (!mine) return;
    for (int i = 0; i < ncol; ++i) {
        const double* col = acc + (size_t)i * NC * nlane + lane;
        const size_t o = ((size_t)g * ncol + i) * npoint + m;
        psi[o] = col[0];
        if constexpr (GRAD) {
            dpsi[3 * o] = col[nlane];
            dpsi[3 * o + 1] = col[2 * nlane];
            dpsi[3 * o + 2] = col[3 * nlane];
        }
    }
}

#ifndef GTO_DENSITY_BODIES_ONLY
template <bool GRAD>
__global__ __launch_bounds__(DEN_NT) void gto_density_kernel(const int* __restrict__ shells, int nshell,
                                                             const double* __restrict__ exps,
                                                             const double* __restrict__ coefs, int natm,
                                                             const double* __restrict__ coords, int nao, int nset,
                                                             const double* __restrict__ dm, int npoint,
                                                             const double* __restrict__ points, double* __restrict__ rho,
                                                             double* __restrict__ drho)
{
    __shared__ gto_den_lds_t s;
    extern __shared__ double den_cols[];        // acc [nset][1 or 4][DEN_NT] | rad [nshell][1 or 2][DEN_NT]: a lane reads
                                                // and writes its own columns only
    gto_den_body<GRAD>((int)blockIdx.x, (int)blockIdx.y, (int)threadIdx.x, DEN_NT, s, den_cols,
                       den_cols + (size_t)nset * (GRAD ? 4 : 1) * DEN_NT, shells, nshell, exps, coefs, natm, coords, nao,
                       nset, dm, npoint, points, rho, drho);
}

template <bool GRAD>
__global__ __launch_bounds__(DEN_NT) void gto_orbital_kernel(const int* __restrict__ shells, int nshell,
                                                             const double* __restrict__ exps,
                                                             const double* __restrict__ coefs, int natm,
                                                             const double* __restrict__ coords, int nao, int ncol,
                                                             const double* __restrict__ cmat, int npoint,
                                                             const double* __restrict__ points, double* __restrict__ psi,
                                                             double* __restrict__ dpsi)
{
    __shared__ gto_den_lds_t s;
    extern __shared__ double den_cols[];        // acc [ncol][1 or 4][DEN_NT]
    gto_orb_body<GRAD>((int)blockIdx.x, (int)blockIdx.y, (int)threadIdx.x, DEN_NT, s, den_cols, shells, nshell, exps, coefs,
                       natm, coords, nao, ncol, cmat, npoint, points, psi, dpsi);
}

// ---- host side --------------------------------------------------------------------------------------------------------
namespace {
// the checks both entries share, in this order, before anything is launched; tab receives the shell table
int den_check(const char* who, int nshell, const int32_t* shells, int nprim_total, const double* exps, const double* coefs,
              int natm, int batch, const double* coords, int nao, int nset, const char* what, const double* in,
              int npoint, const double* points, const double* out, hipStream_t st)
{
    OOVQE_REQUIRE(nshell >= 1 && nshell <= OOVQE_GTO_MAX_SHELL, "%s: nshell = %d (1 .. %d)", who, nshell,
                  OOVQE_GTO_MAX_SHELL);
    OOVQE_REQUIRE(batch >= 0 && batch <= 65535, "%s: batch = %d (at most 65535 geometries per call)", who, batch);
    OOVQE_REQUIRE(natm >= 1 && nprim_total >= 1, "%s: natm = %d, nprim_total = %d", who, natm, nprim_total);
    OOVQE_REQUIRE(nset >= 1 && nset <= DEN_KMAX, "%s: %d %s per geometry (1 .. %d)", who, nset, what, DEN_KMAX);
    OOVQE_REQUIRE(npoint >= 1 && npoint <= DEN_MAX, "%s: npoint = %d (1 .. %d points per geometry)", who, npoint, DEN_MAX);
    if (batch == 0) return 0;
    OOVQE_REQUIRE(shells && exps && coefs && coords && in && points && out, "%s: null pointer", who);
    std::vector<int32_t> tab;
    return gto_read_shells(who, OOVQE_GTO_MAX_L, nshell, shells, nprim_total, natm, nao, st, &tab);
}
}  // namespace

extern "C" int oovqe_gto_density_batch(int nshell, const int32_t* shells, int nprim_total, const double* exps,
                                       const double* coefs, int natm, int batch, const double* coords, int nao, int nset,
                                       const double* dm, int npoint, const double* points, double* rho, double* drho,
                                       oovqe_stream_t stream)
{
    const char* who = "oovqe_gto_density_batch";
    hipStream_t st = (hipStream_t)stream;
    const int rc = den_check(who, nshell, shells, nprim_total, exps, coefs, natm, batch, coords, nao, nset,
                             "density sets", dm, npoint, points, rho, st);
    if (rc != 0 || batch == 0) return rc;
    const size_t lds = ((size_t)nset * (drho ? 4 : 1) + (size_t)nshell * (drho ? 2 : 1)) * DEN_NT * sizeof(double);
    OOVQE_REQUIRE(lds + sizeof(gto_den_lds_t) <= DEN_LDS_MAX,
                  "%s: %d shells and %d sets %s the gradient need %zu bytes of LDS per workgroup (at most %d)", who,
                  nshell, nset, drho ? "with" : "without", lds + sizeof(gto_den_lds_t), DEN_LDS_MAX);
    const dim3 grid((unsigned)((npoint + DEN_NT - 1) / DEN_NT), (unsigned)batch);
    if (drho) {
        hipLaunchKernelGGL(gto_density_kernel<true>, grid, dim3(DEN_NT), lds, st, shells, nshell, exps, coefs, natm,
                           coords, nao, nset, dm, npoint, points, rho, drho);
    } else {
        hipLaunchKernelGGL(gto_density_kernel<false>, grid, dim3(DEN_NT), lds, st, shells, nshell, exps, coefs, natm,
                           coords, nao, nset, dm, npoint, points, rho, drho);
    }
    OOVQE_CHECK_LAUNCH("gto_density_kernel");
    return 0;
}

extern "C" int oovqe_gto_orbital_values_batch(int nshell, const int32_t* shells, int nprim_total, const double* exps,
                                              const double* coefs, int natm, int batch, const double* coords, int nao,
                                              int ncol, const double* cmat, int npoint, const double* points,
                                              double* psi, double* dpsi, oovqe_stream_t stream)
{
    const char* who = "oovqe_gto_orbital_values_batch";
    hipStream_t st = (hipStream_t)stream;
    const int rc = den_check(who, nshell, shells, nprim_total, exps, coefs, natm, batch, coords, nao, ncol,
                             "coefficient columns", cmat, npoint, points, psi, st);
    if (rc != 0 || batch == 0) return rc;
    const size_t lds = (size_t)ncol * (dpsi ? 4 : 1) * DEN_NT * sizeof(double);
    const dim3 grid((unsigned)((npoint + DEN_NT - 1) / DEN_NT), (unsigned)batch);
    if (dpsi) {
        hipLaunchKernelGGL(gto_orbital_kernel<true>, grid, dim3(DEN_NT), lds, st, shells, nshell, exps, coefs, natm,
                           coords, nao, ncol, cmat, npoint, points, psi, dpsi);
    } else {
        hipLaunchKernelGGL(gto_orbital_kernel<false>, grid, dim3(DEN_NT), lds, st, shells, nshell, exps, coefs, natm,
                           coords, nao, ncol, cmat, npoint, points, psi, dpsi);
    }
    OOVQE_CHECK_LAUNCH("gto_orbital_kernel");
    return 0;
}
#endif  // GTO_DENSITY_BODIES_ONLY
