// Shared device helpers of the Gaussian-integral kernels (gto.hip) and of their nuclear-derivative kernels
// (gto_grad.hip): constants, static_for, the Boys function, Hermite expansion coefficients, Hermite Coulomb
// integrals, the layout of the work buffer and the readers of the pair data of gto_pair_kernel.  l is a template
// parameter everywhere: the derivative kernels instantiate gto_herm / gto_boys / gto_R_fill one order higher.
// Behind them the host side every entry point of the gto*.hip files shares: gto_prep_t, the grid of a launch, the lists
// of pair and quartet classes.
#pragma once
#include "common.h"
#include "jacobi.h"
#include <math.h>
#include <utility>
#include <vector>

#define GTO_LMAX 2
#define GTO_NCLS ((GTO_LMAX + 1) * (GTO_LMAX + 2) / 2)
#define GTO_PW 8                 // doubles per primitive pair
#define GTO_NT 64                // threads per workgroup of the integral kernels (one wave)
#define GTO_SPLIT 8              // lanes that share one shell pair / quartet: each takes every 8th primitive pair of the
                                 // bra, the partial sums are added by a butterfly (fixed order: the same bits whatever
                                 // the batch).  A thread's chain of 81 primitive quartets is what a call waits for.
#define GTO_BOYS_SWITCH 5.0      // T below: series for F_L and downward recursion; above: erf and upward recursion
#define GTO_BOYS_TERMS 36        // terms of the series (last term below 1e-17 of the sum for T < 5, n >= 0)
#define GTO_PI 3.14159265358979323846
#define INVSQRT_NT JACOBI_NT

template <class F, int... I>
__host__ __device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>)
{
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F> __host__ __device__ __forceinline__ void static_for(F&& f)
{
    static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// sum over the SPLIT adjacent lanes of a group; every lane of the group receives the same bits
template <int SPLIT> __host__ __device__ __forceinline__ double gto_group_sum(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int o = 1; o < SPLIT; o <<= 1) x += __shfl_xor(x, o, 64);
#endif
    return x;
}

// Cartesian components of a shell of angular momentum l
__host__ __device__ constexpr int gto_ncomp(int l) { return l == 0 ? 1 : (l == 1 ? 3 : 6); }
// power of coordinate d in Cartesian component c of a shell of angular momentum l (s; px, py, pz; dxx, dxy, dxz, dyy,
// dyz, dzz: one hexadecimal digit per component, c = 0 the lowest)
__host__ __device__ constexpr int gto_pow(int l, int c, int d)
{
    return l == 2 ? (((d == 0 ? 0x000112 : (d == 1 ? 0x012010 : 0x210100)) >> (4 * c)) & 15)
                  : ((l == 1 && c == d) ? 1 : 0);
}
__host__ __device__ constexpr int gto_cls(int la, int lb) { return la * (la + 1) / 2 + lb; }
// the l field of a row of the shell table: angular momentum in the low byte, OOVQE_GTO_CARTESIAN for a d shell of 6
// Cartesian functions (without it: 5 real solid harmonics)
__host__ __device__ constexpr int gto_l_of(int field) { return field & 255; }
__host__ __device__ constexpr int gto_nfunc(int field)
{
    return gto_l_of(field) == 2 ? ((field & OOVQE_GTO_CARTESIAN) ? 6 : 5) : gto_ncomp(gto_l_of(field));
}

// ---- Boys function -------------------------------------------------------------------------------------------
// F_n(T) = int_0^1 t^2n exp(-T t^2) dt, n = 0 .. L.
// T < 5: F_L = exp(-T) sum_k (2T)^k / ((2L+1)(2L+3)...(2L+2k+1)) (all terms positive), then downwards
// F_{n-1} = (2T F_n + exp(-T)) / (2n - 1) (a sum of positive terms).  T >= 5: F_0 = sqrt(pi/T) erf(sqrt T) / 2, then
// upwards F_{n+1} = ((2n+1) F_n - exp(-T)) / (2T): for T >= 5 and n <= 4 the subtraction loses less than a bit per
// step.  Against 40-digit arithmetic this scheme in fp64 is within 6.4e-16 relative for n <= 4 on [0, 2000]; for the
// orders 5 .. 8 of the d classes see DESIGN.md ("d shells").
template <int L> __host__ __device__ __forceinline__ void gto_boys(double T, double (&F)[L + 1])
{
    const double et = exp(-T);
    if (T < GTO_BOYS_SWITCH) {
        const double T2 = 2.0 * T;
        double s = 0.0;
#pragma unroll
        for (int k = GTO_BOYS_TERMS; k > 0; --k) s = (s + 1.0) * T2 * (1.0 / (double)(2 * L + 2 * k + 1));
        F[L] = et * (s + 1.0) * (1.0 / (double)(2 * L + 1));
#pragma unroll
        for (int n = L; n > 0; --n) F[n - 1] = (T2 * F[n] + et) * (1.0 / (double)(2 * n - 1));
    } else {
        const double st = sqrt(T);
        F[0] = 0.88622692545275801365 / st * erf(st);        // sqrt(pi) / 2
        const double o2t = 0.5 / T;
#pragma unroll
        for (int n = 0; n < L; ++n) F[n + 1] = ((double)(2 * n + 1) * F[n] - et) * o2t;
    }
}

// ---- Hermite expansion coefficients of one dimension, without the exponential factor --------------------------
// E[i][j][t] = E_t^{ij} / E_0^{00}, i <= LA, j <= LB: E^{i+1,j}_t = E^{ij}_{t-1} / 2p + XPA E^{ij}_t + (t+1) E^{ij}_{t+1}
template <int LA, int LB>
__host__ __device__ __forceinline__ void gto_herm(double (&E)[LA + 1][LB + 1][LA + LB + 1], double xpa, double xpb, double oo2p)
{
#pragma unroll
    for (int i = 0; i <= LA; ++i) {
#pragma unroll
        for (int j = 0; j <= LB; ++j) {
#pragma unroll
            for (int t = 0; t <= LA + LB; ++t) {
                double v = 0.0;
                if (i == 0 && j == 0) {
                    v = (t == 0) ? 1.0 : 0.0;
                } else if (t <= i + j) {
                    const int top = i + j - 1;             // highest t of the parent
                    if (j == 0) {
                        if (t >= 1) v += oo2p * E[i > 0 ? i - 1 : 0][0][t > 0 ? t - 1 : 0];
                        if (t <= top) v += xpa * E[i > 0 ? i - 1 : 0][0][t];
                        if (t + 1 <= top) v += (double)(t + 1) * E[i > 0 ? i - 1 : 0][0][t + 1 <= LA + LB ? t + 1 : 0];
                    } else {
                        if (t >= 1) v += oo2p * E[i][j > 0 ? j - 1 : 0][t > 0 ? t - 1 : 0];
                        if (t <= top) v += xpb * E[i][j > 0 ? j - 1 : 0][t];
                        if (t + 1 <= top) v += (double)(t + 1) * E[i][j > 0 ? j - 1 : 0][t + 1 <= LA + LB ? t + 1 : 0];
                    }
                }
                E[i][j][t] = v;
            }
        }
    }
}

// ---- Hermite Coulomb integrals R^n_tuv from Fs[n] = (-2 alpha)^n F_n(T) (times any common factor) -----------
template <int T, int U, int V, int N, int NF>
__host__ __device__ __forceinline__ double gto_R(const double (&Fs)[NF], double X, double Y, double Z)
{
    if constexpr (T < 0 || U < 0 || V < 0) {
        return 0.0;
    } else if constexpr (T == 0 && U == 0 && V == 0) {
        return Fs[N];
    } else if constexpr (T == 0 && U == 0) {
        double v = Z * gto_R<0, 0, V - 1, N + 1>(Fs, X, Y, Z);
        if constexpr (V > 1) v += (double)(V - 1) * gto_R<0, 0, V - 2, N + 1>(Fs, X, Y, Z);
        return v;
    } else if constexpr (T == 0) {
        double v = Y * gto_R<0, U - 1, V, N + 1>(Fs, X, Y, Z);
        if constexpr (U > 1) v += (double)(U - 1) * gto_R<0, U - 2, V, N + 1>(Fs, X, Y, Z);
        return v;
    } else {
        double v = X * gto_R<T - 1, U, V, N + 1>(Fs, X, Y, Z);
        if constexpr (T > 1) v += (double)(T - 1) * gto_R<T - 2, U, V, N + 1>(Fs, X, Y, Z);
        return v;
    }
}

template <int L>
__host__ __device__ __forceinline__ void gto_R_fill(double (&R)[L + 1][L + 1][L + 1], const double (&Fs)[L + 1], double X,
                                           double Y, double Z)
{
    static_for<L + 1>([&](auto tc) {
        static_for<L + 1>([&](auto uc) {
            static_for<L + 1>([&](auto vc) {
                constexpr int t = decltype(tc)::value, u = decltype(uc)::value, v = decltype(vc)::value;
                if constexpr (t + u + v <= L) R[t][u][v] = gto_R<t, u, v, 0>(Fs, X, Y, Z);
            });
        });
    });
}

// ---- phases of a workgroup-per-pair kernel (gto_d.hip, gto_moments.hip) ------------------------------------------------
// Every phase of those kernels is a loop "for (i = lane; i < count; i += nlane)" followed by a barrier.
// (a CPU build that runs the lanes of a workgroup as host threads, for a thread sanitizer, defines GTO_HOST_BARRIER)
__host__ __device__ __forceinline__ void gto_sync()
{
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#elif defined(GTO_HOST_BARRIER)
    GTO_HOST_BARRIER();
#endif
}
// item i of fewer items than lanes belongs to lane i (to the only lane of a CPU build)
__host__ __device__ __forceinline__ bool gto_mine(int i, int lane, int nlane) { return i % nlane == lane; }

// One index of a component array in LDS, in place: the fibres of 6 Cartesian d components (xx, xy, xz, yy, yz, zz of a
// radial part normalised for xx) become 6 normalised Cartesian functions or the 5 real solid harmonics
// xy, yz, 3z^2 - r^2, xz, x^2 - y^2 (m = -2 .. 2) in the first 5 places.  A fibre is handled by one lane.
__host__ __device__ __forceinline__ void gto_d_pass(double* a, int total, int stride, bool cartesian, int lane,
                                                    int nlane)
{
    const double r3 = 1.7320508075688772935;
    for (int i = lane; i < total; i += nlane) {
        if ((i / stride) % 6 != 0) continue;
        const double xx = a[i], xy = a[i + stride], xz = a[i + 2 * stride], yy = a[i + 3 * stride],
                     yz = a[i + 4 * stride], zz = a[i + 5 * stride];
        if (cartesian) {
            a[i + stride] = r3 * xy;
            a[i + 2 * stride] = r3 * xz;
            a[i + 4 * stride] = r3 * yz;
        } else {
            a[i] = r3 * xy;
            a[i + stride] = r3 * yz;
            a[i + 2 * stride] = zz - 0.5 * (xx + yy);
            a[i + 3 * stride] = r3 * xz;
            a[i + 4 * stride] = (0.5 * r3) * (xx - yy);
        }
    }
    gto_sync();
}

__host__ __device__ __forceinline__ double gto_pick(const double (&a)[3], int d)
{
    return d == 0 ? a[0] : (d == 1 ? a[1] : a[2]);
}

// ---- work buffer ------------------------------------------------------------------------------------------------
// int32 part: ao_off[nshell] | lists[GTO_NCLS][npair][2] (shell of higher l, shell of lower l), padded to 16 bytes;
// then pair data [batch][npair][kp][GTO_PW], pair index i (i + 1) / 2 + j (i >= j), slot ka * nprim_j + kb.
__host__ __device__ inline long gto_int_doubles(int nshell)
{
    const long npair = (long)nshell * (nshell + 1) / 2;
    const long ints = nshell + (long)GTO_NCLS * npair * 2;
    return ((ints + 1) / 2 + 1) & ~1L;
}

// what a consumer keeps of one primitive pair, oriented to ITS order of the two shells (first = higher l)
struct gto_prim_t {
    double p, P[3], cck, oo2p, fa, fb;     // fa = (exponent of the first shell) / p, fb = (second) / p
};
__host__ __device__ __forceinline__ gto_prim_t gto_load_prim(const double* e, bool swapped)
{
    const d2* e2 = reinterpret_cast<const d2*>(e);
    const d2 v0 = e2[0], v1 = e2[1], v2 = e2[2], v3 = e2[3];
    gto_prim_t q;
    q.p = v0.x; q.P[0] = v0.y; q.P[1] = v1.x; q.P[2] = v1.y; q.cck = v2.x; q.oo2p = v2.y;
    q.fa = swapped ? v3.y : v3.x;
    q.fb = swapped ? v3.x : v3.y;
    return q;
}

struct gto_pair_ref_t {
    int sa, sb;                 // shells (l of sa >= l of sb)
    int oa, ob;                 // their AO offsets
    int nprim;                  // primitive pairs
    bool swapped;               // sa < sb: the stored orientation is (sb, sa)
    double AB[3];               // A - B
    const double* data;
};
__host__ __device__ __forceinline__ gto_pair_ref_t gto_pair_ref(const int* lists, int cls, int k, long npair, const int* iw,
                                                       const int* shells, const double* xyz, const double* pairs_g,
                                                       int kp)
{
    gto_pair_ref_t r;
    r.sa = lists[((long)cls * npair + k) * 2];
    r.sb = lists[((long)cls * npair + k) * 2 + 1];
    r.oa = iw[r.sa];
    r.ob = iw[r.sb];
    r.nprim = shells[4 * r.sa + 2] * shells[4 * r.sb + 2];
    r.swapped = r.sa < r.sb;
    const int hi = r.swapped ? r.sb : r.sa, lo = r.swapped ? r.sa : r.sb;
    r.data = pairs_g + ((size_t)hi * (hi + 1) / 2 + lo) * kp * GTO_PW;
    const double* A = xyz + 3 * shells[4 * r.sa];
    const double* B = xyz + 3 * shells[4 * r.sb];
#pragma unroll
    for (int d = 0; d < 3; ++d) r.AB[d] = A[d] - B[d];
    return r;
}

// ---- host side shared by the entry points -------------------------------------------------------------------------
static inline int gto_check_sizes(const char* who, int nshell, int max_nprim, int batch)
{
    OOVQE_REQUIRE(nshell >= 1 && nshell <= OOVQE_GTO_MAX_SHELL, "%s: nshell = %d (1 .. %d)", who, nshell,
                  OOVQE_GTO_MAX_SHELL);
    OOVQE_REQUIRE(max_nprim >= 1 && max_nprim <= OOVQE_GTO_MAX_PRIM, "%s: %d primitives per shell (1 .. %d)", who,
                  max_nprim, OOVQE_GTO_MAX_PRIM);
    OOVQE_REQUIRE(batch >= 0, "%s: batch = %d", who, batch);
    return 0;
}

// The work buffer of every entry: int part | pair data of the stack | the entry's own records.  This is the size of the
// first two; a *_work_size export adds its records, and gto_prep_t::rec is where they begin.
static inline int64_t gto_work_base(int nshell, int max_nprim, int batch)
{
    const int64_t npair = (int64_t)nshell * (nshell + 1) / 2;
    return gto_int_doubles(nshell) + (int64_t)batch * npair * max_nprim * max_nprim * GTO_PW;
}

// What every launcher of an entry needs: what gto_prepare made of the shell table and the work buffer, and the entry's
// arguments it received.  A launcher takes this and the arguments of its own kernel.
struct gto_prep_t {
    int cnt[GTO_NCLS];          // shell pairs per class
    int kp;                     // slots per shell pair of the pair data (largest primitive count squared)
    int batch;
    int* iw;                    // ao_off | class lists
    double* pairs;              // pair data [batch][npair][kp][GTO_PW]
    double* rec;                // the entry's own records, behind the pair data
    const char* who;            // the entry, as its messages name it
    const int32_t* shells; int nshell; const double* charges; int natm; const double* coords; int nao; hipStream_t st;
    long npair() const { return (long)nshell * (nshell + 1) / 2; }
};
int gto_prepare(const char* who, int max_l, int nshell, const int32_t* shells, int nprim_total, const double* exps,
                const double* coefs, int natm, const double* charges, int batch, const double* coords, int nao,
                double* nuc, double* work, hipStream_t st, gto_prep_t* p);
// The read-back of the shell table (16 bytes per shell, once per call) and the checks of every shell against the
// limits, in the order and with the messages of gto_prepare, which uses it; so does the cross overlap, which has no work
// buffer.  tab receives the table [nshell][4].
int gto_read_shells(const char* who, int max_l, int nshell, const int32_t* shells, int nprim_total, int natm, int nao,
                    hipStream_t st, std::vector<int32_t>* tab);
// the classes with a d shell (gto_d.hip)
int gto_d_launch_one_electron(const gto_prep_t& p, double* overlap, double* h_ao);
int gto_d_launch_two_electron(const gto_prep_t& p, double* g_ao);

// ---- grid of a launch ---------------------------------------------------------------------------------------------
// one workgroup per item (the kernels of the d classes) ...
static inline int gto_grid_wg(const char* who, long items, unsigned* grid)
{
    OOVQE_REQUIRE(items < (1L << 31), "%s: %ld workgroups in one launch", who, items);
    *grid = (unsigned)items;
    return 0;
}
// ... or GTO_SPLIT lanes per item in workgroups of GTO_NT (the s/p kernels)
static inline int gto_grid_split(const char* who, long items, unsigned* grid)
{
    return gto_grid_wg(who, (items * GTO_SPLIT + GTO_NT - 1) / GTO_NT, grid);
}
// quartets of a bra class of nbra pairs and a ket class of nket pairs (bra pair >= ket pair within one class)
static inline long gto_quartets(bool same, long nbra, long nket) { return same ? nbra * (nbra + 1) / 2 : nbra * nket; }

// ---- the class lists, in launch order -------------------------------------------------------------------------------
// A pair class <la, lb> or a quartet class <la, lb, lc, ld> as a value: a launcher deduces its template arguments from it.
template <int... L> struct gto_cls_t {};
// f(class) for every class in turn, up to the first return code that is not 0
template <class F, class... C> int gto_each(F&& f, C... c)
{
    int rc = 0;
    (void)(((rc = f(c)) == 0) && ...);
    return rc;
}
template <class F> int gto_sp_pairs(F&& f) { return gto_each(f, gto_cls_t<0, 0>{}, gto_cls_t<1, 0>{}, gto_cls_t<1, 1>{}); }
template <class F> int gto_d_pairs(F&& f) { return gto_each(f, gto_cls_t<2, 2>{}, gto_cls_t<2, 1>{}, gto_cls_t<2, 0>{}); }
// all pair classes, the long workgroups of the d classes first (moments, cross overlap) ...
template <class F> int gto_pairs_d_first(F&& f)
{
    const int rc = gto_d_pairs(f);
    return rc != 0 ? rc : gto_sp_pairs(f);
}
// ... or descending (point charges)
template <class F> int gto_pairs_descending(F&& f)
{
    const int rc = gto_d_pairs(f);
    return rc != 0 ? rc : gto_each(f, gto_cls_t<1, 1>{}, gto_cls_t<1, 0>{}, gto_cls_t<0, 0>{});
}
// the s/p quartets: bra class >= ket class; the long threads of (pp|pp) first, the most numerous (and cheapest) last
template <class F> int gto_sp_quartets(F&& f)
{
    return gto_each(f, gto_cls_t<1, 1, 1, 1>{}, gto_cls_t<1, 1, 1, 0>{}, gto_cls_t<1, 1, 0, 0>{}, gto_cls_t<1, 0, 1, 0>{},
                    gto_cls_t<1, 0, 0, 0>{}, gto_cls_t<0, 0, 0, 0>{});
}
