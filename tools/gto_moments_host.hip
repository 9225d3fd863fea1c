// The bodies of the moment-integral kernels (auto_oo_amd/csrc/gto_moments.hip) run on the CPU: a stand-alone program,
// no device and no HIP runtime call.  tests/test_moments_cpu.py builds it and compares its output with the host twin
// (gaussian.moment_integrals_from_table); built with -DGTO_MOM_THREADS=64 -fsanitize=thread it runs the lanes of every
// workgroup of the d classes as host threads with a real barrier in place of __syncthreads.
//
//   hipcc --cuda-host-only -O2 -std=c++17 -I auto_oo_amd/csrc -I include tools/gto_moments_host.hip -o gto_moments_host
//   gto_moments_host input.txt output.txt
//
// input: nshell natm batch nao order nprim_total | shells [nshell][4] | exps | coefs | coords [batch][natm][3] (Bohr) |
// origin [batch][3]; output: moments [batch][ncomp][nao][nao], one number per line (%.17g).
// The AO offsets, class lists and pair data are made here on the host by the formulas of gto_setup_kernel and
// gto_pair_kernel (the orientation and slot order of a pair are what gto_pair_ref / gto_load_prim read back).
#include <pthread.h>
#ifdef GTO_MOM_THREADS
static pthread_barrier_t g_barrier;
#define GTO_HOST_BARRIER() pthread_barrier_wait(&g_barrier)
#endif
#define GTO_MOMENTS_BODIES_ONLY
#include "gto_moments.hip"

#include <cstdio>
#include <cstdlib>
#include <thread>

namespace {
struct problem_t {
    int nshell, natm, batch, nao, order, nprim_total, ncomp, kp;
    std::vector<int> shells, iw, cnt;
    std::vector<double> exps, coefs, coords, origin, pairs, moments;
};

void prepare(problem_t& q)
{
    const int ns = q.nshell;
    const long npair = (long)ns * (ns + 1) / 2;
    q.iw.assign(ns + GTO_NCLS * npair * 2, 0);
    q.cnt.assign(GTO_NCLS, 0);
    int off = 0, kp = 0;
    for (int s = 0; s < ns; ++s) {
        q.iw[s] = off;
        off += gto_nfunc(q.shells[4 * s + 1]);
        kp = q.shells[4 * s + 2] > kp ? q.shells[4 * s + 2] : kp;
    }
    if (off != q.nao) { fprintf(stderr, "the table has %d functions, nao = %d\n", off, q.nao); exit(2); }
    q.kp = kp * kp;
    int* lists = q.iw.data() + ns;
    for (int i = 0; i < ns; ++i)
        for (int j = 0; j <= i; ++j) {
            const int li = gto_l_of(q.shells[4 * i + 1]), lj = gto_l_of(q.shells[4 * j + 1]);
            const int hi = li >= lj ? i : j, lo = li >= lj ? j : i;
            const int cls = gto_cls(li >= lj ? li : lj, li >= lj ? lj : li);
            lists[((long)cls * npair + q.cnt[cls]) * 2] = hi;
            lists[((long)cls * npair + q.cnt[cls]) * 2 + 1] = lo;
            q.cnt[cls] += 1;
        }
    q.pairs.assign((size_t)q.batch * npair * q.kp * GTO_PW, 0.0);
    for (int g = 0; g < q.batch; ++g)
        for (int i = 0; i < ns; ++i)
            for (int j = 0; j <= i; ++j) {
                const int ni = q.shells[4 * i + 2], nj = q.shells[4 * j + 2];
                const double* A = q.coords.data() + ((size_t)g * q.natm + q.shells[4 * i]) * 3;
                const double* B = q.coords.data() + ((size_t)g * q.natm + q.shells[4 * j]) * 3;
                const double qx = A[0] - B[0], qy = A[1] - B[1], qz = A[2] - B[2];
                for (int k = 0; k < ni * nj; ++k) {
                    const int ka = k / nj, kb = k - ka * nj;
                    const double a = q.exps[q.shells[4 * i + 3] + ka], b = q.exps[q.shells[4 * j + 3] + kb];
                    const double ca = q.coefs[q.shells[4 * i + 3] + ka], cb = q.coefs[q.shells[4 * j + 3] + kb];
                    const double p = a + b, mu = a * b / p;
                    double* o = q.pairs.data() + (((size_t)g * npair + (size_t)i * (i + 1) / 2 + j) * q.kp + k) * GTO_PW;
                    o[0] = p;
                    for (int d = 0; d < 3; ++d) o[1 + d] = (a * A[d] + b * B[d]) / p;
                    o[4] = ca * cb * exp(-mu * (qx * qx + qy * qy + qz * qz));
                    o[5] = 0.5 / p; o[6] = a / p; o[7] = b / p;
                }
            }
}

template <int LA, int LB> void run_sp(problem_t& q)
{
    const int count = q.cnt[gto_cls(LA, LB)];
    for (long tid = 0; tid < (long)count * q.batch; ++tid)
        gto_mom_body<LA, LB, 1>(tid, q.iw.data(), q.shells.data(), q.nshell, count, q.coords.data(), q.natm, q.batch,
                                q.pairs.data(), q.kp, q.nao, q.ncomp, q.origin.data(), q.moments.data());
}

template <int LA, int LB> void run_d(problem_t& q)
{
    const int count = q.cnt[gto_cls(LA, LB)];
    for (long grp = 0; grp < (long)count * q.batch; ++grp) {
        static gto_mom_lds_t<LA, LB> lds;
        auto lane_fn = [&](int lane, int nlane) {
            gto_mom_d_body<LA, LB>(grp, lane, nlane, lds, q.iw.data(), q.shells.data(), q.nshell, count,
                                   q.coords.data(), q.natm, q.batch, q.pairs.data(), q.kp, q.nao, q.ncomp,
                                   q.origin.data(), q.moments.data());
        };
#ifdef GTO_MOM_THREADS
        pthread_barrier_init(&g_barrier, nullptr, GTO_MOM_THREADS);
        std::vector<std::thread> lanes;
        for (int l = 0; l < GTO_MOM_THREADS; ++l) lanes.emplace_back(lane_fn, l, GTO_MOM_THREADS);
        for (auto& t : lanes) t.join();
        pthread_barrier_destroy(&g_barrier);
#else
        lane_fn(0, 1);
#endif
    }
}

template <class T> void read_n(FILE* f, std::vector<T>& v, size_t n, const char* fmt)
{
    v.resize(n);
    for (size_t i = 0; i < n; ++i)
        if (fscanf(f, fmt, &v[i]) != 1) { fprintf(stderr, "short input\n"); exit(2); }
}
}  // namespace

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s input output\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    problem_t q;
    if (fscanf(f, "%d %d %d %d %d %d", &q.nshell, &q.natm, &q.batch, &q.nao, &q.order, &q.nprim_total) != 6) return 2;
    if (q.order < 1 || q.order > 2) { fprintf(stderr, "order = %d\n", q.order); return 2; }
    q.ncomp = q.order == 1 ? 3 : GTO_MOM_NC;
    read_n(f, q.shells, (size_t)q.nshell * 4, "%d");
    read_n(f, q.exps, q.nprim_total, "%lf");
    read_n(f, q.coefs, q.nprim_total, "%lf");
    read_n(f, q.coords, (size_t)q.batch * q.natm * 3, "%lf");
    read_n(f, q.origin, (size_t)q.batch * 3, "%lf");
    fclose(f);
    prepare(q);
    // NaN everywhere first: an element no body writes shows in the comparison
    q.moments.assign((size_t)q.batch * q.ncomp * q.nao * q.nao, __builtin_nan(""));
    run_d<2, 2>(q); run_d<2, 1>(q); run_d<2, 0>(q);
    run_sp<0, 0>(q); run_sp<1, 0>(q); run_sp<1, 1>(q);
    FILE* o = fopen(argv[2], "w");
    if (!o) { perror(argv[2]); return 2; }
    for (double x : q.moments) fprintf(o, "%.17g\n", x);
    fclose(o);
    return 0;
}
