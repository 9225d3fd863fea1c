// The bodies of the potential kernel (auto_oo_amd/csrc/gto_potential.hip) run on the CPU: a stand-alone program, no
// device and no HIP runtime call.  tests/test_potential_cpu.py builds it and compares its output with the host twin
// (gaussian.potential_from_table).  Plain, a workgroup is one lane and a chunk one point; built with
// -DGTO_POT_THREADS=8 (and, say, -fsanitize=thread or -fsanitize=address) the lanes of every workgroup are host threads
// with a real barrier in place of __syncthreads and a chunk has that many points.
//
//   hipcc --cuda-host-only -O2 -std=c++17 -I auto_oo_amd/csrc -I include tools/gto_potential_host.hip -o gto_potential_host
//   gto_potential_host input.txt output.txt
//
// input: nshell natm batch nao nset npoint field nuc_mask nprim_total | shells [nshell][4] | exps | coefs | charges [natm] |
// coords [batch][natm][3] (Bohr) | dm [batch][nset][nao][nao] | points [batch][npoint][3] (Bohr); output: phi
// [batch][nset][npoint], then (field) F [batch][nset][npoint][3], one number per line (%.17g).
// The AO offsets, class lists and pair data are made here on the host by the formulas of gto_setup_kernel and
// gto_pair_kernel (the orientation and slot order of a pair are what gto_pair_ref / gto_load_prim read back).
#include <pthread.h>
#ifdef GTO_POT_THREADS
static pthread_barrier_t g_barrier;
#define GTO_HOST_BARRIER() pthread_barrier_wait(&g_barrier)
#endif
#define GTO_POTENTIAL_BODIES_ONLY
#include "gto_potential.hip"

#include <cstdio>
#include <cstdlib>
#include <thread>

namespace {
struct problem_t {
    int nshell, natm, batch, nao, nset, npoint, field, nprim_total, kp;
    unsigned nuc_mask;
    std::vector<int> shells, iw, cnt;
    std::vector<double> exps, coefs, charges, coords, dm, points, pairs, phi, F;
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

template <bool FIELD> void run(problem_t& q)
{
#ifdef GTO_POT_THREADS
    const int nlane = GTO_POT_THREADS;
#else
    const int nlane = 1;
#endif
    const int nchunk = (q.npoint + nlane - 1) / nlane;
    std::vector<double> acc((size_t)q.nset * 4 * nlane);
    for (int g = 0; g < q.batch; ++g)
        for (int chunk = 0; chunk < nchunk; ++chunk) {
            static gto_pot_lds_t lds;
            auto lane_fn = [&](int lane) {
                gto_pot_body<FIELD>(chunk, g, lane, nlane, lds, acc.data(), q.iw.data(), q.shells.data(), q.nshell,
                                    q.cnt[gto_cls(0, 0)], q.cnt[gto_cls(1, 0)], q.cnt[gto_cls(1, 1)], q.cnt[gto_cls(2, 0)],
                                    q.cnt[gto_cls(2, 1)], q.cnt[gto_cls(2, 2)], q.charges.data(), q.natm, q.coords.data(),
                                    q.pairs.data(), q.kp, q.nao, q.nset, q.dm.data(), q.npoint, q.points.data(),
                                    q.nuc_mask, q.phi.data(), q.F.data());
            };
#ifdef GTO_POT_THREADS
            pthread_barrier_init(&g_barrier, nullptr, nlane);
            std::vector<std::thread> lanes;
            for (int l = 0; l < nlane; ++l) lanes.emplace_back(lane_fn, l);
            for (auto& t : lanes) t.join();
            pthread_barrier_destroy(&g_barrier);
#else
            lane_fn(0);
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
    if (fscanf(f, "%d %d %d %d %d %d %d %u %d", &q.nshell, &q.natm, &q.batch, &q.nao, &q.nset, &q.npoint, &q.field,
               &q.nuc_mask, &q.nprim_total) != 9) return 2;
    if (q.nset < 1 || q.nset > POT_KMAX || q.npoint < 1) { fprintf(stderr, "nset = %d, npoint = %d\n", q.nset, q.npoint); return 2; }
    read_n(f, q.shells, (size_t)q.nshell * 4, "%d");
    read_n(f, q.exps, q.nprim_total, "%lf");
    read_n(f, q.coefs, q.nprim_total, "%lf");
    read_n(f, q.charges, q.natm, "%lf");
    read_n(f, q.coords, (size_t)q.batch * q.natm * 3, "%lf");
    read_n(f, q.dm, (size_t)q.batch * q.nset * q.nao * q.nao, "%lf");
    read_n(f, q.points, (size_t)q.batch * q.npoint * 3, "%lf");
    fclose(f);
    prepare(q);
    // NaN everywhere first: an element no body writes shows in the comparison
    q.phi.assign((size_t)q.batch * q.nset * q.npoint, __builtin_nan(""));
    q.F.assign(q.phi.size() * 3, __builtin_nan(""));
    if (q.field) run<true>(q); else run<false>(q);
    FILE* o = fopen(argv[2], "w");
    if (!o) { perror(argv[2]); return 2; }
    for (double x : q.phi) fprintf(o, "%.17g\n", x);
    if (q.field)
        for (double x : q.F) fprintf(o, "%.17g\n", x);
    fclose(o);
    return 0;
}
