// The bodies of the density and orbital-value kernels (auto_oo_amd/csrc/gto_density.hip) run on the CPU: a stand-alone
// program, no device and no HIP runtime call.  tests/test_density_cpu.py builds it and compares its output with the host
// twins (gaussian.density_from_table, gaussian.orbital_values_from_table).  Plain, a workgroup is one lane and a chunk one
// point; built with -DGTO_DEN_THREADS=8 (and, say, -fsanitize=thread or -fsanitize=address) the lanes of every workgroup
// are host threads with a real barrier in place of __syncthreads and a chunk has that many points.
//
//   hipcc --cuda-host-only -O2 -std=c++17 -I auto_oo_amd/csrc -I include tools/gto_density_host.hip -o gto_density_host
//   gto_density_host input.txt output.txt
//
// input: nshell natm batch nao nset npoint grad orbitals nprim_total | shells [nshell][4] | exps | coefs |
// coords [batch][natm][3] (Bohr) | orbitals = 0: dm [batch][nset][nao][nao], 1: C [batch][nao][nset] |
// points [batch][npoint][3] (Bohr); output: rho or psi [batch][nset][npoint], then (grad) its gradient
// [batch][nset][npoint][3], one number per line (%.17g).
#include <pthread.h>
#ifdef GTO_DEN_THREADS
static pthread_barrier_t g_barrier;
#define GTO_HOST_BARRIER() pthread_barrier_wait(&g_barrier)
#endif
#define GTO_DENSITY_BODIES_ONLY
#include "gto_density.hip"

#include <cstdio>
#include <cstdlib>
#include <thread>

namespace {
struct problem_t {
    int nshell, natm, batch, nao, nset, npoint, grad, orbitals, nprim_total;
    std::vector<int> shells;
    std::vector<double> exps, coefs, coords, in, points, val, der;
};

template <bool GRAD> void run(problem_t& q)
{
#ifdef GTO_DEN_THREADS
    const int nlane = GTO_DEN_THREADS;
#else
    const int nlane = 1;
#endif
    const int nchunk = (q.npoint + nlane - 1) / nlane;
    std::vector<double> acc((size_t)q.nset * 4 * nlane), rad((size_t)q.nshell * 2 * nlane);
    for (int g = 0; g < q.batch; ++g)
        for (int chunk = 0; chunk < nchunk; ++chunk) {
            static gto_den_lds_t lds;
            auto lane_fn = [&](int lane) {
                if (q.orbitals)
                    gto_orb_body<GRAD>(chunk, g, lane, nlane, lds, acc.data(), q.shells.data(), q.nshell, q.exps.data(),
                                       q.coefs.data(), q.natm, q.coords.data(), q.nao, q.nset, q.in.data(), q.npoint,
                                       q.points.data(), q.val.data(), q.der.data());
                else
                    gto_den_body<GRAD>(chunk, g, lane, nlane, lds, acc.data(), rad.data(), q.shells.data(), q.nshell,
                                       q.exps.data(), q.coefs.data(), q.natm, q.coords.data(), q.nao, q.nset, q.in.data(),
                                       q.npoint, q.points.data(), q.val.data(), q.der.data());
            };
#ifdef GTO_DEN_THREADS
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
    if (fscanf(f, "%d %d %d %d %d %d %d %d %d", &q.nshell, &q.natm, &q.batch, &q.nao, &q.nset, &q.npoint, &q.grad,
               &q.orbitals, &q.nprim_total) != 9) return 2;
    if (q.nshell < 1 || q.nshell > OOVQE_GTO_MAX_SHELL || q.nset < 1 || q.nset > DEN_KMAX || q.npoint < 1) {
        fprintf(stderr, "nshell = %d, nset = %d, npoint = %d\n", q.nshell, q.nset, q.npoint);
        return 2;
    }
    read_n(f, q.shells, (size_t)q.nshell * 4, "%d");
    read_n(f, q.exps, q.nprim_total, "%lf");
    read_n(f, q.coefs, q.nprim_total, "%lf");
    read_n(f, q.coords, (size_t)q.batch * q.natm * 3, "%lf");
    read_n(f, q.in, (size_t)q.batch * q.nset * q.nao * (q.orbitals ? 1 : q.nao), "%lf");
    read_n(f, q.points, (size_t)q.batch * q.npoint * 3, "%lf");
    fclose(f);
    int ao = 0;
    for (int s = 0; s < q.nshell; ++s) ao += gto_nfunc(q.shells[4 * s + 1]);
    if (ao != q.nao) { fprintf(stderr, "the table has %d functions, nao = %d\n", ao, q.nao); return 2; }
    // NaN everywhere first: an element no body writes shows in the comparison
    q.val.assign((size_t)q.batch * q.nset * q.npoint, __builtin_nan(""));
    q.der.assign(q.val.size() * 3, __builtin_nan(""));
    if (q.grad) run<true>(q); else run<false>(q);
    FILE* o = fopen(argv[2], "w");
    if (!o) { perror(argv[2]); return 2; }
    for (double x : q.val) fprintf(o, "%.17g\n", x);
    if (q.grad)
        for (double x : q.der) fprintf(o, "%.17g\n", x);
    fclose(o);
    return 0;
}
