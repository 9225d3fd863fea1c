// The bodies of the cross-overlap kernels (auto_oo_amd/csrc/gto_cross.hip) run on the CPU: a stand-alone program, no
// device and no HIP runtime call, one lane per group / workgroup.  tests/test_overlaps_cpu.py builds it and compares its
// output with the host twin (gaussian.cross_overlap_from_table); built with -fsanitize=address,undefined it checks the
// bodies' indexing.
//
//   hipcc --cuda-host-only -O2 -std=c++17 -I auto_oo_amd/csrc -I include tools/gto_cross_host.hip -o gto_cross_host
//   gto_cross_host input.txt output.txt
//
// input: nshell natm npair nao nprim_total | shells [nshell][4] | exps | coefs | coords_a [npair][natm][3] (Bohr) |
// coords_b; output: S_ab [npair][nao][nao], one number per line (%.17g).
#define GTO_CROSS_BODIES_ONLY
#include "gto_cross.hip"

#include <cstdio>
#include <cstdlib>

namespace {
struct problem_t {
    int nshell, natm, npair, nao, nprim_total;
    std::vector<int> shells;
    std::vector<double> exps, coefs, xa, xb, out;
};

template <int LA, int LB> void run_sp(problem_t& q)
{
    for (long tid = 0; tid < (long)q.npair * q.nshell * q.nshell; ++tid)
        gto_cross_body<LA, LB, 1>(tid, q.shells.data(), q.nshell, q.exps.data(), q.coefs.data(), q.natm, q.npair,
                                  q.xa.data(), q.xb.data(), q.nao, q.out.data());
}

template <int LA, int LB> void run_d(problem_t& q)
{
    for (long grp = 0; grp < (long)q.npair * q.nshell * q.nshell; ++grp) {
        static gto_cross_lds_t<LA, LB> lds;
        gto_cross_d_body<LA, LB>(grp, 0, 1, lds, q.shells.data(), q.nshell, q.exps.data(), q.coefs.data(), q.natm,
                                 q.npair, q.xa.data(), q.xb.data(), q.nao, q.out.data());
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
    if (fscanf(f, "%d %d %d %d %d", &q.nshell, &q.natm, &q.npair, &q.nao, &q.nprim_total) != 5) return 2;
    read_n(f, q.shells, (size_t)q.nshell * 4, "%d");
    read_n(f, q.exps, q.nprim_total, "%lf");
    read_n(f, q.coefs, q.nprim_total, "%lf");
    read_n(f, q.xa, (size_t)q.npair * q.natm * 3, "%lf");
    read_n(f, q.xb, (size_t)q.npair * q.natm * 3, "%lf");
    fclose(f);
    // NaN everywhere first: an element no body writes shows in the comparison
    q.out.assign((size_t)q.npair * q.nao * q.nao, __builtin_nan(""));
    run_d<2, 2>(q); run_d<2, 1>(q); run_d<2, 0>(q);
    run_sp<0, 0>(q); run_sp<1, 0>(q); run_sp<1, 1>(q);
    FILE* o = fopen(argv[2], "w");
    if (!o) { perror(argv[2]); return 2; }
    for (double x : q.out) fprintf(o, "%.17g\n", x);
    fclose(o);
    return 0;
}
