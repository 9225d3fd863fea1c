// The determinant and sign routines of the sector-overlap kernel (auto_oo_amd/csrc/overlap.hip) run on the CPU: a
// stand-alone program, no device and no HIP runtime call.  tests/test_overlaps_cpu.py builds it and compares its output
// with mpmath.det and berry.sector_tables; built with -fsanitize=address,undefined it checks the routines' indexing.
//
//   hipcc --cuda-host-only -O2 -std=c++17 -I auto_oo_amd/csrc -I include tools/overlap_host.hip -o overlap_host
//   overlap_host input.txt output.txt
//
// input, any number of records: ncas K n1 n2 | U [ncas][ncas] | list1 [n1] | list2 [n2] (occupation strings, orbital p at
// bit ncas - 1 - p).  output per record, one number per line (%.17g): for K >= 0 the minors det U[occ(list1[j]),
// occ(list2[i])], [n1][n2], of order K (every string must have K bits), through the switch of the kernel; then the signs
// ovl_sign(list1[a], list2[b]), [n1][n2].  K = -1 writes the signs alone.
#define OVERLAP_BODIES_ONLY
#include "overlap.hip"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {
// the switch of ovl_minors_of
double minor_of(int k, const double* U, int ncas, unsigned mj, unsigned mi)
{
    switch (k) {
        case 0: return ovl_minor<0>(U, ncas, mj, mi);
        case 1: return ovl_minor<1>(U, ncas, mj, mi);
        case 2: return ovl_minor<2>(U, ncas, mj, mi);
        case 3: return ovl_minor<3>(U, ncas, mj, mi);
        case 4: return ovl_minor<4>(U, ncas, mj, mi);
        case 5: return ovl_minor<5>(U, ncas, mj, mi);
        case 6: return ovl_minor<6>(U, ncas, mj, mi);
        case 7: return ovl_minor<7>(U, ncas, mj, mi);
        default: return ovl_minor<8>(U, ncas, mj, mi);
    }
}

void read_strings(FILE* f, std::vector<unsigned>& v, int n, int ncas, int K)
{
    v.resize(n);
    for (int i = 0; i < n; ++i) {
        if (fscanf(f, "%u", &v[i]) != 1) { fprintf(stderr, "short input\n"); exit(2); }
        if (v[i] >> ncas || (K >= 0 && __builtin_popcount(v[i]) != K)) {
            fprintf(stderr, "string %u: not %d of %d orbitals\n", v[i], K, ncas);
            exit(2);
        }
    }
}
}  // namespace

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s input output\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    FILE* o = fopen(argv[2], "w");
    if (!o) { perror(argv[2]); return 2; }
    int ncas, K, n1, n2;
    while (fscanf(f, "%d %d %d %d", &ncas, &K, &n1, &n2) == 4) {
        if (ncas < 1 || ncas > 8 || K < -1 || K > ncas || n1 < 0 || n2 < 0) { fprintf(stderr, "bad record\n"); return 2; }
        double U[OVL_US * OVL_US] = {};                      // the kernel's layout: row stride OVL_US, zero beyond ncas
        for (int i = 0; i < ncas; ++i)
            for (int j = 0; j < ncas; ++j)
                if (fscanf(f, "%lf", &U[i * OVL_US + j]) != 1) { fprintf(stderr, "short input\n"); return 2; }
        std::vector<unsigned> l1, l2;
        read_strings(f, l1, n1, ncas, K);
        read_strings(f, l2, n2, ncas, K);
        if (K >= 0)
            for (unsigned mj : l1)
                for (unsigned mi : l2) fprintf(o, "%.17g\n", minor_of(K, U, ncas, mj, mi));
        for (unsigned ma : l1)
            for (unsigned mb : l2) fprintf(o, "%.17g\n", ovl_sign(ma, mb));
    }
    fclose(f);
    fclose(o);
    return 0;
}
