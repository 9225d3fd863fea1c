// The bodies of the integral kernels (auto_oo_amd/csrc/gto.hip, gto_d.hip) run on the CPU: a stand-alone program, no
// device, one lane per group / workgroup.  It checks the cases of tests/_gto_edges.py against their fixtures before
// they are run on a device (tests/test_gto_edges_cpu.py builds it); built with -fsanitize=address,undefined it checks
// the bodies' indexing at 10 primitives per shell and 128 shells.
//
//   hipcc --cuda-host-only -O2 -std=c++17 -I auto_oo_amd/csrc -I include tools/gto_host.hip -o gto_host
//   gto_host input.txt output.txt
//
// input: nshell natm batch nao nprim_total with_g | shells [nshell][4] | exps | coefs | charges | coords
// [batch][natm][3] (Bohr); output: per geometry S [nao][nao], h [nao][nao], nuc, then (with_g) g [nao]^4, as raw
// doubles.  An element no body writes comes back NaN.
#define GTO_BODIES_ONLY
#include "gto.hip"
#include "gto_d.hip"

#include <cstdio>
#include <cstdlib>

namespace {
struct problem_t {
    int nshell, natm, batch, nao, nprim_total, with_g, kp;
    int cnt[GTO_NCLS];
    std::vector<int> shells, iw;
    std::vector<double> exps, coefs, charges, xyz, pairs, S, h, g, nuc;
};

template <int LA, int LB> void one_sp(problem_t& q)
{
    const int count = q.cnt[gto_cls(LA, LB)];
    for (long tid = 0; tid < (long)count * q.batch; ++tid)
        gto_one_body<LA, LB, 1>(tid, q.iw.data(), q.shells.data(), q.nshell, count, q.charges.data(), q.natm,
                                q.xyz.data(), q.batch, q.pairs.data(), q.kp, q.nao, q.S.data(), q.h.data());
}

template <int LA, int LB> void one_d(problem_t& q)
{
    const int count = q.cnt[gto_cls(LA, LB)];
    static gto_d1_lds_t<LA, LB> lds;
    for (long grp = 0; grp < (long)count * q.batch; ++grp)
        gto_d_one_body<LA, LB>(grp, 0, 1, lds, q.iw.data(), q.shells.data(), q.nshell, count, q.charges.data(), q.natm,
                               q.xyz.data(), q.batch, q.pairs.data(), q.kp, q.nao, q.S.data(), q.h.data());
}

template <int LA, int LB, int LC, int LD> void eri(problem_t& q)
{
    const int nbra = q.cnt[gto_cls(LA, LB)], nket = q.cnt[gto_cls(LC, LD)];
    const long nq = (LA == LC && LB == LD) ? (long)nbra * (nbra + 1) / 2 : (long)nbra * nket;
    if constexpr (LA == 2) {
        static gto_dq_lds_t<LA, LB, LC, LD> lds;
        for (long grp = 0; grp < nq * q.batch; ++grp)
            gto_d_eri_body<LA, LB, LC, LD>(grp, 0, 1, lds, q.iw.data(), q.shells.data(), q.nshell, nbra, nket, nq,
                                           q.xyz.data(), q.natm, q.batch, q.pairs.data(), q.kp, q.nao, q.g.data());
    } else {
        for (long tid = 0; tid < nq * q.batch; ++tid)
            gto_eri_body<LA, LB, LC, LD, 1>(tid, q.iw.data(), q.shells.data(), q.nshell, nbra, nket, nq, q.xyz.data(),
                                            q.natm, q.batch, q.pairs.data(), q.kp, q.nao, q.g.data());
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
    if (fscanf(f, "%d %d %d %d %d %d", &q.nshell, &q.natm, &q.batch, &q.nao, &q.nprim_total, &q.with_g) != 6) return 2;
    read_n(f, q.shells, (size_t)q.nshell * 4, "%d");
    read_n(f, q.exps, q.nprim_total, "%lf");
    read_n(f, q.coefs, q.nprim_total, "%lf");
    read_n(f, q.charges, q.natm, "%lf");
    read_n(f, q.xyz, (size_t)q.batch * q.natm * 3, "%lf");
    fclose(f);
    int max_nprim = 0;
    for (int s = 0; s < q.nshell; ++s) max_nprim = q.shells[4 * s + 2] > max_nprim ? q.shells[4 * s + 2] : max_nprim;
    // the work buffer at the size the library asks for, its two parts apart so that a sanitizer sees an overrun of either
    const long npair = (long)q.nshell * (q.nshell + 1) / 2;
    q.kp = max_nprim * max_nprim;
    q.iw.assign((size_t)gto_int_doubles(q.nshell) * 2, 0);
    q.pairs.assign((size_t)q.batch * npair * q.kp * GTO_PW, __builtin_nan(""));
    const double nan = __builtin_nan("");
    const size_t n2 = (size_t)q.nao * q.nao;
    q.S.assign(q.batch * n2, nan);
    q.h.assign(q.batch * n2, nan);
    q.nuc.assign(q.batch, nan);
    if (q.with_g) q.g.assign(q.batch * n2 * n2, nan);
    gto_setup_body(q.shells.data(), q.nshell, q.iw.data());
    for (int c = 0; c < GTO_NCLS; ++c) q.cnt[c] = 0;
    for (int i = 0; i < q.nshell; ++i)
        for (int j = 0; j <= i; ++j) {
            const int li = gto_l_of(q.shells[4 * i + 1]), lj = gto_l_of(q.shells[4 * j + 1]);
            q.cnt[gto_cls(li >= lj ? li : lj, li >= lj ? lj : li)] += 1;
        }
    for (long tid = 0; tid < npair * q.kp * q.batch; ++tid)
        gto_pair_body(tid, q.shells.data(), q.nshell, q.exps.data(), q.coefs.data(), q.charges.data(), q.natm,
                      q.xyz.data(), q.batch, q.kp, q.pairs.data(), q.nuc.data());
    one_d<2, 2>(q); one_d<2, 1>(q); one_d<2, 0>(q);
    one_sp<0, 0>(q); one_sp<1, 0>(q); one_sp<1, 1>(q);
    if (q.with_g) {
        eri<2, 2, 2, 2>(q); eri<2, 2, 2, 1>(q); eri<2, 2, 2, 0>(q); eri<2, 2, 1, 1>(q); eri<2, 2, 1, 0>(q);
        eri<2, 2, 0, 0>(q); eri<2, 1, 2, 1>(q); eri<2, 1, 2, 0>(q); eri<2, 1, 1, 1>(q); eri<2, 1, 1, 0>(q);
        eri<2, 1, 0, 0>(q); eri<2, 0, 2, 0>(q); eri<2, 0, 1, 1>(q); eri<2, 0, 1, 0>(q); eri<2, 0, 0, 0>(q);
        eri<1, 1, 1, 1>(q); eri<1, 1, 1, 0>(q); eri<1, 1, 0, 0>(q); eri<1, 0, 1, 0>(q); eri<1, 0, 0, 0>(q);
        eri<0, 0, 0, 0>(q);
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    bool ok = true;
    for (int g = 0; g < q.batch; ++g) {
        ok = ok && fwrite(&q.S[g * n2], sizeof(double), n2, o) == n2;
        ok = ok && fwrite(&q.h[g * n2], sizeof(double), n2, o) == n2;
        ok = ok && fwrite(&q.nuc[g], sizeof(double), 1, o) == 1;
        if (q.with_g) ok = ok && fwrite(&q.g[g * n2 * n2], sizeof(double), n2 * n2, o) == n2 * n2;
    }
    ok = fclose(o) == 0 && ok;
    if (!ok) { perror(argv[2]); return 2; }
    return 0;
}
