// Spin-summed transition one-particle density matrices between sector vectors (gfx950):
//
//   gamma[n][p][q] = <bra_n| E_pq |ket_n> = sum_c bra_n[c] (E_pq ket_n)[c]
//
// for n pairs of vectors in the layout of sector.hip (c = ia * nb + ib), up to CAS(8e,8o): 4 900 determinants.  The
// matrix is NOT symmetric in (p, q) for bra != ket, and nothing here symmetrises it: its antisymmetric part is what
// the orbital-connection term of a derivative coupling contracts with.  Equal bra and ket give the gamma of
// oovqe_sector_rdms.
//
// One workgroup per pair: both vectors (2 x 39 KB) and the excitation tables of the strings (sector_tables.h, built
// by the workgroup at its start, 2 x 9 KB) lie in LDS.  The a^2 operators are dealt to the waves; the lanes of a wave
// walk the determinants 64 apart, two table words and two amplitudes per element as in sec_build_chunk, and their
// partial sums meet in a butterfly.  The order of every sum is fixed: the same bits whatever the other pairs of the
// call.
#include "sector_tables.h"

namespace {
constexpr int TRDM_THREADS = 256;
constexpr int TRDM_MAX_NCAS = 8;
constexpr int TRDM_MAX_STR = 70;               // C(8, 4)

size_t trdm_lds_bytes(int na, int nb, int ncas)
{
    const size_t Dc = (size_t)na * nb, na2 = (size_t)ncas * ncas;
    return 2 * (Dc + (Dc & 1)) * sizeof(double) + ((((size_t)na + nb) * na2 * sizeof(uint16_t) + 7) & ~(size_t)7);
}

__global__ __launch_bounds__(TRDM_THREADS) void sector_trdm_kernel(
    const double* __restrict__ bra, const double* __restrict__ ket, const uint32_t* __restrict__ unrank_a,
    const uint32_t* __restrict__ unrank_b, const int32_t* __restrict__ rank_a, const int32_t* __restrict__ rank_b,
    int na, int nb, int ncas, double* __restrict__ gamma)
{
    extern __shared__ double lds[];
    const int Dc = na * nb, na2 = ncas * ncas;
    double* kv = lds;                                   // [Dc] ket
    double* bv = kv + Dc + (Dc & 1);                    // [Dc] bra
    uint16_t* tabA = reinterpret_cast<uint16_t*>(bv + Dc + (Dc & 1));      // [a^2][na]
    uint16_t* tabB = tabA + (size_t)na2 * na;                               // [a^2][nb]
    const size_t n = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < Dc; i += TRDM_THREADS) {
        kv[i] = ket[n * Dc + i];
        bv[i] = bra[n * Dc + i];
    }
    sec_build_table(unrank_a, rank_a, na, ncas, true, tabA, TRDM_THREADS);
    sec_build_table(unrank_b, rank_b, nb, ncas, false, tabB, TRDM_THREADS);
    __syncthreads();
    for (int pq = wave; pq < na2; pq += TRDM_THREADS / 64) {
        const uint16_t* ta = tabA + pq * na;
        const uint16_t* tb = tabB + pq * nb;
        double s = 0.0;
        for (int c = lane; c < Dc; c += 64) {
            const int ia = c / nb, ib = c - ia * nb;
            const uint32_t ea = ta[ia], eb = tb[ib];
            const double va = kv[(ea & 2047u) * nb + ib], vb = kv[ia * nb + (eb & 2047u)];
            const bool sa = ((ea >> 12) ^ (eb >> 13)) & 1u, sb = ((eb >> 12) ^ (ea >> 13)) & 1u;
            const double xa = (ea & 2048u) ? (sa ? -va : va) : 0.0;
            const double xb = (eb & 2048u) ? (sb ? -vb : vb) : 0.0;
            s += bv[c] * (xa + xb);
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) gamma[n * na2 + pq] = s;
    }
}
}  // namespace

extern "C" int oovqe_sector_transition_rdm1(const double* bra, const double* ket, int ncas, const uint32_t* unrank_a,
                                            const uint32_t* unrank_b, const int32_t* rank_a, const int32_t* rank_b,
                                            int na, int nb, int npairs, double* gamma, oovqe_stream_t stream)
{
    const char* who = "oovqe_sector_transition_rdm1";
    OOVQE_REQUIRE(ncas >= 1 && ncas <= TRDM_MAX_NCAS, "%s: ncas = %d (1 .. %d)", who, ncas, TRDM_MAX_NCAS);
    OOVQE_REQUIRE(na >= 1 && na == nb && na <= TRDM_MAX_STR, "%s: %d alpha and %d beta strings (equal, 1 .. %d)", who, na,
                  nb, TRDM_MAX_STR);
    OOVQE_REQUIRE(npairs >= 0, "%s: %d pairs", who, npairs);
    if (npairs == 0) return 0;
    OOVQE_REQUIRE(bra && ket && unrank_a && unrank_b && rank_a && rank_b && gamma, "%s: null pointer", who);
    const size_t bytes = trdm_lds_bytes(na, nb, ncas);
    if (int rc = oovqe_ensure_dynamic_lds((const void*)sector_trdm_kernel, bytes)) return rc;
    hipLaunchKernelGGL(sector_trdm_kernel, dim3((unsigned)npairs), dim3(TRDM_THREADS), bytes, (hipStream_t)stream, bra,
                       ket, unrank_a, unrank_b, rank_a, rank_b, na, nb, ncas, gamma);
    OOVQE_CHECK_LAUNCH("sector_trdm_kernel");
    return 0;
}
