// The excitation tables of the strings of a particle-number sector, shared by the kernels of sector.hip and
// sector_trdm.hip.  E_pq = E^alpha_pq + E^beta_pq, and on the determinant (ia, ib)
//   (E^alpha_pq v)[ia, ib] = (-1)^(own_a(ia) + cross_b(ib)) v[src_a(ia), ib]     if valid_a(ia)
// (sector.hip, "Excitation tables of the strings", explains the four fields).  One 16-bit word per (string, pq):
// source index (11 bits) | valid << 11 | own parity << 12 | cross parity << 13.
#pragma once
#include "common.h"

static __device__ __forceinline__ uint32_t sec_orb_mask(int a, int r1, int r2)     // orbitals r1 .. r2 of a string
{
    return r2 < r1 ? 0u : (((1u << (r2 - r1 + 1)) - 1u) << (a - 1 - r2));
}

// tab[pq * nstr + (string index)]; is_alpha selects which cross range the string serves
static __device__ void sec_build_table(const uint32_t* __restrict__ unrank, const int32_t* __restrict__ rank, int nstr,
                                int a, bool is_alpha, uint16_t* __restrict__ tab, int nthreads)
{
    const int na2 = a * a;
    for (int idx = threadIdx.x; idx < nstr * na2; idx += nthreads) {
        const int is = idx / na2, pq = idx - is * na2, p = pq / a, q = pq - p * a;
        const uint32_t st = unrank[is];
        const uint32_t bp = 1u << (a - 1 - p), bq = 1u << (a - 1 - q);
        const int lo = p < q ? p : q, hi = p < q ? q : p;
        uint32_t valid, src;
        if (p == q) { valid = (st & bp) ? 1u : 0u; src = (uint32_t)is; }
        else {
            valid = ((st & bp) && !(st & bq)) ? 1u : 0u;
            src = valid ? (uint32_t)rank[(st & ~bp) | bq] : 0u;
        }
        const uint32_t own = __popc(st & sec_orb_mask(a, lo + 1, hi - 1)) & 1u;
        // the range of THIS spin's electrons that an excitation of the OTHER spin crosses
        const uint32_t cross = is_alpha ? (__popc(st & sec_orb_mask(a, lo + 1, hi)) & 1u)
                                        : (__popc(st & sec_orb_mask(a, lo, hi - 1)) & 1u);
        // operator-major: the lanes of a wave hold consecutive beta strings and read one operator's word each
        // (string-major, 128 bytes apart, all 64 reads fell on two LDS banks)
        tab[pq * nstr + is] = (uint16_t)(src | (valid << 11) | (own << 12) | (cross << 13));
    }
}
