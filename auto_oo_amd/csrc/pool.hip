// ADAPT-VQE pool gradients: the energy derivative with respect to every operator of a pool
// that could be appended to the circuit, at the current state, for a stack of states in ONE launch.
//
// A gate of the table (oovqe_gate_t) rotates the determinant pairs (x, y) of its pair list (oovqe_sector_pairs) by
// sign * theta / 2; appended behind the circuit with its parameter at 0 its derivative is
//     g = sum over the pairs (sign / 2) pi(x) (psi[y] lam[x] - psi[x] lam[y]),     lam = (Hop + Hop^T) psi,
// and an operator of the pool is one parameter driving the gates op_first[k] .. op_first[k + 1] - 1: the sum of theirs.
//
// Layout: grid = (operator tile, state), 256 threads.  psi and lam of the workgroup's state are staged in LDS when both
// fit (POOL_LDS_BYTES: CAS(8e,8o), 2 x 4 900 doubles, two workgroups per CU) and read through L2 otherwise; the pair
// lists are shared by all states and streamed.  One wave takes one operator at a time: the lanes stride the pairs of
// its gates in list order, a butterfly over the wave adds the 64 partial sums in a fixed order, lane 0 stores the
// result.  No atomics: a result has the same bits wherever its state stands in the stack, whatever the tile width the
// host picked and whatever stream it runs on (the convention of gto_grad.hip).
#include "common.h"

constexpr int POOL_THREADS = 256;
constexpr int POOL_WAVES = POOL_THREADS / 64;
constexpr size_t POOL_LDS_BYTES = 80 * 1024;      // psi | lam of one state; two workgroups per CU

__device__ __forceinline__ double pool_wave_sum(double x)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// pairs: [n_gates] counts | [n_gates][stride] words d | e << 15 | parity << 31 (oovqe_sector_pairs)
template <bool IN_LDS>
__global__ __launch_bounds__(POOL_THREADS)
void pool_gradients_kernel(const double* __restrict__ psi_c, const double* __restrict__ lam, int Dc,
                           const uint32_t* __restrict__ pairs, int n_gates, int stride,
                           const int32_t* __restrict__ op_first, const int32_t* __restrict__ gate_sign, int n_ops,
                           int tile, double* __restrict__ out)
{
    extern __shared__ double pool_lds[];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* psi = psi_c + (size_t)b * Dc;
    const double* lm = lam + (size_t)b * Dc;
    if (IN_LDS) {
        for (int d = tid; d < Dc; d += POOL_THREADS) {
            pool_lds[d] = psi[d];
            pool_lds[Dc + d] = lm[d];
        }
        __syncthreads();
        psi = pool_lds;
        lm = pool_lds + Dc;
    }
    const int op0 = blockIdx.x * tile;
    const int op1 = op0 + tile < n_ops ? op0 + tile : n_ops;
    for (int op = op0 + wave; op < op1; op += POOL_WAVES) {
        int g0 = op_first[op], g1 = op_first[op + 1];
        if (g0 < 0) g0 = 0;
        if (g1 > n_gates) g1 = n_gates;
        double acc = 0.0;
        for (int g = g0; g < g1; ++g) {
            int cnt = (int)pairs[g];
            if (cnt > stride) cnt = stride;
            const uint32_t* list = pairs + n_gates + (size_t)g * stride;
            const double half = 0.5 * (double)gate_sign[g];
            for (int i = lane; i < cnt; i += 64) {
                const uint32_t w = list[i];
                const int d = (int)(w & 0x7FFFu), e = (int)((w >> 15) & 0x7FFFu);
                if (d < Dc && e < Dc) {       // (a list made for another sector never reads outside the vectors)
                    const double t = psi[e] * lm[d] - psi[d] * lm[e];
                    acc += ((w >> 31) ? -half : half) * t;
                }
            }
        }
        acc = pool_wave_sum(acc);
        if (lane == 0) out[(size_t)b * n_ops + op] = acc;
    }
}

static int pool_check(const char* who, int na, int nb, int batch, int n_gates, int n_ops)
{
    OOVQE_REQUIRE(na >= 1 && nb >= 1 && (long)na * nb <= 32767,
                  "%s: %ld determinants (pair lists hold at most 32 767)", who, (long)na * nb);
    OOVQE_REQUIRE(batch >= 1 && batch <= 65535, "%s: batch = %d (1 .. 65535)", who, batch);
    OOVQE_REQUIRE(n_ops >= 1 && n_gates >= n_ops && n_gates <= 65535,
                  "%s: %d operators of %d gates (1 <= operators <= gates <= 65535)", who, n_ops, n_gates);
    return 0;
}

extern "C" int oovqe_pool_gradients_batch(const double* psi_c, const double* lam, int na, int nb, int batch,
                                          const uint32_t* pairs, int n_gates, const int32_t* op_first,
                                          const int32_t* gate_sign, int n_ops, double* out, oovqe_stream_t stream)
{
    OOVQE_REQUIRE(psi_c && lam && pairs && op_first && gate_sign && out, "pool_gradients: null pointer");
    int rc;
    if ((rc = pool_check("pool_gradients", na, nb, batch, n_gates, n_ops))) return rc;
    const int Dc = na * nb;
    const int stride = (int)(oovqe_sector_pairs_size(n_gates, na, nb) / n_gates) - 1;
    // tile: operators per workgroup -- wide enough to repay the staging of psi and lam, narrow enough that one state
    // with a pool of thousands still gives every CU two workgroups
    const long want = 2L * oovqe_cu_count();
    long tile = ((long)n_ops * batch + want - 1) / want;
    tile = (tile + POOL_WAVES - 1) / POOL_WAVES * POOL_WAVES;
    if (tile < POOL_WAVES) tile = POOL_WAVES;
    const unsigned ntile = (unsigned)((n_ops + tile - 1) / tile);
    const size_t lds = 2 * (size_t)Dc * sizeof(double);
    const dim3 grid(ntile, (unsigned)batch);
    if (lds <= POOL_LDS_BYTES) {
        if ((rc = oovqe_ensure_dynamic_lds((const void*)pool_gradients_kernel<true>, lds))) return rc;
        hipLaunchKernelGGL(pool_gradients_kernel<true>, grid, dim3(POOL_THREADS), lds, (hipStream_t)stream, psi_c, lam,
                           Dc, pairs, n_gates, stride, op_first, gate_sign, n_ops, (int)tile, out);
    } else {
        hipLaunchKernelGGL(pool_gradients_kernel<false>, grid, dim3(POOL_THREADS), 0, (hipStream_t)stream, psi_c, lam,
                           Dc, pairs, n_gates, stride, op_first, gate_sign, n_ops, (int)tile, out);
    }
    OOVQE_CHECK_LAUNCH("pool_gradients");
    return 0;
}

// work: lam [batch][Dc] (rounded up to 64 doubles), then the workspace of the sector engine's operator
static int64_t pool_lam_doubles(int na, int nb, int batch) { return ((int64_t)batch * na * nb + 63) / 64 * 64; }

extern "C" int64_t oovqe_pool_gradients_from_coefficients_work_size(int ncas, int na, int nb, int batch)
{
    if (ncas < 1 || na < 1 || nb < 1 || batch < 1) return 0;
    return pool_lam_doubles(na, nb, batch) + oovqe_sector_work_size(ncas, na, nb, batch);
}

// The whole step for a stack in one call: lam[b] = (Hop_b + Hop_b^T) psi[b] with the coefficients of geometry b at
// c1 + b c_stride, c2 + b c_stride, then the kernel above.  Where the sector engine serves per-geometry coefficients
// in one launch sequence (oovqe_sector_geometry_coefficients_ok) that is oovqe_sector_lambda_pg; elsewhere the
// geometries are looped over here, one oovqe_sector_lambda each on the same workspace (in stream order).
extern "C" int oovqe_pool_gradients_from_coefficients_batch(
    const double* psi_c, int ncas, const uint32_t* unrank_a, const uint32_t* unrank_b, const int32_t* rank_a,
    const int32_t* rank_b, int na, int nb, int batch, const double* c1, const double* c2, int64_t c_stride,
    const uint16_t* tabs, const uint32_t* pairs, int n_gates, const int32_t* op_first, const int32_t* gate_sign,
    int n_ops, double* work, double* out, oovqe_stream_t stream)
{
    OOVQE_REQUIRE(psi_c && unrank_a && unrank_b && rank_a && rank_b && c1 && c2 && pairs && op_first && gate_sign &&
                  work && out, "pool_gradients_from_coefficients: null pointer");
    OOVQE_REQUIRE(ncas >= 1 && ncas <= 13 && (batch == 1 || c_stride > 0),
                  "pool_gradients_from_coefficients: ncas = %d, stride %ld", ncas, (long)c_stride);
    int rc;
    if ((rc = pool_check("pool_gradients_from_coefficients", na, nb, batch, n_gates, n_ops))) return rc;
    const size_t Dc = (size_t)na * nb;
    double* lam = work;
    double* swork = work + pool_lam_doubles(na, nb, batch);
    if (oovqe_sector_geometry_coefficients_ok(ncas, na, nb)) {
        if ((rc = oovqe_sector_lambda_pg(psi_c, ncas, unrank_a, unrank_b, rank_a, rank_b, na, nb, batch, 1, c1, c2,
                                         c_stride > 0 ? c_stride : 1, tabs, swork, lam, stream)))
            return rc;
    } else {
        for (int b = 0; b < batch; ++b)
            if ((rc = oovqe_sector_lambda(psi_c + b * Dc, ncas, unrank_a, unrank_b, rank_a, rank_b, na, nb, 1,
                                          c1 + (size_t)b * c_stride, c2 + (size_t)b * c_stride, tabs, swork,
                                          lam + b * Dc, stream)))
                return rc;
    }
    return oovqe_pool_gradients_batch(psi_c, lam, na, nb, batch, pairs, n_gates, op_first, gate_sign, n_ops, out,
                                      stream);
}
