// Strength of the fine-level couplings for the aggregation by operator strength (amg_aggregation = 1; sns_export
// SNS_EXPORT_STRENGTH): for every block slot (i, j) of the fp64 BSR operator
//     s_ij = || D_i^-1/2 A_ij D_j^-1/2 ||_F,   D = |point diagonal| of the node's four dofs,
// in fp32; the diagonal slot and every coupling of a Dirichlet dof are 0 (its row and column are unit / zero already).  The
// balanced basis makes the measure independent of the scaling of the dofs: a plain norm only reports the 1/h of the velocity-
// pressure coupling, not slivers (profiles/r3_local_damping_experiment.txt).
//   k_strength_scale  one lane per dof: d^-1/2 of the point diagonal (0 for a zero diagonal), owned rows; the ghost rows'
//                     values come from the owners by the level-0 halo exchange
//   k_strength        ONE pass over the matrix: 8 lanes per block row as in k_spmv (lane = row r of the 4 x 4 block, half hf of
//                     its columns; one 16-B load each, 128 B per block), a shuffle reduction over the 8 lanes, 4 B written per block
#include "sns_ctx.h"

namespace sns {

typedef double strength_f64x2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void k_strength_scale(int32_t n_rows, const int32_t* __restrict__ diag,
                                                        const double* __restrict__ vals, double* __restrict__ scale) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 4 * (int64_t)n_rows) return;
    const int32_t row = (int32_t)(t >> 2);
    const int c = (int)(t & 3);
    const double d = fabs(vals[(int64_t)diag[row] * 16 + 5 * c]);
    scale[t] = d > 0.0 ? 1.0 / sqrt(d) : 0.0;
}

__global__ __launch_bounds__(256) void k_strength(int32_t n_rows, const int32_t* __restrict__ rowptr,
                                                  const int32_t* __restrict__ colind, const double* __restrict__ vals,
                                                  const double* __restrict__ scale, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int t = lane & 7;
    const int r = t >> 1, hf = t & 1;
    const int32_t row = (int32_t)(((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 8 + (lane >> 3));
    const bool live = row < n_rows;
    const int32_t s = live ? rowptr[row] : 0, e = live ? rowptr[row + 1] : 0;
    const double si = live ? scale[4 * (int64_t)row + r] : 0.0;
    const double2* __restrict__ vp = reinterpret_cast<const double2*>(vals) + ((int64_t)s * 8 + r * 2 + hf);
    // the 8 lanes of a row run the same trip count; rows of one wave differ, so the loop runs to the wave's longest row
    // with the shorter rows masked (their shuffles still take part, on zeros)
    int32_t len = e - s;
#pragma unroll
    for (int off = 8; off < 64; off <<= 1) len = max(len, __shfl_xor(len, off));
    for (int32_t k = 0; k < len; ++k) {
        const bool in = k < e - s;
        double q = 0.0;
        int32_t col = row;
        if (in) {
            col = colind[s + k];
            const strength_f64x2 a = __builtin_nontemporal_load(reinterpret_cast<const strength_f64x2*>(vp + 8 * (int64_t)k));
            const double2 sj = *reinterpret_cast<const double2*>(scale + 4 * (int64_t)col + 2 * hf);
            const double x = si * a.x * sj.x, y = si * a.y * sj.y;
            q = x * x + y * y;
        }
        q += __shfl_xor(q, 1);
        q += __shfl_xor(q, 2);
        q += __shfl_xor(q, 4);
        if (in && t == 0) out[s + k] = col == row ? 0.0f : (float)sqrt(q);
    }
}

// out[nnzb of level 0] <- the strength of the current fine-level operator (owned rows; ghost rows' slots 0).  Collective on a
// partitioned handle (one halo exchange of the scales).  `scale` = caller's scratch of 4 * n doubles.
int compute_strength(sns_ctx* h, float* out, double* scale) {
    const Level& L = h->levels[0];
    const int32_t n_own = h->n_owned;
    if (L.nnzb > 0) HIP_TRY(hipMemsetAsync(out, 0, (size_t)L.nnzb * sizeof(float), h->stream));
    HIP_TRY(hipMemsetAsync(scale, 0, 4 * (size_t)L.n * sizeof(double), h->stream));
    if (n_own > 0)
        hipLaunchKernelGGL(k_strength_scale, dim3((unsigned)((4 * (int64_t)n_own + 255) / 256)), dim3(256), 0, h->stream, n_own,
                           L.diag, L.vals, scale);
    Comm* c = h->comm.get();
    if (c && c->active() && c->nranks > 1) SNS_TRY(comm_exchange(c, c->plans[0], scale, h->stream));
    if (n_own > 0)
        hipLaunchKernelGGL(k_strength, dim3((unsigned)((n_own + 31) / 32)), dim3(256), 0, h->stream, n_own, L.rowptr, L.colind,
                           L.vals, scale, out);
    HIP_TRY(hipGetLastError());
    return SNS_OK;
}

}  // namespace sns
