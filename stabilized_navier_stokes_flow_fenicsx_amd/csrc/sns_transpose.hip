// In-place transpose of the assembled fine operator (sns_transpose_operator, sns_adjoint_solve).  The P1-P1 pattern is
// structurally symmetric with sorted rows and the Dirichlet rule zeroes rows AND columns, so A^T has the rowptr / colind of A:
// block (i, j) of A^T is the transposed 4 x 4 block of slot (j, i).  Transposing is a permutation of vals -- no second matrix --
// and everything downstream (low-precision copies, M = A P, the Galerkin products, D^-1 / B^-1, the spectral estimates, the
// Krylov methods) reads the fine operator by value only: P^T A^T P = (P^T A P)^T, the hierarchy of the flipped values is the
// hierarchy of the adjoint operator.
//   k_partner_slot       one lane per slot s = (i, j): binary search for column i in row j's sorted colind -> partner[s] = slot
//                        (j, i), or -1 and the device flag where the pattern is not symmetric.  Built once per handle.
//   k_transpose_inplace  16 lanes per slot, lane (r, c).  The group of a slot s <= partner[s] = p loads entry (c, r) of both
//                        blocks (one 128-B line each, lanes permuted inside the line) and stores entry (r, c) of the OTHER block
//                        (lane-contiguous, one full line per store); a diagonal slot (p == s) is transposed in place.  The groups
//                        of the slots s > p retire after reading partner[s].  A block is read and written by the 16 lanes of ONE
//                        group, i.e. of one wave: every load of the pair is waited for before the first store issues, and no
//                        other group touches the pair, so the result does not depend on the launch order -- plain vector loads
//                        and stores, no atomics, bitwise reproducible, and a second application restores vals bit for bit.
//                        Algorithmic bytes: 2 x 128 B per block (read + write of vals) + 4 B per slot of partner.
#include "sns_ctx.h"

namespace sns {

__global__ __launch_bounds__(256) void k_partner_slot(int64_t nnzb, int32_t n_rows, const int32_t* __restrict__ rowptr,
                                                      const int32_t* __restrict__ colind, const int32_t* __restrict__ slot_row,
                                                      int32_t* __restrict__ partner, int* __restrict__ bad) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nnzb) return;
    const int32_t i = slot_row[s], j = colind[s];
    int32_t p = -1;
    if (j >= 0 && j < n_rows) {
        const int32_t end = rowptr[j + 1];
        int32_t lo = rowptr[j], hi = end;
        while (lo < hi) {                                // first slot of row j whose column is >= i
            const int32_t mid = lo + ((hi - lo) >> 1);
            if (colind[mid] < i) lo = mid + 1;
            else hi = mid;
        }
        if (lo < end && colind[lo] == i) p = lo;
    }
    partner[s] = p;
    if (p < 0) *bad = 1;                                 // (every lane that misses stores the same value)
}

__global__ __launch_bounds__(256) void k_transpose_inplace(int64_t nnzb, const int32_t* __restrict__ partner, double* vals) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t s = t >> 4;
    if (s >= nnzb) return;
    const int64_t p = partner[s];
    if (p < s) return;                                   // the lower slot of a pair moves both blocks
    const int e = (int)(t & 15);                         // entry (r, c) = (e >> 2, e & 3)
    const int et = ((e & 3) << 2) | (e >> 2);            // entry (c, r)
    double* A = vals + 16 * s;
    double* B = vals + 16 * p;
    const double a = A[et];
    const double b = B[et];
    // both loads of every lane of the wave have returned before any store of the pair issues (the first store's own data
    // dependence would cover `a` alone)
    __builtin_amdgcn_s_waitcnt(0);
    if (p != s) B[e] = a;
    A[e] = b;
}

// flips levels[0].vals between A and A^T.  Nothing is modified when it fails with SNS_E_STATE / SNS_E_MESH.
int transpose_operator(sns_ctx* h) {
    if (!h->has_matrix) { set_error("sns_transpose_operator before a matrix was assembled"); return SNS_E_STATE; }
    if (h->comm) {
        set_error("sns_transpose_operator: partitioned handles are not supported (a rank's ghost rows are not complete rows of A)");
        return SNS_E_STATE;
    }
    Level& L = h->levels[0];
    if (L.nnzb <= 0) return SNS_OK;
    if (!h->tr_partner) {
        DevBuf<int32_t> partner;
        DevBuf<int> bad;
        SNS_TRY(partner.alloc((size_t)L.nnzb));
        SNS_TRY(bad.alloc(1));
        int* h_bad = reinterpret_cast<int*>(h->h_scal + 770);
        *h_bad = 0;
        hipError_t e = hipMemsetAsync(bad, 0, sizeof(int), h->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_partner_slot, dim3((unsigned)((L.nnzb + 255) / 256)), dim3(256), 0, h->stream, L.nnzb, L.n, L.rowptr,
                               L.colind, L.slot_row, partner, bad);
            e = hipMemcpyAsync(h_bad, bad, sizeof(int), hipMemcpyDeviceToHost, h->stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess || *h_bad) {
            if (e != hipSuccess) { set_error(std::string("sns_transpose_operator: ") + hipGetErrorString(e)); return SNS_E_HIP; }
            set_error("sns_transpose_operator: pattern not structurally symmetric");
            return SNS_E_MESH;
        }
        h->tr_partner = std::move(partner);
    }
    hipLaunchKernelGGL(k_transpose_inplace, dim3((unsigned)((L.nnzb * 16 + 255) / 256)), dim3(256), 0, h->stream, L.nnzb,
                       h->tr_partner, L.vals);
    h->transposed = !h->transposed;
    h->matrix_key.transposed = h->transposed;            // (the damping caps were taken on the other operator)
    pc_stale(h);
    HIP_TRY(hipGetLastError());
    return sync_stream(h);
}

}  // namespace sns
