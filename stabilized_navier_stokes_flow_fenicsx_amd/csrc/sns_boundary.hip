// Boundary terms (sns_set_boundary_facets, sns_set_boundary_flow, sns_set_boundary_scalar; the reference has no counterpart: its
// forms are volume integrals and its outlets are do-nothing): facet integrals over a list of boundary facets the handle keeps.
// A facet k has vertices (i0, i1, i2), rewound on the host (sns_host.cpp: build_facet_lists) so that (x1 - x0) x (x2 - x0)
// points out of the tet that owns it; |Gamma_k| is half the length of that product, n_k its direction.
//   flow     R(w; v) += - int_Gamma t.v ds - int_Gamma beta_k (u.n)_- u.v ds,   (u.n)_- = min(u.n, 0)
//            t: P1 per facet (9 doubles, [vertex][component]), integrated exactly by the facet mass matrix |Gamma|/12 (1 + d_ab);
//            beta_k >= 0 per facet, the term by the 6-point degree-4 rule with positive weights (BQ_* below); its Jacobian is the
//            exact derivative of the branch each quadrature point takes, -beta [(u.n)_- du.v + H(-u.n)(du.n) u.v], in the 3 x 3
//            velocity part of the blocks (a, b) of the facet.  The pressure rows get nothing.
//   scalars  R_k(c; v) += int_Gamma (alpha_k c_k - g_k) v ds: alpha M_Gamma on the diagonal entries of the facet's blocks,
//            int g v into the right-hand side, both by the facet mass matrix.
// The three nodes of a facet lie in one tet, so every block the pass touches is in the handle's pattern; its slot is found once,
// by binary search in the sorted rows (k_boundary_slots).
//   k_boundary_flow / k_boundary_scalar  owner-computes over the boundary rows, 4 lanes per row (lane = velocity component, the
//            pressure lane idle; lane = species).  The lanes of a row walk the row's (facet, vertex) list in its fixed order,
//            recompute the facet's geometry, add to F / rhs and read-modify-write the row's OWN slots of vals -- no other row
//            touches them, and the volume passes that wrote them are earlier launches on the same stream.  No atomics, no
//            scratch, the summation order is fixed: bitwise reproducible.
// Dirichlet rule of the raw form (oracle/assemble.py): rows of constrained dofs get nothing; columns of constrained dofs are not
// stored, their product with the defect goes into the lifting here -- F += J0[:,B](g - w_B) resp. b -= A0[:,B] g -- because the
// lift kernels of the volume form recompute A0 from cells and do not know the facets.
#include "sns_ctx.h"

namespace sns {
namespace {

// the 6-point degree-4 rule on the triangle (Strang-Fix / Dunavant): points (a, a, 1 - 2a) and permutations, weights times |Gamma|
constexpr double BQ_A1 = 0.445948490915965, BQ_W1 = 0.223381589678011;
constexpr double BQ_A2 = 0.091576213509771, BQ_W2 = 0.109951743655322;

// |Gamma| and the outward unit normal of the (rewound) facet with vertices X
__device__ __forceinline__ double facet_geometry(const double X[3][3], double n[3]) {
    const double e1[3] = {X[1][0] - X[0][0], X[1][1] - X[0][1], X[1][2] - X[0][2]};
    const double e2[3] = {X[2][0] - X[0][0], X[2][1] - X[0][1], X[2][2] - X[0][2]};
    const double c0 = e1[1] * e2[2] - e1[2] * e2[1], c1 = e1[2] * e2[0] - e1[0] * e2[2], c2 = e1[0] * e2[1] - e1[1] * e2[0];
    const double len = sqrt(c0 * c0 + c1 * c1 + c2 * c2);
    const double il = 1.0 / len;
    n[0] = c0 * il; n[1] = c1 * il; n[2] = c2 * il;
    return 0.5 * len;
}

// slot[9 f + 3 a + b] = the BSR slot of block (node a, node b) of facet f (-1: not in the pattern; never for a checked facet)
__global__ __launch_bounds__(256) void k_boundary_slots(int32_t nf, const int32_t* __restrict__ facets,
                                                        const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                        int32_t* __restrict__ slot) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= 9 * (int64_t)nf) return;
    const int32_t f = (int32_t)(gid / 9);
    const int ab = (int)(gid % 9);
    const int32_t row = facets[3 * (int64_t)f + ab / 3], col = facets[3 * (int64_t)f + ab % 3];
    int32_t lo = rowptr[row], hi = rowptr[row + 1];
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (colind[mid] < col) lo = mid + 1;
        else hi = mid;
    }
    slot[gid] = (lo < rowptr[row + 1] && colind[lo] == col) ? lo : -1;
}

// partial[2 block] = number of entries that are not (finite and >= 0), partial[2 block + 1] = number of entries that differ
// from the values in force (old == nullptr: none in force, every entry counts)
__global__ __launch_bounds__(256) void k_check_coefficient(int64_t n, const double* __restrict__ x, const double* __restrict__ old,
                                                           double* __restrict__ partial) {
    __shared__ double red[256][2];
    double bad = 0.0, changed = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double xi = x[i];
        if (!(xi >= 0.0) || !isfinite(xi)) bad += 1.0;
        if (!old || old[i] != xi) changed += 1.0;
    }
    red[threadIdx.x][0] = bad;
    red[threadIdx.x][1] = changed;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            red[threadIdx.x][0] += red[threadIdx.x + o][0];
            red[threadIdx.x][1] += red[threadIdx.x + o][1];
        }
        __syncthreads();
    }
    if (threadIdx.x < 2) partial[2 * blockIdx.x + threadIdx.x] = red[0][threadIdx.x];
}

// lane (r, c): component c of boundary row r.  RAW = false: the pass of an assembly -- F[4 i + c] += the row's boundary
// residual and lifting, vals (where given) += the row's entries of the backflow Jacobian, under the Dirichlet rule.  RAW = true
// (sns_residual_moments): no Dirichlet rule, nothing added -- out[4 r + c] = phi[i] * (the row's boundary residual).
template <bool RAW>
__global__ __launch_bounds__(256) void k_boundary_flow(int32_t nb, const int32_t* __restrict__ rows,
                                                       const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ row_fv,
                                                       const int32_t* __restrict__ facets, const int32_t* __restrict__ slot,
                                                       const double* __restrict__ pts, const double* __restrict__ w,
                                                       const double* __restrict__ t, const double* __restrict__ beta,
                                                       const uint8_t* __restrict__ bc_mask, const double* __restrict__ bc_val,
                                                       double* __restrict__ vals, double* __restrict__ F,
                                                       const double* __restrict__ phi, double* __restrict__ out) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = gid >> 2;
    const int c = (int)(gid & 3);
    if (r >= nb) return;                                   // (no cross-lane traffic in this kernel)
    if (c == 3) {                                          // the pressure rows get nothing
        if (RAW) out[4 * r + 3] = 0.0;
        return;
    }
    const int64_t i = rows[r];
    if (!RAW && bc_mask[4 * i + c]) return;                // rows of constrained dofs get nothing
    double R = 0.0;
    const int32_t e1 = row_ptr[r + 1];
    for (int32_t e = row_ptr[r]; e < e1; ++e) {
        const int32_t fv = row_fv[e];
        const int64_t f = fv >> 2;
        const int a = fv & 3;
        const int32_t nd[3] = {facets[3 * f], facets[3 * f + 1], facets[3 * f + 2]};
        double X[3][3], U[3][3], n[3];
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            const double* pp = pts + 3 * (int64_t)nd[m];
            X[m][0] = pp[0]; X[m][1] = pp[1]; X[m][2] = pp[2];
            const double2 u01 = *reinterpret_cast<const double2*>(w + 4 * (int64_t)nd[m]);
            U[m][0] = u01.x; U[m][1] = u01.y; U[m][2] = w[4 * (int64_t)nd[m] + 2];
        }
        const double area = facet_geometry(X, n);
        if (t) {                                           // - |Gamma|/12 sum_b (1 + d_ab) t_b.e_c
            const double* tf = t + 9 * f;
            const double ta = a == 0 ? tf[c] : (a == 1 ? tf[3 + c] : tf[6 + c]);
            R -= area * (1.0 / 12.0) * (((tf[c] + tf[3 + c]) + tf[6 + c]) + ta);
        }
        const double bt = beta ? beta[f] : 0.0;
        if (!(bt > 0.0)) continue;
        double Jr[3][3];                                   // d R / d u_d(b) of this facet: [b][d]
#pragma unroll
        for (int b = 0; b < 3; ++b) Jr[b][0] = Jr[b][1] = Jr[b][2] = 0.0;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const double aq = q < 3 ? BQ_A1 : BQ_A2, wq = q < 3 ? BQ_W1 : BQ_W2;
            double ph[3], u[3];
#pragma unroll
            for (int m = 0; m < 3; ++m) ph[m] = (q % 3 == m) ? 1.0 - 2.0 * aq : aq;
#pragma unroll
            for (int d = 0; d < 3; ++d) u[d] = (ph[0] * U[0][d] + ph[1] * U[1][d]) + ph[2] * U[2][d];
            const double un = (u[0] * n[0] + u[1] * n[1]) + u[2] * n[2];
            if (!(un < 0.0)) continue;                     // the branch of this point: outflow contributes nothing
            const double pa = a == 0 ? ph[0] : (a == 1 ? ph[1] : ph[2]);
            const double uc = c == 0 ? u[0] : (c == 1 ? u[1] : u[2]);
            const double s = -bt * (wq * area) * pa;
            R += s * un * uc;
#pragma unroll
            for (int b = 0; b < 3; ++b)
#pragma unroll
                for (int d = 0; d < 3; ++d) Jr[b][d] += s * ph[b] * ((c == d ? un : 0.0) + n[d] * uc);
        }
        if (RAW) continue;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const int64_t col = nd[b];
            const int64_t sl = slot[9 * f + 3 * a + b];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                if (bc_mask[4 * col + d]) R += Jr[b][d] * (bc_val[4 * col + d] - w[4 * col + d]);      // the lifting
                else if (vals && sl >= 0) vals[16 * sl + 4 * c + d] += Jr[b][d];
            }
        }
    }
    if (RAW) out[4 * r + c] = phi[i] * R;
    else if (F) F[4 * i + c] += R;
}

// the caller's P1 facet data (ncomp values per vertex, in the vertex order of the caller's facets) into the vertex order of the
// rewound facets: vertices 1 and 2 change places where the host swapped them
__global__ __launch_bounds__(256) void k_take_facet_data(int64_t n_items, int ncomp, const uint8_t* __restrict__ swapped,
                                                         const double* __restrict__ src, double* __restrict__ dst) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_items; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = i / (3 * ncomp);
        const int v = (int)((i / ncomp) % 3), c = (int)(i % ncomp);
        const int sv = (swapped[f] && v > 0) ? 3 - v : v;
        dst[i] = src[(3 * f + sv) * ncomp + c];
    }
}

// out4[c] = sum_r x[4 r + c] in a fixed order (one workgroup: lane-strided partial sums, then a tree)
__global__ __launch_bounds__(256) void k_boundary_sum4(int32_t nb, const double* __restrict__ x, double* __restrict__ out4) {
    __shared__ double red[256][4];
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int32_t r = threadIdx.x; r < nb; r += 256)
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] += x[4 * (int64_t)r + c];
#pragma unroll
    for (int c = 0; c < 4; ++c) red[threadIdx.x][c] = v[c];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o)
#pragma unroll
            for (int c = 0; c < 4; ++c) red[threadIdx.x][c] += red[threadIdx.x + o][c];
        __syncthreads();
    }
    if (threadIdx.x < 4) out4[threadIdx.x] = red[0][threadIdx.x];
}

// lane (r, k): species k of boundary row r.  vals[16 s + 5 k] += alpha M_ab, rhs[4 i + k] += int g v - (lifting)
__global__ __launch_bounds__(256) void k_boundary_scalar(int32_t nb, const int32_t* __restrict__ rows,
                                                         const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ row_fv,
                                                         const int32_t* __restrict__ facets, const int32_t* __restrict__ slot,
                                                         const double* __restrict__ pts, const double* __restrict__ alpha,
                                                         const double* __restrict__ g, const uint8_t* __restrict__ cmask,
                                                         const double* __restrict__ cval, double* __restrict__ vals,
                                                         double* __restrict__ rhs) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = gid >> 2;
    const int k = (int)(gid & 3);
    if (r >= nb) return;
    const int64_t i = rows[r];
    if (cmask[4 * i + k]) return;                          // rows of constrained dofs get nothing
    double B = 0.0;
    const int32_t e1 = row_ptr[r + 1];
    for (int32_t e = row_ptr[r]; e < e1; ++e) {
        const int32_t fv = row_fv[e];
        const int64_t f = fv >> 2;
        const int a = fv & 3;
        const int32_t nd[3] = {facets[3 * f], facets[3 * f + 1], facets[3 * f + 2]};
        double X[3][3], n[3];
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            const double* pp = pts + 3 * (int64_t)nd[m];
            X[m][0] = pp[0]; X[m][1] = pp[1]; X[m][2] = pp[2];
        }
        const double m12 = facet_geometry(X, n) * (1.0 / 12.0);
        const double al = alpha ? alpha[4 * f + k] : 0.0;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const double mab = b == a ? 2.0 * m12 : m12;
            if (g) B += mab * g[12 * f + 4 * b + k];
            if (al == 0.0) continue;
            const int64_t col = nd[b];
            const int64_t sl = slot[9 * f + 3 * a + b];
            if (cmask[4 * col + k]) B -= al * mab * cval[4 * col + k];
            else if (sl >= 0) vals[16 * sl + 5 * k] += al * mab;
        }
    }
    rhs[4 * i + k] += B;
}

inline unsigned row_grid(int32_t nb) { return (unsigned)((4 * (int64_t)nb + 255) / 256); }

// every entry of x[0..n) finite and >= 0?  any entry other than in `old`, the values in force (null: none)?  (one reduction
// launch, one host read)
int check_coefficient(sns_ctx* h, const double* x, const double* old, int64_t n, bool* ok, bool* changed) {
    const int gv = std::max(1, vec_grid(n));
    hipLaunchKernelGGL(k_check_coefficient, dim3(gv), dim3(256), 0, h->stream, n, x, old, h->partial);
    reduce_local(h, gv, 2, h->d_scal + 62);
    double r[2] = {1.0, 1.0};
    SNS_TRY(fetch(h, h->d_scal + 62, 2, r));
    *ok = r[0] == 0.0;
    *changed = r[1] != 0.0;
    return SNS_OK;
}

// copy the caller's src into buf (allocated at the first set); src == NULL: the term is off (the buffer stays).  vertex_comp
// = 0: one group of `count / nf` doubles per facet, as given; > 0: P1 facet data with vertex_comp values per vertex, brought
// into the vertex order of the rewound facets
int take_copy(sns_ctx* h, DevBuf<double>& buf, bool& on, const double* src, size_t count, int vertex_comp = 0) {
    if (src) {
        if (!buf || buf.count() != std::max<size_t>(count, 1)) SNS_TRY(buf.alloc(count));
        if (vertex_comp == 0) {
            HIP_TRY(hipMemcpyAsync(buf, src, count * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        } else {
            hipLaunchKernelGGL(k_take_facet_data, dim3(std::max(1, vec_grid((int64_t)count))), dim3(256), 0, h->stream, (int64_t)count,
                               vertex_comp, h->bnd.swapped.get(), src, buf.get());
            HIP_TRY(hipGetLastError());
        }
    }
    on = src != nullptr;
    return SNS_OK;
}

// a boundary coefficient was written or cleared: another operator
void coefficient_changed(sns_ctx* h) {
    ++h->form.boundary_generation;
    pc_stale(h);
}

}  // namespace

int set_boundary_facets(sns_ctx* h, int32_t nf, const int32_t* facets_host, const int64_t* facet_tets_host) {
    BoundaryState& B = h->bnd;
    BoundaryState N;
    if (nf > 0) {                                          // the lists into a state of their own: a refusal leaves the handle untouched
        SNS_TRY(sync_stream(h));
        // (the handle keeps no host copy of the mesh: one download per call of this setter, which is not on any hot path)
        std::vector<int32_t> tets((size_t)4 * h->E);
        std::vector<double> pts((size_t)3 * h->n);
        HIP_TRY(hipMemcpy(tets.data(), h->tets, tets.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(pts.data(), h->pts, pts.size() * sizeof(double), hipMemcpyDeviceToHost));
        HostFacetLists L;
        try {
            build_facet_lists(h->n, h->E, tets.data(), pts.data(), nf, facets_host, facet_tets_host, L);
        } catch (const std::exception& e) {
            set_error(std::string("sns_set_boundary_facets: ") + e.what());
            return SNS_E_MESH;
        }
        N.nf = nf;
        N.nb = (int32_t)L.rows.size();
        SNS_TRY(N.facets.upload(L.facets));
        SNS_TRY(N.rows.upload(L.rows));
        SNS_TRY(N.row_ptr.upload(L.row_ptr));
        SNS_TRY(N.row_fv.upload(L.row_fv));
        std::vector<uint8_t> swapped((size_t)nf);
        for (int32_t k = 0; k < nf; ++k) swapped[(size_t)k] = L.facets[3 * (size_t)k + 1] != facets_host[3 * (size_t)k + 1];
        SNS_TRY(N.swapped.upload(swapped));
        SNS_TRY(N.slot.alloc((size_t)9 * nf));
        const Level& L0 = h->levels[0];
        hipLaunchKernelGGL(k_boundary_slots, dim3((unsigned)((9 * (int64_t)nf + 255) / 256)), dim3(256), 0, h->stream, nf,
                           N.facets.get(), L0.rowptr.get(), L0.colind.get(), N.slot.get());
        HIP_TRY(hipGetLastError());
        SNS_TRY(sync_stream(h));
    }
    if (B.beta_on || B.alpha_on) coefficient_changed(h);   // the data of the old facets goes with them
    B = std::move(N);
    return SNS_OK;
}

int set_boundary_flow(sns_ctx* h, const double* t, const double* beta) {
    BoundaryState& B = h->bnd;
    bool changed = B.beta_on;                              // (clearing a coefficient in force)
    if (beta) {
        bool ok = false;
        SNS_TRY(check_coefficient(h, beta, B.beta_on ? B.beta.get() : nullptr, B.nf, &ok, &changed));
        if (!ok) { set_error("sns_set_boundary_flow: every beta must be finite and >= 0"); return SNS_E_ARG; }
    }
    if (changed) coefficient_changed(h);                   // (the same beta again, with another t: the operator it was)
    SNS_TRY(take_copy(h, B.t, B.t_on, t, (size_t)9 * B.nf, 3));
    SNS_TRY(take_copy(h, B.beta, B.beta_on, beta, (size_t)B.nf));
    return sync_stream(h);                                 // the caller may free its arrays
}

int set_boundary_scalar(sns_ctx* h, const double* alpha, const double* g) {
    BoundaryState& B = h->bnd;
    bool changed = B.alpha_on;
    if (alpha) {
        bool ok = false;
        SNS_TRY(check_coefficient(h, alpha, B.alpha_on ? B.alpha.get() : nullptr, 4 * (int64_t)B.nf, &ok, &changed));
        if (!ok) { set_error("sns_set_boundary_scalar: every alpha must be finite and >= 0"); return SNS_E_ARG; }
    }
    if (changed) coefficient_changed(h);
    SNS_TRY(take_copy(h, B.alpha, B.alpha_on, alpha, (size_t)4 * B.nf));
    SNS_TRY(take_copy(h, B.g, B.g_on, g, (size_t)12 * B.nf, 4));
    return sync_stream(h);
}

int boundary_flow(sns_ctx* h, const double* w, double* F, double* vals) {
    const BoundaryState& B = h->bnd;
    if (!B.flow_on() || (!F && !vals)) return SNS_OK;
    hipLaunchKernelGGL((k_boundary_flow<false>), dim3(row_grid(B.nb)), dim3(256), 0, h->stream, B.nb, B.rows.get(), B.row_ptr.get(),
                       B.row_fv.get(), B.facets.get(), B.slot.get(), h->pts.get(), w, B.t_on ? B.t.get() : nullptr,
                       B.beta_on ? B.beta.get() : nullptr, h->bc_mask.get(), h->bc_val.get(), vals, F, (const double*)nullptr,
                       (double*)nullptr);
    return SNS_OK;
}

int boundary_scalar(sns_ctx* h, const uint8_t* cmask, const double* cval, double* vals, double* rhs) {
    const BoundaryState& B = h->bnd;
    if (!B.scalar_on()) return SNS_OK;
    hipLaunchKernelGGL(k_boundary_scalar, dim3(row_grid(B.nb)), dim3(256), 0, h->stream, B.nb, B.rows.get(), B.row_ptr.get(),
                       B.row_fv.get(), B.facets.get(), B.slot.get(), h->pts.get(), B.alpha_on ? B.alpha.get() : nullptr,
                       B.g_on ? B.g.get() : nullptr, cmask, cval, vals, rhs);
    return SNS_OK;
}

int boundary_moments(sns_ctx* h, const double* w, const double* phi, double out[4]) {
    BoundaryState& B = h->bnd;
    if (!B.flow_on()) return SNS_OK;
    if (!B.rm || B.rm.count() != (size_t)4 * B.nb) SNS_TRY(B.rm.alloc((size_t)4 * B.nb));
    hipLaunchKernelGGL((k_boundary_flow<true>), dim3(row_grid(B.nb)), dim3(256), 0, h->stream, B.nb, B.rows.get(), B.row_ptr.get(),
                       B.row_fv.get(), B.facets.get(), B.slot.get(), h->pts.get(), w, B.t_on ? B.t.get() : nullptr,
                       B.beta_on ? B.beta.get() : nullptr, (const uint8_t*)nullptr, (const double*)nullptr, (double*)nullptr,
                       (double*)nullptr, phi, B.rm.get());
    hipLaunchKernelGGL(k_boundary_sum4, dim3(1), dim3(256), 0, h->stream, B.nb, B.rm.get(), h->d_scal + 108);
    HIP_TRY(hipGetLastError());
    double add[4];
    SNS_TRY(fetch(h, h->d_scal + 108, 4, add));
    for (int c = 0; c < 4; ++c) out[c] += add[c];
    return SNS_OK;
}

}  // namespace sns
