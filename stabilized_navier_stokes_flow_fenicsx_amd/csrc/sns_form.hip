// The setters of the form state h->form (FormState, csrc/sns_ctx.h): the form variant, the time term, the viscosity law and the
// external fields (the reference has none): a nodal P1 body force f and a per-cell viscosity nu_t in buffers the handle owns.
// What a handle's state refuses is asked by the entry points (policy::check_form_request); a setter that alters the operator
// calls pc_stale, and the next assembly stamps the new values into the operator's key (matrix_changed).
//   body force   no assembly code of its own: with u_t = sigma u + d the form takes a = u_t - f wherever it takes u_t, so the
//                handle keeps the caller's d (tt_d), the caller's f (bf_f) and the effective history tt_eff = d - f, and the TT
//                instantiations of the assembly kernels run on tt_eff (k_effective_history, whenever d or f changes; all
//                zero for a viscosity field without a force or a time term, whose EV instantiations read a history too).
//   viscosity    the EV instantiations (csrc/sns_kernels.hip) read tt.nu_t[cell]; here the positivity check (one reduction
//                launch, one host read), the copy, and the field of the compacted cells for sns_residual_moments.
//   mixture      k_mixture_fields: one lane per tet (log-mixing rule at the centroid) and one lane per node (Boussinesq force).
// Host code and small streaming kernels only; nothing here is on the hot path.
#include "sns_ctx.h"

namespace sns {
namespace {

// out = d - f (d == nullptr: -f); every slot, the pressure slots are never read
__global__ __launch_bounds__(256) void k_effective_history(int64_t n, const double* __restrict__ d, const double* __restrict__ f,
                                                           double* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = (d ? d[i] : 0.0) - f[i];
}

// partial[block] = number of entries that are not (finite and > 0)
__global__ __launch_bounds__(256) void k_count_bad_viscosity(int64_t n, const double* __restrict__ nu, double* __restrict__ partial) {
    __shared__ double red[256];
    double v = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double x = nu[i];
        if (!(x > 0.0) || !isfinite(x)) v += 1.0;
    }
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// lane i: tet i (nu_out, where given) and node i (f_out, where given; the pressure slot is written as zero)
__global__ __launch_bounds__(256) void k_mixture_fields(int64_t n_tets, int32_t n_nodes, const int32_t* __restrict__ tets,
                                                        const double* __restrict__ m, double nu0, double log_ratio, double b0,
                                                        double b1, double b2, double* __restrict__ nu_out,
                                                        double* __restrict__ f_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (nu_out && i < n_tets) {
        const int4 tv = *reinterpret_cast<const int4*>(tets + 4 * i);
        const double mc = 0.25 * (((m[tv.x] + m[tv.y]) + m[tv.z]) + m[tv.w]);
        nu_out[i] = nu0 * exp(log_ratio * mc);
    }
    if (f_out && i < n_nodes) {
        const double mi = m[i];
        double2* o = reinterpret_cast<double2*>(f_out + 4 * i);
        o[0] = make_double2(mi * b0, mi * b1);
        o[1] = make_double2(mi * b2, 0.0);
    }
}

// nu_t of the cells k_support_scatter (csrc/sns_kernels.hip) keeps, at the positions it gives them: the same predicate, the
// same order-preserving ballot ranks, the same block offsets
__global__ __launch_bounds__(256) void k_support_scatter_nu(int64_t n_cells, const int32_t* __restrict__ cells, int32_t n_owned,
                                                            const double* __restrict__ phi, const int64_t* __restrict__ off,
                                                            const double* __restrict__ nu, double* __restrict__ nu_c) {
    __shared__ int wsum[4];
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool f = false;
    if (t < n_cells) {
        const int4 tv = *reinterpret_cast<const int4*>(cells + 4 * t);
        const int32_t nd[4] = {tv.x, tv.y, tv.z, tv.w};
#pragma unroll
        for (int a = 0; a < 4; ++a) f |= nd[a] < n_owned && phi[nd[a]] != 0.0;
    }
    const unsigned long long mk = __ballot(f);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) wsum[wv] = __popcll(mk);
    __syncthreads();
    int base = 0;
    for (int k = 0; k < wv; ++k) base += wsum[k];
    if (f) nu_c[off[blockIdx.x] + base + __popcll(mk & ((1ull << lane) - 1ull))] = nu[t];
}

}  // namespace

int set_form_variant(sns_ctx* h, double c_inverse, double lsic_scale, double pspg_sign, int one_point_quadrature) {
    FormVariant fv;
    fv.ci = c_inverse;
    fv.lsic = lsic_scale;
    fv.pspg = pspg_sign;
    if (one_point_quadrature) fv.qa = fv.qb = 0.25;
    h->form.fv = fv;
    h->has_matrix = h->transposed = false;                // (what was assembled is not the handle's form any more)
    pc_stale(h);
    return SNS_OK;
}

// sigma = theta = 0 without a history: back to the steady form
int set_time_term(sns_ctx* h, double sigma, double theta, const double* d) {
    FormState& S = h->form;
    if (sigma != S.tt.sigma || theta != S.tt.theta) pc_stale(h);      // another operator
    if (sigma == 0.0 && theta == 0.0 && !d) {             // (the buffer stays with the handle)
        S.tt.sigma = S.tt.theta = 0.0;
        S.tt_on = false;
        return refresh_history(h);                        // (a body force stays: the history is -f again)
    }
    const size_t ld = (size_t)ld_of(h);
    if (!S.tt_d) SNS_TRY(S.tt_d.alloc(ld));
    if (d) HIP_TRY(hipMemcpyAsync(S.tt_d, d, ld * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    else HIP_TRY(hipMemsetAsync(S.tt_d, 0, ld * sizeof(double), h->stream));
    S.tt.sigma = sigma;
    S.tt.theta = theta;
    S.tt_on = true;
    SNS_TRY(refresh_history(h));                          // tt.d = the handle's d, or d - f under a body force
    return sync_stream(h);                                // the caller may free d
}

int set_viscosity_law(sns_ctx* h, bool carreau, double lambda, double n, double nu_inf_ratio) {
    FormState& S = h->form;
    ViscosityLaw vl;
    if (carreau) { vl.lambda = lambda; vl.n = n; vl.r = nu_inf_ratio; }
    if (carreau != S.vl_on || vl.lambda != S.vl.lambda || vl.n != S.vl.n || vl.r != S.vl.r) pc_stale(h);   // another operator
    S.vl = vl;
    S.vl_on = carreau;
    return SNS_OK;
}

// nu_e and gamma_dot per cell at the state w (either may be null): the field where one is set, the law's value otherwise
int element_viscosity(sns_ctx* h, const double* w, double* nu_dev, double* gamma_dot_dev) {
    const FormState& S = h->form;
    if (h->E > 0 && S.ev_on && nu_dev) {                  // (gamma_dot below as without a field)
        HIP_TRY(hipMemcpyAsync(nu_dev, S.ev_nu, (size_t)h->E * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        nu_dev = nullptr;
    }
    if (h->E > 0 && (nu_dev || gamma_dot_dev)) {
        const unsigned gt = (unsigned)((h->E + 255) / 256);
        const double nu = 1.0 / h->opt.reynolds;
        dispatch<1, 0>(S.vl_on, [&](auto V) {
            hipLaunchKernelGGL((k_element_viscosity<V() != 0>), dim3(gt), dim3(256), 0, h->stream, h->E, h->tets, h->pts, w, nu,
                               S.vl, nu_dev, gamma_dot_dev);
        });
        HIP_TRY(hipGetLastError());
    }
    return sync_stream(h);
}

int refresh_history(sns_ctx* h) {
    FormState& S = h->form;
    const double* d = S.tt_on ? S.tt_d.get() : nullptr;
    const bool zero = S.ev_on && !S.bf_on && !d;        // the EV instantiations contain the time term: they read a history
    if (!S.bf_on && !zero) {
        S.tt.d = d;
        return SNS_OK;
    }
    const int64_t ld = ld_of(h);
    if (!S.tt_eff) SNS_TRY(S.tt_eff.alloc((size_t)ld));
    if (zero) HIP_TRY(hipMemsetAsync(S.tt_eff, 0, (size_t)ld * sizeof(double), h->stream));
    else hipLaunchKernelGGL(k_effective_history, dim3(vec_grid(ld)), dim3(256), 0, h->stream, ld, d, S.bf_f, S.tt_eff);
    HIP_TRY(hipGetLastError());
    S.tt.d = S.tt_eff;
    return SNS_OK;
}

int set_body_force(sns_ctx* h, const double* f) {
    FormState& S = h->form;
    if (!f) {
        S.bf_on = false;
        return refresh_history(h);
    }
    const size_t ld = (size_t)ld_of(h);
    if (!S.bf_f) SNS_TRY(S.bf_f.alloc(ld));
    HIP_TRY(hipMemcpyAsync(S.bf_f, f, ld * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    S.bf_on = true;
    SNS_TRY(refresh_history(h));
    return sync_stream(h);                                // the caller may free f
}

int set_element_viscosity(sns_ctx* h, const double* nu) {
    FormState& S = h->form;
    if (nu) {
        const int gv = std::max(1, vec_grid(h->E));
        hipLaunchKernelGGL(k_count_bad_viscosity, dim3(gv), dim3(256), 0, h->stream, h->E, nu, h->partial);
        reduce_local(h, gv, 1, h->d_scal + 61);
        double nbad = 1.0;
        SNS_TRY(fetch(h, h->d_scal + 61, 1, &nbad));
        if (nbad != 0.0) { set_error("sns_set_element_viscosity: every entry must be finite and > 0"); return SNS_E_ARG; }
        if (!S.ev_nu) SNS_TRY(S.ev_nu.alloc((size_t)h->E));
        HIP_TRY(hipMemcpyAsync(S.ev_nu, nu, (size_t)h->E * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        SNS_TRY(sync_stream(h));                          // the caller may free nu
    }
    if (nu || S.ev_on) {                                  // another operator: the key of the next assembly differs
        ++S.ev_generation;
        pc_stale(h);
    }
    S.ev_on = nu != nullptr;
    S.tt.nu_t = S.ev_on ? S.ev_nu.get() : nullptr;
    return refresh_history(h);
}

int set_mixture(sns_ctx* h, const double* m, double log_ratio, const double buoyancy[3]) {
    const bool want_nu = m && log_ratio != 0.0;
    const bool want_f = m && buoyancy && (buoyancy[0] != 0.0 || buoyancy[1] != 0.0 || buoyancy[2] != 0.0);
    // both fields into temporaries first: a refusal of the viscosity (a non-finite m) leaves the handle untouched
    DevBuf<double> nu;
    double* f = nullptr;
    if (want_nu) SNS_TRY(nu.alloc((size_t)h->E));
    if (want_f) SNS_TRY(get_vec(h, VEC_SCRATCH, &f));
    if (want_nu || want_f) {
        const int64_t lanes = std::max<int64_t>(h->E, h->n);
        hipLaunchKernelGGL(k_mixture_fields, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, h->stream, h->E, h->n, h->tets, m,
                           1.0 / h->opt.reynolds, log_ratio, want_f ? buoyancy[0] : 0.0, want_f ? buoyancy[1] : 0.0,
                           want_f ? buoyancy[2] : 0.0, nu.get(), f);
        HIP_TRY(hipGetLastError());
    }
    SNS_TRY(set_element_viscosity(h, want_nu ? nu.get() : nullptr));
    return set_body_force(h, want_f ? f : nullptr);
}

int support_nu(sns_ctx* h, const double* phi, int64_t nc) {
    if (!h->rm_nu || (int64_t)h->rm_nu.count() < nc) SNS_TRY(h->rm_nu.alloc((size_t)std::max<int64_t>(nc, h->rm_cap)));
    const int64_t nb = (h->E + 255) / 256;
    hipLaunchKernelGGL(k_support_scatter_nu, dim3((unsigned)nb), dim3(256), 0, h->stream, h->E, h->tets, h->n_owned, phi, h->rm_off,
                       h->form.ev_nu, h->rm_nu);
    return SNS_OK;
}

}  // namespace sns
