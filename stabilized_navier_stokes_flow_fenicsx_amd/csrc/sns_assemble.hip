// Assembly side of the C-ABI layer: the driver of the route policy::plan_assembly (csrc/sns_policy.h) gives a call, and the residual
// moments on the element pass of the same plan; both end with the boundary pass of csrc/sns_boundary.hip where facet terms are
// set.  Host code only: no kernel of its own.  (shared internals in csrc/sns_ctx.h)
#include "sns_ctx.h"

namespace sns {
namespace {

// What a form's passes launch: the kernels (every instantiation has the signature of its template; null where the form has none
// and the plan never asks) and the scalars that go with them.
struct FormPass {
    decltype(&k_fused_offdiag<SNS_FORM_NS, false>) offdiag;
    decltype(&k_fused_diag<SNS_FORM_NS, false>) diag;
    decltype(&k_fused_lift<SNS_FORM_NS, false>) lift;
    decltype(&k_raw_jacobian_apply<SNS_FORM_NS, false>) raw;
    decltype(&k_element<SNS_FORM_NS, false>) element;
    decltype(&k_residual_tet<false>) residual_tet;
    double nu, aux;
    TimeTerm tt;
    ViscosityLaw vl;
};

// THE place where (corrected convection, FormState::ns_variant) becomes the <C, TT, VL, EV> of the 3-D NS assembly kernels: a new compile-time
// variant is added to the kernels' instantiation lists (csrc/sns_kernels.hip) and here, nowhere else.
FormPass form_pass(const sns_ctx* h, int form) {
    const FormState& S = h->form;
    const double nu = 1.0 / h->opt.reynolds;
    if (h->dim == 2 && form == SNS_FORM_NS)
        return {&k_fused_offdiag<SNS_FORM_UGN_2D, false>, &k_fused_diag<SNS_FORM_UGN_2D, false>, &k_fused_lift<SNS_FORM_UGN_2D, false>,
                &k_raw_jacobian_apply<SNS_FORM_UGN_2D, false>, nullptr, nullptr, nu, 0.0, TimeTerm(), ViscosityLaw()};
    if (h->dim == 2)
        return {&k_fused_offdiag<SNS_FORM_STOKES_2D, false>, &k_fused_diag<SNS_FORM_STOKES_2D, false>, nullptr, nullptr, nullptr, nullptr,
                h->opt.stokes_viscosity, h->opt.stokes_beta, TimeTerm(), ViscosityLaw()};
    if (form != SNS_FORM_NS)
        return {&k_fused_offdiag<SNS_FORM_STOKES, false>, &k_fused_diag<SNS_FORM_STOKES, false>, nullptr, nullptr,
                &k_element<SNS_FORM_STOKES, false>, nullptr, nu, 0.0, TimeTerm(), ViscosityLaw()};
    FormPass k{};
    dispatch<1, 0>(h->opt.corrected_convection != 0, [&](auto C) {
        dispatch<3, 2, 1, 0>(S.ns_variant(), [&](auto V) {
            constexpr bool c = C() != 0, ev = V() == 3, tt = V() == 1 || ev, vl = V() == 2;
            k = {&k_fused_offdiag<SNS_FORM_NS, c, tt, vl, ev>, &k_fused_diag<SNS_FORM_NS, c, tt, vl, ev>,
                 &k_fused_lift<SNS_FORM_NS, c, tt, vl, ev>, &k_raw_jacobian_apply<SNS_FORM_NS, c, tt, vl, ev>,
                 &k_element<SNS_FORM_NS, c, tt, vl, ev>, &k_residual_tet<c, tt, vl, ev>, nu, 0.0, S.tt, S.vl};
        });
    });
    return k;
}

// the element pass over `nc` cells of connectivity `cells`: their residuals into Fe (the staged kernel: under the Dirichlet mask
// `mask`, and with store_K their matrices into Ke).  The 2-D Stokes residual kernel serves the moments only.
void launch_element_pass(sns_ctx* h, int form, const FormPass& K, policy::ElementKernel kind, int64_t nc, const int32_t* cells,
                         const double* w, const uint8_t* mask, bool store_K, double* Ke, double* Fe) {
    const unsigned g1 = (unsigned)((nc + 255) / 256), ge = (unsigned)((nc + EL_TETS_PER_BLOCK - 1) / EL_TETS_PER_BLOCK);
    if (kind == policy::ELEMENT_STAGED)
        hipLaunchKernelGGL(K.element, dim3(ge), dim3(256), 0, h->stream, nc, cells, h->pts, w, mask, h->bc_val, K.nu, store_K ? 1 : 0, Ke,
                           Fe, h->form.fv, K.tt, K.vl);
    else if (h->dim == 3)
        hipLaunchKernelGGL(K.residual_tet, dim3(g1), dim3(256), 0, h->stream, nc, cells, h->pts, w, K.nu, Fe, K.tt, K.vl);
    else if (form == SNS_FORM_NS)
        hipLaunchKernelGGL(k_residual_tri, dim3(g1), dim3(256), 0, h->stream, nc, cells, h->pts, w, K.nu, Fe);
    else
        hipLaunchKernelGGL(k_residual_tri_stokes, dim3(g1), dim3(256), 0, h->stream, nc, cells, h->pts, w, K.nu, K.aux, Fe);
}

// does w violate its Dirichlet data?  (one launch, one reduction, one host read)
int bc_violated(sns_ctx* h, const double* w, bool* violated) {
    const int gv = vec_grid(ld_of(h));
    hipLaunchKernelGGL(k_count_bc_violations, dim3(gv), dim3(256), 0, h->stream, ld_of(h), h->bc_mask, h->bc_val, w, h->partial);
    reduce_local(h, gv, 1, h->d_scal + 60);
    double nviol = 1.0;
    SNS_TRY(fetch(h, h->d_scal + 60, 1, &nviol));
    *violated = nviol != 0.0;
    return SNS_OK;
}

// F += A0[:,B] (g - x_B)   (apply_lifting): a third pass over the boundary cells
int lift(sns_ctx* h, const FormPass& K, unsigned gd, const double* w, double* F) {
    double* dl = nullptr;
    SNS_TRY(get_vec(h, VEC_SCRATCH, &dl));
    hipLaunchKernelGGL(k_bc_defect, dim3(vec_grid(ld_of(h))), dim3(256), 0, h->stream, ld_of(h), h->bc_mask, h->bc_val, w, dl);
    hipLaunchKernelGGL(K.lift, dim3(gd), dim3(256), 0, h->stream, h->n_owned, h->levels[0].diag, h->c_ptr, h->c_idx, h->tets, h->pts, w,
                       h->bc_mask, dl, K.nu, F, K.tt, K.vl);
    return SNS_OK;
}

policy::AssemblyFacts facts_of(const sns_ctx* h, int form, bool has_w, bool want_matrix, bool has_F) {
    return {h->dim, form, has_w, want_matrix, has_F, h->opt.assembly_fused != 0, !h->form.fv.is_default(), h->E > 0};
}

}  // namespace

void matrix_changed(sns_ctx* h, int form, const double* scalar_par) {
    h->has_matrix = true;
    h->transposed = h->pc_ready = false;
    h->matrix_form = form;
    policy::stamp_operator(h->matrix_key, form, h->opt.reynolds, h->form.key(), scalar_par);
}

// The owner-lane passes are scratch-free: every BSR block (and every node residual) is computed by the lanes that own it.  The
// staged route goes through the element scratch Ke / Fe and the gathers.  w == NULL with the Stokes form: the system of
// LinearProblem(a, L, bcs) resp. solve_stokes_problem (:197-218), F(0) = the lifting A0[:,B] g at the data extended by zero.
int assemble(sns_ctx* h, int form, const double* w, double* F, bool want_matrix) {
    const policy::AssemblyFacts f = facts_of(h, form, w != nullptr, want_matrix, F != nullptr);
    policy::AssemblyPlan p = policy::plan_assembly(f);
    if (p.error != SNS_OK) { set_error(p.message); return p.error; }
    bool violated = true;
    if (p.bc_check) { SNS_TRY(bc_violated(h, w, &violated)); p = policy::plan_assembly(f, violated); }
    Level& L = h->levels[0];
    const FormPass K = form_pass(h, form);
    const int64_t ndof = ld_of(h);
    const unsigned go = (unsigned)((h->n_od + 255) / 256), gd = (unsigned)((4 * (int64_t)h->n_owned + 255) / 256);
    const double* state = p.state == policy::STATE_GEXT ? h->gext.get() : w;
    if (p.state == policy::STATE_SNAPPED) {
        double* tmp = nullptr;
        SNS_TRY(get_vec(h, VEC_SCRATCH, &tmp));
        HIP_TRY(hipMemcpyAsync(tmp, w, ndof * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        hipLaunchKernelGGL(k_snap_bc, dim3(vec_grid(ndof)), dim3(256), 0, h->stream, ndof, h->bc_mask, h->bc_val, 1e300, tmp);
        state = tmp;
    }
    if (p.offdiag)
        hipLaunchKernelGGL(K.offdiag, dim3(go), dim3(256), 0, h->stream, h->n_od, h->od_order, h->c_ptr, h->c_idx, h->levels[0].slot_row,
                           L.colind, h->tets, h->pts, state, h->bc_mask, K.nu, K.aux, L.vals, K.tt, K.vl);
    if (p.diag)
        hipLaunchKernelGGL(K.diag, dim3(gd), dim3(256), 0, h->stream, h->n_owned, L.diag, h->c_ptr, h->c_idx, h->tets, h->pts, state,
                           h->bc_mask, h->bc_val, K.nu, K.aux, want_matrix ? L.vals.get() : nullptr, F, K.tt, K.vl);
    const bool staged = p.route == policy::ROUTE_STAGED;
    if (staged && want_matrix && !h->Ke) SNS_TRY(h->Ke.alloc((size_t)h->E * 256));
    if ((staged || p.element != policy::ELEMENT_NONE) && !h->Fe) SNS_TRY(h->Fe.alloc((size_t)h->E * 16));
    if (p.element != policy::ELEMENT_NONE)
        launch_element_pass(h, form, K, p.element, h->E, h->tets, w, h->bc_mask, p.store_K, h->Ke, p.Fe_out ? h->Fe.get() : nullptr);
    if (p.gather_matrix)
        hipLaunchKernelGGL(k_gather_matrix, dim3((unsigned)((L.nnzb * 8 + 255) / 256)), dim3(256), 0, h->stream, L.nnzb, h->c_ptr,
                           h->c_idx, h->levels[0].slot_row, L.colind, h->bc_mask, h->Ke, L.vals);
    if (p.gather_residual)
        hipLaunchKernelGGL(k_gather_residual, dim3(gd), dim3(256), 0, h->stream, h->n_owned, h->nt_ptr, h->nt_idx, h->bc_mask,
                           h->bc_val, w, h->Fe, F);
    if (p.lift) SNS_TRY(lift(h, K, gd, w, F));
    if (p.bc_residual)
        hipLaunchKernelGGL(k_bc_residual, dim3(vec_grid(ndof)), dim3(256), 0, h->stream, ndof, h->bc_mask, h->bc_val, w, F);
    // the facet terms of the 3-D NS form, on either route: after the volume passes have written vals and F (nothing set:
    // nothing launched)
    if (form == SNS_FORM_NS && h->dim == 3) SNS_TRY(boundary_flow(h, w, F, want_matrix ? L.vals.get() : nullptr));
    if (p.matrix) {
        // after a scalar-transport assembly (csrc/sns_scalar.hip) the hierarchy's transfers leave out the flow's Dirichlet dofs again
        if (h->matrix_form == SNS_FORM_SCALAR) SNS_TRY(fine_free_mask(h, h->bc_mask));
        matrix_changed(h, form);
    }
    HIP_TRY(hipGetLastError());
    return SNS_OK;
}

// y = J0(w) x or J0(w)^T x by the NS form's raw-Jacobian pass (handle, pointers and the form state were checked by the entry
// point).  Reads the mesh, the form state and the node -> cell lists; writes y and nothing of the handle.
int raw_jacobian_apply(sns_ctx* h, const double* w, const double* x, bool transposed, double* y) {
    if (h->n == 0) return SNS_OK;
    const FormPass K = form_pass(h, SNS_FORM_NS);
    const unsigned g = (unsigned)((4 * (int64_t)h->n + 255) / 256);
    hipLaunchKernelGGL(K.raw, dim3(g), dim3(256), 0, h->stream, h->n, h->nt_ptr, h->nt_idx, h->tets, h->pts, w, x, K.nu,
                       transposed ? 1 : 0, y, K.tt, K.vl);
    HIP_TRY(hipGetLastError());
    return sync_stream(h);
}

int timed_assemble(sns_ctx* h, int form, const double* w, double* F, bool want_matrix) {
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    SNS_TRY(assemble(h, form, w, F, want_matrix));
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    h->tm.assemble_ms += ms;
    return SNS_OK;
}

// form, pointers and the mesh were checked by the entry point
int residual_moments(sns_ctx* h, int form, const double* w, const double* phi, double out[4]) {
    const int64_t ndof = ld_of(h);
    if (!w) {                                        // linear form without a state: R_raw(0) = 0, still one collective pass
        double* z = nullptr;
        SNS_TRY(get_vec(h, VEC_SCRATCH, &z));
        HIP_TRY(hipMemsetAsync(z, 0, ndof * sizeof(double), h->stream));
        w = z;
    }
    // support of the functional behind the owned rows: count, scan, fetch the size, scatter
    const int64_t nb = (h->E + 255) / 256;
    if (!h->rm_off) SNS_TRY(h->rm_off.alloc((size_t)nb));
    hipLaunchKernelGGL(k_support_count, dim3((unsigned)nb), dim3(256), 0, h->stream, h->E, h->tets, h->n_owned, phi, h->rm_off);
    hipLaunchKernelGGL(k_support_scan, dim3(1), dim3(256), 0, h->stream, nb, h->rm_off, h->d_scal + 100);
    double total = 0.0;
    SNS_TRY(fetch(h, h->d_scal + 100, 1, &total));
    const int64_t nc = (int64_t)total;
    if (nc > h->rm_cap) {
        h->rm_cap = 0;
        SNS_TRY(h->rm_cells.alloc((size_t)4 * nc));
        SNS_TRY(h->rm_Fe.alloc((size_t)16 * nc));
        h->rm_nu.reset();
        h->rm_cap = nc;
    }
    if (nc > 0) {
        hipLaunchKernelGGL(k_support_scatter, dim3((unsigned)nb), dim3(256), 0, h->stream, h->E, h->tets, h->n_owned, phi,
                           h->rm_off, h->rm_cells);
        // element residuals of the compacted cells by the element pass the plan gives a residual of the same form at a state
        // that satisfies its data (2-D: always one lane per cell); no lifting: the one-lane-per-cell kernels have none, the
        // staged kernel gets an all-zero Dirichlet mask
        const policy::ElementKernel kind =
            h->dim == 2 ? policy::ELEMENT_RESIDUAL : policy::plan_assembly(facts_of(h, form, true, false, true), false).element;
        if (kind == policy::ELEMENT_STAGED && !h->rm_nomask) {
            SNS_TRY(h->rm_nomask.alloc((size_t)ndof));
            HIP_TRY(hipMemset(h->rm_nomask, 0, (size_t)ndof));
        }
        FormPass K = form_pass(h, form);
        if (form == SNS_FORM_NS && h->form.ev_on) {           // the element kernels index the field by the cell of their pass
            SNS_TRY(support_nu(h, phi, nc));
            K.tt.nu_t = h->rm_nu;
        }
        launch_element_pass(h, form, K, kind, nc, h->rm_cells, w, h->rm_nomask, false, nullptr, h->rm_Fe);
    }
    // fixed-order two-stage reduction (grid fixed by the support size), then the handle's all-reduce over the ranks
    const int gm = (int)std::max<int64_t>(1, std::min<int64_t>((nc + 255) / 256, 2048));
    hipLaunchKernelGGL(k_moments_partial, dim3(gm), dim3(256), 0, h->stream, nc, h->rm_cells, h->dim + 1, h->n_owned, phi,
                       h->rm_Fe, h->partial);
    SNS_TRY(reduce_to(h, gm, 4, h->d_scal + 104));
    HIP_TRY(hipGetLastError());
    SNS_TRY(fetch(h, h->d_scal + 104, 4, out));
    if (h->dim == 2) out[2] = 0.0;
    // ... plus phi . (the boundary residual without the Dirichlet rule): R_raw stays the raw residual of the whole form
    if (form == SNS_FORM_NS && h->dim == 3) SNS_TRY(boundary_moments(h, w, phi, out));
    return SNS_OK;
}

}  // namespace sns
