// The assembly route (csrc/sns_policy.h: policy::plan_assembly) on its own, for tests/test_host.py::test_assembly_plan_table: stdin
// holds one combination per line (dim form has_w want_matrix has_F fused variant cells violated), stdout the plan of each:
// error route bc_check element store_K Fe_out lift gather_matrix gather_residual bc_residual matrix offdiag diag state.
#include <cstdio>

#include "sns_policy.h"

int main() {
    int dim, form, w, m, F, fused, variant, cells, violated;
    while (std::scanf("%d %d %d %d %d %d %d %d %d", &dim, &form, &w, &m, &F, &fused, &variant, &cells, &violated) == 9) {
        sns::policy::AssemblyFacts f;
        f.dim = dim;
        f.form = form;
        f.has_w = w != 0;
        f.want_matrix = m != 0;
        f.has_F = F != 0;
        f.fused = fused != 0;
        f.variant = variant != 0;
        f.cells = cells != 0;
        sns::policy::AssemblyPlan p = sns::policy::plan_assembly(f);
        if (p.error == SNS_OK && p.bc_check) p = sns::policy::plan_assembly(f, violated != 0);      // as the driver asks
        std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", p.error, (int)p.route, (int)p.bc_check, (int)p.element, (int)p.store_K,
                    (int)p.Fe_out, (int)p.lift, (int)p.gather_matrix, (int)p.gather_residual, (int)p.bc_residual, (int)p.matrix,
                    (int)p.offdiag, (int)p.diag, (int)p.state);
    }
    return 0;
}
