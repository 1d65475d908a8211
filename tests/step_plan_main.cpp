// What a linear solve and a set-up may leave out or reorder (csrc/sns_policy.h: policy::plan_step) on its own, for
// tests/test_host_step_plan.py: stdin holds one combination of the facts per line (nranks ksp_type pc_type fine_plain_cycle
// zero_guess_vouched estimates_due plain_step), stdout the plan of each: skip_zero_guess_residual export_ax staged_speculation
// split_cycle setup_two_streams.
#include <cstdio>

#include "sns_policy.h"

int main() {
    int nranks, ksp, pc, plain_cycle, vouched, due, plain_step;
    while (std::scanf("%d %d %d %d %d %d %d", &nranks, &ksp, &pc, &plain_cycle, &vouched, &due, &plain_step) == 7) {
        sns::policy::StepFacts f;
        f.nranks = nranks;
        f.ksp_type = ksp;
        f.pc_type = pc;
        f.fine_plain_cycle = plain_cycle != 0;
        f.zero_guess_vouched = vouched != 0;
        f.estimates_due = due != 0;
        f.plain_step = plain_step != 0;
        const sns::policy::StepPlan p = sns::policy::plan_step(f);
        std::printf("%d %d %d %d %d\n", (int)p.skip_zero_guess_residual, (int)p.export_ax, (int)p.staged_speculation, (int)p.split_cycle,
                    (int)p.setup_two_streams);
    }
    // the default facts: no caller vouches, no cycle that can be cut, estimates due -- nothing is skipped or moved, A x is on offer
    const sns::policy::StepPlan d = sns::policy::plan_step(sns::policy::StepFacts());
    return (d.skip_zero_guess_residual || d.staged_speculation || d.split_cycle || d.setup_two_streams || !d.export_ax) ? 1 : 0;
}
