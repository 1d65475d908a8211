// The rules of the nonlinear drivers (csrc/sns_policy.h: policy::LineSearch, snes_start, snes_after_step, ksp_converged) on their
// own, for tests/test_host_newton_policy.py.  stdin holds one case per line, stdout one answer per case:
//   ls f initslope n g_1 .. g_n                       -> answer k lambda_1 .. lambda_k   (the scripted trial norms are offered in order,
//                                                        whatever step is asked for; answer -1: the script ran out while the search went on)
//   start f atol max_it                               -> reason
//   step f f0 step_norm x_norm it atol rtol stol max_it -> reason
//   ksp rn tol atol                                   -> reason
#include <cstdio>
#include <cstring>
#include <vector>

#include "sns_policy.h"

int main() {
    using namespace sns::policy;
    char what[16];
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "ls")) {
            double f, initslope;
            int n;
            if (std::scanf("%lf %lf %d", &f, &initslope, &n) != 3 || n < 0) return 2;
            std::vector<double> g((size_t)n);
            for (double& v : g)
                if (std::scanf("%lf", &v) != 1) return 2;
            LineSearch ls(f, initslope);
            std::vector<double> tried;
            int answer = -1;
            for (double gn : g) {
                tried.push_back(ls.lambda());
                answer = ls.offer(gn);
                if (answer != LineSearch::TRY_AGAIN) break;
                answer = -1;
            }
            std::printf("%d %zu", answer, tried.size());
            for (double l : tried) std::printf(" %.17g", l);
            std::printf("\n");
        } else if (!std::strcmp(what, "start")) {
            sns_options o{};
            double f;
            if (std::scanf("%lf %lf %d", &f, &o.snes_atol, &o.snes_max_it) != 3) return 2;
            std::printf("%d\n", snes_start(f, o));
        } else if (!std::strcmp(what, "step")) {
            sns_options o{};
            double f, f0, step_norm, x_norm;
            int it;
            if (std::scanf("%lf %lf %lf %lf %d %lf %lf %lf %d", &f, &f0, &step_norm, &x_norm, &it, &o.snes_atol, &o.snes_rtol, &o.snes_stol,
                           &o.snes_max_it) != 9)
                return 2;
            std::printf("%d\n", snes_after_step(f, f0, step_norm, x_norm, it, o));
        } else if (!std::strcmp(what, "ksp")) {
            double rn, tol, atol;
            if (std::scanf("%lf %lf %lf", &rn, &tol, &atol) != 3) return 2;
            std::printf("%d\n", ksp_converged(rn, tol, atol));
        } else {
            return 2;
        }
    }
    // the constants the header names, and the first step
    return (ls_alpha != 1e-4 || ls_max_it != 40 || LineSearch(1.0, 1.0).lambda() != 1.0) ? 1 : 0;
}
