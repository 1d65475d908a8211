// The damping of the levels' smoothers (csrc/sns_policy.h, "smoother damping") on its own, for tests/test_host.py::
// test_damping_predicates and ::test_damping_event_sequences: the three transitions of csrc/sns_damping.hip replayed over the
// header, with synthetic values where the library runs an estimator on the device.  First word of stdin:
//   predicates -- then lines `HAS_ESTIMATE PC_SETUPS NEW_OPERATOR RITZ_OPTION NOT_LAST SWEEPS`; stdout per line: due, takes Ritz, takes growth
//   sequences  -- then one sequence of events per line, on a new handle each:
//     handle N AMG_OMEGA RITZ_OPTION DIRECT_LAST      N levels (first event; DIRECT_LAST: the last of N > 1 levels is solved, not smoothed)
//     setup PC_SETUPS NEW_OPERATOR, then per level SWEEPS LAMBDA RITZ G0 .. G5
//                                                     a set-up at that count of earlier set-ups; per level its sweeps per cycle and
//                                                     what the estimators return if they run: |lambda|max, the Ritz limit, the
//                                                     growth per sweep of trial 0 .. 5
//     retry                                           a retryable failure of a solve (backs off where a retry is offered)
//     amg_omega W | reset_retry | reset_estimates     sns_set_options: the option; its two resets
//   stdout per sequence: after every event but `handle` and `amg_omega`, the levels' dampings as hex floats, events separated by ';'
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "sns_policy.h"

using namespace sns::policy;

struct Synthetic {
    int sweeps = 2;
    double lambda = 0.0, ritz = 0.0, growth[GROWTH_TRIALS] = {};
};

// damping_decide of csrc/sns_damping.hip for a rank with rows on the level, the estimators replaced by their synthetic values
static void decide(LevelDamping& d, const sns_options& o, double backoff, int pc_setups, bool new_operator, bool not_last, bool direct,
                   const Synthetic& s) {
    if (direct) {
        d.omega = capped_damping(o.amg_omega, backoff, 0.0, false, 0.0);
        return;
    }
    const bool due = estimates_due(d.lambda_max > 0.0, pc_setups, new_operator);
    if (due) d.lambda_max = s.lambda;
    const double lam = d.lambda_max;
    const bool ritz = takes_ritz_limit(o, not_last, s.sweeps);
    if (ritz && due) d.ritz_limit = s.ritz;
    d.omega = capped_damping(o.amg_omega, backoff, lam, ritz, d.ritz_limit);
    if (due && lam > 0.0 && takes_growth_check(not_last, s.sweeps)) {
        int trial = 0;
        checked_damping(d.omega, [&](double, double* g) {
            *g = s.growth[trial++];
            return 0;
        });
        d.omega_checked = d.omega;
    } else if (due && lam > 0.0) {
        d.omega_checked = 0.0;
    } else {
        d.omega = held_damping(d.omega, d.omega_checked);
    }
}

static int predicates() {
    int has = 0, setups = 0, newop = 0, ritz = 0, not_last = 0, sweeps = 0;
    sns_options o{};
    while (std::cin >> has >> setups >> newop >> ritz >> not_last >> sweeps) {
        o.amg_ritz_limit = ritz;
        std::printf("%d %d %d\n", (int)estimates_due(has != 0, setups, newop != 0), (int)takes_ritz_limit(o, not_last != 0, sweeps),
                    (int)takes_growth_check(not_last != 0, sweeps));
    }
    return 0;
}

int main() {
    std::string line, ev;
    std::getline(std::cin, line);
    if (line == "predicates") return predicates();
    if (line != "sequences") return 2;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        sns_options o{};
        o.pc_type = SNS_PC_AMG;
        o.amg_retry_damping = 1;
        std::vector<LevelDamping> levels;
        double backoff = 1.0;
        bool direct_last = false, first = true;
        while (in >> ev) {
            if (ev == "handle") {
                int n = 0;
                in >> n >> o.amg_omega >> o.amg_ritz_limit >> direct_last;
                levels.assign((size_t)n, LevelDamping());
                continue;
            } else if (ev == "amg_omega") {
                in >> o.amg_omega;
                continue;
            } else if (ev == "setup") {
                int pc_setups = 0, new_operator = 0;
                in >> pc_setups >> new_operator;
                const int nl = (int)levels.size();
                for (int l = 0; l < nl; ++l) {
                    Synthetic s;
                    in >> s.sweeps >> s.lambda >> s.ritz;
                    for (double& g : s.growth) in >> g;
                    decide(levels[(size_t)l], o, backoff, pc_setups, new_operator != 0, l + 1 < nl, direct_last && l + 1 == nl && nl > 1, s);
                }
            } else if (ev == "retry") {
                if (retry_offered(o, backoff)) {
                    back_off(backoff);
                    for (LevelDamping& d : levels) back_off(d);
                }
            } else if (ev == "reset_retry") {
                if (backoff != 1.0) {
                    backoff = 1.0;
                    for (LevelDamping& d : levels) forget_estimates(d);
                }
            } else if (ev == "reset_estimates") {
                for (LevelDamping& d : levels) forget_estimates(d);
            } else {
                std::cerr << "unknown event " << ev << "\n";
                return 2;
            }
            if (!in) { std::cerr << "short event " << ev << "\n"; return 2; }
            if (!first) std::printf(";");
            first = false;
            for (const LevelDamping& d : levels) std::printf(" %a", d.omega);
        }
        std::printf("\n");
    }
    return 0;
}
