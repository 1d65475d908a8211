// Which set-ups take the spectral estimates again (csrc/sns_policy.h: policy::OperatorKey, stamp_operator, new_operator) on their
// own, for tests/test_host.py::test_operator_key_sequences.  Every line of stdin is one sequence of events on a new handle:
//   sigma V | theta V | law ON LAMBDA N R | field 1 (set) / 0 (clear) | re V | transpose | assemble FORM | scalar K0 K1 K2 K3 S T | setup
// replayed as the library does -- the setters write the form's share of the key (the field: its generation, as
// set_element_viscosity), an assembly stamps the key (matrix_changed), a transpose flips its flag, a set-up compares and takes
// the key over (pc_setup); the every-fourth-set-up cadence is not part of it (tests/damping_policy_main.cpp).  stdout: per sequence one 0 / 1 for every set-up.
#include <iostream>
#include <sstream>
#include <string>

#include "sns_policy.h"

int main() {
    using namespace sns::policy;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        FormKey form;
        bool field_on = false;
        double re = 1.0;
        OperatorKey matrix_key, est_key;
        std::string ev, out;
        while (in >> ev) {
            if (ev == "sigma") in >> form.sigma;
            else if (ev == "theta") in >> form.theta;
            else if (ev == "law") in >> form.law_on >> form.lambda >> form.n >> form.r;
            else if (ev == "field") {
                int set = 0;
                in >> set;
                if (set || field_on) ++form.nu_generation;
                field_on = set != 0;
            } else if (ev == "re") in >> re;
            else if (ev == "transpose") matrix_key.transposed = !matrix_key.transposed;
            else if (ev == "assemble") {
                int f = 0;
                in >> f;
                stamp_operator(matrix_key, f, re, form);
            } else if (ev == "scalar") {
                double par[6];
                for (double& p : par) in >> p;
                stamp_operator(matrix_key, 4, re, form, par);
            } else if (ev == "setup") {
                out += new_operator(matrix_key, est_key, false) ? '1' : '0';
                est_key = matrix_key;
            } else {
                std::cerr << "unknown event " << ev << "\n";
                return 2;
            }
        }
        std::cout << out << "\n";
    }
    return 0;
}
