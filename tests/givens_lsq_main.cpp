// The least-squares problem of the two FGMRES loops (csrc/sns_policy.h: policy::GivensLsq<T>) on its own, for
// tests/test_host_givens_lsq.py.  stdin holds one case per line, stdout one answer per case:
//   real m cycles  { beta ncols  { h_0 .. h_j wn } for j < ncols } per cycle
//   cplx m cycles  the same, every h_k as (re, im)
// Per cycle and column the answer holds  res cs[j] sn[j]  g[0 .. j + 1]  H[0 .. j + 1][j] (the column after its rotations), and
// behind the last column of a cycle y[0 .. ncols); values of type T as (re, im) for cplx.
#include <complex>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sns_policy.h"

static bool get(double& v) { return std::scanf("%lf", &v) == 1; }
static bool get(std::complex<double>& v) {
    double re, im;
    if (std::scanf("%lf %lf", &re, &im) != 2) return false;
    v = {re, im};
    return true;
}
static void put(double v) { std::printf(" %.17g", v); }
static void put(const std::complex<double>& v) { std::printf(" %.17g %.17g", v.real(), v.imag()); }

template <class T>
static int run_case() {
    int m, cycles;
    if (std::scanf("%d %d", &m, &cycles) != 2 || m < 1 || cycles < 0) return 2;
    sns::policy::GivensLsq<T> lsq(m);
    std::vector<T> h((size_t)m);
    for (int c = 0; c < cycles; ++c) {
        double beta;
        int ncols;
        if (!get(beta) || std::scanf("%d", &ncols) != 1 || ncols < 0 || ncols > m) return 2;
        lsq.restart(beta);
        for (int j = 0; j < ncols; ++j) {
            double wn;
            for (int k = 0; k <= j; ++k)
                if (!get(h[(size_t)k])) return 2;
            if (!get(wn)) return 2;
            put(lsq.push_column(j, h.data(), wn));
            put(lsq.cs[(size_t)j]);
            put(lsq.sn[(size_t)j]);
            for (int k = 0; k <= j + 1; ++k) put(lsq.g[(size_t)k]);
            for (int k = 0; k <= j + 1; ++k) put(lsq.H[(size_t)j * (m + 1) + k]);
        }
        const std::vector<T>& y = lsq.solve(ncols);
        for (int k = 0; k < ncols; ++k) put(y[(size_t)k]);
    }
    std::printf("\n");
    return 0;
}

int main() {
    char what[16];
    while (std::scanf("%15s", what) == 1) {
        int rc = 2;
        if (!std::strcmp(what, "real")) rc = run_case<double>();
        else if (!std::strcmp(what, "cplx")) rc = run_case<std::complex<double>>();
        if (rc) return rc;
    }
    return 0;
}
