// The per-cell text of the eigenvalue shape pass (csrc/sns_eigshape_cell.h: eigshape_cell, what k_eigshape_tet runs per lane)
// compiled for the host, for tests/test_host_eigshape.py::test_cell_text_against_the_oracle.  stdin:
//   CORRECTED STRESS_DIV CI LSIC PSPG QA QB CJ CB E
// then per cell 12 vertex coordinates, 16 state values, 16 values of x~, 16 of z~ (masked by the caller) and nu.
// stdout: 12 values per cell (vertex a, direction j), %.17g.  The metric is formed here as tet_metric (csrc/sns_kernels.h)
// forms it.
#include <cmath>
#include <cstdio>

#include "sns_eigshape_cell.h"

static void metric(const double X[4][3], double g[4][3], double G[3][3], double* trG, double* GG, double* det_out) {
    double J[3][3];
    for (int i = 0; i < 3; ++i) {
        J[i][0] = X[1][i] - X[0][i];
        J[i][1] = X[2][i] - X[0][i];
        J[i][2] = X[3][i] - X[0][i];
    }
    const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
    const double c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
    const double c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
    const double id = 1.0 / det;
    double K[3][3];
    K[0][0] = c00 * id; K[1][0] = c01 * id; K[2][0] = c02 * id;
    K[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * id;
    K[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * id;
    K[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * id;
    K[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * id;
    K[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * id;
    K[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * id;
    for (int j = 0; j < 3; ++j) {
        g[1][j] = K[0][j]; g[2][j] = K[1][j]; g[3][j] = K[2][j];
        g[0][j] = -(K[0][j] + K[1][j] + K[2][j]);
    }
    *trG = 0.0;
    *GG = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            G[i][j] = K[0][i] * K[0][j] + K[1][i] * K[1][j] + K[2][i] * K[2][j];
            *GG += G[i][j] * G[i][j];
            if (i == j) *trG += G[i][j];
        }
    *det_out = det;
}

static bool read4x4(double A[4][4]) {
    for (int a = 0; a < 4; ++a)
        for (int c = 0; c < 4; ++c)
            if (std::scanf("%lf", &A[a][c]) != 1) return false;
    return true;
}

int main() {
    int corrected, stress_div;
    long E;
    sns::HessianForm f;
    double cj, cb;
    if (std::scanf("%d %d %lf %lf %lf %lf %lf %lf %lf %ld", &corrected, &stress_div, &f.ci, &f.lsic, &f.pspg, &f.qa, &f.qb, &cj, &cb,
                   &E) != 10)
        return 2;
    for (long e = 0; e < E; ++e) {
        double X[4][3], W[4][4], Xd[4][4], Z[4][4], out[4][3];
        for (int a = 0; a < 4; ++a)
            for (int j = 0; j < 3; ++j)
                if (std::scanf("%lf", &X[a][j]) != 1) return 2;
        if (!read4x4(W) || !read4x4(Xd) || !read4x4(Z) || std::scanf("%lf", &f.nu) != 1) return 2;
        double g[4][3], G[3][3], trG, GG, det;
        metric(X, g, G, &trG, &GG, &det);
        const double wd = std::fabs(det) * (1.0 / 24.0);
        if (corrected)
            sns::eigshape_cell<true>(g, G, trG, GG, wd, W, Xd, Z, f, stress_div != 0, cj, cb, out);
        else
            sns::eigshape_cell<false>(g, G, trG, GG, wd, W, Xd, Z, f, stress_div != 0, cj, cb, out);
        for (int a = 0; a < 4; ++a)
            for (int j = 0; j < 3; ++j) std::printf("%.17g\n", out[a][j]);
    }
    return 0;
}
