// dpq_procrustes.cpp -- orthogonal Procrustes by one-sided (Hestenes) Jacobi in fp64.  Host only: no HIP include,
// compiles with g++ alone (tests/opq_procrustes_main.cpp runs it under the sanitizers).  Every step below is part
// of the stated contract (include/deltapq_amd.h "OPQ / Procrustes"); the library is built with -ffp-contract=off, so
// a multiply and an add are rounded separately and the same input gives the same bytes.
#include "dpq_procrustes.h"

#include <cmath>
#include <cstddef>
#include <vector>

namespace dpq {

namespace {

// sum over rows, ascending, from +0.0, of a[i] * b[i]
double col_dot(const double* a, const double* b, int D) {
    double s = 0.0;
    for (int i = 0; i < D; ++i) s = s + a[i] * b[i];
    return s;
}

}  // namespace

void procrustes(const double* C, int D, double* R_out, int* degenerate, int* sweeps_out) {
    *degenerate = 1;
    if (sweeps_out) *sweeps_out = 0;
    const size_t n = (size_t)D;
    double amax = 0.0;
    for (size_t e = 0; e < n * n; ++e) {
        if (!std::isfinite(C[e])) return;
        const double a = std::fabs(C[e]);
        if (a > amax) amax = a;
    }
    if (amax == 0.0) return;
    // a power of two brings the largest entry into [0.5, 1): exact, and the polar factor does not see a positive scale
    int ex = 0;
    std::frexp(amax, &ex);
    const double scale = std::ldexp(1.0, -ex);

    // columns are contiguous: A[j * D + i] = scale * C[i][j]; V likewise, the identity
    std::vector<double> A(n * n), V(n * n, 0.0), norm(n);
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < n; ++j) A[j * n + i] = C[i * n + j] * scale;
    for (size_t j = 0; j < n; ++j) {
        V[j * n + j] = 1.0;
        norm[j] = col_dot(&A[j * n], &A[j * n], D);
    }

    const double tol2 = (double)D * std::ldexp(1.0, -104);  // skip a pair when gamma^2 <= D * 2^-104 * alpha * beta
    int sweeps = 0;
    for (; sweeps < kProcrustesMaxSweeps; ++sweeps) {
        int rotated = 0;
        for (int p = 0; p + 1 < D; ++p) {
            for (int q = p + 1; q < D; ++q) {
                double* ap = &A[(size_t)p * n];
                double* aq = &A[(size_t)q * n];
                const double alpha = norm[(size_t)p], beta = norm[(size_t)q];
                const double gamma = col_dot(ap, aq, D);
                if (gamma * gamma <= tol2 * alpha * beta) continue;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t);
                const double s = c * t;
                double* vp = &V[(size_t)p * n];
                double* vq = &V[(size_t)q * n];
                for (int i = 0; i < D; ++i) {
                    const double a = ap[i], b = aq[i];
                    ap[i] = c * a - s * b;
                    aq[i] = s * a + c * b;
                    const double va = vp[i], vb = vq[i];
                    vp[i] = c * va - s * vb;
                    vq[i] = s * va + c * vb;
                }
                norm[(size_t)p] = col_dot(ap, ap, D);
                norm[(size_t)q] = col_dot(aq, aq, D);
                ++rotated;
            }
        }
        if (!rotated) break;
    }
    if (sweeps_out) *sweeps_out = sweeps;

    // A = U . S: the singular values are the column norms
    double smax = 0.0, smin = INFINITY;
    for (size_t j = 0; j < n; ++j) {
        norm[j] = std::sqrt(norm[j]);
        if (!std::isfinite(norm[j])) return;
        if (norm[j] > smax) smax = norm[j];
        if (norm[j] < smin) smin = norm[j];
    }
    if (!(smin > (double)D * std::ldexp(1.0, -52) * smax)) return;

    for (size_t j = 0; j < n; ++j)
        for (size_t i = 0; i < n; ++i) A[j * n + i] = A[j * n + i] / norm[j];
    // R[i][k] = sum over j ascending, from +0.0, of U[i][j] * V[k][j]
    for (size_t e = 0; e < n * n; ++e) R_out[e] = 0.0;
    for (size_t j = 0; j < n; ++j)
        for (size_t i = 0; i < n; ++i) {
            const double u = A[j * n + i];
            const double* v = &V[j * n];
            double* r = &R_out[i * n];
            for (size_t k = 0; k < n; ++k) r[k] = r[k] + u * v[k];
        }
    *degenerate = 0;
}

double orthogonality_residual(const float* R, int D) {
    const size_t n = (size_t)D;
    std::vector<double> G(n * n, 0.0);
    for (size_t i = 0; i < n; ++i)
        for (size_t a = 0; a < n; ++a) {
            const double ra = (double)R[i * n + a];
            for (size_t b = a; b < n; ++b) G[a * n + b] = G[a * n + b] + ra * (double)R[i * n + b];
        }
    double worst = 0.0;
    for (size_t a = 0; a < n; ++a)
        for (size_t b = a; b < n; ++b) {
            const double dev = std::fabs(G[a * n + b] - (a == b ? 1.0 : 0.0));
            if (!(dev <= worst)) worst = dev;  // a NaN shows
        }
    return worst;
}

}  // namespace dpq
