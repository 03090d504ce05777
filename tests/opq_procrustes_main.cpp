// Stand-alone driver of dpq::procrustes (deltapq_amd/csrc/dpq_procrustes.cpp) for the sanitizer run of
// tests/test_opq_host.py: g++ -fsanitize=address,undefined links this file with the solver and runs it as a child
// process.  argv[1]: a file of matrices -- int32 count, then per matrix int32 D, int32 expect_degenerate and D * D
// doubles, row-major.  Built in: D = 1 and the D = 1024 identity.  Exit status 0 and an empty stderr are the verdict.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../deltapq_amd/csrc/dpq_procrustes.h"

static int check(const std::vector<double>& C, int D, int expect_degenerate, const char* what) {
    std::vector<double> R((size_t)D * D, 7.0);
    int deg = -1, sweeps = -1;
    dpq::procrustes(C.data(), D, R.data(), &deg, &sweeps);
    if (deg != expect_degenerate) {
        printf("%s: degenerate = %d, expected %d\n", what, deg, expect_degenerate);
        return 1;
    }
    if (deg) {
        for (double v : R)
            if (v != 7.0) {
                printf("%s: a degenerate solve touched the output\n", what);
                return 1;
            }
        return 0;
    }
    double worst = 0.0;
    for (int a = 0; a < D; ++a)
        for (int b = a; b < D; ++b) {
            double s = 0.0;
            for (int i = 0; i < D; ++i) s += R[(size_t)i * D + a] * R[(size_t)i * D + b];
            const double dev = std::fabs(s - (a == b ? 1.0 : 0.0));
            if (!(dev <= worst)) worst = dev;
        }
    if (!(worst <= 1e-9)) {
        printf("%s: |R^T R - I| = %g\n", what, worst);
        return 1;
    }
    return 0;
}

int main(int argc, char** argv) {
    int bad = 0;
    bad += check(std::vector<double>{-3.0}, 1, 0, "D = 1");
    {
        const int D = 1024;
        std::vector<double> I((size_t)D * D, 0.0);
        for (int i = 0; i < D; ++i) I[(size_t)i * D + i] = 1.0;
        bad += check(I, D, 0, "identity 1024");
    }
    if (argc > 1) {
        FILE* f = fopen(argv[1], "rb");
        if (!f) {
            printf("cannot open %s\n", argv[1]);
            return 2;
        }
        int32_t count = 0;
        if (fread(&count, 4, 1, f) != 1) count = -1;
        for (int32_t c = 0; c < count; ++c) {
            int32_t hdr[2];
            if (fread(hdr, 4, 2, f) != 2 || hdr[0] < 1 || hdr[0] > dpq::kProcrustesMaxD) {
                printf("bad matrix header\n");
                bad += 1;
                break;
            }
            std::vector<double> C((size_t)hdr[0] * hdr[0]);
            if (fread(C.data(), sizeof(double), C.size(), f) != C.size()) {
                printf("short matrix\n");
                bad += 1;
                break;
            }
            char what[32];
            snprintf(what, sizeof what, "matrix %d", (int)c);
            bad += check(C, hdr[0], hdr[1], what);
        }
        if (count < 0) bad += 1;
        fclose(f);
    }
    return bad ? 1 : 0;
}
