// Stand-alone program for the sanitizer build (tests/test_host_shwfs_san.py): the Shack-Hartmann sensor's host side of
// fmpc_host.cpp -- fmpc_sh_valid_host over (len, npl) in {64, 128, 96} x {16, 32} with a pupil that leaves lenslets dark, the lit
// map, the factor table at every (pad, s), and the argument rules.
#include <math.h>
#include <stdio.h>
#include <vector>

#include "../../include/fastmpc.h"
#include "fmpc_host.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

int main() {
    const int lens[] = {64, 128, 96}, npls[] = {16, 32};
    for (int len : lens)
        for (int npl : npls) {
            const int nL = len / npl;
            std::vector<double> A((size_t)len * len, 0.0);
            // a disk off centre: column-major, element (row y, column x) at y + len x
            for (int x = 0; x < len; ++x)
                for (int y = 0; y < len; ++y) {
                    const double dx = x + 0.5 - 0.6 * len, dy = y + 0.5 - 0.45 * len;
                    if (dx * dx + dy * dy <= 0.09 * len * len) A[(size_t)x * len + y] = 0.5 + (double)((x * 7 + y * 3) % 11) / 11.0;
                }
            std::vector<unsigned char> valid((size_t)nL * nL, 7), lit;
            int nv = -1;
            CHECK(fmpc_sh_valid_host(len, npl, A.data(), 0.5, valid.data(), &nv) == FMPC_OK);
            int count = 0, nlit = 0;
            for (int j = 0; j < nL; ++j)
                for (int i = 0; i < nL; ++i) {
                    double sum = 0.0;
                    for (int x = 0; x < npl; ++x)
                        for (int y = 0; y < npl; ++y) { const double a = A[(size_t)(j * npl + x) * len + (i * npl + y)]; sum += a * a; }
                    const bool ok = sum / (npl * npl) >= 0.5;
                    CHECK(valid[(size_t)i + (size_t)nL * j] == (ok ? 1 : 0));
                    count += ok ? 1 : 0;
                }
            CHECK(nv == count && count < nL * nL);
            int nv2 = -1;
            CHECK(fmpc_sh_valid_host(len, npl, A.data(), 0.0, nullptr, &nv2) == FMPC_OK && nv2 == nL * nL);
            CHECK(fmpc_sh_valid_host(len, npl, A.data(), 0.5, valid.data(), nullptr) == FMPC_OK);
            fmpc_host_sh_lit(len, npl, A.data(), lit);
            CHECK(lit.size() == (size_t)nL * nL);
            for (size_t l = 0; l < lit.size(); ++l) { nlit += lit[l]; CHECK(lit[l] >= valid[l]); }
            CHECK(nlit >= count && fmpc_host_sh_amplitude_check(len, A.data()) == FMPC_OK);
            // the factor table: unit modulus inside the window, zero beyond it
            for (int pad = 1; pad <= 4; ++pad)
                for (int s = 2; s <= 32 && s <= pad * npl; s += 2) {
                    CHECK(fmpc_host_sh_check(len, npl, pad, s) == FMPC_OK);
                    std::vector<double> F;
                    fmpc_host_sh_factors(npl, pad, s, F);
                    const int nt = s > 16 ? 2 : 1;
                    CHECK(F.size() == (size_t)(npl / 4) * nt * 128);
                    double worst = 0.0;
                    for (int x = 0; x < npl; ++x)
                        for (int a = 0; a < 16 * nt; ++a) {
                            const size_t base = (((size_t)(x / 4) * nt + (a / 16)) * 2) * 64 + (size_t)(x % 4) * 16 + (a % 16);
                            const double m = hypot(F[base], F[base + 64]);
                            if (a < s) { if (fabs(m - 1.0) > worst) worst = fabs(m - 1.0); }
                            else CHECK(m == 0.0);
                            if (x == 0 && a < s) CHECK(F[base] == 1.0 && F[base + 64] == 0.0);
                        }
                    CHECK(worst <= 4e-16);
                }
            printf("len %d npl %d: %d valid of %d, %d lit\n", len, npl, count, nL * nL, nlit);
            // the argument rules
            CHECK(fmpc_sh_valid_host(len, npl, nullptr, 0.5, valid.data(), &nv) == FMPC_E_NULL);
            CHECK(fmpc_sh_valid_host(len, npl, A.data(), 0.5, nullptr, nullptr) == FMPC_E_NULL);
            CHECK(fmpc_sh_valid_host(len, npl, A.data(), NAN, valid.data(), &nv) == FMPC_E_DIM);
            CHECK(fmpc_sh_valid_host(0, npl, A.data(), 0.5, valid.data(), &nv) == FMPC_E_DIM);
            CHECK(fmpc_sh_valid_host(len, 12, A.data(), 0.5, valid.data(), &nv) == FMPC_E_UNSUPPORTED);
            CHECK(fmpc_sh_valid_host(len + 8, npl, A.data(), 0.5, valid.data(), &nv) == FMPC_E_UNSUPPORTED);
            A[5] = -1.0;
            CHECK(fmpc_sh_valid_host(len, npl, A.data(), 0.5, valid.data(), &nv) == FMPC_E_DIM);
            A[5] = INFINITY;
            CHECK(fmpc_sh_valid_host(len, npl, A.data(), 0.5, valid.data(), &nv) == FMPC_E_DIM);
            CHECK(fmpc_host_sh_check(len, npl, 5, 16) == FMPC_E_UNSUPPORTED && fmpc_host_sh_check(len, npl, 2, 7) == FMPC_E_UNSUPPORTED);
            CHECK(fmpc_host_sh_check(len, npl, 1, npl + 2) == FMPC_E_UNSUPPORTED && fmpc_host_sh_check(len, npl, 0, 2) == FMPC_E_DIM);
        }
    printf(fails ? "shwfs host FAILED\n" : "shwfs host ok\n");
    return fails ? 1 : 0;
}
