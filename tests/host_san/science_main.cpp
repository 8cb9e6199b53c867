// Stand-alone program for the sanitizer build (tests/test_host_science_san.py): the science camera's host tables of fmpc_host.cpp
// over len in {64, 192}, every window d and an integer and a fractional sampling, with a pupil that has empty row blocks, and the
// argument rules -- an all-zero pupil is an error, not a division by zero.
#include <math.h>
#include <stdio.h>
#include <vector>

#include "../../include/fastmpc.h"
#include "fmpc_host.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

int main() {
    const int lens[] = {64, 192}, ds[] = {16, 32, 48, 64};
    const double ss[] = {1.0, 2.5};
    for (int len : lens) {
        std::vector<double> A((size_t)len * len, 0.0);
        double want = 0.0;
        for (int x = len / 8; x < len - 5; ++x)
            for (int y = 16; y < len - 16; ++y) { const double a = 0.5 + (double)((x * 7 + y * 3) % 11) / 11.0; A[(size_t)x * len + y] = a; want += a; }
        for (int d : ds)
            for (double s : ss) {
                FmpcSciTables t;
                CHECK(fmpc_host_sci_tables(len, d, s, A.data(), 2.0, t) == FMPC_OK);
                CHECK(t.Fimg.size() == (size_t)len * d * 2 && t.qr.size() == (size_t)2 * (len / 16));
                CHECK(fabs(t.sumA - want) <= 1e-12 * want && fabs(t.I0 - 2.0 * want * want) <= 1e-12 * t.I0 && t.sumA2 > 0.0);
                CHECK(t.qr[0] == 0 && t.qr[1] == 0 && t.qr[2] == len / 32 && t.qr[3] == (len - 6) / 4 + 1);
                CHECK(t.qr[2 * (len / 16) - 2] == 0 && t.qr[2 * (len / 16) - 1] == 0);
                double worst = 0.0;
                for (size_t i = 0; i < t.Fimg.size(); i += 128)
                    for (int l = 0; l < 64; ++l) { const double m = fabs(hypot(t.Fimg[i + l], t.Fimg[i + 64 + l]) - 1.0); if (m > worst) worst = m; }
                CHECK(worst <= 4e-16);
                // the flat output of the C entry point, every pointer and none
                std::vector<double> Fr((size_t)len * d), Fi((size_t)len * d);
                std::vector<int> qr((size_t)2 * (len / 16));
                double sums[3];
                CHECK(fmpc_sci_tables_host(len, d, s, A.data(), 2.0, Fr.data(), Fi.data(), qr.data(), sums) == FMPC_OK);
                CHECK(fmpc_sci_tables_host(len, d, s, A.data(), 2.0, nullptr, nullptr, nullptr, nullptr) == FMPC_OK);
                CHECK(Fr[(size_t)(len / 2) * d + 3] == 1.0 && Fi[(size_t)(len / 2) * d + 3] == 0.0 && Fr[(size_t)5 * d + d / 2] == 1.0 && sums[0] == t.sumA);
                printf("len %d d %d s %.1f: sum A %.6g |F| - 1 <= %.2g\n", len, d, s, t.sumA, worst);
            }
        // the argument rules
        FmpcSciTables t;
        std::vector<double> Z((size_t)len * len, 0.0);
        CHECK(fmpc_host_sci_tables(len, 32, 1.0, Z.data(), 1.0, t) == FMPC_E_DIM);            // all zero
        Z[7] = -1.0;
        CHECK(fmpc_host_sci_tables(len, 32, 1.0, Z.data(), 1.0, t) == FMPC_E_DIM);
        Z[7] = NAN;
        CHECK(fmpc_host_sci_tables(len, 32, 1.0, Z.data(), 1.0, t) == FMPC_E_DIM);
        CHECK(fmpc_host_sci_tables(len, 20, 1.0, A.data(), 1.0, t) == FMPC_E_UNSUPPORTED);
        CHECK(fmpc_host_sci_tables(len + 16, 32, 1.0, A.data(), 1.0, t) == FMPC_E_UNSUPPORTED);
        CHECK(fmpc_host_sci_tables(len, 32, 0.99, A.data(), 1.0, t) == FMPC_E_DIM && fmpc_host_sci_tables(len, 32, INFINITY, A.data(), 1.0, t) == FMPC_E_DIM);
        CHECK(fmpc_host_sci_tables(0, 32, 1.0, A.data(), 1.0, t) == FMPC_E_DIM && fmpc_sci_tables_host(len, 32, 1.0, nullptr, 1.0, nullptr, nullptr, nullptr, nullptr) == FMPC_E_NULL);
    }
    printf(fails ? "science host FAILED\n" : "science host ok\n");
    return fails ? 1 : 0;
}
