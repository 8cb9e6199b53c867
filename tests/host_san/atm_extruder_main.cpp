// Stand-alone program for the sanitizer build (tests/test_host_atm_san.py): the atmosphere's host builder of fmpc_host.cpp at
// W = 18 and 33 -- the extruder by its two defining identities, every prefix of a stencil, the operand images and the argument
// rules -- with ZZ, ZX, XX formed here from fmpc_atm_covariance_host.
#include <math.h>
#include <stdio.h>
#include <vector>

#include "../../include/fastmpc.h"
#include "fmpc_atm.h"
#include "fmpc_host.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static double cov1(double rho, double r0, double L0) {
    double out = 0.0;
    CHECK(fmpc_atm_covariance_host(1, &rho, r0, L0, &out) == FMPC_OK);
    return out;
}

static void identities(int W, int q, const int* st) {
    const double r0 = 0.2, L0 = 42.0, pitch = 1.0 / (W - 2), c0 = cov1(0.0, r0, L0);
    const int N = q * W;
    std::vector<double> A((size_t)W * N), B((size_t)W * W);
    CHECK(fmpc_atm_extruder_host(W, pitch, r0, L0, q, st, A.data(), B.data()) == FMPC_OK);
    auto zz = [&](int r, int c) { return cov1(pitch * hypot((double)(st[r / W] - st[c / W]), (double)(r % W - c % W)), r0, L0); };
    auto zx = [&](int r, int w) { return cov1(pitch * hypot((double)st[r / W], (double)(r % W - w)), r0, L0); };
    double e1 = 0.0, e2 = 0.0;
    for (int w = 0; w < W; ++w) {
        for (int c = 0; c < N; ++c) {
            long double s = 0.0L;
            for (int r = 0; r < N; ++r) s += (long double)A[(size_t)w * N + r] * zz(r, c);
            e1 = fmax(e1, fabs((double)(s - zx(c, w))));
        }
        for (int v = 0; v < W; ++v) {
            long double s = 0.0L;
            for (int k = 0; k < W; ++k) s += (long double)B[(size_t)w * W + k] * B[(size_t)v * W + k];
            for (int r = 0; r < N; ++r) s += (long double)A[(size_t)w * N + r] * zx(r, v);
            e2 = fmax(e2, fabs((double)(s - cov1(pitch * abs(w - v), r0, L0))));
            if (v > w) CHECK(B[(size_t)w * W + v] == 0.0);
        }
        CHECK(B[(size_t)w * W + w] > 0.0);
    }
    printf("W %d q %d: |A ZZ - ZX'| %.3e C0, |B B' + A ZX - XX| %.3e C0\n", W, q, e1 / c0, e2 / c0);
    CHECK(e1 <= 1e-10 * c0 && e2 <= 1e-10 * c0);
}

int main() {
    const int st2[2] = {1, 2}, st3[3] = {1, 2, 17};
    identities(18, 2, st2);
    identities(18, 3, st3);
    identities(33, 3, st3);
    // every prefix, the images, the default stencil
    {
        int def[FMPC_ATM_MAXQ];
        const int W = 33, q = fmpc_host_atm_default_stencil(W, def);
        CHECK(q == 6 && def[5] == 32);
        FmpcAtmExtruders X;
        CHECK(fmpc_host_atm_extruders(W, 1.0 / 31, 0.2, 42.0, q, def, true, X) == FMPC_OK);
        std::vector<double> img;
        unsigned long long off[FMPC_ATM_MAXQ + 1];
        fmpc_host_atm_images(W, q, X, img, off);
        size_t total = 0;
        for (int j = 0; j <= q; ++j) { CHECK(off[j] == total); total += fmpc_atm_img_doubles(W, j); CHECK(X.A[j].size() == (size_t)W * j * W); }
        CHECK(img.size() == total);
        // entry (row 20, k = W + 3) of the image of extruder 2 is A_2(20, W + 3); a padded column is zero
        const int Wp4 = fmpc_atm_wp4(W), KS = 3 * Wp4 / 4, kk = Wp4 + 3, row = 20;
        const size_t at = off[2] + ((size_t)(row / 16) * KS + kk / 4) * 64 + 16 * (kk % 4) + row % 16;
        CHECK(img[at] == X.A[2][(size_t)row * 2 * W + W + 3]);
        const int kp = W;                                   // the first padded column of block 0
        CHECK(img[off[2] + ((size_t)0 * KS + kp / 4) * 64 + 16 * (kp % 4) + 5] == 0.0);
        double b0 = 0.0;
        std::vector<double> B0((size_t)W * W);
        CHECK(fmpc_atm_extruder_host(W, 1.0 / 31, 0.2, 42.0, 0, def, nullptr, B0.data()) == FMPC_OK);
        for (int k = 0; k < W; ++k) b0 += B0[(size_t)5 * W + k] * B0[(size_t)5 * W + k];
        CHECK(fabs(b0 - cov1(0.0, 0.2, 42.0)) <= 1e-10 * b0 && B0 == X.B[0]);
    }
    // the argument rules
    {
        const int bad[2] = {2, 2}, nine[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9};
        CHECK(fmpc_host_atm_check(18, 1.0, 0.2, 42.0, 2, st2) == FMPC_OK);
        CHECK(fmpc_host_atm_check(18, 1.0, 0.2, 42.0, 2, bad) == FMPC_E_DIM);
        CHECK(fmpc_host_atm_check(18, 1.0, 0.2, 42.0, 9, nine) == FMPC_E_UNSUPPORTED);
        CHECK(fmpc_host_atm_check(2049, 1.0, 0.2, 42.0, 2, st2) == FMPC_E_UNSUPPORTED);
        long long n = -1;
        double f = -1.0;
        CHECK(fmpc_atm_displacement_host(4, -0.3, &n, &f) == FMPC_OK && n == 1 && f > 0.19 && f < 0.21);
    }
    printf(fails ? "atm host FAILED\n" : "atm host ok\n");
    return fails ? 1 : 0;
}
