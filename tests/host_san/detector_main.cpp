// Stand-alone program for the sanitizer build (tests/test_host_detector_san.py): the detector's host read-out of fmpc_host.cpp --
// the Poisson draw in every regime (lam = 0, small, both sides of the switch point, large, 2^31, the NaN domain), the model with
// gain, qe, background and read-out noise, padded rows, in place, and the argument rules.
#include <math.h>
#include <stdio.h>
#include <vector>

#include "../../include/fastmpc.h"
#include "fmpc_detector.h"
#include "fmpc_host.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static fmpc_detector det(double gain, double qe, double bg, double rn, int photon) {
    fmpc_detector d;
    d.gain = gain; d.gain_dev = nullptr; d.qe = qe; d.background = bg; d.read_noise = rn; d.photon_noise = photon;
    d.seed = 0xF00DFACE12345678ull; d.step = (1ull << 32) + 5; d.step_dev = nullptr; d.first = 7;
    return d;
}

int main() {
    const double lams[] = {0.0, 1e-3, 0.5, 3.0, 9.999, 10.0, 10.001, 30.0, 1e3, 1e6, 2147483648.0};
    const int batch = 4, p = 501, ld = 512;
    for (double lam : lams) {
        std::vector<double> Y0((size_t)batch * ld, -7.0), Y((size_t)batch * ld, -7.0);
        for (int r = 0; r < batch; ++r) for (int i = 0; i < p; ++i) Y0[(size_t)r * ld + i] = lam;
        const fmpc_detector d = det(1.0, 1.0, 0.0, 0.0, 1);
        CHECK(fmpc_detector_read_host(Y.data(), Y0.data(), batch, p, ld, &d) == FMPC_OK);
        double mean = 0.0;
        for (int r = 0; r < batch; ++r) {
            for (int i = 0; i < p; ++i) { const double k = Y[(size_t)r * ld + i]; CHECK(k >= 0.0 && k == floor(k)); mean += k; }
            for (int i = p; i < ld; ++i) CHECK(Y[(size_t)r * ld + i] == -7.0);
        }
        mean /= batch * p;
        printf("lam %.6g: mean %.6g\n", lam, mean);
        CHECK(fabs(mean - lam) <= 6.0 * sqrt(lam / (batch * p)));
        // the model, in place
        const fmpc_detector m = det(0.5, 0.9, 3.0, 2.0, 1);
        CHECK(fmpc_detector_read_host(Y0.data(), Y0.data(), batch, p, ld, &m) == FMPC_OK);
        for (int r = 0; r < batch; ++r) {
            for (int i = 0; i < p; ++i) CHECK(isfinite(Y0[(size_t)r * ld + i]));
            for (int i = p; i < ld; ++i) CHECK(Y0[(size_t)r * ld + i] == -7.0);
        }
    }
    // the NaN domain, without a leading dimension
    {
        double bad[4] = {-1.0, NAN, INFINITY, 2147483649.0}, out[4];
        const fmpc_detector d = det(1.0, 1.0, 0.0, 0.0, 1);
        CHECK(fmpc_detector_read_host(out, bad, 2, 2, 0, &d) == FMPC_OK);
        for (double v : out) CHECK(isnan(v));
    }
    // the draw's own functions at the ends of their ranges
    CHECK(fmpc_det_exp(-0.0) == 1.0 && fabs(fmpc_det_exp(-10.0) - exp(-10.0)) <= 1e-13 * exp(-10.0));
    CHECK(fmpc_det_ln(1.0) == 0.0 && fabs(fmpc_det_ln(1.1102230246251565e-16) - log(1.1102230246251565e-16)) <= 1e-12);
    CHECK(fmpc_det_floor(-0.5) == -1.0 && fmpc_det_floor(1e19) == 1e19 && fmpc_det_lnfact(15.0) > fmpc_det_lnfact(14.0));
    // the argument rules
    {
        double y[2] = {1.0, 2.0};
        fmpc_detector d = det(1.0, 1.0, 0.0, 0.0, 1);
        CHECK(fmpc_detector_read_host(nullptr, y, 1, 2, 0, &d) == FMPC_E_NULL && fmpc_detector_read_host(y, y, 1, 2, 0, nullptr) == FMPC_E_NULL);
        CHECK(fmpc_detector_read_host(y, y, 1, 2, 1, &d) == FMPC_E_DIM && fmpc_detector_read_host(y, y, 1, (1 << 24) + 1, 0, &d) == FMPC_E_DIM);
        d.qe = 0.0;
        CHECK(fmpc_host_detector_check(&d, 1) == FMPC_E_DIM);
        d = det(0.0, 1.0, 0.0, 0.0, 1);
        CHECK(fmpc_host_detector_check(&d, 1) == FMPC_E_DIM);
        d.gain_dev = y;
        CHECK(fmpc_host_detector_check(&d, 1) == FMPC_OK && fmpc_detector_read_host(y, y, 1, 2, 0, &d) == FMPC_E_DIM);
        CHECK(y[0] == 1.0 && y[1] == 2.0);
    }
    printf(fails ? "detector host FAILED\n" : "detector host ok\n");
    return fails ? 1 : 0;
}
