// Stand-alone program for the sanitizer build (tests/test_host_dm_spline_san.py): the host side of the mirror of spline actuators in
// fmpc_host.cpp -- fmpc_dm_profile_oomao_host into buffers of exactly cap = 400 pieces at five couplings and on a second curve, its
// refusals, and fmpc_dm_profile_eval_host on profiles of 1, 3, 400 and 4096 pieces with queries on, between and beyond the breaks.
#include <math.h>
#include <stdio.h>
#include <vector>

#include "../../include/fastmpc.h"
#include "fmpc_host.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

int main() {
    const double p3[2] = {0.4, 0.7}, p4[2] = {0.6, 0.4}, q3[2] = {0.5, 0.8}, q4[2] = {0.7, 0.35}, o4[2] = {0.5, 0.4};
    const double mechs[] = {0.1, 0.2, 0.3, 0.4, 0.5};
    for (double mech : mechs) {
        // exactly cap = 400: a write behind either array is a heap overflow
        std::vector<double> breaks(401), coef(1600);
        int pieces = -1;
        CHECK(fmpc_dm_profile_oomao_host(0.2, p3, p4, 1.0, 1.0, mech, 400, breaks.data(), coef.data(), &pieces) == FMPC_OK && pieces == 400);
        for (int i = 0; i < 400; ++i) CHECK(breaks[i] < breaks[i + 1]);
        CHECK(breaks[200] == 0.0 && breaks[0] == -breaks[400]);
        const double R = breaks[400];
        std::vector<double> d, f;
        for (int i = 0; i <= 400; ++i) { d.push_back(breaks[i]); if (i < 400) d.push_back(0.5 * (breaks[i] + breaks[i + 1])); }
        d.push_back(nextafter(R, 9.0)); d.push_back(nextafter(-R, -9.0)); d.push_back(1.0); d.push_back(-1.0); d.push_back(1e300);
        f.assign(d.size(), -7.0);
        CHECK(fmpc_dm_profile_eval_host(400, breaks.data(), coef.data(), (long long)d.size(), d.data(), f.data()) == FMPC_OK);
        const size_t nd = d.size();
        CHECK(fabs(f[400] - 1.0) <= 1e-8);                                 // d = 0
        CHECK(f[nd - 5] == 0.0 && f[nd - 4] == 0.0 && f[nd - 1] == 0.0);
        CHECK(fabs(f[nd - 3] - mech) <= 1e-8 && fabs(f[nd - 2] - mech) <= 1e-8);
        for (int i = 0; i < 400; ++i) CHECK(f[2 * i] == coef[4 * i]);      // on a break: the constant of the piece it opens
        printf("mech %.1f: R %.15g f(1) - mech %.3e\n", mech, R, f[nd - 3] - mech);
    }
    {
        std::vector<double> breaks(601), coef(2400, -7.0);
        int pieces = -1;
        CHECK(fmpc_dm_profile_oomao_host(0.15, q3, q4, 1.4, 1.2, 0.25, 600, breaks.data(), coef.data(), &pieces) == FMPC_OK && pieces == 400);
        CHECK(coef[1600] == -7.0 && coef[2399] == -7.0);
        // the refusals
        CHECK(fmpc_dm_profile_oomao_host(0.2, p3, o4, 0.3, 1.0, 0.1, 600, breaks.data(), coef.data(), &pieces) == FMPC_E_DIM);   // 'overshoot'
        CHECK(fmpc_dm_profile_oomao_host(0.2, p3, p4, 1.0, 1.0, 0.1, 399, breaks.data(), coef.data(), &pieces) == FMPC_E_DIM);
        CHECK(fmpc_dm_profile_oomao_host(0.2, p3, p4, 1.0, 1.0, 0.0, 600, breaks.data(), coef.data(), &pieces) == FMPC_E_DIM);
        CHECK(fmpc_dm_profile_oomao_host(0.2, p3, p4, 1.0, 1.0, 1.0, 600, breaks.data(), coef.data(), &pieces) == FMPC_E_DIM);
        CHECK(fmpc_dm_profile_oomao_host(0.2, p3, p4, 1.0, 1.0, NAN, 600, breaks.data(), coef.data(), &pieces) == FMPC_E_DIM);
        CHECK(fmpc_dm_profile_oomao_host(NAN, p3, p4, 1.0, 1.0, 0.1, 600, breaks.data(), coef.data(), &pieces) == FMPC_E_DIM);
        CHECK(fmpc_dm_profile_oomao_host(0.2, p3, p4, 0.0, 1.0, 0.1, 600, breaks.data(), coef.data(), &pieces) == FMPC_E_DIM);
        CHECK(fmpc_dm_profile_oomao_host(0.2, p3, p4, 1.0, INFINITY, 0.1, 600, breaks.data(), coef.data(), &pieces) == FMPC_E_DIM);
        CHECK(fmpc_dm_profile_oomao_host(0.2, nullptr, p4, 1.0, 1.0, 0.1, 600, breaks.data(), coef.data(), &pieces) == FMPC_E_NULL);
        CHECK(fmpc_dm_profile_oomao_host(0.2, p3, p4, 1.0, 1.0, 0.1, 600, breaks.data(), coef.data(), nullptr) == FMPC_E_NULL);
    }
    // pieces = 1, 3 and 4096, in buffers of exactly that size
    const int sizes[] = {1, 3, 4096};
    for (int pieces : sizes) {
        std::vector<double> breaks((size_t)pieces + 1), coef((size_t)4 * pieces);
        for (int i = 0; i <= pieces; ++i) breaks[i] = -1.5 + 3.75 * (double)i / pieces + (i % 2 ? 0.1 / pieces : 0.0);
        for (int i = 0; i < pieces; ++i) { coef[4 * i] = 1.0 + i; coef[4 * i + 1] = -0.5; coef[4 * i + 2] = 0.25; coef[4 * i + 3] = 0.125 * (i % 3); }
        std::vector<double> d, f;
        for (int i = 0; i <= pieces; ++i) { d.push_back(breaks[i]); d.push_back(nextafter(breaks[i], -9.0)); d.push_back(nextafter(breaks[i], 9.0)); }
        d.push_back(-INFINITY); d.push_back(INFINITY); d.push_back(NAN);
        f.assign(d.size(), -7.0);
        CHECK(fmpc_dm_profile_eval_host(pieces, breaks.data(), coef.data(), (long long)d.size(), d.data(), f.data()) == FMPC_OK);
        for (int i = 0; i < pieces; ++i) {
            CHECK(f[3 * i] == coef[4 * i]);
            CHECK(f[3 * i + 2] != 0.0);
            if (i > 0) CHECK(fabs(f[3 * i + 1] - coef[4 * (i - 1)]) > 0.0);
        }
        CHECK(f[1] == 0.0 && f[3 * pieces + 2] == 0.0 && f[3 * pieces] != 0.0);       // below the first break, above and on the last
        const double t = breaks[pieces] - breaks[pieces - 1];
        const double* c = &coef[4 * (size_t)(pieces - 1)];
        CHECK(fabs(f[3 * pieces] - (c[0] + t * (c[1] + t * (c[2] + t * c[3])))) <= 1e-12 * fabs(c[0]));
        const size_t nd = d.size();
        CHECK(f[nd - 3] == 0.0 && f[nd - 2] == 0.0 && isnan(f[nd - 1]));
        CHECK(fmpc_dm_profile_eval_host(pieces, breaks.data(), coef.data(), 0, d.data(), f.data()) == FMPC_OK);
        printf("pieces %d: %zu queries\n", pieces, nd);
    }
    {
        double b[2] = {0.0, 1.0}, c[4] = {1.0, 0.0, 0.0, 0.0}, d[1] = {0.5}, f[1];
        CHECK(fmpc_dm_profile_eval_host(0, b, c, 1, d, f) == FMPC_E_DIM && fmpc_dm_profile_eval_host(4097, b, c, 1, d, f) == FMPC_E_DIM);
        CHECK(fmpc_dm_profile_eval_host(1, b, c, -1, d, f) == FMPC_E_DIM && fmpc_dm_profile_eval_host(1, nullptr, c, 1, d, f) == FMPC_E_NULL);
        b[1] = 0.0;
        CHECK(fmpc_dm_profile_eval_host(1, b, c, 1, d, f) == FMPC_E_DIM);
        b[1] = 1.0; c[2] = NAN;
        CHECK(fmpc_dm_profile_eval_host(1, b, c, 1, d, f) == FMPC_E_DIM);
    }
    printf(fails ? "dm profile host FAILED\n" : "dm profile host ok\n");
    return fails ? 1 : 0;
}
