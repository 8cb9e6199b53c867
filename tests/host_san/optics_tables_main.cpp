// Test driver (CPU only): the host tables of the device optics (fmpc_host.cpp) -- the (n, m) pairs of zernmodfit.m:195-198,
// the factorial quotients of zernfun.m:166-170 for n <= 14, and the pupil ranges per row block that fmpc_est_create and
// fmpc_est_optics_create share.  Prints "modes N count", "coef n |m| c0 c1 ..", "qranges ok"; exits non-zero on a mismatch.
#include <cstdio>
#include <vector>
#include "fmpc_host.h"

int main() {
    const int Ns[] = {0, 1, 6, 14};
    for (int N : Ns) {
        const int cnt = fmpc_host_zernike_modes(N, nullptr, nullptr);
        if (cnt != (N + 1) * (N + 2) / 2) return 2;
        std::vector<int> n(cnt, -99), m(cnt, -99);                  // exactly cnt entries: ASan sees a write past the end
        if (fmpc_host_zernike_modes(N, n.data(), m.data()) != cnt) return 2;
        int j = 0;
        for (int nn = 0; nn <= N; ++nn)
            for (int mm = -nn; mm <= nn; mm += 2, ++j)
                if (n[j] != nn || m[j] != mm) return 3;
        printf("modes %d %d\n", N, cnt);
    }
    if (fmpc_host_zernike_modes(-1, nullptr, nullptr) != 0) return 2;

    std::vector<double> coef(FMPC_ZERNIKE_NCOEF, -1.0);
    unsigned short off[FMPC_ZERNIKE_MAXN + 1][8];
    fmpc_host_zernike_coefficients(coef.data(), off);
    int used = 0;
    for (int n = 0; n <= FMPC_ZERNIKE_MAXN; ++n)
        for (int ma = n & 1; ma <= n; ma += 2) {
            const int terms = (n - ma) / 2 + 1;
            if (off[n][ma / 2] != used) return 4;                   // packed, in (n, |m|) order
            printf("coef %d %d", n, ma);
            for (int s = 0; s < terms; ++s) printf(" %.17g", coef[used + s]);
            printf("\n");
            used += terms;
        }
    if (used != FMPC_ZERNIKE_NCOEF) return 4;

    // pupil ranges: a disk on a 64 x 64 grid, two diversities of which the second is empty; a block outside the disk gives (0, 0)
    const int len = 64, ndiv = 2;
    std::vector<double> Dre((size_t)ndiv * len * len, 0.0), Dim((size_t)ndiv * len * len, 0.0);
    for (int x = 0; x < len; ++x)
        for (int y = 0; y < len; ++y)
            if ((x - 32) * (x - 32) + (y - 40) * (y - 40) <= 15 * 15) Dim[(size_t)x * len + y] = 1.0;       // rows 25..55, columns 17..47
    std::vector<int> qr;
    fmpc_host_estimator_qranges(len, ndiv, Dre.data(), Dim.data(), qr);
    if (qr.size() != (size_t)2 * (len / 16)) return 5;
    for (int b = 0; b < len / 16; ++b) {
        int lo = len, hi = -1;                                       // brute force over the columns
        for (int x = 0; x < len; ++x)
            for (int y = 16 * b; y < 16 * b + 16; ++y)
                if (Dim[(size_t)x * len + y] != 0.0) { if (x < lo) lo = x; if (x > hi) hi = x; }
        const int elo = hi < 0 ? 0 : lo / 4, ehi = hi < 0 ? 0 : hi / 4 + 1;
        if (qr[2 * b] != elo || qr[2 * b + 1] != ehi) return 6;
    }
    if (qr[0] != 0 || qr[1] != 0) return 7;                          // rows 0..15 see no pupil
    printf("qranges ok\n");
    return 0;
}
