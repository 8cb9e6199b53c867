// The host arithmetic that the API files hand to fmpc_host.cpp, under AddressSanitizer + UndefinedBehaviorSanitizer:
//   fmpc_host_bank_first_constants   L L' = B diag(a^2) B', L y0 = B (a^2 o cu) and the three scalars against a long double
//                                    restatement from the inputs, to 32 n 2^-53 of the largest entry; a singular B diag(a^2) B' refused
//   fmpc_host_inverse_images         every entry of every image against the entry of J, A1, A2 its layout names, with ==, from an
//                                    integer-valued J laid out as the panel kernel leaves it (the division by the scale is exact)
//   fmpc_host_bank_desc              the packed ints unpack to the table they came from
//   fmpc_host_spd_inverse            A inv = I to 64 n 2^-53 cond on a matrix whose condition number is set by construction
// usage: api_host_math_test        (no arguments; seeded)
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include <vector>

#include "../../mpc-sensorlessao_amd/csrc/fmpc_bank.h"
#include "../../mpc-sensorlessao_amd/csrc/fmpc_host.h"

typedef long double ld;
static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)
static const double EPS = 1.1102230246251565e-16;      // 2^-53

// ---- fmpc_host_bank_first_constants
static void constants_case(int n, int m, int T, int seed) {
    const int NX = 32;
    const double k = 1e-2;
    std::mt19937_64 rng(seed);
    std::normal_distribution<double> N01(0.0, 1.0);
    std::uniform_real_distribution<double> U01(0.0, 1.0);
    std::vector<double> bt((size_t)m * n), umax(m), umin(m), umid(m), R2(m), rl(m);
    for (double& v : bt) v = N01(rng);
    for (int j = 0; j < m; ++j) {
        umin[j] = -(1.0 + U01(rng)); umax[j] = 1.0 + U01(rng); umid[j] = (umin[j] + umax[j]) / 2;
        R2[j] = 2.0 * (0.5 + U01(rng)); rl[j] = N01(rng);
    }
    std::vector<double> cst;
    const bool ok = fmpc_host_bank_first_constants(n, m, T, k, bt.data(), umax.data(), umin.data(), umid.data(), R2.data(), rl.data(), cst);
    if (m < n && !ok) {       // rank m < n: B diag(a^2) B' is singular, there is no factor to check
        printf("constants n %d m %d T %d: singular (rank %d), refused\n", n, m, T, m);
        return;
    }
    CHECK(ok, "constants n %d m %d T %d: refused", n, m, T);
    if (!ok) return;
    CHECK(cst.size() == (size_t)NX * NX + NX + 8, "constants: %zu doubles", cst.size());
    // the restatement: everything in long double from the inputs
    std::vector<ld> a2(m), cu(m);
    ld acu2 = 0.0L;
    for (int j = 0; j < m; ++j) {
        const ld dp = 1.0L / ((ld)umax[j] - (ld)umid[j]), dm = 1.0L / ((ld)umid[j] - (ld)umin[j]);
        const ld hc = (ld)k * (dp * dp + dm * dm), a = hc / ((ld)R2[j] + hc);
        cu[j] = (ld)R2[j] * (ld)umid[j] + (ld)rl[j] + (ld)k * (dp - dm);
        a2[j] = a * a;
        acu2 += a2[j] * cu[j] * cu[j];
    }
    std::vector<ld> Ma((size_t)n * n, 0.0L), v(n, 0.0L);
    ld maxM = 0.0L, maxv = 0.0L, trace = 0.0L;
    for (int r = 0; r < n; ++r) {
        for (int q = 0; q < n; ++q) {
            for (int j = 0; j < m; ++j) Ma[(size_t)r * n + q] += (ld)bt[(size_t)j * n + r] * a2[j] * (ld)bt[(size_t)j * n + q];
            maxM = fmaxl(maxM, fabsl(Ma[(size_t)r * n + q]));
        }
        for (int j = 0; j < m; ++j) v[r] += (ld)bt[(size_t)j * n + r] * a2[j] * cu[j];
        maxv = fmaxl(maxv, fabsl(v[r]));
        trace += Ma[(size_t)r * n + r];
    }
    const ld tol = 32.0L * n * EPS;
    auto Lel = [&](int i, int q) -> ld { return q <= i ? (ld)cst[(size_t)q * NX + i] : 0.0L; };
    ld worstM = 0.0L, worstv = 0.0L, y2 = 0.0L;
    for (int r = 0; r < n; ++r) {
        for (int q = 0; q < n; ++q) {
            ld t = 0.0L;
            for (int c = 0; c < n; ++c) t += Lel(r, c) * Lel(q, c);
            worstM = fmaxl(worstM, fabsl(t - Ma[(size_t)r * n + q]));
        }
        ld t = 0.0L;
        for (int c = 0; c < n; ++c) t += Lel(r, c) * (ld)cst[(size_t)NX * NX + c];
        worstv = fmaxl(worstv, fabsl(t - v[r]));
        y2 += (ld)cst[(size_t)NX * NX + r] * (ld)cst[(size_t)NX * NX + r];
    }
    CHECK(worstM <= tol * maxM, "constants n %d m %d T %d: L L' off by %.3Le of %.3Le", n, m, T, worstM, maxM);
    CHECK(worstv <= tol * maxv, "constants n %d m %d T %d: L y0 off by %.3Le of %.3Le", n, m, T, worstv, maxv);
    // what lies outside the triangle, the vector and the three scalars is zero
    for (int q = 0; q < NX; ++q)
        for (int i = 0; i < NX; ++i)
            if (i >= n || q > i) CHECK(cst[(size_t)q * NX + i] == 0.0, "constants: entry (%d, %d) outside the factor is %g", q, i, cst[(size_t)q * NX + i]);
    for (int i = n; i < NX; ++i) CHECK(cst[(size_t)NX * NX + i] == 0.0, "constants: y0[%d] = %g", i, cst[(size_t)NX * NX + i]);
    for (int i = 3; i < 8; ++i) CHECK(cst[(size_t)NX * NX + NX + i] == 0.0, "constants: scalar %d = %g", i, cst[(size_t)NX * NX + NX + i]);
    // the scalars: T (sum a^2 cu^2 - |y0|^2) clamped at 0, |L|_F^2 = trace(B diag(a^2) B') and T |y0|^2, the last two times 1 + 1e-12
    const ld c0 = (ld)T * (acu2 - y2), s0 = cst[(size_t)NX * NX + NX], s1 = cst[(size_t)NX * NX + NX + 1], s2 = cst[(size_t)NX * NX + NX + 2];
    CHECK(s0 >= 0.0L && fabsl(s0 - (c0 > 0.0L ? c0 : 0.0L)) <= tol * (ld)T * acu2, "constants: c0 %.17Lg, formula %.17Lg", s0, c0);
    CHECK(fabsl(s1 - trace * (1.0L + 1e-12L)) <= tol * trace, "constants: |L|^2 %.17Lg, formula %.17Lg", s1, trace * (1.0L + 1e-12L));
    CHECK(fabsl(s2 - (ld)T * y2 * (1.0L + 1e-12L)) <= tol * (ld)T * y2, "constants: T |y0|^2 %.17Lg, formula %.17Lg", s2, (ld)T * y2 * (1.0L + 1e-12L));
    printf("constants n %d m %d T %d: L L' %.2Le, L y0 %.2Le of the largest entry (bound %.2Le)\n", n, m, T, worstM / maxM, worstv / maxv, tol);
    // a row of B that is exactly zero: the pivot test refuses
    const int zr = n / 2;
    for (int j = 0; j < m; ++j) bt[(size_t)j * n + zr] = 0.0;
    CHECK(!fmpc_host_bank_first_constants(n, m, T, k, bt.data(), umax.data(), umin.data(), umid.data(), R2.data(), rl.data(), cst),
          "constants n %d m %d T %d: a zero row of B was not refused", n, m, T);
}

// ---- fmpc_host_inverse_images
static void images_case(int n, int T, int has_xf, bool var2, int seed) {
    const int nb = T + has_xf, TN = T * n, nrow = nb * n, ncol = 2 * n + TN, np = 1 + ncol + 2 * n, npanels = (np + FP_NP - 1) / FP_NP;
    const int jks = FP_XKS + (TN + 3) / 4, jks2 = 2 * FP_XKS, jksp = 16 * ((jks + 15) / 16 + 3), jksp2 = 16 * ((jks2 + 15) / 16 + 3);
    const int nrt = (nrow + 15) / 16, nc = 4 * n;
    std::mt19937_64 rng(seed);
    std::uniform_int_distribution<int> I1000(-1000, 1000);
    // J (columns [x0 | x0_pre | w]), J2 (columns [B u1 | B u2]), nuc, A1, A2: integers
    std::vector<double> J((size_t)nrow * ncol), J2((size_t)nrow * 2 * n), nc0(nrow), a1((size_t)n * n), a2((size_t)n * n);
    for (double& v : J) v = I1000(rng);
    for (double& v : J2) v = I1000(rng);
    for (double& v : nc0) v = I1000(rng);
    for (double& v : a1) v = I1000(rng);
    for (double& v : a2) v = I1000(rng);
    // as the panel kernel leaves nu: problem 0 is d = 0, problem 1 + c the unit vector c times the scale, then the 2 n columns of J2
    std::vector<double> nu((size_t)npanels * nrow * FP_NP, 0.0);
    auto slot = [&](int p, int r) -> double& { return nu[((size_t)(p / FP_NP) * nrow + r) * FP_NP + (p % FP_NP)]; };
    for (int r = 0; r < nrow; ++r) {
        slot(0, r) = nc0[r];
        for (int c = 0; c < ncol; ++c) slot(1 + c, r) = nc0[r] + FMPC_INV_SCALE * J[(size_t)r * ncol + c];
        for (int c = 0; c < 2 * n; ++c) slot(1 + ncol + c, r) = nc0[r] + FMPC_INV_SCALE * J2[(size_t)r * 2 * n + c];
    }
    std::vector<double> img, nuc, jst, ncs, img2, eimg, J4, nuc4;
    const bool ok = fmpc_host_inverse_images(n, T, nb, var2, jks, jks2, a1.data(), a2.data(), nu, img, nuc, jst, ncs, img2, eimg, J4, nuc4);
    CHECK(ok, "images T %d xf %d var2 %d: refused", T, has_xf, (int)var2);
    if (!ok) return;
    // the expected images, scattered entry by entry from J, J2, A1, A2 to where the layout comments put them; everything else zero
    auto lane = [](int row, int kk) { return 16 * (kk & 3) + (row & 15); };
    auto Jx = [&](int r, int c) { return (c < n || var2) ? J[(size_t)r * ncol + c] : 0.0; };     // c < 2 n; VAR(1): x0_pre does not enter
    std::vector<double> eimg_((size_t)4 * FP_XKS * 64, 0.0), img_((size_t)nrt * jksp * 64, 0.0), img2_((size_t)nrt * jksp2 * 64, 0.0);
    std::vector<double> jst_((size_t)nb * 2 * FP_XKS * 64, 0.0), ncs_((size_t)nb * 32, 0.0), nuc_((size_t)nrt * 16, 0.0), J4_((size_t)nrow * nc, 0.0);
    for (int r = 0; r < nrow; ++r) {
        nuc_[r] = nc0[r];
        ncs_[(size_t)(r / n) * 32 + r % n] = nc0[r];
        for (int c = 0; c < 2 * n; ++c) {                    // [x0 ; x0_pre]: k-steps 0 .. FP_XKS - 1
            img_[((size_t)(r >> 4) * jksp + c / 4) * 64 + lane(r, c)] = Jx(r, c);
            img2_[((size_t)(r >> 4) * jksp2 + c / 4) * 64 + lane(r, c)] = Jx(r, c);
            const int st = r / n, rl = r % n;
            jst_[(((size_t)st * 2 + rl / 16) * FP_XKS + c / 4) * 64 + lane(rl, c)] = Jx(r, c);
            J4_[(size_t)r * nc + c] = Jx(r, c);
        }
        for (int e = 0; e < TN; ++e) {                       // w: from k-step FP_XKS on
            const int kk = 4 * FP_XKS + e;
            img_[((size_t)(r >> 4) * jksp + kk / 4) * 64 + lane(r, kk)] = J[(size_t)r * ncol + 2 * n + e];
        }
        for (int c = 0; c < 2 * n; ++c) {                    // [B u1 ; B u2]: from k-step FP_XKS on
            const int kk = 4 * FP_XKS + c;
            img2_[((size_t)(r >> 4) * jksp2 + kk / 4) * 64 + lane(r, kk)] = J2[(size_t)r * 2 * n + c];
            J4_[(size_t)r * nc + 2 * n + c] = J2[(size_t)r * 2 * n + c];
        }
    }
    for (int row = 0; row < 2 * n; ++row)                    // E = [A1 A2 ; A2 0]
        for (int kk = 0; kk < 2 * n; ++kk) {
            double v = 0.0;
            if (row < n && kk < n) v = a1[(size_t)row * n + kk];
            else if (row < n) v = var2 ? a2[(size_t)row * n + kk - n] : 0.0;
            else if (kk < n) v = var2 ? a2[(size_t)(row - n) * n + kk] : 0.0;
            eimg_[((size_t)(row >> 4) * FP_XKS + kk / 4) * 64 + lane(row, kk)] = v;
        }
    struct { const char* name; const std::vector<double>* got; const std::vector<double>* want; } cmp[] = {
        {"img", &img, &img_}, {"nuc", &nuc, &nuc_}, {"jst", &jst, &jst_}, {"ncs", &ncs, &ncs_}, {"img2", &img2, &img2_},
        {"eimg", &eimg, &eimg_}, {"J4", &J4, &J4_}};
    for (auto& c : cmp) {
        CHECK(c.got->size() == c.want->size(), "images T %d xf %d var2 %d: %s has %zu entries, not %zu", T, has_xf, (int)var2, c.name,
              c.got->size(), c.want->size());
        size_t bad = 0, first = 0;
        for (size_t i = 0; i < c.got->size() && i < c.want->size(); ++i)
            if (!((*c.got)[i] == (*c.want)[i])) { if (!bad) first = i; ++bad; }
        CHECK(bad == 0, "images T %d xf %d var2 %d: %s differs in %zu entries, first at %zu", T, has_xf, (int)var2, c.name, bad, first);
    }
    CHECK(nuc4.size() == (size_t)nrow && std::equal(nuc4.begin(), nuc4.end(), nc0.begin()), "images: nuc4 is not nuc without its padding");
    if (!var2) {                                             // VAR(1): the x0_pre columns are zero wherever they appear
        bool zero = true;
        for (int r = 0; r < nrow; ++r)
            for (int c = n; c < 2 * n; ++c)
                zero = zero && J4[(size_t)r * nc + c] == 0.0 && img[((size_t)(r >> 4) * jksp + c / 4) * 64 + lane(r, c)] == 0.0 &&
                       img2[((size_t)(r >> 4) * jksp2 + c / 4) * 64 + lane(r, c)] == 0.0;
        CHECK(zero, "images T %d VAR(1): an x0_pre column is not zero", T);
    }
    // one NaN: refused.  Among the unit vectors of [x0 ; x0_pre ; w] it is met before the per-stage images exist; among the columns of
    // [B u1 ; B u2] after them, and jst / ncs are then complete (the caller uploads them before it looks at J')
    const double keep1 = slot(1 + 3, 5), keep2 = slot(1 + ncol + n + 2, nrow - 1);
    slot(1 + 3, 5) = NAN;
    CHECK(!fmpc_host_inverse_images(n, T, nb, var2, jks, jks2, a1.data(), a2.data(), nu, img, nuc, jst, ncs, img2, eimg, J4, nuc4) &&
          jst.empty() && ncs.empty(), "images T %d: a NaN in J was not refused before the per-stage images", T);
    slot(1 + 3, 5) = keep1;
    slot(1 + ncol + n + 2, nrow - 1) = NAN;
    CHECK(!fmpc_host_inverse_images(n, T, nb, var2, jks, jks2, a1.data(), a2.data(), nu, img, nuc, jst, ncs, img2, eimg, J4, nuc4) &&
          jst == jst_ && ncs == ncs_, "images T %d: a NaN in J' was not refused with the per-stage images complete", T);
    slot(1 + ncol + n + 2, nrow - 1) = keep2;
    slot(0, 0) = NAN;
    CHECK(!fmpc_host_inverse_images(n, T, nb, var2, jks, jks2, a1.data(), a2.data(), nu, img, nuc, jst, ncs, img2, eimg, J4, nuc4),
          "images T %d: a NaN in nuc was not refused", T);
    printf("images n %d T %d xf %d VAR(%d): %zu + %zu + %zu + %zu + %zu entries equal\n", n, T, has_xf, var2 ? 2 : 1, img.size(), img2.size(),
           jst_.size(), eimg_.size(), J4_.size());
}

// ---- fmpc_host_bank_desc
static void desc_case(int T, bool var2, bool has_xf, bool xf_is_x) {
    const int nb = T + (has_xf ? 1 : 0);
    FmpcBankTable tab;
    fmpc_host_bank_table(T, var2, has_xf, xf_is_x, tab);
    std::vector<int> ids;
    fmpc_host_bank_desc(tab, nb, ids);
    const int nblk = (int)tab.blocks.size();
    CHECK(ids.size() == (size_t)nblk * FB_DESC_INTS + 3 * (size_t)nb, "desc T %d: %zu ints for %d blocks, %d rows", T, ids.size(), nblk, nb);
    if (ids.size() != (size_t)nblk * FB_DESC_INTS + 3 * (size_t)nb) return;
    for (int k = 0; k < nblk; ++k) {
        const int* d = ids.data() + (size_t)k * FB_DESC_INTS;
        CHECK(d[0] == tab.blocks[k].nterms, "desc T %d: block %d has %d terms, not %d", T, k, d[0], tab.blocks[k].nterms);
        for (int q = 0; q < FB_MAX_TERMS; ++q) {
            const FmpcBankTerm& tm = tab.blocks[k].t[q];
            if (q < tab.blocks[k].nterms)
                CHECK(d[1 + 4 * q] == tm.sign && d[2 + 4 * q] == tm.L && d[3 + 4 * q] == tm.X && d[4 + 4 * q] == tm.R, "desc T %d: block %d term %d", T, k, q);
            else
                CHECK(d[1 + 4 * q] == 0 && d[2 + 4 * q] == 0 && d[3 + 4 * q] == 0 && d[4 + 4 * q] == 0, "desc T %d: block %d term %d is not zero", T, k, q);
        }
    }
    const int* ix = ids.data() + (size_t)nblk * FB_DESC_INTS;
    const std::vector<int>* src[3] = {&tab.idxD, &tab.idx1, &tab.idx2};
    for (int w = 0; w < 3; ++w)
        for (int i = 0; i < nb; ++i) {
            const int want = (*src[w])[i] >= 0 ? (*src[w])[i] : nblk;        // none: the zero block behind the table's
            CHECK(ix[w * nb + i] == want && want <= nblk, "desc T %d: index %d of row %d is %d, not %d", T, w, i, ix[w * nb + i], want);
        }
    for (int i = 0; i < nb; ++i) CHECK(tab.idxD[i] >= 0, "desc T %d: row %d has no diagonal block", T, i);
}

// ---- fmpc_host_spd_inverse, fmpc_host_is_diag, fmpc_host_cm
static void spd_case(int seed) {
    const int n = 8;
    const double cond = 1e4;
    std::mt19937_64 rng(seed);
    std::normal_distribution<double> N01(0.0, 1.0);
    // A = H D H with the reflection H = I - 2 v v' / v'v and D = cond^(i / (n - 1)): eigenvalues 1 .. cond
    std::vector<ld> v(n), H((size_t)n * n);
    ld vv = 0.0L;
    for (ld& x : v) { x = N01(rng); vv += x * x; }
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) H[(size_t)a * n + b] = (a == b ? 1.0L : 0.0L) - 2.0L * v[a] * v[b] / vv;
    std::vector<double> A((size_t)n * n), inv;
    for (int a = 0; a < n; ++a)
        for (int b = 0; b <= a; ++b) {
            ld t = 0.0L;
            for (int c = 0; c < n; ++c) t += H[(size_t)a * n + c] * powl((ld)cond, (ld)c / (n - 1)) * H[(size_t)b * n + c];
            A[(size_t)a * n + b] = A[(size_t)b * n + a] = (double)t;
        }
    CHECK(fmpc_host_spd_inverse(A, n, inv), "spd_inverse: a positive definite matrix refused");
    ld worst = 0.0L;
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) {
            ld t = 0.0L;
            for (int c = 0; c < n; ++c) t += (ld)A[(size_t)a * n + c] * (ld)inv[(size_t)c * n + b];
            worst = fmaxl(worst, fabsl(t - (a == b ? 1.0L : 0.0L)));
            CHECK(inv[(size_t)a * n + b] == inv[(size_t)b * n + a], "spd_inverse: the inverse is not symmetric at (%d, %d)", a, b);
        }
    const ld bound = 64.0L * n * EPS * cond;
    CHECK(worst <= bound, "spd_inverse: A inv - I = %.3Le, bound %.3Le", worst, bound);
    printf("spd_inverse n %d cond %.0e: A inv - I %.2Le (bound %.2Le)\n", n, cond, worst, bound);
    std::vector<double> Z = A;
    Z[0] = 0.0;                                                  // a zero first pivot
    CHECK(!fmpc_host_spd_inverse(Z, n, inv), "spd_inverse: a zero pivot was not refused");
    Z = A;
    for (int c = 0; c < n; ++c) Z[(size_t)3 * n + c] = Z[(size_t)c * n + 3] = 0.0;      // a zero row and column: pivot 3 is exactly zero
    CHECK(!fmpc_host_spd_inverse(Z, n, inv), "spd_inverse: a zero row was not refused");
    // column-major element and the diagonal test of fmpc_create
    const double M[6] = {1, 2, 3, 4, 5, 6};                     // 3 x 2 column-major
    CHECK(fmpc_host_cm(M, 3, 2, 0) == 3 && fmpc_host_cm(M, 3, 0, 1) == 4 && fmpc_host_cm(M, 3, 1, 1) == 5, "fmpc_host_cm");
    std::vector<double> D((size_t)n * n, 0.0);
    for (int a = 0; a < n; ++a) D[(size_t)a * n + a] = 1.0 + a;
    CHECK(fmpc_host_is_diag(D.data(), n), "is_diag: a diagonal matrix");
    D[(size_t)(n - 1) * n] = 1e-300;                            // row 0, column n - 1
    CHECK(!fmpc_host_is_diag(D.data(), n), "is_diag: one entry off the diagonal");
}

int main() {
    // (27, 16, 1) has rank 16 < 27: B diag(a^2) B' is singular, the function's answer there is a refusal; (27, 40, 1) is the
    // smallest-horizon case with a factor
    const int shapes[4][3] = {{27, 144, 2}, {27, 16, 1}, {27, 40, 1}, {5, 8, 3}};
    for (int s = 0; s < 4; ++s) constants_case(shapes[s][0], shapes[s][1], shapes[s][2], 100 + s);
    for (int T = 2; T <= 3; ++T)
        for (int xf = 0; xf < 2; ++xf)
            for (int var2 = 0; var2 < 2; ++var2) images_case(27, T, xf, var2 != 0, 200 + 4 * T + 2 * xf + var2);
    for (int T = 1; T <= 3; ++T)
        for (int var2 = 0; var2 < 2; ++var2)
            for (int xf = 0; xf < 2; ++xf)
                for (int same = 0; same < 2; ++same) desc_case(T, var2 != 0, xf != 0, same != 0);
    spd_case(300);
    if (fails) { printf("%d checks failed\n", fails); return 1; }
    printf("ok\n");
    return 0;
}
