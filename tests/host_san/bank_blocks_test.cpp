// The block table of a model bank (fmpc_host_bank_table, csrc/fmpc_bank.h) against the content-based blocks of the handle's one
// model (fmpc_host_y_blocks), under AddressSanitizer + UndefinedBehaviorSanitizer:
//   generic random model: the structural table lists the same blocks at the same positions (idxD / idx1 / idx2 equal), and every
//   block evaluated in long double reproduces the content-based one to 1e-14 relative -- with Qf != Q and with Qf == Q;
//   a model with A2 = 0 handed to a var_order-2 table: the content-based count shrinks (blocks coincide by their numbers), the
//   structural one keeps the generic count -- the reason the table exists (one table for all models of a bank).
// usage: bank_blocks_test n T var_order has_xf seed
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include <vector>

#include "../../mpc-sensorlessao_amd/csrc/fmpc_bank.h"
#include "../../mpc-sensorlessao_amd/csrc/fmpc_host.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static void spd_inverse_of_2(const std::vector<double>& Q, int n, bool diag, std::vector<double>& X) {
    // (2Q)^-1 for a diagonal Q exactly as a reciprocal, else by Gauss-Jordan in long double
    X.assign((size_t)n * n, 0.0);
    if (diag) { for (int a = 0; a < n; ++a) X[(size_t)a * n + a] = 1.0 / (2.0 * Q[(size_t)a * n + a]); return; }
    std::vector<long double> M((size_t)n * 2 * n, 0.0L);
    for (int a = 0; a < n; ++a) { for (int b = 0; b < n; ++b) M[(size_t)a * 2 * n + b] = 2.0L * Q[(size_t)a * n + b]; M[(size_t)a * 2 * n + n + a] = 1.0L; }
    for (int c = 0; c < n; ++c) {
        const long double pv = M[(size_t)c * 2 * n + c];
        for (int b = 0; b < 2 * n; ++b) M[(size_t)c * 2 * n + b] /= pv;
        for (int a = 0; a < n; ++a) if (a != c) {
            const long double f = M[(size_t)a * 2 * n + c];
            for (int b = 0; b < 2 * n; ++b) M[(size_t)a * 2 * n + b] -= f * M[(size_t)c * 2 * n + b];
        }
    }
    for (int a = 0; a < n; ++a) for (int b = 0; b < n; ++b) X[(size_t)a * n + b] = (double)M[(size_t)a * 2 * n + n + b];
}

int main(int argc, char** argv) {
    if (argc < 6) { printf("usage: %s n T var_order has_xf seed\n", argv[0]); return 2; }
    const int n = atoi(argv[1]), T = atoi(argv[2]), var_order = atoi(argv[3]), has_xf = atoi(argv[4]), seed = atoi(argv[5]);
    const int nn = n * n, nb = T + (has_xf ? 1 : 0);
    const bool var2 = var_order == 2;
    std::mt19937_64 rng(seed);
    std::normal_distribution<double> N01(0.0, 1.0);
    std::vector<double> a1(nn), a2(nn, 0.0);
    for (double& v : a1) v = 0.5 * N01(rng);
    if (var2) for (double& v : a2) v = 0.3 * N01(rng);
    for (int dense = 0; dense < 2; ++dense)
        for (int same_q = 0; same_q < 2; ++same_q) {
            std::vector<double> Q(nn, 0.0), Qf(nn, 0.0);
            for (int a = 0; a < n; ++a) { Q[(size_t)a * n + a] = 1.0 + 0.1 * a; Qf[(size_t)a * n + a] = 50.0 + a; }
            if (dense) {
                std::vector<double> G(nn);
                for (double& v : G) v = N01(rng) / sqrt((double)n);
                for (int a = 0; a < n; ++a) for (int b = 0; b < n; ++b) {
                    double t = 0.0;
                    for (int k = 0; k < n; ++k) t += G[(size_t)a * n + k] * G[(size_t)b * n + k];
                    Q[(size_t)a * n + b] += 0.3 * t; Qf[(size_t)a * n + b] += 2.0 * t;
                }
            }
            if (same_q) Qf = Q;
            std::vector<double> X, Xf;
            spd_inverse_of_2(Q, n, !dense, X); spd_inverse_of_2(Qf, n, !dense, Xf);
            const bool xf_is_x = memcmp(X.data(), Xf.data(), nn * sizeof(double)) == 0;
            CHECK(xf_is_x == (same_q != 0), "Xf == X: %d, Qf == Q: %d", (int)xf_is_x, same_q);
            std::vector<std::vector<double>> blocks;
            std::vector<int> iD, i1, i2;
            fmpc_host_y_blocks(n, T, var2, has_xf != 0, a1, a2, X, Xf, blocks, iD, i1, i2);
            FmpcBankTable tab;
            fmpc_host_bank_table(T, var2, has_xf != 0, xf_is_x, tab);
            CHECK(tab.blocks.size() == blocks.size(), "dense %d same_q %d: %zu structural blocks, %zu by content", dense, same_q, tab.blocks.size(), blocks.size());
            CHECK((int)tab.idxD.size() == nb && tab.idxD == iD && tab.idx1 == i1 && tab.idx2 == i2, "dense %d same_q %d: index arrays differ", dense, same_q);
            double worst = 0.0;
            for (size_t k = 0; k < tab.blocks.size() && k < blocks.size(); ++k) {
                CHECK(tab.blocks[k].nterms >= 1 && tab.blocks[k].nterms <= FB_MAX_TERMS, "block %zu: %d terms", k, tab.blocks[k].nterms);
                std::vector<long double> ev;
                fmpc_host_bank_eval(tab.blocks[k], n, a1.data(), a2.data(), X.data(), Xf.data(), ev);
                long double num = 0.0L, den = 0.0L;
                for (int q = 0; q < nn; ++q) { const long double d = ev[q] - (long double)blocks[k][q]; num += d * d; den += ev[q] * ev[q]; }
                const double rel = (double)sqrtl(num / (den > 0 ? den : 1.0L));
                if (rel > worst) worst = rel;
            }
            CHECK(worst <= 1e-14, "dense %d same_q %d: block differs by %.3e relative", dense, same_q, worst);
            printf("n %d T %d var_order %d xf %d dense %d Qf==Q %d: %zu blocks, worst %.2e\n", n, T, var_order, has_xf, dense, same_q, blocks.size(), worst);
            // A2 = 0 in a var_order-2 handle: coincidences by the numbers of one model
            if (var2 && T >= 4) {
                std::vector<double> z2(nn, 0.0);
                std::vector<std::vector<double>> b0;
                std::vector<int> d0, o1, o2;
                fmpc_host_y_blocks(n, T, true, has_xf != 0, a1, z2, X, Xf, b0, d0, o1, o2);
                CHECK(b0.size() < blocks.size(), "A2 = 0: %zu blocks by content, generic %zu", b0.size(), blocks.size());
                CHECK(tab.blocks.size() == blocks.size(), "A2 = 0: the structural table does not depend on the model");
                // ... and still describes that model: every position evaluates to the content-based block there
                for (int i = 0; i < nb; ++i)
                    for (int which = 0; which < 3; ++which) {
                        const int ks = which == 0 ? tab.idxD[i] : (which == 1 ? tab.idx1[i] : tab.idx2[i]);
                        const int kc = which == 0 ? d0[i] : (which == 1 ? o1[i] : o2[i]);
                        CHECK((ks < 0) == (kc < 0), "A2 = 0: row %d kind %d present in one table only", i, which);
                        if (ks < 0 || kc < 0) continue;
                        std::vector<long double> ev;
                        fmpc_host_bank_eval(tab.blocks[ks], n, a1.data(), z2.data(), X.data(), Xf.data(), ev);
                        long double num = 0.0L, den = 0.0L;
                        for (int q = 0; q < nn; ++q) { const long double d = ev[q] - (long double)b0[kc][q]; num += d * d; den += (long double)b0[kc][q] * b0[kc][q]; }
                        CHECK(num <= 1e-28L * (den > 0 ? den : 1.0L), "A2 = 0: row %d kind %d differs", i, which);
                    }
            }
        }
    if (fails) { printf("%d checks failed\n", fails); return 1; }
    printf("ok\n");
    return 0;
}
