// Host-only builders (see fmpc_host.h).  Plain C++: also compiled by g++ with the address and undefined-behaviour
// sanitizers (tests/host_san).
#include "fmpc_host.h"
#include "fmpc_bank.h"
#include "../../include/fastmpc.h"      // fmpc_noise, the status codes
#include "fmpc_noise.h"
#include "fmpc_detector.h"
#include "fmpc_atm.h"

#include <algorithm>
#include <cmath>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

bool fmpc_host_is_diag(const double* M, int n) {
    for (int c = 0; c < n; ++c)
        for (int r = 0; r < n; ++r)
            if (r != c && fmpc_host_cm(M, n, r, c) != 0.0) return false;
    return true;
}

bool fmpc_host_spd_inverse(const std::vector<double>& A, int n, std::vector<double>& inv) {
    typedef long double ld;
    std::vector<ld> L((size_t)n * n, 0.0L), Li((size_t)n * n, 0.0L);
    for (int c = 0; c < n; ++c) {
        ld d = A[c * n + c];
        for (int k = 0; k < c; ++k) d -= L[c * n + k] * L[c * n + k];
        if (!(d > 0.0L)) return false;
        const ld l = sqrtl(d);
        L[c * n + c] = l;
        for (int r = c + 1; r < n; ++r) {
            ld t = A[r * n + c];
            for (int k = 0; k < c; ++k) t -= L[r * n + k] * L[c * n + k];
            L[r * n + c] = t / l;
        }
    }
    for (int c = 0; c < n; ++c) {                    // Li = L^-1
        Li[c * n + c] = 1.0L / L[c * n + c];
        for (int r = c + 1; r < n; ++r) {
            ld t = 0.0L;
            for (int k = c; k < r; ++k) t += L[r * n + k] * Li[k * n + c];
            Li[r * n + c] = -t / L[r * n + r];
        }
    }
    inv.assign((size_t)n * n, 0.0);
    for (int a = 0; a < n; ++a)
        for (int b = 0; b <= a; ++b) {
            ld t = 0.0L;
            for (int k = a; k < n; ++k) t += Li[k * n + a] * Li[k * n + b];
            inv[a * n + b] = inv[b * n + a] = (double)t;
        }
    return true;
}

void fmpc_host_add_AXBt(std::vector<double>& out, const std::vector<double>& A, const std::vector<double>& X,
                        const std::vector<double>& B, int n, double sign) {
    std::vector<double> AX((size_t)n * n, 0.0);
    for (int a = 0; a < n; ++a)
        for (int c = 0; c < n; ++c) {
            double t = 0.0;
            for (int k = 0; k < n; ++k) t += A[a * n + k] * X[k * n + c];
            AX[a * n + c] = t;
        }
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) {
            double t = 0.0;
            for (int c = 0; c < n; ++c) t += AX[a * n + c] * B[b * n + c];
            out[a * n + b] += sign * t;
        }
}

void fmpc_host_y_blocks(int n, int T, bool var2, bool has_xf, const std::vector<double>& a1, const std::vector<double>& a2,
                        const std::vector<double>& X, const std::vector<double>& Xf,
                        std::vector<std::vector<double>>& blocks, std::vector<int>& idxD, std::vector<int>& idx1, std::vector<int>& idx2) {
    const int nn = n * n, nb = T + (has_xf ? 1 : 0);
    blocks.clear();
    idxD.assign(nb, -1); idx1.assign(nb, -1); idx2.assign(nb, -1);
    auto intern = [&](const std::vector<double>& blk) {
        for (size_t k = 0; k < blocks.size(); ++k)
            if (memcmp(blocks[k].data(), blk.data(), nn * sizeof(double)) == 0) return (int)k;
        blocks.push_back(blk);
        return (int)blocks.size() - 1;
    };
    auto Xj = [&](int j) -> const std::vector<double>& { return j == T ? Xf : X; };
    std::vector<double> eye(nn, 0.0);
    for (int a = 0; a < n; ++a) eye[a * n + a] = 1.0;
    for (int i = 0; i < T; ++i) {
        std::vector<double> d = Xj(i + 1);
        if (i >= 1) fmpc_host_add_AXBt(d, a1, Xj(i), a1, n, 1.0);
        if (i >= 2 && var2) fmpc_host_add_AXBt(d, a2, Xj(i - 1), a2, n, 1.0);
        idxD[i] = intern(d);
        if (i + 1 < T) {
            std::vector<double> o(nn, 0.0);
            fmpc_host_add_AXBt(o, eye, Xj(i + 1), a1, n, -1.0);              // -X_{i+1} A1'
            if (i >= 1 && var2) fmpc_host_add_AXBt(o, a1, Xj(i), a2, n, 1.0);
            idx1[i] = intern(o);
        }
        if (i + 2 < T && var2) {
            std::vector<double> o(nn, 0.0);
            fmpc_host_add_AXBt(o, eye, Xj(i + 1), a2, n, -1.0);              // -X_{i+1} A2'
            idx2[i] = intern(o);
        }
    }
    if (has_xf) {
        idxD[T] = intern(Xf);
        idx1[T - 1] = idxD[T];
    }
}

int fmpc_host_model_classify(int n, int m, const double* Q, const double* R, const double* Qf, FmpcHostModel& M) {
    // dense (symmetric positive definite) Q, Qf, R: fast_mpc_objective.m:51-55 takes any square matrices (the tiled kernel's part)
    const bool denseR = !fmpc_host_is_diag(R, m), denseQ = !fmpc_host_is_diag(Q, n) || !fmpc_host_is_diag(Qf, n);
    std::vector<double>& R2full = M.r2full;
    M.denseQ = denseQ ? 1 : 0; M.denseR = denseR ? 1 : 0; R2full.clear();
    for (int i = 0; i < n; ++i)
        if (!(fmpc_host_cm(Q, n, i, i) > 0.0) || !(fmpc_host_cm(Qf, n, i, i) > 0.0)) return FMPC_E_NOT_PD_PHI;
    for (int i = 0; i < m; ++i)
        if (!(fmpc_host_cm(R, m, i, i) > 0.0)) return FMPC_E_NOT_PD_PHI;
    if (denseQ)
        for (int a = 0; a < n; ++a)
            for (int b = 0; b < a; ++b)
                if (fmpc_host_cm(Q, n, a, b) != fmpc_host_cm(Q, n, b, a) || fmpc_host_cm(Qf, n, a, b) != fmpc_host_cm(Qf, n, b, a)) return FMPC_E_NOT_PD_PHI;
    if (denseR) {
        R2full.assign((size_t)m * m, 0.0);
        for (int a = 0; a < m; ++a)
            for (int b = 0; b < m; ++b) {
                if (fmpc_host_cm(R, m, a, b) != fmpc_host_cm(R, m, b, a)) return FMPC_E_NOT_PD_PHI;
                R2full[(size_t)a * m + b] = 2.0 * fmpc_host_cm(R, m, a, b);
            }
        std::vector<double> tmp;
        if (!fmpc_host_spd_inverse(R2full, m, tmp)) return FMPC_E_NOT_PD_PHI;      // (the inverse itself is not used: a positive definiteness test)
    }
    return FMPC_OK;
}

int fmpc_host_build_model(int n, int m, int T, int var_order, const double* A1, const double* A2, const double* B,
                          const double* Q, const double* R, const double* Qf, const double* q, const double* r, const double* qf,
                          const double* x_min, const double* x_max, const double* u_min, const double* u_max, const double* xf,
                          FmpcHostModel& M) {
    const bool var2 = var_order == 2;
    const int nn = n * n;
    M.n = n; M.m = m; M.T = T; M.has_xf = xf ? 1 : 0; M.nb = T + M.has_xf; M.var2 = var2 ? 1 : 0;
    // ---- row-major copies
    M.a1.assign(nn, 0.0); M.a2.assign(nn, 0.0); M.bt.assign((size_t)m * n, 0.0); M.b.assign((size_t)n * m, 0.0);
    for (int rr = 0; rr < n; ++rr)
        for (int c = 0; c < n; ++c) {
            M.a1[rr * n + c] = fmpc_host_cm(A1, n, rr, c);
            if (var2) M.a2[rr * n + c] = fmpc_host_cm(A2, n, rr, c);
        }
    for (int rr = 0; rr < n; ++rr)
        for (int c = 0; c < m; ++c) M.bt[(size_t)c * n + rr] = M.b[(size_t)rr * m + c] = fmpc_host_cm(B, n, rr, c);
    M.R2.resize(m); M.Q2.resize(n); M.Qf2.resize(n);
    for (int i = 0; i < m; ++i) M.R2[i] = 2.0 * fmpc_host_cm(R, m, i, i);
    for (int i = 0; i < n; ++i) { M.Q2[i] = 2.0 * fmpc_host_cm(Q, n, i, i); M.Qf2[i] = 2.0 * fmpc_host_cm(Qf, n, i, i); }
    M.rl.assign(m, 0.0); if (r) M.rl.assign(r, r + m);
    M.ql.assign(n, 0.0); if (q) M.ql.assign(q, q + n);
    M.qfl.assign(n, 0.0); if (qf) M.qfl.assign(qf, qf + n);
    M.umin.assign(u_min, u_min + m); M.umax.assign(u_max, u_max + m);
    M.umid.resize(m); M.xmid.resize(n);
    for (int i = 0; i < m; ++i) M.umid[i] = (u_min[i] + u_max[i]) / 2;    // fast_mpc_init.m:19-20
    for (int i = 0; i < n; ++i) M.xmid[i] = (x_min[i] + x_max[i]) / 2;
    M.xf.clear(); if (xf) M.xf.assign(xf, xf + n);
    // X = (2Q)^-1, Xf = (2Qf)^-1 as dense row-major matrices (diagonal weights: diagonal matrices)
    M.q2m.assign(nn, 0.0); M.qf2m.assign(nn, 0.0); M.xm.assign(nn, 0.0); M.xfm.assign(nn, 0.0);
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) { M.q2m[a * n + b] = 2.0 * fmpc_host_cm(Q, n, a, b); M.qf2m[a * n + b] = 2.0 * fmpc_host_cm(Qf, n, a, b); }
    if (M.denseQ) {
        if (!fmpc_host_spd_inverse(M.q2m, n, M.xm) || !fmpc_host_spd_inverse(M.qf2m, n, M.xfm)) return FMPC_E_NOT_PD_PHI;
    } else {
        for (int i = 0; i < n; ++i) { M.xm[i * n + i] = 1.0 / M.Q2[i]; M.xfm[i * n + i] = 1.0 / M.Qf2[i]; }
    }
    // ---- iteration-invariant Y blocks, deduplicated; the kernels index them as Yblk + idx*n*n: no padding
    std::vector<std::vector<double>> blocks;
    fmpc_host_y_blocks(n, T, var2, xf != nullptr, M.a1, M.a2, M.xm, M.xfm, blocks, M.idxD, M.idx1, M.idx2);
    M.blocks.clear();
    for (auto& bk : blocks) M.blocks.insert(M.blocks.end(), bk.begin(), bk.end());
    // closed-loop prediction matrices (main.mlx, MPC_DesignMatrices): M1_0 = A1, M2_0 = A2, M1_1 = A1^2 + A2,
    // M2_1 = A1 A2, M1_i = A1 M1_{i-1} + A2 M1_{i-2}, M2_i = M1_{i-1} A2
    M.m1.assign((size_t)T * nn, 0.0); M.m2.assign((size_t)T * nn, 0.0);
    auto mul = [&](const double* X, const double* Y, double* Z, double beta) {     // Z = beta Z + X Y (n x n row-major)
        for (int rr = 0; rr < n; ++rr)
            for (int c = 0; c < n; ++c) {
                double t = 0.0;
                for (int qq = 0; qq < n; ++qq) t += X[rr * n + qq] * Y[qq * n + c];
                Z[rr * n + c] = beta * Z[rr * n + c] + t;
            }
    };
    const double* a1 = M.a1.data(); const double* a2 = M.a2.data();
    for (int i = 0; i < T; ++i) {
        double* m1 = M.m1.data() + (size_t)i * nn; double* m2 = M.m2.data() + (size_t)i * nn;
        if (i == 0) { for (int e = 0; e < nn; ++e) { m1[e] = a1[e]; m2[e] = a2[e]; } }
        else if (i == 1) { for (int e = 0; e < nn; ++e) m1[e] = a2[e]; mul(a1, a1, m1, 1.0); mul(a1, a2, m2, 0.0); }
        else {
            mul(a1, m1 - nn, m1, 0.0); mul(a2, m1 - 2 * nn, m1, 1.0);
            mul(m1 - nn, a2, m2, 0.0);
        }
    }
    return FMPC_OK;
}

void fmpc_host_wave_cold(const FmpcHostModel& M, double k, const int o[14], std::vector<double>& c) {
    const int n = M.n, m = M.m;
    c.assign((size_t)o[8], 0.0);
    for (int j = 0; j < m; ++j) { const FmpcHostModel::Box b = M.box(j, k); c[o[0] + j] = b.cu; c[o[1] + j] = b.hc; c[o[2] + j] = b.wc; }
    const double* bt = M.bt.data();                               // bt[c*n + r] = B[r][c]
    for (int a = 0; a < n; ++a) {
        double cbu = 0.0, bu = 0.0;
        for (int j = 0; j < m; ++j) {
            cbu += bt[(size_t)j * n + a] * c[o[2] + j] * c[o[0] + j];
            bu += bt[(size_t)j * n + a] * M.umid[j];
        }
        c[o[4] + a] = cbu;
        double a1x = 0.0, a2x = 0.0;
        for (int q = 0; q < n; ++q) { a1x += M.a1[a * n + q] * M.xmid[q]; a2x += M.a2[a * n + q] * M.xmid[q]; }
        c[o[5] + a] = M.xmid[a] - bu;
        c[o[6] + a] = M.xmid[a] - bu - a1x;
        c[o[7] + a] = M.xmid[a] - bu - a1x - a2x;
        double va = 0.0, va2 = 0.0;
        for (int j = 0; j < m; ++j) {
            const double aj = c[o[1] + j] * c[o[2] + j];
            va += bt[(size_t)j * n + a] * aj * c[o[0] + j];
            va2 += bt[(size_t)j * n + a] * aj * aj * c[o[0] + j];
        }
        c[o[11] + a] = va; c[o[12] + a] = va2;
        for (int b = 0; b < n; ++b) {
            double g = 0.0, ma = 0.0, ma2 = 0.0;
            for (int j = 0; j < m; ++j) {
                const double bb = bt[(size_t)j * n + a] * bt[(size_t)j * n + b];
                const double aj = c[o[1] + j] * c[o[2] + j];
                g += bb * c[o[2] + j]; ma += bb * aj; ma2 += bb * aj * aj;
            }
            c[o[3] + a * n + b] = g; c[o[9] + a * n + b] = ma; c[o[10] + a * n + b] = ma2;
        }
    }
    for (int j = 0; j < m; ++j) {
        const double aj = c[o[1] + j] * c[o[2] + j], cu = c[o[0] + j];
        c[o[13]] += aj * cu * cu; c[o[13] + 1] += aj * aj * cu * cu;
    }
}

// The block table of a model bank (fmpc_bank.h): the walk of fmpc_host_y_blocks above with term lists in place of numbers.
void fmpc_host_bank_table(int T, bool var2, bool has_xf, bool xf_is_x, FmpcBankTable& out) {
    const int nb = T + (has_xf ? 1 : 0);
    out.blocks.clear();
    out.idxD.assign(nb, -1); out.idx1.assign(nb, -1); out.idx2.assign(nb, -1);
    auto kind = [&](int j) { return (j == T && !xf_is_x) ? FB_XF : FB_X; };
    auto intern = [&](const FmpcBankBlock& blk) {
        for (size_t k = 0; k < out.blocks.size(); ++k) {
            const FmpcBankBlock& o = out.blocks[k];
            bool same = o.nterms == blk.nterms;
            for (int t = 0; same && t < blk.nterms; ++t)
                same = o.t[t].sign == blk.t[t].sign && o.t[t].L == blk.t[t].L && o.t[t].X == blk.t[t].X && o.t[t].R == blk.t[t].R;
            if (same) return (int)k;
        }
        out.blocks.push_back(blk);
        return (int)out.blocks.size() - 1;
    };
    auto add = [](FmpcBankBlock& blk, int sign, int L, int X, int R) { blk.t[blk.nterms++] = FmpcBankTerm{sign, L, X, R}; };
    for (int i = 0; i < T; ++i) {
        FmpcBankBlock d{};
        add(d, 1, FB_I, kind(i + 1), FB_I);
        if (i >= 1) add(d, 1, FB_A1, kind(i), FB_A1);
        if (i >= 2 && var2) add(d, 1, FB_A2, kind(i - 1), FB_A2);
        out.idxD[i] = intern(d);
        if (i + 1 < T) {
            FmpcBankBlock o{};
            add(o, -1, FB_I, kind(i + 1), FB_A1);
            if (i >= 1 && var2) add(o, 1, FB_A1, kind(i), FB_A2);
            out.idx1[i] = intern(o);
        }
        if (i + 2 < T && var2) {
            FmpcBankBlock o{};
            add(o, -1, FB_I, kind(i + 1), FB_A2);
            out.idx2[i] = intern(o);
        }
    }
    if (has_xf) {
        FmpcBankBlock d{};
        add(d, 1, FB_I, kind(T), FB_I);
        out.idxD[T] = intern(d);
        out.idx1[T - 1] = out.idxD[T];
    }
}

void fmpc_host_bank_eval(const FmpcBankBlock& blk, int n, const double* a1, const double* a2, const double* X, const double* Xf,
                         std::vector<long double>& out) {
    out.assign((size_t)n * n, 0.0L);
    std::vector<long double> LX((size_t)n * n);
    auto el = [&](int which, int r, int c) -> long double {
        return which == FB_I ? (r == c ? 1.0L : 0.0L) : (long double)(which == FB_A1 ? a1 : a2)[(size_t)r * n + c];
    };
    for (int t = 0; t < blk.nterms; ++t) {
        const FmpcBankTerm& tm = blk.t[t];
        const double* Xk = tm.X == FB_XF ? Xf : X;
        for (int a = 0; a < n; ++a)
            for (int c = 0; c < n; ++c) {
                long double v = 0.0L;
                for (int k = 0; k < n; ++k) v += el(tm.L, a, k) * (long double)Xk[(size_t)k * n + c];
                LX[(size_t)a * n + c] = v;
            }
        for (int a = 0; a < n; ++a)
            for (int b = 0; b < n; ++b) {
                long double v = 0.0L;
                for (int c = 0; c < n; ++c) v += LX[(size_t)a * n + c] * el(tm.R, b, c);
                out[(size_t)a * n + b] += tm.sign * v;
            }
    }
}

void fmpc_host_bank_desc(const FmpcBankTable& tab, int nb, std::vector<int>& ids) {
    const int nblk = (int)tab.blocks.size();
    ids.assign((size_t)nblk * FB_DESC_INTS, 0);
    for (int k = 0; k < nblk; ++k) {
        int* d = ids.data() + (size_t)k * FB_DESC_INTS;
        d[0] = tab.blocks[k].nterms;
        for (int q = 0; q < tab.blocks[k].nterms; ++q) {
            const FmpcBankTerm& tm = tab.blocks[k].t[q];
            d[1 + 4 * q] = tm.sign; d[2 + 4 * q] = tm.L; d[3 + 4 * q] = tm.X; d[4 + 4 * q] = tm.R;
        }
    }
    for (int i = 0; i < nb; ++i) ids.push_back(tab.idxD[i]);
    for (int i = 0; i < nb; ++i) ids.push_back(tab.idx1[i] >= 0 ? tab.idx1[i] : nblk);
    for (int i = 0; i < nb; ++i) ids.push_back(tab.idx2[i] >= 0 ? tab.idx2[i] : nblk);
}

bool fmpc_host_bank_first_constants(int n, int m, int T, double k, const double* bt, const double* umax, const double* umin,
                                    const double* umid, const double* R2, const double* rl, std::vector<double>& cst) {
    typedef long double ld;
    const int NX = 32;
    cst.assign((size_t)NX * NX + NX + 8, 0.0);
    std::vector<ld> a2(m), cu(m), Ma((size_t)n * n, 0.0L), v0(n, 0.0L), Lm((size_t)n * n, 0.0L), y0(n, 0.0L);
    ld acu2 = 0.0L;
    for (int j = 0; j < m; ++j) {
        const double sp = umax[j] - umid[j], sm = umid[j] - umin[j];
        const double dp = 1.0 / sp, dm = 1.0 / sm;
        const double hc = k * (dp * dp + dm * dm);
        cu[j] = (ld)(R2[j] * umid[j] + rl[j] + k * (dp - dm));
        const double av = hc * (1.0 / (R2[j] + hc));
        a2[j] = (ld)av * (ld)av;
        acu2 += a2[j] * cu[j] * cu[j];
    }
    for (int r = 0; r < n; ++r) {
        for (int q = 0; q < n; ++q) { ld t = 0.0L; for (int j = 0; j < m; ++j) t += (ld)bt[(size_t)j * n + r] * a2[j] * (ld)bt[(size_t)j * n + q]; Ma[(size_t)r * n + q] = t; }
        for (int j = 0; j < m; ++j) v0[r] += (ld)bt[(size_t)j * n + r] * a2[j] * cu[j];
    }
    for (int j = 0; j < n; ++j) {                                  // Cholesky; not positive definite: no form for this handle
        ld d = Ma[(size_t)j * n + j];
        for (int q = 0; q < j; ++q) d -= Lm[(size_t)j * n + q] * Lm[(size_t)j * n + q];
        if (!(d > 0.0L) || !std::isfinite((double)d)) return false;
        const ld dj = sqrtl(d);
        Lm[(size_t)j * n + j] = dj;
        for (int i = j + 1; i < n; ++i) {
            ld t = Ma[(size_t)i * n + j];
            for (int q = 0; q < j; ++q) t -= Lm[(size_t)i * n + q] * Lm[(size_t)j * n + q];
            Lm[(size_t)i * n + j] = t / dj;
        }
    }
    ld y2 = 0.0L, lf2 = 0.0L;
    for (int i = 0; i < n; ++i) {
        ld t = v0[i];
        for (int q = 0; q < i; ++q) t -= Lm[(size_t)i * n + q] * y0[q];
        y0[i] = t / Lm[(size_t)i * n + i];
        y2 += y0[i] * y0[i];
    }
    for (int i = 0; i < n; ++i)
        for (int q = 0; q <= i; ++q) { cst[(size_t)q * NX + i] = (double)Lm[(size_t)i * n + q]; lf2 += Lm[(size_t)i * n + q] * Lm[(size_t)i * n + q]; }
    for (int i = 0; i < n; ++i) cst[(size_t)NX * NX + i] = (double)y0[i];
    const ld c0 = (ld)T * (acu2 - y2);
    cst[(size_t)NX * NX + NX] = (double)(c0 > 0.0L ? c0 : 0.0L);
    cst[(size_t)NX * NX + NX + 1] = (double)lf2 * (1.0 + 1e-12);
    cst[(size_t)NX * NX + NX + 2] = (double)((ld)T * y2) * (1.0 + 1e-12);
    return true;
}

bool fmpc_host_inverse_images(int n, int T, int nb, bool var2, int jks, int jks2, const double* a1, const double* a2,
                              const std::vector<double>& nu, std::vector<double>& img, std::vector<double>& nuc,
                              std::vector<double>& jst, std::vector<double>& ncs, std::vector<double>& img2,
                              std::vector<double>& eimg, std::vector<double>& J4, std::vector<double>& nuc4) {
    const int TN = T * n, nrow = nb * n, ncol = 2 * n + TN;
    const double scale = FMPC_INV_SCALE;
    jst.clear(); ncs.clear();
    auto at = [&](int p, int row) { return nu[((size_t)(p / FP_NP) * nrow + row) * FP_NP + (p % FP_NP)]; };
    const int nrt = (nrow + 15) / 16, jksp = 16 * ((jks + 15) / 16 + 3);
    img.assign((size_t)nrt * jksp * 64, 0.0); nuc.assign((size_t)nrt * 16, 0.0);
    for (int r = 0; r < nrow; ++r) {
        nuc[r] = at(0, r);
        if (!std::isfinite(nuc[r])) return false;                    // the panel path reports what is wrong; this form stays off
    }
    for (int rt = 0; rt < nrt; ++rt)
        for (int ks = 0; ks < jks; ++ks)
            for (int l = 0; l < 64; ++l) {
                const int row = 16 * rt + (l & 15), kk = 4 * ks + (l >> 4);
                int col = -1;                                        // column of d -> index of the unit-vector problem
                if (kk < n) col = kk;
                else if (kk < 2 * n) col = var2 ? kk : -1;           // VAR(1): x0_pre does not enter
                else if (kk >= 4 * FP_XKS && kk - 4 * FP_XKS < TN) col = 2 * n + (kk - 4 * FP_XKS);
                if (row < nrow && col >= 0) {
                    const double v = (at(1 + col, row) - nuc[row]) / scale;
                    if (!std::isfinite(v)) return false;
                    img[((size_t)rt * jksp + ks) * 64 + l] = v;
                }
            }
    // per stage: the rows of J_x as two 16-row A tiles (rows beyond n: zero) and nuc padded to 32 (d_z with the dual solve fused in)
    jst.assign((size_t)nb * 2 * FP_XKS * 64, 0.0); ncs.assign((size_t)nb * 32, 0.0);
    for (int st = 0; st < nb; ++st) {
        for (int r = 0; r < n; ++r) ncs[(size_t)st * 32 + r] = nuc[(size_t)st * n + r];
        for (int I = 0; I < 2; ++I)
            for (int ks = 0; ks < FP_XKS; ++ks)
                for (int l = 0; l < 64; ++l) {
                    const int rl = 16 * I + (l & 15), kk = 4 * ks + (l >> 4);
                    if (rl >= n) continue;
                    const int row = st * n + rl;
                    jst[(((size_t)st * 2 + I) * FP_XKS + ks) * 64 + l] = img[((size_t)(row >> 4) * jksp + ks) * 64 + ((kk & 3) << 4) + (row & 15)];
                }
    }
    // J' = [J_x | d nu+ / d (B u1) | d nu+ / d (B u2)]
    const int jksp2 = 16 * ((jks2 + 15) / 16 + 3);
    img2.assign((size_t)nrt * jksp2 * 64, 0.0);
    for (int rt = 0; rt < nrt; ++rt)
        for (int ks = 0; ks < jks2; ++ks)
            for (int l = 0; l < 64; ++l) {
                const int row = 16 * rt + (l & 15), kk = 4 * ks + (l >> 4);
                if (ks < FP_XKS) { img2[((size_t)rt * jksp2 + ks) * 64 + l] = img[((size_t)rt * jksp + ks) * 64 + l]; continue; }
                const int c = kk - 4 * FP_XKS;
                if (row < nrow && c < 2 * n) {
                    const double v = (at(1 + ncol + c, row) - nuc[row]) / scale;
                    if (!std::isfinite(v)) return false;
                    img2[((size_t)rt * jksp2 + ks) * 64 + l] = v;
                }
            }
    // E = [A1 A2 ; A2 0] (fast_mpc_eq_const.m:39-44), rows 0..53, columns [x0 ; x0_pre]
    eimg.assign((size_t)4 * FP_XKS * 64, 0.0);
    for (int I = 0; I < 4; ++I)
        for (int ks = 0; ks < FP_XKS; ++ks)
            for (int l = 0; l < 64; ++l) {
                const int row = 16 * I + (l & 15), kk = 4 * ks + (l >> 4);
                double v = 0.0;
                if (row < n && kk < n) v = a1[row * n + kk];
                else if (row < n && kk < 2 * n) v = var2 ? a2[row * n + kk - n] : 0.0;
                else if (row < 2 * n && kk < n) v = var2 ? a2[(row - n) * n + kk] : 0.0;
                eimg[((size_t)I * FP_XKS + ks) * 64 + l] = v;
            }
    // host copy for the first-move form: J with the columns [x0 | x0_pre | B u1 | B u2], nuc
    const int nc = 4 * n;
    J4.assign((size_t)nrow * nc, 0.0); nuc4.assign(nuc.begin(), nuc.begin() + nrow);
    for (int r = 0; r < nrow; ++r)
        for (int c = 0; c < nc; ++c) {
            int pidx = -1;
            if (c < n) pidx = 1 + c;
            else if (c < 2 * n) pidx = var2 ? 1 + c : -1;
            else pidx = 1 + ncol + (c - 2 * n);
            if (pidx >= 0) J4[(size_t)r * nc + c] = (at(pidx, r) - nuc[r]) / scale;
        }
    return true;
}

void fmpc_host_panel_layout(int n, int m, int T, int nb, int mp, FmpcPanelIn& L, size_t* o_dump, size_t* total, int* dz_len) {
    const FpVec V = fp_vec_layout(nb, T);
    size_t o = 0;
    L.o_simg = o; o += (size_t)nb * FP_IMG + 3 * FP_IMG;          // Linv per stage, then the prediction images
    L.limg_cap = 9 * nb + 2;                                        // Linv' per stage, a zero image, the edges
    L.o_limg = o; o += (size_t)L.limg_cap * FP_IMGL;
    L.o_bt = o;   o += (size_t)(mp / 16) * FP_KS * 64;
    L.o_aimg = o; o += 5 * FP_IMG;
    L.o_vec = o;  o += V.total;
    L.o_ucon = o; o += 4 * (size_t)mp;
    *dz_len = fd_lds_layout(mp).total_next;
    L.o_dz = o;   o += (size_t)*dz_len;
    L.pool_doubles = o;
    *o_dump = o;  o += (size_t)T * (n + m) + (size_t)nb * n;
    *total = o;
}

// Constants of the panel kernel for barrier weight k (fmpc_panel_layout.h): Y at the cold start is assembled from the
// de-duplicated blocks and G = B diag(wc) B', factored in long double by a block-sparse Cholesky in a twisted elimination
// order, and every operator the device needs becomes an MFMA A-operand image; a list scheduler turns the edges of the
// two sweeps into steps.  30 stages x 27^3: microseconds.
int fmpc_host_build_panel(const FmpcPanelIn& In, double k, FmpcPanelOut& Out) {
    typedef long double ld;
    const FmpcHostModel& hm = *In.M;
    const int n = hm.n, m = hm.m, T = hm.T, nb = hm.nb, mp = In.mp;
    const int nn = n * n;
    Out.valid = 0; Out.nsf = 0; Out.nsb = 0;
    std::vector<double>& pool = Out.pool;
    pool.assign(In.pool_doubles, 0.0);
    auto image = [&](const std::vector<ld>& M, double sign, double* out) {      // standard A-operand image of M (n x n row-major)
        for (int I = 0; I < 2; ++I)
            for (int ks = 0; ks < FP_KS; ++ks)
                for (int l = 0; l < 64; ++l) {
                    const int r = 16 * I + (l & 15), c = 4 * ks + (l >> 4);
                    out[(I * FP_KS + ks) * 64 + l] = (r < n && c < n) ? (double)(sign * M[r * n + c]) : 0.0;
                }
    };
    auto limage = [&](const std::vector<ld>& M, double sign, double* out) {     // the same, lane-major (FP_IMGL doubles)
        for (int I = 0; I < 2; ++I)
            for (int l = 0; l < 64; ++l)
                for (int ks = 0; ks < 8; ++ks) {
                    const int r = 16 * I + (l & 15), c = 4 * ks + (l >> 4);
                    out[(I * 64 + l) * 8 + ks] = (ks < FP_KS && r < n && c < n) ? (double)(sign * M[r * n + c]) : 0.0;
                }
    };
    // ---- u constants (needed for G = B diag(wc) B')
    double* uc = pool.data() + In.o_ucon;
    double sa_cu = 0.0;
    for (int j = 0; j < m; ++j) {
        const FmpcHostModel::Box b = hm.box(j, k);
        uc[j] = b.cu; uc[mp + j] = b.wc; uc[2 * mp + j] = b.hc; uc[3 * mp + j] = hm.umid[j];
        sa_cu += b.cu * b.cu;
    }
    const double* bt = hm.bt.data();                           // bt[c*n + r] = B[r][c]
    // ---- Y = C Phi^-1 C' at the cold start, block by block: Y_ii = const + G (i < T), Y_{i,i+1}, Y_{i,i+2}
    std::vector<ld> G(nn, 0.0L);
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) {
            ld t = 0.0L;
            for (int j = 0; j < m; ++j) t += (ld)bt[(size_t)j * n + a] * (ld)uc[mp + j] * (ld)bt[(size_t)j * n + b];
            G[a * n + b] = t;
        }
    // Elimination order ("twisted" factorisation): the stages 0 .. hs-1 top-down, then nb-1 .. hs+2 bottom-up, then
    // hs, hs+1.  The two chains are independent until the middle, which halves the serial length of both sweeps.
    const int hs = nb >= 8 ? nb / 2 - 1 : nb;
    std::vector<int> perm, rank(nb);
    for (int i = 0; i < (hs < nb ? hs : nb); ++i) perm.push_back(i);
    if (hs < nb) { for (int i = nb - 1; i >= hs + 2; --i) perm.push_back(i); perm.push_back(hs); perm.push_back(hs + 1); }
    for (int a = 0; a < nb; ++a) rank[perm[a]] = a;
    // P[a][b] (a <= b in elimination rank): the block Y[perm[a]][perm[b]]
    std::vector<std::vector<std::vector<ld>>> Pm(nb, std::vector<std::vector<ld>>(nb));
    auto yblock = [&](int i, int j, std::vector<ld>& out) -> bool {     // Y_ij (|i-j| <= 2), false if structurally zero
        out.assign(nn, 0.0L);
        const int lo = i < j ? i : j, d = i < j ? j - i : i - j;
        int id = -1;
        if (d == 0) id = hm.idxD[lo]; else if (d == 1) id = hm.idx1[lo]; else if (d == 2) id = hm.idx2[lo];
        if (d > 2 || id < 0) return false;
        const double* src = hm.blocks.data() + (size_t)id * nn;
        for (int r = 0; r < n; ++r) for (int c = 0; c < n; ++c) out[r * n + c] = i <= j ? (ld)src[r * n + c] : (ld)src[c * n + r];
        if (d == 0 && i < T) for (int q = 0; q < nn; ++q) out[q] += G[q];
        return true;
    };
    for (int a = 0; a < nb; ++a)
        for (int b = a; b < nb; ++b) {
            std::vector<ld> blk;
            if (yblock(perm[a], perm[b], blk)) Pm[a][b] = blk;
        }
    std::vector<std::vector<ld>> Linv(nb, std::vector<ld>(nn, 0.0L));        // by rank
    std::vector<std::vector<std::vector<ld>>> Um(nb, std::vector<std::vector<ld>>(nb));   // U[a][b] = L_a^-1 P[a][b], b > a
    for (int a = 0; a < nb; ++a) {
        // L = chol(P[a][a]) (lower), X = L^-1
        std::vector<ld> Lm(nn, 0.0L);
        const std::vector<ld>& S = Pm[a][a];
        for (int c = 0; c < n; ++c) {
            ld d = S[c * n + c];
            for (int q = 0; q < c; ++q) d -= Lm[c * n + q] * Lm[c * n + q];
            if (!(d > 0.0L)) return 0;                          // not PD at the start point: the exact path reports it
            const ld ldiag = sqrtl(d);
            Lm[c * n + c] = ldiag;
            for (int r = c + 1; r < n; ++r) {
                ld t = S[r * n + c];
                for (int q = 0; q < c; ++q) t -= Lm[r * n + q] * Lm[c * n + q];
                Lm[r * n + c] = t / ldiag;
            }
        }
        std::vector<ld>& X = Linv[a];
        for (int c = 0; c < n; ++c) {
            X[c * n + c] = 1.0L / Lm[c * n + c];
            for (int r = c + 1; r < n; ++r) {
                ld sacc = 0.0L;
                for (int q = c; q < r; ++q) sacc += Lm[r * n + q] * X[q * n + c];
                X[r * n + c] = -sacc / Lm[r * n + r];
            }
        }
        for (int b = a + 1; b < nb; ++b) {
            if (Pm[a][b].empty()) continue;
            std::vector<ld> u(nn);
            for (int r = 0; r < n; ++r) for (int c = 0; c < n; ++c) {
                ld t = 0.0L;
                for (int q = 0; q <= r; ++q) t += X[r * n + q] * Pm[a][b][q * n + c];
                u[r * n + c] = t;
            }
            Um[a][b] = u;
        }
        for (int b1 = a + 1; b1 < nb; ++b1) {
            if (Um[a][b1].empty()) continue;
            for (int b2 = b1; b2 < nb; ++b2) {
                if (Um[a][b2].empty()) continue;
                if (Pm[b1][b2].empty()) Pm[b1][b2].assign(nn, 0.0L);
                std::vector<ld>& dst = Pm[b1][b2];
                const std::vector<ld>& u1 = Um[a][b1]; const std::vector<ld>& u2 = Um[a][b2];
                for (int r = 0; r < n; ++r) for (int c = 0; c < n; ++c) {
                    ld t = 0.0L;
                    for (int q = 0; q < n; ++q) t += u1[q * n + r] * u2[q * n + c];
                    dst[r * n + c] -= t;
                }
            }
        }
    }
    // ---- images: Linv (standard, by stage), Linv' (lane-major id = stage), a zero image (id nb), one per edge
    std::vector<ld> M(nn);
    double* limg = pool.data() + In.o_limg;
    for (int i = 0; i < nb; ++i) {
        const std::vector<ld>& X = Linv[rank[i]];
        image(X, 1.0, pool.data() + In.o_simg + (size_t)i * FP_IMG);
        for (int r = 0; r < n; ++r) for (int c = 0; c < n; ++c) M[r * n + c] = X[c * n + r];
        limage(M, 1.0, limg + (size_t)i * FP_IMGL);
    }
    int nimg = nb + 1;                                            // id nb stays all zero
    struct Edge { int tgt, src, img; };
    std::vector<Edge> ef, eb;                                     // forward: y_tgt += img y_src ; backward: nu_tgt += img nu_src
    for (int a = 0; a < nb; ++a)
        for (int b = a + 1; b < nb; ++b) {
            if (Um[a][b].empty()) continue;
            if (nimg + 2 > In.limg_cap) return 0;        // cannot happen for the penta-diagonal structure
            const std::vector<ld>& u = Um[a][b];
            // forward: -Linv_b U_ab'          (target rank b, source rank a)
            const std::vector<ld>& Xb = Linv[b];
            for (int r = 0; r < n; ++r) for (int c = 0; c < n; ++c) {
                ld t = 0.0L;
                for (int q = 0; q <= r; ++q) t += Xb[r * n + q] * u[c * n + q];
                M[r * n + c] = t;
            }
            limage(M, -1.0, limg + (size_t)nimg * FP_IMGL);
            ef.push_back({perm[b], perm[a], nimg++});
            // backward: -Linv_a' U_ab         (target rank a, source rank b)
            const std::vector<ld>& Xa = Linv[a];
            for (int r = 0; r < n; ++r) for (int c = 0; c < n; ++c) {
                ld t = 0.0L;
                for (int q = r; q < n; ++q) t += Xa[q * n + r] * u[q * n + c];
                M[r * n + c] = t;
            }
            limage(M, -1.0, limg + (size_t)nimg * FP_IMGL);
            eb.push_back({perm[a], perm[b], nimg++});
        }
    // ---- schedules: list scheduling of the edges, <= 4 targets per step (one wave pair each), one edge per target and step
    std::vector<int>& sched = Out.sched;
    sched.assign((size_t)2 * FP_MAX_STEPS(nb) * FP_STEP_INTS, -1);
    auto schedule = [&](const std::vector<Edge>& E, int* out) -> int {
        const int ne = (int)E.size();
        std::vector<int> done_step(nb, -1), pending(nb, 0), estep(ne, -1);
        for (const Edge& e : E) pending[e.tgt]++;
        for (int i = 0; i < nb; ++i) if (pending[i] == 0) done_step[i] = 0;       // final before the sweep starts
        int left = ne, step = 0;
        while (left > 0) {
            ++step;
            if (step > FP_MAX_STEPS(nb)) return -1;
            int groups = 0; int gt[4];
            int* row = out + (size_t)(step - 1) * FP_STEP_INTS;
            std::vector<int> newly;
            for (int e = 0; e < ne && true; ++e) {
                if (estep[e] >= 0) continue;
                const int sd = done_step[E[e].src];
                if (sd < 0 || sd >= step) continue;                   // source not final before this step
                bool taken = false;                                   // one edge per target and step
                for (int q = 0; q < groups; ++q) if (gt[q] == E[e].tgt) taken = true;
                if (taken || groups == 4) continue;
                const int gi = groups; gt[groups++] = E[e].tgt;
                for (int I = 0; I < 2; ++I) {
                    int* ent = row + (2 * gi + I) * 3;
                    ent[0] = E[e].tgt; ent[1] = E[e].src; ent[2] = E[e].img;
                }
                estep[e] = step; --left;
                if (--pending[E[e].tgt] == 0) newly.push_back(E[e].tgt);
            }
            for (int t : newly) done_step[t] = step;
        }
        return step;
    };
    Out.nsf = schedule(ef, sched.data());
    Out.nsb = schedule(eb, sched.data() + (size_t)FP_MAX_STEPS(nb) * FP_STEP_INTS);
    if (Out.nsf < 0 || Out.nsb < 0) return 0;
    if (getenv("FMPC_PANEL_VERBOSE")) fprintf(stderr, "fastmpc panel: nb %d, split %d, %d images, %d forward / %d backward edges, %d / %d steps\n", nb, hs, nimg, (int)ef.size(), (int)eb.size(), Out.nsf, Out.nsb);
    // ---- the prediction terms of stages 0 and 1 folded into product images: -Linv_0 A1, -Linv_0 A2, -Linv_1 A2
    {
        double* dst = pool.data() + In.o_simg + (size_t)nb * FP_IMG;
        auto prod = [&](const std::vector<ld>& X, const double* A) {
            for (int r = 0; r < n; ++r) for (int c = 0; c < n; ++c) {
                ld a = 0.0L;
                for (int q = 0; q <= r; ++q) a += X[r * n + q] * (ld)A[q * n + c];
                M[r * n + c] = a;
            }
        };
        prod(Linv[rank[0]], hm.a1.data()); image(M, -1.0, dst);
        prod(Linv[rank[0]], hm.a2.data()); image(M, -1.0, dst + FP_IMG);
        if (nb > 1) { prod(Linv[rank[1]], hm.a2.data()); image(M, -1.0, dst + 2 * FP_IMG); }
    }
    // ---- model images
    {
        double* dst = pool.data() + In.o_bt;
        for (int J = 0; J < mp / 16; ++J)
            for (int ks = 0; ks < FP_KS; ++ks)
                for (int l = 0; l < 64; ++l) {
                    const int c = 16 * J + (l & 15), q = 4 * ks + (l >> 4);
                    dst[(J * FP_KS + ks) * 64 + l] = (c < m && q < n) ? bt[(size_t)c * n + q] : 0.0;
                }
        double* a = pool.data() + In.o_aimg;
        std::vector<ld> A(nn);
        for (int i = 0; i < nn; ++i) A[i] = hm.a1[i];
        image(A, 1.0, a + FP_AIMG_A1 * FP_IMG);
        for (int r = 0; r < n; ++r) for (int c = 0; c < n; ++c) M[r * n + c] = A[c * n + r];
        image(M, 1.0, a + FP_AIMG_A1T * FP_IMG);
        for (int i = 0; i < nn; ++i) A[i] = hm.a2[i];
        image(A, 1.0, a + FP_AIMG_A2 * FP_IMG);
        for (int r = 0; r < n; ++r) for (int c = 0; c < n; ++c) M[r * n + c] = A[c * n + r];
        image(M, 1.0, a + FP_AIMG_A2T * FP_IMG);
        for (int r = 0; r < n; ++r) for (int c = 0; c < n; ++c) {
            ld t = 0.0L;
            for (int j = 0; j < m; ++j) t += (ld)bt[(size_t)j * n + r] * (ld)bt[(size_t)j * n + c];
            M[r * n + c] = t;
        }
        image(M, 1.0, a + FP_AIMG_BBT * FP_IMG);
    }
    // ---- vectors
    const FpVec V = fp_vec_layout(nb, T);
    double* vec = pool.data() + In.o_vec;
    std::vector<double> cbu(n), bu(n), a1x(n), a2x(n);
    for (int a = 0; a < n; ++a) {
        double t0 = 0.0, t1 = 0.0, t2 = 0.0;
        for (int j = 0; j < m; ++j) {
            t0 += bt[(size_t)j * n + a] * uc[mp + j] * uc[j];
            t1 += bt[(size_t)j * n + a] * hm.umid[j];
            t2 += bt[(size_t)j * n + a] * uc[j];
        }
        cbu[a] = t0; bu[a] = t1; vec[V.bcu + a] = t2;
        double s1 = 0.0, s2 = 0.0;
        for (int q = 0; q < n; ++q) { s1 += hm.a1[a * n + q] * hm.xmid[q]; s2 += hm.a2[a * n + q] * hm.xmid[q]; }
        a1x[a] = s1; a2x[a] = s2;
    }
    std::vector<double> phx((size_t)T * n);
    double rd2_0 = T * sa_cu;
    for (int j = 0; j < T; ++j)
        for (int r = 0; r < n; ++r) {
            const bool last = j + 1 == T;
            const double q2 = last ? hm.Qf2[r] : hm.Q2[r];
            const double d0 = q2 * hm.xmid[r] + (last ? hm.qfl[r] : hm.ql[r]);
            vec[V.dx0 + j * 32 + r] = d0;
            vec[V.iq + j * 32 + r] = 1.0 / q2;
            phx[(size_t)j * n + r] = d0 / q2;
            vec[V.xc + j * 32 + r] = hm.xmid[r] - d0 / q2;
            rd2_0 += d0 * d0;
        }
    const bool var2 = hm.var2 != 0;
    for (int i = 0; i < nb; ++i)
        for (int r = 0; r < n; ++r) {
            double cp, c0;
            if (i < T) {
                cp = hm.xmid[r] - bu[r] - (i >= 1 ? a1x[r] : 0.0) - (i >= 2 ? a2x[r] : 0.0);
                c0 = phx[(size_t)i * n + r] - cbu[r];
                if (i >= 1) for (int q = 0; q < n; ++q) c0 -= hm.a1[r * n + q] * phx[(size_t)(i - 1) * n + q];
                if (i >= 2 && var2) for (int q = 0; q < n; ++q) c0 -= hm.a2[r * n + q] * phx[(size_t)(i - 2) * n + q];
            } else {
                cp = hm.xmid[r] - hm.xf[r];
                c0 = phx[(size_t)(T - 1) * n + r];
            }
            vec[V.cp + i * 32 + r] = cp;
            vec[V.ct + i * 32 + r] = cp - c0;
        }
    // rt_i = Linv_i ct_i and the w-free part of ||r_p||^2
    double rp2c = 0.0;
    for (int i = 0; i < nb; ++i)
        for (int r = 0; r < n; ++r) {
            ld a = 0.0L;
            for (int q = 0; q <= r; ++q) a += Linv[rank[i]][r * n + q] * (ld)vec[V.ct + i * 32 + q];
            vec[V.rt + i * 32 + r] = (double)a;
            if (i >= 2) rp2c += vec[V.cp + i * 32 + r] * vec[V.cp + i * 32 + r];
        }
    Out.rp2c = rp2c;
    Out.rd2_0 = rd2_0;
    {   // LDS image of the d_z kernel, in LDS order
        const FdLds D = fd_lds_layout(mp);
        double* dz = pool.data() + In.o_dz;
        memcpy(dz + D.BT, pool.data() + In.o_bt, (size_t)(mp / 16) * FP_KS * 64 * sizeof(double));
        memcpy(dz + D.A1T, pool.data() + In.o_aimg + FP_AIMG_A1T * FP_IMG, FP_IMG * sizeof(double));
        memcpy(dz + D.A2T, pool.data() + In.o_aimg + FP_AIMG_A2T * FP_IMG, FP_IMG * sizeof(double));
        for (int j = 0; j < mp; ++j) {
            dz[D.UC + j] = -uc[mp + j] * uc[j];
            dz[D.UC + mp + j] = uc[mp + j]; dz[D.UC + 2 * mp + j] = uc[2 * mp + j]; dz[D.UC + 3 * mp + j] = uc[3 * mp + j];
        }
        for (int j = 0; j < mp; ++j) {                               // [c2 | 2R | hp | hm] for the next-exit-test variant
            const bool in = j < m;
            dz[D.UX + j] = in ? hm.R2[j] * hm.umid[j] + hm.rl[j] : 0.0;
            dz[D.UX + mp + j] = in ? hm.R2[j] : 0.0;
            dz[D.UX + 2 * mp + j] = in ? hm.umax[j] - hm.umid[j] : 1.0;
            dz[D.UX + 3 * mp + j] = in ? hm.umid[j] - hm.umin[j] : 1.0;
        }
        for (int r = 0; r < 32; ++r) {
            dz[D.XQ + r] = vec[V.xc + r]; dz[D.XQ + 32 + r] = vec[V.xc + (T - 1) * 32 + r];
            dz[D.XQ + 64 + r] = vec[V.iq + r]; dz[D.XQ + 96 + r] = vec[V.iq + (T - 1) * 32 + r];
        }
    }
    Out.valid = 1;
    Out.nimg = nimg;
    return 0;
}


void fmpc_host_build_first_move(const FmpcFirstIn& In, FmpcFirstOut& Out) {
    typedef long double ld;
    const FmpcHostModel& hm = *In.M;
    const int n = hm.n, m = hm.m, T = hm.T, nb = hm.nb, nc = 4 * n;
    const bool var2 = hm.var2 != 0;
    const double* xf = hm.xf_or_xmid();
    Out.nc = nc;
    std::vector<double> cu(m), wc(m), av(m);
    for (int j = 0; j < m; ++j) { const FmpcHostModel::Box b = hm.box(j, In.k); cu[j] = b.cu; wc[j] = b.wc; av[j] = b.hc * b.wc; }
    const double* bt = hm.bt.data();                                     // bt[c*n + r] = B[r][c]
    // ---- u0 = u0c + K0 d
    Out.K0t.assign((size_t)nc * m, 0.0); Out.u0c.assign(m, 0.0);
    for (int j = 0; j < m; ++j) {
        ld t = 0.0L;
        for (int r = 0; r < n; ++r) t += (ld)bt[(size_t)j * n + r] * (ld)In.nuc[r];
        Out.u0c[j] = (double)((ld)hm.umid[j] + (ld)wc[j] * (t - (ld)cu[j]));
        for (int c = 0; c < nc; ++c) {
            ld s = 0.0L;
            for (int r = 0; r < n; ++r) s += (ld)bt[(size_t)j * n + r] * (ld)In.J[(size_t)r * nc + c];
            Out.K0t[(size_t)c * m + j] = (double)((ld)wc[j] * s);
        }
    }
    // ---- ||e||^2 = d'E d + 2 e'd + e0 :  per stage s, g_s = a o (B' nuc_s - cu), G_s = diag(a) B' J_s
    //      E = sum J_s' Ma2 J_s, e = sum J_s' B (a o g_s), e0 = sum |g_s|^2,  Ma2 = B diag(a^2) B'
    std::vector<ld> Ma2((size_t)n * n, 0.0L);
    for (int r = 0; r < n; ++r)
        for (int q = 0; q < n; ++q) {
            ld t = 0.0L;
            for (int j = 0; j < m; ++j) t += (ld)bt[(size_t)j * n + r] * (ld)av[j] * (ld)av[j] * (ld)bt[(size_t)j * n + q];
            Ma2[(size_t)r * n + q] = t;
        }
    std::vector<ld> E((size_t)nc * nc, 0.0L), e(nc, 0.0L), tmp((size_t)n * nc), bg(n), g(m);
    ld e0 = 0.0L;
    for (int s = 0; s < T; ++s) {
        const double* Js = In.J + (size_t)s * n * nc;
        const double* ncs = In.nuc + (size_t)s * n;
        for (int j = 0; j < m; ++j) {
            ld t = 0.0L;
            for (int r = 0; r < n; ++r) t += (ld)bt[(size_t)j * n + r] * (ld)ncs[r];
            g[j] = (ld)av[j] * (t - (ld)cu[j]);
            e0 += g[j] * g[j];
        }
        for (int r = 0; r < n; ++r) {
            ld t = 0.0L;
            for (int j = 0; j < m; ++j) t += (ld)bt[(size_t)j * n + r] * (ld)av[j] * g[j];
            bg[r] = t;
        }
        for (int r = 0; r < n; ++r)
            for (int c = 0; c < nc; ++c) {
                ld t = 0.0L;
                for (int q = 0; q < n; ++q) t += Ma2[(size_t)r * n + q] * (ld)Js[(size_t)q * nc + c];
                tmp[(size_t)r * nc + c] = t;
            }
        for (int c1 = 0; c1 < nc; ++c1) {
            ld t = 0.0L;
            for (int r = 0; r < n; ++r) t += (ld)Js[(size_t)r * nc + c1] * bg[r];
            e[c1] += t;
            for (int c2 = 0; c2 < nc; ++c2) {
                ld u = 0.0L;
                for (int r = 0; r < n; ++r) u += (ld)Js[(size_t)r * nc + c1] * tmp[(size_t)r * nc + c2];
                E[(size_t)c1 * nc + c2] += u;
            }
        }
    }
    // ---- ||r_p||^2 = |cp - Pb d|^2:  rows of stage 0 [A1 | A2 | -M1_0 | -M2_0], stage 1 [A2 | 0 | -M1_1 | -M2_1], i >= 2 [0 | 0 | -M1_i | -M2_i]
    std::vector<ld> Ep((size_t)nc * nc, 0.0L), ep(nc, 0.0L), row(nc);
    ld ep0 = 0.0L;
    std::vector<ld> bu(n, 0.0L), a1x(n, 0.0L), a2x(n, 0.0L);
    for (int r = 0; r < n; ++r) {
        for (int j = 0; j < m; ++j) bu[r] += (ld)bt[(size_t)j * n + r] * (ld)hm.umid[j];
        for (int q = 0; q < n; ++q) { a1x[r] += (ld)hm.a1[r * n + q] * (ld)hm.xmid[q]; a2x[r] += (ld)hm.a2[r * n + q] * (ld)hm.xmid[q]; }
    }
    for (int i = 0; i < nb; ++i)
        for (int r = 0; r < n; ++r) {
            ld cp;
            for (int c = 0; c < nc; ++c) row[c] = 0.0L;
            if (i < T) {
                cp = (ld)hm.xmid[r] - bu[r] - (i >= 1 ? a1x[r] : 0.0L) - (i >= 2 ? a2x[r] : 0.0L);
                if (i == 0) for (int q = 0; q < n; ++q) { row[q] = hm.a1[r * n + q]; row[n + q] = var2 ? (ld)hm.a2[r * n + q] : 0.0L; }
                if (i == 1 && var2) for (int q = 0; q < n; ++q) row[q] = hm.a2[r * n + q];
                for (int q = 0; q < n; ++q) {
                    row[2 * n + q] = -(ld)hm.m1[((size_t)i * n + r) * n + q];
                    row[3 * n + q] = -(ld)hm.m2[((size_t)i * n + r) * n + q];
                }
            } else {
                cp = (ld)hm.xmid[r] - (ld)xf[r];
            }
            ep0 += cp * cp;
            for (int c1 = 0; c1 < nc; ++c1) {
                if (row[c1] == 0.0L) continue;
                ep[c1] += row[c1] * cp;
                for (int c2 = 0; c2 < nc; ++c2) Ep[(size_t)c1 * nc + c2] += row[c1] * row[c2];
            }
        }
    auto fro = [](const std::vector<ld>& v) { ld s = 0.0L; for (ld x : v) s += x * x; return (double)sqrtl(s); };
    Out.E.resize(E.size()); Out.Ep.resize(Ep.size()); Out.e.resize(nc); Out.ep.resize(nc);
    for (size_t i = 0; i < E.size(); ++i) { Out.E[i] = (double)E[i]; Out.Ep[i] = (double)Ep[i]; }   // symmetric: [c][r] == [r][c]
    for (int c = 0; c < nc; ++c) { Out.e[c] = (double)e[c]; Out.ep[c] = (double)ep[c]; }
    Out.e0 = (double)e0; Out.ep0 = (double)ep0;
    // circulant halves for the kernel: d'E d = sum_r d_r sum_{j=0}^{nc/2} Ec[j][r] d[(r + j) mod nc]  (every unordered pair once;
    // the pairs at distance nc/2 would come twice: kept for r < nc/2)
    const int H = nc / 2 + 1;
    Out.Ec.assign((size_t)H * nc, 0.0); Out.Epc.assign((size_t)H * nc, 0.0);
    for (int j = 0; j < H; ++j)
        for (int r = 0; r < nc; ++r) {
            const int c = (r + j) % nc;
            const ld wgt = j == 0 ? 1.0L : ((j == nc / 2 && r >= nc / 2) ? 0.0L : 2.0L);
            const ld se = (E[(size_t)r * nc + c] + E[(size_t)c * nc + r]) * 0.5L, sp = (Ep[(size_t)r * nc + c] + Ep[(size_t)c * nc + r]) * 0.5L;
            Out.Ec[(size_t)j * nc + r] = (double)(wgt * se);
            Out.Epc[(size_t)j * nc + r] = (double)(wgt * sp);
        }
    Out.normE = fro(E); Out.norme = fro(e); Out.normEp = fro(Ep); Out.normep = fro(ep);
}

void fmpc_host_mfma_images(const double* M, int rows, int cols, int ks, std::vector<double>& img) {
    const int tiles = (rows + 15) / 16;
    img.assign((size_t)tiles * ks * 64, 0.0);
    for (int t = 0; t < tiles; ++t)
        for (int q = 0; q < ks; ++q)
            for (int g = 0; g < 4; ++g)
                for (int r = 0; r < 16; ++r) {
                    const int row = 16 * t + r, col = 4 * q + g;
                    if (row < rows && col < cols) img[((size_t)t * ks + q) * 64 + g * 16 + r] = M[(size_t)row * cols + col];
                }
}

void fmpc_host_build_loop_images(const FmpcFirstOut& O, int n, int m, int ks, bool fused, const double* bt, FmpcLoopImages& out) {
    const int nc = 4 * n, kc = 4 * ks, cst = fused ? kc - 1 : nc;
    auto col = [&](int c) { return fused ? ks * (c / n) + c % n : c; };          // column of d -> column of the images
    std::vector<double> U((size_t)m * kc, 0.0), E2((size_t)kc * kc, 0.0), Ep2((size_t)kc * kc, 0.0);
    for (int j = 0; j < m; ++j) {
        for (int c = 0; c < nc; ++c) U[(size_t)j * kc + col(c)] = O.K0t[(size_t)c * m + j];
        U[(size_t)j * kc + cst] = O.u0c[j];
    }
    for (int r = 0; r < nc; ++r) {
        const int rr = col(r);
        for (int c = 0; c < nc; ++c) {
            const int cc = col(c);
            const double wgt = cc / 16 > rr / 16 ? 2.0 : (cc / 16 == rr / 16 ? 1.0 : 0.0);
            E2[(size_t)rr * kc + cc] = wgt * O.E[(size_t)r * nc + c];
            Ep2[(size_t)rr * kc + cc] = wgt * O.Ep[(size_t)r * nc + c];
        }
        E2[(size_t)rr * kc + cst] = 2.0 * O.e[r];
        Ep2[(size_t)rr * kc + cst] = -2.0 * O.ep[r];
    }
    fmpc_host_mfma_images(U.data(), m, kc, ks, out.imgU);
    fmpc_host_mfma_images(E2.data(), kc, kc, ks, out.imgE);
    fmpc_host_mfma_images(Ep2.data(), kc, kc, ks, out.imgEp);
    out.imgB.clear();
    if (fused && bt) {
        std::vector<double> Brm((size_t)n * m);
        for (int q = 0; q < n; ++q)
            for (int c = 0; c < m; ++c) Brm[(size_t)q * m + c] = bt[(size_t)c * n + q];
        fmpc_host_mfma_images(Brm.data(), n, m, (m + 3) / 4, out.imgB);
    }
}

void fmpc_host_mfma_a_images(const double* M, int rows, std::vector<double>& img) {
    const int tiles = (rows + 15) / 16;
    img.assign((size_t)tiles * FA_KS * 64, 0.0);
    for (int t = 0; t < tiles; ++t)
        for (int q = 0; q < FA_KS; ++q)
            for (int g = 0; g < 4; ++g)
                for (int r = 0; r < 16; ++r) {
                    const int row = 16 * t + r;
                    if (row < rows) img[((size_t)t * FA_KS + q) * 64 + g * 16 + r] = M[(size_t)row * FA_KC + 4 * q + g];
                }
}

// z+ = zc + Kz d, d = [x0 ; x0_pre], from nu+ = nuc + J d (rows of stage s: u_s, then x_{s+1}):
//   u_s+   = umid + wc o (B' nu+_s - cu)                                            (inf_newton_solver.m:34-35 on the u entries)
//   x_j+   = xmid + X_j (-(2 Q_j xmid + q_j) - nu+_{j-1} + A1' nu+_j + A2' nu+_{j+1} [- nu+_T])   j = 1..T, X_j = (2 Q_j)^-1
void fmpc_host_build_affine(const FmpcAffineIn& In, FmpcAffineOut& Out) {
    typedef long double ld;
    const FmpcHostModel& hm = *In.M;
    const int n = hm.n, m = hm.m, T = hm.T, s = n + m, nd = 2 * n, ncJ = In.ncJ;
    Out.rows = T * s; Out.tiles = (Out.rows + 15) / 16;
    Out.Kz.assign((size_t)Out.rows * FA_KC, 0.0);
    std::vector<ld> cu(m), wc(m);
    for (int j = 0; j < m; ++j) {
        const ld sp = (ld)hm.umax[j] - (ld)hm.umid[j], sm = (ld)hm.umid[j] - (ld)hm.umin[j];
        const ld dp = 1.0L / sp, dm = 1.0L / sm;
        cu[j] = (ld)hm.R2[j] * (ld)hm.umid[j] + (ld)hm.rl[j] + (ld)In.k * (dp - dm);
        wc[j] = 1.0L / ((ld)hm.R2[j] + (ld)In.k * (dp * dp + dm * dm));
    }
    // nu+ as an affine function of d: column c < nd of J, column nd = nuc
    auto nuv = [&](int blk, int r, int c) -> ld {
        return c < nd ? (ld)In.J[((size_t)blk * n + r) * ncJ + c] : (ld)In.nuc[(size_t)blk * n + r];
    };
    for (int st = 0; st < T; ++st) {
        for (int j = 0; j < m; ++j) {
            double* row = &Out.Kz[((size_t)st * s + j) * FA_KC];
            for (int c = 0; c <= nd; ++c) {
                ld t = 0.0L;
                for (int r = 0; r < n; ++r) t += (ld)hm.bt[(size_t)j * n + r] * nuv(st, r, c);
                if (c == nd) t = (ld)hm.umid[j] + wc[j] * (t - cu[j]); else t *= wc[j];
                row[c] = (double)t;
            }
        }
        const int jx = st + 1;                                     // x_jx lives in stage st
        const bool last = jx == T;
        for (int r = 0; r < n; ++r) {
            double* row = &Out.Kz[((size_t)st * s + m + r) * FA_KC];
            const ld q2 = last ? (ld)hm.Qf2[r] : (ld)hm.Q2[r], ql = last ? (ld)hm.qfl[r] : (ld)hm.ql[r];
            for (int c = 0; c <= nd; ++c) {
                ld v = -nuv(jx - 1, r, c);
                if (jx < T) for (int q = 0; q < n; ++q) v += (ld)hm.a1[q * n + r] * nuv(jx, q, c);
                if (jx + 1 < T) for (int q = 0; q < n; ++q) v += (ld)hm.a2[q * n + r] * nuv(jx + 1, q, c);
                if (last && hm.has_xf) v -= nuv(T, r, c);
                if (c == nd) v = (ld)hm.xmid[r] + (v - (q2 * (ld)hm.xmid[r] + ql)) / q2; else v /= q2;
                row[c] = (double)v;
            }
        }
    }
    fmpc_host_mfma_a_images(Out.Kz.data(), Out.rows, Out.img);
    // nu+ = nuc + J d as further rows (requested by callers that want the multipliers)
    Out.nu_rows = hm.nb * n; Out.nu_tiles = (Out.nu_rows + 15) / 16;
    std::vector<double> Jn((size_t)Out.nu_rows * FA_KC, 0.0), imgn;
    for (int r = 0; r < Out.nu_rows; ++r) {
        for (int c = 0; c < nd; ++c) Jn[(size_t)r * FA_KC + c] = In.J[(size_t)r * ncJ + c];
        Jn[(size_t)r * FA_KC + nd] = In.nuc[r];
    }
    fmpc_host_mfma_a_images(Jn.data(), Out.nu_rows, imgn);
    Out.img.insert(Out.img.end(), imgn.begin(), imgn.end());
    // ---- the u rows through nu+ (fmpc_kernel_affine_nu.hip): u_st = G [nu+_st ; 1], nu+_st = [J_st | nuc_st] d
    // per stage 1 .. T-1 the 32 rows [J_st | nuc_st] (27), the unit row on the constant column of d (entry 27 of the result is 1.0
    // exactly), four zero rows
    Out.jbase = Out.tiles + Out.nu_tiles;
    fmpc_host_plan_nu(m, n, T, Out.plan);
    if (n != 27) { Out.imgG.clear(); return; }                     // (n + 1 = 28 = 4 FA_NU_KS: the only size the kernel is built for)
    std::vector<double> Jp((size_t)32 * FA_KC);
    for (int st = 1; st < T; ++st) {
        std::fill(Jp.begin(), Jp.end(), 0.0);
        for (int r = 0; r < n; ++r) {
            for (int c = 0; c < nd; ++c) Jp[(size_t)r * FA_KC + c] = In.J[((size_t)st * n + r) * ncJ + c];
            Jp[(size_t)r * FA_KC + nd] = In.nuc[(size_t)st * n + r];
        }
        Jp[(size_t)n * FA_KC + nd] = 1.0;
        fmpc_host_mfma_a_images(Jp.data(), 32, imgn);
        Out.img.insert(Out.img.end(), imgn.begin(), imgn.end());
    }
    // per u tile [diag(wc) B' | umid - wc o cu] of its 16 rows: each entry rounded to double once
    int nut = 0;
    for (int st = 0; st < T; ++st) nut += Out.plan[st].nu;
    Out.imgG.assign((size_t)nut * FA_NU_KS * 64, 0.0);
    for (int st = 1; st < T; ++st)
        for (int u = 0; u < Out.plan[st].nu; ++u) {
            double* im = &Out.imgG[(size_t)(Out.plan[st].ub + u) * FA_NU_KS * 64];
            for (int r = 0; r < 16; ++r) {
                const int j = 16 * (Out.plan[st].tb + u) + r - st * s;                  // actuator of the row
                for (int c = 0; c <= n; ++c) {
                    const ld v = c < n ? wc[j] * (ld)hm.bt[(size_t)j * n + c] : (ld)hm.umid[j] - wc[j] * cu[j];
                    im[(size_t)(c >> 2) * 64 + (c & 3) * 16 + r] = (double)v;
                }
            }
        }
}

void fmpc_host_plan_nu(int m, int n, int T, std::vector<FmpcNuStage>& plan) {
    const int s = n + m, tiles = (T * s + 15) / 16;
    plan.assign(T > 0 ? T : 0, FmpcNuStage{0, 0, 0, 0});
    int ub = 0;
    for (int j = 0; j < T; ++j) {
        const int tb = (s * j + 15) / 16;                            // first tile whose first row lies in stage j
        int te = (s * (j + 1) + 15) / 16;
        if (te > tiles) te = tiles;
        int nu = j >= 1 ? (s * j + m) / 16 - tb : 0;                  // tiles with 16 (t + 1) <= s j + m: a prefix of the item's
        if (nu < 0) nu = 0;
        if (nu > te - tb) nu = te - tb;
        plan[j] = FmpcNuStage{tb, nu, te - tb - nu, ub};
        ub += nu;
    }
}

int fmpc_host_nu_work(const std::vector<FmpcNuStage>& plan) {
    int work = 0;
    for (const FmpcNuStage& S : plan) work += 7 * S.nu + 14 * S.nd;
    return work;
}

int fmpc_host_nu_parts(int T, int work, int W) {
    if (T < 1 || W < 1) return 1;
    int bestP = 1; double best = -1.0;
    for (int P = 1; P <= 8; ++P) {
        const double cost = (double)((T * P + W - 1) / W) * (28.0 + (double)work / ((double)T * P));
        if (best < 0.0 || cost < best) { best = cost; bestP = P; }
    }
    return bestP;
}

int fmpc_host_nu_swap(int T, int parts, int W) {
    return parts == 1 && W >= 1 && T > W - 1 && T % W != 0 ? W - 1 : 0;
}

// debug exports (tests/test_host_affine_nu.py): the tile plan; the affine builder on caller-supplied model arrays
extern "C" int fmpc_debug_plan_nu(int m, int n, int T, int W, int* plan4, int* parts, int* swap) {
    if (m < 1 || n < 1 || T < 1 || !plan4) return -1;
    std::vector<FmpcNuStage> plan;
    fmpc_host_plan_nu(m, n, T, plan);
    for (int j = 0; j < T; ++j) { plan4[4 * j] = plan[j].tb; plan4[4 * j + 1] = plan[j].nu; plan4[4 * j + 2] = plan[j].nd; plan4[4 * j + 3] = plan[j].ub; }
    const int np = fmpc_host_nu_parts(T, fmpc_host_nu_work(plan), W);
    if (parts) *parts = np;
    if (swap) *swap = fmpc_host_nu_swap(T, np, W);
    return 0;
}
// the tiles [*b, *e) of cnt that part p of `parts` takes (FMPC_NU_CUT, as the kernel applies it)
extern "C" int fmpc_debug_nu_cut(int cnt, int p, int parts, int* b, int* e) {
    if (cnt < 0 || parts < 1 || p < 0 || p >= parts || !b || !e) return -1;
    *b = FMPC_NU_CUT(cnt, p, parts); *e = FMPC_NU_CUT(cnt, p + 1, parts);
    return 0;
}
// arr: bt, umax, umin, umid, xmid, R2, rl, Q2, Qf2, ql, qfl, a1, a2, J (nb n x 2 n), nuc.  Out: Kz [rows][FA_KC], the J images
// [2 (T - 1)][FA_KS][64], the u-tile images [u tiles][FA_NU_KS][64] (any of them may be NULL).  Returns the u tiles, < 0 on bad arguments.
extern "C" int fmpc_debug_build_affine_nu(int n, int m, int T, int nb, int has_xf, double k, const double* const* arr, double* Kz, double* imgJ, double* imgG) {
    if (n != 27 || m < 1 || T < 1 || nb < T || !arr) return -1;
    FmpcHostModel M;
    M.n = n; M.m = m; M.T = T; M.nb = nb; M.has_xf = has_xf;
    auto vec = [&](int i, int cnt) { return std::vector<double>(arr[i], arr[i] + cnt); };
    M.bt = vec(0, m * n); M.umax = vec(1, m); M.umin = vec(2, m); M.umid = vec(3, m); M.xmid = vec(4, n); M.R2 = vec(5, m); M.rl = vec(6, m);
    M.Q2 = vec(7, n); M.Qf2 = vec(8, n); M.ql = vec(9, n); M.qfl = vec(10, n); M.a1 = vec(11, n * n); M.a2 = vec(12, n * n);
    FmpcAffineIn In;
    In.M = &M; In.ncJ = 2 * n; In.k = k; In.J = arr[13]; In.nuc = arr[14];
    FmpcAffineOut Out;
    fmpc_host_build_affine(In, Out);
    if (Kz) std::copy(Out.Kz.begin(), Out.Kz.end(), Kz);
    if (imgJ) std::copy(Out.img.begin() + (size_t)Out.jbase * FA_KS * 64, Out.img.end(), imgJ);
    if (imgG) std::copy(Out.imgG.begin(), Out.imgG.end(), imgG);
    return (int)(Out.imgG.size() / (FA_NU_KS * 64));
}

// ---- cold-start step with the ramp-rate rows: constants of the Woodbury form (fmpc_host.h)
void fmpc_host_build_ramp_cold(const FmpcRampColdIn& In, FmpcRampColdOut& Out) {
    typedef long double ld;
    const FmpcHostModel& hm = *In.M;
    const int n = hm.n, m = hm.m, T = hm.T, nb = hm.nb, s = n + m, Nz = T * s, nbn = nb * n;
    const bool var2 = hm.var2 != 0, has_xf = hm.has_xf != 0;
    Out.valid = 0;
    // ---- per actuator: box and ramp terms at the start point, the tridiagonal and its inverse
    std::vector<ld> hb(m), gb(m), erb(m), grb(m);
    for (int c = 0; c < m; ++c) {
        const ld dp = 1.0L / ((ld)hm.umax[c] - (ld)hm.umid[c]), dm = 1.0L / ((ld)hm.umid[c] - (ld)hm.umin[c]);
        hb[c] = (ld)In.k * (dp * dp + dm * dm); gb[c] = (ld)In.k * (dp - dm);
        const ld rp = 1.0L / (ld)In.dumax[c], rm = 1.0L / (-(ld)In.dumin[c]);       // slacks of u_j - u_{j-1} = 0
        erb[c] = (ld)In.k * (rp * rp + rm * rm); grb[c] = (ld)In.k * (rp - rm);
    }
    Out.g0.assign((size_t)T * m, 0.0); Out.Gf.assign((size_t)T * T * m, 0.0); Out.hd.assign((size_t)T * m, 0.0);
    Out.erb.resize(m);
    std::vector<ld> Gl((size_t)T * T * m);                        // Gf in long double, same layout
    std::vector<ld> dg(T), lo(T);
    for (int c = 0; c < m; ++c) {
        Out.erb[c] = (double)erb[c];
        // diag_j = 2R + hb + [j >= 1] erb + [j + 1 < T] erb ; off_{j,j+1} = -erb    (stage 0's own ramp term is the per-problem delta)
        for (int j = 0; j < T; ++j) {
            const ld hdj = hb[c] + (j >= 1 ? erb[c] : 0.0L) + (j + 1 < T ? erb[c] : 0.0L);
            Out.hd[(size_t)j * m + c] = (double)hdj;
            ld d = (ld)hm.R2[c] + hdj;
            if (j > 0) d -= lo[j - 1] * lo[j - 1] * dg[j - 1];
            if (!(d > 0.0L) || !std::isfinite((double)d)) return;
            dg[j] = d;
            lo[j] = j + 1 < T ? -erb[c] / d : 0.0L;
        }
        // inverse of L D L' (L unit lower bidiagonal with sub-diagonal lo): column by column
        for (int col = 0; col < T; ++col) {
            std::vector<ld> x(T, 0.0L);
            x[col] = 1.0L;
            for (int j = 1; j < T; ++j) x[j] -= lo[j - 1] * x[j - 1];
            for (int j = 0; j < T; ++j) x[j] /= dg[j];
            for (int j = T - 2; j >= 0; --j) x[j] -= lo[j] * x[j + 1];
            for (int j = 0; j < T; ++j) Gl[((size_t)j * T + col) * m + c] = x[j];
        }
        for (int i = 0; i < T; ++i)
            for (int j = 0; j < T; ++j) {                          // (symmetrised: the two triangles agree to rounding)
                const ld v = 0.5L * (Gl[((size_t)i * T + j) * m + c] + Gl[((size_t)j * T + i) * m + c]);
                Out.Gf[((size_t)i * T + j) * m + c] = (double)v;
            }
        for (int j = 0; j < T; ++j) Out.g0[(size_t)j * m + c] = Out.Gf[((size_t)j * T + 0) * m + c];
    }
    for (size_t i = 0; i < Gl.size(); ++i) Gl[i] = (ld)Out.Gf[i];   // (the device applies the rounded values: keep the algebra consistent)
    auto qinv = [&](int jx, int r) -> ld { return 1.0L / (jx == T ? (ld)hm.Qf2[r] : (ld)hm.Q2[r]); };   // x_jx, jx = 1..T
    // ---- gbar, phibar = Phibar^-1 (-gbar)
    Out.gbar_u.assign((size_t)T * m, 0.0); Out.gbar_x.assign((size_t)T * n, 0.0);
    Out.phib_u.assign((size_t)T * m, 0.0); Out.phib_x.assign((size_t)T * n, 0.0);
    std::vector<ld> gu((size_t)T * m), gx((size_t)T * n), pu((size_t)T * m), px((size_t)T * n);
    for (int j = 0; j < T; ++j) {
        for (int c = 0; c < m; ++c)
            gu[(size_t)j * m + c] = (ld)hm.R2[c] * (ld)hm.umid[c] + (ld)hm.rl[c] + gb[c] + (j >= 1 ? grb[c] : 0.0L) - (j + 1 < T ? grb[c] : 0.0L);
        for (int r = 0; r < n; ++r) {
            const bool last = j + 1 == T;
            gx[(size_t)j * n + r] = last ? (ld)hm.Qf2[r] * (ld)hm.xmid[r] + (ld)hm.qfl[r] : (ld)hm.Q2[r] * (ld)hm.xmid[r] + (ld)hm.ql[r];
        }
    }
    for (int j = 0; j < T; ++j) {
        for (int c = 0; c < m; ++c) {
            ld t = 0.0L;
            for (int i = 0; i < T; ++i) t -= Gl[((size_t)j * T + i) * m + c] * gu[(size_t)i * m + c];
            pu[(size_t)j * m + c] = t;
        }
        for (int r = 0; r < n; ++r) px[(size_t)j * n + r] = -gx[(size_t)j * n + r] * qinv(j + 1, r);
    }
    for (size_t i = 0; i < gu.size(); ++i) { Out.gbar_u[i] = (double)gu[i]; Out.phib_u[i] = (double)pu[i]; }
    for (size_t i = 0; i < gx.size(); ++i) { Out.gbar_x[i] = (double)gx[i]; Out.phib_x[i] = (double)px[i]; }
    // ---- C as sparse rows (column, value); columns: u_j[c] = j s + c, x_{j+1}[r] = j s + m + r
    struct Ent { int col; ld v; };
    std::vector<std::vector<Ent>> Cr(nbn);
    for (int i = 0; i < T; ++i)
        for (int r = 0; r < n; ++r) {
            std::vector<Ent>& row = Cr[(size_t)i * n + r];
            row.push_back({i * s + m + r, 1.0L});
            for (int c = 0; c < m; ++c) row.push_back({i * s + c, -(ld)hm.bt[(size_t)c * n + r]});
            if (i >= 1) for (int q = 0; q < n; ++q) row.push_back({(i - 1) * s + m + q, -(ld)hm.a1[(size_t)r * n + q]});
            if (var2 && i >= 2) for (int q = 0; q < n; ++q) row.push_back({(i - 2) * s + m + q, -(ld)hm.a2[(size_t)r * n + q]});
        }
    if (has_xf) for (int r = 0; r < n; ++r) Cr[(size_t)T * n + r].push_back({(T - 1) * s + m + r, 1.0L});
    auto zstart = [&](int col) -> ld { const int e = col % s; return e < m ? (ld)hm.umid[e] : (ld)hm.xmid[e - m]; };
    // cpb = C z0 (- xf on the terminal rows), betab = C phibar + cpb
    Out.cpb.assign(nbn, 0.0); Out.betab.assign(nbn, 0.0);
    auto phib_at = [&](int col) -> ld { const int j = col / s, e = col % s; return e < m ? pu[(size_t)j * m + e] : px[(size_t)j * n + (e - m)]; };
    std::vector<ld> cpl(nbn), betal(nbn);
    for (int a = 0; a < nbn; ++a) {
        ld cz = 0.0L, cp = 0.0L;
        for (const Ent& e : Cr[a]) { cz += e.v * zstart(e.col); cp += e.v * phib_at(e.col); }
        if (a >= T * n) cz -= (ld)hm.xf[a - T * n];
        cpl[a] = cz; betal[a] = cp + cz;
        Out.cpb[a] = (double)cz; Out.betab[a] = (double)(cp + cz);
    }
    // ---- P = Phibar^-1 C' (Nz x nbn), Ybar = C P
    std::vector<ld> P((size_t)Nz * nbn, 0.0L);
    for (int b = 0; b < nbn; ++b)
        for (const Ent& e : Cr[b]) {
            const int j = e.col / s, el = e.col % s;
            if (el < m) { for (int jj = 0; jj < T; ++jj) P[((size_t)jj * s + el) * nbn + b] += Gl[((size_t)jj * T + j) * m + el] * e.v; }
            else P[(size_t)e.col * nbn + b] += e.v * qinv(j + 1, el - m);
        }
    std::vector<ld> Y((size_t)nbn * nbn, 0.0L);
    for (int a = 0; a < nbn; ++a)
        for (const Ent& e : Cr[a]) {
            const ld* prow = &P[(size_t)e.col * nbn];
            ld* yrow = &Y[(size_t)a * nbn];
            for (int b = 0; b < nbn; ++b) yrow[b] += e.v * prow[b];
        }
    // Cholesky Y = L L' (lower, in place), then Yinv = L^-T L^-1
    for (int j = 0; j < nbn; ++j) {
        ld d = Y[(size_t)j * nbn + j];
        for (int q = 0; q < j; ++q) d -= Y[(size_t)j * nbn + q] * Y[(size_t)j * nbn + q];
        if (!(d > 0.0L) || !std::isfinite((double)d)) return;
        const ld l = sqrtl(d);
        Y[(size_t)j * nbn + j] = l;
        for (int i = j + 1; i < nbn; ++i) {
            ld v = Y[(size_t)i * nbn + j];
            for (int q = 0; q < j; ++q) v -= Y[(size_t)i * nbn + q] * Y[(size_t)j * nbn + q];
            Y[(size_t)i * nbn + j] = v / l;
        }
    }
    std::vector<ld> Yi((size_t)nbn * nbn, 0.0L), x(nbn);
    for (int col = 0; col < nbn; ++col) {
        for (int i = 0; i < nbn; ++i) {
            ld v = i == col ? 1.0L : 0.0L;
            if (i < col) { x[i] = 0.0L; continue; }
            for (int q = col; q < i; ++q) v -= Y[(size_t)i * nbn + q] * x[q];
            x[i] = v / Y[(size_t)i * nbn + i];
        }
        for (int i = nbn - 1; i >= 0; --i) {
            ld v = x[i];
            for (int q = i + 1; q < nbn; ++q) v -= Y[(size_t)q * nbn + i] * x[q];
            x[i] = v / Y[(size_t)i * nbn + i];
        }
        for (int i = 0; i < nbn; ++i) Yi[(size_t)i * nbn + col] = x[i];
    }
    const int ldy = (nbn + 1) & ~1;                               // rows an even number of doubles apart (16-byte loads), pad column zero
    Out.Yinv.assign((size_t)nbn * ldy, 0.0);
    for (int a = 0; a < nbn; ++a)
        for (int b = 0; b < nbn; ++b) Out.Yinv[(size_t)a * ldy + b] = (double)(0.5L * (Yi[(size_t)a * nbn + b] + Yi[(size_t)b * nbn + a]));
    for (int a = 0; a < nbn; ++a)
        for (int b = 0; b < nbn; ++b) Yi[(size_t)a * nbn + b] = (ld)Out.Yinv[(size_t)a * ldy + b];
    // ---- Xi_u0 = P_{u0,:} Yinv (m x nbn);  G = Gf[0][0] - P_{u0,:} Yinv P_{u0,:}';  y0c = (Kbar^-1 (-[gbar; cpb]))_{u0}
    std::vector<ld> Xi((size_t)m * nbn, 0.0L);
    for (int r = 0; r < m; ++r)
        for (int a = 0; a < nbn; ++a) {
            const ld pv = P[(size_t)r * nbn + a];                 // (rows 0 .. m-1 of P are the u_0 rows)
            if (pv == 0.0L) continue;
            for (int b = 0; b < nbn; ++b) Xi[(size_t)r * nbn + b] += pv * Yi[(size_t)a * nbn + b];
        }
    const int ldg = (m + 1) & ~1;                                 // (rows of G and of Xiu0t an even number of doubles apart: 16-byte loads)
    Out.Xiu0t.assign((size_t)T * n * ldg, 0.0);
    for (int col = 0; col < T * n; ++col)
        for (int r = 0; r < m; ++r) Out.Xiu0t[(size_t)col * ldg + r] = (double)Xi[(size_t)r * nbn + col];
    Out.G.assign((size_t)m * ldg, 0.0);
    for (int r = 0; r < m; ++r)
        for (int c = r; c < m; ++c) {
            ld v = r == c ? Gl[((size_t)0 * T + 0) * m + r] : 0.0L;
            for (int b = 0; b < nbn; ++b) v -= Xi[(size_t)r * nbn + b] * P[(size_t)c * nbn + b];
            Out.G[(size_t)r * ldg + c] = (double)v; Out.G[(size_t)c * ldg + r] = (double)v;
        }
    // y0c: f_z = -gbar, f_nu = -cpb:  phi = phibar, nu = Yinv (C phibar + cpb) = Yinv betab, z_u0 = phibar_u0 - P_{u0,:} nu
    Out.y0c.assign(m, 0.0);
    {
        std::vector<ld> nu(nbn, 0.0L);
        for (int a = 0; a < nbn; ++a) { ld v = 0.0L; for (int b = 0; b < nbn; ++b) v += Yi[(size_t)a * nbn + b] * betal[b]; nu[a] = v; }
        for (int r = 0; r < m; ++r) {
            ld v = pu[r];
            for (int b = 0; b < nbn; ++b) v -= P[(size_t)r * nbn + b] * nu[b];
            Out.y0c[r] = (double)v;
        }
    }
    for (double v : Out.Yinv) if (!std::isfinite(v)) return;
    for (double v : Out.G) if (!std::isfinite(v)) return;
    Out.valid = 1;
}

int fmpc_host_estimator_gain(const double* A_s, int p, int nx, std::vector<double>& G) {
    typedef long double ld;
    std::vector<ld> M((size_t)nx * nx, 0.0L), V((size_t)nx * nx, 0.0L);
    for (int a = 0; a < nx; ++a)
        for (int b = a; b < nx; ++b) {
            ld s = 0.0L;
            for (int i = 0; i < p; ++i) s += (ld)A_s[(size_t)a * p + i] * (ld)A_s[(size_t)b * p + i];
            M[(size_t)a * nx + b] = s; M[(size_t)b * nx + a] = s;
        }
    for (int a = 0; a < nx; ++a) V[(size_t)a * nx + a] = 1.0L;
    // cyclic Jacobi on the symmetric M: M <- J' M J, V <- V J
    for (int sweep = 0; sweep < 60; ++sweep) {
        ld off = 0.0L, dia = 0.0L;
        for (int a = 0; a < nx; ++a) for (int b = 0; b < nx; ++b) { if (a != b) off += M[(size_t)a * nx + b] * M[(size_t)a * nx + b]; else dia += M[(size_t)a * nx + a] * M[(size_t)a * nx + a]; }
        if (off <= 1e-60L * dia || off == 0.0L) break;
        for (int a = 0; a < nx - 1; ++a)
            for (int b = a + 1; b < nx; ++b) {
                const ld apq = M[(size_t)a * nx + b];
                if (apq == 0.0L) continue;
                const ld theta = (M[(size_t)b * nx + b] - M[(size_t)a * nx + a]) / (2.0L * apq);
                const ld t = (theta >= 0.0L ? 1.0L : -1.0L) / (fabsl(theta) + sqrtl(theta * theta + 1.0L));
                const ld c = 1.0L / sqrtl(t * t + 1.0L), s = t * c;
                for (int k = 0; k < nx; ++k) {                       // columns a, b
                    const ld mka = M[(size_t)k * nx + a], mkb = M[(size_t)k * nx + b];
                    M[(size_t)k * nx + a] = c * mka - s * mkb; M[(size_t)k * nx + b] = s * mka + c * mkb;
                }
                for (int k = 0; k < nx; ++k) {                       // rows a, b
                    const ld mak = M[(size_t)a * nx + k], mbk = M[(size_t)b * nx + k];
                    M[(size_t)a * nx + k] = c * mak - s * mbk; M[(size_t)b * nx + k] = s * mak + c * mbk;
                }
                for (int k = 0; k < nx; ++k) {
                    const ld vka = V[(size_t)k * nx + a], vkb = V[(size_t)k * nx + b];
                    V[(size_t)k * nx + a] = c * vka - s * vkb; V[(size_t)k * nx + b] = s * vka + c * vkb;
                }
            }
    }
    ld lmax = 0.0L;
    for (int a = 0; a < nx; ++a) lmax = fmaxl(lmax, fabsl(M[(size_t)a * nx + a]));
    const ld tol = (ld)nx * 2.220446049250313e-16L * lmax;
    int rank = 0;
    std::vector<ld> inv(nx, 0.0L);
    for (int a = 0; a < nx; ++a) if (M[(size_t)a * nx + a] > tol) { inv[a] = 1.0L / M[(size_t)a * nx + a]; ++rank; }
    // pinv = V diag(inv) V' ;  G = pinv A_s'
    std::vector<ld> Pm((size_t)nx * nx, 0.0L);
    for (int a = 0; a < nx; ++a)
        for (int b = 0; b < nx; ++b) {
            ld s = 0.0L;
            for (int k = 0; k < nx; ++k) s += V[(size_t)a * nx + k] * inv[k] * V[(size_t)b * nx + k];
            Pm[(size_t)a * nx + b] = s;
        }
    G.assign((size_t)nx * p, 0.0);
    for (int a = 0; a < nx; ++a)
        for (int i = 0; i < p; ++i) {
            ld s = 0.0L;
            for (int b = 0; b < nx; ++b) s += Pm[(size_t)a * nx + b] * (ld)A_s[(size_t)b * p + i];
            G[(size_t)a * p + i] = (double)s;
        }
    return rank;
}

void fmpc_host_estimator_dft_images(int len, int d, int first, std::vector<double>& img) {
    typedef long double ld;
    const ld two_pi = 6.283185307179586476925286766559L;
    img.assign((size_t)(len / 4) * 2 * 2 * 64, 0.0);
    for (int y = 0; y < len; ++y)
        for (int j = 0; j < d && j < 32; ++j) {
            // the exponent reduced mod len in integers: the argument of cos / sin stays in [0, 2 pi)
            const long long e = ((long long)(first + j - len / 2) * (long long)(y - len / 2)) % len;
            const ld ang = -two_pi * (ld)((e + len) % len) / (ld)len;
            const size_t base = (((size_t)(y / 4) * 2 + (j / 16)) * 2) * 64 + (size_t)(y % 4) * 16 + (j % 16);
            img[base] = (double)cosl(ang);
            img[base + 64] = (double)sinl(ang);
        }
}

// ---- lane plan of a chain of affine steps (fmpc_kernel_affine.hip)
int fmpc_host_plan_lanes(int nsteps, const unsigned* supersedes, int ngroups, int slots, int tiles_used, int cap, int* lane_of_step, int* wpg_out) {
    if (ngroups < 1) ngroups = 1;
    const int wpg_max = (tiles_used + 3) / 4 > 0 ? (tiles_used + 3) / 4 : 1;   // one tile per wavefront at least
    auto wpg_of = [&](int L) { const int w = slots / (ngroups * L); return w < 1 ? 1 : (w > wpg_max ? wpg_max : w); };
    for (int i = 0; i < nsteps; ++i) lane_of_step[i] = 0;
    *wpg_out = wpg_of(1);
    if (nsteps <= 1) return 1;
    // classes: the steps of one output tuple, in chain order.  A step knows "the same tuple as pending step i" (any such i): the
    // lowest one it names, followed down to a step that names none, is its class -- the relation made transitive.
    std::vector<int> cls(nsteps), first, len;
    for (int j = 0; j < nsteps; ++j) {
        int rep = j;
        for (int i = 0; i < j; ++i) if (supersedes[j] >> i & 1u) { rep = first[cls[i]]; break; }
        if (rep == j) { cls[j] = (int)first.size(); first.push_back(j); len.push_back(1); }
        else { cls[j] = cls[rep]; ++len[cls[j]]; }
    }
    const int nc = (int)first.size();
    std::vector<int> order(nc);                                                // longest first, ties in chain order
    for (int c = 0; c < nc; ++c) order[c] = c;
    for (int a = 1; a < nc; ++a)
        for (int b = a; b > 0 && len[order[b]] > len[order[b - 1]]; --b) { const int t = order[b]; order[b] = order[b - 1]; order[b - 1] = t; }
    int Lmax = slots / ngroups < 1 ? 1 : slots / ngroups;
    if (Lmax > nc) Lmax = nc;
    if (cap >= 1 && Lmax > cap) Lmax = cap;
    if (cap < 1) Lmax = 1;
    int bestL = 1; long best = -1;
    std::vector<int> lane_of_cls(nc), best_lanes(nc, 0), load;
    for (int L = 1; L <= Lmax; ++L) {
        load.assign(L, 0);
        for (int o = 0; o < nc; ++o) {
            int to = 0;
            for (int l = 1; l < L; ++l) if (load[l] < load[to]) to = l;        // the least loaded lane, ties to the lowest
            lane_of_cls[order[o]] = to; load[to] += len[order[o]];
        }
        int H = 0;
        for (int l = 0; l < L; ++l) if (load[l] > H) H = load[l];
        const int w = wpg_of(L), R = (tiles_used + 4 * w - 1) / (4 * w);
        const long cost = (long)H * (R + FMPC_LANE_START_ROUNDS);
        if (best < 0 || cost < best) { best = cost; bestL = L; best_lanes = lane_of_cls; }
    }
    for (int j = 0; j < nsteps; ++j) lane_of_step[j] = best_lanes[cls[j]];
    *wpg_out = wpg_of(bestL);
    return bestL;
}

extern "C" int fmpc_debug_plan_lanes(int nsteps, const unsigned* supersedes, int ngroups, int slots, int tiles_used, int cap, int* lane_of_step,
                                     int* lanes, int* wpg) {
    if (nsteps < 0 || nsteps > 32 || (nsteps && (!supersedes || !lane_of_step)) || !lanes || !wpg) return -1;
    int dummy = 0;
    *lanes = fmpc_host_plan_lanes(nsteps, supersedes, ngroups, slots, tiles_used, cap, nsteps ? lane_of_step : &dummy, wpg);
    return 0;
}

void fmpc_host_estimator_qranges(int len, int ndiv, const double* D_re, const double* D_im, std::vector<int>& qr) {
    const int nblk = len / 16, nks = len / 4;
    const size_t npx = (size_t)len * len;
    qr.assign((size_t)2 * nblk, 0);
    for (int b = 0; b < nblk; ++b) {
        int lo = nks, hi = 0;
        for (int Q = 0; Q < nks; ++Q) {
            bool any = false;
            for (int k = 0; k < ndiv && !any; ++k)
                for (int x = 4 * Q; x < 4 * Q + 4 && !any; ++x)
                    for (int y = 16 * b; y < 16 * b + 16; ++y) {
                        const size_t o = (size_t)k * npx + (size_t)x * len + y;            // column-major: (row y, column x)
                        if (D_re[o] != 0.0 || D_im[o] != 0.0) { any = true; break; }
                    }
            if (any) { if (Q < lo) lo = Q; hi = Q + 1; }
        }
        if (hi <= lo) { lo = 0; hi = 0; }
        qr[2 * b] = lo; qr[2 * b + 1] = hi;
    }
}

// ---- Zernike functions (zernfun.m, zernmodfit.m)
int fmpc_host_zernike_modes(int N, int* n_out, int* m_out) {
    if (N < 0) return 0;
    int j = 0;
    for (int n = 0; n <= N; ++n)
        for (int m = -n; m <= n; m += 2, ++j) {        // zernmodfit.m:197: [(-x:2:-1) fliplr(x:-2:0)] = -x:2:x
            if (n_out) n_out[j] = n;
            if (m_out) m_out[j] = m;
        }
    return j;
}

void fmpc_host_zernike_coefficients(double coef[FMPC_ZERNIKE_NCOEF], unsigned short off[FMPC_ZERNIKE_MAXN + 1][8]) {
    double fact[FMPC_ZERNIKE_MAXN + 1];
    fact[0] = 1.0;
    for (int i = 1; i <= FMPC_ZERNIKE_MAXN; ++i) fact[i] = fact[i - 1] * i;
    int o = 0;
    for (int n = 0; n <= FMPC_ZERNIKE_MAXN; ++n) {
        for (int h = 0; h < 8; ++h) off[n][h] = 0;
        for (int ma = n & 1; ma <= n; ma += 2) {
            off[n][ma / 2] = (unsigned short)o;
            for (int s = 0; s <= (n - ma) / 2; ++s)       // zernfun.m:166-170, the quotients taken in its order (each one an integer)
                coef[o++] = (1 - 2 * (s & 1)) * fact[n - s] / fact[s] / fact[(n - ma) / 2 - s] / fact[(n + ma) / 2 - s];
        }
    }
}

// ---- measurement noise (fmpc_noise.h): the argument rules of the fmpc_noise block, the draw on the host
double fmpc_host_mean_square(const double* v, int cnt) {
    double s = 0.0;
    for (int i = 0; i < cnt; ++i) s += v[i] * v[i];
    return cnt > 0 ? s / cnt : 0.0;
}

int fmpc_host_noise_check(const fmpc_noise* nz, int batch, int sigma_only) {
    if (!nz) return FMPC_E_NULL;
    if (nz->mode != FMPC_NOISE_SIGMA && nz->mode != FMPC_NOISE_SNR_MEASURED) return FMPC_E_DIM;
    if (sigma_only && nz->mode != FMPC_NOISE_SIGMA) return FMPC_E_DIM;
    if (batch < 0 || nz->first < 0 || nz->first > (1ll << 32) || nz->first + (long long)batch > (1ll << 32)) return FMPC_E_DIM;
    if (!std::isfinite(nz->value)) return FMPC_E_DIM;
    if (nz->mode == FMPC_NOISE_SIGMA && nz->value < 0.0) return FMPC_E_DIM;
    if (nz->mode == FMPC_NOISE_SNR_MEASURED && nz->sigma_dev) return FMPC_E_DIM;
    return FMPC_OK;
}

extern "C" int fmpc_philox4x32_10(const unsigned int counter[4], const unsigned int key[2], unsigned int out[4]) {
    if (!counter || !key || !out) return FMPC_E_NULL;
    uint32_t c[4] = {counter[0], counter[1], counter[2], counter[3]}, k[2] = {key[0], key[1]}, x[4];
    fmpc_philox4x32_10_block(c, k, x);
    for (int i = 0; i < 4; ++i) out[i] = x[i];
    return FMPC_OK;
}

extern "C" int fmpc_noise_normal_host(double* out, int batch, int p, long long ld, const fmpc_noise* nz) {
    if (!out || !nz) return FMPC_E_NULL;
    const int rc = fmpc_host_noise_check(nz, batch, 1);
    if (rc != FMPC_OK) return rc;
    if (p < 1 || (ld != 0 && ld < p)) return FMPC_E_DIM;
    if (nz->sigma_dev || nz->step_dev) return FMPC_E_DIM;          // device pointers: not readable here
    if (ld == 0) ld = p;
    for (int r = 0; r < batch; ++r)
        for (int i = 0; i < p; ++i)
            out[(size_t)r * ld + i] = fmpc_noise_scaled(nz->value, fmpc_noise_normal(nz->seed, nz->step, (uint32_t)(nz->first + r), (uint32_t)i));
    return FMPC_OK;
}

// ---- detector (fmpc_detector.h): the argument rules of the fmpc_detector block, the read-out on the host
double fmpc_host_sum(const double* v, int cnt) {
    double s = 0.0;
    for (int i = 0; i < cnt; ++i) s += v[i];
    return s;
}

int fmpc_host_detector_check(const fmpc_detector* det, int batch) {
    if (!det) return FMPC_E_NULL;
    if (batch < 0 || det->first < 0 || det->first > (1ll << 32) || det->first + (long long)batch > (1ll << 32)) return FMPC_E_DIM;
    if (!std::isfinite(det->gain) || det->gain < 0.0 || (det->gain == 0.0 && !det->gain_dev)) return FMPC_E_DIM;
    if (!std::isfinite(det->qe) || !(det->qe > 0.0)) return FMPC_E_DIM;
    if (!std::isfinite(det->background) || det->background < 0.0 || !std::isfinite(det->read_noise) || det->read_noise < 0.0) return FMPC_E_DIM;
    return FMPC_OK;
}

extern "C" int fmpc_detector_read_host(double* Y, const double* Y0, int batch, int p, long long ld, const fmpc_detector* det) {
    if (!Y || !Y0 || !det) return FMPC_E_NULL;
    const int rc = fmpc_host_detector_check(det, batch);
    if (rc != FMPC_OK) return rc;
    if (p < 1 || p > FMPC_DET_MAX_P || (ld != 0 && ld < p)) return FMPC_E_DIM;
    if (det->gain_dev || det->step_dev) return FMPC_E_DIM;         // device pointers: not readable here
    if (ld == 0) ld = p;
    for (int r = 0; r < batch; ++r)
        for (int i = 0; i < p; ++i)
            Y[(size_t)r * ld + i] = fmpc_detector_read(Y0[(size_t)r * ld + i], det->gain, det->qe, det->background, det->read_noise, det->photon_noise,
                                                       det->seed, det->step, (uint32_t)(det->first + r), (uint32_t)i);
    return FMPC_OK;
}

// ---- atmosphere: von Karman covariance (OOMAO phaseStats.m:20-39), the extruders A = ZX' ZZ^-1, B = chol(XX - A ZX)
extern "C" int fmpc_atm_covariance_host(int n, const double* rho, double r0, double L0, double* out) {
    if (!rho || !out) return FMPC_E_NULL;
    if (n < 0 || !(r0 > 0.0) || !(L0 > 0.0) || !std::isfinite(r0) || !std::isfinite(L0)) return FMPC_E_DIM;
    const double pi = 3.14159265358979323846;
    const double ratio = pow(L0 / r0, 5.0 / 3.0), lead = pow(24.0 * tgamma(6.0 / 5.0) / 5.0, 5.0 / 6.0);
    const double cst = lead * (tgamma(11.0 / 6.0) / (pow(2.0, 5.0 / 6.0) * pow(pi, 8.0 / 3.0))) * ratio;
    const double var = lead * (tgamma(11.0 / 6.0) * tgamma(5.0 / 6.0) / (2.0 * pow(pi, 8.0 / 3.0))) * ratio;
    for (int i = 0; i < n; ++i) {
        if (!(rho[i] >= 0.0) || !std::isfinite(rho[i])) return FMPC_E_DIM;
        const double u = 2.0 * pi * rho[i] / L0;
        out[i] = u != 0.0 ? cst * pow(u, 5.0 / 6.0) * std::cyl_bessel_k(5.0 / 6.0, u) : var;
    }
    return FMPC_OK;
}

int fmpc_host_atm_check(int W, double pitch, double r0, double L0, int q, const int* stencil) {
    if (W < 3 || !(pitch > 0.0) || !(r0 > 0.0) || !(L0 > 0.0) || !std::isfinite(pitch) || !std::isfinite(r0) || !std::isfinite(L0)) return FMPC_E_DIM;
    if (q < 1) return FMPC_E_DIM;
    for (int j = 0; j < q && j <= FMPC_ATM_MAXQ; ++j)
        if (stencil[j] < 1 || stencil[j] > W || (j > 0 && stencil[j] <= stencil[j - 1])) return FMPC_E_DIM;
    if (q > FMPC_ATM_MAXQ || (long long)q * W > FMPC_ATM_MAXK) return FMPC_E_UNSUPPORTED;
    return FMPC_OK;
}

int fmpc_host_atm_default_stencil(int W, int* stencil) {
    int q = 0;
    for (int s = 1; s <= W - 1 && q < FMPC_ATM_MAXQ; s *= 2) stencil[q++] = s;
    return q;
}

// lower Cholesky factor in place, rows packed (row r at r (r + 1) / 2); false when a pivot is not positive
static bool atm_chol_packed(std::vector<long double>& L, int N) {
    for (int r = 0; r < N; ++r) {
        long double* lr = L.data() + (size_t)r * (r + 1) / 2;
        for (int c = 0; c <= r; ++c) {
            const long double* lc = L.data() + (size_t)c * (c + 1) / 2;
            long double s = lr[c];
            for (int k = 0; k < c; ++k) s -= lr[k] * lc[k];
            if (c == r) {
                if (!(s > 0.0L) || !std::isfinite((double)s)) return false;
                lr[c] = sqrtl(s);
            } else {
                lr[c] = s / lc[c];
            }
        }
    }
    return true;
}

int fmpc_host_atm_extruders(int W, double pitch, double r0, double L0, int q, const int* stencil, bool all, FmpcAtmExtruders& out) {
    const int N = q * W;
    out.A.assign(q + 1, std::vector<double>());
    out.B.assign(q + 1, std::vector<double>());
    // C(pitch hypot(ds, di)) for every line distance ds that occurs: 0, s_a, s_b - s_a
    std::vector<int> dss(1, 0);
    for (int a = 0; a < q; ++a) {
        dss.push_back(stencil[a]);
        for (int b = a + 1; b < q; ++b) dss.push_back(stencil[b] - stencil[a]);
    }
    std::sort(dss.begin(), dss.end());
    dss.erase(std::unique(dss.begin(), dss.end()), dss.end());
    std::vector<std::vector<long double>> cov(dss.size(), std::vector<long double>(W));
    {
        std::vector<double> rho(W), c(W);
        for (size_t d = 0; d < dss.size(); ++d) {
            for (int i = 0; i < W; ++i) rho[i] = pitch * hypot((double)dss[d], (double)i);
            if (fmpc_atm_covariance_host(W, rho.data(), r0, L0, c.data()) != FMPC_OK) return FMPC_E_UNSUPPORTED;
            for (int i = 0; i < W; ++i) {
                if (!std::isfinite(c[i])) return FMPC_E_UNSUPPORTED;
                cov[d][i] = c[i];
            }
        }
    }
    auto C = [&](int ds, int di) -> long double {
        ds = ds < 0 ? -ds : ds; di = di < 0 ? -di : di;
        return cov[std::lower_bound(dss.begin(), dss.end(), ds) - dss.begin()][di];
    };
    // ZZ = L L'
    std::vector<long double> L((size_t)N * (N + 1) / 2);
    for (int a = 0; a < q; ++a)
        for (int i = 0; i < W; ++i) {
            long double* lr = L.data() + (size_t)(a * W + i) * (a * W + i + 1) / 2;
            for (int b = 0; b <= a; ++b)
                for (int k = 0; k < W && b * W + k <= a * W + i; ++k) lr[b * W + k] = C(stencil[a] - stencil[b], i - k);
        }
    if (!atm_chol_packed(L, N)) return FMPC_E_UNSUPPORTED;
    // Y = L^-1 ZX, one right-hand side per point of the new line (stored by right-hand side)
    std::vector<long double> Y((size_t)W * N);
    for (int w = 0; w < W; ++w) {
        long double* y = Y.data() + (size_t)w * N;
        for (int r = 0; r < N; ++r) {
            const long double* lr = L.data() + (size_t)r * (r + 1) / 2;
            long double s = C(stencil[r / W], r % W - w);
            for (int k = 0; k < r; ++k) s -= lr[k] * y[k];
            y[r] = s / lr[r];
        }
    }
    std::vector<long double> a(N), S((size_t)W * (W + 1) / 2);
    for (int j = all ? 0 : q; j <= q; ++j) {
        const int Nj = j * W;
        // A_j: row w solves L_j' a = y_w
        out.A[j].assign((size_t)W * Nj, 0.0);
        for (int w = 0; w < W; ++w) {
            for (int r = 0; r < Nj; ++r) a[r] = Y[(size_t)w * N + r];
            for (int r = Nj - 1; r >= 0; --r) {
                const long double* lr = L.data() + (size_t)r * (r + 1) / 2;
                a[r] /= lr[r];
                for (int k = 0; k < r; ++k) a[k] -= lr[k] * a[r];
            }
            for (int r = 0; r < Nj; ++r) out.A[j][(size_t)w * Nj + r] = (double)a[r];
        }
        // B_j = chol(XX - A_j ZX_j) = chol(XX - Y_j' Y_j)
        for (int w = 0; w < W; ++w)
            for (int v = 0; v <= w; ++v) {
                long double s = C(0, w - v);
                const long double *yw = Y.data() + (size_t)w * N, *yv = Y.data() + (size_t)v * N;
                for (int r = 0; r < Nj; ++r) s -= yw[r] * yv[r];
                S[(size_t)w * (w + 1) / 2 + v] = s;
            }
        if (!atm_chol_packed(S, W)) return FMPC_E_UNSUPPORTED;
        out.B[j].assign((size_t)W * W, 0.0);
        for (int w = 0; w < W; ++w)
            for (int v = 0; v <= w; ++v) out.B[j][(size_t)w * W + v] = (double)S[(size_t)w * (w + 1) / 2 + v];
    }
    return FMPC_OK;
}

void fmpc_host_atm_images(int W, int q, const FmpcAtmExtruders& X, std::vector<double>& img, unsigned long long* off) {
    const int Wp4 = fmpc_atm_wp4(W), NT = fmpc_atm_tiles(W);
    size_t total = 0;
    for (int j = 0; j <= q; ++j) { off[j] = total; total += fmpc_atm_img_doubles(W, j); }
    img.assign(total, 0.0);
    for (int j = 0; j <= q; ++j) {
        const int KS = (j + 1) * (Wp4 / 4);
        for (int tile = 0; tile < NT; ++tile)
            for (int ks = 0; ks < KS; ++ks)
                for (int lane = 0; lane < 64; ++lane) {
                    const int row = 16 * tile + (lane & 15), kk = 4 * ks + (lane >> 4), part = kk / Wp4, i = kk % Wp4;
                    if (row >= W || i >= W) continue;
                    img[off[j] + ((size_t)tile * KS + ks) * 64 + lane] =
                        part < j ? X.A[j][(size_t)row * (j * W) + (size_t)part * W + i] : X.B[j][(size_t)row * W + i];
                }
    }
}

extern "C" int fmpc_atm_extruder_host(int W, double pitch, double r0, double L0, int q, const int* stencil, double* A, double* B) {
    const bool first_line = stencil && q == 0;            // B_0 = chol(XX) of the start-up's first line: no A
    if (!B || (!A && !first_line)) return FMPC_E_NULL;
    int def[FMPC_ATM_MAXQ], one = 1;
    if (!stencil) {
        if (W < 3) return FMPC_E_DIM;
        q = fmpc_host_atm_default_stencil(W, def);
        stencil = def;
    }
    const int rc = first_line ? fmpc_host_atm_check(W, pitch, r0, L0, 1, &one) : fmpc_host_atm_check(W, pitch, r0, L0, q, stencil);
    if (rc != FMPC_OK) return rc;
    FmpcAtmExtruders X;
    const int rb = fmpc_host_atm_extruders(W, pitch, r0, L0, q, stencil, false, X);
    if (rb != FMPC_OK) return rb;
    if (!first_line) memcpy(A, X.A[q].data(), X.A[q].size() * sizeof(double));
    memcpy(B, X.B[q].data(), X.B[q].size() * sizeof(double));
    return FMPC_OK;
}

extern "C" int fmpc_atm_displacement_host(long long k, double px_per_step, long long* lines, double* frac) {
    if (!lines || !frac) return FMPC_E_NULL;
    if (k < 0 || !std::isfinite(px_per_step)) return FMPC_E_DIM;
    const double d = fabs((double)k * px_per_step);
    if (!(d < 4503599627370496.0)) return FMPC_E_UNSUPPORTED;         // 2^52: beyond it a double holds no fraction
    const double n = floor(d);
    *lines = (long long)n;
    *frac = d - n;
    return FMPC_OK;
}

// ---- science camera (include/fastmpc.h: fmpc_sci; layouts: fmpc_science.h)
int fmpc_host_sci_check(int len, int d, double sampling, double scale) {
    if (len < 1 || d < 1 || !std::isfinite(sampling) || sampling < 1.0 || !std::isfinite(scale)) return FMPC_E_DIM;
    if (len % 64 != 0 || len > FMPC_SCI_MAXLEN || (d != 16 && d != 32 && d != 48 && d != 64)) return FMPC_E_UNSUPPORTED;
    return FMPC_OK;
}

int fmpc_host_sci_tables(int len, int d, double sampling, const double* pupil, double scale, FmpcSciTables& out) {
    typedef long double ld;
    const int rc = fmpc_host_sci_check(len, d, sampling, scale);
    if (rc != FMPC_OK) return rc;
    const size_t npx = (size_t)len * len;
    ld sa = 0.0L, sa2 = 0.0L;
    for (size_t i = 0; i < npx; ++i) {
        if (!std::isfinite(pupil[i]) || pupil[i] < 0.0) return FMPC_E_DIM;
        sa += (ld)pupil[i]; sa2 += (ld)pupil[i] * (ld)pupil[i];
    }
    if (!(sa > 0.0L)) return FMPC_E_DIM;                                  // an all-zero pupil has no Strehl ratio
    out.sumA = (double)sa; out.sumA2 = (double)sa2; out.I0 = (double)((ld)scale * sa * sa);
    // F[y][j] = exp(-2 pi i (j - d/2)(y - len/2) / (s len)) as operand images [len / 4][d / 16][re, im][64 lanes],
    // lane = 16 (y mod 4) + (j mod 16).  The turn count n / (s len) is reduced to [-1/2, 1/2] before it meets 2 pi: in integers
    // where s len is one, in long double otherwise (|n| <= 32 len / 2: the quotient is good to 1e-18 of a turn).
    const ld two_pi = 6.283185307179586476925286766559L;
    const ld period = (ld)sampling * (ld)len;
    const bool whole = period == floorl(period) && period < 1.0e15L;
    const long long M = whole ? (long long)period : 0;
    const int nt = d / 16;
    out.Fimg.assign((size_t)(len / 4) * nt * 2 * 64, 0.0);
    for (int y = 0; y < len; ++y)
        for (int j = 0; j < d; ++j) {
            const long long n = (long long)(j - d / 2) * (long long)(y - len / 2);
            ld turn;
            if (whole) turn = (ld)(((n % M) + M) % M) / (ld)M;
            else { turn = (ld)n / period; turn -= roundl(turn); }
            const ld ang = -two_pi * turn;
            const size_t base = (((size_t)(y / 4) * nt + (j / 16)) * 2) * 64 + (size_t)(y % 4) * 16 + (j % 16);
            out.Fimg[base] = (double)cosl(ang);
            out.Fimg[base + 64] = (double)sinl(ang);
        }
    fmpc_host_estimator_qranges(len, 1, pupil, pupil, out.qr);           // (the k-steps with a pixel A != 0)
    return FMPC_OK;
}

extern "C" int fmpc_sci_tables_host(int len, int d, double sampling, const double* pupil, double scale, double* F_re, double* F_im,
                                    int* qrange, double* sums) {
    if (!pupil) return FMPC_E_NULL;
    FmpcSciTables t;
    const int rc = fmpc_host_sci_tables(len, d, sampling, pupil, scale, t);
    if (rc != FMPC_OK) return rc;
    const int nt = d / 16;
    for (int y = 0; y < len && (F_re || F_im); ++y)
        for (int j = 0; j < d; ++j) {
            const size_t base = (((size_t)(y / 4) * nt + (j / 16)) * 2) * 64 + (size_t)(y % 4) * 16 + (j % 16);
            if (F_re) F_re[(size_t)y * d + j] = t.Fimg[base];
            if (F_im) F_im[(size_t)y * d + j] = t.Fimg[base + 64];
        }
    if (qrange) memcpy(qrange, t.qr.data(), t.qr.size() * sizeof(int));
    if (sums) { sums[0] = t.sumA; sums[1] = t.sumA2; sums[2] = t.I0; }
    return FMPC_OK;
}

// ---- Shack-Hartmann sensor
int fmpc_host_sh_check(int len, int npl, int pad, int s) {
    if (len < 1 || npl < 1 || pad < 1 || s < 1) return FMPC_E_DIM;
    if (npl != 16 && npl != 32) return FMPC_E_UNSUPPORTED;
    if (len % npl != 0 || len > FMPC_SH_MAXLEN || pad > 4) return FMPC_E_UNSUPPORTED;
    const int nout = pad * npl;
    if (s % 2 != 0 || s > 32 || s > nout) return FMPC_E_UNSUPPORTED;
    return FMPC_OK;
}

int fmpc_host_sh_amplitude_check(int len, const double* amplitude) {
    const size_t npx = (size_t)len * len;
    for (size_t i = 0; i < npx; ++i)
        if (!std::isfinite(amplitude[i]) || amplitude[i] < 0.0) return FMPC_E_DIM;
    return FMPC_OK;
}

void fmpc_host_sh_lit(int len, int npl, const double* amplitude, std::vector<unsigned char>& lit) {
    const int nL = len / npl;
    lit.assign((size_t)nL * nL, 0);
    for (int x = 0; x < len; ++x)
        for (int y = 0; y < len; ++y)
            if (amplitude[(size_t)x * len + y] > 0.0) lit[(size_t)(y / npl) + (size_t)nL * (x / npl)] = 1;
}

void fmpc_host_sh_factors(int npl, int pad, int s, std::vector<double>& Fimg) {
    typedef long double ld;
    const ld pi = 3.141592653589793238462643383279503L;
    const int nt = s > 16 ? 2 : 1, nout = pad * npl, M = 2 * nout;
    Fimg.assign((size_t)(npl / 4) * nt * 2 * 64, 0.0);
    for (int x = 0; x < npl; ++x)
        for (int a = 0; a < s; ++a) {
            // x (a - (s - 1) / 2) / nOut turns = x (2 a - s + 1) / (2 nOut): reduced in integers before it meets pi
            const int n = ((x * (2 * a - s + 1)) % M + M) % M;
            const ld ang = -pi * (ld)n / (ld)nout;
            const size_t base = (((size_t)(x / 4) * nt + (a / 16)) * 2) * 64 + (size_t)(x % 4) * 16 + (a % 16);
            Fimg[base] = (double)cosl(ang);
            Fimg[base + 64] = (double)sinl(ang);
        }
}

extern "C" int fmpc_sh_valid_host(int len, int npl, const double* amplitude, double min_light_ratio, unsigned char* valid, int* nvalid) {
    typedef long double ld;
    if (!amplitude || (!valid && !nvalid)) return FMPC_E_NULL;
    int rc = fmpc_host_sh_check(len, npl, 1, 2);                          // (the size rules of len and npl alone)
    if (rc != FMPC_OK) return rc;
    if (!std::isfinite(min_light_ratio)) return FMPC_E_DIM;
    rc = fmpc_host_sh_amplitude_check(len, amplitude);
    if (rc != FMPC_OK) return rc;
    const int nL = len / npl;
    int count = 0;
    for (int j = 0; j < nL; ++j)
        for (int i = 0; i < nL; ++i) {
            ld sum = 0.0L;
            for (int x = 0; x < npl; ++x)
                for (int y = 0; y < npl; ++y) {
                    const ld a = (ld)amplitude[(size_t)(j * npl + x) * len + (size_t)(i * npl + y)];
                    sum += a * a;
                }
            const bool ok = (double)(sum / (ld)(npl * npl)) >= min_light_ratio;
            if (valid) valid[(size_t)i + (size_t)nL * j] = ok ? 1 : 0;
            count += ok ? 1 : 0;
        }
    if (nvalid) *nvalid = count;
    return FMPC_OK;
}

// ---------------------------------------------------------------------------------------------------------------- spline mirror
// MATLAB's spline(x, y) for n >= 4 ascending sites: the not-a-knot cubic through them, by its slopes.  The system is tridiagonal
// (the two not-a-knot rows touch two unknowns each) and is solved by elimination without pivoting, in long double.
static bool dmsp_slopes(const std::vector<long double>& x, const std::vector<long double>& y, std::vector<long double>& s) {
    typedef long double ld;
    const size_t n = x.size();
    if (n < 4 || y.size() != n) return false;
    std::vector<ld> h(n - 1), dl(n - 1), lo(n, 0.0L), di(n), up(n, 0.0L), b(n);
    for (size_t i = 0; i + 1 < n; ++i) {
        h[i] = x[i + 1] - x[i];
        if (!(h[i] > 0.0L)) return false;
        dl[i] = (y[i + 1] - y[i]) / h[i];
    }
    const ld d0 = x[2] - x[0], d1 = x[n - 1] - x[n - 3];
    di[0] = h[1]; up[0] = d0;
    b[0] = ((h[0] + 2.0L * d0) * h[1] * dl[0] + h[0] * h[0] * dl[1]) / d0;
    for (size_t i = 1; i + 1 < n; ++i) {
        lo[i] = h[i]; di[i] = 2.0L * (h[i - 1] + h[i]); up[i] = h[i - 1];
        b[i] = 3.0L * (h[i] * dl[i - 1] + h[i - 1] * dl[i]);
    }
    lo[n - 1] = d1; di[n - 1] = h[n - 3];
    b[n - 1] = (h[n - 2] * h[n - 2] * dl[n - 3] + (2.0L * d1 + h[n - 2]) * h[n - 3] * dl[n - 2]) / d1;
    for (size_t i = 1; i < n; ++i) {
        const ld w = lo[i] / di[i - 1];
        di[i] -= w * up[i - 1];
        b[i] -= w * b[i - 1];
    }
    s.assign(n, 0.0L);
    s[n - 1] = b[n - 1] / di[n - 1];
    for (size_t i = n - 1; i-- > 0;) s[i] = (b[i] - up[i] * s[i + 1]) / di[i];
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite((double)s[i])) return false;
    return true;
}

// the four coefficients of piece i in powers of (x - x[i])
static void dmsp_piece(const std::vector<long double>& x, const std::vector<long double>& y, const std::vector<long double>& s, size_t i,
                       long double c[4]) {
    const long double h = x[i + 1] - x[i], dl = (y[i + 1] - y[i]) / h;
    c[0] = y[i]; c[1] = s[i];
    c[2] = (3.0L * dl - 2.0L * s[i] - s[i + 1]) / h;
    c[3] = (s[i] + s[i + 1] - 2.0L * dl) / (h * h);
}

extern "C" int fmpc_dm_profile_oomao_host(double p2x, const double* p3, const double* p4, double ratio, double p6x, double mech, int cap,
                                          double* breaks, double* coef, int* pieces) {
    typedef long double ld;
    if (!p3 || !p4 || !breaks || !coef || !pieces) return FMPC_E_NULL;
    const int NS = 101, NP = 2 * NS - 1, NK = 2 * NP - 1;                 // samples per segment, points of the half curve, knots
    if (cap < NK - 1) return FMPC_E_DIM;
    const double in[] = {p2x, p3[0], p3[1], p4[0], p4[1], ratio, p6x, mech};
    for (double v : in)
        if (!std::isfinite(v)) return FMPC_E_DIM;
    if (!(mech > 0.0 && mech < 1.0) || ratio == 0.0) return FMPC_E_DIM;
    ld P[7][2] = {{0.0L, 1.0L}, {p2x, 1.0L}, {p3[0], p3[1]}, {p4[0], p4[1]}, {0.0L, 0.0L}, {p6x, 0.0L}, {2.0L, 0.0L}};
    for (int k = 0; k < 2; ++k) P[4][k] = -P[2][k] / (ld)ratio + (1.0L + 1.0L / (ld)ratio) * P[3][k];
    // the two Bezier segments at t = 0, 1/100, .., 1 (the second without its t = 0), rounded to double as the reference holds them
    std::vector<ld> bx(NP), by(NP);
    for (int seg = 0; seg < 2; ++seg)
        for (int j = seg; j < NS; ++j) {
            const ld t = (ld)j / (ld)(NS - 1), q = 1.0L - t;
            const ld w[4] = {q * q * q, 3.0L * q * q * t, 3.0L * q * t * t, t * t * t};
            ld px = 0.0L, py = 0.0L;
            for (int k = 0; k < 4; ++k) { px += w[k] * P[3 * seg + k][0]; py += w[k] * P[3 * seg + k][1]; }
            const int at = seg * (NS - 1) + j;
            bx[at] = (ld)(double)px; by[at] = (ld)(double)py;
            if (!std::isfinite((double)px) || !std::isfinite((double)py)) return FMPC_E_DIM;
        }
    // x as a spline of y needs strictly monotone y
    bool down = true, upw = true;
    for (int i = 0; i + 1 < NP; ++i) { down = down && by[i + 1] < by[i]; upw = upw && by[i + 1] > by[i]; }
    if (!down && !upw) return FMPC_E_DIM;
    std::vector<ld> sy(by), sx(bx), s;
    if (down) { std::reverse(sy.begin(), sy.end()); std::reverse(sx.begin(), sx.end()); }
    if (!dmsp_slopes(sy, sx, s)) return FMPC_E_DIM;
    if (!((ld)mech >= sy.front() && (ld)mech <= sy.back())) return FMPC_E_DIM;
    size_t at = (size_t)(std::upper_bound(sy.begin(), sy.end(), (ld)mech) - sy.begin());
    at = at == 0 ? 0 : at - 1;
    if (at > sy.size() - 2) at = sy.size() - 2;
    ld c[4];
    dmsp_piece(sy, sx, s, at, c);
    const ld tm = (ld)mech - sy[at];
    const ld scale = ((c[3] * tm + c[2]) * tm + c[1]) * tm + c[0];
    if (!std::isfinite((double)scale) || !(scale > 0.0L)) return FMPC_E_DIM;
    // the mirrored knots, as doubles; the spline through them
    std::vector<ld> u(NK), v(NK);
    for (int i = 0; i < NP; ++i) {
        const ld xs = (ld)(double)(bx[i] / scale);
        u[NP - 1 + i] = xs; v[NP - 1 + i] = by[i];
        u[NP - 1 - i] = -xs; v[NP - 1 - i] = by[i];
    }
    u[NP - 1] = 0.0L + bx[0] / scale;
    if (!dmsp_slopes(u, v, s)) return FMPC_E_DIM;                          // (false as well when the knots do not ascend)
    for (int i = 0; i < NK; ++i) breaks[i] = (double)u[i];
    for (int i = 0; i + 1 < NK; ++i) {
        dmsp_piece(u, v, s, (size_t)i, c);
        for (int k = 0; k < 4; ++k) {
            coef[4 * i + k] = (double)c[k];
            if (!std::isfinite(coef[4 * i + k])) return FMPC_E_DIM;
        }
    }
    *pieces = NK - 1;
    return FMPC_OK;
}

extern "C" int fmpc_dm_profile_eval_host(int pieces, const double* breaks, const double* coef, long long count, const double* d, double* out) {
    if (!breaks || !coef || !d || !out) return FMPC_E_NULL;
    if (pieces < 1 || pieces > FMPC_DM_MAX_PIECES || count < 0) return FMPC_E_DIM;
    for (int i = 0; i < pieces; ++i)
        if (!(breaks[i] < breaks[i + 1])) return FMPC_E_DIM;
    for (int i = 0; i < 4 * pieces; ++i)
        if (!std::isfinite(coef[i])) return FMPC_E_DIM;
    for (long long i = 0; i < count; ++i) out[i] = fmpc_dm_profile_eval(pieces, breaks, coef, d[i]);
    return FMPC_OK;
}
