// Body of the PSF kernel of the linearised image model, included by fmpc_est_model_psf (fmpc_kernel_est_model.hip: one operating
// point) and fer_psf (fmpc_kernel_est_refine.hip: one per realisation) inside their own braces, so that each kernel compiles the
// very text it compiled before.  The including kernel defines: the template flag PHI, a FemParams P (phi0, part as this
// workgroup is to use them), f (the field: 0 = P_k, 1 + j = 1i Z_j P_k), slot, blk (the 16-row block), nblk.
// One workgroup of FEM_NW wavefronts.
    __shared__ double sTd[FEM_NW * FE_TSTRIDE];               // [NW][2][16][33]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, c = lane & 15;
    const int len = P.len;
    const int y0 = 16 * blk;
    const size_t npx = (size_t)len * len;
    const double* zmap = P.Z + (size_t)(f > 0 ? f - 1 : 0) * npx;          // (field 0 loads map 0 and does not use it)
    d4e TA[FE_MAXDIV][2], TB[FE_MAXDIV][2], TC[FE_MAXDIV][2];
#pragma unroll
    for (int k = 0; k < FE_MAXDIV; ++k)
#pragma unroll
        for (int t = 0; t < 2; ++t) { TA[k][t] = (d4e){0, 0, 0, 0}; TB[k][t] = (d4e){0, 0, 0, 0}; TC[k][t] = (d4e){0, 0, 0, 0}; }
    // ---- T_k += X_k F over this wavefront's columns.  Lane (g, c): pixel (row y0 + c, column 4 Q + g) of the A operand,
    //      entry (k-row 4 Q + g, window column 16 t + c) of the B operand; loads one k-step ahead, as in fmpc_est_psf.
    const int qlo = P.qrange[2 * blk], cnt = P.qrange[2 * blk + 1] - qlo;
    const int i0 = (int)((long long)cnt * wv / FEM_NW), i1 = (int)((long long)cnt * (wv + 1) / FEM_NW), nq = i1 - i0;
    const int Q0 = qlo + i0;
    double ph_n = 0.0, z_n, dr_n[FE_MAXDIV], di_n[FE_MAXDIV], f_n[4];
    {
        const size_t px = (size_t)(4 * Q0 + g) * len + (y0 + c);
        if (PHI) ph_n = P.phi0[px];
        z_n = zmap[px];
#pragma unroll
        for (int k = 0; k < FE_MAXDIV; ++k) { const size_t o = (size_t)(k < P.ndiv ? k : 0) * npx + px; dr_n[k] = P.Dre[o]; di_n[k] = P.Dim[o]; }
        const double* fp = P.Fimg + (size_t)Q0 * 256 + lane;
        f_n[0] = fp[0]; f_n[1] = fp[64]; f_n[2] = fp[128]; f_n[3] = fp[192];
    }
    for (int q = 0; q < nq; ++q) {
        const double ph = ph_n, z = z_n, fr0 = f_n[0], fi0 = f_n[1], fr1 = f_n[2], fi1 = f_n[3];
        double dr[FE_MAXDIV], di[FE_MAXDIV];
#pragma unroll
        for (int k = 0; k < FE_MAXDIV; ++k) { dr[k] = dr_n[k]; di[k] = di_n[k]; }
        {
            const int Qn = Q0 + (q + 1 < nq ? q + 1 : q);
            const size_t px = (size_t)(4 * Qn + g) * len + (y0 + c);
            if (PHI) ph_n = P.phi0[px];
            z_n = zmap[px];
#pragma unroll
            for (int k = 0; k < FE_MAXDIV; ++k) { const size_t o = (size_t)(k < P.ndiv ? k : 0) * npx + px; dr_n[k] = P.Dre[o]; di_n[k] = P.Dim[o]; }
            const double* fp = P.Fimg + (size_t)Qn * 256 + lane;
            f_n[0] = fp[0]; f_n[1] = fp[64]; f_n[2] = fp[128]; f_n[3] = fp[192];
        }
        double sn = 0.0, co = 1.0;
        if (PHI) fe_sincos(ph, sn, co);
        const double fs0 = fr0 + fi0, fs1 = fr1 + fi1;
#pragma unroll
        for (int k = 0; k < FE_MAXDIV; ++k) {
            if (k < P.ndiv) {                                    // (uniform)
                const double br = PHI ? co * dr[k] - sn * di[k] : dr[k], bi = PHI ? co * di[k] + sn * dr[k] : di[k];
                const double pr = f > 0 ? -z * bi : br, pi = f > 0 ? z * br : bi, ps = pr + pi;      // 1i Z_j P_k, or P_k
                TA[k][0] = FE_MFMA(pr, fr0, TA[k][0]); TB[k][0] = FE_MFMA(pi, fi0, TB[k][0]); TC[k][0] = FE_MFMA(ps, fs0, TC[k][0]);
                TA[k][1] = FE_MFMA(pr, fr1, TA[k][1]); TB[k][1] = FE_MFMA(pi, fi1, TB[k][1]); TC[k][1] = FE_MFMA(ps, fs1, TC[k][1]);
            }
        }
    }
    // ---- per diversity: the partial T of the wavefronts meet in LDS; O = F_blk' T, wavefront w the tile (w / 2, w % 2)
    const int tu = (wv >> 1) & 1, tv = wv & 1;
    double far[4], fai[4];                                   // A operand of the second product: F[y0 + 4 q2 + g][16 tu + c]
#pragma unroll
    for (int q2 = 0; q2 < 4; ++q2) {
        const double* fp = P.Fimg + (size_t)(y0 / 4 + q2) * 256 + tu * 128 + lane;
        far[q2] = fp[0]; fai[q2] = fp[64];
    }
    for (int k = 0; k < P.ndiv; ++k) {
        __syncthreads();                                     // sT free again
#pragma unroll
        for (int kk = 0; kk < FE_MAXDIV; ++kk) {
            if (kk == k) {                                   // (uniform; static register indices)
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {          // register rr <-> row 4 rr + g, column 16 t + c
                        sTd[wv * FE_TSTRIDE + (4 * rr + g) * 33 + 16 * t + c] = TA[kk][t][rr] - TB[kk][t][rr];
                        sTd[wv * FE_TSTRIDE + 528 + (4 * rr + g) * 33 + 16 * t + c] = (TC[kk][t][rr] - TA[kk][t][rr]) - TB[kk][t][rr];
                    }
            }
        }
        __syncthreads();
        d4e Or = {0, 0, 0, 0}, Oi = {0, 0, 0, 0};
#pragma unroll
        for (int q2 = 0; q2 < 4; ++q2) {
            // B operand: T[4 q2 + g][16 tv + c], summed over the wavefronts in a fixed order
            const double* b4 = sTd + (4 * q2 + g) * 33 + 16 * tv + c;
            const double tr = (b4[0] + b4[FE_TSTRIDE]) + (b4[2 * FE_TSTRIDE] + b4[3 * FE_TSTRIDE]);
            const double ti = (b4[528] + b4[FE_TSTRIDE + 528]) + (b4[2 * FE_TSTRIDE + 528] + b4[3 * FE_TSTRIDE + 528]);
            const double nfai = -fai[q2];
            Or = FE_MFMA(far[q2], tr, Or); Or = FE_MFMA(nfai, ti, Or);
            Oi = FE_MFMA(far[q2], ti, Oi); Oi = FE_MFMA(fai[q2], tr, Oi);
        }
        // partial window of these 16 rows: [slot][k][blk][re, im][32][32], register rr <-> row 16 tu + 4 rr + g, column 16 tv + c
        double* dst = P.part + (((size_t)slot * P.ndiv + k) * nblk + blk) * 2048;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int o = (16 * tu + 4 * rr + g) * 32 + 16 * tv + c;
            dst[o] = Or[rr]; dst[1024 + o] = Oi[rr];
        }
    }
