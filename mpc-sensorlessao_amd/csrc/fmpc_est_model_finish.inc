// Body of the finish kernel of the linearised image model, included by fmpc_est_model_finish and fer_finish as
// fmpc_est_model_psf.inc is.  The including kernel defines: a FemParams P (part, base, A_s, b_s as this workgroup is to use
// them), f, slot, k (the diversity).  One workgroup of 1024 threads: the partial windows summed in a fixed order; field 0 leaves
// I_k in P.base and b_s, field 1 + j column j of A_s.
    const int tid = threadIdx.x;
    const int d = P.d, nblk = P.len / 16, dd = d * d;
    const size_t p = (size_t)P.ndiv * dd;
    const int v = tid & 31, u = tid >> 5;                    // window column (consecutive lanes read consecutive doubles), row
    if (u >= d || v >= d) return;
    const double* src = P.part + (((size_t)slot * P.ndiv + k) * nblk) * 2048 + u * 32 + v;
    double orr = 0.0, oi = 0.0;                              // fixed order (nblk is a multiple of 4)
    int b = 0;
    for (; b + 8 <= nblk; b += 8) {
        double re[8], im[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { re[j] = src[(size_t)(b + j) * 2048]; im[j] = src[(size_t)(b + j) * 2048 + 1024]; }
        orr += ((re[0] + re[1]) + (re[2] + re[3])) + ((re[4] + re[5]) + (re[6] + re[7]));
        oi += ((im[0] + im[1]) + (im[2] + im[3])) + ((im[4] + im[5]) + (im[6] + im[7]));
    }
    for (; b < nblk; b += 4) {
        double re[4], im[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { re[j] = src[(size_t)(b + j) * 2048]; im[j] = src[(size_t)(b + j) * 2048 + 1024]; }
        orr += (re[0] + re[1]) + (re[2] + re[3]);
        oi += (im[0] + im[1]) + (im[2] + im[3]);
    }
    const size_t idx = (size_t)k * dd + v * d + u;           // reshape(v_im(:,:,k), [], 1): column-major
    double* I = P.base + (size_t)k * 2048 + u * 32 + v;
    if (f == 0) {
        I[0] = orr; I[1024] = oi;
        P.b_s[idx] = (orr * orr + oi * oi) * P.scale;
    } else {
        P.A_s[(size_t)(f - 1) * p + idx] = 2.0 * P.scale * (I[0] * orr + I[1024] * oi);
    }
