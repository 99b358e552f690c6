// Per-symbol arithmetic of the soft demappers, shared by the stand-alone kernels (gf3rx_demap.hip: gf3_soft_demap, and
// through it gf3_soft_demap_csi), the noise-weighted path (gf3rx_noise.hip) and its form for a QAM order per carrier
// (gf3rx_loading.hip): squared distances to the table and the
// max-log difference  min over points with bit = 1 of d^2  -  min over points with bit = 0 of d^2  per label bit.  The
// callers scale the difference (1 / noise_var, or the per-carrier weight) and round it to float32.
#pragma once
#include "gf3rx_host.h"

// The constellation table as the kernels see it (device pointers of the context; SepTab by value).
struct DemapTab {
    int M, mu;
    const double* cre; const double* cim; const int* clab;
    SepTab sep;
};
inline DemapTab demap_tab(const gf3_ctx* c) { return DemapTab{c->cfg.M, c->cfg.mu, c->d_cre, c->d_cim, c->d_clab, c->sep}; }

// Is the separable table of the kind every square Gray QAM generator produces (and the reference's QPSK): 2^HI x 2^HQ
// grid, the first HI label bits the binary index of the I level in `lvI`, the last HQ bits that of the Q level?
inline bool sep_is_binary(const SepTab& sp, int mu, int& hI, int& hQ) {
    hI = hQ = 0;
    while ((1 << hI) < sp.nI) ++hI;
    while ((1 << hQ) < sp.nQ) ++hQ;
    if (sp.nI < 2 || sp.nQ < 2 || (1 << hI) != sp.nI || (1 << hQ) != sp.nQ || hI + hQ != mu || hI != hQ) return false;
    if (sp.maskI != (((1 << hI) - 1) << hQ)) return false;
    for (int k = 0; k < sp.nI; ++k) if (sp.labI[k] != (k << hQ)) return false;
    for (int k = 0; k < sp.nQ; ++k) if (sp.labQ[k] != k) return false;
    return true;
}

// binary-indexed grid up to 64-QAM -> its HI, anything else -> 0 (as run_demap chooses its kernels)
inline int grid_bits(const gf3_ctx* c) {
    int hI = 0, hQ = 0;
    return (c->sep.nI > 0 && sep_is_binary(c->sep, c->cfg.mu, hI, hQ) && hI <= 3) ? hI : 0;
}

// HI > 0: binary-indexed 2^HI x 2^HI grid (levels in registers); HI == 0: any table (literal scan).
template <int HI>
struct Levels {
    double lvI[1 << HI], lvQ[1 << HI];
    GF3_DEV explicit Levels(const DemapTab& t) {
#pragma unroll
        for (int k = 0; k < (1 << HI); ++k) { lvI[k] = t.sep.lvI[k]; lvQ[k] = t.sep.lvQ[k]; }
    }
};

// squared distances of one component to the N levels of its axis
template <int N>
GF3_DEV void axis_d2(double x, const double (&lv)[N], double (&d)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) { const double t = x - lv[k]; d[k] = t * t; }
}

// Any table: dst[b] = (float)((m1 - m0) * scale) for b < mu.  A separable table needs the owning axis' levels only (the
// other axis' term cancels in the difference); everything else scans the M points.
GF3_DEV void maxlog_table(cplx e, const DemapTab& t, double scale, float* dst) {
    double m0[8], m1[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) m0[b] = m1[b] = INFINITY;
    if (t.sep.nI > 0) {
        for (int k = 0; k < t.sep.nI; ++k) {
            const double d = (e.x - t.sep.lvI[k]) * (e.x - t.sep.lvI[k]);
            const int lab = t.sep.labI[k];
#pragma unroll
            for (int b = 0; b < 8; ++b)
                if (b < t.mu && ((t.sep.maskI >> (t.mu - 1 - b)) & 1)) {
                    if ((lab >> (t.mu - 1 - b)) & 1) m1[b] = fmin(m1[b], d); else m0[b] = fmin(m0[b], d);
                }
        }
        for (int k = 0; k < t.sep.nQ; ++k) {
            const double d = (e.y - t.sep.lvQ[k]) * (e.y - t.sep.lvQ[k]);
            const int lab = t.sep.labQ[k];
#pragma unroll
            for (int b = 0; b < 8; ++b)
                if (b < t.mu && !((t.sep.maskI >> (t.mu - 1 - b)) & 1)) {
                    if ((lab >> (t.mu - 1 - b)) & 1) m1[b] = fmin(m1[b], d); else m0[b] = fmin(m0[b], d);
                }
        }
    } else {
        for (int c = 0; c < t.M; ++c) {
            const double dx = e.x - t.cre[c], dy = e.y - t.cim[c];
            const double d = dx * dx + dy * dy;
            const int lab = t.clab[c];
#pragma unroll
            for (int b = 0; b < 8; ++b)
                if (b < t.mu) { if ((lab >> (t.mu - 1 - b)) & 1) m1[b] = fmin(m1[b], d); else m0[b] = fmin(m0[b], d); }
        }
    }
#pragma unroll
    for (int b = 0; b < 8; ++b)
        if (b < t.mu) dst[b] = (float)((m1[b] - m0[b]) * scale);
}

// Binary-indexed 2^HI x 2^HQ grid: which levels carry a 1 in which bit is known at compile time, so the whole reduction
// is straight-line v_min_f64 -- no scalar bit tests, no branches.
template <int HI, int HQ>
GF3_DEV void maxlog_bin(cplx e, const double (&lvI)[1 << HI], const double (&lvQ)[1 << HQ], double (&diff)[HI + HQ]) {
    constexpr int NI = 1 << HI, NQ = 1 << HQ;
    double dI[NI], dQ[NQ];
    axis_d2<NI>(e.x, lvI, dI);
    axis_d2<NQ>(e.y, lvQ, dQ);
#pragma unroll
    for (int b = 0; b < HI; ++b) {                 // label bit b = bit (HI - 1 - b) of the I index
        double m0 = INFINITY, m1 = INFINITY;
#pragma unroll
        for (int k = 0; k < NI; ++k) { if ((k >> (HI - 1 - b)) & 1) m1 = fmin(m1, dI[k]); else m0 = fmin(m0, dI[k]); }
        diff[b] = m1 - m0;
    }
#pragma unroll
    for (int b = 0; b < HQ; ++b) {
        double m0 = INFINITY, m1 = INFINITY;
#pragma unroll
        for (int k = 0; k < NQ; ++k) { if ((k >> (HQ - 1 - b)) & 1) m1 = fmin(m1, dQ[k]); else m0 = fmin(m0, dQ[k]); }
        diff[HI + b] = m1 - m0;
    }
}

// MU float32 LLRs of symbol i, as wide as the row's alignment allows
template <int MU>
GF3_DEV void store_llr(float* llr, int64_t i, const float (&out)[MU]) {
    if constexpr (MU % 4 == 0) {                      // 16-byte aligned rows
#pragma unroll
        for (int b = 0; b < MU; b += 4) *(float4*)(llr + i * MU + b) = make_float4(out[b], out[b + 1], out[b + 2], out[b + 3]);
    } else if constexpr (MU % 2 == 0) {               // 8-byte aligned rows
#pragma unroll
        for (int b = 0; b < MU; b += 2) *(float2*)(llr + i * MU + b) = make_float2(out[b], out[b + 1]);
    } else {
#pragma unroll
        for (int b = 0; b < MU; ++b) llr[i * MU + b] = out[b];
    }
}

// The reference's channel magnitude at data symbol l of a packet (OFDM.py:469), from the magnitudes s = |Hs| and e = |He|
// of the two pilot blocks' estimates on a carrier: the CSI weight is its square (csi_weight_kernel, combine_kernel).
GF3_DEV double csi_mag(double s, double e, int l, int P, int D) {
    return s + (e - s) * (l + P / 2.0) / (double)(D + P);
}

// Squared distance to the point the hard decision picks: in-order scan with strict `<`, so a NaN symbol keeps point 0
// (and a NaN distance).  On a grid table the minimum over the points is the sum of the two axes' minima, exactly:
// rounding is monotonic, so min_k a_k + min_j b_j and min_kj (a_k + b_j) are the same number.
template <int N>
GF3_DEV double axis_min_d2(double x, const double (&lv)[N]) {
    double d[N];
    axis_d2<N>(x, lv, d);
    double bd = d[0];
#pragma unroll
    for (int k = 1; k < N; ++k) if (d[k] < bd) bd = d[k];
    return bd;
}
GF3_DEV double table_min_d2(cplx e, const double* cre, const double* cim, int M) {
    double dx = e.x - cre[0], dy = e.y - cim[0];
    double bd = dx * dx + dy * dy;
    for (int c = 1; c < M; ++c) {
        dx = e.x - cre[c]; dy = e.y - cim[c];
        const double d = dx * dx + dy * dy;
        if (d < bd) bd = d;
    }
    return bd;
}
