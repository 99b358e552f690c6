// The soft-output arithmetic of the library, stated once.  Every kernel that turns an equalised symbol into a decision
// distance or into LLRs calls these pieces: the stand-alone demappers (gf3rx_demap.hip), the noise-weighted paths
// (gf3rx_noise.hip), bit loading (gf3rx_loading.hip), diversity combining (gf3rx_combine.hip), phase tracking
// (gf3rx_track.hip) and the fused demodulator's soft mode (soft_llr, gf3rx_demod.h).  See DESIGN.md §12, "The shared
// soft-output pieces".
//   device: squared distances to the table and the max-log difference
//             min over points with bit = 1 of d^2  -  min over points with bit = 0 of d^2          (maxlog_bin, maxlog_table)
//           the weighted emitter: differences x weight in fp64, rounded to float32 once             (emit_llr, emit_grid_llr)
//           the decided point and its distance: in-order scan, strict <                             (nearest_point, nearest_d2)
//           a packet's mean variance, the weight rule, the CSI weight                               (packet_vbar, noise_weight, csi_weight)
//   host:   table class -> compile-time HI                                                          (grid_bits, with_grid_bits)
#pragma once
#include <type_traits>
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

// binary-indexed grid up to 64-QAM -> its HI, anything else -> 0
inline int grid_bits(const gf3_ctx* c) {
    int hI = 0, hQ = 0;
    return (c->sep.nI > 0 && sep_is_binary(c->sep, c->cfg.mu, hI, hQ) && hI <= 3) ? hI : 0;
}
// The one place where a context's table class becomes a template argument: fn(std::integral_constant<int, HI>) for the
// context's HI, its result handed back.  A kernel family with an HI parameter is launched through this and nothing else.
template <typename Fn>
inline auto with_grid_bits(const gf3_ctx* c, Fn&& fn) {
    switch (grid_bits(c)) {
        case 1: return fn(std::integral_constant<int, 1>{});
        case 2: return fn(std::integral_constant<int, 2>{});
        case 3: return fn(std::integral_constant<int, 3>{});
        default: return fn(std::integral_constant<int, 0>{});
    }
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

// ---- the weighted emitter ------------------------------------------------------------------------------------------
// One symbol's LLRs: out[b] = (float)(diff[b] * w), the product in fp64, rounded once; `store` gets the floats and puts
// them where the caller keeps them (store_llr, the loaded path's 8-byte-aligned store, the de-interleaving scatter, the
// fused kernel's LDS row).  ERASE is the site's rule for w == 0.0, a compile-time choice:
//   ERASE = true   +0.0f whatever the symbol held.  The sites whose weight comes from a noise estimate or from combining
//                  (soft_demap_nw, soft_demap_nw_cs, combine, soft_demap_loaded): there w == 0 MARKS an erasure -- a
//                  variance or a symbol that is not finite -- and diff may be NaN or infinite, so diff * 0 would put a
//                  NaN, and a negative diff a -0, where the decoder must read "no information".
//   ERASE = false  diff * w as it comes.  The sites whose weight is a plain scale (soft_demap_bin_kernel: 1 / noise_var,
//                  never 0 for an accepted call; soft_llr: |H^|^2, 0 only where the channel estimate is 0): nothing is
//                  marked there, and a non-finite symbol shows as a non-finite LLR, as it does with any other weight.
template <int HI, int HQ, bool ERASE, typename Store>
GF3_DEV void emit_grid_llr(cplx e, const double (&lvI)[1 << HI], const double (&lvQ)[1 << HQ], double w, Store&& store) {
    double diff[HI + HQ];
    maxlog_bin<HI, HQ>(e, lvI, lvQ, diff);
    float out[HI + HQ];
#pragma unroll
    for (int b = 0; b < HI + HQ; ++b) out[b] = (ERASE && w == 0.0) ? 0.0f : (float)(diff[b] * w);
    store(out);
}
// The same for the table class HI of with_grid_bits: float[2 HI] on a grid, float[8] with t.mu of them valid for any table.
template <int HI, bool ERASE, typename Store>
GF3_DEV void emit_llr(cplx e, const Levels<HI>& lv, const DemapTab& t, double w, Store&& store) {
    static_assert(HI <= 3, "the stores read a float[8] as `any table`: grid_bits stops at 64-QAM");
    if constexpr (HI > 0) {
        emit_grid_llr<HI, HI, ERASE>(e, lv.lvI, lv.lvQ, w, store);
    } else {
        float out[8];
#pragma unroll
        for (int b = 0; b < 8; ++b) out[b] = 0.0f;
        if (!ERASE || w != 0.0) maxlog_table(e, t, w, out);
        store(out);
    }
}
// the usual store: symbol i of an [n][mu] array (emit_llr's float[2 HI] or float[8])
template <int N>
GF3_DEV void store_llr_any(float* llr, int64_t i, int mu, const float (&out)[N]) {
    if constexpr (N < 8) store_llr<N>(llr, i, out);
    else {
        float* dst = llr + i * mu;
#pragma unroll
        for (int b = 0; b < 8; ++b)
            if (b < mu) dst[b] = out[b];
    }
}

// The reference's channel magnitude at data symbol l of a packet (OFDM.py:469), from the magnitudes s = |Hs| and e = |He|
// of the two pilot blocks' estimates on a carrier: the CSI weight is its square.
GF3_DEV double csi_mag(double s, double e, int l, int P, int D) {
    return s + (e - s) * (l + P / 2.0) / (double)(D + P);
}
// the CSI weight from the two magnitudes (kernels that keep them per carrier across symbols) and from the estimates
GF3_DEV double csi_weight_mag(double s, double e, int l, int P, int D) {
    const double mag = csi_mag(s, e, l, P, D);
    return mag * mag;
}
GF3_DEV double csi_weight(cplx hs, cplx he, int l, int P, int D) {
    return csi_weight_mag(hypot(hs.x, hs.y), hypot(he.x, he.y), l, P, D);
}

// neither NaN nor infinite: what lets a value into a weighted sum (combining, the joint detectors of gf3rx_joint.h)
GF3_DEV bool is_fin(double x) { return fabs(x) < INFINITY; }

// ---- noise weights ---------------------------------------------------------------------------------------------------
// A packet's mean variance from the 256 threads' partial sums: a binary tree in LDS (red[256], barriers included), the
// same number in every workgroup that adds the same partials.  What a thread's partial holds is the caller's matter
// (v[t] + v[t + 256] + ... in ascending order; all branches' such sums, b ascending, when combining); n is the number of
// variances added.  flat: vbar is 0, NaN or Inf -- the packet's weights are 1.
constexpr int VBAR_THREADS = 256;
struct PacketNoise { double vbar; bool flat; double floor_v; };
GF3_DEV PacketNoise packet_vbar(double* red, double partial, double n) {
    const int t = threadIdx.x;
    red[t] = partial;
    __syncthreads();
#pragma unroll
    for (int h = VBAR_THREADS / 2; h > 0; h >>= 1) {
        if (t < h) red[t] += red[t + h];
        __syncthreads();
    }
    const double vbar = red[0] / n;
    return PacketNoise{vbar, !(vbar > 0.0) || !(vbar < INFINITY), 1e-6 * vbar};
}
// The weight rule: 0 where the variance is not finite (an erasure), 1 in a flat packet, else 1 / max(x, 1e-6 vbar).
GF3_DEV double noise_weight(double x, const PacketNoise& p) {
    return !(fabs(x) < INFINITY) ? 0.0 : p.flat ? 1.0 : 1.0 / fmax(x, p.floor_v);
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
// ... and the point itself
template <int N>
GF3_DEV double axis_nearest(double x, const double (&lv)[N]) {
    double t = x - lv[0], bd = t * t, bl = lv[0];
#pragma unroll
    for (int k = 1; k < N; ++k) {
        t = x - lv[k];
        const double d = t * t;
        if (d < bd) { bd = d; bl = lv[k]; }
    }
    return bl;
}
GF3_DEV cplx table_nearest(cplx e, const double* cre, const double* cim, int M) {
    cplx p = cmk(cre[0], cim[0]);
    double dx = e.x - p.x, dy = e.y - p.y;
    double bd = dx * dx + dy * dy;
    for (int c = 1; c < M; ++c) {
        const cplx q = cmk(cre[c], cim[c]);
        dx = e.x - q.x; dy = e.y - q.y;
        const double d = dx * dx + dy * dy;
        if (d < bd) { bd = d; p = q; }
    }
    return p;
}
// both for the table class HI of with_grid_bits (grid_min_d2: a grid whose levels the caller holds)
template <int N>
GF3_DEV double grid_min_d2(cplx e, const double (&lvI)[N], const double (&lvQ)[N]) {
    return axis_min_d2<N>(e.x, lvI) + axis_min_d2<N>(e.y, lvQ);
}
template <int HI>
GF3_DEV double nearest_d2(cplx e, const Levels<HI>& lv, const DemapTab& t) {
    if constexpr (HI > 0) return grid_min_d2<(1 << HI)>(e, lv.lvI, lv.lvQ);
    else return table_min_d2(e, t.cre, t.cim, t.M);
}
template <int HI>
GF3_DEV cplx nearest_point(cplx e, const Levels<HI>& lv, const DemapTab& t) {
    if constexpr (HI > 0) return cmk(axis_nearest<(1 << HI)>(e.x, lv.lvI), axis_nearest<(1 << HI)>(e.y, lv.lvQ));
    else return table_nearest(e, t.cre, t.cim, t.M);
}
