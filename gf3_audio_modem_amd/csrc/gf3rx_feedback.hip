// libgf3rx -- decoder feedback: the residual channel measured on the symbols of re-encoded, trusted codewords, smoothed
// over a time x frequency window and divided out of the equalised symbols (gf3_feedback_equalise).  See DESIGN.md §12.
//
//   known(l, c) <=> all mu known bytes non-zero, eq[l, c] finite in both parts, some table entry carries the label of its
//   mu bits;  s = the first such entry;  r = eq conj(s), q = |s|^2 on known symbols, 0 elsewhere
//   W(l, c) = the (l', c') of the same packet with |l' - l| <= half_symbols and |k_c' - k_c| <= half_bins (bins)
//   A = sum_W r, B = sum_W q, n = known symbols in W;  g = A / B when n >= min_known and A != 0, else 1;  out = eq / g
//
// The rectangle is separable.  A workgroup owns FB_TL symbols x FB_TP carriers of one packet, the carriers counted in
// ascending-bin order (the context's d_bin_order / d_bins_sorted: the bin window of a carrier is a range [lo, hi) of that
// order, whatever the order of data_bins).  Phase 1: thread = one column of the tile and its halo (at most half_bins
// carriers on each side: bins are distinct); it walks the rows l0 - half_symbols .. l1 - 1 + half_symbols once, six at a
// time (the loads of a batch are issued together; a row past the end repeats the last one and counts for nothing), forms
// (r, q, known) of each from 16 bytes of eq and 2 mu bytes of bits and mask -- the label's point comes from a label ->
// point table in LDS -- and adds them to the FB_TL column sums whose window holds the row: each sum receives its rows in
// ascending order, a direct sum, no running add / subtract.  The column sums go to LDS as four planes (consecutive lanes
// read consecutive 8-byte words: no bank conflicts), sized by half_bins so that the default window leaves room for four
// workgroups per compute unit.  Phase 2: thread = (symbol, carrier); it adds the column sums of [lo, hi) in ascending
// order, forms g and writes out (and g).  Every sum has a fixed order and there are no atomics: two calls give identical
// bytes.  No workspace.
#include "gf3rx_demap.h"

namespace {

constexpr int FB_THREADS = 256;
constexpr int FB_TP = 128;                   // carriers (positions of the bin order) per workgroup
constexpr int FB_TL = 8;                     // symbols per workgroup
constexpr int FB_RB = 6;                     // rows per batch of loads (the default window's 12 rows: two batches)
constexpr int FB_MAX_HS = 8, FB_MAX_HB = 64;
static_assert(FB_TP + 2 * FB_MAX_HB <= FB_THREADS, "phase 1 gives every column of the tile and its halo one thread");
static_assert(FB_THREADS == 2 * FB_TP && FB_TL % 2 == 0, "phase 2: two symbols at a time");

struct FeedbackArgs {
    const cplx* eq; const uint8_t* bits; const uint8_t* known; cplx* out; cplx* gain;
    const int* order; const int* sbins;          // [C] carrier at a position of the bin order, its bin
    const int* idx_of_label; const int* clab; const double* cre; const double* cim;
    int D, C, hs, hb, min_known, nrc, nct;
    int W;                                       // columns of the LDS planes: FB_TP + 2 hb
    int wide;                                    // bits and known may be read mu bytes at a time (mu = 2, 4, 8, aligned)
};

// LDS: three fp64 planes and one int plane [FB_TL][W], the columns' bins [W], the label -> point table [2^mu]
inline size_t feedback_lds_bytes(int W, int mu) {
    return (size_t)FB_TL * W * (3 * sizeof(double) + sizeof(int)) + (size_t)W * sizeof(int) + ((size_t)1 << mu) * (sizeof(cplx) + sizeof(int));
}

// the label of a symbol's MU bit bytes (non-zero = 1, first byte most significant) and whether all MU mask bytes are non-zero
template <int MU>
GF3_DEV void load_label(const uint8_t* pb, const uint8_t* pk, bool wide, int& lab, bool& kn) {
    unsigned long long vb = 0, vk = 0;
    if constexpr (MU == 2 || MU == 4 || MU == 8) {
        if (wide) {
            if constexpr (MU == 2) { vb = *(const uint16_t*)pb; vk = *(const uint16_t*)pk; }
            else if constexpr (MU == 4) { vb = *(const uint32_t*)pb; vk = *(const uint32_t*)pk; }
            else { vb = *(const uint64_t*)pb; vk = *(const uint64_t*)pk; }
        } else {
#pragma unroll
            for (int b = 0; b < MU; ++b) { vb |= (unsigned long long)pb[b] << (8 * b); vk |= (unsigned long long)pk[b] << (8 * b); }
        }
    } else {
#pragma unroll
        for (int b = 0; b < MU; ++b) { vb |= (unsigned long long)pb[b] << (8 * b); vk |= (unsigned long long)pk[b] << (8 * b); }
    }
    lab = 0;
    kn = true;
#pragma unroll
    for (int b = 0; b < MU; ++b) {
        lab = (lab << 1) | (((vb >> (8 * b)) & 0xff) != 0 ? 1 : 0);
        kn = kn && ((vk >> (8 * b)) & 0xff) != 0;
    }
}

template <int MU>
__global__ __launch_bounds__(FB_THREADS) void feedback_kernel(FeedbackArgs a) {
    extern __shared__ __align__(16) double fb_lds[];
    const int W = a.W;
    double* vx = fb_lds;                         // [FB_TL][W] each
    double* vy = vx + FB_TL * W;
    double* vq = vy + FB_TL * W;
    cplx* tab = (cplx*)(vq + FB_TL * W);         // [2^MU] the first point of a label
    int* vn = (int*)(tab + (1 << MU));           // [FB_TL][W]
    int* sb = vn + FB_TL * W;                    // [W] the bins of the columns
    int* tok = sb + W;                           // [2^MU] does a point carry the label?
    const int t = threadIdx.x;
    const int C = a.C, D = a.D;
    unsigned bid = blockIdx.x;
    const int ct = (int)(bid % (unsigned)a.nct);
    bid /= (unsigned)a.nct;
    const int rc = (int)(bid % (unsigned)a.nrc);
    const int64_t f = bid / (unsigned)a.nrc;
    const int p0 = ct * FB_TP, p1 = min(p0 + FB_TP, C);
    const int l0 = rc * FB_TL, l1 = min(l0 + FB_TL, D);
    for (int lab = t; lab < (1 << MU); lab += FB_THREADS) {
        const int m = a.idx_of_label[lab];       // the first entry of that label (entry 0 when there is none)
        tab[lab] = cmk(a.cre[m], a.cim[m]);
        tok[lab] = a.clab[m] == lab ? 1 : 0;
    }
    // the tile's columns with their halo, [cb, ce) of the bin order (uniform): lane i asks about the i-th position beyond
    // each end of the tile; the bins ascend, so the positions inside the halo are the first ones and a count is enough
    int cb, ce;
    {
        const int lane = t & 63, below = p0 - 1 - lane, above = p1 + lane;
        const bool in_lo = lane < a.hb && below >= 0 && a.sbins[max(below, 0)] >= a.sbins[p0] - a.hb;
        const bool in_hi = lane < a.hb && above < C && a.sbins[min(above, C - 1)] <= a.sbins[p1 - 1] + a.hb;
        cb = p0 - __popcll(__ballot(in_lo));
        ce = p1 + __popcll(__ballot(in_hi));
    }
    const int64_t row0 = f * D;
    const int col = cb + t;
    if (col < ce) sb[t] = a.sbins[col];
    lds_barrier();                               // (the table)

    // ---- phase 1: column sums over the symbols
    if (col < ce) {
        const int c = a.order[col];
        double ax[FB_TL], ay[FB_TL], aq[FB_TL];
        int an[FB_TL];
#pragma unroll
        for (int j = 0; j < FB_TL; ++j) { ax[j] = ay[j] = aq[j] = 0.0; an[j] = 0; }
        const int r_lo = max(l0 - a.hs, 0), r_hi = min(l1 - 1 + a.hs, D - 1);
        for (int r0 = r_lo; r0 <= r_hi; r0 += FB_RB) {
            cplx e[FB_RB];
            int lab[FB_RB];
            bool kn[FB_RB];
#pragma unroll
            for (int u = 0; u < FB_RB; ++u) {
                const int64_t i = (row0 + min(r0 + u, r_hi)) * C + c;
                e[u] = a.eq[i];
                load_label<MU>(a.bits + i * MU, a.known + i * MU, a.wide != 0, lab[u], kn[u]);
            }
#pragma unroll
            for (int u = 0; u < FB_RB; ++u) {
                const int r = r0 + u;
                const bool ok = r <= r_hi && kn[u] && fabs(e[u].x) < INFINITY && fabs(e[u].y) < INFINITY && tok[lab[u]] != 0;
                const cplx s = tab[lab[u]];
                const cplx rr = cmul_conj(e[u], s);
                const double tx = ok ? rr.x : 0.0, ty = ok ? rr.y : 0.0, tq = ok ? s.x * s.x + s.y * s.y : 0.0;
                const int tn = ok ? 1 : 0;
#pragma unroll
                for (int j = 0; j < FB_TL; ++j) {
                    const bool in = r >= l0 + j - a.hs && r <= l0 + j + a.hs;
                    const double m = in ? 1.0 : 0.0;          // (the terms are finite: a sum outside the window keeps its bits)
                    ax[j] = fma(m, tx, ax[j]);
                    ay[j] = fma(m, ty, ay[j]);
                    aq[j] = fma(m, tq, aq[j]);
                    an[j] += in ? tn : 0;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < FB_TL; ++j) { vx[j * W + t] = ax[j]; vy[j * W + t] = ay[j]; vq[j * W + t] = aq[j]; vn[j * W + t] = an[j]; }
    }
    lds_barrier();

    // ---- phase 2: sums over the bin window, the gain, the output
    const int p = p0 + (t & (FB_TP - 1));
    if (p >= p1) return;
    // its bin window [lo, hi) in columns: lower bounds in the ascending bins of the tile's columns
    const int nw = ce - cb, k = sb[p - cb];
    int lo = 0, hi = 0;
    for (int step = FB_THREADS; step > 0; step >>= 1) {
        if (lo + step <= nw && sb[lo + step - 1] < k - a.hb) lo += step;
        if (hi + step <= nw && sb[hi + step - 1] <= k + a.hb) hi += step;
    }
    const int c = a.order[p];
    for (int j = t / FB_TP; j < l1 - l0; j += 2) {
        const int64_t i = (row0 + l0 + j) * C + c;
        const cplx e = a.eq[i];
        double sx = 0.0, sy = 0.0, sq = 0.0;
        int n = 0;
        for (int w = j * W + lo; w < j * W + hi; ++w) { sx += vx[w]; sy += vy[w]; sq += vq[w]; n += vn[w]; }
        const bool use = n >= a.min_known && (sx != 0.0 || sy != 0.0);
        const cplx g = use ? cmk(sx / sq, sy / sq) : cmk(1.0, 0.0);
        a.out[i] = (g.x == 1.0 && g.y == 0.0) ? e : cdiv_np(e, g);
        if (a.gain) a.gain[i] = g;
    }
}

template <int MU>
hipError_t launch_feedback(const FeedbackArgs& a, int64_t grid, hipStream_t st) {
    return launch(feedback_kernel<MU>, grid, FB_THREADS, feedback_lds_bytes(a.W, MU), st, a);
}

}  // namespace

extern "C" int64_t gf3_feedback_workspace_bytes(const gf3_ctx* c, int64_t F) {
    (void)c; (void)F;
    return 0;                                               // one launch: the column sums live in LDS
}

extern "C" int gf3_feedback_equalise(gf3_ctx* c, const void* d_eq, const uint8_t* d_bits, const uint8_t* d_known, int64_t F,
                                     int32_t half_symbols, int32_t half_bins, int32_t min_known, void* d_out, void* d_gain,
                                     void* d_work, int64_t work_bytes, void* stream) {
    (void)d_work;
    DeviceGuard dg(c);
    if (!c) return fail(c, GF3_EINVAL, "gf3_feedback_equalise: bad argument (no context)");
    if (F < 0) return fail(c, GF3_EINVAL, "gf3_feedback_equalise: F < 0");
    if (half_symbols < 0 || half_symbols > FB_MAX_HS || half_bins < 0 || half_bins > FB_MAX_HB || min_known < 1)
        return fail(c, GF3_EINVAL, "gf3_feedback_equalise: need 0 <= half_symbols <= 8, 0 <= half_bins <= 64, min_known >= 1");
    if (work_bytes < gf3_feedback_workspace_bytes(c, F)) return fail(c, GF3_EINVAL, "gf3_feedback_equalise: workspace too small");
    if (c->cfg.C > 4096) return fail(c, GF3_EINVAL, "gf3_feedback_equalise: C <= 4096");
    if (F == 0) return GF3_OK;
    if (!d_eq || !d_bits || !d_known || !d_out) return fail(c, GF3_EINVAL, "gf3_feedback_equalise: bad argument (null pointer)");
    if (d_out == d_eq) return fail(c, GF3_EINVAL, "gf3_feedback_equalise: d_out must not be d_eq (neighbours are still being read)");
    const int D = c->cfg.D, C = c->cfg.C;
    const int nrc = (D + FB_TL - 1) / FB_TL, nct = (C + FB_TP - 1) / FB_TP;
    if (F > (int64_t)0x7fffffff / ((int64_t)nrc * nct))
        return fail(c, GF3_EINVAL, "gf3_feedback_equalise: too many packets per call (F ceil(D / 8) ceil(C / 128) < 2^31)");
    const int mu = c->cfg.mu;
    const bool wide = (mu == 2 || mu == 4 || mu == 8) && ((uintptr_t)d_bits | (uintptr_t)d_known) % (uintptr_t)mu == 0;
    FeedbackArgs a{(const cplx*)d_eq, d_bits, d_known, (cplx*)d_out, (cplx*)d_gain, c->d_bin_order, c->d_bins_sorted,
                   c->d_idx_of_label, c->d_clab, c->d_cre, c->d_cim, D, C, half_symbols, half_bins, min_known, nrc, nct,
                   FB_TP + 2 * half_bins, wide ? 1 : 0};
    const int64_t grid = F * nrc * nct;
    hipStream_t st = (hipStream_t)stream;
    switch (mu) {
        case 1: HIPCHK(c, launch_feedback<1>(a, grid, st)); break;
        case 2: HIPCHK(c, launch_feedback<2>(a, grid, st)); break;
        case 3: HIPCHK(c, launch_feedback<3>(a, grid, st)); break;
        case 4: HIPCHK(c, launch_feedback<4>(a, grid, st)); break;
        case 5: HIPCHK(c, launch_feedback<5>(a, grid, st)); break;
        case 6: HIPCHK(c, launch_feedback<6>(a, grid, st)); break;
        case 7: HIPCHK(c, launch_feedback<7>(a, grid, st)); break;
        case 8: HIPCHK(c, launch_feedback<8>(a, grid, st)); break;
        default: return fail(c, GF3_EINVAL, "gf3_feedback_equalise: 1 <= mu <= 8");
    }
    return GF3_OK;
}
