// libgf3rx -- transmit diversity, two speakers and one microphone or more: the Alamouti space-time block code over pairs of
// data symbols.  The joint phase slope of the covered pilot estimates (gf3_stbc_slope) and the joint max-log ML detector of
// a pair (gf3_stbc_detect).  Not in the reference; see include/gf3rx.h and DESIGN.md §12.
//
// Wire format: chirps, pilots and cover as gf3rx_mimo.hip states them, so gf3_mimo_pilots gives both columns H_b0, H_b1 of
// every microphone.  The data of ONE stream goes out in pairs: with x0, x1 the carrier's points of symbols a = 2j and
// b' = 2j + 1, speaker 0 sends x0 then -conj(x1), speaker 1 sends x1 then conj(x0), so at microphone b
//   y_a = h0(a) x0 + h1(a) x1,      conj(y_b') = conj(h1(b')) x0 - conj(h0(b')) x1.
//
// stbc_slope_kernel<B>: one workgroup per packet, 256 threads.  d[k] = sum_b sum_t conj(Hs_bt[k]) He_bt[k] over the fit
//   range, its angle to LDS (atan2_fast), then the demodulator's fit on ONE angle series: with c_n the cumulative unwrap
//   corrections (unwrap_corr), sum_n xm_n c_n = sum_i e_i j (L - j) / 2 (gf3rx_demod.h), so no prefix scan.  block_sum
//   adds the threads' parts in a fixed order.
// stbc_detect_kernel<B>: mimo_detect_kernel<B>'s shape -- a workgroup owns 256 consecutive data carriers x Jc consecutive
//   symbol PAIRS of one packet; thread = carrier.  The 2 B magnitudes at both pilot blocks and the 2 B phasors stay in
//   registers; ONE slope serves every branch, so one step advances them all, one complex multiply per entry and symbol.
//   Per pair a thread reads B x 32 bytes of Y and writes 16.  Every sum runs in a fixed order, no atomics: two runs give
//   identical bytes.  NW (gf3_stbc_detect_nw): mimo_detect_kernel's weights -- one per branch and carrier, in a register
//   ahead of the pair loop, on that branch's term of every sum at both slots; 0 or not finite takes the branch out.
#include "gf3rx_joint.h"

namespace {

// ------------------------------------------------------------------------------------------------------------ slope
constexpr int ST_THREADS = 256;

struct StbcSlopeArgs {
    const cplx* H[GF3_MAX_BRANCHES];        // [F][2][2][K]
    double* slope;                          // [F]
    int K, fit_lo, fit_hi;
    double xbar, inv_sxx;
};

template <int B>
__global__ __launch_bounds__(ST_THREADS) void stbc_slope_kernel(StbcSlopeArgs a) {
    extern __shared__ double sl_lds[];
    const int tid = threadIdx.x, K = a.K;
    const int64_t f = blockIdx.x;
    const int L = a.fit_hi - a.fit_lo;
    double* scratch = sl_lds;               // [8] block_sum's partials
    double* q = sl_lds + 8;                 // [L] angle of d at carrier fit_lo + j
    double bad = 0.0;
    for (int j = tid; j < L; j += ST_THREADS) {
        const int k = a.fit_lo + j;
        cplx d = cmk(0.0, 0.0);
#pragma unroll
        for (int b = 0; b < B; ++b) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const cplx hs = a.H[b][((f * 2 + 0) * 2 + t) * K + k];
                const cplx he = a.H[b][((f * 2 + 1) * 2 + t) * K + k];
                d = cadd(d, cmul_conj(he, hs));             // conj(Hs) He
            }
        }
        if (!(is_fin(d.x) && is_fin(d.y))) bad = 1.0;
        q[j] = atan2_fast(d.y, d.x);
    }
    bad = block_sum(bad, scratch);          // (its barriers: every angle is in LDS)
    double acc = 0.0;
    for (int j = tid; j < L; j += ST_THREADS) {
        acc += ((double)j - a.xbar) * q[j];
        if (j > 0) acc += unwrap_corr(q[j] - q[j - 1]) * (0.5 * (double)j * (double)(L - j));
    }
    const double slope = block_sum(acc, scratch) * a.inv_sxx;
    if (tid == 0) a.slope[f] = bad > 0.0 ? (double)NAN : slope;
}

// ------------------------------------------------------------------------------------------------------------ detector
struct StbcDetectArgs {
    const cplx* Y[GF3_MAX_BRANCHES];        // [F*D][NB]
    const cplx* H[GF3_MAX_BRANCHES];        // [F][2][2][K]
    const double* slope;                    // [F]
    float* llr;                             // [F][D][C][2]
    const int* bins;                        // [C] 1-based FFT bin of each data carrier
    int D, C, K, NB, P, Jc, ntile;
    const double* cre; const double* cim; const int* clab;      // the 4 points and their labels
    const double* wgt;                      // NW: [B][F][C] the branches' weights (gf3_joint_noise_weights)
};

template <int B, bool NW>
__global__ __launch_bounds__(JOINT_THREADS) void stbc_detect_kernel(StbcDetectArgs a) {
    const int t = threadIdx.x;
    const int tile = blockIdx.x % a.ntile, chunk = blockIdx.x / a.ntile;
    const int64_t f = blockIdx.y;
    const int c = tile * JOINT_THREADS + t;
    if (c >= a.C) return;
    const int bin = a.bins[c];
    const int D = a.D, P = a.P;
    const int j0 = chunk * a.Jc, j1 = min(j0 + a.Jc, D / 2);
    const double n = (double)(bin - 1);
    const double sl = a.slope[f];
    const bool oks = is_fin(sl);
    const cplx rot = cis_fast(sl * n * ((2 * j0 + P / 2.0) / (double)(D + P)));
    const cplx step = cis_fast(sl * n / (double)(D + P));
    // per-carrier state of the 2 B entries: |Hs|, |He| and the phasor at symbol 2 j0
    double ms[B][2], me[B][2];
    cplx w[B][2];
    bool okh[B];
    double wt[B];
#pragma unroll
    for (int b = 0; b < B; ++b) {
        okh[b] = oks;
        wt[b] = 1.0;
        if constexpr (NW) {
            wt[b] = a.wgt[((int64_t)b * gridDim.y + f) * a.C + c];
            okh[b] = okh[b] && is_fin(wt[b]) && wt[b] != 0.0;
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const cplx hs = a.H[b][((f * 2 + 0) * 2 + s) * a.K + (bin - 1)];
            const cplx he = a.H[b][((f * 2 + 1) * 2 + s) * a.K + (bin - 1)];
            ms[b][s] = hypot(hs.x, hs.y);
            me[b][s] = hypot(he.x, he.y);
            okh[b] = okh[b] && is_fin(ms[b][s]) && is_fin(me[b][s]);
            const cplx u = ms[b][s] > 0.0 ? cmk(hs.x / ms[b][s], hs.y / ms[b][s]) : cmk(1.0, 0.0);
            w[b][s] = cmul(u, rot);
        }
    }
    double px[4], py[4];
    int lab[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { px[i] = a.cre[i]; py[i] = a.cim[i]; lab[i] = a.clab[i]; }

    for (int j = j0; j < j1; ++j) {
        const int64_t sym = f * D + 2 * j;
        const double fa = (2 * j + P / 2.0) / (double)(D + P);      // the reference's f_l (channel_model) at both slots
        const double fb = (2 * j + 1 + P / 2.0) / (double)(D + P);
        cplx ya[B], yb[B];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            ya[b] = a.Y[b][sym * a.NB + bin];
            yb[b] = a.Y[b][(sym + 1) * a.NB + bin];
        }
        double G00 = 0.0, G11 = 0.0;
        cplx G01 = cmk(0.0, 0.0), m0 = cmk(0.0, 0.0), m1 = cmk(0.0, 0.0);
        bool any = false;
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const bool ok = okh[b] && is_fin(ya[b].x) && is_fin(ya[b].y) && is_fin(yb[b].x) && is_fin(yb[b].y);
            any = any || ok;
            const cplx h0a = cscale(w[b][0], ms[b][0] + (me[b][0] - ms[b][0]) * fa);
            const cplx h1a = cscale(w[b][1], ms[b][1] + (me[b][1] - ms[b][1]) * fa);
            w[b][0] = cmul(w[b][0], step);
            w[b][1] = cmul(w[b][1], step);
            const cplx h0b = cscale(w[b][0], ms[b][0] + (me[b][0] - ms[b][0]) * fb);
            const cplx h1b = cscale(w[b][1], ms[b][1] + (me[b][1] - ms[b][1]) * fb);
            w[b][0] = cmul(w[b][0], step);
            w[b][1] = cmul(w[b][1], step);
            const cplx ga = cmul_conj(h1a, h0a), gb = cmul_conj(h1b, h0b);    // conj(h0) h1 at either slot
            const cplx a0 = cmul_conj(ya[b], h0a), a1 = cmul_conj(ya[b], h1a);
            const cplx b0 = cmul_conj(h1b, yb[b]), b1 = cmul_conj(h0b, yb[b]); // h1(b') conj(y_b'), h0(b') conj(y_b')
            double p0 = (h0a.x * h0a.x + h0a.y * h0a.y) + (h1b.x * h1b.x + h1b.y * h1b.y);
            double p1 = (h1a.x * h1a.x + h1a.y * h1a.y) + (h0b.x * h0b.x + h0b.y * h0b.y);
            cplx g = cmk(ga.x - gb.x, ga.y - gb.y);
            cplx s0 = cmk(a0.x + b0.x, a0.y + b0.y), s1 = cmk(a1.x - b1.x, a1.y - b1.y);
            if constexpr (NW) {                             // both slots of the pair carry the branch's one weight
                p0 *= wt[b]; p1 *= wt[b];
                g = cscale(g, wt[b]); s0 = cscale(s0, wt[b]); s1 = cscale(s1, wt[b]);
            }
            G00 += ok ? p0 : 0.0;
            G11 += ok ? p1 : 0.0;
            G01.x += ok ? g.x : 0.0;    G01.y += ok ? g.y : 0.0;
            m0.x += ok ? s0.x : 0.0;    m0.y += ok ? s0.y : 0.0;
            m1.x += ok ? s1.x : 0.0;    m1.y += ok ? s1.y : 0.0;
        }
        // the 16 metrics d[i][k] of (x0 = point i, x1 = point k), reduced once along each symbol of the pair, as
        // mimo_detect_kernel reduces them along each stream: best[0][i] is the minimum over x1 with x0 = point i,
        // best[1][k] the minimum over x0 with x1 = point k.  (Minima round nothing: the numbers are the plain scan's.)
        double A[4], best[2][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            A[i] = G00 * (px[i] * px[i] + py[i] * py[i]) - 2.0 * (px[i] * m0.x + py[i] * m0.y);
            best[0][i] = INFINITY;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double Bk = G11 * (px[k] * px[k] + py[k] * py[k]) - 2.0 * (px[k] * m1.x + py[k] * m1.y);
            const cplx q = cmul(G01, cmk(px[k], py[k]));
            best[1][k] = INFINITY;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double d = A[i] + Bk + 2.0 * (px[i] * q.x + py[i] * q.y);
                best[0][i] = fmin(best[0][i], d);
                best[1][k] = fmin(best[1][k], d);
            }
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {                       // x0 is symbol 2j's, x1 symbol 2j + 1's
            float out[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                double one = INFINITY, zero = INFINITY;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const bool bit = (lab[i] >> (1 - k)) & 1;
                    one = fmin(one, bit ? best[s][i] : INFINITY);
                    zero = fmin(zero, bit ? INFINITY : best[s][i]);
                }
                out[k] = any ? (float)(one - zero) : 0.0f;
            }
            store_llr<2>(a.llr, (sym + s) * (int64_t)a.C + c, out);
        }
    }
}

// what both entries refuse of a context: the cover and the pairing
int stbc_geometry(const gf3_ctx* c, const char* who) {
    if (const int rc = needs_even_cover(c, who)) return rc;
    if (c->cfg.D & 1)
        return fail(c, GF3_EINVAL, "%s: the code pairs the data symbols: an even D (D=%d)", who, c->cfg.D);
    return GF3_OK;
}

}  // namespace

extern "C" int gf3_stbc_slope(gf3_ctx* c, int32_t B, const void* const* d_H, int64_t F, double* d_slope, void* stream) {
    DeviceGuard dg(c);
    if (!c) return fail(c, GF3_EINVAL, "gf3_stbc_slope: null context");
    if (const int rc = stbc_geometry(c, "gf3_stbc_slope")) return rc;
    if (F == 0) return GF3_OK;
    if (!(branches_ok(B, d_H) && d_slope && F >= 0))
        return fail(c, GF3_EINVAL, "gf3_stbc_slope: bad argument (1 <= B <= %d branches of estimates; an output; F >= 0)", GF3_MAX_BRANCHES);
    if (const int rc = too_many_packets_i32(c, F, "gf3_stbc_slope")) return rc;
    const int L = c->fit_hi - c->fit_lo;
    if (L < 2 || c->fit_lo < 0 || c->fit_hi > c->K)
        return fail(c, GF3_EINVAL, "gf3_stbc_slope: the fit range [%d, %d) holds fewer than 2 carriers of %d", c->fit_lo, c->fit_hi, c->K);
    StbcSlopeArgs a{};
    for (int b = 0; b < B; ++b) a.H[b] = (const cplx*)d_H[b];
    a.slope = d_slope;
    a.K = c->K; a.fit_lo = c->fit_lo; a.fit_hi = c->fit_hi; a.xbar = c->xbar; a.inv_sxx = c->inv_sxx;
    const size_t lds = (size_t)(8 + L) * sizeof(double);
    const hipError_t e = with_branches(B, [&](auto nb) {
        return launch((stbc_slope_kernel<decltype(nb)::value>), F, ST_THREADS, lds, (hipStream_t)stream, a);
    });
    HIPCHK(c, e);
    return GF3_OK;
}

// both entries of the detector: `who` names the caller in a refusal, d_w is null for the unweighted one
template <bool NW>
static int stbc_detect_call(gf3_ctx* c, const char* who, int32_t B, const void* const* d_Y, const void* const* d_H,
                            const double* d_slope, const double* d_w, int64_t F, float* d_llr, void* stream) {
    DeviceGuard dg(c);
    if (!c) return fail(c, GF3_EINVAL, "%s: null context", who);
    if (const int rc = needs_4_points(c, who)) return rc;
    if (const int rc = stbc_geometry(c, who)) return rc;
    if (F == 0) return GF3_OK;
    if (!(branches_ok(B, d_Y, d_H) && d_slope && d_llr && F >= 0 && (!NW || d_w)))
        return fail(c, GF3_EINVAL, "%s: bad argument (1 <= B <= %d branches, each with spectra and estimates; one slope "
                                   "array; %san output; F >= 0)", who, GF3_MAX_BRANCHES, NW ? "the weights; " : "");
    if (const int rc = too_many_packets(c, F, who)) return rc;
    StbcDetectArgs a{};
    for (int b = 0; b < B; ++b) { a.Y[b] = (const cplx*)d_Y[b]; a.H[b] = (const cplx*)d_H[b]; }
    a.slope = d_slope;
    a.llr = d_llr;
    a.bins = c->d_bins;
    a.D = c->cfg.D; a.C = c->cfg.C; a.K = c->K; a.NB = c->NC + 1; a.P = c->cfg.P;
    const TileGrid g = tile_grid(c, F, a.D / 2, JOINT_THREADS);
    a.ntile = g.ntile; a.Jc = g.run;
    a.cre = c->d_cre; a.cim = c->d_cim; a.clab = c->d_clab;
    a.wgt = d_w;
    with_branches(B, [&](auto nb) {
        hipLaunchKernelGGL((stbc_detect_kernel<decltype(nb)::value, NW>), g.grid, dim3(JOINT_THREADS), 0, (hipStream_t)stream, a);
    });
    HIPCHK(c, hipGetLastError());
    return GF3_OK;
}

extern "C" int gf3_stbc_detect(gf3_ctx* c, int32_t B, const void* const* d_Y, const void* const* d_H, const double* d_slope,
                               int64_t F, float* d_llr, void* stream) {
    return stbc_detect_call<false>(c, "gf3_stbc_detect", B, d_Y, d_H, d_slope, nullptr, F, d_llr, stream);
}

extern "C" int gf3_stbc_detect_nw(gf3_ctx* c, int32_t B, const void* const* d_Y, const void* const* d_H, const double* d_slope,
                                  const double* d_w, int64_t F, float* d_llr, void* stream) {
    return stbc_detect_call<true>(c, "gf3_stbc_detect_nw", B, d_Y, d_H, d_slope, d_w, F, d_llr, stream);
}
