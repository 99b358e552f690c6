// libgf3rx -- receive diversity: maximal-ratio combining of the equalised symbols of B recordings of one transmission
// (gf3_combine_branches).  See DESIGN.md §12.
//
//   z[f,l,c]  = (sum_b w_b z_b) / W,  W = sum_b w_b,  b ascending;  0 + 0i where W = 0
//   LLR       = maxlog(z; sigma^2 = 1) * W   (float32; +0 where W = 0)
//   csi:    w_b[f,l,c] = csi_weight_mag(|Hs_b|, |He_b|, l) at the carrier's bin (gf3rx_demap.h: the weight of gf3_soft_demap_csi)
//   noise:  vbar[f] = mean over b and c of var_b[f,c];  w_b[f,c] = 1 / max(var_b, 1e-6 vbar), 1 for the whole packet where
//           vbar is 0 or not finite (noise_weight of gf3rx_demap.h, with packet_vbar taken over all branches)
//   w_b = 0 where the weight's input or the weight itself is not finite or z_b is not finite in either part: that symbol
//   of that branch is left out of both sums.
//
// A workgroup owns 256 consecutive carriers x Dc consecutive symbols of one packet; thread = carrier, so a wave reads 1 KB
// contiguously per branch and symbol and the B per-carrier weight factors stay in registers for the whole run.  B is a
// template parameter: the branch loops unroll and the B loads of a symbol are in flight together.  Every sum runs in a
// fixed order (no floating-point atomics): two runs give identical bytes.
#include "gf3rx_demap.h"

namespace {

constexpr int CB_THREADS = VBAR_THREADS;

struct CombineArgs {
    const cplx* eq[GF3_MAX_BRANCHES];
    const cplx* Hs[GF3_MAX_BRANCHES]; const cplx* He[GF3_MAX_BRANCHES];     // csi
    const double* var[GF3_MAX_BRANCHES];                                    // noise
    cplx* eq_out; double* wsum; float* llr;
    const int* bins;                    // [C] 1-based FFT bin of each data carrier: Hs / He column bins[c] - 1
    int D, C, K, P, Dc, ntile;
    DemapTab t;
};

template <int B, bool NOISE, int HI>
__global__ __launch_bounds__(CB_THREADS) void combine_kernel(CombineArgs a) {
    __shared__ double red[CB_THREADS];
    const int t = threadIdx.x, C = a.C;
    const int tile = blockIdx.x % a.ntile, chunk = blockIdx.x / a.ntile;
    const int64_t f = blockIdx.y;
    const int c = tile * CB_THREADS + t;
    // per-carrier weight factors: noise -- the weight itself; csi -- |Hs_b| and |He_b| (NaN marks a non-finite input)
    double w0[B], w1[B];
    if constexpr (NOISE) {
        // vbar: thread t adds var_b[t], var_b[t + 256], ... for b ascending, packet_vbar adds the 256 partial sums: the same
        // number in every workgroup of the packet
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const double* v = a.var[b] + f * C;
            for (int k = t; k < C; k += CB_THREADS) s += v[k];
        }
        const PacketNoise pn = packet_vbar(red, s, (double)B * (double)C);
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const double w = noise_weight(c < C ? a.var[b][f * C + c] : 0.0, pn);
            w0[b] = is_fin(w) ? w : 0.0;
            w1[b] = 0.0;
        }
    } else {
#pragma unroll
        for (int b = 0; b < B; ++b) {
            w0[b] = w1[b] = 0.0;
            if (c < C) {
                const int64_t k = f * a.K + (a.bins[c] - 1);
                const cplx hs = a.Hs[b][k], he = a.He[b][k];
                w0[b] = hypot(hs.x, hs.y);
                w1[b] = hypot(he.x, he.y);
                if (!is_fin(w0[b]) || !is_fin(w1[b])) w0[b] = w1[b] = NAN;
            }
        }
    }
    if (c >= C) return;                             // (after the barriers)
    const Levels<HI> lv(a.t);
    const int l0 = chunk * a.Dc, l1 = min(l0 + a.Dc, a.D);
    for (int l = l0; l < l1; ++l) {
        const int64_t i = (f * a.D + l) * (int64_t)C + c;
        cplx z[B];
#pragma unroll
        for (int b = 0; b < B; ++b) z[b] = a.eq[b][i];
        double sx = 0.0, sy = 0.0, W = 0.0;
#pragma unroll
        for (int b = 0; b < B; ++b) {
            double w;
            if constexpr (NOISE) w = w0[b];
            else w = csi_weight_mag(w0[b], w1[b], l, a.P, a.D);
            if (!is_fin(w) || !is_fin(z[b].x) || !is_fin(z[b].y)) w = 0.0;
            sx += w == 0.0 ? 0.0 : w * z[b].x;
            sy += w == 0.0 ? 0.0 : w * z[b].y;
            W += w;
        }
        const cplx e = W == 0.0 ? cmk(0.0, 0.0) : cmk(sx / W, sy / W);
        if (a.eq_out) a.eq_out[i] = e;
        if (a.wsum) a.wsum[i] = W;
        if (a.llr) emit_llr<HI, true>(e, lv, a.t, W, [llr = a.llr, i, mu = a.t.mu](const auto& out) { store_llr_any(llr, i, mu, out); });
    }
}

}  // namespace

extern "C" int gf3_combine_branches(gf3_ctx* c, int32_t B, const void* const* d_eq, int32_t mode, const void* const* d_Hs,
                                    const void* const* d_He, const double* const* d_var, int64_t F, void* d_eq_out,
                                    double* d_wsum, float* d_llr, void* stream) {
    DeviceGuard dg(c);
    if (c && F == 0) return GF3_OK;
    const bool noise = mode == GF3_COMBINE_NOISE;
    bool ok = c && B >= 1 && B <= GF3_MAX_BRANCHES && d_eq && F >= 0 && (mode == GF3_COMBINE_CSI || noise) &&
              (noise ? d_var != nullptr : (d_Hs && d_He)) && (d_eq_out || d_wsum || d_llr);
    for (int b = 0; ok && b < B; ++b)
        ok = d_eq[b] && d_eq[b] != d_eq_out && (noise ? d_var[b] != nullptr : (d_Hs[b] && d_He[b]));
    if (!ok)
        return fail(c, GF3_EINVAL, "gf3_combine_branches: bad argument (1 <= B <= %d branches, mode 0 or 1 with its weight inputs, "
                                   "at least one output, eq_out none of the inputs)", GF3_MAX_BRANCHES);
    if (const int rc = too_many_packets(c, F, "gf3_combine_branches")) return rc;
    CombineArgs a{};
    for (int b = 0; b < B; ++b) {
        a.eq[b] = (const cplx*)d_eq[b];
        if (noise) a.var[b] = d_var[b];
        else { a.Hs[b] = (const cplx*)d_Hs[b]; a.He[b] = (const cplx*)d_He[b]; }
    }
    a.eq_out = (cplx*)d_eq_out; a.wsum = d_wsum; a.llr = d_llr;
    a.bins = c->d_bins;
    a.D = c->cfg.D; a.C = c->cfg.C; a.K = c->K; a.P = c->cfg.P;
    a.t = demap_tab(c);
    const TileGrid g = tile_grid(c, F, a.D, CB_THREADS);
    a.ntile = g.ntile; a.Dc = g.run;
    with_grid_bits(c, [&](auto hi) {
        with_branches(B, [&](auto nb) {
            constexpr int HI = decltype(hi)::value, NB = decltype(nb)::value;
            if (noise) hipLaunchKernelGGL((combine_kernel<NB, true, HI>), g.grid, dim3(CB_THREADS), 0, (hipStream_t)stream, a);
            else hipLaunchKernelGGL((combine_kernel<NB, false, HI>), g.grid, dim3(CB_THREADS), 0, (hipStream_t)stream, a);
        });
    });
    HIPCHK(c, hipGetLastError());
    return GF3_OK;
}
