// libgf3rx -- decision-directed per-carrier noise estimate and the noise-weighted soft demapper (gf3_noise_estimate,
// gf3_soft_demap_nw).  See DESIGN.md §12.
//
//   v[f, c]   = (1/D) sum_l |eq[f, l, c] - s|^2, s the point the hard decision picks (in-order scan, strict <)
//   vbar[f]   = mean_c v[f, c]
//   w[f, c]   = 0 where v is not finite; 1 for the whole packet where vbar is 0 or not finite; else 1 / max(v, 1e-6 vbar)
//   LLR       = maxlog(eq; sigma^2 = 1) * w   (float32; +0 where w = 0: an erasure, whatever the symbol held)
//
// Every sum runs in a fixed order (no floating-point atomics): two runs give identical bits.
#include "gf3rx_demap.h"

namespace {

constexpr int NE_WAVES = 8;             // waves of a noise_estimate workgroup: the D symbols are dealt out to them
constexpr int NW_THREADS = 256;

struct NoiseArgs {
    const cplx* eq; double* var; const double* var_in; float* llr;
    int64_t F; int D, C, Dc;            // Dc: symbols per soft_demap_nw workgroup
    DemapTab t;
};

// HI > 0: binary-indexed 2^HI x 2^HI grid (levels in registers); HI == 0: any table (literal scan).
template <int HI>
struct Levels {
    double lvI[1 << HI], lvQ[1 << HI];
    GF3_DEV explicit Levels(const DemapTab& t) {
#pragma unroll
        for (int k = 0; k < (1 << HI); ++k) { lvI[k] = t.sep.lvI[k]; lvQ[k] = t.sep.lvQ[k]; }
    }
};

// noise_estimate: a workgroup owns 64 consecutive carriers of one packet (lane = carrier: a wave reads 1 KB
// contiguously per symbol); wave w adds up the symbols l = w, w + 8, w + 16, ... in ascending order, the 8 partial sums
// meet in LDS and wave 0 adds them in the order w = 0 .. 7, then divides by D.
template <int HI>
__global__ __launch_bounds__(64 * NE_WAVES) void noise_estimate_kernel(NoiseArgs a) {
    __shared__ double part[NE_WAVES][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int64_t f = blockIdx.y;
    const Levels<HI> lv(a.t);
    double acc = 0.0;
    if (c < a.C) {
        const cplx* p = a.eq + (f * a.D) * (int64_t)a.C + c;
        for (int l = w; l < a.D; l += NE_WAVES) {
            const cplx e = p[(int64_t)l * a.C];
            if constexpr (HI > 0) acc += axis_min_d2<(1 << HI)>(e.x, lv.lvI) + axis_min_d2<(1 << HI)>(e.y, lv.lvQ);
            else acc += table_min_d2(e, a.t.cre, a.t.cim, a.t.M);
        }
    }
    part[w][lane] = acc;
    __syncthreads();
    if (w == 0 && c < a.C) {
        double s = part[0][lane];
#pragma unroll
        for (int k = 1; k < NE_WAVES; ++k) s += part[k][lane];
        a.var[f * a.C + c] = s / (double)a.D;
    }
}

// soft_demap_nw: a workgroup owns Dc consecutive symbols of one packet.  It first turns the packet's variances into
// weights in LDS (thread t adds v[t], v[t + 256], ... in ascending order, a binary tree over the 256 partial sums gives
// vbar: the same number in every workgroup of the packet), then streams its symbols: thread = carrier, 16 bytes read
// and 4 mu bytes written per symbol, the weight from LDS.
template <int HI>
__global__ __launch_bounds__(NW_THREADS) void soft_demap_nw_kernel(NoiseArgs a) {
    extern __shared__ double nw_lds[];              // [256] partial sums, then [C] weights
    double* red = nw_lds;
    double* wgt = nw_lds + NW_THREADS;
    const int t = threadIdx.x, C = a.C;
    const int64_t f = blockIdx.y;
    const double* v = a.var_in + f * C;
    double s = 0.0;
    for (int c = t; c < C; c += NW_THREADS) s += v[c];
    red[t] = s;
    __syncthreads();
#pragma unroll
    for (int h = NW_THREADS / 2; h > 0; h >>= 1) {
        if (t < h) red[t] += red[t + h];
        __syncthreads();
    }
    const double vbar = red[0] / (double)C;
    const bool flat = !(vbar > 0.0) || !(vbar < INFINITY);          // 0, NaN, Inf: the packet's weights are 1
    const double floor_v = 1e-6 * vbar;
    for (int c = t; c < C; c += NW_THREADS) {
        const double x = v[c];
        wgt[c] = !(fabs(x) < INFINITY) ? 0.0 : flat ? 1.0 : 1.0 / fmax(x, floor_v);
    }
    __syncthreads();
    const Levels<HI> lv(a.t);
    const int l0 = blockIdx.x * a.Dc, l1 = min(l0 + a.Dc, a.D);
    for (int l = l0; l < l1; ++l) {
        const int64_t row = (f * a.D + l) * (int64_t)C;
        for (int c = t; c < C; c += NW_THREADS) {
            const cplx e = a.eq[row + c];
            const double w = wgt[c];
            if constexpr (HI > 0) {
                constexpr int MU = 2 * HI;
                double diff[MU];
                maxlog_bin<HI, HI>(e, lv.lvI, lv.lvQ, diff);
                float out[MU];
#pragma unroll
                for (int b = 0; b < MU; ++b) out[b] = w == 0.0 ? 0.0f : (float)(diff[b] * w);
                store_llr<MU>(a.llr, row + c, out);
            } else {
                float* dst = a.llr + (row + c) * a.t.mu;
                if (w == 0.0) { for (int b = 0; b < a.t.mu; ++b) dst[b] = 0.0f; }
                else maxlog_table(e, a.t, w, dst);
            }
        }
    }
}

// binary-indexed grid up to 64-QAM -> its HI, anything else -> 0 (as run_demap chooses its kernels)
int grid_bits(const gf3_ctx* c) {
    int hI = 0, hQ = 0;
    return (c->sep.nI > 0 && sep_is_binary(c->sep, c->cfg.mu, hI, hQ) && hI <= 3) ? hI : 0;
}

}  // namespace

extern "C" int gf3_noise_estimate(gf3_ctx* c, const void* d_eq, int64_t F, double* d_var, void* stream) {
    DeviceGuard dg(c);
    if (c && F == 0) return GF3_OK;
    if (!c || !d_eq || !d_var || F < 0) return fail(c, GF3_EINVAL, "gf3_noise_estimate: bad argument");
    if (F > 65535) return fail(c, GF3_EINVAL, "gf3_noise_estimate: at most 65535 packets per call");
    NoiseArgs a{(const cplx*)d_eq, d_var, nullptr, nullptr, F, c->cfg.D, c->cfg.C, 0, demap_tab(c)};
    const dim3 grid((unsigned)((a.C + 63) / 64), (unsigned)F), block(64 * NE_WAVES);
    hipStream_t st = (hipStream_t)stream;
    switch (grid_bits(c)) {
        case 1: hipLaunchKernelGGL(noise_estimate_kernel<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(noise_estimate_kernel<2>, grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL(noise_estimate_kernel<3>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(noise_estimate_kernel<0>, grid, block, 0, st, a); break;
    }
    HIPCHK(c, hipGetLastError());
    return GF3_OK;
}

extern "C" int gf3_soft_demap_nw(gf3_ctx* c, const void* d_eq, const double* d_var, int64_t F, float* d_llr, void* stream) {
    DeviceGuard dg(c);
    if (c && F == 0) return GF3_OK;
    if (!c || !d_eq || !d_var || !d_llr || F < 0) return fail(c, GF3_EINVAL, "gf3_soft_demap_nw: bad argument");
    if (F > 65535) return fail(c, GF3_EINVAL, "gf3_soft_demap_nw: at most 65535 packets per call");
    NoiseArgs a{(const cplx*)d_eq, nullptr, d_var, d_llr, F, c->cfg.D, c->cfg.C, 0, demap_tab(c)};
    // about 8 workgroups per compute unit when there are packets enough; a handful of long packets is cut down to
    // single symbols
    int64_t nchunk = (8 * (int64_t)c->n_cu + F - 1) / F;
    if (nchunk > a.D) nchunk = a.D;
    if (nchunk < 1) nchunk = 1;
    a.Dc = (int)((a.D + nchunk - 1) / nchunk);
    const dim3 grid((unsigned)((a.D + a.Dc - 1) / a.Dc), (unsigned)F), block(NW_THREADS);
    const size_t lds = (size_t)(NW_THREADS + a.C) * sizeof(double);
    hipStream_t st = (hipStream_t)stream;
    switch (grid_bits(c)) {
        case 1: hipLaunchKernelGGL(soft_demap_nw_kernel<1>, grid, block, lds, st, a); break;
        case 2: hipLaunchKernelGGL(soft_demap_nw_kernel<2>, grid, block, lds, st, a); break;
        case 3: hipLaunchKernelGGL(soft_demap_nw_kernel<3>, grid, block, lds, st, a); break;
        default: hipLaunchKernelGGL(soft_demap_nw_kernel<0>, grid, block, lds, st, a); break;
    }
    HIPCHK(c, hipGetLastError());
    return GF3_OK;
}
