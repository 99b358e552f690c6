// libgf3rx -- the stand-alone demappers (gf3_demap_hard, gf3_soft_demap, gf3_soft_demap_csi with its weighting kernel) and
// the known-channel zero forcing, which ends in the hard demapper.  The per-symbol arithmetic is gf3rx_demap.h's.
#include "gf3rx_demod.h"
#include "gf3rx_demap.h"

// standalone demappers
struct DemapArgs {
    const cplx* sym; int64_t n;
    DemapTab t;
    uint8_t* bits; float* llr; double inv_nv; uint8_t* idx;
};
__global__ void demap_hard_kernel(DemapArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        const cplx e = a.sym[i];
        const int best = scan_table(e, a.t.cre, a.t.cim, a.t.M);    // literal: this entry point is `demap` itself
        const int lab = a.t.clab[best];
        for (int b = 0; b < a.t.mu; ++b) a.bits[i * a.t.mu + b] = (lab >> (a.t.mu - 1 - b)) & 1;
        if (a.idx) a.idx[i] = (uint8_t)best;
    }
}
// max-log LLR per bit: (min over points with bit=1 of d^2 - min over points with bit=0 of d^2) / noise_var; the
// per-symbol arithmetic is gf3rx_demap.h's
__global__ void soft_demap_kernel(DemapArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        maxlog_table(a.sym[i], a.t, a.inv_nv, a.llr + i * a.t.mu);
    }
}

// Separable tables (grid constellations with per-axis bit labels): a bit owned by one axis sees the other axis'
// term cancel in the difference, so its LLR needs that axis' <= 8 squared distances only.  Everything that steers
// the reduction (which axis owns bit b, which levels carry a 1 there, how many levels exist) is wave-uniform and
// lives in scalar registers; the loops are fully unrolled over MU bits x 8 levels, each step one scalar bit test
// around one v_min_f64.
template <int MU>
__global__ __launch_bounds__(256) void soft_demap_sep_kernel(DemapArgs a) {
    int ones[MU];                                    // bit b: mask of the owning axis' levels whose label has a 1 there
    bool onI[MU];
#pragma unroll
    for (int b = 0; b < MU; ++b) {
        onI[b] = (a.t.sep.maskI >> (MU - 1 - b)) & 1;
        ones[b] = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) ones[b] |= (((onI[b] ? a.t.sep.labI[k] : a.t.sep.labQ[k]) >> (MU - 1 - b)) & 1) << k;
    }
    const int nI = a.t.sep.nI, nQ = a.t.sep.nQ;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        const cplx e = a.sym[i];
        double dI[8], dQ[8];
        axis_d2<8>(e.x, a.t.sep.lvI, dI);
        axis_d2<8>(e.y, a.t.sep.lvQ, dQ);
        float out[MU];
#pragma unroll
        for (int b = 0; b < MU; ++b) {
            double m0 = INFINITY, m1 = INFINITY;
            // (opaque per symbol: otherwise the 8 MU level tests are hoisted out of the symbol loop as 8 MU SGPR
            //  pairs, which spill to VGPR lanes and come back through v_readlane on every use)
            asm volatile("" : "+s"(ones[b]));
            if (onI[b]) {
#pragma unroll
                for (int k = 0; k < 8; ++k) if (k < nI) { if ((ones[b] >> k) & 1) m1 = fmin(m1, dI[k]); else m0 = fmin(m0, dI[k]); }
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) if (k < nQ) { if ((ones[b] >> k) & 1) m1 = fmin(m1, dQ[k]); else m0 = fmin(m0, dQ[k]); }
            }
            out[b] = (float)((m1 - m0) * a.inv_nv);
        }
        store_llr<MU>(a.llr, i, out);
    }
}

// The same for the binary-indexed grids (sep_is_binary: every square Gray QAM generator's table and the reference's
// QPSK): straight-line minima (maxlog_bin; the generic kernel above spends more time steering than computing: 48
// scalar branches per symbol against 48 minima).
template <int HI, int HQ>
__global__ __launch_bounds__(256) void soft_demap_bin_kernel(DemapArgs a) {
    constexpr int MU = HI + HQ, NI = 1 << HI, NQ = 1 << HQ;
    double lvI[NI], lvQ[NQ];
#pragma unroll
    for (int k = 0; k < NI; ++k) lvI[k] = a.t.sep.lvI[k];
#pragma unroll
    for (int k = 0; k < NQ; ++k) lvQ[k] = a.t.sep.lvQ[k];
    // (inv_nv is a scale, never an erasure mark: ERASE = false, see emit_grid_llr)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x)
        emit_grid_llr<HI, HQ, false>(a.sym[i], lvI, lvQ, a.inv_nv, [llr = a.llr, i](const float (&out)[MU]) { store_llr<MU>(llr, i, out); });
}

typedef void (*DemapKernel)(DemapArgs);
static int run_demap(gf3_ctx* c, const void* d_sym, int64_t n, uint8_t* bits, uint8_t* idx, float* llr, double nv, void* stream) {
    // any separable table that is no binary-indexed grid, by its mu = 1 .. 8
    static const DemapKernel sep_k[8] = {soft_demap_sep_kernel<1>, soft_demap_sep_kernel<2>, soft_demap_sep_kernel<3>, soft_demap_sep_kernel<4>,
                                         soft_demap_sep_kernel<5>, soft_demap_sep_kernel<6>, soft_demap_sep_kernel<7>, soft_demap_sep_kernel<8>};
    DemapArgs a{(const cplx*)d_sym, n, demap_tab(c), bits, llr, nv > 0 ? 1.0 / nv : 0.0, idx};
    int64_t grid = (n + 255) / 256;
    if (grid > 256 * 16) grid = 256 * 16;
    DemapKernel k = soft_demap_kernel;                               // literal scan
    if (bits) k = demap_hard_kernel;
    else if (c->sep.nI > 0)                                          // QPSK, 16-QAM, 64-QAM (HI = 1, 2, 3): straight-line minima
        k = with_grid_bits(c, [&](auto hi) -> DemapKernel {
            constexpr int HI = decltype(hi)::value;
            if constexpr (HI > 0) return soft_demap_bin_kernel<HI, HI>;
            else return sep_k[c->cfg.mu - 1];
        });
    HIPCHK(c, launch(k, grid, 256, 0, (hipStream_t)stream, a));
    return GF3_OK;
}

// CSI weighting of max-log LLRs (computed with sigma^2 = 1 by the soft demapper): LLR *= |H^|^2 with the reference's
// magnitude model (csi_weight, gf3rx_demap.h), from Hs / He [F, K] directly.  A thread owns carrier k of symbol (f, l);
// carriers that carry no data (pos[k] < 0) have nothing to do.
struct CsiArgs { float* llr; const cplx* Hs; const cplx* He; const int* pos; int64_t F; int K, D, P, C, mu; };
__global__ __launch_bounds__(256) void csi_weight_kernel(CsiArgs a) {
    const int64_t total = a.F * a.D * a.K, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const int kk = (int)(t % a.K);
        const int pos = a.pos[kk];
        if (pos < 0) continue;
        const int64_t fl = t / a.K, f = fl / a.D;
        const int l = (int)(fl - f * a.D);
        const double wgt = csi_weight(a.Hs[f * a.K + kk], a.He[f * a.K + kk], l, a.P, a.D);
        float* p = a.llr + (fl * a.C + pos) * a.mu;
        for (int b = 0; b < a.mu; ++b) p[b] = (float)((double)p[b] * wgt);
    }
}
static hipError_t launch_csi_weight(const gf3_ctx* c, float* d_llr, const void* d_Hs, const void* d_He, int64_t F, hipStream_t st) {
    CsiArgs a{d_llr, (const cplx*)d_Hs, (const cplx*)d_He, c->d_pos, F, c->K, c->cfg.D, c->cfg.P, c->cfg.C, c->cfg.mu};
    int64_t grid = (F * c->cfg.D * c->K + 255) / 256;
    if (grid > 16 * (int64_t)c->n_cu) grid = 16 * (int64_t)c->n_cu;
    if (grid < 1) return hipSuccess;
    hipLaunchKernelGGL(csi_weight_kernel, dim3((unsigned)grid), dim3(256), 0, st, a);
    return hipGetLastError();
}

extern "C" int gf3_demap_hard(gf3_ctx* c, const void* d_sym, int64_t n, uint8_t* d_bits, uint8_t* d_idx, void* stream) {
    DeviceGuard dg(c);
    if (c && n == 0) return GF3_OK;
    if (!c || !d_sym || !d_bits || n < 0) return fail(c, GF3_EINVAL, "gf3_demap_hard: bad argument");
    return run_demap(c, d_sym, n, d_bits, d_idx, nullptr, 1.0, stream);
}
extern "C" int gf3_soft_demap(gf3_ctx* c, const void* d_sym, int64_t n, double noise_var, float* d_llr, void* stream) {
    DeviceGuard dg(c);
    if (c && n == 0) return GF3_OK;
    if (!c || !d_sym || !d_llr || n < 0 || !(noise_var > 0)) return fail(c, GF3_EINVAL, "gf3_soft_demap: bad argument");
    return run_demap(c, d_sym, n, nullptr, nullptr, d_llr, noise_var, stream);
}
extern "C" int gf3_soft_demap_csi(gf3_ctx* c, const void* d_eq, const void* d_Hs, const void* d_He, int64_t F, float* d_llr, void* stream) {
    DeviceGuard dg(c);
    if (c && F == 0) return GF3_OK;
    if (!c || !d_eq || !d_Hs || !d_He || !d_llr || F < 0) return fail(c, GF3_EINVAL, "gf3_soft_demap_csi: bad argument");
    const int rc = run_demap(c, d_eq, F * c->cfg.D * c->cfg.C, nullptr, nullptr, d_llr, 1.0, stream);   // max-log, sigma^2 = 1
    if (rc != GF3_OK) return rc;
    HIPCHK(c, launch_csi_weight(c, d_llr, d_Hs, d_He, F, (hipStream_t)stream));
    return GF3_OK;
}

__global__ void zf_bins_kernel(const int* pos, int K, int* bins) {      // bins[pos[k]] = k + 1 for every data carrier
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < K && pos[k] >= 0) bins[pos[k]] = k + 1;
}
// known-channel zero forcing (the reference's older flow, `Weekend Challenge.ipynb` cells 9-15: H = fft(h, N),
// symbols = FFT(rx) / H on bins 1..N/2-1).  Not on receive()'s path and without a surviving reference function:
// parity is pinned by the formula only (oracle.zf_known_h).
struct ZfArgs { const cplx* X; const cplx* H; const int* bins; int64_t n_sym; int C, NC; cplx* eq; };
__global__ void zf_kernel(ZfArgs a) {
    const int64_t total = a.n_sym * a.C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / a.C;
        const int b = a.bins[i - s * a.C];
        a.eq[i] = cdiv_np(a.X[s * (a.NC + 1) + b], a.H[b]);              // complex128 division as NumPy performs it
    }
}
extern "C" int64_t gf3_known_h_workspace_bytes(const gf3_ctx* c, int64_t n_sym) {
    if (!c || n_sym < 0) return 0;
    return (int64_t)((size_t)(n_sym + 1) * (c->NC + 1) * sizeof(cplx) + (size_t)2 * c->NC * sizeof(double) + 16 + (size_t)c->cfg.C * 4 + 256);
}
extern "C" int gf3_equalise_known_h(gf3_ctx* c, const void* d_in, int64_t n_in, const int64_t* d_offsets, int64_t n_sym,
                                    const double* d_h, int32_t n_taps, void* d_eq, uint8_t* d_bits, uint8_t* d_idx,
                                    void* d_work, void* stream) {
    DeviceGuard dg(c);
    if (c && n_sym == 0) return GF3_OK;
    if (!c || !d_in || !d_offsets || !d_h || !d_eq || !d_bits || !d_work || n_sym < 0 || n_taps < 1 || n_taps > 2 * c->NC)
        return fail(c, GF3_EINVAL, "gf3_equalise_known_h: bad argument (1 <= n_taps <= N)");
    hipStream_t st = (hipStream_t)stream;
    const int NC = c->NC, N = 2 * NC;
    char* base = (char*)d_work;
    cplx* X = (cplx*)base;                                               // [n_sym][NC+1]
    cplx* H = X + (size_t)n_sym * (NC + 1);                              // [NC+1]
    double* hpad = (double*)(H + (NC + 1));                              // [N] taps, zero padded (np.fft.fft(h, N))
    int64_t* zero = (int64_t*)(hpad + N);                                // offset 0 of the padded taps
    int* bins = (int*)(zero + 2);
    HIPCHK(c, hipMemsetAsync(hpad, 0, (size_t)N * sizeof(double) + 16, st));
    HIPCHK(c, hipMemcpyAsync(hpad, d_h, (size_t)n_taps * sizeof(double), hipMemcpyDeviceToDevice, st));
    // data-carrier bins in output order (the context keeps the carrier -> position map; invert it on the device)
    hipLaunchKernelGGL(zf_bins_kernel, dim3((c->K + 255) / 256), dim3(256), 0, st, (const int*)c->d_pos, c->K, bins);
    HIPCHK(c, run_rfft_nc(NC, FftTables{c->d_tw, c->d_twn}, hpad, N, DT_F64, zero, 1, H, st));
    HIPCHK(c, run_rfft(c, d_in, n_in, c->cfg.in_dtype, d_offsets, n_sym, X, st));
    ZfArgs a{X, H, bins, n_sym, c->cfg.C, NC, (cplx*)d_eq};
    int64_t grid = (n_sym * c->cfg.C + 255) / 256;
    if (grid > 65536) grid = 65536;
    hipLaunchKernelGGL(zf_kernel, dim3((unsigned)grid), dim3(256), 0, st, a);
    HIPCHK(c, hipGetLastError());
    return run_demap(c, d_eq, n_sym * c->cfg.C, d_bits, d_idx, nullptr, 1.0, stream);
}
