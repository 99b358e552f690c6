// libgf3rx -- delay-domain denoising of the pilot channel estimate (not in the reference).
//
// The least-squares estimate Hs / He (OFDM.py:443-451) treats its K carriers as K unknowns; an acoustic channel has a few
// dozen to a few hundred significant taps.  denoise_kernel rewrites one row of the two-phase demodulator's pilot sums
// (psum [F][2][N], gf3rx_demod_split.hip) in place, between pilot_sum_kernel and demod_kernel<.., STAGE_EST>, so that
// the estimate stage -- untouched -- divides a cleaner spectrum.  One workgroup per (packet, side), NC/8 threads:
//   1. v   = sum_n sum_p (x_p[n] - S[n]/P)^2 / ((P-1) N): the noise variance, measured from the P pilot repeats (two-pass
//            form: v >= 0), S read from psum;
//   2. h   = irfft(rfft(S) / (P known)), bins 0 and N/2 zero: N real taps;
//   3. s2  = 2 v / (N P) sum_k 1/|known_k|^2: the noise variance of one tap;
//   4. keep tap n iff h[n]^2 > tau s2; kept = their number, post = the largest kept n < N/2 (-1: none), pre = the largest
//            N - n among kept n >= N/2 (0: none);
//   5. the row stays as it is (applied = 0) when v is not finite, the packet is ragged (zero row) or kept > N/4;
//   6. else psum' = irfft(rfft(h keep) P known), bins 0 and N/2 as they were.
// Four transforms, all fp64, through the device functions of gf3rx_device.h (the inverse is tx_kernel's packing).  Every
// reduction is wave shuffles, then LDS, in a fixed order -- no atomics: two runs give identical bytes.
#include "gf3rx_host.h"

struct DenoiseArgs {
    FftTables t;
    const void* in; int64_t n_in; const int64_t* off;
    int CP, S, P, D;
    const cplx* inv_known;    // [K] 1/known symbol
    double tau;
    double* psum;             // [F][2][2 NC], rewritten in place
    double* report;           // [F][2][5] = {v, kept, post, pre, applied}, or null
};

// Half-spectrum in Spec<NC> slot order (bins 1 .. NC-1) plus the packed point Z0 = ((X_0 + X_NC)/2, (X_0 - X_NC)/2) ->
// the unnormalised inverse: the returned buffer holds y with x[2i] = y[i].x / NC, x[2i+1] = -y[i].y / NC (tx_kernel's
// packing: conj(Z) through the forward transform).  Barriers: before the first store and after the last pass.
template <int NC>
GF3_DEV cplx* irfft_slots(const cplx (&X)[8], cplx Z0, cplx* lds, FftTw<NC>& ft, cplx wb, int tid) {
    constexpr int T = NC / 8;
    lds_barrier();                                          // every reader of the buffers is done
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = Spec<NC>::bin(tid, 2 * r);
        const cplx A = X[2 * r];
        const cplx Bc = (k == NC - k) ? A : X[2 * r + 1];
        const cplx B = cconj(Bc);
        const cplx E = cscale(cadd(A, B), 0.5);
        const cplx Op = cmul_conj(cscale(csub(A, B), 0.5), Spec<NC>::pair_tw(tid, r, wb));
        const cplx Zk = cadd(E, mul_posi(Op));
        const cplx Zm = cadd(cconj(E), mul_posi(cconj(Op)));
        lds[k] = cconj(Zk);
        if (Spec<NC>::live(tid, 2 * r + 1)) lds[NC - k] = cconj(Zm);
    }
    if (tid == 0) lds[0] = cconj(Z0);
    lds_barrier();
    cplx v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = lds[tid + r * T];
    lds_barrier();
    ft.refresh();
    return fft_core<NC>(v, lds, ft, tid);
}

template <int NC, int DT>
__global__ __launch_bounds__(NC / 8) void denoise_kernel(DenoiseArgs a) {
    extern __shared__ double2 smem[];
    __shared__ double red[16];
    __shared__ int redi[3][16];
    constexpr int T = NC / 8, N = 2 * NC, NW = (T + 63) / 64;
    cplx* lds = smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = blockIdx.x, f = row >> 1;
    const int side = (int)(row & 1);
    const int P = a.P;
    cplx* prow = (cplx*)a.psum + row * NC;
    double* rep = a.report ? a.report + row * 5 : nullptr;
    auto say = [&](double v, int kept, int post, int pre, int applied) {
        if (rep && tid == 0) { rep[0] = v; rep[1] = (double)kept; rep[2] = (double)post; rep[3] = (double)pre; rep[4] = (double)applied; }
    };
    const int64_t off = a.off[f];
    const bool ok = off >= 0 && off + (int64_t)(2 * P + a.D) * a.S <= a.n_in;      // pilot_sum_kernel's rule
    if (!ok) { say(0.0, 0, -1, 0, 0); return; }                                      // ragged: the zero row stays

    // ---- 1. noise from the pilot repeats
    double acc = 0.0;
    {
        cplx mean[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) { const cplx s = prow[tid + r * T]; mean[r] = cmk(s.x / (double)P, s.y / (double)P); }
        const int64_t base = off + (int64_t)(side ? P + a.D : 0) * a.S + a.CP + 2 * tid;
        for (int p = 0; p < P; ++p) {
            RawPair<DT> raw[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) raw[r].load(a.in, base + (int64_t)p * a.S + 2 * r * T);
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const cplx d = csub(raw[r].get(), mean[r]);
                acc = fma(d.x, d.x, acc);
                acc = fma(d.y, d.y, acc);
            }
        }
    }
    const double var = block_sum(acc, red) / ((double)(P - 1) * (double)N);
    if (!(fabs(var) < INFINITY)) { say(var, 0, -1, 0, 0); return; }

    // ---- 2. delay-domain estimate  (1/known is fetched where it is used, twice, not held in 32 registers across the transforms)
    double q = 0.0;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const cplx ik = a.inv_known[Spec<NC>::bin(tid, s) - 1];
        if (Spec<NC>::live(tid, s)) q += ik.x * ik.x + ik.y * ik.y;
    }
    const double sum_ik2 = block_sum(q, red);               // sum_k 1/|known_k|^2
    FftTw<NC> ft;
    ft.init(tid, a.t.tw);
    const cplx wb = a.t.twn[tid];
    cplx v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = prow[tid + r * T];
    cplx z0;
    lds_barrier();
    rfft_regs<NC>(v, lds, ft, wb, tid, z0, 0);
    const double invP = 1.0 / (double)P;
#pragma unroll
    for (int s = 0; s < 8; ++s) v[s] = cmul(cscale(v[s], invP), a.inv_known[Spec<NC>::bin(launder(tid), s) - 1]);
    const cplx* y = irfft_slots<NC>(v, cmk(0.0, 0.0), lds, ft, wb, tid);

    // ---- 3, 4. threshold, keep mask and its three reductions
    const double s2 = 2.0 * var / ((double)N * (double)P) * sum_ik2;
    const double thr = a.tau * s2;
    const double sc = 1.0 / (double)NC;
    int kept = 0, post = -1, pre = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int i = tid + r * T;
        const cplx z = y[i];
        double h0 = z.x * sc, h1 = -z.y * sc;
        const bool k0 = h0 * h0 > thr, k1 = h1 * h1 > thr;
        const int n0 = 2 * i, n1 = 2 * i + 1;
        if (k0) { ++kept; if (n0 < NC) post = max(post, n0); else pre = max(pre, N - n0); }
        if (k1) { ++kept; if (n1 < NC) post = max(post, n1); else pre = max(pre, N - n1); }
        v[r] = cmk(k0 ? h0 : 0.0, k1 ? h1 : 0.0);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        kept += __shfl_xor(kept, d, 64);
        post = max(post, __shfl_xor(post, d, 64));
        pre = max(pre, __shfl_xor(pre, d, 64));
    }
    if (lane == 0) { redi[0][wave] = kept; redi[1][wave] = post; redi[2][wave] = pre; }
    lds_barrier();
    kept = 0; post = -1; pre = 0;
    for (int w = 0; w < NW; ++w) { kept += redi[0][w]; post = max(post, redi[1][w]); pre = max(pre, redi[2][w]); }

    // ---- 5. not sparse at this noise level (or noiseless: every tap is kept): nothing to gain
    if (kept > N / 4) { say(var, kept, post, pre, 0); return; }

    // ---- 6. back to the pilot sum's scale
    cplx zh;
    lds_barrier();
    rfft_regs<NC>(v, lds, ft, wb, tid, zh, 0);
    const double dP = (double)P;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const cplx ik = a.inv_known[Spec<NC>::bin(launder(tid), s) - 1];
        const double m2 = ik.x * ik.x + ik.y * ik.y;
        const cplx kn = cscale(cconj(ik), rcp_nr(m2));              // known = 1 / (1/known)
        v[s] = cmul(cscale(v[s], dP), kn);
    }
    y = irfft_slots<NC>(v, z0, lds, ft, wb, tid);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int i = tid + r * T;
        const cplx z = y[i];
        prow[i] = cmk(z.x * sc, -z.y * sc);
    }
    say(var, kept, post, pre, 1);
}

static bool bad_threshold(double t) { return !(t > 0.0) || !(fabs(t) < INFINITY); }

// the denoiser on psum [F][2][N] (pilot_sum_kernel's output for the same samples and offsets), in place
int launch_denoise(const gf3_ctx* c, const void* d_in, int64_t n_in, const int64_t* d_off, int64_t F, double threshold,
                   double* d_psum, double* d_report, hipStream_t st) {
    if (c->cfg.P < 2) return fail(c, GF3_EINVAL, "pilot denoising measures the noise from the pilot repeats: P >= 2 (P=%d)", c->cfg.P);
    if (bad_threshold(threshold)) return fail(c, GF3_EINVAL, "pilot denoising: the threshold must be a finite number > 0");
    if (const int rc = too_many_packets_i32(c, F, "pilot denoising")) return rc;
    DenoiseArgs a{FftTables{c->d_tw, c->d_twn}, d_in, n_in, d_off, c->cfg.CP, c->S, c->cfg.P, c->cfg.D, c->d_known, threshold,
                  d_psum, d_report};
    hipError_t e = hipSuccess;
    DISPATCH_NC(c->NC, c->cfg.in_dtype, e = launch((denoise_kernel<NCC, DTC>), 2 * F, NCC / 8, fft_lds_bytes(NCC), st, a));
    HIPCHK(c, e);
    return GF3_OK;
}

extern "C" int gf3_denoise_pilots(gf3_ctx* c, const void* d_in, int64_t n_in, const int64_t* d_off, int64_t F, double threshold,
                                  double* d_psum_out, double* d_report, void* stream) {
    DeviceGuard dg(c);
    if (!c) return fail(c, GF3_EINVAL, "gf3_denoise_pilots: null context");
    if (c->cfg.P < 2) return fail(c, GF3_EINVAL, "gf3_denoise_pilots: the noise is measured from the pilot repeats, P >= 2 (P=%d)", c->cfg.P);
    if (bad_threshold(threshold)) return fail(c, GF3_EINVAL, "gf3_denoise_pilots: the threshold must be a finite number > 0");
    if (F == 0) return GF3_OK;
    if (!d_in || !d_off || !d_psum_out || F < 0 || n_in < 0) return fail(c, GF3_EINVAL, "gf3_denoise_pilots: bad argument");
    HIPCHK(c, launch_pilot_sum(c, d_in, n_in, d_off, F, d_psum_out, (hipStream_t)stream));
    return launch_denoise(c, d_in, n_in, d_off, F, threshold, d_psum_out, d_report, (hipStream_t)stream);
}
