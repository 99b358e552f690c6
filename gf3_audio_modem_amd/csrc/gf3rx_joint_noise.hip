// libgf3rx -- the two-speaker paths under coloured noise: the per-carrier noise variance of one recording measured on the
// covered pilots (gf3_mimo_pilot_noise) and the weights the joint detectors take from it (gf3_joint_noise_weights; the
// weighted detectors themselves are gf3_mimo_detect_nw and gf3_stbc_detect_nw of gf3rx_mimo.hip and gf3rx_stbc.hip).
// Not in the reference; see include/gf3rx.h and DESIGN.md §12.
//
// The pilots of a block read Y_p[k] = (H_b0[k] + (-1)^p H_b1[k]) X[k] + noise.  gf3_mimo_pilots spends two of the P
// observations per carrier on the two columns; what is left over,
//   v[f, side, k] = 1 / (P - 2) sum_p | Y_p[k] / X[k] - H[f, side, 0, k] - (-1)^p H[f, side, 1, k] |^2,
// is an unbiased estimate of the noise variance per carrier in the units of Y / X, and needs no decision: P >= 4.
//
// mimo_pilot_noise_kernel: mimo_pilots_kernel's shape -- one workgroup per (packet, side), NC/8 threads -- but every pilot
//   symbol is transformed on its own (rfft_regs of gf3rx_device.h, p ascending), the next symbol's samples in flight under
//   the current transform.  A thread keeps 1 / X and both columns of its own 8 bins in registers and adds the squared
//   residuals of those bins there, so nothing is shared between threads: no atomics, a fixed order, identical bytes.
// joint_weights_kernel<B>: one workgroup of 256 threads per packet.  v_b[c] = the mean of the two sides at the carrier's
//   bin; vbar over all branches and data carriers by packet_vbar, the weight by noise_weight (gf3rx_demap.h): the rule of
//   gf3_combine_branches under `var`, stated there once.
#include "gf3rx_demap.h"

namespace {

// ------------------------------------------------------------------------------------------------------------ estimate
struct PilotNoiseArgs {
    FftTables t;
    const void* in; int64_t n_in; const int64_t* off;
    int CP, S, P, D;
    const cplx* inv_known;    // [K] 1/known symbol
    const cplx* H;            // [F][2][2][K] gf3_mimo_pilots' output
    double* var;              // [F][2][K]
    int* status;              // [F]
};

template <int NC, int DT>
__global__ __launch_bounds__(NC / 8) void mimo_pilot_noise_kernel(PilotNoiseArgs a) {
    extern __shared__ double2 smem[];
    constexpr int T = NC / 8, K = NC - 1;
    cplx* lds = smem;
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x, f = row >> 1;
    const int side = (int)(row & 1);
    const int P = a.P;
    double* out = a.var + row * K;
    const int64_t off = a.off[f];
    const int64_t body = (int64_t)(2 * P + a.D) * a.S;
    const bool ok = off >= 0 && body <= a.n_in && off <= a.n_in - body;     // gf3_mimo_pilots' rule
    if (side == 0 && tid == 0) a.status[f] = ok ? 0 : 1;
    if (!ok) {
        for (int i = tid; i < K; i += T) out[i] = NAN;
        return;
    }
    // the thread's own bins: 1 / X and the two columns, in Spec<NC> slot order
    const cplx* Hrow = a.H + row * (2 * K);
    cplx ik[8], h0[8], h1[8];
    double acc[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int k = Spec<NC>::bin(tid, s);                // (thread 0's slot 1 repeats a bin: read, never written)
        ik[s] = a.inv_known[k - 1];
        h0[s] = Hrow[k - 1];
        h1[s] = Hrow[K + k - 1];
        acc[s] = 0.0;
    }
    const int64_t base = off + (int64_t)(side ? P + a.D : 0) * a.S + a.CP + 2 * tid;
    RawPair<DT> next[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) next[r].load(a.in, base + 2 * r * T);
    FftTw<NC> ft;
    ft.init(tid, a.t.tw);
    const cplx wb = a.t.twn[tid];
    for (int p = 0; p < P; ++p) {
        cplx v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = next[r].get();
        if (p + 1 < P) {                                    // the next symbol's samples, in flight under this transform
#pragma unroll
            for (int r = 0; r < 8; ++r) next[r].load(a.in, base + (int64_t)(p + 1) * a.S + 2 * r * T);
        }
        if (p) {
            lds_barrier();                                  // every reader of the buffers is done
            ft.refresh();
        }
        cplx z0;
        rfft_regs<NC>(v, lds, ft, wb, tid, z0, p & 1);
        const double sg = (p & 1) ? -1.0 : 1.0;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const cplx e = csub(csub(cmul(v[s], ik[s]), h0[s]), cscale(h1[s], sg));
            acc[s] += e.x * e.x + e.y * e.y;
        }
    }
    const double scale = 1.0 / (double)(P - 2);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int k = Spec<NC>::bin(tid, s);
        if (Spec<NC>::live(tid, s)) out[k - 1] = acc[s] * scale;
    }
}

// ------------------------------------------------------------------------------------------------------------- weights
struct JointWeightArgs {
    const double* var[GF3_MAX_BRANCHES];    // [F][2][K]
    double* w;                              // [B][F][C]
    const int* bins;                        // [C] 1-based FFT bin of each data carrier
    int C, K;
};

// a branch's variance at data carrier c of packet f: the mean of the two pilot blocks' estimates
GF3_DEV double carrier_var(const double* var, int64_t f, int K, int bin) {
    return 0.5 * (var[(f * 2 + 0) * K + (bin - 1)] + var[(f * 2 + 1) * K + (bin - 1)]);
}

template <int B>
__global__ __launch_bounds__(VBAR_THREADS) void joint_weights_kernel(JointWeightArgs a) {
    __shared__ double red[VBAR_THREADS];
    const int t = threadIdx.x, C = a.C;
    const int64_t f = blockIdx.x, F = gridDim.x;
    // vbar: thread t adds v_b[t], v_b[t + 256], ... for b ascending, packet_vbar adds the 256 partial sums (combine_kernel's order)
    double s = 0.0;
#pragma unroll
    for (int b = 0; b < B; ++b)
        for (int c = t; c < C; c += VBAR_THREADS) s += carrier_var(a.var[b], f, a.K, a.bins[c]);
    const PacketNoise pn = packet_vbar(red, s, (double)B * (double)C);
#pragma unroll
    for (int b = 0; b < B; ++b)
        for (int c = t; c < C; c += VBAR_THREADS) {
            const double w = noise_weight(carrier_var(a.var[b], f, a.K, a.bins[c]), pn);
            a.w[((int64_t)b * F + f) * C + c] = is_fin(w) ? w : 0.0;
        }
}

}  // namespace

extern "C" int gf3_mimo_pilot_noise(gf3_ctx* c, const void* d_in, int64_t n_in, const int64_t* d_off, int64_t F, const void* d_H,
                                    double* d_var, int32_t* d_status, void* stream) {
    DeviceGuard dg(c);
    if (!c) return fail(c, GF3_EINVAL, "gf3_mimo_pilot_noise: null context");
    if (c->cfg.P < 4 || (c->cfg.P & 1))
        return fail(c, GF3_EINVAL, "gf3_mimo_pilot_noise: the two covers take two of the pilot symbols' degrees of freedom: an even "
                                   "number of pilot symbols, P >= 4 (P=%d)", c->cfg.P);
    if (F == 0) return GF3_OK;
    if (!d_in || !d_off || !d_H || !d_var || !d_status || F < 0 || n_in < 0)
        return fail(c, GF3_EINVAL, "gf3_mimo_pilot_noise: bad argument");
    if (const int rc = too_many_packets_i32(c, F, "gf3_mimo_pilot_noise")) return rc;
    PilotNoiseArgs a{FftTables{c->d_tw, c->d_twn}, d_in, n_in, d_off, c->cfg.CP, c->S, c->cfg.P, c->cfg.D, c->d_known,
                     (const cplx*)d_H, d_var, d_status};
    hipError_t e = hipSuccess;
    DISPATCH_NC(c->NC, c->cfg.in_dtype, e = launch((mimo_pilot_noise_kernel<NCC, DTC>), 2 * F, NCC / 8, fft_lds_bytes(NCC), (hipStream_t)stream, a));
    HIPCHK(c, e);
    return GF3_OK;
}

extern "C" int gf3_joint_noise_weights(gf3_ctx* c, int32_t B, const double* const* d_var, int64_t F, double* d_w, void* stream) {
    DeviceGuard dg(c);
    if (!c) return fail(c, GF3_EINVAL, "gf3_joint_noise_weights: null context");
    if (F == 0) return GF3_OK;
    if (!(branches_ok(B, d_var) && d_w && F >= 0))
        return fail(c, GF3_EINVAL, "gf3_joint_noise_weights: bad argument (1 <= B <= %d branches of variances; an output; F >= 0)",
                    GF3_MAX_BRANCHES);
    if (const int rc = too_many_packets_i32(c, F, "gf3_joint_noise_weights")) return rc;
    JointWeightArgs a{};
    for (int b = 0; b < B; ++b) a.var[b] = d_var[b];
    a.w = d_w;
    a.bins = c->d_bins;
    a.C = c->cfg.C; a.K = c->K;
    const hipError_t e = with_branches(B, [&](auto nb) {
        return launch((joint_weights_kernel<decltype(nb)::value>), F, VBAR_THREADS, 0, (hipStream_t)stream, a);
    });
    HIPCHK(c, e);
    return GF3_OK;
}
