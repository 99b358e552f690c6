// libgf3rx -- tone reservation on the transmit side: per data symbol, values for the Ku carriers outside the data band
// (which no receiver reads in a data symbol) that lower the symbol's peak.  Clip-and-project iteration, stated once in
// NumPy in tests/papr_ref.py; gf3_tx_frames_ex sends the result in the filler's place.
//
// One workgroup per (packet, data symbol), the whole iteration in one launch.  A thread owns the same 8 bins in the
// inverse transform's packing (tx_kernel) and in the forward transform's split (rfft_regs) -- Spec<NC>'s mirrored pairs --
// so the spectrum, data and current tones, stays in its registers from start to end; LDS holds one in-place FFT buffer,
// which after an inverse transform is the time symbol, and 16 doubles for the reductions.  The best tones live in the
// output buffer: the owner of a bin rewrites it whenever an iterate improves on the best peak.  NC = 4096: 72 KiB + 128 B of
// the CU's 160 KiB.
#include "gf3rx_host.h"

struct PaprArgs {
    FftTables t;
    int D, K, C, mu, Ku;
    const int* pos; int contig_lo;
    const int* rsv;                   // [K] tone number of a carrier or -1
    const double* cre; const double* cim; const int* idx_of_label;
    const uint8_t* bits; int row_bytes;
    double lin_target, limit, step;   // 10^(target_db / 20), L = 10^(tone_limit_db / 20), N / (2 Ku)
    int iters;
    cplx* tones;                      // [F, D, Ku]
    double* report;                   // [F, D, 4] peak with zero tones, best peak, its iterate, rms of the best symbol
};

template <int NC>
__global__ __launch_bounds__(NC / 8, 2) void papr_kernel(PaprArgs a) {
    extern __shared__ double2 smem[];
    constexpr int T = NC / 8, N = 2 * NC;
    cplx* lds = smem;
    double* red = (double*)(smem + FftGeom<NC>::LDS_ELEMS_INPLACE);
    const int tid = threadIdx.x;
    const int64_t sym = blockIdx.x;
    const int64_t f = sym / a.D;
    const int l = (int)(sym - f * a.D);
    FftTw<NC> ft;
    ft.init(tid, a.t.tw);
    const cplx wb = a.t.twn[tid];
    const uint8_t* brow = a.bits + f * (int64_t)a.row_bytes;
    cplx* out = a.tones + sym * (int64_t)a.Ku;
    // this thread's bins in Spec<NC> slot order: the data points as tx_kernel reads them, zero tones, zero elsewhere
    cplx X[8];
    int slot[8];                                            // tone number of a reserved bin, else -1
    double e = 0.0;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int bn = Spec<NC>::bin(tid, s);
        X[s] = cmk(0.0, 0.0);
        slot[s] = -1;
        if (!Spec<NC>::live(tid, s) || bn < 1 || bn > a.K) continue;
        int ps;
        if (a.contig_lo > 0) ps = (bn >= a.contig_lo && bn < a.contig_lo + a.C) ? bn - a.contig_lo : -1;
        else ps = a.pos[bn - 1];
        if (ps < 0) { slot[s] = a.rsv[bn - 1]; continue; }
        const int o = (l * a.C + ps) * a.mu;                // (point_of of tx_kernel)
        const int b0 = o >> 3, bl = a.row_bytes - 1;
        uint32_t w = ((uint32_t)brow[b0] << 16) | ((uint32_t)brow[min(b0 + 1, bl)] << 8) | (uint32_t)brow[min(b0 + 2, bl)];
        const uint32_t lab = (w >> (24 - a.mu - (o & 7))) & ((1u << a.mu) - 1u);
        const int ix = a.idx_of_label[lab];
        X[s] = cmk(a.cre[ix], a.cim[ix]);
        e += X[s].x * X[s].x + X[s].y * X[s].y;
    }
    const double sigma = sqrt(2.0 * block_sum(e, red)) / (double)N;
    const double A = sigma * a.lin_target;
    const double sc = 1.0 / (double)NC;
    cplx v[8];
    double peak, ss;
    // x(R): the Hermitian packing and inverse transform of tx_kernel without the frame's gain.  Leaves the time symbol in
    // v (v[r] = x[2n] + i x[2n+1], n = tid + r T: the forward transform's input order), its peak and its sum of squares.
    auto synth = [&]() {
        const int tq = launder(tid);
        lds_barrier();                                      // the previous transform's last reads
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = Spec<NC>::bin(tq, 2 * r);
            const cplx P = X[2 * r];
            const cplx Bc = (k == NC - k) ? P : X[2 * r + 1];
            const cplx B = cconj(Bc);
            const cplx E = cscale(cadd(P, B), 0.5);
            const cplx Op = cmul_conj(cscale(csub(P, B), 0.5), Spec<NC>::pair_tw(tq, r, wb));
            const cplx Zk = cadd(E, mul_posi(Op));
            const cplx Zm = cadd(cconj(E), mul_posi(cconj(Op)));
            lds[k] = cconj(Zk);
            if (Spec<NC>::live(tq, 2 * r + 1)) lds[NC - k] = cconj(Zm);
        }
        if (tid == 0) lds[0] = cmk(0.0, 0.0);
        lds_barrier();
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = lds[tid + r * T];
        lds_barrier();
        ft.refresh();
        const cplx* yb = fft_core<NC, false>(v, lds, ft, launder(tid));
        double pk = 0.0, sq = 0.0;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const cplx z = yb[tid + r * T];
            v[r] = cmk(z.x * sc, -z.y * sc);
            pk = fmax(pk, fmax(fabs(v[r].x), fabs(v[r].y)));
            sq += v[r].x * v[r].x + v[r].y * v[r].y;
        }
        peak = block_max(pk, red);                          // (both in a fixed order: two calls give the same bytes)
        ss = block_sum(sq, red);
    };
    synth();
    const double peak0 = peak;
    double best = peak, best_ss = ss;
    int best_i = 0;
#pragma unroll
    for (int s = 0; s < 8; ++s)
        if (slot[s] >= 0) out[slot[s]] = cmk(0.0, 0.0);
    for (int i = 1; i <= a.iters; ++i) {
        if (!(peak > A)) break;                             // nothing is clipped: c is zero everywhere
#pragma unroll
        for (int r = 0; r < 8; ++r)                         // c = x - clip(x, -A, A)
            v[r] = cmk(v[r].x - fmin(fmax(v[r].x, -A), A), v[r].y - fmin(fmax(v[r].y, -A), A));
        cplx z0;
        ft.refresh();
        rfft_regs<NC, false>(v, lds, ft, wb, launder(tid), z0, 0);         // v[s] = fft(c)[bin(tid, s)]
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            if (slot[s] < 0) continue;
            cplx R = cmk(X[s].x - a.step * v[s].x, X[s].y - a.step * v[s].y);
            const double mag = np_cabs(R.x, R.y);
            if (mag > a.limit) R = cscale(R, a.limit / mag);
            X[s] = R;
        }
        synth();
        if (peak < best) {                                  // strictly: the first minimum wins
            best = peak; best_ss = ss; best_i = i;
#pragma unroll
            for (int s = 0; s < 8; ++s)
                if (slot[s] >= 0) out[slot[s]] = X[s];
        }
    }
    if (tid == 0) {
        double* row = a.report + sym * 4;
        row[0] = peak0; row[1] = best; row[2] = (double)best_i; row[3] = sqrt(best_ss / (double)N);
    }
}

extern "C" int gf3_tone_reserve(gf3_ctx* c, const uint8_t* d_bits_packed, int64_t F, double target_db, double tone_limit_db,
                                int32_t iterations, void* d_tones_c128, double* d_report, void* stream) {
    DeviceGuard dg(c);
    if (!c) return fail(c, GF3_EINVAL, "gf3_tone_reserve: null context");
    if (c->Ku == 0) return fail(c, GF3_EINVAL, "gf3_tone_reserve: every carrier is a data carrier, none is left to reserve (Ku = 0)");
    if (!(fabs(target_db) < INFINITY) || !(fabs(tone_limit_db) < INFINITY))
        return fail(c, GF3_EINVAL, "gf3_tone_reserve: target_db and tone_limit_db must be finite numbers");
    if (iterations < 0 || iterations > 64) return fail(c, GF3_EINVAL, "gf3_tone_reserve: iterations must lie in [0, 64], not %d", iterations);
    if (F == 0) return GF3_OK;
    const gf3_config& g = c->cfg;
    if (!d_bits_packed || !d_tones_c128 || !d_report || F < 0 || F > 0x7fffffff / g.D)
        return fail(c, GF3_EINVAL, "gf3_tone_reserve: bad argument");
    PaprArgs a{};
    a.t = {c->d_tw, c->d_twn};
    a.D = g.D; a.K = c->K; a.C = g.C; a.mu = g.mu; a.Ku = c->Ku;
    a.pos = c->d_pos; a.contig_lo = c->contig_lo; a.rsv = c->d_rsv;
    a.cre = c->d_cre; a.cim = c->d_cim; a.idx_of_label = c->d_idx_of_label;
    a.bits = d_bits_packed; a.row_bytes = c->row_bytes;
    a.lin_target = pow(10.0, target_db / 20.0); a.limit = pow(10.0, tone_limit_db / 20.0);
    a.step = (double)(2 * c->NC) / (2.0 * (double)c->Ku);
    a.iters = iterations;
    a.tones = (cplx*)d_tones_c128; a.report = d_report;
    hipStream_t st = (hipStream_t)stream;
    const int64_t grid = F * g.D;
    hipError_t e = hipSuccess;
    switch (c->NC) {
#ifndef GF3_DEV_BUILD
        case 512:  e = launch(papr_kernel<512>, grid, 64, (size_t)FftGeom<512>::LDS_ELEMS_INPLACE * sizeof(cplx) + 128, st, a); break;
        case 1024: e = launch(papr_kernel<1024>, grid, 128, (size_t)FftGeom<1024>::LDS_ELEMS_INPLACE * sizeof(cplx) + 128, st, a); break;
        case 4096: e = launch(papr_kernel<4096>, grid, 512, (size_t)FftGeom<4096>::LDS_ELEMS_INPLACE * sizeof(cplx) + 128, st, a); break;
#endif
        default:   e = launch(papr_kernel<2048>, grid, 256, (size_t)FftGeom<2048>::LDS_ELEMS_INPLACE * sizeof(cplx) + 128, st, a); break;
    }
    HIPCHK(c, e);
    return GF3_OK;
}
