// libgf3rx -- 2 x 2 spatial multiplexing: the two-column pilot estimate (gf3_mimo_pilots) and the joint max-log ML
// detector of the two streams (gf3_mimo_detect, gf3_mimo_detect_nw with weights, gf3_mimo_detect_known with known bits).
// Not in the reference; see include/gf3rx.h and DESIGN.md §12.
//
// Wire format: speaker 0 sends chirps and pilots as ever, speaker 1 is silent during the chirps and negates its pilot
// symbols of odd index, so at microphone b   Y_p[k] = (H_b0[k] + (-1)^p H_b1[k]) X[k]   and, P being even,
//   cover t = mean_p (-1)^(t p) Y_p[k] / X[k] = H_bt[k],  t = 0, 1.
//
// mimo_pilots_kernel: one workgroup per (packet, side), NC/8 threads.  Both signed time-domain sums of the side's P pilot
//   symbols (prefix dropped, p ascending) are formed in registers from one pass over the samples, then transformed one
//   after the other (rfft_regs of gf3rx_device.h) and multiplied by 1 / (P known_k): two transforms instead of P.
// mimo_detect_kernel<B>: a workgroup owns 256 consecutive data carriers x Dc consecutive symbols of one packet pair;
//   thread = carrier (combine_kernel's shape).  Per carrier the 2 B magnitudes at both pilot blocks and the 2 B phasors
//   stay in registers; the phasors advance by one complex multiply per symbol.  Y is read straight from the spectra at
//   bin data_bins[c]: B x 16 bytes per cell, 16 bytes written.  Every sum runs in a fixed order, no atomics: two runs
//   give identical bytes.  NW (gf3_mimo_detect_nw): one weight per branch and carrier, read into a register ahead of the
//   symbol loop, multiplies that branch's term of every sum; a weight that is 0 or not finite takes the branch out at that
//   carrier.  The NW = false instantiations are the arithmetic they were.  KN (gf3_mimo_detect_known): one byte per coded
//   bit says whether the bit is known and one which it is, in the layout of the LLRs; a thread reads its 2 x 2 + 2 x 2 bytes
//   of a cell as four 2-byte loads and forms one 4-bit mask of admissible points per stream; a pair with an inadmissible
//   point enters the two reductions as INFINITY, a known bit leaves as -+GF3_LLR_KNOWN.  Selects and minima round nothing:
//   with nothing known the bytes are those of the KN = false instantiations, which are the code they were.
#include "gf3rx_joint.h"

namespace {

// ---------------------------------------------------------------------------------------------------------- pilots
struct MimoPilotArgs {
    FftTables t;
    const void* in; int64_t n_in; const int64_t* off;
    int CP, S, P, D;
    const cplx* inv_known;    // [K] 1/known symbol
    cplx* H;                  // [F][2][2][K]
    int* status;              // [F]
};

template <int NC, int DT>
__global__ __launch_bounds__(NC / 8) void mimo_pilots_kernel(MimoPilotArgs a) {
    extern __shared__ double2 smem[];
    constexpr int T = NC / 8, K = NC - 1;
    cplx* lds = smem;
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x, f = row >> 1;
    const int side = (int)(row & 1);
    const int P = a.P;
    cplx* out = a.H + row * (2 * K);
    const int64_t off = a.off[f];
    const int64_t body = (int64_t)(2 * P + a.D) * a.S;
    const bool ok = off >= 0 && body <= a.n_in && off <= a.n_in - body;
    if (side == 0 && tid == 0) a.status[f] = ok ? 0 : 1;
    if (!ok) {
        for (int i = tid; i < 2 * K; i += T) out[i] = cmk(NAN, NAN);
        return;
    }
    // the two signed sums, two pilot symbols' loads in flight at once
    cplx s0[8], s1[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) s0[r] = s1[r] = cmk(0.0, 0.0);
    const int64_t base = off + (int64_t)(side ? P + a.D : 0) * a.S + a.CP + 2 * tid;
    for (int p = 0; p < P; p += 2) {
        RawPair<DT> even[8], odd[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            even[r].load(a.in, base + (int64_t)p * a.S + 2 * r * T);
            odd[r].load(a.in, base + (int64_t)(p + 1) * a.S + 2 * r * T);
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const cplx xe = even[r].get(), xo = odd[r].get();
            s0[r] = cadd(cadd(s0[r], xe), xo);
            s1[r] = csub(cadd(s1[r], xe), xo);
        }
    }
    FftTw<NC> ft;
    ft.init(tid, a.t.tw);
    const cplx wb = a.t.twn[tid];
    const double invP = 1.0 / (double)P;
    cplx z0;
    rfft_regs<NC>(s0, lds, ft, wb, tid, z0, 0);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int k = Spec<NC>::bin(tid, s);
        if (Spec<NC>::live(tid, s)) out[k - 1] = cmul(cscale(s0[s], invP), a.inv_known[k - 1]);
    }
    lds_barrier();                                          // every reader of the buffers is done
    ft.refresh();
    rfft_regs<NC>(s1, lds, ft, wb, tid, z0, 1);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int k = Spec<NC>::bin(tid, s);
        if (Spec<NC>::live(tid, s)) out[K + k - 1] = cmul(cscale(s1[s], invP), a.inv_known[k - 1]);
    }
}

// ---------------------------------------------------------------------------------------------------------- detector
struct MimoDetectArgs {
    const cplx* Y[GF3_MAX_BRANCHES];        // [F*D][NB]
    const cplx* H[GF3_MAX_BRANCHES];        // [F][2][2][K]
    const double* slope[GF3_MAX_BRANCHES];  // [F]
    float* llr;                             // [F][2][D][C][2]
    const int* bins;                        // [C] 1-based FFT bin of each data carrier
    int D, C, K, NB, P, Dc, ntile;
    const double* cre; const double* cim; const int* clab;      // the 4 points and their labels
    const double* wgt;                      // NW: [B][F][C] the branches' weights (gf3_joint_noise_weights)
    const uint8_t* bits; const uint8_t* known;                  // KN: [F][2][D][C][2] a bit's value, whether it is known
};

// the two bytes of one stream's symbol at a cell (any alignment: the planes are byte arrays)
struct BytePair { uint8_t v[2]; };
GF3_DEV BytePair byte_pair(const uint8_t* p, int64_t cell) {
    BytePair r;
    __builtin_memcpy(&r, p + 2 * cell, 2);
    return r;
}

template <int B, bool NW, bool KN>
__global__ __launch_bounds__(JOINT_THREADS) void mimo_detect_kernel(MimoDetectArgs a) {
    const int t = threadIdx.x;
    const int tile = blockIdx.x % a.ntile, chunk = blockIdx.x / a.ntile;
    const int64_t f = blockIdx.y;
    const int c = tile * JOINT_THREADS + t;
    if (c >= a.C) return;
    const int bin = a.bins[c];
    const int D = a.D, P = a.P;
    const int l0 = chunk * a.Dc, l1 = min(l0 + a.Dc, D);
    const double n = (double)(bin - 1);
    const double f0 = (l0 + P / 2.0) / (double)(D + P);
    // per-carrier state of the 2 B entries: |Hs|, |He| and the phasor at symbol l0; per branch the phasor's step
    double ms[B][2], me[B][2];
    cplx w[B][2], step[B];
    bool okh[B];
    double wt[B];
#pragma unroll
    for (int b = 0; b < B; ++b) {
        const double sl = a.slope[b][f];
        okh[b] = is_fin(sl);
        wt[b] = 1.0;
        if constexpr (NW) {
            wt[b] = a.wgt[((int64_t)b * gridDim.y + f) * a.C + c];
            okh[b] = okh[b] && is_fin(wt[b]) && wt[b] != 0.0;
        }
        const cplx rot = cis_fast(sl * n * f0);
        step[b] = cis_fast(sl * n / (double)(D + P));
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
    unsigned ones[2] = {0u, 0u};                            // KN: bit i of ones[k] <=> point i carries bit k as 1
    if constexpr (KN) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int k = 0; k < 2; ++k) ones[k] |= (unsigned)((lab[i] >> (1 - k)) & 1) << i;
    }

    for (int l = l0; l < l1; ++l) {
        const int64_t sym = f * D + l;
        const double fl = (l + P / 2.0) / (double)(D + P);  // the reference's f_l (channel_model): one division per symbol
        cplx y[B];
#pragma unroll
        for (int b = 0; b < B; ++b) y[b] = a.Y[b][sym * a.NB + bin];
        double G00 = 0.0, G11 = 0.0;
        cplx G01 = cmk(0.0, 0.0), m0 = cmk(0.0, 0.0), m1 = cmk(0.0, 0.0);
        bool any = false;
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const bool ok = okh[b] && is_fin(y[b].x) && is_fin(y[b].y);
            any = any || ok;
            const cplx h0 = cscale(w[b][0], ms[b][0] + (me[b][0] - ms[b][0]) * fl);
            const cplx h1 = cscale(w[b][1], ms[b][1] + (me[b][1] - ms[b][1]) * fl);
            cplx g = cmul_conj(h1, h0);                     // conj(h0) h1
            cplx a0 = cmul_conj(y[b], h0), a1 = cmul_conj(y[b], h1);
            double p0 = h0.x * h0.x + h0.y * h0.y, p1 = h1.x * h1.x + h1.y * h1.y;
            if constexpr (NW) {
                p0 *= wt[b]; p1 *= wt[b];
                g = cscale(g, wt[b]); a0 = cscale(a0, wt[b]); a1 = cscale(a1, wt[b]);
            }
            G00 += ok ? p0 : 0.0;
            G11 += ok ? p1 : 0.0;
            G01.x += ok ? g.x : 0.0;  G01.y += ok ? g.y : 0.0;
            m0.x += ok ? a0.x : 0.0;  m0.y += ok ? a0.y : 0.0;
            m1.x += ok ? a1.x : 0.0;  m1.y += ok ? a1.y : 0.0;
            w[b][0] = cmul(w[b][0], step[b]);
            w[b][1] = cmul(w[b][1], step[b]);
        }
        // the 16 metrics d[i][j] of (x0 = point i, x1 = point j), reduced once along each stream: best[0][i] is the minimum
        // over x1 with x0 = point i, best[1][j] the minimum over x0 with x1 = point j.  A bit of stream s then needs the
        // minimum of best[s] over the points that carry it as 1, and as 0 -- 8 selects per bit where the plain scan of the
        // pairs has 64.  (Minima round nothing: the numbers are those of the plain scan.)
        // KN: adm[s] bit i set <=> point i agrees with every known bit of stream s at this cell (never empty: 4 labels).  An
        // inadmissible point's own term A or Bj is INFINITY, and with it every pair's metric that holds the point; the
        // admissible pairs' metrics are the sums they were.
        BytePair kb[2], kk[2];
        unsigned adm[2] = {15u, 15u};
        if constexpr (KN) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int64_t cell = ((f * 2 + s) * D + l) * (int64_t)a.C + c;
                kb[s] = byte_pair(a.bits, cell);
                kk[s] = byte_pair(a.known, cell);
#pragma unroll
                for (int k = 0; k < 2; ++k)
                    if (kk[s].v[k] != 0) adm[s] &= kb[s].v[k] != 0 ? ones[k] : ~ones[k];
            }
        }
        double A[4], best[2][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            A[i] = G00 * (px[i] * px[i] + py[i] * py[i]) - 2.0 * (px[i] * m0.x + py[i] * m0.y);
            if constexpr (KN) A[i] = (adm[0] >> i) & 1u ? A[i] : INFINITY;
            best[0][i] = INFINITY;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double Bj = G11 * (px[j] * px[j] + py[j] * py[j]) - 2.0 * (px[j] * m1.x + py[j] * m1.y);
            if constexpr (KN) Bj = (adm[1] >> j) & 1u ? Bj : INFINITY;
            const cplx q = cmul(G01, cmk(px[j], py[j]));
            best[1][j] = INFINITY;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double d = A[i] + Bj + 2.0 * (px[i] * q.x + py[i] * q.y);
                best[0][i] = fmin(best[0][i], d);
                best[1][j] = fmin(best[1][j], d);
            }
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
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
                if constexpr (KN)
                    if (kk[s].v[k] != 0) out[k] = kb[s].v[k] != 0 ? -GF3_LLR_KNOWN : GF3_LLR_KNOWN;
            }
            store_llr<2>(a.llr, ((f * 2 + s) * D + l) * (int64_t)a.C + c, out);
        }
    }
}

}  // namespace

extern "C" int gf3_mimo_pilots(gf3_ctx* c, const void* d_in, int64_t n_in, const int64_t* d_off, int64_t F, void* d_H_out,
                               int32_t* d_status, void* stream) {
    DeviceGuard dg(c);
    if (!c) return fail(c, GF3_EINVAL, "gf3_mimo_pilots: null context");
    if (const int rc = needs_even_cover(c, "gf3_mimo_pilots")) return rc;
    if (F == 0) return GF3_OK;
    if (!d_in || !d_off || !d_H_out || !d_status || F < 0 || n_in < 0) return fail(c, GF3_EINVAL, "gf3_mimo_pilots: bad argument");
    if (const int rc = too_many_packets_i32(c, F, "gf3_mimo_pilots")) return rc;
    MimoPilotArgs a{FftTables{c->d_tw, c->d_twn}, d_in, n_in, d_off, c->cfg.CP, c->S, c->cfg.P, c->cfg.D, c->d_known,
                    (cplx*)d_H_out, d_status};
    hipError_t e = hipSuccess;
    DISPATCH_NC(c->NC, c->cfg.in_dtype, e = launch((mimo_pilots_kernel<NCC, DTC>), 2 * F, NCC / 8, fft_lds_bytes(NCC), (hipStream_t)stream, a));
    HIPCHK(c, e);
    return GF3_OK;
}

// the entries of the detector: `who` names the caller in a refusal, d_w is null for the unweighted ones, KN takes the planes
template <bool NW, bool KN>
static int mimo_detect_call(gf3_ctx* c, const char* who, int32_t B, const void* const* d_Y, const void* const* d_H,
                            const double* const* d_slope, const double* d_w, const uint8_t* d_bits, const uint8_t* d_known,
                            int64_t F, float* d_llr, void* stream) {
    DeviceGuard dg(c);
    if (!c) return fail(c, GF3_EINVAL, "%s: null context", who);
    if (const int rc = needs_4_points(c, who)) return rc;
    if (F == 0) return GF3_OK;
    if (!(branches_ok(B, d_Y, d_H, d_slope) && d_llr && F >= 0 && (!NW || d_w) && (!KN || (d_bits && d_known))))
        return fail(c, GF3_EINVAL, "%s: bad argument (1 <= B <= %d branches, each with spectra, estimates and slopes; %s%s"
                                   "an output; F >= 0)", who, GF3_MAX_BRANCHES, NW ? "the weights; " : "",
                    KN ? "the planes of the bits and of what is known; " : "");
    if (const int rc = too_many_packets(c, F, who)) return rc;
    MimoDetectArgs a{};
    for (int b = 0; b < B; ++b) { a.Y[b] = (const cplx*)d_Y[b]; a.H[b] = (const cplx*)d_H[b]; a.slope[b] = d_slope[b]; }
    a.llr = d_llr;
    a.bins = c->d_bins;
    a.D = c->cfg.D; a.C = c->cfg.C; a.K = c->K; a.NB = c->NC + 1; a.P = c->cfg.P;
    const TileGrid g = tile_grid(c, F, a.D, JOINT_THREADS);
    a.ntile = g.ntile; a.Dc = g.run;
    a.cre = c->d_cre; a.cim = c->d_cim; a.clab = c->d_clab;
    a.wgt = d_w;
    a.bits = d_bits; a.known = d_known;
    with_branches(B, [&](auto nb) {
        hipLaunchKernelGGL((mimo_detect_kernel<decltype(nb)::value, NW, KN>), g.grid, dim3(JOINT_THREADS), 0, (hipStream_t)stream, a);
    });
    HIPCHK(c, hipGetLastError());
    return GF3_OK;
}

extern "C" int gf3_mimo_detect(gf3_ctx* c, int32_t B, const void* const* d_Y, const void* const* d_H, const double* const* d_slope,
                               int64_t F, float* d_llr, void* stream) {
    return mimo_detect_call<false, false>(c, "gf3_mimo_detect", B, d_Y, d_H, d_slope, nullptr, nullptr, nullptr, F, d_llr, stream);
}

extern "C" int gf3_mimo_detect_nw(gf3_ctx* c, int32_t B, const void* const* d_Y, const void* const* d_H, const double* const* d_slope,
                                  const double* d_w, int64_t F, float* d_llr, void* stream) {
    return mimo_detect_call<true, false>(c, "gf3_mimo_detect_nw", B, d_Y, d_H, d_slope, d_w, nullptr, nullptr, F, d_llr, stream);
}

extern "C" int gf3_mimo_detect_known(gf3_ctx* c, int32_t B, const void* const* d_Y, const void* const* d_H,
                                     const double* const* d_slope, const double* d_w, const uint8_t* d_bits, const uint8_t* d_known,
                                     int64_t F, float* d_llr, void* stream) {
    const char* who = "gf3_mimo_detect_known";
    return d_w ? mimo_detect_call<true, true>(c, who, B, d_Y, d_H, d_slope, d_w, d_bits, d_known, F, d_llr, stream)
               : mimo_detect_call<false, true>(c, who, B, d_Y, d_H, d_slope, nullptr, d_bits, d_known, F, d_llr, stream);
}
