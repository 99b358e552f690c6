// libgf3rx -- the C ABI (include/gf3rx.h) of the stages that have no unit of their own: the batched transform, the fused
// demodulation and its spectra form, the transmit synthesiser, Schmidl-Cox and PS + decode.  Map of the units: gf3rx_host.h.
#include "gf3rx_demod.h"

extern "C" int gf3_rfft_batch(gf3_ctx* c, const void* d_in, int64_t n_in, const int64_t* d_offsets, int64_t n_sym,
                              void* d_out, void* stream) {
    DeviceGuard dg(c);
    if (c && n_sym == 0) return GF3_OK;
    if (!c || !d_in || !d_offsets || !d_out || n_sym < 0) return fail(c, GF3_EINVAL, "gf3_rfft_batch: bad argument");
    HIPCHK(c, run_rfft(c, d_in, n_in, c->cfg.in_dtype, d_offsets, n_sym, (cplx*)d_out, (hipStream_t)stream));
    return GF3_OK;
}

// Everything a demodulation launch takes from the context; inputs, outputs and spectra pointers are left null for the caller.
static DemodArgs demod_args(const gf3_ctx* c) {
    const gf3_config& g = c->cfg;
    DemodArgs a{};
    a.t = {c->d_tw, c->d_twn}; a.dt = g.in_dtype;
    a.CP = g.CP; a.S = c->S; a.P = g.P; a.D = g.D; a.K = c->K; a.C = g.C; a.mu = g.mu; a.M = g.M;
    a.inv_known = c->d_known; a.pos = c->d_pos; a.contig_lo = c->contig_lo; a.ring = demod_ring(c);
    a.cre = c->d_cre; a.cim = c->d_cim; a.clab = c->d_clab;
    a.fit_lo = c->fit_lo; a.fit_hi = c->fit_hi; a.xbar = c->xbar; a.inv_sxx = c->inv_sxx;
    a.row_bytes = c->row_bytes; a.qpsk_q = c->qpsk_q; a.ug = c->ug;
    return a;
}

static thread_local LastCall g_demod_last;                    // (gf3_demod_frames_last)

// Whether precision -1 (auto: plain gf3_demod_frames, gf3_demod_frames_ex) takes the screened path where it applies.
// Decided by the same-box A/B of DESIGN 3.5 / 4; precision 1 asks for the screen explicitly either way.
#define GF3_DEMOD_AUTO_SCREEN 1

// [count | pad | listed packet numbers]
extern "C" int64_t gf3_demod_screen_workspace_bytes(const gf3_ctx* c, int64_t F) { return list_workspace_bytes(c, F); }

// precision 0: all fp64 (the reference of the screened path's tests).  1: the fp32 screen of the data symbols under a
// proven bound (gf3rx_dscreen.h), then the fp64 kernel on the packets it listed, whenever that applies -- the reference
// QPSK table, bits only (no eq, no Hest), the one-launch form, f32 / i16 / u8 storage, F <= INT_MAX and a list workspace
// to be had (the caller's `d_list` of gf3_demod_screen_workspace_bytes(F), else the context's per stream and host thread;
// none while the stream is being captured and nothing exists yet) -- and all fp64 otherwise.  -1 (auto): as 1 when
// GF3_DEMOD_AUTO_SCREEN, else as 0.  The outputs are the same every way.
static int demod_frames_impl(gf3_ctx* c, const void* d_in, int64_t n_in, const int64_t* d_off, int64_t F,
                             uint8_t* d_bits, void* d_eq, void* d_Hs, void* d_He, double* d_slope, void* d_Hest,
                             int32_t* d_status, void* d_work, int32_t mode, int32_t precision, void* d_list,
                             cf* dbg_ep, float* dbg_E, int32_t* dbg_cls, bool screen_only, void* stream) {
    DeviceGuard dg(c);
    if (c && F == 0) return GF3_OK;
    if (!c || !d_in || !d_off || !d_bits || F < 0 || mode < 0 || mode > 2 || precision < -1 || precision > 1)
        return fail(c, GF3_EINVAL, "gf3_demod_frames: bad argument");
    hipStream_t st = (hipStream_t)stream;
    DemodArgs a = demod_args(c);
    a.in = d_in; a.n_in = n_in; a.off = d_off; a.bits = d_bits; a.stamps = c->stamps;
    a.eq = (cplx*)d_eq; a.Hs = (cplx*)d_Hs; a.He = (cplx*)d_He; a.slope = d_slope; a.Hest = (cplx*)d_Hest; a.status = d_status;
    g_demod_last.set(c, stream, 2, 0);
    // long packets, few at a time: pilot sums, estimate and data symbols as three launches (gf3rx_demod_split.hip)
    if (d_work && demod_wants_split(c, F, mode)) {
        if (screen_only) return fail(c, GF3_EINVAL, "gf3_debug_demod_screen: the two-phase form is not screened");
        return demod_split(c, a, F, d_work, st);
    }
    const bool want_screen = precision == 1 || (precision == -1 && GF3_DEMOD_AUTO_SCREEN);
    void* list_ws = nullptr;
    if (want_screen && demod_screen_applies(c) && !d_eq && !d_Hest && F <= 0x7fffffff)
        list_ws = d_list ? d_list : ctx_workspace(c, st, gf3_ctx::WS_DEMOD, gf3_demod_screen_workspace_bytes(c, F));
    if (screen_only && !list_ws) return fail(c, GF3_EINVAL, "gf3_debug_demod_screen: the screen does not apply to this context");
    if (list_ws) {
        a.tw32 = c->d_tw32; a.dwork = (int*)list_ws; a.dbg_ep = dbg_ep; a.dbg_E = dbg_E;
        g_demod_last.set(c, stream, 0, (int32_t)F);
        HIPCHK(c, hipMemsetAsync(a.dwork, 0, LIST_HEAD, st));
        HIPCHK(c, launch_demod_screen(c, a, F, st));
        if (dbg_cls) HIPCHK(c, launch_demod_verdicts(a.dwork, dbg_cls, F, st));
        if (screen_only) return GF3_OK;
        HIPCHK(c, launch_demod_listed(c, a, F, st));
        return GF3_OK;
    }
    hipError_t e = hipSuccess;
    if (d_eq || d_Hest) e = launch_demod_full(c, a, F, st);
    else if (c->qpsk_q > 0.0) e = launch_demod_qpsk(c, a, F, st);
    else e = launch_demod_scan(c, a, F, st);
    HIPCHK(c, e);
    return GF3_OK;
}
extern "C" int gf3_demod_frames_px(gf3_ctx* c, const void* d_in, int64_t n_in, const int64_t* d_off, int64_t F,
                                   uint8_t* d_bits, void* d_eq, void* d_Hs, void* d_He, double* d_slope, void* d_Hest,
                                   int32_t* d_status, void* d_work, int32_t mode, int32_t precision, void* stream) {
    return demod_frames_impl(c, d_in, n_in, d_off, F, d_bits, d_eq, d_Hs, d_He, d_slope, d_Hest, d_status, d_work, mode, precision,
                             nullptr, nullptr, nullptr, nullptr, false, stream);
}
extern "C" int gf3_demod_frames_ex(gf3_ctx* c, const void* d_in, int64_t n_in, const int64_t* d_off, int64_t F,
                                   uint8_t* d_bits, void* d_eq, void* d_Hs, void* d_He, double* d_slope, void* d_Hest,
                                   int32_t* d_status, void* d_work, int32_t mode, void* stream) {
    return gf3_demod_frames_px(c, d_in, n_in, d_off, F, d_bits, d_eq, d_Hs, d_He, d_slope, d_Hest, d_status, d_work, mode, -1, stream);
}
extern "C" int gf3_demod_frames(gf3_ctx* c, const void* d_in, int64_t n_in, const int64_t* d_off, int64_t F,
                                uint8_t* d_bits, void* d_eq, void* d_Hs, void* d_He, double* d_slope, void* d_Hest,
                                int32_t* d_status, void* stream) {
    return gf3_demod_frames_px(c, d_in, n_in, d_off, F, d_bits, d_eq, d_Hs, d_He, d_slope, d_Hest, d_status, nullptr, 1, -1, stream);
}
// The two-phase form with the pilot sums denoised between its first and second launch (gf3rx_denoise.hip).
extern "C" int gf3_demod_frames_dn(gf3_ctx* c, const void* d_in, int64_t n_in, const int64_t* d_off, int64_t F,
                                   uint8_t* d_bits, void* d_eq, void* d_Hs, void* d_He, double* d_slope, void* d_Hest,
                                   int32_t* d_status, void* d_work, double threshold, double* d_report, void* stream) {
    DeviceGuard dg(c);
    if (!c) return fail(c, GF3_EINVAL, "gf3_demod_frames_dn: null context");
    if (c->cfg.P < 2) return fail(c, GF3_EINVAL, "gf3_demod_frames_dn: the noise is measured from the pilot repeats, P >= 2 (P=%d)", c->cfg.P);
    if (!(threshold > 0.0) || !(fabs(threshold) < INFINITY)) return fail(c, GF3_EINVAL, "gf3_demod_frames_dn: the threshold must be a finite number > 0");
    if (!d_work) return fail(c, GF3_EINVAL, "gf3_demod_frames_dn: null workspace (gf3_demod_workspace_bytes)");
    if (F == 0) return GF3_OK;
    if (!d_in || !d_off || !d_bits || F < 0) return fail(c, GF3_EINVAL, "gf3_demod_frames_dn: bad argument");
    DemodArgs a = demod_args(c);
    a.in = d_in; a.n_in = n_in; a.off = d_off; a.bits = d_bits; a.stamps = c->stamps;
    a.eq = (cplx*)d_eq; a.Hs = (cplx*)d_Hs; a.He = (cplx*)d_He; a.slope = d_slope; a.Hest = (cplx*)d_Hest; a.status = d_status;
    g_demod_last.set(c, stream, 2, 0);
    return demod_split(c, a, F, d_work, (hipStream_t)stream, threshold, d_report);
}
extern "C" int gf3_demod_frames_last(const gf3_ctx* c, void* stream, int32_t* path, int32_t* listed_capacity) {
    return g_demod_last.query("gf3_demod_frames_last", c, stream, path, listed_capacity);
}
// tests: the screening pass alone -- the fp32 rotated symbols of the data carriers [F][D][C] (data_bins order), the bound
// per symbol [F][D], the verdict per packet (0 decided, 1 listed), the listed packets in d_list; d_bits gets the screen's rows
extern "C" int gf3_debug_demod_screen(gf3_ctx* c, const void* d_in, int64_t n_in, const int64_t* d_off, int64_t F,
                                      uint8_t* d_bits, void* d_ep32, float* d_E, int32_t* d_cls, void* d_list, void* stream) {
    if (!d_list) return fail(c, GF3_EINVAL, "gf3_debug_demod_screen: null workspace");
    return demod_frames_impl(c, d_in, n_in, d_off, F, d_bits, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1,
                             d_list, (cf*)d_ep32, d_E, d_cls, true, stream);
}

// Samples to weighted max-log LLRs in one launch (MODE_SOFT of demod_kernel): what gf3_demod_frames(eq, Hs, He) +
// gf3_soft_demap_csi compute in three steps, without the eq round trip.  The max-log difference is defined for every
// table the context accepts (gf3_soft_demap applies no table condition either), so none is refused here.
extern "C" int gf3_demod_frames_llr(gf3_ctx* c, const void* d_in, int64_t n_in, const int64_t* d_off, int64_t F,
                                    float* d_llr, int32_t weight, void* d_Hs, void* d_He, double* d_slope, int32_t* d_status,
                                    void* d_work, int32_t mode, void* stream) {
    DeviceGuard dg(c);
    if (c && F == 0) return GF3_OK;
    if (!c || !d_in || !d_off || !d_llr || F < 0 || mode < 0 || mode > 2 || ((uintptr_t)d_llr & 3))
        return fail(c, GF3_EINVAL, "gf3_demod_frames_llr: bad argument");
    if (weight != 0 && weight != 1) return fail(c, GF3_EINVAL, "gf3_demod_frames_llr: weight must be 0 (unit) or 1 (|H^|^2)");
    DemodArgs a = demod_args(c);
    a.in = d_in; a.n_in = n_in; a.off = d_off; a.stamps = c->stamps;
    a.Hs = (cplx*)d_Hs; a.He = (cplx*)d_He; a.slope = d_slope; a.status = d_status;
    a.bits = (uint8_t*)d_llr; a.row_bytes = (int)sizeof(float) * c->cfg.D * c->cfg.C * c->cfg.mu; a.ring = 0;
    a.soft = 1; a.soft_weight = weight; a.sep = c->sep; a.soft_stage = demod_soft_stages(c) ? 1 : 0;
    a.soft_kind = grid_bits(c);
    if (d_work && demod_wants_split(c, F, mode)) return demod_split(c, a, F, d_work, (hipStream_t)stream);
    HIPCHK(c, launch_demod_soft(c, a, F, (hipStream_t)stream));
    return GF3_OK;
}

extern "C" int gf3_equalise(gf3_ctx* c, const void* d_data, const void* d_start, const void* d_end, int64_t F,
                            void* d_eq_all, void* d_Hs, void* d_He, double* d_slope, void* d_Hest,
                            uint8_t* d_bits, void* stream) {
    DeviceGuard dg(c);
    if (c && F == 0) return GF3_OK;
    if (!c || !d_data || !d_start || !d_end || !d_bits || F < 0) return fail(c, GF3_EINVAL, "gf3_equalise: bad argument");
    DemodArgs a = demod_args(c);
    a.bits = d_bits; a.Hs = (cplx*)d_Hs; a.He = (cplx*)d_He; a.slope = d_slope; a.Hest = (cplx*)d_Hest;
    a.sp_data = (const cplx*)d_data; a.sp_start = (const cplx*)d_start; a.sp_end = (const cplx*)d_end; a.eq_all = (cplx*)d_eq_all;
    const hipError_t e = launch_demod_spectra(c, a, F, (hipStream_t)stream);
    HIPCHK(c, e);
    return GF3_OK;
}

// d_tones [F, D, Ku] (gf3_tone_reserve) replaces the filler on the data symbols; body_gain scales pilots and data, not the chirp
extern "C" int gf3_tx_frames_ex(gf3_ctx* c, const uint8_t* d_bits_packed, const void* d_filler_c128, const int64_t* d_gaps,
                                int64_t F, void* d_out, int64_t stride, int32_t out_dtype, const void* d_tones_c128,
                                double body_gain, void* stream) {
    DeviceGuard dg(c);
    if (c && !(body_gain > 0.0 && body_gain < INFINITY)) return fail(c, GF3_EINVAL, "gf3_tx_frames: body_gain must be a finite number > 0");
    if (c && d_tones_c128 && c->Ku == 0) return fail(c, GF3_EINVAL, "gf3_tx_frames: tones given, but every carrier is a data carrier");
    if (c && F == 0) return GF3_OK;
    if (!c || !d_bits_packed || (!d_filler_c128 && !d_tones_c128) || !d_out || F < 0 || (out_dtype != GF3_F32 && out_dtype != GF3_F64))
        return fail(c, GF3_EINVAL, "gf3_tx_frames: bad argument");
    const gf3_config& g = c->cfg;
    if (stride < (int64_t)c->Lc + (int64_t)(2 * g.P + g.D) * c->S) return fail(c, GF3_EINVAL, "gf3_tx_frames: stride shorter than a packet");
    hipStream_t st = (hipStream_t)stream;
    TxArgs a{};
    a.t = {c->d_tw, c->d_twn};
    a.CP = g.CP; a.S = c->S; a.K = c->K; a.mu = g.mu; a.M = g.M; a.Lc = c->Lc;
    a.pos = c->d_pos; a.cre = c->d_cre; a.cim = c->d_cim; a.idx_of_label = c->d_idx_of_label; a.chirp = c->d_chirp;
    a.P = g.P; a.D = g.D; a.C = g.C; a.contig_lo = c->contig_lo; a.filler = (const cplx*)d_filler_c128;
    a.known_time = c->d_known_time; a.bits = d_bits_packed; a.row_bytes = c->row_bytes; a.gaps = d_gaps;
    a.out = d_out; a.stride = stride; a.out_dt = out_dtype == GF3_F32 ? DT_F32 : DT_F64;
    a.tones = (const cplx*)d_tones_c128; a.rsv = c->d_rsv; a.Ku = c->Ku; a.gain2 = 2.0 * body_gain;
    return tx_launch(c, a, F, st);
}
extern "C" int gf3_tx_frames(gf3_ctx* c, const uint8_t* d_bits_packed, const void* d_filler_c128, const int64_t* d_gaps,
                             int64_t F, void* d_out, int64_t stride, int32_t out_dtype, void* stream) {
    return gf3_tx_frames_ex(c, d_bits_packed, d_filler_c128, d_gaps, F, d_out, stride, out_dtype, nullptr, 1.0, stream);
}

// Schmidl & Cox timing metric (receiver.schmidlcox_method, OFDM.py:376-387)
//   P[0] = 0, P[d+1] = P[d] + r[d+L] r[d+2L] - r[d] r[d+L]; answer = first argmax |P| + N - 1
// One workgroup walks the search range in chunks: per-thread terms -> wave shuffle scan -> carry;
// the running arg-max keeps (|P|, smallest index) and is reduced across the block at the end.
struct ScArgs { const void* in; int dt; int64_t S; int L; int N; int64_t* out; };

__global__ __launch_bounds__(1024) void schmidl_cox_kernel(ScArgs a) {
    __shared__ double wsum[16];                // (its own scan, not block_scan: doubles, whose sum depends on the order
    __shared__ double bval[16];                //  carry + woff + (incl - run) -- an integer helper would re-associate it)
    __shared__ long long bidx[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int ITEMS = 4;
    double best = 0.0;                 // |P[0]| = 0 at index 0
    long long besti = 0;
    double carry = 0.0;
    for (int64_t base = 0; base < a.S - 1; base += 1024 * ITEMS) {
        const int64_t d0 = base + (int64_t)tid * ITEMS;
        double t[ITEMS], run = 0.0;
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            const int64_t d = d0 + k;
            double x = 0.0;
            if (d < a.S - 1) {
                const double r0 = load_sample(a.in, d, a.dt), r1 = load_sample(a.in, d + a.L, a.dt),
                             r2 = load_sample(a.in, d + 2 * a.L, a.dt);
                x = r1 * r2 - r0 * r1;
            }
            run += x;
            t[k] = run;                // inclusive prefix inside the thread
        }
        double incl = run;             // block-wide inclusive scan of the per-thread totals
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const double y = __shfl_up(incl, o, 64); if (lane >= o) incl += y; }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        double woff = 0.0, tot = 0.0;
        for (int w = 0; w < 16; ++w) { if (w < wave) woff += wsum[w]; tot += wsum[w]; }
        const double before = carry + woff + (incl - run);
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            const int64_t d = d0 + k;
            if (d < a.S - 1) {
                const double v = fabs(before + t[k]);      // |P[d+1]|
                if (v > best) { best = v; besti = d + 1; }
            }
        }
        carry += tot;
        __syncthreads();
    }
    // arg-max with first-index tie rule: wave reduction, then across waves
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double ov = __shfl_xor(best, o, 64);
        const long long oi = __shfl_xor(besti, o, 64);
        if (ov > best || (ov == best && oi < besti)) { best = ov; besti = oi; }
    }
    if (lane == 0) { bval[wave] = best; bidx[wave] = besti; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w)
            if (bval[w] > best || (bval[w] == best && bidx[w] < besti)) { best = bval[w]; besti = bidx[w]; }
        a.out[0] = besti + a.N - 1;
    }
}

extern "C" int gf3_schmidl_cox(gf3_ctx* c, const void* d_r, int64_t n, int64_t search_len, int64_t* d_index, void* stream) {
    DeviceGuard dg(c);
    if (!c || !d_r || !d_index || search_len < 2) return fail(c, GF3_EINVAL, "gf3_schmidl_cox: bad argument");
    const int L = c->K + 1;
    if (n < search_len - 1 + 2 * (int64_t)L) return fail(c, GF3_EINVAL, "gf3_schmidl_cox: stream shorter than search length + 2L");
    ScArgs a{d_r, c->cfg.in_dtype, search_len, L, 2 * c->NC, d_index};
    hipLaunchKernelGGL(schmidl_cox_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
    HIPCHK(c, hipGetLastError());
    return GF3_OK;
}
// PS + decode (OFDM.py:504-505, 541-544): packed decisions -> the int64 0/1 array the reference returns, whitening
// mask applied.  A thread owns two consecutive output elements (one 16-byte store; a wave writes 1 KB contiguously),
// which is what lets the destination be pinned HOST memory written over PCIe by the kernel itself.
struct UnpackArgs { const uint8_t* packed; int row_bytes; int64_t bpf, total; const uint8_t* mask; int n_mask; long long* out; };
__global__ __launch_bounds__(256) void unpack_bits_kernel(UnpackArgs a) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; 2 * t < a.total; t += stride) {
        long long v[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t e = 2 * t + h;                               // output index = global bit number
            const int64_t f = e / a.bpf, j = e - f * a.bpf;            // packet, bit inside the packet
            unsigned bit = e < a.total ? (a.packed[f * a.row_bytes + (j >> 3)] >> (7 - (int)(j & 7))) & 1u : 0u;
            if (a.mask) bit ^= a.mask[e % a.n_mask] & 1u;              // tile(mask)[:len] runs over the whole stream
            v[h] = (long long)bit;
        }
        if (2 * t + 1 < a.total) *(longlong2*)(a.out + 2 * t) = make_longlong2(v[0], v[1]);
        else a.out[2 * t] = v[0];
    }
}
extern "C" int gf3_unpack_bits(gf3_ctx* c, const uint8_t* d_bits, int64_t F, const uint8_t* d_mask, int32_t n_mask, void* out, void* stream) {
    DeviceGuard dg(c);
    if (c && F == 0) return GF3_OK;
    if (!c || !d_bits || !out || F < 0 || (d_mask && n_mask < 1) || ((uintptr_t)out & 15)) return fail(c, GF3_EINVAL, "gf3_unpack_bits: bad argument (out must be 16-byte aligned)");
    // where does `out` live?  Device memory is used as it is; pinned host memory through its device-side address; anything
    // else (pageable memory) cannot be written by a kernel
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, out) != hipSuccess) { (void)hipGetLastError(); return fail(c, GF3_EINVAL, "gf3_unpack_bits: out is neither device memory nor pinned host memory"); }
    void* dst = out;
    if (at.type == hipMemoryTypeHost) {
        dst = at.devicePointer;
        if (!dst) return fail(c, GF3_EINVAL, "gf3_unpack_bits: the pinned host buffer is not mapped into the device's address space");
    } else if (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged && at.type != hipMemoryTypeUnified)
        return fail(c, GF3_EINVAL, "gf3_unpack_bits: out is neither device memory nor pinned host memory");
    const int64_t bpf = (int64_t)c->cfg.D * c->cfg.C * c->cfg.mu;
    UnpackArgs a{d_bits, c->row_bytes, bpf, F * bpf, d_mask, n_mask, (long long*)dst};
    int64_t grid = (a.total / 2 + 255) / 256;
    if (grid > 8 * (int64_t)c->n_cu) grid = 8 * (int64_t)c->n_cu;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(unpack_bits_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
    HIPCHK(c, hipGetLastError());
    return GF3_OK;
}
