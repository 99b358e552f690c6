// Host-side plumbing shared by the translation units of libgf3rx: kernel argument blocks, the context, error
// reporting, launch helpers and the launchers each kernel family exports to the units that hold the C ABI.
// Kernels live in per-family translation units compiled in parallel (gf3_audio_modem_amd/build.py):
//   gf3rx_fft.hip            rfft_kernel, tx_kernel
//   gf3rx_demod_{qpsk,scan,full,soft}.hip   the four modes of demod_kernel (gf3rx_demod.h)
//   gf3rx_demod_split.hip, gf3rx_dsplit_{qpsk,scan,full,soft}.hip   the two-phase demodulation of long packets
//   gf3rx_demod_screen.hip   demod_screen_kernel (fp32 data-symbol transforms under a bound, gf3rx_dscreen.h) and demod_listed_kernel, the fp64 pass over the packets it listed
//   gf3rx_corr.hip           corr_kernel, spec_kernel, ols_kernel
//   gf3rx_screen.hip         scr_ring_kernel, scr_ols_kernel, scr_refine_kernel (gf3rx_screen.h)
//   gf3rx_fscreen.hip        corr_screen_kernel: the fp32 screen of the frames-mode sync (gf3rx_fscreen.h)
//   gf3rx_stamp.cpp          the build stamp (source hash), recompiled on every change
//   gf3rx_sync.hip           pk_*, ck_*, scr list kernels + gf3_sync_stream*, gf3_sync_chunk, gf3_sync_decide (the peak rule they share with corr_kernel: gf3rx_peak.h)
//   gf3rx_detect.hip         det_* + gf3_detect_chunk, gf3_detect_decide: the self-normalised chirp detection (Pearson correlation of every
//                            window with the replica; on P of gf3rx_sync.hip's all-fp64 overlap-save)
//   gf3rx_ldpc.hip           ldpc_encode_kernel, ldpc_decode_kernel + gf3_ldpc_*
//   gf3rx_outer.hip          rs_encode_kernel, rs_recover_kernel + gf3_outer_encode, gf3_outer_recover (field arithmetic: gf3rx_outer.h)
//   gf3rx_crc.hip            crc_kernel + gf3_crc_attach, gf3_crc_check (per-codeword CRC-32)
//   gf3rx_noise.hip          noise_estimate_kernel, soft_demap_nw_kernel + gf3_noise_estimate, gf3_soft_demap_nw; their
//                            carrier x symbol forms and interleave_kernel + gf3_noise_estimate_cs, gf3_soft_demap_nw_cs, gf3_interleave
//                            (the soft-output arithmetic every unit from here to gf3rx_demap.hip shares is gf3rx_demap.h)
//   gf3rx_loading.hip        noise_estimate_loaded_kernel, soft_demap_loaded_kernel + gf3_loading_*, gf3_noise_estimate_loaded,
//                            gf3_soft_demap_loaded (adaptive bit loading: a QAM order per carrier, the noise pair for such a packet)
//   gf3rx_combine.hip        combine_kernel + gf3_combine_branches (receive diversity: maximal-ratio combining of B branches' symbols)
//   gf3rx_mimo.hip           mimo_pilots_kernel, mimo_detect_kernel + gf3_mimo_pilots, gf3_mimo_detect (2 x 2 spatial multiplexing: both
//                            columns of the channel from the covered pilots; joint max-log ML detection of the two streams;
//                            gf3_mimo_detect_known: the same detector told which coded bits are already known)
//   gf3rx_stbc.hip           stbc_slope_kernel, stbc_detect_kernel + gf3_stbc_slope, gf3_stbc_detect (transmit diversity: the Alamouti code over
//                            pairs of data symbols; one phase slope from all paths, joint max-log ML detection of a pair)
//   gf3rx_track.hip          track_phase_kernel + gf3_track_phase (per-symbol phase and timing tracking inside a packet)
//   gf3rx_feedback.hip       feedback_kernel + gf3_feedback_equalise (residual channel from re-encoded codewords, divided out)
//   gf3rx_blank.hip          blank_stats_kernel, blank_level_kernel, blank_write_kernel + gf3_blank_impulses (impulse blanking of the samples)
//   gf3rx_resample.hip       resample_kernel + gf3_resample_frames, gf3_resample_coefficients (sampling-clock correction of the packet
//                            bodies; the storage rounding it shares with gf3rx_blank.hip is gf3rx_storage.h);
//                            resample_stream_kernel + gf3_resample_stream (whole-stream rate conversion in front of the sync)
//   gf3rx_window.hip         window_kernel + gf3_window_frames (receive windowing: every symbol of the packet bodies tapered into
//                            its cyclic prefix, between the clock correction and demodulation)
//   gf3rx_denoise.hip        denoise_kernel + gf3_denoise_pilots (delay-domain denoising of the pilot sums ahead of the estimate stage)
//   gf3rx_papr.hip           papr_kernel + gf3_tone_reserve (transmit side: per data symbol, values for the carriers outside the
//                            data band that lower the symbol's peak; gf3_tx_frames_ex sends them in the filler's place)
//   gf3rx_demap.hip          the stand-alone demapper kernels, csi_weight_kernel + gf3_demap_hard, gf3_soft_demap(_csi); zero forcing (gf3_equalise_known_h)
//   gf3rx_sync_frames.hip    gf3_sync_frames*: the dispatch between corr_kernel and the fp32 screen, and its workspaces
//   gf3rx_ctx.hip            error text, gf3_ctx_create / gf3_ctx_destroy (table classification, plans; host arithmetic: gf3rx_plans.h), getters
//   gf3rx_abi.hip            the rest: gf3_rfft_batch, gf3_demod_frames(_ex, _dn), gf3_demod_frames_llr, gf3_equalise, gf3_tx_frames, Schmidl-Cox, gf3_unpack_bits
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <thread>
#include <type_traits>
#include <vector>

#include "gf3rx.h"
#include "gf3rx_device.h"
#include "gf3rx_screen_defs.h"

// ============================================================================
// kernel argument blocks
// ============================================================================
// Grid constellation whose bit labels split per axis (square Gray QAM, the reference QPSK):
// point = lvI[a] + j lvQ[b], label = labI[a] | labQ[b].  Distances then separate per axis, so
// hard decisions and max-log LLRs cost O(levels) instead of O(points).  n = 0: not separable.
struct SepTab {
    int nI, nQ;
    double lvI[8], lvQ[8];
    int labI[8], labQ[8];       // label bits contributed by each level (already in label position)
    int maskI;                  // label bits owned by the I axis
};

// The same kind of table when, in addition, the levels of each axis are equally spaced (square Gray QAM, the reference
// QPSK): the nearest level is then one rint() away.  Levels are numbered in ascending order here; pack holds the
// label bits the i-th level contributes, one byte each (mu <= 8).  nI = 0: not such a table.
struct UniGrid {
    int nI, nQ;
    double loI, invI, loQ, invQ;             // lowest level and 1 / spacing per axis
    unsigned long long packI, packQ;
};

struct FftTables {
    const cplx* tw;    // [NC]      exp(-2 pi i m / NC)
    const cplx* twn;   // [NC/2+1]  exp(-2 pi i k / N)
};

struct RfftArgs {
    FftTables t;
    const void* in; int64_t n_in; const int64_t* off; int dt;
    cplx* out;
};

struct DemodArgs {
    FftTables t;
    const void* in; int64_t n_in; const int64_t* off; int dt;
    int CP, S, P, D, K, C, mu, M;
    const cplx* inv_known;    // [K] 1/known symbol
    const int* pos;           // [K] data-carrier position or -1
    int contig_lo;            // >0: data bins are contig_lo .. contig_lo+C-1 in order (no table look-up)
    int ring;                 // symbols held by the decision-byte ring in LDS (power of two, see demod_ring)
    const double* cre; const double* cim; const int* clab;   // [M]
    int fit_lo, fit_hi;       // effective python-slice bounds, fit_hi <= K
    double xbar, inv_sxx;
    uint8_t* bits; int row_bytes;
    cplx* eq; cplx* Hs; cplx* He; double* slope; cplx* Hest; int* status;
    union {
        // spectra mode (receiver.equalise as a stand-alone stage): frequency-domain inputs
        struct {
            const cplx* sp_data;      // [F, D, K]
            const cplx* sp_start;     // [F, P, K]
            const cplx* sp_end;       // [F, P, K]
            cplx* eq_all;             // [F*D, K] equalised symbols on all carriers
        };
        // the screened QPSK demodulation (gf3rx_dscreen.h: time-domain input, bits only) keeps its pointers in the same
        // four slots, so that the block -- which the soft mode copies to its stack -- is the size it was
        struct {
            const cf* tw32;           // [NC | NC/2+1] the two twiddle tables rounded once to fp32, one after the other
            int* dwork;               // [count | pad to 16 ints | packet numbers]: the screen appends the packets it cannot
                                      // decide; demod_listed_kernel reads them: packet = dwork[16 + blockIdx.x], blockIdx.x < dwork[0]
            cf* dbg_ep; float* dbg_E; // optional (tests): [F][D][C] fp32 rotated symbols, [F][D] the bound
        };
    };
    double qpsk_q;            // >0: table is the reference QPSK table (+-q +-qj): decide by signs away from ties
    UniGrid ug;
    unsigned long long* stamps;   // diagnostic build only (-DGF3_STAMPS): [F][8] s_memtime per phase
    // two-phase form for long packets (gf3rx_demod_split.hip): the data stage runs nchunk workgroups per packet, each on
    // Dc consecutive data symbols, from the channel state the estimate stage left in Hs / He / slope
    int Dc, nchunk;
    const double* psum;       // [F][2][N] time-domain sums of each side's P pilot symbols (input of the estimate stage)
    // MODE_SOFT (gf3_demod_frames_llr; appended: the other modes' argument offsets are what they were).  `bits` is then the
    // float32 LLR array and row_bytes = 4 D C mu; ring = 0 (no decisions are staged).
    int soft;                 // 1: the soft mode is asked for (host dispatch)
    int soft_weight;          // 0: unit weight, 1: |Hest|^2
    int soft_kind;            // h of a binary-indexed 2^h x 2^h grid (maxlog_bin<h, h>), 0: maxlog_table
    int soft_stage;           // 1: a symbol's LLRs are staged in the FFT buffer (demod_soft_stages)
    SepTab sep;
};

#ifdef GF3_STAMPS
#define GF3_STAMP(i) do { if (a.stamps && threadIdx.x == 0) { unsigned long long t_; \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); a.stamps[blockIdx.x * 8 + (i)] = t_; } } while (0)
// slots 6 / 7: s_memrealtime (100 MHz) next to the first / last s_memtime stamp -> shader clock = d(memtime) / d(memrealtime) x 100 MHz
#define GF3_STAMP_RT(i) do { if (a.stamps && threadIdx.x == 0) { unsigned long long t_; \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); a.stamps[blockIdx.x * 8 + (i)] = t_; } } while (0)
#else
#define GF3_STAMP(i) do { } while (0)
#define GF3_STAMP_RT(i) do { } while (0)
#endif

// occupancy targets: min waves per SIMD handed to __launch_bounds__ (blocks of NC/8 threads).
// 2048 -> 3 blocks of 4 waves per CU (<=168 VGPRs), 4096 -> 1 block of 8 waves (<=256).
template <int NC> struct Occ { static constexpr int WPS = 2; };

struct CorrArgs {
    FftTables t;
    const void* in; int64_t n_in; int dt;
    const cplx* Hq;           // [Q][NC+1] spectra of the zero-padded chirp partitions
    int Q, Lp, Lc, Wmax;
    int64_t stride; int win_lo; int W;      // window f = chirp-start lags [f*stride + win_lo, +W)
    int64_t* starts; double* peak; double thresh;
    const int* list; const int* count;      // LISTED launches (the screened sync's unresolved windows): window = list[blockIdx.x], blockIdx.x < *count
};

// ============================================================================
// stream-mode matched filter: uniformly partitioned overlap-save with a spectral delay line
// (convolve(r, chirp[::-1]) over a whole stream, OFDM.py:357-358).
//   hop H = Lp (partition length).  Window j = samples [jH - (Lc-1), +N) is transformed ONCE
//   (spec_kernel); output block b = lags [bH, (b+1)H) of P is
//       P_b = irfft( sum_q  X_{b+q} . conj(H_q) )        (ols_kernel)
//   so the cost per H lags is one forward and one inverse transform plus Q spectrum MACs,
//   instead of Q+1 transforms.
// ============================================================================
#define OLS_B 3      /* output blocks per ols_kernel workgroup */
struct OlsArgs {
    FftTables t;
    const void* in; int64_t n_in; int dt;
    const cplx* Hq; int Q, H, Lc;
    cplx* spec;               // [NWIN][NC+1]
    int64_t nwin, plen;
    double* corr;
    double* part;             // [ols work items] maximum of the lags each workgroup wrote (the global max is max over these)
    int64_t nitems;           // logical work items of the launch (windows for spec_kernel, groups of OLS_B blocks for ols_kernel)
};

// ============================================================================
// transmit-side synthesiser: one packet per workgroup
// transmitter.map / build_OFDM_symbol / ifft / add_cp / send_to_stream (OFDM.py:196-259)
//   row f = [gap_f zeros | chirp Lc | P known symbols | D data symbols | P known symbols | zeros]
//   data symbol = 2 * irfft(X), X[bin] = point(label) on data carriers, filler on the others
// gf3_tx_frames_ex: `tones` given, data symbol (f, l) takes tones[f, l, rsv[bin - 1]] on the others instead; gain2 = 2 * body_gain
// is the gain of pilots and data (2.0 exactly for gf3_tx_frames: the same products as before it existed)
// ============================================================================
struct TxArgs {
    FftTables t;
    int CP, S, P, D, K, C, mu, M, Lc;
    const int* pos;               // [K] data position of a carrier or -1
    int contig_lo;
    const double* cre; const double* cim; const int* idx_of_label;   // label -> table index
    const cplx* filler;           // [K] value of a non-data carrier (indexed by carrier)
    const double* chirp;          // [Lc]
    const double* known_time;     // [S] one pilot symbol with its prefix, before the x2 gain
    const uint8_t* bits; int row_bytes;       // [F, row_bytes] packed payload (np.packbits order)
    const int64_t* gaps;          // [F] leading zeros of each row (may be null)
    void* out; int64_t stride; int out_dt;    // [F, stride] samples, f32 or f64
    const cplx* tones;            // [F, D, Ku] or null
    const int* rsv;               // [K] number of a carrier among the reserved ones (ascending bins) or -1 for a data carrier
    int Ku;
    double gain2;
};

// ============================================================================
// host side: context + C ABI
// ============================================================================
// a correlation plan has its own FFT size: the chirp search need not use the OFDM symbol's N
struct CorrPlan { int NC = 0, Q = 0, Lp = 0, W = 0; cplx* d_Hq = nullptr; FftTables t{nullptr, nullptr}; };

struct gf3_ctx {
    gf3_config cfg;
    int NC, K, S, Lc, row_bytes;
    int fit_lo, fit_hi;
    double xbar, inv_sxx;
    cplx *d_tw = nullptr, *d_twn = nullptr, *d_known = nullptr;
    cf* d_tw32 = nullptr;               // d_tw, then d_twn, rounded once to fp32: the screened demodulation's data-symbol transforms (gf3rx_dscreen.h)
    cplx *d_tw_x[2] = {nullptr, nullptr}, *d_twn_x[2] = {nullptr, nullptr};   // twiddles of plans whose FFT size != N
    int nc_x[2] = {0, 0};
    int *d_pos = nullptr, *d_clab = nullptr;
    int* d_bins = nullptr;              // [C] data_bins as given (1-based FFT bins in output order): gf3_track_phase's carrier offsets
    double bin_mean = 0.0;              // their mean
    int* d_bin_order = nullptr;         // [C] carrier index at each position of the ascending-bin order (gf3_feedback_equalise)
    int* d_bins_sorted = nullptr;       // [C] data_bins[d_bin_order[p]]
    double *d_cre = nullptr, *d_cim = nullptr;
    CorrPlan frames_plan, stream_plan;
    double qpsk_q = 0.0;
    int* d_idx_of_label = nullptr;
    int* d_rsv = nullptr;               // [K] number of a carrier among the Ku = K - C carriers outside data_bins, ascending, or -1 (gf3_tone_reserve)
    int Ku = 0;
    double* d_chirp = nullptr;
    double chirp_sum = 0.0, chirp_var = 0.0;   // Sc and Ec - Sc^2 / Lc of the replica (gf3rx_detect.hip)
    double* d_chirp_t = nullptr;  // the same taps in the order scr_refine_kernel's lanes consume them (RefineArgs::chirp_t)
    double* d_known_time = nullptr;     // one pilot symbol in the time domain (transmit side)
    SepTab sep{};
    UniGrid ug{};
    unsigned long long* stamps = nullptr;
    int contig_lo = 0;
    int device = 0;                     // HIP device the context (tables, plans) lives on
    int n_cu = 256;                     // its compute units (grid sizing of the persistent-style kernels)
    // single-precision screening plan of the stream-mode sync (gf3rx_screen.h); ok = false: always the fp64 path
    struct { bool ok = false; int Q = 0, H = 0; cf *d_tw = nullptr, *d_twn = nullptr; float4* d_Hs = nullptr;
             float *d_H0N = nullptr, *d_Hinf = nullptr;
             bool ring = false; float4* d_Hb = nullptr; float* d_ecoef = nullptr; int R_forced = 0; } scr;   // band-limited kernel (scr_ring_kernel)
    // single-precision screening plan of the frames-mode sync (gf3rx_fscreen.h): 2048-sample transforms, partitions of 2048 - wmax + 1 taps
    struct { bool ok = false; int Q = 0, Lp = 0, wmax = 0; cf *d_tw = nullptr, *d_twn = nullptr; float4* d_Hs = nullptr;
             float *d_H0N = nullptr, *d_Hinf = nullptr; } fscr;
    // Three things a call may write after gf3_ctx_create.  (i) The default evaluation mode of the legacy entry point
    // gf3_sync_stream (gf3_sync_stream_mode sets it; gf3_sync_stream_ex takes the mode per call and never reads it).
    // 0: by stream length (screen from GF3_SCR_MIN_SAMPLES on); 1: fp64 only; 2: screen whenever a plan exists; 3: as 2 with the general kernel
    std::atomic<int> default_stream_mode{0};
    // (ii) The list workspaces of the screened paths in auto mode, under ws_mu: per (stream, host thread) one
    // [count | pad | F numbers] buffer for the frames-mode sync's unresolved windows (slot WS_SYNC: gf3_sync_frames;
    // sync_frames_impl) and one for the QPSK demodulation's listed packets (slot WS_DEMOD: gf3_demod_frames_px) -- two
    // slots, because a demodulation queued behind a sync on the same stream must not overwrite the list the sync's fp64 pass
    // still reads.  Created on first use and grow-only.  Calls of one thread on one stream share a buffer through stream
    // order; other streams and other threads have their own.  A buffer that is outgrown may still be read by a queued
    // kernel: it goes to ws_retired, which gf3_ctx_destroy frees after a device synchronise.
    enum { WS_SYNC = 0, WS_DEMOD = 1, WS_SLOTS = 2 };
    struct Work { hipStream_t stream; std::thread::id thread; void* d[WS_SLOTS] = {nullptr, nullptr}; int64_t bytes[WS_SLOTS] = {0, 0}; };
    std::mutex ws_mu;
    std::vector<Work> ws_work;
    std::vector<void*> ws_retired;
    // (iii) The resampler's coefficient tables (gf3rx_resample.hip), [1025][2T] for T = 16 and T = 32: made on the first
    // gf3_resample_frames with that T, under ws_mu, entered in `owned`
    double* d_resample_h[2] = {nullptr, nullptr};
    std::vector<double> chirp;
    std::vector<cplx> known_pts;
    std::vector<void*> owned;           // every device allocation that lives as long as the context (gf3rx_ctx.hip)
};

// ============================================================================
// errors, device selection, launches
// ============================================================================
// Message of the calling thread's last failure.  One buffer per host thread, none in the context: concurrent calls
// on one context (different streams, different threads) cannot overwrite each other's text, and a failing call
// writes nothing into the context it was given.  (gf3rx_ctx.hip owns the buffer and `fail`.)
int fail(const gf3_ctx*, int code, const char* fmt, ...);
#define HIPCHK(c, x) do { hipError_t e_ = (x); if (e_ != hipSuccess) \
    return fail(c, GF3_EHIP, "%s failed: %s", #x, hipGetErrorString(e_)); } while (0)

// Every entry point that launches work runs on the context's device, whatever device the calling thread had
// current (kernels, copies and frees of a context created on cuda:1 must not land on cuda:0's streams).
struct DeviceGuard {
    int prev = -1; bool switched = false;
    explicit DeviceGuard(const gf3_ctx* c) {
        if (!c) return;
        if (hipGetDevice(&prev) == hipSuccess && prev != c->device) switched = hipSetDevice(c->device) == hipSuccess;
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};

constexpr size_t fft_lds_bytes(int NC) {
    return (size_t)((NC == 1024 || NC == 2048) ? 2 * NC : NC + NC / 8) * sizeof(cplx);
}
static_assert(fft_lds_bytes(512) == FftGeom<512>::LDS_ELEMS * sizeof(cplx) && fft_lds_bytes(1024) == FftGeom<1024>::LDS_ELEMS * sizeof(cplx) &&
              fft_lds_bytes(2048) == FftGeom<2048>::LDS_ELEMS * sizeof(cplx) && fft_lds_bytes(4096) == FftGeom<4096>::LDS_ELEMS * sizeof(cplx),
              "fft_lds_bytes restates FftGeom<NC>::LDS_ELEMS");

template <typename Kern, typename Args>
static hipError_t launch(Kern k, int64_t grid, int threads, size_t lds, hipStream_t st, const Args& a) {
    if (grid <= 0) return hipSuccess;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(threads), lds, st, a);
    return hipGetLastError();
}

// Kernels whose grid carries the packet in y: the refusal of a call with more packets than a grid's y extent.
inline int too_many_packets(const gf3_ctx* c, int64_t F, const char* who) {
    return F > 65535 ? fail(c, GF3_EINVAL, "%s: at most 65535 packets per call", who) : GF3_OK;
}
// Kernels whose grid carries the packet in x (two workgroups per packet at the most): at most 2^30 - 1 packets, so that
// the workgroup count stays a positive 32-bit number.
inline int too_many_packets_i32(const gf3_ctx* c, int64_t F, const char* who) {
    return F > 0x3fffffff ? fail(c, GF3_EINVAL, "%s: more than 2^30 - 1 packets in one call", who) : GF3_OK;
}
// 1 <= B <= GF3_MAX_BRANCHES, and every table given is there and holds B entries that are not null
template <typename... Tab>
inline bool branches_ok(int B, Tab... tabs) {
    if (B < 1 || B > GF3_MAX_BRANCHES || !(... && (tabs != nullptr))) return false;
    for (int b = 0; b < B; ++b)
        if (!(... && (tabs[b] != nullptr))) return false;
    return true;
}
// The one place where a branch count becomes a template argument: fn(std::integral_constant<int, B>) for a checked B, its
// result handed back (with_grid_bits' idiom, gf3rx_demap.h).
template <typename Fn>
inline auto with_branches(int B, Fn&& fn) {
    switch (B) {
        case 1: return fn(std::integral_constant<int, 1>{});
        case 2: return fn(std::integral_constant<int, 2>{});
        case 3: return fn(std::integral_constant<int, 3>{});
        default: return fn(std::integral_constant<int, 4>{});
    }
}
// Data symbols per workgroup of a kernel that streams a packet's D symbols, `per` workgroups per chunk of symbols (the
// packets, times the carrier tiles where a packet has several): about 8 workgroups per compute unit when there are
// packets enough; a handful of long packets is cut down to single symbols.
inline int symbols_per_group(const gf3_ctx* c, int64_t per, int D) {
    int64_t nchunk = (8 * (int64_t)c->n_cu + per - 1) / per;
    if (nchunk > D) nchunk = D;
    if (nchunk < 1) nchunk = 1;
    return (int)((D + nchunk - 1) / nchunk);
}
// The grid of such a kernel whose threads are carriers: ntile tiles of `threads` data carriers x chunks of `run` of the
// packet's `units` streamed units (symbols, or pairs of them) in x, the packet in y.
struct TileGrid { int ntile, run; dim3 grid; };
inline TileGrid tile_grid(const gf3_ctx* c, int64_t F, int units, int threads) {
    const int ntile = (c->cfg.C + threads - 1) / threads;
    const int run = symbols_per_group(c, F * ntile, units);
    return TileGrid{ntile, run, dim3((unsigned)(ntile * ((units + run - 1) / run)), (unsigned)F)};
}

#ifdef GF3_DEV_BUILD   /* developer iteration: only N=4096 with f32/f64 samples */
#define DISPATCH_DT(DTv, CALL)                                            \
    switch (DTv) {                                                        \
        case DT_F64: { constexpr int DTC = DT_F64; CALL; break; }         \
        default:     { constexpr int DTC = DT_F32; CALL; break; }         \
    }
#define DISPATCH_NC(NCv, DTv, CALL) { constexpr int NCC = 2048; DISPATCH_DT(DTv, CALL); }
#define DISPATCH_NC_F64(NCv, CALL) { constexpr int NCC = 2048; CALL; }
#else
#define DISPATCH_DT(DTv, CALL)                                            \
    switch (DTv) {                                                        \
        case DT_F64: { constexpr int DTC = DT_F64; CALL; break; }         \
        case DT_F32: { constexpr int DTC = DT_F32; CALL; break; }         \
        case DT_I16: { constexpr int DTC = DT_I16; CALL; break; }         \
        default:     { constexpr int DTC = DT_U8;  CALL; break; }         \
    }
#define DISPATCH_NC(NCv, DTv, CALL)                                       \
    switch (NCv) {                                                        \
        case 512:  { constexpr int NCC = 512;  DISPATCH_DT(DTv, CALL); break; }   \
        case 1024: { constexpr int NCC = 1024; DISPATCH_DT(DTv, CALL); break; }   \
        case 2048: { constexpr int NCC = 2048; DISPATCH_DT(DTv, CALL); break; }   \
        default:   { constexpr int NCC = 4096; DISPATCH_DT(DTv, CALL); break; }   \
    }
/* kernels that exist for f64 input only (spectra from memory, the estimate stage's pilot sums) */
#define DISPATCH_NC_F64(NCv, CALL)                                        \
    switch (NCv) {                                                        \
        case 512:  { constexpr int NCC = 512;  CALL; break; }             \
        case 1024: { constexpr int NCC = 1024; CALL; break; }             \
        case 4096: { constexpr int NCC = 4096; CALL; break; }             \
        default:   { constexpr int NCC = 2048; CALL; break; }             \
    }
#endif

// ============================================================================
// launchers exported by the kernel translation units
// ============================================================================
// gf3rx_fft.hip
hipError_t run_rfft_nc(int NCv, FftTables t, const void* d_in, int64_t n_in, int dt, const int64_t* d_off,
                       int64_t n_sym, cplx* d_out, hipStream_t st);
inline hipError_t run_rfft(const gf3_ctx* c, const void* d_in, int64_t n_in, int dt, const int64_t* d_off,
                           int64_t n_sym, cplx* d_out, hipStream_t st) {
    return run_rfft_nc(c->NC, FftTables{c->d_tw, c->d_twn}, d_in, n_in, dt, d_off, n_sym, d_out, st);
}
int tx_launch(gf3_ctx* c, const TxArgs& a, int64_t F, hipStream_t st);
// gf3rx_ctx.hip: the context's list workspace of the calling thread on this stream (slot: gf3_ctx::WS_*), at least `bytes`;
// nullptr: none can be had now (the stream is being captured and nothing large enough exists, the table is full, the
// allocation failed) -- the caller then runs its fp64 path
void* ctx_workspace(gf3_ctx* c, hipStream_t st, int slot, int64_t bytes);
// The list protocol the two screened dispatchers share (frames sync: sync_frames_impl, QPSK demodulation: demod_frames_impl).
// The screen appends what it cannot decide to a workspace [count | pad to LIST_HEAD bytes | F numbers] (int each); the
// dispatcher zeroes the head before the screen, and the fp64 pass reads the list.
enum { LIST_HEAD = 64 };
inline int64_t list_workspace_bytes(const gf3_ctx* c, int64_t F) {
    if (!c || F < 0) return 0;
    return (int64_t)((size_t)F * sizeof(int) + LIST_HEAD);
}
// What the calling thread's last call of a dispatcher did -- each keeps one thread_local record, like every other
// diagnostic -- and the answer to its *_last query: path 0 screened | 2 all fp64 | -1 no such call on this context and stream.
struct LastCall {
    const gf3_ctx* ctx = nullptr; void* stream = nullptr; int32_t path = -1, cap = 0;
    void set(const gf3_ctx* c, void* st, int32_t p, int32_t n) { ctx = c; stream = st; path = p; cap = n; }
    int query(const char* who, const gf3_ctx* c, void* st, int32_t* p, int32_t* n) const {
        if (!c || !p) return fail(c, GF3_EINVAL, "%s: null argument", who);
        const bool mine = ctx == c && stream == st;
        *p = mine ? path : -1;
        if (n) *n = mine ? cap : 0;
        return GF3_OK;
    }
};
// gf3rx_demod_screen.hip: the screened QPSK demodulation (gf3rx_dscreen.h) and the fp64 kernel on the packets it listed
bool demod_screen_applies(const gf3_ctx* c);
hipError_t launch_demod_screen(const gf3_ctx* c, const DemodArgs& a, int64_t F, hipStream_t st);
hipError_t launch_demod_listed(const gf3_ctx* c, const DemodArgs& a, int64_t F, hipStream_t st);
hipError_t launch_demod_verdicts(const int* dwork, int* cls, int64_t F, hipStream_t st);     // tests: cls[f] = 1 for listed f, else 0
// gf3rx_demod_{qpsk,scan,full}.hip: one packet per workgroup (time-domain input); `full` also serves the spectra mode
hipError_t launch_demod_qpsk(const gf3_ctx* c, const DemodArgs& a, int64_t F, hipStream_t st);
hipError_t launch_demod_scan(const gf3_ctx* c, const DemodArgs& a, int64_t F, hipStream_t st);
hipError_t launch_demod_full(const gf3_ctx* c, const DemodArgs& a, int64_t F, hipStream_t st);
hipError_t launch_demod_spectra(const gf3_ctx* c, const DemodArgs& a, int64_t F, hipStream_t st);
hipError_t launch_demod_soft(const gf3_ctx* c, const DemodArgs& a, int64_t F, hipStream_t st);      // gf3rx_demod_soft.hip: LLRs, no bits
// gf3rx_demod_split.hip + gf3rx_dsplit_{qpsk,scan,full}.hip: the two-phase form for long packets, few at a time
bool demod_wants_split(const gf3_ctx* c, int64_t F, int mode);
int demod_split(const gf3_ctx* c, DemodArgs a, int64_t F, void* d_work, hipStream_t st, double denoise = 0.0, double* d_report = nullptr);
hipError_t launch_pilot_sum(const gf3_ctx* c, const void* d_in, int64_t n_in, const int64_t* d_off, int64_t F, double* psum, hipStream_t st);
// gf3rx_denoise.hip: the delay-domain denoiser on pilot sums [F][2][N], in place (refuses P < 2 and a threshold that is not finite or <= 0)
int launch_denoise(const gf3_ctx* c, const void* d_in, int64_t n_in, const int64_t* d_off, int64_t F, double threshold,
                   double* d_psum, double* d_report, hipStream_t st);
hipError_t launch_dsplit_qpsk(const gf3_ctx* c, const DemodArgs& a, int64_t grid, hipStream_t st);
hipError_t launch_dsplit_scan(const gf3_ctx* c, const DemodArgs& a, int64_t grid, hipStream_t st);
hipError_t launch_dsplit_full(const gf3_ctx* c, const DemodArgs& a, int64_t grid, hipStream_t st);
hipError_t launch_dsplit_soft(const gf3_ctx* c, const DemodArgs& a, int64_t grid, hipStream_t st);
// gf3rx_corr.hip
hipError_t run_corr(const gf3_ctx* c, const CorrPlan& pl, const CorrArgs& a, int64_t grid, hipStream_t st, bool listed = false);
// gf3rx_fscreen.hip: the screened frames sync (fp32 with a bound per window; unresolved windows are listed for corr_kernel)
struct FScreenArgs;
hipError_t launch_fscreen(const gf3_ctx* c, const FScreenArgs& a, int64_t F, hipStream_t st);
hipError_t run_spec_ols(const CorrPlan& pl, OlsArgs a, int64_t nwin, int64_t nblk, hipStream_t st);   // spec_kernel, then ols_kernel
// gf3rx_sync.hip, for gf3rx_detect.hip: P of d_in [n] by the all-fp64 overlap-save of gf3_sync_stream, in a workspace of
// gf3_sync_stream_workspace_bytes(c, n) bytes (*P: where in it, n + Lc - 1 doubles); pk_scan on `n` counts; the read-back of a
// call's result words (valid until the calling thread's next one); {count, status} of a peak list -> *n_peaks or GF3_ERANGE
int stream_corr(const gf3_ctx* c, const void* d_in, int64_t n, void* d_work, double** P, hipStream_t st);
void launch_pk_scan(const int64_t* counts, int64_t n, int64_t* offsets, int64_t* total, hipStream_t st);
int read_back(const gf3_ctx* c, hipStream_t st, const void** h, const void* d_src, size_t bytes, const void* d_src2 = nullptr, size_t bytes2 = 0);
int finish_peaks(const gf3_ctx* c, const char* who, const int64_t* h, int64_t cap, int64_t* n_peaks);
// gf3rx_screen.hip
hipError_t launch_screen(const gf3_ctx* c, ScreenArgs a, bool general, hipStream_t st);
hipError_t launch_refine(const gf3_ctx* c, const RefineArgs& a, int64_t cap_cells, hipStream_t st);
