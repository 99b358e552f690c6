/*
 * gf3rx.h -- C ABI of the MI355X-native OFDM receive-path engine (libgf3rx.so).
 *
 * This is the drop-in boundary for the demodulation path of the GF3 audio
 * modem.  The reference has no FFI of its own (it is one Python file); the
 * boundary is the set of methods of class `receiver` in /root/reference/OFDM.py
 * that `receiver.receive` (OFDM.py:581-657) strings together.  Each entry
 * point below names the reference method(s) it replaces.  INTEGRATION.md shows
 * the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C, no exceptions; every call returns 0 (GF3_OK) or a negative
 *     gf3_status; gf3_last_error(ctx) holds a message for the last failure.
 *   - every `d_*` pointer is DEVICE memory owned by the caller (e.g. a
 *     torch tensor's data_ptr()); the library owns only the context and its
 *     look-up tables.  `stream` is a hipStream_t passed as void* (NULL = the
 *     default stream).  All work is enqueued asynchronously on that stream;
 *     only gf3_sync_stream synchronises (it returns a count to the host).
 *   - a context's tables and plans are immutable after creation, so
 *     concurrent calls on one context from different host threads / on
 *     different streams are safe (every call brings its own workspace and
 *     outputs; error text and diagnostics are kept per calling THREAD, not in
 *     the context, and so are the 256 bytes of pinned host memory the calls
 *     that return counts read them back into).  Two exceptions: the legacy convenience
 *     gf3_sync_stream_mode, which stores a default mode for the legacy entry
 *     point gf3_sync_stream (gf3_sync_stream_ex takes the mode per call), and
 *     the small workspaces gf3_sync_frames keeps in the context, one per
 *     (stream, host thread), under a mutex of the context's own.
 *   - complex128 arrays are interleaved (re, im) doubles, as NumPy stores them.
 *   - every typed array is aligned as its element type is.  Every workspace
 *     (`d_work`, `d_list`) must be 16-BYTE ALIGNED: the library carves int32 /
 *     int64 counts, doubles and complex128 arrays out of it at offsets that keep
 *     each type's alignment and reads the counts as aligned words.  It cannot check
 *     the size of a device pointer and does not check this either: a workspace
 *     off that alignment gives counts and offsets read from the wrong bytes,
 *     and indices computed from them are not bounded.
 */
#ifndef GF3RX_H
#define GF3RX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GF3RX_VERSION "0.1.0"

typedef enum {
    GF3_OK = 0,
    GF3_EINVAL = -1,      /* bad argument / unsupported geometry            */
    GF3_EHIP = -2,        /* a HIP runtime call failed                      */
    GF3_ENOMEM = -3,
    GF3_ERANGE = -4,      /* capacity of an output buffer exceeded          */
    GF3_ENODETECT = -5    /* sync found fewer than two chirps (the reference
                             dies in np.vstack([]) here, OFDM.py:400)       */
} gf3_status;

/* storage type of the input sample stream (samples are widened to fp64 in
 * registers; all arithmetic is fp64) */
typedef enum { GF3_F64 = 0, GF3_F32 = 1, GF3_I16 = 2, GF3_U8 = 3 } gf3_dtype;

/*
 * Engine configuration == the attributes CamG.__init__ sets (OFDM.py:18-101),
 * generalised: any N in {1024,2048,4096,8192}, any CP, any constellation.
 */
typedef struct {
    int32_t N;                  /* ofdm_symbol_size            OFDM.py:27   */
    int32_t CP;                 /* cp_length                   OFDM.py:42   */
    int32_t P;                  /* no_pilots (each side), >=1  OFDM.py:51   */
    int32_t D;                  /* packet_length               OFDM.py:50   */
    int32_t Lc;                 /* chirp_length; 0 => 5*(N+CP) OFDM.py:64   */
    double  fs, f0, f1;         /* 48000, 0, 8000              OFDM.py:24,62-63 */
    double  thresh;             /* 0.4                         OFDM.py:361  */
    int32_t fit_lo, fit_hi;     /* 500, 1000 (python slice)    OFDM.py:462  */
    int32_t mu;                 /* bits per constellation point             */
    int32_t M;                  /* constellation size (<= 64)               */
    const double  *const_re;    /* [M] points in mapping_table insertion    */
    const double  *const_im;    /*     order                   OFDM.py:72-77 */
    const uint8_t *const_bits;  /* [M*mu] bit labels, tuple order           */
    const double  *known_re;    /* [K] map(known_sequence[:K*mu]) OFDM.py:429 */
    const double  *known_im;    /*     K = N/2-1                            */
    const int32_t *data_bins;   /* [C] data_carriers (FFT bin numbers 1..K),
                                   output bit order follows this array  OFDM.py:47,603 */
    int32_t C;
    int32_t in_dtype;           /* gf3_dtype of the sample stream           */
    int32_t max_window;         /* largest search window (lags) gf3_sync_frames
                                   will be asked for; 0 => 512               */
} gf3_config;

typedef struct gf3_ctx gf3_ctx;

const char *gf3_version(void);
/* SHA-256 (hex) of the sources + compiler flags this binary was built from, "unknown" for a build made by hand */
const char *gf3_source_hash(void);

/* replaces CamG.__init__ + sync_chirp (OFDM.py:18-109): builds twiddles, the
 * chirp replica and its partition spectra, demap tables, on the current device */
int gf3_ctx_create(const gf3_config *cfg, gf3_ctx **out);
void gf3_ctx_destroy(gf3_ctx *ctx);
/* message of the CALLING THREAD's last failed call (the argument is ignored: nothing is stored in a context) */
const char *gf3_last_error(const gf3_ctx *ctx);
/* Returns and CLEARS the HIP runtime's sticky last error of the calling thread (0 = none).  For callers that made a HIP
 * call of their own that may fail by design -- e.g. pinning a read-only mapping with hipHostRegister before handing it
 * to the ingest path -- so that the refusal is not reported by the next unrelated launch check. */
int gf3_clear_runtime_error(void);

/* diagnostics: in a library built with -DGF3_STAMPS, gf3_demod_frames writes eight s_memtime
 * stamps per frame into this device buffer ([F][8] uint64); a no-op in the product build */
void gf3_debug_set_stamps(gf3_ctx *ctx, void *d_buf_u64);

/* derived sizes a caller needs to allocate outputs */
int32_t gf3_bytes_per_frame(const gf3_ctx *ctx);     /* ceil(D*C*mu/8)            */
int32_t gf3_sync_max_window(const gf3_ctx *ctx);     /* lags one gf3_sync_frames block resolves */
int64_t gf3_sync_stream_workspace_bytes(const gf3_ctx *ctx, int64_t n);

/* chirp replica, Lc doubles, copied to HOST memory (sync_chirp, OFDM.py:106-109) */
int gf3_chirp_replica(const gf3_ctx *ctx, double *h_out);

/*
 * remove_cp + np.fft.fft (OFDM.py:407-408, 593) on n_sym independent symbols.
 * d_offsets[i] = index (in samples, into d_in) of the first of the N samples of
 * symbol i (i.e. already past its cyclic prefix).  Output: [n_sym, N/2+1]
 * complex128, bins 0..N/2 of the unnormalised forward DFT.
 */
int gf3_rfft_batch(gf3_ctx *ctx, const void *d_in, int64_t n_in,
                   const int64_t *d_offsets, int64_t n_sym,
                   void *d_out_c128, void *stream);

/*
 * get_symbols + remove_cp + fft + get_data + equalise + data-carrier select +
 * demap + PS (OFDM.py:391-505, 593, 603) fused, one packet ("frame") per
 * workgroup.  d_frame_offsets[f] = sample index of the first pilot symbol's
 * cyclic prefix (what get_symbols computes as peak+2, OFDM.py:393).
 *
 *   d_bits_packed  [F, gf3_bytes_per_frame] uint8, MSB-first (np.packbits order),
 *                  bit order packet -> symbol -> data carrier -> bit (OFDM.py:505)
 *   d_eq           optional [F*D, C] complex128: equalised data-carrier symbols
 *   d_Hs, d_He     optional [F, K]   complex128: Hest_start / Hest_end (OFDM.py:450-451)
 *   d_slope        optional [F]      float64   : polyfit slope p (OFDM.py:462)
 *   d_Hest         optional [F, D, K] complex128: channel model (OFDM.py:471-475)
 * A frame whose samples fall outside [0, n_in) decodes to zero bits and sets
 * bit 0 of *d_status (optional int32 on the device); its rows of d_eq, d_Hs,
 * d_He, d_slope and d_Hest are NOT written (they keep what the caller put
 * there), in every form of the call below (_ex in both forms, _px, _dn, _llr).
 * The kernels only ever set bits in *d_status: the caller zeroes it.
 */
int gf3_demod_frames(gf3_ctx *ctx, const void *d_in, int64_t n_in,
                     const int64_t *d_frame_offsets, int64_t F,
                     uint8_t *d_bits_packed, void *d_eq, void *d_Hs, void *d_He,
                     double *d_slope, void *d_Hest, int32_t *d_status, void *stream);

/*
 * The same call with a workspace, which opens the TWO-PHASE form for LONG packets, FEW at a time -- the reference's
 * own geometry (no_pilots = 20, packet_length = 180, OFDM.py:18; three packets in Final System Test.ipynb cell 7), where
 * one packet per workgroup would leave the chip idle.  The triple loop of equalise (OFDM.py:466-478) is independent over
 * (symbol, carrier) once Hest_start, Hest_end and the slope exist (OFDM.py:443-462), so: the pilot symbols of each side
 * are summed in the time domain over F x 2 x N/512 workgroups, the channel estimate runs once per packet, and the
 * data symbols of a packet are spread over ceil(D / Dc) workgroups that each pack their own word-aligned bit range.
 * Outputs are those of gf3_demod_frames: Hs / He / slope bit for bit, equalised symbols to ~1e-13 (the phasor of a
 * chunk's first symbol is computed directly instead of by recurrence), bits identical.
 *   d_work   gf3_demod_workspace_bytes(ctx, F) bytes of device memory, or NULL (then always the one-launch kernel)
 *   mode     0: the library chooses by F and D (two-phase when F <= 2 x CUs and a packet cuts into >= 2 chunks of the
 *               length that fills the chip once -- the measured crossover, tools/ab/time_split.py)
 *            1: always the one-launch kernel      2: two-phase whenever d_work is given
 */
int64_t gf3_demod_workspace_bytes(const gf3_ctx *ctx, int64_t F);
/* what gf3_demod_frames_ex(F, mode) does when it is given a workspace: returns 1 for the two-phase form (0: one launch)
 * and stores the chunk length Dc (data symbols per workgroup) and the chunks per packet it would use */
int gf3_demod_split_plan(const gf3_ctx *ctx, int64_t F, int32_t mode, int32_t *h_Dc, int32_t *h_nchunk);
int gf3_demod_frames_ex(gf3_ctx *ctx, const void *d_in, int64_t n_in,
                        const int64_t *d_frame_offsets, int64_t F,
                        uint8_t *d_bits_packed, void *d_eq, void *d_Hs, void *d_He,
                        double *d_slope, void *d_Hest, int32_t *d_status,
                        void *d_work, int32_t mode, void *stream);

/*
 * The same call with the PRECISION of the QPSK data-symbol transforms chosen per call.  With the reference QPSK table and
 * bits-only output, what the caller receives from a data symbol is two sign bits per carrier, and on a usable signal
 * those sit orders of magnitude above the rounding of an fp32 transform.  The screened path keeps the whole pilot stage
 * (channel estimate, slope fit, phasors) in fp64 -- Hs, He and slope are bit for bit the fp64 kernel's --, transforms the
 * data symbols in fp32 with a proven error bound per symbol, and lists every packet in which a sign is not backed by the
 * bound; the fp64 kernel then runs on the listed packets.  The outputs are the all-fp64 outputs, bit for bit.
 *   precision  -1: auto (what gf3_demod_frames and gf3_demod_frames_ex mean): screened whenever the screen applies
 *               0: all fp64 on every packet (the reference the screened path is tested against)
 *               1: the explicit request for the screen: screened whenever the screen applies, whatever auto means in this
 *                  build (auto takes the screen because the A/B recorded in profiles/demod_screen_ab.json showed a clear gain)
 * The screen applies when the constellation is the reference QPSK table, neither d_eq nor d_Hest is asked for, the
 * one-launch form is chosen (the two-phase form is never screened), the samples are stored as f32, i16 or u8 (f64 is not:
 * fp32 does not hold it exactly), F <= 2^31 - 1, and a list workspace can be had.  The library keeps one such workspace per
 * (stream, calling host thread), created on first use and grow-only, next to the frames sync's and under the same rules:
 * nothing is allocated while the stream is being captured into a graph (call once with the largest F before capturing),
 * a failed allocation or a full table (64 per context) means the all-fp64 path, not an error.
 * COST ON NOISY INPUT: a listed packet is demodulated twice, and one unbacked sign among a packet's tens of thousands lists
 * it.  The bound is rigorous and therefore loose (about 1/230 of a QPSK part): nothing is listed on clean input and at 20 dB
 * of SNR, but at 10 dB and below MOST packets are, and the call then costs the fp32 pass plus nearly a whole fp64 pass --
 * slower than the all-fp64 path (DESIGN 3.5 has the measured shares and times).  precision = 0 is the way out for input
 * known to be that poor.
 *
 * gf3_demod_frames_last: what the CALLING THREAD's last gf3_demod_frames / _ex / _px call did, if that call was on this
 * context and stream, without a device read: *path = 0 screened, 2 all fp64, -1 no such call; *listed_capacity (optional)
 * = packets the fp64 pass of a screened call could take (F), 0 otherwise.
 */
int gf3_demod_frames_px(gf3_ctx *ctx, const void *d_in, int64_t n_in,
                        const int64_t *d_frame_offsets, int64_t F,
                        uint8_t *d_bits_packed, void *d_eq, void *d_Hs, void *d_He,
                        double *d_slope, void *d_Hest, int32_t *d_status,
                        void *d_work, int32_t mode, int32_t precision, void *stream);
int gf3_demod_frames_last(const gf3_ctx *ctx, void *stream, int32_t *path, int32_t *listed_capacity);

/*
 * Delay-domain denoising of the pilot channel estimate (not in the reference, whose least-squares estimate treats its K
 * carriers as K unknowns, OFDM.py:443-451; an acoustic channel has a few dozen to a few hundred significant taps).  Per
 * packet and per side (start / end pilot block), with tau = threshold and x_p[n] the N samples after the prefix of pilot
 * symbol p = 0 .. P-1, all in fp64:
 *     S[n] = sum_p x_p[n]                                      (the two-phase form's pilot sum, bit for bit)
 *     v    = sum_n sum_p (x_p[n] - S[n]/P)^2 / ((P-1) N)       (noise variance, from the pilot repeats)
 *     H_k  = rfft(S)_k / (P known_k), k = 1 .. K;  H_0 = H_{N/2} = 0;   h = irfft(H)     (N real taps)
 *     s2   = 2 v / (N P) sum_k 1/|known_k|^2                   (noise variance of one tap)
 *     tap n is kept iff h[n]^2 > tau s2 (strict);  kept = their number;  post = the largest kept n < N/2, -1 if none;
 *     pre = the largest N - n among kept n >= N/2, 0 if none
 *     the row stays bit for bit as it was (applied = 0) when v is not finite, when the packet does not lie inside the
 *     samples (its pilot sum is the zero row; reported as v = 0, kept = 0, post = -1, pre = 0), or when kept > N/4 (the
 *     channel is not sparse at this noise level; also noiseless input, where every tap is kept);
 *     else S' = irfft(X'), X'_k = rfft(h keep)_k P known_k for k = 1 .. K, X'_0 and X'_{N/2} as in rfft(S); applied = 1.
 *   d_report [F][2][5] float64 = {v, kept, post, pre, applied} per (packet, side), or NULL.  post and pre are the measured
 *   delay spread: whether the cyclic prefix is long enough.
 *   - gf3_denoise_pilots: the stage on its own (tests, tools): the pilot sums of the two-phase form, then the denoiser.
 *     d_psum_out [F][2][N] float64.
 *   - gf3_demod_frames_dn: gf3_demod_frames_ex in its two-phase form, always, with the denoiser run on the workspace's pilot
 *     sums between the first and the second launch; everything after that (estimate, slope fit, data stage, eq / Hest
 *     dumps) is the two-phase form as it stands, on the cleaner sums.  There is no fused-LLR variant and no fp32 screen.
 *     d_work of gf3_demod_workspace_bytes(ctx, F) is required.
 *   GF3_EINVAL (the text names the function) for a context with P < 2, a threshold that is not finite or <= 0, a NULL
 *   workspace (gf3_demod_frames_dn), a null pointer with F > 0, F < 0.  F == 0 is a no-op.  One workgroup per (packet,
 *   side), four transforms each; reductions in a fixed order, no atomics: two runs give identical bytes.
 */
int gf3_denoise_pilots(gf3_ctx *ctx, const void *d_in, int64_t n_in, const int64_t *d_frame_offsets, int64_t F,
                       double threshold, double *d_psum_out, double *d_report, void *stream);
int gf3_demod_frames_dn(gf3_ctx *ctx, const void *d_in, int64_t n_in,
                        const int64_t *d_frame_offsets, int64_t F,
                        uint8_t *d_bits_packed, void *d_eq, void *d_Hs, void *d_He,
                        double *d_slope, void *d_Hest, int32_t *d_status,
                        void *d_work, double threshold, double *d_report, void *stream);
/* tests: the screening pass alone.  d_ep32 [F][D][C] complex64: the rotated fp32 symbols (2 X conj(g)) of the data carriers
 * in data_bins order; d_E [F][D] float32: the bound of each symbol; d_cls [F] int32: 0 decided, 1 listed; d_list: AT LEAST
 * gf3_demod_screen_workspace_bytes(ctx, F) bytes, [count | pad to 64 bytes | listed packet numbers]; d_bits_packed gets the
 * screen's own rows.  Fails where the screen does not apply.  A packet whose samples fall outside [0, n_in) gets a zero row
 * of d_bits_packed and d_cls 0 and is not listed; its rows of d_ep32 and d_E are NOT written.  Of d_list the count word is
 * defined; the pad and the order of the entries behind it are not. */
int64_t gf3_demod_screen_workspace_bytes(const gf3_ctx *ctx, int64_t F);
/* tests: the fp32 transform of the screened demodulation alone (the same passes on single-precision points, the context's
 * twiddles rounded once): d_out_c64 [n_sym, N/2+1] complex64 spectra of the N samples at each offset, as gf3_rfft_batch
 * gives them in fp64.  f32 / i16 / u8 samples only. */
int gf3_debug_rfft_sp_batch(gf3_ctx *ctx, const void *d_in, int64_t n_in, const int64_t *d_offsets, int64_t n_sym,
                           void *d_out_c64, void *stream);
/* tests: the same of the instantiation the screened demodulation runs since it transforms two data symbols at a time:
 * workgroup w takes symbols 2w and 2w + 1 as the halves of one pair transform (an odd n_sym: the last pair's second half is
 * absent); output as above. */
int gf3_debug_rfft_sp_pair_batch(gf3_ctx *ctx, const void *d_in, int64_t n_in, const int64_t *d_offsets, int64_t n_sym,
                                void *d_out_c64, void *stream);
int gf3_debug_demod_screen(gf3_ctx *ctx, const void *d_in, int64_t n_in, const int64_t *d_frame_offsets, int64_t F,
                           uint8_t *d_bits_packed, void *d_ep32, float *d_E, int32_t *d_cls, void *d_list, void *stream);

/*
 * receiver.equalise as a stand-alone stage (OFDM.py:422-480): the same kernel
 * as gf3_demod_frames, fed with frequency-domain symbols instead of samples.
 *   d_data [F, D, K], d_start [F, P, K], d_end [F, P, K] complex128 (get_data's outputs)
 *   d_eq_all [F*D, K] complex128 (all carriers, as the reference returns)
 *   d_Hs, d_He, d_slope, d_Hest: as above, optional;  d_bits: packed decisions
 *   on the data carriers (required scratch/out, [F, gf3_bytes_per_frame]).
 */
int gf3_equalise(gf3_ctx *ctx, const void *d_data, const void *d_start, const void *d_end,
                 int64_t F, void *d_eq_all, void *d_Hs, void *d_He, double *d_slope,
                 void *d_Hest, uint8_t *d_bits, void *stream);

/*
 * chirp_method + the '+2' of get_symbols (OFDM.py:356-372, 393) for a batch of
 * independent frame buffers: frame f is searched for a chirp START in sample
 * range [f*stride + win_lo, f*stride + win_hi).  Peak rule as the reference:
 * correlation normalised by the window maximum, first local extremum above
 * `thresh`.  d_starts[f] = sample index of the first pilot symbol (chirp start +
 * Lc), ready to be passed to gf3_demod_frames; -1 where nothing qualifies.
 *
 * This entry point is gf3_sync_frames_ex in mode -1 (auto): the indices are those of the all-fp64 kernel, taken in fp32
 * wherever a proven bound decides them (see below), in a workspace the context owns.
 */
int gf3_sync_frames(gf3_ctx *ctx, const void *d_in, int64_t n_in,
                    int64_t F, int64_t stride, int32_t win_lo, int32_t win_hi,
                    int64_t *d_starts, double *d_peak_or_null, void *stream);

/*
 * The same search with the evaluation chosen per call.  The fp32 SCREEN (gf3rx_fscreen.h) evaluates every window in single
 * precision with a proven bound on |fp32 lag - exact lag| (2048-sample transforms held by one wave each, the chirp's
 * partition spectra multiplied in, one inverse transform) and takes the decision -- the index of the first extremum above
 * thresh x the window's maximum -- only where the bound decides it: every lag is certainly out, certainly in, or undecided,
 * and a window is resolved when no undecided lag precedes the first certain one.  Unresolved windows (noise at the threshold,
 * flat tops, non-finite samples, a maximum the bound cannot tell from zero) are listed on the device and the all-fp64 kernel
 * runs on exactly those.  No decision rests on an fp32 value the bound does not back: d_starts is what mode 0 writes.
 *   mode   -1: auto (== gf3_sync_frames).  The screen, in a workspace the context keeps for the calling thread on this
 *              stream (created on first use, grow-only: a call with a larger F than any before it on that stream allocates
 *              device memory; outgrown buffers are freed by gf3_ctx_destroy).  Calls of one thread on one stream share the
 *              workspace through stream order; other streams and threads have their own, at most 64 per context.
 *              All fp64 instead when the screen does not apply (below), and when no workspace can be had: the stream is
 *              being captured into a graph and no large-enough workspace exists yet (nothing is allocated under capture:
 *              call once with the largest F before capturing), the allocation fails, or all 64 are taken.  d_work is ignored.
 *           0: all fp64: the all-fp64 kernel on every window (the reference the screen is tested against)
 *           1: the screen in the CALLER's workspace d_work (NULL selects mode 0)
 *   d_work  mode 1: AT LEAST gf3_sync_frames_workspace_bytes(ctx, F) bytes of device memory -- the library cannot check the
 *           size of a device pointer, a smaller buffer is written past its end.  After the call its first int32 holds the
 *           number of windows that went to the fp64 kernel (0 when the call ran all fp64 for one of the reasons below).
 * The screen does not apply -- every mode then runs all fp64 -- when d_peak is asked for (an fp64 VALUE), when the window is
 * wider than the context's max_window or than 1024 lags, and when F exceeds 2^31.
 *
 * gf3_sync_frames_last: what the CALLING THREAD's last gf3_sync_frames / gf3_sync_frames_ex call did, if that call was on
 * this context and stream, without a device read: *path = 0 screened, 2 all fp64, -1 no such call;
 * *unresolved_capacity (optional) = windows the fp64 pass of a screened call could take (F), 0 otherwise.
 */
int64_t gf3_sync_frames_workspace_bytes(const gf3_ctx *ctx, int64_t F);
int gf3_sync_frames_ex(gf3_ctx *ctx, const void *d_in, int64_t n_in, int64_t F, int64_t stride,
                       int32_t win_lo, int32_t win_hi, int64_t *d_starts, double *d_peak_or_null,
                       int32_t mode, void *d_work, void *stream);
int gf3_sync_frames_last(const gf3_ctx *ctx, void *stream, int32_t *path, int32_t *unresolved_capacity);
/* tests: the screening pass alone.  d_y32 [F][W] fp32 lags, d_err [F] the bound of each window, d_cls [F] 0 resolved with a
 * detection / 1 resolved without / 2 unresolved (d_starts[f] is then left alone); d_work as above */
int gf3_debug_frames_screen(gf3_ctx *ctx, const void *d_in, int64_t n_in, int64_t F, int64_t stride,
                            int32_t win_lo, int32_t win_hi, int64_t *d_starts, float *d_y32, float *d_err,
                            int32_t *d_cls, void *d_work, void *stream);

/*
 * chirp_method with full reference semantics on one contiguous stream
 * (OFDM.py:356-372): full-coverage matched filter, normalisation by the GLOBAL
 * maximum, extremum-and-threshold candidates, sequential non-max suppression
 * over Lc samples, and the except-branch that drops every detection when a
 * chirp ends within the last two samples.  Writes the indices i with
 * zeros[i]==True (ascending) to d_peaks (capacity cap) and their count to
 * *n_peaks (host).  d_work: gf3_sync_stream_workspace_bytes(ctx, n) bytes.
 * d_corr (optional, n+Lc-1 doubles) receives the raw correlation P (OFDM.py:358).
 */
int gf3_sync_stream(gf3_ctx *ctx, const void *d_r, int64_t n,
                    int64_t *d_peaks, int64_t cap, int64_t *n_peaks,
                    void *d_work, double *d_corr_or_null, void *stream);

/*
 * How the stream-mode sync evaluates the matched filter.  Screened: every lag is first evaluated in fp32 with a proven
 * error bound; only the lags that the bound cannot exclude (a few around every chirp) are re-evaluated as fp64 dot
 * products, and the reference's rule (global maximum, threshold, extremum test) is applied to those fp64 values -- no
 * decision rests on an fp32 number; streams on which the screen is not selective take the all-fp64 overlap-save.
 * mode 0 (default): screened for streams of 2^23 samples or more (below that the all-fp64 path is the faster one);
 * mode 1: always all-fp64; mode 2: screened at any length; mode 3: as 2, with the general screening kernel even
 * where the band-limited one applies (a chirp whose spectrum lives below 3/16 of the sample rate, as the reference's
 * 0-8 kHz sweep at 48 kHz does: the bins above are left out of the fp32 products and their norm joins the error
 * bound).  Calls that ask for d_corr are always all-fp64.
 *
 * gf3_sync_stream_ex is gf3_sync_stream with the mode as an argument and the diagnostics as an output; it reads the
 * context only, so any number of threads may call it on one context at once.
 *   h_info4 (host, optional): path taken (0 screened, 1 fp64 after a non-selective screen, 2 fp64), cells (of 14 lags)
 *   re-evaluated in fp64, cells among them that hold a candidate, candidates found.
 */
int gf3_sync_stream_ex(const gf3_ctx *ctx, const void *d_r, int64_t n,
                       int64_t *d_peaks, int64_t cap, int64_t *n_peaks,
                       void *d_work, double *d_corr_or_null,
                       int32_t mode, int64_t *h_info4_or_null, void *stream);
/* legacy conveniences: the default mode gf3_sync_stream uses (the one field of a context that a call writes; an atomic
 * int), and the h_info4 of the CALLING THREAD's last gf3_sync_stream / gf3_sync_stream_ex */
int gf3_sync_stream_mode(gf3_ctx *ctx, int32_t mode);
int gf3_sync_stream_info(const gf3_ctx *ctx, int64_t *h_out4);
/*
 * chirp_method (OFDM.py:356-372) on a stream that arrives piece by piece -- host ingest through pinned buffers, streams
 * longer than HBM -- with the reference's EXACT global rule.  The 0.4 threshold is relative to the maximum of the whole
 * stream (OFDM.py:359), known only at the end; so each piece keeps the running maximum and the few lags that could
 * still pass whatever the final maximum is, with the raw fp64 values the rule looks at, and the rule itself is applied
 * afterwards (or provisionally, with the maximum so far) by gf3_sync_decide.  Engine.receive_host (engine.py) drives
 * the two calls; INTEGRATION.md shows the loop.
 *
 * gf3_sync_chunk: all-fp64 matched filter of d_buf[0..n) -- a piece of the stream with at least Lc + 1 samples of the
 * previous piece in front of it (none at the stream's start) -- restricted to the lags [lag_lo, lag_hi) of the buffer's
 * own full convolution P_buf[m] = sum_k buf[m-Lc+1+k] chirp[k] (1 <= lag_lo <= lag_hi <= n+Lc-2; the caller chooses
 * them so that every lag of the stream is owned by exactly one piece and its taps and both neighbours are complete).
 *   d_run_max (device, TWO doubles): [0] in  = maximum of the earlier pieces (-inf before the first), NumPy's NaN rule;
 *                                        out = maximum including this piece's lags;   [1] out = this piece's own maximum
 *   *h_piece_max (host, optional): that own maximum -- a piece whose list overflowed needs no second look if its own
 *                        maximum stays below thresh * (final maximum) * (1 - 1e-6): none of its lags can pass
 *   listed: every owned lag g with P[g] >= thresh * run_max * (1 - 1e-6) (every owned lag while run_max is not a
 *           positive finite number): d_idx[k] = g - 1 + lag_offset (the zeros-index of OFDM.py:360 in the caller's
 *           global numbering), d_val3[3k..3k+2] = P[g-1], P[g], P[g+1]; ascending; *n_listed (host) = how many.
 *   GF3_ERANGE with *n_listed = the number wanted when cap is too small (nothing is written): look at the piece again
 *   with a larger list, or once the final maximum is known (preset *d_run_max).
 *   d_work: gf3_sync_chunk_workspace_bytes(ctx, n) bytes.  Synchronises the stream (it returns a count).
 */
int64_t gf3_sync_chunk_workspace_bytes(const gf3_ctx *ctx, int64_t n);
int gf3_sync_chunk(const gf3_ctx *ctx, const void *d_buf, int64_t n,
                   int64_t lag_lo, int64_t lag_hi, int64_t lag_offset,
                   double *d_run_max, int64_t *d_idx, double *d_val3, int64_t cap,
                   int64_t *n_listed, double *h_piece_max_or_null, void *d_work, void *stream);
/*
 * gf3_sync_decide: the reference's rule on the listed raw values -- p = P / *d_max first, candidate <=>
 * (p1-p0)(p2-p1) <= 0 and p1 > thresh (OFDM.py:359-361) -- then the suppression walk over Lc samples with the
 * except-branch (OFDM.py:364-370) for a stream whose zeros array has nz_total = n_total + Lc - 3 entries (pass
 * INT64_MAX / 2 for a provisional decision on a stream that has not ended).  Peaks as gf3_sync_stream returns them.
 *   d_work: gf3_sync_decide_workspace_bytes(ctx, n_listed) bytes.  Synchronises the stream.
 */
int64_t gf3_sync_decide_workspace_bytes(const gf3_ctx *ctx, int64_t n_listed);
int gf3_sync_decide(const gf3_ctx *ctx, const int64_t *d_idx, const double *d_val3, int64_t n_listed,
                    const double *d_max, int64_t nz_total,
                    int64_t *d_peaks, int64_t cap, int64_t *n_peaks, void *d_work, void *stream);

/*
 * Self-normalised chirp detection: a rule of this library's own, next to the reference's (opt-in).  Where
 * chirp_method thresholds the matched filter against the maximum of the WHOLE stream, this rule thresholds the Pearson
 * correlation of every full window with the replica c (Lc samples, Sc = sum c, Ec = sum c^2):
 *     V[g]   = S2[g] - S1[g]^2 / Lc                        (S1, S2: the window's sums of r and r^2)
 *     rho[g] = (P[g] - S1[g] Sc / Lc) / sqrt((Ec - Sc^2 / Lc) V[g])         in [-1, 1], unchanged under a r + b
 * with rho[g] = 0 where V[g] <= 2^-36 Vrun[g], Vrun[g] = the largest V over the lags <= g of the stream (exact-zero gaps,
 * constant stretches), and rho[g] = NaN exactly where the window holds a sample that is not finite.  A lag g is detected
 * iff rho[g] > tau and rho[g] is the largest rho over the full-window lags in (g - Lc, g + Lc), the smallest lag winning a
 * tie.  Nothing in it looks further than Lc - 1 lags to either side, so a stream may be cut anywhere: the detections do not
 * depend on the cut, and a terminating chirp at the very end of a stream is a detection like any other (no except-branch).
 * Detections are reported as g - 1, the reference's zeros-index: + 2 is the packet's first sample, as after gf3_sync_stream.
 * All three calls read the context only, so any number of threads may call them on one context at once.
 *
 * gf3_detect_chunk: rho of d_buf[0..n) -- a piece of the stream with Lc - 1 samples of what came before in front of it
 * (none at the stream's start) -- on the lags [lag_lo, lag_hi) of the buffer's own full convolution (0 <= lag_lo <= lag_hi
 * <= n+Lc-1), restricted to the full windows of the buffer, Lc-1 <= g <= n-1.  Every storage type of the context.
 *   tau: the threshold; GF3_EINVAL unless it is a finite number inside (0, 1).  0.3 is the rule's constant.
 *   d_vrun (device, one double): in  = Vrun behind the earlier pieces (0 before the first);  out = with this piece's lags
 *   listed: every owned lag with rho > tau: d_idx[k] = g - 1 + lag_offset, d_rho[k] = rho[g]; ascending; *n_listed (host).
 *   GF3_ERANGE with *n_listed = the number wanted when cap is too small: no list is written and *d_vrun keeps its value;
 *   call again with a larger list.  (cap == 0 with no list buffers only counts.)
 *   d_rho_all (optional, n+Lc-1 doubles): rho[g] of every owned lag at [g]; the other entries are not written.
 *   d_work: gf3_detect_chunk_workspace_bytes(ctx, n) bytes.  Synchronises the stream (it returns a count).  The sums
 *   have a fixed order: two calls on the same buffer give identical bytes.
 */
int64_t gf3_detect_chunk_workspace_bytes(const gf3_ctx *ctx, int64_t n);
int gf3_detect_chunk(const gf3_ctx *ctx, const void *d_buf, int64_t n,
                     int64_t lag_lo, int64_t lag_hi, int64_t lag_offset, double tau,
                     double *d_vrun, int64_t *d_idx, double *d_rho, int64_t cap,
                     int64_t *n_listed, double *d_rho_all_or_null, void *d_work, void *stream);
/*
 * gf3_detect_decide: the windowed-maximum rule on a list as gf3_detect_chunk writes it (d_idx ascending; lists of several
 * pieces simply follow one another): entry k is a detection iff no entry within Lc - 1 of d_idx[k] has a larger rho, or
 * the same rho at a smaller index.  Emitted are the detections whose whole neighbourhood (d_idx[k] - Lc, d_idx[k] + Lc)
 * lies below final_below, the first index (in d_idx's numbering) that has not been through gf3_detect_chunk yet; the
 * others are withheld until a later call knows their neighbourhood.  Pass INT64_MAX / 2 at the end of a stream.  An
 * entry further than 2 Lc below final_below can no longer change a decision and may be dropped from the list.
 *   d_peaks (capacity cap), *n_peaks (host), GF3_ERANGE: as gf3_sync_decide.  d_work: 64 bytes.  Synchronises the stream.
 */
int gf3_detect_decide(const gf3_ctx *ctx, const int64_t *d_idx, const double *d_rho, int64_t n_listed,
                      int64_t final_below, int64_t *d_peaks, int64_t cap, int64_t *n_peaks,
                      void *d_work, void *stream);

/* tests: the fp32 screening pass alone.  d_p32 [n+Lc-1] float; d_blk [2*nblk] float: per block of *h_hop lags its
 * maximum, then the bound on |P32 - P| of its lags (nblk = ceil((n+Lc-1) / hop)) */
int gf3_debug_stream_screen(gf3_ctx *ctx, const void *d_r, int64_t n, float *d_p32, float *d_blk,
                            int32_t *h_hop, void *stream);

/*
 * receiver.schmidlcox_method (OFDM.py:376-387; unused by receive()): running-sum
 * autocorrelation metric P[d+1] = P[d] + r[d+L] r[d+2L] - r[d] r[d+L] (L = K+1) over search_len lags;
 * *d_index (device int64) = first index of max |P| + N - 1.  Needs n >= search_len - 1 + 2L samples.
 */
int gf3_schmidl_cox(gf3_ctx *ctx, const void *d_r, int64_t n, int64_t search_len,
                    int64_t *d_index, void *stream);

/*
 * demap (OFDM.py:484-500) standalone: hard decisions for n symbols.
 * d_bits_u8: [n*mu] one byte per bit (0/1); d_idx_u8 (optional): [n] index of
 * the chosen constellation point (hardDecision = constellation[idx]).
 */
int gf3_demap_hard(gf3_ctx *ctx, const void *d_sym_c128, int64_t n,
                   uint8_t *d_bits_u8, uint8_t *d_idx_u8, void *stream);

/*
 * Transmit-side synthesiser: transmitter.map + build_OFDM_symbol + ifft + add_cp +
 * send_to_stream (OFDM.py:196-259) for F packets, one row of `stride` samples per packet:
 *   [gap_f zeros | chirp | P known symbols | D data symbols | P known symbols | zeros], symbols x2.
 *   d_bits_packed [F, gf3_bytes_per_frame]: payload in the format gf3_demod_frames writes
 *   d_filler_c128 [K]: value of every carrier that is not a data carrier (random_qpsk, OFDM.py:201-215),
 *                      indexed by carrier (entries of data carriers are ignored)
 *   d_gaps        [F] int64 leading zeros per row, or NULL
 *   out_dtype     GF3_F32 or GF3_F64
 * Every sample of every row is written, the zeros included.  GF3_EINVAL, and nothing written, for a stride shorter than
 * one packet, Lc + (2P + D)(N + CP).  The gaps live in device memory and are not checked: 0 <= d_gaps[f] <= stride - that
 * length is the caller's to keep (a longer gap would carry the packet beyond its row).
 */
int gf3_tx_frames(gf3_ctx *ctx, const uint8_t *d_bits_packed, const void *d_filler_c128,
                  const int64_t *d_gaps, int64_t F, void *d_out, int64_t stride,
                  int32_t out_dtype, void *stream);

/*
 * gf3_tx_frames with two more arguments.  gf3_tx_frames is this call with d_tones_c128 = NULL and body_gain = 1.0.
 *   d_tones_c128  [F, D, Ku] complex128 or NULL: the reserved carriers (carriers 1..K outside data_bins, ascending; Ku = K - C)
 *                 of data symbol (f, l) take tones[f, l] instead of the filler (which may then be NULL).  The pilot
 *                 symbols and the chirp are what they are without it.  GF3_EINVAL when given with Ku = 0.
 *   body_gain     finite, > 0: multiplies the x2 of the pilot and data symbols, not the chirp
 */
int gf3_tx_frames_ex(gf3_ctx *ctx, const uint8_t *d_bits_packed, const void *d_filler_c128,
                     const int64_t *d_gaps, int64_t F, void *d_out, int64_t stride,
                     int32_t out_dtype, const void *d_tones_c128, double body_gain, void *stream);

/*
 * Tone reservation: per data symbol, values for the reserved carriers that lower the symbol's peak (no receiver reads
 * them in a data symbol).  With X the data-carrier values gf3_tx_frames would send and x(R) the real N-sample symbol
 * of X and the tones R (DC and Nyquist zero, np.fft.ifft scaling, without the frame's x2):
 *   sigma = sqrt(2 sum |X_k|^2) / N,  A = sigma 10^(target_db/20),  L = 10^(tone_limit_db/20)
 *   R = 0; for i = 1..iterations: c = x(R) - clip(x(R), -A, A); stop if c == 0; R -= N / (2 Ku) fft(c) on the reserved
 *   bins; |R_k| > L is scaled back to L; the iterate of the smallest max|x(R)| is kept (iterate 0, R = 0, included; the
 *   first minimum wins) -- so the result is never worse than a zero filler.
 *   d_tones_c128 [F, D, Ku] complex128;  d_report_f64 [F, D, 4] = (peak at R = 0, best peak, its iterate, rms of the best symbol)
 * One workgroup per symbol, fixed reduction order: two calls give identical bytes.  GF3_EINVAL for Ku = 0, null
 * pointers, parameters that are not finite and iterations outside [0, 64].
 */
int gf3_tone_reserve(gf3_ctx *ctx, const uint8_t *d_bits_packed, int64_t F, double target_db,
                     double tone_limit_db, int32_t iterations, void *d_tones_c128,
                     double *d_report_f64, void *stream);

/*
 * Known-channel zero forcing, the reference's older receive flow (`Weekend Challenge.ipynb` cells 9-19:
 * H = np.fft.fft(h, N); symbols = FFT(rx_no_cp) / H; demap of the data carriers): an optional extra mode with
 * sample-exact timing supplied by the caller, not part of receive() (OFDM.py:581-657 estimates the channel from
 * pilots instead, gf3_demod_frames).  The function it used (`equalise(OFDM_demod, H)`) no longer exists in OFDM.py, so
 * parity is pinned by the formula only.
 *   d_offsets [n_sym] int64: first of the N samples of each symbol (past its prefix);  d_h [n_taps] float64 channel taps
 *   d_eq [n_sym, C] complex128 equalised data-carrier symbols;  d_bits [n_sym*C*mu] one byte per bit;  d_idx optional
 *   d_work: gf3_known_h_workspace_bytes(ctx, n_sym) bytes
 */
int64_t gf3_known_h_workspace_bytes(const gf3_ctx *ctx, int64_t n_sym);
int gf3_equalise_known_h(gf3_ctx *ctx, const void *d_in, int64_t n_in, const int64_t *d_offsets, int64_t n_sym,
                         const double *d_h, int32_t n_taps, void *d_eq_c128, uint8_t *d_bits_u8,
                         uint8_t *d_idx_u8_or_null, void *d_work, void *stream);

/*
 * PS + decode (OFDM.py:504-505, 541-544) on the packed decisions of gf3_demod_frames: one int64 0/1 per bit, in the
 * reference's order (packet -> symbol -> data carrier -> bit), XORed with the whitening mask when one is given --
 * `bits ^ tile(known_sequence[:C*mu])[:len]` for encoding "XOR", d_mask_u8 = NULL for encoding "None".
 *   d_bits_packed [F, gf3_bytes_per_frame] uint8     d_mask_u8 [n_mask] one byte per bit (0/1), or NULL
 *   out_i64       [F * D*C*mu] int64: DEVICE memory, or PINNED host memory (hipHostMalloc / hipHostRegister -- e.g. a
 *                 torch tensor with pin_memory=True): the kernel then writes the array the reference returns straight
 *                 into host memory, 16 bytes per lane, and no separate copy is needed.  Pageable host memory is refused.
 *                 out_i64 must be 16-BYTE ALIGNED, wherever it lives (GF3_EINVAL otherwise).
 */
int gf3_unpack_bits(gf3_ctx *ctx, const uint8_t *d_bits_packed, int64_t F, const uint8_t *d_mask_u8, int32_t n_mask,
                    void *out_i64, void *stream);

/* max-log soft demapping (not in the reference; LLR > 0 <=> bit 0). [n*mu] f32 */
int gf3_soft_demap(gf3_ctx *ctx, const void *d_sym_c128, int64_t n,
                   double noise_var, float *d_llr_f32, void *stream);

/*
 * Channel-state-weighted soft demapping (not in the reference): the max-log LLRs of gf3_soft_demap with noise_var = 1,
 * each multiplied by |H^_{f,l,k}|^2, the squared magnitude of the reference's per-symbol channel model
 * |Hs| + (|He| - |Hs|) (l + P/2) / (D + P) (OFDM.py:469) -- the reliability of carrier k of data symbol l after single-tap
 * zero forcing.  Hest is not needed: the weight comes from the pilot estimates directly.  Normalised min-sum decoding is
 * invariant to one global LLR scale, so no noise-variance estimate enters.
 *   d_eq_c128 [F*D, C] equalised data-carrier symbols (gf3_demod_frames' d_eq)
 *   d_Hs_c128, d_He_c128 [F, K] start / end pilot estimates (gf3_demod_frames' d_Hs / d_He)
 *   d_llr_f32 [F*D*C*mu] in the reference's bit order (packet -> symbol -> data carrier -> bit); LLR > 0 <=> bit 0
 */
int gf3_soft_demap_csi(gf3_ctx *ctx, const void *d_eq_c128, const void *d_Hs_c128, const void *d_He_c128,
                       int64_t F, float *d_llr_f32, void *stream);

/*
 * Samples to weighted max-log LLRs in ONE launch (not in the reference): get_symbols ... equalise and the data-carrier
 * select (OFDM.py:391-480, 603) as gf3_demod_frames runs them, with the soft demapper and the CSI weight in the place of
 * demap + PS -- the fused kernel's soft output mode.  Replaces gf3_demod_frames(d_eq, d_Hs, d_He) + gf3_soft_demap_csi on the
 * coded receive path: the equalised symbols never travel to memory, the weight |H^|^2 is taken from the magnitude model
 * the kernel holds per carrier, and (max-log difference) x weight is rounded to float32 once (the staged pair rounds twice:
 * the two agree to 1.5 x 2^-23 relative).  No hard bits are produced.
 *   d_llr_f32 [F*D*C*mu] in the reference's bit order (packet -> symbol -> data carrier in data_bins order -> bit);
 *             LLR > 0 <=> bit 0.  The layout gf3_soft_demap_csi writes.
 *   weight    0: unit weight (gf3_soft_demap(eq, 1.0))      1: |H^_{f,l,k}|^2 (gf3_soft_demap_csi)
 *   d_Hs, d_He, d_slope, d_status   optional, as in gf3_demod_frames (the same values, bit for bit, in the same form)
 *   d_work, mode                    as in gf3_demod_frames_ex (gf3_demod_workspace_bytes; NULL: the one-launch kernel)
 * A frame whose samples fall outside [0, n_in) gets a row of +0.0f (erasures to a decoder) and sets bit 0 of *d_status.
 * Every table the context accepts has max-log LLRs (gf3_soft_demap refuses none), so none is refused here; GF3_EINVAL for a
 * weight other than 0 or 1.  Non-finite samples are outside this call's contract.  F == 0 is a no-op.
 */
int gf3_demod_frames_llr(gf3_ctx *ctx, const void *d_in, int64_t n_in,
                         const int64_t *d_frame_offsets, int64_t F,
                         float *d_llr_f32, int32_t weight,
                         void *d_Hs, void *d_He, double *d_slope, int32_t *d_status,
                         void *d_work, int32_t mode, void *stream);

/*
 * Noise-weighted soft demapping (not in the reference): per-carrier effective noise variances measured on the equalised
 * data symbols themselves, and max-log LLRs divided by them.  Opt-in; gf3_soft_demap_csi is unchanged.
 *   gf3_noise_estimate:  v[f, c] = (1/D) sum_l |eq[f, l, c] - s|^2, s the constellation point the hard decision picks
 *     (gf3_demap_hard's rule; a NaN / Inf symbol makes v[f, c] non-finite).  fp64, summed in a fixed order (symbols
 *     l = w, w + 8, ... ascending for w = 0 .. 7, then the eight partial sums in the order of w): two calls give
 *     identical bits.
 *   gf3_soft_demap_nw:  LLR[f, l, c, b] = maxlog(eq[f, l, c]; sigma^2 = 1)[b] * w[f, c] with vbar[f] = mean_c v[f, c] and
 *     w = 0 where v[f, c] is not finite (the LLR is then +0: an erasure), else 1 for the whole packet where vbar[f] is 0
 *     or not finite (a noiseless synthetic stream), else 1 / max(v[f, c], 1e-6 vbar[f]).  No |H^|^2 factor: the
 *     residual is measured after the divide by H^ and already contains it.
 *   d_eq_c128 [F*D, C] (gf3_demod_frames' d_eq)   d_var_f64 [F, C]   d_llr_f32 [F*D*C*mu], bit order and sign as
 *   gf3_soft_demap_csi.  F == 0 is a no-op; at most 65535 packets per call.
 */
int gf3_noise_estimate(gf3_ctx *ctx, const void *d_eq_c128, int64_t F, double *d_var_f64, void *stream);
int gf3_soft_demap_nw(gf3_ctx *ctx, const void *d_eq_c128, const double *d_var_f64, int64_t F, float *d_llr_f32,
                      void *stream);

/*
 * Impulse noise (clicks, dropouts: a few whole data symbols are garbage): the carrier x symbol form of the pair above and
 * a packet-wide bit interleaver.  The two only work together: spread over every codeword, unmarked garbage is worse
 * than garbage left in place.  Opt-in; the entry points above are unchanged.  (The names carry no digit because the
 * project's ABI check reads the header's declarations as lower-case words: "cs" = carrier x symbol.)
 *   gf3_noise_estimate_cs:  one pass over eq gives v[f, c] as gf3_noise_estimate does -- the same bits -- and
 *     vs[f, l] = (1/C) sum_c |eq[f, l, c] - s|^2.  fp64, fixed order (a lane adds the terms of its carriers c = 64 k +
 *     lane for the columns k of its half of the carriers ascending, an xor butterfly 32, 16, .. 1 adds the 64 lanes,
 *     then first half + second half): two calls give identical bits.  One workgroup per packet keeps 64 C + 16 D bytes
 *     of partial sums in LDS: GF3_ERANGE beyond 160 KB or C > 2048.
 *   gf3_soft_demap_nw_cs:  LLR = maxlog(eq; sigma^2 = 1) * w[f, l, c] with vbar[f] = mean_c v[f, c] (the number
 *     gf3_soft_demap_nw uses) and w = 0 where v[f, c] or vs[f, l] is not finite (+0: an erasure), else 1 for the whole
 *     packet where vbar[f] is 0 or not finite, else 1 / max(v[f, c] vs[f, l] / vbar[f], 1e-6 vbar[f]).
 *     deinterleave = 0: LLRs in transmitted order, as gf3_soft_demap_nw writes them.  1: the LLR of transmitted position
 *     pi(i) is written at coded position i of its packet -- bit for bit gf3_interleave(inverse = 1) of the former.
 *   gf3_interleave:  the bare permutation of [F, nbp] arrays of 1- or 4-byte elements, nbp = D C mu per packet.  Coded
 *     bit i travels at position pi(i) = (i s) mod nbp, s the smallest integer >= C mu + 1 with gcd(s, nbp) = 1 (2801 for
 *     2800 bits per symbol and D = 180): consecutive coded bits land in consecutive symbols.
 *     inverse = 0: out[pi(i)] = in[i] (transmit side).  1: out[i] = in[pi(i)].  Out of place; nbp < 2^31.
 *   d_var_c_f64 [F, C]   d_var_s_f64 [F, D]   F == 0 is a no-op; at most 65535 packets per call.
 */
int gf3_noise_estimate_cs(gf3_ctx *ctx, const void *d_eq_c128, int64_t F, double *d_var_c_f64, double *d_var_s_f64,
                          void *stream);
int gf3_soft_demap_nw_cs(gf3_ctx *ctx, const void *d_eq_c128, const double *d_var_c_f64, const double *d_var_s_f64,
                         int64_t F, int32_t deinterleave, float *d_llr_f32, void *stream);
int gf3_interleave(gf3_ctx *ctx, const void *d_in, void *d_out, int64_t F, int32_t elem_bytes, int32_t inverse,
                   void *stream);

/*
 * Adaptive bit loading (not in the reference): a QAM order per data carrier, and the noise pair above for such a
 * mixed-order packet.  Opt-in; every entry point above is unchanged and still works on the context's one table.
 *   A loading is order[C] in data_bins order, each 0, 2, 4 or 6 bits.  Bs = sum(order) coded bits travel per data symbol,
 *   carrier c's at off[c] = sum(order[:c]) (packet -> symbol -> carrier -> bit, the existing order with a variable
 *   width; every off[c] is even).  A carrier of order m > 0 uses the Gray-coded square 2^m-QAM of unit energy, label
 *   bits MSB first, the first m/2 on the I axis: level i of an axis of L = 2^(m/2) levels is the double
 *   (2i - (L-1)) * (1 / sqrt(2 (L^2 - 1) / 3)) and carries the label bits i ^ (i >> 1).  At m = 2 this is NOT the
 *   reference's QPSK table, whose first bit lies on the Q axis.  A carrier of order 0 carries no payload: it transmits
 *   the pilot symbol of its bin (gf3_config.known_re / known_im), so it stays a measured carrier.
 *   gf3_loading_create:  validates on the host (GF3_EINVAL: null argument, C != the context's C, a value outside
 *     {0, 2, 4, 6}, no loaded carrier) and uploads the tables to the context's device.  The object is immutable: it can
 *     be shared by calls in flight on any stream, and must outlive them.  It does not keep the context.
 *   gf3_loading_bits:  Bs (0 for a null handle).
 *   gf3_noise_estimate_loaded:  gf3_noise_estimate with s the point of carrier c's OWN table that the hard decision
 *     picks, and the known pilot point on a carrier of order 0 (a residual with no decision error in it).  The same
 *     structure and summation order: on an all-m loading and a context of that table, the same bits.
 *   gf3_soft_demap_loaded:  LLR[f, l, off[c] + b] = (float)(maxlog(eq[f, l, c]; table of order[c])[b] * w), the product
 *     in fp64 and rounded once; +0 where w = 0; carriers of order 0 write nothing.  The weight is chosen by the optional
 *     arguments:  d_var given: gf3_soft_demap_nw's rule, vbar the mean of v over all C carriers.  d_Hs and d_He given:
 *     gf3_soft_demap_csi's weight (|Hs| + (|He| - |Hs|) (l + P/2) / (D + P))^2 at the carrier's bin.  None: w = 1.
 *     d_var together with d_Hs / d_He, or only one of d_Hs / d_He: GF3_EINVAL.
 *   d_eq_c128 [F*D, C]   d_var_f64 [F, C]   d_Hs / d_He [F, K]   d_llr_f32 [F*D*Bs].  F == 0 is a no-op; at most 65535
 *   packets per call.  d_llr_f32 must be 8-BYTE ALIGNED (every off[c] and Bs are even, so each carrier's LLRs are stored
 *   two at a time): GF3_EINVAL otherwise.  Every element of d_llr_f32 is written (a carrier of order 0 owns none).
 */
typedef struct gf3_loading gf3_loading;
int gf3_loading_create(const gf3_ctx *ctx, const uint8_t *h_order, int32_t C, gf3_loading **out);
void gf3_loading_destroy(gf3_loading *ld);
int gf3_loading_bits(const gf3_loading *ld);
int gf3_noise_estimate_loaded(gf3_ctx *ctx, const gf3_loading *ld, const void *d_eq_c128, int64_t F,
                              double *d_var_f64, void *stream);
int gf3_soft_demap_loaded(gf3_ctx *ctx, const gf3_loading *ld, const void *d_eq_c128,
                          const void *d_Hs_c128_or_null, const void *d_He_c128_or_null,
                          const double *d_var_f64_or_null, int64_t F, float *d_llr_f32, void *stream);

/*
 * Receive diversity (not in the reference): maximal-ratio combining of the equalised symbols of B recordings of ONE
 * transmission (the two channels of a stereo recording, a second microphone), each synchronised and demodulated on its
 * own.  A reflection puts deep nulls into each microphone's transfer function; another microphone has them at other
 * frequencies, and the weights fill each branch's nulls from the others.
 *   z[f, l, c] = (sum_b w_b z_b) / W,  W = sum_b w_b,  z_b = eq_b[f, l, c], summed for b ascending; 0 + 0i where W = 0.
 *   mode GF3_COMBINE_CSI:    w_b[f, l, c] = (|Hs_b| + (|He_b| - |Hs_b|) (l + P/2) / (D + P))^2 at the carrier's bin: the
 *     weight of gf3_soft_demap_csi.  d_Hs_c128[b], d_He_c128[b]: [F, K] of gf3_demod_frames; d_var_f64 is not read.
 *   mode GF3_COMBINE_NOISE:  vbar[f] = the mean over all b and c of var_b[f, c];  w_b[f, c] = 1 / max(var_b[f, c],
 *     1e-6 vbar[f]), and 1 for the whole packet where vbar[f] is 0 or not finite: the rule of gf3_soft_demap_nw taken
 *     over all branches, so a noiseless branch dominates a noisy one.  d_var_f64[b]: [F, C] of gf3_noise_estimate on
 *     branch b; d_Hs_c128, d_He_c128 are not read.
 *   In both modes w_b = 0 where its input (|Hs_b|, |He_b| or var_b) is not finite, where it comes out not finite, or
 *   where z_b is not finite in either part: that symbol of that branch is left out of both sums.
 *   d_eq_c128, d_Hs_c128, d_He_c128, d_var_f64: HOST arrays of B device pointers (read during the call only), 1 <= B <=
 *   GF3_MAX_BRANCHES; d_eq_c128[b] is [F*D, C] as gf3_demod_frames writes it.  Outputs, each optional, at least one:
 *     d_eq_out_c128 [F*D, C]  z (none of the d_eq_c128[b])
 *     d_wsum_f64 [F*D, C]     W
 *     d_llr_f32 [F*D*C*mu]    (float)(maxlog(z; sigma^2 = 1) * W) in the order and sign of gf3_soft_demap_csi; +0 where W = 0
 *   With B = 1 the LLRs are those of gf3_soft_demap_csi / gf3_soft_demap_nw to float32 rounding.
 *   GF3_EINVAL (the text names gf3_combine_branches) for a null context, B out of range, a null branch pointer, no
 *   output, F < 0, an unknown mode, more than 65535 packets.  F == 0 is a no-op.  One launch, no allocation, no host
 *   synchronisation, asynchronous on `stream`; every sum in a fixed order, no atomics: two calls give identical bytes.
 */
#define GF3_MAX_BRANCHES 4
#define GF3_COMBINE_CSI 0
#define GF3_COMBINE_NOISE 1
int gf3_combine_branches(gf3_ctx *ctx, int32_t B, const void *const *d_eq_c128, int32_t mode,
                         const void *const *d_Hs_c128, const void *const *d_He_c128, const double *const *d_var_f64,
                         int64_t F, void *d_eq_out_c128, double *d_wsum_f64, float *d_llr_f32, void *stream);

/*
 * 2 x 2 spatial multiplexing (not in the reference): two packets sent at once, one per loudspeaker, sample-aligned, and
 * separated per carrier from B >= 1 recordings (B >= 2 to separate two streams that both carry data).  Speaker 0 sends
 * every chirp and its pilots as they are; speaker 1 is silent during the chirps and negates its pilot symbols of odd index
 * p (counted from each block's first symbol).  At microphone b the pilots then read Y_p[k] = (H_b0[k] + (-1)^p H_b1[k]) X[k],
 * so for an even P the two covers
 *     cover t:  mean_p (-1)^(t p) Y_p[k] / X[k],  t = 0, 1
 * are the two columns H_b0, H_b1 of the channel; cover 0 is what gf3_demod_frames returns as Hs / He.
 *   - gf3_mimo_pilots: d_H_out_c128 [F][2 sides][2 covers][K] complex128 (side 0: the start block, 1: the end block) from the
 *     samples d_in [n_in] of the context's type and the packets' first-pilot offsets.  Per (packet, side) the signed
 *     time-domain sums sum_p (-1)^(t p) x_p[n] of the P pilot symbols without their prefix (p ascending), one real transform
 *     each, times 1 / (P known_k).  d_status_i32 [F]: 1 for a packet whose body [offset, offset + (2P + D)(N + CP)) leaves
 *     [0, n_in) at either end, else 0; such a packet's rows are NaN in both parts, never left unwritten.
 *     GF3_EINVAL for a context whose P is odd or < 2, a null pointer with F > 0, F < 0, n_in < 0, more than 2^30 - 1
 *     packets.  F == 0 is a no-op.
 *   - gf3_mimo_detect: joint max-log ML detection of the two streams' symbols over the 4 x 4 pairs of constellation points.
 *     Inputs are HOST arrays of B device pointers (read during the call only), 1 <= B <= GF3_MAX_BRANCHES:
 *       d_Y_c128[b]     [F*D, N/2+1]  the data symbols' spectra as gf3_rfft_batch writes them; data carrier c is read at
 *                                     bin data_bins[c]
 *       d_H_c128[b]     [F, 2, 2, K]  gf3_mimo_pilots' output for recording b
 *       d_slope_f64[b]  [F]           gf3_demod_frames' slope for recording b (one pair of clocks: it serves both columns)
 *     Per cell (f, l, c), with n = data_bins[c] - 1, f_l = (l + P/2) / (D + P), and for each of the B x 2 entries the
 *     reference's channel model from its start and end estimates Hs, He:
 *       h_bt = (|Hs| + (|He| - |Hs|) f_l) (Hs / |Hs|) exp(i slope_b n f_l)        (Hs / |Hs| = 1 where |Hs| = 0)
 *       G00 = sum_b |h_b0|^2,  G11 = sum_b |h_b1|^2,  G01 = sum_b conj(h_b0) h_b1,  m_t = sum_b conj(h_bt) y_b   (b ascending)
 *       metric(x0, x1) = G00 |x0|^2 + G11 |x1|^2 + 2 Re(conj(x0) G01 x1) - 2 Re(conj(x0) m0) - 2 Re(conj(x1) m1)
 *       LLR of a bit of stream s = min over the pairs with that bit 1 - min over the pairs with that bit 0      (> 0: bit 0)
 *     which is sum_b |y_b - h_b0 x0 - h_b1 x1|^2 less the term without x.  A branch whose y_b, whose slope or any of whose
 *     four estimates at the cell is not finite is left out of every sum; where every branch is, the four LLRs are +0.
 *     d_llr_f32 [F][GF3_MIMO_STREAMS][D][C][mu] float32: flattened, the coded order of packets 2f and 2f + 1.
 *     GF3_EINVAL for a null context, a context whose table is not mu = 2 with 4 points, B out of range, a null pointer,
 *     F < 0, more than 65535 packets.  F == 0 is a no-op.
 *   Both: one launch, no allocation, no host synchronisation, asynchronous on `stream`; every sum in a fixed order, no
 *   atomics: two calls give identical bytes.  The text of a refusal names the function.
 */
#define GF3_MIMO_STREAMS 2
int gf3_mimo_pilots(gf3_ctx *ctx, const void *d_in, int64_t n_in, const int64_t *d_frame_offsets, int64_t F,
                    void *d_H_out_c128, int32_t *d_status_i32, void *stream);
int gf3_mimo_detect(gf3_ctx *ctx, int32_t B, const void *const *d_Y_c128, const void *const *d_H_c128,
                    const double *const *d_slope_f64, int64_t F, float *d_llr_f32, void *stream);

/*
 * Transmit diversity (not in the reference): two loudspeakers, B >= 1 recordings -- one microphone is the point -- and the
 * Alamouti space-time block code over pairs of data symbols.  ONE stream is sent.  Chirps, pilots and cover are those of
 * spatial multiplexing above (P even and >= 2), so gf3_mimo_pilots gives both columns H_b0, H_b1 of every recording.  D is
 * even; with X_l the spectrum of data symbol l, for j = 0 .. D/2 - 1
 *     slot a = 2j:       speaker 0 sends  X_a,          speaker 1  X_b'
 *     slot b' = 2j + 1:  speaker 0 sends  -conj(X_b'),  speaker 1  conj(X_a)
 * (the symbols are real: conj(X) is the N-sample body reversed in time, x[(-n) mod N], under a prefix rebuilt from it).  Per
 * carrier, with x0, x1 the points of symbols a and b':  y_a = h0(a) x0 + h1(a) x1,  conj(y_b') = conj(h1(b')) x0 - conj(h0(b')) x1,
 * and a single microphone sees |H0|^2 + |H1|^2 where one speaker gives |H0|^2 and the same signal on both |H0 + H1|^2.
 *   - gf3_stbc_slope: the phase the channel gains per carrier between the two pilot blocks -- what gf3_demod_frames' slope
 *     means -- fitted ONCE per packet on all paths together.  d_H_c128 is a HOST array of B device pointers (read during
 *     the call only), 1 <= B <= GF3_MAX_BRANCHES, each gf3_mimo_pilots' output [F, 2, 2, K].  Per packet f
 *       d[k] = sum_b sum_t conj(H_b[f, 0, t, k]) H_b[f, 1, t, k]                 (b, then t, ascending)
 *       y = unwrap(angle d) along k;  slope = the first-degree least-squares coefficient of y over [fit_lo, fit_hi)
 *     with the demodulator's own angle, unwrap correction and cumulative-correction fit.  The clock drift it measures is
 *     common to every path, and d has a null only where every path has one, where the angle series of ONE path breaks at
 *     that path's nulls.  d_slope_f64 [F]; NaN for a packet with a d[k] of the fit range that is not finite.  One workgroup
 *     per packet.  GF3_EINVAL for a null context, an odd P or P < 2, an odd D, B out of range, a null pointer, F < 0, more
 *     than 2^30 - 1 packets.  F == 0 is a no-op.
 *   - gf3_stbc_detect: joint max-log ML detection of every pair over the 4 x 4 pairs of constellation points.  d_Y_c128 and
 *     d_H_c128 are HOST arrays of B device pointers as gf3_mimo_detect takes them; d_slope_f64 [F] is ONE device array, the
 *     slope of every branch.  Per branch b the B x 2 channel entries h_t(l) at both slots are the reference's channel model
 *     as gf3_mimo_detect states it, and per (f, j, c)
 *       G00 = sum_b |h0(a)|^2 + |h1(b')|^2        G11 = sum_b |h1(a)|^2 + |h0(b')|^2
 *       G01 = sum_b conj(h0(a)) h1(a) - h1(b') conj(h0(b'))
 *       m0 = sum_b conj(h0(a)) y_a + h1(b') conj(y_b')        m1 = sum_b conj(h1(a)) y_a - h0(b') conj(y_b')     (b ascending)
 *     go into gf3_mimo_detect's metric and LLR rule; the LLRs of x0 go to symbol 2j, those of x1 to symbol 2j + 1.  G01 is
 *     what the channel's change between the two slots leaves (0 on a static channel); with it the detector is the exact
 *     max-log ML of the pair.  A branch whose y at either slot, whose four estimates at the carrier, or the slope is not
 *     finite is left out of every sum; where every branch is, both symbols' LLRs are +0.
 *     d_llr_f32 [F][D][C][mu] float32: flattened, the coded order of one stream.
 *     GF3_EINVAL for a null context, a context whose table is not mu = 2 with 4 points, an odd P or P < 2, an odd D, B out
 *     of range, a null pointer, F < 0, more than 65535 packets.  F == 0 is a no-op.
 *   Both: one launch, no allocation, no host synchronisation, asynchronous on `stream`; every sum in a fixed order, no
 *   atomics: two calls give identical bytes.  The text of a refusal names the function.
 */
int gf3_stbc_slope(gf3_ctx *ctx, int32_t B, const void *const *d_H_c128, int64_t F, double *d_slope_f64, void *stream);
int gf3_stbc_detect(gf3_ctx *ctx, int32_t B, const void *const *d_Y_c128, const void *const *d_H_c128,
                    const double *d_slope_f64, int64_t F, float *d_llr_f32, void *stream);

/*
 * The two-speaker paths under coloured noise (not in the reference).  The joint metric sum_b |y_b - h_b0 x0 - h_b1 x1|^2
 * weights every recording and carrier alike, which is maximum likelihood only in white noise of one level.  With a weight
 * w_b[f, c] per recording, packet and data carrier the statistics of gf3_mimo_detect and gf3_stbc_detect become
 *     G00 = sum_b w_b |h_b0|^2,  G11, G01, m0, m1 likewise (for the space-time code both slots of a pair under the one w_b),
 * everything after the sums unchanged: the maximum-likelihood metric for noise of variance 1 / w_b.  The variance is
 * measured on the covered pilots, where nothing has to be decided: two of a block's P observations per carrier give the
 * two columns (gf3_mimo_pilots), the other P - 2 the noise.
 *   - gf3_mimo_pilot_noise: d_var_out_f64 [F][2 sides][K] float64 from the samples and offsets as gf3_mimo_pilots takes them
 *     and that call's output d_H_c128 [F][2][2][K]:
 *       v[f, side, k] = 1 / (P - 2) sum_p | Y_p[k] / X[k] - H[f, side, 0, k] - (-1)^p H[f, side, 1, k] |^2
 *     over the side's P pilot symbols without their prefix, p ascending, each transformed on its own; 1 / X as in
 *     gf3_mimo_pilots.  The unit is that of |H|^2: white noise of deviation sigma per sample gives
 *     N sigma^2 / |X|^2 under the library's unnormalised transform.  d_status_i32 [F] and the NaN rows of a packet whose
 *     body leaves [0, n_in) are gf3_mimo_pilots' rule.  One workgroup per (packet, side).
 *     GF3_EINVAL for a null context, a context whose P is odd or < 4 (P = 2 leaves no degree of freedom), a null pointer
 *     with F > 0, F < 0, n_in < 0, more than 2^30 - 1 packets.  F == 0 is a no-op.
 *   - gf3_joint_noise_weights: d_var_f64 is a HOST array of B device pointers (read during the call only), 1 <= B <=
 *     GF3_MAX_BRANCHES, each gf3_mimo_pilot_noise's output [F][2][K] for one recording.  Per data carrier c
 *       v_b[f, c] = 0.5 (var_b[f, 0, data_bins[c] - 1] + var_b[f, 1, data_bins[c] - 1])
 *     and then gf3_combine_branches' rule under GF3_COMBINE_NOISE: vbar[f] the mean of v_b[f, c] over all branches and data
 *     carriers (fixed order), w = 1 for the whole packet where vbar is 0 or not finite, else w = 1 / max(v, 1e-6 vbar);
 *     w = 0 where v is not finite.  d_w_out_f64 [B][F][C] float64.  One workgroup per packet.
 *     GF3_EINVAL for a null context, B out of range, a null pointer, F < 0, more than 2^30 - 1 packets.  F == 0 is a no-op.
 *   - gf3_mimo_detect_nw, gf3_stbc_detect_nw: gf3_mimo_detect and gf3_stbc_detect with d_w_f64 [B][F][C], ONE device array,
 *     gf3_joint_noise_weights' output.  A branch whose weight at a carrier is 0 or not finite is left out of every sum
 *     there, as one with a non-finite estimate is; where every branch is, the LLRs are +0.  Arguments, outputs and refusals
 *     are the unweighted calls', and a null d_w_f64 is refused.
 *   All: one launch, no allocation, no host synchronisation, asynchronous on `stream`; every sum in a fixed order, no
 *   atomics: two calls give identical bytes.  The text of a refusal names the function.
 */
int gf3_mimo_pilot_noise(gf3_ctx *ctx, const void *d_in, int64_t n_in, const int64_t *d_frame_offsets, int64_t F,
                         const void *d_H_c128, double *d_var_out_f64, int32_t *d_status_i32, void *stream);
int gf3_joint_noise_weights(gf3_ctx *ctx, int32_t B, const double *const *d_var_f64, int64_t F, double *d_w_out_f64,
                            void *stream);
int gf3_mimo_detect_nw(gf3_ctx *ctx, int32_t B, const void *const *d_Y_c128, const void *const *d_H_c128,
                       const double *const *d_slope_f64, const double *d_w_f64, int64_t F, float *d_llr_f32, void *stream);
int gf3_stbc_detect_nw(gf3_ctx *ctx, int32_t B, const void *const *d_Y_c128, const void *const *d_H_c128,
                       const double *d_slope_f64, const double *d_w_f64, int64_t F, float *d_llr_f32, void *stream);

/*
 * Spatial multiplexing with known bits (not in the reference): the joint detector told what a decoder has already settled,
 * for successive interference cancellation driven by the code.  The two packets of a pair share every cell and their
 * codewords are different codewords; once one stream's bit at a cell is known, the pairs that contradict it are out, and
 * with x0 wholly known stream 1 sees y - h0 x0 through h1 alone: gain G11 instead of G11 (1 - |G01|^2 / (G00 G11)).
 *   - gf3_mimo_detect_known: gf3_mimo_detect (d_w_f64 null) or gf3_mimo_detect_nw (d_w_f64 [B][F][C]) with two more inputs,
 *     d_bits_u8 and d_known_u8 [F][GF3_MIMO_STREAMS][D][C][mu] uint8, one byte per coded bit in the layout and order of the
 *     LLRs (the transmitted order of packets 2f and 2f + 1): a non-zero d_known_u8 byte says the bit is known, a non-zero
 *     d_bits_u8 byte that it is 1 (read where the bit is known only).  G00, G11, G01, m0, m1, the rule that leaves a branch
 *     out and the order of every sum are those calls'.  A pair (x0 = point i, x1 = point j) is ADMISSIBLE when for both
 *     streams every known bit of the cell equals that bit of the stream's point's label.  Then
 *       an unknown bit: LLR = min over the admissible pairs with that bit 1 - min over the admissible pairs with that bit 0
 *                       (neither set is empty: 4 points, 4 labels); +0 where no branch is left
 *       a known bit:    -GF3_LLR_KNOWN if it is 1, +GF3_LLR_KNOWN if it is 0, also where no branch is left
 *     GF3_LLR_KNOWN is finite, so nothing downstream forms inf - inf.  Minima round nothing: with d_known_u8 all zero the
 *     output is byte for byte gf3_mimo_detect's (d_w_f64 null) or gf3_mimo_detect_nw's.
 *     GF3_EINVAL for a null context, a context whose table is not mu = 2 with 4 points, B out of range, a null pointer (a
 *     null d_w_f64 selects the unweighted metric), F < 0, more than 65535 packets.  F == 0 is a no-op.
 *   One launch, no allocation, no host synchronisation, asynchronous on `stream`; every sum in a fixed order, no atomics:
 *   two calls give identical bytes.  The text of a refusal names the function.
 */
#define GF3_LLR_KNOWN 1e30f
int gf3_mimo_detect_known(gf3_ctx *ctx, int32_t B, const void *const *d_Y_c128, const void *const *d_H_c128,
                          const double *const *d_slope_f64, const double *d_w_f64, const uint8_t *d_bits_u8,
                          const uint8_t *d_known_u8, int64_t F, float *d_llr_f32, void *stream);

/*
 * Per-symbol phase and timing tracking inside a packet (not in the reference, whose channel model is fixed at the two
 * pilot blocks and interpolated linearly between them).  Opt-in; a stage of its own on the equalised symbols, before
 * any of the weights above.  Per packet, sequentially over the data symbols l = 0 .. D-1, two numbers are followed by a
 * decision-directed first-order loop with a velocity term: a common phase a (rad) and a phase slope b (rad per bin)
 * around the centre of the data band, kappa_c = k_c - mean(k) with k_c = data_bins[c] (the bins, in whatever order).
 *   state a = b = va = vb = 0 at the start of every packet; per symbol
 *     pa = a + va, pb = b + vb;   z_c = eq[l, c] exp(-i (pa + pb kappa_c));
 *     s_c = the point gf3_demap_hard picks for z_c (in-order scan, strict <); a z_c with a non-finite part is left out;
 *     r_c = z_c conj(s_c);  S0 = sum r_c, S1 = sum kappa_c r_c, S2 = sum kappa_c^2 r_c, E = sum |z_c - s_c|^2,
 *     P = sum |s_c|^2;   da = atan2(Im S0, Re S0) (0 for S0 = 0), u = exp(-i da), den = Re(u S2);
 *     measured <=> all seven real sums finite, den > 0 and E <= P:  a' = pa + da, b' = pb + Im(u S1) / den;
 *     else the symbol coasts: a' = pa, b' = pb;   va = a' - a, vb = b' - b, a = a', b = b';
 *     out[l, c] = eq[l, c] exp(-i (a + b kappa_c))   (non-finite inputs stay non-finite).
 *   No amplitude tracking, no cycle-slip detection (the model is anchored at the end pilots: phase[f, D-1] should be
 *   near zero), no per-carrier tracking; the lock range is first order: the change of velocity per symbol at the band
 *   edge must stay well inside the decision region.
 *   d_eq_c128, d_out_c128 [F*D, C]; d_out == d_eq is allowed (in place).  d_phase_f64 [F, D, 2] = (a, b) after each
 *   symbol, d_measured [F, D] = 0 / 1; both optional.  One workgroup per packet (the symbols depend on each other), a
 *   thread owns carriers t, t + 512, ...; each sum is formed in fp64 in a fixed order (a thread's carriers ascending, an
 *   xor butterfly 32, 16, .. 1 over the 64 lanes, the eight waves in order): two calls give identical bits.  No
 *   workspace.  F == 0 is a no-op; C <= 4096 (GF3_ERANGE beyond).
 */
int gf3_track_phase(gf3_ctx *ctx, const void *d_eq_c128, int64_t F, void *d_out_c128, double *d_phase_f64_or_null,
                    uint8_t *d_measured_or_null, void *stream);

/*
 * Decoder feedback: re-equalise from decoded codewords (not in the reference).  Opt-in; a stage of its own on the
 * equalised symbols (after gf3_track_phase where that runs), before any of the weights above.  The symbols of codewords
 * that decoded and can be trusted are known; the residual channel measured on them is smoothed over a small time x
 * frequency window and divided out of every symbol of the packet, the unknown ones included.  Per packet f, with
 * eq [F*D, C] as gf3_demod_frames returns it:
 *   d_bits_u8, d_known_u8 [F, D C mu]: one byte per coded bit (non-zero = 1) and per-bit mask, in TRANSMITTED order, packet ->
 *     symbol -> carrier -> bit: the order of gf3_soft_demap_csi's LLRs, before the interleaver is undone.
 *   symbol (l, c) is known <=> all mu of its known bytes are non-zero, both parts of eq[l, c] are finite and some table
 *     entry's label equals its mu bits; s[l, c] is then the first such entry in table order.
 *   r = eq conj(s), q = |s|^2 on known symbols, both 0 elsewhere.
 *   W(l, c) = the (l', c') of the same packet with |l' - l| <= half_symbols and |k_c' - k_c| <= half_bins, k_c =
 *     data_bins[c]: distance in BINS, whatever the order of the carriers.
 *   A = sum over W of r, B = sum over W of q, n = the known symbols in W: fp64 direct sums (no running add / subtract).
 *   g[l, c] = A / B when n >= min_known and A != 0, else 1;   out[l, c] = eq[l, c] / g[l, c]  (out = eq bit for bit where
 *     g = 1; non-finite inputs stay non-finite; a symbol that is itself unknown is corrected from its neighbours).
 *   0 <= half_symbols <= 8, 0 <= half_bins <= 64, min_known >= 1, C <= 4096.
 *   d_eq_c128, d_out_c128, d_gain_c128 (optional: g) [F*D, C]; d_out must not be d_eq (neighbours are still being read).
 *   GF3_EINVAL for null pointers, F < 0, arguments out of range, d_out == d_eq, work_bytes below
 *   gf3_feedback_workspace_bytes (which is 0: d_work may be null).  F == 0 is a no-op.  No allocation, no host
 *   synchronisation, asynchronous on `stream`.  One launch: a workgroup owns 8 symbols x 128 carriers in ascending-bin
 *   order, sums each column over the symbols (rows ascending), then the columns of a carrier's bin window (bins
 *   ascending) from LDS: a fixed order, no atomics -- two calls give identical bytes.
 */
int gf3_feedback_equalise(gf3_ctx *ctx, const void *d_eq_c128, const uint8_t *d_bits_u8, const uint8_t *d_known_u8,
                          int64_t F, int32_t half_symbols, int32_t half_bins, int32_t min_known,
                          void *d_out_c128, void *d_gain_c128_or_null, void *d_work, int64_t work_bytes, void *stream);
int64_t gf3_feedback_workspace_bytes(const gf3_ctx *ctx, int64_t F);

/*
 * Impulse blanking in the sample domain, between sync and demodulation (not in the reference).  Opt-in.  A click of a few
 * milliseconds otherwise costs the whole OFDM symbol it falls into; here the few samples that stand far above the packet's
 * own level are replaced by the baseline, and the symbol survives with a little less energy.
 *   The body of packet f is its M = 2P + D symbols of S = N + CP samples, [s_f, s_f + M S), s_f = d_frame_offsets[f] (the
 *   first pilot's cyclic prefix: what gf3_demod_frames takes).  Sample values are the stored ones widened to fp64 (u8 is
 *   0 .. 255 with its baseline near 128).
 *     per symbol m, over its n finite samples:  mean = sum v / n,  energy[f, m] = max(sum v^2 / n - mean^2, 0);
 *       n = 0: energy = +Inf, mean = 0;
 *     level: the symbol of 0-based rank (M - 1) / 4 among the packet's energies in ascending order (ties to the lower
 *       index) gives sigma_f = sqrt(its energy) and the baseline mu_f = its mean (0 if that is not finite);
 *       level[f] = (mu_f, sigma_f), T_f = kappa sigma_f;
 *     a sample of the body is flagged if it is not finite or |v - mu_f| > T_f (fp64, strict: T_f = 0 flags every sample
 *       that differs from mu_f, T_f = Inf only the non-finite ones);
 *     it is blanked if a flagged sample of the SAME body lies within `guard` samples of it (across symbol boundaries,
 *       never beyond the body: the chirp and the gaps are neither read nor written);
 *     a blanked sample of d_out becomes mu_f in the storage type (u8, i16: rint, half to even, clamped; f32: a cast);
 *     counts[f, m] = blanked samples of symbol m.
 *   A packet whose body is not inside [0, n_in) writes no sample: counts[f, :] = -1, energy[f, :] = 0, level[f] = (0, 0);
 *   the demodulator flags it as before.  Bodies are expected not to overlap; if they do, which packet's value lands in the
 *   shared samples is unspecified, and nothing outside the bodies is touched in any case.
 *   It cannot see a click that stays under kappa sigma, does not treat clicks on the chirp, and its level is wrong once
 *   more than about three quarters of a packet's symbols are hit or a quarter have faded.  On clean Gaussian-like samples
 *   kappa = 4.5 still blanks a few samples per packet.
 *   d_out is a second buffer of n_in samples that the caller has filled with a copy of d_in: the kernels read d_in only
 *   and write blanked samples of d_out only (a blanked neighbour cannot change a flag; two runs give identical bytes: every
 *   sum is formed in a fixed order, no floating-point atomics).  d_out == d_in, a null pointer, F < 0, kappa not finite or
 *   <= 0 and guard outside [0, 64] are GF3_EINVAL (the text names gf3_blank_impulses); F == 0 is a no-op.  The three
 *   report arrays d_energy_f64 [F, M], d_level_f64 [F, 2], d_counts_i32 [F, M] are required: they are the call's
 *   workspace too.  No allocation, no host synchronisation; asynchronous on `stream`.
 */
int gf3_blank_impulses(gf3_ctx *ctx, const void *d_in, int64_t n_in, const int64_t *d_frame_offsets, int64_t F,
                       double kappa, int32_t guard, void *d_out, double *d_energy_f64, double *d_level_f64,
                       int32_t *d_counts_i32, void *stream);

/*
 * Sampling-clock correction in the sample domain, between sync (and blanking) and demodulation (not in the reference).
 * Opt-in.  Two sound cards differ by tens to hundreds of ppm; the phase slope between the pilot blocks, which the
 * demodulator fits and removes, is the visible part of that offset, the inter-carrier interference inside every symbol
 * (about (pi k eps)^2 / 3 of carrier k's power) is not.  Here every packet body is resampled at its own rate.
 *   Clock model: receiver sample j of a body that starts at s holds the transmitted waveform at time j (1 + eps); eps > 0
 *   means the receiver took fewer samples than were sent; ppm = 1e6 eps.  From the fitted slope of gf3_demod_frames (the
 *   phase per carrier index accrued over the (P + D) S samples between the pilot blocks' centres):
 *       eps = slope N / (2 pi (P + D) S).
 *   Packet f: body [s_f, s_f + M S), s_f = d_frame_offsets[f], M = 2P + D, eps_f = d_eps_f64[f]; all in fp64:
 *       r   = 1.0 / (1.0 + eps_f)
 *       t_j = (double)j * r                       (one rounding; j = 0 .. M S - 1)
 *       i_j = floor(t_j),  mu = t_j - i_j,  q = mu * L,  p = min((int)q, L - 1),  a = q - p
 *       c_k = h[p][k] + a * (h[p+1][k] - h[p][k])           (k = 0 .. 2T - 1; formed with one fused multiply-add)
 *       out[f, j] = sum_k c_k * x[s_f + i_j + k - T + 1]    (ascending k, one fused multiply-add per tap; samples outside
 *                                                            [0, n_in) read as 0)
 *   Table: L = 1024 phases, rows p = 0 .. L, T = half_taps, Kaiser window with beta = 10:
 *       h[p][k] = sinc(u) I0(beta sqrt(1 - (u / T)^2)) / I0(beta),   u = (k - T + 1) - p / L,   window 0 for |u| >= T;
 *   rows 0 and L are unit impulses exactly, so eps = 0 returns the bodies unchanged for finite input.
 *   gf3_resample_coefficients writes the (L + 1) x 2T table to host memory: pure host code, no GPU, no context.
 *   Band: T = 16 keeps the interpolation error under -100 dB up to 0.74 pi (carriers <= 1500 of N = 4096), -40 dB at
 *   0.85 pi; T = 32 under -100 dB up to 0.85 pi, about -20 dB at 0.95 pi.  Neither reaches the top few percent of the
 *   band: full-band modes want T = 32 and still lose their highest carriers.
 *   d_out is a packed [F, M S] array in the context's storage type (fp64 as is, f32 by a cast, i16 / u8 by rint, half to
 *   even, clamped); frame offsets f M S into it feed every demodulator entry point.
 *   d_status_i32 [F]: bit 0 -- the body is not inside [0, n_in) (the rule of gf3_blank_impulses), the row is zeros;
 *   bit 1 -- eps_f is not finite or |eps_f| > 2e-3, the row is resampled with eps = 0 (a copy of the body).  Taps that
 *   merely reach past either end of the recording read zeros and set nothing: with eps < 0 the last end pilot of a
 *   recording that stops right after the body loses its last few samples.
 *   GF3_EINVAL (the text names the function) for a null pointer with F > 0, d_out == d_in, F < 0, n_in < 0, half_taps
 *   other than 16 or 32, and more than 2^31 - 1 tiles of 512 outputs in one call.  F == 0 is a no-op.  One launch, no
 *   atomics (two runs give identical bytes), asynchronous on `stream`.  The context holds the device copy of the table
 *   and makes it on the first call with that half_taps (one allocation and one blocking copy: not inside a stream
 *   capture); later calls neither allocate nor synchronise.
 */
int gf3_resample_coefficients(int32_t half_taps, double *h_out);
int gf3_resample_frames(gf3_ctx *ctx, const void *d_in, int64_t n_in, const int64_t *d_frame_offsets, int64_t F,
                        const double *d_eps_f64, int32_t half_taps, void *d_out, int32_t *d_status_i32, void *stream);

/*
 * Receive windowing, between sync (blanking, clock correction) and demodulation (not in the reference).  Opt-in.  Every
 * transform cuts a symbol out with a rectangle of N samples, and whatever is not periodic in N -- a whistle, a fan, the
 * interference a residual clock offset leaves -- leaks into every carrier with the rectangle's sidelobes, 1 / distance.
 * gf3_window_frames tapers the last L samples of every symbol's body and folds in the L samples one period (N) earlier,
 * the last L of its cyclic prefix.  Where the prefix outlasts the channel the two stretches carry the same signal, which
 * therefore passes unchanged, and everything else is seen through a window whose edges follow the ramp.
 *   Packet f: body [s_f, s_f + M S), s_f = d_frame_offsets[f], M = 2P + D, S = N + CP.  Symbol m with samples
 *   s[0 .. S) = x[s_f + m S ..), ramp r = d_ramp_f64 [L], 1 <= L <= CP; all in fp64, i = 0 .. L - 1:
 *       out[f, m S + S - L + i] = s[S - L + i] * (1 - r[i]) + s[CP - L + i] * r[i]
 *   (four rounded operations, of which the compiler may contract one into a fused multiply-add); every other sample of
 *   the body is copied.  The ramp is the caller's: any r with r[i] + r[L - 1 - i] = 1 keeps the window Nyquist.
 *   d_out is a packed [F, M S] array in the context's storage type (gf3_resample_frames' conversion: fp64 as is, f32 by a
 *   cast, i16 / u8 by rint, half to even, clamped); frame offsets f M S into it feed every demodulator entry point, and
 *   gf3_resample_frames' rows with their offsets are a valid input here.
 *   d_report_f64 [F, M, 2], per symbol: [0] = sum_i (s[S-L+i] - s[CP-L+i])^2, the prefix mismatch; [1] = sum_i
 *   (s[S-L+i]^2 + s[CP-L+i]^2).  Their ratio grows when the channel's tail reaches into the ramp.  A sample among those
 *   2L that is not finite makes that symbol's two sums NaN and no other's; in `out` it reaches the one or two outputs it
 *   enters.  Every sum runs in a fixed order (a thread's elements ascending, the wave butterfly, the waves in order).
 *   d_status_i32 [F]: bit 0 -- the body is not inside [0, n_in) (the rule of gf3_blank_impulses): the row is zeros and
 *   the packet's report NaN.
 *   GF3_EINVAL (the text names the function) for a null context, a null pointer with F > 0, d_out == d_in, F < 0,
 *   n_in < 0, L outside [1, CP] and more than 65535 packets in one call.  F == 0 is a no-op.  One launch, no atomics (two
 *   runs give identical bytes), no workspace, asynchronous on `stream`.  Samples are read and written at their element
 *   alignment; 16-byte accesses are taken where the addresses allow them.
 */
int gf3_window_frames(gf3_ctx *ctx, const void *d_in, int64_t n_in, const int64_t *d_frame_offsets, int64_t F,
                      const double *d_ramp_f64, int32_t L, void *d_out, double *d_report_f64, int32_t *d_status_i32,
                      void *stream);

/*
 * Whole-stream rate conversion, in front of the sync (not in the reference).  Opt-in.  Every kernel here assumes samples
 * taken at cfg.fs; a recording at 44.1, 88.2 or 96 kHz is 88 435 ppm and more away, far beyond what the per-packet
 * correction above can take.  gf3_resample_stream converts a stream by any ratio, in either direction, and can be cut
 * into blocks.
 *   r = input_rate / output_rate: input samples per output sample, a double in [0.25, 4].  T = half_taps = 16 or 32,
 *   h the table of gf3_resample_coefficients, [L + 1, 2T], L = 1024.  All in fp64, every product rounded once.
 *   Output j (a GLOBAL index, int64, j >= 0) reads at
 *       t_j = (double)j * r,   i_j = floor(t_j),   mu = t_j - i_j.
 *   r <= 1 (the input is the slower side): gf3_resample_frames' rule, by the same code:
 *       q = mu L,  p = min((int)q, L - 1),  a = q - p,  c_k = fma(a, h[p+1][k] - h[p][k], h[p][k])
 *       out[j] = sum_{k = 0 .. 2T-1} c_k x[i_j + k - T + 1]        (ascending k, one fused multiply-add per tap)
 *     r = 1 copies finite input exactly.
 *   r > 1 (the input is the faster side): the low-pass moves down to the OUTPUT's Nyquist frequency:
 *       rho = 1.0 / r,  Tw = (int)ceil(T r);  taps k = 0 .. 2 Tw - 1,  d = k - Tw + 1
 *       v = ((double)d - mu) rho,  n = ceil(v),  f = n - v,  q = f L,  p = min((int)q, L - 1),  a = q - p,  col = n + T - 1
 *       c_k = rho fma(a, h[p+1][col] - h[p][col], h[p][col]),   c_k = 0 where col lies outside [0, 2T)
 *       out[j] = sum_k c_k x[i_j + d]                               (ascending k, one fused multiply-add per tap)
 *   The input buffer d_in holds x[in_origin .. in_origin + n_in) in the stream's numbering, in the storage type in_dtype
 *   (a gf3_dtype; it need not be the context's); every sample outside it reads as 0.  The call writes outputs
 *   j = j0 .. j0 + n_out - 1 to d_out[0 .. n_out) in the CONTEXT's storage type (fp64 as is, f32 by a cast, i16 / u8 by
 *   rint, half to even, clamped): an 8- or 16-bit recording becomes float32 without a second context.
 *   Because j and the input index are global, a stream converted in blocks gives the bytes of the stream converted whole,
 *   as long as each block's buffer holds every sample its outputs' taps reach: i_j - Tw + 1 .. i_j + Tw (T for Tw where
 *   r <= 1).  A whole recording of n_in samples yields as many outputs as there are j >= 0 with (double)j r <= n_in - 1;
 *   outputs j with i_j + Tw <= n_seen - 1 are final once n_seen input samples have arrived.
 *   Band: as gf3_resample_frames, relative to the NARROWER of the two Nyquist frequencies: T = 16 within -100 dB up to
 *   0.74 of it, T = 32 up to 0.85; at r > 1 what lies above (2 - 0.74 | 0.85) of the output's Nyquist is rejected by
 *   more than 105 dB.  sum_k |c_k| < 2.8.
 *   GF3_EINVAL (the text names the function) for a null d_out, or a null d_in with n_in > 0, when n_out > 0;
 *   d_out == d_in; half_taps other than 16 or 32; in_dtype that is no gf3_dtype; r that is not finite or lies outside
 *   [0.25, 4]; a negative n_in, n_out, in_origin or j0; more than 2^31 - 1 tiles of 512 outputs; indices beyond 2^51.
 *   n_out == 0 is a no-op and needs no addresses.  No refusal writes anything.  One launch, no atomics (two runs give
 *   identical bytes), asynchronous on `stream`; the table is the context's, made on first use as for gf3_resample_frames.
 */
int gf3_resample_stream(gf3_ctx *ctx, const void *d_in, int32_t in_dtype, int64_t n_in, int64_t in_origin, double r,
                        int32_t half_taps, int64_t j0, int64_t n_out, void *d_out, void *stream);

/*
 * Quasi-cyclic LDPC codes (not in the reference, whose pyldpc code is marked broken there).  Lifting size Z = 64, 128
 * or 256; the shift table h_shifts [mb*nb] (row major, int16) holds -1 for a zero block and s in [0, Z) for the
 * circulant whose row z has its one in column (z + s) mod Z.  Block columns 0 .. nb-mb-1 carry the message (systematic
 * part), the last mb the parity; codeword bit j*Z + t is bit t of block column j.  n = Z nb, k = Z (nb - mb).  The
 * project's own families (rates 1/2, 2/3, 3/4, 5/6 at n = 1536, 3072, 6144) are
 * gf3_audio_modem_amd/data/qcldpc_z64.json, qcldpc_z128.json and qcldpc_z256.json.
 *   - gf3_ldpc_create validates Z in {64, 128, 256} (any other: GF3_EINVAL, the text names "Z=<value>"),
 *     0 < mb < nb <= 32, every shift in [-1, Z) and at least two non-zero blocks per block row, and uploads the table
 *     to the current device.  Z > 64 also needs mb <= 12 (GF3_EINVAL otherwise): codes of more block rows decode at
 *     Z = 64 only.  It records whether the parity part is dual-diagonal (first parity column shifts x, 0, x at rows 0,
 *     some middle row and mb-1; every other parity column shift 0 at rows c-1 and c): only then can gf3_ldpc_encode
 *     encode (GF3_EINVAL otherwise); any valid code decodes.  Error text of create / encode / decode:
 *     gf3_last_error(NULL), per calling thread.
 *   - a code object is immutable: share it across threads and streams freely.  Encode and decode are asynchronous on
 *     `stream` and run on the device the code was created on.
 *   - gf3_ldpc_encode: d_msg [n_cw, k] uint8 0/1 -> d_cw [n_cw, n] uint8 0/1, systematic first.
 *   - gf3_ldpc_decode: layered normalised min-sum (alpha = 0.75; block rows in order, within a row the non-zero
 *     blocks in column order), Z/64 wavefronts per codeword (one at Z = 64; at Z = 128, 256 one workgroup, its waves
 *     meeting at a barrier after every block row), stopping after the first full iteration whose decisions satisfy
 *     every check of the codeword, or after max_iter >= 1 iterations.  d_llr [n_cw, n] f32, LLR > 0 <=> bit 0;
 *     non-finite LLRs are outside the contract.  d_bits [n_cw, k] uint8 decisions of the systematic part
 *     (1 <=> APP < 0); d_app [n_cw, n] f32 a-posteriori LLRs or NULL; d_iters [n_cw] int32 or NULL: iterations used,
 *     -max_iter when the syndrome is still non-zero after max_iter.  The float32 arithmetic is fixed (no contraction)
 *     and the same for every Z: results are bit-identical to a float32 restatement of the same schedule.
 */
typedef struct gf3_ldpc gf3_ldpc;
int gf3_ldpc_create(int32_t mb, int32_t nb, int32_t Z, const int16_t *h_shifts, gf3_ldpc **out);
void gf3_ldpc_destroy(gf3_ldpc *code);
int32_t gf3_ldpc_n(const gf3_ldpc *code);
int32_t gf3_ldpc_k(const gf3_ldpc *code);
int gf3_ldpc_encode(const gf3_ldpc *code, const uint8_t *d_msg, int64_t n_cw, uint8_t *d_cw, void *stream);
int gf3_ldpc_decode(const gf3_ldpc *code, const float *d_llr, int64_t n_cw, int32_t max_iter,
                    uint8_t *d_bits, float *d_app_or_null, int32_t *d_iters_or_null, void *stream);

/*
 * Outer Reed-Solomon erasure code across codewords (not in the reference): R parity codewords per group of G data
 * codewords repair any R members of the group that the inner decoder reports as failed (d_iters < 0), exactly.
 * Stateless: no object, no workspace, no host synchronisation; asynchronous on `stream` of the current device.
 *   Field GF(2^8), polynomial x^8 + x^4 + x^3 + x^2 + 1 (0x11D).  Byte b of a member is its message bits 8b .. 8b+7,
 *   most significant first; every array holds one byte per bit (0 / 1) and must be 8-byte aligned.
 *   Parity is systematic, from the Cauchy matrix C[r][j] = 1 / (r xor (R + j)):  P_r[b] = xor_j C[r][j] D_j[b].
 *   1 <= R <= 16, G >= 1, G + R <= 255, k a multiple of 8 in [8, 2^20]: GF3_EINVAL otherwise, text in
 *   gf3_last_error(NULL).  NG == 0 is a no-op.
 *   - gf3_outer_encode: d_msg_bits [NG*G, k], member j of group g is row g*G + j  ->  d_par_bits [NG*R, k], row g*R + r.
 *   - gf3_outer_recover: d_bits [(G+R)*NG, k] in TRANSMITTED order, member t of group g is row t*NG + g (t < G data,
 *     then parity), repaired in place; d_iters [(G+R)*NG] in the same order, < 0 = erased; d_status [NG]:
 *       0     no data member erased: nothing is written;
 *       -e_d  e_d data members erased and fewer than e_d parity members survive: nothing is written;
 *       e_d   the e_d erased data members are rewritten from the surviving data members and the first e_d surviving
 *             parity members (in index order).  Erased rows are never read; parity rows are never written.
 *     A member whose decoder converged to a wrong codeword (iters > 0) counts as good: this call does not detect it.
 *     gf3_crc_check (below) does, where the codewords carry a CRC: it turns such a member's iters negative first.
 */
int gf3_outer_encode(const uint8_t *d_msg_bits, int64_t NG, int32_t G, int32_t R, int32_t k,
                     uint8_t *d_par_bits, void *stream);
int gf3_outer_recover(uint8_t *d_bits, const int32_t *d_iters, int64_t NG, int32_t G, int32_t R, int32_t k,
                      int32_t *d_status, void *stream);

/*
 * Per-codeword CRC-32 (not in the reference): the last 32 of a codeword's k message bits are the CRC of the k - 32
 * payload bits before them, so that a codeword the LDPC decoder converged on WRONGLY (zero syndrome, iters > 0) is seen
 * and can be erased for the outer code; an undetected error has probability 2^-32 per codeword.
 * Stateless: no object, no workspace, no host synchronisation; asynchronous on `stream` of the current device.
 *   CRC-32/IEEE (reflected polynomial 0xEDB88320, initial value and final xor 0xFFFFFFFF: zlib's crc32) of the payload
 *   bytes, byte b being payload bits 8b .. 8b+7, most significant first (the bytes of the outer code); message bit
 *   k - 32 + i is bit 31 - i of the CRC.  Every array holds one byte per bit (0 / 1; only bit 0 of an input byte is
 *   read) and the bit arrays must be 8-byte aligned; the payload array and the message array must not overlap.
 *   k a multiple of 8 in [40, 7936]: GF3_EINVAL otherwise, text in gf3_last_error(NULL).  n_cw == 0 is a no-op.
 *   - gf3_crc_attach: d_payload [n_cw, k - 32]  ->  d_msg [n_cw, k], each payload followed by its CRC field.
 *   - gf3_crc_check: d_msg [n_cw, k]; every output may be NULL.
 *       d_bad [n_cw]             1 where the field differs from the CRC of the row's payload, else 0;
 *       d_payload [n_cw, k - 32] the payload of every row, bad or not;
 *       d_iters [n_cw]           updated in place: v > 0 on a bad row becomes -v, every other value stays.  Afterwards
 *                                d_iters < 0 means "erase" to gf3_outer_recover, and |v| < max_iter on a bad row records
 *                                that the decoder had converged.
 *     Two runs give identical bytes (no atomics).
 */
int gf3_crc_attach(const uint8_t *d_payload, int64_t n_cw, int32_t k, uint8_t *d_msg, void *stream);
int gf3_crc_check(const uint8_t *d_msg, int64_t n_cw, int32_t k, uint8_t *d_payload_or_null,
                  int32_t *d_iters_or_null, uint8_t *d_bad_or_null, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GF3RX_H */
