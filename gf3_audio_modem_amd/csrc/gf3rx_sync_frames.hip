// libgf3rx -- the frames-mode chirp sync: gf3_sync_frames* and the dispatch between the all-fp64 corr_kernel and the fp32
// screen with a proven bound (gf3rx_fscreen.h), in a list workspace the context keeps per stream and host thread (ctx_workspace, gf3rx_ctx.hip).
#include "gf3rx_host.h"
#include "gf3rx_fscreen.h"

// [count | pad | unresolved window numbers]
extern "C" int64_t gf3_sync_frames_workspace_bytes(const gf3_ctx* c, int64_t F) { return list_workspace_bytes(c, F); }

static thread_local LastCall g_fs_last;                       // (gf3_sync_frames_last)

// mode 0: all fp64 (corr_kernel on every window).  mode 1: fp32 screen with a proven bound per window (gf3rx_fscreen.h) in
// the caller's workspace; the windows it cannot decide are listed and corr_kernel runs on those.  mode -1 (auto, what plain
// gf3_sync_frames means): as mode 1 in a workspace the context owns, whenever the screen applies and such a workspace can
// be had; all fp64 otherwise.  The starts are the same every way.
static int sync_frames_impl(gf3_ctx* c, const void* d_in, int64_t n_in, int64_t F, int64_t stride, int32_t win_lo, int32_t win_hi,
                            int64_t* d_starts, double* d_peak, int32_t mode, void* d_work, float* dbg_y32, float* dbg_err, int* dbg_cls,
                            bool screen_only, void* stream) {
    DeviceGuard dg(c);
    if (c && F == 0) return GF3_OK;
    if (!c || !d_in || !d_starts || F < 0 || mode < -1 || mode > 1) return fail(c, GF3_EINVAL, "gf3_sync_frames: bad argument");
    const int W = win_hi - win_lo;
    const CorrPlan& pl = c->frames_plan;
    if (W < 3 || W > pl.W) return fail(c, GF3_EINVAL, "gf3_sync_frames: window %d outside [3, %d]", W, pl.W);
    hipStream_t st = (hipStream_t)stream;
    CorrArgs a{};
    a.t = pl.t; a.in = d_in; a.n_in = n_in; a.dt = c->cfg.in_dtype;
    a.Hq = pl.d_Hq; a.Q = pl.Q; a.Lp = pl.Lp; a.Lc = c->Lc; a.Wmax = W;
    a.stride = stride; a.win_lo = win_lo; a.W = W; a.starts = d_starts; a.peak = d_peak; a.thresh = c->cfg.thresh;
    const auto& fp = c->fscr;
    // the screen serves index-only calls within its plan's window; a caller that wants the fp64 peak VALUE gets the fp64 kernel
    const bool can_screen = fp.ok && W <= fp.wmax && !d_peak && F <= 0x7fffffff;
    if (mode == 1 && !d_work) mode = 0;
    void* work = mode == 1 ? d_work : nullptr;
    if (mode == -1 && can_screen) work = ctx_workspace(c, st, gf3_ctx::WS_SYNC, gf3_sync_frames_workspace_bytes(c, F));
    const bool screened = can_screen && work;
    if (screen_only && !screened) return fail(c, GF3_EINVAL, "gf3_debug_frames_screen: no screening plan for this window (max_window %d)", fp.wmax);
    g_fs_last.set(c, stream, screened ? 0 : 2, screened ? (int32_t)F : 0);
    if (!screened) {
        if (d_work) HIPCHK(c, hipMemsetAsync(d_work, 0, LIST_HEAD, st));      // a caller's workspace never keeps an earlier call's count
        HIPCHK(c, run_corr(c, pl, a, F, st));
        return GF3_OK;
    }
    int* count = (int*)work;
    int* list = (int*)((char*)work + LIST_HEAD);
    HIPCHK(c, hipMemsetAsync(count, 0, LIST_HEAD, st));
    FScreenArgs fa{d_in, n_in, c->cfg.in_dtype, fp.d_tw, fp.d_twn, fp.d_Hs, fp.d_H0N, fp.d_Hinf, fp.Q, fp.Lp, c->Lc, W,
                   stride, win_lo, W, (float)c->cfg.thresh, d_starts, list, count, dbg_y32, dbg_err, dbg_cls};
    HIPCHK(c, launch_fscreen(c, fa, F, st));
    if (screen_only) return GF3_OK;
    a.list = list; a.count = count;
    HIPCHK(c, run_corr(c, pl, a, F, st, true));               // (grid = the list's capacity; workgroups past its length return at once)
    return GF3_OK;
}
extern "C" int gf3_sync_frames(gf3_ctx* c, const void* d_in, int64_t n_in, int64_t F, int64_t stride,
                               int32_t win_lo, int32_t win_hi, int64_t* d_starts, double* d_peak, void* stream) {
    return sync_frames_impl(c, d_in, n_in, F, stride, win_lo, win_hi, d_starts, d_peak, -1, nullptr, nullptr, nullptr, nullptr, false, stream);
}
extern "C" int gf3_sync_frames_ex(gf3_ctx* c, const void* d_in, int64_t n_in, int64_t F, int64_t stride,
                                  int32_t win_lo, int32_t win_hi, int64_t* d_starts, double* d_peak, int32_t mode, void* d_work, void* stream) {
    return sync_frames_impl(c, d_in, n_in, F, stride, win_lo, win_hi, d_starts, d_peak, mode, d_work, nullptr, nullptr, nullptr, false, stream);
}
extern "C" int gf3_sync_frames_last(const gf3_ctx* c, void* stream, int32_t* path, int32_t* unresolved_capacity) {
    return g_fs_last.query("gf3_sync_frames_last", c, stream, path, unresolved_capacity);
}
// tests: the screening pass alone -- fp32 lags [F][W], the bound per window, the verdict per window (0 resolved with a
// detection, 1 resolved without, 2 unresolved: d_starts is then left alone), the unresolved windows in d_work
extern "C" int gf3_debug_frames_screen(gf3_ctx* c, const void* d_in, int64_t n_in, int64_t F, int64_t stride, int32_t win_lo, int32_t win_hi,
                                       int64_t* d_starts, float* d_y32, float* d_err, int32_t* d_cls, void* d_work, void* stream) {
    return sync_frames_impl(c, d_in, n_in, F, stride, win_lo, win_hi, d_starts, nullptr, 1, d_work, d_y32, d_err, d_cls, true, stream);
}
