// The reference's peak rule (chirp_method, OFDM.py:359-361) and its maximum, stated once for every sync path: the frames
// window (corr_kernel), the all-fp64 stream path (pk_candidates), the screened stream path (scr_mlo_kernel,
// scr_decide_kernel) and the piece-wise host path (ck_list_kernel, ck_decide_kernel).
#pragma once
#include "gf3rx_device.h"

// Division first (OFDM.py:359-361): p = P / max(P), then a candidate is a local extremum or flat step above the
// threshold.  The arguments are the already divided values -- one correctly rounded division per lag, by the SIGNED
// maximum, shared by the lag's three uses -- so every caller divides before it asks.
GF3_DEV bool is_peak(double p0, double p1, double p2, double thresh) { return ((p1 - p0) * (p2 - p1) <= 0.0) && (p1 > thresh); }

// The prefilter: a lag with P < peak_limit(max, thresh) cannot pass is_peak, so it may skip its divisions.
// Why that is exact: with max and thresh positive and finite, lim = fl(thresh max (1 - 1e-6)) is within a few 2^-53 of the
// product, so P < lim puts the exact quotient P / max below thresh (1 - 1e-6 + 4e-16); the correctly rounded division moves
// it by at most 2^-53 relative and rounding is monotone: fl(P / max) < thresh.  A maximum or threshold that is not
// positive and finite excludes nothing (-INFINITY: the division by a negative maximum turns the order round, NaN compares
// false) -- `!(P < lim)` then keeps every lag, a NaN lag included.
GF3_DEV double peak_limit(double mx, double thresh) {
    const bool filt = mx > 0.0 && thresh > 0.0 && mx < INFINITY && thresh < INFINITY;
    return filt ? thresh * mx * (1.0 - 1e-6) : -INFINITY;
}

// np.amax over the block (OFDM.py:359: it propagates NaN).  mx: the thread's fmax accumulator, which drops NaN; nan: whether
// the thread saw one -- the or-reduced flag puts it back.  scratch: as block_max; contains barriers.
GF3_DEV double block_amax(double mx, bool nan, double* scratch) {
    mx = block_max(mx, scratch);
    return __syncthreads_or(nan ? 1 : 0) ? NAN : mx;
}
