// What the entries of the two joint detectors -- spatial multiplexing (gf3rx_mimo.hip) and the space-time code
// (gf3rx_stbc.hip) -- share on the host: the thread count of both kernels and what they refuse of a context.  The branch
// dispatch, the carrier-tile grid and the argument checks they share with other units are in gf3rx_host.h (with_branches,
// tile_grid, branches_ok, too_many_packets_i32).  See DESIGN.md §12, "The shared joint-detector pieces".
#pragma once
#include "gf3rx_demap.h"

// a workgroup of either detector owns JOINT_THREADS consecutive data carriers; thread = carrier (combine_kernel's shape)
constexpr int JOINT_THREADS = 256;

inline int needs_4_points(const gf3_ctx* c, const char* who) {
    if (c->cfg.mu == 2 && c->cfg.M == 4) return GF3_OK;
    return fail(c, GF3_EINVAL, "%s: the joint detector scans 4 x 4 pairs: a table of 4 points with mu = 2 (M=%d, mu=%d)", who,
                c->cfg.M, c->cfg.mu);
}
// gf3_mimo_pilots' cover, which the space-time code's entries need as well
inline int needs_even_cover(const gf3_ctx* c, const char* who) {
    if (c->cfg.P >= 2 && !(c->cfg.P & 1)) return GF3_OK;
    return fail(c, GF3_EINVAL, "%s: the two covers need an even number of pilot symbols, P >= 2 (P=%d)", who, c->cfg.P);
}
