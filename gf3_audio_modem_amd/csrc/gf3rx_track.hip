// libgf3rx -- per-symbol phase and timing tracking inside a packet (gf3_track_phase).  See DESIGN.md §12.
//
// Two numbers per data symbol, a common phase a and a phase slope b around the centre of the data band
// (kappa_c = data_bins[c] - mean(data_bins)), follow a decision-directed loop with a velocity term:
//   pa = a + va, pb = b + vb;  z_c = eq[l, c] exp(-i (pa + pb kappa_c));  s_c the point the hard decision picks for z_c
//   (nearest_point of gf3rx_demap.h: the in-order scan with strict <, the twin of the noise estimate's nearest_d2)
//   r_c = z_c conj(s_c);  S0 = sum r, S1 = sum kappa r, S2 = sum kappa^2 r, E = sum |z - s|^2, P = sum |s|^2
//   da = atan2(Im S0, Re S0), u = exp(-i da), den = Re(u S2);  measured <=> sums finite, den > 0, E <= P
//   measured: a' = pa + da, b' = pb + Im(u S1) / den;  else a' = pa, b' = pb;  va = a' - a, vb = b' - b
//   out[l, c] = eq[l, c] exp(-i (a' + b' kappa_c))
//
// The symbols of a packet depend on each other, so ONE workgroup owns a packet and walks its symbols; with few packets the
// call uses few compute units (as noise_estimate_cs_kernel).  Thread t owns the carriers t, t + 512, ...: a symbol's row
// sits in its registers from the load to the store, 16 bytes per carrier each way, and the next row's loads are issued
// before the reduction.  The eight partial sums go through the wave butterfly, meet in LDS and are added in wave order
// by lanes 0 .. 7 of EVERY wave (lane j adds sum j), which hand them to the wave's other lanes: every thread forms da, u,
// den and the gate from the same eight numbers, so the branch is uniform.  Two LDS sets alternate by symbol parity: a
// symbol costs one barrier (a wave can only write set p again after the barrier of the symbol in between, which every
// wave reaches after its reads of set p).  No atomics, no workspace: two runs give identical bits.
#include "gf3rx_demap.h"

namespace {

constexpr int TR_THREADS = 512, TR_WAVES = TR_THREADS / 64;
constexpr int TR_MAX_CPT = 8;            // carriers per thread at most: C <= 8 * 512

struct TrackArgs {
    const cplx* eq; cplx* out; double* phase; uint8_t* measured;
    const int* bins; double bin_mean;
    int D, C;
    DemapTab t;
};

// e exp(-i x)
GF3_DEV cplx derotate(cplx e, double x) {
    double s, c;
    sincos_fast(x, s, c);
    return cmk(e.x * c + e.y * s, e.y * c - e.x * s);
}

template <int HI, int CPT>
__global__ __launch_bounds__(TR_THREADS) void track_phase_kernel(TrackArgs a) {
    __shared__ double red[2][TR_WAVES][8];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int C = a.C;
    const int64_t base = (int64_t)blockIdx.x * a.D;
    const cplx* src = a.eq + base * C;
    cplx* dst = a.out + base * C;
    const Levels<HI> lv(a.t);
    double kap[CPT];
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int c = t + k * TR_THREADS;
        kap[k] = c < C ? (double)a.bins[c] - a.bin_mean : 0.0;
    }
    cplx cur[CPT], nxt[CPT];
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int c = t + k * TR_THREADS;
        cur[k] = c < C ? src[c] : cmk(0.0, 0.0);
        nxt[k] = cur[k];
    }
    double sa = 0.0, sb = 0.0, va = 0.0, vb = 0.0;
    for (int l = 0; l < a.D; ++l) {
        const double pa = sa + va, pb = sb + vb;
        if (l + 1 < a.D) {                                  // the next row travels while this one is reduced
            const cplx* row = src + (int64_t)(l + 1) * C;
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                const int c = t + k * TR_THREADS;
                if (c < C) nxt[k] = row[c];
            }
        }
        double acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.0;
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const cplx z = derotate(cur[k], pa + pb * kap[k]);
            const bool ok = t + k * TR_THREADS < C && fabs(z.x) < INFINITY && fabs(z.y) < INFINITY;
            const cplx s = nearest_point<HI>(z, lv, a.t);
            const cplx r = cmul_conj(z, s);
            const double dx = z.x - s.x, dy = z.y - s.y, kp = kap[k], k2 = kp * kp;
            acc[0] += ok ? r.x : 0.0;
            acc[1] += ok ? r.y : 0.0;
            acc[2] += ok ? kp * r.x : 0.0;
            acc[3] += ok ? kp * r.y : 0.0;
            acc[4] += ok ? k2 * r.x : 0.0;
            acc[5] += ok ? k2 * r.y : 0.0;
            acc[6] += ok ? dx * dx + dy * dy : 0.0;
            acc[7] += ok ? s.x * s.x + s.y * s.y : 0.0;
        }
        double* set = &red[l & 1][0][0];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const double x = wave_sum(acc[j]);
            if (lane == 0) set[w * 8 + j] = x;
        }
        lds_barrier();
        double mine = set[lane & 7];                        // lane j (and its copies j + 8, ...) adds sum j in wave order
#pragma unroll
        for (int i = 1; i < TR_WAVES; ++i) mine += set[i * 8 + (lane & 7)];
        double tot[8];
        bool fin = true;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            tot[j] = __shfl(mine, j, 64);
            fin = fin && fabs(tot[j]) < INFINITY;
        }
        const double da = atan2_fast(tot[1], tot[0]);
        double us, uc;
        sincos_fast(da, us, uc);                            // u = (uc, -us)
        const double den = uc * tot[4] + us * tot[5];       // Re(u S2)
        const bool meas = fin && den > 0.0 && tot[6] <= tot[7];
        double na = pa, nb = pb;
        if (meas) {
            na = pa + da;
            nb = pb + (uc * tot[3] - us * tot[2]) / den;    // Im(u S1) / den
        }
        va = na - sa; vb = nb - sb; sa = na; sb = nb;
        cplx* orow = dst + (int64_t)l * C;
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int c = t + k * TR_THREADS;
            if (c < C) orow[c] = derotate(cur[k], sa + sb * kap[k]);
            cur[k] = nxt[k];
        }
        if (t == 0) {
            if (a.phase) { a.phase[2 * (base + l)] = sa; a.phase[2 * (base + l) + 1] = sb; }
            if (a.measured) a.measured[base + l] = meas ? 1 : 0;
        }
    }
}

hipError_t launch_track(const gf3_ctx* c, const TrackArgs& a, int64_t F, hipStream_t st) {
    const int cpt = (a.C + TR_THREADS - 1) / TR_THREADS;
    return with_grid_bits(c, [&](auto hi) {
        constexpr int HI = decltype(hi)::value;
        if (cpt <= 1) return launch(track_phase_kernel<HI, 1>, F, TR_THREADS, 0, st, a);
        if (cpt <= 2) return launch(track_phase_kernel<HI, 2>, F, TR_THREADS, 0, st, a);
        if (cpt <= 3) return launch(track_phase_kernel<HI, 3>, F, TR_THREADS, 0, st, a);
        if (cpt <= 4) return launch(track_phase_kernel<HI, 4>, F, TR_THREADS, 0, st, a);
        return launch(track_phase_kernel<HI, TR_MAX_CPT>, F, TR_THREADS, 0, st, a);
    });
}

}  // namespace

extern "C" int gf3_track_phase(gf3_ctx* c, const void* d_eq, int64_t F, void* d_out, double* d_phase, uint8_t* d_measured,
                               void* stream) {
    DeviceGuard dg(c);
    if (c && F == 0) return GF3_OK;
    if (!c || !d_eq || !d_out || F < 0) return fail(c, GF3_EINVAL, "gf3_track_phase: bad argument");
    if (F > 0x7fffffff) return fail(c, GF3_EINVAL, "gf3_track_phase: at most 2^31 - 1 packets per call");
    if (c->cfg.C > TR_MAX_CPT * TR_THREADS) return fail(c, GF3_ERANGE, "gf3_track_phase: C <= 4096");
    TrackArgs a{(const cplx*)d_eq, (cplx*)d_out, d_phase, d_measured, c->d_bins, c->bin_mean, c->cfg.D, c->cfg.C, demap_tab(c)};
    HIPCHK(c, launch_track(c, a, F, (hipStream_t)stream));
    return GF3_OK;
}
