// Host-side table arithmetic of the context's plans: twiddle sets, the fp64 host FFT and the two single-precision
// screening plans (gf3rx_screen.h, gf3rx_fscreen.h).  Everything here is computed in fp64 / long double and rounded once
// to the element type; nothing here calls HIP -- gf3rx_ctx.hip uploads what these functions return.
#pragma once
#include "gf3rx_host.h"
#include "gf3rx_fscreen.h"

// tw[m] = exp(-2 pi i m / NC), m < NC;  twn[k] = exp(-2 pi i k / (2 NC)), k < n_twn.  T: cplx or cf.
template <typename T> struct Twiddles { std::vector<T> tw, twn; };
template <typename T>
inline Twiddles<T> make_twiddles(int NC, int n_twn) {
    typedef decltype(T::x) R;
    const long double PI2 = 6.283185307179586476925286766559005768L;
    Twiddles<T> t{std::vector<T>(NC), std::vector<T>(n_twn)};
    for (int m = 0; m < NC; ++m) { const long double a = -PI2 * m / NC; t.tw[m].x = (R)cosl(a); t.tw[m].y = (R)sinl(a); }
    for (int k = 0; k < n_twn; ++k) { const long double a = -PI2 * k / (2 * NC); t.twn[k].x = (R)cosl(a); t.twn[k].y = (R)sinl(a); }
    return t;
}

// iterative radix-2, a few hundred kflop per plan
inline void host_fft(std::vector<double>& re, std::vector<double>& im) {           // in place, length a power of two
    const size_t n = re.size();
    for (size_t i = 1, j = 0; i < n; ++i) {
        size_t bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) { std::swap(re[i], re[j]); std::swap(im[i], im[j]); }
    }
    for (size_t len = 2; len <= n; len <<= 1) {
        for (size_t i = 0; i < n; i += len)
            for (size_t k = 0; k < len / 2; ++k) {
                const long double ang = -6.283185307179586476925286766559005768L * (long double)k / (long double)len;
                const double wr = (double)cosl(ang), wi = (double)sinl(ang);
                const size_t a = i + k, b = i + k + len / 2;
                const double xr = re[b] * wr - im[b] * wi, xi = re[b] * wi + im[b] * wr;
                re[b] = re[a] - xr; im[b] = im[a] - xi;
                re[a] += xr; im[a] += xi;
            }
    }
}

// What a screening kernel is handed: spectra of the chirp partitions in its slot order with max |H_q| per partition for the
// error bound, and its twiddles.  L: partition length (the stream plan's hop H, the frames plan's Lp).  Hb, ecoef, ring:
// the band-limited extras of the stream plan only.  ok = false: outside the plan's range (fp64 path only).
struct ScreenPlanHost {
    bool ok = false, ring = false;
    int Q = 0, L = 0;
    Twiddles<cf> tw;
    std::vector<float> Hs, H0N, Hinf, Hb, ecoef;
};

// Partition q (taps [q L, (q + 1) L) of the chirp) zero-padded to N = 2 NC and transformed; Hinf and H0N of slot q filled in.
struct Spectrum { std::vector<double> re, im; };
inline Spectrum partition_spectrum(const std::vector<double>& chirp, int q, int NC, ScreenPlanHost& p) {
    const int N = 2 * NC, Lc = (int)chirp.size();
    Spectrum s{std::vector<double>(N, 0.0), std::vector<double>(N, 0.0)};
    for (int k = 0; k < p.L && q * p.L + k < Lc; ++k) s.re[k] = chirp[(size_t)q * p.L + k];
    host_fft(s.re, s.im);
    double mx = 0.0;
    for (int k = 0; k <= NC; ++k) mx = fmax(mx, hypot(s.re[k], s.im[k]));
    p.Hinf[q] = (float)(mx * (1.0 + 1e-6));
    p.H0N[2 * q] = (float)s.re[0]; p.H0N[2 * q + 1] = (float)s.re[NC];
    return s;
}
// Pair slots of T threads x 8 rows: o[r][t] = (H[k], H[NC - k]), k = t + T r; lane 0 of row 0 takes the self-paired bin NC / 2.
inline void pack_pair_slots(const Spectrum& s, int NC, int T, float* o) {
    for (int r = 0; r < 8; ++r)
        for (int t = 0; t < T; ++t, o += 4) {
            const int k = (t == 0 && r == 0) ? NC / 2 : t + T * r;
            o[0] = (float)s.re[k]; o[1] = (float)s.im[k]; o[2] = (float)s.re[NC - k]; o[3] = (float)s.im[NC - k];
        }
}
inline ScreenPlanHost screen_plan_begin(int Q, int L, int NC, int T, int n_twn) {
    ScreenPlanHost p;
    p.Q = Q; p.L = L;
    p.Hs.resize((size_t)Q * 8 * T * 4); p.H0N.resize((size_t)Q * 2); p.Hinf.resize(Q);
    p.tw = make_twiddles<cf>(NC, n_twn);
    return p;
}

// Screening plan of the stream-mode sync (gf3rx_screen.h): 8192-sample windows.
inline ScreenPlanHost screen_plan_host(const std::vector<double>& chirp) {
    constexpr int NC = GF3_SCR_NC, N = 2 * GF3_SCR_NC, T = GF3_SCR_T, KS = GF3_SCR_KS;
    const int Lc = (int)chirp.size(), Q = (Lc + NC - 1) / NC;
    // hop = partition length: the full 4096 whenever the chirp needs more than one partition (the last one is short) --
    // every sample is then transformed exactly twice and the blocks are as few as they can be (config 3: 78 342
    // instead of 83 565 with six equal partitions of 3 840)
    int H = Q > 1 ? NC : Lc;
    H += H & 1;                                          // even: the kernel stores lag pairs
    if (Q > 16 || H > NC || H < 1024) return ScreenPlanHost{};   // (scr_cells_kernel's block mask assumes at most 64 blocks
                                                                 //  under one workgroup's 57 346 lags)
    ScreenPlanHost p = screen_plan_begin(Q, H, NC, T, NC / 2 + 1);
    // band-limited kernel: the kept bins in its slot order, and per partition the error per unit |x|_2 -- rounding
    // (GF3_SCR_GAMMA max|H_q|) plus the 2-norm of what the dropped bins |k| >= 256 KS hold (gf3rx_screen.h)
    p.Hb.resize((size_t)Q * (KS / 2) * T * 4); p.ecoef.resize(2 * (size_t)Q);
    double hout_sum = 0.0, hall_sum = 0.0;
    for (int q = 0; q < Q; ++q) {
        const Spectrum s = partition_spectrum(chirp, q, NC, p);
        const std::vector<double>&re = s.re, &im = s.im;
        pack_pair_slots(s, NC, T, &p.Hs[(size_t)q * 8 * T * 4]);
        for (int pr = 0; pr < KS / 2; ++pr)
            for (int t = 0; t < T; ++t) {
                const int k = t + 512 * pr;
                float* o = &p.Hb[(((size_t)q * (KS / 2) + pr) * T + t) * 4];
                o[0] = (float)re[k]; o[1] = (float)im[k]; o[2] = (float)re[k + 256]; o[3] = (float)im[k + 256];
            }
        double out2 = re[NC] * re[NC] + im[NC] * im[NC], all2 = 0.0;       // two-sided sums over the N bins of the real window
        for (int k = 256 * KS; k < NC; ++k) out2 += 2.0 * (re[k] * re[k] + im[k] * im[k]);
        for (int k = 0; k < N; ++k) all2 += re[k] * re[k] + im[k] * im[k];
        const double hout = sqrt(out2 / N) * (1.0 + 1e-9);
        p.ecoef[q] = (float)((double)GF3_SCR_GAMMA * ((double)p.Hinf[q] + hout) * (1.0 + 1e-6));   // per unit |x|_2
        p.ecoef[Q + q] = (float)(hout * (1.0 + 1e-6));                                             // per unit |x_out|_2
        hout_sum += hout; hall_sum += sqrt(all2 / N);
    }
    // (selective only when the chirp lives below the cut: the reference's 0-8 kHz sweep at 48 kHz drops ~1.3 %)
    p.ring = Q <= GF3_SCR_RQ && hout_sum <= 0.05 * hall_sum;
    p.ok = true;
    return p;
}

// Screening plan of the frames-mode sync (gf3rx_fscreen.h): 2048-sample transforms, partitions of 2048 - wmax + 1 taps.
inline ScreenPlanHost fscreen_plan_host(const std::vector<double>& chirp, int wmax) {
    constexpr int NC = GF3_FS_NC, N = 2 * GF3_FS_NC, T = 64;
    if (wmax < 3 || wmax > N / 2) return ScreenPlanHost{};      // (wider windows: the all-fp64 kernel only)
    const int Lp = N - wmax + 1, Q = ((int)chirp.size() + Lp - 1) / Lp;
    if (Q > 256) return ScreenPlanHost{};
    ScreenPlanHost p = screen_plan_begin(Q, Lp, NC, T, T);
    for (int q = 0; q < Q; ++q) pack_pair_slots(partition_spectrum(chirp, q, NC, p), NC, T, &p.Hs[(size_t)q * 8 * T * 4]);
    p.ok = true;
    return p;
}
