// libgf3rx -- impulse blanking in the sample domain, ahead of the demodulator (gf3_blank_impulses).  See DESIGN.md §12.
//
// The body of packet f is its M = 2P + D symbols of S = N + CP samples from the first pilot's prefix on, [s_f, s_f + M S).
//   1. per symbol m, over its finite samples: mean = sum v / n, energy = max(sum v^2 / n - mean^2, 0)   (n = 0: +Inf, mean 0)
//   2. the symbol of rank (M - 1) / 4 among the packet's energies (ties to the lower index) gives the level:
//      mu_f = its mean (0 if not finite), sigma_f = sqrt(its energy), T_f = kappa sigma_f
//   3. a sample is flagged if it is not finite or |v - mu_f| > T_f (fp64, strict)
//   4. a sample is blanked if a flagged sample of the same body lies within `guard` samples of it
//   5. blanked samples of `out` become mu_f in the storage type; nothing else of `out` is written
//
// Three launches on the caller's stream, no atomics on floating-point values, no workspace besides the report arrays:
//   blank_stats_kernel   one workgroup per (packet, symbol): thread t adds samples t, t + 256, ... ascending, the wave
//                        butterfly (xor 32 .. 1), then the four waves in order -> energy[f, m]; ragged packets get their
//                        energy = 0 and counts = -1 here
//   blank_level_kernel   one workgroup per packet: rank counting over the M energies, then the sums of the chosen symbol
//                        once more, in the same order -> level[f]
//   blank_write_kernel   one workgroup per (packet, symbol).  The body is cut into words of 64 samples counted from s_f; a
//                        wave turns 64 samples into one __ballot word.  The words that overlap the symbol and ONE more on
//                        each side (guard <= 64) go to LDS, the halo re-evaluated from d_in and clipped to the body.  A
//                        thread per word dilates by shifts and ORs of the 128-bit pairs (previous : this), (this : next),
//                        counts the bits that fall inside the symbol with __popcll, and the threads then store mu_f
//                        under the mask.  S is not a multiple of 64 in any mode, so a symbol's first and last word are
//                        shared with its neighbours: each workgroup counts and writes only its own samples.
// The kernels read d_in only and write d_out only under the mask: a blanked neighbour cannot change a flag, and two runs
// give identical bytes.
#include "gf3rx_host.h"
#include "gf3rx_storage.h"       // to_storage: mu in the storage type

namespace {

constexpr int BL_THREADS = 256, BL_WAVES = BL_THREADS / 64;

struct BlankArgs {
    const void* in; void* out; int64_t n_in; const int64_t* off;
    int M, S;
    double kappa; int guard;
    double* energy; double* level; int* counts;
};

// first sample of the packet's body, or -1 when the body is not inside [0, n_in)
GF3_DEV int64_t body_start(const BlankArgs& a, int64_t f) {
    const int64_t s = a.off[f], len = (int64_t)a.M * a.S;
    return (s < 0 || len > a.n_in || s > a.n_in - len) ? -1 : s;
}

// (sum v, sum v^2, n) over the finite samples of p[0 .. S), the same bits in every thread
template <typename E>
GF3_DEV void symbol_sums(const E* p, int S, double (*red)[3], double& sum, double& sq, double& n) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    double s1 = 0.0, s2 = 0.0, cn = 0.0;
#pragma unroll 4
    for (int i = t; i < S; i += BL_THREADS) {
        const double v = (double)p[i];
        const bool ok = fabs(v) < INFINITY;
        s1 += ok ? v : 0.0;
        s2 += ok ? v * v : 0.0;
        cn += ok ? 1.0 : 0.0;
    }
    s1 = wave_sum(s1); s2 = wave_sum(s2); cn = wave_sum(cn);
    __syncthreads();                                        // (earlier readers of red are done)
    if (lane == 0) { red[w][0] = s1; red[w][1] = s2; red[w][2] = cn; }
    __syncthreads();
    sum = red[0][0]; sq = red[0][1]; n = red[0][2];
#pragma unroll
    for (int i = 1; i < BL_WAVES; ++i) { sum += red[i][0]; sq += red[i][1]; n += red[i][2]; }
}

template <int DT>
__global__ __launch_bounds__(BL_THREADS) void blank_stats_kernel(BlankArgs a) {
    typedef typename RawT<DT>::E E;
    __shared__ double red[BL_WAVES][3];
    const int64_t f = blockIdx.x / a.M;
    const int m = blockIdx.x % a.M;
    const int64_t s = body_start(a, f);
    if (s < 0) {
        if (threadIdx.x == 0) { a.energy[f * a.M + m] = 0.0; a.counts[f * a.M + m] = -1; }
        return;
    }
    double sum, sq, n;
    symbol_sums((const E*)a.in + s + (int64_t)m * a.S, a.S, red, sum, sq, n);
    if (threadIdx.x == 0) {
        double e = INFINITY;
        if (n > 0.0) { const double mean = sum / n; e = fmax(sq / n - mean * mean, 0.0); }
        a.energy[f * a.M + m] = e;
    }
}

template <int DT>
__global__ __launch_bounds__(BL_THREADS) void blank_level_kernel(BlankArgs a) {
    typedef typename RawT<DT>::E E;
    __shared__ double red[BL_WAVES][3];
    __shared__ int pick;
    const int64_t f = blockIdx.x;
    const int64_t s = body_start(a, f);
    if (s < 0) {
        if (threadIdx.x == 0) { a.level[2 * f] = 0.0; a.level[2 * f + 1] = 0.0; }
        return;
    }
    const double* en = a.energy + f * a.M;
    const int rank = (a.M - 1) / 4;
    if (threadIdx.x == 0) pick = 0;
    __syncthreads();
    for (int m = threadIdx.x; m < a.M; m += BL_THREADS) {   // energies are never NaN: the order is total, one m matches
        const double e = en[m];
        int below = 0;
        for (int j = 0; j < a.M; ++j) {
            const double x = en[j];
            below += (x < e || (x == e && j < m)) ? 1 : 0;
        }
        if (below == rank) pick = m;
    }
    __syncthreads();
    const int m = pick;
    double sum, sq, n;
    symbol_sums((const E*)a.in + s + (int64_t)m * a.S, a.S, red, sum, sq, n);
    if (threadIdx.x == 0) {
        const double mean = n > 0.0 ? sum / n : 0.0;
        a.level[2 * f] = fabs(mean) < INFINITY ? mean : 0.0;
        a.level[2 * f + 1] = sqrt(en[m]);
    }
}

typedef unsigned long long u64;

// OR of the 128-bit value hi:lo shifted up by 0 .. g (0 <= g <= 64), its high word: bit i of the result is set when a
// bit of hi:lo at most g places below bit 64 + i is.  Doubling: shifts 0 .. c ORed with themselves shifted by s <= c + 1
// cover 0 .. c + s.  (Bits that leave the top belong to the next word, which forms them itself.)
GF3_DEV u64 smear_up(u64 lo, u64 hi, int g) {
    for (int c = 0; c < g;) {
        const int s = min(c + 1, g - c);                    // (1 .. 32: c runs 0, 1, 3, .. 63)
        hi |= (hi << s) | (lo >> (64 - s));
        lo |= lo << s;
        c += s;
    }
    return hi;
}
// the mirror image: hi:lo shifted down by 0 .. g, its low word
GF3_DEV u64 smear_down(u64 lo, u64 hi, int g) {
    for (int c = 0; c < g;) {
        const int s = min(c + 1, g - c);
        lo |= (lo >> s) | (hi << (64 - s));
        hi |= hi >> s;
        c += s;
    }
    return lo;
}

template <int DT>
__global__ __launch_bounds__(BL_THREADS) void blank_write_kernel(BlankArgs a) {
    typedef typename RawT<DT>::E E;
    extern __shared__ u64 words[];                          // [nw] flags, then [nw] dilated
    __shared__ int total;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t f = blockIdx.x / a.M;
    const int m = blockIdx.x % a.M;
    const int64_t s = body_start(a, f);
    if (s < 0) return;                                      // (counts = -1 is blank_stats_kernel's)
    const double mu = a.level[2 * f], T = a.kappa * a.level[2 * f + 1];
    const int64_t len = (int64_t)a.M * a.S;                 // samples of the body
    const int64_t lo = (int64_t)m * a.S, hi = lo + a.S;     // this symbol inside the body
    const int64_t w0 = (lo >> 6) - 1;                       // first word held (the lower halo; -1 for symbol 0)
    const int nw = (int)(((hi - 1) >> 6) - w0) + 2;         // the symbol's words and one on each side
    u64* flags = words;
    u64* dil = words + nw;
    const E* in = (const E*)a.in + s;
    if (t == 0) total = 0;
    for (int k = w; k < nw; k += BL_WAVES) {                // (uniform per wave: __ballot sees all 64 lanes)
        const int64_t i = (w0 + k) * 64 + lane;
        const bool inside = i >= 0 && i < len;
        const double v = inside ? (double)in[i] : mu;
        const bool flag = inside && (!(fabs(v) < INFINITY) || fabs(v - mu) > T);
        const u64 word = __ballot(flag);
        if (lane == 0) flags[k] = word;
    }
    __syncthreads();
    for (int k = 1 + t; k < nw - 1; k += BL_THREADS) {
        const u64 d = smear_up(flags[k - 1], flags[k], a.guard) | smear_down(flags[k], flags[k + 1], a.guard);
        dil[k] = d;
        const int64_t b = (w0 + k) * 64;                    // the word's first sample; own = its bits inside [lo, hi)
        u64 own = ~0ull;
        if (b < lo) own &= ~0ull << (lo - b);
        if (b + 64 > hi) own &= ~0ull >> (b + 64 - hi);
        const int c = __popcll(d & own);
        if (c) atomicAdd(&total, c);                        // (an integer count in LDS: order does not matter)
    }
    __syncthreads();
    E* out = (E*)a.out + s;
    const E rep = to_storage<DT>(mu);
    for (int64_t i = lo + t; i < hi; i += BL_THREADS) {
        const u64 d = dil[(i >> 6) - w0];
        if ((d >> (i & 63)) & 1ull) out[i] = rep;
    }
    if (t == 0) a.counts[f * a.M + m] = total;
}

template <int DT>
hipError_t launch_blank(const BlankArgs& a, int64_t F, hipStream_t st) {
    hipError_t e = launch(blank_stats_kernel<DT>, F * a.M, BL_THREADS, 0, st, a);
    if (e != hipSuccess) return e;
    e = launch(blank_level_kernel<DT>, F, BL_THREADS, 0, st, a);
    if (e != hipSuccess) return e;
    const size_t lds = 2 * sizeof(u64) * (size_t)(a.S / 64 + 4);          // nw <= S / 64 + 4
    return launch(blank_write_kernel<DT>, F * a.M, BL_THREADS, lds, st, a);
}

}  // namespace

extern "C" int gf3_blank_impulses(gf3_ctx* c, const void* d_in, int64_t n_in, const int64_t* d_off, int64_t F, double kappa,
                                  int32_t guard, void* d_out, double* d_energy, double* d_level, int32_t* d_counts, void* stream) {
    DeviceGuard dg(c);
    if (!c || F < 0 || n_in < 0) return fail(c, GF3_EINVAL, "gf3_blank_impulses: bad argument");
    if (d_out && d_out == d_in) return fail(c, GF3_EINVAL, "gf3_blank_impulses: d_out must be a second buffer, not d_in");
    if (!(kappa > 0.0) || !(kappa < INFINITY)) return fail(c, GF3_EINVAL, "gf3_blank_impulses: kappa must be finite and > 0");
    if (guard < 0 || guard > 64) return fail(c, GF3_EINVAL, "gf3_blank_impulses: guard must be in [0, 64]");
    if (F == 0) return GF3_OK;                              // (the arrays of no packets may be empty: no address)
    if (!d_in || !d_out || !d_off || !d_energy || !d_level || !d_counts) return fail(c, GF3_EINVAL, "gf3_blank_impulses: null pointer");
    const int M = 2 * c->cfg.P + c->cfg.D;
    if (F > 0x7fffffff / M) return fail(c, GF3_EINVAL, "gf3_blank_impulses: at most (2^31 - 1) / (2P + D) packets per call");
    if (c->S > (1 << 17)) return fail(c, GF3_ERANGE, "gf3_blank_impulses: N + CP <= 2^17");
    BlankArgs a{d_in, d_out, n_in, d_off, M, c->S, kappa, guard, d_energy, d_level, d_counts};
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_DT(c->cfg.in_dtype, HIPCHK(c, launch_blank<DTC>(a, F, st)));
    return GF3_OK;
}
