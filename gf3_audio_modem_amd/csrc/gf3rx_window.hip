// libgf3rx -- receive windowing: every symbol of a packet's body tapered into its cyclic prefix, between sync (blanking,
// clock correction) and demodulation (gf3_window_frames).  See DESIGN.md §12.
//
// The body of packet f is its M = 2P + D symbols of S = N + CP samples from s_f on.  Symbol m with samples s[0 .. S), ramp
// r[0 .. L), 1 <= L <= CP, all in fp64:
//     out[S - L + i] = s[S - L + i] * (1 - r[i]) + s[CP - L + i] * r[i]         (i = 0 .. L - 1; s[CP - L + i] lies N earlier)
// and every other sample is copied: `out` is a packed [F, M S] array in the storage type (gf3rx_storage.h), as
// gf3_resample_frames leaves one.  report[f, m] = (sum_i (s[S-L+i] - s[CP-L+i])^2, sum_i (s[S-L+i]^2 + s[CP-L+i]^2)); a sample
// among those 2L that is not finite makes the pair NaN.  A body that is not inside [0, n_in) (body_start's rule of
// gf3rx_blank.hip): status bit 0, a row of zeros, a NaN report.
//
// One launch, a workgroup per (packet, run of symbols): the run comes from symbols_per_group, about 8 workgroups per compute
// unit where there are symbols enough.  The kernel streams: S - L samples of a symbol are moved as they are, L take two more
// reads (the prefix sample, the ramp).  Samples are only element-aligned -- a packet starts where the sync found it -- so the
// workgroup writes the few samples in front of the first 16-byte boundary of its output one by one, then 16 bytes per lane
// and instruction, then the rest one by one; the reads are 16 bytes wide too where input and output share their offset
// within 16 bytes, and one element wide otherwise (consecutive lanes still read consecutive addresses).  No LDS besides the
// reduction's twelve words, no atomics: for the report thread t adds the ramp's samples t, t + 256, ... in ascending order,
// whatever the addresses, then the wave butterfly (xor 32 .. 1), then the four waves in order -- two runs give identical
// bytes, and so do two placements of the same arrays.
#include "gf3rx_host.h"
#include "gf3rx_storage.h"

namespace {

constexpr int WN_THREADS = 256, WN_WAVES = WN_THREADS / 64;

struct WindowArgs {
    const void* in; void* out; int64_t n_in; const int64_t* off; const double* ramp; double* report; int* status;
    int M, S, N, L;
    int run;                                                // symbols per workgroup
};

// one output of the ramp: a = s[S - L + i], b = s[CP - L + i]
template <int DT>
GF3_DEV typename RawT<DT>::E taper(double a, double b, double r) {
    return to_storage<DT>(a * (1.0 - r) + b * r);
}

// 16 bytes of samples as the vector unit moves them (an extended vector: its elements stay in registers)
template <typename E> struct Vec16 { typedef E T __attribute__((ext_vector_type(16 / sizeof(E)))); };

// One symbol: src[0 .. S) -> dst[0 .. S).  ALIGNED: src + head is a 16-byte address whenever dst + head is one.
template <int DT, bool ALIGNED>
GF3_DEV void window_symbol(const WindowArgs& a, const typename RawT<DT>::E* src, typename RawT<DT>::E* dst, int head, int nvec) {
    typedef typename RawT<DT>::E E;
    typedef typename Vec16<E>::T VE;
    constexpr int V = 16 / (int)sizeof(E);
    const int t = threadIdx.x;
    const int edge = a.S - a.L;                             // first sample of the ramp
    const double* ramp = a.ramp;
    for (int q = t; q < nvec; q += WN_THREADS) {
        const int j0 = head + q * V;
        VE v;
        if (ALIGNED) v = *(const VE*)(src + j0);
        else {
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] = src[j0 + k];
        }
        if (j0 + V > edge) {
            VE p = v;
            const bool wide = ALIGNED && j0 >= a.N;         // (N samples are a multiple of 16 bytes in every storage type)
            if (wide) p = *(const VE*)(src + j0 - a.N);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const int j = j0 + k;
                if (j >= edge) {                            // (j - N >= CP - L >= 0)
                    const E b = wide ? (E)p[k] : src[j - a.N];
                    v[k] = taper<DT>((double)v[k], (double)b, ramp[j - edge]);
                }
            }
        }
        *(VE*)(dst + j0) = v;
    }
    // the samples in front of the first 16-byte boundary of dst and behind the last
    const int tail0 = head + nvec * V, loose = head + (a.S - tail0);
    for (int e = t; e < loose; e += WN_THREADS) {
        const int j = e < head ? e : tail0 + (e - head);
        E v = src[j];
        if (j >= edge) v = taper<DT>((double)v, (double)src[j - a.N], ramp[j - edge]);
        dst[j] = v;
    }
}

template <int DT>
__global__ __launch_bounds__(WN_THREADS) void window_kernel(WindowArgs a) {
    typedef typename RawT<DT>::E E;
    constexpr int V = 16 / (int)sizeof(E);
    __shared__ double red[WN_WAVES][3];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t f = blockIdx.y;
    const int m0 = blockIdx.x * a.run, m1 = min(m0 + a.run, a.M);
    const int64_t len = (int64_t)a.M * a.S;
    const int64_t s = a.off[f];
    const bool ragged = s < 0 || len > a.n_in || s > a.n_in - len;
    if (blockIdx.x == 0 && t == 0) a.status[f] = ragged ? 1 : 0;
    E* row = (E*)a.out + f * len;
    double* report = a.report + 2 * (f * a.M);
    if (ragged) {
        const int64_t j1 = (int64_t)m1 * a.S;
        for (int64_t j = (int64_t)m0 * a.S + t; j < j1; j += WN_THREADS) row[j] = to_storage<DT>(0.0);
        for (int m = m0 + t; m < m1; m += WN_THREADS) { report[2 * m] = NAN; report[2 * m + 1] = NAN; }
        return;
    }
    for (int m = m0; m < m1; ++m) {
        const E* src = (const E*)a.in + s + (int64_t)m * a.S;
        E* dst = row + (int64_t)m * a.S;
        // dst is element-aligned: `head` samples lie in front of its first 16-byte boundary
        const int head = min((int)(((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u) / sizeof(E)), a.S);
        const int nvec = (a.S - head) / V;
        if ((((uintptr_t)(src + head)) & 15u) == 0) window_symbol<DT, true>(a, src, dst, head, nvec);
        else window_symbol<DT, false>(a, src, dst, head, nvec);
        // the report: thread t takes the ramp's samples t, t + 256, ... whatever the addresses, so that the sums' order is the
        // same for every placement of the arrays (the samples come from L1 / L2 a second time: 2L of a symbol's S + L reads)
        double diff = 0.0, both = 0.0, bad = 0.0;
        for (int i = t; i < a.L; i += WN_THREADS) {
            const double u = (double)src[a.S - a.L + i], v = (double)src[a.S - a.L + i - a.N];
            const double d = u - v;
            diff += d * d;
            both += u * u + v * v;
            bad += (fabs(u) < INFINITY && fabs(v) < INFINITY) ? 0.0 : 1.0;
        }
        const double s0 = wave_sum(diff), s1 = wave_sum(both), s2 = wave_sum(bad);
        __syncthreads();                                    // (the readers of the symbol before are done)
        if (lane == 0) { red[w][0] = s0; red[w][1] = s1; red[w][2] = s2; }
        __syncthreads();
        if (t == 0) {
            double sd = red[0][0], sb = red[0][1], nb = red[0][2];
#pragma unroll
            for (int i = 1; i < WN_WAVES; ++i) { sd += red[i][0]; sb += red[i][1]; nb += red[i][2]; }
            report[2 * m] = nb > 0.0 ? NAN : sd;
            report[2 * m + 1] = nb > 0.0 ? NAN : sb;
        }
    }
}

}  // namespace

extern "C" int gf3_window_frames(gf3_ctx* c, const void* d_in, int64_t n_in, const int64_t* d_off, int64_t F, const double* d_ramp,
                                 int32_t L, void* d_out, double* d_report, int32_t* d_status, void* stream) {
    DeviceGuard dg(c);
    if (!c || F < 0 || n_in < 0) return fail(c, GF3_EINVAL, "gf3_window_frames: bad argument");
    if (d_out && d_out == d_in) return fail(c, GF3_EINVAL, "gf3_window_frames: d_out must be a second buffer, not d_in");
    if (L < 1 || L > c->cfg.CP) return fail(c, GF3_EINVAL, "gf3_window_frames: L must be in [1, CP = %d], not %d", c->cfg.CP, L);
    if (int rc = too_many_packets(c, F, "gf3_window_frames")) return rc;
    if (F == 0) return GF3_OK;                              // (the arrays of no packets may be empty: no address)
    if (!d_in || !d_out || !d_off || !d_ramp || !d_report || !d_status) return fail(c, GF3_EINVAL, "gf3_window_frames: null pointer");
    const int M = 2 * c->cfg.P + c->cfg.D;
    const int run = symbols_per_group(c, F, M);
    WindowArgs a{d_in, d_out, n_in, d_off, d_ramp, d_report, d_status, M, c->S, c->cfg.N, L, run};
    const dim3 grid((unsigned)((M + run - 1) / run), (unsigned)F);
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_DT(c->cfg.in_dtype, { hipLaunchKernelGGL(window_kernel<DTC>, grid, dim3(WN_THREADS), 0, st, a); HIPCHK(c, hipGetLastError()); });
    return GF3_OK;
}
