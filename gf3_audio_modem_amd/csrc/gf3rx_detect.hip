// libgf3rx -- self-normalised chirp detection (gf3_detect_chunk / gf3_detect_decide): the Pearson correlation
// rho[g] of every full window of a buffer with the chirp replica, from P of the all-fp64 overlap-save (stream_corr,
// gf3rx_sync.hip) and the window's own sums of r and r^2; the lags above a threshold are listed, and the windowed-maximum
// rule is applied to the list.  Unlike the reference's rule (a threshold relative to the GLOBAL maximum, gf3rx_peak.h) the
// statistic carries its own scale, so a piece of a stream is decided without the rest of it.
//
// Window sums.  With x' = r - pivot (pivot: the buffer's first finite sample; rho does not change under a shift, and
// without it the 128^2 of 8-bit audio eats the mantissa -- with it the sums of the integer storages are exact), the
// buffer is cut into blocks of DET_BLOCK samples; det_totals_kernel sums x' and x'^2 per block, det_segscan_kernel turns
// the totals into prefixes that RESTART every DET_SEG_BLOCKS blocks (2^14 samples) and keeps each segment's total.  The
// window sum of the lag in front of a tile of DET_BLOCK lags is then a difference of two prefixes of at most 2^14 terms
// plus the totals of the segments in between, and inside the tile the sums advance by x'[g] - x'[g - Lc], scanned over
// the workgroup: no value that enters a window's V = S2 - S1^2 / Lc has seen more than 2^14 + Lc samples, whatever came
// earlier in the piece.  Every sum has a fixed order: two calls give identical bytes.
//
// Samples that are not finite count as x' = 0 and are counted per window (an integer sum of the same shape): a window
// that holds one has rho = NaN, and no other window does -- P is then taken from a copy of the buffer with those samples
// zeroed (the transforms of the overlap-save would spread them over whole output blocks).
#include "gf3rx_host.h"

#define DET_THREADS 256
#define DET_ITEMS 4
#define DET_BLOCK (DET_THREADS * DET_ITEMS)
#define DET_SEG_BLOCKS 16
#define DET_GUARD 0x1p-36                        /* silence guard: rho = 0 where V <= DET_GUARD * (largest V so far) */

// DET_ITEMS consecutive samples from i on as doubles; a sample outside [0, n) reads as `outside`.  One access of
// DET_ITEMS elements (16 bytes of f32) where all of them exist; element-aligned, as every sample access of the library is.
template <int DT> GF3_DEV void det_load(const void* p, int64_t i, int64_t n, double outside, double (&x)[DET_ITEMS]) {
    typedef typename RawT<DT>::E E;
    struct __attribute__((packed, aligned(sizeof(E)))) V4 { E v[DET_ITEMS]; };
    const E* s = (const E*)p;
    if (i >= 0 && i + DET_ITEMS <= n) {
        const V4 r = *(const V4*)(s + i);
#pragma unroll
        for (int k = 0; k < DET_ITEMS; ++k) x[k] = (double)r.v[k];
    } else {
#pragma unroll
        for (int k = 0; k < DET_ITEMS; ++k) x[k] = (i + k >= 0 && i + k < n) ? (double)s[i + k] : outside;
    }
}
// x' of a sample and whether it is not finite
GF3_DEV double det_centre(double x, double piv, int& bad) {
    const bool fin = fabs(x) < INFINITY;
    bad = fin ? 0 : 1;
    return fin ? x - piv : 0.0;
}
// Exclusive scans of one double per thread over the workgroup, in a fixed order (doubling steps inside a wave, the waves
// in sequence).  wtot: DET_THREADS / 64 doubles of LDS of the call's own; two barriers inside.
GF3_DEV double det_scan_sum(double v, double* wtot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double x = wave_scan(v, lane);
    const double up = __shfl_up(x, 1, 64);
    __syncthreads();
    if (lane == 63) wtot[wave] = x;
    __syncthreads();
    double off = 0.0;
    for (int w = 0; w < wave; ++w) off += wtot[w];
    return lane ? off + up : off;
}
GF3_DEV double det_scan_max(double v, double* wtot) {          // (fmax: a NaN operand is dropped)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const double y = __shfl_up(x, d, 64); if (lane >= d) x = fmax(x, y); }
    const double up = __shfl_up(x, 1, 64);
    __syncthreads();
    if (lane == 63) wtot[wave] = x;
    __syncthreads();
    double off = -INFINITY;
    for (int w = 0; w < wave; ++w) off = fmax(off, wtot[w]);
    return lane ? fmax(off, up) : off;
}

// scalars of a call: [0] pivot, [1] samples that are not finite (uint64), [2] the running maximum of V behind this piece,
// [3] lags to list (int64)
enum { DET_PIVOT = 0, DET_BAD = 1, DET_VRUN = 2, DET_TOTAL = 3 };

// one wave: the pivot = the first finite sample among the buffer's first 64, 0 if there is none
template <int DT> __global__ void det_pivot_kernel(const void* in, int64_t n, double* misc) {
    typedef typename RawT<DT>::E E;
    const int lane = threadIdx.x;
    const double v = lane < n ? (double)((const E*)in)[lane] : NAN;
    const unsigned long long m = __ballot(fabs(v) < INFINITY);
    const double p = __shfl(v, m ? __ffsll((long long)m) - 1 : 0, 64);
    if (lane == 0) { misc[DET_PIVOT] = m ? p : 0.0; ((unsigned long long*)misc)[DET_BAD] = 0ull; }
}
// per block of DET_BLOCK samples: the sums of x', of x'^2 and the number of samples that are not finite
template <int DT> __global__ __launch_bounds__(DET_THREADS) void det_totals_kernel(const void* in, int64_t n, const double* misc,
                                                                                 double* E1, double* E2, int* Eb) {
    __shared__ double scratch[16];
    const double piv = misc[DET_PIVOT];
    double x[DET_ITEMS];
    det_load<DT>(in, (int64_t)blockIdx.x * DET_BLOCK + threadIdx.x * DET_ITEMS, n, piv, x);
    double s1 = 0.0, s2 = 0.0, sb = 0.0;
#pragma unroll
    for (int k = 0; k < DET_ITEMS; ++k) { int bad; const double u = det_centre(x[k], piv, bad); s1 += u; s2 = fma(u, u, s2); sb += bad; }
    s1 = block_sum(s1, scratch);
    s2 = block_sum(s2, scratch);
    sb = block_sum(sb, scratch);
    if (threadIdx.x == 0) { E1[blockIdx.x] = s1; E2[blockIdx.x] = s2; Eb[blockIdx.x] = (int)sb; }
}
// one thread per segment of DET_SEG_BLOCKS blocks: the totals become exclusive prefixes inside the segment, in place; G =
// the segment's total
__global__ void det_segscan_kernel(double* E1, double* E2, int* Eb, int64_t nblk, double* G1, double* G2, int* Gb, int64_t nseg,
                                   double* misc) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nseg) return;
    double a1 = 0.0, a2 = 0.0;
    int ab = 0;
    for (int64_t b = s * DET_SEG_BLOCKS; b < nblk && b < (s + 1) * DET_SEG_BLOCKS; ++b) {
        const double t1 = E1[b], t2 = E2[b];
        const int tb = Eb[b];
        E1[b] = a1; E2[b] = a2; Eb[b] = ab;
        a1 += t1; a2 += t2; ab += tb;
    }
    G1[s] = a1; G2[s] = a2; Gb[s] = ab;
    if (ab) atomicAdd((unsigned long long*)misc + DET_BAD, (unsigned long long)ab);
}

struct DetArgs {
    const void* in; int64_t n; int Lc;
    const double* P;                             // [n + Lc - 1] the buffer's full convolution with the replica
    int64_t lag_lo, lag_hi, lag_offset, tile0;   // owned lags (full windows only); first tile of the launch
    double tau, sc, inv_lc, vc;                  // threshold; Sc, 1 / Lc, Ec - Sc^2 / Lc
    const double* misc;
    const double *E1, *E2; const int* Eb; const double *G1, *G2; const int* Gb;
    double* vtile;                               // pass 0: out, a tile's largest V; later: in, the largest V in front of the tile
    int64_t* counts; const int64_t* offsets; int64_t* idx; double* rho; double* rho_all;
};
// One tile of DET_BLOCK lags per workgroup.  PASS 0: the tile's largest V.  PASS 1: rho of the owned lags (written to
// rho_all when given), counted where rho > tau.  PASS 2: the counted lags written as (g - 1 + lag_offset, rho), ascending.
template <int DT, int PASS> __global__ __launch_bounds__(DET_THREADS) void det_rho_kernel(DetArgs a) {
    __shared__ double scratch[16];
    __shared__ double wtot[3][DET_THREADS / 64];
    __shared__ int wbad[DET_THREADS / 64], wcnt[DET_THREADS / 64];
    if (PASS == 2 && a.counts[blockIdx.x] == 0) return;
    const int tid = threadIdx.x;
    const int64_t t = a.tile0 + blockIdx.x, j0 = t * DET_BLOCK, jl = j0 - a.Lc;
    const double piv = a.misc[DET_PIVOT];
    // sums over the samples [jl, j0): the window of the lag in front of the tile (samples in front of the buffer count as
    // x' = 0: such windows are partial and owned by nobody)
    double S1 = a.E1[t], S2 = a.E2[t];
    int Sb = a.Eb[t];
    {
        const int64_t seg_hi = t / DET_SEG_BLOCKS;
        int64_t seg_from = 0;
        double h1 = 0.0, h2 = 0.0;
        int hb = 0;
        if (jl > 0) {                            // (the same in every thread)
            const int64_t b0 = jl / DET_BLOCK, seg_lo = b0 / DET_SEG_BLOCKS, i0 = b0 * DET_BLOCK + tid * DET_ITEMS;
            double z[DET_ITEMS];
            det_load<DT>(a.in, i0, a.n, piv, z);
            double p1 = 0.0, p2 = 0.0, pb = 0.0;
#pragma unroll
            for (int k = 0; k < DET_ITEMS; ++k)
                if (i0 + k < jl) { int bad; const double u = det_centre(z[k], piv, bad); p1 += u; p2 = fma(u, u, p2); pb += bad; }
            p1 = a.E1[b0] + block_sum(p1, scratch);              // [start of b0's segment, jl)
            p2 = a.E2[b0] + block_sum(p2, scratch);
            const int qb = a.Eb[b0] + (int)block_sum(pb, scratch);
            if (seg_lo == seg_hi) { h1 = -p1; h2 = -p2; hb = -qb; seg_from = seg_hi; }
            else { h1 = a.G1[seg_lo] - p1; h2 = a.G2[seg_lo] - p2; hb = a.Gb[seg_lo] - qb; seg_from = seg_lo + 1; }
        }
        for (int64_t s = seg_from; s < seg_hi; ++s) { h1 += a.G1[s]; h2 += a.G2[s]; hb += a.Gb[s]; }
        S1 += h1; S2 += h2; Sb += hb;
    }
    // the tile's own lags g = j0 + i: the sums advance by x'[g] - x'[g - Lc]
    const int64_t g0 = j0 + tid * DET_ITEMS;
    double xh[DET_ITEMS], xl[DET_ITEMS], s1[DET_ITEMS], s2[DET_ITEMS];
    int nb[DET_ITEMS];
    det_load<DT>(a.in, g0, a.n, piv, xh);
    det_load<DT>(a.in, g0 - a.Lc, a.n, piv, xl);
    {
        double r1 = 0.0, r2 = 0.0;
        int rb = 0;
#pragma unroll
        for (int k = 0; k < DET_ITEMS; ++k) {
            int bh, bl;
            const double uh = det_centre(xh[k], piv, bh), ul = det_centre(xl[k], piv, bl);
            r1 += uh - ul;
            r2 += fma(uh, uh, -(ul * ul));
            rb += bh - bl;
            s1[k] = r1; s2[k] = r2; nb[k] = rb;
        }
        const double o1 = S1 + det_scan_sum(r1, wtot[0]), o2 = S2 + det_scan_sum(r2, wtot[1]);
        int tb;
        const int ob = Sb + block_scan(rb, wbad, DET_THREADS / 64, tb);
#pragma unroll
        for (int k = 0; k < DET_ITEMS; ++k) { s1[k] += o1; s2[k] += o2; nb[k] += ob; }
    }
    double V[DET_ITEMS], run = -INFINITY;
    bool own[DET_ITEMS];
#pragma unroll
    for (int k = 0; k < DET_ITEMS; ++k) {
        V[k] = fma(-s1[k] * s1[k], a.inv_lc, s2[k]);
        own[k] = g0 + k >= a.lag_lo && g0 + k < a.lag_hi;
        if (own[k] && nb[k] == 0) run = fmax(run, V[k]);
        s2[k] = run;                                             // (from here on: the largest V of the thread's lags up to k)
    }
    if (PASS == 0) {
        run = block_max(run, scratch);
        if (tid == 0) a.vtile[blockIdx.x] = run;
        return;
    }
    const double seed = fmax(a.vtile[blockIdx.x], det_scan_max(run, wtot[2]));
    double p[DET_ITEMS];
    if (g0 + DET_ITEMS <= a.n + a.Lc - 1) {
        const double2 q0 = *(const double2*)(a.P + g0), q1 = *(const double2*)(a.P + g0 + 2);
        p[0] = q0.x; p[1] = q0.y; p[2] = q1.x; p[3] = q1.y;
    } else {
#pragma unroll
        for (int k = 0; k < DET_ITEMS; ++k) p[k] = (g0 + k < a.n + a.Lc - 1) ? a.P[g0 + k] : 0.0;
    }
    static_assert(DET_ITEMS == 4, "the accesses to P and rho_all are written for four lags per thread");
    int c = 0;
    unsigned flags = 0;
#pragma unroll
    for (int k = 0; k < DET_ITEMS; ++k) {
        double rho = 0.0;
        if (nb[k] != 0) rho = NAN;
        else if (V[k] > DET_GUARD * fmax(seed, s2[k])) rho = (p[k] - a.sc * fma(s1[k], a.inv_lc, piv)) / sqrt(a.vc * V[k]);
        p[k] = rho;
        if (own[k] && rho > a.tau && rho < INFINITY) { flags |= 1u << k; ++c; }
    }
    if (PASS == 1 && a.rho_all) {
        if (own[0] && own[DET_ITEMS - 1]) {
            *(double2*)(a.rho_all + g0) = make_double2(p[0], p[1]);
            *(double2*)(a.rho_all + g0 + 2) = make_double2(p[2], p[3]);
        } else {
#pragma unroll
            for (int k = 0; k < DET_ITEMS; ++k) if (own[k]) a.rho_all[g0 + k] = p[k];
        }
    }
    int total;
    const int before = block_scan(c, wcnt, DET_THREADS / 64, total);
    if (PASS == 1) { if (tid == 0) a.counts[blockIdx.x] = total; return; }
    int64_t o = a.offsets[blockIdx.x] + before;
#pragma unroll
    for (int k = 0; k < DET_ITEMS; ++k)
        if (flags & (1u << k)) { a.idx[o] = g0 + k - 1 + a.lag_offset; a.rho[o] = p[k]; ++o; }
}
// One workgroup: vtile[i] (a tile's largest V) -> the largest V in front of tile i, the carried value included;
// *vrun_out = the largest of all.
__global__ __launch_bounds__(DET_THREADS) void det_vscan_kernel(double* vtile, int64_t nt, const double* vrun_in, double* vrun_out) {
    __shared__ double wtot[DET_THREADS / 64];
    const int64_t per = (nt + DET_THREADS - 1) / DET_THREADS;
    const int64_t lo = min(nt, (int64_t)threadIdx.x * per), hi = min(nt, lo + per);
    double m = -INFINITY;
    for (int64_t i = lo; i < hi; ++i) m = fmax(m, vtile[i]);
    double run = fmax(fmax(vrun_in[0], 0.0), det_scan_max(m, wtot));
    for (int64_t i = lo; i < hi; ++i) { const double v = vtile[i]; vtile[i] = run; run = fmax(run, v); }
    if (threadIdx.x == DET_THREADS - 1) vrun_out[0] = run;
}
// the buffer with the samples that are not finite set to zero (f32 / f64 storage)
template <typename E> __global__ void det_clean_kernel(const E* in, int64_t n, E* out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const E v = in[i];
        out[i] = fabs((double)v) < INFINITY ? v : (E)0;
    }
}
// The windowed-maximum rule on a list (idx ascending, rho): entry i is a detection iff no entry within Lc - 1 of it has a
// larger rho, or the same rho at a smaller index; emitted iff its neighbourhood ends below final_below.  One workgroup.
__global__ __launch_bounds__(1024) void det_decide_kernel(const int64_t* idx, const double* rho, int64_t n, int64_t Lc, int64_t final_below,
                                                          int64_t* peaks, int64_t cap, int64_t* np) {
    __shared__ int wsum[16];
    __shared__ int64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t b0 = 0; b0 < n; b0 += 1024) {
        const int64_t i = b0 + threadIdx.x;
        int f = 0;
        if (i < n) {
            const int64_t g = idx[i];
            const double r = rho[i];
            f = (r == r && g + Lc <= final_below) ? 1 : 0;
            for (int64_t m = i - 1; f && m >= 0 && idx[m] > g - Lc; --m) if (rho[m] >= r) f = 0;
            for (int64_t m = i + 1; f && m < n && idx[m] < g + Lc; ++m) if (rho[m] > r) f = 0;
        }
        int tot;
        const int before = block_scan(f, wsum, 16, tot);
        if (f && carry + before < cap) peaks[carry + before] = idx[i];
        __syncthreads();
        if (threadIdx.x == 0) carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) { np[0] = carry; np[1] = carry > cap ? 2 : 0; }
}

// workspace: the overlap-save's own (gf3_sync_stream_workspace_bytes), then this unit's arrays
struct DetWs { int64_t nblk, nseg; size_t o_E1, o_E2, o_Eb, o_G1, o_G2, o_Gb, o_vt, o_cnt, o_off, o_misc, o_clean, total; };
static DetWs det_ws(const gf3_ctx* c, int64_t n) {
    DetWs w{};
    w.nblk = (n + DET_BLOCK - 1) / DET_BLOCK;
    w.nseg = (w.nblk + DET_SEG_BLOCKS - 1) / DET_SEG_BLOCKS;
    size_t o = ((size_t)gf3_sync_stream_workspace_bytes(c, n) + 255) & ~(size_t)255;
    auto take = [&](size_t bytes) { size_t r = o; o += (bytes + 255) & ~(size_t)255; return r; };
    w.o_E1 = take((size_t)w.nblk * 8); w.o_E2 = take((size_t)w.nblk * 8); w.o_Eb = take((size_t)w.nblk * 4);
    w.o_G1 = take((size_t)w.nseg * 8); w.o_G2 = take((size_t)w.nseg * 8); w.o_Gb = take((size_t)w.nseg * 4);
    w.o_vt = take((size_t)w.nblk * 8); w.o_cnt = take((size_t)w.nblk * 8); w.o_off = take((size_t)w.nblk * 8);
    w.o_misc = take(64);
    const int dt = c->cfg.in_dtype;
    w.o_clean = take(dt == DT_F64 ? (size_t)n * 8 : dt == DT_F32 ? (size_t)n * 4 : 0);
    w.total = o;
    return w;
}
extern "C" int64_t gf3_detect_chunk_workspace_bytes(const gf3_ctx* c, int64_t n) {
    if (!c || n < 1) return 0;
    return (int64_t)det_ws(c, n).total;
}

extern "C" int gf3_detect_chunk(const gf3_ctx* c, const void* d_buf, int64_t n, int64_t lag_lo, int64_t lag_hi, int64_t lag_offset, double tau,
                                double* d_vrun, int64_t* d_idx, double* d_rho, int64_t cap, int64_t* n_listed, double* d_rho_all,
                                void* d_work, void* stream) {
    DeviceGuard dg(c);
    if (!c || !d_buf || !d_vrun || !n_listed || !d_work || n < 3 || cap < 0 || (cap > 0 && (!d_idx || !d_rho)))
        return fail(c, GF3_EINVAL, "gf3_detect_chunk: bad argument");
    if (!(tau > 0.0 && tau < 1.0)) return fail(c, GF3_EINVAL, "gf3_detect_chunk: tau must be a finite number inside (0, 1)");
    const int64_t plen = n + c->Lc - 1;
    if (lag_lo < 0 || lag_hi > plen || lag_lo > lag_hi)
        return fail(c, GF3_EINVAL, "gf3_detect_chunk: lags [%lld, %lld) outside [0, %lld]", (long long)lag_lo, (long long)lag_hi, (long long)plen);
    *n_listed = 0;
    const int64_t lo = lag_lo > c->Lc - 1 ? lag_lo : c->Lc - 1, hi = lag_hi < n ? lag_hi : n;      // full windows only
    if (lo >= hi) return GF3_OK;
    hipStream_t st = (hipStream_t)stream;
    const DetWs w = det_ws(c, n);
    char* base = (char*)d_work;
    double* misc = (double*)(base + w.o_misc);
    int64_t *cnt = (int64_t*)(base + w.o_cnt), *offs = (int64_t*)(base + w.o_off);
    const int dt = c->cfg.in_dtype;
    DetArgs a{};
    a.in = d_buf; a.n = n; a.Lc = c->Lc;
    a.lag_lo = lo; a.lag_hi = hi; a.lag_offset = lag_offset; a.tile0 = lo / DET_BLOCK;
    a.tau = tau; a.sc = c->chirp_sum; a.inv_lc = 1.0 / (double)c->Lc; a.vc = c->chirp_var;
    a.misc = misc;
    a.E1 = (double*)(base + w.o_E1); a.E2 = (double*)(base + w.o_E2); a.Eb = (int*)(base + w.o_Eb);
    a.G1 = (double*)(base + w.o_G1); a.G2 = (double*)(base + w.o_G2); a.Gb = (int*)(base + w.o_Gb);
    a.vtile = (double*)(base + w.o_vt);
    a.counts = cnt; a.offsets = offs; a.idx = d_idx; a.rho = d_rho; a.rho_all = d_rho_all;
    const unsigned nt = (unsigned)((hi - 1) / DET_BLOCK - a.tile0 + 1);
    // the window sums' prefixes, P, the running maximum of V
    DISPATCH_DT(dt, hipLaunchKernelGGL((det_pivot_kernel<DTC>), dim3(1), dim3(64), 0, st, d_buf, n, misc));
    DISPATCH_DT(dt, hipLaunchKernelGGL((det_totals_kernel<DTC>), dim3((unsigned)w.nblk), dim3(DET_THREADS), 0, st, d_buf, n, (const double*)misc,
                                        (double*)a.E1, (double*)a.E2, (int*)a.Eb));
    hipLaunchKernelGGL(det_segscan_kernel, dim3((unsigned)((w.nseg + 255) / 256)), dim3(256), 0, st, (double*)a.E1, (double*)a.E2, (int*)a.Eb, w.nblk,
                       (double*)a.G1, (double*)a.G2, (int*)a.Gb, w.nseg, misc);
    double* P = nullptr;
    int rc = stream_corr(c, d_buf, n, d_work, &P, st);
    if (rc != GF3_OK) return rc;
    a.P = P;
    DISPATCH_DT(dt, hipLaunchKernelGGL((det_rho_kernel<DTC, 0>), dim3(nt), dim3(DET_THREADS), 0, st, a));
    hipLaunchKernelGGL(det_vscan_kernel, dim3(1), dim3(DET_THREADS), 0, st, a.vtile, (int64_t)nt, (const double*)d_vrun, misc + DET_VRUN);
    const void* h = nullptr;
    auto count = [&]() -> int {                  // rho of every owned lag, the lags to list counted; -> h = [bad, vrun, total]
        DISPATCH_DT(dt, hipLaunchKernelGGL((det_rho_kernel<DTC, 1>), dim3(nt), dim3(DET_THREADS), 0, st, a));
        launch_pk_scan(cnt, nt, offs, (int64_t*)misc + DET_TOTAL, st);
        HIPCHK(c, hipGetLastError());
        return read_back(c, st, &h, misc + DET_BAD, 24);
    };
    if ((rc = count()) != GF3_OK) return rc;
    if (*(const unsigned long long*)h != 0 && (dt == DT_F64 || dt == DT_F32)) {
        // samples that are not finite: P again, of the buffer with those samples zeroed -- the windows that hold one are
        // marked by their own count, every other window gets the P it would have without them
        void* clean = base + w.o_clean;
        const unsigned g = (unsigned)std::min<int64_t>((n + 255) / 256, 2048);
        if (dt == DT_F64) hipLaunchKernelGGL(det_clean_kernel<double>, dim3(g), dim3(256), 0, st, (const double*)d_buf, n, (double*)clean);
        else hipLaunchKernelGGL(det_clean_kernel<float>, dim3(g), dim3(256), 0, st, (const float*)d_buf, n, (float*)clean);
        if ((rc = stream_corr(c, clean, n, d_work, &P, st)) != GF3_OK) return rc;
        if ((rc = count()) != GF3_OK) return rc;
    }
    const int64_t want = ((const int64_t*)h)[2];
    *n_listed = want;
    if (want > cap) return fail(c, GF3_ERANGE, "gf3_detect_chunk: %lld lags to list exceed capacity %lld", (long long)want, (long long)cap);
    if (want > 0) DISPATCH_DT(dt, hipLaunchKernelGGL((det_rho_kernel<DTC, 2>), dim3(nt), dim3(DET_THREADS), 0, st, a));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(d_vrun, misc + DET_VRUN, 8, hipMemcpyDeviceToDevice, st));
    return GF3_OK;
}

extern "C" int gf3_detect_decide(const gf3_ctx* c, const int64_t* d_idx, const double* d_rho, int64_t n_listed, int64_t final_below,
                                 int64_t* d_peaks, int64_t cap, int64_t* n_peaks, void* d_work, void* stream) {
    DeviceGuard dg(c);
    if (!c || !d_peaks || !n_peaks || !d_work || n_listed < 0 || cap < 1 || (n_listed > 0 && (!d_idx || !d_rho)))
        return fail(c, GF3_EINVAL, "gf3_detect_decide: bad argument");
    hipStream_t st = (hipStream_t)stream;
    int64_t* np = (int64_t*)d_work;                            // [count, status]
    hipLaunchKernelGGL(det_decide_kernel, dim3(1), dim3(1024), 0, st, d_idx, d_rho, n_listed, (int64_t)c->Lc, final_below, d_peaks, cap, np);
    HIPCHK(c, hipGetLastError());
    const void* h = nullptr;
    const int rc = read_back(c, st, &h, np, 16);
    return rc != GF3_OK ? rc : finish_peaks(c, "gf3_detect_decide", (const int64_t*)h, cap, n_peaks);
}
