// libgf3rx -- sampling-clock correction: packet bodies resampled with a windowed-sinc interpolator, between sync (and
// blanking) and demodulation (gf3_resample_frames, gf3_resample_coefficients); and, on the same table and arithmetic, the
// conversion of a whole stream from another sampling rate in front of the sync (gf3_resample_stream, further down).  See
// DESIGN.md §12.
//
// Clock model.  Receiver sample j of a body that starts at s holds the transmitted waveform at time j (1 + eps): eps > 0
// means the receiver took fewer samples than were sent; ppm = 1e6 eps.
// Correction of packet f (body [s_f, s_f + M S), M = 2P + D, offset eps_f), all in fp64:
//     r   = 1.0 / (1.0 + eps_f)                    (once)
//     t_j = (double)j * r                          (one rounding; j = 0 .. M S - 1)
//     i_j = floor(t_j),  mu = t_j - i_j,  q = mu * L,  p = min((int)q, L - 1),  a = q - p
//     c_k = h[p][k] + a * (h[p+1][k] - h[p][k])    (k = 0 .. 2T - 1; the kernel forms it as fma(a, h[p+1][k] - h[p][k], h[p][k]))
//     out[f, j] = sum_k c_k * x[s_f + i_j + k - T + 1]    (ascending k, one fma per tap; samples outside [0, n_in) read as 0)
// Coefficient table: L = 1024 phases, rows p = 0 .. L, T = half_taps = 16 or 32, Kaiser window with beta = 10:
//     h[p][k] = sinc(u) I0(beta sqrt(1 - (u / T)^2)) / I0(beta),   u = (k - T + 1) - p / L,   window 0 for |u| >= T
// with sin(pi u) taken as -(-1)^(k - T + 1) sin(pi p / L), so that rows 0 and L are unit impulses exactly: eps = 0 returns the
// body unchanged for finite input.  T = 16 holds -100 dB up to 0.74 pi, T = 32 up to 0.85 pi; neither reaches the top few
// percent of the band.
// `out` is a packed [F, M S] array in the context's storage type (gf3rx_storage.h); offsets f M S then feed any demodulator
// entry point.  status[f]: bit 0 -- the body is not inside [0, n_in) (body_start's rule of gf3rx_blank.hip), the row is zeros;
// bit 1 -- eps_f is not finite or |eps_f| > 2e-3, the row is resampled with eps = 0 (a copy).  Taps that merely reach past
// either end of the recording read zeros and set nothing: with eps < 0 the last end pilot of a recording that stops right
// after the body loses its last few samples.
//
// One launch, a workgroup per (packet, tile of RS_TILE outputs).  The tile's input window -- floor(j r) of its first output
// to that of its last, and T - 1 / T taps around them -- is staged once in LDS, widened to fp64.  A wave takes 64 consecutive
// outputs, lane by lane: consecutive lanes read consecutive LDS words (no bank conflict) and table rows that lie close
// together.  mu moves by |eps| from one output to the next, that is |eps| L table rows: 0.07 rows across a wave at 1 ppm,
// 3 at 50 ppm, 131 at the cap of 2e-3 -- at the offsets sound cards have, the lanes of a wave are NOT on one row, and every
// lane reads its own two rows.  Read from memory (the table, 264 KB at T = 16 and 528 KB at T = 32, stays in L2), those
// 16 T bytes per tap pair and lane are what bounds the kernel: the vector L1 returns 64 bytes a clock.  So a tile whose
// rows are few -- 512 |eps| L + 2 of them unless mu wraps inside the tile: up to 225 ppm at T = 16, 115 ppm at T = 32 --
// first copies them to LDS (RowCache), and a wave whose lanes all find their rows there (a ballot) reads them from LDS;
// any other wave reads the table in memory.  Both go through one expression (`interpolate`), so which way a wave went
// cannot be seen in the bits.  No atomics: two runs give identical bytes.
#include "gf3rx_host.h"
#include "gf3rx_storage.h"

namespace {

constexpr int RS_L = 1024;                                  // phases of the table (rows 0 .. RS_L)
constexpr double RS_BETA = 10.0;
constexpr double RS_MAX_EPS = 2e-3;
constexpr int RS_THREADS = 256, RS_TILE = 512;
// window of a tile: floor((j0 + RS_TILE - 1) r) - floor(j0 r) < (RS_TILE - 1) r + 1 <= 511 / (1 - 2e-3) + 1 < 514, plus 2T <= 64 taps
constexpr int RS_WIN = RS_TILE + 4 + 64;
static_assert((RS_TILE - 1) / (1.0 - RS_MAX_EPS) + 1.0 + 64.0 < RS_WIN, "a tile's input window fits the LDS buffer");
// the tile's table rows in LDS: 32 KB of rows padded by two words, so that row i starts 4 i banks on and up to 16 rows that
// the lanes of a wave are on do not collide (ds_read_b64: bank = dword address mod 64) -- 120 rows at T = 16, 62 at T = 32
constexpr int RS_TAB = 4096;
template <int T> struct RowCache { static constexpr int STRIDE = 2 * T + 2, ROWS = RS_TAB / STRIDE; };

struct ResampleArgs {
    const void* in; void* out; int64_t n_in; const int64_t* off; const double* eps; const double* h; int* status;
    int64_t len;                                            // M S
    int tiles;                                              // ceil(len / RS_TILE)
};

// Where output j reads: i_j = floor(t_j) as a double, the table row p and the weight a of row p + 1.  t_j = (double)j * r is
// rounded ONCE, as the definition says: a product contracted into the subtraction that follows it (the compiler's default)
// moves mu by an ulp of t_j, which the table's slope turns into 1e-12 of the output.
GF3_DEV double read_point(int64_t j, double r, int& p, double& al) {
#pragma clang fp contract(off)
    const double tj = (double)j * r;
    const double fl = floor(tj);
    const double q = (tj - fl) * RS_L;
    p = min((int)q, RS_L - 1);
    al = q - (double)p;
    return fl;
}

// one output from table rows h0 = h[p], h0 + STRIDE = h[p + 1] and the window samples w[0 .. 2T): the one expression both
// sources of the rows go through
template <int T, int STRIDE>
GF3_DEV double interpolate(const double* h0, double al, const double* w) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 2 * T; ++k) {
        const double c0 = h0[k], c1 = h0[STRIDE + k];
        acc = fma(fma(al, c1 - c0, c0), w[k], acc);
    }
    return acc;
}

template <int DT, int T>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(ResampleArgs a) {
    typedef typename RawT<DT>::E E;
    typedef RowCache<T> RC;
    __shared__ double win[RS_WIN];
    __shared__ __align__(16) double tab[RS_TAB];
    const int t = threadIdx.x;
    const int64_t f = blockIdx.x / a.tiles;
    const int tile = blockIdx.x % a.tiles;
    const int64_t s = a.off[f];
    const bool ragged = s < 0 || a.len > a.n_in || s > a.n_in - a.len;
    double eps = a.eps[f];
    const bool bad = !(fabs(eps) <= RS_MAX_EPS);            // (NaN and +-Inf too)
    if (bad) eps = 0.0;
    if (tile == 0 && t == 0) a.status[f] = (ragged ? 1 : 0) | (bad ? 2 : 0);
    const int64_t j0 = (int64_t)tile * RS_TILE, j1 = min(j0 + (int64_t)RS_TILE, a.len);
    E* out = (E*)a.out + f * a.len;
    if (ragged) {
        for (int64_t j = j0 + t; j < j1; j += RS_THREADS) out[j] = to_storage<DT>(0.0);
        return;
    }
    const double r = 1.0 / (1.0 + eps);
    const int64_t i_first = (int64_t)floor((double)j0 * r), i_last = (int64_t)floor((double)(j1 - 1) * r);
    const int W = min((int)(i_last - i_first) + 2 * T, RS_WIN);     // (never more: the static_assert above)
    const int64_t g0 = s + i_first - T + 1;                 // win[w] = x[g0 + w]
    const E* in = (const E*)a.in;
    for (int w = t; w < W; w += RS_THREADS) {
        const int64_t g = g0 + w;
        win[w] = (g >= 0 && g < a.n_in) ? (double)in[g] : 0.0;
    }
    // The rows this tile will ask for.  mu moves one way through a tile; where it does not wrap inside the tile (i_j - j is
    // the same at both ends) the rows lie between those of the first and the last output, plo .. phi, and go to LDS if
    // they fit.  Nothing depends on that argument: a lane that finds its row outside the cached range sends its wave to
    // the table in memory.
    int pa, pb;
    double unused;
    (void)read_point(j0, r, pa, unused);
    (void)read_point(j1 - 1, r, pb, unused);
    const int plo = min(pa, pb), phi = max(pa, pb) + 1;
    const bool cached = (i_first - j0) == (i_last - (j1 - 1)) && phi - plo + 1 <= RC::ROWS;
    if (cached) {
        const double* src = a.h + (size_t)plo * (2 * T);    // (rows lie one after the other: a linear, coalesced read)
        for (int e = t; e < (phi - plo + 1) * 2 * T; e += RS_THREADS) tab[(e / (2 * T)) * RC::STRIDE + (e % (2 * T))] = src[e];
    }
    __syncthreads();
    for (int64_t j = j0 + t; j < j1; j += RS_THREADS) {
        int p;
        double al;
        const double fl = read_point(j, r, p, al);
        // t_j is monotonic in j, so i_first <= i_j <= i_last and the 2T words from w on lie inside the window
        const double* w = win + min((int)((int64_t)fl - i_first), RS_WIN - 2 * T);
        const bool miss = !cached || p < plo || p >= phi;   // (rows p and p + 1 are both wanted)
        double v;
        if (__ballot(miss) == 0ull) v = interpolate<T, RC::STRIDE>(tab + (p - plo) * RC::STRIDE, al, w);
        else v = interpolate<T, 2 * T>(a.h + (size_t)p * (2 * T), al, w);
        out[j] = to_storage<DT>(v);
    }
}

// I0 by its power series: every term is positive, so the sum is good to a few ulp for 0 <= x <= beta
double bessel_i0(double x) {
    const double y = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; ++k) {
        term *= y / ((double)k * (double)k);
        sum += term;
        if (term < 1e-17 * sum) break;
    }
    return sum;
}

void fill_table(int T, double* h) {
    const double i0b = bessel_i0(RS_BETA);
    for (int p = 0; p <= RS_L; ++p)
        for (int k = 0; k < 2 * T; ++k) {
            const int n = k - T + 1;
            double v;
            if (p == 0 || p == RS_L) v = (n == (p ? 1 : 0)) ? 1.0 : 0.0;           // u is an integer: sinc is 1 at 0, else 0
            else {
                const double ph = (double)p / RS_L, u = (double)n - ph;
                if (fabs(u) >= (double)T) v = 0.0;
                else {
                    const double sn = ((n & 1) ? 1.0 : -1.0) * sin(M_PI * ph);      // sin(pi u) = -(-1)^n sin(pi p / L)
                    const double z = u / (double)T;
                    v = sn / (M_PI * u) * (bessel_i0(RS_BETA * sqrt(1.0 - z * z)) / i0b);
                }
            }
            h[(size_t)p * 2 * T + k] = v;
        }
}

// the context's device copy of the table for T, made on first use (gf3_ctx::d_resample_h, entered in c->owned)
const double* device_table(gf3_ctx* c, int T) {
    const int slot = T == 16 ? 0 : 1;
    std::lock_guard<std::mutex> lock(c->ws_mu);
    if (c->d_resample_h[slot]) return c->d_resample_h[slot];
    std::vector<double> h((size_t)(RS_L + 1) * 2 * T);
    fill_table(T, h.data());
    double* d = nullptr;
    if (hipMalloc((void**)&d, h.size() * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    c->owned.push_back(d);
    if (hipMemcpy(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    c->d_resample_h[slot] = d;
    return d;
}

template <int DT>
hipError_t launch_resample(const ResampleArgs& a, int T, int64_t grid, hipStream_t st) {
    if (T == 16) return launch(resample_kernel<DT, 16>, grid, RS_THREADS, 0, st, a);
    return launch(resample_kernel<DT, 32>, grid, RS_THREADS, 0, st, a);
}

// ---- whole-stream rate conversion (gf3_resample_stream; the rule is stated in include/gf3rx.h) ---------------------------
// One workgroup per tile of RS_TILE outputs j = j0 + tile RS_TILE ...; the tile's input window -- floor(j r) of its first
// output to that of its last and the taps around them -- is staged once in LDS, widened to fp64, zeros where it leaves the
// buffer.  A wave takes 64 consecutive outputs.  r <= 1 goes through read_point / interpolate, the frames kernel's own code;
// r > 1 widens the kernel to Tw = ceil(T r) taps to either side, and every tap of every lane has its own two table rows.
// Rows are read from the table in memory on both paths: a ratio such as 147/160 walks through its 160 phases in no order
// that a tile could cache as a range, and the table (264 / 528 KB) stays in L2.
constexpr double RS_MIN_RATIO = 0.25, RS_MAX_RATIO = 4.0;
constexpr int RS_MAX_TW = 128;                              // ceil(32 x 4)
// window of a tile: floor((j0 + RS_TILE - 1) r) - floor(j0 r) <= 511 x 4 + 1 = 2045 input steps, plus 2 Tw <= 256 taps
constexpr int RS_SWIN = 2304;
static_assert((RS_TILE - 1) * RS_MAX_RATIO + 1.0 + 2.0 * RS_MAX_TW <= RS_SWIN, "a tile's input window fits the LDS buffer");
static_assert(32 * RS_MAX_RATIO <= RS_MAX_TW, "Tw = ceil(T r) stays within RS_MAX_TW");

struct StreamArgs {
    const void* in; void* out; const double* h;
    int64_t n_in, in_origin, j0, n_out;
    double r;
};

// t_j = (double)j * r rounded once -> floor(t_j) as a double, mu = t_j - floor(t_j)  (read_point's first two lines)
GF3_DEV double read_time(int64_t j, double r, double& mu) {
#pragma clang fp contract(off)
    const double tj = (double)j * r;
    const double fl = floor(tj);
    mu = tj - fl;
    return fl;
}

// coefficient of the tap at distance d from floor(t_j) on the down path: the table read at u = (d - mu) rho = n - f,
// column n + T - 1, phase f; 0 where the column lies outside the table.  Every product is rounded once.
template <int T>
GF3_DEV double down_tap(const double* h, int d, double mu, double rho) {
#pragma clang fp contract(off)
    const double v = ((double)d - mu) * rho;
    const double n = ceil(v);
    const double q = (n - v) * RS_L;
    const int p = min((int)q, RS_L - 1);
    const double al = q - (double)p;
    const int col = (int)n + T - 1;
    const bool inside = col >= 0 && col < 2 * T;
    const double* h0 = h + (size_t)p * (2 * T) + (inside ? col : 0);
    const double c0 = h0[0], c1 = h0[2 * T];
    const double c = rho * fma(al, c1 - c0, c0);
    return inside ? c : 0.0;
}

template <int DI, int DO, int T>
__global__ __launch_bounds__(RS_THREADS) void resample_stream_kernel(StreamArgs a) {
    typedef typename RawT<DI>::E EI;
    typedef typename RawT<DO>::E EO;
    __shared__ double win[RS_SWIN];
    const int t = threadIdx.x;
    const int64_t ja = a.j0 + (int64_t)blockIdx.x * RS_TILE, jb = min(ja + (int64_t)RS_TILE, a.j0 + a.n_out);
    const double r = a.r;
    const bool down = r > 1.0;
    const int Tw = down ? min((int)ceil((double)T * r), RS_MAX_TW) : T;
    double unused;
    const int64_t i_first = (int64_t)read_time(ja, r, unused), i_last = (int64_t)read_time(jb - 1, r, unused);
    const int W = (int)min(i_last - i_first + 2 * (int64_t)Tw, (int64_t)RS_SWIN);     // (never more: the static_assert above)
    const int64_t g0 = i_first - Tw + 1 - a.in_origin;     // win[w] = in[g0 + w]
    const EI* in = (const EI*)a.in;
    for (int w = t; w < W; w += RS_THREADS) {
        const int64_t g = g0 + w;
        win[w] = (g >= 0 && g < a.n_in) ? (double)in[g] : 0.0;
    }
    __syncthreads();
    EO* out = (EO*)a.out;
    for (int64_t j = ja + t; j < jb; j += RS_THREADS) {
        double v;
        if (!down) {
            int p;
            double al;
            const double fl = read_point(j, r, p, al);
            const double* w = win + max(min((int)((int64_t)fl - i_first), RS_SWIN - 2 * T), 0);
            v = interpolate<T, 2 * T>(a.h + (size_t)p * (2 * T), al, w);
        } else {
            double mu;
            const double fl = read_time(j, r, mu);
            const double* w = win + max(min((int)((int64_t)fl - i_first), RS_SWIN - 2 * Tw), 0);
            const double rho = 1.0 / r;
            v = 0.0;
            for (int k = 0; k < 2 * Tw; ++k) v = fma(down_tap<T>(a.h, k - Tw + 1, mu, rho), w[k], v);
        }
        out[j - a.j0] = to_storage<DO>(v);
    }
}

template <int DI, int DO>
hipError_t launch_stream(const StreamArgs& a, int T, int64_t grid, hipStream_t st) {
    if (T == 16) return launch(resample_stream_kernel<DI, DO, 16>, grid, RS_THREADS, 0, st, a);
    return launch(resample_stream_kernel<DI, DO, 32>, grid, RS_THREADS, 0, st, a);
}

template <int DO>
hipError_t launch_stream_from(int in_dtype, const StreamArgs& a, int T, int64_t grid, hipStream_t st) {
    switch (in_dtype) {
        case DT_F64: return launch_stream<DT_F64, DO>(a, T, grid, st);
        case DT_F32: return launch_stream<DT_F32, DO>(a, T, grid, st);
        case DT_I16: return launch_stream<DT_I16, DO>(a, T, grid, st);
        default:     return launch_stream<DT_U8, DO>(a, T, grid, st);
    }
}

}  // namespace

extern "C" int gf3_resample_coefficients(int32_t half_taps, double* h_out) {
    if (half_taps != 16 && half_taps != 32) return fail(nullptr, GF3_EINVAL, "gf3_resample_coefficients: half_taps must be 16 or 32, not %d", half_taps);
    if (!h_out) return fail(nullptr, GF3_EINVAL, "gf3_resample_coefficients: null pointer");
    fill_table(half_taps, h_out);
    return GF3_OK;
}

extern "C" int gf3_resample_frames(gf3_ctx* c, const void* d_in, int64_t n_in, const int64_t* d_off, int64_t F, const double* d_eps,
                                   int32_t half_taps, void* d_out, int32_t* d_status, void* stream) {
    DeviceGuard dg(c);
    if (!c || F < 0 || n_in < 0) return fail(c, GF3_EINVAL, "gf3_resample_frames: bad argument");
    if (d_out && d_out == d_in) return fail(c, GF3_EINVAL, "gf3_resample_frames: d_out must be a second buffer, not d_in");
    if (half_taps != 16 && half_taps != 32) return fail(c, GF3_EINVAL, "gf3_resample_frames: half_taps must be 16 or 32, not %d", half_taps);
    if (F == 0) return GF3_OK;                              // (the arrays of no packets may be empty: no address)
    if (!d_in || !d_out || !d_off || !d_eps || !d_status) return fail(c, GF3_EINVAL, "gf3_resample_frames: null pointer");
    const int64_t len = (int64_t)(2 * c->cfg.P + c->cfg.D) * c->S;
    const int64_t tiles = (len + RS_TILE - 1) / RS_TILE;
    if (tiles > 0x7fffffff || F > 0x7fffffff / tiles)
        return fail(c, GF3_EINVAL, "gf3_resample_frames: at most 2^31 - 1 tiles of %d outputs per call (F = %lld packets of %lld samples)",
                    RS_TILE, (long long)F, (long long)len);
    const double* h = device_table(c, half_taps);
    if (!h) return fail(c, GF3_EHIP, "gf3_resample_frames: the coefficient table could not be made on the device");
    ResampleArgs a{d_in, d_out, n_in, d_off, d_eps, h, d_status, len, (int)tiles};
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_DT(c->cfg.in_dtype, HIPCHK(c, launch_resample<DTC>(a, half_taps, F * tiles, st)));
    return GF3_OK;
}

extern "C" int gf3_resample_stream(gf3_ctx* c, const void* d_in, int32_t in_dtype, int64_t n_in, int64_t in_origin, double r,
                                   int32_t half_taps, int64_t j0, int64_t n_out, void* d_out, void* stream) {
    DeviceGuard dg(c);
    constexpr int64_t EXACT = (int64_t)1 << 51;             // (double)j and j r <= 4 j stay exact integers / below 2^53
    if (!c || n_in < 0 || n_out < 0 || in_origin < 0 || j0 < 0) return fail(c, GF3_EINVAL, "gf3_resample_stream: bad argument (a negative count or index)");
    if (in_dtype < DT_F64 || in_dtype > DT_U8) return fail(c, GF3_EINVAL, "gf3_resample_stream: in_dtype must be one of GF3_F64 .. GF3_U8, not %d", in_dtype);
    if (d_out && d_out == d_in) return fail(c, GF3_EINVAL, "gf3_resample_stream: d_out must be a second buffer, not d_in");
    if (half_taps != 16 && half_taps != 32) return fail(c, GF3_EINVAL, "gf3_resample_stream: half_taps must be 16 or 32, not %d", half_taps);
    if (!(r >= RS_MIN_RATIO && r <= RS_MAX_RATIO)) return fail(c, GF3_EINVAL, "gf3_resample_stream: r must be a finite ratio in [0.25, 4], not %g", r);
    const int64_t tiles = n_out / RS_TILE + (n_out % RS_TILE ? 1 : 0);
    if (tiles > 0x7fffffff)
        return fail(c, GF3_EINVAL, "gf3_resample_stream: at most 2^31 - 1 tiles of %d outputs per call (n_out = %lld)", RS_TILE, (long long)n_out);
    if (n_in > EXACT || in_origin > EXACT || j0 > EXACT - n_out) return fail(c, GF3_EINVAL, "gf3_resample_stream: indices beyond 2^51");
    if (n_out == 0) return GF3_OK;                          // (no outputs: no address is needed)
    if (!d_out || (!d_in && n_in > 0)) return fail(c, GF3_EINVAL, "gf3_resample_stream: null pointer");
    const double* h = device_table(c, half_taps);
    if (!h) return fail(c, GF3_EHIP, "gf3_resample_stream: the coefficient table could not be made on the device");
    StreamArgs a{d_in, d_out, h, n_in, in_origin, j0, n_out, r};
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_DT(c->cfg.in_dtype, HIPCHK(c, launch_stream_from<DTC>(in_dtype, a, half_taps, tiles, st)));
    return GF3_OK;
}
