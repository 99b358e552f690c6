// libgf3rx -- adaptive bit loading: the loading object (gf3_loading_*) and the noise pair for a packet whose carriers
// carry different QAM orders (gf3_noise_estimate_loaded, gf3_soft_demap_loaded).  See DESIGN.md §12.
//
//   order[c] in {0, 2, 4, 6}   Bs = sum_c order[c]   off[c] = sum(order[:c])  (even)
//   table of order m > 0: Gray-coded square 2^m-QAM of unit energy, binary-indexed per axis as Levels<m/2> wants it:
//     lv[i ^ (i >> 1)] = (2i - (L-1)) * (1 / sqrt(2 (L^2 - 1) / 3)), L = 2^(m/2)
//   order 0: no payload; the carrier transmits its bin's pilot symbol
//
//   v[f, c]            = (1/D) sum_l |eq[f, l, c] - s|^2, s the point of carrier c's table that the hard decision picks;
//                        the pilot symbol on a carrier of order 0
//   LLR[f, l, off[c]+b] = (float)(maxlog(eq[f, l, c]; table of order[c])[b] * w), +0 where w = 0
//   w                  = noise_weight (var) | csi_weight (Hs, He) | 1          (gf3rx_demap.h, as every other weight rule)
//
// The kernels have the shape of noise_estimate_kernel and soft_demap_nw_kernel (gf3rx_noise.hip) with the table chosen
// per carrier: the same work split, the same order of every sum, and the same pieces of gf3rx_demap.h (grid_min_d2,
// packet_vbar, noise_weight, csi_weight_mag, emit_grid_llr), so that an all-m loading gives the bits the uniform kernels give.
#include "gf3rx_demap.h"

// The three families' axis levels, by value in the kernel arguments.
struct LoadLevels { double lv1[2], lv2[4], lv3[8]; };

struct gf3_loading {
    const gf3_ctx* ctx = nullptr;       // the context it was made for (compared, never dereferenced through the handle)
    int C = 0, Bs = 0, device = 0;
    uint8_t* d_order = nullptr;         // [C]
    int* d_off = nullptr;               // [C + 1]
    cplx* d_known = nullptr;            // [C] the pilot symbol of each carrier's bin (read on carriers of order 0)
    LoadLevels lv{};
};

namespace {

constexpr int LE_WAVES = 8;             // as NE_WAVES of noise_estimate_kernel
constexpr int LD_THREADS = VBAR_THREADS; // as NW_THREADS of soft_demap_nw_kernel
enum { W_UNIT = 0, W_VAR = 1, W_CSI = 2 };

struct LoadArgs {
    const cplx* eq; double* var; const double* var_in; const cplx* Hs; const cplx* He; float* llr;
    const uint8_t* order; const int* off; const cplx* known; const int* bins;
    int D, C, Dc, Bs, K, P;
    LoadLevels lv;
};

// a wave's share of one carrier's sum on a 2^H x 2^H grid: symbols l = w, w + 8, ... ascending
template <int H>
GF3_DEV double grid_residual(const cplx* p, int w, int D, int C, const double (&lv)[1 << H]) {
    double acc = 0.0;
    for (int l = w; l < D; l += LE_WAVES) acc += grid_min_d2<(1 << H)>(p[(int64_t)l * C], lv, lv);
    return acc;
}

// noise_estimate_loaded: noise_estimate_kernel's structure -- 64 carriers per workgroup, lane = carrier, wave w takes
// the symbols w, w + 8, ..., the partial sums are added in the order of w and divided by D.  A lane's order does not
// change over the symbols, so the branch on it stands outside the loop: a wave runs one loop per order present in it.
__global__ __launch_bounds__(64 * LE_WAVES) void noise_estimate_loaded_kernel(LoadArgs a) {
    __shared__ double part[LE_WAVES][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int64_t f = blockIdx.y;
    double acc = 0.0;
    if (c < a.C) {
        const cplx* p = a.eq + (f * a.D) * (int64_t)a.C + c;
        switch (a.order[c]) {
            case 2: acc = grid_residual<1>(p, w, a.D, a.C, a.lv.lv1); break;
            case 4: acc = grid_residual<2>(p, w, a.D, a.C, a.lv.lv2); break;
            case 6: acc = grid_residual<3>(p, w, a.D, a.C, a.lv.lv3); break;
            default: {
                const cplx s = a.known[c];
                for (int l = w; l < a.D; l += LE_WAVES) {
                    const cplx e = p[(int64_t)l * a.C];
                    const double dx = e.x - s.x, dy = e.y - s.y;
                    acc += dx * dx + dy * dy;
                }
            }
        }
    }
    part[w][lane] = acc;
    __syncthreads();
    if (w == 0 && c < a.C) {
        double s = part[0][lane];
#pragma unroll
        for (int k = 1; k < LE_WAVES; ++k) s += part[k][lane];
        a.var[f * a.C + c] = s / (double)a.D;
    }
}

// one carrier-symbol of order 2 H through the weighted emitter (w = 0 erases, as in soft_demap_nw_kernel); off is even,
// so a carrier's LLRs start on an 8-byte boundary: 8-byte stores, and 16-byte stores declared at that alignment
typedef float llr_quad __attribute__((ext_vector_type(4), aligned(8)));
template <int H>
GF3_DEV void demap_store(cplx e, const double (&lv)[1 << H], double w, float* dst) {
    emit_grid_llr<H, H, true>(e, lv, lv, w, [dst](const float (&out)[2 * H]) {
        if constexpr (H >= 2) *(llr_quad*)dst = llr_quad{out[0], out[1], out[2], out[3]};
        if constexpr (H != 2) *(float2*)(dst + 2 * H - 2) = make_float2(out[2 * H - 2], out[2 * H - 1]);
    });
}

// soft_demap_loaded: soft_demap_nw_kernel's shape -- a workgroup owns Dc consecutive symbols of one packet, prepares the
// per-carrier state in LDS once (W_VAR: the weight, from packet_vbar over all C variances; W_CSI: |Hs| and
// |He| at the carrier's bin; always off[c] and order[c] in one int) and streams its symbols: thread = carrier, one
// 16-byte load per carrier and symbol, a switch on the carrier's order.  Real loadings are long runs of one order, so a
// wave takes one case except where a run ends.
template <int WM>
__global__ __launch_bounds__(LD_THREADS) void soft_demap_loaded_kernel(LoadArgs a) {
    extern __shared__ double ld_lds[];              // [256] partial sums, [C] wa, (W_CSI: [C] wb), then [C] int off * 8 + order
    double* red = ld_lds;
    double* wa = ld_lds + LD_THREADS;
    double* wb = wa + a.C;
    int* oo = (int*)(wa + (WM == W_CSI ? 2 : 1) * (size_t)a.C);
    const int t = threadIdx.x, C = a.C;
    const int64_t f = blockIdx.y;
    if constexpr (WM == W_VAR) {
        const double* v = a.var_in + f * C;
        double s = 0.0;
        for (int c = t; c < C; c += LD_THREADS) s += v[c];
        const PacketNoise pn = packet_vbar(red, s, (double)C);
        for (int c = t; c < C; c += LD_THREADS) wa[c] = noise_weight(v[c], pn);
    }
    if constexpr (WM == W_CSI) {
        for (int c = t; c < C; c += LD_THREADS) {
            const int kk = a.bins[c] - 1;
            const cplx hs = a.Hs[f * a.K + kk], he = a.He[f * a.K + kk];
            wa[c] = hypot(hs.x, hs.y);
            wb[c] = hypot(he.x, he.y);
        }
    }
    for (int c = t; c < C; c += LD_THREADS) oo[c] = a.off[c] * 8 + a.order[c];
    __syncthreads();
    const int l0 = blockIdx.x * a.Dc, l1 = min(l0 + a.Dc, a.D);
    for (int l = l0; l < l1; ++l) {
        const int64_t sym = f * a.D + l;
        const cplx* row = a.eq + sym * C;
        float* out = a.llr + sym * a.Bs;
        for (int c = t; c < C; c += LD_THREADS) {
            const cplx e = row[c];
            const int st = oo[c];
            double w = 1.0;
            if constexpr (WM == W_VAR) w = wa[c];
            if constexpr (WM == W_CSI) w = csi_weight_mag(wa[c], wb[c], l, a.P, a.D);
            float* dst = out + (st >> 3);
            switch (st & 7) {
                case 2: demap_store<1>(e, a.lv.lv1, w, dst); break;
                case 4: demap_store<2>(e, a.lv.lv2, w, dst); break;
                case 6: demap_store<3>(e, a.lv.lv3, w, dst); break;
                default: break;                                         // order 0: no payload, nothing to write
            }
        }
    }
}

struct LoadGuard {                      // run on the device the loading's tables live on
    int prev = -1; bool switched = false;
    explicit LoadGuard(const gf3_loading* q) {
        if (q && hipGetDevice(&prev) == hipSuccess && prev != q->device) switched = hipSetDevice(q->device) == hipSuccess;
    }
    ~LoadGuard() { if (switched) (void)hipSetDevice(prev); }
};

// lv[Gray(i)] = level i: the doubles engine.square_qam_table produces (the division by the scale is a multiplication
// by its reciprocal there, and so here)
template <int N>
void fill_levels(double (&lv)[N]) {
    const double inv = 1.0 / sqrt(2.0 * ((double)N * N - 1.0) / 3.0);
    for (int i = 0; i < N; ++i) lv[i ^ (i >> 1)] = (double)(2 * i - (N - 1)) * inv;
}

LoadArgs load_args(const gf3_ctx* c, const gf3_loading* q) {
    LoadArgs a{};
    a.order = q->d_order; a.off = q->d_off; a.known = q->d_known; a.bins = c->d_bins;
    a.D = c->cfg.D; a.C = c->cfg.C; a.Bs = q->Bs; a.K = c->K; a.P = c->cfg.P;
    a.lv = q->lv;
    return a;
}

}  // namespace

extern "C" int gf3_loading_create(const gf3_ctx* c, const uint8_t* h_order, int32_t C, gf3_loading** out) {
    if (!c || !h_order || !out) return fail(c, GF3_EINVAL, "gf3_loading_create: null argument");
    *out = nullptr;
    if (C != c->cfg.C) return fail(c, GF3_EINVAL, "gf3_loading_create: the table has %d entries, the context %d data carriers", C, c->cfg.C);
    std::vector<int> off(C + 1, 0), bins(C);
    std::vector<cplx> known(C);
    {
        DeviceGuard dg(c);
        HIPCHK(c, hipMemcpy(bins.data(), c->d_bins, (size_t)C * sizeof(int), hipMemcpyDeviceToHost));
    }
    for (int i = 0; i < C; ++i) {
        const int m = h_order[i];
        if (m != 0 && m != 2 && m != 4 && m != 6)
            return fail(c, GF3_EINVAL, "gf3_loading_create: order[%d]=%d (a carrier takes 0, 2, 4 or 6 bits)", i, m);
        off[i + 1] = off[i] + m;
        known[i] = c->known_pts[bins[i] - 1];
    }
    if (off[C] == 0) return fail(c, GF3_EINVAL, "gf3_loading_create: no carrier is loaded");
    gf3_loading* q = new gf3_loading;
    q->ctx = c; q->C = C; q->Bs = off[C]; q->device = c->device;
    fill_levels(q->lv.lv1); fill_levels(q->lv.lv2); fill_levels(q->lv.lv3);
    LoadGuard g(q);
    hipError_t e = hipMalloc((void**)&q->d_order, (size_t)C);
    if (e == hipSuccess) e = hipMalloc((void**)&q->d_off, off.size() * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&q->d_known, known.size() * sizeof(cplx));
    if (e == hipSuccess) e = hipMemcpy(q->d_order, h_order, (size_t)C, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(q->d_off, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(q->d_known, known.data(), known.size() * sizeof(cplx), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        gf3_loading_destroy(q);
        return fail(c, GF3_EHIP, "gf3_loading_create: %s", hipGetErrorString(e));
    }
    *out = q;
    return GF3_OK;
}

extern "C" void gf3_loading_destroy(gf3_loading* q) {
    if (!q) return;
    LoadGuard g(q);
    if (q->d_order) (void)hipFree(q->d_order);
    if (q->d_off) (void)hipFree(q->d_off);
    if (q->d_known) (void)hipFree(q->d_known);
    delete q;
}

extern "C" int gf3_loading_bits(const gf3_loading* q) { return q ? q->Bs : 0; }

extern "C" int gf3_noise_estimate_loaded(gf3_ctx* c, const gf3_loading* q, const void* d_eq, int64_t F, double* d_var, void* stream) {
    DeviceGuard dg(c);
    if (c && q && F == 0) return GF3_OK;
    if (!c || !q || !d_eq || !d_var || F < 0) return fail(c, GF3_EINVAL, "gf3_noise_estimate_loaded: bad argument");
    if (q->ctx != c) return fail(c, GF3_EINVAL, "gf3_noise_estimate_loaded: the loading was made for another context");
    if (const int rc = too_many_packets(c, F, "gf3_noise_estimate_loaded")) return rc;
    LoadArgs a = load_args(c, q);
    a.eq = (const cplx*)d_eq; a.var = d_var;
    const dim3 grid((unsigned)((a.C + 63) / 64), (unsigned)F), block(64 * LE_WAVES);
    hipLaunchKernelGGL(noise_estimate_loaded_kernel, grid, block, 0, (hipStream_t)stream, a);
    HIPCHK(c, hipGetLastError());
    return GF3_OK;
}

extern "C" int gf3_soft_demap_loaded(gf3_ctx* c, const gf3_loading* q, const void* d_eq, const void* d_Hs, const void* d_He,
                                     const double* d_var, int64_t F, float* d_llr, void* stream) {
    DeviceGuard dg(c);
    if (c && q && F == 0) return GF3_OK;
    if (!c || !q || !d_eq || !d_llr || F < 0) return fail(c, GF3_EINVAL, "gf3_soft_demap_loaded: bad argument");
    if (q->ctx != c) return fail(c, GF3_EINVAL, "gf3_soft_demap_loaded: the loading was made for another context");
    if ((d_Hs != nullptr) != (d_He != nullptr)) return fail(c, GF3_EINVAL, "gf3_soft_demap_loaded: d_Hs and d_He go together");
    if (d_var && d_Hs) return fail(c, GF3_EINVAL, "gf3_soft_demap_loaded: give d_var or d_Hs / d_He, not both");
    if (((uintptr_t)d_llr & 7) != 0) return fail(c, GF3_EINVAL, "gf3_soft_demap_loaded: d_llr must be 8-byte aligned");
    if (const int rc = too_many_packets(c, F, "gf3_soft_demap_loaded")) return rc;
    LoadArgs a = load_args(c, q);
    a.eq = (const cplx*)d_eq; a.var_in = d_var; a.Hs = (const cplx*)d_Hs; a.He = (const cplx*)d_He; a.llr = d_llr;
    a.Dc = symbols_per_group(c, F, a.D);
    const dim3 grid((unsigned)((a.D + a.Dc - 1) / a.Dc), (unsigned)F), block(LD_THREADS);
    const size_t lds = (size_t)(LD_THREADS + (d_Hs ? 2 : 1) * (size_t)a.C) * sizeof(double) + (size_t)a.C * sizeof(int);
    hipStream_t st = (hipStream_t)stream;
    if (d_var) hipLaunchKernelGGL(soft_demap_loaded_kernel<W_VAR>, grid, block, lds, st, a);
    else if (d_Hs) hipLaunchKernelGGL(soft_demap_loaded_kernel<W_CSI>, grid, block, lds, st, a);
    else hipLaunchKernelGGL(soft_demap_loaded_kernel<W_UNIT>, grid, block, lds, st, a);
    HIPCHK(c, hipGetLastError());
    return GF3_OK;
}
