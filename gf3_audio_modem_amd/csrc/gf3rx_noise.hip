// libgf3rx -- decision-directed per-carrier noise estimate and the noise-weighted soft demapper (gf3_noise_estimate,
// gf3_soft_demap_nw), their carrier x symbol forms for impulse noise (gf3_noise_estimate_cs, gf3_soft_demap_nw_cs) and
// the packet interleaver (gf3_interleave).  See DESIGN.md §12.
//
//   v[f, c]   = (1/D) sum_l |eq[f, l, c] - s|^2, s the point the hard decision picks (in-order scan, strict <)
//   vbar[f]   = mean_c v[f, c]
//   w[f, c]   = 0 where v is not finite; 1 for the whole packet where vbar is 0 or not finite; else 1 / max(v, 1e-6 vbar)
//   LLR       = maxlog(eq; sigma^2 = 1) * w   (float32; +0 where w = 0: an erasure, whatever the symbol held)
// The decided point's distance (nearest_d2), the tree behind vbar (packet_vbar), the weight rule (noise_weight) and the
// weighted emitter (emit_llr) are gf3rx_demap.h's: these kernels hold the work split and the order of the sums.
//
// carrier x symbol form (clicks, dropouts: a few whole symbols are garbage):
//   vs[f, l]  = (1/C) sum_c |eq[f, l, c] - s|^2
//   w[f,l,c]  = 0 where v[f, c] or vs[f, l] is not finite; else 1 for the whole packet where vbar is 0 or not finite;
//               else 1 / max(v vs / vbar, 1e-6 vbar)
// packet interleaver: coded bit i of a packet's nbp = D C mu travels at position pi(i) = (i s) mod nbp, s the smallest
// integer >= C mu + 1 coprime to nbp.
//
// Every sum runs in a fixed order (no floating-point atomics): two runs give identical bits.
#include "gf3rx_demap.h"

namespace {

constexpr int NE_WAVES = 8;             // waves of a noise_estimate workgroup: the D symbols are dealt out to them
constexpr int NW_THREADS = VBAR_THREADS;

struct NoiseArgs {
    const cplx* eq; double* var; const double* var_in; float* llr;
    int64_t F; int D, C, Dc;            // Dc: symbols per soft_demap_nw workgroup
    DemapTab t;
};

// noise_estimate: a workgroup owns 64 consecutive carriers of one packet (lane = carrier: a wave reads 1 KB
// contiguously per symbol); wave w adds up the symbols l = w, w + 8, w + 16, ... in ascending order, the 8 partial sums
// meet in LDS and wave 0 adds them in the order w = 0 .. 7, then divides by D.
template <int HI>
__global__ __launch_bounds__(64 * NE_WAVES) void noise_estimate_kernel(NoiseArgs a) {
    __shared__ double part[NE_WAVES][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int64_t f = blockIdx.y;
    const Levels<HI> lv(a.t);
    double acc = 0.0;
    if (c < a.C) {
        const cplx* p = a.eq + (f * a.D) * (int64_t)a.C + c;
        for (int l = w; l < a.D; l += NE_WAVES) acc += nearest_d2<HI>(p[(int64_t)l * a.C], lv, a.t);
    }
    part[w][lane] = acc;
    __syncthreads();
    if (w == 0 && c < a.C) {
        double s = part[0][lane];
#pragma unroll
        for (int k = 1; k < NE_WAVES; ++k) s += part[k][lane];
        a.var[f * a.C + c] = s / (double)a.D;
    }
}

// soft_demap_nw: a workgroup owns Dc consecutive symbols of one packet.  It first turns the packet's variances into
// weights in LDS (thread t adds v[t], v[t + 256], ... in ascending order, packet_vbar's tree over the 256 partial sums
// gives vbar: the same number in every workgroup of the packet), then streams its symbols: thread = carrier, 16 bytes
// read and 4 mu bytes written per symbol, the weight from LDS.
template <int HI>
__global__ __launch_bounds__(NW_THREADS) void soft_demap_nw_kernel(NoiseArgs a) {
    extern __shared__ double nw_lds[];              // [256] partial sums, then [C] weights
    double* red = nw_lds;
    double* wgt = nw_lds + NW_THREADS;
    const int t = threadIdx.x, C = a.C;
    const int64_t f = blockIdx.y;
    const double* v = a.var_in + f * C;
    double s = 0.0;
    for (int c = t; c < C; c += NW_THREADS) s += v[c];
    const PacketNoise pn = packet_vbar(red, s, (double)C);
    for (int c = t; c < C; c += NW_THREADS) wgt[c] = noise_weight(v[c], pn);
    __syncthreads();
    const Levels<HI> lv(a.t);
    const int l0 = blockIdx.x * a.Dc, l1 = min(l0 + a.Dc, a.D);
    for (int l = l0; l < l1; ++l) {
        const int64_t row = (f * a.D + l) * (int64_t)C;
        for (int c = t; c < C; c += NW_THREADS) {
            const cplx e = a.eq[row + c];
            const double w = wgt[c];
            // (the store captures by value: by reference the address arithmetic of the row comes out longer)
            emit_llr<HI, true>(e, lv, a.t, w, [llr = a.llr, i = row + c, mu = a.t.mu](const auto& out) { store_llr_any(llr, i, mu, out); });
        }
    }
}

// ---- carrier x symbol estimate ---------------------------------------------------------------------------------
// noise_estimate_cs: ONE pass over eq gives both variances, so a workgroup owns a whole packet (there is no other way
// to finish both sums without a second pass or memory shared between workgroups).  16 waves = 2 carrier halves g x 8
// symbol phases w; lane = carrier as in noise_estimate_kernel: half g holds the 64-carrier columns g ncg .. g ncg + ncg
// - 1, wave (g, w) walks the symbols l = w, w + 8, ... ascending and reads its ncg columns of each (ncg loads of 1 KB
// in flight).  Carrier sums: one register per column, added in that symbol order, the 8 phases meet in LDS and are
// added in the order of w, then / D -- the order of noise_estimate_kernel, so v is the same bits.  Symbol sums: a lane
// adds its columns' terms in ascending column order, an xor butterfly (32, 16, .. 1) adds the 64 lanes, the two
// halves meet in LDS and are added g = 0 then 1, then / C.
constexpr int CS_THREADS = 1024;
constexpr int CS_MAX_NCG = 16;          // columns per half at most: C <= 2 * 16 * 64

struct NoiseCsArgs {
    const cplx* eq; double* var_c; double* var_s;
    int D, C, ncg;
    DemapTab t;
};

template <int HI, int NCG>
__global__ __launch_bounds__(CS_THREADS) void noise_estimate_cs_kernel(NoiseCsArgs a) {
    extern __shared__ double cs_lds[];              // [8][C] carrier partial sums, [D][2] symbol partial sums
    double* part = cs_lds;
    double* spart = cs_lds + 8 * (size_t)a.C;
    const int lane = threadIdx.x & 63, w = (threadIdx.x >> 6) & 7, g = threadIdx.x >> 9;
    const int64_t f = blockIdx.x;
    const Levels<HI> lv(a.t);
    const cplx* p = a.eq + (f * a.D) * (int64_t)a.C;
    double acc[NCG];
#pragma unroll
    for (int k = 0; k < NCG; ++k) acc[k] = 0.0;
    // the lane's carrier in column k of its half is c0 + 64 k: taken while it is below cend (the load of any other slot
    // takes carrier 0 and its term is dropped)
    const int c0 = g * a.ncg * 64 + lane, cend = min(a.C, (g + 1) * a.ncg * 64);
    for (int l = w; l < a.D; l += 8) {
        const cplx* row = p + (int64_t)l * a.C;
        double srow = 0.0;
        constexpr int NB = NCG > 8 ? 4 : NCG;         // loads in flight per batch (more would spill: 128 VGPRs at 16 waves)
#pragma unroll
        for (int k0 = 0; k0 < NCG; k0 += NB) {
            cplx e[NB];
#pragma unroll
            for (int k = 0; k < NB; ++k) e[k] = row[c0 + 64 * (k0 + k) < cend ? c0 + 64 * (k0 + k) : 0];
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                double d2 = nearest_d2<HI>(e[k], lv, a.t);
                d2 = c0 + 64 * (k0 + k) < cend ? d2 : 0.0;
                acc[k0 + k] += d2;
                srow += d2;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) srow += __shfl_xor(srow, off);
        if (lane == 0) spart[2 * l + g] = srow;
    }
#pragma unroll
    for (int k = 0; k < NCG; ++k)
        if (c0 + 64 * k < cend) part[(size_t)w * a.C + c0 + 64 * k] = acc[k];
    __syncthreads();
    for (int c = threadIdx.x; c < a.C; c += CS_THREADS) {
        double s = part[c];
#pragma unroll
        for (int k = 1; k < 8; ++k) s += part[(size_t)k * a.C + c];
        a.var_c[f * a.C + c] = s / (double)a.D;
    }
    for (int l = threadIdx.x; l < a.D; l += CS_THREADS)
        a.var_s[f * a.D + l] = (spart[2 * l] + spart[2 * l + 1]) / (double)a.C;
}

// ---- packet interleaver ----------------------------------------------------------------------------------------
// pi(i) = (i s) mod nbp and its inverse pi^-1(p) = (p s^-1) mod nbp.  Kernels never divide per element: a thread takes
// one 64-bit product modulo nbp for its first element and walks on by precomputed steps with a conditional subtract
// (nbp < 2^31, so the sums fit 32 bits).
struct Perm { uint32_t nbp, s, sinv; };              // s, sinv already reduced modulo nbp

GF3_DEV uint32_t addmod(uint32_t x, uint32_t step, uint32_t n) { x += step; return x >= n ? x - n : x; }

bool perm_of(const gf3_ctx* c, Perm& p) {
    const int64_t B = (int64_t)c->cfg.C * c->cfg.mu, nbp = B * c->cfg.D;
    if (nbp < 1 || nbp >= (int64_t)1 << 31) return false;
    auto gcd = [](int64_t x, int64_t y) { while (y) { const int64_t r = x % y; x = y; y = r; } return x; };
    int64_t s = B + 1;
    while (gcd(s, nbp) != 1) ++s;
    // extended Euclid: s x == 1 (mod nbp)
    int64_t r0 = nbp, r1 = s % nbp, x0 = 0, x1 = 1;
    while (r1) { const int64_t q = r0 / r1, r = r0 - q * r1, x = x0 - q * x1; r0 = r1; r1 = r; x0 = x1; x1 = x; }
    p.nbp = (uint32_t)nbp; p.s = (uint32_t)(s % nbp); p.sinv = (uint32_t)(((x0 % nbp) + nbp) % nbp);
    return true;
}

constexpr int IL_THREADS = 256, IL_PER = 8;          // elements per thread, 256 apart

// out[f, j] = in[f, (j m) mod nbp]: m = s undoes the interleaver, m = s^-1 applies it.  Stores are contiguous, loads strided.
template <typename T>
__global__ __launch_bounds__(IL_THREADS) void interleave_kernel(const T* in, T* out, uint32_t nbp, uint32_t m, uint32_t step) {
    const int64_t base = (int64_t)blockIdx.y * nbp;
    const uint64_t j0 = (uint64_t)blockIdx.x * (IL_THREADS * IL_PER) + threadIdx.x;
    if (j0 >= nbp) return;
    uint32_t idx = (uint32_t)((j0 * m) % nbp);
#pragma unroll
    for (int u = 0; u < IL_PER; ++u) {
        const uint64_t j = j0 + (uint64_t)u * IL_THREADS;
        if (j < nbp) out[base + j] = in[base + idx];
        idx = addmod(idx, step, nbp);
    }
}

// ---- carrier x symbol demapper ---------------------------------------------------------------------------------
// soft_demap_nw_cs: soft_demap_nw_kernel with the weight 1 / max(v vs / vbar, floor) formed per symbol from two factors
// kept in LDS: ic[c] = vbar / v[c] and is[l] = 1 / vs[l] (0 marks an erasure, 1 a flat packet), w = ic is capped at
// 1 / floor -- one multiply and a compare per symbol, no division in the stream.  This is noise_weight(x, pn) of
// gf3rx_demap.h for x = v vs / vbar, factored (equal in exact arithmetic; the roundings are this kernel's own and its
// restatement's): 1 / max(x, floor) = min(1 / x, 1 / floor) for x > 0, and 1 / x = (vbar / v) (1 / vs); a variance that
// is not finite gives a zero factor and so the weight 0; in a flat packet both factors and the cap are 1.  vbar comes
// from packet_vbar as in soft_demap_nw_kernel: the same bits there, here, and in every workgroup of the packet.
// DEINT: each LLR goes to its coded position pi^-1(p) of the packet instead of its transmitted position p.
struct NwCsArgs {
    const cplx* eq; const double* var_c; const double* var_s; float* llr;
    int D, C, Dc;
    uint32_t nbp, sinv, step_c, step_l;             // DEINT: (256 mu s^-1) mod nbp, (C mu s^-1) mod nbp
    DemapTab t;
};

template <int HI, bool DEINT>
__global__ __launch_bounds__(NW_THREADS) void soft_demap_nw_cs_kernel(NwCsArgs a) {
    extern __shared__ double nw_lds[];              // [256] partial sums, [C] carrier factors, [Dc] symbol factors
    double* red = nw_lds;
    double* ic = nw_lds + NW_THREADS;
    double* is = ic + a.C;
    const int t = threadIdx.x, C = a.C;
    const int64_t f = blockIdx.y;
    const double* v = a.var_c + f * C;
    const int l0 = blockIdx.x * a.Dc, l1 = min(l0 + a.Dc, a.D);
    double s = 0.0;
    for (int c = t; c < C; c += NW_THREADS) s += v[c];
    const PacketNoise pn = packet_vbar(red, s, (double)C);
    const double wmax = pn.flat ? 1.0 : 1.0 / pn.floor_v;
    for (int c = t; c < C; c += NW_THREADS) {
        const double x = v[c];
        ic[c] = !(fabs(x) < INFINITY) ? 0.0 : pn.flat ? 1.0 : pn.vbar / x;
    }
    for (int l = l0 + t; l < l1; l += NW_THREADS) {
        const double x = a.var_s[f * a.D + l];
        is[l - l0] = !(fabs(x) < INFINITY) ? 0.0 : pn.flat ? 1.0 : 1.0 / x;
    }
    __syncthreads();
    const Levels<HI> lv(a.t);
    const int mu = a.t.mu;
    float* pk = a.llr + f * (int64_t)a.nbp;         // DEINT: the packet's LLRs
    uint32_t irow = 0;                              // DEINT: coded position of bit 0 of (l, carrier t)
    if constexpr (DEINT) irow = (uint32_t)(((uint64_t)((int64_t)l0 * C + t) * (uint64_t)mu % a.nbp) * a.sinv % a.nbp);
    for (int l = l0; l < l1; ++l) {
        const int64_t row = (f * a.D + l) * (int64_t)C;
        const double sl = is[l - l0];
        uint32_t i0 = irow;
        for (int c = t; c < C; c += NW_THREADS) {
            const cplx e = a.eq[row + c];
            const double cf = ic[c], pr = cf * sl;
            // a zero factor: erasure; pr not below the cap (v vs / vbar under the floor, Inf from a zero variance) or not
            // positive: the cap
            const double w = (cf == 0.0 || sl == 0.0) ? 0.0 : (pr > 0.0 && pr < wmax) ? pr : wmax;
            // (the stores capture by value: by reference the address arithmetic of the row comes out longer)
            if constexpr (DEINT)                                    // bit b goes to coded position i0 + b s^-1 (mod nbp)
                emit_llr<HI, true>(e, lv, a.t, w, [pk, i0, mu, sinv = a.sinv, nbp = a.nbp](const auto& out) {
                    constexpr int NB = sizeof(out) / sizeof(float);    // 2 HI on a grid (= mu), 8 of which mu are valid for any table
                    uint32_t i = i0;
#pragma unroll
                    for (int b = 0; b < NB; ++b)
                        if (NB < 8 || b < mu) { pk[i] = out[b]; i = addmod(i, sinv, nbp); }
                });
            else
                emit_llr<HI, true>(e, lv, a.t, w, [llr = a.llr, i = row + c, mu](const auto& out) { store_llr_any(llr, i, mu, out); });
            if constexpr (DEINT) i0 = addmod(i0, a.step_c, a.nbp);
        }
        if constexpr (DEINT) irow = addmod(irow, a.step_l, a.nbp);
    }
}

}  // namespace

extern "C" int gf3_noise_estimate(gf3_ctx* c, const void* d_eq, int64_t F, double* d_var, void* stream) {
    DeviceGuard dg(c);
    if (c && F == 0) return GF3_OK;
    if (!c || !d_eq || !d_var || F < 0) return fail(c, GF3_EINVAL, "gf3_noise_estimate: bad argument");
    if (const int rc = too_many_packets(c, F, "gf3_noise_estimate")) return rc;
    NoiseArgs a{(const cplx*)d_eq, d_var, nullptr, nullptr, F, c->cfg.D, c->cfg.C, 0, demap_tab(c)};
    const dim3 grid((unsigned)((a.C + 63) / 64), (unsigned)F), block(64 * NE_WAVES);
    hipStream_t st = (hipStream_t)stream;
    with_grid_bits(c, [&](auto hi) { hipLaunchKernelGGL(noise_estimate_kernel<decltype(hi)::value>, grid, block, 0, st, a); });
    HIPCHK(c, hipGetLastError());
    return GF3_OK;
}

extern "C" int gf3_soft_demap_nw(gf3_ctx* c, const void* d_eq, const double* d_var, int64_t F, float* d_llr, void* stream) {
    DeviceGuard dg(c);
    if (c && F == 0) return GF3_OK;
    if (!c || !d_eq || !d_var || !d_llr || F < 0) return fail(c, GF3_EINVAL, "gf3_soft_demap_nw: bad argument");
    if (const int rc = too_many_packets(c, F, "gf3_soft_demap_nw")) return rc;
    NoiseArgs a{(const cplx*)d_eq, nullptr, d_var, d_llr, F, c->cfg.D, c->cfg.C, 0, demap_tab(c)};
    a.Dc = symbols_per_group(c, F, a.D);
    const dim3 grid((unsigned)((a.D + a.Dc - 1) / a.Dc), (unsigned)F), block(NW_THREADS);
    const size_t lds = (size_t)(NW_THREADS + a.C) * sizeof(double);
    hipStream_t st = (hipStream_t)stream;
    with_grid_bits(c, [&](auto hi) { hipLaunchKernelGGL(soft_demap_nw_kernel<decltype(hi)::value>, grid, block, lds, st, a); });
    HIPCHK(c, hipGetLastError());
    return GF3_OK;
}

// (NCG in steps of 4: a slot beyond the half's columns costs a repeated load of carrier 0)
hipError_t launch_noise_cs(const gf3_ctx* c, const NoiseCsArgs& a, int64_t F, size_t lds, hipStream_t st) {
    return with_grid_bits(c, [&](auto hi) {
        constexpr int HI = decltype(hi)::value;
        if (a.ncg <= 4) return launch(noise_estimate_cs_kernel<HI, 4>, F, CS_THREADS, lds, st, a);
        if (a.ncg <= 8) return launch(noise_estimate_cs_kernel<HI, 8>, F, CS_THREADS, lds, st, a);
        if (a.ncg <= 12) return launch(noise_estimate_cs_kernel<HI, 12>, F, CS_THREADS, lds, st, a);
        return launch(noise_estimate_cs_kernel<HI, 16>, F, CS_THREADS, lds, st, a);
    });
}

extern "C" int gf3_noise_estimate_cs(gf3_ctx* c, const void* d_eq, int64_t F, double* d_var_c, double* d_var_s, void* stream) {
    DeviceGuard dg(c);
    if (c && F == 0) return GF3_OK;
    if (!c || !d_eq || !d_var_c || !d_var_s || F < 0) return fail(c, GF3_EINVAL, "gf3_noise_estimate_cs: bad argument");
    if (const int rc = too_many_packets(c, F, "gf3_noise_estimate_cs")) return rc;
    NoiseCsArgs a{(const cplx*)d_eq, d_var_c, d_var_s, c->cfg.D, c->cfg.C, 0, demap_tab(c)};
    a.ncg = ((a.C + 63) / 64 + 1) / 2;
    const size_t lds = (8 * (size_t)a.C + 2 * (size_t)a.D) * sizeof(double);
    if (a.ncg > CS_MAX_NCG || lds > 160 * 1024)
        return fail(c, GF3_ERANGE, "gf3_noise_estimate_cs: a packet's partial sums (64 C + 16 D bytes) must fit 160 KB of LDS, C <= 2048");
    HIPCHK(c, launch_noise_cs(c, a, F, lds, (hipStream_t)stream));
    return GF3_OK;
}

extern "C" int gf3_soft_demap_nw_cs(gf3_ctx* c, const void* d_eq, const double* d_var_c, const double* d_var_s, int64_t F,
                                    int32_t deinterleave, float* d_llr, void* stream) {
    DeviceGuard dg(c);
    if (c && F == 0) return GF3_OK;
    if (!c || !d_eq || !d_var_c || !d_var_s || !d_llr || F < 0 || (deinterleave != 0 && deinterleave != 1))
        return fail(c, GF3_EINVAL, "gf3_soft_demap_nw_cs: bad argument");
    if (const int rc = too_many_packets(c, F, "gf3_soft_demap_nw_cs")) return rc;
    Perm pm;
    if (!perm_of(c, pm)) return fail(c, GF3_ERANGE, "gf3_soft_demap_nw_cs: D C mu must be below 2^31");
    NwCsArgs a{(const cplx*)d_eq, d_var_c, d_var_s, d_llr, c->cfg.D, c->cfg.C, 0, pm.nbp, pm.sinv, 0, 0, demap_tab(c)};
    a.step_c = (uint32_t)((uint64_t)NW_THREADS * c->cfg.mu % pm.nbp * pm.sinv % pm.nbp);
    a.step_l = (uint32_t)((uint64_t)a.C * c->cfg.mu % pm.nbp * pm.sinv % pm.nbp);
    a.Dc = symbols_per_group(c, F, a.D);
    const dim3 grid((unsigned)((a.D + a.Dc - 1) / a.Dc), (unsigned)F), block(NW_THREADS);
    const size_t lds = (size_t)(NW_THREADS + a.C + a.Dc) * sizeof(double);
    hipStream_t st = (hipStream_t)stream;
    with_grid_bits(c, [&](auto hi) {
        constexpr int HI = decltype(hi)::value;
        if (deinterleave) hipLaunchKernelGGL((soft_demap_nw_cs_kernel<HI, true>), grid, block, lds, st, a);
        else hipLaunchKernelGGL((soft_demap_nw_cs_kernel<HI, false>), grid, block, lds, st, a);
    });
    HIPCHK(c, hipGetLastError());
    return GF3_OK;
}

extern "C" int gf3_interleave(gf3_ctx* c, const void* d_in, void* d_out, int64_t F, int32_t elem_bytes, int32_t inverse, void* stream) {
    DeviceGuard dg(c);
    if (c && F == 0) return GF3_OK;
    if (!c || !d_in || !d_out || d_in == d_out || F < 0 || (elem_bytes != 1 && elem_bytes != 4) || (inverse != 0 && inverse != 1))
        return fail(c, GF3_EINVAL, "gf3_interleave: bad argument (elem_bytes 1 or 4, inverse 0 or 1, out of place)");
    if (const int rc = too_many_packets(c, F, "gf3_interleave")) return rc;
    Perm pm;
    if (!perm_of(c, pm)) return fail(c, GF3_ERANGE, "gf3_interleave: D C mu must be below 2^31");
    const uint32_t m = inverse ? pm.s : pm.sinv;
    const uint32_t step = (uint32_t)((uint64_t)IL_THREADS % pm.nbp * m % pm.nbp);
    const dim3 grid((pm.nbp + IL_THREADS * IL_PER - 1) / (IL_THREADS * IL_PER), (unsigned)F), block(IL_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (elem_bytes == 4) hipLaunchKernelGGL(interleave_kernel<uint32_t>, grid, block, 0, st, (const uint32_t*)d_in, (uint32_t*)d_out, pm.nbp, m, step);
    else hipLaunchKernelGGL(interleave_kernel<uint8_t>, grid, block, 0, st, (const uint8_t*)d_in, (uint8_t*)d_out, pm.nbp, m, step);
    HIPCHK(c, hipGetLastError());
    return GF3_OK;
}
