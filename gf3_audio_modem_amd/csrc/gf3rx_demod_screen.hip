// libgf3rx -- the screened QPSK demodulation (gf3rx_dscreen.h): demod_screen_kernel, the fp32 form of the one-launch QPSK
// kernel's data symbols, and demod_kernel<.., VAR_LISTED>, the fp64 kernel on the packets the screen listed.  f64 storage is
// not screened (fp32 does not hold it exactly), so neither kernel is built for it.
#include "gf3rx_demod.h"

template <int NC, int DT> constexpr auto demod_screen_kernel = demod_kernel<NC, DT, false, MODE_QPSK, STAGE_ALL, VAR_SCREEN>;
template <int NC, int DT> constexpr auto demod_listed_kernel = demod_kernel<NC, DT, false, MODE_QPSK, STAGE_ALL, VAR_LISTED>;

#ifdef GF3_DEV_BUILD
#define DISPATCH_DT32(DTv, CALL) { constexpr int DTC = DT_F32; CALL; }
#else
#define DISPATCH_DT32(DTv, CALL)                                          \
    switch (DTv) {                                                        \
        case DT_F32: { constexpr int DTC = DT_F32; CALL; break; }         \
        case DT_I16: { constexpr int DTC = DT_I16; CALL; break; }         \
        default:     { constexpr int DTC = DT_U8;  CALL; break; }         \
    }
#endif
#ifdef GF3_DEV_BUILD
#define DISPATCH_NC32(NCv, DTv, CALL) { constexpr int NCC = 2048; DISPATCH_DT32(DTv, CALL); }
#else
#define DISPATCH_NC32(NCv, DTv, CALL)                                     \
    switch (NCv) {                                                        \
        case 512:  { constexpr int NCC = 512;  DISPATCH_DT32(DTv, CALL); break; }   \
        case 1024: { constexpr int NCC = 1024; DISPATCH_DT32(DTv, CALL); break; }   \
        case 2048: { constexpr int NCC = 2048; DISPATCH_DT32(DTv, CALL); break; }   \
        default:   { constexpr int NCC = 4096; DISPATCH_DT32(DTv, CALL); break; }   \
    }
#endif

// the reference QPSK table (sign decisions) on a storage that converts to fp32 exactly
bool demod_screen_applies(const gf3_ctx* c) {
    return c->qpsk_q > 0.0 && (c->cfg.in_dtype == DT_F32 || c->cfg.in_dtype == DT_I16 || c->cfg.in_dtype == DT_U8);
}
// Same LDS layout as the fp64 kernel (the pilot stage is the fp64 kernel's); the fp32 transforms use the first half of
// the FFT buffer.
hipError_t launch_demod_screen(const gf3_ctx* c, const DemodArgs& a, int64_t F, hipStream_t st) {
    hipError_t e = hipSuccess;
    DISPATCH_NC32(c->NC, a.dt, e = launch((demod_screen_kernel<NCC, DTC>), F, NCC / 8, demod_lds_bytes(c, true), st, a));
    return e;
}
// grid = the list's capacity; workgroups past its length return at once
hipError_t launch_demod_listed(const gf3_ctx* c, const DemodArgs& a, int64_t F, hipStream_t st) {
    hipError_t e = hipSuccess;
    DISPATCH_NC32(c->NC, a.dt, e = launch((demod_listed_kernel<NCC, DTC>), F, NCC / 8, demod_lds_bytes(c, true), st, a));
    return e;
}

// tests (gf3_debug_demod_screen): the list as a verdict per packet
__global__ void demod_verdict_kernel(const int* dwork, int* cls, int64_t F) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < F && i < dwork[0]) cls[dwork[16 + i]] = 1;
}
hipError_t launch_demod_verdicts(const int* dwork, int* cls, int64_t F, hipStream_t st) {
    hipError_t e = hipMemsetAsync(cls, 0, (size_t)F * sizeof(int), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(demod_verdict_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, st, dwork, cls, F);
    return hipGetLastError();
}

// tests (gf3_debug_rfft_sp_batch): the fp32 transform alone, in the very instantiation the screen runs -- rfft_regs<NC, PP,
// TWICE, float2> with the context's rounded twiddles -- one symbol per workgroup, the whole half spectrum X[0 .. NC] out
// (the slots hold 2 X: halved on the way out, exactly)
struct Rfft32Args { RfftArgs r; const cf* tw32; cf* out32; };
template <int NC, int DT>
__global__ __launch_bounds__(NC / 8, 2) void rfft32_kernel(Rfft32Args ra) {
    extern __shared__ double2 smem[];
    const RfftArgs& a = ra.r;
    const cf* tw32 = ra.tw32;
    cf* out32 = ra.out32;
    constexpr int T = NC / 8;
    const int tid = threadIdx.x;
    const int64_t sym = blockIdx.x;
    const int64_t off = a.off[sym];
    cf* out = out32 + sym * (int64_t)(NC + 1);
    FftTw<NC, cf> ft;
    ft.init(tid, tw32);
    const cf wb = tw32[NC + tid];
    cf v[8], z0;
    const bool ok = off >= 0 && off + 2 * NC <= a.n_in;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        RawPair<DT> raw;
        if (ok) raw.load(a.in, off + 2 * (int64_t)(tid + r * T)); else raw.zero();
        v[r] = make_float2((float)raw.v.a, (float)raw.v.b);
    }
    rfft_regs<NC, DemodOcc<NC, MODE_QPSK>::PP, true>(v, (cf*)smem, ft, wb, tid, z0, 0);
#pragma unroll
    for (int s2 = 0; s2 < 8; ++s2)
        if (Spec<NC>::live(tid, s2)) out[Spec<NC>::bin(tid, s2)] = make_float2(0.5f * v[s2].x, 0.5f * v[s2].y);
    if (tid == 0) {
        out[0] = make_float2(z0.x + z0.y, 0.0f);
        out[NC] = make_float2(z0.x - z0.y, 0.0f);
    }
}
extern "C" int gf3_debug_rfft_sp_batch(gf3_ctx* c, const void* d_in, int64_t n_in, const int64_t* d_offsets, int64_t n_sym,
                                      void* d_out_c64, void* stream) {
    DeviceGuard dg(c);
    if (c && n_sym == 0) return GF3_OK;
    if (!c || !d_in || !d_offsets || !d_out_c64 || n_sym < 0) return fail(c, GF3_EINVAL, "gf3_debug_rfft_sp_batch: bad argument");
    if (c->cfg.in_dtype == DT_F64) return fail(c, GF3_EINVAL, "gf3_debug_rfft_sp_batch: f64 samples are not transformed in fp32");
    Rfft32Args a{RfftArgs{FftTables{c->d_tw, c->d_twn}, d_in, n_in, d_offsets, c->cfg.in_dtype, nullptr}, c->d_tw32, (cf*)d_out_c64};
    const size_t lds = (size_t)(demod_pp_size(c->NC) ? 2 * c->NC : c->NC + c->NC / 8) * sizeof(cf);
    hipError_t e = hipSuccess;
    DISPATCH_NC32(c->NC, a.r.dt, e = launch((rfft32_kernel<NCC, DTC>), n_sym, NCC / 8, lds, (hipStream_t)stream, a));
    HIPCHK(c, e);
    return GF3_OK;
}

// tests (gf3_debug_rfft_sp_pair_batch): the transform the screen runs on its data symbols -- rfft_regs<NC, PP, TWICE, cf2>,
// two symbols as the halves of one point -- workgroup w on symbols 2w and 2w + 1 (an odd n_sym: the last second half is
// absent, zeros in and nothing out); output as rfft32_kernel's
struct Rfft32PairArgs { Rfft32Args r; int64_t n_sym; };
template <int NC, int DT>
__global__ __launch_bounds__(NC / 8, 2) void rfft32_pair_kernel(Rfft32PairArgs pa) {
    extern __shared__ double2 smem[];
    const RfftArgs& a = pa.r.r;
    const cf* tw32 = pa.r.tw32;
    constexpr int T = NC / 8;
    const int tid = threadIdx.x;
    const int64_t sa = 2 * (int64_t)blockIdx.x, sb = sa + 1;
    const bool hb = sb < pa.n_sym;
    const int64_t offa = a.off[sa], offb = hb ? a.off[sb] : -1;
    FftTw<NC, cf> ft;
    ft.init(tid, tw32);
    const cf wb = tw32[NC + tid];
    cf2 v[8], z0;
    const bool oka = offa >= 0 && offa + 2 * NC <= a.n_in, okb = hb && offb >= 0 && offb + 2 * NC <= a.n_in;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        RawPair<DT> ra, rb;
        if (oka) ra.load(a.in, offa + 2 * (int64_t)(tid + r * T)); else ra.zero();
        if (okb) rb.load(a.in, offb + 2 * (int64_t)(tid + r * T)); else rb.zero();
        v[r] = pair_of(make_float2((float)ra.v.a, (float)ra.v.b), make_float2((float)rb.v.a, (float)rb.v.b));
    }
    rfft_regs<NC, DemodOcc<NC, MODE_QPSK>::PP, true>(v, (cf2*)smem, ft, wb, tid, z0, 0);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (h == 1 && !hb) break;
        cf* out = pa.r.out32 + (sa + h) * (int64_t)(NC + 1);
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2) {
            const cf x = h ? half_b(v[s2]) : half_a(v[s2]);
            if (Spec<NC>::live(tid, s2)) out[Spec<NC>::bin(tid, s2)] = make_float2(0.5f * x.x, 0.5f * x.y);
        }
        if (tid == 0) {
            const cf z = h ? half_b(z0) : half_a(z0);
            out[0] = make_float2(z.x + z.y, 0.0f);
            out[NC] = make_float2(z.x - z.y, 0.0f);
        }
    }
}
extern "C" int gf3_debug_rfft_sp_pair_batch(gf3_ctx* c, const void* d_in, int64_t n_in, const int64_t* d_offsets, int64_t n_sym,
                                           void* d_out_c64, void* stream) {
    DeviceGuard dg(c);
    if (c && n_sym == 0) return GF3_OK;
    if (!c || !d_in || !d_offsets || !d_out_c64 || n_sym < 0) return fail(c, GF3_EINVAL, "gf3_debug_rfft_sp_pair_batch: bad argument");
    if (c->cfg.in_dtype == DT_F64) return fail(c, GF3_EINVAL, "gf3_debug_rfft_sp_pair_batch: f64 samples are not transformed in fp32");
    Rfft32PairArgs a{Rfft32Args{RfftArgs{FftTables{c->d_tw, c->d_twn}, d_in, n_in, d_offsets, c->cfg.in_dtype, nullptr}, c->d_tw32, (cf*)d_out_c64}, n_sym};
    const size_t lds = (size_t)(demod_pp_size(c->NC) ? 2 * c->NC : c->NC + c->NC / 8) * sizeof(cf2);
    hipError_t e = hipSuccess;
    DISPATCH_NC32(c->NC, a.r.r.dt, e = launch((rfft32_pair_kernel<NCC, DTC>), (n_sym + 1) / 2, NCC / 8, lds, (hipStream_t)stream, a));
    HIPCHK(c, e);
    return GF3_OK;
}
