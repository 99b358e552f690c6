// libgf3rx -- the screened QPSK demodulation (gf3rx_dscreen.h): demod_screen_kernel, the one-launch QPSK kernel with its data
// symbols in fp32 under a bound, and demod_listed_kernel, the fp64 kernel on the packets the screen listed.  f64 storage is
// not screened (fp32 does not hold it exactly), so neither kernel is built for it.
#include "gf3rx_demod.h"

// The data symbols of demod_screen_kernel; everything before them is demod_kernel's (gf3rx_demod.h), whose lean LDS layout
// this keeps: the fp32 transforms use the whole FFT buffer as cf2 points.  In: the first sample offset, the output row, the
// fp64 start-up's g_0 and gstep, and `unsafe` (a non-finite end-pilot estimate); nxt is the fetch buffer, free on entry.
// The data symbols go through the transform two at a time, as the halves of cf2 points (gf3rx_device.h): symbols (l, l + 1)
// from nxt and nxb -> fp32 spectrum slots in vp, the next pair prefetched (its first symbol under the transform, its second
// under the decisions).  An odd last symbol runs the same code with an absent second half: no loads, zeros, no decisions.
// Each symbol's l1 norm is summed while its samples are converted; the per-wave sums go to l1s[parity][half][wave] ahead
// of the transform's barriers and are read back after them (two parities: pair i + 1 writes before every wave has read
// pair i's; i + 2 writes only after the barriers of transform i + 1).
template <int NC, int DT>
GF3_DEV void demod_screen_data(const DemodArgs& a, const DemodLdsPtr& m, int64_t f, int64_t off, int tid, uint8_t* row, bool unsafe,
                               RawPair<DT> (&nxt)[8], const cplx (&g0)[8], const cplx (&gstep)[8]) {
    constexpr int T = NC / 8;
    const int P = a.P, D = a.D, C = a.C;
    uint8_t* labs = m.labs;
    // scratch, now that the slope fit is done with it: the packet's "listed" flag in double 8, the l1 sums in doubles [16, 32)
    int* unsafe_flag = (int*)(m.scratch + 8);
    float* l1s = (float*)(m.scratch + 16);                                // [2][2][8]
    if (tid == 0) *unsafe_flag = 0;                                        // (read after the last transform's barriers)
    FftTw<NC, cf> ft32;
    ft32.init(tid, a.tw32);
    cf wb32 = a.tw32[NC + tid];
    // g_0 and gstep rounded once; the recurrence runs in fp32 from here on (gf3rx_dscreen.h, "The rotation") and
    // the 64 registers of fp64 state are free inside the data loop
    cf g32[8], gs32[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        g32[s] = make_float2((float)g0[s].x, (float)g0[s].y);
        gs32[s] = make_float2((float)gstep[s].x, (float)gstep[s].y);
    }
    // data position of every slot, resolved once as in the fp64 sign mode, two to a register (C < 65535; 0xffff: no data carrier)
    uint32_t psp[4];
#pragma unroll
    for (int s = 0; s < 8; s += 2) psp[s >> 1] = ((uint32_t)demod_pos_of<NC>(a, tid, s) & 0xffffu) | ((uint32_t)demod_pos_of<NC>(a, tid, s + 1) << 16);
    // cf2 points are as large as fp64 points, so the pair transform's LDS addresses are the pilot transforms': derived from
    // tid they would be computed once at the top of the kernel and held (or spilled) across the fit
    const int tp = launder(tid);
    RawPair<DT> nxb[8];                                                    // a pair's second symbol
    cf2 vp[8], z0p;
    // The first pair of data symbols, held behind the fp64 start-up by the scheduling barrier.  Fetched earlier (with the
    // last pilot, as the one-symbol loop does, or under the rotation tables) the f32 instantiations of the fused sizes
    // spill 8-11 VGPRs: the start-up has the 32 table reads of its rotations in flight next to u and gstep.  (One exposed
    // fetch per packet; the CU's other workgroup runs under it.)
    __builtin_amdgcn_sched_barrier(0);
    demod_fetch<NC, DT, STAGE_ALL>(a, f, off, tid, 2 * P, nxt);
    if (D > 1) demod_fetch<NC, DT, STAGE_ALL>(a, f, off, tid, 2 * P + 1, nxb);
    // Two symbols decided and two packed per turn.  The ring (demod_ring): while demod_pack_words(l - 2) and (l - 1) read slots
    // l - 2 - ceil(32 / (C mu)) .. l - 1, NO slot is written -- the barrier below stands between the packing and the
    // decisions of symbols l, l + 1, whose slots may then be any the coming packs no longer need: they overwrite l - ring
    // and l + 1 - ring, and the oldest slot still to be read is l - ceil(32 / (C mu)) (the turn after), so
    // ring >= ceil(32 / (C mu)) + 2 as for one symbol per turn.  (Without the barrier five slots would be in use at
    // C mu = 4092 and the ring would have to double, which two workgroups per CU have no LDS for.)
    for (int l = 0; l < D; l += 2) {
        const bool hb = l + 1 < D;
        const int par = (l >> 1) & 1;
        {   // the pair's transform
            float sa = 0.0f, sb = 0.0f;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const cf pa = make_float2((float)nxt[r].v.a, (float)nxt[r].v.b);
                const cf pb = make_float2(hb ? (float)nxb[r].v.a : 0.0f, hb ? (float)nxb[r].v.b : 0.0f);
                sa += fabsf(pa.x) + fabsf(pa.y);
                sb += fabsf(pb.x) + fabsf(pb.y);
                vp[r] = pair_of(pa, pb);
            }
            if (l + 2 < D) demod_fetch<NC, DT, STAGE_ALL>(a, f, off, tid, 2 * P + l + 2, nxt);
            sa = scr_wave_reduce<false>(sa);
            sb = scr_wave_reduce<false>(sb);
            if ((tid & 63) == 0) { l1s[par * 16 + (tid >> 6)] = sa; l1s[par * 16 + 8 + (tid >> 6)] = sb; }
            ft32.refresh();
            asm volatile("" : "+v"(wb32.x), "+v"(wb32.y));
            rfft_regs<NC, DemodOcc<NC, MODE_QPSK>::PP, true>(vp, (cf2*)m.fft, ft32, wb32, tp, z0p, par);
        }
        // the next pair's second symbol is fetched under the packing and the decisions, its first under the transform: two
        // symbols in flight across the transform do not fit the register file (f32 storage: 16 VGPRs each)
        if (l + 3 < D) demod_fetch<NC, DT, STAGE_ALL>(a, f, off, tid, 2 * P + l + 3, nxb);
        if (l > 0) { demod_pack_words<NC>(a, row, labs, tid, l - 2, false); demod_pack_words<NC>(a, row, labs, tid, l - 1, false); }
        lds_barrier();
        float l1a = 0.0f, l1b = 0.0f;
#pragma unroll
        for (int w = 0; w < (T + 63) / 64; ++w) { l1a += l1s[par * 16 + w]; l1b += l1s[par * 16 + 8 + w]; }
        const float Ea = dscr_bound<NC>(l1a), Eb = dscr_bound<NC>(l1b);      // (an absent half: l1b = 0, Eb finite)
        unsafe = unsafe || !(Ea < INFINITY) || !(Eb < INFINITY);
        if (a.dbg_E && tid == 0) {
            a.dbg_E[f * D + l] = Ea;
            if (hb) a.dbg_E[f * D + l + 1] = Eb;
        }
        uint8_t* lab_a = labs + (l & (a.ring - 1)) * C;
        uint8_t* lab_b = labs + ((l + 1) & (a.ring - 1)) * C;
        const float Ca = dscr_rot(l), Cb = dscr_rot(l + 1);
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const cf ga = g32[s];
            const cf gb = cmul(ga, gs32[s]);                               // the recurrence of the fp64 kernel, in fp32
            g32[s] = cmul(gb, gs32[s]);
            cf epa, epb;
            bool safe_a, safe_b;
            const uint32_t la = dscr_decide(half_a(vp[s]), ga, Ea, Ca, epa, safe_a);
            const uint32_t lb = dscr_decide(half_b(vp[s]), gb, Eb, Cb, epb, safe_b);
            const int ps = (int)((psp[s >> 1] >> (16 * (s & 1))) & 0xffffu);
            if (ps != 0xffff) {
                lab_a[ps] = (uint8_t)la;
                unsafe = unsafe || !safe_a;
                if (a.dbg_ep) a.dbg_ep[(f * D + l) * (int64_t)C + ps] = epa;
                if (hb) {
                    lab_b[ps] = (uint8_t)lb;
                    unsafe = unsafe || !safe_b;
                    if (a.dbg_ep) a.dbg_ep[(f * D + l + 1) * (int64_t)C + ps] = epb;
                }
            }
        }
    }
    GF3_STAMP(4);
    if (unsafe) *unsafe_flag = 1;
    lds_barrier();
    if ((D & 1) == 0) demod_pack_words<NC>(a, row, labs, tid, D - 2, false);             // the last pair's first symbol
    demod_pack_words<NC>(a, row, labs, tid, D - 1, ((D * C * a.mu) & 31) != 0);
    if (tid == 0) {                                                        // (the row is written anyway: the fp64 pass overwrites it)
        if (*unsafe_flag) a.dwork[16 + atomicAdd(a.dwork, 1)] = (int)f;
    }
    GF3_STAMP(5);
    GF3_STAMP_RT(7);
}
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
