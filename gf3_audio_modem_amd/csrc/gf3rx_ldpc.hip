// libgf3rx -- quasi-cyclic LDPC coding (lifting Z = 64 = one wavefront): the code object, the dual-diagonal encoder,
// the layered normalised min-sum decoder and the channel-state weighting of gf3_soft_demap_csi.  See DESIGN.md §12.
//
// Bit j*64 + t of a codeword is bit t of block column j; a non-zero block (i, j) with shift s is the circulant whose row z
// has its one in column (z + s) & 63.  Lane z of a wave owns check row z of every block row (decoder) or bit z of every
// block (encoder); one wave is one codeword and the waves of a workgroup are independent (no barrier anywhere).
#include "gf3rx_host.h"

// The decoder's parity contract is bit-exactness with a float32 NumPy restatement of the same schedule
// (tests/ldpc_ref.py): no multiply-add may be contracted into an FMA in this unit.
#pragma clang fp contract(off)

namespace {

constexpr int LZ = 64;                  // lifting size == wavefront
constexpr int LWAVES = 4;               // codewords per workgroup
constexpr int LMAX_NB = 32;             // block columns (and so row degree) at most: a row's sign bits fit one word
constexpr float LALPHA = 0.75f;         // min-sum normalisation

struct LdpcArgs {
    const int* rp;                      // [mb+1] first entry of each block row
    const int* ent;                     // [nnz] column | shift << 8, row by row, columns ascending
    int mb, nb, kb;
    int64_t n_cw;
    const float* llr; int max_iter; uint8_t* bits; float* app; int32_t* iters;      // decoder
    const uint8_t* msg; uint8_t* cw; int x, mid;                                    // encoder
};

// Other lanes read what this lane wrote to LDS (and the reverse): LDS operations of one wave complete in order, so
// all that is needed is that the compiler keeps them in program order across this point.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Layered normalised min-sum.  APP lives in LDS as [nb][64] f32 per wave (the circulant access (z + s) & 63 puts the
// 64 lanes on 64 consecutive words: no bank conflicts).  The check messages of block row L are kept compressed per lane:
// min1, min2, the index of min1 and the sign bits of the row's R values; R is never stored per edge but recomputed,
// bit-identically, as R_e = +-alpha * (e == idx ? min2 : min1) where it is needed.
//
// One block row (layer) for lane z; (m1, m2, ix, rs) is the row's state, updated in place.  R starts at +0 (state 0).
__device__ __forceinline__ void ldpc_layer(const LdpcArgs& a, float* app, int L, int z, float& m1, float& m2, int& ix,
                                           unsigned& rs) {
    const int e0 = a.rp[L], e1 = a.rp[L + 1];
    const float o1 = m1, o2 = m2;
    const int oix = ix;
    const unsigned ors = rs;                                   // bit e: R_e < 0
    float n1 = INFINITY, n2 = INFINITY;
    int nix = 0;
    unsigned neg = 0u;
    for (int e = e0; e < e1; ++e) {                            // pass 1: q = APP - R_old, the two minima, the signs
        const int t = a.ent[e], k = e - e0;
        const float v = app[(t & 0xff) * LZ + ((z + (t >> 8)) & 63)];
        float r = LALPHA * (k == oix ? o2 : o1);
        if ((ors >> k) & 1u) r = -r;
        const float q = v - r;
        const float aq = fabsf(q);
        if (aq < n1) { n2 = n1; n1 = aq; nix = k; }            // first minimum wins ties
        else if (aq < n2) n2 = aq;
        neg |= (unsigned)(q < 0.0f) << k;                       // sign(0) = +
    }
    const unsigned nrs = (__popc(neg) & 1) ? ~neg : neg;       // sign of the product of the OTHER q's
    for (int e = e0; e < e1; ++e) {                            // pass 2: the same q again, APP = q + R_new
        const int t = a.ent[e], k = e - e0;
        const int at = (t & 0xff) * LZ + ((z + (t >> 8)) & 63);
        float r = LALPHA * (k == oix ? o2 : o1);
        if ((ors >> k) & 1u) r = -r;
        const float q = app[at] - r;
        float rn = LALPHA * (k == nix ? n2 : n1);
        if ((nrs >> k) & 1u) rn = -rn;
        app[at] = q + rn;
    }
    m1 = n1; m2 = n2; ix = nix; rs = nrs;
    wave_sync();
}
// check row z of block row L on the decisions APP < 0
__device__ __forceinline__ unsigned ldpc_parity(const LdpcArgs& a, const float* app, int L, int z) {
    unsigned par = 0u;
    for (int e = a.rp[L]; e < a.rp[L + 1]; ++e) {
        const int t = a.ent[e];
        par ^= (unsigned)(app[(t & 0xff) * LZ + ((z + (t >> 8)) & 63)] < 0.0f);
    }
    return par;
}

// MAXL > 0: the row states live in VGPRs (4 per block row, loops unrolled to MAXL rows; 4 codewords per workgroup).
// MAXL == 0: codes with more block rows keep them in LDS after the wave's APP ([4][mb][64] words; one codeword per
// workgroup).
template <int MAXL>
__global__ __launch_bounds__(256) void ldpc_decode_kernel(LdpcArgs a) {
    extern __shared__ float ldpc_lds[];
    const int w = threadIdx.x >> 6, z = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * (blockDim.x >> 6) + w;
    if (c >= a.n_cw) return;                                   // (a whole wave: nothing below synchronises the workgroup)
    const int nb = a.nb, mb = a.mb, n = nb * LZ;
    float* app = ldpc_lds + (size_t)w * (n + (MAXL > 0 ? 0 : 4 * mb * LZ));
    const float* in = a.llr + c * n;
    for (int j = 0; j < nb; ++j) app[j * LZ + z] = in[j * LZ + z];
    float m1[MAXL > 0 ? MAXL : 1], m2[MAXL > 0 ? MAXL : 1];
    int ix[MAXL > 0 ? MAXL : 1];
    unsigned rs[MAXL > 0 ? MAXL : 1];
    float* st = app + n;                                       // (MAXL == 0) [4][mb][64]: min1, min2, idx, sign bits
    if constexpr (MAXL > 0) {
#pragma unroll
        for (int L = 0; L < MAXL; ++L) { m1[L] = 0.0f; m2[L] = 0.0f; ix[L] = 0; rs[L] = 0u; }
    } else {
        for (int i = 0; i < 4 * mb; ++i) st[i * LZ + z] = 0.0f;
    }
    wave_sync();
    int used = -a.max_iter;
    for (int it = 0; it < a.max_iter; ++it) {
        unsigned bad = 0u;
        if constexpr (MAXL > 0) {
#pragma unroll
            for (int L = 0; L < MAXL; ++L)
                if (L < mb) ldpc_layer(a, app, L, z, m1[L], m2[L], ix[L], rs[L]);
#pragma unroll
            for (int L = 0; L < MAXL; ++L)
                if (L < mb) bad |= ldpc_parity(a, app, L, z);
        } else {
            for (int L = 0; L < mb; ++L) {
                float s1 = st[(0 * mb + L) * LZ + z], s2 = st[(1 * mb + L) * LZ + z];
                int si = __float_as_int(st[(2 * mb + L) * LZ + z]);
                unsigned ss = __float_as_uint(st[(3 * mb + L) * LZ + z]);
                ldpc_layer(a, app, L, z, s1, s2, si, ss);
                st[(0 * mb + L) * LZ + z] = s1; st[(1 * mb + L) * LZ + z] = s2;
                st[(2 * mb + L) * LZ + z] = __int_as_float(si); st[(3 * mb + L) * LZ + z] = __uint_as_float(ss);
            }
            for (int L = 0; L < mb; ++L) bad |= ldpc_parity(a, app, L, z);
        }
        if (!__any((int)bad)) { used = it + 1; break; }
    }
    const int k = a.kb * LZ;
    for (int j = 0; j < a.kb; ++j) a.bits[c * k + j * LZ + z] = (uint8_t)(app[j * LZ + z] < 0.0f);
    if (a.app)
        for (int j = 0; j < nb; ++j) a.app[c * n + j * LZ + z] = app[j * LZ + z];
    if (a.iters && z == 0) a.iters[c] = used;
}

// Dual-diagonal encoder: lambda_i = sum_j P^{s_ij} m_j over the message blocks of row i, p0 = sum_i lambda_i,
// p1 = lambda_0 + P^x p0, p_{i+1} = lambda_i + p_i (+ p0 at the middle row).  Lane z computes bit z of every block.
__device__ __forceinline__ unsigned ldpc_lambda(const LdpcArgs& a, const uint8_t* m, int i, int z) {
    unsigned l = 0u;
    for (int e = a.rp[i]; e < a.rp[i + 1]; ++e) {
        const int t = a.ent[e], col = t & 0xff;
        if (col < a.kb) l ^= m[col * LZ + ((z + (t >> 8)) & 63)];
    }
    return l;
}
__global__ __launch_bounds__(256) void ldpc_encode_kernel(LdpcArgs a) {
    __shared__ uint8_t ms[LWAVES][LMAX_NB * LZ];
    __shared__ uint8_t p0s[LWAVES][LZ];
    const int w = threadIdx.x >> 6, z = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * LWAVES + w;
    if (c >= a.n_cw) return;
    const int kb = a.kb, mb = a.mb, k = kb * LZ, n = a.nb * LZ;
    const uint8_t* msg = a.msg + c * k;
    uint8_t* out = a.cw + c * n;
    uint8_t* m = ms[w];
    for (int j = 0; j < kb; ++j) {
        const uint8_t v = msg[j * LZ + z] & 1;
        m[j * LZ + z] = v;
        out[j * LZ + z] = v;
    }
    wave_sync();
    unsigned p0 = 0u;
    for (int i = 0; i < mb; ++i) p0 ^= ldpc_lambda(a, m, i, z);
    p0s[w][z] = (uint8_t)p0;
    wave_sync();
    out[k + z] = (uint8_t)p0;
    unsigned p = ldpc_lambda(a, m, 0, z) ^ p0s[w][(z + a.x) & 63];
    out[k + LZ + z] = (uint8_t)p;
    for (int i = 1; i < mb - 1; ++i) {
        p ^= ldpc_lambda(a, m, i, z) ^ (i == a.mid ? p0 : 0u);
        out[k + (i + 1) * LZ + z] = (uint8_t)p;
    }
}

// CSI weighting of max-log LLRs (computed with sigma^2 = 1 by the soft demapper): LLR *= |H^|^2 with the reference's
// magnitude model |Hs| + (|He| - |Hs|) (l + P/2) / (D + P) (OFDM.py:469), from Hs / He [F, K] directly.  A thread owns
// carrier k of symbol (f, l); carriers that carry no data (pos[k] < 0) have nothing to do.
struct CsiArgs { float* llr; const cplx* Hs; const cplx* He; const int* pos; int64_t F; int K, D, P, C, mu; };
__global__ __launch_bounds__(256) void csi_weight_kernel(CsiArgs a) {
    const int64_t total = a.F * a.D * a.K, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const int kk = (int)(t % a.K);
        const int pos = a.pos[kk];
        if (pos < 0) continue;
        const int64_t fl = t / a.K, f = fl / a.D;
        const int l = (int)(fl - f * a.D);
        const cplx hs = a.Hs[f * a.K + kk], he = a.He[f * a.K + kk];
        const double s = hypot(hs.x, hs.y), e = hypot(he.x, he.y);
        const double mag = s + (e - s) * (l + a.P / 2.0) / (double)(a.D + a.P);
        const double wgt = mag * mag;
        float* p = a.llr + (fl * a.C + pos) * a.mu;
        for (int b = 0; b < a.mu; ++b) p[b] = (float)((double)p[b] * wgt);
    }
}

}  // namespace

hipError_t launch_csi_weight(const gf3_ctx* c, float* d_llr, const void* d_Hs, const void* d_He, int64_t F, hipStream_t st) {
    CsiArgs a{d_llr, (const cplx*)d_Hs, (const cplx*)d_He, c->d_pos, F, c->K, c->cfg.D, c->cfg.P, c->cfg.C, c->cfg.mu};
    int64_t grid = (F * c->cfg.D * c->K + 255) / 256;
    if (grid > 16 * (int64_t)c->n_cu) grid = 16 * (int64_t)c->n_cu;
    if (grid < 1) return hipSuccess;
    hipLaunchKernelGGL(csi_weight_kernel, dim3((unsigned)grid), dim3(256), 0, st, a);
    return hipGetLastError();
}

// ============================================================================
// the code object and its entry points (include/gf3rx.h)
// ============================================================================
struct gf3_ldpc {
    int mb = 0, nb = 0, kb = 0, nnz = 0, device = 0;
    bool encodable = false;
    int x = 0, mid = 0;                 // dual-diagonal parameters (encodable codes)
    int* d_rp = nullptr;
    int* d_ent = nullptr;
};

namespace {
struct LdpcGuard {                      // run on the device the code's tables live on
    int prev = -1; bool switched = false;
    explicit LdpcGuard(const gf3_ldpc* q) {
        if (q && hipGetDevice(&prev) == hipSuccess && prev != q->device) switched = hipSetDevice(q->device) == hipSuccess;
    }
    ~LdpcGuard() { if (switched) (void)hipSetDevice(prev); }
};

// dual-diagonal parity part (first parity column x, 0, x at rows 0, mid, mb-1; the others bidiagonal with shift 0)?
bool dual_diagonal(const std::vector<int16_t>& h, int mb, int nb, int& x, int& mid) {
    const int kb = nb - mb;
    if (mb < 3) return false;
    auto at = [&](int i, int j) { return (int)h[(size_t)i * nb + j]; };
    int cnt = 0;
    mid = -1;
    for (int i = 0; i < mb; ++i)
        if (at(i, kb) >= 0) { ++cnt; if (i != 0 && i != mb - 1) mid = i; }
    if (cnt != 3 || mid < 0 || at(0, kb) < 0 || at(0, kb) != at(mb - 1, kb) || at(mid, kb) != 0) return false;
    x = at(0, kb);
    for (int col = 1; col < mb; ++col)
        for (int i = 0; i < mb; ++i) {
            const int want = (i == col - 1 || i == col) ? 0 : -1;
            if (at(i, kb + col) != want) return false;
        }
    return true;
}
}  // namespace

extern "C" int gf3_ldpc_create(int32_t mb, int32_t nb, int32_t Z, const int16_t* h_shifts, gf3_ldpc** out) {
    if (!h_shifts || !out) return fail(nullptr, GF3_EINVAL, "gf3_ldpc_create: null argument");
    *out = nullptr;
    if (Z != LZ) return fail(nullptr, GF3_EINVAL, "gf3_ldpc_create: Z=%d unsupported (the lifting size is 64)", Z);
    if (mb < 1 || nb > LMAX_NB || mb >= nb) return fail(nullptr, GF3_EINVAL, "gf3_ldpc_create: need 0 < mb < nb <= 32 (mb=%d, nb=%d)", mb, nb);
    std::vector<int16_t> h(h_shifts, h_shifts + (size_t)mb * nb);
    std::vector<int> rp(mb + 1, 0), ent;
    for (int i = 0; i < mb; ++i) {
        for (int j = 0; j < nb; ++j) {
            const int s = h[(size_t)i * nb + j];
            if (s < -1 || s >= LZ) return fail(nullptr, GF3_EINVAL, "gf3_ldpc_create: shift %d at (%d, %d) outside [-1, 64)", s, i, j);
            if (s >= 0) ent.push_back(j | (s << 8));
        }
        rp[i + 1] = (int)ent.size();
        if (rp[i + 1] - rp[i] < 2) return fail(nullptr, GF3_EINVAL, "gf3_ldpc_create: block row %d has fewer than 2 non-zero blocks", i);
    }
    gf3_ldpc* q = new gf3_ldpc;
    q->mb = mb; q->nb = nb; q->kb = nb - mb; q->nnz = (int)ent.size();
    q->encodable = dual_diagonal(h, mb, nb, q->x, q->mid);
    hipError_t e = hipGetDevice(&q->device);
    if (e == hipSuccess) e = hipMalloc((void**)&q->d_rp, rp.size() * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&q->d_ent, ent.size() * sizeof(int));
    if (e == hipSuccess) e = hipMemcpy(q->d_rp, rp.data(), rp.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(q->d_ent, ent.data(), ent.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        gf3_ldpc_destroy(q);
        return fail(nullptr, GF3_EHIP, "gf3_ldpc_create: %s", hipGetErrorString(e));
    }
    *out = q;
    return GF3_OK;
}

extern "C" void gf3_ldpc_destroy(gf3_ldpc* q) {
    if (!q) return;
    LdpcGuard g(q);
    if (q->d_rp) (void)hipFree(q->d_rp);
    if (q->d_ent) (void)hipFree(q->d_ent);
    delete q;
}

extern "C" int32_t gf3_ldpc_n(const gf3_ldpc* q) { return q ? q->nb * LZ : 0; }
extern "C" int32_t gf3_ldpc_k(const gf3_ldpc* q) { return q ? q->kb * LZ : 0; }

static LdpcArgs ldpc_args(const gf3_ldpc* q, int64_t n_cw) {
    LdpcArgs a{};
    a.rp = q->d_rp; a.ent = q->d_ent; a.mb = q->mb; a.nb = q->nb; a.kb = q->kb; a.n_cw = n_cw;
    a.x = q->x; a.mid = q->mid;
    return a;
}

extern "C" int gf3_ldpc_encode(const gf3_ldpc* q, const uint8_t* d_msg, int64_t n_cw, uint8_t* d_cw, void* stream) {
    if (q && n_cw == 0) return GF3_OK;
    if (!q || !d_msg || !d_cw || n_cw < 0) return fail(nullptr, GF3_EINVAL, "gf3_ldpc_encode: bad argument");
    if (!q->encodable) return fail(nullptr, GF3_EINVAL, "gf3_ldpc_encode: the code has no dual-diagonal parity part (decoding only)");
    LdpcGuard g(q);
    LdpcArgs a = ldpc_args(q, n_cw);
    a.msg = d_msg; a.cw = d_cw;
    const int64_t grid = (n_cw + LWAVES - 1) / LWAVES;
    if (grid > 0x7fffffff) return fail(nullptr, GF3_EINVAL, "gf3_ldpc_encode: n_cw too large");
    hipLaunchKernelGGL(ldpc_encode_kernel, dim3((unsigned)grid), dim3(LWAVES * LZ), 0, (hipStream_t)stream, a);
    HIPCHK(nullptr, hipGetLastError());
    return GF3_OK;
}

extern "C" int gf3_ldpc_decode(const gf3_ldpc* q, const float* d_llr, int64_t n_cw, int32_t max_iter, uint8_t* d_bits,
                               float* d_app, int32_t* d_iters, void* stream) {
    if (q && n_cw == 0 && max_iter >= 1) return GF3_OK;
    if (!q || !d_llr || !d_bits || n_cw < 0 || max_iter < 1) return fail(nullptr, GF3_EINVAL, "gf3_ldpc_decode: bad argument (max_iter >= 1)");
    LdpcGuard g(q);
    LdpcArgs a = ldpc_args(q, n_cw);
    a.llr = d_llr; a.max_iter = max_iter; a.bits = d_bits; a.app = d_app; a.iters = d_iters;
    const int64_t grid = (n_cw + LWAVES - 1) / LWAVES;
    if (n_cw > 0x7fffffff) return fail(nullptr, GF3_EINVAL, "gf3_ldpc_decode: n_cw too large");
    if (q->mb <= 12) {
        const size_t lds = (size_t)LWAVES * q->nb * LZ * sizeof(float);
        hipLaunchKernelGGL(ldpc_decode_kernel<12>, dim3((unsigned)grid), dim3(LWAVES * LZ), lds, (hipStream_t)stream, a);
    } else {                                                   // <= 40 KB of LDS for one wave
        const size_t lds = (size_t)(q->nb + 4 * q->mb) * LZ * sizeof(float);
        hipLaunchKernelGGL(ldpc_decode_kernel<0>, dim3((unsigned)n_cw), dim3(LZ), lds, (hipStream_t)stream, a);
    }
    HIPCHK(nullptr, hipGetLastError());
    return GF3_OK;
}
