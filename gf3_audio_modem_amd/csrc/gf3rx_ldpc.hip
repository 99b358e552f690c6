// libgf3rx -- quasi-cyclic LDPC coding (lifting Z = 64, 128 or 256): the code object, the dual-diagonal encoder, the
// layered normalised min-sum decoder.  See DESIGN.md §12.
//
// Bit j*Z + t of a codeword is bit t of block column j; a non-zero block (i, j) with shift s is the circulant whose row z
// has its one in column (z + s) mod Z.  Thread z owns check row z of every block row (decoder) or bit z of every block
// (encoder).  Z = 64: one wave is one codeword and the waves of a workgroup are independent (no barrier anywhere).
// Z = 128, 256 (the *_wide kernels): the Z/64 waves of one workgroup share one codeword and meet at workgroup barriers.
#include "gf3rx_host.h"

// The decoder's parity contract is bit-exactness with a float32 NumPy restatement of the same schedule
// (tests/ldpc_ref.py): no multiply-add may be contracted into an FMA in this unit.
#pragma clang fp contract(off)

namespace {

constexpr int LZ = 64;                  // lifting size == wavefront (the kernels that are not *_wide)
constexpr int LZ_MAX = 256;             // largest lifting size: one workgroup of four waves
constexpr int LWAVES = 4;               // codewords per workgroup (Z = 64)
constexpr int LMAX_NB = 32;             // block columns (and so row degree) at most: a row's sign bits fit one word
constexpr float LALPHA = 0.75f;         // min-sum normalisation

struct LdpcArgs {
    const int* rp;                      // [mb+1] first entry of each block row
    const int* ent;                     // [nnz] column | shift << 8, row by row, columns ascending
    int mb, nb, kb;
    int Z;                              // lifting size: read by the *_wide kernels only (== blockDim.x there)
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
// WIDE = false: the lifting size is the constant 64 and one wave owns the codeword.  WIDE = true: Z = a.Z threads, Z/64
// waves, own it, so a point where other rows' LDS writes must have landed is a workgroup barrier.
template <bool WIDE> __device__ __forceinline__ int ldpc_z(const LdpcArgs& a) { return WIDE ? a.Z : LZ; }
template <bool WIDE> __device__ __forceinline__ void ldpc_sync() {
    if constexpr (WIDE) __syncthreads(); else wave_sync();
}

// Layered normalised min-sum.  APP lives in LDS as [nb][Z] f32 per codeword (the circulant access (z + s) & (Z - 1) puts
// the 64 lanes of a wave on 64 consecutive words, wrapped at most once: no bank conflicts).  The check messages of block row L are kept compressed per lane:
// min1, min2, the index of min1 and the sign bits of the row's R values; R is never stored per edge but recomputed,
// bit-identically, as R_e = +-alpha * (e == idx ? min2 : min1) where it is needed.
//
// One block row (layer) for check row z; (m1, m2, ix, rs) is the row's state, updated in place.  R starts at +0
// (state 0).  A block row has one circulant per block column, so within a layer every APP word belongs to exactly one
// check row: rows conflict only between layers, which is where the synchronisation at the end stands.
template <bool WIDE>
__device__ __forceinline__ void ldpc_layer(const LdpcArgs& a, float* app, int L, int z, float& m1, float& m2, int& ix,
                                           unsigned& rs) {
    const int Z = ldpc_z<WIDE>(a), zm = Z - 1;
    const int e0 = a.rp[L], e1 = a.rp[L + 1];
    const float o1 = m1, o2 = m2;
    const int oix = ix;
    const unsigned ors = rs;                                   // bit e: R_e < 0
    float n1 = INFINITY, n2 = INFINITY;
    int nix = 0;
    unsigned neg = 0u;
    for (int e = e0; e < e1; ++e) {                            // pass 1: q = APP - R_old, the two minima, the signs
        const int t = a.ent[e], k = e - e0;
        const float v = app[(t & 0xff) * Z + ((z + (t >> 8)) & zm)];
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
        const int at = (t & 0xff) * Z + ((z + (t >> 8)) & zm);
        float r = LALPHA * (k == oix ? o2 : o1);
        if ((ors >> k) & 1u) r = -r;
        const float q = app[at] - r;
        float rn = LALPHA * (k == nix ? n2 : n1);
        if ((nrs >> k) & 1u) rn = -rn;
        app[at] = q + rn;
    }
    m1 = n1; m2 = n2; ix = nix; rs = nrs;
    ldpc_sync<WIDE>();
}
// check row z of block row L on the decisions APP < 0
template <bool WIDE>
__device__ __forceinline__ unsigned ldpc_parity(const LdpcArgs& a, const float* app, int L, int z) {
    const int Z = ldpc_z<WIDE>(a), zm = Z - 1;
    unsigned par = 0u;
    for (int e = a.rp[L]; e < a.rp[L + 1]; ++e) {
        const int t = a.ent[e];
        par ^= (unsigned)(app[(t & 0xff) * Z + ((z + (t >> 8)) & zm)] < 0.0f);
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
                if (L < mb) ldpc_layer<false>(a, app, L, z, m1[L], m2[L], ix[L], rs[L]);
#pragma unroll
            for (int L = 0; L < MAXL; ++L)
                if (L < mb) bad |= ldpc_parity<false>(a, app, L, z);
        } else {
            for (int L = 0; L < mb; ++L) {
                float s1 = st[(0 * mb + L) * LZ + z], s2 = st[(1 * mb + L) * LZ + z];
                int si = __float_as_int(st[(2 * mb + L) * LZ + z]);
                unsigned ss = __float_as_uint(st[(3 * mb + L) * LZ + z]);
                ldpc_layer<false>(a, app, L, z, s1, s2, si, ss);
                st[(0 * mb + L) * LZ + z] = s1; st[(1 * mb + L) * LZ + z] = s2;
                st[(2 * mb + L) * LZ + z] = __int_as_float(si); st[(3 * mb + L) * LZ + z] = __uint_as_float(ss);
            }
            for (int L = 0; L < mb; ++L) bad |= ldpc_parity<false>(a, app, L, z);
        }
        if (!__any((int)bad)) { used = it + 1; break; }
    }
    const int k = a.kb * LZ;
    for (int j = 0; j < a.kb; ++j) a.bits[c * k + j * LZ + z] = (uint8_t)(app[j * LZ + z] < 0.0f);
    if (a.app)
        for (int j = 0; j < nb; ++j) a.app[c * n + j * LZ + z] = app[j * LZ + z];
    if (a.iters && z == 0) a.iters[c] = used;
}

// Z = 128, 256: one codeword per workgroup of Z threads (blockDim.x == a.Z), thread z = check row z of every block row,
// the row states in VGPRs as above (mb <= MAXL).  Same schedule, arithmetic and stop rule as ldpc_decode_kernel; what is
// new is that the rows of a codeword sit in Z/64 waves:
//   - every layer ends in a workgroup barrier (ldpc_layer<true>), and so does the parity pass, before the next
//     iteration's first layer overwrites the APP words a slower wave may still be reading;
//   - the stop decision is the codeword's: each wave stores its own __any in its own LDS word before that barrier and
//     every wave reads all of them after it.  A word is rewritten one iteration later, after mb >= 1 layer barriers
//     that its readers have passed, and never reset.  The decision is the same in every wave, so all of them leave the
//     loop together: no wave skips a barrier (and there is no early return: a workgroup has no idle waves).
template <int MAXL>
__global__ __launch_bounds__(LZ_MAX) void ldpc_decode_wide_kernel(LdpcArgs a) {
    extern __shared__ float ldpc_lds[];
    const int Z = a.Z, z = threadIdx.x, w = z >> 6, nw = Z >> 6;
    const int64_t c = blockIdx.x;
    const int nb = a.nb, mb = a.mb, n = nb * Z;
    float* app = ldpc_lds;                                     // [nb][Z]
    int* vote = (int*)(ldpc_lds + n);                          // [Z / 64]
    const float* in = a.llr + c * n;
    for (int j = 0; j < nb; ++j) app[j * Z + z] = in[j * Z + z];
    float m1[MAXL], m2[MAXL];
    int ix[MAXL];
    unsigned rs[MAXL];
#pragma unroll
    for (int L = 0; L < MAXL; ++L) { m1[L] = 0.0f; m2[L] = 0.0f; ix[L] = 0; rs[L] = 0u; }
    __syncthreads();
    int used = -a.max_iter;
    for (int it = 0; it < a.max_iter; ++it) {
        unsigned bad = 0u;
#pragma unroll
        for (int L = 0; L < MAXL; ++L)
            if (L < mb) ldpc_layer<true>(a, app, L, z, m1[L], m2[L], ix[L], rs[L]);
#pragma unroll
        for (int L = 0; L < MAXL; ++L)
            if (L < mb) bad |= ldpc_parity<true>(a, app, L, z);
        const int any = __any((int)bad);
        if ((z & 63) == 0) vote[w] = any;
        __syncthreads();
        int all = 0;
        for (int v = 0; v < nw; ++v) all |= vote[v];
        if (!all) { used = it + 1; break; }                    // (workgroup-uniform)
    }
    const int k = a.kb * Z;
    for (int j = 0; j < a.kb; ++j) a.bits[c * k + j * Z + z] = (uint8_t)(app[j * Z + z] < 0.0f);
    if (a.app)
        for (int j = 0; j < nb; ++j) a.app[c * n + j * Z + z] = app[j * Z + z];
    if (a.iters && z == 0) a.iters[c] = used;
}

// Dual-diagonal encoder: lambda_i = sum_j P^{s_ij} m_j over the message blocks of row i, p0 = sum_i lambda_i,
// p1 = lambda_0 + P^x p0, p_{i+1} = lambda_i + p_i (+ p0 at the middle row).  Lane z computes bit z of every block.
template <bool WIDE>
__device__ __forceinline__ unsigned ldpc_lambda(const LdpcArgs& a, const uint8_t* m, int i, int z) {
    const int Z = ldpc_z<WIDE>(a), zm = Z - 1;
    unsigned l = 0u;
    for (int e = a.rp[i]; e < a.rp[i + 1]; ++e) {
        const int t = a.ent[e], col = t & 0xff;
        if (col < a.kb) l ^= m[col * Z + ((z + (t >> 8)) & zm)];
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
    for (int i = 0; i < mb; ++i) p0 ^= ldpc_lambda<false>(a, m, i, z);
    p0s[w][z] = (uint8_t)p0;
    wave_sync();
    out[k + z] = (uint8_t)p0;
    unsigned p = ldpc_lambda<false>(a, m, 0, z) ^ p0s[w][(z + a.x) & 63];
    out[k + LZ + z] = (uint8_t)p;
    for (int i = 1; i < mb - 1; ++i) {
        p ^= ldpc_lambda<false>(a, m, i, z) ^ (i == a.mid ? p0 : 0u);
        out[k + (i + 1) * LZ + z] = (uint8_t)p;
    }
}
// Z = 128, 256: one codeword per workgroup of Z threads; the message and p0 are read across waves, hence the barriers.
__global__ __launch_bounds__(LZ_MAX) void ldpc_encode_wide_kernel(LdpcArgs a) {
    __shared__ uint8_t m[LMAX_NB * LZ_MAX];
    __shared__ uint8_t p0s[LZ_MAX];
    const int Z = a.Z, z = threadIdx.x;
    const int64_t c = blockIdx.x;
    const int kb = a.kb, mb = a.mb, k = kb * Z, n = a.nb * Z;
    const uint8_t* msg = a.msg + c * k;
    uint8_t* out = a.cw + c * n;
    for (int j = 0; j < kb; ++j) {
        const uint8_t v = msg[j * Z + z] & 1;
        m[j * Z + z] = v;
        out[j * Z + z] = v;
    }
    __syncthreads();
    unsigned p0 = 0u;
    for (int i = 0; i < mb; ++i) p0 ^= ldpc_lambda<true>(a, m, i, z);
    p0s[z] = (uint8_t)p0;
    __syncthreads();
    out[k + z] = (uint8_t)p0;
    unsigned p = ldpc_lambda<true>(a, m, 0, z) ^ p0s[(z + a.x) & (Z - 1)];
    out[k + Z + z] = (uint8_t)p;
    for (int i = 1; i < mb - 1; ++i) {
        p ^= ldpc_lambda<true>(a, m, i, z) ^ (i == a.mid ? p0 : 0u);
        out[k + (i + 1) * Z + z] = (uint8_t)p;
    }
}

}  // namespace

// ============================================================================
// the code object and its entry points (include/gf3rx.h)
// ============================================================================
struct gf3_ldpc {
    int Z = LZ, mb = 0, nb = 0, kb = 0, nnz = 0, device = 0;
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
    if (Z != 64 && Z != 128 && Z != 256) return fail(nullptr, GF3_EINVAL, "gf3_ldpc_create: Z=%d unsupported (the lifting size is 64, 128 or 256)", Z);
    if (mb < 1 || nb > LMAX_NB || mb >= nb) return fail(nullptr, GF3_EINVAL, "gf3_ldpc_create: need 0 < mb < nb <= 32 (mb=%d, nb=%d)", mb, nb);
    if (Z > LZ && mb > 12)
        return fail(nullptr, GF3_EINVAL, "gf3_ldpc_create: Z=%d needs mb <= 12 (mb=%d): more block rows decode at Z=64 only", Z, mb);
    std::vector<int16_t> h(h_shifts, h_shifts + (size_t)mb * nb);
    std::vector<int> rp(mb + 1, 0), ent;
    for (int i = 0; i < mb; ++i) {
        for (int j = 0; j < nb; ++j) {
            const int s = h[(size_t)i * nb + j];
            if (s < -1 || s >= Z) return fail(nullptr, GF3_EINVAL, "gf3_ldpc_create: shift %d at (%d, %d) outside [-1, %d)", s, i, j, Z);
            if (s >= 0) ent.push_back(j | (s << 8));
        }
        rp[i + 1] = (int)ent.size();
        if (rp[i + 1] - rp[i] < 2) return fail(nullptr, GF3_EINVAL, "gf3_ldpc_create: block row %d has fewer than 2 non-zero blocks", i);
    }
    gf3_ldpc* q = new gf3_ldpc;
    q->Z = Z; q->mb = mb; q->nb = nb; q->kb = nb - mb; q->nnz = (int)ent.size();
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

extern "C" int32_t gf3_ldpc_n(const gf3_ldpc* q) { return q ? q->nb * q->Z : 0; }
extern "C" int32_t gf3_ldpc_k(const gf3_ldpc* q) { return q ? q->kb * q->Z : 0; }

static LdpcArgs ldpc_args(const gf3_ldpc* q, int64_t n_cw) {
    LdpcArgs a{};
    a.rp = q->d_rp; a.ent = q->d_ent; a.mb = q->mb; a.nb = q->nb; a.kb = q->kb; a.n_cw = n_cw;
    a.x = q->x; a.mid = q->mid; a.Z = q->Z;
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
    if (n_cw > 0x7fffffff) return fail(nullptr, GF3_EINVAL, "gf3_ldpc_encode: n_cw too large");
    if (q->Z > LZ) hipLaunchKernelGGL(ldpc_encode_wide_kernel, dim3((unsigned)n_cw), dim3(q->Z), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(ldpc_encode_kernel, dim3((unsigned)grid), dim3(LWAVES * LZ), 0, (hipStream_t)stream, a);
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
    if (q->Z > LZ) {                                           // (mb <= 12: gf3_ldpc_create)  <= 32 KB of LDS
        const size_t lds = ((size_t)q->nb * q->Z + q->Z / LZ) * sizeof(float);
        hipLaunchKernelGGL(ldpc_decode_wide_kernel<12>, dim3((unsigned)n_cw), dim3(q->Z), lds, (hipStream_t)stream, a);
    } else if (q->mb <= 12) {
        const size_t lds = (size_t)LWAVES * q->nb * LZ * sizeof(float);
        hipLaunchKernelGGL(ldpc_decode_kernel<12>, dim3((unsigned)grid), dim3(LWAVES * LZ), lds, (hipStream_t)stream, a);
    } else {                                                   // <= 40 KB of LDS for one wave
        const size_t lds = (size_t)(q->nb + 4 * q->mb) * LZ * sizeof(float);
        hipLaunchKernelGGL(ldpc_decode_kernel<0>, dim3((unsigned)n_cw), dim3(LZ), lds, (hipStream_t)stream, a);
    }
    HIPCHK(nullptr, hipGetLastError());
    return GF3_OK;
}
