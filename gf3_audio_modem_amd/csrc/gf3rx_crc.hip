// libgf3rx -- per-codeword CRC-32: a codeword's message of k bits is a payload of k - 32 bits followed by the CRC-32/IEEE
// of the payload's bytes, so that a codeword the LDPC decoder converged on wrongly is seen and erased for the outer code.
// See DESIGN.md §12 and tests/crc_ref.py (zlib.crc32 and np.packbits: what these kernels are pinned to, byte for byte).
//
// Both kernels are one streaming pass built on linearity: the CRC of a row is the xor of one 32-bit word per set payload
// bit, plus the CRC of as many zero bytes.  The word of a bit depends only on how many bits follow it in the order the CRC
// consumes them, so ONE table (crc_bit_tab, made at compile time) serves every k.  A lane owns the same 8 bytes (8 bits,
// one payload byte) of every row it works on, so it reads its 8 table words once, keeps them in registers for all its
// rows, and a row costs it one 8-byte load, 8 x (mask from the bit, and-xor) and one 8-byte store.  No look-up indexed by
// data anywhere.  The 32 field bits are lane items like the others, with the words 2^31 .. 2^0: the xor over a whole
// valid row is then the CRC of the zero bytes, and the check is one compare.
// The partial words of a row's lanes meet without atomics: an inclusive xor scan inside each wave, the scans into LDS, and
// the xor over lanes a .. b is prefix(b) ^ prefix(a - 1), prefix(x) the scan at x with the totals of the waves before x in
// wave order (xor is exact, so any order gives the same bits; this one is fixed).  Rows shorter than the workgroup share
// it: the lanes of a wave may belong to different rows.
#include "gf3rx_host.h"

namespace {

constexpr uint32_t CRC_POLY = 0xEDB88320u;                   // CRC-32/IEEE, reflected
constexpr int CRC_BITS = 32;
constexpr int CRC_MIN_K = 40, CRC_MAX_K = 7936;              // 7936 = 31 * 256: the largest k gf3_ldpc_create accepts
constexpr int CRC_MAX_PAYLOAD = CRC_MAX_K - CRC_BITS;
constexpr int CRC_THREADS = 256;
constexpr int CRC_MAX_GRID = 2048;                           // 8 workgroups per compute unit; the rest by a strided loop

constexpr uint32_t crc_step(uint32_t s) { return (s >> 1) ^ ((0u - (s & 1u)) & CRC_POLY); }    // one zero bit

// v[d]: what a set bit adds to the CRC when d bits follow it (the state 1 consumed by the bit's own step and d more)
struct alignas(16) CrcBitTab { uint32_t v[CRC_MAX_PAYLOAD]; };
constexpr CrcBitTab crc_make_bits() {
    CrcBitTab t{};
    uint32_t s = CRC_POLY;
    for (int d = 0; d < CRC_MAX_PAYLOAD; ++d) {
        t.v[d] = s;
        s = crc_step(s);
    }
    return t;
}
// v[nb]: the CRC of nb zero bytes
struct CrcZeroTab { uint32_t v[CRC_MAX_PAYLOAD / 8 + 1]; };
constexpr CrcZeroTab crc_make_zero() {
    CrcZeroTab t{};
    uint32_t s = 0xFFFFFFFFu;
    for (int nb = 0; nb <= CRC_MAX_PAYLOAD / 8; ++nb) {
        t.v[nb] = ~s;
        for (int i = 0; i < 8; ++i) s = crc_step(s);
    }
    return t;
}

__constant__ CrcBitTab crc_bit_tab = crc_make_bits();
constexpr CrcZeroTab crc_zero_tab = crc_make_zero();
static_assert(crc_zero_tab.v[0] == 0u && crc_zero_tab.v[1] == 0xD202EF8Du && crc_zero_tab.v[4] == 0x2144DF1Cu,
              "CRC-32 of 0, 1 and 4 zero bytes");

struct CrcArgs {
    const uint8_t* in; uint8_t* out;        // attach: payload rows -> message rows; check: message rows -> payload rows or null
    int32_t* iters; uint8_t* bad;           // check: either may be null
    int64_t n_cw, n_pass;
    int Q, W, rp;                           // lane items (8 bytes) of a message row; threads of a row; rows of a pass
    uint32_t zero;                          // CRC of the payload's count of zero bytes
};

// xor of the partial words of threads 0 .. x: the scan of x's wave at x, and the totals of the waves before it in order
__device__ __forceinline__ uint32_t crc_prefix(const uint32_t* scan, int x) {
    uint32_t v = scan[x];
#pragma unroll
    for (int wv = 0; wv < CRC_THREADS / 64 - 1; ++wv)
        if (64 * wv + 63 < (x & ~63)) v ^= scan[64 * wv + 63];
    return v;
}

// Thread t serves row r = t / W of a pass and the lane items q = c + u W of it, c = t - r W, u < U (U W >= Q; rp > 1 rows
// only where U = 1).  A workgroup takes the passes blockIdx.x, blockIdx.x + gridDim.x, ...: the same items of other rows.
template <int U, bool CHECK>
__global__ __launch_bounds__(CRC_THREADS) void crc_kernel(CrcArgs a) {
    __shared__ uint32_t s_scan[2][CRC_THREADS];
    const int t = threadIdx.x, lane = t & 63;
    const int Q = a.Q, W = a.W, NB = Q - CRC_BITS / 8;
    const int r = t / W, c = t - r * W;
    const bool active = r < a.rp;
    const int first = r * W, last = first + W - 1;             // the row's threads (< blockDim.x for an active row)
    uint32_t w[U][8];
    bool field = false, closes = false;                        // owns bits of the CRC field; owns the row's last item
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int q = c + u * W;
        if (active && q < NB) {                                // payload byte q: 8 (NB - 1 - q) + j bits follow its byte j
            const uint4* p = (const uint4*)&crc_bit_tab.v[8 * (NB - 1 - q)];
            const uint4 lo = p[0], hi = p[1];
            w[u][0] = lo.x; w[u][1] = lo.y; w[u][2] = lo.z; w[u][3] = lo.w;
            w[u][4] = hi.x; w[u][5] = hi.y; w[u][6] = hi.z; w[u][7] = hi.w;
        } else if (active && q < Q) {                          // field bits 8 (q - NB) + j: bit 31 - i of the CRC
#pragma unroll
            for (int j = 0; j < 8; ++j) w[u][j] = 0x80000000u >> (8 * (q - NB) + j);
            field = true;
            closes = closes || q == Q - 1;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) w[u][j] = 0u;
        }
    }
    const int n_in = CHECK ? Q : NB;                           // items of an input row
    // the thread's items of the row it serves in `pass` (zeros beyond the rows and beyond the row's items)
    auto load = [&](int64_t pass, uint2 (&x)[U]) {
        const int64_t row = pass * a.rp + r;
        const bool ok = active && pass < a.n_pass && row < a.n_cw;
        const uint8_t* src = a.in + row * (8 * (int64_t)n_in);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = c + u * W;
            x[u] = ok && q < n_in ? *(const uint2*)(src + 8 * q) : make_uint2(0u, 0u);
        }
    };
    uint2 x[U], nx[U];
    load(blockIdx.x, x);
    int buf = 0;
    for (int64_t pass = blockIdx.x; pass < a.n_pass; pass += gridDim.x, buf ^= 1) {
        const int64_t row = pass * a.rp + r;
        const bool ok = active && row < a.n_cw;
        load(pass + gridDim.x, nx);                            // in flight behind this pass's arithmetic and barrier
        uint32_t part = 0u;
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) {                      // bit 0 of byte j -> 0 / ~0
                part ^= w[u][j] & (uint32_t)((int32_t)(x[u].x << (31 - 8 * j)) >> 31);
                part ^= w[u][4 + j] & (uint32_t)((int32_t)(x[u].y << (31 - 8 * j)) >> 31);
            }
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const uint32_t o = __shfl_up(part, s);
            if (lane >= s) part ^= o;
        }
        s_scan[buf][t] = part;
        // (one barrier a pass: the other buffer is rewritten only behind the next pass's barrier, which every thread
        // reaches after its reads of this one)
        __syncthreads();
        uint32_t total = 0u;                                   // attach: the CRC; check: 0 on a good row
        if (ok && field)
            total = crc_prefix(s_scan[buf], last) ^ (first ? crc_prefix(s_scan[buf], first - 1) : 0u) ^ a.zero;
        const uint32_t one = 0x01010101u;
        if (!ok) {
        } else if (!CHECK) {
            uint8_t* dst = a.out + row * (8 * (int64_t)Q);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int q = c + u * W;
                uint2 o = make_uint2(x[u].x & one, x[u].y & one);
                if (q >= NB) {
                    o = make_uint2(0u, 0u);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        o.x |= (uint32_t)((total & w[u][j]) != 0u) << (8 * j);
                        o.y |= (uint32_t)((total & w[u][4 + j]) != 0u) << (8 * j);
                    }
                }
                if (q < Q) *(uint2*)(dst + 8 * q) = o;
            }
        } else {
            if (a.out) {
                uint8_t* dst = a.out + row * (8 * (int64_t)NB);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int q = c + u * W;
                    if (q < NB) *(uint2*)(dst + 8 * q) = make_uint2(x[u].x & one, x[u].y & one);
                }
            }
            if (closes) {
                const bool bad = total != 0u;
                if (a.bad) a.bad[row] = (uint8_t)bad;
                if (a.iters && bad) {
                    const int32_t v = a.iters[row];
                    if (v > 0) a.iters[row] = -v;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = nx[u];
    }
}

int crc_geometry(const char* fn, int64_t n_cw, int k) {
    if (n_cw < 0) return fail(nullptr, GF3_EINVAL, "%s: n_cw=%lld is negative", fn, (long long)n_cw);
    if (k < CRC_MIN_K || k > CRC_MAX_K || k % 8)
        return fail(nullptr, GF3_EINVAL, "%s: k=%d must be a multiple of 8 in [%d, %d] (whole payload bytes and a 32-bit field)",
                    fn, k, CRC_MIN_K, CRC_MAX_K);
    return GF3_OK;
}
bool crc_aligned(const void* p) { return ((uintptr_t)p & 7u) == 0; }

template <bool CHECK> int crc_launch(CrcArgs a, int64_t n_cw, int k, hipStream_t st) {
    const int Q = k / 8, U = (Q + CRC_THREADS - 1) / CRC_THREADS;              // 1 .. 4 items per thread
    const int UT = U == 3 ? 4 : U;
    a.n_cw = n_cw; a.Q = Q;
    a.W = (Q + UT - 1) / UT;
    a.rp = UT == 1 ? CRC_THREADS / a.W : 1;
    a.n_pass = (n_cw + a.rp - 1) / a.rp;
    a.zero = crc_zero_tab.v[Q - CRC_BITS / 8];
    const int threads = (a.rp * a.W + 63) / 64 * 64;
    const unsigned grid = (unsigned)(a.n_pass < CRC_MAX_GRID ? a.n_pass : CRC_MAX_GRID);
    if (UT == 1) hipLaunchKernelGGL((crc_kernel<1, CHECK>), dim3(grid), dim3(threads), 0, st, a);
    else if (UT == 2) hipLaunchKernelGGL((crc_kernel<2, CHECK>), dim3(grid), dim3(threads), 0, st, a);
    else hipLaunchKernelGGL((crc_kernel<4, CHECK>), dim3(grid), dim3(threads), 0, st, a);
    HIPCHK(nullptr, hipGetLastError());
    return GF3_OK;
}

}  // namespace

extern "C" int gf3_crc_attach(const uint8_t* d_payload, int64_t n_cw, int32_t k, uint8_t* d_msg, void* stream) {
    if (int rc = crc_geometry("gf3_crc_attach", n_cw, k)) return rc;
    if (n_cw == 0) return GF3_OK;
    if (!d_payload || !d_msg || !crc_aligned(d_payload) || !crc_aligned(d_msg))
        return fail(nullptr, GF3_EINVAL, "gf3_crc_attach: null or not 8-byte aligned array");
    CrcArgs a{};
    a.in = d_payload; a.out = d_msg;
    return crc_launch<false>(a, n_cw, k, (hipStream_t)stream);
}

extern "C" int gf3_crc_check(const uint8_t* d_msg, int64_t n_cw, int32_t k, uint8_t* d_payload_or_null,
                             int32_t* d_iters_or_null, uint8_t* d_bad_or_null, void* stream) {
    if (int rc = crc_geometry("gf3_crc_check", n_cw, k)) return rc;
    if (n_cw == 0) return GF3_OK;
    if (!d_msg || !crc_aligned(d_msg) || !crc_aligned(d_payload_or_null) || ((uintptr_t)d_iters_or_null & 3u))
        return fail(nullptr, GF3_EINVAL, "gf3_crc_check: null message array, bits not 8-byte aligned or iteration counts not 4-byte aligned");
    CrcArgs a{};
    a.in = d_msg; a.out = d_payload_or_null; a.iters = d_iters_or_null; a.bad = d_bad_or_null;
    return crc_launch<true>(a, n_cw, k, (hipStream_t)stream);
}
