// libgf3rx -- outer Reed-Solomon erasure code across LDPC codewords: systematic Cauchy parity over GF(2^8) on the
// message bytes of a group of codewords, and the repair of the members the inner decoder reports as failed.
// See DESIGN.md §12 and tests/outer_ref.py (the NumPy restatement these kernels are pinned to, bit for bit).
//
// Both kernels are the same streaming pass: E destination rows are each the GF(2^8) combination of M source rows with
// coefficients that are the same in every lane of a wave,  dst_t[b] = xor_m coef[m][t] * src_m[b]  per byte position b.
// A lane owns four consecutive byte positions (32 bytes of a row, one byte per bit) packed into one 32-bit word; the
// eight words d x^i are made once per source row on the vector unit and a destination accumulates those whose bit i
// of its coefficient is set -- the bit, a scalar, is spread into a 0 / ~0 mask on the scalar unit.  No table look-up
// by data anywhere.  Encoding: sources = the G data members, coefficients = the Cauchy matrix.  Recovery: sources = the
// surviving data members and the chosen parity rows, coefficients = A^-1 folded into the Cauchy rows, destinations =
// the erased data members.
#include <type_traits>

#include "gf3rx_host.h"
#include "gf3rx_outer.h"

namespace {

__constant__ RsInvTab rs_inv_tab = rs_make_inv();

constexpr int RS_THREADS = 256;
constexpr int RS_MAX_K = 1 << 20;       // message bits per codeword at most (index arithmetic of a row stays in 32 bits)

__device__ __forceinline__ void rs_wave_sync() {             // LDS written by other lanes of this wave (gf3rx_ldpc.hip)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// coefficient words in LDS: row m holds the RT coefficients of source m, four to a word (RT < 4: one word)
template <int RT> constexpr int rs_row_words() { return (RT + 3) / 4; }

// The lane's four byte positions (nv >= 1 of them exist) of M sources -> E <= RT destinations.  src(m) / dst(t) give
// the address of the lane's first byte in that row (8-byte aligned).
template <int RT, class Src, class Dst>
__device__ __forceinline__ void rs_stream(const uint32_t* coef, int M, int E, int nv, Src src, Dst dst) {
    constexpr int RW = rs_row_words<RT>();
    uint32_t acc[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) acc[t] = 0u;
    for (int m = 0; m < M; ++m) {
        const uint2* p = (const uint2*)src(m);
        uint2 w[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) w[s] = s < nv ? p[s] : make_uint2(0u, 0u);
        uint32_t d[8];
        d[0] = rs_pack(w[0].x, w[1].x, w[2].x, w[3].x, w[0].y, w[1].y, w[2].y, w[3].y);
#pragma unroll
        for (int i = 1; i < 8; ++i) d[i] = rs_xtime(d[i - 1]);
#pragma unroll
        for (int rw = 0; rw < RW; ++rw) {
            const int cw = __builtin_amdgcn_readfirstlane((int)coef[m * RW + rw]);
#pragma unroll
            for (int rr = 0; rr < (RT < 4 ? RT : 4); ++rr)
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    acc[rw * 4 + rr] ^= d[i] & (uint32_t)__builtin_amdgcn_sbfe(cw, 8 * rr + i, 1);
        }
    }
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        if (t < E) {
            uint2 o[4];
            rs_unpack(acc[t], o[0].x, o[1].x, o[2].x, o[3].x, o[0].y, o[1].y, o[2].y, o[3].y);
            uint2* q = (uint2*)dst(t);
#pragma unroll
            for (int s = 0; s < 4; ++s)
                if (s < nv) q[s] = o[s];
        }
    }
}

struct RsArgs {
    const uint8_t* msg; uint8_t* par;                          // encoder
    uint8_t* bits; const int32_t* iters; int32_t* status;      // recovery
    int64_t NG; int G, R, k;
    int Q;                                                     // lane items of a row: ceil(k / 32)
};

// Lane item T is byte positions 4q .. 4q+3 of group g, T = g Q + q: the Cauchy coefficients do not depend on the
// group, so the lanes of a wave may belong to different groups and short rows still fill the waves.
template <int RT>
__global__ __launch_bounds__(RS_THREADS) void rs_encode_kernel(RsArgs a) {
    constexpr int RW = rs_row_words<RT>();
    __shared__ uint32_t coef[RS_MAX_N * RW];
    for (int idx = threadIdx.x; idx < a.G * RW; idx += RS_THREADS) {       // C[r][j] = 1 / (r ^ (R + j)), 0 for r >= R
        const int j = idx / RW, rw = idx - j * RW;
        uint32_t w = 0u;
        for (int rr = 0; rr < 4; ++rr) {
            const int r = rw * 4 + rr;
            if (r < a.R) w |= (uint32_t)rs_inv_tab.v[r ^ (a.R + j)] << (8 * rr);
        }
        coef[idx] = w;
    }
    __syncthreads();
    const int64_t T = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    const int64_t g = T / a.Q;
    if (g >= a.NG) return;
    const int q = (int)(T - g * a.Q);
    const int nv = min(4, a.k / 8 - 4 * q);
    const int64_t k = a.k;
    rs_stream<RT>(coef, a.G, a.R, nv,
                  [&](int j) { return a.msg + ((g * a.G + j) * k + 32 * q); },
                  [&](int r) { return a.par + ((g * a.R + r) * k + 32 * q); });
}

// One workgroup per group.  Wave 0 reads the G + R flags, sorts the members into lists, writes the status and, for a
// group that can be repaired, inverts A in LDS; a group with nothing to repair ends there for every wave.  Then all
// waves fold A^-1 into the coefficients and stream.
template <int RT>
__global__ __launch_bounds__(RS_THREADS) void rs_recover_kernel(RsArgs a) {
    constexpr int RW = rs_row_words<RT>();
    __shared__ int s_status;
    __shared__ uint8_t s_dst[RS_MAX_R];                        // erased data members j, ascending (the first 16)
    __shared__ uint8_t s_prow[RS_MAX_R];                       // surviving parity rows r, ascending (the first 16)
    __shared__ uint8_t s_src[RS_MAX_N + 1];                    // sources: surviving data members, then G + chosen parity rows
    __shared__ uint8_t s_aug[RS_MAX_R][2 * RS_MAX_R];          // [A | I] -> [I | A^-1]
    __shared__ uint32_t s_coef[RS_MAX_N * RW];
    const int64_t g = blockIdx.x, NG = a.NG;
    const int G = a.G, R = a.R, n = G + R, tid = threadIdx.x;
    if (tid < 64) {
        const int lane = tid;
        const unsigned long long below = (1ull << lane) - 1ull;
        int n_ed = 0, n_sd = 0, n_ep = 0, n_sp = 0;
        for (int base = 0; base < n; base += 64) {
            const int t = base + lane;
            const bool in = t < n, data = t < G;
            const bool er = in && a.iters[(int64_t)t * NG + g] < 0;
            const unsigned long long b_ed = __ballot(er && data), b_sd = __ballot(in && !er && data);
            const unsigned long long b_ep = __ballot(er && !data), b_sp = __ballot(in && !er && !data);
            if (er && data) {
                const int i = n_ed + __popcll(b_ed & below);
                if (i < RS_MAX_R) s_dst[i] = (uint8_t)t;
            }
            if (in && !er && data) s_src[n_sd + __popcll(b_sd & below)] = (uint8_t)t;
            if (in && !er && !data) {
                const int i = n_sp + __popcll(b_sp & below);
                if (i < RS_MAX_R) s_prow[i] = (uint8_t)(t - G);
            }
            n_ed += __popcll(b_ed); n_sd += __popcll(b_sd); n_ep += __popcll(b_ep); n_sp += __popcll(b_sp);
        }
        const int e = n_ed;
        const int status = e == 0 ? 0 : (e > R - n_ep ? -e : e);
        if (lane == 0) { a.status[g] = status; s_status = status; }
        if (status > 0) {                                      // (the same in every lane: e <= n_sp <= 16)
            rs_wave_sync();
            if (lane < e) s_src[n_sd + lane] = (uint8_t)(G + s_prow[lane]);
            for (int idx = lane; idx < RS_MAX_R * 2 * RS_MAX_R; idx += 64) {
                const int i = idx >> 5, c = idx & 31;
                if (i < e && c < 2 * e)
                    s_aug[i][c] = c < e ? rs_inv_tab.v[s_prow[i] ^ (R + s_dst[c])] : (uint8_t)(c - e == i);
            }
            // Gauss-Jordan without row exchanges: every leading minor of a Cauchy matrix is non-zero, so is every pivot
            const int c = lane & 31;
            for (int p = 0; p < e; ++p) {
                rs_wave_sync();
                const unsigned pinv = rs_inv_tab.v[s_aug[p][p]];
                rs_wave_sync();
                if (lane < 2 * e) s_aug[p][lane] = (uint8_t)rs_mul(s_aug[p][lane], pinv);
                rs_wave_sync();
                const unsigned rowp = s_aug[p][c];
                unsigned f[8], v[8];
#pragma unroll
                for (int it = 0; it < 8; ++it) {               // row i = 2 it + lane / 32: read everything, then write
                    const int i = 2 * it + (lane >> 5);
                    f[it] = s_aug[i][p];
                    v[it] = s_aug[i][c];
                }
                rs_wave_sync();
#pragma unroll
                for (int it = 0; it < 8; ++it) {
                    const int i = 2 * it + (lane >> 5);
                    if (i < e && i != p && c < 2 * e) s_aug[i][c] = (uint8_t)(v[it] ^ rs_mul(f[it], rowp));
                }
            }
        }
    }
    __syncthreads();
    const int e = s_status;
    if (e <= 0) return;
    // D_t = xor_i Ainv[t][i] (P_ri ^ xor_j C[ri][j] D_j):  coefficient of a surviving D_j = xor_i Ainv[t][i] C[ri][j],
    // of the chosen P_ri = Ainv[t][i]
    for (int idx = tid; idx < G * RW; idx += blockDim.x) {
        const int m = idx / RW, rw = idx - m * RW, src = s_src[m];
        uint32_t w = 0u;
        for (int rr = 0; rr < 4; ++rr) {
            const int t = rw * 4 + rr;
            if (t >= e) break;
            unsigned cf = 0u;
            if (src >= G) cf = s_aug[t][e + (m - (G - e))];
            else
                for (int i = 0; i < e; ++i) cf ^= rs_mul(s_aug[t][e + i], rs_inv_tab.v[s_prow[i] ^ (R + src)]);
            w |= cf << (8 * rr);
        }
        s_coef[idx] = w;
    }
    __syncthreads();
    const int nb = a.k / 8, Q = a.Q;
    const int64_t k = a.k;
    for (int q = tid; q < Q; q += blockDim.x) {
        const int nv = min(4, nb - 4 * q);
        rs_stream<RT>(s_coef, G, e, nv,
                      [&](int m) { return a.bits + (((int64_t)s_src[m] * NG + g) * k + 32 * q); },
                      [&](int t) { return a.bits + (((int64_t)s_dst[t] * NG + g) * k + 32 * q); });
    }
}

int rs_geometry(const char* fn, int64_t NG, int G, int R, int k) {
    if (NG < 0) return fail(nullptr, GF3_EINVAL, "%s: NG=%lld is negative", fn, (long long)NG);
    if (R < 1 || R > RS_MAX_R) return fail(nullptr, GF3_EINVAL, "%s: need 1 <= R <= %d parity members (R=%d)", fn, RS_MAX_R, R);
    if (G < 1 || G + R > RS_MAX_N) return fail(nullptr, GF3_EINVAL, "%s: need G >= 1 and G + R <= %d (G=%d, R=%d)", fn, RS_MAX_N, G, R);
    if (k < 8 || k % 8 || k > RS_MAX_K)
        return fail(nullptr, GF3_EINVAL, "%s: k=%d must be a multiple of 8 in [8, %d] (whole bytes of message bits)", fn, k, RS_MAX_K);
    if (NG > 0x7fffffffll || NG * (int64_t)((k / 8 + 3) / 4) > 0x7fffffffll * RS_THREADS)      // (grid sizes)
        return fail(nullptr, GF3_EINVAL, "%s: NG=%lld too large", fn, (long long)NG);
    return GF3_OK;
}
bool rs_aligned(const void* p) { return ((uintptr_t)p & 7u) == 0; }

template <typename Fn> void rs_dispatch(int R, Fn&& fn) {
    if (R <= 1) fn(std::integral_constant<int, 1>());
    else if (R <= 2) fn(std::integral_constant<int, 2>());
    else if (R <= 4) fn(std::integral_constant<int, 4>());
    else if (R <= 8) fn(std::integral_constant<int, 8>());
    else fn(std::integral_constant<int, 16>());
}

}  // namespace

extern "C" int gf3_outer_encode(const uint8_t* d_msg_bits, int64_t NG, int32_t G, int32_t R, int32_t k,
                                uint8_t* d_par_bits, void* stream) {
    if (int rc = rs_geometry("gf3_outer_encode", NG, G, R, k)) return rc;
    if (NG == 0) return GF3_OK;
    if (!d_msg_bits || !d_par_bits || !rs_aligned(d_msg_bits) || !rs_aligned(d_par_bits))
        return fail(nullptr, GF3_EINVAL, "gf3_outer_encode: null or not 8-byte aligned array");
    RsArgs a{};
    a.msg = d_msg_bits; a.par = d_par_bits; a.NG = NG; a.G = G; a.R = R; a.k = k; a.Q = (k / 8 + 3) / 4;
    const int64_t grid = (NG * a.Q + RS_THREADS - 1) / RS_THREADS;
    rs_dispatch(R, [&](auto rt) {
        hipLaunchKernelGGL(rs_encode_kernel<decltype(rt)::value>, dim3((unsigned)grid), dim3(RS_THREADS), 0, (hipStream_t)stream, a);
    });
    HIPCHK(nullptr, hipGetLastError());
    return GF3_OK;
}

extern "C" int gf3_outer_recover(uint8_t* d_bits, const int32_t* d_iters, int64_t NG, int32_t G, int32_t R, int32_t k,
                                 int32_t* d_status, void* stream) {
    if (int rc = rs_geometry("gf3_outer_recover", NG, G, R, k)) return rc;
    if (NG == 0) return GF3_OK;
    if (!d_bits || !d_iters || !d_status || !rs_aligned(d_bits))
        return fail(nullptr, GF3_EINVAL, "gf3_outer_recover: null array, or bits not 8-byte aligned");
    RsArgs a{};
    a.bits = d_bits; a.iters = d_iters; a.status = d_status; a.NG = NG; a.G = G; a.R = R; a.k = k; a.Q = (k / 8 + 3) / 4;
    const int threads = a.Q >= RS_THREADS ? RS_THREADS : (a.Q + 63) / 64 * 64;
    rs_dispatch(R, [&](auto rt) {
        hipLaunchKernelGGL(rs_recover_kernel<decltype(rt)::value>, dim3((unsigned)NG), dim3(threads), 0, (hipStream_t)stream, a);
    });
    HIPCHK(nullptr, hipGetLastError());
    return GF3_OK;
}
