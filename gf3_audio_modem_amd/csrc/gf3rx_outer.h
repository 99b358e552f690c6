// GF(2^8) arithmetic of the outer Reed-Solomon erasure code (gf3rx_outer.hip): the field is
// GF(2)[x] / (x^8 + x^4 + x^3 + x^2 + 1) (0x11D).  Everything here is exact integer arithmetic and compiles for the host
// as well, so that it can be exercised without a device.
//
// Storage is one byte per bit.  A symbol is 8 consecutive bytes b0 .. b7 of a message row, b0 its most significant bit
// (np.packbits order).  A lane works on FOUR consecutive symbols at a time, SWAR style: the 8 x 4 bytes it loaded are
// turned into one 32-bit word with symbol s in byte s (rs_pack), the products are accumulated in that form, and a
// finished word is turned back into 4 x 8 bytes (rs_unpack).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RS_HD __host__ __device__ __forceinline__
#else
#define RS_HD inline
#endif

constexpr unsigned RS_POLY = 0x11Du;
constexpr int RS_MAX_R = 16;            // parity members of a group at most
constexpr int RS_MAX_N = 255;           // members of a group at most (the x_r, y_j of the Cauchy matrix are distinct bytes)

// a * b, table-free (shift and add): used where a product is needed once (the inversion, the combined coefficients)
RS_HD unsigned rs_mul(unsigned a, unsigned b) {
    unsigned p = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        p ^= (0u - ((b >> i) & 1u)) & a;
        a = (a << 1) ^ ((0u - (a >> 7)) & RS_POLY);            // (a < 256 before and after: 0x11D clears bit 8)
    }
    return p;
}

// 1 / a for a != 0, and 0 for 0: a^254 built at compile time into a table (the Cauchy coefficients are inverses)
struct RsInvTab { uint8_t v[256]; };
constexpr RsInvTab rs_make_inv() {
    RsInvTab t{};
    uint8_t ex[255] = {};
    int lg[256] = {};
    unsigned x = 1u;
    for (int i = 0; i < 255; ++i) {                            // x = 2^i: 2 generates the multiplicative group
        ex[i] = (uint8_t)x;
        lg[x] = i;
        x <<= 1;
        if (x & 0x100u) x ^= RS_POLY;
    }
    for (int a = 1; a < 256; ++a) t.v[a] = ex[(255 - lg[a]) % 255];
    return t;
}

// v_perm_b32: byte k of the result is byte sel[k] (0 .. 7) of the 64-bit value hi:lo
RS_HD uint32_t rs_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t v = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0u;
    for (int k = 0; k < 4; ++k) r |= (uint32_t)((v >> (8 * ((sel >> (8 * k)) & 7u))) & 0xffu) << (8 * k);
    return r;
#endif
}

// 4 x 4 byte transpose, in place: byte p of word s <-> byte s of word p (its own inverse)
RS_HD void rs_transpose(uint32_t& a0, uint32_t& a1, uint32_t& a2, uint32_t& a3) {
    const uint32_t u0 = rs_perm(a1, a0, 0x05010400u);          // a0.0 a1.0 a0.1 a1.1
    const uint32_t u1 = rs_perm(a1, a0, 0x07030602u);          // a0.2 a1.2 a0.3 a1.3
    const uint32_t u2 = rs_perm(a3, a2, 0x05010400u);
    const uint32_t u3 = rs_perm(a3, a2, 0x07030602u);
    a0 = rs_perm(u2, u0, 0x05040100u);                         // a0.0 a1.0 a2.0 a3.0
    a1 = rs_perm(u2, u0, 0x07060302u);
    a2 = rs_perm(u3, u1, 0x05040100u);
    a3 = rs_perm(u3, u1, 0x07060302u);
}

// lo[s] = bytes b0 .. b3 (bits 7 .. 4) and hi[s] = bytes b4 .. b7 (bits 3 .. 0) of symbol s, each byte 0 or 1
// -> the four symbols, symbol s in byte s
RS_HD uint32_t rs_pack(uint32_t l0, uint32_t l1, uint32_t l2, uint32_t l3, uint32_t h0, uint32_t h1, uint32_t h2,
                       uint32_t h3) {
    rs_transpose(l0, l1, l2, l3);                              // l_p: byte s = bit 7 - p of symbol s
    rs_transpose(h0, h1, h2, h3);                              // h_p: byte s = bit 3 - p of symbol s
    return (l0 << 7) | (l1 << 6) | (l2 << 5) | (l3 << 4) | (h0 << 3) | (h1 << 2) | (h2 << 1) | h3;
}
RS_HD void rs_unpack(uint32_t x, uint32_t& l0, uint32_t& l1, uint32_t& l2, uint32_t& l3, uint32_t& h0, uint32_t& h1,
                     uint32_t& h2, uint32_t& h3) {
    const uint32_t one = 0x01010101u;
    l0 = (x >> 7) & one; l1 = (x >> 6) & one; l2 = (x >> 5) & one; l3 = (x >> 4) & one;
    h0 = (x >> 3) & one; h1 = (x >> 2) & one; h2 = (x >> 1) & one; h3 = x & one;
    rs_transpose(l0, l1, l2, l3);
    rs_transpose(h0, h1, h2, h3);
}

// four symbols times x
RS_HD uint32_t rs_xtime(uint32_t d) {
    const uint32_t top = (d >> 7) & 0x01010101u;
    return ((d & 0x7f7f7f7fu) << 1) ^ (((top << 8) - top) & 0x1d1d1d1du);
}
