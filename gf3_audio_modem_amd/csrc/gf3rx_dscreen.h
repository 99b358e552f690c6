// QPSK demodulation, screened: the data-symbol transforms of demod_kernel<.., MODE_QPSK> in fp32 with a proven bound, the
// sign decisions taken only where the bound backs them -- the demodulator's counterpart of gf3rx_fscreen.h.
//
// What MODE_QPSK hands the caller from a data symbol is two sign bits per carrier: the signs of Re and Im of
//   ep = (2 X[n]) conj(g),   X = rfft of the symbol's N samples,  g = the channel model's unit phasor of that carrier
// (the transforms leave 2 X in the slots: rfft_regs<.., TWICE>).  On a usable signal those parts sit four to five orders
// above the rounding of an fp32 transform.  demod_screen_kernel is demod_kernel with
//   * the pilot stage UNTOUCHED, in fp64: time-domain pilot sums, two fp64 transforms, Hs, He, the fit-range angles, the
//     unwrap corrections (discontinuous in the angles: nothing of this may move to fp32), slope and the start-up rotations.
//     Hs, He, slope, g_0 and gstep are the fp64 kernel's, bit for bit;
//   * each data symbol converted to fp32 (exact for f32 / i16 / u8 storage; f64 storage is never screened), transformed by
//     the same passes with the same Spec<NC> slot map on float2 points (rfft_regs<.., float2>: one source, gf3rx_device.h;
//     twiddles = the context's fp64 tables rounded once), rotated by the phasor of the fp32 recurrence g32 <- g32 s32
//     started from g_0 and gstep rounded once ("The rotation" below): ep32 = X32 conj(g32);
//     The data symbols go through the passes two at a time, as the halves of one cf2 point (gf3rx_device.h): the twiddles are
//     computed once and applied to both halves, and per half the sequence of operations is the float2 instantiation's, so
//     the bound below applies to each half unchanged, with that half's own l1 norm (an odd last symbol's partner is zeros);
//   * per symbol l the bound E_l >= |2 X32[n] - 2 X[n]| for EVERY bin n, from the symbol's l1 norm (accumulated while the
//     samples are converted; the per-wave sums ride on the transform's own barriers);
//   * a part of a DATA carrier is SAFE when  |part| > E_l + C_l u (|ep32.x| + |ep32.y|)  (written so that NaN fails; +-0,
//     NaN and Inf are never safe).  A safe part has the sign of the exact value, hence of the fp64 kernel's (whose own
//     rounding, ~1e-15 relative to |x|_1, is eleven orders inside the margin taken below); both parts being non-zero and
//     finite there, the fp64 kernel's label is the two sign bits too (qpsk_sign_rule's common case);
//   * a packet with any unsafe part in any data symbol, a non-finite E_l or a non-finite end-pilot estimate (which the sign
//     mode would otherwise see only through the fit's angles) is appended to a list (atomicAdd on a count,
//     then the packet number -- as corr_screen_kernel does), and demod_listed_kernel -- the fp64 kernel, same code
//     path for everything but where its packet number comes from -- runs on the listed packets and overwrites their rows.
//     No decision rests on an fp32 value that the bound does not back.
// Ragged packets do what demod_kernel does (zero row, status bit) and are not listed.
//
// The bound.  u = 2^-24 (fp32 unit roundoff).  z[m] = x[2m] + i x[2m+1], so sum|z[m]| <= |x|_1.  Every stage computes
// outputs y_i = sum_j a_ij x_j with |a_ij| = 1 (a twiddle power times a DFT-matrix entry) as sum_j a_ij (1 + eta_ij) x_j,
// |eta_ij| <= eps of that stage, so through all the stages every bin of the complex transform obeys
//   |Z32[k] - Z[k]| <= (prod (1 + eps_p) - 1) sum|z|  <~  (sum_p eps_p) |x|_1 :
// the componentwise bound of an FFT, each output a log-depth sum of NC terms z[m] w.  (An l2 bound on ONE bin would cost a
// factor sqrt(N), hence l1.)  The stages, in units of u:
//   twiddle powers.  A table twiddle is cos / sin rounded from fp64 to fp32: absolute error d <= u/2 per part (values <= 1).
//     The powers w^2 .. w^(R-1) come from the three-term recurrence w^(k+1) = 2 cos(t) w^k - w^(k-1) started at (1, w~):
//     its exact solution for the rounded start is (T_k(c~), w~.y U_(k-1)(c~)), which differs from (cos kt, -sin kt) by at
//     most k^2 d in the real part (|T_k'| <= k^2) and (k + k (k^2 - 1) / 3) d in the imaginary part (the rounding of w~.y
//     times |U_(k-1)| <= k, plus |U_(k-1)'| <= k (k^2 - 1) / 3 times d); each step adds one fma rounding <= u per part,
//     which the recurrence carries on with weight |U_m| <= m + 1: sum_(m=1..k-1) m u.
//       radix 8 (k <= 7): real (24.5 + 21) u, imaginary (59.5 + 21) u, modulus <= 93 u  -> tau_8 = 96 u
//       radix 4 (k <= 3): real (4.5 + 3) u,  imaginary (5.5 + 3) u,   modulus <= 12 u  -> tau_4 = 12 u
//   bfly8 (first pass, no twiddles): three levels of additions, u each (componentwise, so u in modulus); the odd outputs'
//     1/sqrt2 rides on an fma: the sum p = re + im (sqrt2 u of the operand's modulus), the rounded constant (u/2), the fma
//     (u): <= 5 u; taken as 8 u.
//   bfly8_tw: the twiddle products (complex fma: two roundings per part; 2u - s reuses a rounded sum: <= 3 u of the two
//     operands), a complex multiply ahead of a complex fma (<= 6 u together), one plain level (u), the 1/sqrt2 level (3 u):
//     <= 10 u; taken as 16 u, plus tau_8:   eps = 112 u.
//   bfly4_tw: the same without the third level: <= 7 u; taken as 12 u, plus tau_4:   eps = 24 u.
//   packed-real split, TWICE: 2 X[k] = Z[k] (1 - i w) + conj(Z[NC-k]) (1 + i w), and |1 - i w| + |1 + i w| <= 2 sqrt2 for
//     |w| = 1, so the errors of the complex transform reach 2 X with weight 2 sqrt2; the split's own twiddle (the table
//     value, for r > 0 times a rounded constant: <= 4 u), two additions, a complex fma and 2E - X: <= 10 u, taken as 16 u.
//     TWICE drops the two halvings, which are exact anyway.
//   passes per size (rfft_regs never takes fft_pass's second-butterfly twiddle step: its radix-4 passes on the fused sizes
//   read both butterflies' twiddles from the table):
//     NC =  512: bfly8, bfly8_tw, bfly8_tw, split            8 + 2 x 112 + 16       = 248 u
//     NC = 1024: bfly8, bfly8_tw, bfly4_tw, bfly4_tw, split  8 + 112 + 2 x 24 + 16  = 184 u
//     NC = 2048: bfly8, bfly8_tw, bfly8_tw, bfly4_tw, split  8 + 2 x 112 + 24 + 16  = 272 u
//     NC = 4096: bfly8, 3 x bfly8_tw, split                  8 + 3 x 112 + 16       = 360 u
//   GAMMA(NC) = SAFETY x 2 sqrt2 x that sum, SAFETY = 2 (the second-order terms of the product are < 1e-4 of the sum; the
//   factor is there for what a derivation by hand may have missed):  1403 u, 1041 u, 1539 u, 2037 u.
//   E_l = GAMMA |x_l|_1 (1 + 1e-3) + 1e-30.  The 1e-3 covers the fp32 summation of |x|_1 (16 terms per thread, six
//   cross-lane steps, <= 8 per-wave sums: < 40 u relative) a hundred times over; the absolute term covers results that
//   underflow (a signal whose parts are below 1e-30 is listed, i.e. demodulated in fp64).
// The rotation.  The start-up rotations are the fp64 kernel's (g_0 = u r0 and gstep from the rotation tables); then g_0 and
// gstep are rounded to fp32 ONCE and the recurrence runs in fp32: g32_0 = fl(g_0), s32 = fl(gstep), g32_(l+1) =
// fl(g32_l s32).  g is not an output: it is used once per symbol, by the product below, which rounded it to fp32 anyway.
// With G_l = g_0 gstep^l the exact recurrence on the fp64 start values (the fp64 kernel's own g_l differs from it by
// ~ 4 l 2^-53, |G_l| from 1 by as little: nine orders inside what follows) and e_l = |g32_l - G_l|:
//   rounding of the start values: componentwise relative u, so |g32_0 - g_0| <= u and |s32 - gstep| <= u, |s32| <= 1 + u
//     (a part that underflows is off by 2^-126 at the most: nothing next to u);
//   one complex multiply a b, each part a product rounded or kept exact inside an fma (whichever the compiler contracts)
//     and a final rounding: the rounded products form a vector of modulus <= sqrt2 u |a| |b|, the final roundings one of
//     u |a b|: rho <= (1 + sqrt2) u |a| |b| (1 + u) < 2.42 u |a| |b|;
//   g32_l s32 - G_l gstep = (g32_l - G_l) s32 + G_l (s32 - gstep), |g32_l| <= 1 + e_l:
//     e_(l+1) <= e_l (1 + u) + u + 2.42 u (1 + u) (1 + e_l)  <=  e_l (1 + 3.5 u) + 3.5 u,   e_0 <= u,
//     so 1 + e_l <= exp(3.5 u (l + 1)): 3.5 u per step to first order, modulus drift included (e_l is a vector error).
// The product ep32 = fl(X32 conj(g32_l)): |ep32 - X32 conj(g_l)| <= |X32| e_l + 2.42 u |X32| |g32_l|, and
// |X32| |g32_l| <= |ep32| (1 + 2.5 u), |g32_l| >= 1 - e_l, so with x = 3.5 u (l + 1)
//     |ep32 - X32 conj(g_l)| <= (2.43 u + (e^x - 1) / (2 - e^x)) |ep32|,   |ep32| <= |ep32.x| + |ep32.y|.
// C_l = 8 + 8 (l + 1): the constant term as before (2.43 u against 8 u), the per-step term the derived 3.5 u doubled and
// rounded up.  It holds for ANY number of data symbols: both parts of a carrier can only be safe while C_l u < 1/2 (add the
// two conditions |part| > C_l u (|ep32.x| + |ep32.y|)), i.e. while x < 3.5 / 16 = 0.22, and there (e^x - 1) / (2 - e^x) <=
// 1.48 x against the 16 x / 7 = 2.29 x that C_l grants; for l + 1 <= 2^17 the exponential is within 1.5 % of x and the
// whole factor of two is spare.  Beyond l + 1 = 2^20 nothing is safe and every packet is listed (such packets take the
// two-phase form anyway, which is never screened).  Mode A2 (D = 180): C_l <= 1448, C_l u <= 8.7e-5 of |ep32.x| +
// |ep32.y|, against E_l at about 1/230 = 4.3e-3 of a part: a twenty-fifth of the threshold at the last symbol.
// tests/test_demod_screen_gpu.py holds max|ep32 - ep64| of every symbol to HALF of E_l on clean, noisy, DC-biased,
// full-scale int16, one-dominant-carrier and impulse inputs (the last drives |x|_1 down and the l1 bound to its tightest)
// at D = 8; tests/test_demod_pairs_gpu.py holds every carrier to half of E_l + C_l u (|ep32.x| + |ep32.y|) at D = 180;
// what is realised is in DESIGN 3.5.
//
// Cost of the bound being loose: GAMMA |x|_1 ~ 1.2e-4 x 50 |x|_2 ~ 0.006 |x|_2 for an OFDM symbol, against parts of about
// 1.4 |x|_2 (2 X of a QPSK carrier): the threshold is about 1/230 of a part.  Nothing is listed on clean input or at 20 dB
// of SNR.  But a packet has tens of thousands of parts and one unsafe part lists it: at 10 dB (noise sigma ~ 0.32 of a part)
// most packets are listed, and the call costs the fp32 pass plus nearly a whole fp64 pass (measured).
#pragma once
#include "gf3rx_screen.h"

#define GF3_DSCR_U 5.9604645e-8f            /* 2^-24 */
#define GF3_DSCR_SAFETY 2.0f
#define GF3_DSCR_C 8.0f                     /* the rotation's constant term ... */
#define GF3_DSCR_C_STEP 8.0f                /* ... and what every step of the fp32 phasor recurrence adds to it */
// sum of the stage constants above, in units of u
constexpr float dscr_stage_sum(int NC) {
    return NC == 512 ? 248.0f : (NC == 1024 ? 184.0f : (NC == 2048 ? 272.0f : 360.0f));
}
constexpr float dscr_gamma(int NC) { return GF3_DSCR_SAFETY * 2.8284272f * dscr_stage_sum(NC) * GF3_DSCR_U; }

// E_l from the symbol's l1 norm (the same value in every thread)
template <int NC> GF3_DEV float dscr_bound(float l1) { return fmaf(l1, dscr_gamma(NC) * 1.001f, 1e-30f); }

// C_l u for data symbol l (counted from the packet's first): the same value in every thread
GF3_DEV float dscr_rot(int l) { return (GF3_DSCR_C + GF3_DSCR_C_STEP * (float)(l + 1)) * GF3_DSCR_U; }

// One slot of one data symbol: rotate, take the sign bits, say whether the bound backs both of them.
GF3_DEV uint32_t dscr_decide(cf X, cf g, float El, float Clu, cf& ep, bool& safe) {
    ep = cmul_conj(X, g);
    const float ax = fabsf(ep.x), ay = fabsf(ep.y);
    const float thr = fmaf(Clu, ax + ay, El);
    safe = (ax > thr) && (ay > thr);                                       // (NaN fails both)
    return ((__float_as_uint(ep.y) >> 31) << 1) | (__float_as_uint(ep.x) >> 31);
}
