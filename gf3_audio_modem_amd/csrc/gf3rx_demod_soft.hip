// libgf3rx -- demod_kernel<.., MODE_SOFT>: samples to weighted max-log LLRs in one launch, any constellation, no bits.
#include "gf3rx_demod.h"

hipError_t launch_demod_soft(const gf3_ctx* c, const DemodArgs& a, int64_t F, hipStream_t st) {
    hipError_t e = hipSuccess;
    DISPATCH_NC(c->NC, a.dt, e = launch((demod_kernel<NCC, DTC, false, MODE_SOFT>), F, NCC / 8, demod_soft_lds_bytes(c), st, a));
    return e;
}
