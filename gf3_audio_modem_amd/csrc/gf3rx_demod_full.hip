// libgf3rx -- demod_kernel<.., MODE_FULL>: bits + the dumps (eq, Hest); also the spectra-input form behind gf3_equalise.
#include "gf3rx_demod.h"

hipError_t launch_demod_full(const gf3_ctx* c, const DemodArgs& a, int64_t F, hipStream_t st) {
    hipError_t e = hipSuccess;
    DISPATCH_NC(c->NC, a.dt, e = launch((demod_kernel<NCC, DTC, false, MODE_FULL>), F, NCC / 8, demod_lds_bytes(c, false), st, a));
    return e;
}

// receiver.equalise as a stand-alone stage: frequency-domain inputs (complex128), everything else as above
hipError_t launch_demod_spectra(const gf3_ctx* c, const DemodArgs& a, int64_t F, hipStream_t st) {
    hipError_t e = hipSuccess;
    DISPATCH_NC_F64(c->NC, e = launch((demod_kernel<NCC, DT_F64, true, MODE_FULL>), F, NCC / 8, demod_lds_bytes(c), st, a));
    return e;
}
