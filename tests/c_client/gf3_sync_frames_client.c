/*
 * A plain C99 caller of the frames-mode sync as a C client meets it: gf3_sync_frames, no workspace, no mode -- the library
 * chooses the evaluation and owns what it needs (include/gf3rx.h).
 *
 *   gf3_sync_frames_client <case.bin> <starts_out.bin> <W> <lo_0> [<lo_1> ...]
 *
 * case.bin: the file of gf3_c_client.c (tests/test_c_client.py writes it).  One call per <lo_i>, all on the default
 * stream: one window of W lags whose first lag is sample lo_i.  starts_out.bin: int64 count, then per call the start the
 * library found and the path gf3_sync_frames_last reports for it (int64 each).
 * Exit code 0 on success; 2 + the gf3_status on a library error (message on stderr).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "gf3rx.h"

#define HIPOK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)
#define GF3OK(x) do { int rc_ = (x); if (rc_ != GF3_OK) { fprintf(stderr, "%s: %d %s\n", #x, rc_, gf3_last_error(NULL)); return 2 - rc_; } } while (0)

static int rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n ? 0 : 1; }

int main(int argc, char** argv) {
    if (argc < 5) { fprintf(stderr, "usage: %s case.bin starts_out.bin W lo_0 [lo_1 ...]\n", argv[0]); return 64; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 65; }
    int32_t h[12];
    double fl[4];
    int32_t fit[2];
    if (rd(f, h, sizeof h) || rd(f, fl, sizeof fl) || rd(f, fit, sizeof fit)) return 66;
    const int N = h[0], mu = h[5], M = h[6], C = h[7], K = N / 2 - 1;
    const int64_t n = (int64_t)(uint32_t)h[9] | ((int64_t)h[10] << 32);
    const int esz = h[8] == GF3_F64 ? 8 : (h[8] == GF3_F32 ? 4 : (h[8] == GF3_I16 ? 2 : 1));
    double* cre = malloc(sizeof(double) * M); double* cim = malloc(sizeof(double) * M);
    uint8_t* cbits = malloc((size_t)M * mu);
    double* kre = malloc(sizeof(double) * K); double* kim = malloc(sizeof(double) * K);
    int32_t* bins = malloc(sizeof(int32_t) * C);
    uint8_t* mask = malloc((size_t)C * mu);
    void* samples = malloc((size_t)n * esz);
    if (rd(f, cre, sizeof(double) * M) || rd(f, cim, sizeof(double) * M) || rd(f, cbits, (size_t)M * mu) || rd(f, kre, sizeof(double) * K) ||
        rd(f, kim, sizeof(double) * K) || rd(f, bins, sizeof(int32_t) * C) || rd(f, mask, (size_t)C * mu) || rd(f, samples, (size_t)n * esz)) return 67;
    fclose(f);

    const int32_t W = (int32_t)atol(argv[3]);
    const int calls = argc - 4;
    gf3_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.N = N; cfg.CP = h[1]; cfg.P = h[2]; cfg.D = h[3]; cfg.Lc = h[4]; cfg.mu = mu; cfg.M = M; cfg.C = C; cfg.in_dtype = h[8];
    cfg.fs = fl[0]; cfg.f0 = fl[1]; cfg.f1 = fl[2]; cfg.thresh = fl[3]; cfg.fit_lo = fit[0]; cfg.fit_hi = fit[1];
    cfg.const_re = cre; cfg.const_im = cim; cfg.const_bits = cbits; cfg.known_re = kre; cfg.known_im = kim; cfg.data_bins = bins;
    cfg.max_window = W;
    gf3_ctx* ctx = NULL;
    GF3OK(gf3_ctx_create(&cfg, &ctx));

    void* d_r = NULL;
    int64_t* d_starts = NULL;
    HIPOK(hipMalloc(&d_r, (size_t)n * esz));
    HIPOK(hipMemcpy(d_r, samples, (size_t)n * esz, hipMemcpyHostToDevice));
    HIPOK(hipMalloc((void**)&d_starts, sizeof(int64_t) * (size_t)calls));
    int64_t* out = malloc(sizeof(int64_t) * (size_t)(1 + 2 * calls));
    int64_t* starts = malloc(sizeof(int64_t) * (size_t)calls);
    out[0] = 2 * calls;
    for (int i = 0; i < calls; ++i) {
        const int32_t lo = (int32_t)atol(argv[4 + i]);
        int32_t path = -1, cap = -1;
        GF3OK(gf3_sync_frames(ctx, d_r, n, 1, 0, lo, lo + W, d_starts + i, NULL, NULL));
        GF3OK(gf3_sync_frames_last(ctx, NULL, &path, &cap));
        out[1 + 2 * i + 1] = path;
    }
    HIPOK(hipDeviceSynchronize());
    HIPOK(hipMemcpy(starts, d_starts, sizeof(int64_t) * (size_t)calls, hipMemcpyDeviceToHost));
    for (int i = 0; i < calls; ++i) out[1 + 2 * i] = starts[i];

    FILE* g = fopen(argv[2], "wb");
    if (!g) { perror(argv[2]); return 68; }
    fwrite(out, sizeof(int64_t), (size_t)(1 + 2 * calls), g);
    fclose(g);
    printf("gf3_sync_frames_client: library %s, %lld samples, %d windows of %d lags\n", gf3_version(), (long long)n, calls, (int)W);
    gf3_ctx_destroy(ctx);
    HIPOK(hipFree(d_r));
    HIPOK(hipFree(d_starts));
    return 0;
}
