// libgf3rx -- the context: error text, gf3_ctx_create / gf3_ctx_destroy with the constellation classification and the
// plans built at creation (correlation plans, the known pilot symbol, the two screening plans of gf3rx_plans.h), and the
// small getters.  Every device allocation that lives as long as the context is entered in c->owned and freed from it.
#include "gf3rx_plans.h"

// message of the calling thread's last failure (one buffer per host thread: gf3rx_host.h)
static thread_local char g_err[512] = "";
int fail(const gf3_ctx*, int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
extern "C" const char* gf3_last_error(const gf3_ctx*) { return g_err; }
extern "C" int gf3_clear_runtime_error(void) { return (int)hipGetLastError(); }

// Device memory made at set-up: allocated, filled from `h` when given, and entered in `owner`, which frees it -- c->owned
// (gf3_ctx_destroy, also on the failure paths of gf3_ctx_create), or a DevTmp for scratch that must go on every return path.
struct DevTmp { std::vector<void*> p; ~DevTmp() { for (void* q : p) (void)hipFree(q); } };
template <typename T> static hipError_t dev_new(std::vector<void*>& owner, T** out, size_t bytes, const void* h = nullptr) {
    hipError_t e = hipMalloc((void**)out, bytes);
    if (e != hipSuccess) return e;
    owner.push_back((void*)*out);
    return h ? hipMemcpy((void*)*out, h, bytes, hipMemcpyHostToDevice) : hipSuccess;
}
template <typename T, typename V> static hipError_t dev_new(std::vector<void*>& owner, T** out, const std::vector<V>& h) {
    return dev_new(owner, out, h.size() * sizeof(V), h.data());
}

// spectra of the zero-padded chirp partitions, computed with the engine's own FFT
static int build_plan(gf3_ctx* c, CorrPlan* pl, int NCp, FftTables t, int Lp_max) {
    const int N = 2 * NCp;
    pl->NC = NCp; pl->t = t;
    int Q = (c->Lc + Lp_max - 1) / Lp_max;
    int Lp = (c->Lc + Q - 1) / Q;
    pl->Q = Q; pl->Lp = Lp; pl->W = N - Lp + 1;
    std::vector<double> h((size_t)Q * N, 0.0);
    for (int q = 0; q < Q; ++q)
        for (int k = 0; k < Lp && q * Lp + k < c->Lc; ++k) h[(size_t)q * N + k] = c->chirp[(size_t)q * Lp + k];
    std::vector<int64_t> off(Q);
    for (int q = 0; q < Q; ++q) off[q] = (int64_t)q * N;
    double* d_h = nullptr; int64_t* d_off = nullptr;
    DevTmp tmp;                                        // frees d_h, d_off on every path out of here
    HIPCHK(c, dev_new(tmp.p, &d_h, h));
    HIPCHK(c, dev_new(tmp.p, &d_off, off));
    HIPCHK(c, dev_new(c->owned, &pl->d_Hq, (size_t)Q * (NCp + 1) * sizeof(cplx)));
    HIPCHK(c, run_rfft_nc(NCp, t, d_h, (int64_t)h.size(), DT_F64, d_off, Q, pl->d_Hq, 0));
    HIPCHK(c, hipStreamSynchronize(0));
    return GF3_OK;
}

// Known pilot symbol in the time domain (with prefix, before the x2 gain), built once at context
// creation with the transmit kernel itself: a one-symbol packet whose "filler" is the known-symbol
// vector and which has no data carriers.
static int build_known_time(gf3_ctx* c) {
    const gf3_config& g = c->cfg;
    TxArgs a{};
    a.t = {c->d_tw, c->d_twn};
    a.CP = g.CP; a.S = c->S; a.K = c->K; a.mu = g.mu; a.M = g.M; a.Lc = c->Lc;
    a.cre = c->d_cre; a.cim = c->d_cim; a.idx_of_label = c->d_idx_of_label; a.chirp = c->d_chirp;
    cplx* d_kn = nullptr; double* d_row = nullptr; int* d_nopos = nullptr; uint8_t* d_nobits = nullptr;
    std::vector<int> nopos(c->K, -1);
    const int64_t rowlen = c->Lc + c->S;
    DevTmp tmp;                                        // frees the four scratch buffers on every path out of here
    HIPCHK(c, dev_new(tmp.p, &d_kn, c->known_pts));
    HIPCHK(c, dev_new(tmp.p, &d_nopos, nopos));
    HIPCHK(c, dev_new(tmp.p, &d_row, (size_t)rowlen * sizeof(double)));
    HIPCHK(c, dev_new(tmp.p, &d_nobits, (size_t)16));
    HIPCHK(c, dev_new(c->owned, &c->d_known_time, c->S * sizeof(double)));
    HIPCHK(c, hipMemset(c->d_known_time, 0, c->S * sizeof(double)));
    a.P = 0; a.D = 1; a.C = 0; a.pos = d_nopos; a.contig_lo = 0; a.filler = d_kn; a.known_time = c->d_known_time;
    a.bits = d_nobits; a.row_bytes = 0; a.gaps = nullptr; a.out = d_row; a.stride = rowlen; a.out_dt = DT_F64;
    a.gain2 = 2.0;
    int rc = tx_launch(c, a, 1, 0);
    if (rc != GF3_OK) return rc;
    HIPCHK(c, hipStreamSynchronize(0));
    std::vector<double> h(c->S);
    HIPCHK(c, hipMemcpy(h.data(), d_row + c->Lc, c->S * sizeof(double), hipMemcpyDeviceToHost));
    for (auto& x : h) x *= 0.5;                          // stored before the x2 gain
    HIPCHK(c, hipMemcpy(c->d_known_time, h.data(), c->S * sizeof(double), hipMemcpyHostToDevice));
    return GF3_OK;
}

// The two screening plans: computed on the host (gf3rx_plans.h), uploaded here.  D: gf3_ctx::scr or gf3_ctx::fscr.
template <typename D> static int upload_screen_plan(gf3_ctx* c, D& d, const ScreenPlanHost& p) {
    d.Q = p.Q;
    HIPCHK(c, dev_new(c->owned, &d.d_tw, p.tw.tw));
    HIPCHK(c, dev_new(c->owned, &d.d_twn, p.tw.twn));
    HIPCHK(c, dev_new(c->owned, &d.d_Hs, p.Hs));
    HIPCHK(c, dev_new(c->owned, &d.d_H0N, p.H0N));
    HIPCHK(c, dev_new(c->owned, &d.d_Hinf, p.Hinf));
    d.ok = true;
    return GF3_OK;
}
static int build_screen_plan(gf3_ctx* c) {
    auto& sp = c->scr;
    const ScreenPlanHost p = screen_plan_host(c->chirp);
    if (!p.ok) return GF3_OK;
    sp.H = p.L; sp.ring = p.ring;
#ifdef GF3_DEV_BUILD
    if (const char* e = getenv("GF3_SCR_R")) sp.R_forced = atoi(e);       // (tuning aid of developer builds only: output blocks per workgroup)
#endif
    HIPCHK(c, dev_new(c->owned, &sp.d_Hb, p.Hb));
    HIPCHK(c, dev_new(c->owned, &sp.d_ecoef, p.ecoef));
    return upload_screen_plan(c, sp, p);
}
static int build_fscreen_plan(gf3_ctx* c, int wmax) {
    const ScreenPlanHost p = fscreen_plan_host(c->chirp, wmax);
    if (!p.ok) return GF3_OK;
    c->fscr.Lp = p.L; c->fscr.wmax = wmax;
    return upload_screen_plan(c, c->fscr, p);
}

// Twiddle set for a plan's FFT size: the context's own, or one of two extra sets made on first use.
static bool fft_tables(gf3_ctx* c, int NCp, FftTables& t) {
    if (NCp == c->NC) { t = FftTables{c->d_tw, c->d_twn}; return true; }
    for (int i = 0; i < 2; ++i) if (c->nc_x[i] == NCp) { t = FftTables{c->d_tw_x[i], c->d_twn_x[i]}; return true; }
    const int i = c->nc_x[0] ? 1 : 0;
    const Twiddles<cplx> h = make_twiddles<cplx>(NCp, NCp / 2 + 1);
    if (dev_new(c->owned, &c->d_tw_x[i], h.tw) != hipSuccess || dev_new(c->owned, &c->d_twn_x[i], h.twn) != hipSuccess) return false;
    c->nc_x[i] = NCp;
    t = FftTables{c->d_tw_x[i], c->d_twn_x[i]};
    return true;
}

// Which fast paths a constellation table may take (tests/tables.py::classify restates these rules).  clab[m]: the label of
// point m as an integer, first bit most significant.
struct TableClass { SepTab sep; UniGrid ug; double qpsk_q; };
static TableClass classify_table(const gf3_config& cfg, const std::vector<int>& clab) {
    TableClass r{};
    SepTab& sp = r.sep;
    UniGrid& ug = r.ug;
    // separable grid? distinct re / im levels, full grid, every label bit a function of one axis only
    std::vector<double> li, lq;
    auto find = [](std::vector<double>& v, double x) { for (size_t i = 0; i < v.size(); ++i) if (v[i] == x) return (int)i; v.push_back(x); return (int)v.size() - 1; };
    std::vector<int> ai(cfg.M), aq(cfg.M);
    for (int m = 0; m < cfg.M; ++m) { ai[m] = find(li, cfg.const_re[m]); aq[m] = find(lq, cfg.const_im[m]); }
    bool ok = li.size() <= 8 && lq.size() <= 8 && (int)(li.size() * lq.size()) == cfg.M;
    std::vector<int> seen(64, 0);
    for (int m = 0; ok && m < cfg.M; ++m) { int& sflag = seen[ai[m] * 8 + aq[m]]; if (sflag) ok = false; sflag = 1; }
    int maskI = 0, maskQ = 0;
    for (int b = 0; ok && b < cfg.mu; ++b) {
        const int bit = 1 << (cfg.mu - 1 - b);
        bool byI = true, byQ = true;
        std::vector<int> vi(8, -1), vq(8, -1);
        for (int m = 0; m < cfg.M; ++m) {
            const int v = (clab[m] & bit) ? 1 : 0;
            if (vi[ai[m]] < 0) vi[ai[m]] = v; else if (vi[ai[m]] != v) byI = false;
            if (vq[aq[m]] < 0) vq[aq[m]] = v; else if (vq[aq[m]] != v) byQ = false;
        }
        if (byI) maskI |= bit; else if (byQ) maskQ |= bit; else ok = false;
    }
    if (ok) {
        sp.nI = (int)li.size(); sp.nQ = (int)lq.size(); sp.maskI = maskI;
        for (int m = 0; m < cfg.M; ++m) {
            sp.lvI[ai[m]] = cfg.const_re[m]; sp.labI[ai[m]] = clab[m] & maskI;
            sp.lvQ[aq[m]] = cfg.const_im[m]; sp.labQ[aq[m]] = clab[m] & maskQ;
        }
    }
    // equally spaced levels on both axes?  (sorted ascending; spacing equal to 1e-12 relative)
    auto axis = [](const double* lv, const int* lab, int n, double& lo, double& inv, unsigned long long& pack) -> bool {
        if (n < 2 || n > 8) return false;
        int order[8];
        for (int i = 0; i < n; ++i) order[i] = i;
        for (int i = 0; i < n; ++i) for (int j = i + 1; j < n; ++j) if (lv[order[j]] < lv[order[i]]) { int t = order[i]; order[i] = order[j]; order[j] = t; }
        const double step = (lv[order[n - 1]] - lv[order[0]]) / (n - 1);
        if (!(step > 0.0)) return false;
        pack = 0;
        for (int i = 0; i < n; ++i) {
            if (fabs(lv[order[i]] - (lv[order[0]] + i * step)) > 1e-12 * step) return false;
            if (lab[order[i]] & ~0xff) return false;
            pack |= (unsigned long long)(lab[order[i]] & 0xff) << (8 * i);
        }
        lo = lv[order[0]]; inv = 1.0 / step;
        return true;
    };
    if (sp.nI > 0 && axis(sp.lvI, sp.labI, sp.nI, ug.loI, ug.invI, ug.packI) && axis(sp.lvQ, sp.labQ, sp.nQ, ug.loQ, ug.invQ, ug.packQ)) {
        ug.nI = sp.nI; ug.nQ = sp.nQ;
    } else ug.nI = ug.nQ = 0;
    // the reference's QPSK table (OFDM.py:72-77): (+,+)00 (+,-)10 (-,-)11 (-,+)01 with |re|=|im|
    if (cfg.M == 4 && cfg.mu == 2) {
        const double q = cfg.const_re[0];
        const double sr[4] = {1, 1, -1, -1}, si[4] = {1, -1, -1, 1};
        const int labs[4] = {0, 2, 3, 1};
        bool okq = q > 0.1 && q < 10.0;
        for (int m = 0; m < 4; ++m)
            okq = okq && cfg.const_re[m] == sr[m] * q && cfg.const_im[m] == si[m] * q && clab[m] == labs[m];
        r.qpsk_q = okq ? q : 0.0;
    }
    return r;
}

extern "C" int gf3_ctx_create(const gf3_config* cfg, gf3_ctx** out) {
    if (!cfg || !out) return fail(nullptr, GF3_EINVAL, "null argument");
    *out = nullptr;
    const int N = cfg->N;
    if (N != 1024 && N != 2048 && N != 4096 && N != 8192)
        return fail(nullptr, GF3_EINVAL, "N=%d unsupported (1024, 2048, 4096, 8192)", N);
    if (cfg->CP < 0 || cfg->P < 1 || cfg->D < 1) return fail(nullptr, GF3_EINVAL, "need CP>=0, P>=1, D>=1");
    if (cfg->M < 2 || cfg->M > 64 || cfg->mu < 1 || cfg->mu > 8 || (1 << cfg->mu) < cfg->M)
        return fail(nullptr, GF3_EINVAL, "Invalid Modulation Type (M=%d, mu=%d)", cfg->M, cfg->mu);
    if (!cfg->const_re || !cfg->const_im || !cfg->const_bits || !cfg->known_re || !cfg->known_im || !cfg->data_bins)
        return fail(nullptr, GF3_EINVAL, "null table pointer");
    if (cfg->in_dtype < 0 || cfg->in_dtype > 3) return fail(nullptr, GF3_EINVAL, "bad in_dtype");
#ifdef GF3_DEV_BUILD   /* developer iteration builds instantiate N = 4096 with f32 / f64 samples only: say so instead of launching the wrong kernel */
    if (N != 4096 || cfg->in_dtype > GF3_F32)
        return fail(nullptr, GF3_EINVAL, "developer build (-DGF3_DEV_BUILD): only N=4096 with f64 / f32 samples is instantiated (asked for N=%d, in_dtype=%d)", N, cfg->in_dtype);
#endif
    gf3_ctx* c = new gf3_ctx();
    c->cfg = *cfg;
    if (hipGetDevice(&c->device) != hipSuccess) { delete c; return fail(nullptr, GF3_EHIP, "hipGetDevice failed: no usable GPU"); }
    if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || c->n_cu < 1) c->n_cu = 256;
    c->NC = N / 2; c->K = N / 2 - 1; c->S = N + cfg->CP;
    c->Lc = cfg->Lc > 0 ? cfg->Lc : 5 * c->S;
    const int K = c->K;
    if (cfg->C < 1 || cfg->C > K) { delete c; return fail(nullptr, GF3_EINVAL, "C out of range"); }
    c->row_bytes = (int)(((int64_t)cfg->D * cfg->C * cfg->mu + 7) / 8);
    // polyfit range: python slice [fit_lo:fit_hi] of a length-K row (OFDM.py:462)
    c->fit_lo = cfg->fit_lo < K ? cfg->fit_lo : K;
    c->fit_hi = cfg->fit_hi < K ? cfg->fit_hi : K;
    const int L = c->fit_hi - c->fit_lo;
    if (L < 2) { delete c; return fail(nullptr, GF3_EINVAL, "phase-slope fit range [%d:%d] holds %d carriers (K=%d)", cfg->fit_lo, cfg->fit_hi, L, K); }
    c->xbar = 0.5 * (L - 1);
    { double sxx = 0; for (int i = 0; i < L; ++i) { const double d = i - c->xbar; sxx += d * d; } c->inv_sxx = 1.0 / sxx; }
    const int NC = c->NC;
    const Twiddles<cplx> tw = make_twiddles<cplx>(NC, NC / 2 + 1);
    std::vector<cplx> known(K);
    c->known_pts.resize(K);
    for (int k = 0; k < K; ++k) {                      // 1/known = conj(known)/|known|^2
        const long double re = cfg->known_re[k], im = cfg->known_im[k], d = re * re + im * im;
        known[k] = make_double2((double)(re / d), (double)(-im / d));
        c->known_pts[k] = make_double2(cfg->known_re[k], cfg->known_im[k]);
    }
    std::vector<int> pos(K, -1), clab(cfg->M);
    for (int i = 0; i < cfg->C; ++i) {
        const int b = cfg->data_bins[i];
        if (b < 1 || b > K || pos[b - 1] != -1) { delete c; return fail(nullptr, GF3_EINVAL, "data_bins[%d]=%d invalid or repeated", i, b); }
        pos[b - 1] = i;
    }
    bool contig = true;
    for (int i = 1; i < cfg->C; ++i) contig = contig && cfg->data_bins[i] == cfg->data_bins[0] + i;
    c->contig_lo = contig ? cfg->data_bins[0] : 0;
    for (int m = 0; m < cfg->M; ++m) {
        int lab = 0;
        for (int b = 0; b < cfg->mu; ++b) lab = (lab << 1) | (cfg->const_bits[m * cfg->mu + b] & 1);
        clab[m] = lab;
    }
    { const TableClass tc = classify_table(*cfg, clab); c->sep = tc.sep; c->ug = tc.ug; c->qpsk_q = tc.qpsk_q; }
    // chirp replica (sync_chirp, OFDM.py:106-109): linspace incl. endpoint, scipy linear chirp, /5
    c->chirp.resize(c->Lc);
    const double t1 = (double)c->Lc / cfg->fs;
    const double step = t1 / (double)(c->Lc - 1);
    const double beta = (cfg->f1 - cfg->f0) / t1;
    for (int i = 0; i < c->Lc; ++i) {
        const double t = (i == c->Lc - 1) ? t1 : (double)i * step;
        const double ph = 2 * M_PI * (cfg->f0 * t + 0.5 * beta * t * t);
        c->chirp[i] = cos(ph) / 5;
    }
    {   // the replica's sum and its centred energy Ec - Sc^2 / Lc (gf3_detect_chunk's normaliser)
        long double s = 0.0L, e = 0.0L;
        for (double v : c->chirp) { s += v; e += (long double)v * v; }
        c->chirp_sum = (double)s;
        c->chirp_var = (double)(e - s * s / c->Lc);
    }
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { int rc_ = fail(nullptr, GF3_EHIP, "%s: %s", #x, hipGetErrorString(e_)); gf3_ctx_destroy(c); return rc_; } } while (0)
    CK(dev_new(c->owned, &c->d_tw, tw.tw));
    CK(dev_new(c->owned, &c->d_twn, tw.twn));
    {
        std::vector<cf> tw32;                                           // the fp64 tables rounded once (gf3rx_dscreen.h)
        for (const cplx& w : tw.tw) tw32.push_back(make_float2((float)w.x, (float)w.y));
        for (const cplx& w : tw.twn) tw32.push_back(make_float2((float)w.x, (float)w.y));
        CK(dev_new(c->owned, &c->d_tw32, tw32));
    }
    CK(dev_new(c->owned, &c->d_known, known));
    CK(dev_new(c->owned, &c->d_pos, pos));
    {
        std::vector<int> rsv(K, -1);                                    // the carriers no data symbol uses, numbered in ascending order
        for (int k = 0; k < K; ++k) if (pos[k] < 0) rsv[k] = c->Ku++;
        CK(dev_new(c->owned, &c->d_rsv, rsv));
    }
    CK(dev_new(c->owned, &c->d_clab, clab));
    {
        const std::vector<int> bins(cfg->data_bins, cfg->data_bins + cfg->C);
        int64_t sum = 0;
        for (int b : bins) sum += b;
        c->bin_mean = (double)sum / (double)cfg->C;
        CK(dev_new(c->owned, &c->d_bins, bins));
        // the carriers in ascending bin order (bins are distinct): gf3_feedback_equalise's bin window is a range of it
        std::vector<int> order(cfg->C), sorted(cfg->C);
        for (int i = 0; i < cfg->C; ++i) order[i] = i;
        std::sort(order.begin(), order.end(), [&](int x, int y) { return bins[x] < bins[y]; });
        for (int i = 0; i < cfg->C; ++i) sorted[i] = bins[order[i]];
        CK(dev_new(c->owned, &c->d_bin_order, order));
        CK(dev_new(c->owned, &c->d_bins_sorted, sorted));
    }
    std::vector<int> inv(1 << cfg->mu, 0);
    for (int m = cfg->M - 1; m >= 0; --m) inv[clab[m]] = m;
    CK(dev_new(c->owned, &c->d_idx_of_label, inv));
    CK(dev_new(c->owned, &c->d_chirp, c->chirp));
    const int nst = (c->Lc + SCR_REF_WT - 1) / SCR_REF_WT;
    std::vector<double> tiled((size_t)nst * SCR_REF_WT, 0.0);
    for (int st = 0; st < nst; ++st)
        for (int q = 0; q < 8; ++q)
            for (int lane = 0; lane < 64; ++lane)
                for (int h = 0; h < 2; ++h) {
                    const int k = SCR_REF_WT * st + 16 * lane + 2 * q + h;
                    if (k < c->Lc) tiled[(((size_t)st * 8 + q) * 64 + lane) * 2 + h] = c->chirp[k];
                }
    CK(dev_new(c->owned, &c->d_chirp_t, tiled));
    CK(dev_new(c->owned, &c->d_cre, (size_t)cfg->M * sizeof(double), cfg->const_re));
    CK(dev_new(c->owned, &c->d_cim, (size_t)cfg->M * sizeof(double), cfg->const_im));
#undef CK
    // the tables are now device-resident; do not keep the caller's host pointers
    c->cfg.const_re = c->cfg.const_im = c->cfg.known_re = c->cfg.known_im = nullptr;
    c->cfg.const_bits = nullptr; c->cfg.data_bins = nullptr;
    int wmax = cfg->max_window > 0 ? cfg->max_window : 512;
    if (wmax > N / 2) wmax = N / 2;
    // frames-mode plan: (Q+1) transforms of size Nf per packet; pick Nf in {N, N/2} by cost ~ (Q+1) Nf log2 Nf
    int NCf = NC;
    if (NC >= 1024 && wmax <= NC / 2) {
        auto cost = [&](int nc) { const int nf = 2 * nc, lp = nf - wmax + 1; const int q = (c->Lc + lp - 1) / lp;
                                  return (double)(q + 1) * nf * log2((double)nf); };
        if (cost(NC / 2) < cost(NC)) NCf = NC / 2;
    }
    // stream-mode plan (spectral delay line, hop = partition length): FFT size 2N where the kernels exist --
    // half as many partitions, half the spectrum bytes per lag
    int NCs = NC;
#ifndef GF3_DEV_BUILD
    if (2 * NC <= 4096) NCs = 2 * NC;
#endif
    FftTables tf, ts;
    if (!fft_tables(c, NCf, tf) || !fft_tables(c, NCs, ts)) { gf3_ctx_destroy(c); return fail(nullptr, GF3_EHIP, "table upload failed"); }
    int rc = build_plan(c, &c->frames_plan, NCf, tf, 2 * NCf - wmax + 1);
    if (rc == GF3_OK) rc = build_plan(c, &c->stream_plan, NCs, ts, NCs);
    if (rc == GF3_OK) rc = build_known_time(c);
    if (rc == GF3_OK) rc = build_screen_plan(c);
    if (rc == GF3_OK) rc = build_fscreen_plan(c, wmax);
    if (rc != GF3_OK) { gf3_ctx_destroy(c); return rc; }
    *out = c;
    return GF3_OK;
}

extern "C" void gf3_ctx_destroy(gf3_ctx* c) {
    if (!c) return;
    DeviceGuard dg(c);
    for (void* p : c->owned) (void)hipFree(p);
    // the screened paths' list workspaces, current and outgrown: kernels queued by earlier calls may still read them
    if (!c->ws_work.empty() || !c->ws_retired.empty()) (void)hipDeviceSynchronize();
    for (auto& w : c->ws_work) for (void* p : w.d) if (p) (void)hipFree(p);
    for (void* p : c->ws_retired) if (p) (void)hipFree(p);
    delete c;
}

#define GF3_MAX_WORKSPACES 64
// An outgrown buffer is retired, not freed: a queued kernel may still read it.
void* ctx_workspace(gf3_ctx* c, hipStream_t st, int slot, int64_t bytes) {
    const std::thread::id me = std::this_thread::get_id();
    std::lock_guard<std::mutex> lock(c->ws_mu);
    gf3_ctx::Work* e = nullptr;
    for (auto& w : c->ws_work) if (w.stream == st && w.thread == me) { e = &w; break; }
    if (e && e->d[slot] && e->bytes[slot] >= bytes) return e->d[slot];
    if (!e && c->ws_work.size() >= GF3_MAX_WORKSPACES) return nullptr;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (cap != hipStreamCaptureStatusNone) return nullptr;               // an allocation would break the capture
    int64_t want = bytes;
    if (e && want < e->bytes[slot] + e->bytes[slot] / 2) want = e->bytes[slot] + e->bytes[slot] / 2;   // (a slowly growing F: few retired buffers)
    void* d = nullptr;
    if (hipMalloc(&d, (size_t)want) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (!e) { c->ws_work.push_back(gf3_ctx::Work{st, me}); e = &c->ws_work.back(); }
    if (e->d[slot]) c->ws_retired.push_back(e->d[slot]);
    e->d[slot] = d; e->bytes[slot] = want;
    return d;
}

// diagnostic builds only: device buffer [F][8] of uint64 that receives per-phase s_memtime stamps
extern "C" void gf3_debug_set_stamps(gf3_ctx* c, void* d_buf) { if (c) c->stamps = (unsigned long long*)d_buf; }

extern "C" int32_t gf3_bytes_per_frame(const gf3_ctx* c) { return c ? c->row_bytes : 0; }
extern "C" int32_t gf3_sync_max_window(const gf3_ctx* c) { return c ? c->frames_plan.W : 0; }

extern "C" int gf3_chirp_replica(const gf3_ctx* c, double* h_out) {
    if (!c || !h_out) return fail(c, GF3_EINVAL, "null argument");
    memcpy(h_out, c->chirp.data(), c->chirp.size() * sizeof(double));
    return GF3_OK;
}
