// Host entry points of the analysis side: resampling, dataset statistics, silence trimming, YIN / pYIN pitch tracking, DTW, BS.1770 loudness,
// STOI / ESTOI, the STFT distance, voice quality, formants, perturbation, harmonic differences, contour functionals, auditory descriptors, formant tracks, SRMR, speech rate, the spectral envelope and the phase vocoder (kernels: ev_analysis_kernels.h).  Part of ev_engine.hip's translation unit: that file includes this one
// after ev_handle, fail / HIPCHK / enter, dev_upload, drop_owned, scratch_acquire and launch<>.  None of these calls runs on the engine's conv
// path; ev_load_mel_basis, ev_mel_spectrogram, ev_denoise and ev_stft_magnitude do, and stay in ev_engine.hip.
#pragma once

namespace {

// The checks these calls share.  `who` is the entry point's name (__func__), so every ev_last_error text names its call.
int check_batch(ev_handle* h, const char* who, int B) {
    return B < 1 || B > 65535 ? fail(h, "%s: B=%d outside 1 <= B <= 65535", who, B) : 0;
}
int check_hop(ev_handle* h, const char* who, int H) {
    return H < 64 || H > 4096 || H % 64 ? fail(h, "%s: hop_length=%d must be a multiple of 64 and at most 4096", who, H) : 0;
}
int check_frame_length(ev_handle* h, const char* who, int W) {
    return W < 64 || W > 4096 || W % 64 ? fail(h, "%s: frame_length=%d must be a multiple of 64 with 64 <= frame_length <= 4096", who, W) : 0;
}
int check_lag_range(ev_handle* h, const char* who, int tau_min, int tau_max) {
    return tau_min < 1 || tau_min > tau_max || tau_max > 2048
               ? fail(h, "%s: tau_min=%d tau_max=%d outside 1 <= tau_min <= tau_max <= 2048", who, tau_min, tau_max) : 0;
}
// every entry of a host table is finite
int check_finite(ev_handle* h, const char* who, const char* name, const double* v, int n) {
    for (int j = 0; j < n; ++j) if (!std::isfinite(v[j])) return fail(h, "%s: %s[%d] is not finite", who, name, j);
    return 0;
}
// ceil(L / H): the frames of a row of L samples at hop H
int frames_of(int L, int H) { return (int)(((long long)L + H - 1) / H); }
// the geometry of a windowed DFT as a GEMM (the float64 DFT GEMM kernels of ev_analysis_kernels.h)
int check_dft_geometry(ev_handle* h, const char* who, int W, int H, int nfft, int nfft_max) {
    if (nfft < 16 || nfft > nfft_max || nfft % 2) return fail(h, "%s: nfft=%d must be even with 16 <= nfft <= %d", who, nfft, nfft_max);
    if ((nfft - W) % 2) return fail(h, "%s: nfft - W = %d must be even (the window is padded centrally)", who, nfft - W);
    if (W < 4 || W > nfft || W % 4) return fail(h, "%s: W=%d must be a multiple of 4 with 4 <= W <= nfft = %d", who, W, nfft);
    if (H < 1 || H > 512) return fail(h, "%s: H=%d outside 1 <= H <= 512", who, H);
    return 0;
}

// The tables of a load that open with the windowed DFT basis: window and twiddles go to the device as temporaries, one block of `bytes` is allocated
// behind them, stft_dist_basis_kernel builds the (W, nfft / 2 + 1) basis at the head of the block, extra(block, d_tw) makes the caller's further copies
// and launches, and after ONE synchronisation the temporaries are freed.  Returns 0 with *blk the caller's to own; else the message is set (`what`:
// "basis" or "tables") and nothing is left allocated.  (extern "C++": ev_engine.hip includes this file inside extern "C", where no template may stand.)
extern "C++" template <typename Extra>
int build_dft_basis(ev_handle* h, const char* who, const char* what, const double* window, const double* twiddle, int W, int nfft, size_t bytes, char** blk, Extra extra) {
    const int NB = nfft / 2 + 1;
    double* d_win = nullptr; double* d_tw = nullptr;
    HIPCHK(h, hipMalloc((void**)&d_win, (size_t)W * sizeof(double)));
    if (hipMalloc((void**)&d_tw, (size_t)2 * nfft * sizeof(double)) != hipSuccess) { hipFree(d_win); return fail(h, "%s: hipMalloc of the twiddles failed", who); }
    hipError_t e = hipMalloc((void**)blk, bytes);
    if (e == hipSuccess) e = hipMemcpy(d_win, window, (size_t)W * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_tw, twiddle, (size_t)2 * nfft * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        StftBasisParams pb{d_win, d_tw, (double2*)*blk, W, nfft, NB};
        launch<stft_dist_basis_kernel>(h->device, dim3((unsigned)(((size_t)W * NB + 255) / 256)), dim3(256), 0, (hipStream_t)nullptr, pb);
        e = extra(*blk, d_tw);
        if (e == hipSuccess) e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    hipFree(d_win); hipFree(d_tw);
    if (e != hipSuccess) { if (*blk) hipFree(*blk); return fail(h, "%s: building the %s failed: %s", who, what, hipGetErrorString(e)); }
    return 0;
}

}  // namespace

extern "C" {

// The resampler.  LDS budget of a launch: 64 KiB (16384 floats) for the phase table and the input span together, so that at least two
// workgroups share a CU and no launch needs a raised LDS grant.  Plan: 1024 outputs per workgroup while their input span fits the budget,
// else 256, else the span is not staged at all (the kernel reads x from global memory: filters of tens of thousands of taps per phase);
// the table is staged when it fits beside the span, else read from global memory (L2-resident: at most 66 K floats).
int ev_load_resampler(ev_handle* h, const float* taps, int n_taps, int up, int down) {
    if (enter(h)) return 1;
    if (!taps) return fail(h, "ev_load_resampler: null taps");
    if (up < 1 || up > 640 || down < 1 || down > 640) return fail(h, "ev_load_resampler: up=%d down=%d outside 1 <= up, down <= 640", up, down);
    if (std::gcd(up, down) != 1) return fail(h, "ev_load_resampler: gcd(up, down) must be 1 (up=%d down=%d: reduce the ratio)", up, down);
    if (n_taps < 1 || n_taps > 65537 || !(n_taps & 1)) return fail(h, "ev_load_resampler: n_taps=%d must be odd and <= 65537", n_taps);
    ResamplerW r;
    r.up = up; r.down = down; r.n_taps = n_taps;
    r.W = (n_taps + up - 1) / up; r.Wp = r.W | 1; r.tab_floats = round_up(up * r.Wp, 4);
    std::vector<float> tab((size_t)r.tab_floats, 0.f);
    for (int k = 0; k < n_taps; ++k) tab[(size_t)(k % up) * r.Wp + k / up] = taps[k];
    ResamplerW& cur = h->rs;
    if (cur.loaded) { if (drop_owned(h, {cur.table})) return 1; cur = ResamplerW(); }
    if (dev_upload(h, tab, &r.table)) return 1;
    r.loaded = true;
    cur = r;
    return 0;
}

int ev_resample(ev_handle* h, const float* d_x, const int32_t* d_len, int B, int L_in, float* d_y, int L_out, void* stream) {
    if (enter(h)) return 1;
    const ResamplerW& r = h->rs;
    if (!r.loaded) return fail(h, "resampler not loaded (ev_load_resampler)");
    if (check_batch(h, __func__, B)) return 1;
    if (L_in < 1 || !d_x || !d_y) return fail(h, "ev_resample: bad arguments L_in=%d (L_in >= 1, non-null tensors)", L_in);
    const long long want = ((long long)L_in * r.up + r.down - 1) / r.down;
    if (want > 2147483647LL || (long long)L_out != want)
        return fail(h, "ev_resample: L_out=%d must be ceil(L_in * up / down) = %lld (L_in=%d up=%d down=%d) and fit 31 bits", L_out, want, L_in, r.up, r.down);
    h->stream = (hipStream_t)stream;
    constexpr int BUDGET = 16384;           // floats of LDS per workgroup
    auto span_of = [&](int tile) { return (long long)r.W + ((long long)(r.up - 1) + (long long)(tile - 1) * r.down) / r.up; };
    int tile = 1024;
    bool sx = true;
    if (span_of(1024) > BUDGET) { tile = 256; sx = span_of(256) <= BUDGET; }
    const int span = sx ? (int)span_of(tile) : 0;
    const bool st = span + r.tab_floats <= BUDGET;
    ResampleParams p{};
    p.x = d_x; p.len = d_len; p.y = d_y; p.table = r.table;
    p.L_in = L_in; p.L_out = L_out; p.up = r.up; p.down = r.down; p.c = (r.n_taps - 1) / 2; p.W = r.W; p.Wp = r.Wp; p.span = span; p.tab_floats = r.tab_floats;
    const size_t smem = ((size_t)span + (st ? r.tab_floats : 0)) * sizeof(float);
    const dim3 grid((unsigned)((L_out + tile - 1) / tile), (unsigned)B);
    hipStream_t s = h->stream;
    if (tile == 1024) { if (st) launch<resample_kernel<1024, true, true>>(h->device, grid, dim3(256), smem, s, p); else launch<resample_kernel<1024, true, false>>(h->device, grid, dim3(256), smem, s, p); }
    else if (sx)      { if (st) launch<resample_kernel<256, true, true>>(h->device, grid, dim3(256), smem, s, p);  else launch<resample_kernel<256, true, false>>(h->device, grid, dim3(256), smem, s, p); }
    else              { if (st) launch<resample_kernel<256, false, true>>(h->device, grid, dim3(256), smem, s, p); else launch<resample_kernel<256, false, false>>(h->device, grid, dim3(256), smem, s, p); }
    HIPCHK(h, hipGetLastError());
    return 0;
}

int ev_mel_stats(ev_handle* h, const float* d_mel, const int32_t* d_len, int B, int C, int T, double* d_row_sums, void* stream) {
    if (enter(h)) return 1;
    if (B < 1 || B > 65535 || C < 1 || T < 1 || !d_mel || !d_len || !d_row_sums)
        return fail(h, "ev_mel_stats: bad arguments B=%d C=%d T=%d (1 <= B <= 65535, C >= 1, T >= 1, non-null tensors)", B, C, T);
    h->stream = (hipStream_t)stream;
    const int ntiles = (T + 31) / 32;
    if (scratch_acquire(h, h->stat_ws, (size_t)B * ntiles * 2 * sizeof(double))) return 1;
    double* part = (double*)h->stat_ws.p;
    hipLaunchKernelGGL(mel_stats_kernel, dim3(ntiles, B), dim3(256), 0, h->stream, d_mel, d_len, C, T, part, ntiles);
    hipLaunchKernelGGL(cfm_loss_merge_kernel, dim3((B + 63) / 64), dim3(64), 0, h->stream, (const double*)part, ntiles, B, d_row_sums);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// Silence trimming.  The hop blocks of a row start at -off, off = (F/2) mod H, so that every frame [f H - F/2, f H + F/2) is F / H whole
// blocks (kernels: ev_analysis_kernels.h); nblk = ceil((L + off) / H) blocks per row, 12 bytes each: all float64 sums first, then all fp32 maxima.
int ev_trim_bounds(ev_handle* h, const float* d_x, const int32_t* d_len, int B, int L, int frame_length, int hop_length, float top_db,
                   int32_t* d_bounds, float* d_peak, void* stream) {
    if (enter(h)) return 1;
    if (check_batch(h, __func__, B)) return 1;
    if (L < 1 || !d_x || !d_bounds) return fail(h, "ev_trim_bounds: bad arguments L=%d (L >= 1, non-null d_x and d_bounds)", L);
    const int F = frame_length, H = hop_length;
    if (check_hop(h, __func__, H)) return 1;
    if (F < H || F % H) return fail(h, "ev_trim_bounds: frame_length=%d must be a multiple of hop_length=%d (frame_length %% hop_length != 0)", F, H);
    if (F / H > 64) return fail(h, "ev_trim_bounds: frame_length / hop_length = %d exceeds 64 (frame_length=%d hop_length=%d)", F / H, F, H);
    h->stream = (hipStream_t)stream;
    const int R = F / H, off = (F / 2) % H;
    const int nblk = (int)(((long long)L + off + H - 1) / H);
    if (scratch_acquire(h, h->trim_ws, (size_t)B * nblk * 12)) return 1;
    double* bsum = (double*)h->trim_ws.p;
    float* bmax = (float*)(bsum + (size_t)B * nblk);
    TrimBlocksParams pb{};
    pb.x = d_x; pb.len = d_len; pb.bsum = bsum; pb.bmax = bmax; pb.L = L; pb.H = H; pb.off = off; pb.nblk = nblk;
    launch<trim_blocks_kernel>(h->device, dim3((unsigned)((nblk + TRIM_TILE - 1) / TRIM_TILE), (unsigned)B), dim3(256), 0, h->stream, pb);
    TrimBoundsParams pf{};
    pf.bsum = bsum; pf.bmax = bmax; pf.len = d_len; pf.bounds = d_bounds; pf.peak = d_peak;
    pf.L = L; pf.H = H; pf.R = R; pf.off = off; pf.nblk = nblk; pf.F = (double)F; pf.thr = pow(10.0, -(double)top_db / 10.0);
    launch<trim_bounds_kernel>(h->device, dim3((unsigned)B), dim3(256), 0, h->stream, pf);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int ev_trim_apply(ev_handle* h, const float* d_x, const int32_t* d_bounds, const float* d_peak, float target_peak, int B, int L,
                  float* d_y, int L_out, int32_t* d_out_len, void* stream) {
    if (enter(h)) return 1;
    if (check_batch(h, __func__, B)) return 1;
    if (L < 1 || L_out < 1 || !d_x || !d_bounds || !d_y || !d_out_len)
        return fail(h, "ev_trim_apply: bad arguments L=%d L_out=%d (L >= 1, L_out >= 1, non-null d_x, d_bounds, d_y and d_out_len)", L, L_out);
    h->stream = (hipStream_t)stream;
    TrimApplyParams p{};
    p.x = d_x; p.bounds = d_bounds; p.peak = d_peak; p.y = d_y; p.out_len = d_out_len; p.target = target_peak; p.L = L; p.L_out = L_out;
    launch<gather_scale_kernel>(h->device, dim3((unsigned)(((long long)L_out + 1023) / 1024), (unsigned)B), dim3(256), 0, h->stream, p);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// Pitch tracking: one workgroup per (frame, row); LDS = 4 (tau_max + 1) float64 partials + the W + tau_max + 1 staged samples (ev_analysis_kernels.h).
int ev_pitch_yin(ev_handle* h, const float* d_x, const int32_t* d_len, int B, int L, int frame_length, int hop_length, int tau_min,
                 int tau_max, float threshold, int32_t* d_lag, float* d_period, float* d_cmnd, void* stream) {
    if (enter(h)) return 1;
    if (check_batch(h, __func__, B)) return 1;
    if (L < 1 || !d_x) return fail(h, "ev_pitch_yin: bad arguments L=%d (L >= 1, non-null d_x)", L);
    const int W = frame_length, H = hop_length;
    if (check_hop(h, __func__, H) || check_frame_length(h, __func__, W) || check_lag_range(h, __func__, tau_min, tau_max)) return 1;
    if (!(threshold > 0.f && threshold <= 1.f)) return fail(h, "ev_pitch_yin: threshold=%g outside 0 < threshold <= 1", (double)threshold);
    if (!d_lag && !d_period && !d_cmnd) return fail(h, "ev_pitch_yin: no output (at least one of d_lag, d_period, d_cmnd must be non-null)");
    h->stream = (hipStream_t)stream;
    PitchYinParams p{};
    p.x = d_x; p.len = d_len; p.lag = d_lag; p.period = d_period; p.cmnd = d_cmnd;
    p.L = L; p.F = frames_of(L, H); p.W = W; p.H = H; p.tau_min = tau_min; p.tau_max = tau_max; p.thr = (double)threshold;
    const size_t n = (size_t)tau_max + 1;
    const size_t smem = 4 * n * sizeof(double) + ((size_t)W + n) * sizeof(float);
    launch<pitch_yin_kernel>(h->device, dim3((unsigned)p.F, (unsigned)B), dim3(256), smem, h->stream, p);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// Probabilistic YIN, the observation: pitch_yin_kernel's grid and LDS plus the trough tables behind them (pyin_observe_kernel, ev_analysis_kernels.h).
// The threshold prior travels in the kernel's arguments (n_thr <= 128), with its ascending prefix sums.
int ev_pyin_observe(ev_handle* h, const float* d_x, const int32_t* d_len, int B, int L, int frame_length, int hop_length, int tau_min,
                    int tau_max, double sr, double fmin, int bins_per_octave, int n_bins, const double* w, int n_thr, double boltzmann,
                    double no_trough_prob, double* d_obs, double* d_pv, void* stream) {
    if (enter(h)) return 1;
    if (check_batch(h, __func__, B)) return 1;
    if (L < 1 || !d_x) return fail(h, "ev_pyin_observe: bad arguments L=%d (L >= 1, non-null d_x)", L);
    const int W = frame_length, H = hop_length;
    if (check_hop(h, __func__, H) || check_frame_length(h, __func__, W) || check_lag_range(h, __func__, tau_min, tau_max)) return 1;
    if (n_thr < 1 || n_thr > 128) return fail(h, "ev_pyin_observe: n_thr=%d outside 1 <= n_thr <= 128", n_thr);
    if (n_bins < 2 || n_bins > 1024) return fail(h, "ev_pyin_observe: n_bins=%d outside 2 <= n_bins <= 1024", n_bins);
    if (bins_per_octave < 1) return fail(h, "ev_pyin_observe: bins_per_octave=%d must be at least 1", bins_per_octave);
    if (!(sr > 0.0) || !(fmin > 0.0) || !std::isfinite(sr) || !std::isfinite(fmin))
        return fail(h, "ev_pyin_observe: sr=%g and fmin=%g must be positive and finite", sr, fmin);
    if (!(boltzmann > 0.0) || !std::isfinite(boltzmann)) return fail(h, "ev_pyin_observe: boltzmann=%g must be positive and finite", boltzmann);
    if (!(no_trough_prob >= 0.0 && no_trough_prob <= 1.0))
        return fail(h, "ev_pyin_observe: no_trough_prob=%g outside 0 <= no_trough_prob <= 1", no_trough_prob);
    if (!w) return fail(h, "ev_pyin_observe: w must be non-null (HOST, n_thr doubles)");
    for (int t = 0; t < n_thr; ++t)
        if (!(w[t] >= 0.0) || !std::isfinite(w[t])) return fail(h, "ev_pyin_observe: w[%d]=%g is not a finite weight >= 0", t, w[t]);
    if (!d_obs || !d_pv) return fail(h, "ev_pyin_observe: no output (d_obs and d_pv must be non-null)");
    h->stream = (hipStream_t)stream;
    PyinObserveParams p{};
    p.x = d_x; p.len = d_len; p.obs = d_obs; p.pv = d_pv;
    p.L = L; p.F = frames_of(L, H); p.W = W; p.H = H; p.tau_min = tau_min; p.tau_max = tau_max;
    p.n_bins = n_bins; p.n_thr = n_thr; p.kmax = (tau_max - tau_min) / 2 + 1;
    p.sr = sr; p.fmin = fmin; p.bpo = (double)bins_per_octave; p.lambda = boltzmann; p.c0 = 1.0 - std::exp(-boltzmann); p.ntp = no_trough_prob;
    double run = 0.0;
    for (int t = 0; t < n_thr; ++t) { p.w[t] = w[t]; run += w[t]; p.cw[t + 1] = run; }
    const size_t n = (size_t)tau_max + 1, kmax = (size_t)p.kmax;
    const size_t yin = (4 * n * sizeof(double) + ((size_t)W + n) * sizeof(float) + 7) / 8 * 8;
    p.off_extra = (int)yin;
    const size_t smem = yin + (2 * kmax + 1 + (size_t)n_thr + 1 + (size_t)n_bins + 4) * sizeof(double)
                      + (3 * kmax + 8 + (kmax + 63) / 64 * ((size_t)n_thr + 1)) * sizeof(int);
    launch<pyin_observe_kernel>(h->device, dim3((unsigned)p.F, (unsigned)B), dim3(256), smem, h->stream, p);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// Probabilistic YIN, the decoding: one workgroup per row, one thread per state (two beyond 1024 states); LDS = 2 x 2 n_bins float64 of delta,
// the two transition tables and the end state's reduction (pyin_decode_kernel, ev_analysis_kernels.h).  The host tables travel in the kernel's arguments.
int ev_pyin_decode(ev_handle* h, const double* d_obs, const double* d_pv, const int32_t* d_len, int B, int L, int hop_length, int n_bins, int R,
                   const double* log_tri, const double* log_Z, double log_stay, double log_switch, uint8_t* d_back, int32_t* d_state,
                   double* d_loglik, void* stream) {
    if (enter(h)) return 1;
    if (check_batch(h, __func__, B)) return 1;
    if (L < 1) return fail(h, "ev_pyin_decode: L=%d must be at least 1", L);
    const int H = hop_length;
    if (check_hop(h, __func__, H)) return 1;
    if (n_bins < 2 || n_bins > 1024) return fail(h, "ev_pyin_decode: n_bins=%d outside 2 <= n_bins <= 1024", n_bins);
    if (R < 0 || R > 63) return fail(h, "ev_pyin_decode: R=%d outside 0 <= R <= 63", R);
    if (!(log_stay < 0.0) || !(log_switch < 0.0) || !std::isfinite(log_stay) || !std::isfinite(log_switch))
        return fail(h, "ev_pyin_decode: switch_prob outside 0 < switch_prob < 1 (log_stay=%g and log_switch=%g must be finite and negative)",
                    log_stay, log_switch);
    if (!d_obs || !d_pv) return fail(h, "ev_pyin_decode: d_obs and d_pv must be non-null");
    if (!log_tri || !log_Z) return fail(h, "ev_pyin_decode: log_tri (HOST, R + 1 doubles) and log_Z (HOST, n_bins doubles) must be non-null");
    if (!d_back) return fail(h, "ev_pyin_decode: d_back must be non-null (B x F x 2 n_bins bytes of the caller's)");
    if (!d_state || !d_loglik) return fail(h, "ev_pyin_decode: no output (d_state and d_loglik must be non-null)");
    for (int d = 0; d <= R; ++d) if (!std::isfinite(log_tri[d])) return fail(h, "ev_pyin_decode: log_tri[%d]=%g is not finite", d, log_tri[d]);
    for (int j = 0; j < n_bins; ++j) if (!std::isfinite(log_Z[j])) return fail(h, "ev_pyin_decode: log_Z[%d]=%g is not finite", j, log_Z[j]);
    h->stream = (hipStream_t)stream;
    PyinDecodeParams p{};
    p.obs = d_obs; p.pv = d_pv; p.len = d_len; p.back = d_back; p.state = d_state; p.loglik = d_loglik;
    p.L = L; p.F = frames_of(L, H); p.H = H; p.n_bins = n_bins; p.R = R;
    p.init = -std::log(2.0 * (double)n_bins); p.tiny = std::numeric_limits<double>::min();
    for (int d = 0; d <= R; ++d) { p.t_stay[d] = log_tri[d] + log_stay; p.t_switch[d] = log_tri[d] + log_switch; }
    if (n_bins <= 128) for (int j = 0; j < n_bins; ++j) p.zc[j] = log_Z[j];
    else {
        for (int j = 63; j <= n_bins - 64; ++j)
            if (log_Z[j] != log_Z[63])
                return fail(h, "ev_pyin_decode: log_Z[%d] differs from log_Z[63]: log_Z must be constant over R <= j <= n_bins - 1 - R", j);
        for (int j = 0; j < 64; ++j) { p.zc[j] = log_Z[j]; p.zc[64 + j] = log_Z[n_bins - 64 + j]; }
    }
    const int S = 2 * n_bins, NT = std::min(1024, round_up(S, 64));
    const size_t smem = (2 * (size_t)S + 16 + 128) * sizeof(double) + 16 * sizeof(int);
    launch<pyin_decode_kernel>(h->device, dim3(B), dim3(NT), smem, h->stream, p);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// Dynamic time warping: one workgroup per row (dtw_kernel, ev_analysis_kernels.h).  LDS plan in bytes: [D ring 3 x Tx float64][S ring 3 x Tx uint16],
// reused after the forward pass as the path stage of Tx + Ty - 1 words; then the decision words ceil(Ty / 32) x Tx x 8 bytes where they still
// fit into the CU's 160 KiB, else in the handle's arena.  Without a path there are no decision words at all.
int ev_dtw(ev_handle* h, const float* d_x, const float* d_y, const int32_t* d_xlen, const int32_t* d_ylen, int B, int C, int Tx, int Ty, int metric,
           double* d_cost, int32_t* d_steps, int32_t* d_path, void* stream) {
    if (enter(h)) return 1;
    constexpr size_t LDS_MAX = 160 * 1024 - 64;                          // (the kernel's one static word is taken off the CU's 160 KiB)
    if (check_batch(h, __func__, B)) return 1;
    if (C < 1 || C > 128) return fail(h, "ev_dtw: C=%d outside 1 <= C <= 128", C);
    if (Tx < 1 || Tx > 4096) return fail(h, "ev_dtw: Tx=%d outside 1 <= Tx <= 4096", Tx);
    if (Ty < 1 || Ty > 4096) return fail(h, "ev_dtw: Ty=%d outside 1 <= Ty <= 4096", Ty);
    if (metric != 0 && metric != 1) return fail(h, "ev_dtw: metric=%d is neither 0 (Euclidean) nor 1 (squared Euclidean)", metric);
    if (!d_x || !d_y) return fail(h, "ev_dtw: d_x and d_y must be non-null");
    if (!d_cost || !d_steps) return fail(h, "ev_dtw: d_cost and d_steps must be non-null");
    h->stream = (hipStream_t)stream;
    DtwParams p{};
    p.x = d_x; p.y = d_y; p.xlen = d_xlen; p.ylen = d_ylen; p.cost = d_cost; p.steps = d_steps; p.path = d_path;
    p.C = C; p.Tx = Tx; p.Ty = Ty; p.nyw = (Ty + 31) / 32; p.metric = metric;
    p.off_s = 3 * Tx * (int)sizeof(double);
    const size_t ring = (size_t)p.off_s + 3 * (size_t)Tx * sizeof(unsigned short);
    size_t smem = (ring + 15) / 16 * 16;
    if (d_path) {
        smem = (std::max(ring, (size_t)(Tx + Ty - 1) * sizeof(unsigned int)) + 15) / 16 * 16;
        p.off_bits = (int)smem;
        const size_t bit_bytes = (size_t)p.nyw * Tx * sizeof(unsigned long long);
        if (smem + bit_bytes <= LDS_MAX) smem += bit_bytes;
        else {
            if (scratch_acquire(h, h->dtw_ws, (size_t)B * bit_bytes)) return 1;
            p.gbits = (unsigned long long*)h->dtw_ws.p;
        }
    }
    const int NT = std::min(1024, round_up(Tx, 64));
    const int R = (Tx + NT - 1) / NT;                                    // 1 .. 4 rows of the matrix per thread
    if (R == 1) launch<dtw_kernel<1, 8>>(h->device, dim3(B), dim3(NT), smem, h->stream, p);
    else if (R == 2) launch<dtw_kernel<2, 8>>(h->device, dim3(B), dim3(NT), smem, h->stream, p);
    else launch<dtw_kernel<4, 4>>(h->device, dim3(B), dim3(NT), smem, h->stream, p);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// Loudness (kernels and the scheme: ev_analysis_kernels.h).  Arena, in doubles: [state B x NC x 4][pieces B x NC x npp][sub-block energies B x NS, only
// without d_sub]; NC = ceil(NS S / LOUD_CHUNK) chunks that can hold a counted sample, npp = the most sub-blocks a chunk can touch.
int ev_loudness(ev_handle* h, const float* d_x, const int32_t* d_len, int B, int L, int sub_len, const double* coef, double abs_gate,
                double* d_sub, double* d_block, double* d_gated, int32_t* d_counts, void* stream) {
    if (enter(h)) return 1;
    const int S = sub_len;
    if (check_batch(h, __func__, B)) return 1;
    if (S < 16 || S > 65536) return fail(h, "ev_loudness: sub_len=%d outside 16 <= sub_len <= 65536", S);
    if (L < 1) return fail(h, "ev_loudness: L=%d must be at least 1", L);
    if (!d_x) return fail(h, "ev_loudness: d_x must be non-null");
    if (!coef) return fail(h, "ev_loudness: coef must be non-null (HOST, 10 doubles)");
    if (!d_gated || !d_counts) return fail(h, "ev_loudness: d_gated and d_counts must be non-null");
    for (int st = 0; st < 2; ++st) {
        const double a1 = coef[5 * st + 3], a2 = coef[5 * st + 4];
        bool finite = true;
        for (int i = 0; i < 5; ++i) finite = finite && std::isfinite(coef[5 * st + i]);
        if (!(finite && std::fabs(a2) < 1.0 && std::fabs(a1) < 1.0 + a2))
            return fail(h, "ev_loudness: coef stage %d is unstable or not finite (a1=%g a2=%g; |a2| < 1 and |a1| < 1 + a2 expected)", st + 1, a1, a2);
    }
    h->stream = (hipStream_t)stream;
    LoudCoef k{coef[0], coef[1], coef[2], coef[3], coef[4], coef[5], coef[6], coef[7], coef[8], coef[9]};
    const int NS = L / S, NB = std::max(NS - 3, 0);
    const int NC = (int)(((long long)NS * S + LOUD_CHUNK - 1) / LOUD_CHUNK);
    const int npp = (LOUD_CHUNK + S - 2) / S + 1;
    const size_t n_state = (size_t)B * NC * 4, n_part = (size_t)B * NC * npp, n_sub = d_sub ? 0 : (size_t)B * NS;
    double* sub = d_sub;
    if (NS > 0) {
        if (scratch_acquire(h, h->loud_ws, (n_state + n_part + n_sub) * sizeof(double))) return 1;
        double* state = (double*)h->loud_ws.p;
        double* part = state + n_state;
        if (!sub) sub = part + n_part;
        LoudChunkParams pc{};
        pc.x = d_x; pc.len = d_len; pc.state = state; pc.part = part; pc.L = L; pc.S = S; pc.NC = NC; pc.npp = npp; pc.k = k;
        LoudCarryParams pk{};
        pk.state = state; pk.len = d_len; pk.L = L; pk.S = S; pk.NC = NC;
        for (int c = 0; c < 4; ++c) {                                    // column c of M: the state LOUD_CHUNK zero samples after unit state c
            double s[4] = {0.0, 0.0, 0.0, 0.0};
            s[c] = 1.0;
            for (int n = 0; n < LOUD_CHUNK; ++n) {
                const double x = 0.0;
                const double y1 = std::fma(k.b0, x, s[0]);
                s[0] = std::fma(-k.a1, y1, std::fma(k.b1, x, s[1]));
                s[1] = std::fma(-k.a2, y1, k.b2 * x);
                const double y2 = std::fma(k.c0, y1, s[2]);
                s[2] = std::fma(-k.d1, y2, std::fma(k.c1, y1, s[3]));
                s[3] = std::fma(-k.d2, y2, k.c2 * y1);
            }
            for (int r = 0; r < 4; ++r) pk.M[4 * r + c] = s[r];
        }
        const dim3 grid((unsigned)((NC + 63) / 64), (unsigned)B);
        launch<loud_chunk_kernel<false>>(h->device, grid, dim3(64), 0, h->stream, pc);
        launch<loud_carry_kernel>(h->device, dim3((unsigned)B), dim3(64), 0, h->stream, pk);
        launch<loud_chunk_kernel<true>>(h->device, grid, dim3(64), 0, h->stream, pc);
        LoudMergeParams pm{};
        pm.part = part; pm.len = d_len; pm.sub = sub; pm.L = L; pm.S = S; pm.NC = NC; pm.npp = npp; pm.NS = NS;
        launch<loud_merge_kernel>(h->device, dim3((unsigned)((NS + 255) / 256), (unsigned)B), dim3(256), 0, h->stream, pm);
    }
    LoudGateParams pg{};
    pg.sub = sub; pg.len = d_len; pg.block = d_block; pg.gated = d_gated; pg.counts = d_counts;
    pg.L = L; pg.S = S; pg.NS = NS; pg.NB = NB; pg.abs_gate = abs_gate;
    launch<loud_gate_kernel>(h->device, dim3((unsigned)B), dim3(256), 0, h->stream, pg);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// SRMR (kernels and the scheme: ev_analysis_kernels.h; the definition: include/emojivoice.h).  The load computes both zero-input transitions
// over H samples by running the kernels' own recurrences on unit states, and puts everything into ONE device block.  Arena of a call, in doubles:
// [channel states B x NC x 8 N][band states B x NC x 2 N K][window-quarter sums B x NC x 4 N K], NC = NF + 3 chunks.
int ev_load_srmr(ev_handle* h, const double* chan, const double* mod, const double* window, const double* erb, const double* cutoff, int N, int K, int H) {
    STOI_EXACT
    if (enter(h)) return 1;
    if (!chan || !mod || !window || !erb || !cutoff) return fail(h, "ev_load_srmr: chan, mod, window, erb and cutoff must be non-null (HOST)");
    if (N < 1 || N > SRMR_MAXN) return fail(h, "ev_load_srmr: N=%d outside 1 <= N <= %d", N, SRMR_MAXN);
    if (K < 1 || K > SRMR_MAXK) return fail(h, "ev_load_srmr: K=%d outside 1 <= K <= %d", K, SRMR_MAXK);
    if (H < 64 || H > 1024 || H % 64) return fail(h, "ev_load_srmr: H=%d must be a multiple of 64 with 64 <= H <= 1024", H);
    const int W = 4 * H;
    if (check_finite(h, __func__, "chan", chan, 3 * N) || check_finite(h, __func__, "window", window, W) || check_finite(h, __func__, "erb", erb, N) ||
        check_finite(h, __func__, "cutoff", cutoff, K)) return 1;
    for (int j = 0; j < N; ++j) {
        const double r = std::hypot(chan[3 * j], chan[3 * j + 1]);
        if (!(r < 1.0)) return fail(h, "ev_load_srmr: chan[%d] has |a| = %g; |a| < 1 expected", j, r);
    }
    for (int k = 0; k < K; ++k) {
        const double a1 = mod[5 * k + 3], a2 = mod[5 * k + 4];
        bool finite = true;
        for (int i = 0; i < 5; ++i) finite = finite && std::isfinite(mod[5 * k + i]);
        if (!(finite && std::fabs(a2) < 1.0 && std::fabs(a1) < 1.0 + a2))
            return fail(h, "ev_load_srmr: mod band %d is unstable or not finite (a1=%g a2=%g; |a2| < 1 and |a1| < 1 + a2 expected)", k, a1, a2);
    }
    const size_t o_chan = 0, o_Mc = o_chan + 3 * (size_t)N, o_mod = o_Mc + 20 * (size_t)N, o_Mb = o_mod + 5 * (size_t)K, o_win = o_Mb + 4 * (size_t)K,
                 o_erb = o_win + W, o_cut = o_erb + N, total = o_cut + K;
    std::vector<double> blk(total);
    std::copy(chan, chan + 3 * N, blk.begin() + o_chan);
    std::copy(mod, mod + 5 * K, blk.begin() + o_mod);
    std::copy(window, window + W, blk.begin() + o_win);
    std::copy(erb, erb + N, blk.begin() + o_erb);
    std::copy(cutoff, cutoff + K, blk.begin() + o_cut);
    for (int j = 0; j < N; ++j) {                                        // column c of a channel's M: the cascade H zero samples after unit state c
        const double ar = chan[3 * j], ai = chan[3 * j + 1];
        for (int c = 0; c < 4; ++c) {
            double r[4] = {0.0, 0.0, 0.0, 0.0}, i[4] = {0.0, 0.0, 0.0, 0.0};
            r[c] = 1.0;
            for (int n = 0; n < H; ++n) {
                const double xv = 0.0;
                double nr = xv + (ar * r[0] - ai * i[0]), ni = ar * i[0] + ai * r[0];
                r[0] = nr; i[0] = ni;
                for (int s = 1; s < 4; ++s) {
                    nr = r[s - 1] + (ar * r[s] - ai * i[s]); ni = i[s - 1] + (ar * i[s] + ai * r[s]);
                    r[s] = nr; i[s] = ni;
                }
            }
            for (int s = c; s < 4; ++s) {
                blk[o_Mc + 20 * (size_t)j + 2 * (s * (s + 1) / 2 + c)] = r[s];
                blk[o_Mc + 20 * (size_t)j + 2 * (s * (s + 1) / 2 + c) + 1] = i[s];
            }
        }
    }
    for (int k = 0; k < K; ++k) {                                        // column c of a band's M
        const double* m = mod + 5 * k;
        for (int c = 0; c < 2; ++c) {
            double s1 = c == 0 ? 1.0 : 0.0, s2 = c == 1 ? 1.0 : 0.0;
            for (int n = 0; n < H; ++n) {
                const double e = 0.0;
                const double y = std::fma(m[0], e, s1);
                s1 = std::fma(-m[3], y, std::fma(m[1], e, s2));
                s2 = std::fma(-m[4], y, m[2] * e);
            }
            blk[o_Mb + 4 * (size_t)k + c] = s1; blk[o_Mb + 4 * (size_t)k + 2 + c] = s2;
        }
    }
    SrmrW& cur = h->srmr;
    if (cur.loaded) { if (drop_owned(h, {(void*)cur.blk})) return 1; cur = SrmrW(); }
    SrmrW t;
    if (dev_upload(h, blk, &t.blk)) return 1;
    t.t = SrmrTables{t.blk + o_chan, t.blk + o_Mc, t.blk + o_mod, t.blk + o_Mb, t.blk + o_win, t.blk + o_erb, t.blk + o_cut, N, K, H};
    t.loaded = true;
    cur = t;
    return 0;
}

int ev_srmr(ev_handle* h, const float* d_x, const int32_t* d_len, int B, int L, double* d_frame, double* d_mean, double* d_srmr, int32_t* d_counts,
            void* stream) {
    if (enter(h)) return 1;
    const SrmrW& w = h->srmr;
    if (!w.loaded) return fail(h, "ev_srmr: tables not loaded (ev_load_srmr)");
    if (check_batch(h, __func__, B)) return 1;
    if (L < 1) return fail(h, "ev_srmr: L=%d must be at least 1", L);
    if (!d_x) return fail(h, "ev_srmr: d_x must be non-null");
    if (!d_mean || !d_srmr || !d_counts) return fail(h, "ev_srmr: d_mean, d_srmr and d_counts must be non-null");
    h->stream = (hipStream_t)stream;
    const int N = w.t.N, K = w.t.K, H = w.t.H, NK = N * K;
    const int NF = L >= 4 * H ? (L - 4 * H) / H + 1 : 0, NC = NF > 0 ? NF + 3 : 0;
    double* cst = nullptr; double* bst = nullptr; double* part = nullptr;
    if (NF > 0) {
        const size_t n_c = (size_t)B * NC * 8 * N, n_b = (size_t)B * NC * 2 * NK, n_p = (size_t)B * NC * 4 * NK;
        if (scratch_acquire(h, h->srmr_ws, (n_c + n_b + n_p) * sizeof(double))) return 1;
        cst = (double*)h->srmr_ws.p; bst = cst + n_c; part = bst + n_b;
        SrmrChunkParams pc{d_x, d_len, cst, bst, part, w.t, L, NC};
        SrmrCarryParams kc{cst, d_len, w.t, L, NC}, kb{bst, d_len, w.t, L, NC};
        const dim3 grid((unsigned)NC, (unsigned)B);
        launch<srmr_chunk_kernel<0>>(h->device, grid, dim3(64), 0, h->stream, pc);
        launch<srmr_carry_chan_kernel>(h->device, dim3((unsigned)B), dim3(64), 0, h->stream, kc);
        launch<srmr_chunk_kernel<1>>(h->device, grid, dim3(64), 0, h->stream, pc);
        launch<srmr_carry_band_kernel>(h->device, dim3((unsigned)B), dim3(256), 0, h->stream, kb);
        launch<srmr_chunk_kernel<2>>(h->device, grid, dim3(64), 0, h->stream, pc);
    }
    SrmrRowsParams pr{part, d_len, d_frame, d_mean, d_srmr, d_counts, w.t, L, NC, NF};
    launch<srmr_rows_kernel>(h->device, dim3((unsigned)B), dim3(256), 0, h->stream, pr);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// STOI / ESTOI (kernels, the definition and every order: ev_analysis_kernels.h).  Arena: [E B x NF doubles][band spectra B x 2 x n_bands x NM doubles,
// only without d_tob][segment scores B x NSEG x 2 doubles, only without d_seg][idx B x NF int32].
int ev_load_stoi(ev_handle* h, const double* window, const double* twiddle, const int32_t* bands, int W, int H, int nfft, int n_bands, int N) {
    if (enter(h)) return 1;
    if (!window || !twiddle || !bands) return fail(h, "ev_load_stoi: window, twiddle and bands must be non-null (HOST)");
    if (H < 32 || H > 256 || H % 32) return fail(h, "ev_load_stoi: H=%d must be a multiple of 32 with 32 <= H <= 256", H);
    if (W != 2 * H) return fail(h, "ev_load_stoi: W=%d must be 2 H = %d (the overlap-add has exactly two terms)", W, 2 * H);
    if (nfft < W || nfft > 1024) return fail(h, "ev_load_stoi: nfft=%d outside W <= nfft <= 1024 (W=%d)", nfft, W);
    if (n_bands < 1 || n_bands > 32) return fail(h, "ev_load_stoi: n_bands=%d outside 1 <= n_bands <= 32", n_bands);
    if (N < 2 || N > 64) return fail(h, "ev_load_stoi: N=%d outside 2 <= N <= 64", N);
    StoiW t;
    t.W = W; t.H = H; t.nfft = nfft; t.n_bands = n_bands; t.N = N;
    t.bin_lo = nfft; t.bin_hi = 0;
    for (int r = 0; r < n_bands; ++r) {
        const int first = bands[2 * r], end = bands[2 * r + 1];
        if (first < 0 || first >= end || end > nfft / 2 + 1)
            return fail(h, "ev_load_stoi: bands[%d] = [%d, %d) outside 0 <= first < end <= nfft / 2 + 1 = %d", r, first, end, nfft / 2 + 1);
        t.bin_lo = std::min(t.bin_lo, first); t.bin_hi = std::max(t.bin_hi, end);
    }
    if (check_finite(h, __func__, "window", window, W) || check_finite(h, __func__, "twiddle", twiddle, 2 * nfft)) return 1;
    StoiW& cur = h->stoi;
    if (cur.loaded) { if (drop_owned(h, {cur.win, cur.tw, cur.bands})) return 1; cur = StoiW(); }
    if (dev_upload(h, std::vector<double>(window, window + W), &t.win)) return 1;
    if (dev_upload(h, std::vector<double>(twiddle, twiddle + 2 * (size_t)nfft), &t.tw)) return 1;
    if (dev_upload(h, std::vector<int32_t>(bands, bands + 2 * (size_t)n_bands), &t.bands)) return 1;
    t.loaded = true;
    cur = t;
    return 0;
}

int ev_stoi(ev_handle* h, const float* d_x, const float* d_y, const int32_t* d_len, int B, int L, double silence_ratio, double clip,
            uint8_t* d_keep, double* d_tob, double* d_seg, double* d_score, int32_t* d_counts, void* stream) {
    if (enter(h)) return 1;
    const StoiW& w = h->stoi;
    if (!w.loaded) return fail(h, "ev_stoi: tables not loaded (ev_load_stoi)");
    if (check_batch(h, __func__, B)) return 1;
    if (L < 1) return fail(h, "ev_stoi: L=%d must be at least 1", L);
    if (!d_x || !d_y) return fail(h, "ev_stoi: d_x and d_y must be non-null");
    if (!(silence_ratio > 0.0 && silence_ratio < 1.0)) return fail(h, "ev_stoi: silence_ratio=%g outside 0 < silence_ratio < 1", silence_ratio);
    if (!(clip > 1.0) || !std::isfinite(clip)) return fail(h, "ev_stoi: clip=%g must be finite and greater than 1", clip);
    if (!d_score || !d_counts) return fail(h, "ev_stoi: d_score and d_counts must be non-null");
    h->stream = (hipStream_t)stream;
    const int NF = L > w.W ? (L - w.W + w.H - 1) / w.H : 0, NM = std::max(NF - 1, 0), NSEG = std::max(NM - w.N + 1, 0);
    const size_t n_e = (size_t)B * NF, n_tob = d_tob ? 0 : (size_t)B * 2 * w.n_bands * NM, n_seg = d_seg ? 0 : (size_t)B * NSEG * 2;
    if (scratch_acquire(h, h->stoi_ws, (n_e + n_tob + n_seg) * sizeof(double) + n_e * sizeof(int32_t))) return 1;
    double* E = (double*)h->stoi_ws.p;
    double* tob = d_tob ? d_tob : E + n_e;
    double* seg = d_seg ? d_seg : E + n_e + n_tob;
    int32_t* idx = (int32_t*)(E + n_e + n_tob + n_seg);
    StoiTables t{w.win, w.tw, w.bands, w.W, w.H, w.nfft, w.n_bands, w.N, w.bin_lo, w.bin_hi};
    if (NF > 0) {
        StoiEnergyParams pe{d_x, d_len, E, t, L, NF};
        launch<stoi_energy_kernel>(h->device, dim3((unsigned)((NF + 63) / 64), (unsigned)B), dim3(64), 0, h->stream, pe);
    }
    StoiSelectParams ps{E, d_len, idx, d_keep, d_counts, t, L, NF, silence_ratio};
    launch<stoi_select_kernel>(h->device, dim3((unsigned)B), dim3(256), 0, h->stream, ps);
    if (NM > 0) {
        StoiBandParams pb{d_x, d_y, idx, d_counts, tob, t, L, NF, NM};
        const size_t smem = ((size_t)2 * w.nfft + 2 * w.W + 2 * (w.bin_hi - w.bin_lo)) * sizeof(double);
        launch<stoi_band_kernel>(h->device, dim3((unsigned)NM, (unsigned)B), dim3(256), smem, h->stream, pb);
    }
    if (NSEG > 0) {
        StoiSegParams pg{tob, d_counts, seg, t, NM, NSEG, clip};
        const size_t smem = ((size_t)2 * w.n_bands * (w.N | 1) + 64) * sizeof(double);
        launch<stoi_segment_kernel>(h->device, dim3((unsigned)NSEG, (unsigned)B), dim3(64), smem, h->stream, pg);
    }
    StoiMeanParams pm{seg, d_counts, d_score, NSEG};
    launch<stoi_mean_kernel>(h->device, dim3((unsigned)B), dim3(256), 0, h->stream, pm);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// Multi-resolution STFT distance at one resolution (kernels, the definition and every order: ev_analysis_kernels.h).  Arena: B x NF x 4 doubles, only
// without d_frame.
int ev_load_stft_dist(ev_handle* h, const double* window, const double* twiddle, int W, int H, int nfft) {
    if (enter(h)) return 1;
    if (!window || !twiddle) return fail(h, "ev_load_stft_dist: window and twiddle must be non-null (HOST)");
    if (check_dft_geometry(h, __func__, W, H, nfft, 2048)) return 1;
    if (check_finite(h, __func__, "window", window, W) || check_finite(h, __func__, "twiddle", twiddle, 2 * nfft)) return 1;
    StftDistW w;
    w.t.W = W; w.t.H = H; w.t.nfft = nfft; w.t.NB = nfft / 2 + 1; w.t.skew = dft_skew(H);
    StftDistW& cur = h->stftd;
    if (cur.loaded) { if (drop_owned(h, {(void*)cur.t.basis})) return 1; cur = StftDistW(); }
    char* blk = nullptr;
    auto none = [](char*, const double*) { return hipSuccess; };
    if (build_dft_basis(h, __func__, "basis", window, twiddle, W, nfft, (size_t)W * w.t.NB * sizeof(double2), &blk, none)) return 1;
    w.t.basis = (const double2*)blk;
    h->owned.push_back(blk);
    ++h->n_allocs;                          // (the basis is the handle's largest table: 33.6 MB at W = nfft = 2048)
    w.loaded = true;
    cur = w;
    return 0;
}

int ev_stft_dist(ev_handle* h, const float* d_x, const float* d_y, const int32_t* d_len, int B, int L, double power_floor,
                 double* d_frame, double* d_sums, int32_t* d_counts, void* stream) {
    if (enter(h)) return 1;
    const StftDistW& w = h->stftd;
    if (!w.loaded) return fail(h, "ev_stft_dist: tables not loaded (ev_load_stft_dist)");
    if (check_batch(h, __func__, B)) return 1;
    if (L < 1) return fail(h, "ev_stft_dist: L=%d must be at least 1", L);
    if (!d_x || !d_y) return fail(h, "ev_stft_dist: d_x and d_y must be non-null");
    if (!(power_floor > 0.0) || !std::isfinite(power_floor)) return fail(h, "ev_stft_dist: power_floor=%g must be finite and greater than 0", power_floor);
    if (!d_sums || !d_counts) return fail(h, "ev_stft_dist: d_sums and d_counts must be non-null");
    h->stream = (hipStream_t)stream;
    const StftDistTables& t = w.t;
    if (L / t.H > 0x7fffffef) return fail(h, "ev_stft_dist: L=%d at H=%d has more frames than an int32 tile index holds", L, t.H);
    const int NF = L > t.nfft / 2 ? 1 + L / t.H : 0;
    double* frame = d_frame;
    if (!frame && NF > 0) {
        if (scratch_acquire(h, h->stftd_ws, (size_t)B * NF * 4 * sizeof(double))) return 1;
        frame = (double*)h->stftd_ws.p;
    }
    if (NF > 0) {
        StftFramesParams pf{d_x, d_y, d_len, frame, t, L, NF, power_floor};
        const size_t smem = (size_t)2 * dft_span_words(15 * t.H + t.W, t.H, t.skew) * sizeof(float);
        launch<stft_dist_frames_kernel>(h->device, dim3((unsigned)((NF + 15) / 16), (unsigned)B), dim3(256), smem, h->stream, pf);
    }
    StftRowsParams pr{frame, d_len, d_sums, d_counts, t, L, NF};
    launch<stft_dist_rows_kernel>(h->device, dim3((unsigned)B), dim3(256), 0, h->stream, pr);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// Voice quality: spectral balance and cepstral peak prominence per frame (kernels, the definition and every order: ev_analysis_kernels.h).  One
// device block per load holds the four tables; a call needs no arena.
int ev_load_voice_quality(ev_handle* h, const double* window, const double* twiddle, int W, int H, int nfft, const int32_t* bands,
                          const double* slope_w, int q_fit, int q_min, int q_max, const double* fit_w, double q_mean) {
    if (enter(h)) return 1;
    if (!window || !twiddle || !bands || !slope_w || !fit_w)
        return fail(h, "ev_load_voice_quality: window, twiddle, bands, slope_w and fit_w must be non-null (HOST)");
    if (check_dft_geometry(h, __func__, W, H, nfft, 1024)) return 1;
    const int NB = nfft / 2 + 1;
    for (int i = 0; i < 6; ++i) {
        const int lo = bands[2 * i], hi = bands[2 * i + 1];
        if (lo < 0 || hi > NB || lo >= hi) return fail(h, "ev_load_voice_quality: bands[%d] = [%d, %d) must be non-empty inside [0, %d]", i, lo, hi, NB);
        if (i >= 4 && hi - lo < 2) return fail(h, "ev_load_voice_quality: bands[%d] = [%d, %d) must hold at least 2 bins (a slope)", i, lo, hi);
    }
    if (q_fit < 1 || q_fit > q_min || q_min > q_max || q_max > nfft / 2 || q_max - q_fit + 1 < 2)
        return fail(h, "ev_load_voice_quality: q_fit=%d q_min=%d q_max=%d outside 1 <= q_fit <= q_min <= q_max <= nfft / 2 = %d with at least 2 quefrencies",
                    q_fit, q_min, q_max, nfft / 2);
    const int NQ = q_max - q_fit + 1;
    if (check_finite(h, __func__, "window", window, W) || check_finite(h, __func__, "twiddle", twiddle, 2 * nfft)
        || check_finite(h, __func__, "slope_w", slope_w, 2 * NB) || check_finite(h, __func__, "fit_w", fit_w, NQ)) return 1;
    if (!std::isfinite(q_mean)) return fail(h, "ev_load_voice_quality: q_mean=%g is not finite", q_mean);
    VoiceQW w;
    VoiceQTables& t = w.t;
    t.W = W; t.H = H; t.nfft = nfft; t.NB = NB; t.NBp = (NB + 3) / 4 * 4; t.NQ = NQ; t.skew = dft_skew(H);
    t.S = NB + ((2 - NB) % 32 + 32) % 32;                               // the smallest S >= NB with S = 2 mod 32
    t.q_fit = q_fit; t.q_min = q_min; t.q_max = q_max; t.q_mean = q_mean;
    for (int i = 0; i < 12; ++i) t.band[i] = bands[i];
    w.lds = (size_t)16 * t.S * sizeof(double) + (size_t)dft_span_words(15 * H + W, H, t.skew) * sizeof(float);
    if (w.lds > 160 * 1024) return fail(h, "ev_load_voice_quality: nfft=%d H=%d W=%d need %zu bytes of LDS, over 160 KiB", nfft, H, W, w.lds);
    VoiceQW& cur = h->voiceq;
    if (cur.loaded) { if (drop_owned(h, {(void*)cur.t.basis})) return 1; cur = VoiceQW(); }
    const size_t n_basis = (size_t)W * NB, n_cep = (size_t)t.NBp * NQ;
    char* blk = nullptr;
    const size_t o_cep = 2 * n_basis, o_sw = o_cep + n_cep, o_fw = o_sw + 2 * (size_t)NB;   // in doubles from the block's start, behind the basis
    auto rest = [&](char* b, const double* d_tw) {
        double* d = (double*)b;
        hipError_t e = hipMemcpy(d + o_sw, slope_w, (size_t)2 * NB * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d + o_fw, fit_w, (size_t)NQ * sizeof(double), hipMemcpyHostToDevice);
        VoiceQCepParams pc{d_tw, d + o_cep, nfft, NB, t.NBp, NQ, q_fit};
        if (e == hipSuccess) launch<voiceq_cep_basis_kernel>(h->device, dim3((unsigned)((n_cep + 255) / 256)), dim3(256), 0, (hipStream_t)nullptr, pc);
        return e;
    };
    if (build_dft_basis(h, __func__, "tables", window, twiddle, W, nfft, (o_fw + NQ) * sizeof(double), &blk, rest)) return 1;
    const double* d = (const double*)blk;
    t.basis = (const double2*)blk; t.cep = d + o_cep; t.slope_w = d + o_sw; t.fit_w = d + o_fw;
    h->owned.push_back(blk);
    ++h->n_allocs;                          // (one block: both bases, slope_w and fit_w; 9.7 MB at W = nfft = 1024 with 319 quefrencies)
    w.loaded = true;
    cur = w;
    return 0;
}

int ev_voice_quality(ev_handle* h, const float* d_x, const int32_t* d_len, int B, int L, double power_floor,
                     double* d_frame, int32_t* d_peak, double* d_cepstrum, void* stream) {
    if (enter(h)) return 1;
    const VoiceQW& w = h->voiceq;
    if (!w.loaded) return fail(h, "ev_voice_quality: tables not loaded (ev_load_voice_quality)");
    if (check_batch(h, __func__, B)) return 1;
    if (L < 1) return fail(h, "ev_voice_quality: L=%d must be at least 1", L);
    if (!d_x) return fail(h, "ev_voice_quality: d_x must be non-null");
    if (!(power_floor > 0.0) || !std::isfinite(power_floor)) return fail(h, "ev_voice_quality: power_floor=%g must be finite and greater than 0", power_floor);
    if (!d_frame || !d_peak) return fail(h, "ev_voice_quality: d_frame and d_peak must be non-null");
    if (L / w.t.H > 0x7fffffef) return fail(h, "ev_voice_quality: L=%d at H=%d has more frames than an int32 tile index holds", L, w.t.H);
    h->stream = (hipStream_t)stream;
    const int NF = frames_of(L, w.t.H);
    VoiceQParams pv{d_x, d_len, d_frame, d_peak, d_cepstrum, w.t, L, NF, power_floor};
    launch<voice_quality_kernel>(h->device, dim3((unsigned)((NF + 15) / 16), (unsigned)B), dim3(256), w.lds, h->stream, pv);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// Formants: Burg's linear prediction, the roots of the prediction polynomial and the formants per frame (formants_kernel, ev_analysis_kernels.h; the
// definition: include/emojivoice.h).  A load owns one device block, the window; the starting points of the root finder travel in the kernel's
// arguments; a call needs no arena.
int ev_load_formants(ev_handle* h, const double* window, int W, int H, int order, double pre_emphasis, double sr, double f_lo, int n_formants) {
    if (enter(h)) return 1;
    if (!window) return fail(h, "ev_load_formants: window must be non-null (HOST, W doubles)");
    if (order < 2 || order > 32) return fail(h, "ev_load_formants: order=%d outside 2 <= order <= 32", order);
    if (W < 8 || W > 1024 || W <= 2 * order) return fail(h, "ev_load_formants: W=%d outside 8 <= W <= 1024 with W > 2 order = %d", W, 2 * order);
    if (H < 1 || H > 512) return fail(h, "ev_load_formants: H=%d outside 1 <= H <= 512", H);
    if (n_formants < 1 || n_formants > 16) return fail(h, "ev_load_formants: n_formants=%d outside 1 <= n_formants <= 16", n_formants);
    if (!(pre_emphasis >= 0.0 && pre_emphasis < 1.0)) return fail(h, "ev_load_formants: pre_emphasis=%g outside 0 <= pre_emphasis < 1", pre_emphasis);
    if (!(sr > 0.0) || !std::isfinite(sr)) return fail(h, "ev_load_formants: sr=%g must be positive and finite", sr);
    if (!(f_lo > 0.0 && f_lo < sr / 4.0)) return fail(h, "ev_load_formants: f_lo=%g outside 0 < f_lo < sr / 4 = %g", f_lo, sr / 4.0);
    if (check_finite(h, __func__, "window", window, W)) return 1;
    FormantW w;
    w.W = W; w.H = H; w.order = order; w.nform = n_formants; w.pre = pre_emphasis; w.sr = sr; w.f_lo = f_lo;
    w.R = 1;
    while (64 * w.R < W) w.R *= 2;                                      // 1, 2, 4, 8 or 16 samples per lane
    for (int i = 0; i < order; ++i) {
        const double ang = 2.0 * M_PI * (double)i / (double)order + 0.4;
        w.z0[2 * i] = 0.9 * std::cos(ang); w.z0[2 * i + 1] = 0.9 * std::sin(ang);
    }
    void* blk = nullptr;                                                // the new block first: a failed load leaves the tables in use as they are
    if (hipMalloc(&blk, (size_t)W * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); return fail(h, "ev_load_formants: hipMalloc of the window failed"); }
    if (hipMemcpy(blk, window, (size_t)W * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError(); hipFree(blk);
        return fail(h, "ev_load_formants: the copy of the window failed");
    }
    FormantW& cur = h->fmt;
    if (cur.loaded) { if (drop_owned(h, {(void*)cur.win})) { hipFree(blk); return 1; } cur = FormantW(); }
    w.win = (double*)blk;
    h->owned.push_back(blk);
    ++h->n_allocs;
    w.loaded = true;
    cur = w;
    return 0;
}

int ev_formants(ev_handle* h, const float* d_x, const int32_t* d_len, int B, int L, double power_floor, double* d_lpc, double* d_formant,
                int32_t* d_count, void* stream) {
    if (enter(h)) return 1;
    const FormantW& w = h->fmt;
    if (!w.loaded) return fail(h, "ev_formants: tables not loaded (ev_load_formants)");
    if (check_batch(h, __func__, B)) return 1;
    if (L < 1) return fail(h, "ev_formants: L=%d must be at least 1", L);
    if (!d_x) return fail(h, "ev_formants: d_x must be non-null");
    if (!(power_floor > 0.0) || !std::isfinite(power_floor)) return fail(h, "ev_formants: power_floor=%g must be finite and greater than 0", power_floor);
    if (!d_formant || !d_count) return fail(h, "ev_formants: d_formant and d_count must be non-null");
    h->stream = (hipStream_t)stream;
    FormantParams p{};
    p.x = d_x; p.len = d_len; p.win = w.win; p.lpc = d_lpc; p.formant = d_formant; p.count = d_count;
    p.L = L; p.NF = frames_of(L, w.H); p.W = w.W; p.H = w.H; p.order = w.order; p.nform = w.nform;
    p.pre = w.pre; p.floor = power_floor; p.f_scale = w.sr / (2.0 * M_PI); p.bw_scale = w.sr / M_PI; p.f_lo = w.f_lo; p.f_hi = w.sr / 2.0 - w.f_lo;
    for (int i = 0; i < 64; ++i) p.z0[i] = w.z0[i];
    const dim3 grid((unsigned)((p.NF - 1) / 4 + 1), (unsigned)B), block(256);
    switch (w.R) {
        case 1: launch<formants_kernel<1>>(h->device, grid, block, 0, h->stream, p); break;
        case 2: launch<formants_kernel<2>>(h->device, grid, block, 0, h->stream, p); break;
        case 4: launch<formants_kernel<4>>(h->device, grid, block, 0, h->stream, p); break;
        case 8: launch<formants_kernel<8>>(h->device, grid, block, 0, h->stream, p); break;
        default: launch<formants_kernel<16>>(h->device, grid, block, 0, h->stream, p); break;
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

// Perturbation: jitter, shimmer, RAP and the harmonic strength per frame at the lags ev_pitch_yin wrote (perturbation_kernel, ev_analysis_kernels.h;
// the definition: include/emojivoice.h).  No load step, no tables, no arena: one launch whose arguments carry everything.
int ev_perturbation(ev_handle* h, const float* d_x, const int32_t* d_len, int B, int L, int hop_length, const int32_t* d_lag, int n_cycles,
                    int corr_length, double period_factor, double amplitude_factor, double power_floor, double* d_frame, int32_t* d_count,
                    int32_t* d_marks, void* stream) {
    if (enter(h)) return 1;
    if (check_batch(h, __func__, B)) return 1;
    if (L < 1) return fail(h, "ev_perturbation: L=%d must be at least 1", L);
    if (hop_length < 1 || hop_length > 4096) return fail(h, "ev_perturbation: hop_length=%d outside 1 <= hop_length <= 4096", hop_length);
    if (n_cycles < 1 || n_cycles > 16) return fail(h, "ev_perturbation: n_cycles=%d outside 1 <= n_cycles <= 16", n_cycles);
    if (corr_length < 8 || corr_length > 4096) return fail(h, "ev_perturbation: corr_length=%d outside 8 <= corr_length <= 4096", corr_length);
    if (!(period_factor > 1.0) || !std::isfinite(period_factor))
        return fail(h, "ev_perturbation: period_factor=%g must be finite and greater than 1", period_factor);
    if (!(amplitude_factor > 1.0) || !std::isfinite(amplitude_factor))
        return fail(h, "ev_perturbation: amplitude_factor=%g must be finite and greater than 1", amplitude_factor);
    if (!(power_floor > 0.0) || !std::isfinite(power_floor)) return fail(h, "ev_perturbation: power_floor=%g must be finite and greater than 0", power_floor);
    if (!d_x) return fail(h, "ev_perturbation: d_x must be non-null");
    if (!d_lag) return fail(h, "ev_perturbation: d_lag must be non-null");
    if (!d_frame || !d_count) return fail(h, "ev_perturbation: d_frame and d_count must be non-null");
    h->stream = (hipStream_t)stream;
    PerturbParams p{};
    p.x = d_x; p.len = d_len; p.lag = d_lag; p.frame = d_frame; p.count = d_count; p.marks = d_marks;
    p.L = L; p.NF = frames_of(L, hop_length); p.H = hop_length; p.nc = n_cycles; p.W = corr_length;
    p.pf = period_factor; p.af = amplitude_factor; p.floor2 = power_floor * power_floor;
    launch<perturbation_kernel>(h->device, dim3((unsigned)((p.NF - 1) / 4 + 1), (unsigned)B), dim3(256), 0, h->stream, p);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// Harmonic differences: H1-H2, H1-A3 and the harmonic levels at F1, F2, F3 over H1 per frame, at the periods ev_pitch_yin wrote and the formants
// ev_formants wrote (harmonics_kernel, ev_analysis_kernels.h; the definition: include/emojivoice.h).  One device block per load holds the basis; a
// call needs no arena.
int ev_load_harmonics(ev_handle* h, const double* window, const double* twiddle, int W, int H, int nfft, double sr, int n_harm, double search,
                      double min_spacing, double a3_range) {
    if (enter(h)) return 1;
    if (!window || !twiddle) return fail(h, "ev_load_harmonics: window and twiddle must be non-null (HOST)");
    if (check_dft_geometry(h, __func__, W, H, nfft, 2048)) return 1;
    if (!(sr > 0.0) || !std::isfinite(sr)) return fail(h, "ev_load_harmonics: sr=%g must be positive and finite", sr);
    if (n_harm < 1 || n_harm > 64) return fail(h, "ev_load_harmonics: n_harm=%d outside 1 <= n_harm <= 64", n_harm);
    if (!(search > 0.0 && search <= 0.5)) return fail(h, "ev_load_harmonics: search=%g outside 0 < search <= 0.5", search);
    if (!(min_spacing >= 2.0) || !std::isfinite(min_spacing)) return fail(h, "ev_load_harmonics: min_spacing=%g must be finite and at least 2", min_spacing);
    if (!(a3_range >= 0.0 && a3_range <= 0.5)) return fail(h, "ev_load_harmonics: a3_range=%g outside 0 <= a3_range <= 0.5", a3_range);
    if (check_finite(h, __func__, "window", window, W) || check_finite(h, __func__, "twiddle", twiddle, 2 * nfft)) return 1;
    HarmW w;
    HarmTables& t = w.t;
    t.W = W; t.H = H; t.nfft = nfft; t.NB = nfft / 2 + 1; t.skew = dft_skew(H); t.n_harm = n_harm;
    t.S = t.NB + ((2 - t.NB) % 32 + 32) % 32;                           // the smallest S >= NB with S = 2 mod 32
    t.bin_hz = sr / (double)nfft; t.sr = sr; t.search = search; t.min_spacing = min_spacing; t.a3_range = a3_range;
    // the log-spectrum, the harmonics, the four waves' live counts (64 words), the skewed span
    w.lds = (size_t)16 * t.S * sizeof(double) + (size_t)16 * n_harm * 2 * sizeof(double) + 64 * sizeof(int32_t)
          + (size_t)dft_span_words(15 * H + W, H, t.skew) * sizeof(float);
    if (w.lds > 160 * 1024)
        return fail(h, "ev_load_harmonics: nfft=%d H=%d W=%d n_harm=%d need %zu bytes of LDS, over 160 KiB", nfft, H, W, n_harm, w.lds);
    char* blk = nullptr;                                                // the new block first: a failed load leaves the tables in use as they are
    auto none = [](char*, const double*) { return hipSuccess; };
    if (build_dft_basis(h, __func__, "basis", window, twiddle, W, nfft, (size_t)W * t.NB * sizeof(double2), &blk, none)) return 1;
    HarmW& cur = h->harm;
    if (cur.loaded) { if (drop_owned(h, {(void*)cur.t.basis})) { hipFree(blk); return 1; } cur = HarmW(); }
    t.basis = (const double2*)blk;
    h->owned.push_back(blk);
    ++h->n_allocs;                          // (one block: the basis, 8.4 MB at W = nfft = 1024)
    w.loaded = true;
    cur = w;
    return 0;
}

int ev_harmonics(ev_handle* h, const float* d_x, const int32_t* d_len, int B, int L, const float* d_period, const double* d_formant,
                 const int32_t* d_fcount, int n_formants, double power_floor, double* d_frame, int32_t* d_count, double* d_harm, void* stream) {
    if (enter(h)) return 1;
    const HarmW& w = h->harm;
    if (!w.loaded) return fail(h, "ev_harmonics: tables not loaded (ev_load_harmonics)");
    if (check_batch(h, __func__, B)) return 1;
    if (L < 1) return fail(h, "ev_harmonics: L=%d must be at least 1", L);
    if (L / w.t.H > 0x7fffffef) return fail(h, "ev_harmonics: L=%d at H=%d has more frames than an int32 tile index holds", L, w.t.H);
    if (!(power_floor > 0.0) || !std::isfinite(power_floor)) return fail(h, "ev_harmonics: power_floor=%g must be finite and greater than 0", power_floor);
    if (!d_x) return fail(h, "ev_harmonics: d_x must be non-null");
    if (!d_period) return fail(h, "ev_harmonics: d_period must be non-null");
    if (!d_frame || !d_count) return fail(h, "ev_harmonics: d_frame and d_count must be non-null");
    if ((d_formant == nullptr) != (d_fcount == nullptr)) return fail(h, "ev_harmonics: d_formant and d_fcount must both be given or both be null");
    if (d_formant && (n_formants < 1 || n_formants > 16)) return fail(h, "ev_harmonics: n_formants=%d outside 1 <= n_formants <= 16", n_formants);
    h->stream = (hipStream_t)stream;
    const int NF = frames_of(L, w.t.H);
    HarmParams ph{d_x, d_len, d_period, d_formant, d_fcount, d_frame, d_count, d_harm, w.t, L, NF, d_formant ? n_formants : 0, power_floor};
    launch<harmonics_kernel>(h->device, dim3((unsigned)((NF + 15) / 16), (unsigned)B), dim3(256), w.lds, h->stream, ph);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// Auditory descriptors: loudness of an auditory spectrum, spectral flux, power and MFCC per frame (auditory_kernel, ev_analysis_kernels.h; the
// definition: include/emojivoice.h).  One device block per load holds the basis, the mel table padded with zeros to (NBp, NMp), eq and dct; a call
// needs no arena.
int ev_load_auditory(ev_handle* h, const double* window, const double* twiddle, int W, int H, int nfft, const double* mel_w, int n_mel,
                     const double* eq, const double* dct, int n_ceps, int k_lo, int k_hi, double compress) {
    if (enter(h)) return 1;
    if (!window || !twiddle || !mel_w || !eq || !dct)
        return fail(h, "ev_load_auditory: window, twiddle, mel_w, eq and dct must be non-null (HOST)");
    if (check_dft_geometry(h, __func__, W, H, nfft, 1024)) return 1;
    const int NB = nfft / 2 + 1;
    if (n_mel < 1 || n_mel > 64) return fail(h, "ev_load_auditory: n_mel=%d outside 1 <= n_mel <= 64", n_mel);
    if (n_ceps < 1 || n_ceps > 16) return fail(h, "ev_load_auditory: n_ceps=%d outside 1 <= n_ceps <= 16", n_ceps);
    if (k_lo < 0 || k_lo >= k_hi || k_hi > NB) return fail(h, "ev_load_auditory: k_lo=%d k_hi=%d outside 0 <= k_lo < k_hi <= %d", k_lo, k_hi, NB);
    if (!(compress > 0.0 && compress <= 1.0)) return fail(h, "ev_load_auditory: compress=%g outside 0 < compress <= 1", compress);
    if (check_finite(h, __func__, "window", window, W) || check_finite(h, __func__, "twiddle", twiddle, 2 * nfft)
        || check_finite(h, __func__, "mel_w", mel_w, NB * n_mel) || check_finite(h, __func__, "eq", eq, n_mel)
        || check_finite(h, __func__, "dct", dct, n_mel * n_ceps)) return 1;
    for (int j = 0; j < NB * n_mel; ++j) if (mel_w[j] < 0.0) return fail(h, "ev_load_auditory: mel_w[%d] = %g must not be negative", j, mel_w[j]);
    for (int j = 0; j < n_mel; ++j) if (!(eq[j] > 0.0)) return fail(h, "ev_load_auditory: eq[%d] = %g must be greater than 0", j, eq[j]);
    AudW w;
    AudTables& t = w.t;
    t.W = W; t.H = H; t.nfft = nfft; t.NB = NB; t.NBp = (NB + 3) / 4 * 4; t.skew = dft_skew(H);
    t.S = NB + ((2 - NB) % 32 + 32) % 32;                               // the smallest S >= NB with S = 2 mod 32
    t.n_mel = n_mel; t.NMp = (n_mel + 15) / 16 * 16; t.LS = t.NMp + 1; t.n_ceps = n_ceps; t.k_lo = k_lo; t.k_hi = k_hi; t.compress = compress;
    // the power spectrum, log(Ef) and pow(eq Ef, compress), the skewed span
    w.lds = (size_t)16 * t.S * sizeof(double) + (size_t)32 * t.LS * sizeof(double) + (size_t)dft_span_words(15 * H + W, H, t.skew) * sizeof(float);
    if (w.lds > 160 * 1024)
        return fail(h, "ev_load_auditory: nfft=%d H=%d W=%d n_mel=%d need %zu bytes of LDS, over 160 KiB", nfft, H, W, n_mel, w.lds);
    const size_t n_basis = (size_t)W * NB, n_melp = (size_t)t.NBp * t.NMp;
    const size_t o_mel = 2 * n_basis, o_eq = o_mel + n_melp, o_dct = o_eq + (size_t)n_mel;   // in doubles from the block's start, behind the basis
    std::vector<double> melp(n_melp, 0.0);
    for (int k = 0; k < NB; ++k) for (int m = 0; m < n_mel; ++m) melp[(size_t)k * t.NMp + m] = mel_w[(size_t)k * n_mel + m];
    char* blk = nullptr;                                                // the new block first: a failed load leaves the tables in use as they are
    auto rest = [&](char* b, const double*) {
        double* d = (double*)b;
        hipError_t e = hipMemcpy(d + o_mel, melp.data(), n_melp * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d + o_eq, eq, (size_t)n_mel * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d + o_dct, dct, (size_t)n_mel * n_ceps * sizeof(double), hipMemcpyHostToDevice);
        return e;
    };
    if (build_dft_basis(h, __func__, "tables", window, twiddle, W, nfft, (o_dct + (size_t)n_mel * n_ceps) * sizeof(double), &blk, rest)) return 1;
    AudW& cur = h->aud;
    if (cur.loaded) { if (drop_owned(h, {(void*)cur.t.basis})) { hipFree(blk); return 1; } cur = AudW(); }
    const double* d = (const double*)blk;
    t.basis = (const double2*)blk; t.mel = d + o_mel; t.eq = d + o_eq; t.dct = d + o_dct;
    h->owned.push_back(blk);
    ++h->n_allocs;                          // (one block: the basis, mel, eq and dct; 8.5 MB at W = nfft = 1024 with 26 bands)
    w.loaded = true;
    cur = w;
    return 0;
}

int ev_auditory(ev_handle* h, const float* d_x, const int32_t* d_len, int B, int L, double power_floor, double* d_frame, double* d_mfcc,
                int32_t* d_flags, double* d_bands, void* stream) {
    if (enter(h)) return 1;
    const AudW& w = h->aud;
    if (!w.loaded) return fail(h, "ev_auditory: tables not loaded (ev_load_auditory)");
    if (check_batch(h, __func__, B)) return 1;
    if (L < 1) return fail(h, "ev_auditory: L=%d must be at least 1", L);
    if (!d_x) return fail(h, "ev_auditory: d_x must be non-null");
    if (!(power_floor > 0.0) || !std::isfinite(power_floor)) return fail(h, "ev_auditory: power_floor=%g must be finite and greater than 0", power_floor);
    if (!d_frame || !d_mfcc || !d_flags) return fail(h, "ev_auditory: d_frame, d_mfcc and d_flags must be non-null");
    if (L / w.t.H > 0x7fffffef) return fail(h, "ev_auditory: L=%d at H=%d has more frames than an int32 tile index holds", L, w.t.H);
    h->stream = (hipStream_t)stream;
    const int NF = frames_of(L, w.t.H);
    AudParams pa{d_x, d_len, d_frame, d_mfcc, d_flags, d_bands, w.t, L, NF, power_floor};
    launch<auditory_kernel>(h->device, dim3((unsigned)((NF + 14) / 15), (unsigned)B), dim3(256), w.lds, h->stream, pa);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// Contour functionals: moments, order statistics, slopes of the rising and falling parts, peaks, runs and gaps of every contour of a batch
// (functionals_kernel, ev_analysis_kernels.h; the definition: include/emojivoice.h).  No load step, no tables, no arena: one launch, a workgroup
// per contour, whose arguments carry everything (the percentiles' q travel by value).
int ev_functionals(ev_handle* h, const double* d_v, const uint8_t* d_mask, const int32_t* d_len, int B, int K, int F, const double* q, int NQ,
                   double* d_stat, int32_t* d_count, void* stream) {
    if (enter(h)) return 1;
    if (check_batch(h, __func__, B)) return 1;
    if (K < 1 || K > 65535) return fail(h, "ev_functionals: K=%d outside 1 <= K <= 65535", K);
    if (F < 1 || F > 4096) return fail(h, "ev_functionals: F=%d outside 1 <= F <= 4096", F);
    if (NQ < 0 || NQ > 16) return fail(h, "ev_functionals: NQ=%d outside 0 <= NQ <= 16", NQ);
    if (NQ > 0 && !q) return fail(h, "ev_functionals: q must be non-null (HOST) when NQ > 0");
    if (check_finite(h, __func__, "q", q, NQ)) return 1;
    for (int r = 0; r < NQ; ++r) if (!(q[r] >= 0.0 && q[r] <= 1.0)) return fail(h, "ev_functionals: q[%d]=%g outside 0 <= q <= 1", r, q[r]);
    if (!d_v) return fail(h, "ev_functionals: d_v must be non-null");
    if (!d_stat) return fail(h, "ev_functionals: d_stat must be non-null");
    if (!d_count) return fail(h, "ev_functionals: d_count must be non-null");
    h->stream = (hipStream_t)stream;
    FuncParams p{};
    p.v = d_v; p.mask = d_mask; p.len = d_len; p.stat = d_stat; p.count = d_count;
    p.K = K; p.F = F; p.NQ = NQ; p.P = 256;
    while (p.P < F) p.P <<= 1;
    for (int r = 0; r < NQ; ++r) p.q[r] = q[r];
    // 64 doubles and 64 words of hand-over, then u (8 B) and g, st (2 B each) per frame: 48.5 KiB at F = 4096
    launch<functionals_kernel>(h->device, dim3((unsigned)K, (unsigned)B), dim3(256), 512 + (size_t)12 * p.P, h->stream, p);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// Formant tracking: a Viterbi pass over the candidates ev_formants wrote, one workgroup per row (formant_track_kernel, ev_analysis_kernels.h; the
// definition: include/emojivoice.h).  No load step, no tables, no arena: one launch whose arguments carry the reference frequencies and the three
// costs.  LDS in doubles: delta 2 S, the states' tuples S, two table buffers of 16 x 17 + 256 each, the ring of four staged frames 4 x 48, ref 16;
// then four words of m: 10 368 bytes at S = 10, 34 704 at S = 1024.
int ev_formant_track(ev_handle* h, const double* d_formant, const int32_t* d_count, int B, int NF, int n_cand, int n_tracks, const double* ref,
                     double cost_f, double cost_b, double cost_j, uint16_t* d_back, double* d_track, int32_t* d_sel, double* d_cost, void* stream) {
    if (enter(h)) return 1;
    if (check_batch(h, __func__, B)) return 1;
    if (NF < 1) return fail(h, "ev_formant_track: NF=%d must be at least 1", NF);
    if (n_cand < 1 || n_cand > 16) return fail(h, "ev_formant_track: n_cand=%d outside 1 <= n_cand <= 16", n_cand);
    if (n_tracks < 1 || n_tracks > n_cand) return fail(h, "ev_formant_track: n_tracks=%d outside 1 <= n_tracks <= n_cand = %d", n_tracks, n_cand);
    long long S = 1;
    for (int i = 1; i <= n_tracks; ++i) S = S * (n_cand - n_tracks + i) / i;                 // C(n_cand, n_tracks), exact at every step
    if (S > 1024) return fail(h, "ev_formant_track: S=%lld states = C(n_cand=%d, n_tracks=%d) over the limit S <= 1024", S, n_cand, n_tracks);
    if (!ref) return fail(h, "ev_formant_track: ref (HOST, n_tracks doubles) must be non-null");
    for (int k = 0; k < n_tracks; ++k)
        if (!(ref[k] > 0.0) || !std::isfinite(ref[k])) return fail(h, "ev_formant_track: ref[%d]=%g must be finite and greater than 0", k, ref[k]);
    if (!(cost_f >= 0.0) || !std::isfinite(cost_f)) return fail(h, "ev_formant_track: cost_f=%g must be finite and at least 0", cost_f);
    if (!(cost_b >= 0.0) || !std::isfinite(cost_b)) return fail(h, "ev_formant_track: cost_b=%g must be finite and at least 0", cost_b);
    if (!(cost_j >= 0.0) || !std::isfinite(cost_j)) return fail(h, "ev_formant_track: cost_j=%g must be finite and at least 0", cost_j);
    if (!d_formant || !d_count) return fail(h, "ev_formant_track: d_formant and d_count must be non-null");
    if (!d_back) return fail(h, "ev_formant_track: d_back must be non-null (B x NF x S uint16 of the caller's)");
    if (!d_track || !d_sel) return fail(h, "ev_formant_track: d_track and d_sel must be non-null");
    h->stream = (hipStream_t)stream;
    FormantTrackParams p{};
    p.formant = d_formant; p.count = d_count; p.back = d_back; p.track = d_track; p.sel = d_sel; p.cost = d_cost;
    p.NF = NF; p.nc = n_cand; p.nt = n_tracks; p.S = (int)S;
    p.G = 1;
    while (p.S * p.G * 2 <= 64) p.G *= 2;                                                    // lanes per target state: S G <= 64 (S = 10: 4)
    p.cf = cost_f; p.cb = cost_b; p.cj = cost_j;
    for (int k = 0; k < n_tracks; ++k) p.ref[k] = ref[k];
    const int NT = std::min(1024, round_up(p.S, 64));
    const size_t smem = (3 * (size_t)p.S + 2 * FTRACK_TABLE + 4 * 48 + 16) * sizeof(double) + 4 * sizeof(int);
    launch<formant_track_kernel>(h->device, dim3(B), dim3(NT), smem, h->stream, p);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// Modulation spectra of contours: per contour the pooled power on a grid of modulation frequencies and the peak of up to four bands
// (modulation_kernel, ev_analysis_kernels.h; the definition: include/emojivoice.h).  No load step, no tables, no arena: one launch, a workgroup
// per contour, whose arguments carry the grid and the bands.
int ev_modulation(ev_handle* h, const double* d_v, const uint8_t* d_mask, const int32_t* d_len, int B, int K, int F, double nu0, double dnu, int NM,
                  int min_run, double min_cycles, const int32_t* band, int NBAND, double* d_spec, int32_t* d_weight, double* d_peak, double* d_stat,
                  int32_t* d_count, void* stream) {
    if (enter(h)) return 1;
    if (check_batch(h, __func__, B)) return 1;
    if (K < 1 || K > 65535) return fail(h, "ev_modulation: K=%d outside 1 <= K <= 65535", K);
    if (F < 1 || F > 4096) return fail(h, "ev_modulation: F=%d outside 1 <= F <= 4096", F);
    if (NM < 1 || NM > 128) return fail(h, "ev_modulation: NM=%d outside 1 <= NM <= 128", NM);
    if (!std::isfinite(nu0) || !(nu0 > 0.0)) return fail(h, "ev_modulation: nu0=%g must be finite and greater than 0", nu0);
    if (!std::isfinite(dnu) || !(dnu > 0.0)) return fail(h, "ev_modulation: dnu=%g must be finite and greater than 0", dnu);
    if (!(nu0 + (double)(NM - 1) * dnu <= 0.5))
        return fail(h, "ev_modulation: the grid ends at nu0 + (NM - 1) dnu = %g cycles per frame, over the limit 0.5", nu0 + (double)(NM - 1) * dnu);
    if (min_run < 3 || min_run > F) return fail(h, "ev_modulation: min_run=%d outside 3 <= min_run <= F = %d", min_run, F);
    if (!std::isfinite(min_cycles) || !(min_cycles >= 0.0)) return fail(h, "ev_modulation: min_cycles=%g must be finite and at least 0", min_cycles);
    if (NBAND < 0 || NBAND > 4) return fail(h, "ev_modulation: NBAND=%d outside 0 <= NBAND <= 4", NBAND);
    if (NBAND > 0 && !band) return fail(h, "ev_modulation: band must be non-null (HOST) when NBAND > 0");
    for (int i = 0; i < NBAND; ++i)
        if (band[2 * i] < 0 || band[2 * i] >= band[2 * i + 1] || band[2 * i + 1] > NM)
            return fail(h, "ev_modulation: band[%d] = [%d, %d) outside 0 <= j_lo < j_hi <= NM = %d", i, band[2 * i], band[2 * i + 1], NM);
    if (!d_v) return fail(h, "ev_modulation: d_v must be non-null");
    if (!d_spec) return fail(h, "ev_modulation: d_spec must be non-null");
    if (!d_weight) return fail(h, "ev_modulation: d_weight must be non-null");
    if (NBAND > 0 && !d_peak) return fail(h, "ev_modulation: d_peak must be non-null when NBAND > 0");
    if (!d_stat) return fail(h, "ev_modulation: d_stat must be non-null");
    if (!d_count) return fail(h, "ev_modulation: d_count must be non-null");
    h->stream = (hipStream_t)stream;
    ModParams p{};
    p.v = d_v; p.mask = d_mask; p.len = d_len; p.spec = d_spec; p.weight = d_weight; p.peak = NBAND ? d_peak : nullptr; p.stat = d_stat; p.count = d_count;
    p.K = K; p.F = F; p.NM = NM; p.NBAND = NBAND; p.min_run = min_run;
    p.MR = std::max(2, round_up((F + 1) / 4, 2));                                    // the most runs of >= 3 frames, each a frame apart, that F frames hold
    p.nu0 = nu0; p.dnu = dnu; p.min_cycles = min_cycles;
    for (int i = 0; i < 2 * NBAND; ++i) p.band[i] = band[i];
    // wr (8 B a frame), the runs' window sums and packed bounds (12 B a run), the pooled spectrum and weights (128 x 12 B), 24 words: 45.6 KiB at 4096
    const size_t smem = ((size_t)F + (F & 1) + p.MR + 128) * sizeof(double) + ((size_t)p.MR + 128 + 24) * sizeof(int);
    launch<modulation_kernel>(h->device, dim3((unsigned)K, (unsigned)B), dim3(256), smem, h->stream, p);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// Speech rate and pauses: the power contour, the sounding / silent segmentation and the syllable nuclei of every row (speech_power_kernel and
// speech_rate_rows_kernel, ev_analysis_kernels.h; the definition: include/emojivoice.h).  A load owns one device block, the window; its sum is
// formed here, once, in ascending order.  Arena of a call without d_power: the power contour, B x NF doubles.
int ev_load_speech_rate(ev_handle* h, const double* window, int W, int H) {
    STOI_EXACT
    if (enter(h)) return 1;
    if (!window) return fail(h, "ev_load_speech_rate: window must be non-null (HOST, W doubles)");
    if (W < 8 || W > 4096 || W % 2) return fail(h, "ev_load_speech_rate: W=%d must be even with 8 <= W <= 4096", W);
    if (H < 64 || H > 1024 || H % 64) return fail(h, "ev_load_speech_rate: H=%d must be a multiple of 64 with 64 <= H <= 1024", H);
    if (check_finite(h, __func__, "window", window, W)) return 1;
    double sw = 0.0;
    for (int j = 0; j < W; ++j) sw = sw + window[j];
    if (!(sw > 0.0) || !std::isfinite(sw)) return fail(h, "ev_load_speech_rate: the window's sum sw=%g must be finite and greater than 0", sw);
    RateW t;                                                            // the new block first: a failed load leaves the tables in use as they are
    if (dev_upload(h, std::vector<double>(window, window + W), &t.win)) return 1;
    ++h->n_allocs;
    t.W = W; t.H = H; t.sw = sw; t.loaded = true;
    RateW& cur = h->rate;
    if (cur.loaded && drop_owned(h, {(void*)cur.win})) return 1;
    cur = t;
    return 0;
}

int ev_speech_rate(ev_handle* h, const float* d_x, const int32_t* d_len, const uint8_t* d_voiced, int B, int L, double power_floor,
                   double rank_fraction, double silence_ratio, double dip_ratio, int min_pause, int min_sound, double* d_power, uint8_t* d_mark,
                   double* d_stat, int32_t* d_count, void* stream) {
    if (enter(h)) return 1;
    const RateW& w = h->rate;
    if (!w.loaded) return fail(h, "ev_speech_rate: tables not loaded (ev_load_speech_rate)");
    if (check_batch(h, __func__, B)) return 1;
    if (L < 1) return fail(h, "ev_speech_rate: L=%d must be at least 1", L);
    const int NF = frames_of(L, w.H);
    if (NF > RATE_MAXF) return fail(h, "ev_speech_rate: NF=%d frames (L=%d at H=%d) over the limit NF <= %d", NF, L, w.H, RATE_MAXF);
    if (!(power_floor > 0.0) || !std::isfinite(power_floor)) return fail(h, "ev_speech_rate: power_floor=%g must be finite and greater than 0", power_floor);
    if (!(rank_fraction >= 0.0 && rank_fraction < 1.0)) return fail(h, "ev_speech_rate: rank_fraction=%g outside 0 <= rank_fraction < 1", rank_fraction);
    if (!(silence_ratio > 0.0 && silence_ratio < 1.0)) return fail(h, "ev_speech_rate: silence_ratio=%g outside 0 < silence_ratio < 1", silence_ratio);
    if (!(dip_ratio >= 1.0) || !std::isfinite(dip_ratio)) return fail(h, "ev_speech_rate: dip_ratio=%g must be finite and at least 1", dip_ratio);
    if (min_pause < 1 || min_pause > 4096) return fail(h, "ev_speech_rate: min_pause=%d outside 1 <= min_pause <= 4096", min_pause);
    if (min_sound < 1 || min_sound > 4096) return fail(h, "ev_speech_rate: min_sound=%d outside 1 <= min_sound <= 4096", min_sound);
    if (!d_x) return fail(h, "ev_speech_rate: d_x must be non-null");
    if (!d_stat) return fail(h, "ev_speech_rate: d_stat must be non-null");
    if (!d_count) return fail(h, "ev_speech_rate: d_count must be non-null");
    h->stream = (hipStream_t)stream;
    double* power = d_power;
    if (!power) {
        if (scratch_acquire(h, h->rate_ws, (size_t)B * NF * sizeof(double))) return 1;
        power = (double*)h->rate_ws.p;
    }
    RatePowerParams pp{d_x, d_len, w.win, power, L, NF, w.W, w.H, w.sw};
    // the tile's span of samples as float: 7.4 KiB at H = 64, W = 1024; 76 KiB at H = 1024, W = 4096
    launch<speech_power_kernel>(h->device, dim3((unsigned)((NF - 1) / RATE_T + 1), (unsigned)B), dim3(256),
                                ((size_t)(RATE_T - 1) * w.H + w.W) * sizeof(float), h->stream, pp);
    RateRowsParams pr{power, d_len, d_voiced, d_mark, d_stat, d_count, L, NF, w.H, min_pause, min_sound, power_floor, rank_fraction, silence_ratio, dip_ratio};
    // the row's power (8 B a frame) and flags (1 B), 32 doubles and 224 words of hand-over: 145.1 KiB at NF = 16384
    launch<speech_rate_rows_kernel>(h->device, dim3((unsigned)B), dim3(1024), (size_t)9 * NF + 1152, h->stream, pr);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// Spectral envelope and mel-cepstrum: CheapTrick on ev_pitch_yin's periods and freqt (envelope_power_kernel and envelope_cepstrum_kernel,
// ev_analysis_kernels.h; the definition: include/emojivoice.h).  H follows the DFT families' rule, 1 <= H <= 512.  A load owns one device block: the
// plain DFT basis (stft_dist_basis_kernel under a window of ones, W = nfft), the cepstral basis (voiceq_cep_basis_kernel at q_fit = 0, NQ = NB) and
// the warp table, transposed to (NBp, n_mcep) with zero rows from NB on and row 0 halved (c[0] = c'[0] / 2).  Arena of a call: the power spectra,
// B x NF x NB doubles.
int ev_load_envelope(ev_handle* h, const double* twiddle, int H, int nfft, double sr, double default_period, double q1, const double* warp, int n_mcep) {
    if (enter(h)) return 1;
    if (!twiddle || !warp) return fail(h, "ev_load_envelope: twiddle and warp must be non-null (HOST)");
    if (nfft < 16 || nfft > 1024 || nfft % 2) return fail(h, "ev_load_envelope: nfft=%d must be even with 16 <= nfft <= 1024", nfft);
    if (H < 1 || H > 512) return fail(h, "ev_load_envelope: H=%d outside 1 <= H <= 512", H);
    if (n_mcep < 1 || n_mcep > 64) return fail(h, "ev_load_envelope: n_mcep=%d outside 1 <= n_mcep <= 64", n_mcep);
    if (!(sr > 0.0) || !std::isfinite(sr)) return fail(h, "ev_load_envelope: sr=%g must be finite and greater than 0", sr);
    if (!std::isfinite(q1)) return fail(h, "ev_load_envelope: q1=%g is not finite", q1);
    const int NB = nfft / 2 + 1, NBp = (NB + 3) / 4 * 4;
    const double T_max = (double)(nfft - 3) / 3.0;
    if (!std::isfinite(default_period)) return fail(h, "ev_load_envelope: default_period=%g is not finite", default_period);
    const double T_def = default_period == 0.0 ? sr / 500.0 : default_period;
    if (!(T_def >= 2.0 && T_def <= T_max))
        return fail(h, "ev_load_envelope: default_period=%g (0: sr / 500) outside 2 <= default_period <= (nfft - 3) / 3 = %g", T_def, T_max);
    if (check_finite(h, __func__, "twiddle", twiddle, 2 * nfft) || check_finite(h, __func__, "warp", warp, n_mcep * NB)) return 1;
    EnvW w;
    EnvTables& t = w.t;
    t.H = H; t.nfft = nfft; t.NB = NB; t.NBp = NBp; t.n_mcep = n_mcep; t.T_max = T_max; t.T_def = T_def; t.q1 = q1;
    const int rows = (nfft + 3) / 4 * 4;
    t.S1 = rows + ((2 - rows) % 32 + 32) % 32;                          // the smallest numbers >= the rows of a frame / of a plane that are 2 mod 32
    t.S = NBp + ((2 - NBp) % 32 + 32) % 32;
    w.lds1 = (size_t)16 * t.S1 * sizeof(double);
    w.lds2 = (size_t)2 * 16 * t.S * sizeof(double);
    if (w.lds1 > 160 * 1024 || w.lds2 > 160 * 1024)
        return fail(h, "ev_load_envelope: nfft=%d needs %zu and %zu bytes of LDS, over 160 KiB", nfft, w.lds1, w.lds2);
    std::vector<double> ones((size_t)nfft, 1.0), wt((size_t)NBp * n_mcep, 0.0);
    for (int m = 0; m < n_mcep; ++m)
        for (int q = 0; q < NB; ++q) wt[(size_t)q * n_mcep + m] = (q == 0 ? 0.5 : 1.0) * warp[(size_t)m * NB + q];
    const size_t n_basis = (size_t)nfft * NB, n_cep = (size_t)NBp * NB;
    const size_t o_cep = 2 * n_basis, o_warp = o_cep + n_cep;          // in doubles from the block's start, behind the basis
    char* blk = nullptr;                                                // the new block first: a failed load leaves the tables in use as they are
    auto rest = [&](char* b, const double* d_tw) {
        double* d = (double*)b;
        hipError_t e = hipMemcpy(d + o_warp, wt.data(), wt.size() * sizeof(double), hipMemcpyHostToDevice);
        VoiceQCepParams pc{d_tw, d + o_cep, nfft, NB, NBp, NB, 0};
        if (e == hipSuccess) launch<voiceq_cep_basis_kernel>(h->device, dim3((unsigned)((n_cep + 255) / 256)), dim3(256), 0, (hipStream_t)nullptr, pc);
        return e;
    };
    if (build_dft_basis(h, __func__, "tables", ones.data(), twiddle, nfft, nfft, (o_warp + wt.size()) * sizeof(double), &blk, rest)) return 1;
    const double* d = (const double*)blk;
    t.basis = (const double2*)blk; t.cep = d + o_cep; t.warp = d + o_warp;
    EnvW& cur = h->env;
    if (cur.loaded && drop_owned(h, {(void*)cur.t.basis})) { hipFree(blk); return 1; }
    h->owned.push_back(blk);
    ++h->n_allocs;                          // (one block: 8.4 MB of basis, 2.1 MB of cepstral basis and the warp table at nfft = 1024)
    w.loaded = true;
    cur = w;
    return 0;
}

int ev_envelope(ev_handle* h, const float* d_x, const int32_t* d_len, const float* d_period, int B, int L, double power_floor,
                double* d_env, double* d_mcep, int32_t* d_class, void* stream) {
    if (enter(h)) return 1;
    const EnvW& w = h->env;
    if (!w.loaded) return fail(h, "ev_envelope: tables not loaded (ev_load_envelope)");
    if (check_batch(h, __func__, B)) return 1;
    if (L < 1) return fail(h, "ev_envelope: L=%d must be at least 1", L);
    if (!d_x) return fail(h, "ev_envelope: d_x must be non-null");
    if (!d_period) return fail(h, "ev_envelope: d_period must be non-null (ev_pitch_yin's periods; 0 where unvoiced)");
    if (!(power_floor > 0.0) || !std::isfinite(power_floor)) return fail(h, "ev_envelope: power_floor=%g must be finite and greater than 0", power_floor);
    if (!d_mcep || !d_class) return fail(h, "ev_envelope: d_mcep and d_class must be non-null");
    if (L / w.t.H > 0x7fffffef) return fail(h, "ev_envelope: L=%d at H=%d has more frames than an int32 tile index holds", L, w.t.H);
    h->stream = (hipStream_t)stream;
    const int NF = frames_of(L, w.t.H);
    if (scratch_acquire(h, h->env_ws, (size_t)B * NF * w.t.NB * sizeof(double))) return 1;
    double* P = (double*)h->env_ws.p;
    const dim3 grid((unsigned)((NF + 15) / 16), (unsigned)B);
    EnvPowerParams pp{d_x, d_len, d_period, P, w.t, L, NF};
    launch<envelope_power_kernel>(h->device, grid, dim3(256), w.lds1, h->stream, pp);
    EnvCepParams pc{d_len, d_period, P, d_env, d_mcep, d_class, w.t, L, NF, power_floor};
    launch<envelope_cepstrum_kernel>(h->device, grid, dim3(256), w.lds2, h->stream, pc);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// Phase vocoder: time stretching by stft -> phase propagation -> istft (pv_analysis_kernel, pv_propagate_kernel and pv_synthesis_kernel,
// ev_analysis_kernels.h; the definition: include/emojivoice.h).  W = nfft, H = nfft / 4.  A load owns one device block: the windowed DFT basis
// (stft_dist_basis_kernel), the inverse basis (pv_inv_basis_kernel), w / nfft and w^2 (formed here, one rounding each).  Arena of a call: mag and
// ang, 2 x B x NF x NB doubles, and without d_stretch Y, B x NO x NB pairs.
int ev_load_phase_vocoder(ev_handle* h, const double* window, const double* twiddle, int nfft) {
    if (enter(h)) return 1;
    if (!window || !twiddle) return fail(h, "ev_load_phase_vocoder: window and twiddle must be non-null (HOST)");
    if (nfft < 16 || nfft > 2048 || nfft % 16) return fail(h, "ev_load_phase_vocoder: nfft=%d must be a multiple of 16 with 16 <= nfft <= 2048", nfft);
    if (check_finite(h, __func__, "window", window, nfft) || check_finite(h, __func__, "twiddle", twiddle, 2 * nfft)) return 1;
    PvW w;
    PvTables& t = w.t;
    t.nfft = nfft; t.H = nfft / 4; t.NB = nfft / 2 + 1; t.NBp = (t.NB + 3) / 4 * 4; t.skew = dft_skew(t.H);
    w.lds = (size_t)dft_span_words(15 * t.H + nfft, t.H, t.skew) * sizeof(float);
    std::vector<double> tab((size_t)2 * nfft);
    for (int j = 0; j < nfft; ++j) { tab[j] = window[j] / (double)nfft; tab[(size_t)nfft + j] = window[j] * window[j]; }
    const size_t n_basis = (size_t)nfft * t.NB, n_inv = (size_t)t.NBp * nfft;
    const size_t o_inv = 2 * n_basis, o_wn = o_inv + 2 * n_inv;       // in doubles from the block's start
    char* blk = nullptr;                                                // the new block first: a failed load leaves the tables in use as they are
    auto rest = [&](char* b, const double* d_tw) {
        double* d = (double*)b;
        hipError_t e = hipMemcpy(d + o_wn, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice);
        PvInvParams pi{d_tw, (double2*)(d + o_inv), nfft, t.H, t.NB, t.NBp};
        if (e == hipSuccess) launch<pv_inv_basis_kernel>(h->device, dim3((unsigned)((n_inv + 255) / 256)), dim3(256), 0, (hipStream_t)nullptr, pi);
        return e;
    };
    if (build_dft_basis(h, __func__, "tables", window, twiddle, nfft, nfft, (o_wn + tab.size()) * sizeof(double), &blk, rest)) return 1;
    const double* d = (const double*)blk;
    t.basis = (const double2*)blk; t.inv = (const double2*)(d + o_inv); t.wn = d + o_wn; t.wsq = d + o_wn + nfft;
    PvW& cur = h->pv;
    if (cur.loaded && drop_owned(h, {(void*)cur.t.basis})) { hipFree(blk); return 1; }
    h->owned.push_back(blk);
    ++h->n_allocs;                          // (one block: 8.4 MB of basis and 8.5 MB of inverse basis at nfft = 1024)
    w.loaded = true;
    cur = w;
    return 0;
}

int ev_phase_vocoder(ev_handle* h, const float* d_x, const int32_t* d_len, int B, int L, double rate, float* d_y, int L_out, int32_t* d_out_len,
                     int32_t* d_counts, double* d_stretch, void* stream) {
    if (enter(h)) return 1;
    const PvW& w = h->pv;
    if (!w.loaded) return fail(h, "ev_phase_vocoder: tables not loaded (ev_load_phase_vocoder)");
    if (check_batch(h, __func__, B)) return 1;
    if (L < 1) return fail(h, "ev_phase_vocoder: L=%d must be at least 1", L);
    if (!std::isfinite(rate) || rate < 0.125 || rate > 8.0) return fail(h, "ev_phase_vocoder: rate=%g must be finite with 0.125 <= rate <= 8", rate);
    const long long want = (long long)std::rint((double)L / rate);
    if (L_out != want) return fail(h, "ev_phase_vocoder: L_out=%d must be rint(L / rate) = %lld", L_out, want);
    if (!d_x) return fail(h, "ev_phase_vocoder: d_x must be non-null");
    if (!d_y || !d_out_len) return fail(h, "ev_phase_vocoder: d_y and d_out_len must be non-null");
    const PvTables& t = w.t;
    const int NF = 1 + L / t.H, NO = pv_steps(NF, rate);
    const size_t n_ma = (size_t)B * NF * t.NB, n_y = d_stretch ? 0 : (size_t)B * NO * t.NB * 2;
    const size_t bytes = (2 * n_ma + n_y) * sizeof(double);
    if (bytes > ((size_t)4 << 30))
        return fail(h, "ev_phase_vocoder: B=%d rows of L=%d at rate=%g need %zu bytes of scratch, over 4 GiB: split the batch", B, L, rate, bytes);
    h->stream = (hipStream_t)stream;
    if (scratch_acquire(h, h->pv_ws, bytes)) return 1;
    double* mag = (double*)h->pv_ws.p;
    double* ang = mag + n_ma;
    double2* Y = d_stretch ? (double2*)d_stretch : (double2*)(ang + n_ma);
    PvAnalysisParams pa{d_x, d_len, mag, ang, t, L, NF};
    launch<pv_analysis_kernel>(h->device, dim3((unsigned)((NF + 15) / 16), (unsigned)B), dim3(256), w.lds, h->stream, pa);
    PvPropParams pp{mag, ang, d_len, Y, d_out_len, d_counts, t, L, NF, NO, rate};
    launch<pv_propagate_kernel>(h->device, dim3((unsigned)((t.NB + 63) / 64), (unsigned)B), dim3(64), 0, h->stream, pp);
    PvSynthParams ps{Y, d_len, d_y, t, L, NO, L_out, rate};
    launch<pv_synthesis_kernel>(h->device, dim3((unsigned)((NO + 3 + 12) / 13), (unsigned)B), dim3(256), 0, h->stream, ps);
    HIPCHK(h, hipGetLastError());
    return 0;
}

}  // extern "C"
