// Analysis kernels: dataset statistics, resampling, silence trimming, YIN / pYIN pitch tracking, DTW, BS.1770 loudness, STOI / ESTOI, the
// STFT distance and voice quality.  None of them shares code with the synthesis engine: ev_kernels.h includes this file at its end, after every helper the
// kernels below use (the f32x4 vector type and cfm_valid_len, nothing else).  Their host entry points are in ev_analysis.h.
#pragma once

// Dataset statistics of ev_mel_stats: sum x and sum x^2 in float64 over the row's len[b] x C valid cells of a (B, C, T) mel.  One workgroup
// per (row, 32 frames), lane = frame (32 consecutive floats of one channel row per half-wave), the eight half-waves walk the channels; the
// same fixed shuffle tree and wave order as cfm_loss_kernel, the same per-row merge (cfm_loss_merge_kernel): no atomics.
__global__ __launch_bounds__(256) void mel_stats_kernel(const float* __restrict__ mel, const int32_t* __restrict__ len, int C, int T,
                                                         double* part, int ntiles) {
    __shared__ double red[4][2];
    const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    const int t = tile * 32 + (tid & 31);
    const int valid = cfm_valid_len(len[b], T);
    double s1 = 0.0, s2 = 0.0;
    if (t < valid) {
        for (int c = tid >> 5; c < C; c += 8) {
            const double v = (double)mel[((size_t)b * C + c) * T + t];
            s1 += v;
            s2 += v * v;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_down(s1, o); s2 += __shfl_down(s2, o); }
    if ((tid & 63) == 0) { red[tid >> 6][0] = s1; red[tid >> 6][1] = s2; }
    __syncthreads();
    if (tid == 0) {
        double* o = part + ((size_t)b * ntiles + tile) * 2;
        o[0] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
        o[1] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    }
}

// ---------------------------------------------------------------------------
// Rational polyphase FIR resampler (ev_resample):  y[n] = sum_i x[i] taps[n down - i up + c],  c = (n_taps - 1) / 2,  x zero outside [0, len).
// With q = n down + c, phase ph = q mod up and i0 = q / up the sum is  sum_{j = 0}^{W - 1} table[ph][j] x[i0 - j],  W = ceil(n_taps / up),
// table[ph][j] = taps[ph + j up] (zero beyond n_taps; row stride Wp = W | 1, so the rows of different phases start on different LDS banks).
// ARITHMETIC: one fp32 fmaf chain per output, acc = fmaf(table[ph][j], x[i0 - j], acc) for j = 0, 1, ... W - 1 from acc = +0, all W terms
// always (a sample outside the row enters as +0 and leaves acc as it is).  The chain depends on (n, taps, the row's samples) only: not on the
// tile, the batch or the padding behind the row.
// One workgroup owns TILE consecutive outputs of one row (thread t: outputs t, t + 256, ...: coalesced stores).  64-bit arithmetic fixes the
// tile's origin (q0 = n0 down + c, base_i = q0 / up, r0 = q0 mod up: n down and i up pass 2^31 for minutes of audio); inside the tile
// everything is a 32-bit offset from it (r0 + t down <= 639 + 1023 * 640).  SX: the input span the tile reads, x[base_i - (W - 1) ..
// base_i + (r0 + (TILE - 1) down) / up], is staged into LDS by coalesced loads (zeros outside the row); ST: so is the whole phase table
// (16-byte copies).  Without SX / ST the kernel reads x / the table from global memory (the fallbacks of filters too long for the budget).
// dynamic LDS: [ST: tab_floats] [SX: span] floats.
struct ResampleParams {
    const float* x; const int32_t* len; float* y; const float* table;
    int L_in, L_out, up, down, c, W, Wp, span, tab_floats;
};

template <int TILE, bool SX, bool ST>
__global__ __launch_bounds__(256) void resample_kernel(const ResampleParams p) {
    extern __shared__ __attribute__((aligned(16))) float rs_sm[];
    constexpr int PER = TILE / 256;
    const int tid = threadIdx.x, b = blockIdx.y;
    const long long n0 = (long long)blockIdx.x * TILE;
    int len = p.len ? p.len[b] : p.L_in;
    if (len < 1 || len > p.L_in) len = 0;                                   // a bad row is a row of zeros (the ev_mas_align convention)
    const long long lout = ((long long)len * p.up + p.down - 1) / p.down;   // outputs the row has: beyond them zeros
    float* yrow = p.y + (size_t)b * p.L_out;
    if (n0 >= lout) {                                                       // (uniform over the workgroup)
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const long long n = n0 + tid + 256 * k;
            if (n < p.L_out) yrow[n] = 0.f;
        }
        return;
    }
    const long long q0 = n0 * p.down + p.c;
    const long long base_i = q0 / p.up;
    const int r0 = (int)(q0 - base_i * p.up);
    const long long span_base = base_i - (p.W - 1);
    const float* xrow = p.x + (size_t)b * p.L_in;
    float* xs = rs_sm + (ST ? p.tab_floats : 0);
    if (ST) {
        for (int i = tid; i < p.tab_floats / 4; i += 256) ((f32x4*)rs_sm)[i] = ((const f32x4*)p.table)[i];
    }
    if (SX) {
        for (int s = tid; s < p.span; s += 256) {
            const long long gi = span_base + s;
            xs[s] = (gi >= 0 && gi < len) ? xrow[gi] : 0.f;
        }
    }
    if (SX || ST) __syncthreads();
    const float* trow[PER];
    int so[PER];
    float acc[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int v = r0 + (tid + 256 * k) * p.down;
        const int di = v / p.up, ph = v - di * p.up;
        trow[k] = (ST ? (const float*)rs_sm : p.table) + ph * p.Wp;
        so[k] = di + p.W - 1;                                               // x[i0] sits at xs[so]; tap j reads xs[so - j]
        acc[k] = 0.f;
    }
    for (int j = 0; j < p.W; ++j) {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            float xv;
            if (SX) xv = xs[so[k] - j];
            else {
                const long long gi = span_base + so[k] - j;
                xv = (gi >= 0 && gi < len) ? xrow[gi] : 0.f;
            }
            acc[k] = fmaf(trow[k][j], xv, acc[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const long long n = n0 + tid + 256 * k;
        if (n < p.L_out) yrow[n] = n < lout ? acc[k] : 0.f;
    }
}

// ---------------------------------------------------------------------------
// Silence trimming and levelling (ev_trim_bounds, ev_trim_apply): librosa.effects.trim's frames and the vocoder dataset's peak gain.
// Frame f of a row covers samples [f H - F/2, f H + F/2), zeros outside [0, len); it is non-silent iff
// max(ms[f], 1e-10) > max(max_f ms, 1e-10) * 10^(-top_db / 10), ms[f] = (sum x^2) / F.  F = R H, so a frame is R consecutive HOP BLOCKS of
// a grid whose origin is -off, off = (F/2) mod H (0 for even R, H/2 for odd R): block j covers samples [j H - off, (j + 1) H - off) and
// frame f is blocks f - R/2 ... f - R/2 + R - 1.
// ARITHMETIC of a block: each fp32 sample widened to float64 and squared (exact), summed per lane in ascending sample index -- sample c of
// the block belongs to lane (c / 4) mod 64 -- then one fixed shuffle tree over the wave.  One wave owns a whole block, so its sum depends
// on the block's samples only: not on the tile, the batch, the padding behind the row or the row's alignment (an unaligned row takes
// 4-byte loads in the same lane assignment).  No atomics.
struct TrimBlocksParams {
    const float* x; const int32_t* len; double* bsum; float* bmax;     // bsum, bmax: (B, nblk)
    int L, H, off, nblk;
};

constexpr int TRIM_TILE = 8;                                            // hop blocks per workgroup: two per wave

__global__ __launch_bounds__(256) void trim_blocks_kernel(const TrimBlocksParams p) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int len = p.len ? p.len[b] : p.L;
    if (len < 1 || len > p.L) len = 0;                                  // a bad row is a row of zeros (the ev_mas_align convention)
    const float* xrow = p.x + (size_t)b * p.L;
    const bool vec = (((size_t)xrow) & 15) == 0;                        // (H and off are multiples of 32 samples: every block keeps the row's alignment)
    for (int k = wave; k < TRIM_TILE; k += 4) {                         // (uniform over the wave)
        const long long j = (long long)blockIdx.x * TRIM_TILE + k;
        if (j >= p.nblk) break;
        const long long s0 = j * p.H - p.off;                           // the block's first sample: -off for j = 0
        double acc = 0.0;
        float pk = 0.f;
        for (int c = 4 * lane; c < p.H; c += 256) {
            const long long i = s0 + c;                                 // (a multiple of 4: i < 0 means the whole quad is left of the row)
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (i >= 0 && i + 4 <= len) {
                if (vec) {
                    const f32x4 q = *(const f32x4*)(xrow + i);
                    v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = xrow[i + e];
                }
            } else if (i >= 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (i + e < len) v[e] = xrow[i + e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double d = (double)v[e];
                acc += d * d;
                pk = fmaxf(pk, fabsf(v[e]));
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { acc += __shfl_down(acc, o); pk = fmaxf(pk, __shfl_down(pk, o)); }
        if (lane == 0) { p.bsum[(size_t)b * p.nblk + j] = acc; p.bmax[(size_t)b * p.nblk + j] = pk; }
    }
}

// One workgroup per row over the block sums: frame sums (R blocks in ascending order, blocks outside the row +0), ref = max_f ms, the
// predicate, the first and last non-silent frame, start = f_first H, end = min(len, (f_last + 1) H) and the row's peak (max of the block
// maxima).  Every reduction is a max or a min: the thread count does not enter the result.  A bad row, or one without a non-silent frame
// (top_db <= 0), gets bounds (0, 0).
struct TrimBoundsParams {
    const double* bsum; const float* bmax; const int32_t* len; int32_t* bounds; float* peak;
    int L, H, R, off, nblk;
    double F, thr;                                                      // thr = 10^(-top_db / 10)
};

__device__ __forceinline__ double trim_frame_ms(const double* bs, int f, int R, int nb, double F) {
    const int j0 = f - R / 2;
    double s = 0.0;
    for (int r = 0; r < R; ++r) {
        const int j = j0 + r;
        s += (j >= 0 && j < nb) ? bs[j] : 0.0;
    }
    return s / F;
}

__global__ __launch_bounds__(256) void trim_bounds_kernel(const TrimBoundsParams p) {
    __shared__ double red_d[4];
    __shared__ float red_f[4];
    __shared__ int red_i[4][2];
    const int b = blockIdx.x, tid = threadIdx.x;
    int len = p.len ? p.len[b] : p.L;
    if (len < 1 || len > p.L) len = 0;
    const int nf = len ? 1 + len / p.H : 0;
    const int nb = len ? (int)(((long long)len + p.off + p.H - 1) / p.H) : 0;   // blocks that hold a sample of the row (<= nblk)
    const double* bs = p.bsum + (size_t)b * p.nblk;
    const float* bm = p.bmax + (size_t)b * p.nblk;
    double ref = 0.0;
    float pk = 0.f;
    for (int f = tid; f < nf; f += 256) ref = fmax(ref, trim_frame_ms(bs, f, p.R, nb, p.F));
    for (int j = tid; j < nb; j += 256) pk = fmaxf(pk, bm[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { ref = fmax(ref, __shfl_down(ref, o)); pk = fmaxf(pk, __shfl_down(pk, o)); }
    if ((tid & 63) == 0) { red_d[tid >> 6] = ref; red_f[tid >> 6] = pk; }
    __syncthreads();
    ref = fmax(fmax(red_d[0], red_d[1]), fmax(red_d[2], red_d[3]));
    pk = fmaxf(fmaxf(red_f[0], red_f[1]), fmaxf(red_f[2], red_f[3]));
    const double cut = fmax(ref, 1e-10) * p.thr;
    int first = 0x7fffffff, last = -1;
    for (int f = tid; f < nf; f += 256) {
        if (fmax(trim_frame_ms(bs, f, p.R, nb, p.F), 1e-10) > cut) { first = min(first, f); last = max(last, f); }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { first = min(first, __shfl_down(first, o)); last = max(last, __shfl_down(last, o)); }
    if ((tid & 63) == 0) { red_i[tid >> 6][0] = first; red_i[tid >> 6][1] = last; }
    __syncthreads();
    if (tid == 0) {
        first = min(min(red_i[0][0], red_i[1][0]), min(red_i[2][0], red_i[3][0]));
        last = max(max(red_i[0][1], red_i[1][1]), max(red_i[2][1], red_i[3][1]));
        int start = 0, end = 0;
        if (last >= 0) {
            start = (int)((long long)first * p.H);
            end = (int)min((long long)len, ((long long)last + 1) * p.H);
        }
        p.bounds[2 * b] = start;
        p.bounds[2 * b + 1] = end;
        if (p.peak) p.peak[b] = pk;
    }
}

// y[b, j] = x[b, start[b] + j] * gain[b] for j < min(end[b] - start[b], L_out), +0 up to L_out; out_len[b] = that count.  Bounds and peak
// come from device memory; gain = target / peak[b] (one correctly rounded fp32 division) when a peak is given, target > 0 and peak > 0,
// else 1 (x * 1 is x: a bit-exact copy).  Bounds outside 0 <= start <= end <= L make a row of zeros.  One workgroup per (row, 1024
// outputs); 16-byte stores where the output row is aligned (the source starts at an arbitrary sample: 4-byte loads).
struct TrimApplyParams {
    const float* x; const int32_t* bounds; const float* peak; float* y; int32_t* out_len;
    float target;
    int L, L_out;
};

__global__ __launch_bounds__(256) void gather_scale_kernel(const TrimApplyParams p) {
    const int b = blockIdx.y, tid = threadIdx.x;
    int start = p.bounds[2 * b];
    const int end = p.bounds[2 * b + 1];
    int n = 0;
    if (start >= 0 && end >= start && end <= p.L) n = min(end - start, p.L_out);
    else start = 0;
    float g = 1.f;
    if (p.peak && p.target > 0.f) {
        const float pk = p.peak[b];
        if (pk > 0.f) g = __fdiv_rn(p.target, pk);
    }
    if (blockIdx.x == 0 && tid == 0) p.out_len[b] = n;
    const float* xs = p.x + (size_t)b * p.L + start;
    float* yrow = p.y + (size_t)b * p.L_out;
    const long long j0 = (long long)blockIdx.x * 1024;
    if ((((size_t)yrow) & 15) == 0) {
        const long long j = j0 + 4 * tid;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (j + e < n) ? xs[j + e] * g : 0.f;
        if (j + 4 <= p.L_out) { const f32x4 q = {v[0], v[1], v[2], v[3]}; *(f32x4*)(yrow + j) = q; }
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (j + e < p.L_out) yrow[j + e] = v[e];
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long j = j0 + tid + 256 * k;
            if (j < p.L_out) yrow[j] = (j < n) ? xs[j] * g : 0.f;
        }
    }
}

// ---------------------------------------------------------------------------
// Pitch tracking (ev_pitch_yin): de Cheveigne and Kawahara's YIN without its last ("best local estimate") step.  Frame f of a row
// analyses the span x[s_f + i], 0 <= i < W + tau_max + 1, s_f = f H + H/2 - (W + tau_max) / 2, zeros outside [0, len):
//   d(tau)  = sum_{j < W} (x[j] - x[j + tau])^2                       1 <= tau <= n = tau_max + 1
//   d'(tau) = d(tau) * tau / S(tau), S(tau) = sum_{k <= tau} d(k)     (1 where S(tau) is not > 0)
//   tau0    = the smallest tau in [tau_min, tau_max] with d'(tau) < threshold, then walked down to the local minimum on its right;
//   period  = tau0 + the parabola's vertex through d'(tau0 - 1), d'(tau0), d'(tau0 + 1)
// One workgroup of four waves per (frame, row).  The span is staged in LDS once, as fp32.  TILE: lane l of every wave owns the lags
// 1 + l + 64 c of lag chunk c, four chunks at a time (one broadcast read of x[j] serves four lags; x[j + tau] over consecutive lags is
// conflict-free); wave q covers the quarter q W/4 <= j < (q + 1) W/4 of the window for EVERY lag, so the four SIMDs carry equal work
// whatever tau_max is.
// ARITHMETIC of d(tau): both samples widened to float64, the difference (exact) squared and added by one fma per term, in ascending j
// inside a quarter; d = (P0 + P1) + (P2 + P3) over the quarters' partials.  S is one ascending chain of float64 adds (one lane), d' =
// (d * tau) / S in float64, and the decision runs in wave 0.  Nothing depends on the batch, the grid, the padding behind a row or
// ev_set_arithmetic; no atomics.
// LDS: 4 n float64 (the partials; later d, S and d' in place) and W + n fp32: at most 64 KiB + 24 KiB at tau_max = 2048,
// 16.0 KiB at the defaults (W 1024, tau_max 340).
struct PitchYinParams {
    const float* x; const int32_t* len; int32_t* lag; float* period; float* cmnd;
    int L, F, W, H, tau_min, tau_max;
    double thr;
};

// The partial sums of wave `lane`'s lags in chunks c0 .. c0 + NK - 1 over j0 <= j < j1
template <int NK>
__device__ __forceinline__ void pitch_yin_pass(const float* xs, double* part, int c0, int n, int j0, int j1, int lane) {
    int t[NK];
    double a[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) { t[k] = min(1 + lane + 64 * (c0 + k), n); a[k] = 0.0; }   // (a lane past the last lag repeats it and stores nothing)
    for (int j = j0; j < j1; ++j) {
        const double xj = (double)xs[j];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const double d = xj - (double)xs[j + t[k]];
            a[k] = fma(d, d, a[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int tau = 1 + lane + 64 * (c0 + k);
        if (tau <= n) part[tau - 1] = a[k];
    }
}

// Frame f of a row of len valid samples: stages its span and leaves d'(tau), 1 <= tau <= n = tau_max + 1, at index tau - 1 of the returned
// LDS array (n float64; the n before it hold S, the n before those d).  Every thread of the 256 calls it; it ends on a barrier.  smem:
// 4 n float64 + W + n fp32.  Shared by pitch_yin_kernel and pyin_observe_kernel: one framing, one d, one S chain, one d'.
__device__ __forceinline__ const double* pitch_cmnd_frame(float* smem, const float* xrow, int len, int f, int W, int H, int tau_max, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    const int n = tau_max + 1, span = W + n;
    double* part = (double*)smem;                                       // [4][n]: a quarter's partials; then row 0 = d, row 1 = S, row 2 = d'
    float* xs = (float*)(part + 4 * (size_t)n);                         // [span]
    const long long s0 = (long long)f * H + H / 2 - (W + tau_max) / 2;
    for (int i = tid; i < span; i += 256) {
        const long long g = s0 + i;
        xs[i] = (g >= 0 && g < len) ? xrow[g] : 0.f;
    }
    __syncthreads();
    const int nch = (n + 63) >> 6, jq = W >> 2;
    double* mine = part + (size_t)wave * n;
    for (int c0 = 0; c0 < nch; c0 += 4) {                               // (uniform over the wave)
        const int nk = min(4, nch - c0), j0 = wave * jq, j1 = j0 + jq;
        if (nk == 4) pitch_yin_pass<4>(xs, mine, c0, n, j0, j1, lane);
        else if (nk == 3) pitch_yin_pass<3>(xs, mine, c0, n, j0, j1, lane);
        else if (nk == 2) pitch_yin_pass<2>(xs, mine, c0, n, j0, j1, lane);
        else pitch_yin_pass<1>(xs, mine, c0, n, j0, j1, lane);
    }
    __syncthreads();
    double* dd = part;
    double* S = part + n;
    double* cm = part + 2 * (size_t)n;
    for (int i = tid; i < n; i += 256) dd[i] = (part[i] + part[n + i]) + (part[2 * (size_t)n + i] + part[3 * (size_t)n + i]);
    __syncthreads();
    if (tid == 0) {                                                     // S(tau): ONE ascending chain
        double s = 0.0;
        for (int i = 0; i < n; ++i) { s += dd[i]; S[i] = s; }
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256) {                                // (index i holds lag tau = i + 1)
        const double s = S[i];
        cm[i] = s > 0.0 ? dd[i] * (double)(i + 1) / s : 1.0;
    }
    __syncthreads();
    return cm;
}

__global__ __launch_bounds__(256) void pitch_yin_kernel(const PitchYinParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t o = (size_t)b * p.F + f;
    int len = p.len ? p.len[b] : p.L;
    if (len < 1 || len > p.L) len = 0;                                  // a bad row is a row of zeros (the ev_mas_align convention)
    const int nf = (int)(((long long)len + p.H - 1) / p.H);
    if (f >= nf) {                                                      // (uniform over the workgroup)
        if (tid == 0) {
            if (p.lag) p.lag[o] = 0;
            if (p.period) p.period[o] = 0.f;
            if (p.cmnd) p.cmnd[o] = 0.f;
        }
        return;
    }
    const double* cm = pitch_cmnd_frame(smem, p.x + (size_t)b * p.L, len, f, p.W, p.H, p.tau_max, tid);
    if (wave != 0) return;
    int first = 0x7fffffff;
    double mn = 1.0 / 0.0;
    for (int tau = p.tau_min + lane; tau <= p.tau_max; tau += 64) {
        const double v = cm[tau - 1];
        if (v < p.thr) first = min(first, tau);
        mn = fmin(mn, v);
    }
#pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1) { first = min(first, __shfl_down(first, sft)); mn = fmin(mn, __shfl_down(mn, sft)); }
    if (lane != 0) return;
    int tau0 = 0;
    float per = 0.f;
    double ap = mn;                                                     // unvoiced: the smallest d' of the search range
    if (first != 0x7fffffff) {
        tau0 = first;
        while (tau0 + 1 <= p.tau_max && cm[tau0] < cm[tau0 - 1]) ++tau0;
        const double a = cm[tau0 - 2], bq = cm[tau0 - 1], c = cm[tau0];  // tau0 >= 2: d'(1) is 1 and threshold <= 1; tau0 + 1 <= n
        const double den = a - 2.0 * bq + c;
        double shift = 0.0;
        if (den > 0.0) {
            shift = 0.5 * (a - c) / den;
            if (!(fabs(shift) <= 1.0)) shift = 0.0;
        }
        per = (float)((double)tau0 + shift);
        ap = bq;
    }
    if (p.lag) p.lag[o] = tau0;
    if (p.period) p.period[o] = per;
    if (p.cmnd) p.cmnd[o] = (float)ap;
}

// ---------------------------------------------------------------------------
// Probabilistic YIN, the observation (ev_pyin_observe): Mauch and Dixon's pYIN over the d' of pitch_cmnd_frame, d'(0) := 1.  Per frame:
//   troughs   tau in [tau_min, tau_max] with d'(tau) < d'(tau - 1) and d'(tau) <= d'(tau + 1), ascending (no two are adjacent: K <= kmax =
//             (tau_max - tau_min) / 2 + 1); trough k has ONE activation index a_k = the least t with d'(tau_k) < t / n_thr (n_thr + 1: none)
//   P_k       sum over t >= a_k, ascending, of G_t E[pos(k, t)]: E[p] = exp(-lambda p), pos(k, t) = #{m < k : a_m <= t}, N(t) = #{m : a_m <= t},
//             G_t = w_t (1 - e^-lambda) / (1 - E[N(t)]); the trough g of least d' (lowest lag on ties) gains no_trough_prob * cw[a_g - 1],
//             cw the host's ascending prefix sums of w
//   bin_k     clip(rint(bpo log2(sr / (period_k fmin))), 0, n_bins - 1), period_k = tau_k + pitch_yin_kernel's parabolic shift
//   obs[bin_k] += P_k (P_k > 0) in ascending k; pv = min(sum_i obs[i], 1) in ascending i
// One workgroup of four waves per (frame, row), as pitch_yin_kernel.  Trough k = tid + 256 r is thread tid's: wave q holds the 64-trough
// blocks q, q + 4, ...  pos comes from ballots: a first sweep over t counts each block's active troughs (cnt[block][t], one lane stores),
// n_thr threads turn the counts into exclusive prefixes over the blocks, N(t) and G_t, and a second sweep adds G_t E[prefix + the active
// lanes below mine].  period_k does not decrease with k (the lags differ by >= 2, the shifts by <= 2), so equal bins are RUNS of k: the first
// trough of a run sums it in ascending k and stores the bin: no atomics, no read-modify-write between threads.  One lane sums pv.
// LDS beyond pitch_cmnd_frame's: (2 kmax + n_thr + n_bins + 6) float64 + (3 kmax + ceil(kmax / 64) (n_thr + 1) + 8) int32: 9.2 KiB at the
// defaults (kmax 153, n_thr 100, 385 bins), 46 KiB at the limits.  Nothing depends on the batch, the grid or the padding behind a row.
struct PyinObserveParams {
    const float* x; const int32_t* len; double* obs; double* pv;
    int L, F, W, H, tau_min, tau_max, n_bins, n_thr, kmax, off_extra;
    double sr, fmin, bpo, lambda, c0, ntp;
    double w[128];                      // w_t at t - 1
    double cw[129];                     // cw[t] = w_1 + ... + w_t, one ascending chain; cw[0] = 0
};

__global__ __launch_bounds__(256) void pyin_observe_kernel(const PyinObserveParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t o = (size_t)b * p.F + f;
    double* orow = p.obs + o * (size_t)p.n_bins;
    int len = p.len ? p.len[b] : p.L;
    if (len < 1 || len > p.L) len = 0;                                  // a bad row is a row of zeros
    const int nf = (int)(((long long)len + p.H - 1) / p.H);
    if (f >= nf) {                                                      // (uniform over the workgroup)
        for (int i = tid; i < p.n_bins; i += 256) orow[i] = 0.0;
        if (tid == 0) p.pv[o] = 0.0;
        return;
    }
    const double* cm = pitch_cmnd_frame(smem, p.x + (size_t)b * p.L, len, f, p.W, p.H, p.tau_max, tid);
    const int kmax = p.kmax, n_thr = p.n_thr, n_bins = p.n_bins, ldc = n_thr + 1;
    double* E = (double*)((unsigned char*)smem + p.off_extra);          // [kmax + 1]
    double* P = E + kmax + 1;                                           // [kmax]
    double* G = P + kmax;                                               // [n_thr + 1]
    double* ob = G + ldc;                                               // [n_bins]
    double* rv = ob + n_bins;                                           // [4]
    int* tl = (int*)(rv + 4);                                           // [kmax] trough lags
    int* act = tl + kmax;                                               // [kmax] activation indices
    int* bn = act + kmax;                                               // [kmax] bins
    int* wt = bn + kmax;                                                // [4] troughs found per wave
    int* ri = wt + 4;                                                   // [4]
    int* cnt = ri + 4;                                                  // [ceil(kmax / 64)][n_thr + 1]
    // 1. the troughs, in ascending lag: thread tid looks at a contiguous piece of the range, a scan of the counts places them
    const int m = p.tau_max - p.tau_min + 1, seg = (m + 255) >> 8;
    const int ta = p.tau_min + tid * seg, tb = min(ta + seg, p.tau_max + 1);
    int found = 0;
    for (int tau = ta; tau < tb; ++tau) {
        const double v = cm[tau - 1], l = tau > 1 ? cm[tau - 2] : 1.0;
        found += (v < l && v <= cm[tau]) ? 1 : 0;
    }
    int inc = found;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) { const int u = __shfl_up(inc, s); if (lane >= s) inc += u; }
    if (lane == 63) wt[wave] = inc;
    for (int i = tid; i < n_bins; i += 256) ob[i] = 0.0;
    __syncthreads();
    int k0 = inc - found;
    for (int q = 0; q < wave; ++q) k0 += wt[q];
    const int K = min(wt[0] + wt[1] + wt[2] + wt[3], kmax);
    for (int tau = ta; tau < tb; ++tau) {
        const double v = cm[tau - 1], l = tau > 1 ? cm[tau - 2] : 1.0;
        if (v < l && v <= cm[tau]) { if (k0 < kmax) tl[k0] = tau; ++k0; }
    }
    for (int i = tid; i <= K; i += 256) E[i] = exp(-p.lambda * (double)i);
    if (K == 0) {                                                       // (uniform) a silent frame, or one without a trough
        for (int i = tid; i < n_bins; i += 256) orow[i] = 0.0;
        if (tid == 0) p.pv[o] = 0.0;
        return;
    }
    __syncthreads();
    // 2. per trough: activation index, period, bin; the trough of least d'
    const double nd = (double)n_thr;
    double bv = 1.0 / 0.0;
    int bk = 0x7fffffff;
    for (int k = tid; k < K; k += 256) {
        const int tau = tl[k];
        const double a = tau > 1 ? cm[tau - 2] : 1.0, bq = cm[tau - 1], c = cm[tau];
        int at = n_thr + 1;
        if (bq < 1.0) {
            at = min(max((int)(bq * nd) + 1, 1), n_thr);
            while (at > 1 && bq < (double)(at - 1) / nd) --at;
            while (at <= n_thr && !(bq < (double)at / nd)) ++at;
        }
        act[k] = at;
        const double den = a - 2.0 * bq + c;
        double shift = 0.0;
        if (den > 0.0) {
            shift = 0.5 * (a - c) / den;
            if (!(fabs(shift) <= 1.0)) shift = 0.0;
        }
        const double q = rint(p.bpo * log2(p.sr / (((double)tau + shift) * p.fmin)));
        bn[k] = (int)fmin(fmax(q, 0.0), (double)(n_bins - 1));
        if (bq < bv) { bv = bq; bk = k; }                               // (ascending k: the lowest lag of the least)
    }
#pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1) {
        const double ov = __shfl_down(bv, sft);
        const int ok = __shfl_down(bk, sft);
        if (ov < bv || (ov == bv && ok < bk)) { bv = ov; bk = ok; }
    }
    if (lane == 0) { rv[wave] = bv; ri[wave] = bk; }
    // 3. first sweep: the active troughs of each block at each threshold
    const int nblk = (K + 63) >> 6;
    for (int kb = wave; kb < nblk; kb += 4) {                           // (uniform over the wave; trough 64 kb + lane is this thread's own)
        const int k = 64 * kb + lane, at = k < K ? act[k] : n_thr + 1;
        for (int t = 1; t <= n_thr; ++t) {
            const unsigned long long bal = __ballot(at <= t);
            if (lane == 0) cnt[kb * ldc + t] = __popcll(bal);
        }
    }
    __syncthreads();
    int g = ri[0];
    {
        double gv = rv[0];
#pragma unroll
        for (int q = 1; q < 4; ++q) if (rv[q] < gv || (rv[q] == gv && ri[q] < g)) { gv = rv[q]; g = ri[q]; }
    }
    for (int t = 1 + tid; t <= n_thr; t += 256) {
        int run = 0;
        for (int kb = 0; kb < nblk; ++kb) { const int c = cnt[kb * ldc + t]; cnt[kb * ldc + t] = run; run += c; }
        G[t] = run > 0 ? p.w[t - 1] * p.c0 / (1.0 - E[run]) : 0.0;
    }
    __syncthreads();
    // 4. second sweep: P_k
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int kb = wave; kb < nblk; kb += 4) {
        const int k = 64 * kb + lane, at = k < K ? act[k] : n_thr + 1;
        double acc = 0.0;
        for (int t = 1; t <= n_thr; ++t) {
            const unsigned long long bal = __ballot(at <= t);
            if (at <= t) acc += G[t] * E[cnt[kb * ldc + t] + __popcll(bal & below)];
        }
        if (k == g) acc += p.ntp * p.cw[at - 1];
        if (k < K) P[k] = acc;
    }
    __syncthreads();
    // 5. runs of equal bins into obs, then pv
    for (int k = tid; k < K; k += 256) {
        const int bin = bn[k];
        if (k > 0 && bn[k - 1] == bin) continue;
        double s = 0.0;
        for (int q = k; q < K && bn[q] == bin; ++q) if (P[q] > 0.0) s += P[q];
        ob[bin] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < n_bins; ++i) s += ob[i];
        p.pv[o] = fmin(s, 1.0);
    }
    for (int i = tid; i < n_bins; i += 256) orow[i] = ob[i];
}

// ---------------------------------------------------------------------------
// Probabilistic YIN, the decoding (ev_pyin_decode): Viterbi over the 2 n_bins states s = v n_bins + i (v = 0 voiced, 1 unvoiced) of one
// row, one workgroup per row, sequential in time like dtw_kernel.  Thread t owns the states t and t + blockDim.x.  Per frame and state:
//   l      = log(e + tiny), e = obs[i] (voiced) or (1 - pv) / n_bins (unvoiced)
//   delta  = max over v' in {0, 1}, j in [i - R, i + R] within [0, n_bins), in ascending s' = v' n_bins + j, a later one replacing an
//            earlier one only when STRICTLY greater, of dz[s'] + T[|i - j|], plus l; dz[s'] = delta_prev[s'] - log Z_j is what LDS holds,
//            T = t_stay (v' = v) or t_switch, log_tri[d] + log_stay / log_switch, formed on the host
// so the recursion is one float64 add and one compare per candidate: 2 (2 R + 1) of them per state; both T tables sit in LDS (128 float64).  dz is double-buffered: frame t reads
// buffer (t - 1) & 1 and writes t & 1: ONE barrier per frame.  The back-pointer byte v' (2 R + 1) + (j - i + R) goes to the caller's d_back;
// after the last frame the lowest state of greatest delta is found by a reduction and lane 0 walks the bytes back (F dependent loads).
// log Z_j reaches the kernel in 128 doubles: all of it for n_bins <= 128; else its first 64, its last 64 and between them the constant
// they both end on (R <= 63: Z_j is constant for R <= j <= n_bins - 1 - R; the host checks that the caller's table is).
struct PyinDecodeParams {
    const double* obs; const double* pv; const int32_t* len; unsigned char* back; int32_t* state; double* loglik;
    int L, F, H, n_bins, R;
    double init, tiny;                  // -log(2 n_bins); the smallest normal double
    double t_stay[64], t_switch[64];
    double zc[128];
};

__global__ __launch_bounds__(1024) void pyin_decode_kernel(const PyinDecodeParams p) {
    extern __shared__ __attribute__((aligned(16))) double pyin_lds[];
    const int b = blockIdx.x, tid = threadIdx.x, NT = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const int nb = p.n_bins, S = 2 * nb, R = p.R, F = p.F;
    int len = p.len ? p.len[b] : p.L;
    if (len < 1 || len > p.L) len = 0;
    const int nf = (int)(((long long)len + p.H - 1) / p.H);
    int32_t* st = p.state + (size_t)b * F;
    if (nf == 0) {                                                      // a bad row (uniform): no path, log-likelihood 0
        for (int t = tid; t < F; t += NT) st[t] = -1;
        if (tid == 0) p.loglik[b] = 0.0;
        return;
    }
    double* dz = pyin_lds;                                              // [2][S]
    double* rv = pyin_lds + 2 * (size_t)S;                              // [16]
    double* tT = rv + 16;                                               // [2][64]: t_stay, t_switch (a broadcast LDS read per candidate)
    int* ri = (int*)(tT + 128);                                         // [16]
    for (int d = tid; d <= R; d += NT) { tT[d] = p.t_stay[d]; tT[64 + d] = p.t_switch[d]; }   // (read from frame 1 on: behind frame 0's barrier)
    const double* ob = p.obs + (size_t)b * F * nb;
    const double* pvr = p.pv + (size_t)b * F;
    unsigned char* back = p.back + (size_t)b * F * S;
    int si[2], sv[2];
    bool have[2];
    double lz[2], delta[2], e[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int s = tid + u * NT;
        have[u] = s < S;
        sv[u] = (have[u] && s >= nb) ? 1 : 0;
        si[u] = have[u] ? s - sv[u] * nb : 0;
        const int j = si[u];
        lz[u] = nb <= 128 ? p.zc[j] : (j < 64 ? p.zc[j] : (j >= nb - 64 ? p.zc[j - (nb - 128)] : p.zc[64]));
        delta[u] = 0.0;
        e[u] = !have[u] ? 0.0 : (sv[u] ? (1.0 - pvr[0]) / (double)nb : ob[si[u]]);
    }
    for (int t = 0; t < nf; ++t) {
        double en[2] = {0.0, 0.0};
        if (t + 1 < nf) {                                               // the next frame's emissions travel while this one is decided
#pragma unroll
            for (int u = 0; u < 2; ++u)
                if (have[u]) en[u] = sv[u] ? (1.0 - pvr[t + 1]) / (double)nb : ob[(size_t)(t + 1) * nb + si[u]];
        }
        const double* prev = dz + (size_t)((t - 1) & 1) * S;
        double* cur = dz + (size_t)(t & 1) * S;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (!have[u]) continue;
            const double l = log(e[u] + p.tiny);
            if (t == 0) delta[u] = p.init + l;
            else {
                const int i = si[u];
                double best = -1.0 / 0.0;
                int arg = 0;
                for (int vp = 0; vp < 2; ++vp) {
                    const double* pr = prev + vp * nb;
                    const double* T = tT + (vp == sv[u] ? 0 : 64);
                    const int base = vp * (2 * R + 1) + R;
#pragma unroll 4
                    for (int d = -R; d <= R; ++d) {                     // ascending j = i + d; a j outside the bins is a candidate of -inf
                        const int j = i + d, ad = d < 0 ? -d : d;
                        const double c = (j >= 0 && j < nb) ? pr[min(max(j, 0), nb - 1)] + T[ad] : -1.0 / 0.0;
                        if (c > best) { best = c; arg = base + d; }
                    }
                }
                delta[u] = best + l;
                back[(size_t)t * S + tid + u * NT] = (unsigned char)arg;
            }
            cur[tid + u * NT] = delta[u] - lz[u];
        }
        e[0] = en[0]; e[1] = en[1];
        __syncthreads();
    }
    // the end state: the lowest s of greatest delta
    double bv = -1.0 / 0.0;
    int bs = 0x7fffffff;
#pragma unroll
    for (int u = 0; u < 2; ++u) if (have[u] && delta[u] > bv) { bv = delta[u]; bs = tid + u * NT; }
#pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1) {
        const double ov = __shfl_down(bv, sft);
        const int os = __shfl_down(bs, sft);
        if (ov > bv || (ov == bv && os < bs)) { bv = ov; bs = os; }
    }
    if (lane == 0) { rv[wave] = bv; ri[wave] = bs; }
    __syncthreads();
    for (int t = nf + tid; t < F; t += NT) st[t] = -1;
    if (tid != 0) return;
    const int nw = (NT + 63) >> 6;
    bv = rv[0]; bs = ri[0];
    for (int q = 1; q < nw; ++q) if (rv[q] > bv || (rv[q] == bv && ri[q] < bs)) { bv = rv[q]; bs = ri[q]; }
    p.loglik[b] = bv;
    int s = bs;
    for (int t = nf - 1; t >= 0; --t) {
        st[t] = s;
        if (t == 0) break;
        const int code = back[(size_t)t * S + s], vp = min(code / (2 * R + 1), 1), d = code - vp * (2 * R + 1) - R;
        const int v = s >= nb ? 1 : 0;
        s = vp * nb + min(max(s - v * nb + d, 0), nb - 1);             // (the clamp keeps a damaged byte inside the row's states)
    }
}

// ---------------------------------------------------------------------------
// Dynamic time warping (ev_dtw): the sibling of mas_search_kernel.  For a row with tx x ty cells
//   c[i, j] = sum_c (x[c, i] - y[c, j])^2 (float64, one fma per channel in ascending c; one __dsqrt_rn for metric 0)
//   D[i, j] = c[i, j] + min(D[i-1, j-1], D[i-1, j], D[i, j-1]) over the predecessors that exist, a later one replacing an earlier one
//             only when strictly smaller; S[i, j] = S[chosen] + 1, S[0, 0] = 1
// One workgroup per row walks the tx + ty - 1 anti-diagonals k = i + j, one barrier each.  Thread t owns the matrix rows i = t + r NT,
// r < R.  A ring of three diagonals of D (float64) and of S (16 bits: S <= 8191) lives in LDS, indexed by i: diagonal k is written to
// buffer k % 3 while k - 1 (up, at i - 1) and k - 2 (diagonal, at i - 1) are read, which is why one barrier per diagonal is enough;
// the left neighbour D[i, j - 1] is the thread's own previous cell and stays in a register.  The cell does exactly the sequential
// loop's arithmetic: the wavefront is the only parallelism.
// Local costs: W diagonals ahead of the DP each thread forms the W cells of its rows into REGISTERS (acc[R][W]): x[c, i] is read once
// per channel and block, y[c, k - i] W times, both coalesced over i; columns are clamped into [0, ty), so nothing behind a row's length
// is read and cells outside the matrix cost nothing that is used.  The cost matrix never exists in memory.
// Decision: 2 bits per cell (0 diagonal, 1 up, 2 left), 32 cells of a matrix row per 64-bit word, gathered in a register and stored
// once per 32 columns at word (j / 32) * Tx + i: in LDS where they fit beside the ring, else in the handle's arena (p.gbits); none
// when no path is asked for.  Thread 0 replays the bits from (tx-1, ty-1) into an LDS stage that reuses the ring (K = S[tx-1, ty-1]
// is known, so entry k goes to slot k), then the workgroup writes the path in ascending order and the -1 tail.
// No atomics; nothing depends on B, Tx, Ty, the block size or ev_set_arithmetic.
struct DtwParams {
    const float* x; const float* y; const int32_t* xlen; const int32_t* ylen;
    double* cost; int32_t* steps; int32_t* path;
    unsigned long long* gbits;          // decision words per row [nyw][Tx], or NULL: in LDS (or no path)
    int C, Tx, Ty, nyw, metric;
    int off_s, off_bits;                // LDS plan in bytes (the D ring, and later the path stage, are at 0)
};

template <int R, int W>
__global__ __launch_bounds__(1024) void dtw_kernel(const DtwParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dtw_lds[];
    __shared__ int dtw_K;
    const int b = blockIdx.x, tid = threadIdx.x, NT = blockDim.x;
    const int C = p.C, Tx = p.Tx, Ty = p.Ty, NP = Tx + Ty - 1;
    int tx = p.xlen ? p.xlen[b] : Tx, ty = p.ylen ? p.ylen[b] : Ty;
    int32_t* path = p.path ? p.path + (size_t)b * NP * 2 : nullptr;
    if (tx < 1 || ty < 1 || tx > Tx || ty > Ty) {                       // a bad row (uniform over the workgroup): cost 0, steps 0, path -1
        if (tid == 0) { p.cost[b] = 0.0; p.steps[b] = 0; }
        if (path) for (int e = tid; e < 2 * NP; e += NT) path[e] = -1;
        return;
    }
    double* ring = (double*)dtw_lds;                                    // [3][Tx]
    unsigned short* sring = (unsigned short*)(dtw_lds + p.off_s);       // [3][Tx]
    unsigned long long* bits = !path ? nullptr : (p.gbits ? p.gbits + (size_t)b * p.nyw * Tx : (unsigned long long*)(dtw_lds + p.off_bits));
    const float* xb = p.x + (size_t)b * C * Tx;
    const float* yb = p.y + (size_t)b * C * Ty;
    double leftD[R];
    int leftS[R];
    unsigned long long word[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { leftD[r] = 0.0; leftS[r] = 0; word[r] = 0ull; }
    double* d0 = ring;                                                  // diagonal k
    double* d1 = ring + Tx;                                             // k - 1
    double* d2 = ring + 2 * Tx;                                         // k - 2
    unsigned short* s0 = sring;
    unsigned short* s1 = sring + Tx;
    unsigned short* s2 = sring + 2 * Tx;
    const int nk = tx + ty - 1;
    for (int k0 = 0; k0 < nk; k0 += W) {
        double acc[R][W];
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int w = 0; w < W; ++w) acc[r][w] = 0.0;
            const int i = tid + r * NT, j0 = k0 - i;
            if (i >= tx || j0 + W <= 0 || j0 >= ty) continue;            // no cell of this row on these diagonals
            int jc[W];
#pragma unroll
            for (int w = 0; w < W; ++w) jc[w] = min(max(j0 + w, 0), ty - 1);
            for (int c = 0; c < C; ++c) {
                const double xv = (double)xb[(size_t)c * Tx + i];
                const float* yr = yb + (size_t)c * Ty;
#pragma unroll
                for (int w = 0; w < W; ++w) { const double d = xv - (double)yr[jc[w]]; acc[r][w] = fma(d, d, acc[r][w]); }
            }
            if (p.metric == 0) {
#pragma unroll
                for (int w = 0; w < W; ++w) acc[r][w] = __dsqrt_rn(acc[r][w]);
            }
        }
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const int k = k0 + w;
            if (k < nk) {                                                // (uniform)
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int i = tid + r * NT, j = k - i;
                    if (i < tx && j >= 0 && j < ty) {
                        double best = 0.0;
                        int sb = 0, ch = 0;
                        bool have = false;
                        if (i > 0) {
                            if (j > 0) { best = d2[i - 1]; sb = s2[i - 1]; have = true; }
                            const double up = d1[i - 1];
                            if (!have || up < best) { best = up; sb = s1[i - 1]; ch = 1; have = true; }
                        }
                        if (j > 0 && (!have || leftD[r] < best)) { best = leftD[r]; sb = leftS[r]; ch = 2; }
                        const double D = acc[r][w] + best;               // (cell (0, 0): best = 0 is added, D = c exactly)
                        const int S = sb + 1;
                        d0[i] = D; s0[i] = (unsigned short)S;
                        leftD[r] = D; leftS[r] = S;
                        if (bits) {
                            word[r] |= (unsigned long long)ch << (2 * (j & 31));
                            if ((j & 31) == 31 || j == ty - 1) { bits[(size_t)(j >> 5) * Tx + i] = word[r]; word[r] = 0ull; }
                        }
                        if (i == tx - 1 && j == ty - 1) { p.cost[b] = D; p.steps[b] = S; dtw_K = S; }
                    }
                }
                __syncthreads();
                double* t = d2; d2 = d1; d1 = d0; d0 = t;
                unsigned short* u = s2; s2 = s1; s1 = s0; s0 = u;
            }
        }
    }
    if (!path) return;
    const int K = dtw_K;                                                // (written before the last barrier)
    unsigned int* stage = (unsigned int*)dtw_lds;                       // [K]: i | j << 16, over the ring that is no longer read
    if (tid == 0) {
        int i = tx - 1, j = ty - 1;
        for (int k = K - 1; k >= 0; --k) {
            stage[k] = (unsigned int)i | ((unsigned int)j << 16);
            int ch = (int)((bits[(size_t)(j >> 5) * Tx + i] >> (2 * (j & 31))) & 3ull);
            if (i == 0) ch = 2; else if (j == 0) ch = 1;                 // (what the forward step recorded there; keeps the walk inside the matrix)
            if (ch != 2) --i;
            if (ch != 1) --j;
            if (i < 0 || j < 0) break;                                   // (0, 0) was entry 0
        }
    }
    __syncthreads();
    for (int e = tid; e < 2 * NP; e += NT) {
        const int k = e >> 1;
        int v = -1;
        if (k < K) { const unsigned int s = stage[k]; v = (e & 1) ? (int)(s >> 16) : (int)(s & 0xffffu); }
        path[e] = v;
    }
}

// ---------------------------------------------------------------------------
// Loudness (ev_loudness): ITU-R BS.1770-4 K-weighting, 100 ms sub-block energies, 400 ms blocks, two gates.  All float64.
// The K-weighting is two biquads in series, each in transposed direct form II (what scipy.signal.lfilter runs):
//     y = b0 x + s1;   s1 = (b1 x + s2) - a1 y;   s2 = b2 x - a2 y
// so a row's filter state is FOUR doubles (s1, s2 of the shelf, then of the high pass) and the filter is linear in (state, input): the state
// after a chunk of LOUD_CHUNK samples is (the state the chunk reaches from zero) + M . (the state before it), M the 4 x 4 zero-input
// transition over one chunk (the host runs this very recurrence on the four unit states and passes M by value).  A row is therefore NOT one
// chain of len steps but three launches whose longest chain is one chunk plus the carry:
//   1. loud_chunk_kernel<false>: one lane per (row, chunk) runs its chunk from zero state and keeps the four doubles;
//   2. loud_carry_kernel:        one wave per row forms s[c + 1] = M s[c] + z[c] in ascending c, in place: slot c then holds the state at the
//                                START of chunk c;
//   3. loud_chunk_kernel<true>:  one lane per (row, chunk) reruns the chunk from that state and sums y^2 per PIECE, a piece being the part of
//                                one sub-block that lies inside the chunk (one fma per sample, ascending);
// then loud_merge_kernel adds the pieces of sub-block i over the chunks it touches in ascending chunk order (e_i), and loud_gate_kernel forms
// the blocks, both gates and the two means per row.  No atomics anywhere; the chunk grid hangs on the row's first sample, so nothing depends
// on the batch, on L or on what lies behind the row.
// Only samples below lim = (len / S) S are ever read (the incomplete tail is discarded by the standard, and nothing at or behind len may be
// read).  Staging: a workgroup is ONE wave holding 64 consecutive chunks of a row; a lane reading its own chunk straight from memory would be
// a 4 KiB-strided access, so the wave loads a tile of 64 chunks x LOUD_T samples with 16-byte loads (8 lanes per chunk: 128 contiguous bytes)
// into LDS rows of LOUD_T + 4 floats (9 sixteen-byte slots: 16 consecutive lanes reading their rows' same quad hit 16 different slots) and
// each lane then reads its row with 16-byte LDS loads.  The next tile's global loads are issued before the current tile is filtered and
// written to the other LDS buffer after it: one barrier per tile.
constexpr int LOUD_CHUNK = 1024;                                        // samples per chunk
constexpr int LOUD_T = 32;                                              // samples per chunk and staged tile
constexpr int LOUD_ROW = LOUD_T + 4;                                    // floats per LDS row

struct LoudCoef { double b0, b1, b2, a1, a2, c0, c1, c2, d1, d2; };     // stage 1 (b, a), stage 2 (c, d)

struct LoudChunkParams {
    const float* x; const int32_t* len; double* state; double* part;   // state (B, NC, 4); part (B, NC, npp)
    int L, S, NC, npp;
    LoudCoef k;
};

__device__ __forceinline__ long long loud_lim(const int32_t* len, int b, int L, int S) {
    int n = len ? len[b] : L;
    if (n < 1 || n > L) n = 0;                                          // a bad row is an empty row (the ev_mas_align convention)
    return (long long)(n / S) * S;
}

template <bool ENERGY>
__global__ __launch_bounds__(64) void loud_chunk_kernel(const LoudChunkParams p) {
    __shared__ __attribute__((aligned(16))) float xs[2][64 * LOUD_ROW];
    const int b = blockIdx.y, lane = threadIdx.x;
    const long long lim = loud_lim(p.len, b, p.L, p.S);
    const long long c0 = (long long)blockIdx.x * 64;                    // the wave's first chunk
    if (c0 * LOUD_CHUNK >= lim) return;                                 // (uniform) nothing of this row in these chunks
    const float* xrow = p.x + (size_t)b * p.L;
    const bool vec = (((size_t)xrow) & 15) == 0;                        // (chunks and tiles start at multiples of 4 samples of the row)
    const long long c = c0 + lane, n0 = c * LOUD_CHUNK;
    const int cnt = (int)max(0LL, min((long long)LOUD_CHUNK, lim - n0));    // samples of this lane's chunk below lim
    const int ntile = (int)((min((long long)LOUD_CHUNK, lim - c0 * LOUD_CHUNK) + LOUD_T - 1) / LOUD_T);   // (uniform: lane 0 has the most)
    const LoudCoef k = p.k;
    double s1 = 0.0, s2 = 0.0, u1 = 0.0, u2 = 0.0;
    double acc = 0.0;
    int rem = 0;
    double* part = nullptr;
    if (ENERGY) {
        if (cnt > 0) {
            const double* st = p.state + ((size_t)b * p.NC + c) * 4;
            s1 = st[0]; s2 = st[1]; u1 = st[2]; u2 = st[3];
        }
        const long long i0 = n0 / p.S;
        rem = (int)((i0 + 1) * p.S - n0);                               // samples left in the sub-block the chunk starts in
        part = p.part + ((size_t)b * p.NC + (cnt > 0 ? c : 0)) * p.npp;
    }
    // the tile loader: instruction r of 8 covers chunks 8 r .. 8 r + 7, lane -> (chunk 8 r + lane / 8, quad lane % 8)
    const int lq = lane & 7, lc = lane >> 3;
    f32x4 stage[8];
    auto load_tile = [&](int t) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const long long n = (c0 + 8 * r + lc) * LOUD_CHUNK + t * LOUD_T + 4 * lq;
            f32x4 q = {0.f, 0.f, 0.f, 0.f};
            if (n + 4 <= lim) {
                if (vec) q = *(const f32x4*)(xrow + n);
                else { q[0] = xrow[n]; q[1] = xrow[n + 1]; q[2] = xrow[n + 2]; q[3] = xrow[n + 3]; }
            } else if (n < lim) {
                if (n + 0 < lim) q[0] = xrow[n];
                if (n + 1 < lim) q[1] = xrow[n + 1];
                if (n + 2 < lim) q[2] = xrow[n + 2];
                if (n + 3 < lim) q[3] = xrow[n + 3];
            }
            stage[r] = q;
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int r = 0; r < 8; ++r) *(f32x4*)(&xs[buf][(8 * r + lc) * LOUD_ROW + 4 * lq]) = stage[r];
    };
    load_tile(0);
    store_tile(0);
    __syncthreads();
    for (int t = 0; t < ntile; ++t) {
        if (t + 1 < ntile) load_tile(t + 1);
        const float* row = &xs[t & 1][lane * LOUD_ROW];
        const int v = cnt - t * LOUD_T;                                 // samples of this tile that belong to the lane's chunk (may be <= 0)
#pragma unroll
        for (int j = 0; j < LOUD_T / 4; ++j) {
            const f32x4 q = *(const f32x4*)(row + 4 * j);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double x = (double)q[e];
                const double y1 = fma(k.b0, x, s1);
                s1 = fma(-k.a1, y1, fma(k.b1, x, s2));
                s2 = fma(-k.a2, y1, k.b2 * x);
                const double y2 = fma(k.c0, y1, u1);
                u1 = fma(-k.d1, y2, fma(k.c1, y1, u2));
                u2 = fma(-k.d2, y2, k.c2 * y1);
                if (ENERGY) {
                    if (4 * j + e < v) {
                        acc = fma(y2, y2, acc);
                        if (--rem == 0) { *part++ = acc; acc = 0.0; rem = p.S; }
                    }
                }
            }
        }
        if (t + 1 < ntile) store_tile((t + 1) & 1);
        __syncthreads();
    }
    if (ENERGY) {
        if (cnt > 0 && rem != p.S) *part = acc;                         // the piece the chunk's end cuts (lim is a multiple of S: the row's last
    } else {                                                            // chunk ends on a sub-block's end and leaves none)
        if (cnt == LOUD_CHUNK) {
            double* st = p.state + ((size_t)b * p.NC + c) * 4;
            st[0] = s1; st[1] = s2; st[2] = u1; st[3] = u2;
        }
    }
}

// The carry.  One wave per row; every lane walks the same chain (uniform work, no divergence): 64 chunk results at a time come into LDS with
// one coalesced load, the chain takes them in ascending order, lane k keeps the state at the start of chunk base + k, and one coalesced store
// puts those back in place.  s'[r] = (M[r][0] s0 + M[r][1] s1) + (z[r] + M[r][2] s2 + M[r][3] s3), fmas in that association.
struct LoudCarryParams {
    double* state; const int32_t* len;
    int L, S, NC;
    double M[16];
};

__global__ __launch_bounds__(64) void loud_carry_kernel(const LoudCarryParams p) {
    __shared__ double zs[64][4];
    const int b = blockIdx.x, lane = threadIdx.x;
    const long long lim = loud_lim(p.len, b, p.L, p.S);
    const long long nact = (lim + LOUD_CHUNK - 1) / LOUD_CHUNK;         // chunks that hold a sample below lim; all but the last are whole
    double* st = p.state + (size_t)b * p.NC * 4;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (long long base = 0; base < nact; base += 64) {
        const long long c = base + lane;
        const bool whole = c < nact - 1;                                // (the last active chunk's result is not needed, and may not exist)
#pragma unroll
        for (int r = 0; r < 4; ++r) zs[lane][r] = whole ? st[c * 4 + r] : 0.0;
        __syncthreads();
        double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0;
        const int n = (int)min(64LL, nact - base);
        for (int kk = 0; kk < n; ++kk) {
            if (lane == kk) { m0 = s0; m1 = s1; m2 = s2; m3 = s3; }
            const double z0 = zs[kk][0], z1 = zs[kk][1], z2 = zs[kk][2], z3 = zs[kk][3];
            const double t0 = fma(p.M[1], s1, p.M[0] * s0) + fma(p.M[3], s3, fma(p.M[2], s2, z0));
            const double t1 = fma(p.M[5], s1, p.M[4] * s0) + fma(p.M[7], s3, fma(p.M[6], s2, z1));
            const double t2 = fma(p.M[9], s1, p.M[8] * s0) + fma(p.M[11], s3, fma(p.M[10], s2, z2));
            const double t3 = fma(p.M[13], s1, p.M[12] * s0) + fma(p.M[15], s3, fma(p.M[14], s2, z3));
            s0 = t0; s1 = t1; s2 = t2; s3 = t3;
        }
        __syncthreads();
        if (c < nact) { st[c * 4] = m0; st[c * 4 + 1] = m1; st[c * 4 + 2] = m2; st[c * 4 + 3] = m3; }
    }
}

// e[b, i] = the pieces of sub-block i, added in ascending chunk order starting from the first piece itself; 0 for i >= ns.
struct LoudMergeParams {
    const double* part; const int32_t* len; double* sub;               // sub (B, NS)
    int L, S, NC, npp, NS;
};

__global__ __launch_bounds__(256) void loud_merge_kernel(const LoudMergeParams p) {
    const int b = blockIdx.y;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.NS) return;
    const long long ns = loud_lim(p.len, b, p.L, p.S) / p.S;
    double e = 0.0;
    if (i < ns) {
        const long long c_lo = i * p.S / LOUD_CHUNK, c_hi = ((i + 1) * p.S - 1) / LOUD_CHUNK;
        const double* part = p.part + (size_t)b * p.NC * p.npp;
        for (long long c = c_lo; c <= c_hi; ++c) {
            const double v = part[c * p.npp + (i - c * LOUD_CHUNK / p.S)];
            e = c == c_lo ? v : e + v;
        }
    }
    p.sub[(size_t)b * p.NS + i] = e;
}

// One workgroup per row over its sub-block energies: z[j] = ((e[j] + e[j+1]) + (e[j+2] + e[j+3])) / (4 S) for j < nb = max(ns - 3, 0); the
// absolute gate z > abs_gate; m_abs = the mean of the blocks that pass it; the relative gate z > 0.1 m_abs on top; the mean of the blocks
// that pass both.  SUMMATION ORDER of either mean: thread t of 256 adds its blocks j = t, t + 256, ... in ascending j; the 64 partials of a
// wave are added by the fixed shuffle tree (offsets 32, 16, ... 1); the four waves' sums as (w0 + w1) + (w2 + w3).  It depends on j alone.
struct LoudGateParams {
    const double* sub; const int32_t* len; double* block; double* gated; int32_t* counts;
    int L, S, NS, NB;
    double abs_gate;
};

__device__ __forceinline__ double loud_block(const double* e, long long j, double four_s) {
    return ((e[j] + e[j + 1]) + (e[j + 2] + e[j + 3])) / four_s;
}

__device__ __forceinline__ void loud_reduce(double& s, int& n, double* red_d, int* red_i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_down(s, o); n += __shfl_down(n, o); }
    __syncthreads();                                                    // (the previous use of red_* is over)
    if ((threadIdx.x & 63) == 0) { red_d[threadIdx.x >> 6] = s; red_i[threadIdx.x >> 6] = n; }
    __syncthreads();
    s = (red_d[0] + red_d[1]) + (red_d[2] + red_d[3]);
    n = (red_i[0] + red_i[1]) + (red_i[2] + red_i[3]);
}

__global__ __launch_bounds__(256) void loud_gate_kernel(const LoudGateParams p) {
    __shared__ double red_d[4];
    __shared__ int red_i[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long ns = loud_lim(p.len, b, p.L, p.S) / p.S;
    const long long nb = ns > 3 ? ns - 3 : 0;
    const double* e = p.sub + (size_t)b * p.NS;
    const double four_s = 4.0 * (double)p.S;
    if (p.block)
        for (long long j = tid; j < p.NB; j += 256) p.block[(size_t)b * p.NB + j] = j < nb ? loud_block(e, j, four_s) : 0.0;
    double s = 0.0;
    int n = 0;
    for (long long j = tid; j < nb; j += 256) {
        const double z = loud_block(e, j, four_s);
        if (z > p.abs_gate) { s += z; ++n; }
    }
    loud_reduce(s, n, red_d, red_i);
    const int n_abs = n;
    const double m_abs = n_abs > 0 ? s / (double)n_abs : 0.0;
    const double rel = 0.1 * m_abs;
    s = 0.0; n = 0;
    for (long long j = tid; j < nb; j += 256) {
        const double z = loud_block(e, j, four_s);
        if (z > p.abs_gate && z > rel) { s += z; ++n; }
    }
    loud_reduce(s, n, red_d, red_i);
    if (tid == 0) {
        p.gated[2 * b] = n > 0 ? s / (double)n : 0.0;
        p.gated[2 * b + 1] = m_abs;
        p.counts[3 * b] = (int32_t)nb; p.counts[3 * b + 1] = n_abs; p.counts[3 * b + 2] = n;
    }
}

// ---------------------------------------------------------------------------
// STOI / ESTOI (ev_stoi): short-time objective intelligibility of a processed row y against a clean row x (Taal et al. 2011; Jensen and
// Taal 2016).  All float64; every kernel below compiles with floating-point contraction OFF (STOI_EXACT), so an fma is an fma only where fma()
// is written and a product that feeds a sum is rounded first wherever `*` and `+` are written.  No atomics.  Five launches:
//   1. stoi_energy_kernel:   one lane per (row, frame f): E[f] = fma chain over j of t_j^2, t_j = w[j] x[f H + j], ascending j, from 0;
//   2. stoi_select_kernel:   one workgroup per row: the maximum of E (exact in any order), the mask E[f] > silence_ratio * max, and an
//                            ordered compaction of the kept frames into idx (256 frames per round: one ballot and one popcount prefix per
//                            wave, the four waves' totals through LDS, the running base carried from round to round); writes d_keep and
//                            d_counts = {nf, nk, nseg};
//   3. stoi_band_kernel:     one workgroup per (row, frame m) for BOTH signals (they share every twiddle read): z through LDS, one lane per
//                            bin, four fma chains per lane (re and im of x and of y), then one lane per band;
//   4. stoi_segment_kernel:  one wave per (row, segment): the N frames of every band through LDS; one lane per band for STOI, then one lane
//                            per band and one lane per frame for the two normalisations of ESTOI;
//   5. stoi_mean_kernel:     one workgroup per row: the two means in the fixed tree of loud_reduce.
// Everything a row's outputs depend on hangs on the row's own samples below len: nothing depends on the batch, on L or on what lies behind.
#define STOI_EXACT _Pragma("clang fp contract(off)")
constexpr double STOI_EPS = 2.220446049250313e-16;                     // 2^-52

struct StoiTables { const double* win; const double* tw; const int32_t* bands; int W, H, nfft, n_bands, N, bin_lo, bin_hi; };

__device__ __forceinline__ int stoi_frames(const int32_t* len, int b, int L, int W, int H) {
    int n = len ? len[b] : L;
    if (n < 1 || n > L) n = 0;                                          // a bad row is an empty row (the ev_mas_align convention)
    return n > W ? (n - W + H - 1) / H : 0;                             // range(0, n - W, H): a row of exactly W + k H samples has k frames
}

struct StoiEnergyParams { const float* x; const int32_t* len; double* E; StoiTables t; int L, NF; };

__global__ __launch_bounds__(64) void stoi_energy_kernel(const StoiEnergyParams p) {
    STOI_EXACT
    const int b = blockIdx.y, f = blockIdx.x * 64 + threadIdx.x;
    if (f >= p.NF) return;
    const int nf = stoi_frames(p.len, b, p.L, p.t.W, p.t.H);
    double e = 0.0;
    if (f < nf) {
        const float* x = p.x + (size_t)b * p.L + (size_t)f * p.t.H;    // (f H + W - 1 < len: the frame lies inside the row)
#pragma unroll 8
        for (int j = 0; j < p.t.W; ++j) {                               // (W is a multiple of 64: the loads of eight steps go out together)
            const double t = p.t.win[j] * (double)x[j];
            e = fma(t, t, e);
        }
    }
    p.E[(size_t)b * p.NF + f] = e;
}

struct StoiSelectParams { const double* E; const int32_t* len; int32_t* idx; uint8_t* keep; int32_t* counts; StoiTables t; int L, NF; double ratio; };

__global__ __launch_bounds__(256) void stoi_select_kernel(const StoiSelectParams p) {
    STOI_EXACT
    __shared__ double red_d[4];
    __shared__ int red_i[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nf = stoi_frames(p.len, b, p.L, p.t.W, p.t.H);
    const double* E = p.E + (size_t)b * p.NF;
    double mx = 0.0;                                                    // (energies are >= 0)
    for (int f = tid; f < nf; f += 256) mx = fmax(mx, E[f]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
    if (lane == 0) red_d[wv] = mx;
    __syncthreads();
    mx = fmax(fmax(red_d[0], red_d[1]), fmax(red_d[2], red_d[3]));
    const double thr = p.ratio * mx;
    int base = 0;                                                       // kept frames before this round (uniform)
    for (int f0 = 0; f0 < nf; f0 += 256) {
        const int f = f0 + tid;
        const bool k = f < nf && E[f] > thr;
        const unsigned long long m = __ballot(k);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        __syncthreads();                                                // (the previous round's red_i is read)
        if (lane == 0) red_i[wv] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wv; ++w) off += red_i[w];
        if (k) p.idx[(size_t)b * p.NF + off + before] = f;
        base += (red_i[0] + red_i[1]) + (red_i[2] + red_i[3]);
        if (p.keep && f < p.NF) p.keep[(size_t)b * p.NF + f] = k ? 1 : 0;
    }
    if (p.keep) {                                                       // zeros from the last round's end up to NF (nf <= NF)
        const int done = (nf + 255) / 256 * 256;
        for (int f = done + tid; f < p.NF; f += 256) p.keep[(size_t)b * p.NF + f] = 0;
    }
    if (tid == 0) {
        const int nm = base > 0 ? base - 1 : 0;
        p.counts[3 * b] = nf; p.counts[3 * b + 1] = base; p.counts[3 * b + 2] = nm >= p.t.N ? nm - p.t.N + 1 : 0;
    }
}

// Band spectra of frame m of the silence-removed signals, which never exist in memory: sample n = m H + j of s gathers from the kept frames
// k = n / H - 1 and n / H (W = 2 H: exactly two overlap), i.e. from kept frames m - 1 and m for j < H and m and m + 1 for j >= H
// (m + 1 <= nk - 1 always, m - 1 >= 0 from the second frame on).  s = t_lo + t_hi with t_k = w[n - k H] * x[idx[k] H + n - k H], each product
// rounded, added in ascending k (the first frame's lower half has the one term); z[j] = w[j] * s.  Bin k of lane (k - bin_lo):
// re = fma(z[j], cos[(j k) mod nfft], re), sm = fma(z[j], sin[(j k) mod nfft], sm) over ascending j from 0, im = -sm, p = fma(im, im, re * re).
// Band: the p of its bins added in ascending k from 0, then sqrt (correctly rounded).  LDS (doubles): [twiddle 2 nfft][z 2 W][p 2 nbin].
struct StoiBandParams { const float* x; const float* y; const int32_t* idx; const int32_t* counts; double* tob; StoiTables t; int L, NF, NM; };

__global__ __launch_bounds__(256) void stoi_band_kernel(const StoiBandParams p) {
    STOI_EXACT
    extern __shared__ __attribute__((aligned(16))) double stoi_smem[];
    const int b = blockIdx.y, m = blockIdx.x, tid = threadIdx.x;
    const int W = p.t.W, H = p.t.H, nfft = p.t.nfft, nb = p.t.n_bands;
    const int nk = p.counts[3 * b + 1], nm = nk > 0 ? nk - 1 : 0;
    double* tobx = p.tob + ((size_t)b * 2 * nb) * p.NM + m;             // band r of x at tobx[r NM], of y at tobx[(nb + r) NM]
    if (m >= nm) {                                                      // (uniform) zeros past the row's own frames
        for (int r = tid; r < 2 * nb; r += 256) tobx[(size_t)r * p.NM] = 0.0;
        return;
    }
    double* tw = stoi_smem;                                             // (nfft, 2)
    double* zx = tw + 2 * nfft;                                         // (W)
    double* zy = zx + W;
    double* px = zy + W;                                                // (bin_hi - bin_lo)
    const int nbin = p.t.bin_hi - p.t.bin_lo;
    double* py = px + nbin;
    for (int i = tid; i < 2 * nfft; i += 256) tw[i] = p.t.tw[i];
    const int32_t* idx = p.idx + (size_t)b * p.NF;
    const float* xr = p.x + (size_t)b * p.L;
    const float* yr = p.y + (size_t)b * p.L;
    for (int j = tid; j < W; j += 256) {
        const int k_hi = j < H ? m : m + 1, k_lo = k_hi - 1;            // the two kept frames that overlap at sample m H + j
        const int o_hi = j < H ? j : j - H, o_lo = o_hi + H;            // the sample's offset inside each
        const size_t a_hi = (size_t)idx[k_hi] * H + o_hi;
        const double w_hi = p.t.win[o_hi];
        double sx = w_hi * (double)xr[a_hi], sy = w_hi * (double)yr[a_hi];
        if (k_lo >= 0) {
            const size_t a_lo = (size_t)idx[k_lo] * H + o_lo;
            const double w_lo = p.t.win[o_lo];
            sx = w_lo * (double)xr[a_lo] + sx;
            sy = w_lo * (double)yr[a_lo] + sy;
        }
        const double wj = p.t.win[j];
        zx[j] = wj * sx;
        zy[j] = wj * sy;
    }
    __syncthreads();
    for (int q = tid; q < nbin; q += 256) {
        const int k = p.t.bin_lo + q;                                   // k <= nfft / 2 < nfft
        double rx = 0.0, ix = 0.0, ry = 0.0, iy = 0.0;
        int ph = 0;                                                     // (j k) mod nfft
        for (int j = 0; j < W; ++j) {
            const double c = tw[2 * ph], s = tw[2 * ph + 1];
            const double a = zx[j], d = zy[j];
            rx = fma(a, c, rx); ix = fma(a, s, ix);
            ry = fma(d, c, ry); iy = fma(d, s, iy);
            ph += k;
            if (ph >= nfft) ph -= nfft;
        }
        ix = -ix; iy = -iy;
        px[q] = fma(ix, ix, rx * rx);
        py[q] = fma(iy, iy, ry * ry);
    }
    __syncthreads();
    for (int r = tid; r < 2 * nb; r += 256) {
        const int band = r < nb ? r : r - nb;
        const double* pp = r < nb ? px : py;
        const int k0 = p.t.bands[2 * band] - p.t.bin_lo, k1 = p.t.bands[2 * band + 1] - p.t.bin_lo;
        double acc = 0.0;
        for (int k = k0; k < k1; ++k) acc = acc + pp[k];
        tobx[(size_t)r * p.NM] = sqrt(acc);
    }
}

// One wave per (row, segment q): frames [q, q + N) of every band of both signals in LDS rows of NP = N | 1 doubles (an odd stride: the lanes
// that each walk one band's row hit different banks).  EVERY sum below runs in ascending index from 0, `a * a` terms as fma(a, a, sum).
// STOI, lane = band r: nx = sqrt(sum X^2), ny = sqrt(sum Y^2), a = nx / (ny + EPS); Y'[i] = min(a * Y[i], clip * X[i]); mx = (sum X) / N,
//   my = (sum Y') / N; dx = sqrt(sum (X - mx)^2) + EPS, dy = sqrt(sum (Y' - my)^2) + EPS; rho = sum of ((X - mx) / dx) * ((Y' - my) / dy).
//   d_seg[q][0] = (sum of rho over the bands, ascending) / n_bands.
// ESTOI, X and Y alike, in place: lane = band: mean over the N frames (sum / N) removed, then divided by (sqrt(sum of squares) + EPS);
//   lane = frame: mean over the bands (sum / n_bands) removed, then divided by (sqrt(sum of squares) + EPS); c_i = fma chain over the bands of
//   X[r][i] * Y[r][i]; d_seg[q][1] = (sum of c_i over the frames, ascending) / N.
struct StoiSegParams { const double* tob; const int32_t* counts; double* seg; StoiTables t; int NM, NSEG; double clip; };

__global__ __launch_bounds__(64) void stoi_segment_kernel(const StoiSegParams p) {
    STOI_EXACT
    extern __shared__ __attribute__((aligned(16))) double stoi_smem[];
    const int b = blockIdx.y, q = blockIdx.x, lane = threadIdx.x;
    const int N = p.t.N, nb = p.t.n_bands, NP = N | 1;
    const int nseg = p.counts[3 * b + 2];
    double* out = p.seg + ((size_t)b * p.NSEG + q) * 2;
    if (q >= nseg) {                                                    // (uniform)
        if (lane < 2) out[lane] = 0.0;
        return;
    }
    double* X = stoi_smem;                                              // (nb, NP)
    double* Y = X + nb * NP;
    double* red = Y + nb * NP;                                          // (64)
    const double* src = p.tob + ((size_t)b * 2 * nb) * p.NM + q;
    for (int r = 0; r < nb; ++r)
        if (lane < N) { X[r * NP + lane] = src[(size_t)r * p.NM + lane]; Y[r * NP + lane] = src[(size_t)(nb + r) * p.NM + lane]; }
    __syncthreads();
    const double dN = (double)N, dB = (double)nb;
    double rho = 0.0;
    if (lane < nb) {
        const double* x = X + lane * NP;
        const double* y = Y + lane * NP;
        double sxx = 0.0, syy = 0.0;
        for (int i = 0; i < N; ++i) { sxx = fma(x[i], x[i], sxx); syy = fma(y[i], y[i], syy); }
        const double a = sqrt(sxx) / (sqrt(syy) + STOI_EPS);
        double sx = 0.0, sy = 0.0;
        for (int i = 0; i < N; ++i) { sx = sx + x[i]; sy = sy + fmin(a * y[i], p.clip * x[i]); }
        const double mx = sx / dN, my = sy / dN;
        sxx = 0.0; syy = 0.0;
        for (int i = 0; i < N; ++i) {
            const double u = x[i] - mx, v = fmin(a * y[i], p.clip * x[i]) - my;
            sxx = fma(u, u, sxx); syy = fma(v, v, syy);
        }
        const double dx = sqrt(sxx) + STOI_EPS, dy = sqrt(syy) + STOI_EPS;
        for (int i = 0; i < N; ++i) {
            const double u = (x[i] - mx) / dx, v = (fmin(a * y[i], p.clip * x[i]) - my) / dy;
            rho = rho + u * v;
        }
    }
    red[lane] = rho;
    __syncthreads();
    if (lane == 0) {
        double s = 0.0;
        for (int r = 0; r < nb; ++r) s = s + red[r];
        out[0] = s / dB;
    }
    __syncthreads();                                                    // (STOI has read X and Y; ESTOI rewrites them)
    if (lane < nb) {
#pragma unroll
        for (int sig = 0; sig < 2; ++sig) {
            double* v = (sig ? Y : X) + lane * NP;
            double s = 0.0;
            for (int i = 0; i < N; ++i) s = s + v[i];
            const double mu = s / dN;
            double ss = 0.0;
            for (int i = 0; i < N; ++i) { const double u = v[i] - mu; ss = fma(u, u, ss); }
            const double d = sqrt(ss) + STOI_EPS;
            for (int i = 0; i < N; ++i) v[i] = (v[i] - mu) / d;
        }
    }
    __syncthreads();
    double c = 0.0;
    if (lane < N) {
#pragma unroll
        for (int sig = 0; sig < 2; ++sig) {
            double* v = (sig ? Y : X) + lane;
            double s = 0.0;
            for (int r = 0; r < nb; ++r) s = s + v[r * NP];
            const double mu = s / dB;
            double ss = 0.0;
            for (int r = 0; r < nb; ++r) { const double u = v[r * NP] - mu; ss = fma(u, u, ss); }
            const double d = sqrt(ss) + STOI_EPS;
            for (int r = 0; r < nb; ++r) v[r * NP] = (v[r * NP] - mu) / d;
        }
        for (int r = 0; r < nb; ++r) c = fma(X[r * NP + lane], Y[r * NP + lane], c);
    }
    red[lane] = c;
    __syncthreads();
    if (lane == 0) {
        double s = 0.0;
        for (int i = 0; i < N; ++i) s = s + red[i];
        out[1] = s / dN;
    }
}

// d_score[b] = {mean of d_seg[., 0], mean of d_seg[., 1]} over the row's nseg segments, 0 without a segment: thread t of 256 adds its segments
// t, t + 256, ... in ascending order, the 64 partials of a wave go through the shuffle tree (offsets 32 .. 1), the four waves' sums are added
// as (w0 + w1) + (w2 + w3) — the tree of ev_loudness — and one division by nseg follows.
struct StoiMeanParams { const double* seg; const int32_t* counts; double* score; int NSEG; };

__global__ __launch_bounds__(256) void stoi_mean_kernel(const StoiMeanParams p) {
    STOI_EXACT
    __shared__ double red[2][4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nseg = p.counts[3 * b + 2];
    const double* seg = p.seg + (size_t)b * p.NSEG * 2;
    double s0 = 0.0, s1 = 0.0;
    for (int q = tid; q < nseg; q += 256) { s0 = s0 + seg[2 * q]; s1 = s1 + seg[2 * q + 1]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s0 = s0 + __shfl_down(s0, o); s1 = s1 + __shfl_down(s1, o); }
    if ((tid & 63) == 0) { red[0][tid >> 6] = s0; red[1][tid >> 6] = s1; }
    __syncthreads();
    if (tid < 2) {
        const double s = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
        p.score[2 * b + tid] = nseg > 0 ? s / (double)nseg : 0.0;
    }
}

// ---------------------------------------------------------------------------
// Multi-resolution STFT distance (ev_stft_dist): spectral convergence, log-magnitude L1 (Yamamoto et al. 2020) and log-spectral distance of a
// processed row y against a reference row x at ONE resolution (W, H, nfft); the caller runs it once per resolution.  All float64, contraction
// OFF (STOI_EXACT), no atomics.  The DFT is a float64 GEMM on v_mfma_f64_16x16x4_f64: frames x samples times the dense windowed basis
//   basis[j][k] = {w[j] cos(2 pi (j + off) k / nfft), w[j] sin(2 pi (j + off) k / nfft)},  off = (nfft - W) / 2,  0 <= j < W,  0 <= k < NB,
// which stft_dist_basis_kernel builds once per load (one rounding per entry, the phase index in exact integers), {cos, sin} interleaved so
// that one 16-byte load feeds both planes.  Launches of a call:
//   1. stft_dist_frames_kernel: one workgroup of 4 waves per (row, 16 frames from the row's frame 0) -> d_frame (B, NF, 4);
//   2. stft_dist_rows_kernel:   one workgroup per row: the four sums in the fixed tree of loud_reduce / stoi_mean_kernel, and the count.
// Everything a row's outputs depend on hangs on the row's own samples below len.
struct StftDistTables { const double2* basis; int W, H, nfft, NB, skew; };
typedef double stftd_acc __attribute__((ext_vector_type(4)));

// (n, nf) of row b: a row with len < 1, len > L or len <= nfft / 2 is an empty row (the reflect padding of nfft / 2 needs more samples)
__device__ __forceinline__ int stftd_frames(const int32_t* len, int b, int L, const StftDistTables& t, int* n_out) {
    int n = len ? len[b] : L;
    if (n < 1 || n > L || n <= t.nfft / 2) n = 0;
    *n_out = n;
    return n > 0 ? 1 + n / t.H : 0;
}

struct StftBasisParams { const double* win; const double* tw; double2* basis; int W, nfft, NB; };

__global__ __launch_bounds__(256) void stft_dist_basis_kernel(const StftBasisParams p) {
    STOI_EXACT
    const int i = blockIdx.x * 256 + threadIdx.x;                       // (W NB <= 2048 x 1025)
    if (i >= p.W * p.NB) return;
    const int j = i / p.NB, k = i - j * p.NB;
    const int ph = ((j + (p.nfft - p.W) / 2) * k) % p.nfft;             // (< 2048 x 1024: exact)
    const double w = p.win[j];
    p.basis[i] = make_double2(w * p.tw[2 * ph], w * p.tw[2 * ph + 1]);
}

// ---------------------------------------------------------------------------
// The float64 DFT GEMM of stft_dist_frames_kernel and voice_quality_kernel: what both share.  A workgroup of 4 waves owns a tile of 16
// frames; wave w owns the column tiles (bins, or quefrencies) w, w + 4, ... of 16 columns; per column tile the K dimension runs in steps of
// one v_mfma_f64_16x16x4_f64 per (signal, plane).  Lane l of an A fragment holds row (frame) l & 15 at k0 + (l >> 4), lane l of a B fragment
// row k0 + (l >> 4) of the basis at column l & 15 (read from global memory: L2-resident), and register i of lane l of an accumulator is frame
// (l >> 4) + 4 i, column l & 15.
// SKEW.  A tile's raw span of 15 H + W samples is staged once into LDS as fp32 and an A fragment reads t = (l & 15) H + k0 + (l >> 4), widened
// on the way out: with ds_read_b32 banked over 32 words and served in two groups of 32 lanes, a frame stride H = 0 mod 4 (240: 16 banks) lands
// the 16 frames of a group on few banks.  So sample t lives at word t + skew * (t / H) with skew = (2 - H) mod 4, and the frame stride
// H + skew is 2 mod 4: 2 r (odd) mod 32 is 16 distinct even banks for r = 0 .. 15, and the two k of a lane group fill the odd ones —
// conflict-free (except where k0 + (l >> 4) crosses a multiple of H inside a group).  At most 3 (16 + W / H) pad words per signal.
__host__ __device__ __forceinline__ int dft_skew(int H) { return ((2 - H) % 4 + 4) % 4; }
__host__ __device__ __forceinline__ int dft_span_words(int span, int H, int skew) { return span + skew * ((span - 1) / H); }   // (the last word + 1)
__device__ __forceinline__ int dft_word(int t, int H, int skew) { return t + skew * (t / H); }

// The word of sample r H + j of frame r, r (H + skew) + j + skew (j / H), for j = q, q + 4, ... without a division per step:
// (j + 4) / H = j / H + 4 / H + (j % H + 4 % H >= H); step_pad is non-zero for H < 4 only.
struct DftSkewWalk {
    int H, skew, step_mod, step_pad, rbase, j, jm, pad;
    __device__ __forceinline__ DftSkewWalk(int r, int h, int k) : H(h), skew(k), step_mod(4 % h), step_pad(k * (4 / h)), rbase(r * (h + k)), j(0), jm(0), pad(0) {}
    __device__ __forceinline__ void start(int q) { j = q; jm = q % H; pad = skew * (q / H); }
    __device__ __forceinline__ int word() const { return rbase + j + pad; }
    __device__ __forceinline__ void step() { j += 4; jm += step_mod; pad += step_pad; if (jm >= H) { jm -= H; pad += skew; } }
};

// The hand-over of per-frame sums: over the 16 column lanes of a frame by one xor tree (offsets 8, 4, 2, 1; in each kernel, its sums side by
// side), then, from the waves' partials in LDS (red[wave][frame][term]), over the waves as ((w0 + w1) + w2) + w3.
template <int C>
__device__ __forceinline__ double dft_waves_sum(const double (&red)[4][16][C], int fr, int c) { STOI_EXACT return ((red[0][fr][c] + red[1][fr][c]) + red[2][fr][c]) + red[3][fr][c]; }

// One workgroup per (row b, tile of 16 frames f0 .. f0 + 15).  The tile's raw span, samples f0 H - W / 2 + t for 0 <= t < 15 H + W of both
// signals, is staged with the reflection applied (what a frame >= nf would read outside the row is staged as 0 and that frame is masked):
// 78 160 bytes for both signals at H = 511, W = 2048, the largest footprint.  Per bin tile W / 4 steps of four MFMAs (x c, x s, y c, y s):
// the A fragment of each signal serves both planes, the B fragment both signals.  Epilogue per (frame, bin): p = max(fma(sm, sm, re * re),
// floor), m = sqrt(p), l = log(p) for both signals; the four terms are accumulated per frame over the wave's bin tiles in ascending order
// (squares as fma(d, d, sum)) and handed over.  Bins >= NB (the address is clamped, the term dropped) and frames >= nf (zeros) are masked.
struct StftFramesParams { const float* x; const float* y; const int32_t* len; double* frame; StftDistTables t; int L, NF; double floor; };

__global__ __launch_bounds__(256) void stft_dist_frames_kernel(const StftFramesParams p) {
    STOI_EXACT
    extern __shared__ __attribute__((aligned(16))) float stftd_smem[];
    __shared__ double red[4][16][4];
    const int b = blockIdx.y, f0 = blockIdx.x * 16, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int W = p.t.W, H = p.t.H, NB = p.t.NB, skew = p.t.skew;
    int n;
    const int nf = stftd_frames(p.len, b, p.L, p.t, &n);
    double* out = p.frame + ((size_t)b * p.NF + f0) * 4;
    if (f0 >= nf) {                                                     // (uniform) zeros past the row's own frames
        if (tid < 64 && f0 + (tid >> 2) < p.NF) out[tid] = 0.0;
        return;
    }
    const int span = 15 * H + W;
    float* sx = stftd_smem;
    float* sy = sx + dft_span_words(span, H, skew);
    {
        const float* xr = p.x + (size_t)b * p.L;
        const float* yr = p.y + (size_t)b * p.L;
        const long long i0 = (long long)f0 * H - W / 2;
        for (int t = tid; t < span; t += 256) {
            long long i = i0 + t;
            if (i < 0) i = -i;
            else if (i >= n) i = 2LL * (n - 1) - i;
            const bool ok = i >= 0 && i < n;                            // (always, for a frame < nf)
            const int a = dft_word(t, H, skew);
            sx[a] = ok ? xr[i] : 0.f;
            sy[a] = ok ? yr[i] : 0.f;
        }
    }
    __syncthreads();
    const int r = lane & 15, q = lane >> 4;
    const int ntile = (NB + 15) >> 4, nsteps = W >> 2;
    DftSkewWalk walk(r, H, skew);
    double t0[4] = {0.0, 0.0, 0.0, 0.0}, t1[4] = {0.0, 0.0, 0.0, 0.0}, t2[4] = {0.0, 0.0, 0.0, 0.0}, t3[4] = {0.0, 0.0, 0.0, 0.0};
    for (int bt = wv; bt < ntile; bt += 4) {
        const int col = bt * 16 + r;
        const double2* bp = p.t.basis + (size_t)q * NB + (col < NB ? col : NB - 1);
        stftd_acc xc = {0.0, 0.0, 0.0, 0.0}, xs = xc, yc = xc, ys = xc;
        walk.start(q);
        // four steps per round; the basis of the NEXT round is requested before this round's products (the index clamped at the last
        // step: a repeated load, never one past the basis), so its L2 latency hides behind sixteen matrix instructions
        double2 cur[4], nxt[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) cur[u] = bp[(size_t)(u < nsteps ? u : nsteps - 1) * 4 * NB];
        for (int s0 = 0; s0 < nsteps; s0 += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) nxt[u] = bp[(size_t)(s0 + 4 + u < nsteps ? s0 + 4 + u : nsteps - 1) * 4 * NB];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (s0 + u < nsteps) {                                  // (uniform)
                    const int a = walk.word();
                    const double ax = (double)sx[a], ay = (double)sy[a];
                    xc = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, cur[u].x, xc, 0, 0, 0);
                    xs = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, cur[u].y, xs, 0, 0, 0);
                    yc = __builtin_amdgcn_mfma_f64_16x16x4f64(ay, cur[u].x, yc, 0, 0, 0);
                    ys = __builtin_amdgcn_mfma_f64_16x16x4f64(ay, cur[u].y, ys, 0, 0, 0);
                    walk.step();
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
        }
        if (col < NB) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double px = fmax(fma(xs[i], xs[i], xc[i] * xc[i]), p.floor), py = fmax(fma(ys[i], ys[i], yc[i] * yc[i]), p.floor);
                const double mx = sqrt(px), my = sqrt(py);
                const double dm = my - mx, dl = log(py) - log(px);
                t0[i] = fma(dm, dm, t0[i]);
                t1[i] = fma(mx, mx, t1[i]);
                t2[i] = t2[i] + fabs(dl);
                t3[i] = fma(dl, dl, t3[i]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {
            t0[i] = t0[i] + __shfl_xor(t0[i], o, 64); t1[i] = t1[i] + __shfl_xor(t1[i], o, 64);
            t2[i] = t2[i] + __shfl_xor(t2[i], o, 64); t3[i] = t3[i] + __shfl_xor(t3[i], o, 64);
        }
        if (r == 0) { double* d = red[wv][q + 4 * i]; d[0] = t0[i]; d[1] = t1[i]; d[2] = t2[i]; d[3] = t3[i]; }
    }
    __syncthreads();
    if (tid < 64) {
        const int fr = tid >> 2, c = tid & 3;
        const double v = dft_waves_sum(red, fr, c);
        if (f0 + fr < p.NF) out[tid] = f0 + fr < nf ? v : 0.0;
    }
}

// d_sums[b] = {sum_f d_frame[f][0], sum_f [1], sum_f [2], sum_f sqrt([3] / NB)} over the row's nf frames, d_counts[b] = nf: thread t of 256
// adds its frames t, t + 256, ... in ascending order, the 64 partials of a wave go through the shuffle tree (offsets 32 .. 1), the four
// waves' sums are added as (w0 + w1) + (w2 + w3) — the tree of ev_loudness / ev_stoi.
struct StftRowsParams { const double* frame; const int32_t* len; double* sums; int32_t* counts; StftDistTables t; int L, NF; };

__global__ __launch_bounds__(256) void stft_dist_rows_kernel(const StftRowsParams p) {
    STOI_EXACT
    __shared__ double red[4][4];
    const int b = blockIdx.x, tid = threadIdx.x;
    int n;
    const int nf = stftd_frames(p.len, b, p.L, p.t, &n);
    const double* fr = p.frame + (size_t)b * p.NF * 4;
    const double dNB = (double)p.t.NB;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int f = tid; f < nf; f += 256) {
        s0 = s0 + fr[4 * (size_t)f]; s1 = s1 + fr[4 * (size_t)f + 1]; s2 = s2 + fr[4 * (size_t)f + 2];
        s3 = s3 + sqrt(fr[4 * (size_t)f + 3] / dNB);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s0 = s0 + __shfl_down(s0, o); s1 = s1 + __shfl_down(s1, o); s2 = s2 + __shfl_down(s2, o); s3 = s3 + __shfl_down(s3, o);
    }
    if ((tid & 63) == 0) { red[0][tid >> 6] = s0; red[1][tid >> 6] = s1; red[2][tid >> 6] = s2; red[3][tid >> 6] = s3; }
    __syncthreads();
    if (tid < 4) p.sums[4 * (size_t)b + tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
    if (tid == 0) p.counts[b] = nf;
}

// ---------------------------------------------------------------------------
// Voice quality (ev_voice_quality): the spectral-balance descriptors of eGeMAPS (alpha ratio, Hammarberg index, the spectral slopes of two bands;
// Eyben et al. 2016) and the cepstral peak prominence (Hillenbrand et al. 1994) of every frame of a row, from ONE float64 log-power spectrum
// and its linear real cepstrum.  All float64, contraction OFF (STOI_EXACT), no atomics.  Two GEMMs on v_mfma_f64_16x16x4_f64, chained
// through LDS inside one launch:
//   GEMM 1  frames x samples times ev_stft_dist's windowed basis {w[j] cos, w[j] sin}(2 pi (j + off) k / nfft) (stft_dist_basis_kernel builds it):
//           raw = fma(sm, sm, re * re), p = max(raw, floor), Ldb = (10 / ln 10) log(p);
//   GEMM 2  Ldb (16 frames x NBp bins, from LDS) times cep[k][q - q_fit] = g[k] cos_tab[(k q) mod nfft] / nfft (g = 1 at k = 0 and k = nfft / 2,
//           else 2; rows NB <= k < NBp = the next multiple of 4 are zeros), which voiceq_cep_basis_kernel builds once per load: one rounding
//           of the quotient per entry (g cos is exact), the phase index in exact integers.
// Everything a row's outputs depend on hangs on the row's own samples below len.
struct VoiceQTables {
    const double2* basis; const double* cep; const double* slope_w; const double* fit_w;
    int W, H, nfft, NB, NBp, NQ, skew, S, q_fit, q_min, q_max;
    int band[12];                                                       // {first, end} of alpha lo, alpha hi, Hammarberg lo, Hammarberg hi, slope 0, slope 1
    double q_mean;
};
constexpr double VOICEQ_DB = 4.342944819032518;                         // 10 / ln 10

// (n, nf) of row b: a row with len < 1 or len > L is an empty row; nf = ceil(n / H), pitch_yin's frames
__device__ __forceinline__ int voiceq_frames(const int32_t* len, int b, int L, int H, int* n_out) {
    int n = len ? len[b] : L;
    if (n < 1 || n > L) n = 0;
    *n_out = n;
    return (int)(((long long)n + H - 1) / H);
}

struct VoiceQCepParams { const double* tw; double* cep; int nfft, NB, NBp, NQ, q_fit; };

__global__ __launch_bounds__(256) void voiceq_cep_basis_kernel(const VoiceQCepParams p) {
    STOI_EXACT
    const int i = blockIdx.x * 256 + threadIdx.x;                       // (NBp NQ <= 516 x 512)
    if (i >= p.NBp * p.NQ) return;
    const int k = i / p.NQ, q = p.q_fit + (i - k * p.NQ);
    const int ph = (k * q) % p.nfft;                                    // (< 516 x 512: exact)
    const double g = (k == 0 || k == p.nfft / 2) ? 1.0 : 2.0;
    p.cep[i] = k < p.NB ? g * p.tw[2 * ph] / (double)p.nfft : 0.0;
}

// One workgroup of 4 waves per (row b, tile of 16 frames f0 .. f0 + 15), on the shared pieces above.  Dynamic LDS: Ld, the tile's log-spectrum
// (16 frames x S doubles), then the tile's raw span, samples f0 H + H / 2 - W / 2 + t for 0 <= t < 15 H + W, staged under the skew with ZEROS
// outside [0, len) (no reflection).
// PHASE 1 is stft_dist_frames_kernel's loop for one signal: per bin tile W / 4 steps of two MFMAs (cos, sin).  Epilogue per (frame, bin): raw,
// p, Ldb as above; Ldb goes to Ld[frame S + bin]; per frame the lane accumulates over its tiles in ascending order: the two alpha sums and the
// power (s = s + p), the two slope sums (s = fma(slope_w[b][k], Ldb, s) over every bin: the weights outside a band are zeros), the two
// Hammarberg maxima, the count of bins with raw > floor; then the hand-over (the maxima by fmax through the same tree and over the waves).
// PHASE 2, after one barrier: wave w owns the quefrency tiles w, w + 4, ... of 16 columns from q_fit; per tile NBp / 4 steps of one MFMA.  Lane
// l of an A fragment reads Ld[(l & 15) S + k0 + (l >> 4)] with ds_read_b64 (k >= NB: the address is clamped to NB - 1, the basis row is zero);
// the B fragment is cep[k0 + (l >> 4)][16 tile + (l & 15)] (the column clamped at NQ - 1, the term dropped).
// BANKS: ds_read_b64 is banked over 64 dwords and served in two groups of 32 lanes; lane l of a group reads dwords 2 ((l & 15) S + k0 + q)
// and the next one, q = l >> 4 in {0, 1} or {2, 3}.  With S = 2 mod 32, 2 r S = 4 r mod 64: the group's 32 lanes start at the dword banks
// 4 r + 2 q + const, all 32 even residues mod 64, each read covering its even bank and the odd one after it: all 64 banks once, conflict-free.
// S is the smallest such number >= NB (NB = 513: S = 514).  The epilogue's stores of Ldb (once per bin tile) are not conflict-free and need not be.
// Epilogue per (frame, quefrency): sum C (s = s + C) and sum fit_w C (s = fma(fit_w, C, s)) over the lane's tiles in ascending order, the
// maximum over q_min <= q <= q_max with its index (strictly greater replaces: the lowest q of a tie), optionally the store of C; the sums are
// handed over, the maximum through the same tree (of equal maxima the lower index) and over the waves in the order w0 .. w3.
// Thread f < 16 then forms the frame's eight figures: mean = sum C / NQ, base = mean + (sum fit_w C) (q* - q_mean), cpp = C[q*] - base,
// alpha = (10 / ln 10) (log(hi) - log(lo)).  A SILENT frame (no bin with raw > floor) keeps its power; its other figures, d_peak and
// cepstrum are zeros by definition.  Frames >= nf are zeros.
struct VoiceQParams { const float* x; const int32_t* len; double* frame; int32_t* peak; double* cepstrum; VoiceQTables t; int L, NF; double floor; };

__global__ __launch_bounds__(256) void voice_quality_kernel(const VoiceQParams p) {
    STOI_EXACT
    extern __shared__ __attribute__((aligned(16))) double voiceq_smem[];
    __shared__ double red[4][16][7];
    __shared__ int red_live[4][16];
    __shared__ double red2[4][16][3];
    __shared__ int red2_i[4][16];
    const int b = blockIdx.y, f0 = blockIdx.x * 16, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int W = p.t.W, H = p.t.H, NB = p.t.NB, NQ = p.t.NQ, skew = p.t.skew, S = p.t.S;
    int n;
    const int nf = voiceq_frames(p.len, b, p.L, H, &n);
    double* out = p.frame + ((size_t)b * p.NF + f0) * 8;
    int32_t* pk = p.peak + (size_t)b * p.NF + f0;
    double* cp = p.cepstrum ? p.cepstrum + ((size_t)b * p.NF + f0) * NQ : nullptr;
    const int nfr = p.NF - f0 < 16 ? p.NF - f0 : 16;                    // the tile's frames inside the outputs (>= 1)
    if (f0 >= nf) {                                                     // (uniform) zeros past the row's own frames
        if (tid < 8 * nfr) out[tid] = 0.0;
        if (tid < nfr) pk[tid] = 0;
        if (cp) for (int i = tid; i < nfr * NQ; i += 256) cp[i] = 0.0;
        return;
    }
    double* Ld = voiceq_smem;                                           // (16, S)
    float* sx = (float*)(Ld + 16 * S);
    const int span = 15 * H + W;
    {
        const float* xr = p.x + (size_t)b * p.L;
        const long long i0 = (long long)f0 * H + H / 2 - W / 2;
        for (int t = tid; t < span; t += 256) {
            const long long i = i0 + t;
            sx[dft_word(t, H, skew)] = i >= 0 && i < n ? xr[i] : 0.f;
        }
    }
    __syncthreads();
    const int r = lane & 15, q = lane >> 4;
    {
        const int ntile = (NB + 15) >> 4, nsteps = W >> 2;
        DftSkewWalk walk(r, H, skew);
        const double ninf = -__builtin_huge_val();
        double al[4] = {0.0, 0.0, 0.0, 0.0}, ah[4] = {0.0, 0.0, 0.0, 0.0}, s0[4] = {0.0, 0.0, 0.0, 0.0}, s1[4] = {0.0, 0.0, 0.0, 0.0};
        double pw[4] = {0.0, 0.0, 0.0, 0.0}, hl[4] = {ninf, ninf, ninf, ninf}, hh[4] = {ninf, ninf, ninf, ninf};
        int live[4] = {0, 0, 0, 0};
        for (int bt = wv; bt < ntile; bt += 4) {
            const int col = bt * 16 + r, colc = col < NB ? col : NB - 1;
            const double2* bp = p.t.basis + (size_t)q * NB + colc;
            const double w0 = p.t.slope_w[colc], w1 = p.t.slope_w[NB + colc];
            stftd_acc xc = {0.0, 0.0, 0.0, 0.0}, xs = xc;
            walk.start(q);
            double2 cur[4], nxt[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) cur[u] = bp[(size_t)(u < nsteps ? u : nsteps - 1) * 4 * NB];
            for (int t0 = 0; t0 < nsteps; t0 += 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) nxt[u] = bp[(size_t)(t0 + 4 + u < nsteps ? t0 + 4 + u : nsteps - 1) * 4 * NB];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (t0 + u < nsteps) {                              // (uniform)
                        const double ax = (double)sx[walk.word()];
                        xc = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, cur[u].x, xc, 0, 0, 0);
                        xs = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, cur[u].y, xs, 0, 0, 0);
                        walk.step();
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
            }
            if (col < NB) {
                const bool in_al = col >= p.t.band[0] && col < p.t.band[1], in_ah = col >= p.t.band[2] && col < p.t.band[3];
                const bool in_hl = col >= p.t.band[4] && col < p.t.band[5], in_hh = col >= p.t.band[6] && col < p.t.band[7];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double raw = fma(xs[i], xs[i], xc[i] * xc[i]);
                    const double pp = fmax(raw, p.floor);
                    const double ld = VOICEQ_DB * log(pp);
                    Ld[(q + 4 * i) * S + col] = ld;
                    if (in_al) al[i] = al[i] + pp;
                    if (in_ah) ah[i] = ah[i] + pp;
                    if (in_hl) hl[i] = fmax(hl[i], ld);
                    if (in_hh) hh[i] = fmax(hh[i], ld);
                    s0[i] = fma(w0, ld, s0[i]);
                    s1[i] = fma(w1, ld, s1[i]);
                    pw[i] = pw[i] + pp;
                    live[i] += raw > p.floor ? 1 : 0;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) {
                al[i] = al[i] + __shfl_xor(al[i], o, 64); ah[i] = ah[i] + __shfl_xor(ah[i], o, 64);
                s0[i] = s0[i] + __shfl_xor(s0[i], o, 64); s1[i] = s1[i] + __shfl_xor(s1[i], o, 64);
                pw[i] = pw[i] + __shfl_xor(pw[i], o, 64);
                hl[i] = fmax(hl[i], __shfl_xor(hl[i], o, 64)); hh[i] = fmax(hh[i], __shfl_xor(hh[i], o, 64));
                live[i] += __shfl_xor(live[i], o, 64);
            }
            if (r == 0) {
                double* d = red[wv][q + 4 * i];
                d[0] = al[i]; d[1] = ah[i]; d[2] = hl[i]; d[3] = hh[i]; d[4] = s0[i]; d[5] = s1[i]; d[6] = pw[i];
                red_live[wv][q + 4 * i] = live[i];
            }
        }
    }
    __syncthreads();                                                    // Ld and the band terms are complete
    {
        const int nqt = (NQ + 15) >> 4, nsteps = p.t.NBp >> 2;
        const double ninf = -__builtin_huge_val();
        bool keep[4];                                                   // the frame is one of the row's and is not silent
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int fr = q + 4 * i;
            keep[i] = f0 + fr < nf && red_live[0][fr] + red_live[1][fr] + red_live[2][fr] + red_live[3][fr] > 0;
        }
        double sc[4] = {0.0, 0.0, 0.0, 0.0}, sf[4] = {0.0, 0.0, 0.0, 0.0}, bv[4] = {ninf, ninf, ninf, ninf};
        int bi[4] = {0, 0, 0, 0};
        const double* La = Ld + r * S;
        for (int qt = wv; qt < nqt; qt += 4) {
            const int col = qt * 16 + r;
            const double* bp = p.t.cep + (size_t)q * NQ + (col < NQ ? col : NQ - 1);
            stftd_acc c = {0.0, 0.0, 0.0, 0.0};
            double cur[4], nxt[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) cur[u] = bp[(size_t)(u < nsteps ? u : nsteps - 1) * 4 * NQ];
            for (int t0 = 0; t0 < nsteps; t0 += 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) nxt[u] = bp[(size_t)(t0 + 4 + u < nsteps ? t0 + 4 + u : nsteps - 1) * 4 * NQ];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (t0 + u < nsteps) {                              // (uniform)
                        const int k = 4 * (t0 + u) + q;
                        c = __builtin_amdgcn_mfma_f64_16x16x4f64(La[k < NB ? k : NB - 1], cur[u], c, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
            }
            if (col < NQ) {
                const double fw = p.t.fit_w[col];
                const bool srch = p.t.q_fit + col >= p.t.q_min;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    sc[i] = sc[i] + c[i];
                    sf[i] = fma(fw, c[i], sf[i]);
                    if (srch && c[i] > bv[i]) { bv[i] = c[i]; bi[i] = col; }
                    if (cp && q + 4 * i < nfr) cp[(size_t)(q + 4 * i) * NQ + col] = keep[i] ? c[i] : 0.0;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) {
                sc[i] = sc[i] + __shfl_xor(sc[i], o, 64); sf[i] = sf[i] + __shfl_xor(sf[i], o, 64);
                const double ov = __shfl_xor(bv[i], o, 64);
                const int oi = __shfl_xor(bi[i], o, 64);
                if (ov > bv[i] || (ov == bv[i] && oi < bi[i])) { bv[i] = ov; bi[i] = oi; }
            }
            if (r == 0) {
                double* d = red2[wv][q + 4 * i];
                d[0] = sc[i]; d[1] = sf[i]; d[2] = bv[i];
                red2_i[wv][q + 4 * i] = bi[i];
            }
        }
    }
    __syncthreads();
    if (tid < nfr) {
        const int fr = tid;
        double cpp = 0.0, alpha = 0.0, ham = 0.0, sl0 = 0.0, sl1 = 0.0, power = 0.0, cq = 0.0, base = 0.0;
        int qs = 0;
        if (f0 + fr < nf) {
            power = dft_waves_sum(red, fr, 6);
            if (red_live[0][fr] + red_live[1][fr] + red_live[2][fr] + red_live[3][fr] > 0) {
                const double lo = dft_waves_sum(red, fr, 0);
                const double hi = dft_waves_sum(red, fr, 1);
                alpha = VOICEQ_DB * (log(hi) - log(lo));
                ham = fmax(fmax(red[0][fr][2], red[1][fr][2]), fmax(red[2][fr][2], red[3][fr][2]))
                    - fmax(fmax(red[0][fr][3], red[1][fr][3]), fmax(red[2][fr][3], red[3][fr][3]));
                sl0 = dft_waves_sum(red, fr, 4);
                sl1 = dft_waves_sum(red, fr, 5);
                const double sumc = dft_waves_sum(red2, fr, 0);
                const double sumf = dft_waves_sum(red2, fr, 1);
                cq = red2[0][fr][2];
                int bi = red2_i[0][fr];
#pragma unroll
                for (int w = 1; w < 4; ++w) {
                    const double v = red2[w][fr][2];
                    const int vi = red2_i[w][fr];
                    if (v > cq || (v == cq && vi < bi)) { cq = v; bi = vi; }
                }
                qs = p.t.q_fit + bi;
                base = sumc / (double)NQ + sumf * ((double)qs - p.t.q_mean);
                cpp = cq - base;
            }
        }
        double* o = out + 8 * fr;
        o[0] = cpp; o[1] = alpha; o[2] = ham; o[3] = sl0; o[4] = sl1; o[5] = power; o[6] = cq; o[7] = base;
        pk[fr] = qs;
    }
}

// ---------------------------------------------------------------------------
// Formants (ev_formants): per frame the linear prediction of the pre-emphasised, windowed samples by Burg's lattice, the roots of the prediction
// polynomial by the Aberth-Ehrlich iteration (all at once), and the formants as the roots of the upper half plane inside the band, lowest first
// (the definition: include/emojivoice.h).  All float64, contraction OFF (STOI_EXACT), no atomics, no scratch, no LDS, no barrier: ONE WAVE PER
// FRAME, four frames to a workgroup of 256 threads, and everything a frame needs lives in its wave's registers.
//   samples   lane l holds y[n], n = l R + r for 0 <= r < R, R = the power of two >= ceil(W / 64) (<= 16), read straight from the row (ZEROS outside
//             [0, len), no reflection); n >= W holds 0 and never takes part.  W < 64: lanes >= ceil(W / R) hold nothing.
//   Burg      f[R], b[R] in registers; b[n - 1] of a lane's first sample is lane l - 1's last (one __shfl_up).  num and den: the lane adds its
//             terms in ascending r (terms outside m <= n < W are +0.0), then an xor tree over the 64 lanes (offsets 32 .. 1): every lane ends with
//             the same bits.  E0 the same way.  Lane i holds a[i]; step m reads a[m - i] by one shuffle.
//   roots     lane i < p owns z_i (starting points: the host's table in the arguments).  a_1 .. a_p and the other lanes' roots come by wave
//             broadcasts (__shfl from a uniform lane) in ascending index; P and P' by one complex Horner pass; complex products and quotients
//             by the textbook formulas ((a c + b d, b c - a d) / (c^2 + d^2) for the quotient).  max |w| is an fmax xor tree.
//   formants  rank counting: a candidate's slot is the number of candidates below it (of equal f the lower lane first); lane s < n_formants
//             collects the candidate of rank s and stores slot s, zeros where there is none.
// Orders are fixed and depend on the frame's own samples and the loaded geometry only.
struct FormantParams {
    const float* x; const int32_t* len; const double* win; double* lpc; double* formant; int32_t* count;
    int L, NF, W, H, order, nform;
    double pre, floor, f_scale, bw_scale, f_lo, f_hi;                   // f_scale = sr / (2 pi), bw_scale = sr / pi, f_hi = sr / 2 - f_lo
    double z0[64];                                                      // {re, im} of the starting points 0.9 exp(i (2 pi i / p + 0.4))
};
constexpr double FORMANT_STOP = 9.313225746154785e-10;                  // 2^-30
constexpr int FORMANT_MAX_ITERS = 64;

__device__ __forceinline__ double formant_wave_sum(double v) {
    STOI_EXACT
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

template <int R>
__global__ __launch_bounds__(256) void formants_kernel(const FormantParams p) {
    STOI_EXACT
    const int b = blockIdx.y, lane = threadIdx.x & 63, fr = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (fr >= p.NF) return;                                             // (wave-uniform; the kernel has no barrier)
    const int W = p.W, P = p.order, NFM = p.nform;
    int n;
    const int nf = voiceq_frames(p.len, b, p.L, p.H, &n);
    const size_t fi = (size_t)b * p.NF + fr;
    double* o_lpc = p.lpc ? p.lpc + fi * (P + 2) : nullptr;
    double* o_fm = p.formant + fi * NFM * 2;
    if (fr >= nf) {                                                     // zeros past the row's own frames (and in a row without frames)
        if (o_lpc && lane < P + 2) o_lpc[lane] = 0.0;
        if (lane < 2 * NFM) o_fm[lane] = 0.0;
        if (lane == 0) p.count[fi] = 0;
        return;
    }
    // ---- the windowed, pre-emphasised samples and E0
    double f[R], bk[R];
    double e0 = 0.0;
    {
        const float* xr = p.x + (size_t)b * p.L;
        const long long i0 = (long long)fr * p.H + p.H / 2 - W / 2 + (long long)lane * R;
        long long i = i0 - 1;
        double prev = i >= 0 && i < n ? (double)xr[i] : 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            i = i0 + r;
            const int j = lane * R + r;
            const double s = i >= 0 && i < n ? (double)xr[i] : 0.0;
            const double y = j < W ? p.win[j] * (s - p.pre * prev) : 0.0;
            prev = s;
            f[r] = y; bk[r] = y;
            e0 = e0 + y * y;
        }
        e0 = formant_wave_sum(e0);
    }
    if (!(e0 > p.floor)) {                                              // SILENT (uniform): zeros
        if (o_lpc && lane < P + 2) o_lpc[lane] = 0.0;
        if (lane < 2 * NFM) o_fm[lane] = 0.0;
        if (lane == 0) p.count[fi] = 0;
        return;
    }
    // ---- Burg's lattice
    double a = lane == 0 ? 1.0 : 0.0;                                   // lane i: a[i]
    double gain = e0 / (double)W;
    for (int m = 1; m <= P; ++m) {
        const double up = __shfl_up(bk[R - 1], 1, 64);
        double bp[R];
        double num = 0.0, den = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int j = lane * R + r;
            const bool on = j >= m && j < W;
            bp[r] = r == 0 ? up : bk[r - 1];
            num = num + (on ? f[r] * bp[r] : 0.0);
            den = den + (on ? f[r] * f[r] + bp[r] * bp[r] : 0.0);
        }
        num = -2.0 * formant_wave_sum(num);
        den = formant_wave_sum(den);
        const double k = den > 0.0 ? num / den : 0.0;
#pragma unroll
        for (int r = R - 1; r >= 0; --r) {
            const int j = lane * R + r;
            if (j >= m && j < W) {
                const double fo = f[r];
                f[r] = fo + k * bp[r];
                bk[r] = bp[r] + k * fo;
            }
        }
        const int src = m - lane;
        const double am = __shfl(a, src >= 0 ? src : 0, 64);
        if (lane >= 1 && lane <= m) a = a + k * am;
        gain = gain * (1.0 - k * k);
    }
    if (o_lpc) {
        if (lane >= 1 && lane <= P) o_lpc[lane - 1] = a;
        if (lane == 0) { o_lpc[P] = gain; o_lpc[P + 1] = e0; }
    }
    // ---- the roots: Aberth-Ehrlich, lane i < P owns z_i
    const bool own = lane < P;
    double zr = p.z0[2 * (own ? lane : 0)], zi = p.z0[2 * (own ? lane : 0) + 1];
    int left = -1;
    bool conv = false;
    for (int it = 0; it < FORMANT_MAX_ITERS; ++it) {
        double pr = 1.0, pi = 0.0, dr = 0.0, di = 0.0;                  // P(z), P'(z) by Horner
        for (int i = 1; i <= P; ++i) {
            const double ai = __shfl(a, i, 64);
            const double ndr = (dr * zr - di * zi) + pr, ndi = (dr * zi + di * zr) + pi;
            const double npr = (pr * zr - pi * zi) + ai, npi = pr * zi + pi * zr;
            dr = ndr; di = ndi; pr = npr; pi = npi;
        }
        const double dd = dr * dr + di * di;
        const double rr = (pr * dr + pi * di) / dd, ri = (pi * dr - pr * di) / dd;   // r = P / P'
        double sr = 0.0, si = 0.0;                                      // s = sum_{j != i} 1 / (z_i - z_j)
        for (int j = 0; j < P; ++j) {
            const double qr = zr - __shfl(zr, j, 64), qi = zi - __shfl(zi, j, 64);
            if (j != lane) {
                const double q2 = qr * qr + qi * qi;
                sr = sr + qr / q2;
                si = si - qi / q2;
            }
        }
        const double tr = 1.0 - (rr * sr - ri * si), ti = -(rr * si + ri * sr);      // 1 - r s
        const double t2 = tr * tr + ti * ti;
        const double wr = (rr * tr + ri * ti) / t2, wi = (ri * tr - rr * ti) / t2;   // w = r / (1 - r s)
        zr = zr - wr; zi = zi - wi;
        double mx = own ? sqrt(wr * wr + wi * wi) : 0.0;
        const bool bad = own && !(isfinite(zr) && isfinite(zi));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
        if (__any(bad)) break;                                          // (uniform) UNCONVERGED
        if (left < 0) { if (mx <= FORMANT_STOP) left = 2; }
        else if (--left == 0) { conv = true; break; }
    }
    if (!conv) {                                                        // UNCONVERGED: the coefficients stay, the formants are zeros
        if (lane < 2 * NFM) o_fm[lane] = 0.0;
        if (lane == 0) p.count[fi] = -1;
        return;
    }
    // ---- candidates, ranks, slots
    const double fq = own ? atan2(zi, zr) * p.f_scale : 0.0;
    const double bw = own ? -log(sqrt(zr * zr + zi * zi)) * p.bw_scale : 0.0;
    const bool cand = own && zi > 0.0 && fq > p.f_lo && fq < p.f_hi;
    int rank = 0, total = 0;
    for (int j = 0; j < P; ++j) {
        const double fj = __shfl(fq, j, 64);
        const int cj = __shfl((int)cand, j, 64);
        total += cj;
        if (cj && (fj < fq || (fj == fq && j < lane))) ++rank;
    }
    double of = 0.0, ob = 0.0;
    for (int j = 0; j < P; ++j) {
        const double fj = __shfl(fq, j, 64), bj = __shfl(bw, j, 64);
        const int cj = __shfl((int)cand, j, 64), rj = __shfl(rank, j, 64);
        if (cj && rj == lane) { of = fj; ob = bj; }
    }
    if (lane < NFM) { o_fm[2 * lane] = of; o_fm[2 * lane + 1] = ob; }
    if (lane == 0) p.count[fi] = total < NFM ? total : NFM;
}

// ---------------------------------------------------------------------------
// Perturbation (ev_perturbation): per frame the pitch marks around the frame's centre by peak picking at the frame's YIN lag, jitter, shimmer and RAP
// from the refined marks, and the harmonic strength as the normalised cross-correlation at that lag (the definition: include/emojivoice.h).  All
// float64 on widened fp32 samples, contraction OFF (STOI_EXACT), no atomics, no scratch, no LDS, no barrier: ONE WAVE PER FRAME, four frames to a
// workgroup of 256 threads; samples are read straight from the row.
//   search    lane l looks at the range's elements l, l + 64, ... in ascending order and keeps its first maximum; a 6-step xor reduction on (value,
//             offset) prefers the higher value, then the lower offset: every lane ends with the range's lowest-index maximum.  The forward and the
//             backward chain advance in the same loop, one search each per step.
//   marks     lane s holds the mark of slot s = n_cycles + k, its refined time and amplitude; periods, pairs and triples come by one shuffle from
//             the neighbours; every sum is one chain over the slots in ascending order by wave broadcasts (absent and uncounted terms are +0.0,
//             which changes no bit of a sum of non-negative terms).
//   r         lane l adds the terms j = l, l + 64, ... < W of E0 and of C and E1 at the three lags in ascending j, one fma per term (the products
//             of widened fp32 samples are exact), then an xor tree over the 64 lanes (offsets 32 .. 1).
// Orders are fixed and depend on the frame's own samples and the arguments only.
struct PerturbParams {
    const float* x; const int32_t* len; const int32_t* lag; double* frame; int32_t* count; int32_t* marks;
    int L, NF, H, nc, W;
    double pf, af, floor2;                                              // floor2 = power_floor^2
};

__device__ __forceinline__ float perturb_sample(const float* xr, int n, long long i) { return i >= 0 && i < n ? xr[i] : 0.0f; }

// the lowest index of the maximum of x over [a, a + cnt), cnt >= 1; +0 outside [0, n)
__device__ __forceinline__ long long perturb_argmax(const float* xr, int n, long long a, int cnt, int lane) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int o = lane; o < cnt; o += 64) {
        const float v = perturb_sample(xr, n, a + o);
        if (v > bv) { bv = v; bi = o; }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const float ov = __shfl_xor(bv, s, 64);
        const int oi = __shfl_xor(bi, s, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    return a + bi;
}

__device__ __forceinline__ bool perturb_accepted(const float* xr, int n, long long m) {
    const float v = perturb_sample(xr, n, m);
    return v > 0.0f && v > perturb_sample(xr, n, m - 1) && v >= perturb_sample(xr, n, m + 1);
}

// the vertex of the parabola through (-1, a), (0, b), (1, c): its offset into *shift, its value returned
__device__ __forceinline__ double perturb_vertex(double a, double b, double c, double* shift) {
    STOI_EXACT
    const double den = (a - 2.0 * b) + c;
    double s = 0.0;
    if (den < 0.0) {
        s = 0.5 * (a - c) / den;
        if (!(fabs(s) <= 1.0)) s = 0.0;
    }
    *shift = s;
    return b - 0.25 * (a - c) * s;
}

__global__ __launch_bounds__(256) void perturbation_kernel(const PerturbParams p) {
    STOI_EXACT
    const int b = blockIdx.y, lane = threadIdx.x & 63, fr = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (fr >= p.NF) return;                                             // (wave-uniform; the kernel has no barrier)
    int n;
    const int nf = voiceq_frames(p.len, b, p.L, p.H, &n);
    const size_t fi = (size_t)b * p.NF + fr;
    const int nc = p.nc, NM = 2 * nc + 1;
    double* o_fr = p.frame + fi * 8;
    int32_t* o_ct = p.count + fi * 4;
    int32_t* o_mk = p.marks ? p.marks + fi * NM : nullptr;
    const int tau0 = fr < nf ? p.lag[fi] : 0;
    if (tau0 < 16 || tau0 > 2048) {                                     // UNVOICED, or past the row's own frames (uniform)
        if (lane < 8) o_fr[lane] = 0.0;
        if (lane < 4) o_ct[lane] = 0;
        if (o_mk && lane < NM) o_mk[lane] = -1;
        return;
    }
    const float* xr = p.x + (size_t)b * p.L;
    const long long c = (long long)fr * p.H + p.H / 2;
    // ---- the marks: lane s keeps the mark of slot s
    int mine = -1;
    {
        const int q = tau0 / 8, lo = tau0 - q, hi = tau0 + q;
        const long long m0 = perturb_argmax(xr, n, c - tau0 / 2, tau0, lane);
        if (perturb_accepted(xr, n, m0)) {
            if (lane == nc) mine = (int)m0;
            long long mf = m0, mb = m0;
            bool fa = true, ba = true;
            for (int k = 1; k <= nc && (fa || ba); ++k) {
                if (fa) {
                    mf = perturb_argmax(xr, n, mf + lo, 2 * q + 1, lane);
                    fa = perturb_accepted(xr, n, mf);
                    if (fa && lane == nc + k) mine = (int)mf;
                }
                if (ba) {
                    mb = perturb_argmax(xr, n, mb - hi, 2 * q + 1, lane);
                    ba = perturb_accepted(xr, n, mb);
                    if (ba && lane == nc - k) mine = (int)mb;
                }
            }
        }
    }
    // ---- refined times and amplitudes, periods, pairs and triples
    const bool has = mine >= 0;
    double t = 0.0, A = 0.0;
    if (has) {
        double shift;
        A = perturb_vertex((double)perturb_sample(xr, n, (long long)mine - 1), (double)xr[mine], (double)perturb_sample(xr, n, (long long)mine + 1), &shift);
        t = (double)mine + shift;
    }
    // (every shuffle is executed by the whole wave: none sits behind a lane's own condition)
    const int has_n = __shfl_down((int)has, 1, 64);
    const bool hasT = has && has_n && lane < 63;                        // slots s and s + 1 both hold a mark: period s
    const double An = __shfl_down(A, 1, 64), tn = __shfl_down(t, 1, 64);
    const double T = hasT ? tn - t : 0.0;
    const double Tn = __shfl_down(T, 1, 64), Tp = __shfl_up(T, 1, 64);
    const int hasT_n = __shfl_down((int)hasT, 1, 64);
    const bool pp = hasT && hasT_n && fmax(T, Tn) <= p.pf * fmin(T, Tn);
    const bool ap = hasT && fmax(A, An) <= p.af * fmin(A, An);
    const int pp_p = __shfl_up((int)pp, 1, 64);
    const bool tr = pp && pp_p && lane > 0;                             // the triple centred on period s
    const double dT = pp ? fabs(T - Tn) : 0.0;
    const double dA = ap ? fabs(A - An) : 0.0;
    double dB = 0.0;
    if (ap) dB = fabs(20.0 * log10(An / A));
    const double dR = tr ? fabs(T - ((Tp + T) + Tn) / 3.0) : 0.0;
    const int N = __popcll(__ballot(has)), nT = __popcll(__ballot(hasT)), npp = __popcll(__ballot(pp)), nap = __popcll(__ballot(ap)),
              ntr = __popcll(__ballot(tr));
    double sT = 0.0, sA = 0.0, sdT = 0.0, sdA = 0.0, sdB = 0.0, sdR = 0.0;
    for (int s = 0; s < NM; ++s) {
        sT = sT + __shfl(T, s, 64);
        sA = sA + __shfl(A, s, 64);
        sdT = sdT + __shfl(dT, s, 64);
        sdA = sdA + __shfl(dA, s, 64);
        sdB = sdB + __shfl(dB, s, 64);
        sdR = sdR + __shfl(dR, s, 64);
    }
    const double Tmean = nT ? sT / (double)nT : 0.0, Amean = N ? sA / (double)N : 0.0;
    const double jit_abs = npp ? sdT / (double)npp : 0.0;
    const double jit = npp ? jit_abs / Tmean : 0.0;
    const double shim = nap ? sdA / (double)nap / Amean : 0.0;
    const double shim_db = nap ? sdB / (double)nap : 0.0;
    const double rap = ntr ? sdR / (double)ntr / Tmean : 0.0;
    // ---- the harmonic strength
    double hr;
    {
        const int W = p.W;
        const long long s0 = c - (W + tau0) / 2;
        double e0 = 0.0, c0 = 0.0, c1 = 0.0, c2 = 0.0, e10 = 0.0, e11 = 0.0, e12 = 0.0;
        for (int j = lane; j < W; j += 64) {
            const long long i = s0 + j;
            const double u = (double)perturb_sample(xr, n, i);
            const double v0 = (double)perturb_sample(xr, n, i + tau0 - 1), v1 = (double)perturb_sample(xr, n, i + tau0),
                         v2 = (double)perturb_sample(xr, n, i + tau0 + 1);
            e0 = fma(u, u, e0);
            c0 = fma(u, v0, c0); c1 = fma(u, v1, c1); c2 = fma(u, v2, c2);
            e10 = fma(v0, v0, e10); e11 = fma(v1, v1, e11); e12 = fma(v2, v2, e12);
        }
        e0 = formant_wave_sum(e0);
        c0 = formant_wave_sum(c0); c1 = formant_wave_sum(c1); c2 = formant_wave_sum(c2);
        e10 = formant_wave_sum(e10); e11 = formant_wave_sum(e11); e12 = formant_wave_sum(e12);
        const double p0 = e0 * e10, p1 = e0 * e11, p2 = e0 * e12;
        const double r0 = p0 > p.floor2 ? c0 / sqrt(p0) : 0.0, r1 = p1 > p.floor2 ? c1 / sqrt(p1) : 0.0, r2 = p2 > p.floor2 ? c2 / sqrt(p2) : 0.0;
        double shift;
        hr = perturb_vertex(r0, r1, r2, &shift);
    }
    if (lane == 0) {
        o_fr[0] = jit; o_fr[1] = jit_abs; o_fr[2] = shim; o_fr[3] = shim_db; o_fr[4] = hr; o_fr[5] = Tmean; o_fr[6] = Amean; o_fr[7] = rap;
        o_ct[0] = nT; o_ct[1] = npp; o_ct[2] = nap; o_ct[3] = ntr;
    }
    if (o_mk && lane < NM) o_mk[lane] = mine;
}

// ---------------------------------------------------------------------------
// Harmonic differences (ev_harmonics): per frame the levels of the harmonics of the frame's YIN period in ONE float64 log-power spectrum, and from
// them H1-H2, H1-A3 and the level of the harmonic nearest F1, F2, F3 over H1 (eGeMAPS; Hanson 1997; the definition: include/emojivoice.h).  All
// float64, contraction OFF (STOI_EXACT), no atomics, no scratch.  One workgroup of 4 waves per (row b, tile of 16 frames f0 .. f0 + 15), on the shared
// pieces of the float64 DFT GEMM above.  Dynamic LDS: Ld, the tile's log-spectrum (16 frames x S doubles, S = 2 mod 32 as in voice_quality_kernel);
// Ht, the tile's harmonics (16 frames x n_harm x {f_h, A_h}); the live-bin counts (4 waves x 16 frames); then the tile's raw span, samples
// f0 H + H / 2 - W / 2 + t for 0 <= t < 15 H + W, staged under the skew with ZEROS outside [0, len) (no reflection).
// PHASE 1 is voice_quality_kernel's first loop: per bin tile W / 4 steps of two MFMAs (cos, sin), the basis of the next four steps requested ahead.
// Epilogue per (frame, bin): raw = fma(sm, sm, re re), p = max(raw, floor), Ldb = (10 / ln 10) log(p) to Ld[frame S + bin]; the bins with raw > floor
// are counted per frame (integers: over the 16 column lanes by an xor tree, over the waves in phase 2).
// PHASE 2, after one barrier: thread t serves frame t >> 4, and lane j = t & 15 of that frame the harmonics j + 1, j + 17, ...: the range lo .. hi of
// harmonic h is scanned in ascending k (strictly greater replaces: the lowest k of a tie), the vertex formed and {f_h, A_h} stored to Ht; harmonics
// that are not measured, and every harmonic of an unvoiced, silent or unresolved frame, are stored as zeros.  A search is one lane's own loop: no
// cross-lane step, so every order depends on the frame alone.  lo >= 1 and hi <= NB - 2 hold by the limits (v >= min_spacing >= 2, search <= 0.5), so
// k* - 1 and k* + 1 are bins of the frame; lo is clamped at 1 all the same.
// BANKS of the scan: the 16 lanes of a frame read different bins of one row, the four frames of a wave rows S apart; the scans are short (2 r + 1
// bins, r = max(1, search v)) and not conflict-free, which phase 1 (W / 4 x 2 MFMAs per bin tile) hides.
// PHASE 3, after a second barrier: thread f < 16 forms the frame's eight figures and the flags (the A3 maximum: one ascending loop over at most
// n_harm terms); all threads copy Ht to d_harm.  Frames >= nf are zeros.
struct HarmTables { const double2* basis; int W, H, nfft, NB, skew, S, n_harm; double bin_hz, sr, search, min_spacing, a3_range; };
struct HarmParams {
    const float* x; const int32_t* len; const float* period; const double* formant; const int32_t* fcount; double* frame; int32_t* count; double* harm;
    HarmTables t; int L, NF, nform; double floor;
};

// harmonic h of spacing v is measured: floor(h v + r) <= NB - 2 (compared in float64: h v has no bound)
__device__ __forceinline__ bool harm_measured(int h, double v, double r, int NB, double* c_out) {
    STOI_EXACT
    const double c = (double)h * v;
    *c_out = c;
    return floor(c + r) <= (double)(NB - 2);
}

// the class of frame f of the tile: true when it is voiced (T > 0), not silent and resolved; v is 0 for an unvoiced or silent frame
__device__ __forceinline__ bool harm_class(const HarmParams& p, const int* live_w, int b, int f0, int f, int nf, double* T_out, double* v_out, double* r_out) {
    STOI_EXACT
    double T = 0.0, v = 0.0, r = 0.0;
    bool comb = false;
    if (f0 + f < nf) {
        T = (double)p.period[(size_t)b * p.NF + f0 + f];
        if (T > 0.0 && live_w[f] + live_w[16 + f] + live_w[32 + f] + live_w[48 + f] > 0) {
            v = (double)p.t.nfft / T;
            comb = !(v < p.t.min_spacing);
            r = fmax(1.0, p.t.search * v);
        }
    }
    *T_out = T; *v_out = v; *r_out = r;
    return comb;
}

__global__ __launch_bounds__(256) void harmonics_kernel(const HarmParams p) {
    STOI_EXACT
    extern __shared__ __attribute__((aligned(16))) double harm_smem[];
    const int b = blockIdx.y, f0 = blockIdx.x * 16, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int W = p.t.W, H = p.t.H, NB = p.t.NB, skew = p.t.skew, S = p.t.S, NH = p.t.n_harm;
    int n;
    const int nf = voiceq_frames(p.len, b, p.L, H, &n);
    double* out = p.frame + ((size_t)b * p.NF + f0) * 8;
    int32_t* oc = p.count + ((size_t)b * p.NF + f0) * 2;
    double* oh = p.harm ? p.harm + ((size_t)b * p.NF + f0) * NH * 2 : nullptr;
    const int nfr = p.NF - f0 < 16 ? p.NF - f0 : 16;                    // the tile's frames inside the outputs (>= 1)
    if (f0 >= nf) {                                                     // (uniform) zeros past the row's own frames
        if (tid < 8 * nfr) out[tid] = 0.0;
        if (tid < 2 * nfr) oc[tid] = 0;
        if (oh) for (int i = tid; i < nfr * NH * 2; i += 256) oh[i] = 0.0;
        return;
    }
    double* Ld = harm_smem;                                             // (16, S)
    double* Ht = Ld + 16 * S;                                           // (16, n_harm, 2)
    int* live_w = (int*)(Ht + 16 * NH * 2);                             // (4, 16)
    float* sx = (float*)(live_w + 64);
    const int span = 15 * H + W;
    {
        const float* xr = p.x + (size_t)b * p.L;
        const long long i0 = (long long)f0 * H + H / 2 - W / 2;
        for (int t = tid; t < span; t += 256) {
            const long long i = i0 + t;
            sx[dft_word(t, H, skew)] = i >= 0 && i < n ? xr[i] : 0.f;
        }
    }
    __syncthreads();
    {
        const int r = lane & 15, q = lane >> 4;
        const int ntile = (NB + 15) >> 4, nsteps = W >> 2;
        DftSkewWalk walk(r, H, skew);
        int live[4] = {0, 0, 0, 0};
        for (int bt = wv; bt < ntile; bt += 4) {
            const int col = bt * 16 + r, colc = col < NB ? col : NB - 1;
            const double2* bp = p.t.basis + (size_t)q * NB + colc;
            stftd_acc xc = {0.0, 0.0, 0.0, 0.0}, xs = xc;
            walk.start(q);
            double2 cur[4], nxt[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) cur[u] = bp[(size_t)(u < nsteps ? u : nsteps - 1) * 4 * NB];
            for (int t0 = 0; t0 < nsteps; t0 += 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) nxt[u] = bp[(size_t)(t0 + 4 + u < nsteps ? t0 + 4 + u : nsteps - 1) * 4 * NB];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (t0 + u < nsteps) {                              // (uniform)
                        const double ax = (double)sx[walk.word()];
                        xc = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, cur[u].x, xc, 0, 0, 0);
                        xs = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, cur[u].y, xs, 0, 0, 0);
                        walk.step();
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
            }
            if (col < NB) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double raw = fma(xs[i], xs[i], xc[i] * xc[i]);
                    Ld[(q + 4 * i) * S + col] = VOICEQ_DB * log(fmax(raw, p.floor));
                    live[i] += raw > p.floor ? 1 : 0;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) live[i] += __shfl_xor(live[i], o, 64);
            if (r == 0) live_w[wv * 16 + q + 4 * i] = live[i];
        }
    }
    __syncthreads();                                                    // Ld and the live counts are complete
    const int fr = tid >> 4, j = tid & 15;
    {
        double T, v, rr;
        const bool comb = harm_class(p, live_w, b, f0, fr, nf, &T, &v, &rr);
        const double* Lf = Ld + fr * S;
        double* Hf = Ht + fr * NH * 2;
        for (int h = j + 1; h <= NH; h += 16) {
            double fh = 0.0, Ah = 0.0, c;
            if (comb && harm_measured(h, v, rr, NB, &c)) {
                int lo = (int)ceil(c - rr);
                const int hi = (int)floor(c + rr);                      // (<= NB - 2)
                if (lo < 1) lo = 1;                                     // (never, by the limits)
                int ks = lo;
                double best = Lf[lo];
                for (int k = lo + 1; k <= hi; ++k) {
                    const double l = Lf[k];
                    if (l > best) { best = l; ks = k; }
                }
                double shift;
                Ah = perturb_vertex(Lf[ks - 1], best, Lf[ks + 1], &shift);
                fh = ((double)ks + shift) * p.t.bin_hz;
            }
            Hf[2 * (h - 1)] = fh; Hf[2 * (h - 1) + 1] = Ah;
        }
    }
    __syncthreads();                                                    // Ht is complete
    if (oh) for (int i = tid; i < nfr * NH * 2; i += 256) oh[i] = Ht[i];
    if (tid < nfr) {
        const int f = tid;
        double T, vv, r2;
        const bool cmb = harm_class(p, live_w, b, f0, f, nf, &T, &vv, &r2);
        double o[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, vv};
        int nh = 0, flags = 0;
        if (cmb) {
            const double* Hf = Ht + f * NH * 2;
            double c;
            while (nh < NH && harm_measured(nh + 1, vv, r2, NB, &c)) ++nh;
            if (nh >= 1) { o[5] = Hf[1]; o[6] = Hf[0]; }
            if (nh >= 2) { o[0] = Hf[1] - Hf[3]; flags |= 1; }
            if (p.formant && nh >= 1) {
                const double u = p.t.sr / T;
                const size_t bf = (size_t)b * p.NF + f0 + f;
                const int fc = p.fcount[bf];
                const double* Fp = p.formant + bf * p.nform * 2;
                const int ni = p.nform < 3 ? p.nform : 3;
#pragma unroll
                for (int i = 1; i <= 3; ++i) {
                    if (i > ni || i > fc) continue;
                    const double F = Fp[2 * (i - 1)];
                    if (!(F > 0.0)) continue;
                    const double g = F / u;
                    const double hd = floor(g + 0.5);
                    if (hd >= 1.0 && hd <= (double)nh) {
                        o[1 + i] = Hf[2 * ((int)hd - 1) + 1] - Hf[1];
                        flags |= 1 << i;
                    }
                    if (i == 3) {
                        const double w = fmax(0.5, p.t.a3_range * g);
                        const double lod = fmax(1.0, ceil(g - w)), hid = fmin((double)nh, floor(g + w));
                        if (lod <= hid) {                               // (1 <= lod <= hid <= nh <= 64)
                            const int l3 = (int)lod, h3 = (int)hid;
                            double a3 = Hf[2 * (l3 - 1) + 1];
                            for (int h = l3 + 1; h <= h3; ++h) { const double a = Hf[2 * (h - 1) + 1]; if (a > a3) a3 = a; }
                            o[1] = Hf[1] - a3;
                            flags |= 16;
                        }
                    }
                }
            }
        }
        double* of = out + 8 * f;
#pragma unroll
        for (int i = 0; i < 8; ++i) of[i] = o[i];
        oc[2 * f] = nh; oc[2 * f + 1] = flags;
    }
}

// ---------------------------------------------------------------------------
// Contour functionals (ev_functionals): per contour (b, k) of F frames the eGeMAPS functionals: moments, order statistics, the slopes of the rising
// and of the falling parts, peaks, and the lengths of the runs of valid frames and of the gaps between them (the definition: include/emojivoice.h).
// All float64, contraction OFF (STOI_EXACT), no atomics, no scratch.  ONE WORKGROUP of 256 threads PER CONTOUR, everything in dynamic LDS: 64 doubles
// and 64 words of hand-over, then u (P doubles), g and st (P uint16 each), P = F rounded up to a power of two and at least 256: 512 + 12 P bytes,
// 48.5 KiB at F = 4096.  Element i of the compacted contour belongs to thread i mod 256 in every phase, which is the slot rule of the sums.
//   PHASE 1  tiles of 256 frames in ascending order, one coalesced read each: the validity flag, a ballot per wave, the four waves' counts through
//            LDS (two alternating sets: one barrier per tile) and the running total give each valid frame its place in u / g.
//   PHASE 2  tiles of 256 elements of u: the classes of the pairs i - 1, i, i + 1 from the neighbours, then two inclusive max-scans of "a run starts
//            here" / "a part starts here" markers (6 shuffle steps, the waves' last values through LDS, a running carry): they carry the start of
//            the run / part to every element, so a part may cross every wave and tile.  The thread of a part's LAST pair forms its slope and keeps
//            the start in st[i] (0xffff elsewhere); the thread of a run's last element squares its length; gaps come from g's differences.
//   PHASE 3  the sums: slot accumulators in registers (ascending i), an xor tree per wave, the four waves added in ascending order by every thread;
//            then the second pass (squared deviations from the means; the slopes are formed again from st, by the same operations).
//   PHASE 4  u[k ..] = +inf up to the next power of two and a bitonic network in place, one barrier per stage.
//   PHASE 5  thread r forms percentile r; thread 0 writes the rest.
struct FuncParams {
    const double* v; const uint8_t* mask; const int32_t* len; double* stat; int32_t* count;
    int K, F, NQ, P;                                                    // P: F rounded up to a power of two, at least 256
    double q[16];
};

__device__ __forceinline__ int func_wave_isum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ int func_class(double a, double b) { return (b > a) - (b < a); }     // of the adjacent pair (a, b)

__global__ __launch_bounds__(256) void functionals_kernel(const FuncParams p) {
    STOI_EXACT
    extern __shared__ __attribute__((aligned(16))) double func_smem[];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, b = blockIdx.y;
    const int F = p.F, NQ = p.NQ, NS = 12 + NQ;
    double* rd = func_smem;                                             // [2][4][3]: the waves' sums of pass 1 and of pass 2
    int* ri = (int*)(func_smem + 32);                                   // [4][9]: the waves' counts
    int* wc = ri + 36;                                                  // [2][4]: phase 1, the waves' valid frames of a tile
    int* wm = ri + 44;                                                  // [2][4][2]: phase 2, the waves' last scan values of a tile
    double* u = func_smem + 64;
    unsigned short* g = (unsigned short*)(u + p.P);
    unsigned short* st = g + p.P;
    const size_t row = (size_t)b * p.K + blockIdx.x;
    double* o_st = p.stat + row * NS;
    int32_t* o_ct = p.count + row * 8;
    const int n = p.len ? p.len[b] : F;
    if (n < 0 || n > F) {                                               // a bad row is a row of zeros (uniform; before any barrier)
        if (t < NS) o_st[t] = 0.0;
        if (t < 8) o_ct[t] = 0;
        return;
    }
    // ---- phase 1: validity and ordered compaction
    const double* vr = p.v + row * F;
    const uint8_t* mk = p.mask ? p.mask + row * F : nullptr;
    int k = 0, dropped = 0;
    for (int f0 = 0; f0 < n; f0 += 256) {
        const int f = f0 + t;
        const bool on = f < n && (!mk || mk[f] != 0);
        const double x = on ? vr[f] : 0.0;
        const bool valid = on && fabs(x) <= 1.7976931348623157e308;     // finite (NaN compares false)
        dropped += on && !valid;
        const unsigned long long bal = __ballot(valid);
        const int slot = (f0 >> 8 & 1) * 4;
        if (lane == 0) wc[slot + w] = __popcll(bal);
        __syncthreads();
        const int c0 = wc[slot], c1 = wc[slot + 1], c2 = wc[slot + 2], c3 = wc[slot + 3];
        if (valid) {
            const int at = k + (w > 0 ? c0 : 0) + (w > 1 ? c1 : 0) + (w > 2 ? c2 : 0) + __popcll(bal & ((1ull << lane) - 1ull));
            u[at] = x; g[at] = (unsigned short)f;
        }
        k += c0 + c1 + c2 + c3;
    }
    __syncthreads();
    // ---- phases 2 and 3, first pass
    double su = 0.0, sr = 0.0, sf = 0.0;
    int nrise = 0, nfall = 0, npeak = 0, nruns = 0, ngaps = 0, nadj = 0, s2r = 0, s2g = 0;
    int car_r = -1, car_p = -1;
    for (int i0 = 0; i0 < k; i0 += 256) {
        const int i = i0 + t;
        const bool in = i < k;
        double ui = 0.0, un = 0.0, up = 0.0;
        int gi = 0, gn = 0, cP = 0, cI = 0, cN = 0;
        bool adjP = false, adjN = false;
        if (in) {
            ui = u[i]; gi = g[i];
            if (i > 0) { up = u[i - 1]; adjP = (int)g[i - 1] + 1 == gi; }
            if (i + 1 < k) { un = u[i + 1]; gn = g[i + 1]; adjN = gn == gi + 1; }
            if (adjP) cP = func_class(up, ui);
            if (adjN) cI = func_class(ui, un);
            if (i + 2 < k && (int)g[i + 2] == gn + 1) cN = func_class(un, u[i + 2]);
        }
        int mr = in && !adjP ? i : -1;                                  // a run starts at i
        int mp = in && cI != 0 && cP != cI ? i : -1;                    // a part starts with pair i
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {                              // (every shuffle is executed by the whole wave)
            const int a = __shfl_up(mr, o, 64), c = __shfl_up(mp, o, 64);
            if (lane >= o) { mr = max(mr, a); mp = max(mp, c); }
        }
        const int slot = (i0 >> 8 & 1) * 8;
        if (lane == 63) { wm[slot + 2 * w] = mr; wm[slot + 2 * w + 1] = mp; }
        __syncthreads();
        mr = max(mr, car_r); mp = max(mp, car_p);
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int a = wm[slot + 2 * x], c = wm[slot + 2 * x + 1];
            if (x < w) { mr = max(mr, a); mp = max(mp, c); }
            car_r = max(car_r, a); car_p = max(car_p, c);
        }
        if (in) {
            su = su + ui;
            nadj += adjN;
            npeak += adjP && adjN && ui > up && ui >= un;
            if (!adjN) { const int l = i - mr + 1; ++nruns; s2r += l * l; }
            if (i == 0 && gi > 0) { ++ngaps; s2g += gi * gi; }
            const int d = i + 1 < k ? gn - gi - 1 : n - 1 - gi;         // the gap behind i, the trailing one behind the last
            if (d > 0) { ++ngaps; s2g += d * d; }
            int code = 0xffff;
            if (cI != 0 && cN != cI) {                                  // pair i is the last of its part, which began with pair mp
                code = mp;
                const double s = (un - u[mp]) / (double)(i + 1 - mp);
                if (cI > 0) { sr = sr + s; ++nrise; } else { sf = sf + s; ++nfall; }
            }
            st[i] = (unsigned short)code;                               // (read back by this thread only)
        }
    }
    su = formant_wave_sum(su); sr = formant_wave_sum(sr); sf = formant_wave_sum(sf);
    dropped = func_wave_isum(dropped); nrise = func_wave_isum(nrise); nfall = func_wave_isum(nfall); npeak = func_wave_isum(npeak);
    nruns = func_wave_isum(nruns); ngaps = func_wave_isum(ngaps); nadj = func_wave_isum(nadj); s2r = func_wave_isum(s2r); s2g = func_wave_isum(s2g);
    if (lane == 0) {
        rd[3 * w] = su; rd[3 * w + 1] = sr; rd[3 * w + 2] = sf;
        int* r = ri + 9 * w;
        r[0] = dropped; r[1] = nrise; r[2] = nfall; r[3] = npeak; r[4] = nruns; r[5] = ngaps; r[6] = nadj; r[7] = s2r; r[8] = s2g;
    }
    __syncthreads();
    su = ((rd[0] + rd[3]) + rd[6]) + rd[9]; sr = ((rd[1] + rd[4]) + rd[7]) + rd[10]; sf = ((rd[2] + rd[5]) + rd[8]) + rd[11];
    dropped = ri[0] + ri[9] + ri[18] + ri[27]; nrise = ri[1] + ri[10] + ri[19] + ri[28]; nfall = ri[2] + ri[11] + ri[20] + ri[29];
    npeak = ri[3] + ri[12] + ri[21] + ri[30]; nruns = ri[4] + ri[13] + ri[22] + ri[31]; ngaps = ri[5] + ri[14] + ri[23] + ri[32];
    nadj = ri[6] + ri[15] + ri[24] + ri[33]; s2r = ri[7] + ri[16] + ri[25] + ri[34]; s2g = ri[8] + ri[17] + ri[26] + ri[35];
    const double mean = k ? su / (double)k : 0.0, rmean = nrise ? sr / (double)nrise : 0.0, fmean = nfall ? sf / (double)nfall : 0.0;
    // ---- second pass: squared deviations
    double q2 = 0.0, r2 = 0.0, f2 = 0.0;
    for (int i = t; i < k; i += 256) {
        const double d = u[i] - mean;
        q2 = q2 + d * d;
        const int a = st[i];
        if (a != 0xffff) {
            const double ue = u[i + 1], ua = u[a];
            const double s = (ue - ua) / (double)(i + 1 - a);
            if (ue > ua) { const double e = s - rmean; r2 = r2 + e * e; }
            else { const double e = s - fmean; f2 = f2 + e * e; }
        }
    }
    q2 = formant_wave_sum(q2); r2 = formant_wave_sum(r2); f2 = formant_wave_sum(f2);
    if (lane == 0) { rd[12 + 3 * w] = q2; rd[13 + 3 * w] = r2; rd[14 + 3 * w] = f2; }
    __syncthreads();                                                    // (also: every read of u in compacted order lies before it)
    q2 = ((rd[12] + rd[15]) + rd[18]) + rd[21]; r2 = ((rd[13] + rd[16]) + rd[19]) + rd[22]; f2 = ((rd[14] + rd[17]) + rd[20]) + rd[23];
    // ---- phase 4: the bitonic network over PS >= max(k, 2) elements, ascending by <
    int PS = 2;
    while (PS < k) PS <<= 1;
    for (int i = k + t; i < PS; i += 256) u[i] = INFINITY;
    __syncthreads();
    for (int size = 2; size <= PS; size <<= 1) {
        for (int j = size >> 1; j > 0; j >>= 1) {
            for (int pi = t; pi < PS >> 1; pi += 256) {
                const int lo = (pi & ~(j - 1)) << 1 | (pi & (j - 1)), hi = lo | j;
                const double a = u[lo], c = u[hi];
                if ((lo & size) == 0 ? c < a : a < c) { u[lo] = c; u[hi] = a; }
            }
            __syncthreads();
        }
    }
    // ---- phase 5
    if (k > 0 && t < NQ) {
        double qq = 0.0;
#pragma unroll
        for (int r = 0; r < 16; ++r) if (t == r) qq = p.q[r];            // (static indices: the arguments stay in scalar registers)
        const double pp = qq * (double)(k - 1);
        const double jf = floor(pp);
        const int j = (int)jf, j1 = min(j + 1, k - 1);
        const double tt = pp - jf, sj = u[j];
        o_st[12 + t] = sj + tt * (u[j1] - sj);
    }
    if (k == 0 && t < NQ) o_st[12 + t] = 0.0;
    if (t == 0) {
        if (k == 0 && n > 0) { ngaps = 1; s2g = n * n; }
        const long long nr = nruns, ng = ngaps, s1r = k, s1g = n - k;
        o_st[0] = mean;
        o_st[1] = k ? sqrt(q2 / (double)k) : 0.0;
        o_st[2] = k ? u[0] : 0.0;
        o_st[3] = k ? u[k - 1] : 0.0;
        o_st[4] = rmean;
        o_st[5] = nrise ? sqrt(r2 / (double)nrise) : 0.0;
        o_st[6] = fmean;
        o_st[7] = nfall ? sqrt(f2 / (double)nfall) : 0.0;
        o_st[8] = nr ? (double)s1r / (double)nr : 0.0;
        o_st[9] = nr ? sqrt((double)(nr * s2r - s1r * s1r)) / (double)nr : 0.0;
        o_st[10] = ng ? (double)s1g / (double)ng : 0.0;
        o_st[11] = ng ? sqrt((double)(ng * s2g - s1g * s1g)) / (double)ng : 0.0;
        o_ct[0] = k; o_ct[1] = dropped; o_ct[2] = nrise; o_ct[3] = nfall; o_ct[4] = npeak; o_ct[5] = nruns; o_ct[6] = ngaps; o_ct[7] = nadj;
    }
}

// ---------------------------------------------------------------------------
// Modulation spectra of contours (ev_modulation): per contour (b, k) of F frames the power of its oscillations on a grid of NM modulation
// frequencies, pooled over the runs of valid frames that are long enough, and the strongest local peak of up to four bands (the definition:
// include/emojivoice.h).  All float64, contraction OFF (STOI_EXACT), no atomics, no scratch.  ONE WORKGROUP of 256 threads PER CONTOUR,
// everything in dynamic LDS: wr (F doubles: the value, NaN where the frame is not valid, then w_t r_t in place), sw (MR doubles, a run's window
// sum), the pooled spectrum (128 doubles), the runs as start | length << 16 (MR words), the pooled weights (128 words) and 24 words of hand-over,
// MR = (F + 1) / 4 rounded up to even being the most runs of at least 3 frames that F frames hold: 45.6 KiB at F = 4096.
//   PHASE A  (1) one coalesced read: wr[f] = the value or NaN, the counts of valid and dropped frames.  (2) tiles of 256 frames: functionals_kernel's
//            inclusive max-scan of "a run starts here" carries the start to the run's last frame, whose thread knows the length; the runs of at
//            least min_run frames are appended to the table in ascending order through a ballot per wave and the waves' counts.  (3) WAVE 0 alone
//            takes the runs in ascending order, frame t of a run in lane t mod 64: the mean and the slope, then r_t, the window, wr = w_t r_t in
//            place and the sums of w and of r^2 (an xor tree each); it also pools the two statistics.  Phase B dwarfs this: three waves idle here.
//   PHASE B  thread (j, c) = (unit >> 2, unit & 3) of 4 NM units, 256 a pass: over the runs in ascending order the chain c of xr and xi (frames
//            t = c mod 4 ascending, a rounded product and a rounded sum each), the four chains of a j joined through shuffles inside their
//            quad of lanes, P, and the pooled sum.  A wave reads FOUR addresses of wr per step (16 j x 4 chains: four adjacent doubles, distinct
//            banks, each a broadcast to 16 lanes), so LDS traffic is one ds_read_b64 per two library calls; the float64 cospi / sinpi bound the
//            kernel.
//   PHASE C  wave x < NBAND takes band x: lane l scans j = j_lo + l, + 64 for candidates, a wave-wide (power, lowest j) maximum, lane 0 adds the
//            band's mean in ascending j and forms the parabola.  Thread 0 writes the statistics and the counts.
struct ModParams {
    const double* v; const uint8_t* mask; const int32_t* len; double* spec; int32_t* weight; double* peak; double* stat; int32_t* count;
    int K, F, NM, NBAND, min_run, MR;
    double nu0, dnu, min_cycles;
    int band[8];
};

__device__ __forceinline__ bool mod_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }     // (NaN compares false)

__global__ __launch_bounds__(256) void modulation_kernel(const ModParams p) {
    STOI_EXACT
    extern __shared__ __attribute__((aligned(16))) double mod_smem[];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, b = blockIdx.y;
    const int F = p.F, NM = p.NM, NB = p.NBAND;
    double* wr = mod_smem;                                              // [F + (F & 1)]
    double* rsw = wr + F + (F & 1);                                     // [MR]
    double* sp = rsw + p.MR;                                            // [128]
    int* rs = (int*)(sp + 128);                                         // [MR]
    int* wg = rs + p.MR;                                                // [128]
    int* wm = wg + 128;                                                 // [2][4]: the waves' last scan values of a tile
    int* wc = wm + 8;                                                   // [2][4]: the waves' analysed runs of a tile
    int* tot = wc + 8;                                                  // [4][2]: the waves' valid and dropped frames
    const size_t row = (size_t)b * p.K + blockIdx.x;
    double* o_sp = p.spec + row * NM;
    int32_t* o_wg = p.weight + row * NM;
    double* o_pk = p.peak ? p.peak + row * NB * 4 : nullptr;
    double* o_st = p.stat + row * 2;
    int32_t* o_ct = p.count + row * (4 + NB);
    const int n = p.len ? p.len[b] : F;
    if (n < 0 || n > F) {                                               // a bad row is a row of zeros (uniform; before any barrier)
        if (t < NM) { o_sp[t] = 0.0; o_wg[t] = 0; }
        if (t < 4 * NB) o_pk[t] = 0.0;
        if (t < 2) o_st[t] = 0.0;
        if (t < 4 + NB) o_ct[t] = 0;
        return;
    }
    // ---- phase A1: validity
    const double* vr = p.v + row * F;
    const uint8_t* mk = p.mask ? p.mask + row * F : nullptr;
    int nvalid = 0, dropped = 0;
    for (int f = t; f < n; f += 256) {
        const bool on = !mk || mk[f] != 0;
        const double x = on ? vr[f] : 0.0;
        const bool valid = on && mod_finite(x);
        nvalid += valid; dropped += on && !valid;
        wr[f] = valid ? x : __builtin_nan("");
    }
    nvalid = func_wave_isum(nvalid); dropped = func_wave_isum(dropped);
    if (lane == 0) { tot[2 * w] = nvalid; tot[2 * w + 1] = dropped; }
    __syncthreads();
    // ---- phase A2: the runs of at least min_run frames, in ascending order
    int nruns = 0, car = -1;
    for (int f0 = 0; f0 < n; f0 += 256) {
        const int f = f0 + t;
        const bool vi = f < n && mod_finite(wr[f]);
        const bool vp = vi && f > 0 && mod_finite(wr[f - 1]), vn = vi && f + 1 < n && mod_finite(wr[f + 1]);
        int mr = vi && !vp ? f : -1;                                    // a run starts at f
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {                              // (every shuffle is executed by the whole wave)
            const int a = __shfl_up(mr, o, 64);
            if (lane >= o) mr = max(mr, a);
        }
        const int slot = (f0 >> 8 & 1) * 4;
        if (lane == 63) wm[slot + w] = mr;
        __syncthreads();
        mr = max(mr, car);
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int a = wm[slot + x];
            if (x < w) mr = max(mr, a);
            car = max(car, a);
        }
        const int l = vi && !vn ? f - mr + 1 : 0;                       // the thread of a run's last frame (mr >= 0 there) knows its length
        const bool an = l >= p.min_run;
        const unsigned long long bal = __ballot(an);
        if (lane == 0) wc[slot + w] = __popcll(bal);
        __syncthreads();
        const int c0 = wc[slot], c1 = wc[slot + 1], c2 = wc[slot + 2], c3 = wc[slot + 3];
        if (an) {                                                       // (at < MR: runs of >= 3 frames are at least one frame apart)
            const int at = nruns + (w > 0 ? c0 : 0) + (w > 1 ? c1 : 0) + (w > 2 ? c2 : 0) + __popcll(bal & ((1ull << lane) - 1ull));
            rs[at] = mr | l << 16;
        }
        nruns += c0 + c1 + c2 + c3;
    }
    __syncthreads();
    // ---- phase A3: wave 0 detrends and windows every analysed run in place
    double q_sum = 0.0, lb_sum = 0.0;
    int aframes = 0;
    if (w == 0) {
        for (int r = 0; r < nruns; ++r) {
            const int e = rs[r], s = e & 0xffff, l = e >> 16;
            const double hl = (double)(l - 1) / 2.0, dl = (double)l;
            double su = 0.0, sc = 0.0;
            for (int i = lane; i < l; i += 64) {
                const double u = wr[s + i], tc = (double)i - hl;
                su = su + u;
                sc = sc + tc * u;
            }
            su = formant_wave_sum(su); sc = formant_wave_sum(sc);
            const long long li = l;
            const double m = su / dl, bb = sc / ((double)(li * (li * li - 1)) / 12.0);
            double sw = 0.0, s2 = 0.0;
            for (int i = lane; i < l; i += 64) {
                const double tc = (double)i - hl;
                const double rr = (wr[s + i] - m) - bb * tc;
                const double ww = 0.5 - 0.5 * cospi((double)(2 * i + 1) / dl);
                sw = sw + ww;
                s2 = s2 + rr * rr;
                wr[s + i] = ww * rr;
            }
            sw = formant_wave_sum(sw); s2 = formant_wave_sum(s2);
            if (lane == 0) rsw[r] = sw;
            q_sum = q_sum + s2;
            lb_sum = lb_sum + dl * bb;
            aframes += l;
        }
    }
    __syncthreads();
    // ---- phase B: the spectra of the runs and their pooling
    for (int u0 = 0; u0 < 4 * NM; u0 += 256) {                          // (uniform)
        const int j = (u0 + t) >> 2, c = t & 3;
        const bool act = j < NM;
        const double nu = p.nu0 + (double)j * p.dnu;
        double acc = 0.0;
        int W = 0;
        for (int r = 0; r < nruns; ++r) {
            const int e = rs[r], s = e & 0xffff, l = e >> 16;
            const bool res = act && nu * (double)l >= p.min_cycles;
            double ar = 0.0, ai = 0.0;
            if (res) {
                for (int i = c; i < l; i += 4) {
                    const double x = wr[s + i], ph = nu * (double)i;
                    ar = ar + x * cospi(2.0 * ph);
                    ai = ai + x * sinpi(2.0 * ph);
                }
            }
            const int q0 = lane & ~3;                                   // (every shuffle is executed by the whole wave)
            const double xr = ((__shfl(ar, q0, 64) + __shfl(ar, q0 + 1, 64)) + __shfl(ar, q0 + 2, 64)) + __shfl(ar, q0 + 3, 64);
            const double xi = ((__shfl(ai, q0, 64) + __shfl(ai, q0 + 1, 64)) + __shfl(ai, q0 + 2, 64)) + __shfl(ai, q0 + 3, 64);
            if (res) {
                const double sw = rsw[r];
                const double P = 2.0 * (xr * xr + xi * xi) / (sw * sw);
                acc = acc + (double)l * P;
                W += l;
            }
        }
        if (act && c == 0) {
            const double Pm = W ? acc / (double)W : 0.0;
            sp[j] = Pm; wg[j] = W;
            o_sp[j] = Pm; o_wg[j] = W;
        }
    }
    __syncthreads();
    // ---- phase C: the peak of every band
    if (w < NB) {
        int jlo = 0, jhi = 0;
#pragma unroll
        for (int x = 0; x < 4; ++x) if (w == x) { jlo = p.band[2 * x]; jhi = p.band[2 * x + 1]; }     // (static indices: scalar registers)
        double bp = 0.0;
        int bj = -1;
        for (int j = jlo + lane; j < jhi; j += 64) {
            if (j >= 1 && j <= NM - 2) {
                const double Pa = sp[j - 1], Pc = sp[j], Pe = sp[j + 1];
                const bool cand = wg[j - 1] > 0 && wg[j] > 0 && wg[j + 1] > 0 && Pa > 0.0 && Pe > 0.0 && Pc > Pa && Pc >= Pe;
                if (cand && Pc > bp) { bp = Pc; bj = j; }               // (ascending j: the lowest of equal powers stays)
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double op = __shfl_xor(bp, o, 64);
            const int oj = __shfl_xor(bj, o, 64);
            if (oj >= 0 && (bj < 0 || op > bp || (op == bp && oj < bj))) { bp = op; bj = oj; }
        }
        if (lane == 0) {
            double pk[4] = {0.0, 0.0, 0.0, 0.0};
            if (bj >= 0) {
                double bs = 0.0;
                int bn = 0;
                for (int j = jlo; j < jhi; ++j) if (wg[j] > 0) { bs = bs + sp[j]; ++bn; }
                const double bm = bs / (double)bn;                      // (bn >= 1: the peak itself)
                const double a = log(sp[bj - 1]), cc = log(sp[bj]), e = log(sp[bj + 1]);
                const double den = (a - 2.0 * cc) + e;
                const double off = den < 0.0 ? 0.5 * (a - e) / den : 0.0;
                const double pw = exp(cc - 0.25 * (a - e) * off);
                pk[0] = p.nu0 + ((double)bj + off) * p.dnu; pk[1] = sqrt(2.0 * pw); pk[2] = bm; pk[3] = pw / bm;
            }
            double* o = o_pk + 4 * w;
            o[0] = pk[0]; o[1] = pk[1]; o[2] = pk[2]; o[3] = pk[3];
            o_ct[4 + w] = bj;
        }
    }
    if (t == 0) {
        o_st[0] = aframes ? q_sum / (double)aframes : 0.0;
        o_st[1] = aframes ? lb_sum / (double)aframes : 0.0;
        o_ct[0] = tot[0] + tot[2] + tot[4] + tot[6]; o_ct[1] = tot[1] + tot[3] + tot[5] + tot[7]; o_ct[2] = nruns; o_ct[3] = aframes;
    }
}

// ---------------------------------------------------------------------------
// Auditory descriptors (ev_auditory): per frame the loudness of an auditory spectrum, the spectral flux against the frame before, the power and
// the first cepstral coefficients over mel bands (MFCC), from ONE float64 power spectrum (the definition: include/emojivoice.h; Eyben et al. 2016).
// All float64, contraction OFF (STOI_EXACT), no atomics.  Two GEMMs on v_mfma_f64_16x16x4_f64, chained through LDS inside one launch, on the shared
// pieces of the float64 DFT GEMM above; the device sees only tables (mel: (NBp, NMp) zero-padded, NMp = 16 ceil(n_mel / 16); eq (n_mel); dct
// (n_mel, n_ceps)).
// One workgroup of 4 waves per (row b, tile).  The flux of frame f needs the spectrum of frame f - 1, so the 16 matrix rows of a tile are the
// frames f0 - 1 .. f0 + 14 and tiles advance by 15 frames, f0 = 15 blockIdx.x: row 0 is carried for the flux of row 1 only and nothing of it is
// written (1 / 15 more matrix work; no second launch, no arena, no dependence between workgroups).  Dynamic LDS: P, the tile's power spectrum (16
// rows x S doubles, S = 2 mod 32 as in voice_quality_kernel); Lg and Lc (16 rows x LS doubles each, LS = NMp + 1): log(Ef) and pow(eq Ef, compress);
// then the tile's raw span, samples (f0 - 1) H + H / 2 - W / 2 + t for 0 <= t < 15 H + W, staged under the skew with ZEROS outside [0, len).
// 1024 / 256 / 1024 with 26 bands: 65 792 + 2 x 4 224 + 19 600 = 93 840 bytes, and 896 static: 92.5 KiB, one workgroup per CU.
// PHASE 1 is voice_quality_kernel's first loop.  Epilogue per (row, bin): raw = fma(sm, sm, re * re) goes to P[row S + bin]; per row the lane
// accumulates over its bin tiles in ascending order the power (s = s + raw) and the count of bins with raw > floor; then the hand-over (xor tree 8, 4,
// 2, 1 over the 16 column lanes, the waves as ((w0 + w1) + w2) + w3).
// PHASE 2, after one barrier: wave w < NMp / 16 owns the band tile w: NBp / 4 steps of one MFMA, lane l of an A fragment reads P[(l & 15) S + k0 +
// (l >> 4)] with ds_read_b64 (k >= NB: the address clamped to NB - 1, the table row zero), the B fragment is mel[k0 + (l >> 4)][16 w + (l & 15)] from
// L2, the next four steps requested ahead: E[m] is the sum over k ascending in steps of 4.  Its epilogue is PHASE 3: Ef = max(E, floor), Lg = log(Ef),
// Lc = pow(eq[m] Ef, compress), and the store of E to d_bands.
// FLUX, by every wave in the same phase: the 16 lanes j of lane group g = tid >> 4 serve row (g >> 1) + 8 (g & 1) >= 1 over the bins k = j mod 16 of
// [k_lo, k_hi) ascending, d = sqrt(P[row][k]) - sqrt(P[row - 1][k]), s = fma(d, d, s); xor tree 8, 4, 2, 1; flux = sqrt(s / (k_hi - k_lo)).
// PHASE 4, after one barrier: thread (row g, i) forms mfcc[i] = fma(Lg[m], dct[m][i], s) over ascending m; thread (row g, 15) adds the loudness s = s +
// Lc[m] over ascending m and writes the frame's four figures and its flags.  Every order depends on the geometry and the frame only.
// BANKS (from the LDS table of the micro-architecture guide; no counter was read).  Phase 2's ds_read_b64 is voice_quality_kernel's: conflict-free
// at S = 2 mod 32.  Flux: ds_read_b64 is served in groups of 32 lanes and banked over 64 dwords; a group holds the rows r and r + 8, each 16
// consecutive doubles (32 dwords), and 8 S doubles = 32 mod 64 dwords: all 64 banks once, conflict-free (that is what the row order of g is for).
// Phase 3's ds_write_b64 is served 16 contiguous lanes at a time, here 16 consecutive doubles of one row: conflict-free.  Phase 4's reads are two
// broadcast addresses per group, LS doubles = 2 NMp + 2 dwords apart: distinct banks.  Phase 1's stores of raw are voice_quality_kernel's stores of
// Ldb: not conflict-free (rows q and q + 4 i at 4 mod 32 dwords), once per bin tile.
// A SILENT frame (no bin with raw > floor) keeps its power and its flux; loudness, log-energy, d_mfcc and d_bands are zeros and the live bit is 0.
// Frames >= nf are zeros.
struct AudTables {
    const double2* basis; const double* mel; const double* eq; const double* dct;
    int W, H, nfft, NB, NBp, skew, S, n_mel, NMp, LS, n_ceps, k_lo, k_hi;
    double compress;
};
struct AudParams { const float* x; const int32_t* len; double* frame; double* mfcc; int32_t* flags; double* bands; AudTables t; int L, NF; double floor; };

__global__ __launch_bounds__(256) void auditory_kernel(const AudParams p) {
    STOI_EXACT
    extern __shared__ __attribute__((aligned(16))) double aud_smem[];
    __shared__ double red[4][16][1];
    __shared__ int red_live[4][16];
    __shared__ double flux_s[16];
    const int b = blockIdx.y, f0 = blockIdx.x * 15, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int W = p.t.W, H = p.t.H, NB = p.t.NB, skew = p.t.skew, S = p.t.S, NM = p.t.n_mel, NMp = p.t.NMp, LS = p.t.LS, NC = p.t.n_ceps;
    int n;
    const int nf = voiceq_frames(p.len, b, p.L, H, &n);
    const size_t o0 = (size_t)b * p.NF + f0;
    double* out = p.frame + o0 * 4;
    double* mf = p.mfcc + o0 * NC;
    int32_t* fl = p.flags + o0;
    double* bd = p.bands ? p.bands + o0 * NM : nullptr;
    const int nfr = p.NF - f0 < 15 ? p.NF - f0 : 15;                    // the tile's frames inside the outputs (>= 1)
    if (f0 >= nf) {                                                     // (uniform) zeros past the row's own frames
        if (tid < 4 * nfr) out[tid] = 0.0;
        if (tid < nfr) fl[tid] = 0;
        if (tid < nfr * NC) mf[tid] = 0.0;
        if (bd) for (int i = tid; i < nfr * NM; i += 256) bd[i] = 0.0;
        return;
    }
    double* P = aud_smem;                                               // (16, S)
    double* Lg = P + 16 * S;                                            // (16, LS)
    double* Lc = Lg + 16 * LS;                                          // (16, LS)
    float* sx = (float*)(Lc + 16 * LS);
    const int span = 15 * H + W;
    {
        const float* xr = p.x + (size_t)b * p.L;
        const long long i0 = ((long long)f0 - 1) * H + H / 2 - W / 2;
        for (int t = tid; t < span; t += 256) {
            const long long i = i0 + t;
            sx[dft_word(t, H, skew)] = i >= 0 && i < n ? xr[i] : 0.f;
        }
    }
    __syncthreads();
    const int r = lane & 15, q = lane >> 4;
    {
        const int ntile = (NB + 15) >> 4, nsteps = W >> 2;
        DftSkewWalk walk(r, H, skew);
        double pw[4] = {0.0, 0.0, 0.0, 0.0};
        int live[4] = {0, 0, 0, 0};
        for (int bt = wv; bt < ntile; bt += 4) {
            const int col = bt * 16 + r;
            const double2* bp = p.t.basis + (size_t)q * NB + (col < NB ? col : NB - 1);
            stftd_acc xc = {0.0, 0.0, 0.0, 0.0}, xs = xc;
            walk.start(q);
            double2 cur[4], nxt[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) cur[u] = bp[(size_t)(u < nsteps ? u : nsteps - 1) * 4 * NB];
            for (int t0 = 0; t0 < nsteps; t0 += 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) nxt[u] = bp[(size_t)(t0 + 4 + u < nsteps ? t0 + 4 + u : nsteps - 1) * 4 * NB];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (t0 + u < nsteps) {                              // (uniform)
                        const double ax = (double)sx[walk.word()];
                        xc = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, cur[u].x, xc, 0, 0, 0);
                        xs = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, cur[u].y, xs, 0, 0, 0);
                        walk.step();
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
            }
            if (col < NB) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double raw = fma(xs[i], xs[i], xc[i] * xc[i]);
                    P[(q + 4 * i) * S + col] = raw;
                    pw[i] = pw[i] + raw;
                    live[i] += raw > p.floor ? 1 : 0;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) {
                pw[i] = pw[i] + __shfl_xor(pw[i], o, 64);
                live[i] += __shfl_xor(live[i], o, 64);
            }
            if (r == 0) { red[wv][q + 4 * i][0] = pw[i]; red_live[wv][q + 4 * i] = live[i]; }
        }
    }
    __syncthreads();                                                    // P, the powers and the live counts are complete
    if (wv < (NMp >> 4)) {                                              // (uniform per wave) E = P x mel, then phase 3
        const int nsteps = p.t.NBp >> 2;
        const int col = wv * 16 + r;                                    // (< NMp)
        const double* bp = p.t.mel + (size_t)q * NMp + col;
        const double* Pa = P + r * S;
        stftd_acc c = {0.0, 0.0, 0.0, 0.0};
        double cur[4], nxt[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) cur[u] = bp[(size_t)(u < nsteps ? u : nsteps - 1) * 4 * NMp];
        for (int t0 = 0; t0 < nsteps; t0 += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) nxt[u] = bp[(size_t)(t0 + 4 + u < nsteps ? t0 + 4 + u : nsteps - 1) * 4 * NMp];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (t0 + u < nsteps) {                                  // (uniform)
                    const int k = 4 * (t0 + u) + q;
                    c = __builtin_amdgcn_mfma_f64_16x16x4f64(Pa[k < NB ? k : NB - 1], cur[u], c, 0, 0, 0);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
        }
        if (col < NM) {
            const double eqv = p.t.eq[col];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = q + 4 * i;
                const double ef = fmax(c[i], p.floor);
                Lg[row * LS + col] = log(ef);
                Lc[row * LS + col] = pow(eqv * ef, p.t.compress);
                if (bd && row >= 1 && row <= nfr) {
                    const bool keep = f0 - 1 + row < nf && red_live[0][row] + red_live[1][row] + red_live[2][row] + red_live[3][row] > 0;
                    bd[(size_t)(row - 1) * NM + col] = keep ? c[i] : 0.0;
                }
            }
        }
    }
    {                                                                   // flux of row `row` against row - 1
        const int g = tid >> 4, j = tid & 15;
        const int row = (g >> 1) | ((g & 1) << 3);
        double s = 0.0;
        if (row >= 1) {
            const double* pa = P + row * S;
            const double* pb = pa - S;
            for (int k = p.t.k_lo + ((j - p.t.k_lo) & 15); k < p.t.k_hi; k += 16) {
                const double d = sqrt(pa[k]) - sqrt(pb[k]);
                s = fma(d, d, s);
            }
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
        if (j == 0) flux_s[row] = sqrt(s / (double)(p.t.k_hi - p.t.k_lo));
    }
    __syncthreads();                                                    // Lg, Lc and the fluxes are complete
    {
        const int row = tid >> 4, i = tid & 15;
        if (row >= 1 && row <= nfr) {
            const int f = f0 - 1 + row;
            const bool in = f < nf;
            const bool alive = in && red_live[0][row] + red_live[1][row] + red_live[2][row] + red_live[3][row] > 0;
            if (i < NC) {
                double s = 0.0;
                if (alive) for (int m = 0; m < NM; ++m) s = fma(Lg[row * LS + m], p.t.dct[m * NC + i], s);
                mf[(size_t)(row - 1) * NC + i] = s;
            }
            if (i == 15) {
                double loud = 0.0, power = 0.0, le = 0.0;
                if (in) power = dft_waves_sum(red, row, 0);
                if (alive) {
                    for (int m = 0; m < NM; ++m) loud = loud + Lc[row * LS + m];
                    le = log(fmax(power, p.floor));
                }
                double* o = out + 4 * (row - 1);
                o[0] = loud; o[1] = in && f >= 1 ? flux_s[row] : 0.0; o[2] = power; o[3] = le;
                fl[row - 1] = in ? (alive ? 1 : 0) | (f >= 1 ? 2 : 0) : 0;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Formant tracking (ev_formant_track): a Viterbi pass over the ways of mapping n_tracks tracks onto the candidates ev_formants wrote for a frame
// (the definition: include/emojivoice.h; Praat's Formant: Track is the model).  All float64, contraction OFF (STOI_EXACT), no atomics, no scratch.
// One workgroup per row, sequential over the frames like pyin_decode_kernel.  The S = C(n_cand, n_tracks) states are the strictly increasing index
// tuples in lexicographic order; a thread unranks its tuple once by the combinatorial number system into 16 nibbles of one 64-bit word (tup[s] in
// LDS for the predecessors, its own in a register), so no table is loaded and no array is indexed at run time.
//   lanes     S <= 32: one wave, G = the power of two with S G <= 64 lanes per target state (S = 10: 4); else one thread per target, G = 1, and
//             round_up(S, 64) threads.  Lane sub of a target scans the predecessors sub, sub + G, ... in ascending order, a later one replacing an
//             earlier one only when STRICTLY smaller; the G partial minima meet in an xor tree on (value, lowest index).  Min-with-lowest-index is
//             associative and commutative, so the split changes no bit.
//   per frame three pieces run, each for its own frame, and ONE barrier closes them:
//     A  delta_t from delta_{t-1} (LDS, double-buffered: t reads (t - 1) & 1 and writes t & 1), the tables of frame t and the back-pointer to d_back;
//     B  the tables of frame t + 1 into the other table buffer: Lt[k][c] = (cost_f |f - ref_k|) / 1000 + (cost_b bw) / f and, inside a segment,
//        D[c][c'] = cost_j |lg_t[c] - lg_{t+1}[c']|, so local is n_tracks lookups added in ascending k and trans another n_tracks: the same terms in
//        the same order as the direct formulas, and no log2, abs or division in the S^2 loop;
//     C  wave 0 stages frame t + 2 into a ring of four: {f, bw, log2 f} of its candidates and m (-1: a GAP; the finite / positive test is one ballot),
//        from registers whose loads were asked for a frame earlier.
//   Gaps, segment starts and segment ends are read from the ring's m and are uniform over the workgroup: nothing diverges around the barrier.
//   A state that is not valid in its frame holds +inf; D is 0 wherever a candidate at or past m is involved, so inf + D stays inf and never wins
//   (the state (0, 1, ..) is valid in every trackable frame: a valid target always has a finite minimum).
//   Behind the barrier of a segment's last frame wave 0 finds the lowest state of least delta (lane-strided read, xor tree) and lane 0 walks
//   d_back to the segment's first frame, writing d_sel and d_cost; the other waves go on and meet it at the next barrier.  After the last frame
//   the workgroup gathers d_track from d_sel in parallel.
// BANKS (from the LDS table of the kernel guide; no counter was read): ds_read_b64 is served 32 lanes at a time over 64 dword banks.  With G = 1
// the 64 lanes of a wave scan the same predecessor: tup[s] and delta[s] are broadcasts, and D[c_s(k)][c'(k)] is ONE row, at most 16 consecutive
// doubles: conflict-free.  With G > 1 a group's lanes read up to G rows; rows are 17 doubles apart (34 dwords), so rows r and r + 1 .. r + 15 start
// on different banks and two lanes meet on a bank only by chance of their columns (S <= 32: at most 3 x n_tracks such reads per frame).
struct FormantTrackParams {
    const double* formant; const int32_t* count; unsigned short* back; double* track; int32_t* sel; double* cost;
    int NF, nc, nt, S, G;
    double cf, cb, cj;
    double ref[16];
};
constexpr int FTRACK_DROW = 17;                                         // doubles per row of D
constexpr int FTRACK_TABLE = 16 * FTRACK_DROW + 256;                    // D, then Lt[k][16]

__device__ __forceinline__ int ftrack_binom(int n, int k) {             // C(n, k), exact (n <= 16)
    if (k < 0 || k > n) return 0;
    int r = 1;
    for (int i = 1; i <= k; ++i) r = r * (n - k + i) / i;
    return r;
}

__global__ __launch_bounds__(1024) void formant_track_kernel(const FormantTrackParams p) {
    STOI_EXACT
    extern __shared__ __attribute__((aligned(16))) double ftrack_lds[];
    const int b = blockIdx.x, tid = threadIdx.x, NT = blockDim.x, lane = tid & 63;
    const int NF = p.NF, nc = p.nc, nt = p.nt, S = p.S, G = p.G;
    const double inf = 1.0 / 0.0;
    double* dl = ftrack_lds;                                            // [2][S]
    unsigned long long* tup = (unsigned long long*)(dl + 2 * (size_t)S);   // [S]
    double* tb = (double*)(tup + S);                                    // [2][FTRACK_TABLE]
    double* ring = tb + 2 * FTRACK_TABLE;                               // [4][48]: f, bw, log2 f
    double* rf = ring + 4 * 48;                                         // [16]
    int* mm = (int*)(rf + 16);                                          // [4]
    const double* fmr = p.formant + (size_t)b * NF * nc * 2;
    const int32_t* ctr = p.count + (size_t)b * NF;
    unsigned short* back = p.back + (size_t)b * NF * S;
    double* trk = p.track + (size_t)b * NF * nt * 2;
    int32_t* sel = p.sel + (size_t)b * NF;
    double* cst = p.cost ? p.cost + (size_t)b * NF : nullptr;

    // C: frame w into ring slot w & 3 (wave 0 only; lanes >= n_cand hold no candidate).  fetch(w) asks for the frame's count and for every lane's
    // candidate, inside the count or not (the entry exists: lane < n_cand), into registers and waits for nothing; stage(w) uses them one frame
    // later, so the two loads, which do not depend on each other, travel under a whole frame's work instead of stalling it.
    int pc = 0;
    double pf = 0.0, pb = 0.0;
    auto fetch = [&](int w) {
        pc = ctr[w];
        if (lane < nc) { pf = fmr[((size_t)w * nc + lane) * 2]; pb = fmr[((size_t)w * nc + lane) * 2 + 1]; }
    };
    auto stage = [&](int w) {
        const int m = min(pc, nc);
        const bool mine = lane < m;                                     // (m <= n_cand <= 16)
        const double f = mine ? pf : 0.0, bw = mine ? pb : 0.0;
        const bool bad = mine && !(f > 0.0 && f < inf && fabs(bw) < inf);
        const bool gap = m < nt || __ballot(bad) != 0ull;
        if (lane < 16) {
            double* r = ring + (w & 3) * 48;
            r[lane] = f; r[16 + lane] = bw; r[32 + lane] = mine && !bad ? log2(f) : 0.0;
        }
        if (lane == 0) mm[w & 3] = gap ? -1 : m;
    };
    // B: the tables of frame u (trackable, m = mu) into buffer u & 1; D only where frame u - 1 is trackable too (mp >= 0)
    auto tables = [&](int u, int mu, int mp) {
        double* T = tb + (u & 1) * FTRACK_TABLE;
        const double* r = ring + (u & 3) * 48;
        const double* rp = ring + ((u - 1) & 3) * 48;
        for (int i = tid; i < nt * nc; i += NT) {
            const int k = i / nc, c = i - k * nc;
            double v = 0.0;
            if (c < mu) { const double f = r[c]; v = (p.cf * fabs(f - rf[k])) / 1000.0 + (p.cb * r[16 + c]) / f; }
            T[16 * FTRACK_DROW + k * 16 + c] = v;
        }
        if (mp >= 0)
            for (int i = tid; i < nc * nc; i += NT) {
                const int c = i / nc, c2 = i - c * nc;
                T[c * FTRACK_DROW + c2] = (c < mp && c2 < mu) ? p.cj * fabs(rp[32 + c] - r[32 + c2]) : 0.0;
            }
    };

    if (tid < 16) rf[tid] = tid < nt ? p.ref[tid] : 0.0;
    if (tid < S) {                                                      // the tuple of state tid: lexicographic unranking
        unsigned long long t = 0ull;
        int r = tid, x = 0;
        for (int i = 0; i < nt; ++i) {
            for (;; ++x) {
                const int below = ftrack_binom(nc - x - 1, nt - i - 1);
                if (r < below) break;
                r -= below;
            }
            t |= (unsigned long long)x << (4 * i);
            ++x;
        }
        tup[tid] = t;
    }
    if (tid < 64) {
        fetch(0); stage(0);
        if (NF > 1) { fetch(1); stage(1); }
        if (NF > 2) fetch(2);
    }
    __syncthreads();
    const int sp = min(tid / G, S - 1), sub = tid & (G - 1);
    const bool owner = tid / G < S && sub == 0;
    const unsigned long long mine = tup[sp];
    const int top = (int)((mine >> (4 * (nt - 1))) & 15);               // the state is valid in a frame iff top < m
    {
        const int m0 = mm[0];
        if (m0 >= 0) tables(0, m0, -1);
    }
    __syncthreads();

    int seg0 = 0;                                                       // the first frame of the segment frame t lies in
    for (int t = 0; t < NF; ++t) {
        const int m = mm[t & 3], mp = t > 0 ? mm[(t - 1) & 3] : -1, mn = t + 1 < NF ? mm[(t + 1) & 3] : -1;
        if (m >= 0) {
            const double* T = tb + (t & 1) * FTRACK_TABLE;
            const double* Lt = T + 16 * FTRACK_DROW;
            double local = Lt[(int)(mine & 15)];
            for (int k = 1; k < nt; ++k) local = local + Lt[k * 16 + (int)((mine >> (4 * k)) & 15)];
            double d;
            if (mp < 0) { seg0 = t; d = local; }
            else {
                const double* prev = dl + (size_t)((t - 1) & 1) * S;
                double best = inf;
                int arg = 0x7fffffff;
                for (int s = sub; s < S; s += G) {
                    const unsigned long long ts = tup[s];
                    double tr = T[(int)(ts & 15) * FTRACK_DROW + (int)(mine & 15)];
                    for (int k = 1; k < nt; ++k)
                        tr = tr + T[(int)((ts >> (4 * k)) & 15) * FTRACK_DROW + (int)((mine >> (4 * k)) & 15)];
                    const double v = prev[s] + tr;
                    if (v < best) { best = v; arg = s; }
                }
                for (int o = G >> 1; o > 0; o >>= 1) {                  // (G is uniform: every lane of the wave takes part)
                    const double ov = __shfl_xor(best, o, 64);
                    const int os = __shfl_xor(arg, o, 64);
                    if (ov < best || (ov == best && os < arg)) { best = ov; arg = os; }
                }
                d = best + local;
                if (owner) back[(size_t)t * S + sp] = (unsigned short)(top < m && arg < S ? arg : 0);
            }
            if (owner) dl[(size_t)(t & 1) * S + sp] = top < m ? d : inf;
        } else {                                                        // a GAP: zeros and -1
            if (tid == 0) { sel[t] = -1; if (cst) cst[t] = 0.0; }
        }
        if (mn >= 0) tables(t + 1, mn, m);
        if (tid < 64 && t + 2 < NF) {
            stage(t + 2);
            if (t + 3 < NF) fetch(t + 3);
        }
        __syncthreads();
        if (m >= 0 && mn < 0 && tid < 64) {                             // the segment seg0 .. t is complete: its end state and its path
            const double* cur = dl + (size_t)(t & 1) * S;
            double bv = inf;
            int bs = 0x7fffffff;
            for (int s = lane; s < S; s += 64) { const double v = cur[s]; if (v < bv) { bv = v; bs = s; } }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ov = __shfl_xor(bv, o, 64);
                const int os = __shfl_xor(bs, o, 64);
                if (ov < bv || (ov == bv && os < bs)) { bv = ov; bs = os; }
            }
            if (tid == 0) {
                int s = min(bs, S - 1);
                for (int q = t; q >= seg0; --q) {
                    sel[q] = s;
                    if (cst) cst[q] = q == t ? bv : 0.0;
                    if (q > seg0) s = min((int)back[(size_t)q * S + s], S - 1);   // (the clamp keeps a damaged word inside the states)
                }
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < NF * nt; i += NT) {                           // d_track: a copy of the chosen candidates, zeros on gaps
        const int t = i / nt, k = i - t * nt, s = sel[t];
        double f = 0.0, bw = 0.0;
        if (s >= 0) {
            const int c = (int)((tup[min(s, S - 1)] >> (4 * k)) & 15);
            f = fmr[((size_t)t * nc + c) * 2]; bw = fmr[((size_t)t * nc + c) * 2 + 1];
        }
        trk[(size_t)i * 2] = f; trk[(size_t)i * 2 + 1] = bw;
    }
}

// ---------------------------------------------------------------------------
// SRMR (ev_srmr): the speech-to-reverberation modulation energy ratio of a row (Falk, Zheng and Chan 2010), the definition and every order:
// include/emojivoice.h.  All float64, contraction OFF (STOI_EXACT): an fma is an fma only where fma() is written.  No atomics.
// A row is cut into chunks of H samples from its first sample; a row of nf frames has nc = nf + 3 chunks, all of them whole and inside len.  Both
// recurrences are linear in (state, input) (the cascade over the complex numbers, a band's biquad over the reals), the envelope between them is not,
// so the true states come in two rounds.  Six launches:
//   1. srmr_chunk_kernel<0>:   a wave per (row, chunk), lane = channel: the cascade from zero state; keeps the 4 complex states it reaches;
//   2. srmr_carry_chan_kernel: a wave per row, lane = channel: s[c + 1] = M s[c] + z[c] in ascending c, in place: slot c then holds the state at the
//                              START of chunk c;
//   3. srmr_chunk_kernel<1>:   lane = (channel, half of the bands): the cascade from its true state, the envelope, the lane's up to four bands from
//                              zero state; keeps the two doubles per band they reach;
//   4. srmr_carry_band_kernel: a workgroup per row, thread = (channel, band): the 2 x 2 carry, in place;
//   5. srmr_chunk_kernel<2>:   everything from its true state; per band the four window-quarter sums of the chunk (one fma per sample, ascending);
//   6. srmr_rows_kernel:       a workgroup per row, thread = (channel, band): E[f] from the pieces of four chunks, the ascending mean; then thread 0
//                              takes the shares, j90, K* and the ratio in the header's order.
// MAPPING.  The channels of one (row, chunk) read the SAME samples and the same window values, so they lie along the lanes of one wave and those
// reads are wave-uniform (scalar loads).  A lane with all eight bands would hold 16 band states, 32 piece sums, 40 coefficients and the cascade:
// well over a hundred doubles.  Two lanes per channel (bands 0..3 and 4..7) hold 55 each and both run the cascade: it is a third of a lane's work.
// Lanes past N, and bands past K, run on zero coefficients and store nothing.
constexpr int SRMR_MAXN = 32, SRMR_MAXK = 8, SRMR_KB = 4;               // channels, bands, bands per lane

struct SrmrTables {
    const double* chan; const double* Mc;                              // (N, 3) {Re a, Im a, gain}; (N, 10, 2) the lower triangle of M by rows {re, im}
    const double* mod; const double* Mb;                               // (K, 5) {b0, b1, b2, a1, a2}; (K, 4) {M00, M01, M10, M11}
    const double* win; const double* erb; const double* cut;           // (4 H); (N); (K)
    int N, K, H;
};

__device__ __forceinline__ int srmr_frames(const int32_t* len, int b, int L, int H) {
    int n = len ? len[b] : L;
    if (n < 1 || n > L) n = 0;                                          // a bad row is an empty row (the ev_mas_align convention)
    return n >= 4 * H ? (n - 4 * H) / H + 1 : 0;
}

// Arena: cst (B, NC, 8, N) {re1, im1 .. re4, im4}; bst (B, NC, 2, N K); part (B, NC, 4, N K)
struct SrmrChunkParams { const float* x; const int32_t* len; double* cst; double* bst; double* part; SrmrTables t; int L, NC; };

template <int PASS>
__global__ __launch_bounds__(64) void srmr_chunk_kernel(const SrmrChunkParams p) {
    STOI_EXACT
    const int b = blockIdx.y, c = blockIdx.x, lane = threadIdx.x;
    const int N = p.t.N, K = p.t.K, H = p.t.H, NK = N * K;
    const int nf = srmr_frames(p.len, b, p.L, H);
    if (nf == 0 || c >= nf + 3) return;                                 // (uniform) chunk c is no chunk of this row
    const int j = PASS == 0 ? lane : lane >> 1, k0 = PASS == 0 ? 0 : (lane & 1) * SRMR_KB;
    const bool live = j < N;
    const int jj = live ? j : 0;
    const double ar = live ? p.t.chan[3 * jj] : 0.0, ai = live ? p.t.chan[3 * jj + 1] : 0.0, g = live ? p.t.chan[3 * jj + 2] : 0.0;
    double* cs = p.cst + ((size_t)b * p.NC + c) * 8 * N + jj;
    double r1 = 0.0, i1 = 0.0, r2 = 0.0, i2 = 0.0, r3 = 0.0, i3 = 0.0, r4 = 0.0, i4 = 0.0;
    if (PASS > 0 && live) {
        r1 = cs[0]; i1 = cs[N]; r2 = cs[2 * N]; i2 = cs[3 * N]; r3 = cs[4 * N]; i3 = cs[5 * N]; r4 = cs[6 * N]; i4 = cs[7 * N];
    }
    double b0[SRMR_KB], b1[SRMR_KB], b2[SRMR_KB], a1[SRMR_KB], a2[SRMR_KB], s1[SRMR_KB], s2[SRMR_KB], acc[SRMR_KB][4];
    double* bs = p.bst + ((size_t)b * p.NC + c) * 2 * NK + (size_t)jj * K;
    if (PASS > 0) {
#pragma unroll
        for (int i = 0; i < SRMR_KB; ++i) {
            const bool on = live && k0 + i < K;
            const double* m = p.t.mod + 5 * (on ? k0 + i : 0);
            b0[i] = on ? m[0] : 0.0; b1[i] = on ? m[1] : 0.0; b2[i] = on ? m[2] : 0.0; a1[i] = on ? m[3] : 0.0; a2[i] = on ? m[4] : 0.0;
            s1[i] = PASS == 2 && on ? bs[k0 + i] : 0.0;
            s2[i] = PASS == 2 && on ? bs[NK + k0 + i] : 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[i][q] = 0.0;
        }
    }
    const float* x = p.x + (size_t)b * p.L + (size_t)c * H;             // ((c + 1) H <= (nf + 3) H <= len: the chunk lies inside the row)
    const double* w = p.t.win;
#pragma unroll 4
    for (int t = 0; t < H; ++t) {
        const double xv = (double)x[t];                                 // (wave-uniform, as the window values below)
        double nr, ni;                                                  // stage k: s = v + a s, v the stage before's NEW value (stage 1: the sample)
        nr = xv + (ar * r1 - ai * i1); ni = ar * i1 + ai * r1;        r1 = nr; i1 = ni;
        nr = r1 + (ar * r2 - ai * i2); ni = i1 + (ar * i2 + ai * r2); r2 = nr; i2 = ni;
        nr = r2 + (ar * r3 - ai * i3); ni = i2 + (ar * i3 + ai * r3); r3 = nr; i3 = ni;
        nr = r3 + (ar * r4 - ai * i4); ni = i3 + (ar * i4 + ai * r4); r4 = nr; i4 = ni;
        if (PASS > 0) {
            const double e = g * sqrt(r4 * r4 + i4 * i4);
            double wq[4];
            if (PASS == 2) {
#pragma unroll
                for (int q = 0; q < 4; ++q) wq[q] = w[q * H + t];
            }
#pragma unroll
            for (int i = 0; i < SRMR_KB; ++i) {
                const double y = fma(b0[i], e, s1[i]);                  // transposed direct form II, ev_loudness's fmas
                s1[i] = fma(-a1[i], y, fma(b1[i], e, s2[i]));
                s2[i] = fma(-a2[i], y, b2[i] * e);
                if (PASS == 2) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) { const double v = wq[q] * y; acc[i][q] = fma(v, v, acc[i][q]); }
                }
            }
        }
    }
    if (!live) return;
    if (PASS == 0) {
        cs[0] = r1; cs[N] = i1; cs[2 * N] = r2; cs[3 * N] = i2; cs[4 * N] = r3; cs[5 * N] = i3; cs[6 * N] = r4; cs[7 * N] = i4;
    } else if (PASS == 1) {
#pragma unroll
        for (int i = 0; i < SRMR_KB; ++i) if (k0 + i < K) { bs[k0 + i] = s1[i]; bs[NK + k0 + i] = s2[i]; }
    } else {
        double* pt = p.part + ((size_t)b * p.NC + c) * 4 * NK + (size_t)j * K;
#pragma unroll
        for (int i = 0; i < SRMR_KB; ++i)
            if (k0 + i < K) {
#pragma unroll
                for (int q = 0; q < 4; ++q) pt[(size_t)q * NK + k0 + i] = acc[i][q];
            }
    }
}

// The carries.  Slot c of a row's states goes from "what chunk c reaches from zero" to "the state at the start of chunk c", in ascending c.  Four
// chunks' results are loaded before the chain takes them (the loads do not wait for the chain).
// Channel: s'[r] = z[r] + sum over k <= r of M[r][k] s[k] as complex numbers, k ascending from z[r]: re = re + (Mre sre - Mim sim),
// im = im + (Mre sim + Mim sre).
struct SrmrCarryParams { double* st; const int32_t* len; SrmrTables t; int L, NC; };

__global__ __launch_bounds__(64) void srmr_carry_chan_kernel(const SrmrCarryParams p) {
    STOI_EXACT
    const int b = blockIdx.x, j = threadIdx.x, N = p.t.N;
    const int nf = srmr_frames(p.len, b, p.L, p.t.H);
    if (nf == 0 || j >= N) return;
    const int nc = nf + 3;
    double M[20];
#pragma unroll
    for (int i = 0; i < 20; ++i) M[i] = p.t.Mc[20 * j + i];
    double* st = p.st + (size_t)b * p.NC * 8 * N + j;
    double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int c0 = 0; c0 < nc; c0 += 4) {
        double z[4][8];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int r = 0; r < 8; ++r) z[u][r] = c0 + u < nc ? st[((size_t)(c0 + u) * 8 + r) * N] : 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (c0 + u >= nc) break;
            double n[8];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double re = z[u][2 * r], im = z[u][2 * r + 1];
#pragma unroll
                for (int k = 0; k <= r; ++k) {
                    const double mr = M[2 * (r * (r + 1) / 2 + k)], mi = M[2 * (r * (r + 1) / 2 + k) + 1];
                    re = re + (mr * s[2 * k] - mi * s[2 * k + 1]);
                    im = im + (mr * s[2 * k + 1] + mi * s[2 * k]);
                }
                n[2 * r] = re; n[2 * r + 1] = im;
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) { st[((size_t)(c0 + u) * 8 + r) * N] = s[r]; s[r] = n[r]; }
        }
    }
}

// Band: s1' = (z1 + M00 s1) + M01 s2; s2' = (z2 + M10 s1) + M11 s2.
__global__ __launch_bounds__(256) void srmr_carry_band_kernel(const SrmrCarryParams p) {
    STOI_EXACT
    const int b = blockIdx.x, jk = threadIdx.x, NK = p.t.N * p.t.K;
    const int nf = srmr_frames(p.len, b, p.L, p.t.H);
    if (nf == 0 || jk >= NK) return;
    const int nc = nf + 3;
    const double* m = p.t.Mb + 4 * (jk % p.t.K);
    const double m00 = m[0], m01 = m[1], m10 = m[2], m11 = m[3];
    double* st = p.st + (size_t)b * p.NC * 2 * NK + jk;
    double s1 = 0.0, s2 = 0.0;
    for (int c0 = 0; c0 < nc; c0 += 4) {
        double z[4][2];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            z[u][0] = c0 + u < nc ? st[(size_t)(c0 + u) * 2 * NK] : 0.0;
            z[u][1] = c0 + u < nc ? st[(size_t)(c0 + u) * 2 * NK + NK] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (c0 + u >= nc) break;
            const double n1 = (z[u][0] + m00 * s1) + m01 * s2, n2 = (z[u][1] + m10 * s1) + m11 * s2;
            st[(size_t)(c0 + u) * 2 * NK] = s1; st[(size_t)(c0 + u) * 2 * NK + NK] = s2;
            s1 = n1; s2 = n2;
        }
    }
}

// One workgroup per row; thread (j, k) walks the frames in ascending f, then thread 0 closes the row in the header's order.
struct SrmrRowsParams { const double* part; const int32_t* len; double* frame; double* mean; double* srmr; int32_t* counts; SrmrTables t; int L, NC, NF; };

__global__ __launch_bounds__(256) void srmr_rows_kernel(const SrmrRowsParams p) {
    STOI_EXACT
    __shared__ double mean[SRMR_MAXN * SRMR_MAXK];
    __shared__ double chan[SRMR_MAXN];
    const int b = blockIdx.x, jk = threadIdx.x, N = p.t.N, K = p.t.K, NK = N * K;
    const int nf = srmr_frames(p.len, b, p.L, p.t.H);
    if (jk < NK) {
        const double* pt = p.part + (size_t)b * p.NC * 4 * NK + jk;     // (not read where nf == 0: there may be no arena)
        double* fr = p.frame ? p.frame + (size_t)b * p.NF * NK + jk : nullptr;
        double sum = 0.0;
#pragma unroll 4
        for (int f = 0; f < nf; ++f) {
            const double E = (pt[((size_t)f * 4) * NK] + pt[((size_t)(f + 1) * 4 + 1) * NK]) + (pt[((size_t)(f + 2) * 4 + 2) * NK] + pt[((size_t)(f + 3) * 4 + 3) * NK]);
            if (fr) fr[(size_t)f * NK] = E;
            sum = sum + E;
        }
        if (fr) for (int f = nf; f < p.NF; ++f) fr[(size_t)f * NK] = 0.0;
        const double m = nf > 0 ? sum / (double)nf : 0.0;
        mean[jk] = m;
        p.mean[(size_t)b * NK + jk] = m;
    }
    __syncthreads();
    if (jk != 0) return;
    double ratio = 0.0, bw = 0.0;
    int j90 = 0, ks = 0;
    if (nf > 0) {
        double total = 0.0;
        for (int j = 0; j < N; ++j) {
            double ch = 0.0;
            for (int k = 0; k < K; ++k) ch = ch + mean[j * K + k];
            chan[j] = ch;
            total = total + ch;
        }
        double cum = 0.0;
        j90 = N - 1;                                                    // (silence: no share exceeds anything)
        for (int j = 0; j < N; ++j) {
            cum = cum + chan[j] / total;
            if (cum > 0.9) { j90 = j; break; }
        }
        bw = p.t.erb[j90];
        int below = 0;
        for (int k = 0; k < K; ++k) below += p.t.cut[k] < bw ? 1 : 0;
        ks = min(K, max(min(5, K), below));
        double num = 0.0, den = 0.0;
        for (int j = 0; j < N; ++j)
            for (int k = 0; k < min(4, K); ++k) num = num + mean[j * K + k];
        for (int j = 0; j < N; ++j)
            for (int k = 4; k < ks; ++k) den = den + mean[j * K + k];
        ratio = K > 4 && den > 0.0 ? num / den : 0.0;
    }
    p.srmr[2 * b] = ratio; p.srmr[2 * b + 1] = bw;
    p.counts[3 * b] = nf; p.counts[3 * b + 1] = j90; p.counts[3 * b + 2] = ks;
}

// ---------------------------------------------------------------------------
// Speech rate and pauses (ev_speech_rate): De Jong and Wempe's syllable nuclei on ev_pitch_yin's frame grid: a power contour, a sounding / silent
// segmentation with minimum durations, and the local peaks of the power that are followed by a dip and are voiced (the definition:
// include/emojivoice.h).  All float64, contraction OFF (STOI_EXACT), no atomics.  Two launches.
//   speech_power_kernel      grid (tiles of RATE_T frames, B), 256 threads.  The tile's span of (T - 1) H + W samples is staged ONCE in LDS as
//            float (zero outside [0, len): nothing at or behind len is read), so a sample leaves global memory once per tile and not W / H
//            times.  A wave per frame, lane = slot: term j belongs to lane j mod 64, which adds its terms in ascending j, then
//            formant_wave_sum's xor tree (32, 16, 8, 4, 2, 1), which leaves the same bits in every lane.  A wave takes its four frames TOGETHER:
//            four independent chains per lane that share every load of the window, which is read from global memory (W doubles, coalesced,
//            resident in L2 for the whole grid).  Frames in [nf, NF) are written as zeros.
//   speech_rate_rows_kernel  grid B, 1024 threads, the row's power in dynamic LDS (8 B a frame) beside one byte of flags per frame and 1152 bytes
//            of hand-over: 9 NF + 1152 bytes, 145.1 KiB at NF = 16384.  Frame f belongs to thread f mod 1024 of tile f / 1024 in every phase.
//            (1) the (k + 1)-th largest power by 64 passes over the bit patterns (held in registers, 16 a thread), most significant bit first: a
//            ballot per wave and tile counts the frames
//            that agree with the prefix found so far and carry the bit, the 16 waves' counts go through LDS (two alternating sets: one barrier
//            a pass).  (2) every decision on runs is a FORWARD pass and a BACKWARD pass over the tiles: forward, functionals_kernel's inclusive
//            max-scan of "a run starts here" brings the start to the run's last frame, whose thread knows the length and leaves the decision in
//            bit 7 of its flag byte; backward, the same scan on mirrored indices brings every frame the last frame of its run, where it reads the
//            decision.  Step (a) reads bit 1 (raw) and writes bit 2, step (b) reads bit 2 and writes bit 0 (snd), so no pass reads a bit that it
//            writes.  (3) a forward pass over the runs of snd counts the pauses and marks the candidates (bit 2); (4) a backward SEGMENTED
//            min-scan, whose segments end in front of every candidate, brings candidate c the minimum over (c, e).  (5) integer reductions.
constexpr int RATE_T = 16;                                              // frames per tile of speech_power_kernel
constexpr int RATE_MAXF = 16384;                                        // frames per row: the row's power stays in LDS

__device__ __forceinline__ int rate_frames(const int32_t* len, int b, int L, int H, int* n_out) {
    const int n = len ? len[b] : L;
    *n_out = n;
    return n < 1 || n > L ? 0 : (n + H - 1) / H;                        // (n <= L <= RATE_MAXF * 1024)
}

struct RatePowerParams { const float* x; const int32_t* len; const double* win; double* power; int L, NF, W, H; double sw; };

__global__ __launch_bounds__(256) void speech_power_kernel(const RatePowerParams p) {
    STOI_EXACT
    extern __shared__ __attribute__((aligned(16))) float rate_xs[];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, b = blockIdx.y, f0 = blockIdx.x * RATE_T;
    const int W = p.W, H = p.H;
    int n;
    const int nf = rate_frames(p.len, b, p.L, H, &n);
    const int nt = min(RATE_T, nf - f0);                                // the tile's live frames (none where <= 0)
    double* out = p.power + (size_t)b * p.NF;
    if (nt <= 0) {                                                      // (uniform; before any barrier)
        if (t < RATE_T && f0 + t < p.NF) out[f0 + t] = 0.0;
        return;
    }
    const float* xr = p.x + (size_t)b * p.L;
    const int base = f0 * H + H / 2 - W / 2, span = (RATE_T - 1) * H + W;
    for (int i = t; i < span; i += 256) {                               // (the whole span, so that every frame of the tile reads defined values)
        const int g = base + i;
        rate_xs[i] = g >= 0 && g < n ? xr[g] : 0.0f;
    }
    __syncthreads();
    // wave w takes frames w, w + 4, w + 8 and w + 12 of the tile TOGETHER: four independent chains per lane share every load of the window
    const float* s = rate_xs + w * H;
    double a[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0}, m[4];
    for (int j = lane; j < W; j += 64) {
        const double wj = p.win[j];
#pragma unroll
        for (int r = 0; r < 4; ++r) a[r] = a[r] + wj * (double)s[4 * r * H + j];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) m[r] = formant_wave_sum(a[r]) / p.sw;
    for (int j = lane; j < W; j += 64) {
        const double wj = p.win[j];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double d = (double)s[4 * r * H + j] - m[r];
            q[r] = q[r] + wj * (d * d);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double P = formant_wave_sum(q[r]) / p.sw;
        const int fi = w + 4 * r;
        if (lane == 0 && f0 + fi < p.NF) out[f0 + fi] = fi < nt ? P : 0.0;
    }
}

struct RateRowsParams {
    const double* power; const int32_t* len; const uint8_t* voiced; uint8_t* mark; double* stat; int32_t* count;
    int L, NF, H, min_pause, min_sound;
    double floor, rank, silence, dip;
};

// One tile of an inclusive max-scan over the workgroup's 1024 threads in ascending (FWD) or descending thread order, `car` the running maximum of
// the tiles before; wm: 16 words, another set than the tile before used (one barrier per tile).  Every thread of the workgroup calls it.
template <bool FWD>
__device__ __forceinline__ int rate_scan_max(int v, int& car, int* wm, int lane, int w) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int a = FWD ? __shfl_up(v, o, 64) : __shfl_down(v, o, 64);
        if (FWD ? lane >= o : lane + o < 64) v = max(v, a);
    }
    if (lane == (FWD ? 63 : 0)) wm[w] = v;
    __syncthreads();
    v = max(v, car);
#pragma unroll
    for (int x = 0; x < 16; ++x) {
        const int a = wm[x];
        if (FWD ? x < w : x > w) v = max(v, a);
        car = max(car, a);
    }
    return v;
}

__device__ __forceinline__ int rate_bit(const uint8_t* mk, int f, int bit) { return mk[f] >> bit & 1; }

// Forward: whether frame f is the last of its run of equal `bit`; *start: the run's first frame (valid there)
__device__ __forceinline__ bool rate_run_fwd(const uint8_t* mk, int f, int nf, int bit, int& car, int* wm, int lane, int w, int* fl, int* start) {
    const bool in = f < nf;
    *fl = in ? rate_bit(mk, f, bit) : 0;
    const bool first = in && (f == 0 || rate_bit(mk, f - 1, bit) != *fl), last = in && (f + 1 == nf || rate_bit(mk, f + 1, bit) != *fl);
    *start = rate_scan_max<true>(first ? f : -1, car, wm, lane, w);
    return last;
}

// Backward: the last frame of the run of equal `bit` that holds frame f (for f < nf)
__device__ __forceinline__ int rate_run_bwd(const uint8_t* mk, int f, int nf, int bit, int& car, int* wm, int lane, int w) {
    const bool last = f < nf && (f + 1 == nf || rate_bit(mk, f + 1, bit) != rate_bit(mk, f, bit));
    return nf - 1 - rate_scan_max<false>(last ? nf - 1 - f : -1, car, wm, lane, w);
}

// The bit pattern of the (k + 1)-th largest of Pl[0 .. nf), nf <= 1024 NT: 64 passes, most significant bit first, over the thread's NT frames held
// in registers (0 past nf: it never carries a bit); per pass a ballot per wave and tile counts the frames that agree with the prefix found so far
// and carry the bit, and the 16 waves' counts go through wc (two alternating sets of 16 words: one barrier a pass).  Every thread calls it.
template <int NT>
__device__ __forceinline__ unsigned long long rate_select(const double* Pl, int nf, int k, int* wc, int t) {
    const int lane = t & 63, w = t >> 6;
    unsigned long long pv[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int f = (i << 10) + t;
        pv[i] = f < nf ? (unsigned long long)__double_as_longlong(Pl[f]) : 0ull;
    }
    unsigned long long pre = 0ull;
    for (int bit = 63; bit >= 0; --bit) {
        const unsigned long long want = pre >> bit | 1ull;
        int c = 0;
#pragma unroll
        for (int i = 0; i < NT; ++i) c += __popcll(__ballot(pv[i] >> bit == want));
        int* set = wc + (bit & 1) * 16;
        if (lane == 0) set[w] = c;
        __syncthreads();
        int tot = 0;
#pragma unroll
        for (int x = 0; x < 16; ++x) tot += set[x];
        if (tot > k) pre |= 1ull << bit; else k -= tot;
    }
    return pre;
}

__global__ __launch_bounds__(1024) void speech_rate_rows_kernel(const RateRowsParams p) {
    STOI_EXACT
    extern __shared__ __attribute__((aligned(16))) double rate_smem[];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, b = blockIdx.x, NF = p.NF;
    double* Pl = rate_smem;                                             // [NF]
    double* wv = Pl + NF;                                               // [2][16]: the waves' minima of a tile (segmented scan)
    int* wm = (int*)(wv + 32);                                          // [2][16]: the waves' last scan values of a tile
    int* wh = wm + 32;                                                  // [2][16]: the waves' segment flags of a tile
    int* wc = wh + 32;                                                  // [2][16]: the waves' counts of a selection pass
    int* red = wc + 32;                                                 // [16][8]
    uint8_t* mk = (uint8_t*)(red + 128);                                // [NF]
    uint8_t* o_mk = p.mark ? p.mark + (size_t)b * NF : nullptr;
    double* o_st = p.stat + (size_t)b * 4;
    int32_t* o_ct = p.count + (size_t)b * 8;
    int n;
    const int nf = rate_frames(p.len, b, p.L, p.H, &n);
    if (nf == 0) {                                                      // a bad row is a row of zeros (uniform; before any barrier)
        if (o_mk) for (int f = t; f < NF; f += 1024) o_mk[f] = 0;
        if (t < 4) o_st[t] = 0.0;
        if (t < 8) o_ct[t] = 0;
        return;
    }
    const double* pw = p.power + (size_t)b * NF;
    for (int f = t; f < nf; f += 1024) Pl[f] = pw[f];
    __syncthreads();
    const int ntile = (nf + 1023) >> 10;
    // ---- (1) the (k + 1)-th largest of the bit patterns
    const int k = (int)floor(p.rank * (double)(nf - 1));
    const unsigned long long pre = ntile <= 1 ? rate_select<1>(Pl, nf, k, wc, t) : ntile <= 4 ? rate_select<4>(Pl, nf, k, wc, t) : rate_select<RATE_MAXF / 1024>(Pl, nf, k, wc, t);
    const double ref = __longlong_as_double((long long)pre), thr = ref * p.silence;
    for (int f = t; f < nf; f += 1024) { const double v = Pl[f]; mk[f] = v > thr && v > p.floor ? 2 : 0; }
    __syncthreads();
    int it = 0, car;
    // ---- (2a) silent runs under min_pause between raw frames become sounding: bit 1 -> bit 2
    car = -1;
    for (int i = 0; i < ntile; ++i, ++it) {
        const int f = (i << 10) + t;
        int fl, s;
        if (rate_run_fwd(mk, f, nf, 1, car, wm + (it & 1) * 16, lane, w, &fl, &s))
            mk[f] = (uint8_t)(fl << 1 | (!fl && s > 0 && f + 1 < nf && f - s + 1 < p.min_pause ? 0x80 : 0));
    }
    __syncthreads();
    car = -1;
    for (int i = ntile - 1; i >= 0; --i, ++it) {
        const int f = (i << 10) + t;
        const int e = rate_run_bwd(mk, f, nf, 1, car, wm + (it & 1) * 16, lane, w);
        if (f < nf) { const int m = mk[f]; mk[f] = (uint8_t)(m | ((m & 2) || (mk[e] & 0x80) ? 4 : 0)); }
    }
    __syncthreads();
    // ---- (2b) sounding runs under min_sound become silent: bit 2 -> bit 0
    car = -1;
    for (int i = 0; i < ntile; ++i, ++it) {
        const int f = (i << 10) + t;
        int fl, s;
        if (rate_run_fwd(mk, f, nf, 2, car, wm + (it & 1) * 16, lane, w, &fl, &s))
            mk[f] = (uint8_t)((mk[f] & 0x7f) | (fl && f - s + 1 < p.min_sound ? 0x80 : 0));
    }
    __syncthreads();
    car = -1;
    for (int i = ntile - 1; i >= 0; --i, ++it) {
        const int f = (i << 10) + t;
        const int e = rate_run_bwd(mk, f, nf, 2, car, wm + (it & 1) * 16, lane, w);
        if (f < nf) { const int m = mk[f]; mk[f] = (uint8_t)(m | ((m & 4) && !(mk[e] & 0x80) ? 1 : 0)); }
    }
    __syncthreads();
    // ---- (3) the runs of snd: pauses, the leading and the trailing silence; the candidates (bit 2 from here on)
    int nsnd = 0, npause = 0, s1 = 0, s2 = 0, ncand = 0, nnuc = 0, lead = 0, trail = 0;
    car = -1;
    for (int i = 0; i < ntile; ++i, ++it) {
        const int f = (i << 10) + t;
        int fl, s;
        const bool last = rate_run_fwd(mk, f, nf, 0, car, wm + (it & 1) * 16, lane, w, &fl, &s);
        if (f < nf) {
            nsnd += fl;
            if (last && !fl) {
                const int l = f - s + 1;
                if (s == 0) lead = l;                                   // (a row without a sounding frame is all leading silence)
                else if (f + 1 == nf) trail = l;
                else { ++npause; s1 += l; s2 += l * l; }
            }
            bool cand = false;
            if (fl && f >= 1 && f + 2 <= nf) { const double v = Pl[f]; cand = v > Pl[f - 1] && v >= Pl[f + 1] && v > thr; }
            ncand += cand;
            mk[f] = (uint8_t)((mk[f] & 3) | (cand ? 4 : 0));
        }
    }
    __syncthreads();
    // ---- (4) element f stands for frame f + 1; a segment ends (h) at the row's last frame and in front of a candidate
    double carv = INFINITY;
    for (int i = ntile - 1; i >= 0; --i, ++it) {
        const int f = (i << 10) + t, g = f + 1;
        double v = g < nf ? Pl[g] : INFINITY;
        int h = g + 1 >= nf || (mk[g + 1] & 4) ? 1 : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double a = __shfl_down(v, o, 64);
            const int c = __shfl_down(h, o, 64);
            if (lane + o < 64) { if (!h && a < v) v = a; h |= c; }
        }
        double* sv = wv + (it & 1) * 16;
        int* sh = wh + (it & 1) * 16;
        if (lane == 0) { sv[w] = v; sh[w] = h; }
        __syncthreads();
        double av = carv, rv = v;
#pragma unroll
        for (int x = 15; x >= 0; --x) {                                 // the tiles behind, then the waves behind, nearest last
            if (x == w && !h && av < v) rv = av;
            const double xv = sv[x];
            const int xh = sh[x];
            if (xh) av = xv; else if (xv < av) av = xv;
        }
        carv = av;
        if (f < nf) {
            int m = mk[f];
            if (m & 4) {
                const bool dip = rv * p.dip <= Pl[f];
                if (dip && (!p.voiced || p.voiced[(size_t)b * NF + f] != 0)) { m |= 8; ++nnuc; }
            }
            if (o_mk) o_mk[f] = (uint8_t)(m & 15);
        }
    }
    if (o_mk) for (int f = nf + t; f < NF; f += 1024) o_mk[f] = 0;
    // ---- (5)
    nsnd = func_wave_isum(nsnd); npause = func_wave_isum(npause); s1 = func_wave_isum(s1); s2 = func_wave_isum(s2);
    ncand = func_wave_isum(ncand); nnuc = func_wave_isum(nnuc); lead = func_wave_isum(lead); trail = func_wave_isum(trail);
    if (lane == 0) {
        int* r = red + 8 * w;
        r[0] = nsnd; r[1] = npause; r[2] = s1; r[3] = s2; r[4] = ncand; r[5] = nnuc; r[6] = lead; r[7] = trail;
    }
    __syncthreads();
    if (t < 8) {
        int v = 0;
#pragma unroll
        for (int x = 0; x < 16; ++x) v += red[8 * x + t];
        if (t != 3) o_ct[t == 0 ? 1 : t < 3 ? t + 1 : t] = v;          // {sounding, pauses, pause frames, -, candidates, nuclei, leading, trailing}
        const long long np = __shfl(v, 1, 64), S1 = __shfl(v, 2, 64), S2 = __shfl(v, 3, 64);
        if (t == 0) {
            o_ct[0] = nf;
            o_st[0] = ref; o_st[1] = thr;
            o_st[2] = np ? (double)S1 / (double)np : 0.0;
            o_st[3] = np ? sqrt((double)(np * S2 - S1 * S1)) / (double)np : 0.0;
        }
    }
}

// ---------------------------------------------------------------------------
// Spectral envelope and mel-cepstrum (ev_envelope): CheapTrick's f0-adaptive envelope (Morise 2015) and its frequency-warped cepstrum (SPTK's
// freqt) on ev_voice_quality's frames, the period of every frame from ev_pitch_yin (the definition, steps 1 to 7: include/emojivoice.h).  All
// float64, contraction OFF (STOI_EXACT), no atomics, no scratch.  Two launches on the grid (ceil(NF / 16), B), a workgroup of 4 waves per tile of 16
// frames, four GEMMs on v_mfma_f64_16x16x4_f64 with the fragment layout of the float64 DFT GEMM above:
//   envelope_power_kernel     GEMM 1  the windowed, mean-removed frames (16 x K, float64 in LDS) times the PLAIN DFT basis {cos, sin}(2 pi m k / nfft)
//                                     (stft_dist_basis_kernel with a window of ones and W = nfft): sample j of a frame stands at row m = j + nfft / 2
//                                     (the shift is a sign per bin: |X|^2 does not see it).  The window differs per frame, so it is applied to the
//                                     A operand, not baked into the basis, and K runs over the tile's LONGEST window only: rows m_lo <= m < m_hi,
//                                     m_lo = (nfft / 2 - hmax) rounded down and m_hi = nfft / 2 + hmax + 1 rounded up to a multiple of 4, shorter
//                                     windows padded with zeros.  P = fma(sm, sm, re re) goes to the handle's arena (B, NF, NB).
//   envelope_cepstrum_kernel  steps 3 and 4 per frame in LDS; GEMM 2: Lg (16 x NBp) times voiceq_cep_basis_kernel's table at q_fit = 0, NQ = NB,
//                                     the lifter in its epilogue; GEMM 3a: the liftered cepstrum times the SAME table (g[q] cos(2 pi q k / nfft) is
//                                     nfft cep[q][k]), skipped without d_env; GEMM 3b: the liftered cepstrum times the warp table (NBp, n_mcep).
// A tile holds frames of ONE row and everything in it hangs on that row's samples below len and its own periods: a row's outputs do not depend on
// the batch or on L (m_lo and m_hi follow the row's own periods; a product with a padding zero adds +0).
// ORDERS.  Window sums (sum w^2, sum w, sum x w): wave v owns the frames 4 v .. 4 v + 3; lane l adds its samples i = l, l + 64, ... (i = j + half)
// in ascending order, then one xor tree over the 64 lanes (offsets 32 .. 1).  live (the count of P[k] > floor): the same, over bins.  The
// smoothing sum: one lane per (frame, bin), ascending cells.  GEMMs: K ascending in steps of 4 inside the matrix instruction.
struct EnvTables {
    const double2* basis; const double* cep; const double* warp;       // (nfft, NB) pairs, (NBp, NB), (NBp, n_mcep) with zero rows from NB on
    int H, nfft, NB, NBp, S1, S, n_mcep;                                // S1, S: the LDS row strides of the frames and of the planes, both 2 mod 32
    double T_max, T_def, q1;
};

// the period of frame idx of the row and its class (0: ev_pitch_yin's, 1: the default period)
__device__ __forceinline__ double env_period(const float* pr, size_t idx, const EnvTables& t, int* cls) {
    const double T = (double)pr[idx];
    const bool ok = T > 0.0 && T >= 2.0 && T <= t.T_max;                // (a NaN is not > 0)
    *cls = ok ? 0 : 1;
    return ok ? T : t.T_def;
}
__device__ __forceinline__ int env_half(double T) { STOI_EXACT return (int)floor(1.5 * T + 0.5); }
__device__ __forceinline__ double env_wave_sum(double v) {
    STOI_EXACT
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

// Dynamic LDS: the tile's frames, 16 x S1 doubles (S1 the smallest number >= nfft rounded up to 4 that is 2 mod 32: 131 328 bytes at nfft = 1024).
// The samples come straight from the row (each is read by about (2 half + 1) / H frames: cache hits), zeros outside [0, len).
// BANKS.  The window passes write and read ws[m] with m consecutive over the 64 lanes (ds_write_b64 / ds_read_b64: consecutive doubles,
// conflict-free).  The A fragment of GEMM 1 reads frames[(l & 15) S1 + m_lo + 4 s + (l >> 4)] with ds_read_b64: voice_quality_kernel's phase 2
// pattern with the same stride class (S1 = 2 mod 32, m_lo a constant offset): all 64 banks once per group of 32 lanes, conflict-free.
struct EnvPowerParams { const float* x; const int32_t* len; const float* period; double* P; EnvTables t; int L, NF; };

__global__ __launch_bounds__(256) void envelope_power_kernel(const EnvPowerParams p) {
    STOI_EXACT
    extern __shared__ __attribute__((aligned(16))) double env_smem[];
    const int b = blockIdx.y, f0 = blockIdx.x * 16, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int H = p.t.H, nfft = p.t.nfft, NB = p.t.NB, S1 = p.t.S1, hn = nfft >> 1;
    int n;
    const int nf = voiceq_frames(p.len, b, p.L, H, &n);
    if (f0 >= nf) return;                                               // (uniform) envelope_cepstrum_kernel writes this tile's zeros and reads no P
    const float* xr = p.x + (size_t)b * p.L;
    const float* pr = p.period + (size_t)b * p.NF;
    int hmax = 0;                                                       // the tile's longest window (uniform: every thread walks the 16 periods)
    for (int fr = 0; fr < 16 && f0 + fr < nf; ++fr) {
        int c;
        const int hf = env_half(env_period(pr, (size_t)(f0 + fr), p.t, &c));
        hmax = hf > hmax ? hf : hmax;
    }
    const int m_lo = (hn - hmax) & ~3, m_hi = (hn + hmax + 4) & ~3;     // (hmax <= nfft / 2 - 1: 0 <= m_lo, m_hi <= nfft rounded up to 4 <= S1)
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
        const int fr = 4 * wv + i;
        double* ws = env_smem + (size_t)fr * S1;
        int half = -1;                                                  // (a frame past the row: zeros throughout)
        if (f0 + fr < nf) {
            int c;
            const double T = env_period(pr, (size_t)(f0 + fr), p.t, &c);
            const double a = 1.5 * T;
            half = env_half(T);
            const long long ctr = (long long)(f0 + fr) * H + H / 2;
            double sw2 = 0.0, sw = 0.0, sxw = 0.0;
            for (int ii = lane; ii <= 2 * half; ii += 64) {
                const int j = ii - half;
                const double w = 0.5 * cospi((double)j / a) + 0.5;
                const long long s = ctr + j;
                const double xv = s >= 0 && s < n ? (double)xr[s] : 0.0;
                const double xw = xv * w;
                ws[hn + j] = xw;
                sw2 = sw2 + w * w; sw = sw + w; sxw = sxw + xw;
            }
            sw2 = env_wave_sum(sw2); sw = env_wave_sum(sw); sxw = env_wave_sum(sxw);
            const double nrm = sqrt(sw2), ratio = sxw / sw;             // s[j] = (x w - w (sum x w) / (sum w)) / sqrt(sum w^2)
            for (int ii = lane; ii <= 2 * half; ii += 64) {             // (each lane returns to the entries it wrote itself)
                const int j = ii - half;
                const double w = 0.5 * cospi((double)j / a) + 0.5;
                ws[hn + j] = (ws[hn + j] - w * ratio) / nrm;
            }
        }
        for (int m = m_lo + lane; m < m_hi; m += 64)
            if (m < hn - half || m > hn + half) ws[m] = 0.0;
    }
    __syncthreads();
    const int r = lane & 15, q = lane >> 4;
    const int ntile = (NB + 15) >> 4, nsteps = (m_hi - m_lo) >> 2;      // (nsteps >= 1)
    const double* La = env_smem + (size_t)r * S1 + m_lo + q;
    double* Pt = p.P + ((size_t)b * p.NF + f0) * NB;
    for (int bt = wv; bt < ntile; bt += 4) {
        const int col = bt * 16 + r;
        const double2* bp = p.t.basis + (col < NB ? col : NB - 1);
        stftd_acc xc = {0.0, 0.0, 0.0, 0.0}, xs = xc;
        // the basis row of step s is m_lo + 4 s + q, clamped to nfft - 1 (nfft no multiple of 4: the frames hold zeros there); the rows of the NEXT
        // four steps are requested before this round's products, the step clamped at the last one, as in the kernels above
        double2 cur[4], nxt[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int m = m_lo + 4 * (u < nsteps ? u : nsteps - 1) + q;
            cur[u] = bp[(size_t)(m < nfft ? m : nfft - 1) * NB];
        }
        for (int s0 = 0; s0 < nsteps; s0 += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int m = m_lo + 4 * (s0 + 4 + u < nsteps ? s0 + 4 + u : nsteps - 1) + q;
                nxt[u] = bp[(size_t)(m < nfft ? m : nfft - 1) * NB];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (s0 + u < nsteps) {                                  // (uniform)
                    const double ax = La[4 * (s0 + u)];
                    xc = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, cur[u].x, xc, 0, 0, 0);
                    xs = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, cur[u].y, xs, 0, 0, 0);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
        }
        if (col < NB) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (f0 + q + 4 * i < nf) Pt[(size_t)(q + 4 * i) * NB + col] = fma(xs[i], xs[i], xc[i] * xc[i]);
        }
    }
}

// One GEMM of envelope_cepstrum_kernel: C (16 frames x ncol) = plane (16 x NBp, LDS, row stride S) times tab (NBp x ncol, row-major, its rows from
// NB on zeros), wave w owning the column tiles w, w + 4, ...; voice_quality_kernel's phase 2 loop.  La is the plane at the lane's row, (l & 15) S;
// k >= NB reads the address NB - 1 (the table's row is zero).  epi(col, c) takes the finished tile: register i of c is frame (l >> 4) + 4 i.
template <typename Epi>
__device__ __forceinline__ void env_gemm(const double* La, const double* tab, int ncol, int NB, int NBp, int wv, int r, int q, Epi epi) {
    STOI_EXACT
    const int nt = (ncol + 15) >> 4, nsteps = NBp >> 2;
    for (int ct = wv; ct < nt; ct += 4) {
        const int col = ct * 16 + r;
        const double* bp = tab + (size_t)q * ncol + (col < ncol ? col : ncol - 1);
        stftd_acc c = {0.0, 0.0, 0.0, 0.0};
        double cur[4], nxt[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) cur[u] = bp[(size_t)(u < nsteps ? u : nsteps - 1) * 4 * ncol];
        for (int t0 = 0; t0 < nsteps; t0 += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) nxt[u] = bp[(size_t)(t0 + 4 + u < nsteps ? t0 + 4 + u : nsteps - 1) * 4 * ncol];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (t0 + u < nsteps) {                                  // (uniform)
                    const int k = 4 * (t0 + u) + q;
                    c = __builtin_amdgcn_mfma_f64_16x16x4f64(La[k < NB ? k : NB - 1], cur[u], c, 0, 0, 0);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
        }
        if (col < ncol) epi(col, c);
    }
}

// Dynamic LDS: two planes X and Y of 16 x S doubles (S the smallest number >= NBp that is 2 mod 32: 131 584 bytes at nfft = 1024).  Wave v owns
// the frames 4 v .. 4 v + 3 in the passes per frame, lane l the bins l, l + 64, ...; a barrier stands between any two passes.
//   pass 1  X[k] = P[k] from the arena; live = the count of P[k] > floor; the frame's T, class, half and kd; d_class
//   pass 2  Y[k] = P'[k]: for k <= kd, u = nfft / T - k, i = floor(u), P[k] + (P[i] (1 - (u - i)) + P[min(i + 1, NB - 1)] (u - i)), read from X
//   pass 3  X[k] = log(max(S[k], floor)), S[k] = (sum over the cells of [k - wd / 2, k + wd / 2) of Y) / wd, wd = (2 nfft) / (3 T): with lo and hi
//           the ends, ilo = floor(lo + 0.5), ihi = floor(hi + 0.5): ilo == ihi: Y[ilo] (hi - lo); else Y[ilo] ((ilo + 0.5) - lo), then Y[i] for
//           ilo < i < ihi ascending, then Y[ihi] (hi - (ihi - 0.5)); an index i < 0 reads -i, one > nfft / 2 reads nfft - i (wd <= nfft / 3: once)
//   GEMM 2  Y[q] = (c sinc) comp, c = (X times cep)[q], sinc = sinpi(q / T) / (pi (q / T)) (1 at q = 0), comp = (1 - 2 q1) + (2 q1) cospi(2 (q / T))
//   GEMM 3a d_env[k] = nfft (Y times cep)[k];  GEMM 3b d_mcep[m] = (Y times warp)[m].  Zeros for a silent frame (live = 0) and past the row.
// BANKS.  Passes 1 to 3 touch a plane at consecutive doubles over the 64 lanes, pass 2's interpolation at consecutive doubles descending and pass 3's
// cells at a common offset from consecutive bins (mirrored: descending): conflict-free but where a mirror folds a group onto itself (2-way, at the
// two ends of the spectrum only).  The A fragments of the three GEMMs are voice_quality_kernel's phase 2 reads (S = 2 mod 32): conflict-free.
// GEMM 2's epilogue stores Y[(q + 4 i) S + col] once per quefrency tile: 16 consecutive doubles per frame, the two frames of a group of 32 lanes
// 2 S = 4 mod 64 dwords apart, so their spans overlap on 28 banks: 2-way, as voice_quality_kernel's stores of Ldb, and as rare.
struct EnvCepParams { const int32_t* len; const float* period; const double* P; double* env; double* mcep; int32_t* cls; EnvTables t; int L, NF; double floor; };

__global__ __launch_bounds__(256) void envelope_cepstrum_kernel(const EnvCepParams p) {
    STOI_EXACT
    extern __shared__ __attribute__((aligned(16))) double env_smem[];
    __shared__ double Ts[16];
    __shared__ int keep_s[16];
    const int b = blockIdx.y, f0 = blockIdx.x * 16, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int H = p.t.H, nfft = p.t.nfft, NB = p.t.NB, NBp = p.t.NBp, S = p.t.S, NM = p.t.n_mcep, hn = nfft >> 1;
    int n;
    const int nf = voiceq_frames(p.len, b, p.L, H, &n);
    const int nfr = p.NF - f0 < 16 ? p.NF - f0 : 16;                    // the tile's frames inside the outputs (>= 1)
    int32_t* ck = p.cls + ((size_t)b * p.NF + f0) * 3;
    double* ev = p.env ? p.env + ((size_t)b * p.NF + f0) * NB : nullptr;
    double* mc = p.mcep + ((size_t)b * p.NF + f0) * NM;
    if (f0 >= nf) {                                                     // (uniform) zeros past the row's own frames, class 3
        if (tid < 3 * nfr) ck[tid] = tid % 3 == 0 ? 3 : 0;
        for (int i = tid; i < nfr * NM; i += 256) mc[i] = 0.0;
        if (ev) for (int i = tid; i < nfr * NB; i += 256) ev[i] = 0.0;
        return;
    }
    double* X = env_smem;
    double* Y = env_smem + (size_t)16 * S;
    const float* pr = p.period + (size_t)b * p.NF;
    double T[4], rn[4];                                                 // of the wave's own frames: the period and nfft / T
    int kd[4];
    // ---- pass 1
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int fr = 4 * wv + i;
        const bool in = f0 + fr < nf;
        double* xa = X + (size_t)fr * S;
        int cls = 3, live = 0, half = 0;
        T[i] = p.t.T_def;
        if (in) {
            T[i] = env_period(pr, (size_t)(f0 + fr), p.t, &cls);
            half = env_half(T[i]);
            const double* Pg = p.P + ((size_t)b * p.NF + f0 + fr) * NB;
            for (int k = lane; k < NB; k += 64) { const double v = Pg[k]; xa[k] = v; live += v > p.floor ? 1 : 0; }
        } else {
            for (int k = lane; k < NB; k += 64) xa[k] = 0.0;
        }
        rn[i] = (double)nfft / T[i];
        kd[i] = in ? (int)floor(rn[i]) : -1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) live += __shfl_xor(live, o, 64);
        if (lane == 0) {
            Ts[fr] = T[i];
            keep_s[fr] = in && live > 0 ? 1 : 0;
            if (fr < nfr) { ck[3 * fr] = in ? (live > 0 ? cls : 2) : 3; ck[3 * fr + 1] = half; ck[3 * fr + 2] = in ? kd[i] : 0; }
        }
    }
    __syncthreads();
    // ---- pass 2
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int fr = 4 * wv + i;
        const double* xa = X + (size_t)fr * S;
        double* ya = Y + (size_t)fr * S;
        for (int k = lane; k < NB; k += 64) {
            double v = xa[k];
            if (k <= kd[i]) {
                const double u = rn[i] - (double)k;
                const int i0 = (int)floor(u);
                const double fu = u - (double)i0;
                const int i1 = i0 + 1 < NB - 1 ? i0 + 1 : NB - 1;
                v = v + (xa[i0] * (1.0 - fu) + xa[i1] * fu);
            }
            ya[k] = v;
        }
    }
    __syncthreads();
    // ---- pass 3
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
        const int fr = 4 * wv + i;
        double* xa = X + (size_t)fr * S;
        const double* ya = Y + (size_t)fr * S;
        const double wd = (2.0 * (double)nfft) / (3.0 * Ts[fr]), hw = 0.5 * wd;
        for (int k = lane; k < NB; k += 64) {
            const double lo = (double)k - hw, hi = (double)k + hw;
            const int ilo = (int)floor(lo + 0.5), ihi = (int)floor(hi + 0.5);
            const int alo = ilo < 0 ? -ilo : ilo > hn ? nfft - ilo : ilo;
            double acc;
            if (ilo == ihi) acc = ya[alo] * (hi - lo);
            else {
                acc = ya[alo] * (((double)ilo + 0.5) - lo);
                for (int c = ilo + 1; c < ihi; ++c) acc = acc + ya[c < 0 ? -c : c > hn ? nfft - c : c];
                acc = acc + ya[ihi < 0 ? -ihi : ihi > hn ? nfft - ihi : ihi] * (hi - ((double)ihi - 0.5));
            }
            xa[k] = log(fmax(acc / wd, p.floor));
        }
    }
    __syncthreads();
    const int r = lane & 15, q = lane >> 4;
    // ---- GEMM 2 and the lifter
    {
        const double q1 = p.t.q1, c0 = 1.0 - 2.0 * q1, c1 = 2.0 * q1;
        env_gemm(X + (size_t)r * S, p.t.cep, NB, NB, NBp, wv, r, q, [&](int col, const stftd_acc& c) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int fr = q + 4 * i;
                const double x = (double)col / Ts[fr];
                const double sinc = col == 0 ? 1.0 : sinpi(x) / (3.141592653589793 * x);
                const double comp = c0 + c1 * cospi(2.0 * x);
                Y[(size_t)fr * S + col] = (c[i] * sinc) * comp;
            }
        });
    }
    __syncthreads();
    // ---- GEMM 3a and 3b
    if (ev) {
        const double dn = (double)nfft;
        env_gemm(Y + (size_t)r * S, p.t.cep, NB, NB, NBp, wv, r, q, [&](int col, const stftd_acc& c) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int fr = q + 4 * i;
                if (fr < nfr) ev[(size_t)fr * NB + col] = keep_s[fr] ? dn * c[i] : 0.0;
            }
        });
    }
    env_gemm(Y + (size_t)r * S, p.t.warp, NM, NB, NBp, wv, r, q, [&](int col, const stftd_acc& c) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int fr = q + 4 * i;
            if (fr < nfr) mc[(size_t)fr * NM + col] = keep_s[fr] ? c[i] : 0.0;
        }
    });
}

// ---------------------------------------------------------------------------
// Phase vocoder (ev_phase_vocoder): time stretching of every row by librosa's stft -> phase_vocoder -> istft chain (the definition, with every
// order: include/emojivoice.h; tests/phase_vocoder_ref.py restates it).  W = nfft, H = nfft / 4, NB = nfft / 2 + 1.  All float64, contraction OFF
// (STOI_EXACT), no atomics.  Launches of a call:
//   1. pv_analysis_kernel:  one workgroup of 4 waves per (row, 16 frames from the row's frame 0): the DFT GEMM of stft_dist_frames_kernel for one
//      signal on the windowed basis (stft_dist_basis_kernel builds it) -> mag, ang (B, NF, NB), bins fast.  Frames at and behind nf are not
//      stored: the definition's two zero frames behind nf - 1 are what pv_propagate_kernel takes for every frame >= nf.
//   2. pv_propagate_kernel: one thread per (row, bin) walks t = 0 .. n_out - 1 -> Y (B, NO, NB) pairs {re, im}, zeros from n_out on.
//   3. pv_synthesis_kernel: the inverse DFT as a GEMM, frames x bins times inv[k][.] = {c_k cos, -c_k sin}(2 pi j k / nfft) (pv_inv_basis_kernel
//      builds it: exact multiples of the twiddles, zero rows from NB on, zero sine entries at DC and Nyquist), the window, the overlap-add in
//      ascending frame order and the division by the window's sum of squares formed in the same order -> d_y.
// Everything a row's outputs depend on hangs on the row's own samples below len.
struct PvTables { const double2* basis; const double2* inv; const double* wn; const double* wsq; int nfft, H, NB, NBp, skew; };
#define PV_TWO_PI 6.283185307179586

// (n, nf) of row b: a row with len < 1 or len > L is an empty row
__device__ __forceinline__ int pv_frames(const int32_t* len, int b, int L, int H, int* n_out) {
    int n = len ? len[b] : L;
    if (n < 1 || n > L) n = 0;
    *n_out = n;
    return n > 0 ? 1 + n / H : 0;
}
// ceil(nf / rate): the output frames of nf input frames (host: NO from NF by the same expression, so n_out <= NO)
__host__ __device__ __forceinline__ int pv_steps(int nf, double rate) { return nf > 0 ? (int)ceil((double)nf / rate) : 0; }
__device__ __forceinline__ int pv_out_len(int n, double rate) { return n > 0 ? (int)rint((double)n / rate) : 0; }

// inv (NBp, nfft) in the column order of pv_synthesis_kernel: column 16 tile + c holds sample j = (c >> 2) H + 4 tile + (c & 3)
struct PvInvParams { const double* tw; double2* inv; int nfft, H, NB, NBp; };

__global__ __launch_bounds__(256) void pv_inv_basis_kernel(const PvInvParams p) {
    const int i = blockIdx.x * 256 + threadIdx.x;                       // (NBp nfft <= 1028 x 2048)
    if (i >= p.NBp * p.nfft) return;
    const int k = i / p.nfft, col = i - k * p.nfft, c = col & 15;
    const int j = (c >> 2) * p.H + 4 * (col >> 4) + (c & 3);
    double2 v = make_double2(0.0, 0.0);
    if (k < p.NB) {
        const int ph = (j * k) % p.nfft;                                // (< 2048 x 1024: exact)
        const bool edge = k == 0 || k == p.NB - 1;                      // irfft: the imaginary parts of DC and Nyquist are ignored
        v = edge ? make_double2(p.tw[2 * ph], 0.0) : make_double2(2.0 * p.tw[2 * ph], -2.0 * p.tw[2 * ph + 1]);
    }
    p.inv[i] = v;
}

// The K loop of one bin tile for ONE signal: stft_dist_frames_kernel's loop (four steps a round, the basis of the next round requested before
// this round's products) with the cos and sin planes of a single staged signal.
__device__ __forceinline__ void dft_tile_planes(const float* sx, DftSkewWalk& walk, const double2* bp, int NB, int nsteps, int q, stftd_acc& xc, stftd_acc& xs) {
    walk.start(q);
    double2 cur[4], nxt[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) cur[u] = bp[(size_t)(u < nsteps ? u : nsteps - 1) * 4 * NB];
    for (int s0 = 0; s0 < nsteps; s0 += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) nxt[u] = bp[(size_t)(s0 + 4 + u < nsteps ? s0 + 4 + u : nsteps - 1) * 4 * NB];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (s0 + u < nsteps) {                                      // (uniform)
                const double ax = (double)sx[walk.word()];
                xc = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, cur[u].x, xc, 0, 0, 0);
                xs = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, cur[u].y, xs, 0, 0, 0);
                walk.step();
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
    }
}

// One workgroup per (row b, tile of 16 frames f0 .. f0 + 15).  The tile's raw span, samples f0 H - nfft / 2 + t for 0 <= t < 15 H + nfft, is staged
// once as fp32 with the skew, zeros outside [0, n): 39 KB at nfft = 2048.  Epilogue per (frame < nf, bin < NB): re = sum cos, im = -sum sin,
// mag = sqrt(fma(im, im, re re)), ang = atan2(im, re).
struct PvAnalysisParams { const float* x; const int32_t* len; double* mag; double* ang; PvTables t; int L, NF; };

__global__ __launch_bounds__(256) void pv_analysis_kernel(const PvAnalysisParams p) {
    STOI_EXACT
    extern __shared__ __attribute__((aligned(16))) float pv_smem[];
    const int b = blockIdx.y, f0 = blockIdx.x * 16, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int W = p.t.nfft, H = p.t.H, NB = p.t.NB, skew = p.t.skew;
    int n;
    const int nf = pv_frames(p.len, b, p.L, H, &n);
    if (f0 >= nf) return;                                               // (uniform)
    const int span = 15 * H + W;
    {
        const float* xr = p.x + (size_t)b * p.L;
        const long long i0 = (long long)f0 * H - W / 2;
        for (int t = tid; t < span; t += 256) {
            const long long i = i0 + t;
            pv_smem[dft_word(t, H, skew)] = i >= 0 && i < n ? xr[i] : 0.f;
        }
    }
    __syncthreads();
    const int r = lane & 15, q = lane >> 4;
    const int ntile = (NB + 15) >> 4, nsteps = W >> 2;
    DftSkewWalk walk(r, H, skew);
    for (int bt = wv; bt < ntile; bt += 4) {
        const int col = bt * 16 + r;
        const double2* bp = p.t.basis + (size_t)q * NB + (col < NB ? col : NB - 1);
        stftd_acc xc = {0.0, 0.0, 0.0, 0.0}, xs = xc;
        dft_tile_planes(pv_smem, walk, bp, NB, nsteps, q, xc, xs);
        if (col < NB) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int fr = f0 + q + 4 * i;
                if (fr < nf) {
                    const double re = xc[i], im = -xs[i];
                    const size_t o = ((size_t)b * p.NF + fr) * NB + col;
                    p.mag[o] = sqrt(fma(im, im, re * re));
                    p.ang[o] = atan2(im, re);
                }
            }
        }
    }
}

// One thread per (row b, bin k), 64 bins a workgroup: the loads of a step do not depend on the phase, so those of step t + 1 are issued before
// step t's sine and cosine; the loads and the stores are coalesced over the bins.  Thread k = 0 also writes the row's out_len and counts.
struct PvPropParams { const double* mag; const double* ang; const int32_t* len; double2* Y; int32_t* out_len; int32_t* counts; PvTables t; int L, NF, NO; double rate; };

__global__ __launch_bounds__(64) void pv_propagate_kernel(const PvPropParams p) {
    STOI_EXACT
    const int b = blockIdx.y, k = blockIdx.x * 64 + threadIdx.x;
    const int NB = p.t.NB;
    int n;
    const int nf = pv_frames(p.len, b, p.L, p.t.H, &n);
    const int n_out = pv_steps(nf, p.rate);
    if (k == 0) {
        p.out_len[b] = pv_out_len(n, p.rate);
        if (p.counts) { p.counts[2 * b] = nf; p.counts[2 * b + 1] = n_out; }
    }
    if (k >= NB) return;
    const double* mg = p.mag + (size_t)b * p.NF * NB + k;
    const double* ag = p.ang + (size_t)b * p.NF * NB + k;
    double2* y = p.Y + (size_t)b * p.NO * NB + k;
    const double omega = (PV_TWO_PI * (double)(p.t.H * k)) / (double)p.t.nfft;
    // frames >= nf are the definition's zero frames (nothing is stored for them)
    int i = 0;
    double al = 0.0;
    double m0 = 0.0, m1 = 0.0, a0 = 0.0, a1 = 0.0;
    if (n_out > 0) {
        m0 = mg[0]; a0 = ag[0];
        if (1 < nf) { m1 = mg[(size_t)NB]; a1 = ag[(size_t)NB]; }
    }
    double phi = a0;
    for (int t = 0; t < n_out; ++t) {
        int in = i; double aln = 0.0, n0 = 0.0, n1 = 0.0, b0 = 0.0, b1 = 0.0;
        if (t + 1 < n_out) {
            const double s = (double)(t + 1) * p.rate;
            const double fl = floor(s);
            in = (int)fl; aln = s - fl;
            if (in < nf) { n0 = mg[(size_t)in * NB]; b0 = ag[(size_t)in * NB]; }
            if (in + 1 < nf) { n1 = mg[(size_t)(in + 1) * NB]; b1 = ag[(size_t)(in + 1) * NB]; }
        }
        const double m = (1.0 - al) * m0 + al * m1;
        y[(size_t)t * NB] = make_double2(m * cos(phi), m * sin(phi));
        double d = a1 - a0 - omega;
        d = d - PV_TWO_PI * rint(d / PV_TWO_PI);
        phi = phi + (omega + d);
        i = in; al = aln; m0 = n0; m1 = n1; a0 = b0; a1 = b1;
    }
    for (int t = n_out; t < p.NO; ++t) y[(size_t)t * NB] = make_double2(0.0, 0.0);
}

// One workgroup of 4 waves per (row b, group g): the 16 output frames t0 .. t0 + 15 with t0 = 13 g - 3, and the 13 hop segments s = 13 g ..
// 13 g + 12 (padded samples s H .. s H + H - 1) that these frames cover completely: segment s takes frame s - q at its quarter q = 3, 2, 1, 0,
// i.e. in ascending frame order.  Wave w owns the column tiles w, w + 4, ... of nfft / 16; tile c holds, for the four offsets m = 4 c .. 4 c + 3
// inside a hop, the four quarters j = q H + m, so every term of 13 x 4 output samples lies in the wave's own accumulators.  They cross through a
// 16 x 16 exchange in LDS (8.5 KB for the four waves, whatever nfft is), after the window: ex[frame][column] = wn[j] (acc_cos + acc_sin).  Lane
// (sl, mm) < 52 then adds the frames that exist (0 <= t < n_out) and the squares of the window in the same order, divides where the sum of
// squares is above FLT_MIN, rounds once to fp32 and stores; outside [0, min(out_len, H (n_out - 1) + nfft / 2)) it stores zeros, so that every
// sample of d_y's row is written exactly once per call.  A lane of an A fragment reads Y[t0 + (l & 15)][k0 + (l >> 4)] from global memory (frames
// outside [0, n_out) and bins >= NB: the address clamped, the value zero), a B fragment inv[k0 + (l >> 4)][16 tile + (l & 15)].
struct PvSynthParams { const double2* Y; const int32_t* len; float* y; PvTables t; int L, NO, L_out; double rate; };

__global__ __launch_bounds__(256) void pv_synthesis_kernel(const PvSynthParams p) {
    STOI_EXACT
    __shared__ double ex[4][16][17];
    const int b = blockIdx.y, g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nfft = p.t.nfft, H = p.t.H, NB = p.t.NB;
    int n;
    const int nf = pv_frames(p.len, b, p.L, H, &n);
    const int n_out = pv_steps(nf, p.rate);
    long long lim = 0;
    if (n_out > 0) {
        lim = (long long)H * (n_out - 1) + nfft / 2;
        const long long ol = pv_out_len(n, p.rate);
        if (ol < lim) lim = ol;
    }
    if (lim > p.L_out) lim = p.L_out;
    float* yr = p.y + (size_t)b * p.L_out;
    const long long i_first = (long long)13 * g * H - nfft / 2;         // the block's samples: i_first <= i < i_first + 13 H
    if (i_first >= lim) {                                               // (uniform) zeros behind the row's own output
        for (int u = tid; u < 13 * H; u += 256) {
            const long long i = i_first + u;
            if (i >= 0 && i < p.L_out) yr[i] = 0.f;
        }
        return;
    }
    const int r = lane & 15, q = lane >> 4;
    const int t0 = 13 * g - 3, ta = t0 + r;
    const bool live = ta >= 0 && ta < n_out;
    const double2* arow = p.Y + ((size_t)b * p.NO + (live ? ta : 0)) * NB;
    const int ntile = nfft >> 4, nsteps = p.t.NBp >> 2;
    const int sl = lane >> 2, mm = lane & 3;
    for (int c0 = 0; c0 < ntile; c0 += 4) {                             // (uniform: every wave meets both barriers)
        const int ct = c0 + wv;
        if (ct < ntile) {
            const double2* bp = p.t.inv + (size_t)q * nfft + ct * 16 + r;
            stftd_acc ac = {0.0, 0.0, 0.0, 0.0}, as = ac;
            double2 ca[4], cb[4], na[4], nb[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int s = u < nsteps ? u : nsteps - 1, k = 4 * s + q;
                ca[u] = arow[k < NB ? k : NB - 1];
                cb[u] = bp[(size_t)s * 4 * nfft];
            }
            for (int s0 = 0; s0 < nsteps; s0 += 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int s = s0 + 4 + u < nsteps ? s0 + 4 + u : nsteps - 1, k = 4 * s + q;
                    na[u] = arow[k < NB ? k : NB - 1];
                    nb[u] = bp[(size_t)s * 4 * nfft];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (s0 + u < nsteps) {                              // (uniform)
                        const bool ok = live && 4 * (s0 + u) + q < NB;
                        const double are = ok ? ca[u].x : 0.0, aim = ok ? ca[u].y : 0.0;
                        ac = __builtin_amdgcn_mfma_f64_16x16x4f64(are, cb[u].x, ac, 0, 0, 0);
                        as = __builtin_amdgcn_mfma_f64_16x16x4f64(aim, cb[u].y, as, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) { ca[u] = na[u]; cb[u] = nb[u]; }
            }
            const double wj = p.t.wn[(r >> 2) * H + 4 * ct + (r & 3)];
#pragma unroll
            for (int i = 0; i < 4; ++i) ex[wv][q + 4 * i][r] = wj * (ac[i] + as[i]);
        }
        __syncthreads();
        if (ct < ntile && lane < 52) {
            const int m = 4 * ct + mm, s = 13 * g + sl;
            double num = 0.0, wss = 0.0;
#pragma unroll
            for (int qt = 3; qt >= 0; --qt) {
                const int t = s - qt;
                if (t >= 0 && t < n_out) { num = num + ex[wv][sl + 3 - qt][4 * qt + mm]; wss = wss + p.t.wsq[qt * H + m]; }
            }
            const double v = wss > 1.1754943508222875e-38 ? num / wss : num;
            const long long i = (long long)s * H + m - nfft / 2;
            if (i >= 0 && i < p.L_out) yr[i] = i < lim ? (float)v : 0.f;
        }
        __syncthreads();
    }
}
