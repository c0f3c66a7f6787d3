/*
 * emojivoice.h — C ABI of the MI355X-native EmojiVoice TTS hot path.
 *
 * The reference (rosielab/emojivoice, vendored Matcha-TTS) is pure Python on
 * stock torch ops; it has no FFI of its own.  The entry points below are what a
 * binding for its hot path replaces (paths relative to Matcha-TTS/matcha/):
 *
 *   ev_cfm_decode   <-  BASECFM.forward / solve_euler      models/components/flow_matching.py:32-85
 *                       driving Decoder.forward            models/components/decoder.py:363-443
 *                       (BasicTransformerBlock             models/components/transformer.py:243-316,
 *                        diffusers Attention, SnakeBeta    transformer.py:17-80)
 *   ev_hifigan      <-  Generator.forward                  hifigan/models.py:181-197
 *                       (ResBlock1.forward                 hifigan/models.py:90-97,
 *                        ResBlock2.forward                 hifigan/models.py:106-145: x = x + c_d(lrelu(x)) for two dilations,
 *                        keys resblocks.N.convs.{0,1}.{weight,bias})
 *   ev_text_encoder <-  TextEncoder.forward                models/components/text_encoder.py:378-410
 *                       (ConvReluNorm :36-67, Encoder :276-325, MultiHeadAttention + RoPE :97-246, FFN :255-273,
 *                        DurationPredictor :70-94, channel LayerNorm :15-33) — the caller of the hot path
 *   ev_load_estimator <- MatchaTTS.load_from_checkpoint -> state_dict["decoder.estimator.*"]   cli.py:110-118
 *   ev_load_text_encoder <- same checkpoint, state_dict["encoder.*"] + the derived "rope_theta" table
 *   ev_load_vocoder   <- Generator.load_state_dict(ckpt["generator"]) + remove_weight_norm()   cli.py:84-90
 *   ev_load_vocoder_cfg <- the same for the Generator(h) of any HiFi-GAN config inside the supported envelope (V1, V2, V3 ...)
 *   ev_mel_spectrogram <- mel_spectrogram(y, 1024, num_mels, sr, 256, 1024, fmin, fmax, center=False)   utils/audio.py:45-82
 *                       (the same function again in hifigan/meldataset.py:52), optionally with normalize() of utils/model.py fused
 *   ev_load_mel_basis  <- the librosa mel filter bank that function caches per (fmax, device)
 *   ev_log_prior       <- the log-likelihood matrix of MatchaTTS.forward                         models/matcha_tts.py:186-193
 *   ev_maximum_path    <- monotonic_align.maximum_path (maximum_path_c / maximum_path_each)      utils/monotonic_align/{__init__.py,core.pyx}
 *   ev_mas_align       <- both, plus attn.sum(-1) and mu_y = attn^T mu_x                          models/matcha_tts.py:186-199, :226-228
 *   ev_estimator_rows  <- Decoder.forward with t of shape (B,)                                    models/components/decoder.py:363-443
 *   ev_cfm_loss        <- BASECFM.compute_loss (one time per utterance) + the prior loss's sum        models/components/flow_matching.py:87-118, models/matcha_tts.py:241-242
 *   ev_mel_stats       <- compute_data_statistics (sum x, sum x^2 per utterance)                  utils/generate_data_statistics.py:25-47
 *   ev_resample        <- no counterpart: the reference asks for 22050 Hz files (README.md:156: fine-tuning audio "must be 22050",
 *                       data/text_mel_datamodule.py:201 asserts it) while its own recorder writes 44.1 kHz ones (record_audio.py:31)
 *   ev_load_resampler  <- no counterpart (the filter of ev_resample)
 *   ev_trim_bounds     <- no counterpart: the recorder's takes begin and end on a key press (record_audio.py); librosa.effects.trim is the model
 *   ev_trim_apply      <- the gain is normalize(audio) * 0.95 of the vocoder's dataset code                hifigan/meldataset.py:152
 *   ev_pitch_yin       <- no counterpart: the reference never measures pitch; librosa.yin is the model
 *   ev_dtw             <- no counterpart: the reference never compares what it says with what was recorded; MCD-DTW evaluation is the model
 *   ev_loudness        <- no counterpart; ITU-R BS.1770-4 is the model
 *   ev_load_srmr       <- no counterpart; Falk, Zheng and Chan 2010 (SRMR) and Hohmann 2002 (complex gammatone) are the model
 *   ev_srmr            <- no counterpart; Falk, Zheng and Chan 2010 (SRMR) and Hohmann 2002 (complex gammatone) are the model
 *   ev_load_speech_rate <- no counterpart; De Jong and Wempe 2009 (syllable nuclei) is the model
 *   ev_speech_rate     <- no counterpart; De Jong and Wempe 2009 (syllable nuclei) is the model
 *   ev_load_envelope   <- no counterpart; Morise 2015 (CheapTrick) and SPTK's freqt are the model
 *   ev_envelope        <- no counterpart; Morise 2015 (CheapTrick) and SPTK's freqt are the model
 *   ev_load_phase_vocoder <- no counterpart; librosa.effects.time_stretch (stft -> phase_vocoder -> istft) is the model
 *   ev_phase_vocoder   <- no counterpart; librosa.effects.time_stretch (stft -> phase_vocoder -> istft) is the model
 *   ev_load_stoi       <- no counterpart; Taal et al. 2011 / Jensen and Taal 2016 are the model
 *   ev_stoi            <- no counterpart; Taal et al. 2011 / Jensen and Taal 2016 are the model
 *   ev_load_stft_dist  <- no counterpart; Yamamoto et al. 2020 (multi-resolution STFT loss) is the model
 *   ev_stft_dist       <- no counterpart; Yamamoto et al. 2020 (multi-resolution STFT loss) is the model
 *   ev_load_voice_quality <- no counterpart; Eyben et al. 2016 (eGeMAPS) and Hillenbrand et al. 1994 (CPP) are the model
 *   ev_voice_quality   <- no counterpart; Eyben et al. 2016 (eGeMAPS) and Hillenbrand et al. 1994 (CPP) are the model
 *   ev_load_formants   <- no counterpart; Burg 1975 (maximum-entropy linear prediction), Aberth 1973 / Ehrlich 1967 and Praat's formant analysis are the model
 *   ev_formants        <- no counterpart; Burg 1975 (maximum-entropy linear prediction), Aberth 1973 / Ehrlich 1967 and Praat's formant analysis are the model
 *   ev_formant_track   <- no counterpart; Praat's Formant: Track is the model
 *   ev_perturbation    <- no counterpart; Praat's voice report (jitter local / absolute / RAP, shimmer local / dB, cc harmonicity; Boersma 1993) is the model
 *   ev_load_harmonics  <- no counterpart; Eyben et al. 2016 and Hanson 1997 are the model
 *   ev_harmonics       <- no counterpart; Eyben et al. 2016 and Hanson 1997 are the model
 *   ev_functionals     <- no counterpart; the functionals of Eyben et al. 2016 (eGeMAPS) as openSMILE computes them are the model
 *   ev_modulation      <- no counterpart; the modulation spectrum (Takamichi et al. 2016 for cepstral trajectories) is the model
 *   ev_load_auditory   <- no counterpart; Eyben et al. 2016 (eGeMAPS) as openSMILE's cMelspec / cMfcc / cPlp / cSpectral compute them are the model
 *   ev_auditory        <- no counterpart; Eyben et al. 2016 (eGeMAPS) as openSMILE's cMelspec / cMfcc / cPlp / cSpectral compute them are the model
 *   ev_pyin_observe    <- no counterpart; librosa.pyin is the model
 *   ev_pyin_decode     <- no counterpart; librosa.pyin is the model
 *
 * Conventions
 *   - All tensors are fp32.  Pointers named d_* are DEVICE pointers owned by the
 *     caller (PyTorch-ROCm in the shipped host layer); they are borrowed for the
 *     duration of the call and all work is enqueued asynchronously on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream).
 *   - The handle owns the re-laid-out weights and a workspace that grows on demand, geometrically (growth = a wait for the
 *     handle's streams + hipFree + hipMalloc).  ev_reserve sizes everything once, up front, so that no later call at or below
 *     the reserved shape allocates or waits (a streaming server reserves its longest utterance: ev_alloc_count stays put).
 *   - Graph capture: ev_cfm_decode is capturable at any (B, Tp) the workspace already holds (ev_reserve, or an earlier eager call at the
 *     largest shape: planning must not allocate under capture): it enqueues kernels only and never waits on the host.  A handle may hold captured calls of MANY shapes (ABI 4; a serving loop keeps one graph per utterance length)
 *     and serve eager calls of any shape in between: once a call has been captured, every call on the handle — captured or eager —
 *     begins by re-zeroing the estimator's part of the workspace for its own plan, so none depends on what another left there.  A
 *     captured call consists of kernel nodes only (its re-zeroing is a kernel too): the time-MLP output for its step count must already be on the device, i.e.
 *     one EAGER ev_cfm_decode with the same n_steps must have run on the handle before (the handle keeps that output per step count;
 *     a host-to-device copy captured from pinned memory, and a captured memset, are not safe to replay on this runtime: later eager copies /
 *     memsets recycle their staging — profiles/r04_graph_capture_h2d_hazard.txt).
 *     What returns an error instead of pulling memory from under the graphs: a growth of the workspace beyond what is reserved, more
 *     Euler steps than the workspace is planned for (64, or the largest n_steps of an earlier call), a captured call with a step
 *     count no eager call has used.
 *   - Layout at the boundary is the reference's: mel-like tensors are (B, 80, T)
 *     channel-major contiguous; waveforms are (B, 256*T) contiguous.
 *   - Every function returns 0 on success, non-zero on failure; the message is
 *     available from ev_last_error().  Nothing throws across this boundary.
 *   - One handle per (device, stream user); calls on one handle are not thread-safe.  Different handles are independent:
 *     the library keeps no mutable process-global launch state, so two host threads may drive two handles concurrently.
 */
#ifndef EMOJIVOICE_H
#define EMOJIVOICE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EV_ABI_VERSION 4   /* 4 + additions that change nothing of 4: ev_vocoder_config, ev_load_vocoder_cfg, ev_load_mel_basis, ev_mel_spectrogram, ev_maximum_path, ev_log_prior, ev_mas_align, ev_estimator_rows, ev_cfm_loss, ev_load_resampler, ev_resample, ev_mel_stats, ev_trim_bounds, ev_trim_apply, ev_pitch_yin, ev_dtw, ev_loudness, ev_pyin_observe, ev_pyin_decode, ev_op_groupnorm_mish2, ev_op_conv_groupnorm, ev_op_attention2, ev_op_attn_out2, ev_load_stoi, ev_stoi, ev_load_stft_dist, ev_stft_dist, ev_load_voice_quality, ev_voice_quality, ev_load_formants, ev_formants, ev_perturbation, ev_load_harmonics, ev_harmonics, ev_functionals, ev_load_auditory, ev_auditory, ev_formant_track, ev_modulation, ev_load_srmr, ev_srmr, ev_load_speech_rate, ev_speech_rate, ev_load_envelope, ev_envelope, ev_load_phase_vocoder, ev_phase_vocoder, ev_op_conv1d_epi (look the symbol up to detect them);
                              4: ev_dbg_set_amax, ev_dbg_set_attn_h16, ev_dbg_set_chain, ev_dbg_sk_taken, captured decodes of many shapes; 3: ev_set_arithmetic / ev_get_arithmetic, ev_profile_read_split, test hooks; everything of earlier versions unchanged */

typedef struct ev_handle ev_handle;

/* One tensor of a weight blob: `name` is the reference state_dict key with the
 * module prefix stripped ("down_blocks.0.0.block1.block.0.weight", "conv_pre.weight" ...),
 * `offset` is in floats from the start of the HOST blob. */
typedef struct ev_tensor_index {
    const char *name;
    uint64_t offset;
    int32_t ndim;
    int64_t shape[4];
} ev_tensor_index;

/* Static model dimensions (reference configs/model/decoder/default.yaml, hifigan/config.py:1-28). */
typedef struct ev_model_dims {
    int32_t n_feats;       /* 80 */
    int32_t spk_emb_dim;   /* 64 (0 for a single-speaker checkpoint) */
    int32_t channels;      /* 256 */
    int32_t heads;         /* 2 */
    int32_t head_dim;      /* 64 */
} ev_model_dims;

int ev_abi_version(void);
int ev_create(ev_handle **out, int device, const ev_model_dims *dims);
void ev_destroy(ev_handle *h);
const char *ev_last_error(ev_handle *h);

/* Weights: host blob + index; copied and re-laid-out into library-owned device memory. */
int ev_load_estimator(ev_handle *h, const float *blob, const ev_tensor_index *index, size_t n);
int ev_load_vocoder(ev_handle *h, const float *blob, const ev_tensor_index *index, size_t n);   /* the V1 config (hifigan/config.py:1-28) */

/* A HiFi-GAN generator config (the `h` of hifigan/models.py:148-179).  Channel widths come from the tensors (conv_pre's output
 * halving per level).  Supported envelope — anything else fails with a message naming the constraint:
 *   1..4 levels, product of the rates 256; k >= u and k - u even per level; exactly 3 resblock kernel sizes, odd, <= 16;
 *   3 dilations per ResBlock1 (halo (k-1) d / 2 <= 32), 2 per ResBlock2 (halo <= 64); every level's width a multiple of 8. */
typedef struct ev_vocoder_config {
    int32_t resblock;                   /* 1: ResBlock1, 2: ResBlock2 */
    int32_t num_levels;                 /* len(upsample_rates) */
    int32_t upsample_rates[4];
    int32_t upsample_kernel_sizes[4];
    int32_t resblock_kernel_sizes[3];
    int32_t resblock_dilations[3][3];   /* per kernel size; ResBlock2 reads the first two */
} ev_vocoder_config;
int ev_load_vocoder_cfg(ev_handle *h, const float *blob, const ev_tensor_index *index, size_t n, const ev_vocoder_config *cfg);
/* Text-encoder keys: state_dict["encoder.<key>"] (matcha_tts.py:52-60) plus "rope_theta" =
 * 1 / (10000 ** (arange(0, d, 2) / d)), d = 64  (text_encoder.py:115-117), computed by the loader with the reference's ops. */
int ev_load_text_encoder(ev_handle *h, const float *blob, const ev_tensor_index *index, size_t n);

/* Bytes of device workspace the two hot calls need at a given shape (0 on bad args). */
size_t ev_workspace_bytes(ev_handle *h, int B, int Tp_cfm, int T_voc);

/* Conditional-flow-matching ODE decode: n_steps Euler steps of the U-Net estimator.
 *   d_mu      (B, 80, Tp)  aligned encoder output mu_y          (matcha_tts.py:134-135)
 *   d_lengths (B) int32    valid frames per utterance (y_lengths; mask = t < length)
 *   d_spk     (B, 64)      speaker/emoji embedding rows (NULL iff spk_emb_dim == 0)
 *   d_z       (B, 80, Tp)  initial state x0 = noise * temperature (flow_matching.py:51)
 *   d_out     (B, 80, Tp)  decoder output; out_scale/out_shift fuse denormalize()
 *                          (utils/model.py:71-90): out = dec*out_scale + out_shift
 *   Tp must be a multiple of 4 (fix_len_compatibility, utils/model.py:14-20). */
int ev_cfm_decode(ev_handle *h, const float *d_mu, const int32_t *d_lengths, const float *d_spk, const float *d_z,
                  int B, int Tp, int n_steps, float out_scale, float out_shift, float *d_out, void *stream);

/* The same decode with both of the reference's outputs (matcha_tts.py:139-152): d_dec = "decoder_outputs" (may be NULL),
 * d_mel = "mel" = denormalize(decoder_outputs, mel_mean, mel_std) = dec * mel_std + mel_mean (may be NULL; not both). */
int ev_cfm_decode2(ev_handle *h, const float *d_mu, const int32_t *d_lengths, const float *d_spk, const float *d_z,
                   int B, int Tp, int n_steps, float *d_dec, float mel_std, float mel_mean, float *d_mel, void *stream);

/* Pre-size everything the hot calls allocate on demand, for batches of B utterances of up to Tx_max tokens (ev_text_encoder),
 * Tp_max mel frames (ev_cfm_decode / ev_estimator; multiple of 4) and T_voc_max mel frames (ev_hifigan, ev_denoise and
 * ev_mel_spectrogram at L = 256 * T_voc_max): the workspace arena, the text-encoder and denoiser scratch, the pinned time-embedding ring, the
 * denoiser's DFT bases and the side streams of the small-call vocoder.  0 skips a stage.  After it, calls with the same B and
 * lengths up to the reserved ones never allocate (ev_alloc_count does not move) and never wait for the device to re-plan.
 * The reference has no counterpart: torch's caching allocator amortises the same cost (feel_me.py:181-203). */
int ev_reserve(ev_handle *h, int B, int Tx_max, int Tp_max, int T_voc_max, void *stream);
/* Device / pinned allocations made by the hot calls since ev_create (workspace growth, scratch growth, staging). */
int64_t ev_alloc_count(ev_handle *h);

/* One estimator evaluation v = Decoder(x, mask, mu, t, spk)  (decoder.py:363-443). */
int ev_estimator(ev_handle *h, const float *d_x, const float *d_mu, const int32_t *d_lengths, const float *d_spk,
                 float t, int B, int Tp, float *d_v, void *stream);

/* Text encoder + duration predictor (the stage in front of ev_cfm_decode; matcha_tts.py:118-121):
 *   d_ids     (B, Tx) int64  phoneme ids (torch.long, as the reference passes them)
 *   d_lengths (B) int32      valid tokens per utterance (x_lengths; mask = t < length)
 *   d_spk     (B, 64)        speaker/emoji embedding rows (NULL iff the model is single-speaker)
 *   d_mu      (B, 80, Tx)    mu_x, masked          d_logw (B, Tx)  log-durations, masked
 * Duration rounding, the monotonic alignment path and mu_y = attn^T mu_x stay with the caller (data-dependent sizes). */
int ev_text_encoder(ev_handle *h, const int64_t *d_ids, const int32_t *d_lengths, const float *d_spk, int B, int Tx,
                    float *d_mu, float *d_logw, void *stream);

/* The reference's nn.Embedding raises IndexError for a token id outside [0, n_vocab) (text_encoder.py:395).  The device
 * stage cannot raise mid-stream: it computes from a clamped id and records the event.  This call waits for `stream` and
 * returns non-zero ("index out of range in self") if any ev_text_encoder call since the last check saw such an id among
 * the valid tokens; the host layer calls it at its first natural synchronisation point (the read of max(y_lengths)). */
int ev_text_encoder_status(ev_handle *h, void *stream);

/* Hard monotonic alignment and expansion (utils/model.py:29-41 generate_path; matcha_tts.py:131-135):
 *   d_wceil (B, Tx) f32   ceil(exp(logw) * x_mask) * length_scale        d_mu_x (B, 80, Tx)
 *   d_xlen (B) int32, d_ylen (B) int64 (= clamp_min(sum(w_ceil), 1).long(), computed by the caller: its maximum fixes Tp)
 *   d_mu_y (B, 80, Tp) = attn^T mu_x;   d_attn (B, Tx, Tp) 0/1 path, may be NULL */
int ev_align(ev_handle *h, const float *d_wceil, const float *d_mu_x, const int32_t *d_xlen, const int64_t *d_ylen,
             int B, int Tx, int Tp, float *d_mu_y, float *d_attn, void *stream);

/* Largest ev_hifigan call (B*T mel frames) that fans its ResBlock1 chains out over three streams (see ev_hifigan); 0 = never.
 * Default 16384, or EV_MRF_STREAMS_MAX.  A caller that already overlaps the vocoder with other work on a second stream, and
 * must not have the host wait inside the call, sets 0 (emojivoice_amd/pipeline.py does). */
int ev_set_mrf_streams_max(ev_handle *h, int max_frames);

/* HiFi-GAN generator of the loaded config: d_mel (B, 80, T) -> d_wav (B, 256*T), tanh output, no clamp/denoiser.
 * Calls of B*T <= 16384 mel frames (EV_MRF_STREAMS_MAX) first wait for `stream` to drain on the host, then run the three
 * ResBlock1 chains of each level on `stream` and two streams of the handle, joined back into `stream` by events before the
 * call returns: the result is ordered on `stream` like that of any other call.  Such a call is not graph-capturable. */
int ev_hifigan(ev_handle *h, const float *d_mel, int B, int T, float *d_wav, void *stream);

/* Denoiser stage that every reference caller applies to the vocoder output (hifigan/denoiser.py:10-64; cli.py:121-126,
 * feel_me.py:181-187): torch.stft / torch.istft semantics at n_fft = win = 1024, hop 256, periodic Hann window, centred
 * with reflect padding, evaluated as two DFT-basis convolutions on the matrix cores.
 *   ev_stft_magnitude: d_audio (B, L) -> d_mag (B, 513, L/256 + 1)     (Denoiser.__init__'s bias spectrum)
 *   ev_denoise:        d_out = ISTFT(clamp(|X| - bias*strength, 0) * exp(i*angle(X))), X = STFT(d_audio); d_bias_spec (513)
 * L must be a multiple of 256 (it is 256 * mel frames) and >= 768: like torch.stft's reflect padding (512 each side), which
 * the reference relies on, inputs of 512 samples or fewer are an error. */
int ev_stft_magnitude(ev_handle *h, const float *d_audio, int B, int L, float *d_mag, void *stream);
int ev_denoise(ev_handle *h, const float *d_audio, int B, int L, const float *d_bias_spec, float strength, float *d_out, void *stream);

/* The analysis side: the reference's mel_spectrogram (utils/audio.py:45-82) at n_fft = win_size = 1024, hop_size 256, center=False.
 * The signal is reflect-padded by (1024 - 256) / 2 = 384 samples a side, the STFT is the denoiser's forward DFT-basis convolution
 * (periodic Hann window, exact fp32 MFMA in every arithmetic setting), and one kernel (mel_project_kernel) turns the
 * [re | im] rows into the finished mel: sqrt(re^2 + im^2 + 1e-9), the filter bank, log(clamp(., 1e-5)), scale and shift.
 *   ev_load_mel_basis: the filter bank, HOST (n_mels, n_freq) row-major; n_freq must be 513, 1 <= n_mels <= 128.  The handle keeps,
 *     per filter, [first bin, count] and the weights of that span only (a Slaney triangle covers at most ~60 of the 513 bins at
 *     80 mels).  A row whose non-zero weights are NOT one contiguous run is kept as the single span from its first to its last
 *     non-zero bin, the zeros in between included (in the worst case the whole row: the dense product), so any basis gives the
 *     result of the dense matrix product.  Loading again replaces the bank (it waits for the device first).
 *   ev_mel_spectrogram: d_audio (B, L) -> d_mel (B, n_mels, L / 256):
 *       log(clamp(basis @ sqrt(re^2 + im^2 + 1e-9), 1e-5)) * out_scale + out_shift
 *     out_scale = 1 / mel_std, out_shift = -mel_mean / mel_std fuse normalize() (utils/model.py); 1, 0 is the reference function.
 *     L must be a positive multiple of 256 and > 384 (torch's reflect padding of 384 needs more samples than that); L / 256 frames
 *     come out, the reference's frame count for such L.  Scratch is the denoiser's: ev_reserve(.., T_voc_max) covers a call at
 *     L = 256 * T_voc_max.  Needs no estimator or vocoder weights; without a loaded basis the call fails with a message. */
int ev_load_mel_basis(ev_handle *h, const float *basis, int n_mels, int n_freq);
int ev_mel_spectrogram(ev_handle *h, const float *d_audio, int B, int L, float out_scale, float out_shift, float *d_mel, void *stream);

/* Monotonic alignment search on the device: the no-grad side of MatchaTTS.forward (matcha_tts.py:186-199) and the reference's only native
 * code, utils/monotonic_align/core.pyx.  Everything is enqueued on `stream`; nothing waits on the host or copies to or from it.
 *   ev_maximum_path: the search alone, on scores the caller supplies (any Glow-TTS-style aligner).
 *       d_value (B, Tx, Ty) f32, read only      d_xlen, d_ylen (B) int32: t_x, t_y of each row (what the reference takes from its mask)
 *       d_path (B, Tx, Ty) f32 0/1 or NULL      d_dur (B, Tx) int32 = sum_j path[b, i, j], or NULL
 *     Semantics are maximum_path_each's: value[x, y] += max(x == y ? -1e9 : value[x, y-1], x == 0 ? (y == 0 ? 0 : -1e9) : value[x-1, y-1])
 *     inside the band max(0, t_x + y - t_y) <= x < min(t_x, y + 1), then the backtrack from t_x - 1 that steps down where
 *     `index == y or value[index, y-1] < value[index-1, y-1]` (strict: a tie stays on the token).  One fp32 max and one fp32 add per cell:
 *     path and durations are BIT-EQUAL to that loop for every finite input, ties included.  Rows of d_path beyond xlen and columns
 *     beyond ylen are written as zeros, as the reference's path is.
 *   ev_log_prior: d_mu_x (B, C, Tx), d_y (B, C, Ty) -> d_logp (B, Tx, Ty), every cell, unmasked; C = n_feats of the handle:
 *       logp[b, i, j] = -0.5 sum_c (y[c, j] - mu_x[c, i])^2 - 0.5 C log(2 pi)
 *     the quantity the reference expands into two matmuls and a row sum; here the direct form, one fp32 fmaf chain over the channels
 *     in every arithmetic setting (no fp16 / bf16 pieces: the scores feed a hard decision).
 *   ev_mas_align: the fused call.  One workgroup per utterance forms the scores of 16 frames at a time in LDS, takes the DP steps on
 *     a running column and keeps ONE decision bit per cell (the backtrack's predicate); the fp32 (B, Tx, Ty) matrix is never written
 *     unless d_logp is given, and then d_logp holds the very values the search consumed (the bits ev_log_prior gives).
 *       d_attn (B, Tx, Ty) 0/1 or NULL      d_dur (B, Tx) int32 or NULL      d_mu_y (B, C, Ty) = attn^T mu_x (a gather) or NULL
 *       d_logp (B, Tx, Ty) or NULL
 *     attn / dur are bit-equal to ev_maximum_path on that d_logp.
 * Limits: 1 <= B <= 65535, 1 <= Tx <= 4096 (two columns and a tile of at least four frames in the CU's 160 KiB of LDS), 1 <= Ty.
 * A row with xlen < 1, xlen > ylen (where the reference reads outside the row), xlen > Tx or ylen > Ty is no error and no out-of-bounds
 * access: its path, durations and mu_y are written as zeros.
 * Scratch: B x Ty int32 (frame -> token) plus, only when Ty x ceil(Tx / 64) x 8 bytes of decision bits do not fit into LDS beside the tile,
 * that many bytes per row — an arena of the handle that grows on demand like the denoiser's and counts in ev_alloc_count (a second call
 * at the same shape allocates nothing); ev_reserve does not cover it. */
int ev_maximum_path(ev_handle *h, const float *d_value, const int32_t *d_xlen, const int32_t *d_ylen, int B, int Tx, int Ty,
                    float *d_path, int32_t *d_dur, void *stream);
int ev_log_prior(ev_handle *h, const float *d_mu_x, const float *d_y, int B, int Tx, int Ty, float *d_logp, void *stream);
int ev_mas_align(ev_handle *h, const float *d_mu_x, const float *d_y, const int32_t *d_xlen, const int32_t *d_ylen, int B, int Tx, int Ty,
                 float *d_attn, int32_t *d_dur, float *d_mu_y, float *d_logp, void *stream);

/* The estimator with one time per utterance, and the flow-matching loss of a batch on top of it: the no-grad validation pass
 * (MatchaTTS.forward over (text, mel) pairs) at batch speed.  Both are EAGER-ONLY: they copy the B times' sinusoids from the host, and
 * under stream capture they fail with a message (the staging hazard of "Graph capture" above).  `t` is a HOST pointer to B floats.
 *   ev_estimator_rows: ev_estimator, utterance b evaluated at t[b] — what Decoder.forward computes for t of shape (B,).  With every
 *     t[b] equal it agrees with ev_estimator to rounding (the time MLP may run on another build at B rows than at one).
 *   ev_cfm_loss: compute_loss for given draws, without gradients.
 *       d_x1 (B, 80, Ty) the target mel      d_mu_y (B, 80, Ty)      d_ylen (B) int32      d_spk (B, 64) or NULL as for ev_cfm_decode
 *       d_z (B, 80, Ty) unit normal noise    t (B) HOST              Ty >= 1, any value: the call pads to Tp = ceil(Ty / 4) * 4 itself,
 *                                                                    with masked frames
 *       d_row_sums (B, 2) float64:  [b][0] = sum (v - u)^2,  [b][1] = sum 0.5 ((x1 - mu_y)^2 + log 2 pi)  over the row's ylen[b] x 80 valid cells
 *       d_v (B, 80, Ty) or NULL: the estimator's velocity (zeros past a row's length)
 *     y_t = (1 - (1 - sigma_min) t) z + t x1 and u = x1 - (1 - sigma_min) z are formed in float32 in the reference's operation order,
 *     and never stored: y_t goes straight into the estimator's input, u is formed where v is read.  The squares accumulate in float64,
 *     per (row, 32 frames), merged per row in ascending order without atomics: two calls give the same bits.  The batch losses are
 *     sum_b sums / (sum_b ylen * 80); the caller divides.  (The reference's mse_loss also counts the PADDED frames of shorter rows, where
 *     v = 0 and u is whatever x1 and z hold there; that term needs no estimator and is the caller's, emojivoice_amd/matcha_tts.py.)
 *     A row with ylen < 1 or ylen > Ty is no error: its sums and its d_v are zeros.
 * Both plan one time slot per utterance: B beyond the planned Euler steps (64, or the largest n_steps so far) re-plans the workspace
 * like a longer decode does, which a handle that holds a captured call refuses.  One such growth moves ev_alloc_count once; a second
 * call at the same shape allocates nothing. */
int ev_estimator_rows(ev_handle *h, const float *d_x, const float *d_mu, const int32_t *d_lengths, const float *d_spk,
                      const float *t /* HOST (B) */, int B, int Tp, float *d_v, void *stream);
int ev_cfm_loss(ev_handle *h, const float *d_x1, const float *d_mu_y, const int32_t *d_ylen, const float *d_spk, const float *d_z,
                const float *t /* HOST (B) */, int B, int Ty, float sigma_min, double *d_row_sums, float *d_v, void *stream);

/* Sample-rate conversion on the device: a rational polyphase FIR, so that recordings at 44.1 / 48 / 16 kHz reach the 22.05 kHz analysis
 * side (and synthesis can be written at a playback device's rate).  With c = (n_taps - 1) / 2,
 *       y[b, n] = sum_i x[b, i] * taps[n * down - i * up + c]      for 0 <= n < L_out = ceil(L_in * up / down),
 * x zero outside [0, len[b]) (d_len == NULL: every row is L_in long); `taps` carries the gain `up`.  This is
 * scipy.signal.resample_poly(x, up, down, window=taps / up, padtype="constant"); emojivoice_amd.audio.resample_filter restates scipy's
 * default Kaiser design.  Outputs at or beyond ceil(len[b] * up / down) are written as zeros; a row with len < 1 or len > L_in is no
 * error: it is written as zeros (the ev_mas_align convention).
 *   ev_load_resampler: taps HOST (n_taps).  1 <= up, down <= 640 (8 / 11.025 / 16 / 32 / 44.1 / 48 / 96 kHz against 22.05 kHz),
 *     gcd(up, down) == 1, n_taps odd and <= 65537; each violation fails with a message naming it.  up = down = 1 with one tap is a scaled
 *     copy.  The handle keeps the taps phase-major, [up][ceil(n_taps / up)] zero-padded: output n reads ONE contiguous row, that of phase
 *     (n * down + c) mod up.  Loading again replaces the filter (it waits for the device first).
 *   ev_resample: d_x (B, L_in), d_len (B) int32 or NULL -> d_y (B, L_out); 1 <= B <= 65535, L_out must equal the formula above.  Without
 *     a loaded resampler the call fails with a message.
 *     Arithmetic: one fp32 fmaf chain per output in every arithmetic setting (no fp16 / bf16 pieces), over the taps of the output's phase
 *     in ascending tap index (i descending), ALL ceil(n_taps / up) of them, samples outside the row entering as +0.  The order does not
 *     depend on tiling or on the batch: a row resampled alone, inside a batch, or as the prefix (d_len) of a longer padded row gives the
 *     same bits.  Index arithmetic is 64-bit per tile (n * down and i * up pass 2^31 after minutes of audio).
 *     The call enqueues one kernel on `stream`; its only scratch is the handle's tap table (nothing to reserve, ev_alloc_count never moves).
 * Dataset statistics (utils/generate_data_statistics.py:25-47, what a fine-tuning config needs as mel_mean / mel_std):
 *   ev_mel_stats: d_mel (B, C, T), d_len (B) int32 -> d_row_sums (B, 2) float64: [b][0] = sum x, [b][1] = sum x^2 over the row's
 *     len[b] x C valid cells.  float64 accumulation per (row, 32 frames), merged per row in ascending order without atomics: two calls
 *     give the same bits.  A row with len < 1 or len > T is written as zeros.  mean = sum_b [0] / (sum_b len * C),
 *     std = sqrt(sum_b [1] / (sum_b len * C) - mean^2); the caller combines (emojivoice_amd.audio.data_statistics).
 *     Scratch: B x ceil(T / 32) x 16 bytes in an arena of the handle that grows on demand and counts in ev_alloc_count; ev_reserve does
 *     not cover it. */
int ev_load_resampler(ev_handle *h, const float *taps /* HOST (n_taps) */, int n_taps, int up, int down);
int ev_resample(ev_handle *h, const float *d_x /* (B, L_in) */, const int32_t *d_len /* (B) or NULL */, int B, int L_in,
                float *d_y /* (B, L_out) */, int L_out, void *stream);
int ev_mel_stats(ev_handle *h, const float *d_mel /* (B, C, T) */, const int32_t *d_len /* (B) */, int B, int C, int T,
                 double *d_row_sums /* (B, 2): sum x, sum x^2 over the row's len[b] x C valid cells */, void *stream);

/* Dataset preparation: trim the silence around a recording and level it, on the device.  The semantics are those of
 * librosa.effects.trim(y, top_db, ref=np.max, frame_length, hop_length) and of normalize(audio) * 0.95 (hifigan/meldataset.py:152).
 * For a row of len samples, F = frame_length, H = hop_length:
 *   frames     n_frames = 1 + len / H; frame f covers samples [f H - F/2, f H + F/2), zeros outside [0, len) (center=True, constant padding)
 *   ms[f]      (1 / F) sum x^2 over the frame
 *   non-silent max(ms[f], 1e-10) > max(max_f ms, 1e-10) * 10^(-top_db / 10): amplitude_to_db(rms, ref=np.max, amin=1e-5, top_db=None) > -top_db
 *              in the power domain
 *   bounds     start = f_first H, end = min(len, (f_last + 1) H), f_first / f_last the first / last non-silent frame.  The loudest frame
 *              passes for any top_db > 0, so an all-zero row keeps [0, len); top_db <= 0 leaves no frame and gives (0, 0), as librosa does
 *   peak       max |x| over the WHOLE row (levelling precedes trimming in meldataset.py)
 *   ev_trim_bounds: d_x (B, L), d_len (B) int32 or NULL (every row L long) -> d_bounds (B, 2) int32 {start, end}, d_peak (B) or NULL.
 *     1 <= B <= 65535; hop_length a multiple of 64 and at most 4096; frame_length a multiple of hop_length; frame_length / hop_length <= 64;
 *     each violation fails with a message naming it.
 *     Arithmetic: the row is cut into hop blocks of H samples starting at -((F/2) mod H), so that a frame is F / H whole blocks.  A block is
 *     read once; each fp32 sample is widened to float64 and squared (exact) and the block summed in a fixed order (per-lane partials in
 *     ascending sample index, one fixed tree over the wave); a frame is the sum of its blocks in ascending order, blocks outside the row
 *     +0.  No atomics: two calls give the same bits, and a row alone, inside a batch, or as the d_len prefix of a longer padded row gives
 *     the same block sums, bounds and peak.  ev_set_arithmetic does not reach it.
 *     Scratch: B x ceil((L + (F/2) mod H) / H) x 12 bytes (B x ceil(L / H) x 12 when F / H is even) in an arena of the handle that grows on
 *     demand and counts in ev_alloc_count; a second call at the same shape allocates nothing; ev_reserve does not cover it.
 *   ev_trim_apply: y[b, j] = x[b, start[b] + j] * gain[b] for j < out_len[b] = min(end[b] - start[b], L_out), +0 from there up to L_out
 *     (L_out >= 1 is the caller's choice: a longer row is truncated).  gain[b] = target_peak / d_peak[b], one fp32 division, when d_peak is
 *     given, target_peak > 0 and d_peak[b] > 0; otherwise 1 (a bit-exact copy).  One fp32 multiply per sample.  d_bounds and d_peak are read
 *     on the device: the output of ev_trim_bounds feeds it without a trip to the host.
 *   Bad rows are no error and no out-of-bounds access (the ev_mas_align convention): len < 1 or len > L gives bounds (0, 0) and peak 0;
 *   bounds outside 0 <= start <= end <= L give a row of zeros and out_len 0.
 *   Both calls enqueue kernels on `stream` only (capturable once the scratch has its size) and need no weights. */
int ev_trim_bounds(ev_handle *h, const float *d_x /* (B, L) */, const int32_t *d_len /* (B) or NULL */, int B, int L,
                   int frame_length, int hop_length, float top_db,
                   int32_t *d_bounds /* (B, 2): start, end */, float *d_peak /* (B) or NULL */, void *stream);
int ev_trim_apply(ev_handle *h, const float *d_x /* (B, L) */, const int32_t *d_bounds /* (B, 2) */,
                  const float *d_peak /* (B) or NULL */, float target_peak /* <= 0: no levelling */, int B, int L,
                  float *d_y /* (B, L_out) */, int L_out, int32_t *d_out_len /* (B) */, void *stream);

/* Pitch tracking on the device: de Cheveigne and Kawahara's YIN (JASA 111, 2002) without its final "best local estimate" step; librosa.yin is
 * the model.  W = frame_length, H = hop_length, F = ceil(L / H) frames per row of the outputs; a row of len samples has ceil(len / H) frames.
 *   framing    frame f analyses x[s_f + j], 0 <= j < W + tau_max + 1, s_f = f H + H/2 - (W + tau_max) / 2 (integer divisions): the span is
 *              centred on the centre of frame f of ev_mel_spectrogram at the same hop.  Samples outside [0, len) enter as +0.
 *   d(tau)     sum_{j < W} (x[j] - x[j + tau])^2 for 1 <= tau <= tau_max + 1
 *   d'(tau)    d(tau) * tau / S(tau) where S(tau) = sum_{k <= tau} d(k) > 0, else 1 (the cumulative mean normalised difference)
 *   decision   tau0 = the smallest tau in [tau_min, tau_max] with d'(tau) < threshold; then, while tau0 + 1 <= tau_max and
 *              d'(tau0 + 1) < d'(tau0), tau0 advances.  No such tau: the frame is unvoiced (a silent frame has every d = 0 and is unvoiced)
 *   refinement a, b, c = d'(tau0 - 1), d'(tau0), d'(tau0 + 1) (tau0 >= 2 because d'(1) = 1; d is computed one lag beyond tau_max);
 *              shift = 0.5 (a - c) / (a - 2 b + c) when the denominator is > 0 and |shift| <= 1, else 0; period = tau0 + shift
 *   d_lag (B, F) int32 or NULL     tau0, 0 when unvoiced
 *   d_period (B, F) or NULL        the period in samples (f0 = sample rate / period), rounded once to float32; 0 when unvoiced
 *   d_cmnd (B, F) or NULL          d'(tau0) of a voiced frame; of an unvoiced one min d' over [tau_min, tau_max], the aperiodicity a caller
 *                                  thresholds for itself
 *   Frames at or beyond a row's ceil(len / H) are written as zeros in all three outputs.  A row with len < 1 or len > L is no error and no
 *   out-of-bounds access: it is written as zeros (the ev_mas_align convention).  d_len == NULL: every row is L long.
 * Limits, each violation failing with a message that names it: 1 <= B <= 65535; hop_length a multiple of 64 and at most 4096; frame_length a
 *   multiple of 64 with 64 <= frame_length <= 4096; 1 <= tau_min <= tau_max <= 2048; 0 < threshold <= 1; at least one output non-NULL.
 * Arithmetic: all of it float64, in one fixed order.  Both fp32 samples are widened, so the difference is exact; it is squared and added by one
 *   fma per term, in ascending j within each quarter [q W/4, (q + 1) W/4) of the window (one lane per lag and quarter), and
 *   d = (P0 + P1) + (P2 + P3) over the four quarters' partials.  S is one chain of adds in ascending tau, d' = (d * tau) / S.  No atomics.
 *   Nothing depends on the batch, the grid or ev_set_arithmetic: a row alone, inside a batch, or as the d_len prefix of a longer padded row,
 *   and a second call, give the same bits.
 * One kernel launch (pitch_yin_kernel, one workgroup per frame and row) on `stream`; capturable; no weights and no scratch: ev_alloc_count
 *   never moves.  Cost: W (tau_max + 1) float64 fmas per frame. */
int ev_pitch_yin(ev_handle *h, const float *d_x /* (B, L) */, const int32_t *d_len /* (B) or NULL */, int B, int L,
                 int frame_length /* W */, int hop_length /* H */, int tau_min, int tau_max, float threshold,
                 int32_t *d_lag /* (B, F) or NULL */, float *d_period /* (B, F) or NULL */, float *d_cmnd /* (B, F) or NULL */,
                 void *stream);

/* Probabilistic YIN on the device: Mauch and Dixon's pYIN (ICASSP 2014); librosa.pyin is the model.  Two calls: ev_pyin_observe turns every
 * frame into a distribution over pitch bins and a voicing probability, ev_pyin_decode picks the contour by a Viterbi pass over
 * (voiced / unvoiced) x pitch bins.  W, H, F, the framing, d(tau) and d'(tau) for 1 <= tau <= tau_max + 1 are EXACTLY ev_pitch_yin's (the same
 * device code: same spans, same zeros outside [0, len), same fma order, same S chain); additionally d'(0) := 1.
 * Observation, per frame:
 *   troughs     the lags tau in [tau_min, tau_max] with d'(tau) < d'(tau - 1) and d'(tau) <= d'(tau + 1), in ascending lag tau_0 < tau_1 < ...
 *               d' exists one lag beyond each end of the range, so the ends need no rule of their own (librosa pads the ends of its range
 *               instead).  A silent frame (d' = 1 at every lag) has none.
 *   thresholds  theta_t = t / n_thr (float64 division), t = 1 .. n_thr; w (HOST, n_thr float64, read during the call): w[t - 1] = the prior
 *               mass of (theta_{t-1}, theta_t] (audio.pyin_threshold_prior: Beta(2, 18) over 100 thresholds)
 *   activity    active(k, t) = d'(tau_k) < theta_t (monotone in t); pos(k, t) = #{m < k : active(m, t)}; N(t) = #{m : active(m, t)}
 *   P_k         sum over t, ascending, of active(k, t) G_t exp(-boltzmann pos(k, t)), G_t = w_t (1 - exp(-boltzmann)) / (1 - exp(-boltzmann N(t)))
 *   global min  g = the trough of smallest d', lowest lag on ties: P_g += no_trough_prob * (the sum of w_t over the t with active(g, t) false,
 *               a prefix of t, in ascending t)
 *   period_k    tau_k + shift_k, the parabolic shift of ev_pitch_yin (denominator > 0 and |shift| <= 1, else 0), kept in float64
 *   bin_k       clip(rint(bins_per_octave * log2(sr / (period_k * fmin))), 0, n_bins - 1), halves to even: bin i is fmin 2^(i / bins_per_octave)
 *   d_obs (B, F, n_bins) float64   obs[bin_k] += P_k over the troughs with P_k > 0, in ascending k; every other bin 0
 *   d_pv (B, F) float64            min(sum_i obs[i], 1), summed in ascending i: the probability that the frame is voiced
 *   Frames at or beyond a row's ceil(len / H), and rows with len < 1 or len > L, are zeros in both.  d_len == NULL: every row is L long.
 * Limits, each violation failing with a message that names it: those of ev_pitch_yin for B, frame_length, hop_length, tau_min and tau_max;
 *   1 <= n_thr <= 128; 2 <= n_bins <= 1024; bins_per_octave >= 1; sr, fmin > 0; boltzmann > 0; 0 <= no_trough_prob <= 1; finite w >= 0;
 *   d_obs and d_pv non-NULL.
 * One kernel launch (pyin_observe_kernel, one workgroup per frame and row) on `stream`; all float64; no atomics; capturable; every buffer is
 *   the caller's: ev_alloc_count never moves.  A row alone, inside a batch, or as the d_len prefix of a longer padded row, and a second call,
 *   give the same bits.  Cost: ev_pitch_yin's W (tau_max + 1) fmas per frame plus 2 n_thr ballots per 64 troughs. */
int ev_pyin_observe(ev_handle *h, const float *d_x /* (B, L) */, const int32_t *d_len /* (B) or NULL */, int B, int L,
                    int frame_length /* W */, int hop_length /* H */, int tau_min, int tau_max, double sr, double fmin,
                    int bins_per_octave, int n_bins, const double *w /* HOST (n_thr) */, int n_thr, double boltzmann,
                    double no_trough_prob, double *d_obs /* (B, F, n_bins) */, double *d_pv /* (B, F) */, void *stream);

/* Decoding, per row, over that row's own nf = ceil(len / H) frames of d_obs / d_pv (any float64 arrays of those shapes; F = ceil(L / H)).
 *   states      s = v n_bins + i, v = 0 voiced, v = 1 unvoiced
 *   emission    e(0, i) = obs[i], e(1, i) = (1 - pv) / n_bins; l = log(e + tiny), tiny the smallest normal double
 *   transition  (v', j) -> (v, i) exists for |i - j| <= R and has log a = T[|i - j|] - log_Z[j], T[d] = log_tri[d] + (v' == v ? log_stay :
 *               log_switch), formed first.  HOST float64 tables, read during the call (audio.pyin_transition): log_tri[d] = log(R + 1 - d)
 *               for d <= R; log_Z[j] = log of the sum of R + 1 - |i - j| over the i inside [0, n_bins); log_stay = log(1 - switch_prob),
 *               log_switch = log(switch_prob)
 *   recursion   delta_0(s) = -log(2 n_bins) + l_0(s); delta_t(s) = max_{s'} [(delta_{t-1}(s') - log_Z[j]) + T[|i - j|]] + l_t(s): float64 adds
 *               and compares only, plus one log per emission.  Predecessors are visited in ascending s' and a later one replaces an earlier one
 *               only when STRICTLY greater; the end state is the lowest s of greatest delta
 *   d_back (B, F, 2 n_bins) uint8   scratch of the caller's: the back-pointer byte v' (2 R + 1) + (j - i + R) of frames 1 .. nf - 1
 *   d_state (B, F) int32            the best path's state per frame; -1 at and beyond nf (a row with len < 1 or len > L: all -1)
 *   d_loglik (B) float64            delta of the end state (0 for such a row)
 * Limits, each violation failing with a message that names it: 1 <= B <= 65535; hop_length a multiple of 64 and at most 4096;
 *   2 <= n_bins <= 1024; 0 <= R <= 63; log_stay and log_switch finite and negative (0 < switch_prob < 1); finite tables; log_Z constant over
 *   R <= j <= n_bins - 1 - R (as its definition makes it); every pointer but d_len non-NULL.
 * One kernel launch (pyin_decode_kernel) on `stream`, one workgroup per row, delta double-buffered in LDS, one barrier per frame; one lane walks
 *   the back-pointers.  Latency-bound like ev_dtw: 2 (2 R + 1) add-compares per state and frame.  No atomics, no scratch of the handle
 *   (ev_alloc_count never moves), capturable; a row alone, inside a batch, or as a prefix, and a second call, give the same bits. */
int ev_pyin_decode(ev_handle *h, const double *d_obs /* (B, F, n_bins) */, const double *d_pv /* (B, F) */,
                   const int32_t *d_len /* (B) or NULL */, int B, int L, int hop_length /* H */, int n_bins, int R,
                   const double *log_tri /* HOST (R + 1) */, const double *log_Z /* HOST (n_bins) */, double log_stay, double log_switch,
                   uint8_t *d_back /* (B, F, 2 n_bins) */, int32_t *d_state /* (B, F) */, double *d_loglik /* (B) */, void *stream);

/* Dynamic time warping on the device between two feature sequences per row: x (B, C, Tx) against y (B, C, Ty), tx = d_xlen[b] and
 * ty = d_ylen[b] frames of them (a NULL length pointer: the padded size).  The step pattern is the plain one (diagonal, up, left; weight 1).
 *   local cost  c[i, j] = sum_c (x[c, i] - y[c, j])^2: both fp32 values widened to float64, one float64 fma per channel in ascending c;
 *               metric 0 (Euclidean): one correctly rounded square root follows; metric 1: the squared distance itself.  The order depends
 *               on nothing else: not on tiling, the batch or ev_set_arithmetic.
 *   recurrence  float64, one min chain and one add per cell: D[0, 0] = c[0, 0]; otherwise D[i, j] = c[i, j] + m, m the smallest of the
 *               predecessors that exist, taken in the order diagonal (i-1, j-1), up (i-1, j), left (i, j-1); a later candidate replaces
 *               an earlier one only when STRICTLY smaller, so ties go diagonal, then up, then left.  S[i, j] = S[chosen] + 1, S[0, 0] = 1.
 *   d_cost (B) float64    D[tx-1, ty-1]
 *   d_steps (B) int32     S[tx-1, ty-1] = K, the length of the path: max(tx, ty) <= K <= tx + ty - 1
 *   d_path (B, Tx + Ty - 1, 2) int32 or NULL   (i_k, j_k) for k < K, ascending from (0, 0) to (tx-1, ty-1); every entry at or beyond K is
 *                         (-1, -1).  The backtrack replays the forward step's own choice (2 bits per cell); it never compares again.
 *   A row with tx < 1, ty < 1, tx > Tx or ty > Ty is no error and no out-of-bounds access: cost 0, steps 0, a path of -1 (the ev_mas_align
 *   convention).  Nothing behind a row's tx / ty frames is read.  Only finite inputs are specified.
 * Limits, each violation failing with a message that names it: 1 <= B <= 65535; 1 <= C <= 128; 1 <= Tx <= 4096; 1 <= Ty <= 4096;
 *   metric 0 or 1; d_cost and d_steps non-NULL.
 * One kernel launch (dtw_kernel) on `stream`, one workgroup per row walking the tx + ty - 1 anti-diagonals: latency-bound like the alignment
 *   search.  The cell on the wavefront does the sequential loop's arithmetic, no atomics: a row alone, inside a batch, or as the length
 *   prefix of longer padded rows, and a second call, give the same bits.  The (B, Tx, Ty) cost matrix never exists in memory.
 * Scratch: none with d_path == NULL (ev_alloc_count never moves).  With a path, decision bits that do not fit in LDS (Tx * Ty / 4 bytes
 *   beside 30 Tx bytes of ring in 160 KiB) live in an arena of the handle that grows on demand like the alignment search's and counts in
 *   ev_alloc_count: a second call at the same shape allocates nothing; ev_reserve does not cover it.  No host wait and no copy: capturable
 *   once the arena has its size. */
int ev_dtw(ev_handle *h, const float *d_x /* (B, C, Tx) */, const float *d_y /* (B, C, Ty) */,
           const int32_t *d_xlen /* (B) or NULL */, const int32_t *d_ylen /* (B) or NULL */,
           int B, int C, int Tx, int Ty, int metric /* 0 Euclidean, 1 squared Euclidean */,
           double *d_cost /* (B) */, int32_t *d_steps /* (B) */,
           int32_t *d_path /* (B, Tx + Ty - 1, 2) or NULL */, void *stream);

/* Loudness on the device: ITU-R BS.1770-4 / EBU R 128 integrated loudness of mono rows (K-weighting, 400 ms blocks with 75 % overlap, an
 * absolute and a relative gate).  S = sub_len is the samples per 100 ms; NS = L / S (integer division) sub-blocks and NB = max(NS - 3, 0)
 * blocks per row of the outputs.  A row of len samples has ns = len / S complete sub-blocks and nb = max(ns - 3, 0) gating blocks; the
 * incomplete tail is discarded, as the standard says.  d_len == NULL: every row is L long.
 *   coef      HOST, 10 doubles, read during the call and passed to the kernels by value (no load step, no host-to-device copy: the call stays
 *             capturable once the arena has its size): {b0, b1, b2, a1, a2} of stage 1 (the high shelf), then of stage 2 (the high pass), a0 = 1.
 *             emojivoice_amd.audio.k_weighting(sr) designs them for any rate.  A stage is stable iff |a2| < 1 and |a1| < 1 + a2; an unstable
 *             (or non-finite) stage fails the call with a message naming it.  The kernel does not tie coef to S.
 *   filter    per stage y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2], every row from zero state, stage 2 on stage 1's output.
 *             Samples are widened to float64 and everything is float64; ev_set_arithmetic does not reach it.
 *   d_sub     (B, NS) float64 or NULL: e_i = sum of y^2 over samples [i S, (i + 1) S); 0 for i >= ns
 *   d_block   (B, NB) float64 or NULL: z_j = ((e_j + e_{j+1}) + (e_{j+2} + e_{j+3})) / (4 S), in exactly that association (one correctly rounded
 *             division by the double 4 S): bit-derivable from d_sub; 0 for j >= nb
 *   gates     in the power domain, strict: absolute z_j > abs_gate (the caller passes 10^((-70 + 0.691) / 10)); relative, additionally,
 *             z_j > 0.1 * m_abs, m_abs the mean of z over the blocks that pass the absolute gate (one multiply gives the -10 LU)
 *   d_gated   (B, 2) float64: {mean of z over the blocks passing both gates, m_abs}; 0 where the set is empty
 *   d_counts  (B, 3) int32: {nb, blocks passing the absolute gate, blocks passing both}
 *   The caller takes -0.691 + 10 log10(.) itself: there is no logarithm on the device.
 * A row with len < 1 or len > L is no error and no out-of-bounds access: all its outputs are zeros (the ev_mas_align convention).  Nothing at or
 * behind ns S is read, so nothing at or behind len is.
 * Limits, each violation failing with a message that names it: 1 <= B <= 65535; 16 <= sub_len <= 65536; L >= 1; d_gated and d_counts non-NULL.
 * Parallel in time: the 4th-order recurrence is not walked as one chain per row.  A row is cut into chunks of 1024 samples from its first sample.
 *   The filter's state is four doubles (transposed direct form II, two per stage) and the filter is linear, so the state after a chunk is
 *   (the state the chunk reaches from zero) + M (the state before it); M, the 4 x 4 zero-input transition over one chunk, is computed on the
 *   host in double by running the recurrence on the four unit states, and passed by value.  Launches: (1) one lane per (row, chunk) runs its
 *   chunk from zero state and keeps four doubles; (2) one wave per row carries s[c + 1] = M s[c] + z[c] in ascending c; (3) one lane per (row,
 *   chunk) reruns the chunk from its true state and sums y^2 (one fma per sample, ascending) per piece of a sub-block inside the chunk; (4) the
 *   pieces of a sub-block are added in ascending chunk order; (5) one workgroup per row forms blocks, gates and means.  The longest dependent
 *   chain per row is one chunk plus the carry (len / 1024 steps of one 4 x 4 product).  Samples reach the lanes through LDS tiles (a lane
 *   reading its own chunk would stride 4 KiB).
 *   Order of the two means: thread t of 256 adds its blocks j = t, t + 256, ... in ascending j, the 64 partials of a wave go through one fixed
 *   shuffle tree (offsets 32 .. 1), the four waves' sums are added as (w0 + w1) + (w2 + w3).
 *   No atomics, and the chunk grid hangs on the row's first sample: a row alone, inside a batch, or as the d_len prefix of a longer padded row
 *   with anything behind it, and a second call, give the same bits in every output.
 * Scratch: per (row, chunk) 4 + ((1024 + S - 2) / S + 1) doubles, plus B x NS doubles when d_sub is NULL, in an arena of the handle that grows on
 *   demand like the trim and DTW arenas and counts in ev_alloc_count: a second call at the same shape allocates nothing; ev_reserve does not
 *   cover it.  Five kernel launches on `stream` (one when L < S), no host wait, no copy. */
int ev_loudness(ev_handle *h, const float *d_x /* (B, L) */, const int32_t *d_len /* (B) or NULL */, int B, int L,
                int sub_len /* S: samples per 100 ms */, const double *coef /* HOST (10) */, double abs_gate /* mean square */,
                double *d_sub /* (B, NS) or NULL */, double *d_block /* (B, NB) or NULL */,
                double *d_gated /* (B, 2) */, int32_t *d_counts /* (B, 3) */, void *stream);

/* SRMR on the device: the speech-to-reverberation modulation energy ratio of mono rows (Falk, Zheng and Chan, IEEE TASLP 18(7), 2010), a
 * NON-INTRUSIVE measure: no clean reference.  A cochlear filterbank, the temporal envelope of every channel, a modulation filterbank over each
 * envelope, and the energy in the low modulation bands over the energy in the high ones.  ev_load_srmr stores the tables; ev_srmr measures rows that
 * are ALREADY at the rate the tables were designed for (emojivoice_amd.audio.srmr_tables designs them, audio.srmr resamples).  Everything is
 * float64, samples are widened, floating-point contraction is off (an fma only where one is written below); ev_set_arithmetic does not reach it.
 *
 * ev_load_srmr: HOST tables, copied to the device; N channels, K modulation bands, hop H, frame W = 4 H.  A second load replaces the first.
 *   chan    (N, 3)  {Re a, Im a, gain} per channel, |a| < 1
 *   mod     (K, 5)  {b0, b1, b2, a1, a2} per band, a0 = 1; stable iff |a2| < 1 and |a1| < 1 + a2 (ev_loudness's rule and message)
 *   window  (W)     the frame window
 *   erb     (N)     the bandwidth of every channel, channels ascending in frequency
 *   cutoff  (K)     the lower edge of every band
 * Limits, each violation failing with a message that names it: 1 <= N <= 32; 1 <= K <= 8; H a multiple of 64 with 64 <= H <= 1024; every table
 * finite and non-NULL.
 *
 * DEFINITION.  x[n] is a row's sample n as a double.
 *   channel   a fourth-order complex gammatone (Hohmann, Acta Acustica 88, 2002): four cascaded one-pole stages s_k[n] = v_{k-1}[n] + a s_k[n-1],
 *             v_0 = x, v_k = s_k (the value of THIS sample), every row from zero state.  Written out in reals, s = (r, i), a = (ar, ai):
 *                 r' = v_r + (ar r - ai i);   i' = v_i + (ar i + ai r)        (stage 1, whose input is real: i' = ar i + ai r)
 *             with every product rounded, then the inner sum or difference, then the outer sum.
 *   envelope  e[n] = gain * sqrt(r4 r4 + i4 i4).  The analytic filter yields the envelope with no Hilbert transform over the whole row: a stated
 *             deviation from SRMRpy's real ERB filterbank and FFT Hilbert transform.  Absolute values are this definition's own.
 *   bands     per band the biquad in transposed direct form II on e, from zero state, with ev_loudness's fmas:
 *                 m = fma(b0, e, s1);   s1 = fma(-a1, m, fma(b1, e, s2));   s2 = fma(-a2, m, b2 e)
 *   frames    frame f covers samples [f H, f H + W); nf = (len - W) / H + 1 for len >= W, else 0; NF is the same of L.  Nothing at or behind
 *             (nf + 3) H <= len is read.  E[f, j, k] = sum over t of (window[t] m_k[f H + t])^2.
 * PARALLEL IN TIME (the bits depend on it).  A row is cut into chunks of H samples from its first sample; the nf + 3 chunks of a row are all
 *   whole.  The state at a chunk's start is carried in ascending chunk order as s[c + 1] = M s[c] + z[c]: z[c] the state chunk c reaches from zero,
 *   M the zero-input transition over H samples, computed by ev_load_srmr on the host in double by running the recurrences above on unit states
 *   (4 x 4 complex lower triangular per channel, 2 x 2 per band).  Channel row r: from z[r], for k = 0 .. r: re = re + (Mre sre - Mim sim),
 *   im = im + (Mre sim + Mim sre).  Band: s1' = (z1 + M00 s1) + M01 s2, s2' = (z2 + M10 s1) + M11 s2.  Inside a chunk the recurrences run
 *   sequentially from the carried state.  The envelope is not linear in the channel state, so there are three passes over the samples with a carry
 *   between each pair: channels from zero; channels true and bands from zero; everything true.  In the last pass chunk c leaves per (channel,
 *   band) four sums p[c, q] = sum over its samples t of (window[q H + t] m)^2, q = 0 .. 3, each from 0 by acc = fma(v, v, acc), v the rounded
 *   product, in ascending t.  E[f] = ((p[f, 0] + p[f + 1, 1]) + (p[f + 2, 2] + p[f + 3, 3])).
 * PER ROW, sequentially, no atomics:
 *   Em[j, k]  the sum of E[f, j, k] over ascending f from 0, divided by nf
 *   shares    ch[j] = sum of Em[j, k] over ascending k; total = sum of ch[j] over ascending j; cum = cum + ch[j] / total over ascending j
 *   j90       the first channel at which cum > 0.9 (N - 1 when none does: silence);  bw = erb[j90]
 *   K*        min(K, max(min(5, K), #{k : cutoff[k] < bw}))
 *   ratio     (sum over ascending j, then ascending k < min(4, K), of Em) / (the same over 4 <= k < K*), one accumulator each; 0 where the
 *             denominator is 0 or K <= 4 (the caller makes NaN of it)
 * Outputs of ev_srmr:
 *   d_frame   (B, NF, N, K) float64 or NULL: E[f, j, k]; 0 for f >= nf
 *   d_mean    (B, N, K) float64: Em
 *   d_srmr    (B, 2) float64: {ratio, bw}
 *   d_counts  (B, 3) int32: {nf, j90, K*}
 * A row with len < W or len > L is no error and no out-of-bounds access: all its outputs are zeros.  d_len == NULL: every row is L long.
 * Limits of ev_srmr, each violation failing with a message that names it: tables loaded; 1 <= B <= 65535; L >= 1; d_x, d_mean, d_srmr and d_counts
 * non-NULL.  A failed call writes nothing and leaves ev_alloc_count unmoved.
 * Scratch: per (row, chunk) 8 N + 6 N K doubles in an arena of the handle that grows on demand and counts in ev_alloc_count: a second call at the
 *   same shape allocates nothing; ev_reserve does not cover it.  Six kernel launches on `stream` (one when L < W), no host wait, no copy: the call
 *   is capturable once the arena has its size.
 * The same inputs give the same bits in every output: a row alone, inside a batch, as the d_len prefix of a longer row with anything (NaN
 *   included) behind it, in a second call, under every ev_set_arithmetic setting, and from a captured graph. */
int ev_load_srmr(ev_handle *h, const double *chan /* HOST (N, 3) */, const double *mod /* HOST (K, 5) */, const double *window /* HOST (4 H) */,
                 const double *erb /* HOST (N) */, const double *cutoff /* HOST (K) */, int N, int K, int H);
int ev_srmr(ev_handle *h, const float *d_x /* (B, L) */, const int32_t *d_len /* (B) or NULL */, int B, int L,
            double *d_frame /* (B, NF, N, K) or NULL */, double *d_mean /* (B, N, K) */, double *d_srmr /* (B, 2) */,
            int32_t *d_counts /* (B, 3) */, void *stream);

/* Speech rate and pauses on the device: the syllable nuclei of mono rows after De Jong and Wempe (Behavior Research Methods 41, 2009): a power
 * contour, a sounding / silent segmentation with minimum durations, and the local peaks of the power that are followed by a dip and are voiced.
 * No transcript and no alignment.  ev_load_speech_rate stores the window; ev_speech_rate measures on the grid of ev_pitch_yin and ev_formants, so
 * frame f of every contour is the same frame.  Everything is float64, the fp32 samples are widened, floating-point contraction is off;
 * ev_set_arithmetic does not reach it.
 *
 * ev_load_speech_rate: HOST window of W doubles, copied to the device; hop H.  Limits, each violation failing with a message that names it: window
 * non-NULL and finite with sw > 0; 8 <= W <= 4096, W even; H a multiple of 64 with 64 <= H <= 1024 (W need not be a multiple of H).  The load owns
 * one device block and counts once in ev_alloc_count; loading again waits for the device and drops the old block; a failed load leaves the previous
 * tables in use.
 *
 * DEFINITION.  NF = ceil(L / H); a row of len samples has nf = ceil(len / H) frames.  d_len == NULL: every row is L long.
 *   power     s_f[j] = x[f H + H/2 - W/2 + j] for j = 0 .. W-1, zero outside [0, len).  sw = sum of w[j], formed once on the host in ascending j.
 *             m = (sum w[j] s_f[j]) / sw (Praat's "subtract mean");  P[f] = (sum w[j] (s_f[j] - m)^2) / sw.  The terms are the rounded products
 *             w[j] s and w[j] ((s - m)(s - m)).  Both sums use the 64-slot rule of ev_modulation: term j belongs to slot j mod 64, a slot starts at
 *             +0.0 and adds its terms in ascending j, and the 64 slots are reduced by the xor tree with offsets 32, 16, 8, 4, 2, 1.  The order
 *             depends on the frame's own samples and the loaded window only.
 *   decisions are made on P, in the power domain: the thresholds arrive as ratios (the host forms silence_ratio = 10^(-silence_db / 10) and
 *             dip_ratio = 10^(dip_db / 10)) and no decision passes through a logarithm, so a restatement that adds in the same order takes the
 *             same decisions.
 *   level     k = floor(rank_fraction * (double)(nf - 1)), one rounded product; ref is the (k + 1)-th largest of P[0 .. nf): rank_fraction = 0 is
 *             the maximum, 0.01 the script's 99 % quantile without interpolation.  P >= 0 (for a window without negative entries), so its bit
 *             pattern orders as an unsigned 64-bit integer, and the selection counts bits: no float arithmetic.  thr = ref * silence_ratio.
 *   sounding  raw[f] = P[f] > thr and P[f] > power_floor.  (a) every maximal run of non-raw frames of length < min_pause becomes sounding, if raw
 *             frames lie on both of its sides; (b) then every maximal sounding run of length < min_sound becomes silent: snd[f].  A PAUSE is a
 *             maximal silent run with sounding frames on both sides; the leading and the trailing silent run are counted on their own, and a row
 *             without a sounding frame is all leading silence, so sounding + pause + leading + trailing frames = nf.
 *   candidate 1 <= f <= nf - 2, P[f] > P[f-1] and P[f] >= P[f+1] (ev_perturbation's local-peak rule), P[f] > thr, snd[f]:  c_0 < c_1 < ...
 *   nucleus   for candidate c_i let e = c_{i+1}, and e = nf for the last one (the published script never counts its last peak: a stated
 *             difference).  d = min P over (c_i, e); the candidate has its DIP when d * dip_ratio <= P[c_i], one product.  An empty interval has
 *             no dip (under the peak rule frame c_i + 1 is never a candidate, so the interval holds at least that frame).  A candidate with its
 *             dip is a NUCLEUS when d_voiced is NULL or d_voiced[b, c_i] != 0.
 * Outputs:
 *   d_power   (B, NF) float64 or NULL: P, zeros at and past nf
 *   d_mark    (B, NF) uint8 or NULL: bit 0 snd, bit 1 raw, bit 2 candidate, bit 3 nucleus; zeros past nf
 *   d_count   (B, 8) int32: {nf, sounding frames, pauses, pause frames, candidates, nuclei, leading silent frames, trailing silent frames}
 *   d_stat    (B, 4) float64: {ref, thr, mean, sd of the pause lengths in frames}; mean and sd by ev_functionals' integer formula (S1, S2 in
 *             64-bit integers, then one conversion: S1 / n, sqrt(n S2 - S1 S1) / n); both 0 without a pause
 * A row with len < 1 or len > L is no error and no out-of-bounds access: zeros in every output.  Nothing at or behind len is read; d_voiced is
 * read only at candidates with their dip, inside nf.  Nothing depends on B, L, NF or the place in the grid: the same inputs give the same bits in
 * every output for a row alone, inside a batch, as the d_len prefix of a longer row with anything (NaN included) behind it, in a second call,
 * under every ev_set_arithmetic setting, and from a captured graph.
 * Limits of ev_speech_rate, each violation failing with a message that names it, the call writing nothing: tables loaded; 1 <= B <= 65535; L >= 1
 * and NF <= 16384 (the row's power stays in LDS); power_floor finite and > 0; 0 <= rank_fraction < 1; 0 < silence_ratio < 1; dip_ratio finite and
 * >= 1; 1 <= min_pause, min_sound <= 4096; d_x, d_stat and d_count non-NULL.
 * Scratch: without d_power the power contour (B x NF doubles) lives in an arena of the handle that grows on demand and counts in ev_alloc_count: a
 *   second call at the same shape allocates nothing; ev_reserve does not cover it.  Two kernel launches on `stream`, no atomics, no host wait, no
 *   copy: the call is capturable once the arena has its size. */
int ev_load_speech_rate(ev_handle *h, const double *window /* HOST (W) */, int W, int H);
int ev_speech_rate(ev_handle *h, const float *d_x /* (B, L) */, const int32_t *d_len /* (B) or NULL */,
                   const uint8_t *d_voiced /* (B, NF) or NULL */, int B, int L,
                   double power_floor, double rank_fraction, double silence_ratio, double dip_ratio,
                   int min_pause, int min_sound,
                   double *d_power /* (B, NF) or NULL */, uint8_t *d_mark /* (B, NF) or NULL */,
                   double *d_stat /* (B, 4) */, int32_t *d_count /* (B, 8) */, void *stream);

/* Spectral envelope and mel-cepstrum on the device: the f0-adaptive envelope of CheapTrick (Morise, Speech Communication 67, 2015), the envelope
 * WORLD uses, and its frequency-warped cepstrum by the recursion of SPTK's freqt, per frame of ev_voice_quality's grid, the period of every frame
 * coming from ev_pitch_yin's d_period.  pyworld and pysptk are NOT the yardstick: the published algorithms are the model and the definition below
 * is what the device is held to (tests/envelope_ref.py restates it in numpy float64).  Everything is float64, the fp32 samples and periods are
 * widened, floating-point contraction is off; ev_set_arithmetic does not reach it.
 *
 * ev_load_envelope: HOST twiddle (nfft, 2) {cos, sin}(2 pi n / nfft); hop H; the rate sr in Hz; default_period in samples (0: sr / 500, WORLD's
 * default f0); the lifter's q1 (CheapTrick: -0.15); HOST warp (n_mcep, NB), the matrix A of step 7 (NB = nfft / 2 + 1).  Limits, each violation
 * failing with a message that names it: twiddle and warp non-NULL and finite; nfft even with 16 <= nfft <= 1024; 1 <= H <= 512 (the DFT families'
 * rule); 1 <= n_mcep <= 64; sr finite and > 0; q1 and default_period finite; 2 <= default_period <= T_max; the two launches' LDS (16 S1 and 32 S
 * doubles, S1 and S the row strides: 131 328 and 131 584 bytes at nfft = 1024) at most 160 KiB.  The load owns one device block (the plain DFT
 * basis, the cepstral basis, the warp table) and counts once in ev_alloc_count; loading again waits for the device and drops the old block; a
 * failed load leaves the previous tables in use.
 *
 * DEFINITION.  NF = ceil(L / H); a row of len samples has nf = ceil(len / H) frames; a row with len < 1 or len > L is empty.  d_len == NULL: every
 * row is L long.  Frame f is centred at sample c = f H + H / 2.  T = (double)d_period[b, f]; if T is not > 0 (unvoiced, NaN), T < T_min = 2 or
 * T > T_max = (nfft - 3) / 3 (CheapTrick's f0 floor 3 sr / (nfft - 3)), then T = default_period and the frame's class is 1.  Every integer below is
 * formed from T by exactly the stated float64 expression.
 *   1 window    half = floor(1.5 T + 0.5); w[j] = 0.5 cospi(j / (1.5 T)) + 0.5 for -half <= j <= half.  x[c + j] is 0 outside [0, len) (WORLD
 *               repeats the edge sample; this project pads with zeros, as its other frame families do).  With the three sums sum w w, sum w and
 *               sum x w, each over the 64-slot rule (term i = j + half belongs to slot i mod 64, ascending in a slot, then the xor tree with offsets
 *               32 .. 1): s[j] = (x w - w ((sum x w) / (sum w))) / sqrt(sum w w): the window has unit energy and the weighted mean is removed.
 *               WORLD's random safeguard noise is left out: the output is deterministic.
 *   2 power     P[k] = |DFT_nfft(s)|^2 = fma(im, im, re re), k = 0 .. NB - 1.  A frame with no P[k] > power_floor is SILENT (class 2): its d_env
 *               and d_mcep are zeros.
 *   3 DC        rn = nfft / T, kd = floor(rn).  For 0 <= k <= kd: u = rn - k, i = floor(u), P'[k] = P[k] + (P[i] (1 - (u - i)) + P[min(i + 1,
 *               NB - 1)] (u - i)), the interpolation reading the uncorrected P.  P'[k] = P[k] for every other k.
 *   4 smoothing wd = (2 nfft) / (3 T) bins (2 f0 / 3).  S[k] = (1 / wd) times the integral over [lo, hi) = [k - wd / 2, k + wd / 2) of the
 *               piecewise-constant P', cell i covering [i - 1/2, i + 1/2), an index i < 0 reading -i and i > nfft / 2 reading nfft - i.  With
 *               ilo = floor(lo + 0.5) and ihi = floor(hi + 0.5): P'[ilo] (hi - lo) if ilo == ihi, else P'[ilo] ((ilo + 0.5) - lo), plus P'[i] for
 *               ilo < i < ihi in ascending order, plus P'[ihi] (hi - (ihi - 0.5)); then one division by wd.  WORLD takes the same integral as a
 *               difference of cumulative sums; the direct sum adds positive terms only, so no weak bin is lost to cancellation.
 *   5 lifter    Lg[k] = log(max(S[k], power_floor));  c^[q] = sum_k Lg[k] (g[k] cos(2 pi k q / nfft) / nfft), q = 0 .. nfft / 2, g = 1 at k = 0 and
 *               k = nfft / 2, else 2 (ev_voice_quality's cepstral table at q_fit = 0);  c'[q] = (c^[q] sinc) comp with x = q / T,
 *               sinc = sinpi(x) / (pi x) (1 at q = 0) and comp = (1 - 2 q1) + (2 q1) cospi(2 x).
 *   6 envelope  Le[k] = nfft sum_q c'[q] (g[q] cos(2 pi q k / nfft) / nfft): the log POWER envelope in nepers (d_env; 10 / ln 10 times it is dB).
 *   7 mcep      c[0] = c'[0] / 2, c[m] = c'[m]: SPTK's one-sided cepstrum of the log AMPLITUDE.  mc = A c, A (n_mcep, NB) the matrix of freqt at
 *               alpha: column n is the result of the recursion on the unit vector e_n: for i = N down to 0, with d = g saved from the previous
 *               pass: g[0] = c[i] + alpha d[0]; g[1] = (1 - alpha^2) d[0] + alpha d[1]; g[m] = d[m-1] + alpha (d[m] - g[m-1]) for m >= 2.
 *               (alpha = 0.455 suits 22.05 kHz.)  The host builds A in float64; the load folds the halving of c[0] into its copy.
 * The sums over k and q are matrix products on v_mfma_f64_16x16x4_f64, K ascending in steps of 4.
 * Outputs:
 *   d_env     (B, NF, NB) float64 or NULL: Le
 *   d_mcep    (B, NF, n_mcep) float64: mc
 *   d_class   (B, NF, 3) int32: {class, half, kd}; class 0 voiced (T from d_period), 1 default period, 2 silent (half and kd as computed),
 *             3 beyond the row ({3, 0, 0})
 * Frames at and past nf are zeros in d_env and d_mcep.  Nothing at or behind len is read, of d_x or of d_period's frames past nf.  Nothing depends
 * on B, L or the place in the grid: the same inputs give the same bits for a row alone, inside a batch, at a larger L, in a second call, under
 * every ev_set_arithmetic setting and from a captured graph.
 * Limits of ev_envelope, each violation failing with a message that names it, the call writing nothing: tables loaded; 1 <= B <= 65535; L >= 1;
 * d_x, d_period, d_mcep and d_class non-NULL; power_floor finite and > 0.
 * Scratch: the power spectra (B x NF x NB doubles: 135 MB at 64 rows of 6 s) live in an arena of the handle that grows on demand and counts in
 *   ev_alloc_count: a second call at the same shape allocates nothing; ev_reserve does not cover it.  Two kernel launches on `stream`, no atomics,
 *   no host wait, no copy: the call is capturable once the arena has its size. */
int ev_load_envelope(ev_handle *h, const double *twiddle /* HOST (nfft, 2) */, int H, int nfft, double sr, double default_period, double q1,
                     const double *warp /* HOST (n_mcep, nfft / 2 + 1) */, int n_mcep);
int ev_envelope(ev_handle *h, const float *d_x /* (B, L) */, const int32_t *d_len /* (B) or NULL */, const float *d_period /* (B, NF) */,
                int B, int L, double power_floor, double *d_env /* (B, NF, NB) or NULL */, double *d_mcep /* (B, NF, n_mcep) */,
                int32_t *d_class /* (B, NF, 3) */, void *stream);

/* Time stretching on the device: the phase vocoder.  ev_load_phase_vocoder stores the tables of one nfft; ev_phase_vocoder renders every row of a
 * batch `rate` times faster (rate > 1) or slower (rate < 1) at its own pitch.  The model is librosa.stft -> librosa.phase_vocoder -> librosa.istft
 * (librosa 0.10 defaults: center=True with zero padding, periodic Hann, hop nfft / 4); librosa is NOT the yardstick: the definition below is what
 * the device is held to, and tests/phase_vocoder_ref.py restates it in numpy (float64 and longdouble).  Everything is float64, the fp32 samples
 * are widened, floating-point contraction is off; ev_set_arithmetic does not reach it.  A pitch shift is a stretch followed by ev_resample.
 *
 * ev_load_phase_vocoder: HOST window (nfft) float64 (the periodic Hann window for the model), HOST twiddle (nfft, 2) {cos, sin}(2 pi n / nfft).
 * Limits, each violation failing with a message that names it: window and twiddle non-NULL and finite; nfft a multiple of 16 with
 * 16 <= nfft <= 2048.  The load owns one device block (the windowed DFT basis (nfft, NB), the inverse basis (NBp, nfft), w / nfft and w^2; NBp the
 * next multiple of 4 from NB: 67 MB at nfft = 2048, 17 MB at 1024) and counts once in ev_alloc_count; loading again waits for the device and
 * drops the old block; a failed load leaves the previous tables in use.
 *
 * DEFINITION.  W = nfft, H = nfft / 4, NB = nfft / 2 + 1.  A row of n = len samples has nf = 1 + n / H frames (integer division); NF = 1 + L / H.
 * d_len == NULL: every row is L long.  A row with len < 1 or len > L is empty: its outputs are zeros, its out_len and counts 0.
 *   analysis    frame f reads t_j = x[f H - nfft / 2 + j], 0 <= j < nfft, zeros outside [0, n).  re_k = sum_j t_j w_j cos(2 pi j k / nfft),
 *               im_k = -sum_j t_j w_j sin(2 pi j k / nfft) (matrix products on v_mfma_f64_16x16x4_f64, j ascending in steps of 4, the phase index
 *               (j k) mod nfft in exact integers, w_j cos and w_j sin rounded once); mag = sqrt(fma(im, im, re re)), ang = atan2(im, re) with the
 *               device library's float64 functions (atan2(0, 0) = 0).  Every frame >= nf is all zeros (two of them are read at most).
 *   time steps  n_out = ceil((double)nf / rate); s_t = (double)t rate (ONE float64 product), i_t = floor(s_t), a_t = s_t - i_t.  The steps are part
 *               of the definition and they are float64: a restatement in higher precision takes s_t as given (t 1.7 floors differently in long
 *               double and then selects another frame).
 *   propagation per bin k, in ascending t, sequentially, with omega_k = (2 pi (H k)) / nfft and 2 pi = 6.283185307179586:  phi_0 = ang[0][k];
 *               Y_t[k] = ((1 - a_t) mag[i_t][k] + a_t mag[i_t + 1][k]) (cos phi_t, sin phi_t) — the phasor is formed before the phase moves on;
 *               d = ang[i_t + 1][k] - ang[i_t][k] - omega_k;  d = d - 2 pi rint(d / 2 pi);  phi_{t+1} = phi_t + (omega_k + d).
 *   synthesis   g_t[j] = (w_j / nfft) sum_k c_k (Re Y_t[k] cos(2 pi j k / nfft) - Im Y_t[k] sin(2 pi j k / nfft)), c_0 = c_{NB-1} = 1, c_k = 2
 *               otherwise, the imaginary parts of DC and Nyquist ignored (irfft); two matrix products, k ascending in steps of 4 (the cosine
 *               terms, the sine terms), added once.  In padded coordinates p = i + nfft / 2: num[p] = sum_t g_t[p - t H] and wss[p] = sum_t
 *               w[p - t H]^2 over the frames 0 <= t < n_out that cover p, in ascending t.  y[i] = num / wss where wss > FLT_MIN, else num.
 *               out_len = (int)rint((double)n / rate); y[i] = 0 for i >= min(out_len, H (n_out - 1) + nfft / 2).  Rounded once to float32.
 * L_out must be rint(L / rate); NO = ceil(NF / rate).
 * Outputs:
 *   d_y        (B, L_out) float32: the stretched rows, zeros from the row's own end on
 *   d_out_len  (B) int32: out_len
 *   d_counts   (B, 2) int32 or NULL: {nf, n_out}
 *   d_stretch  (B, NO, NB, 2) float64 or NULL: Y as {re, im}, zeros at t >= n_out
 * Nothing at or behind len is read.  Nothing depends on B, L or the place in the grid: the same samples give the same bits for a row alone, inside
 * a batch, as the d_len prefix of a longer row with anything behind it, and in a second call.  A row of one sample is a valid row.
 * Limits of ev_phase_vocoder, each violation failing with a message that names it, the call writing nothing: tables loaded; 1 <= B <= 65535;
 * L >= 1; rate finite with 0.125 <= rate <= 8; L_out == rint(L / rate); d_x, d_y and d_out_len non-NULL; the scratch of the call at most 4 GiB
 * (the message names the figure; the caller splits the batch).
 * Kernels: pv_analysis_kernel, one workgroup per (row, 16 frames): the span staged once in LDS as fp32, the DFT GEMM of ev_stft_dist for one
 *   signal; pv_propagate_kernel, one thread per (row, bin), the loads of step t + 1 issued ahead of step t's sine and cosine; pv_synthesis_kernel,
 *   one workgroup per (row, 16 output frames): it owns the 13 hop segments those frames cover completely, the column tiles ordered (j mod H,
 *   quarter) so that the four terms of a sample meet inside one wave's accumulators, crossing through 8.5 KB of LDS; edge tiles add the frames that
 *   exist.  One fixed order, no atomics.
 * Scratch: mag and ang (2 x B x NF x NB doubles) and, without d_stretch, Y (B x NO x NB pairs: 0.7 GB together at 64 rows of 6 s, rate 0.8) live
 *   in an arena of the handle that grows on demand and counts in ev_alloc_count: a second call at the same shape allocates nothing; ev_reserve
 *   does not cover it.  Three kernel launches on `stream`, no host wait, no copy: the call is capturable once the arena has its size. */
int ev_load_phase_vocoder(ev_handle *h, const double *window /* HOST (nfft) */, const double *twiddle /* HOST (nfft, 2) */, int nfft);
int ev_phase_vocoder(ev_handle *h, const float *d_x /* (B, L) */, const int32_t *d_len /* (B) or NULL */, int B, int L, double rate,
                     float *d_y /* (B, L_out) */, int L_out, int32_t *d_out_len /* (B) */, int32_t *d_counts /* (B, 2): nf, n_out; or NULL */,
                     double *d_stretch /* (B, NO, NB, 2): Y, zeros at t >= n_out; or NULL */, void *stream);

/* STOI and ESTOI on the device: short-time objective intelligibility of a processed row y against the clean, sample-aligned row x (Taal,
 * Hendriks, Heusdens and Jensen, IEEE TASL 19(7), 2011) and its extended form (Jensen and Taal, IEEE/ACM TASLP 24(11), 2016), for rows already
 * at the measure's rate (10 kHz in the papers).  ev_load_stoi stores the tables; ev_stoi measures.  Everything is float64 (the samples are
 * widened), in ONE fixed order, stated below; the kernels are compiled with floating-point contraction off, so "fma" below is an fma and every
 * other product or sum is rounded on its own.  No atomics; ev_set_arithmetic does not reach it.
 * ev_load_stoi: HOST tables, copied to the device.  window (W) doubles w; twiddle (nfft, 2) doubles {cos, sin}(2 pi n / nfft); bands (n_bands, 2)
 *   int32 {first bin, end bin (exclusive)}; H the hop, N the frames per segment.  Limits, each violation failing with a message that names it:
 *   H a multiple of 32 with 32 <= H <= 256; W = 2 H (the overlap-add below has exactly two terms); W <= nfft <= 1024; 1 <= n_bands <= 32;
 *   0 <= first < end <= nfft / 2 + 1 for every band; 2 <= N <= 64; finite window and twiddle; non-NULL tables.  Loading again replaces the
 *   tables; it waits for the device first.  ev_stoi without loaded tables fails with a message.
 * Sizes, with frames(n) = n > W ? ceil((n - W) / H) : 0 (the model frames with range(0, len - W, H): a row of exactly W + k H samples has k
 *   frames, not k + 1): NF = frames(L), NM = max(NF - 1, 0), NSEG = max(NM - N + 1, 0); a row of len samples has nf = frames(len).
 *   d_len == NULL: every row is L long.  EPS = 2^-52.
 * Definition, per row:
 *   energies  E[f] = the fma chain e = fma(t_j, t_j, e) over ascending j from 0 with t_j = w[j] * x[f H + j], for f < nf: the clean signal only
 *   mask      frame f is kept iff E[f] > silence_ratio * max_f E[f]: one multiply, strict, in the power domain (the caller passes 10^(-40/10)).
 *             This is the model's 20 log10(norm + EPS) test without the logarithms; the two differ only for an all-zero clean row, of which the
 *             device keeps NO frame (the model would keep all of them).  idx[k] = the k-th kept frame, ascending; nk their number.
 *             d_keep (B, NF) uint8 or NULL: 1 for a kept frame, 0 otherwise and for f >= nf
 *   signals   s[n] = sum over k in {n / H - 1, n / H} with 0 <= k < nk of w[n - k H] * x[idx[k] H + n - k H], every product rounded, added in
 *             ascending k, for 0 <= n < (nk - 1) H + W; the same idx for y.  s is never stored: frame m of s gathers from kept frames
 *             m - 1, m and m + 1 of the input
 *   spectra   nm = max(nk - 1, 0) frames; z_m[j] = w[j] * s[m H + j]; for every bin k from the lowest first to the highest end of the bands:
 *             re_k = fma(z_m[j], cos[(j k) mod nfft], re_k) and sm_k = fma(z_m[j], sin[(j k) mod nfft], sm_k) over ascending j from 0,
 *             im_k = -sm_k, p_k = fma(im_k, im_k, re_k * re_k); tob[band, m] = sqrt(p_k added over the band in ascending k from 0), the square
 *             root correctly rounded.  d_tob (B, 2, n_bands, NM) or NULL: [b][0] of x, [b][1] of y; zeros at m >= nm
 *   segments  nseg = max(nm - N + 1, 0); segment q covers frames [q, q + N); X, Y the N values of one band.  Every sum runs in ascending index
 *             from 0, sums of squares as fma(a, a, sum).
 *             STOI, per band: a = sqrt(sum X^2) / (sqrt(sum Y^2) + EPS); Y' = min(a * Y, clip * X) element-wise (the caller passes
 *             clip = 1 + 10^(15/20)); mx = (sum X) / N, my = (sum Y') / N; dx = sqrt(sum (X - mx)^2) + EPS, dy alike of Y' - my;
 *             rho = sum of ((X - mx) / dx) * ((Y' - my) / dy).  d_seg[q][0] = (sum of rho over the bands in ascending order) / n_bands.
 *             ESTOI, X and Y alike: every band's mean over the N frames ((sum) / N) removed, then divided by (sqrt(sum of squares) + EPS); then
 *             every frame's mean over the bands ((sum) / n_bands) removed, then divided by (sqrt(sum of squares) + EPS); c_i = fma(X[r][i],
 *             Y[r][i], c_i) over the bands r; d_seg[q][1] = (sum of c_i over the frames i) / N.
 *             d_seg (B, NSEG, 2) or NULL; zeros at q >= nseg
 *   scores    d_score (B, 2) = {STOI, ESTOI}: the mean of each column of d_seg over the nseg segments, 0 when nseg = 0.  Thread t of 256 adds its
 *             segments t, t + 256, ... in ascending order, the 64 partials of a wave go through one shuffle tree (offsets 32 .. 1), the four
 *             waves' sums are added as (w0 + w1) + (w2 + w3) (the tree of ev_loudness); one division by nseg follows.
 *   d_counts  (B, 3) int32: {nf, nk, nseg}
 * A row with len < 1 or len > L is no error and no out-of-bounds access: all its outputs are zeros (the ev_mas_align convention); so are those
 * of an all-zero clean row, except nf.  Nothing at or behind len is read, and nothing depends on the batch or on L: a row alone, inside a batch,
 * or as the d_len prefix of a longer padded row with anything behind it, and a second call, give the same bits in every output.
 * Limits of ev_stoi, each violation failing with a message that names it and writing nothing: 1 <= B <= 65535; L >= 1; 0 < silence_ratio < 1;
 * clip > 1; d_x, d_y, d_score and d_counts non-NULL.
 * Kernels (five launches on `stream`, fewer where NF, NM or NSEG is 0; no host wait, no copy): (1) one lane per (row, frame): E; (2) one workgroup per
 *   row: the maximum of E — taken here, not in (1), since a maximum is exact in any order and this needs no atomics — the mask, and idx by
 *   a ballot and popcount prefix per wave, 256 frames per round with the base carried across rounds; d_keep and d_counts; (3) one workgroup per
 *   (row, frame m) for BOTH signals, which share every twiddle read: z through LDS, one lane per bin, then one lane per band; (4) one wave per
 *   (row, segment) with the segment in LDS: one lane per band for STOI, one lane per band and then one lane per frame for ESTOI; (5) one
 *   workgroup per row: the two means.  The DFT is a vector float64 fma chain, not the matrix core.
 * Scratch: B x NF doubles of E and B x NF int32 of idx, plus B x 2 x n_bands x NM doubles when d_tob is NULL and B x NSEG x 2 when d_seg is
 *   NULL, in an arena of the handle that grows on demand like the loudness arena and counts in ev_alloc_count: a second call at the same
 *   shape allocates nothing; ev_reserve does not cover it.  The call is capturable once the arena has its size. */
int ev_load_stoi(ev_handle *h, const double *window /* HOST (W) */, const double *twiddle /* HOST (nfft, 2): cos, sin of 2 pi n / nfft */,
                 const int32_t *bands /* HOST (n_bands, 2): first bin, end bin (exclusive) */,
                 int W, int H, int nfft, int n_bands, int N /* frames per segment */);
int ev_stoi(ev_handle *h, const float *d_x /* (B, L) clean */, const float *d_y /* (B, L) processed */, const int32_t *d_len /* (B) or NULL */,
            int B, int L, double silence_ratio /* 10^(-40/10) */, double clip /* 1 + 10^(15/20) */,
            uint8_t *d_keep /* (B, NF) or NULL */, double *d_tob /* (B, 2, n_bands, NM) or NULL */, double *d_seg /* (B, NSEG, 2) or NULL */,
            double *d_score /* (B, 2): STOI, ESTOI */, int32_t *d_counts /* (B, 3): nf, nk, nseg */, void *stream);

/* STFT distance at one resolution on the device: the terms of the multi-resolution STFT distance (spectral convergence and log-magnitude L1;
 * Yamamoto, Song and Kim, "Parallel WaveGAN", ICASSP 2020) and of the log-spectral distance in dB, of a processed row y against the
 * sample-aligned reference row x.  ev_load_stft_dist stores one resolution (window, hop, n_fft); ev_stft_dist measures; a caller that wants
 * the multi-resolution figure holds one handle per resolution and averages.  Everything is float64 (the fp32 samples are widened), the kernels
 * are compiled with floating-point contraction off; no atomics; ev_set_arithmetic does not reach it.
 * ev_load_stft_dist: HOST tables.  window (W) doubles w; twiddle (nfft, 2) doubles {cos, sin}(2 pi n / nfft); H the hop.  Limits, each
 *   violation failing with a message that names it: nfft even with 16 <= nfft <= 2048; W a multiple of 4 with 4 <= W <= nfft; nfft - W even;
 *   1 <= H <= 512 (any integer); finite, non-NULL tables.  With off = (nfft - W) / 2 and NB = nfft / 2 + 1 the handle builds the dense basis
 *     c[j][k] = w[j] * cos_tab[((j + off) k) mod nfft],  s[j][k] = w[j] * sin_tab[((j + off) k) mod nfft],  0 <= j < W, 0 <= k < NB,
 *   on the device at load time: each entry rounded once, the index in exact integer arithmetic (torch.stft with `window` zero-padded
 *   centrally to n_fft).  It takes 16 W NB bytes (33.6 MB at W = nfft = 2048) and counts once in ev_alloc_count.  Loading again replaces the
 *   basis; it waits for the device first.  ev_stft_dist without a loaded basis fails with a message.
 * Sizes, with frames(n) = n > nfft / 2 ? 1 + n / H : 0 (torch's reflect padding of nfft / 2 needs more samples than that): NF = frames(L); a
 *   row of len samples has nf = frames(len).  d_len == NULL: every row is L long.
 * Definition, per row:
 *   framing   frame f reads t_j = x[refl(f H - W / 2 + j)] for 0 <= j < W; refl(i) = -i for i < 0, 2 (len - 1) - i for i >= len, i otherwise
 *             (center=True, pad_mode="reflect"; one reflection suffices because len > nfft / 2 >= W / 2); y alike
 *   spectra   re_k = sum_j t_j c[j][k], sm_k = sum_j t_j s[j][k] for 0 <= k < NB; p_k = max(fma(sm_k, sm_k, re_k * re_k), power_floor);
 *             m_k = sqrt(p_k), correctly rounded; l_k = log(p_k), the device library's float64 natural logarithm.  The sums over j run on
 *             v_mfma_f64_16x16x4_f64 in steps of four j from 0; the order inside the instruction is the hardware's: fixed, not spelled out
 *   d_frame   (B, NF, 4) or NULL: [b][f] = {sum_k (my_k - mx_k)^2, sum_k mx_k^2, sum_k |ly_k - lx_k|, sum_k (ly_k - lx_k)^2} over the NB bins,
 *             squares added as fma(d, d, sum); bins k = 16 (w + 4 i) + c are added per (w, c) in ascending i, then over c by an xor tree
 *             (offsets 8, 4, 2, 1), then over w as ((w0 + w1) + w2) + w3.  Zeros at f >= nf
 *   d_sums    (B, 4) = {sum_f [0], sum_f [1], sum_f [2], sum_f sqrt([3] / NB)} over the nf frames: thread t of 256 adds frames t, t + 256, ...
 *             in ascending order, the 64 partials of a wave go through one shuffle tree (offsets 32 .. 1), the four waves' sums are added
 *             as (w0 + w1) + (w2 + w3) (the tree of ev_loudness and ev_stoi)
 *   d_counts  (B) int32: nf
 *   The caller takes sc = sqrt(s0 / s1), log_mag = 0.5 s2 / (nf NB) (the L1 of log magnitudes: half the log power) and
 *   lsd_db = (10 / ln 10) s3 / nf.
 * A row with len < 1, len > L or len <= nfft / 2 is no error and no out-of-bounds access: all its outputs are zeros (the ev_mas_align
 * convention).  Nothing at or behind len is read, and nothing depends on the batch or on L: a row alone, inside a batch, or as the d_len
 * prefix of a longer padded row with anything behind it, and a second call, give the same bits in every output.
 * Limits of ev_stft_dist, each violation failing with a message that names it and writing nothing: 1 <= B <= 65535; L >= 1 (and L / H below
 * 2^31 - 16); power_floor > 0 and finite; d_x, d_y, d_sums and d_counts non-NULL.
 * Kernels (two launches on `stream`, one where NF = 0; no host wait, no copy): (1) one workgroup of four waves per (row, 16 frames): the
 *   tile's span of 15 H + W samples of both signals staged once in LDS as fp32, reflection applied, then per wave and 16-bin tile W / 4 steps
 *   of four matrix instructions (x c, x s, y c, y s: 16 frames x 4 samples times 4 samples x 16 bins); (2) one workgroup per row: d_sums.
 * Scratch: B x NF x 4 doubles when d_frame is NULL, in an arena of the handle that grows on demand like the loudness arena and counts in
 *   ev_alloc_count: a second call at the same shape allocates nothing; ev_reserve does not cover it.  The call is capturable once the arena
 *   has its size. */
int ev_load_stft_dist(ev_handle *h, const double *window /* HOST (W) */, const double *twiddle /* HOST (nfft, 2): cos, sin of 2 pi n / nfft */,
                      int W, int H, int nfft);
int ev_stft_dist(ev_handle *h, const float *d_x /* (B, L) reference */, const float *d_y /* (B, L) processed */, const int32_t *d_len /* (B) or NULL */,
                 int B, int L, double power_floor /* 1e-7 */,
                 double *d_frame /* (B, NF, 4) or NULL */, double *d_sums /* (B, 4) */, int32_t *d_counts /* (B) */, void *stream);

/* Voice quality per frame on the device: the spectral-balance descriptors of the eGeMAPS set (alpha ratio, Hammarberg index, the spectral slopes
 * of two bands; Eyben et al., IEEE Trans. Affective Computing 2016) and the cepstral peak prominence (CPP; Hillenbrand, Cleveland and Erickson,
 * JSHR 1994), all from one float64 log-power spectrum of the frame and its cepstrum.  ev_load_voice_quality stores one geometry;
 * ev_voice_quality measures.  Everything is float64 (the fp32 samples are widened), the kernels are compiled with floating-point contraction off;
 * no atomics; ev_set_arithmetic does not reach it.
 * COMPARABILITY: the cepstrum here is the linear real cepstrum of the dB spectrum.  Hillenbrand's and Praat's CPP put the cepstral magnitude
 *   itself in dB as well, and VoiceSauce analyses pitch-synchronous windows: these figures are comparable across runs of THIS library (recorded
 *   against synthesised, per voice), not to the digit with those tools.
 * ev_load_voice_quality: HOST tables.  window (W) doubles w; twiddle (nfft, 2) doubles {cos, sin}(2 pi n / nfft) (ev_load_stft_dist's); H the
 *   hop; bands (6, 2) int32 {first bin, end bin (exclusive)} of: alpha low, alpha high, Hammarberg low, Hammarberg high, slope 0, slope 1;
 *   slope_w (2, NB) and fit_w (NQ) doubles, q_mean (below); quefrencies q_fit, q_min, q_max in samples.  NB = nfft / 2 + 1, off = (nfft - W) / 2,
 *   NQ = q_max - q_fit + 1.  Limits, each violation failing with a message that names it: nfft even with 16 <= nfft <= 1024; W a multiple of 4
 *   with 4 <= W <= nfft; nfft - W even; 1 <= H <= 512; every band non-empty inside [0, NB], both slope bands of at least 2 bins;
 *   1 <= q_fit <= q_min <= q_max <= nfft / 2 with NQ >= 2; finite, non-NULL tables, q_mean finite; at most 160 KiB of LDS per workgroup (cannot
 *   be exceeded inside the other limits).  The handle builds on the device, each entry rounded once and every phase index in exact integers,
 *   ev_stft_dist's basis c[j][k], s[j][k] = w[j] {cos_tab, sin_tab}[((j + off) k) mod nfft] and the cepstral basis
 *     cep[k][q] = g[k] cos_tab[(k q) mod nfft] / nfft,  g = 1 for k = 0 and k = nfft / 2, else 2,  0 <= k < NB,  q_fit <= q <= q_max.
 *   All tables live in one device block that counts once in ev_alloc_count.  Loading again replaces the tables; it waits for the device
 *   first.  ev_voice_quality without loaded tables fails with a message.
 *   The host tables are least-squares lines in their centred form: fit_w[i] = (q_i - q_mean) / sum (q - q_mean)^2 over q_fit .. q_max with q_mean
 *   their mean; slope_w[b][k] = (x_k - xbar) / sum (x - xbar)^2 over band b with x_k = k sr / nfft / 1000 (dB per kHz), 0 outside the band.
 * Sizes: NF = ceil(L / H); a row of len samples has nf = ceil(len / H) frames, ev_pitch_yin's.  d_len == NULL: every row is L long.
 * Definition, per row:
 *   framing   frame f reads s_j = x[f H + H / 2 - W / 2 + j] for 0 <= j < W, ZERO where the index is outside [0, len): no reflection (the one
 *             staging difference from ev_stft_dist).  At an equal hop the frames line up with ev_pitch_yin's and the mel's
 *   spectrum  re_k = sum_j s_j c[j][k], sm_k = sum_j s_j s[j][k] for 0 <= k < NB; raw_k = fma(sm_k, sm_k, re_k * re_k);
 *             p_k = max(raw_k, power_floor); Ldb_k = (10 / ln 10) log(p_k), the device library's float64 natural logarithm
 *   cepstrum  C_q = sum_k Ldb_k cep[k][q] for q_fit <= q <= q_max
 *   peak      q* = argmax C_q over q_min <= q <= q_max, the lowest q of a tie
 *   baseline  base = (sum_q C_q) / NQ + (sum_q fit_w[q - q_fit] C_q) (q* - q_mean): the least-squares line through C over q_fit .. q_max, at q*
 *   d_frame   (B, NF, 8): {cpp = C[q*] - base,
 *                          alpha = (10 / ln 10) (log sum_{alpha high} p - log sum_{alpha low} p),
 *                          hammarberg = max_{Hammarberg low} Ldb - max_{Hammarberg high} Ldb,
 *                          slope0 = sum_k slope_w[0][k] Ldb_k, slope1 = sum_k slope_w[1][k] Ldb_k (over all NB bins),
 *                          power = sum_k p_k, C[q*], base}
 *   d_peak    (B, NF) int32: q*
 *   d_cepstrum (B, NF, NQ) or NULL: C_q
 *   A SILENT frame, one without a bin of raw_k > power_floor, keeps its power; its other seven entries, its d_peak and its cepstrum are
 *   zeros by definition (with every bin clamped C is summation noise and its argmax arbitrary).  Frames at or past nf are zeros.
 * Orders (fixed; the sums over j and over k of the two matrix products run on v_mfma_f64_16x16x4_f64 in steps of four from 0, the order
 *   inside the instruction is the hardware's): sums over the bins k = 16 (w + 4 i) + c, and over the quefrencies q = q_fit + 16 (w + 4 i) + c,
 *   are added per (w, c) in ascending i (weighted terms as fma(weight, value, sum)), then over c by an xor tree (offsets 8, 4, 2, 1), then
 *   over w as ((w0 + w1) + w2) + w3; maxima are exact in any order.
 * A row with len < 1 or len > L is no error and no out-of-bounds access: all its outputs are zeros.  Nothing at or behind len is read, and
 * nothing depends on the batch or on L: a row alone, inside a batch, or as the d_len prefix of a longer padded row with anything behind it,
 * a second call, and a call with d_cepstrum NULL give the same bits in every output.
 * Limits of ev_voice_quality, each violation failing with a message that names it and writing nothing: 1 <= B <= 65535; L >= 1 (and L / H below
 * 2^31 - 16); power_floor > 0 and finite; d_x, d_frame and d_peak non-NULL.
 * Kernel (one launch on `stream`; no host wait, no copy, no arena: a call never allocates): one workgroup of four waves per (row, 16 frames);
 *   the tile's span of 15 H + W samples staged once in LDS, the first matrix product, the log-spectrum of the 16 frames kept in LDS (16 rows of
 *   S doubles, S = 2 mod 32), the second matrix product against the cepstral basis, the reductions.  The call is capturable. */
int ev_load_voice_quality(ev_handle *h, const double *window /* HOST (W) */, const double *twiddle /* HOST (nfft, 2): cos, sin of 2 pi n / nfft */,
                          int W, int H, int nfft, const int32_t *bands /* HOST (6, 2) */, const double *slope_w /* HOST (2, NB) */,
                          int q_fit, int q_min, int q_max, const double *fit_w /* HOST (NQ) */, double q_mean);
int ev_voice_quality(ev_handle *h, const float *d_x /* (B, L) */, const int32_t *d_len /* (B) or NULL */, int B, int L, double power_floor /* 1e-7 */,
                     double *d_frame /* (B, NF, 8) */, int32_t *d_peak /* (B, NF) */, double *d_cepstrum /* (B, NF, NQ) or NULL */, void *stream);

/* Formants per frame on the device: the vocal-tract resonances F1 .. Fn with their bandwidths (the other half of the eGeMAPS minimal set; Eyben et
 * al. 2016), from the linear prediction of every frame by Burg's lattice and the roots of its prediction polynomial, found all at once by the
 * Aberth-Ehrlich iteration.  ev_load_formants stores one geometry; ev_formants measures.  Everything is float64 (the fp32 samples are widened), the
 * kernel is compiled with floating-point contraction off; no atomics, no scratch; ev_set_arithmetic does not reach it.  The signal is expected at
 * twice the highest formant looked for (audio.formants decimates to 11025 Hz for 5500 Hz, as Praat resamples); the window is the caller's (Praat's
 * Gaussian window in audio.formant_window).  No tracking across frames: every frame stands alone.
 * Sizes: NF = ceil(L / H); a row of len samples has nf = ceil(len / H) frames, ev_pitch_yin's and ev_voice_quality's.  d_len == NULL: every row is L long.
 * Definition, per row and frame f, p = order:
 *   frames(n)  = ceil(n / H)                                   (pitch_yin's and voice_quality's grid)
 *   s_f[j]     = x[f H + H/2 - W/2 + j],  j = -1 .. W-1,  ZERO outside [0, len)      (no reflection)
 *   y[j]       = w[j] (s_f[j] - pre * s_f[j-1]),  j = 0 .. W-1                        (float64 from the fp32 samples)
 *   E0         = sum y[j]^2 ;  a frame with E0 <= power_floor is SILENT: all its outputs are zeros, count 0
 *   Burg, order p:  f_0 = b_0 = y;  for m = 1 .. p over n = m .. W-1:
 *       num = -2 sum f_{m-1}[n] b_{m-1}[n-1],  den = sum (f_{m-1}[n]^2 + b_{m-1}[n-1]^2),  k_m = den > 0 ? num / den : 0
 *       a_m[i] = a_{m-1}[i] + k_m a_{m-1}[m-i] (i = 1 .. m, a[0] = 1, a_{m-1}[m] = 0)
 *       f_m[n] = f_{m-1}[n] + k_m b_{m-1}[n-1],  b_m[n] = b_{m-1}[n-1] + k_m f_{m-1}[n]
 *       gain   = (E0 / W) prod (1 - k_m^2)
 *   roots of P(z) = z^p + a_1 z^(p-1) + ... + a_p by Aberth-Ehrlich, all p at once:
 *       z_i = 0.9 exp(i (2 pi i / p + 0.4));  per iteration r_i = P(z_i) / P'(z_i) (Horner), s_i = sum_{j != i} 1 / (z_i - z_j),
 *       w_i = r_i / (1 - r_i s_i),  z_i -= w_i;  once max_i |w_i| <= 2^-30 exactly two more iterations run and the iteration stops;
 *       more than 64 iterations in all, or any non-finite value: the frame is UNCONVERGED: count -1, formant entries zeros (a_i and gain stay)
 *   candidates: roots with Im z > 0 and f_lo < f < sr/2 - f_lo,  f = atan2(Im z, Re z) sr / (2 pi),  bw = -ln|z| sr / pi
 *   formants   = the n_formants candidates of lowest f, ascending;  count = how many there are (0 .. n_formants);  the rest zeros
 *   Real roots, with or without rounding noise in Im, land at f = 0 or f = sr / 2 (to rounding); the band rule removes them, which is why f_lo > 0.
 *   d_lpc     (B, NF, p + 2) or NULL: a_1 .. a_p, gain, E0
 *   d_formant (B, NF, n_formants, 2): {f, bw} in Hz
 *   d_count   (B, NF) int32
 *   Frames at or past nf are zeros.
 * Orders (fixed; they depend on the frame's own samples and the loaded geometry only): with R the power of two >= ceil(W / 64), the sums over n are
 *   added per c = floor(n / R) in ascending n, then over c by an xor tree over 64 terms (offsets 32, 16, 8, 4, 2, 1; absent terms are +0.0); Horner's
 *   recurrences and the sum over j run in ascending index; complex products and quotients by the textbook formulas (the quotient a / b as
 *   a conj(b) / |b|^2), |w| and |z| as sqrt(re^2 + im^2); sr / (2 pi) and sr / pi are formed once on the host; atan2, log and sqrt are the device
 *   library's float64 ones; the starting points are formed on the host (std::cos, std::sin).
 * A row with len < 1 or len > L is no error and no out-of-bounds access: all its outputs are zeros.  Nothing at or behind len is read, and nothing
 * depends on the batch or on L: a row alone, inside a batch, or as the d_len prefix of a longer padded row with anything behind it, a second call,
 * and a call with d_lpc NULL give the same bits in every output.
 * Limits of ev_load_formants (HOST window of W doubles), each violation failing with a message that names it: 2 <= order <= 32; 8 <= W <= 1024 and
 *   W > 2 order; 1 <= H <= 512; 1 <= n_formants <= 16; 0 <= pre_emphasis < 1; sr > 0 and finite; 0 < f_lo < sr / 4; the window finite and non-NULL.
 *   The load owns one device block, the window, which counts once in ev_alloc_count.  Loading again drops the old block (it waits for the device
 *   first); a failed load leaves the previous tables in use and the count unchanged.  ev_formants without loaded tables fails with a message.
 * Limits of ev_formants, each violation failing with a message that names it and writing nothing: 1 <= B <= 65535; L >= 1; power_floor > 0 and
 *   finite; d_x, d_formant and d_count non-NULL.
 * Kernel (one launch on `stream`; no host wait, no copy, no arena: a call never allocates): one wavefront per frame, four frames to a workgroup;
 *   lane l holds the samples l R .. l R + R - 1 of both lattice signals in registers, lane i the coefficient a_i and then the root z_i; no LDS and
 *   no barrier.  The call is capturable. */
int ev_load_formants(ev_handle *h, const double *window /* HOST (W) */, int W, int H, int order, double pre_emphasis,
                     double sr, double f_lo, int n_formants);
int ev_formants(ev_handle *h, const float *d_x /* (B, L) */, const int32_t *d_len /* (B) or NULL */, int B, int L, double power_floor,
                double *d_lpc /* (B, NF, order + 2): a_1 .. a_p, gain, E0; or NULL */,
                double *d_formant /* (B, NF, n_formants, 2): Hz, bandwidth Hz */, int32_t *d_count /* (B, NF) */, void *stream);

/* Formant tracks through the candidates ev_formants wrote: which candidate of a frame is F1, which F2, which F3.  ev_formants keeps the candidates
 * of lowest frequency, so one spurious low root (a nasal pole, a split F1, a root just inside f_lo) moves every formant up by one slot for that
 * frame.  This is Praat's tracker (Formant: Track; Formant_tracker: a Viterbi pass over the ways of mapping tracks onto a frame's candidates),
 * restated so that every order is fixed.  Everything is float64, the kernel is compiled with floating-point contraction off; no atomics, no
 * scratch; ev_set_arithmetic does not reach it.
 * Inputs are ev_formants' outputs, unchanged: d_formant (B, NF, n_cand, 2) {f, bw} in Hz and d_count (B, NF) int32.  There is no audio and no
 *   d_len: frames past a row's end already have count 0 and are therefore gaps.
 * Parameters: 1 <= n_cand <= 16;  1 <= n_tracks <= n_cand;  HOST ref[n_tracks] in Hz, finite and > 0;  cost_f, cost_b, cost_j finite and >= 0;
 *   S = C(n_cand, n_tracks) <= 1024.
 * States: the S strictly increasing index tuples c(0) < .. < c(n_tracks - 1) over 0 .. n_cand - 1, numbered in lexicographic order.  Formants do
 *   not cross, so track k takes the k-th chosen candidate.
 * Trackable frames: with m = min(count, n_cand), a frame is trackable iff m >= n_tracks and its first m candidates have finite f > 0 and finite bw.
 *   Every other frame is a GAP: silent frames, unconverged frames (count -1), frames with too few candidates, frames past the row.  A state is
 *   valid in a frame iff c(n_tracks - 1) < m; a state that is not valid costs +inf.
 * Segments: a maximal run of trackable frames.  Every segment is decoded on its own and nothing crosses a gap.  (Praat refuses frames with too
 *   few candidates; here such a frame ends a segment.)
 * Costs, float64, sums in ascending track k starting from the first term:
 *   local(t, s)      = sum_k ( (cost_f |f - ref[k]|) / 1000 + (cost_b bw) / f ),  f, bw of candidate c_s(k) in frame t
 *   trans(t, s -> s') = sum_k cost_j |lg_{t-1}[c_s(k)] - lg_t[c_s'(k)]|,  lg = log2(f) from the device library
 *   delta_t0(s)      = local(t0, s) at a segment's first frame t0
 *   delta_t(s')      = min_s (delta_{t-1}(s) + trans(t, s -> s')) + local(t, s');  of equal minima the lowest s wins
 *   At the segment's last frame the lowest s of least delta ends the path, and the back-pointers give the rest.
 *   Min-with-lowest-index is associative and commutative: how the predecessor scan is split over lanes cannot change a bit.
 * Outputs:
 *   d_track (B, NF, n_tracks, 2): {f, bw} of the chosen candidates, copies of the input entries; zeros on gaps
 *   d_sel   (B, NF) int32: the state number, -1 on gaps
 *   d_cost  (B, NF) float64 or NULL: the segment's optimum at the segment's LAST frame, 0 elsewhere
 *   d_back  (B, NF, S) uint16: the caller's work buffer, as ev_pyin_decode's d_back is; what it holds after the call is not defined
 * Nothing depends on the batch or on NF: a row alone, inside a batch, with extra gap frames behind it (a larger NF), a second call, a call with
 *   d_cost NULL and a replay from a captured graph give the same bits.
 * Limits, each violation failing with a message that names it and writing nothing: 1 <= B <= 65535; NF >= 1; the parameters above (the message for
 *   S names S); ref, d_formant, d_count, d_back, d_track and d_sel non-NULL.
 * Kernel (one launch on `stream`; no load step, no host wait, no copy, no arena: ev_alloc_count never moves): one workgroup per row, sequential
 *   over the frames with one barrier each; a thread per target state, its tuple unranked once by the combinatorial number system (for S <= 32 the
 *   predecessor scan of a target is spread over 64 / S lanes, a power of two, and reduced on (value, lowest index)); delta double-buffered in
 *   LDS; ref and the costs travel in the kernel's arguments; lane 0 walks d_back per segment.  The call is capturable. */
int ev_formant_track(ev_handle *h, const double *d_formant /* (B, NF, n_cand, 2) */, const int32_t *d_count /* (B, NF) */, int B, int NF,
                     int n_cand, int n_tracks, const double *ref /* HOST (n_tracks) Hz */, double cost_f, double cost_b, double cost_j,
                     uint16_t *d_back /* (B, NF, S) work */, double *d_track /* (B, NF, n_tracks, 2) */, int32_t *d_sel /* (B, NF) */,
                     double *d_cost /* (B, NF) or NULL */, void *stream);

/* Jitter, shimmer and the harmonics-to-noise ratio per frame on the device: how regular the voice is from one glottal cycle to the next (the
 * remaining time-domain members of eGeMAPS; Eyben et al. 2016), on ev_pitch_yin's frame grid and at the lag it wrote.  Everything is float64 on the
 * widened fp32 samples, the kernel is compiled with floating-point contraction off; no atomics, no scratch; ev_set_arithmetic does not reach it.
 * H is the hop.  There are F = ceil(L / H) frames per row; a row of len samples has ceil(len / H) of its own.  The centre of frame f is
 * c = f H + H / 2, ev_pitch_yin's.  Samples outside [0, len) enter as +0.  d_len == NULL: every row is L long.
 * tau0 = d_lag[b, f] (B, F), the integer lag ev_pitch_yin wrote, read on the device.  A frame with tau0 < 16 or tau0 > 2048 is UNVOICED (0 is the
 * usual case): zeros in d_frame and d_count, -1 in every mark.
 * Marks, by peak picking on the raw fp32 samples; every decision is exact, ties go to the lowest index:
 *   q = tau0 / 8, lo = tau0 - q, hi = tau0 + q                       (integer divisions)
 *   the anchor m_0 = argmax x[n] over s <= n < s + tau0, s = c - tau0 / 2
 *   forward m_{k+1} = argmax over [m_k + lo, m_k + hi];  backward m_{k-1} = argmax over [m_k - hi, m_k - lo];  k runs to n_cycles on each side
 *   a mark is accepted when x[m] > 0, x[m] > x[m - 1] and x[m] >= x[m + 1]; the first mark that is not accepted ends its direction; an anchor that
 *   is not accepted leaves the frame with no marks.
 *   (The window is +-1/8 of the period and not wider: with +-1/4 a secondary resonance peak 17 % away was picked on synthetic pulses at 120 Hz.)
 * Refinement, float64 in this order:  a, b, c = x[m - 1], x[m], x[m + 1];  den = (a - 2 b) + c;  shift = 0.5 (a - c) / den when den < 0 and
 *   |shift| <= 1, else 0;  t = m + shift;  A = b - 0.25 (a - c) shift.
 * Periods T_i = t_{i+1} - t_i over consecutive marks, amplitudes A_i over the marks.  A period pair (T_i, T_{i+1}) counts when
 *   max <= period_factor min, an amplitude pair (A_i, A_{i+1}) when max <= amplitude_factor min, a triple when both of its period pairs count.
 *   Every sum is a single chain in ascending i.
 * d_frame[b, f, 0..7] float64:  0 local jitter mean|T_i - T_{i+1}| / Tmean;  1 absolute jitter mean|T_i - T_{i+1}| in samples;  2 local shimmer
 *   mean|A_i - A_{i+1}| / Amean;  3 shimmer in dB mean|20 log10(A_{i+1} / A_i)|;  4 the harmonic strength r;  5 Tmean over all periods;  6 Amean
 *   over all marks;  7 RAP mean|T_i - (T_{i-1} + T_i + T_{i+1}) / 3| / Tmean over the counted triples.  The means of 0 .. 3 run over the counted
 *   pairs; a mean over no terms is 0.
 * d_count[b, f, 0..3] int32: the periods, the counted period pairs, the counted amplitude pairs, the counted triples.
 * d_marks[b, f, n_cycles + k] int32 (B, F, 2 n_cycles + 1), may be NULL: m_k, or -1 where there is no mark.
 * Harmonic strength: the normalised cross-correlation (Praat's "cc" harmonicity; it needs no window correction).  W = corr_length,
 *   s = c - (W + tau0) / 2, the base is x[s + j], j < W.  For tau in {tau0 - 1, tau0, tau0 + 1}:  C = sum x[s + j] x[s + j + tau],
 *   E1 = sum x[s + j + tau]^2,  E0 = sum x[s + j]^2,  r(tau) = C / sqrt(E0 E1) when E0 E1 > power_floor^2, else 0.  With a, b, c = r(tau0 - 1),
 *   r(tau0), r(tau0 + 1) the output is b - 0.25 (a - c) shift under the shift rule above.  HNR in dB is 10 log10(r / (1 - r)).
 *   Order of the sums: float64, every product of widened fp32 samples (exact), one fma per term; term j belongs to lane j mod 64, a lane adds its
 *   terms in ascending j, then an xor tree over the 64 lanes (offsets 32, 16, 8, 4, 2, 1; absent terms are +0.0).  power_floor^2 is formed once on
 *   the host; sqrt and log10 are the device library's float64 ones.
 * Frames at or past a row's ceil(len / H) are zeros with -1 in the marks; so is every frame of a row with len < 1 or len > L, which is no error and
 * no out-of-bounds access.  Nothing at or behind len is read, and every order depends on the frame's samples and the arguments only: a row alone,
 * inside a batch, as the d_len prefix of a longer padded row, a call with d_marks NULL, a second call and a call under every ev_set_arithmetic
 * setting give the same bits.
 * Limits, each violation failing with a message that names it and writing nothing: 1 <= B <= 65535; L >= 1; 1 <= hop_length <= 4096;
 *   1 <= n_cycles <= 16; 8 <= corr_length <= 4096; period_factor and amplitude_factor finite and greater than 1; power_floor finite and greater
 *   than 0; d_x, d_lag, d_frame and d_count non-NULL.
 * Kernel (one launch on `stream`; no load step, no host wait, no copy, no arena: ev_alloc_count never moves): one wavefront per frame, four frames to
 *   a workgroup; a search is a lane-strided read of its range and a 6-step reduction on (value, index); the forward and the backward chain advance
 *   in one loop; no LDS and no barrier.  The call is capturable. */
int ev_perturbation(ev_handle *h, const float *d_x /* (B, L) */, const int32_t *d_len /* (B) or NULL */, int B, int L, int hop_length,
                    const int32_t *d_lag /* (B, F) */, int n_cycles, int corr_length, double period_factor /* 1.3 */,
                    double amplitude_factor /* 1.6 */, double power_floor, double *d_frame /* (B, F, 8) */, int32_t *d_count /* (B, F, 4) */,
                    int32_t *d_marks /* (B, F, 2 n_cycles + 1) or NULL */, void *stream);

/* Harmonic differences per frame on the device: H1-H2 (the first harmonic over the second: the correlate of open quotient, a breathy against a
 * pressed voice; Hanson 1997), H1-A3 (the first harmonic over the strongest harmonic in the third formant's range: the source's spectral tilt) and
 * the level of the harmonic at F1, F2 and F3 over H1 (eGeMAPS's formant relative energy; Eyben et al. 2016), on ev_pitch_yin's frame grid, at the
 * period it wrote and the formants ev_formants wrote.  ev_load_harmonics stores one geometry; ev_harmonics measures.  Everything is float64 (the
 * fp32 samples are widened), the kernel is compiled with floating-point contraction off; no atomics, no scratch; ev_set_arithmetic does not reach it.
 * Sizes: NB = nfft / 2 + 1; NF = ceil(L / H); a row of len samples has nf = ceil(len / H) frames.  d_len == NULL: every row is L long.
 * Framing and spectrum are ev_voice_quality's: s_j = x[f H + H / 2 - W / 2 + j], zero outside [0, len), no reflection; ev_stft_dist's windowed
 *   basis on v_mfma_f64_16x16x4_f64;  raw_k = fma(sm, sm, re re),  p_k = max(raw_k, power_floor),  Ldb_k = (10 / ln 10) log(p_k).
 * Frame classes, in this order.  T = (double)d_period[b, f].  UNVOICED: T is not > 0.  SILENT: no bin has raw_k > power_floor.  UNRESOLVED:
 *   v = (double)nfft / T < min_spacing (under a Hann window harmonics closer than 4 bins merge).  All three give zeros in d_frame and d_harm and a
 *   count of 0, except that entry 7 (v) is kept for UNRESOLVED.
 * Comb.  For h = 1, 2, ...:  c = (double)h v;  r = fmax(1.0, search v);  lo = (int)ceil(c - r), hi = (int)floor(c + r).  Harmonic h is measured
 *   while hi <= NB - 2 and h <= n_harm; n_h is the number measured.  lo >= 1 follows from min_spacing >= 2 and search <= 0.5.
 * Peak of one harmonic.  k* = argmax Ldb_k over lo .. hi, the lowest k of a tie;  a, b, c' = Ldb[k* - 1], Ldb[k*], Ldb[k* + 1];
 *   den = (a - 2 b) + c';  shift = 0.5 (a - c') / den when den < 0 and |shift| <= 1, else 0 (ev_perturbation's vertex rule);
 *   A_h = b - 0.25 (a - c') shift in dB;  f_h = (k* + shift) (sr / nfft), the quotient sr / nfft formed once on the host.
 * Formant terms, only with d_formant and d_fcount.  u = sr / T.  For i = 1 .. min(3, n_formants): F_i = d_formant[b, f, i - 1, 0] is valid when
 *   i <= d_fcount[b, f] and F_i > 0;  g = F_i / u,  h_i = (int)floor(g + 0.5), valid when 1 <= h_i <= n_h;  rel_i = A_{h_i} - A_1.
 * A3.  g = F_3 / u;  w = fmax(0.5, a3_range g);  the range is max(1, ceil(g - w)) .. min(n_h, floor(g + w));  A3 is the maximum of A_h over it
 *   (one ascending loop, the lowest h of a tie), valid when F_3 is valid and the range is not empty.
 * d_frame[b, f, 0..7] float64:  0 H1-H2 = A_1 - A_2;  1 H1-A3 = A_1 - A3;  2, 3, 4 rel_1, rel_2, rel_3;  5 A_1;  6 f_1;  7 v.  An entry whose
 *   ingredients are not valid is 0.
 * d_count[b, f, 0..1] int32: n_h and the flags: bit 0 n_h >= 2; bits 1-3 rel_i valid; bit 4 A3 valid.
 * d_harm[b, f, h - 1, 0..1] float64 (B, NF, n_harm, 2), may be NULL: {f_h, A_h} for h <= n_h, zeros behind.
 * Frames at or past a row's ceil(len / H) are zeros; so is every frame of a row with len < 1 or len > L, which is no error and no out-of-bounds
 * access.  Nothing at or behind len is read (of d_x, d_period, d_formant and d_fcount alike), and nothing depends on the batch or on L: a row alone,
 * inside a batch, as the d_len prefix of a longer padded row, a call with d_harm NULL, a second call, a call under every ev_set_arithmetic setting
 * and a replay from a captured graph give the same bits; a call with d_formant NULL gives the same entries 0, 5, 6, 7 and bit 0, and zeros in the
 * formant entries and flags.
 * Orders: the DFT sums are ev_stft_dist's (one chain of W / 4 matrix steps per bin); a search is one ascending scan by one lane; log is the device
 *   library's float64 one.
 * Loading (ev_load_harmonics: host tables, one device block with the basis, counted once in ev_alloc_count; loading again replaces the block after
 *   waiting for the device; a failed load leaves the previous tables in use and the count unchanged).  ev_harmonics without loaded tables fails with
 *   a message.  Limits of a load, each violation failing with a message that names it: nfft even, 16 <= nfft <= 2048; W a multiple of 4,
 *   4 <= W <= nfft, nfft - W even; 1 <= H <= 512; sr positive and finite; 1 <= n_harm <= 64; 0 < search <= 0.5; min_spacing finite and at least 2;
 *   0 <= a3_range <= 0.5; finite, non-NULL tables; at most 160 KiB of LDS per workgroup: 16 S doubles of log-spectrum (S the smallest number >= NB
 *   with S = 2 mod 32), the skewed span of 15 H + W floats (at most 3 (16 + W / H) pad words), 16 n_harm 2 doubles of harmonics and 64 words of
 *   counts.  nfft = 2048 with H = 256 fits up to n_harm = 34; nfft = 2048 with H = 512 does not.
 * Limits of ev_harmonics, each violation failing with a message that names it and writing nothing: 1 <= B <= 65535; L >= 1 (and L / H below
 *   2^31 - 16); power_floor finite and greater than 0; d_x, d_period, d_frame and d_count non-NULL; d_formant and d_fcount both NULL or both
 *   non-NULL, with 1 <= n_formants <= 16 when given.
 * Kernel (harmonics_kernel: one launch on `stream`, no host wait, no copy, no arena: ev_alloc_count never moves): one workgroup of four waves per
 *   (row, 16 frames); phase 1 is ev_voice_quality's first matrix product into a log-spectrum in LDS; phase 2, after one barrier, gives each frame 16
 *   lanes, lane j searching harmonics j + 1, j + 17, ...; phase 3, after a second barrier, forms the figures with one thread per frame.  The call is
 *   capturable. */
int ev_load_harmonics(ev_handle *h, const double *window /* HOST (W) */, const double *twiddle /* HOST (nfft, 2) */, int W, int H, int nfft,
                      double sr, int n_harm, double search /* 0.25 */, double min_spacing /* 4.0 */, double a3_range /* 0.1 */);
int ev_harmonics(ev_handle *h, const float *d_x /* (B, L) */, const int32_t *d_len /* (B) or NULL */, int B, int L,
                 const float *d_period /* (B, NF): ev_pitch_yin's d_period, 0 = unvoiced */,
                 const double *d_formant /* (B, NF, n_formants, 2) or NULL */, const int32_t *d_fcount /* (B, NF) or NULL */, int n_formants,
                 double power_floor, double *d_frame /* (B, NF, 8) */, int32_t *d_count /* (B, NF, 2) */,
                 double *d_harm /* (B, NF, n_harm, 2) or NULL */, void *stream);

/* Contour functionals on the device: what turns the per-frame contours above (pitch, voice quality, formants, perturbation, harmonic differences)
 * into a description of an utterance (the eGeMAPS functionals; Eyben et al. 2016): moments, percentiles, the slopes of the rising and of the
 * falling parts, the peaks, and the lengths of the stretches of valid frames and of the gaps between them.  K contours of F frames per row, every
 * contour on its own.  Everything is float64, the kernel is compiled with floating-point contraction off; no atomics, no scratch;
 * ev_set_arithmetic does not reach it.
 * Valid frames: n = d_len[b], or F when d_len is NULL.  A row with n < 0 or n > F is zeros in both outputs, which is no error and no out-of-bounds
 *   access; nothing at or behind n is read.  Frame f of contour (b, k) is VALID when f < n, d_mask[b, k, f] != 0 (d_mask NULL: every byte is 1) and
 *   d_v[b, k, f] is finite; a frame inside n with a non-zero mask byte and a non-finite value is DROPPED: counted, and invalid for everything else.
 *   The valid values in ascending frame order are u_0 .. u_{k-1}, at the frames g_0 < .. < g_{k-1}.  Pair i (u_i, u_{i+1}) is ADJACENT when
 *   g_{i+1} = g_i + 1.
 * Moments: mean = sum u / k;  sd = sqrt(sum (u - mean)^2 / k) (population, two passes).
 * Order statistics: s is u sorted ascending by < on the values (equal values are interchangeable; -0 equals +0).  min = s_0, max = s_{k-1}; for
 *   each q_r:  p = q_r (double)(k - 1) (one rounded product),  j = floor(p),  t = p - j,  the result is s_j + t (s_{min(j+1, k-1)} - s_j): numpy's
 *   linear interpolation up to rounding.
 * Parts: the class of pair i is +1 when it is adjacent and u_{i+1} > u_i, -1 when adjacent and u_{i+1} < u_i, else 0 (a gap or an equal pair ends
 *   a part).  A rising part is a maximal run of consecutive pairs of class +1, from index a to index e of u; its slope is
 *   (u_e - u_a) / (double)(e - a) per frame; falling parts likewise, with negative slopes.  rise_mean, rise_sd, fall_mean, fall_sd: the mean and the
 *   population sd of the slopes over the parts, two passes.
 * Peaks: index i is a peak when both of its pairs are adjacent, u_i > u_{i-1} and u_i >= u_{i+1} (ev_perturbation's local-peak rule).
 * Runs and gaps: inside [0, n) a RUN is a maximal stretch of valid frames, a GAP a maximal stretch of frames that are not valid, the leading and
 *   the trailing one included.  With N stretches of lengths l:  S1 = sum l, S2 = sum l^2 (integers);  mean = (double)S1 / (double)N;
 *   sd = sqrt((double)(N S2 - S1 S1)) / (double)N, in 64-bit integer arithmetic before the one conversion.
 * d_stat[b, k, .] float64: 0 mean, 1 sd, 2 min, 3 max, 4 rise_mean, 5 rise_sd, 6 fall_mean, 7 fall_sd, 8 run_mean, 9 run_sd, 10 gap_mean,
 *   11 gap_sd, 12 + r the percentile at q_r.  d_count[b, k, .] int32: 0 k, 1 dropped frames, 2 rising parts, 3 falling parts, 4 peaks, 5 runs,
 *   6 gaps, 7 adjacent pairs.  A statistic over no terms is 0.
 * Order of the float64 sums, one rule for every sum over an index i (sum u and sum (u - mean)^2 over the values; the slope sums over the PAIRS,
 *   where a part's slope, or its squared deviation, sits at the index of the part's last pair and +0.0 elsewhere): term i belongs to slot i mod 256;
 *   a slot starts at +0.0 and adds its terms in ascending i; the 256 slots are reduced by an xor tree (offsets 32, 16, 8, 4, 2, 1) inside each group
 *   of 64; the four group sums are added in ascending order, ((g0 + g1) + g2) + g3.  Products are rounded before they are added.  The order depends
 *   on k and the values only, never on B, K, F or the place in the grid: a contour alone, inside a batch, at another k, as the d_len prefix of a
 *   longer F, in a second call, under every ev_set_arithmetic setting and from a captured graph gives the same bits.
 * Limits, each violation failing with a message that names it and writing nothing: 1 <= B <= 65535; 1 <= K <= 65535; 1 <= F <= 4096 (ev_dtw's
 *   frame limit); 0 <= NQ <= 16; every q_r finite with 0 <= q_r <= 1 (checked on the host); q non-NULL when NQ > 0; d_v, d_stat and d_count
 *   non-NULL.
 * Kernel (functionals_kernel: one launch on `stream`; no load step, no host wait, no copy, no arena: ev_alloc_count never moves): one workgroup of
 *   four waves per contour, everything in LDS: u (8 bytes per frame), g and the parts' start indices (2 bytes each) at F rounded up to a power of
 *   two and at least 256, and 512 bytes of hand-over: 48.5 KiB at F = 4096.  One coalesced pass compacts the valid frames by ballots and a running
 *   prefix; two max-scans carry the start of every run and of every part to its end; the sums; a bitonic network sorts u in place behind +inf
 *   padding; thread r forms percentile r.  The call is capturable. */
int ev_functionals(ev_handle *h, const double *d_v /* (B, K, F) */, const uint8_t *d_mask /* (B, K, F) or NULL */,
                   const int32_t *d_len /* (B) frames, or NULL */, int B, int K, int F,
                   const double *q /* HOST (NQ), may be NULL when NQ == 0 */, int NQ,
                   double *d_stat /* (B, K, 12 + NQ) */, int32_t *d_count /* (B, K, 8) */, void *stream);

/* Modulation spectra of contours on the device: how a contour OSCILLATES in time, which the functionals above do not say.  Tremor and vibrato are a
 * 4-12 Hz oscillation of f0 and of loudness; the loudness contour's modulation spectrum peaks at the syllable rate; the modulation spectrum of the
 * mel-cepstral trajectories is the measure of a synthesiser that flattens fast spectral movement (Takamichi et al. 2016).  All three are one
 * computation on ev_functionals' interface: K contours of F frames per row under masks, every contour on its own.  On a fixed frequency grid the
 * spectrum does not move with a shift in time and is comparable between rows of different length, so it needs no sample alignment.  Everything is
 * float64, the kernel is compiled with floating-point contraction off; no atomics, no scratch; ev_set_arithmetic does not reach it.
 * Valid frames, dropped frames, runs: ev_functionals' rules.  n = d_len[b], or F when d_len is NULL.  A row with n < 0 or n > F is zeros in EVERY
 *   output (the peak indices of d_count included), which is no error and no out-of-bounds access; nothing at or behind n is read.  Frame f of
 *   contour (b, k) is VALID when f < n, d_mask[b, k, f] != 0 (d_mask NULL: every byte is 1) and d_v[b, k, f] is finite; a frame inside n with a
 *   non-zero mask byte and a non-finite value is DROPPED: counted, and invalid for everything else.  A RUN is a maximal stretch of valid frames
 *   inside [0, n); a run of length l >= min_run is ANALYSED.  Nothing crosses a gap and nothing is interpolated: a figure over a gap would be invented.
 * Grid: nu_j = nu0 + (double)j * dnu cycles per frame, 0 <= j < NM (one rounded product, one rounded sum).
 * One analysed run u_0 .. u_{l-1}, t run-local:  tc = (double)t - (double)(l - 1) / 2 (exact);  m = sum u / l;
 *   b = sum(tc u) / ((double)(l (l l - 1)) / 12.0), the least-squares line (the product of integers is exact in 64 bits before the one conversion);
 *   r_t = (u_t - m) - b tc;  w_t = 0.5 - 0.5 cospi((double)(2 t + 1) / (double)l), a symmetric Hann window that is never zero inside the run;
 *   sw = sum w_t;  ph = nu_j * (double)t (one rounded product);  xr_j = sum w_t r_t cospi(2 ph),  xi_j = sum w_t r_t sinpi(2 ph);
 *   P_j = 2 (xr^2 + xi^2) / (sw sw): half the squared amplitude of a sinusoid at nu_j, in the contour's units squared.
 *   (run, j) is RESOLVED when nu_j * (double)l >= min_cycles (one IEEE product).
 * Pooling over the analysed runs in ascending order:  W_j = sum l over the runs that resolve j (an integer);  Pm_j = (sum (double)l * P_j) /
 *   (double)W_j, 0 when W_j = 0.  d_spec = Pm, d_weight = W.  d_stat[0] = (sum over the runs of sum_t r_t^2) / (frames analysed): the variance of
 *   what the lines leave;  d_stat[1] = (sum (double)l * b) / (frames analysed): the length-weighted mean slope per frame.  Both are 0 without an
 *   analysed run.
 * Peak per band [j_lo, j_hi): the candidates are the j of the band with 1 <= j <= NM - 2, W_{j-1}, W_j, W_{j+1} > 0, Pm_{j-1}, Pm_{j+1} > 0,
 *   Pm_j > Pm_{j-1} and Pm_j >= Pm_{j+1} (ev_perturbation's local-peak rule; the neighbours may lie outside the band).  The peak is the candidate
 *   with the largest Pm_j, the lowest j among equals.  With a, c, e = log Pm_{j-1}, log Pm_j, log Pm_{j+1}:  den = (a - 2 c) + e;
 *   off = den < 0 ? (0.5 (a - e)) / den : 0;  pw = exp(c - (0.25 (a - e)) off), the peak power.
 *   d_peak[b, k, band, .] = { nu0 + ((double)j + off) dnu,  sqrt(2 pw): the amplitude,  the mean of Pm over the band's j with W_j > 0 (added in
 *   ascending j),  pw / that mean }.  Without a candidate the four are zeros and the band's entry of d_count is -1; otherwise that entry is j.
 * d_count[b, k, .] int32: 0 valid frames, 1 dropped frames, 2 analysed runs, 3 analysed frames, 4 + band the peak index.
 * Order of the float64 sums.  Per run (sum u, sum tc u, sum w, sum r^2): term t belongs to slot t mod 64; a slot starts at +0.0 and adds its terms
 *   in ascending t; the 64 slots are reduced by an xor tree (offsets 32, 16, 8, 4, 2, 1).  xr and xi: four chains c = t mod 4, each from +0.0 in
 *   ascending t, a term being the rounded product (w_t r_t) cospi(2 ph) added by a rounded sum (no fused multiply-add anywhere, so that a
 *   restatement without one adds the same numbers); joined as ((s0 + s1) + s2) + s3.  The sums over the runs (Pm's numerator, both statistics)
 *   start at +0.0 and add the runs in ascending order.  Products are rounded before they are added.  Every order is a function of the contour, the
 *   grid and min_run alone, never of B, K, F or the place in the grid: a contour alone, inside a batch, at another k, as the d_len prefix of a
 *   longer F, in a second call, under every ev_set_arithmetic setting and from a captured graph gives the same bits.
 * Limits, each violation failing with a message that names it and writing nothing: 1 <= B <= 65535; 1 <= K <= 65535; 1 <= F <= 4096; 1 <= NM <=
 *   128; nu0 and dnu finite and greater than 0; nu0 + (NM - 1) dnu <= 0.5; 3 <= min_run <= F; min_cycles finite and at least 0; 0 <= NBAND <= 4
 *   with 0 <= j_lo < j_hi <= NM for every band; band non-NULL and d_peak non-NULL when NBAND > 0; d_v, d_spec, d_weight, d_stat and d_count
 *   non-NULL.
 * Kernel (modulation_kernel: one launch on `stream`; no load step, no host wait, no copy, no arena: ev_alloc_count never moves): one workgroup of
 *   four waves per contour, everything in LDS: w_t r_t (8 bytes per frame), the table of the analysed runs (12 bytes each, at most (F + 1) / 4 of
 *   them) and the pooled spectrum: 45.6 KiB at F = 4096.  Phase A finds the runs with ev_functionals' max-scan, detrends and windows them in
 *   place; phase B gives every (j, chain) a thread, which reads w_t r_t as an LDS broadcast and calls the device library's float64 cospi and sinpi
 *   (they bound the kernel); phase C pools, picks the peaks (log, exp, sqrt: the device library's) and writes.  The call is capturable. */
int ev_modulation(ev_handle *h, const double *d_v /* (B, K, F) */, const uint8_t *d_mask /* (B, K, F) or NULL */,
                  const int32_t *d_len /* (B) frames, or NULL */, int B, int K, int F,
                  double nu0, double dnu, int NM, int min_run, double min_cycles,
                  const int32_t *band /* HOST (NBAND, 2): j_lo, j_hi; may be NULL when NBAND == 0 */, int NBAND,
                  double *d_spec /* (B, K, NM) */, int32_t *d_weight /* (B, K, NM) */, double *d_peak /* (B, K, NBAND, 4) or NULL when NBAND == 0 */,
                  double *d_stat /* (B, K, 2) */, int32_t *d_count /* (B, K, 4 + NBAND) */, void *stream);

/* Auditory descriptors per frame on the device: the descriptors of timbre and dynamics that eGeMAPS (Eyben et al. 2016) adds to pitch, balance,
 * formants and perturbation: the LOUDNESS of an auditory spectrum (mel bands under an equal-loudness weighting, compressed by a power law), the
 * SPECTRAL FLUX (how fast the magnitude spectrum moves from one frame to the next) and the first MEL-FREQUENCY CEPSTRAL COEFFICIENTS, with the frame's
 * power and log-energy, on ev_pitch_yin's frame grid.  ev_load_auditory stores one geometry and its tables; ev_auditory measures.  Everything is
 * float64 (the fp32 samples are widened), the kernel is compiled with floating-point contraction off; no atomics, no scratch; ev_set_arithmetic does
 * not reach it.  The device sees only tables: which mel scale, which equal-loudness curve, which cepstral coefficients and which lifter is the host
 * layer's choice (audio.auditory_tables: HTK mel triangles, Hermansky 1990, DCT-II columns 1 .. n_ceps with the HTK lifter, compress 0.33).
 * Units: the figures are comparable across this project's runs and NOT to the digit with openSMILE's, which frames differently (25 ms Hamming
 * windows for its MFCC), and scales the spectrum and the loudness its own way.
 * Sizes: NB = nfft / 2 + 1; NF = ceil(L / H); a row of len samples has nf = ceil(len / H) frames (ev_pitch_yin's and ev_voice_quality's frames).
 * d_len == NULL: every row is L long.
 *   s_f[j]    = x[f H + H / 2 - W / 2 + j], ZERO outside [0, len)          (no reflection)
 *   re, sm    = s_f @ {c, s}                                               (ev_stft_dist's windowed basis, on v_mfma_f64_16x16x4_f64)
 *   raw[k]    = fma(sm, sm, re re),  0 <= k < NB
 *   power     = sum_k raw[k]
 *   E[m]      = sum_k raw[k] mel_w[k][m],  0 <= m < n_mel                  (mel_w: dense (NB, n_mel) host doubles, finite and >= 0)
 *   Ef[m]     = max(E[m], power_floor)
 *   loudness  = sum_m pow(eq[m] Ef[m], compress)                           (eq: n_mel host doubles, finite and > 0;  0 < compress <= 1)
 *   mfcc[i]   = sum_m log(Ef[m]) dct[m][i],  0 <= i < n_ceps               (dct: (n_mel, n_ceps) host doubles, finite; it carries the lifter)
 *   flux_f    = sqrt( sum_{k_lo <= k < k_hi} (sqrt(raw_f[k]) - sqrt(raw_{f-1}[k]))^2 / (k_hi - k_lo) )   for 1 <= f < nf
 *   flux_0    = 0 by definition: frame -1 is not a frame of the row, although its window reaches into the row when W > H
 *   live_f    = some raw_f[k] > power_floor
 * d_frame[b, f, 0..3] float64: {loudness, flux, power, log(max(power, power_floor))};  d_mfcc[b, f, i] float64 (B, NF, n_ceps);
 * d_flags[b, f] int32: bit 0 live, bit 1 f >= 1 (the frame has a predecessor);  d_bands[b, f, m] float64 (B, NF, n_mel), may be NULL: E[m], unfloored.
 * A SILENT frame (not live) keeps its power and its flux (an offset into silence is a flux event); its loudness, log-energy, d_mfcc and d_bands are
 * zeros and its live bit is 0.  Frames at or past a row's ceil(len / H) are zeros in every output, flags included; so is every frame of a row with
 * len < 1 or len > L, which is no error and no out-of-bounds access.  Nothing at or behind len is read, and nothing depends on the batch or on L: a
 * row alone, inside a batch, as the d_len prefix of a longer padded row, a call with d_bands NULL, a second call, a call under every
 * ev_set_arithmetic setting and a replay from a captured graph give the same bits.
 * Orders: the DFT sums are ev_stft_dist's (one chain of W / 4 matrix steps per bin); power: per lane over its bin tiles ascending, an xor tree (8, 4,
 *   2, 1) over the 16 column lanes, the four waves as ((w0 + w1) + w2) + w3; E[m]: one chain of ceil(NB / 4) matrix steps over ascending k; the flux:
 *   lane j of 16 adds the bins k = j mod 16 of [k_lo, k_hi) ascending as fma(d, d, s), then the xor tree; mfcc[i] one chain of fma over ascending m; the
 *   loudness one chain of additions over ascending m.  log, pow and sqrt are the device library's float64 ones.
 * Loading (ev_load_auditory: host tables, one device block with the basis, mel_w padded with zeros to (4 ceil(NB / 4), 16 ceil(n_mel / 16)), eq and
 *   dct, counted once in ev_alloc_count; loading again replaces the block after waiting for the device; a failed load leaves the previous tables in
 *   use and the count unchanged).  ev_auditory without loaded tables fails with a message.  Limits of a load, each violation failing with a message
 *   that names it: nfft even, 16 <= nfft <= 1024; W a multiple of 4, 4 <= W <= nfft, nfft - W even; 1 <= H <= 512; 1 <= n_mel <= 64; 1 <= n_ceps <=
 *   16; 0 <= k_lo < k_hi <= NB; 0 < compress <= 1; finite, non-NULL tables, no negative entry in mel_w, every entry of eq greater than 0; at most 160
 *   KiB of LDS per workgroup: 16 S doubles of power spectrum (S the smallest number >= NB with S = 2 mod 32), 32 (16 ceil(n_mel / 16) + 1) doubles of
 *   band terms and the skewed span of 15 H + W floats (at most 3 (16 + W / H) pad words): 93 840 bytes at 1024 / 256 / 1024 with 26 bands.
 * Limits of ev_auditory, each violation failing with a message that names it and writing nothing: 1 <= B <= 65535; L >= 1 (and L / H below
 *   2^31 - 16); power_floor finite and greater than 0; d_x, d_frame, d_mfcc and d_flags non-NULL.
 * Kernel (auditory_kernel: one launch on `stream`, no host wait, no copy, no arena: ev_alloc_count never moves): one workgroup of four waves per
 *   (row, 15 frames): the 16 matrix rows of a tile are the 15 frames and the one before them, carried for the first flux only, so no spectrum crosses
 *   a workgroup; phase 1 is ev_voice_quality's first matrix product into a power spectrum in LDS; phase 2, after one barrier, the product with mel_w
 *   on the matrix cores (one band tile per wave) and the flux (16 lanes per frame); phase 3 the band terms; phase 4, after a second barrier, the
 *   cepstral coefficients (a thread per (frame, i)) and the frame's figures.  The call is capturable. */
int ev_load_auditory(ev_handle *h, const double *window /* HOST (W) */, const double *twiddle /* HOST (nfft, 2) */, int W, int H, int nfft,
                     const double *mel_w /* HOST (NB, n_mel) */, int n_mel, const double *eq /* HOST (n_mel) */,
                     const double *dct /* HOST (n_mel, n_ceps) */, int n_ceps, int k_lo, int k_hi, double compress /* 0.33 */);
int ev_auditory(ev_handle *h, const float *d_x /* (B, L) */, const int32_t *d_len /* (B) or NULL */, int B, int L, double power_floor,
                double *d_frame /* (B, NF, 4) */, double *d_mfcc /* (B, NF, n_ceps) */, int32_t *d_flags /* (B, NF) */,
                double *d_bands /* (B, NF, n_mel) or NULL */, void *stream);

/* Timing hooks for bench.py: HIP-event time (ms) of the dominant kernel family
 * (implicit-GEMM convs, fused pairs, fused LayerNorm + MLP, fused attention) accumulated over the calls since the last reset,
 * measured on the stream the kernels run on. */
int ev_profile_enable(ev_handle *h, int on);
int ev_profile_read(ev_handle *h, double *conv_ms, double *conv_flops, int64_t *conv_launches, int reset);
/* ... and, of those, the launches that ran on the bf16 matrix pipe (conv_split_kernel, conv_split_bal_kernel,
 * resblock_pair_split_kernel: every fp32 product as six exact bf16 products, fp32 accumulation); call before a resetting
 * ev_profile_read.  The rest of the family runs on v_mfma_f32_32x32x2_f32. */
int ev_profile_read_split(ev_handle *h, double *ms, double *flops, int64_t *launches);
/* Arithmetic of the contractions.  Tensors are fp32 and every accumulation is fp32 in every setting.
 *   16 (default): layers deep enough to pay for it form each fp32 product from THREE fp16 x fp16 products on the fp16 matrix pipe: an
 *                 operand, times a power-of-two block scale (weights: one per layer; activations: one per workgroup tile, from the
 *                 tile's maximum), is cut into two fp16 pieces h0 + h1 (22-23 significand bits), the product is h0 g0 + h0 g1 + h1 g0.
 *                 Errors against fp64 at the level of the fp32 FMA chain (one conv layer, tools/arith_accuracy.py: rms 3.4e-7 of the
 *                 output scale against 5.4e-7 for the fp32 MFMA), independent of the activations' scale; ~2.1x the fp32 MFMA's throughput
 *   6:            three bf16 pieces per operand (exact split, no range handling), the six products of weight <= 2: fp32-grade too, ~1.45x
 *   0:            every layer on the fp32 MFMA (v_mfma_f32_32x32x2_f32, bit-identical to an fmaf chain)
 *   3:            opt-in fast bf16 setting of the vocoder's deep layers: three products of weight <= 1, ~16 significand bits per product
 *                 (waveform RMS difference to the fp32 MFMA result 7e-5 against 1.7e-6 for 16 and 6): inside the 1e-3 gate, NOT fp32-grade
 *   9:            accuracy A/B of conv_split_kernel only (tools/bf16_split_probe.hip); the other split builds run 6
 * The environment variable EV_SPLIT presets it for handles created afterwards.  Takes effect with the next call on the handle. */
int ev_set_arithmetic(ev_handle *h, int setting);
int ev_get_arithmetic(ev_handle *h);

/* Test hook: the build the last conv / fused-pair launch of this handle took (tile configuration id: 0 / 1 / 2 / 5 / 6 / 8 = conv_gemm_kernel
 * tiles, 56 = the balanced 64 x 64 grid, 9 / 19 = the split-K small-launch builds, 40 / 60 = conv_split_kernel / its balanced grid, 46 / 47 / 66 =
 * the fp16 builds, 140 + taps = resblock_pair_split_kernel, 160 + taps = resblock_pair_h16_kernel, 100 + taps = resblock_pair_kernel, others:
 * see launch_conv). */
int ev_dbg_last_cfg(ev_handle *h);

/* Kernel microbenchmark hook (tools/conv_bench.py, not part of the product path): times `iters` launches of one
 * resblock-style conv (prologue leaky-relu, bias, residual) at a given geometry with HIP events on the default stream;
 * dbg = ablation bits, cfg = forced tile configuration + 100 x workgroups per CU (< 0: the engine's own choice).  A forced
 * configuration must be one launch_conv selects (0, 1, 2, 5, 6, 8, 9, 19, 40, 41, 43, 46, 49, 60); any other value, and the
 * retired two-chunk staging (cfg >= 1000), fails the call.  EV_FORCE_CFG takes the same values. */
int ev_dbg_conv_bench(ev_handle *h, int Cin, int Cout, int K, int dil, int B, int T, int P, int iters, int dbg, int cfg, float *ms_out);

/* Diagnostic / A-B switch: the fp16 builds need max |x| over the rows a tile stages.  on = 1 (default): they take it from the bounds their
 * producers left per 128-row granule (every launch of ev_hifigan's chain leaves an upper bound of |y| from its accumulators — no second read
 * of the input); on = 0: every tile pre-scans its input (the behaviour before ABI 4; also what inputs without bounds get).  The environment
 * variable EV_NO_AMAX=1 presets 0 for handles created afterwards.  Results differ only through the choice of the power-of-two block scale. */
int ev_dbg_set_amax(ev_handle *h, int on);
/* Diagnostic / A-B switch (ABI 4): on = 1 (default): under arithmetic setting 16 the self-attention of the U-Net's transformer blocks (transformer.py:262-271)
 * runs on the fp16 matrix pipe — q, k, v leave the LayerNorm + projection kernel as fp16 piece pairs times a power of two that the loader derives from a
 * bound no input can exceed, and both products of the attention use all piece products (22-bit operands, fp32 accumulation); on = 0: the attention
 * stays on the fp32 MFMA as before ABI 4.  EV_NO_ATTN_H16=1 presets 0 for handles created afterwards.  Arithmetic settings 6 / 0 never take this path. */
int ev_dbg_set_attn_h16(ev_handle *h, int on);
/* Diagnostic / A-B switch (ABI 4): on = 1 (default): under arithmetic setting 16, ev_hifigan runs a whole ResBlock1 (hifigan/models.py:90-97: three
 * (dilated conv, conv) pairs with their residual adds) as ONE launch where the level is narrow (32 / 64 channels) and the kernel size small enough
 * for the summed halos (k = 3): the running x stays in registers between the pairs; on = 0: three fused-pair launches as before.  EV_NO_CHAIN=1
 * presets 0.  The same switch turns off the one-launch ResBlock2 (resblock2_h16_kernel; off: one conv launch per step).
 * Results differ by rounding only (other tile boundaries, hence other power-of-two tile scales). */
int ev_dbg_set_chain(ev_handle *h, int on);

/* Diagnostic: the control words of the balanced ("stream-K") launches (ev_kernels.h, SkCtl) after a device synchronisation:
 * out3 = {launches so far (epoch), arrivals of an unfinished launch (0), hand-off waits that ran out and were recomputed}. */
int ev_dbg_sk_stats(ev_handle *h, uint32_t *out3);
/* Diagnostic (ABI 4): contributor shares the owners of balanced launches took over because the contributor had not started yet (an owner no
 * longer waits for a workgroup that is not resident — with two pipelines in flight the vocoder holds CU slots — it computes the share itself,
 * with the bits the contributor would have delivered), since the handle was created; -1 on error.  Synchronises the device. */
int64_t ev_dbg_sk_taken(ev_handle *h);

/* ---- operator-level entry points (unit parity tests call these) ------------------
 * Activations here are frame-major (rows, C) fp32 with an explicit row stride. */
int ev_op_conv1d(ev_handle *h, const float *d_x /*(B,Cin,T)*/, const float *w /*HOST (Cout,Cin,K)*/,
                 const float *bias /*HOST (Cout) or NULL*/, int B, int Cin, int T, int Cout, int K, int dilation,
                 int transposed, int stride, int padding, float pre_lrelu_slope /*<0: none*/, float *d_y, void *stream);
/* ev_op_conv1d with the whole fused epilogue of a conv launch (tests/test_gpu_conv.py).  The layer is packed and the input staged exactly as
 * ev_op_conv1d does ('same' conv; stride-2 k3 over the pair view, even T and P; polyphase transposed conv), then ONE launch runs with this
 * epilogue, in the order  +bias, act, *mask1, *scale, +R, +Yold, /3, lrelu(act2_slope), *mask2,  and Y2 = v * rowmask beside it.
 * Sizes and lengths are in OUTPUT frames Tout (T; T / 2; T * stride). */
typedef struct ev_conv_epi {
  int32_t act;                /* 0 none, 1 leaky-relu(act_slope in [0, 1]), 2 tanh, 3 SiLU, 4 Mish, 5 SnakeBeta */
  float act_slope;
  const float *d_alpha_exp;   /* SnakeBeta: exp(alpha) and 1 / (exp(beta) + 1e-9), device (Cout), 16-byte aligned */
  const float *d_beta_inv;
  const int32_t *d_lengths;   /* device (B) valid output frames per utterance, or NULL (no row mask; mask1 / mask2 / d_y2 need it; not with transposed) */
  int32_t mask1, mask2;
  float scale;
  const float *d_R;           /* device (B, Cout, Tout) or NULL */
  int32_t accum;              /* add what Y held before the launch: d_yold */
  const float *d_yold;        /* device (B, Cout, Tout) or NULL: the valid frames of Y before the launch (NULL: EV_CONV_EPI_SENTINEL) */
  int32_t div3;
  float act2_slope;           /* < 0: none */
  float pre_lrelu_slope;      /* < 0: none */
} ev_conv_epi;
#define EV_CONV_EPI_SENTINEL 1234.5f
/* P: pad rows a side of every utterance (input frames); fewer than the layer's halo is refused.  Y's pad rows hold EV_CONV_EPI_SENTINEL before
 * the launch.  d_y (B, Cout, Tout): the valid frames; d_y2 (B, Cout, Tout) or NULL: the second output; d_ypad or NULL: the whole padded
 * frame-major Y, (B * (Tout + 2 * Pout), Cout) with Pout = P (stride 1), P / 2 (stride 2), P * stride (transposed).  Bad arguments fail the
 * call with a message and launch nothing.  bias NULL is allowed.  Column-split views, GroupNorm statistics and amax emission are not reachable. */
int ev_op_conv1d_epi(ev_handle *h, const float *d_x /*(B,Cin,T)*/, const float *w /*HOST, as ev_op_conv1d*/, const float *bias /*HOST or NULL*/,
                     int B, int Cin, int T, int Cout, int K, int dilation, int transposed, int stride, int padding, int P,
                     const ev_conv_epi *ep, float *d_y, float *d_y2, float *d_ypad, void *stream);
int ev_op_groupnorm_mish(ev_handle *h, const float *d_x /*(B,C,T)*/, const float *d_gamma, const float *d_beta,
                         const int32_t *d_lengths, int B, int C, int T, int groups, float *d_y, void *stream);
/* ev_op_groupnorm_mish with the three epilogues of the U-Net's ResnetBlock1D (GNParams in ev_kernels.h): mode 0: mish(gn(x)) * m; mode 1:
 * (mish(gn(x)) * m + temb[c]) * m with d_temb (1, 256) and temb_stride 0 (every utterance shares one row) or (B, 256) and temb_stride 256;
 * mode 2: mish(gn(x)) * m + R with d_R (B, 256, T).  X and R are staged as the estimator holds them: one 512-wide frame-major buffer, X in
 * columns [0, 256), R in [256, 512).  d_temb / d_R may be NULL in the modes that do not read them. */
int ev_op_groupnorm_mish2(ev_handle *h, const float *d_x /*(B,C,T)*/, const float *d_gamma, const float *d_beta,
                          const int32_t *d_lengths, int B, int C, int T, int groups, int mode, const float *d_temb,
                          int temb_stride, const float *d_R, float *d_y, void *stream);
/* One utterance through conv (Cin -> 256, K taps, 'same' padding; w, bias HOST) and GroupNorm + Mish (mode as above, d_temb (256),
 * d_R (1, 256, T)) the way the estimator chains them: the conv is asked for per-tile GroupNorm statistics and the norm is handed them.
 * d_conv (1, 256, T): the conv output; d_part (256 x 8 x 4): per (32-row tile of the padded utterance: 2 pad rows in front, group)
 * {count, mean, M2, -}; d_y (1, 256, T); *tiles_out: row tiles whose statistics the conv left (0: it took a build that leaves none and
 * the norm computed its own). */
int ev_op_conv_groupnorm(ev_handle *h, const float *d_x /*(1,Cin,T)*/, const float *w /*HOST (256,Cin,K)*/,
                         const float *bias /*HOST (256) or NULL*/, int Cin, int T, int K, const float *d_gamma,
                         const float *d_beta, const int32_t *d_lengths /*(1)*/, int mode, const float *d_temb, const float *d_R,
                         float *d_conv, float *d_part, float *d_y, int *tiles_out, void *stream);
/* The three bf16 pieces (as fp32 values, (3, n)) the split builds cut every fp32 operand into: p0 + p1 + p2 == x exactly. */
int ev_op_split_pieces(ev_handle *h, const float *d_x, int n, float *d_pieces, void *stream);
int ev_op_layernorm(ev_handle *h, const float *d_x /*(rows,C)*/, const float *d_gamma, const float *d_beta, int rows,
                    int C, float *d_y, void *stream);
/* ln_mlp_kernel: y = x + W2.SnakeBeta(W1.LN(x) + b1) + b2, rows * mask (mode 0; transformer.py:300-316) or y = W1.LN(x) [+ b1]
 * (mode 1: the QKV projection, y is (rows, M1)); x (rows, 256); alpha_exp = exp(alpha), beta_inv = 1/(exp(beta)+1e-9) (M1);
 * w1 (M1, 256) and w2 (256, M1) are HOST pointers; M1 a multiple of 128; rowmask (rows) or NULL. */
int ev_op_ln_mlp(ev_handle *h, const float *d_x, const float *d_ln_g, const float *d_ln_b, const float *w1, const float *b1,
                 const float *d_alpha_exp, const float *d_beta_inv, const float *w2, const float *b2, const float *d_rowmask,
                 int rows, int M1, int mode, float *d_y, void *stream);
int ev_op_attention(ev_handle *h, const float *d_qkv /*(B,T,3*heads*64)*/, const int32_t *d_lengths, int B, int T,
                    int heads, float *d_out /*(B,T,heads*64)*/, void *stream);

/* attn_out_kernel: d_hid (B*T, 256) <- d_hid + Wout . Attention(d_qkv) + bout, both heads, additive float mask (transformer.py:262-271);
 * d_qkv (B, T, 384) = [q | k | v] x (2 heads x 64); w_out (256, 128) and b_out (256) are HOST pointers. */
int ev_op_attn_out(ev_handle *h, const float *d_qkv, const int32_t *d_lengths, int B, int T, const float *w_out, const float *b_out,
                   float *d_hid, void *stream);

/* The two attention ops as the estimator launches them (launch_attn / launch_attn_out in ev_engine.hip).
 * Geometry: utterance b's frame t is row b * S + P + t of every buffer, S >= P + T (the estimator's level 0: S = T + 4, P = 2); rows outside
 * [P, P + T) are neither read as queries or keys nor written.  d_lengths (B) int32: the additive float mask is 1.0 on keys t < length, 0.0 on
 * the padded frames, which stay live keys (transformer.py:262-271).
 * ev_op_attention2: heads = 2 only; d_qkv (B*S, 3*heads*64), d_out (B*S, heads*64).  no_scratch = 0: launch_attn is handed split-key scratch sized as the
 *   estimator's and picks the build by its own rule (split-key iff few workgroups and >= 4 key tiles); 1: no scratch, always attention_kernel.
 *   ran (2 ints, may be NULL): {0 = attention_kernel | 1 = attention_part_kernel + attention_merge_kernel, KS = parts per query tile (else 0)}.
 * ev_op_attn_out2: d_qkv (B*S, 384), d_hid (B*S, 256) in place; w_out (256, 128), b_out (256) HOST.  sq, sk, sv: the powers of two of the fp16
 *   form (what qkv_pack_scales derives from a weight bound); all three 0 = derive them from the data's maxima, as ev_op_attn_out does (some but not all 0 is refused).  They
 *   matter only where the fp16 pipe runs (arithmetic setting 16 with ev_dbg_set_attn_h16 on).
 *   ran (3 ints, may be NULL): {0 = attn_out_kernel | 1 = attn_out_h16_kernel, ntail = queries of a short last tile that attn_tail_path took
 *   (0: none), nq = 32-query tiles per utterance on the main path}. */
int ev_op_attention2(ev_handle *h, const float *d_qkv, const int32_t *d_lengths, int B, int S, int P, int T, int heads, int no_scratch,
                     float *d_out, int *ran, void *stream);
int ev_op_attn_out2(ev_handle *h, const float *d_qkv, const int32_t *d_lengths, int B, int S, int P, int T, const float *w_out,
                    const float *b_out, float sq, float sk, float sv, float *d_hid, int *ran, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* EMOJIVOICE_H */
