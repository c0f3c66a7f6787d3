"""The analysis side: counterpart of ``matcha.utils.audio`` (the same function again in ``hifigan/meldataset.py:52``).

    mel = mel_spectrogram(y, 1024, 80, 22050, 256, 1024, 0, 8000, center=False)     # (B, L) on the GPU -> (B, 80, L / 256)

``mel_spectrogram`` runs entirely in the HIP library (``ev_mel_spectrogram``: reflect padding, the DFT-basis convolution of the
denoiser, then one kernel for magnitude / mel projection / log compression); there is no torch fallback.  The reference takes its
filter bank from ``librosa.filters.mel``; ``mel_filterbank`` restates that function's defaults (Slaney scale, Slaney normalisation)
from the published definition.

In front of it, for recordings that are not at 22.05 kHz (the reference's own recorder writes 44.1 kHz, its data module asserts 22050):

    y = load_audio("voice.wav", 22050)                        # any rate, 16 / 24 bit, any channel count -> (1, L) on the GPU
    y = resample(y, 44100, 22050)                             # (B, L) on the GPU -> (B, ceil(L / 2)): ev_resample, scipy's resample_poly

and behind it ``data_statistics``: the mel_mean / mel_std a fine-tuning config needs (utils/generate_data_statistics.py), reduced on the
device by ``ev_mel_stats``.

Between a raw take and all of that (the recorder's files begin and end on a key press, at the microphone's level):

    y, (start, end) = trim_silence(y)                         # librosa.effects.trim's call shape, on the device (ev_trim_bounds / ev_trim_apply)
    y = peak_normalize(y, 0.95)                               # normalize(audio) * 0.95 of hifigan/meldataset.py:152
    y, info = prepare_recording("take.wav", 22050)            # load_audio -> trim -> level: one read of the bounds comes back to the host

And beside the mel, frame for frame, the pitch (``ev_pitch_yin``: YIN; librosa.yin is the model):

    p = pitch_yin(y)                                          # {"f0" (B, F) Hz, "voiced" (B, F) bool, "aperiodicity" (B, F)}, F = ceil(L / 256)
    p = pitch_pyin(y)                                         # {"f0", "voiced", "voiced_prob"}: probabilistic YIN + Viterbi (ev_pyin_observe / ev_pyin_decode; librosa.pyin)
    s = prosody_statistics(p["f0"], p["voiced"])              # voiced fraction, f0 median / 5th / 95th percentile, range in semitones per row

And between a recording and its synthesised rendering, which differ in length and timing (``ev_dtw``: dynamic time warping):

    a = dtw(mel_cepstrum(mel_a), mel_cepstrum(mel_b))         # {"cost" (B,) float64, "steps" (B,), "path" (B, Ta + Tb - 1, 2)}
    mcd = mel_cepstral_distortion(mel_a, mel_b)               # dB per utterance over the aligned frame pairs
    e = f0_errors(f0_a, voiced_a, f0_b, voiced_b, a["path"], a["steps"])   # f0 RMSE in cents, voicing-decision error along the path

And level as a listener hears it (``ev_loudness``: ITU-R BS.1770-4 / EBU R 128 integrated loudness; peak says little about it):

    r = loudness(y)                                           # {"integrated" (B,) LUFS, "momentary" (B, NB) LUFS, "blocks", "gated_blocks", "sub_energy"}
    y, gain_db, capped = loudness_normalize(y, -23.0)         # every row to -23 LUFS, the gain capped where the peak would pass 0.95

And a processed waveform against the sample-aligned recording it was made from (``ev_stoi``: STOI, Taal et al. 2011, and ESTOI, Jensen and
Taal 2016 — what copy synthesis through a vocoder costs in intelligibility):

    r = stoi(recording, synthesis)                            # {"stoi" (B,), "estoi" (B,), "segments" (B, NSEG, 2), "counts" (B, 3), "keep" (B, NF)}

And their spectral-magnitude distance (``ev_stft_dist``: the multi-resolution STFT distance of Yamamoto et al. 2020 and the log-spectral
distance, a float64 DFT on the matrix cores):

    r = stft_distance(recording, synthesis)                   # {"mstft" (B,), "sc" (B,), "log_mag" (B,), "lsd_db" (B,), "per_resolution", "frames" (B, 3)}

And voice quality, what separates a tense voice from a breathy or a flat one (``ev_voice_quality``: the spectral-balance descriptors of
eGeMAPS, Eyben et al. 2016, and the cepstral peak prominence of Hillenbrand et al. 1994, per frame on ``pitch_yin``'s frames; the figures are
comparable across this project's runs, not to the digit with Praat or VoiceSauce):

    vq = voice_quality(y)                                     # {"cpp_db", "alpha_ratio_db", "hammarberg_db", "slope_0_500", "slope_500_1500", "power",
                                                              #  "peak_quefrency", "cepstral_f0"}, each (B, F)
    st = voice_quality_statistics(vq, pitch_yin(y)["voiced"]) # per row the means over the voiced, non-silent frames, their count and the sums
"""
from __future__ import annotations

import itertools
import math
import wave
from typing import Callable, Dict, Iterable, Optional, Tuple

import numpy as np
import torch

from ._lib import Engine, EvLibraryError  # noqa: F401  (EvLibraryError: what every call here raises without the library / a GPU)

_F_SP = 200.0 / 3.0                 # Hz per mel below 1 kHz
_MIN_LOG_HZ = 1000.0
_MIN_LOG_MEL = _MIN_LOG_HZ / _F_SP  # = 15
_LOGSTEP = math.log(6.4) / 27.0     # mel step of the logarithmic part


def hz_to_mel(f):
    """Slaney's mel scale (Auditory Toolbox): linear below 1 kHz, logarithmic above."""
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= _MIN_LOG_HZ, _MIN_LOG_MEL + np.log(np.maximum(f, 1e-300) / _MIN_LOG_HZ) / _LOGSTEP, f / _F_SP)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= _MIN_LOG_MEL, _MIN_LOG_HZ * np.exp(_LOGSTEP * (m - _MIN_LOG_MEL)), _F_SP * m)


def mel_filterbank(sr: int, n_fft: int, n_mels: int, fmin: float = 0.0, fmax: Optional[float] = None) -> np.ndarray:
    """The (n_mels, n_fft // 2 + 1) triangular filter bank ``librosa.filters.mel(sr=, n_fft=, n_mels=, fmin=, fmax=)`` returns
    with its defaults (``htk=False, norm="slaney"``): band edges equally spaced on Slaney's mel scale between fmin and fmax
    (None: sr / 2), each triangle scaled by 2 / (f_hi - f_lo).  Computed in float64, rounded once to float32."""
    if fmax is None:
        fmax = sr / 2.0
    n_freq = n_fft // 2 + 1
    fft_f = np.arange(n_freq, dtype=np.float64) * (float(sr) / n_fft)
    edges = mel_to_hz(np.linspace(float(hz_to_mel(fmin)), float(hz_to_mel(fmax)), n_mels + 2))
    fdiff = np.diff(edges)
    ramps = edges[:, None] - fft_f[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper))
    w *= (2.0 / (edges[2:] - edges[:-2]))[:, None]
    return w.astype(np.float32)


# (device index, sr, n_mels, fmin, fmax) -> Engine with that bank loaded; the reference caches per (fmax, device)
_engines: Dict[Tuple, Engine] = {}


def _engine_for(device: torch.device, sr, n_mels, fmin, fmax) -> Engine:
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (idx, int(sr), int(n_mels), float(fmin), None if fmax is None else float(fmax))
    eng = _engines.get(key)
    if eng is None:
        eng = Engine(idx)
        eng.load_mel_basis(mel_filterbank(sr, 1024, n_mels, fmin, fmax))
        _engines[key] = eng
    return eng


def _check_args(n_fft, num_mels, hop_size, win_size, center) -> None:
    if n_fft != 1024 or win_size != 1024:
        raise ValueError(f"mel_spectrogram: the HIP engine implements n_fft = win_size = 1024 only (got n_fft={n_fft}, win_size={win_size})")
    if hop_size != 256:
        raise ValueError(f"mel_spectrogram: the HIP engine implements hop_size = 256 only (got {hop_size})")
    if center:
        raise ValueError("mel_spectrogram: the HIP engine implements center=False only (the reference's only call)")
    if not 1 <= int(num_mels) <= 128:
        raise ValueError(f"mel_spectrogram: num_mels must be 1..128 (got {num_mels})")


@torch.inference_mode()
def mel_spectrogram(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False, out_scale: float = 1.0,
                    out_shift: float = 0.0):
    """``matcha.utils.audio.mel_spectrogram`` (utils/audio.py:45-82): ``y`` (B, L) on the GPU -> log-mel (B, num_mels, L / 256).

    What the engine does not implement raises ``ValueError``: n_fft = win_size = 1024, hop_size 256, center=False, L a multiple of
    256 (and > 384, which the reflect padding needs as in torch).  The filter bank and the native handle are cached per
    (device, sampling_rate, num_mels, fmin, fmax).  The reference's two ``print``s for samples outside [-1, 1] are not reproduced:
    they would force a host synchronisation on every call.  ``out_scale`` / ``out_shift`` (not in the reference) fuse
    ``normalize(mel, mel_mean, mel_std)`` of utils/model.py: 1 / mel_std and -mel_mean / mel_std."""
    _check_args(n_fft, num_mels, hop_size, win_size, center)
    if y.dim() != 2:
        raise ValueError(f"mel_spectrogram: y must be (B, L), got shape {tuple(y.shape)}")
    L = int(y.shape[1])
    if L % 256 or L <= 384:
        raise ValueError(f"mel_spectrogram: L must be a multiple of 256 and > 384 (got {L}); trim or pad the signal")
    if not y.is_cuda:
        raise EvLibraryError("mel_spectrogram runs on a ROCm GPU only (no CPU fallback): move y to the GPU")
    return _engine_for(y.device, sampling_rate, num_mels, fmin, fmax).mel_spectrogram(y, out_scale, out_shift)


@torch.inference_mode()
def mel_reconstruction_error(vocoder, mel, lengths=None):
    """Per-utterance mean |mel - mel_spectrogram(vocoder(mel))| over the valid frames and all mel bins, (B,) on the device: HiFi-GAN's
    validation measure (the ``mel_loss`` spectrogram of hifigan/meldataset.py:202 against the generator's output, without the x45
    training weight), with the analysis parameters of the vocoder's config (fmax = ``h.fmax``: the bank the input mel was made
    with).  ``lengths`` (B,): valid frames per utterance (None: all).  Nothing leaves the device."""
    h = vocoder.h
    mel = mel.to(vocoder.device, torch.float32)
    wav = vocoder(mel).squeeze(1)
    got = mel_spectrogram(wav, h.get("n_fft", 1024), h.get("num_mels", 80), h.get("sampling_rate", 22050), h.get("hop_size", 256),
                          h.get("win_size", 1024), h.get("fmin", 0), h.get("fmax", 8000))
    diff = (mel - got).abs()
    B, M, T = diff.shape
    if lengths is None:
        return diff.mean(dim=(1, 2))
    lengths = lengths.to(diff.device)
    mask = (torch.arange(T, device=diff.device)[None, :] < lengths[:, None]).to(diff.dtype)
    return (diff * mask[:, None, :]).sum(dim=(1, 2)) / (lengths.to(diff.dtype) * M)


def read_wav_pcm(path, sr: int = 22050) -> np.ndarray:
    """A mono 16- or 24-bit PCM wav at ``sr`` as float32 in [-1, 1): the inverse of ``cli.write_wav_pcm24`` for 24-bit files
    (q / (2**23 - 1)), q / 32768 for 16-bit ones (MAX_WAV_VALUE of utils/audio.py)."""
    with wave.open(str(path), "rb") as f:
        if f.getnchannels() != 1:
            raise ValueError(f"{path}: {f.getnchannels()} channels (mono only)")
        if f.getframerate() != sr:
            raise ValueError(f"{path}: {f.getframerate()} Hz (this front end does not resample: {sr} Hz only)")
        width, raw = f.getsampwidth(), f.readframes(f.getnframes())
    if width == 2:
        return (np.frombuffer(raw, dtype="<i2").astype(np.float64) / 32768.0).astype(np.float32)
    if width == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3)
        q = np.zeros((b.shape[0], 4), dtype=np.uint8)
        q[:, 1:] = b                                              # into the top three bytes: the shift back sign-extends
        q = q.reshape(-1).view("<i4") >> 8
        return (q.astype(np.float64) / (2**23 - 1)).astype(np.float32)
    raise ValueError(f"{path}: {8 * width}-bit samples (16- or 24-bit PCM only)")


def read_wav(path) -> Tuple[np.ndarray, int]:
    """(float32 samples in [-1, 1), rate) of a 16- or 24-bit PCM wav at ANY rate; several channels are averaged in float64.  The
    sample scaling is ``read_wav_pcm``'s (q / 32768, q / (2**23 - 1))."""
    with wave.open(str(path), "rb") as f:
        ch, rate, width, raw = f.getnchannels(), f.getframerate(), f.getsampwidth(), f.readframes(f.getnframes())
    if width == 2:
        q = np.frombuffer(raw, dtype="<i2").astype(np.float64) / 32768.0
    elif width == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3)
        w = np.zeros((b.shape[0], 4), dtype=np.uint8)
        w[:, 1:] = b                                              # into the top three bytes: the shift back sign-extends
        q = (w.reshape(-1).view("<i4") >> 8).astype(np.float64) / (2**23 - 1)
    else:
        raise ValueError(f"{path}: {8 * width}-bit samples (16- or 24-bit PCM only)")
    if ch > 1:
        q = q.reshape(-1, ch).mean(axis=1)
    return q.astype(np.float32), int(rate)


def resample_ratio(orig_sr: int, new_sr: int) -> Tuple[int, int]:
    """(up, down) of a conversion orig_sr -> new_sr: the rates over their gcd (44100 -> 22050: (1, 2); 48000 -> 22050: (147, 320))."""
    orig_sr, new_sr = int(orig_sr), int(new_sr)
    if orig_sr < 1 or new_sr < 1:
        raise ValueError(f"resample: sample rates must be positive (got {orig_sr} -> {new_sr})")
    g = math.gcd(orig_sr, new_sr)
    return new_sr // g, orig_sr // g


def resample_filter(up: int, down: int, zeros: int = 10, beta: float = 5.0) -> np.ndarray:
    """The low-pass of ``scipy.signal.resample_poly(x, up, down)`` restated: with m = max(up, down), 2 * zeros * m + 1 taps
    sinc(n / m) / m * kaiser(beta) for n = -zeros * m .. zeros * m, normalised to unit sum, times ``up``
    (= ``firwin(2 * zeros * m + 1, 1 / m, window=("kaiser", beta)) * up``; zeros = 10 and beta = 5.0 are scipy's defaults).  Computed in
    float64, rounded once to float32."""
    return _resample_filter64(up, down, zeros, beta).astype(np.float32)


def _resample_filter64(up: int, down: int, zeros: int = 10, beta: float = 5.0) -> np.ndarray:
    m = max(int(up), int(down))
    half = int(zeros) * m
    n = np.arange(-half, half + 1, dtype=np.float64)
    h = np.sinc(n / m) / m * np.kaiser(2 * half + 1, float(beta))
    return h / h.sum() * up


# (device index, up, down, zeros, beta) -> Engine with that filter loaded; (device index, "stats") -> the Engine of data_statistics
_rs_engines: Dict[Tuple, Engine] = {}


def _cached_engine(device: torch.device, key: Tuple, load: Optional[Callable] = None) -> Engine:
    """The Engine of ``_rs_engines`` under (device index, *key), made on first use; ``load(engine)`` puts its tables in before it is kept."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    eng = _rs_engines.get((idx,) + key)
    if eng is None:
        eng = Engine(idx)
        if load is not None:
            load(eng)
        _rs_engines[(idx,) + key] = eng
    return eng


def _resampler_for(device: torch.device, up: int, down: int, zeros: int, beta: float) -> Engine:
    return _cached_engine(device, (int(up), int(down), int(zeros), float(beta)),
                          lambda eng: eng.load_resampler(resample_filter(up, down, zeros, beta), up, down))


@torch.inference_mode()
def resample(y, orig_sr: int, new_sr: int, lengths=None, zeros: int = 10, beta: float = 5.0):
    """``y`` (B, L) on the GPU at ``orig_sr`` -> (B, ceil(L * up / down)) at ``new_sr``, up / down the rates over their gcd: what
    ``scipy.signal.resample_poly(y, up, down, axis=-1)`` computes (zero padding, its default Kaiser filter for zeros = 10, beta = 5.0),
    in the HIP library (``ev_resample``; no torch fallback).  ``lengths`` (B,): samples per row of a padded batch; the outputs past
    ceil(len * up / down) are zeros.  ``orig_sr == new_sr`` returns ``y`` itself.  The filter and the native handle are cached per
    (device, up, down, zeros, beta); a ratio outside 1 <= up, down <= 640 raises ``EvLibraryError``."""
    if int(orig_sr) == int(new_sr):
        return y
    up, down = resample_ratio(orig_sr, new_sr)
    if y.dim() != 2:
        raise ValueError(f"resample: y must be (B, L), got shape {tuple(y.shape)}")
    if not y.is_cuda:
        raise EvLibraryError("resample runs on a ROCm GPU only (no CPU fallback): move y to the GPU")
    return _resampler_for(y.device, up, down, zeros, beta).resample(y, lengths)


def load_audio(path, sr: int = 22050, device="cuda"):
    """A wav at any rate (``read_wav``) as a (1, L) float32 tensor on ``device`` at ``sr``, resampled on the device when the file's
    rate differs."""
    y, rate = read_wav(path)
    return resample(torch.from_numpy(y).to(device).unsqueeze(0), rate, sr)


def statistics_from_sums(sum_x: float, sum_x2: float, total_len: int, n_feats: int) -> Dict[str, float]:
    """compute_data_statistics' last two lines (utils/generate_data_statistics.py:44-45) in Python float64."""
    n = float(total_len) * float(n_feats)
    mean = float(sum_x) / n
    return {"mel_mean": mean, "mel_std": math.sqrt(float(sum_x2) / n - mean * mean)}


def _device_row_sums(mel, lengths) -> np.ndarray:
    if not mel.is_cuda:
        raise EvLibraryError("data_statistics runs on a ROCm GPU only (no CPU fallback): move the mels to the GPU")
    return _cached_engine(mel.device, ("stats",)).mel_stats(mel, lengths).cpu().numpy()


def data_statistics(batches: Iterable, n_feats: int = 80, row_sums: Optional[Callable] = None) -> Dict[str, float]:
    """``compute_data_statistics`` (utils/generate_data_statistics.py:25-47) over ``batches``, an iterable of (mel (B, n_feats, T) on
    the GPU, lengths (B,)): {"mel_mean": sum x / (sum len * n_feats), "mel_std": sqrt(sum x^2 / (sum len * n_feats) - mean^2)}.  Each
    batch is reduced on the device to per-row float64 sums over the valid cells (``ev_mel_stats``; the reference sums the zero padding
    too, which adds nothing); rows and batches are combined here in Python float64 (``math.fsum``).  ``row_sums``: the per-batch
    reduction, (mel, lengths) -> (B, 2) float64 array — the device call unless given."""
    reduce = row_sums or _device_row_sums
    sx, sx2, total = [], [], 0
    for mel, lengths in batches:
        if mel.shape[1] != n_feats:
            raise ValueError(f"data_statistics: mel has {mel.shape[1]} channels, n_feats is {n_feats}")
        ln = [int(v) for v in np.asarray(torch.as_tensor(lengths).cpu()).reshape(-1)]
        if any(v < 1 or v > mel.shape[2] for v in ln):
            raise ValueError(f"data_statistics: lengths must be 1..{mel.shape[2]} (got {ln})")
        s = np.asarray(reduce(mel, lengths), dtype=np.float64)
        sx.extend(s[:, 0].tolist())
        sx2.extend(s[:, 1].tolist())
        total += sum(ln)
    if total == 0:
        raise ValueError("data_statistics: no frames")
    return statistics_from_sums(math.fsum(sx), math.fsum(sx2), total, n_feats)


def _trim_engine(device: torch.device) -> Engine:
    return _cached_engine(device, ("trim",))


def _trim_input(y, what: str):
    if not torch.is_tensor(y) or y.dim() not in (1, 2):
        raise ValueError(f"{what}: y must be a 1-D tensor or a (B, L) batch")
    if not y.is_cuda:
        raise EvLibraryError(f"{what} runs on a ROCm GPU only (no CPU fallback): move y to the GPU")
    if y.shape[-1] < 1:
        raise ValueError(f"{what}: y is empty")


@torch.inference_mode()
def trim_silence(y, top_db: float = 60, frame_length: int = 2048, hop_length: int = 512, lengths=None):
    """``librosa.effects.trim(y, top_db=, frame_length=, hop_length=)`` on the device (``ev_trim_bounds`` + ``ev_trim_apply``; no torch
    fallback): a frame of ``frame_length`` samples centred on every ``hop_length``-th sample is non-silent when its mean square lies
    within ``top_db`` dB of the loudest frame's.  ``y`` 1-D on the GPU -> ``(y[start:end], (start, end))``, librosa's return shape.
    ``y`` (B, L) with ``lengths`` (B,) or None -> ``(batch (B, max out_len) zero-padded, out_len (B,) int32, bounds (B, 2) int32)``, all on
    the device.  One read of the bounds goes back to the host, to size the result."""
    _trim_input(y, "trim_silence")
    eng = _trim_engine(y.device)
    x = y.unsqueeze(0) if y.dim() == 1 else y
    bounds, _ = eng.trim_bounds(x, lengths if y.dim() == 2 else None, top_db, frame_length, hop_length, want_peak=False)
    host = bounds.cpu()
    n = int((host[:, 1] - host[:, 0]).max())
    out, out_len = eng.trim_apply(x, bounds, None, 0.0, out_len=max(n, 1))
    if y.dim() == 1:
        return out[0, :n], (int(host[0, 0]), int(host[0, 1]))
    return out[:, :n], out_len, bounds


@torch.inference_mode()
def peak_normalize(y, peak: float = 0.95, lengths=None):
    """``y * (peak / max |y|)`` per row on the device: ``normalize(audio) * 0.95`` of the vocoder's dataset code
    (hifigan/meldataset.py:152; librosa.util.normalize with its default norm=inf).  ``y`` 1-D, or (B, L) with ``lengths`` (B,) or None:
    the samples past a row's length do not enter its peak and come back as zeros.  An all-zero row stays as it is."""
    _trim_input(y, "peak_normalize")
    eng = _trim_engine(y.device)
    x = y.unsqueeze(0) if y.dim() == 1 else y
    B, L = x.shape
    ln = torch.full((B,), L, dtype=torch.int32, device=x.device) if lengths is None or y.dim() == 1 else torch.as_tensor(lengths).to(x.device, torch.int32)
    _, pk = eng.trim_bounds(x, ln)                                   # (the bounds are not used: the peak is the whole row's)
    whole = torch.stack([torch.zeros_like(ln), ln], dim=1)
    out, _ = eng.trim_apply(x, whole, pk, peak)
    return out[0] if y.dim() == 1 else out


@torch.inference_mode()
def prepare_recording(path, sr: int = 22050, top_db: float = 60, peak: float = 0.95, device="cuda"):
    """A raw take -> a fine-tuning sample: ``load_audio`` (any rate or channel count, resampled on the device to ``sr``), the bounds of
    ``trim_silence`` and the whole take's peak (``ev_trim_bounds``), then the trimmed samples times ``peak / max |y|``
    (``ev_trim_apply``).  Returns (1-D waveform on the device, {"start", "end", "seconds_in", "seconds_out"}); the bounds are samples at
    ``sr``.  One read of the bounds goes back to the host, to size the result.  ``peak <= 0`` leaves the level alone."""
    y = load_audio(path, sr, device)
    eng = _trim_engine(y.device)
    bounds, pk = eng.trim_bounds(y, None, top_db)
    start, end = (int(v) for v in bounds[0].cpu())
    out, _ = eng.trim_apply(y, bounds, pk, peak, out_len=max(end - start, 1))
    return out[0, : end - start], {"start": start, "end": end, "seconds_in": y.shape[1] / float(sr), "seconds_out": (end - start) / float(sr)}


def pitch_lag_range(sr: int, fmin: float, fmax: float) -> Tuple[int, int]:
    """The lags YIN searches for f0 in [fmin, fmax] at rate ``sr``: (floor(sr / fmax), ceil(sr / fmin)); the library takes 1 <= tau_min <=
    tau_max <= 2048."""
    if not (0 < fmin <= fmax):
        raise ValueError(f"pitch_yin: 0 < fmin <= fmax expected (got fmin={fmin} fmax={fmax})")
    return int(math.floor(sr / fmax)), int(math.ceil(sr / fmin))


@torch.inference_mode()
def pitch_yin(y, sr: int = 22050, fmin: float = 65.0, fmax: float = 600.0, frame_length: int = 1024, hop_length: int = 256,
              threshold: float = 0.1, lengths=None):
    """The fundamental frequency per frame by YIN on the device (``ev_pitch_yin``; no torch fallback; ``librosa.yin`` is the model): frame f
    is centred where mel frame f of ``mel_spectrogram`` at the same hop is, so the contour lines up with the mel.  ``y`` 1-D, or (B, L)
    with ``lengths`` (B,) samples or None, on the GPU -> {"f0" (B, F) float32 Hz, 0 where unvoiced; "voiced" (B, F) bool; "aperiodicity"
    (B, F) float32: d' at the chosen lag, or its minimum over the search range for an unvoiced frame}, F = ceil(L / hop_length); a 1-D
    input gives B = 1.  Frames past a row's ceil(len / hop_length) are unvoiced with aperiodicity 0."""
    _trim_input(y, "pitch_yin")
    tau_min, tau_max = pitch_lag_range(sr, fmin, fmax)
    eng = _trim_engine(y.device)
    x = y.unsqueeze(0) if y.dim() == 1 else y
    lag, period, cmnd = eng.pitch_yin(x, lengths if y.dim() == 2 else None, frame_length, hop_length, tau_min, tau_max, threshold)
    voiced = lag > 0
    f0 = torch.where(voiced, float(sr) / torch.where(voiced, period, torch.ones_like(period)), torch.zeros_like(period))
    return {"f0": f0, "voiced": voiced, "aperiodicity": cmnd}


def _beta_cdf_integer(x: float, a: int, b: int) -> float:
    """I_x(a, b) for integers a, b >= 1: the upper tail sum_{j >= a} C(n, j) x^j (1 - x)^(n - j) of a binomial over n = a + b - 1 trials."""
    n = a + b - 1
    return float(sum(math.comb(n, j) * x ** j * (1.0 - x) ** (n - j) for j in range(a, n + 1)))


def pyin_threshold_prior(n_thresholds: int = 100, beta_parameters=(2, 18)) -> np.ndarray:
    """pYIN's prior over the YIN threshold, float64 (n_thresholds,): entry t - 1 is the Beta(a, b) mass of ((t - 1) / n, t / n], n =
    ``n_thresholds`` (the ``w`` of ``ev_pyin_observe``).  Integer a, b use the closed form (a binomial tail); others need scipy's
    regularised incomplete beta function."""
    n = int(n_thresholds)
    if not 1 <= n <= 128:
        raise ValueError(f"pitch_pyin: 1 <= n_thresholds <= 128 expected (got {n_thresholds})")
    a, b = beta_parameters
    if not (a > 0 and b > 0):
        raise ValueError(f"pitch_pyin: beta_parameters must be positive (got {beta_parameters})")
    theta = [t / n for t in range(n + 1)]
    if float(a).is_integer() and float(b).is_integer():
        cdf = np.array([_beta_cdf_integer(t, int(a), int(b)) for t in theta], dtype=np.float64)
    else:
        try:
            from scipy.special import betainc
        except ImportError as e:
            raise ValueError(f"pitch_pyin: beta_parameters={beta_parameters} are not integers, which needs scipy") from e
        cdf = np.asarray(betainc(float(a), float(b), np.array(theta)), dtype=np.float64)
    return np.diff(cdf)


def pyin_bins(fmin: float, fmax: float, resolution: float = 0.1) -> Tuple[int, int]:
    """(bins_per_octave, n_bins) of pYIN's pitch grid: 12 ceil(1 / resolution) bins per octave from ``fmin``; bin i is fmin 2^(i / bpo)."""
    if not (0 < fmin < fmax) or not (0 < resolution <= 1):
        raise ValueError(f"pitch_pyin: 0 < fmin < fmax and 0 < resolution <= 1 expected (got fmin={fmin} fmax={fmax} resolution={resolution})")
    bpo = 12 * int(math.ceil(1.0 / resolution))
    return bpo, int(math.floor(bpo * math.log2(fmax / fmin))) + 1


def pyin_transition_radius(sr: int, hop_length: int, bins_per_octave: int, max_transition_rate: float = 35.92) -> int:
    """R, the most bins the pitch may move between two frames: (bpo / 12) round(max_transition_rate 12 H / sr) / 2, rounded down."""
    return int((bins_per_octave // 12) * round(max_transition_rate * 12 * hop_length / sr) / 2)


def pyin_transition(n_bins: int, R: int, switch_prob: float = 0.01):
    """The host tables of ``ev_pyin_decode``, float64: (log_tri (R + 1,): log(R + 1 - d); log_Z (n_bins,): log of the triangle's mass that
    stays inside [0, n_bins) when it is centred on bin j; log_stay = log(1 - switch_prob); log_switch = log(switch_prob))."""
    if not 0 < switch_prob < 1:
        raise ValueError(f"pitch_pyin: 0 < switch_prob < 1 expected (got {switch_prob})")
    n_bins, R = int(n_bins), int(R)
    num = (R + 1 - np.arange(R + 1)).astype(np.float64)
    j = np.arange(n_bins)[:, None]
    i = np.arange(n_bins)[None, :]
    Z = np.clip(R + 1 - np.abs(i - j), 0, None).astype(np.float64).sum(axis=1)          # (integers: exact in any order)
    return np.log(num), np.log(Z), math.log(1.0 - switch_prob), math.log(switch_prob)


PYIN_SLICE_BYTES = 1 << 30           # pitch_pyin processes this much of obs + back at a time


@torch.inference_mode()
def pitch_pyin(y, sr: int = 22050, fmin: float = 65.0, fmax: float = 600.0, frame_length: int = 1024, hop_length: int = 256, lengths=None,
               n_thresholds: int = 100, beta_parameters=(2, 18), boltzmann_parameter: float = 2.0, resolution: float = 0.1,
               max_transition_rate: float = 35.92, switch_prob: float = 0.01, no_trough_prob: float = 0.01):
    """The fundamental frequency per frame by probabilistic YIN on the device (``ev_pyin_observe`` + ``ev_pyin_decode``; no torch fallback;
    ``librosa.pyin`` is the model): every trough of YIN's d' is a candidate with a probability under a Beta prior on the threshold, and a
    Viterbi pass over (voiced / unvoiced) x pitch bins picks the contour, so one frame's octave error or drop-out does not stand against
    its neighbours.  The frames are ``pitch_yin``'s and the mel's.  ``y`` 1-D, or (B, L) with ``lengths`` (B,) samples or None, on the GPU
    -> {"f0" (B, F) float32 Hz: fmin 2^(i / bins_per_octave) of the chosen bin, 0 where unvoiced; "voiced" (B, F) bool; "voiced_prob"
    (B, F) float32: the observation's probability that the frame is voiced}, F = ceil(L / hop_length).  Frames past a row's
    ceil(len / hop_length) are unvoiced with probability 0.  Rows are processed in slices whose obs and back-pointers stay under 1 GiB."""
    _trim_input(y, "pitch_pyin")
    tau_min, tau_max = pitch_lag_range(sr, fmin, fmax)
    bpo, n_bins = pyin_bins(fmin, fmax, resolution)
    R = pyin_transition_radius(sr, hop_length, bpo, max_transition_rate)
    w = pyin_threshold_prior(n_thresholds, beta_parameters)
    log_tri, log_Z, log_stay, log_switch = pyin_transition(n_bins, R, switch_prob)
    eng = _trim_engine(y.device)
    x = y.unsqueeze(0) if y.dim() == 1 else y
    B, L = x.shape
    ln = None if lengths is None or y.dim() == 1 else torch.as_tensor(lengths).to(x.device, torch.int32)
    if ln is not None and ln.numel() != B:
        raise ValueError(f"pitch_pyin: {B} lengths expected, got {ln.numel()}")
    F = -(-L // max(int(hop_length), 1))
    rows = max(1, min(B, PYIN_SLICE_BYTES // max(F * n_bins * 10, 1)))      # 8 bytes of obs and 2 of back per frame and bin
    state = torch.empty((B, F), dtype=torch.int32, device=x.device)
    pv = torch.empty((B, F), dtype=torch.float64, device=x.device)
    obs = torch.empty((rows, F, n_bins), dtype=torch.float64, device=x.device)
    back = torch.empty((rows, F, 2 * n_bins), dtype=torch.uint8, device=x.device)
    for r0 in range(0, B, rows):
        nr = min(rows, B - r0)
        lr = None if ln is None else ln[r0: r0 + nr]
        eng.pyin_observe(x[r0: r0 + nr], lr, frame_length, hop_length, tau_min, tau_max, sr, fmin, bpo, n_bins, w, boltzmann_parameter,
                         no_trough_prob, out=(obs[:nr], pv[r0: r0 + nr]))
        st, _ = eng.pyin_decode(obs[:nr], pv[r0: r0 + nr], lr, L, hop_length, R, log_tri, log_Z, log_stay, log_switch, back=back[:nr])
        state[r0: r0 + nr] = st
    voiced = (state >= 0) & (state < n_bins)
    f0 = torch.where(voiced, float(fmin) * torch.exp2(state.clamp_min(0).to(torch.float64) / float(bpo)), torch.zeros((), dtype=torch.float64,
                                                                                                                     device=x.device))
    return {"f0": f0.to(torch.float32), "voiced": voiced, "voiced_prob": pv.to(torch.float32)}


def semitones(f_hi, f_lo):
    return 12.0 * torch.log2(f_hi / f_lo)


@torch.inference_mode()
def prosody_statistics(f0, voiced, lengths=None):
    """Per utterance, from the contour of ``pitch_yin``: {"voiced_fraction", "f0_median", "f0_p05", "f0_p95" (Hz), "f0_range_semitones" (the
    5-to-95 range)}, each (B,) float32 where ``f0`` lives (torch ops only).  ``f0`` and ``voiced`` are (B, F) or 1-D; ``lengths`` (B,): the
    FRAMES that belong to each row (None: F), the denominator of the voiced fraction.  Percentiles interpolate linearly (numpy's default).
    An utterance without a voiced frame gets NaN for the pitch fields and 0 for the fraction."""
    f0 = torch.as_tensor(f0, dtype=torch.float32)
    voiced = torch.as_tensor(voiced, dtype=torch.bool, device=f0.device)
    if f0.dim() == 1:
        f0, voiced = f0.unsqueeze(0), voiced.unsqueeze(0)
    B, F = f0.shape
    n = torch.full((B,), F, dtype=torch.int64, device=f0.device) if lengths is None else torch.as_tensor(lengths).to(f0.device, torch.int64)
    if n.numel() != B:
        raise ValueError(f"prosody_statistics: {B} lengths expected, got {n.numel()}")
    voiced = voiced & (torch.arange(F, device=f0.device)[None, :] < n[:, None])
    count = voiced.sum(dim=1)
    q = torch.tensor([0.05, 0.5, 0.95], dtype=torch.float32, device=f0.device)
    pct = torch.full((B, 3), float("nan"), dtype=torch.float32, device=f0.device)
    for b in torch.nonzero(count > 0).flatten().tolist():
        pct[b] = torch.quantile(f0[b][voiced[b]], q)
    return {"voiced_fraction": count.float() / n.clamp_min(1).float(), "f0_median": pct[:, 1], "f0_p05": pct[:, 0], "f0_p95": pct[:, 2],
            "f0_range_semitones": semitones(pct[:, 2], pct[:, 0])}


MCD_DB = 10.0 * math.sqrt(2.0) / math.log(10.0)    # dB per unit of Euclidean distance between natural-log cepstra (6.1418...)


def dct_matrix(n_mels: int, n_coeffs: int) -> np.ndarray:
    """Rows 1 .. n_coeffs of the orthonormal DCT-II over ``n_mels`` points, float64 (n_coeffs, n_mels): row k is
    sqrt(2 / n) cos(pi k (2 m + 1) / (2 n)).  Row 0, the energy, is not among them."""
    if not 1 <= n_coeffs < n_mels:
        raise ValueError(f"mel_cepstrum: 1 <= n_coeffs < n_mels expected (got n_coeffs={n_coeffs} n_mels={n_mels})")
    k = np.arange(1, n_coeffs + 1, dtype=np.float64)[:, None]
    m = np.arange(n_mels, dtype=np.float64)[None, :]
    return math.sqrt(2.0 / n_mels) * np.cos(math.pi * k * (2.0 * m + 1.0) / (2.0 * n_mels))


@torch.inference_mode()
def mel_cepstrum(mel, n_coeffs: int = 13):
    """Mel-cepstral coefficients 1 .. ``n_coeffs`` of a log-mel (B, n_mels, T): the orthonormal DCT-II over the mel axis without its 0th
    coefficient (the energy).  The float64 matrix is applied in float64 and the result rounded once to float32: (B, n_coeffs, T) where
    ``mel`` lives (torch ops only)."""
    if mel.dim() != 3:
        raise ValueError(f"mel_cepstrum: mel must be (B, n_mels, T), got shape {tuple(mel.shape)}")
    D = torch.from_numpy(dct_matrix(int(mel.shape[1]), n_coeffs)).to(mel.device)
    return torch.matmul(D, mel.to(torch.float64)).to(torch.float32)


@torch.inference_mode()
def dtw(x, y, x_lengths=None, y_lengths=None, metric="euclidean"):
    """Dynamic time warping on the device (``ev_dtw``; no torch fallback) of ``x`` (B, C, Tx) against ``y`` (B, C, Ty), or (C, T) each for
    one pair: {"cost" (B,) float64: the summed local cost along the best monotone path from (0, 0) to (tx-1, ty-1) with steps diagonal /
    up / left; "steps" (B,) int32: its length K; "path" (B, Tx + Ty - 1, 2) int32: (i, j) per step, (-1, -1) from K on}.  ``metric``:
    "euclidean" or "sqeuclidean" between frames."""
    if not torch.is_tensor(x) or not torch.is_tensor(y) or x.dim() != y.dim() or x.dim() not in (2, 3):
        raise ValueError("dtw: x and y must both be (C, T) tensors or (B, C, T) batches")
    if not x.is_cuda or not y.is_cuda:
        raise EvLibraryError("dtw runs on a ROCm GPU only (no CPU fallback): move x and y to the GPU")
    if x.dim() == 2:
        x, y = x.unsqueeze(0), y.unsqueeze(0)
    cost, steps, path = _trim_engine(x.device).dtw(x, y, x_lengths, y_lengths, metric)
    return {"cost": cost, "steps": steps, "path": path}


def mcd_from_cost(cost, steps):
    """MCD in dB from the DTW cost over Euclidean cepstral distances and the path length: (10 sqrt 2 / ln 10) cost / steps, float64;
    NaN where steps is 0."""
    cost = torch.as_tensor(cost, dtype=torch.float64)
    steps = torch.as_tensor(steps).to(cost.device, torch.float64)
    return torch.where(steps > 0, MCD_DB * cost / steps.clamp_min(1.0), torch.full_like(cost, float("nan")))


@torch.inference_mode()
def mel_cepstral_distortion(mel_a, mel_b, len_a=None, len_b=None, n_coeffs: int = 13):
    """Per-utterance mel-cepstral distortion in dB between two log-mels (B, n_mels, Ta) and (B, n_mels, Tb) of different lengths, (B,)
    float64 on the device: MCD = (10 sqrt 2 / ln 10) * cost / steps, the mean over the frame pairs that dynamic time warping aligns
    (``ev_dtw`` over the Euclidean distance of ``mel_cepstrum``'s coefficients 1 .. ``n_coeffs``) — the convention of mel-spectrogram
    MCD-DTW.  ``len_a`` / ``len_b`` (B,): frames per row (None: all).

    The cepstrum is computed from the log-mel's DCT, not from a WORLD spectral envelope: the figure is comparable across this project's
    runs, not with published WORLD-based MCD figures."""
    out = dtw(mel_cepstrum(mel_a, n_coeffs), mel_cepstrum(mel_b, n_coeffs), len_a, len_b, "euclidean")
    return mcd_from_cost(out["cost"], out["steps"])


ENVELOPE_POWER_FLOOR = 1e-7                        # a frame with no bin of |X|^2 above it is silent; the clamp before the logarithm, ``voice_quality``'s
ENVELOPE_Q1 = -0.15                                # CheapTrick's compensation coefficient
ENVELOPE_CLASSES = ("voiced", "default_period", "silent", "beyond")


def freq_warp_matrix(n_in: int, order: int, alpha: float) -> np.ndarray:
    """The frequency warping of a one-sided cepstrum as a matrix, float64 (order + 1, n_in): column n is what SPTK's ``freqt`` recursion makes
    of the unit vector e_n (for i = n_in - 1 down to 0, with d the g of the previous pass: g[0] = c[i] + alpha d[0]; g[1] = (1 - alpha^2) d[0]
    + alpha d[1]; g[m] = d[m-1] + alpha (d[m] - g[m-1])), so A @ c is freqt of c at ``alpha`` (0.455 suits 22.05 kHz; 0 is the identity)."""
    n_in, order, alpha = int(n_in), int(order), float(alpha)
    if n_in < 1 or order < 0 or not abs(alpha) < 1.0:
        raise ValueError(f"freq_warp_matrix: n_in >= 1, order >= 0 and |alpha| < 1 expected (got n_in={n_in} order={order} alpha={alpha})")
    g = np.zeros((order + 1, n_in), dtype=np.float64)
    for i in range(n_in - 1, -1, -1):
        d = g.copy()
        g[0] = alpha * d[0]
        g[0, i] += 1.0                                                   # (c[i] of the unit vector e_n is 1 at n = i)
        if order >= 1:
            g[1] = (1.0 - alpha * alpha) * d[0] + alpha * d[1]
        for m in range(2, order + 1):
            g[m] = d[m - 1] + alpha * (d[m] - g[m - 1])
    return g


def _envelope_engine(device: torch.device, sr, n_fft: int, hop: int, order: int, alpha: float) -> Engine:
    return _cached_engine(device, ("envelope", float(sr), int(n_fft), int(hop), int(order), float(alpha)),
                          lambda eng: eng.load_envelope(stoi_twiddle(n_fft), hop, n_fft, float(sr),
                                                        freq_warp_matrix(n_fft // 2 + 1, order, alpha), 0.0, ENVELOPE_Q1))


def _device_envelope_rows(x, lengths, period, sr, n_fft, hop, order, alpha, want_envelope):
    return _envelope_engine(x.device, sr, n_fft, hop, order, alpha).envelope(x, lengths, period, ENVELOPE_POWER_FLOOR, want_envelope)


@torch.inference_mode()
def spectral_envelope(y, period, sr: int = 22050, n_fft: int = 1024, hop_length: int = 256, order: int = 24, alpha: float = 0.455, lengths=None,
                      envelope: bool = False, rows: Optional[Callable] = None):
    """The f0-adaptive spectral envelope and its mel-cepstrum per frame on the device (``ev_envelope``; no torch fallback): CheapTrick (Morise
    2015: a pitch-synchronous window of three periods, the DC correction, the smoothing over 2 f0 / 3 and the cepstral lifter that removes the
    harmonic structure) and SPTK's ``freqt`` at ``alpha``, both as defined in DESIGN section 3.29 and include/emojivoice.h (zero padding at the
    edges, no safeguard noise: deterministic; held to a numpy restatement, not to pyworld).  ``y`` 1-D, or (B, L) with ``lengths`` (B,) samples
    or None, on the GPU; ``period`` (F,) or (B, F): the period of every frame in samples, 0 where unvoiced (``sr / f0`` of ``pitch_yin`` at the
    same hop: frame f is its frame f); a frame without a period inside [2, (n_fft - 3) / 3] is analysed at sr / 500.  -> {"mcep" (B, F, order +
    1) float64: the mel-cepstrum of the log amplitude, coefficient 0 the level; "class" (B, F) int32: an index into ENVELOPE_CLASSES;
    "log_envelope" (B, F, n_fft / 2 + 1) float64 with ``envelope``: the log power envelope in nepers, else None}, F = ceil(L / hop_length).
    Silent frames and frames past a row are zeros."""
    if not torch.is_tensor(y) or y.dim() not in (1, 2) or y.numel() == 0:
        raise ValueError("spectral_envelope: y must be a non-empty tensor, 1-D or (B, L)")
    if not 0 <= int(order) <= 63 or not abs(float(alpha)) < 1.0 or int(order) > int(n_fft) // 2:
        raise ValueError(f"spectral_envelope: 0 <= order <= min(63, n_fft / 2) and |alpha| < 1 expected (got order={order} alpha={alpha})")
    if int(n_fft) % 2 or not 16 <= int(n_fft) <= 1024 or not 1 <= int(hop_length) <= 512:
        raise ValueError(f"spectral_envelope: n_fft even with 16 <= n_fft <= 1024 and 1 <= hop_length <= 512 expected (got {n_fft}, {hop_length})")
    if not 2.0 <= float(sr) / 500.0 <= (int(n_fft) - 3) / 3.0:
        raise ValueError(f"spectral_envelope: the default period sr / 500 = {float(sr) / 500.0:g} lies outside [2, (n_fft - 3) / 3] at sr={sr} n_fft={n_fft}")
    x = y.unsqueeze(0) if y.dim() == 1 else y
    F = -(-x.shape[1] // int(hop_length))
    pd = torch.as_tensor(period)
    pd = pd.unsqueeze(0) if pd.dim() == 1 else pd
    if tuple(pd.shape) != (x.shape[0], F):
        raise ValueError(f"spectral_envelope: period must be ({x.shape[0]}, {F}), got {tuple(pd.shape)}")
    if rows is None and not y.is_cuda:
        raise EvLibraryError("spectral_envelope runs on a ROCm GPU only (no CPU fallback): move y to the GPU")
    env, mcep, cls = (rows or _device_envelope_rows)(x, lengths if y.dim() == 2 else None, pd, sr, int(n_fft), int(hop_length), int(order),
                                                     float(alpha), bool(envelope))
    return {"mcep": mcep, "class": cls[:, :, 0], "log_envelope": env}


def period_from_pitch(pitch, sr) -> torch.Tensor:
    """(B, F) float32 periods in samples from a pitch tracker's dict ({"f0", "voiced"}): sr / f0 where voiced, else 0."""
    f0 = torch.as_tensor(pitch["f0"], dtype=torch.float32)
    v = torch.as_tensor(pitch["voiced"]).to(f0.device, torch.bool) & (f0 > 0)
    return torch.where(v, float(sr) / torch.where(v, f0, torch.ones_like(f0)), torch.zeros_like(f0))


@torch.inference_mode()
def envelope_cepstra(y, period, sr: int = 22050, n_fft: int = 1024, hop_length: int = 256, order: int = 24, alpha: float = 0.455, lengths=None,
                     rows: Optional[Callable] = None):
    """What ``envelope_mcd`` aligns, of one side: (coefficients 1 .. ``order`` of ``spectral_envelope``'s mel-cepstrum as (B, order, F) float32
    with the frames that are neither silent nor past the row moved to the front in their order, their count per row (B,) int32)."""
    if order < 1:
        raise ValueError(f"envelope_cepstra: order={order} must be at least 1 (coefficient 0, the level, is left out)")
    if not torch.is_tensor(y) or y.dim() != 2:
        raise ValueError("envelope_cepstra: y must be a (B, L) tensor")
    out = spectral_envelope(y, period, sr, n_fft, hop_length, order, alpha, lengths, rows=rows)
    keep = out["class"] < 2                                              # voiced or default period
    first = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)   # the kept frames first, in their order
    mc = torch.gather(out["mcep"], 1, first[:, :, None].expand(-1, -1, out["mcep"].shape[2]))[:, :, 1:]
    return mc.transpose(1, 2).to(torch.float32).contiguous(), keep.sum(dim=1).to(torch.int32)


@torch.inference_mode()
def cepstra_mcd(cep_a, n_a, cep_b, n_b):
    """MCD in dB, (B,) float64, between two sides of ``envelope_cepstra``: ``dtw`` over the Euclidean distance of the first n_a / n_b frames and
    ``mcd_from_cost``; NaN for a pair with no frame on a side."""
    if cep_a.shape[0] != cep_b.shape[0]:
        raise ValueError(f"cepstra_mcd: {cep_a.shape[0]} rows against {cep_b.shape[0]}")
    got = dtw(cep_a, cep_b, n_a.clamp_min(1), n_b.clamp_min(1), "euclidean")
    mcd = mcd_from_cost(got["cost"], got["steps"])
    both = ((n_a > 0) & (n_b > 0)).to(mcd.device)
    return torch.where(both, mcd, torch.full_like(mcd, float("nan")))


@torch.inference_mode()
def envelope_mcd(y_a, y_b, sr: int = 22050, len_a=None, len_b=None, pitch: Optional[Callable] = None, n_fft: int = 1024, hop_length: int = 256,
                 order: int = 24, alpha: float = 0.455, rows: Optional[Callable] = None):
    """Mel-cepstral distortion in dB between two batches of recordings (B, La) and (B, Lb) the way the TTS literature takes it, (B,) float64:
    ``pitch`` (a tracker such as ``pitch_yin`` or ``pitch_pyin``: ``pitch(y, sr, hop_length=..., lengths=...)`` -> {"f0", "voiced"}; None:
    ``pitch_yin``) gives the periods, ``spectral_envelope`` the mel-cepstra of CheapTrick's envelope, ``dtw`` aligns coefficients 1 .. ``order``
    (the level, coefficient 0, is left out) by their Euclidean distance and ``mcd_from_cost`` scales the mean over the path.  Silent frames
    and frames past a row are left out on both sides before the alignment: the frames kept move to the front and their count is the row's
    length, the way ``mel_cepstral_distortion`` takes ``len_a`` / ``len_b``.  NaN for a pair with no frame kept on a side.  The envelope is
    CheapTrick as DESIGN section 3.29 defines it (no pyworld): of the kind of the WORLD-based figures, not equal to them to the digit."""
    track = pitch_yin if pitch is None else pitch
    sides = []
    for y, ln in ((y_a, len_a), (y_b, len_b)):
        if not torch.is_tensor(y) or y.dim() != 2:
            raise ValueError("envelope_mcd: y_a and y_b must be (B, L) tensors")
        pd = period_from_pitch(track(y, sr, hop_length=hop_length, lengths=ln), sr)
        sides.append(envelope_cepstra(y, pd, sr, n_fft, hop_length, order, alpha, ln, rows))
    return cepstra_mcd(*sides[0], *sides[1])


@torch.inference_mode()
def f0_errors(f0_a, voiced_a, f0_b, voiced_b, path, steps):
    """Pitch agreement over a DTW path, per utterance: ``f0_a`` / ``voiced_a`` (B, Fa), ``f0_b`` / ``voiced_b`` (B, Fb), ``path``
    (B, P, 2) and ``steps`` (B,) as ``dtw`` returns them (row b uses its first steps[b] pairs (i, j): frame i of a against frame j of b).
    -> {"rmse_cents": list of B floats, the RMS of 1200 log2(f0_a[i] / f0_b[j]) over the pairs where both are voiced, None without such
    a pair; "voicing_error" (B,) float64: the share of pairs whose voicing flags differ (NaN for no pair); "voiced_pairs" (B,) int64;
    "sq_cents" (B,) float64: the sum of the squared cents, for pooling}.  Gathers and reductions in torch where ``f0_a`` lives, float64."""
    f0_a, f0_b = torch.as_tensor(f0_a).to(torch.float64), torch.as_tensor(f0_b).to(torch.float64)
    dev = f0_a.device
    f0_b = f0_b.to(dev)
    voiced_a, voiced_b = torch.as_tensor(voiced_a).to(dev, torch.bool), torch.as_tensor(voiced_b).to(dev, torch.bool)
    path, steps = torch.as_tensor(path).to(dev, torch.int64), torch.as_tensor(steps).to(dev, torch.int64)
    if f0_a.dim() == 1:
        f0_a, f0_b, voiced_a, voiced_b, path, steps = (f0_a[None], f0_b[None], voiced_a[None], voiced_b[None], path[None], steps.reshape(1))
    P = path.shape[1]
    valid = torch.arange(P, device=dev)[None, :] < steps[:, None]
    i, j = path[..., 0].clamp_min(0), path[..., 1].clamp_min(0)
    fa, fb = torch.gather(f0_a, 1, i), torch.gather(f0_b, 1, j)
    va, vb = torch.gather(voiced_a, 1, i) & valid, torch.gather(voiced_b, 1, j) & valid
    both = va & vb
    one = torch.ones_like(fa)
    cents = 1200.0 * torch.log2(torch.where(both, fa, one) / torch.where(both, fb, one))
    sq = (cents * cents).sum(dim=1)
    n_both = both.sum(dim=1)
    n = valid.sum(dim=1)
    verr = torch.where(n > 0, (va ^ vb).sum(dim=1).to(torch.float64) / n.clamp_min(1).to(torch.float64),
                       torch.full((n.numel(),), float("nan"), dtype=torch.float64, device=dev))
    rmse = [math.sqrt(s / c) if c > 0 else None for s, c in zip(sq.tolist(), n_both.tolist())]
    return {"rmse_cents": rmse, "voicing_error": verr, "voiced_pairs": n_both, "sq_cents": sq}


# ---- loudness: ITU-R BS.1770-4 / EBU R 128 -------------------------------------------------------------------------------------------------
LOUDNESS_OFFSET = -0.691                                       # LUFS = -0.691 + 10 log10(mean square of the K-weighted signal)
ABSOLUTE_GATE = 10.0 ** ((-70.0 - LOUDNESS_OFFSET) / 10.0)     # the -70 LUFS gate as a mean square


def k_weighting(sr: int) -> np.ndarray:
    """The K-weighting of BS.1770-4 at rate ``sr``: 10 float64 {b0, b1, b2, a1, a2} of the high shelf, then of the high pass (a0 = 1), the
    layout ``ev_loudness`` takes.  The standard tabulates the two biquads at 48 kHz only; they are the bilinear transforms of an analogue
    shelf (f0 1681.97 Hz, +4.00 dB, Q 0.7072) and an analogue high pass (f0 38.135 Hz, Q 0.5003), and this is that design at any rate:
    ``k_weighting(48000)`` equals the table to better than 1e-13.  ``sr`` must be a multiple of 10 (a 100 ms sub-block is a whole number of
    samples) and at least 8000 (the shelf's f0 must stay well below Nyquist)."""
    if int(sr) != sr or int(sr) % 10 or int(sr) < 8000:
        raise ValueError(f"k_weighting: sr must be a multiple of 10 and at least 8000 (got {sr})")
    sr = int(sr)
    f0, gain_db, q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    k = math.tan(math.pi * f0 / sr)
    vh = 10.0 ** (gain_db / 20.0)
    vb = vh ** 0.4996667741545416
    a0 = 1.0 + k / q + k * k
    shelf = [(vh + vb * k / q + k * k) / a0, 2.0 * (k * k - vh) / a0, (vh - vb * k / q + k * k) / a0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0]
    f0, q = 38.13547087602444, 0.5003270373238773
    k = math.tan(math.pi * f0 / sr)
    a0 = 1.0 + k / q + k * k
    return np.array(shelf + [1.0, -2.0, 1.0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0], dtype=np.float64)


def lufs(mean_square):
    """-0.691 + 10 log10(mean square) of a float64 tensor; -inf where it is not positive."""
    ms = torch.as_tensor(mean_square, dtype=torch.float64)
    return torch.where(ms > 0, LOUDNESS_OFFSET + 10.0 * torch.log10(ms.clamp_min(1e-300)), torch.full_like(ms, float("-inf")))


@torch.inference_mode()
def loudness(y, sr: int = 22050, lengths=None):
    """Integrated loudness by ITU-R BS.1770-4 on the device (``ev_loudness``; no torch fallback) of mono ``y``, 1-D or (B, L) with
    ``lengths`` (B,) samples or None, on the GPU: the signal through ``k_weighting(sr)``, mean squares over 400 ms blocks every 100 ms, the
    absolute gate at -70 LUFS and the relative gate 10 LU below the loudness of what passed it.  -> {"integrated" (B,) float64 LUFS, -inf
    where no block passes (silence, or a row under 400 ms); "momentary" (B, NB) float64: the LUFS of every block, -inf past a row's own blocks
    and for digital silence; "blocks" (B,) int32: the row's 400 ms blocks; "gated_blocks" (B,) int32: those that passed both gates;
    "sub_energy" (B, L // S) float64: the sum of squares of the K-weighted signal per 100 ms, S = sr / 10}; a 1-D input gives B = 1.  The
    incomplete last 100 ms of a row is discarded, as the standard says."""
    coef = k_weighting(sr)
    _trim_input(y, "loudness")
    x = y.unsqueeze(0) if y.dim() == 1 else y
    sub, block, gated, counts = _trim_engine(y.device).loudness(x, lengths if y.dim() == 2 else None, int(sr) // 10, coef, ABSOLUTE_GATE)
    return {"integrated": lufs(gated[:, 0]), "momentary": lufs(block), "blocks": counts[:, 0], "gated_blocks": counts[:, 2], "sub_energy": sub}


@torch.inference_mode()
def peak_level(y, lengths=None):
    """max |y| per row, (B,) float32 on the device (``ev_trim_bounds``' d_peak): ``y`` 1-D or (B, L) with ``lengths`` (B,) or None."""
    _trim_input(y, "peak_level")
    x = y.unsqueeze(0) if y.dim() == 1 else y
    _, pk = _trim_engine(y.device).trim_bounds(x, lengths if y.dim() == 2 else None)
    return pk


def loudness_gain(integrated, peak, target_lufs: float = -23.0, peak_ceiling: float = 0.95):
    """The gain that takes a row of loudness ``integrated`` (LUFS) and peak ``peak`` to ``target_lufs``: 10^((target - L) / 20), capped at
    peak_ceiling / peak so that the levelled peak stays at or under the ceiling (``peak_ceiling`` None or <= 0: no cap).  A row without a
    loudness (L = -inf) keeps gain 1.  -> (gain (B,) float64, gain_db (B,) float64, capped (B,) bool); torch ops where ``integrated`` lives."""
    loud = torch.as_tensor(integrated, dtype=torch.float64)
    pk = torch.as_tensor(peak).to(loud.device, torch.float64)
    measured = torch.isfinite(loud)
    gain = torch.where(measured, 10.0 ** ((float(target_lufs) - torch.where(measured, loud, torch.zeros_like(loud))) / 20.0), torch.ones_like(loud))
    capped = torch.zeros_like(measured)
    if peak_ceiling is not None and peak_ceiling > 0:
        limit = float(peak_ceiling) / pk.clamp_min(1e-300)
        capped = measured & (pk > 0) & (gain > limit)
        gain = torch.where(capped, limit, gain)
    return gain, 20.0 * torch.log10(gain), capped


@torch.inference_mode()
def loudness_normalize(y, target_lufs: float = -23.0, sr: int = 22050, lengths=None, peak_ceiling: float = 0.95):
    """Every row of ``y`` (1-D, or (B, L) with ``lengths`` (B,) or None, on the GPU) levelled to ``target_lufs`` integrated loudness
    (``loudness``), the gain capped where the row's peak (``ev_trim_bounds``' d_peak) would pass ``peak_ceiling`` (``loudness_gain``).  A row
    without a loudness (silence, under 400 ms) is left untouched.  -> (levelled rows, float32, zeros past a row's length; gain_db (B,)
    float64; capped (B,) bool).  The measurement runs in the HIP library; applying the gain is one torch multiply."""
    r = loudness(y, sr, lengths)
    x = y.unsqueeze(0) if y.dim() == 1 else y
    ln = lengths if y.dim() == 2 else None
    gain, gain_db, capped = loudness_gain(r["integrated"], peak_level(x, ln), target_lufs, peak_ceiling)
    out = x.to(torch.float32) * gain.to(torch.float32)[:, None]
    if ln is not None:
        n = torch.as_tensor(ln).to(x.device, torch.int64)
        out = out * (torch.arange(x.shape[1], device=x.device)[None, :] < n[:, None])
    return (out[0] if y.dim() == 1 else out), gain_db, capped


# ---- intelligibility: STOI (Taal, Hendriks, Heusdens, Jensen 2011) and ESTOI (Jensen, Taal 2016) ------------------------------------------------
STOI_SR = 10000                                    # the rate the measure is defined at
STOI_WINDOW, STOI_HOP, STOI_NFFT = 256, 128, 512   # 25.6 ms frames, 50 % overlap, zero-padded to 512
STOI_BANDS, STOI_MIN_FREQ = 15, 150.0              # one-third octave bands from 150 Hz
STOI_SEGMENT = 30                                  # frames per segment: 384 ms
STOI_SILENCE_RATIO = 10.0 ** (-40.0 / 10.0)        # frames 40 dB under the loudest clean frame are removed (a power ratio)
STOI_CLIP = 1.0 + 10.0 ** (15.0 / 20.0)            # the -15 dB signal-to-distortion bound of the clipping


def stoi_window(W: int) -> np.ndarray:
    """The analysis window of STOI: a Hann window of W + 2 points without its two zero end points, float64."""
    return np.hanning(int(W) + 2)[1:-1].astype(np.float64)


def stoi_twiddle(nfft: int) -> np.ndarray:
    """(nfft, 2) float64 {cos, sin}(2 pi n / nfft): the table ``ev_load_stoi`` takes."""
    a = 2.0 * np.pi * np.arange(int(nfft), dtype=np.float64) / int(nfft)
    return np.stack([np.cos(a), np.sin(a)], axis=1)


def third_octave_bands(fs: int = STOI_SR, nfft: int = STOI_NFFT, n_bands: int = STOI_BANDS, min_freq: float = STOI_MIN_FREQ) -> np.ndarray:
    """The one-third octave bands of STOI as (n_bands, 2) int32 {first bin, end bin (exclusive)} of an nfft-point DFT at rate fs: band k has
    the centre min_freq * 2^(k / 3) and the edges min_freq * 2^((2 k - 1) / 6) and min_freq * 2^((2 k + 1) / 6); each edge goes to the
    nearest point (argmin of the squared distance) of the grid linspace(0, fs, nfft + 1)[:nfft // 2 + 1]."""
    f = np.linspace(0.0, float(fs), int(nfft) + 1)[: int(nfft) // 2 + 1]
    k = np.arange(int(n_bands), dtype=np.float64)
    lo = float(min_freq) * 2.0 ** ((2.0 * k - 1.0) / 6.0)
    hi = float(min_freq) * 2.0 ** ((2.0 * k + 1.0) / 6.0)
    first = [int(np.argmin((f - v) ** 2)) for v in lo]
    end = [int(np.argmin((f - v) ** 2)) for v in hi]
    return np.array(list(zip(first, end)), dtype=np.int32).reshape(-1, 2)


def _stoi_engine(device: torch.device) -> Engine:
    return _cached_engine(device, ("stoi",), lambda eng: eng.load_stoi(stoi_window(STOI_WINDOW), stoi_twiddle(STOI_NFFT), third_octave_bands(),
                                                                      STOI_HOP, STOI_NFFT, STOI_SEGMENT))


def _aligned_pair(what: str, reference, degraded, lengths, on_device: bool):
    """The shared opening of ``stoi`` and ``stft_distance``: the checks of a sample-aligned pair, then both as (B, L) batches and the rows'
    lengths as int64 (B,) on the host, or None."""
    if not torch.is_tensor(reference) or not torch.is_tensor(degraded) or reference.dim() not in (1, 2) or reference.shape != degraded.shape:
        raise ValueError(f"{what}: reference and degraded must be tensors of one shape, 1-D or (B, L)")
    if reference.shape[-1] < 1:
        raise ValueError(f"{what}: the signals are empty")
    if on_device and not (reference.is_cuda and degraded.is_cuda):
        raise EvLibraryError(f"{what} runs on a ROCm GPU only (no CPU fallback): move the signals to the GPU")
    x = reference.unsqueeze(0) if reference.dim() == 1 else reference
    y = degraded.unsqueeze(0) if degraded.dim() == 1 else degraded
    ln = None
    if lengths is not None and reference.dim() == 2:
        ln = torch.as_tensor(lengths).to(torch.int64).reshape(-1).cpu()
        if ln.numel() != x.shape[0]:
            raise ValueError(f"{what}: {x.shape[0]} lengths expected, got {ln.numel()}")
    return x, y, ln


def _device_stoi_rows(x, y, lengths):
    keep, _, seg, score, counts = _stoi_engine(x.device).stoi(x, y, lengths, STOI_SILENCE_RATIO, STOI_CLIP)
    return keep, seg, score, counts


@torch.inference_mode()
def stoi(reference, degraded, sr: int = 22050, lengths=None, rows: Optional[Callable] = None):
    """STOI and ESTOI of ``degraded`` against the clean, SAMPLE-ALIGNED ``reference`` (copy synthesis against its recording), on the device
    (``ev_stoi``; no torch fallback): both 1-D or (B, L) at ``sr`` on the GPU, ``lengths`` (B,) samples per row or None.  Both signals go to
    10 kHz through ``resample`` (22050 -> 10000: up 200, down 441) unless ``sr`` is 10000; this project's Kaiser filter is a stated difference
    from the published implementation's resampler, so figures are comparable across this project's runs, not to the digit with other tools.
    Then 25.6 ms Hann frames at 50 % overlap, the frames 40 dB under the loudest clean frame removed from both, 15 one-third octave bands from
    150 Hz, segments of 30 frames.  -> {"stoi" (B,) float64, "estoi" (B,) float64, "segments" (B, NSEG, 2) float64: {STOI, ESTOI} of every
    segment, zeros past a row's own; "counts" (B, 3) int32: {frames, frames kept, segments}; "keep" (B, NF) uint8}; a 1-D input gives B = 1.
    A row without a segment (under about 0.4 s of signal after the silent frames are gone) gets NaN for both scores: the published
    implementation returns 1e-5 with a warning, but a number that looks like a score is not handed out for a signal too short to score.
    ``rows``: the per-batch measurement, (x, y, lengths) at 10 kHz -> (keep, segments, score (B, 2), counts) — the device call unless given."""
    if int(sr) != sr or int(sr) < 1:
        raise ValueError(f"stoi: sr must be a positive integer (got {sr})")
    x, y, ln = _aligned_pair("stoi", reference, degraded, lengths, rows is None)
    if int(sr) != STOI_SR:
        up, down = resample_ratio(int(sr), STOI_SR)
        x, y = resample(x, int(sr), STOI_SR, lengths=ln), resample(y, int(sr), STOI_SR, lengths=ln)
        if ln is not None:
            ln = torch.where((ln >= 1) & (ln <= reference.shape[-1]), -(-ln * up // down), torch.zeros_like(ln))
    keep, seg, score, counts = (rows or _device_stoi_rows)(x, y, ln)
    score = torch.as_tensor(score, dtype=torch.float64)
    scored = (torch.as_tensor(counts)[:, 2] > 0).to(score.device)
    nan = torch.full_like(score[:, 0], float("nan"))
    return {"stoi": torch.where(scored, score[:, 0], nan), "estoi": torch.where(scored, score[:, 1], nan), "segments": seg, "counts": counts, "keep": keep}


# ---- reverberation: the speech-to-reverberation modulation energy ratio (Falk, Zheng, Chan 2010) ----------------------------------------------------
SRMR_SR = 16000                                    # the rate the measure's tables are designed for
SRMR_EAR_Q, SRMR_MIN_BW = 9.26449, 24.7            # Glasberg and Moore's ERB scale
SRMR_GAMMATONE_ORDER = 4


def srmr_tables(sr: int = SRMR_SR, n_channels: int = 23, low_freq: float = 125.0, n_bands: int = 8, mod_lo: float = 4.0, mod_hi: float = 128.0,
                q: float = 2.0, frame_ms: float = 256, hop_ms: float = 64) -> Dict:
    """The tables ``ev_load_srmr`` takes, all float64, for rows at ``sr``:
      * "centres" (N,): ERB-spaced centre frequencies (Glasberg and Moore, EarQ = 9.26449, minBW = 24.7; Slaney's spacing) ascending from
        ``low_freq`` to below sr / 2; "erb" (N,) = centre / EarQ + minBW;
      * "chan" (N, 3) {Re a, Im a, gain}: Hohmann's (2002) complex pole a = lambda exp(2 pi i centre / sr), lambda = exp(-2 pi (erb / a_4) / sr),
        a_4 = pi 6! / (2^6 (3!)^2) the order-4 gammatone's bandwidth factor; gain = 2 (1 - |a|)^4;
      * "mod_centres" (K,): log-spaced from ``mod_lo`` to ``mod_hi``; "mod" (K, 5) {b0, b1, b2, a1, a2}: the second-order band pass with
        W0 = tan(pi f / sr), B0 = W0 / q: b = (B0, 0, -B0) / a0, a = (1 + B0 + W0^2, 2 W0^2 - 2, 1 - B0 + W0^2) / a0; "cutoff" (K,) =
        f - B0 sr / (2 pi), the lower band edges;
      * "window" (W,): the symmetric Hamming window of W = sr frame_ms / 1000 samples; "hop" H = sr hop_ms / 1000.
    The device wants W = 4 H and H a multiple of 64 between 64 and 1024, 1 <= N <= 32 and 1 <= K <= 8."""
    sr, N, K = int(sr), int(n_channels), int(n_bands)
    H, W = sr * hop_ms / 1000.0, sr * frame_ms / 1000.0
    if H != int(H) or W != int(W) or int(W) != 4 * int(H) or int(H) % 64 or not 64 <= int(H) <= 1024:
        raise ValueError(f"srmr_tables: hop {H:g} and frame {W:g} samples: the frame must be 4 hops and the hop a multiple of 64 with 64 <= hop <= 1024")
    if not 1 <= N <= 32 or not 1 <= K <= 8:
        raise ValueError(f"srmr_tables: n_channels={N} outside 1 .. 32 or n_bands={K} outside 1 .. 8")
    if not 0 < low_freq < sr / 2.0 or not 0 < mod_lo <= mod_hi < sr / 2.0 or not q > 0:
        raise ValueError(f"srmr_tables: 0 < low_freq < sr / 2, 0 < mod_lo <= mod_hi < sr / 2 and q > 0 expected (got {low_freq}, {mod_lo}, {mod_hi}, {q})")
    H, W = int(H), int(W)
    c = SRMR_EAR_Q * SRMR_MIN_BW
    i = np.arange(1, N + 1, dtype=np.float64)
    centres = (-c + np.exp(i * (np.log(low_freq + c) - np.log(sr / 2.0 + c)) / N) * (sr / 2.0 + c))[::-1].copy()
    erb = centres / SRMR_EAR_Q + SRMR_MIN_BW
    g = SRMR_GAMMATONE_ORDER
    a_g = math.pi * math.factorial(2 * g - 2) * 2.0 ** -(2 * g - 2) / math.factorial(g - 1) ** 2
    lam = np.exp(-2.0 * np.pi * (erb / a_g) / sr)
    beta = 2.0 * np.pi * centres / sr
    chan = np.stack([lam * np.cos(beta), lam * np.sin(beta), 2.0 * (1.0 - lam) ** 4], axis=1)
    mod_centres = mod_lo * (mod_hi / mod_lo) ** (np.arange(K, dtype=np.float64) / max(K - 1, 1))
    W0 = np.tan(np.pi * mod_centres / sr)
    B0 = W0 / q
    a0 = 1.0 + B0 + W0 ** 2
    mod = np.stack([B0 / a0, np.zeros(K), -B0 / a0, (2.0 * W0 ** 2 - 2.0) / a0, (1.0 - B0 + W0 ** 2) / a0], axis=1)
    cutoff = mod_centres - B0 * sr / (2.0 * np.pi)
    return {"sr": sr, "hop": H, "centres": centres, "erb": erb, "chan": np.ascontiguousarray(chan), "mod_centres": mod_centres,
            "mod": np.ascontiguousarray(mod), "cutoff": cutoff, "window": np.hamming(W).astype(np.float64)}


def _srmr_engine(device: torch.device) -> Engine:
    def load(eng):
        t = srmr_tables()
        eng.load_srmr(t["chan"], t["mod"], t["window"], t["erb"], t["cutoff"], t["hop"])
    return _cached_engine(device, ("srmr",), load)


def _device_srmr_rows(x, lengths, want_frame):
    return _srmr_engine(x.device).srmr(x, lengths, want_frame)


@torch.inference_mode()
def srmr(y, sr: int = 22050, lengths=None, rows: Optional[Callable] = None, energies: bool = False):
    """The speech-to-reverberation modulation energy ratio of ``y`` (1-D or (B, L) at ``sr`` on the GPU), on the device (``ev_srmr``; no torch
    fallback): NON-INTRUSIVE, no clean reference.  The rows go to 16 kHz through ``resample`` unless ``sr`` is 16000; then 23 gammatone channels
    from 125 Hz, their envelopes, 8 modulation bands from 4 to 128 Hz, 256 ms Hamming frames every 64 ms (``srmr_tables``).  A dry voice reads
    high, a reverberant one low.  The envelope comes from a complex gammatone (Hohmann 2002), a stated difference from SRMRpy: figures compare
    across this project's runs, not with other tools.  -> {"srmr" (B,) float64: NaN for a row without a frame (under 256 ms) or without energy
    in the high bands; "bw" (B,) float64: the bandwidth of the channel that closes 90 % of the energy; "k_star" (B,) int32: the bands counted;
    "frames" (B,) int32; "mean" (B, N, K) float64: the mean energy per (channel, band); with ``energies`` "energies" (B, NF, N, K) float64};
    a 1-D input gives B = 1.  ``rows``: the per-batch measurement, (x, lengths, want_frame) at 16 kHz -> (frame or None, mean, (B, 2) {ratio,
    bw}, counts (B, 3) {frames, j90, K*}) — the device call unless given."""
    if int(sr) != sr or int(sr) < 1:
        raise ValueError(f"srmr: sr must be a positive integer (got {sr})")
    if not torch.is_tensor(y) or y.dim() not in (1, 2) or y.shape[-1] < 1:
        raise ValueError("srmr: y must be a non-empty tensor, 1-D or (B, L)")
    if rows is None and not y.is_cuda:
        raise EvLibraryError("srmr runs on a ROCm GPU only (no CPU fallback): move y to the GPU")
    x = y.unsqueeze(0) if y.dim() == 1 else y
    ln = None
    if lengths is not None and y.dim() == 2:
        ln = torch.as_tensor(lengths).to(torch.int64).reshape(-1).cpu()
        if ln.numel() != x.shape[0]:
            raise ValueError(f"srmr: {x.shape[0]} lengths expected, got {ln.numel()}")
    if int(sr) != SRMR_SR:
        up, down = resample_ratio(int(sr), SRMR_SR)
        x = resample(x, int(sr), SRMR_SR, lengths=ln)
        if ln is not None:
            ln = torch.where((ln >= 1) & (ln <= y.shape[-1]), -(-ln * up // down), torch.zeros_like(ln))
    frame, mean, out, counts = (rows or _device_srmr_rows)(x, ln, bool(energies))
    out, counts = torch.as_tensor(out, dtype=torch.float64), torch.as_tensor(counts)
    scored = ((counts[:, 0] > 0).to(out.device)) & (out[:, 0] > 0)
    res = {"srmr": torch.where(scored, out[:, 0], torch.full_like(out[:, 0], float("nan"))), "bw": out[:, 1], "k_star": counts[:, 2],
           "frames": counts[:, 0], "mean": mean}
    if energies:
        res["energies"] = frame
    return res


# ---- speech rate and pauses: syllable nuclei (De Jong and Wempe 2009) --------------------------------------------------------------------------------
SPEECH_RATE_POWER_FLOOR = 1e-12                    # a frame at or under this power is silent whatever the row's level (digital silence)
SPEECH_RATE_MAX_FRAMES = 16384                     # ``ev_speech_rate``'s frame limit: 190 s at hop 256 and 22.05 kHz


def intensity_window(W: int) -> np.ndarray:
    """Praat's intensity window, ``np.kaiser(W, 20.24)`` in float64."""
    return np.kaiser(int(W), 20.24).astype(np.float64)


def speech_rate_geometry(sr, hop_length: int = 256, min_pitch: float = 50.0) -> Tuple[int, int]:
    """(W, H) of ``speech_rate``: the window of 3.2 / min_pitch seconds (Praat's intensity analysis) rounded to the nearest even number of
    samples, and the hop.  The device wants 8 <= W <= 4096 and H a multiple of 64 with 64 <= H <= 1024."""
    if not sr > 0 or not min_pitch > 0:
        raise ValueError(f"speech_rate_geometry: sr and min_pitch must be positive (got {sr}, {min_pitch})")
    W, H = 2 * int(round(3.2 / float(min_pitch) * float(sr) / 2.0)), int(hop_length)
    if not 8 <= W <= 4096:
        raise ValueError(f"speech_rate_geometry: the window of 3.2 / {min_pitch:g} s at {sr} Hz is {W} samples, outside 8 .. 4096")
    if H != hop_length or H % 64 or not 64 <= H <= 1024:
        raise ValueError(f"speech_rate_geometry: hop_length={hop_length} must be a multiple of 64 with 64 <= hop_length <= 1024")
    return W, H


def _speech_rate_engine(device: torch.device, W: int, H: int) -> Engine:
    return _cached_engine(device, ("speech_rate", W, H), lambda eng: eng.load_speech_rate(intensity_window(W), H))


def _device_speech_rate_rows(x, lengths, voiced, W, H, power_floor, rank_fraction, silence_ratio, dip_ratio, min_pause, min_sound):
    return _speech_rate_engine(x.device, W, H).speech_rate(x, lengths, voiced, power_floor, rank_fraction, silence_ratio, dip_ratio, min_pause,
                                                           min_sound)


@torch.inference_mode()
def speech_rate(y, sr: int = 22050, voiced=None, lengths=None, hop_length: int = 256, silence_db: float = 25.0, dip_db: float = 2.0,
                min_pause_s: float = 0.3, min_sound_s: float = 0.1, rank_fraction: float = 0.01, rows: Optional[Callable] = None):
    """How fast ``y`` (1-D or (B, L) at ``sr`` on the GPU) speaks and where it pauses, by De Jong and Wempe's (2009) syllable nuclei on the device
    (``ev_speech_rate``; no torch fallback), on ``pitch_yin``'s frames: the power under Praat's intensity window, frames more than ``silence_db``
    under the 99 % quantile (``rank_fraction``) silent, silences under ``min_pause_s`` filled and sounds under ``min_sound_s`` dropped, and as
    nuclei the local peaks of the power that are followed by a dip of ``dip_db`` and lie on a frame of ``voiced`` ((B, F) as ``pitch_yin``
    returns it; None: every frame).  The last peak counts, which the published script never does.  -> {"nuclei", "pauses", "frames" (B,) int32;
    "speech_rate" (nuclei per second of the row), "articulation_rate" (nuclei per sounding second), "phonation_ratio" (sounding over all
    frames), "pause_mean_s", "pause_sd_s" (B,) float64, a rate over zero seconds NaN; "intensity_db" (B, F) float64, 10 log10 of the power
    (-inf where it is 0); "mark" (B, F) uint8: 1 sounding, 2 raw, 4 candidate, 8 nucleus; "sounding", "leading", "trailing" (B,) int32 frames};
    a 1-D input gives B = 1.  ``rows``: the per-batch measurement, (x, lengths, voiced, W, H, power_floor, rank_fraction, silence_ratio,
    dip_ratio, min_pause, min_sound) -> (power (B, F), mark (B, F), stat (B, 4), count (B, 8)) — the device call unless given."""
    if not torch.is_tensor(y) or y.dim() not in (1, 2) or y.shape[-1] < 1:
        raise ValueError("speech_rate: y must be a non-empty tensor, 1-D or (B, L)")
    if rows is None and not y.is_cuda:
        raise EvLibraryError("speech_rate runs on a ROCm GPU only (no CPU fallback): move y to the GPU")
    if not silence_db > 0 or not dip_db >= 0 or not min_pause_s > 0 or not min_sound_s > 0 or not 0 <= rank_fraction < 1:
        raise ValueError(f"speech_rate: silence_db > 0, dip_db >= 0, min_pause_s > 0, min_sound_s > 0 and 0 <= rank_fraction < 1 expected (got "
                         f"{silence_db}, {dip_db}, {min_pause_s}, {min_sound_s}, {rank_fraction})")
    W, H = speech_rate_geometry(sr, hop_length)
    x = y.unsqueeze(0) if y.dim() == 1 else y
    F = -(-x.shape[1] // H)
    if F > SPEECH_RATE_MAX_FRAMES:
        raise ValueError(f"speech_rate: {F} frames over the limit of {SPEECH_RATE_MAX_FRAMES} ({SPEECH_RATE_MAX_FRAMES * H / float(sr):.0f} s)")
    ln = None
    if lengths is not None and y.dim() == 2:
        ln = torch.as_tensor(lengths).to(torch.int64).reshape(-1).cpu()
        if ln.numel() != x.shape[0]:
            raise ValueError(f"speech_rate: {x.shape[0]} lengths expected, got {ln.numel()}")
    if voiced is not None:
        voiced = torch.as_tensor(voiced)
        voiced = voiced.unsqueeze(0) if voiced.dim() == 1 else voiced
        if tuple(voiced.shape) != (x.shape[0], F):
            raise ValueError(f"speech_rate: voiced must be ({x.shape[0]}, {F}), got {tuple(voiced.shape)}")
    frame_s = H / float(sr)
    clamp = lambda s: min(max(int(round(s / frame_s)), 1), 4096)
    power, mark, stat, count = (rows or _device_speech_rate_rows)(x, ln, voiced, W, H, SPEECH_RATE_POWER_FLOOR, float(rank_fraction),
                                                                 10.0 ** (-float(silence_db) / 10.0), 10.0 ** (float(dip_db) / 10.0),
                                                                 clamp(min_pause_s), clamp(min_sound_s))
    power, stat, count = torch.as_tensor(power, dtype=torch.float64), torch.as_tensor(stat, dtype=torch.float64), torch.as_tensor(count)
    c = count.to(torch.float64).to(stat.device)
    nan = torch.full_like(c[:, 0], float("nan"))
    over = lambda a, b: torch.where(b > 0, a / torch.where(b > 0, b, torch.ones_like(b)), nan)
    return {"nuclei": count[:, 5], "pauses": count[:, 2], "frames": count[:, 0], "sounding": count[:, 1], "leading": count[:, 6],
            "trailing": count[:, 7], "speech_rate": over(c[:, 5], c[:, 0] * frame_s), "articulation_rate": over(c[:, 5], c[:, 1] * frame_s),
            "phonation_ratio": over(c[:, 1], c[:, 0]), "pause_mean_s": stat[:, 2] * frame_s, "pause_sd_s": stat[:, 3] * frame_s,
            "pause_s": c[:, 3] * frame_s, "intensity_db": 10.0 * torch.log10(power), "mark": torch.as_tensor(mark)}


def speech_rate_difference(a, b):
    """What ``speech_rate`` says of two renderings of the same text, row by row (b against a): {"rate_ratio": speech rate of b over a, minus 1
    (0.15: b is 15 % faster), "articulation_ratio": the same of the articulation rates, "pauses_delta": pauses of b minus a, "pause_s_delta":
    the time spent in pauses, b minus a, in seconds}; NaN where a rate of a is 0 or NaN."""
    ra, rb = torch.as_tensor(a["speech_rate"]), torch.as_tensor(b["speech_rate"]).to(torch.as_tensor(a["speech_rate"]).device)
    aa, ab = torch.as_tensor(a["articulation_rate"]), torch.as_tensor(b["articulation_rate"]).to(ra.device)
    nan = torch.full_like(ra, float("nan"))
    ratio = lambda p, q: torch.where(p > 0, q / torch.where(p > 0, p, torch.ones_like(p)) - 1.0, nan)
    return {"rate_ratio": ratio(ra, rb), "articulation_ratio": ratio(aa, ab),
            "pauses_delta": torch.as_tensor(b["pauses"]).cpu().to(torch.int64) - torch.as_tensor(a["pauses"]).cpu().to(torch.int64),
            "pause_s_delta": torch.as_tensor(b["pause_s"]).to(ra.device) - torch.as_tensor(a["pause_s"])}


# ---- spectral-magnitude distance: multi-resolution STFT (Yamamoto, Song, Kim 2020) and log-spectral distance ---------------------------------------
MSTFT_RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))   # (n_fft, hop, win): the published defaults
MSTFT_POWER_FLOOR = 1e-7                                                    # the clamp of |X|^2 before the root and the logarithm


def stft_dist_window(W: int) -> np.ndarray:
    """The periodic Hann window of W points, float64 (``torch.hann_window(W)``): 0.5 - 0.5 cos(2 pi n / W)."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(int(W), dtype=np.float64) / int(W))


def _stft_dist_engine(device: torch.device, resolution) -> Engine:
    nfft, hop, win = (int(v) for v in resolution)
    return _cached_engine(device, ("stft_dist", nfft, hop, win), lambda eng: eng.load_stft_dist(stft_dist_window(win), stoi_twiddle(nfft), hop, nfft))


def _device_stft_dist_rows(x, y, lengths, resolution):
    _, sums, counts = _stft_dist_engine(x.device, resolution).stft_dist(x, y, lengths, MSTFT_POWER_FLOOR)
    return sums, counts


@torch.inference_mode()
def stft_distance(reference, degraded, lengths=None, resolutions=MSTFT_RESOLUTIONS, rows: Optional[Callable] = None):
    """The multi-resolution STFT distance (spectral convergence + log-magnitude L1; Yamamoto et al. 2020, the "M-STFT" of BigVGAN) and the
    log-spectral distance of ``degraded`` against the SAMPLE-ALIGNED ``reference``, on the device (``ev_stft_dist``; no torch fallback): both
    1-D or (B, L) on the GPU at their own rate (nothing is resampled), ``lengths`` (B,) samples per row or None.  ``resolutions``: (n_fft,
    hop, win) triples; every one is ``torch.stft`` with a periodic Hann window, center=True and reflect padding, the power clamped at 1e-7,
    in float64.  Per resolution and row: sc = ||my - mx||_F / ||mx||_F, log_mag = mean |log my - log mx|, lsd_db = the mean over the frames
    of the RMS over the bins of the log-power difference in dB.  -> {"sc", "log_mag", "lsd_db": (B,) float64, the mean over the resolutions;
    "mstft" (B,) float64: the mean over the resolutions of sc + log_mag; "per_resolution": a list of {"n_fft", "hop", "win", "sc", "log_mag",
    "lsd_db"}; "frames" (B, R) int32}; a 1-D input gives B = 1.  A row without a frame at some resolution (not more than n_fft / 2 samples)
    gets NaN at that resolution and in every mean.  ``rows``: the per-resolution measurement, (x, y, lengths, resolution) -> (sums (B, 4),
    counts (B,)) in ev_stft_dist's terms — the device call unless given."""
    res = [tuple(int(v) for v in r) for r in resolutions]
    if not res or any(len(r) != 3 for r in res):
        raise ValueError("stft_distance: resolutions must be a non-empty list of (n_fft, hop, win)")
    x, y, ln = _aligned_pair("stft_distance", reference, degraded, lengths, rows is None)
    per, frames = [], []
    for nfft, hop, win in res:
        sums, counts = (rows or _device_stft_dist_rows)(x, y, ln, (nfft, hop, win))
        s = torch.as_tensor(sums, dtype=torch.float64)
        nf = torch.as_tensor(counts).to(s.device)
        has = nf > 0
        n = nf.clamp(min=1).to(torch.float64)
        nan = torch.full_like(s[:, 0], float("nan"))
        per.append({"n_fft": nfft, "hop": hop, "win": win,
                    "sc": torch.where(has, torch.sqrt(s[:, 0] / s[:, 1].clamp(min=1e-300)), nan),
                    "log_mag": torch.where(has, 0.5 * s[:, 2] / (n * (nfft // 2 + 1)), nan),
                    "lsd_db": torch.where(has, (10.0 / math.log(10.0)) * s[:, 3] / n, nan)})
        frames.append(nf.to(torch.int32))
    def mean(vals):                                                      # added in the order of ``resolutions``, element by element: a row's
        acc = vals[0]                                                    # figures do not depend on the batch it is measured in
        for v in vals[1:]:
            acc = acc + v
        return acc / float(len(vals))

    return {"sc": mean([p["sc"] for p in per]), "log_mag": mean([p["log_mag"] for p in per]), "lsd_db": mean([p["lsd_db"] for p in per]),
            "mstft": mean([p["sc"] + p["log_mag"] for p in per]), "per_resolution": per, "frames": torch.stack(frames, dim=1)}


VOICE_QUALITY_FIGURES = ("cpp_db", "alpha_ratio_db", "hammarberg_db", "slope_0_500", "slope_500_1500")
VOICE_QUALITY_BANDS_HZ = ((50, 1000), (1000, 5000), (0, 2000), (2000, 5000), (0, 500), (500, 1500))   # alpha lo / hi, Hammarberg lo / hi, slopes


def voice_quality_tables(sr: int, n_fft: int, fmin: float = 65.0, fmax: float = 600.0) -> Dict:
    """The host tables of ``ev_load_voice_quality`` at rate ``sr``: {"bands" (6, 2) int32: the bins [ceil(lo n_fft / sr), ceil(hi n_fft / sr)) of
    the alpha ratio's 50-1000 and 1000-5000 Hz, the Hammarberg index's 0-2000 and 2000-5000 Hz and the slopes' 0-500 and 500-1500 Hz;
    "slope_w" (2, n_fft / 2 + 1) float64: the centred least-squares slope weights of the two slope bands over x = bin frequency in kHz, zeros
    outside; "q_fit" = round(sr / 1000) (1 ms), "q_min" = ceil(sr / fmax), "q_max" = min(floor(sr / fmin), n_fft / 2): the quefrencies of the
    baseline fit and of the peak search, in samples; "fit_w" (q_max - q_fit + 1,) float64: the centred slope weights over q_fit .. q_max;
    "q_mean": their mean}."""
    sr, n_fft = int(sr), int(n_fft)
    if sr < 1 or n_fft < 16 or n_fft % 2:
        raise ValueError(f"voice_quality_tables: sr={sr} must be positive and n_fft={n_fft} even and at least 16")
    if not (0 < fmin <= fmax):
        raise ValueError(f"voice_quality_tables: 0 < fmin <= fmax expected (got fmin={fmin} fmax={fmax})")
    NB = n_fft // 2 + 1
    bands = np.array([[-(-(lo * n_fft) // sr), -(-(hi * n_fft) // sr)] for lo, hi in VOICE_QUALITY_BANDS_HZ], dtype=np.int32)
    if int(bands.max()) > NB or bool((bands[:, 1] <= bands[:, 0]).any()) or bool((bands[4:, 1] - bands[4:, 0] < 2).any()):
        raise ValueError(f"voice_quality_tables: sr={sr} with n_fft={n_fft} leaves a band empty, a slope band under 2 bins or a band past the "
                         f"Nyquist bin (bins {bands.tolist()} of {NB})")
    slope_w = np.zeros((2, NB), dtype=np.float64)
    for b in range(2):
        lo, hi = int(bands[4 + b, 0]), int(bands[4 + b, 1])
        x = np.arange(lo, hi, dtype=np.float64) * sr / n_fft / 1000.0
        d = x - x.mean()
        slope_w[b, lo:hi] = d / np.sum(d * d)
    q_fit, q_min, q_max = int(round(sr / 1000.0)), int(math.ceil(sr / fmax)), min(int(math.floor(sr / fmin)), n_fft // 2)
    if not (1 <= q_fit <= q_min <= q_max) or q_max - q_fit + 1 < 2:
        raise ValueError(f"voice_quality_tables: sr={sr} n_fft={n_fft} fmin={fmin} fmax={fmax} give q_fit={q_fit} q_min={q_min} q_max={q_max}, "
                         "outside 1 <= q_fit <= q_min <= q_max")
    q = np.arange(q_fit, q_max + 1, dtype=np.float64)
    d = q - q.mean()
    return {"bands": bands, "slope_w": slope_w, "q_fit": q_fit, "q_min": q_min, "q_max": q_max, "fit_w": d / np.sum(d * d), "q_mean": float(q.mean())}


def _voice_quality_engine(device: torch.device, sr: int, n_fft: int, hop: int, fmin: float, fmax: float) -> Engine:
    def load(eng):
        t = voice_quality_tables(sr, n_fft, fmin, fmax)
        eng.load_voice_quality(stft_dist_window(n_fft), stoi_twiddle(n_fft), hop, n_fft, t["bands"], t["slope_w"], t["q_fit"], t["q_min"], t["q_max"],
                               t["fit_w"], t["q_mean"])
    return _cached_engine(device, ("voice_quality", int(sr), int(n_fft), int(hop), float(fmin), float(fmax)), load)


@torch.inference_mode()
def voice_quality(y, sr: int = 22050, fmin: float = 65.0, fmax: float = 600.0, frame_length: int = 1024, hop_length: int = 256, lengths=None,
                  power_floor: float = 1e-7):
    """Voice quality per frame on the device (``ev_voice_quality``; no torch fallback): from the float64 log-power spectrum of every frame
    (periodic Hann window of ``frame_length`` = n_fft points, zeros outside the row, the power clamped at ``power_floor``) the alpha ratio
    (1-5 kHz over 50-1000 Hz), the Hammarberg index (strongest bin of 0-2 kHz over that of 2-5 kHz), the least-squares spectral slopes of
    0-500 Hz and 500-1500 Hz in dB per kHz (eGeMAPS; Eyben et al. 2016), and from its cepstrum the cepstral peak prominence (Hillenbrand et
    al. 1994): the cepstral peak between sr / fmax and sr / fmin over the least-squares line through the cepstrum from 1 ms on, at the peak.
    Frame f is ``pitch_yin``'s frame f at the same hop.  ``y`` 1-D, or (B, L) with ``lengths`` (B,) samples or None, on the GPU ->
    {"cpp_db", "alpha_ratio_db", "hammarberg_db", "slope_0_500", "slope_500_1500", "power": (B, F) float64; "peak_quefrency" (B, F) int32:
    q* in samples; "cepstral_f0" (B, F) float32: sr / q*}, F = ceil(L / hop_length); a 1-D input gives B = 1.  A silent frame (no bin above
    the floor) and a frame past a row's ceil(len / hop_length) have zeros everywhere but a silent frame's power.  The cepstrum is the linear
    real cepstrum of the dB spectrum: the figures are comparable across runs of this project (a recording against its synthesis, voice by
    voice); Praat and Hillenbrand put the cepstral magnitude in dB as well and VoiceSauce analyses pitch-synchronous windows, so they are not
    comparable to the digit with those tools."""
    _trim_input(y, "voice_quality")
    eng = _voice_quality_engine(y.device, sr, frame_length, hop_length, fmin, fmax)
    x = y.unsqueeze(0) if y.dim() == 1 else y
    frame, peak, _ = eng.voice_quality(x, lengths if y.dim() == 2 else None, power_floor)
    has = peak > 0
    out = {k: frame[:, :, i] for i, k in enumerate(VOICE_QUALITY_FIGURES + ("power",))}
    out["peak_quefrency"] = peak
    out["cepstral_f0"] = torch.where(has, float(sr) / peak.clamp(min=1).to(torch.float64), torch.zeros_like(peak, dtype=torch.float64)).to(torch.float32)
    return out


# The five figure families of the voice report (voice quality, formants, perturbation, harmonics, auditory), each described once and shared by its
# ``*_statistics`` function and ``voice_functionals``: ``_coerced`` brings what a family reads of its analysis function's dict to one device,
# ``_inside`` gives the rows their batch axis and their lengths, a ``_*_contours`` function turns the tensors and the base mask ``use`` (voiced
# and inside the row; for the auditory family, which is not a matter of the voiced frames alone, inside the row) into (the family's frames mask, {figure: (values (B, F) float64, the frames behind the figure (B, F) bool)}) in the order
# of the family's ``*_FIGURES``, and ``_reduce`` sums every contour under its mask.
def _coerced(d, lead: str, f64=(), dev=None, voiced=None):
    """{``lead``: d[lead] as it is, every key of ``f64`` as float64, "voiced": ``voiced`` as bool when given}, where d[lead] lives (``dev``:
    there instead).  The first entry leads: its first two axes are (B, F)."""
    first = torch.as_tensor(d[lead])
    dev = first.device if dev is None else dev
    t = {lead: first.to(dev), **{k: torch.as_tensor(d[k], dtype=torch.float64).to(dev) for k in f64}}
    if voiced is not None:
        t["voiced"] = torch.as_tensor(voiced, dtype=torch.bool, device=dev)
    return t


def _inside(t, n_frames, who: str, one: bool = False, shapes=None):
    """The rows of ``t`` ({name: tensor or None}, the first entry leading): a single row (``one``) gains the batch axis in every entry,
    ``shapes(t, B, F)`` says what is wrong with the shapes (None: nothing) -> (t, (B, F) bool: frame f lies inside row b's ``n_frames`` (None:
    every frame), the lengths as int64 (B,))."""
    if one:
        t = {k: None if v is None else v.unsqueeze(0) for k, v in t.items()}
    lead = next(iter(t.values()))
    B, F = lead.shape[:2]
    wrong = shapes(t, B, F) if shapes is not None else None
    if wrong:
        raise ValueError(f"{who}: {wrong}")
    n = torch.full((B,), F, dtype=torch.int64, device=lead.device) if n_frames is None else torch.as_tensor(n_frames).to(lead.device, torch.int64)
    if n.numel() != B:
        raise ValueError(f"{who}: {B} lengths expected, got {n.numel()}")
    return t, torch.arange(F, device=lead.device)[None, :] < n[:, None], n


def _voice_quality_contours(t, use):
    """The voiced frames that are not silent, behind every figure."""
    use = use & (t["peak_quefrency"] > 0)
    return use, {k: (t[k], use) for k in VOICE_QUALITY_FIGURES}


def _formant_contours(t, use, max_bandwidth: float):
    """The voiced frames with at least three formants; behind F_i and its bandwidth those of them whose F_i is at most ``max_bandwidth`` wide."""
    use = use & (t["count"] >= 3)
    oks = [use & (t["bandwidth"][:, :, i] <= float(max_bandwidth)) for i in range(3)]
    return use, {f"{q}{i + 1}_hz": (t[key][:, :, i], oks[i]) for q, key in (("f", "frequency"), ("b", "bandwidth")) for i in range(3)}


_PERTURBATION_READ = ("jitter", "rap", "shimmer", "shimmer_db", "r")       # what the report's figures are made of


def _perturbation_contours(t, use):
    """``use`` itself; behind a figure (in the report's units: per cent, dB, ``hnr_db``(r)) the frames with a counted pair of its kind (period
    pairs, triples, amplitude pairs; hnr_db: every frame of ``use``)."""
    pairs, amps, triples = use & (t["count"][..., 1] > 0), use & (t["count"][..., 2] > 0), use & (t["count"][..., 3] > 0)
    return use, {"jitter_pct": (100.0 * t["jitter"], pairs), "rap_pct": (100.0 * t["rap"], triples), "shimmer_pct": (100.0 * t["shimmer"], amps),
                 "shimmer_db": (t["shimmer_db"], amps), "hnr_db": (hnr_db(t["r"]), use)}


def _harmonic_contours(t, use, band, max_bandwidth: float):
    """``use`` itself; behind a figure the frames that carry its flag and, with ``band`` (B, F, n >= 3), whose formant is at most
    ``max_bandwidth`` wide."""
    out = {}
    for name in HARMONIC_FIGURES:
        ok = use & ((t["flags"] & _HARMONIC_FLAG[name]) != 0)
        if band is not None and name in _HARMONIC_FORMANT:
            ok = ok & (band[:, :, _HARMONIC_FORMANT[name]] <= float(max_bandwidth))
        out[name] = (t[name], ok)
    return use, out


def _reduce(frames, contours):
    """{"frames" (B,) int64: the frames of the mask ``frames``; "used", "sums", "means": {figure: (B,)}: the frames behind each contour, its sum
    over them and sum / frames, NaN without a frame}.  Contours that share a mask share its count."""
    counts = {id(frames): frames.sum(dim=1)}
    out = {"frames": counts[id(frames)], "used": {}, "sums": {}, "means": {}}
    for name, (v, ok) in contours.items():
        if id(ok) not in counts:
            counts[id(ok)] = ok.sum(dim=1)
        k = counts[id(ok)]
        s = torch.where(ok, v, torch.zeros_like(v)).sum(dim=1)
        out["used"][name], out["sums"][name] = k, s
        out["means"][name] = torch.where(k > 0, s / k.clamp(min=1).to(torch.float64), torch.full_like(s, float("nan")))
    return out


@torch.inference_mode()
def voice_quality_statistics(vq, voiced, lengths=None):
    """Per utterance, from ``voice_quality`` and a voicing mask at the same hop (``pitch_yin`` / ``pitch_pyin``): {"cpp_db", "alpha_ratio_db",
    "hammarberg_db", "slope_0_500", "slope_500_1500": (B,) float64, the mean over the frames that are voiced and not silent
    (``peak_quefrency`` > 0), NaN where no frame qualifies; "frames" (B,) int64: how many did; "sums": the same five keys, (B,) float64 sums
    over those frames, for pooling over utterances}, where ``vq`` lives (torch ops only).  Entries are (B, F) or 1-D; ``lengths`` (B,): the
    FRAMES that belong to each row (None: F)."""
    t = _coerced(vq, "peak_quefrency", VOICE_QUALITY_FIGURES, voiced=voiced)

    def shapes(t, B, F):
        if t["voiced"].shape != t["peak_quefrency"].shape:
            return f"the mask {tuple(t['voiced'].shape)} does not match the figures {tuple(t['peak_quefrency'].shape)}"

    t, inside, _ = _inside(t, lengths, "voice_quality_statistics", t["peak_quefrency"].dim() == 1, shapes)
    r = _reduce(*_voice_quality_contours(t, t["voiced"] & inside))
    return {"frames": r["frames"], "sums": r["sums"], **r["means"]}


FORMANT_POWER_FLOOR = 1e-10                        # frames whose windowed, pre-emphasised energy is at or under it are silent: no formants


def formant_window(W: int) -> np.ndarray:
    """Praat's Gaussian analysis window over ``W`` points, float64: (exp(-48 ((j + 0.5) / W - 0.5)^2) - e^-12) / (1 - e^-12)."""
    j = np.arange(int(W), dtype=np.float64)
    e = np.exp(-12.0)
    return (np.exp(-48.0 * ((j + 0.5) / int(W) - 0.5) ** 2) - e) / (1.0 - e)


def formant_geometry(sr: int = 22050, max_formant: float = 5500.0, order: Optional[int] = None, frame_length: int = 1024, hop_length: int = 256) -> Dict:
    """What ``formants`` analyses at: {"d": the integer decimation max(1, floor(sr / (2 max_formant))), "sr": the rate sr / d, "W" =
    frame_length / d, "H" = hop_length / d, "pre" = exp(-2 pi 50 d / sr) (pre-emphasis from 50 Hz), "order" (2 + round(sr / d / 1000) when
    None)}.  ``frame_length`` and ``hop_length`` must be multiples of d (ValueError): then ceil(ceil(L / d) / H) = ceil(L / hop_length) and the
    frames line up one to one with ``pitch_yin``'s and ``voice_quality``'s at the same hop."""
    if not (sr > 0 and max_formant > 0):
        raise ValueError(f"formants: sr={sr} and max_formant={max_formant} must be positive")
    d = max(1, int(math.floor(sr / (2.0 * max_formant))))
    if int(frame_length) % d or int(hop_length) % d or int(hop_length) < d:
        raise ValueError(f"formants: frame_length={frame_length} and hop_length={hop_length} must be multiples of the decimation {d} "
                         f"(sr={sr}, max_formant={max_formant})")
    rate = float(sr) / d
    return {"d": d, "sr": rate, "W": int(frame_length) // d, "H": int(hop_length) // d, "pre": math.exp(-2.0 * math.pi * 50.0 * d / float(sr)),
            "order": 2 + int(round(rate / 1000.0)) if order is None else int(order)}


def _formant_engine(device: torch.device, rate: float, W: int, H: int, order: int, n_formants: int, f_lo: float, pre: float) -> Engine:
    return _cached_engine(device, ("formants", float(rate), int(W), int(H), int(order), int(n_formants), float(f_lo)),
                          lambda eng: eng.load_formants(formant_window(W), H, order, pre, rate, f_lo, n_formants))


@torch.inference_mode()
def formants(y, sr: int = 22050, max_formant: float = 5500.0, n_formants: int = 4, order: Optional[int] = None, frame_length: int = 1024,
             hop_length: int = 256, f_lo: float = 50.0, lengths=None, power_floor: float = FORMANT_POWER_FLOOR):
    """Formants per frame on the device (``ev_formants``; no torch fallback), the way Praat's Burg analysis finds them: the rows are decimated
    by the integer d = max(1, floor(sr / (2 max_formant))) through ``resample`` (22050 -> 11025 Hz for 5500 Hz), every frame is pre-emphasised
    from 50 Hz, weighted by ``formant_window`` (frame_length / d points), predicted linearly by Burg's lattice at ``order`` (2 + round(sr / d /
    1000) when None: 13 at 11025 Hz), and the roots of the prediction polynomial inside f_lo < f < sr / (2 d) - f_lo are the candidates; the
    ``n_formants`` of lowest frequency are kept, in ascending order.  Frame f is ``pitch_yin``'s and ``voice_quality``'s frame f at the same
    hop.  No tracking across frames.  ``y`` 1-D, or (B, L) with ``lengths`` (B,) samples or None, on the GPU -> {"frequency", "bandwidth"
    (B, F, n_formants) float64 Hz, zeros past "count"; "count" (B, F) int32: the formants found (0 on a silent frame and past a row's frames,
    -1 where the root finder did not converge); "gain" (B, F) float64: the prediction error power per sample; "lpc" (B, F, order) float64:
    a_1 .. a_p}, F = ceil(L / hop_length); a 1-D input gives B = 1."""
    _trim_input(y, "formants")
    g = formant_geometry(sr, max_formant, order, frame_length, hop_length)
    x = y.unsqueeze(0) if y.dim() == 1 else y
    ln = lengths if y.dim() == 2 else None
    d = g["d"]
    if d > 1:
        x = resample(x.float(), d, 1, ln)
        if ln is not None:
            ln = -(-torch.as_tensor(ln).to(torch.int64) // d)
    eng = _formant_engine(y.device, g["sr"], g["W"], g["H"], g["order"], n_formants, f_lo, g["pre"])
    lpc, fm, count = eng.formants(x, ln, power_floor)
    p = g["order"]
    return {"frequency": fm[..., 0], "bandwidth": fm[..., 1], "count": count, "gain": lpc[..., p], "lpc": lpc[..., :p]}


@torch.inference_mode()
def formant_statistics(fm, voiced, lengths=None, max_bandwidth: float = 700.0):
    """Per utterance, from ``formants`` and a voicing mask at the same hop (``pitch_yin`` / ``pitch_pyin``): {"f1_hz", "f2_hz", "f3_hz",
    "b1_hz", "b2_hz", "b3_hz": (B,) float64, the means of F_i and of its bandwidth over the frames that are voiced, lie inside ``lengths`` and
    have count >= 3, leaving out for that i the frames whose F_i has a bandwidth over ``max_bandwidth``; NaN where no frame qualifies; "frames"
    (B,) int64: the voiced frames with count >= 3; "unconverged_frames" (B,) int64: the frames inside ``lengths`` with count -1; "used" (B, 3)
    int64: the frames behind each i's means; "sums": the six keys, (B,) float64 sums over those frames, for pooling over utterances}, where
    ``fm`` lives (torch ops only).  Entries are (B, F, n) / (B, F) or one row without the leading axis; ``lengths`` (B,): the FRAMES that
    belong to each row (None: F)."""
    t = _coerced(fm, "count", ("frequency", "bandwidth"), voiced=voiced)

    def shapes(t, B, F):
        count, freq, band = t["count"], t["frequency"], t["bandwidth"]
        if t["voiced"].shape != count.shape:
            return f"the mask {tuple(t['voiced'].shape)} does not match the figures {tuple(count.shape)}"
        if freq.shape[:2] != count.shape or freq.shape != band.shape or freq.shape[2] < 3:
            return f"frequency and bandwidth must be ({B}, {F}, n >= 3), got {tuple(freq.shape)} and {tuple(band.shape)}"

    t, inside, _ = _inside(t, lengths, "formant_statistics", t["count"].dim() == 1, shapes)
    r = _reduce(*_formant_contours(t, t["voiced"] & inside, max_bandwidth))
    out = {"frames": r["frames"], "unconverged_frames": (inside & (t["count"] < 0)).sum(dim=1), "sums": {}}
    for name in (f"{q}{i + 1}_hz" for i in range(3) for q in "fb"):
        out["sums"][name], out[name] = r["sums"][name], r["means"][name]
    out["used"] = torch.stack([r["used"][f"f{i + 1}_hz"] for i in range(3)], dim=1)
    return out


FORMANT_FIGURES = ("f1_hz", "f2_hz", "f3_hz", "b1_hz", "b2_hz", "b3_hz")

FORMANT_TRACK_REFERENCE = (550.0, 1650.0, 2750.0)  # Hz: the resonances of a neutral vocal tract of 17.5 cm, Praat's defaults for F1 .. F3
FORMANT_TRACK_MAX_STATES = 1024                    # ``ev_formant_track``'s limit on S = C(n_cand, n_tracks)


def formant_track_arguments(fm, n_tracks: int = 3, reference=FORMANT_TRACK_REFERENCE, frequency_cost: float = 1.0, bandwidth_cost: float = 1.0,
                            transition_cost: float = 1.0) -> Dict:
    """``formant_tracks``' checks, on the host and before any device is touched (ValueError): ``fm`` holds "frequency" and "bandwidth" (B, F,
    n_cand) or one row (F, n_cand) and "count" (B, F) or (F,) with F >= 1 and 1 <= n_cand <= 16; 1 <= n_tracks <= n_cand; ``reference`` holds
    n_tracks finite frequencies greater than 0; the three costs are finite and at least 0; S = C(n_cand, n_tracks) <= 1024 -> {"one": a single
    row, "n_cand", "n_tracks", "S", "reference": (n_tracks,) float64}."""
    who = "formant_tracks"
    if not isinstance(fm, dict) or any(k not in fm for k in ("frequency", "bandwidth", "count")):
        raise ValueError(f"{who}: fm must be the dict of formants (frequency, bandwidth, count)")
    freq, band, count = (torch.as_tensor(fm[k]) for k in ("frequency", "bandwidth", "count"))
    if freq.dim() not in (2, 3) or freq.shape != band.shape or tuple(count.shape) != tuple(freq.shape[:-1]):
        raise ValueError(f"{who}: frequency and bandwidth must be (B, F, n_cand) or (F, n_cand) and count (B, F) or (F,), got {tuple(freq.shape)}, "
                         f"{tuple(band.shape)} and {tuple(count.shape)}")
    F, nc = int(freq.shape[-2]), int(freq.shape[-1])
    if F < 1:
        raise ValueError(f"{who}: no frames")
    if not 1 <= nc <= 16:
        raise ValueError(f"{who}: n_cand={nc} outside 1 <= n_cand <= 16")
    if isinstance(n_tracks, bool) or int(n_tracks) != n_tracks or not 1 <= int(n_tracks) <= nc:
        raise ValueError(f"{who}: n_tracks={n_tracks} outside 1 <= n_tracks <= n_cand = {nc}")
    nt = int(n_tracks)
    ref = np.asarray(reference, dtype=np.float64).reshape(-1)
    if ref.size != nt:
        raise ValueError(f"{who}: reference must hold n_tracks = {nt} frequencies, got {ref.size}")
    if not (np.isfinite(ref) & (ref > 0)).all():
        raise ValueError(f"{who}: reference={ref.tolist()} must be finite and greater than 0")
    for name, v in (("frequency_cost", frequency_cost), ("bandwidth_cost", bandwidth_cost), ("transition_cost", transition_cost)):
        if not (math.isfinite(float(v)) and float(v) >= 0.0):
            raise ValueError(f"{who}: {name}={v} must be finite and at least 0")
    S = math.comb(nc, nt)
    if S > FORMANT_TRACK_MAX_STATES:
        raise ValueError(f"{who}: S={S} states = C(n_cand={nc}, n_tracks={nt}) over the limit S <= {FORMANT_TRACK_MAX_STATES}")
    return {"one": freq.dim() == 2, "n_cand": nc, "n_tracks": nt, "S": S, "reference": ref}


def formant_track_states(n_cand: int, n_tracks: int) -> np.ndarray:
    """(S, n_tracks) int64: the states of ``ev_formant_track`` in their numbering, the strictly increasing index tuples over 0 .. n_cand - 1 in
    lexicographic order."""
    return np.array(list(itertools.combinations(range(int(n_cand)), int(n_tracks))), dtype=np.int64).reshape(-1, int(n_tracks))


@torch.inference_mode()
def formant_tracks(fm, n_tracks: int = 3, reference=FORMANT_TRACK_REFERENCE, frequency_cost: float = 1.0, bandwidth_cost: float = 1.0,
                   transition_cost: float = 1.0):
    """Formant tracks through the candidates of ``formants`` on the device (``ev_formant_track``; no torch fallback; Praat's Formant: Track is
    the model): per row a Viterbi pass over the ways of mapping ``n_tracks`` tracks, which do not cross, onto each frame's candidates.  A
    mapping costs, per track k, frequency_cost |f - reference[k]| / 1000 + bandwidth_cost bw / f in its frame and transition_cost |log2 f -
    log2 f'| against the frame before.  A frame with fewer than ``n_tracks`` candidates (silent, unconverged, past the row) is a gap; the runs
    of frames between gaps are segments, each decoded on its own.  Ask ``formants`` for more candidates than tracks (n_formants=5 for three
    tracks), so that a spurious candidate can be left out.  ``fm``: the dict of ``formants``, on the GPU -> {"frequency", "bandwidth" (B, F,
    n_tracks) float64: the chosen candidates, zeros on gaps; "count" (B, F) int32: n_tracks on tracked frames, 0 on gaps, -1 where the input
    was -1; "selection" (B, F, n_tracks) int64: the chosen candidates' indices, -1 on gaps; "cost" (B, F) float64: each segment's optimum at
    its last frame, 0 elsewhere; "segments" (B,) int64}: the same contract as ``formants``', so the result goes wherever its dict goes
    (``formant_statistics``, ``harmonics``, ``harmonic_statistics``, ``voice_functionals``).  A single row (F, n_cand) gives B = 1."""
    a = formant_track_arguments(fm, n_tracks, reference, frequency_cost, bandwidth_cost, transition_cost)
    freq, band, count = (torch.as_tensor(fm[k]) for k in ("frequency", "bandwidth", "count"))
    if not (freq.is_cuda and band.device == freq.device and count.device == freq.device):
        raise EvLibraryError("formant_tracks runs on a ROCm GPU only (no CPU fallback): its input is the dict formants returned")
    if a["one"]:
        freq, band, count = freq.unsqueeze(0), band.unsqueeze(0), count.unsqueeze(0)
    cand = torch.stack((freq.to(torch.float64), band.to(torch.float64)), dim=-1).contiguous()
    count = count.to(torch.int32).contiguous()
    eng = _cached_engine(freq.device, ("formant_track",))
    track, sel, cost = eng.formant_track(cand, count, a["n_tracks"], a["reference"], frequency_cost, bandwidth_cost, transition_cost)
    tracked = sel >= 0
    table = torch.from_numpy(formant_track_states(a["n_cand"], a["n_tracks"])).to(freq.device)
    selection = torch.where(tracked[..., None], table[sel.clamp(min=0).to(torch.int64)], torch.full_like(table[:1], -1))
    after = torch.cat((tracked[:, 1:], torch.zeros_like(tracked[:, :1])), dim=1)
    out_count = torch.where(tracked, torch.full_like(count, a["n_tracks"]), torch.where(count < 0, torch.full_like(count, -1), torch.zeros_like(count)))
    return {"frequency": track[..., 0], "bandwidth": track[..., 1], "count": out_count, "selection": selection, "cost": cost,
            "segments": (tracked & ~after).sum(dim=1)}


PERTURBATION_POWER_FLOOR = 1e-10                   # a correlation whose energies' product is at or under its square gives r = 0
PERTURBATION_FIGURES = ("jitter_pct", "rap_pct", "shimmer_pct", "shimmer_db", "hnr_db")
_PERTURBATION_FRAME = ("jitter", "jitter_abs", "shimmer", "shimmer_db", "r", "period", "amplitude", "rap")


@torch.inference_mode()
def perturbation(y, sr: int = 22050, fmin: float = 65.0, fmax: float = 600.0, frame_length: int = 1024, hop_length: int = 256, lengths=None,
                 lag=None, n_cycles: int = 3, period_factor: float = 1.3, amplitude_factor: float = 1.6,
                 power_floor: float = PERTURBATION_POWER_FLOOR):
    """Jitter, shimmer and the harmonic strength per frame on the device (``ev_perturbation``; no torch fallback; Praat's voice report is the
    model): around the centre of every voiced frame up to ``n_cycles`` pitch marks on each side are picked as waveform peaks one YIN lag apart
    (within an eighth of it) and refined by a parabola; the periods between them and their amplitudes give the cycle-to-cycle figures, the
    normalised cross-correlation over ``frame_length`` samples at the lag gives r.  ``lag`` (B, F) int32: the lags of ``Engine.pitch_yin`` at the
    same hop; None runs YIN on the device (fmin, fmax, frame_length).  ``y`` 1-D, or (B, L) with ``lengths`` (B,) samples or None, on the GPU ->
    {"jitter" (local, a ratio), "jitter_abs" (samples), "shimmer" (local, a ratio), "shimmer_db", "r", "period" (the mean, samples), "amplitude"
    (the mean), "rap": (B, F) float64, zeros on unvoiced frames; "count" (B, F, 4) int32: the periods, the counted period pairs, amplitude pairs
    and triples; "marks" (B, F, 2 n_cycles + 1) int32, -1 where there is none; "lag" (B, F) int32}, F = ceil(L / hop_length)."""
    _trim_input(y, "perturbation")
    eng = _trim_engine(y.device)
    x = y.unsqueeze(0) if y.dim() == 1 else y
    ln = lengths if y.dim() == 2 else None
    if lag is None:
        tau_min, tau_max = pitch_lag_range(sr, fmin, fmax)
        lag, _, _ = eng.pitch_yin(x, ln, frame_length, hop_length, tau_min, tau_max, want_period=False, want_cmnd=False)
    frame, count, marks = eng.perturbation(x, ln, lag, hop_length, n_cycles, frame_length, period_factor, amplitude_factor, power_floor)
    out = {k: frame[..., i] for i, k in enumerate(_PERTURBATION_FRAME)}
    out.update(count=count, marks=marks, lag=lag)
    return out


def hnr_db(r):
    """The harmonics-to-noise ratio in dB of a harmonic strength r (the normalised cross-correlation at the period): 10 log10(r / (1 - r)), r
    clipped to [1e-6, 1 - 1e-9] (-60 .. 90 dB).  Torch ops only."""
    r = torch.as_tensor(r, dtype=torch.float64).clamp(1e-6, 1.0 - 1e-9)
    return 10.0 * torch.log10(r / (1.0 - r))


@torch.inference_mode()
def perturbation_statistics(pt, voiced, lengths=None):
    """Per utterance, from ``perturbation`` and a voicing mask at the same hop: {"jitter_pct", "rap_pct", "shimmer_pct", "shimmer_db", "hnr_db":
    (B,) float64, the means of 100 jitter, 100 rap, 100 shimmer, shimmer_db and ``hnr_db``(r) over the frames that are voiced, lie inside
    ``lengths`` and have at least one counted pair of the figure's kind (period pairs, triples, amplitude pairs; for hnr_db every such voiced
    frame); NaN where no frame qualifies; "frames" (B,) int64: the voiced frames inside; "used": {figure: (B,) int64, the frames behind its
    mean}; "sums": {figure: (B,) float64 sums over those frames, for pooling over utterances}}, where ``pt`` lives (torch ops only).  Entries
    are (B, F) / (B, F, 4) or one row without the leading axis; ``lengths`` (B,): the FRAMES that belong to each row (None: F)."""
    t = _coerced(pt, "count", _PERTURBATION_READ, voiced=voiced)

    def shapes(t, B, F):
        vals = [t[k] for k in _PERTURBATION_READ]
        if t["count"].dim() != 3 or t["count"].shape[2] != 4 or t["voiced"].shape != (B, F) or any(v.shape != (B, F) for v in vals):
            return (f"count (B, F, 4), the mask and the figures (B, F) expected, got {tuple(t['count'].shape)}, {tuple(t['voiced'].shape)} "
                    f"and {[tuple(v.shape) for v in vals]}")

    t, inside, _ = _inside(t, lengths, "perturbation_statistics", t["count"].dim() == 2, shapes)
    r = _reduce(*_perturbation_contours(t, t["voiced"] & inside))
    return {"frames": r["frames"], "used": r["used"], "sums": r["sums"], **r["means"]}


HARMONIC_POWER_FLOOR = 1e-7                        # the clamp of |X|^2 before the logarithm, ``voice_quality``'s
HARMONIC_FIGURES = ("h1_h2_db", "h1_a3_db", "f1_rel_db", "f2_rel_db", "f3_rel_db")
_HARMONIC_FRAME = HARMONIC_FIGURES + ("h1_db", "h1_hz", "spacing_bins")
_HARMONIC_FLAG = {"h1_h2_db": 1, "f1_rel_db": 2, "f2_rel_db": 4, "f3_rel_db": 8, "h1_a3_db": 16}
_HARMONIC_FORMANT = {"f1_rel_db": 0, "f2_rel_db": 1, "f3_rel_db": 2, "h1_a3_db": 2}       # the formant whose bandwidth a figure hangs on


def harmonic_arguments(n_harm: int = 48, search: float = 0.25, min_spacing: float = 4.0, a3_range: float = 0.1) -> None:
    """ValueError unless the comb's parameters are ones ``ev_load_harmonics`` takes: 1 <= n_harm <= 64, 0 < search <= 0.5, min_spacing finite
    and at least 2, 0 <= a3_range <= 0.5."""
    if not 1 <= int(n_harm) <= 64:
        raise ValueError(f"harmonics: n_harm={n_harm} outside 1 <= n_harm <= 64")
    if not 0.0 < float(search) <= 0.5:
        raise ValueError(f"harmonics: search={search} outside 0 < search <= 0.5")
    if not (float(min_spacing) >= 2.0 and math.isfinite(float(min_spacing))):
        raise ValueError(f"harmonics: min_spacing={min_spacing} must be finite and at least 2")
    if not 0.0 <= float(a3_range) <= 0.5:
        raise ValueError(f"harmonics: a3_range={a3_range} outside 0 <= a3_range <= 0.5")


_formants = formants                               # (``harmonics`` has an argument of that name)


def _harmonics_engine(device: torch.device, sr, n_fft: int, hop: int, n_harm: int, search: float, min_spacing: float, a3_range: float) -> Engine:
    return _cached_engine(device, ("harmonics", float(sr), int(n_fft), int(hop), int(n_harm), float(search), float(min_spacing), float(a3_range)),
                          lambda eng: eng.load_harmonics(stft_dist_window(n_fft), stoi_twiddle(n_fft), hop, n_fft, sr, n_harm, search, min_spacing,
                                                         a3_range))


@torch.inference_mode()
def harmonics(y, sr: int = 22050, fmin: float = 65.0, fmax: float = 600.0, frame_length: int = 1024, hop_length: int = 256, lengths=None,
              period=None, formants=None, n_harm: int = 48, search: float = 0.25, min_spacing: float = 4.0, a3_range: float = 0.1,
              power_floor: float = HARMONIC_POWER_FLOOR):
    """Harmonic differences per frame on the device (``ev_harmonics``; no torch fallback; Hanson 1997 and eGeMAPS, Eyben et al. 2016, are the
    model): in the float64 log-power spectrum of every voiced frame (``voice_quality``'s: periodic Hann window of ``frame_length`` = n_fft
    points, zeros outside the row) the harmonics of the frame's YIN period are found as the peaks within ``search`` of the spacing around
    h nfft / period, refined by a parabola, and give H1-H2, H1-A3 (A3: the strongest harmonic within ``a3_range`` of F3) and the level of the
    harmonic nearest F1, F2, F3 over H1.  A frame whose harmonics are closer than ``min_spacing`` bins is unresolved and gives zeros.
    ``period`` (B, F) float32: the periods of ``Engine.pitch_yin`` at the same hop; None runs YIN on the device (fmin, fmax, frame_length).
    ``formants``: the dict of ``formants`` at the same hop; None runs it; False leaves the formant terms out.  ``y`` 1-D, or (B, L) with
    ``lengths`` (B,) samples or None, on the GPU -> {"h1_h2_db", "h1_a3_db", "f1_rel_db", "f2_rel_db", "f3_rel_db", "h1_db", "h1_hz",
    "spacing_bins": (B, F) float64; "n_harmonics" (B, F) int32; "flags" (B, F) int32: bit 0 h1_h2_db, bits 1-3 fi_rel_db, bit 4 h1_a3_db is
    valid (an entry that is not valid is 0); "harmonic_hz", "harmonic_db" (B, F, n_harm) float64, zeros past n_harmonics}, F = ceil(L /
    hop_length); a 1-D input gives B = 1.  The levels are not corrected for the formants' gain (no H1*-H2*)."""
    _trim_input(y, "harmonics")
    harmonic_arguments(n_harm, search, min_spacing, a3_range)
    x = y.unsqueeze(0) if y.dim() == 1 else y
    ln = lengths if y.dim() == 2 else None
    if period is None:
        tau_min, tau_max = pitch_lag_range(sr, fmin, fmax)
        _, period, _ = _trim_engine(y.device).pitch_yin(x, ln, frame_length, hop_length, tau_min, tau_max, want_lag=False, want_cmnd=False)
    fm = fc = None
    if formants is None:
        formants = _formants(x, sr, frame_length=frame_length, hop_length=hop_length, lengths=ln)
    if formants is not False:
        fm = torch.stack((formants["frequency"], formants["bandwidth"]), dim=-1).contiguous()
        fc = formants["count"]
    eng = _harmonics_engine(y.device, sr, frame_length, hop_length, n_harm, search, min_spacing, a3_range)
    frame, count, harm = eng.harmonics(x, ln, period, fm, fc, power_floor)
    out = {k: frame[..., i] for i, k in enumerate(_HARMONIC_FRAME)}
    out.update(n_harmonics=count[..., 0], flags=count[..., 1], harmonic_hz=harm[..., 0], harmonic_db=harm[..., 1])
    return out


@torch.inference_mode()
def harmonic_statistics(hm, voiced, lengths=None, fm=None, max_bandwidth: float = 700.0):
    """Per utterance, from ``harmonics`` and a voicing mask at the same hop: {"h1_h2_db", "h1_a3_db", "f1_rel_db", "f2_rel_db", "f3_rel_db":
    (B,) float64, the mean of each figure over the frames that are voiced, lie inside ``lengths`` and carry the figure's flag; with ``fm``
    (the dict of ``formants`` at the same hop) fi_rel_db also needs F_i's bandwidth, and h1_a3_db F_3's, at or under ``max_bandwidth``; NaN
    where no frame qualifies; "frames" (B,) int64: the voiced frames inside; "used": {figure: (B,) int64, the frames behind its mean}; "sums":
    {figure: (B,) float64 sums over those frames, for pooling over utterances}}, where ``hm`` lives (torch ops only).  Entries are (B, F) or
    one row without the leading axis; ``lengths`` (B,): the FRAMES that belong to each row (None: F)."""
    t = _coerced(hm, "flags", HARMONIC_FIGURES, voiced=voiced)
    t["band"] = None if fm is None else torch.as_tensor(fm["bandwidth"], dtype=torch.float64).to(t["flags"].device)

    def shapes(t, B, F):
        vals, band = [t[k] for k in HARMONIC_FIGURES], t["band"]
        if t["flags"].dim() != 2 or t["voiced"].shape != (B, F) or any(v.shape != (B, F) for v in vals):
            return (f"flags, the mask and the figures (B, F) expected, got {tuple(t['flags'].shape)}, {tuple(t['voiced'].shape)} "
                    f"and {[tuple(v.shape) for v in vals]}")
        if band is not None and (band.dim() != 3 or tuple(band.shape[:2]) != (B, F) or band.shape[2] < 3):
            return f"the bandwidths must be ({B}, {F}, n >= 3), got {tuple(band.shape)}"

    t, inside, _ = _inside(t, lengths, "harmonic_statistics", t["flags"].dim() == 1, shapes)
    r = _reduce(*_harmonic_contours(t, t["voiced"] & inside, t["band"], max_bandwidth))
    return {"frames": r["frames"], "used": r["used"], "sums": r["sums"], **r["means"]}


AUDITORY_POWER_FLOOR = 1e-7                        # the clamp of the band energies before the logarithm and the power law, ``voice_quality``'s
AUDITORY_COMPRESS = 0.33                           # the exponent of the loudness: the cube-root law of Hermansky 1990 as openSMILE's cPlp rounds it
_AUDITORY_CONTOURS = ("loudness", "spectral_flux", "spectral_flux_voiced", "spectral_flux_unvoiced", "mfcc_1", "mfcc_2", "mfcc_3", "mfcc_4",
                      "mfcc_1_voiced", "mfcc_2_voiced", "mfcc_3_voiced", "mfcc_4_voiced")
AUDITORY_FIGURES = _AUDITORY_CONTOURS + ("equivalent_level_db",)
_AUDITORY_FRAME = ("loudness", "spectral_flux", "power", "log_energy")


def htk_mel(f):
    """The HTK mel scale, 2595 log10(1 + f / 700)."""
    return 2595.0 * np.log10(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def htk_mel_to_hz(m):
    return 700.0 * (10.0 ** (np.asarray(m, dtype=np.float64) / 2595.0) - 1.0)


def equal_loudness(f):
    """The equal-loudness weight of Hermansky 1990 (eq. 4) at ``f`` Hz: ((w^2 + 56.8e6) w^4) / ((w^2 + 6.3e6)^2 (w^2 + 0.38e9)), w = 2 pi f."""
    w2 = (2.0 * np.pi * np.asarray(f, dtype=np.float64)) ** 2
    return (w2 + 56.8e6) * w2 * w2 / ((w2 + 6.3e6) ** 2 * (w2 + 0.38e9))


def auditory_tables(sr: int, n_fft: int, n_mels: int = 26, fmin: float = 20.0, fmax: float = 8000.0, n_ceps: int = 4, lifter: float = 22.0,
                    flux_band=(0.0, None)) -> Dict:
    """The host tables of ``ev_load_auditory`` at rate ``sr``, float64 numpy: {"mel_w" (n_fft / 2 + 1, n_mels): triangular filters on the POWER
    spectrum whose corners are n_mels + 2 points equally spaced on the HTK mel scale from ``fmin`` to ``fmax``, linear in mel between them (HTK's
    and openSMILE's cMelspec: adjacent triangles sum to 1 between the first and the last centre); "centres_hz" (n_mels,); "eq" (n_mels,): the
    equal-loudness weights of Hermansky 1990 at the centres; "dct" (n_mels, n_ceps): the DCT-II columns i = 1 .. n_ceps, sqrt(2 / n_mels)
    cos(pi i (m + 1 / 2) / n_mels), times the HTK lifter 1 + lifter / 2 sin(pi i / lifter) (``lifter`` 0: none) - column 0, the level, is left
    out: a gain moves nothing else; "k_lo", "k_hi": the bins [ceil(lo n_fft / sr), ceil(hi n_fft / sr)) of the spectral flux, ``flux_band`` =
    (lo, hi) in Hz (hi None: up to and including the Nyquist bin); "compress": 0.33}.  ValueError on arguments ``ev_load_auditory`` would refuse,
    on a band without a bin and on a flux range without one: everything is checked here, without a device."""
    sr, n_fft, n_mels, n_ceps = int(sr), int(n_fft), int(n_mels), int(n_ceps)
    if sr < 1 or n_fft < 16 or n_fft > 1024 or n_fft % 2:
        raise ValueError(f"auditory_tables: sr={sr} must be positive and n_fft={n_fft} even with 16 <= n_fft <= 1024")
    if not 1 <= n_mels <= 64:
        raise ValueError(f"auditory_tables: n_mels={n_mels} outside 1 <= n_mels <= 64")
    if not 1 <= n_ceps <= min(16, max(n_mels - 1, 1)):
        raise ValueError(f"auditory_tables: n_ceps={n_ceps} outside 1 <= n_ceps <= min(16, n_mels - 1) = {min(16, max(n_mels - 1, 1))}")
    if not (math.isfinite(fmin) and math.isfinite(fmax) and 0.0 <= fmin < fmax <= sr / 2.0):
        raise ValueError(f"auditory_tables: 0 <= fmin < fmax <= sr / 2 expected (got fmin={fmin} fmax={fmax} sr={sr})")
    if not (math.isfinite(lifter) and (lifter == 0.0 or lifter >= 1.0)):
        raise ValueError(f"auditory_tables: lifter={lifter} must be 0 (none) or at least 1")
    NB = n_fft // 2 + 1
    lo, hi = flux_band
    if not (math.isfinite(lo) and lo >= 0.0 and (hi is None or (math.isfinite(hi) and hi > lo))):
        raise ValueError(f"auditory_tables: flux_band={flux_band} must be (lo, hi) in Hz with 0 <= lo < hi, or hi None")
    k_lo = int(math.ceil(lo * n_fft / sr))
    k_hi = NB if hi is None else min(NB, int(math.ceil(hi * n_fft / sr)))
    if not 0 <= k_lo < k_hi:
        raise ValueError(f"auditory_tables: flux_band={flux_band} holds no bin at sr={sr}, n_fft={n_fft} (bins [{k_lo}, {k_hi}))")
    corners = np.linspace(float(htk_mel(fmin)), float(htk_mel(fmax)), n_mels + 2)
    mel_k = htk_mel(np.arange(NB, dtype=np.float64) * sr / n_fft)[:, None]
    left, centre, right = corners[None, :-2], corners[None, 1:-1], corners[None, 2:]
    mel_w = np.maximum(0.0, np.minimum((mel_k - left) / (centre - left), (right - mel_k) / (right - centre)))
    empty = np.flatnonzero(~(mel_w > 0.0).any(axis=0))
    if empty.size:
        raise ValueError(f"auditory_tables: band {int(empty[0])} of {n_mels} from {fmin} to {fmax} Hz holds no bin at sr={sr}, n_fft={n_fft}: "
                         "fewer bands, a higher fmin or a longer n_fft")
    centres = htk_mel_to_hz(corners[1:-1])
    i = np.arange(1, n_ceps + 1, dtype=np.float64)[None, :]
    dct = math.sqrt(2.0 / n_mels) * np.cos(np.pi * i * (np.arange(n_mels, dtype=np.float64)[:, None] + 0.5) / n_mels)
    if lifter:
        dct = dct * (1.0 + 0.5 * lifter * np.sin(np.pi * i / lifter))
    return {"mel_w": np.ascontiguousarray(mel_w), "centres_hz": centres, "eq": equal_loudness(centres), "dct": np.ascontiguousarray(dct),
            "k_lo": k_lo, "k_hi": k_hi, "compress": AUDITORY_COMPRESS}


def _auditory_engine(device: torch.device, sr: int, n_fft: int, hop: int, n_mels: int, fmin: float, fmax: float, n_ceps: int, lifter: float,
                     flux_band) -> Engine:
    def load(eng):
        t = auditory_tables(sr, n_fft, n_mels, fmin, fmax, n_ceps, lifter, flux_band)
        eng.load_auditory(stft_dist_window(n_fft), stoi_twiddle(n_fft), hop, n_fft, t["mel_w"], t["eq"], t["dct"], t["k_lo"], t["k_hi"], t["compress"])
    band = (float(flux_band[0]), None if flux_band[1] is None else float(flux_band[1]))
    return _cached_engine(device, ("auditory", int(sr), int(n_fft), int(hop), int(n_mels), float(fmin), float(fmax), int(n_ceps), float(lifter), band), load)


@torch.inference_mode()
def auditory(y, sr: int = 22050, frame_length: int = 1024, hop_length: int = 256, lengths=None, n_mels: int = 26, fmin: float = 20.0,
             fmax: float = 8000.0, n_ceps: int = 4, lifter: float = 22.0, flux_band=(0.0, None), power_floor: float = AUDITORY_POWER_FLOOR):
    """Timbre and dynamics per frame on the device (``ev_auditory``; no torch fallback; eGeMAPS, Eyben et al. 2016, is the model): from the float64
    power spectrum of every frame (``voice_quality``'s: periodic Hann window of ``frame_length`` = n_fft points, zeros outside the row) the
    energies of ``n_mels`` HTK mel bands between ``fmin`` and ``fmax`` (clamped at ``power_floor``), and from them the loudness (the sum over the
    bands of (equal-loudness weight x energy)^0.33), the cepstral coefficients 1 .. ``n_ceps`` (DCT-II of the log energies, HTK lifter
    ``lifter``), and beside them the spectral flux (the rms difference of the magnitude spectrum to the frame before, over the bins of
    ``flux_band`` Hz), the power and its logarithm (``auditory_tables`` has the details).  Frame f is ``pitch_yin``'s frame f at the same hop.
    ``y`` 1-D, or (B, L) with ``lengths`` (B,) samples or None, on the GPU -> {"loudness", "spectral_flux", "power", "log_energy": (B, F)
    float64; "mfcc" (B, F, n_ceps) float64; "live" (B, F) bool: some bin lies above the floor; "has_previous" (B, F) bool: the frame has a
    predecessor in its row (every frame of a row but the first: the first frame's flux is 0 by definition)}, F = ceil(L / hop_length); a 1-D input
    gives B = 1.  A silent frame keeps its power and its flux and has zeros elsewhere; a frame past a row's ceil(len / hop_length) has zeros and
    False everywhere.  The figures are comparable across runs of this project, not to the digit with openSMILE's, which frames differently (25 ms
    Hamming windows for MFCC) and scales its own way."""
    _trim_input(y, "auditory")
    eng = _auditory_engine(y.device, sr, frame_length, hop_length, n_mels, fmin, fmax, n_ceps, lifter, flux_band)
    x = y.unsqueeze(0) if y.dim() == 1 else y
    r = eng.auditory(x, lengths if y.dim() == 2 else None, power_floor)
    out = {k: r["frame"][:, :, i] for i, k in enumerate(_AUDITORY_FRAME)}
    out.update(mfcc=r["mfcc"], live=(r["flags"] & 1) != 0, has_previous=(r["flags"] & 2) != 0)
    return out


def _auditory_contours(t, use):
    """``use`` here is the frames inside the row (timbre and dynamics are not figures of the voiced frames alone) and t["voiced"] the voicing.
    The frames mask: the live frames inside; behind the loudness and the MFCC those, behind the flux the frames with a predecessor, behind a
    ``_voiced`` / ``_unvoiced`` figure the voiced / unvoiced ones of them."""
    if t["mfcc"].shape[-1] < 4:
        raise ValueError(f"auditory contours need the cepstral coefficients 1 .. 4, got {t['mfcc'].shape[-1]}")
    live, moved = use & t["live"], use & t["has_previous"]
    live_v, moved_v, moved_u = live & t["voiced"], moved & t["voiced"], moved & ~t["voiced"]
    out = {"loudness": (t["loudness"], live), "spectral_flux": (t["spectral_flux"], moved), "spectral_flux_voiced": (t["spectral_flux"], moved_v),
           "spectral_flux_unvoiced": (t["spectral_flux"], moved_u)}
    out.update({f"mfcc_{i + 1}": (t["mfcc"][:, :, i], live) for i in range(4)})
    out.update({f"mfcc_{i + 1}_voiced": (t["mfcc"][:, :, i], live_v) for i in range(4)})
    return live, out


def _auditory_coerced(au, voiced, dev=None):
    t = _coerced(au, "live", ("loudness", "spectral_flux", "power", "mfcc"), dev, voiced)
    t["live"], t["has_previous"] = t["live"].to(torch.bool), torch.as_tensor(au["has_previous"]).to(t["live"].device, torch.bool)
    return t


@torch.inference_mode()
def auditory_statistics(au, voiced, lengths=None):
    """Per utterance, from ``auditory`` and a voicing mask at the same hop: {"loudness", "mfcc_1" .. "mfcc_4": (B,) float64, the mean over the live
    frames inside ``lengths``; "spectral_flux": over the frames inside that have a predecessor; "spectral_flux_voiced", "spectral_flux_unvoiced",
    "mfcc_1_voiced" .. "mfcc_4_voiced": over the voiced / unvoiced ones of those; "equivalent_level_db": 10 log10 of the mean power over every
    frame inside (a level comparable across runs, not dB SPL); NaN where no frame qualifies (-inf for an all-zero row); "frames" (B,) int64: the
    live frames inside; "used": {figure: (B,) int64, the frames behind its mean}; "sums": {figure: (B,) float64 sums over those frames, for pooling
    over utterances - under "equivalent_level_db" the sum of the POWER, which is what pools}}, where ``au`` lives (torch ops only).  Entries are (B,
    F) (mfcc (B, F, n_ceps >= 4)) or one row without the leading axis; ``lengths`` (B,): the FRAMES that belong to each row (None: F)."""
    t = _auditory_coerced(au, voiced)

    def shapes(t, B, F):
        flat = [t[k] for k in ("has_previous", "voiced", "loudness", "spectral_flux", "power")]
        if t["live"].dim() != 2 or any(v.shape != (B, F) for v in flat) or t["mfcc"].dim() != 3 or tuple(t["mfcc"].shape[:2]) != (B, F):
            return (f"live, has_previous, the mask and the figures (B, F) and mfcc (B, F, n_ceps) expected, got {tuple(t['live'].shape)}, "
                    f"{[tuple(v.shape) for v in flat]} and {tuple(t['mfcc'].shape)}")

    t, inside, _ = _inside(t, lengths, "auditory_statistics", t["live"].dim() == 1, shapes)
    frames, contours = _auditory_contours(t, inside)
    contours["equivalent_level_db"] = (t["power"], inside)
    r = _reduce(frames, contours)
    r["means"]["equivalent_level_db"] = 10.0 * torch.log10(r["means"]["equivalent_level_db"])
    return {"frames": r["frames"], "used": r["used"], "sums": r["sums"], **r["means"]}


FUNCTIONAL_STATISTICS = ("mean", "sd", "min", "max", "rise_mean", "rise_sd", "fall_mean", "fall_sd", "run_mean", "run_sd", "gap_mean", "gap_sd")
FUNCTIONAL_COUNTS = ("valid", "dropped", "rising_parts", "falling_parts", "peaks", "runs", "gaps", "adjacent_pairs")
_FUNCTIONAL_BEHIND = {"mean": 0, "sd": 0, "min": 0, "max": 0, "rise_mean": 2, "rise_sd": 2, "fall_mean": 3, "fall_sd": 3, "run_mean": 5, "run_sd": 5,
                      "gap_mean": 6, "gap_sd": 6}              # the count behind each statistic: 0 of it makes the statistic NaN
FUNCTIONAL_MAX_FRAMES = 4096                                   # ``ev_functionals``' (and ``ev_dtw``'s) frame limit: 47 s at hop 256 and 22.05 kHz
SEMITONE_REFERENCE_HZ = 27.5                                   # eGeMAPS's semitone scale starts at 27.5 Hz


def functional_arguments(values, mask=None, lengths=None, percentiles=(0.2, 0.5, 0.8)):
    """ValueError unless ``functionals`` takes the arguments (everything that needs no device): ``values`` a floating tensor of 1 to 3
    dimensions with 1 <= F <= 4096 frames, ``mask`` broadcastable to it, one length per row, at most 16 ``percentiles``, each finite and in
    [0, 1].  Returns (B, K, F) and the percentiles as a float64 array."""
    if not torch.is_tensor(values) or not values.is_floating_point() or values.dim() not in (1, 2, 3):
        raise ValueError("functionals: values must be a floating tensor (B, K, F), (B, F) or 1-D")
    F = int(values.shape[-1])
    B = int(values.shape[0]) if values.dim() > 1 else 1
    K = int(values.shape[1]) if values.dim() == 3 else 1
    if not 1 <= F <= FUNCTIONAL_MAX_FRAMES:
        raise ValueError(f"functionals: F={F} outside 1 <= F <= {FUNCTIONAL_MAX_FRAMES}")
    if B < 1 or K < 1:
        raise ValueError(f"functionals: values {tuple(values.shape)} has no contour")
    q = np.asarray(percentiles, dtype=np.float64).reshape(-1)
    if q.shape[0] > 16:
        raise ValueError(f"functionals: {q.shape[0]} percentiles given, at most 16 are taken")
    if not bool(np.all(np.isfinite(q) & (q >= 0.0) & (q <= 1.0))):
        raise ValueError(f"functionals: percentiles {[float(v) for v in q]} must be finite and lie in [0, 1] (fractions, not per cent)")
    if mask is not None:
        try:
            torch.broadcast_shapes(tuple(torch.as_tensor(mask).shape), tuple(values.shape))
        except RuntimeError:
            raise ValueError(f"functionals: the mask {tuple(torch.as_tensor(mask).shape)} does not broadcast to the values {tuple(values.shape)}") from None
        if torch.as_tensor(mask).dim() > values.dim():
            raise ValueError(f"functionals: the mask {tuple(torch.as_tensor(mask).shape)} has more dimensions than the values {tuple(values.shape)}")
    if lengths is not None and torch.as_tensor(lengths).numel() != B:
        raise ValueError(f"functionals: {B} lengths expected, got {torch.as_tensor(lengths).numel()}")
    return (B, K, F), q


@torch.inference_mode()
def functionals(values, mask=None, lengths=None, percentiles=(0.2, 0.5, 0.8)):
    """The eGeMAPS functionals (Eyben et al. 2016) of every contour on the device (``ev_functionals``: one launch per call, a workgroup per
    contour; no torch fallback).  ``values`` (B, K, F), (B, F) (K = 1) or 1-D (B = K = 1), any float dtype, on the GPU; ``mask`` broadcastable
    to ``values`` (non-zero: the frame counts) or None; ``lengths`` (B,): the FRAMES of each row (None: F); ``percentiles``: up to 16 fractions
    in [0, 1].  A frame is valid inside its row's length, under a non-zero mask and with a finite value.  -> a dict of (B, K) tensors:
    "mean", "sd" (population), "min", "max"; "rise_mean", "rise_sd", "fall_mean", "fall_sd": the slopes per FRAME of the maximal strictly rising
    / falling stretches of adjacent valid frames; "run_mean", "run_sd", "gap_mean", "gap_sd": the lengths in frames of the stretches of valid
    frames and of the gaps between them (leading and trailing gaps included), float64, NaN where the count behind a statistic is 0;
    "percentiles" (B, K, NQ) (numpy's linear interpolation) and "range", the last percentile minus the first (NaN without a valid frame or
    without percentiles); "valid", "dropped" (non-finite values under the mask), "rising_parts", "falling_parts", "peaks" (u_i > u_{i-1} and
    u_i >= u_{i+1} among adjacent frames), "runs", "gaps", "adjacent_pairs": int32."""
    (B, K, F), q = functional_arguments(values, mask, lengths, percentiles)
    if not values.is_cuda:
        raise EvLibraryError("functionals runs on a ROCm GPU only (no CPU fallback): move values to the GPU")
    v = values.reshape(B, K, F).to(torch.float64)
    m = None
    if mask is not None:
        m = torch.as_tensor(mask, device=values.device)
        m = (m != 0).expand(values.shape).reshape(B, K, F).to(torch.uint8).contiguous()
    stat, count = _trim_engine(values.device).functionals(v, m, lengths, q)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=v.device)
    out = {k: torch.where(count[..., _FUNCTIONAL_BEHIND[k]] > 0, stat[..., i], nan) for i, k in enumerate(FUNCTIONAL_STATISTICS)}
    has = count[..., 0] > 0
    out["percentiles"] = torch.where(has[..., None], stat[..., 12:], nan)
    out["range"] = out["percentiles"][..., -1] - out["percentiles"][..., 0] if q.shape[0] else nan.expand(B, K).clone()
    out.update({k: count[..., i] for i, k in enumerate(FUNCTIONAL_COUNTS)})
    return out


@torch.inference_mode()
def voice_functionals(pitch, vq, n_frames=None, fm=None, pt=None, hm=None, sr: int = 22050, hop_length: int = 256, percentiles=(0.2, 0.5, 0.8),
                      max_bandwidth: float = 700.0, harmonic_fm=None, au=None):
    """The functionals of every contour the voice report has, in ONE ``functionals`` call per batch: ``pitch`` (the dict of ``pitch_yin`` /
    ``pitch_pyin``), ``vq`` (of ``voice_quality``) and, when given, ``fm`` (``formants``), ``pt`` (``perturbation``), ``hm`` (``harmonics``) and
    ``au`` (``auditory``), all (B, F) at the same hop on the GPU; ``n_frames`` (B,): the frames of each row (None: F).  The contours and their masks, each the mask
    of the matching ``*_statistics`` function (so a contour's "mean" is that function's mean):
      "f0_semitones"              12 log2(f0 / 27.5), eGeMAPS's scale, over the voiced frames (``prosody_statistics``' mask)
      VOICE_QUALITY_FIGURES       voiced and not silent (``voice_quality_statistics``)
      FORMANT_FIGURES             voiced, at least three formants, F_i's bandwidth at most ``max_bandwidth`` (``formant_statistics``)
      PERTURBATION_FIGURES        voiced with YIN's lag > 0 and a counted pair of the figure's kind (``perturbation_statistics`` as --perturbation
                                  calls it), in its units: per cent, dB, ``hnr_db``(r)
      HARMONIC_FIGURES            voiced and carrying the figure's flag, and under the bandwidth rule of ``harmonic_statistics`` at the formants
                                  ``harmonic_fm`` (None: ``fm``; neither: no bandwidth rule)
      the auditory contours       AUDITORY_FIGURES without the level: loudness and MFCC 1-4 over the live frames inside the row, the flux over the
                                  frames with a predecessor, the ``_voiced`` / ``_unvoiced`` ones under the voicing (``auditory_statistics``);
                                  "peaks_per_s" of "loudness" is eGeMAPS's loudness peaks per second
    -> {contour: {statistic: (B,)}} with the keys of ``functionals`` and, beside them, "peaks_per_s" (peaks over the row's seconds) and the
    four slope statistics in units per SECOND (scaled by sr / hop_length); "segments": {"voiced_per_s", "voiced_mean_s", "voiced_sd_s",
    "unvoiced_mean_s", "unvoiced_sd_s"} from the runs and the gaps of the voicing contour; "contours": the names in stacking order."""
    f0 = torch.as_tensor(pitch["f0"])
    if f0.dim() == 1:
        raise ValueError("voice_functionals: (B, F) contours expected (add the batch axis to a single row)")
    B, F = f0.shape
    dev = f0.device
    t, inside, n = _inside({"f0": f0, "voiced": torch.as_tensor(pitch["voiced"], dtype=torch.bool, device=dev)}, n_frames, "voice_functionals")
    use = t["voiced"] & inside
    contours = {"f0_semitones": (12.0 * torch.log2(torch.where(use, f0.to(torch.float64), torch.full((), SEMITONE_REFERENCE_HZ, dtype=torch.float64, device=dev))
                                                   / SEMITONE_REFERENCE_HZ), use)}
    contours.update(_voice_quality_contours(_coerced(vq, "peak_quefrency", VOICE_QUALITY_FIGURES, dev), use)[1])
    band = None
    if fm is not None:
        tf = _coerced(fm, "count", ("frequency", "bandwidth"), dev)
        band = tf["bandwidth"]
        contours.update(_formant_contours(tf, use, max_bandwidth)[1])
    if pt is not None:
        contours.update(_perturbation_contours(_coerced(pt, "count", _PERTURBATION_READ, dev), use & (torch.as_tensor(pt["lag"]).to(dev) > 0))[1])
    if hm is not None:
        if harmonic_fm is not None:
            band = torch.as_tensor(harmonic_fm["bandwidth"], dtype=torch.float64).to(dev)
        contours.update(_harmonic_contours(_coerced(hm, "flags", HARMONIC_FIGURES, dev), use, band, max_bandwidth)[1])
    if au is not None:
        contours.update(_auditory_contours(_auditory_coerced(au, t["voiced"], dev), inside)[1])
    names = list(contours) + ["voicing"]                     # the runs and gaps of the voicing itself: the temporal group
    vals = [v for v, _ in contours.values()] + [torch.zeros((B, F), dtype=torch.float64, device=dev)]
    masks = [m for _, m in contours.values()] + [use]
    fn = functionals(torch.stack(vals, dim=1), torch.stack(masks, dim=1), n, percentiles)
    rate = float(sr) / float(hop_length)
    seconds = n.to(torch.float64) / rate
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    out = {"contours": tuple(names[:-1])}
    for j, name in enumerate(names[:-1]):
        o = {k: v[:, j] for k, v in fn.items()}
        for k in ("rise_mean", "rise_sd", "fall_mean", "fall_sd"):
            o[k] = o[k] * rate
        o["peaks_per_s"] = torch.where(seconds > 0, o["peaks"].to(torch.float64) / seconds.clamp(min=1e-300), nan)
        out[name] = o
    j = len(names) - 1
    out["segments"] = {"voiced_per_s": torch.where(seconds > 0, fn["runs"][:, j].to(torch.float64) / seconds.clamp(min=1e-300), nan),
                       "voiced_mean_s": fn["run_mean"][:, j] / rate, "voiced_sd_s": fn["run_sd"][:, j] / rate,
                       "unvoiced_mean_s": fn["gap_mean"][:, j] / rate, "unvoiced_sd_s": fn["gap_sd"][:, j] / rate}
    return out


MODULATION_MAX_FREQUENCIES = 128                               # ``ev_modulation``'s grid limit
MODULATION_MIN_RUN_S = 0.2                                     # runs of valid frames shorter than this are not analysed (17 frames at hop 256)
MODULATION_MIN_CYCLES = 2.0                                    # a run speaks for a frequency when it holds at least two cycles of it
MODULATION_TREMOR_HZ = (4.0, 12.0)                             # tremor and vibrato of f0 and of loudness
MODULATION_RHYTHM_HZ = (2.0, 8.0)                              # the syllable rate of the loudness contour
MODULATION_COUNTS = ("valid", "dropped", "runs", "frames")


def _modulation_grid(frame_rate: float, fmin_hz: float, fmax_hz: float, step_hz: float) -> Tuple[float, float, int]:
    vals = (frame_rate, fmin_hz, fmax_hz, step_hz)
    if not all(math.isfinite(float(v)) and float(v) > 0.0 for v in vals) or fmax_hz < fmin_hz:
        raise ValueError(f"modulation: frame_rate={frame_rate}, fmin_hz={fmin_hz}, fmax_hz={fmax_hz}, step_hz={step_hz} must be finite and greater "
                         "than 0 with fmin_hz <= fmax_hz")
    NM = int(math.floor((float(fmax_hz) - float(fmin_hz)) / float(step_hz) + 1e-9)) + 1
    if NM > MODULATION_MAX_FREQUENCIES:
        raise ValueError(f"modulation: {fmin_hz} .. {fmax_hz} Hz in steps of {step_hz} Hz are {NM} frequencies, at most {MODULATION_MAX_FREQUENCIES} "
                         "are taken")
    nu0, dnu = float(fmin_hz) / float(frame_rate), float(step_hz) / float(frame_rate)
    if nu0 + (NM - 1) * dnu > 0.5:
        raise ValueError(f"modulation: the grid ends at {fmin_hz + (NM - 1) * step_hz} Hz, over half the frame rate of {frame_rate} Hz")
    return nu0, dnu, NM


def modulation_grid(sr, hop_length, fmin_hz: float = 1.0, fmax_hz: float = 16.0, step_hz: float = 0.125) -> Tuple[float, float, int]:
    """(nu0, dnu, NM) of ``ev_modulation`` for contours at ``sr`` / ``hop_length`` frames per second: the frequencies fmin_hz + j step_hz up
    to fmax_hz, in cycles per frame.  ValueError for more than 128 of them or for a grid over half the frame rate.  At 0.125 Hz a sinusoid
    between two grid points loses under 1 % of its extent to the parabola through the log powers; at 0.25 Hz and 6 s it loses 18 %."""
    if not (float(sr) > 0 and float(hop_length) > 0):
        raise ValueError(f"modulation_grid: sr={sr} and hop_length={hop_length} must be greater than 0")
    return _modulation_grid(float(sr) / float(hop_length), fmin_hz, fmax_hz, step_hz)


def modulation_bands(bands_hz, fmin_hz: float, step_hz: float, NM: int):
    """The index ranges [j_lo, j_hi) of the grid points inside each closed band (lo_hz, hi_hz); ValueError for more than four bands or for a
    band without a grid point."""
    bands = [tuple(float(x) for x in b) for b in bands_hz]
    if len(bands) > 4:
        raise ValueError(f"modulation: {len(bands)} bands given, at most 4 are taken")
    out = []
    for lo, hi in bands:
        j_lo = max(int(math.ceil((lo - fmin_hz) / step_hz - 1e-9)), 0)
        j_hi = min(int(math.floor((hi - fmin_hz) / step_hz + 1e-9)) + 1, NM)
        if not (math.isfinite(lo) and math.isfinite(hi)) or j_lo >= j_hi:
            raise ValueError(f"modulation: the band {lo} .. {hi} Hz holds no frequency of the grid")
        out.append((j_lo, j_hi))
    return out


def modulation_arguments(values, mask=None, lengths=None, frame_rate: float = 22050.0 / 256.0, bands_hz=(), fmin_hz: float = 1.0,
                         fmax_hz: float = 16.0, step_hz: float = 0.125, min_run: Optional[int] = None, min_cycles: float = MODULATION_MIN_CYCLES):
    """ValueError unless ``modulation`` takes the arguments (everything that needs no device): ``functionals``' rules for ``values``, ``mask``
    and ``lengths``, a grid ``modulation_grid`` accepts, at most four bands that each hold a grid point, 3 <= min_run <= F (None: the frames
    of MODULATION_MIN_RUN_S, inside those bounds), min_cycles finite and at least 0.  Returns ((B, K, F), (nu0, dnu, NM), the bands as index
    pairs, min_run)."""
    try:
        shape, _ = functional_arguments(values, mask, lengths, ())
    except ValueError as e:
        raise ValueError(str(e).replace("functionals:", "modulation:")) from None
    grid = _modulation_grid(frame_rate, fmin_hz, fmax_hz, step_hz)
    bands = modulation_bands(bands_hz, float(fmin_hz), float(step_hz), grid[2])
    F = shape[2]
    if F < 3:
        raise ValueError(f"modulation: F={F} frames, at least 3 are needed")
    if min_run is None:
        min_run = min(max(int(math.ceil(MODULATION_MIN_RUN_S * float(frame_rate))), 3), F)
    if not 3 <= int(min_run) <= F:
        raise ValueError(f"modulation: min_run={min_run} outside 3 <= min_run <= F = {F}")
    if not (math.isfinite(float(min_cycles)) and float(min_cycles) >= 0.0):
        raise ValueError(f"modulation: min_cycles={min_cycles} must be finite and at least 0")
    return shape, grid, bands, int(min_run)


@torch.inference_mode()
def modulation(values, mask=None, lengths=None, frame_rate: float = 22050.0 / 256.0, bands_hz=(), fmin_hz: float = 1.0, fmax_hz: float = 16.0,
               step_hz: float = 0.125, min_run: Optional[int] = None, min_cycles: float = MODULATION_MIN_CYCLES):
    """The modulation spectrum of every contour on the device (``ev_modulation``: one launch per call, a workgroup per contour; no torch
    fallback): how strongly the contour oscillates at each of the frequencies fmin_hz + j step_hz, and the strongest local peak of up to four
    bands.  ``values``, ``mask`` and ``lengths`` follow ``functionals``' rules; ``frame_rate``: frames per second.  Every run of at least
    ``min_run`` valid frames is detrended by its own line, Hann-windowed and analysed on its own: nothing crosses a gap.  A run counts at a
    frequency when it holds ``min_cycles`` cycles of it; runs pool by their lengths.  -> {"frequencies_hz" (NM,) float64; "spectrum" (B, K,
    NM) float64: half the squared amplitude of the oscillation at each frequency, in the contour's units squared, 0 where no run counts;
    "weight" (B, K, NM) int32: the frames behind each; per band (B, K, NBAND): "rate_hz", the interpolated frequency of the peak, "extent",
    its amplitude in the contour's units, "prominence_db", 10 log10 of its power over the band's mean, "band_mean", NaN where the band has
    no local peak, and "peak_index" int32, -1 there; "residual_variance" and "slope" (per second) (B, K): what the lines leave and their
    length-weighted mean, NaN without an analysed run; "valid", "dropped", "runs", "frames" (B, K) int32: the valid frames, the non-finite
    ones under the mask, the analysed runs and their frames}."""
    (B, K, F), (nu0, dnu, NM), bands, min_run = modulation_arguments(values, mask, lengths, frame_rate, bands_hz, fmin_hz, fmax_hz, step_hz, min_run,
                                                                     min_cycles)
    if not values.is_cuda:
        raise EvLibraryError("modulation runs on a ROCm GPU only (no CPU fallback): move values to the GPU")
    v = values.reshape(B, K, F).to(torch.float64)
    m = None
    if mask is not None:
        m = torch.as_tensor(mask, device=values.device)
        m = (m != 0).expand(values.shape).reshape(B, K, F).to(torch.uint8).contiguous()
    spec, weight, peak, stat, count = _trim_engine(values.device).modulation(v, m, lengths, nu0, dnu, NM, min_run, float(min_cycles), bands)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=v.device)
    idx = count[..., 4:]
    has = idx >= 0
    ran = count[..., 2] > 0
    out = {"frequencies_hz": torch.from_numpy(float(fmin_hz) + np.arange(NM, dtype=np.float64) * float(step_hz)).to(v.device),
           "spectrum": spec, "weight": weight,
           "rate_hz": torch.where(has, peak[..., 0] * float(frame_rate), nan), "extent": torch.where(has, peak[..., 1], nan),
           "band_mean": torch.where(has, peak[..., 2], nan),
           "prominence_db": torch.where(has, 10.0 * torch.log10(torch.where(has, peak[..., 3], torch.ones_like(peak[..., 3]))), nan),
           "peak_index": idx, "residual_variance": torch.where(ran, stat[..., 0], nan),
           "slope": torch.where(ran, stat[..., 1] * float(frame_rate), nan)}
    out.update({k: count[..., i] for i, k in enumerate(MODULATION_COUNTS)})
    return out


VOICE_MODULATION_FIGURES = ("tremor_rate_hz", "tremor_extent_st", "tremor_prominence_db", "f0_residual_sd_st", "loudness_tremor_rate_hz",
                            "loudness_tremor_depth", "rhythm_rate_hz", "rhythm_depth", "rhythm_prominence_db")


@torch.inference_mode()
def voice_modulation(pitch, au, n_frames=None, sr: int = 22050, hop_length: int = 256, min_run: Optional[int] = None,
                     min_cycles: float = MODULATION_MIN_CYCLES, fmin_hz: float = 1.0, fmax_hz: float = 16.0, step_hz: float = 0.125):
    """Tremor and rhythm of a voice in ONE ``modulation`` call over two contours: ``pitch`` (the dict of ``pitch_yin`` / ``pitch_pyin``) and
    ``au`` (of ``auditory``), (B, F) at the same hop on the GPU; ``n_frames`` (B,): the frames of each row (None: F).
      "f0_semitones"   12 log2(f0 / 27.5) under the voicing (``voice_functionals``' contour): the tremor band is 4-12 Hz, the extent in semitones
      "loudness"       over the live frames inside the row: the rhythm band is 2-8 Hz; a depth is the amplitude over the mean loudness
    -> {figure: (B,) float64 for the VOICE_MODULATION_FIGURES, NaN where the band has no peak (or no run was analysed); "f0_semitones" and
    "loudness": the two contours' rows of ``modulation``'s result; "frequencies_hz"}."""
    f0 = torch.as_tensor(pitch["f0"])
    if f0.dim() == 1:
        raise ValueError("voice_modulation: (B, F) contours expected (add the batch axis to a single row)")
    B, F = f0.shape
    dev = f0.device
    t, inside, n = _inside({"f0": f0, "voiced": torch.as_tensor(pitch["voiced"], dtype=torch.bool, device=dev)}, n_frames, "voice_modulation")
    use = t["voiced"] & inside
    st = 12.0 * torch.log2(torch.where(use, f0.to(torch.float64), torch.full((), SEMITONE_REFERENCE_HZ, dtype=torch.float64, device=dev))
                           / SEMITONE_REFERENCE_HZ)
    ta = _auditory_coerced(au, t["voiced"], dev)
    if tuple(ta["loudness"].shape) != (B, F):
        raise ValueError(f"voice_modulation: the loudness {tuple(ta['loudness'].shape)} and the pitch {(B, F)} are not at the same frames")
    live = inside & ta["live"]
    md = modulation(torch.stack([st, ta["loudness"]], dim=1), torch.stack([use, live], dim=1), n, float(sr) / float(hop_length),
                    (MODULATION_TREMOR_HZ, MODULATION_RHYTHM_HZ), fmin_hz, fmax_hz, step_hz, min_run, min_cycles)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    cnt = live.sum(dim=1)
    mean_l = torch.where(cnt > 0, (ta["loudness"] * live).sum(dim=1) / cnt.clamp(min=1), nan)
    mean_l = torch.where(mean_l > 0, mean_l, nan)
    out = {"tremor_rate_hz": md["rate_hz"][:, 0, 0], "tremor_extent_st": md["extent"][:, 0, 0], "tremor_prominence_db": md["prominence_db"][:, 0, 0],
           "f0_residual_sd_st": torch.sqrt(md["residual_variance"][:, 0]),
           "loudness_tremor_rate_hz": md["rate_hz"][:, 1, 0], "loudness_tremor_depth": md["extent"][:, 1, 0] / mean_l,
           "rhythm_rate_hz": md["rate_hz"][:, 1, 1], "rhythm_depth": md["extent"][:, 1, 1] / mean_l, "rhythm_prominence_db": md["prominence_db"][:, 1, 1]}
    for j, name in enumerate(("f0_semitones", "loudness")):
        out[name] = {k: v[:, j] for k, v in md.items() if k != "frequencies_hz"}
    out["frequencies_hz"] = md["frequencies_hz"]
    return out


MS_DISTANCE_GRID_HZ = (1.0, 32.0, 0.25)                        # fmin, fmax, step of ``modulation_spectrum_distance``: 125 frequencies


@torch.inference_mode()
def cepstral_modulation_distance(cep_a, cep_b, len_a=None, len_b=None, sr: int = 22050, hop_length: int = 256, min_run: Optional[int] = None,
                                 min_cycles: float = MODULATION_MIN_CYCLES):
    """``modulation_spectrum_distance`` of two stacks of trajectories (B, K, Ta) and (B, K, Tb) that are already cepstra (or any K contours per
    row): two ``modulation`` calls and the comparison in dB."""
    if cep_a.dim() != 3 or cep_b.dim() != 3 or cep_a.shape[:2] != cep_b.shape[:2]:
        raise ValueError(f"modulation_spectrum_distance: two stacks (B, K, T) of one batch expected, got {tuple(cep_a.shape)} and {tuple(cep_b.shape)}")
    fmin, fmax, step = MS_DISTANCE_GRID_HZ
    rate = float(sr) / float(hop_length)
    sp = []
    for cep, ln in ((cep_a, len_a), (cep_b, len_b)):
        md = modulation(cep, None, ln, rate, (), fmin, fmax, step, min_run, min_cycles)
        sp.append((md["spectrum"], md["weight"]))
    (pa, wa), (pb, wb) = sp
    both = (wa > 0) & (wb > 0) & (pa > 0) & (pb > 0)
    one = torch.ones_like(pa)
    d = torch.where(both, 10.0 * torch.log10(torch.where(both, pb, one)) - 10.0 * torch.log10(torch.where(both, pa, one)), torch.zeros_like(pa))
    pairs = both.sum(dim=(1, 2))
    nan = torch.full((), float("nan"), dtype=torch.float64, device=pa.device)
    cnt = pairs.clamp(min=1).to(torch.float64)
    return {"ms_distortion_db": torch.where(pairs > 0, torch.sqrt((d * d).sum(dim=(1, 2)) / cnt), nan),
            "ms_shift_db": torch.where(pairs > 0, d.sum(dim=(1, 2)) / cnt, nan), "pairs": pairs}


@torch.inference_mode()
def modulation_spectrum_distance(mel_a, mel_b, len_a=None, len_b=None, n_coeffs: int = 13, sr: int = 22050, hop_length: int = 256,
                                 min_run: Optional[int] = None, min_cycles: float = MODULATION_MIN_CYCLES):
    """How much trajectory detail the second of two log-mels (B, n_mels, Ta) and (B, n_mels, Tb) lacks (Takamichi et al. 2016): the modulation
    spectra of ``mel_cepstrum``'s coefficients 1 .. ``n_coeffs`` over 1-32 Hz at 0.25 Hz, compared in dB.  The spectrum lives on a fixed grid
    and does not move with a shift in time, so the two need no alignment and may differ in length (recorded against synthesised).
    ``len_a`` / ``len_b`` (B,): frames per row (None: all).  -> {"ms_distortion_db" (B,) float64: the rms over (coefficient, frequency resolved
    on both sides, with a power above 0) of 10 log10 Pm_b - 10 log10 Pm_a; "ms_shift_db": their signed mean, negative when the second input is
    the smoother; "pairs" (B,) int64: the terms behind them; both figures NaN where no frequency is resolved on both sides}."""
    if mel_a.dim() != 3 or mel_b.dim() != 3 or mel_a.shape[:2] != mel_b.shape[:2]:
        raise ValueError(f"modulation_spectrum_distance: two log-mels (B, n_mels, T) of one batch expected, got {tuple(mel_a.shape)} and {tuple(mel_b.shape)}")
    return cepstral_modulation_distance(mel_cepstrum(mel_a, n_coeffs), mel_cepstrum(mel_b, n_coeffs), len_a, len_b, sr, hop_length, min_run, min_cycles)


# ---- time stretching and pitch shifting: the phase vocoder (librosa.effects.time_stretch / pitch_shift are the model) ---------------------------
PHASE_VOCODER_SCRATCH_BYTES = 4 << 30              # ``ev_phase_vocoder``'s limit on the scratch of one call: ``time_stretch`` splits the batch below it
PITCH_RATIO_MAX_DENOMINATOR = 320                  # p / q ~ 2^(n_steps / 12) with q <= 320 and |n_steps| <= 12: p, q <= 640, ``ev_load_resampler``'s limit


def phase_vocoder_window(n_fft: int) -> np.ndarray:
    """The periodic Hann window of librosa.stft's default (scipy's get_window("hann", n_fft, fftbins=True)), float64."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(int(n_fft), dtype=np.float64) / int(n_fft))


def phase_vocoder_arguments(rate, n_fft) -> Tuple[float, int]:
    """The checks of ``time_stretch``: rate finite with 0.125 <= rate <= 8, n_fft a multiple of 16 with 16 <= n_fft <= 2048 -> (rate, n_fft)."""
    if isinstance(rate, bool) or not isinstance(rate, (int, float, np.floating, np.integer)) or not math.isfinite(float(rate)) \
            or not 0.125 <= float(rate) <= 8.0:
        raise ValueError(f"time_stretch: rate must be a finite number with 0.125 <= rate <= 8 (got {rate!r})")
    if int(n_fft) != n_fft or int(n_fft) < 16 or int(n_fft) > 2048 or int(n_fft) % 16:
        raise ValueError(f"time_stretch: n_fft must be a multiple of 16 with 16 <= n_fft <= 2048 (got {n_fft!r})")
    return float(rate), int(n_fft)


def phase_vocoder_scratch_bytes(B: int, L: int, rate: float, n_fft: int) -> int:
    """What ``ev_phase_vocoder`` needs for B rows of L samples without d_stretch: magnitudes, angles and the stretched spectra, float64."""
    NF, NB = 1 + int(L) // (int(n_fft) // 4), int(n_fft) // 2 + 1
    NO = int(np.ceil(np.float64(NF) / np.float64(rate)))
    return 8 * int(B) * NB * (2 * NF + 2 * NO)


def _phase_vocoder_engine(device: torch.device, n_fft: int) -> Engine:
    return _cached_engine(device, ("phase_vocoder", int(n_fft)), lambda eng: eng.load_phase_vocoder(phase_vocoder_window(n_fft), stoi_twiddle(n_fft), n_fft))


def _device_time_stretch_rows(x, lengths, rate, n_fft):
    y, out_len, _, _ = _phase_vocoder_engine(x.device, n_fft).phase_vocoder(x, lengths, rate)
    return y, out_len


@torch.inference_mode()
def time_stretch(y, rate: float, lengths=None, n_fft: int = 1024, rows: Optional[Callable] = None):
    """``y`` 1-D or (B, L) on the GPU rendered ``rate`` times faster (``rate`` > 1) or slower (< 1) at its own pitch, by the phase vocoder on the
    device (``ev_phase_vocoder``; no torch fallback): what ``librosa.effects.time_stretch(y, rate=rate, n_fft=n_fft)`` computes with librosa
    0.10's defaults (hop n_fft / 4, periodic Hann, centred frames over zero padding), as include/emojivoice.h defines it, in float64, rounded
    once to float32.  ``lengths`` (B,): samples per row of a padded batch or None.  -> (y_out (B, rint(L / rate)) float32, zeros from a row's own
    end on; out_lengths (B,) int64 on the host: rint(len / rate), 0 for a row with len < 1 or len > L).  A 1-D input gives B = 1.  The tables and
    the native handle are cached per (device, n_fft); a batch whose scratch would pass 4 GiB is processed in row groups below it.
    ``rows``: the per-batch call, (x, lengths, rate, n_fft) -> (y, out_len) — the device call unless given."""
    rate, n_fft = phase_vocoder_arguments(rate, n_fft)
    if not torch.is_tensor(y) or y.dim() not in (1, 2):
        raise ValueError("time_stretch: y must be a tensor, 1-D or (B, L)")
    if y.shape[-1] < 1:
        raise ValueError("time_stretch: the signal is empty")
    if rows is None and not y.is_cuda:
        raise EvLibraryError("time_stretch runs on a ROCm GPU only (no CPU fallback): move y to the GPU")
    x = y.unsqueeze(0) if y.dim() == 1 else y
    B, L = x.shape
    ln = None
    if lengths is not None:
        ln = torch.as_tensor(lengths).to(torch.int64).reshape(-1).cpu()
        if ln.numel() != B:
            raise ValueError(f"time_stretch: {B} lengths expected, got {ln.numel()}")
    L_out = int(np.rint(np.float64(L) / np.float64(rate)))
    if L_out < 1:                                                        # (a row of under five samples at rate 8)
        return torch.zeros((B, 0), dtype=torch.float32, device=x.device), torch.zeros(B, dtype=torch.int64)
    per_row = phase_vocoder_scratch_bytes(1, L, rate, n_fft)
    if per_row > PHASE_VOCODER_SCRATCH_BYTES:
        raise ValueError(f"time_stretch: one row of {L} samples needs {per_row} bytes of scratch, over 4 GiB: cut the recording")
    group = max(1, min(B, 65535, PHASE_VOCODER_SCRATCH_BYTES // per_row))
    call = rows or _device_time_stretch_rows
    ys, ns = [], []
    for b0 in range(0, B, group):
        yo, no = call(x[b0:b0 + group], None if ln is None else ln[b0:b0 + group], rate, n_fft)
        ys.append(yo)
        ns.append(torch.as_tensor(no).to(torch.int64).cpu())
    return (ys[0] if len(ys) == 1 else torch.cat(ys, dim=0)), torch.cat(ns)


def pitch_ratio(n_steps: float):
    """The frequency ratio of a shift by ``n_steps`` semitones as a fraction p / q ~ 2^(n_steps / 12) with q <= 320
    (``Fraction.limit_denominator``), for |n_steps| <= 12: both terms are at most 640, the resampler's limit.  +1: 196 / 185 (0.006 cents off)."""
    from fractions import Fraction

    if isinstance(n_steps, bool) or not isinstance(n_steps, (int, float, np.floating, np.integer)) or not math.isfinite(float(n_steps)) \
            or abs(float(n_steps)) > 12:
        raise ValueError(f"pitch_shift: n_steps must be a finite number with |n_steps| <= 12 (got {n_steps!r})")
    return Fraction(2.0 ** (float(n_steps) / 12.0)).limit_denominator(PITCH_RATIO_MAX_DENOMINATOR)


def pitch_cents(ratio) -> float:
    """1200 log2(p / q): the shift a ratio realises, in cents."""
    return 1200.0 * math.log2(ratio.numerator / ratio.denominator)


@torch.inference_mode()
def pitch_shift(y, n_steps: float, sr: int = 22050, lengths=None, n_fft: int = 1024, rows: Optional[Callable] = None,
                resampler: Optional[Callable] = None):
    """``y`` 1-D or (B, L) on the GPU, ``n_steps`` semitones higher (> 0) or lower at its own duration, as librosa.effects.pitch_shift does it:
    ``time_stretch`` at rate q / p, then ``resample`` with up = q, down = p, p / q = ``pitch_ratio(n_steps)``; every row is then cut or
    zero-padded to its input length (samples from ``lengths[b]`` on are zeros).  ``sr`` does not enter the arithmetic (the ratio is all the
    resampler needs); it is kept for the model's signature.  -> (y_out (B, L) float32, cents: the shift realised, 1200 log2(p / q)).
    ``n_steps == 0`` returns a copy.  ``rows``: ``time_stretch``'s hook; ``resampler``: (y, q, p, lengths) -> y at q / p times the rate — the
    device resampler unless given."""
    ratio = pitch_ratio(n_steps)
    phase_vocoder_arguments(1.0, n_fft)
    if not torch.is_tensor(y) or y.dim() not in (1, 2):
        raise ValueError("pitch_shift: y must be a tensor, 1-D or (B, L)")
    if int(sr) != sr or int(sr) < 1:
        raise ValueError(f"pitch_shift: sr must be a positive integer (got {sr})")
    x = y.unsqueeze(0) if y.dim() == 1 else y
    B, L = x.shape
    ln = torch.full((B,), L, dtype=torch.int64) if lengths is None else torch.as_tensor(lengths).to(torch.int64).reshape(-1).cpu()
    if ln.numel() != B:
        raise ValueError(f"pitch_shift: {B} lengths expected, got {ln.numel()}")
    p, q = ratio.numerator, ratio.denominator
    if p == q:
        return x.to(torch.float32).clone(), 0.0
    st, st_len = time_stretch(x, q / p, ln, n_fft, rows)
    rs = resampler(st, q, p, st_len) if resampler is not None else resample(st, p, q, lengths=st_len)
    out = torch.zeros((B, L), dtype=torch.float32, device=rs.device)
    keep = min(L, rs.shape[-1])
    out[:, :keep] = rs[:, :keep]
    valid = torch.where((ln >= 1) & (ln <= L), ln, torch.zeros_like(ln)).to(out.device)
    out = out * (torch.arange(L, device=out.device)[None, :] < valid[:, None])
    return out, pitch_cents(ratio)
