"""Counterpart of the ``matcha-tts`` CLI (reference Matcha-TTS/matcha/cli.py:160-250) for the MI355X path
(SURVEY §8 f-2).  The phonemiser front end (espeak-ng) is out of scope, so utterances are given as phoneme-id
sequences (``--ids "12 0 45 ..."`` or ``--file`` with one sequence per line, optional ``|speaker`` suffix like
cli.py:332-336) or as pre-phonemised IPA text (``--phonemes "həlˈoʊ wˈɜːld"``, mapped through the reference's symbol table,
emojivoice_amd/text.py); everything after that point mirrors the reference: validate_args (:138-158), load_matcha / load_vocoder
(:84-118), unbatched / batched synthesis (:277-317, :389-425), ``to_waveform`` (:121-126), PCM_24 wav files (:134).

    python -m emojivoice_amd.cli --checkpoint_path model.ckpt --vocoder_path g_02500000 --ids "0 23 0 51 0" --spk 12
    python -m emojivoice_amd.cli --synthetic --emoji-text "Hello world 🙂" --ids "0 23 0 51 0"
    python -m emojivoice_amd.cli --mel_from_wav voice.wav [--vocoder_path g_02500000 | --synthetic]     # analysis: voice.wav.mel.npy (+ copy synthesis)
    python -m emojivoice_amd.cli --checkpoint_path model.ckpt --align_wav voice.wav --phonemes "həlˈoʊ" --spk 12   # voice.wav.durations.npy
    python -m emojivoice_amd.cli --checkpoint_path model.ckpt --align_wav voice.wav --phonemes "həlˈoʊ" --spk 12 --losses   # + voice.wav.losses.json
    python -m emojivoice_amd.cli --data_statistics train.txt --batch_size 32                            # train.txt.stats.json: mel_mean / mel_std
    python -m emojivoice_amd.cli --synthetic --ids "0 23 0 51 0" --sample_rate 44100                    # wavs at 44.1 kHz
    python -m emojivoice_amd.cli --prepare_dataset raw.txt --out_dir clean                              # trimmed, levelled 22.05 kHz wavs + clean/filelist.txt + raw.txt.durations.json
    python -m emojivoice_amd.cli --prosody_report clean/filelist.txt                                    # clean/filelist.txt.prosody.json: f0 per file and per speaker
    python -m emojivoice_amd.cli --evaluate_pairs pairs.txt                                             # pairs.txt.eval.json: MCD, f0 RMSE, voicing error per 'recorded.wav|synthesised.wav[|spk]'
    python -m emojivoice_amd.cli --voice_report clean/filelist.txt                                      # clean/filelist.txt.voice.json: CPP, alpha ratio, Hammarberg index, spectral slopes per file and per speaker
    python -m emojivoice_amd.cli --voice_report clean/filelist.txt --formants                           # ... and F1-F3 with their bandwidths (Burg's linear prediction at 11025 Hz), per file and per speaker
    python -m emojivoice_amd.cli --voice_report clean/filelist.txt --formants --track_formants          # ... with F1-F3 tracked across frames through five candidates per frame (a Viterbi pass per file) instead of the three lowest
    python -m emojivoice_amd.cli --evaluate_pairs pairs.txt --formants                                  # ... and, per pair, the mean F1-F3 / B1-B3 of both sides and their differences
    python -m emojivoice_amd.cli --voice_report clean/filelist.txt --perturbation                       # ... and jitter, RAP, shimmer and HNR over the voiced frames, per file and per speaker
    python -m emojivoice_amd.cli --evaluate_pairs pairs.txt --perturbation                              # ... and, per pair, jitter, RAP, shimmer and HNR of both sides and their differences
    python -m emojivoice_amd.cli --voice_report clean/filelist.txt --harmonics                          # ... and H1-H2, H1-A3 and the harmonic levels at F1-F3 over H1, per file and per speaker
    python -m emojivoice_amd.cli --voice_report clean/filelist.txt --functionals                        # ... and per contour mean, sd, percentiles, slopes and peak rate, and the voiced / unvoiced segment lengths (the eGeMAPS functionals)
    python -m emojivoice_amd.cli --evaluate_pairs pairs.txt --harmonics                                 # ... and, per pair, the harmonic differences of both sides and their differences
    python -m emojivoice_amd.cli --voice_report clean/filelist.txt --auditory --functionals             # ... and loudness, spectral flux, MFCC 1-4 and the equivalent level, per file and per speaker, with their functionals (loudness peaks per second among them)
    python -m emojivoice_amd.cli --voice_report clean/filelist.txt --modulation                         # ... and rate, extent and prominence of the tremor / vibrato of f0 and of the loudness and of the syllable rhythm, from the modulation spectra of the two contours
    python -m emojivoice_amd.cli --evaluate_pairs pairs.txt --modulation                                # ... the same of both sides with their differences, and the modulation-spectrum distance of the mel-cepstral trajectories (over-smoothing)
    python -m emojivoice_amd.cli --evaluate_pairs pairs.txt --auditory                                  # ... and, per pair, loudness, spectral flux, MFCC 1-4 and the level of both sides and their differences
    python -m emojivoice_amd.cli --evaluate_pairs pairs.txt --voice_quality                             # ... and, per pair, the voice-quality figures of both sides and their differences
    python -m emojivoice_amd.cli --loudness_report clean/filelist.txt                                   # clean/filelist.txt.loudness.json: BS.1770 LUFS per file and per speaker
    python -m emojivoice_amd.cli --reverb_report clean/filelist.txt                                     # clean/filelist.txt.srmr.json: SRMR (reverberation, no clean reference needed) per file and per speaker
    python -m emojivoice_amd.cli --evaluate_pairs pairs.txt --srmr                                      # ... and, per pair, the SRMR of both sides and their difference
    python -m emojivoice_amd.cli --prosody_report clean/filelist.txt --rhythm                           # ... and, per file and per speaker, speech rate, articulation rate, pauses and phonation ratio (syllable nuclei)
    python -m emojivoice_amd.cli --evaluate_pairs pairs.txt --rhythm                                    # ... and, per pair, rate and pauses of both sides and their differences
    python -m emojivoice_amd.cli --evaluate_pairs pairs.txt --envelope_mcd                              # ... and, per pair, the MCD of the mel-cepstra of CheapTrick's spectral envelope (the literature's kind of MCD)
    python -m emojivoice_amd.cli --prepare_dataset raw.txt --out_dir clean --target_lufs -23            # levelled by loudness instead of by peak
    python -m emojivoice_amd.cli --augment_dataset clean/filelist.txt --out_dir aug --rates 0.9,1.1 --semitones -1,1   # slower / faster / lower / higher copies + aug/filelist.txt + FILELIST.augment.json
    python -m emojivoice_amd.cli --vocoder_report clean/filelist.txt --vocoder_path g_02500000          # clean/filelist.txt.vocoder.json: STOI / ESTOI, mel L1 and loudness shift of copy synthesis
    python -m emojivoice_amd.cli --vocoder_report clean/filelist.txt --vocoder_path g_02500000 --spectral_distance   # + multi-resolution STFT distance and log-spectral distance

The wavs of --mel_from_wav, --align_wav and --data_statistics may have any sample rate (the reference's recorder writes 44.1 kHz,
record_audio.py:31): they are resampled to the analysis rate on the device (emojivoice_amd.audio.resample).
"""
from __future__ import annotations

import argparse
import collections
import datetime as dt
import json
import math
import os
import struct
import sys
import warnings
from pathlib import Path

import numpy as np
import torch


from .text import cleaned_text_to_sequence, intersperse  # noqa: E402  (utils/utils.py:131-135, text/__init__.py:27-35)


def write_wav_pcm24(path, wav: np.ndarray, sr: int = 22050):
    """soundfile.write(..., 'PCM_24') equivalent (cli.py:134) with the stdlib only."""
    x = np.clip(np.asarray(wav, dtype=np.float64), -1.0, 1.0)
    q = np.round(x * (2**23 - 1)).astype(np.int32)
    b = (q & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(b)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, sr, sr * 3, 3, 24))
        f.write(b"data" + struct.pack("<I", len(b)) + b)


def write_wav_pcm16(path, wav: np.ndarray, sr: int = 22050):
    """A 16-bit mono PCM wav (the format of the reference's recorder, record_audio.py) with the stdlib only: round(x * 32767) after
    clipping to [-1, 1], the 24-bit writer's rule."""
    x = np.clip(np.asarray(wav, dtype=np.float64), -1.0, 1.0)
    b = np.round(x * 32767.0).astype("<i2").tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(b)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, sr, sr * 2, 2, 16))
        f.write(b"data" + struct.pack("<I", len(b)) + b)


def validate_args(args):
    if getattr(args, "spectral_distance", False):
        assert getattr(args, "vocoder_report", None), "--spectral_distance is an option of --vocoder_report"
    for family in report_families():
        if getattr(args, family.pairs_flag, False):
            homes = (["voice_report"] if family.report_flag else []) + ["evaluate_pairs"]
            assert any(getattr(args, h, None) for h in homes), f"--{family.pairs_flag} is an option of " + " and of ".join("--" + h for h in homes)
    if getattr(args, "functionals", False):
        assert getattr(args, "voice_report", None), "--functionals is an option of --voice_report"
    if getattr(args, "modulation", False):
        assert getattr(args, "voice_report", None) or getattr(args, "evaluate_pairs", None), \
            "--modulation is an option of --voice_report and of --evaluate_pairs"
    if getattr(args, "rhythm", False):
        assert getattr(args, "prosody_report", None) or getattr(args, "evaluate_pairs", None), \
            "--rhythm is an option of --prosody_report and of --evaluate_pairs"
    if getattr(args, "envelope_mcd", False):
        assert getattr(args, "evaluate_pairs", None), "--envelope_mcd is an option of --evaluate_pairs"
    if getattr(args, "track_formants", False):
        assert (getattr(args, "voice_report", None) or getattr(args, "evaluate_pairs", None)) and (getattr(args, "formants", False) or getattr(args, "harmonics", False)), \
            "--track_formants is an option of --formants and of --harmonics under --voice_report and --evaluate_pairs"
    if args.sample_rate is not None:
        assert args.sample_rate > 0, "--sample_rate must be positive"
    if getattr(args, "augment_dataset", None):
        assert args.out_dir, "--augment_dataset needs --out_dir"
        assert args.batch_size > 0, "Batch size must be greater than 0"
        args.rates, args.semitones = augment_values(args.rates, "--rates"), augment_values(args.semitones, "--semitones")
        assert args.rates or args.semitones, "--augment_dataset needs at least one of --rates and --semitones"
        assert all(0.125 <= r <= 8.0 and r != 1.0 for r in args.rates), "--rates must lie in [0.125, 8] and differ from 1"
        assert all(abs(v) <= 12 and v != 0 for v in args.semitones), "--semitones must lie in [-12, 12] and differ from 0"
        return args
    if args.prepare_dataset:
        assert args.out_dir, "--prepare_dataset needs --out_dir"
        assert 0 <= args.peak <= 1, "--peak must lie in [0, 1] (0: no levelling)"
        if getattr(args, "target_lufs", None) is not None:
            assert math.isfinite(args.target_lufs), "--target_lufs must be a finite LUFS value"
            assert args.peak > 0, "--target_lufs caps the gain at --peak: --peak must lie in (0, 1]"
            sr = int(args.sample_rate or 22050)
            assert sr % 10 == 0 and sr >= 8000, "--target_lufs needs a --sample_rate that is a multiple of 10 and at least 8000"
        return args
    if (getattr(args, "prosody_report", None) or getattr(args, "evaluate_pairs", None) or getattr(args, "loudness_report", None) or getattr(args, "voice_report", None)
            or getattr(args, "reverb_report", None)):
        assert args.batch_size > 0, "Batch size must be greater than 0"
        return args
    if getattr(args, "vocoder_report", None):
        assert args.batch_size > 0, "Batch size must be greater than 0"
        assert args.synthetic or args.vocoder_path, "--vocoder_report needs --vocoder_path (or --synthetic)"
        return args
    if args.mel_from_wav:
        return args
    if args.data_statistics:
        assert args.batch_size > 0, "Batch size must be greater than 0"
        return args
    if args.align_mel or args.align_wav:
        assert not (args.align_mel and args.align_wav), "--align_mel and --align_wav exclude each other"
        assert args.ids or args.phonemes, "--align_mel / --align_wav need the text of that one utterance: --ids or --phonemes"
        assert args.synthetic or args.checkpoint_path, "--checkpoint_path is required (or --synthetic)"
        return args
    assert args.ids or args.file or args.phonemes, "One of --ids, --phonemes or --file must be provided"
    assert args.temperature >= 0, "Sampling temperature cannot be negative"
    assert args.steps > 0, "Number of ODE steps must be greater than 0"
    if args.speaking_rate is None:
        args.speaking_rate = 1.0
    if args.batched:
        assert args.batch_size > 0, "Batch size must be greater than 0"
    assert args.speaking_rate > 0, "Speaking rate must be greater than 0"
    return args


def load_models(args, device):
    from . import weights as W
    from .denoiser import Denoiser
    from .hifigan import AttrDict, Generator
    from .matcha_tts import MatchaTTS

    h = AttrDict(vocoder_config(args.vocoder_config))
    if args.synthetic:
        model = MatchaTTS(W.synthetic_matcha_state(), device=device)
        voc_sd = W.synthetic_hifigan_state(h)
    else:
        model = MatchaTTS.load_from_checkpoint(args.checkpoint_path, map_location=device)
        voc_sd = torch.load(args.vocoder_path, map_location="cpu")["generator"]
    vocoder = Generator(h).to(device)
    vocoder.load_state_dict(voc_sd)
    vocoder.eval()
    vocoder.remove_weight_norm()
    denoiser = Denoiser(vocoder, mode="zeros") if args.denoiser_strength > 0 else None
    return model.eval(), vocoder, denoiser


def vocoder_config(name: str) -> dict:
    """--vocoder_config: v1 / v2 / v3, or the path of an upstream HiFi-GAN config.json."""
    import json

    from . import hifigan

    if name in ("v1", "v2", "v3"):
        return dict(getattr(hifigan, name))
    with open(name, encoding="utf-8") as f:
        h = json.load(f)
    hifigan.check_config(h)
    return h


@torch.inference_mode()
def to_waveform(mel, vocoder, denoiser=None, strength=0.00025):
    audio = vocoder(mel).clamp(-1, 1)
    if denoiser is not None:
        audio = denoiser(audio.squeeze(), strength=strength).cpu().squeeze()
    return audio.cpu().squeeze()


def parse_lines(args):
    if args.phonemes is not None:
        # pre-phonemised (IPA) text -> ids exactly as process_text does after its cleaner (cli.py:52-56): always with blanks
        return [(intersperse(cleaned_text_to_sequence(args.phonemes), 0), None)]
    lines = [args.ids] if args.ids else open(args.file, encoding="utf-8").read().splitlines()
    out = []
    for ln in lines:
        ln = ln.strip()
        if not ln:
            continue
        spk = None
        if "|" in ln:
            ln, s = ln.rsplit("|", 1)
            spk = int(s)
        if args.file_phonemes:
            ids = intersperse(cleaned_text_to_sequence(ln), 0)
        else:
            ids = [int(t) for t in ln.split()]
            if args.add_blank:
                ids = intersperse(ids, 0)
        out.append((ids, spk))
    return out


def wav_at_rate(path, sr: int, device):
    """The wav at ``path`` (any rate, 16 / 24 bit PCM, channels averaged) as a (1, n) tensor on the device at ``sr``, trimmed to a
    multiple of 256 samples; None when fewer than 512 are left.  Prints the file's rate."""
    from .audio import read_wav, resample

    y, rate = read_wav(path)
    print(f"[i] {path}: {rate} Hz, {len(y)} samples" + ("" if rate == sr else f" -> resampled to {sr} Hz on the device"))
    y = resample(torch.from_numpy(y).to(device).unsqueeze(0), rate, sr)
    n = y.shape[1] // 256 * 256
    return y[:, :n].contiguous() if n > 384 else None


@torch.inference_mode()
def mel_from_wav(args, device):
    """--mel_from_wav: PATH (PCM at any rate, 16 / 24 bit; resampled on the device to the config's rate) -> PATH.mel.npy (80, frames) with the analysis parameters of the
    vocoder config (hifigan/meldataset.py:52 as text_mel_datamodule.py:202 calls it), the signal trimmed to a multiple of 256
    samples; with vocoder weights also PATH.copysyn.wav, the vocoder's rendering of that mel (copy synthesis)."""
    from . import weights as W
    from .audio import mel_spectrogram
    from .hifigan import AttrDict, Generator

    h = AttrDict(vocoder_config(args.vocoder_config))
    y = wav_at_rate(args.mel_from_wav, int(h.get("sampling_rate", 22050)), device)
    if y is None:
        sys.exit(f"[-] {args.mel_from_wav}: at least 512 samples at {int(h.get('sampling_rate', 22050))} Hz are needed")
    n = y.shape[1]
    mel = mel_spectrogram(y, h.get("n_fft", 1024), h.get("num_mels", 80), h.get("sampling_rate", 22050), h.get("hop_size", 256),
                          h.get("win_size", 1024), h.get("fmin", 0), h.get("fmax", 8000))
    out = f"{args.mel_from_wav}.mel.npy"
    np.save(out, mel[0].cpu().numpy())
    print(f"[+] Mel saved: {Path(out).resolve()}  ({mel.shape[-1]} frames, {n / 22050:.2f} s)")
    if not (args.vocoder_path or args.synthetic):
        return
    sd = W.synthetic_hifigan_state(h) if args.synthetic else torch.load(args.vocoder_path, map_location="cpu")["generator"]
    vocoder = Generator(h).to(device)
    vocoder.load_state_dict(sd)
    vocoder.eval()
    vocoder.remove_weight_norm()
    wav = vocoder(mel).clamp(-1, 1).reshape(-1).cpu().numpy()
    out = f"{args.mel_from_wav}.copysyn.wav"
    write_wav_pcm24(out, wav)
    print(f"[+] Copy synthesis saved: {Path(out).resolve()}")


@torch.inference_mode()
def align_durations(args, device):
    """--align_mel MEL.npy (a normalised (80, frames) mel) / --align_wav VOICE.wav (analysed as --mel_from_wav does, normalize() fused)
    with the text of that utterance -> <input>.durations.npy: the Tx integer durations of MatchaTTS.align, what
    utils/get_durations_from_trained_model.py saves per file.  With --losses also <input>.losses.json: the utterance's dur_loss,
    prior_loss and diff_loss of MatchaTTS.score, the time and the noise of the flow-matching loss drawn on the CPU from --seed."""
    from . import weights as W
    from .audio import mel_spectrogram
    from .matcha_tts import MatchaTTS

    model = MatchaTTS(W.synthetic_matcha_state(), device=device) if args.synthetic else MatchaTTS.load_from_checkpoint(args.checkpoint_path, map_location=device)
    src = args.align_mel or args.align_wav
    if args.align_mel:
        mel = torch.from_numpy(np.load(src).astype(np.float32)).to(device).reshape(1, model.n_feats, -1)
    else:
        y = wav_at_rate(src, 22050, device)
        if y is None:
            sys.exit(f"[-] {src}: at least 512 samples at 22050 Hz are needed")
        mel = mel_spectrogram(y, 1024, model.n_feats, 22050, 256, 1024, 0, 8000,
                              out_scale=1.0 / model.mel_std, out_shift=-model.mel_mean / model.mel_std)
    ids, spk = parse_lines(args)[0]
    x = torch.tensor([ids], dtype=torch.long, device=device)
    spks = torch.tensor([spk if spk is not None else (args.spk or 0)], dtype=torch.long, device=device)
    x_len, y_len = torch.tensor([len(ids)], device=device), torch.tensor([mel.shape[-1]], device=device)
    if args.losses:
        t, z = loss_draws(args.seed, model.n_feats, mel.shape[-1])
        out = model.score(x, x_len, mel, y_len, spks, t=t, z=z)
    else:
        out = model.align(x, x_len, mel, y_len, spks)
    dur = out["durations"][0].cpu().numpy()
    np.save(f"{src}.durations.npy", dur)
    print(f"[+] Durations saved: {Path(f'{src}.durations.npy').resolve()}  ({len(dur)} tokens over {mel.shape[-1]} frames)")
    if args.losses:
        rec = {k: float(out[k][0]) for k in ("dur_loss", "prior_loss", "diff_loss")}
        rec.update(seed=int(args.seed), t=float(t[0]), tokens=len(ids), frames=int(mel.shape[-1]))
        with open(f"{src}.losses.json", "w") as f:
            json.dump(rec, f, indent=1)
        print(f"[+] Losses saved: {Path(f'{src}.losses.json').resolve()}  (dur {rec['dur_loss']:.4f}  prior {rec['prior_loss']:.4f}  diff {rec['diff_loss']:.4f})")


@torch.inference_mode()
def data_statistics(args, device):
    """--data_statistics FILELIST: the first '|'-separated field of each line is a wav path, as in the reference's filelists
    (data/text_mel_datamodule.py:96-99; relative paths are taken from the filelist's folder when they do not exist as given).  The
    mels are those of --mel_from_wav, reduced --batch_size files at a time (padded to the longest); FILELIST.stats.json receives
    {"mel_mean", "mel_std"}, the content utils/generate_data_statistics.py writes."""
    from . import audio
    from .hifigan import AttrDict

    h = AttrDict(vocoder_config(args.vocoder_config))
    sr, n_mels = int(h.get("sampling_rate", 22050)), int(h.get("num_mels", 80))
    flist = Path(args.data_statistics)
    paths = [ln.split("|")[0].strip() for ln in flist.read_text(encoding="utf-8").splitlines() if ln.strip()]
    paths = [p if os.path.exists(p) else str(flist.parent / p) for p in paths]
    if not paths:
        sys.exit(f"[-] {flist}: no files listed")

    def batches():
        for b0 in range(0, len(paths), args.batch_size):
            wavs = [wav_at_rate(p, sr, device) for p in paths[b0:b0 + args.batch_size]]
            wavs = [w for w in wavs if w is not None]             # (files under 512 samples give no frame)
            if not wavs:
                continue
            mels = [audio.mel_spectrogram(w, h.get("n_fft", 1024), n_mels, sr, h.get("hop_size", 256), h.get("win_size", 1024), h.get("fmin", 0),
                                          h.get("fmax", 8000)) for w in wavs]     # per file: each signal's own reflect padding
            mel = torch.zeros(len(mels), n_mels, max(m.shape[2] for m in mels), device=device)
            for r, m in enumerate(mels):
                mel[r, :, : m.shape[2]] = m[0]
            yield mel, torch.tensor([m.shape[2] for m in mels])

    stats = audio.data_statistics(batches(), n_mels)
    out = f"{flist}.stats.json"
    with open(out, "w") as f:
        json.dump(stats, f)
    print(f"[+] Data statistics saved: {Path(out).resolve()}  ({len(paths)} files: mel_mean {stats['mel_mean']:.6f}  mel_std {stats['mel_std']:.6f})")


TWO_MINUTES = 2.0    # minutes of audio per emoji the reference's README names as the least that fine-tunes a voice


def parse_filelist(path):
    """The lines of a reference filelist (data/text_mel_datamodule.py:96-99) as (wav path, speaker id as written or None, the
    fields after the path): 'path|spk|text' or 'path|text'.  Relative paths that do not exist as given are taken from the filelist's
    folder; empty lines are skipped."""
    flist = Path(path)
    out = []
    for ln in flist.read_text(encoding="utf-8").splitlines():
        if not ln.strip():
            continue
        fields = ln.split("|")
        wav = fields[0].strip()
        if not os.path.exists(wav) and (flist.parent / wav).exists():
            wav = str(flist.parent / wav)
        spk = fields[1].strip() if len(fields) >= 3 else None
        out.append((wav, spk, fields[1:]))
    return out


def duration_report(files, sr: int, top_db: float, peak: float):
    """The content of FILELIST.durations.json: per file the seconds before and after trimming, per speaker id the minutes after
    trimming (what get_duration.ipynb adds up), and the speakers below two minutes.  ``files``: dicts with path, out, speaker,
    seconds_in, seconds_out.  A filelist without a speaker column counts as speaker "0"."""
    speakers = {}
    for f in files:
        s = speakers.setdefault(f["speaker"], {"files": 0, "seconds": []})
        s["files"] += 1
        s["seconds"].append(f["seconds_out"])
    per_spk = {k: {"files": v["files"], "minutes": math.fsum(v["seconds"]) / 60.0} for k, v in speakers.items()}
    for v in per_spk.values():
        v["below_two_minutes"] = v["minutes"] < TWO_MINUTES
    return {"sample_rate": sr, "top_db": top_db, "peak": peak, "files": files, "speakers": per_spk,
            "below_two_minutes": sorted(k for k, v in per_spk.items() if v["below_two_minutes"]),
            "total_minutes_in": math.fsum(f["seconds_in"] for f in files) / 60.0,
            "total_minutes_out": math.fsum(f["seconds_out"] for f in files) / 60.0}


def prepare_dataset(args, device):
    """--prepare_dataset FILELIST --out_dir DIR: every listed recording (any rate, channel count, 16 / 24 bit) through
    audio.prepare_recording (resampled to --sample_rate, silence trimmed at --top_db, levelled to --peak, all on the device), written
    as a 16-bit mono wav of the same base name under DIR; DIR/filelist.txt repeats the lines with the new paths and
    FILELIST.durations.json holds ``duration_report``.  With --target_lufs X the level comes from loudness instead of from the peak: the take is
    trimmed with its level untouched, then audio.loudness_normalize takes it to X LUFS (BS.1770), the gain capped where the peak would pass
    --peak; every file's entry then also holds "integrated_lufs" (before levelling; null without a loudness), "gain_db" and "capped", and the
    report "target_lufs"."""
    from . import audio

    target = getattr(args, "target_lufs", None)

    sr = int(args.sample_rate or 22050)
    entries = parse_filelist(args.prepare_dataset)
    if not entries:
        sys.exit(f"[-] {args.prepare_dataset}: no files listed")
    names = [Path(wav).stem + ".wav" for wav, _, _ in entries]
    if len(set(names)) != len(names):
        sys.exit(f"[-] {args.prepare_dataset}: two recordings share a base name; they would overwrite each other under {args.out_dir}")
    out_dir = Path(args.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    files, lines = [], []
    for (wav, spk, rest), name in zip(entries, names):
        level = {}
        if target is None:
            y, info = audio.prepare_recording(wav, sr, args.top_db, args.peak, device)
        else:
            y, info = audio.prepare_recording(wav, sr, args.top_db, 0.0, device)
            before = audio.loudness(y, sr)["integrated"]
            y, gain_db, capped = audio.loudness_normalize(y, target, sr, peak_ceiling=args.peak)
            level = {"integrated_lufs": float(before[0]) if math.isfinite(float(before[0])) else None, "gain_db": float(gain_db[0]), "capped": bool(capped[0])}
        dst = (out_dir / name).resolve()
        write_wav_pcm16(dst, y.cpu().numpy(), sr)
        files.append({"path": wav, "out": str(dst), "speaker": spk if spk is not None else "0",
                      "seconds_in": info["seconds_in"], "seconds_out": info["seconds_out"], **level})
        lines.append("|".join([str(dst)] + rest))
        print(f"[+] {wav}: {info['seconds_in']:.2f} s -> {info['seconds_out']:.2f} s  ({dst})"
              + (f"  gain {level['gain_db']:+.2f} dB" + ("  (capped at the peak)" if level["capped"] else "") if level else ""))
    (out_dir / "filelist.txt").write_text("\n".join(lines) + "\n", encoding="utf-8")
    rep = duration_report(files, sr, args.top_db, args.peak)
    if target is not None:
        rep["target_lufs"] = float(target)
    out = f"{args.prepare_dataset}.durations.json"
    with open(out, "w") as f:
        json.dump(rep, f, indent=1)
    for k in sorted(rep["speakers"]):
        v = rep["speakers"][k]
        print(f"[i] speaker {k}: {v['files']} files, {v['minutes']:.2f} min" + ("  (below two minutes)" if v["below_two_minutes"] else ""))
    print(f"[+] File list saved: {(out_dir / 'filelist.txt').resolve()}\n[+] Durations saved: {Path(out).resolve()}")
    return rep


def augment_values(text, flag: str):
    """The finite numbers of a comma-separated option (a list passes through; None or "": none)."""
    if text is None or isinstance(text, (list, tuple)):
        return [float(v) for v in (text or [])]
    try:
        vals = [float(v) for v in str(text).split(",") if v.strip()]
    except ValueError:
        raise AssertionError(f"{flag} takes comma-separated numbers (got {text!r})") from None
    assert all(math.isfinite(v) for v in vals), f"{flag} takes finite numbers (got {text!r})"
    return vals


def augment_report(files, sr: int, rates, semitones, cents):
    """The content of FILELIST.augment.json: per speaker the seconds before (the listed files) and after (with every variant), whether the speaker
    is still below two minutes, and per shift the cents realised.  ``files``: dicts with path, speaker, seconds and variants [{out, kind, value,
    seconds}]."""
    speakers = {}
    for f in files:
        s = speakers.setdefault(f["speaker"], {"files": 0, "variants": 0, "before": [], "after": []})
        s["files"] += 1
        s["variants"] += len(f["variants"])
        s["before"].append(f["seconds"])
        s["after"].extend([f["seconds"]] + [v["seconds"] for v in f["variants"]])
    per_spk = {}
    for k, v in speakers.items():
        before, after = math.fsum(v["before"]), math.fsum(v["after"])
        per_spk[k] = {"files": v["files"], "variants": v["variants"], "seconds_before": before, "seconds_after": after,
                      "below_two_minutes_before": before / 60.0 < TWO_MINUTES, "below_two_minutes": after / 60.0 < TWO_MINUTES}
    return {"sample_rate": sr, "rates": list(rates), "semitones": list(semitones), "realised_cents": {f"{v:+.2f}": c for v, c in zip(semitones, cents)},
            "files": files, "speakers": per_spk, "below_two_minutes": sorted(k for k, v in per_spk.items() if v["below_two_minutes"])}


def augment_dataset(args, device, rows=None, resampler=None):
    """--augment_dataset FILELIST --out_dir DIR [--rates 0.9,1.1] [--semitones -1,1]: every recording of the filelist --prepare_dataset writes,
    rendered once per rate (audio.time_stretch: slower below 1, faster above) and once per shift (audio.pitch_shift) — no cross product —
    --batch_size files at a time on the device (padded to the longest, each row with its own length).  DIR/<base>_r0.90.wav and
    DIR/<base>_p+1.00.wav are 16-bit mono wavs; DIR/filelist.txt holds the original lines followed by the variants with the same speaker and
    text; FILELIST.augment.json holds ``augment_report``.  ``rows`` / ``resampler``: the hooks of audio.time_stretch and audio.pitch_shift."""
    from . import audio

    sr = int(args.sample_rate or PROSODY_SR)
    entries = parse_filelist(args.augment_dataset)
    if not entries:
        sys.exit(f"[-] {args.augment_dataset}: no files listed")
    stems = [Path(wav).stem for wav, _, _ in entries]
    if len(set(stems)) != len(stems):
        sys.exit(f"[-] {args.augment_dataset}: two recordings share a base name; their variants would overwrite each other under {args.out_dir}")
    out_dir = Path(args.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    cents = [audio.pitch_cents(audio.pitch_ratio(v)) for v in args.semitones]
    originals = ["|".join([wav] + rest) for wav, _, rest in entries]
    files, lines, at = [], [], 0
    for chunk, batch, lens in filelist_batches(args.augment_dataset, args.batch_size, sr, device):
        recs = [{"path": wav, "speaker": spk if spk is not None else "0", "seconds": n / sr, "variants": []} for (wav, spk, _), n in zip(chunk, lens)]
        renders = [("rate", r, f"_r{r:.2f}") + audio.time_stretch(batch, r, lens, rows=rows) for r in args.rates]
        for v in args.semitones:
            shifted, _ = audio.pitch_shift(batch, v, sr, lens, rows=rows, resampler=resampler)
            renders.append(("semitones", v, f"_p{v:+.2f}", shifted, lens))
        for kind, value, tag, y, out_lens in renders:
            y = y.cpu().numpy()
            for r, ((wav, _, rest), rec) in enumerate(zip(chunk, recs)):
                n = int(out_lens[r])
                dst = (out_dir / (stems[at + r] + tag + ".wav")).resolve()
                write_wav_pcm16(dst, y[r, :n], sr)
                rec["variants"].append({"out": str(dst), "kind": kind, "value": value, "seconds": n / sr})
                lines.append("|".join([str(dst)] + rest))
        files.extend(recs)
        at += len(chunk)
    (out_dir / "filelist.txt").write_text("\n".join(originals + lines) + "\n", encoding="utf-8")
    rep = augment_report(files, sr, args.rates, args.semitones, cents)
    out = f"{args.augment_dataset}.augment.json"
    with open(out, "w") as f:
        json.dump(rep, f, indent=1)
    for k in sorted(rep["speakers"]):
        v = rep["speakers"][k]
        print(f"[i] speaker {k}: {v['files']} files + {v['variants']} variants, {v['seconds_before'] / 60.0:.2f} -> {v['seconds_after'] / 60.0:.2f} min"
              + ("  (still below two minutes)" if v["below_two_minutes"] else ""))
    print(f"[+] File list saved: {(out_dir / 'filelist.txt').resolve()}\n[+] Report saved: {Path(out).resolve()}")
    return rep


def filelist_batches(path, batch_size: int, sr: int, device):
    """(chunk, batch, lens) per ``batch_size`` entries of ``parse_filelist(path)`` (none: exit): the chunk's files through
    audio.load_audio(path, sr) as one (rows, longest) tensor on the device, zero-padded, and every row's own length in samples."""
    from . import audio

    entries = parse_filelist(path)
    if not entries:
        sys.exit(f"[-] {path}: no files listed")
    for chunk in (entries[b0:b0 + batch_size] for b0 in range(0, len(entries), batch_size)):
        ys = [audio.load_audio(wav, sr, device) for wav, _, _ in chunk]
        lens = [int(y.shape[-1]) for y in ys]
        batch = torch.zeros(len(ys), max(max(lens), 1), device=ys[0].device)
        for r, y in enumerate(ys):
            batch[r, : lens[r]] = y.reshape(-1)
        yield chunk, batch, lens


PROSODY_SR, PROSODY_HOP = 22050, 256    # the analysis rate and the mel's hop: frame f of the contour is mel frame f


def pitch_summary(f0_voiced):
    """{"f0_median", "f0_p05", "f0_p95" (Hz), "f0_range_semitones"} of a 1-D tensor of voiced f0 values (linear-interpolated percentiles);
    None for every field when it is empty."""
    if f0_voiced.numel() == 0:
        return {"f0_median": None, "f0_p05": None, "f0_p95": None, "f0_range_semitones": None}
    p05, med, p95 = (float(v) for v in torch.quantile(f0_voiced.float(), torch.tensor([0.05, 0.5, 0.95], device=f0_voiced.device)))
    return {"f0_median": med, "f0_p05": p05, "f0_p95": p95, "f0_range_semitones": 12.0 * math.log2(p95 / p05)}


def pitch_method(args) -> str:
    return getattr(args, "pitch_method", None) or "yin"


def pitch_tracker(args):
    """--pitch_method: audio.pitch_yin (the default; every frame decided on its own) or audio.pitch_pyin (probabilistic YIN: a Viterbi
    pass over the frames' candidates).  Both return "f0" and "voiced" of the same shapes and dtypes; looked up at call time."""
    from . import audio

    return audio.pitch_pyin if pitch_method(args) == "pyin" else audio.pitch_yin


@torch.inference_mode()
def prosody_report(args, device):
    """--prosody_report FILELIST: the filelist --prepare_dataset writes ('path|spk|text'; 'path|text' counts as speaker "0").  Every file
    is loaded with audio.load_audio(path, 22050) and tracked by audio.pitch_yin (--pitch_method pyin: audio.pitch_pyin, and the report
    gains "pitch_method": "pyin"), --batch_size files at a time (padded to the longest,
    each row with its own length).  FILELIST.prosody.json receives, per file, the numbers of audio.prosody_statistics (voiced fraction,
    f0 median / 5th / 95th percentile in Hz, the 5-to-95 range in semitones; null where a file has no voiced frame) and, per speaker,
    the same over that speaker's POOLED voiced frames, with the file count.
    --rhythm adds per file "rhythm": RHYTHM_REPORT_KEYS of audio.speech_rate (syllable nuclei on the same frames, voiced by the tracker this
    report ran; null for a rate over zero seconds) with "nuclei", and per speaker "rhythm": their plain means over the files that have them
    and "pooled_speech_rate", the speaker's nuclei over the speaker's seconds."""
    from . import audio

    want_rhythm = getattr(args, "rhythm", False)
    files, pooled, frames_of = [], {}, {}
    for chunk, batch, lens in filelist_batches(args.prosody_report, args.batch_size, PROSODY_SR, device):
        out = pitch_tracker(args)(batch, PROSODY_SR, hop_length=PROSODY_HOP, lengths=lens)
        n_frames = [-(-n // PROSODY_HOP) for n in lens]
        st = {k: v.cpu() for k, v in audio.prosody_statistics(out["f0"], out["voiced"], n_frames).items()}
        rhythm = rhythm_rows(audio, args, batch, PROSODY_SR, PROSODY_HOP, lens, out["voiced"]) if want_rhythm else None
        for r, (wav, spk, _) in enumerate(chunk):
            spk = spk if spk is not None else "0"
            rec = {"path": wav, "speaker": spk, "seconds": lens[r] / float(PROSODY_SR), "frames": n_frames[r]}
            for k, v in st.items():
                rec[k] = None if math.isnan(float(v[r])) else float(v[r])
            if want_rhythm:
                rec["rhythm"] = rhythm[r]
            files.append(rec)
            pooled.setdefault(spk, []).append(out["f0"][r, : n_frames[r]][out["voiced"][r, : n_frames[r]]])
            frames_of[spk] = frames_of.get(spk, 0) + n_frames[r]
    speakers = {}
    for spk, parts in pooled.items():
        v = torch.cat(parts)
        speakers[spk] = {"files": len(parts), "voiced_fraction": v.numel() / max(frames_of[spk], 1), **pitch_summary(v)}
        if want_rhythm:
            mine = [f for f in files if f["speaker"] == spk]
            secs = math.fsum(f["frames"] * PROSODY_HOP / float(PROSODY_SR) for f in mine)
            speakers[spk]["rhythm"] = {**rhythm_means([f["rhythm"] for f in mine]),
                                       "pooled_speech_rate": sum(f["rhythm"]["nuclei"] for f in mine) / secs if secs > 0 else None}
    rep = {"sample_rate": PROSODY_SR, "hop_length": PROSODY_HOP, "files": files, "speakers": speakers}
    if pitch_method(args) != "yin":
        rep["pitch_method"] = pitch_method(args)
    out_path = f"{args.prosody_report}.prosody.json"
    with open(out_path, "w") as f:
        json.dump(rep, f, indent=1)
    for k in sorted(speakers):
        v = speakers[k]
        pitch = "no voiced frame" if v["f0_median"] is None else (f"f0 median {v['f0_median']:.1f} Hz, {v['f0_p05']:.1f} .. {v['f0_p95']:.1f} Hz "
                                                                  f"({v['f0_range_semitones']:.1f} semitones)")
        print(f"[i] speaker {k}: {v['files']} files, voiced {100 * v['voiced_fraction']:.0f} %, {pitch}")
    print(f"[+] Prosody report saved: {Path(out_path).resolve()}")
    return rep


RHYTHM_REPORT_KEYS = ("speech_rate", "articulation_rate", "pauses", "pause_mean_s", "phonation_ratio")


def rhythm_rows(audio, args, sig, sr, hop, lens, voiced):
    """Per row of ``sig`` {RHYTHM_REPORT_KEYS ..., "nuclei", "pause_s"} of audio.speech_rate under the tracker's voicing (None for NaN)."""
    out = audio.speech_rate(sig, sr, voiced=voiced, lengths=lens, hop_length=hop, rows=getattr(args, "speech_rate_rows", None))
    cols = {k: torch.as_tensor(out[k]).cpu() for k in RHYTHM_REPORT_KEYS + ("nuclei", "pause_s")}
    val = lambda k, v: int(v) if k in ("pauses", "nuclei") else (None if math.isnan(float(v)) else float(v))
    return [{k: val(k, v[r]) for k, v in cols.items()} for r in range(sig.shape[0])]


def rhythm_means(rows, keys=RHYTHM_REPORT_KEYS):
    """{key: the plain mean over the rows that have it, or None}"""
    out = {}
    for k in keys:
        d = [row[k] for row in rows if row[k] is not None]
        out[k] = math.fsum(d) / len(d) if d else None
    return out


def rhythm_difference(a, b):
    """audio.speech_rate_difference on two report rows: {"rate_ratio" (0.15: the synthesis is 15 % faster), "pauses_delta", "pause_s_delta"}."""
    ok = a["speech_rate"] is not None and a["speech_rate"] > 0 and b["speech_rate"] is not None
    return {"rate_ratio": b["speech_rate"] / a["speech_rate"] - 1.0 if ok else None, "pauses_delta": b["pauses"] - a["pauses"],
            "pause_s_delta": b["pause_s"] - a["pause_s"]}


Family = collections.namedtuple("Family", "report_flag pairs_flag block figures frames_key counts used measure finish", defaults=(None,))


TRACK_CANDIDATES, TRACK_FORMANTS = 5, 3             # --track_formants: candidates per frame from audio.formants, tracks through them


def formant_tracking_parameters():
    """The top-level "formant_tracking" object of a report made with --track_formants: what audio.formant_tracks ran with."""
    from . import audio

    return {"candidates": TRACK_CANDIDATES, "tracks": TRACK_FORMANTS, "reference_hz": list(audio.FORMANT_TRACK_REFERENCE), "frequency_cost": 1.0,
            "bandwidth_cost": 1.0, "transition_cost": 1.0}


def report_families(track: bool = False):
    """The figure families of --voice_report and --evaluate_pairs, in the order of the reports.  ``track`` (--track_formants): the formants that
    the formants and the harmonics family read are audio.formant_tracks' (TRACK_CANDIDATES candidates per frame tracked to TRACK_FORMANTS), and the
    formants family also counts tracked_frames and track_segments.  Per family: ``report_flag`` and ``pairs_flag``,
    the args attributes that switch it on in the two reports (None: always on); ``block``, its name in the evaluation report; ``figures``,
    its tuple in audio; ``frames_key``, the report's key of its frame count; ``counts``, further keys of its statistics that the report sums;
    ``used(st)`` -> {figure: (B,) the frames behind its mean}; ``measure(batch, sr, hop, lens, voiced, n_frames, got)`` -> its
    audio.*_statistics of the batch, after leaving its per-frame dict under got[block] for the families behind it and for --functionals;
    ``finish(means)`` (None: nothing) turns pooled means that are not yet the report's figures into them, in place."""
    from . import audio

    def voice(batch, sr, hop, lens, voiced, n_frames, got):
        got["voice"] = audio.voice_quality(batch, sr, hop_length=hop, lengths=lens)
        return audio.voice_quality_statistics(got["voice"], voiced, n_frames)

    def analysed_formants(batch, sr, hop, lens):
        if not track:
            return audio.formants(batch, sr, hop_length=hop, lengths=lens)
        return audio.formant_tracks(audio.formants(batch, sr, hop_length=hop, lengths=lens, n_formants=TRACK_CANDIDATES), n_tracks=TRACK_FORMANTS)

    def formants(batch, sr, hop, lens, voiced, n_frames, got):
        fm = got["formants"] = analysed_formants(batch, sr, hop, lens)
        st = audio.formant_statistics(fm, voiced, n_frames)
        if track:
            st.update(tracked_frames=(fm["count"] > 0).sum(dim=1), track_segments=fm["segments"])
        return st

    def perturbation(batch, sr, hop, lens, voiced, n_frames, got):
        """audio.perturbation at YIN's own lags, reduced over the frames that the pitch tracker AND YIN call voiced."""
        pt = got["perturbation"] = audio.perturbation(batch, sr, hop_length=hop, lengths=lens)
        return audio.perturbation_statistics(pt, voiced & (pt["lag"] > 0), n_frames)

    def harmonics(batch, sr, hop, lens, voiced, n_frames, got):
        """audio.harmonics at YIN's own periods and the formants of --formants (without it audio.formants is run here), reduced over the frames
        that the pitch tracker calls voiced and whose figures YIN's period and the formants' bandwidths admit."""
        fm = got["harmonic_fm"] = got["formants"] if "formants" in got else analysed_formants(batch, sr, hop, lens)
        got["harmonics"] = audio.harmonics(batch, sr, hop_length=hop, lengths=lens, formants=fm)
        return audio.harmonic_statistics(got["harmonics"], voiced, n_frames, fm=fm)

    def auditory(batch, sr, hop, lens, voiced, n_frames, got):
        """audio.auditory over every frame of the row: loudness and MFCC over the live frames, the flux over the frames with a predecessor, the
        _voiced / _unvoiced figures under the pitch tracker's voicing."""
        got["auditory"] = audio.auditory(batch, sr, hop_length=hop, lengths=lens)
        return audio.auditory_statistics(got["auditory"], voiced, n_frames)

    def level_db(means):
        """equivalent_level_db pools as a mean POWER (audio.auditory_statistics' sums hold the power): the level is taken last."""
        p = means["equivalent_level_db"]
        means["equivalent_level_db"] = 10.0 * math.log10(p) if p is not None and p > 0.0 else None

    per_figure = lambda st: st["used"]
    return (Family(None, "voice_quality", "voice", audio.VOICE_QUALITY_FIGURES, "voiced_frames", (), lambda st: {k: st["frames"] for k in st["sums"]}, voice),
            Family("formants", "formants", "formants", audio.FORMANT_FIGURES, "formant_frames",
                   ("unconverged_frames",) + (("tracked_frames", "track_segments") if track else ()),
                   lambda st: {k: st["used"][:, int(k[1]) - 1] for k in st["sums"]}, formants),          # f_i and b_i share used[:, i]
            Family("perturbation", "perturbation", "perturbation", audio.PERTURBATION_FIGURES, "perturbation_frames", (), per_figure, perturbation),
            Family("harmonics", "harmonics", "harmonics", audio.HARMONIC_FIGURES, "harmonic_frames", (), per_figure, harmonics),
            Family("auditory", "auditory", "auditory", audio.AUDITORY_FIGURES, "auditory_frames", (), per_figure, auditory, level_db))


def enabled_families(args, flag: str):
    """The families of report_families() that ``args`` switches on; ``flag``: "report_flag" (--voice_report) or "pairs_flag" (--evaluate_pairs)."""
    return [f for f in report_families(getattr(args, "track_formants", False)) if getattr(f, flag) is None or getattr(args, getattr(f, flag), False)]


def family_rows(st, family):
    """A family's audio.*_statistics result as one host record per row: {"frames": int, every key of family.counts: int, "used": {figure: int},
    "sums": {figure: float}}.  The counts cross to the host in one copy and the sums in another."""
    used = family.used(st)
    ints = torch.stack([st["frames"]] + [st[k] for k in family.counts] + [used[k] for k in family.figures]).cpu()
    sums = torch.stack([st["sums"][k] for k in family.figures]).cpu()
    nc = 1 + len(family.counts)
    return [{"frames": int(ints[0, r]), **{k: int(ints[1 + j, r]) for j, k in enumerate(family.counts)},
             "used": {k: int(ints[nc + j, r]) for j, k in enumerate(family.figures)}, "sums": {k: float(sums[j, r]) for j, k in enumerate(family.figures)}}
            for r in range(ints.shape[1])]


def family_means(rows, family):
    """A family's figures of some rows of family_rows together, as a file's, a speaker's and the overall record hold them: every mean pooled
    over the frames behind it (the rows' sums over the rows' counts; None without a frame), then the frame count and family.counts summed."""
    out = {}
    for k in family.figures:
        n = sum(r["used"][k] for r in rows)
        out[k] = math.fsum(r["sums"][k] for r in rows) / n if n else None
    if family.finish is not None:
        family.finish(out)
    for key, field in ((family.frames_key, "frames"),) + tuple((k, k) for k in family.counts):
        out[key] = sum(r[field] for r in rows)
    return out


FUNCTIONAL_REPORT_KEYS = ("mean", "sd", "p20", "p50", "p80", "range", "rise_mean", "rise_sd", "fall_mean", "fall_sd", "peaks_per_s")
SEGMENT_REPORT_KEYS = ("voiced_per_s", "voiced_mean_s", "voiced_sd_s", "unvoiced_mean_s", "unvoiced_sd_s")


def functional_rows(vf):
    """audio.voice_functionals' result (at the percentiles 0.2, 0.5, 0.8) as one host record per row: {"functionals": {contour: {key: float or
    None}}, "segments": {key: float or None}}, the keys of FUNCTIONAL_REPORT_KEYS and SEGMENT_REPORT_KEYS; None where there is no value (NaN).
    Everything crosses to the host in one copy."""
    names = list(vf["contours"])

    def fields(o):
        pct = o["percentiles"]
        return [o["mean"], o["sd"], pct[:, 0], pct[:, 1], pct[:, 2], o["range"], o["rise_mean"], o["rise_sd"], o["fall_mean"], o["fall_sd"], o["peaks_per_s"]]

    table = torch.stack([torch.stack(fields(vf[c])) for c in names]).cpu()                      # (contours, keys, rows)
    seg = torch.stack([vf["segments"][k] for k in SEGMENT_REPORT_KEYS]).cpu()                    # (keys, rows)
    val = lambda x: None if math.isnan(float(x)) else float(x)
    return [{"functionals": {c: {k: val(table[i, j, r]) for j, k in enumerate(FUNCTIONAL_REPORT_KEYS)} for i, c in enumerate(names)},
             "segments": {k: val(seg[j, r]) for j, k in enumerate(SEGMENT_REPORT_KEYS)}} for r in range(seg.shape[1])]


def functional_means(rows):
    """The --functionals block of some rows of functional_rows together: for every value {"mean": the PLAIN mean over the files that have one
    (None without one), "files": how many those were}.  Percentiles do not pool from sums and an eGeMAPS vector describes one utterance, so a
    speaker's figure is the mean of the utterances' figures, not a figure of the pooled frames."""
    def mean(vals):
        vals = [v for v in vals if v is not None]
        return {"mean": math.fsum(vals) / len(vals) if vals else None, "files": len(vals)}

    contours = list(rows[0]["functionals"]) if rows else []
    return {"functionals": {c: {k: mean([r["functionals"][c][k] for r in rows]) for k in FUNCTIONAL_REPORT_KEYS} for c in contours},
            "segments": {k: mean([r["segments"][k] for r in rows]) for k in SEGMENT_REPORT_KEYS}}


def modulation_rows(vm):
    """audio.voice_modulation's figures as one host record per row: {"modulation": {figure: float or None}}, the keys of
    audio.VOICE_MODULATION_FIGURES; None where there is no value (NaN).  Everything crosses to the host in one copy."""
    from . import audio

    table = torch.stack([vm[k] for k in audio.VOICE_MODULATION_FIGURES]).cpu()                   # (figures, rows)
    val = lambda x: None if math.isnan(float(x)) else float(x)
    return [{"modulation": {k: val(table[j, r]) for j, k in enumerate(audio.VOICE_MODULATION_FIGURES)}} for r in range(table.shape[1])]


def modulation_means(rows):
    """The --modulation block of some rows of modulation_rows together: per figure {"mean": the PLAIN mean over the files that have one (None
    without one), "files": how many those were}, as --functionals does it: a rate and an extent describe one utterance."""
    def mean(vals):
        vals = [v for v in vals if v is not None]
        return {"mean": math.fsum(vals) / len(vals) if vals else None, "files": len(vals)}

    figures = list(rows[0]["modulation"]) if rows else []
    return {"modulation": {k: mean([r["modulation"][k] for r in rows]) for k in figures}}


def voice_modulation_of(audio, pitch, got, sig, sr, hop, lens, n_frames):
    """audio.voice_modulation of a batch, on the auditory frames of --auditory where that ran (``got``), else on its own."""
    au = got["auditory"] if "auditory" in got else audio.auditory(sig, sr, hop_length=hop, lengths=lens)
    return modulation_rows(audio.voice_modulation(pitch, au, n_frames, sr=sr, hop_length=hop))


@torch.inference_mode()
def voice_report(args, device):
    """--voice_report FILELIST (the filelist format of --prosody_report): every file is loaded with audio.load_audio(path, 22050), measured by
    audio.voice_quality on the frames of the pitch tracker (--pitch_method) and reduced by audio.voice_quality_statistics over the frames that are
    voiced and not silent, --batch_size files at a time.  FILELIST.voice.json receives per file seconds, frames, voiced_frames and the means
    of cpp_db, alpha_ratio_db, hammarberg_db, slope_0_500 and slope_500_1500 (null without such a frame); per speaker and overall the same
    means POOLED over the voiced frames (the files' sums over the files' counts), with the file count.  The figures are comparable across
    runs of this tool, not to the digit with Praat or VoiceSauce (audio.voice_quality says why).
    --formants adds per file f1_hz .. f3_hz and b1_hz .. b3_hz (audio.formants reduced by audio.formant_statistics over the voiced frames with
    at least three formants; null without such a frame), formant_frames (those frames) and unconverged_frames; per speaker and overall the
    means pooled over the frames behind each figure, and both counts summed.
    --track_formants (with --formants or --harmonics) analyses five candidates per frame and tracks F1-F3 through them (audio.formant_tracks: a
    Viterbi pass per row, Praat's Formant: Track), so that a spurious low candidate no longer shifts every formant by one slot; the tracked dict
    stands wherever the formants are passed on (the formant figures, the harmonics' formant input, --functionals).  The formants family gains
    tracked_frames and track_segments per file, summed per speaker and overall, and the report a top-level "formant_tracking" object with the
    parameters.
    --perturbation adds per file jitter_pct, rap_pct, shimmer_pct, shimmer_db and hnr_db (audio.perturbation reduced by
    audio.perturbation_statistics over the voiced frames; null without a frame that has a counted pair) and perturbation_frames (the voiced
    frames); per speaker and overall the means pooled over the frames behind each figure, and the count summed.
    --harmonics adds per file h1_h2_db, h1_a3_db, f1_rel_db, f2_rel_db and f3_rel_db (audio.harmonics reduced by audio.harmonic_statistics over
    the voiced frames that carry each figure, at formants of at most 700 Hz bandwidth; null without such a frame) and harmonic_frames (the
    voiced frames); per speaker and overall the means pooled over the frames behind each figure, and the count summed.  With --formants the
    formants are analysed once for both.
    --auditory adds per file loudness and mfcc_1 .. mfcc_4 (audio.auditory reduced by audio.auditory_statistics over the frames that are not silent),
    spectral_flux (over the frames with a predecessor), spectral_flux_voiced, spectral_flux_unvoiced and mfcc_1_voiced .. mfcc_4_voiced (under the
    pitch tracker's voicing), equivalent_level_db (10 log10 of the mean power over every frame) and auditory_frames (the frames that are not silent);
    per speaker and overall the means pooled over the frames behind each figure (the level from the pooled power), and the count summed.
    --functionals adds per file "functionals": {contour: {mean, sd, p20, p50, p80, range, rise_mean, rise_sd, fall_mean, fall_sd, peaks_per_s}}
    for f0_semitones (12 log2(f0 / 27.5)), the five voice-quality figures and the figures of the other flags given, each over the frames its mean
    above runs over (audio.voice_functionals: one device call per batch; slopes in units per second; null where there is no value), and
    "segments": voiced segments per second and the mean and sd length in seconds of the voiced and of the unvoiced segments.  Per speaker and
    overall every value becomes {"mean", "files"}: the PLAIN mean over the files that have the value and how many those were; percentiles do
    not pool from sums, and an eGeMAPS vector (Eyben et al. 2016) describes one utterance, so nothing here is pooled over frames.
    --modulation adds per file "modulation": the rate in Hz, the extent in semitones and the prominence in dB of the strongest 4-12 Hz
    oscillation of f0 over the voiced runs (tremor, vibrato), the sd of what the runs' lines leave, the same band of the loudness, and the
    rate, depth (relative to the mean loudness) and prominence of its strongest 2-8 Hz oscillation (the syllable rhythm)
    (audio.voice_modulation: one device call per batch; null where no run is long enough or the band has no peak).  Per speaker and overall
    every figure becomes {"mean", "files"} like the functionals: the figures are per utterance, not per frame, so they do not go through the
    figure families."""
    from . import audio

    want_func = getattr(args, "functionals", False)
    want_mod = getattr(args, "modulation", False)
    families = enabled_families(args, "report_flag")
    files, pooled = [], {}
    for chunk, batch, lens in filelist_batches(args.voice_report, args.batch_size, PROSODY_SR, device):
        pitch = pitch_tracker(args)(batch, PROSODY_SR, hop_length=PROSODY_HOP, lengths=lens)
        n_frames = [-(-n // PROSODY_HOP) for n in lens]
        got = {}                                     # block -> the per-frame dict of its analysis: every one runs once per batch
        rows = {f.block: family_rows(f.measure(batch, PROSODY_SR, PROSODY_HOP, lens, pitch["voiced"], n_frames, got), f) for f in families}
        if want_func:
            rows["functionals"] = functional_rows(audio.voice_functionals(pitch, got["voice"], n_frames, fm=got.get("formants"), pt=got.get("perturbation"),
                                                                          hm=got.get("harmonics"), sr=PROSODY_SR, hop_length=PROSODY_HOP,
                                                                          harmonic_fm=got.get("harmonic_fm"), au=got.get("auditory")))
        if want_mod:
            rows["modulation"] = voice_modulation_of(audio, pitch, got, batch, PROSODY_SR, PROSODY_HOP, lens, n_frames)
        for r, (wav, spk, _) in enumerate(chunk):
            spk = spk if spk is not None else "0"
            rec = {"path": wav, "speaker": spk, "seconds": lens[r] / float(PROSODY_SR), "frames": n_frames[r],
                   "voiced_frames": None}            # (filled by the first family: the key keeps this place, ahead of the figures)
            for f in families:
                rec.update(family_means([rows[f.block][r]], f))
            if want_func:
                rec.update(rows["functionals"][r])
            if want_mod:
                rec.update(rows["modulation"][r])
            files.append(rec)
            acc = pooled.setdefault(spk, {"files": 0, **{k: [] for k in rows}})
            acc["files"] += 1
            for k in rows:
                acc[k].append(rows[k][r])

    def pool(accs):
        out = {"files": sum(a["files"] for a in accs), "voiced_frames": None}
        for f in families:
            out.update(family_means([row for a in accs for row in a[f.block]], f))
        if want_func:
            out.update(functional_means([row for a in accs for row in a["functionals"]]))
        if want_mod:
            out.update(modulation_means([row for a in accs for row in a["modulation"]]))
        return out

    rep = {"sample_rate": PROSODY_SR, "hop_length": PROSODY_HOP, "files": files, "speakers": {k: pool([v]) for k, v in pooled.items()},
           "overall": pool(list(pooled.values()))}
    if pitch_method(args) != "yin":
        rep["pitch_method"] = pitch_method(args)
    if getattr(args, "track_formants", False):
        rep["formant_tracking"] = formant_tracking_parameters()
    out_path = f"{args.voice_report}.voice.json"
    with open(out_path, "w") as f:
        json.dump(rep, f, indent=1)
    for k in sorted(rep["speakers"]):
        v = rep["speakers"][k]
        fig = "no voiced frame" if v["cpp_db"] is None else (f"CPP {v['cpp_db']:.2f} dB, alpha ratio {v['alpha_ratio_db']:.1f} dB, Hammarberg {v['hammarberg_db']:.1f} dB, "
                                                            f"slopes {v['slope_0_500']:.1f} / {v['slope_500_1500']:.1f} dB/kHz")
        print(f"[i] speaker {k}: {v['files']} files, {v['voiced_frames']} voiced frames, {fig}")
    print(f"[+] Voice report saved: {Path(out_path).resolve()}")
    return rep


LOUDNESS_SR = 22050          # the analysis rate, as for the prosody report
LOUDNESS_OUTLIER_LU = 3.0    # a file this far from its speaker's mean is listed


def loudness_summary(values):
    """{"measured", "mean", "std", "min", "max"} of a speaker's integrated LUFS values (the files that have one): plain mean and population
    standard deviation of the LUFS figures; None for every statistic when there is none."""
    n = len(values)
    if n == 0:
        return {"measured": 0, "mean": None, "std": None, "min": None, "max": None}
    mean = math.fsum(values) / n
    return {"measured": n, "mean": mean, "std": math.sqrt(math.fsum((v - mean) ** 2 for v in values) / n), "min": min(values), "max": max(values)}


@torch.inference_mode()
def loudness_report(args, device):
    """--loudness_report FILELIST: the filelist format of --prosody_report.  Every file is loaded with audio.load_audio(path, 22050) and measured by
    audio.loudness (ITU-R BS.1770-4 on the device) and audio.peak_level, --batch_size files at a time (padded to the longest, each row with its
    own length).  FILELIST.loudness.json receives per file "integrated_lufs", "max_momentary_lufs" (the loudest 400 ms block), "peak_dbfs" and
    "seconds" (null where a figure does not exist: silence, a file under 400 ms) and per speaker the file count, mean / std / min / max of the
    integrated LUFS over the files that have one, and under "outliers" the files more than 3 LU from that mean."""
    from . import audio

    finite = lambda v: float(v) if math.isfinite(float(v)) else None
    files = []
    for chunk, batch, lens in filelist_batches(args.loudness_report, args.batch_size, LOUDNESS_SR, device):
        out = audio.loudness(batch, LOUDNESS_SR, lengths=lens)
        integrated, blocks = out["integrated"].cpu(), out["blocks"].cpu()
        momentary = out["momentary"].cpu()
        peak = audio.peak_level(batch, lens).cpu()
        for r, (wav, spk, _) in enumerate(chunk):
            nb = int(blocks[r])
            files.append({"path": wav, "speaker": spk if spk is not None else "0", "seconds": lens[r] / float(LOUDNESS_SR),
                          "integrated_lufs": finite(integrated[r]), "max_momentary_lufs": finite(momentary[r, :nb].max()) if nb > 0 else None,
                          "peak_dbfs": 20.0 * math.log10(float(peak[r])) if float(peak[r]) > 0 else None})
    speakers = {}
    for spk in dict.fromkeys(f["speaker"] for f in files):
        mine = [f for f in files if f["speaker"] == spk]
        st = loudness_summary([f["integrated_lufs"] for f in mine if f["integrated_lufs"] is not None])
        outliers = [f["path"] for f in mine if f["integrated_lufs"] is not None and abs(f["integrated_lufs"] - st["mean"]) > LOUDNESS_OUTLIER_LU]
        speakers[spk] = {"files": len(mine), **st, "outliers": outliers}
    rep = {"sample_rate": LOUDNESS_SR, "outlier_lu": LOUDNESS_OUTLIER_LU, "files": files, "speakers": speakers}
    out_path = f"{args.loudness_report}.loudness.json"
    with open(out_path, "w") as f:
        json.dump(rep, f, indent=1)
    for k in sorted(speakers):
        v = speakers[k]
        level = "no file with a loudness" if v["mean"] is None else (f"{v['mean']:.1f} LUFS mean, std {v['std']:.1f} LU, {v['min']:.1f} .. {v['max']:.1f}"
                                                                    + (f", {len(v['outliers'])} more than {LOUDNESS_OUTLIER_LU:g} LU off" if v["outliers"] else ""))
        print(f"[i] speaker {k}: {v['files']} files, {level}")
    print(f"[+] Loudness report saved: {Path(out_path).resolve()}")
    return rep


REVERB_SR = 22050            # the rate the files are loaded at, as for the other reports; audio.srmr takes them to 16 kHz


def reverb_summary(values):
    """{"measured", "mean", "std", "min"} of SRMR values (the files that have one), as ``loudness_summary`` forms them; the minimum is the most
    reverberant file.  None for every statistic when there is none."""
    return {k: v for k, v in loudness_summary(values).items() if k != "max"}


def srmr_value(v):
    return None if math.isnan(float(v)) else float(v)


@torch.inference_mode()
def reverb_report(args, device):
    """--reverb_report FILELIST: the filelist format of --loudness_report.  Every file is loaded with audio.load_audio(path, 22050) and measured by
    audio.srmr (the speech-to-reverberation modulation energy ratio on the device; no clean reference needed), --batch_size files at a time
    (padded to the longest, each row with its own length).  FILELIST.srmr.json receives per file "srmr" (null for a file under 256 ms or without
    energy in the high modulation bands; a dry voice reads high, a reverberant one low), "frames", "k_star" (the modulation bands counted) and
    "seconds"; per speaker and overall the file count and measured / mean / std / min of the SRMR over the files that have one."""
    from . import audio

    files = []
    for chunk, batch, lens in filelist_batches(args.reverb_report, args.batch_size, REVERB_SR, device):
        out = audio.srmr(batch, REVERB_SR, lengths=lens, rows=getattr(args, "srmr_rows", None))
        ratio, frames, ks = out["srmr"].cpu(), out["frames"].cpu(), out["k_star"].cpu()
        for r, (wav, spk, _) in enumerate(chunk):
            files.append({"path": wav, "speaker": spk if spk is not None else "0", "seconds": lens[r] / float(REVERB_SR), "srmr": srmr_value(ratio[r]),
                          "frames": int(frames[r]), "k_star": int(ks[r])})
    pool = lambda mine: {"files": len(mine), **reverb_summary([f["srmr"] for f in mine if f["srmr"] is not None])}
    speakers = {spk: pool([f for f in files if f["speaker"] == spk]) for spk in dict.fromkeys(f["speaker"] for f in files)}
    rep = {"sample_rate": REVERB_SR, "srmr_sample_rate": audio.SRMR_SR, "files": files, "speakers": speakers, "overall": pool(files)}
    out_path = f"{args.reverb_report}.srmr.json"
    with open(out_path, "w") as f:
        json.dump(rep, f, indent=1)
    for k in sorted(speakers):
        v = speakers[k]
        fig = "no file long enough to measure" if v["mean"] is None else f"SRMR {v['mean']:.2f} mean, std {v['std']:.2f}, {v['min']:.2f} min"
        print(f"[i] speaker {k}: {v['files']} files, {fig}")
    print(f"[+] Reverberation report saved: {Path(out_path).resolve()}")
    return rep


VOCODER_REPORT_KEYS = ("stoi", "estoi", "mel_l1", "lufs_shift")


VOCODER_DISTANCE_KEYS = ("mstft", "sc", "log_mag", "lsd_db")     # --spectral_distance: lower is better


def vocoder_summary(files, keys=VOCODER_REPORT_KEYS):
    """{"files", "unscored": the paths without a STOI score, and per key of ``keys`` {"mean", "min"} over the files that have the figure
    (null where none has) — {"mean", "max"} for the keys of VOCODER_DISTANCE_KEYS, where lower is better} of a list of --vocoder_report
    file entries."""
    out = {"files": len(files), "unscored": [f["path"] for f in files if f["stoi"] is None]}
    for k in keys:
        v = [f[k] for f in files if f[k] is not None]
        worst, pick = ("max", max) if k in VOCODER_DISTANCE_KEYS else ("min", min)
        out[k] = {"mean": math.fsum(v) / len(v) if v else None, worst: pick(v) if v else None}
    return out


@torch.inference_mode()
def vocoder_report(args, device):
    """--vocoder_report FILELIST (the filelist format of --prosody_report) with --vocoder_path / --synthetic and --vocoder_config: what copy
    synthesis through this vocoder costs.  Every file is loaded at the config's rate and analysed as --mel_from_wav does (the recording cut to
    256 x frames samples), --batch_size files at a time (padded with silence to the longest, each row with its own length), then vocoded; the
    synthesis is sample-aligned with the recording.  FILELIST.vocoder.json receives per file "stoi" and "estoi" (audio.stoi: the synthesis
    against the recording; null for a file too short to score), "mel_l1" (audio.mel_reconstruction_error), "lufs_shift" (the integrated
    loudness, audio.loudness, of the synthesis minus that of the recording; null where either has none) and "seconds"; per speaker and
    under "overall" the mean and the minimum of each and the files without a score.  With --spectral_distance every file also gets "mstft",
    "sc", "log_mag" and "lsd_db" (audio.stft_distance at the config's rate: the multi-resolution STFT distance, its two terms and the
    log-spectral distance in dB; null for a file too short for the widest window), the summaries their mean and maximum, and the report
    "stft_resolutions"."""
    from . import audio
    from . import weights as W
    from .hifigan import AttrDict, Generator

    entries = parse_filelist(args.vocoder_report)
    if not entries:
        sys.exit(f"[-] {args.vocoder_report}: no files listed")
    h = AttrDict(vocoder_config(args.vocoder_config))
    sr = int(h.get("sampling_rate", 22050))
    sd = W.synthetic_hifigan_state(h) if args.synthetic else torch.load(args.vocoder_path, map_location="cpu")["generator"]
    vocoder = Generator(h).to(device)
    vocoder.load_state_dict(sd)
    vocoder.eval()
    vocoder.remove_weight_norm()
    loud_ok = sr % 10 == 0 and sr >= 8000                                # the rates audio.k_weighting designs a filter for
    value = lambda v: float(v) if math.isfinite(float(v)) else None
    dist_keys = VOCODER_DISTANCE_KEYS if getattr(args, "spectral_distance", False) else ()
    keys = VOCODER_REPORT_KEYS + dist_keys
    files = []
    for b0 in range(0, len(entries), args.batch_size):
        chunk = entries[b0:b0 + args.batch_size]
        ys = [wav_at_rate(wav, sr, device) for wav, _, _ in chunk]
        rows = [r for r, y in enumerate(ys) if y is not None]
        fig = {}
        if rows:
            lens = [int(ys[r].shape[-1]) for r in rows]
            rec = torch.zeros(len(rows), max(lens), device=device)
            for i, r in enumerate(rows):
                rec[i, : lens[i]] = ys[r].reshape(-1)
            mel = audio.mel_spectrogram(rec, h.get("n_fft", 1024), h.get("num_mels", 80), sr, h.get("hop_size", 256), h.get("win_size", 1024),
                                        h.get("fmin", 0), h.get("fmax", 8000))
            frames = torch.tensor([n // 256 for n in lens], device=device)
            syn = vocoder(mel).squeeze(1).clamp(-1, 1).contiguous()
            if syn.shape != rec.shape:
                sys.exit(f"[-] the vocoder renders {syn.shape[1]} samples for {rec.shape[1]}: --vocoder_report needs a config that upsamples by 256")
            sc = audio.stoi(rec, syn, sr, lengths=lens)
            l1 = audio.mel_reconstruction_error(vocoder, mel, frames).cpu()
            shift = (audio.loudness(syn, sr, lengths=lens)["integrated"] - audio.loudness(rec, sr, lengths=lens)["integrated"]).cpu() if loud_ok else None
            st, es = sc["stoi"].cpu(), sc["estoi"].cpu()
            for i, r in enumerate(rows):
                fig[r] = {"seconds": lens[i] / float(sr), "stoi": value(st[i]), "estoi": value(es[i]), "mel_l1": value(l1[i]),
                          "lufs_shift": value(shift[i]) if shift is not None else None}
            if dist_keys:
                dist = audio.stft_distance(rec, syn, lengths=lens)
                for k in dist_keys:
                    col = dist[k].cpu()
                    for i, r in enumerate(rows):
                        fig[r][k] = value(col[i])
        for r, (wav, spk, _) in enumerate(chunk):
            files.append({"path": wav, "speaker": spk if spk is not None else "0",
                          **fig.get(r, {"seconds": None, **{k: None for k in keys}})})
    speakers = {spk: vocoder_summary([f for f in files if f["speaker"] == spk], keys) for spk in dict.fromkeys(f["speaker"] for f in files)}
    rep = {"sample_rate": sr, "vocoder_config": args.vocoder_config, "stoi_sample_rate": audio.STOI_SR, "files": files, "speakers": speakers,
           "overall": vocoder_summary(files, keys)}
    if dist_keys:
        rep["stft_resolutions"] = [list(r) for r in audio.MSTFT_RESOLUTIONS]
    out_path = f"{args.vocoder_report}.vocoder.json"
    with open(out_path, "w") as f:
        json.dump(rep, f, indent=1)
    for k in sorted(speakers):
        v = speakers[k]
        score = "no file long enough to score" if v["stoi"]["mean"] is None else (
            f"STOI {v['stoi']['mean']:.3f} mean, {v['stoi']['min']:.3f} min, ESTOI {v['estoi']['mean']:.3f} mean, mel L1 {v['mel_l1']['mean']:.3f}"
            + ("" if v["lufs_shift"]["mean"] is None else f", loudness {v['lufs_shift']['mean']:+.2f} LU")
            + ("" if not dist_keys or v["mstft"]["mean"] is None else f", M-STFT {v['mstft']['mean']:.3f} mean, LSD {v['lsd_db']['mean']:.2f} dB")
            + (f", {len(v['unscored'])} without a score" if v["unscored"] else ""))
        print(f"[i] speaker {k}: {v['files']} files, {score}")
    print(f"[+] Vocoder report saved: {Path(out_path).resolve()}")
    return rep


EVAL_MEL = (1024, 80, 22050, 256, 1024, 0, 8000)    # n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax of the vocoder config
EVAL_MAX_FRAMES = 4096                              # ev_dtw's limit per side (47.5 s)


def parse_pairs(path):
    """The lines of a pairs file as (recorded wav, synthesised wav, speaker): 'recorded.wav|synthesised.wav' or
    'recorded.wav|synthesised.wav|spk'; no speaker column counts as "0".  Relative paths resolve as in parse_filelist."""
    flist = Path(path)

    def resolve(wav):
        wav = wav.strip()
        return str(flist.parent / wav) if not os.path.exists(wav) and (flist.parent / wav).exists() else wav

    out = []
    for ln in flist.read_text(encoding="utf-8").splitlines():
        if not ln.strip():
            continue
        fields = ln.split("|")
        if len(fields) < 2:
            sys.exit(f"[-] {path}: 'recorded.wav|synthesised.wav[|spk]' expected, got {ln!r}")
        out.append((resolve(fields[0]), resolve(fields[1]), fields[2].strip() if len(fields) >= 3 and fields[2].strip() else "0"))
    return out


def evaluation_means(pairs):
    """The means over per-pair records: MCD and voicing error averaged over the pairs, the f0 RMSE pooled over all both-voiced frame
    pairs (None without one)."""
    n = len(pairs)
    voiced = sum(p["voiced_pairs"] for p in pairs)
    sq = math.fsum(p["f0_rmse_cents"] ** 2 * p["voiced_pairs"] for p in pairs if p["f0_rmse_cents"] is not None)
    return {"pairs": n, "mcd_db": math.fsum(p["mcd_db"] for p in pairs) / n, "f0_rmse_cents": math.sqrt(sq / voiced) if voiced else None,
            "voicing_error": math.fsum(p["voicing_error"] for p in pairs) / n, "voiced_pairs": voiced}


@torch.inference_mode()
def evaluate_pairs(args, device):
    """--evaluate_pairs PAIRS: how close is what the model says to what the actor recorded.  Each line names a recording and the
    synthesised wav of the same sentence (and optionally the speaker).  Both go through wav_at_rate(..., 22050), the vocoder config's mel,
    audio.mel_cepstrum, and audio.pitch_yin (whose first L / 256 frames are the mel's; --pitch_method pyin: audio.pitch_pyin, and the
    report gains "pitch_method": "pyin"); ev_dtw aligns the two cepstral sequences,
    --batch_size pairs at a time (padded to the longest, each row with its lengths).  PAIRS.eval.json receives per pair mcd_db,
    f0_rmse_cents (null without a frame pair voiced on both sides), voicing_error, voiced_pairs, frames_recorded, frames_synthesised and
    path_steps; per speaker and overall their means, f0 pooled over the both-voiced frame pairs; and under "skipped" the pairs with a file
    too short for a mel (or longer than 4096 frames).  Needs no checkpoint.
    --voice_quality adds per pair "voice": {"recorded", "synthesised", "delta"}: the means of audio.voice_quality's five figures over each
    side's own voiced, non-silent frames and synthesised - recorded (null where a side has no such frame), and per speaker and overall
    "voice": per figure the mean and the mean absolute value of the deltas.  It compares utterance-level means, so it needs no alignment.
    --formants adds "formants" in the same form: the means of F1-F3 and B1-B3 (audio.formants, audio.formant_statistics) of each side, their
    differences, and per speaker and overall the mean and mean absolute difference: a vowel-quality shift, where "voice" shows a tilt shift.
    --perturbation adds "perturbation" in the same form: jitter_pct, rap_pct, shimmer_pct, shimmer_db and hnr_db (audio.perturbation,
    audio.perturbation_statistics) of each side and their differences: wobbling periods or a buzzy waveform where pitch and spectrum agree.
    --harmonics adds "harmonics" in the same form: h1_h2_db, h1_a3_db, f1_rel_db, f2_rel_db and f3_rel_db (audio.harmonics,
    audio.harmonic_statistics) of each side and their differences: a breathier or a more pressed source where the vowel is the same.
    --auditory adds "auditory" in the same form: loudness, the spectral flux, MFCC 1-4, their voiced / unvoiced variants and equivalent_level_db
    (audio.auditory, audio.auditory_statistics) of each side and their differences: a duller, flatter or quieter rendering of the same sentence.
    --track_formants (with --formants or --harmonics): the formants of both are audio.formant_tracks' (five candidates per frame tracked to F1-F3);
    the report gains a top-level "formant_tracking" object with the parameters and keeps every other key.
    --modulation adds per pair "modulation": {"recorded", "synthesised", "delta"} over audio.voice_modulation's figures of each side (tremor
    and rhythm: rates, extents, prominences) and "ms_distortion_db" / "ms_shift_db", the distance between the modulation spectra of the two
    sides' mel-cepstral trajectories (audio.cepstral_modulation_distance: no alignment; a negative shift says the synthesised side moves
    less, i.e. is over-smoothed); per speaker and overall the mean and mean absolute difference per figure and the plain means of the two
    distances over the pairs that have them.
    --srmr adds per pair "srmr": {"recorded", "synthesised", "delta"}, audio.srmr of each side (non-intrusive: it needs no alignment; null for
    a side without a figure) and synthesised - recorded; per speaker and overall "srmr": the means of the three over the pairs that have them.
    --rhythm adds per pair "rhythm": {"recorded", "synthesised"} (RHYTHM_REPORT_KEYS of audio.speech_rate with "nuclei" and "pause_s", voiced by
    the tracker of this report) and "delta": {"rate_ratio" (0.15: the synthesis speaks 15 % faster), "pauses_delta", "pause_s_delta"}; per
    speaker and overall "rhythm": the means of the three differences over the pairs that have them.
    --envelope_mcd adds per pair "mcd_env_db": the mel-cepstral distortion of the mel-cepstra (order 24, alpha 0.455, coefficient 0 left out) of
    CheapTrick's spectral envelope on the tracker's periods (audio.envelope_cepstra, audio.cepstra_mcd: silent frames left out, an alignment of
    its own), null for a pair with a side without a frame; per speaker and overall "mcd_env_db": the mean over the pairs that have it."""
    from . import audio

    want_env = getattr(args, "envelope_mcd", False)
    want_mod = getattr(args, "modulation", False)
    want_srmr = getattr(args, "srmr", False)
    want_rhythm = getattr(args, "rhythm", False)

    entries = parse_pairs(args.evaluate_pairs)
    if not entries:
        sys.exit(f"[-] {args.evaluate_pairs}: no pairs listed")
    sr, hop = EVAL_MEL[2], EVAL_MEL[3]
    records, skipped = [], []
    families = enabled_families(args, "pairs_flag")

    def side(wavs):
        """mel cepstra (B, 13, T) padded with zeros, frames per row, and the pitch of every row"""
        frames = [w.shape[1] // hop for w in wavs]
        cep = torch.zeros(len(wavs), 13, max(frames), device=device)
        sig = torch.zeros(len(wavs), max(frames) * hop, device=device)
        for r, w in enumerate(wavs):
            cep[r, :, : frames[r]] = audio.mel_cepstrum(audio.mel_spectrogram(w, *EVAL_MEL), 13)[0]   # per file: each signal's own reflect padding
            sig[r, : w.shape[1]] = w[0]
        lens = [w.shape[1] for w in wavs]
        pitch = pitch_tracker(args)(sig, sr, hop_length=hop, lengths=lens)
        clipped, got = [min(n, sig.shape[1]) for n in lens], {}
        for f in families:
            st = f.measure(sig, sr, hop, lens if f.block == "voice" else clipped, pitch["voiced"], frames, got)
            pitch[f.block] = [{k: v for k, v in family_means([row], f).items() if k in f.figures} for row in family_rows(st, f)]
        if want_mod:
            pitch["modulation"] = [row["modulation"] for row in voice_modulation_of(audio, pitch, got, sig, sr, hop, clipped, frames)]
        if want_srmr:
            pitch["srmr"] = [srmr_value(v) for v in audio.srmr(sig, sr, lengths=clipped, rows=getattr(args, "srmr_rows", None))["srmr"].cpu()]
        if want_rhythm:
            pitch["rhythm"] = rhythm_rows(audio, args, sig, sr, hop, clipped, pitch["voiced"])
        if want_env:
            pitch["envelope"] = audio.envelope_cepstra(sig, audio.period_from_pitch(pitch, sr), sr, hop_length=hop, lengths=clipped,
                                                       rows=getattr(args, "envelope_rows", None))
        return cep, frames, pitch

    for b0 in range(0, len(entries), args.batch_size):
        chunk = []
        for rec, syn, spk in entries[b0:b0 + args.batch_size]:
            a, b = wav_at_rate(rec, sr, device), wav_at_rate(syn, sr, device)
            short = [p for p, w in ((rec, a), (syn, b)) if w is None]
            long_ = [p for p, w in ((rec, a), (syn, b)) if w is not None and w.shape[1] // hop > EVAL_MAX_FRAMES]
            if short or long_:
                skipped.append({"recorded": rec, "synthesised": syn, "speaker": spk,
                                "reason": (f"too short for a mel: {', '.join(short)}" if short else f"longer than {EVAL_MAX_FRAMES} frames: {', '.join(long_)}")})
                continue
            chunk.append((rec, syn, spk, a, b))
        if not chunk:
            continue
        cep_a, fr_a, pitch_a = side([c[3] for c in chunk])
        cep_b, fr_b, pitch_b = side([c[4] for c in chunk])
        al = audio.dtw(cep_a, cep_b, fr_a, fr_b, "euclidean")
        mcd = audio.mcd_from_cost(al["cost"], al["steps"]).cpu()
        f0 = audio.f0_errors(pitch_a["f0"], pitch_a["voiced"], pitch_b["f0"], pitch_b["voiced"], al["path"], al["steps"])
        steps, verr, nv = al["steps"].cpu(), f0["voicing_error"].cpu(), f0["voiced_pairs"].cpu()
        if want_mod:
            msd = audio.cepstral_modulation_distance(cep_a, cep_b, fr_a, fr_b, sr, hop)
            msd = torch.stack([msd["ms_distortion_db"], msd["ms_shift_db"]]).cpu()
        if want_env:
            mcd_env = audio.cepstra_mcd(*pitch_a["envelope"], *pitch_b["envelope"]).cpu()
        for r, (rec, syn, spk, _, _) in enumerate(chunk):
            records.append({"recorded": rec, "synthesised": syn, "speaker": spk, "mcd_db": float(mcd[r]), "f0_rmse_cents": f0["rmse_cents"][r],
                            "voicing_error": float(verr[r]), "voiced_pairs": int(nv[r]), "frames_recorded": fr_a[r], "frames_synthesised": fr_b[r],
                            "path_steps": int(steps[r])})
            for f in families:
                va, vb = pitch_a[f.block][r], pitch_b[f.block][r]
                records[-1][f.block] = {"recorded": va, "synthesised": vb,
                                        "delta": {k: (None if va[k] is None or vb[k] is None else vb[k] - va[k]) for k in va}}
            if want_mod:
                va, vb = pitch_a["modulation"][r], pitch_b["modulation"][r]
                val = lambda x: None if math.isnan(float(x)) else float(x)
                records[-1]["modulation"] = {"recorded": va, "synthesised": vb,
                                             "delta": {k: (None if va[k] is None or vb[k] is None else vb[k] - va[k]) for k in va},
                                             "ms_distortion_db": val(msd[0, r]), "ms_shift_db": val(msd[1, r])}
            if want_srmr:
                va, vb = pitch_a["srmr"][r], pitch_b["srmr"][r]
                records[-1]["srmr"] = {"recorded": va, "synthesised": vb, "delta": None if va is None or vb is None else vb - va}
            if want_rhythm:
                va, vb = pitch_a["rhythm"][r], pitch_b["rhythm"][r]
                records[-1]["rhythm"] = {"recorded": va, "synthesised": vb, "delta": rhythm_difference(va, vb)}
            if want_env:
                records[-1]["mcd_env_db"] = None if math.isnan(float(mcd_env[r])) else float(mcd_env[r])

    def means(recs):
        out = evaluation_means(recs)
        for f in families:
            out[f.block] = {}
            for k in f.figures:
                d = [r[f.block]["delta"][k] for r in recs if r[f.block]["delta"][k] is not None]
                out[f.block][k] = {"mean_delta": math.fsum(d) / len(d) if d else None, "mean_abs_delta": math.fsum(abs(v) for v in d) / len(d) if d else None}
        if want_mod:
            out["modulation"] = {}
            for k in audio.VOICE_MODULATION_FIGURES:
                d = [r["modulation"]["delta"][k] for r in recs if r["modulation"]["delta"][k] is not None]
                out["modulation"][k] = {"mean_delta": math.fsum(d) / len(d) if d else None,
                                        "mean_abs_delta": math.fsum(abs(v) for v in d) / len(d) if d else None}
            for k in ("ms_distortion_db", "ms_shift_db"):
                d = [r["modulation"][k] for r in recs if r["modulation"][k] is not None]
                out["modulation"][k] = {"mean": math.fsum(d) / len(d) if d else None, "pairs": len(d)}
        if want_srmr:
            out["srmr"] = {}
            for k in ("recorded", "synthesised", "delta"):
                d = [r["srmr"][k] for r in recs if r["srmr"][k] is not None]
                out["srmr"][k] = math.fsum(d) / len(d) if d else None
        if want_rhythm:
            out["rhythm"] = rhythm_means([r["rhythm"]["delta"] for r in recs], ("rate_ratio", "pauses_delta", "pause_s_delta"))
        if want_env:
            d = [r["mcd_env_db"] for r in recs if r["mcd_env_db"] is not None]
            out["mcd_env_db"] = math.fsum(d) / len(d) if d else None
        return out

    by_spk = {}
    for r in records:
        by_spk.setdefault(r["speaker"], []).append(r)
    rep = {"sample_rate": sr, "hop_length": hop, "n_coeffs": 13, "pairs": records, "speakers": {k: means(v) for k, v in by_spk.items()},
           "overall": means(records) if records else None, "skipped": skipped}
    if pitch_method(args) != "yin":
        rep["pitch_method"] = pitch_method(args)
    if getattr(args, "track_formants", False):
        rep["formant_tracking"] = formant_tracking_parameters()
    out_path = f"{args.evaluate_pairs}.eval.json"
    with open(out_path, "w") as f:
        json.dump(rep, f, indent=1)
    for k in sorted(rep["speakers"]):
        v = rep["speakers"][k]
        f0s = "no frame pair voiced on both sides" if v["f0_rmse_cents"] is None else f"f0 RMSE {v['f0_rmse_cents']:.1f} cents"
        print(f"[i] speaker {k}: {v['pairs']} pairs, MCD {v['mcd_db']:.2f} dB, {f0s}, voicing error {100 * v['voicing_error']:.1f} %")
    print(f"[+] Evaluation report saved: {Path(out_path).resolve()}  ({len(records)} pairs, {len(skipped)} skipped)")
    return rep


def loss_draws(seed: int, n_feats: int, frames: int):
    """(t (1,), z (1, n_feats, frames)) of --losses: one CPU generator seeded with --seed, t first."""
    g = torch.Generator().manual_seed(int(seed))
    return torch.rand(1, generator=g), torch.randn(1, n_feats, frames, generator=g)


@torch.inference_mode()
def cli(argv=None):
    p = argparse.ArgumentParser(description="Matcha-TTS / EmojiVoice synthesis on MI355X")
    p.add_argument("--checkpoint_path", type=str, default=None)
    p.add_argument("--vocoder_path", type=str, default=None, help="HiFi-GAN generator checkpoint (dict with 'generator')")
    p.add_argument("--synthetic", action="store_true", help="random-init weights (no checkpoint is available offline)")
    p.add_argument("--vocoder_config", type=str, default="v1", help="HiFi-GAN generator config: v1, v2, v3 or the path of an upstream "
                   "config.json (with --synthetic: random weights of that config)")
    p.add_argument("--ids", type=str, default=None, help="phoneme ids of one utterance, space separated")
    p.add_argument("--phonemes", type=str, default=None, help="one pre-phonemised (IPA) utterance, e.g. the output of english_cleaners2; "
                   "mapped through the 198-symbol table and interspersed with blanks like the reference front end")
    p.add_argument("--file", type=str, default=None, help="one id sequence per line, optional '|speaker'")
    p.add_argument("--file_phonemes", action="store_true", help="lines of --file are IPA strings, not ids")
    p.add_argument("--add_blank", action="store_true", help="intersperse ids with 0 like the reference front end")
    p.add_argument("--emoji-text", type=str, default=None, help="LLM-style text; its first mapped emoji selects the speaker (feel_me.py)")
    p.add_argument("--spk", type=int, default=None)
    p.add_argument("--temperature", type=float, default=0.667)
    p.add_argument("--speaking_rate", type=float, default=None)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--denoiser_strength", type=float, default=0.00025)
    p.add_argument("--output_folder", type=str, default=os.getcwd())
    p.add_argument("--batched", action="store_true")
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--mel_from_wav", type=str, default=None, help="analysis instead of synthesis: a PCM wav (16 / 24 bit, any rate: resampled on the device) -> PATH.mel.npy; "
                   "with --vocoder_path or --synthetic also PATH.copysyn.wav (copy synthesis)")
    p.add_argument("--align_mel", type=str, default=None, help="alignment instead of synthesis: a normalised mel (80, frames) .npy of the utterance "
                   "given by --ids / --phonemes -> PATH.durations.npy (monotonic alignment search, Tx integers)")
    p.add_argument("--align_wav", type=str, default=None, help="the same from a PCM wav at any rate, analysed as --mel_from_wav does and normalised")
    p.add_argument("--losses", action="store_true", help="with --align_mel / --align_wav: also PATH.losses.json, the utterance's dur_loss, prior_loss and "
                   "diff_loss (MatchaTTS.score); the loss's time and noise are drawn from --seed")
    p.add_argument("--seed", type=int, default=0, help="seed of the draws of --losses")
    p.add_argument("--data_statistics", type=str, default=None, help="dataset statistics instead of synthesis: a filelist whose first '|'-separated field "
                   "per line is a wav path -> FILELIST.stats.json with mel_mean / mel_std (--batch_size files per batch)")
    p.add_argument("--sample_rate", type=int, default=None, help="write the synthesised wavs at this rate (resampled on the device from 22050 Hz); "
                   "omitted: 22050 Hz, untouched.  With --prepare_dataset: the rate of the prepared recordings (default 22050)")
    p.add_argument("--prepare_dataset", type=str, default=None, help="dataset preparation instead of synthesis: a filelist 'path|spk|text' or 'path|text' of raw "
                   "recordings -> trimmed, levelled 16-bit mono wavs under --out_dir, DIR/filelist.txt and FILELIST.durations.json")
    p.add_argument("--out_dir", type=str, default=None, help="folder of --prepare_dataset's / --augment_dataset's wavs and filelist.txt")
    p.add_argument("--augment_dataset", type=str, default=None, help="dataset augmentation instead of synthesis: the filelist 'path|spk|text' --prepare_dataset "
                   "writes -> every file once per --rates value (time-stretched) and once per --semitones value (pitch-shifted) under --out_dir, "
                   "--out_dir/filelist.txt (originals, then variants) and FILELIST.augment.json (phase vocoder on the device, --batch_size files per batch)")
    p.add_argument("--rates", type=str, default=None, help="--augment_dataset: comma-separated speed factors, e.g. 0.9,1.1 (each in [0.125, 8], not 1)")
    p.add_argument("--semitones", type=str, default=None, help="--augment_dataset: comma-separated pitch shifts in semitones, e.g. -1,1 (each in [-12, 12], not 0)")
    p.add_argument("--top_db", type=float, default=60.0, help="--prepare_dataset: frames this many dB below the loudest one are silence (librosa.effects.trim)")
    p.add_argument("--peak", type=float, default=0.95, help="--prepare_dataset: peak level of the prepared recordings (hifigan/meldataset.py:152); 0: level untouched")
    p.add_argument("--prosody_report", type=str, default=None, help="pitch analysis instead of synthesis: a filelist 'path|spk|text' (the one --prepare_dataset "
                   "writes) -> FILELIST.prosody.json: voiced fraction, f0 median / 5th / 95th percentile and range in semitones per file and per speaker "
                   "(YIN on the device, --batch_size files per batch; needs no checkpoint)")
    p.add_argument("--evaluate_pairs", type=str, default=None, help="objective evaluation instead of synthesis: a file of 'recorded.wav|synthesised.wav[|spk]' lines -> "
                   "PAIRS.eval.json: mel-cepstral distortion (dB), f0 RMSE (cents) and voicing-decision error over the DTW path per pair, per speaker "
                   "and overall (DTW on the device, --batch_size pairs per batch; needs no checkpoint)")
    p.add_argument("--pitch_method", type=str, default="yin", choices=["yin", "pyin"], help="--prosody_report / --evaluate_pairs: the pitch tracker. yin decides "
                   "every frame on its own; pyin (probabilistic YIN) keeps every candidate of a frame and picks the contour by a Viterbi pass, which "
                   "removes most octave jumps and dropped frames; its report carries \"pitch_method\": \"pyin\"")
    p.add_argument("--loudness_report", type=str, default=None, help="loudness analysis instead of synthesis: a filelist 'path|spk|text' -> FILELIST.loudness.json: "
                   "ITU-R BS.1770-4 integrated LUFS, loudest 400 ms block, peak in dBFS and seconds per file; mean / std / min / max per speaker and the files "
                   "more than 3 LU from their speaker's mean (on the device, --batch_size files per batch; needs no checkpoint)")
    p.add_argument("--reverb_report", type=str, default=None, help="reverberation analysis instead of synthesis: a filelist 'path|spk|text' -> FILELIST.srmr.json: "
                   "the speech-to-reverberation modulation energy ratio (SRMR, non-intrusive; a dry voice reads high, a reverberant room low), frames, "
                   "modulation bands counted and seconds per file; mean / std / min per speaker and overall (on the device, --batch_size files per "
                   "batch; needs no checkpoint)")
    p.add_argument("--srmr", action="store_true", help="--evaluate_pairs: add \"srmr\" per pair (the SRMR of the recording, of the synthesis and their "
                   "difference; no alignment needed) and the means per speaker and overall")
    p.add_argument("--rhythm", action="store_true", help="--prosody_report and --evaluate_pairs: add \"rhythm\" (speech rate and articulation rate in "
                   "syllable nuclei per second, pauses, mean pause and phonation ratio by De Jong and Wempe's method on the device, voiced by the "
                   "report's pitch tracker); per pair both sides and the relative rate difference, the pause-count and the pause-time difference")
    p.add_argument("--envelope_mcd", action="store_true", help="--evaluate_pairs: add \"mcd_env_db\" per pair, per speaker and overall: the mel-cepstral "
                   "distortion of the mel-cepstra (order 24, alpha 0.455) of CheapTrick's f0-adaptive spectral envelope on the report's pitch tracker, "
                   "aligned by DTW on the device: the literature's kind of MCD beside the log-mel one")
    p.add_argument("--target_lufs", type=float, default=None, help="--prepare_dataset: level every recording to this integrated loudness (BS.1770, e.g. -23) "
                   "instead of to --peak; the gain is capped where the peak would pass --peak, and the gain and the cap go into FILELIST.durations.json")
    p.add_argument("--vocoder_report", type=str, default=None, help="vocoder evaluation instead of synthesis: a filelist 'path|spk|text' -> FILELIST.vocoder.json: "
                   "STOI / ESTOI of copy synthesis against the recording, mel L1, loudness shift and seconds per file; mean and minimum per speaker and "
                   "overall (with --vocoder_path or --synthetic, --vocoder_config; on the device, --batch_size files per batch)")
    p.add_argument("--spectral_distance", action="store_true", help="--vocoder_report: add the multi-resolution STFT distance (\"mstft\": spectral convergence "
                   "\"sc\" + log-magnitude L1 \"log_mag\" at 1024/120/600, 2048/240/1200 and 512/50/240) and the log-spectral distance \"lsd_db\" per file, "
                   "with mean and maximum per speaker and overall")
    p.add_argument("--voice_report", type=str, default=None, help="voice-quality analysis instead of synthesis: a filelist 'path|spk|text' -> FILELIST.voice.json: "
                   "cepstral peak prominence, alpha ratio, Hammarberg index and the spectral slopes 0-500 / 500-1500 Hz, averaged over the voiced frames "
                   "(--pitch_method) per file, per speaker and overall (on the device, --batch_size files per batch; needs no checkpoint)")
    p.add_argument("--voice_quality", action="store_true", help="--evaluate_pairs: add \"voice\" per pair (the five voice-quality means of the recording, of the "
                   "synthesis and their differences) and per speaker and overall (mean and mean absolute difference)")
    p.add_argument("--formants", action="store_true", help="--voice_report: add the mean F1-F3 and their bandwidths B1-B3 in Hz over the voiced frames "
                   "(Burg's linear prediction at 11025 Hz, Praat's settings; no tracking across frames) per file, per speaker and overall; "
                   "--evaluate_pairs: add \"formants\" per pair (both sides and their differences) and per speaker and overall")
    p.add_argument("--perturbation", action="store_true", help="--voice_report: add the mean local jitter, RAP and local shimmer in percent, shimmer in dB "
                   "and the harmonics-to-noise ratio in dB over the voiced frames (pitch marks by peak picking at YIN's lag, three cycles each side) "
                   "per file, per speaker and overall; --evaluate_pairs: add \"perturbation\" per pair (both sides and their differences) and per "
                   "speaker and overall")
    p.add_argument("--track_formants", action="store_true", help="with --formants or --harmonics under --voice_report or --evaluate_pairs: analyse five "
                   "candidates per frame and track F1-F3 through them on the device (a Viterbi pass per file, Praat's Formant: Track) instead of taking "
                   "the three lowest; adds tracked_frames and track_segments to the formants' keys and \"formant_tracking\" (the parameters) to the report")
    p.add_argument("--modulation", action="store_true", help="--voice_report: add \"modulation\" per file: rate (Hz), extent (semitones) and prominence "
                   "(dB) of the strongest 4-12 Hz oscillation of f0 (tremor, vibrato) and of the loudness, and rate, depth and prominence of the "
                   "loudness contour's strongest 2-8 Hz oscillation (the syllable rhythm), from the modulation spectra of the two contours (one device "
                   "call per batch); per speaker and overall the mean over the files that have each figure.  --evaluate_pairs: the same figures of "
                   "both sides with their differences, and ms_distortion_db / ms_shift_db, the distance between the modulation spectra of the two "
                   "sides' mel-cepstral trajectories (negative shift: the synthesised side is over-smoothed)")
    p.add_argument("--functionals", action="store_true", help="--voice_report: add \"functionals\" per file: mean, sd, the 20th / 50th / 80th percentile and "
                   "their range, mean and sd of the rising and of the falling slopes per second and the peaks per second of every contour the report "
                   "measures (f0 in semitones from 27.5 Hz, the voice-quality figures, and those of --formants / --perturbation / --harmonics), and "
                   "\"segments\": rate and lengths of the voiced and unvoiced segments (the eGeMAPS functionals, one device call per batch); per "
                   "speaker and overall the plain mean of each value over the files that have one")
    p.add_argument("--harmonics", action="store_true", help="--voice_report: add the mean H1-H2, H1-A3 and the level of the harmonic at F1, F2 and F3 "
                   "over H1 in dB over the voiced frames (the harmonics of YIN's period in the log spectrum, at the formants of --formants) per "
                   "file, per speaker and overall; --evaluate_pairs: add \"harmonics\" per pair (both sides and their differences) and per speaker "
                   "and overall")
    p.add_argument("--auditory", action="store_true", help="--voice_report: add the mean loudness (mel bands under an equal-loudness weighting, "
                   "compressed by a 0.33 power law) and MFCC 1-4 over the frames that are not silent, the mean spectral flux over the frames with a "
                   "predecessor, the flux and the MFCC over the voiced (the flux also over the unvoiced) frames and the equivalent level in dB, with "
                   "auditory_frames, per file, per speaker and overall; with --functionals the functionals of these contours (the peaks per second of "
                   "\"loudness\" is the eGeMAPS loudness peak rate); --evaluate_pairs: add \"auditory\" per pair (both sides and their differences) "
                   "and per speaker and overall")
    args = validate_args(p.parse_args(argv))
    if args.voice_report:
        if not torch.cuda.is_available():
            sys.exit("[-] No ROCm GPU visible: this CLI drives the MI355X path only (no CPU fallback)")
        return voice_report(args, torch.device("cuda", 0))
    if args.vocoder_report:
        if not torch.cuda.is_available():
            sys.exit("[-] No ROCm GPU visible: this CLI drives the MI355X path only (no CPU fallback)")
        return vocoder_report(args, torch.device("cuda", 0))
    if args.reverb_report:
        if not torch.cuda.is_available():
            sys.exit("[-] No ROCm GPU visible: this CLI drives the MI355X path only (no CPU fallback)")
        return reverb_report(args, torch.device("cuda", 0))
    if args.loudness_report:
        if not torch.cuda.is_available():
            sys.exit("[-] No ROCm GPU visible: this CLI drives the MI355X path only (no CPU fallback)")
        return loudness_report(args, torch.device("cuda", 0))
    if args.evaluate_pairs:
        if not torch.cuda.is_available():
            sys.exit("[-] No ROCm GPU visible: this CLI drives the MI355X path only (no CPU fallback)")
        return evaluate_pairs(args, torch.device("cuda", 0))
    if args.prosody_report:
        if not torch.cuda.is_available():
            sys.exit("[-] No ROCm GPU visible: this CLI drives the MI355X path only (no CPU fallback)")
        return prosody_report(args, torch.device("cuda", 0))
    if args.augment_dataset:
        if not torch.cuda.is_available():
            sys.exit("[-] No ROCm GPU visible: this CLI drives the MI355X path only (no CPU fallback)")
        return augment_dataset(args, torch.device("cuda", 0))
    if args.prepare_dataset:
        if not torch.cuda.is_available():
            sys.exit("[-] No ROCm GPU visible: this CLI drives the MI355X path only (no CPU fallback)")
        return prepare_dataset(args, torch.device("cuda", 0))
    if args.align_mel or args.align_wav:
        if not torch.cuda.is_available():
            sys.exit("[-] No ROCm GPU visible: this CLI drives the MI355X path only (no CPU fallback)")
        return align_durations(args, torch.device("cuda", 0))
    if args.mel_from_wav:
        if not torch.cuda.is_available():
            sys.exit("[-] No ROCm GPU visible: this CLI drives the MI355X path only (no CPU fallback)")
        return mel_from_wav(args, torch.device("cuda", 0))
    if args.data_statistics:
        if not torch.cuda.is_available():
            sys.exit("[-] No ROCm GPU visible: this CLI drives the MI355X path only (no CPU fallback)")
        return data_statistics(args, torch.device("cuda", 0))
    if not args.synthetic:
        assert args.checkpoint_path and args.vocoder_path, "--checkpoint_path and --vocoder_path are required (or --synthetic)"
    if not torch.cuda.is_available():
        sys.exit("[-] No ROCm GPU visible: this CLI drives the MI355X path only (no CPU fallback)")
    device = torch.device("cuda", 0)
    model, vocoder, denoiser = load_models(args, device)
    spk_default = args.spk
    if args.emoji_text is not None:
        from .emoji import parse_response

        _, spk_default = parse_response(args.emoji_text)
        print(f"[emoji] speaker {spk_default} selected from {args.emoji_text!r}")
    if spk_default is None:
        warnings.warn("[-] No speaker provided, using speaker number 0.", UserWarning)
        spk_default = 0
    items = parse_lines(args)
    folder = Path(args.output_folder)
    folder.mkdir(exist_ok=True, parents=True)
    rtfs = []
    bs = args.batch_size if args.batched else 1
    for b0 in range(0, len(items), bs):
        chunk = items[b0:b0 + bs]
        lens = torch.tensor([len(i) for i, _ in chunk], dtype=torch.long)
        x = torch.zeros(len(chunk), int(lens.max()), dtype=torch.long)
        for r, (ids, _) in enumerate(chunk):
            x[r, :len(ids)] = torch.tensor(ids)
        spks = torch.tensor([s if s is not None else spk_default for _, s in chunk], dtype=torch.long)
        t0 = dt.datetime.now()
        out = model.synthesise(x.to(device), lens.to(device), n_timesteps=args.steps, temperature=args.temperature,
                               spks=spks.to(device), length_scale=args.speaking_rate)
        wav = to_waveform(out["mel"], vocoder, denoiser, args.denoiser_strength)
        t = (dt.datetime.now() - t0).total_seconds()
        wav = wav.reshape(len(chunk), -1)
        rtf_w = t * 22050 / wav.shape[-1] / len(chunk)
        rtfs.append(rtf_w)
        print(f"[batch {b0 // bs + 1}] Matcha-TTS RTF: {out['rtf']:.4f}  + VOCODER RTF: {rtf_w:.4f}")
        for r in range(len(chunk)):
            n = int(out["mel_lengths"][r])
            name = f"utterance_{b0 + r + 1:03d}_speaker_{int(spks[r]):03d}"
            np.save(folder / name, out["mel"][r, :, :n].cpu().numpy())
            if args.sample_rate is None or args.sample_rate == 22050:
                write_wav_pcm24(folder / f"{name}.wav", wav[r, : n * 256].numpy())
            else:
                from .audio import resample

                out_wav = resample(wav[r, : n * 256].to(device).unsqueeze(0), 22050, args.sample_rate)[0].cpu().numpy()
                write_wav_pcm24(folder / f"{name}.wav", out_wav, sr=args.sample_rate)
            print(f"[+] Waveform saved: {(folder / (name + '.wav')).resolve()}  ({n * 256 / 22050:.2f} s)")
    print(f"[avg] Matcha-TTS + VOCODER RTF: {np.mean(rtfs):.4f} ± {np.std(rtfs):.4f}")


if __name__ == "__main__":
    cli()
