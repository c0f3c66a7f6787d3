"""ctypes binding of ``libemojivoice_hip.so`` (C ABI declared in include/emojivoice.h).

There is NO CPU fallback: importing works everywhere (so the package can be
inspected on a CPU box) but any compute call raises ``EvLibraryError`` when the
HIP library is missing or no GPU is visible.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess
from typing import Dict, Optional

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EV_LIB_PATH") or os.path.join(_HERE, "lib", "libemojivoice_hip.so")   # EV_LIB_PATH: A/B builds of the same ABI
CSRC = os.path.join(_HERE, "csrc")
# Everything the library is built from: the one translation unit first, then what it includes.  build_library rebuilds when any is newer.
SOURCES = [os.path.join(CSRC, n) for n in ("ev_engine.hip", "ev_kernels.h", "ev_analysis_kernels.h", "ev_analysis.h")] \
    + [os.path.join(os.path.dirname(_HERE), "include", "emojivoice.h")]

EXPORTS = [
    "ev_abi_version", "ev_create", "ev_destroy", "ev_last_error", "ev_load_estimator", "ev_load_vocoder", "ev_load_vocoder_cfg", "ev_load_text_encoder", "ev_text_encoder",
    "ev_text_encoder_status", "ev_stft_magnitude", "ev_denoise", "ev_align", "ev_dbg_conv_bench",
    "ev_workspace_bytes", "ev_cfm_decode", "ev_estimator", "ev_hifigan", "ev_profile_enable", "ev_profile_read", "ev_profile_read_split", "ev_dbg_last_cfg", "ev_set_arithmetic", "ev_get_arithmetic",
    "ev_op_conv1d", "ev_op_groupnorm_mish", "ev_op_groupnorm_mish2", "ev_op_conv_groupnorm", "ev_op_layernorm", "ev_op_split_pieces", "ev_op_attention", "ev_op_ln_mlp", "ev_set_mrf_streams_max",
    "ev_cfm_decode2", "ev_reserve", "ev_alloc_count", "ev_dbg_sk_stats", "ev_op_attn_out", "ev_dbg_set_amax", "ev_dbg_set_attn_h16", "ev_dbg_set_chain", "ev_dbg_sk_taken",
    "ev_load_mel_basis", "ev_mel_spectrogram",
    "ev_maximum_path", "ev_log_prior", "ev_mas_align",
    "ev_estimator_rows", "ev_cfm_loss",
    "ev_load_resampler", "ev_resample", "ev_mel_stats",
    "ev_trim_bounds", "ev_trim_apply",
    "ev_pitch_yin", "ev_dtw",
    "ev_loudness",
    "ev_pyin_observe", "ev_pyin_decode",
    "ev_op_attention2", "ev_op_attn_out2",
    "ev_load_stoi", "ev_stoi",
    "ev_load_stft_dist", "ev_stft_dist",
    "ev_load_voice_quality", "ev_voice_quality",
    "ev_load_formants", "ev_formants", "ev_formant_track",
    "ev_perturbation",
    "ev_load_harmonics", "ev_harmonics",
    "ev_functionals", "ev_modulation",
    "ev_load_auditory", "ev_auditory",
    "ev_load_srmr", "ev_srmr",
    "ev_load_speech_rate", "ev_speech_rate",
    "ev_load_envelope", "ev_envelope",
    "ev_load_phase_vocoder", "ev_phase_vocoder",
    "ev_op_conv1d_epi",
]


class EvLibraryError(RuntimeError):
    pass


class ev_tensor_index(C.Structure):
    _fields_ = [("name", C.c_char_p), ("offset", C.c_uint64), ("ndim", C.c_int32), ("shape", C.c_int64 * 4)]


class ev_model_dims(C.Structure):
    _fields_ = [("n_feats", C.c_int32), ("spk_emb_dim", C.c_int32), ("channels", C.c_int32), ("heads", C.c_int32),
                ("head_dim", C.c_int32)]


class ev_vocoder_config(C.Structure):
    _fields_ = [("resblock", C.c_int32), ("num_levels", C.c_int32), ("upsample_rates", C.c_int32 * 4), ("upsample_kernel_sizes", C.c_int32 * 4),
                ("resblock_kernel_sizes", C.c_int32 * 3), ("resblock_dilations", (C.c_int32 * 3) * 3)]


class ev_conv_epi(C.Structure):
    _fields_ = [("act", C.c_int32), ("act_slope", C.c_float), ("d_alpha_exp", C.c_void_p), ("d_beta_inv", C.c_void_p), ("d_lengths", C.c_void_p),
                ("mask1", C.c_int32), ("mask2", C.c_int32), ("scale", C.c_float), ("d_R", C.c_void_p), ("accum", C.c_int32), ("d_yold", C.c_void_p),
                ("div3", C.c_int32), ("act2_slope", C.c_float), ("pre_lrelu_slope", C.c_float)]


CONV_EPI_SENTINEL = 1234.5                         # EV_CONV_EPI_SENTINEL: what ev_op_conv1d_epi leaves in Y's pad rows before the launch
CONV_ACTS = {"none": 0, "lrelu": 1, "tanh": 2, "silu": 3, "mish": 4, "snake": 5}


def vocoder_config(h) -> ev_vocoder_config:
    """The C form of a HiFi-GAN config dict (emojivoice_amd.hifigan.check_config has vetted it)."""
    c = ev_vocoder_config()
    c.resblock = 1 if str(h["resblock"]) == "1" else 2
    c.num_levels = len(h["upsample_rates"])
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        c.upsample_rates[i], c.upsample_kernel_sizes[i] = int(u), int(k)
    for j, (k, ds) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
        c.resblock_kernel_sizes[j] = int(k)
        for m, d in enumerate(ds):
            c.resblock_dilations[j][m] = int(d)
    return c


def vocoder_frame_bytes(h) -> int:
    """Bytes per mel frame of the widest tensor ev_hifigan plans for config h, padding excluded, and the pad frames a side
    of the mel level (ev_engine.hip: load_vocoder sets P0, plan_voc the level geometry).  V1: (32768, 4)."""
    rates, rb1 = list(h["upsample_rates"]), str(h["resblock"]) == "1"
    widest, prod, p0 = 0, 1, 4
    for i, u in enumerate(rates):
        prod *= u
        widest = max(widest, prod * (h["upsample_initial_channel"] // 2 ** (i + 1)) * 4)
        halo = 3 if i == len(rates) - 1 else 0
        for k, ds in zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"]):
            for d in (ds if rb1 else ds[:2]):
                halo = max(halo, (k - 1) * d // 2)
        p0 = max(p0, -(-halo // prod))
    return widest, p0


def build_library(force: bool = False, verbose: bool = False) -> str:
    """Compile the HIP sources for gfx950 into emojivoice_amd/lib/ (hipcc cross-compiles without a GPU)."""
    src = SOURCES[0]
    if not force and os.path.exists(LIB_PATH) and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(d) for d in SOURCES):
        return LIB_PATH
    os.makedirs(os.path.dirname(LIB_PATH), exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-value", src, "-o", LIB_PATH]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return LIB_PATH


_lib: Optional[C.CDLL] = None


def load_library() -> C.CDLL:
    """dlopen the library and declare every prototype.  Does not touch the GPU."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EvLibraryError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the EmojiVoice hot path)")
    lib = C.CDLL(LIB_PATH)
    vp, i32, f32, u64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    lib.ev_abi_version.restype = C.c_int
    lib.ev_create.argtypes = [C.POINTER(vp), i32, C.POINTER(ev_model_dims)]
    lib.ev_destroy.argtypes = [vp]
    lib.ev_destroy.restype = None
    lib.ev_last_error.argtypes = [vp]
    lib.ev_last_error.restype = C.c_char_p
    for f in (lib.ev_load_estimator, lib.ev_load_vocoder, lib.ev_load_text_encoder):
        f.argtypes = [vp, vp, C.POINTER(ev_tensor_index), u64]
    lib.ev_load_vocoder_cfg.argtypes = [vp, vp, C.POINTER(ev_tensor_index), u64, C.POINTER(ev_vocoder_config)]
    lib.ev_set_mrf_streams_max.argtypes = [vp, i32]
    lib.ev_set_mrf_streams_max.restype = i32
    lib.ev_workspace_bytes.argtypes = [vp, i32, i32, i32]
    lib.ev_workspace_bytes.restype = u64
    lib.ev_cfm_decode.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, vp, vp]
    lib.ev_cfm_decode2.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp, f32, f32, vp, vp]
    lib.ev_reserve.argtypes = [vp, i32, i32, i32, i32, vp]
    lib.ev_alloc_count.argtypes = [vp]
    lib.ev_alloc_count.restype = C.c_int64
    lib.ev_dbg_sk_stats.argtypes = [vp, C.POINTER(C.c_uint32)]
    lib.ev_estimator.argtypes = [vp, vp, vp, vp, vp, f32, i32, i32, vp, vp]
    lib.ev_estimator_rows.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, vp, vp]
    lib.ev_cfm_loss.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, vp, vp, vp]
    lib.ev_hifigan.argtypes = [vp, vp, i32, i32, vp, vp]
    lib.ev_text_encoder.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, vp]
    lib.ev_text_encoder_status.argtypes = [vp, vp]
    lib.ev_dbg_conv_bench.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(C.c_float)]
    lib.ev_stft_magnitude.argtypes = [vp, vp, i32, i32, vp, vp]
    lib.ev_align.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]
    lib.ev_denoise.argtypes = [vp, vp, i32, i32, vp, f32, vp, vp]
    lib.ev_load_mel_basis.argtypes = [vp, vp, i32, i32]
    lib.ev_mel_spectrogram.argtypes = [vp, vp, i32, i32, f32, f32, vp, vp]
    lib.ev_load_resampler.argtypes = [vp, vp, i32, i32, i32]
    lib.ev_resample.argtypes = [vp, vp, vp, i32, i32, vp, i32, vp]
    lib.ev_mel_stats.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp]
    lib.ev_trim_bounds.argtypes = [vp, vp, vp, i32, i32, i32, i32, f32, vp, vp, vp]
    lib.ev_trim_apply.argtypes = [vp, vp, vp, vp, f32, i32, i32, vp, i32, vp, vp]
    lib.ev_pitch_yin.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, vp, vp, vp, vp]
    lib.ev_dtw.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp]
    lib.ev_loudness.argtypes = [vp, vp, vp, i32, i32, i32, vp, C.c_double, vp, vp, vp, vp, vp]
    f64 = C.c_double
    lib.ev_pyin_observe.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, f64, f64, i32, i32, vp, i32, f64, f64, vp, vp, vp]
    lib.ev_pyin_decode.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, f64, f64, vp, vp, vp, vp]
    lib.ev_load_stoi.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32]
    lib.ev_stoi.argtypes = [vp, vp, vp, vp, i32, i32, C.c_double, C.c_double, vp, vp, vp, vp, vp, vp]
    lib.ev_load_stft_dist.argtypes = [vp, vp, vp, i32, i32, i32]
    lib.ev_stft_dist.argtypes = [vp, vp, vp, vp, i32, i32, C.c_double, vp, vp, vp, vp]
    lib.ev_load_voice_quality.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, i32, i32, i32, vp, C.c_double]
    lib.ev_voice_quality.argtypes = [vp, vp, vp, i32, i32, C.c_double, vp, vp, vp, vp]
    lib.ev_load_formants.argtypes = [vp, vp, i32, i32, i32, C.c_double, C.c_double, C.c_double, i32]
    lib.ev_formants.argtypes = [vp, vp, vp, i32, i32, C.c_double, vp, vp, vp, vp]
    lib.ev_formant_track.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, C.c_double, C.c_double, C.c_double, vp, vp, vp, vp, vp]
    lib.ev_perturbation.argtypes = [vp, vp, vp, i32, i32, i32, vp, i32, i32, C.c_double, C.c_double, C.c_double, vp, vp, vp, vp]
    lib.ev_load_harmonics.argtypes = [vp, vp, vp, i32, i32, i32, C.c_double, i32, C.c_double, C.c_double, C.c_double]
    lib.ev_harmonics.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, i32, C.c_double, vp, vp, vp, vp]
    lib.ev_functionals.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, i32, vp, vp, vp]
    lib.ev_modulation.argtypes = [vp, vp, vp, vp, i32, i32, i32, C.c_double, C.c_double, i32, i32, C.c_double, vp, i32, vp, vp, vp, vp, vp, vp]
    lib.ev_load_auditory.argtypes = [vp, vp, vp, i32, i32, i32, vp, i32, vp, vp, i32, i32, i32, C.c_double]
    lib.ev_auditory.argtypes = [vp, vp, vp, i32, i32, C.c_double, vp, vp, vp, vp, vp]
    lib.ev_load_srmr.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32]
    lib.ev_srmr.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp]
    lib.ev_load_speech_rate.argtypes = [vp, vp, i32, i32]
    lib.ev_speech_rate.argtypes = [vp, vp, vp, vp, i32, i32, C.c_double, C.c_double, C.c_double, C.c_double, i32, i32, vp, vp, vp, vp, vp]
    lib.ev_load_envelope.argtypes = [vp, vp, i32, i32, C.c_double, C.c_double, C.c_double, vp, i32]
    lib.ev_envelope.argtypes = [vp, vp, vp, vp, i32, i32, C.c_double, vp, vp, vp, vp]
    lib.ev_load_phase_vocoder.argtypes = [vp, vp, vp, i32]
    lib.ev_phase_vocoder.argtypes = [vp, vp, vp, i32, i32, C.c_double, vp, i32, vp, vp, vp, vp]
    lib.ev_maximum_path.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]
    lib.ev_log_prior.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp]
    lib.ev_mas_align.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]
    lib.ev_profile_enable.argtypes = [vp, i32]
    lib.ev_profile_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64), i32]
    lib.ev_profile_read_split.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    lib.ev_dbg_last_cfg.argtypes = [vp]
    lib.ev_set_arithmetic.argtypes = [vp, i32]
    lib.ev_get_arithmetic.argtypes = [vp]
    lib.ev_dbg_set_amax.argtypes = [vp, i32]
    lib.ev_dbg_set_attn_h16.argtypes = [vp, i32]
    lib.ev_dbg_set_chain.argtypes = [vp, i32]
    lib.ev_dbg_sk_taken.argtypes = [vp]
    lib.ev_dbg_sk_taken.restype = C.c_int64
    lib.ev_op_conv1d.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, f32, vp, vp]
    lib.ev_op_conv1d_epi.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(ev_conv_epi), vp, vp, vp, vp]
    lib.ev_op_groupnorm_mish.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]
    lib.ev_op_groupnorm_mish2.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, i32, vp, vp, vp]
    lib.ev_op_conv_groupnorm.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, C.POINTER(C.c_int), vp]
    lib.ev_op_layernorm.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp]
    lib.ev_op_split_pieces.argtypes = [vp, vp, i32, vp, vp]
    lib.ev_op_attention.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp]
    lib.ev_op_attn_out.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp]
    lib.ev_op_attention2.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, C.POINTER(C.c_int), vp]
    lib.ev_op_attn_out2.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, vp, f32, f32, f32, vp, C.POINTER(C.c_int), vp]
    lib.ev_op_ln_mlp.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp]
    for n in EXPORTS:
        getattr(lib, n)  # raises AttributeError if a declared symbol is not exported
    _lib = lib
    return lib


def _stream_ptr() -> int:
    return int(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    """The device address of an optional tensor (None: a null pointer)."""
    return None if t is None else t.data_ptr()


class Engine:
    """One ``ev_handle`` on one GPU.  Tensors are torch CUDA tensors (fp32, contiguous)."""

    def __init__(self, device: int = 0, spk_emb_dim: int = 64, heads: int = 2):
        if not torch.cuda.is_available():
            raise EvLibraryError("no ROCm GPU visible: the EmojiVoice hot path has no CPU fallback")
        self.lib = load_library()
        self.device = device
        dims = ev_model_dims(80, spk_emb_dim, 256, heads, 64)
        h = C.c_void_p()
        rc = self.lib.ev_create(C.byref(h), device, C.byref(dims))
        if rc != 0:
            raise EvLibraryError(f"ev_create failed with code {rc}")
        self.h = h
        self.spk_emb_dim = spk_emb_dim
        env = os.environ.get("EV_MRF_STREAMS_MAX", "")   # the handle's default: ev_create reads the same variable the same way (empty = unset)
        if env:                                          # C: `if (fp && *fp) limit = atoi(fp)` — leading integer, 0 when there is none
            import re
            m = re.match(r"\s*([+-]?\d+)", env)
            self.mrf_streams_max = int(m.group(1)) if m else 0
        else:
            self.mrf_streams_max = 16384
        self.pipeline_owner = None                       # {holders, saved limit} while BatchPipelines hold the vocoder's fan-out off (pipeline.py)
        self.voc_frame_bytes, self.voc_pad0 = 256 * 128, 4   # widest vocoder tensor per mel frame, pad frames a side (V1 until load_vocoder says otherwise)

    def set_mrf_streams_max(self, max_frames: int) -> None:
        """Largest ``hifigan`` call (B*T mel frames) that runs its three ResBlock1 chains on three streams (0 = never)."""
        if self.lib.ev_set_mrf_streams_max(self.h, int(max_frames)) != 0:
            raise EvLibraryError(self.lib.ev_last_error(self.h).decode())
        self.mrf_streams_max = int(max_frames)

    def close(self):
        if getattr(self, "h", None):
            self.lib.ev_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise EvLibraryError(f"{what} failed: {self.lib.ev_last_error(self.h).decode()}")

    # ---- weights -----------------------------------------------------------
    def _load(self, fn, tensors: Dict[str, torch.Tensor], what: str, *extra):
        names = list(tensors.keys())
        arrs = [np.ascontiguousarray(tensors[k].detach().to("cpu", torch.float32).numpy()).reshape(-1) for k in names]
        blob = np.concatenate(arrs) if arrs else np.zeros(1, np.float32)
        idx = (ev_tensor_index * len(names))()
        off = 0
        keep = []
        for i, k in enumerate(names):
            b = k.encode()
            keep.append(b)
            shp = tuple(tensors[k].shape)
            idx[i].name = b
            idx[i].offset = off
            idx[i].ndim = len(shp)
            for d, s in enumerate(shp):
                idx[i].shape[d] = s
            off += arrs[i].size
        self._check(fn(self.h, blob.ctypes.data_as(C.c_void_p), idx, len(names), *extra), what)

    def load_estimator(self, tensors: Dict[str, torch.Tensor]):
        """``tensors``: reference ``decoder.estimator.*`` entries with that prefix stripped, plus the derived
        ``*.ff.net.0.alpha_exp`` / ``*.ff.net.0.beta_inv`` (see matcha_tts.estimator_tensors)."""
        self._load(self.lib.ev_load_estimator, tensors, "ev_load_estimator")

    def load_vocoder(self, tensors: Dict[str, torch.Tensor], h=None):
        """Generator weights (folded weight norm).  ``h``: a HiFi-GAN config inside the supported envelope (ev_load_vocoder_cfg); None: V1."""
        if h is None:
            self._load(self.lib.ev_load_vocoder, tensors, "ev_load_vocoder")
            self.voc_frame_bytes, self.voc_pad0 = 256 * 128, 4
            return
        cfg = vocoder_config(h)
        self._load(self.lib.ev_load_vocoder_cfg, tensors, "ev_load_vocoder_cfg", C.byref(cfg))
        self.voc_frame_bytes, self.voc_pad0 = vocoder_frame_bytes(h)

    def align(self, w_ceil, mu_x, x_lengths, y_lengths, Tp: int, want_attn: bool = True):
        """generate_path + mu_y = attn^T mu_x (utils/model.py:29-41, matcha_tts.py:131-135).  Returns (mu_y (B,80,Tp), attn (B,1,Tx,Tp))."""
        w = self._f32(w_ceil).reshape(w_ceil.shape[0], -1)
        mu_x = self._f32(mu_x)
        B, F, Tx = mu_x.shape
        assert F == 80 and w.shape == (B, Tx)
        xl = x_lengths.to(mu_x.device, torch.int32).contiguous()
        yl = y_lengths.to(mu_x.device, torch.int64).contiguous()
        mu_y = torch.empty((B, F, Tp), dtype=torch.float32, device=mu_x.device)
        attn = torch.empty((B, 1, Tx, Tp), dtype=torch.float32, device=mu_x.device) if want_attn else None
        self._check(self.lib.ev_align(self.h, w.data_ptr(), mu_x.data_ptr(), xl.data_ptr(), yl.data_ptr(), B, Tx, int(Tp), mu_y.data_ptr(),
                                      attn.data_ptr() if attn is not None else None, _stream_ptr()), "ev_align")
        return mu_y, attn

    def stft_magnitude(self, audio):
        """|STFT| (B, 513, L/256 + 1) of (B, L) audio with the denoiser's STFT (denoiser.py:36-56)."""
        audio = self._f32(audio)
        B, L = audio.shape
        mag = torch.empty((B, 513, L // 256 + 1), dtype=torch.float32, device=audio.device)
        self._check(self.lib.ev_stft_magnitude(self.h, audio.data_ptr(), B, L, mag.data_ptr(), _stream_ptr()), "ev_stft_magnitude")
        return mag

    def denoise(self, audio, bias_spec, strength: float):
        """Denoiser.forward (denoiser.py:58-64) on (B, L) audio; bias_spec (513,)."""
        audio = self._f32(audio)
        B, L = audio.shape
        bias = self._f32(bias_spec).reshape(-1)
        assert bias.numel() == 513
        out = torch.empty_like(audio)
        self._check(self.lib.ev_denoise(self.h, audio.data_ptr(), B, L, bias.data_ptr(), float(strength), out.data_ptr(), _stream_ptr()), "ev_denoise")
        return out

    def load_mel_basis(self, basis) -> None:
        """The mel filter bank (n_mels, 513) of ``mel_spectrogram`` (ev_load_mel_basis); a host array or tensor."""
        b = np.ascontiguousarray(torch.as_tensor(basis).detach().to("cpu", torch.float32).numpy())
        if b.ndim != 2:
            raise ValueError(f"mel basis must be (n_mels, n_freq), got shape {b.shape}")
        self._check(self.lib.ev_load_mel_basis(self.h, b.ctypes.data_as(C.c_void_p), b.shape[0], b.shape[1]), "ev_load_mel_basis")
        self.n_mels = int(b.shape[0])

    def mel_spectrogram(self, audio, out_scale: float = 1.0, out_shift: float = 0.0):
        """log-mel (B, n_mels, L/256) of (B, L) audio: the reference's ``mel_spectrogram`` at n_fft 1024 / hop 256 / center=False
        (utils/audio.py:45-82), times ``out_scale`` plus ``out_shift`` (ev_mel_spectrogram)."""
        audio = self._f32(audio)
        B, L = audio.shape
        n_mels = getattr(self, "n_mels", 0)
        mel = torch.empty((B, n_mels, L // 256), dtype=torch.float32, device=audio.device)
        self._check(self.lib.ev_mel_spectrogram(self.h, audio.data_ptr(), B, L, float(out_scale), float(out_shift), mel.data_ptr(), _stream_ptr()),
                    "ev_mel_spectrogram")
        return mel

    def load_resampler(self, taps, up: int, down: int) -> None:
        """The FIR of ``resample`` (ev_load_resampler): ``taps`` (n_taps,) on the host, carrying the gain ``up``; n_taps odd,
        gcd(up, down) = 1, 1 <= up, down <= 640.  ``audio.resample_filter`` makes scipy's default."""
        t = np.ascontiguousarray(torch.as_tensor(taps).detach().to("cpu", torch.float32).numpy()).reshape(-1)
        self._check(self.lib.ev_load_resampler(self.h, t.ctypes.data_as(C.c_void_p), int(t.shape[0]), int(up), int(down)), "ev_load_resampler")
        self.rs_ratio = (int(up), int(down))

    def resample(self, x, lengths=None):
        """(B, L) -> (B, ceil(L * up / down)) by the loaded polyphase filter (ev_resample): scipy.signal.resample_poly with zero padding.
        ``lengths`` (B,): samples per row (None: L); a row's outputs past ceil(len * up / down) are zeros."""
        x, B, L, ln = self._rows(x, lengths, "resample")
        up, down = getattr(self, "rs_ratio", (1, 1))
        L_out = -(-L * up // down)
        y = torch.empty((B, L_out), dtype=torch.float32, device=x.device)
        self._check(self.lib.ev_resample(self.h, x.data_ptr(), _ptr(ln), B, L, y.data_ptr(), L_out, _stream_ptr()), "ev_resample")
        return y

    def mel_stats(self, mel, lengths):
        """(B, 2) float64 on the device: per row sum x and sum x^2 over its lengths[b] x C valid cells of ``mel`` (B, C, T) (ev_mel_stats)."""
        mel = self._f32(mel)
        B, Cc, T = mel.shape
        ln = torch.as_tensor(lengths).to(mel.device, torch.int32).contiguous()
        if ln.numel() != B:
            raise ValueError(f"mel_stats: {B} lengths expected, got {ln.numel()}")
        sums = torch.empty((B, 2), dtype=torch.float64, device=mel.device)
        self._check(self.lib.ev_mel_stats(self.h, mel.data_ptr(), ln.data_ptr(), B, Cc, T, sums.data_ptr(), _stream_ptr()), "ev_mel_stats")
        return sums

    def trim_bounds(self, x, lengths=None, top_db: float = 60.0, frame_length: int = 2048, hop_length: int = 512, want_peak: bool = True):
        """librosa.effects.trim's bounds for every row of ``x`` (B, L) (ev_trim_bounds): (bounds (B, 2) int32 {start, end}, peak (B,) fp32
        = max |x| over the whole row, or None), both on the device.  ``lengths`` (B,): samples per row (None: L).  hop_length a multiple
        of 64 up to 4096, frame_length a multiple of it, frame_length / hop_length <= 64."""
        x, B, L, ln = self._rows(x, lengths, "trim_bounds")
        bounds = torch.empty((B, 2), dtype=torch.int32, device=x.device)
        peak = torch.empty((B,), dtype=torch.float32, device=x.device) if want_peak else None
        self._check(self.lib.ev_trim_bounds(self.h, x.data_ptr(), _ptr(ln), B, L, int(frame_length), int(hop_length), float(top_db),
                                            bounds.data_ptr(), _ptr(peak), _stream_ptr()), "ev_trim_bounds")
        return bounds, peak

    def trim_apply(self, x, bounds, peak=None, target_peak: float = 0.0, out_len: Optional[int] = None):
        """y[b, j] = x[b, start[b] + j] * gain[b] (ev_trim_apply): (y (B, L_out), out_len (B,) int32) on the device, zeros right of each
        row's out_len.  ``bounds`` (B, 2) int32 and ``peak`` (B,) fp32 are device tensors (those of ``trim_bounds``); gain is
        target_peak / peak when a peak is given, target_peak > 0 and the peak > 0, else 1.  ``out_len``: L_out (None: L); longer rows are
        truncated to it."""
        x, B, L, _ = self._rows(x, None, "trim_apply")
        bounds = torch.as_tensor(bounds).to(x.device, torch.int32).contiguous()
        if tuple(bounds.shape) != (B, 2):
            raise ValueError(f"trim_apply: bounds must be ({B}, 2), got shape {tuple(bounds.shape)}")
        pk = None if peak is None else self._f32(torch.as_tensor(peak).to(x.device))
        if pk is not None and pk.numel() != B:
            raise ValueError(f"trim_apply: {B} peaks expected, got {pk.numel()}")
        L_out = L if out_len is None else int(out_len)
        y = torch.empty((B, max(L_out, 1)), dtype=torch.float32, device=x.device)
        n = torch.empty((B,), dtype=torch.int32, device=x.device)
        self._check(self.lib.ev_trim_apply(self.h, x.data_ptr(), bounds.data_ptr(), _ptr(pk), float(target_peak), B, L,
                                           y.data_ptr(), L_out, n.data_ptr(), _stream_ptr()), "ev_trim_apply")
        return y, n

    def pitch_yin(self, x, lengths=None, frame_length: int = 1024, hop_length: int = 256, tau_min: int = 36, tau_max: int = 340,
                  threshold: float = 0.1, want_lag: bool = True, want_period: bool = True, want_cmnd: bool = True):
        """YIN per frame of every row of ``x`` (B, L) (ev_pitch_yin): (lag (B, F) int32, period (B, F) fp32 in samples, cmnd (B, F) fp32) on
        the device, F = ceil(L / hop_length); an output that is not wanted is None.  Unvoiced frames have lag 0 and period 0, and cmnd =
        min d' over [tau_min, tau_max].  ``lengths`` (B,): samples per row (None: L); frames past ceil(len / hop_length) are zeros."""
        x, B, L, ln = self._rows(x, lengths, "pitch_yin")
        F = -(-L // max(int(hop_length), 1))
        lag = torch.empty((B, F), dtype=torch.int32, device=x.device) if want_lag else None
        period = torch.empty((B, F), dtype=torch.float32, device=x.device) if want_period else None
        cmnd = torch.empty((B, F), dtype=torch.float32, device=x.device) if want_cmnd else None
        self._check(self.lib.ev_pitch_yin(self.h, x.data_ptr(), _ptr(ln), B, L, int(frame_length), int(hop_length), int(tau_min), int(tau_max),
                                          float(threshold), _ptr(lag), _ptr(period), _ptr(cmnd), _stream_ptr()), "ev_pitch_yin")
        return lag, period, cmnd

    DTW_METRICS = {"euclidean": 0, "sqeuclidean": 1}

    def dtw(self, x, y, x_lengths=None, y_lengths=None, metric="euclidean", want_path: bool = True):
        """Dynamic time warping of ``x`` (B, C, Tx) against ``y`` (B, C, Ty) (ev_dtw): (cost (B,) float64, steps (B,) int32, path
        (B, Tx + Ty - 1, 2) int32 or None) on the device.  Row b's path holds (i, j) for k < steps[b], ascending from (0, 0), and (-1, -1)
        behind.  ``x_lengths`` / ``y_lengths`` (B,): frames per row (None: the padded size).  ``metric``: "euclidean" (0) or "sqeuclidean"
        (1), or the integer itself."""
        x, y = self._f32(x), self._f32(y)
        if x.dim() != 3 or y.dim() != 3 or x.shape[:2] != y.shape[:2]:
            raise ValueError(f"dtw: x (B, C, Tx) and y (B, C, Ty) expected, got {tuple(x.shape)} and {tuple(y.shape)}")
        if isinstance(metric, str):
            if metric not in self.DTW_METRICS:
                raise ValueError(f"dtw: metric {metric!r} is none of {sorted(self.DTW_METRICS)}")
            metric = self.DTW_METRICS[metric]
        B, C, Tx = x.shape
        Ty = y.shape[2]
        lens = []
        for name, v in (("x_lengths", x_lengths), ("y_lengths", y_lengths)):
            v = None if v is None else torch.as_tensor(v).to(x.device, torch.int32).contiguous()
            if v is not None and v.numel() != B:
                raise ValueError(f"dtw: {B} {name} expected, got {v.numel()}")
            lens.append(v)
        cost = torch.empty((B,), dtype=torch.float64, device=x.device)
        steps = torch.empty((B,), dtype=torch.int32, device=x.device)
        path = torch.empty((B, max(Tx + Ty - 1, 0), 2), dtype=torch.int32, device=x.device) if want_path else None
        self._check(self.lib.ev_dtw(self.h, x.data_ptr(), y.data_ptr(), _ptr(lens[0]), _ptr(lens[1]), B, C, Tx, Ty, int(metric), cost.data_ptr(),
                                    steps.data_ptr(), _ptr(path), _stream_ptr()), "ev_dtw")
        return cost, steps, path

    def loudness(self, x, lengths, sub_len: int, coef, abs_gate: float, want_sub: bool = True, want_block: bool = True):
        """BS.1770 gated loudness of every row of ``x`` (B, L) (ev_loudness): (sub (B, L // S) float64 or None, block (B, max(L // S - 3, 0))
        float64 or None, gated (B, 2) float64 {mean square over the blocks passing both gates, over those passing the absolute gate}, counts
        (B, 3) int32 {blocks, passing the absolute gate, passing both}) on the device.  ``coef``: the 10 float64 of ``audio.k_weighting``,
        read on the host during the call; ``sub_len`` = S, the samples per 100 ms; ``abs_gate`` a mean square.  ``lengths`` (B,): samples per
        row (None: L)."""
        x, B, L, ln = self._rows(x, lengths, "loudness")
        coef = np.ascontiguousarray(np.asarray(coef, dtype=np.float64).reshape(-1))
        if coef.size != 10:
            raise ValueError(f"loudness: 10 coefficients expected, got {coef.size}")
        S = int(sub_len)
        NS = L // S if S > 0 else 0
        sub = torch.empty((B, NS), dtype=torch.float64, device=x.device) if want_sub else None
        block = torch.empty((B, max(NS - 3, 0)), dtype=torch.float64, device=x.device) if want_block else None
        gated = torch.empty((B, 2), dtype=torch.float64, device=x.device)
        counts = torch.empty((B, 3), dtype=torch.int32, device=x.device)
        self._check(self.lib.ev_loudness(self.h, x.data_ptr(), _ptr(ln), B, L, S, coef.ctypes.data, float(abs_gate), _ptr(sub), _ptr(block),
                                         gated.data_ptr(), counts.data_ptr(), _stream_ptr()), "ev_loudness")
        return sub, block, gated, counts

    def load_srmr(self, chan, mod, window, erb, cutoff, hop: int) -> None:
        """The tables of ``srmr`` (ev_load_srmr), all float64 on the host: ``chan`` (N, 3) {Re a, Im a, gain}, ``mod`` (K, 5) {b0, b1, b2, a1,
        a2}, ``window`` (4 hop,), ``erb`` (N,), ``cutoff`` (K,): what ``audio.srmr_tables`` designs."""
        f = lambda v, *shape: np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(*shape))
        ch, md, w, eb, ct = f(chan, -1, 3), f(mod, -1, 5), f(window, -1), f(erb, -1), f(cutoff, -1)
        N, K, H = int(ch.shape[0]), int(md.shape[0]), int(hop)
        if w.shape[0] != 4 * H or eb.shape[0] != N or ct.shape[0] != K:
            raise ValueError(f"load_srmr: window ({4 * H},), erb ({N},) and cutoff ({K},) expected, got {w.shape}, {eb.shape} and {ct.shape}")
        self._check(self.lib.ev_load_srmr(self.h, ch.ctypes.data, md.ctypes.data, w.ctypes.data, eb.ctypes.data, ct.ctypes.data, N, K, H), "ev_load_srmr")
        self.srmr_geometry = (N, K, H)

    def srmr(self, x, lengths, want_frame: bool = False):
        """SRMR of every row of ``x`` (B, L) at the tables' rate (ev_srmr, after load_srmr): (frame (B, NF, N, K) float64 or None, mean (B, N, K)
        float64, srmr (B, 2) float64 {ratio (0 without a frame or a denominator), bw}, counts (B, 3) int32 {frames, j90, K*}) on the device.
        ``lengths`` (B,): samples per row (None: L)."""
        if not hasattr(self, "srmr_geometry"):
            raise EvLibraryError("srmr: tables not loaded (load_srmr)")
        x, B, L, ln = self._rows(x, lengths, "srmr")
        N, K, H = self.srmr_geometry
        NF = (L - 4 * H) // H + 1 if L >= 4 * H else 0
        frame = torch.empty((B, NF, N, K), dtype=torch.float64, device=x.device) if want_frame else None
        mean = torch.empty((B, N, K), dtype=torch.float64, device=x.device)
        out = torch.empty((B, 2), dtype=torch.float64, device=x.device)
        counts = torch.empty((B, 3), dtype=torch.int32, device=x.device)
        self._check(self.lib.ev_srmr(self.h, x.data_ptr(), _ptr(ln), B, L, _ptr(frame), mean.data_ptr(), out.data_ptr(), counts.data_ptr(),
                                     _stream_ptr()), "ev_srmr")
        return frame, mean, out, counts

    def load_speech_rate(self, window, hop: int) -> None:
        """The geometry of ``speech_rate`` (ev_load_speech_rate): ``window`` (W,) float64 on the host (``audio.intensity_window``), W even with
        8 <= W <= 4096; ``hop`` a multiple of 64 with 64 <= hop <= 1024."""
        w = np.ascontiguousarray(np.asarray(window, dtype=np.float64).reshape(-1))
        self._check(self.lib.ev_load_speech_rate(self.h, w.ctypes.data, int(w.shape[0]), int(hop)), "ev_load_speech_rate")
        self.speech_rate_geometry = (int(w.shape[0]), int(hop))

    def speech_rate(self, x, lengths, voiced, power_floor: float, rank_fraction: float, silence_ratio: float, dip_ratio: float, min_pause: int,
                    min_sound: int, want_power: bool = True, want_mark: bool = True):
        """Power contour, sounding / silent segmentation and syllable nuclei of every row of ``x`` (B, L) (ev_speech_rate, after
        load_speech_rate): (power (B, NF) float64 or None, mark (B, NF) uint8 {1 sounding, 2 raw, 4 candidate, 8 nucleus} or None, stat (B, 4)
        float64 {ref, thr, mean, sd of the pause lengths in frames}, count (B, 8) int32 {frames, sounding, pauses, pause frames, candidates,
        nuclei, leading, trailing silent frames}) on the device.  ``lengths`` (B,): samples per row (None: L); ``voiced`` (B, NF) uint8 / bool or
        None: the frames a nucleus may lie on."""
        if not hasattr(self, "speech_rate_geometry"):
            raise EvLibraryError("speech_rate: tables not loaded (load_speech_rate)")
        x, B, L, ln = self._rows(x, lengths, "speech_rate")
        NF = -(-L // self.speech_rate_geometry[1])
        vc = None
        if voiced is not None:
            vc = torch.as_tensor(voiced).to(x.device).ne(0).to(torch.uint8).contiguous()
            if tuple(vc.shape) != (B, NF):
                raise ValueError(f"speech_rate: voiced must be ({B}, {NF}), got {tuple(vc.shape)}")
        power = torch.empty((B, NF), dtype=torch.float64, device=x.device) if want_power else None
        mark = torch.empty((B, NF), dtype=torch.uint8, device=x.device) if want_mark else None
        stat = torch.empty((B, 4), dtype=torch.float64, device=x.device)
        count = torch.empty((B, 8), dtype=torch.int32, device=x.device)
        self._check(self.lib.ev_speech_rate(self.h, x.data_ptr(), _ptr(ln), _ptr(vc), B, L, float(power_floor), float(rank_fraction),
                                            float(silence_ratio), float(dip_ratio), int(min_pause), int(min_sound), _ptr(power), _ptr(mark),
                                            stat.data_ptr(), count.data_ptr(), _stream_ptr()), "ev_speech_rate")
        return power, mark, stat, count

    def load_envelope(self, twiddle, H: int, nfft: int, sr: float, warp, default_period: float = 0.0, q1: float = -0.15) -> None:
        """One geometry of ``envelope`` (ev_load_envelope), the tables on the host: ``twiddle`` (nfft, 2) float64 {cos, sin}(2 pi n / nfft),
        ``H`` the hop, the rate ``sr`` in Hz, ``warp`` (n_mcep, nfft / 2 + 1) float64 (``audio.freq_warp_matrix``), ``default_period`` in samples
        for the frames without a usable period (0: sr / 500) and the lifter's ``q1``."""
        tw = np.ascontiguousarray(np.asarray(twiddle, dtype=np.float64).reshape(-1, 2))
        wp = np.ascontiguousarray(np.asarray(warp, dtype=np.float64))
        NB = int(nfft) // 2 + 1
        if tw.shape[0] != int(nfft) or wp.ndim != 2 or wp.shape[1] != NB:
            raise ValueError(f"load_envelope: {nfft} twiddles and warp (n_mcep, {NB}) expected, got {tw.shape[0]} and {tuple(wp.shape)}")
        self._check(self.lib.ev_load_envelope(self.h, tw.ctypes.data, int(H), int(nfft), float(sr), float(default_period), float(q1), wp.ctypes.data,
                                              int(wp.shape[0])), "ev_load_envelope")
        self.envelope_geometry = (int(H), int(nfft), int(wp.shape[0]))

    def envelope(self, x, lengths, period, power_floor: float, want_envelope: bool = False):
        """CheapTrick's envelope and its mel-cepstrum for every frame of every row of ``x`` (B, L) (ev_envelope, after load_envelope):
        (env (B, NF, NB) float64: the log power envelope in nepers, or None; mcep (B, NF, n_mcep) float64; cls (B, NF, 3) int32: {class, half,
        kd}) on the device, NF = ceil(L / H).  ``period`` (B, NF) float32: ev_pitch_yin's periods in samples, 0 where unvoiced; ``lengths``
        (B,): samples per row (None: L)."""
        if not hasattr(self, "envelope_geometry"):
            raise EvLibraryError("envelope: tables not loaded (load_envelope)")
        x, B, L, ln = self._rows(x, lengths, "envelope")
        H, nfft, NM = self.envelope_geometry
        NF = -(-L // H)
        pd = torch.as_tensor(period, device=x.device).to(torch.float32).contiguous()
        if tuple(pd.shape) != (B, NF):
            raise ValueError(f"envelope: period must be ({B}, {NF}), got {tuple(pd.shape)}")
        env = torch.empty((B, NF, nfft // 2 + 1), dtype=torch.float64, device=x.device) if want_envelope else None
        mcep = torch.empty((B, NF, NM), dtype=torch.float64, device=x.device)
        cls = torch.empty((B, NF, 3), dtype=torch.int32, device=x.device)
        self._check(self.lib.ev_envelope(self.h, x.data_ptr(), _ptr(ln), pd.data_ptr(), B, L, float(power_floor), _ptr(env), mcep.data_ptr(),
                                         cls.data_ptr(), _stream_ptr()), "ev_envelope")
        return env, mcep, cls

    def load_phase_vocoder(self, window, twiddle, nfft: int) -> None:
        """One nfft of ``phase_vocoder`` (ev_load_phase_vocoder), the tables on the host: ``window`` (nfft,) float64 (the periodic Hann window for
        librosa's defaults), ``twiddle`` (nfft, 2) float64 {cos, sin}(2 pi n / nfft).  The hop is nfft / 4."""
        w = np.ascontiguousarray(np.asarray(window, dtype=np.float64).reshape(-1))
        tw = np.ascontiguousarray(np.asarray(twiddle, dtype=np.float64).reshape(-1, 2))
        if w.shape[0] != int(nfft) or tw.shape[0] != int(nfft):
            raise ValueError(f"load_phase_vocoder: a window and twiddles of {nfft} entries expected, got {w.shape[0]} and {tw.shape[0]}")
        self._check(self.lib.ev_load_phase_vocoder(self.h, w.ctypes.data, tw.ctypes.data, int(nfft)), "ev_load_phase_vocoder")
        self.phase_vocoder_nfft = int(nfft)

    def phase_vocoder(self, x, lengths, rate: float, want_counts: bool = False, want_stretch: bool = False):
        """Every row of ``x`` (B, L) rendered ``rate`` times faster at its own pitch (ev_phase_vocoder, after load_phase_vocoder): (y (B, L_out)
        float32 with L_out = rint(L / rate), out_len (B,) int32, counts (B, 2) int32 {frames in, frames out} or None, stretch (B, NO, NB, 2)
        float64 — the stretched spectra {re, im} — or None) on the device.  ``lengths`` (B,): samples per row (None: L)."""
        if not hasattr(self, "phase_vocoder_nfft"):
            raise EvLibraryError("phase_vocoder: tables not loaded (load_phase_vocoder)")
        x, B, L, ln = self._rows(x, lengths, "phase_vocoder")
        nfft, rate = self.phase_vocoder_nfft, float(rate)
        if not (math.isfinite(rate) and 0.125 <= rate <= 8.0):
            raise ValueError(f"phase_vocoder: rate must be finite with 0.125 <= rate <= 8 (got {rate})")
        L_out = int(np.rint(np.float64(L) / np.float64(rate)))
        NO = int(np.ceil(np.float64(1 + L // (nfft // 4)) / np.float64(rate)))
        y = torch.empty((B, L_out), dtype=torch.float32, device=x.device)
        out_len = torch.empty((B,), dtype=torch.int32, device=x.device)
        counts = torch.empty((B, 2), dtype=torch.int32, device=x.device) if want_counts else None
        st = torch.empty((B, NO, nfft // 2 + 1, 2), dtype=torch.float64, device=x.device) if want_stretch else None
        self._check(self.lib.ev_phase_vocoder(self.h, x.data_ptr(), _ptr(ln), B, L, rate, y.data_ptr(), L_out, out_len.data_ptr(), _ptr(counts),
                                              _ptr(st), _stream_ptr()), "ev_phase_vocoder")
        return y, out_len, counts, st

    def load_stoi(self, window, twiddle, bands, hop: int, n_fft: int, seg_frames: int) -> None:
        """The tables of ``stoi`` (ev_load_stoi), all on the host: ``window`` (W,) float64 with W = 2 hop, ``twiddle`` (n_fft, 2) float64
        {cos, sin}(2 pi n / n_fft), ``bands`` (n_bands, 2) int32 {first bin, end bin}; ``seg_frames`` = N, the frames per segment."""
        w = np.ascontiguousarray(np.asarray(window, dtype=np.float64).reshape(-1))
        tw = np.ascontiguousarray(np.asarray(twiddle, dtype=np.float64).reshape(-1, 2))
        bd = np.ascontiguousarray(np.asarray(bands, dtype=np.int32).reshape(-1, 2))
        if tw.shape[0] != int(n_fft):
            raise ValueError(f"load_stoi: {n_fft} twiddles expected, got {tw.shape[0]}")
        self._check(self.lib.ev_load_stoi(self.h, w.ctypes.data, tw.ctypes.data, bd.ctypes.data, int(w.shape[0]), int(hop), int(n_fft), int(bd.shape[0]),
                                          int(seg_frames)), "ev_load_stoi")
        self.stoi_geometry = (int(w.shape[0]), int(hop), int(n_fft), int(bd.shape[0]), int(seg_frames))

    def stoi(self, x, y, lengths, silence_ratio: float, clip: float, want_keep: bool = True, want_tob: bool = False, want_seg: bool = True):
        """STOI / ESTOI of every processed row of ``y`` against the clean row of ``x``, both (B, L) at the measure's rate (ev_stoi, after
        load_stoi): (keep (B, NF) uint8 or None, tob (B, 2, n_bands, NM) float64 or None, seg (B, NSEG, 2) float64 or None, score (B, 2)
        float64 {STOI, ESTOI}, 0 for a row without a segment, counts (B, 3) int32 {frames, kept frames, segments}) on the device.
        ``lengths`` (B,): samples per row (None: L)."""
        x, y = self._f32(x), self._f32(y)
        if x.dim() != 2 or y.shape != x.shape:
            raise ValueError(f"stoi: x and y must be (B, L) alike, got shapes {tuple(x.shape)} and {tuple(y.shape)}")
        if not hasattr(self, "stoi_geometry"):
            raise EvLibraryError("stoi: tables not loaded (load_stoi)")
        x, B, L, ln = self._rows(x, lengths, "stoi")
        W, H, _, nb, N = self.stoi_geometry
        NF = -(-(L - W) // H) if L > W else 0
        NM = max(NF - 1, 0)
        NSEG = max(NM - N + 1, 0)
        keep = torch.empty((B, NF), dtype=torch.uint8, device=x.device) if want_keep else None
        tob = torch.empty((B, 2, nb, NM), dtype=torch.float64, device=x.device) if want_tob else None
        seg = torch.empty((B, NSEG, 2), dtype=torch.float64, device=x.device) if want_seg else None
        score = torch.empty((B, 2), dtype=torch.float64, device=x.device)
        counts = torch.empty((B, 3), dtype=torch.int32, device=x.device)
        self._check(self.lib.ev_stoi(self.h, x.data_ptr(), y.data_ptr(), _ptr(ln), B, L, float(silence_ratio), float(clip), _ptr(keep), _ptr(tob), _ptr(seg),
                                     score.data_ptr(), counts.data_ptr(), _stream_ptr()), "ev_stoi")
        return keep, tob, seg, score, counts

    def load_stft_dist(self, window, twiddle, H: int, nfft: int) -> None:
        """One resolution of ``stft_dist`` (ev_load_stft_dist), the tables on the host: ``window`` (W,) float64, ``twiddle`` (nfft, 2) float64
        {cos, sin}(2 pi n / nfft); ``H`` the hop.  The handle builds the dense windowed DFT basis (W, nfft / 2 + 1) on the device."""
        w = np.ascontiguousarray(np.asarray(window, dtype=np.float64).reshape(-1))
        tw = np.ascontiguousarray(np.asarray(twiddle, dtype=np.float64).reshape(-1, 2))
        if tw.shape[0] != int(nfft):
            raise ValueError(f"load_stft_dist: {nfft} twiddles expected, got {tw.shape[0]}")
        self._check(self.lib.ev_load_stft_dist(self.h, w.ctypes.data, tw.ctypes.data, int(w.shape[0]), int(H), int(nfft)), "ev_load_stft_dist")
        self.stft_dist_geometry = (int(w.shape[0]), int(H), int(nfft))

    def stft_dist(self, x, y, lengths, power_floor: float, want_frames: bool = False):
        """The STFT-distance sums of every processed row of ``y`` against the reference row of ``x``, both (B, L), at the loaded resolution
        (ev_stft_dist, after load_stft_dist): (frame (B, NF, 4) float64 or None: per frame {sum (my - mx)^2, sum mx^2, sum |ly - lx|,
        sum (ly - lx)^2} over the bins, sums (B, 4) float64: {sum_f [0], sum_f [1], sum_f [2], sum_f sqrt([3] / NB)}, counts (B,) int32: the
        row's frames) on the device.  ``lengths`` (B,): samples per row (None: L)."""
        x, y = self._f32(x), self._f32(y)
        if x.dim() != 2 or y.shape != x.shape:
            raise ValueError(f"stft_dist: x and y must be (B, L) alike, got shapes {tuple(x.shape)} and {tuple(y.shape)}")
        if not hasattr(self, "stft_dist_geometry"):
            raise EvLibraryError("stft_dist: tables not loaded (load_stft_dist)")
        x, B, L, ln = self._rows(x, lengths, "stft_dist")
        _, H, nfft = self.stft_dist_geometry
        NF = 1 + L // H if L > nfft // 2 else 0
        frame = torch.empty((B, NF, 4), dtype=torch.float64, device=x.device) if want_frames else None
        sums = torch.empty((B, 4), dtype=torch.float64, device=x.device)
        counts = torch.empty((B,), dtype=torch.int32, device=x.device)
        self._check(self.lib.ev_stft_dist(self.h, x.data_ptr(), y.data_ptr(), _ptr(ln), B, L, float(power_floor), _ptr(frame), sums.data_ptr(),
                                          counts.data_ptr(), _stream_ptr()), "ev_stft_dist")
        return frame, sums, counts

    def load_voice_quality(self, window, twiddle, H: int, nfft: int, bands, slope_w, q_fit: int, q_min: int, q_max: int, fit_w, q_mean: float) -> None:
        """One geometry of ``voice_quality`` (ev_load_voice_quality), the tables on the host: ``window`` (W,) float64, ``twiddle`` (nfft, 2)
        float64 {cos, sin}(2 pi n / nfft), ``H`` the hop, ``bands`` (6, 2) int32 {first bin, end bin}, ``slope_w`` (2, nfft / 2 + 1) float64,
        the quefrencies, ``fit_w`` (q_max - q_fit + 1,) float64 and ``q_mean`` (``audio.voice_quality_tables`` makes them).  The handle builds
        the windowed DFT basis and the cepstral basis on the device."""
        w = np.ascontiguousarray(np.asarray(window, dtype=np.float64).reshape(-1))
        tw = np.ascontiguousarray(np.asarray(twiddle, dtype=np.float64).reshape(-1, 2))
        bd = np.ascontiguousarray(np.asarray(bands, dtype=np.int32).reshape(-1))
        sw = np.ascontiguousarray(np.asarray(slope_w, dtype=np.float64).reshape(-1))
        fw = np.ascontiguousarray(np.asarray(fit_w, dtype=np.float64).reshape(-1))
        NQ = int(q_max) - int(q_fit) + 1
        if tw.shape[0] != int(nfft) or bd.size != 12 or sw.size != 2 * (int(nfft) // 2 + 1) or fw.size != NQ:
            raise ValueError(f"load_voice_quality: {nfft} twiddles, 12 band edges, {2 * (int(nfft) // 2 + 1)} slope weights and {NQ} fit weights "
                             f"expected, got {tw.shape[0]}, {bd.size}, {sw.size} and {fw.size}")
        self._check(self.lib.ev_load_voice_quality(self.h, w.ctypes.data, tw.ctypes.data, int(w.shape[0]), int(H), int(nfft), bd.ctypes.data,
                                                   sw.ctypes.data, int(q_fit), int(q_min), int(q_max), fw.ctypes.data, float(q_mean)),
                    "ev_load_voice_quality")
        self.voice_quality_geometry = (int(w.shape[0]), int(H), int(nfft), NQ)

    def voice_quality(self, x, lengths, power_floor: float, want_cepstrum: bool = False):
        """The voice-quality figures of every frame of every row of ``x`` (B, L) at the loaded geometry (ev_voice_quality, after
        load_voice_quality): (frame (B, NF, 8) float64: per frame {cpp, alpha ratio, Hammarberg index, slope 0, slope 1, power, C[q*], the
        baseline at q*}, peak (B, NF) int32: q*, cepstrum (B, NF, NQ) float64 or None) on the device, NF = ceil(L / H).  ``lengths`` (B,):
        samples per row (None: L)."""
        if not hasattr(self, "voice_quality_geometry"):
            raise EvLibraryError("voice_quality: tables not loaded (load_voice_quality)")
        x, B, L, ln = self._rows(x, lengths, "voice_quality")
        _, H, _, NQ = self.voice_quality_geometry
        NF = -(-L // H)
        frame = torch.empty((B, NF, 8), dtype=torch.float64, device=x.device)
        peak = torch.empty((B, NF), dtype=torch.int32, device=x.device)
        cep = torch.empty((B, NF, NQ), dtype=torch.float64, device=x.device) if want_cepstrum else None
        self._check(self.lib.ev_voice_quality(self.h, x.data_ptr(), _ptr(ln), B, L, float(power_floor), frame.data_ptr(), peak.data_ptr(), _ptr(cep),
                                              _stream_ptr()), "ev_voice_quality")
        return frame, peak, cep

    def load_formants(self, window, H: int, order: int, pre_emphasis: float, sr: float, f_lo: float, n_formants: int) -> None:
        """One geometry of ``formants`` (ev_load_formants): ``window`` (W,) float64 on the host (``audio.formant_window``), ``H`` the hop, the
        order of the linear prediction, the pre-emphasis coefficient, the rate ``sr`` of the rows in Hz, the band edge ``f_lo`` in Hz (roots at
        or below f_lo and at or above sr / 2 - f_lo are no formants) and the number of formants kept per frame."""
        w = np.ascontiguousarray(np.asarray(window, dtype=np.float64).reshape(-1))
        self._check(self.lib.ev_load_formants(self.h, w.ctypes.data, int(w.shape[0]), int(H), int(order), float(pre_emphasis), float(sr), float(f_lo),
                                              int(n_formants)), "ev_load_formants")
        self.formants_geometry = (int(w.shape[0]), int(H), int(order), int(n_formants))

    def formants(self, x, lengths, power_floor: float, want_lpc: bool = True):
        """The formants of every frame of every row of ``x`` (B, L) at the loaded geometry (ev_formants, after load_formants): (lpc (B, NF,
        order + 2) float64 or None: per frame a_1 .. a_p, the gain and E0; formant (B, NF, n_formants, 2) float64: frequency and bandwidth in
        Hz, lowest frequency first, zeros past count; count (B, NF) int32: the formants found, -1 where the root finder did not converge) on
        the device, NF = ceil(L / H).  ``lengths`` (B,): samples per row (None: L)."""
        if not hasattr(self, "formants_geometry"):
            raise EvLibraryError("formants: tables not loaded (load_formants)")
        x, B, L, ln = self._rows(x, lengths, "formants")
        _, H, order, nform = self.formants_geometry
        NF = -(-L // H)
        lpc = torch.empty((B, NF, order + 2), dtype=torch.float64, device=x.device) if want_lpc else None
        formant = torch.empty((B, NF, nform, 2), dtype=torch.float64, device=x.device)
        count = torch.empty((B, NF), dtype=torch.int32, device=x.device)
        self._check(self.lib.ev_formants(self.h, x.data_ptr(), _ptr(ln), B, L, float(power_floor), _ptr(lpc), formant.data_ptr(), count.data_ptr(),
                                         _stream_ptr()), "ev_formants")
        return lpc, formant, count

    def formant_track(self, formant, count, n_tracks: int, reference, cost_f: float = 1.0, cost_b: float = 1.0, cost_j: float = 1.0,
                      want_cost: bool = True, back=None):
        """Tracks through the candidates ``formants`` wrote (ev_formant_track; no load step): ``formant`` (B, NF, n_cand, 2) float64 and ``count``
        (B, NF) int32 on the GPU, ``reference`` the ``n_tracks`` reference frequencies in Hz on the host: (track (B, NF, n_tracks, 2) float64: the
        chosen candidates, zeros on gaps; sel (B, NF) int32: the state, -1 on gaps; cost (B, NF) float64 or None: each segment's optimum at its
        last frame) on the device.  ``back``: (B, NF, S) int16 scratch (16-bit words) to use instead of a new tensor, S = C(n_cand, n_tracks)."""
        if formant.dtype != torch.float64 or formant.dim() != 4 or formant.shape[3] != 2 or count.dtype != torch.int32 or tuple(count.shape) != tuple(formant.shape[:2]):
            raise ValueError(f"formant_track: float64 formant (B, NF, n_cand, 2) and int32 count (B, NF) expected, got {formant.dtype} "
                             f"{tuple(formant.shape)} and {count.dtype} {tuple(count.shape)}")
        if not formant.is_cuda or count.device != formant.device:
            raise EvLibraryError("no CPU fallback: formant_track needs its inputs on one GPU")
        formant, count = formant.contiguous(), count.contiguous()
        B, NF, nc, _ = formant.shape
        nt = int(n_tracks)
        ref = np.ascontiguousarray(np.asarray(reference, dtype=np.float64).reshape(-1))
        if ref.size != nt:
            raise ValueError(f"formant_track: reference must hold n_tracks = {nt} values, got {ref.size}")
        S = math.comb(nc, nt) if 1 <= nt <= nc else 1
        if S <= 1024:                                                    # (over it the library fails with its message; nothing is allocated for it)
            if back is None:
                back = torch.empty((B, NF, S), dtype=torch.int16, device=formant.device)
            elif back.dtype != torch.int16 or back.numel() < B * NF * S or not back.is_contiguous():
                raise ValueError(f"formant_track: back must be contiguous int16 with at least {B * NF * S} elements")
        track = torch.empty((B, NF, max(nt, 0), 2), dtype=torch.float64, device=formant.device)
        sel = torch.empty((B, NF), dtype=torch.int32, device=formant.device)
        cost = torch.empty((B, NF), dtype=torch.float64, device=formant.device) if want_cost else None
        self._check(self.lib.ev_formant_track(self.h, formant.data_ptr(), count.data_ptr(), B, NF, nc, nt, ref.ctypes.data, float(cost_f), float(cost_b),
                                              float(cost_j), _ptr(back), track.data_ptr(), sel.data_ptr(), _ptr(cost), _stream_ptr()),
                    "ev_formant_track")
        return track, sel, cost

    def perturbation(self, x, lengths, lag, hop_length: int, n_cycles: int, corr_length: int, period_factor: float = 1.3,
                     amplitude_factor: float = 1.6, power_floor: float = 1e-10, want_marks: bool = True):
        """Jitter, shimmer and the harmonic strength of every frame of every row of ``x`` (B, L) at the lags ``lag`` (B, F) int32 that
        ``pitch_yin`` wrote (ev_perturbation; no load step): (frame (B, F, 8) float64: local jitter, absolute jitter in samples, local shimmer,
        shimmer in dB, the harmonic strength r, the mean period, the mean amplitude, RAP; count (B, F, 4) int32: the periods, the counted period
        pairs, the counted amplitude pairs, the counted triples; marks (B, F, 2 n_cycles + 1) int32 or None: the pitch marks, -1 where there is
        none) on the device, F = ceil(L / hop_length).  ``lengths`` (B,): samples per row (None: L)."""
        x, B, L, ln = self._rows(x, lengths, "perturbation")
        F = -(-L // int(hop_length))
        if lag.dtype != torch.int32 or tuple(lag.shape) != (B, F) or lag.device != x.device:
            raise EvLibraryError(f"perturbation: lag must be int32 ({B}, {F}) on {x.device}, got {lag.dtype} {tuple(lag.shape)} on {lag.device}")
        lag = lag.contiguous()
        frame = torch.empty((B, F, 8), dtype=torch.float64, device=x.device)
        count = torch.empty((B, F, 4), dtype=torch.int32, device=x.device)
        marks = torch.empty((B, F, 2 * int(n_cycles) + 1), dtype=torch.int32, device=x.device) if want_marks and 1 <= int(n_cycles) <= 16 else None
        self._check(self.lib.ev_perturbation(self.h, x.data_ptr(), _ptr(ln), B, L, int(hop_length), lag.data_ptr(), int(n_cycles), int(corr_length),
                                             float(period_factor), float(amplitude_factor), float(power_floor), frame.data_ptr(), count.data_ptr(),
                                             _ptr(marks), _stream_ptr()), "ev_perturbation")
        return frame, count, marks

    def load_harmonics(self, window, twiddle, H: int, nfft: int, sr: float, n_harm: int, search: float = 0.25, min_spacing: float = 4.0,
                       a3_range: float = 0.1) -> None:
        """One geometry of ``harmonics`` (ev_load_harmonics), the tables on the host: ``window`` (W,) float64, ``twiddle`` (nfft, 2) float64
        {cos, sin}(2 pi n / nfft); ``H`` the hop, ``sr`` the rate of the rows in Hz, ``n_harm`` the harmonics kept per frame, ``search`` the half
        width of a harmonic's search range as a fraction of the spacing, ``min_spacing`` the least harmonic spacing in bins that is resolved,
        ``a3_range`` the half width of A3's range as a fraction of F3.  The handle builds the windowed DFT basis on the device."""
        w = np.ascontiguousarray(np.asarray(window, dtype=np.float64).reshape(-1))
        tw = np.ascontiguousarray(np.asarray(twiddle, dtype=np.float64).reshape(-1, 2))
        if tw.shape[0] != int(nfft):
            raise ValueError(f"load_harmonics: {nfft} twiddles expected, got {tw.shape[0]}")
        self._check(self.lib.ev_load_harmonics(self.h, w.ctypes.data, tw.ctypes.data, int(w.shape[0]), int(H), int(nfft), float(sr), int(n_harm),
                                               float(search), float(min_spacing), float(a3_range)), "ev_load_harmonics")
        self.harmonics_geometry = (int(w.shape[0]), int(H), int(nfft), int(n_harm))

    def harmonics(self, x, lengths, period, formant=None, fcount=None, power_floor: float = 1e-7, want_harm: bool = True):
        """The harmonic differences of every frame of every row of ``x`` (B, L) at the loaded geometry (ev_harmonics, after load_harmonics), at
        the periods ``period`` (B, NF) float32 that ``pitch_yin`` wrote (0: unvoiced) and, when given, the formants ``formant`` (B, NF,
        n_formants, 2) float64 and ``fcount`` (B, NF) int32 that ``formants`` wrote: (frame (B, NF, 8) float64: per frame {H1-H2, H1-A3, the
        level of the harmonic at F1, F2, F3 over H1, H1 in dB, H1 in Hz, the harmonic spacing in bins}; count (B, NF, 2) int32: the harmonics
        measured and the flags; harm (B, NF, n_harm, 2) float64 or None: {Hz, dB} of every harmonic) on the device, NF = ceil(L / H).
        ``lengths`` (B,): samples per row (None: L)."""
        if not hasattr(self, "harmonics_geometry"):
            raise EvLibraryError("harmonics: tables not loaded (load_harmonics)")
        x, B, L, ln = self._rows(x, lengths, "harmonics")
        _, H, _, n_harm = self.harmonics_geometry
        NF = -(-L // H)
        if period.dtype != torch.float32 or tuple(period.shape) != (B, NF) or period.device != x.device:
            raise EvLibraryError(f"harmonics: period must be float32 ({B}, {NF}) on {x.device}, got {period.dtype} {tuple(period.shape)} on {period.device}")
        period = period.contiguous()
        if (formant is None) != (fcount is None):
            raise EvLibraryError("harmonics: formant and fcount must both be given or both be None")
        nform = 0
        if formant is not None:
            if (formant.dtype != torch.float64 or formant.dim() != 4 or tuple(formant.shape[:2]) != (B, NF) or formant.shape[3] != 2
                    or formant.device != x.device):
                raise EvLibraryError(f"harmonics: formant must be float64 ({B}, {NF}, n_formants, 2) on {x.device}, got {formant.dtype} "
                                     f"{tuple(formant.shape)} on {formant.device}")
            if fcount.dtype != torch.int32 or tuple(fcount.shape) != (B, NF) or fcount.device != x.device:
                raise EvLibraryError(f"harmonics: fcount must be int32 ({B}, {NF}) on {x.device}, got {fcount.dtype} {tuple(fcount.shape)} on {fcount.device}")
            formant, fcount, nform = formant.contiguous(), fcount.contiguous(), int(formant.shape[2])
        frame = torch.empty((B, NF, 8), dtype=torch.float64, device=x.device)
        count = torch.empty((B, NF, 2), dtype=torch.int32, device=x.device)
        harm = torch.empty((B, NF, n_harm, 2), dtype=torch.float64, device=x.device) if want_harm else None
        self._check(self.lib.ev_harmonics(self.h, x.data_ptr(), _ptr(ln), B, L, period.data_ptr(), _ptr(formant), _ptr(fcount), nform,
                                          float(power_floor), frame.data_ptr(), count.data_ptr(), _ptr(harm), _stream_ptr()), "ev_harmonics")
        return frame, count, harm

    def load_auditory(self, window, twiddle, H: int, nfft: int, mel_w, eq, dct, k_lo: int, k_hi: int, compress: float) -> None:
        """One geometry of ``auditory`` (ev_load_auditory), the tables on the host (``audio.auditory_tables`` makes them): ``window`` (W,)
        float64, ``twiddle`` (nfft, 2) float64 {cos, sin}(2 pi n / nfft), ``H`` the hop, ``mel_w`` (nfft / 2 + 1, n_mel) float64 (no entry
        negative), ``eq`` (n_mel,) float64 (every entry positive), ``dct`` (n_mel, n_ceps) float64 (it carries the lifter), the bins
        [k_lo, k_hi) of the spectral flux and the exponent ``compress`` of the loudness.  The handle builds the windowed DFT basis on the
        device."""
        w = np.ascontiguousarray(np.asarray(window, dtype=np.float64).reshape(-1))
        tw = np.ascontiguousarray(np.asarray(twiddle, dtype=np.float64).reshape(-1, 2))
        mw = np.ascontiguousarray(np.asarray(mel_w, dtype=np.float64))
        e = np.ascontiguousarray(np.asarray(eq, dtype=np.float64).reshape(-1))
        d = np.ascontiguousarray(np.asarray(dct, dtype=np.float64))
        NB = int(nfft) // 2 + 1
        if tw.shape[0] != int(nfft) or mw.ndim != 2 or mw.shape[0] != NB or d.ndim != 2 or e.size != mw.shape[1] or d.shape[0] != mw.shape[1]:
            raise ValueError(f"load_auditory: {nfft} twiddles, mel_w ({NB}, n_mel), eq (n_mel,) and dct (n_mel, n_ceps) expected, got "
                             f"{tw.shape[0]}, {tuple(mw.shape)}, {tuple(e.shape)} and {tuple(d.shape)}")
        self._check(self.lib.ev_load_auditory(self.h, w.ctypes.data, tw.ctypes.data, int(w.shape[0]), int(H), int(nfft), mw.ctypes.data,
                                              int(mw.shape[1]), e.ctypes.data, d.ctypes.data, int(d.shape[1]), int(k_lo), int(k_hi),
                                              float(compress)), "ev_load_auditory")
        self.auditory_geometry = (int(w.shape[0]), int(H), int(nfft), int(mw.shape[1]), int(d.shape[1]))

    def auditory(self, x, lengths, power_floor: float, want_bands: bool = False):
        """The auditory descriptors of every frame of every row of ``x`` (B, L) at the loaded geometry (ev_auditory, after load_auditory): a
        dict of device tensors {"frame" (B, NF, 4) float64: per frame {loudness, spectral flux, power, log(max(power, floor))}; "mfcc" (B, NF,
        n_ceps) float64; "flags" (B, NF) int32: 1 the frame is live, 2 it has a predecessor; "bands" (B, NF, n_mel) float64 or None: the mel
        band energies}, NF = ceil(L / H).  ``lengths`` (B,): samples per row (None: L)."""
        if not hasattr(self, "auditory_geometry"):
            raise EvLibraryError("auditory: tables not loaded (load_auditory)")
        x, B, L, ln = self._rows(x, lengths, "auditory")
        _, H, _, n_mel, n_ceps = self.auditory_geometry
        NF = -(-L // H)
        frame = torch.empty((B, NF, 4), dtype=torch.float64, device=x.device)
        mfcc = torch.empty((B, NF, n_ceps), dtype=torch.float64, device=x.device)
        flags = torch.empty((B, NF), dtype=torch.int32, device=x.device)
        bands = torch.empty((B, NF, n_mel), dtype=torch.float64, device=x.device) if want_bands else None
        self._check(self.lib.ev_auditory(self.h, x.data_ptr(), _ptr(ln), B, L, float(power_floor), frame.data_ptr(), mfcc.data_ptr(),
                                         flags.data_ptr(), _ptr(bands), _stream_ptr()), "ev_auditory")
        return {"frame": frame, "mfcc": mfcc, "flags": flags, "bands": bands}

    def functionals(self, v, mask=None, lengths=None, q=(0.2, 0.5, 0.8)):
        """The functionals of every contour of ``v`` (B, K, F) float64 on the device (ev_functionals; no load step): (stat (B, K, 12 + NQ)
        float64: mean, sd, min, max, the mean and sd of the rising and of the falling slopes per frame, the mean and sd length of the runs of
        valid frames and of the gaps, then the percentile at every ``q``; count (B, K, 8) int32: the valid frames, the dropped (non-finite)
        ones, the rising parts, the falling parts, the peaks, the runs, the gaps, the adjacent pairs) on the device.  ``mask`` (B, K, F) uint8 or
        bool beside v, or None: the frames that count; ``lengths`` (B,): frames per row (None: F); ``q``: up to 16 numbers in [0, 1], read on
        the host during the call.  A statistic over no terms is 0."""
        if v.dtype != torch.float64 or v.dim() != 3:
            raise EvLibraryError(f"functionals: v must be float64 (B, K, F), got {v.dtype} {tuple(v.shape)}")
        v = v.contiguous()
        B, K, F = v.shape
        if mask is not None:
            if tuple(mask.shape) != (B, K, F) or mask.device != v.device or mask.dtype not in (torch.uint8, torch.bool):
                raise EvLibraryError(f"functionals: mask must be uint8 or bool ({B}, {K}, {F}) on {v.device}, got {mask.dtype} {tuple(mask.shape)} "
                                     f"on {mask.device}")
            mask = mask.contiguous()
        ln = None if lengths is None else torch.as_tensor(lengths).to(v.device, torch.int32).contiguous()
        if ln is not None and ln.numel() != B:
            raise ValueError(f"functionals: {B} lengths expected, got {ln.numel()}")
        qa = np.ascontiguousarray(np.asarray(q, dtype=np.float64).reshape(-1))
        NQ = int(qa.shape[0])
        stat = torch.empty((B, K, 12 + max(min(NQ, 16), 0)), dtype=torch.float64, device=v.device)
        count = torch.empty((B, K, 8), dtype=torch.int32, device=v.device)
        self._check(self.lib.ev_functionals(self.h, v.data_ptr(), _ptr(mask), _ptr(ln), B, K, F, qa.ctypes.data if NQ else None, NQ,
                                            stat.data_ptr(), count.data_ptr(), _stream_ptr()), "ev_functionals")
        return stat, count

    def modulation(self, v, mask, lengths, nu0: float, dnu: float, NM: int, min_run: int, min_cycles: float = 2.0, bands=()):
        """The modulation spectrum of every contour of ``v`` (B, K, F) float64 on the device (ev_modulation; no load step): (spec (B, K, NM)
        float64: the power at nu0 + j dnu cycles per frame, pooled over the runs of at least ``min_run`` valid frames that hold at least
        ``min_cycles`` cycles of it; weight (B, K, NM) int32: the frames behind each; peak (B, K, NBAND, 4) float64: per band the interpolated
        frequency in cycles per frame, the amplitude, the band's mean power and the peak's power over it, zeros without a peak; stat (B, K, 2):
        the variance the lines leave, the mean slope per frame; count (B, K, 4 + NBAND) int32: the valid frames, the dropped (non-finite) ones,
        the analysed runs, the analysed frames, then per band the peak's grid index or -1) on the device.  ``mask`` and ``lengths`` as for
        ``functionals``; ``bands``: up to four (j_lo, j_hi) index pairs, read on the host."""
        if v.dim() != 3 or v.dtype != torch.float64:
            raise EvLibraryError(f"modulation: v must be float64 (B, K, F), got {v.dtype} {tuple(v.shape)}")
        v = v.contiguous()
        B, K, F = v.shape
        if mask is not None:
            if tuple(mask.shape) != (B, K, F) or mask.device != v.device or mask.dtype not in (torch.uint8, torch.bool):
                raise EvLibraryError(f"modulation: mask must be uint8 or bool ({B}, {K}, {F}) on {v.device}, got {mask.dtype} {tuple(mask.shape)} "
                                     f"on {mask.device}")
            mask = mask.contiguous()
        ln = None if lengths is None else torch.as_tensor(lengths).to(v.device, torch.int32).contiguous()
        if ln is not None and ln.numel() != B:
            raise ValueError(f"modulation: {B} lengths expected, got {ln.numel()}")
        ba = np.ascontiguousarray(np.asarray(bands, dtype=np.int32).reshape(-1, 2))
        NB, NMo = int(ba.shape[0]), max(min(int(NM), 128), 1)
        spec = torch.empty((B, K, NMo), dtype=torch.float64, device=v.device)
        weight = torch.empty((B, K, NMo), dtype=torch.int32, device=v.device)
        peak = torch.empty((B, K, max(min(NB, 4), 0), 4), dtype=torch.float64, device=v.device)
        stat = torch.empty((B, K, 2), dtype=torch.float64, device=v.device)
        count = torch.empty((B, K, 4 + max(min(NB, 4), 0)), dtype=torch.int32, device=v.device)
        self._check(self.lib.ev_modulation(self.h, v.data_ptr(), _ptr(mask), _ptr(ln), B, K, F, float(nu0), float(dnu), int(NM), int(min_run),
                                           float(min_cycles), ba.ctypes.data if NB else None, NB, spec.data_ptr(), weight.data_ptr(),
                                           peak.data_ptr() if NB else None, stat.data_ptr(), count.data_ptr(), _stream_ptr()), "ev_modulation")
        return spec, weight, peak, stat, count

    def pyin_observe(self, x, lengths, frame_length: int, hop_length: int, tau_min: int, tau_max: int, sr: float, fmin: float,
                     bins_per_octave: int, n_bins: int, w, boltzmann: float = 2.0, no_trough_prob: float = 0.01, out=None):
        """pYIN's observation per frame of every row of ``x`` (B, L) (ev_pyin_observe): (obs (B, F, n_bins) float64: the probability of each
        pitch bin, pv (B, F) float64: the probability that the frame is voiced) on the device, F = ceil(L / hop_length).  ``w``: the
        threshold prior of ``audio.pyin_threshold_prior``, float64, read on the host during the call.  ``out``: (obs, pv) tensors to write
        into instead of new ones."""
        x, B, L, ln = self._rows(x, lengths, "pyin_observe")
        w = np.ascontiguousarray(np.asarray(w, dtype=np.float64).reshape(-1))
        F = -(-L // max(int(hop_length), 1))
        nb = max(int(n_bins), 0)
        if out is None:
            obs = torch.empty((B, F, nb), dtype=torch.float64, device=x.device)
            pv = torch.empty((B, F), dtype=torch.float64, device=x.device)
        else:
            obs, pv = out
            if obs.dtype != torch.float64 or pv.dtype != torch.float64 or tuple(obs.shape) != (B, F, nb) or tuple(pv.shape) != (B, F) \
                    or not obs.is_contiguous() or not pv.is_contiguous():
                raise ValueError(f"pyin_observe: out must be contiguous float64 ({B}, {F}, {nb}) and ({B}, {F})")
        self._check(self.lib.ev_pyin_observe(self.h, x.data_ptr(), _ptr(ln), B, L, int(frame_length), int(hop_length), int(tau_min), int(tau_max),
                                             float(sr), float(fmin), int(bins_per_octave), int(n_bins), w.ctypes.data, int(w.size),
                                             float(boltzmann), float(no_trough_prob), obs.data_ptr(), pv.data_ptr(), _stream_ptr()),
                    "ev_pyin_observe")
        return obs, pv

    def pyin_decode(self, obs, pv, lengths, L: int, hop_length: int, R: int, log_tri, log_Z, log_stay: float, log_switch: float, back=None):
        """The Viterbi pass over (voiced / unvoiced) x pitch bins (ev_pyin_decode) of ``obs`` (B, F, n_bins) and ``pv`` (B, F), float64, F =
        ceil(L / hop_length): (state (B, F) int32: v n_bins + i per frame, v = 0 voiced, -1 past a row's ceil(len / hop_length) frames;
        loglik (B,) float64) on the device.  ``lengths`` (B,): SAMPLES per row (None: L).  The tables of ``audio.pyin_transition`` are read on
        the host during the call.  ``back``: (B, F, 2 n_bins) uint8 scratch to use instead of a new tensor."""
        if obs.dtype != torch.float64 or pv.dtype != torch.float64 or obs.dim() != 3 or pv.dim() != 2 or obs.shape[:2] != pv.shape:
            raise ValueError(f"pyin_decode: float64 obs (B, F, n_bins) and pv (B, F) expected, got {tuple(obs.shape)} and {tuple(pv.shape)}")
        if not obs.is_cuda:
            raise EvLibraryError("no CPU fallback: pyin_decode needs its inputs on the GPU")
        obs, pv = obs.contiguous(), pv.contiguous()
        B, F, nb = obs.shape
        if F != -(-int(L) // max(int(hop_length), 1)):
            raise ValueError(f"pyin_decode: obs has {F} frames, L={L} at hop_length={hop_length} has {-(-int(L) // max(int(hop_length), 1))}")
        ln = None if lengths is None else torch.as_tensor(lengths).to(obs.device, torch.int32).contiguous()
        if ln is not None and ln.numel() != B:
            raise ValueError(f"pyin_decode: {B} lengths expected, got {ln.numel()}")
        log_tri = np.ascontiguousarray(np.asarray(log_tri, dtype=np.float64).reshape(-1))
        log_Z = np.ascontiguousarray(np.asarray(log_Z, dtype=np.float64).reshape(-1))
        if log_tri.size != int(R) + 1 or log_Z.size != nb:
            raise ValueError(f"pyin_decode: log_tri must hold R + 1 = {int(R) + 1} values and log_Z n_bins = {nb} (got {log_tri.size} and {log_Z.size})")
        if back is None:
            back = torch.empty((B, F, 2 * nb), dtype=torch.uint8, device=obs.device)
        elif back.dtype != torch.uint8 or back.numel() < B * F * 2 * nb or not back.is_contiguous():
            raise ValueError(f"pyin_decode: back must be contiguous uint8 with at least {B * F * 2 * nb} elements")
        state = torch.empty((B, F), dtype=torch.int32, device=obs.device)
        loglik = torch.empty((B,), dtype=torch.float64, device=obs.device)
        self._check(self.lib.ev_pyin_decode(self.h, obs.data_ptr(), pv.data_ptr(), _ptr(ln), B, int(L), int(hop_length), nb, int(R),
                                            log_tri.ctypes.data, log_Z.ctypes.data, float(log_stay), float(log_switch), back.data_ptr(),
                                            state.data_ptr(), loglik.data_ptr(), _stream_ptr()), "ev_pyin_decode")
        return state, loglik

    def maximum_path(self, value, x_lengths, y_lengths, want_path: bool = True, want_dur: bool = True):
        """monotonic_align.maximum_path on (B, Tx, Ty) fp32 scores with per-row lengths (ev_maximum_path): (path (B, Tx, Ty) 0/1 or None,
        durations (B, Tx) int32 or None), bit-equal to the reference's loop.  ``value`` is not modified."""
        value = self._f32(value)
        B, Tx, Ty = value.shape
        xl = x_lengths.to(value.device, torch.int32).contiguous()
        yl = y_lengths.to(value.device, torch.int32).contiguous()
        path = torch.empty((B, Tx, Ty), dtype=torch.float32, device=value.device) if want_path else None
        dur = torch.empty((B, Tx), dtype=torch.int32, device=value.device) if want_dur else None
        self._check(self.lib.ev_maximum_path(self.h, value.data_ptr(), xl.data_ptr(), yl.data_ptr(), B, Tx, Ty,
                                             path.data_ptr() if want_path else None, dur.data_ptr() if want_dur else None, _stream_ptr()), "ev_maximum_path")
        return path, dur

    def log_prior(self, mu_x, y):
        """log N(y_j; mu_i, I) for every (token, frame) pair (matcha_tts.py:186-193, ev_log_prior): (B, Tx, Ty), unmasked."""
        mu_x, y = self._f32(mu_x), self._f32(y)
        B, F, Tx = mu_x.shape
        Ty = y.shape[2]
        assert y.shape[:2] == (B, F)
        logp = torch.empty((B, Tx, Ty), dtype=torch.float32, device=mu_x.device)
        self._check(self.lib.ev_log_prior(self.h, mu_x.data_ptr(), y.data_ptr(), B, Tx, Ty, logp.data_ptr(), _stream_ptr()), "ev_log_prior")
        return logp

    def mas_align(self, mu_x, y, x_lengths, y_lengths, want_attn: bool = True, want_dur: bool = True, want_mu_y: bool = True, want_logp: bool = False):
        """Scores + search + expansion in one call (ev_mas_align): {"attn" (B, Tx, Ty), "dur" (B, Tx) int32, "mu_y" (B, 80, Ty),
        "logp" (B, Tx, Ty)}, None for what was not asked for."""
        mu_x, y = self._f32(mu_x), self._f32(y)
        B, F, Tx = mu_x.shape
        Ty = y.shape[2]
        assert y.shape[:2] == (B, F)
        dev = mu_x.device
        xl = x_lengths.to(dev, torch.int32).contiguous()
        yl = y_lengths.to(dev, torch.int32).contiguous()
        attn = torch.empty((B, Tx, Ty), dtype=torch.float32, device=dev) if want_attn else None
        dur = torch.empty((B, Tx), dtype=torch.int32, device=dev) if want_dur else None
        mu_y = torch.empty((B, F, Ty), dtype=torch.float32, device=dev) if want_mu_y else None
        logp = torch.empty((B, Tx, Ty), dtype=torch.float32, device=dev) if want_logp else None
        self._check(self.lib.ev_mas_align(self.h, mu_x.data_ptr(), y.data_ptr(), xl.data_ptr(), yl.data_ptr(), B, Tx, Ty,
                                          _ptr(attn), _ptr(dur), _ptr(mu_y), _ptr(logp), _stream_ptr()), "ev_mas_align")
        return {"attn": attn, "dur": dur, "mu_y": mu_y, "logp": logp}

    def load_text_encoder(self, tensors: Dict[str, torch.Tensor]):
        self._load(self.lib.ev_load_text_encoder, tensors, "ev_load_text_encoder")

    def text_encoder(self, ids, lengths, spk):
        """(mu_x (B,80,Tx), logw (B,1,Tx)) of TextEncoder.forward (text_encoder.py:378-410), masked by the token lengths."""
        assert ids.is_cuda and ids.dim() == 2
        ids = ids.to(torch.int64).contiguous()
        B, Tx = ids.shape
        lengths = lengths.to(ids.device, torch.int32).contiguous()
        spk_p = None
        if spk is not None:
            spk = self._f32(spk)
            spk_p = spk.data_ptr()
        mu = torch.empty((B, 80, Tx), dtype=torch.float32, device=ids.device)
        logw = torch.empty((B, 1, Tx), dtype=torch.float32, device=ids.device)
        self._check(self.lib.ev_text_encoder(self.h, ids.data_ptr(), lengths.data_ptr(), spk_p, B, Tx, mu.data_ptr(), logw.data_ptr(), _stream_ptr()),
                    "ev_text_encoder")
        return mu, logw

    def text_encoder_status(self):
        """Raises IndexError if a token id outside [0, n_vocab) was seen since the last check (the reference's nn.Embedding
        raises at the lookup, text_encoder.py:395); waits for the current stream."""
        if self.lib.ev_text_encoder_status(self.h, _stream_ptr()) != 0:
            raise IndexError(self.lib.ev_last_error(self.h).decode())

    # ---- hot calls -----------------------------------------------------------
    @staticmethod
    def _f32(t: torch.Tensor) -> torch.Tensor:
        assert t.is_cuda, "tensor must live on the GPU"
        return t.contiguous().float()

    def _rows(self, x, lengths, who: str):
        """The opening of the per-row analysis calls: (x as contiguous fp32 (B, L), B, L, ``lengths`` as int32 (B,) beside x or None)."""
        x = self._f32(x)
        if x.dim() != 2:
            raise ValueError(f"{who}: x must be (B, L), got shape {tuple(x.shape)}")
        B, L = x.shape
        ln = None if lengths is None else torch.as_tensor(lengths).to(x.device, torch.int32).contiguous()
        if ln is not None and ln.numel() != B:
            raise ValueError(f"{who}: {B} lengths expected, got {ln.numel()}")
        return x, B, L, ln

    def cfm_decode(self, mu, lengths, spk, z, n_steps: int, out_scale: float = 1.0, out_shift: float = 0.0):
        mu, z = self._f32(mu), self._f32(z)
        B, F, Tp = mu.shape
        assert F == 80 and z.shape == mu.shape
        lengths = lengths.to(mu.device, torch.int32).contiguous()
        spk_p = None
        if spk is not None:
            spk = self._f32(spk)
            spk_p = spk.data_ptr()
        out = torch.empty_like(mu)
        self._check(self.lib.ev_cfm_decode(self.h, mu.data_ptr(), lengths.data_ptr(), spk_p, z.data_ptr(), B, Tp, int(n_steps),
                                           float(out_scale), float(out_shift), out.data_ptr(), _stream_ptr()), "ev_cfm_decode")
        return out

    def cfm_decode2(self, mu, lengths, spk, z, n_steps: int, mel_std: float, mel_mean: float):
        """(decoder_outputs, mel) of one decode: both reference outputs from the library, no framework kernel in between."""
        mu, z = self._f32(mu), self._f32(z)
        B, F, Tp = mu.shape
        assert F == 80 and z.shape == mu.shape
        lengths = lengths.to(mu.device, torch.int32).contiguous()
        spk_p = None
        if spk is not None:
            spk = self._f32(spk)
            spk_p = spk.data_ptr()
        dec, mel = torch.empty_like(mu), torch.empty_like(mu)
        self._check(self.lib.ev_cfm_decode2(self.h, mu.data_ptr(), lengths.data_ptr(), spk_p, z.data_ptr(), B, Tp, int(n_steps),
                                            dec.data_ptr(), float(mel_std), float(mel_mean), mel.data_ptr(), _stream_ptr()), "ev_cfm_decode2")
        return dec, mel

    def reserve(self, B: int, Tx_max: int = 0, Tp_max: int = 0, T_voc_max: int = 0) -> None:
        """Pre-size workspace, scratch and staging for batches of B utterances up to these lengths (ev_reserve)."""
        self._check(self.lib.ev_reserve(self.h, int(B), int(Tx_max), int(Tp_max), int(T_voc_max), _stream_ptr()), "ev_reserve")

    def alloc_count(self) -> int:
        return int(self.lib.ev_alloc_count(self.h))

    def sk_taken(self) -> int:
        """Contributor shares taken over by their owners (work stealing of the balanced launches) since the handle was created."""
        return int(self.lib.ev_dbg_sk_taken(self.h))

    def sk_stats(self):
        """(balanced launches so far, arrivals of an unfinished one, hand-off waits that ran out) — diagnostic."""
        out = (C.c_uint32 * 3)()
        self._check(self.lib.ev_dbg_sk_stats(self.h, out), "ev_dbg_sk_stats")
        return tuple(int(v) for v in out)

    def estimator(self, x, mu, lengths, spk, t: float):
        x, mu = self._f32(x), self._f32(mu)
        B, F, Tp = mu.shape
        lengths = lengths.to(mu.device, torch.int32).contiguous()
        spk_p = None
        if spk is not None:
            spk = self._f32(spk)
            spk_p = spk.data_ptr()
        out = torch.empty_like(mu)
        self._check(self.lib.ev_estimator(self.h, x.data_ptr(), mu.data_ptr(), lengths.data_ptr(), spk_p, float(t), B, Tp,
                                          out.data_ptr(), _stream_ptr()), "ev_estimator")
        return out

    @staticmethod
    def _host_times(t, B: int) -> np.ndarray:
        """(B,) float32 on the host: what the two per-row calls take their times as."""
        tv = np.ascontiguousarray(torch.as_tensor(t).detach().to("cpu", torch.float32).numpy().reshape(-1))
        if tv.shape[0] != B:
            raise ValueError(f"t must hold one time per utterance: {B} expected, got {tv.shape[0]}")
        return tv

    def estimator_rows(self, x, mu, lengths, spk, t):
        """``estimator`` with one time per utterance (ev_estimator_rows): ``t`` (B,), a tensor or a sequence.  Eager-only."""
        x, mu = self._f32(x), self._f32(mu)
        B, F, Tp = mu.shape
        assert F == 80 and x.shape == mu.shape
        lengths = lengths.to(mu.device, torch.int32).contiguous()
        tv = self._host_times(t, B)
        spk_p = None
        if spk is not None:
            spk = self._f32(spk)
            spk_p = spk.data_ptr()
        out = torch.empty_like(mu)
        self._check(self.lib.ev_estimator_rows(self.h, x.data_ptr(), mu.data_ptr(), lengths.data_ptr(), spk_p, tv.ctypes.data_as(C.c_void_p), B, Tp,
                                               out.data_ptr(), _stream_ptr()), "ev_estimator_rows")
        return out

    def cfm_loss(self, x1, mu_y, y_lengths, spk, z, t, sigma_min: float, want_v: bool = False):
        """compute_loss for given draws in one call (ev_cfm_loss): x1, mu_y, z (B, 80, Ty) with any Ty, t (B,).  Returns (sums, v): sums
        (B, 2) float64 = per row {sum (v - u)^2, sum 0.5 ((x1 - mu_y)^2 + log 2 pi)} over its y_lengths[b] x 80 valid cells, v the
        velocity (B, 80, Ty) or None.  Eager-only."""
        x1, mu_y, z = self._f32(x1), self._f32(mu_y), self._f32(z)
        B, F, Ty = x1.shape
        assert F == 80 and mu_y.shape == x1.shape and z.shape == x1.shape
        yl = y_lengths.to(x1.device, torch.int32).contiguous()
        tv = self._host_times(t, B)
        spk_p = None
        if spk is not None:
            spk = self._f32(spk)
            spk_p = spk.data_ptr()
        sums = torch.empty((B, 2), dtype=torch.float64, device=x1.device)
        v = torch.empty_like(x1) if want_v else None
        self._check(self.lib.ev_cfm_loss(self.h, x1.data_ptr(), mu_y.data_ptr(), yl.data_ptr(), spk_p, z.data_ptr(), tv.ctypes.data_as(C.c_void_p), B, Ty,
                                         float(sigma_min), sums.data_ptr(), v.data_ptr() if want_v else None, _stream_ptr()), "ev_cfm_loss")
        return sums, v

    def hifigan(self, mel):
        mel = self._f32(mel)
        B, F, T = mel.shape
        assert F == 80
        wav = torch.empty((B, 1, T * 256), dtype=torch.float32, device=mel.device)
        # the kernels address tensors with 32-bit byte offsets (< 4 GiB each): the widest vocoder tensor holds
        # (T + 2 P0) x voc_frame_bytes per utterance (V1: 256 * (T + 8) frames x 128 B, levels 2-4), so very large batches are processed in row chunks
        per_utt = (T + 2 * self.voc_pad0) * self.voc_frame_bytes
        bmax = max(1, int((2**32 - 2**20) // per_utt))
        for b0 in range(0, B, bmax):
            b1 = min(B, b0 + bmax)
            self._check(self.lib.ev_hifigan(self.h, mel[b0:b1].data_ptr(), b1 - b0, T, wav[b0:b1].data_ptr(), _stream_ptr()), "ev_hifigan")
        return wav

    def workspace_bytes(self, B: int, Tp: int, Tv: int) -> int:
        return int(self.lib.ev_workspace_bytes(self.h, B, Tp, Tv))

    # ---- profiling hooks (bench.py) -------------------------------------------
    def profile_enable(self, on: bool):
        self._check(self.lib.ev_profile_enable(self.h, int(on)), "ev_profile_enable")

    def op_split_pieces(self, x):
        """(3, n) fp32: the three bf16 pieces of every element of x, as the split builds' staging code cuts them."""
        x = self._f32(x).reshape(-1)
        out = torch.empty((3, x.numel()), dtype=torch.float32, device=x.device)
        self._check(self.lib.ev_op_split_pieces(self.h, x.data_ptr(), x.numel(), out.data_ptr(), _stream_ptr()), "ev_op_split_pieces")
        return out

    def set_arithmetic(self, bf16_products: int):
        """Datapath of the deep layers' products (ev_set_arithmetic).  16 (default): two block-scaled fp16 pieces per operand,
        three fp16 products per fp32 product (22-23 significand bits, fp32 accumulation); 6: three bf16 pieces, six exact products;
        0: every product on the exact fp32 MFMA (v_mfma_f32_32x32x2_f32); 3: opt-in fast bf16 setting, NOT fp32-grade; 9: A/B."""
        self._check(self.lib.ev_set_arithmetic(self.h, int(bf16_products)), "ev_set_arithmetic")

    def set_amax(self, on: bool) -> None:
        """True (default): the fp16 builds take their tile scales from the producers' amax slots; False: every tile pre-scans (ev_dbg_set_amax)."""
        self._check(self.lib.ev_dbg_set_amax(self.h, int(bool(on))), "ev_dbg_set_amax")

    def set_attn_h16(self, on: bool) -> None:
        """True (default): under arithmetic setting 16 the U-Net's self-attention runs on the fp16 pipe (attn_out_h16_kernel); False: on the fp32 MFMA."""
        self._check(self.lib.ev_dbg_set_attn_h16(self.h, int(bool(on))), "ev_dbg_set_attn_h16")

    def set_chain(self, on: bool) -> None:
        """True (default): ResBlock1 chains that qualify (narrow levels, k = 3) run as one launch (resblock_chain_h16_kernel); False: as three fused pairs."""
        self._check(self.lib.ev_dbg_set_chain(self.h, int(bool(on))), "ev_dbg_set_chain")

    def arithmetic(self) -> int:
        return int(self.lib.ev_get_arithmetic(self.h))

    def last_cfg(self) -> int:
        return int(self.lib.ev_dbg_last_cfg(self.h))

    def profile_read_split(self):
        """(ms, flops, launches) of the bf16-split builds among the launches recorded since the last reset."""
        ms, fl, n = C.c_double(), C.c_double(), C.c_int64()
        self._check(self.lib.ev_profile_read_split(self.h, C.byref(ms), C.byref(fl), C.byref(n)), "ev_profile_read_split")
        return ms.value, fl.value, n.value

    def profile_read(self, reset: bool = True):
        ms, fl, n = C.c_double(), C.c_double(), C.c_int64()
        self._check(self.lib.ev_profile_read(self.h, C.byref(ms), C.byref(fl), C.byref(n), int(reset)), "ev_profile_read")
        return ms.value, fl.value, n.value

    # ---- operator-level entry points (unit tests) ---------------------------------
    def op_conv1d(self, x, w, bias, dilation=1, transposed=False, stride=1, padding=0, pre_lrelu_slope=-1.0):
        x = self._f32(x)
        B, Cin, T = x.shape
        w = np.ascontiguousarray(w.detach().cpu().float().numpy())
        if transposed:
            Cout, K = w.shape[1], w.shape[2]
            Tout = T * stride
        else:
            Cout, K = w.shape[0], w.shape[2]
            Tout = T // stride
        bp = None
        if bias is not None:
            bnp = np.ascontiguousarray(bias.detach().cpu().float().numpy())
            bp = bnp.ctypes.data_as(C.c_void_p)
        y = torch.empty((B, Cout, Tout), dtype=torch.float32, device=x.device)
        self._check(self.lib.ev_op_conv1d(self.h, x.data_ptr(), w.ctypes.data_as(C.c_void_p), bp, B, Cin, T, Cout, K, dilation,
                                          int(transposed), stride, padding, float(pre_lrelu_slope), y.data_ptr(), _stream_ptr()),
                    "ev_op_conv1d")
        return y

    def op_conv1d_epi(self, x, w, bias, dilation=1, transposed=False, stride=1, padding=0, P=32, pre_lrelu_slope=-1.0, act="none",
                      act_slope=0.0, alpha_exp=None, beta_inv=None, lengths=None, mask1=False, mask2=False, scale=1.0, R=None, yold=None,
                      accum=False, div3=False, act2_slope=-1.0, want_y2=False, want_padded=False):
        """One conv launch with the whole fused epilogue (ev_op_conv1d_epi; +bias, act, *mask1, *scale, +R, +Yold, /3, lrelu2, *mask2).
        x (B, Cin, T); R, yold (B, Cout, Tout); lengths (B,) in output frames; P pad rows a side.  Returns (y, y2 or None, padded Y or None):
        the padded Y is frame-major (B * (Tout + 2 Pout), Cout), its pad rows CONV_EPI_SENTINEL unless the launch stored there."""
        x = self._f32(x)
        B, Cin, T = x.shape
        w = np.ascontiguousarray(w.detach().cpu().float().numpy())
        if transposed:
            Cout, K, Tout, Pout = w.shape[1], w.shape[2], T * stride, P * stride
        else:
            Cout, K, Tout, Pout = w.shape[0], w.shape[2], T // stride, P // stride
        bp = None
        if bias is not None:
            bnp = np.ascontiguousarray(bias.detach().cpu().float().numpy())
            bp = bnp.ctypes.data_as(C.c_void_p)
        keep = [None if t is None else self._f32(t) for t in (alpha_exp, beta_inv, R, yold)]
        if lengths is not None:
            lengths = lengths.to(x.device, torch.int32).contiguous()
        for t in keep[2:]:
            if t is not None and tuple(t.shape) != (B, Cout, Tout):
                raise ValueError(f"R / yold must be {(B, Cout, Tout)}, got {tuple(t.shape)}")
        for t in keep[:2]:
            if t is not None and t.numel() != Cout:
                raise ValueError("alpha_exp / beta_inv must hold Cout values")
        ep = ev_conv_epi(CONV_ACTS[act], float(act_slope), _ptr(keep[0]), _ptr(keep[1]), _ptr(lengths), int(mask1), int(mask2), float(scale),
                         _ptr(keep[2]), int(accum), _ptr(keep[3]), int(div3), float(act2_slope), float(pre_lrelu_slope))
        y = torch.empty((B, Cout, Tout), dtype=torch.float32, device=x.device)
        y2 = torch.empty_like(y) if want_y2 else None
        ypad = torch.empty((B * (Tout + 2 * Pout), Cout), dtype=torch.float32, device=x.device) if want_padded else None
        self._check(self.lib.ev_op_conv1d_epi(self.h, x.data_ptr(), w.ctypes.data_as(C.c_void_p), bp, B, Cin, T, Cout, K, dilation, int(transposed),
                                              stride, padding, int(P), C.byref(ep), y.data_ptr(), _ptr(y2), _ptr(ypad), _stream_ptr()),
                    "ev_op_conv1d_epi")
        return y, y2, ypad

    def op_groupnorm_mish(self, x, gamma, beta, lengths, groups=8):
        x, gamma, beta = self._f32(x), self._f32(gamma), self._f32(beta)
        B, Cc, T = x.shape
        lengths = lengths.to(x.device, torch.int32).contiguous()
        y = torch.empty_like(x)
        self._check(self.lib.ev_op_groupnorm_mish(self.h, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), lengths.data_ptr(), B, Cc, T,
                                                  groups, y.data_ptr(), _stream_ptr()), "ev_op_groupnorm_mish")
        return y

    def op_groupnorm_mish2(self, x, gamma, beta, lengths, mode=0, temb=None, R=None, groups=8):
        """groupnorm_mish_kernel through launch_gn in the estimator's layout (X | R in one 512-wide buffer).  mode 1: temb (256,) or
        (1, 256) shared, (B, 256) one row per utterance; mode 2: R (B, 256, T)."""
        x, gamma, beta = self._f32(x), self._f32(gamma), self._f32(beta)
        B, Cc, T = x.shape
        lengths = lengths.to(x.device, torch.int32).contiguous()
        tp, stride, rp = None, 0, None
        if mode == 1:
            temb = self._f32(temb).reshape(-1, Cc)
            if temb.shape[0] not in (1, B):
                raise ValueError("temb: (1, C) or (B, C)")
            stride = Cc if (temb.shape[0] == B and B > 1) else 0
            tp = temb.data_ptr()
        if mode == 2:
            R = self._f32(R)
            if R.shape != x.shape:
                raise ValueError("R: the shape of x")
            rp = R.data_ptr()
        y = torch.empty_like(x)
        self._check(self.lib.ev_op_groupnorm_mish2(self.h, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), lengths.data_ptr(), B, Cc, T,
                                                   groups, int(mode), tp, stride, rp, y.data_ptr(), _stream_ptr()), "ev_op_groupnorm_mish2")
        return y

    def op_conv_groupnorm(self, x, w, bias, gamma, beta, length=None, mode=0, temb=None, R=None):
        """One utterance x (1, Cin, T) through conv (w (256, Cin, K), 'same' padding) and GroupNorm + Mish as the estimator chains them.
        Returns (conv output (1, 256, T), part (256, 8, 4): per (32-row tile, group) {count, mean, M2, -}, GroupNorm output (1, 256, T),
        tiles): tiles = row tiles whose statistics the conv left for the norm, 0 when it left none."""
        x, gamma, beta = self._f32(x), self._f32(gamma), self._f32(beta)
        _, Cin, T = x.shape
        wh = np.ascontiguousarray(w.detach().cpu().float().numpy())
        K = wh.shape[2]
        bh = None if bias is None else np.ascontiguousarray(bias.detach().cpu().float().numpy())
        lengths = torch.tensor([T if length is None else int(length)], dtype=torch.int32, device=x.device)
        tp = rp = None
        if mode == 1:
            temb = self._f32(temb).reshape(-1)
            tp = temb.data_ptr()
        if mode == 2:
            R = self._f32(R)
            rp = R.data_ptr()
        conv = torch.empty((1, 256, T), dtype=torch.float32, device=x.device)
        y = torch.empty_like(conv)
        part = torch.empty((256, 8, 4), dtype=torch.float32, device=x.device)
        tiles = C.c_int(0)
        self._check(self.lib.ev_op_conv_groupnorm(self.h, x.data_ptr(), wh.ctypes.data_as(C.c_void_p),
                                                  None if bh is None else bh.ctypes.data_as(C.c_void_p), Cin, T, K, gamma.data_ptr(),
                                                  beta.data_ptr(), lengths.data_ptr(), int(mode), tp, rp, conv.data_ptr(), part.data_ptr(),
                                                  y.data_ptr(), C.byref(tiles), _stream_ptr()), "ev_op_conv_groupnorm")
        return conv, part, y, int(tiles.value)

    def op_layernorm(self, x, gamma, beta):
        x, gamma, beta = self._f32(x), self._f32(gamma), self._f32(beta)
        rows, Cc = x.shape
        y = torch.empty_like(x)
        self._check(self.lib.ev_op_layernorm(self.h, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rows, Cc, y.data_ptr(),
                                             _stream_ptr()), "ev_op_layernorm")
        return y

    def op_ln_mlp(self, x, ln_g, ln_b, w1, b1, alpha=None, beta=None, w2=None, b2=None, rowmask=None):
        """ln_mlp_kernel on (rows, 256): with w2 -> x + W2.SnakeBeta(W1.LN(x)+b1)+b2 (* rowmask); without -> W1.LN(x) (+ b1)."""
        x, ln_g, ln_b = self._f32(x), self._f32(ln_g), self._f32(ln_b)
        rows = x.shape[0]
        M1 = w1.shape[0]
        host = lambda t: None if t is None else np.ascontiguousarray(t.detach().cpu().float().numpy())   # noqa: E731
        w1h, b1h, w2h, b2h = host(w1), host(b1), host(w2), host(b2)
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
        mode = 0 if w2 is not None else 1
        a_exp = self._f32(torch.exp(alpha.float()).to(x.device)) if alpha is not None else None
        b_inv = self._f32((1.0 / (torch.exp(beta.float()) + 0.000000001)).to(x.device)) if beta is not None else None
        rm = self._f32(rowmask) if rowmask is not None else None
        y = torch.empty((rows, 256 if mode == 0 else M1), dtype=torch.float32, device=x.device)
        self._check(self.lib.ev_op_ln_mlp(self.h, x.data_ptr(), ln_g.data_ptr(), ln_b.data_ptr(), ptr(w1h), ptr(b1h), _ptr(a_exp), _ptr(b_inv),
                                          ptr(w2h), ptr(b2h), _ptr(rm), rows, M1, mode, y.data_ptr(), _stream_ptr()), "ev_op_ln_mlp")
        return y

    def op_attention(self, qkv, lengths, heads=2):
        qkv = self._f32(qkv)
        B, T, _ = qkv.shape
        lengths = lengths.to(qkv.device, torch.int32).contiguous()
        out = torch.empty((B, T, heads * 64), dtype=torch.float32, device=qkv.device)
        self._check(self.lib.ev_op_attention(self.h, qkv.data_ptr(), lengths.data_ptr(), B, T, heads, out.data_ptr(), _stream_ptr()),
                    "ev_op_attention")
        return out

    def op_attn_out(self, qkv, lengths, w_out, b_out, hid):
        """attn_out_kernel: hid + Wout . attention(qkv) + bout; qkv (B, T, 384), hid (B, T, 256), lengths (B,)."""
        qkv, hid = self._f32(qkv), self._f32(hid).clone()
        B, T, _ = qkv.shape
        lengths = lengths.to(qkv.device, torch.int32).contiguous()
        wh = np.ascontiguousarray(w_out.detach().cpu().float().numpy())
        bh = np.ascontiguousarray(b_out.detach().cpu().float().numpy())
        self._check(self.lib.ev_op_attn_out(self.h, qkv.data_ptr(), lengths.data_ptr(), B, T, wh.ctypes.data_as(C.c_void_p), bh.ctypes.data_as(C.c_void_p),
                                            hid.data_ptr(), _stream_ptr()), "ev_op_attn_out")
        return hid

    def op_attention2(self, qkv, lengths, S, P, T, heads=2, scratch=True, out=None):
        """launch_attn in a padded geometry: qkv (B*S, 3*heads*64), frame t of utterance b in row b*S + P + t.  scratch: hand it the split-key
        scratch (the engine's rule then picks the build).  out (B*S, heads*64) is written in place where given (its pad rows stay).
        Returns (out, {"split": bool, "KS": int})."""
        qkv = self._f32(qkv)
        B = qkv.shape[0] // S
        if qkv.shape != (B * S, 3 * heads * 64):
            raise ValueError("qkv: (B*S, 3*heads*64)")
        lengths = lengths.to(qkv.device, torch.int32).contiguous()
        if out is None:
            out = torch.zeros((B * S, heads * 64), dtype=torch.float32, device=qkv.device)
        if out.shape != (B * S, heads * 64) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("out: contiguous fp32 (B*S, heads*64)")
        ran = (C.c_int * 2)()
        self._check(self.lib.ev_op_attention2(self.h, qkv.data_ptr(), lengths.data_ptr(), B, S, P, T, heads, 0 if scratch else 1, out.data_ptr(),
                                              ran, _stream_ptr()), "ev_op_attention2")
        return out, {"split": bool(ran[0]), "KS": int(ran[1])}

    def op_attn_out2(self, qkv, lengths, w_out, b_out, hid, S, P, T, scales=None):
        """launch_attn_out in a padded geometry, IN PLACE on hid (B*S, 256); qkv (B*S, 384).  scales: (sq, sk, sv) powers of two for the fp16
        form, None = from the data's maxima.  Returns (hid, {"h16": bool, "ntail": int, "nq": int})."""
        qkv = self._f32(qkv)
        B = qkv.shape[0] // S
        if qkv.shape != (B * S, 384) or hid.shape != (B * S, 256) or hid.dtype != torch.float32 or not hid.is_contiguous():
            raise ValueError("qkv: (B*S, 384); hid: contiguous fp32 (B*S, 256)")
        lengths = lengths.to(qkv.device, torch.int32).contiguous()
        wh = np.ascontiguousarray(w_out.detach().cpu().float().numpy())
        bh = np.ascontiguousarray(b_out.detach().cpu().float().numpy())
        sq, sk, sv = (0.0, 0.0, 0.0) if scales is None else (float(x) for x in scales)
        ran = (C.c_int * 3)()
        self._check(self.lib.ev_op_attn_out2(self.h, qkv.data_ptr(), lengths.data_ptr(), B, S, P, T, wh.ctypes.data_as(C.c_void_p),
                                             bh.ctypes.data_as(C.c_void_p), sq, sk, sv, hid.data_ptr(), ran, _stream_ptr()), "ev_op_attn_out2")
        return hid, {"h16": bool(ran[0]), "ntail": int(ran[1]), "nq": int(ran[2])}
