"""Drop-in for ``matcha.models.matcha_tts.MatchaTTS`` on the inference path.

Keeps the reference call surface (matcha_tts.py:78, return keys :145-152):

    MatchaTTS.synthesise(x, x_lengths, n_timesteps, temperature=1.0, spks=None, length_scale=1.0) -> dict

``.n_spks``, ``.eval()``, ``.to(device)`` and ``MatchaTTS.load_from_checkpoint(path,
map_location=)`` behave as the callers in cli.py / feel_me.py expect.  The text
encoder + duration predictor (``ev_text_encoder``), the monotonic alignment
(``ev_align``) and the CFM Euler loop over the U-Net estimator (``ev_cfm_decode2``)
run in the HIP library through the C ABI; only the duration rounding and the
integer ``y_lengths`` stay torch ops (data-dependent sizes, matcha_tts.py:121-128).
``encoder_stage = "host"`` selects the plain-torch text encoder + alignment instead
(north_star's "run once on host").

``forward`` (matcha_tts.py:154-246) is the no-grad pass over (text, mel) pairs that the reference's validation step and
``utils/get_durations_from_trained_model.py`` make: log-likelihood scores, monotonic alignment search and ``mu_y`` in one
library call (``ev_mas_align``), the three losses from there.  ``align`` is the durations script without the losses.
Training with gradients is out of scope.
"""
from __future__ import annotations

import datetime as dt
import math
import pickle
from collections import OrderedDict
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from . import weights as W
from ._lib import Engine, EvLibraryError
from .text_encoder import TextEncoder, duration_loss, fix_len_compatibility, generate_path, sequence_mask

EST_PREFIX = "decoder.estimator."


def estimator_tensors(sd: Dict[str, torch.Tensor]) -> "OrderedDict[str, torch.Tensor]":
    """Estimator entries of a Matcha state dict with the prefix stripped, plus the two
    derived SnakeBeta vectors the kernels consume (transformer.py:71-78, evaluated with the
    same torch ops as the reference): ``alpha_exp = exp(alpha)``, ``beta_inv = 1/(exp(beta)+1e-9)``."""
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for k, v in sd.items():
        if not k.startswith(EST_PREFIX):
            continue
        name = k[len(EST_PREFIX):]
        v = v.detach().to("cpu", torch.float32)
        out[name] = v
        if name.endswith(".ff.net.0.alpha"):
            out[name + "_exp"] = torch.exp(v)
        elif name.endswith(".ff.net.0.beta"):
            out[name + "_inv"] = 1.0 / (torch.exp(v) + 0.000000001)
    return out


def text_encoder_tensors(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Tensors handed to ``ev_load_text_encoder``: ``encoder.*`` without the prefix, plus the rotary frequency table built
    with the reference's own expression (text_encoder.py:115-117; d = int(k_channels * 0.5), :196-199)."""
    out: Dict[str, torch.Tensor] = {}
    for k, v in sd.items():
        if k.startswith("encoder."):
            out[k[len("encoder."):]] = v.detach().float()
    n_heads = 2
    kc = out["encoder.attn_layers.0.conv_q.weight"].shape[0] // n_heads
    d = int(kc * 0.5)
    out["rope_theta"] = 1.0 / (10000.0 ** (torch.arange(0, d, 2).float() / d))
    return out


def row_losses(sums, logw, logw_, x_lengths, y_lengths, n_feats: int = 80) -> Dict[str, torch.Tensor]:
    """Per-utterance losses from the (B, 2) float64 row sums of ``ev_cfm_loss`` {sum (v - u)^2, sum prior}: each row's sum over its
    y_lengths[b] * n_feats cells divided by that count; dur_loss of a row = sum (logw - logw_)^2 / x_lengths[b].  Float64 (B,) each; the
    callers round once to the reference's float32."""
    B = sums.shape[0]
    cells = y_lengths.reshape(B).double() * n_feats
    dur = torch.sum((logw.double() - logw_.double()).reshape(B, -1) ** 2, dim=1) / x_lengths.reshape(B).double()
    return {"dur_loss": dur, "prior_loss": sums[:, 1].double() / cells, "diff_loss": sums[:, 0].double() / cells}


def batch_losses(sums, padded_sum, logw, logw_, x_lengths, y_lengths, n_feats: int = 80):
    """(dur_loss, prior_loss, diff_loss) of the batch as the reference defines them (matcha_tts.py:203-204, :241-242,
    flow_matching.py:115-117), float64 scalars: sum_b sums / (sum_b y_lengths * n_feats).  ``padded_sum``: the
    diff_loss share of the padded frames (``padded_frames_sum``), which the reference's mse_loss counts and the row sums do not."""
    n_valid = torch.sum(y_lengths).double() * n_feats
    dur_loss = duration_loss(logw.double(), logw_.double(), x_lengths)
    return dur_loss, torch.sum(sums[:, 1].double()) / n_valid, (torch.sum(sums[:, 0].double()) + padded_sum) / n_valid


def padded_frames_sum(y, z, y_lengths, sigma_min: float) -> torch.Tensor:
    """sum u^2 over the frames at or past each row's length, float64 scalar, u = y - (1 - sigma_min) z in float32: the reference's
    F.mse_loss(estimator(...), u, reduction="sum") runs over the padded frames of the shorter rows too, where the estimator is exactly 0
    and u is not (flow_matching.py:115-117).  It needs no estimator; a batch of full-length rows has none."""
    Ty = y.shape[2]
    tail = Ty - int(y_lengths.min())
    if tail <= 0:
        return torch.zeros((), dtype=torch.float64, device=y.device)
    y, z = y[:, :, Ty - tail:], z[:, :, Ty - tail:]                          # only the columns some row pads
    pad = ~sequence_mask(y_lengths, Ty)[:, Ty - tail:].unsqueeze(1)
    return torch.sum(((y - (1 - sigma_min) * z) * pad).double() ** 2)


class MatchaTTS:
    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda:0", n_heads_encoder: int = 2, n_layers_encoder: int = 6):
        sd = {k: v.detach().float() for k, v in state_dict.items()}
        self.n_spks = int(sd["spk_emb.weight"].shape[0]) if "spk_emb.weight" in sd else 1
        self.spk_emb_dim = int(sd["spk_emb.weight"].shape[1]) if self.n_spks > 1 else 0
        self.n_vocab = int(sd["encoder.emb.weight"].shape[0])
        self.n_feats = int(sd["encoder.proj_m.weight"].shape[0])
        self.mel_mean = float(sd.get("mel_mean", torch.tensor(0.0)))
        self.mel_std = float(sd.get("mel_std", torch.tensor(1.0)))
        self.sigma_min = 1e-4           # cfm_params.sigma_min (configs/model/cfm/default.yaml): not part of a state dict
        self._cpu_sd = sd
        self._enc_cfg = (n_heads_encoder, n_layers_encoder)
        self.encoder_stage = "device"   # "device": ev_text_encoder (HIP, through the C ABI); "host": the plain-torch TextEncoder
        self.rng = "cpu"   # "cpu": z drawn exactly as the reference CPU run draws it (seed parity); "device": torch.cuda RNG
        self.decode_graphs = None   # enable_decode_graphs(): the CFM decode replayed from HIP graphs (one per shape)
        self.engine: Optional[Engine] = None
        self.device = torch.device("cpu")
        self.to(device)

    # ---- nn.Module-like surface ------------------------------------------------
    def eval(self):
        return self

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise EvLibraryError("emojivoice_amd.MatchaTTS runs on a ROCm GPU only (no CPU fallback); got device " + str(device))
        idx = device.index if device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        self._sd = {k: v.to(self.device) for k, v in self._cpu_sd.items() if not k.startswith(EST_PREFIX)}
        self.encoder = TextEncoder(self._sd, *self._enc_cfg)
        if self.engine is not None:
            self.engine.close()
        self.engine = Engine(idx, spk_emb_dim=self.spk_emb_dim)
        self.engine.load_estimator(estimator_tensors(self._cpu_sd))
        self.engine.load_text_encoder(text_encoder_tensors(self._cpu_sd))
        return self

    def encode(self, x, x_lengths, spk):
        """TextEncoder.forward (text_encoder.py:378-410): (mu_x, logw, x_mask).  ``encoder_stage = "host"`` runs the plain
        torch restatement instead (north_star's "text encoder run once on host")."""
        if self.encoder_stage == "host":
            return self.encoder(x, x_lengths, spk)
        mu_x, logw = self.engine.text_encoder(x, x_lengths, spk)
        x_mask = sequence_mask(x_lengths, x.shape[1]).unsqueeze(1).to(mu_x.dtype)
        return mu_x, logw, x_mask

    def state_dict(self):
        return dict(self._cpu_sd)

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, map_location=None):
        """cli.py:110-118.  A Lightning ``.ckpt`` is a pickle with ``state_dict`` and ``hyper_parameters``;
        only tensors are needed here, so unknown classes in ``hyper_parameters`` (omegaconf, functools.partial
        of an optimizer) are stubbed by a restricted unpickler instead of being imported."""
        ckpt = _load_ckpt(checkpoint_path)
        sd = ckpt["state_dict"] if "state_dict" in ckpt else ckpt
        return cls(sd, device=map_location if map_location is not None else "cuda:0")

    # ---- the no-grad pass over (text, mel) pairs -----------------------------------
    def _encode_pairs(self, x, x_lengths, y, y_lengths, spks):
        """Speaker embedding and text encoder for (text, mel) pairs, after the length check both public methods share: the
        reference's search reads outside its rows for x_lengths > y_lengths or an empty row (one device read here)."""
        dev = self.device
        x, x_lengths, y_lengths = x.to(dev), x_lengths.to(dev).long(), y_lengths.to(dev).long()
        y = y.to(dev, torch.float32).contiguous()
        if y.dim() != 3 or y.shape[0] != x.shape[0] or y.shape[1] != self.n_feats:
            raise ValueError(f"y must be (B, {self.n_feats}, Ty), got {tuple(y.shape)} for {x.shape[0]} texts")
        xl, yl = torch.stack([x_lengths, y_lengths]).cpu()
        if bool((xl < 1).any()) or bool((yl < 1).any()) or bool((xl > yl).any()) or int(xl.max()) > x.shape[1] or int(yl.max()) > y.shape[2]:
            raise ValueError(f"every row needs 1 <= x_lengths <= y_lengths within the padded shapes (monotonic alignment search is undefined "
                             f"otherwise): x_lengths {xl.tolist()}, y_lengths {yl.tolist()}, x {tuple(x.shape)}, y {tuple(y.shape)}")
        spk = F.embedding(spks.to(dev).long(), self._sd["spk_emb.weight"]) if self.n_spks > 1 else None
        mu_x, logw, x_mask = self.encode(x, x_lengths, spk)
        if self.encoder_stage != "host":
            self.engine.text_encoder_status()
        return x_lengths, y, y_lengths, spk, mu_x, logw, x_mask

    @torch.inference_mode()
    def align(self, x, x_lengths, y, y_lengths, spks=None):
        """What utils/get_durations_from_trained_model.py takes from ``forward``: the monotonic alignment of each text to its
        (normalised) mel.  Returns {"attn" (B, Tx, Ty), "durations" (B, Tx) int64 = attn.sum(-1), "logw_" (B, 1, Tx), "mu_y" (B, 80, Ty)}."""
        x_lengths, y, y_lengths, _, mu_x, _, x_mask = self._encode_pairs(x, x_lengths, y, y_lengths, spks)
        r = self.engine.mas_align(mu_x, y, x_lengths, y_lengths)
        logw_ = torch.log(1e-8 + r["dur"].to(mu_x.dtype)).unsqueeze(1) * x_mask
        return {"attn": r["attn"], "durations": r["dur"].long(), "logw_": logw_, "mu_y": r["mu_y"]}

    def _align_pairs(self, durations, mu_x, logw, x_mask, y, x_lengths, y_lengths):
        """(mu_y, attn (B, Tx, Ty), logw_) of forward: from given durations through generate_path, else the search."""
        if durations is not None:
            mu_y, attn = self.engine.align(durations.to(self.device).float(), mu_x, x_lengths, y_lengths, y.shape[2])
            attn = attn.squeeze(1)
            tok = attn.sum(-1)
        else:
            r = self.engine.mas_align(mu_x, y, x_lengths, y_lengths)
            mu_y, attn, tok = r["mu_y"], r["attn"], r["dur"].to(mu_x.dtype)
        return mu_y, attn, torch.log(1e-8 + tok).unsqueeze(1) * x_mask

    def _draws(self, y, t, z):
        """t (B,) and z (B, 80, Ty) of compute_loss (flow_matching.py:105-110): drawn here unless given."""
        B = y.shape[0]
        t = torch.rand([B], device=self.device, dtype=y.dtype) if t is None else t.to(self.device, y.dtype).reshape(B)
        z = torch.randn_like(y) if z is None else z.to(self.device, y.dtype)
        return t, z

    @torch.inference_mode()
    def forward(self, x, x_lengths, y, y_lengths, spks=None, out_size=None, cond=None, durations=None, *, t=None, z=None, batched=False):
        """Reference matcha_tts.py:154-246 without gradients: (dur_loss, prior_loss, diff_loss, attn (B, Tx, Ty)).
        ``durations`` (B, 1, Tx) or (B, Tx), as under the reference's ``use_precomputed_durations``, replace the search by
        generate_path.  Extension: keyword-only ``t`` (B,) and ``z`` (B, 80, Ty) replace the draws of compute_loss
        (flow_matching.py:105-110) for reproducible runs.  ``batched=False``: the estimator runs one row at a time (``ev_estimator``
        takes one scalar t per call) between torch ops.  ``batched=True``: ``diff_loss`` and ``prior_loss`` come from ONE
        ``ev_cfm_loss`` call over the batch (one time per utterance inside the U-Net, y_t and u never stored); same 4-tuple."""
        if out_size is not None:
            raise NotImplementedError("out_size (the random segment cut of matcha_tts.py:206-231, a training memory hack) is not supported: pass out_size=None")
        x_lengths, y, y_lengths, spk, mu_x, logw, x_mask = self._encode_pairs(x, x_lengths, y, y_lengths, spks)
        if batched:
            return self._forward_batched(x_lengths, y, y_lengths, spk, mu_x, logw, x_mask, durations, t, z)
        B, _, Ty = y.shape
        y_mask = sequence_mask(y_lengths, Ty).unsqueeze(1).to(x_mask.dtype)
        mu_y, attn, logw_ = self._align_pairs(durations, mu_x, logw, x_mask, y, x_lengths, y_lengths)
        # the three reductions accumulate in float64 and round once to the reference's float32 (a few thousand elements each)
        dur_loss = duration_loss(logw.double(), logw_.double(), x_lengths).float()
        n_valid = torch.sum(y_lengths).double() * self.n_feats
        prior_loss = (torch.sum(0.5 * ((y - mu_y).double() ** 2 + math.log(2 * math.pi)) * y_mask) / n_valid).float()
        # compute_loss (flow_matching.py:87-118)
        t, z = self._draws(y, t, z)
        tb = t.view(B, 1, 1)
        y_t = (1 - (1 - self.sigma_min) * tb) * z + tb * y
        u = y - (1 - self.sigma_min) * z
        pad = fix_len_compatibility(Ty) - Ty          # the U-Net needs a multiple of 4: masked frames, cut off again below
        y_t_p, mu_y_p = F.pad(y_t, (0, pad)).contiguous(), F.pad(mu_y, (0, pad)).contiguous()
        v = torch.empty_like(y_t_p)
        for b, tv in enumerate(t.cpu().tolist()):
            v[b:b + 1] = self.engine.estimator(y_t_p[b:b + 1], mu_y_p[b:b + 1], y_lengths[b:b + 1], None if spk is None else spk[b:b + 1], tv)
        diff_loss = (torch.sum((v[:, :, :Ty] - u).double() ** 2) / n_valid).float()
        return dur_loss, prior_loss, diff_loss, attn

    def _forward_batched(self, x_lengths, y, y_lengths, spk, mu_x, logw, x_mask, durations, t, z):
        """forward(batched=True) after the encoder: the alignment, then one ev_cfm_loss call for both mel-side sums."""
        mu_y, attn, logw_ = self._align_pairs(durations, mu_x, logw, x_mask, y, x_lengths, y_lengths)
        t, z = self._draws(y, t, z)
        sums, _ = self.engine.cfm_loss(y, mu_y, y_lengths, spk, z, t, self.sigma_min)
        dur_loss, prior_loss, diff_loss = batch_losses(sums, padded_frames_sum(y, z, y_lengths, self.sigma_min), logw, logw_, x_lengths, y_lengths, self.n_feats)
        return dur_loss.float(), prior_loss.float(), diff_loss.float(), attn

    @torch.inference_mode()
    def score(self, x, x_lengths, y, y_lengths, spks=None, durations=None, *, t=None, z=None):
        """The three losses PER UTTERANCE (the number that finds a badly aligned recording), always through ``ev_cfm_loss``:
        {"dur_loss", "prior_loss", "diff_loss"} each (B,) float32, "attn" (B, Tx, Ty), "durations" (B, Tx) int64.  A row's ``diff_loss``
        and ``prior_loss`` are its sums over its own y_lengths[b] x 80 cells divided by that count (no padded frame of a longer batch
        enters), its ``dur_loss`` is sum (logw - logw_)^2 / x_lengths[b].  ``t`` and ``z`` as for ``forward``."""
        x_lengths, y, y_lengths, spk, mu_x, logw, x_mask = self._encode_pairs(x, x_lengths, y, y_lengths, spks)
        mu_y, attn, logw_ = self._align_pairs(durations, mu_x, logw, x_mask, y, x_lengths, y_lengths)
        t, z = self._draws(y, t, z)
        sums, _ = self.engine.cfm_loss(y, mu_y, y_lengths, spk, z, t, self.sigma_min)
        out = {k: v.float() for k, v in row_losses(sums, logw, logw_, x_lengths, y_lengths, self.n_feats).items()}
        out["attn"], out["durations"] = attn, attn.sum(-1).long()
        return out

    __call__ = forward

    # ---- the hot call ------------------------------------------------------------
    def _durations(self, x, x_lengths, spks, length_scale):
        """matcha_tts.py:116-125: speaker embedding, text encoder, duration rounding.  Returns
        (spk, mu_x, w_ceil, x_mask, x_lengths, y_lengths) on the device and max(y_lengths) as a host int."""
        dev = self.device
        x, x_lengths = x.to(dev), x_lengths.to(dev)
        if self.n_spks > 1:
            spk = F.embedding(spks.to(dev).long(), self._sd["spk_emb.weight"])   # AttributeError on None, like the reference
        else:
            spk = None
        mu_x, logw, x_mask = self.encode(x, x_lengths, spk)
        w = torch.exp(logw) * x_mask
        w_ceil = torch.ceil(w) * length_scale
        # y_lengths is an INTEGER output (truncation of a float sum): with a fractional length_scale the sum sits on or next to
        # an integer (55 x 0.8 = 44) and the summation order decides the truncation.  The reduction is therefore done by the same
        # torch CPU op the reference CPU run uses, on the (B, Tx) durations copied to the host — the copy replaces the
        # device -> host read of max(y_lengths) that the path needs anyway (matcha_tts.py:125), so it adds no synchronisation.
        y_lengths_host = torch.clamp_min(torch.sum(w_ceil.cpu(), [1, 2]), 1).long()
        return spk, mu_x, w_ceil, x_mask, x_lengths, y_lengths_host.to(dev), int(y_lengths_host.max())

    def _decode_aligned(self, spk, mu_x, w_ceil, x_mask, x_lengths, y_lengths, y_max_length, n_timesteps, temperature, z=None):
        """matcha_tts.py:125-152 for a given (possibly global, see dist.synthesise_sharded) maximum length."""
        y_max_length_ = fix_len_compatibility(y_max_length)
        y_mask = sequence_mask(y_lengths, y_max_length_).unsqueeze(1).to(x_mask.dtype)
        if self.encoder_stage == "host":
            attn_mask = x_mask.unsqueeze(-1) * y_mask.unsqueeze(2)
            attn = generate_path(w_ceil.squeeze(1), attn_mask.squeeze(1)).unsqueeze(1)
            mu_y = torch.matmul(attn.squeeze(1).transpose(1, 2), mu_x.transpose(1, 2)).transpose(1, 2)
        else:
            mu_y, attn = self.engine.align(w_ceil, mu_x, x_lengths, y_lengths, y_max_length_)
        encoder_outputs = mu_y[:, :, :y_max_length]
        dec, mel = self.decode(mu_y, y_lengths, n_timesteps, temperature, spk, z=z)
        return encoder_outputs, dec[:, :, :y_max_length], mel[:, :, :y_max_length], attn[:, :, :y_max_length]

    @torch.inference_mode()
    def synthesise(self, x, x_lengths, n_timesteps, temperature=1.0, spks=None, length_scale=1.0, *, z=None):
        """Reference matcha_tts.py:77-152.  Extension: keyword-only ``z`` (unit normal, (B, 80, Tp)) replaces the
        internal draw for bit-reproducible parity runs."""
        t0 = dt.datetime.now()
        spk, mu_x, w_ceil, x_mask, x_lengths, y_lengths, y_max_length = self._durations(x, x_lengths, spks, length_scale)
        if self.encoder_stage != "host":
            self.engine.text_encoder_status()        # out-of-range token id -> IndexError, as nn.Embedding raises
        encoder_outputs, dec, mel, attn = self._decode_aligned(spk, mu_x, w_ceil, x_mask, x_lengths, y_lengths, y_max_length,
                                                                n_timesteps, temperature, z=z)
        t = (dt.datetime.now() - t0).total_seconds()
        rtf = t * 22050 / (dec.shape[-1] * 256)
        return {
            "encoder_outputs": encoder_outputs,
            "decoder_outputs": dec,
            "attn": attn,
            "mel": mel,
            "mel_lengths": y_lengths,
            "rtf": rtf,
        }

    @torch.inference_mode()
    def warmup(self, n_tokens: int = 16, n_timesteps: int = 2, max_frames: int = 0, max_tokens: int = 0, batch: int = 1) -> None:
        """One tiny synthesis so that the first real request does not pay for code-object loading and the first workspace
        allocation (150-400 ms on a fresh process).  ``max_frames`` (mel frames of the longest utterance to expect; ``max_tokens``
        likewise for the text, default ``max_frames``) pre-sizes the workspace, scratch and staging through ``ev_reserve``, so
        that no later request up to that length allocates or re-plans on the request path.  No reference counterpart (torch's
        caching allocator amortises the same cost, feel_me.py:181-203)."""
        if max_frames > 0:
            self.engine.reserve(batch, max_tokens if max_tokens > 0 else max_frames, fix_len_compatibility(max_frames), 0)
        ids = torch.ones((1, n_tokens), dtype=torch.long, device=self.device)
        lens = torch.tensor([n_tokens], device=self.device)
        spks = torch.zeros((1,), dtype=torch.long, device=self.device) if self.n_spks > 1 else None
        self.synthesise(ids, lens, n_timesteps, 0.667, spks, 1.0)
        torch.cuda.synchronize(self.device)

    def draw_noise(self, B: int, Tp: int) -> torch.Tensor:
        """The reference draws ``randn_like(mu_y)`` (flow_matching.py:51) where ``mu_y`` is a transposed view
        (matcha_tts.py:134-135): the draw keeps those strides and uses torch's strided ``normal_`` path.  Doing
        exactly that on the CPU reproduces the reference's noise for a given ``torch.manual_seed``."""
        if self.rng == "device":
            return torch.randn(B, Tp, self.n_feats, device=self.device).transpose(1, 2)
        return torch.randn_like(torch.empty(B, Tp, self.n_feats).transpose(1, 2)).to(self.device)

    def decode(self, mu_y, y_lengths, n_timesteps, temperature=1.0, spk=None, z=None):
        """CFM.forward (flow_matching.py:32-53) + denormalize (utils/model.py:71-90) through the C ABI.
        Returns (decoder_outputs, mel), both (B, 80, Tp)."""
        B, _, Tp = mu_y.shape
        if z is None:
            z = self.draw_noise(B, Tp)
        x0 = (z.to(self.device) * temperature).contiguous()
        mu_c = mu_y.contiguous()
        if self.decode_graphs is not None and spk is not None:
            return self.decode_graphs.run(mu_c, y_lengths, spk, x0, n_timesteps)
        return self.engine.cfm_decode2(mu_c, y_lengths, spk, x0, n_timesteps, self.mel_std, self.mel_mean)

    def enable_decode_graphs(self, max_graphs: int = 256) -> "DecodeGraphs":
        """Replay the CFM decode from HIP graphs, one per (batch, padded length, step count) — the streaming loop's ~700 launches per
        utterance (feel_me.py:189-203) become one ``hipGraphLaunch``.  Call after ``warmup(max_frames=...)``: a captured decode needs
        the workspace to be there already.  Results are those of the eager call, bit for bit (``tests/test_gpu_configs.py``)."""
        self.decode_graphs = DecodeGraphs(self, max_graphs)
        return self.decode_graphs


class DecodeGraphs:
    """LRU cache of captured ``ev_cfm_decode2`` calls of one ``MatchaTTS``.  A graph owns static input / output tensors (inputs are
    copied in, outputs cloned out: ~0.4 MB per utterance); the engine keeps the graphs of different shapes valid beside each other
    and beside eager calls (include/emojivoice.h, "Graph capture").  A length that cannot be captured (workspace too small for it:
    not reserved) falls back to the eager call — and says so once."""

    def __init__(self, model: MatchaTTS, max_graphs: int = 256):
        self.model, self.max_graphs = model, int(max_graphs)
        self.stream = torch.cuda.Stream(device=model.device)
        self._cache: "Dict[tuple, dict]" = {}
        self._order: list = []
        self.hits = self.captures = self.fallbacks = 0
        self._warned = False

    def _capture(self, key, mu, lengths, spk, x0, n_timesteps):
        m = self.model
        ent = {"mu": mu.clone(), "len": lengths.to(m.device, torch.int32).clone(), "spk": spk.to(torch.float32).contiguous().clone(), "x0": x0.clone()}
        # one eager call first: it leaves the time-MLP output for this step count on the device (a captured call must find it there,
        # include/emojivoice.h "Graph capture") and is the plain-library error path for anything the shape cannot do
        m.engine.cfm_decode2(ent["mu"], ent["len"], ent["spk"], ent["x0"], n_timesteps, m.mel_std, m.mel_mean)
        cur = torch.cuda.current_stream(m.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=self.stream):
                ent["dec"], ent["mel"] = m.engine.cfm_decode2(ent["mu"], ent["len"], ent["spk"], ent["x0"], n_timesteps, m.mel_std, m.mel_mean)
        cur.wait_stream(self.stream)
        ent["graph"] = g
        self.captures += 1
        return ent

    def run(self, mu, lengths, spk, x0, n_timesteps):
        key = (tuple(mu.shape), int(n_timesteps))
        ent = self._cache.get(key)
        if ent is None:
            try:
                ent = self._capture(key, mu, lengths, spk, x0, n_timesteps)
            except Exception as e:  # noqa: BLE001 - the eager call is always available
                self.fallbacks += 1
                if not self._warned:
                    self._warned = True
                    print(f"[emojivoice_amd] decode graph for shape {key} not captured ({type(e).__name__}: {e}); running eagerly")
                m = self.model
                return m.engine.cfm_decode2(mu, lengths, spk, x0, n_timesteps, m.mel_std, m.mel_mean)
            self._cache[key] = ent
            self._order.append(key)
            if len(self._order) > self.max_graphs:
                old = self._order.pop(0)
                self._cache.pop(old, None)
        else:
            self.hits += 1
            self._order.remove(key)
            self._order.append(key)
        ent["mu"].copy_(mu); ent["len"].copy_(lengths); ent["spk"].copy_(spk); ent["x0"].copy_(x0)
        ent["graph"].replay()
        return ent["dec"].clone(), ent["mel"].clone()


# ---------------------------------------------------------------------------
# checkpoint reading without lightning / omegaconf
# ---------------------------------------------------------------------------
class _Stub(dict):
    """Inert stand-in for any class the checkpoint pickles that is not a tensor container (omegaconf nodes,
    functools.partial of an optimizer, lightning enums ...): accepts every way pickle builds or fills an object."""

    def __init__(self, *a, **k):
        super().__init__()

    def __call__(self, *a, **k):
        return self

    def __setstate__(self, s):
        pass

    def __reduce_ex__(self, protocol):
        return (_Stub, ())

    def append(self, *_):
        pass

    def extend(self, *_):
        pass

    def add(self, *_):
        pass

    def __setattr__(self, k, v):
        pass


# Exact (module, name) pairs a tensor checkpoint needs.  Everything else — including the rest of ``builtins`` (eval, exec,
# getattr, __import__ ...), ``torch`` (hub.load ...) and ``numpy`` (load ...) — resolves to the inert ``_Stub``: a pickle
# can name any importable callable in a REDUCE, so allow-listing whole modules is arbitrary code execution.
_ALLOWED_GLOBALS = {
    ("collections", "OrderedDict"), ("collections", "defaultdict"),
    ("torch._utils", "_rebuild_tensor_v2"), ("torch._utils", "_rebuild_tensor"), ("torch._utils", "_rebuild_parameter"),
    ("torch._utils", "_rebuild_parameter_with_state"),
    ("torch", "Size"), ("torch", "device"), ("torch", "dtype"),
    ("torch.serialization", "_get_layout"),
    ("numpy.core.multiarray", "_reconstruct"), ("numpy.core.multiarray", "scalar"),
    ("numpy._core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "scalar"),
    ("numpy", "dtype"), ("numpy", "ndarray"),
    ("_codecs", "encode"),
    ("builtins", "set"), ("builtins", "frozenset"), ("builtins", "dict"), ("builtins", "list"), ("builtins", "tuple"),
    ("builtins", "int"), ("builtins", "float"), ("builtins", "bool"), ("builtins", "str"), ("builtins", "bytes"),
    ("builtins", "bytearray"), ("builtins", "complex"), ("builtins", "slice"),
    ("__builtin__", "set"), ("__builtin__", "frozenset"), ("__builtin__", "dict"), ("__builtin__", "list"),
    ("__builtin__", "tuple"), ("__builtin__", "int"), ("__builtin__", "long"), ("__builtin__", "float"),
    ("__builtin__", "bool"), ("__builtin__", "complex"), ("__builtin__", "slice"),
}
_TORCH_STORAGES = {"FloatStorage", "DoubleStorage", "HalfStorage", "BFloat16Storage", "LongStorage", "IntStorage", "ShortStorage",
                   "CharStorage", "ByteStorage", "BoolStorage", "UntypedStorage"}
_TORCH_DTYPES = {"float32", "float64", "float16", "bfloat16", "int64", "int32", "int16", "int8", "uint8", "bool", "float", "double",
                 "half", "long", "int", "short"}


class _RestrictedUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if (module, name) in _ALLOWED_GLOBALS:
            if module == "__builtin__":
                module, name = "builtins", ("int" if name == "long" else name)
            return super().find_class(module, name)
        if module == "torch" and (name in _TORCH_STORAGES or name in _TORCH_DTYPES):
            return getattr(torch, name)
        return _Stub


class _PickleShim:
    Unpickler = _RestrictedUnpickler
    __name__ = "pickle"

    @staticmethod
    def load(f, **kw):
        return _RestrictedUnpickler(f, **kw).load()


def _load_ckpt(path):
    try:
        return torch.load(path, map_location="cpu", weights_only=True)
    except Exception:  # noqa: BLE001 - hyper_parameters hold non-tensor classes
        return torch.load(path, map_location="cpu", weights_only=False, pickle_module=_PickleShim)


def synthetic(n_vocab: int = W.N_VOCAB_DEFAULT, n_spks: int = W.N_SPKS_EMOJI, device="cuda:0") -> MatchaTTS:
    """Random-init model of the emoji architecture (no checkpoint exists offline)."""
    return MatchaTTS(W.synthetic_matcha_state(n_vocab, n_spks), device=device)
