"""Host side of the batched flow-matching loss: the C ABI's declarations and exports (ev_estimator_rows, ev_cfm_loss), the Python
surface (MatchaTTS.forward(batched=), MatchaTTS.score, Engine.estimator_rows / cfm_loss), and the host formulas that turn the row sums
of ev_cfm_loss into the three losses, against tests/mas_ref.py on a float64 velocity.  No GPU."""
import inspect
import math
import os
import re
import subprocess

import numpy as np
import torch

import mas_ref as R
from emojivoice_amd import _lib
from emojivoice_amd import matcha_tts as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ev_estimator_rows", "ev_cfm_loss")


def test_c_abi_declares_and_exports_the_per_row_calls():
    with open(os.path.join(REPO, "include", "emojivoice.h")) as f:
        header = f.read()
    for n in NAMES:
        assert re.search(rf"\bint\s+{n}\s*\(\s*ev_handle\s*\*", header), f"{n} is not declared in include/emojivoice.h"
        assert n in _lib.EXPORTS
    m = re.search(r"\bint\s+ev_cfm_loss\s*\(([^;]*)\)\s*;", header)
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.search(r"double\s*\*\s*d_row_sums", args) and re.search(r"float\s+sigma_min", args) and re.search(r"int\s+B\s*,\s*int\s+Ty", args)
    assert len(args.split(",")) == 13
    assert re.search(r"#define\s+EV_ABI_VERSION\s+4\b", header), "additions that change nothing of 4 keep the version"
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = _lib.load_library()
    assert lib.ev_abi_version() == 4
    for n in NAMES:
        assert hasattr(lib, n), f"{n} is not exported by the built library"
    nm = "/opt/rocm/llvm/bin/llvm-nm"
    if os.path.exists(nm):
        syms = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        for n in NAMES:
            assert re.search(rf"\sT\s+{n}\b", syms), n


def test_python_surface():
    fwd = inspect.signature(M.MatchaTTS.forward).parameters
    assert fwd["batched"].kind is inspect.Parameter.KEYWORD_ONLY and fwd["batched"].default is False
    assert list(fwd)[:9] == ["self", "x", "x_lengths", "y", "y_lengths", "spks", "out_size", "cond", "durations"], "the reference's positional surface"
    assert M.MatchaTTS.__call__ is M.MatchaTTS.forward
    sc = inspect.signature(M.MatchaTTS.score).parameters
    assert list(sc) == ["self", "x", "x_lengths", "y", "y_lengths", "spks", "durations", "t", "z"]
    assert sc["t"].kind is inspect.Parameter.KEYWORD_ONLY and sc["z"].kind is inspect.Parameter.KEYWORD_ONLY and "out_size" not in sc
    assert list(inspect.signature(_lib.Engine.estimator_rows).parameters) == ["self", "x", "mu", "lengths", "spk", "t"]
    cl = inspect.signature(_lib.Engine.cfm_loss).parameters
    assert list(cl) == ["self", "x1", "mu_y", "y_lengths", "spk", "z", "t", "sigma_min", "want_v"] and cl["want_v"].default is False


def test_the_engine_forms_the_reference_float32_constant():
    """ev_cfm_loss takes sigma_min as a float and forms float(1 - double(sigma_min)); torch multiplies a float32 tensor by the Python
    scalar 1 - 1e-4 rounded to float32.  The same bits, so y_t and u are the reference's float32 values."""
    c_engine = np.float32(1.0 - float(np.float32(R.SIGMA_MIN)))
    c_torch = (torch.ones(1) * (1 - R.SIGMA_MIN)).numpy()[0]
    assert c_engine.tobytes() == c_torch.tobytes()


def _rows_case(seed=4):
    """A batch with ragged lengths, a full row and a one-frame row, all in float64; v is 0 on padded frames as the estimator's is."""
    g = torch.Generator().manual_seed(seed)
    B, Tx, Ty = 5, 7, 23
    xl, yl = torch.tensor([7, 1, 4, 3, 5]), torch.tensor([23, 1, 4, 17, 9])
    mu_x = torch.randn(B, 80, Tx, generator=g, dtype=torch.float64)
    y, z = torch.randn(B, 80, Ty, generator=g, dtype=torch.float64), torch.randn(B, 80, Ty, generator=g, dtype=torch.float64)
    logw = torch.randn(B, 1, Tx, generator=g, dtype=torch.float64) * (torch.arange(Tx)[None, None, :] < xl[:, None, None])
    t = torch.rand(B, generator=g, dtype=torch.float64)
    path, _ = R.maximum_path(R.log_prior(mu_x, y).float(), xl, yl)
    attn = torch.from_numpy(path.astype(np.float64))
    y_mask = (torch.arange(Ty)[None, :] < yl[:, None]).double().unsqueeze(1)
    v = torch.randn(B, 80, Ty, generator=g, dtype=torch.float64) * y_mask
    return xl, yl, mu_x, y, z, logw, t, attn, y_mask, v


def test_host_formulas_agree_with_the_float64_yardsticks():
    xl, yl, mu_x, y, z, logw, t, attn, y_mask, v = _rows_case()
    B = y.shape[0]
    d64, p64, mu_y = R.dur_and_prior_loss(attn, logw, mu_x, y, xl, yl)
    _, u = R.cfm_inputs(y, t, z)
    l64 = R.diff_loss_from_velocity(v, u, yl)
    # the row sums as ev_cfm_loss defines them: over each row's valid cells only
    sums = torch.stack([torch.sum(((v - u) ** 2) * y_mask, dim=(1, 2)), torch.sum(0.5 * ((y - mu_y) ** 2 + math.log(2 * math.pi)) * y_mask, dim=(1, 2))], dim=1)
    x_mask = (torch.arange(logw.shape[-1])[None, :] < xl[:, None]).double().unsqueeze(1)
    logw_ = torch.log(1e-8 + attn.sum(-1)).unsqueeze(1) * x_mask
    pad = M.padded_frames_sum(y, z, yl, R.SIGMA_MIN)
    assert pad.dtype == torch.float64 and float(pad) > 0, "ragged rows: the reference's sum has a padded-frame share"
    dur, prior, diff = M.batch_losses(sums, pad, logw, logw_, xl, yl)
    assert abs(float(dur) - d64) <= 1e-12 * d64 and abs(float(prior) - p64) <= 1e-12 * p64 and abs(float(diff) - l64) <= 1e-12 * l64
    assert abs(float(M.batch_losses(sums, 0.0, logw, logw_, xl, yl)[2]) - l64) > 1e-3 * l64, "without that share the batch value is another number"
    rows = M.row_losses(sums, logw, logw_, xl, yl)
    for b in range(B):
        one = slice(b, b + 1)
        L, Lx = int(yl[b]), int(xl[b])
        d_b, p_b, _ = R.dur_and_prior_loss(attn[one, :Lx, :L], logw[one, :, :Lx], mu_x[one, :, :Lx], y[one, :, :L], xl[one], yl[one])
        l_b = R.diff_loss_from_velocity(v[one, :, :L], u[one, :, :L], yl[one])
        for k, want in (("dur_loss", d_b), ("prior_loss", p_b), ("diff_loss", l_b)):
            assert rows[k].shape == (B,) and abs(float(rows[k][b]) - want) <= 1e-12 * max(want, 1.0), (b, k)
    # a batch of full rows has no padded share, and then batch and row values are the same thing
    full = torch.full_like(yl, y.shape[2])
    assert float(M.padded_frames_sum(y, z, full, R.SIGMA_MIN)) == 0.0
