"""The fp64 yardstick of tests/test_gpu_vocoder_v1.py, on the CPU: the V1 receptive field that lets a window stand in for a whole row,
window == row on interior, head and tail windows, restate == oracle.hifigan_forward for V1, and the linear-regime checkpoint."""
import torch

from emojivoice_amd import weights as W
from oracle import matcha_oracle as O
from vocoder_ref import HOP, MARGIN, linear_regime_state, restate, restate_body, restate_post, restate_windows

V1 = W.HIFIGAN_V1
REACH = 14           # frames either side of a changed mel frame whose output may change (measured: 12.4 left, 13.4 right)


def _mel(B, T, seed):
    return torch.randn(B, 80, T, generator=torch.Generator().manual_seed(seed)) * 2.0 - 5.0


def test_receptive_field_is_bounded():
    """A change to mel frame f changes no output sample outside frames [f - 14, f + 14]; it does reach past 12 frames on either side
    (the bound is tight, so MARGIN = 16 is not an accident of a small field)."""
    sd = W.synthetic_hifigan_state()
    T, f = 64, 31
    mel = _mel(1, T, 1)
    bumped = mel.clone()
    bumped[0, :, f] += torch.randn(80, generator=torch.Generator().manual_seed(2))
    d = (restate(sd, bumped, V1) - restate(sd, mel, V1))[0, 0].abs()
    changed = torch.nonzero(d > 0).flatten()
    lo, hi = int(changed.min()), int(changed.max())
    assert lo >= HOP * (f - REACH) and hi < HOP * (f + REACH + 1), (lo / HOP, hi / HOP)
    assert lo < HOP * (f - 12) and hi >= HOP * (f + 13), (lo / HOP, hi / HOP)
    assert REACH < MARGIN


def test_windows_equal_the_full_row():
    """restate_windows on head, tail, partly clipped and random interior windows == the same frames of the full rows, for both
    checkpoints (the body is shared; only conv_post differs)."""
    sds = [W.synthetic_hifigan_state(), linear_regime_state()]
    B, T = 2, 100
    mel = _mel(B, T, 3)
    body = restate_body(sds[0], mel, V1)
    full = [restate_post(sd, body)[:, 0] for sd in sds]
    g = torch.Generator().manual_seed(4)
    wins = [(0, 0, 8), (1, T - 8, T), (0, 5, 13), (1, T - 20, T - 3), (0, 0, T)]
    for _ in range(4):
        t0 = int(torch.randint(MARGIN, T - MARGIN - 8, (1,), generator=g))
        wins.append((int(torch.randint(0, B, (1,), generator=g)), t0, t0 + int(torch.randint(1, 9, (1,), generator=g))))
    got = restate_windows(sds, mel, V1, wins, margin=MARGIN)
    for i in range(len(sds)):
        for n, (r, t0, t1) in enumerate(wins):
            ref = full[i][r, HOP * t0:HOP * t1]
            assert got[i][n].shape == ref.shape
            assert float((got[i][n] - ref).abs().max()) <= 1e-12, (i, wins[n])


def test_restate_equals_the_oracle_for_v1():
    sd = {k: v.double() for k, v in W.synthetic_hifigan_state().items()}
    mel = _mel(2, 20, 5).double()
    ref = O.hifigan_forward(sd, mel, V1)
    got = restate(sd, mel, V1)
    assert ref.dtype == torch.float64 and got.shape == ref.shape
    assert float((got - ref).abs().max()) <= 1e-12


def test_linear_regime_checkpoint_keeps_tanh_linear():
    """Standard weights saturate the output tanh (an upstream error at a saturated sample reaches the waveform shrunk by tanh');
    the linear-regime checkpoint (conv_post x 0.05) keeps fewer than 1 % of the samples above |0.5|, and is not silent."""
    sd, lin = W.synthetic_hifigan_state(), linear_regime_state()
    assert set(sd) == set(lin)
    assert all(torch.equal(sd[k], lin[k]) for k in sd if not k.startswith("conv_post."))
    mel = _mel(2, 48, 6)
    body = restate_body(sd, mel, V1)
    std_wav, lin_wav = restate_post(sd, body), restate_post(lin, body)
    assert float((std_wav.abs() > 0.95).double().mean()) > 0.1
    assert float((lin_wav.abs() > 0.5).double().mean()) < 0.01
    assert float(lin_wav.pow(2).mean().sqrt()) > 0.02
