"""The fp64 yardstick of tests/test_gpu_vocoder_configs_fp64.py, on the CPU, for every generator config that file runs: V2, V3, the
four-level ResBlock2 config of the golden (``offstd``) and the two configs with a wide last level (``v3_512``, ``rb1_2lvl``).

  reach      ``vocoder_ref.reach(h)`` bounds the receptive field (a bumped mel frame moves nothing outside it) and is tight to within a
             frame, so the margin ``restate_windows`` derives from it is neither too small nor an accident of a small field; ``offstd``
             reaches 18.62 frames, past V1's margin of 16, and a window computed at 16 is wrong
  windows    head, tail, clipped and interior windows == the full row, for the standard and the linear-regime checkpoint
  regime     the standard checkpoint saturates the output tanh, the linear-regime one (conv_post x 0.05) does not and is not silent
  sensitive  a restatement with one dilation off by one, or a leaky_relu slope of 0.11, misses the true one by more than the per-row
             gates of the GPU tests on every row: those gates would see such a kernel
"""
import pytest
import torch

from emojivoice_amd import weights as W
from emojivoice_amd.hifigan import v2, v3
from test_vocoder_configs import WIDE_LAST, golden_config, golden_vocoder
from vocoder_ref import GATE, HOP, MARGIN, default_margin, linear_regime_state, reach, restate_body, restate_post, restate_windows, row_errors

NAMES = ("v2", "v3", "offstd", "v3_512", "rb1_2lvl")
T = 96


def configs():
    """{name: config} of the generators the per-row tests cover (plain dicts; ``offstd`` is the golden's)."""
    return dict({"v2": dict(v2), "v3": dict(v3), "offstd": dict(golden_config(golden_vocoder(), "offstd"))}, **WIDE_LAST)


_CACHE = {}


def _case(name):
    """One config's T = 96 case, computed once: config, both checkpoints, a 2-row mel, the fp64 body and both full waveforms."""
    if name not in _CACHE:
        h = configs()[name]
        sds = [W.synthetic_hifigan_state(h), linear_regime_state(h)]
        mel = torch.randn(2, 80, T, generator=torch.Generator().manual_seed(960 + NAMES.index(name))) * 2.0 - 5.0
        body = restate_body(sds[0], mel, h)
        _CACHE[name] = (h, sds, mel, body, [restate_post(sd, body)[:, 0] for sd in sds])
    return _CACHE[name]


@pytest.mark.parametrize("name", NAMES)
def test_reach_bounds_the_receptive_field_and_is_tight(name):
    """Frames left of the bumped frame's first sample and right of its last one that change.  Measured (bound): v2 12.68 / 12.66 (12.73),
    v3 and v3_512 10.09 (10.09), offstd 18.62 (18.62), rb1_2lvl 7.53 (7.53): the ResBlock2 configs and the 16x upsamplers attain the
    bound, V2's k = 4, u = 2 upsamplers feed each output sample from two taps only and fall 13 and 18 samples short of it."""
    h, sds, mel, _, _ = _case(name)
    f = 47
    both = torch.cat([mel[:1], mel[:1]])                  # (one call for both: the same arithmetic wherever the bump does not reach)
    both[1, :, f] += torch.randn(80, generator=torch.Generator().manual_seed(2))
    wav = restate_post(sds[1], restate_body(sds[1], both, h))[:, 0]       # (the linear-regime output: no sample saturates)
    d = (wav[1] - wav[0]).abs()
    changed = torch.nonzero(d > 0).flatten()
    left, right = f - int(changed.min()) / HOP, (int(changed.max()) + 1) / HOP - (f + 1)
    print(f"REACH {name:<9s} bound {reach(h):.4f}  measured left {left:.4f}  right {right:.4f}  margin {default_margin(h)}")
    assert left <= reach(h) and right <= reach(h), (left, right, reach(h))
    assert left > reach(h) - 1 and right > reach(h) - 1, (left, right, reach(h))
    assert default_margin(h) >= reach(h) + 2 > 2 and default_margin(h) + f + 1 <= T and f - default_margin(h) >= 0   # (the bump sat clear of both ends)


def test_offstd_needs_more_than_the_v1_margin():
    """The offstd config reaches 18.62 frames: an interior window run on 16 frames of context differs from the full row, and the margin
    derived from the config does not.  (This is why the margin follows the config.)"""
    h, sds, mel, _, full = _case("offstd")
    assert reach(h) > MARGIN and default_margin(h) == 21
    win = [(0, 40, 48)]
    ref = full[0][0, HOP * 40:HOP * 48]
    short = restate_windows(sds, mel, h, win, margin=MARGIN)[0][0]
    assert float((short - ref).abs().max()) > 1e-9
    assert float((restate_windows(sds, mel, h, win)[0][0] - ref).abs().max()) <= 1e-12


@pytest.mark.parametrize("name", NAMES)
def test_windows_equal_the_full_row(name):
    h, sds, mel, _, full = _case(name)
    m = default_margin(h)
    g = torch.Generator().manual_seed(4)
    wins = [(0, 0, 8), (1, T - 8, T), (0, 5, 13), (1, T - 20, T - 3), (0, 0, T)]
    for _ in range(4):
        t0 = int(torch.randint(m, T - m - 8, (1,), generator=g))
        wins.append((int(torch.randint(0, 2, (1,), generator=g)), t0, t0 + int(torch.randint(1, 9, (1,), generator=g))))
    got = restate_windows(sds, mel, h, wins)
    for i in range(len(sds)):
        for n, (r, t0, t1) in enumerate(wins):
            ref = full[i][r, HOP * t0:HOP * t1]
            assert got[i][n].shape == ref.shape
            assert float((got[i][n] - ref).abs().max()) <= 1e-12, (i, wins[n])


@pytest.mark.parametrize("name", NAMES)
def test_linear_regime_checkpoint_keeps_tanh_linear(name):
    _, sds, _, _, (std_wav, lin_wav) = _case(name)
    assert all(torch.equal(sds[0][k], sds[1][k]) for k in sds[0] if not k.startswith("conv_post."))
    assert float((std_wav.abs() > 0.95).double().mean()) > 0.1
    assert float((lin_wav.abs() > 0.5).double().mean()) < 0.01
    for r in range(lin_wav.shape[0]):
        assert float(lin_wav[r].pow(2).mean().sqrt()) > 0.02


def _mutations(h):
    """(label, config, slope): the first dilation of each ResBlock one larger (the weights' shapes do not depend on it), and the slope."""
    out = []
    for j in range(3):
        rd = [list(ds) for ds in h["resblock_dilation_sizes"]]
        rd[j][0] += 1
        out.append((f"k = {h['resblock_kernel_sizes'][j]} dilation {rd[j][0] - 1} -> {rd[j][0]}", dict(h, resblock_dilation_sizes=rd), 0.1))
    return out + [("slope 0.1 -> 0.11", h, 0.11)]


@pytest.mark.parametrize("name", NAMES)
def test_the_gates_see_a_wrong_dilation_and_a_wrong_slope(name):
    """Each mutated restatement, taken as if it were the kernel's output, misses BOTH per-row gates (RMS and L-inf) of the GPU tests on
    every row, under either checkpoint: std absolute, lin relative to the row's fp64 RMS."""
    h, sds, mel, _, full = _case(name)
    wins = [(r, 0, T) for r in range(mel.shape[0])]
    for label, hm, slope in _mutations(h):
        body = restate_body(sds[0], mel, hm, slope=slope)
        for i, w in enumerate(("std", "lin")):
            wav = restate_post(sds[i], body)
            for r, (rms, linf, rr, _) in row_errors(wav, wins, list(full[i])).items():
                scale = 1.0 if w == "std" else rr
                assert rms > GATE[w][0] * scale and linf > GATE[w][1] * scale, (name, label, w, r, rms, linf, rr)
