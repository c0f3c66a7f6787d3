"""HiFi-GAN V2 / V3 and other configs inside the supported envelope: the CPU side (names, shapes, weights, envelope, ABI, code object).

``restate`` (tests/vocoder_ref.py) is a plain-torch statement of ``matcha.hifigan.models.Generator.forward`` for ResBlock1 and ResBlock2
(models.py:80-197) at any config and precision; it is checked here against the reference's own output (tests/golden/vocoder_configs.npz, written by
tests/golden/make_vocoder_golden.py) and serves the GPU tests (test_gpu_vocoder_configs.py) as their fp64 yardstick for shapes the
golden does not hold.  oracle.matcha_oracle.hifigan_forward knows ResBlock1 only.
"""
import hashlib
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

from emojivoice_amd import _lib
from emojivoice_amd import weights as W
from emojivoice_amd.hifigan import AttrDict, Generator, check_config, v1, v2, v3
from vocoder_ref import restate  # noqa: F401  (test_gpu_vocoder_configs imports it from here)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "vocoder_configs.npz")
NAMES = ("v2", "v3", "offstd")


# configs whose last level is neither 8, 16 nor 32 channels: conv_post runs as a generic conv launch + a pass that strips the pad rows
WIDE_LAST = {
    "v3_512": dict(v3, upsample_initial_channel=512),                                  # levels 256 / 128 / 64, ResBlock2 at 256 on the conv launches
    "rb1_2lvl": dict(v1, upsample_rates=[16, 16], upsample_kernel_sizes=[32, 32], upsample_initial_channel=256),   # two levels: 128 / 64
}


def golden_vocoder():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def golden_config(g, name):
    return AttrDict(json.loads(str(g[f"{name}_config"])))


# ---- names, shapes, weights ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_shapes_equal_the_reference_modules(name):
    g = golden_vocoder()
    h = golden_config(g, name)
    want = {str(k): tuple(int(d) for d in s if d) for k, s in zip(g[f"{name}_param_names"], g[f"{name}_param_shapes"])}
    got = {k: tuple(s) for k, s in W.hifigan_shapes(h).items()}
    assert got == want


def test_v2_v3_dicts_are_the_golden_configs():
    """Pins v2 / v3 against drift from the configs the golden was generated with (which were these dicts: this does not check them
    against the upstream config_v2.json / config_v3.json)."""
    g = golden_vocoder()
    for name, h in (("v2", v2), ("v3", v3)):
        assert all(h[k] == v for k, v in golden_config(g, name).items()), name


def test_v1_shapes_and_synthetic_weights_unchanged():
    """Digests of hifigan_shapes(V1) and synthetic_hifigan_state(V1) as they were before ResBlock2 support (the committed goldens use them)."""
    hs = hashlib.sha256()
    for k, s in W.hifigan_shapes(W.HIFIGAN_V1).items():
        hs.update(f"{k}:{tuple(s)};".encode())
    assert hs.hexdigest() == "e5172dac80b1a45d6426a757b300d7e4d1143e9df3cb8fd208b00339ab57af91"
    hw = hashlib.sha256()
    for k, t in W.synthetic_hifigan_state(W.HIFIGAN_V1).items():
        hw.update(k.encode())
        hw.update(t.contiguous().numpy().tobytes())
    assert hw.hexdigest() == "408757bf26f8389b515c0f8b4f40bafec64e6cb69417f33ef8e2cec82393b25f"


def test_resblock2_convs_are_damped():
    sd = W.synthetic_hifigan_state(v3)
    for k, t in sd.items():
        if ".convs." in k and k.endswith(".weight"):
            assert abs(float(t.std()) * (t.shape[1] * t.shape[2]) ** 0.5 - 0.5) < 0.05, k


def test_generator_v3_constructs_and_loads_strict():
    g = Generator(AttrDict(v3))
    assert g.num_kernels == 3 and g.num_upsamples == 3
    g.load_state_dict(W.synthetic_hifigan_state(v3), strict=True)
    g.load_state_dict(W.weight_norm_split(W.synthetic_hifigan_state(v3)), strict=True)   # the raw checkpoint form
    with pytest.raises(RuntimeError):
        g.load_state_dict(W.synthetic_hifigan_state(v1), strict=True)


# ---- the envelope -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("change,needle", [
    (dict(upsample_rates=[8, 8, 2, 4], upsample_kernel_sizes=[16, 16, 4, 8]), "product of upsample_rates"),
    (dict(resblock_kernel_sizes=[3, 7], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5]]), "exactly 3 resblock kernel sizes"),
    (dict(upsample_initial_channel=64), "not a multiple of 8"),
    (dict(upsample_kernel_sizes=[16, 16, 4, 5]), "k - u even"),
    (dict(resblock_kernel_sizes=[3, 6, 11]), "odd"),
    (dict(resblock_dilation_sizes=[[1, 3], [1, 3], [1, 3]]), "3 dilations"),
    (dict(num_mels=100), "num_mels"),
    (dict(upsample_rates=[4, 4, 4, 2, 2], upsample_kernel_sizes=[8, 8, 8, 4, 4]), "1 to 4 upsampling levels"),
])
def test_configs_outside_the_envelope_raise(change, needle):
    h = AttrDict(dict(v2, **change))   # V2: the change alone breaks it (its last level is 8 channels)
    with pytest.raises(ValueError, match=re.escape(needle)):
        Generator(h)


def test_envelope_holds_the_published_configs():
    for h in (v1, v2, v3):
        check_config(h)
    with pytest.raises(ValueError, match="halo"):
        check_config(dict(v3, resblock_dilation_sizes=[[1, 2], [2, 6], [3, 30]]))


def test_cli_reads_a_config_json(tmp_path):
    from emojivoice_amd.cli import vocoder_config

    path = tmp_path / "config.json"
    path.write_text(json.dumps(dict(v3)))
    assert vocoder_config(str(path))["resblock_dilation_sizes"] == [[1, 2], [2, 6], [3, 12]]
    assert vocoder_config("v2")["upsample_initial_channel"] == 128
    path.write_text(json.dumps(dict(v3, upsample_rates=[8, 8, 8])))
    with pytest.raises(ValueError):
        vocoder_config(str(path))


def test_chunk_sizing_follows_the_config():
    assert _lib.vocoder_frame_bytes(v1) == (256 * 128, 4)                    # the V1 sizing Engine.hifigan always used
    assert _lib.vocoder_frame_bytes(v3) == (256 * 32 * 4, 5)                 # level 3: 256 x 32 channels; k = 7, d = 12 needs 36 pad frames at level 1
    assert _lib.vocoder_frame_bytes(v2) == (8 * 64 * 4 * 4, 4)


# ---- the restatement against the reference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_golden(name):
    g = golden_vocoder()
    h = golden_config(g, name)
    wav = restate(W.synthetic_hifigan_state(h), torch.from_numpy(g[f"{name}_mel"]), h)
    err = wav.numpy() - g[f"{name}_wav"]
    assert float(np.abs(err).max()) <= 1e-5


# ---- C ABI and code object ----------------------------------------------------------------------------------------------------------------
def test_config_entry_point_is_exported():
    assert "ev_load_vocoder_cfg" in _lib.EXPORTS
    with open(os.path.join(REPO, "include", "emojivoice.h")) as f:
        hdr = f.read()
    assert "ev_vocoder_config" in hdr and re.search(r"\bev_load_vocoder_cfg\s*\(", hdr)
    import ctypes

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "ev_load_vocoder_cfg")
    assert ctypes.sizeof(_lib.ev_vocoder_config) == 4 * (2 + 4 + 4 + 3 + 9)


def test_resblock2_kernel_has_no_spills_and_no_scratch():
    spec = importlib.util.spec_from_file_location("code_object", os.path.join(REPO, "tools", "code_object.py"))
    co = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(co)
    if not os.path.exists(co.READELF):
        pytest.skip("llvm-readelf of the ROCm toolchain is not installed")
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    ks = [k for k in co.kernels(_lib.LIB_PATH) if k["demangled"].startswith("resblock2_h16_kernel<")]
    assert len(ks) == 6, [k["demangled"] for k in ks]                       # C = 32 / 64 / 128, plain and running-sum epilogues
    bad = [(k["demangled"], k["vgpr_spill_count"], k["private_segment_fixed_size"]) for k in ks
           if k["vgpr_spill_count"] != 0 or k["private_segment_fixed_size"] != 0]
    assert not bad
