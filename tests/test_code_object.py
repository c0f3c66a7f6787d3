"""Register / scratch census of the built library's gfx950 code object.

Round 3 shipped two U-Net kernels that ran out of registers: ``ln_mlp_h16_kernel`` (512 VGPR + AGPR, 150 spilled, 604 B of scratch per
lane) and ``conv_h16_bal_kernel`` (256, 64-113 spilled).  The cause was not the K loops but loop-invariant per-lane ADDRESSES (hand-off
slots, staging rows, the epilogue's row walk) that hipcc hoisted above the persistent unit loop and then spilled (DESIGN section 3,
"Registers").  This test reads the NT_AMDGPU_METADATA note of the code object inside ``libemojivoice_hip.so`` (tools/code_object.py) and
asserts, for every kernel on the config-2 launch list and for every build of the shipped arithmetic and of the batch-1 path:
``vgpr_spill_count == 0`` and ``private_segment_fixed_size == 0``.  Runs on CPU: the metadata is static.
"""
import importlib.util
import os
import re

import pytest

from emojivoice_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Kernels one config-2 step launches (names from the rocprofv3 kernel trace of `bench.py --no-extras`, profiles/r03_bench_b64_kernel_stats.csv
# and its round-4 successor; template arguments as the trace prints them).
CONFIG2_LAUNCH_LIST = [
    r"conv_h16_kernel<128, 128, 2, 2, 1, 1>", r"conv_h16_kernel<128, 128, 2, 2, 3, 1>", r"conv_h16_kernel<64, 128, 2, 2, 1, 1>",
    r"conv_h16_kernel<128, 128, 2, 2, 1, 0>", r"conv_h16_kernel<128, 128, 2, 2, 3, 0>", r"conv_h16_kernel<64, 128, 2, 2, 1, 0>",
    r"ln_mlp_h16_kernel<0>", r"ln_qkv_h16_kernel<0>", r"conv_h16_bal_kernel<128, 128, 2, 2, 1, 9, 9>",
    r"resblock_pair_h16_kernel<2, 2, 1>", r"resblock_pair_h16_kernel<1, 4, 1>", r"resblock_pair_h16_kernel<4, 1, 1>",
    r"resblock_pair_h16_kernel<2, 2, 3>", r"resblock_pair_h16_kernel<1, 4, 3>",
    r"resblock_chain_h16_kernel<1, 4, 1>", r"resblock_chain_h16_kernel<2, 2, 1>", r"resblock_chain_h16_kernel<1, 4, 3>", r"resblock_chain_h16_kernel<2, 2, 3>",
    r"attn_out_kernel", r"attn_out_h16_kernel", r"groupnorm_mish_kernel<512, false>",
    r"conv_gemm_kernel<64, 64, 2, 2, false, false, 1, 1>", r"conv_gemm_kernel<64, 64, 2, 2, false, false, 0, 1>",
    r"conv_gemm_kernel<64, 128, 2, 2, false, false, 1, 1>", r"conv_gemm_kernel<64, 64, 2, 2, true, true, 0, 1>",
    r"conv_gemm_kernel<32, 256, 1, 4, false, false, 0, 1>", r"conv_post_kernel<32, 7>", r"conv_gemm_sk_kernel<8, true, 0, 1>",
    r"conv_sk32_kernel<1>", r"cm_to_fm_kernel", r"fm_to_cm_kernel", r"rowmask_kernel", r"bcast_rows_kernel", r"zero_pads_kernel", r"strip_pad_kernel",
    r"chan_layernorm_kernel<4>", r"chan_layernorm_kernel<3>", r"enc_attention_kernel", r"enc_rope_kernel", r"enc_embed_kernel", r"enc_align_kernel",
]
# Builds that exist only for A/B runs of another arithmetic setting and still touch scratch (documented in DESIGN section 3, "Registers"):
# everything else in the library — every build of the shipped fp16 arithmetic, the exact-fp32 builds `value_fp32_mfma` runs on, the batch-1
# (small-launch) builds of config 5 — must be clean.
SCRATCH_ALLOWED = {
    "conv_split_bal_kernel<128, 128, 2, 2, 3, 6>(ConvParams)":            "bf16 six-product setting (EV_SPLIT=6), running-sum epilogue: 96 weight-ring + 64 accumulator + 48 operand registers",
    "ln_mlp_kernel<0, 3>(MlpParams)":                                     "fp32 MFMA, one tile per workgroup at three workgroups per CU (168-register cap): two address registers",
}


@pytest.fixture(scope="module")
def census():
    spec = importlib.util.spec_from_file_location("code_object", os.path.join(REPO, "tools", "code_object.py"))
    co = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(co)
    if not os.path.exists(co.READELF):
        pytest.skip("llvm-readelf of the ROCm toolchain is not installed")
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    ks = co.kernels(_lib.LIB_PATH)
    assert len(ks) > 150, "metadata note not parsed"
    return {k["demangled"]: k for k in ks}


def _find(census, pat):
    hits = [k for n, k in census.items() if n.startswith(pat) and (len(n) == len(pat) or n[len(pat)] in "(<")]
    assert hits, f"kernel {pat} is not in the library (launch list out of date?)"
    return hits


def test_config2_launch_list_has_no_spills_and_no_scratch(census):
    bad = []
    for pat in CONFIG2_LAUNCH_LIST:
        for k in _find(census, pat):
            if k["vgpr_spill_count"] != 0 or k["private_segment_fixed_size"] != 0:
                bad.append((k["demangled"], k["vgpr_spill_count"], k["private_segment_fixed_size"]))
    assert not bad, f"kernels on the config-2 launch list spill / use scratch: {bad}"


def test_the_two_round3_offenders_fit_their_register_files(census):
    """The numbers VERDICT round 3 quoted: 512 + 150 spilled / 256 + 64..113 spilled.  Now: inside the file, with room."""
    mlp = _find(census, "ln_mlp_h16_kernel<0>")[0]
    assert mlp["vgpr_spill_count"] == 0 and mlp["private_segment_fixed_size"] == 0 and mlp["vgpr_count"] <= 512
    for k in _find(census, "conv_h16_bal_kernel"):
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0 and k["vgpr_count"] <= 256, k


def test_whole_library_scratch_census(census):
    """No kernel outside the documented A/B builds touches scratch — the shipped arithmetic, the exact-fp32 setting and the batch-1 builds alike."""
    dirty = {n: (k["vgpr_spill_count"], k["private_segment_fixed_size"]) for n, k in census.items()
             if (k["vgpr_spill_count"] or k["private_segment_fixed_size"]) and n not in SCRATCH_ALLOWED}
    assert not dirty, f"kernels with spills / scratch that are not on the documented allow-list: {dirty}"
    stale = [n for n in SCRATCH_ALLOWED if n in census and not (census[n]["vgpr_spill_count"] or census[n]["private_segment_fixed_size"])]
    assert not stale, f"allow-list entries that are clean now (remove them): {stale}"


def test_every_h16_build_is_clean(census):
    for n, k in census.items():
        if re.search(r"h16", n):
            assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (n, k)
