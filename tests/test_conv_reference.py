"""Host-only checks of tests/conv_ref.py: the restatement is the convolution torch computes, the yardstick is finite, no frame is gated
against nothing, the input classes stay inside their dynamic-range window and every mutant falls outside the gates it is held against.
Nothing here touches the GPU or the engine."""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R

F64 = torch.float64
ALL_BUILDS = R.FORCED_BUILDS + R.BALANCED_BUILDS
SMALL = sorted(n for n, L in R.LAYERS.items() if L["B"] == 3)


def _torch_conv(L, x, w):
    if L["form"] == "same":
        return F.conv1d(x, w, padding=L["padding"], dilation=L["d"])
    if L["form"] == "s2":
        return F.conv1d(x, w, stride=2, padding=1)
    return F.conv_transpose1d(x, w, stride=L["stride"], padding=L["padding"])


@pytest.mark.parametrize("layer", sorted(R.LAYERS))
def test_restatement_is_the_convolution(layer):
    """fp64, every shape tests/test_gpu_conv.py runs: sum-over-taps equals F.conv1d / F.conv_transpose1d to 1e-12 of the output scale, with
    the layer's own pad rows and with more of them."""
    L = R.LAYERS[layer]
    c = R.case(layer)
    x, w = c["x"].double(), c["w"].double()
    want = _torch_conv(L, x, w)
    got = R.conv(L, x, w)
    assert got.shape == want.shape == (L["B"], L["Cout"], R.out_frames(L))
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    if L["form"] == "same" and L["B"] == 3:
        assert torch.equal(R.conv(L, x, w, P=L["P"] + 5), got), "the sums do not depend on the pad rows"
    assert L["P"] >= R.halo_rows(L) * (2 if L["form"] == "s2" else 1)
    S = L["T"] + 2 * L["P"]
    assert L["T"] < 32 or S % 32 != 0, "tiles must straddle utterances"


def test_epilogue_order_against_plain_torch():
    """The documented order, written out once more without the restatement's switches."""
    c = R.case("k3", "randn", "mrf2")
    x, w = c["x"].double(), c["w"].double()
    v = F.conv1d(F.leaky_relu(x, 0.1), w, c["bias"].double(), padding=1)
    want = F.leaky_relu((v + c["R"].double() + c["yold"].double()) / 3, 0.25)
    got, _ = R.evaluate(c, F64)
    assert float((got - want).abs().max()) <= 1e-12
    c = R.case("c224", "randn", "euler")
    m = c["mask"].double()
    v = F.conv1d(c["x"].double(), c["w"].double(), c["bias"].double(), padding=1) * m * float(torch.tensor(R.DT)) + c["R"].double()
    got, got2 = R.evaluate(c, F64)
    assert float((got - v).abs().max()) <= 1e-12 and torch.equal(got2, got * m)
    c = R.case("k3", "randn", "snake")
    v = F.conv1d(c["x"].double(), c["w"].double(), c["bias"].double(), padding=1)
    want = v + c["beta_inv"].double()[None, :, None] * torch.sin(v * c["alpha_exp"].double()[None, :, None]) ** 2
    assert float((R.evaluate(c, F64)[0] - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("build", ALL_BUILDS)
def test_plan_is_gateable(build):
    """Every case of a build: finite fp32 yardstick, every frame's rms A above A_RMS_FLOOR, the class inside its 2^12 window, the plain
    fp32 evaluation inside its own gate, and the references' masked frames exact."""
    for layer, cls, epi in R.plan(build):
        L = R.LAYERS[layer]
        if L["B"] > 3 and (cls not in ("randn", "rows") or epi not in ("plain", "mrf2")):
            continue                                       # (the 8256-row cases: the GPU module computes the rest once, there)
        c = R.case(layer, cls, epi)
        y64, z64, y32, z32, A = R.references(c)
        tag = f"{build} {layer} {cls} {epi}"
        assert bool(torch.isfinite(y32).all()) and bool(torch.isfinite(y64).all()), tag
        assert float(A.pow(2).mean(dim=1).sqrt().min()) >= R.A_RMS_FLOOR, tag
        assert bool((A >= y64.abs() * (1 - 1e-12)).all()) or R.EPIS[epi].get("act") in ("silu", "mish", "snake"), tag
        assert R.window_range(cls, L) < R.RANGE_LIMIT, tag
        bad, worst = R.failures(y32, z32, c, build, tag)
        assert not bad and worst <= 1.0 / R.MARGIN + 1e-12, (bad, worst)
        if L["form"] != "T":
            assert int(c["lengths"].min()) < R.out_frames(L) or R.out_frames(L) == 1, "ragged"


@pytest.mark.parametrize("name", sorted(R.MUTANTS))
def test_mutant_is_outside_the_gate(name, capsys):
    """Each wrong reference exceeds the gate of the builds it is held against by at least 10 x on at least one frame."""
    builds = R.MUTANT_BUILDS.get(name, (0, 46, 40))
    shown = builds if R.LAYERS[R.MUTANTS[name][0]]["Cin"] % 64 else tuple(dict.fromkeys(builds + (46, 40)))     # (report: the 16-bit gates too)
    ratios = {b: R.mutant_ratio(name, b) for b in shown}
    with capsys.disabled():
        print(f"\n  mutant {name:11s} on {R.MUTANTS[name]}: worst error / gate " + "  ".join(f"build {b}: {r:.3g}" for b, r in ratios.items()))
    for b in builds:
        assert ratios[b] >= 10.0, (name, b, ratios[b])


def test_masked_frame_rules_catch_a_late_mask():
    """mask1 applied after +R leaves 0 where R belongs: the exactness rule fails it, apart from the gate."""
    c = R.case("k3", "randn", "m1_R")
    y, _ = R.evaluate(c, torch.float32, mut="mask_late")
    assert any("masked frames" in str(b) for b in R.masked_failures(y, None, c))
    good, _ = R.evaluate(c, torch.float32)
    assert not R.masked_failures(good, None, c)


def test_truncation_pieces_are_exact_and_the_pipe_constants():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4096, generator=g) * 10.0 ** torch.randint(-3, 4, (4096,), generator=g).float()
    assert torch.equal(R.truncate_bf16(x, 3), x)
    r1 = (x - R.truncate_bf16(x, 1)).abs()
    r2 = (x - R.truncate_bf16(x, 2)).abs()
    assert bool((r1 < 2.0 ** -7 * x.abs()).all()) and bool((r2 < 2.0 ** -14 * x.abs()).all()), "the bounds C_BF16 is derived from"
    assert R.C_BF16 == 2 * 2.0 ** -21 + 2.0 ** -28 and R.C_FP16 == 3 * 2.0 ** -22
    assert R.c_pipe(19) == 0.0 and R.c_pipe(47) == R.C_FP16 and R.c_pipe(60) == R.C_BF16
    assert set(ALL_BUILDS) == set(R.FP32_BUILDS + R.FP16_BUILDS + R.BF16_BUILDS)
