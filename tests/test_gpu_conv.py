"""Every conv build and every epilogue flavour on a real MI355X, per output frame against the fp64 restatement of tests/conv_ref.py.

How a case gets to its kernel: Engine.op_conv1d_epi (ev_op_conv1d_epi) packs the layer and stages the input as ev_op_conv1d does and calls
launch_conv ONCE with the case's epilogue and pad rows.  Every case asserts Engine.last_cfg() — a case that lands on another build fails —,
repeats the launch and compares the bits, checks that every pad row of the padded Y still holds the sentinel the hook put there, and holds the
valid frames (and Y2) to the gate of the build's pipe, masked frames exactly (conv_ref.failures).

  test_forced_build[code]    one Engine under EV_FORCE_CFG=<code>, B = 3, a few hundred frames, S = T + 2 P no multiple of 32 (tiles straddle
                             utterances, last tile partial), plus T = 1 and T = 5 under a halo of 9.  The layers of a code meet pick_cfg's own
                             condition for its tile (conv_ref.BUILD_LAYERS).  The first layer of a code runs every epilogue its kernel
                             dispatches — conv_gemm_kernel (0, 1, 2, 5, 6, 8) and conv_gemm_sk_kernel (9; 19 with a prologue, K padding or a
                             generic epilogue): lean 1 / 2 / 3, compact 0 (the Euler step) and FULL (tanh, SiLU, Mish); conv_sk32_kernel (19,
                             128 -> 128 k3 and 256 -> 256 k7): lean 1 / 2 / 3; conv_split_kernel (40; 41 under setting 6) and conv_h16_kernel
                             (46; 47 = forced 41 under setting 16): lean 1 / 3 on the 16 x 16 x 32 loop, SnakeBeta (lean 2) on the other.
  test_forced_classes[code]  the eight input classes on that layer
  test_generic_epilogues[code]  the lean-capable combinations again on a handle under EV_NO_LEAN=1 (compact 0 / FULL for SnakeBeta)
  test_balanced_build[code], test_balanced_classes[code-class]   56 (setting 0), 60 (setting 6), 66 (setting 16) by the engine's own choice,
                             never forced, at the smallest shapes pick_cfg sends there on 256 CUs (16 utterances, 8256 rows):
                               56  128 -> 512 k3: 64 x 64 tiles 8 x 129 = 1032 cost ceil(1032 / 256) x 4 x 1.08 = 21.6 against 24 for 64 x 128
                                   (520 tiles) and 64 x 192 (344); 1032 > 320 (not the prefetching build), 256 <= 1032 < 4096 and 1032 x 4 k-chunks
                                   >= 1024 workgroups: bal_ok.
                               60 / 66  256 -> 256: 64 x 192 wins (172 tiles: 12 against 16 and 12.96), 128 x 128 tiles 2 x 65 = 130 < 1024 (not
                                   the deep-grid build), 130 x 2 >= 256 and 130 x 4 chunks >= 512 workgroups: split_bal_ok.  k3 (halo 2: nine
                                   staging passes in conv_h16_bal_kernel) and k7 d3 (halo 18: 128 + 18 > 144, twelve).
  test_device_disagrees_with_mutants   four mutant references of conv_ref against a device output: the device must be outside the gate
                             drawn around the mutant.

Gates: conv_ref's — MARGIN = 4 x the worst error of the chain-order fp32 evaluation (conv_ref.conv_chain) over the frames of the case, relative to the frame's rms A,
floor 2^-21 of the frame's fp64 L-inf, plus c_pipe x A on the 16-bit pipes; no build has another margin.  With -s the module prints per
build and class the worst ratio error / gate over all frames of all cases (1.00 is the gate).

Measured on an MI355X: worst error / gate per build and class over all layers, epilogues and frames of the build (the larger of L-inf and
RMS; 1.00 is the gate, 0.25 an error equal to the worst frame of the chain-order fp32 evaluation, 0.00 the rounded fp64 result):
    0  randn 0.30  mixed 0.32  rows 0.25  channels 0.17  offset 0.25  zero 0.00  tiny 0.25  huge 0.23
    1  randn 0.32  mixed 0.32  rows 0.25  channels 0.17  offset 0.25  zero 0.00  tiny 0.25  huge 0.23
    2  randn 0.29  mixed 0.27  rows 0.25  channels 0.29  offset 0.25  zero 0.00  tiny 0.25  huge 0.24
    5  randn 0.31  mixed 0.27  rows 0.25  channels 0.17  offset 0.25  zero 0.00  tiny 0.25  huge 0.23
    6  randn 0.32  mixed 0.25  rows 0.25  channels 0.17  offset 0.25  zero 0.00  tiny 0.25  huge 0.23
    8  randn 0.31  mixed 0.24  rows 0.25  channels 0.17  offset 0.25  zero 0.00  tiny 0.25  huge 0.23
    9  randn 0.16  mixed 0.12  rows 0.13  channels 0.09  offset 0.12  zero 0.00  tiny 0.12  huge 0.12
   19  randn 0.16  mixed 0.12  rows 0.14  channels 0.17  offset 0.11  zero 0.00  tiny 0.13  huge 0.11
   40  randn 0.13  mixed 0.13  rows 0.14  channels 0.09  offset 0.10  zero 0.00  tiny 0.09  huge 0.10
   41  randn 0.13  mixed 0.13  rows 0.15  channels 0.08  offset 0.10  zero 0.00  tiny 0.10  huge 0.10
   46  randn 0.11  mixed 0.12  rows 0.13  channels 0.08  offset 0.07  zero 0.00  tiny 0.08  huge 0.07
   47  randn 0.11  mixed 0.17  rows 0.12  channels 0.07  offset 0.07  zero 0.00  tiny 0.10  huge 0.08
   56  randn 0.25  mixed 0.24  rows 0.25  channels 0.15  offset 0.27  zero 0.00  tiny 0.25  huge 0.24
   60  randn 0.07  mixed 0.06  rows 0.10  channels 0.08  offset 0.04  zero 0.00  tiny 0.05  huge 0.05
   66  randn 0.05  mixed 0.04  rows 0.09  channels 0.06  offset 0.04  zero 0.00  tiny 0.05  huge 0.05
Maximum 0.32 (64 x 128 and 64 x 64 tiles, randn / mixed): the exact fp32 MFMA builds sit at 1.0 to 1.3 x the chain evaluation, the split-K
builds and the 16-bit pipes (whose gate carries c_pipe x A) well inside; no build needed another margin and no case exposed a bug.  Every
pad row came back as the sentinel and every repeat gave the same bits.
Wall time on that machine: 12 s for the module's 58 tests (the largest, test_balanced_build[56], 1.3 s), in a whole GPU suite of 374 to 395 s
(1465 tests, two runs on two machines; 12 s less without it).  The gate is no measurement of speed."""
import os

import pytest
import torch

import conv_ref as R
from emojivoice_amd._lib import CONV_EPI_SENTINEL, Engine, EvLibraryError

pytestmark = pytest.mark.gpu

F64 = torch.float64
_RATIOS = {}
_ENGINES = {}
# forced code -> (EV_FORCE_CFG, arithmetic setting or None, the code last_cfg reports)
FORCE = {b: (b, None, b) for b in R.FORCED_BUILDS}
FORCE[41] = (41, 6, 41)
FORCE[47] = (41, 16, 47)
BAL_ARITH = {56: 0, 60: 6, 66: 16}


def _engine(build, no_lean=False):
    """One handle per (code, epilogue kind), created under the switches ev_create reads and kept for the module."""
    key = (build, no_lean)
    if key not in _ENGINES:
        old = {k: os.environ.get(k) for k in ("EV_FORCE_CFG", "EV_NO_LEAN")}
        try:
            os.environ.pop("EV_FORCE_CFG", None)
            os.environ.pop("EV_NO_LEAN", None)
            arith = BAL_ARITH.get(build)
            if build in FORCE:
                os.environ["EV_FORCE_CFG"] = str(FORCE[build][0])
                arith = FORCE[build][1]
            if no_lean:
                os.environ["EV_NO_LEAN"] = "1"
            e = Engine(0)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        if arith is not None:
            e.set_arithmetic(arith)
        _ENGINES[key] = e
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _handles():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()
    if _RATIOS:
        print("\nworst error / gate per build and class (1.00 is the gate):")
        for b in sorted({k[0] for k in _RATIOS}):
            print(f"  {b:3d}  " + "  ".join(f"{cls} {_RATIOS[(b, cls)]:.2f}" for cls in R.CLASSES if (b, cls) in _RATIOS))


def _launch(eng, c):
    L, E = R.LAYERS[c["layer"]], R.EPIS[c["epi"]]
    masked = bool(E.get("mask1") or E.get("mask2") or E.get("y2"))
    snake = E.get("act") == "snake"
    cu = lambda t: t.cuda()   # noqa: E731
    return eng.op_conv1d_epi(
        cu(c["x"]), c["w"], c["bias"] if E.get("bias", True) else None, dilation=L["d"], transposed=L["form"] == "T", stride=L["stride"],
        padding=L["padding"], P=L["P"], pre_lrelu_slope=E.get("pro", -1.0), act=E.get("act", "none"), act_slope=E.get("act_slope", 0.0),
        alpha_exp=cu(c["alpha_exp"]) if snake else None, beta_inv=cu(c["beta_inv"]) if snake else None,
        lengths=cu(c["lengths"]) if masked else None, mask1=bool(E.get("mask1")), mask2=bool(E.get("mask2")), scale=E.get("scale", 1.0),
        R=cu(c["R"]) if E.get("R") else None, yold=cu(c["yold"]) if E.get("accum") else None, accum=bool(E.get("accum")),
        div3=bool(E.get("div3")), act2_slope=E.get("act2", -1.0), want_y2=bool(E.get("y2")), want_padded=True)


def _run(eng, build, layer, cls, epi):
    """One case on `eng`: the build, the repeat, the pad rows, the gate.  Returns the failures.  A device fault ends the session: nothing
    more is started on a device that has faulted."""
    try:
        return _run_case(eng, build, layer, cls, epi)
    except (EvLibraryError, RuntimeError) as ex:
        if any(s in str(ex) for s in ("illegal memory", "HIP error", "sync failed", "hipError")):
            pytest.exit(f"device fault in build {build} {layer} {cls} {epi}: {ex}", returncode=3)
        raise


def _run_case(eng, build, layer, cls, epi):
    c = R.case(layer, cls, epi)
    L = R.LAYERS[layer]
    tag = f"build {build} {layer} {cls} {epi}"
    y, y2, ypad = _launch(eng, c)
    got_cfg = eng.last_cfg()
    if got_cfg != build:
        return [(tag, f"ran on build {got_cfg}")]
    ya, y2a, ypada = _launch(eng, c)
    bad = []
    if not (torch.equal(y, ya) and torch.equal(ypad, ypada) and (y2 is None or torch.equal(y2, y2a))):
        bad.append((tag, "a repeated launch gave other bits"))
    B, Cout, To = y.shape
    Po = L["P"] * L["stride"] if L["form"] == "T" else L["P"] // L["stride"]
    pv = ypad.view(B, To + 2 * Po, Cout)
    if not (bool((pv[:, :Po] == CONV_EPI_SENTINEL).all()) and bool((pv[:, Po + To:] == CONV_EPI_SENTINEL).all())):
        bad.append((tag, "a pad row of Y was written"))
    if not torch.equal(pv[:, Po:Po + To].transpose(1, 2), y):
        bad.append((tag, "the padded Y and the valid frames differ"))
    b2, worst = R.failures(y.cpu(), None if y2 is None else y2.cpu(), c, build, tag)
    k = (build, cls)
    _RATIOS[k] = max(_RATIOS.get(k, 0.0), worst)
    return bad + b2


def _check(bad):
    assert not bad, "\n".join(str(b) for b in bad)


@pytest.mark.parametrize("build", R.FORCED_BUILDS)
def test_forced_build(build):
    eng = _engine(build)
    bad = []
    for layer, cls, epi in R.plan(build):
        if cls in ("randn", "mixed"):
            bad += _run(eng, build, layer, cls, epi)
    _check(bad)


@pytest.mark.parametrize("build", R.FORCED_BUILDS)
def test_forced_classes(build):
    eng = _engine(build)
    bad = []
    for layer, cls, epi in R.plan(build):
        if cls not in ("randn", "mixed"):
            bad += _run(eng, build, layer, cls, epi)
    _check(bad)


@pytest.mark.parametrize("build", [b for b in R.FORCED_BUILDS if b in R.FP32_BUILDS])
def test_generic_epilogues(build):
    """EV_NO_LEAN=1: the lean-capable combinations on the compact (SnakeBeta: the FULL) epilogue of the same build."""
    eng = _engine(build, no_lean=True)
    layer = R.BUILD_LAYERS[build][0]
    bad = []
    for epi in R.LEAN_EPIS:
        bad += _run(eng, build, layer, "randn", epi)
    bad += _run(eng, build, layer, "mixed", "plain")
    _check(bad)


@pytest.mark.parametrize("build", R.BALANCED_BUILDS)
def test_balanced_build(build):
    eng = _engine(build)
    bad = []
    for layer, cls, epi in R.plan(build):
        if cls in ("randn", "mixed"):
            bad += _run(eng, build, layer, cls, epi)
    _check(bad)


@pytest.mark.parametrize("cls", R.CLASSES[2:])
@pytest.mark.parametrize("build", R.BALANCED_BUILDS)
def test_balanced_classes(build, cls):
    _check(_run(_engine(build), build, R.BUILD_LAYERS[build][0], cls, "plain"))


@pytest.mark.parametrize("build,mutant", [(1, "tapdrop"), (0, "prohalo"), (46, "x_fp16"), (19, "div3_early")])
def test_device_disagrees_with_mutants(build, mutant):
    """The device output is inside the gate around the fp64 reference and outside the same gate drawn around the mutant reference."""
    layer, epi = R.MUTANTS[mutant]
    c = R.case(layer, "randn", epi)
    eng = _engine(build)
    y, _, _ = _launch(eng, c)
    assert eng.last_cfg() == build
    y = y.cpu()
    y64, _, y32, _, A = R.references(c)
    ok, _ = R.gate_failures(y, y64, y32, A, build)
    assert not ok, ok
    ym, _ = R.evaluate(c, F64, mut=mutant)
    bad, worst = R.gate_failures(y, y64, y32, A, build, around=ym)
    assert bad and worst > 10.0, (mutant, worst)


def test_hook_refuses_bad_arguments():
    """Bad arguments fail the call with a message (and launch nothing): fewer pad rows than the halo, a mask without lengths, a running sum
    without Yold, SnakeBeta without its vectors, a row mask on a transposed conv, an odd P under the pair view."""
    eng = _engine(1)
    c = R.case("k7d3")
    x, lens = c["x"].cuda(), c["lengths"].cuda()
    kw = {"dilation": 3, "padding": 9}
    for more, msg in (({"P": 8}, "halo"), ({"P": 9, "mask1": True}, "d_lengths"), ({"P": 9, "accum": True}, "d_yold"),
                      ({"P": 9, "act": "snake"}, "SnakeBeta"), ({"P": 9, "act_slope": 2.0, "act": "lrelu"}, "act_slope"),
                      ({"P": 9, "scale": float("inf")}, "scale")):
        with pytest.raises(EvLibraryError, match=msg):
            eng.op_conv1d_epi(x, c["w"], c["bias"], **kw, **more)
    t = R.case("t2")
    with pytest.raises(EvLibraryError, match="transposed"):
        eng.op_conv1d_epi(t["x"].cuda(), t["w"], t["bias"], transposed=True, stride=2, padding=1, P=1, lengths=t["lengths"].cuda(), mask2=True)
    s2 = R.case("s2")
    with pytest.raises(EvLibraryError, match="even P"):
        eng.op_conv1d_epi(s2["x"].cuda(), s2["w"], s2["bias"], stride=2, padding=1, P=3)
    y, _, _ = eng.op_conv1d_epi(x, c["w"], c["bias"], P=9, lengths=lens, mask2=True, **kw)      # ... and the handle still works
    assert eng.last_cfg() == 1 and bool(torch.isfinite(y).all())
