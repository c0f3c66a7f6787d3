"""The U-Net's normalisation kernels on a real MI355X, per slab / per row against the fp64 restatements of tests/norm_ref.py.

What each case reaches (launch_gn / launch_ln / launch_mlp in ev_engine.hip):
  test_groupnorm_builds   ev_op_groupnorm_mish2 -> launch_gn, X | R in the estimator's 512-wide buffer (ldx = ldr = 512), modes 0, 1 (shared
                          temb, stride 0; one row per utterance, stride 256) and 2:
                            B = 3   groupnorm_mish_kernel<1024>, 128 frames per pass: T = 1, 127, 128, 129 and 1024 in registers, 1025 the
                                    three-pass fallback
                            B = 32  groupnorm_mish_kernel<512>, 64 frames per pass: T = 1, 63, 64, 65 and 768 in registers, 769 and 1030 the
                                    three-pass fallback
  test_apply_path         ev_op_conv_groupnorm: conv 256 -> 256 k3 of one utterance on conv_sk32_kernel (build 19) leaving per-tile
                          {count, mean, M2}, then groupnorm_apply_kernel merging them: T = 4 (1 tile), 31, 33 (2), 516 (17), 2052 and 2100
                          (65 and 66 tiles: the merge's second round of 64); under EV_NO_GN_STATS=1 no statistics and groupnorm_mish_kernel<1024>
  test_layernorm_rows     layernorm256_kernel, 101 and 16640 rows
  test_ln_fused           ev_ln256_row inside ln_mlp_kernel<1, 2> / <0, 2> (70 rows: one tile per workgroup; 9000 rows: the balanced grid),
                          ln_qkv_h16_kernel (build 122) and ln_mlp_h16_kernel (16640 rows, setting 16), ln_mlp_kernel<1, 2> on the persistent grid and
                          ln_mlp_split_kernel (16640 rows, setting 6) — through their linear outputs

Gates: norm_ref's — 4 x the worst error of the plain fp32 evaluation on the same case and class, floor 2^-21 of the fp64 L-inf, derived
in-process and never from a kernel.  With -s the module prints, per class, the worst ratio kernel error / fp32 yardstick (the gate is at 4).

Worst ratio kernel error / fp32 yardstick per class, measured on an MI355X (the larger of RMS and L-inf over all cases of the kernel; the
gate is at 4; 0.00: kernel and fp64 agree to the last bit of the fp32 output):
  groupnorm_mish_kernel<1024> regs    randn 1.19  offset 2.50  const 0.96  zero 0.96  outlier 1.40  tiny 1.46  huge 1.00  cross 1.15
  groupnorm_mish_kernel<1024> 3pass   randn 1.26  offset 1.41  const 0.66  zero 0.66  outlier 0.44  tiny 1.27  huge 0.92  cross 0.95
  groupnorm_mish_kernel<512> regs     randn 1.19  offset 1.38  const 0.96  zero 0.96  outlier 1.35  tiny 1.37  huge 1.21  cross 1.36
  groupnorm_mish_kernel<512> 3pass    randn 1.08  offset 1.79  const 0.80  zero 0.80  outlier 2.08  tiny 1.46  huge 1.19  cross 1.00
  conv_sk32_kernel tile statistics    mean 0.16  M2 1.18
  groupnorm_apply_kernel              1.58 (one round of the merge)  1.53 (two rounds)      groupnorm_mish_kernel<1024> after the conv 1.64
  layernorm256_kernel                 randn 1.36  offset 0.64  const 0.00  zero 0.00  outlier 1.22  tiny 0.43  huge 1.11
  ln_mlp_kernel<1,2>                  randn 1.92  offset 1.07  const 1.58  zero 1.58  outlier 1.39  tiny 0.90  huge 1.26
  ln_mlp_kernel<1,2> persistent grid  randn 1.65  offset 0.66  const 1.41  zero 1.41  outlier 1.51  tiny 1.67  huge 1.91
  ln_qkv_h16_kernel                   randn 1.01  offset 0.66  const 1.05  zero 1.05  outlier 0.98  tiny 1.20  huge 0.91
  ln_mlp_kernel<0,2>                  randn 2.80  offset 1.11  const 0.37  zero 2.93  outlier 0.38  tiny 2.73  huge 0.38
  ln_mlp_kernel<0,2> balanced         randn 2.34  offset 0.66  const 0.34  zero 2.77  outlier 0.41  tiny 1.84  huge 0.44
  ln_mlp_h16_kernel                   randn 2.27  offset 0.67  const 0.35  zero 1.47  outlier 0.41  tiny 2.21  huge 0.48
  ln_mlp_split_kernel                 randn 3.23  offset 0.67  const 0.40  zero 2.91  outlier 0.41  tiny 2.73  huge 0.48
Maximum 3.23 (ln_mlp_split_kernel, randn rows): the feed-forward rows whose LayerNorm output is O(1) carry ev_sin2's absolute error
(2e-7 per hidden unit, ev_kernels.h) on top of the fp32 sums; no kernel needed a wider gate and no case exposed a bug."""
import pytest
import torch
import torch.nn.functional as F

import norm_ref as N
from emojivoice_amd._lib import Engine

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
_RATIOS = {}


def _note(kernel, ratios):
    for (cls, kind), r in ratios.items():
        k = (kernel, cls)
        _RATIOS[k] = max(_RATIOS.get(k, 0.0), r)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0, spk_emb_dim=64)
    yield e
    e.close()
    for kernel in sorted({k[0] for k in _RATIOS}):
        print(f"\nNORMRATIO {kernel}: " + "  ".join(f"{c} {r:.2f}" for (kk, c), r in sorted(_RATIOS.items()) if kk == kernel))
    if _RATIOS:
        print(f"NORMRATIO max {max(_RATIOS.values()):.2f}")


# ---------------------------------------------------------------------------------------------------------------------
# groupnorm_mish_kernel<1024> and <512>: pass widths, the register / three-pass boundary, every epilogue
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", N.GN_SHAPES)
def test_groupnorm_builds(eng, B, T):
    c = N.gn_case(B, T)
    x, ga, be, L = c["x"].cuda(), c["gamma"].cuda(), c["beta"].cuda(), c["lengths"].cuda()
    build = 1024 if B < 32 else 512
    path = "regs" if T <= (1024 if B < 32 else 768) else "3pass"
    bad = []
    for v in N.GN_VARIANTS:
        mode, temb, R = N.gn_args(c, v)
        got = eng.op_groupnorm_mish2(x, ga, be, L, mode, None if temb is None else temb.cuda(), None if R is None else R.cuda())
        again = eng.op_groupnorm_mish2(x, ga, be, L, mode, None if temb is None else temb.cuda(), None if R is None else R.cuda())
        if not torch.equal(got, again):
            bad.append((v, "a second call gives other bits"))
        f, ratios = N.gn_failures(got.cpu(), c, v, tag=f"{B}x{T} {v}")
        print(f"NORMERR groupnorm_mish_kernel<{build}> {path} {B}x{T} {v}: " + " ".join(f"{k[0]}/{k[1]} {r:.2f}" for k, r in sorted(ratios.items())))
        bad += f
        _note(f"groupnorm_mish_kernel<{build}> {path}", ratios)
    if B == 3 and T == 129:
        # the old entry point is the same launch in the 256-wide layout
        assert torch.equal(eng.op_groupnorm_mish(x, ga, be, L), eng.op_groupnorm_mish2(x, ga, be, L, 0))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# conv_sk32_kernel's per-tile statistics and groupnorm_apply_kernel's merge
# ---------------------------------------------------------------------------------------------------------------------
def _apply_check(e, T, want_stats, bad):
    c = N.apply_case(T)
    x, ga, be = c["x"].cuda(), c["gamma"].cuda(), c["beta"].cuda()
    length = int(c["lengths"][0])
    ref_conv = F.conv1d(c["x"].double(), c["w"].double(), c["bias"].double(), padding=1)
    for mode, temb, R in ((0, None, None), (1, c["temb_shared"], None), (2, None, c["R"])):
        conv, part, y, tiles = e.op_conv_groupnorm(x, c["w"], c["bias"], ga, be, length, mode, None if temb is None else temb.cuda(),
                                                   None if R is None else R.cuda())
        tag = f"T {T} mode {mode} tiles {tiles}"
        conv, part, y = conv.cpu(), part.cpu(), y.cpu()
        nt = (T + 4 + 31) // 32
        if want_stats:
            assert tiles == nt and tiles > (64 if T >= 2052 else 0), f"{tag}: the conv was expected to leave statistics of {nt} tiles (build {e.last_cfg()})"
        else:
            assert tiles == 0, tag
        # the hook's conv is the conv (staging, bias, 'same' padding)
        cerr = float((conv.double() - ref_conv).abs().max())
        if not cerr <= 3e-5 * float(ref_conv.abs().max()):
            bad.append((tag, f"conv output off by {cerr:.3e}"))
        c64 = conv.double()
        if tiles:
            # the triples, against the fp64 statistics of the device's own conv output; yardstick: the same two passes in fp32
            st64, st32, sc = N.tile_stats(c64[0]), N.tile_stats(conv[0]).double(), N.tile_scales(c64[0])
            got = part[:nt].double()
            if not torch.equal(got[..., 0], st64[..., 0]):
                bad.append((tag, "tile counts differ"))
            live = st64[..., 0] > 0
            for name, i, scale, floor in (("mean", 1, sc[..., 0], N.FLOOR * sc[..., 1]), ("M2", 2, st64[..., 2], N.FLOOR * st64[..., 2])):
                yard = float(((st32[..., i] - st64[..., i]).abs() / scale)[live].max())
                err = (got[..., i] - st64[..., i]).abs()
                gate = torch.maximum(N.MARGIN * yard * scale, floor)
                r = float((err / torch.maximum(yard * scale, floor / N.MARGIN))[live].max())
                _note("conv_sk32_kernel tile statistics", {(name, "linf"): r})
                print(f"NORMERR {tag} tile {name}: ratio {r:.2f} (fp32 yardstick {yard:.3e})")
                if not bool((err <= gate)[live].all()):
                    bad.append((tag, f"tile {name}: worst error / yardstick {r:.2f}"))
        # the norm, against the restatement on the device's own conv output
        cv = lambda t, dt: None if t is None else t.to(dt)   # noqa: E731
        ref64 = N.groupnorm_mish(c64, c["gamma"].double(), c["beta"].double(), c["lengths"], mode, cv(temb, F64), cv(R, F64))
        y32 = N.groupnorm_mish(conv, c["gamma"], c["beta"], c["lengths"], mode, temb, R)
        f, ratios = N.gate_failures(N.gn_slab_errors(y, ref64, c["lengths"]), N.gn_slab_errors(y32, ref64, c["lengths"]), c["cls"], ("mix",), tag=tag)
        bad += f + N.gn_masked_failures(y, c["lengths"], R, tag)
        kern = "groupnorm_apply_kernel" + (" 2 rounds" if tiles > 64 else "") if tiles else "groupnorm_mish_kernel<1024> after conv"
        print(f"NORMERR {tag} {kern}: " + " ".join(f"{k[1]} {r:.2f}" for k, r in sorted(ratios.items())))
        _note(kern, ratios)
        conv2, part2, y2, _ = e.op_conv_groupnorm(x, c["w"], c["bias"], ga, be, length, mode, None if temb is None else temb.cuda(),
                                                  None if R is None else R.cuda())
        if not (torch.equal(y2.cpu(), y) and torch.equal(part2.cpu()[:nt], part[:nt])):
            bad.append((tag, "a second call gives other bits"))


@pytest.mark.parametrize("T", N.APPLY_T)
def test_apply_path(eng, T):
    bad = []
    _apply_check(eng, T, True, bad)
    assert eng.last_cfg() == 19
    assert not bad, bad


def test_apply_path_switched_off(eng, monkeypatch):
    """EV_NO_GN_STATS=1: the conv leaves no statistics, groupnorm_mish_kernel computes them — same gate."""
    monkeypatch.setenv("EV_NO_GN_STATS", "1")
    e = Engine(0)
    bad = []
    try:
        for T in N.APPLY_T:
            _apply_check(e, T, False, bad)
    finally:
        e.close()
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm: the stand-alone kernel and ev_ln256_row inside the fused kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", N.LN_ROWS)
def test_layernorm_rows(eng, rows):
    c = N.ln_case(rows)
    got = eng.op_layernorm(c["x"].cuda(), c["gamma"].cuda(), c["beta"].cuda()).cpu()
    ref = N.ln_eval(c, "ln", None, F64)
    bad, ratios = N.gate_failures(N.row_errors(got, ref), N.row_errors(N.ln_eval(c, "ln", None, F32), ref), c["cls"], N.LN_CLASSES, tag=f"{rows} rows")
    print(f"NORMERR layernorm256_kernel {rows}: " + " ".join(f"{k[0]}/{k[1]} {r:.2f}" for k, r in sorted(ratios.items())))
    _note("layernorm256_kernel", ratios)
    assert not bad, bad


@pytest.mark.parametrize("rows,setting,proj_kernel,ff_kernel", [
    (70, None, "ln_mlp_kernel<1,2>", "ln_mlp_kernel<0,2>"),
    (9000, None, "ln_mlp_kernel<1,2> persistent grid", "ln_mlp_kernel<0,2> balanced"),
    (16640, 16, "ln_qkv_h16_kernel", "ln_mlp_h16_kernel"),
    (16640, 6, "ln_mlp_kernel<1,2> persistent grid", "ln_mlp_split_kernel"),
])
def test_ln_fused(eng, rows, setting, proj_kernel, ff_kernel):
    c = N.ln_case(rows)
    x, ga, be = c["x"].cuda(), c["gamma"].cuda(), c["beta"].cuda()
    wq, wf = N.mlp_weights(384, 1), N.mlp_weights(1024, 2)
    mask = N.ln_rowmask(rows)
    keep = mask > 0
    orig = eng.arithmetic()
    bad = []
    try:
        if setting is not None:
            eng.set_arithmetic(setting)
        got = eng.op_ln_mlp(x, ga, be, wq["w1"], None).cpu()       # (the projection's units are whole tiles: no hand-offs, no epoch to read)
        if setting == 16:
            assert eng.last_cfg() == 122
        ref = N.ln_eval(c, "proj", wq, F64)
        f, ratios = N.gate_failures(N.row_errors(got, ref), N.row_errors(N.ln_eval(c, "proj", wq, F32), ref), c["cls"], N.LN_CLASSES,
                                    tag=f"{rows} rows {proj_kernel}")
        print(f"NORMERR {proj_kernel} {rows}: " + " ".join(f"{k[0]}/{k[1]} {r:.2f}" for k, r in sorted(ratios.items())))
        _note(proj_kernel, ratios)
        bad += f
        s0 = eng.sk_stats()[0]
        got = eng.op_ln_mlp(x, ga, be, wf["w1"], wf["b1"], wf["alpha"], wf["beta"], wf["w2"], wf["b2"], mask.cuda()).cpu()
        if rows >= 9000:
            assert eng.sk_stats()[0] > s0, "this shape was expected to take a balanced grid"
        ref = N.ln_eval(c, "ff", wf, F64)
        f, ratios = N.gate_failures(N.row_errors(got, ref), N.row_errors(N.ln_eval(c, "ff", wf, F32), ref), c["cls"], N.LN_CLASSES, keep=keep,
                                    tag=f"{rows} rows {ff_kernel}")
        print(f"NORMERR {ff_kernel} {rows}: " + " ".join(f"{k[0]}/{k[1]} {r:.2f}" for k, r in sorted(ratios.items())))
        _note(ff_kernel, ratios)
        bad += f
        if float(got[~keep].abs().max()) != 0.0:
            bad.append((ff_kernel, "masked rows are not exactly 0"))
    finally:
        eng.set_arithmetic(orig)
    assert not bad, bad
