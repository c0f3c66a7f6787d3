"""tests/norm_ref.py on the CPU: the fp64 restatements against torch's own GroupNorm / Mish / LayerNorm, the conditions the GPU module
(tests/test_gpu_norms.py) relies on, and the gates' power: every mutant of the restatement — each one a plausible kernel bug — is
rejected by the same gate the kernels are held to."""
import pytest
import torch
import torch.nn.functional as F

import norm_ref as N

F64, F32 = torch.float64, torch.float32


# ---------------------------------------------------------------------------------------------------------------------
# the restatements
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(3, 129), (2, 1), (5, 40)])
def test_groupnorm_mish_matches_torch(B, T):
    c = N.gn_case(B, T)
    x, ga, be = c["x"].double(), c["gamma"].double(), c["beta"].double()
    m = N.frame_mask(c["lengths"], T, F64)
    base = F.mish(F.group_norm(x, 8, ga, be, eps=1e-5)) * m
    scale = float(base.abs().max())
    assert float((N.gn_eval(c, "m0", F64) - base).abs().max()) <= 1e-12 * scale
    assert float((N.gn_eval(c, "m1s", F64) - (base + c["temb_shared"].double()[:, :, None]) * m).abs().max()) <= 1e-12 * scale
    assert float((N.gn_eval(c, "m1r", F64) - (base + c["temb_rows"].double()[:, :, None]) * m).abs().max()) <= 1e-12 * scale
    assert float((N.gn_eval(c, "m2", F64) - (base + c["R"].double())).abs().max()) <= 1e-12 * scale
    # the mask as the kernel comment states it: a padded frame is 0 in modes 0 and 1 (not temb), R in mode 2
    for v in N.GN_VARIANTS:
        assert not N.gn_masked_failures(N.gn_eval(c, v, F64), c["lengths"], c["R"].double() if v == "m2" else None)


def test_layernorm_matches_torch():
    c = N.ln_case(101)
    x, ga, be = c["x"].double(), c["gamma"].double(), c["beta"].double()
    ref = F.layer_norm(x, (256,), ga, be, eps=1e-5)
    assert float((N.layernorm(x, ga, be) - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


@pytest.mark.parametrize("T", [4, 33, 517, 2100])
def test_chan_merge_of_unequal_tiles_is_the_direct_statistics(T):
    """Tiles of 30, 32, ..., 32 and a short last one (the padded utterance's) with widely different means, merged in fp64"""
    y = N.apply_case(T)["x"][0].double() * 0.01 + torch.randn(256, T, generator=torch.Generator().manual_seed(T)).double()
    part = N.tile_stats(y)
    assert int(part[:, 0, 0].sum()) == 32 * T and len({int(v) for v in part[:, 0, 0]}) > (1 if T > 30 else 0)
    n, mean, m2 = N.chan_merge(part)
    v = y.reshape(8, -1)
    dm = v.mean(dim=1)
    dq = ((v - dm[:, None]) ** 2).sum(dim=1)
    assert torch.equal(n, torch.full((8,), 32.0 * T, dtype=F64))
    assert float(((mean - dm).abs() / v.abs().amax(dim=1)).max()) <= 1e-12
    assert float(((m2 - dq).abs() / dq).max()) <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# conditions of the GPU module's cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", N.GN_SHAPES)
def test_groupnorm_cases_have_output_rms(B, T):
    c = N.gn_case(B, T)
    assert int(c["lengths"].max()) == T and (B == 1 or int(c["lengths"].min()) == 1)
    assert len({tuple(r.tolist()) for r in c["temb_rows"]}) == B
    assert set(c["cls"].flatten().tolist()) == set(range(8))
    for v in N.GN_VARIANTS:
        e = N.gn_slab_errors(torch.zeros(B, 256, T), N.gn_eval(c, v, F64), c["lengths"])
        assert float(e[2].min()) >= N.RMS_FLOOR, (v, float(e[2].min()))


@pytest.mark.parametrize("T", N.APPLY_T)
def test_apply_cases_have_output_rms(T):
    c = N.apply_case(T)
    conv = F.conv1d(c["x"].double(), c["w"].double(), c["bias"].double(), padding=1)
    for mode, temb, R in ((0, None, None), (1, c["temb_shared"].double(), None), (2, None, c["R"].double())):
        ref = N.groupnorm_mish(conv, c["gamma"].double(), c["beta"].double(), c["lengths"], mode, temb, R)
        assert float(N.gn_slab_errors(torch.zeros_like(ref), ref, c["lengths"])[2].min()) >= N.RMS_FLOOR


def test_layernorm_cases_have_output_rms():
    for rows in sorted(set(N.LN_ROWS + N.MLP_ROWS)):
        c = N.ln_case(rows)
        assert set(c["cls"][:32].tolist()) == set(range(7)) and set(c["cls"][-32:].tolist()) == set(range(7)) or rows < 64
        assert float(N.row_errors(torch.zeros(rows, 256), N.ln_eval(c, "ln", None, F64))[2].min()) >= N.RMS_FLOOR
        if rows in N.MLP_ROWS:
            assert float(N.row_errors(torch.zeros(rows, 384), N.ln_eval(c, "proj", N.mlp_weights(384, 1), F64))[2].min()) >= N.RMS_FLOOR
            keep = N.ln_rowmask(rows) > 0
            ff = N.ln_eval(c, "ff", N.mlp_weights(1024, 2), F64)
            assert float(N.row_errors(torch.zeros(rows, 256), ff)[2][keep].min()) >= N.RMS_FLOOR
            assert float(ff[~keep].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the gates reject mutants
# ---------------------------------------------------------------------------------------------------------------------
MUTANTS = {                       # name: (variant it is run in, what it does)
    "divisor n - 1": "m0", "eps 1e-6": "m0", "statistics over the valid frames only": "m0", "one-pass E[x^2] - mean^2 in fp32": "m0",
    "last frame left out of the statistics": "m0", "last frame left out of the apply": "m0", "no softplus threshold, naive exp": "m0",
    "temb of row b - 1": "m1r", "temb added without the second mask": "m1s", "R read with ldr = 256": "m2",
}


def _gn_mutant(c, variant, kind):
    """The restatement with one thing wrong, evaluated in fp64 (in fp32 where the mutation is one of fp32 arithmetic), rounded to fp32."""
    dt = F32 if kind in ("one-pass E[x^2] - mean^2 in fp32", "no softplus threshold, naive exp") else F64
    x, ga, be = c["x"].to(dt), c["gamma"].to(dt), c["beta"].to(dt)
    B, _, T = x.shape
    L = c["lengths"]
    mode, temb, R = N.gn_args(c, variant)
    m = N.frame_mask(L, T, dt)
    xg = x.reshape(B, 8, 32, T)
    w = torch.ones(B, 1, 1, T, dtype=dt)              # frames the statistics count
    if kind == "statistics over the valid frames only":
        w = m[:, :, None, :]
    if kind == "last frame left out of the statistics":
        w = w.clone()
        w[..., T - 1] = 0
    n = (w.sum(dim=(2, 3), keepdim=True) * 32).clamp(min=1)
    mean = (xg * w).sum(dim=(2, 3), keepdim=True) / n
    if kind == "one-pass E[x^2] - mean^2 in fp32":
        var = (xg * xg * w).sum(dim=(2, 3), keepdim=True) / n - mean * mean
    else:
        var = ((xg - mean) ** 2 * w).sum(dim=(2, 3), keepdim=True) / (n - 1 if kind == "divisor n - 1" else n)
    eps = 1e-6 if kind == "eps 1e-6" else 1e-5
    y = ((xg - mean) / torch.sqrt(var + eps)).reshape(B, 256, T) * ga[None, :, None] + be[None, :, None]
    if kind == "no softplus threshold, naive exp":      # ev_mish's closed form x * n / (n + 2), n = e^x (e^x + 2), without its clamp and branch
        e = torch.exp(y)
        q = e * (e + 2)
        y = y * (q / (q + 2))
    else:
        y = N.mish(y)
    y = y * m
    if mode == 1:
        t = temb.to(dt).reshape(-1, 256)
        if kind == "temb of row b - 1":
            t = torch.roll(t, 1, dims=0)
        y = y + t[:, :, None]
        if kind != "temb added without the second mask":
            y = y * m
    if mode == 2:
        Rm = R.to(dt)
        if kind == "R read with ldr = 256":            # the 512-wide [X | R] buffer of the estimator, rows b * (T + 4) + 2 + t, read at R + n * 256
            S = T + 4
            AR = torch.zeros(B * S + 1, 512, dtype=dt)
            rows = (torch.arange(B)[:, None] * S + 2 + torch.arange(T)[None, :]).flatten()
            AR[rows, :256] = x.transpose(1, 2).reshape(-1, 256)
            AR[rows, 256:] = Rm.transpose(1, 2).reshape(-1, 256)
            flat = AR.flatten()
            Rm = flat[(256 + rows[:, None] * 256 + torch.arange(256)[None, :])].reshape(B, T, 256).transpose(1, 2)
        y = y + Rm
    if kind == "last frame left out of the apply":
        y = y.clone()
        y[:, :, T - 1] = 0
    return y.to(F32)


@pytest.fixture(scope="module")
def mutant_case():
    c = N.gn_case(3, 129)
    refs = {v: (N.gn_eval(c, v, F64), N.gn_eval(c, v, F32)) for v in N.GN_VARIANTS}
    return c, refs


def test_the_fp32_evaluation_passes_its_own_gate(mutant_case):
    c, refs = mutant_case
    for v in N.GN_VARIANTS:
        bad, ratios = N.gn_failures(refs[v][1], c, v, *refs[v])
        assert not bad and max(ratios.values()) <= 1.0 + 1e-12, (bad, ratios)


@pytest.mark.parametrize("kind", list(MUTANTS))
def test_gate_rejects_mutant(mutant_case, kind):
    c, refs = mutant_case
    v = MUTANTS[kind]
    bad, _ = N.gn_failures(_gn_mutant(c, v, kind), c, v, *refs[v])
    print(f"NORMMUTANT {kind}: {bad[:3]}")
    assert bad, f"the gate lets the mutant '{kind}' pass"


def test_unmutated_restatement_passes(mutant_case):
    """_gn_mutant with no mutation is the restatement: what rejects the mutants is the mutation, not the helper."""
    c, refs = mutant_case
    for v in N.GN_VARIANTS:
        bad, _ = N.gn_failures(_gn_mutant(c, v, "none"), c, v, *refs[v])
        assert not bad, bad


@pytest.mark.parametrize("kind", ["divisor n - 1", "eps 1e-6", "one-pass in fp32", "last channel left out"])
def test_layernorm_gate_rejects_mutant(kind):
    c = N.ln_case(101)
    ref, y32 = N.ln_eval(c, "ln", None, F64), N.ln_eval(c, "ln", None, F32)
    dt = F32 if kind == "one-pass in fp32" else F64
    x, ga, be = c["x"].to(dt), c["gamma"].to(dt), c["beta"].to(dt)
    xs = x[:, :255] if kind == "last channel left out" else x
    mean = xs.mean(dim=1, keepdim=True)
    if kind == "one-pass in fp32":
        var = (x * x).mean(dim=1, keepdim=True) - mean * mean
    else:
        var = ((xs - mean) ** 2).sum(dim=1, keepdim=True) / (xs.shape[1] - (1 if kind == "divisor n - 1" else 0))
    y = ((x - mean) / torch.sqrt(var + (1e-6 if kind == "eps 1e-6" else 1e-5)) * ga + be).to(F32)
    bad, _ = N.gate_failures(N.row_errors(y, ref), N.row_errors(y32, ref), c["cls"], N.LN_CLASSES)
    assert bad, f"the gate lets the mutant '{kind}' pass"
    assert not N.gate_failures(N.row_errors(y32, ref), N.row_errors(y32, ref), c["cls"], N.LN_CLASSES)[0]
