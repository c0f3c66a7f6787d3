"""Yardsticks, inputs and checks of the monotonic-alignment tests (tests/test_mas_host.py, tests/test_gpu_mas.py).

``maximum_path`` restates the reference's search (monotonic_align/core.pyx) in numpy float32 from its description: the forward
DP ``value[x, y] += max(x == y ? -1e9 : value[x, y-1], x == 0 ? (y == 0 ? 0 : -1e9) : value[x-1, y-1])`` over the band
``max(0, t_x + y - t_y) <= x < min(t_x, y + 1)`` and the backtrack from ``t_x - 1`` that steps down where
``index == y or value[index, y-1] < value[index-1, y-1]`` (strict).  One float32 max and one float32 add per cell: any IEEE machine
gives the same bits, which is why the device search is held to it exactly.  tests/golden/mas_vectors.npz pins it to the reference's
compiled code.

``log_prior`` is the score matrix of matcha_tts.py:186-196: in float64 the direct form (the yardstick), in float32 the reference's
expanded form with its two matmuls ("the reference's own arithmetic", whose distance from the yardstick sets the gate).
``losses`` evaluates the three losses of matcha_tts.py:201-246 in float64 FOR A GIVEN attn.
"""
import itertools
import math

import numpy as np
import torch

NEG = np.float32(-1e9)
SIGMA_MIN = 1e-4
SHAPES = [(1, 1, 1), (1, 1, 37), (3, 17, 17), (3, 50, 129), (64, 120, 516), (1, 400, 1032), (2, 1100, 1200)]


# ---------------------------------------------------------------------------------------------------------------------
# the search
# ---------------------------------------------------------------------------------------------------------------------
def maximum_path_each(value, t_x, t_y):
    """value (Tx, Ty) float32, modified in place like the reference's; returns path (Tx, Ty) int8."""
    assert value.dtype == np.float32
    path = np.zeros(value.shape, np.int8)
    for y in range(t_y):
        lo, hi = max(0, t_x + y - t_y), min(t_x, y + 1)
        if hi <= lo:
            continue
        if y == 0:
            v_cur = np.full(hi - lo, NEG, np.float32)                    # x == y == 0
            v_prev = np.zeros(hi - lo, np.float32)
        else:
            xs = np.arange(lo, hi)
            v_cur = np.where(xs == y, NEG, value[np.minimum(xs, value.shape[0] - 1), y - 1]).astype(np.float32)
            v_prev = np.where(xs == 0, NEG, value[np.maximum(xs - 1, 0), y - 1]).astype(np.float32)
        value[lo:hi, y] = np.maximum(v_cur, v_prev) + value[lo:hi, y]
    index = t_x - 1
    for y in range(t_y - 1, -1, -1):
        path[index, y] = 1
        if index != 0 and (index == y or value[index, y - 1] < value[index - 1, y - 1]):
            index -= 1
    return path


def maximum_path(value, x_lengths, y_lengths):
    """(path (B, Tx, Ty) int8, final value (B, Tx, Ty) float32) for scores (B, Tx, Ty) and per-row lengths (1 <= t_x <= t_y)."""
    value = np.array(torch.as_tensor(value).detach().cpu().numpy(), dtype=np.float32, copy=True)
    paths = np.zeros(value.shape, np.int8)
    for b in range(value.shape[0]):
        tx, ty = int(x_lengths[b]), int(y_lengths[b])
        assert 1 <= tx <= ty <= value.shape[2] and tx <= value.shape[1], (tx, ty, value.shape)
        paths[b] = maximum_path_each(value[b], tx, ty)
    return paths, value


def masked_value(log_prior, x_lengths, y_lengths):
    """What the reference's wrapper hands to its compiled loop: log_prior * mask as float32."""
    v = np.array(log_prior, np.float32, copy=True)
    B, Tx, Ty = v.shape
    xl, yl = np.asarray(x_lengths).reshape(B, 1, 1), np.asarray(y_lengths).reshape(B, 1, 1)
    mask = ((np.arange(Tx)[None, :, None] < xl) & (np.arange(Ty)[None, None, :] < yl)).astype(np.float32)
    return v * mask                                                     # a product, as the reference's: a masked negative score is -0.0


def monotonic_paths(t_x, t_y):
    """Every monotonic surjective path of t_y frames onto t_x tokens, as the tuple of token durations (each >= 1, sum t_y)."""
    for cuts in itertools.combinations(range(1, t_y), t_x - 1):
        edges = (0,) + cuts + (t_y,)
        yield tuple(edges[i + 1] - edges[i] for i in range(t_x))


def path_score(value, durs):
    """Score of one path on raw scores, in float64."""
    s, y = 0.0, 0
    for i, d in enumerate(durs):
        s += float(np.sum(value[i, y:y + d].astype(np.float64)))
        y += d
    return s


def check_structure(attn, x_lengths, y_lengths, dur=None):
    """Every frame below y_length has exactly one token, the token never decreases and never skips, starts at 0 and ends at
    t_x - 1; nothing is set beyond the lengths; durations are the row sums, all >= 1 below t_x and sum to t_y."""
    a = torch.as_tensor(attn).detach().cpu()
    assert bool(((a == 0) | (a == 1)).all())
    for b in range(a.shape[0]):
        tx, ty = int(x_lengths[b]), int(y_lengths[b])
        assert float(a[b, tx:].abs().sum()) == 0 and float(a[b, :, ty:].abs().sum()) == 0, b
        assert bool((a[b, :, :ty].sum(0) == 1).all()), b
        tok = a[b, :, :ty].argmax(0)
        step = tok[1:] - tok[:-1]
        assert int(tok[0]) == 0 and int(tok[-1]) == tx - 1 and bool(((step == 0) | (step == 1)).all()), b
        d = a[b].sum(-1)
        assert bool((d[:tx] >= 1).all()) and int(d.sum()) == ty, b
        if dur is not None:
            assert torch.equal(torch.as_tensor(dur).detach().cpu()[b].long(), d.long()), b


# ---------------------------------------------------------------------------------------------------------------------
# scores and losses
# ---------------------------------------------------------------------------------------------------------------------
def log_prior(mu_x, y, dtype=torch.float64):
    """(B, Tx, Ty).  float64: -0.5 ||y_j - mu_i||^2 - 0.5 C log(2 pi), the true quantity.  Any other dtype: the reference's
    expanded form, op for op (matcha_tts.py:191-196), on the CPU in that dtype."""
    mu_x, y = torch.as_tensor(mu_x).detach().cpu().to(dtype), torch.as_tensor(y).detach().cpu().to(dtype)
    const = -0.5 * math.log(2 * math.pi) * mu_x.shape[1]
    if dtype == torch.float64:
        d = y.unsqueeze(2) - mu_x.unsqueeze(3)                                  # (B, C, Tx, Ty)
        return -0.5 * d.pow(2).sum(1) + const
    factor = -0.5 * torch.ones(mu_x.shape, dtype=mu_x.dtype)
    y_square = torch.matmul(factor.transpose(1, 2), y**2)
    y_mu_double = torch.matmul(2.0 * (factor * mu_x).transpose(1, 2), y)
    mu_square = torch.sum(factor * (mu_x**2), 1).unsqueeze(-1)
    return y_square - y_mu_double + mu_square + const


def log_prior_fp64_chunked(mu_x, y, rows=64):
    """The float64 yardstick for large shapes, a block of token rows at a time (same values, less memory)."""
    mu_x = torch.as_tensor(mu_x).detach().cpu()
    return torch.cat([log_prior(mu_x[:, :, i:i + rows], y) for i in range(0, mu_x.shape[2], rows)], dim=1)


def duration_loss(logw, logw_, lengths):
    return float(torch.sum((logw.double() - logw_.double()) ** 2) / torch.sum(lengths).double())


def dur_and_prior_loss(attn, logw, mu_x, y, x_lengths, y_lengths):
    """(dur_loss, prior_loss, mu_y) in float64 for a given attn (B, Tx, Ty): matcha_tts.py:203-204, :234-235, :241-242."""
    attn, logw, mu_x, y = (torch.as_tensor(a).detach().cpu().double() for a in (attn, logw, mu_x, y))
    B, Tx, Ty = attn.shape
    x_mask = (torch.arange(Tx)[None, :] < x_lengths.cpu()[:, None]).double().unsqueeze(1)
    y_mask = (torch.arange(Ty)[None, :] < y_lengths.cpu()[:, None]).double().unsqueeze(1)
    logw_ = torch.log(1e-8 + attn.sum(-1)).unsqueeze(1) * x_mask
    dur = duration_loss(logw.reshape(B, 1, Tx), logw_, x_lengths.cpu())
    mu_y = torch.matmul(attn.transpose(1, 2), mu_x.transpose(1, 2)).transpose(1, 2)
    prior = torch.sum(0.5 * ((y - mu_y) ** 2 + math.log(2 * math.pi)) * y_mask) / (torch.sum(y_mask) * y.shape[1])
    return dur, float(prior), mu_y


def cfm_inputs(y, t, z):
    """(y_t, u) of compute_loss (flow_matching.py:112-113) in the dtype of y."""
    tb = t.reshape(-1, 1, 1).to(y.dtype)
    return (1 - (1 - SIGMA_MIN) * tb) * z + tb * y, y - (1 - SIGMA_MIN) * z


def diff_loss_from_velocity(v, u, y_lengths):
    """sum (v - u)^2 / (sum(mask) * n_feats), float64 (flow_matching.py:115-117; the sum runs over the padded frames too, as the
    reference's does: the estimator is 0 there and u is not)."""
    v, u = v.detach().cpu().double(), u.detach().cpu().double()
    return float(torch.sum((v - u) ** 2) / (float(y_lengths.sum()) * u.shape[1]))


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def ragged_lengths(B, Tx, Ty, seed):
    """Row 0 full; the others random with 1 <= t_x <= t_y; one row with t_x == t_y where there are three or more."""
    g = torch.Generator().manual_seed(seed)
    xl = torch.randint(1, Tx + 1, (B,), generator=g)
    xl[0] = Tx
    yl = torch.stack([torch.randint(int(x), Ty + 1, (1,), generator=g)[0] for x in xl])
    yl[0] = Ty
    if B >= 3:
        yl[2] = xl[2]
    return xl.long(), yl.long()


def random_scores(B, Tx, Ty, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, Tx, Ty, generator=g) * scale


def mel_pairs(kind, B, Tx, Ty, seed, mu_x=None, x_lengths=None, y_lengths=None, C=80):
    """(mu_x (B, C, Tx), y (B, C, Ty), x_lengths, y_lengths).  ``aligned``: y is mu_x expanded by random integer durations plus
    0.5 N(0, 1); ``noise``: y ~ N(0, 1) (near-degenerate alignment, close ties).  mu_x ~ 1.5 N(0, 1) unless given."""
    g = torch.Generator().manual_seed(seed)
    if x_lengths is None:
        x_lengths, y_lengths = ragged_lengths(B, Tx, Ty, seed + 1)
    if mu_x is None:
        mu_x = torch.randn(B, C, Tx, generator=g) * 1.5
    mu_x = torch.as_tensor(mu_x).detach().cpu().float()
    y = torch.randn(B, mu_x.shape[1], Ty, generator=g)
    if kind == "aligned":
        y = y * 0.5
        for b in range(B):
            tx, ty = int(x_lengths[b]), int(y_lengths[b])
            cuts = torch.sort(torch.randperm(ty - 1, generator=g)[: tx - 1] + 1).values.tolist() if tx > 1 else []
            edges = [0] + cuts + [ty]
            tok = torch.repeat_interleave(torch.arange(tx), torch.tensor([edges[i + 1] - edges[i] for i in range(tx)]))
            y[b, :, :ty] += mu_x[b][:, tok]
    else:
        assert kind == "noise", kind
    return mu_x, y, x_lengths, y_lengths


# ---------------------------------------------------------------------------------------------------------------------
# MatchaTTS.forward cases (synthetic checkpoint, 178 symbols, 109 speakers)
# ---------------------------------------------------------------------------------------------------------------------
FORWARD_CASES = {"B3 ragged": (3, 21, 62, 31), "B16": (16, 24, 64, 32)}          # B, Tx, Ty, seed


def forward_texts(B, Tx, Ty, seed, n_vocab=178, n_spks=109):
    """(ids (B, Tx), x_lengths, speaker ids, y_lengths, t (B,), z (B, 80, Ty)): row 0 full, one row with t_x == t_y in the ragged case."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, n_vocab, (B, Tx), generator=g)
    spks = torch.randint(0, n_spks, (B,), generator=g)
    xl, yl = ragged_lengths(B, Tx, Ty, seed + 1)
    t = torch.rand(B, generator=g)
    z = torch.randn(B, 80, Ty, generator=g)
    return ids, xl, spks, yl, t, z


def velocity_padded(velocity, sd, y_t, mu_y, y_lengths, spk, t, dtype):
    """The estimator of compute_loss row by row (one scalar t per call, as ev_estimator takes it) on frames padded to a multiple
    of 4 and cut back: ``velocity`` is tests/decoder_ref.velocity."""
    Ty = y_t.shape[-1]
    pad = -Ty % 4
    y_p, mu_p = torch.nn.functional.pad(y_t, (0, pad)), torch.nn.functional.pad(mu_y, (0, pad))
    rows = [velocity(sd, y_p[b:b + 1], mu_p[b:b + 1], y_lengths[b:b + 1], spk[b:b + 1], float(t[b]), dtype=dtype) for b in range(y_t.shape[0])]
    return torch.cat(rows)[:, :, :Ty]


def diff_loss_fp32_oracle(velocity, sd, y, mu_y, y_lengths, spk, t, z, want):
    """Relative error, against the float64 value ``want``, of compute_loss evaluated as the reference evaluates it in float32 on the
    CPU: y_t and u, the estimator (tests/decoder_ref.velocity in float32) and both reductions in float32."""
    y_t, u = cfm_inputs(y.float(), t.float(), z.float())
    v = velocity_padded(velocity, sd, y_t, mu_y.float(), y_lengths, spk, t, torch.float32).float()
    mask = (torch.arange(y.shape[-1])[None, :] < y_lengths[:, None]).float().unsqueeze(1)
    loss = torch.nn.functional.mse_loss(v, u, reduction="sum") / (torch.sum(mask) * u.shape[1])
    assert loss.dtype == torch.float32
    return abs(float(loss) - want) / want
