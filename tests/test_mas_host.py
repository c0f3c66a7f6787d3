"""Host side of the monotonic alignment search: the numpy restatement (tests/mas_ref.py) against the reference's compiled search
(tests/golden/mas_vectors.npz, written by tests/golden/make_mas_golden.py) and against brute force, the C ABI's declarations and
exports, and the loss helpers on a hand-computed example.  No GPU."""
import math
import os
import re
import subprocess

import numpy as np
import torch

import mas_ref as R
from emojivoice_amd import _lib
from emojivoice_amd.text_encoder import duration_loss

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ev_maximum_path", "ev_log_prior", "ev_mas_align")


def golden_cases():
    with np.load(os.path.join(REPO, "tests", "golden", "mas_vectors.npz")) as z:
        names = sorted(k[: -len("_value")] for k in z.files if k.endswith("_value"))
        return {n: {k: z[f"{n}_{k}"] for k in ("value", "xlen", "ylen", "path", "final")} for n in names}


def test_restatement_reproduces_the_reference_search_exactly():
    cases = golden_cases()
    assert {"random", "square", "one_token", "grid_ties", "all_equal"} <= set(cases)
    for name, c in cases.items():
        path, final = R.maximum_path(R.masked_value(c["value"], c["xlen"], c["ylen"]), c["xlen"], c["ylen"])
        assert np.array_equal(path, c["path"]), name
        assert final.tobytes() == c["final"].tobytes(), f"{name}: the DP's value array differs in some bit"
        R.check_structure(path, c["xlen"], c["ylen"])
    assert any((c["xlen"] == c["ylen"]).any() for c in cases.values()) and any((c["xlen"] == 1).all() for c in cases.values())


def test_masking_does_not_matter_inside_the_band():
    """The device entry point takes raw scores and lengths: the cells the search reads are all inside the mask."""
    for name, c in golden_cases().items():
        path, _ = R.maximum_path(c["value"], c["xlen"], c["ylen"])
        assert np.array_equal(path, c["path"]), name


def test_search_finds_the_brute_force_maximum_and_the_reference_tie():
    g = torch.Generator().manual_seed(3)
    for tx in range(1, 5):
        for ty in range(tx, 8):
            for kind in ("random", "grid"):
                v = torch.randn(1, tx, ty, generator=g) if kind == "random" else torch.randint(-1, 2, (1, tx, ty), generator=g).float()
                path, _ = R.maximum_path(v, [tx], [ty])
                durs = tuple(int(d) for d in path[0].sum(-1))
                scores = {d: R.path_score(v[0].numpy(), d) for d in R.monotonic_paths(tx, ty)}
                assert len(scores) == math.comb(ty - 1, tx - 1) and durs in scores
                assert scores[durs] >= max(scores.values()) - 1e-5, (tx, ty, kind)
                if kind == "grid":        # exact arithmetic.  The backtrack's strict '<' stays on the token at a tie, so among the maximal
                    best = [d for d, s in scores.items() if s == max(scores.values())]   # paths it gives the LAST token the most frames,
                    assert scores[durs] == max(scores.values())                            # then the one before it, and so on
                    assert durs == max(best, key=lambda d: d[::-1]), (tx, ty, durs, best)


def test_one_decision_bit_per_cell_is_enough():
    """The device kernel keeps only the running column and, per cell, the bit `x != 0 and (x == y or v_cur < v_prev)` taken in the
    forward step; a backtrack over those bits gives the restatement's path."""
    g = torch.Generator().manual_seed(8)
    for (tx, ty, scale) in ((1, 1, 1.0), (1, 9, 1.0), (7, 7, 1.0), (13, 40, 1.0), (40, 90, 1e6), (12, 33, 0.0)):
        v = (torch.randn(tx, ty, generator=g) * scale).numpy().astype(np.float32)
        want, _ = R.maximum_path(v[None], [tx], [ty])
        bits = np.zeros((tx, ty), bool)
        prev = np.zeros(tx, np.float32)
        for y in range(ty):
            cur = prev.copy()
            for x in range(max(0, tx + y - ty), min(tx, y + 1)):
                vc = R.NEG if x == y else prev[x]
                vp = (np.float32(0) if y == 0 else R.NEG) if x == 0 else prev[x - 1]
                cur[x] = np.float32(max(vc, vp)) + v[x, y]
                bits[x, y] = x != 0 and (x == y or vc < vp)
            prev = cur
        path = np.zeros((tx, ty), np.int8)
        index = tx - 1
        for y in range(ty - 1, -1, -1):
            path[index, y] = 1
            if index != 0 and bits[index, y]:
                index -= 1
        assert np.array_equal(path, want[0]), (tx, ty, scale)


def test_header_declares_and_library_exports_the_search():
    with open(os.path.join(REPO, "include", "emojivoice.h")) as f:
        header = f.read()
    for n in NAMES:
        assert re.search(rf"\bint\s+{n}\s*\(\s*ev_handle\s*\*", header), f"{n} is not declared in include/emojivoice.h"
        assert n in _lib.EXPORTS
    assert re.search(r"#define\s+EV_ABI_VERSION\s+4\b", header)
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = _lib.load_library()
    for n in NAMES:
        assert hasattr(lib, n), f"{n} is not exported by the built library"
    nm = "/opt/rocm/llvm/bin/llvm-nm"
    if os.path.exists(nm):
        syms = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        for n in NAMES:
            assert re.search(rf"\sT\s+{n}\b", syms), n


def test_loss_helpers_on_a_hand_computed_example():
    # two tokens, three frames, one channel pair: token 0 takes frames 0-1, token 1 takes frame 2
    attn = torch.tensor([[[1.0, 1.0, 0.0], [0.0, 0.0, 1.0]]])
    logw = torch.tensor([[[math.log(2.0), 0.5]]])
    xl, yl = torch.tensor([2]), torch.tensor([3])
    mu_x = torch.tensor([[[1.0, -1.0], [0.0, 2.0]]])                      # (1, C = 2, Tx = 2)
    y = torch.tensor([[[1.5, 1.0, 0.0], [0.0, -1.0, 2.0]]])              # (1, 2, 3)
    dur, prior, mu_y = R.dur_and_prior_loss(attn, logw, mu_x, y, xl, yl)
    # logw_ = log(1e-8 + [2, 1]); (log 2 - log(2 + 1e-8))^2 + (0.5 - log(1 + 1e-8))^2 over 2 tokens
    want_dur = ((math.log(2.0) - math.log(2.0 + 1e-8)) ** 2 + (0.5 - math.log(1.0 + 1e-8)) ** 2) / 2
    assert abs(dur - want_dur) <= 1e-15
    assert torch.equal(mu_y, torch.tensor([[[1.0, 1.0, -1.0], [0.0, 0.0, 2.0]]], dtype=torch.float64))
    # (y - mu_y)^2 = [[.25, 0, 1], [0, 1, 0]] -> sum 2.25; 0.5 * (2.25 + 6 log 2 pi) / (3 * 2)
    want_prior = 0.5 * (2.25 + 6 * math.log(2 * math.pi)) / 6
    assert abs(prior - want_prior) <= 1e-15
    logw_ = torch.log(1e-8 + attn.double().sum(-1)).unsqueeze(1)
    assert abs(float(duration_loss(logw.double(), logw_, xl)) - want_dur) <= 1e-15
    assert abs(float(duration_loss(logw, logw_.float(), xl)) - want_dur) <= 1e-6
    # the flow-matching loss: v = 0 everywhere, t = 0.5, z = 1: u = y - (1 - 1e-4), loss = sum u^2 / (3 * 2)
    z = torch.ones_like(y)
    y_t, u = R.cfm_inputs(y.double(), torch.tensor([0.5], dtype=torch.float64), z.double())
    assert torch.allclose(y_t, (1 - (1 - 1e-4) * 0.5) * z.double() + 0.5 * y.double(), rtol=0, atol=1e-15)
    want = float(((y.double() - (1 - 1e-4)) ** 2).sum() / 6)
    assert abs(R.diff_loss_from_velocity(torch.zeros_like(y), u, yl) - want) <= 1e-15


def test_log_prior_forms_agree():
    mu_x, y, _, _ = R.mel_pairs("aligned", 2, 9, 30, seed=4)
    a, b = R.log_prior(mu_x, y), R.log_prior(mu_x, y, torch.float32)
    assert a.dtype == torch.float64 and b.dtype == torch.float32 and tuple(a.shape) == (2, 9, 30)
    assert float((a - b.double()).abs().max()) <= 1e-3
    assert float((a - R.log_prior_fp64_chunked(mu_x, y, rows=4)).abs().max()) <= 1e-11
    i, j = 3, 7
    want = -0.5 * float(((y[1, :, j].double() - mu_x[1, :, i].double()) ** 2).sum()) - 0.5 * math.log(2 * math.pi) * 80
    assert abs(float(a[1, i, j]) - want) <= 1e-10
