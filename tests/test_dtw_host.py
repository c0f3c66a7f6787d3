"""The DTW yardstick and the host layer of the evaluation report, without a GPU.

tests/dtw_ref.py is what tests/test_gpu_dtw.py holds ev_dtw to; here it is held to the plain double loop it restates, to the minimum over
every monotone path (enumerated), and to a hand-written tie case.  audio.mel_cepstrum, the MCD constant and audio.f0_errors are plain
torch / numpy and are checked on known answers.  Last, the Euclidean cases of the GPU tests are shown to have a path margin far above what a
different rounding of the local cost could move.
"""
import itertools
import math

import numpy as np
import pytest
import torch

import dtw_ref as R
from emojivoice_amd import audio


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("C,tx,ty", [(1, 1, 1), (1, 1, 6), (2, 6, 1), (3, 7, 5), (2, 12, 19), (4, 33, 20)])
def test_vectorised_restatement_equals_the_double_loop(C, tx, ty, metric):
    for maker in (R.integer_pair, R.noisy_warp_pair):
        x, y = maker(C, tx, ty, seed=tx + 3 * ty)
        cost, steps, cells, _ = R.dtw_row(x, y, metric)
        cost2, steps2, cells2 = R.dtw_loop(x, y, metric)
        assert cost == cost2 and steps == steps2 and np.array_equal(cells, cells2)
        assert max(tx, ty) <= steps <= tx + ty - 1 and tuple(cells[0]) == (0, 0) and tuple(cells[-1]) == (tx - 1, ty - 1)
        d = np.diff(cells, axis=0)
        assert np.all((d >= 0) & (d <= 1)) and np.all(d.sum(axis=1) >= 1), "steps are diagonal, up or left"


def monotone_paths(tx, ty):
    def walk(i, j):
        if i == tx - 1 and j == ty - 1:
            yield [(i, j)]
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < tx and j + dj < ty:
                for rest in walk(i + di, j + dj):
                    yield [(i, j)] + rest
    return walk(0, 0)


@pytest.mark.parametrize("tx,ty", list(itertools.product(range(1, 5), range(1, 5))))
def test_cost_is_the_minimum_over_all_monotone_paths(tx, ty):
    x, y = R.integer_pair(2, tx, ty, seed=10 * tx + ty)                      # integers under metric 1: every sum is exact in any order
    c = R.local_cost(x, y, 1)
    best = min(sum(c[i, j] for i, j in path) for path in monotone_paths(tx, ty))
    cost, steps, cells, _ = R.dtw_row(x, y, 1)
    assert cost == best and sum(c[i, j] for i, j in cells) == cost and steps == len(cells)


def test_ties_go_diagonal_then_up_then_left():
    # one channel, metric 1: c[i, j] = (x_i - y_j)^2.  x = y = 0 everywhere: every cell ties, the path is the diagonal.
    z = np.zeros((1, 3), np.float32)
    cost, steps, cells, margin = R.dtw_row(z, z, 1)
    assert cost == 0.0 and steps == 3 and cells.tolist() == [[0, 0], [1, 1], [2, 2]] and margin == 0.0
    # x = (0, 0, 0) against y = (0, 1, 0): c = [[0, 1, 0]] * 3.  D = [[0, 1, 1], [0, 1, 1], [0, 1, 1]]: cell (2, 2) has diagonal 1, up 1, left 1
    # -> diagonal to (1, 1); (1, 1) has diagonal 0, up 1, left 0 -> diagonal to (0, 0).
    y = np.array([[0, 1, 0]], np.float32)
    cost, steps, cells, _ = R.dtw_row(z, y, 1)
    assert cost == 1.0 and steps == 3 and cells.tolist() == [[0, 0], [1, 1], [2, 2]]
    # 3 x 2, all zero: (2, 1) ties -> diagonal (1, 0); (1, 0) has only up.  The path goes up first, never left.
    cost, steps, cells, _ = R.dtw_row(z, z[:, :2], 1)
    assert steps == 3 and cells.tolist() == [[0, 0], [1, 0], [2, 1]]
    # up before left: x = (0, 5, 0), y = (0, 0): c = [[0, 0], [25, 25], [0, 0]], D = [[0, 0], [25, 25], [25, 25]].  (2, 1): diagonal 25, up 25,
    # left 25 -> diagonal (1, 0) -> up (0, 0).  (1, 1): diagonal 0, up 0, left 25 -> diagonal.
    x = np.array([[0, 5, 0]], np.float32)
    cost, steps, cells, _ = R.dtw_row(x, z[:, :2], 1)
    assert cost == 25.0 and cells.tolist() == [[0, 0], [1, 0], [2, 1]]
    # left only when strictly smaller: 2 x 3 with x = (0, 0), y = (0, 0, 0): (1, 2) ties -> diagonal (0, 1) -> left (0, 0)
    cost, steps, cells, _ = R.dtw_row(z[:, :2], z, 1)
    assert cells.tolist() == [[0, 0], [0, 1], [1, 2]]


def test_batch_wrapper_pads_and_zeroes_bad_rows():
    rows = [R.integer_pair(2, 5, 4, 1), R.integer_pair(2, 3, 6, 2)]
    x, y, xl, yl = R.pad_batch(rows)
    xl2, yl2 = xl + [0], yl + [3]
    x3, y3 = np.concatenate([x, x[:1]]), np.concatenate([y, y[:1]])
    out = R.dtw(x3, y3, xl2, yl2, 1)
    assert out["path"].shape == (3, 5 + 6 - 1, 2)
    for b, (a, c) in enumerate(rows):
        cost, steps, cells, _ = R.dtw_row(a, c, 1)
        assert out["cost"][b] == cost and out["steps"][b] == steps and np.array_equal(out["path"][b, :steps], cells)
        assert np.all(out["path"][b, steps:] == -1)
    assert out["cost"][2] == 0 and out["steps"][2] == 0 and np.all(out["path"][2] == -1)


def test_covering_warp_is_recovered_exactly():
    g = np.random.default_rng(3)
    x = g.standard_normal((4, 9)).astype(np.float32)
    idx = R.covering_warp(9, 15, seed=4)
    assert np.all(np.diff(idx) >= 0) and set(idx.tolist()) == set(range(9))
    cost, steps, cells, _ = R.dtw_row(x, x[:, idx], 0)
    assert cost == 0.0 and steps == 15 and cells.tolist() == [[int(i), j] for j, i in enumerate(idx)]


# ---- the host layer ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels,n_coeffs", [(80, 13), (80, 79), (16, 5)])
def test_dct_matrix_is_orthonormal(n_mels, n_coeffs):
    D = audio.dct_matrix(n_mels, n_coeffs)
    assert D.dtype == np.float64 and D.shape == (n_coeffs, n_mels)
    assert np.max(np.abs(D @ D.T - np.eye(n_coeffs))) <= 1e-14
    assert np.max(np.abs(D @ np.ones(n_mels))) <= 1e-13, "coefficient 0 (the energy) is left out: a constant mel has no cepstrum"


def test_mel_cepstrum_shape_dtype_and_single_rounding():
    g = torch.Generator().manual_seed(0)
    mel = torch.randn(2, 80, 7, generator=g) * 2 - 5
    c = audio.mel_cepstrum(mel, 13)
    assert c.shape == (2, 13, 7) and c.dtype == torch.float32
    want = np.einsum("km,bmt->bkt", audio.dct_matrix(80, 13), mel.numpy().astype(np.float64))
    assert np.max(np.abs(c.numpy().astype(np.float64) - want)) <= 2.0 ** -24 * np.max(np.abs(want)) * 1.01
    with pytest.raises(ValueError, match="n_coeffs"):
        audio.mel_cepstrum(mel, 80)


def test_mcd_constant_on_a_one_frame_pair():
    assert audio.MCD_DB == 10.0 * math.sqrt(2.0) / math.log(10.0) and abs(audio.MCD_DB - 6.141851463713754) < 1e-12
    a = np.array([[0.5], [-1.25], [2.0]], np.float32)
    b = np.array([[0.25], [0.75], [-1.0]], np.float32)
    cost, steps, _, _ = R.dtw_row(a, b, 0)
    norm = math.sqrt(0.25 ** 2 + 2.0 ** 2 + 3.0 ** 2)
    assert steps == 1 and cost == norm
    mcd = audio.mcd_from_cost(torch.tensor([cost, 0.0], dtype=torch.float64), torch.tensor([steps, 0]))
    assert mcd.dtype == torch.float64 and abs(float(mcd[0]) - audio.MCD_DB * norm) <= 1e-12 * audio.MCD_DB * norm and math.isnan(float(mcd[1]))


def test_f0_errors_on_a_hand_made_path():
    f0_a = torch.tensor([[200.0, 220.0, 0.0, 440.0], [100.0, 0.0, 0.0, 0.0]])
    v_a = f0_a > 0
    f0_b = torch.tensor([[100.0, 0.0, 220.0], [0.0, 50.0, 0.0]])
    v_b = f0_b > 0
    # row 0: pairs (0,0) 2:1 -> 1200 cents; (1,0) 220/100; (2,1) both unvoiced; (3,2) 2:1 -> 1200; the (-1, -1) tail is not a pair
    path = torch.tensor([[[0, 0], [1, 0], [2, 1], [3, 2], [-1, -1], [-1, -1]],
                         [[0, 0], [0, 1], [-1, -1], [-1, -1], [-1, -1], [-1, -1]]], dtype=torch.int32)
    out = audio.f0_errors(f0_a, v_a, f0_b, v_b, path, torch.tensor([4, 2], dtype=torch.int32))
    c1 = 1200.0 * math.log2(2.2)
    assert out["voiced_pairs"].tolist() == [3, 1]
    assert abs(out["rmse_cents"][0] - math.sqrt((1200.0 ** 2 * 2 + c1 ** 2) / 3)) <= 1e-9
    assert abs(out["rmse_cents"][1] - 1200.0) <= 1e-9, "a 2:1 frequency ratio is 1200 cents"
    assert out["voicing_error"].dtype == torch.float64 and out["voicing_error"].tolist() == [0.0, 0.5]
    # no pair voiced on both sides: None; a differing flag on every pair: 1
    out = audio.f0_errors(f0_a[:1], v_a[:1], torch.zeros(1, 3), torch.zeros(1, 3, dtype=torch.bool), path[:1], torch.tensor([2]))
    assert out["rmse_cents"] == [None] and out["voiced_pairs"].tolist() == [0] and out["voicing_error"].tolist() == [1.0]
    # steps limits the pairs that count
    out = audio.f0_errors(f0_a[:1], v_a[:1], f0_b[:1], v_b[:1], path[:1], torch.tensor([1]))
    assert out["voiced_pairs"].tolist() == [1] and abs(out["rmse_cents"][0] - 1200.0) <= 1e-9 and out["voicing_error"].tolist() == [0.0]


def test_evaluation_means_pool_f0_over_voiced_pairs():
    from emojivoice_amd.cli import evaluation_means

    pairs = [{"mcd_db": 4.0, "f0_rmse_cents": 30.0, "voicing_error": 0.1, "voiced_pairs": 10},
             {"mcd_db": 6.0, "f0_rmse_cents": None, "voicing_error": 0.3, "voiced_pairs": 0},
             {"mcd_db": 8.0, "f0_rmse_cents": 60.0, "voicing_error": 0.2, "voiced_pairs": 30}]
    m = evaluation_means(pairs)
    assert m["pairs"] == 3 and m["mcd_db"] == 6.0 and abs(m["voicing_error"] - 0.2) < 1e-15 and m["voiced_pairs"] == 40
    assert abs(m["f0_rmse_cents"] - math.sqrt((900.0 * 10 + 3600.0 * 30) / 40)) < 1e-9
    assert evaluation_means(pairs[1:2])["f0_rmse_cents"] is None


def test_parse_pairs(tmp_path):
    from emojivoice_amd.cli import parse_pairs

    (tmp_path / "a.wav").write_bytes(b"")
    (tmp_path / "b.wav").write_bytes(b"")
    f = tmp_path / "pairs.txt"
    f.write_text("a.wav|b.wav\n\n" + f"{tmp_path / 'a.wav'}|b.wav|7\n")
    assert parse_pairs(f) == [(str(tmp_path / "a.wav"), str(tmp_path / "b.wav"), "0"), (str(tmp_path / "a.wav"), str(tmp_path / "b.wav"), "7")]


# ---- the margins of the GPU tests' Euclidean cases ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,Tx,Ty", R.EUCLID_CASES, ids=[f"C{c}-{a}x{b}" for c, a, b in R.EUCLID_CASES])
def test_euclidean_cases_have_a_path_margin(C, Tx, Ty):
    x, y, xl, yl = R.euclid_batch(C, Tx, Ty)
    ref = R.dtw(x, y, xl, yl, 0)
    print(f"\nDTW margins C{C} {Tx}x{Ty}: {ref['margin']}")
    assert np.all(ref["margin"] >= 1e-9)


@pytest.mark.parametrize("Tx,Ty", R.EDGE_CASES)
def test_edge_cases_have_a_path_margin(Tx, Ty):
    x, y, xl, yl = R.edge_batch(Tx, Ty)
    ref = R.dtw(x, y, xl, yl, 0)
    print(f"\nDTW margin edge {Tx}x{Ty}: {ref['margin']}")
    assert np.all(ref["margin"] >= 1e-9)
