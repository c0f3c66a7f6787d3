"""numpy float64 restatement of ev_dtw's semantics (include/emojivoice.h), vectorised per anti-diagonal so that
4096 x 4096 cells are feasible, and the input builders the DTW tests share.

For a row with tx frames of x (C, tx) and ty frames of y (C, ty):
    c[i, j]   sum_c (x[c, i] - y[c, j])^2 in float64, ascending c; metric 0 takes the square root, metric 1 leaves the square
    D[0, 0]   c[0, 0];  otherwise D[i, j] = c[i, j] + m, m the smallest of the predecessors that exist, in the order diagonal (i-1, j-1),
              up (i-1, j), left (i, j-1), a later one replacing an earlier one only when STRICTLY smaller (ties: diagonal, up, left)
    S[i, j]   S[chosen] + 1, S[0, 0] = 1
    outputs   cost = D[tx-1, ty-1], steps = K = S[tx-1, ty-1], path = the K cells from (0, 0) to (tx-1, ty-1) that replaying the choices
              from the end visits, ascending, then (-1, -1) up to Tx + Ty - 1 entries
A row with tx < 1, ty < 1, tx > Tx or ty > Ty gives cost 0, steps 0 and a path of -1.

numpy has no fma: the local cost here is a multiply and an add per channel where the device uses one fma, and the cost of a path of K
cells may therefore differ by about K 2^-53 relative.  A different rounding can only change the PATH where two predecessors of a cell on
it are that close, so every result carries its PATH MARGIN: the smallest gap between the best and the second-best predecessor over the
cells of the path, divided by the cost (inf where every cell of the path has a single predecessor, or where the cost is 0 and no gap is).
Integer-valued inputs under metric 1 are exact in float64 in any order, ties included: there the comparison is for equality of
everything, whatever the margin.
"""
import numpy as np

GARBAGE = 50.0                           # what lies behind a row's length: loud, so that reading it would show
INF = float("inf")


def local_cost(x, y, metric=0):
    """c (tx, ty) float64 of x (C, tx) against y (C, ty)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    acc = np.zeros((x.shape[1], y.shape[1]))
    for c in range(x.shape[0]):
        d = x[c][:, None] - y[c][None, :]
        acc += d * d
    return np.sqrt(acc) if metric == 0 else acc


def backtrack(choice, tx, ty):
    """The cells from (0, 0) to (tx-1, ty-1), ascending, that the recorded choices (0 diagonal, 1 up, 2 left) lead through."""
    i, j, cells = tx - 1, ty - 1, []
    while True:
        cells.append((i, j))
        if i == 0 and j == 0:
            break
        ch = int(choice[i, j])
        if ch != 2:
            i -= 1
        if ch != 1:
            j -= 1
    return np.asarray(cells[::-1], dtype=np.int32)


def path_margin(D, cells, cost):
    gap = INF
    for i, j in cells:
        pred = []
        if i > 0 and j > 0:
            pred.append(D[i - 1, j - 1])
        if i > 0:
            pred.append(D[i - 1, j])
        if j > 0:
            pred.append(D[i, j - 1])
        if len(pred) >= 2:
            pred.sort()
            gap = min(gap, pred[1] - pred[0])
    if gap == 0:
        return 0.0
    return INF if (gap == INF or cost == 0) else float(gap / cost)


def dtw_row(x, y, metric=0):
    """One row: (cost, steps, cells (K, 2) int32, margin), the recurrence run one anti-diagonal at a time."""
    D = local_cost(x, y, metric)                                  # holds c; cell by cell it becomes D
    tx, ty = D.shape
    choice = np.zeros((tx, ty), dtype=np.uint8)
    s1 = np.zeros(tx, dtype=np.int64)                             # S of diagonal k - 1, indexed by i
    s2 = np.zeros(tx, dtype=np.int64)                             # k - 2
    s1[0] = 1
    for k in range(1, tx + ty - 1):
        i = np.arange(max(0, k - ty + 1), min(tx - 1, k) + 1)
        j = k - i
        hi, hj = i > 0, j > 0
        dg = np.full(i.size, INF)
        up = np.full(i.size, INF)
        lf = np.full(i.size, INF)
        m = hi & hj
        dg[m] = D[i[m] - 1, j[m] - 1]
        up[hi] = D[i[hi] - 1, j[hi]]
        lf[hj] = D[i[hj], j[hj] - 1]
        best, ch = dg, np.zeros(i.size, dtype=np.uint8)
        t = up < best
        best = np.where(t, up, best)
        ch[t] = 1
        t = lf < best
        best = np.where(t, lf, best)
        ch[t] = 2
        D[i, j] += best
        choice[i, j] = ch
        im = np.maximum(i - 1, 0)
        s0 = np.zeros(tx, dtype=np.int64)
        s0[i] = np.where(ch == 0, s2[im], np.where(ch == 1, s1[im], s1[i])) + 1
        s2, s1 = s1, s0
    cells = backtrack(choice, tx, ty)
    cost, steps = float(D[-1, -1]), int(s1[tx - 1])
    assert steps == len(cells)
    return cost, steps, cells, path_margin(D, cells, cost)


def dtw_loop(x, y, metric=0):
    """The same semantics as a plain double loop (the statement dtw_row is checked against): (cost, steps, cells)."""
    c = local_cost(x, y, metric)
    tx, ty = c.shape
    D, S, choice = np.zeros((tx, ty)), np.zeros((tx, ty), dtype=np.int64), np.zeros((tx, ty), dtype=np.uint8)
    for i in range(tx):
        for j in range(ty):
            if i == 0 and j == 0:
                D[0, 0], S[0, 0] = c[0, 0], 1
                continue
            best, ch = None, 0
            if i > 0 and j > 0:
                best, ch = D[i - 1, j - 1], 0
            if i > 0 and (best is None or D[i - 1, j] < best):
                best, ch = D[i - 1, j], 1
            if j > 0 and (best is None or D[i, j - 1] < best):
                best, ch = D[i, j - 1], 2
            D[i, j] = c[i, j] + best
            S[i, j] = S[(i - 1, j - 1) if ch == 0 else (i - 1, j) if ch == 1 else (i, j - 1)] + 1
            choice[i, j] = ch
    return float(D[-1, -1]), int(S[-1, -1]), backtrack(choice, tx, ty)


def dtw(x, y, x_lengths=None, y_lengths=None, metric=0):
    """The batch: x (B, C, Tx), y (B, C, Ty) -> {"cost" (B,) float64, "steps" (B,) int32, "path" (B, Tx + Ty - 1, 2) int32, "margin" (B,)};
    a bad row has margin inf."""
    x, y = np.asarray(x), np.asarray(y)
    B, _, Tx = x.shape
    Ty = y.shape[2]
    out = {"cost": np.zeros(B), "steps": np.zeros(B, dtype=np.int32), "path": np.full((B, Tx + Ty - 1, 2), -1, dtype=np.int32),
           "margin": np.full(B, INF)}
    for b in range(B):
        tx = Tx if x_lengths is None else int(x_lengths[b])
        ty = Ty if y_lengths is None else int(y_lengths[b])
        if tx < 1 or ty < 1 or tx > Tx or ty > Ty:
            continue
        cost, steps, cells, margin = dtw_row(x[b, :, :tx], y[b, :, :ty], metric)
        out["cost"][b], out["steps"][b], out["margin"][b] = cost, steps, margin
        out["path"][b, :steps] = cells
    return out


# ---- input builders --------------------------------------------------------------------------------------------------------------------
def integer_pair(C, tx, ty, seed):
    """Integer-valued features in [-2, 2]: everything is exact under metric 1, and ties are frequent."""
    g = np.random.default_rng(seed)
    return g.integers(-2, 3, (C, tx)).astype(np.float32), g.integers(-2, 3, (C, ty)).astype(np.float32)


def noisy_warp_pair(C, tx, ty, seed, noise=0.3):
    """Seeded Gaussian x (C, tx); y = x at ty sorted random indices plus ``noise`` sigma of Gaussian noise."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((C, tx))
    idx = np.sort(g.integers(0, tx, ty))
    y = x[:, idx] + noise * g.standard_normal((C, ty))
    return x.astype(np.float32), y.astype(np.float32)


def covering_warp(tx, ty, seed):
    """ty >= tx non-decreasing indices into tx frames that cover every one of them."""
    assert ty >= tx
    g = np.random.default_rng(seed)
    return np.sort(np.concatenate([np.arange(tx), g.integers(0, tx, ty - tx)]))


def pad_batch(rows, Tx=None, Ty=None, fill=GARBAGE):
    """[(x (C, tx), y (C, ty)), ...] -> x (B, C, Tx), y (B, C, Ty) with ``fill`` behind each row's length, xlen, ylen."""
    C = rows[0][0].shape[0]
    xl, yl = [r[0].shape[1] for r in rows], [r[1].shape[1] for r in rows]
    Tx, Ty = Tx or max(xl), Ty or max(yl)
    x, y = np.full((len(rows), C, Tx), fill, np.float32), np.full((len(rows), C, Ty), fill, np.float32)
    for b, (a, c) in enumerate(rows):
        x[b, :, : xl[b]], y[b, :, : yl[b]] = a, c
    return x, y, xl, yl


EXACT_CASES = [(1, 7, 5), (2, 23, 31), (5, 64, 65)]                                      # (C, Tx, Ty), metric 1
EUCLID_CASES = [(13, 37, 45), (1, 65, 3), (128, 5, 70), (13, 130, 97), (80, 70, 129)]    # (C, Tx, Ty), metric 0
EDGE_CASES = [(1, 1), (1, 9), (9, 1), (1025, 3), (3, 1025)]                              # (Tx, Ty), C = 3
LIMIT_CASE = (1, 4096, 4096)                                                              # (C, Tx, Ty), see limit_pair


def ragged_lengths(Tx, Ty):
    """The three rows of a Euclidean case: the padded size, and two shorter ones."""
    return [(Tx, Ty), (max(1, 2 * Tx // 3), max(1, 3 * Ty // 4)), (max(1, Tx // 2 + 1), Ty)]


def euclid_batch(C, Tx, Ty):
    rows = [noisy_warp_pair(C, tx, ty, seed=1000 * C + 10 * Tx + r) for r, (tx, ty) in enumerate(ragged_lengths(Tx, Ty))]
    return pad_batch(rows, Tx, Ty)


def exact_batch(C, Tx, Ty):
    rows = [integer_pair(C, tx, ty, seed=77 * C + Tx + r) for r, (tx, ty) in enumerate([(Tx, Ty), (max(1, Tx - 3), max(1, Ty - 2))])]
    return pad_batch(rows, Tx, Ty)


def edge_batch(Tx, Ty, C=3):
    return pad_batch([noisy_warp_pair(C, Tx, Ty, seed=5 * Tx + Ty)], Tx, Ty)


LIMIT_METRIC = 1


def limit_pair():
    """The case at the limit, (B, C, Tx, Ty) = (1, 1, 4096, 4096), for LIMIT_METRIC = 1.  One channel under metric 0 is one-dimensional L1:
    every partial sum of |x_i - y_j| over float32 inputs is exact in float64, so paths that tie on paper tie in the bits, and the margin is
    exactly 0 (seen at every seed tried, from 1024 x 1024 up).  The squared distance has no such structure; of the seeds 4096 .. 4101 this
    one has a margin of 2.2e-9 (the others 2e-13 .. 4e-10; tests/test_gpu_dtw.py asserts it before it compares)."""
    C, Tx, Ty = LIMIT_CASE
    x, y = noisy_warp_pair(C, Tx, Ty, seed=4100)
    return x[None], y[None]
