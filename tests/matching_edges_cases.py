"""Seeded inputs of the matching-edges tests (no test in here; numpy only): batches of puzzles as pfpp_match_edges takes them.

A Batch is host data: per puzzle the assignment (int64 [N'_b], -1 = unmatched, empty = no rows), n_critical_pcs and n_pcs [B, P],
n_valid [B] and per puzzle critical_pcs_idx (int64 [sum n_pcs[b]]: per piece its n_critical_pcs distinct local indices in ascending
order, zeros behind them, as the classifier's compaction writes them)."""
from __future__ import annotations

from typing import List, NamedTuple

import numpy as np

CANARY = -7777          # what the tests write into corr / idx_a / idx_b before a launch


class Batch(NamedTuple):
    perm: List[np.ndarray]
    n_critical_pcs: np.ndarray
    n_valid: np.ndarray
    n_pcs: np.ndarray
    critical_pcs_idx: List[np.ndarray]

    def take(self, picks) -> "Batch":
        picks = list(picks)
        return Batch([self.perm[b] for b in picks], self.n_critical_pcs[picks], self.n_valid[picks], self.n_pcs[picks],
                     [self.critical_pcs_idx[b] for b in picks])


def points_and_critical(nc: np.ndarray, rng) -> tuple:
    """n_pcs [P] (every piece a few points more than its critical ones; a piece without critical points may be empty) and the
    puzzle's critical_pcs_idx"""
    nc = np.asarray(nc, dtype=np.int64)
    n_pcs = nc + rng.integers(0, 40, nc.size)
    crit = []
    for n, c in zip(n_pcs, nc):
        x = np.zeros(n, dtype=np.int64)
        x[:c] = np.sort(rng.choice(n, size=c, replace=False))
        crit.append(x)
    return n_pcs, np.concatenate(crit) if crit else np.zeros(0, np.int64)


def join(puzzles) -> Batch:
    """[(perm, nc [P], n_valid, n_pcs [P], crit)] -> Batch"""
    return Batch([np.asarray(p[0], dtype=np.int64) for p in puzzles], np.stack([p[1] for p in puzzles]).astype(np.int64),
                 np.asarray([p[2] for p in puzzles], dtype=np.int64), np.stack([p[3] for p in puzzles]).astype(np.int64), [p[4] for p in puzzles])


def fixture_batch(g, names) -> Batch:
    """the puzzles `names` of tests/matching_cases.py with the assignment, n_critical_pcs and critical_pcs_idx the reference's code
    produced for them (g = tests/golden/matching_head.npz)"""
    import matching_cases as cases

    pzs = [cases.make_puzzle(k) for k in names]
    return Batch([g[f"{k}_perm"].astype(np.int64) for k in names], np.stack([g[f"{k}_n_critical_pcs"] for k in names]).astype(np.int64),
                 np.asarray([int(p["part_valids"].sum()) for p in pzs], dtype=np.int64), np.stack([p["n_pcs"] for p in pzs]),
                 [g[f"{k}_critical_pcs_idx"].astype(np.int64) for k in names])


# ------------------------------------------------------------------------------------------------ the seeded batch
SIZES =[63, 64, 65, 257, 0, 1, 130, 1025]              # wave and workgroup edges, an empty piece in the middle, a one-row piece
RULE_SIZES = [10, 9, 12, 7, 0, 1, 8, 6]
# (row piece, row ordinals, column piece, column ordinals) of the rule puzzle
RULE_BLOCKS = [
    (0, [0, 1], 1, [3, 4]), (1, [0], 0, [0]),                       # (0, 1): 2 against 1 -> exactly 2: dropped
    (0, [2, 3, 4], 2, [5, 1, 7]),                                   # (0, 2): exactly 3 against 0: kept, rows ascending, columns not
    (1, [1, 2, 3], 2, [0, 2, 3]), (2, [0, 1, 2], 1, [8, 7, 6]),     # (1, 2): 3 against 3, a tie: the first block wins
    (0, [5, 6], 3, [0, 1]), (3, [0, 1, 2, 3], 0, [9, 7, 3, 1]),     # (0, 3): 2 against 4: the transposed block wins, its rows by column
    (6, [0, 1, 2], 6, [2, 0, 1]),                                   # same-piece matches: counted on the diagonal, never an edge
    (7, [0, 1, 2, 3], 6, [4, 5, 6, 7]),                             # (6, 7): 0 against 4: transposed
    (5, [0], 7, [5]),                                               # the one-row piece: 1 match, dropped
]


def random_puzzle(sizes, n_valid: int, rng, unmatched: float = 0.05):
    nc = np.asarray(sizes, dtype=np.int64)
    n = int(nc.sum())
    perm = rng.permutation(n).astype(np.int64)          # a random permutation: same-piece matches included
    perm[rng.random(n) < unmatched] = -1
    return (perm, nc, n_valid, *points_and_critical(nc, rng))


def rule_puzzle(rng):
    nc = np.asarray(RULE_SIZES, dtype=np.int64)
    start = np.cumsum(nc) - nc
    perm = np.full(int(nc.sum()), -1, dtype=np.int64)
    for pr, rows, pc, cols in RULE_BLOCKS:
        for r, c in zip(rows, cols):
            assert perm[start[pr] + r] == -1 and r < nc[pr] and c < nc[pc]
            perm[start[pr] + r] = start[pc] + c
    matched = perm[perm >= 0]
    assert np.unique(matched).size == matched.size
    return (perm, nc, 8, *points_and_critical(nc, rng))


def seeded_batch(seed: int = 5) -> Batch:
    """0: the piece sizes SIZES under a random permutation with 5 % of the rows unmatched; 1: the rule puzzle; 2: n_valid = 2 with
    critical points in four pieces; 3: no rows although pieces have critical points (assign=False); 4: a second random puzzle of
    other sizes; 5: no critical points and no rows; 6: an assignment of 100 rows for 140 critical points (it ends inside piece 1)"""
    rng = np.random.default_rng(seed)
    empty = lambda sizes, nv: (np.zeros(0, np.int64), np.asarray(sizes, dtype=np.int64), nv, *points_and_critical(sizes, rng))
    short = random_puzzle([50, 50, 0, 0, 0, 0, 0, 0], 3, rng)
    short = (short[0], np.asarray([50, 60, 30, 0, 0, 0, 0, 0], dtype=np.int64), 3, *points_and_critical([50, 60, 30, 0, 0, 0, 0, 0], rng))
    return join([random_puzzle(SIZES, 8, rng), rule_puzzle(rng), random_puzzle([40, 50, 30, 20, 0, 0, 0, 0], 2, rng),
                 empty([5, 6, 7, 0, 0, 0, 0, 0], 3), random_puzzle([200, 0, 190, 3, 66, 129, 511, 2], 7, rng), empty([0] * 8, 0), short])


# ------------------------------------------------------------------------------------------------ every pair kept
def all_pairs_batch(seed: int = 9) -> Batch:
    """P = 20 pieces of 57 critical points, 3 matches per ORDERED pair of pieces (N' = 1,140): every block ties with its opposite, the
    first wins, all 190 pairs are kept with 3 correspondences each.  Row 3 q + s of piece i (q = the rank of piece j among the others)
    goes to column 3 q' + sigma(s) of piece j (q' = the rank of i among j's others): a permutation"""
    rng = np.random.default_rng(seed)
    P, per = 20, 57
    nc = np.full(P, per, dtype=np.int64)
    perm = np.full(P * per, -1, dtype=np.int64)
    rank = lambda i, j: j if j < i else j - 1            # rank of piece j among the pieces other than i
    for i in range(P):
        for j in range(P):
            if i != j:
                sigma = rng.permutation(3)
                for s in range(3):
                    perm[i * per + 3 * rank(i, j) + s] = j * per + 3 * rank(j, i) + sigma[s]
    assert sorted(perm.tolist()) == list(range(P * per))
    return join([(perm, nc, P, *points_and_critical(nc, rng))])


# ------------------------------------------------------------------------------------------------ bad input
def bad_batch(kind: str, seed: int = 3) -> Batch:
    """three puzzles, the middle one broken: 'duplicate' (two rows with one column), 'too_large' (an entry equal to N'), 'negative'
    (an entry of -2).  Without the broken entry the middle puzzle has edges."""
    rng = np.random.default_rng(seed)
    pz = [random_puzzle([30, 41, 0, 29], 4, rng), random_puzzle([64, 70, 66, 0], 3, rng), random_puzzle([33, 0, 31, 36], 4, rng)]
    perm = pz[1][0]
    rows = np.nonzero(perm >= 0)[0]
    if kind == "duplicate":
        perm[rows[7]] = perm[rows[150]]
    elif kind == "too_large":
        perm[rows[11]] = perm.size
    elif kind == "negative":
        perm[rows[120]] = -2
    else:
        raise KeyError(kind)
    return join(pz)
