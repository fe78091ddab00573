"""The numpy restatement of lf_mkd_select_edges_device (include/lf_mkd.h), in two independent formulations -- a stable argsort
of -votes over the candidates with the UNIQUE rule as one boolean table, and a plain Python sort of (-votes, column) tuples with
the UNIQUE rule in loops -- and the tables the CPU and the GPU tests share.

    candidates of row i   the columns j with votes[i][j] >= min_votes, under skip_self also j != i
    order                 larger votes first, among equal votes the LOWER column first
    picks P(i)            the first min(k, candidates) of them; rank [n_a][k] holds them, -1 behind; rank_votes their votes, 0
    edges                 the picks in the order i, then rank; with `unique` a pick (i, j) is an edge iff j > i, or j < i and
                          i is not in P(j), and it is written (min, max)
    counts                [min(S, capacity), S, picks, rows with a pick]; the arrays hold 0xFFFFFFFF (votes: 0) behind the edges
"""
import numpy as np

PAD = 0xFFFFFFFF
SKIP_SELF, UNIQUE = 1, 2


class Result:
    def __init__(self, rank, rank_votes, edge_a, edge_b, edge_votes, counts):
        self.rank, self.rank_votes = np.asarray(rank, np.int32), np.asarray(rank_votes, np.uint32)
        self.edge_a, self.edge_b, self.edge_votes = (np.asarray(x, np.uint32) for x in (edge_a, edge_b, edge_votes))
        self.counts = [int(c) for c in counts]

    def arrays(self):
        return [self.rank, self.rank_votes, self.edge_a, self.edge_b, self.edge_votes, np.array(self.counts, np.uint32)]

    def same(self, other):
        return all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(self.arrays(), other.arrays()))


def finish(n_a, k, rank, rank_votes, edges, capacity):
    capacity = n_a * k if capacity is None else capacity
    kept = edges[:capacity]
    pad = capacity - len(kept)
    ea = np.array([e[0] for e in kept] + [PAD] * pad, np.uint32)
    eb = np.array([e[1] for e in kept] + [PAD] * pad, np.uint32)
    ev = np.array([e[2] for e in kept] + [0] * pad, np.uint32)
    picks = int((rank >= 0).sum())
    rows = int((rank[:, 0] >= 0).sum()) if k and n_a else 0
    return Result(rank, rank_votes, ea, eb, ev, [len(kept), len(edges), picks, rows])


def select_edges(votes, k, min_votes=1, skip_self=False, unique=False, capacity=None, loops=False):
    """the restatement; loops=True: the second formulation"""
    votes = np.asarray(votes).astype(np.uint32, copy=False)
    n_a, n_b = votes.shape
    assert not unique or n_a == n_b
    rank = np.full((n_a, k), -1, np.int32)
    rank_votes = np.zeros((n_a, k), np.uint32)
    if loops:
        for i in range(n_a):
            cand = [(-int(votes[i, j]), j) for j in range(n_b) if int(votes[i, j]) >= min_votes and not (skip_self and j == i)]
            for c, (v, j) in enumerate(sorted(cand)[:k]):
                rank[i, c], rank_votes[i, c] = j, -v
        edges = []
        for i in range(n_a):
            for c in range(k):
                j = int(rank[i, c])
                if j < 0:
                    continue
                if not unique:
                    edges.append((i, j, int(rank_votes[i, c])))
                elif j > i:
                    edges.append((i, j, int(rank_votes[i, c])))
                elif j < i and i not in [int(x) for x in rank[j]]:
                    edges.append((j, i, int(rank_votes[i, c])))
        return finish(n_a, k, rank, rank_votes, edges, capacity)
    for i in range(n_a):
        ok = votes[i] >= min_votes
        if skip_self and i < n_b:
            ok[i] = False
        cand = np.flatnonzero(ok)
        best = cand[np.argsort(-votes[i, cand].astype(np.int64), kind="stable")][:k]
        rank[i, :len(best)] = best
        rank_votes[i, :len(best)] = votes[i, best]
    ii = np.repeat(np.arange(n_a, dtype=np.int64), k)
    jj = rank.reshape(-1).astype(np.int64)
    vv = rank_votes.reshape(-1).astype(np.int64)
    edge = jj >= 0
    if unique:
        picked = np.zeros((n_a, n_a), bool)                                     # picked[i][j]: j is in P(i)
        picked[ii[edge], jj[edge]] = True
        j_ok = np.where(edge, jj, 0)
        edge = edge & (jj != ii) & ((jj > ii) | ~picked[j_ok, ii])
        lo, hi = np.minimum(ii, jj), np.maximum(ii, jj)
    else:
        lo, hi = ii, jj
    edges = list(zip(lo[edge].tolist(), hi[edge].tolist(), vv[edge].tolist()))
    return finish(n_a, k, rank, rank_votes, edges, capacity)


def table(kind, n_a, n_b, seed=0):
    """(votes uint32 [n_a][n_b], the min_votes values worth running) of one kind of table"""
    rng = np.random.default_rng([seed, n_a, n_b])
    col = np.arange(n_b, dtype=np.uint64)[None, :]
    row = np.arange(n_a, dtype=np.uint64)[:, None]
    if kind == "ties":                                                         # nearly everything ties
        return rng.integers(0, 4, (n_a, n_b)).astype(np.uint32), (0, 1, 3)
    if kind == "equal":
        return np.full((n_a, n_b), 7, np.uint32), (1, 7)
    if kind == "zero":
        return np.zeros((n_a, n_b), np.uint32), (0, 1)
    if kind == "ascending":                                                    # every column enters the list: the slow extreme
        return (col + 5 * row + 1).astype(np.uint32), (1,)
    if kind == "descending":                                                   # only the first ones do
        return (n_b - col + 5 * row).astype(np.uint32), (1,)
    if kind == "huge":                                                         # the sign bit and 2^32 - 1 are ordinary
        v = rng.integers(2 ** 31 - 2, 2 ** 31 + 3, (n_a, n_b)).astype(np.uint32)
        v[rng.random((n_a, n_b)) < 0.2] = 0xFFFFFFFF
        v[rng.random((n_a, n_b)) < 0.2] = 3
        return v, (1, 2 ** 31, 0xFFFFFFFF)
    if kind == "diagonal":                                                     # every row's maximum is its own column
        v = rng.integers(0, 100, (n_a, n_b)).astype(np.uint32)
        d = np.arange(min(n_a, n_b))
        v[d, d] = 1000
        return v, (1,)
    if kind == "above":                                                        # min_votes above every entry
        return rng.integers(0, 50, (n_a, n_b)).astype(np.uint32), (50,)
    raise ValueError(kind)


KINDS = ("ties", "equal", "zero", "ascending", "descending", "huge", "diagonal", "above")


def unique_table():
    """5 images: 0 and 1 pick each other (mutual), 2 picks 0 but 0 does not pick 2 (one-sided, larger picks smaller), 1 picks
    3 but 3 picks 4 only (one-sided, smaller picks larger), and 4's best column is itself (a self pick without skip_self).
    k = 2, min_votes = 1."""
    v = np.zeros((5, 5), np.uint32)
    v[0, 1], v[1, 0] = 9, 8
    v[1, 3] = 5
    v[2, 0] = 7
    v[3, 4] = 6
    v[4, 4], v[4, 3] = 10, 2
    return v


def cases():
    """(name, votes, k, min_votes, skip_self, unique) of every small case both formulations are run on"""
    out = []
    for n_a, n_b in ((1, 1), (1, 7), (3, 2), (3, 65), (7, 33), (2, 130)):
        for kind in KINDS:
            v, mins = table(kind, n_a, n_b)
            for k in (1, 2, 3, 5, 32):
                for m in mins:
                    out.append((f"{kind} {n_a}x{n_b} k={k} min={m}", v, k, m, False, False))
            out.append((f"{kind} {n_a}x{n_b} skip self", v, 3, mins[0], True, False))
    for n in (1, 2, 3, 9, 40):
        for kind in KINDS:
            v, mins = table(kind, n, n, seed=1)
            for k in (1, 2, 4, 32):
                for skip_self in (False, True):
                    out.append((f"{kind} {n}^2 k={k} unique skip={skip_self}", v, k, mins[0], skip_self, True))
    out.append(("unique by hand", unique_table(), 2, 1, False, True))
    out.append(("unique by hand, skip self", unique_table(), 2, 1, True, True))
    return out
