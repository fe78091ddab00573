"""Inputs that reach the parts of the screen matcher (match_screen + match_verify, local-features_amd/csrc/mkd_match.hip)
which random unit vectors leave alone: the screening margin, the record ring, the splits' shared floor, the fallback scan
with exclusion ranges, negative and zero similarities, rows far from unit norm.

Every generator returns (a, b, lo, hi, what): float32 rows, per-row exclusion ranges (or None, None) and a dict that says
how the case is meant to run (`splits` for LF_MKD_MATCH_SPLITS, `ratio`, the planted rows, ...).  Every generator has a
check_*() beside it that proves, with numpy alone, that the case reaches what it is meant to reach; tests/test_match_twin.py
asserts them on the CPU, so a case that has gone vacuous fails there and not on the GPU.

The model of the device the checks use, nothing of the library itself:
  screen   s~ = f64(f16(a)) @ f64(f16(b)).T, numpy's round-to-nearest f16 (match_split's conversion; the products of two f16
           are exact in f32, the f32 accumulation's ~1e-7 is far below everything checked here)
  margin   2.02e-3 |a| max|b| + 5e-7 (|a| + max|b|), the norms times 1.00001 (screen_margin, match_split)
  geometry a split is a contiguous range of 32-row b tiles, a stage two tiles; the lane group g = (row % 16) // 4 of a b row
           and its split name the stream (of one a row) that records it; an a row's sub-tile is (row % 64) // 16, its wave
           row // 64."""
import numpy as np

from test_gpu_match import descriptor_sets, unit

TILE, STAGE, REC_CAP = 32, 64, 64


def exact(a, b):
    return a.astype(np.float64) @ b.astype(np.float64).T


def screen(a, b):
    return a.astype(np.float16).astype(np.float64) @ b.astype(np.float16).astype(np.float64).T


def norms(x):
    return np.sqrt((x.astype(np.float64) ** 2).sum(axis=1)) * 1.00001


def margin(a, b):
    """the model's screening margin of every a row"""
    na, bm = norms(a), norms(b).max()
    return 2.02e-3 * na * bm + 5e-7 * (na + bm)


def split_of(rows, nb, splits):
    """the b split of b rows under LF_MKD_MATCH_SPLITS=splits (match_splits, launch_match_screen)"""
    tiles = (nb + TILE - 1) // TILE
    splits = max(1, min(splits, tiles))
    per = (tiles + splits - 1) // splits
    return np.asarray(rows) // (per * TILE)


def stage_of(rows, nb, splits):
    """the stage, within its split, at which a b row is scanned"""
    tiles = (nb + TILE - 1) // TILE
    per = (tiles + max(1, min(splits, tiles)) - 1) // max(1, min(splits, tiles))
    return (np.asarray(rows) % (per * TILE)) // STAGE


def mask_excluded(s, lo, hi):
    if lo is None:
        return s
    cols = np.arange(s.shape[1])[None, :]
    return np.where((cols >= lo[:, None]) & (cols < hi[:, None]), -np.inf, s)


def top2(s):
    """(index of the largest, the largest, the second largest) of every row"""
    order = np.argsort(s, axis=1, kind="stable")
    rows = np.arange(len(s))
    return order[:, -1], s[rows, order[:, -1]], s[rows, order[:, -2]]


# ---- (a) the screening margin -------------------------------------------------------------------------------------------

def _grid(rng, n, target):
    """n values on the f16 grid as (k, e, sign): mantissa 1 + k / 1024 with k in 1 .. 47, exponent -3, lowered to -4 or -5
    for as many elements as brings the squared norm below `target`, random signs."""
    k = rng.integers(1, 48, n)
    e = np.full(n, -3)
    for i in rng.permutation(n):
        if ((2.0 ** e * (1 + k / 1024)) ** 2).sum() < target:
            break
        e[i] = rng.integers(-5, -3)
    return k, e, rng.choice([-1.0, 1.0], n)


def _moved(grid, side):
    """the grid values moved by side * 0.49 ulp16 in magnitude, as float32: rounding to f16 takes them back to the grid"""
    k, e, sg = grid
    return (sg * (2.0 ** e * (1 + k / 1024) + side * 0.49 * 2.0 ** (e - 10))).astype(np.float32)


def _sq(x):
    return float((x.astype(np.float64) ** 2).sum())


N_DECOYS = 4
GAPS = (2e-5, 4e-5, 6e-5, 8e-5)       # s(true best) - s(decoy), float64


def margin_inversion(n_rows=12, na=200, nb=4096, seed=31):
    """n_rows queries whose true best is not among the screen's top two and sits deep inside the margin below them.
    Dimensions 0 .. 62 (U) carry the query and its true best b_t, both 0.49 ulp16 ABOVE the f16 grid in magnitude: the
    screen rounds them down and underestimates <a, b_t> by ~2^-10 relative.  Dimensions 64 .. 127 (V) carry the query and
    N_DECOYS decoys, 0.49 ulp16 BELOW the grid: the screen overestimates them as much.  Dimension 63 holds f16-exact values
    (2^-4 in the query, a multiple of 2^-16 in each decoy) that set the true gap s(b_t) - s(decoy) to GAPS.  With the query's
    halves parallel to b_t and to the decoys the inversion is 4 delta |b_t||b_d| against a margin of 2.02e-3 sqrt(2) |b_t|
    max|b|: 0.65 of the margin at |b_t| = max|b|, a little less here, where the planted norms stay below the ordinary
    rows' 1."""
    rng = np.random.default_rng(seed)
    a, b = descriptor_sets(na, nb, seed)
    q_rows = np.sort(rng.choice(na, n_rows, replace=False))
    # b rows: one per 16-row group; a query's five planted rows go round the four splits of LF_MKD_MATCH_SPLITS=4
    per_split = nb // 16 // 4
    free = [list(s * per_split + rng.permutation(per_split)) for s in range(4)]
    planted = []
    for j, q in enumerate(q_rows):
        rows = np.array([free[(j + r) % 4].pop() * 16 + rng.integers(0, 16) for r in range(1 + N_DECOYS)])
        t_row = rows[rng.integers(0, 1 + N_DECOYS)]
        d_rows = rows[rows != t_row]
        u = _moved(_grid(rng, 63, 0.97), +1.0)
        gv = _grid(rng, 64, 0.96)
        # the decoys' half is brought to within 3e-4 of the true best's in squared norm, one mantissa step (3e-5) at a time,
        # so that the spare dimension's values stay below 2^-5, where the f16 grid is 2^-16 or finer
        for _ in range(100000):
            diff = _sq(u) - 5e-5 - _sq(_moved(gv, -1.0))
            if abs(diff) < 3e-4:
                break
            i = rng.choice(np.flatnonzero(gv[1] == -3))
            gv[0][i] = min(47, max(1, gv[0][i] + (1 if diff > 0 else -1)))
        v = _moved(gv, -1.0)
        qa = np.zeros(128, np.float32)
        qa[:63], qa[63], qa[64:] = u, 2.0 ** -4, v
        bt = np.zeros(128, np.float32)
        bt[:63] = u
        s_t = float(exact(qa[None], bt[None])[0, 0])
        a[q], b[t_row] = qa, bt
        s_v = _sq(v)
        for d, gap in zip(d_rows, rng.permutation(GAPS)):
            bd = np.zeros(128, np.float32)
            bd[64:] = v
            bd[63] = np.round((s_t - gap - s_v) * 2.0 ** 4 * 2.0 ** 16) / 2.0 ** 16      # f16-exact: below 2^-5 in magnitude
            b[d] = bd
        planted.append((int(q), int(t_row), [int(d) for d in d_rows]))
    return a, b, None, None, {"name": "margin_inversion", "planted": planted, "splits": 4, "ratio": 0.0, "overflowed": 0}


def check_margin_inversion(case, lo_cap=0.55, hi_cap=0.9):
    """-> the inversion, as a share of the margin, of every planted query"""
    a, b, _, _, what = case
    s, st, m = exact(a, b), screen(a, b), margin(a, b)
    bn = norms(b)
    shares = []
    for q, t, ds in what["planted"]:
        assert len(ds) >= 3
        assert np.array_equal(b[t].astype(np.float16).astype(np.float32) != b[t], b[t] != 0) and not b[t, 64:].any()
        assert all(not b[d, :63].any() for d in ds)
        assert bn[[t] + ds].max() < bn.max(), "the planted rows do not set the largest norm"
        assert len({r // 16 for r in [t] + ds}) == 1 + len(ds), "one planted row per 16-row group"
        assert len(set(split_of([t] + ds, len(b), what["splits"]))) > 1, "more than one split"
        gaps = s[q, t] - s[q, ds]
        assert gaps.min() >= 1e-5 and gaps.max() <= 1e-4, (q, gaps)
        assert int(np.argmax(s[q])) == t, "b_t is the true best"
        assert float(np.abs(b[ds, 63]).max()) < 2.0 ** -5 and np.array_equal(b[ds, 63].astype(np.float16).astype(np.float32), b[ds, 63])
        u = np.sort(st[q])[-2]
        assert set(np.argsort(st[q])[-2:].tolist()) <= set(ds), "the screen's top two are decoys"
        share = (u - st[q, t]) / m[q]
        assert lo_cap <= share <= hi_cap, (q, share)
        shares.append(float(share))
    return shares


# ---- (b) the splits' shared floor ---------------------------------------------------------------------------------------

def floor_mixup(stride=1, seed=41):
    """192 a rows that alternate, every `stride` rows, between HIGH (every high row has eight candidates near 0.95 early in
    split 0, so the floor its splits share is ~0.95 from the first exchange on) and LOW (best ~0.10, second ~0.09, every
    other similarity below 0.02).  A floor that reaches the wrong row -- the neighbour in the sub-tile (stride 1), the same
    lane's next sub-tile (16), another wave (64) -- removes the low row's two candidates, which sit in splits 1 .. 3 at
    stages 3 and 7, after the floors have been taken.  nb = 2048, LF_MKD_MATCH_SPLITS=4: 512 rows = 8 stages per split.
    The low rows own one axis each of a 96-dimensional subspace, everything else lives in the other 32 dimensions."""
    rng = np.random.default_rng(seed)
    na, nb, splits = 192, 2048, 4
    basis, _ = np.linalg.qr(rng.normal(size=(128, 128)))
    low_axes, hi_sub = basis[:, :96].T, basis[:, 96:].T             # [96, 128], [32, 128]

    def in_hi(n, scale=1.0):
        x = rng.normal(size=(n, 32))
        return scale * (x / np.linalg.norm(x, axis=1, keepdims=True)) @ hi_sub

    high = (np.arange(na) // stride) % 2 == 0
    centre = in_hi(1)
    a = np.zeros((na, 128))
    a[high] = unit(centre + in_hi(int(high.sum()), 0.3))
    a[~high] = low_axes[: int((~high).sum())]
    b = unit(in_hi(nb) + 0.01 * rng.normal(size=(nb, 96)) @ low_axes / np.sqrt(96)).astype(np.float64)
    raisers = np.array([3, 9, 18, 23, 36, 41, 54, 60])             # split 0, stage 0: two per lane group
    b[raisers] = unit(centre + in_hi(len(raisers), 0.02))
    # per split 1 .. 3: stage 0-1 = the high rows' best, stage 3 = a low candidate, stage 7 = a low candidate and the high
    # rows' second
    free = {(s, st): list(512 * s + 64 * st + rng.permutation(64 if st else 128)) for s in (1, 2, 3) for st in (0, 3, 6, 7)}
    plan = {}
    for j, i in enumerate(np.flatnonzero(high)):
        s2 = 1 + (j + 1) % 3
        late = free[(s2, 7)] if len(free[(s2, 7)]) > 32 else free[(s2, 6)]
        r1, r2 = free[(1 + j % 3, 0)].pop(), late.pop()
        b[r1], b[r2] = unit(a[i:i + 1] + in_hi(1, 0.08))[0], unit(a[i:i + 1] + in_hi(1, 0.16))[0]
        plan[int(i)] = (int(r1), int(r2))
    for j, i in enumerate(np.flatnonzero(~high)):
        r1, r2 = free[(1 + j % 3, 3)].pop(), free[(1 + (j + 1) % 3, 7)].pop()
        if j % 2:
            r1, r2 = r2, r1                                         # the best is the late one for every other row
        b[r1] = 0.10 * a[i] + np.sqrt(1 - 0.10 ** 2) * in_hi(1)[0]
        b[r2] = 0.09 * a[i] + np.sqrt(1 - 0.09 ** 2) * in_hi(1)[0]
        plan[int(i)] = (int(r1), int(r2))
    return a.astype(np.float32), b.astype(np.float32), None, None, {
        "name": f"floor_mixup stride {stride}", "high": high, "plan": plan, "raisers": raisers, "stride": stride,
        "splits": splits, "ratio": 0.8, "overflowed": 0}


def check_floor_mixup(case):
    a, b, _, _, what = case
    high, stride, splits = what["high"], what["stride"], what["splits"]
    na, nb = len(a), len(b)
    assert na == 192 and nb == 2048
    s, st, m = exact(a, b), screen(a, b), margin(a, b)
    idx, s1, s2 = top2(s)
    for i in range(na):
        other = i + stride if i + stride < na else i - stride
        assert high[i] != high[other], "neighbours at the stride differ in kind"
        r1, r2 = what["plan"][i]
        assert idx[i] == r1 and s2[i] == s[i, r2], "the planted rows are the row's two best"
        assert s1[i] - s2[i] > 2 * m[i] and s2[i] - np.sort(s[i])[-3] > 2 * m[i], "and clear of each other and the rest"
        assert split_of(r1, nb, splits) != split_of(r2, nb, splits)
    # the floor the high rows publish at stage 2 of split 0 (their second best of stages 0-1, less the margin)
    early = np.sort(st[:, :2 * STAGE], axis=1)[:, -2] - m
    assert (split_of(what["raisers"], nb, splits) == 0).all() and (stage_of(what["raisers"], nb, splits) < 2).all()
    assert (early[high] > 0.9).all()
    for i in np.flatnonzero(~high):
        r = np.array(what["plan"][int(i)])
        assert (split_of(r, nb, splits) != 0).all() and (stage_of(r, nb, splits) >= 3).all()
        assert sorted(stage_of(r, nb, splits).tolist()) == [3, 7]
        assert 0.05 < s2[i] < s1[i] < 0.15 and st[i, r].max() + m[i] < early[high].min() - 0.5, "a neighbour's floor removes them"
    for i in np.flatnonzero(high):
        r = np.array(what["plan"][int(i)])
        assert st[i, r].min() > early[i] + m[i], "a row's own floor keeps its two best"
        assert sorted(stage_of(r, nb, splits).tolist())[0] < 2 and sorted(stage_of(r, nb, splits).tolist())[1] >= 6
    return float(early[high].min())


# ---- (c) the record ring -----------------------------------------------------------------------------------------------

def ring_ladder(k, tight, descending=False, seed=51):
    """k near-copies of one query in the b rows of ONE stream -- rows 16 m + 0 .. 3 (lane group 0) of split 0, from the
    split's first row on -- with ascending similarity (descending: the order reversed); every other b row is a random
    unit vector (similarity below 0.5).
    tight: the k values lie within a quarter of the margin: every one is recorded, 64 fill the ring exactly (no row is
    redone), the 65th pushes one out that verify would have re-scored (the row is redone).
    not tight: steps of 2.5 margins: every candidate is a new best and recorded, the ring wraps and what it loses lies far
    below what verify keeps: nothing is redone and the result is exact."""
    rng = np.random.default_rng(seed + k)
    na, nb, splits, q_row = 40, 2048, 2, 21
    a = unit(rng.normal(size=(na, 128)))
    b = unit(rng.normal(size=(nb, 128))).astype(np.float64)
    q = a[q_row].astype(np.float64)
    m = float(margin(a, b)[q_row])
    sims = 0.95 - (m / 5) * np.arange(k)[::-1] / max(k - 1, 1) if tight else 0.95 - 2.5 * m * np.arange(k)[::-1]
    if descending:
        sims = sims[::-1]
    rows = np.array([16 * (j // 4) + j % 4 for j in range(k)])
    r = rng.normal(size=(k, 128))
    r -= np.outer(r @ q, q) / (q @ q)
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    b[rows] = (sims[:, None] * q[None, :] / np.sqrt(q @ q) + np.sqrt(1 - sims ** 2)[:, None] * r) * 0.999
    over = 1 if tight and k > REC_CAP else 0
    return a, b.astype(np.float32), None, None, {
        "name": f"ring_ladder k {k} {'tight' if tight else 'steps'}{' descending' if descending else ''}", "rows": rows,
        "query": q_row, "tight": tight, "splits": splits, "ratio": 0.0, "overflowed": over}


def check_ring_ladder(case):
    a, b, _, _, what = case
    q, rows, nb, splits = what["query"], what["rows"], len(b), what["splits"]
    s, st, m = exact(a, b)[q], screen(a, b)[q], float(margin(a, b)[q])
    assert (split_of(rows, nb, splits) == 0).all() and ((rows % 16) // 4 == 0).all() and rows[0] == 0
    assert len(np.unique(rows)) == len(rows) and (np.diff(rows) > 0).all()
    assert len(rows) == 4 * (len(rows) // 4) + len(rows) % 4 and rows[-1] == 16 * ((len(rows) - 1) // 4) + (len(rows) - 1) % 4
    ladder, lt = s[rows], st[rows]
    rest = np.ones(nb, bool)
    rest[rows] = False
    assert s[rest].max() < 0.5 and st[rest].max() + m < np.sort(lt)[-2] - m, "no background row near the ladder's top"
    if what["tight"]:
        assert ladder.max() - ladder.min() < m / 4 and lt.max() - lt.min() < m / 2, "all k within the margin of each other"
        assert (np.abs(np.diff(ladder)) > 1e-6).all(), "and distinct in f32"
    else:
        up = np.diff(ladder) if ladder[-1] > ladder[0] else -np.diff(ladder)
        assert (np.abs(up - 2.5 * m) < 0.05 * m).all() and (np.abs(np.diff(lt)) > 2 * m).all()
        # what the ring loses (all but the last 64) lies far below what verify keeps
        assert len(rows) > REC_CAP and lt[: len(rows) - REC_CAP].max() < np.sort(lt)[-2] - 2 * m
    return m


# ---- (d) the fallback scan with exclusion ranges -------------------------------------------------------------------------

def crowded_with_exclusion(n_over=4, seed=5):
    """600 near-duplicates of one centre in b rows 100 .. 699 (LF_MKD_MATCH_SPLITS=4 of 2648 rows: split 0 ends at row 672,
    which is also a tile edge) and n_over a rows at the centre: each of their streams sees more than 64 candidates within
    the margin, so the rows are redone by the three-term scan -- alone (n_over = 4, among 300 ordinary rows: match_split_rows
    gathers their exclusion ranges) or with everybody (n_over = 16400 > 16384).  Every crowded row's range holds its true
    best (a copy of the row) and part of the cluster, and straddles row 672."""
    rng = np.random.default_rng(seed)
    centre = unit(rng.normal(size=(1, 128)))
    nb = 600 + 2048
    b = unit(rng.normal(size=(nb, 128)))
    b[100:700] = unit(centre + 2e-4 * rng.normal(size=(600, 128)))
    crowded = unit(centre + 1e-4 * rng.normal(size=(n_over, 128)))
    few = n_over <= 16384
    # (the ordinary rows are orthogonal to the centre: the cluster is nowhere near their best, they stay in their rings)
    plain = rng.normal(size=(300, 128))
    plain -= (plain @ centre.T.astype(np.float64)) * centre
    a = np.concatenate([crowded, unit(plain)]) if few else crowded
    na = len(a)
    lo = rng.integers(0, nb - 40, na).astype(np.uint32)
    hi = lo + rng.integers(0, 40, na).astype(np.uint32)
    hi[rng.random(na) < 0.3] = 0                                   # some rows exclude nothing
    lo[:n_over] = 672 - rng.integers(1, 40, n_over)
    hi[:n_over] = 672 + rng.integers(1, 28, n_over)
    lo[0], hi[0] = 641, 673                                          # one row and one whole tile either side of the edge
    if few:
        for i in range(n_over):
            b[int(rng.integers(lo[i], hi[i]))] = a[i]                # the true best: inside the range
    order = rng.permutation(na) if few else np.arange(na)            # the crowded rows anywhere among the others
    a, lo, hi = a[order], lo[order], hi[order]
    rows = np.flatnonzero(order < n_over)
    return a, b, lo, hi, {"name": f"crowded_with_exclusion {n_over}", "crowded": rows, "splits": 4, "ratio": 0.8,
                          "overflowed": (n_over, n_over) if few else (16385, n_over)}


def check_crowded_with_exclusion(case):
    a, b, lo, hi, what = case
    rows, nb, splits = what["crowded"], len(b), what["splits"]
    rows = rows[:64]                                                  # (a sample of the "all" case)
    s, st, m = exact(a[rows], b), screen(a[rows], b), margin(a, b)[rows]
    edge = int(np.flatnonzero(np.diff(split_of(np.arange(nb), nb, splits)))[0]) + 1
    assert edge % TILE == 0
    l, h = lo[rows].astype(np.int64), hi[rows].astype(np.int64)
    assert (l < edge).all() and (h > edge).all(), "every range straddles the split edge, which is a tile edge"
    assert (l >= 100).all() and (h - l < 100).all(), "and cuts only part of the cluster"
    if len(a) < 16384:
        assert ((np.argmax(s, axis=1) >= l) & (np.argmax(s, axis=1) < h)).all(), "the true best is cut out"
    kept = mask_excluded(st, lo[rows], hi[rows])
    u = np.sort(kept, axis=1)[:, -2]
    # the candidates within the margin of the second best, per stream of split 0: more than the ring holds
    for j in range(len(rows)):
        near = np.flatnonzero(kept[j] >= u[j] - m[j])
        near = near[split_of(near, nb, splits) == 0]
        per_stream = np.bincount((near % 16) // 4, minlength=4)
        assert per_stream.max() > REC_CAP, (j, per_stream)
    others = np.setdiff1d(np.arange(len(a)), what["crowded"])
    if len(others):
        so = mask_excluded(screen(a[others], b), lo[others], hi[others])
        uo = np.sort(so, axis=1)[:, -2]
        mo = margin(a, b)[others]
        assert (so[:, 100:700].max(axis=1) < uo - 3 * mo).all(), "the cluster is far below an ordinary row's second best"
        assert ((so >= (uo - mo)[:, None]).sum(axis=1) < REC_CAP // 2).all(), "the ordinary rows stay in their rings"
    return edge


# ---- (e) negative similarities, zero rows, duplicates --------------------------------------------------------------------

def signs_and_zeros(seed=61):
    """na = 77, nb = 1003 (neither a multiple of 16 or 32), LF_MKD_MATCH_SPLITS=3 (352 rows per split).  b rows have only
    positive elements, so the a rows that are NEGATED copies of b rows have no positive similarity; half of them exclude the
    all-zero b row 500 and keep a negative best, the others find it (similarity -0).  a row 40 is all zero: every candidate
    ties, the highest index wins and the row is redone by the scan.  b rows 100 and 900 (splits 0 and 2) are identical
    and a row 5's best."""
    rng = np.random.default_rng(seed)
    na, nb = 77, 1003
    b = unit(np.abs(rng.normal(size=(nb, 128))))
    a = unit(b[rng.integers(0, nb, na)] + 0.05 * rng.normal(size=(na, 128)))
    b[500] = 0.0
    b[900] = b[100]
    a[5] = unit(b[100:101] + 0.02 * rng.normal(size=(1, 128)))[0]
    negated = np.arange(10, 22)
    a[negated] = -b[rng.choice(np.setdiff1d(np.arange(nb), [500]), len(negated), replace=False)]
    a[40] = 0.0
    lo, hi = np.zeros(na, np.uint32), np.zeros(na, np.uint32)
    lo[negated[::2]], hi[negated[::2]] = 500, 501
    return a, b, lo, hi, {"name": "signs_and_zeros", "negated": negated, "zero_a": 40, "zero_b": 500, "dup": (5, 100, 900),
                          "splits": 3, "overflowed": (1, 1)}


def check_signs_and_zeros(case):
    a, b, lo, hi, what = case
    na, nb = len(a), len(b)
    assert na % 16 and nb % 16 and nb % 32
    s = mask_excluded(exact(a, b), lo, hi)
    neg = what["negated"]
    assert (s[neg] <= 0).all() and (s[neg[::2]].max(axis=1) < -0.1).all() and (s[neg[1::2]].max(axis=1) == 0).all()
    assert not a[what["zero_a"]].any() and not b[what["zero_b"]].any()
    q, d0, d1 = what["dup"]
    assert np.array_equal(b[d0], b[d1]) and split_of(d0, nb, what["splits"]) != split_of(d1, nb, what["splits"])
    assert int(np.argmax(s[q])) in (d0, d1) and s[q, d0] == np.sort(s[q])[-2]
    return True


# ---- (f) rows far from unit norm --------------------------------------------------------------------------------------

SCALES = [(1e-3, 1.0), (3e-5, 2e-4), (50.0, 0.01), (300.0, 120.0)]


def scaled(scale_a, scale_b, na=700, nb=1500, seed=11):
    """descriptor_sets scaled as test_match_of_unnormalised_rows scales them (f16 subnormals included), and one b row of 8
    times the others' largest norm along minus the first axis, where every query is positive: it sets max|b|, and so every margin, and is
    nobody's best."""
    a, b = descriptor_sets(na, nb, seed)
    a[:, 0], b[:, 0] = np.abs(a[:, 0]), np.abs(b[:, 0])           # element 0 positive everywhere: the outlier's axis
    rng = np.random.default_rng(seed + 1)
    a = (a * scale_a * rng.uniform(0.5, 2.0, (na, 1))).astype(np.float32)
    b = (b * scale_b * rng.uniform(0.5, 2.0, (nb, 1))).astype(np.float32)
    out = nb // 2 + 27
    b[out] = 0.0
    b[out, 0] = -8 * 2.0 * scale_b
    return a, b, None, None, {"name": f"scaled {scale_a:g} x {scale_b:g}", "outlier": out, "splits": None, "ratio": 0.0,
                              "overflowed": 0}


def check_scaled(case):
    a, b, _, _, what = case
    out = what["outlier"]
    assert np.isfinite(a).all() and np.isfinite(b).all() and max(np.abs(a).max(), np.abs(b).max()) < 65504
    bn = norms(b)
    assert int(np.argmax(bn)) == out and bn[out] >= 7.9 * np.delete(bn, out).max()
    idx, s1, s2 = top2(exact(a, b))
    assert (idx != out).all() and (exact(a, b)[:, out] < s2).all(), "the outlier is nobody's best or second"
    return float(bn[out])
