"""Pools whose byte offsets pass 2^31 and 2^32, described sparsely: a pool is `total` rows that all hold one background row
(or seeded noise) except a few hundred PLANTED rows around the byte marks, at row 0 and at the end.  Only the planted rows
ever exist on the host; the expected result of a call is one of the suite's numpy restatements run on the planted rows alone
(plus one background row where every row is a candidate), with the indices mapped back.

The top byte mark B is a parameter of every builder: the marks of a pool are B / 2 and B.  At B = 2^32 that is the 2 GiB and
the 4 GiB mark of a 4.3 GB pool; at B = 2^16 the same pool has a few hundred rows, is materialised on the host
(SparsePool.to_numpy) and goes through the full restatement -- tests/test_big_pool_cases.py proves there that the sparse
expectation IS the full one, and that a pool read through a wrapped address (row r mod B / R) gives another result."""
import numpy as np

import fundamental_cases as fcases
import homography_cases as hcases
import match_guided_cases as mgcases
import match_pairs_cases as pcases
import q8_cases as qcases
import q8_edges_cases as ecases
import q8_grouped_cases as gcases
import q8_guided_cases as q8g
import q8_knn_cases as kcases
import q8_pairs_cases as pq
import tracks_cases as tcases

SMALL = 1 << 16
MARKS = (SMALL, 1 << 31, 1 << 32)           # the values of B the GPU tests run
SENTINEL = -7
RATIO = qcases.RATIO
NA_BIG_B, NB_BIG_A = 96, 64                 # the small side's rows when b / a is the big side
GROUP_RUN = 3                               # critical rows per group of the grouped form


def marks(B):
    return (B // 2, B)


def tail_rows(B):
    """rows behind the top mark: ragged, not a multiple of any tile"""
    return 4096 + 37 if B >= 1 << 31 else 64 + 37


def total_rows(B, R):
    return -(-B // R) + tail_rows(B)


def critical_rows(B, R, total, seed, n_seeded=20, spread=40):
    """sorted rows of a pool of `total` rows of R bytes: the rows in front of, at and behind either mark (floor and ceil where
    the mark falls inside a row), n_seeded seeded rows within +-spread of either mark, row 0 and the last row"""
    rng = np.random.default_rng(seed)
    rows = {0, total - 1}
    for m in marks(B):
        lo, hi = m // R, -(-m // R)
        rows |= {lo - 1, lo, lo + 1, hi, hi + 1}
        rows |= set((lo + rng.integers(-spread, spread + 1, n_seeded)).tolist())
    return np.array(sorted(r for r in rows if 0 <= r < total), np.int64)


class SparsePool:
    """`total` rows of `width` elements: `fill_row` everywhere (a background pool), or seeded noise that no expected value
    depends on (fill_row None), except the planted blocks"""

    def __init__(self, total, width, dtype, fill_row=None):
        self.total, self.width, self.dtype = int(total), int(width), np.dtype(dtype)
        self.fill_row = None if fill_row is None else np.ascontiguousarray(fill_row, self.dtype).reshape(width)
        self.blocks = []                    # [(first row, rows [n, width])], disjoint

    def plant(self, first, rows):
        rows = np.ascontiguousarray(rows, self.dtype).reshape(-1, self.width)
        first = int(first)
        assert 0 <= first and first + len(rows) <= self.total, (first, len(rows), self.total)
        for f, r in self.blocks:
            assert first + len(rows) <= f or f + len(r) <= first, "planted blocks overlap"
        self.blocks.append((first, rows))
        self.blocks.sort(key=lambda b: b[0])

    def plant_rows(self, index, rows):
        """single rows at the sorted positions `index`, consecutive ones as one block"""
        index = np.asarray(index, np.int64)
        cut = np.flatnonzero(np.diff(index) != 1) + 1
        for i, r in zip(np.split(index, cut), np.split(np.asarray(rows), cut)):
            self.plant(i[0], r)

    def take(self, first, n):
        """the host rows [first, first + n): all of them must be planted, within one block"""
        first, n = int(first), int(n)
        if n == 0:
            return np.zeros((0, self.width), self.dtype)
        for f, r in self.blocks:
            if f <= first and first + n <= f + len(r):
                return r[first - f:first - f + n]
        raise AssertionError(("rows not planted", first, n))

    def planted(self):
        """(row indices, rows) of everything planted, in row order"""
        idx = np.concatenate([np.arange(f, f + len(r)) for f, r in self.blocks])
        return idx.astype(np.int64), np.concatenate([r for _, r in self.blocks])

    def to_numpy(self, seed=99):
        """the whole pool on the host -- for the small mark only"""
        assert self.total * self.width * self.dtype.itemsize <= 1 << 26, "a pool of this size never exists on the host"
        if self.fill_row is not None:
            full = np.tile(self.fill_row, (self.total, 1))
        elif self.dtype == np.uint8:
            full = np.random.default_rng(seed).integers(1, 256, (self.total, self.width)).astype(np.uint8)
        else:
            full = (0.09 * np.random.default_rng(seed).normal(size=(self.total, self.width))).astype(self.dtype)
        for f, r in self.blocks:
            full[f:f + len(r)] = r
        return full


def wrapped(full, B, R):
    """what a 32-bit byte offset would read of a host pool: row r mod B / R"""
    return full[np.arange(len(full)) % (B // R)]


# --- single-pair calls over q8 rows: one side is the big pool, every b row a candidate --------------------------------
class SingleQ8:
    """The big side: total_rows(B, 128) rows, the background row except at the critical rows.  Planted rows are unit(c + g_i)
    for one common direction c, the background is close to -c, and the small side's rows are noisy copies of planted rows: a
    query's own row scores about 0.95 (x 2^16), any other planted row about 0.5, the background about -0.5 -- so the
    background never reaches an output, which background_below() asserts on the reference and does not assume.  The rows in
    front of and at either mark are one row twice: a tie across the mark, decided by the index."""

    def __init__(self, B, seed):
        self.B, self.total = B, total_rows(B, 128)
        self.crit = critical_rows(B, 128, self.total, seed)
        P = len(self.crit)
        rng = np.random.default_rng(seed + 1)
        c = pcases.unit(rng.normal(size=(1, 128)))
        f = pcases.unit(c + pcases.unit(rng.normal(size=(P, 128))))
        first = []
        for m in marks(B):
            i = int(np.searchsorted(self.crit, m // 128 - 1))
            assert self.crit[i] == m // 128 - 1 and self.crit[i + 1] == m // 128 and self.crit[i + 2] == m // 128 + 1
            f[i + 1] = f[i]
            first += [i, i + 1, i + 2]
        first += [0, P - 1]
        self.planted = qcases.quantize(f)
        self.background = qcases.quantize(pcases.unit(-c + 0.3 * pcases.unit(rng.normal(size=(1, 128)))))[0]
        # the small side: the rows at the marks, row 0 and the last row first, then the others in turn
        src = np.array(first + [i for i in range(P) if i not in first])
        n = max(NA_BIG_B, NB_BIG_A)
        src = src[np.arange(n) % P]
        self.small = qcases.quantize(pcases.unit(f[src] + 0.03 * rng.normal(size=(n, 128))))
        self.pool = SparsePool(self.total, 128, np.uint8, self.background)
        self.pool.plant_rows(self.crit, self.planted)

    # the compressed problem: the planted rows in row order, then ONE background row
    def compressed(self):
        return np.concatenate([self.planted, self.background[None]])

    def to_rows(self, index):
        """compressed b indices -> pool rows; the background row (index P) must not occur"""
        index = np.asarray(index, np.int64)
        assert (index < len(self.crit)).all(), "a background row reached an output"
        return np.where(index >= 0, self.crit[np.maximum(index, 0)], -1).astype(np.int32)

    def background_below(self, a, last):
        """the condition the compression rests on: every query's last reported candidate scores strictly above the background"""
        s_bg = qcases.similarities(a, self.background[None])[:, 0]
        assert (np.asarray(last, np.int64) > s_bg).all(), "a background row would reach an output"

    def ranges(self):
        """(lo, hi, lo_c, hi_c): exclusion ranges [lo, hi) of pool rows that start and end at critical rows and take up to half
        of the planted rows away (every eighth: nothing), and the same ranges over the compressed problem's rows"""
        P, na = len(self.crit), NA_BIG_B
        rng = np.random.default_rng(self.B % 1000 + 7)
        x = rng.integers(0, P - 1, na)
        y = np.minimum(x + rng.integers(1, P // 2, na), P - 1)
        y[::8] = x[::8]
        lo, hi = self.crit[x], self.crit[y]
        assert (self.total - (hi - lo) - (P - (y - x)) > 0).all(), "a background row must stay a candidate"
        return lo.astype(np.uint32), hi.astype(np.uint32), x, y

    def groups_of_planted(self):
        """the grouped form's ids: row j is in group (critical rows <= j) // GROUP_RUN, so the ids change at critical rows"""
        return ((np.arange(len(self.crit)) + 1) // GROUP_RUN).astype(np.uint32)

    def groups_full(self):
        return (np.searchsorted(self.crit, np.arange(self.total), side="right") // GROUP_RUN).astype(np.uint32)

    # --- big b: the small side asks, the pool is searched -----------------------------------------------------------
    def expect_match_big_b(self, ratio=RATIO, ranges=False):
        a = self.small[:NA_BIG_B]
        lo = hi = None
        if ranges:
            _, _, lo, hi = self.ranges()
        m, best, second = qcases.match_q8(a, self.compressed(), ratio, lo, hi)
        self.background_below(a, second)
        return self.to_rows(m), best, second

    def expect_knn_big_b(self, k):
        a = self.small[:NA_BIG_B]
        index, score = kcases.knn_q8(a, self.compressed(), k)
        self.background_below(a, score[:, -1])
        return self.to_rows(index), score

    def expect_grouped_big_b(self, ratio=RATIO):
        a = self.small[:NA_BIG_B]
        groups = np.concatenate([self.groups_of_planted(), np.array([0xFFFFFFFF], np.uint32)])   # the background: a group of its own
        m, best, rival = gcases.match_q8_grouped(a, self.compressed(), groups, ratio)
        self.background_below(a, rival)
        return self.to_rows(m), best, rival

    # --- big a: the pool asks, the small side is searched; every background row gets one scalar tuple ---------------
    def groups_small(self):
        return gcases.runs(NB_BIG_A, GROUP_RUN)

    def expect_big_a(self, form, k=None, ratio=RATIO):
        """(outputs of the planted rows, outputs of ONE background row) of `form` in "match", "knn", "grouped" """
        b = self.small[:NB_BIG_A]
        rows = np.concatenate([self.planted, self.background[None]])
        if form == "match":
            out = qcases.match_q8(rows, b, ratio)
        elif form == "knn":
            out = kcases.knn_q8(rows, b, k)
        else:
            out = gcases.match_q8_grouped(rows, b, self.groups_small(), ratio)
        return [o[:-1] for o in out], [o[-1] for o in out]


def expand_big_a(single, planted_out, background_out):
    """the sparse expectation of a big-a call as full arrays (small mark only)"""
    full = []
    for p, bg in zip(planted_out, background_out):
        x = np.empty((single.total,) + p.shape[1:], p.dtype)
        x[:] = bg
        x[single.crit] = p
        full.append(x)
    return full


# --- the f32 matcher: one side is a far pool of f32 rows ------------------------------------------------------------------
NB_BIG_A_F32 = 384
SCREEN_ROWS = 16384             # the screen form's smallest na
GAP_F32 = 1e-2                  # the header puts every form within about 1e-7 of an f32 dot product: five orders of margin


class SingleF32:
    """SingleQ8 for lf_mkd_match_device: total_rows(B, 512) f32 rows, the background row except at the critical rows; the same
    geometry (own row about 0.95, other planted rows about 0.5, the background about -0.5), the same tie across either mark.
    The expected values come from the caller's reference (oracle.match, the screen form's twin) run on compressed()."""

    def __init__(self, B, seed):
        self.B, self.total = B, total_rows(B, 512)
        crit = critical_rows(B, 512, self.total, seed)
        # every critical row's neighbour r ^ 1 is planted too.  A stream of the screen form (one query, one of its four lanes,
        # one b split) reads b rows in aligned groups of four and keeps 64 records; until it has seen TWO rows above the
        # background its threshold is the background's score, every one of the identical background rows is a candidate, and
        # the ring wraps over the record of a planted row seen before them -- the fallback scan then redoes the query
        # (csrc/mkd_match.hip, "every value is a candidate").  With its neighbour beside it no planted row is alone in a
        # stream, so the screen form itself, not the fallback, decides every query.
        self.crit = np.unique(np.concatenate([crit, crit ^ 1]))
        self.crit = self.crit[self.crit < self.total]
        P = len(self.crit)
        rng = np.random.default_rng(seed + 1)
        c = pcases.unit(rng.normal(size=(1, 128)))
        f = pcases.unit(c + pcases.unit(rng.normal(size=(P, 128))))
        first = []
        for m in marks(B):
            i = int(np.searchsorted(self.crit, m // 512 - 1))
            assert self.crit[i] == m // 512 - 1 and self.crit[i + 1] == m // 512 and self.crit[i + 2] == m // 512 + 1
            f[i + 1] = f[i]
            first += [i, i + 1, i + 2]
        first += [0, P - 1]
        self.planted = f
        self.background = pcases.unit(-c + 0.3 * pcases.unit(rng.normal(size=(1, 128))))[0]
        src = np.array(first + [i for i in range(P) if i not in first])
        self.queries = pcases.unit(f[src[np.arange(NA_BIG_B) % P]] + 0.03 * rng.normal(size=(NA_BIG_B, 128)))
        src = src[np.arange(NB_BIG_A_F32) % P]
        self.small_b = pcases.unit(f[src] + 0.03 * rng.normal(size=(NB_BIG_A_F32, 128)))
        self.pool = SparsePool(self.total, 128, np.float32, self.background)
        self.pool.plant_rows(self.crit, f)

    def compressed(self):
        return np.ascontiguousarray(np.concatenate([self.planted, self.background[None]]))

    def a_rows(self, screen):
        """the small side of a big-b call: the 96 queries, for the screen form repeated to its smallest na"""
        return np.ascontiguousarray(self.queries[np.arange(SCREEN_ROWS) % NA_BIG_B]) if screen else self.queries

    def to_rows(self, index):
        index = np.asarray(index, np.int64)
        assert (index < len(self.crit)).all(), "a background row reached an output"
        return np.where(index >= 0, self.crit[np.maximum(index, 0)], -1).astype(np.int32)

    def background_below(self, a, second):
        """every query's second best scores at least GAP_F32 above the background (float64 of the f32 rows)"""
        s_bg = a.astype(np.float64) @ self.background.astype(np.float64)
        assert (np.asarray(second, np.float64) - s_bg >= GAP_F32).all(), "a background row would reach an output"

    def big_a_rows(self):
        """the rows of the big-a call's reference: the planted rows, then ONE background row"""
        return self.compressed()


# --- pooled calls over q8 rows: small images at the marks, at the end and near row 0 ------------------------------------
# rows of (the image ending at a mark, the one starting at it, the straddling image's rows in front of and from the mark on, the
# image ending at the total, the control) for a pool used as a / as b: around a 32-row tile, none a multiple of anything
SIZES = {"a": (37, 41, 19, 14, 33, 33), "b": (29, 35, 11, 23, 31, 36)}


def far_calls(B, R, total, sizes):
    """the offset lists of the calls over a far pool, one list a call: per mark an image ending exactly at it and one starting
    exactly at it (two pairs), then one straddling it; one ending at the total; one control at row 3"""
    before, after, left, right, last, control = sizes
    calls = []
    for m in marks(B):
        c = m // R
        calls += [[c - before, c, c + after], [c - left, c + right]]
    calls += [[total - last, total], [3, 3 + control]]
    return calls


def near_calls(shape, sizes, lead=5):
    """calls of the same shape over a compact pool: the images back to back behind `lead` rows; returns (calls, total)"""
    calls, pos, k = [], lead, 0
    for n_pairs in shape:
        o = [pos]
        for _ in range(n_pairs):
            pos += sizes[k % len(sizes)] + k
            k += 1
            o.append(pos)
        calls.append(o)
    return calls, pos + 7


SIZES_F32 = {"a": (13, 15, 7, 6, 9, 9), "b": (11, 14, 5, 8, 10, 12)}      # (a mark of the small f32 pool is 64 rows from the next)


class Pooled:
    """Two pools of q8 rows (f32 rows with f32=True) and the calls (offsets_a, offsets_b) over them; far in "a", "b" or "both".
    Every image is a noisy view of one small scene, so matches survive the ratio test and the cross-check; the rest of a
    pool is noise.  guide = 0 / 1 (LF_MKD_GUIDE_HOMOGRAPHY / _FUNDAMENTAL): every pair also has keypoints and a model, those
    of match_guided_cases' pairs; the keypoints are per call (kps[call][side] = (first row, rows [n, 5])), written into pools
    of NaN rows in front of their call, because a straddling image shares its rows with the two images it straddles."""

    def __init__(self, B, far, seed, f32=False, guide=None):
        self.B, self.far, self.f32, self.guide = B, far, f32, guide
        self.R = R = 512 if f32 else 128
        rng = np.random.default_rng(seed)
        points = 24 if f32 else 50                                     # (the f32 images are smaller: a smaller scene)
        scene = pcases.unit(rng.normal(size=(points, 128)))
        rows = lambda n: pcases.unit(scene[rng.permutation(points)[:n]] + 0.03 * rng.normal(size=(n, 128)))
        self.view = rows if f32 else (lambda n: qcases.quantize(rows(n)))
        sizes = SIZES_F32 if f32 else SIZES
        total = total_rows(B, R)
        shape = [len(c) - 1 for c in far_calls(B, R, total, sizes["a"])]
        self.pools, self.offsets = {}, {}
        for side in "ab":
            if far in (side, "both"):
                calls, n = far_calls(B, R, total, sizes[side]), total
            else:
                calls, n = near_calls(shape, sizes[side])
            pool = SparsePool(n, 128, np.float32 if f32 else np.uint8)
            for c in sorted(calls, key=lambda c: c[0] - c[-1]):          # the widest first: a straddling image is a slice of
                if not any(f <= c[0] and c[-1] <= f + len(r) for f, r in pool.blocks):      # the two images it straddles
                    pool.plant(c[0], np.concatenate([self.view(c[p + 1] - c[p]) for p in range(len(c) - 1)]))
            self.pools[side], self.offsets[side] = pool, [np.array(c, np.uint64) for c in calls]
        self.calls = list(zip(self.offsets["a"], self.offsets["b"]))
        self.kps, self.models = [], []
        if guide is not None:
            for oa, ob in self.calls:
                ka, kb, models = [], [], []
                for p in range(len(oa) - 1):
                    a, b, m = (mgcases._pair_h if guide == 0 else mgcases._pair_f)(rng, int(oa[p + 1] - oa[p]), int(ob[p + 1] - ob[p]))
                    ka.append(mgcases._keypoints(a))
                    kb.append(mgcases._keypoints(b))
                    models.append(m)
                self.kps.append({"a": (int(oa[0]), np.concatenate(ka)), "b": (int(ob[0]), np.concatenate(kb))})
                self.models.append(np.ascontiguousarray(np.stack(models), np.float32))

    def pairs(self):
        """(call, pair of the call, first a row, a rows, first b row, b rows) of every pair"""
        for c, (oa, ob) in enumerate(self.calls):
            for p in range(len(oa) - 1):
                a0, na, b0, nb = int(oa[p]), int(oa[p + 1] - oa[p]), int(ob[p]), int(ob[p + 1] - ob[p])
                yield c, p, a0, self.pools["a"].take(a0, na), b0, self.pools["b"].take(b0, nb)

    def problems(self, thr):
        """the pairs as match_guided_cases.twin_masks takes them, in the order of pairs()"""
        out = []
        for c, p, a0, x, b0, y in self.pairs():
            ka, kb = self.kps[c]["a"], self.kps[c]["b"]
            out.append((self.guide, thr, self.models[c][p], ka[1][a0 - ka[0]:a0 - ka[0] + len(x), :2], kb[1][b0 - kb[0]:b0 - kb[0] + len(y), :2]))
        return out

    def expect_guided(self, masks, ratio=RATIO, mutual=False):
        """as expect(), over 8-bit rows under the twin's masks [(fwd, rev, _)] (in the order of pairs()): q8_guided_cases.decide"""
        calls = [{"ab": [], "ba": [], "best": [], "second": []} for _ in self.calls]
        for (c, p, a0, x, b0, y), (fwd, rev, _) in zip(self.pairs(), masks):
            ab, best, second = q8g.decide(x, y, fwd, ratio)
            ba = q8g.decide(y, x, rev, ratio)[0]
            if mutual:
                ab, ba = pcases.mutual(ab, ba, [0, len(x)], [0, len(y)])
            for name, first, v in (("ab", a0, ab), ("ba", b0, ba), ("best", a0, best), ("second", a0, second)):
                calls[c][name].append((first, v))
        return calls

    def expect(self, ratio=RATIO, mutual=False):
        """per call {"ab" / "ba" / "best" / "second": [(first entry, values)]}: per pair q8_pairs_cases.match_one on the pair's
        own host rows, both directions, and match_pairs_cases.mutual.  (Per call, because the straddling image's entries are
        also entries of the two images it straddles: the outputs are checked and reset after every call.)"""
        calls = []
        for oa, ob in self.calls:
            out = {"ab": [], "ba": [], "best": [], "second": []}
            for p in range(len(oa) - 1):
                a0, na, b0, nb = int(oa[p]), int(oa[p + 1] - oa[p]), int(ob[p]), int(ob[p + 1] - ob[p])
                x, y = self.pools["a"].take(a0, na), self.pools["b"].take(b0, nb)
                ab, best, second = pq.match_one(x, y, ratio)
                ba = pq.match_one(y, x, ratio)[0]
                if mutual:
                    ab, ba = pcases.mutual(ab, ba, [0, na], [0, nb])
                for name, first, v in (("ab", a0, ab), ("ba", b0, ba), ("best", a0, best), ("second", a0, second)):
                    out[name].append((first, v))
            calls.append(out)
        return calls


def expand(segments, n, fill=SENTINEL, dtype=np.int32):
    """[(first, values)] as a full array of n entries, `fill` everywhere else (small mark only)"""
    x = np.full(n, fill, dtype)
    for first, v in segments:
        x[first:first + len(v)] = v
    return x


# --- the edge calls: one shared pool, two sets of image offsets over the same rows -------------------------------------
def control_rows(B):
    """rows of the control image at row 3: the image of the long leading range"""
    return 500 if B >= 1 << 31 else 100


class EdgesQ8:
    """One far pool read through two image-offset arrays: side a has, per mark, the image ending at it and the one starting at
    it; side b the image straddling it; both have the 500-row control image at row 3, the image ending at the total and the
    gaps between them as images on no edge.  `long_range`: the a side's layout is not made from the ids -- the first edge's
    range is [0, B / 4 + 5) over the control image, so every later edge's entries lie B bytes into the int32 outputs."""

    def __init__(self, B, seed, long_range=False):
        self.B, self.total = B, total_rows(B, 128)
        rng = np.random.default_rng(seed)
        scene = pcases.unit(rng.normal(size=(600, 128)))
        view = lambda n: qcases.quantize(pcases.unit(scene[rng.permutation(600)[:n]] + 0.03 * rng.normal(size=(n, 128))))
        before, after, left, right, last, _ = SIZES["a"]
        c1, c2 = (m // 128 for m in marks(B))
        CONTROL = self.control = control_rows(B)
        assert 3 + CONTROL < c1 - before, "the mark is too small for the control image"
        self.pool = SparsePool(self.total, 128, np.uint8)
        for first, n in ((3, CONTROL), (c1 - before, before + after), (c2 - before, before + after), (self.total - last, last)):
            self.pool.plant(first, view(n))
        t = self.total
        self.io_a = np.array([3, 3 + CONTROL, c1 - before, c1, c1 + after, c2 - before, c2, c2 + after, t - last, t], np.int64)
        self.io_b = np.array([3, 3 + CONTROL, c1 - left, c1 + right, c2 - left, c2 + right, t - last, t], np.int64)
        # a: 0 control, 2 / 3 around the low mark, 5 / 6 around the top mark, 8 the end; b: 0 control, 2 / 4 straddling, 6 the end
        edges = [(0, 2), (2, 2), (3, 2), (5, 4), (6, 4), (8, 6), (2, 4), (6, 2), (8, 0), (3, 6), (6, 6), (9, 2), (2, 7)]
        self.ea = np.array([e[0] for e in edges], np.uint32)
        self.eb = np.array([e[1] for e in edges], np.uint32)
        self.la = ecases.edge_layout(self.io_a, t, self.ea)
        self.lb = ecases.edge_layout(self.io_b, t, self.eb)
        if long_range:
            self.la = self.la + np.uint64(B // 4 + 5 - CONTROL)          # (2^30 + 5 entries at B = 2^32)
            self.la[0] = 0
        self.cap_a, self.cap_b = int(self.la[-1]), int(self.lb[-1])

    def expect(self, ratio=RATIO, mutual=False):
        """as Pooled.expect, per edge over the two WHOLE images, at the layouts' entries"""
        out = {"ab": [], "ba": [], "best": [], "second": []}
        for e in range(len(self.ea)):
            a0, na = ecases.image_bounds(self.io_a, self.total, self.ea[e])
            b0, nb = ecases.image_bounds(self.io_b, self.total, self.eb[e])
            x, y = self.pool.take(a0, na), self.pool.take(b0, nb)
            ab, best, second = pq.match_one(x, y, ratio)
            ba = pq.match_one(y, x, ratio)[0]
            if mutual:
                ab, ba = pcases.mutual(ab, ba, [0, na], [0, nb])
            la, lb = int(self.la[e]), int(self.lb[e])
            assert int(self.la[e + 1]) - la >= na and int(self.lb[e + 1]) - lb == nb
            for name, first, v in (("ab", la, ab), ("ba", lb, ba), ("best", la, best), ("second", la, second)):
                out[name].append((first, v))
        return out


# --- gather and layout: rows of any width from a far pool into an edge layout whose rows pass the mark as well --------------
class Gather:
    """A noise pool of row_bytes-byte rows.  Two edge lists over two image-offset arrays, each led by a BALLAST image of about
    B / row_bytes rows that ends just below the top mark, so that the far images' destination rows lie around and beyond byte B
    of dst as their source rows lie around and beyond byte B of src.  The ballast itself spans the low mark on both sides and
    is compared on the device."""

    def __init__(self, B, row_bytes, seed):
        self.B, self.R, self.total = B, row_bytes, total_rows(B, row_bytes)
        rng = np.random.default_rng(seed)
        before, after, left, right, last, control = SIZES["a"]
        c, t = B // row_bytes, self.total
        self.pool = SparsePool(t, row_bytes, np.uint8)
        for first, n in ((3, 5), (c - 48, 48 + after), (t - last, last)):
            self.pool.plant(first, rng.integers(1, 256, (n, row_bytes)).astype(np.uint8))
        # (image offsets, edge images): image 1 is the ballast, [8, ...)
        self.lists = [
            (np.array([3, 8, c - 48, c - before, c, c + after, t - last, t], np.int64), np.array([1, 0, 3, 4, 6, 2, 9], np.uint32)),
            (np.array([3, 8, c - left, c + right, t], np.int64), np.array([1, 2, 0], np.uint32)),
        ]

    def layout(self, k):
        io, edge = self.lists[k]
        return ecases.edge_layout(io, self.total, edge)

    def expect(self, k):
        """(ballast (src first, dst first, rows), [(dst first, host rows)]) of list k"""
        io, edge = self.lists[k]
        lay = self.layout(k)
        first, n = ecases.image_bounds(io, self.total, 1)
        assert edge[0] == 1 and n > self.B // self.R - 64
        segs = []
        for e in range(1, len(edge)):
            f, m = ecases.image_bounds(io, self.total, edge[e])
            segs.append((int(lay[e]), self.pool.take(f, m)))
        return (first, 0, n), segs


# --- the quantiser over a far f32 pool ----------------------------------------------------------------------------------
class Quantize:
    """total_rows(B, 512) f32 rows: one background row, and at the critical rows random unit rows scaled up so that some
    elements clamp, the quantiser's edge values among them"""

    def __init__(self, B, seed):
        self.B, self.total = B, total_rows(B, 512)
        self.crit = critical_rows(B, 512, self.total, seed)
        rng = np.random.default_rng(seed + 1)
        rows = (pcases.unit(rng.normal(size=(len(self.crit), 128))) * rng.uniform(0.5, 6, (len(self.crit), 1))).astype(np.float32)
        edge = qcases.edge_values()
        i = int(np.searchsorted(self.crit, B // 512))
        rows[i - 1], rows[i] = edge[0], edge[1]
        self.rows = rows
        self.background = pcases.unit(rng.normal(size=(1, 128)))[0]
        self.pool = SparsePool(self.total, 128, np.float32, self.background)
        self.pool.plant_rows(self.crit, rows)

    def expect(self):
        return qcases.quantize(self.rows), qcases.quantize(self.background[None])[0]


# --- the verifiers: one pool of 20-byte keypoint rows, pairs around either mark ----------------------------------------------
VERIFY_HYPOTHESES = 64
B_SHIFT = 200                   # the b image of a pair lies this many rows from its a image, in the same pool


class Verify:
    """One keypoint pool of ceil(B / 20) + tail rows (214.8 M at B = 2^32) that serves as d_kps_a AND d_kps_b, a match array and
    a `verified` array of that length.  The a images are far_calls' (ending at, starting at and straddling either mark -- which
    falls inside a row here, so floor(B / 20) is used and the row holding the mark belongs to the image starting there -- the
    end of the pool, a control near row 0); the b image of each lies B_SHIFT rows further on (further back at the end of the
    pool).  Per call: keypoints, matches and the pairs' problems ((ka, kb, match) as the suite's twins take them: planted
    homographies / two-view scenes with outliers, b permuted, a few rows unmatched).  The pool is NaN outside the call."""

    def __init__(self, B, kind, seed):
        self.B, self.kind = B, kind
        self.total = total_rows(B, 20)
        rng = np.random.default_rng(seed)
        self.calls = []
        for c, oa in enumerate(far_calls(B, 20, self.total, SIZES["a"])):
            oa = np.array(oa, np.int64)
            ob = oa + (B_SHIFT if oa[-1] + B_SHIFT <= self.total else -B_SHIFT)
            ka, kb, mt, pairs = [], [], [], []
            for p in range(len(oa) - 1):
                m = int(oa[p + 1] - oa[p])
                if kind == 0:
                    a, b, ident = hcases.planted(m, 0.6, seed + 10 * c + p)
                else:
                    a, b, ident, _ = fcases.two_view(m, 0.3, seed + 10 * c + p)
                order = rng.permutation(m)
                b, match = np.ascontiguousarray(b[order]), np.argsort(order).astype(np.int32)
                match[rng.choice(m, 3, replace=False)] = -1
                ka.append(a), kb.append(b), mt.append(match), pairs.append((a, b, match))
            self.calls.append(dict(oa=oa, ob=ob, ka=np.concatenate(ka), kb=np.concatenate(kb), match=np.concatenate(mt), pairs=pairs))


# --- tracks over a pool of B / 4 + 3 images + 37 rows: int32 labels whose byte offsets pass B ---------------------------
class Tracks:
    """Images of `rows` rows back to back from row 0 (the last 37 rows belong to no image).  Ten of them are TOUCHED: the
    first three, the three around row B / 8, the three around row B / 4 and the last three (which share two).  About 40 edges among them: a chain
    from the first image to the last whose links pass one row on, random edges with random links, a self edge, an edge given
    twice, conflicts.  The match array is addressed through a layout whose first range is [0, B / 4 + 5) over the first
    image, so every later edge's entries lie B bytes into it.  The expected labels are tracks_cases.build_tracks on the
    COMPRESSED pool -- the touched images kept in order; a label is the component's smallest row, so it survives the monotone
    re-indexing -- and every untouched row is its own track."""

    def __init__(self, B, seed):
        self.B = B
        self.rows = rows = 8192 if B >= 1 << 31 else 64
        self.total = B // 4 + rows * 3 + 37
        self.n_images = n = self.total // rows
        mid1, mid2 = (B // 8) // rows, (B // 4) // rows
        self.touched = np.unique([0, 1, 2, mid1 - 1, mid1, mid1 + 1, mid2 - 1, mid2, mid2 + 1, n - 3, n - 2, n - 1]).astype(np.int64)
        assert len(self.touched) == 10 and mid2 + 1 == n - 2          # the images around row B / 4 are among the last four
        T = len(self.touched)
        rng = np.random.default_rng(seed)
        edges = [(k, k + 1) for k in range(T - 1)]                              # the chain, first image to last
        edges += [(T - 1, 0), (5, 5), (3, 8), (3, 8)]
        while len(edges) < 40:
            edges.append(tuple(int(v) for v in rng.integers(0, T, 2)))
        self.edges_c = np.array(edges, np.int64)                                # ids of the compressed pool
        self.ea, self.eb = (self.touched[self.edges_c[:, k]].astype(np.uint32) for k in (0, 1))
        self.segments = []                                                      # per edge: match values of its a image's rows
        for e, (ia, ib) in enumerate(edges):
            seg = np.full(rows, -1, np.int32)
            if e < T - 1:
                seg[np.arange(10) + e] = np.arange(10) + e + 1                  # row r of image k to row r + 1 of image k + 1
                seg[rows - 1] = 0
            else:
                r = rng.choice(rows, 24, replace=False)
                seg[r] = rng.integers(0, rows, 24)
                seg[rng.choice(rows, 5, replace=False)] = np.array([-7, rows, rows + 3, tcases.INT32_MAX, -1], np.int32)
            self.segments.append(seg)
        self.la_c = np.arange(len(edges) + 1, dtype=np.uint64) * np.uint64(rows)      # the compressed reference's layout
        self.la = self.la_c + np.uint64(B // 4 + 5 - rows)                            # the device's: a long first range
        self.la[0] = 0
        self.cap = int(self.la[-1])

    def image_offsets(self):
        return np.arange(self.n_images + 1, dtype=np.int64) * self.rows

    def to_pool_rows(self, r):
        """compressed rows -> pool rows"""
        r = np.asarray(r, np.int64)
        return self.touched[r // self.rows] * self.rows + r % self.rows

    def expect(self, edges=slice(None), into=None):
        """(track, len, dup) over the COMPRESSED rows (to_pool_rows maps rows and labels back); `edges`: the slice of the edge
        list to link; `into`: an earlier expect()'s labels to accumulate onto"""
        T = len(self.touched)
        io_c = np.arange(T + 1, dtype=np.int64) * self.rows
        sel = np.arange(len(self.edges_c))[edges]
        match = np.concatenate([self.segments[e] for e in sel]) if len(sel) else np.zeros(0, np.int32)
        lay = np.arange(len(sel) + 1, dtype=np.uint64) * np.uint64(self.rows)
        track, length, dup = tcases.build_tracks(io_c, T * self.rows, self.edges_c[sel, 0].astype(np.uint32),
                                                 self.edges_c[sel, 1].astype(np.uint32), lay, int(lay[-1]), match, into)
        return track, length, dup

    def touched_ranges(self):
        return [(int(m) * self.rows, self.rows) for m in self.touched]
