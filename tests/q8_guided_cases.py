"""Inputs and restatements for guided matching over 8-bit rows (lf_mkd_match_q8_guided_pairs_device): the ragged batch the CPU
and GPU tests share -- quantised descriptors, keypoints and one model per pair for either kind, with planted rows --, the
masked integer reference (tests/q8_cases.py's sums under the host twin's masks, tests/match_guided_cases.py), and the coverage
the batch must have for the GPU tests to mean something.  The sizes are chosen for the kernel's shape: R = 128 rows of x per
workgroup, 32-row tiles, stages of 4 tiles = 128 rows of y."""
import functools
import re

import numpy as np

import match_guided_cases as gcases
import match_pairs_cases as pcases
import q8_cases as qcases

HOMOGRAPHY, FUNDAMENTAL = gcases.HOMOGRAPHY, gcases.FUNDAMENTAL
KINDS = (HOMOGRAPHY, FUNDAMENTAL)
THRESHOLDS = gcases.THRESHOLDS
INT32_MIN = qcases.INT32_MIN
RATIO = qcases.RATIO
SENTINEL = -7
R, TILE, STAGE = 128, 32, 128

# (na, nb) of pair p
SIZES = [(37, 300), (300, 37),
         (128, 128),                 # one block, one stage
         (129, 257),                 # a block of one row; three stages, the last of one row in the reused buffer
         (1, 1), (1, 2), (2, 1), (0, 9), (5, 0), (33, 129), (130, 31),
         (600, 1003),                # five blocks, the last with an idle wave; 32 y tiles, the last of 11 rows
         (40, 50),                   # all-zero model
         (30, 20)]                   # a NaN in the model
ZERO_MODEL, NAN_MODEL = 12, 13
LEAD, TRAIL = (3, 21), (6, 2)        # rows of neither pair in front of and behind them

# Planted rows, per pair: rev (x = b), and rows local to the pair's x and y sides.  The x rows' keypoints lie far outside the
# frame, each at a spot of its own, so that what they admit holds nothing but the y rows put there:
#   dup   (i, j0, j1):      y rows j0 < j1 are ONE descriptor, both admissible for x row i and its best: second == best, j1 wins
#   lone  (i, j0, j1, j2):  j0 < j1 are one descriptor again, x row i's best, but j1 is NOT admissible; j2 is, and is the second
#   last  (i, j0, j1):      x row i's only admissible rows, both in the last partial tile of y; j1 the best
PLANTS = {0: dict(rev=False, dup=(3, 40, 170), lone=(9, 75, 210, 100), last=(20, 290, 297)),
          1: dict(rev=True, dup=(3, 40, 170), lone=(9, 75, 210, 100), last=(20, 290, 297)),
          11: dict(rev=False, dup=(3, 40, 700), lone=(9, 75, 800, 300), last=(20, 995, 1001))}


def _spot(k):
    """the k-th spot outside the frame: no two spots, and no spot and the frame, within hundreds of pixels of each other"""
    return np.array([gcases.W + 350.0 + 260.0 * k, gcases.H + 300.0 + 210.0 * k])


def _plant(kind, rng, P, xd, yd, xs, ys, m):
    """the plants P of one pair into its f32 descriptors (xd, yd) and keypoints (xs, ys), all changed in place"""
    rev = P["rev"]
    fresh = lambda: pcases.unit(rng.normal(size=(1, 128)))[0]
    beside = lambda u, s: pcases.unit((u + s * fresh())[None])[0]
    near = lambda i: gcases._near(kind, m, xs[i], rev, rng, 0.3)
    i, j0, j1 = P["dup"]
    xs[i] = _spot(0)
    ys[j0], ys[j1] = near(i), near(i)
    yd[j1] = yd[j0]
    xd[i] = beside(yd[j0], 0.1)
    i, j0, j1, j2 = P["lone"]
    xs[i] = _spot(1)
    ys[j0], ys[j2] = near(i), near(i)                    # (j1 keeps its place in the frame)
    yd[j1] = yd[j0]
    xd[i] = beside(yd[j0], 0.1)
    yd[j2] = beside(xd[i], 1.2)                          # similarity about 0.64
    i, j0, j1 = P["last"]
    xs[i] = _spot(2)
    ys[j0], ys[j1] = near(i), near(i)
    xd[i] = fresh()
    yd[j1], yd[j0] = beside(xd[i], 0.2), beside(xd[i], 1.2)


class Batch:
    """The ragged batch of one kind: qa / qb quantised descriptors [N, 128] uint8 (a / b: the f32 rows they were quantised
    from), ka / kb keypoints [N, 5] with NaN in every field but x and y, oa / ob offsets [n_pairs + 1] (starting above 0,
    ending below the totals), model f32 [n_pairs, 9]."""

    def __init__(self, kind):
        self.kind = kind
        rng = np.random.default_rng(5200 + kind)
        desc, xa, xb, models = [], [], [], []
        for p, (na, nb) in enumerate(SIZES):
            if na and nb:
                da, db = pcases.descriptor_sets(na, nb, 3000 + p)
            else:
                da, db = pcases.unit(rng.normal(size=(na, 128))), pcases.unit(rng.normal(size=(nb, 128)))
            a, b, m = (gcases._pair_h if kind == HOMOGRAPHY else gcases._pair_f)(rng, na, nb)
            if p in PLANTS:
                if PLANTS[p]["rev"]:
                    _plant(kind, rng, PLANTS[p], db, da, b, a, m)
                else:
                    _plant(kind, rng, PLANTS[p], da, db, a, b, m)
            if p == ZERO_MODEL:
                m = np.zeros(9, np.float32)
            if p == NAN_MODEL:
                m = m.copy()
                m[4] = np.nan
            desc.append((da, db))
            xa.append(a)
            xb.append(b)
            models.append(m)
        self.a, self.oa, self.b, self.ob = pcases.concatenate(desc, LEAD, TRAIL, seed=81)
        self.qa, self.qb = qcases.quantize(self.a), qcases.quantize(self.b)
        self.ka = gcases._keypoints(np.concatenate([gcases._uniform(rng, LEAD[0])] + xa + [gcases._uniform(rng, TRAIL[0])]))
        self.kb = gcases._keypoints(np.concatenate([gcases._uniform(rng, LEAD[1])] + xb + [gcases._uniform(rng, TRAIL[1])]))
        self.model = np.ascontiguousarray(np.stack(models), np.float32)
        self.n_pairs = len(SIZES)
        assert self.oa[0] > 0 and self.ob[0] > 0 and self.oa[-1] < len(self.a) and self.ob[-1] < len(self.b)
        assert len(self.ka) == len(self.a) and len(self.kb) == len(self.b)
        assert np.isnan(self.ka[:, 2:]).all() and np.isnan(self.kb[:, 2:]).all() and self.qa.min() >= 1 and self.qb.min() >= 1
        for arr in (self.a, self.b, self.qa, self.qb, self.ka, self.kb, self.oa, self.ob, self.model):
            arr.setflags(write=False)

    def pair(self, p):
        """(a rows, b rows) of pair p as slices"""
        return slice(int(self.oa[p]), int(self.oa[p + 1])), slice(int(self.ob[p]), int(self.ob[p + 1]))

    def sides(self, p, rev):
        """(x rows, y rows) of pair p, quantised: x = b when rev"""
        sa, sb = self.pair(p)
        return (self.qb[sb], self.qa[sa]) if rev else (self.qa[sa], self.qb[sb])


@functools.lru_cache(maxsize=None)
def batch(kind):
    return Batch(kind)


def batch_masks(exe, tmp, kind, thr):
    """the host twin's masks of every pair of batch(kind) at threshold thr: [(fwd [na, nb], rev [nb, na], ref [na, nb])]"""
    B = batch(kind)
    probs = []
    for p in range(B.n_pairs):
        sa, sb = B.pair(p)
        probs.append((kind, thr, B.model[p], B.ka[sa, :2], B.kb[sb, :2]))
    return gcases.twin_masks(exe, tmp, probs)


def all_masks(exe, tmp):
    """{(kind, thr): batch_masks}: both kinds, both thresholds"""
    return {(kind, thr): batch_masks(exe, tmp, kind, thr) for kind in KINDS for thr in THRESHOLDS[kind]}


# --- the masked integer reference ---------------------------------------------------------------------------------------
def decide(x, y, mask, ratio=RATIO):
    """(match, best, second) of rows x against the rows of y that mask [nx, ny] admits: lf_mkd_match_q8_device's decision over
    the admissible rows only.  Inadmissible sums are INT32_MIN, below every sum; a stable ascending sort leaves the highest
    index last among equals; one candidate: second = INT32_MIN, accepted; none: -1 and INT32_MIN twice."""
    nx, ny = len(x), len(y)
    lowest = np.full(nx, INT32_MIN, np.int32)
    if nx == 0 or ny == 0:
        return np.full(nx, -1, np.int32), lowest, lowest.copy()
    s = np.where(np.asarray(mask, bool).reshape(nx, ny), qcases.similarities(x, y), INT32_MIN)
    order = np.argsort(s, axis=1, kind="stable")
    rows = np.arange(nx)
    idx = order[:, -1]
    best = s[rows, idx]
    second = s[rows, order[:, -2]] if ny >= 2 else lowest
    idx = np.where(best == INT32_MIN, -1, idx)
    ok = (idx >= 0) & ((np.float32(ratio) <= 0) | (best.astype(np.float32) * np.float32(ratio) > second.astype(np.float32)))
    return np.where(ok, idx, -1).astype(np.int32), best.astype(np.int32), second.astype(np.int32)


def reference(B, masks, ratio=RATIO, n_pairs=None, fill=SENTINEL):
    """(match_ab [Na], match_ba [Nb], best [Na], second [Na]) of the call without the mutual filter over the first n_pairs
    pairs of B under masks [(fwd, rev, _)]; rows outside those pairs hold `fill`."""
    ab, ba = np.full(len(B.qa), fill, np.int32), np.full(len(B.qb), fill, np.int32)
    best, second = np.full(len(B.qa), fill, np.int32), np.full(len(B.qa), fill, np.int32)
    for p in range(B.n_pairs if n_pairs is None else n_pairs):
        sa, sb = B.pair(p)
        fwd, rev, _ = masks[p]
        ab[sa], best[sa], second[sa] = decide(B.qa[sa], B.qb[sb], fwd, ratio)
        ba[sb] = decide(B.qb[sb], B.qa[sa], rev, ratio)[0]
    return ab, ba, best, second


# --- what the batch must cover -----------------------------------------------------------------------------------------
def tiles_used(mask):
    """[x tiles, y tiles] bool: which 32 x 32 tiles of mask [nx, ny] hold an admissible pair (x tiles counted from the pair's
    first row, as the kernel's blocks of R = 4 tiles are)"""
    nx, ny = mask.shape
    tx, ty = (nx + TILE - 1) // TILE, (ny + TILE - 1) // TILE
    full = np.zeros((tx * TILE, ty * TILE), bool)
    full[:nx, :ny] = mask
    return full.reshape(tx, TILE, ty, TILE).any(axis=(1, 3))


def check_plants(B, p, mask):
    """the claims of PLANTS[p] under mask [nx, ny] of its direction; returns how many x rows it checked"""
    P = PLANTS[p]
    x, y = B.sides(p, P["rev"])
    s = qcases.similarities(x, y)
    ny = len(y)
    i, j0, j1 = P["dup"]
    adm = np.flatnonzero(mask[i])
    assert j0 < j1 and np.array_equal(y[j0], y[j1]) and mask[i, j0] and mask[i, j1], (p, "dup")
    assert s[i, j0] == s[i, j1] == s[i, adm].max() and (s[i, adm] == s[i, j1]).sum() == 2, (p, "dup", s[i, adm])
    assert j0 // STAGE != j1 // STAGE                                        # ... and the two copies arrive in different stages
    i, j0, j1, j2 = P["lone"]
    adm = np.flatnonzero(mask[i])
    assert j0 < j1 and np.array_equal(y[j0], y[j1]) and mask[i, j0] and not mask[i, j1] and mask[i, j2], (p, "lone")
    assert s[i, j0] == s[i, adm].max() and (s[i, adm] == s[i, j0]).sum() == 1, (p, "lone")
    assert s[i, j2] == np.sort(s[i, adm])[-2] and s[i, j0] * RATIO > s[i, j2], (p, "lone", s[i, adm])
    i, j0, j1 = P["last"]
    adm = np.flatnonzero(mask[i])
    assert ny % TILE and len(adm) >= 2 and adm.min() >= (ny // TILE) * TILE, (p, "last", adm)
    assert adm[s[i, adm].argmax()] == j1 and (s[i, adm] == s[i, j1]).sum() == 1, (p, "last")
    return 3


def coverage(masks_by_case):
    """masks_by_case: {(kind, thr): [(fwd, rev, ref)]}.  Asserts, over both kinds, both thresholds and both directions taken
    together: rows with 0, 1, 2, 3-16 and >= 17 candidates; a row with candidates in two different stages; 32 x 32 tiles with
    no admissible pair and with some; an x tile whose walk over the y tiles goes used-skipped-used; a last partial tile used
    and one skipped; and the plants as claimed, in every case.  Returns {(kind, thr): counts} and the totals under "all"."""
    keys = ["0", "1", "2", "3-16", ">=17", "rows spanning stages", "empty tiles", "used tiles", "used-skipped-used walks",
            "last partial tile used", "last partial tile skipped", "planted rows checked"]
    out = {}
    for (kind, thr), masks in masks_by_case.items():
        B = batch(kind)
        c = dict.fromkeys(keys, 0)
        for p, (fwd, rev, _) in enumerate(masks):
            for is_rev, m in ((False, fwd), (True, rev)):                   # rows of x against candidates y
                nx, ny = m.shape
                if nx == 0:
                    continue
                n = m.sum(axis=1)
                for name, sel in (("0", n == 0), ("1", n == 1), ("2", n == 2), ("3-16", (n >= 3) & (n <= 16)), (">=17", n >= 17)):
                    c[name] += int(sel.sum())
                if ny:
                    ns = (ny + STAGE - 1) // STAGE
                    full = np.zeros((nx, ns * STAGE), bool)
                    full[:, :ny] = m
                    c["rows spanning stages"] += int((full.reshape(nx, ns, STAGE).any(axis=2).sum(axis=1) > 1).sum())
                    used = tiles_used(m)
                    c["used tiles"] += int(used.sum())
                    c["empty tiles"] += int((~used).sum())
                    for walk in used:
                        c["used-skipped-used walks"] += bool(re.search("US+U", "".join("U" if u else "S" for u in walk)))
                    if ny % TILE:
                        c["last partial tile used"] += int(used[:, -1].sum())
                        c["last partial tile skipped"] += int((~used[:, -1]).sum())
                if p in PLANTS and PLANTS[p]["rev"] == is_rev:
                    c["planted rows checked"] += check_plants(B, p, m)
        assert c["planted rows checked"] == 3 * len(PLANTS), ((kind, thr), c)
        out[(kind, thr)] = c
    total = {k: sum(c[k] for c in out.values()) for k in keys}
    assert all(total.values()), total
    out["all"] = total
    return out
