"""Inputs and restatements for guided matching (lf_mkd_match_guided_pairs_device): the small ragged batch the CPU and GPU
tests share -- descriptors, keypoints and one model per pair for either kind --, the driver of the host twin
(tests/cpp/guided_twin.cpp: the kernel's own predicate header, local-features_amd/csrc/mkd_guided_math.h, under g++), a
float64 evaluation of the two predicates, and the coverage the batch must have for the GPU tests to mean something.  A second
batch, walk_batch(kind), has the sizes at which the kernel's tile walk and its 4096-row keypoint chunks do all they can do."""
import functools
import os
import re
import struct
import subprocess

import numpy as np

import match_pairs_cases as pcases

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "local-features_amd", "csrc")
HOMOGRAPHY, FUNDAMENTAL = 0, 1
W, H = 640, 480

# (na, nb) of pair p; the last two carry an all-zero model and a model with a NaN
SIZES = [(37, 300), (300, 37), (16, 16), (130, 17), (1, 2), (40, 50), (0, 9), (5, 0), (20, 30), (30, 20)]
ZERO_MODEL, NAN_MODEL = 8, 9
LEAD, TRAIL = (3, 21), (6, 2)                       # rows of neither pair in front of and behind them
THRESHOLDS = {HOMOGRAPHY: (3.0, 12.0), FUNDAMENTAL: (1.5, 20.0)}


def _keypoints(xy):
    """rows of 5 floats; size, angle and response are NaN: only x and y may be read"""
    k = np.full((len(xy), 5), np.nan, np.float32)
    k[:, :2] = xy
    return k


def _uniform(rng, n):
    return np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], axis=1)


def map_points(h, xy):
    p = np.concatenate([xy, np.ones((len(xy), 1))], axis=1) @ np.asarray(h, np.float64).reshape(3, 3).T
    return p[:, :2] / p[:, 2:3]


def _pair_h(rng, na, nb):
    """a uniform in the frame; half of b the true map of a rows + 0.7 px noise; 24 b rows (fewer in a small pair) within 1.4 px
    of the map of a row 0, spread over the whole index range; the rest uniform.  -> (a xy, b xy, H f32 [9])"""
    h = np.array([[1 + rng.uniform(-.05, .05), rng.uniform(-.05, .05), rng.uniform(-25, 25)],
                  [rng.uniform(-.05, .05), 1 + rng.uniform(-.05, .05), rng.uniform(-25, 25)],
                  [rng.uniform(-4e-5, 4e-5), rng.uniform(-4e-5, 4e-5), 1.0]])
    a, b = _uniform(rng, na), _uniform(rng, nb)
    if na and nb:
        true = rng.permutation(nb)[:nb // 2]
        b[true] = map_points(h, a[rng.integers(0, na, len(true))]) + rng.normal(0, 0.7, (len(true), 2))
        n_c = min(24, nb // 2)
        cluster = np.unique(np.linspace(0, nb - 1, n_c).astype(np.int64)) if n_c else np.zeros(0, np.int64)
        ang, rad = rng.uniform(0, 2 * np.pi, len(cluster)), rng.uniform(0, 1.4, len(cluster))
        b[cluster] = map_points(h, a[:1]) + np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
    return a, b, h.astype(np.float32).reshape(9)


def _pair_f(rng, na, nb):
    """two views of a random 3-D cloud: a its projections in view 1, half of b the projections in view 2 of a rows + 0.4 px
    noise, the rest uniform.  -> (a xy, b xy, F f32 [9] with b^T F a = 0 and its largest |entry| 1)"""
    K = np.array([[520.0, 0, W / 2], [0, 520.0, H / 2], [0, 0, 1]])
    n3 = max(na, 1)
    X = np.stack([rng.uniform(-3, 3, n3), rng.uniform(-2.2, 2.2, n3), rng.uniform(5, 12, n3)], axis=1)
    rx, ry, rz = rng.uniform(-.06, .06), rng.uniform(-.12, .12), rng.uniform(-.04, .04)
    Rx = np.array([[1, 0, 0], [0, np.cos(rx), -np.sin(rx)], [0, np.sin(rx), np.cos(rx)]])
    Ry = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
    Rz = np.array([[np.cos(rz), -np.sin(rz), 0], [np.sin(rz), np.cos(rz), 0], [0, 0, 1]])
    R, t = Rz @ Ry @ Rx, np.array([rng.uniform(.5, 1.0), rng.uniform(-.3, .3), rng.uniform(-.2, .2)])
    proj = lambda P: (P @ K.T)[:, :2] / (P @ K.T)[:, 2:3]
    a = proj(X)[:na]
    b = _uniform(rng, nb)
    if na and nb:
        true = rng.permutation(nb)[:nb // 2]
        b[true] = proj(X[rng.integers(0, na, len(true))] @ R.T + t) + rng.normal(0, 0.4, (len(true), 2))
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    F = np.linalg.inv(K).T @ tx @ R @ np.linalg.inv(K)
    F = F / F.reshape(-1)[np.abs(F).argmax()]
    return a, b, F.astype(np.float32).reshape(9)


class Batch:
    """The ragged batch of one kind: a / b descriptors [N, 128], ka / kb keypoints [N, 5], oa / ob offsets [n_pairs + 1]
    (starting above 0, ending below the totals), model f32 [n_pairs, 9]."""

    def __init__(self, kind):
        self.kind = kind
        rng = np.random.default_rng(4100 + kind)
        desc, xa, xb, models = [], [], [], []
        for p, (na, nb) in enumerate(SIZES):
            if na and nb:
                desc.append(pcases.descriptor_sets(na, nb, 3000 + p))
            else:
                desc.append((pcases.unit(rng.normal(size=(na, 128))), pcases.unit(rng.normal(size=(nb, 128)))))
            a, b, m = (_pair_h if kind == HOMOGRAPHY else _pair_f)(rng, na, nb)
            if p == ZERO_MODEL:
                m = np.zeros(9, np.float32)
            if p == NAN_MODEL:
                m = m.copy()
                m[4] = np.nan
            xa.append(a)
            xb.append(b)
            models.append(m)
        self.a, self.oa, self.b, self.ob = pcases.concatenate(desc, LEAD, TRAIL, seed=78)
        self.ka = _keypoints(np.concatenate([_uniform(rng, LEAD[0])] + xa + [_uniform(rng, TRAIL[0])]))
        self.kb = _keypoints(np.concatenate([_uniform(rng, LEAD[1])] + xb + [_uniform(rng, TRAIL[1])]))
        self.model = np.ascontiguousarray(np.stack(models), np.float32)
        self.n_pairs = len(SIZES)
        assert self.oa[0] > 0 and self.ob[0] > 0 and self.oa[-1] < len(self.a) and self.ob[-1] < len(self.b)
        assert len(self.ka) == len(self.a) and len(self.kb) == len(self.b)

    def pair(self, p):
        """(a rows, b rows) of pair p as slices"""
        return slice(int(self.oa[p]), int(self.oa[p + 1])), slice(int(self.ob[p]), int(self.ob[p + 1]))


@functools.lru_cache(maxsize=None)
def batch(kind):
    return Batch(kind)


# --- the host twin -----------------------------------------------------------------------------------------------------
def build(out_dir, extra=()):
    """g++ -std=c++17 -O2 -ffp-contract=off of the twin into out_dir; returns the program's path."""
    exe = os.path.join(str(out_dir), "guided_twin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", *extra, "-I", CSRC,
                           os.path.join(TESTS, "cpp", "guided_twin.cpp"), "-o", exe])
    return exe


def twin_masks(exe, tmp, problems):
    """problems: [(kind, thr, model [9], a xy [na, 2], b xy [nb, 2])] -> [(fwd [na, nb], rev [nb, na], ref [na, nb])] bool"""
    src, dst = os.path.join(str(tmp), "guided.in"), os.path.join(str(tmp), "guided.out")
    with open(src, "wb") as f:
        for kind, thr, m, a, b in problems:
            a, b = np.ascontiguousarray(a, np.float32).reshape(-1, 2), np.ascontiguousarray(b, np.float32).reshape(-1, 2)
            f.write(struct.pack("<3If", kind, len(a), len(b), thr) + np.asarray(m, np.float32).tobytes() + a.tobytes() + b.tobytes())
    done = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    buf = np.fromfile(dst, np.uint8)
    out, at = [], 0
    for kind, thr, m, a, b in problems:
        na, nb = len(a), len(b)
        n = na * nb
        out.append((buf[at:at + n].reshape(na, nb).astype(bool), buf[at + n:at + 2 * n].reshape(nb, na).astype(bool),
                    buf[at + 2 * n:at + 3 * n].reshape(na, nb).astype(bool)))
        at += 3 * n
    assert at == len(buf), (at, len(buf))
    return out


def batch_masks(exe, tmp, kind, thr):
    """the twin's masks of every pair of batch(kind) at threshold thr: [(fwd, rev, ref)]"""
    B = batch(kind)
    probs = []
    for p in range(B.n_pairs):
        sa, sb = B.pair(p)
        probs.append((kind, thr, B.model[p], B.ka[sa, :2], B.kb[sb, :2]))
    return twin_masks(exe, tmp, probs)


# --- the two predicates in float64 -------------------------------------------------------------------------------------
def f64_residual(kind, m, a, b, thr):
    """(admissible [na, nb], num / (thr2 den) [na, nb]) in float64 from the f32 inputs; thr2 is the f32 square"""
    m = np.asarray(m, np.float32).astype(np.float64)
    a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    ax, ay, bx, by = a[:, 0, None], a[:, 1, None], b[None, :, 0], b[None, :, 1]
    thr2 = float(np.float32(thr) * np.float32(thr))
    with np.errstate(all="ignore"):
        if kind == HOMOGRAPHY:
            u, v, w = m[0] * ax + m[1] * ay + m[2], m[3] * ax + m[4] * ay + m[5], m[6] * ax + m[7] * ay + m[8]
            num, den = (bx * w - u) ** 2 + (by * w - v) ** 2, w * w + 0 * bx
            ok = (w > 0) & (num < thr2 * den)
        else:
            l0, l1, l2 = m[0] * ax + m[1] * ay + m[2], m[3] * ax + m[4] * ay + m[5], m[6] * ax + m[7] * ay + m[8]
            m0, m1 = m[0] * bx + m[3] * by + m[6], m[1] * bx + m[4] * by + m[7]
            num, den = (bx * l0 + by * l1 + l2) ** 2, l0 * l0 + l1 * l1 + m0 * m0 + m1 * m1
            ok = num < thr2 * den
        return ok, num / (thr2 * den)


# --- what the batch must cover -----------------------------------------------------------------------------------------
def coverage(all_masks):
    """all_masks: {(kind, thr): [(fwd, rev, ref)]}.  Asserts, over the eight (kind, threshold, direction) combinations taken
    together: rows with 0, 1, 2, 3-16 and >= 17 candidates; a row with candidates in two different waves' tiles; a row with
    two candidates inside one lane's four rows; a 16 x 16 tile with no admissible pair and one with some.  Returns the
    numbers it found."""
    classes = {"0": 0, "1": 0, "2": 0, "3-16": 0, ">=17": 0}
    two_waves = one_lane = empty_tiles = used_tiles = 0
    for masks in all_masks.values():
        for fwd, rev, _ in masks:
            for m in (fwd, rev):                       # rows of x against candidates y
                if m.shape[0] == 0:
                    continue
                c = m.sum(axis=1)
                for name, sel in (("0", c == 0), ("1", c == 1), ("2", c == 2), ("3-16", (c >= 3) & (c <= 16)), (">=17", c >= 17)):
                    classes[name] += int(sel.sum())
                for row in m:
                    j = np.flatnonzero(row)
                    two_waves += len(set((j // 16) % 16)) > 1
                    one_lane += len(set(j // 4)) < len(j)
                for i0 in range(0, m.shape[0], 16):
                    for j0 in range(0, m.shape[1], 16):
                        if m[i0:i0 + 16, j0:j0 + 16].any():
                            used_tiles += 1
                        else:
                            empty_tiles += 1
    assert all(classes.values()), classes
    assert two_waves and one_lane and empty_tiles and used_tiles, (two_waves, one_lane, empty_tiles, used_tiles)
    return dict(classes, two_waves=int(two_waves), one_lane=int(one_lane), empty_tiles=empty_tiles, used_tiles=used_tiles)


# --- the walk batch: long tile walks and the 4096 seam -------------------------------------------------------------------
# Pair p as (na, nb, what it is there for).  A side of ny rows is ceil(ny / 16) tiles, taken round-robin by 16 waves, in chunks
# of kKpChunk = 4096 rows = 256 tiles whose keypoints are staged together.
#
#   p  (na, nb)      geometry     y tiles, a -> b / b -> a                        thresholds
#   0  (600, 1003)   _pair_h/_f   63 (4 a wave, 3 for wave 15; last of 11 rows) / 38   all
#   1  (40, 4096)    seam         256: one chunk exactly / 3                      all
#   2  (40, 4097)    seam         257: one row in a second chunk / 3              all
#   3  (40, 4136)    seam+plants  259: two tiles and 8 rows in a second chunk / 3 all
#   4  (16, 8200)    seam         513: three chunks, two seams / 1                all
#   5  (4136, 40)    seam+plants  3 / 259: the chunks in Guide<1> and Guide<3>    all
#   6  (1000, 1000)  _pair_h/_f   63 / 63                                         fundamental: 1.5 px only
#   7  (2000, 2000)  _pair_h/_f   125 (8 a wave): the operating point             fundamental: 1.5 px only
#
# The last WALK_NARROW_ONLY pairs are not run under the fundamental kind's 20 px: a band that wide admits about 15 % of
# a frame, 150 000 and 600 000 candidates for the two pairs, and the reference gathers a descriptor row per candidate
# (WALK_CAP).  They sit at the end of the batch so that a call with fewer pairs leaves them out.
WALK_SIZES = [(600, 1003), (40, 4096), (40, 4097), (40, 4136), (16, 8200), (4136, 40), (1000, 1000), (2000, 2000)]
WALK_NARROW_ONLY = 2
WALK_CAP = 1 << 18                                   # admissible candidates per (kind, threshold, direction): 128 MiB of f32 rows
CHUNK, WAVES = 4096, 16
# seam pairs: x is the small side, y the large one (x = a, or x = b in pair 5).  kill: (wave, chunk) whose tiles of y no x row
# admits; plants: rows of y put where a row of x needs them, all local to the pair:
#   dup (x rows, j0, j1): y rows j0 < 4096 <= j1 are one descriptor and one keypoint, the best of each of the x rows
#   b0s1 / b1s0 [(x row, best, second)]: the row's best admissible y row on one side of the seam, its second on the other,
#     far enough below it for the ratio test at 0.8
#   only1 [(x row, j)]: y row j >= 4096 is admissible for the row, no row below 4096 is
_P0 = [16 * (5 + 16 * k) + 3 for k in range(8)]       # rows of wave 5's tiles in chunk 0
_P1 = [4096 + k for k in (1, 3, 5, 7, 9, 11, 13)] + [4128 + k for k in (0, 2, 4, 6)]   # rows of tiles 256 and 258
_PLANTS = dict(dup=((0, 1, 2), _P0[0], _P1[0]), b0s1=[(3 + k, _P0[1 + k], _P1[1 + k]) for k in range(3)],
               b1s0=[(6 + k, _P1[4 + k], _P0[4 + k]) for k in range(3)], only1=[(9 + k, _P1[7 + k]) for k in range(3)])
SEAMS = {1: dict(rev=False, kill=[(3, 0)], plants={}),
         2: dict(rev=False, kill=[], plants=dict(b1s0=[(5, 4096, _P0[0])])),
         3: dict(rev=False, kill=[(0, 0), (1, 1)], plants=_PLANTS),
         4: dict(rev=False, kill=[(0, 1), (3, 0), (4, 1), (5, 0), (5, 1)], plants={}),
         5: dict(rev=True, kill=[(0, 0), (1, 1)], plants=_PLANTS)}


def _residual_xy(kind, m, xs, ys, rev, thr):
    """float64 num / (thr2 den) of rows xs against rows ys, [len(xs), len(ys)]; x = b when rev"""
    return f64_residual(kind, m, ys, xs, thr)[1].T if rev else f64_residual(kind, m, xs, ys, thr)[1]


def _dead(kind, m, xs, rev, rng, n):
    """n points of the y side at more than twice the wide threshold from what any row of xs admits (float64)"""
    out, have = [], 0
    for _ in range(400):
        q = _uniform(rng, 4096).astype(np.float32).astype(np.float64)
        q = q[(_residual_xy(kind, m, xs, q, rev, THRESHOLDS[kind][1]) > 4.0).all(axis=0)]
        out.append(q)
        have += len(q)
        if have >= n:
            return np.concatenate(out)[:n]
    raise AssertionError("no room for rows that nothing admits")


def _near(kind, m, p, rev, rng, r):
    """a point of the y side within r px of what the x point p admits: in the transfer disc, or beside the epipolar line"""
    m = np.asarray(m, np.float64).reshape(3, 3)
    ang, rad = rng.uniform(0, 2 * np.pi), r * np.sqrt(rng.uniform())
    d = rad * np.array([np.cos(ang), np.sin(ang)])
    if kind == HOMOGRAPHY:
        return map_points(np.linalg.inv(m), (p + d)[None])[0] if rev else map_points(m, p[None])[0] + d
    l = (m.T if rev else m) @ np.array([p[0], p[1], 1.0])
    for _ in range(64):
        if abs(l[1]) >= abs(l[0]):
            u = rng.uniform(0, W)
            q = np.array([u, -(l[0] * u + l[2]) / l[1]])
        else:
            u = rng.uniform(0, H)
            q = np.array([-(l[1] * u + l[2]) / l[0], u])
        if 0 <= q[0] < W and 0 <= q[1] < H:
            break
    return q + rng.uniform(-r, r) * l[:2] / np.hypot(l[0], l[1])


def _pair_seam(kind, rng, xd, yd, rev, kill, plants):
    """A pair whose small side x (descriptors xd) meets a y side (yd) of more than one chunk.  x lies in a strip of its frame
    (the rows of `only1` in another); a tile of y is, with probability 1/2 each, 16 rows that no x row admits, or rows of
    which half lie within 0.7 px of what some x row admits and half anywhere; the tiles of `kill` are of the first sort.  Then
    the plants, which change descriptor rows of xd and yd in place.  -> (x xy, y xy, model)"""
    ns, nl = len(xd), len(yd)
    m = (_pair_h if kind == HOMOGRAPHY else _pair_f)(rng, 8, 8)[2]
    xs = np.stack([rng.uniform(0.1 * W, 0.9 * W, ns), rng.uniform(0.35 * H, 0.55 * H, ns)], axis=1)
    only = [i for i, _ in plants.get("only1", [])]
    xs[only] = np.stack([rng.uniform(0.1 * W, 0.9 * W, len(only)), rng.uniform(0.8 * H, 0.85 * H, len(only))], axis=1)
    if "dup" in plants:
        rows = plants["dup"][0]
        xs[list(rows[1:])] = xs[rows[0]] + rng.uniform(-0.2, 0.2, (len(rows) - 1, 2))
    xs = xs.astype(np.float32).astype(np.float64)
    ys = np.zeros((nl, 2))
    n_tiles = (nl + 15) // 16
    live = rng.random(n_tiles) < 0.5
    for w, c in kill:
        live[c * (CHUNK // 16) + w:(c + 1) * (CHUNK // 16):WAVES] = False
    for j in range(nl):
        if live[j // 16]:
            ys[j] = _near(kind, m, xs[rng.integers(0, ns)], rev, rng, 0.7) if rng.random() < 0.5 else _uniform(rng, 1)[0]
    ys = ys.astype(np.float32).astype(np.float64)
    if only:                                             # below the seam, nothing near what the only1 rows admit
        close = (_residual_xy(kind, m, xs[only], ys, rev, THRESHOLDS[kind][1]) <= 4.0).any(axis=0)
        close[CHUNK:] = False
        live_row = np.repeat(live, 16)[:nl] & ~close
    else:
        live_row = np.repeat(live, 16)[:nl]
    ys[~live_row] = _dead(kind, m, xs, rev, rng, int((~live_row).sum()))
    fresh = lambda: pcases.unit(rng.normal(size=(1, 128)))[0]
    beside = lambda u, s: pcases.unit((u + s * fresh())[None])[0]
    if "dup" in plants:
        rows, j0, j1 = plants["dup"]
        ys[j0] = ys[j1] = _near(kind, m, xs[rows[0]], rev, rng, 0.3)
        yd[j1] = yd[j0]
        for i in rows:
            xd[i] = beside(yd[j0], 0.1)
    for i, jb, js in plants.get("b0s1", []) + plants.get("b1s0", []):
        xd[i] = fresh()
        yd[jb], yd[js] = beside(xd[i], 0.2), beside(xd[i], 1.2)      # similarities about 0.98 and 0.64
        ys[jb], ys[js] = _near(kind, m, xs[i], rev, rng, 0.3), _near(kind, m, xs[i], rev, rng, 0.3)
    for i, j in plants.get("only1", []):
        xd[i] = fresh()
        yd[j] = beside(xd[i], 0.2)
        ys[j] = _near(kind, m, xs[i], rev, rng, 0.3)
    return xs, ys, m


class WalkBatch(Batch):
    """Batch's layout over WALK_SIZES; `seams` are SEAMS' pairs."""

    def __init__(self, kind):
        self.kind = kind
        rng = np.random.default_rng(4200 + kind)
        desc, xa, xb, models = [], [], [], []
        for p, (na, nb) in enumerate(WALK_SIZES):
            da, db = pcases.descriptor_sets(na, nb, 5000 + p)
            if p in SEAMS:
                S = SEAMS[p]
                if S["rev"]:
                    b, a, m = _pair_seam(kind, rng, db, da, True, S["kill"], S["plants"])
                else:
                    a, b, m = _pair_seam(kind, rng, da, db, False, S["kill"], S["plants"])
            else:
                a, b, m = (_pair_h if kind == HOMOGRAPHY else _pair_f)(rng, na, nb)
            desc.append((da, db))
            xa.append(a)
            xb.append(b)
            models.append(m)
        self.a, self.oa, self.b, self.ob = pcases.concatenate(desc, LEAD, TRAIL, seed=79)
        self.ka = _keypoints(np.concatenate([_uniform(rng, LEAD[0])] + xa + [_uniform(rng, TRAIL[0])]))
        self.kb = _keypoints(np.concatenate([_uniform(rng, LEAD[1])] + xb + [_uniform(rng, TRAIL[1])]))
        self.model = np.ascontiguousarray(np.stack(models), np.float32)
        self.n_pairs = len(WALK_SIZES)
        assert self.oa[0] > 0 and self.ob[0] > 0 and self.oa[-1] < len(self.a) and self.ob[-1] < len(self.b)
        assert len(self.ka) == len(self.a) and len(self.kb) == len(self.b)
        assert np.abs(np.linalg.norm(self.a, axis=1) - 1).max() < 1e-6 and np.abs(np.linalg.norm(self.b, axis=1) - 1).max() < 1e-6

    def run_pairs(self, thr):
        """how many of the batch's pairs (from the front) are run at threshold thr"""
        wide = self.kind == FUNDAMENTAL and thr == THRESHOLDS[FUNDAMENTAL][1]
        return self.n_pairs - (WALK_NARROW_ONLY if wide else 0)

    def sides(self, p, rev):
        """(x descriptors, y descriptors) of pair p: x = b when rev"""
        sa, sb = self.pair(p)
        return (self.b[sb], self.a[sa]) if rev else (self.a[sa], self.b[sb])


@functools.lru_cache(maxsize=None)
def walk_batch(kind):
    return WalkBatch(kind)


def walk_masks(exe, tmp, kind, thr):
    """the twin's masks of the pairs of walk_batch(kind) that are run at threshold thr: [(fwd, rev, ref)]"""
    B = walk_batch(kind)
    probs = []
    for p in range(B.run_pairs(thr)):
        sa, sb = B.pair(p)
        probs.append((kind, thr, B.model[p], B.ka[sa, :2], B.kb[sb, :2]))
    return twin_masks(exe, tmp, probs)


def walks(mask, nx, ny):
    """{(block, wave, chunk): the wave's walk} for rows x [nx] against candidates y [ny] under mask [nx, ny].  A block is 16
    rows of x; wave w of a block visits tiles w, w + 16, ... of each chunk of 256 tiles of y (a tile: 16 rows); a tile is used
    ("U") for a block iff any of its 16 x 16 mask entries is set, skipped ("S") otherwise.  A wave without a tile in a chunk
    has no walk there."""
    mask = np.asarray(mask, bool).reshape(nx, ny)
    n_blocks, n_tiles = (nx + 15) // 16, (ny + 15) // 16
    full = np.zeros((n_blocks * 16, n_tiles * 16), bool)
    full[:nx, :ny] = mask
    used = full.reshape(n_blocks, 16, n_tiles, 16).any(axis=(1, 3))
    out = {}
    per_chunk = CHUNK // 16
    for c in range((n_tiles + per_chunk - 1) // per_chunk):
        for w in range(WAVES):
            sub = used[:, c * per_chunk + w:min((c + 1) * per_chunk, n_tiles):WAVES]
            if sub.shape[1] == 0:
                continue
            text = np.where(sub, ord("U"), ord("S")).astype(np.uint8)
            for blk in range(n_blocks):
                out[(blk, w, c)] = text[blk].tobytes().decode()
    return out


def _top(x, y, cand):
    """candidates by float64 similarity to the row x, best first (later index first among equals): (indices, similarities)"""
    s = np.array([np.dot(x.astype(np.float64), y[j].astype(np.float64)) for j in cand])
    order = np.lexsort((-np.asarray(cand), -s))
    return np.asarray(cand)[order], s[order]


def walk_coverage(all_masks):
    """all_masks: {(kind, thr): [(fwd, rev, ref)] of the pairs run}.  Asserts, over both kinds, thresholds and directions taken
    together, that every pattern of a walk the kernel distinguishes occurs (the keys of the result), that the planted rows of
    SEAMS are what they claim to be -- float64 similarities over the twin's admissible rows, 1e-4 between the ranks
    concerned, the duplicates tying exactly -- and that no (kind, threshold, direction) has WALK_CAP candidates or more.
    Returns the counts."""
    pat = {"used-skipped-used": re.compile("USU"), "two or more skipped between used": re.compile("US{2,}U"),
           "two or more skipped, then used": re.compile("^S{2,}U"), "used, then two or more skipped to the end": re.compile("US{2,}$"),
           "four or more used in a row": re.compile("U{4,}")}
    found = dict.fromkeys(list(pat) + ["a wave all skipped beside a used one", "last partial tile used", "last partial tile skipped",
                                       "seam: skipped then used", "seam: used then skipped", "seam: used on both sides",
                                       "walks", "longest walk", "planted rows checked"], 0)
    most = 0
    for (kind, thr), masks in all_masks.items():
        B = walk_batch(kind)
        assert len(masks) == B.run_pairs(thr)
        for rev in (False, True):
            total = 0
            for p, (fwd, back, _) in enumerate(masks):
                m = back if rev else fwd
                nx, ny = m.shape
                total += int(m.sum())
                ws = walks(m, nx, ny)
                found["walks"] += len(ws)
                n_tiles, last = (ny + 15) // 16, (ny + 15) // 16 - 1
                for (blk, w, c), text in ws.items():
                    found["longest walk"] = max(found["longest walk"], len(text))
                    for name, rx in pat.items():
                        found[name] += bool(rx.search(text))
                    if ny % 16 and c == last // 256 and w == last % 16:
                        found["last partial tile used" if text[-1] == "U" else "last partial tile skipped"] += 1
                    if c == 0 and (blk, w, 1) in ws:
                        u0, u1 = "U" in text, "U" in ws[(blk, w, 1)]
                        found["seam: skipped then used"] += (not u0) and u1
                        found["seam: used then skipped"] += u0 and not u1
                        found["seam: used on both sides"] += u0 and u1
                for blk in range((nx + 15) // 16):
                    any_used = ["U" in "".join(ws.get((blk, w, c), "") for c in range((n_tiles + 255) // 256)) for w in range(min(WAVES, n_tiles))]
                    found["a wave all skipped beside a used one"] += any(any_used) and not all(any_used)
                if p in SEAMS and SEAMS[p]["rev"] == rev:
                    found["planted rows checked"] += _check_plants(B, p, rev, m)
            assert total < WALK_CAP, (kind, thr, rev, total)
            most = max(most, total)
    assert all(found.values()), found
    found["most candidates in one (kind, threshold, direction)"] = most
    return found


def _check_plants(B, p, rev, mask):
    """the claims of SEAMS[p]["plants"] under mask [nx, ny]; returns how many x rows it checked"""
    x, y = B.sides(p, rev)
    plants, n = SEAMS[p]["plants"], 0
    gap = lambda s, k: len(s) <= k + 1 or s[k] - s[k + 1] >= 1e-4
    if "dup" in plants:
        rows, j0, j1 = plants["dup"]
        assert j0 < CHUNK <= j1 and len(rows) >= 3 and np.array_equal(y[j0], y[j1])
        for i in rows:
            idx, s = _top(x[i], y, np.flatnonzero(mask[i]))
            assert tuple(idx[:2]) == (j1, j0) and s[0] == s[1] and gap(s, 1), (p, i, idx[:3], s[:3])
            n += 1
    for name, side in (("b0s1", (True, False)), ("b1s0", (False, True))):
        for i, jb, js in plants.get(name, []):
            idx, s = _top(x[i], y, np.flatnonzero(mask[i]))
            assert tuple(idx[:2]) == (jb, js) and (jb < CHUNK, js < CHUNK) == side and gap(s, 0) and gap(s, 1), (p, name, i, idx[:3], s[:3])
            assert s[0] * 0.8 > s[1] + 1e-3, (p, name, i, s[:2])                 # accepted at ratio 0.8 too
            n += 1
    for i, j in plants.get("only1", []):
        cand = np.flatnonzero(mask[i])
        idx, s = _top(x[i], y, cand)
        assert len(cand) and cand.min() >= CHUNK and idx[0] == j and gap(s, 0), (p, i, cand[:4])
        assert len(s) == 1 or s[0] * 0.8 > s[1] + 1e-3, (p, i, s[:2])
        n += 1
    return n
