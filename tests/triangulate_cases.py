"""Scenes for the track triangulation call (include/lf_mkd.h, lf_mkd_triangulate_tracks_device) and a float64 numpy
restatement of its steps 1 - 7.

A `table` is a dict of the device call's arrays under its argument names: kps [rows, 5] float32, track_offsets uint64
[tracks + 1], obs_row int32 / obs_image uint32 [observations], counts uint32 [2], intrinsics [images, 4], poses [images, 12]
(R row-major, then t; world to camera).  The generators add what they know under other keys: `X` the true points, `clean` per
observation whether it is the point's projection plus noise (False: a planted outlier).

The restatement sums with numpy in whatever order numpy likes: it is held to the twin within a tolerance, and decisions
(counts, reasons, pairs, states) exactly.  So that a decision cannot flip between two valid orders it reports how close it
came to one (`margins`), and `decided` says whether a case is far enough from all of them: the generators and tests keep
decided cases only."""
import numpy as np

THRESHOLD_MARGIN = 1e-6     # a squared error this close (relative) to thr2 is undecided
SINGULAR = 1e-12
NONE = 0xFFFFFFFF


# ---- the restatement -------------------------------------------------------------------------------------------------------

def _arrays(t):
    return (np.ascontiguousarray(t["kps"], np.float32).reshape(-1, 5), np.ascontiguousarray(t["track_offsets"], np.uint64),
            np.ascontiguousarray(t["obs_row"], np.int32), np.ascontiguousarray(t["obs_image"], np.uint32),
            np.ascontiguousarray(t["counts"], np.uint32)[:2], np.ascontiguousarray(t["intrinsics"], np.float32).reshape(-1, 4),
            np.ascontiguousarray(t["poses"], np.float32).reshape(-1, 12))


class _Track:
    """one track's usable positions in float64: x, y, K, R, t, the unit rays u and the centres c, the contributions W"""

    def __init__(self, kps, row, img, K, P):
        n_rows, n_images = len(kps), len(K)
        ok = (row >= 0) & (row < n_rows) & (img < n_images)
        r, m = np.where(ok, row, 0), np.where(ok, img, 0).astype(np.int64)
        if n_rows == 0 or n_images == 0:
            ok[:] = False
            self.usable = ok
            return
        k, p, xy = K[m].astype(np.float64), P[m].astype(np.float64), kps[r][:, :2].astype(np.float64)
        with np.errstate(all="ignore"):
            ok &= np.isfinite(k).all(1) & (k[:, 0] > 0) & (k[:, 1] > 0) & np.isfinite(p).all(1) & (p[:, :9] != 0).any(1)
            ok &= np.isfinite(xy).all(1)
            self.usable = ok
            self.k, self.R, self.t, self.xy = k, p[:, :9].reshape(-1, 3, 3), p[:, 9:], xy
            xn = np.stack([(xy[:, 0] - k[:, 2]) / k[:, 0], (xy[:, 1] - k[:, 3]) / k[:, 1], np.ones(len(xy))], 1)
            d = np.einsum("nij,ni->nj", self.R, xn)
            self.u = d / np.sqrt((d * d).sum(1))[:, None]
            self.c = -np.einsum("nij,ni->nj", self.R, self.t)
            uc = (self.u * self.c).sum(1)
            Pm = np.eye(3)[None] - self.u[:, :, None] * self.u[:, None, :]
            self.A, self.b = Pm, self.c - self.u * uc[:, None]

    def solve(self, S, margins):
        """step 3 over the set S (a boolean mask): X, or None if singular"""
        with np.errstate(all="ignore"):
            A, b = self.A[S].sum(0), self.b[S].sum(0)
            det, m = np.linalg.det(A), np.trace(A) / 3.0
            bound = SINGULAR * m ** 3
            margins["singular"] = min(margins["singular"], abs(np.log10(det / bound)) if det > 0 and bound > 0 else 9.0)
            if not det > bound:
                return None
            c = np.array([[A[1, 1] * A[2, 2] - A[1, 2] ** 2, A[0, 2] * A[1, 2] - A[0, 1] * A[2, 2], A[0, 1] * A[1, 2] - A[0, 2] * A[1, 1]],
                          [0, A[0, 0] * A[2, 2] - A[0, 2] ** 2, A[0, 1] * A[0, 2] - A[0, 0] * A[1, 2]],
                          [0, 0, A[0, 0] * A[1, 1] - A[0, 1] ** 2]])
            c = c + np.triu(c, 1).T
            return c @ b / det

    def errors(self, X):
        with np.errstate(all="ignore"):
            p = np.einsum("nij,j->ni", self.R, X) + self.t
            ex = self.k[:, 0] * (p[:, 0] / p[:, 2]) + self.k[:, 2] - self.xy[:, 0]
            ey = self.k[:, 1] * (p[:, 1] / p[:, 2]) + self.k[:, 3] - self.xy[:, 1]
            return p[:, 2] > 0, ex * ex + ey * ey

    def inliers(self, X, thr2, margins):
        front, e2 = self.errors(X)
        with np.errstate(all="ignore"):
            near = np.abs(e2 - thr2)[self.usable & front & np.isfinite(e2)] / thr2
            if near.size:
                margins["threshold"] = min(margins["threshold"], float(near.min()))
            return self.usable & front & (e2 <= thr2)


def reference(t, px=4.0, rounds=2):
    """-> dict: points float64 [T, 4], stats int64 [T, 4], err float64 [T, 2], obs_state int64 [O] (-1 where no track's range
    covers an entry), margins {threshold, singular, parallax}: the closest any decision came to flipping."""
    kps, off, row, img, counts, K, P = _arrays(t)
    tcap, ocap = len(off) - 1, len(row)
    T, O = min(int(counts[0]), tcap), min(int(counts[1]), ocap)
    thr2 = float(np.float32(px)) ** 2
    points, stats, err = np.zeros((T, 4)), np.zeros((T, 4), np.int64), np.zeros((T, 2))
    state = np.full(ocap, -1, np.int64)
    margins = {"threshold": 9.0, "singular": 9.0, "parallax": 9.0}
    for i in range(T):
        lo, hi = min(int(off[i]), O), min(int(off[i + 1]), O)
        hi = max(hi, lo)
        tr = _Track(kps, row[lo:hi], img[lo:hi], K, P)
        usable = tr.usable
        U = int(usable.sum())
        state[lo:hi] = usable.astype(np.int64)
        points[i], stats[i] = (0, 0, 0, 2), (U, 0, 1, NONE)
        if U < 2:
            continue
        cand = np.flatnonzero(usable)[:8]
        best, pair, Xw = -1, NONE, None
        for a in range(len(cand)):
            for b in range(a + 1, len(cand)):
                if best == U:
                    continue
                S = np.zeros(len(usable), bool)
                S[[cand[a], cand[b]]] = True
                X = tr.solve(S, margins)
                if X is None:
                    continue
                score = int(tr.inliers(X, thr2, margins).sum())
                if score > best:
                    best, pair, Xw = score, a << 16 | b, X
        stats[i, 3] = pair
        if Xw is None:
            stats[i, 2] = 2
            continue
        if best < 2:
            stats[i, 2] = 3
            continue
        S, X, reason = tr.inliers(Xw, thr2, margins), None, 0
        X = tr.solve(S, margins)
        if X is None:
            stats[i, 2] = 2
            continue
        for _ in range(rounds):
            S2 = tr.inliers(X, thr2, margins)
            if (S2 == S).all():
                break
            if S2.sum() < 2:
                reason = 3
                break
            S, X = S2, tr.solve(S2, margins)
            if X is None:
                reason = 2
                break
        if reason == 0:
            S = tr.inliers(X, thr2, margins)
            if S.sum() < 2:
                reason = 3
        if reason:
            stats[i, 2] = reason
            continue
        idx = np.flatnonzero(S)
        d0 = tr.u[idx] @ tr.u[idx[0]]
        a = idx[np.argmin(d0)]
        if len(idx) > 2:
            two = np.sort(d0)[:2]
            margins["parallax"] = min(margins["parallax"], float(two[1] - two[0]))
        cosine = float((tr.u[idx] @ tr.u[a]).min())
        _, e2 = tr.errors(X)
        points[i], stats[i] = (X[0], X[1], X[2], cosine), (U, len(idx), 0, pair)
        err[i] = (np.sqrt(e2[idx].mean()), np.sqrt(e2[idx].max()))
        state[lo:hi][S] = 2
    return {"points": points, "stats": stats, "err": err, "obs_state": state, "margins": margins}


def decided(ref):
    """is every decision of the restatement far from flipping under another summation order?  (the threshold test by
    THRESHOLD_MARGIN relative, the singular test by a factor of 100 either way, the parallax anchor by 1e-9 in cosine)"""
    m = ref["margins"]
    return m["threshold"] > THRESHOLD_MARGIN and m["singular"] > 2.0 and m["parallax"] > 1e-9


# ---- scenes ----------------------------------------------------------------------------------------------------------------

def look_at(centre, target, roll=0.0):
    """world-to-camera (R, t) of a camera at `centre` looking at `target`"""
    z = target - centre
    z = z / np.linalg.norm(z)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    c, s = np.cos(roll), np.sin(roll)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) @ np.stack([x, y, z])
    return R, -R @ centre


def cameras(n, rng, depth=10.0, spread=4.0):
    """n cameras around the origin's near side, all looking at a point `depth` ahead: intrinsics [n, 4], poses [n, 12]"""
    K, P = np.zeros((n, 4), np.float32), np.zeros((n, 12), np.float32)
    for i in range(n):
        centre = np.array([rng.uniform(-spread, spread), rng.uniform(-0.3 * spread, 0.3 * spread), rng.uniform(-1.0, 1.0)])
        R, t = look_at(centre, np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), depth]), rng.uniform(-0.2, 0.2))
        K[i] = (rng.uniform(700, 900), rng.uniform(700, 900), rng.uniform(300, 340), rng.uniform(220, 260))
        P[i] = np.concatenate([R.reshape(9), t])
    return K, P


def project(K, P, X):
    p = P[:9].astype(np.float64).reshape(3, 3) @ X + P[9:].astype(np.float64)
    return np.array([K[0] * p[0] / p[2] + K[2], K[1] * p[1] / p[2] + K[3]])


def scene(rng, lengths, n_images, noise=0.5, outliers=0.1, outlier_px=(30.0, 100.0), depth=(6.0, 14.0), shuffle=True):
    """One track per entry of `lengths`, each a point at `depth` seen by that many observations over n_images cameras (distinct
    images while they last), `noise` px of Gaussian noise, a fraction `outliers` of the observations displaced by outlier_px
    in a random direction.  Every observation has a keypoint row of its own; the rows are shuffled in the pool."""
    K, P = cameras(n_images, rng)
    n_obs = int(np.sum(lengths))
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    kps = np.zeros((n_obs, 5), np.float32)
    kps[:, 2:] = rng.uniform(1, 4, (n_obs, 3))
    row = (rng.permutation(n_obs) if shuffle else np.arange(n_obs)).astype(np.int32)
    img, clean, X = np.zeros(n_obs, np.uint32), np.ones(n_obs, bool), np.zeros((len(lengths), 3))
    for i, n in enumerate(lengths):
        X[i] = (rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(*depth))
        ims = np.concatenate([rng.permutation(n_images)] * (n // n_images + 1))[:n] if n else np.zeros(0, int)
        for j in range(n):
            k = int(off[i]) + j
            img[k] = ims[j]
            xy = project(K[ims[j]], P[ims[j]], X[i]) + rng.normal(0, noise, 2) if noise else project(K[ims[j]], P[ims[j]], X[i])
            if rng.uniform() < outliers:
                a = rng.uniform(0, 2 * np.pi)
                xy = xy + rng.uniform(*outlier_px) * np.array([np.cos(a), np.sin(a)])
                clean[k] = False
            kps[row[k], :2] = xy
    return {"kps": kps, "track_offsets": off, "obs_row": row, "obs_image": img, "counts": np.array([len(lengths), n_obs], np.uint32),
            "intrinsics": K, "poses": P, "X": X, "clean": clean}


def decided_scene(seed, *args, px=4.0, rounds=2, **kw):
    """the first scene of seeds seed, seed + 1000, ... whose restatement is decided -> (table, reference)"""
    for attempt in range(20):
        t = scene(np.random.default_rng(seed + 1000 * attempt), *args, **kw)
        ref = reference(t, px, rounds)
        if decided(ref):
            return t, ref
    raise AssertionError("no decided scene in 20 seeds")


def families(seed=7):
    """the issue's batch: 64 tracks of 2 .. 12 views over 6 cameras, 0.5 px noise, 10 % outliers of 30 .. 100 px; with the
    call's defaults (4 px, 2 rounds)"""
    lengths = np.random.default_rng(seed).integers(2, 13, 64)
    return decided_scene(seed, lengths, 6, noise=0.5, outliers=0.1)


SEAM_LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 200, 5000)


def seams(seed=11):
    """tracks of the lengths at which the kernel's slots, registers and chunks change, one of 5000 positions among them"""
    return decided_scene(seed, np.array(SEAM_LENGTHS), 12, noise=0.5, outliers=0.1)


def subset(t, tracks):
    """the table of the given tracks of t, in that order (the pool, the cameras and the rows stay)"""
    off = np.asarray(t["track_offsets"]).astype(np.int64)
    idx = np.concatenate([np.arange(off[i], off[i + 1]) for i in tracks] + [np.zeros(0, np.int64)]).astype(np.int64)
    new = np.concatenate([[0], np.cumsum([off[i + 1] - off[i] for i in tracks])]).astype(np.uint64)
    out = dict(t)
    out.update(track_offsets=new, obs_row=np.asarray(t["obs_row"])[idx], obs_image=np.asarray(t["obs_image"])[idx],
               counts=np.array([len(tracks), len(idx)], np.uint32))
    return out


def _plain(seed, lengths, n_images):
    return scene(np.random.default_rng(seed), np.array(lengths), n_images, noise=0.5, outliers=0.0)


def with_cameras(t, K_rows, P_rows):
    """t with more images at the end of its camera arrays -> (table, the first new image id)"""
    out = dict(t)
    first = len(t["intrinsics"])
    out["intrinsics"] = np.concatenate([t["intrinsics"], np.asarray(K_rows, np.float32).reshape(-1, 4)])
    out["poses"] = np.concatenate([t["poses"], np.asarray(P_rows, np.float32).reshape(-1, 12)])
    return out, first


def unusable_causes(seed=21):
    """8 tracks of 6 clean views; in each, one or two positions are made unusable by one cause each: a row outside the pool
    (-1, n_rows), an image id of 0xFFFFFFFF and of n_images, an all-zero R (with a non-zero t), a NaN pose entry, an infinite
    t, fx = 0, fy < 0, a NaN intrinsic, a NaN x and an infinite y.  -> (table, the positions made unusable)"""
    t = _plain(seed, [6] * 8, 8)
    good_K, good_P = t["intrinsics"][0], t["poses"][0]
    P_zero = np.concatenate([np.zeros(9), [1, 2, 3]])
    P_nan, P_inf = good_P.copy(), good_P.copy()
    P_nan[4], P_inf[10] = np.nan, np.inf
    K_fx0, K_fyneg, K_nan = good_K.copy(), good_K.copy(), good_K.copy()
    K_fx0[0], K_fyneg[1], K_nan[2] = 0.0, -800.0, np.nan
    t, new = with_cameras(t, [good_K, good_K, good_K, K_fx0, K_fyneg, K_nan], [P_zero, P_nan, P_inf, good_P, good_P, good_P])
    n_images, n_rows = len(t["intrinsics"]), len(t["kps"])
    row, img, kps = t["obs_row"].copy(), t["obs_image"].copy(), t["kps"].copy()
    bad = []
    row[0 * 6 + 1], row[0 * 6 + 4] = -1, n_rows
    img[1 * 6 + 0], img[1 * 6 + 3] = 0xFFFFFFFF, n_images
    for k, cam in ((2 * 6 + 2, 0), (3 * 6 + 5, 1), (3 * 6 + 0, 2), (4 * 6 + 1, 3), (4 * 6 + 2, 4), (5 * 6 + 3, 5)):
        img[k] = new + cam
        bad.append(k)
    kps[row[6 * 6 + 2], 0], kps[row[7 * 6 + 5], 1] = np.nan, np.inf
    bad += [1, 4, 6, 9, 6 * 6 + 2, 7 * 6 + 5]
    t.update(obs_row=row, obs_image=img, kps=kps)
    return t, sorted(bad)


def no_point_reasons(seed=22):
    """tracks that end with each reason, in this order: 0 a point; 1 an empty track, a track of one position, a track of four
    with one usable; 2 three observations of one keypoint in one image (every pair singular); 3 two views that do not agree
    (no hypothesis has two inliers), and a point behind both cameras' image planes"""
    t = _plain(seed, [5, 0, 1, 4, 3, 2, 2], 6)
    off = t["track_offsets"].astype(np.int64)
    row, img, kps = t["obs_row"].copy(), t["obs_image"].copy(), t["kps"].copy()
    img[off[3] + 1:off[4]] = 0xFFFFFFFF
    row[off[4]:off[5]], img[off[4]:off[5]] = row[off[4]], img[off[4]]
    kps[row[off[5]], :2] += (60.0, -45.0)
    # the last track's two observations mirrored through their principal points: the rays meet behind the cameras
    for k in (off[6], off[6] + 1):
        c = t["intrinsics"][img[k], 2:]
        kps[row[k], :2] = 2 * c - kps[row[k], :2]
    t.update(obs_row=row, obs_image=img, kps=kps)
    return t, [0, 1, 1, 1, 2, 3, 3]


def shared_slots(seed=23):
    """one track of 27 positions whose usable ones are 0, 8, 16, 24 (all slot 0), 3, 11 (slot 3) and 26, the positions in
    between observations of an image that is not registered; and a second, plain track"""
    t = _plain(seed, [27, 4], 9)
    t, new = with_cameras(t, [t["intrinsics"][0]], [np.zeros(12)])
    img = t["obs_image"].copy()
    keep = {0, 8, 16, 24, 3, 11, 26}
    for k in range(27):
        if k not in keep:
            img[k] = new
    t.update(obs_image=img)
    return t


def reading_rules(seed=24):
    """six clean tracks read under every rule: -> [(name, table)]; the tables' arrays are longer or shorter than their counts
    say"""
    base = _plain(seed, [3, 5, 2, 9, 4, 6], 6)
    n_t, n_o = 6, int(base["track_offsets"][-1])
    out = []

    def variant(name, counts=None, off=None):
        t = dict(base)
        if counts is not None:
            t["counts"] = np.array(counts, np.uint32)
        if off is not None:
            t["track_offsets"] = np.array(off, np.uint64)
        out.append((name, t))

    variant("as made")
    variant("fewer tracks than the capacity", counts=(4, n_o))              # rows 4 and 5 untouched
    variant("more tracks than the capacity", counts=(1000, n_o))
    variant("more observations than the capacity", counts=(n_t, 0xFFFFFFFF))
    variant("fewer observations: offsets beyond O", counts=(n_t, 12))       # tracks end at 12, later ones are empty
    variant("no observations", counts=(n_t, 0))
    variant("no tracks", counts=(0, n_o))
    off = base["track_offsets"].astype(np.int64).copy()
    off[-1] = off[-2] - 3                                                   # the last track's range is inverted
    variant("an inverted range", off=off)
    off = base["track_offsets"].astype(np.int64).copy()
    off[-1] = 1 << 40
    off[-2] = 1 << 33                                                       # past everything: clamped to O
    variant("offsets past 2^32", off=off)
    return out
