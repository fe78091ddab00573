"""Cases for the camera resection call (lf_mkd_resect_cameras_device) and a float64 numpy restatement of its algorithm
(include/lf_mkd.h): quartic roots by numpy.roots, the same sampler, guards, selection and refit rules, plain sums.  The
restatement shares no code with csrc/mkd_resect_math.h; tests/test_resect_twin.py holds the twin to it.

A scene is a dict of the device call's arrays under its argument names (kps [rows, 5], image_offsets, row_track, points
[tracks, 4], counts, intrinsics, poses) plus `truth` [n_images, 12], the poses the keypoints were projected with, and `clean`
[rows], the rows that are true correspondences."""
import numpy as np

MASK = (1 << 64) - 1
COLLINEAR, LEAD_REL = 1e-12, 2.0 ** -20
NONE = 0xFFFFFFFF
SEAM_M = (0, 1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)   # 1025: the first M with two slices


def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def sample3(seed_i, k, M):
    """the 3 positions of sample k of image `seed_i` = seed + image id, or None"""
    if M < 3:
        return None
    key, got = ((seed_i & 0xFFFFFFFF) << 32) ^ (k << 6), []
    for t in range(64):
        pos = ((splitmix64(key ^ t) >> 32) * M) >> 32
        if pos not in got:
            got.append(pos)
            if len(got) == 3:
                return got
    return None


# ---- the generator ------------------------------------------------------------------------------------------------

def rotation(w):
    """Rodrigues"""
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def camera_points(rng, family, n, K):
    """n points in the camera's frame that it sees: a cloud at depths 4 .. 8, a tilted plane, or a deep corridor (what forward
    motion looks at: depths 2 .. 30)"""
    fx, fy, cx, cy = K
    px = np.stack([rng.uniform(0, 2 * cx, n), rng.uniform(0, 2 * cy, n)], 1)
    ray = np.stack([(px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy, np.ones(n)], 1)
    if family == "plane":
        nrm = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), -1.0])
        depth = (nrm @ np.array([0, 0, rng.uniform(4, 8)])) / (ray @ nrm)
    elif family == "forward":
        depth = rng.uniform(2, 30, n)
    else:
        depth = rng.uniform(4, 8, n)
    return ray * depth[:, None]


def image(rng, family, m, K, noise=0.5, wrong=0.3, extra=0.2):
    """one image: m correspondences (a share `wrong` of them with a keypoint somewhere else) among rows without a track or with
    a track without a point (a share `extra` of the rows); returns kps [rows, 5], track slot per row (-1: none, -2: a track with
    the "none" point), points [m, 3] f32, the true pose [12], clean [rows]"""
    R = rotation(rng.normal(0, 0.25, 3))
    t = rng.uniform(-1, 1, 3) if family != "forward" else np.array([0.1 * rng.normal(), 0.1 * rng.normal(), rng.uniform(-2, 2)])
    Xc = camera_points(rng, family, m, K)
    Xw = ((Xc - t) @ R).astype(np.float32)                     # X = R^T (Xc - t)
    p = Xw.astype(np.float64) @ R.T + t
    xy = np.stack([K[0] * p[:, 0] / p[:, 2] + K[2], K[1] * p[:, 1] / p[:, 2] + K[3]], 1) + rng.normal(0, noise, (m, 2))
    bad = rng.random(m) < wrong
    xy[bad] = np.stack([rng.uniform(0, 2 * K[2], bad.sum()), rng.uniform(0, 2 * K[3], bad.sum())], 1)
    n_extra = int(round(extra * m / max(1e-9, 1 - extra))) if m else 3
    rows = m + n_extra
    slot = np.full(rows, -1, np.int64)
    where = np.sort(rng.permutation(rows)[:m])
    slot[where] = np.arange(m)
    fill = np.flatnonzero(slot == -1)
    slot[fill[::2]] = -2
    kps = np.zeros((rows, 5), np.float32)
    kps[:, :2] = np.stack([rng.uniform(0, 2 * K[2], rows), rng.uniform(0, 2 * K[3], rows)], 1)
    kps[where, :2] = xy
    kps[:, 2] = 8.0
    clean = np.zeros(rows, bool)
    clean[where] = ~bad
    return kps, slot, Xw, np.concatenate([R.reshape(-1), t]).astype(np.float32), clean


def scene(seed, sizes, families=("cloud", "plane", "forward"), focal=1000.0, noise=0.5, wrong=0.3, extra=0.2):
    """images of sizes[i] correspondences, family i mod len(families); every pose all zero (not registered)"""
    rng = np.random.default_rng(seed)
    K = np.array([focal, focal, 640.0, 480.0])
    kps, rt, pts, truth, clean, off = [], [], [], [], [], [0]
    n_tracks = 0
    for i, m in enumerate(sizes):
        k, slot, Xw, pose, cl = image(rng, families[i % len(families)], m, K, noise, wrong, extra)
        track = np.where(slot >= 0, slot + n_tracks, -1)
        n_none = int((slot == -2).sum())
        track[slot == -2] = n_tracks + m + np.arange(n_none)
        pts.append(np.concatenate([np.concatenate([Xw, np.full((m, 1), 0.9, np.float32)], 1),
                                   np.tile(np.array([[0, 0, 0, 2]], np.float32), (n_none, 1))]))
        n_tracks += m + n_none
        kps.append(k), rt.append(track), truth.append(pose), clean.append(cl), off.append(off[-1] + len(k))
    n = len(sizes)
    return dict(kps=np.concatenate(kps), image_offsets=np.array(off, np.uint64), row_track=np.concatenate(rt).astype(np.int32),
                points=np.concatenate(pts), counts=np.array([n_tracks, 0], np.uint32),
                intrinsics=np.tile(K.astype(np.float32), (n, 1)), poses=np.zeros((n, 12), np.float32),
                truth=np.stack(truth), clean=np.concatenate(clean))


def families(seed=1):
    """twelve images of 3 .. 600 correspondences: cloud, plane, forward motion, 30 % wrong"""
    return scene(seed, (3, 7, 12, 40, 65, 100, 256, 257, 300, 420, 513, 600))


def seams(seed=2):
    return scene(seed, SEAM_M, wrong=0.2)


def realistic(seed=3, n=16):
    """the recovery case: 0.5 px noise, 30 % wrong, M 30 .. 400, planar scenes among them"""
    rng = np.random.default_rng(seed)
    return scene(seed, tuple(int(x) for x in rng.integers(30, 401, n)))


def sub_scene(s, images):
    """the images `images` of a scene alone, in that order, as a scene (the tracks are kept whole)"""
    off = s["image_offsets"].astype(np.int64)
    rows = np.concatenate([np.arange(off[i], off[i + 1]) for i in images]) if len(images) else np.zeros(0, np.int64)
    new_off = np.concatenate([[0], np.cumsum([off[i + 1] - off[i] for i in images])]).astype(np.uint64)
    r = dict(s)
    r.update(kps=s["kps"][rows], row_track=s["row_track"][rows], image_offsets=new_off, intrinsics=s["intrinsics"][list(images)],
             poses=s["poses"][list(images)], truth=s["truth"][list(images)], clean=s["clean"][rows])
    return r


def reading_rules(seed=4, counts_delta=0):
    """eight images of 80 correspondences and four more ranges -- empty, inverted, reaching beyond the pool, wholly beyond
    it --, rows whose track is -1, T and INT32_MAX, the "none" point, NaN and Inf in points and keypoints, parallax cosines on
    both sides of cos(5 degrees), unusable intrinsics, a non-finite pose and a registered image; counts_delta moves
    d_table_counts[0] below (negative) or above the capacity.  To be run at min_parallax_deg = 5."""
    s = scene(seed, (80,) * 8, wrong=0.1)
    off, n = s["image_offsets"].astype(np.int64), len(s["kps"])
    s["image_offsets"] = np.concatenate([off, [off[8], off[7], n + 50, n + 100]]).astype(np.uint64)
    s["intrinsics"] = np.concatenate([s["intrinsics"], s["intrinsics"][[7, 7, 7, 7]]])
    s["poses"] = np.zeros((12, 12), np.float32)
    s["truth"] = np.concatenate([s["truth"], s["truth"][[7, 7, 7, 7]]])
    T = len(s["points"])
    rt, pts, kps = s["row_track"], s["points"], s["kps"]
    first = np.arange(off[0], off[1])
    rows = first[(rt[first] >= 0) & (pts[np.maximum(rt[first], 0), 3] < 1.5)][:14]     # image 0's first correspondences, one rule each
    rt[rows[0]], rt[rows[1]], rt[rows[2]] = -1, T, 0x7FFFFFFF
    pts[rt[rows[3]]] = [0, 0, 0, 2]
    pts[rt[rows[4]], 0], pts[rt[rows[5]], 1], pts[rt[rows[6]], 2] = np.nan, np.inf, -np.inf
    pts[rt[rows[7]], 3], pts[rt[rows[8]], 3], pts[rt[rows[9]], 3] = np.nan, 0.999, 0.99     # cos(5 deg) = 0.99619
    kps[rows[10], 0], kps[rows[11], 1] = np.nan, np.inf
    near = np.float32(np.cos(np.radians(5.0)))                                   # the f32 values around cmin
    pts[rt[rows[12]], 3], pts[rt[rows[13]], 3] = np.nextafter(near, np.float32(2)), np.nextafter(near, np.float32(0))
    s["intrinsics"][2, 0] = 0.0
    s["intrinsics"][3, 3] = np.nan
    s["poses"][4, 10] = np.inf
    s["poses"][5] = s["truth"][5]
    s["counts"] = np.array([T + counts_delta, 0], np.uint32)
    return s


def reasons(seed=6):
    """one image per reason: 0 a pose; 1 registered; 2 two correspondences; 2 every point on one line (every triple collinear);
    3 every correspondence wrong"""
    good, junk = scene(seed, (120, 90, 2, 60), wrong=0.2), scene(seed + 1, (60,), wrong=1.0)
    off = good["image_offsets"].astype(np.int64)
    rows = np.arange(off[3], off[4])
    on = rows[good["row_track"][rows] >= 0]
    tr = good["row_track"][on]
    real = good["points"][tr, 3] < 1.5
    good["points"][tr[real], :3] = (np.array([0.5, -0.25, 6.0]) + np.linspace(-2, 2, real.sum())[:, None] * np.array([1.0, 0.5, 0.25])
                                    ).astype(np.float32)
    s = dict(good)
    n_t = len(good["points"])
    jt = junk["row_track"].copy()
    jt[jt >= 0] += n_t
    s.update(kps=np.concatenate([good["kps"], junk["kps"]]), row_track=np.concatenate([good["row_track"], jt]),
             points=np.concatenate([good["points"], junk["points"]]),
             image_offsets=np.concatenate([off, [off[-1] + len(junk["kps"])]]).astype(np.uint64),
             intrinsics=np.concatenate([good["intrinsics"], junk["intrinsics"]]), poses=np.zeros((5, 12), np.float32),
             truth=np.concatenate([good["truth"], junk["truth"]]), clean=np.concatenate([good["clean"], junk["clean"]]),
             counts=np.array([n_t + len(junk["points"]), 0], np.uint32))
    s["poses"][1] = s["truth"][1]
    return s


def chain(seed=8, n_points=700, noise=0.25):
    """five cameras around a cloud, camera 0 at [I | 0] and camera 1 at distance 1 from it (the gauge the pose call fixes); a
    point is seen by a random subset of at least two cameras.  Returns (kps [rows, 5] f32, image_offsets, edges (a, b) over
    every pair, matches per edge as arrays over image a's rows (the row within image b or -1), K [4], truth [5, 12], F [10, 9]
    f32: the true fundamental matrix of every edge)"""
    rng = np.random.default_rng(seed)
    K = np.array([1000.0, 1000.0, 640.0, 480.0])
    X = np.stack([rng.uniform(-3, 3, n_points), rng.uniform(-2, 2, n_points), rng.uniform(4, 8, n_points)], 1)
    centres = np.array([[0, 0, 0], [1, 0, 0], [-0.9, 0.3, 0.2], [0.4, -0.8, -0.3], [1.8, 0.5, 0.4]], np.float64)
    Rs = [np.eye(3)] + [rotation(rng.normal(0, 0.08, 3)) for _ in range(4)]
    truth = np.stack([np.concatenate([R.reshape(-1), -R @ c]) for R, c in zip(Rs, centres)])
    seen = rng.random((n_points, 5)) < 0.55
    seen[seen.sum(1) < 2] = True
    kps, row_of, off = [], [], [0]
    for i in range(5):
        ids = rng.permutation(np.flatnonzero(seen[:, i]))
        p = X[ids] @ Rs[i].T + truth[i, 9:]
        xy = np.stack([K[0] * p[:, 0] / p[:, 2] + K[2], K[1] * p[:, 1] / p[:, 2] + K[3]], 1) + rng.normal(0, noise, (len(ids), 2))
        k = np.zeros((len(ids), 5), np.float32)
        k[:, :2], k[:, 2] = xy, 8.0
        r = np.full(n_points, -1, np.int64)
        r[ids] = np.arange(len(ids))
        kps.append(k), row_of.append(r), off.append(off[-1] + len(ids))
    ea, eb, matches, Fs = [], [], [], []
    Kinv = np.linalg.inv(np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]]))
    for a in range(5):
        for b in range(a + 1, 5):
            m = np.full(off[a + 1] - off[a], -1, np.int32)
            both = np.flatnonzero(seen[:, a] & seen[:, b])
            m[row_of[a][both]] = row_of[b][both]
            R = Rs[b] @ Rs[a].T
            t = truth[b, 9:] - R @ truth[a, 9:]
            tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
            F = Kinv.T @ tx @ R @ Kinv
            ea.append(a), eb.append(b), matches.append(m), Fs.append((F / np.abs(F).max()).reshape(-1))
    return (np.concatenate(kps), np.array(off, np.int64), (np.array(ea, np.int32), np.array(eb, np.int32)), matches,
            K.astype(np.float32), truth, np.array(Fs, np.float32))


# ---- the restatement ----------------------------------------------------------------------------------------------

def correspondences(s, i, deg=0.0):
    """(rows, cs [M, 5] float64 = x, y, X, Y, Z) of image i by the reading rules"""
    kps, off, rt, pts = s["kps"], s["image_offsets"].astype(np.int64), s["row_track"], s["points"]
    n, T = len(kps), min(int(np.asarray(s["counts"]).reshape(-1)[0]), len(pts))
    lo, hi = min(off[i], n), min(off[i + 1], n)
    cmin = np.cos(np.float64(np.float32(deg)) * (np.pi / 180.0))
    rows = []
    for r in range(lo, max(lo, hi)):
        t = int(rt[r])
        if 0 <= t < T and np.isfinite(pts[t, :3]).all() and pts[t, 3] <= cmin and np.isfinite(kps[r, :2]).all():
            rows.append(r)
    rows = np.array(rows, np.int64)
    cs = np.concatenate([kps[rows, :2], pts[rt[rows], :3]], 1).astype(np.float64) if len(rows) else np.zeros((0, 5))
    return rows, cs


def candidate_image(K, P, resect_all):
    K, P = np.asarray(K, np.float64), np.asarray(P, np.float64)
    return bool(np.isfinite(K).all() and K[0] > 0 and K[1] > 0 and np.isfinite(P).all() and (resect_all or not P[:9].any()))


def bearings(xy, K):
    xn = np.stack([(xy[:, 0] - K[2]) / K[0], (xy[:, 1] - K[3]) / K[1], np.ones(len(xy))], 1)
    return xn / np.linalg.norm(xn, axis=1)[:, None]


def frame(P1, P2, P3):
    e1 = (P2 - P1) / np.linalg.norm(P2 - P1)
    e3 = np.cross(e1, P3 - P1)
    e3 = e3 / np.linalg.norm(e3)
    return np.stack([e1, np.cross(e3, e1), e3], 1)


def p3p(tri, K):
    """the candidates of a sample tri [3, 5]: None if the sample is invalid, else (the quartic's roots as numpy.roots gives
    them, {j: (R, t)} for the real roots j in ascending order whose pose is kept)"""
    f, X = bearings(tri[:, :2], K), tri[:, 2:]
    d12, d13, d23 = X[1] - X[0], X[2] - X[0], X[2] - X[1]
    a2, b2, c2 = d23 @ d23, d13 @ d13, d12 @ d12
    cr = np.cross(d12, d13)
    if not cr @ cr > COLLINEAR * c2 * b2:
        return None
    ca, cb, cg = f[1] @ f[2], f[0] @ f[2], f[0] @ f[1]
    with np.errstate(all="ignore"):
        p, q = (a2 - c2) / b2, (a2 + c2) / b2
        A4 = (p - 1) ** 2 - 4 * (c2 / b2) * ca ** 2
        A3 = 4 * (p * (1 - p) * cb - (1 - q) * ca * cg + 2 * (c2 / b2) * ca ** 2 * cb)
        A2 = 2 * (p ** 2 - 1 + 2 * p ** 2 * cb ** 2 + 2 * ((b2 - c2) / b2) * ca ** 2 - 4 * q * ca * cb * cg
                  + 2 * ((b2 - a2) / b2) * cg ** 2)
        A1 = 4 * (-p * (1 + p) * cb + 2 * (a2 / b2) * cg ** 2 * cb - (1 - q) * ca * cg)
        A0 = (1 + p) ** 2 - 4 * (a2 / b2) * cg ** 2
    A = np.array([A4, A3, A2, A1, A0])
    if not np.isfinite(A).all() or not abs(A4) > LEAD_REL * np.abs(A[1:]).max():
        return None
    roots = np.roots(A)
    real = np.sort(roots[roots.imag == 0].real)
    poses = {}
    for j, v in enumerate(real):
        with np.errstate(all="ignore"):
            den = 2 * (cg - v * ca)
            u = ((p - 1) * v * v - 2 * p * cb * v + 1 + p) / den if den != 0 else np.nan
            if not (v > 0 and den != 0 and u > 0):
                continue
            s1 = np.sqrt(b2 / (1 + v * v - 2 * v * cb))
            Y = np.stack([s1 * f[0], u * s1 * f[1], v * s1 * f[2]])
            R = frame(*Y) @ frame(*X).T
            t = Y[0] - R @ X[0]
        if np.isfinite(R).all() and np.isfinite(t).all():
            poses[j] = (R, t)
    return roots, poses


def unsafe_roots(roots, tol=1e-5):
    """is a sample's root structure too close to a change for two root finders to have to agree: two roots within tol
    (relative to max(1, |v|)) of each other, or a complex root within tol of the real axis"""
    for a in range(len(roots)):
        s = tol * max(1.0, abs(roots[a]))
        if roots[a].imag != 0 and abs(roots[a].imag) < s:
            return True
        for b in range(a + 1, len(roots)):
            if abs(roots[a] - roots[b]) < s and not (roots[a].imag != 0 and roots[b] == np.conj(roots[a])):
                return True
    return False


def errors2(R, t, K, cs):
    """(squared reprojection errors, in front) of the correspondences cs under (R, t)"""
    with np.errstate(all="ignore"):
        p = cs[:, 2:] @ R.T + t
        ex = K[0] * (p[:, 0] / p[:, 2]) + K[2] - cs[:, 0]
        ey = K[1] * (p[:, 1] / p[:, 2]) + K[3] - cs[:, 1]
        return ex * ex + ey * ey, p[:, 2] > 0


def inliers(R, t, K, cs, thr2):
    e2, front = errors2(R, t, K, cs)
    with np.errstate(invalid="ignore"):
        return front & (e2 <= thr2), e2


def msac(R, t, K, cs, thr2):
    is_in, e2 = inliers(R, t, K, cs, thr2)
    return float(np.where(is_in, e2, thr2).sum())


def cayley(w):
    wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return ((1 - w @ w) * np.eye(3) + 2 * np.outer(w, w) + 2 * wx) / (1 + w @ w)


def refit(R, t, K, cs, thr2, rounds):
    for _ in range(rounds):
        is_in, _ = inliers(R, t, K, cs, thr2)
        c = cs[is_in]
        q = c[:, 2:] @ R.T
        p = q + t
        ex = K[0] * p[:, 0] / p[:, 2] + K[2] - c[:, 0]
        ey = K[1] * p[:, 1] / p[:, 2] + K[3] - c[:, 1]
        J = np.zeros((len(c), 2, 6))
        for n in range(len(c)):
            de = np.array([[K[0] / p[n, 2], 0, -K[0] * p[n, 0] / p[n, 2] ** 2], [0, K[1] / p[n, 2], -K[1] * p[n, 1] / p[n, 2] ** 2]])
            qx = np.array([[0, -q[n, 2], q[n, 1]], [q[n, 2], 0, -q[n, 0]], [-q[n, 1], q[n, 0], 0]])
            J[n] = de @ np.concatenate([-2 * qx, np.eye(3)], 1)
        Jf, e = J.reshape(-1, 6), np.stack([ex, ey], 1).reshape(-1)
        H, g = Jf.T @ Jf, Jf.T @ e
        try:
            np.linalg.cholesky(H)
            d = -np.linalg.solve(H, g)
        except np.linalg.LinAlgError:
            break
        Rn, tn = cayley(d[:3]) @ R, t + d[3:]
        if not msac(Rn, tn, K, cs, thr2) <= msac(R, t, K, cs, thr2):
            break
        R, t = Rn, tn
    return R, t


def resect_image(cs, K, seed_i, px=4.0, n_samples=64, min_inliers=12, rounds=3):
    """the algorithm on one candidate image's correspondences -> dict stats [4], pose [12] f32, inlier [M] bool, err [2], tie
    (the two best candidates' counts are equal), counts {c: score}"""
    K = np.asarray(K, np.float64)
    M, thr2 = len(cs), float(np.float32(px)) ** 2
    counts, poses = {}, {}
    for k in range(n_samples):
        s = sample3(seed_i, k, M)
        got = p3p(cs[s], K) if s is not None else None
        for j, (R, t) in (got[1] if got else {}).items():
            counts[4 * k + j] = int(inliers(R, t, K, cs, thr2)[0].sum())
            poses[4 * k + j] = (R, t)
    res = dict(stats=[M, 0, 2, NONE], pose=np.zeros(12, np.float32), inlier=np.zeros(M, bool), err=[0.0, 0.0], tie=False,
               counts=counts)
    if not counts:
        return res
    order = sorted(counts, key=lambda c: (-counts[c], c))
    win = order[0]
    res["tie"] = len(order) > 1 and counts[order[1]] == counts[win]
    R, t = refit(*poses[win], K, cs, thr2, rounds)
    P = np.concatenate([R.reshape(-1), t]).astype(np.float32)
    is_in, e2 = inliers(P[:9].astype(np.float64).reshape(3, 3), P[9:].astype(np.float64), K, cs, thr2)
    n = int(is_in.sum())
    if n < max(min_inliers, 3):
        res["stats"] = [M, 0, 3, win]
        return res
    res.update(stats=[M, n, 0, win], pose=P, inlier=is_in, err=[float(np.sqrt(e2[is_in].sum() / n)), float(np.sqrt(e2[is_in].max()))])
    return res


def pose_error(P, truth):
    """(rotation error in radians, |t - t_true| / max(1, |t_true|)) of a pose [12] against the truth [12]"""
    P, Q = np.asarray(P, np.float64), np.asarray(truth, np.float64)
    c = (np.trace(P[:9].reshape(3, 3) @ Q[:9].reshape(3, 3).T) - 1) / 2
    return float(np.arccos(np.clip(c, -1, 1))), float(np.linalg.norm(P[9:] - Q[9:]) / max(1.0, np.linalg.norm(Q[9:])))
