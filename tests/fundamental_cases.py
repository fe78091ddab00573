"""Synthetic two-view problems the fundamental-matrix tests share (tests/test_fundamental_api.py,
tests/test_gpu_fundamental.py, tests/test_fundamental_twin.py, tests/test_gpu_fundamental_exact.py): random 3-D points
seen by two cameras with known K, R and t, so that
F_true = K^-T [t]x R K^-1 (b^T F a = 0 for a in view 1 and b in view 2), with 0.5 px noise and planted outliers."""
import numpy as np

THR = 1.5
WIDTH, HEIGHT = 1024, 768
K = np.array([[800.0, 0.0, WIDTH / 2], [0.0, 800.0, HEIGHT / 2], [0.0, 0.0, 1.0]])
FAMILIES = ("general", "sideways", "forward", "near_planar", "duplicates")


def rotation(rx, ry, rz):
    """Rotation by rx, ry, rz degrees about x, y, z (applied in that order)."""
    ax, ay, az = np.deg2rad([rx, ry, rz])
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx_ = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry_ = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz_ = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rz_ @ ry_ @ rx_


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def f_true(r, t, k=K):
    ki = np.linalg.inv(k)
    f = ki.T @ skew(t) @ r @ ki
    return f / np.abs(f).max()


MOTIONS = {   # (R, t) of camera 2 relative to camera 1
    "general": (rotation(2.0, -4.0, 3.0), np.array([0.8, 0.15, 0.3])),
    "sideways": (np.eye(3), np.array([1.0, 0.0, 0.0])),            # epipoles at infinity: F33 = 0
    "forward": (rotation(0.5, 1.0, 0.0), np.array([0.02, -0.01, 1.0])),   # epipole inside the image
    "near_planar": (rotation(1.0, -3.0, 2.0), np.array([0.7, 0.2, 0.2])),
    "duplicates": (rotation(-2.0, 3.0, -1.0), np.array([-0.6, 0.3, 0.25])),
}


def _project(k, x):
    p = x @ k.T
    return p[:, :2] / p[:, 2:]


def scene(g, m, family, depth=(4.0, 12.0)):
    """m 3-D points in front of both cameras and inside both frames (a few margins of slack): (X, a, b) noise-free."""
    r, t = MOTIONS[family]
    pts, a_all, b_all = [], [], []
    while sum(len(p) for p in pts) < m:
        n = 4 * m + 64
        uv = g.uniform([-100, -100], [WIDTH + 100, HEIGHT + 100], (n, 2))
        if family == "near_planar":   # a plane 8 units away, tilted, plus 2 % of depth relief
            z = 8.0 + 0.3 * (uv[:, 0] - WIDTH / 2) / WIDTH + g.uniform(-0.08, 0.08, n)
        else:
            z = g.uniform(*depth, n)
        x = np.concatenate([(uv - K[:2, 2]) / K[0, 0] * z[:, None], z[:, None]], axis=1)
        x2 = x @ r.T + t
        ok = x2[:, 2] > 0.5
        a, b = _project(K, x[ok]), _project(K, x2[ok])
        inside = (b[:, 0] > -100) & (b[:, 0] < WIDTH + 100) & (b[:, 1] > -100) & (b[:, 1] < HEIGHT + 100)
        pts.append(x[ok][inside])
        a_all.append(a[inside])
        b_all.append(b[inside])
    return np.concatenate(pts)[:m], np.concatenate(a_all)[:m], np.concatenate(b_all)[:m]


def _rows(a, b):
    ka, kb = np.zeros((len(a), 5), np.float32), np.zeros((len(b), 5), np.float32)
    ka[:, :2], kb[:, :2] = a, b
    ka[:, 2] = kb[:, 2] = 4.0
    return ka, kb


def two_view(m, outliers, seed, family="general", sigma=0.5):
    """m matches of `family` (kps as [m,5] f32, identity match array), a fraction `outliers` replaced by random points of
    view 2; returns (ka, kb, match, info) with info = F_true, the noise-free b, the inlier mask."""
    g = np.random.default_rng(seed)
    _, a, b = scene(g, m, family)
    bn = b + g.normal(0, sigma, b.shape)
    out = g.random(m) < outliers
    bn[out] = g.uniform([0, 0], [WIDTH, HEIGHT], (int(out.sum()), 2))
    if family == "duplicates":   # a fifth of the rows repeat another row exactly (a and b): duplicates in samples
        dup = g.random(m) < 0.2
        src = g.integers(0, m, int(dup.sum()))
        a[dup], bn[dup], b[dup], out[dup] = a[src], bn[src], b[src], out[src]
    ka, kb = _rows(a, bn)
    return ka, kb, np.arange(m, dtype=np.int32), {"F": f_true(*MOTIONS[family]), "a": a, "b": b, "inlier": ~out}


def band(prob, f, thr=THR, rel=0.05):
    """Considered matches whose Sampson error under f lies within `rel` of thr^2 (where f32 and f64 may disagree)."""
    e = prob.error(f)
    return ~np.isfinite(e) | (np.abs(e - thr * thr) <= rel * thr * thr)


def f32_band(prob, f, thr=THR, roundings=16):
    """Considered matches that f32 arithmetic in pixel coordinates cannot decide under f: e = b . F a is a sum of nine
    products b_j F_jk a_k, and F's entries (after the denormalisation: up to 6 roundings on the constant entry) and the
    Sampson test's fused steps (2 per line coefficient, 3 for e) each round at 2^-24 of a partial sum no larger than
    T = sum |b_j F_jk a_k|.  So the computed |e| is off by at most roundings * 2^-24 * T with roundings = 16, and a match is
    undecided when | |e| - thr sqrt(l0^2 + l1^2 + l'0^2 + l'1^2) | is within that.  For coordinates within a frame at the
    origin this is a fraction of the 5 % band; at an offset C it grows with C^2, and at a threshold below f32's
    resolution it is what remains."""
    f = np.asarray(f, np.float64).reshape(3, 3)
    ah = np.concatenate([prob.a, np.ones((prob.m, 1))], axis=1)
    bh = np.concatenate([prob.b, np.ones((prob.m, 1))], axis=1)
    with np.errstate(all="ignore"):
        t = np.einsum("ij,jk,ik->i", np.abs(bh), np.abs(f), np.abs(ah))
        num, den = prob.sampson(f)
        gap = np.abs(np.sqrt(num) - thr * np.sqrt(den))
        return ~np.isfinite(gap) | (gap <= roundings * 2.0 ** -24 * t)


def undecided(prob, f, thr=THR):
    """band() or f32_band(): the matches on which an f32 and an f64 evaluation of the Sampson test under f may differ."""
    return band(prob, f, thr) | f32_band(prob, f, thr)


def pairs(n_pairs=48):
    """A ragged batch: empty pairs, M < 7, M = 7 exactly, and ordinary problems of every family with rows that do not
    count (-1 and out-of-range matches) and b rows nobody matches."""
    g = np.random.default_rng(7)
    out = []
    for p in range(n_pairs):
        kind = p % 8
        if kind == 0:
            ka, kb, mt = np.zeros((0, 5), np.float32), np.zeros((0, 5), np.float32), np.zeros(0, np.int32)
        elif kind == 1:
            ka, kb, mt, _ = two_view(6, 0.0, p)
        elif kind == 2:
            ka, kb, mt, _ = two_view(7, 0.0, p)
        else:
            n = int(g.integers(20, 1500))
            ka, kb, mt, _ = two_view(n, float(g.uniform(0.1, 0.6)), 2000 + p, FAMILIES[p % len(FAMILIES)])
            extra = g.uniform(0, 1000, (n // 3, 5)).astype(np.float32)
            kb = np.concatenate([kb, extra])
            perm = g.permutation(len(kb))
            inv = np.argsort(perm)
            kb, mt = kb[perm], inv[mt].astype(np.int32)
            mt[g.random(n) < 0.25] = -1
            mt[g.random(n) < 0.02] = len(kb) + 3
        out.append((ka, kb, mt))
    return out


# ---- edge cases (tests/test_fundamental_twin.py: twin against the restatement; tests/test_gpu_fundamental_exact.py: device
# against the twin).  What include/lf_mkd.h promises of each is asserted by those tests. -------------------------------
THR_MIN, THR_MAX = 1.0842022e-19, 1.8446743e19   # the smallest and the largest threshold the entry points accept


def _with_outliers(g, a, b, outliers, sigma):
    m = len(a)
    bn = b + g.normal(0, sigma, b.shape)
    out = g.random(m) < outliers
    bn[out] = g.uniform([0, 0], [WIDTH, HEIGHT], (int(out.sum()), 2))
    ka, kb = _rows(a, bn)
    return ka, kb, np.arange(m, dtype=np.int32)


def _plane_points(g, m):
    """m points of the plane Z = 8 + 0.3 (x - W/2) / W seen by the near_planar cameras: b is a homography of a."""
    r, t = MOTIONS["near_planar"]
    uv = g.uniform([0, 0], [WIDTH, HEIGHT], (m, 2))
    z = 8.0 + 0.3 * (uv[:, 0] - WIDTH / 2) / WIDTH
    x = np.concatenate([(uv - K[:2, 2]) / K[0, 0] * z[:, None], z[:, None]], axis=1)
    return _project(K, x), _project(K, x @ r.T + t)


def edge_cases(m=200):
    """[(name, ka, kb, match, threshold)]: degenerate geometry, repeated rows, a large coordinate offset and the two ends of
    the threshold's range."""
    g = np.random.default_rng(23)
    out = []
    a, b = _plane_points(g, m)
    out.append(("plane_exact", *_with_outliers(g, a, b, 0.0, 0.0), THR))
    out.append(("plane_noisy", *_with_outliers(g, a, b, 0.3, 0.5), THR))
    ka, kb, mt, _ = two_view(m, 0.3, 31)
    ka[:, 1] = np.float32(0.3) * ka[:, 0] + np.float32(100.0)          # every a point on one line
    out.append(("collinear_a", ka, kb, mt, THR))
    ka, kb = _rows(np.tile([[100.0, 200.0]], (50, 1)), np.tile([[300.0, 250.0]], (50, 1)))
    out.append(("identical_rows", ka, kb, np.arange(50, dtype=np.int32), THR))
    a8 = np.tile([[400.0, 300.0]], (8, 1))
    b8 = np.tile([[420.0, 310.0]], (8, 1))
    a8[7], b8[7] = (100.0, 50.0), (140.0, 90.0)
    out.append(("seven_repeated", *_rows(a8, b8), np.arange(8, dtype=np.int32), THR))
    rot = K @ rotation(2.0, -4.0, 3.0) @ np.linalg.inv(K)               # t = 0: b = K R K^-1 a, a homography
    a = g.uniform([0, 0], [WIDTH, HEIGHT], (m, 2))
    bh = np.concatenate([a, np.ones((m, 1))], axis=1) @ rot.T
    out.append(("pure_rotation", *_with_outliers(g, a, bh[:, :2] / bh[:, 2:], 0.3, 0.5), THR))
    ka, kb, mt, _ = two_view(m, 0.4, 37)
    ka[:, :2] += np.float32(1e5)
    kb[:, :2] += np.float32(1e5)
    out.append(("large_offset", ka, kb, mt, THR))
    ka, kb, mt, _ = two_view(m, 0.4, 41)
    out.append(("threshold_min", ka, kb, mt, THR_MIN))
    out.append(("threshold_max", ka, kb, mt, THR_MAX))
    return out


BAD_ROW = 5


def non_finite(bad, m=300):
    """Four copies of one problem with `bad` (NaN, +Inf or -Inf) in considered row BAD_ROW: a.x, a.y, b.x, b.y."""
    ka, kb, mt, _ = two_view(m, 0.4, 43)
    out = []
    for which, col in ((0, 0), (0, 1), (1, 0), (1, 1)):
        a, b = ka.copy(), kb.copy()
        (a if which == 0 else b)[BAD_ROW, col] = bad
        out.append((a, b, mt))
    return out
