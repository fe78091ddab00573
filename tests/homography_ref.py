"""CPU restatement of lf_mkd_verify_homography (include/lf_mkd.h, steps 1-6) in numpy float64.

The sampler is exact integer arithmetic, so every hypothesis draws the same four matches as on the device; the minimal
solver, the scores and the refit are the same formulas in float64 (the refit by an SVD least-squares solve), so a device
count may differ from this one only for points whose squared transfer error lies within rounding of threshold^2."""
import numpy as np

MASK64 = (1 << 64) - 1
NO_REFINE = 1
DEGENERATE = 1e-4
INVALID = 0xFFFFFFFF


def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def sample(seed_p, k, m):
    """The first 4 distinct positions of hypothesis k (None if 32 draws give fewer)."""
    key = ((seed_p & 0xFFFFFFFF) << 32) ^ (k << 5)
    got = []
    for t in range(32):
        pos = ((splitmix64(key ^ t) >> 32) * m) >> 32
        if pos not in got:
            got.append(pos)
            if len(got) == 4:
                return got
    return None


def considered(kps_a, kps_b, match):
    """(row indices i, a points [M,2], b points [M,2]) of the considered matches, by ascending i."""
    match = np.asarray(match, np.int64)
    rows = np.flatnonzero((match >= 0) & (match < len(kps_b)))
    a = np.asarray(kps_a, np.float64).reshape(-1, 5)[rows, :2]
    b = np.asarray(kps_b, np.float64).reshape(-1, 5)[match[rows], :2]
    return rows, a, b


def normalisation(p):
    """(centroid, scale): RMS distance sqrt(2) from the centroid after scaling."""
    if len(p) == 0:
        return np.zeros(2), 1.0
    c = p.mean(axis=0)
    d = ((p - c) ** 2).sum()
    return c, (np.sqrt(2.0 * len(p) / d) if d > 0 else 1.0)


def _cross(p0, p1, p2):
    return (p1[0] - p0[0]) * (p2[1] - p0[1]) - (p2[0] - p0[0]) * (p1[1] - p0[1])


def _quad_ok(q):
    c = [_cross(q[0], q[1], q[2]), _cross(q[0], q[1], q[3]), _cross(q[0], q[2], q[3]), _cross(q[1], q[2], q[3])]
    return min(abs(v) for v in c) >= DEGENERATE


def square_to_quad(q):
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = q
    sx, sy = x0 - x1 + x2 - x3, y0 - y1 + y2 - y3
    dx1, dx2, dy1, dy2 = x1 - x2, x3 - x2, y1 - y2, y3 - y2
    den = dx1 * dy2 - dx2 * dy1
    g, h = sx * dy2 - dx2 * sy, dx1 * sy - sx * dy1
    return np.array([[(x1 - x0) * den + g * x1, (x3 - x0) * den + h * x3, x0 * den],
                     [(y1 - y0) * den + g * y1, (y3 - y0) * den + h * y3, y0 * den],
                     [g, h, den]])


def adjugate(a):
    return np.array([[a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1], a[0, 2] * a[2, 1] - a[0, 1] * a[2, 2], a[0, 1] * a[1, 2] - a[0, 2] * a[1, 1]],
                     [a[1, 2] * a[2, 0] - a[1, 0] * a[2, 2], a[0, 0] * a[2, 2] - a[0, 2] * a[2, 0], a[0, 2] * a[1, 0] - a[0, 0] * a[1, 2]],
                     [a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0], a[0, 1] * a[2, 0] - a[0, 0] * a[2, 1], a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]]])


def denormalise(hn, ca, sa, cb, sb):
    ta = np.array([[sa, 0, -sa * ca[0]], [0, sa, -sa * ca[1]], [0, 0, 1.0]])
    tb_inv = np.array([[1 / sb, 0, cb[0]], [0, 1 / sb, cb[1]], [0, 0, 1.0]])
    return tb_inv @ hn @ ta


class Problem:
    """One pair: the considered matches and their normalisation."""

    def __init__(self, kps_a, kps_b, match):
        self.rows, self.a, self.b = considered(kps_a, kps_b, match)
        self.na = len(np.asarray(match))
        self.m = len(self.rows)
        self.ca, self.sa = normalisation(self.a)
        self.cb, self.sb = normalisation(self.b)
        self.an = (self.a - self.ca) * self.sa
        self.bn = (self.b - self.cb) * self.sb

    def hypothesis(self, seed_p, k):
        """H (pixels, oriented so that the samples have w > 0) of hypothesis k, or None if it is invalid."""
        if self.m < 4:
            return None
        pos = sample(seed_p, k, self.m)
        if pos is None:
            return None
        qa, qb = self.an[pos], self.bn[pos]
        if not (_quad_ok(qa) and _quad_ok(qb)):
            return None
        hn = square_to_quad(qb) @ adjugate(square_to_quad(qa))
        big = np.abs(hn).max()
        if not (np.isfinite(big) and big > 0):
            return None
        hn = hn / big
        w = hn[2, 0] * qa[:, 0] + hn[2, 1] * qa[:, 1] + hn[2, 2]
        if not ((w > 0).all() or (w < 0).all()):
            return None
        if (w < 0).all():
            hn = -hn
        h = denormalise(hn, self.ca, self.sa, self.cb, self.sb)
        return h if np.isfinite(h).all() else None

    def residuals(self, h):
        """(w, squared forward transfer error) of every considered match under h."""
        u = h[0, 0] * self.a[:, 0] + h[0, 1] * self.a[:, 1] + h[0, 2]
        v = h[1, 0] * self.a[:, 0] + h[1, 1] * self.a[:, 1] + h[1, 2]
        w = h[2, 0] * self.a[:, 0] + h[2, 1] * self.a[:, 1] + h[2, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            e2 = (self.b[:, 0] - u / w) ** 2 + (self.b[:, 1] - v / w) ** 2
        return w, e2

    def inliers(self, h, thr):
        w, e2 = self.residuals(h)
        return (w > 0) & (e2 < thr * thr)

    def cost(self, h, thr):
        """Truncated quadratic (MSAC) cost: an inlier adds its squared transfer error, any other match thr^2."""
        w, e2 = self.residuals(h)
        inl = (w > 0) & (e2 < thr * thr)
        return float(np.where(inl, e2, thr * thr).sum())

    def refit(self, mask):
        """Least squares with h8 = 1 over the masked matches in normalised coordinates (SVD solve), in pixels."""
        x, y = self.an[mask, 0], self.an[mask, 1]
        u, v = self.bn[mask, 0], self.bn[mask, 1]
        if len(x) < 4:
            return None
        z, o = np.zeros_like(x), np.ones_like(x)
        r1 = np.stack([x, y, o, z, z, z, -x * u, -y * u], axis=1)
        r2 = np.stack([z, z, z, x, y, o, -x * v, -y * v], axis=1)
        sol, _, rank, _ = np.linalg.lstsq(np.concatenate([r1, r2]), np.concatenate([u, v]), rcond=None)
        if rank < 8:
            return None
        h = denormalise(np.append(sol, 1.0).reshape(3, 3), self.ca, self.sa, self.cb, self.sb)
        return h if np.isfinite(h).all() else None


def score_all(prob, seed_p, n_hyp, thr):
    """(counts [n_hyp] with -1 for invalid hypotheses, list of H or None)."""
    counts = np.full(n_hyp, -1, np.int64)
    hs = []
    for k in range(n_hyp):
        h = prob.hypothesis(seed_p, k)
        hs.append(h)
        if h is not None:
            counts[k] = int(prob.inliers(h, thr).sum())
    return counts, hs


def verify(kps_a, kps_b, match, n_hyp=2048, thr=3.0, seed=0, flags=0):
    """One pair as lf_mkd_verify_homography computes it: dict with H (scaled H[8] = 1, or zeros), verified [na], stats [4],
    plus what the tests look at: the problem, all counts and hypotheses, the final mask over the considered matches."""
    prob = Problem(kps_a, kps_b, match)
    counts, hs = score_all(prob, seed, n_hyp, thr)
    out = {"problem": prob, "counts": counts, "hyps": hs}
    verified = np.full(prob.na, -1, np.int32)
    if counts.max(initial=-1) < 0:
        out.update(H=np.zeros((3, 3)), verified=verified, stats=np.array([0, 0, INVALID, prob.m], np.int64), mask=None, k=None)
        return out
    k = int(np.argmax(counts))               # first index of the maximum: ties go to the smallest k
    h = hs[k]
    mask = prob.inliers(h, thr)
    n = int(mask.sum())
    cost = prob.cost(h, thr)
    if not flags & NO_REFINE:
        for _ in range(3):
            h2 = prob.refit(mask)
            if h2 is None:
                break
            mask2 = prob.inliers(h2, thr)
            cost2 = prob.cost(h2, thr)
            if cost2 > cost:      # a refit is kept unless its truncated quadratic cost rises
                break
            changed = bool((mask2 != mask).any())
            h, mask, n, cost = h2, mask2, int(mask2.sum()), cost2
            if not changed:
                break
    verified[prob.rows[mask]] = np.asarray(match, np.int64)[prob.rows[mask]]
    out.update(H=h / h[2, 2], verified=verified, stats=np.array([n, counts[k], k, prob.m], np.int64), mask=mask, k=k, h=h)
    return out


def map_points(h, pts):
    pts = np.asarray(pts, np.float64)
    q = np.concatenate([pts, np.ones((len(pts), 1))], axis=1) @ np.asarray(h, np.float64).T
    return q[:, :2] / q[:, 2:]
