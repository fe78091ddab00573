"""CPU restatement of lf_mkd_verify_fundamental (include/lf_mkd.h, steps 1-6) in numpy float64.

The sampler is exact integer arithmetic, so every sample draws the same seven matches as on the device.  The null space
follows the kernel's elimination and pivot rule, and the cubic, its bracketing and the candidates' order are the kernel's
formulas, all in float64.  So a device candidate c = 3 k + j is this module's candidate c unless f32 and f64 disagree on a
pivot or on the number of real roots, and a device count differs from this one only for points whose Sampson error lies
within rounding of threshold^2."""
import numpy as np

from homography_ref import considered, normalisation, splitmix64  # noqa: F401  (splitmix64: re-exported for the tests)

NO_REFINE = 1
INVALID = 0xFFFFFFFF
PIVOT_REL = 1e-5
LEAD_REL = 2.0 ** -20
JACOBI_SWEEPS = 6


def sample(seed_p, k, m):
    """The first 7 distinct positions of sample k (None if 64 draws give fewer, or m < 7)."""
    if m < 7:
        return None
    key = ((seed_p & 0xFFFFFFFF) << 32) ^ (k << 6)
    got = []
    for t in range(64):
        pos = ((splitmix64(key ^ t) >> 32) * m) >> 32
        if pos not in got:
            got.append(pos)
            if len(got) == 7:
                return got
    return None


def design_rows(an, bn):
    """[M, 9] rows [u x, u y, u, v x, v y, v, x, y, 1] of normalised matches a = (x, y), b = (u, v)."""
    x, y, u, v = an[:, 0], an[:, 1], bn[:, 0], bn[:, 1]
    return np.stack([u * x, u * y, u, v * x, v * y, v, x, y, np.ones_like(x)], axis=1)


def null_space(a, info=None):
    """(F1, F2) of the 7 x 9 system by Gauss-Jordan with full pivoting (the kernel's rule), or None if a pivot is not above
    PIVOT_REL times the first.  `info` (a dict) receives how close the decisions were: pivot_ratio = the smallest
    pivot / first pivot seen, pivot_tie = the smallest (pivot - runner-up) / pivot over the steps, the runner-up being the
    largest eligible |entry| strictly below the pivot (1 if there is none)."""
    a = np.array(a, np.float64)
    used_r, used_c, piv = set(), set(), {}
    first = None
    if info is not None:
        info.update(pivot_ratio=1.0, pivot_tie=1.0)
    for _ in range(7):
        best, pr, pc = -1.0, 0, 0
        for r in range(7):
            for c in range(9):
                if r not in used_r and c not in used_c and abs(a[r, c]) > best:
                    best, pr, pc = abs(a[r, c]), r, c
        first = best if first is None else first
        if info is not None and np.isfinite(best) and best > 0 and first > 0:
            free = np.abs(a[np.ix_([r for r in range(7) if r not in used_r], [c for c in range(9) if c not in used_c])])
            below = free[free < best]
            info["pivot_ratio"] = min(info["pivot_ratio"], best / first)
            if below.size:
                info["pivot_tie"] = min(info["pivot_tie"], (best - below.max()) / best)
        if not (best > PIVOT_REL * first) or not np.isfinite(best):
            return None
        prow = a[pr].copy()
        for r in range(7):
            if r != pr:
                a[r] = a[r] - (a[r, pc] / prow[pc]) * prow
                a[r, pc] = 0.0
        used_r.add(pr)
        used_c.add(pc)
        piv[pr] = pc
    free = [c for c in range(9) if c not in used_c]
    f1, f2 = np.zeros(9), np.zeros(9)
    f1[free[0]] = f2[free[1]] = 1.0
    for r, c in piv.items():
        f1[c] = -a[r, free[0]] / a[r, c]
        f2[c] = -a[r, free[1]] / a[r, c]
    return f1, f2


def cofactors(m):
    m = np.asarray(m, np.float64).reshape(9)
    return np.array([m[4] * m[8] - m[5] * m[7], m[5] * m[6] - m[3] * m[8], m[3] * m[7] - m[4] * m[6],
                     m[2] * m[7] - m[1] * m[8], m[0] * m[8] - m[2] * m[6], m[1] * m[6] - m[0] * m[7],
                     m[1] * m[5] - m[2] * m[4], m[2] * m[3] - m[0] * m[5], m[0] * m[4] - m[1] * m[3]])


def cubic_coefficients(f1, f2):
    """(c0, c1, c2, c3) of det(l F1 + (1 - l) F2) = det(G + l D), G = F2, D = F1 - F2."""
    g, d = np.asarray(f2, np.float64), np.asarray(f1, np.float64) - np.asarray(f2, np.float64)
    cg, cd = cofactors(g), cofactors(d)
    return float(g[:3] @ cg[:3]), float(cg @ d), float(cd @ g), float(d[:3] @ cd[:3])


def cubic_roots(c0, c1, c2, c3, bisect=80, newton=4, info=None):
    """Real roots, ascending, by the kernel's bracketing (three monotone pieces of [-R, R]), bisection and Newton.  `info`
    (a dict) receives how close the decisions were: lead = |c3| / max(|c0|, |c1|, |c2|), and end_value = the smallest
    |p(e)| / (|c3 e^3| + |c2 e^2| + |c1 e| + |c0|) over the derivative's roots e that cut the bracket (1 if there are none)."""
    big = max(abs(c0), abs(c1), abs(c2))
    if info is not None:
        with np.errstate(all="ignore"):
            info.update(lead=abs(c3) / big if big > 0 and np.isfinite(big) else np.inf, end_value=1.0)
    if not all(np.isfinite([c0, c1, c2, c3])) or not abs(c3) > LEAD_REL * big:
        return []
    p = lambda x: ((c3 * x + c2) * x + c1) * x + c0
    r_bound = 1.0 + big / abs(c3)
    t = 3.0 * c3
    disc = c2 * c2 - t * c1
    e1 = e2 = r_bound
    if disc > 0:
        s = np.sqrt(disc)
        q = -(c2 + np.copysign(s, c2))
        r1, r2 = q / t, c1 / q
        e1 = min(max(min(r1, r2), -r_bound), r_bound)
        e2 = min(max(max(r1, r2), -r_bound), r_bound)
        if info is not None:
            for e in (e1, e2):
                scale = abs(c3 * e ** 3) + abs(c2 * e * e) + abs(c1 * e) + abs(c0)
                info["end_value"] = min(info["end_value"], abs(p(e)) / scale if scale > 0 else 0.0)
    ends = [-r_bound, e1, e2, r_bound]
    roots = []
    for lo, hi in zip(ends[:-1], ends[1:]):
        neg_lo = p(lo) < 0
        if neg_lo == (p(hi) < 0):
            continue
        for _ in range(bisect):
            m = (lo + hi) * 0.5
            if (p(m) < 0) == neg_lo:
                lo = m
            else:
                hi = m
        r = (lo + hi) * 0.5
        for _ in range(newton):
            d = (t * r + 2 * c2) * r + c1
            with np.errstate(divide="ignore", invalid="ignore"):
                rn = r - p(r) / d
            if lo <= rn <= hi:
                r = rn
        roots.append(r)
    return roots


def denormalise(fn, ca, sa, cb, sb):
    """F in normalised coordinates -> pixels: Tb^T Fn Ta."""
    ta = np.array([[sa, 0, -sa * ca[0]], [0, sa, -sa * ca[1]], [0, 0, 1.0]])
    tb = np.array([[sb, 0, -sb * cb[0]], [0, sb, -sb * cb[1]], [0, 0, 1.0]])
    return tb.T @ np.asarray(fn, np.float64).reshape(3, 3) @ ta


def smallest_eigenvector(s, sweeps=JACOBI_SWEEPS):
    """The kernel's cyclic Jacobi on a symmetric 3x3: (eigenvalues, eigenvector of the smallest one)."""
    s = np.array(s, np.float64)
    v = np.eye(3)
    for _ in range(sweeps):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = s[p, q]
            if apq == 0.0:
                continue
            theta = (s[q, q] - s[p, p]) / (2.0 * apq)
            with np.errstate(over="ignore"):
                t = (-1.0 if theta < 0 else 1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
            c = 1.0 / np.sqrt(t * t + 1.0)
            sn = t * c
            rot = np.eye(3)
            rot[p, p] = rot[q, q] = c
            rot[p, q], rot[q, p] = sn, -sn
            s = rot.T @ s @ rot
            v = v @ rot
    d = np.diag(s)
    return d, v[:, int(np.argmin(d))]


def rank2(f):
    """F (I - v v^T), v the eigenvector of F^T F with the smallest eigenvalue (Jacobi)."""
    f = np.asarray(f, np.float64).reshape(3, 3)
    _, v = smallest_eigenvector(f.T @ f)
    return f - np.outer(f @ v, v)


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

    def sample_rows(self, seed_p, k):
        pos = sample(seed_p, k, self.m)
        return None if pos is None else design_rows(self.an[pos], self.bn[pos])

    def candidates(self, seed_p, k, info=None):
        """[3] list of (F pixels, Fn normalised scaled by its largest |entry|) or None, in the kernel's slot order.  `info`:
        as null_space's and cubic_roots', for this sample."""
        out = [None, None, None]
        a = self.sample_rows(seed_p, k)
        if a is None:
            return out
        ns = null_space(a, info)
        if ns is None:
            return out
        f1, f2 = ns
        d = f1 - f2
        for j, lam in enumerate(cubic_roots(*cubic_coefficients(f1, f2), info=info)):
            g = f2 + lam * d
            big = np.abs(g).max()
            if not (np.isfinite(big) and big > 0):
                continue
            fn = g / big
            f = denormalise(fn, self.ca, self.sa, self.cb, self.sb)
            if np.isfinite(f).all():
                out[j] = (f, fn)
        return out

    def sampson(self, f):
        """(numerator (b . F a)^2, denominator l0^2 + l1^2 + l'0^2 + l'1^2) of every considered match."""
        f = np.asarray(f, np.float64).reshape(3, 3)
        ah = np.concatenate([self.a, np.ones((self.m, 1))], axis=1)
        bh = np.concatenate([self.b, np.ones((self.m, 1))], axis=1)
        l, lp = ah @ f.T, bh @ f
        e = (bh * l).sum(axis=1)
        return e * e, l[:, 0] ** 2 + l[:, 1] ** 2 + lp[:, 0] ** 2 + lp[:, 1] ** 2

    def error(self, f):
        num, den = self.sampson(f)
        with np.errstate(divide="ignore", invalid="ignore"):
            return num / den

    def inliers(self, f, thr):
        num, den = self.sampson(f)
        return num < thr * thr * den

    def cost(self, f, thr):
        """MSAC: an inlier adds its Sampson error, any other match thr^2."""
        inl = self.inliers(f, thr)
        return float(np.where(inl, self.error(f), thr * thr).sum())

    def refit(self, mask, fn_cur):
        """(F pixels, Fn) of the least squares with f_c = 1 (c: the largest |entry| of the current Fn) over the masked matches,
        made rank 2; None if it is singular."""
        if mask.sum() < 8:
            return None
        a = design_rows(self.an[mask], self.bn[mask])
        c = int(np.argmax(np.abs(np.asarray(fn_cur).reshape(9))))
        rest = [i for i in range(9) if i != c]
        sol, _, rank, _ = np.linalg.lstsq(a[:, rest], -a[:, c], rcond=None)
        if rank < 8:
            return None
        f = np.ones(9)
        f[rest] = sol
        g = rank2(f).reshape(9)
        fn = g / np.abs(g).max()
        fp = denormalise(fn, self.ca, self.sa, self.cb, self.sb)
        return (fp, fn) if np.isfinite(fp).all() else None


def score_all(prob, seed_p, n_hyp, thr):
    """(counts [3 n_hyp] with -1 for invalid candidates, list of (F, Fn) or None), index c = 3 k + j."""
    counts = np.full(3 * n_hyp, -1, np.int64)
    cands = []
    for k in range(n_hyp):
        for j, cand in enumerate(prob.candidates(seed_p, k)):
            cands.append(cand)
            if cand is not None:
                counts[3 * k + j] = int(prob.inliers(cand[0], thr).sum())
    return counts, cands


def scale_f(f):
    """F divided by its entry of largest magnitude (the first in row-major order on a tie)."""
    f = np.asarray(f, np.float64).reshape(9)
    return (f / f[int(np.argmax(np.abs(f)))]).reshape(3, 3)


def verify(kps_a, kps_b, match, n_hyp=2048, thr=1.5, seed=0, flags=0):
    """One pair as lf_mkd_verify_fundamental computes it: dict with F (scaled, or zeros), verified [na], stats [4], plus the
    problem, all counts and candidates, the final mask over the considered matches and the unscaled pixel F `f`."""
    prob = Problem(kps_a, kps_b, match)
    counts, cands = score_all(prob, seed, n_hyp, thr)
    out = {"problem": prob, "counts": counts, "cands": cands}
    verified = np.full(prob.na, -1, np.int32)
    if counts.max(initial=-1) < 0:
        out.update(F=np.zeros((3, 3)), verified=verified, stats=np.array([0, 0, INVALID, prob.m], np.int64), mask=None, c=None)
        return out
    c = int(np.argmax(counts))               # first index of the maximum: ties go to the smallest c
    f, fn = cands[c]
    mask = prob.inliers(f, thr)
    n = int(mask.sum())
    cost = prob.cost(f, thr)
    if not flags & NO_REFINE:
        for _ in range(3):
            r = prob.refit(mask, fn)
            if r is None:
                break
            f2, fn2 = r
            mask2 = prob.inliers(f2, thr)
            cost2 = prob.cost(f2, thr)
            if cost2 > cost:
                break
            changed = bool((mask2 != mask).any())
            f, fn, mask, n, cost = f2, fn2, mask2, int(mask2.sum()), cost2
            if not changed:
                break
    verified[prob.rows[mask]] = np.asarray(match, np.int64)[prob.rows[mask]]
    out.update(F=scale_f(f), verified=verified, stats=np.array([n, counts[c], c, prob.m], np.int64), mask=mask, c=c, f=f)
    return out


def epipolar_distance(f, a, b):
    """Symmetric epipolar distance of correspondences a -> b under F: the mean of b's distance to F a and a's to F^T b."""
    f = np.asarray(f, np.float64).reshape(3, 3)
    ah = np.concatenate([np.asarray(a, np.float64), np.ones((len(a), 1))], axis=1)
    bh = np.concatenate([np.asarray(b, np.float64), np.ones((len(b), 1))], axis=1)
    l, lp = ah @ f.T, bh @ f
    e = np.abs((bh * l).sum(axis=1))
    return 0.5 * (e / np.hypot(l[:, 0], l[:, 1]) + e / np.hypot(lp[:, 0], lp[:, 1]))
