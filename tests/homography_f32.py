"""f32 twin of the homography verifier (csrc/mkd_verify.hip with mkd_homography_math.h): its operations in its order, on the CPU.

homography_ref.py restates the algorithm (include/lf_mkd.h, steps 1-6) in float64; this file transcribes the device code
instead, so that it gives the device's bits:
  * every f32 `*`, `+`, `-`, `/` and sqrtf is one correctly rounded numpy float32 operation (the kernel is compiled with
    contraction off, so `a*b - c*d` is three roundings), evaluated left to right as the source writes it;
  * fmaf is emulated exactly (fmaf below); fminf / fmaxf are np.fmin / np.fmax (llvm.minnum / maxnum ignore a NaN);
  * sums run in the kernel's order: each of 256 threads adds its own rows r = tid, tid + 256, ... (considered rows only),
    then a __shfl_xor butterfly within each wave of 64 (offsets 32 .. 1), then the four wave totals in order;
  * the refit's normal equations and Cholesky factorisation are the same f64 operations (Python floats).
The sampler is homography_ref.sample."""
import math

import numpy as np

from homography_ref import INVALID, NO_REFINE, sample

F32 = np.float32
THREADS = 256
DEGENERATE = F32(1e-4)
N_SUMS = 23


def fmaf(a, b, c):
    """Correctly rounded f32 a * b + c, elementwise.  The product of two f32 values is exact in f64; the f64 sum s can
    differ from the exact one only by its rounding error e (TwoSum), and rounding s to f32 is then wrong only when s is
    exactly an f32 midpoint and e != 0: there the result goes to the side e points to."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    shape = a.shape
    a, b, c = a.ravel(), b.ravel(), c.ravel()
    p = a.astype(np.float64) * b.astype(np.float64)
    c64 = c.astype(np.float64)
    with np.errstate(all="ignore"):
        s = p + c64
        r = np.array(s.astype(F32))
        # an f32 midpoint has at most 25 significant bits: the low 28 bits of its f64 fraction are zero
        cand = ((s.view(np.uint64) & np.uint64(0x0FFFFFFF)) == 0) & (r.astype(np.float64) != s) & np.isfinite(s)
        if cand.any():
            idx = np.nonzero(cand)
            ps, cs, ss, rs = p[idx], c64[idx], s[idx], r[idx]
            bb = ss - ps
            e = (ps - (ss - bb)) + (cs - bb)
            other = np.where(rs.astype(np.float64) > ss, np.nextafter(rs, F32(-np.inf)), np.nextafter(rs, F32(np.inf)))
            lo, hi = np.minimum(rs, other), np.maximum(rs, other)
            # (an infinite neighbour stands for 2^128, the first value past the f32 range)
            lo64 = np.where(np.isinf(lo), np.copysign(2.0 ** 128, lo.astype(np.float64)), lo.astype(np.float64))
            hi64 = np.where(np.isinf(hi), np.copysign(2.0 ** 128, hi.astype(np.float64)), hi.astype(np.float64))
            fix = (lo64 + (hi64 - lo64) * 0.5 == ss) & (e != 0)
            r[idx] = np.where(fix, np.where(e > 0, hi, lo), rs)
    return r.reshape(shape)


def block_sum(partials):
    """The kernel's block_sum of per-thread values [..., 256]: butterfly within each wave, then the 4 waves in order."""
    v = partials.reshape(partials.shape[:-1] + (THREADS // 64, 64))
    o = 32
    while o:
        v = v[..., :o] + v[..., o:2 * o]
        o //= 2
    w = v[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def thread_partials(rows, vals, na, dtype):
    """Per-thread running sums of vals [n, ...] (row rows[i] holds vals[i]; rows ascending): thread r % 256 adds its rows
    in ascending order, starting from 0."""
    vals = np.asarray(vals, dtype)
    acc = np.zeros((THREADS,) + vals.shape[1:], dtype)
    rows = np.asarray(rows, np.int64)
    for j in range((na + THREADS - 1) // THREADS):
        sel = (rows >= j * THREADS) & (rows < (j + 1) * THREADS)
        if sel.any():
            t = rows[sel] - j * THREADS
            acc[t] = acc[t] + vals[sel]
    return np.moveaxis(acc, 0, -1)


def inlier_cost(h, ax, ay, bx, by, thr2):
    """inlier_cost() for hypotheses h [K, 9] over points [M]: (inlier [K, M], cost f32 [K, M])."""
    h = np.asarray(h, F32).reshape(-1, 9)
    c = [h[:, i, None] for i in range(9)]
    with np.errstate(all="ignore"):
        u = fmaf(c[0], ax, fmaf(c[1], ay, c[2]))
        v = fmaf(c[3], ax, fmaf(c[4], ay, c[5]))
        w = fmaf(c[6], ax, fmaf(c[7], ay, c[8]))
        ex, ey = fmaf(bx, w, -u), fmaf(by, w, -v)
        num, den = fmaf(ex, ex, ey * ey), w * w
        inl = (w > 0) & (num < thr2 * den)
        cost = np.where(inl, num / den, thr2).astype(F32)
    return inl, cost


def _cross3(x0, y0, x1, y1, x2, y2):
    return (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)


def quad_ok(x, y):
    """x, y [K, 4] f32 -> bool [K]"""
    c0 = _cross3(x[:, 0], y[:, 0], x[:, 1], y[:, 1], x[:, 2], y[:, 2])
    c1 = _cross3(x[:, 0], y[:, 0], x[:, 1], y[:, 1], x[:, 3], y[:, 3])
    c2 = _cross3(x[:, 0], y[:, 0], x[:, 2], y[:, 2], x[:, 3], y[:, 3])
    c3 = _cross3(x[:, 1], y[:, 1], x[:, 2], y[:, 2], x[:, 3], y[:, 3])
    return np.fmin(np.fmin(np.abs(c0), np.abs(c1)), np.fmin(np.abs(c2), np.abs(c3))) >= DEGENERATE


def square_to_quad(x, y):
    """x, y [K, 4] f32 -> [K, 9] f32"""
    x0, x1, x2, x3 = (x[:, i] for i in range(4))
    y0, y1, y2, y3 = (y[:, i] for i in range(4))
    sx, sy = x0 - x1 + x2 - x3, y0 - y1 + y2 - y3
    dx1, dx2, dy1, dy2 = x1 - x2, x3 - x2, y1 - y2, y3 - y2
    den = dx1 * dy2 - dx2 * dy1
    g, hh = sx * dy2 - dx2 * sy, dx1 * sy - sx * dy1
    return np.stack([(x1 - x0) * den + g * x1, (x3 - x0) * den + hh * x3, x0 * den,
                     (y1 - y0) * den + g * y1, (y3 - y0) * den + hh * y3, y0 * den, g, hh, den], axis=1)


class Pair:
    """One pair as the device sees it: verify_prepare's list and normalisation, and everything computed from them."""

    def __init__(self, kps_a, kps_b, match):
        ka = np.ascontiguousarray(kps_a, F32).reshape(-1, 5)
        kb = np.ascontiguousarray(kps_b, F32).reshape(-1, 5)
        mt = np.ascontiguousarray(match, np.int32).reshape(-1)
        self.na, self.match = len(mt), mt
        self.rows = np.flatnonzero((mt >= 0) & (mt < len(kb)))
        self.m = len(self.rows)
        self.ax, self.ay = ka[self.rows, 0], ka[self.rows, 1]
        self.bx, self.by = kb[mt[self.rows], 0], kb[mt[self.rows], 1]
        with np.errstate(all="ignore"):
            s = block_sum(thread_partials(self.rows, np.stack([self.ax, self.ay, self.bx, self.by], 1), self.na, F32))
            inv = F32(1) / F32(self.m) if self.m else F32(0)
            self.ca = (s[0] * inv, s[1] * inv)
            self.cb = (s[2] * inv, s[3] * inv)
            x, y, u, v = self.ax - self.ca[0], self.ay - self.ca[1], self.bx - self.cb[0], self.by - self.cb[1]
            d = block_sum(thread_partials(self.rows, np.stack([x * x + y * y, u * u + v * v], 1), self.na, F32))
            self.sa = np.sqrt(F32(2) * F32(self.m) / d[0]) if d[0] > 0 else F32(1)
            self.sb = np.sqrt(F32(2) * F32(self.m) / d[1]) if d[1] > 0 else F32(1)
            # normalised coordinates, as hypothesis() and the refit's moments compute them
            self.xn, self.yn = (self.ax - self.ca[0]) * self.sa, (self.ay - self.ca[1]) * self.sa
            self.un, self.vn = (self.bx - self.cb[0]) * self.sb, (self.by - self.cb[1]) * self.sb

    def denormalise(self, n):
        """n [K, 9] -> (h [K, 9], all finite [K])"""
        sa, (ca0, ca1), (cb0, cb1) = self.sa, self.ca, self.cb
        with np.errstate(all="ignore"):
            x = np.empty_like(n)
            for r in range(3):
                x[:, 3 * r] = n[:, 3 * r] * sa
                x[:, 3 * r + 1] = n[:, 3 * r + 1] * sa
                x[:, 3 * r + 2] = n[:, 3 * r + 2] - x[:, 3 * r] * ca0 - x[:, 3 * r + 1] * ca1
            ib = F32(1) / self.sb
            h = np.empty_like(n)
            for c in range(3):
                h[:, c] = x[:, c] * ib + cb0 * x[:, 6 + c]
                h[:, 3 + c] = x[:, 3 + c] * ib + cb1 * x[:, 6 + c]
                h[:, 6 + c] = x[:, 6 + c]
        return h, np.isfinite(h).all(axis=1)

    def hypotheses(self, seed_p, ks):
        """hypothesis() for every k in ks (seed_p: one seed, or one per k): (valid [K], H [K, 9] f32 in pixels; rows of
        invalid ones are meaningless)."""
        ks = np.asarray(ks, np.int64).reshape(-1)
        seeds = np.broadcast_to(np.asarray(seed_p, np.int64) & 0xFFFFFFFF, ks.shape)
        K = len(ks)
        valid = np.zeros(K, bool)
        h = np.zeros((K, 9), F32)
        if self.m < 4 or K == 0:
            return valid, h
        pos = np.zeros((K, 4), np.int64)
        for i, k in enumerate(ks):
            s = sample(int(seeds[i]), int(k), self.m)
            if s is not None:
                valid[i] = True
                pos[i] = s
        with np.errstate(all="ignore"):
            ax, ay, bx, by = self.xn[pos], self.yn[pos], self.un[pos], self.vn[pos]
            valid &= quad_ok(ax, ay) & quad_ok(bx, by)
            A, B = square_to_quad(ax, ay), square_to_quad(bx, by)
            J = np.stack([A[:, 4] * A[:, 8] - A[:, 5] * A[:, 7], A[:, 2] * A[:, 7] - A[:, 1] * A[:, 8],
                          A[:, 1] * A[:, 5] - A[:, 2] * A[:, 4], A[:, 5] * A[:, 6] - A[:, 3] * A[:, 8],
                          A[:, 0] * A[:, 8] - A[:, 2] * A[:, 6], A[:, 2] * A[:, 3] - A[:, 0] * A[:, 5],
                          A[:, 3] * A[:, 7] - A[:, 4] * A[:, 6], A[:, 1] * A[:, 6] - A[:, 0] * A[:, 7],
                          A[:, 0] * A[:, 4] - A[:, 1] * A[:, 3]], axis=1)
            n = np.empty((K, 9), F32)
            big = np.zeros(K, F32)
            for r in range(3):
                for c in range(3):
                    n[:, 3 * r + c] = B[:, 3 * r] * J[:, c] + B[:, 3 * r + 1] * J[:, 3 + c] + B[:, 3 * r + 2] * J[:, 6 + c]
                    big = np.fmax(big, np.abs(n[:, 3 * r + c]))
            valid &= (big > 0) & np.isfinite(big)
            ib = F32(1) / big
            n = n * ib[:, None]
            w = n[:, 6, None] * ax + n[:, 7, None] * ay + n[:, 8, None]
            npos, nneg = (w > 0).sum(axis=1), (w < 0).sum(axis=1)
            valid &= (npos == 4) | (nneg == 4)
            n = np.where((nneg == 4)[:, None], -n, n)
            h, finite = self.denormalise(n)
        valid &= finite
        return valid, h

    def inliers(self, h, thr2):
        return inlier_cost(h, self.ax, self.ay, self.bx, self.by, thr2)

    def counts(self, seed_p, n_hyp, thr2, chunk=1 << 22):
        """ransac_score<HomographyModel> summed over the slices: (counts int64 [n_hyp], -1 for an invalid hypothesis; valid; H)."""
        valid, h = self.hypotheses(seed_p, np.arange(n_hyp))
        counts = np.full(n_hyp, -1, np.int64)
        step = max(1, chunk // max(self.m, 1))
        for k0 in range(0, n_hyp, step):
            sel = np.flatnonzero(valid[k0:k0 + step]) + k0
            if len(sel):
                counts[sel] = self.inliers(h[sel], thr2)[0].sum(axis=1)
        return counts, valid, h

    def moments(self, inl):
        """add_moments over the rows in `inl` [M]: per-thread f64 partials [23, 256]."""
        x, y = self.xn.astype(np.float64), self.yn.astype(np.float64)
        u, v = self.un.astype(np.float64), self.vn.astype(np.float64)
        xx, xy, yy, R = x * x, x * y, y * y, u * u + v * v
        mom = np.stack([xx, xy, yy, x, y, np.ones_like(x), u * xx, u * xy, u * yy, u * x, u * y, v * xx, v * xy, v * yy,
                        v * x, v * y, R * xx, R * xy, R * yy, u, v, R * x, R * y], axis=1)
        return thread_partials(self.rows[inl], mom[inl], self.na, np.float64)

    def cost_sum(self, cost):
        return float(block_sum(thread_partials(self.rows, cost.astype(np.float64), self.na, np.float64)))


def _fmax(a, b):
    """fmax(): a NaN operand is ignored"""
    return b if math.isnan(a) else a if math.isnan(b) else max(a, b)


def solve_refit(m):
    """solve_refit(): the 8x8 normal equations from the 23 sums, Cholesky in f64 -> (ok, n [9] f32)."""
    N = [[0.0] * 8 for _ in range(8)]
    N[0][0] = N[3][3] = m[0]; N[0][1] = N[3][4] = m[1]; N[1][1] = N[4][4] = m[2]
    N[0][2] = N[3][5] = m[3]; N[1][2] = N[4][5] = m[4]; N[2][2] = N[5][5] = m[5]
    N[0][6] = -m[6]; N[0][7] = -m[7]; N[1][6] = -m[7]; N[1][7] = -m[8]; N[2][6] = -m[9]; N[2][7] = -m[10]
    N[3][6] = -m[11]; N[3][7] = -m[12]; N[4][6] = -m[12]; N[4][7] = -m[13]; N[5][6] = -m[14]; N[5][7] = -m[15]
    N[6][6] = m[16]; N[6][7] = m[17]; N[7][7] = m[18]
    r = [m[9], m[10], m[19], m[14], m[15], m[20], -m[21], -m[22]]
    dmax = 0.0
    for i in range(8):
        dmax = _fmax(dmax, N[i][i])
    floor = 1e-12 * dmax
    ok = dmax > 0.0
    for j in range(8):
        d = N[j][j]
        for k in range(j):
            d -= N[k][j] * N[k][j]
        ok = ok and d > floor
        lj = math.sqrt(_fmax(d, floor))
        N[j][j] = lj
        for i in range(j + 1, 8):
            s = N[j][i]
            for k in range(j):
                s -= N[k][j] * N[k][i]
            N[j][i] = s / lj
    for i in range(8):
        s = r[i]
        for k in range(i):
            s -= N[k][i] * r[k]
        r[i] = s / N[i][i]
    for i in range(7, -1, -1):
        s = r[i]
        for k in range(i + 1, 8):
            s -= N[i][k] * r[k]
        r[i] = s / N[i][i]
    with np.errstate(all="ignore"):
        n = np.array(r + [1.0], np.float64).astype(F32)
    return bool(ok and np.isfinite(n[:8]).all()), n


def thr_square(threshold):
    """thr2 as launch_verify computes it"""
    with np.errstate(all="ignore"):
        return F32(threshold) * F32(threshold)


def verify(kps_a, kps_b, match, n_hyp=2048, thr=3.0, seed=0, flags=0, counts=None):
    """One pair as the device computes it, seeded with `seed` (= seed + p of a batched call): dict with H f32 [3, 3],
    verified int32 [na], stats uint32 [4], and what tests look at: counts / valid / hyps of every hypothesis, k, the
    4-point H, `rounds` (what each refit round did: "failed", "rejected", "kept", "settled" = kept and the inlier set
    did not change) and the pair (Pair).  `counts` may pass a (counts, valid, hyps) computed before for this pair."""
    pair = Pair(kps_a, kps_b, match)
    thr2 = thr_square(thr)
    seed &= 0xFFFFFFFF
    cnt, valid, hyps = counts if counts is not None else pair.counts(seed, n_hyp, thr2)
    out = dict(pair=pair, counts=cnt, valid=valid, hyps=hyps, rounds=[], k=None, h4=None)
    verified = np.full(pair.na, -1, np.int32)
    if not valid.any():
        out.update(H=np.zeros((3, 3), F32), verified=verified,
                   stats=np.array([0, 0, INVALID, pair.m], np.uint32), mask=np.zeros(pair.m, bool))
        return out
    # argmax on (count, -k): ties go to the smallest k
    best = int(cnt.max())
    k = int(np.flatnonzero(cnt == best)[0])
    h = hyps[k].copy()
    inl, cost = pair.inliers(h, thr2)
    inl, cost = inl[0], cost[0]
    n_cur, cost_cur = int(inl.sum()), pair.cost_sum(cost)
    assert n_cur == best
    m = pair.moments(inl)
    if not flags & NO_REFINE:
        for _ in range(3):
            ok, nh = solve_refit(block_sum(m).tolist())
            if ok:
                h2, ok = pair.denormalise(nh[None])
                h2, ok = h2[0], bool(ok[0])
            if not ok:
                out["rounds"].append("failed")
                break
            in2, cost2 = pair.inliers(h2, thr2)
            in2, cost2 = in2[0], pair.cost_sum(cost2[0])
            if cost2 > cost_cur:
                out["rounds"].append("rejected")
                break
            changed = bool((pair.inliers(h, thr2)[0][0] != in2).any())
            h, m, n_cur, cost_cur = h2, pair.moments(in2), int(in2.sum()), cost2
            out["rounds"].append("kept" if changed else "settled")
            if not changed:
                break
    inl = pair.inliers(h, thr2)[0][0]
    verified[pair.rows[inl]] = pair.match[pair.rows[inl]]
    with np.errstate(all="ignore"):
        H = (h / h[8]).astype(F32)
    out.update(H=H.reshape(3, 3), verified=verified, stats=np.array([n_cur, best, k, pair.m], np.uint32), mask=inl, k=k,
               h4=hyps[k], h=h)
    return out
