"""Scenes for the bundle adjustment tests, and a plain float64 numpy restatement of the algorithm of include/lf_mkd.h
(lf_mkd_bundle_adjust_device): the same Levenberg-Marquardt loop, the same damping, HELD rules and preconditioned conjugate
gradients with the same stopping rules, written with numpy's own sums and solves.  It shares no code with
csrc/mkd_bundle_math.h; tests/test_bundle_twin.py holds the host twin to it.

A scene is a dict of the device call's arrays under its argument names (tests/bundle_twin.py: arrays) plus `truth`: the poses
[n_images, 12] and points [T, 3] the keypoints were projected from."""
import numpy as np

K0 = np.array([800.0, 790.0, 512.0, 384.0], np.float32)


def cayley(w):
    w = np.asarray(w, np.float64)
    n = w @ w
    S = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return ((1 - n) * np.eye(3) + 2 * np.outer(w, w) + 2 * S) / (1 + n)


def look_at(c, target=np.zeros(3)):
    z = target - c
    z = z / np.linalg.norm(z)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x = x / np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return R, -R @ c


def build(seed, visible, noise=0.5, outliers=0.0, perturb=(0.004, 0.02, 0.02), fixed=(0, 1), extra_rows=3, capacity=(0, 0)):
    """visible bool [T, N]: which camera sees which point.  Cameras on a ring of radius 6 looking at the origin, points in a
    ball of radius 1.5; a keypoint is the projection plus `noise` px, an outlier (share `outliers`) is 15 .. 60 px off.  The
    pool holds per image `extra_rows` rows no track names, then the image's observations in track order.  The input poses and
    points are the truth perturbed by (rotation as a Cayley vector, translation, point) sigmas; the cameras in `fixed` keep the
    truth.  capacity = (tracks, observations) beyond the counts."""
    g = np.random.default_rng(seed)
    visible = np.asarray(visible, bool)
    T, N = visible.shape
    ang = 2 * np.pi * (np.arange(N) + 0.25 * g.random(N)) / max(N, 1)
    centres = np.stack([6 * np.cos(ang), 0.8 * g.standard_normal(N), 6 * np.sin(ang)], 1)
    Rs, ts = zip(*[look_at(c) for c in centres]) if N else ((), ())
    X = g.standard_normal((T, 3))
    X = 1.5 * X / np.maximum(1.0, np.linalg.norm(X, axis=1, keepdims=True))
    truth_poses = np.array([np.concatenate([R.reshape(9), t]) for R, t in zip(Rs, ts)], np.float32).reshape(N, 12)
    rows_of = [[None] * extra_rows for _ in range(N)]
    obs = []                                              # (track, image, local row)
    for t in range(T):
        for i in np.flatnonzero(visible[t]):
            p = Rs[i] @ X[t] + ts[i]
            xy = np.array([K0[0] * p[0] / p[2] + K0[2], K0[1] * p[1] / p[2] + K0[3]]) + noise * g.standard_normal(2)
            if g.random() < outliers:
                a = g.uniform(0, 2 * np.pi)
                xy += g.uniform(15, 60) * np.array([np.cos(a), np.sin(a)])
            obs.append((t, i, len(rows_of[i])))
            rows_of[i].append(xy)
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows_of])]).astype(np.uint64)
    kps = np.zeros((int(off[-1]), 5), np.float32)
    kps[:, 2] = 3.0
    for i, rows in enumerate(rows_of):
        for k, xy in enumerate(rows):
            kps[int(off[i]) + k, :2] = xy if xy is not None else g.uniform(0, 700, 2)
    tcap, ocap = T + capacity[0], len(obs) + capacity[1]
    toff = np.full(tcap + 1, len(obs), np.uint64)
    toff[:T + 1] = np.concatenate([[0], np.cumsum(visible.sum(1))])
    obs_row, obs_image = np.full(ocap, -1, np.int32), np.zeros(ocap, np.uint32)
    for k, (t, i, local) in enumerate(obs):
        obs_row[k], obs_image[k] = int(off[i]) + local, i
    poses = truth_poses.astype(np.float64)
    for i in range(N):
        if i in fixed:
            continue
        R = cayley(perturb[0] * g.standard_normal(3)) @ poses[i, :9].reshape(3, 3)
        poses[i, :9], poses[i, 9:] = R.reshape(9), poses[i, 9:] + perturb[1] * g.standard_normal(3)
    points = np.zeros((tcap, 4), np.float32)
    points[:, 3] = 2.0
    points[:T, :3] = X + perturb[2] * g.standard_normal((T, 3))
    points[:T, 3] = 0.9
    cf = np.zeros(N, np.uint32)
    cf[[i for i in fixed if i < N]] = 1
    return dict(kps=kps, image_offsets=off, track_offsets=toff, obs_row=obs_row, obs_image=obs_image,
                counts=np.array([T, len(obs)], np.uint32), points=points, intrinsics=np.tile(K0, (N, 1)),
                poses=poses.astype(np.float32), obs_state=None, camera_fixed=cf, truth=dict(poses=truth_poses, points=X))


def random_views(seed, T, N, lo=2, hi=9):
    g = np.random.default_rng(seed + 1000)
    v = np.zeros((T, N), bool)
    for t in range(T):
        v[t, g.choice(N, size=min(N, int(g.integers(lo, hi + 1))), replace=False)] = True
    return v


def realistic(seed=3):
    """about 12 cameras, 400 tracks of 2 .. 9 views, 0.5 px noise, 5 % wrong observations, perturbed poses and points"""
    return build(seed, random_views(seed, 400, 12), noise=0.5, outliers=0.05)


def track_lengths(seed=5):
    """tracks of 2, 3, 4, 5, 8, 9 positions: the 4-slot seam"""
    g = np.random.default_rng(seed)
    v = np.zeros((60, 9), bool)
    for t in range(60):
        v[t, g.choice(9, size=(2, 3, 4, 5, 8, 9)[t % 6], replace=False)] = True
    return build(seed, v, outliers=0.03)


def image_rows(seed=7):
    """images with 255, 256, 257 and 513 active rows (the 256-slot seam); two more see every track"""
    v = np.zeros((513, 6), bool)
    v[:, 0] = v[:, 1] = True
    v[:255, 2] = v[:256, 3] = v[:257, 4] = v[:, 5] = True
    return build(seed, v, outliers=0.02)


def many_images(n, seed=9):
    """n images with a handful of rows each (the global-sum seam): track t is seen by images t, t + 1, t + 2 (mod n)"""
    T = max(n, 4)
    v = np.zeros((T, n), bool)
    for t in range(T):
        v[t, [(t + d) % n for d in range(min(3, n))]] = True
    return build(seed, v, fixed=(0, 1) if n > 2 else (0,) if n == 2 else ())


def many_tracks(T, seed=11):
    """T tracks over 5 cameras (the cost-sum seam)"""
    return build(seed, random_views(seed, T, 5, 2, 4))


def tiny(seed=13):
    """3 free cameras of 5 and 12 points: small enough for a dense solve"""
    return build(seed, np.ones((12, 5), bool), noise=0.3, perturb=(0.003, 0.01, 0.01))


def mixed(seed=15):
    """fixed, unregistered and free cameras together: image 2 has an all-zero pose, image 5 a NaN in its intrinsics"""
    s = build(seed, random_views(seed, 120, 8, 3, 6), outliers=0.04)
    s["poses"][2] = 0
    s["intrinsics"][5, 1] = np.nan
    return s


def garbage(seed=17):
    """NaN keypoints, rows and images out of range, offsets inverted or past the end, non-finite points.  Whatever is broken
    is inactive by the call's rules, and no two ranges that stay overlap, so every output word is still defined."""
    s = build(seed, random_views(seed, 90, 7, 3, 6), outliers=0.04, capacity=(5, 9))
    g = np.random.default_rng(seed)
    O = int(s["counts"][1])
    pick = g.choice(O, 40, replace=False)
    s["kps"][s["obs_row"][pick[:8]], 0] = np.nan
    s["kps"][s["obs_row"][pick[8:12]], 1] = np.inf
    s["obs_row"][pick[12:16]] = -5
    s["obs_row"][pick[16:20]] = len(s["kps"]) + 7
    s["obs_image"][pick[20:24]] = 7
    s["obs_image"][pick[24:28]] = 0xFFFFFFF0
    for p in pick[28:40]:                                                    # a row of the next image that no track names:
        s["obs_row"][p] = int(s["image_offsets"][(int(s["obs_image"][p]) + 1) % 7])   # outside its image's range
    s["points"][3, 0], s["points"][4, 2], s["points"][5, 3], s["points"][6, 3] = np.nan, np.inf, np.nan, 1.5
    toff = s["track_offsets"]
    toff[20], toff[21] = toff[21], toff[20]                                  # inverted: track 20 is empty, 19 and 21 overlap ...
    s["obs_row"][int(toff[21]):int(toff[20])] = -1                           # ... over positions that are inactive for both
    toff[int(s["counts"][0]) + 1:] = O + 1000                                # past the end ...
    s["counts"][0] += 2                                                      # ... and two such tracks below T: clamped to O, empty
    ioff = s["image_offsets"]
    ioff[-1] = len(s["kps"]) + 50                                            # past the end: clamped
    ioff[3], ioff[4] = ioff[4], ioff[3]                                      # inverted: image 3 is empty, 2 and 4 would overlap ...
    rows = np.arange(int(ioff[4]), int(ioff[3]))
    s["kps"][rows, 0] = np.nan                                               # ... over rows that are inactive
    return s


def pose_error(P, truth):
    """(rotation angle in radians, distance of the camera centres) between two [12] poses"""
    P, truth = np.asarray(P, np.float64), np.asarray(truth, np.float64)
    Ra, Rb = P[:9].reshape(3, 3), truth[:9].reshape(3, 3)
    c = np.clip((np.trace(Ra @ Rb.T) - 1) / 2, -1, 1)
    return float(np.arccos(c)), float(np.linalg.norm(-Ra.T @ P[9:] + Rb.T @ truth[9:]))


# ---- the numpy restatement ---------------------------------------------------------------------------------------------------
def _finite32(a):
    return np.isfinite(np.asarray(a, np.float32).astype(np.float64))


def active_set(s):
    """(position, track, image, row) of every ACTIVE observation, ascending by position; the usable and free masks"""
    N, rows = len(s["intrinsics"]), len(s["kps"])
    K, P = np.asarray(s["intrinsics"], np.float32), np.asarray(s["poses"], np.float32)
    usable = _finite32(K).all(1) & (K[:, 0] > 0) & (K[:, 1] > 0) & _finite32(P).all(1) & (P[:, :9] != 0).any(1) if N else np.zeros(0, bool)
    fixed = np.zeros(N, bool) if s.get("camera_fixed") is None else np.asarray(s["camera_fixed"]) != 0
    T = min(int(s["counts"][0]), len(s["points"]))
    O = min(int(s["counts"][1]), len(s["obs_row"]))
    ioff = np.minimum(np.asarray(s["image_offsets"], np.uint64), rows).astype(np.int64)
    toff = np.minimum(np.asarray(s["track_offsets"], np.uint64), O).astype(np.int64)
    pts = np.asarray(s["points"], np.float32)
    out = []
    for t in range(T):
        if not (_finite32(pts[t, :3]).all() and pts[t, 3] <= 1):
            continue
        for p in range(toff[t], max(toff[t + 1], toff[t])):
            r, i = int(s["obs_row"][p]), int(s["obs_image"][p])
            if r < 0 or r >= rows or i >= N or not usable[i] or not _finite32(s["kps"][r, :2]).all():
                continue
            if not (ioff[i] <= r < max(ioff[i + 1], ioff[i])):
                continue
            if s.get("obs_state") is not None and s["obs_state"][p] != 2:
                continue
            out.append((p, t, i, r))
    return np.array(out, np.int64).reshape(-1, 4), usable, usable & ~fixed, T


def restate(s, px=4.0, lambda0=1e-3, iterations=4, cg_iterations=8, cg_tol=0.1, dense_first_step=False):
    """-> dict poses f32 [N, 12], points f32 [tcap, 4], obs_state [ocap] (-1 where nothing is written), trace [iterations, 8],
    counts [4], near_tie (did a decision hang on less than the margins of tests/test_bundle_twin.py), x0 (the first step's
    camera update), and with dense_first_step the dense damped normal equations' solution for the same step"""
    act, usable, cam_free, T = active_set(s)
    N = len(usable)
    thr2 = float(np.float32(px)) ** 2
    tol2 = float(np.float32(cg_tol)) ** 2
    lam = float(np.float32(lambda0))
    K = np.asarray(s["intrinsics"], np.float32).astype(np.float64)
    P0 = np.asarray(s["poses"], np.float32).astype(np.float64)
    R, tr = P0[:, :9].reshape(N, 3, 3).copy(), P0[:, 9:].copy()
    X = np.asarray(s["points"], np.float32).astype(np.float64)[:, :3].copy()
    op, ot, oi, orow = act.T if len(act) else (np.zeros(0, np.int64),) * 4
    xy = np.asarray(s["kps"], np.float32).astype(np.float64)[orow, :2]
    pt_free = np.zeros(len(X), bool)
    pt_free[ot] = True
    n = len(op)
    near = False

    def project(R, tr, X):
        q = np.einsum("nij,nj->ni", R[oi], X[ot])
        p = q + tr[oi]
        with np.errstate(all="ignore"):
            u = p[:, :2] / p[:, 2:3]
            e = K[oi, :2] * u + K[oi, 2:] - xy
        return q, p, u, e, (e * e).sum(1)

    def cost_of(R, tr, X):
        nonlocal near
        _, p, _, _, e2 = project(R, tr, X)
        inl = (p[:, 2] > 0) & (e2 <= thr2)
        near = near or bool((np.abs(e2 - thr2) <= 1e-9 * thr2).any())
        return float(np.where(inl, e2, thr2).sum()), inl

    trace = np.zeros((iterations, 8))
    x_first = dense = None
    accepted = 0
    for it in range(iterations):
        q, p, u, e, e2 = project(R, tr, X)
        cost_k, inl = cost_of(R, tr, X)
        with np.errstate(all="ignore"):
            a, b = K[oi, 0] / p[:, 2], K[oi, 1] / p[:, 2]
        gx, gy = -a * u[:, 0], -b * u[:, 1]
        z = np.zeros(n)
        Jx = np.stack([2 * gx * q[:, 1], 2 * (a * q[:, 2] - gx * q[:, 0]), -2 * a * q[:, 1], a, z, gx], 1)
        Jy = np.stack([2 * (gy * q[:, 1] - b * q[:, 2]), -2 * gy * q[:, 0], 2 * b * q[:, 0], z, b, gy], 1)
        Rr = R[oi]
        Px = a[:, None] * Rr[:, 0] + gx[:, None] * Rr[:, 2]
        Py = b[:, None] * Rr[:, 1] + gy[:, None] * Rr[:, 2]
        m = inl.astype(np.float64)[:, None, None]
        Uo = (Jx[:, :, None] * Jx[:, None, :] + Jy[:, :, None] * Jy[:, None, :]) * m
        Vo = (Px[:, :, None] * Px[:, None, :] + Py[:, :, None] * Py[:, None, :]) * m
        Wo = Jx[:, :, None] * Px[:, None, :] + Jy[:, :, None] * Py[:, None, :]
        gco = (Jx * e[:, :1] + Jy * e[:, 1:]) * m[:, 0]
        gpo = (Px * e[:, :1] + Py * e[:, 1:]) * m[:, 0]
        keep = inl                                             # (outliers may hold NaNs: they add nothing)
        U, gc = np.zeros((N, 6, 6)), np.zeros((N, 6))
        V, gp = np.zeros((len(X), 3, 3)), np.zeros((len(X), 3))
        np.add.at(U, oi[keep], Uo[keep]), np.add.at(gc, oi[keep], gco[keep])
        np.add.at(V, ot[keep], Vo[keep]), np.add.at(gp, ot[keep], gpo[keep])
        n_in = np.bincount(ot[keep], minlength=len(X))
        for M in (U, V):
            d = np.einsum("nii->ni", M)
            d += lam * np.maximum(d, 1e-6)
        cam_moves = cam_free.copy()
        Uinv = np.zeros_like(U)
        for i in np.flatnonzero(cam_free):
            try:
                assert np.isfinite(U[i]).all()
                np.linalg.cholesky(U[i])
                Uinv[i] = np.linalg.inv(U[i])
            except (np.linalg.LinAlgError, AssertionError):
                cam_moves[i] = False
        with np.errstate(all="ignore"):
            det = np.linalg.det(V)
            mean = np.einsum("nii->n", V) / 3
            pt_moves = pt_free & (n_in >= 2) & (det > 1e-12 * mean ** 3)
        Vinv = np.zeros_like(V)
        Vinv[pt_moves] = np.linalg.inv(V[pt_moves])
        cpl = inl & cam_moves[oi] & pt_moves[ot]

        def wt(v):                                             # per track: sum W^T v
            out = np.zeros((len(X), 3))
            np.add.at(out, ot[cpl], np.einsum("nij,ni->nj", Wo[cpl], v[oi[cpl]]))
            return out

        def w(y):                                              # per image: sum W y
            out = np.zeros((N, 6))
            np.add.at(out, oi[cpl], np.einsum("nij,nj->ni", Wo[cpl], y[ot[cpl]]))
            return out

        solve_v = lambda b_: np.einsum("nij,nj->ni", Vinv, b_)
        solve_u = lambda b_: np.einsum("nij,nj->ni", Uinv, b_)
        mask = cam_moves[:, None]
        rhs = np.where(mask, gc - w(solve_v(gp)), 0.0)
        x, r = np.zeros((N, 6)), rhs.copy()
        zz = solve_u(r)
        pp = zz.copy()
        rz = rz0 = float((r * zz).sum())
        steps = 0
        for _ in range(cg_iterations):
            Ap = np.where(mask, np.einsum("nij,nj->ni", U, pp) - w(solve_v(wt(pp))), 0.0)
            pAp = float((pp * Ap).sum())
            if not (pAp > 0) or not (rz > 0):
                break
            alpha = rz / pAp
            steps += 1
            x, r = x + alpha * pp, r - alpha * Ap
            zz = solve_u(r)
            rz_new = float((r * zz).sum())
            beta, rz = rz_new / rz, rz_new
            if not (rz_new > 0) or rz_new <= tol2 * rz0:
                break
            pp = zz + beta * pp
        if it == 0:
            x_first = x.copy()
            if dense_first_step:
                dense = _dense_step(U, V, Wo, gc, gp, cpl, oi, ot, cam_moves, pt_moves)
        dp = solve_v(gp - wt(x))
        Rn, tn, Xn = R.copy(), tr.copy(), X.copy()
        for i in np.flatnonzero(cam_moves):
            Rn[i], tn[i] = cayley(-x[i, :3]) @ R[i], tr[i] - x[i, 3:]
        Xn[pt_moves] = X[pt_moves] - dp[pt_moves]
        cost_new, _ = cost_of(Rn, tn, Xn)
        near = near or abs(cost_new - cost_k) <= 1e-12 * cost_k
        ok = cost_new <= cost_k
        trace[it] = [cost_k, cost_new, lam, ok, steps, inl.sum(), (cam_free & ~cam_moves).sum(), (pt_free & ~pt_moves).sum()]
        if ok:
            R, tr, X, accepted = Rn, tn, Xn, accepted + 1
            lam = max(lam / 4, 2.0 ** -40)
        else:
            lam = min(8 * lam, 2.0 ** 40)

    poses = np.asarray(s["poses"], np.float32).copy()
    poses[cam_free] = np.concatenate([R.reshape(N, 9), tr], 1).astype(np.float32)[cam_free]
    points = np.asarray(s["points"], np.float32).copy()
    points[pt_free, :3] = X.astype(np.float32)[pt_free]
    state = np.full(len(s["obs_row"]), -1, np.int64)
    O = min(int(s["counts"][1]), len(s["obs_row"]))
    toff = np.minimum(np.asarray(s["track_offsets"], np.uint64), O).astype(np.int64)
    for t in range(T):
        state[toff[t]:max(toff[t], toff[t + 1])] = 0
    P32 = poses.astype(np.float64)
    _, p, _, _, e2 = project(P32[:, :9].reshape(N, 3, 3), P32[:, 9:], points[:, :3].astype(np.float64))
    near = near or bool((np.abs(e2 - thr2) <= 1e-9 * thr2).any())
    state[op] = np.where((p[:, 2] > 0) & (e2 <= thr2), 2, 1)
    return dict(poses=poses, points=points, obs_state=state, trace=trace, near_tie=near, x0=x_first, dense=dense,
                counts=np.array([cam_free.sum(), pt_free.sum(), n, accepted]), rms=_rms(e2, p, thr2))


def _rms(e2, p, thr2):
    inl = (p[:, 2] > 0) & (e2 <= thr2)
    return float(np.sqrt(e2[inl].mean())) if inl.any() else 0.0


def _dense_step(U, V, Wo, gc, gp, cpl, oi, ot, cam_moves, pt_moves):
    """the camera part of numpy.linalg.solve on the dense damped normal equations over the moving cameras and points"""
    cams, pts = np.flatnonzero(cam_moves), np.flatnonzero(pt_moves)
    ci, pi = {c: k for k, c in enumerate(cams)}, {p_: k for k, p_ in enumerate(pts)}
    nc, npt = 6 * len(cams), 3 * len(pts)
    H, g = np.zeros((nc + npt, nc + npt)), np.zeros(nc + npt)
    for c in cams:
        H[6 * ci[c]:6 * ci[c] + 6, 6 * ci[c]:6 * ci[c] + 6] = U[c]
        g[6 * ci[c]:6 * ci[c] + 6] = gc[c]
    for p_ in pts:
        k = nc + 3 * pi[p_]
        H[k:k + 3, k:k + 3] = V[p_]
        g[k:k + 3] = gp[p_]
    for k in np.flatnonzero(cpl):
        a, b = 6 * ci[oi[k]], nc + 3 * pi[ot[k]]
        H[a:a + 6, b:b + 3] += Wo[k]
        H[b:b + 3, a:a + 6] += Wo[k].T
    sol = np.linalg.solve(H, g)
    out = np.zeros((len(cam_moves), 6))
    out[cams] = sol[:nc].reshape(-1, 6)
    return out


def rms_of(s, poses, points, px=4.0):
    """the rms reprojection error of the inliers of (poses, points) over the scene's active observations"""
    act, _, _, _ = active_set(s)
    op, ot, oi, orow = act.T
    P = np.asarray(poses, np.float32).astype(np.float64)
    X = np.asarray(points, np.float32).astype(np.float64)[:, :3]
    K = np.asarray(s["intrinsics"], np.float32).astype(np.float64)
    p = np.einsum("nij,nj->ni", P[oi, :9].reshape(-1, 3, 3), X[ot]) + P[oi, 9:]
    e = K[oi, :2] * p[:, :2] / p[:, 2:3] + K[oi, 2:] - np.asarray(s["kps"], np.float64)[orow, :2]
    e2 = (e * e).sum(1)
    return _rms(e2, p, float(np.float32(px)) ** 2)
