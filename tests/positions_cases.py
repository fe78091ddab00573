"""Scenes for the tree-pose and global-positioning tests, and a plain float64 numpy restatement of the two algorithms of
include/lf_mkd.h (lf_mkd_tree_poses_device, lf_mkd_global_positions_device): the same chains and unit steps, the same usable
rules, weights, point and camera steps, gauge and final weights, written with numpy's own sums, determinants and solves.  It
shares no code with csrc/mkd_positions_math.h; tests/test_positions_twin.py holds the host twin to it.

A positions scene is a dict of the device call's arrays under its argument names (tests/positions_twin.py: arrays) plus
`truth`: the centres [n_images, 3] and points [T, 3] the keypoints were projected from.  A tree scene is a dict of edge_a,
edge_b, t, rotations, image_stats."""
import numpy as np

K0 = np.array([800.0, 790.0, 512.0, 384.0], np.float32)
NONE = 0xFFFFFFFF
SINGULAR = 1e-12


def look_at(c, target):
    z = target - c
    z = z / np.linalg.norm(z)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x = x / np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z])


def unit_step_centres(centres):
    """what lf_mkd_tree_poses_device gives a chain 0 - 1 - 2 ..: unit steps along the true directions"""
    c = np.zeros_like(centres)
    for i in range(1, len(centres)):
        d = centres[i] - centres[i - 1]
        c[i] = c[i - 1] + d / np.linalg.norm(d)
    return c


def build(seed, centres, targets, X, visible, noise=0.5, outliers=0.1, extra_rows=3, capacity=(0, 0), twice=()):
    """visible bool [T, N]: which camera sees which point.  A keypoint is the projection plus `noise` px; an outlier (share
    `outliers`) is replaced by a position anywhere in the frame: a wrong ray.  The pool holds per image `extra_rows` rows no
    track names, then the image's observations in track order; (t, i) in `twice` gives track t a second row of image i.  The
    input poses are the true rotations with unit-step chain centres.  capacity = (tracks, observations) beyond the counts."""
    g = np.random.default_rng(seed)
    visible = np.asarray(visible, bool)
    T, N = visible.shape
    Rs = [look_at(c, t) for c, t in zip(centres, targets)]
    rows_of = [[None] * extra_rows for _ in range(N)]
    obs, lengths = [], []
    for t in range(T):
        seen = [int(i) for i in np.flatnonzero(visible[t])]
        seen += [i for (tt, i) in twice if tt == t]
        for i in seen:
            p = Rs[i] @ (X[t] - centres[i])
            xy = np.array([K0[0] * p[0] / p[2] + K0[2], K0[1] * p[1] / p[2] + K0[3]]) + noise * g.standard_normal(2)
            if g.random() < outliers:
                xy = g.uniform(0, 1, 2) * np.array([1024.0, 768.0])
            obs.append((t, i, len(rows_of[i])))
            rows_of[i].append(xy)
        lengths.append(len(seen))
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows_of])]).astype(np.uint64)
    kps = np.zeros((int(off[-1]), 5), np.float32)
    kps[:, 2] = 3.0
    row_track = np.full(int(off[-1]), -1, np.int32)
    for i, rows in enumerate(rows_of):
        for k, xy in enumerate(rows):
            kps[int(off[i]) + k, :2] = xy if xy is not None else g.uniform(0, 700, 2)
    tcap, ocap = T + capacity[0], len(obs) + capacity[1]
    toff = np.full(tcap + 1, len(obs), np.uint64)
    toff[:T + 1] = np.concatenate([[0], np.cumsum(lengths)])
    obs_row, obs_image = np.full(ocap, -1, np.int32), np.zeros(ocap, np.uint32)
    for k, (t, i, local) in enumerate(obs):
        obs_row[k], obs_image[k] = int(off[i]) + local, i
        row_track[int(off[i]) + local] = t
    start = unit_step_centres(np.asarray(centres, np.float64))
    poses = np.array([np.concatenate([R.reshape(9), -R @ c]) for R, c in zip(Rs, start)], np.float32).reshape(N, 12)
    return dict(kps=kps, image_offsets=off, track_offsets=toff, obs_row=obs_row, obs_image=obs_image,
                counts=np.array([T, len(obs)], np.uint32), row_track=row_track, intrinsics=np.tile(K0, (N, 1)), poses=poses,
                truth=dict(centres=np.asarray(centres, np.float64), points=np.asarray(X, np.float64)))


def ring(n, npts, seed, share=0.6, **kw):
    """n cameras on a ring of radius 5 around npts points, each seeing a point with probability `share`"""
    g = np.random.default_rng(seed + 500)
    ang = np.linspace(0, 2 * np.pi, n, endpoint=False)
    centres = np.stack([5 * np.cos(ang), np.zeros(n), 5 * np.sin(ang)], 1) + 0.3 * g.standard_normal((n, 3))
    X = 1.2 * g.standard_normal((npts, 3))
    X = X / np.maximum(1.0, np.linalg.norm(X, axis=1, keepdims=True) / 2.4)
    visible = g.random((npts, n)) < share
    for t in range(npts):                                  # every point is seen twice at least
        while visible[t].sum() < 2:
            visible[t, g.integers(n)] = True
    return build(seed, centres, np.zeros((n, 3)), X, visible, **kw)


def scene_a(seed=3):
    """A: 6 cameras on a ring around 60 points, 0.5 px noise, 10 % wrong rays, unit-step tree poses"""
    return ring(6, 60, seed)


def scene_b(seed=4):
    """B: 8 cameras on a straight line, looking sideways at 120 points 4 .. 9 away; the same noise and outliers"""
    g = np.random.default_rng(seed + 500)
    n, npts = 8, 120
    centres = np.stack([0.5 * np.arange(n), np.zeros(n), np.zeros(n)], 1) + 0.02 * g.standard_normal((n, 3))
    targets = centres + np.array([0.0, 0.0, 6.0])
    X = np.stack([g.uniform(-2, 0.5 * n + 2, npts), g.uniform(-2, 2, npts), g.uniform(4, 9, npts)], 1)
    visible = np.zeros((npts, n), bool)
    for i in range(n):
        d = X - centres[i]
        visible[:, i] = (d[:, 2] / np.linalg.norm(d, axis=1) > np.cos(np.radians(30))) & (g.random(npts) < 0.8)
    keep = visible.sum(1) >= 2
    return build(seed, centres, targets, X[keep], visible[keep])


def scene_c(seed=5):
    """C, the kernels' seams: images with 255, 256 and 257 rows (3 of them in no track), tracks of 2, 3, 4, 5, 8 and 9
    positions, a track with two rows of one image, and capacities beyond the counts"""
    g = np.random.default_rng(seed + 500)
    n, big, npts = 9, 254, 314
    ang = np.linspace(0, 2 * np.pi, n, endpoint=False)
    centres = np.stack([5 * np.cos(ang), 0.5 * g.standard_normal(n), 5 * np.sin(ang)], 1)
    X = g.standard_normal((npts, 3))
    visible = np.zeros((npts, n), bool)
    visible[:252, 0] = visible[:253, 1] = visible[:254, 2] = True      # + 3 extra rows: 255, 256, 257
    for t in range(npts):                                  # the first 254 tracks: 3 .. 9 positions; the others: 2 .. 5, images 3 .. 8
        want = (3, 4, 5, 8, 9)[t % 5] if t < big else (2, 3, 4, 5)[t % 4]
        for i in g.permutation(np.arange(3, n)):
            if visible[t].sum() >= want:
                break
            visible[t, i] = True
    again = int(np.flatnonzero(visible[260])[0])           # track 260 gets a second row of its first image
    return build(seed, centres, np.zeros((n, 3)), X, visible, outliers=0.05, capacity=(5, 11), twice=((260, again),))


def tiny(seed=6, **kw):
    """4 cameras and 12 points, every point seen by every camera, no outliers: a few lines of scene for the properties"""
    g = np.random.default_rng(seed + 500)
    ang = np.linspace(0, 2 * np.pi, 4, endpoint=False)
    centres = np.stack([4 * np.cos(ang), 0.3 * g.standard_normal(4), 4 * np.sin(ang)], 1)
    return build(seed, centres, np.zeros((4, 3)), g.standard_normal((12, 3)), np.ones((12, 4), bool), outliers=0.0, **kw)


def scene_d(verify):
    """D: the collection of tests/reconstruction_cases.py -- its pool, and the track table its chain builds (the verifier through
    `verify`, a backend's method as reconstruction_cases.run_chain calls it; the link table, the tracks and the track table by
    the integer-exact restatements) -- under the true rotations with unit-step chain centres in image order.  Its tracks carry
    wrong matches and two rows of one image; image 3 sees 18 points."""
    import link_table_cases
    import reconstruction_cases as rc
    import track_table_cases
    import tracks_cases
    s, p = rc.scene(), rc.PARAMS
    kps, off, ea, eb = s["kps"], s["offsets"], s["edge_a"], s["edge_b"]
    la, _, cap, _, match = rc.layouts(s)
    ver = np.full(cap, -1, np.int32)
    for e in range(len(ea)):
        a, b = int(ea[e]), int(eb[e])
        ver[la[e]:la[e + 1]] = verify(e, kps[off[a]:off[a + 1]], kps[off[b]:off[b + 1]], match[la[e]:la[e + 1]], p["n_hyp"], p["f_thr"],
                                      p["seed"] + e)[1]
    links = link_table_cases.link_table(off, len(kps), ea, eb, la, cap, ver, min_links=p["min_links"], into=np.full(cap, -1, np.int32))
    track, length, dup = tracks_cases.build_tracks(off, len(kps), ea, eb, la, cap, links.match_kept)
    tt = track_table_cases.track_table(track, length, dup, min_len=2, consistent=True, image_offsets=off)
    truth = s["truth_poses"]
    R = truth[:, :9].reshape(-1, 3, 3)
    centres = -np.einsum("nji,nj->ni", R, truth[:, 9:])
    start = unit_step_centres(centres)
    poses = np.concatenate([truth[:, :9], -np.einsum("nij,nj->ni", R, start)], 1).astype(np.float32)
    return dict(kps=kps, image_offsets=off.astype(np.uint64), track_offsets=np.asarray(tt.offsets, np.uint64), obs_row=tt.obs_row,
                obs_image=tt.obs_image, counts=np.array(tt.counts[:2], np.uint32), row_track=tt.row_track,
                intrinsics=rc.intrinsics(s), poses=poses, truth=dict(centres=centres, points=s["truth_points"]))


# ---- tree scenes ----------------------------------------------------------------------------------------------------------------
def tree_scene(seed=8, n=7, flip=(2, 4), scale=True):
    """A chain 0 - 1 - .. - (n - 1) rooted at image 0 plus two edges that are no tree edge; tree edge of image i is (i - 1, i),
    stored as (i, i - 1) for i in `flip`.  t has an arbitrary positive length per edge."""
    g = np.random.default_rng(seed)
    centres = np.cumsum(g.standard_normal((n, 3)) + np.array([1.5, 0, 0]), 0)
    Rs = np.array([look_at(c, c + g.standard_normal(3) + np.array([0, 0, 4.0])) for c in centres])
    pairs = [((i, i - 1) if i in flip else (i - 1, i)) for i in range(1, n)] + [(0, 3), (5, 2)]
    ea, eb = np.array([p[0] for p in pairs], np.uint32), np.array([p[1] for p in pairs], np.uint32)
    t = np.array([Rs[b] @ (centres[a] - centres[b]) for a, b in pairs])
    if scale:
        t = t * g.uniform(0.2, 3.0, (len(pairs), 1)) / np.linalg.norm(t, axis=1, keepdims=True)
    stats = np.zeros((n, 4), np.uint32)
    stats[:, 1], stats[:, 2] = np.arange(n), np.arange(n) - 1
    stats[0, 2] = NONE
    return dict(edge_a=ea, edge_b=eb, t=t.astype(np.float32), rotations=Rs.reshape(n, 9).astype(np.float32), image_stats=stats,
                truth=centres)


def tree_reference(s, max_depth=64):
    """lf_mkd_tree_poses_device in float64 numpy -> poses f32 [n_images, 12]"""
    ea, eb, t = np.asarray(s["edge_a"], np.int64), np.asarray(s["edge_b"], np.int64), np.asarray(s["t"], np.float64).reshape(-1, 3)
    rot, st = np.asarray(s["rotations"], np.float64).reshape(-1, 3, 3), np.asarray(s["image_stats"], np.int64).reshape(-1, 4)
    n, E = len(rot), len(ea)
    poses = np.zeros((n, 12), np.float32)
    for i in range(n):
        steps, j, ok = [], i, True
        while True:
            if st[j, 1] == NONE or not rot[j].any():
                ok = False
            if not ok or st[j, 1] == 0:
                break
            e = st[j, 2]
            if len(steps) == max_depth or e >= E:
                ok = False
                break
            a, b = ea[e], eb[e]
            if a >= n or b >= n or a == b or j not in (a, b) or not np.isfinite(t[e]).all() or not np.isfinite(rot[b]).all():
                ok = False
                break
            d = -rot[b].T @ t[e]
            if not np.linalg.norm(d) > 0:
                ok = False
                break
            steps.append(d / np.linalg.norm(d) if j == b else -d / np.linalg.norm(d))
            j = b if j == a else a
        if ok:
            c = np.zeros(3)
            for u in reversed(steps):
                c = c + u
            poses[i, :9], poses[i, 9:] = rot[i].reshape(9), -rot[i] @ c
    return poses


# ---- global positions -----------------------------------------------------------------------------------------------------------
def _rays(kps, rows, K, R):
    f = np.stack([(kps[rows, 0] - K[:, 2]) / K[:, 0], (kps[rows, 1] - K[:, 3]) / K[:, 1], np.ones(len(rows))], 1)
    v = np.einsum("nji,nj->ni", R, f)
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _weights(v, X, c, s0, robust):
    if not robust:
        return np.ones(len(v))
    r = X - c
    depth = np.einsum("ni,ni->n", v, r)
    pr = r - v * depth[:, None]
    pr2, rr = np.einsum("ni,ni->n", pr, pr), np.einsum("ni,ni->n", r, r)
    with np.errstate(all="ignore"):
        s = np.sqrt(pr2 / rr)
        w = np.where(s > s0, s0 / s, 1.0)
    bad = ~(depth > 0) | ~(rr > 0) | ~np.isfinite(pr2) | ~np.isfinite(rr) | ~np.isfinite(s)
    return np.where(bad, 0.0, w)


def _solve(idx, m, v, w, y, min_obs):
    """per group g < m: A = sum w (I - v v^T), b = sum w (I - v v^T) y -> (solution [m, 3], reason [m])"""
    P = np.eye(3)[None] - v[:, :, None] * v[:, None, :]
    A, b = np.zeros((m, 3, 3)), np.zeros((m, 3))
    np.add.at(A, idx, w[:, None, None] * P)
    np.add.at(b, idx, w[:, None] * np.einsum("nij,nj->ni", P, y))
    weighted = np.bincount(idx[w > 0], minlength=m)
    mean = np.trace(A, axis1=1, axis2=2) / 3.0
    good = np.linalg.det(A) > SINGULAR * mean ** 3
    x = np.zeros((m, 3))
    if good.any():
        x[good] = np.linalg.solve(A[good], b[good][:, :, None])[:, :, 0]
    good &= np.isfinite(x).all(1)
    return x, np.where(weighted < min_obs, 2, np.where(good, 0, 3))


def reference(s, sweeps=50, warm=3, robust_deg=0.2, min_obs=2):
    """lf_mkd_global_positions_device in float64 numpy -> dict(poses, points, obs_state, image_stats, trace, counts, centres)"""
    kps = np.asarray(s["kps"], np.float32).reshape(-1, 5).astype(np.float64)
    ioff, toff = np.asarray(s["image_offsets"], np.int64), np.asarray(s["track_offsets"], np.int64)
    obs_row, obs_image = np.asarray(s["obs_row"], np.int64), np.asarray(s["obs_image"], np.int64)
    row_track = np.asarray(s["row_track"], np.int64)
    K32, P32 = np.asarray(s["intrinsics"], np.float32).reshape(-1, 4), np.asarray(s["poses"], np.float32).reshape(-1, 12)
    K, P = K32.astype(np.float64), P32.astype(np.float64)
    n, n_rows, tcap, ocap = len(K), len(kps), len(toff) - 1, len(obs_row)
    T, O = min(int(s["counts"][0]), tcap), min(int(s["counts"][1]), ocap)
    s0 = np.sin(np.radians(np.float64(np.float32(robust_deg))))
    reg = np.isfinite(K).all(1) & (K[:, 0] > 0) & (K[:, 1] > 0) & np.isfinite(P).all(1) & (P[:, :9] != 0).any(1)
    R = P[:, :9].reshape(n, 3, 3)
    cen = np.where(reg[:, None], -np.einsum("nji,nj->ni", R, np.where(reg[:, None], P[:, 9:], 0.0)), 0.0)
    finite_kp = np.isfinite(kps[:, 0]) & np.isfinite(kps[:, 1]) if n_rows else np.zeros(0, bool)
    # the point side: the positions of the tracks below T
    lo = np.minimum(toff[:T], O)
    hi = np.maximum(np.minimum(toff[1:T + 1], O), lo)
    p_pos = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)] + [np.zeros(0, np.int64)]).astype(np.int64)
    p_track = np.concatenate([np.full(b - a, t) for t, (a, b) in enumerate(zip(lo, hi))] + [np.zeros(0, np.int64)]).astype(np.int64)

    def usable_positions(pos):
        row, img = obs_row[pos], obs_image[pos]
        ok = (row >= 0) & (row < n_rows) & (img < n)
        ok[ok] &= reg[img[ok]] & finite_kp[row[ok]]
        return ok
    p_ok = usable_positions(p_pos)
    pp, pt_, pr, pi = p_pos[p_ok], p_track[p_ok], obs_row[p_pos[p_ok]], obs_image[p_pos[p_ok]]
    pv = _rays(kps, pr, K[pi], R[pi]) if len(pp) else np.zeros((0, 3))
    # the camera side: the rows of the registered images
    r_row, r_img = [], []
    for i in np.flatnonzero(reg):
        a = min(ioff[i], n_rows)
        b = max(min(ioff[i + 1], n_rows), a)
        rows = np.arange(a, b)
        rows = rows[(row_track[rows] >= 0) & (row_track[rows] < T) & finite_kp[rows]]
        r_row.append(rows), r_img.append(np.full(len(rows), i))
    r_row = np.concatenate(r_row + [np.zeros(0, np.int64)]).astype(np.int64)
    r_img = np.concatenate(r_img + [np.zeros(0, np.int64)]).astype(np.int64)
    r_track = row_track[r_row]
    rv = _rays(kps, r_row, K[r_img], R[r_img]) if len(r_row) else np.zeros((0, 3))
    # the trace's side: every usable position below O, its track by its row
    q_pos = np.arange(O)
    q_ok = usable_positions(q_pos)
    q_pos = q_pos[q_ok]
    q_track = row_track[obs_row[q_pos]]
    inside = (q_track >= 0) & (q_track < T)
    q_pos, q_track = q_pos[inside], q_track[inside]
    q_img = obs_image[q_pos]
    qv = _rays(kps, obs_row[q_pos], K[q_img], R[q_img]) if len(q_pos) else np.zeros((0, 3))

    pts, solved = np.zeros((T, 3)), np.zeros(T, bool)
    held, reason = np.zeros(n, np.int64), np.where(reg, 0, 1)
    trace, counts = np.zeros((sweeps, 4)), np.zeros(8, np.int64)
    counts[7] = sweeps

    def gauge():
        nonlocal cen, pts
        if not reg.any():
            counts[5] += 1
            return
        m = cen[reg].mean(0)
        rho = np.sqrt(((cen[reg] - m) ** 2).sum(1).mean())
        if not (np.isfinite(m).all() and np.isfinite(rho) and rho > 0):
            counts[5] += 1
            return
        cen = np.where(reg[:, None], (cen - m) / rho, cen)
        pts = (pts - m) / rho
    gauge()
    for sw in range(sweeps):
        robust = sw >= warm
        w = _weights(pv, pts[pt_], cen[pi], s0, robust)
        w = np.where(solved[pt_], w, 1.0) if robust else w
        x, why = _solve(pt_, T, pv, w, cen[pi], min_obs)
        solved = why == 0
        pts = np.where(solved[:, None], x, pts)
        unsolved = int((~solved).sum())
        on = solved[r_track]
        w = _weights(rv[on], pts[r_track[on]], cen[r_img[on]], s0, robust)
        x, why = _solve(r_img[on], n, rv[on], w, pts[r_track[on]], min_obs)
        moved = reg & (why == 0)
        cen = np.where(moved[:, None], x, cen)
        reason = np.where(reg, why, 1)
        held += reg & (why != 0)
        n_held = int((reg & (why != 0)).sum())
        gauge()
        on = solved[q_track]
        X, c = pts[q_track[on]], cen[q_img[on]]
        w = _weights(qv[on], X, c, s0, robust)
        r = X - c
        pr_ = r - qv[on] * np.einsum("ni,ni->n", qv[on], r)[:, None]
        trace[sw] = [(w * np.einsum("ni,ni->n", pr_, pr_))[w > 0].sum(), (w > 0).sum(), n_held, unsolved]
        counts[4] = n_held
    last = sweeps > 0 and sweeps - 1 >= warm
    poses = np.zeros((n, 12), np.float32)
    poses[reg, :9] = P32[reg, :9]
    poses[reg, 9:] = -np.einsum("nij,nj->ni", R[reg], cen[reg])
    image_stats = np.zeros((n, 4), np.uint32)
    on = solved[r_track]
    w = _weights(rv[on], pts[r_track[on]], cen[r_img[on]], s0, last)
    image_stats[:, 0] = np.bincount(r_img[on], minlength=n)
    image_stats[:, 1] = np.bincount(r_img[on][w >= 0.5], minlength=n)
    image_stats[:, 2], image_stats[:, 3] = held, reason
    counts[0], counts[1], counts[2], counts[3], counts[6] = reg.sum(), solved.sum(), image_stats[:, 0].sum(), image_stats[:, 1].sum(), T
    obs_state = np.full(ocap, NONE, np.uint32)                 # NONE: not written
    obs_state[p_pos] = 0
    w = np.where(solved[pt_], _weights(pv, pts[pt_], cen[pi], s0, last), 0.0)
    obs_state[pp] = np.where(solved[pt_] & (w >= 0.5), 2, 1)
    points = np.zeros((T, 4), np.float32)
    points[:, 3] = 2.0
    for t in np.flatnonzero(solved):
        mine = (pt_ == t) & (w > 0)
        v = pv[mine]
        cos = min([2.0] + [float(v[0] @ u) for u in v[1:]])
        points[t] = [*pts[t], cos]
    return dict(poses=poses, points=points, obs_state=obs_state, image_stats=image_stats, trace=trace,
                counts=counts.astype(np.uint32), centres=cen, registered=reg)


def similarity_error(c, truth):
    """the largest distance between the centres c and the truth after the similarity (Umeyama, with scale) that fits c to the
    truth, in units of the truth's rms radius"""
    c, truth = np.asarray(c, np.float64), np.asarray(truth, np.float64)
    mc, mt = c.mean(0), truth.mean(0)
    a, b = c - mc, truth - mt
    U, S, Vt = np.linalg.svd(b.T @ a)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    Rf = U @ D @ Vt
    scale = (S * np.diag(D)).sum() / (a * a).sum()
    fit = scale * a @ Rf.T + mt
    return float(np.linalg.norm(fit - truth, axis=1).max() / np.sqrt((b * b).sum(1).mean()))


def centres_of(poses):
    P = np.asarray(poses, np.float64).reshape(-1, 12)
    return -np.einsum("nji,nj->ni", P[:, :9].reshape(-1, 3, 3), P[:, 9:])
