"""What the two-view pose tests share (tests/test_pose_twin.py, tests/test_gpu_two_view_pose.py, tools/bench_two_view_pose.py):
`table`s -- the device call's arrays under its argument names, made from tests/fundamental_cases.py's synthetic two-view
problems -- and a float64 numpy restatement of the algorithm of include/lf_mkd.h (lf_mkd_two_view_pose_device) that uses
numpy.linalg.eigh where the kernel runs its Jacobi.  The restatement numbers the candidates by ITS eigenvectors' signs, so
candidate indices are its own; everything else is comparable."""
import numpy as np

import fundamental_cases as fc
from fundamental_cases import FAMILIES, K, MOTIONS, f_true, two_view  # noqa: F401  (re-exported for the tests)

NONE = 0xFFFFFFFF
K4 = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float32)
NONE_ROW = np.array([0.0, 0.0, 0.0, 2.0], np.float32)


def problem(m, outliers, seed, family, sigma=0.5):
    """(ka, kb, match) of fundamental_cases.two_view; m == 0 gives an empty problem."""
    if m == 0:
        return np.zeros((0, 5), np.float32), np.zeros((0, 5), np.float32), np.zeros(0, np.int32)
    ka, kb, mt, _ = two_view(m, outliers, seed, family, sigma)
    return ka, kb, mt


def make_table(problems, models, shift=None):
    """One pool: edge e joins images 2 e and 2 e + 1, whose rows are problem e's ka and kb; its links are the rows i with
    0 <= match[i] < nb, in ascending i, as pool rows.  models [n][3, 3] float64 (b^T F a = 0 in the problems' own pixels).
    shift: per image a pixel offset (dx, dy) added to its keypoints and principal point, F moved with it, so that every
    image has intrinsics of its own."""
    n = len(problems)
    shift = np.zeros((2 * n, 2)) if shift is None else np.asarray(shift, np.float64).reshape(2 * n, 2)
    kps, la, lb, off, fs = [], [], [], [0], []
    intr = np.tile(K4.astype(np.float64), (2 * n, 1))
    intr[:, 2:] += shift
    first = 0
    for e, (ka, kb, mt) in enumerate(problems):
        ka, kb = ka.copy(), kb.copy()
        ka[:, :2] += shift[2 * e].astype(np.float32)
        kb[:, :2] += shift[2 * e + 1].astype(np.float32)
        rows = np.flatnonzero((mt >= 0) & (mt < len(kb)))
        la.append(first + rows)
        lb.append(first + len(ka) + mt[rows])
        off.append(off[-1] + len(rows))
        kps += [ka, kb]
        first += len(ka) + len(kb)
        ta, tb = np.eye(3), np.eye(3)           # x = x' - shift: F' = Tb^T F Ta
        ta[:2, 2], tb[:2, 2] = -shift[2 * e], -shift[2 * e + 1]
        f = tb.T @ np.asarray(models[e], np.float64).reshape(3, 3) @ ta
        big = np.abs(f).max()
        fs.append(f / big if big > 0 and np.isfinite(big) else f)
    with np.errstate(invalid="ignore"):
        f32 = np.array(fs, np.float64).reshape(n, 9).astype(np.float32)
    return {"kps": np.concatenate(kps + [np.zeros((0, 5), np.float32)]).astype(np.float32),
            "edge_a": np.arange(0, 2 * n, 2, dtype=np.uint32), "edge_b": np.arange(1, 2 * n, 2, dtype=np.uint32),
            "intrinsics": intr.astype(np.float32), "F": f32, "link_offsets": np.array(off, np.uint64),
            "link_a": np.concatenate(la + [np.zeros(0, np.int64)]).astype(np.int32),
            "link_b": np.concatenate(lb + [np.zeros(0, np.int64)]).astype(np.int32)}


def edge_table(t, e):
    """Edge e of table t as a table of its own (the same pool, intrinsics and link arrays; one edge, its own range)."""
    out = dict(t)
    out["edge_a"], out["edge_b"], out["F"] = t["edge_a"][e:e + 1], t["edge_b"][e:e + 1], t["F"][e:e + 1]
    out["link_offsets"] = t["link_offsets"][e:e + 2]
    return out


def family_batch(n_edges=48, seed=11):
    """The five families in one call: ragged lengths, noise, outliers, rows without a match, per-image intrinsics."""
    g = np.random.default_rng(seed)
    probs, models = [], []
    for e in range(n_edges):
        fam = FAMILIES[e % len(FAMILIES)]
        m = int(g.integers(8, 700))
        ka, kb, mt = problem(m, float(g.uniform(0.0, 0.5)), 3000 + e, fam)
        mt = mt.copy()
        mt[g.random(m) < 0.2] = -1
        mt[g.random(m) < 0.03] = m + 5
        probs.append((ka, kb, mt))
        models.append(f_true(*MOTIONS[fam]))
    return make_table(probs, models, g.uniform(-60, 60, (2 * n_edges, 2)))


LENGTHS = (0, 1, 7, 255, 256, 257, 1500)


def length_batch():
    """Edges of 0, 1, 7, 255, 256, 257 and 1500 links (the last: several turns of the workgroup's loop)."""
    probs = [problem(m, 0.2 if m > 7 else 0.0, 4000 + m, FAMILIES[i % len(FAMILIES)]) for i, m in enumerate(LENGTHS)]
    return make_table(probs, [f_true(*MOTIONS[FAMILIES[i % len(FAMILIES)]]) for i in range(len(LENGTHS))])


NO_POSE = ("zero_F", "nan_F", "fx_zero", "bad_id", "all_behind", "rank1_F")


def no_pose_batch(m=300):
    """One ordinary edge, then one edge per no-pose cause, then another ordinary edge."""
    names = ("ok",) + NO_POSE + ("ok",)
    probs = [problem(m, 0.1, 5000 + i, "general") for i in range(len(names))]
    models = [f_true(*MOTIONS["general"]) for _ in names]
    models[1] = np.zeros((3, 3))
    models[2] = models[2].copy()
    models[2][1, 1] = np.nan
    models[6] = np.outer([0.3, -0.5, 1.0], [0.2, 1.0, -0.4])
    # all behind: a link whose two rays make the SAME angle with the baseline is in front under no candidate.  With unit
    # p = R xa, q = xb and a = p.t = q.t, c = p.q: na = a (c - 1) and nb = a (1 - c) have opposite signs, under either twisted
    # rotation (both leave p.t as it is) and either sign of t.  So every b point is its a ray turned about t by 20 .. 40
    # degrees; the margins a (1 - c) are ~1e-2, far above what rounding F and the pixels to f32 moves.
    r, tr = MOTIONS["general"]
    tr = tr / np.linalg.norm(tr)
    ka, _, mt = probs[5]
    g = np.random.default_rng(77)
    p = _rays(ka, np.arange(len(ka)), K4) @ r.T
    phi = np.deg2rad(g.uniform(20, 40, len(ka)))
    turn = lambda a: p * np.cos(a)[:, None] + np.cross(tr, p) * np.sin(a)[:, None] + tr * ((p @ tr) * (1 - np.cos(a)))[:, None]
    q, q2 = turn(phi), turn(-phi)
    q = np.where((q[:, 2] / np.linalg.norm(q, axis=1) > q2[:, 2] / np.linalg.norm(q2, axis=1))[:, None], q, q2)
    assert (q[:, 2] > 0.2).all()
    kb = ka.copy()
    kb[:, 0] = K4[0] * q[:, 0] / q[:, 2] + K4[2]
    kb[:, 1] = K4[1] * q[:, 1] / q[:, 2] + K4[3]
    probs[5] = (ka, kb, mt)
    t = make_table(probs, models)
    t["intrinsics"] = t["intrinsics"].copy()
    t["intrinsics"][2 * 3 + 1, 0] = 0.0
    t["edge_b"] = t["edge_b"].copy()
    t["edge_b"][4] = NONE
    return t, names


def bad_rows_table(m=400):
    """One edge whose link arrays hold out-of-range and negative rows and whose keypoints hold a NaN; a second, clean edge."""
    t = make_table([problem(m, 0.1, 6001, "general"), problem(m, 0.1, 6002, "duplicates")],
                   [f_true(*MOTIONS["general"]), f_true(*MOTIONS["duplicates"])])
    la, lb, kps = t["link_a"].copy(), t["link_b"].copy(), t["kps"].copy()
    n = len(kps)
    la[3], la[40], lb[7], lb[41], la[100], lb[100] = -1, n, -7, n + 1000, -2 ** 31, 2 ** 31 - 1
    kps[la[20], 0] = np.nan
    kps[lb[21], 1] = np.nan
    t["link_a"], t["link_b"], t["kps"] = la, lb, kps
    return t


def odd_offsets_table(m=200):
    """Three edges over no range twice: the middle one's end lies beyond link_capacity, the last one's range is inverted."""
    fams = ("general", "sideways", "forward")
    t = make_table([problem(m, 0.0, 6100 + i, f) for i, f in enumerate(fams)], [f_true(*MOTIONS[f]) for f in fams])
    off = t["link_offsets"].copy()         # [0, m, 2 m, 3 m]
    off[2] = 2 ** 40                       # edge 1: [m, beyond) reads as [m, capacity): its own links and half of edge 2's
    off[3] = 2 * m + 50                    # edge 2: [capacity, 2 m + 50) is inverted: empty
    t["link_offsets"] = off
    t["link_capacity"] = int(2 * m + m // 2)
    return t


# ---- the float64 restatement -----------------------------------------------------------------------------------------
def _rays(kps, rows, k4):
    k4 = np.asarray(k4, np.float64)
    xy = np.asarray(kps, np.float32)[rows, :2].astype(np.float64)
    return np.stack([(xy[:, 0] - k4[2]) / k4[0], (xy[:, 1] - k4[3]) / k4[1], np.ones(len(rows))], axis=1)


def decompose(f, ka, kb):
    """None (no pose), or (candidates [(R, t)] * 4, sigma [3]) of F [9] f32 under intrinsics ka, kb (fx, fy, cx, cy) f32."""
    f = np.asarray(f, np.float32).astype(np.float64).reshape(3, 3)
    ka, kb = np.asarray(ka, np.float32).astype(np.float64), np.asarray(kb, np.float32).astype(np.float64)
    if not (np.isfinite(ka).all() and np.isfinite(kb).all() and ka[0] > 0 and ka[1] > 0 and kb[0] > 0 and kb[1] > 0):
        return None
    if not np.isfinite(f).all() or not f.any():
        return None
    mk = lambda k: np.array([[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1.0]])
    e = mk(kb).T @ f @ mk(ka)
    w, v = np.linalg.eigh(e.T @ e)
    order = np.argsort(-w, kind="stable")
    w, v = w[order], v[:, order]
    s = np.sqrt(np.maximum(w, 0.0))
    if not (np.isfinite(s[0]) and s[0] > 0) or s[1] <= 1e-3 * s[0]:
        return None
    v1, v2 = v[:, 0], v[:, 1]
    u1 = e @ v1
    u1 /= np.linalg.norm(u1)
    u2 = e @ v2
    u2 -= (u1 @ u2) * u1
    u2 /= np.linalg.norm(u2)
    u3, v3 = np.cross(u1, u2), np.cross(v1, v2)
    r1 = np.outer(u2, v1) - np.outer(u1, v2) + np.outer(u3, v3)
    r2 = np.outer(u1, v2) - np.outer(u2, v1) + np.outer(u3, v3)
    return [(r1, u3), (r1, -u3), (r2, u3), (r2, -u3)], s / s[0]


def vote(r, t, xa, xb):
    """det, na, nb, their margins (|value| over the sum of the magnitudes of its terms) and p.p, q.q, p.q per link."""
    p, q = xa @ r.T, xb
    pp, qq, pq, pt, qt = (p * p).sum(1), (q * q).sum(1), (p * q).sum(1), p @ t, q @ t
    det = pp * qq - pq * pq
    na = pq * qt - pt * qq
    nb = pp * qt - pq * pt
    with np.errstate(all="ignore"):
        ma = np.abs(na) / (np.abs(pq * qt) + np.abs(pt * qq))
        mb = np.abs(nb) / (np.abs(pp * qt) + np.abs(pq * pt))
    return {"det": det, "na": na, "nb": nb, "margin": np.minimum(ma, mb), "pp": pp, "qq": qq, "pq": pq}


def reference(t, deg):
    """The restatement over every edge of table t -> a list of dicts: pose (bool), R, t, sigma, stats (front, other, parallax;
    no candidate index), front [links] bool, points [links, 4] float64, margin (the smallest over links and candidates),
    parallax_margin, valid [links] (the entries that are links)."""
    cmin = np.cos(np.float64(np.float32(deg)) * (np.pi / 180.0))
    cap = int(t.get("link_capacity", len(t["link_a"])))
    n_rows, n_images = len(t["kps"]), len(t["intrinsics"])
    out = []
    for e in range(len(t["edge_a"])):
        lo, hi = (min(int(o), cap) for o in t["link_offsets"][e:e + 2])
        hi = max(hi, lo)
        la, lb = t["link_a"][lo:hi].astype(np.int64), t["link_b"][lo:hi].astype(np.int64)
        valid = (la >= 0) & (la < n_rows) & (lb >= 0) & (lb < n_rows)
        res = {"pose": False, "R": np.zeros((3, 3)), "t": np.zeros(3), "sigma": np.zeros(3), "stats": (0, 0, 0), "range": (lo, hi),
               "front": np.zeros(hi - lo, bool), "points": np.tile(NONE_ROW.astype(np.float64), (hi - lo, 1)), "valid": valid,
               "margin": np.inf, "parallax_margin": np.inf}
        out.append(res)
        a, b = int(t["edge_a"][e]), int(t["edge_b"][e])
        if a >= n_images or b >= n_images:
            continue
        dec = decompose(t["F"][e], t["intrinsics"][a], t["intrinsics"][b])
        if dec is None:
            continue
        cands, sigma = dec
        xa, xb = _rays(t["kps"], la[valid], t["intrinsics"][a]), _rays(t["kps"], lb[valid], t["intrinsics"][b])
        votes = [vote(r, tt, xa, xb) for r, tt in cands]
        fronts = [(v["det"] > 0) & (v["na"] > 0) & (v["nb"] > 0) for v in votes]
        counts = [int(f.sum()) for f in fronts]
        finite = np.isfinite(xa).all(1) & np.isfinite(xb).all(1)
        if finite.any():
            res["margin"] = min(float(v["margin"][finite].min()) for v in votes)
        c = int(np.argmax(counts))                     # the first of the largest
        if counts[c] == 0:
            continue
        r, tt = cands[c]
        v, front = votes[c], fronts[c]
        with np.errstate(all="ignore"):
            root = np.sqrt(v["pp"] * v["qq"])
            wide = front & (v["pq"] <= cmin * root)
            if front.any():
                res["parallax_margin"] = float((np.abs(v["pq"] - cmin * root) / root)[front].min())
            la_, lb_ = v["na"] / v["det"], v["nb"] / v["det"]
            x = 0.5 * (la_[:, None] * xa + (lb_[:, None] * xb - tt) @ r)
            pts = np.concatenate([x, (v["pq"] / root)[:, None]], axis=1)
        pts[~front] = NONE_ROW
        res["front"][valid] = front
        res["points"][valid] = pts
        res.update(pose=True, R=r, t=tt, sigma=sigma, stats=(counts[c], max(counts[:c] + counts[c + 1:]), int(wide.sum())),
                   other_R=cands[(c + 2) % 4][0])
    return out


def rotation_angle_deg(r1, r2):
    """The angle between two rotations in degrees, from the chord |r1 - r2|_F = 2 sqrt(2) sin(angle / 2) (an arccos of the
    trace resolves nothing below 1e-2 degrees for f32 entries)."""
    d = np.linalg.norm(np.asarray(r1, np.float64) - np.asarray(r2, np.float64))
    return float(np.degrees(2.0 * np.arcsin(min(d / (2.0 * np.sqrt(2.0)), 1.0))))
