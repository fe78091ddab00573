"""Scenes for the view-graph call and a float64 numpy restatement of its definitions (include/lf_mkd.h,
lf_mkd_view_graph_device), written from the header's text and not from csrc/mkd_view_graph_math.h.

A scene has no keypoints: image rotations (the truth, world to camera), an edge list, each edge's relative rotation R with
R_b = R R_a (about 0.5 degrees of noise on a right edge, a further 10 .. 180 degrees on a wrong one) and pose statistics as
lf_mkd_two_view_pose_device writes them (a wrong edge has fewer links in front), and a match array laid out edge by edge for
the filter.  `reference()` states the definitions serially: integer words are exact, the averaging sums in plain order (the
canonical slot order is the twin's business), so its f32 words agree with the twin's within a measured gate only."""
import numpy as np

NONE = 0xFFFFFFFF
UNUSABLE, REJECTED, UNCHECKED, SUPPORTED = 0, 1, 2, 3
USE_UNCHECKED = 1


# ---- rotations ---------------------------------------------------------------------------------------------------------------

def rotation(axis, angle):
    """Rodrigues: the rotation by `angle` (rad) about `axis`"""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def angle_of(R):
    """the rotation angle of a 3x3 matrix (rad)"""
    return float(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))


def _random_rotation(rng, sigma):
    v = rng.normal(0.0, sigma, 3)
    a = np.linalg.norm(v)
    return rotation(v, a) if a > 0 else np.eye(3)


# ---- scenes ------------------------------------------------------------------------------------------------------------------

def _finish(n, edges, truth, wrong, rng, noise_deg, stats=None):
    """relative rotations, statistics and a match layout for the edge list"""
    E = len(edges)
    R = np.zeros((E, 9), np.float32)
    ps = np.zeros((E, 4), np.uint32)
    order = rng.permutation(E)
    for e, (a, b) in enumerate(edges):
        rel = truth[b] @ truth[a].T
        rel = _random_rotation(rng, np.deg2rad(noise_deg) / np.sqrt(3.0)) @ rel
        if wrong[e]:
            rel = rotation(rng.normal(size=3), np.deg2rad(rng.uniform(10.0, 180.0))) @ rel
        R[e] = rel.reshape(9).astype(np.float32)
        front = int(rng.integers(20, 60)) if wrong[e] else 100 + int(order[e])   # right edges: all different, so no tie in the tree
        ps[e] = [front, front // 10, int(rng.integers(0, 4)), (front * 4) // 5]
    lens = rng.integers(3, 10, E)
    off = np.concatenate([[5], 5 + np.cumsum(lens)]).astype(np.uint64)          # entries 0 .. 4 and the last 7 are in no range
    match = rng.integers(-1, 40, int(off[-1]) + 7).astype(np.int32)
    return dict(n_images=n, edge_a=np.array([e[0] for e in edges], np.uint32), edge_b=np.array([e[1] for e in edges], np.uint32),
                R=R, pose_stats=ps, truth=truth, wrong=np.asarray(wrong, bool), edge_offsets=off, match=match, params={})


def ring(n, window, chords, wrong_fraction, seed, noise_deg=0.5):
    """n cameras in a ring, every one tied to its `window` successors, `chords` random further pairs; every second edge is stored
    as (later, earlier); wrong_fraction of the edges get a wrong rotation"""
    rng = np.random.default_rng(seed)
    truth = np.stack([_random_rotation(rng, 1.0) for _ in range(n)])
    pairs = [(i, (i + k) % n) for i in range(n) for k in range(1, window + 1)]
    have = {frozenset(p) for p in pairs}
    while len(pairs) < n * window + chords:
        i, j = (int(x) for x in rng.integers(0, n, 2))
        if i != j and frozenset((i, j)) not in have:
            have.add(frozenset((i, j)))
            pairs.append((i, j))
    edges = [(b, a) if k % 2 else (a, b) for k, (a, b) in enumerate(pairs)]
    wrong = np.zeros(len(edges), bool)
    wrong[rng.choice(len(edges), int(round(wrong_fraction * len(edges))), replace=False)] = True
    return _finish(n, edges, truth, wrong, rng, noise_deg)


SEEDS = dict(A=3, B=4, C=5, D=6)


def scene_a():
    return ring(24, 3, 6, 0.10, SEEDS["A"])


def scene_b():
    return ring(64, 4, 20, 0.15, SEEDS["B"])


def scene_c():
    """300 images: a row of the table is longer than one 256-lane pass (and than four 64-lane ones)"""
    s = ring(300, 4, 0, 0.10, SEEDS["C"])
    s["params"] = dict(tree_rounds=48)                                          # the ring is 38 steps of 4 deep
    return s


D_MIN_FRONT = 10
D = dict(padding=12, self_edge=13, no_pose=14, few_front=15, nan=16, duplicate=17, representative=2, bridge=24, isolated=10,
         second_cluster=(6, 7, 8, 9))


def scene_d():
    """the edge cases in one list: images 0 .. 5 a ring of window 2 (edges 0 .. 11), then the padding, a self edge, an edge
    without a pose, one below min_front, one with a NaN, pair (1, 2) once more as (2, 1) with R transposed, the complete graph
    on images 6 .. 9 (edges 18 .. 23), the bridge (5, 6) that closes no triangle, and image 10 that no edge names"""
    rng = np.random.default_rng(SEEDS["D"])
    n = 11
    truth = np.stack([_random_rotation(rng, 1.0) for _ in range(n)])
    edges = [(i, (i + k) % 6) for i in range(6) for k in (1, 2)]                # (1, 2) is edge 2
    assert edges[D["representative"]] == (1, 2)
    edges += [(0, 0), (2, 2), (0, 3), (1, 4), (2, 5), (2, 1)]                   # 12 .. 17 (12 becomes the padding)
    edges += [(i, j) for i in range(6, 10) for j in range(i + 1, 10)]           # 18 .. 23
    edges += [(5, 6)]                                                           # 24
    s = _finish(n, edges, truth, np.zeros(len(edges), bool), rng, 0.5)
    s["edge_a"][D["padding"]] = s["edge_b"][D["padding"]] = NONE
    s["pose_stats"][D["no_pose"]] = [0, 0, NONE, 0]
    s["pose_stats"][D["few_front"], 0] = D_MIN_FRONT - 1
    s["R"][D["nan"], 4] = np.nan
    s["R"][D["duplicate"]] = s["R"][D["representative"]].reshape(3, 3).T.reshape(9)
    s["params"] = dict(min_front=D_MIN_FRONT)
    return s


def shuffled(s, seed=1):
    """the same scene with its edge list in another order: (scene, perm) with new edge k = old edge perm[k]"""
    perm = np.random.default_rng(seed).permutation(len(s["edge_a"]))
    lens = np.diff(s["edge_offsets"].astype(np.int64))[perm]
    off = np.concatenate([[5], 5 + np.cumsum(lens)]).astype(np.uint64)
    match = s["match"].copy()
    for k, e in enumerate(perm):
        match[int(off[k]):int(off[k + 1])] = s["match"][int(s["edge_offsets"][e]):int(s["edge_offsets"][e + 1])]
    t = dict(s, edge_a=s["edge_a"][perm], edge_b=s["edge_b"][perm], R=s["R"][perm], pose_stats=s["pose_stats"][perm],
             wrong=s["wrong"][perm], edge_offsets=off, match=match)
    return t, perm


# ---- the restatement ---------------------------------------------------------------------------------------------------------

def _quat(R):
    """definition 2: Shepperd's method on the f32 entries widened to f64, one normalisation"""
    r = np.asarray(R, np.float64).reshape(3, 3)
    t = r[0, 0] + r[1, 1] + r[2, 2]
    k = int(np.argmax([t, r[0, 0], r[1, 1], r[2, 2]]))                          # (argmax takes the lowest index on a tie)
    if k == 0:
        q = [1 + t, r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1]]
    elif k == 1:
        q = [r[2, 1] - r[1, 2], 1 + r[0, 0] - r[1, 1] - r[2, 2], r[0, 1] + r[1, 0], r[0, 2] + r[2, 0]]
    elif k == 2:
        q = [r[0, 2] - r[2, 0], r[0, 1] + r[1, 0], 1 - r[0, 0] + r[1, 1] - r[2, 2], r[1, 2] + r[2, 1]]
    else:
        q = [r[1, 0] - r[0, 1], r[0, 2] + r[2, 0], r[1, 2] + r[2, 1], 1 - r[0, 0] - r[1, 1] + r[2, 2]]
    q = np.array(q, np.float64)
    return q / np.sqrt(q @ q)


def _mul(p, q):
    pw, pv, qw, qv = p[0], p[1:], q[0], q[1:]
    return np.concatenate([[pw * qw - pv @ qv], pw * qv + qw * pv + np.cross(pv, qv)])


def _conj(q):
    return np.array([q[0], -q[1], -q[2], -q[3]])


def _matrix(q):
    w, x, y, z = q
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def reference(s, deg=3.0, min_front=0, root=NONE, tree_rounds=16, iterations=10, flags=0, match=True):
    """The definitions of include/lf_mkd.h, serially, in float64: a dict of rotations f32 [n, 9], edge_stats uint32 [E, 4],
    residual f32 [E], image_stats uint32 [n, 4], counts uint32 [8], match_out int32 or None (out of place: a copy of match),
    and `tree` = the rotations f32 [n, 9] before the first sweep."""
    n, ea, eb = int(s["n_images"]), np.asarray(s["edge_a"], np.int64), np.asarray(s["edge_b"], np.int64)
    E, R, ps = len(ea), np.asarray(s["R"], np.float32).reshape(-1, 9), np.asarray(s["pose_stats"], np.uint32).reshape(-1, 4)
    cmax = np.cos(np.float64(np.float32(deg)) * (np.pi / 180.0))
    unchecked_too = bool(flags & USE_UNCHECKED)
    usable = [bool(ea[e] < n and eb[e] < n and ea[e] != eb[e] and ps[e, 2] != NONE and ps[e, 0] >= min_front and np.isfinite(R[e]).all())
              for e in range(E)]
    q = {e: _quat(R[e]) for e in range(E) if usable[e]}
    rep = {}
    for e in range(E):
        if usable[e]:
            rep.setdefault(frozenset((int(ea[e]), int(eb[e]))), e)
    nbr = [dict() for _ in range(n)]                                            # nbr[i][j] = the representative of {i, j}
    for pair, e in rep.items():
        i, j = tuple(pair)
        nbr[i][j] = nbr[j][i] = e
    directed = lambda e, x: q[e] if ea[e] == x else _conj(q[e])                 # q(x -> the other end) of representative e
    edge_stats = np.zeros((E, 4), np.uint32)
    edge_stats[:, 3] = NONE
    image_stats = np.zeros((n, 4), np.uint32)
    image_stats[:, 1:3] = NONE
    counts = np.zeros(8, np.uint32)
    for e in range(E):
        if not usable[e]:
            continue
        a, b = int(ea[e]), int(eb[e])
        closed = consistent = 0
        for c in sorted(set(nbr[a]) & set(nbr[b])):
            L = _mul(directed(nbr[a][c], c), _mul(directed(nbr[b][c], b), q[e]))
            closed += 1
            consistent += bool(2 * L[0] * L[0] - 1 >= cmax)
        state = SUPPORTED if consistent else REJECTED if closed else UNCHECKED
        edge_stats[e] = [closed, consistent, state, nbr[a][b]]
        counts[0] += 1
        counts[{SUPPORTED: 1, REJECTED: 2, UNCHECKED: 3}[state]] += 1
        if state == REJECTED:
            image_stats[[a, b], 3] += 1
    kept = lambda e: edge_stats[e, 3] == e and (edge_stats[e, 2] == SUPPORTED or (unchecked_too and edge_stats[e, 2] == UNCHECKED))
    for e in range(E):
        if usable[e] and kept(e):
            counts[4] += 1
            image_stats[[int(ea[e]), int(eb[e])], 0] += 1
    Q = np.zeros((n, 4))
    if root == NONE and E:
        root = int(np.argmax(image_stats[:, 0])) if n else NONE                 # (the lowest id on a tie)
    if root != NONE:
        image_stats[root, 1], Q[root] = 0, [1, 0, 0, 0]
        if E:
            counts[5], counts[6] = 1, root
    for r in range(1, tree_rounds + 1):
        new = {}
        for i in range(n):
            if image_stats[i, 1] != NONE:
                continue
            cand = [(-int(edge_stats[e, 2]), -int(ps[e, 0]), e, j) for j, e in nbr[i].items() if kept(e) and image_stats[j, 1] < r]
            if cand:
                _, _, e, j = min(cand)
                p = _mul(directed(e, j), Q[j])
                new[i] = (p / np.sqrt(p @ p), e)
        for i, (p, e) in new.items():
            Q[i], image_stats[i, 1], image_stats[i, 2] = p, r, e
            counts[5] += 1
    labelled = image_stats[:, 1] != NONE
    tree = Q.copy()
    for _ in range(iterations):
        nxt = Q.copy()
        for i in range(n):
            if not labelled[i] or image_stats[i, 1] == 0:
                continue
            terms = []
            for j in sorted(nbr[i]):
                e = nbr[i][j]
                if kept(e) and labelled[j]:
                    p = _mul(directed(e, j), Q[j])
                    terms.append(-p if p @ Q[i] < 0 else p)
            if terms:
                v = np.sum(terms, axis=0) + len(terms) * Q[i]
                nxt[i] = v / np.sqrt(v @ v)
        Q = nxt
    to_rows = lambda quats: np.stack([_matrix(quats[i]).reshape(9) if labelled[i] else np.zeros(9) for i in range(n)]).astype(np.float32) \
        if n else np.zeros((0, 9), np.float32)
    residual = np.full(E, 2.0, np.float32)
    for e in range(E):
        if usable[e] and labelled[ea[e]] and labelled[eb[e]]:
            d = Q[eb[e]] @ _mul(q[e], Q[ea[e]])
            residual[e] = np.float32(2 * d * d - 1)
    out = None
    if match and s.get("match") is not None:
        out, off, cap = s["match"].copy(), s["edge_offsets"].astype(np.int64), len(s["match"])
        for e in range(E):
            lo, hi = min(off[e], cap), min(off[e + 1], cap)
            if not (usable[e] and kept(e)):
                out[lo:hi] = -1
    return dict(rotations=to_rows(Q), tree=to_rows(tree), edge_stats=edge_stats, residual=residual, image_stats=image_stats,
                counts=counts, match_out=out)


# ---- against the truth -------------------------------------------------------------------------------------------------------

def gauge_error(rotations, image_stats, truth):
    """the largest rotation error (rad) over the labelled images against the truth in the root's gauge, R_i R_root^T"""
    st = np.asarray(image_stats).reshape(-1, 4)
    root = np.flatnonzero(st[:, 1] == 0)
    if len(root) == 0:
        return 0.0
    R = np.asarray(rotations, np.float64).reshape(-1, 3, 3)
    worst = 0.0
    for i in np.flatnonzero(st[:, 1] != NONE):
        worst = max(worst, angle_of(R[i] @ (truth[i] @ truth[root[0]].T).T))
    return worst


def residual_angles(residual):
    """the residual cosines as angles (rad); none (2) as NaN"""
    r = np.asarray(residual, np.float64)
    return np.where(r > 1.5, np.nan, np.arccos(np.clip(r, -1.0, 1.0)))
