"""A synthetic collection for the whole reconstruction chain, and the chain itself composed on the host.

`scene()` makes keypoints with no images, the way resect_cases.chain and bundle_cases.build do: eight cameras around one cloud,
a point seen by the cameras its group names, 0.5 px of noise, rows no match names, wrong matches, epipolar decoys that tie two
rows of one image into one track, one edge between two images that share no point, one image that sees too few points to be
registered and one that shares points only with images outside the initial pair.

`run_chain()` is the order in which examples/match_collection.py calls the stages, from the verifier to the bundle step, with
every stage's arithmetic left to a `backend`: `Reference` here composes the float64 numpy restatements of the stage tests
(fundamental_ref.verify, pose_cases.reference, triangulate_cases.reference, resect_cases.resect_image, bundle_cases.restate,
bundle_intr_cases.restate), tests/reconstruction_twin.py's backend runs the C++ twins.  The tables between them
(link_table_cases.link_table, tracks_cases.build_tracks, track_table_cases.track_table) are integer-exact restatements and
serve both.  A stage hands the next one its outputs as the device would hold them: f32 and 32-bit words.  No arithmetic of a
stage is restated here: an adapter only builds the dict the stage's module expects.

`in_gauge()` re-expresses the truth in the chain's gauge (the initial pair: camera a = [I | 0], |t| = 1), `errors()` measures a
chain's poses and points against it."""
import numpy as np

import bundle_cases
import bundle_intr_cases
import fundamental_ref
import link_table_cases
import pose_cases
import q8_edges_cases as ecases
import resect_cases
import track_table_cases
import tracks_cases
import triangulate_cases

NONE = 0xFFFFFFFF
N_IMAGES = 8
UNREGISTERABLE, LATE = 3, 7                 # the image that sees too few points; the image that registers in round 2
FALSE_EDGE = (0, 7)                         # two images that share no point
FOCAL_SCALE = 1.03                          # the second scene: the focal length handed to the chain is 3 % too long
# One set of parameters for the reference chain, the twin chain and the device chain.  n_hyp 64 and n_samples 8 are small
# because the Python RANSAC is slow (the reference chain takes about a second), and with them it still registers every
# registerable image on SEED; min_inliers 20 so that an image of 18 points is "too few" while its edges survive min_links 10,
# which the 8 matches F keeps of the false edge's 14 do not; resect_rounds 0 (no Gauss-Newton refit of the P3P winner) and the
# few samples so that the poses reach the bundle step as rough as a minimal sample leaves them: the bundle has work to do.
PARAMS = dict(n_hyp=64, f_thr=1.5, seed=5, min_links=10, pose_deg=1.0, px=4.0, tri_rounds=2, n_samples=8, min_inliers=20,
              resect_rounds=0, register=3, iterations=6, cg_iterations=10, cg_tol=0.1, lambda0=1e-3)
SEED = 10
CENTRES_X = (-2.6, -1.0, -0.3, 0.3, 0.9, 1.5, 2.1, 2.7)      # images 0 and 1 far apart: the gauge rests on a wide baseline


# ---- the scene -------------------------------------------------------------------------------------------------------------

def window_edges(n, w):
    pairs = [(t, t + d) for d in range(1, w + 1) for t in range(n - d)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def _visibility(rng):
    """seen [points, images] bool.  Group 1: the initial pair (0, 1) and the images that register from it in round 1; group 2:
    images 1, 2, 4, 5, never image 0; group 3: images 4 .. 7 -- the only points image 7 sees, none of them seen by 0 or 1, so
    image 7 has nothing to register from before 4, 5 and 6 are in.  Image 3 sees 18 points that 2 and 4 see too."""
    g1 = np.zeros((160, N_IMAGES), bool)
    g1[:, :2] = True
    for i, p in ((2, 0.8), (4, 0.7), (5, 0.6), (6, 0.6)):
        g1[:, i] = rng.random(160) < p
    g2 = np.zeros((100, N_IMAGES), bool)
    for i, p in ((1, 0.6), (2, 0.6), (4, 0.6), (5, 0.4)):
        g2[:, i] = rng.random(100) < p
    g2[g2.sum(1) < 2, 2] = g2[g2.sum(1) < 2, 4] = True
    g3 = np.zeros((120, N_IMAGES), bool)
    for i, p in ((4, 0.4), (5, 0.6), (6, 0.6), (7, 0.8)):
        g3[:, i] = rng.random(120) < p
    g3[g3.sum(1) < 2, 5] = g3[g3.sum(1) < 2, 6] = True
    seen = np.concatenate([g1, g2, g3])
    both = np.flatnonzero(seen[:, 2] & seen[:, 4])
    seen[rng.choice(both, 18, replace=False), UNREGISTERABLE] = True
    return seen


def scene(seed=SEED, noise=0.5, wrong=0.15, extra=20, decoys=4, false_matches=14):
    """-> dict: kps [rows, 5] f32 (the pool), offsets int64 [9], edge_a / edge_b int32 [14] (window 2, then FALSE_EDGE), matches
    (per edge an int32 array over image a's rows: the row within image b, or -1), K f32 [4], truth_poses [8, 12] and
    truth_points [380, 3] float64, row_point int64 [rows] (the point a row shows; -1: a row of no point), seen [380, 8]"""
    rng = np.random.default_rng(seed)
    K = np.array([1000.0, 1000.0, 640.0, 480.0])
    seen = _visibility(rng)
    n_points = len(seen)
    X = np.stack([rng.uniform(-3, 3, n_points), rng.uniform(-2, 2, n_points), rng.uniform(4, 8, n_points)], 1)
    centres = np.stack([np.array(CENTRES_X) + rng.normal(0, 0.1, N_IMAGES), rng.normal(0, 0.3, N_IMAGES),
                        rng.normal(0, 0.3, N_IMAGES)], 1)
    Rs = [resect_cases.rotation(rng.normal(0, 0.08, 3)) for _ in range(N_IMAGES)]
    truth = np.stack([np.concatenate([R.reshape(-1), -R @ c]) for R, c in zip(Rs, centres)])
    project = lambda i, Y: (lambda p: np.stack([K[0] * p[:, 0] / p[:, 2] + K[2], K[1] * p[:, 1] / p[:, 2] + K[3]], 1))(
        Y @ Rs[i].T + truth[i, 9:])
    ea, eb = window_edges(N_IMAGES, 2)
    ea, eb = ea + [FALSE_EDGE[0]], eb + [FALSE_EDGE[1]]
    # the decoys: for an edge (t, t + 1) a point that t, t + 1 and t + 2 all see; a row of image t + 1 that lies on the epipolar
    # line of the point's keypoint in image t (another depth on the same ray), to which the edge's match will point.  The true
    # row of t + 1 joins the track through (t + 1, t + 2) and (t, t + 2): two rows of one image in one track.
    decoy_of = {}                                               # (edge, point) -> the local row of image b
    decoy_xy = [[] for _ in range(N_IMAGES)]
    for t in (0, 4, 5):
        e = [k for k in range(len(ea)) if (ea[k], eb[k]) == (t, t + 1)][0]
        for p in rng.choice(np.flatnonzero(seen[:, t] & seen[:, t + 1] & seen[:, t + 2]), decoys, replace=False):
            Y = centres[t] + rng.uniform(1.3, 1.6) * (X[p] - centres[t])
            decoy_of[(e, int(p))] = len(decoy_xy[t + 1])
            decoy_xy[t + 1].append(project(t + 1, Y[None])[0] + rng.normal(0, 0.3, 2))
    kps, row_of, row_point, off = [], [], [], [0]
    for i in range(N_IMAGES):
        ids = np.flatnonzero(seen[:, i])
        xy = np.concatenate([project(i, X[ids]) + rng.normal(0, noise, (len(ids), 2)), np.array(decoy_xy[i]).reshape(-1, 2),
                             np.stack([rng.uniform(0, 2 * K[2], extra), rng.uniform(0, 2 * K[3], extra)], 1)])
        point = np.concatenate([ids, np.full(len(xy) - len(ids), -1)])
        order = rng.permutation(len(xy))
        k = np.zeros((len(xy), 5), np.float32)
        k[:, :2], k[:, 2] = xy[order], 8.0
        where = np.empty(len(xy), np.int64)
        where[order] = np.arange(len(xy))                       # the row of entry j of (points, decoys, extras)
        r = np.full(n_points, -1, np.int64)
        r[ids] = where[:len(ids)]
        decoy_xy[i] = where[len(ids):len(ids) + len(decoy_xy[i])]   # from here on: the decoys' rows
        kps.append(k), row_of.append(r), row_point.append(point[order]), off.append(off[-1] + len(xy))
    matches = []
    for e, (a, b) in enumerate(zip(ea, eb)):
        na, nb = off[a + 1] - off[a], off[b + 1] - off[b]
        m = np.full(na, -1, np.int32)
        if (a, b) == FALSE_EDGE:
            assert not (seen[:, a] & seen[:, b]).any()
            m[rng.choice(na, false_matches, replace=False)] = rng.integers(0, nb, false_matches)
        else:
            both = np.flatnonzero(seen[:, a] & seen[:, b])
            m[row_of[a][both]] = row_of[b][both]
            bad = both[rng.random(len(both)) < wrong]
            m[row_of[a][bad]] = rng.integers(0, nb, len(bad))
            for (ed, p), local in decoy_of.items():
                if ed == e:
                    m[row_of[a][p]] = decoy_xy[b][local]
        matches.append(m)
    return dict(kps=np.concatenate(kps), offsets=np.array(off, np.int64), edge_a=np.array(ea, np.int32), edge_b=np.array(eb, np.int32),
                matches=matches, K=K.astype(np.float32), truth_poses=truth, truth_points=X, row_point=np.concatenate(row_point),
                seen=seen)


def intrinsics(s, scale=1.0):
    """[n_images, 4] f32: the scene's camera for every image, its focal lengths times `scale`"""
    K = np.tile(s["K"], (N_IMAGES, 1)).astype(np.float32)
    K[:, :2] *= np.float32(scale)
    return K


# ---- the gauge and the errors ----------------------------------------------------------------------------------------------

def in_gauge(s, a, b):
    """the truth with camera a at [I | 0] and camera b at distance 1 from it: (poses [n, 12], points [P, 3]) float64"""
    P = s["truth_poses"]
    Ra, ta = P[a, :9].reshape(3, 3), P[a, 9:]
    Rb = P[b, :9].reshape(3, 3) @ Ra.T
    scale = 1.0 / np.linalg.norm(P[b, 9:] - Rb @ ta)
    poses = np.zeros_like(P)
    for i in range(len(P)):
        R = P[i, :9].reshape(3, 3) @ Ra.T
        poses[i] = np.concatenate([R.reshape(-1), scale * (P[i, 9:] - R @ ta)])
    return poses, scale * (s["truth_points"] @ Ra.T + ta)


def track_points(s, table):
    """per track of the table the scene's point most of its rows show (-1: none does)"""
    T = table.counts[0]
    out = np.full(T, -1, np.int64)
    for t in range(T):
        ids = s["row_point"][table.obs_row[int(table.offsets[t]):int(table.offsets[t + 1])]]
        ids = ids[ids >= 0]
        if len(ids):
            v, c = np.unique(ids, return_counts=True)
            out[t] = v[np.argmax(c)]
    return out


def errors(s, chain, poses, points):
    """(largest rotation error in radians, largest distance of the camera centres, median point error) of poses [n, 12] and
    points [tracks, 4] against the truth in the chain's gauge: over the registered images, and over the tracks with a point"""
    a, b = chain["pair"]
    tp, tx = in_gauge(s, a, b)
    P = np.asarray(poses, np.float64)
    reg = np.flatnonzero((P[:, :9] != 0).any(1))
    e = [bundle_cases.pose_error(P[i], tp[i]) for i in reg]
    T = chain["table"].counts[0]
    X = np.asarray(points, np.float64)[:T]
    ids = track_points(s, chain["table"])
    have = (X[:, 3] <= 1) & (ids >= 0)
    d = np.linalg.norm(X[have, :3] - tx[ids[have]], axis=1)
    return max(x[0] for x in e), max(x[1] for x in e), float(np.median(d))


def focal_error(groups):
    """|s * 1.03 - 1| of the second scene's refined focal scale"""
    return float(bundle_intr_cases.focal_error(FOCAL_SCALE, np.asarray(groups, np.float32).reshape(-1, 3))[0])


# ---- the chain -------------------------------------------------------------------------------------------------------------

def u32(a):
    """the words of an f32 / int32 / uint32 array"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a.astype(np.uint32)


def f32(words):
    return np.ascontiguousarray(words, np.uint32).view(np.float32)


def layouts(s):
    """(layout_a, layout_b, capacity_a, capacity_b, match): both sides' edge layouts, and the matches in the a side's"""
    off, n = s["offsets"], int(s["offsets"][-1])
    la, lb = ecases.edge_layout(off, n, s["edge_a"]).astype(np.int64), ecases.edge_layout(off, n, s["edge_b"]).astype(np.int64)
    return la, lb, int(la[-1]), int(lb[-1]), np.concatenate(s["matches"]).astype(np.int32)


def initial_pair(stats):
    """the edge with the most links with parallax among the edges that have a pose (the first of them): stats [E, 4] words"""
    st = np.asarray(stats).astype(np.uint32).view(np.int32).reshape(-1, 4)
    return int(np.argmax(np.where(st[:, 2] >= 0, st[:, 3], -1)))


def run_chain(s, K, backend, focal=False, params=PARAMS):
    """The chain on scene `s` under the intrinsics K [n_images, 4] f32.  Every stage's outputs are words (uint32 arrays; the
    trace uint64) shaped as the device call writes them, cut to what the header defines: `verify` (F [E, 9], verified, stats
    [E, 4]), `links` (link_table_cases.Table), `pose` (R, t, stats, sigma, points [links, 4]), `edge` and `pair` (the initial
    pair), `tracks` (track, length, dup), `table` (track_table_cases.Table), `tri` (a list: the first triangulation, then one
    per round) and `resect` (one per round), `poses0` (before the rounds), `poses` (after them), `held`, `bundle` (the last
    stage; with focal=True bundle_adjust_intrinsics with one group and the focal scale refined)."""
    p = params
    kps, off, ea, eb = s["kps"], s["offsets"], s["edge_a"], s["edge_b"]
    n, n_images, E = len(kps), len(off) - 1, len(ea)
    la, lb, cap, _, match = layouts(s)
    out = dict(params=p, K=K)
    # verify, edge by edge: the pair's keypoints in the two edge layouts, seed + e
    F, ver, vst = np.zeros((E, 9), np.uint32), np.full(cap, -1, np.int32), np.zeros((E, 4), np.uint32)
    for e in range(E):
        a, b = int(ea[e]), int(eb[e])
        f, v, st = backend.verify(e, kps[off[a]:off[a + 1]], kps[off[b]:off[b + 1]], match[la[e]:la[e + 1]], p["n_hyp"], p["f_thr"],
                                  p["seed"] + e)
        F[e], ver[la[e]:la[e + 1]], vst[e] = u32(f).reshape(9), v, st
    out["verify"] = dict(F=F, verified=ver, stats=vst)
    links = link_table_cases.link_table(off, n, ea, eb, la, cap, ver, min_links=p["min_links"], into=np.full(cap, -1, np.int32))
    out["links"] = links
    table = dict(kps=kps, edge_a=ea.astype(np.uint32), edge_b=eb.astype(np.uint32), intrinsics=K, F=f32(F), link_offsets=links.offsets,
                 link_a=links.link_a, link_b=links.link_b)
    out["pose"] = pose = backend.pose(table, p["pose_deg"])
    e0 = out["edge"] = initial_pair(pose["stats"])
    out["pair"] = (int(ea[e0]), int(eb[e0]))
    poses = np.zeros((n_images, 12), np.float32)
    poses[ea[e0]] = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    poses[eb[e0]] = np.concatenate([f32(pose["R"][e0]), f32(pose["t"][e0])])
    out["poses0"] = u32(poses.copy())
    track, length, dup = tracks_cases.build_tracks(off, n, ea, eb, la, cap, links.match_kept)
    out["tracks"] = dict(track=track, length=length, dup=dup)
    tt = out["table"] = track_table_cases.track_table(track, length, dup, min_len=2, consistent=True, image_offsets=off)
    counts = np.array(tt.counts[:2], np.uint32)
    tri_in = lambda P: dict(kps=kps, track_offsets=tt.offsets, obs_row=tt.obs_row, obs_image=tt.obs_image, counts=counts, intrinsics=K,
                            poses=P)
    out["tri"] = [backend.triangulate(tri_in(poses), p["px"], p["tri_rounds"])]
    out["resect"] = []
    held = (poses[:, :9] != 0).any(1).astype(np.uint32)
    for _ in range(p["register"]):
        sc = dict(kps=kps, image_offsets=off.astype(np.uint64), row_track=tt.row_track, points=f32(out["tri"][-1]["points"]),
                  counts=counts, intrinsics=K, poses=poses)
        r = backend.resect(sc, px=p["px"], deg=0.0, n_samples=p["n_samples"], min_inliers=p["min_inliers"], rounds=p["resect_rounds"],
                           seed=p["seed"], flags=0)
        poses = f32(r["poses"]).reshape(n_images, 12).copy()
        out["resect"].append(r)
        out["tri"].append(backend.triangulate(tri_in(poses), p["px"], p["tri_rounds"]))
    out["poses"], out["held"] = u32(poses.copy()), held
    last = out["tri"][-1]
    sc = dict(kps=kps, image_offsets=off.astype(np.uint64), track_offsets=tt.offsets, obs_row=tt.obs_row, obs_image=tt.obs_image,
              counts=counts, points=f32(last["points"]), intrinsics=K, poses=poses, obs_state=last["obs_state"], camera_fixed=held)
    kw = dict(px=p["px"], lambda0=p["lambda0"], iterations=p["iterations"], cg_iterations=p["cg_iterations"], cg_tol=p["cg_tol"])
    out["bundle"] = backend.bundle_intrinsics(dict(sc, camera_group=None, n_groups=1), refine=1, **kw) if focal else backend.bundle(sc, **kw)
    return out


def tracks_with_point(tri, T):
    return int((np.asarray(tri["stats"])[:T, 2] == 0).sum())


class Reference:
    """the stages as the float64 numpy restatements compute them, their results rounded to the words a device call leaves"""

    def __init__(self):
        self._verified = {}

    def verify(self, e, ka, kb, match, n_hyp, thr, seed):
        # (F does not depend on the intrinsics: the two scenes of one collection share it)
        key = (ka.tobytes(), kb.tobytes(), match.tobytes(), n_hyp, thr, seed)
        if key not in self._verified:
            r = fundamental_ref.verify(ka, kb, match, n_hyp, thr, seed)
            self._verified[key] = (np.asarray(r["F"], np.float32).reshape(9), r["verified"].astype(np.int32),
                                   (np.asarray(r["stats"], np.int64) & 0xFFFFFFFF).astype(np.uint32))
        return self._verified[key]

    def pose(self, table, deg):
        ref = pose_cases.reference(table, deg)
        E, L = len(ref), len(table["link_a"])
        R, t, sg = np.zeros((E, 9), np.float32), np.zeros((E, 3), np.float32), np.zeros((E, 3), np.float32)
        st, pts = np.zeros((E, 4), np.uint32), np.tile(pose_cases.NONE_ROW, (L, 1))
        for e, r in enumerate(ref):
            lo, hi = r["range"]
            R[e], t[e], sg[e] = r["R"].reshape(9), r["t"], r["sigma"]
            st[e] = (r["stats"][0], r["stats"][1], 0 if r["pose"] else NONE, r["stats"][2])    # (the candidate's index is its own)
            pts[lo:hi] = r["points"]
        return dict(R=u32(R), t=u32(t), stats=st, sigma=u32(sg), points=u32(pts))

    def triangulate(self, table, px, rounds):
        r = triangulate_cases.reference(table, px, rounds)
        return dict(points=u32(r["points"].astype(np.float32)), stats=(r["stats"] & 0xFFFFFFFF).astype(np.uint32),
                    err=u32(r["err"].astype(np.float32)), obs_state=r["obs_state"][:int(table["counts"][1])].astype(np.uint32))

    def resect(self, sc, px, deg, n_samples, min_inliers, rounds, seed, flags):
        n_images = len(sc["intrinsics"])
        poses, stats = np.array(sc["poses"], np.float32), np.zeros((n_images, 4), np.uint32)
        err, state = np.zeros((n_images, 2), np.float32), np.full(len(sc["kps"]), NONE, np.uint32)
        off = np.asarray(sc["image_offsets"]).astype(np.int64)
        for i in range(n_images):
            K = sc["intrinsics"][i].astype(np.float64)
            if not resect_cases.candidate_image(K, sc["poses"][i], bool(flags & 1)):
                stats[i] = (0, 0, 1, NONE)
                continue
            rows, cs = resect_cases.correspondences(sc, i, deg)
            r = resect_cases.resect_image(cs, K, seed + i, px, n_samples, min_inliers, rounds)
            poses[i], stats[i], err[i] = r["pose"], r["stats"], r["err"]
            state[off[i]:off[i + 1]] = 0
            state[rows] = np.where(r["inlier"], 2, 1)
        return dict(poses=u32(poses), stats=stats, err=u32(err), row_state=state)

    @staticmethod
    def _bundle_words(r):
        out = dict(poses=u32(r["poses"]), points=u32(r["points"]), obs_state=(r["obs_state"] & 0xFFFFFFFF).astype(np.uint32),
                   trace=r["trace"], counts=np.asarray(r["counts"]).astype(np.uint32))
        if "groups" in r:
            out.update(intrinsics=u32(r["intrinsics"]), groups=u32(r["groups"]))
        return out

    def bundle(self, sc, **kw):
        return self._bundle_words(bundle_cases.restate(sc, **kw))

    def bundle_intrinsics(self, sc, refine, **kw):
        return self._bundle_words(bundle_intr_cases.restate(sc, refine=refine, **kw))
