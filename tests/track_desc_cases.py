"""Track descriptors (include/lf_mkd.h, lf_mkd_track_descriptors_device): the cases the CPU and GPU tests share, a numpy
restatement of the contract, and the driver of the host twin (tests/cpp/track_desc_twin.cpp: the kernel's own
csrc/mkd_track_desc_math.h compiled by g++ under -fsanitize=address,undefined).

A call is a dict under the device call's argument names: q [rows, 128] uint8, track_offsets uint64 [track_capacity + 1],
obs_row int32 [obs_capacity], counts uint32 [2], obs_state uint32 [obs_capacity] or None, min_state, points f32
[track_capacity, 4] or None, deg, scale, stats (bool).  The restatement shares no code with the header: int64 sums,
np.rint((S * scale) / np.sqrt(n2)) in float64, an int32 spread."""
import os
import struct
import subprocess

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "local-features_amd", "csrc")
INT32_MIN = -2 ** 31
MAX_OBS = 65536
LENGTHS = (1, 2, 3, 7, 8, 9, 63, 64, 65, 256, 257)      # around the group's 8 lanes, the wave's 64 and the long-track seam
LONG = 70000                                            # crosses the 65 536 cap


# ---- the restatement ----------------------------------------------------------------------------------------------

def restate(c):
    """-> (desc uint8 [track_capacity, 128], stats int32 [track_capacity, 2])"""
    q = np.asarray(c["q"], np.uint8).reshape(-1, 128)
    off, row = np.asarray(c["track_offsets"], np.uint64).astype(np.int64), np.asarray(c["obs_row"], np.int32).astype(np.int64)
    tcap, ocap, n = len(off) - 1, len(row), len(q)
    T, O = min(int(c["counts"][0]), tcap), min(int(c["counts"][1]), ocap)
    scale = np.float64(np.float32(c["scale"]) if np.float32(c["scale"]) != 0 else np.float32(256))
    cmin = np.cos(np.float64(np.float32(c["deg"])) * (np.pi / 180.0))
    desc, stats = np.full((tcap, 128), 128, np.uint8), np.zeros((tcap, 2), np.int32)
    stats[:, 1] = INT32_MIN
    for t in range(T):
        lo, hi = min(off[t], O), min(off[t + 1], O)
        hi = min(max(lo, hi), lo + MAX_OBS)
        r = row[lo:hi]
        keep = (r >= 0) & (r < n)
        if c["obs_state"] is not None:
            keep &= np.asarray(c["obs_state"], np.uint32)[lo:hi] >= c["min_state"]
        C = int(keep.sum())
        stats[t, 0] = C
        described = True
        if c["points"] is not None:
            p = np.asarray(c["points"], np.float32).reshape(-1, 4)[t]
            with np.errstate(invalid="ignore"):
                described = bool(np.isfinite(p[:3]).all() and np.float64(p[3]) <= cmin)
        if not described or C == 0:
            continue
        centred = q[r[keep]].astype(np.int64) - 128
        S = centred.sum(axis=0)
        n2 = int((S * S).sum())
        if n2 == 0:
            continue
        qq = np.clip(np.rint((S.astype(np.float64) * scale) / np.sqrt(np.float64(n2))), -127, 127).astype(np.int64)
        desc[t] = (qq + 128).astype(np.uint8)
        stats[t, 1] = np.int32((centred @ qq).min())
    return desc, stats


# ---- the generator ------------------------------------------------------------------------------------------------

def pool(rng, n):
    """n quantised unit rows; the first 10 are raw bytes 0 .. 255 (rows that hold byte 0)"""
    x = rng.normal(size=(n, 128))
    x /= np.linalg.norm(x, axis=1)[:, None]
    q = (np.clip(np.rint(x * 256), -127, 127) + 128).astype(np.uint8)
    q[:10] = rng.integers(0, 256, (10, 128), dtype=np.uint8)
    q[0, :4] = 0
    return q


def table(tracks, track_capacity=None, obs_capacity=None, pad_row=-7):
    """the CSR arrays of a list of row lists; capacities beyond them hold offsets that go on rising and rows that are no row"""
    lens = np.array([len(t) for t in tracks], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    rows = np.concatenate([np.asarray(t, np.int64) for t in tracks] + [np.zeros(0, np.int64)])
    T, Oc = len(tracks), len(rows)
    tcap = T if track_capacity is None else track_capacity
    ocap = Oc if obs_capacity is None else obs_capacity
    off = np.concatenate([off, off[-1] + 3 * np.arange(1, tcap - T + 1)])
    rows = np.concatenate([rows, np.full(ocap - Oc, pad_row, np.int64)])
    return off.astype(np.uint64), rows.astype(np.int32), np.array([T, Oc], np.uint32)


def call(q, tracks, track_capacity=None, obs_capacity=None, obs_state=None, min_state=2, points=None, deg=0.0, scale=256.0,
         stats=True):
    off, rows, counts = table(tracks, track_capacity, obs_capacity)
    return dict(q=q, track_offsets=off, obs_row=rows, counts=counts, obs_state=obs_state, min_state=min_state, points=points,
                deg=deg, scale=scale, stats=stats)


def length_tracks(seed=1, n_rows=3000, long=LONG):
    """(q, tracks): every length of LENGTHS, an empty track, one of `long` positions, a spike, a cancelling pair, rows that hold
    byte 0, and rows that are no row (-1, n_rows, INT32_MAX) among valid ones"""
    rng = np.random.default_rng(seed)
    q = pool(rng, n_rows)
    spike = np.full(128, 128, np.uint8)
    spike[37] = 255
    q[10] = spike                                   # one contributor: v = scale at one k, the clamp at 127
    q[12] = (256 - q[11].astype(np.int64)).astype(np.uint8)     # q[11] + q[12] cancel (quantised bytes are 1 .. 255)
    tracks = [rng.integers(13, n_rows, n).tolist() for n in LENGTHS]
    tracks += [[], [10], [11, 12], [0, 1, 2], [3, -1, 4, n_rows, 5, 0x7FFFFFFF], [-1, n_rows], rng.integers(0, n_rows, 20).tolist()]
    if long:
        tracks.insert(4, rng.integers(0, n_rows, long).tolist())
    return q, tracks


def lengths(seed=1, long=LONG, **kw):
    q, tracks = length_tracks(seed, long=long)
    T, Oc = len(tracks), sum(len(t) for t in tracks)
    return call(q, tracks, track_capacity=T + 5, obs_capacity=Oc + 11, **kw)


def no_tracks():
    c = lengths(long=0)
    c["counts"] = np.array([0, c["counts"][1]], np.uint32)
    return c


def counts_beyond():
    """d_table_counts above both capacities: every row of the capacity is a track, read from offsets that stay inside"""
    q, tracks = length_tracks(2, long=0)
    c = call(q, tracks)
    c["counts"] = np.array([len(tracks) + 1000, len(c["obs_row"]) + 1000], np.uint32)
    return c


def wild_offsets():
    """offsets beyond the observations, an inverted range, a range that reaches past O"""
    c = lengths(3, long=0)
    off = c["track_offsets"].astype(np.int64)
    O = int(c["counts"][1])
    off[3], off[4] = off[4], off[3]
    off[9] = O + 1000
    off[int(c["counts"][0])] = 1 << 62
    off[int(c["counts"][0]) - 2] = O - 7
    c["track_offsets"] = off.astype(np.uint64)
    return c


def states(min_state, seed=4):
    """random states 0 .. 2 and a 7; track 0 has state 0 everywhere (no contributor from min_state 1 on)"""
    c = lengths(seed, long=0)
    rng = np.random.default_rng(seed)
    st = rng.integers(0, 3, len(c["obs_row"])).astype(np.uint32)
    off = c["track_offsets"].astype(np.int64)
    st[off[5]:off[6]] = 0
    st[off[8]] = 7
    c.update(obs_state=st, min_state=min_state)
    return c


def point_filter(deg, seed=5):
    """points: real ones, the "none" row, NaN and Inf, parallax cosines at and next to cos(deg)"""
    c = lengths(seed, long=0)
    rng = np.random.default_rng(seed)
    tcap = len(c["track_offsets"]) - 1
    pts = np.concatenate([rng.normal(size=(tcap, 3)), rng.uniform(0.2, 0.9, (tcap, 1))], 1).astype(np.float32)
    at = np.float32(np.cos(np.float64(np.float32(deg)) * (np.pi / 180.0)))
    pts[0] = [0, 0, 0, 2]
    pts[1, 0], pts[2, 1], pts[3, 2], pts[5, 3] = np.nan, np.inf, -np.inf, np.nan
    pts[6, 3], pts[7, 3], pts[8, 3] = at, np.nextafter(at, np.float32(2)), np.nextafter(at, np.float32(-2))
    pts[9, 3], pts[10, 3] = 1.0, np.nextafter(np.float32(1), np.float32(2))
    c.update(points=pts, deg=deg)
    return c


def ties():
    """single contributors whose v_k fall on .5: S = (5, 12) at scale 6.5 gives 2.5 -> 2, S = (3, 4) at scale 2.5 gives 1.5 -> 2"""
    q = np.full((2, 128), 128, np.uint8)
    q[0, 3], q[0, 90] = 128 + 5, 128 + 12
    q[1, 0], q[1, 127] = 128 + 3, 128 - 4
    return [call(q, [[0], [1]], scale=6.5), call(q, [[0], [1]], scale=2.5), call(q, [[0], [1]], scale=3.5)]


def many(seed=8, n_tracks=1500, n_rows=5000):
    """what a collection looks like, over more than one workgroup and more than one grid step of a wave: tracks of 2 .. 12
    observations, a few of them longer, states and points as triangulation leaves them, a tail up to the capacity"""
    rng = np.random.default_rng(seed)
    q = pool(rng, n_rows)
    tracks = [rng.integers(0, n_rows, int(n)).tolist() for n in rng.integers(2, 13, n_tracks)]
    for i in (7, 500, 1499):
        tracks[i] = rng.integers(0, n_rows, 300 + i).tolist()
    c = call(q, tracks, track_capacity=n_tracks + 77, obs_capacity=sum(len(t) for t in tracks) + 5)
    pts = np.concatenate([rng.normal(size=(n_tracks + 77, 3)), rng.uniform(0.2, 0.9, (n_tracks + 77, 1))], 1).astype(np.float32)
    pts[rng.random(n_tracks + 77) < 0.2] = [0, 0, 0, 2]
    c.update(obs_state=rng.integers(0, 3, len(c["obs_row"])).astype(np.uint32), min_state=2, points=pts)
    return c


def permuted(c_tracks, q, order, **kw):
    return call(q, [c_tracks[i] for i in order], **kw)


def cpu_cases():
    """(name, call) of everything the twin is held to numpy on"""
    out = [("lengths", lengths()), ("no stats", lengths(long=0, stats=False)), ("T = 0", no_tracks()),
           ("counts beyond", counts_beyond()), ("wild offsets", wild_offsets())]
    out += [("state %d" % m, states(m)) for m in (0, 1, 2)]
    out += [("points %g" % d, point_filter(d)) for d in (0.0, 5.0, 180.0)]
    out += [("scale %g" % s, lengths(6, long=0, scale=s)) for s in (0.0, 256.0, 100.0)]
    out += [("ties %d" % i, c) for i, c in enumerate(ties())]
    both = states(2, seed=7)
    both.update(points=point_filter(5.0, seed=7)["points"], deg=5.0)
    out.append(("states and points", both))
    out.append(("many", many()))
    return out


# ---- the twin -----------------------------------------------------------------------------------------------------

def build(out_dir, extra=("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")):
    """g++ -std=c++17 -O2 -ffp-contract=off of the twin, a stand-alone program, with the sanitizers; returns its path."""
    exe = os.path.join(str(out_dir), "track_desc_twin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-ffp-contract=off", *extra, "-I", CSRC,
                           os.path.join(TESTS, "cpp", "track_desc_twin.cpp"), "-o", exe])
    return exe


def arrays(c):
    """the call's arrays in the call's types"""
    st = None if c["obs_state"] is None else np.ascontiguousarray(c["obs_state"], np.uint32)
    pts = None if c["points"] is None else np.ascontiguousarray(c["points"], np.float32).reshape(-1, 4)
    return (np.ascontiguousarray(c["q"], np.uint8).reshape(-1, 128), np.ascontiguousarray(c["track_offsets"], np.uint64),
            np.ascontiguousarray(c["obs_row"], np.int32), np.ascontiguousarray(c["counts"], np.uint32), st, pts)


def _encode(c):
    q, off, row, counts, st, pts = arrays(c)
    assert st is None or len(st) == len(row)
    assert pts is None or len(pts) == len(off) - 1
    head = struct.pack("<QQQIIIIff", len(q), len(off) - 1, len(row), st is not None, c["min_state"], pts is not None,
                       bool(c["stats"]), np.float32(c["deg"]), np.float32(c["scale"]))
    return b"".join([head, counts.tobytes(), q.tobytes(), off.tobytes(), row.tobytes(), b"" if st is None else st.tobytes(),
                     b"" if pts is None else pts.tobytes()])


def run_calls(exe, tmp, calls):
    """every call in one run of the program -> [(desc uint8 [track_capacity, 128], stats int32 [track_capacity, 2] or None)]"""
    src, dst = os.path.join(str(tmp), "track_desc.in"), os.path.join(str(tmp), "track_desc.out")
    with open(src, "wb") as f:
        f.write(b"".join(_encode(c) for c in calls))
    done = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    with open(dst, "rb") as f:
        buf = f.read()
    out, at = [], 0
    for c in calls:
        tcap = len(c["track_offsets"]) - 1
        desc = np.frombuffer(buf, np.uint8, 128 * tcap, at).reshape(tcap, 128)
        at += 128 * tcap
        stats = None
        if c["stats"]:
            stats = np.frombuffer(buf, "<i4", 2 * tcap, at).reshape(tcap, 2)
            at += 8 * tcap
        out.append((desc, stats))
    assert at == len(buf), (at, len(buf))
    return out


# ---- the route: a model from four cameras of resect_cases.chain(), the fifth held out ---------------------------------

def route_scene(seed=11, held=4, sigma=0.05, n_clutter=150):
    """resect_cases.chain()'s five cameras with descriptors: every 3-D point gets a random unit descriptor, every observation
    that descriptor plus Gaussian noise of `sigma` a component, renormalised and quantised.  Camera `held` (the last) is held
    out: the model's table holds the tracks of at least two observations among the other four.  The query pool is the held-out
    image's rows followed by n_clutter unrelated rows (image 0), then n_clutter more unrelated rows alone (image 1).
    Returns a dict: pool_kps, pool_q (the four cameras' rows), image_offsets, table = (track_offsets, obs_row, obs_image,
    counts), K, truth; query_kps, query_q, query_offsets, true_row_track (the table index of a query row's own track, -1 for
    none), n_held."""
    import q8_cases
    import resect_cases
    kps, off, (ea, eb), matches, K, truth, _ = resect_cases.chain()
    assert held == 4, "the held-out camera's rows are the pool's last"
    n, rng = len(kps), np.random.default_rng(seed)
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, m in zip(ea, eb, matches):
        for i in np.flatnonzero(m >= 0):
            ra, rb = find(off[a] + i), find(off[b] + m[i])
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    root = np.array([find(i) for i in range(n)])
    ident = rng.normal(size=(n, 128))

    def rows_of(d):
        return q8_cases.quantize((d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32))

    q = rows_of(ident[root] / np.linalg.norm(ident[root], axis=1)[:, None] + sigma * rng.normal(size=(n, 128)))
    n_pool = int(off[held])
    tracks, index_of = [], {}
    for r in range(n_pool):
        if root[r] == r or root[r] not in index_of:
            members = np.flatnonzero(root[:n_pool] == root[r])
            if len(members) >= 2 and root[r] not in index_of:
                index_of[root[r]] = len(tracks)
                tracks.append(members.tolist())
    toff, obs_row, counts = table(tracks)
    obs_image = (np.searchsorted(off, obs_row, side="right") - 1).astype(np.uint32)
    held_rows = np.arange(off[held], off[held + 1])
    true_rt = np.array([index_of.get(root[r], -1) for r in held_rows] + [-1] * (2 * n_clutter), np.int32)
    clutter_kps = np.zeros((2 * n_clutter, 5), np.float32)
    clutter_kps[:, 0], clutter_kps[:, 1], clutter_kps[:, 2] = rng.uniform(0, 1280, 2 * n_clutter), rng.uniform(0, 960, 2 * n_clutter), 8.0
    return dict(pool_kps=kps[:n_pool], pool_q=q[:n_pool], image_offsets=off[:held + 1], table=(toff, obs_row, obs_image, counts),
                K=K, truth=truth, query_kps=np.concatenate([kps[held_rows], clutter_kps]),
                query_q=np.concatenate([q[held_rows], rows_of(rng.normal(size=(2 * n_clutter, 128)))]),
                query_offsets=np.array([0, len(held_rows) + n_clutter, len(held_rows) + 2 * n_clutter], np.int64),
                true_row_track=true_rt, n_held=len(held_rows))
