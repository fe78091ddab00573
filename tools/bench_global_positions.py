#!/usr/bin/env python3
"""Device time of lf_mkd_tree_poses_device and lf_mkd_global_positions_device (camera centres and track points at once under
held rotations) against the routes there are beside them, on the same device tensors in one process:

    tree          lf_mkd_tree_poses_device on ONE chain through the case's images (256 of them at most: the deepest tree there
                  is), replayed from a graph
    graph_S       lf_mkd_global_positions_device at S = 10, 50 and 200 sweeps without a trace, the warmed-up call captured
                  once in a hipGraph and replayed; per_sweep_us = (graph_200 - graph_50) / 150
    call_50       the same call's plain launches at 50 sweeps (4 + 3 x 50 of them)
    trace_50      the graph at 50 sweeps WITH d_trace: the cost pass is one workgroup over every observation
    torch_50      the same algorithm in torch float64 tensor operations (index_add_ into the 3x3 systems, batched
                  torch.linalg.solve, the gauge as tensor reductions; no HELD rules, no singularity test), HIP events
    twin_10       the host twin (tests/cpp/positions_twin.cpp, the kernels' own math header under g++ -O2) on one host core at
                  10 sweeps: wall clock of the program on a call file (file I/O included), scaled by nothing
    register      what the global route replaces, on the same tables through the LocalFeatures wrappers: two images at their true
                  poses, triangulate_tracks, then ROUNDS times (resect_cameras in place, triangulate_tracks), ROUNDS = the rounds
                  that loop needs until it registers no further image (found before timing); beside it `global_route` =
                  global_positions at 50 sweeps in place + triangulate_tracks (the tree call is timed apart)

The query case times the graphs at 10 and 50 sweeps and the twin alone (its trace, torch and register forms take minutes).
`--trace K` makes 3 plain calls of case K at 50 sweeps and exits: for `rocprofv3 --kernel-trace --stats` (the kernels' shares).

The device forms alternate call by call, each timed with HIP events -- 5 warm-up and 20 timed rounds; the median is reported,
and the 10th and 90th percentile as the run-to-run spread (bench_tracks.py's `timed`).  Before timing, every output word of the
call at 10 sweeps must equal the twin's.

Cases: synthetic pinhole scenes, 0.5 px noise, 10 % wrong rays, unit-step chain poses as input: 64 images of about 2000 rows
(18 000 tracks of 2 .. 12 views), 256 frames with tracks along a window of 4, one query image against 1024 (a track per
query row: ONE image owns half the rows).  Prints one JSON line per case with the times in microseconds.
Development aid; bench.py is the contract for the headline metric."""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("local-features_amd", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import local_features_python as lfp  # noqa: E402
import positions_cases as cases  # noqa: E402
import positions_twin as pt  # noqa: E402
from bench_tracks import TIMED, WARMUP, timed  # noqa: E402

WARM, DEG, MIN_OBS = 3, 0.2, 2


def scene(centres, targets, X, visible, seed):
    """positions_cases.build, vectorised for large tables: the same layout without the extra rows.  visible: bool [T, n], or
    the pair (track, image) of every observation in table order"""
    g = np.random.default_rng(seed)
    t_idx, i_idx = visible if isinstance(visible, tuple) else np.nonzero(visible)
    R = np.stack([cases.look_at(c, t) for c, t in zip(centres, targets)])
    p = np.einsum("nij,nj->ni", R[i_idx], X[t_idx] - centres[i_idx])
    xy = np.stack([cases.K0[0] * p[:, 0] / p[:, 2] + cases.K0[2], cases.K0[1] * p[:, 1] / p[:, 2] + cases.K0[3]], 1)
    xy += 0.5 * g.standard_normal(xy.shape)
    wrong = g.random(len(xy)) < 0.10
    xy[wrong] = g.uniform(0, 1, (int(wrong.sum()), 2)) * np.array([1024.0, 768.0])
    n, T, O = len(centres), len(X), len(t_idx)
    order = np.argsort(i_idx, kind="stable")                       # the pool: image by image, in track order
    row_of = np.empty(O, np.int64)
    row_of[order] = np.arange(O)
    kps = np.zeros((O, 5), np.float32)
    kps[row_of, :2], kps[:, 2] = xy, 3.0
    row_track = np.empty(O, np.int32)
    row_track[row_of] = t_idx
    ioff = np.concatenate([[0], np.cumsum(np.bincount(i_idx, minlength=n))]).astype(np.uint64)
    toff = np.concatenate([[0], np.cumsum(np.bincount(t_idx, minlength=T))]).astype(np.uint64)
    start = cases.unit_step_centres(np.asarray(centres, np.float64))
    poses = np.concatenate([R.reshape(n, 9), -np.einsum("nij,nj->ni", R, start)], 1).astype(np.float32)
    truth_poses = np.concatenate([R.reshape(n, 9), -np.einsum("nij,nj->ni", R, np.asarray(centres, np.float64))], 1).astype(np.float32)
    return dict(kps=kps, image_offsets=ioff, track_offsets=toff, obs_row=row_of.astype(np.int32), obs_image=i_idx.astype(np.uint32),
                counts=np.array([T, O], np.uint32), row_track=row_track, intrinsics=np.tile(cases.K0, (n, 1)), poses=poses,
                truth=dict(centres=np.asarray(centres, np.float64), poses=truth_poses))


def make_case(k):
    g = np.random.default_rng(k)
    if k == 0:
        n, T = 64, 18000
        ang = np.linspace(0, 2 * np.pi, n, endpoint=False)
        centres = np.stack([6 * np.cos(ang), 0.5 * g.standard_normal(n), 6 * np.sin(ang)], 1)
        X = 1.5 * g.standard_normal((T, 3)) / 1.5
        visible = np.zeros((T, n), bool)
        for t, m in enumerate(g.integers(2, 13, T)):
            visible[t, g.choice(n, m, replace=False)] = True
        visible[:, 0] &= g.random(T) < 0.5
        return "images_64", scene(centres, np.zeros((n, 3)), X, visible, 1)
    if k == 1:
        n, per = 256, 400
        centres = np.stack([0.5 * np.arange(n), 0.05 * g.standard_normal(n), 0.05 * g.standard_normal(n)], 1)
        T = n * per
        first = np.repeat(np.arange(n), per)
        X = np.stack([0.5 * first + g.uniform(0, 1.5, T), g.uniform(-2, 2, T), g.uniform(5, 9, T)], 1)
        visible = np.zeros((T, n), bool)
        for d in range(5):
            ok = (first + d < n) & ((d < 2) | (g.random(T) < 0.6))
            visible[np.flatnonzero(ok), (first + d)[ok]] = True
        keep = visible.sum(1) >= 2
        return "window4_256", scene(centres, centres + np.array([0, 0, 6.0]), X[keep], visible[keep], 2)
    n, per = 1025, 1280
    ang = np.linspace(0, 2 * np.pi, n - 1, endpoint=False)
    centres = np.concatenate([[[0.0, 0.0, -8.0]], np.stack([7 * np.cos(ang), g.uniform(-1, 1, n - 1), 7 * np.sin(ang)], 1)])
    T = (n - 1) * per
    X = g.standard_normal((T, 3))
    t_idx = np.repeat(np.arange(T), 2)
    i_idx = np.stack([np.zeros(T, np.int64), 1 + np.arange(T) // per], 1).reshape(-1)
    return "query_1024", scene(centres, np.zeros((n, 3)), X, (t_idx, i_idx), 3)


class Device:
    def __init__(self, s, sweeps):
        kps, ioff, toff, row, img, tc, rt, K, P = pt.arrays(s)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.kps, self.ioff, self.toff = up(kps), up(ioff.view(np.int64)), up(toff.view(np.int64))
        self.row, self.img, self.tc, self.rt = up(row), up(img.view(np.int32)), up(tc.view(np.int32)), up(rt)
        self.K, self.P = up(K), up(P)
        self.n, self.n_rows, self.tcap, self.ocap = len(K), len(kps), len(toff) - 1, len(row)
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda")
        self.out, self.points = torch.empty((self.n, 12), dtype=torch.float32, device="cuda"), torch.empty((self.tcap, 4), dtype=torch.float32, device="cuda")
        self.state, self.ims, self.counts = i32(self.ocap), i32(self.n, 4), i32(8)
        self.trace = torch.zeros((max(sweeps), 4), dtype=torch.float64, device="cuda")


def call(h, d, sweeps, stream, trace=False):
    h.global_positions_device(d.kps.data_ptr(), d.ioff.data_ptr(), d.n, d.n_rows, d.toff.data_ptr(), d.tcap, d.row.data_ptr(),
                              d.img.data_ptr(), d.ocap, d.tc.data_ptr(), d.rt.data_ptr(), d.K.data_ptr(), d.P.data_ptr(),
                              d.out.data_ptr(), d.ims.data_ptr(), d.counts.data_ptr(), d.points.data_ptr(), d.state.data_ptr(),
                              d.trace.data_ptr() if trace else None, sweeps, WARM, DEG, MIN_OBS, 0, stream)


def torch_route(d, sweeps):
    """the same sweeps in torch float64 tensor operations; returns the centres"""
    f64 = torch.float64
    K, P = d.K.to(f64), d.P.to(f64)
    R = P[:, :9].reshape(-1, 3, 3)
    cen = -torch.einsum("nji,nj->ni", R, P[:, 9:])
    img, row = d.img.long(), d.row.long()
    track = d.rt.long()[row]
    f = torch.stack([(d.kps[row, 0].to(f64) - K[img, 2]) / K[img, 0], (d.kps[row, 1].to(f64) - K[img, 3]) / K[img, 1],
                     torch.ones(len(row), dtype=f64, device="cuda")], 1)
    v = torch.nn.functional.normalize(torch.einsum("nji,nj->ni", R[img], f), dim=1)
    Pm = torch.eye(3, dtype=f64, device="cuda")[None] - v[:, :, None] * v[:, None, :]
    s0 = float(np.sin(np.radians(DEG)))
    pts = torch.zeros((d.tcap, 3), dtype=f64, device="cuda")

    def solve(idx, m, w, y):
        A = torch.zeros((m, 3, 3), dtype=f64, device="cuda").index_add_(0, idx, w[:, None, None] * Pm)
        b = torch.zeros((m, 3), dtype=f64, device="cuda").index_add_(0, idx, w[:, None] * torch.einsum("nij,nj->ni", Pm, y))
        return torch.linalg.solve(A + 1e-12 * torch.eye(3, dtype=f64, device="cuda"), b)

    def weights(robust):
        if not robust:
            return torch.ones(len(row), dtype=f64, device="cuda")
        r = pts[track] - cen[img]
        depth = (v * r).sum(1)
        s = torch.sqrt(((r - v * depth[:, None]) ** 2).sum(1) / (r * r).sum(1))
        return torch.where(depth > 0, s0 / torch.clamp(s, min=s0), torch.zeros_like(s))

    def gauge():
        nonlocal cen, pts
        m = cen.mean(0)
        rho = torch.sqrt(((cen - m) ** 2).sum(1).mean())
        cen, pts = (cen - m) / rho, (pts - m) / rho
    gauge()
    for s in range(sweeps):
        pts = solve(track, d.tcap, weights(s >= WARM and s > 0), cen[img])
        cen = solve(img, d.n, weights(s >= WARM), pts[track])
        gauge()
    return cen


def time_register(lf, s, d):
    """the incremental loop against the global route on the case's tables: (forms to time, rounds, images registered)"""
    table = (d.toff, d.row, d.img, d.tc)
    start = torch.zeros((d.n, 12), dtype=torch.float32, device="cuda")
    start[:2] = torch.from_numpy(s["truth"]["poses"][:2]).cuda()
    poses = start.clone()

    def loop(rounds):
        poses.copy_(start)
        points = lf.triangulate_tracks(d.kps, table, d.K, poses)[0]
        for _ in range(rounds):
            lf.resect_cameras(d.kps, d.ioff, d.rt, points, d.tc, d.K, poses, out=poses)
            points = lf.triangulate_tracks(d.kps, table, d.K, poses)[0]
    rounds, registered = 0, 2
    while rounds < 96:                                              # (read back between rounds here, before timing, only)
        loop(rounds + 1)
        now = int((poses[:, :9] != 0).any(1).sum())
        if now == registered:
            break
        rounds, registered = rounds + 1, now
    gp = d.P.clone()

    def global_route():
        gp.copy_(d.P)
        lf.global_positions(d.kps, d.ioff, (d.toff, d.row, d.img, d.rt, d.tc), d.K, gp, sweeps=50, warm=WARM, robust_deg=DEG,
                            min_obs=MIN_OBS, out_poses=gp, points=False, obs_state=False)
        lf.triangulate_tracks(d.kps, table, d.K, gp)
    return {"register": lambda: loop(rounds), "global_route": global_route}, rounds, registered


def time_case(h, s, stream, exe, tmp, light=False, lf=None):
    sweeps = (10, 50) if light else (10, 50, 200)
    d = Device(s, sweeps)
    call(h, d, max(sweeps), stream)                                # warm: the scratch grows once
    call(h, d, 10, stream, trace=not light)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = pt.run(exe, tmp, s, sweeps=10, warm=WARM, robust_deg=DEG, min_obs=MIN_OBS)
    twin_us = (time.perf_counter() - t0) * 1e6
    got = dict(poses=d.out, points=d.points, obs_state=d.state, image_stats=d.ims, counts=d.counts)
    if not light:
        got["trace"] = d.trace[:10]
    for k, t in got.items():
        a, b = t.cpu().numpy().reshape(-1).view(np.uint32), np.ascontiguousarray(want[k]).reshape(-1).view(np.uint32)
        assert np.array_equal(a, b), "the call and the twin differ in " + k
    forms = {}
    graphs = []
    for S, trace in [(S, False) for S in sweeps] + ([] if light else [(50, True)]):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call(h, d, S, torch.cuda.current_stream().cuda_stream, trace=trace)
        graphs.append(g)
        forms[("trace_%d" if trace else "graph_%d") % S] = g.replay
    forms["call_50"] = lambda: call(h, d, 50, stream)
    extra = {}
    if not light:
        forms["torch_50"] = lambda: torch_route(d, 50)
        more, rounds, registered = time_register(lf, s, d)
        forms.update(more)
        extra = {"register_rounds": rounds, "register_images": registered}
    torch.cuda.synchronize()
    r = timed(forms)
    call(h, d, 50, stream)
    torch.cuda.synchronize()
    ours = cases.centres_of(d.out.cpu().numpy())
    med = lambda k: r[k]["median_us"]
    if not light:
        theirs = torch_route(d, 50).cpu().numpy()
        extra.update(torch_centre_error_50=round(cases.similarity_error(theirs, s["truth"]["centres"]), 6),
                     torch_over_graph_50=round(med("torch_50") / med("graph_50"), 1),
                     register_over_global_route=round(med("register") / med("global_route"), 2))
    launches, scratch = lfp.global_positions_plan(d.n, d.tcap, 50)
    lo, hi = (10, 50) if light else (50, 200)
    return {"images": d.n, "rows": d.n_rows, "tracks": d.tcap, "observations": d.ocap, "launches_50": launches, "scratch_bytes": scratch,
            "centre_error_50": round(cases.similarity_error(ours, s["truth"]["centres"]), 6), **extra,
            **{k + "_" + f: v[f] for k, v in r.items() for f in v},
            "per_sweep_us": round((med("graph_%d" % hi) - med("graph_%d" % lo)) / (hi - lo), 2), "twin_10_wall_us": round(twin_us, 1),
            "call_over_graph_50": round(med("call_50") / med("graph_50"), 2),
            "twin_over_graph_10": round(twin_us / med("graph_10"), 1), "warmup": WARMUP, "timed": TIMED, "lib": os.path.basename(lfp.LIB_PATH)}


def time_tree(h, n, stream):
    """a chain of n images, every tree edge stored as (parent, child): depth n - 1 for the last one"""
    s = cases.tree_scene(seed=5, n=n, flip=())
    ea, eb, t, rot, st = pt.tree_arrays(s)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = [up(ea.view(np.int32)), up(eb.view(np.int32)), up(t), up(rot), up(st.view(np.int32))]
    out = torch.empty((n, 12), dtype=torch.float32, device="cuda")
    run = lambda sm: h.tree_poses_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), len(ea), d[3].data_ptr(), d[4].data_ptr(), n,
                                         out.data_ptr(), 4096, sm)
    run(stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return timed({"tree": g.replay})["tree"]


def main():
    torch.cuda.init()
    torch.cuda.set_stream(torch.cuda.Stream())
    s = torch.cuda.current_stream().cuda_stream
    h = lfp.MkdHandle(max_features=64)
    only = [int(a) for a in sys.argv[1:] if a.isdigit()] or range(3)
    if "--trace" in sys.argv[1:]:
        name, sc = make_case(list(only)[0])
        d = Device(sc, (50,))
        for _ in range(3):
            call(h, d, 50, s)
        torch.cuda.synchronize()
        return
    lf = lfp.LocalFeatures(64, 64, 16)
    with tempfile.TemporaryDirectory() as tmp:
        exe = pt.build(tmp)
        for k in only:
            name, sc = make_case(k)
            tree = time_tree(h, min(len(sc["intrinsics"]), 256), s)
            print(json.dumps({"bench": "global_positions", "case": name, **{"tree_chain_" + f: v for f, v in tree.items()},
                              **time_case(h, sc, s, exe, tmp, light=k == 2, lf=lf)}), flush=True)


if __name__ == "__main__":
    main()
