#!/usr/bin/env python3
"""Device time of lf_mkd_triangulate_tracks_device (per track its 3-D point, stats, errors, and per observation a state)
against the routes there were before it, on the same device tensors in one process:

    tri           the call with every output, enqueued directly
    tri_graph     the same call captured once in a graph and replayed
    tri_points    the call with d_err = d_obs_state = NULL
    torch         the route without the call, f64: rays and contributions per observation, repeat_interleave for the track
                  of every observation (its result has a dynamic size, so the route synchronises), index_add_ for the 3x3
                  systems, a batched torch.linalg.solve, the inlier test, and two trimming rounds that sum and solve again.
                  It has NO pair stage (torch has no per-track enumeration of pairs without padding every track to 8
                  candidates): it starts from the least squares over all observations, which on these outlier-free scenes
                  is where the call ends up too.  HIP events like the others
    host          the table, the keypoints and the cameras copied to the host, then the same route in numpy (np.add.at);
                  wall clock, 1 warm-up + 3 timed rounds

The device forms alternate call by call, each timed with HIP events -- 5 warm-up and 20 timed rounds; the median is reported,
and the 10th and 90th percentile as the run-to-run spread (bench_tracks.py's `timed`).  Before timing, the call's points must
agree with the torch route's within 1e-5 of their size wherever both have one, and both must have one for 99 % of the tracks.

Cases (noise 0.5 px, no outliers, cameras of tests/triangulate_cases.py): about 40 000 tracks of 2 .. 12 views over 64 images;
1.3 M tracks of length 2 over 1025 images; 256 images with window-4 tracks (2 .. 5 consecutive images, 30 000 tracks); ONE
track of 100 000 observations.  Prints one JSON line per case with the times in microseconds.
Development aid; bench.py is the contract for the headline metric."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("local-features_amd", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import local_features_python as lfp  # noqa: E402
import triangulate_cases as cases  # noqa: E402
from bench_tracks import TIMED, WARMUP, timed  # noqa: E402

HOST_WARMUP, HOST_TIMED = 1, 3
PX, ROUNDS = 4.0, 2


def scene(lengths, n_images, seed, stride_one=False, noise=0.5):
    """tests/triangulate_cases.scene vectorised: track i sees its point from lengths[i] images s, s + d, s + 2 d, ... (mod
    n_images; d odd, or 1), every observation a keypoint row of its own"""
    g = np.random.default_rng(seed)
    K, P = cases.cameras(n_images, g)
    lengths = np.asarray(lengths, np.int64)
    T, n_obs = len(lengths), int(lengths.sum())
    off = np.concatenate([[0], np.cumsum(lengths)])
    track = np.repeat(np.arange(T), lengths)
    j = np.arange(n_obs) - off[track]
    start, step = g.integers(0, n_images, T), np.ones(T, np.int64) if stride_one else 2 * g.integers(0, 8, T) + 1
    img = (start[track] + j * step[track]) % n_images
    X = np.stack([g.uniform(-3, 3, T), g.uniform(-2, 2, T), g.uniform(6, 14, T)], 1)
    R, t, k = P[img, :9].astype(np.float64).reshape(-1, 3, 3), P[img, 9:].astype(np.float64), K[img].astype(np.float64)
    p = np.einsum("nij,nj->ni", R, X[track]) + t
    kps = np.zeros((n_obs, 5), np.float32)
    row = g.permutation(n_obs).astype(np.int32)
    kps[row, 0] = k[:, 0] * p[:, 0] / p[:, 2] + k[:, 2] + g.normal(0, noise, n_obs)
    kps[row, 1] = k[:, 1] * p[:, 1] / p[:, 2] + k[:, 3] + g.normal(0, noise, n_obs)
    return {"kps": kps, "track_offsets": off.astype(np.uint64), "obs_row": row, "obs_image": img.astype(np.uint32),
            "counts": np.array([T, n_obs], np.uint32), "intrinsics": K, "poses": P}


class Device:
    def __init__(self, t):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.kps, self.intr, self.poses = up(t["kps"]), up(t["intrinsics"]), up(t["poses"])
        self.off, self.row, self.img = up(t["track_offsets"].view(np.int64)), up(t["obs_row"]), up(t["obs_image"].view(np.int32))
        self.counts = up(np.concatenate([t["counts"], t["counts"]]).view(np.int32))
        self.T, self.O = len(t["track_offsets"]) - 1, len(t["obs_row"])
        self.points = torch.empty((self.T, 4), dtype=torch.float32, device="cuda")
        self.err = torch.empty((self.T, 2), dtype=torch.float32, device="cuda")
        self.stats = torch.empty((self.T, 4), dtype=torch.int32, device="cuda")
        self.state = torch.empty((self.O,), dtype=torch.int32, device="cuda")


def call_tri(h, d, stream, extras=True):
    h.triangulate_tracks_device(d.kps.data_ptr(), d.kps.shape[0], d.off.data_ptr(), d.T, d.row.data_ptr(), d.img.data_ptr(), d.O,
                                d.counts.data_ptr(), d.intr.data_ptr(), d.poses.data_ptr(), d.intr.shape[0], d.points.data_ptr(),
                                d.stats.data_ptr(), d.err.data_ptr() if extras else None, d.state.data_ptr() if extras else None,
                                PX, ROUNDS, 0, stream)


def route(xp, kps, off, row, img, K, P, T):
    """the torch / numpy route (xp = torch or numpy; arrays of that library) -> points [T, 3] f64, has_point [T]"""
    is_t = xp is torch
    f64 = torch.float64 if is_t else np.float64
    cast = (lambda a: a.to(f64)) if is_t else (lambda a: a.astype(f64))
    idx = (lambda a: a.long()) if is_t else (lambda a: a.astype(np.int64))
    lengths = off[1:] - off[:-1]
    ar = torch.arange(T, device="cuda") if is_t else np.arange(T)
    track = torch.repeat_interleave(ar, lengths) if is_t else np.repeat(ar, lengths)     # (torch: synchronises)
    im = idx(img)
    k, p, xy = cast(K[im]), cast(P[im]), cast(kps[idx(row)][:, :2])
    R, t = p[:, :9].reshape(-1, 3, 3), p[:, 9:]
    xn = xp.stack([(xy[:, 0] - k[:, 2]) / k[:, 0], (xy[:, 1] - k[:, 3]) / k[:, 1], xp.ones_like(xy[:, 0])], 1)
    d = (xn[:, :, None] * R).sum(1)                                  # R^T xn
    u = d / xp.sqrt((d * d).sum(1))[:, None]
    c = -(t[:, :, None] * R).sum(1)
    eye = torch.eye(3, dtype=f64, device="cuda") if is_t else np.eye(3)
    A = eye[None] - u[:, :, None] * u[:, None, :]
    b = c - u * (u * c).sum(1)[:, None]

    def solve(mask):
        w = cast(mask)
        if is_t:
            As = torch.zeros((T, 3, 3), dtype=f64, device="cuda").index_add_(0, track, A * w[:, None, None])
            bs = torch.zeros((T, 3), dtype=f64, device="cuda").index_add_(0, track, b * w[:, None])
            n = torch.zeros(T, dtype=f64, device="cuda").index_add_(0, track, w)
            ok = n >= 2
            As = torch.where(ok[:, None, None], As, eye[None])
            return torch.linalg.solve(As, bs), ok
        As, bs, n = np.zeros((T, 3, 3)), np.zeros((T, 3)), np.zeros(T)
        np.add.at(As, track, A * w[:, None, None])
        np.add.at(bs, track, b * w[:, None])
        np.add.at(n, track, w)
        ok = n >= 2
        As[~ok] = eye
        return np.linalg.solve(As, bs[:, :, None])[:, :, 0], ok

    def inliers(X):
        q = (R * X[track][:, None, :]).sum(2) + t
        ex = k[:, 0] * (q[:, 0] / q[:, 2]) + k[:, 2] - xy[:, 0]
        ey = k[:, 1] * (q[:, 1] / q[:, 2]) + k[:, 3] - xy[:, 1]
        return (q[:, 2] > 0) & (ex * ex + ey * ey <= PX * PX)

    X, ok = solve(xp.ones_like(xy[:, 0]) > 0)
    for _ in range(ROUNDS):
        X, ok = solve(inliers(X))
    return X, ok


def time_case(h, t, stream):
    d = Device(t)
    call_tri(h, d, stream)
    torch.cuda.synchronize()
    X, ok = route(torch, d.kps, d.off, d.row, d.img, d.intr, d.poses, d.T)
    st = d.stats.cpu().numpy()
    both = torch.from_numpy(st[:, 2] == 0).cuda() & ok
    assert int(both.sum()) >= 0.99 * d.T, "fewer than 99 % of the tracks have a point on both routes"
    scale = X[both].abs().max(1).values.clamp(min=1.0)
    dev = float(((d.points[both, :3].double() - X[both]).abs().max(1).values / scale).max())
    assert dev < 1e-5, "the points differ: %g" % dev
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call_tri(h, d, torch.cuda.current_stream().cuda_stream)
    r = timed({"tri": lambda: call_tri(h, d, stream), "tri_graph": g.replay, "tri_points": lambda: call_tri(h, d, stream, False),
               "torch": lambda: route(torch, d.kps, d.off, d.row, d.img, d.intr, d.poses, d.T)})
    host = []
    for it in range(HOST_WARMUP + HOST_TIMED):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        route(np, d.kps.cpu().numpy(), d.off.cpu().numpy(), d.row.cpu().numpy(), d.img.cpu().numpy(), d.intr.cpu().numpy(),
              d.poses.cpu().numpy(), d.T)
        if it >= HOST_WARMUP:
            host.append((time.perf_counter() - t0) * 1e6)
    med = lambda k: r[k]["median_us"]
    cos = d.points[:, 3].cpu().numpy()[st[:, 2] == 0]
    return {"tracks": d.T, "observations": d.O, "images": int(d.intr.shape[0]), "points": int((st[:, 2] == 0).sum()),
            "inliers": int(st[:, 1].sum()), "median_parallax_deg": round(float(np.degrees(np.arccos(np.clip(np.median(cos), -1, 1)))), 2),
            "largest_deviation_from_torch": dev, **{k + "_" + f: v[f] for k, v in r.items() for f in v},
            "host_wall_median_us": round(statistics.median(host), 1), "torch_over_tri": round(med("torch") / med("tri_graph"), 2),
            "host_over_tri": round(statistics.median(host) / med("tri_graph"), 1), "warmup": WARMUP, "timed": TIMED,
            "lib": os.path.basename(lfp.LIB_PATH)}


def make_case(k):
    g = np.random.default_rng(0)
    if k == 0:
        return "40k_tracks_2_to_12_views_64_images", scene(g.integers(2, 13, 40000), 64, 1)
    if k == 1:
        return "1300k_tracks_of_2_1025_images", scene(np.full(1300000, 2), 1025, 2, stride_one=True)
    if k == 2:
        return "window4_256_images", scene(g.integers(2, 6, 30000), 256, 3, stride_one=True)
    return "one_track_100k_observations", scene(np.array([100000]), 64, 4)


def main():
    torch.cuda.init()
    torch.cuda.set_stream(torch.cuda.Stream())
    s = torch.cuda.current_stream().cuda_stream
    h = lfp.MkdHandle(max_features=64)
    only = [int(a) for a in sys.argv[1:] if a.isdigit()] or range(4)
    for k in only:
        name, t = make_case(k)
        print(json.dumps({"bench": "triangulate", "case": name, **time_case(h, t, s)}), flush=True)


if __name__ == "__main__":
    main()
