#!/usr/bin/env python3
"""Device time of lf_mkd_bundle_adjust_device at 10 iterations x 10 CG steps.  The parent of this call had no route at all, so
the comparison is with two other routes on the same arrays, each named as what it is:

    bundle          the call with every output, enqueued directly (5 + 10 x (6 + 5 x 10) = 565 launches)
    bundle_graph    the same call captured once in a graph and replayed
    bundle_1cg      the replayed call at 10 iterations x 1 CG step: (bundle_graph - bundle_1cg) / 90 is the time of a CG step
    twin            tests/cpp/bundle_twin.cpp (the kernels' math header under g++ -O2, one host core), the whole program run on
                    the call's arrays written to a file: wall clock of the process, file reading included, one round
    torch_f64       the same algorithm (the same damping, HELD masks, PCG and stopping rules) written with torch float64
                    tensor operations on the device -- index_add_ for the sums, batched inverses for the blocks -- with the
                    host deciding every branch (a read-back per CG step): wall clock of one call after one warm-up call

The device forms alternate call by call, each timed with HIP events -- 5 warm-up and 20 timed rounds; the median is reported,
and the 10th and 90th percentile as the run-to-run spread (bench_tracks.py's `timed`).  Before timing, the call's words must
equal the twin's (the twin is skipped, and so is that check, above TWIN_MAX_OBS observations).  The LARGEST case is warmed
first and every graph is captured after it: a call that needs more scratch than the handle holds replaces it, and a graph
captured before that names the scratch that was freed.

Cases (0.5 px noise, 5 % wrong observations, perturbed poses and points, tracks of 4 views): 64 images of about 2000 rows, the
views drawn over all images; a window of 256 frames of about 1000 rows, the views in consecutive frames; one free query image
of 2000 rows against 1024 fixed ones; ONE image owning 500 000 rows.  Prints one JSON line per case with the times in
microseconds.  `--trace CASE` makes 3 plain calls for rocprofv3 --kernel-trace --stats.
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
import bundle_cases as cases  # noqa: E402
import bundle_twin as twin  # noqa: E402
from bench_tracks import TIMED, WARMUP, timed  # noqa: E402

PARAMS = dict(px=4.0, lambda0=1e-3, iterations=10, cg_iterations=10, cg_tol=0.0)
TWIN_MAX_OBS = 300000


def scene(seed, n_images, n_tracks, views, mode, n_fixed=2):
    """a vectorised tests/bundle_cases.py build(): `views` views per track, drawn over all images ("all"), in consecutive
    images ("window"), or image n_images - 1 and views - 1 others ("query")"""
    g = np.random.default_rng(seed)
    N, T, v = n_images, n_tracks, min(views, n_images)
    ang = 2 * np.pi * np.arange(N) / N
    centres = np.stack([6 * np.cos(ang), 0.8 * g.standard_normal(N), 6 * np.sin(ang)], 1)
    poses = np.array([np.concatenate([R.reshape(9), t]) for R, t in (cases.look_at(c) for c in centres)])
    X = g.standard_normal((T, 3))
    X = 1.5 * X / np.maximum(1.0, np.linalg.norm(X, axis=1, keepdims=True))
    if mode == "window":
        img = (g.integers(0, N, T)[:, None] + np.arange(v)[None, :]) % N
    elif mode == "query":
        img = np.concatenate([np.argsort(g.random((T, N - 1)), 1)[:, :v - 1], np.full((T, 1), N - 1)], 1)
    else:
        img = np.argsort(g.random((T, N)), 1)[:, :v]
    img = np.sort(img, 1)
    ot, oi = np.repeat(np.arange(T), v), img.reshape(-1)
    p = np.einsum("nij,nj->ni", poses[oi, :9].reshape(-1, 3, 3), X[ot]) + poses[oi, 9:]
    xy = cases.K0[None, :2] * p[:, :2] / p[:, 2:3] + cases.K0[None, 2:] + 0.5 * g.standard_normal((len(ot), 2))
    wrong = g.random(len(ot)) < 0.05
    a = g.uniform(0, 2 * np.pi, wrong.sum())
    xy[wrong] += g.uniform(15, 60, wrong.sum())[:, None] * np.stack([np.cos(a), np.sin(a)], 1)
    order = np.argsort(oi, kind="stable")                      # the pool: image by image, in track order
    row = np.empty(len(ot), np.int64)
    row[order] = np.arange(len(ot))
    kps = np.zeros((len(ot), 5), np.float32)
    kps[row, :2], kps[:, 2] = xy, 3.0
    start = poses.copy()
    for i in range(min(n_fixed, N), N) if mode != "query" else [N - 1]:
        start[i, :9] = (cases.cayley(0.004 * g.standard_normal(3)) @ poses[i, :9].reshape(3, 3)).reshape(9)
        start[i, 9:] += 0.02 * g.standard_normal(3)
    points = np.concatenate([X + 0.02 * g.standard_normal((T, 3)), np.full((T, 1), 0.9)], 1).astype(np.float32)
    fixed = np.zeros(N, np.uint32)
    if mode == "query":
        fixed[:N - 1] = 1
    elif N > n_fixed:
        fixed[:n_fixed] = 1
    return dict(kps=kps, image_offsets=np.concatenate([[0], np.cumsum(np.bincount(oi, minlength=N))]).astype(np.uint64),
                track_offsets=(np.arange(T + 1) * v).astype(np.uint64), obs_row=row.astype(np.int32), obs_image=oi.astype(np.uint32),
                counts=np.array([T, len(ot)], np.uint32), points=points, intrinsics=np.tile(cases.K0, (N, 1)),
                poses=start.astype(np.float32), obs_state=None, camera_fixed=fixed)


def make_case(k):
    if k == 0:
        return "64_images_2000_rows", scene(1, 64, 32000, 4, "all")
    if k == 1:
        return "window_256_frames_1000_rows", scene(2, 256, 64000, 4, "window")
    if k == 2:
        return "one_query_against_1024", scene(3, 1025, 2000, 4, "query")
    return "one_image_500k_rows", scene(4, 1, 500000, 1, "all", n_fixed=0)


class Device:
    def __init__(self, s):
        a = twin.arrays(s)
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        self.kps, self.ioff, self.toff = up(a["kps"]), up(a["image_offsets"].view(np.int64)), up(a["track_offsets"].view(np.int64))
        self.row, self.img, self.tc = up(a["obs_row"]), up(a["obs_image"].view(np.int32)), up(a["counts"].view(np.int32))
        self.pts, self.K, self.poses, self.fixed = up(a["points"]), up(a["intrinsics"]), up(a["poses"]), up(a["camera_fixed"].view(np.int32))
        self.n, self.rows, self.tcap, self.ocap = len(a["intrinsics"]), len(a["kps"]), len(a["points"]), len(a["obs_row"])
        self.out, self.pout = torch.empty_like(self.poses), torch.empty_like(self.pts)
        self.state = torch.empty((self.ocap,), dtype=torch.int32, device="cuda")
        self.trace = torch.zeros((64, 8), dtype=torch.float64, device="cuda")
        self.counts = torch.zeros((4,), dtype=torch.int32, device="cuda")


def call(h, d, stream, cg_iterations=PARAMS["cg_iterations"]):
    h.bundle_adjust_device(d.kps.data_ptr(), d.ioff.data_ptr(), d.n, d.rows, d.toff.data_ptr(), d.tcap, d.row.data_ptr(),
                           d.img.data_ptr(), d.ocap, d.tc.data_ptr(), d.pts.data_ptr(), d.K.data_ptr(), d.poses.data_ptr(),
                           d.out.data_ptr(), d.pout.data_ptr(), d.trace.data_ptr(), d.counts.data_ptr(), d_camera_fixed=d.fixed.data_ptr(),
                           d_obs_state_out=d.state.data_ptr(), max_reproj_px=PARAMS["px"], lambda0=PARAMS["lambda0"],
                           iterations=PARAMS["iterations"], cg_iterations=cg_iterations, cg_tol=PARAMS["cg_tol"], stream=stream)


def torch_route(d, px, lambda0, iterations, cg_iterations, cg_tol):
    """the algorithm of include/lf_mkd.h in torch float64 on the device (every observation of a bench scene is active)"""
    f64, dev = torch.float64, d.kps.device
    oi, ot = d.img.long(), torch.repeat_interleave(torch.arange(d.tcap, device=dev), (d.toff[1:] - d.toff[:-1]))
    xy, K = d.kps[d.row.long(), :2].to(f64), d.K.to(f64)
    R, tr, X = d.poses[:, :9].reshape(-1, 3, 3).to(f64), d.poses[:, 9:].to(f64), d.pts[:, :3].to(f64)
    N, T, thr2, tol2, lam = d.n, d.tcap, float(np.float32(px)) ** 2, float(np.float32(cg_tol)) ** 2, float(np.float32(lambda0))
    cam_free = d.fixed == 0
    eye6, eye3 = torch.eye(6, dtype=f64, device=dev), torch.eye(3, dtype=f64, device=dev)

    def project(R, tr, X):
        q = torch.einsum("nij,nj->ni", R[oi], X[ot])
        p = q + tr[oi]
        u = p[:, :2] / p[:, 2:3]
        e = K[oi, :2] * u + K[oi, 2:] - xy
        return q, p, u, e, (e * e).sum(1)

    def cost_of(R, tr, X):
        _, p, _, _, e2 = project(R, tr, X)
        inl = (p[:, 2] > 0) & (e2 <= thr2)
        return torch.where(inl, e2, torch.full_like(e2, thr2)).sum(), inl

    for _ in range(iterations):
        q, p, u, e, e2 = project(R, tr, X)
        cost_k, inl = cost_of(R, tr, X)
        a, b = K[oi, 0] / p[:, 2], K[oi, 1] / p[:, 2]
        gx, gy, z = -a * u[:, 0], -b * u[:, 1], torch.zeros_like(a)
        Jx = torch.stack([2 * gx * q[:, 1], 2 * (a * q[:, 2] - gx * q[:, 0]), -2 * a * q[:, 1], a, z, gx], 1)
        Jy = torch.stack([2 * (gy * q[:, 1] - b * q[:, 2]), -2 * gy * q[:, 0], 2 * b * q[:, 0], z, b, gy], 1)
        Rr = R[oi]
        Px, Py = a[:, None] * Rr[:, 0] + gx[:, None] * Rr[:, 2], b[:, None] * Rr[:, 1] + gy[:, None] * Rr[:, 2]
        m = inl.to(f64)[:, None]
        Jx, Jy, Px, Py = torch.nan_to_num(Jx * m), torch.nan_to_num(Jy * m), torch.nan_to_num(Px * m), torch.nan_to_num(Py * m)
        W = Jx[:, :, None] * Px[:, None, :] + Jy[:, :, None] * Py[:, None, :]
        U = torch.zeros((N, 6, 6), dtype=f64, device=dev).index_add_(0, oi, Jx[:, :, None] * Jx[:, None, :] + Jy[:, :, None] * Jy[:, None, :])
        V = torch.zeros((T, 3, 3), dtype=f64, device=dev).index_add_(0, ot, Px[:, :, None] * Px[:, None, :] + Py[:, :, None] * Py[:, None, :])
        en = torch.nan_to_num(e * m)
        gc = torch.zeros((N, 6), dtype=f64, device=dev).index_add_(0, oi, Jx * en[:, :1] + Jy * en[:, 1:])
        gp = torch.zeros((T, 3), dtype=f64, device=dev).index_add_(0, ot, Px * en[:, :1] + Py * en[:, 1:])
        n_in = torch.zeros(T, dtype=f64, device=dev).index_add_(0, ot, m[:, 0])
        U = U + lam * torch.diag_embed(torch.clamp(torch.diagonal(U, dim1=1, dim2=2), min=1e-6))
        V = V + lam * torch.diag_embed(torch.clamp(torch.diagonal(V, dim1=1, dim2=2), min=1e-6))
        cam_moves = cam_free & (torch.linalg.cholesky_ex(U).info == 0)
        pt_moves = (n_in >= 2) & (torch.linalg.det(V) > 1e-12 * (torch.diagonal(V, dim1=1, dim2=2).sum(1) / 3) ** 3)
        Uinv = torch.linalg.inv(torch.where(cam_moves[:, None, None], U, eye6)) * cam_moves[:, None, None]
        Vinv = torch.linalg.inv(torch.where(pt_moves[:, None, None], V, eye3)) * pt_moves[:, None, None]
        W = W * (cam_moves[oi] & pt_moves[ot]).to(f64)[:, None, None]
        wt = lambda vv: torch.zeros((T, 3), dtype=f64, device=dev).index_add_(0, ot, torch.einsum("nij,ni->nj", W, vv[oi]))
        w = lambda yy: torch.zeros((N, 6), dtype=f64, device=dev).index_add_(0, oi, torch.einsum("nij,nj->ni", W, yy[ot]))
        solve_v, solve_u = (lambda b_: torch.einsum("nij,nj->ni", Vinv, b_)), (lambda b_: torch.einsum("nij,nj->ni", Uinv, b_))
        mask = cam_moves[:, None].to(f64)
        r = (gc - w(solve_v(gp))) * mask
        x, zz = torch.zeros_like(r), solve_u(r)
        pp = zz.clone()
        rz = rz0 = float((r * zz).sum())
        for _ in range(cg_iterations):
            Ap = (torch.einsum("nij,nj->ni", U, pp) - w(solve_v(wt(pp)))) * mask
            pAp = float((pp * Ap).sum())
            if not (pAp > 0) or not (rz > 0):
                break
            alpha = rz / pAp
            x, r = x + alpha * pp, r - alpha * Ap
            zz = solve_u(r)
            rz_new = float((r * zz).sum())
            beta, rz = rz_new / rz, rz_new
            if not (rz_new > 0) or rz_new <= tol2 * rz0:
                break
            pp = zz + beta * pp
        dp = solve_v(gp - wt(x))
        wv = -x[:, :3]
        n2 = (wv * wv).sum(1)[:, None, None]
        S = torch.zeros((N, 3, 3), dtype=f64, device=dev)
        S[:, 0, 1], S[:, 0, 2], S[:, 1, 0], S[:, 1, 2], S[:, 2, 0], S[:, 2, 1] = -wv[:, 2], wv[:, 1], wv[:, 2], -wv[:, 0], -wv[:, 1], wv[:, 0]
        C = ((1 - n2) * eye3 + 2 * wv[:, :, None] * wv[:, None, :] + 2 * S) / (1 + n2)
        Rn, tn, Xn = C @ R, tr - x[:, 3:], X - dp
        cost_new, _ = cost_of(Rn, tn, Xn)
        if bool(cost_new <= cost_k):
            R, tr, X, lam = Rn, tn, Xn, max(lam / 4, 2.0 ** -40)
        else:
            lam = min(8 * lam, 2.0 ** 40)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return R, tr, X


def time_case(h, d, s, stream, tmp, exe):
    call(h, d, stream)
    torch.cuda.synchronize()
    tr = d.trace.cpu().numpy()[:PARAMS["iterations"]]
    twin_us = 0.0
    if d.ocap <= TWIN_MAX_OBS:
        t0 = time.perf_counter()
        want = twin.run(exe, tmp, s, **PARAMS)
        twin_us = (time.perf_counter() - t0) * 1e6
        assert np.array_equal(d.out.cpu().numpy().view(np.uint32), want["poses"]), "not the twin's poses"
        assert np.array_equal(d.pout.cpu().numpy().view(np.uint32), want["points"]) and np.array_equal(tr.view(np.uint64), want["trace_words"])
    graphs = {}
    for cg in (PARAMS["cg_iterations"], 1):
        call(h, d, stream, cg)
        torch.cuda.synchronize()
        graphs[cg] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[cg]):
            call(h, d, torch.cuda.current_stream().cuda_stream, cg)
    r = timed({"bundle": lambda: call(h, d, stream), "bundle_graph": graphs[PARAMS["cg_iterations"]].replay, "bundle_1cg": graphs[1].replay})
    torch_route(d, **PARAMS)
    t0 = time.perf_counter()
    torch_route(d, **PARAMS)
    torch_us = (time.perf_counter() - t0) * 1e6
    med = lambda k: r[k]["median_us"]
    steps = PARAMS["iterations"] * (PARAMS["cg_iterations"] - 1)
    return {"images": d.n, "rows": d.rows, "tracks": d.tcap, "observations": d.ocap, "free_cameras": int(d.counts[0]),
            "accepted": int(tr[:, 3].sum()), "cost_first": round(float(tr[0, 0]), 1), "cost_last": round(float(tr[-1, 1]), 1),
            "launches": 5 + PARAMS["iterations"] * (6 + 5 * PARAMS["cg_iterations"]),
            **{k + "_" + f: v[f] for k, v in r.items() for f in v}, "cg_step_us": round((med("bundle_graph") - med("bundle_1cg")) / steps, 2),
            "twin_program_wall_us": round(twin_us, 1), "torch_f64_wall_us": round(torch_us, 1),
            "twin_over_bundle": round(twin_us / med("bundle_graph"), 1), "torch_over_bundle": round(torch_us / med("bundle_graph"), 1),
            "warmup": WARMUP, "timed": TIMED, "lib": os.path.basename(lfp.LIB_PATH)}


def main():
    torch.cuda.init()
    torch.cuda.set_stream(torch.cuda.Stream())
    s = torch.cuda.current_stream().cuda_stream
    h = lfp.MkdHandle(max_features=64)
    args = sys.argv[1:]
    if args[:1] == ["--trace"]:
        d = Device(make_case(int(args[1]) if len(args) > 1 else 0)[1])
        for _ in range(3):
            call(h, d, s)
        torch.cuda.synchronize()
        return
    made = [make_case(k) for k in ([int(a) for a in args if a.isdigit()] or range(4))]
    devices = [Device(sc) for _, sc in made]
    # warm the largest size before any graph is captured
    call(h, max(devices, key=lambda d: lfp_scratch(d)), s)
    torch.cuda.synchronize()
    with tempfile.TemporaryDirectory() as tmp:
        exe = twin.build(tmp)
        for (name, sc), d in zip(made, devices):
            print(json.dumps({"bench": "bundle", "case": name, **time_case(h, d, sc, s, tmp, exe)}), flush=True)


def lfp_scratch(d):
    """the call's scratch in bytes, by the header's figures (4 a position, 156 a track, 664 an image, 12 a row)"""
    return 4 * d.ocap + 156 * d.tcap + 664 * d.n + 12 * d.rows


if __name__ == "__main__":
    main()
