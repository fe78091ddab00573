#!/usr/bin/env python3
"""Device time of lf_mkd_resect_cameras_device (per unregistered image its pose, stats, errors, and per row a state).  The
parent of this call had no route at all, so the comparison is with the two host programs of the tests on the same arrays, each
named as what it is:

    resect          the call with every output, enqueued directly
    resect_graph    the same call captured once in a graph and replayed
    resect_128 / resect_2048   the replayed call at 128 and 2048 samples instead of 512
    twin            tests/cpp/resect_twin.cpp (the kernels' math header under g++ -O2, one host core), the whole program run
                    on the call's arrays written to a file: wall clock of the process, file reading included, one round
    numpy           tests/resect_cases.py's float64 restatement (numpy.roots, vectorised scoring) on the first NUMPY_IMAGES
                    candidate images of at most NUMPY_MAX_M correspondences, wall clock, scaled to the number of candidates:
                    an estimate, marked as one (0: not timed)

The device forms alternate call by call, each timed with HIP events -- 5 warm-up and 20 timed rounds; the median is reported,
and the 10th and 90th percentile as the run-to-run spread (bench_tracks.py's `timed`).  Before timing, the call's words must
equal the twin's.

Cases (0.5 px noise, 30 % wrong correspondences, 20 % of the rows without a point): 64 images of about 2000 rows with 62
candidates; 256 frames of about 1000 rows of which the last 4 are candidates (a window); one query image of 2000 rows against
a map of 1.3 M points; ONE image of 10^6 rows.  Prints one JSON line per case with the times in microseconds.  `--trace CASE`
makes 20 plain calls for rocprofv3 --kernel-trace --stats.
Development aid; bench.py is the contract for the headline metric."""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("local-features_amd", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import local_features_python as lfp  # noqa: E402
import resect_cases as cases  # noqa: E402
import resect_twin as twin  # noqa: E402
from bench_tracks import TIMED, WARMUP, timed  # noqa: E402

NUMPY_IMAGES, NUMPY_MAX_M = 2, 10000      # (numpy on an image of 800 000 correspondences takes minutes: not timed, reported as 0)
PARAMS = dict(px=4.0, deg=0.0, n_samples=512, min_inliers=12, rounds=3, seed=0, flags=0)


class Device:
    def __init__(self, s):
        kps, off, rtk, pts, counts, intr, poses = twin.arrays(s)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.kps, self.off, self.rtk, self.pts = up(kps), up(off.view(np.int64)), up(rtk), up(pts)
        self.counts, self.intr, self.poses = up(counts.view(np.int32)), up(intr), up(poses)
        self.n, self.rows = len(intr), len(kps)
        self.out = torch.empty((self.n, 12), dtype=torch.float32, device="cuda")
        self.stats = torch.empty((self.n, 4), dtype=torch.int32, device="cuda")
        self.err = torch.empty((self.n, 2), dtype=torch.float32, device="cuda")
        self.state = torch.empty((self.rows,), dtype=torch.int32, device="cuda")


def call(h, d, stream, n_samples=PARAMS["n_samples"]):
    h.resect_cameras_device(d.kps.data_ptr(), d.off.data_ptr(), d.n, d.rows, d.rtk.data_ptr(), d.pts.data_ptr(), d.pts.shape[0],
                            d.counts.data_ptr(), d.intr.data_ptr(), d.poses.data_ptr(), d.out.data_ptr(), d.stats.data_ptr(),
                            d.err.data_ptr(), d.state.data_ptr(), PARAMS["px"], PARAMS["deg"], n_samples, PARAMS["min_inliers"],
                            PARAMS["rounds"], PARAMS["seed"], PARAMS["flags"], stream)


def make_case(k):
    if k == 0:
        s = cases.scene(1, (1600,) * 64)
        s["poses"][:2] = s["truth"][:2]
        return "64_images_2000_rows_62_candidates", s
    if k == 1:
        s = cases.scene(2, (800,) * 256)
        s["poses"][:252] = s["truth"][:252]
        return "256_frames_window_4", s
    if k == 2:
        s = cases.scene(3, (1600,))
        g = np.random.default_rng(3)
        more = np.concatenate([g.uniform(-50, 50, (1300000, 3)), np.full((1300000, 1), 0.9)], 1).astype(np.float32)
        s["points"] = np.concatenate([s["points"], more])
        s["counts"] = np.array([len(s["points"]), 0], np.uint32)
        return "one_query_against_1300k_points", s
    return "one_image_1000k_rows", cases.scene(4, (800000,))


def time_case(h, s, stream, tmp, exe):
    d = Device(s)
    call(h, d, stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = twin.run(exe, tmp, s, **PARAMS)
    twin_us = (time.perf_counter() - t0) * 1e6
    st = d.stats.cpu().numpy().view(np.uint32)
    assert np.array_equal(st, want["stats"]) and np.array_equal(d.out.cpu().numpy().view(np.uint32), want["poses"]), "not the twin's"
    assert np.array_equal(d.err.cpu().numpy().view(np.uint32), want["err"])
    graphs = {}
    # the LARGEST size first: a call that needs more scratch than the handle holds replaces it, and a graph captured before
    # that names the scratch that was freed
    for n in (2048, 512, 128):
        call(h, d, stream, n)
        torch.cuda.synchronize()
        graphs[n] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[n]):
            call(h, d, torch.cuda.current_stream().cuda_stream, n)
    r = timed({"resect": lambda: call(h, d, stream), "resect_graph": graphs[512].replay, "resect_128": graphs[128].replay,
               "resect_2048": graphs[2048].replay})
    cand = [i for i in range(d.n) if st[i, 2] != 1 and st[i, 0] <= NUMPY_MAX_M][:NUMPY_IMAGES]
    t0 = time.perf_counter()
    for i in cand:
        cases.resect_image(cases.correspondences(s, i)[1], s["intrinsics"][i], i, PARAMS["px"], PARAMS["n_samples"],
                           PARAMS["min_inliers"], PARAMS["rounds"])
    n_cand = int((st[:, 2] != 1).sum())
    numpy_us = (time.perf_counter() - t0) * 1e6 / max(len(cand), 1) * n_cand if cand else 0.0
    med = lambda k: r[k]["median_us"]
    return {"images": d.n, "rows": d.rows, "candidates": n_cand, "posed": int((st[:, 2] == 0).sum()),
            "correspondences": int(st[:, 0].sum()), "inliers": int(st[:, 1].sum()),
            **{k + "_" + f: v[f] for k, v in r.items() for f in v}, "twin_program_wall_us": round(twin_us, 1),
            "numpy_estimate_wall_us": round(numpy_us, 1), "numpy_images_timed": len(cand),
            "twin_over_resect": round(twin_us / med("resect_graph"), 1), "numpy_over_resect": round(numpy_us / med("resect_graph"), 1),
            "warmup": WARMUP, "timed": TIMED, "lib": os.path.basename(lfp.LIB_PATH)}


def main():
    torch.cuda.init()
    torch.cuda.set_stream(torch.cuda.Stream())
    s = torch.cuda.current_stream().cuda_stream
    h = lfp.MkdHandle(max_features=64)
    args = sys.argv[1:]
    if args[:1] == ["--trace"]:
        d = Device(make_case(int(args[1]) if len(args) > 1 else 0)[1])
        for _ in range(20):
            call(h, d, s)
        torch.cuda.synchronize()
        return
    with tempfile.TemporaryDirectory() as tmp:
        exe = twin.build(tmp)
        for k in [int(a) for a in args if a.isdigit()] or range(4):
            name, sc = make_case(k)
            print(json.dumps({"bench": "resect", "case": name, **time_case(h, sc, s, tmp, exe)}), flush=True)


if __name__ == "__main__":
    main()
