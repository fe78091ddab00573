#!/usr/bin/env python3
"""Device time of lf_mkd_bundle_adjust_intrinsics_device at 10 iterations x 10 CG steps against its sibling,
lf_mkd_bundle_adjust_device, on the same arrays: tools/bench_bundle.py's 64 images of about 2000 rows (0.5 px noise, 5 % wrong
observations, perturbed poses and points, tracks of 4 views), the input focal lengths 3 % off.

    fixed              lf_mkd_bundle_adjust_device, captured once in a graph and replayed (565 launches)
    refine0            the new call with nothing refined (its double-intrinsics kernels, no group free; 676 launches)
    refine1, refine3   one group, the focal scale / the focal scale and the principal point refined
    per_image_refine1  a group per image (64 groups): every per-group workgroup walks all image ids
    *_1cg              the same at 10 iterations x 1 CG step: (x - x_1cg) / 90 is the time of a CG step

Every form is a replayed graph, timed with HIP events in alternation -- 5 warm-up and 20 timed rounds, the median, and the 10th
and 90th percentile as the spread (bench_tracks.py's `timed`).  Before timing, refine1's words must equal the twin's
(tests/cpp/bundle_intr_twin.cpp) and refine0's shared words the sibling's.  `cg_steps_*`: the CG steps the trace shows over 10
iterations when CG may stop by its tolerance (cg_iterations 64, cg_tol 0.1), without and with the shared block.
Prints one JSON line with the times in microseconds.  Development aid; bench.py is the contract for the headline metric."""
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("local-features_amd", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import local_features_python as lfp  # noqa: E402
import bundle_intr_twin as twin  # noqa: E402
import bench_bundle as base  # noqa: E402
from bench_tracks import TIMED, WARMUP, timed  # noqa: E402

PARAMS = dict(base.PARAMS)
SCALE = 1.03


class Device(base.Device):
    def __init__(self, s):
        super().__init__(s)
        self.kout = torch.empty_like(self.K)
        self.per_image = torch.arange(self.n, dtype=torch.int32, device="cuda")
        self.gout = torch.zeros((self.n, 3), dtype=torch.float32, device="cuda")
        self.trace9 = torch.zeros((64, 9), dtype=torch.float64, device="cuda")
        self.counts5 = torch.zeros((5,), dtype=torch.int32, device="cuda")


def call(h, d, stream, refine, per_image=False, cg_iterations=PARAMS["cg_iterations"], cg_tol=PARAMS["cg_tol"]):
    h.bundle_adjust_intrinsics_device(
        d.kps.data_ptr(), d.ioff.data_ptr(), d.n, d.rows, d.toff.data_ptr(), d.tcap, d.row.data_ptr(), d.img.data_ptr(), d.ocap,
        d.tc.data_ptr(), d.pts.data_ptr(), d.K.data_ptr(), d.poses.data_ptr(), d.out.data_ptr(), d.pout.data_ptr(), d.kout.data_ptr(),
        d.trace9.data_ptr(), d.counts5.data_ptr(), d_camera_fixed=d.fixed.data_ptr(),
        d_camera_group=d.per_image.data_ptr() if per_image else None, n_groups=d.n if per_image else 1, refine=refine,
        d_group_out=d.gout.data_ptr(), d_obs_state_out=d.state.data_ptr(), max_reproj_px=PARAMS["px"], lambda0=PARAMS["lambda0"],
        iterations=PARAMS["iterations"], cg_iterations=cg_iterations, cg_tol=cg_tol, stream=stream)


def main():
    torch.cuda.init()
    torch.cuda.set_stream(torch.cuda.Stream())
    stream = torch.cuda.current_stream().cuda_stream
    h = lfp.MkdHandle(max_features=64)
    name, s = base.make_case(0)
    s["intrinsics"] = s["intrinsics"].copy()
    s["intrinsics"][:, :2] *= np.float32(SCALE)
    d = Device(s)
    words = lambda x, t=np.uint32: x.cpu().numpy().view(t)
    # the largest scratch first (a group per image), then the checks
    call(h, d, stream, 1, per_image=True)
    torch.cuda.synchronize()
    with tempfile.TemporaryDirectory() as tmp:
        want = twin.run(twin.build(tmp), tmp, s, refine=1, **PARAMS)
    call(h, d, stream, 1)
    torch.cuda.synchronize()
    assert np.array_equal(words(d.out), want["poses"]) and np.array_equal(words(d.pout), want["points"]), "not the twin's words"
    assert np.array_equal(words(d.kout), want["intrinsics"]) and np.array_equal(words(d.trace9, np.uint64)[:10], want["trace_words"])
    sigma = float(d.gout[0, 0])
    call(h, d, stream, 0)
    torch.cuda.synchronize()
    shared = [words(d.out).copy(), words(d.pout).copy(), words(d.trace9, np.uint64)[:10, :8].copy()]
    base.call(h, d, stream)
    torch.cuda.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(shared, [words(d.out), words(d.pout), words(d.trace, np.uint64)[:10]])), \
        "refine 0 is not the sibling's words"
    steps = {}
    for key, refine in (("cg_steps_fixed_intrinsics", 0), ("cg_steps_refine1", 1), ("cg_steps_refine3", 3)):
        call(h, d, stream, refine, cg_iterations=64, cg_tol=0.1)
        torch.cuda.synchronize()
        steps[key] = int(d.trace9[:10, 4].sum())
    forms = {"fixed": lambda st, cg: base.call(h, d, st, cg), "refine0": lambda st, cg: call(h, d, st, 0, cg_iterations=cg),
             "refine1": lambda st, cg: call(h, d, st, 1, cg_iterations=cg), "refine3": lambda st, cg: call(h, d, st, 3, cg_iterations=cg),
             "per_image_refine1": lambda st, cg: call(h, d, st, 1, per_image=True, cg_iterations=cg)}
    graphs = {}
    for key, f in forms.items():
        for cg in (PARAMS["cg_iterations"], 1):
            f(stream, cg)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                f(torch.cuda.current_stream().cuda_stream, cg)
            graphs[key + ("" if cg != 1 else "_1cg")] = g
    r = timed({k: g.replay for k, g in graphs.items()})
    med = lambda k: r[k]["median_us"]
    n_steps = PARAMS["iterations"] * (PARAMS["cg_iterations"] - 1)
    it, cg = PARAMS["iterations"], PARAMS["cg_iterations"]
    out = {"bench": "bundle_intrinsics", "case": name, "images": d.n, "rows": d.rows, "tracks": d.tcap, "observations": d.ocap,
           "input_focal_scale": SCALE, "refine1_sigma_times_scale": round(sigma * SCALE, 6),
           "launches_fixed": 5 + it * (6 + 5 * cg), "launches_intrinsics": 6 + it * (7 + 6 * cg), **steps,
           **{k + "_" + f: v[f] for k, v in r.items() for f in v},
           **{"cg_step_us_" + k: round((med(k) - med(k + "_1cg")) / n_steps, 2) for k in forms},
           **{k + "_over_fixed": round(med(k) / med("fixed"), 3) for k in forms if k != "fixed"},
           "warmup": WARMUP, "timed": TIMED, "lib": os.path.basename(lfp.LIB_PATH)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
