#!/usr/bin/env python3
"""Device time of lf_mkd_verify_fundamental_device (RANSAC fundamental matrix, three launches per call): one pair of ~1000
matches x 2048 samples, 128 pairs of ~1000 matches in one call, and one pair of 20000 matches x 16384 samples.

Each case records back-to-back calls in one torch CUDA graph and replays it: the per-call figure is device time without host
enqueue gaps.  Prints one JSON line: us per call and candidate-point evaluations per second (3 x n_hypotheses x M summed over
the pairs, divided by the time: every sample is scored as three candidates).

--trace: one pair of 1000 matches x 2048 samples, 50 plain calls on one stream, for a per-kernel trace of the three launches
(rocprofv3 --kernel-trace --stats -- python tools/bench_verify_fundamental.py --trace)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-features_amd"))
import local_features_python as lfp  # noqa: E402

REPLAYS = 10
K = np.array([[800.0, 0.0, 512.0], [0.0, 800.0, 384.0], [0.0, 0.0, 1.0]])


def two_view(m, g, outliers=0.5):
    """m matches of random 3-D points (depth 4 .. 12) seen by two cameras with a general motion, 0.5 px noise."""
    ang = np.deg2rad([2.0, -4.0, 3.0])
    c, s = np.cos(ang), np.sin(ang)
    r = (np.array([[c[2], -s[2], 0], [s[2], c[2], 0], [0, 0, 1]]) @ np.array([[c[1], 0, s[1]], [0, 1, 0], [-s[1], 0, c[1]]])
         @ np.array([[1, 0, 0], [0, c[0], -s[0]], [0, s[0], c[0]]]))
    t = np.array([0.8, 0.15, 0.3])
    uv = g.uniform([0, 0], [1024, 768], (m, 2))
    z = g.uniform(4.0, 12.0, m)
    x = np.concatenate([(uv - K[:2, 2]) / K[0, 0] * z[:, None], z[:, None]], axis=1)
    p = (x @ r.T + t) @ K.T
    b = p[:, :2] / p[:, 2:] + g.normal(0, 0.5, (m, 2))
    out = g.random(m) < outliers
    b[out] = g.uniform([0, 0], [1024, 768], (int(out.sum()), 2))
    ka, kb = np.zeros((m, 5), np.float32), np.zeros((m, 5), np.float32)
    ka[:, :2], kb[:, :2] = uv, b
    return ka, kb, np.arange(m, dtype=np.int32)


def _inputs(sizes, g):
    pairs = [two_view(m, g) for m in sizes]
    oa = torch.tensor(np.cumsum([0] + sizes), dtype=torch.int64, device="cuda")
    ka = torch.from_numpy(np.concatenate([p[0] for p in pairs])).cuda()
    kb = torch.from_numpy(np.concatenate([p[1] for p in pairs])).cuda()
    mt = torch.from_numpy(np.concatenate([p[2] for p in pairs])).cuda()
    n = len(sizes)
    return ka, kb, mt, oa, torch.empty((n, 9), device="cuda"), torch.empty((len(ka),), dtype=torch.int32, device="cuda"), \
        torch.empty((n, 4), dtype=torch.int32, device="cuda")


def time_case(h, sizes, n_hyp, g, calls):
    ka, kb, mt, oa, F, ver, st = _inputs(sizes, g)
    n = len(sizes)

    def call(stream):
        h.verify_fundamental_device(ka.data_ptr(), oa.data_ptr(), kb.data_ptr(), oa.data_ptr(), mt.data_ptr(), n, F.data_ptr(),
                                    ver.data_ptr(), st.data_ptr(), n_hyp, 1.5, 0, 0, stream)

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        call(s.cuda_stream)          # grows the handle's scratch: the captured calls allocate nothing
    s.synchronize()
    g_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_):
        for _ in range(calls):
            call(torch.cuda.current_stream().cuda_stream)
    g_.replay()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(REPLAYS):
        g_.replay()
    t1.record()
    torch.cuda.synchronize()
    us = t0.elapsed_time(t1) * 1e3 / (calls * REPLAYS)
    inl = st[:, 0].cpu().numpy()
    return {"us": round(us, 2), "candidate_evals_per_s": float(3 * n_hyp * sum(sizes) / (us * 1e-6)),
            "mean_inlier_fraction": round(float(inl.sum() / sum(sizes)), 3)}


def trace(h, g, calls=50):
    ka, kb, mt, oa, F, ver, st = _inputs([1000], g)
    s = torch.cuda.Stream()
    for _ in range(calls):
        h.verify_fundamental_device(ka.data_ptr(), oa.data_ptr(), kb.data_ptr(), oa.data_ptr(), mt.data_ptr(), 1, F.data_ptr(),
                                    ver.data_ptr(), st.data_ptr(), 2048, 1.5, 0, 0, s.cuda_stream)
    s.synchronize()
    print(json.dumps({"bench": "verify_fundamental trace", "calls": calls, "stats": st.cpu().tolist()}))


def main():
    torch.cuda.init()
    h = lfp.MkdHandle(max_features=64)
    g = np.random.default_rng(0)
    if "--trace" in sys.argv[1:]:
        return trace(h, g)
    out = {"bench": "verify_fundamental", "launches_per_call": 3}
    out["single_pair_M1000_hyp2048"] = time_case(h, [1000], 2048, g, 20)
    out["batch_128x1000_hyp2048"] = time_case(h, [int(x) for x in g.integers(900, 1100, 128)], 2048, g, 5)
    out["single_pair_M20000_hyp16384"] = time_case(h, [20000], 16384, g, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
