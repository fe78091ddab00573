#!/usr/bin/env python3
"""Device time of lf_mkd_verify_homography_device (RANSAC homography verification, three launches per call): one pair of
M in {500, 2000, 20000} matches x n_hypotheses in {256, 2048, 16384}, and 128 pairs of ~1000 matches in one call.

Each case records 20 back-to-back calls in one torch CUDA graph and replays it: the per-call figure is device time without
host enqueue gaps.  Prints one JSON line: us per call and hypothesis-point evaluations per second (n_hypotheses x M summed
over the pairs, divided by the time).

--trace: only the example's operating point (one pair of 1000 matches, 2048 hypotheses), 50 plain calls on one stream, for
a per-kernel trace of the three launches (rocprofv3 --kernel-trace --stats -- python tools/bench_verify.py --trace)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-features_amd"))
import local_features_python as lfp  # noqa: E402

CALLS, REPLAYS = 20, 10
H_TRUE = np.array([[0.92, -0.18, 60.0], [0.12, 1.05, -30.0], [1.2e-4, -1.5e-4, 1.0]])


def planted(m, g, frac=0.5):
    a = g.uniform(0, 1000, (m, 2))
    q = np.concatenate([a, np.ones((m, 1))], axis=1) @ H_TRUE.T
    b = q[:, :2] / q[:, 2:] + g.normal(0, 0.5, (m, 2))
    out = g.random(m) >= frac
    b[out] = g.uniform(0, 1000, (int(out.sum()), 2))
    ka, kb = np.zeros((m, 5), np.float32), np.zeros((m, 5), np.float32)
    ka[:, :2], kb[:, :2] = a, b
    return ka, kb, np.arange(m, dtype=np.int32)


def time_case(h, sizes, n_hyp, g):
    pairs = [planted(m, g) for m in sizes]
    oa = torch.tensor(np.cumsum([0] + sizes), dtype=torch.int64, device="cuda")
    ka = torch.from_numpy(np.concatenate([p[0] for p in pairs])).cuda()
    kb = torch.from_numpy(np.concatenate([p[1] for p in pairs])).cuda()
    mt = torch.from_numpy(np.concatenate([p[2] for p in pairs])).cuda()
    n = len(sizes)
    H = torch.empty((n, 9), device="cuda")
    ver = torch.empty((len(ka),), dtype=torch.int32, device="cuda")
    st = torch.empty((n, 4), dtype=torch.int32, device="cuda")

    def call(stream):
        h.verify_homography_device(ka.data_ptr(), oa.data_ptr(), kb.data_ptr(), oa.data_ptr(), mt.data_ptr(), n, H.data_ptr(),
                                   ver.data_ptr(), st.data_ptr(), n_hyp, 3.0, 0, 0, stream)

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        call(s.cuda_stream)          # grows the handle's scratch: the captured calls allocate nothing
    s.synchronize()
    g_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_):
        for _ in range(CALLS):
            call(torch.cuda.current_stream().cuda_stream)
    g_.replay()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(REPLAYS):
        g_.replay()
    t1.record()
    torch.cuda.synchronize()
    us = t0.elapsed_time(t1) * 1e3 / (CALLS * REPLAYS)
    inl = st[:, 0].cpu().numpy()
    return {"us": round(us, 2), "evals_per_s": float(n_hyp * sum(sizes) / (us * 1e-6)),
            "mean_inlier_fraction": round(float(inl.sum() / sum(sizes)), 3)}


def trace(h, g, calls=50):
    ka, kb, mt = (torch.from_numpy(x).cuda() for x in planted(1000, g))
    oa = torch.tensor([0, 1000], dtype=torch.int64, device="cuda")
    H = torch.empty((1, 9), device="cuda")
    ver = torch.empty((1000,), dtype=torch.int32, device="cuda")
    st = torch.empty((1, 4), dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    for _ in range(calls):
        h.verify_homography_device(ka.data_ptr(), oa.data_ptr(), kb.data_ptr(), oa.data_ptr(), mt.data_ptr(), 1, H.data_ptr(),
                                   ver.data_ptr(), st.data_ptr(), 2048, 3.0, 0, 0, s.cuda_stream)
    s.synchronize()
    print(json.dumps({"bench": "verify_homography trace", "calls": calls, "stats": st.cpu().tolist()}))


def main():
    torch.cuda.init()
    h = lfp.MkdHandle(max_features=64)
    g = np.random.default_rng(0)
    if "--trace" in sys.argv[1:]:
        return trace(h, g)
    out = {"bench": "verify_homography", "launches_per_call": 3, "single_pair": {}}
    for m in (500, 2000, 20000):
        for n_hyp in (256, 2048, 16384):
            out["single_pair"][f"M{m}_hyp{n_hyp}"] = time_case(h, [m], n_hyp, g)
    out["example_point_M1000_hyp2048"] = time_case(h, [1000], 2048, g)
    out["batch_128x1000_hyp2048"] = time_case(h, [int(x) for x in g.integers(900, 1100, 128)], 2048, g)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
