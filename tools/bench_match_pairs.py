#!/usr/bin/env python3
"""Device time of lf_mkd_match_pairs_device (many pairs, one launch) against the only way there was before it: a loop of
lf_mkd_match_both_device over the same pairs.

Cases, all both-directional: 128 pairs of about 2000 x 2000 rows (sizes drawn in 1800 .. 2200), the same with
LF_MKD_MATCH_MUTUAL (the loop has no counterpart for the filter: it is timed without), 256 pairs of about 500 x 500, and
one pair of 2000 x 2000.

Each side is recorded in a torch CUDA graph (several calls back to back) and the replays are timed by events: device time
without host enqueue gaps, which is the generous reading of the loop.  The loop is also timed as plain calls on a stream,
which is what a caller pays today.  The sides alternate, five repeats each, so that the spread is known.  Prints one JSON
line: microseconds per call (one call = all pairs), the ratio of the medians, and pairs per second.

--trace: the single pair only, 50 plain calls of either entry point alternating on one stream, for a per-kernel trace that
sets match_small_pairs beside match_small_both on the same rows
(rocprofv3 --kernel-trace --stats -- python tools/bench_match_pairs.py --trace)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-features_amd"))
import local_features_python as lfp  # noqa: E402

REPEATS, REPLAYS = 5, 5


class Case:
    def __init__(self, h, sizes, flags=0):
        self.h, self.sizes, self.flags = h, sizes, flags
        na, nb = sum(s[0] for s in sizes), sum(s[1] for s in sizes)
        g = torch.Generator(device="cuda").manual_seed(na + nb)
        unit = lambda n: torch.nn.functional.normalize(torch.randn((n, 128), device="cuda", generator=g), dim=1)
        self.a, self.b = unit(na), unit(nb)
        self.oa = np.cumsum([0] + [s[0] for s in sizes]).astype(np.int64)
        self.ob = np.cumsum([0] + [s[1] for s in sizes]).astype(np.int64)
        self.d_oa, self.d_ob = torch.from_numpy(self.oa).cuda(), torch.from_numpy(self.ob).cuda()
        self.ab = torch.empty((na,), dtype=torch.int32, device="cuda")
        self.ba = torch.empty((nb,), dtype=torch.int32, device="cuda")
        self.ab_loop, self.ba_loop = torch.empty_like(self.ab), torch.empty_like(self.ba)

    def batched(self, stream):
        self.h.match_pairs_device(self.a.data_ptr(), self.d_oa.data_ptr(), self.a.shape[0], self.b.data_ptr(), self.d_ob.data_ptr(),
                                  self.b.shape[0], len(self.sizes), self.ab.data_ptr(), self.ba.data_ptr(), 0.8, self.flags,
                                  None, None, stream)

    def loop(self, stream):
        pa, pb, pab, pba = self.a.data_ptr(), self.b.data_ptr(), self.ab_loop.data_ptr(), self.ba_loop.data_ptr()
        for p, (na, nb) in enumerate(self.sizes):
            o, q = int(self.oa[p]), int(self.ob[p])
            self.h.match_both_device(pa + o * 512, na, pb + q * 512, nb, pab + o * 4, pba + q * 4, 0.8, stream)

    def graph(self, fn, calls):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            fn(s.cuda_stream)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(calls):
                fn(torch.cuda.current_stream().cuda_stream)
        g.replay()
        torch.cuda.synchronize()
        return g


def replay_us(g, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(REPLAYS):
        g.replay()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / (calls * REPLAYS)


def plain_us(fn, calls):
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    w0 = time.perf_counter()
    with torch.cuda.stream(s):
        for _ in range(calls):
            fn(s.cuda_stream)
    s.synchronize()
    return (time.perf_counter() - w0) * 1e6 / calls


def time_case(h, sizes, flags=0):
    c = Case(h, sizes, flags)
    n = len(sizes)
    calls_b = 20
    calls_l = 20 if n == 1 else max(1, 256 // n)        # the loop's graph holds calls_l x n launches
    g_b, g_l = c.graph(c.batched, calls_b), c.graph(c.loop, calls_l)
    if not flags:       # the two ways agree (the mutual filter has no counterpart in the loop)
        assert torch.equal(c.ab, c.ab_loop) and torch.equal(c.ba, c.ba_loop)
    batched, loop, plain, plain_b = [], [], [], []
    for _ in range(REPEATS):
        batched.append(replay_us(g_b, calls_b))
        loop.append(replay_us(g_l, calls_l))
        plain.append(plain_us(c.loop, 2 if n > 1 else 20))
        plain_b.append(plain_us(c.batched, 20))
    med = lambda x: float(np.median(x))
    r = lambda x: [round(v, 2) for v in x]
    return {"pairs": n, "rows_a": int(c.oa[-1]), "rows_b": int(c.ob[-1]), "launches_per_call": 3 if flags else 1,
            "batched_us": r(batched), "loop_graph_us": r(loop), "loop_plain_us": r(plain), "batched_plain_us": r(plain_b),
            "batched_median_us": round(med(batched), 2), "loop_graph_median_us": round(med(loop), 2),
            "loop_plain_median_us": round(med(plain), 2),
            "loop_graph_over_batched": round(med(loop) / med(batched), 3), "loop_plain_over_batched": round(med(plain) / med(batched), 3),
            "pairs_per_s": round(n / (med(batched) * 1e-6), 1),
            "row_pairs_per_s": float(2 * sum(a * b for a, b in sizes) / (med(batched) * 1e-6))}


def main():
    torch.cuda.init()
    h = lfp.MkdHandle(max_features=64)
    g = np.random.default_rng(0)
    big = [(int(x), int(y)) for x, y in g.integers(1800, 2201, (128, 2))]
    small = [(int(x), int(y)) for x, y in g.integers(450, 551, (256, 2))]
    if "--trace" in sys.argv[1:]:
        c = Case(h, [(2000, 2000)])
        s = torch.cuda.Stream()
        for _ in range(50):
            c.batched(s.cuda_stream)
            c.loop(s.cuda_stream)
        s.synchronize()
        print(json.dumps({"bench": "match_pairs trace", "pairs": 1, "calls_each": 50}))
        return
    out = {"bench": "match_pairs", "repeats": REPEATS,
           "128x2000": time_case(h, big), "128x2000_mutual": time_case(h, big, lfp.MATCH_MUTUAL),
           "256x500": time_case(h, small), "1x2000": time_case(h, [(2000, 2000)])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
