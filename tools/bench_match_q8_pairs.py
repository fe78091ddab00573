#!/usr/bin/env python3
"""Device time of lf_mkd_match_q8_pairs_device (many pairs of 8-bit rows, one matcher launch) against the two ways there were
before it, on the same rows in one process:

    f32_pairs   lf_mkd_match_pairs_device on the f32 rows the 8-bit rows were quantised from
    q8_loop     a captured hipGraph of lf_mkd_match_q8_device over the same pairs, one call per pair and direction (the graph
                is the generous reading of the loop: no host enqueue gaps; it has no counterpart for the mutual filter and is
                timed without)
    q8_pairs    the new call

The three alternate launch by launch, each timed with HIP events -- 5 warm-up and 20 timed rounds, the median is reported
(the method of bench_match_q8.py).  Cases, all both-directional with LF_MKD_MATCH_MUTUAL: 128 pairs of about 2000 x 2000 rows
(sizes drawn in 1800 .. 2200), 256 pairs of about 500 x 500, and one pair of 2000 x 2000.  Before timing, the unfiltered
q8_pairs result is compared with the loop's: they must be equal.  Prints one JSON line per case: microseconds per call (one
call = all pairs, both directions), pairs per second, and the share of the i8 MFMA peak.  Development aid; bench.py is the
contract for the headline metric."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-features_amd"))
import local_features_python as lfp  # noqa: E402

WARMUP, TIMED = 5, 20
I8_PEAK = 5.0e15     # dense int8 MFMA operations per second of an MI355X: twice the 2.5e15 of f16


class Case:
    def __init__(self, h, sizes, stream):
        self.h, self.sizes, self.s = h, sizes, stream
        na, nb = sum(s[0] for s in sizes), sum(s[1] for s in sizes)
        g = torch.Generator(device="cuda").manual_seed(na + nb)
        unit = lambda n: torch.nn.functional.normalize(torch.randn((n, 128), device="cuda", generator=g), dim=1)
        self.a, self.b = unit(na), unit(nb)
        self.qa = torch.empty((na, 128), dtype=torch.uint8, device="cuda")
        self.qb = torch.empty((nb, 128), dtype=torch.uint8, device="cuda")
        h.quantize_descriptors_device(self.a.data_ptr(), na, self.qa.data_ptr(), stream=stream)
        h.quantize_descriptors_device(self.b.data_ptr(), nb, self.qb.data_ptr(), stream=stream)
        self.oa = np.cumsum([0] + [s[0] for s in sizes]).astype(np.int64)
        self.ob = np.cumsum([0] + [s[1] for s in sizes]).astype(np.int64)
        self.d_oa, self.d_ob = torch.from_numpy(self.oa).cuda(), torch.from_numpy(self.ob).cuda()
        new = lambda n: torch.empty((n,), dtype=torch.int32, device="cuda")
        self.out = {k: (new(na), new(nb)) for k in ("f32_pairs", "q8_pairs", "q8_loop")}

    def f32_pairs(self, flags=lfp.MATCH_MUTUAL):
        ab, ba = self.out["f32_pairs"]
        self.h.match_pairs_device(self.a.data_ptr(), self.d_oa.data_ptr(), self.a.shape[0], self.b.data_ptr(), self.d_ob.data_ptr(),
                                  self.b.shape[0], len(self.sizes), ab.data_ptr(), ba.data_ptr(), 0.8, flags, None, None, self.s)

    def q8_pairs(self, flags=lfp.MATCH_MUTUAL):
        ab, ba = self.out["q8_pairs"]
        self.h.match_q8_pairs_device(self.qa.data_ptr(), self.d_oa.data_ptr(), self.qa.shape[0], self.qb.data_ptr(),
                                     self.d_ob.data_ptr(), self.qb.shape[0], len(self.sizes), ab.data_ptr(), ba.data_ptr(), 0.8,
                                     flags, None, None, self.s)

    def q8_loop(self, stream):
        ab, ba = self.out["q8_loop"]
        pa, pb, pab, pba = self.qa.data_ptr(), self.qb.data_ptr(), ab.data_ptr(), ba.data_ptr()
        for p, (na, nb) in enumerate(self.sizes):
            o, q = int(self.oa[p]), int(self.ob[p])
            self.h.match_q8_device(pa + o * 128, na, pb + q * 128, nb, pab + o * 4, 0.8, stream=stream)
            self.h.match_q8_device(pb + q * 128, nb, pa + o * 128, na, pba + q * 4, 0.8, stream=stream)

    def loop_graph(self):
        self.q8_loop(self.s)                   # warm: the handle's q8 scratch has grown to the largest plan
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.q8_loop(torch.cuda.current_stream().cuda_stream)
        return g


def time_case(h, sizes, stream):
    c = Case(h, sizes, stream)
    g = c.loop_graph()
    g.replay()
    c.q8_pairs(flags=0)
    torch.cuda.synchronize()
    assert torch.equal(c.out["q8_pairs"][0], c.out["q8_loop"][0]) and torch.equal(c.out["q8_pairs"][1], c.out["q8_loop"][1])
    calls = {"f32_pairs": c.f32_pairs, "q8_loop": g.replay, "q8_pairs": c.q8_pairs}
    events = {k: [] for k in calls}
    for it in range(WARMUP + TIMED):
        for k, fn in calls.items():            # f32, loop, q8; f32, loop, q8; ...
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            if it >= WARMUP:
                events[k].append((e0, e1))
    torch.cuda.synchronize()
    us = {k: statistics.median(e0.elapsed_time(e1) for e0, e1 in v) * 1e3 for k, v in events.items()}
    n = len(sizes)
    row_pairs = 2.0 * sum(a * b for a, b in sizes)
    R, grid = lfp.match_q8_pairs_plan(int(c.oa[-1]), int(c.ob[-1]), n, True)
    return {"pairs": n, "rows_a": int(c.oa[-1]), "rows_b": int(c.ob[-1]), "block_rows": R, "workgroups": grid,
            "f32_pairs_us": round(us["f32_pairs"], 2), "q8_loop_graph_us": round(us["q8_loop"], 2), "q8_pairs_us": round(us["q8_pairs"], 2),
            "f32_over_q8_pairs": round(us["f32_pairs"] / us["q8_pairs"], 3), "q8_loop_over_q8_pairs": round(us["q8_loop"] / us["q8_pairs"], 3),
            "q8_pairs_per_s": round(n / (us["q8_pairs"] * 1e-6), 1), "q8_row_pairs_per_s": row_pairs / (us["q8_pairs"] * 1e-6),
            "q8_fraction_of_i8_peak": round(row_pairs * 256 / (us["q8_pairs"] * 1e-6) / I8_PEAK, 4),
            "mutual_q8": int((c.out["q8_pairs"][0] >= 0).sum()), "mutual_f32": int((c.out["f32_pairs"][0] >= 0).sum()),
            "warmup": WARMUP, "timed": TIMED}


def main():
    torch.cuda.init()
    torch.cuda.set_stream(torch.cuda.Stream())
    s = torch.cuda.current_stream().cuda_stream
    h = lfp.MkdHandle(max_features=64)
    g = np.random.default_rng(0)
    big = [(int(x), int(y)) for x, y in g.integers(1800, 2201, (128, 2))]
    small = [(int(x), int(y)) for x, y in g.integers(450, 551, (256, 2))]
    for name, sizes in (("128x2000", big), ("256x500", small), ("1x2000", [(2000, 2000)])):
        print(json.dumps({"bench": "match_q8_pairs", "case": name, **time_case(h, sizes, s)}), flush=True)


if __name__ == "__main__":
    main()
