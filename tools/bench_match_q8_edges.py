#!/usr/bin/env python3
"""Device time of lf_mkd_match_q8_edges_device (any pairs of images from one pool, no row copied) against the only route there
was before it, on the same pool and the same edges in one process:

    edges        the new call on the pool, both edge layouts already made (lf_mkd_edge_layout_device, timed on its own below)
    copy_pairs   torch.index_select of every edge's rows into pair layout (into buffers that exist already), then
                 lf_mkd_match_q8_pairs_device on the copies with the edge layouts as its offsets.  A side whose edge list is
                 0, 1, 2, .. is in pair layout as it stands and is NOT copied: the route is given its best form
    pairs_only   that route's matcher alone, on copies made before the clock starts: the matcher's share of copy_pairs

The three alternate call by call, each timed with HIP events -- 5 warm-up and 20 timed rounds; the median is reported, and
the 10th and 90th percentile as the run-to-run spread (the method of bench_match_q8_pairs.py).  Every call is both ways with
LF_MKD_MATCH_MUTUAL.  Before timing, the edges result is compared with the route's: they must be equal.

Cases: 64 images of about 2000 rows, all 2016 pairs; one query of 2000 rows against 1024 database images of about 2000 rows
(two pools); 256 frames of about 500 rows, every frame against the next 4.  Then the layout call alone at 2016 and at 2^20
edges.  Prints one JSON line per case with the times in microseconds and the bytes of row copies the edges call avoids.
Development aid; bench.py is the contract for the headline metric."""
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


def pool(h, sizes, seed, stream):
    """(q [n,128] uint8, offsets [len(sizes) + 1] int64) on the device: random unit rows, quantised"""
    n = int(sum(sizes))
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.nn.functional.normalize(torch.randn((n, 128), device="cuda", generator=g), dim=1)
    q = torch.empty((n, 128), dtype=torch.uint8, device="cuda")
    h.quantize_descriptors_device(x.data_ptr(), n, q.data_ptr(), stream=stream)
    return q, torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)).cuda()


def layout(h, o, total, edge, stream):
    out = torch.empty((edge.numel() + 1,), dtype=torch.int64, device="cuda")
    h.edge_layout_device(o.data_ptr(), o.numel() - 1, total, edge.data_ptr(), edge.numel(), out.data_ptr(), stream)
    return out


def timed(calls):
    events = {k: [] for k in calls}
    for it in range(WARMUP + TIMED):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            if it >= WARMUP:
                events[k].append((e0, e1))
    torch.cuda.synchronize()
    out = {}
    for k, v in events.items():
        us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in v)
        out[k] = {"median_us": round(statistics.median(us), 2), "p10_us": round(us[len(us) // 10], 2),
                  "p90_us": round(us[len(us) - 1 - len(us) // 10], 2)}
    return out


class Side:
    """one side of a case: the pool, the edge ids, the layout, and the rows in pair layout for the parent's route"""

    def __init__(self, h, q, o, edge, stream):
        self.q, self.o, self.edge = q, o, edge
        self.n_images, self.total = o.numel() - 1, q.shape[0]
        self.layout = layout(h, o, self.total, edge, stream)
        torch.cuda.synchronize()
        self.cap = int(self.layout[-1])
        self.in_place = edge.numel() == self.n_images and bool((edge == torch.arange(self.n_images, device="cuda", dtype=edge.dtype)).all())
        if self.in_place:                      # already in pair layout: the route passes the pool and its offsets
            self.rows, self.copy = q, None
            self.offsets, self.rows_total = o, self.total
        else:
            e_of = torch.searchsorted(self.layout, torch.arange(self.cap, device="cuda"), right=True) - 1
            self.index = torch.arange(self.cap, device="cuda") - self.layout[e_of] + o[edge.long()[e_of]]
            self.rows = torch.empty((self.cap, 128), dtype=torch.uint8, device="cuda")
            self.copy = lambda: torch.index_select(q, 0, self.index, out=self.rows)
            self.copy()
            self.offsets, self.rows_total = self.layout, self.cap
        self.copied_bytes = 0 if self.in_place else self.cap * 128


def time_case(h, A, B, stream):
    n_edges = A.edge.numel()
    new = lambda n: torch.empty((n,), dtype=torch.int32, device="cuda")
    out_e, out_p = (new(A.cap), new(B.cap)), (new(A.cap), new(B.cap))

    def edges():
        h.match_q8_edges_device(A.q.data_ptr(), A.o.data_ptr(), A.n_images, A.total, B.q.data_ptr(), B.o.data_ptr(), B.n_images,
                                B.total, A.edge.data_ptr(), B.edge.data_ptr(), A.layout.data_ptr(), A.cap, n_edges, out_e[0].data_ptr(),
                                B.layout.data_ptr(), B.cap, out_e[1].data_ptr(), 0.8, lfp.MATCH_MUTUAL, None, None, stream)

    def pairs_only():
        # (with a side in place its match array is indexed like the pool: the same entries, the pool's offsets)
        h.match_q8_pairs_device(A.rows.data_ptr(), A.offsets.data_ptr(), A.rows_total, B.rows.data_ptr(), B.offsets.data_ptr(),
                                B.rows_total, n_edges, out_p[0].data_ptr(), out_p[1].data_ptr(), 0.8, lfp.MATCH_MUTUAL, None, None, stream)

    def copy_pairs():
        for side in (A, B):
            if side.copy:
                side.copy()
        pairs_only()

    edges()
    copy_pairs()
    torch.cuda.synchronize()
    assert torch.equal(out_e[0], out_p[0]) and torch.equal(out_e[1], out_p[1]), "the edges call and the copy route disagree"
    t = timed({"edges": edges, "copy_pairs": copy_pairs, "pairs_only": pairs_only})
    R, grid = lfp.match_q8_pairs_plan(A.cap, B.cap, n_edges, True)
    return {"edges": n_edges, "images_a": A.n_images, "images_b": B.n_images, "pool_rows_a": A.total, "pool_rows_b": B.total,
            "layout_rows_a": A.cap, "layout_rows_b": B.cap, "block_rows": R, "workgroups": grid,
            "copied_bytes_avoided": A.copied_bytes + B.copied_bytes, "mutual_matches": int((out_e[0] >= 0).sum()),
            **{k + "_" + f: v[f] for k, v in t.items() for f in v},
            "edges_over_pairs_only": round(t["edges"]["median_us"] / t["pairs_only"]["median_us"], 3),
            "copy_pairs_over_edges": round(t["copy_pairs"]["median_us"] / t["edges"]["median_us"], 3), "warmup": WARMUP, "timed": TIMED}


def main():
    torch.cuda.init()
    torch.cuda.set_stream(torch.cuda.Stream())
    s = torch.cuda.current_stream().cuda_stream
    h = lfp.MkdHandle(max_features=64)
    g = np.random.default_rng(0)
    ids = lambda x: torch.tensor(np.asarray(x, np.int32), device="cuda")
    # 64 images of about 2000 rows, all 2016 pairs
    q, o = pool(h, g.integers(1800, 2201, 64), 1, s)
    i, j = np.triu_indices(64, 1)
    A, B = Side(h, q, o, ids(i), s), Side(h, q, o, ids(j), s)
    print(json.dumps({"bench": "match_q8_edges", "case": "all_pairs_64x2000", **time_case(h, A, B, s)}), flush=True)
    t = timed({"layout": lambda: layout(h, o, q.shape[0], A.edge, s)})
    print(json.dumps({"bench": "edge_layout", "edges": 2016, **t["layout"]}), flush=True)
    del A, B, q, o
    # one query of 2000 rows against 1024 database images of about 2000 rows
    qq, oq = pool(h, [2000], 2, s)
    qd, od = pool(h, g.integers(1800, 2201, 1024), 3, s)
    A, B = Side(h, qq, oq, ids(np.zeros(1024)), s), Side(h, qd, od, ids(np.arange(1024)), s)
    print(json.dumps({"bench": "match_q8_edges", "case": "query_2000_x_1024_images", **time_case(h, A, B, s)}), flush=True)
    big = ids(g.integers(0, 1024, 1 << 20))
    want = torch.cat([od[:1] * 0, torch.cumsum((od[1:] - od[:-1])[big.long()], 0)])
    assert torch.equal(layout(h, od, qd.shape[0], big, s), want), "the layout at 2^20 edges is not the prefix sum"
    t = timed({"layout": lambda: layout(h, od, qd.shape[0], big, s)})
    print(json.dumps({"bench": "edge_layout", "edges": 1 << 20, **t["layout"]}), flush=True)
    del A, B, qq, oq, qd, od, big
    # 256 frames of about 500 rows, every frame against the next 4
    q, o = pool(h, g.integers(450, 551, 256), 4, s)
    pairs = [(t, t + d) for d in range(1, 5) for t in range(256 - d)]
    A, B = Side(h, q, o, ids([p[0] for p in pairs]), s), Side(h, q, o, ids([p[1] for p in pairs]), s)
    print(json.dumps({"bench": "match_q8_edges", "case": "window4_256x500", **time_case(h, A, B, s)}), flush=True)


if __name__ == "__main__":
    main()
