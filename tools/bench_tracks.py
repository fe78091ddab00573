#!/usr/bin/env python3
"""Device time of lf_mkd_build_tracks_device (the tracks of an edge list's matches: a label per pool row, per track its length
and its conflicting rows) against the only route there was before it, on the same arrays in one process:

    tracks        the call without the statistics (labels only)
    tracks_stats  the call with d_track_len and d_track_dup
    no_edges      the call with n_edges = 0 and no statistics: its init and flatten launches alone, so that
                  tracks - no_edges is the link launch and tracks_stats - tracks the three statistics launches
    tracks_len    the call with d_track_len alone (zero + len), tracks_dup with d_track_dup alone (zero + dup, every row
                  scanning: without the lengths no row is known to be alone)
    host          the match array and the layout copied to the host, the links taken from them with numpy, then
                  scipy.sparse.csgraph.connected_components (or, without scipy, the numpy union-find of tests/tracks_cases.py)
                  and the components' smallest rows: labels only, the copies included, wall clock from a synchronised start

The five device forms alternate call by call, each timed with HIP events -- 5 warm-up and 20 timed rounds; the median is
reported, and the 10th and 90th percentile as the run-to-run spread (the method of bench_match_q8_edges.py).  The host route
runs 1 + 5 times.  Before timing, the device's labels are compared with the host route's: they must be equal.

Cases, the three of bench_match_q8_edges.py over ONE pool, with synthetic match arrays of which about 40 % of the entries are
links: 64 images of about 2000 rows, all 2016 pairs; one query of 2000 rows against 1024 images of about 2000 rows; 256 frames
of about 500 rows, every frame against the next 4.  "scene": every image's rows are a random subset of the points of one scene
and a row is matched to the row of the other image that shows the same point, so the tracks are the scene's points, consistent
and at most one row an image.  "random" (the 64-image case only): every link goes to a random row of the other image, which
ties nearly all rows into ONE track -- every link then contends on one tree.
Prints one JSON line per case with the times in microseconds.  Development aid; bench.py is the contract for the headline
metric."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-features_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import local_features_python as lfp  # noqa: E402

try:
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    HOST = "scipy.sparse.csgraph.connected_components"
except ImportError:
    import tracks_cases
    HOST = "numpy union-find (tests/tracks_cases.py)"

WARMUP, TIMED = 5, 20
HOST_WARMUP, HOST_TIMED = 1, 5
LINKED = 0.4


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


class Case:
    """a pool's offsets, an edge list, the a side's layout and a synthetic match array in it, all on the device"""

    def __init__(self, h, sizes, edges, seed, stream, scene=True):
        g = torch.Generator(device="cuda").manual_seed(seed)
        sizes = np.asarray(sizes, np.int64)
        self.n_images, self.total, self.n_edges = len(sizes), int(sizes.sum()), len(edges)
        self.o = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)])).cuda()
        self.ea = torch.tensor([e[0] for e in edges], dtype=torch.int32, device="cuda")
        self.eb = torch.tensor([e[1] for e in edges], dtype=torch.int32, device="cuda")
        self.la = torch.empty((self.n_edges + 1,), dtype=torch.int64, device="cuda")
        h.edge_layout_device(self.o.data_ptr(), self.n_images, self.total, self.ea.data_ptr(), self.n_edges, self.la.data_ptr(), stream)
        torch.cuda.synchronize()
        self.cap = int(self.la[-1])
        at = torch.arange(self.cap, device="cuda")
        e_of = torch.searchsorted(self.la, at, right=True) - 1
        row_a = at - self.la[e_of] + self.o[self.ea.long()[e_of]]                  # the entry's pool row
        image_b = self.eb.long()[e_of]
        d_sizes = torch.from_numpy(sizes).cuda()
        if scene:
            # every image shows a random subset of P points, P such that two images share about LINKED of their rows
            P = int(sizes.max() / LINKED)
            point = torch.empty((self.total,), dtype=torch.int64, device="cuda")
            where = torch.full((self.n_images, P), -1, dtype=torch.int32, device="cuda")   # the row of image m that shows point p
            first = np.concatenate([[0], np.cumsum(sizes)])
            for m in range(self.n_images):
                pts = torch.randperm(P, device="cuda", generator=g)[:int(sizes[m])]
                point[int(first[m]):int(first[m + 1])] = pts
                where[m, pts] = torch.arange(int(sizes[m]), dtype=torch.int32, device="cuda")
            self.match = where[image_b, point[row_a]].contiguous()
        else:
            j = (torch.rand((self.cap,), device="cuda", generator=g) * d_sizes[image_b]).long().clamp_(max=int(sizes.max()) - 1)
            linked = torch.rand((self.cap,), device="cuda", generator=g) < LINKED
            self.match = torch.where(linked & (j < d_sizes[image_b]), j, torch.full_like(j, -1)).int().contiguous()
        self.track = torch.empty((self.total,), dtype=torch.int32, device="cuda")
        self.len = torch.empty((self.total,), dtype=torch.int32, device="cuda")
        self.dup = torch.empty((self.total,), dtype=torch.int32, device="cuda")

    def call(self, h, stream, stats, n_edges=None, length=True, dup=True):
        h.build_tracks_device(self.o.data_ptr(), self.n_images, self.total, self.ea.data_ptr(), self.eb.data_ptr(), self.la.data_ptr(),
                              self.cap, self.n_edges if n_edges is None else n_edges, self.match.data_ptr(), self.track.data_ptr(),
                              self.len.data_ptr() if stats and length else None, self.dup.data_ptr() if stats and dup else None, 0,
                              stream)

    def host(self):
        """labels by the route without the call: everything it needs copied to the host first"""
        match, la = self.match.cpu().numpy(), self.la.cpu().numpy()
        o, ea, eb = self.o.cpu().numpy(), self.ea.cpu().numpy(), self.eb.cpu().numpy()
        if HOST.startswith("numpy"):
            return tracks_cases.build_tracks(o, self.total, ea, eb, la.astype(np.uint64), len(match), match)[0]
        rows = np.diff(o)
        e_of = np.repeat(np.arange(len(ea)), np.diff(la))
        r = np.arange(len(match)) - la[e_of]
        ok = (match >= 0) & (match < rows[eb][e_of])
        u, v = (o[ea][e_of] + r)[ok], (o[eb][e_of] + match)[ok]
        graph = coo_matrix((np.ones(len(u), np.int8), (u, v)), shape=(self.total, self.total))
        _, comp = connected_components(graph, directed=False)
        _, first = np.unique(comp, return_index=True)                           # a component's first row is its smallest
        return first[comp].astype(np.int32)


def time_case(h, c, stream):
    c.call(h, stream, True)
    torch.cuda.synchronize()
    want = c.host()
    assert np.array_equal(c.track.cpu().numpy(), want), "the call and the host route disagree"
    length, dup = c.len.cpu().numpy(), c.dup.cpu().numpy()
    assert np.array_equal(length, np.bincount(want, minlength=c.total)), "the lengths are not the labels' counts"
    t = timed({"tracks": lambda: c.call(h, stream, False), "tracks_stats": lambda: c.call(h, stream, True),
               "no_edges": lambda: c.call(h, stream, False, n_edges=0), "tracks_len": lambda: c.call(h, stream, True, dup=False),
               "tracks_dup": lambda: c.call(h, stream, True, length=False)})
    host = []
    for it in range(HOST_WARMUP + HOST_TIMED):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c.host()
        if it >= HOST_WARMUP:
            host.append((time.perf_counter() - t0) * 1e6)
    host.sort()
    med = lambda k: t[k]["median_us"]
    return {"images": c.n_images, "edges": c.n_edges, "pool_rows": c.total, "layout_entries": c.cap,
            "links": int(((c.match >= 0)).sum()), "tracks_of_2_or_more": int((length >= 2).sum()), "longest": int(length.max()),
            "conflicting_rows": int(dup.sum()),
            **{k + "_" + f: v[f] for k, v in t.items() for f in v},
            "link_launch_us": round(med("tracks") - med("no_edges"), 2), "statistics_launches_us": round(med("tracks_stats") - med("tracks"), 2),
            "host_route": HOST, "host_median_us": round(statistics.median(host), 1), "host_min_us": round(host[0], 1),
            "host_max_us": round(host[-1], 1), "host_over_tracks": round(statistics.median(host) / med("tracks"), 1),
            "host_over_tracks_stats": round(statistics.median(host) / med("tracks_stats"), 1), "warmup": WARMUP, "timed": TIMED,
            "host_rounds": HOST_TIMED}


def main():
    torch.cuda.init()
    torch.cuda.set_stream(torch.cuda.Stream())
    s = torch.cuda.current_stream().cuda_stream
    h = lfp.MkdHandle(max_features=64)
    g = np.random.default_rng(0)
    sizes = g.integers(1800, 2201, 64)
    i, j = np.triu_indices(64, 1)
    for scene in (True, False):
        c = Case(h, sizes, list(zip(i.tolist(), j.tolist())), 1, s, scene=scene)
        print(json.dumps({"bench": "build_tracks", "case": "all_pairs_64x2000", "matches": "scene" if scene else "random",
                          **time_case(h, c, s)}), flush=True)
        del c
    c = Case(h, np.concatenate([[2000], g.integers(1800, 2201, 1024)]), [(0, k) for k in range(1, 1025)], 2, s)
    print(json.dumps({"bench": "build_tracks", "case": "query_2000_x_1024_images", "matches": "scene", **time_case(h, c, s)}), flush=True)
    del c
    pairs = [(t, t + d) for d in range(1, 5) for t in range(256 - d)]
    c = Case(h, g.integers(450, 551, 256), pairs, 4, s)
    print(json.dumps({"bench": "build_tracks", "case": "window4_256x500", "matches": "scene", **time_case(h, c, s)}), flush=True)


if __name__ == "__main__":
    main()
