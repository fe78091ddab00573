#!/usr/bin/env python3
"""Device time of lf_mkd_link_table_device (the CSR table of the links an edge list's match array holds, the per-edge counts and
the pruned match array) against the only route there was before it, on the same device tensors in one process:

    table         the call with every output (offsets, link_a, link_b, link_edge, edge_links, match_kept, counts)
    kept_only     the call with d_match_kept alone (link_capacity = 0, no link arrays): what a caller that only prunes pays
    count_scan    the call with link_capacity = 0 and no d_match_kept: every launch but the scatter
    gather        lf_mkd_gather_track_rows_device over the keypoints (20-byte rows), once: a caller runs it per side
    torch         the route without the call: searchsorted for the edge of an entry, a gather of both images' bounds, the link
                  mask, bincount + cumsum for the counts and offsets, torch.nonzero of the kept links and three gathers, and
                  torch.where for the pruned array.  torch.nonzero's result has a dynamic size, so the route synchronises;
                  timed with HIP events like the others, and once more as wall clock from a synchronised start to a
                  synchronised end

The device forms alternate call by call, each timed with HIP events -- 5 warm-up and 20 timed rounds; the median is reported,
and the 10th and 90th percentile as the run-to-run spread (the method of bench_tracks.py, whose cases and `timed` are imported).
Before timing, every output of the call is compared with the torch route's: they must be equal.

Cases: 64 images of about 2000 rows with all 2016 pairs, one query against 1024 images, 256 frames with window 4; each at
min_links 0 and at min_links 800 / 800 / 200 (0.4 of an image's mean rows: most edges are dropped).  Prints one JSON line per case and
configuration with the times in microseconds.

--trace CASE: only that case (0 .. 2), 20 plain calls per configuration and nothing else, for a per-kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/bench_link_table.py --trace 0): the share of every launch.
LF_MKD_LIB selects a build of another scan fan-out (-DLF_MKD_LT_SCAN_FANOUT).
Development aid; bench.py is the contract for the headline metric."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-features_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import local_features_python as lfp  # noqa: E402
from bench_tracks import Case, TIMED, WARMUP, timed  # noqa: E402


class Table:
    """the outputs of the call for one case, at the capacity that always suffices"""

    def __init__(self, c):
        i32 = lambda k: torch.empty((k,), dtype=torch.int32, device="cuda")
        self.l_cap = c.cap
        self.offsets = torch.empty((c.n_edges + 1,), dtype=torch.int64, device="cuda")
        self.a, self.b, self.edge, self.links, self.kept, self.counts = i32(c.cap), i32(c.cap), i32(c.cap), i32(c.n_edges), i32(c.cap), i32(4)
        self.kps = torch.zeros((c.cap, 5), dtype=torch.float32, device="cuda")


def call_table(h, c, t, min_links, stream, form="table"):
    full = form == "table"
    p = lambda x: x.data_ptr() if full else None
    h.link_table_device(c.o.data_ptr(), c.n_images, c.total, c.ea.data_ptr(), c.eb.data_ptr(), c.la.data_ptr(), c.cap, c.n_edges,
                        c.match.data_ptr(), min_links, 0, t.l_cap if full else 0, t.offsets.data_ptr(), p(t.a), p(t.b), p(t.edge),
                        p(t.links), t.kept.data_ptr() if form != "count_scan" else None, t.counts.data_ptr(), stream)


def call_gather(h, c, t, kps, stream):
    h.gather_track_rows_device(kps.data_ptr(), 20, c.total, t.a.data_ptr(), t.counts.data_ptr(), t.l_cap, t.kps.data_ptr(), stream)


def torch_route(c, min_links):
    """(offsets, link_a, link_b, link_edge, edge_links, match_kept) with torch alone; waits for the device once (nonzero)"""
    at = torch.arange(c.cap, device="cuda")
    e_of = torch.searchsorted(c.la, at, right=True) - 1
    r = at - c.la[e_of]
    first_a, first_b = c.o[c.ea.long()][e_of], c.o[c.eb.long()][e_of]
    nb = c.o[c.eb.long() + 1][e_of] - first_b
    mask = (c.match >= 0) & (c.match < nb)
    links = torch.bincount(e_of[mask], minlength=c.n_edges)
    sel = links >= min_links
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(torch.where(sel, links, 0), 0)])
    keep = mask & sel[e_of]
    idx = torch.nonzero(keep).reshape(-1)
    return (offsets, (first_a + r)[idx], first_b[idx] + c.match[idx], e_of[idx], links,
            torch.where(keep, c.match, torch.full_like(c.match, -1)))


def time_case(h, c, stream, min_links):
    kps = torch.rand((c.total, 5), device="cuda")
    t = Table(c)
    call_table(h, c, t, min_links, stream)
    call_gather(h, c, t, kps, stream)
    torch.cuda.synchronize()
    offsets, a, b, e, links, kept = torch_route(c, min_links)
    n_kept, n_links = (int(x) for x in t.counts[:2].cpu())
    assert n_links == a.numel() and n_kept == int((links >= min_links).sum()), "the call and the torch route disagree on the counts"
    assert torch.equal(t.offsets, offsets) and torch.equal(t.links.long(), links), "the offsets or the per-edge counts differ"
    assert torch.equal(t.a[:n_links].long(), a) and torch.equal(t.b[:n_links].long(), b) and torch.equal(t.edge[:n_links].long(), e), \
        "the tables differ"
    assert torch.equal(t.kept, kept) and torch.equal(t.kps[:n_links], kps[a]), "match_kept or the gathered keypoints differ"
    r = timed({"table": lambda: call_table(h, c, t, min_links, stream),
               "kept_only": lambda: call_table(h, c, t, min_links, stream, "kept_only"),
               "count_scan": lambda: call_table(h, c, t, min_links, stream, "count_scan"),
               "gather": lambda: call_gather(h, c, t, kps, stream),
               "torch": lambda: torch_route(c, min_links)})
    call_table(h, c, t, min_links, stream)                                     # (the other forms left the counts of capacity 0)
    wall = []
    for it in range(WARMUP + TIMED):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch_route(c, min_links)
        torch.cuda.synchronize()
        if it >= WARMUP:
            wall.append((time.perf_counter() - t0) * 1e6)
    wall.sort()
    med = lambda k: r[k]["median_us"]
    slot, slots, fan, levels, scratch = lfp.link_table_plan(c.cap, c.n_edges)
    return {"pool_rows": c.total, "entries": c.cap, "edges": c.n_edges, "min_links": min_links, "kept_edges": n_kept, "links": n_links,
            "slot_entries": slot, "slots": slots, "scan_fanout": fan, "scan_levels": levels, "scratch_bytes": scratch,
            **{k + "_" + f: v[f] for k, v in r.items() for f in v},
            "scatter_us": round(med("table") - med("count_scan"), 2),
            "torch_wall_median_us": round(statistics.median(wall), 1), "torch_wall_p10_us": round(wall[len(wall) // 10], 1),
            "torch_wall_p90_us": round(wall[len(wall) - 1 - len(wall) // 10], 1),
            "torch_over_table": round(med("torch") / med("table"), 2),
            "torch_wall_over_table": round(statistics.median(wall) / med("table"), 2), "warmup": WARMUP, "timed": TIMED,
            "lib": os.path.basename(lfp.LIB_PATH)}


def make_case(k, h, s):
    g = np.random.default_rng(0)
    sizes = g.integers(1800, 2201, 64)
    i, j = np.triu_indices(64, 1)
    query = np.concatenate([[2000], g.integers(1800, 2201, 1024)])
    frames = g.integers(450, 551, 256)
    if k == 0:
        return "all_pairs_64x2000", (0, 800), Case(h, sizes, list(zip(i.tolist(), j.tolist())), 1, s, scene=True)
    if k == 1:
        return "query_2000_x_1024_images", (0, 800), Case(h, query, [(0, k) for k in range(1, 1025)], 2, s)
    return "window4_256x500", (0, 200), Case(h, frames, [(t, t + d) for d in range(1, 5) for t in range(256 - d)], 4, s)


def main():
    torch.cuda.init()
    torch.cuda.set_stream(torch.cuda.Stream())
    s = torch.cuda.current_stream().cuda_stream
    h = lfp.MkdHandle(max_features=64)
    args = sys.argv[1:]
    if "--trace" in args:
        name, configs, c = make_case(int(args[args.index("--trace") + 1]), h, s)
        t = Table(c)
        for min_links in configs:
            for _ in range(20):
                call_table(h, c, t, min_links, s)
        torch.cuda.synchronize()
        print(json.dumps({"bench": "link_table trace", "case": name, "calls": 20}))
        return
    only = [int(a) for a in args if a.isdigit()] or range(3)
    for k in only:
        name, configs, c = make_case(k, h, s)
        for min_links in configs:
            print(json.dumps({"bench": "link_table", "case": name, **time_case(h, c, s, min_links)}), flush=True)
        del c


if __name__ == "__main__":
    main()
