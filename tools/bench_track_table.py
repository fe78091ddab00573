#!/usr/bin/env python3
"""Device time of lf_mkd_track_table_device (the CSR table of the tracks lf_mkd_build_tracks_device labelled) and of
lf_mkd_gather_track_rows_device against the only route there was before them, on the same device tensors in one process:

    table         the call with every output (offsets, rows, images, row_track, counts)
    select_keys   the call with obs_capacity = 0: its first four launches alone (select, scan, apply, keys), so that
                  table - select_keys is the radix passes and the finalise launch
    gather        lf_mkd_gather_track_rows_device over the keypoints (20-byte rows)
    build_tracks  lf_mkd_build_tracks_device with both statistics on the same case: what made the arrays
    torch         the route without the call: torch.nonzero of the selected mask, cumsum of the lengths, the label -> index map,
                  torch.nonzero of the member rows, a stable torch.sort of their table indices, index_select of the keypoints.
                  torch.nonzero's result has a dynamic size, so the route synchronises twice; timed with HIP events like the
                  others, and once more as wall clock from a synchronised start to a synchronised end

The device forms alternate call by call, each timed with HIP events -- 5 warm-up and 20 timed rounds; the median is reported,
and the 10th and 90th percentile as the run-to-run spread (the method of bench_tracks.py, whose cases and generators are
imported).  Before timing, the call's table and gathered keypoints are compared with the torch route's: they must be equal.

Cases, bench_tracks.py's four: 64 images of about 2000 rows with all 2016 pairs ("scene" matches, and "random" ones that tie
all rows into ONE track), one query against 1024 images, 256 frames with window 4; each at min_len 2 with
LF_MKD_TRACK_TABLE_CONSISTENT and at min_len 1 without the flag.  Prints one JSON line per case and configuration with the
times in microseconds.

--trace CASE: only that case (0 .. 3), 20 plain calls per configuration and nothing else, for a per-kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/bench_track_table.py --trace 0): the share of every launch group.
LF_MKD_LIB selects a build of another digit width or block size (-DLF_MKD_TT_DIGIT_BITS, -DLF_MKD_TT_BLOCK_ROWS).
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

CONFIGS = ((2, True), (1, False))


class Table:
    """the outputs of the call for one case, at the capacities that always suffice"""

    def __init__(self, c, min_len):
        n = c.total
        self.t_cap, self.o_cap = n // min_len, n
        i32 = lambda k: torch.empty((k,), dtype=torch.int32, device="cuda")
        self.offsets = torch.empty((self.t_cap + 1,), dtype=torch.int64, device="cuda")
        self.rows, self.images, self.row_track, self.counts = i32(n), i32(n), i32(n), i32(4)
        self.kps = torch.zeros((n, 5), dtype=torch.float32, device="cuda")


def call_table(h, c, t, min_len, consistent, stream, o_cap=None):
    h.track_table_device(c.o.data_ptr(), c.n_images, c.total, c.track.data_ptr(), c.len.data_ptr(), c.dup.data_ptr(), min_len,
                         lfp.TRACK_TABLE_CONSISTENT if consistent else 0, t.t_cap, t.o_cap if o_cap is None else o_cap,
                         t.offsets.data_ptr(), t.rows.data_ptr(), t.images.data_ptr(), t.row_track.data_ptr(), t.counts.data_ptr(), stream)


def call_gather(h, c, t, kps, stream):
    h.gather_track_rows_device(kps.data_ptr(), 20, c.total, t.rows.data_ptr(), t.counts.data_ptr(), t.o_cap, t.kps.data_ptr(), stream)


def torch_route(c, kps, min_len, consistent):
    """(offsets, rows, row_track, gathered keypoints) with torch alone; waits for the device twice (the two nonzero calls)"""
    n = c.total
    at = torch.arange(n, device="cuda", dtype=torch.int32)
    sel = (c.track == at) & (c.len >= min_len)
    if consistent:
        sel &= c.dup == 0
    labels = torch.nonzero(sel).reshape(-1)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(c.len[labels].long(), 0)])
    index = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    index[labels] = torch.arange(labels.numel(), device="cuda", dtype=torch.int32)
    row_track = index[c.track.long()]
    rows = torch.nonzero(row_track >= 0).reshape(-1)
    order = torch.sort(row_track[rows], stable=True).indices
    rows = rows[order]
    return offsets, rows, row_track, torch.index_select(kps, 0, rows)


def time_case(h, c, stream, min_len, consistent):
    kps = torch.rand((c.total, 5), device="cuda")
    c.call(h, stream, True)
    t = Table(c, min_len)
    call_table(h, c, t, min_len, consistent, stream)
    call_gather(h, c, t, kps, stream)
    torch.cuda.synchronize()
    offsets, rows, row_track, kt = torch_route(c, kps, min_len, consistent)
    n_tracks, n_obs = (int(x) for x in t.counts[:2].cpu())
    assert n_tracks == offsets.numel() - 1 and n_obs == rows.numel(), "the call and the torch route disagree on the counts"
    assert torch.equal(t.offsets[:n_tracks + 1], offsets) and torch.equal(t.rows[:n_obs].long(), rows), "the tables differ"
    assert torch.equal(t.row_track, row_track) and torch.equal(t.kps[:n_obs], kt), "row_track or the gathered keypoints differ"
    lengths = torch.diff(offsets)
    r = timed({"table": lambda: call_table(h, c, t, min_len, consistent, stream),
               "select_keys": lambda: call_table(h, c, t, min_len, consistent, stream, o_cap=0),
               "gather": lambda: call_gather(h, c, t, kps, stream),
               "build_tracks": lambda: c.call(h, stream, True),
               "torch": lambda: torch_route(c, kps, min_len, consistent)})
    call_table(h, c, t, min_len, consistent, stream)                         # (select_keys left the counts of capacity 0)
    wall = []
    for it in range(WARMUP + TIMED):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch_route(c, kps, min_len, consistent)
        torch.cuda.synchronize()
        if it >= WARMUP:
            wall.append((time.perf_counter() - t0) * 1e6)
    wall.sort()
    med = lambda k: r[k]["median_us"]
    bits, passes, block, scratch = lfp.track_table_plan(c.total, min_len)
    return {"pool_rows": c.total, "min_len": min_len, "consistent": consistent, "tracks": n_tracks, "observations": n_obs,
            "longest": int(lengths.max()) if n_tracks else 0, "key_bits": bits, "passes": passes, "block_rows": block,
            "scratch_bytes": scratch, **{k + "_" + f: v[f] for k, v in r.items() for f in v},
            "sort_and_finalise_us": round(med("table") - med("select_keys"), 2),
            "torch_wall_median_us": round(statistics.median(wall), 1), "torch_wall_p10_us": round(wall[len(wall) // 10], 1),
            "torch_wall_p90_us": round(wall[len(wall) - 1 - len(wall) // 10], 1),
            "torch_over_table_and_gather": round(med("torch") / (med("table") + med("gather")), 2),
            "torch_wall_over_table_and_gather": round(statistics.median(wall) / (med("table") + med("gather")), 2),
            "table_over_build_tracks": round(med("table") / med("build_tracks"), 2), "warmup": WARMUP, "timed": TIMED,
            "lib": os.path.basename(lfp.LIB_PATH)}


def make_case(k, h, s):
    g = np.random.default_rng(0)
    sizes = g.integers(1800, 2201, 64)
    i, j = np.triu_indices(64, 1)
    query = np.concatenate([[2000], g.integers(1800, 2201, 1024)])
    frames = g.integers(450, 551, 256)
    if k == 0:
        return "all_pairs_64x2000", "scene", Case(h, sizes, list(zip(i.tolist(), j.tolist())), 1, s, scene=True)
    if k == 1:
        return "all_pairs_64x2000", "random", Case(h, sizes, list(zip(i.tolist(), j.tolist())), 1, s, scene=False)
    if k == 2:
        return "query_2000_x_1024_images", "scene", Case(h, query, [(0, k) for k in range(1, 1025)], 2, s)
    return "window4_256x500", "scene", Case(h, frames, [(t, t + d) for d in range(1, 5) for t in range(256 - d)], 4, s)


def main():
    torch.cuda.init()
    torch.cuda.set_stream(torch.cuda.Stream())
    s = torch.cuda.current_stream().cuda_stream
    h = lfp.MkdHandle(max_features=64)
    args = sys.argv[1:]
    if "--trace" in args:
        name, matches, c = make_case(int(args[args.index("--trace") + 1]), h, s)
        c.call(h, s, True)
        for min_len, consistent in CONFIGS:
            t = Table(c, min_len)
            for _ in range(20):
                call_table(h, c, t, min_len, consistent, s)
        torch.cuda.synchronize()
        print(json.dumps({"bench": "track_table trace", "case": name, "matches": matches, "calls": 20}))
        return
    only = [int(a) for a in args if a.isdigit()] or range(4)
    for k in only:
        name, matches, c = make_case(k, h, s)
        for min_len, consistent in CONFIGS:
            print(json.dumps({"bench": "track_table", "case": name, "matches": matches, **time_case(h, c, s, min_len, consistent)}),
                  flush=True)
        del c


if __name__ == "__main__":
    main()
