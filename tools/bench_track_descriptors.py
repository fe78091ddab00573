#!/usr/bin/env python3
"""Device time of lf_mkd_track_descriptors_device (per track one 8-bit row from its observations' pool rows) and of
LocalFeatures.localize, each beside the route a user had before them, on the same tensors and named as what it is:

    desc            the call without d_desc_stats, captured once in a graph and replayed (8 lanes a track: the product)
    desc_stats      the same with d_desc_stats (the second walk over the rows)
    lanes_4 / lanes_16   `desc` at the other group widths (LF_MKD_TRACK_DESC_LANES at capture)
    desc_direct     `desc` enqueued directly, no graph
    torch           the torch route: index_select of the observations' rows, an int32 index_add_ per track (the track of
                    every observation is given to it, precomputed), normalise and quantise in f64 -- enqueued directly, as a
                    user would; torch_graph: the same captured and replayed.  It synchronises nowhere; it holds the gathered
                    rows as int32 (obs x 512 bytes) and the sums (tracks x 512 bytes) while it runs.  Its bytes must equal
                    the call's.

Cases (every observation a pool row of its own, scattered over the pool; states all 2 and points all real, both filters on):
64 images of about 2000 rows (40 000 tracks of 2 .. 12); 256 frames with window 4 (30 000 tracks of 2 .. 5); one query against
1024 images (1 300 000 tracks of 2); ONE track of 65 536 observations, the most a track contributes.

`--localize`: 64 query images of about 2000 rows (tests/resect_cases.scene: 0.5 px noise, 30 % wrong keypoints) against a
model of their tracks.  localize = one lf_mkd_match_q8_device against the tracks' rows + one resection; grouped = the route
before it: lf_mkd_match_q8_grouped_device against ALL observation rows (3 a track) with group = track, a torch gather of the
matched row's track, the same resection.  Both directly enqueued; resident bytes of each route's model are reported.

The forms alternate call by call, each timed with HIP events -- 5 warm-up and 20 timed rounds; the median is reported, and
the 10th and 90th percentile as the run-to-run spread (bench_tracks.py's `timed`).  Prints one JSON line per case with the times
in microseconds and a UTC clock stamp.  Development aid; bench.py is the contract for the headline metric."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("local-features_amd", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import local_features_python as lfp  # noqa: E402
import resect_cases  # noqa: E402
from bench_tracks import TIMED, WARMUP, timed  # noqa: E402

SCALE = 256.0


def stamp():
    return time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime())


class Table:
    """tracks of the given lengths over a pool in which every observation is a row of its own, all on the device"""

    def __init__(self, lengths, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        lengths = np.asarray(lengths, np.int64)
        self.T, self.n_obs = len(lengths), int(lengths.sum())
        self.off = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)])).cuda()
        self.row = torch.randperm(self.n_obs, generator=g, device="cuda").int()
        self.q = torch.randint(1, 256, (self.n_obs, 128), generator=g, device="cuda", dtype=torch.uint8)
        self.counts = torch.tensor([self.T, self.n_obs, 0, 0], dtype=torch.int32, device="cuda")
        self.state = torch.full((self.n_obs,), 2, dtype=torch.int32, device="cuda")
        self.points = torch.cat([torch.randn((self.T, 3), generator=g, device="cuda"),
                                 torch.full((self.T, 1), 0.9, device="cuda")], 1).contiguous()
        self.track_of = torch.repeat_interleave(torch.arange(self.T, device="cuda"), torch.from_numpy(lengths).cuda())
        self.desc = torch.empty((self.T, 128), dtype=torch.uint8, device="cuda")
        self.stats = torch.empty((self.T, 2), dtype=torch.int32, device="cuda")


def call(h, t, stream, stats=False):
    h.track_descriptors_device(t.q.data_ptr(), t.n_obs, t.off.data_ptr(), t.T, t.row.data_ptr(), t.n_obs, t.counts.data_ptr(),
                               t.desc.data_ptr(), t.stats.data_ptr() if stats else None, t.state.data_ptr(), 2, t.points.data_ptr(),
                               0.0, SCALE, stream)


def torch_route(t):
    c = t.q.index_select(0, t.row.long()).to(torch.int32) - 128
    S = torch.zeros((t.T, 128), dtype=torch.int32, device="cuda").index_add_(0, t.track_of, c)
    Sd = S.double()
    v = torch.round(Sd * SCALE / Sd.pow(2).sum(1).sqrt()[:, None]).clamp(-127, 127)
    return (torch.nan_to_num(v, nan=0.0) + 128).to(torch.uint8)


def capture(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def time_case(h, t, stream):
    cur = lambda: torch.cuda.current_stream().cuda_stream
    graphs = {"desc": capture(lambda: call(h, t, cur())), "desc_stats": capture(lambda: call(h, t, cur(), True))}
    for lanes in ("4", "16"):
        os.environ["LF_MKD_TRACK_DESC_LANES"] = lanes
        graphs["lanes_" + lanes] = capture(lambda: call(h, t, cur()))
        os.environ.pop("LF_MKD_TRACK_DESC_LANES")
    keep = {}

    def run_torch():
        keep["out"] = torch_route(t)

    graphs["torch_graph"] = capture(run_torch)
    call(h, t, stream)
    torch.cuda.synchronize()
    same = bool(torch.equal(torch_route(t), t.desc))
    forms = {k: g.replay for k, g in graphs.items()}
    forms["desc_direct"] = lambda: call(h, t, stream)
    forms["torch"] = run_torch
    r = timed(forms)
    med = lambda k: r[k]["median_us"]
    return {"tracks": t.T, "observations": t.n_obs, "torch_bytes_equal": same,
            **{k + "_" + f: v[f] for k, v in r.items() for f in v},
            "torch_over_desc": round(med("torch") / med("desc"), 2), "torch_graph_over_desc": round(med("torch_graph") / med("desc"), 2),
            "lanes_4_over_desc": round(med("lanes_4") / med("desc"), 2), "lanes_16_over_desc": round(med("lanes_16") / med("desc"), 2),
            "torch_synchronisations": 0, "torch_temporary_bytes": 512 * (t.n_obs + t.T) + 8 * 128 * t.T * 2,
            "gathered_GB_per_s_desc": round(128e-3 * t.n_obs / med("desc"), 1), "warmup": WARMUP, "timed": TIMED,
            "lib": os.path.basename(lfp.LIB_PATH), "utc": stamp()}


def make_case(k):
    g = np.random.default_rng(0)
    if k == 0:
        return "40k_tracks_2_to_12_views_64_images", Table(g.integers(2, 13, 40000), 1)
    if k == 1:
        return "window4_256_images", Table(g.integers(2, 6, 30000), 3)
    if k == 2:
        return "1300k_tracks_of_2_1025_images", Table(np.full(1300000, 2), 2)
    return "one_track_65536_observations", Table(np.array([65536]), 4)


def localize_case(copies=3, sigma=0.1):
    """64 query images against the model of their tracks; the pool the grouped route needs holds `copies` rows a track"""
    s = resect_cases.scene(1, (1600,) * 64)
    g = np.random.default_rng(5)
    T, n = len(s["points"]), len(s["kps"])
    unit = lambda x: x / np.linalg.norm(x, axis=1)[:, None]
    quant = lambda x: (np.clip(np.rint(x * SCALE), -127, 127) + 128).astype(np.uint8)
    ident = unit(g.normal(size=(T, 128))).astype(np.float32)
    rt = s["row_track"]
    rows = np.where(rt[:, None] >= 0, ident[np.maximum(rt, 0)], 0) + np.where(rt[:, None] >= 0, sigma, 1.0) * g.normal(size=(n, 128))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pool = quant(unit(np.repeat(ident, copies, 0) + sigma * g.normal(size=(copies * T, 128)).astype(np.float32)))
    return dict(q_query=up(quant(unit(rows))), kps=up(s["kps"]), off=up(s["image_offsets"].view(np.int64)),
                model=up(quant(ident)), points=up(s["points"]), counts=up(np.array([T, 0, 0, 0], np.int32)),
                K=up(s["intrinsics"]), pool=up(pool), group=up(np.repeat(np.arange(T, dtype=np.int32), copies)), T=T, rows=n,
                truth=s["truth"])


def time_localize():
    c = localize_case()
    lf = lfp.LocalFeatures(64, 64, 16)
    zero = torch.zeros((64, 12), dtype=torch.float32, device="cuda")
    keep = {}

    def new():
        keep["new"] = lf.localize(c["q_query"], c["kps"], c["off"], c["model"], c["points"], c["counts"], c["K"])

    def grouped():
        m = lf.match_q8_grouped(c["q_query"], c["pool"], c["group"], ratio=0.8)
        row_track = torch.where(m >= 0, c["group"][m.clamp(min=0).long()], torch.full_like(m, -1))
        keep["grouped"] = lf.resect_cameras(c["kps"], c["off"], row_track, c["points"], c["counts"], c["K"], zero)

    def match_only():
        keep["match"] = torch.empty((c["rows"],), dtype=torch.int32, device="cuda")
        lf._inner.match_q8_device(c["q_query"].data_ptr(), c["rows"], c["model"].data_ptr(), c["T"], keep["match"].data_ptr(), 0.8,
                                  stream=torch.cuda.current_stream().cuda_stream)

    for fn in (new, grouped, match_only):
        fn()
    torch.cuda.synchronize()
    r = timed({"localize": new, "grouped_route": grouped, "localize_match_alone": match_only})
    posed = lambda st: int((st.cpu().numpy()[:, 2] == 0).sum())
    pool_rows = c["pool"].shape[0]
    return {"query_images": 64, "query_rows": c["rows"], "tracks": c["T"], "pool_rows": pool_rows,
            **{k + "_" + f: v[f] for k, v in r.items() for f in v},
            "grouped_over_localize": round(r["grouped_route"]["median_us"] / r["localize"]["median_us"], 2),
            "posed_localize": posed(keep["new"][1]), "posed_grouped": posed(keep["grouped"][1]),
            "resident_bytes_localize": c["T"] * (128 + 16), "resident_bytes_grouped": pool_rows * (128 + 4) + c["T"] * 16,
            "warmup": WARMUP, "timed": TIMED, "lib": os.path.basename(lfp.LIB_PATH), "utc": stamp()}


def main():
    torch.cuda.init()
    torch.cuda.set_stream(torch.cuda.Stream())
    s = torch.cuda.current_stream().cuda_stream
    args = sys.argv[1:]
    if "--localize" in args:
        print(json.dumps({"bench": "localize", **time_localize()}), flush=True)
        return
    h = lfp.MkdHandle(max_features=64)
    for k in [int(a) for a in args if a.isdigit()] or range(4):
        name, t = make_case(k)
        print(json.dumps({"bench": "track_descriptors", "case": name, **time_case(h, t, s)}), flush=True)


if __name__ == "__main__":
    main()
