#!/usr/bin/env python3
"""Device time of lf_mkd_covisibility_device (per pair of images the tracks of a track table that both see) beside the routes
there were before it, on tables the real calls make on synthetic links and on two adversarial tables written in numpy.

Cases (bench_track_table.py's, its generators are imported):
  0  64 images of about 2000 rows, all 2016 pairs
  1  one query of 2000 rows against 1024 images
  2  256 frames of about 500 rows, window 4
each through lf_mkd_build_tracks_device and lf_mkd_track_table_device at min_len 2 with LF_MKD_TRACK_TABLE_CONSISTENT and at
min_len 1 without, and
  3  4 images, 10^6 tracks of length 2 .. 4 (contention: every add lands on 16 words)
  4  256 images, 4096 tracks of length 256 (pair-bound: 268 M adds)

Timed, alternating call by call, HIP events, 5 warm-up + 20 timed rounds, medians with the 10th and 90th percentile:
  covisibility   the whole call (zero, both counting launches), no mask
  masked         the call with the case's edge list as the mask (cases 0 .. 2)
  torch_dense    the route with torch alone on the same tensors: the track of every observation (repeat_interleave on the
                 lengths, which WAITS for the device), a dense [tracks][images] f32 incidence matrix, B.T @ B; exact below 2^24
  torch_sparse   the same with a sparse COO incidence matrix and torch.sparse.mm, where this torch has it
and wall clock, 1 + 5 rounds:
  host           the arrays copied to the host, scipy.sparse B.T @ B (numpy add.at on a dense table without scipy)
A route that cannot allocate or fails is reported as null with the reason.  Checks the call against the dense route (or the
host route) for equality first.  One JSON line per case and configuration.

--curve: the contention curve -- 10^6 tracks of length 2 .. 4 over 2, 4, 8, 16, 32, 64, 128 images; run it once with the
library as built and once with a build of -DLF_COVIS_LDS_IMAGES=0 (LF_MKD_LIB selects it) to see where counting in LDS first
stops paying.  Development aid; bench.py is the contract for the headline metric."""
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
from bench_tracks import TIMED, WARMUP, timed  # noqa: E402
from bench_track_table import Table, call_table, make_case  # noqa: E402

try:
    from scipy.sparse import csr_matrix
    HOST = "scipy.sparse"
except ImportError:
    HOST = "numpy add.at"

SCENES = (0, 2, 3)               # bench_track_table.make_case's scene cases
CONFIGS = ((2, True), (1, False))


class Tab:
    """a track table on the device: offsets int64 [t_cap + 1], images int32 [o_cap], counts int32 [4], n images"""

    def __init__(self, offsets, images, counts, n, t_cap, o_cap):
        self.offsets, self.images, self.counts, self.n, self.t_cap, self.o_cap = offsets, images, counts, n, t_cap, o_cap
        self.covis = torch.empty((n, n), dtype=torch.int32, device="cuda")
        self.T, self.O = (int(x) for x in counts[:2].cpu())


def synthetic(n, lengths, seed):
    """consistent tracks of the given lengths over n images, written directly"""
    g = np.random.default_rng(seed)
    lengths = np.asarray(lengths, np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    if (lengths == n).all():
        images = np.tile(np.arange(n, dtype=np.int32), len(lengths))
    else:                                                                        # a random start and ascending steps within n
        start = g.integers(0, n - lengths + 1)
        images = (np.repeat(start, lengths) + np.arange(offsets[-1]) - np.repeat(offsets[:-1], lengths)).astype(np.int32)
    counts = np.array([len(lengths), offsets[-1], len(lengths), offsets[-1]], np.int64).astype(np.int32)
    return Tab(torch.from_numpy(offsets).cuda(), torch.from_numpy(images).cuda(), torch.from_numpy(counts).cuda(), n, len(lengths),
               int(offsets[-1]))


def call(h, t, stream, edges=None, flags=0):
    ea, eb = edges if edges is not None else (None, None)
    h.covisibility_device(t.offsets.data_ptr(), t.t_cap, t.images.data_ptr(), t.o_cap, t.counts.data_ptr(), t.n,
                          ea.data_ptr() if ea is not None else None, eb.data_ptr() if eb is not None else None,
                          ea.numel() if ea is not None else 0, flags, t.covis.data_ptr(), stream)


def incidence(t):
    """(track of every observation, its image): repeat_interleave reads the lengths back"""
    lengths = torch.diff(t.offsets[:t.T + 1])
    return torch.repeat_interleave(torch.arange(t.T, device="cuda"), lengths), t.images[:t.O].long()


def torch_dense(t):
    rows, cols = incidence(t)
    B = torch.zeros((t.T, t.n), dtype=torch.float32, device="cuda")
    B[rows, cols] = 1.0
    return (B.T @ B).to(torch.int32)


def torch_sparse(t):
    rows, cols = incidence(t)
    B = torch.sparse_coo_tensor(torch.stack([rows, cols]), torch.ones(rows.numel(), device="cuda"), (t.T, t.n)).coalesce()
    B = torch.sparse_coo_tensor(B.indices(), torch.ones_like(B.values()), B.shape)      # (a repeated image counts once)
    return torch.sparse.mm(B.t(), B).to_dense().to(torch.int32)


def host(t):
    offsets, images = t.offsets.cpu().numpy(), t.images.cpu().numpy()
    T, O = (int(x) for x in t.counts[:2].cpu().numpy())
    rows = np.repeat(np.arange(T), np.diff(offsets[:T + 1]))
    if HOST == "scipy.sparse":
        B = csr_matrix((np.ones(O, np.int64), (rows, images[:O])), shape=(T, t.n))
        B.data[:] = 1
        return np.asarray((B.T @ B).todense()).astype(np.int32)
    B = np.zeros((T, t.n), np.int64)
    B[rows, images[:O]] = 1
    return (B.T @ B).astype(np.int32)


def attempt(fn):
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, None
    except Exception as e:                                                       # out of memory, or a torch without the operator
        torch.cuda.empty_cache()
        return None, type(e).__name__ + ": " + str(e).splitlines()[0][:120]


def wall_clock(fn, warmup, rounds):
    out = []
    for it in range(warmup + rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if it >= warmup:
            out.append((time.perf_counter() - t0) * 1e6)
    return round(statistics.median(out), 1)


def time_tab(h, t, stream, edges=None, host_route=True):
    call(h, t, stream)
    torch.cuda.synchronize()
    got = t.covis.clone()
    dense, why_dense = attempt(lambda: torch_dense(t)) if t.T * t.n * 4 <= 64 << 30 else (None, "dense incidence matrix above 64 GiB")
    sparse, why_sparse = attempt(lambda: torch_sparse(t))
    ref = dense if dense is not None else sparse if sparse is not None else torch.from_numpy(host(t)).cuda()
    assert torch.equal(got, ref), "the call and the other route disagree"
    del ref
    calls = {"covisibility": lambda: call(h, t, stream)}
    if edges is not None:
        calls["masked"] = lambda: call(h, t, stream, edges)
    if dense is not None:
        calls["torch_dense"] = lambda: torch_dense(t)
    if sparse is not None:
        calls["torch_sparse"] = lambda: torch_sparse(t)
    del dense, sparse
    r = timed(calls)
    out = {"images": t.n, "tracks": t.T, "observations": t.O, "pairs_added": int(got.long().sum()),
           "longest": int(torch.diff(t.offsets[:t.T + 1]).max()) if t.T else 0}
    form, groups, launches, scratch = lfp.covisibility_plan(t.n, t.t_cap, t.o_cap, 0 if edges is None else edges[0].numel())
    out.update({"form_lanes": form & 255, "form_lds": bool(form & lfp.COVIS_FORM_LDS), "workgroups": groups, "launches": launches,
                "scratch_bytes": scratch})
    out.update({k + "_" + f: v[f] for k, v in r.items() for f in v})
    out["torch_dense_skipped"], out["torch_sparse_skipped"] = why_dense, why_sparse
    for k in ("torch_dense", "torch_sparse"):
        if k in calls:
            out[k + "_wall_us"] = wall_clock(calls[k], WARMUP, TIMED)
            out[k + "_over_call"] = round(r[k]["median_us"] / r["covisibility"]["median_us"], 2)
    if host_route:
        out["host"] = HOST
        out["host_wall_us"] = wall_clock(lambda: host(t), 1, 5)
        out["host_over_call"] = round(out["host_wall_us"] / r["covisibility"]["median_us"], 1)
    out.update({"warmup": WARMUP, "timed": TIMED, "lib": os.path.basename(lfp.LIB_PATH)})
    return out


def scene_tab(h, c, stream, min_len, consistent):
    c.call(h, stream, True)
    t = Table(c, min_len)
    call_table(h, c, t, min_len, consistent, stream)
    torch.cuda.synchronize()
    return Tab(t.offsets, t.images, t.counts, c.n_images, t.t_cap, t.o_cap)


def main():
    torch.cuda.init()
    torch.cuda.set_stream(torch.cuda.Stream())
    s = torch.cuda.current_stream().cuda_stream
    h = lfp.MkdHandle(max_features=64)
    args = sys.argv[1:]
    g = np.random.default_rng(1)
    if "--curve" in args:
        for n in (2, 4, 8, 16, 32, 64, 128):
            t = synthetic(n, np.minimum(g.integers(2, 5, 10 ** 6), n), n)
            call(h, t, s)
            r = timed({"covisibility": lambda: call(h, t, s)})["covisibility"]
            form = lfp.covisibility_plan(t.n, t.t_cap, t.o_cap)[0]
            print(json.dumps({"bench": "covisibility curve", "images": n, "tracks": t.T, "form_lanes": form & 255,
                              "form_lds": bool(form & lfp.COVIS_FORM_LDS), **r, "lib": os.path.basename(lfp.LIB_PATH)}), flush=True)
        return
    only = [int(a) for a in args if a.isdigit()] or range(5)
    for k in only:
        if k < 3:
            name, matches, c = make_case(SCENES[k], h, s)
            for min_len, consistent in CONFIGS:
                t = scene_tab(h, c, s, min_len, consistent)
                print(json.dumps({"bench": "covisibility", "case": name, "min_len": min_len, "consistent": consistent,
                                  **time_tab(h, t, s, edges=(c.ea, c.eb))}), flush=True)
                del t
            del c
        elif k == 3:
            t = synthetic(4, g.integers(2, 5, 10 ** 6), 3)
            print(json.dumps({"bench": "covisibility", "case": "contention_4_images_1M_tracks", **time_tab(h, t, s)}), flush=True)
        else:
            t = synthetic(256, np.full(4096, 256), 4)
            print(json.dumps({"bench": "covisibility", "case": "pair_bound_256_images_4096x256", **time_tab(h, t, s)}), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
