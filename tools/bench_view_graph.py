#!/usr/bin/env python3
"""Device time of lf_mkd_view_graph_device (the triangle vote over posed edges, global rotations by a tree and quaternion
averaging, residuals) against the routes there are beside it, on the same device tensors in one process:

    graph         the warmed-up call captured once in a hipGraph and replayed (what a pipeline that records its chain pays)
    call          the call's plain launches (5 + tree_rounds + iterations of them, each about 6.5 us of launch cost)
    torch_vote    the vote alone without the call, f64: Shepperd's quaternions batched, a dense [n][n][4] table of the pairs'
                  quaternions and a [n][n] mask, then per block of 4096 edges the loop products against every third image
                  batched and the two counts as masked sums; HIP events like the others
    twin          the host twin (tests/cpp/view_graph_twin.cpp, the kernels' own math header under g++ -O2) on one host core,
                  the whole call: wall clock of the program on a call file, 1 warm-up + 3 timed runs (file I/O included)

The device forms alternate call by call, each timed with HIP events -- 5 warm-up and 20 timed rounds; the median is reported,
and the 10th and 90th percentile as the run-to-run spread (bench_tracks.py's `timed`).  Before timing, the call's closed and
consistent counts must equal the torch route's and every output word the twin's.

Cases: random camera rotations, relative rotations with 0.5 degrees of noise, 10 % of the edges wrong by 10 .. 180 degrees:
64 images with all 2016 pairs, 1024 images with 32 picks each, 256 frames with window 4.  Prints one JSON line per case with
the times in microseconds.
Development aid; bench.py is the contract for the headline metric."""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("local-features_amd", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import local_features_python as lfp  # noqa: E402
import view_graph_twin as vt  # noqa: E402
from bench_tracks import TIMED, WARMUP, timed  # noqa: E402

HOST_WARMUP, HOST_TIMED = 1, 3
DEG, ITERATIONS = 3.0, 10
BLOCK = 4096


def rotations(v):
    """Rodrigues, batched: rotation vectors [m, 3] -> matrices [m, 3, 3]"""
    a = np.linalg.norm(v, axis=1)
    k = v / np.maximum(a, 1e-300)[:, None]
    K = np.zeros((len(v), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    return np.eye(3) + np.sin(a)[:, None, None] * K + (1 - np.cos(a))[:, None, None] * (K @ K)


def scene(n, edges, seed, tree_rounds):
    g = np.random.default_rng(seed)
    ea, eb = np.array([e[0] for e in edges], np.uint32), np.array([e[1] for e in edges], np.uint32)
    E = len(ea)
    truth = rotations(g.normal(0, 1.0, (n, 3)))
    rel = rotations(g.normal(0, np.deg2rad(0.5) / np.sqrt(3), (E, 3))) @ truth[eb] @ truth[ea].transpose(0, 2, 1)
    wrong = g.random(E) < 0.10
    axis = g.normal(size=(E, 3))
    off = rotations(axis / np.linalg.norm(axis, axis=1)[:, None] * np.deg2rad(g.uniform(10, 180, E))[:, None])
    rel = np.where(wrong[:, None, None], off @ rel, rel)
    ps = np.zeros((E, 4), np.uint32)
    ps[:, 0] = np.where(wrong, g.integers(20, 60, E), 100 + g.permutation(E))
    return dict(n_images=n, edge_a=ea, edge_b=eb, R=rel.reshape(E, 9).astype(np.float32), pose_stats=ps, tree_rounds=tree_rounds)


class Device:
    def __init__(self, s):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.ea, self.eb = up(s["edge_a"].view(np.int32)), up(s["edge_b"].view(np.int32))
        self.R, self.ps = up(s["R"]), up(s["pose_stats"].view(np.int32))
        self.n, self.E, self.T = s["n_images"], len(s["edge_a"]), s["tree_rounds"]
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda")
        self.rot = torch.empty((self.n, 9), dtype=torch.float32, device="cuda")
        self.res = torch.empty((self.E,), dtype=torch.float32, device="cuda")
        self.es, self.ims, self.counts = i32(self.E, 4), i32(self.n, 4), i32(8)


def call(h, d, stream):
    h.view_graph_device(d.ea.data_ptr(), d.eb.data_ptr(), d.E, d.R.data_ptr(), d.ps.data_ptr(), d.n, d.rot.data_ptr(),
                        d.es.data_ptr(), d.ims.data_ptr(), d.counts.data_ptr(), d.res.data_ptr(), max_loop_deg=DEG,
                        tree_rounds=d.T, iterations=ITERATIONS, stream=stream)


def qmul(p, q):
    pw, px, py, pz = p.unbind(-1)
    qw, qx, qy, qz = q.unbind(-1)
    return torch.stack([pw * qw - px * qx - py * qy - pz * qz, pw * qx + px * qw + py * qz - pz * qy,
                        pw * qy - px * qz + py * qw + pz * qx, pw * qz + px * qy - py * qx + pz * qw], -1)


def torch_vote(d):
    """(closed [E], consistent [E]) in f64 with torch alone; every pair of the scenes has one edge and every edge is usable"""
    r = d.R.to(torch.float64).reshape(-1, 3, 3)
    t = r[:, 0, 0] + r[:, 1, 1] + r[:, 2, 2]
    k = torch.stack([t, r[:, 0, 0], r[:, 1, 1], r[:, 2, 2]], 1).argmax(1)
    forms = torch.stack([
        torch.stack([1 + t, r[:, 2, 1] - r[:, 1, 2], r[:, 0, 2] - r[:, 2, 0], r[:, 1, 0] - r[:, 0, 1]], 1),
        torch.stack([r[:, 2, 1] - r[:, 1, 2], 1 + 2 * r[:, 0, 0] - t, r[:, 0, 1] + r[:, 1, 0], r[:, 0, 2] + r[:, 2, 0]], 1),
        torch.stack([r[:, 0, 2] - r[:, 2, 0], r[:, 0, 1] + r[:, 1, 0], 1 + 2 * r[:, 1, 1] - t, r[:, 1, 2] + r[:, 2, 1]], 1),
        torch.stack([r[:, 1, 0] - r[:, 0, 1], r[:, 0, 2] + r[:, 2, 0], r[:, 1, 2] + r[:, 2, 1], 1 + 2 * r[:, 2, 2] - t], 1)], 1)
    q = torch.nn.functional.normalize(forms[torch.arange(d.E, device="cuda"), k], dim=1)
    a, b = d.ea.long(), d.eb.long()
    table = torch.zeros((d.n, d.n, 4), dtype=torch.float64, device="cuda")
    has = torch.zeros((d.n, d.n), dtype=torch.bool, device="cuda")
    conj = q * torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=torch.float64, device="cuda")
    table[a, b], table[b, a] = q, conj                                          # table[x, y] = q(x -> y)
    has[a, b] = has[b, a] = True
    cmax = float(np.cos(np.float64(np.float32(DEG)) * (np.pi / 180.0)))
    closed, consistent = [], []
    for lo in range(0, d.E, BLOCK):
        aa, bb, qe = a[lo:lo + BLOCK], b[lo:lo + BLOCK], q[lo:lo + BLOCK]
        L = qmul(table[:, aa].transpose(0, 1), qmul(table[bb], qe[:, None, :]))  # [block, n, 4]: q(c -> a) (q(b -> c) q_e)
        m = has[aa] & has[bb]
        closed.append(m.sum(1))
        consistent.append((m & (2 * L[..., 0] * L[..., 0] - 1 >= cmax)).sum(1))
    return torch.cat(closed), torch.cat(consistent)


def time_case(h, s, stream, exe, tmp):
    d = Device(s)
    call(h, d, stream)
    torch.cuda.synchronize()
    closed, consistent = torch_vote(d)
    es = d.es.cpu().numpy()
    assert (es[:, 0] == closed.cpu().numpy()).all() and (es[:, 1] == consistent.cpu().numpy()).all(), "the call and the torch route disagree"
    want = vt.run(exe, tmp, s, deg=DEG, tree_rounds=d.T, iterations=ITERATIONS)
    for got, k in ((d.rot, "rotations"), (d.es, "edge_stats"), (d.res, "residual"), (d.ims, "image_stats"), (d.counts, "counts")):
        assert np.array_equal(got.cpu().numpy().view(np.uint32).reshape(want[k].shape), want[k]), "the call and the twin differ in " + k
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(h, d, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    r = timed({"graph": g.replay, "call": lambda: call(h, d, stream), "torch_vote": lambda: torch_vote(d)})
    src, dst = os.path.join(tmp, "view_graph.in"), os.path.join(tmp, "view_graph.out")    # (vt.run left the call file there)
    host = []
    for it in range(HOST_WARMUP + HOST_TIMED):
        t0 = time.perf_counter()
        subprocess.run([exe, src, dst], check=True)
        if it >= HOST_WARMUP:
            host.append((time.perf_counter() - t0) * 1e6)
    counts = d.counts.cpu().numpy()
    launches, scratch, _ = lfp.view_graph_plan(d.n, d.E, d.T, ITERATIONS)
    med = lambda k: r[k]["median_us"]
    return {"images": d.n, "edges": d.E, "tree_rounds": d.T, "iterations": ITERATIONS, "launches": launches, "scratch_bytes": scratch,
            "supported": int(counts[1]), "rejected": int(counts[2]), "unchecked": int(counts[3]), "labelled": int(counts[5]),
            **{k + "_" + f: v[f] for k, v in r.items() for f in v},
            "twin_wall_median_us": round(statistics.median(host), 1), "call_over_graph": round(med("call") / med("graph"), 2),
            "torch_vote_over_graph": round(med("torch_vote") / med("graph"), 2),
            "twin_over_graph": round(statistics.median(host) / med("graph"), 1),
            "warmup": WARMUP, "timed": TIMED, "lib": os.path.basename(lfp.LIB_PATH)}


def make_case(k):
    g = np.random.default_rng(0)
    if k == 0:
        i, j = np.triu_indices(64, 1)
        return "all_pairs_64", scene(64, list(zip(i.tolist(), j.tolist())), 1, 4)
    if k == 1:
        pairs = set()
        for i in range(1024):
            for j in g.choice(1024, 32, replace=False).tolist():
                if i != j:
                    pairs.add((min(i, j), max(i, j)))
        return "picks_1024x32", scene(1024, sorted(pairs), 2, 8)
    return "window4_256", scene(256, [(t, t + w) for w in range(1, 5) for t in range(256 - w)], 4, 64)


def main():
    torch.cuda.init()
    torch.cuda.set_stream(torch.cuda.Stream())
    s = torch.cuda.current_stream().cuda_stream
    h = lfp.MkdHandle(max_features=64)
    only = [int(a) for a in sys.argv[1:] if a.isdigit()] or range(3)
    with tempfile.TemporaryDirectory() as tmp:
        exe = vt.build(tmp)
        for k in only:
            name, sc = make_case(k)
            print(json.dumps({"bench": "view_graph", "case": name, **time_case(h, sc, s, exe, tmp)}), flush=True)


if __name__ == "__main__":
    main()
