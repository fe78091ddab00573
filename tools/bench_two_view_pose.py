#!/usr/bin/env python3
"""Device time of lf_mkd_two_view_pose_device (per edge R, t, stats, sigma, and the links' triangulated points) against the
routes there were before it, on the same device tensors in one process:

    pose          the call with every output
    pose_no_points  the call with d_points = NULL (the vote and the parallax count alone)
    torch         the route without the call, f64: E = Kb^T F Ka batched, torch.linalg.eigh of E^T E, the four candidates,
                  repeat_interleave for the edge of every link (its result has a dynamic size, so the route synchronises),
                  the four in-front tests per link, index_add for the counts, argmax, and the elementwise triangulation under
                  the chosen candidate; HIP events like the others, and once more as wall clock
    host          F, the intrinsics, the keypoints and the link table copied to the host, then the numpy restatement of
                  tests/pose_cases.py (an eigh and a vectorised vote per edge); wall clock, 1 warm-up + 3 timed rounds

The device forms alternate call by call, each timed with HIP events -- 5 warm-up and 20 timed rounds; the median is reported,
and the 10th and 90th percentile as the run-to-run spread (bench_tracks.py's `timed`).  Before timing, the call's in-front
counts must equal the torch route's, R and t must agree within 1e-6 and the points within 1e-5 of their size (the scenes are exact: no link is near a decision).

Cases: a synthetic scene of 3-D points seen by pinhole cameras on a small baseline, every image showing a random subset, an
edge's links the points both images show (about 0.4 of an image's rows): 64 images of about 2000 rows with all 2016 pairs,
one query against 1024 images, 256 frames of about 500 rows with window 4; and one edge of 100 000 links.  Prints one JSON
line per case with the times in microseconds.
Development aid; bench.py is the contract for the headline metric."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("local-features_amd", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import local_features_python as lfp  # noqa: E402
import pose_cases as pc  # noqa: E402
from bench_tracks import TIMED, WARMUP, timed  # noqa: E402

HOST_WARMUP, HOST_TIMED = 1, 3
LINKED = 0.4
K4 = np.array([800.0, 800.0, 512.0, 384.0])
DEG = 2.0


def scene(sizes, edges, seed, share=LINKED):
    """a table (tests/pose_cases.py's dict) of a synthetic scene: image m shows sizes[m] of P points through its own camera"""
    g = np.random.default_rng(seed)
    n = len(sizes)
    P = int(max(sizes) / share)
    X = np.concatenate([g.uniform(-3, 3, (P, 2)), g.uniform(4, 12, (P, 1))], axis=1)
    cams = [(pc.fc.rotation(*g.uniform(-3, 3, 3)), g.uniform(-0.8, 0.8, 3) * [1, 0.3, 0.3]) for _ in range(n)]
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    kps = np.zeros((int(first[-1]), 5), np.float32)
    shown = []
    for m in range(n):
        pts = g.permutation(P)[:sizes[m]] if sizes[m] < P else np.arange(P)
        x = X[pts] @ cams[m][0].T + cams[m][1]
        kps[first[m]:first[m + 1], 0] = K4[0] * x[:, 0] / x[:, 2] + K4[2]
        kps[first[m]:first[m + 1], 1] = K4[1] * x[:, 1] / x[:, 2] + K4[3]
        where = np.full(P, -1, np.int64)
        where[pts] = np.arange(len(pts))
        shown.append(where)
    la, lb, off, fs = [], [], [0], []
    ki = np.linalg.inv(np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1.0]]))
    for a, b in edges:
        both = np.flatnonzero((shown[a] >= 0) & (shown[b] >= 0))
        both = both[np.argsort(shown[a][both])]
        la.append(first[a] + shown[a][both])
        lb.append(first[b] + shown[b][both])
        off.append(off[-1] + len(both))
        r = cams[b][0] @ cams[a][0].T                      # x_b = R x_a + t
        t = cams[b][1] - r @ cams[a][1]
        f = ki.T @ pc.fc.skew(t) @ r @ ki
        fs.append(f / np.abs(f).max())
    return {"kps": kps, "edge_a": np.array([e[0] for e in edges], np.uint32), "edge_b": np.array([e[1] for e in edges], np.uint32),
            "intrinsics": np.tile(K4.astype(np.float32), (n, 1)), "F": np.array(fs).reshape(-1, 9).astype(np.float32),
            "link_offsets": np.array(off, np.uint64), "link_a": np.concatenate(la).astype(np.int32),
            "link_b": np.concatenate(lb).astype(np.int32)}


class Device:
    def __init__(self, t):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.kps, self.intr, self.F = up(t["kps"]), up(t["intrinsics"]), up(t["F"])
        self.ea, self.eb = up(t["edge_a"].view(np.int32)), up(t["edge_b"].view(np.int32))
        self.off, self.la, self.lb = up(t["link_offsets"].view(np.int64)), up(t["link_a"]), up(t["link_b"])
        self.n_edges, self.cap = len(t["edge_a"]), len(t["link_a"])
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
        self.R, self.t, self.sigma, self.points = f32(self.n_edges, 9), f32(self.n_edges, 3), f32(self.n_edges, 3), f32(self.cap, 4)
        self.stats = torch.empty((self.n_edges, 4), dtype=torch.int32, device="cuda")


def call_pose(h, d, stream, points=True):
    h.two_view_pose_device(d.kps.data_ptr(), d.kps.shape[0], d.ea.data_ptr(), d.eb.data_ptr(), d.n_edges, d.intr.data_ptr(),
                           d.intr.shape[0], d.F.data_ptr(), d.off.data_ptr(), d.la.data_ptr(), d.lb.data_ptr(), d.cap,
                           d.R.data_ptr(), d.t.data_ptr(), d.stats.data_ptr(), d.sigma.data_ptr(),
                           d.points.data_ptr() if points else None, DEG, 0, stream)


def torch_route(d):
    """(R [E,3,3], t [E,3], front counts [E,4], chosen [E], points [links,4]) in f64 with torch alone"""
    f64 = torch.float64
    E_n = d.n_edges
    ka, kb = d.intr[d.ea.long()].to(f64), d.intr[d.eb.long()].to(f64)

    def kmat(k):
        m = torch.zeros((E_n, 3, 3), dtype=f64, device="cuda")
        m[:, 0, 0], m[:, 1, 1], m[:, 0, 2], m[:, 1, 2], m[:, 2, 2] = k[:, 0], k[:, 1], k[:, 2], k[:, 3], 1.0
        return m

    E = kmat(kb).transpose(1, 2) @ d.F.to(f64).reshape(-1, 3, 3) @ kmat(ka)
    w, v = torch.linalg.eigh(E.transpose(1, 2) @ E)                  # ascending
    v1, v2 = v[:, :, 2], v[:, :, 1]
    u1 = torch.nn.functional.normalize((E @ v1[:, :, None])[:, :, 0], dim=1)
    u2 = (E @ v2[:, :, None])[:, :, 0]
    u2 = torch.nn.functional.normalize(u2 - (u1 * u2).sum(1, keepdim=True) * u1, dim=1)
    u3, v3 = torch.linalg.cross(u1, u2), torch.linalg.cross(v1, v2)
    outer = lambda a, b: a[:, :, None] * b[:, None, :]
    r1 = outer(u2, v1) - outer(u1, v2) + outer(u3, v3)
    r2 = outer(u1, v2) - outer(u2, v1) + outer(u3, v3)
    Rs = torch.stack([r1, r1, r2, r2], dim=1)                        # [E,4,3,3]
    ts = torch.stack([u3, -u3, u3, -u3], dim=1)                      # [E,4,3]
    counts = (d.off[1:] - d.off[:-1])
    e_of = torch.repeat_interleave(torch.arange(E_n, device="cuda"), counts)   # (synchronises: the result's size)
    n = e_of.numel()

    def rays(rows, k):
        xy = d.kps[rows.long()[:n], :2].to(f64)
        return torch.stack([(xy[:, 0] - k[:, 2]) / k[:, 0], (xy[:, 1] - k[:, 3]) / k[:, 1], torch.ones(n, dtype=f64, device="cuda")], 1)

    xa, xb = rays(d.la, ka[e_of]), rays(d.lb, kb[e_of])

    def vote(R, t):
        p = (R @ xa[:, :, None])[:, :, 0]
        pp, qq, pq, pt, qt = (p * p).sum(1), (xb * xb).sum(1), (p * xb).sum(1), (p * t).sum(1), (xb * t).sum(1)
        det, na, nb = pp * qq - pq * pq, pq * qt - pt * qq, pp * qt - pq * pt
        return det, na, nb, pp, qq, pq

    front = torch.zeros((E_n, 4), dtype=torch.int64, device="cuda")
    for c in range(4):
        det, na, nb, _, _, _ = vote(Rs[e_of, c], ts[e_of, c])
        front[:, c] = torch.zeros(E_n, dtype=torch.int64, device="cuda").index_add_(0, e_of, ((det > 0) & (na > 0) & (nb > 0)).long())
    c = torch.argmax(front, dim=1)
    R, t = Rs[torch.arange(E_n), c], ts[torch.arange(E_n), c]
    det, na, nb, pp, qq, pq = vote(R[e_of], t[e_of])
    ok = (det > 0) & (na > 0) & (nb > 0)
    la_, lb_ = na / det, nb / det
    w_ = lb_[:, None] * xb - t[e_of]
    X = 0.5 * (la_[:, None] * xa + (R[e_of].transpose(1, 2) @ w_[:, :, None])[:, :, 0])
    pts = torch.cat([X, (pq / torch.sqrt(pp * qq))[:, None]], 1)
    none = torch.tensor([0.0, 0.0, 0.0, 2.0], dtype=f64, device="cuda")
    return R, t, front, c, torch.where(ok[:, None], pts, none).float()


def time_case(h, t, stream):
    d = Device(t)
    call_pose(h, d, stream)
    torch.cuda.synchronize()
    R, tt, front, c, pts = torch_route(d)
    st = d.stats.cpu().numpy()
    best = front.max(1).values.cpu().numpy()
    assert (st[:, 0] == best).all(), "the call and the torch route disagree on the in-front counts"
    assert float((d.R.reshape(-1, 3, 3) - R.float()).abs().max()) < 1e-6 and float((d.t - tt.float()).abs().max()) < 1e-6, "R or t differ"
    n = pts.shape[0]
    scale = pts[:, :3].abs().max(1).values.clamp(min=1.0)         # (depths are in units of the baseline: large for a short one)
    assert float(((d.points[:n] - pts).abs().max(1).values / scale).max()) < 1e-5, "the points differ"
    r = timed({"pose": lambda: call_pose(h, d, stream), "pose_no_points": lambda: call_pose(h, d, stream, False),
               "torch": lambda: torch_route(d)})
    wall, host = [], []
    for it in range(WARMUP + TIMED):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch_route(d)
        torch.cuda.synchronize()
        if it >= WARMUP:
            wall.append((time.perf_counter() - t0) * 1e6)
    for it in range(HOST_WARMUP + HOST_TIMED):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tab = {"kps": d.kps.cpu().numpy(), "edge_a": d.ea.cpu().numpy().view(np.uint32), "edge_b": d.eb.cpu().numpy().view(np.uint32),
               "intrinsics": d.intr.cpu().numpy(), "F": d.F.cpu().numpy(), "link_offsets": d.off.cpu().numpy().view(np.uint64),
               "link_a": d.la.cpu().numpy(), "link_b": d.lb.cpu().numpy()}
        pc.reference(tab, DEG)
        if it >= HOST_WARMUP:
            host.append((time.perf_counter() - t0) * 1e6)
    med = lambda k: r[k]["median_us"]
    return {"pool_rows": int(d.kps.shape[0]), "edges": d.n_edges, "links": n, "poses": int((st[:, 2] >= 0).sum()),
            "in_front": int(st[:, 0].sum()), "with_parallax": int(st[:, 3].sum()),
            **{k + "_" + f: v[f] for k, v in r.items() for f in v},
            "torch_wall_median_us": round(statistics.median(wall), 1), "host_wall_median_us": round(statistics.median(host), 1),
            "torch_over_pose": round(med("torch") / med("pose"), 2), "host_over_pose": round(statistics.median(host) / med("pose"), 1),
            "warmup": WARMUP, "timed": TIMED, "lib": os.path.basename(lfp.LIB_PATH)}


def make_case(k):
    g = np.random.default_rng(0)
    if k == 0:
        i, j = np.triu_indices(64, 1)
        return "all_pairs_64x2000", scene(g.integers(1800, 2201, 64), list(zip(i.tolist(), j.tolist())), 1)
    if k == 1:
        return "query_2000_x_1024_images", scene(np.concatenate([[2000], g.integers(1800, 2201, 1024)]), [(0, m) for m in range(1, 1025)], 2)
    if k == 2:
        return "window4_256x500", scene(g.integers(450, 551, 256), [(t, t + d) for d in range(1, 5) for t in range(256 - d)], 4)
    return "one_edge_100k_links", scene(np.array([100000, 100000]), [(0, 1)], 5, share=1.0)


def main():
    torch.cuda.init()
    torch.cuda.set_stream(torch.cuda.Stream())
    s = torch.cuda.current_stream().cuda_stream
    h = lfp.MkdHandle(max_features=64)
    only = [int(a) for a in sys.argv[1:] if a.isdigit()] or range(4)
    for k in only:
        name, t = make_case(k)
        print(json.dumps({"bench": "two_view_pose", "case": name, **time_case(h, t, s)}), flush=True)


if __name__ == "__main__":
    main()
