#!/usr/bin/env python3
"""Device time of lf_mkd_match_guided_pairs_device (guided matching: candidates restricted by each pair's H or F) against
lf_mkd_match_pairs_device on the same rows in the same run, both with LF_MKD_MATCH_MUTUAL (three launches each).

Shapes: 128 pairs of about 2000 x 2000 rows (sizes drawn in 1800 .. 2200) and 256 pairs of about 500 x 500.  Keypoints of
the a side are uniform in 1920 x 1080; half of each pair's b side is the true image of a rows under the pair's model (0.5 px
noise), the rest uniform.  Models: a true homography per pair at 3 px, a true fundamental matrix per pair (two views of a
3-D cloud) at 1.5 px -- the verifiers' thresholds.

Each side is recorded in a torch CUDA graph (several calls back to back) and the replays are timed by events; the sides
alternate, five repeats each, so that the spread is known.  Prints one JSON line: microseconds per call (one call = all
pairs, both directions, the filter), the ratio to the unguided call, and the share of 16 x 16 tiles the guided kernel
skips, counted outside the kernel from the admissibility masks (f32 on the device: a statistic, not the kernel's bits).

--trace: 30 plain calls of either entry point on the 128-pair homography case, for a per-kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/bench_match_guided.py --trace)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-features_amd"))
import local_features_python as lfp  # noqa: E402

REPEATS, REPLAYS, CALLS = 5, 5, 10
W, H = 1920.0, 1080.0


def _uniform(rng, n):
    return np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], axis=1)


def _homography_pair(rng, na, nb):
    h = np.array([[1 + rng.uniform(-.05, .05), rng.uniform(-.05, .05), rng.uniform(-40, 40)],
                  [rng.uniform(-.05, .05), 1 + rng.uniform(-.05, .05), rng.uniform(-40, 40)],
                  [rng.uniform(-2e-5, 2e-5), rng.uniform(-2e-5, 2e-5), 1.0]])
    a, b = _uniform(rng, na), _uniform(rng, nb)
    true = rng.permutation(nb)[:nb // 2]
    p = np.concatenate([a[rng.integers(0, na, len(true))], np.ones((len(true), 1))], axis=1) @ h.T
    b[true] = p[:, :2] / p[:, 2:3] + rng.normal(0, 0.5, (len(true), 2))
    return a, b, h.reshape(9)


def _fundamental_pair(rng, na, nb):
    K = np.array([[1500.0, 0, W / 2], [0, 1500.0, H / 2], [0, 0, 1]])
    X = np.stack([rng.uniform(-3.5, 3.5, na), rng.uniform(-2, 2, na), rng.uniform(5, 12, na)], axis=1)
    ry = rng.uniform(-.12, .12)
    R = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
    t = np.array([rng.uniform(.5, 1.0), rng.uniform(-.3, .3), rng.uniform(-.2, .2)])
    proj = lambda P: (P @ K.T)[:, :2] / (P @ K.T)[:, 2:3]
    a, b = proj(X), _uniform(rng, nb)
    true = rng.permutation(nb)[:nb // 2]
    b[true] = proj(X[rng.integers(0, na, len(true))] @ R.T + t) + rng.normal(0, 0.5, (len(true), 2))
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    F = np.linalg.inv(K).T @ tx @ R @ np.linalg.inv(K)
    return a, b, (F / F.reshape(-1)[np.abs(F).argmax()]).reshape(9)


class Case:
    def __init__(self, h, sizes, kind):
        self.h, self.sizes, self.kind = h, sizes, kind
        self.thr = 3.0 if kind == lfp.GUIDE_HOMOGRAPHY else 1.5
        na, nb = sum(s[0] for s in sizes), sum(s[1] for s in sizes)
        g = torch.Generator(device="cuda").manual_seed(na + nb)
        unit = lambda n: torch.nn.functional.normalize(torch.randn((n, 128), device="cuda", generator=g), dim=1)
        self.a, self.b = unit(na), unit(nb)
        rng = np.random.default_rng(na + 7 * kind)
        make = _homography_pair if kind == lfp.GUIDE_HOMOGRAPHY else _fundamental_pair
        parts = [make(rng, x, y) for x, y in sizes]
        kp = lambda xy: torch.from_numpy(np.concatenate([xy, np.zeros((len(xy), 3))], axis=1).astype(np.float32)).cuda()
        self.ka, self.kb = kp(np.concatenate([p[0] for p in parts])), kp(np.concatenate([p[1] for p in parts]))
        self.model = torch.from_numpy(np.stack([p[2] for p in parts]).astype(np.float32)).cuda()
        self.oa = np.cumsum([0] + [s[0] for s in sizes]).astype(np.int64)
        self.ob = np.cumsum([0] + [s[1] for s in sizes]).astype(np.int64)
        self.d_oa, self.d_ob = torch.from_numpy(self.oa).cuda(), torch.from_numpy(self.ob).cuda()
        self.ab = torch.empty((na,), dtype=torch.int32, device="cuda")
        self.ba = torch.empty((nb,), dtype=torch.int32, device="cuda")
        self.ab_plain, self.ba_plain = torch.empty_like(self.ab), torch.empty_like(self.ba)

    def guided(self, stream):
        self.h.match_guided_pairs_device(self.a.data_ptr(), self.ka.data_ptr(), self.d_oa.data_ptr(), self.a.shape[0],
                                         self.b.data_ptr(), self.kb.data_ptr(), self.d_ob.data_ptr(), self.b.shape[0],
                                         self.model.data_ptr(), len(self.sizes), self.ab.data_ptr(), self.ba.data_ptr(), self.kind,
                                         self.thr, 0.8, lfp.MATCH_MUTUAL, None, None, stream)

    def unguided(self, stream):
        self.h.match_pairs_device(self.a.data_ptr(), self.d_oa.data_ptr(), self.a.shape[0], self.b.data_ptr(), self.d_ob.data_ptr(),
                                  self.b.shape[0], len(self.sizes), self.ab_plain.data_ptr(), self.ba_plain.data_ptr(), 0.8,
                                  lfp.MATCH_MUTUAL, None, None, stream)

    def graph(self, fn):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            fn(s.cuda_stream)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(CALLS):
                fn(torch.cuda.current_stream().cuda_stream)
        g.replay()
        torch.cuda.synchronize()
        return g

    def tiles(self):
        """(16 x 16 tiles of all pairs, those with an admissible pair, admissible point pairs) -- one direction; the other
        direction's tiles are these transposed"""
        total = used = adm = 0
        thr2 = self.thr * self.thr
        for p, (na, nb) in enumerate(self.sizes):
            a, b = self.ka[self.oa[p]:self.oa[p + 1], :2], self.kb[self.ob[p]:self.ob[p + 1], :2]
            m = self.model[p]
            ax, ay, bx, by = a[:, 0, None], a[:, 1, None], b[None, :, 0], b[None, :, 1]
            l0, l1, l2 = m[0] * ax + m[1] * ay + m[2], m[3] * ax + m[4] * ay + m[5], m[6] * ax + m[7] * ay + m[8]
            if self.kind == lfp.GUIDE_HOMOGRAPHY:
                ok = (l2 > 0) & ((bx * l2 - l0) ** 2 + (by * l2 - l1) ** 2 < thr2 * l2 * l2)
            else:
                m0, m1 = m[0] * bx + m[3] * by + m[6], m[1] * bx + m[4] * by + m[7]
                ok = (bx * l0 + by * l1 + l2) ** 2 < thr2 * (l0 * l0 + l1 * l1 + m0 * m0 + m1 * m1)
            ta, tb = (na + 15) // 16, (nb + 15) // 16
            pad = torch.zeros((ta * 16, tb * 16), dtype=torch.bool, device="cuda")
            pad[:na, :nb] = ok
            used += int(pad.view(ta, 16, tb, 16).any(dim=3).any(dim=1).sum())
            total += ta * tb
            adm += int(ok.sum())
        return total, used, adm


def replay_us(g):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(REPLAYS):
        g.replay()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / (CALLS * REPLAYS)


def time_case(h, sizes, kind):
    c = Case(h, sizes, kind)
    g_g, g_u = c.graph(c.guided), c.graph(c.unguided)
    guided, unguided = [], []
    for _ in range(REPEATS):
        guided.append(replay_us(g_g))
        unguided.append(replay_us(g_u))
    total, used, adm = c.tiles()
    med = lambda x: float(np.median(x))
    r = lambda x: [round(v, 2) for v in x]
    return {"pairs": len(sizes), "rows_a": int(c.oa[-1]), "rows_b": int(c.ob[-1]), "threshold_px": c.thr,
            "guided_us": r(guided), "unguided_us": r(unguided), "guided_median_us": round(med(guided), 2),
            "unguided_median_us": round(med(unguided), 2), "guided_over_unguided": round(med(guided) / med(unguided), 3),
            "tiles": total, "tiles_skipped_share": round(1.0 - used / total, 4),
            "admissible_per_row": round(adm / max(int(c.oa[-1]), 1), 2),
            "guided_matches": int((c.ab >= 0).sum()), "unguided_matches": int((c.ab_plain >= 0).sum())}


def main():
    torch.cuda.init()
    h = lfp.MkdHandle(max_features=64)
    g = np.random.default_rng(0)
    big = [(int(x), int(y)) for x, y in g.integers(1800, 2201, (128, 2))]
    small = [(int(x), int(y)) for x, y in g.integers(450, 551, (256, 2))]
    if "--trace" in sys.argv[1:]:
        c = Case(h, big, lfp.GUIDE_HOMOGRAPHY)
        s = torch.cuda.Stream()
        for _ in range(30):
            c.guided(s.cuda_stream)
            c.unguided(s.cuda_stream)
        s.synchronize()
        print(json.dumps({"bench": "match_guided trace", "pairs": len(big), "calls_each": 30}))
        return
    out = {"bench": "match_guided", "repeats": REPEATS, "calls_per_replay": CALLS, "flags": "LF_MKD_MATCH_MUTUAL",
           "128x2000_homography": time_case(h, big, lfp.GUIDE_HOMOGRAPHY),
           "128x2000_fundamental": time_case(h, big, lfp.GUIDE_FUNDAMENTAL),
           "256x500_homography": time_case(h, small, lfp.GUIDE_HOMOGRAPHY),
           "256x500_fundamental": time_case(h, small, lfp.GUIDE_FUNDAMENTAL)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
