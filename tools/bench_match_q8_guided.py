#!/usr/bin/env python3
"""Device time of lf_mkd_match_q8_guided_pairs_device (guided matching over 8-bit rows) against the two calls it joins, all
three on the same rows in the same process, all with LF_MKD_MATCH_MUTUAL (three launches each):

    q8_guided   the new call, on the quantised rows
    f32_guided  lf_mkd_match_guided_pairs_device on the f32 rows the bytes were quantised from: same keypoints, model, threshold
    q8_pairs    lf_mkd_match_q8_pairs_device on the same bytes: the unguided call whose y stream the new one keeps

Shapes, keypoints and models are those of tools/bench_match_guided.py (its generators are imported): 128 pairs of about
2000 x 2000 rows and 256 pairs of about 500 x 500; a true homography per pair at 3 px, a true fundamental matrix per pair at
1.5 px.  The descriptors are random unit rows, quantised on the device at the default scale.

Each call is recorded in a torch CUDA graph (CALLS calls back to back) and the replays are timed by events; the three
alternate, REPEATS repeats each, so that the spread is known.  The share of 32 x 32 tiles without an admissible pair -- what
the new kernel skips -- is counted outside the kernel from the admissibility masks, both directions (f32 on the device: a
statistic, not the kernel's bits).  Prints one JSON line per case, and with --out DIR writes DIR/q8_guided.json and the table
DIR/q8_guided.md."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-features_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_features_python as lfp  # noqa: E402
import bench_match_guided as f32bench  # noqa: E402

REPEATS, REPLAYS, CALLS = 5, 5, 10
TILE = 32


class Case(f32bench.Case):
    """bench_match_guided's case (f32 rows, keypoints, models, offsets) plus the quantised rows and the outputs of three calls"""

    def __init__(self, h, sizes, kind):
        super().__init__(h, sizes, kind)
        na, nb = self.a.shape[0], self.b.shape[0]
        self.qa = torch.empty((na, 128), dtype=torch.uint8, device="cuda")
        self.qb = torch.empty((nb, 128), dtype=torch.uint8, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        h.quantize_descriptors_device(self.a.data_ptr(), na, self.qa.data_ptr(), stream=s)
        h.quantize_descriptors_device(self.b.data_ptr(), nb, self.qb.data_ptr(), stream=s)
        torch.cuda.synchronize()
        self.ab_q8g, self.ba_q8g = torch.empty_like(self.ab), torch.empty_like(self.ba)
        self.ab_q8, self.ba_q8 = torch.empty_like(self.ab), torch.empty_like(self.ba)

    def q8_guided(self, stream):
        self.h.match_q8_guided_pairs_device(self.qa.data_ptr(), self.ka.data_ptr(), self.d_oa.data_ptr(), self.qa.shape[0],
                                            self.qb.data_ptr(), self.kb.data_ptr(), self.d_ob.data_ptr(), self.qb.shape[0],
                                            self.model.data_ptr(), len(self.sizes), self.ab_q8g.data_ptr(), self.ba_q8g.data_ptr(),
                                            self.kind, self.thr, 0.8, lfp.MATCH_MUTUAL, None, None, stream)

    def q8_pairs(self, stream):
        self.h.match_q8_pairs_device(self.qa.data_ptr(), self.d_oa.data_ptr(), self.qa.shape[0], self.qb.data_ptr(),
                                     self.d_ob.data_ptr(), self.qb.shape[0], len(self.sizes), self.ab_q8.data_ptr(),
                                     self.ba_q8.data_ptr(), 0.8, lfp.MATCH_MUTUAL, None, None, stream)

    def tiles32(self):
        """(32 x 32 tiles of all pairs, those with an admissible pair, admissible point pairs): the tiling is the same in both
        directions (x tiles counted from the pair's first row), so one count serves both"""
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
            ta, tb = (na + TILE - 1) // TILE, (nb + TILE - 1) // TILE
            pad = torch.zeros((ta * TILE, tb * TILE), dtype=torch.bool, device="cuda")
            pad[:na, :nb] = ok
            used += int(pad.view(ta, TILE, tb, TILE).any(dim=3).any(dim=1).sum())
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
    calls = {"q8_guided": c.q8_guided, "f32_guided": c.guided, "q8_pairs": c.q8_pairs}
    graphs = {k: c.graph(fn) for k, fn in calls.items()}
    us = {k: [] for k in calls}
    for _ in range(REPEATS):
        for k in calls:                                   # the three alternate
            us[k].append(replay_us(graphs[k]))
    total, used, adm = c.tiles32()
    med = {k: float(np.median(v)) for k, v in us.items()}
    out = {"pairs": len(sizes), "rows_a": int(c.oa[-1]), "rows_b": int(c.ob[-1]), "threshold_px": c.thr}
    for k in calls:
        out[k + "_us"] = [round(v, 2) for v in us[k]]
        out[k + "_median_us"] = round(med[k], 2)
    out.update({"f32_guided_over_q8_guided": round(med["f32_guided"] / med["q8_guided"], 3),
                "q8_guided_over_q8_pairs": round(med["q8_guided"] / med["q8_pairs"], 3),
                "tiles_32x32": total, "tiles_skipped_share": round(1.0 - used / total, 4),
                "admissible_per_row": round(adm / max(int(c.oa[-1]), 1), 2),
                "q8_guided_matches": int((c.ab_q8g >= 0).sum()), "f32_guided_matches": int((c.ab >= 0).sum()),
                "q8_pairs_matches": int((c.ab_q8 >= 0).sum())})
    return out


def table(results):
    spread = lambda v: f"{np.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"
    lines = ["| case | q8 guided, us | f32 guided, us | q8 unguided, us | f32 guided / q8 guided | q8 guided / q8 unguided | 32 x 32 tiles skipped |",
             "|---|---|---|---|---|---|---|"]
    for name, r in results.items():
        lines.append(f"| {name} | {spread(r['q8_guided_us'])} | {spread(r['f32_guided_us'])} | {spread(r['q8_pairs_us'])} | "
                     f"{r['f32_guided_over_q8_guided']:.2f} | {r['q8_guided_over_q8_pairs']:.2f} | {100 * r['tiles_skipped_share']:.1f} % |")
    return "\n".join(lines)


def main():
    args = sys.argv[1:]
    out_dir = args[args.index("--out") + 1] if "--out" in args else None
    torch.cuda.init()
    h = lfp.MkdHandle(max_features=64)
    g = np.random.default_rng(0)
    big = [(int(x), int(y)) for x, y in g.integers(1800, 2201, (128, 2))]
    small = [(int(x), int(y)) for x, y in g.integers(450, 551, (256, 2))]
    results = {}
    for name, sizes, kind in (("128 pairs of ~2000 x 2000, H at 3 px", big, lfp.GUIDE_HOMOGRAPHY),
                              ("128 pairs of ~2000 x 2000, F at 1.5 px", big, lfp.GUIDE_FUNDAMENTAL),
                              ("256 pairs of ~500 x 500, H at 3 px", small, lfp.GUIDE_HOMOGRAPHY),
                              ("256 pairs of ~500 x 500, F at 1.5 px", small, lfp.GUIDE_FUNDAMENTAL)):
        results[name] = time_case(h, sizes, kind)
        print(json.dumps({"bench": "match_q8_guided", "case": name, **results[name]}), flush=True)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        meta = {"bench": "match_q8_guided", "device": torch.cuda.get_device_name(0), "repeats": REPEATS, "replays": REPLAYS,
                "calls_per_replay": CALLS, "flags": "LF_MKD_MATCH_MUTUAL", "cases": results}
        with open(os.path.join(out_dir, "q8_guided.json"), "w") as f:
            json.dump(meta, f, indent=1)
            f.write("\n")
        with open(os.path.join(out_dir, "q8_guided.md"), "w") as f:
            f.write("Microseconds per call: median (min .. max) of %d repeats, %d calls per hipGraph, %d replays per repeat; one call = all "
                    "pairs, both directions, LF_MKD_MATCH_MUTUAL.  %s.\n\n" % (REPEATS, CALLS, REPLAYS, meta["device"]))
            f.write(table(results) + "\n")


if __name__ == "__main__":
    main()
