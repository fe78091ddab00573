#!/usr/bin/env python3
"""Grouped matching over 8-bit rows against the unchanged calls, same rows, same process: lf_mkd_match_q8_device,
lf_mkd_knn_q8_device (k = 4, 8) and lf_mkd_match_q8_grouped_device alternate launch by launch, each timed with HIP events --
5 warm-up and 20 timed launches each, the median is reported.  The grouped call runs three times per round: with groups of
2000 consecutive rows (a pooled database of images), with group = index (the top-2 call's question) and with a single group
(the degenerate case: its gate never closes).  lf_mkd_vote_groups_device behind the grouped call is timed as well, and,
outside the alternation, the route a user had before: knn k = 8, the copy of its table to the host and find_image.py's
rank_images (wall clock, median of 3).  One JSON line per size: 2000 x 200 000 (one query image against 100 pooled images),
65 536 x 65 536, 2^20 x 2^20.

    bench_match_q8_grouped.py [--out DIR]   every size, each in a child process of its own under its own time limit; stops
                                            at the first size that fails; writes DIR/q8_grouped.json and DIR/q8_grouped.md
                                            (default: profiles/)
    bench_match_q8_grouped.py --size NA NB  one size, in this process, one JSON line on stdout

Development aid; bench.py is the contract for the headline metric.  LF_MKD_LIB selects a build of another workgroup shape."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((2000, 200000, 180), (65536, 65536, 300), (1 << 20, 1 << 20, 900))   # (na, nb, time limit in s)
GROUP_ROWS = 2000
KS = (4, 8)
WARMUP, TIMED = 5, 20
RATIO = 0.8


def one_size(na, nb):
    sys.path.insert(0, os.path.join(ROOT, "local-features_amd"))
    sys.path.insert(0, os.path.join(ROOT, "local-features_amd", "examples"))
    import numpy as np
    import torch
    import local_features_python as lfp
    from find_image import rank_images

    torch.cuda.set_stream(torch.cuda.Stream())
    h = lfp.MkdHandle(max_features=64)
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(na + nb)
    qa = torch.empty((na, 128), dtype=torch.uint8, device="cuda")
    qb = torch.empty((nb, 128), dtype=torch.uint8, device="cuda")
    for q, n in ((qa, na), (qb, nb)):
        for r0 in range(0, n, 1 << 18):       # (in pieces: the f32 rows of the largest size need not exist all at once)
            r1 = min(n, r0 + (1 << 18))
            x = torch.nn.functional.normalize(torch.randn((r1 - r0, 128), device="cuda", generator=g), dim=1)
            h.quantize_descriptors_device(x.data_ptr(), r1 - r0, q[r0:r1].data_ptr(), stream=s)
    n_groups = -(-nb // GROUP_ROWS)
    groups = {"images": torch.arange(nb, dtype=torch.int32, device="cuda") // GROUP_ROWS,
              "index": torch.arange(nb, dtype=torch.int32, device="cuda"),
              "single": torch.zeros(nb, dtype=torch.int32, device="cuda")}

    def ints(*shape):
        return torch.empty(shape, dtype=torch.int32, device="cuda")

    m, best, second = ints(na), ints(na), ints(na)
    index, score = {k: ints(na, k) for k in KS}, {k: ints(na, k) for k in KS}
    out = {name: (ints(na), ints(na), ints(na)) for name in groups}
    votes = ints(1, n_groups)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        return e0, e1

    def grouped(name, ratio=RATIO):
        o = out[name]
        h.match_q8_grouped_device(qa.data_ptr(), na, qb.data_ptr(), nb, groups[name].data_ptr(), o[0].data_ptr(), ratio, None,
                                  None, o[1].data_ptr(), o[2].data_ptr(), stream=s)

    def grouped_and_vote():
        grouped("images")
        h.vote_groups_device(out["images"][0].data_ptr(), na, groups["images"].data_ptr(), nb, n_groups, votes.data_ptr(), stream=s)

    calls = {"match_q8": lambda: h.match_q8_device(qa.data_ptr(), na, qb.data_ptr(), nb, m.data_ptr(), RATIO, None, None,
                                                   best.data_ptr(), second.data_ptr(), stream=s)}
    for k in KS:
        calls[f"knn{k}"] = (lambda k=k: h.knn_q8_device(qa.data_ptr(), na, qb.data_ptr(), nb, k, index[k].data_ptr(),
                                                        score[k].data_ptr(), stream=s))
    for name in groups:
        calls[f"grouped_{name}"] = (lambda name=name: grouped(name))
    calls["grouped_images_and_vote"] = grouped_and_vote
    events = {name: [] for name in calls}
    for it in range(WARMUP + TIMED):
        for name, fn in calls.items():            # match_q8, knn4, knn8, grouped ...; match_q8, ...
            ev = timed(fn)
            if it >= WARMUP:
                events[name].append(ev)
    torch.cuda.synchronize()
    times = {name: sorted(e0.elapsed_time(e1) for e0, e1 in v) for name, v in events.items()}
    ms = {name: statistics.median(v) for name, v in times.items()}
    # the calls agree where they must: group = index is the matcher, best is the top-k table's column 0
    agree = all(bool((a == b).all()) for a, b in zip(out["index"], (m, best, second)))
    agree = agree and all(bool((out[name][1] == score[KS[0]][:, 0]).all()) for name in groups)
    agree = agree and bool((out["single"][2] == -2 ** 31).all()) and bool((out["single"][0] >= 0).all())
    agree = agree and int(votes.sum()) == int((out["images"][0] >= 0).sum())
    # the route a user had before: k = 8 neighbours, their table to the host, the first neighbour of another image in numpy
    offsets = np.minimum(np.arange(n_groups + 1, dtype=np.int64) * GROUP_ROWS, nb)
    route = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        calls["knn8"]()
        torch.cuda.current_stream().synchronize()
        old_votes = rank_images(index[8].cpu().numpy(), score[8].cpu().numpy(), offsets, RATIO)
        route.append((time.perf_counter() - t0) * 1e3)
    exact_votes = votes.cpu().numpy().reshape(-1).astype(np.int64)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = lfp.match_q8_grouped_plan(na, nb, cus)
    res = {"na": na, "nb": nb, "group_rows": GROUP_ROWS, "match_q8_ms": round(ms["match_q8"], 4),
           "knn_ms": {str(k): round(ms[f"knn{k}"], 4) for k in KS},
           "grouped_ms": {name: round(ms[f"grouped_{name}"], 4) for name in groups},
           "grouped_images_and_vote_ms": round(ms["grouped_images_and_vote"], 4),
           "knn8_copy_rank_images_wall_ms": round(statistics.median(route), 3),
           "grouped_images_over_knn4": round(ms["grouped_images"] / ms["knn4"], 3),
           "grouped_images_over_match_q8": round(ms["grouped_images"] / ms["match_q8"], 3),
           "min_max_ms": {name: [round(v[0], 4), round(v[-1], 4)] for name, v in times.items()},
           "grouped_grid": list(plan[:2]), "grouped_scratch_bytes": plan[2],
           "match_q8_grid": list(lfp.match_q8_plan(na, nb, cus)[:2]), "knn_grid": list(lfp.knn_q8_plan(na, nb, 4, cus)[:2]),
           "votes_exact": int(exact_votes.sum()), "votes_k8_rule": int(old_votes.sum()),
           "exact_at_most_k8_rule": bool((exact_votes <= old_votes).all()),
           "agrees": agree, "lib": os.path.basename(os.path.dirname(lfp.LIB_PATH)) + "/" + os.path.basename(lfp.LIB_PATH),
           "warmup": WARMUP, "timed": TIMED}
    print(json.dumps(res), flush=True)
    return 0 if agree and res["exact_at_most_k8_rule"] else 2


def fmt(ms):
    return f"{ms * 1e3:.1f} us" if ms < 1 else f"{ms:.3f} ms"


def write_report(rows, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "q8_grouped.json"), "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    lines = ["# Grouped matching over 8-bit rows against the top-2 matcher and the top-k search", "",
             "`python tools/bench_match_q8_grouped.py` on one MI355X: `lf_mkd_match_q8_device`, `lf_mkd_knn_q8_device` (both unchanged",
             "code, so the parent commit's) and `lf_mkd_match_q8_grouped_device` alternate launch by launch in one process on the same",
             f"quantised unit-norm random rows, each launch between two HIP events, {WARMUP} warm-up and {TIMED} timed launches each, medians.",
             f"Each size ran in a child process of its own.  `images`: groups of {GROUP_ROWS} consecutive rows; `index`: group = index;",
             "`single`: one group, the degenerate case.  `+ vote`: the grouped call and `lf_mkd_vote_groups_device` together.",
             "`k = 8 route`: knn k = 8, its table copied to the host and `rank_images` in numpy, wall clock, median of 3.",
             "", "```"] + [json.dumps(r) for r in rows] + ["```", "",
             "| rows | match_q8 | knn k = 4 | knn k = 8 | grouped, images | grouped, index | grouped, single | + vote | k = 8 route |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        gm = r["grouped_ms"]
        lines.append(f"| {r['na']} x {r['nb']} | {fmt(r['match_q8_ms'])} | {fmt(r['knn_ms']['4'])} | {fmt(r['knn_ms']['8'])} | "
                     f"{fmt(gm['images'])} ({r['grouped_images_over_knn4']:.2f} x knn 4) | {fmt(gm['index'])} | {fmt(gm['single'])} | "
                     f"{fmt(r['grouped_images_and_vote_ms'])} | {fmt(r['knn8_copy_rank_images_wall_ms'])} |")
    lines += [""]
    with open(os.path.join(out_dir, "q8_grouped.md"), "w") as f:
        f.write("\n".join(lines))


def main():
    args = sys.argv[1:]
    if len(args) == 3 and args[0] == "--size":
        return one_size(int(args[1]), int(args[2]))
    out_dir = args[1] if len(args) == 2 and args[0] == "--out" else os.path.join(ROOT, "profiles")
    rows = []
    for na, nb, limit in SIZES:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--size", str(na), str(nb)], timeout=limit,
                               stdout=subprocess.PIPE, text=True)
            rc = p.returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"bench_match_q8_grouped: {na} x {nb} ended with status {rc}; stopping", file=sys.stderr)
            return rc
        print(p.stdout, end="", flush=True)
        rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
        write_report(rows, out_dir)
    return 0


if __name__ == "__main__":
    sys.exit(main())
