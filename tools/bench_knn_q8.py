#!/usr/bin/env python3
"""The top-k search over 8-bit rows against the top-2 matcher, same rows, same process: lf_mkd_match_q8_device and
lf_mkd_knn_q8_device (k = 1, 2, 4, 8, 16) alternate launch by launch, each timed with HIP events -- 5 warm-up and 20 timed
launches each, the median is reported.  One JSON line per size: 2000 x 2000, 10 000 x 10 000, 65 536 x 65 536, 2^20 x 2^20.
Where it fits (10 000^2, and 65 536^2 in row chunks of at most 4 GiB) the route a user had before is timed as well: the f32
product of the de-biased rows followed by torch.topk, k = 8.

    bench_knn_q8.py [--out DIR]           every size, each in a child process of its own under its own time limit; stops at
                                          the first size that fails; writes DIR/q8_knn.json and DIR/q8_knn.md (default:
                                          profiles/)
    bench_knn_q8.py --size NA NB [K ...]  one size, in this process, one JSON line on stdout

Development aid; bench.py is the contract for the headline metric."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((2000, 2000, 120), (10000, 10000, 180), (65536, 65536, 300), (1 << 20, 1 << 20, 900))   # (na, nb, time limit in s)
KS = (1, 2, 4, 8, 16)
WARMUP, TIMED = 5, 20
TOPK_K = 8
CHUNK_BYTES = 4 << 30


def one_size(na, nb, ks):
    sys.path.insert(0, os.path.join(ROOT, "local-features_amd"))
    import torch
    import local_features_python as lfp

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
    m = torch.empty(na, dtype=torch.int32, device="cuda")
    best = torch.empty(na, dtype=torch.int32, device="cuda")
    second = torch.empty(na, dtype=torch.int32, device="cuda")
    index = {k: torch.empty((na, k), dtype=torch.int32, device="cuda") for k in ks}
    score = {k: torch.empty((na, k), dtype=torch.int32, device="cuda") for k in ks}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        return e0, e1

    calls = {"match_q8": lambda: h.match_q8_device(qa.data_ptr(), na, qb.data_ptr(), nb, m.data_ptr(), 0.0, None, None,
                                                   best.data_ptr(), second.data_ptr(), stream=s)}
    for k in ks:
        calls[f"knn{k}"] = (lambda k=k: h.knn_q8_device(qa.data_ptr(), na, qb.data_ptr(), nb, k, index[k].data_ptr(),
                                                        score[k].data_ptr(), stream=s))
    chunk = min(na, CHUNK_BYTES // (4 * nb))
    dense = na * nb * 4 <= 16 * CHUNK_BYTES and chunk >= 1
    if dense:
        fa, fb = qa.float() - 128.0, qb.float() - 128.0

        def product_topk():
            for r0 in range(0, na, chunk):
                torch.topk(fa[r0:r0 + chunk] @ fb.T, min(TOPK_K, nb), dim=1)

        calls["product_topk"] = product_topk
    events = {name: [] for name in calls}
    for it in range(WARMUP + TIMED):
        for name, fn in calls.items():            # match_q8, knn1, knn2, ...; match_q8, knn1, ...
            ev = timed(fn)
            if it >= WARMUP:
                events[name].append(ev)
    torch.cuda.synchronize()
    ms = {name: statistics.median(e0.elapsed_time(e1) for e0, e1 in v) for name, v in events.items()}
    # the two calls agree where they must: column 0 and the scores of columns 0 / 1
    agree = all(bool((index[k][:, 0] == m).all()) and bool((score[k][:, 0] == best).all())
                and (k < 2 or bool((score[k][:, 1] == second).all())) for k in ks)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = {"na": na, "nb": nb, "match_q8_ms": round(ms["match_q8"], 4), "match_q8_grid": list(lfp.match_q8_plan(na, nb, cus)[:2]),
           "knn_ms": {str(k): round(ms[f"knn{k}"], 4) for k in ks},
           "knn_over_match_q8": {str(k): round(ms[f"knn{k}"] / ms["match_q8"], 3) for k in ks},
           "knn_grid": {str(k): list(lfp.knn_q8_plan(na, nb, k, cus)[:2]) for k in ks},
           "knn_scratch_bytes": {str(k): lfp.knn_q8_plan(na, nb, k, cus)[2] for k in ks},
           "agrees_with_match_q8": agree, "warmup": WARMUP, "timed": TIMED}
    if dense:
        out["product_topk_ms"] = round(ms["product_topk"], 4)
        out["product_topk_k"] = TOPK_K
        out["product_topk_row_chunk"] = chunk
        if TOPK_K in ks:
            out["product_topk_over_knn"] = round(ms["product_topk"] / ms[f"knn{TOPK_K}"], 1)
    print(json.dumps(out), flush=True)
    return 0 if agree else 2


def fmt(ms):
    return f"{ms * 1e3:.1f} us" if ms < 1 else f"{ms:.3f} ms"


def write_report(rows, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "q8_knn.json"), "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    ks = [k for k in rows[0]["knn_ms"]]
    lines = ["# The top-k search over 8-bit rows against the top-2 matcher", "",
             "`python tools/bench_knn_q8.py` on one MI355X: `lf_mkd_match_q8_device` (unchanged code, so the parent commit's) and",
             "`lf_mkd_knn_q8_device` alternate launch by launch in one process on the same quantised unit-norm random rows, each launch",
             f"between two HIP events, {WARMUP} warm-up and {TIMED} timed launches each, medians.  Each size ran in a child process of its own.",
             f"`product + topk` is the f32 product of the de-biased rows followed by `torch.topk`, k = {TOPK_K}, in row chunks of at most 4 GiB.",
             "", "```"] + [json.dumps(r) for r in rows] + ["```", "",
             "| rows | match_q8 | " + " | ".join(f"knn k = {k}" for k in ks) + " | product + topk | / knn k = 8 |",
             "|---|---|" + "---|" * (len(ks) + 2)]
    for r in rows:
        cells = [f"{fmt(r['knn_ms'][k])} ({r['knn_over_match_q8'][k]:.2f} x)" for k in ks]
        dense = fmt(r["product_topk_ms"]) if "product_topk_ms" in r else "does not fit"
        over = f"{r['product_topk_over_knn']} x" if "product_topk_over_knn" in r else ""
        lines.append(f"| {r['na']} x {r['nb']} | {fmt(r['match_q8_ms'])} | " + " | ".join(cells) + f" | {dense} | {over} |")
    lines += ["", "(In brackets: knn(k) / match_q8.)", ""]
    with open(os.path.join(out_dir, "q8_knn.md"), "w") as f:
        f.write("\n".join(lines))


def main():
    args = sys.argv[1:]
    if len(args) >= 3 and args[0] == "--size":
        return one_size(int(args[1]), int(args[2]), tuple(int(k) for k in args[3:]) or KS)
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
            print(f"bench_knn_q8: {na} x {nb} ended with status {rc}; stopping", file=sys.stderr)
            return rc
        print(p.stdout, end="", flush=True)
        rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
        write_report(rows, out_dir)
    return 0


if __name__ == "__main__":
    sys.exit(main())
