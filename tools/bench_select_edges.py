#!/usr/bin/env python3
"""Device time of lf_mkd_select_edges_device (per row of a vote table its k best columns, and the edge list those picks make)
against the route there was before it, on the same device tensors in one process:

    select        the call with every output, LF_MKD_SELECT_SKIP_SELF on the square tables, min_votes = 0 (the torch route drops
                  no column either)
    unique        the same with LF_MKD_SELECT_UNIQUE (square tables only)
    rank_only     the call with edge_capacity = 0: the selection and the three small launches behind it, no edge written
    torch         examples/match_collection.py --retrieve's route: masked_fill of the diagonal (square tables), torch.topk of
                  the table as int64, repeat_interleave of the row ids
    torch_unique  that route plus a dedupe of the unordered pairs: minimum / maximum, one 64-bit key, torch.unique.  Its result
                  has a dynamic size, so it synchronises: timed with HIP events like the others, and once more as wall clock
                  from a synchronised start to a synchronised end

The forms alternate call by call, each timed with HIP events -- 5 warm-up and 20 timed rounds; the median is reported, and the
10th and 90th percentile as the run-to-run spread.  Before timing, the call's rank_votes must equal torch.topk's values (the
columns may differ among equal votes: torch.topk promises no order there), and its UNIQUE edge count the dedupe's at the rows
where no tie is cut.

Tables: votes in [0, 40) with a band of neighbours that agree (120 - 10 |i - j| for |i - j| <= 8, plus noise), so that most
picks are mutual, as in a collection whose neighbours see the same scene.  Shapes: 64^2, 1024^2 and 16 384^2 at k = 4, 8, 32,
and the query cases 1 x 1024 and 1 x 65 536 at k = 8.  `read_gb_s` is the table's bytes over the median of `select`.

--matcher: lf_mkd_match_q8_edges_device (both directions, the cross-check) on 64 images of about 2000 rows over the edge list
of --retrieve 4 (256 edges, every mutual pick twice) and over that of --select 4 (256 entries, the mutual picks once and
padding behind): the matcher work the dedupe saves.
--trace N K: only the square shape N at K, 20 plain calls of `select`, for a per-kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/bench_select_edges.py --trace 16384 4).
LF_MKD_LIB selects another build.  Development aid; bench.py is the contract for the headline metric."""
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
from bench_match_q8_edges import WARMUP, TIMED, layout, pool, timed  # noqa: E402


def vote_table(n_a, n_b, seed):
    """[n_a, n_b] int32 on the device: noise below 40 and, on square tables, a band of agreeing neighbours"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    v = torch.randint(0, 40, (n_a, n_b), dtype=torch.int32, device="cuda", generator=g)
    if n_a == n_b:
        i = torch.arange(n_a, device="cuda")
        for d in range(1, 9):
            j = i[:-d] if d < n_a else i[:0]
            v[j, j + d] += 120 - 10 * d
            v[j + d, j] += 120 - 10 * d
    return v


class Outputs:
    def __init__(self, n_a, k):
        i32 = lambda n: torch.empty((n,), dtype=torch.int32, device="cuda")
        self.cap = n_a * k
        self.rank, self.rank_votes, self.ea, self.eb, self.ev, self.counts = i32(self.cap), i32(self.cap), i32(self.cap), i32(self.cap), i32(self.cap), i32(4)


def call_select(h, v, k, flags, o, stream, edges=True):
    p = lambda x: x.data_ptr() if edges else None
    h.select_edges_device(v.data_ptr(), v.shape[0], v.shape[1], k, 0, flags, o.cap if edges else 0, o.rank.data_ptr(),
                          o.rank_votes.data_ptr(), p(o.ea), p(o.eb), p(o.ev), o.counts.data_ptr(), stream)


def torch_route(v, k):
    """(edge_a, edge_b, values) as --retrieve makes them"""
    n_a, n_b = v.shape
    if n_a == n_b:
        v = v.masked_fill(torch.eye(n_a, dtype=torch.bool, device=v.device), -1)
    top = torch.topk(v.long(), k, dim=1)
    return torch.arange(n_a, dtype=torch.int32, device=v.device).repeat_interleave(k), top.indices.reshape(-1).int(), top.values


def torch_unique(v, k):
    ea, eb, _ = torch_route(v, k)
    lo, hi = torch.minimum(ea, eb).long(), torch.maximum(ea, eb).long()
    key = torch.unique(lo * v.shape[1] + hi)                                   # (synchronises: the size of the result)
    return (key // v.shape[1]).int(), (key % v.shape[1]).int()


def time_case(h, n_a, n_b, k, stream):
    v = vote_table(n_a, n_b, n_a + k)
    square = n_a == n_b
    o = Outputs(n_a, k)
    skip = lfp.SELECT_SKIP_SELF if square else 0
    call_select(h, v, k, skip, o, stream)
    torch.cuda.synchronize()
    _, _, values = torch_route(v, k)
    assert torch.equal(o.rank_votes.reshape(n_a, k).long(), values), "the call's votes and torch.topk's values differ"
    picks = int(o.counts[2])
    assert picks == n_a * k and int(o.counts[0]) == picks
    calls = {"select": lambda: call_select(h, v, k, skip, o, stream),
             "rank_only": lambda: call_select(h, v, k, skip, o, stream, edges=False),
             "torch": lambda: torch_route(v, k)}
    extra = {}
    if square:
        call_select(h, v, k, skip | lfp.SELECT_UNIQUE, o, stream)
        torch.cuda.synchronize()
        extra["unique_edges"] = int(o.counts[0])
        extra["torch_unique_edges"] = int(torch_unique(v, k)[0].numel())      # (differs only where torch.topk cut a tie elsewhere)
        calls["unique"] = lambda: call_select(h, v, k, skip | lfp.SELECT_UNIQUE, o, stream)
        calls["torch_unique"] = lambda: torch_unique(v, k)
    r = timed(calls)
    med = lambda name: r[name]["median_us"]
    if square:
        wall = []
        for it in range(WARMUP + TIMED):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            torch_unique(v, k)
            torch.cuda.synchronize()
            if it >= WARMUP:
                wall.append((time.perf_counter() - t0) * 1e6)
        extra["torch_unique_wall_median_us"] = round(statistics.median(wall), 1)
        extra["torch_unique_over_unique"] = round(med("torch_unique") / med("unique"), 2)
    ck, rows, groups, launches, scratch = lfp.select_edges_plan(n_a, n_b, k)
    return {"n_a": n_a, "n_b": n_b, "k": k, "compiled_k": ck, "rows_per_workgroup": rows, "workgroups": groups, "launches": launches,
            "scratch_bytes": scratch, "picks": picks, **extra, **{name + "_" + f: x[f] for name, x in r.items() for f in x},
            "torch_over_select": round(med("torch") / med("select"), 2),
            "read_gb_s": round(n_a * n_b * 4 / med("select") / 1e3, 1), "warmup": WARMUP, "timed": TIMED,
            "lib": os.path.basename(lfp.LIB_PATH)}


def time_matcher(h, stream):
    """match_q8_edges over --retrieve 4's list against --select 4's, on 64 images of about 2000 random rows"""
    n, k = 64, 4
    g = np.random.default_rng(0)
    q, o = pool(h, g.integers(1800, 2201, n), 1, stream)
    total = q.shape[0]
    v = vote_table(n, n, 3)
    ea_r, eb_r, _ = torch_route(v, k)
    out = Outputs(n, k)
    call_select(h, v, k, lfp.SELECT_SKIP_SELF | lfp.SELECT_UNIQUE, out, stream)
    torch.cuda.synchronize()
    kept = int(out.counts[0])
    new = lambda m: torch.empty((m,), dtype=torch.int32, device="cuda")
    calls, sizes = {}, {}
    for name, ea, eb in (("retrieve", ea_r.contiguous(), eb_r.contiguous()), ("select", out.ea, out.eb)):
        la, lb = layout(h, o, total, ea, stream), layout(h, o, total, eb, stream)
        torch.cuda.synchronize()
        cap_a, cap_b = int(la[-1]), int(lb[-1])
        bufs = (new(cap_a), new(cap_b), new(cap_a), new(cap_a))
        sizes[name] = (cap_a, cap_b)

        def run(ea=ea, eb=eb, la=la, lb=lb, cap_a=cap_a, cap_b=cap_b, bufs=bufs):
            h.match_q8_edges_device(q.data_ptr(), o.data_ptr(), n, total, q.data_ptr(), o.data_ptr(), n, total, ea.data_ptr(),
                                    eb.data_ptr(), la.data_ptr(), cap_a, ea.numel(), bufs[0].data_ptr(), lb.data_ptr(), cap_b,
                                    bufs[1].data_ptr(), 0.8, lfp.MATCH_MUTUAL, bufs[2].data_ptr(), bufs[3].data_ptr(), stream)
        calls[name] = run
    r = timed(calls)
    return {"images": n, "k": k, "pool_rows": total, "retrieve_edges": int(ea_r.numel()), "select_edges": kept,
            "select_entries": int(out.ea.numel()), "retrieve_layout": sizes["retrieve"], "select_layout": sizes["select"],
            **{name + "_" + f: x[f] for name, x in r.items() for f in x},
            "select_over_retrieve": round(r["select"]["median_us"] / r["retrieve"]["median_us"], 3)}


def main():
    torch.cuda.init()
    torch.cuda.set_stream(torch.cuda.Stream())
    s = torch.cuda.current_stream().cuda_stream
    h = lfp.MkdHandle(max_features=64)
    args = sys.argv[1:]
    if "--trace" in args:
        n, k = int(args[args.index("--trace") + 1]), int(args[args.index("--trace") + 2])
        v, o = vote_table(n, n, n + k), Outputs(n, k)
        for _ in range(20):
            call_select(h, v, k, lfp.SELECT_SKIP_SELF | lfp.SELECT_UNIQUE, o, s)
        torch.cuda.synchronize()
        print(json.dumps({"bench": "select_edges trace", "n": n, "k": k, "calls": 20}))
        return
    if "--matcher" in args:
        print(json.dumps({"bench": "select_edges matcher", **time_matcher(h, s)}), flush=True)
        return
    shapes = [(n, n, k) for n in (64, 1024, 16384) for k in (4, 8, 32)] + [(1, 1024, 8), (1, 65536, 8)]
    only = [int(a) for a in args if a.isdigit()]
    for n_a, n_b, k in shapes:
        if only and n_b not in only:
            continue
        print(json.dumps({"bench": "select_edges", **time_case(h, n_a, n_b, k, s)}), flush=True)


if __name__ == "__main__":
    main()
