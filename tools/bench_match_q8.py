#!/usr/bin/env python3
"""The int8 matcher against the f32 matcher, same rows, same process: lf_mkd_match_device and lf_mkd_match_q8_device (on the
rows' quantisation at scale 256) alternate launch by launch, each timed with HIP events -- 5 warm-up and 20 timed launches
each, the median is reported.  One JSON line per size: 2000 x 2000, 10 000 x 10 000, 65 536 x 65 536, 2^20 x 2^20.

    bench_match_q8.py                 every size, each in a child process of its own under its own time limit; stops at
                                      the first size that fails
    bench_match_q8.py --size NA NB    one size, in this process

The quantiser is timed as well (it is not part of the q8 figure: rows are quantised once and matched many times).  The
shader clock is that of a describe launch right after the timed loop (lf_mkd_kernel_clock measures describe launches only):
what the chip holds at that moment, not an average over the matcher's run.  Development aid; bench.py is the contract for
the headline metric."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((2000, 2000, 120), (10000, 10000, 120), (65536, 65536, 180), (1 << 20, 1 << 20, 420))   # (na, nb, time limit in s)
WARMUP, TIMED = 5, 20
I8_PEAK = 5.0e15     # dense int8 MFMA operations per second of an MI355X: twice the 2.5e15 of f16


def one_size(na, nb):
    sys.path.insert(0, os.path.join(ROOT, "local-features_amd"))
    import torch
    import local_features_python as lfp

    torch.cuda.set_stream(torch.cuda.Stream())
    h = lfp.MkdHandle(max_features=64, flags=lfp.FLAG_KERNEL_TIMING)
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(na + nb)
    a = torch.nn.functional.normalize(torch.randn((na, 128), device="cuda", generator=g), dim=1)
    b = torch.nn.functional.normalize(torch.randn((nb, 128), device="cuda", generator=g), dim=1)
    qa = torch.empty((na, 128), dtype=torch.uint8, device="cuda")
    qb = torch.empty((nb, 128), dtype=torch.uint8, device="cuda")
    m32 = torch.empty(na, dtype=torch.int32, device="cuda")
    m8 = torch.empty(na, dtype=torch.int32, device="cuda")
    patches = torch.rand((256, 32, 32), device="cuda")
    desc = torch.empty((256, 128), device="cuda")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        return e0, e1

    calls = {
        "f32": lambda: h.match_device(a.data_ptr(), na, b.data_ptr(), nb, m32.data_ptr(), 0.8, stream=s),
        "q8": lambda: h.match_q8_device(qa.data_ptr(), na, qb.data_ptr(), nb, m8.data_ptr(), 0.8, stream=s),
        "quantize": lambda: (h.quantize_descriptors_device(a.data_ptr(), na, qa.data_ptr(), stream=s),
                             h.quantize_descriptors_device(b.data_ptr(), nb, qb.data_ptr(), stream=s)),
    }
    calls["quantize"]()
    events = {k: [] for k in calls}
    for it in range(WARMUP + TIMED):
        for k, fn in calls.items():            # f32, q8, quantise; f32, q8, quantise; ...
            ev = timed(fn)
            if it >= WARMUP:
                events[k].append(ev)
    torch.cuda.synchronize()
    ms = {k: statistics.median(e0.elapsed_time(e1) for e0, e1 in v) for k, v in events.items()}
    h.describe_patches_device(patches.data_ptr(), 256, desc.data_ptr(), stream=s)
    mhz, _ = h.kernel_clock(s)
    a_blocks, splits, scratch = lfp.match_q8_plan(na, nb, torch.cuda.get_device_properties(0).multi_processor_count)
    pairs = float(na) * nb
    print(json.dumps({
        "na": na, "nb": nb, "f32_ms": round(ms["f32"], 4), "q8_ms": round(ms["q8"], 4), "quantize_ms": round(ms["quantize"], 4),
        "q8_over_f32_speed": round(ms["f32"] / ms["q8"], 3), "f32_pairs_per_s": pairs / (ms["f32"] * 1e-3),
        "q8_pairs_per_s": pairs / (ms["q8"] * 1e-3), "q8_fraction_of_i8_peak": round(pairs * 256 / (ms["q8"] * 1e-3) / I8_PEAK, 4),
        "q8_grid": [a_blocks, splits], "q8_scratch_bytes": scratch, "accepted_f32": int((m32 >= 0).sum()),
        "accepted_q8": int((m8 >= 0).sum()), "rows_redone_f32": h.match_overflowed(s), "shader_mhz_after": round(mhz, 1),
        "warmup": WARMUP, "timed": TIMED}), flush=True)


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--size":
        one_size(int(sys.argv[2]), int(sys.argv[3]))
        return 0
    for na, nb, limit in SIZES:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--size", str(na), str(nb)], timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"bench_match_q8: {na} x {nb} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
