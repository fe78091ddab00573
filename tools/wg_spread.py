#!/usr/bin/env python3
"""Per-workgroup clock of one patch-mode describe launch (development aid): who starts when, who ends when.
Needs a library built with -DLF_WG_CLOCK (tools/ab_build.sh NAME "-DLF_WG_CLOCK", LF_MKD_LIB=ab/liblf_mkd_NAME.so): every
workgroup leaves its entry and exit stamps of the constant 100 MHz clock, its batch count and its XCD behind the
descriptors.  tools/wg_spread.py [n [angle_mode]] prints the start skew, the end spread relative to workgroup 0's exit,
the mean duration per XCD and the batches-per-workgroup histogram of the LAST of three launches."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-features_amd"))
import numpy as np
import torch
import local_features_python as lfp

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
angles = [int(sys.argv[2])] if len(sys.argv) > 2 else [lfp.ANGLE_SHADER, lfp.ANGLE_EXACT_ZERO]
cus = torch.cuda.get_device_properties(0).multi_processor_count
grid = min((n + 127) // 128, cus)
p = torch.rand((n, 32, 32), device="cuda")
out = torch.zeros(n * 128 + 8 * grid, device="cuda")
TICK_US = 0.01   # s_memrealtime counts at 100 MHz
print(f"library {os.path.basename(lfp.LIB_PATH)}; n = {n}, {(n + 127) // 128} batches of 128, grid {grid}")
for angle in angles:
    h = lfp.MkdHandle(max_features=n, angle_mode=angle, pool_mode=lfp.POOL_F16X3)
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(3):
        out[n * 128:].zero_()
        h.describe_patches_device(p.data_ptr(), n, out.data_ptr(), s)
    torch.cuda.synchronize()
    rec = out[n * 128:].view(torch.int32).cpu().numpy().view(np.uint32).reshape(grid, 8).astype(np.uint64)
    t_in = (rec[:, 0] | (rec[:, 1] << np.uint64(32))).astype(np.int64)
    t_out = (rec[:, 2] | (rec[:, 3] << np.uint64(32))).astype(np.int64)
    nb, xcd = rec[:, 4].astype(np.int64), rec[:, 5].astype(np.int64)
    if not t_in.all() or not t_out.all():
        sys.exit("no stamps: is LF_MKD_LIB a -DLF_WG_CLOCK build?")
    t0 = t_in.min()
    dur = (t_out - t_in) * TICK_US
    rel = (t_out - t_out[0]) * TICK_US                 # exit relative to workgroup 0's
    batch_us = float(np.median(dur / nb))
    late = float((t_out.max() - np.median(t_out)) * TICK_US)
    print(f"angle={angle}: launch (first entry to last exit) {(t_out.max() - t0) * TICK_US:.1f} us; "
          f"workgroup 0: {dur[0]:.1f} us; one batch (median) {batch_us:.1f} us")
    print(f"  start skew (first to last entry)   {(t_in.max() - t0) * TICK_US:8.1f} us   "
          f"(median {float(np.median(t_in - t0)) * TICK_US:.1f} us)")
    print(f"  exit - workgroup 0's exit: min {rel.min():8.1f}  median {float(np.median(rel)):8.1f}  "
          f"p95 {float(np.percentile(rel, 95)):8.1f}  last {rel.max():8.1f} us")
    print(f"  last exit - median exit            {late:8.1f} us = {late / batch_us:.2f} batch times "
          f"(workgroup {int(t_out.argmax())}, XCD {int(xcd[t_out.argmax()])}, {int(nb[t_out.argmax()])} batches)")
    print(f"  idle CU time before the last exit  {float((t_out.max() - t_out).mean()) * TICK_US:8.1f} us per workgroup (mean)")
    for x in sorted(set(xcd.tolist())):
        m = xcd == x
        print(f"  XCD {x}: {int(m.sum()):3d} workgroups, mean duration {dur[m].mean():8.1f} us, mean batches {nb[m].mean():6.2f}, "
              f"per batch {float((dur[m] / nb[m]).mean()):.2f} us, mean entry {float((t_in[m] - t0).mean()) * TICK_US:6.1f} us, "
              f"last exit {rel[m].max():7.1f} us")
    vals, cnt = np.unique(nb, return_counts=True)
    print("  batches per workgroup: " + ", ".join(f"{int(v)}: {int(c)}" for v, c in zip(vals, cnt)))
