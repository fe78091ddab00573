"""Driver of the camera resection call's host twin (tests/cpp/resect_twin.cpp): the kernels' own math header,
local-features_amd/csrc/mkd_resect_math.h, compiled by g++ and run under a serial restatement of the three kernels.

There is no arithmetic here.  This module only builds the program, writes its binary call files and reads its results.  A
call is a `scene` as tests/resect_cases.py makes them: a dict of the device call's arrays under its argument names (kps,
image_offsets, row_track, points, counts, intrinsics, poses; n_rows_total and track_capacity are the arrays' lengths)."""
import os
import struct
import subprocess

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "local-features_amd", "csrc")
NONE = 0xFFFFFFFF
FILL = 0x7FC0BEEF          # what the outputs hold where a call writes nothing (a NaN pattern no result has)
OUTPUTS = (("poses", 12), ("stats", 4), ("err", 2), ("row_state", 1))
DEFAULTS = dict(px=4.0, deg=0.0, n_samples=64, min_inliers=12, rounds=3, seed=0, flags=0)


def build(out_dir, extra=()):
    """g++ -std=c++17 -O2 -ffp-contract=off of the twin into out_dir; returns the program's path."""
    exe = os.path.join(str(out_dir), "resect_twin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", *extra, "-I", CSRC,
                           os.path.join(TESTS, "cpp", "resect_twin.cpp"), "-o", exe])
    return exe


def arrays(s):
    """the scene's arrays in the call's types: kps [rows, 5], offsets, row_track, points [T, 4], counts [2], intrinsics, poses"""
    counts = np.zeros(2, np.uint32)
    counts[0] = np.asarray(s["counts"]).reshape(-1)[0]
    return (np.ascontiguousarray(s["kps"], np.float32).reshape(-1, 5), np.ascontiguousarray(s["image_offsets"], np.uint64),
            np.ascontiguousarray(s["row_track"], np.int32), np.ascontiguousarray(s["points"], np.float32).reshape(-1, 4), counts,
            np.ascontiguousarray(s["intrinsics"], np.float32).reshape(-1, 4),
            np.ascontiguousarray(s["poses"], np.float32).reshape(-1, 12))


def _encode(s, fill, dump, px, deg, n_samples, min_inliers, rounds, seed, flags):
    kps, off, rt, pts, counts, intr, poses = arrays(s)
    assert len(off) == len(intr) + 1 and len(rt) == len(kps) and len(intr) == len(poses)
    head = struct.pack("<8IffQQ", len(intr), n_samples, min_inliers, rounds, seed & 0xFFFFFFFF, flags, fill, int(dump),
                       np.float32(px), np.float32(deg), len(kps), len(pts))
    return (b"".join([head, counts.tobytes(), kps.tobytes(), off.tobytes(), rt.tobytes(), pts.tobytes(), intr.tobytes(),
                      poses.tobytes()]), len(intr), len(kps), 4 * n_samples if dump else 0)


def run_calls(exe, tmp, calls, fill=FILL, dump=False):
    """calls = [(scene, {parameter: value})]: every call in one run of the program -> a list of dicts poses uint32 [n_images,
    12], stats [n_images, 4], err [n_images, 2], row_state [n_rows] (the outputs' words; view poses and err as float32 for
    their values) and, with dump, candidates float64 [n_images, 4 n_samples, 14] = valid, score, R, t."""
    enc = [_encode(s, fill, dump, **{**DEFAULTS, **kw}) for s, kw in calls]
    src, dst = os.path.join(str(tmp), "resect.in"), os.path.join(str(tmp), "resect.out")
    with open(src, "wb") as f:
        f.write(b"".join(e[0] for e in enc))
    done = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    with open(dst, "rb") as f:
        buf = f.read()
    out, at = [], 0
    for _, n_images, n_rows, n_cand in enc:
        r = {}
        for name, width in OUTPUTS:
            rows = n_rows if name == "row_state" else n_images
            r[name] = np.frombuffer(buf, "<u4", width * rows, at).reshape((rows, width) if width > 1 else (rows,))
            at += 4 * width * rows
        if dump:
            r["candidates"] = np.frombuffer(buf, "<f8", 14 * n_cand * n_images, at).reshape(n_images, n_cand, 14)
            at += 8 * 14 * n_cand * n_images
        out.append(r)
    assert at == len(buf), (at, len(buf))
    return out


def run(exe, tmp, scene, fill=FILL, dump=False, **kw):
    return run_calls(exe, tmp, [(scene, kw)], fill, dump)[0]


def f32(words):
    return np.ascontiguousarray(words).view(np.float32)
