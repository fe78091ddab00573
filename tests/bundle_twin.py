"""Driver of the bundle adjustment call's host twin (tests/cpp/bundle_twin.cpp): the kernels' own math header,
local-features_amd/csrc/mkd_bundle_math.h, compiled by g++ and run under a serial restatement of the kernels.

There is no arithmetic here.  This module only builds the program, writes its binary call files and reads its results.  A
call is a `scene` as tests/bundle_cases.py makes them: a dict of the device call's arrays under its argument names (kps,
image_offsets, track_offsets, obs_row, obs_image, counts, points, intrinsics, poses, and obs_state / camera_fixed or None;
n_rows_total, track_capacity and obs_capacity are the arrays' lengths)."""
import os
import struct
import subprocess

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "local-features_amd", "csrc")
FILL = 0x7FC0BEEF          # what the outputs hold where a call writes nothing (a NaN pattern no result has)
DEFAULTS = dict(px=4.0, lambda0=1e-3, iterations=4, cg_iterations=8, cg_tol=0.1)
TRACE = ("cost", "cost_new", "lambda", "accepted", "cg_steps", "inliers", "held_cameras", "held_points")


def build(out_dir, extra=()):
    """g++ -std=c++17 -O2 -ffp-contract=off of the twin into out_dir; returns the program's path."""
    exe = os.path.join(str(out_dir), "bundle_twin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", *extra, "-I", CSRC,
                           os.path.join(TESTS, "cpp", "bundle_twin.cpp"), "-o", exe])
    return exe


def arrays(s):
    """the scene's arrays in the call's types, as a dict"""
    c = np.zeros(2, np.uint32)
    c[:] = np.asarray(s["counts"]).reshape(-1)[:2]
    opt = lambda k: None if s.get(k) is None else np.ascontiguousarray(s[k], np.uint32).reshape(-1)
    a = dict(kps=np.ascontiguousarray(s["kps"], np.float32).reshape(-1, 5),
             image_offsets=np.ascontiguousarray(s["image_offsets"], np.uint64).reshape(-1),
             track_offsets=np.ascontiguousarray(s["track_offsets"], np.uint64).reshape(-1),
             obs_row=np.ascontiguousarray(s["obs_row"], np.int32).reshape(-1),
             obs_image=np.ascontiguousarray(s["obs_image"], np.uint32).reshape(-1), counts=c,
             points=np.ascontiguousarray(s["points"], np.float32).reshape(-1, 4),
             intrinsics=np.ascontiguousarray(s["intrinsics"], np.float32).reshape(-1, 4),
             poses=np.ascontiguousarray(s["poses"], np.float32).reshape(-1, 12), obs_state=opt("obs_state"),
             camera_fixed=opt("camera_fixed"))
    n, t, o = len(a["intrinsics"]), len(a["points"]), len(a["obs_row"])
    assert len(a["image_offsets"]) == n + 1 and len(a["track_offsets"]) == t + 1 and len(a["obs_image"]) == o and len(a["poses"]) == n
    assert a["obs_state"] is None or len(a["obs_state"]) == o
    assert a["camera_fixed"] is None or len(a["camera_fixed"]) == n
    return a


def _encode(s, fill, dump, px, lambda0, iterations, cg_iterations, cg_tol):
    a = arrays(s)
    has = (1 if a["obs_state"] is not None else 0) | (2 if a["camera_fixed"] is not None else 0)
    n, rows, t, o = len(a["intrinsics"]), len(a["kps"]), len(a["points"]), len(a["obs_row"])
    head = struct.pack("<8I4f3Q", n, iterations, cg_iterations, has, fill, int(dump), 0, 0, np.float32(px), np.float32(lambda0),
                       np.float32(cg_tol), 0.0, rows, t, o)
    parts = [head] + [a[k].tobytes() for k in ("counts", "kps", "image_offsets", "track_offsets", "obs_row", "obs_image", "points",
                                               "intrinsics", "poses")]
    parts += [a[k].tobytes() for k in ("obs_state", "camera_fixed") if a[k] is not None]
    return b"".join(parts), n, t, o, iterations, bool(dump)


def run_calls(exe, tmp, calls, fill=FILL, dump=False):
    """calls = [(scene, {parameter: value})]: every call in one run of the program -> a list of dicts poses uint32 [n_images,
    12], points uint32 [track_capacity, 4], obs_state uint32 [obs_capacity] (the outputs' words), trace float64 [iterations,
    8] (as uint64 words under "trace_words" too), counts uint32 [4] and, with dump, x float64 [n_images, 6]."""
    enc = [_encode(s, fill, dump, **{**DEFAULTS, **kw}) for s, kw in calls]
    src, dst = os.path.join(str(tmp), "bundle.in"), os.path.join(str(tmp), "bundle.out")
    with open(src, "wb") as f:
        f.write(b"".join(e[0] for e in enc))
    done = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    with open(dst, "rb") as f:
        buf = f.read()
    out, at = [], 0
    for _, n, t, o, iters, dumped in enc:
        r = {}
        for name, count, shape in (("poses", 12 * n, (n, 12)), ("points", 4 * t, (t, 4)), ("obs_state", o, (o,))):
            r[name] = np.frombuffer(buf, "<u4", count, at).reshape(shape)
            at += 4 * count
        r["trace_words"] = np.frombuffer(buf, "<u8", 8 * iters, at).reshape(iters, 8)
        r["trace"] = r["trace_words"].view(np.float64)
        at += 64 * iters
        r["counts"] = np.frombuffer(buf, "<u4", 4, at)
        at += 16
        if dumped:
            r["x"] = np.frombuffer(buf, "<f8", 6 * n, at).reshape(n, 6)
            at += 48 * n
        out.append(r)
    assert at == len(buf), (at, len(buf))
    return out


def run(exe, tmp, scene, fill=FILL, dump=False, **kw):
    return run_calls(exe, tmp, [(scene, kw)], fill, dump)[0]


def f32(words):
    return np.ascontiguousarray(words).view(np.float32)
