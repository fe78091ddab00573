"""Driver of the host twin of lf_mkd_bundle_adjust_intrinsics_device (tests/cpp/bundle_intr_twin.cpp): the kernels' own math
header, local-features_amd/csrc/mkd_bundle_math.h, compiled by g++ and run under a serial restatement of the kernels.

There is no arithmetic here.  A call is a `scene` as tests/bundle_cases.py makes them (tests/bundle_twin.py: arrays) with an
optional `camera_group` (uint32 [n_images] or None) and `n_groups` (default 1), and the parameters of DEFAULTS."""
import os
import struct
import subprocess

import numpy as np

import bundle_twin as bt

FILL = bt.FILL
DEFAULTS = dict(bt.DEFAULTS, refine=1)
TRACE = bt.TRACE + ("held_groups",)
OUTPUTS = ("poses", "points", "intrinsics", "groups", "obs_state", "trace", "counts")


def build(out_dir, extra=()):
    """g++ -std=c++17 -O2 -ffp-contract=off of the twin into out_dir; returns the program's path."""
    exe = os.path.join(str(out_dir), "bundle_intr_twin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", *extra, "-I", bt.CSRC,
                           os.path.join(bt.TESTS, "cpp", "bundle_intr_twin.cpp"), "-o", exe])
    return exe


def arrays(s):
    """the scene's arrays in the call's types, with camera_group (or None) and n_groups"""
    a = bt.arrays(s)
    g = s.get("camera_group")
    a["camera_group"] = None if g is None else np.ascontiguousarray(g, np.uint32).reshape(-1)
    assert a["camera_group"] is None or len(a["camera_group"]) == len(a["intrinsics"])
    a["n_groups"] = int(s.get("n_groups", 1))
    return a


def _encode(s, fill, dump, px, lambda0, iterations, cg_iterations, cg_tol, refine):
    a = arrays(s)
    has = (1 if a["obs_state"] is not None else 0) | (2 if a["camera_fixed"] is not None else 0) | (4 if a["camera_group"] is not None else 0)
    n, rows, t, o = len(a["intrinsics"]), len(a["kps"]), len(a["points"]), len(a["obs_row"])
    head = struct.pack("<8I4f3Q", n, iterations, cg_iterations, has, fill, int(dump), a["n_groups"], refine, np.float32(px),
                       np.float32(lambda0), np.float32(cg_tol), 0.0, rows, t, o)
    parts = [head] + [a[k].tobytes() for k in ("counts", "kps", "image_offsets", "track_offsets", "obs_row", "obs_image", "points",
                                               "intrinsics", "poses")]
    parts += [a[k].tobytes() for k in ("obs_state", "camera_fixed", "camera_group") if a[k] is not None]
    return b"".join(parts), n, t, o, iterations, bool(dump), a["n_groups"]


def run_calls(exe, tmp, calls, fill=FILL, dump=False):
    """calls = [(scene, {parameter: value})] in one run of the program -> a list of dicts of the outputs' words: poses uint32
    [n_images, 12], points [track_capacity, 4], intrinsics [n_images, 4], groups [n_groups, 3], obs_state [obs_capacity],
    trace float64 [iterations, 9] ("trace_words": the same as uint64), counts uint32 [5] and, with dump, x float64 [n_images,
    6] and xg [n_groups, 3]."""
    enc = [_encode(s, fill, dump, **{**DEFAULTS, **kw}) for s, kw in calls]
    src, dst = os.path.join(str(tmp), "bundle_intr.in"), os.path.join(str(tmp), "bundle_intr.out")
    with open(src, "wb") as f:
        f.write(b"".join(e[0] for e in enc))
    done = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    with open(dst, "rb") as f:
        buf = f.read()
    out, at = [], 0
    for _, n, t, o, iters, dumped, ng in enc:
        r = {}
        for name, count, shape in (("poses", 12 * n, (n, 12)), ("points", 4 * t, (t, 4)), ("intrinsics", 4 * n, (n, 4)),
                                   ("groups", 3 * ng, (ng, 3)), ("obs_state", o, (o,))):
            r[name] = np.frombuffer(buf, "<u4", count, at).reshape(shape)
            at += 4 * count
        r["trace_words"] = np.frombuffer(buf, "<u8", 9 * iters, at).reshape(iters, 9)
        r["trace"] = r["trace_words"].view(np.float64)
        at += 72 * iters
        r["counts"] = np.frombuffer(buf, "<u4", 5, at)
        at += 20
        if dumped:
            r["x"] = np.frombuffer(buf, "<f8", 6 * n, at).reshape(n, 6)
            at += 48 * n
            r["xg"] = np.frombuffer(buf, "<f8", 3 * ng, at).reshape(ng, 3)
            at += 24 * ng
        out.append(r)
    assert at == len(buf), (at, len(buf))
    return out


def run(exe, tmp, scene, fill=FILL, dump=False, **kw):
    return run_calls(exe, tmp, [(scene, kw)], fill, dump)[0]


f32 = bt.f32
