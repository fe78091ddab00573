"""Driver of the host twin of the tree-pose and global-positioning calls (tests/cpp/positions_twin.cpp): the kernels' own
math header, local-features_amd/csrc/mkd_positions_math.h, compiled by g++ and run under a serial restatement of the kernels.

There is no arithmetic here.  This module only builds the program, writes its binary call files and reads its results.  A
call is a scene as tests/positions_cases.py makes them: a dict of the device call's arrays under its argument names."""
import os
import struct
import subprocess

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "local-features_amd", "csrc")
NONE = 0xFFFFFFFF
FILL = 0x7FC0BEEF          # what the outputs hold where a call writes nothing (a NaN pattern no result has)
DEFAULTS = dict(sweeps=50, warm=3, robust_deg=0.2, min_obs=2)


def build(out_dir, extra=()):
    """g++ -std=c++17 -O2 -ffp-contract=off of the twin into out_dir; returns the program's path."""
    exe = os.path.join(str(out_dir), "positions_twin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", *extra, "-I", CSRC,
                           os.path.join(TESTS, "cpp", "positions_twin.cpp"), "-o", exe])
    return exe


def arrays(s):
    """the scene's arrays in the call's types: kps f32 [rows, 5], image_offsets uint64 [n + 1], track_offsets uint64
    [track_capacity + 1], obs_row int32 / obs_image uint32 [obs_capacity], counts uint32 [2], row_track int32 [rows],
    intrinsics f32 [n, 4], poses f32 [n, 12]"""
    c = np.ascontiguousarray
    return (c(s["kps"], np.float32).reshape(-1, 5), c(s["image_offsets"], np.uint64).reshape(-1),
            c(s["track_offsets"], np.uint64).reshape(-1), c(s["obs_row"], np.int32).reshape(-1),
            c(s["obs_image"], np.uint32).reshape(-1), c(s["counts"], np.uint32).reshape(2), c(s["row_track"], np.int32).reshape(-1),
            c(s["intrinsics"], np.float32).reshape(-1, 4), c(s["poses"], np.float32).reshape(-1, 12))


def tree_arrays(s):
    c = np.ascontiguousarray
    return (c(s["edge_a"], np.uint32).reshape(-1), c(s["edge_b"], np.uint32).reshape(-1), c(s["t"], np.float32).reshape(-1, 3),
            c(s["rotations"], np.float32).reshape(-1, 9), c(s["image_stats"], np.uint32).reshape(-1, 4))


def _encode(s, fill, points, state, trace, sweeps, warm, robust_deg, min_obs):
    kps, ioff, toff, row, img, tc, rt, K, P = arrays(s)
    n = len(K)
    head = struct.pack("<10IffQQQ", 1, n, sweeps, warm, min_obs, fill, int(points), int(state), int(trace), 0, np.float32(robust_deg), 0.0,
                       len(kps), len(toff) - 1, len(row))
    blob = b"".join([head, tc.tobytes(), ioff.tobytes(), toff.tobytes(), kps.tobytes(), rt.tobytes(), row.tobytes(), img.tobytes(),
                     K.tobytes(), P.tobytes()])
    layout = [("poses", "<u4", (n, 12)), ("points", "<u4", (len(toff) - 1 if points else 0, 4)),
              ("obs_state", "<u4", (len(row) if state else 0,)), ("image_stats", "<u4", (n, 4)),
              ("trace", "<f8", (sweeps if trace else 0, 4)), ("counts", "<u4", (8,))]
    return blob, layout


def _encode_tree(s, fill, max_depth):
    ea, eb, t, rot, st = tree_arrays(s)
    head = struct.pack("<5I", 0, len(rot), len(ea), max_depth, fill)
    return b"".join([head, ea.tobytes(), eb.tobytes(), t.tobytes(), rot.tobytes(), st.tobytes()]), [("poses", "<u4", (len(rot), 12))]


def _run(exe, tmp, enc):
    src, dst = os.path.join(str(tmp), "positions.in"), os.path.join(str(tmp), "positions.out")
    with open(src, "wb") as f:
        f.write(b"".join(e[0] for e in enc))
    done = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    with open(dst, "rb") as f:
        buf = f.read()
    out, at = [], 0
    for _, layout in enc:
        res = {}
        for name, dtype, shape in layout:
            count = int(np.prod(shape))
            res[name] = np.frombuffer(buf, dtype, count, at).reshape(shape)
            at += count * np.dtype(dtype).itemsize
        out.append(res)
    assert at == len(buf), (at, len(buf))
    return out


def run_calls(exe, tmp, calls, fill=FILL):
    """calls = [(scene, {parameter: value})] (DEFAULTS' parameters; points, state, trace = True / False): every call in one run
    of the program -> a list of dicts of the outputs' words: poses uint32 [n, 12], points uint32 [track_capacity, 4],
    obs_state uint32 [obs_capacity], image_stats uint32 [n, 4], trace float64 [sweeps, 4], counts uint32 [8]."""
    enc = []
    for s, kw in calls:
        kw = dict(kw)
        points, state, trace = kw.pop("points", True), kw.pop("state", True), kw.pop("trace", True)
        enc.append(_encode(s, fill, points, state, trace, **{**DEFAULTS, **kw}))
    return _run(exe, tmp, enc)


def run(exe, tmp, scene, fill=FILL, **kw):
    return run_calls(exe, tmp, [(scene, kw)], fill)[0]


def run_tree(exe, tmp, scene, max_depth=64, fill=FILL):
    """-> poses uint32 [n_images, 12]"""
    return _run(exe, tmp, [_encode_tree(scene, fill, max_depth)])[0]["poses"]


def f32(words):
    return np.ascontiguousarray(words).view(np.float32)
