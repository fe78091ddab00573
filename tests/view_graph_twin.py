"""Driver of the view-graph call's host twin (tests/cpp/view_graph_twin.cpp): the kernels' own math header,
local-features_amd/csrc/mkd_view_graph_math.h, compiled by g++ and run under a serial restatement of the kernels.

There is no arithmetic here.  This module only builds the program, writes its binary call files and reads its results.  A
call is a `scene` as tests/view_graph_cases.py makes them: a dict of the device call's arrays under its argument names
(edge_a, edge_b, R, pose_stats, n_images; optionally edge_offsets and match)."""
import os
import struct
import subprocess

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "local-features_amd", "csrc")
NONE = 0xFFFFFFFF
FILL = 0x7FC0BEEF          # what the outputs hold where a call writes nothing (a NaN pattern no result has)
OUTPUTS = (("rotations", 9), ("edge_stats", 4), ("residual", 1), ("image_stats", 4), ("counts", 8), ("match_out", 1))
DEFAULTS = dict(deg=3.0, min_front=0, root=NONE, tree_rounds=16, iterations=10, flags=0)


def build(out_dir, extra=()):
    """g++ -std=c++17 -O2 -ffp-contract=off of the twin into out_dir; returns the program's path."""
    exe = os.path.join(str(out_dir), "view_graph_twin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", *extra, "-I", CSRC,
                           os.path.join(TESTS, "cpp", "view_graph_twin.cpp"), "-o", exe])
    return exe


def arrays(s):
    """the scene's arrays in the call's types: edge_a, edge_b uint32 [E], R f32 [E, 9], pose_stats uint32 [E, 4], and the match
    filter's (edge_offsets uint64 [E + 1], match int32) or (None, None)"""
    ea, eb = np.ascontiguousarray(s["edge_a"], np.uint32).reshape(-1), np.ascontiguousarray(s["edge_b"], np.uint32).reshape(-1)
    R, ps = np.ascontiguousarray(s["R"], np.float32).reshape(-1, 9), np.ascontiguousarray(s["pose_stats"], np.uint32).reshape(-1, 4)
    assert len(eb) == len(ea) == len(R) == len(ps)
    if s.get("match") is None:
        return ea, eb, R, ps, None, None
    off, m = np.ascontiguousarray(s["edge_offsets"], np.uint64).reshape(-1), np.ascontiguousarray(s["match"], np.int32).reshape(-1)
    assert len(off) == len(ea) + 1
    return ea, eb, R, ps, off, m


def rows(s):
    """rows of every output of a call on scene s (match_out: 0 without a match array)"""
    E, n = len(np.asarray(s["edge_a"]).reshape(-1)), int(s["n_images"])
    return {"rotations": n, "edge_stats": E, "residual": E, "image_stats": n, "counts": 1,
            "match_out": 0 if s.get("match") is None else len(np.asarray(s["match"]).reshape(-1))}


def _encode(s, fill, match, residual, deg, min_front, root, tree_rounds, iterations, flags):
    ea, eb, R, ps, off, m = arrays(s)
    with_match = 0 if m is None or not match else 2 if match == "in place" else 1
    head = struct.pack("<10IffQ", int(s["n_images"]), len(ea), min_front, root, tree_rounds, iterations, flags, fill, with_match,
                       int(residual), np.float32(deg), 0.0, len(m) if with_match else 0)
    parts = [head, ea.tobytes(), eb.tobytes(), R.tobytes(), ps.tobytes()]
    if with_match:
        parts += [off.tobytes(), m.tobytes()]
    r = rows(s)
    if not with_match:
        r["match_out"] = 0
    return b"".join(parts), r


def run_calls(exe, tmp, calls, fill=FILL):
    """calls = [(scene, {parameter: value})] (besides DEFAULTS' parameters: match = True / False / "in place", residual = True /
    False): every call in one run of the program -> a list of dicts of the outputs' words (uint32; view rotations and residual
    as float32 for their values): rotations [n_images, 9], edge_stats [E, 4], residual [E], image_stats [n_images, 4], counts
    [8], match_out [entries]."""
    enc = []
    for s, kw in calls:
        kw = dict(kw)
        match, residual = kw.pop("match", True), kw.pop("residual", True)
        enc.append(_encode(s, fill, match, residual, **{**DEFAULTS, **kw}))
    src, dst = os.path.join(str(tmp), "view_graph.in"), os.path.join(str(tmp), "view_graph.out")
    with open(src, "wb") as f:
        f.write(b"".join(e[0] for e in enc))
    done = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    with open(dst, "rb") as f:
        buf = f.read()
    out, at = [], 0
    for _, r in enc:
        res = {}
        for name, width in OUTPUTS:
            n = r[name]
            res[name] = np.frombuffer(buf, "<u4", width * n, at).reshape((n, width) if width > 1 and name != "counts" else (width * n,))
            at += 4 * width * n
        out.append(res)
    assert at == len(buf), (at, len(buf))
    return out


def run(exe, tmp, scene, fill=FILL, **kw):
    return run_calls(exe, tmp, [(scene, kw)], fill)[0]


def f32(words):
    return np.ascontiguousarray(words).view(np.float32)
