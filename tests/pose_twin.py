"""Driver of the two-view pose call's host twin (tests/cpp/pose_twin.cpp): the kernel's own math header,
local-features_amd/csrc/mkd_pose_math.h, compiled by g++ and run under a serial restatement of the kernel's workgroup.

There is no arithmetic here.  This module only builds the program, writes its binary call files and reads its results.  A
call is a `table` as tests/pose_cases.py makes them: a dict of the device call's arrays under its argument names."""
import os
import struct
import subprocess

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "local-features_amd", "csrc")
NONE = 0xFFFFFFFF
FILL = 0x7FC0BEEF          # what the outputs hold where a call writes nothing (a NaN pattern no result has)


def build(out_dir):
    """g++ -std=c++17 -O2 -ffp-contract=off of the twin into out_dir; returns the program's path."""
    exe = os.path.join(str(out_dir), "pose_twin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", CSRC,
                           os.path.join(TESTS, "cpp", "pose_twin.cpp"), "-o", exe])
    return exe


def _encode(t, deg, fill):
    kps = np.ascontiguousarray(t["kps"], np.float32).reshape(-1, 5)
    ea, eb = np.ascontiguousarray(t["edge_a"], np.uint32), np.ascontiguousarray(t["edge_b"], np.uint32)
    intr = np.ascontiguousarray(t["intrinsics"], np.float32).reshape(-1, 4)
    f = np.ascontiguousarray(t["F"], np.float32).reshape(-1, 9)
    off = np.ascontiguousarray(t["link_offsets"], np.uint64)
    la, lb = np.ascontiguousarray(t["link_a"], np.int32), np.ascontiguousarray(t["link_b"], np.int32)
    cap = int(t.get("link_capacity", len(la)))
    assert len(ea) == len(eb) == len(f) == len(off) - 1 and len(la) >= cap and len(lb) >= cap
    head = struct.pack("<3IfQQ", len(ea), len(intr), fill, np.float32(deg), len(kps), cap)
    return b"".join([head, kps.tobytes(), ea.tobytes(), eb.tobytes(), intr.tobytes(), f.tobytes(), off.tobytes(),
                     la[:cap].tobytes(), lb[:cap].tobytes()]), len(ea), cap


def run_calls(exe, tmp, calls, fill=FILL):
    """calls = [(table, min_parallax_deg)]: every call in one run of the program -> a list of dicts R uint32 [n, 9], t [n, 3],
    stats [n, 4], sigma [n, 3], points [link_capacity, 4]: the outputs' words (view them as float32 for their values)."""
    enc = [_encode(t, deg, fill) for t, deg in calls]
    src, dst = os.path.join(str(tmp), "pose.in"), os.path.join(str(tmp), "pose.out")
    with open(src, "wb") as f:
        f.write(b"".join(e[0] for e in enc))
    done = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    with open(dst, "rb") as f:
        buf = f.read()
    out, at = [], 0
    for _, n, cap in enc:
        r = {}
        for name, width, rows in (("R", 9, n), ("t", 3, n), ("stats", 4, n), ("sigma", 3, n), ("points", 4, cap)):
            r[name] = np.frombuffer(buf, "<u4", width * rows, at).reshape(rows, width)
            at += 4 * width * rows
        out.append(r)
    assert at == len(buf), (at, len(buf))
    return out


def run(exe, tmp, table, deg, fill=FILL):
    return run_calls(exe, tmp, [(table, deg)], fill)[0]


def f32(words):
    return np.ascontiguousarray(words).view(np.float32)
