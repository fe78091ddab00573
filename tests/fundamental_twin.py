"""Driver of the fundamental-matrix verifier's host twin (tests/cpp/fundamental_twin.cpp): the kernel's own math header,
local-features_amd/csrc/mkd_fundamental_math.h, compiled by g++ and run under a serial restatement of the two kernels.

There is no f32 emulation here.  This module only builds the program, writes its binary problem files and reads its
results.  The considered rows and the pair's normalisation (what the kernels' first launch, verify_prepare, computes) come
from tests/homography_f32.py's Pair, which tests/test_gpu_homography_exact.py holds to the device bit for bit."""
import os
import struct
import subprocess

import numpy as np

import homography_f32 as h32

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "local-features_amd", "csrc")
INVALID = 0xFFFFFFFF
NO_REFINE = 1

_REC = np.dtype([("pos", "<u4", 7), ("valid", "<u4"), ("f", "<f4", (3, 9)), ("fn", "<f4", (3, 9)), ("count", "<u4", 3)])


def build(out_dir):
    """g++ -std=c++17 -O2 -ffp-contract=off of the twin into out_dir; returns the program's path."""
    exe = os.path.join(str(out_dir), "fundamental_twin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", CSRC,
                           os.path.join(TESTS, "cpp", "fundamental_twin.cpp"), "-o", exe])
    return exe


class Call:
    """One pair and the calls wanted of it: `seeds` (each is seed + p of a batched call), n_hyp, thr, flags; records = every
    sample's positions, valid bits, candidates and counts as well."""

    def __init__(self, kps_a, kps_b, match, seeds, n_hyp, thr, flags=0, records=False):
        self.ka = np.ascontiguousarray(kps_a, np.float32).reshape(-1, 5)
        self.kb = np.ascontiguousarray(kps_b, np.float32).reshape(-1, 5)
        self.match = np.ascontiguousarray(match, np.int32).reshape(-1)
        self.seeds = np.atleast_1d(np.asarray(seeds, np.int64) & 0xFFFFFFFF).astype(np.uint32)
        self.n_hyp, self.thr, self.flags, self.records = int(n_hyp), float(thr), int(flags), bool(records)
        self.pair = h32.Pair(self.ka, self.kb, self.match)

    def encode(self):
        p = self.pair
        head = struct.pack("<8If", 1, len(self.match), len(self.kb), p.m, len(self.seeds), self.n_hyp, self.flags,
                           int(self.records), self.thr)
        vp = np.array([p.ca[0], p.ca[1], p.sa, p.cb[0], p.cb[1], p.sb], np.float32).tobytes() + struct.pack("<2I", p.m, 0)
        return b"".join([head, vp, self.ka.tobytes(), self.kb.tobytes(), self.match.tobytes(),
                         p.rows.astype(np.int32).tobytes(), self.seeds.tobytes()])

    def decode(self, buf, at):
        """-> (list of one dict per seed, the position after them)"""
        na, out = len(self.match), []
        for seed in self.seeds:
            r = {"seed": int(seed), "pair": self.pair}
            r["F"] = np.frombuffer(buf, "<f4", 9, at).reshape(3, 3)
            r["stats"] = np.frombuffer(buf, "<u4", 4, at + 36)
            r["verified"] = np.frombuffer(buf, "<i4", na, at + 52)
            at += 52 + 4 * na
            if self.records:
                r["records"] = np.frombuffer(buf, _REC, self.n_hyp, at)
                at += _REC.itemsize * self.n_hyp
            out.append(r)
        return out, at


def _run(exe, payload, tmp):
    src, dst = os.path.join(str(tmp), "twin.in"), os.path.join(str(tmp), "twin.out")
    with open(src, "wb") as f:
        f.write(payload)
    done = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    with open(dst, "rb") as f:
        return f.read()


def run_calls(exe, calls, tmp):
    """Every call in one run of the program: a list (one entry per call) of lists (one dict per seed)."""
    buf = _run(exe, b"".join(c.encode() for c in calls), tmp)
    out, at = [], 0
    for c in calls:
        res, at = c.decode(buf, at)
        out.append(res)
    assert at == len(buf), (at, len(buf))
    return out


def verify(exe, tmp, kps_a, kps_b, match, n_hyp, thr, seed=0, flags=0, records=False):
    """One pair, one seed: dict with F f32 [3, 3], verified int32 [na], stats uint32 [4], pair, and `records` if asked."""
    return run_calls(exe, [Call(kps_a, kps_b, match, seed, n_hyp, thr, flags, records)], tmp)[0][0]


def cubic_roots(exe, tmp, coeffs):
    """cubic_roots() of rows (c0, c1, c2, c3) f32 -> (number of roots [n], x f32 [n, 3])."""
    c = np.ascontiguousarray(coeffs, np.float32).reshape(-1, 4)
    buf = _run(exe, struct.pack("<2I", 2, len(c)) + c.tobytes(), tmp)
    r = np.frombuffer(buf, np.dtype([("n", "<u4"), ("x", "<f4", 3)]), len(c))
    return r["n"].astype(np.int64), r["x"]


def null_space(exe, tmp, systems):
    """null_space() of 7 x 9 systems f32 -> (ok [n], F1 f32 [n, 9], F2 f32 [n, 9])."""
    a = np.ascontiguousarray(systems, np.float32).reshape(-1, 63)
    buf = _run(exe, struct.pack("<2I", 3, len(a)) + a.tobytes(), tmp)
    r = np.frombuffer(buf, np.dtype([("ok", "<u4"), ("f1", "<f4", 9), ("f2", "<f4", 9)]), len(a))
    return r["ok"].astype(bool), r["f1"], r["f2"]
