"""Driver of the screen matcher's host twin (tests/cpp/match_twin.cpp): an exhaustive scan with match_verify's own f32 dot
product (one product and seven fmaf per lane over 8 contiguous elements, then the fixed tree p += p[l ^ m], m = 8, 4, 2, 1)
and verify's rule for best, second, index and the ratio test.

There is no arithmetic here.  This module only builds the program, writes its binary problem file and reads its results."""
import os
import struct
import subprocess

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
MAGIC = 0x3157544D           # "MTW1"
EXCLUDE, WIDE = 1, 2
THREADS = 16                 # the program uses no more, whatever it is asked for


def build(out_dir):
    """g++ -std=c++17 -O2 -ffp-contract=off of the twin into out_dir; returns the program's path."""
    exe = os.path.join(str(out_dir), "match_twin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread",
                           os.path.join(TESTS, "cpp", "match_twin.cpp"), "-o", exe])
    return exe


class Scan:
    """What the twin says of one problem: match int32 [na], best / second float32 [na]; with wide=True also best64 /
    second64 (the row's two largest similarities in float64) and sabs (the row's largest sum |a_k b_k|), float64 [na]."""

    def __init__(self, match, best, second, best64=None, second64=None, sabs=None):
        self.match, self.best, self.second = match, best, second
        self.best64, self.second64, self.sabs = best64, second64, sabs

    def bits(self):
        """(match, best as int32 bits, second as int32 bits)"""
        return self.match, self.best.view(np.int32), self.second.view(np.int32)


_N_RUNS = [0]


def scan(exe, tmp, a, b, ratio=0.8, lo=None, hi=None, wide=False):
    """The exhaustive scan of a [na, 128] against b [nb, 128] (float32), b[lo[i]:hi[i]] skipped for a[i]."""
    a = np.ascontiguousarray(a, "<f4").reshape(-1, 128)
    b = np.ascontiguousarray(b, "<f4").reshape(-1, 128)
    na, nb = len(a), len(b)
    flags = (EXCLUDE if lo is not None else 0) | (WIDE if wide else 0)
    _N_RUNS[0] += 1
    src = os.path.join(str(tmp), f"match_twin_{_N_RUNS[0]}.in")
    dst = os.path.join(str(tmp), f"match_twin_{_N_RUNS[0]}.out")
    with open(src, "wb") as f:
        f.write(struct.pack("<4IfI", MAGIC, na, nb, flags, ratio, THREADS))
        f.write(a.tobytes())
        f.write(b.tobytes())
        if lo is not None:
            f.write(np.ascontiguousarray(lo, "<u4").reshape(na).tobytes())
            f.write(np.ascontiguousarray(hi, "<u4").reshape(na).tobytes())
    done = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    with open(dst, "rb") as f:
        buf = f.read()
    os.remove(src)
    os.remove(dst)
    assert len(buf) == na * (12 + (24 if wide else 0)), (len(buf), na, wide)
    out = [np.frombuffer(buf, "<i4", na, 0), np.frombuffer(buf, "<f4", na, 4 * na), np.frombuffer(buf, "<f4", na, 8 * na)]
    if wide:
        out += [np.frombuffer(buf, "<f8", na, 12 * na + 8 * na * k) for k in range(3)]
    return Scan(*out)
