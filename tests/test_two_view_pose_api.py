"""CPU tests of the two-view pose calls (include/lf_mkd.h: lf_mkd_two_view_pose_device, lf_mkd_two_view_pose): the symbols
exist with the header's arities, and every refusal is made with its message before any device is touched (a null handle is the
LAST thing looked at: a call whose only fault is the missing handle says so)."""
import ctypes
import os
import re

from conftest import ROOT

import local_features_python as lfp

BIG = (1 << 31) - 1
NAN = float("nan")


def test_the_symbols_are_exported():
    L = lfp.load_library()
    header = open(os.path.join(ROOT, "include", "lf_mkd.h")).read()
    for name, arity in (("lf_mkd_two_view_pose_device", 21), ("lf_mkd_two_view_pose", 16)):
        assert name in lfp.SYMBOLS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == arity
        proto = re.search(r"int %s\((.*?)\);" % name, header, flags=re.S).group(1)
        assert len(proto.split(",")) == arity
    assert hasattr(lfp.LocalFeatures, "two_view_pose")
    assert hasattr(lfp.MkdHandle, "two_view_pose_device") and hasattr(lfp.MkdHandle, "two_view_pose")


def _refused(L, rc, who, what, kw):
    assert rc == -1, (who, kw)
    msg = L.lf_mkd_last_error(None)
    assert msg.startswith(who + b": ") and what in msg, (who, kw, msg)


def test_the_device_call_refuses_bad_arguments_without_a_device():
    L = lfp.load_library()
    p, odd4, odd8 = ctypes.c_void_p(64), ctypes.c_void_p(66), ctypes.c_void_p(68)

    def call(kps=p, rows=100, ea=p, eb=p, n_edges=3, intr=p, n_images=4, F=p, off=p, la=p, lb=p, cap=50, deg=1.0, flags=0,
             R=p, t=p, stats=p, sigma=p, points=p):
        return L.lf_mkd_two_view_pose_device(None, kps, rows, ea, eb, n_edges, intr, n_images, F, off, la, lb, cap, deg, flags,
                                             R, t, stats, sigma, points, None)

    cases = [({}, b"null handle"), ({"sigma": None, "points": None}, b"null handle"), ({"deg": 0.0}, b"null handle"),
             ({"deg": 180.0}, b"null handle"), ({"cap": 0, "la": None, "lb": None, "kps": None}, b"null handle"),
             ({"rows": BIG, "cap": BIG, "n_edges": BIG}, b"null handle"), ({"n_images": 0, "intr": None}, b"null handle"),
             ({"ea": None}, b"null edge array"), ({"eb": None}, b"null edge array"),
             ({"F": None}, b"null d_F"), ({"off": None}, b"null d_F"), ({"R": None}, b"null d_F"), ({"t": None}, b"null d_F"),
             ({"stats": None}, b"null d_F"), ({"intr": None}, b"null d_intrinsics"),
             ({"la": None}, b"null d_link_a"), ({"lb": None}, b"null d_link_a"), ({"kps": None}, b"null d_kps"),
             ({"flags": 1}, b"unknown flag bits"), ({"flags": 0x80000000}, b"unknown flag bits"),
             ({"deg": -0.001}, b"min_parallax_deg"), ({"deg": 180.001}, b"min_parallax_deg"), ({"deg": NAN}, b"min_parallax_deg"),
             ({"deg": float("inf")}, b"min_parallax_deg"),
             ({"off": odd8}, b"8-byte aligned"), ({"off": odd4}, b"8-byte aligned")]
    cases += [({k: odd4}, b"4-byte aligned") for k in ("kps", "ea", "eb", "intr", "F", "la", "lb", "R", "t", "stats", "sigma", "points")]
    cases += [({"rows": BIG + 1}, b"2^31 - 1"), ({"cap": BIG + 1}, b"2^31 - 1"), ({"cap": 1 << 40}, b"2^31 - 1"),
              ({"n_edges": BIG + 1}, b"2^31 - 1")]
    for kw, what in cases:
        if what == b"null handle":
            assert call(**kw) == -1 and L.lf_mkd_last_error(None) == b"two_view_pose_device: null handle", kw
        else:
            _refused(L, call(**kw), b"two_view_pose_device", what, kw)
    # n_edges == 0 needs nothing but a handle
    assert call(n_edges=0, ea=None, eb=None, F=None, off=None, R=None, t=None, stats=None) == -1
    assert L.lf_mkd_last_error(None) == b"two_view_pose_device: null handle"


def test_the_host_call_refuses_bad_arguments_without_a_device():
    L = lfp.load_library()
    p = ctypes.c_void_p(64)

    def call(F=p, Ka=p, Kb=p, ka=p, na=10, kb=p, nb=10, match=p, deg=1.0, flags=0, R=p, t=p, stats=p, sigma=p, points=p):
        return L.lf_mkd_two_view_pose(None, F, Ka, Kb, ka, na, kb, nb, match, deg, flags, R, t, stats, sigma, points)

    cases = [({}, b"null handle"), ({"sigma": None, "points": None}, b"null handle"),
             ({"na": 0, "ka": None, "match": None}, b"null handle"), ({"nb": 0, "kb": None}, b"null handle"),
             ({"na": BIG - 10}, b"null handle")]
    cases += [({k: None}, b"null pointer") for k in ("F", "Ka", "Kb", "R", "t", "stats")]
    cases += [({k: None}, b"null keypoint or match array") for k in ("ka", "kb", "match")]
    cases += [({"flags": 2}, b"unknown flag bits"), ({"deg": -1.0}, b"min_parallax_deg"), ({"deg": 181.0}, b"min_parallax_deg"),
              ({"deg": NAN}, b"min_parallax_deg"), ({"na": BIG + 1}, b"2^31 - 1"), ({"nb": BIG + 1}, b"2^31 - 1"),
              ({"na": BIG - 5, "nb": 6}, b"2^31 - 1")]
    for kw, what in cases:
        if what == b"null handle":
            assert call(**kw) == -1 and L.lf_mkd_last_error(None) == b"two_view_pose: null handle", kw
        else:
            _refused(L, call(**kw), b"two_view_pose", what, kw)
