"""CPU tests of the track triangulation calls (include/lf_mkd.h: lf_mkd_triangulate_tracks_device,
lf_mkd_triangulate_tracks): the symbols exist with the header's arities, and every refusal is made with its message before
any device is touched (a null handle is the LAST thing looked at: a call whose only fault is the missing handle says so)."""
import ctypes
import os
import re

from conftest import ROOT

import local_features_python as lfp

BIG = (1 << 31) - 1
NAN, INF = float("nan"), float("inf")


def test_the_symbols_are_exported():
    L = lfp.load_library()
    header = open(os.path.join(ROOT, "include", "lf_mkd.h")).read()
    for name, arity in (("lf_mkd_triangulate_tracks_device", 20), ("lf_mkd_triangulate_tracks", 18)):
        assert name in lfp.SYMBOLS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == arity
        proto = re.search(r"int %s\((.*?)\);" % name, header, flags=re.S).group(1)
        assert len(proto.split(",")) == arity
    assert hasattr(lfp.LocalFeatures, "triangulate_tracks")
    assert hasattr(lfp.MkdHandle, "triangulate_tracks_device") and hasattr(lfp.MkdHandle, "triangulate_tracks")


def _refused(L, rc, who, what, kw):
    assert rc == -1, (who, kw)
    msg = L.lf_mkd_last_error(None)
    assert msg.startswith(who + b": ") and what in msg, (who, kw, msg)


def test_the_device_call_refuses_bad_arguments_without_a_device():
    L = lfp.load_library()
    p, odd4, odd8 = ctypes.c_void_p(64), ctypes.c_void_p(66), ctypes.c_void_p(68)

    def call(kps=p, rows=100, off=p, tcap=10, row=p, img=p, ocap=50, counts=p, intr=p, poses=p, n_images=4, px=4.0, rounds=2,
             flags=0, points=p, stats=p, err=p, state=p):
        return L.lf_mkd_triangulate_tracks_device(None, kps, rows, off, tcap, row, img, ocap, counts, intr, poses, n_images, px,
                                                  rounds, flags, points, stats, err, state, None)

    cases = [({}, b"null handle"), ({"err": None, "state": None}, b"null handle"), ({"rounds": 0}, b"null handle"),
             ({"rounds": 4}, b"null handle"), ({"px": 1e-30}, b"null handle"), ({"px": 3e38}, b"null handle"),
             ({"ocap": 0, "row": None, "img": None, "kps": None, "intr": None, "poses": None}, b"null handle"),
             ({"rows": 0, "kps": None}, b"null handle"), ({"n_images": 0, "intr": None, "poses": None}, b"null handle"),
             ({"rows": BIG, "tcap": BIG, "ocap": BIG}, b"null handle"),
             ({"off": None}, b"null d_track_offsets"), ({"counts": None}, b"null d_track_offsets"),
             ({"points": None}, b"null d_track_offsets"), ({"stats": None}, b"null d_track_offsets"),
             ({"row": None}, b"null d_obs_row"), ({"img": None}, b"null d_obs_row"), ({"kps": None}, b"null d_kps"),
             ({"intr": None}, b"null d_intrinsics"), ({"poses": None}, b"null d_intrinsics"),
             ({"flags": 1}, b"unknown flag bits"), ({"flags": 0x80000000}, b"unknown flag bits"),
             ({"px": 0.0}, b"max_reproj_px"), ({"px": -1.0}, b"max_reproj_px"), ({"px": NAN}, b"max_reproj_px"),
             ({"px": INF}, b"max_reproj_px"), ({"px": -INF}, b"max_reproj_px"),
             ({"rounds": 5}, b"rounds"), ({"rounds": 0xFFFFFFFF}, b"rounds"),
             ({"off": odd8}, b"8-byte aligned"), ({"off": odd4}, b"8-byte aligned")]
    cases += [({k: odd4}, b"4-byte aligned") for k in ("kps", "row", "img", "counts", "intr", "poses", "points", "stats", "err", "state")]
    cases += [({"rows": BIG + 1}, b"2^31 - 1"), ({"tcap": BIG + 1}, b"2^31 - 1"), ({"ocap": BIG + 1}, b"2^31 - 1"),
              ({"ocap": 1 << 40}, b"2^31 - 1")]
    for kw, what in cases:
        if what == b"null handle":
            assert call(**kw) == -1 and L.lf_mkd_last_error(None) == b"triangulate_tracks_device: null handle", kw
        else:
            _refused(L, call(**kw), b"triangulate_tracks_device", what, kw)
    # track_capacity == 0 needs nothing but a handle
    assert call(tcap=0, off=None, counts=None, points=None, stats=None, row=None, img=None) == -1
    assert L.lf_mkd_last_error(None) == b"triangulate_tracks_device: null handle"


def test_the_host_call_refuses_bad_arguments_without_a_device():
    L = lfp.load_library()
    p = ctypes.c_void_p(64)

    def call(kps=p, rows=100, off=p, n=10, row=p, img=p, n_obs=50, intr=p, poses=p, n_images=4, px=4.0, rounds=2, flags=0,
             points=p, stats=p, err=p, state=p):
        return L.lf_mkd_triangulate_tracks(None, kps, rows, off, n, row, img, n_obs, intr, poses, n_images, px, rounds, flags,
                                           points, stats, err, state)

    cases = [({}, b"null handle"), ({"err": None, "state": None}, b"null handle"),
             ({"n": 0, "off": None, "points": None, "stats": None}, b"null handle"),
             ({"n_obs": 0, "row": None, "img": None, "kps": None, "intr": None, "poses": None}, b"null handle"),
             ({"rows": BIG, "n": BIG, "n_obs": BIG}, b"null handle")]
    cases += [({k: None}, b"null track_offsets") for k in ("off", "points", "stats")]
    cases += [({k: None}, b"null obs_row") for k in ("row", "img")]
    cases += [({"kps": None}, b"null kps"), ({"intr": None}, b"null intrinsics"), ({"poses": None}, b"null intrinsics"),
              ({"flags": 2}, b"unknown flag bits"), ({"px": 0.0}, b"max_reproj_px"), ({"px": NAN}, b"max_reproj_px"),
              ({"px": INF}, b"max_reproj_px"), ({"rounds": 5}, b"rounds"), ({"rows": BIG + 1}, b"2^31 - 1"),
              ({"n": BIG + 1}, b"2^31 - 1"), ({"n_obs": BIG + 1}, b"2^31 - 1")]
    for kw, what in cases:
        if what == b"null handle":
            assert call(**kw) == -1 and L.lf_mkd_last_error(None) == b"triangulate_tracks: null handle", kw
        else:
            _refused(L, call(**kw), b"triangulate_tracks", what, kw)
