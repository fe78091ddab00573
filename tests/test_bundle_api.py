"""CPU tests of the bundle adjustment calls (include/lf_mkd.h: lf_mkd_bundle_adjust_device, lf_mkd_bundle_adjust): the symbols
exist with the header's arities, and every refusal is made with its message before any device is touched (a null handle is the
LAST thing looked at: a call whose only fault is the missing handle says so)."""
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
    for name, arity in (("lf_mkd_bundle_adjust_device", 28), ("lf_mkd_bundle_adjust", 26)):
        assert name in lfp.SYMBOLS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == arity
        proto = re.search(r"int %s\((.*?)\);" % name, header, flags=re.S).group(1)
        assert len(proto.split(",")) == arity
    assert hasattr(lfp.LocalFeatures, "bundle_adjust")
    assert hasattr(lfp.MkdHandle, "bundle_adjust_device") and hasattr(lfp.MkdHandle, "bundle_adjust")


def _refused(L, rc, who, what, kw):
    assert rc == -1, (who, kw)
    msg = L.lf_mkd_last_error(None)
    assert msg.startswith(who + b": ") and what in msg, (who, kw, msg)


def test_the_device_call_refuses_bad_arguments_without_a_device():
    L = lfp.load_library()
    p, odd4, odd8 = ctypes.c_void_p(64), ctypes.c_void_p(66), ctypes.c_void_p(68)

    def call(kps=p, ioff=p, n_images=4, rows=100, toff=p, tcap=10, row=p, img=p, ocap=30, counts=p, points=p, intr=p, poses=p,
             state=p, fixed=p, px=4.0, lam=1e-3, iters=10, cg=10, tol=0.1, flags=0, out=p, pout=p, sout=p, trace=p, cnt=p):
        return L.lf_mkd_bundle_adjust_device(None, kps, ioff, n_images, rows, toff, tcap, row, img, ocap, counts, points, intr, poses,
                                             state, fixed, px, lam, iters, cg, tol, flags, out, pout, sout, trace, cnt, None)

    cases = [({}, b"null handle"), ({"state": None, "fixed": None, "sout": None}, b"null handle"), ({"iters": 1}, b"null handle"),
             ({"iters": 64}, b"null handle"), ({"cg": 1}, b"null handle"), ({"cg": 256}, b"null handle"), ({"tol": 0.0}, b"null handle"),
             ({"tol": 0.999}, b"null handle"), ({"px": 3e38, "lam": 3e38}, b"null handle"), ({"lam": 1e-38}, b"null handle"),
             ({"rows": 0, "kps": None}, b"null handle"), ({"ocap": 0, "row": None, "img": None, "kps": None}, b"null handle"),
             ({"tcap": 0, "toff": None, "points": None, "pout": None, "row": None, "img": None, "kps": None}, b"null handle"),
             ({"out": p, "poses": p, "pout": p, "points": p}, b"null handle"),
             ({"rows": BIG, "tcap": BIG, "ocap": BIG, "n_images": BIG}, b"null handle")]
    cases += [({k: None}, b"null d_image_offsets") for k in ("ioff", "counts", "intr", "poses", "out", "trace", "cnt")]
    cases += [({k: None}, b"null d_track_offsets") for k in ("toff", "points", "pout")]
    cases += [({"row": None}, b"null d_obs_row"), ({"img": None}, b"null d_obs_row"), ({"kps": None}, b"null d_kps"),
              ({"kps": None, "ioff": None}, b"null d_image_offsets"), ({"row": None, "toff": None}, b"null d_track_offsets"),
              ({"flags": 1}, b"unknown flag bits"), ({"flags": 0x80000000}, b"unknown flag bits"), ({"flags": 1, "kps": None}, b"null d_kps"),
              ({"px": 0.0}, b"max_reproj_px"), ({"px": -1.0}, b"max_reproj_px"), ({"px": NAN}, b"max_reproj_px"),
              ({"px": INF}, b"max_reproj_px"), ({"px": 0.0, "flags": 1}, b"unknown flag bits"),
              ({"lam": 0.0}, b"lambda0"), ({"lam": -1e-3}, b"lambda0"), ({"lam": NAN}, b"lambda0"), ({"lam": INF}, b"lambda0"),
              ({"lam": 0.0, "px": 0.0}, b"max_reproj_px"),
              ({"iters": 0}, b": iterations must be"), ({"iters": 65}, b": iterations must be"), ({"iters": 0xFFFFFFFF}, b": iterations must be"),
              ({"iters": 0, "lam": 0.0}, b"lambda0"),
              ({"cg": 0}, b"cg_iterations"), ({"cg": 257}, b"cg_iterations"), ({"cg": 0xFFFFFFFF}, b"cg_iterations"),
              ({"cg": 0, "iters": 0}, b": iterations must be"),
              ({"tol": 1.0}, b"cg_tol"), ({"tol": -0.1}, b"cg_tol"), ({"tol": NAN}, b"cg_tol"), ({"tol": INF}, b"cg_tol"),
              ({"tol": 1.0, "cg": 0}, b"cg_iterations")]
    cases += [({k: v}, b"8-byte aligned") for k in ("ioff", "toff", "trace") for v in (odd4, odd8)]
    cases += [({"ioff": odd8, "tol": 1.0}, b"cg_tol")]
    cases += [({k: odd4}, b"4-byte aligned") for k in ("kps", "row", "img", "counts", "points", "intr", "poses", "state", "fixed", "out",
                                                       "pout", "sout", "cnt")]
    cases += [({"kps": odd4, "ioff": odd8}, b"8-byte aligned")]
    cases += [({k: BIG + 1}, b"2^31 - 1") for k in ("rows", "tcap", "ocap", "n_images")] + [({"rows": 1 << 40}, b"2^31 - 1"),
                                                                                           ({"rows": BIG + 1, "kps": odd4}, b"4-byte aligned")]
    for kw, what in cases:
        _refused(L, call(**kw), b"bundle_adjust_device", what, kw)


def test_no_images_is_ok_and_touches_nothing():
    L = lfp.load_library()

    def call(iters=10):
        return L.lf_mkd_bundle_adjust_device(None, None, None, 0, 0, None, 0, None, None, 0, None, None, None, None, None, None, 4.0, 1e-3,
                                             iters, 10, 0.1, 0, None, None, None, None, None, None)

    _refused(L, call(), b"bundle_adjust_device", b"null handle", {})           # every pointer null: the only fault is the handle
    _refused(L, call(iters=0), b"bundle_adjust_device", b": iterations must be", {})   # ... and the scalars are still checked


def test_the_host_form_refuses_bad_arguments_without_a_device():
    L = lfp.load_library()
    p = ctypes.c_void_p(64)

    def call(kps=p, ioff=p, n_images=4, rows=100, toff=p, n_tracks=10, row=p, img=p, n_obs=30, points=p, intr=p, poses=p, state=p,
             fixed=p, px=4.0, lam=1e-3, iters=10, cg=10, tol=0.1, flags=0, out=p, pout=p, sout=p, trace=p, cnt=p):
        return L.lf_mkd_bundle_adjust(None, kps, ioff, n_images, rows, toff, n_tracks, row, img, n_obs, points, intr, poses, state,
                                      fixed, px, lam, iters, cg, tol, flags, out, pout, sout, trace, cnt)

    cases = [({}, b"null handle"), ({"state": None, "fixed": None, "sout": None}, b"null handle"),
             ({"n_images": 0, "ioff": None, "intr": None, "poses": None, "out": None, "trace": None, "cnt": None}, b"null handle"),
             ({"n_tracks": 0, "toff": None, "points": None, "pout": None}, b"null handle")]
    cases += [({k: None}, b"null image_offsets") for k in ("ioff", "intr", "poses", "out", "trace", "cnt")]
    cases += [({k: None}, b"null track_offsets") for k in ("toff", "points", "pout")]
    cases += [({"row": None}, b"null obs_row"), ({"img": None}, b"null obs_row"), ({"kps": None}, b"null kps"),
              ({"flags": 2}, b"unknown flag bits"), ({"px": 0.0}, b"max_reproj_px"), ({"px": NAN}, b"max_reproj_px"),
              ({"lam": 0.0}, b"lambda0"), ({"lam": INF}, b"lambda0"), ({"iters": 0}, b": iterations must be"), ({"iters": 65}, b": iterations must be"),
              ({"cg": 0}, b"cg_iterations"), ({"cg": 257}, b"cg_iterations"), ({"tol": 1.0}, b"cg_tol"), ({"tol": NAN}, b"cg_tol"),
              ({"rows": BIG + 1}, b"2^31 - 1"), ({"n_tracks": BIG + 1}, b"2^31 - 1"), ({"n_obs": BIG + 1}, b"2^31 - 1"),
              ({"n_images": BIG + 1}, b"2^31 - 1"), ({"rows": BIG + 1, "tol": 1.0}, b"cg_tol")]
    for kw, what in cases:
        _refused(L, call(**kw), b"bundle_adjust", what, kw)
