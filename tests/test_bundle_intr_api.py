"""CPU tests of the self-calibrating bundle adjustment calls (include/lf_mkd.h: lf_mkd_bundle_adjust_intrinsics_device,
lf_mkd_bundle_adjust_intrinsics): the symbols exist with the header's arities, and every refusal is made with its message
before any device is touched, in the header's order (a null handle is the LAST thing looked at)."""
import ctypes
import os
import re

from conftest import ROOT

import local_features_python as lfp

BIG = (1 << 31) - 1
NAN, INF = float("nan"), float("inf")
DEV, HOST = b"bundle_adjust_intrinsics_device", b"bundle_adjust_intrinsics"


def test_the_symbols_are_exported():
    L = lfp.load_library()
    header = open(os.path.join(ROOT, "include", "lf_mkd.h")).read()
    for name, arity in (("lf_mkd_bundle_adjust_intrinsics_device", 33), ("lf_mkd_bundle_adjust_intrinsics", 31)):
        assert name in lfp.SYMBOLS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == arity
        proto = re.search(r"int %s\((.*?)\);" % name, header, flags=re.S).group(1)
        assert len(proto.split(",")) == arity
    assert re.search(r"#define LF_MKD_BA_REFINE_FOCAL \(1u\)", header) and re.search(r"#define LF_MKD_BA_REFINE_PRINCIPAL \(2u\)", header)
    assert (lfp.BA_REFINE_FOCAL, lfp.BA_REFINE_PRINCIPAL) == (1, 2)
    assert hasattr(lfp.LocalFeatures, "bundle_adjust_intrinsics")
    assert hasattr(lfp.MkdHandle, "bundle_adjust_intrinsics_device") and hasattr(lfp.MkdHandle, "bundle_adjust_intrinsics")


def _refused(L, rc, who, what, kw):
    assert rc == -1, (who, kw)
    msg = L.lf_mkd_last_error(None)
    assert msg.startswith(who + b": ") and what in msg, (who, kw, msg)


def test_the_device_call_refuses_bad_arguments_without_a_device():
    L = lfp.load_library()
    p, odd4, odd8 = ctypes.c_void_p(64), ctypes.c_void_p(66), ctypes.c_void_p(68)

    def call(kps=p, ioff=p, n_images=4, rows=100, toff=p, tcap=10, row=p, img=p, ocap=30, counts=p, points=p, intr=p, poses=p,
             state=p, fixed=p, group=p, n_groups=2, refine=3, px=4.0, lam=1e-3, iters=10, cg=10, tol=0.1, flags=0, out=p, pout=p,
             kout=p, gout=p, sout=p, trace=p, cnt=p):
        return L.lf_mkd_bundle_adjust_intrinsics_device(None, kps, ioff, n_images, rows, toff, tcap, row, img, ocap, counts, points, intr,
                                                        poses, state, fixed, group, n_groups, refine, px, lam, iters, cg, tol, flags,
                                                        out, pout, kout, gout, sout, trace, cnt, None)

    cases = [({}, b"null handle"), ({"state": None, "fixed": None, "sout": None, "gout": None}, b"null handle"),
             ({"group": None, "n_groups": 1}, b"null handle"), ({"refine": 0}, b"null handle"), ({"refine": 1}, b"null handle"),
             ({"refine": 2}, b"null handle"), ({"n_groups": BIG}, b"null handle"), ({"kout": p, "intr": p}, b"null handle"),
             ({"iters": 64, "cg": 256, "tol": 0.0}, b"null handle"),
             ({"tcap": 0, "toff": None, "points": None, "pout": None, "row": None, "img": None, "kps": None}, b"null handle"),
             ({"rows": BIG, "tcap": BIG, "ocap": BIG, "n_images": BIG}, b"null handle")]
    # the sibling's list, in its order, with d_intrinsics_out among the required pointers
    cases += [({k: None}, b"null d_image_offsets") for k in ("ioff", "counts", "intr", "poses", "out", "kout", "trace", "cnt")]
    cases += [({"kout": None}, b"d_intrinsics_out")]
    cases += [({k: None}, b"null d_track_offsets") for k in ("toff", "points", "pout")]
    cases += [({"row": None}, b"null d_obs_row"), ({"img": None}, b"null d_obs_row"), ({"kps": None}, b"null d_kps"),
              ({"kps": None, "kout": None}, b"null d_image_offsets"),
              # the groups: after the pointers, before the scalars
              ({"refine": 4}, b"unknown refine bits"), ({"refine": 0x80000001}, b"unknown refine bits"), ({"refine": 4, "kps": None}, b"null d_kps"),
              ({"n_groups": 0}, b"n_groups must be at least 1"), ({"n_groups": 0, "refine": 4}, b"unknown refine bits"),
              ({"group": None, "n_groups": 2}, b"n_groups must be 1"), ({"group": None, "n_groups": 0}, b"n_groups must be at least 1"),
              ({"flags": 1}, b"unknown flag bits"), ({"flags": 1, "refine": 4}, b"unknown refine bits"), ({"flags": 1, "n_groups": 0}, b"n_groups"),
              ({"px": 0.0}, b"max_reproj_px"), ({"px": NAN}, b"max_reproj_px"), ({"px": INF}, b"max_reproj_px"),
              ({"lam": 0.0}, b"lambda0"), ({"lam": NAN}, b"lambda0"), ({"lam": INF}, b"lambda0"),
              ({"iters": 0}, b": iterations must be"), ({"iters": 65}, b": iterations must be"),
              ({"cg": 0}, b"cg_iterations"), ({"cg": 257}, b"cg_iterations"),
              ({"tol": 1.0}, b"cg_tol"), ({"tol": -0.1}, b"cg_tol"), ({"tol": NAN}, b"cg_tol")]
    cases += [({k: v}, b"8-byte aligned") for k in ("ioff", "toff", "trace") for v in (odd4, odd8)]
    cases += [({"ioff": odd8, "tol": 1.0}, b"cg_tol"), ({"ioff": odd8, "refine": 4}, b"unknown refine bits")]
    cases += [({k: odd4}, b"4-byte aligned") for k in ("kps", "row", "img", "counts", "points", "intr", "poses", "state", "fixed", "group",
                                                       "out", "pout", "kout", "gout", "sout", "cnt")]
    cases += [({k: BIG + 1}, b"2^31 - 1") for k in ("rows", "tcap", "ocap", "n_images", "n_groups")]
    cases += [({"n_groups": BIG + 1, "group": odd4}, b"4-byte aligned")]
    for kw, what in cases:
        _refused(L, call(**kw), DEV, what, kw)


def test_no_images_is_ok_and_touches_nothing():
    L = lfp.load_library()

    def call(iters=10, refine=1, n_groups=0):
        return L.lf_mkd_bundle_adjust_intrinsics_device(None, None, None, 0, 0, None, 0, None, None, 0, None, None, None, None, None, None,
                                                        None, n_groups, refine, 4.0, 1e-3, iters, 10, 0.1, 0, None, None, None, None, None,
                                                        None, None, None)

    _refused(L, call(), DEV, b"null handle", {})               # every pointer null, no group: the only fault is the handle
    _refused(L, call(iters=0), DEV, b": iterations must be", {})          # ... and the scalars are still checked
    _refused(L, call(refine=7), DEV, b"unknown refine bits", {})


def test_the_host_form_refuses_bad_arguments_without_a_device():
    L = lfp.load_library()
    p = ctypes.c_void_p(64)

    def call(kps=p, ioff=p, n_images=4, rows=100, toff=p, n_tracks=10, row=p, img=p, n_obs=30, points=p, intr=p, poses=p, state=p,
             fixed=p, group=p, n_groups=2, refine=1, px=4.0, lam=1e-3, iters=10, cg=10, tol=0.1, flags=0, out=p, pout=p, kout=p,
             gout=p, sout=p, trace=p, cnt=p):
        return L.lf_mkd_bundle_adjust_intrinsics(None, kps, ioff, n_images, rows, toff, n_tracks, row, img, n_obs, points, intr, poses,
                                                 state, fixed, group, n_groups, refine, px, lam, iters, cg, tol, flags, out, pout, kout,
                                                 gout, sout, trace, cnt)

    cases = [({}, b"null handle"), ({"state": None, "fixed": None, "sout": None, "gout": None, "group": None, "n_groups": 1}, b"null handle"),
             ({"n_images": 0, "ioff": None, "intr": None, "poses": None, "out": None, "kout": None, "trace": None, "cnt": None,
               "n_groups": 0}, b"null handle"),
             ({"n_tracks": 0, "toff": None, "points": None, "pout": None}, b"null handle")]
    cases += [({k: None}, b"null image_offsets") for k in ("ioff", "intr", "poses", "out", "kout", "trace", "cnt")]
    cases += [({k: None}, b"null track_offsets") for k in ("toff", "points", "pout")]
    cases += [({"row": None}, b"null obs_row"), ({"img": None}, b"null obs_row"), ({"kps": None}, b"null kps"),
              ({"refine": 4}, b"unknown refine bits"), ({"n_groups": 0}, b"n_groups must be at least 1"),
              ({"group": None}, b"n_groups must be 1"),
              ({"flags": 2}, b"unknown flag bits"), ({"px": 0.0}, b"max_reproj_px"), ({"lam": INF}, b"lambda0"),
              ({"iters": 0}, b": iterations must be"), ({"cg": 257}, b"cg_iterations"), ({"tol": NAN}, b"cg_tol"),
              ({"rows": BIG + 1}, b"2^31 - 1"), ({"n_tracks": BIG + 1}, b"2^31 - 1"), ({"n_obs": BIG + 1}, b"2^31 - 1"),
              ({"n_images": BIG + 1}, b"2^31 - 1"), ({"n_groups": BIG + 1}, b"2^31 - 1"), ({"rows": BIG + 1, "tol": 1.0}, b"cg_tol")]
    for kw, what in cases:
        _refused(L, call(**kw), HOST, what, kw)
