"""CPU tests of the camera resection calls (include/lf_mkd.h: lf_mkd_resect_cameras_device, lf_mkd_resect_camera): the
symbols exist with the header's arities, and every refusal is made with its message before any device is touched (a null
handle is the LAST thing looked at: a call whose only fault is the missing handle says so)."""
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
    for name, arity in (("lf_mkd_resect_cameras_device", 23), ("lf_mkd_resect_camera", 18)):
        assert name in lfp.SYMBOLS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == arity
        proto = re.search(r"int %s\((.*?)\);" % name, header, flags=re.S).group(1)
        assert len(proto.split(",")) == arity
    assert hasattr(lfp.LocalFeatures, "resect_cameras") and lfp.RESECT_ALL == 1
    assert re.search(r"#define LF_MKD_RESECT_ALL \(1u\)", header)
    assert hasattr(lfp.MkdHandle, "resect_cameras_device") and hasattr(lfp.MkdHandle, "resect_camera")


def _refused(L, rc, who, what, kw):
    assert rc == -1, (who, kw)
    msg = L.lf_mkd_last_error(None)
    assert msg.startswith(who + b": ") and what in msg, (who, kw, msg)


def test_the_device_call_refuses_bad_arguments_without_a_device():
    L = lfp.load_library()
    p, odd4, odd8 = ctypes.c_void_p(64), ctypes.c_void_p(66), ctypes.c_void_p(68)

    def call(kps=p, off=p, n_images=4, rows=100, rt=p, points=p, tcap=10, counts=p, intr=p, poses=p, px=4.0, deg=0.0, n_samples=64,
             min_inliers=12, rounds=3, seed=0, flags=0, out=p, stats=p, err=p, state=p):
        return L.lf_mkd_resect_cameras_device(None, kps, off, n_images, rows, rt, points, tcap, counts, intr, poses, px, deg,
                                              n_samples, min_inliers, rounds, seed, flags, out, stats, err, state, None)

    cases = [({}, b"null handle"), ({"err": None, "state": None}, b"null handle"), ({"rounds": 0}, b"null handle"),
             ({"rounds": 4}, b"null handle"), ({"px": 1e-30}, b"null handle"), ({"px": 3e38}, b"null handle"),
             ({"deg": 180.0}, b"null handle"), ({"n_samples": 1}, b"null handle"), ({"n_samples": 4096}, b"null handle"),
             ({"flags": 1}, b"null handle"), ({"min_inliers": 0xFFFFFFFF, "seed": 0xFFFFFFFF}, b"null handle"),
             ({"rows": 0, "kps": None, "rt": None, "points": None}, b"null handle"), ({"tcap": 0, "points": None}, b"null handle"),
             ({"out": p, "poses": p}, b"null handle"), ({"rows": BIG, "tcap": BIG, "n_images": BIG}, b"null handle")]
    cases += [({k: None}, b"null d_image_offsets") for k in ("off", "counts", "intr", "poses", "out", "stats")]
    cases += [({"kps": None}, b"null d_kps"), ({"rt": None}, b"null d_kps"), ({"points": None}, b"null d_points"),
              ({"flags": 2}, b"unknown flag bits"), ({"flags": 0x80000001}, b"unknown flag bits"),
              ({"px": 0.0}, b"max_reproj_px"), ({"px": -1.0}, b"max_reproj_px"), ({"px": NAN}, b"max_reproj_px"),
              ({"px": INF}, b"max_reproj_px"), ({"px": -INF}, b"max_reproj_px"),
              ({"deg": -0.5}, b"min_parallax_deg"), ({"deg": 180.5}, b"min_parallax_deg"), ({"deg": NAN}, b"min_parallax_deg"),
              ({"deg": INF}, b"min_parallax_deg"),
              ({"n_samples": 0}, b"n_samples"), ({"n_samples": 4097}, b"n_samples"), ({"n_samples": 0xFFFFFFFF}, b"n_samples"),
              ({"rounds": 5}, b"rounds"), ({"rounds": 0xFFFFFFFF}, b"rounds"),
              ({"off": odd8}, b"8-byte aligned"), ({"off": odd4}, b"8-byte aligned")]
    cases += [({k: odd4}, b"4-byte aligned") for k in ("kps", "rt", "points", "counts", "intr", "poses", "out", "stats", "err", "state")]
    cases += [({"rows": BIG + 1}, b"2^31 - 1"), ({"tcap": BIG + 1}, b"2^31 - 1"), ({"n_images": BIG + 1}, b"2^31 - 1"),
              ({"rows": 1 << 40}, b"2^31 - 1")]
    for kw, what in cases:
        _refused(L, call(**kw), b"resect_cameras_device", what, kw)


def test_no_images_is_ok_and_touches_nothing():
    L = lfp.load_library()
    # every pointer null, no handle needed to say so: the only fault is the missing handle ...
    rc = L.lf_mkd_resect_cameras_device(None, None, None, 0, 0, None, None, 0, None, None, None, 4.0, 0.0, 64, 12, 3, 0, 0, None,
                                        None, None, None, None)
    _refused(L, rc, b"resect_cameras_device", b"null handle", {})
    # ... and the scalars are still checked
    rc = L.lf_mkd_resect_cameras_device(None, None, None, 0, 0, None, None, 0, None, None, None, 4.0, 0.0, 0, 12, 3, 0, 0, None,
                                        None, None, None, None)
    _refused(L, rc, b"resect_cameras_device", b"n_samples", {})


def test_the_host_form_refuses_bad_arguments_without_a_device():
    L = lfp.load_library()
    p = ctypes.c_void_p(64)

    def call(kps=p, rows=100, rt=p, points=p, n_tracks=10, intr=p, px=4.0, deg=0.0, n_samples=64, min_inliers=12, rounds=3, seed=0,
             flags=0, pose=p, stats=p, err=p, state=p):
        return L.lf_mkd_resect_camera(None, kps, rows, rt, points, n_tracks, intr, px, deg, n_samples, min_inliers, rounds, seed,
                                      flags, pose, stats, err, state)

    cases = [({}, b"null handle"), ({"err": None, "state": None}, b"null handle"),
             ({"rows": 0, "kps": None, "rt": None, "points": None}, b"null handle"),
             ({"intr": None}, b"null intrinsics"), ({"pose": None}, b"null intrinsics"), ({"stats": None}, b"null intrinsics"),
             ({"kps": None}, b"null kps"), ({"rt": None}, b"null kps"), ({"points": None}, b"null points"),
             ({"flags": 4}, b"unknown flag bits"), ({"px": 0.0}, b"max_reproj_px"), ({"px": NAN}, b"max_reproj_px"),
             ({"deg": 181.0}, b"min_parallax_deg"), ({"n_samples": 0}, b"n_samples"), ({"n_samples": 4097}, b"n_samples"),
             ({"rounds": 5}, b"rounds"), ({"rows": BIG + 1}, b"2^31 - 1"), ({"n_tracks": BIG + 1}, b"2^31 - 1")]
    for kw, what in cases:
        _refused(L, call(**kw), b"resect_camera", what, kw)
