"""CPU tests of the tree-pose and global-positioning calls (include/lf_mkd.h: lf_mkd_tree_poses_device, lf_mkd_tree_poses,
lf_mkd_global_positions_plan, lf_mkd_global_positions_device, lf_mkd_global_positions): the symbols exist with the header's
arities, and every refusal the header lists is made with its message before any device is touched (a null handle is the LAST
thing looked at: a call whose only fault is the missing handle says so)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

import local_features_python as lfp

BIG = (1 << 31) - 1
NAN, INF = float("nan"), float("inf")


def test_the_symbols_are_exported():
    L = lfp.load_library()
    header = open(os.path.join(ROOT, "include", "lf_mkd.h")).read()
    for name, arity in (("lf_mkd_tree_poses_device", 11), ("lf_mkd_tree_poses", 10), ("lf_mkd_global_positions_plan", 5),
                        ("lf_mkd_global_positions_device", 26), ("lf_mkd_global_positions", 24)):
        assert name in lfp.SYMBOLS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == arity
        proto = re.search(r"int %s\((.*?)\);" % name, header, flags=re.S).group(1)
        assert len(proto.split(",")) == arity
    assert hasattr(lfp.LocalFeatures, "tree_poses") and hasattr(lfp.LocalFeatures, "global_positions")
    assert hasattr(lfp.MkdHandle, "global_positions_device") and hasattr(lfp.MkdHandle, "global_positions")
    assert hasattr(lfp.MkdHandle, "tree_poses_device") and hasattr(lfp.MkdHandle, "tree_poses")
    assert lfp.GLOBAL_POSITIONS_MAX_SWEEPS == int(re.search(r"LF_MKD_GLOBAL_POSITIONS_MAX_SWEEPS \((\d+)u\)", header).group(1))


def _refused(L, rc, who, what, kw):
    assert rc == -1, (who, kw)
    msg = L.lf_mkd_last_error(None)
    assert msg.startswith(who + b": ") and what in msg, (who, kw, msg)


def test_global_positions_device_refuses_bad_arguments_without_a_device():
    L = lfp.load_library()
    p, odd4, odd8 = ctypes.c_void_p(64), ctypes.c_void_p(66), ctypes.c_void_p(68)

    def call(kps=p, ioff=p, n_images=4, rows=100, toff=p, tcap=10, row=p, img=p, ocap=30, counts=p, rt=p, intr=p, poses=p, sweeps=50,
             warm=3, deg=0.2, min_obs=2, flags=0, out=p, pout=p, sout=p, ims=p, trace=p, cnt=p):
        return L.lf_mkd_global_positions_device(None, kps, ioff, n_images, rows, toff, tcap, row, img, ocap, counts, rt, intr, poses,
                                                sweeps, warm, deg, min_obs, flags, out, pout, sout, ims, trace, cnt, None)

    cases = [({}, b"null handle"), ({"pout": None, "sout": None, "trace": None}, b"null handle"), ({"sweeps": 0}, b"null handle"),
             ({"sweeps": 4096, "warm": 0xFFFFFFFF}, b"null handle"), ({"deg": 90.0}, b"null handle"), ({"min_obs": 0xFFFFFFFF}, b"null handle"),
             ({"rows": 0, "kps": None, "rt": None}, b"null handle"), ({"ocap": 0, "row": None, "img": None}, b"null handle"),
             ({"tcap": 0, "toff": None, "row": None, "img": None}, b"null handle"), ({"out": p, "poses": p}, b"null handle"),
             ({"rows": BIG, "tcap": BIG, "ocap": BIG, "n_images": BIG}, b"null handle")]
    cases += [({k: None}, b"null d_image_offsets") for k in ("ioff", "counts", "intr", "poses", "out", "ims", "cnt")]
    cases += [({"toff": None}, b"null d_track_offsets"), ({"row": None}, b"null d_obs_row"), ({"img": None}, b"null d_obs_row"),
              ({"kps": None}, b"null d_kps"), ({"rt": None}, b"null d_kps"), ({"kps": None, "ioff": None}, b"null d_image_offsets"),
              ({"row": None, "toff": None}, b"null d_track_offsets"),
              ({"flags": 1}, b"unknown flag bits"), ({"flags": 0x80000000}, b"unknown flag bits"), ({"flags": 1, "kps": None}, b"null d_kps"),
              ({"sweeps": 4097}, b"sweeps must be"), ({"sweeps": 0xFFFFFFFF}, b"sweeps must be"), ({"sweeps": 4097, "flags": 1}, b"unknown flag bits"),
              ({"deg": 0.0}, b"robust_deg"), ({"deg": -1.0}, b"robust_deg"), ({"deg": 90.5}, b"robust_deg"), ({"deg": NAN}, b"robust_deg"),
              ({"deg": INF}, b"robust_deg"), ({"deg": 0.0, "sweeps": 4097}, b"sweeps must be"),
              ({"min_obs": 0}, b"min_obs"), ({"min_obs": 1}, b"min_obs"), ({"min_obs": 1, "deg": 0.0}, b"robust_deg")]
    cases += [({k: v}, b"8-byte aligned") for k in ("ioff", "toff", "trace") for v in (odd4, odd8)]
    cases += [({"ioff": odd8, "min_obs": 1}, b"min_obs")]
    cases += [({k: odd4}, b"4-byte aligned") for k in ("kps", "row", "img", "counts", "rt", "intr", "poses", "out", "pout", "sout", "ims", "cnt")]
    cases += [({"kps": odd4, "ioff": odd8}, b"8-byte aligned")]
    cases += [({k: BIG + 1}, b"2^31 - 1") for k in ("rows", "tcap", "ocap", "n_images")] + [({"rows": 1 << 40}, b"2^31 - 1"),
                                                                                           ({"rows": BIG + 1, "kps": odd4}, b"4-byte aligned")]
    for kw, what in cases:
        _refused(L, call(**kw), b"global_positions_device", what, kw)


def test_no_images_is_ok_and_touches_nothing():
    L = lfp.load_library()

    def call(sweeps=10):
        return L.lf_mkd_global_positions_device(None, None, None, 0, 0, None, 0, None, None, 0, None, None, None, None, sweeps, 3, 0.2, 2, 0,
                                                None, None, None, None, None, None, None)

    _refused(L, call(), b"global_positions_device", b"null handle", {})        # every pointer null: the only fault is the handle
    _refused(L, call(sweeps=5000), b"global_positions_device", b"sweeps must be", {})   # ... and the scalars are still checked
    rc = L.lf_mkd_tree_poses_device(None, None, None, None, 0, None, None, 0, 64, None, None)
    _refused(L, rc, b"tree_poses_device", b"null handle", {})


def test_the_host_form_refuses_bad_arguments_without_a_device():
    L = lfp.load_library()
    p = ctypes.c_void_p(64)

    def call(kps=p, ioff=p, n_images=4, rows=100, toff=p, n_tracks=10, row=p, img=p, n_obs=30, rt=p, intr=p, poses=p, sweeps=50, warm=3,
             deg=0.2, min_obs=2, flags=0, out=p, pout=p, sout=p, ims=p, trace=p, cnt=p):
        return L.lf_mkd_global_positions(None, kps, ioff, n_images, rows, toff, n_tracks, row, img, n_obs, rt, intr, poses, sweeps, warm,
                                         deg, min_obs, flags, out, pout, sout, ims, trace, cnt)

    cases = [({}, b"null handle"), ({"pout": None, "sout": None, "trace": None}, b"null handle"),
             ({"n_images": 0, "ioff": None, "intr": None, "poses": None, "out": None, "ims": None, "cnt": None, "kps": None, "rt": None},
              b"null handle"), ({"n_tracks": 0, "toff": None}, b"null handle")]
    cases += [({k: None}, b"null image_offsets") for k in ("ioff", "intr", "poses", "out", "ims", "cnt")]
    cases += [({"toff": None}, b"null track_offsets"), ({"row": None}, b"null obs_row"), ({"img": None}, b"null obs_row"),
              ({"kps": None}, b"null kps"), ({"rt": None}, b"null kps"), ({"flags": 2}, b"unknown flag bits"),
              ({"sweeps": 4097}, b"sweeps must be"), ({"deg": 0.0}, b"robust_deg"), ({"deg": NAN}, b"robust_deg"), ({"min_obs": 1}, b"min_obs"),
              ({"rows": BIG + 1}, b"2^31 - 1"), ({"n_tracks": BIG + 1}, b"2^31 - 1"), ({"n_obs": BIG + 1}, b"2^31 - 1"),
              ({"n_images": BIG + 1}, b"2^31 - 1"), ({"rows": BIG + 1, "min_obs": 1}, b"min_obs")]
    for kw, what in cases:
        _refused(L, call(**kw), b"global_positions", what, kw)


def test_tree_poses_refuse_bad_arguments_without_a_device():
    L = lfp.load_library()
    p, odd4 = ctypes.c_void_p(64), ctypes.c_void_p(66)

    def device(ea=p, eb=p, t=p, n_edges=5, rot=p, st=p, n_images=4, depth=64, poses=p):
        return L.lf_mkd_tree_poses_device(None, ea, eb, t, n_edges, rot, st, n_images, depth, poses, None)

    def host(ea=p, eb=p, t=p, n_edges=5, rot=p, st=p, n_images=4, depth=64, poses=p):
        return L.lf_mkd_tree_poses(None, ea, eb, t, n_edges, rot, st, n_images, depth, poses)

    cases = [({}, b"null handle"), ({"depth": 0}, b"null handle"), ({"depth": 4096}, b"null handle"),
             ({"n_edges": 0, "ea": None, "eb": None, "t": None}, b"null handle"),
             ({"n_images": 0, "rot": None, "st": None, "poses": None, "ea": None}, b"null handle"),
             ({"depth": 4097}, b"max_depth"), ({"depth": 0xFFFFFFFF}, b"max_depth"),
             ({"n_images": BIG + 1}, b"2^31 - 1"), ({"n_edges": BIG + 1}, b"2^31 - 1")]
    for d, prefix in ((True, b"d_"), (False, b"")):
        who = b"tree_poses_device" if d else b"tree_poses"
        for kw, what in cases + [({k: None}, b"null " + prefix + b"rotations") for k in ("rot", "st", "poses")] + [
                ({k: None}, b"null " + prefix + b"edge_a") for k in ("ea", "eb", "t")] + [({"rot": None, "depth": 4097}, b"rotations")]:
            _refused(L, (device if d else host)(**kw), who, what, kw)
    for k in ("ea", "eb", "t", "rot", "st", "poses"):
        _refused(L, device(**{k: odd4}), b"tree_poses_device", b"4-byte aligned", k)
    _refused(L, device(ea=odd4, depth=4097), b"tree_poses_device", b"max_depth", {})


def test_the_plan_refuses_and_counts():
    L = lfp.load_library()
    assert lfp.global_positions_plan(8, 1000, 50)[0] == 154 and lfp.global_positions_plan(8, 1000, 0)[0] == 4
    assert lfp.global_positions_plan(0, 1000, 50) == (0, 0)
    for args, what in (((8, 1000, 4097), b"sweeps must be"), ((BIG + 1, 10, 5), b"2^31 - 1"), ((8, BIG + 1, 5), b"2^31 - 1")):
        _refused(L, L.lf_mkd_global_positions_plan(*args, None, None), b"global_positions_plan", what, args)
    with pytest.raises(RuntimeError, match="sweeps must be"):
        lfp.global_positions_plan(8, 1000, 5000)
