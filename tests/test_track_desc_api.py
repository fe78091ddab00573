"""The refusals of lf_mkd_track_descriptors_device and of its host form: every call below is made with a NULL handle and fake
pointers that are never dereferenced, so a refusal proves that nothing was touched; each LF_MKD_ERR_BAD_ARG comes back with
the call's prefix, in the order include/lf_mkd.h lists them, and the missing handle is the last fault reported."""
import pytest

import local_features_python as lfp

P, ODD2, ODD4, ODD8 = 64, 66, 68, 72   # fake addresses: aligned to 64; not to 4; to 4 but not 8; to 8 but not 16
BIG = (1 << 31) - 1
NAN, INF = float("nan"), float("inf")

DEVICE = [("q", P), ("rows", 100), ("toff", P), ("tcap", 10), ("obs_row", P), ("ocap", 30), ("counts", P), ("state", None),
          ("min_state", 2), ("points", None), ("deg", 0.0), ("scale", 256.0), ("desc", P), ("stats", None), ("stream", None)]
HOST = [("q", P), ("rows", 100), ("toff", P), ("n_tracks", 10), ("obs_row", P), ("n_obs", 30), ("state", None), ("min_state", 2),
        ("points", None), ("deg", 0.0), ("scale", 256.0), ("desc", P), ("stats", None)]

NULLS = "null d_track_offsets, d_table_counts or d_desc"
SCALE = "scale must be a positive, finite, normal f32 (0: the default, 256)"
ALIGN4 = "the observation, count, state, point and statistics arrays must be 4-byte aligned"
DEVICE_CASES = [
    ({}, "null handle"), ({"scale": 0.0}, "null handle"), ({"scale": 100.0, "min_state": 0, "deg": 180.0}, "null handle"),
    ({"state": P, "points": P, "stats": P}, "null handle"),
    ({"toff": None}, NULLS), ({"counts": None}, NULLS), ({"desc": None}, NULLS), ({"obs_row": None}, "null d_obs_row"),
    ({"obs_row": None, "ocap": 0}, "null handle"), ({"q": None}, "null d_q"), ({"q": None, "rows": 0}, "null handle"),
    ({"q": None, "ocap": 0, "obs_row": None}, "null handle"), ({"q": None, "toff": None}, NULLS),
    ({"min_state": 3}, "min_state must be 0 .. 2"), ({"min_state": 3, "q": None}, "null d_q"),
    ({"deg": -0.5}, "min_parallax_deg must be in [0, 180]"), ({"deg": 180.5}, "min_parallax_deg must be in [0, 180]"),
    ({"deg": NAN}, "min_parallax_deg must be in [0, 180]"), ({"deg": NAN, "min_state": 3}, "min_state must be 0 .. 2"),
    ({"scale": -1.0}, SCALE), ({"scale": NAN}, SCALE), ({"scale": INF}, SCALE), ({"scale": 1e-40}, SCALE),
    ({"scale": -1.0, "deg": 181.0}, "min_parallax_deg must be in [0, 180]"),
    ({"q": ODD8}, "d_q and d_desc must be 16-byte aligned"), ({"desc": ODD8}, "d_q and d_desc must be 16-byte aligned"),
    ({"q": ODD8, "scale": -1.0}, SCALE), ({"toff": ODD4}, "d_track_offsets must be 8-byte aligned"),
    ({"toff": ODD4, "q": ODD8}, "d_q and d_desc must be 16-byte aligned"),
    ({"obs_row": ODD2}, ALIGN4), ({"counts": ODD2}, ALIGN4), ({"state": ODD2}, ALIGN4), ({"points": ODD2}, ALIGN4),
    ({"stats": ODD2}, ALIGN4), ({"stats": ODD2, "toff": ODD4}, "d_track_offsets must be 8-byte aligned"),
    ({"rows": BIG + 1}, "a total or a capacity above 2^31 - 1"), ({"tcap": BIG + 1}, "a total or a capacity above 2^31 - 1"),
    ({"ocap": 1 << 40}, "a total or a capacity above 2^31 - 1"), ({"rows": BIG, "tcap": BIG, "ocap": BIG}, "null handle"),
    ({"rows": BIG + 1, "obs_row": ODD2}, ALIGN4),
    # refuse, then the early out: an empty call with a bad scalar is still a bad call
    ({"tcap": 0, "min_state": 3}, "min_state must be 0 .. 2"),
    ({"tcap": 0, "toff": None, "counts": None, "desc": None, "q": None, "obs_row": None}, "null handle"),
]
HOST_NULLS = "null track_offsets or desc"
HOST_CASES = [
    ({}, "null handle"), ({"scale": 0.0}, "null handle"), ({"toff": None}, HOST_NULLS), ({"desc": None}, HOST_NULLS),
    ({"obs_row": None}, "null obs_row"), ({"obs_row": None, "n_obs": 0}, "null handle"), ({"q": None}, "null q"),
    ({"q": None, "rows": 0}, "null handle"), ({"min_state": 3}, "min_state must be 0 .. 2"),
    ({"deg": NAN}, "min_parallax_deg must be in [0, 180]"), ({"scale": -1.0}, SCALE), ({"scale": -1.0, "toff": None}, HOST_NULLS),
    ({"rows": BIG + 1}, "a total above 2^31 - 1"), ({"n_tracks": BIG + 1}, "a total above 2^31 - 1"),
    ({"n_obs": BIG + 1}, "a total above 2^31 - 1"), ({"q": ODD2, "toff": ODD2, "desc": ODD2}, "null handle"),
    ({"n_tracks": 0, "toff": None, "desc": None}, "null handle"), ({"n_tracks": 0, "deg": -1.0}, "min_parallax_deg must be in [0, 180]"),
]


@pytest.mark.parametrize("name, sig, cases", [("lf_mkd_track_descriptors_device", DEVICE, DEVICE_CASES),
                                              ("lf_mkd_track_descriptors", HOST, HOST_CASES)])
def test_every_refusal_has_its_prefix_and_comes_before_any_device(name, sig, cases):
    L = lfp.load_library()
    fn = getattr(L, name)
    assert len(fn.argtypes) == len(sig) + 1
    prefix = name[len("lf_mkd_"):] + ": "
    for kw, want in cases:
        assert set(kw) <= {k for k, _ in sig}, kw
        assert L.lf_mkd_match_q8_plan(5, 1, 0, None, None, None) == -1          # another message in between
        rc = fn(None, *[kw.get(k, v) for k, v in sig])
        assert rc == -1 and L.lf_mkd_last_error(None).decode() == prefix + want, (kw, rc, L.lf_mkd_last_error(None))


def test_the_symbols_are_declared_and_bound():
    assert {"lf_mkd_track_descriptors", "lf_mkd_track_descriptors_device"} <= set(lfp.SYMBOLS)
    assert callable(lfp.MkdHandle.track_descriptors) and callable(lfp.MkdHandle.track_descriptors_device)
    assert callable(lfp.LocalFeatures.track_descriptors) and callable(lfp.LocalFeatures.localize)
