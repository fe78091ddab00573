"""The global route on the host (tests/positions_route.py) on the collection of tests/reconstruction_cases.py: the twins'
route against the numpy restatements' and against the truth.  No GPU.

The numpy route's own largest centre errors (after a similarity fit, in units of the true centres' rms radius):
    after global positions   1.9651e-2   ->  bound 3.930e-2          (the view graph's rotations are held: they are the floor)
    after the bundle         6.2392e-3   ->  bound 1.248e-2
All 8 images come out registered: image 3, whose 18 points are too few for the incremental chain's resection (min_inliers 20),
is labelled by the view graph and solved by the positions call like any other camera."""
import numpy as np
import pytest

import positions_route as route
import positions_twin as pt
import reconstruction_cases as cases
import reconstruction_twin as rtwin
import view_graph_twin as vgt

BOUND = dict(positions=2 * 1.9651e-2, bundle=2 * 6.2392e-3)
GATE = 2.0 ** -23


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("positions_route")
    twins, exe_vg, exe_gp = rtwin.Twins(tmp), vgt.build(tmp), pt.build(tmp)
    s = cases.scene()
    K = cases.intrinsics(s)
    ch = rtwin.run(twins, s, K)
    return s, ch, route.twin_route(twins, exe_vg, exe_gp, tmp, s, K, ch), route.numpy_route(s, K, ch)


def test_the_numpy_route_finds_the_truth(routes):
    s, ch, _, ref = routes
    for stage, poses in (("positions", ref["positions"]["poses"]), ("bundle", cases.f32(ref["bundle"]["poses"]))):
        err, registered = route.centre_error(s, poses)
        print("%s: the numpy route's largest centre error %.5g over %d images" % (stage, err, registered))
        assert registered == cases.N_IMAGES and err <= BOUND[stage] / 2 * 1.0005


def test_the_twin_route_agrees_and_finds_the_truth(routes):
    s, ch, tw, ref = routes
    gp, want = tw["positions"], ref["positions"]
    T = ch["table"].counts[0]
    assert np.array_equal(gp["image_stats"], want["image_stats"]) and np.array_equal(gp["counts"], want["counts"])
    assert np.abs(cases.f32(gp["poses"]).reshape(-1, 12) - want["poses"]).max() <= GATE
    assert np.abs(cases.f32(gp["points"]).reshape(-1, 4)[:T] - want["points"]).max() <= GATE
    for stage, poses in (("positions", cases.f32(gp["poses"])), ("bundle", cases.f32(tw["bundle"]["poses"]))):
        err, registered = route.centre_error(s, poses)
        assert registered == cases.N_IMAGES and err <= BOUND[stage], (stage, err)
    # image 3 is labelled by the view graph and solved here, from its 18 rows
    assert tw["view_graph"]["image_stats"][cases.UNREGISTERABLE, 1] != 0xFFFFFFFF
    assert gp["image_stats"][cases.UNREGISTERABLE].tolist() == [18, 18, 0, 0]
    assert cases.tracks_with_point(tw["tri"], T) > 0.9 * T
