"""CPU tests of the view-graph call (include/lf_mkd.h, lf_mkd_view_graph_device): the float64 numpy restatement of its
definitions (tests/view_graph_cases.py) against the truth of synthetic scenes, the host twin (tests/cpp/view_graph_twin.cpp:
the kernels' own csrc/mkd_view_graph_math.h under g++) against the restatement, the edge list's order, duplicates, the
degenerate shapes, the match filter, the seam to the reconstruction chain's poses, and every refusal without a device.
tests/test_gpu_view_graph.py holds the device to the twin word for word.

Measured on cases.SEEDS (DESIGN.md 6w repeats the figures); printed by every run (pytest -s)."""
import ctypes

import numpy as np
import pytest

import reconstruction_cases as rcases
import view_graph_cases as cases
import view_graph_twin as vt

import local_features_python as lfp

NONE = cases.NONE
# The restatement's largest rotation error (rad) over the labelled images against the truth in the root's gauge, after the 10
# sweeps; the twin is bounded at twice it (the margin of DESIGN.md 6v: room for another summation order, far below a slipped
# convention -- a transposed or conjugated quaternion costs an error of the order of the rotations themselves, 1 rad).
MEASURED = dict(A=1.0777e-2, B=2.1487e-2, C=5.2344e-2, D=5.463e-3)
FACTOR = 2.0
# The twin's f32 words of rotations and residuals against the restatement's: the largest difference measured on A, B, C and D
# is 0 (the two differ in the order of f64 sums only, and the rounding to f32 hides it).  Four times nothing is nothing, so the
# gate is the number format's own step instead: one f32 ulp of 1, the largest magnitude a rotation entry or a cosine has.
GATE_MEASURED, GATE = 0.0, 2.0 ** -23
# the chain seam: the largest angle between a relative rotation of the view graph's output and that of the chain's final
# bundle poses, over the pairs of images both register (rad); the twin is bounded at twice the restatement's
SEAM_MEASURED = 3.519e-3
SCENES = dict(A=cases.scene_a, B=cases.scene_b, C=cases.scene_c, D=cases.scene_d)


@pytest.fixture(scope="module")
def scenes():
    return {k: make() for k, make in SCENES.items()}


@pytest.fixture(scope="module")
def reference(scenes):
    """the restatement on every scene: computed once, not changed"""
    return {k: cases.reference(s, **s["params"]) for k, s in scenes.items()}


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("view_graph_twin")
    exe = vt.build(tmp)
    return lambda scene, **kw: vt.run(exe, tmp, scene, **kw)


@pytest.fixture(scope="module")
def host(scenes, twin):
    return {k: twin(s, **s["params"]) for k, s in scenes.items()}


def integers_equal(got, want, what):
    for k in ("edge_stats", "image_stats", "counts"):
        assert np.array_equal(got[k], np.asarray(want[k], np.uint32)), (what, k)


def floats_close(got, want, what):
    worst = 0.0
    for k in ("rotations", "residual"):
        d = np.abs(vt.f32(got[k]).astype(np.float64) - np.asarray(want[k], np.float64).reshape(got[k].shape))
        worst = max(worst, float(d.max()) if d.size else 0.0)
    print(what, "largest f32 difference twin - restatement", worst, "gate", GATE)
    assert worst <= GATE, (what, worst)
    return worst


@pytest.mark.parametrize("which", sorted(SCENES))
def test_the_restatement_against_the_truth(scenes, reference, which):
    s, ref = scenes[which], reference[which]
    st, w = ref["edge_stats"], s["wrong"]
    assert not (st[w, 2] == cases.SUPPORTED).any(), "a wrong edge is supported"
    assert (st[w & (st[:, 0] > 0), 2] == cases.REJECTED).all(), "a wrong edge that closes a triangle is not rejected"
    ang = cases.residual_angles(ref["residual"])
    if which in "AB":
        print(which, "residual angles: right max", np.nanmax(ang[~w]), "wrong min", np.nanmin(ang[w]))
        assert np.nanmax(ang[~w]) < np.nanmin(ang[w])
    err, tree = cases.gauge_error(ref["rotations"], ref["image_stats"], s["truth"]), cases.gauge_error(ref["tree"], ref["image_stats"], s["truth"])
    print(which, "rotation error against the truth: tree", tree, "after the sweeps", err, "measured", MEASURED[which])
    assert abs(err - MEASURED[which]) <= 0.01 * MEASURED[which], (which, err)
    if which in "AB":
        assert err <= tree, (which, err, tree)
        assert (ref["image_stats"][:, 1] != NONE).all()


@pytest.mark.parametrize("which", sorted(SCENES))
def test_the_twin_against_the_restatement(scenes, reference, host, which):
    s, ref, got = scenes[which], reference[which], host[which]
    integers_equal(got, ref, which)
    floats_close(got, ref, which)
    err = cases.gauge_error(vt.f32(got["rotations"]), got["image_stats"], s["truth"])
    print(which, "the twin's rotation error against the truth", err, "bound", FACTOR * MEASURED[which])
    assert err <= FACTOR * MEASURED[which]
    # out of place: the entries of no edge keep the fill pattern, the others are the restatement's
    off, out = s["edge_offsets"].astype(np.int64), got["match_out"]
    assert (out[:off[0]] == vt.FILL).all() and (out[off[-1]:] == vt.FILL).all()
    assert np.array_equal(out[off[0]:off[-1]].view(np.int32), ref["match_out"][off[0]:off[-1]])


def test_the_edge_lists_order_does_not_matter(scenes, host, twin):
    """the sums run over the neighbours' ids, the representative and the tree's ties over values, never over the edge index"""
    s, base = scenes["A"], host["A"]
    t, perm = cases.shuffled(s)
    got = twin(t)
    back = np.empty_like(perm)
    back[perm] = np.arange(len(perm))                                          # old edge e is new edge back[e]
    es = got["edge_stats"][back].copy()
    es[:, 3] = perm[es[:, 3]]                                                  # (every edge of A is usable: a representative each)
    assert np.array_equal(es, base["edge_stats"])
    assert np.array_equal(got["residual"][back], base["residual"])
    ims = got["image_stats"].copy()
    has = ims[:, 2] != NONE
    ims[has, 2] = perm[ims[has, 2]]
    assert np.array_equal(ims, base["image_stats"])
    assert np.array_equal(got["rotations"], base["rotations"]) and np.array_equal(got["counts"], base["counts"])


def test_duplicates_and_the_edge_cases(scenes, host, twin):
    s, got = scenes["D"], host["D"]
    D, st, ims = cases.D, got["edge_stats"], got["image_stats"]
    for k in ("padding", "self_edge", "no_pose", "few_front", "nan"):
        assert st[D[k]].tolist() == [0, 0, 0, NONE], k
        assert vt.f32(got["residual"])[D[k]] == 2.0
    dup, rep = D["duplicate"], D["representative"]
    assert st[dup, :2].tolist() == st[rep, :2].tolist() and st[dup, 3] == rep == st[rep, 3] and st[dup, 2] == st[rep, 2] == cases.SUPPORTED
    off = s["edge_offsets"].astype(np.int64)
    kept_range = lambda e: got["match_out"][off[e]:off[e + 1]].view(np.int32)
    assert (kept_range(dup) == -1).all() and np.array_equal(kept_range(rep), s["match"][off[rep]:off[rep + 1]])
    # the bridge closes no triangle: unchecked, so the second cluster is not labelled by default ...
    assert st[D["bridge"]].tolist() == [0, 0, cases.UNCHECKED, D["bridge"]]
    cluster, rest = list(D["second_cluster"]), [0, 1, 2, 3, 4, 5]
    assert (ims[cluster, 1] == NONE).all() and (ims[rest, 1] != NONE).all() and ims[D["isolated"]].tolist() == [0, NONE, NONE, 0]
    rot = got["rotations"]
    assert not rot[cluster].any() and not rot[D["isolated"]].any() and rot[rest].any(1).all()
    assert got["counts"].tolist()[:6] == [20, 19, 0, 1, 18, 6] and got["counts"][6] in rest
    # ... and is under the flag, through the bridge
    flagged = twin(s, flags=cases.USE_UNCHECKED, **s["params"])
    assert (flagged["image_stats"][cluster + rest, 1] != NONE).all() and flagged["image_stats"][D["isolated"], 1] == NONE
    assert flagged["counts"].tolist()[4:6] == [19, 10] and (flagged["match_out"][off[D["bridge"]]:off[D["bridge"] + 1]].view(np.int32)
                                                           == s["match"][off[D["bridge"]]:off[D["bridge"] + 1]]).all()
    ref = cases.reference(s, flags=cases.USE_UNCHECKED, **s["params"])
    integers_equal(flagged, ref, "D under the flag")
    floats_close(flagged, ref, "D under the flag")


@pytest.mark.parametrize("kw", (dict(tree_rounds=0), dict(iterations=0), dict(tree_rounds=2, iterations=1), dict(root=5),
                                dict(deg=0.0), dict(deg=180.0), dict(min_front=150)))
def test_other_parameters(scenes, twin, kw):
    s = scenes["A"]
    got, ref = twin(s, **kw), cases.reference(s, **kw)
    integers_equal(got, ref, str(kw))
    floats_close(got, ref, str(kw))
    if kw.get("tree_rounds") == 0:
        assert got["counts"][5] == 1 and (got["image_stats"][:, 1] != NONE).sum() == 1
        root = int(got["counts"][6])
        assert vt.f32(got["rotations"][root]).tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1] and not np.delete(got["rotations"], root, 0).any()
    if "root" in kw:
        assert got["counts"][6] == 5 and got["image_stats"][5, 1] == 0
    if kw.get("deg") == 180.0:
        assert (got["edge_stats"][:, 1] == got["edge_stats"][:, 0]).all()


def test_degenerate_shapes(scenes, twin):
    s = scenes["A"]
    empty = dict(s, edge_a=s["edge_a"][:0], edge_b=s["edge_b"][:0], R=s["R"][:0], pose_stats=s["pose_stats"][:0],
                 edge_offsets=s["edge_offsets"][:1])
    got = twin(empty)
    assert not got["rotations"].any() and not got["counts"].any() and (got["image_stats"] == [0, NONE, NONE, 0]).all()
    assert (got["match_out"] == vt.FILL).all()
    got = twin(empty, root=7)
    assert vt.f32(got["rotations"][7]).tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1] and not np.delete(got["rotations"], 7, 0).any()
    assert not got["counts"].any() and got["image_stats"][7].tolist() == [0, 0, NONE, 0]
    integers_equal(got, cases.reference(empty, root=7), "no edges, a root")
    one = dict(empty, n_images=1)
    got = twin(one)
    assert not got["rotations"].any() and not got["counts"].any()
    # one image and an edge list that names nothing usable: the automatic root is image 0
    junk = dict(s, n_images=1)
    got = twin(junk)
    assert got["counts"].tolist() == [0, 0, 0, 0, 0, 1, 0, 0] and vt.f32(got["rotations"][0]).tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    integers_equal(got, cases.reference(junk), "one image")
    none = dict(empty, n_images=0)
    got = twin(none)
    assert (got["counts"] == vt.FILL).all() and got["rotations"].size == 0


def test_the_match_filter_in_place_and_out_of_place(scenes, reference, twin):
    s, ref = scenes["B"], reference["B"]
    off = s["edge_offsets"].astype(np.int64)
    out, inp, without = twin(s), twin(s, match="in place"), twin(s, match=False)
    assert without["match_out"].size == 0
    for k in ("rotations", "edge_stats", "residual", "image_stats", "counts"):
        assert np.array_equal(out[k], inp[k]) and np.array_equal(out[k], without[k]), k
    assert np.array_equal(inp["match_out"].view(np.int32), ref["match_out"])
    assert np.array_equal(inp["match_out"][:off[0]].view(np.int32), s["match"][:off[0]])            # entries of no edge survive
    assert np.array_equal(inp["match_out"][off[-1]:].view(np.int32), s["match"][off[-1]:])
    dropped = ref["edge_stats"][:, 2] != cases.SUPPORTED
    assert dropped.sum() > 30 and all((ref["match_out"][off[e]:off[e + 1]] == -1).all() for e in np.flatnonzero(dropped))
    # a layout that runs past the array is clamped to it
    short = dict(s, match=s["match"][:int(off[100]) + 2])
    got, want = twin(short, match="in place"), cases.reference(short)
    assert np.array_equal(got["match_out"].view(np.int32), want["match_out"])


def _relative_agreement(rot, labelled, poses):
    """the largest angle (rad) between R_j R_i^T of the view graph and of the poses, over the pairs both know"""
    R, P = np.asarray(rot, np.float64).reshape(-1, 3, 3), np.asarray(poses, np.float64).reshape(-1, 12)[:, :9].reshape(-1, 3, 3)
    both = [i for i in range(len(R)) if labelled[i] and P[i].any()]
    worst = 0.0
    for i in both:
        for j in both:
            worst = max(worst, cases.angle_of((R[j] @ R[i].T) @ (P[j] @ P[i].T).T))
    return worst, len(both)


def test_the_seam_to_the_reconstruction_chain(twin):
    """the chain's two-view poses (its plain scene, nothing changed) into the view graph: every posed edge is supported, and the
    rotations agree with the chain's final bundle poses"""
    s = rcases.scene()
    ch = rcases.run_chain(s, rcases.intrinsics(s), rcases.Reference())
    pose = ch["pose"]
    vg = dict(n_images=rcases.N_IMAGES, edge_a=s["edge_a"], edge_b=s["edge_b"], R=rcases.f32(pose["R"]).reshape(-1, 9),
              pose_stats=np.asarray(pose["stats"], np.uint32).reshape(-1, 4))
    ref, got = cases.reference(vg), twin(vg)
    integers_equal(got, ref, "chain")
    floats_close(got, ref, "chain")
    posed = vg["pose_stats"][:, 2] != NONE
    assert posed.sum() >= 10 and (got["edge_stats"][posed, 2] == cases.SUPPORTED).all() and (got["edge_stats"][~posed, 2] == 0).all()
    final = rcases.f32(ch["bundle"]["poses"]).reshape(-1, 12)
    a, n_ref = _relative_agreement(ref["rotations"], ref["image_stats"][:, 1] != NONE, final)
    b, n_twin = _relative_agreement(vt.f32(got["rotations"]), got["image_stats"][:, 1] != NONE, final)
    print("chain seam: relative rotations against the bundle's, restatement", a, "twin", b, "over", n_ref, "images; measured", SEAM_MEASURED)
    assert n_ref == n_twin >= 6
    assert abs(a - SEAM_MEASURED) <= 0.01 * SEAM_MEASURED and b <= FACTOR * SEAM_MEASURED


def _refused(L, rc, who, what, kw):
    assert rc == -1, (who, kw)
    msg = L.lf_mkd_last_error(None)
    assert msg.startswith(who + b": ") and what in msg, (who, kw, msg)


def test_the_symbols_and_the_plan():
    L = lfp.load_library()
    for name, arity in (("lf_mkd_view_graph_plan", 9), ("lf_mkd_view_graph_device", 23), ("lf_mkd_view_graph", 22)):
        assert name in lfp.SYMBOLS and len(getattr(L, name).argtypes) == arity
    assert hasattr(lfp.LocalFeatures, "view_graph") and hasattr(lfp.MkdHandle, "view_graph") and hasattr(lfp.MkdHandle, "view_graph_device")
    assert lfp.VIEW_GRAPH_USE_UNCHECKED == 1 and lfp.VIEW_GRAPH_AUTO_ROOT == NONE
    for n, E, T, I, m in ((24, 78, 16, 10, False), (24, 78, 16, 10, True), (300, 1200, 48, 10, True), (5, 0, 3, 2, True), (1, 0, 0, 0, False)):
        launches, scratch, form = lfp.view_graph_plan(n, E, T, I, with_match=m)
        assert launches == 3 + T + I + (2 + m if E else 0) and form == 0
        assert scratch == 32 * E + 64 * n + 4 * n * n
    assert lfp.view_graph_plan(0, 10) == (0, 0, 0)
    for kw, what in ((dict(n_images=46341), b"n_images^2"), (dict(n_edges=1 << 31), b"n_edges"), (dict(tree_rounds=4097), b"tree_rounds"),
                     (dict(iterations=4097), b"tree_rounds"), (dict(flags=2), b"unknown flag")):
        a = dict(n_images=10, n_edges=10, tree_rounds=1, iterations=1, flags=0)
        a.update(kw)
        rc = L.lf_mkd_view_graph_plan(a["n_images"], a["n_edges"], a["tree_rounds"], a["iterations"], a["flags"], 0, None, None, None)
        _refused(L, rc, b"view_graph_plan", what, kw)
    assert L.lf_mkd_view_graph_plan(46340, (1 << 31) - 1, 4096, 4096, 1, 1, None, None, None) == 0


def test_the_device_call_refuses_bad_arguments_without_a_device():
    L = lfp.load_library()
    p, odd4, odd8 = ctypes.c_void_p(64), ctypes.c_void_p(66), ctypes.c_void_p(68)
    NAN, INF = float("nan"), float("inf")

    def call(ea=p, eb=p, n_edges=10, R=p, ps=p, n_images=8, deg=3.0, min_front=0, root=NONE, tree_rounds=16, iterations=10, flags=0,
             off=None, cap=0, match=None, out=None, rot=p, es=p, res=p, ims=p, counts=p):
        return L.lf_mkd_view_graph_device(None, ea, eb, n_edges, R, ps, n_images, deg, min_front, root, tree_rounds, iterations, flags,
                                          off, cap, match, out, rot, es, res, ims, counts, None)

    triple = dict(off=p, match=p, out=p, cap=100)
    cases_ = [({}, b"null handle"), ({"res": None}, b"null handle"), (triple, b"null handle"), (dict(triple, out=p, match=p), b"null handle"),
              ({"deg": 0.0}, b"null handle"), ({"deg": 180.0}, b"null handle"), ({"root": 7}, b"null handle"), ({"flags": 1}, b"null handle"),
              ({"tree_rounds": 0, "iterations": 0}, b"null handle"), ({"tree_rounds": 4096, "iterations": 4096}, b"null handle"),
              ({"n_edges": 0, "ea": None, "eb": None, "R": None, "ps": None, "es": None}, b"null handle"),
              ({"n_images": 46340, "n_edges": (1 << 31) - 1}, b"null handle"), ({"min_front": NONE}, b"null handle"),
              ({"n_images": 0, "rot": None, "ims": None, "counts": None, "ea": None}, b"null handle")]
    cases_ += [({k: None}, b"null d_rotations") for k in ("rot", "ims", "counts")]
    cases_ += [({k: None}, b"null d_edge_a") for k in ("ea", "eb", "R", "ps", "es")]
    cases_ += [(dict(triple, **{k: None}), b"go together") for k in ("off", "match", "out")]
    cases_ += [({k: p}, b"go together") for k in ("off", "match", "out")]
    cases_ += [({"flags": 2}, b"unknown flag bits"), ({"flags": 0x80000001}, b"unknown flag bits"),
               ({"deg": -0.5}, b"max_loop_deg"), ({"deg": 180.5}, b"max_loop_deg"), ({"deg": NAN}, b"max_loop_deg"), ({"deg": INF}, b"max_loop_deg"),
               ({"root": 8}, b"root"), ({"root": NONE - 1}, b"root"),
               ({"tree_rounds": 4097}, b"tree_rounds"), ({"iterations": 4097}, b"iterations"),
               ({"n_images": 46341}, b"n_images^2"), ({"n_images": NONE, "root": 0}, b"n_images^2"), ({"n_edges": 1 << 31}, b"n_edges above"),
               (dict(triple, off=odd4), b"8-byte aligned"), (dict(triple, off=odd8), b"8-byte aligned"),
               (dict(triple, match=odd4), b"4-byte aligned"), (dict(triple, out=odd4), b"4-byte aligned"),
               (dict(triple, cap=1 << 31), b"ea_capacity")]
    cases_ += [({k: odd4}, b"4-byte aligned") for k in ("ea", "eb", "R", "ps", "rot", "es", "res", "ims", "counts")]
    for kw, what in cases_:
        _refused(L, call(**kw), b"view_graph_device", what, kw)


def test_the_host_form_refuses_bad_arguments_without_a_device():
    L = lfp.load_library()
    p = ctypes.c_void_p(64)

    def call(ea=p, eb=p, n_edges=10, R=p, ps=p, n_images=8, deg=3.0, root=NONE, tree_rounds=16, iterations=10, flags=0, off=None,
             entries=0, match=None, out=None, rot=p, es=p, res=p, ims=p, counts=p):
        return L.lf_mkd_view_graph(None, ea, eb, n_edges, R, ps, n_images, deg, 0, root, tree_rounds, iterations, flags, off, entries,
                                   match, out, rot, es, res, ims, counts)

    cases_ = [({}, b"null handle"), ({"res": None}, b"null handle"), ({"off": p, "match": p, "out": p, "entries": 9}, b"null handle"),
              ({"rot": None}, b"null rotations"), ({"counts": None}, b"null rotations"), ({"R": None}, b"null edge_a"),
              ({"es": None}, b"null edge_a"), ({"off": p}, b"go together"), ({"flags": 2}, b"unknown flag bits"),
              ({"deg": float("nan")}, b"max_loop_deg"), ({"deg": 181.0}, b"max_loop_deg"), ({"root": 8}, b"root"),
              ({"tree_rounds": 5000}, b"tree_rounds"), ({"n_images": 46341}, b"n_images^2"), ({"n_edges": 1 << 31}, b"n_edges above"),
              ({"off": p, "match": p, "out": p, "entries": 1 << 31}, b"n_entries")]
    for kw, what in cases_:
        _refused(L, call(**kw), b"view_graph", what, kw)
    # the wrapper's own checks come before the library
    with pytest.raises(RuntimeError, match="one row per entry"):
        lfp.MkdHandle.view_graph(None, [0, 1], [1], np.zeros((2, 9)), np.zeros((2, 4)), 3)
