"""GPU tests of the x-odd cartesian columns of mkd_pool in LF_MKD_POOL_F16X3 (run with -m gpu on an MI355X).

That mode spends no matrix instruction on the three x-odd cartesian kernels EC 6, 7, 8: the 21 descriptor entries
175 + 9 i + 6 + b (in-dim i = 0..6, b = 0..2) are summed in f32 on the vector ALU as gy_b(y) * sum_x fx(x) s_o(x, y) and put
back into their accumulator tiles once per batch (csrc/mkd_describe.hip, valu_odd_cart).  A whole-row L2 could hide a wrong
small column, so these tests look at the 21 entries alone as well."""
import numpy as np
import pytest

from conftest import DRIFT, GATE, golden, kp_form, rel_l2

pytestmark = pytest.mark.gpu

ODD_CART = np.array([175 + 9 * i + 6 + b for i in range(7) for b in range(3)])


@pytest.fixture(scope="module")
def lfp():
    import local_features_python as m
    return m


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


def _patches():
    """[kind][48, 32, 32]: random and blocky patches, their mirror images, and left-right ramps 0.5 + a (x - 15.5) / 31 plus
    5 % noise.  The 21 entries carry 2-6 % of the raw norm of a random patch and 6-23 % of a blocky one.  A ramp is odd in x
    about 1/2, but its gradient is constant: the streams' odd halves are the noise's alone and the entries 0.2-1 % of the
    norm -- the hardest case for an error measured relative to the 21 entries themselves."""
    rng = np.random.default_rng(0x0DDCA27)
    n = 48
    r = rng.random((n, 32, 32)).astype(np.float32)
    blocks = (np.kron(rng.random((n, 4, 4)), np.ones((8, 8))) * 0.6 + 0.2 + 0.05 * rng.random((n, 32, 32))).astype(np.float32)
    a = rng.uniform(0.3, 0.8, (n, 1, 1)) * rng.choice([-1.0, 1.0], (n, 1, 1))
    x = np.arange(32, dtype=np.float64)[None, None, :]
    ramps = (0.5 + a * (x - 15.5) / 31 + 0.05 * (rng.random((n, 32, 32)) - 0.5)).astype(np.float32)
    return {"random": r, "blocks": blocks, "random mirrored": np.ascontiguousarray(r[:, :, ::-1]),
            "blocks mirrored": np.ascontiguousarray(blocks[:, :, ::-1]), "ramps": ramps}


@pytest.fixture(scope="module")
def cases(oracle):
    """the 240 patches and the oracle's 238-D descriptors before whitening, per angle mode: computed once"""
    from oracle import ATAN_LIBM, ATAN_SHADER, BLUR_CONTRACT
    kinds = _patches()
    p = np.concatenate(list(kinds.values()))
    assert len(p) == 240
    ref = {name: oracle.describe_patches(p, atan_mode=mode | BLUR_CONTRACT, nthreads=8, want_raw=True)[1]
           for name, mode in (("shader", ATAN_SHADER), ("exact", ATAN_LIBM))}
    for v in ref.values():
        v.setflags(write=False)
    return list(kinds), p, ref


def _raw(lfp, torch, p, angle, n):
    """the 238-D descriptors before whitening of the 240 patches tiled to n, through LF_MKD_POOL_F16X3"""
    reps = -(-n // len(p))
    h = lfp.MkdHandle(max_features=n, angle_mode=angle, pool_mode=lfp.POOL_F16X3)
    dp = torch.from_numpy(np.tile(p, (reps, 1, 1))[:n].copy()).cuda()
    out = torch.empty((n, 238), device="cuda")
    h.raw_descriptors_device(dp.data_ptr(), n, out.data_ptr())
    h.synchronize()
    return out


# n = 240: the one-round (4-wave) form.  n = 32768 + 128 + 5: the 8-wave form, 258 batches of 128 on at most 256 workgroups:
# a workgroup runs two batches (sums not reset between batches would show) and the last batch is ragged (5 patches)
@pytest.mark.parametrize("n", [240, 32768 + 128 + 5], ids=["one-round form", "8-wave form"])
@pytest.mark.parametrize("angle", ["shader", "exact"])
def test_odd_cartesian_columns_against_the_oracle(lfp, torch, cases, angle, n):
    names, p, ref = cases
    want = ref[angle]
    out = _raw(lfp, torch, p, lfp.ANGLE_SHADER if angle == "shader" else lfp.ANGLE_EXACT, n)
    # every repetition of the 240 patches has the bits of the first, the ragged tail included
    first = out[:240]
    for lo in range(240, n, 240):
        hi = min(lo + 240, n)
        assert torch.equal(out[lo:hi], first[:hi - lo]), (lo, "a repeated block differs")
    got = first.cpu().numpy()
    assert np.isfinite(got).all()
    e_sub = rel_l2(got[:, ODD_CART], want[:, ODD_CART])
    e_row = rel_l2(got, want)
    share = np.linalg.norm(want[:, ODD_CART], axis=1) / np.linalg.norm(want, axis=1)
    for i, k in enumerate(names):
        s = slice(48 * i, 48 * (i + 1))
        print(f"odd cartesian columns, {angle} angle, n = {n}, {k}: worst relative L2 of the 21 entries {e_sub[s].max():.2e}, "
              f"of the row {e_row[s].max():.2e}; the entries' share of the row norm {share[s].min():.3f} .. {share[s].max():.3f}")
    assert e_sub.max() < GATE, (names[int(e_sub.argmax()) // 48], e_sub.max())
    big = np.abs(want[:, ODD_CART]) > 1e-3 * np.linalg.norm(want, axis=1, keepdims=True)
    assert big[:192].any(axis=1).all()    # (not vacuous: every random and blocky patch has such entries)
    assert np.array_equal(np.sign(got[:, ODD_CART])[big], np.sign(want[:, ODD_CART])[big])
    assert e_row.max() < GATE, (names[int(e_row.argmax()) // 48], e_row.max())
    assert e_row.max() < DRIFT, e_row.max()


def test_keypoint_forms_agree(lfp, torch):
    """33 keypoints (two batches of 32: one full, one ragged) on a smooth 256 x 256 frame through every form of the keypoint
    kernel: 2 + 2 waves whole-patch, row-split over 2 and over 4 workgroups (the partial sums of the 21 columns are
    rebuilt into their tiles before they are published), and -- tiled beyond one round of 32-keypoint workgroups -- 4 + 4."""
    rng = np.random.default_rng(0xCA27)
    y, x = np.mgrid[0:256, 0:256].astype(np.float64)
    img = (0.5 + 0.2 * np.sin(x / 9.0) * np.cos(y / 13.0) + 0.15 * np.sin((x + 2 * y) / 23.0) + 0.1 * np.cos((3 * x - y) / 31.0))
    img = img.astype(np.float32)
    n = 33
    k5 = np.stack([rng.uniform(48, 208, n), rng.uniform(48, 208, n), rng.uniform(6, 20, n), rng.uniform(0, 360, n),
                   np.ones(n)], axis=1).astype(np.float32)
    reps = 8192 // n + 2                      # > 32 keypoints x 256 CUs: the 4 + 4 form
    h = lfp.MkdHandle(max_features=n * reps, max_image_width=256, max_image_height=256)
    h.set_image(img)
    with kp_form(1):
        whole = h.describe_keypoints(k5)
    assert np.isfinite(whole).all()
    for form in (2, 4):
        with kp_form(form):
            d = h.describe_keypoints(k5)
        e = rel_l2(d, whole).max()
        print(f"row-split form R = {form} vs the whole-patch 2 + 2 form: worst relative L2 {e:.2e}")
        assert e < DRIFT, (form, e)
    wide = h.describe_keypoints(np.tile(k5, (reps, 1)))
    assert np.array_equal(wide[:n], wide[n:2 * n])
    e = rel_l2(wide[:n], whole).max()
    print(f"4 + 4 form vs the whole-patch 2 + 2 form: worst relative L2 {e:.2e}")
    assert e < DRIFT, e


@pytest.mark.parametrize("pool", ["f32", "fp6"])
@pytest.mark.parametrize("angle", ["shader", "exact"])
def test_the_other_pooling_modes_keep_their_bits(lfp, torch, pool, angle):
    """LF_MKD_POOL_F32 and LF_MKD_POOL_F16_FP6 keep meeting every LUT tile with matrix instructions: 256 seeded patches
    against the rows the build before the change gave (tools/dump_pool_mode_rows.py), bit for bit"""
    p = torch.from_numpy(np.random.default_rng(0xB175).random((256, 32, 32), dtype=np.float32)).cuda()
    h = lfp.MkdHandle(max_features=256, angle_mode=lfp.ANGLE_SHADER if angle == "shader" else lfp.ANGLE_EXACT,
                      pool_mode=lfp.POOL_F32 if pool == "f32" else lfp.POOL_F16_FP6)
    out = torch.empty((256, 128), device="cuda")
    h.describe_patches_device(p.data_ptr(), 256, out.data_ptr())
    h.synchronize()
    want = golden(f"pool_{pool}_{angle}_rows.npy")
    got = out.cpu().numpy()
    assert got.dtype == want.dtype and np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
        int((got.view(np.uint32) != want.view(np.uint32)).sum())
