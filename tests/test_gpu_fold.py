"""GPU tests of the row fold in mkd_pool (run with -m gpu on an MI355X): the kernel folds every patch row about its middle
and pools the even and the odd half of the streams against a half-width LUT (csrc/mkd_consts.hpp).  Patches built to stress
exactly that, on both folded pooling modes and both workgroup forms, against the oracle at the suite's gate."""
import numpy as np
import pytest

from conftest import DRIFT, GATE, golden, rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lfp():
    import local_features_python as m
    return m


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


def _stress_patches():
    """[kind][n, 32, 32]: exactly x-symmetric patches (every odd half o(x) = s(x) - s(31-x) vanishes up to the streams' own
    rounding), patches that are 1/2 plus an exactly x-antisymmetric part (gradients antisymmetric in x), random and blocky patches
    and their mirror images."""
    rng = np.random.default_rng(0xF01D)
    n = 48
    r = rng.random((n, 32, 32)).astype(np.float32)
    sym = (r + r[:, :, ::-1]) * np.float32(0.5)                       # a + b is commutative: exactly symmetric
    assert np.array_equal(sym, sym[:, :, ::-1])
    d = np.round((r - r[:, :, ::-1]) * 1024) / np.float32(4096)       # multiples of 2^-12 in [-1/4, 1/4]: 1/2 +- d is exact
    anti = (np.float32(0.5) + d).astype(np.float32)
    assert np.array_equal(anti - np.float32(0.5), -(anti[:, :, ::-1] - np.float32(0.5)))
    # blocks of 8 x 8 pixels plus a little noise: strong, sparse gradients
    smooth = (np.kron(rng.random((n, 4, 4)), np.ones((8, 8))) * 0.6 + 0.2 + 0.05 * rng.random((n, 32, 32))).astype(np.float32)
    assert all(len(v) == n for v in (sym, anti, r, smooth))
    return {"symmetric": sym, "antisymmetric": anti, "random": r, "random mirrored": np.ascontiguousarray(r[:, :, ::-1]),
            "blocks": smooth, "blocks mirrored": np.ascontiguousarray(smooth[:, :, ::-1])}


def _describe(lfp, torch, p, angle, pool, wide, raw=False):
    """descriptors (or the 238-D descriptors before whitening) of p; wide: through the 8-wave form (a request of more than one
    round of 64-patch workgroups), else through the one-round form"""
    reps = 1 + (64 * 400) // len(p) if wide else 1
    h = lfp.MkdHandle(max_features=len(p) * reps, angle_mode=angle, pool_mode=pool)
    dp = torch.from_numpy(np.tile(p, (reps, 1, 1))).cuda()
    out = torch.empty((len(dp), 238 if raw else 128), device="cuda")
    (h.raw_descriptors_device if raw else h.describe_patches_device)(dp.data_ptr(), len(dp), out.data_ptr())
    h.synchronize()
    if reps > 1:
        assert torch.equal(out[:len(p)], out[len(p):2 * len(p)])
    return out[:len(p)].cpu().numpy()


@pytest.mark.parametrize("wide", [False, True], ids=["one-round form", "8-wave form"])
def test_patches_that_stress_the_fold(lfp, torch, oracle, wide):
    from oracle import ATAN_LIBM, ATAN_SHADER, BLUR_CONTRACT
    kinds = _stress_patches()
    names = list(kinds)
    p = np.concatenate([kinds[k] for k in names])
    n = len(kinds[names[0]])
    worst = 0.0
    for angle, mode in ((lfp.ANGLE_SHADER, ATAN_SHADER), (lfp.ANGLE_EXACT, ATAN_LIBM)):
        ref, ref_raw = oracle.describe_patches(p, atan_mode=mode | BLUR_CONTRACT, nthreads=8, want_raw=True)
        for pool in (lfp.POOL_F16X3, lfp.POOL_F32):
            d = _describe(lfp, torch, p, angle, pool, wide)
            raw = _describe(lfp, torch, p, angle, pool, wide, raw=True)
            e, er = rel_l2(d, ref), rel_l2(raw, ref_raw)
            for i, k in enumerate(names):
                print(f"fold stress, angle {angle} pool {pool} {'W8' if wide else 'one round'}, {k}: worst relative L2 vs oracle "
                      f"{e[i * n:(i + 1) * n].max():.2e} (before whitening {er[i * n:(i + 1) * n].max():.2e})")
            assert np.isfinite(d).all()
            assert e.max() < GATE, (angle, pool, names[int(e.argmax()) // n], e.max())
            assert er.max() < GATE, (angle, pool, names[int(er.argmax()) // n], er.max())
            worst = max(worst, e.max())
            # A patch and its mirror image, against EACH OTHER's oracle result.  Mirroring a patch in x multiplies every entry
            # of the 238-D descriptor by +-1 (m(x) -> m(31-x), theta -> pi - theta, and every spatial kernel is even or odd in
            # x): the signs are read from the oracle's own pair of results, then the kernel's descriptor of the one patch must
            # be the oracle's of the other.  (The signs are exact up to the kernels' mirror defect, a few 1e-6.)
            for a, b in (("random", "random mirrored"), ("blocks", "blocks mirrored")):
                ia, ib = names.index(a) * n, names.index(b) * n
                sign = np.sign(ref_raw[ia:ia + n] * ref_raw[ib:ib + n])
                for got, want, what in ((raw[ib:ib + n], ref_raw[ia:ia + n], f"{b} vs oracle of {a}"),
                                        (raw[ia:ia + n], ref_raw[ib:ib + n], f"{a} vs oracle of {b}")):
                    em = rel_l2(sign * got, want)
                    print(f"fold stress, angle {angle} pool {pool}: {what}: worst relative L2 {em.max():.2e}")
                    assert em.max() < GATE, (angle, pool, what, em.max())
    assert worst < DRIFT, worst


def test_bench_workload_descriptors_stay_where_the_unfolded_kernel_put_them(lfp, torch, tmp_path):
    """The first 1024 rows of `bench.py --dump-outputs` on the default workload (2^20 seeded patches, shader angle, f16x3)
    against the same rows from the build before the fold (tests/golden/bench_unfolded_rows.npy): the fold changes only the
    pooling's summation and symmetrises the LUT -- 5.6e-6 relative L2 at worst over these rows when the fold was made (mean 2.6e-6),
    the size of the kernel's own distance from the oracle; the drift bar holds it."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    subprocess.check_call([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1",
                           "--dump-outputs", str(tmp_path)], timeout=600, stdout=subprocess.DEVNULL)
    got = np.load(tmp_path / "descriptors.npy")[:1024]
    want = golden("bench_unfolded_rows.npy")
    e = rel_l2(got, want)
    print(f"bench workload, folded vs unfolded build: worst relative L2 per row {e.max():.2e}, mean {e.mean():.2e}")
    assert e.max() < DRIFT, e.max()
