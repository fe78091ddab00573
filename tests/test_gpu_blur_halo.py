"""GPU tests of the blur halos of mkd_pool's pair forms -- patch mode, LF_MKD_POOL_F16X3 -- (run with -m gpu on an MI355X).

Those forms pass the horizontal blur's neighbours between the lanes of a patch through records in LDS: a lane writes its eight
vertical sums into a per-wave area laid over an idle piece of the LUT row buffers and reads four values each from the
records of lanes -16 and +16, then the blurred row's edge pixels the same way (csrc/mkd_describe.hip, halo_records and
hblur_row_fold_rec).  None of that may change a bit of a descriptor: tests/golden/blur_halo_f16x3_*_rows.npy are the rows of
the build before the change, which fetched the same values with ds_bpermute (tools/dump_blur_halo_rows.py)."""
import numpy as np
import pytest

from conftest import assert_patch_parity, golden, rel_l2
from blur_halo_cases import GROUPS, halo_patches

pytestmark = pytest.mark.gpu

TOL = 2e-5                 # tests/test_gpu_row_pairs.py's bound for this mode against the oracle
N_WIDE = 32768 + 128 + 5   # the 8-wave form: 258 batches of 128 on at most 256 workgroups -- a workgroup runs two batches, so the
                           # whitening slots that overlay the record areas are used between them -- and the last batch is ragged
STRUCTURED = ("columns", "constant_along_y", "hot_pixels")


@pytest.fixture(scope="module")
def lfp():
    import local_features_python as m
    return m


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


def _describe(lfp, torch, p, angle, n):
    """descriptors (a device tensor) of the patches p tiled to n, through LF_MKD_POOL_F16X3"""
    reps = -(-n // len(p))
    h = lfp.MkdHandle(max_features=n, angle_mode=lfp.ANGLE_SHADER if angle == "shader" else lfp.ANGLE_EXACT,
                      pool_mode=lfp.POOL_F16X3)
    dp = torch.from_numpy(np.tile(p, (reps, 1, 1))[:n].copy()).cuda()
    out = torch.empty((n, 128), device="cuda")
    h.describe_patches_device(dp.data_ptr(), n, out.data_ptr())
    h.synchronize()
    return out


def _same_bits(got, want):
    got = np.ascontiguousarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape)
    diff = got.view(np.uint32) != want.view(np.uint32)
    assert not diff.any(), (int(diff.sum()), "entries differ, first in row", int(np.argwhere(diff)[0][0]))


@pytest.fixture(scope="module")
def oracle_rows(oracle):
    """the patches and the oracle's descriptors of them (the blur contracted, as the kernel's is), per angle mode"""
    from oracle import ATAN_LIBM, ATAN_SHADER, BLUR_CONTRACT
    p = halo_patches()
    ref = {name: oracle.describe_patches(p, atan_mode=mode | BLUR_CONTRACT, nthreads=8)
           for name, mode in (("shader", ATAN_SHADER), ("exact", ATAN_LIBM))}
    for v in ref.values():
        v.setflags(write=False)
    return p, ref


@pytest.mark.parametrize("angle", ["shader", "exact"])
def test_both_workgroup_forms_keep_the_parents_bits(lfp, torch, angle):
    p = halo_patches()
    want = golden(f"blur_halo_f16x3_{angle}_rows.npy")
    n = len(p)
    _same_bits(_describe(lfp, torch, p, angle, n).cpu().numpy(), want)            # one round: the 4-wave form
    wide = _describe(lfp, torch, p, angle, N_WIDE)
    for lo in range(n, N_WIDE, n):   # every repetition has the bits of the first, the ragged tail included
        hi = min(lo + n, N_WIDE)
        assert torch.equal(wide[lo:hi], wide[:hi - lo]), (lo, "a repeated block differs")
    _same_bits(wide[:n].cpu().numpy(), want)


@pytest.mark.parametrize("angle", ["shader", "exact"])
def test_halos_against_the_oracle(lfp, torch, oracle, oracle_rows, angle):
    from oracle import ATAN_LIBM, ATAN_SHADER
    p, ref = oracle_rows
    got = _describe(lfp, torch, p, angle, len(p)).cpu().numpy()
    assert np.isfinite(got).all()
    e = rel_l2(got, ref[angle])
    worst = {name: float(e[lo:lo + n].max()) for name, (lo, n) in GROUPS.items()}
    print(f"{angle} angle: worst relative L2 against the oracle -- " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for name in STRUCTURED:
        lo, n = GROUPS[name]
        assert worst[name] < TOL, (name, lo + int(e[lo:lo + n].argmax()), worst[name])
    lo, n = GROUPS["random"]
    assert assert_patch_parity(oracle, p[lo:lo + n], got[lo:lo + n], ATAN_SHADER if angle == "shader" else ATAN_LIBM,
                               what=("blur halos", angle)) < TOL


@pytest.mark.parametrize("n", [1, 17])
@pytest.mark.parametrize("angle", ["shader", "exact"])
def test_a_lone_patch_and_a_partly_filled_wave(lfp, torch, oracle_rows, angle, n):
    """n = 1: fifteen lanes of sixteen recompute the last patch, so every record of a segment holds the same values;
    n = 17: the second wave holds one patch.  The patches are the first of the set: a column of 1.0 at x = 0, 1, ..."""
    p, ref = oracle_rows
    got = _describe(lfp, torch, p[:n], angle, n).cpu().numpy()
    e = rel_l2(got, ref[angle][:n])
    print(f"n = {n}, {angle} angle: worst relative L2 against the oracle {e.max():.2e}")
    _same_bits(got, golden(f"blur_halo_f16x3_{angle}_rows.npy")[:n])
    assert e.max() < TOL, e.max()
