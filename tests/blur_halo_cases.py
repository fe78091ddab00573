"""Patches for tests/test_gpu_blur_halo.py and tools/dump_blur_halo_rows.py (which records the parent build's descriptors of
the same patches): what a blur halo taken from the wrong lane, the wrong plane of a halo record or a stale record in
mkd_pool's pair forms would show on.  A lane holds the pixels x in [4q, 4q+4) and [28-4q, 32-4q) of a patch row, so the
block edges are 3|4, 7|8, 11|12, the fold's seam 15|16 and their mirrors, and the patch's edges 0 and 31 replicate."""
import numpy as np

HOT_X = (0, 3, 4, 15, 16, 27, 28, 31)
HOT_Y = (0, 16)
# the groups, in the order of the set: name -> (first patch, number of patches)
GROUPS = {"columns": (0, 32), "constant_along_y": (32, 64), "hot_pixels": (96, 16), "random": (112, 64)}


def halo_patches():
    """[32 + 64 + 16 + 64, 32, 32] = 11 waves of 16 patches, no two patches alike (so a record read from another patch's lane shows):
    32 patches with one column of 1.0 at x = 0..31 and 16 with one pixel of 1.0 at HOT_X x HOT_Y, both on a uniform
    background in [0, 0.05); 64 patches constant along y whose 32 columns all differ (the transposes of row_pairs_cases' row
    patches: gy is 0, every pixel's gx crosses a block edge somewhere); 64 random."""
    rng = np.random.default_rng(0xB10A)
    cols = rng.random((32, 32, 32), dtype=np.float32) * np.float32(0.05)
    for c in range(32):
        cols[c, :, c] = 1.0
    along_y = np.repeat(rng.random((64, 1, 32), dtype=np.float32), 32, axis=1)
    hot = rng.random((len(HOT_X) * len(HOT_Y), 32, 32), dtype=np.float32) * np.float32(0.05)
    for i, (y, x) in enumerate((y, x) for y in HOT_Y for x in HOT_X):
        hot[i, y, x] = 1.0
    p = np.ascontiguousarray(np.concatenate([cols, along_y, hot, rng.random((64, 32, 32), dtype=np.float32)]))
    assert len(p) == sum(n for _, n in GROUPS.values()) and len(p) % 16 == 0
    return p
