"""Patches for tests/test_gpu_row_pairs.py and tools/dump_f16x3_rows.py (which records the parent build's descriptors of the
same patches): what a wrong ring slot, a wrong replicated row or a late raw row in mkd_pool's row pairs would show on."""
import numpy as np

HOT_ROWS = (0, 1, 2, 5, 6, 29, 30, 31)   # the first body, the first pair, the slot wrap (rows 5 -> 6), the last pair, row 31


def seeded_patches():
    """the 256 random patches of tools/dump_pool_mode_rows.py"""
    return np.random.default_rng(0xB175).random((256, 32, 32), dtype=np.float32)


def structured_patches():
    """[64 + 8 + 64, 32, 32]: 64 patches constant along x whose 32 rows all differ (a row taken from the wrong slot, or
    replicated from the wrong row, changes gy of whole rows), 8 patches with one row of 1.0 on 0.0 at HOT_ROWS, 64 random."""
    rng = np.random.default_rng(0x20A5)
    rows = np.repeat(rng.random((64, 32, 1), dtype=np.float32), 32, axis=2)
    hot = np.zeros((len(HOT_ROWS), 32, 32), np.float32)
    for i, y in enumerate(HOT_ROWS):
        hot[i, y, :] = 1.0
    return np.ascontiguousarray(np.concatenate([rows, hot, rng.random((64, 32, 32), dtype=np.float32)]))
