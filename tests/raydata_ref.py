"""Independent restatements for the data-layer tests (tests/test_raydata_cpu.py, tests/test_raydata_gpu.py):

* `perm`: the epoch permutation of csrc/ray_perm.hpp in NumPy (vectorised over positions, uint64 arithmetic);
* `colours`: the reference's image arithmetic on bytes with torch CPU ops: `/ 255.0` in float64 rounded to float32
  (blender.py:246; splitter.py:331 + llff.py:40) and the white-background composition of blender.py:114-117."""
import numpy as np
import torch

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _mix(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def perm(n: int, seed: int, epoch: int, start: int = 0, count: int = None) -> np.ndarray:
    """positions [start, start + count) of the permutation of [0, n) keyed by (seed, epoch), int64."""
    count = n - start if count is None else count
    k = 1
    while (1 << (2 * k)) < n:
        k += 1
    kb, mask = np.uint64(k), np.uint64((1 << k) - 1)
    base = _mix(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) ^ _mix(np.uint64(epoch)))
    with np.errstate(over="ignore"):
        keys = [_mix(base + np.uint64(r)) for r in range(4)]
    x = np.arange(start, start + count, dtype=np.uint64)
    todo = np.ones(count, dtype=bool)
    walks = 0
    while todo.any():
        v = x[todo]
        left, right = (v >> kb) & mask, v & mask
        for key in keys:
            f = (_mix(right ^ key) >> np.uint64(32)) & mask
            left, right = right, left ^ f
        v = (left << kb) | right
        x[todo] = v
        todo[todo] = v >= np.uint64(n)
        walks += 1
        assert walks <= (1 << (2 * k)), "cycle walking did not end"
    return x.astype(np.int64)


def colours(imgs_u8, white_bkgd: bool) -> torch.Tensor:
    """uint8 [..., 3|4] -> float32 [..., 3] as the reference's datasets hold them."""
    f = torch.from_numpy((np.asarray(imgs_u8) / 255.0).astype(np.float32))
    if white_bkgd:
        return f[..., :3] * f[..., -1:] + (1.0 - f[..., -1:])
    return f[..., :3]
