"""Plain reference of the frame ingest (os_frames_ingest): Pillow's convert('RGB').resize((S, S), BILINEAR).convert('L') followed by
ToTensor's division, restated in numpy int64.  tests/test_frames_ref_cpu.py pins it to Pillow itself; the GPU tests compare with it."""
import math

import numpy as np

PB = 22      # fixed-point bits of a coefficient


def axis_table(n_in, n_out):
    """(coef [n_out][ksize] int64, lo [n_out], cnt [n_out]) of the triangle filter, every step in IEEE double in Pillow's order."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    ss = 1.0 / fs
    coef = np.zeros((n_out, 2 * int(math.ceil(support)) + 1), np.int64)
    lo, cnt = np.zeros(n_out, np.int64), np.zeros(n_out, np.int64)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - xmin
        w = [abs((x + xmin - center + 0.5) * ss) for x in range(n)]
        w = [1.0 - a if a < 1.0 else 0.0 for a in w]
        ww = 0.0
        for v in w:             # left to right
            ww += v
        for x in range(n):
            coef[xx, x] = int(0.5 + (w[x] / ww if ww != 0.0 else w[x]) * (1 << PB))
        lo[xx], cnt[xx] = xmin, n
    return coef, lo, cnt


def resample(a, n_out, axis):
    """One pass along `axis` of a uint8 array; an axis that already has n_out entries passes through."""
    if a.shape[axis] == n_out:
        return a
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    coef, lo, cnt = axis_table(a.shape[0], n_out)
    out = np.empty((n_out,) + a.shape[1:], np.int64)
    for xx in range(n_out):
        acc = (1 << (PB - 1)) + np.tensordot(coef[xx, :cnt[xx]], a[lo[xx]:lo[xx] + cnt[xx]], axes=(0, 0))
        out[xx] = np.clip(acc >> PB, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def ingest(frames, size):
    """frames [N][H][W][C] uint8, C = 1 | 3 -> [N][size][size] float32: horizontal pass, vertical pass, luma, / 255."""
    t = resample(resample(frames, size, 2), size, 1).astype(np.int64)
    lum = t[..., 0] if t.shape[3] == 1 else (19595 * t[..., 0] + 38470 * t[..., 1] + 7471 * t[..., 2] + 32768) >> 16
    return lum.astype(np.float32) / np.float32(255)


def batch(H, W, C, seed=0):
    """The three test images of a geometry: seeded random bytes, all 255, a 0 / 255 checkerboard."""
    fr = np.empty((3, H, W, C), np.uint8)
    fr[0] = np.random.default_rng(seed).integers(0, 256, (H, W, C), dtype=np.uint8)
    fr[1] = 255
    fr[2] = (((np.arange(H)[:, None] + np.arange(W)[None, :]) & 1) * 255).astype(np.uint8)[:, :, None]
    return fr
