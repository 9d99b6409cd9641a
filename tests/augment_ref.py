"""Plain reference of the frame augmentation (os_frames_augment): Pillow's nearest-neighbour rotate and transform(PERSPECTIVE), the
two flips and crop().resize(BILINEAR) on an S x S uint8 image, restated in numpy.  tests/test_augment_ref_cpu.py pins it to Pillow
itself; the GPU tests compare with it."""
import numpy as np

import frames_ref


def _pick(g, xi, yi):
    """g[yi][xi] where the index is inside the image, 0 elsewhere."""
    S = g.shape[0]
    ok = (xi >= 0) & (xi < S) & (yi >= 0) & (yi < S)
    return np.where(ok, g[np.clip(yi, 0, S - 1), np.clip(xi, 0, S - 1)], 0).astype(np.uint8)


def rotate(g, a):
    """transform(AFFINE, a, NEAREST): 16.16 fixed point in 32-bit integers that wrap."""
    fix = lambda v: np.int64(np.floor(v * 65536.0 + 0.5))           # noqa: E731
    A = [fix(a[0]), fix(a[1]), fix(a[2] + a[0] * 0.5 + a[1] * 0.5), fix(a[3]), fix(a[4]), fix(a[5] + a[3] * 0.5 + a[4] * 0.5)]
    y, x = np.mgrid[0:g.shape[0], 0:g.shape[0]].astype(np.int64)
    wrap = lambda v: ((v + 2 ** 31) % 2 ** 32 - 2 ** 31) >> 16      # noqa: E731
    return _pick(g, wrap(A[2] + y * A[1] + x * A[0]), wrap(A[5] + y * A[4] + x * A[3]))


def perspective(g, c):
    """transform(PERSPECTIVE, c, NEAREST): float64, a coordinate below 0 is -1, anything else truncates."""
    y, x = np.mgrid[0:g.shape[0], 0:g.shape[0]].astype(np.float64) + 0.5
    with np.errstate(all="ignore"):
        den = c[6] * x + c[7] * y + 1.0
        xs, ys = (c[0] * x + c[1] * y + c[2]) / den, (c[3] * x + c[4] * y + c[5]) / den
        coord = lambda v: np.where(v >= 0, np.minimum(v, 2.0 ** 31), -1.0).astype(np.int64)     # noqa: E731  (a NaN is outside)
        return _pick(g, coord(xs), coord(ys))


def crop_resize(q, top, left, h, w):
    """crop((left, top, left + w, top + h)).resize((S, S), BILINEAR): horizontal pass rounded to uint8, then the vertical one."""
    S = q.shape[0]
    return frames_ref.resample(frames_ref.resample(q[top:top + h, left:left + w], S, 1), S, 0)


def cases(S):
    """name -> (angle, vflip, hflip, perspective coefficients, crop (top, left, h, w)) for Pillow and optistate_amd.augment.record."""
    from optistate_amd.augment import perspective_coeffs
    d = S // 5
    persp = perspective_coeffs([[0, 0], [S - 1, 0], [S - 1, S - 1], [0, S - 1]], [[d, 2], [S - 3, d // 2], [S - 1 - d, S - 2], [1, S - 1 - d]])
    flip = [0.9, 0.05, 1.0, -0.03, 1.1, 2.0, -2.0 / S, 0.001]       # the denominator changes sign near x = S / 2
    wmin, hmin, e = int(S * 0.72 ** 0.5), int(S * (0.8 / 0.9) ** 0.5), S - S // 10
    return {"none": (None, False, False, None, None),
            "rotate": (7.3, False, False, None, None), "vflip": (None, True, False, None, None), "hflip": (None, False, True, None, None),
            "perspective": (None, False, False, persp, None), "crop": (None, False, False, None, (S // 10, S // 8, S - S // 5, S - S // 4)),
            "all": (-4.6, True, True, persp, (2, 3, e, e - 1)),
            "rotate+10": (10.0, False, False, None, None), "rotate-10": (-10.0, False, False, None, None),
            "perspective-sign": (None, False, False, flip, None),
            "crop-origin": (None, False, False, None, (0, 0, e, e)), "crop-far": (None, False, False, None, (S - e, S - e - 1, e, e + 1)),
            "crop-full": (None, False, False, None, (0, 0, S, S)), "crop-smallest": (3.0, False, True, None, (3, 5, hmin, wmin))}


def augment(gray, params):
    """gray [N][S][S] uint8, params [N][20] float64 -> [N][S][S] float32: rotate, vflip, hflip, perspective, crop, / 255."""
    out = np.empty(gray.shape, np.float32)
    for n, (g, p) in enumerate(zip(gray, params)):
        flags = int(p[14])
        g = rotate(g, p[0:6]) if flags & 1 else g
        g = g[::-1] if flags & 2 else g
        g = g[:, ::-1] if flags & 4 else g
        g = perspective(g, p[6:14]) if flags & 8 else g
        g = crop_resize(g, *(int(v) for v in p[15:19])) if flags & 16 else g
        out[n] = g.astype(np.float32) / np.float32(255)
    return out
