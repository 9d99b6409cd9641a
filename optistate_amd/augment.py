"""Host side of the frame augmentation (Engine.augment_frames / os_frames_augment): the per-image parameter records of the
auto-encoder's training transform between Grayscale and ToTensor (transformer/autoencoder_training.py:45-52)

    RandomRotation(+-10) -> RandomVerticalFlip(.5) -> RandomHorizontalFlip(.5) -> RandomPerspective(p=.5)
    -> RandomApply([RandomResizedCrop(S, scale=(.8, 1), ratio=(.9, 1.1))], p=.3)

The randomness lives here and only here; the device applies explicit records, bit for bit as Pillow would.  A record is 20 float64
(include/optistate_hip.h): [0:6] the affine matrix of Image.rotate, [6:14] Pillow's PERSPECTIVE coefficients, [14] flags,
[15:19] crop top, left, height, width, [19] 0.  numpy and the standard library only.
"""
import math

import numpy as np

ROTATE, VFLIP, HFLIP, PERSPECTIVE, CROP = 1, 2, 4, 8, 16
RECORD = 20


def rotation_matrix(angle, S):
    """The six coefficients that PIL's Image.rotate(angle) (expand=False, no center, no translate) builds for an S x S image and
    hands to transform(AFFINE) -- its own Python arithmetic, the decimal round(., 15) of cos and sin included -- or None where
    rotate takes a fast path and the rotation stage must stay off: `angle % 360` of 0 (a copy).  180 and, for a square image, 90 and
    270 are transposes in Pillow, which its affine path does not reproduce: they raise."""
    angle = angle % 360.0
    if angle == 0:
        return None
    if angle in (90, 180, 270):
        raise ValueError("optistate_amd.augment: Image.rotate turns 90 / 180 / 270 degrees into a transpose, not an affine transform")
    center = (S / 2, S / 2)
    angle = -math.radians(angle)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    x, y = -center[0], -center[1]
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += center[0]
    m[5] += center[1]
    return m


def perspective_coeffs(startpoints, endpoints):
    """Pillow's PERSPECTIVE data (c0..c7, output pixel -> input pixel) of the map that takes the four `startpoints` to the four
    `endpoints`, as torchvision's functional perspective() sets it up: the 8 x 8 system solved in float64."""
    a = np.zeros((8, 8), np.float64)
    for i, (p1, p2) in enumerate(zip(endpoints, startpoints)):
        a[2 * i] = [p1[0], p1[1], 1, 0, 0, 0, -p2[0] * p1[0], -p2[0] * p1[1]]
        a[2 * i + 1] = [0, 0, 0, p1[0], p1[1], 1, -p2[1] * p1[0], -p2[1] * p1[1]]
    b = np.asarray(startpoints, np.float64).reshape(8)
    return np.linalg.solve(a, b).tolist()


def record(S, angle=None, vflip=False, hflip=False, perspective=None, crop=None):
    """One record.  angle: degrees for Image.rotate; perspective: the eight coefficients; crop: (top, left, height, width) inside
    the image.  What is None / False leaves its stage off."""
    r = np.zeros(RECORD, np.float64)
    flags = 0
    m = rotation_matrix(angle, S) if angle is not None else None
    if m is not None:
        r[0:6], flags = m, flags | ROTATE
    flags |= (VFLIP if vflip else 0) | (HFLIP if hflip else 0)
    if perspective is not None:
        r[6:14], flags = perspective, flags | PERSPECTIVE
    if crop is not None:
        top, left, h, w = (int(v) for v in crop)
        if not (0 <= top and 0 <= left and 1 <= h and 1 <= w and top + h <= S and left + w <= S):
            raise ValueError(f"optistate_amd.augment: crop {tuple(crop)} is not inside a {S} x {S} image")
        r[15:19], flags = (top, left, h, w), flags | CROP
    r[14] = flags
    return r


def _perspective_points(S, distortion, rng):
    """torchvision's RandomPerspective.get_params as documented: every corner moves inwards by up to distortion * S // 2 per axis."""
    d = int(distortion * (S // 2))
    lo = lambda: int(rng.integers(0, d + 1))              # noqa: E731
    hi = lambda: int(rng.integers(S - d - 1, S))          # noqa: E731
    topleft = [lo(), lo()]
    topright = [hi(), lo()]
    botright = [hi(), hi()]
    botleft = [lo(), hi()]
    return [[0, 0], [S - 1, 0], [S - 1, S - 1], [0, S - 1]], [topleft, topright, botright, botleft]


def _crop_box(S, scale, ratio, rng):
    """RandomResizedCrop.get_params: ten tries for an area in `scale` and a log-uniform aspect in `ratio`, then the centre crop."""
    for _ in range(10):
        area = S * S * rng.uniform(scale[0], scale[1])
        aspect = math.exp(rng.uniform(math.log(ratio[0]), math.log(ratio[1])))
        w, h = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
        if 0 < w <= S and 0 < h <= S:
            return int(rng.integers(0, S - h + 1)), int(rng.integers(0, S - w + 1)), h, w
    return 0, 0, S, S              # a square image's ratio of 1 lies inside `ratio`: the whole image


def sample_params(N, S, generator=None):
    """[N][20] float64 records with the reference's probabilities and ranges: angle uniform in [-10, 10]; each flip with
    probability .5; a perspective with probability .5, corners as torchvision documents get_params at distortion_scale .5; with
    probability .3 a crop of scale (.8, 1), ratio (.9, 1.1) resized back to S x S.  `generator`: a numpy Generator or a seed.
    Which draw comes first, and how a draw maps to a number, follows torchvision's documented order but cannot be checked against
    torchvision here (it is not a dependency and its stream is torch's): a seed does not reproduce torchvision's augmentations.
    The record is the contract -- what a record does is pinned to Pillow.  Move the result to the device (torch.from_numpy(...)
    .cuda()) for Engine.augment_frames."""
    rng = generator if isinstance(generator, np.random.Generator) else np.random.default_rng(generator)
    out = np.zeros((N, RECORD), np.float64)
    for n in range(N):
        angle = float(rng.uniform(-10.0, 10.0))
        vflip, hflip = bool(rng.random() < 0.5), bool(rng.random() < 0.5)
        persp = perspective_coeffs(*_perspective_points(S, 0.5, rng)) if rng.random() < 0.5 else None
        crop = _crop_box(S, (0.8, 1.0), (0.9, 1.1), rng) if rng.random() < 0.3 else None
        out[n] = record(S, angle, vflip, hflip, persp, crop)
    return out
