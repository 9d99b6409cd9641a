"""CPU: the numpy restatement of the frame augmentation (tests/augment_ref.py) and the host helpers that build its records
(optistate_amd/augment.py) equal Pillow itself, pixel for pixel, on the cases of tests/test_gpu_augment.py."""
import numpy as np
import pytest

import augment_ref
import frames_ref
from optistate_amd import augment

SIZES = (224, 40)
NAMES = sorted(augment_ref.cases(40))


def pillow_chain(Image, g, angle, vflip, hflip, persp, crop):
    S = g.shape[0]
    im = Image.fromarray(g)
    if angle is not None:
        im = im.rotate(angle, Image.NEAREST, fillcolor=0)
    if vflip:
        im = im.transpose(Image.FLIP_TOP_BOTTOM)
    if hflip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    if persp is not None:
        im = im.transform((S, S), Image.PERSPECTIVE, persp, Image.NEAREST, fillcolor=0)
    if crop is not None:
        top, left, h, w = crop
        im = im.crop((left, top, left + w, top + h)).resize((S, S), Image.BILINEAR)
    return np.asarray(im, np.float32) / np.float32(255)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("S", SIZES)
def test_restatement_and_records_equal_pillow(S, name):
    Image = pytest.importorskip("PIL.Image")
    case = augment_ref.cases(S)[name]
    gray = frames_ref.batch(S, S, 1, seed=S)[..., 0]
    mine = augment_ref.augment(gray, np.stack([augment.record(S, *case)] * 3))
    for n in range(3):
        assert np.array_equal(mine[n], pillow_chain(Image, gray[n], *case))
    assert mine[0].any()


def test_rotation_fast_path_and_perspective_solve():
    assert augment.rotation_matrix(0.0, 224) is None and augment.rotation_matrix(360.0, 224) is None
    assert augment.record(224, angle=-720.0)[14] == 0
    start, end = [[0, 0], [39, 0], [39, 39], [0, 39]], [[4, 2], [36, 5], [33, 38], [1, 30]]
    c = augment.perspective_coeffs(start, end)
    for (sx, sy), (ex, ey) in zip(start, end):                    # output corner (end) -> input corner (start)
        den = c[6] * ex + c[7] * ey + 1
        assert abs((c[0] * ex + c[1] * ey + c[2]) / den - sx) < 1e-9 and abs((c[3] * ex + c[4] * ey + c[5]) / den - sy) < 1e-9


def test_frame_kernels_use_no_scratch():
    """The register budget of DESIGN.md 4.9.1, read from the built library's code objects as tests/test_codeobj_budget.py does."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import codeobj_report as cr
    if not os.path.exists(cr.LIB) or not os.path.exists(os.path.join(cr.LLVM, "llvm-readelf")):
        pytest.skip("needs the built library and llvm-readelf")
    rows = {r["name"]: r for r in cr.report()}
    for name in ("osfr::frames_augment_kernel", "osfr::frames_ingest_u8_kernel<1>", "osfr::frames_ingest_u8_kernel<3>"):
        assert rows[name]["private_segment_fixed_size"] == 0 and rows[name]["vgpr_spill_count"] == 0, name


def test_sampled_records_are_valid_and_seeded():
    p = augment.sample_params(400, 224, 7)
    assert np.array_equal(p, augment.sample_params(400, 224, np.random.default_rng(7)))
    flags = p[:, 14].astype(int)
    assert ((flags & 1) == 1).all() and (flags < 32).all()          # a uniform angle is never 0: every image rotates
    assert all(0.4 < ((flags & b) > 0).mean() < 0.6 for b in (2, 4, 8)) and 0.2 < (flags & 16 > 0).mean() < 0.4
    assert np.abs(p[:, 0]).max() <= 1.0 and p[:, 0].min() >= round(np.cos(np.radians(10.0)), 15)
    top, left, h, w = p[flags & 16 > 0][:, 15:19].T
    assert (top >= 0).all() and (left >= 0).all() and (top + h <= 224).all() and (left + w <= 224).all()
    assert h.min() >= int(224 * (0.8 / 1.1) ** 0.5) and w.min() >= int(224 * 0.72 ** 0.5)
