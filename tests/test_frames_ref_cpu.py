"""CPU: the numpy restatement of the frame ingest (tests/frames_ref.py) equals Pillow itself, pixel for pixel, on the geometries of
tests/test_gpu_frames.py -- what the reference's loaders feed the ViT (gru/gru_test.py:49-53)."""
import numpy as np
import pytest

import frames_ref

GEOMETRIES = [(37, 53, 3, 48), (480, 640, 3, 224), (64, 40, 1, 224), (224, 300, 3, 224), (224, 224, 1, 224), (1000, 31, 3, 32),
              (120, 160, 3, 224)]


@pytest.mark.parametrize("H,W,C,S", GEOMETRIES)
def test_restatement_equals_pillow(H, W, C, S):
    Image = pytest.importorskip("PIL.Image")
    frames = frames_ref.batch(H, W, C, seed=H + W)
    mine = frames_ref.ingest(frames, S)
    for n in range(frames.shape[0]):
        im = Image.fromarray(frames[n] if C == 3 else frames[n, :, :, 0])
        pil = np.asarray(im.convert("RGB").resize((S, S), Image.BILINEAR).convert("L"), np.float32) / np.float32(255)
        assert int((pil != mine[n]).sum()) == 0
