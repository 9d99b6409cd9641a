"""GPU: frame augmentation on the HIP path (os_frames_augment, os_frames_ingest_u8) against the numpy restatement of Pillow's
transforms (tests/augment_ref.py, pinned to Pillow by tests/test_augment_ref_cpu.py).  Index maps, integer arithmetic and a
correctly rounded division: the bar is bit equality."""
import functools

import numpy as np
import pytest
import torch

import augment_ref
import frames_ref
from optistate_amd import augment

pytestmark = pytest.mark.gpu

SIZES = (224, 40)          # the real plane (LDS pitch, 16-byte staging); not a multiple of a wave or of 16, ragged rows
NAMES = sorted(augment_ref.cases(40))


@functools.lru_cache(maxsize=None)
def gray(S):
    """Three S x S images: seeded random bytes, all 255, a checkerboard."""
    return frames_ref.batch(S, S, 1, seed=S)[..., 0]


@pytest.fixture(scope="module")
def eng():
    from optistate_amd import Engine
    return Engine(0)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("S", SIZES)
def test_augment_is_bit_equal_to_the_restatement(eng, S, name):
    params = np.stack([augment.record(S, *augment_ref.cases(S)[name])] * 3)
    out = eng.augment_frames(torch.from_numpy(gray(S)).cuda(), params)
    assert out.shape == (3, S, S) and out.dtype == torch.float32
    assert torch.equal(out.cpu(), torch.from_numpy(augment_ref.augment(gray(S), params)))
    if name == "none":
        assert torch.equal(out.cpu(), torch.from_numpy(gray(S)).float() / 255)


@pytest.mark.parametrize("S", SIZES)
def test_images_of_one_launch_take_their_own_records(eng, S):
    c = augment_ref.cases(S)
    params = np.stack([augment.record(S, *c[k]) for k in ("all", "none", "crop-smallest")])
    ref = torch.from_numpy(augment_ref.augment(gray(S), params))
    dev, pdev = torch.from_numpy(gray(S)).cuda(), torch.from_numpy(params).cuda()
    out = eng.augment_frames(dev, pdev)
    assert torch.equal(out.cpu(), ref)
    assert torch.equal(eng.augment_frames(dev, pdev), out)         # the same batch again: the same bits
    flat = torch.zeros(3 * S * S + 1, dtype=torch.uint8, device="cuda")
    flat[1:] = dev.reshape(-1)
    assert torch.equal(eng.augment_frames(flat[1:].view(3, S, S), pdev), out)      # images that do not start at a multiple of 16


def test_sampled_batch_and_size_limit(eng):
    S, N = 40, 64
    g = np.random.default_rng(3).integers(0, 256, (N, S, S), dtype=np.uint8)
    params = augment.sample_params(N, S, 11)
    assert torch.equal(eng.augment_frames(torch.from_numpy(g).cuda(), params).cpu(), torch.from_numpy(augment_ref.augment(g, params)))
    with pytest.raises(RuntimeError, match="S <= 256"):
        eng.augment_frames(torch.zeros((1, 272, 272), dtype=torch.uint8, device="cuda"), np.zeros((1, 20)))


def test_byte_ingest_and_preprocess_with_augmentation(eng):
    from optistate_amd.transformer_model import Transformer_Autoencoder
    frames = frames_ref.batch(37, 53, 3, seed=90)
    dev = torch.from_numpy(frames).cuda()
    u8 = eng.ingest_frames_u8(dev, 48)
    # divided on the host: the device's division of a tensor by a scalar multiplies by 1 / 255, which is not the correctly rounded quotient
    assert u8.dtype == torch.uint8 and torch.equal(u8.cpu().float() / 255, eng.ingest_frames(dev, 48).cpu())
    m = Transformer_Autoencoder()
    params = torch.from_numpy(augment.sample_params(3, m.img_size, 5)).cuda()
    pre = m.preprocess(dev, augment=params)
    assert pre.shape == (3, 1, m.img_size, m.img_size)
    assert torch.equal(pre[:, 0], eng.augment_frames(eng.ingest_frames_u8(dev, m.img_size), params))
    assert torch.equal(m.preprocess(dev)[:, 0], eng.ingest_frames(dev, m.img_size))
