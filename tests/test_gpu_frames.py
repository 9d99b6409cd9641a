"""GPU: frame ingest on the HIP path (os_frames_ingest / os_vit_encode_frames) against the numpy restatement of Pillow's transform
(tests/frames_ref.py, pinned to Pillow by tests/test_frames_ref_cpu.py).  The arithmetic is integer and the division correctly
rounded: the bar is bit equality."""
import functools

import numpy as np
import pytest
import torch

import frames_ref

pytestmark = pytest.mark.gpu

GEOMETRIES = [(37, 53, 3, 48),        # odd row bytes, ragged tiles on both axes
              (480, 640, 3, 224),     # the real shape
              (64, 40, 1, 224),       # up-scaling, one channel
              (224, 300, 3, 224),     # vertical pass skipped
              (224, 224, 1, 224),     # both passes skipped
              (1000, 31, 3, 32)]      # ratio 31.25 (64 taps) down, up-scaling across


@functools.lru_cache(maxsize=None)
def case(H, W, C, S):
    frames = frames_ref.batch(H, W, C, seed=H + W)
    return frames, torch.from_numpy(frames_ref.ingest(frames, S))


@pytest.fixture(scope="module")
def eng():
    from optistate_amd import Engine
    return Engine(0)


@pytest.mark.parametrize("H,W,C,S", GEOMETRIES)
def test_ingest_is_bit_equal_to_the_restatement(eng, H, W, C, S):
    frames, ref = case(H, W, C, S)
    dev = torch.from_numpy(frames).cuda()
    out = eng.ingest_frames(dev, S)
    assert out.shape == (3, S, S) and out.dtype == torch.float32
    assert torch.equal(out.cpu(), ref)
    assert bool((out[1] == 1.0).all())                         # all 255 in -> exactly 1.0 out
    assert torch.equal(eng.ingest_frames(dev, S), out)         # the plan-cache hit
    if C == 1:                                                 # (N,H,W) is (N,H,W,1); a numpy array is copied over
        assert torch.equal(eng.ingest_frames(frames[..., 0], S).cpu(), ref)


def test_geometry_switch_replaces_and_rebuilds_plans(eng):
    first = GEOMETRIES[0]
    for H, W, C, S in [first] + GEOMETRIES[1:] + [first]:      # five other geometries in between: more than the cache holds
        frames, ref = case(H, W, C, S)
        assert torch.equal(eng.ingest_frames(frames, S).cpu(), ref)


def test_fused_call_and_preprocess_are_bit_identical():
    from optistate_amd import pipeline
    from optistate_amd.transformer_model import Transformer_Autoencoder
    torch.manual_seed(0)
    m = Transformer_Autoencoder().to("cuda")
    frames = np.random.default_rng(5).integers(0, 256, (5, 120, 160, 3), dtype=np.uint8)
    dev = torch.from_numpy(frames).cuda()
    pre = m.preprocess(dev)
    assert pre.shape == (5, 1, 224, 224)
    assert torch.equal(pre.cpu()[:, 0], torch.from_numpy(frames_ref.ingest(frames, 224)))
    lat = m.encode_frames(dev)
    assert lat.shape == (5, 1, 128)
    assert torch.equal(lat, m.forward_encoder(pre))
    assert torch.equal(pipeline.latents_from_frames(m, dev, chunk=5), lat[:, 0])


def test_chunked_latents_equal_the_whole_batch():
    """The frame loop in chunks gives every image the bits of the whole batch: the ingest is exact, and the encoder's result for an
    image does not depend on the rows its tokens occupy in the token matrix (chunks of 2 put images 2-4 at other rows)."""
    from optistate_amd import pipeline
    from optistate_amd.transformer_model import Transformer_Autoencoder
    torch.manual_seed(0)
    m = Transformer_Autoencoder().to("cuda")
    dev = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (5, 120, 160, 3), dtype=np.uint8)).cuda()
    whole, parts = m.encode_frames(dev)[:, 0], pipeline.latents_from_frames(m, dev, chunk=2)
    print("max abs difference per image:", (parts - whole).abs().amax(dim=1).tolist())
    assert torch.equal(parts, whole)


def test_errors_leave_the_next_call_exact(eng):
    frames, ref = case(*GEOMETRIES[0])
    dev = torch.from_numpy(frames).cuda()
    with pytest.raises(TypeError):
        eng.ingest_frames(dev.float(), 48)
    with pytest.raises(ValueError):
        eng.ingest_frames(dev[..., :2].contiguous(), 48)       # C = 2
    with pytest.raises(RuntimeError, match=r"\(-2\)"):          # the C-ABI's own argument check
        eng._check(eng.lib.os_frames_ingest(eng._h, 3, dev.data_ptr(), 37, 53, 2, 48, dev.data_ptr(), None), "os_frames_ingest")
    with pytest.raises(RuntimeError, match="ratio up to 32"):   # 70000 rows -> 16: far outside what a tile's window can hold
        eng.ingest_frames(torch.zeros((1, 70000, 8, 1), dtype=torch.uint8, device="cuda"), 16)
    assert torch.equal(eng.ingest_frames(dev, 48).cpu(), ref)
