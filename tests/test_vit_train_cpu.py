"""CPU: surface of the auto-encoder's training step (no GPU needed): the C-ABI exports, the CPU-tensor refusal, and that the
trainable flag changes nothing for modules that do not set it."""
import pytest
import torch

from optistate_amd import _capi
from optistate_amd.transformer_model import Transformer_Autoencoder

SMALL = dict(img_size=32, depth=1, decoder_depth=1)


def test_training_calls_are_exported():
    assert {"os_vit_train_ws_floats", "os_vit_forward_train", "os_vit_backward"} <= set(_capi.EXPORTS)


def test_trainable_module_refuses_cpu_tensors_under_grad():
    m = Transformer_Autoencoder(decoder=True, trainable=True, **SMALL)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.rand(1, 1, 32, 32))
    with pytest.raises(ValueError):
        Transformer_Autoencoder(trainable=True, **SMALL)          # the loss is the decoder's


def test_untrainable_modules_are_unchanged():
    a, b = Transformer_Autoencoder(decoder=True, **SMALL), Transformer_Autoencoder(decoder=True, trainable=True, **SMALL)
    assert not a.trainable and list(a.state_dict()) == list(b.state_dict())
    a.load_state_dict(b.state_dict(), strict=True)
    assert not a.pos_embed.requires_grad and not a.decoder_pos_embed.requires_grad
    flat = torch.cat([p.detach().reshape(-1) for p in b._train_params()])       # the order of the two flat layouts
    assert torch.equal(flat, torch.cat([b._flat("cpu"), b._flat_decoder("cpu")]))
    offs = b._train_offsets()
    assert offs[0] == (0, 0) and (1, 0) in offs
