"""CPU: what VitTrainer refuses, and the decay groups it and its callers use (timm's add_weight_decay rule)."""
import pytest
import torch


def test_trainer_refuses_cpu_and_decoderless_models():
    from optistate_amd.train import VitTrainer
    from optistate_amd.transformer_model import Transformer_Autoencoder
    small = dict(img_size=32, depth=1, decoder_depth=1)
    with pytest.raises(RuntimeError):
        VitTrainer(Transformer_Autoencoder(decoder=True, **small))
    with pytest.raises(ValueError):
        VitTrainer(Transformer_Autoencoder(**small))


def test_decay_partition_on_the_reference_names():
    from optistate_amd.train import add_weight_decay, decay_partition
    from optistate_amd.transformer_model import Transformer_Autoencoder
    m = Transformer_Autoencoder(decoder=True)
    named = dict(m.named_parameters())
    decay, no_decay = decay_partition(named.items())
    matrices = {k for k, p in named.items() if k.endswith(".weight") and p.dim() > 1}
    assert "patch_embed.proj.weight" in matrices and len(matrices) == 1 + 4 * 6 + 2
    assert set(decay) == matrices | {"cls_token", "decoder_noise_token"}
    assert set(decay) | set(no_decay) == set(named) - {"pos_embed", "decoder_pos_embed"} and not set(decay) & set(no_decay)
    groups = add_weight_decay(m, 0.001)
    assert [g["weight_decay"] for g in groups] == [0.0, 0.001]
    assert [len(g["params"]) for g in groups] == [len(no_decay), len(decay)]
