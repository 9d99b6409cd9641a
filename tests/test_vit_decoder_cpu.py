"""CPU: the weight container of Transformer_Autoencoder(decoder=True) -- the reference's state_dict names and shapes
(transformer/transformer_model.py:20-47), its fixed decoder position table, and the C-ABI's flat decoder length."""
import ctypes as C

import torch

from conftest import load_golden

BLOCK = {"norm1.weight": (128,), "norm1.bias": (128,), "attn.qkv.weight": (384, 128), "attn.qkv.bias": (384,),
         "attn.proj.weight": (128, 128), "attn.proj.bias": (128,), "norm2.weight": (128,), "norm2.bias": (128,),
         "mlp.fc1.weight": (512, 128), "mlp.fc1.bias": (512,), "mlp.fc2.weight": (128, 512), "mlp.fc2.bias": (128,)}
REFERENCE = {"patch_embed.proj.weight": (128, 1, 16, 16), "patch_embed.proj.bias": (128,), "cls_token": (1, 1, 128),
             "pos_embed": (1, 197, 128), "norm.weight": (128,), "norm.bias": (128,),
             "decoder_embed.weight": (128, 128), "decoder_embed.bias": (128,), "decoder_noise_token": (1, 1, 128),
             "decoder_pos_embed": (1, 197, 128), "decoder_norm.weight": (128,), "decoder_norm.bias": (128,),
             "decoder_pred.weight": (256, 128), "decoder_pred.bias": (256,),
             **{f"{pre}.{i}.{k}": v for pre in ("blocks", "decoder_blocks") for i in range(3) for k, v in BLOCK.items()}}


def test_decoder_state_dict_is_the_reference_key_set():
    from optistate_amd.transformer_model import Transformer_Autoencoder
    m = Transformer_Autoencoder(decoder=True)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == REFERENCE
    assert not m.decoder_pos_embed.requires_grad
    # G10: the reference's own transformer/pos_embed.py output -- the decoder's table is the same function at the same size
    assert torch.equal(m.decoder_pos_embed[0], torch.from_numpy(load_golden("vit_g10_pos_embed.npz")["enc_128_14"]).float())


def test_decoder_param_count_equals_the_flat_length():
    from optistate_amd import _capi
    from optistate_amd.transformer_model import Transformer_Autoencoder
    lib = _capi.load()
    for kw in ({}, {"img_size": 96, "embed_dim": 256, "decoder_depth": 2}, {"img_size": 64, "decoder_embed_dim": 256, "decoder_depth": 1}):
        m = Transformer_Autoencoder(decoder=True, **kw)
        assert lib.os_vit_decoder_param_count(C.byref(m._decoder_dims()), m.embed_dim) == m._flat_decoder("cpu").numel()
