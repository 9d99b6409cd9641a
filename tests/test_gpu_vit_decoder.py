"""GPU: decoder half of the ViT auto-encoder (os_vit_decode / os_vit_recon_loss, Transformer_Autoencoder(decoder=True)) against
a float64 restatement of the reference's forward_decoder + forward_loss (transformer/transformer_model.py:137-169, timm-0.3.2
blocks as in oracle/vit_oracle.py).

Bars: the same restatement run in float32 on the CPU on these very inputs lies within 2.2e-6 of the float64 pred (l-inf; per
case 2.1e-6, 1.2e-6, 1.7e-6, 2.2e-6) and within 8.8e-8 of its loss (relative; per case 5.7e-8, 1.0e-8, 3.9e-8, 8.8e-8).  The bar
is 4 x that, rounded up to one digit (the MFMA tiles sum in another order, gelu_erf's erf is good to 1.5e-7): PRED_TOL = 9e-6,
LOSS_RTOL = 4e-7.  The module test runs the HIP encoder in front, whose own bar on the latent is 2e-5.  At that test's inputs the
float32 restatement is 1.7e-6 (pred) and 2.9e-8 (loss) away, and moving every latent component by +-2e-5 moves the float64 pred
by 1.1e-6 and the loss by 2.2e-8: 4 x the sums, rounded up, are FWD_TOL = 2e-5 and FWD_LOSS_RTOL = 3e-7."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy.special import erf

pytestmark = pytest.mark.gpu

PRED_TOL, LOSS_RTOL, FWD_TOL, FWD_LOSS_RTOL = 9e-6, 4e-7, 2e-5, 3e-7


def decode(latent, images, sd, heads, patch=16, dt=np.float64):
    """latent [N][De], images [N][H][W], sd with the reference's decoder_* keys -> (pred [N][L-1][P*P], loss), all in `dt`."""
    g = lambda k: np.asarray(sd[k], dtype=dt)

    def ln(x, w, b):
        mu = x.mean(-1, keepdims=True)
        return (x - mu) / np.sqrt(((x - mu) ** 2).mean(-1, keepdims=True) + 1e-5) * w + b
    x = np.asarray(latent, dtype=dt)[:, None, :] @ g("decoder_embed.weight").T + g("decoder_embed.bias")
    N, D = x.shape[0], x.shape[-1]
    pos = g("decoder_pos_embed").reshape(-1, D)
    x = np.concatenate([x, np.broadcast_to(g("decoder_noise_token").reshape(1, 1, D), (N, len(pos) - 1, D))], axis=1) + pos
    hd = D // heads
    for i in range(1 + max(int(k.split(".")[1]) for k in sd if k.startswith("decoder_blocks."))):
        p = f"decoder_blocks.{i}."
        qkv = ln(x, g(p + "norm1.weight"), g(p + "norm1.bias")) @ g(p + "attn.qkv.weight").T + g(p + "attn.qkv.bias")
        q, k, v = qkv.reshape(N, -1, 3, heads, hd).transpose(2, 0, 3, 1, 4)
        att = (q @ k.transpose(0, 1, 3, 2)) * hd ** -0.5
        att = np.exp(att - att.max(-1, keepdims=True))
        o = ((att / att.sum(-1, keepdims=True)) @ v).transpose(0, 2, 1, 3).reshape(N, -1, D)
        x = x + o @ g(p + "attn.proj.weight").T + g(p + "attn.proj.bias")
        h = ln(x, g(p + "norm2.weight"), g(p + "norm2.bias")) @ g(p + "mlp.fc1.weight").T + g(p + "mlp.fc1.bias")
        x = x + (0.5 * h * (1.0 + erf(h * 0.5 ** 0.5))) @ g(p + "mlp.fc2.weight").T + g(p + "mlp.fc2.bias")
    pred = (ln(x, g("decoder_norm.weight"), g("decoder_norm.bias")) @ g("decoder_pred.weight").T + g("decoder_pred.bias"))[:, 1:]
    G = images.shape[1] // patch
    target = np.asarray(images, dtype=dt).reshape(N, G, patch, G, patch).transpose(0, 1, 3, 2, 4).reshape(N, G * G, patch * patch)
    return pred, ((pred - target) ** 2).mean()


def seeded_module(seed, **kw):
    """Seeded weights with every 1-d parameter and the noise token moved by 0.1 randn, so biases and LayerNorm affines count."""
    from optistate_amd.transformer_model import Transformer_Autoencoder
    torch.manual_seed(seed)
    m = Transformer_Autoencoder(decoder=True, **kw)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.dim() == 1 or n == "decoder_noise_token":
                p.add_(0.1 * torch.randn_like(p))
    return m


CASES = [(224, 128, 128, 3, 4, 3),     # 197 tokens, MFMA attention, 588 patch rows: a partial last tile in dec_pred_kernel
         (64, 128, 128, 1, 2, 2),      # 17 tokens, head dimension 64
         (96, 256, 128, 2, 4, 5),      # latent width != decoder width
         (64, 128, 256, 2, 4, 1)]      # decoder width 256: the unfused block tail, dec_pred_kernel<256>


def case_inputs(img, embed_dim, dec_dim, dec_depth, dec_heads, N):
    m = seeded_module(11, img_size=img, embed_dim=embed_dim, depth=1, decoder_embed_dim=dec_dim, decoder_depth=dec_depth,
                      decoder_num_heads=dec_heads)
    return m, torch.rand(N, embed_dim), torch.rand(N, img, img)


@pytest.mark.parametrize("img,embed_dim,dec_dim,dec_depth,dec_heads,N", CASES)
def test_decode_matches_the_float64_restatement(img, embed_dim, dec_dim, dec_depth, dec_heads, N):
    from optistate_amd import Engine
    from optistate_amd.engine import _ptr
    m, latent, images = case_inputs(img, embed_dim, dec_dim, dec_depth, dec_heads, N)
    sd = {k: v.numpy() for k, v in m.state_dict().items()}
    ref_pred, ref_loss = decode(latent.numpy(), images.numpy(), sd, dec_heads)
    e = Engine(0)
    flat, d = m._flat_decoder(torch.device("cuda:0")), m._decoder_dims()
    assert flat.numel() == e.lib.os_vit_decoder_param_count(C.byref(d), embed_dim)
    e._check(e.lib.os_vit_load_decoder(e._h, C.byref(d), embed_dim, _ptr(flat)), "os_vit_load_decoder")     # no os_vit_load
    lat, imgs = latent.cuda(), images.cuda()
    pred = torch.empty((N, m.num_patches, 256), device="cuda")
    recon = torch.empty((N, 1, img, img), device="cuda")
    loss = torch.empty((2,), device="cuda")
    for i in range(2):
        e._check(e.lib.os_vit_decode(e._h, N, _ptr(lat), _ptr(imgs), _ptr(pred), _ptr(recon), _ptr(loss[i:]), e._stream()), "os_vit_decode")
    torch.cuda.synchronize()
    err = np.abs(pred.cpu().numpy() - ref_pred).max()
    rel = abs(loss[0].item() - ref_loss) / ref_loss
    print(f"pred linf {err:.2e}, loss rel {rel:.2e}")
    assert err < PRED_TOL, err
    assert torch.equal(recon, m.unpatchify(pred))
    assert rel < LOSS_RTOL, rel
    assert loss[0].item() == loss[1].item()                              # fixed summation order: the same bits
    only = torch.empty((), device="cuda")
    e._check(e.lib.os_vit_recon_loss(e._h, N, _ptr(imgs), _ptr(pred), _ptr(only), e._stream()), "os_vit_recon_loss")
    assert abs(only.item() - ref_loss) / ref_loss < LOSS_RTOL


def test_module_surface_at_the_reference_shape():
    from optistate_amd.transformer_model import Transformer_Autoencoder
    from oracle import vit_oracle
    src = seeded_module(12)
    m = Transformer_Autoencoder(decoder=True)
    m.load_state_dict({k: v.clone() for k, v in src.state_dict().items()}, strict=True)
    m = m.to("cuda")
    x = torch.rand(2, 1, 224, 224)
    sd = {k: v.numpy() for k, v in src.state_dict().items()}
    ref_pred, ref_loss = decode(vit_oracle.encode(x[:, 0].numpy(), sd), x[:, 0].numpy(), sd, 4)
    loss, pred = m(x.cuda())
    assert loss.shape == () and pred.shape == (2, 196, 256)
    err = np.abs(pred.cpu().numpy() - ref_pred).max()
    print(f"forward: pred linf {err:.2e}, loss rel {abs(loss.item() - ref_loss) / ref_loss:.2e}")
    assert err < FWD_TOL, err
    assert abs(loss.item() - ref_loss) / ref_loss < FWD_LOSS_RTOL
    assert torch.equal(m.unpatchify(m.patchify(x)), x)
    assert abs(m.forward_loss(x.cuda(), pred).item() - loss.item()) <= 2e-7 * loss.item()
    assert torch.equal(m.reconstruct(x.cuda()), m.unpatchify(pred))
    assert torch.equal(m.forward_decoder(m.forward_encoder(x.cuda())), pred)
