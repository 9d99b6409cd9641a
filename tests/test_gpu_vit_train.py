"""GPU: training step of the ViT auto-encoder (os_vit_forward_train / os_vit_backward, Transformer_Autoencoder(decoder=True,
trainable=True)) against torch autograd on a float64 restatement of encoder + decoder + loss (the maths of
oracle/vit_oracle.py `encode` and test_gpu_vit_decoder.py `decode`, written with torch ops) on the CPU.

Measure, per parameter tensor: max|g - g64| / max|g64|; the same for the loss.  Bars: the restatement run in float32 on the CPU on
these very inputs lies, at its worst tensor, within 1.02e-6 of the float64 gradients (per case 1.02e-6 cls_token, 5.58e-7
patch_embed.proj.weight, 6.32e-7 and 5.69e-7 blocks.0.mlp.fc1.weight) and within 4.48e-8 of the loss (per case 7.16e-9, 4.48e-8,
1.12e-8, 2.16e-8); the three losses of the AdamW loop lie within 1.93e-7 (4.48e-8, 1.93e-7, 1.28e-7).  The bar is 4 x that,
rounded up to one digit (the HIP path sums its MFMA tiles and weight-gradient slices in another order, its erf is good to
1.5e-7): GRAD_TOL = 5e-6, LOSS_RTOL = 2e-7, LOOP_LOSS_RTOL = 8e-7.  Every compared float64 gradient has max|g64| > 0 (checked
when the seed was chosen, and asserted).
"""
import functools

import pytest
import torch

from test_gpu_vit_decoder import seeded_module

pytestmark = pytest.mark.gpu
F = torch.nn.functional

#        img  encoder (width, depth, heads)  decoder (width, depth, heads)  N
CASES = [(32, (128, 1, 4), (128, 1, 4), 1),       # 5 tokens: one key tile, one image
         (96, (128, 1, 4), (128, 2, 4), 3),       # 37 tokens: a ragged second key tile, 111 rows
         (64, (128, 1, 4), (256, 1, 8), 2),       # 17 tokens, the widths differ
         (224, (128, 3, 4), (128, 3, 4), 5)]      # the reference's model: 985 rows = 3.85 weight-gradient slices of 256
GRAD_TOL, LOSS_RTOL, LOOP_LOSS_RTOL = 5e-6, 2e-7, 8e-7


def restate(sd, imgs, heads, dec_heads, patch=16):
    """sd: the reference's state_dict keys -> tensors of one dtype; imgs [N][H][W] -> (loss, pred)."""
    def ln(x, pre):
        return F.layer_norm(x, x.shape[-1:], sd[pre + ".weight"], sd[pre + ".bias"], 1e-5)

    def blocks(x, pre, nh):
        i = 0
        while f"{pre}{i}.norm1.weight" in sd:
            p, (N, L, D) = f"{pre}{i}.", x.shape
            qkv = ln(x, p + "norm1") @ sd[p + "attn.qkv.weight"].T + sd[p + "attn.qkv.bias"]
            q, k, v = qkv.reshape(N, L, 3, nh, D // nh).permute(2, 0, 3, 1, 4)
            o = (torch.softmax(q @ k.transpose(-1, -2) * (D // nh) ** -0.5, -1) @ v).transpose(1, 2).reshape(N, L, D)
            x = x + o @ sd[p + "attn.proj.weight"].T + sd[p + "attn.proj.bias"]
            h = ln(x, p + "norm2") @ sd[p + "mlp.fc1.weight"].T + sd[p + "mlp.fc1.bias"]
            x = x + F.gelu(h) @ sd[p + "mlp.fc2.weight"].T + sd[p + "mlp.fc2.bias"]
            i += 1
        return x
    N, G = imgs.shape[0], imgs.shape[1] // patch
    target = imgs.reshape(N, G, patch, G, patch).permute(0, 1, 3, 2, 4).reshape(N, G * G, patch * patch)
    D = sd["cls_token"].shape[-1]
    tok = target @ sd["patch_embed.proj.weight"].reshape(D, -1).T + sd["patch_embed.proj.bias"] + sd["pos_embed"][:, 1:]
    x = blocks(torch.cat([(sd["cls_token"] + sd["pos_embed"][:, :1]).expand(N, -1, -1), tok], 1), "blocks.", heads)
    x = torch.sigmoid(ln(x, "norm")[:, :1]) @ sd["decoder_embed.weight"].T + sd["decoder_embed.bias"]
    x = torch.cat([x, sd["decoder_noise_token"].expand(N, G * G, -1)], 1) + sd["decoder_pos_embed"]
    x = blocks(x, "decoder_blocks.", dec_heads)
    pred = (ln(x, "decoder_norm") @ sd["decoder_pred.weight"].T + sd["decoder_pred.bias"])[:, 1:]
    return ((pred - target) ** 2).mean(), pred


def leaves(module, dtype):
    fixed = ("pos_embed", "decoder_pos_embed")
    return {k: v.detach().to(dtype).clone().requires_grad_(k not in fixed) for k, v in module.state_dict().items()}


def build(img, enc, dec, seed=21):
    return seeded_module(seed, img_size=img, embed_dim=enc[0], depth=enc[1], num_heads=enc[2], decoder_embed_dim=dec[0],
                         decoder_depth=dec[1], decoder_num_heads=dec[2], trainable=True)


@functools.lru_cache(maxsize=None)
def reference(img, enc, dec, N):
    """(module on the CPU, images, float64 loss, {name: float64 gradient}), computed once per case."""
    m = build(img, enc, dec)
    imgs = torch.rand(N, img, img)
    sd = leaves(m, torch.float64)
    loss, _ = restate(sd, imgs.double(), enc[2], dec[2])
    loss.backward()
    return m, imgs, loss.item(), {k: v.grad for k, v in sd.items() if v.requires_grad}


def rel(g, ref):
    return ((g.double().cpu() - ref).abs().max() / ref.abs().max()).item()


@pytest.mark.parametrize("img,enc,dec,N", CASES)
def test_gradients_match_float64_autograd(img, enc, dec, N):
    m, imgs, ref_loss, ref = reference(img, enc, dec, N)
    g = build(img, enc, dec).to("cuda")
    g.load_state_dict(m.state_dict())
    loss, pred = g(imgs.cuda().unsqueeze(1))
    loss.backward()
    lerr = abs(loss.item() - ref_loss) / ref_loss
    errs = {}
    for k, p in g.named_parameters():
        if p.requires_grad:
            assert ref[k].abs().max() > 0, k                        # nothing is compared against a zero gradient
            assert p.grad is not None and p.grad.shape == p.shape, k
            errs[k] = rel(p.grad, ref[k])
    worst = max(errs, key=errs.get)
    print(f"img {img}: loss rel {lerr:.2e}, worst gradient {worst} {errs[worst]:.2e}")
    assert set(errs) == set(ref)
    assert g.pos_embed.grad is None and g.decoder_pos_embed.grad is None and not pred.requires_grad
    assert lerr < LOSS_RTOL, lerr
    assert errs[worst] < GRAD_TOL, errs


def test_backward_is_bit_reproducible():
    from optistate_amd.engine import _ptr
    img, enc, dec, N = CASES[3]
    m, imgs, _, _ = reference(img, enc, dec, N)
    g = build(img, enc, dec).to("cuda")
    g.load_state_dict(m.state_dict())
    x = imgs.cuda()
    eng = g._engine(x)
    g._load_locked(eng, x.device)
    ws = torch.empty(eng.lib.os_vit_train_ws_floats(eng._h, N), device="cuda")
    loss, one = torch.empty((), device="cuda"), torch.ones((), device="cuda")
    eng._check(eng.lib.os_vit_forward_train(eng._h, N, _ptr(x), _ptr(ws), None, _ptr(loss), eng._stream()), "os_vit_forward_train")
    out = []
    for _ in range(2):
        ge, gd = torch.full_like(g._loaded[1], 7.0), torch.full_like(g._loaded[2], 7.0)     # overwritten, not accumulated into
        eng._check(eng.lib.os_vit_backward(eng._h, N, _ptr(x), _ptr(ws), _ptr(one), _ptr(ge), _ptr(gd), eng._stream()), "os_vit_backward")
        out.append((ge, gd))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert out[0][0].abs().max() < 7.0 and out[0][1].abs().max() < 7.0
    n0 = 128 * 256 + 2 * 128
    assert not out[0][0][n0:n0 + 197 * 128].any()                       # the position table's slot is written as zero


def test_module_surface():
    img, enc, dec, N = CASES[1]
    m, imgs, _, _ = reference(img, enc, dec, N)
    g = build(img, enc, dec).to("cuda")
    g.load_state_dict(m.state_dict())
    a, b = imgs.cuda().unsqueeze(1), torch.rand(N, 1, img, img, device="cuda")
    loss, pred = g(a)
    assert loss.requires_grad and loss.shape == () and pred.shape == (N, g.num_patches, 256)
    grads = []
    for x in (a, b):
        g.zero_grad()
        g(x)[0].backward()
        grads.append({k: p.grad.clone() for k, p in g.named_parameters() if p.requires_grad})
    g.zero_grad()
    (g(a)[0] + g(b)[0]).backward()                                      # two graphs alive at once
    for k, p in g.named_parameters():
        if p.requires_grad:
            assert p.grad.shape == p.shape
            s = (grads[0][k] + grads[1][k]).double().cpu()
            assert rel(p.grad, s) < GRAD_TOL, k
    from optistate_amd.transformer_model import Transformer_Autoencoder
    inf = Transformer_Autoencoder(img_size=img, embed_dim=enc[0], depth=enc[1], num_heads=enc[2], decoder_embed_dim=dec[0],
                                  decoder_depth=dec[1], decoder_num_heads=dec[2], decoder=True).to("cuda")
    inf.load_state_dict(m.state_dict())
    with torch.no_grad():
        l0, p0 = g(a)
    l1, p1 = inf(a)
    assert not l0.requires_grad and torch.equal(p0, p1) and torch.equal(l0, l1)


def test_three_adamw_steps_follow_the_float64_loop():
    img, enc, dec, N = CASES[1]
    m, imgs, _, _ = reference(img, enc, dec, N)
    g = build(img, enc, dec).to("cuda")
    g.load_state_dict(m.state_dict())
    sd = leaves(m, torch.float64)
    kw = dict(lr=4e-4, betas=(0.9, 0.95), weight_decay=0.001)
    opt = torch.optim.AdamW([p for p in g.parameters() if p.requires_grad], **kw)
    opt64 = torch.optim.AdamW([v for v in sd.values() if v.requires_grad], **kw)
    x = imgs.cuda().unsqueeze(1)
    for step in range(3):
        opt.zero_grad()
        loss, _ = g(x)
        loss.backward()
        opt.step()
        opt64.zero_grad()
        loss64, _ = restate(sd, imgs.double(), enc[2], dec[2])
        loss64.backward()
        opt64.step()
        err = abs(loss.item() - loss64.item()) / loss64.item()
        print(f"step {step}: loss {loss.item():.6f}, rel {err:.2e}")
        assert err < LOOP_LOSS_RTOL, (step, err)
