"""GPU: the resident-weight trainer of the ViT auto-encoder (optistate_amd.train.VitTrainer, os_vit_adamw_step).

Measure of the kernel test, per parameter tensor after three steps: max|w - w64| / max|w64| against torch.optim.AdamW in float64 on
the CPU with timm's two decay groups.  It runs at weight_decay = 0.1, not the reference's 1e-3: three steps then move a decayed
tensor by 3 lr wd = 1.2e-4 of itself through the decay alone (1.2e-6 at 1e-3, under any honest bar), so a tensor with the wrong
decay flag misses the bar 60-fold (the Adam term moves the weights by 2e-2).  Bar: torch.optim.AdamW in float32 on the CPU
(foreach=False) on these very weights and gradients at that setting lies, at its worst tensor, within 2.81e-7 of float64 (per case
2.44e-7 blocks.0.attn.proj.weight, 2.81e-7 decoder_blocks.0.mlp.fc1.weight, 2.60e-7 blocks.2.attn.proj.weight); 4 x that, rounded
up to one digit: ADAMW_TOL = 2e-6.
Loop: with the grouped optimiser the float32 restatement's three losses lie within 2.37e-7 of the float64 loop's (4.48e-8, 2.37e-7,
1.27e-7; with every parameter decayed, as test_gpu_vit_train runs it, 1.93e-7).  4 x 2.37e-7 = 9.5e-7 no longer rounds up to that
file's LOOP_LOSS_RTOL = 8e-7, so this loop's bar is LOOP_RTOL = 1e-6.
"""
import functools

import pytest
import torch

from test_gpu_vit_decoder import seeded_module
from test_gpu_vit_train import CASES as TRAIN_CASES, leaves, reference, restate

pytestmark = pytest.mark.gpu

#        img  encoder (width, depth, heads)  decoder (width, depth, heads)  N
CASES = [(32, (128, 1, 4), (128, 1, 4), 1),       # 5 tokens, the smallest tables
         (64, (128, 1, 4), (256, 1, 8), 2),       # K = 256 tiles, decoder_embed 256 x 128 unpacked
         (224, (128, 3, 4), (128, 3, 4), 2)]      # the reference's matrices and depths: every kind of work-table entry
HYPER = dict(lr=4e-4, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-3)
KERNEL_HYPER = dict(HYPER, weight_decay=0.1)      # three steps of decay = 1.2e-4 of a weight: a wrong decay flag is 60 x the bar
ADAMW_TOL, LOOP_RTOL = 2e-6, 1e-6
FIXED = ("pos_embed", "decoder_pos_embed")


def build(img, enc, dec, seed=33, **kw):
    return seeded_module(seed, img_size=img, embed_dim=enc[0], depth=enc[1], num_heads=enc[2], decoder_embed_dim=dec[0],
                         decoder_depth=dec[1], decoder_num_heads=dec[2], **kw)


def grouped_adamw(named, hyper=HYPER):
    from optistate_amd.train import decay_partition
    decay, no_decay = decay_partition(named.items())
    kw = {k: v for k, v in hyper.items() if k != "weight_decay"}
    return torch.optim.AdamW([{"params": [named[k] for k in no_decay], "weight_decay": 0.0},
                              {"params": [named[k] for k in decay], "weight_decay": hyper["weight_decay"]}], foreach=False, **kw)


def flat_grads(m, t):
    """Seeded gradient vectors (encoder, decoder) of step t, the position tables' slots included."""
    n = [0, 0]
    for p, (which, _) in zip(m._train_params(), m._train_offsets()):
        n[which] += p.numel()
    gen = torch.Generator().manual_seed(1000 + t)
    return [1e-3 * torch.randn(k, generator=gen) for k in n]


def adamw_cpu(m, dtype):
    """{name: weights after three grouped AdamW steps in dtype on the CPU}, fed the float32 gradients of flat_grads."""
    named = {k: p.detach().to(dtype).clone().requires_grad_(p.requires_grad) for k, p in m.named_parameters()}
    by_param = {id(p): k for k, p in m.named_parameters()}
    opt = grouped_adamw(named, KERNEL_HYPER)
    for t in range(1, 4):
        g = flat_grads(m, t)
        for p, (which, off) in zip(m._train_params(), m._train_offsets()):
            if p.requires_grad:
                named[by_param[id(p)]].grad = g[which][off:off + p.numel()].view_as(p).to(dtype)
        opt.step()
    return {k: v.detach() for k, v in named.items()}


def fwd_bwd(module, x):
    """(loss, encoder gradients, decoder gradients) of one os_vit_forward_train + os_vit_backward on the module's loaded weights."""
    from optistate_amd.engine import _ptr
    eng = module._engine(x)
    module._load_locked(eng, x.device)
    ws = torch.empty(eng.lib.os_vit_train_ws_floats(eng._h, x.shape[0]), device="cuda")
    loss, one = torch.empty((), device="cuda"), torch.ones((), device="cuda")
    ge, gd = torch.empty_like(module._loaded[1]), torch.empty_like(module._loaded[2])
    eng._check(eng.lib.os_vit_forward_train(eng._h, x.shape[0], _ptr(x), _ptr(ws), None, _ptr(loss), eng._stream()), "os_vit_forward_train")
    eng._check(eng.lib.os_vit_backward(eng._h, x.shape[0], _ptr(x), _ptr(ws), _ptr(one), _ptr(ge), _ptr(gd), eng._stream()), "os_vit_backward")
    return loss, ge, gd


def adamw_step(tr, t, w=None):
    from optistate_amd.engine import _ptr
    e, w = tr.eng, tr.w if w is None else w
    return e.lib.os_vit_adamw_step(e._h, _ptr(w[0]), _ptr(w[1]), _ptr(tr.g[0]), _ptr(tr.g[1]), _ptr(tr.m[0]), _ptr(tr.v[0]), _ptr(tr.m[1]),
                                   _ptr(tr.v[1]), tr.lr, tr.betas[0], tr.betas[1], tr.eps, tr.weight_decay, t, e._stream())


@functools.lru_cache(maxsize=None)
def stepped(img, enc, dec, N):
    """Three os_vit_adamw_step calls on seeded gradients, then -- before any other module takes the context -- one inference
    forward and one forward + backward on the packs that the kernel left behind."""
    from optistate_amd.train import VitTrainer
    cpu = build(img, enc, dec)
    model = build(img, enc, dec).to("cuda")
    tr = VitTrainer(model, **KERNEL_HYPER)
    loaded = model._loaded
    fixed = {k: getattr(model, k).detach().clone() for k in FIXED}
    for t in range(1, 4):
        for dst, src in zip(tr.g, flat_grads(cpu, t)):
            dst.copy_(src)
        assert adamw_step(tr, t) == 0
    x = torch.rand(N, img, img, generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        loss, pred = model(x.unsqueeze(1))
    fb = fwd_bwd(model, x)
    assert model._loaded is loaded                                       # no reload since the trainer's: these ran on the kernel's packs
    return dict(cpu=cpu, model=model, tr=tr, fixed=fixed, x=x, loss=loss, pred=pred, fb=fb)


@pytest.mark.parametrize("img,enc,dec,N", CASES)
def test_kernel_follows_float64_adamw(img, enc, dec, N):
    s = stepped(img, enc, dec, N)
    ref = adamw_cpu(s["cpu"], torch.float64)
    errs = {k: ((p.detach().double().cpu() - ref[k]).abs().max() / ref[k].abs().max()).item() for k, p in s["model"].named_parameters()}
    worst = max(errs, key=errs.get)
    print(f"img {img}: worst tensor {worst} {errs[worst]:.2e}")
    assert errs[worst] < ADAMW_TOL, errs
    for (p, (which, off)) in zip(s["model"]._train_params(), s["model"]._train_offsets()):
        if not p.requires_grad:                                          # the position tables: bits kept, no optimiser state
            sl = slice(off, off + p.numel())
            assert not s["tr"].m[which][sl].any() and not s["tr"].v[which][sl].any()
    assert all(torch.equal(getattr(s["model"], k), v) for k, v in s["fixed"].items())


@pytest.mark.parametrize("img,enc,dec,N", CASES)
def test_packs_are_bit_exact(img, enc, dec, N):
    s = stepped(img, enc, dec, N)
    sd = s["model"].state_dict()
    fresh = build(img, enc, dec, seed=1).to("cuda")                      # os_vit_load: vit_pack_w_kernel
    fresh.load_state_dict(sd)
    with torch.no_grad():
        loss, pred = fresh(s["x"].unsqueeze(1))
    assert torch.equal(loss, s["loss"]) and torch.equal(pred, s["pred"])             # a stale or wrong forward pack
    fresh = build(img, enc, dec, seed=1, trainable=True).to("cuda")      # no step since its load: vit_pack_wt_kernel
    fresh.load_state_dict(sd)
    loss, ge, gd = fwd_bwd(fresh, s["x"])
    assert torch.equal(loss, s["fb"][0]) and torch.equal(ge, s["fb"][1]) and torch.equal(gd, s["fb"][2])     # a wrong transposed pack


def test_loop_follows_the_float64_loop_and_sees_torch_writes():
    from optistate_amd.train import VitTrainer
    img, enc, dec, N = TRAIN_CASES[1]
    m, imgs, _, _ = reference(img, enc, dec, N)
    initial = {k: v.clone() for k, v in m.state_dict().items()}
    g = seeded_module(1, img_size=img, embed_dim=enc[0], depth=enc[1], num_heads=enc[2], decoder_embed_dim=dec[0],
                      decoder_depth=dec[1], decoder_num_heads=dec[2]).to("cuda")
    g.load_state_dict(initial)
    tr = VitTrainer(g, **HYPER)
    sd = leaves(m, torch.float64)
    opt64 = grouped_adamw({k: v for k, v in sd.items()})
    x, losses = imgs.cuda().unsqueeze(1), []
    for step in range(3):
        losses.append(tr.step(x).clone())
        opt64.zero_grad()
        loss64, _ = restate(sd, imgs.double(), enc[2], dec[2])
        loss64.backward()
        opt64.step()
        err = abs(losses[-1].item() - loss64.item()) / loss64.item()
        print(f"step {step}: loss {losses[-1].item():.6f}, rel {err:.2e}")
        assert err < LOOP_RTOL, (step, err)
    g.load_state_dict(initial)                                           # a write through torch: picked up and packed again
    assert torch.equal(tr.step(x), losses[0])
    for k, p in g.named_parameters():
        p.data.copy_(initial[k].cuda())                                  # behind the version counters: the caller says so
    tr.invalidate()
    assert torch.equal(tr.step(x), losses[0])


def test_determinism_and_errors():
    from optistate_amd.train import VitTrainer
    img, enc, dec, N = CASES[0]
    x = torch.rand(N, 1, img, img, generator=torch.Generator().manual_seed(5)).cuda()
    flats = []
    for _ in range(2):
        tr = VitTrainer(build(img, enc, dec).to("cuda"), **HYPER)
        tr.step(x), tr.step(x)
        flats.append(tr._w.clone())
    assert torch.equal(flats[0], flats[1])
    tr.model._load_locked(tr.eng, x.device)
    assert adamw_step(tr, 3, w=(tr.w[0].clone(), tr.w[1])) == -5         # not the loaded vector
    assert adamw_step(tr, 0) == -2
    assert torch.equal(tr._w, flats[1])
    tr.model.cls_token.data = tr.model.cls_token.data.clone()           # rebound: the adoption ends, the step says -5
    with pytest.raises(RuntimeError):
        tr.step(x)
