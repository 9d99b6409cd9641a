"""GRU hidden sizes 160 .. 256 (weight-streaming kernels, csrc/gru_stream_kernels.hip) against torch's own GRU in float64 on the
CPU: inference, training forward + backward, one trainer step."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def reference(sd, dims, x, y=None):
    """torch.nn.GRU + Linear + sigmoid in float64 (the checker, not the product); with y also the reference's criterion and its
    gradients (gru/gru_train.py:232-249)."""
    I, H, L, C = dims
    gru = torch.nn.GRU(I, H, L, batch_first=True).double()
    fc = torch.nn.Linear(H, C).double()
    gru.load_state_dict({k[4:]: v.double() for k, v in sd.items() if k.startswith("gru.")})
    fc.load_state_dict({k[3:]: v.double() for k, v in sd.items() if k.startswith("fc.")})
    xx = x.double().requires_grad_(y is not None)
    o, hn = gru(xx)
    out = torch.sigmoid(fc(o[:, -1, :]))
    if y is None:
        return out.detach(), hn.detach()
    tgt = torch.cat([y.double(), (out[:, :C // 2].detach() - y.double()).abs()], dim=1)
    loss = torch.nn.functional.mse_loss(out, tgt)
    loss.backward()
    grads = {f"gru.{k}": p.grad for k, p in gru.named_parameters()}
    grads.update({f"fc.{k}": p.grad for k, p in fc.named_parameters()})
    return out.detach(), loss.item(), grads, xx.grad


@pytest.mark.parametrize("I,H,L,C,B,T", [(61, 160, 1, 6, 33, 3),        # odd chunk count, odd K, one full tile + 1 row
                                         (60, 256, 1, 24, 1, 1),        # B = 1, T = 1
                                         (188, 256, 2, 24, 70, 4),      # second layer K = H = 256, ragged tile
                                         (40, 192, 2, 24, 130, 2),
                                         (60, 224, 3, 24, 64, 5),       # whole tiles, three layers
                                         (8, 160, 1, 6, 16400, 2)])     # 64-row tiles (a workgroup per CU and more), ragged
def test_inference_matches_float64(I, H, L, C, B, T):
    from optistate_amd import RNN
    torch.manual_seed(3)
    m = RNN(I, H, L, C, torch.device("cuda")).to("cuda")
    x = torch.rand(B, T, I)
    ref_out, ref_hn = reference({k: v.detach().cpu() for k, v in m.state_dict().items()}, (I, H, L, C), x)
    with torch.no_grad():
        out = m(x.cuda())
        eng = m._engine
        assert eng.kernel_name("gru_layer").startswith("gru_stream_layer_kernel"), eng.kernel_name("gru_layer")
        out2, hl = eng.gru_forward(x.cuda(), want_h_last=True)
    err, err_h = (out.cpu().double() - ref_out).abs().max().item(), (hl.cpu().double() - ref_hn).abs().max().item()
    print(f"max |out - ref| {err:.3e}, max |h_last - ref| {err_h:.3e}")
    assert err < 1e-5 and err_h < 1e-5
    assert torch.equal(out, out2)


@pytest.mark.parametrize("dims,B,T", [((61, 160, 2, 6), 33, 3), ((188, 256, 2, 24), 70, 4),
                                      ((60, 256, 1, 24), 64, 1)])      # T = 1, whole tiles, one layer
def test_backward_matches_float64_autograd_and_repeats_bit_equal(dims, B, T):
    from optistate_amd import RNN
    I, H, L, C = dims
    torch.manual_seed(2)
    m = RNN(I, H, L, C, torch.device("cuda")).to("cuda")
    x = torch.rand(B, T, I); y = torch.rand(B, C // 2)
    ref_out, ref_loss, ref_g, ref_dx = reference({k: v.detach().cpu() for k, v in m.state_dict().items()}, dims, x, y)
    runs = []
    for _ in range(2):                                       # no atomics in the sweep and weight-gradient kernels: same bits twice
        m.zero_grad()
        xg = x.cuda().requires_grad_(True)                   # the need_dx path of layer 0
        out = m(xg)
        tgt = torch.cat([y.cuda(), (out[:, :C // 2].detach() - y.cuda()).abs()], dim=1)
        loss = torch.nn.functional.mse_loss(out, tgt)        # the reference's criterion; torch only does bookkeeping
        loss.backward()
        runs.append({k: p.grad.clone() for k, p in m.named_parameters()} | {"x": xg.grad.clone()})
    assert (out.detach().cpu().double() - ref_out).abs().max().item() < 1e-5
    assert abs(loss.item() - ref_loss) < 1e-6
    assert m._engine.kernel_name("train_sweep") == "bwd_sweep_stream_kernel" and m._engine.kernel_name("train_dw") == "dw_stream_kernel"
    for k, r in list(ref_g.items()) + [("x", ref_dx)]:
        g, scale = runs[0][k].cpu().double(), max(r.abs().max().item(), 1e-8)
        print(f"{k}: max |g - ref| {(g - r).abs().max().item():.3e} of {scale:.3e}")
        assert (g - r).abs().max().item() < 2e-4 * scale + 1e-9, (k, (g - r).abs().max().item(), scale)
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_trainer_step_at_hidden_256():
    from optistate_amd import RNN
    from optistate_amd.train import DataParallelTrainer
    dims, B, T = (60, 256, 2, 24), 64, 3
    torch.manual_seed(4)
    m = RNN(*dims, torch.device("cuda")).to("cuda")
    x = torch.rand(B, T, dims[0]); y = torch.rand(B, dims[3] // 2)
    _, ref_loss, _, _ = reference({k: v.detach().cpu() for k, v in m.state_dict().items()}, dims, x, y)
    tr = DataParallelTrainer(m, lr=0.0001)
    loss = tr.step(x.cuda(), y.cuda()).item()
    assert abs(loss - ref_loss) < 1e-6
    assert tr.step(x.cuda(), y.cuda()).item() != loss        # the fused Adam moved the weights the second forward read
