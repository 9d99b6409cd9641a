#!/usr/bin/env python3
"""Time of the key-tiled attention kernels (vit_attn_tiled.hip) inside the training step of the ViT auto-encoder, N = 64 seeded images:
  (a) the reference's geometry (224 x 224, 3 + 3 blocks of width 128, 4 heads x 32) on two contexts of ONE process: the default
      (attention_mfma_dma_kernel forward, attention_bwd_kernel backward) and OS_VIT_ATT_TILED=1 (the tiled pair);
  (b) embed_dim = decoder_embed_dim = 256 with 4 heads x 64, which only the tiled pair serves.
A step here is os_vit_forward_train + os_vit_backward on a context that holds its model (no optimiser, no reload), timed by the host
clock around both calls and a device synchronise, the arms alternating in blocks behind warm-up steps.  The attention kernels' own time
comes from a second pass, profiler on: the `vit_attn` phase (device events around each launch) read behind the forward and behind the
backward.  Share of peak: the products the algorithm needs, 4 L^2 hd flop per (image, head) forward and 14 L^2 hd backward (the
recompute form: S and dP in both backward kernels, seven tile products against the forward's two), over kernel time and 157.3 TFLOP/s.
usage: python3 tools/vit_attention_tiled.py [--steps 100] [--block 10] [--warm 3] [--batch 64] [--out profiles/vit_attention_tiled.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from optistate_amd import Engine                                             # noqa: E402
from optistate_amd.engine import _ptr                                        # noqa: E402
from optistate_amd.transformer_model import Transformer_Autoencoder         # noqa: E402

PEAK_FP32_MFMA = 157.3e12


class Arm:
    """One context with its own copy of the model loaded, its workspace and gradient vectors."""

    def __init__(self, tiled, x, **kw):
        os.environ["OS_VIT_ATT_TILED"] = "1" if tiled else "0"            # read once, by os_create
        self.eng = Engine(0)
        del os.environ["OS_VIT_ATT_TILED"]
        torch.manual_seed(0)
        self.m = Transformer_Autoencoder(decoder=True, trainable=True, **kw).to("cuda")
        self.m._load_flats_locked(self.eng, self.m._flat(x.device), self.m._flat_decoder(x.device))
        self.x, self.N = x, x.shape[0]
        self.ws = torch.empty(self.eng.lib.os_vit_train_ws_floats(self.eng._h, self.N), device="cuda")
        self.loss, self.one = torch.empty((), device="cuda"), torch.ones((), device="cuda")
        self.ge, self.gd = torch.empty_like(self.m._loaded[1]), torch.empty_like(self.m._loaded[2])

    def forward(self):
        e = self.eng
        e._check(e.lib.os_vit_forward_train(e._h, self.N, _ptr(self.x), _ptr(self.ws), None, _ptr(self.loss), e._stream()), "os_vit_forward_train")

    def backward(self):
        e = self.eng
        e._check(e.lib.os_vit_backward(e._h, self.N, _ptr(self.x), _ptr(self.ws), _ptr(self.one), _ptr(self.ge), _ptr(self.gd), e._stream()),
                 "os_vit_backward")

    def attention_ms(self, warm, reps):
        """(forward, backward) device time of the vit_attn phase per step, and the kernels' names."""
        for _ in range(warm):
            self.forward(), self.backward()
        torch.cuda.synchronize()
        self.eng.profile(True)
        self.eng.profile_read()
        f = b = 0.0
        names = []
        for _ in range(reps):
            self.forward()
            torch.cuda.synchronize()
            f += self.eng.profile_read()["vit_attn"][0]
            names.append(self.eng.kernel_name("vit_attn"))
            self.backward()
            torch.cuda.synchronize()
            b += self.eng.profile_read()["vit_attn"][0]
            names.append(self.eng.kernel_name("vit_attn"))
        self.eng.profile(False)
        return f / reps, b / reps, names[:2]


def spread(ts):
    ts = sorted(ts)
    return {"median_ms": statistics.median(ts), "p10_ms": ts[len(ts) // 10], "p90_ms": ts[len(ts) * 9 // 10], "steps": len(ts)}


def measure(arms, args):
    times = {k: [] for k in arms}
    while len(times[next(iter(arms))]) < args.steps:
        for name, arm in arms.items():
            for i in range(args.warm + args.block):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                arm.forward(), arm.backward()
                torch.cuda.synchronize()
                if i >= args.warm:
                    times[name].append((time.perf_counter() - t0) * 1e3)
    out = {}
    for name, arm in arms.items():
        f, b, names = arm.attention_ms(args.warm, 5)
        m = arm.m
        flop = 0.0
        for dim, depth, heads in ((m.embed_dim, m.depth, m.num_heads), (m.decoder_embed_dim, m.decoder_depth, m.decoder_num_heads)):
            flop += depth * arm.N * heads * (m.num_patches + 1) ** 2 * (dim // heads)
        out[name] = {"step_forward_backward": spread(times[name]), "attention_forward_ms": f, "attention_backward_ms": b, "kernels": names,
                     "loss": arm.loss.item()}
        if names[0].startswith("attention_tiled"):                          # the flop count above is the tiled pair's
            out[name]["attention_forward_share_of_fp32_mfma_peak"] = 4 * flop / (f * 1e-3) / PEAK_FP32_MFMA
            out[name]["attention_backward_share_of_fp32_mfma_peak"] = 14 * flop / (b * 1e-3) / PEAK_FP32_MFMA
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vit_attention_tiled.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vit_attention_tiled: needs the MI355X (a kernel time is a GPU measurement)")
    x = torch.rand(args.batch, 224, 224, generator=torch.Generator().manual_seed(1)).cuda()
    res = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "block": args.block, "warm": args.warm}
    res["a_reference_geometry_4x32"] = measure({"whole_head_kernels": Arm(False, x), "tiled_pair": Arm(True, x)}, args)
    wide = dict(embed_dim=256, num_heads=4, decoder_embed_dim=256, decoder_num_heads=4)
    res["b_width_256_4x64"] = measure({"tiled_pair": Arm(False, x, **wide)}, args)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
