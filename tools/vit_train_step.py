#!/usr/bin/env python3
"""Step time of the ViT auto-encoder's training loop at the reference's shape (224 x 224, 3 + 3 blocks of width 128, N = 64 seeded
images), two loops in ONE process:
  (a) Transformer_Autoencoder(decoder=True, trainable=True): loss.backward() through autograd + torch.optim.AdamW on the decay
      groups of optistate_amd.train.add_weight_decay -- every step re-concatenates and re-packs the weights;
  (b) optistate_amd.train.VitTrainer: resident weights, os_vit_adamw_step.
They alternate in blocks (the context holds one model: the first steps of a block reload it, so every block starts with untimed
warm-up steps).  A step is timed by the host clock around the step and a device synchronise.  Both loops take the same steps
from the same weights on the same images, so their losses are compared too.  A second pass, profiler on, gives the engine's
per-phase split (device time and launches per step); torch's own kernels (loop (a)'s optimiser and concatenations) are not in it.
usage: python3 tools/vit_train_step.py [--steps 60] [--block 10] [--warm 3] [--batch 64] [--out profiles/vit_train_step.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from optistate_amd.train import VitTrainer, add_weight_decay                # noqa: E402
from optistate_amd.transformer_model import Transformer_Autoencoder         # noqa: E402

HYPER = dict(lr=4e-4, betas=(0.9, 0.95), eps=1e-8)
WEIGHT_DECAY, LOOP_LOSS_RTOL = 1e-3, 8e-7


def spread(ts):
    ts = sorted(ts)
    return {"median_ms": statistics.median(ts), "p10_ms": ts[len(ts) // 10], "p90_ms": ts[len(ts) * 9 // 10], "min_ms": ts[0],
            "max_ms": ts[-1], "steps": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vit_train_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vit_train_step: needs the MI355X (a step time is a GPU measurement)")
    torch.manual_seed(0)
    a = Transformer_Autoencoder(decoder=True, trainable=True).to("cuda")
    b = Transformer_Autoencoder(decoder=True).to("cuda")
    b.load_state_dict(a.state_dict())
    x = torch.rand(args.batch, 1, 224, 224, generator=torch.Generator().manual_seed(1)).cuda()
    opt = torch.optim.AdamW(add_weight_decay(a, WEIGHT_DECAY), **HYPER)
    tr = VitTrainer(b, weight_decay=WEIGHT_DECAY, **HYPER)

    def step_a():
        opt.zero_grad()
        loss, _ = a(x)
        loss.backward()
        opt.step()
        return loss

    loops = {"autograd_torch_adamw": step_a, "vit_trainer": lambda: tr.step(x)}
    times, losses = {k: [] for k in loops}, {k: [] for k in loops}
    while len(times["vit_trainer"]) < args.steps:
        for name, step in loops.items():
            for i in range(args.warm + args.block):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loss = step()
                torch.cuda.synchronize()
                if i >= args.warm:
                    times[name].append((time.perf_counter() - t0) * 1e3)
                losses[name].append(loss.item())
    res = {"shape": {"img": 224, "batch": args.batch, "encoder": [128, 3, 4], "decoder": [128, 3, 4]}, "hyper": {**HYPER, "weight_decay": WEIGHT_DECAY},
           "device": torch.cuda.get_device_name(0), "block": args.block, "warm": args.warm}
    for name in loops:
        res[name] = spread(times[name])
    la, lb = losses["autograd_torch_adamw"], losses["vit_trainer"]
    rel = [abs(p - q) / abs(p) for p, q in zip(la, lb)]
    res["losses"] = {"steps_taken": len(la), "first": [la[0], lb[0]], "after_3": [la[2], lb[2]], "last": [la[-1], lb[-1]],
                     "rel_after_3": max(rel[:3]), "rel_last": rel[-1], "rel_max": max(rel), "rtol": LOOP_LOSS_RTOL,
                     "after_3_within_rtol": max(rel[:3]) < LOOP_LOSS_RTOL, "last_within_rtol": rel[-1] < LOOP_LOSS_RTOL}
    # the engine's phases, profiler on: a pass of its own
    eng, nprof = tr.eng, 5
    eng.profile(True)
    res["phases_per_step"] = {}
    for name, step in loops.items():
        for _ in range(args.warm):
            step()
        torch.cuda.synchronize()
        eng.profile_read()
        for _ in range(nprof):
            step()
        torch.cuda.synchronize()
        res["phases_per_step"][name] = {k: {"ms": ms / nprof, "launches": n / nprof} for k, (ms, n) in eng.profile_read().items() if n}
    eng.profile(False)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
