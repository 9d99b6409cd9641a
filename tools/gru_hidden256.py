"""RNN(188, 256, 4, 24) on the weight-streaming kernels (csrc/gru_stream_kernels.hip): inference at B = 65,536, T = 100 and one
training step at B = 8,192, T = 10, per-phase device times from Engine.profile.

    python tools/gru_hidden256.py [--out profiles/gru_hidden256.json]

Share of peak: the gate GEMM's flops, 2 B T 3H (K + H) per layer, against the 157.3 TFLOP/s fp32 MFMA peak bench.py uses."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from optistate_amd import RNN  # noqa: E402
from optistate_amd.train import DataParallelTrainer  # noqa: E402

PEAK_TF = 157.3
DIMS = (188, 256, 4, 24)


def phases(eng, fn, iters):
    fn(); torch.cuda.synchronize()                           # warm-up: allocations, packing
    eng.profile(True); eng.profile_read()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record(); torch.cuda.synchronize()
    prof = eng.profile_read(); eng.profile(False)
    return t0.elapsed_time(t1) / iters, {k: (ms / iters, n // iters) for k, (ms, n) in prof.items() if n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/gru_hidden256.json")
    a = ap.parse_args()
    I, H, L, C = DIMS
    torch.manual_seed(0)
    m = RNN(I, H, L, C, torch.device("cuda")).to("cuda")
    res = {"command": "python tools/gru_hidden256.py", "model": "RNN(188, 256, 4, 24)", "fp32_mfma_peak_tflops": PEAK_TF}

    B, T = 65536, 100
    x = torch.rand(B, T, I, device="cuda")
    with torch.no_grad():
        m(x[:64])                                            # binds the engine
        ms, prof = phases(m._engine, lambda: m(x), 3)
    lay_ms = prof["gru_layer"][0] / L
    flops = sum(2.0 * B * T * 3 * H * ((I if l == 0 else H) + H) for l in range(L))
    res["inference_B65536_T100"] = {"ms_per_pass": ms, "ms_per_layer_mean": lay_ms, "kernel": m._engine.kernel_name("gru_layer"),
                                    "gate_gemm_tflops": flops / (prof["gru_layer"][0] * 1e-3) / 1e12,
                                    "share_of_fp32_mfma_peak": flops / (prof["gru_layer"][0] * 1e-3) / 1e12 / PEAK_TF,
                                    "steps_per_s": B * T / (ms * 1e-3)}
    del x

    B, T = 8192, 10
    x, y = torch.rand(B, T, I, device="cuda"), torch.rand(B, C // 2, device="cuda")
    tr = DataParallelTrainer(m, lr=1e-4)
    ms, prof = phases(m._engine, lambda: tr.step(x, y), 5)
    res["training_B8192_T10"] = {"ms_per_step": ms, "forward_layers_ms": prof["gru_layer"][0], "sweep_ms": prof["train_sweep"][0],
                                 "dw_ms": prof["train_dw"][0], "misc_ms": prof.get("train_misc", (0.0, 0))[0],
                                 "kernels": {p: m._engine.kernel_name(p) for p in ("gru_layer", "train_sweep", "train_dw")}}
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
