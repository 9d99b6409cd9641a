#!/usr/bin/env python3
"""Device time of the frame ingest at the reference's shape: N seeded 480 x 640 x 3 uint8 frames resident on the device ->
224 x 224 float frames (os_frames_ingest), and the ViT latent from frames (os_vit_encode_frames) beside the latent from float
frames (os_vit_encode), alternating in one process.  Every call is timed by a pair of device events on the launch stream; after a
warm-up the median and the 10th / 90th percentile over the repetitions are reported, with the byte floor
(N H W C + 4 N S^2 bytes at 8 TB/s), the read traffic of the tile windows from the plan, and the outputs' bit equality with the
two-call path.
usage: python3 tools/frames_ingest_time.py [--frames 1024] [--reps 40] [--warm 5] [--out profiles/frames_ingest.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from optistate_amd.engine import default_engine, _ptr                       # noqa: E402
from optistate_amd.transformer_model import Transformer_Autoencoder         # noqa: E402

H, W, CH, S = 480, 640, 3, 224
HBM_BYTES_PER_S = 8e12


def spread(ts):
    ts = sorted(ts)
    return {"median_ms": ts[len(ts) // 2], "p10_ms": ts[len(ts) // 10], "p90_ms": ts[len(ts) * 9 // 10], "min_ms": ts[0],
            "max_ms": ts[-1], "calls": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_ingest.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frames_ingest_time: needs the MI355X (a kernel time is a GPU measurement)")
    N = args.frames
    eng = default_engine(0)
    torch.manual_seed(0)
    model = Transformer_Autoencoder().to("cuda")
    frames = torch.randint(0, 256, (N, H, W, CH), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    floats = model.preprocess(frames)
    lat_ref = model.forward_encoder(floats)            # loads the weights; the two-call path's bits
    out = torch.empty((N, S, S), dtype=torch.float32, device="cuda")
    lat = torch.empty((N, model.embed_dim), dtype=torch.float32, device="cuda")
    fptr, st = C.c_void_p(frames.data_ptr()), eng._stream()
    calls = {
        "os_frames_ingest": lambda: eng.lib.os_frames_ingest(eng._h, N, fptr, H, W, CH, S, _ptr(out), st),
        "os_vit_encode_frames": lambda: eng.lib.os_vit_encode_frames(eng._h, N, fptr, H, W, CH, _ptr(lat), st),
        "os_vit_encode": lambda: eng.lib.os_vit_encode(eng._h, N, _ptr(floats), _ptr(lat), st),
    }
    times = {k: [] for k in calls}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(args.warm + args.reps):
        for name, call in calls.items():               # alternating: the three share whatever else the machine is doing
            e0.record()
            eng._check(call(), name)
            e1.record()
            e1.synchronize()
            if rep >= args.warm:
                times[name].append(e0.elapsed_time(e1))
    eng._check(calls["os_vit_encode_frames"](), "os_vit_encode_frames")
    torch.cuda.synchronize()
    plan = eng.frames_plan_info(H, W, CH, S)
    floor_bytes = N * H * W * CH + 4 * N * S * S
    res = {"shape": {"frames": N, "H": H, "W": W, "C": CH, "out_size": S}, "device": torch.cuda.get_device_name(0),
           "reps": args.reps, "warm": args.warm, "plan": plan,
           "bit_equal": {"ingest_vs_preprocess": bool(torch.equal(out, floats[:, 0])),
                         "encode_frames_vs_two_calls": bool(torch.equal(lat, lat_ref[:, 0]))}}
    for name in calls:
        res[name] = spread(times[name])
    t = res["os_frames_ingest"]["median_ms"] * 1e-3
    res["byte_floor"] = {"bytes": floor_bytes, "ms_at_8TBps": floor_bytes / HBM_BYTES_PER_S * 1e3,
                         "achieved_TBps": floor_bytes / t / 1e12, "share_of_8TBps": floor_bytes / t / HBM_BYTES_PER_S}
    res["window_read_ratio"] = plan["read_bytes_per_image"] / (H * W * CH)      # stage A's loads over the image's bytes
    res["encode_frames_minus_encode_ms"] = res["os_vit_encode_frames"]["median_ms"] - res["os_vit_encode"]["median_ms"]
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
