#!/usr/bin/env python3
"""Device time of the frame augmentation at the reference's shape: N seeded 224 x 224 uint8 gray images and their
optistate_amd.augment.sample_params records resident on the device -> augmented float frames (os_frames_augment), beside
os_frames_ingest of N 480 x 640 x 3 frames in the same run, alternating in one process.  Every call is timed by a pair of device
events on the launch stream; after a warm-up the median and the 10th / 90th percentile over the repetitions are reported, with the
byte floor N S^2 (1 + 4) bytes at 8 TB/s, the share of images that take the crop path, and bit equality of the first images with
the Pillow chain on the host, whose per-image time (one thread, a CPU measurement of the machine this runs on) is reported too.
usage: python3 tools/frames_augment_time.py [--frames 64 1024] [--reps 40] [--warm 5] [--out profiles/frames_augment.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from optistate_amd import augment                                           # noqa: E402
from optistate_amd.engine import default_engine, _ptr                       # noqa: E402
from frames_ingest_time import spread, HBM_BYTES_PER_S                       # noqa: E402

H, W, CH, S = 480, 640, 3, 224


def pillow_chain(g, p):
    """The record's transforms through Pillow itself (the matrix goes to transform(AFFINE), as Image.rotate hands it over)."""
    from PIL import Image
    im, flags = Image.fromarray(g), int(p[14])
    if flags & 1:
        im = im.transform((S, S), Image.AFFINE, list(p[0:6]), Image.NEAREST, fillcolor=0)
    if flags & 2:
        im = im.transpose(Image.FLIP_TOP_BOTTOM)
    if flags & 4:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    if flags & 8:
        im = im.transform((S, S), Image.PERSPECTIVE, list(p[6:14]), Image.NEAREST, fillcolor=0)
    if flags & 16:
        top, left, h, w = (int(v) for v in p[15:19])
        im = im.crop((left, top, left + w, top + h)).resize((S, S), Image.BILINEAR)
    return np.asarray(im, np.float32) / np.float32(255)


def measure(eng, N, reps, warm):
    gray_h = np.random.default_rng(1).integers(0, 256, (N, S, S), dtype=np.uint8)
    params_h = augment.sample_params(N, S, 2)
    gray, params = torch.from_numpy(gray_h).cuda(), torch.from_numpy(params_h).cuda()
    frames = torch.randint(0, 256, (N, H, W, CH), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    out = torch.empty((N, S, S), dtype=torch.float32, device="cuda")
    out2 = torch.empty_like(out)
    st = eng._stream()
    calls = {
        "os_frames_augment": lambda: eng.lib.os_frames_augment(eng._h, N, C.c_void_p(gray.data_ptr()), S, C.c_void_p(params.data_ptr()),
                                                               _ptr(out), st),
        "os_frames_ingest": lambda: eng.lib.os_frames_ingest(eng._h, N, C.c_void_p(frames.data_ptr()), H, W, CH, S, _ptr(out2), st),
    }
    times = {k: [] for k in calls}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(warm + reps):
        for name, call in calls.items():               # alternating: the two share whatever else the machine is doing
            e0.record()
            eng._check(call(), name)
            e1.record()
            e1.synchronize()
            if rep >= warm:
                times[name].append(e0.elapsed_time(e1))
    k = min(N, 32)
    t0 = time.perf_counter()
    host = np.stack([pillow_chain(gray_h[n], params_h[n]) for n in range(k)])
    cpu_ms = (time.perf_counter() - t0) * 1e3 / k
    floor_bytes = N * S * S * (1 + 4)
    res = {"frames": N, "crop_share": float((params_h[:, 14].astype(int) & 16 > 0).mean()),
           "bit_equal_to_pillow_first_images": bool(np.array_equal(out[:k].cpu().numpy(), host)), "images_compared": k,
           "pillow_chain_cpu_ms_per_image": cpu_ms}
    for name in calls:
        res[name] = spread(times[name])
    t = res["os_frames_augment"]["median_ms"] * 1e-3
    res["byte_floor"] = {"bytes": floor_bytes, "ms_at_8TBps": floor_bytes / HBM_BYTES_PER_S * 1e3,
                         "achieved_TBps": floor_bytes / t / 1e12, "share_of_8TBps": floor_bytes / t / HBM_BYTES_PER_S}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_augment.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frames_augment_time: needs the MI355X (a kernel time is a GPU measurement)")
    eng = default_engine(0)
    res = {"shape": {"S": S, "ingest": [H, W, CH]}, "device": torch.cuda.get_device_name(0), "reps": args.reps, "warm": args.warm,
           "runs": [measure(eng, N, args.reps, args.warm) for N in args.frames]}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
