"""From decoded frames to the loader's batch, for a config-4 batch: 4 samples x (1 target + 4 views) pictures of 800 x 800 with their
masks, to 512 (masks to 64), two paths interleaved in one process on one MI355X ("Pictures in"):
  device  PictureFront.batch on frames that are already on the device                  the launches of include/picture/cd360_picture.h
  host    what the reference's loader does per picture with its image library (crop, resize(BICUBIC), ToTensor, x * 2 - 1; the mask
          through > 125, a mode-"1" image, crop, resize; conv2d + clamp), then the upload of the batch
Host clock around each call, ended by a device synchronise.  Two warm calls per path, then 10 timed rounds whose order alternates.  The
uint8 frames' own upload (20 x 1.9 MB) is timed separately: the device path needs it where frames are decoded on the host.  The two
paths' pictures are compared (levels that differ).  Usage: python tools/bench_pictures.py"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "custom-diffusion360_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

import picture_cases as PC
from cd360 import pictures

B, N_REF, SIDE, S = 4, 4, 800, 512
dev = torch.device("cuda:0")
front = pictures.PictureFront(img_size=S)
n = B * (1 + N_REF)
frames = [PC.picture(SIDE, SIDE, 3, seed=j, kind=("smooth", "noise")[j % 2]) for j in range(n)]
masks = [PC.blob_mask(SIDE, SIDE, seed=100 + j) for j in range(n)]
boxes = front.boxes([(SIDE, SIDE)] * n, [None if j % (1 + N_REF) == 0 else [90 + 7 * j, 60, 700 + 5 * j, 790] for j in range(n)])
d_frames, d_masks = [torch.from_numpy(f).to(dev) for f in frames], [torch.from_numpy(m).to(dev) for m in masks]


def device():
    out = front.batch(d_frames, d_masks, boxes, N_REF)
    torch.cuda.synchronize()
    return out


def upload():
    out = [torch.from_numpy(f).to(dev) for f in frames] + [torch.from_numpy(m).to(dev) for m in masks]
    torch.cuda.synchronize()
    return out


def host():
    x, m, pad = [], [], []
    for f, k, b in zip(frames, masks, boxes):
        box = tuple(int(v) for v in b)
        x.append(torch.from_numpy(np.array(Image.fromarray(f).crop(box).resize((S, S), Image.BICUBIC))).permute(2, 0, 1).float().div(255) * 2.0 - 1.0)
        m.append(torch.from_numpy(np.array(Image.fromarray(k > 125).crop(box).resize((S // 8, S // 8)))).float()[None])
        pad.append(torch.from_numpy(np.array(Image.fromarray(np.ones_like(k) > 0).crop(box).resize((S // 8, S // 8)))).float()[None])
    x, m, pad = torch.stack(x).reshape(B, 1 + N_REF, 3, S, S), torch.stack(m).reshape(B, 1 + N_REF, 1, S // 8, S // 8), torch.stack(pad)
    dil = torch.clamp(F.conv2d(m[:, 0], torch.ones(1, 1, 7, 7), padding="same"), 0, 1)
    out = {"jpg": x[:, 0].to(dev), "jpg_ref": x[:, 1:].to(dev), "mask": dil.to(dev), "depth": m[:, 0].to(dev),
           "mask_ref": pad.reshape(B, 1 + N_REF, 1, S // 8, S // 8)[:, 1:].to(dev)}
    torch.cuda.synchronize()
    return out


a, b = device(), host()
for key in ("jpg", "jpg_ref"):
    d = ((a[key] - b[key]).abs() * 127.5).round()
    print(f"{key}: {tuple(a[key].shape)} | values that differ between the paths: {int((d > 0).sum())} of {d.numel()} | max {int(d.max())} level(s)")
for key in ("mask", "depth", "mask_ref"):
    print(f"{key}: {tuple(a[key].shape)} | values that differ: {int((a[key] != b[key]).sum())}")
for _ in range(2):
    device(), host(), upload()
t = {"device": [], "host": [], "upload": []}
fns = (("device", device), ("host", host), ("upload", upload))
for r in range(10):
    for name, fn in fns if r % 2 == 0 else fns[::-1]:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t[name].append((time.perf_counter() - t0) * 1e3)
for name, v in t.items():
    print(f"{name}: median {statistics.median(v):.2f} ms | min {min(v):.2f} | max {max(v):.2f} | n {len(v)}")
