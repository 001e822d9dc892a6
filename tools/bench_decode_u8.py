"""Final latent -> host-ready uint8 image at latent 128 x 128 (SDXL ddconfig, fp32 parameters, seeded synthetic weights), two paths
interleaved in one process on one MI355X ("From the job to images"):
  new     FirstStage.decode_u8(z).cpu()                               cd360_post_quant_f32 -> Decoder.forward_u8 (cd360_vae_conv_out_u8)
  parent  (torch.clip(dec(pqc(1 / sf * z))[0].permute(1, 2, 0) * 0.5 + 0.5, 0, 1.).cpu().numpy() * 255).astype(np.uint8)   (sample.py:346)
          the framework's 1 x 1 convolution, Decoder.forward, then the reference's own image conversion through torch and numpy
Host clock around each call; both end in a device-to-host copy, which synchronises.  Two warm calls per path, then 12 timed rounds whose
order alternates.  Usage: python tools/bench_decode_u8.py"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "custom-diffusion360_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import numpy as np
import torch

import weights as W
from cd360 import images
from sgm.modules.diffusionmodules.model import Decoder

CFG = dict(attn_type="vanilla-xformers", double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128,
           ch_mult=[1, 2, 4, 4], num_res_blocks=2, attn_resolutions=[], dropout=0.0)
dev = torch.device("cuda:0")
dec = Decoder(**CFG).eval()
W.load_into(dec, 3)
pqc = torch.nn.Conv2d(4, 4, 1)
with torch.no_grad():
    pqc.weight.copy_(W.tensor("pqc.w", (4, 4, 1, 1), seed=3) * 0.5)
    pqc.bias.copy_(W.tensor("pqc.b", (4,), seed=3) * 0.05)
dec, pqc = dec.to(dev), pqc.to(dev)
for p in list(dec.parameters()) + list(pqc.parameters()):
    p.requires_grad_(False)
fs = images.FirstStage(None, dec, None, pqc)
sf = 0.13025
z = W.tensor("z128", (1, 4, 128, 128), seed=1).to(dev) * sf


def new():
    return fs.decode_u8(z).cpu().numpy()[0]


@torch.no_grad()
def parent():
    out = dec(pqc(1.0 / sf * z))
    return (torch.clip(out[0].permute(1, 2, 0) * 0.5 + 0.5, 0, 1.).cpu().numpy() * 255).astype(np.uint8)


a, b = new(), parent()
print("image", a.shape, a.dtype, "| bytes that differ between the paths:", int((a != b).sum()), "of", a.size,
      "| max |difference|", int(np.abs(a.astype(int) - b.astype(int)).max()))
for _ in range(2):
    new(), parent()
t = {"new": [], "parent": []}
for r in range(12):
    for name, fn in (("new", new), ("parent", parent)) if r % 2 == 0 else (("parent", parent), ("new", new)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t[name].append((time.perf_counter() - t0) * 1e3)
for name, v in t.items():
    print(f"{name}: median {statistics.median(v):.2f} ms | min {min(v):.2f} | max {max(v):.2f} | n {len(v)}")
print(f"median(parent) - median(new) = {statistics.median(t['parent']) - statistics.median(t['new']):.2f} ms")
