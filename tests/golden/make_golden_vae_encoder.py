"""Golden vectors of the first stage's Encoder (reference sgm/modules/diffusionmodules/model.py:487-601), produced by the reference's own
module (CPU, fp32) through refshim.py, with make_golden.py's helpers imported (not copied).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vae_encoder.py

Writes vae_encoder.npz (images x.<case> and fp32 outputs out.<case>, the moments before quant_conv).  Weights come from
weights.load_into(module, SEED) and are not stored: tests/test_vae_encoder_gpu.py regenerates them.  Cases:
  sdxl    the SDXL ddconfig (ch 128, ch_mult [1, 2, 4, 4], configs/train_co3d_concept.yaml:98-114), image 2 x 3 x 64 x 64;
  narrow  ch 64, ch_mult [1, 2, 2], num_res_blocks 1, attn_resolutions [16] (level 2 carries attention), image 1 x 3 x 64 x 80;
  ragged  the narrow config at 1 x 3 x 43 x 51: both Downsamples see odd sizes (43 x 51 -> 21 x 25 -> 10 x 12), the attention has
          N = 120 pixels, and no activation is a whole number of GroupNorm statistics slabs.
"""
from __future__ import annotations

import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402  (refshim import, npz helper)
from make_golden_vae import NARROW_DDCONFIG, SDXL_DDCONFIG, SEED  # noqa: E402

import torch  # noqa: E402

W = G.W
CASES = {"sdxl": (SDXL_DDCONFIG, (2, 3, 64, 64)), "narrow": (NARROW_DDCONFIG, (1, 3, 64, 80)), "ragged": (NARROW_DDCONFIG, (1, 3, 43, 51))}


def main():
    model = importlib.import_module("sgm.modules.diffusionmodules.model")
    arrays = {}
    for name, (cfg, xshape) in CASES.items():
        enc = model.Encoder(**cfg).eval()
        W.load_into(enc, SEED)
        x = W.tensor(f"x.{name}", xshape, SEED)
        with torch.no_grad():
            out = enc(x)
        assert torch.isfinite(out).all()
        print(name, tuple(out.shape), "max", out.abs().max().item(), "std", out.std().item())
        arrays[f"x.{name}"], arrays[f"out.{name}"] = x, out
    G.npz("vae_encoder", **arrays)


if __name__ == "__main__":
    main()
    assert not os.path.exists(os.path.join(G.refshim.REF_ROOT, "sgm", "__pycache__")), "bytecode leaked into the reference tree"
