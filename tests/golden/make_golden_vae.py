"""Golden vectors of the first stage's Decoder (reference sgm/modules/diffusionmodules/model.py:604-733), produced by the reference's own
module (CPU, fp32) through refshim.py, with make_golden.py's helpers imported (not copied).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vae.py

Writes vae_decoder.npz (latents z.<case> and fp32 outputs out.<case>) and vae_decoder.keys.json.gz / vae_encoder.keys.json.gz (names and
shapes at the SDXL ddconfig, configs/train_co3d_concept.yaml:98-114).  Weights come from weights.load_into(module, SEED) and are not
stored: tests/test_vae_gpu.py regenerates them.  Cases:
  sdxl    SDXL widths (ch 128, ch_mult [1, 2, 4, 4]), 16 x 16 latent, batch 2, attn_type vanilla-xformers (the config's);
  narrow  ch 64, ch_mult [1, 2, 2], attn_resolutions [16] (so the up blocks carry attention), 20 x 24 latent: N = 480 pixels, not a
          multiple of the 64-pixel query blocks of cd360_attn_single_bf16 (its 32-key tiles divide it);
  ragged  the narrow config at a 21 x 25 latent: N = 525 pixels, a ragged last 32-key tile (13 keys) in every attention block and no
          GroupNorm slab statistics (H W is not a multiple of 64).
"""
from __future__ import annotations

import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402  (refshim import, npz / keyfile)

import torch  # noqa: E402

W = G.W
SEED = 3
SDXL_DDCONFIG = dict(attn_type="vanilla-xformers", double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128,
                     ch_mult=[1, 2, 4, 4], num_res_blocks=2, attn_resolutions=[], dropout=0.0)
NARROW_DDCONFIG = dict(attn_type="vanilla-xformers", double_z=True, z_channels=4, resolution=64, in_channels=3, out_ch=3, ch=64,
                       ch_mult=[1, 2, 2], num_res_blocks=1, attn_resolutions=[16], dropout=0.0)
CASES = {"sdxl": (SDXL_DDCONFIG, (2, 4, 16, 16)), "narrow": (NARROW_DDCONFIG, (1, 4, 20, 24)), "ragged": (NARROW_DDCONFIG, (1, 4, 21, 25))}


def main():
    model = importlib.import_module("sgm.modules.diffusionmodules.model")
    arrays = {}
    for name, (cfg, zshape) in CASES.items():
        dec = model.Decoder(**cfg).eval()
        W.load_into(dec, SEED)
        z = W.tensor(f"z.{name}", zshape, SEED)
        with torch.no_grad():
            out = dec(z)
        assert torch.isfinite(out).all()
        print(name, tuple(out.shape), "max", out.abs().max().item(), "std", out.std().item())
        arrays[f"z.{name}"], arrays[f"out.{name}"] = z, out
        if name == "sdxl":
            G.keyfile("vae_decoder", dec)
            G.keyfile("vae_encoder", model.Encoder(**cfg))
    G.npz("vae_decoder", **arrays)


if __name__ == "__main__":
    main()
    assert not os.path.exists(os.path.join(G.refshim.REF_ROOT, "sgm", "__pycache__")), "bytecode leaked into the reference tree"
