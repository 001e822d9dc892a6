"""fp32 framework restatement of the reference's first-stage Encoder.forward (sgm/modules/diffusionmodules/model.py:74-90,487-601) on a
state_dict, built from the block helpers of tests/vae_fp32.py; Downsample is F.pad(x, (0, 1, 0, 1)) + F.conv2d(stride=2).  It runs
wherever its tensors are (CPU or GPU): the yardstick of tests/test_vae_encoder_gpu.py at full size and the baseline column of
tools/bench_vae.py.  Not part of the product."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from vae_fp32 import _conv, _gn, attnblock, resblock


def downsample(sd, p, x):
    return F.conv2d(F.pad(x, (0, 1, 0, 1)), sd[p + ".conv.weight"], sd[p + ".conv.bias"], stride=2)


def encode(sd: dict, x: torch.Tensor, ch_mult, num_res_blocks: int) -> torch.Tensor:
    """Encoder.forward(x) for the state_dict `sd` (fp32 tensors on x's device)."""
    h = _conv(sd, "conv_in", x)
    for lvl in range(len(ch_mult)):
        for i in range(num_res_blocks):
            h = resblock(sd, f"down.{lvl}.block.{i}", h)
            if f"down.{lvl}.attn.{i}.q.weight" in sd:
                h = attnblock(sd, f"down.{lvl}.attn.{i}", h)
        if lvl != len(ch_mult) - 1:
            h = downsample(sd, f"down.{lvl}.downsample", h)
    h = resblock(sd, "mid.block_1", h)
    h = attnblock(sd, "mid.attn_1", h)
    h = resblock(sd, "mid.block_2", h)
    return _conv(sd, "conv_out", _gn(sd, "norm_out", h, True))
