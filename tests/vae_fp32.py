"""fp32 framework restatement of the reference's first-stage Decoder.forward (sgm/modules/diffusionmodules/model.py:94-265,604-733) on a
state_dict: F.conv2d, F.group_norm, nearest F.interpolate and single-head attention chunked over the queries (no full N x N fp32 score
matrix).  It runs wherever its tensors are (CPU or GPU): the yardstick of tests/test_vae_gpu.py at full size and the baseline column of
tools/bench_vae.py.  Not part of the product."""
from __future__ import annotations

import torch
import torch.nn.functional as F


def _gn(sd, p, x, silu):
    x = F.group_norm(x, 32, sd[p + ".weight"], sd[p + ".bias"], eps=1e-6)
    return x * torch.sigmoid(x) if silu else x


def _conv(sd, p, x, pad=1):
    return F.conv2d(x, sd[p + ".weight"], sd[p + ".bias"], padding=pad)


def resblock(sd, p, x):
    h = _conv(sd, p + ".conv1", _gn(sd, p + ".norm1", x, True))
    h = _conv(sd, p + ".conv2", _gn(sd, p + ".norm2", h, True))
    if p + ".nin_shortcut.weight" in sd:
        x = _conv(sd, p + ".nin_shortcut", x, 0)
    elif p + ".conv_shortcut.weight" in sd:
        x = _conv(sd, p + ".conv_shortcut", x)
    return x + h


def attention(q, k, v, chunk=2048):
    """softmax(q k^T / sqrt(C)) v for q, k, v [B, N, C] fp32, `chunk` queries at a time."""
    scale = q.shape[-1] ** -0.5
    out = torch.empty_like(q)
    for i in range(0, q.shape[1], chunk):
        s = torch.matmul(q[:, i:i + chunk], k.transpose(1, 2)) * scale
        out[:, i:i + chunk] = torch.matmul(torch.softmax(s, -1), v)
    return out


def attnblock(sd, p, x):
    b, c, h, w = x.shape
    hn = _gn(sd, p + ".norm", x, False)
    q, k, v = (_conv(sd, f"{p}.{n}", hn, 0).reshape(b, c, h * w).transpose(1, 2) for n in "qkv")
    a = attention(q, k, v).transpose(1, 2).reshape(b, c, h, w)
    return x + _conv(sd, p + ".proj_out", a, 0)


def decode(sd: dict, z: torch.Tensor, ch_mult, num_res_blocks: int) -> torch.Tensor:
    """Decoder.forward(z) for the state_dict `sd` (fp32 tensors on z's device)."""
    h = _conv(sd, "conv_in", z)
    h = resblock(sd, "mid.block_1", h)
    h = attnblock(sd, "mid.attn_1", h)
    h = resblock(sd, "mid.block_2", h)
    for lvl in reversed(range(len(ch_mult))):
        for i in range(num_res_blocks + 1):
            h = resblock(sd, f"up.{lvl}.block.{i}", h)
            if f"up.{lvl}.attn.{i}.q.weight" in sd:
                h = attnblock(sd, f"up.{lvl}.attn.{i}", h)
        if lvl != 0:
            h = _conv(sd, f"up.{lvl}.upsample.conv", F.interpolate(h, scale_factor=2.0, mode="nearest"))
    return _conv(sd, "conv_out", _gn(sd, "norm_out", h, True))
