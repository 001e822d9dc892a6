"""Golden vectors of the reference's rank-32 attention adapters (add_lora=True, sgm/modules/attention.py:330-347,373-376,421-424) in one
pose block, produced by the reference's own modules (CPU, fp32) through refshim.py, with make_golden.py's helpers imported (not copied).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lora.py

Writes block_lora_eval.npz, block_lora_train.npz and block_lora.keys.json.gz.  Sizes and inputs are those of make_golden.case_block.
Every parameter, the zero-initialised up weights included, is randomised by weights.load_into: an all-zero up weight would make each
comparison vacuous.  In the TRAIN fixture the reference's four adapter dropouts (dropoutq / k / v / o of attn1 and attn2) are set to p = 0
here, in the generator: their masks are drawn by torch's generator and cannot be reproduced by a counter-based kernel.  Everything else
runs in train mode: the stratified xy / depth jitter is recorded as case_block does, and the fp32 autograd gradients of the fixed scalar
loss (out * cot).sum() + fg.sum() + rgb.sum() are stored for every `poseattn`-trainable parameter (diffusion.py:117-150: the pose
parameters and attn1 / attn2 of the pose block, adapters included) as grad.<name>.
"""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402  (refshim import, Recorder, npz / keyfile / jitter_kw)

import torch  # noqa: E402

W, ns, synth, pack_cameras = G.W, G.ns, G.synth, G.pack_cameras


def make_lora_block(C, heads, ctx_dim, S):
    return ns.attention.BasicTransformerBlock(C, heads, 64, context_dim=ctx_dim, checkpoint=False, attn_mode="softmax-xformers", image_cross=True,
                                              far=2, num_samples=S, rgb_predict=True, mode="feature-nerf", stratified=True, add_lora=True)


def poseattn(name: str) -> bool:
    return "pose" in name or name.startswith(("attn1.", "attn2."))


def case_block_lora(train: bool):
    C, heads, r, n, S, b, T, cd = 64, 1, 8, 2, 4, 2, 77, 32
    blk = make_lora_block(C, heads, cd, S)
    W.load_into(blk, seed=2)
    assert all(blk.state_dict()[f"{a}.to_{w}_attn3_up.weight"].abs().max() > 0 for a in ("attn1", "attn2") for w in "qkvo")
    blk.train(train)
    for a in (blk.attn1, blk.attn2):
        for w in "qkvo":
            getattr(a, f"dropout{w}").p = 0.0  # see the module docstring
    pose = synth.pose_batch(b, n, seed=4)
    x = W.tensor("x", (b, r * r, C), seed=2)
    ctx = W.tensor("ctx", (b, T, cd), seed=2)
    cref = W.tensor("cref", (b * n, r * r, C), seed=2)
    torch.manual_seed(12)
    for name, p_ in blk.named_parameters():
        p_.requires_grad = train and poseattn(name)
    with G.Recorder() as rec, torch.set_grad_enabled(train):
        out, fg, wts, alphas, rgb = blk(x, context=ctx, context_ref=cref, pose=pose)
        assert wts is None
        grads = {}
        if train:
            cot = W.tensor("cot", tuple(out.shape), seed=2)
            ((out * cot).sum() + fg.sum() + rgb.sum()).backward()
            grads = {f"grad.{name}": p_.grad for name, p_ in blk.named_parameters() if p_.requires_grad and p_.grad is not None}
    with torch.no_grad():
        plain = blk(x, context=ctx)[0] if not train else None
    G.npz("block_lora_train" if train else "block_lora_eval", cams=pack_cameras(pose), x=x, ctx=ctx, cref=cref, out=out.detach(), fg=fg.detach(),
          alphas=alphas.detach(), rgb=rgb.detach(), plain=plain, **G.jitter_kw(rec), **grads)
    if not train:
        G.keyfile("block_lora", blk)


if __name__ == "__main__":
    case_block_lora(False)
    case_block_lora(True)
    assert not os.path.exists(os.path.join(G.refshim.REF_ROOT, "sgm", "__pycache__")), "bytecode leaked into the reference tree"
