"""add_lora=True (the reference's rank-32 attention adapters, sgm/modules/attention.py:330-347) on the host side: the drop-in state_dict,
the reference's initialisation, the fine-tuning selection / optimiser groups / delta checkpoint, and the C ABI of the adapter kernel."""
import gzip
import json
import os

import torch

from cd360 import finetune

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ADAPTERS = [f"{a}.to_{w}_attn3_{d}.weight" for a in ("attn1", "attn2") for w in "qkvo" for d in ("down", "up")]


def _block(**kw):
    from sgm.modules.attention import BasicTransformerBlock
    return BasicTransformerBlock(64, 1, 64, context_dim=32, checkpoint=False, attn_mode="softmax-xformers", image_cross=True, far=2, num_samples=4,
                                 rgb_predict=True, mode="feature-nerf", stratified=True, add_lora=True, **kw)


def _tiny_unet(add_lora=True):
    from make_golden_params import UNET_TINY
    from sgm.modules.diffusionmodules.openaimodel import UNetModel
    return UNetModel(**{**UNET_TINY, "add_lora": add_lora})


def test_state_dict_keys_shapes_and_order_match_reference():
    with gzip.open(os.path.join(GOLD, "block_lora.keys.json.gz"), "rt") as f:
        want = json.load(f)
    got = {k: list(v.shape) for k, v in _block().state_dict().items()}
    assert list(got) == list(want) and got == want
    assert all(k in got for k in ADAPTERS)
    assert got["attn1.to_q_attn3_down.weight"] == [32, 64] and got["attn2.to_k_attn3_down.weight"] == [32, 32]
    assert got["attn2.to_o_attn3_up.weight"] == [64, 32]


def test_adapter_init_is_the_references():
    torch.manual_seed(0)
    from sgm.modules.attention import MemoryEfficientCrossAttention
    a = MemoryEfficientCrossAttention(1280, context_dim=2048, heads=20, add_lora=True)
    for w in "qkvo":
        assert torch.count_nonzero(getattr(a, f"to_{w}_attn3_up").weight) == 0
        d = getattr(a, f"to_{w}_attn3_down").weight
        assert abs(d.std().item() - 1 / 32) < 1e-3 and abs(d.mean().item()) < 1e-3
        assert getattr(a, f"dropout{w}").p == 0.1
    assert not hasattr(MemoryEfficientCrossAttention(64, add_lora=False), "to_q_attn3_down")


def test_adapter_sites_are_distinct_per_block_and_attention():
    b1, b2 = _block(), _block()
    sites = [b.attn1._lora_site for b in (b1, b2)] + [b.attn2._lora_site for b in (b1, b2)]
    assert len(set(sites)) == 4 and b1.attn2._lora_site == b1.attn1._lora_site + 4 and b1.attn1._lora_site % 8 == 0


def test_select_trainable_and_param_groups_take_the_adapters_under_poseattn():
    net = _tiny_unet()
    names = [n for n, _ in net.named_parameters()]
    adapters = [n for n in names if "_attn3_" in n]
    assert adapters and all(".transformer_blocks.0." in n for n in adapters)  # only the pose blocks carry them (attention.py:775)
    pa = finetune.select_trainable(net, "poseattn")
    assert set(adapters) <= set(pa)
    assert not set(adapters) & set(finetune.select_trainable(net, "pose"))
    g = finetune.optimizer_param_groups(net, "poseattn", lr=1e-4, multiplier=0.05)
    assert set(adapters) <= set(g[1]["names"]) and not set(adapters) & set(g[0]["names"])
    assert abs(g[1]["lr"] - 5e-6) < 1e-12
    finetune.select_trainable(net, "poseattn")
    opt = finetune.MasterAdamW(finetune.optimizer_param_groups(net, "poseattn", lr=1e-4), lr=1e-4)
    assert len(opt.params) == len(pa)


def test_delta_checkpoint_carries_no_adapters_and_the_full_state_dict_does():
    import weights as W
    src, dst = _tiny_unet(), _tiny_unet()
    W.load_into(src, seed=8)
    W.load_into(dst, seed=9)
    full = src.state_dict()
    delta = finetune.delta_state_dict({"model.diffusion_model." + k: v for k, v in full.items()})
    assert not any("_attn3_" in k for k in delta)  # main.py:611-625 keeps pose / references only: reproduced as it is
    dst.load_state_dict(full)
    for k, v in dst.state_dict().items():
        if "_attn3_" in k:
            assert torch.equal(v, full[k]), k
    assert any("_attn3_up" in k and v.abs().max() > 0 for k, v in full.items())


def test_lowrank_entry_points_are_declared_and_typed():
    import re
    from cd360 import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "cd360_hip.h")).read()
    for name in ("cd360_lowrank_add_bf16", "cd360_dropout_apply_bf16", "cd360_dropout_tick"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES
    lib = _lib.load()
    # argument checks on the host side of the ABI (no launch): r outside {16, 32, 64}, N % 16, p outside [0, 1)
    assert lib.cd360_lowrank_add_bf16(None, 0, None, 32, None, 32, None, 640, 8, 640, 32, 0.0, None, 0, None) == -1
    fake = 1 << 20  # an aligned non-null address: every call below is refused before anything touches it
    assert lib.cd360_lowrank_add_bf16(None, 0, fake, 48, fake, 48, fake, 640, 8, 640, 48, 0.0, None, 0, None) == -2
    assert lib.cd360_lowrank_add_bf16(None, 0, fake, 32, fake, 32, fake, 648, 8, 648, 32, 0.0, None, 0, None) == -2
    assert lib.cd360_lowrank_add_bf16(None, 0, fake, 32, fake, 32, fake, 640, 8, 640, 32, 1.0, fake, 0, None) == -1
    assert lib.cd360_lowrank_add_bf16(None, 0, fake, 32, fake, 32, fake, 640, 8, 640, 32, 0.1, None, 0, None) == -1
    assert lib.cd360_dropout_apply_bf16(fake, 644, fake, 644, 8, 644, 0.1, fake, 0, None) == -2
