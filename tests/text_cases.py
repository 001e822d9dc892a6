"""What tests/test_text_cpu.py and tests/test_text_gpu.py share (plain helper module, like optim_cases.py; no tests, no fixtures): the names
include/text/cd360_text.h adds (the library's entry in sampler_cases.LIBRARIES, where the header / table / library rule is stated), the
small architectures, and builders of the embedders next to their tests/text_fp32.py reference on one state dict."""
import json
import os

import torch

import sampler_cases as SC
import text_fp32 as T32

LIBRARY = 3  # in SC.LIBRARIES
NEW = SC.LIBRARIES[LIBRARY][3]
HEADER = os.path.join("text", "cd360_text.h")
KERNELS = ("text_embed_kernel", "text_causal_attn_kernel", "text_act_kernel", "text_eot_pool_kernel")
# the guarded cases of tests/test_text_gpu.py::test_text_entry_points_write_their_outputs_only: (id, entry points the case must reach)
GUARDED = [("embed-stats", ["cd360_text_embed_bf16"]), ("causal-attn-merged", ["cd360_text_causal_attn_bf16"]),
           ("act-both-kinds", ["cd360_text_act_bf16"]), ("eot-pool", ["cd360_text_eot_pool_bf16"])]
# the small towers: head dim 64 (the HIP route's), three layers so that a first, a middle and a last layer exist, 77 tokens
SMALL = dict(vocab=96, width=128, heads=2, layers=3, mlp=512, proj=128)
# the real widths, one layer each
CLIP_L = dict(vocab=96, width=768, heads=12, layers=1, mlp=3072, proj=768)
BIG_G = dict(vocab=96, width=1280, heads=20, layers=1, mlp=5120, proj=1280)


# ------------------------------------------------------------------------------------------------ embedders and their references
def clip_arch(a=SMALL):
    return dict(vocab_size=a["vocab"], width=a["width"], heads=a["heads"], layers=a["layers"], mlp_width=a["mlp"])


def openclip_arch(a=SMALL):
    return dict(clip_arch(a), proj_dim=a["proj"])


def _count(modifier):
    return 0 if modifier is None else modifier.count("+") + 1


def clip_embedder(modifier, arch=SMALL, layer="hidden", layer_idx=11, **kw):
    from sgm.modules.encoders.modules import FrozenCLIPEmbedder
    return FrozenCLIPEmbedder(modifier_token=modifier, layer=layer, layer_idx=layer_idx, **clip_arch(arch), **kw)


def openclip_embedder(modifier, arch=SMALL, layer="penultimate", always_return_pooled=True, legacy=False, **kw):
    from sgm.modules.encoders.modules import FrozenOpenCLIPEmbedder
    return FrozenOpenCLIPEmbedder(modifier_token=modifier, layer=layer, always_return_pooled=always_return_pooled, legacy=legacy,
                                  **openclip_arch(arch), **kw)


def clip_pair(modifier, seed, arch=SMALL, **kw):
    """(embedder, text_fp32 tower, state dict): both hold the same deterministic fp32 weights, the token table grown by the modifier rows."""
    emb = clip_embedder(modifier, arch, **kw)
    ref = T32.HFTextTower(arch["vocab"] + _count(modifier), arch["width"], arch["heads"], arch["layers"], arch["mlp"]).eval()
    sd = T32.synth_weights(ref, seed)
    ref.load_state_dict(sd, strict=True)
    emb.load_state_dict(sd, strict=True)
    return emb, ref, sd


def openclip_pair(modifier, seed, arch=SMALL, **kw):
    emb = openclip_embedder(modifier, arch, **kw)
    ref = T32.OpenCLIPTextTower(arch["vocab"] + _count(modifier), arch["width"], arch["heads"], arch["layers"], arch["mlp"], arch["proj"]).eval()
    sd = T32.synth_weights(ref, seed)
    ref.load_state_dict(sd, strict=True)
    emb.load_state_dict(sd, strict=True)
    return emb, ref, sd


def emb_models(modifier="<new1>", arches=(SMALL, SMALL)):
    """The five emb_models of the shipped config (tests/golden/conditioner_emb_models.json holds its settings) with small architecture
    arguments added to the two prompt encoders."""
    cfgs = json.load(open(os.path.join(SC.ROOT, "tests", "golden", "conditioner_emb_models.json")))
    assert len(cfgs) == 5
    for cfg, arch in zip(cfgs[:2], (clip_arch(arches[0]), openclip_arch(arches[1]))):
        assert cfg["params"]["modifier_token"] == "<new1>"
        cfg["params"].update(arch)
        cfg["params"]["modifier_token"] = modifier
    return cfgs


def conditioner(modifier="<new1>", seed=21, arches=(SMALL, SMALL)):
    """sgm.modules.GeneralConditioner, resolved as the YAML resolves it, on deterministic weights."""
    from sgm.util import instantiate_from_config
    cond = instantiate_from_config({"target": "sgm.modules.GeneralConditioner", "params": {"emb_models": emb_models(modifier, arches)}})
    for i, e in enumerate(cond.embedders[:2]):
        e.load_state_dict(T32.synth_weights(e, seed + i), strict=True)
    return cond


def batch(n_target, n_ref, seed=0, device="cpu"):
    """What the data loader hands the conditioner: token ids for `txt` / `txt_ref` (the modifier id inside every prompt) and the three size
    conditionings, for n_target target rows and n_ref reference views."""
    V = SMALL["vocab"]
    out = {}
    for suffix, n, s in (("", n_target, seed), ("_ref", n_ref, seed + 1)):
        out["txt" + suffix] = T32.token_ids(n, V, seed=s, modifier=(V, 5))
        out["original_size_as_tuple" + suffix] = torch.tensor([[512.0, 512.0]]).repeat(n, 1).to(device)
        out["crop_coords_top_left" + suffix] = torch.tensor([[0.0, 16.0 + 8 * len(suffix)]]).repeat(n, 1).to(device)
        out["target_size_as_tuple" + suffix] = torch.tensor([[512.0, 384.0]]).repeat(n, 1).to(device)
    return out
