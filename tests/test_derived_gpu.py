"""Every site that caches derived weights through cd360.derived.derived, on the GPU in bf16: after each thing that can happen to a source
parameter (tests/derived_cases.py) the site's pack is rebuilt and equals, tensor for tensor, the pack of a freshly constructed module
holding the same parameters.  Only the pack accessors are called, no forward: torch's own copy kernels are all that runs."""
import pytest
import torch
import torch.nn as nn

import derived_cases as DC

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _block():
    from sgm.modules.attention import BasicTransformerBlock
    return BasicTransformerBlock(128, 2, 64, context_dim=64, checkpoint=False, attn_mode="softmax-xformers", image_cross=True, far=2, num_samples=6,
                                 rgb_predict=True, mode="feature-nerf", stratified=True)


def _attn(lora):
    from sgm.modules.attention import MemoryEfficientCrossAttention
    return lambda: MemoryEfficientCrossAttention(128, heads=2, dim_head=64, add_lora=lora)


def _out_holder():
    holder = nn.Module()
    holder.out = nn.Sequential(nn.Identity(), nn.Identity(), nn.Conv2d(64, 4, 3, padding=1))
    return holder


def _spatial():
    from sgm.modules.attention import SpatialTransformer
    return SpatialTransformer(128, 2, 64, depth=1, context_dim=64, use_linear=True, use_checkpoint=False, image_cross=False)


def _vae(name, *a, **kw):
    def make():
        from sgm.modules.diffusionmodules import model
        return getattr(model, name)(*a, **kw)
    return make


_TINY_DD = dict(ch=64, out_ch=3, ch_mult=[1], num_res_blocks=1, attn_resolutions=[], in_channels=3, resolution=8, z_channels=4, double_z=True)


def _ends(pack_out):
    def pack(net):
        from cd360 import ops
        from sgm.modules.diffusionmodules import model
        return model._ends_pack(net, getattr(ops, pack_out))
    return pack


def _unet_up():
    from sgm.modules.diffusionmodules.openaimodel import Upsample
    return Upsample(64, True)


def _nerf_encoding():
    from sgm.modules.nerfsd_pytorch3d import FeatureNeRFEncoding
    return FeatureNeRFEncoding(64, 64, rgb_predict=True)


def _util(name):
    def pack(conv):
        from sgm.modules.diffusionmodules import util
        return getattr(util, name)(conv)
    return pack


def _out4(holder):
    from sgm.modules.diffusionmodules.openaimodel import UNetModel
    return UNetModel._out_conv4_pack(holder)


_FROZEN = ("qkv", "o1", "q2", "o2", "ff1", "ff2")  # BasicTransformerBlock._packed: these keys in one slot, "pose" in a slot of its own

# name -> (constructor, pack accessor, the source parameters to disturb as (path of the submodule, attribute[, the keys of the pack that
# share a slot with this parameter]): one weight, and one bias where the site has one)
SITES = {
    "packed_conv": (lambda: nn.Conv2d(64, 64, 3, padding=1), _util("packed_conv"), [("", "weight"), ("", "bias")]),
    "packed_conv_dgrad": (lambda: nn.Conv2d(64, 64, 3, padding=1), _util("packed_conv_dgrad"), [("", "weight")]),
    "upsample_phase_weights": (_unet_up, lambda m: m._phase_weights(), [("conv", "weight"), ("conv", "bias")]),
    "out_conv4_pack": (_out_holder, _out4, [("out.2", "weight"), ("out.2", "bias")]),
    "merged_qkv": (_attn(False), lambda m: m._merged_weight("qkv"), [("to_k", "weight")]),
    "merged_kv": (_attn(False), lambda m: m._merged_weight("kv"), [("to_v", "weight")]),
    "merged_qkv_lora": (_attn(True), lambda m: m._merged_weight("qkv"), [("to_k", "weight"), ("to_q_attn3_up", "weight")]),
    "merged_kv_lora": (_attn(True), lambda m: m._merged_weight("kv"), [("to_v", "weight"), ("to_k_attn3_down", "weight")]),
    "block_packed": (_block, lambda m: m._packed(), [("attn1.to_q", "weight", _FROZEN), ("ff.net.2", "bias", _FROZEN), ("pose_emb_layers", "weight", ("pose",))]),
    "spatial_proj_pack": (_spatial, lambda m: m._proj_pack(), [("proj_in", "weight"), ("proj_out", "bias")]),
    "nerf_fused_weights": (_nerf_encoding, lambda m: m.fused_weights(), [("plane_coefs.0", "weight"), ("plane_coefs.2", "bias")]),
    "vae_resnet_packs": (_vae("ResnetBlock", in_channels=64, out_channels=128, dropout=0.0, temb_channels=0), lambda m: m._packs(),
                         [("conv1", "weight"), ("nin_shortcut", "bias")]),
    "vae_attn_pack": (_vae("_SingleHeadAttn", 64), lambda m: m._pack(), [("q", "weight"), ("proj_out", "bias")]),
    "vae_upsample_pack": (_vae("Upsample", 64, True), lambda m: m._pack(), [("conv", "weight"), ("conv", "bias")]),
    "vae_downsample_pack": (_vae("Downsample", 64, True), lambda m: m._pack(), [("conv", "weight"), ("conv", "bias")]),
    "vae_decoder_ends": (_vae("Decoder", **_TINY_DD), _ends("pack_vae_conv_out_weight"), [("conv_in", "weight"), ("conv_out", "bias")]),
    "vae_encoder_ends": (_vae("Encoder", **_TINY_DD), _ends("pack_vae_enc_conv_out_weight"), [("conv_out", "weight"), ("conv_in", "bias")]),
}


def _snap(pack):
    return dict(pack) if isinstance(pack, dict) else pack  # BasicTransformerBlock._packed refills one dict in place


def _on_device(make, state=None):
    """A frozen eval module in bf16 on the device; every parameter random (zero-initialised ones too) unless `state` is given."""
    mod = make().eval().requires_grad_(False)
    if state is None:
        gen = torch.Generator().manual_seed(5)
        with torch.no_grad():
            for p in mod.parameters():
                p.copy_(torch.randn(p.shape, generator=gen) * 0.25 + 0.5)
    mod = mod.to(DEV, BF)
    if state is not None:
        mod.load_state_dict(state)
    return mod


@torch.no_grad()
@pytest.mark.parametrize("site", list(SITES))
def test_pack_follows_its_source_parameters(site):
    make, pack, targets = SITES[site]
    mod = _on_device(make)
    last = _snap(pack(mod))
    assert DC.served(last, pack(mod))
    for path, attr, *parts in targets:
        for mutate in DC.MUTATIONS:
            mutate(mod.get_submodule(path), attr)
            got = _snap(pack(mod))
            if not parts:
                assert DC.rebuilt(last, got), (path, attr, mutate.__name__)
            else:  # the pack is a dict filled from two slots: the named keys are new, the others served
                assert all(DC.rebuilt(last[k], got[k]) if k in parts[0] else got[k] is last[k] for k in last), (path, attr, mutate.__name__)
            fresh = _on_device(make, {k: v.clone() for k, v in mod.state_dict().items()})
            assert DC.same(got, pack(fresh)), (path, attr, mutate.__name__)
            assert DC.served(got, pack(mod)), (path, attr, mutate.__name__)
            last = got


@torch.no_grad()
def test_pose_weight_update_repacks_only_the_pose_half():
    """One fine-tuning step touches pose_emb_layers.weight alone: the frozen packs stay the same objects, "pose" is new."""
    blk = _on_device(_block)
    before = _snap(blk._packed())
    torch.autograd.graph.increment_version(blk.pose_emb_layers.weight)
    after = blk._packed()
    assert set(after) == set(before) == {*_FROZEN, "pose"}
    for k in before:
        if k == "pose":
            assert DC.rebuilt(before[k], after[k]) and DC.same(before[k], after[k])
        else:
            assert after[k] is before[k], k
