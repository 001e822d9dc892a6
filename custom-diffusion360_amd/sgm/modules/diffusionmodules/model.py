"""The first stage's autoencoder network (reference sgm/modules/diffusionmodules/model.py) on the HIP kernels: `Decoder` serves
`AutoencoderKL.decode` (sgm/models/autoencoder.py:295-296, diffusion.py:208-212) and `Encoder` serves `AutoencoderKL.encode`
(encode_first_stage, diffusion.py:238-248), so neither needs xformers.

Constructors, attribute names and state_dict keys are the reference's, so checkpoints load unchanged.  Activations travel between the
submodules as NCHW-shaped bf16 tensors in torch.channels_last memory format -- physically the channels-last rows [N, H W, C] the kernels
read and write, no copy -- and every forward keeps the reference's call contract (NCHW in, NCHW out; a forward hook sees real values).
A submodule called on its own with another dtype or layout converts its input once.  Kernel map:

  ResnetBlock       gn_silu -> conv 3x3 (emits the GroupNorm slab sums) -> gn_silu on those sums -> conv 3x3 + residual
                    (x, or the nin_shortcut 1x1 / conv_shortcut 3x3 output when in != out)
  Attn blocks       GroupNorm -> ONE q|k|v 1x1 GEMM (q rows prescaled) -> cd360_attn_single_bf16 -> proj_out 1x1 + residual x
  Upsample          cd360_conv_up2x_bf16 (nearest 2x folded into four 2x2-tap phases)
  Downsample        cd360_vae_downsample_bf16 (pad (0, 1, 0, 1) + 3x3 / stride 2; emits the next norm1's GroupNorm slab sums)
  Decoder ends      cd360_vae_conv_in_f32 (fp32 NCHW latent in) and norm_out + SiLU -> cd360_vae_conv_out_bf16 (fp32 NCHW out), or, for
                    forward_u8, -> cd360_vae_conv_out_u8 (the uint8 HWC image)
  Encoder ends      cd360_vae_conv_in_f32 (fp32 NCHW image in) and norm_out + SiLU -> cd360_vae_enc_conv_out_bf16 (fp32 NCHW moments)

Packed weights are cached per module by cd360.derived.derived: its docstring states when they are rebuilt, and the one edit it cannot see.
Forward only: a call autograd would have to record raises (decode_first_stage and encode_first_stage run under no_grad)."""
from __future__ import annotations

import torch
import torch.nn as nn

from cd360 import ops
from cd360.derived import derived
from .util import _tagged_gn_stats, tag_gn_stats

_INT32_BYTES = 2 ** 31  # the convolution cores address one operand with 32-bit byte offsets (cd360_conv_igemm_bf16)


def nonlinearity(x):
    # swish
    return x * torch.sigmoid(x)


def Normalize(in_channels, num_groups=32):
    return torch.nn.GroupNorm(num_groups=num_groups, num_channels=in_channels, eps=1e-6, affine=True)


# ----------------------------------------------------------------------------------------------- layout / cache helpers
def _check_no_grad(mod: nn.Module) -> None:
    if torch.is_grad_enabled() and any(p.requires_grad for p in mod.parameters()):
        raise NotImplementedError("the first-stage HIP modules have no backward; call them under torch.no_grad() (decode_first_stage does)")


def _rows(x: torch.Tensor):
    """NCHW-shaped x -> (channels-last bf16 rows [N, H W, C], N, C, H, W); converts once unless x already is bf16 channels_last on the GPU."""
    if not x.is_cuda:
        raise ops.Cd360Error("the first-stage HIP modules run only on the GPU; got a CPU tensor")
    n, c, h, w = x.shape
    if x.dtype != torch.bfloat16 or not x.is_contiguous(memory_format=torch.channels_last):
        x = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    return x.permute(0, 2, 3, 1).reshape(n, h * w, c), n, c, h, w


def _nchw(rows: torch.Tensor, n: int, h: int, w: int) -> torch.Tensor:
    """[N, H W, C] contiguous rows -> the NCHW-shaped channels_last view of the same memory."""
    return rows.view(n, h, w, rows.shape[-1]).permute(0, 3, 1, 2)


def _gn(norm: nn.GroupNorm, rows: torch.Tensor, silu: bool, tile_stats=None, out=None) -> torch.Tensor:
    return ops.gn_silu(rows, ops.bias_f32(norm.weight), ops.bias_f32(norm.bias), norm.num_groups, norm.eps, silu, out=out, tile_stats=tile_stats)


def _conv_pack(conv: nn.Conv2d):
    return ops.pack_conv_weight(conv.weight), ops.bias_f32(conv.bias).clone() if conv.bias is not None else None


def _ends_pack(net: nn.Module, pack_out):
    """(conv_in weight, bias, conv_out weight, bias) of an Encoder / Decoder as its two end kernels read them."""
    ci, co = net.conv_in, net.conv_out
    return derived(net, "_cd360_pack", (ci.weight, ci.bias, co.weight, co.bias), lambda: (
        ops.pack_vae_conv_in_weight(ci.weight), ops.bias_f32(ci.bias).clone(), pack_out(co.weight), ops.bias_f32(co.bias).clone()))


# ----------------------------------------------------------------------------------------------- blocks
class Upsample(nn.Module):
    def __init__(self, in_channels, with_conv):
        super().__init__()
        self.with_conv = with_conv
        if self.with_conv:
            self.conv = torch.nn.Conv2d(in_channels, in_channels, kernel_size=3, stride=1, padding=1)

    def _pack(self):
        return derived(self, "_cd360_pack", (self.conv.weight, self.conv.bias),
                       lambda: (ops.pack_upsample_conv_weight(self.conv.weight), ops.bias_f32(self.conv.bias).clone()))

    def forward(self, x):
        if not self.with_conv:
            raise NotImplementedError("Upsample(with_conv=False) is not used by the first stage (resamp_with_conv=True)")
        _check_no_grad(self)
        rows, n, c, h, w = _rows(x)
        wph, b = self._pack()
        return _nchw(ops.conv_up2x(rows, wph, b, n, h, w), n, 2 * h, 2 * w)


class Downsample(nn.Module):
    def __init__(self, in_channels, with_conv):
        super().__init__()
        self.with_conv = with_conv
        if self.with_conv:
            # no asymmetric padding in torch conv, must do it ourselves
            self.conv = torch.nn.Conv2d(in_channels, in_channels, kernel_size=3, stride=2, padding=0)

    def _pack(self):
        return derived(self, "_cd360_pack", (self.conv.weight, self.conv.bias), lambda: _conv_pack(self.conv))

    def forward(self, x):
        if not self.with_conv:
            raise NotImplementedError("Downsample(with_conv=False) is not used by the first stage (resamp_with_conv=True)")
        _check_no_grad(self)
        rows, n, c, h, w = _rows(x)
        wp, b = self._pack()
        out, st = ops.vae_downsample(rows, wp, b, n, h, w)
        return tag_gn_stats(_nchw(out, n, h // 2, w // 2), st)


class ResnetBlock(nn.Module):
    def __init__(self, *, in_channels, out_channels=None, conv_shortcut=False, dropout, temb_channels=512):
        super().__init__()
        self.in_channels = in_channels
        out_channels = in_channels if out_channels is None else out_channels
        self.out_channels = out_channels
        self.use_conv_shortcut = conv_shortcut

        self.norm1 = Normalize(in_channels)
        self.conv1 = torch.nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1)
        if temb_channels > 0:
            self.temb_proj = torch.nn.Linear(temb_channels, out_channels)
        self.norm2 = Normalize(out_channels)
        self.dropout = torch.nn.Dropout(dropout)
        self.conv2 = torch.nn.Conv2d(out_channels, out_channels, kernel_size=3, stride=1, padding=1)
        if self.in_channels != self.out_channels:
            if self.use_conv_shortcut:
                self.conv_shortcut = torch.nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1)
            else:
                self.nin_shortcut = torch.nn.Conv2d(in_channels, out_channels, kernel_size=1, stride=1, padding=0)

    def _shortcut(self):
        if self.in_channels == self.out_channels:
            return None
        return self.conv_shortcut if self.use_conv_shortcut else self.nin_shortcut

    def _packs(self):
        sc = self._shortcut()
        convs = (self.conv1, self.conv2) + ((sc,) if sc is not None else ())
        return derived(self, "_cd360_pack", [p for m in convs for p in (m.weight, m.bias)], lambda: [_conv_pack(m) for m in convs])

    def forward(self, x, temb=None, **kwargs):
        if temb is not None:
            raise NotImplementedError("ResnetBlock with a time embedding (Model); the first stage passes temb=None")
        if self.training and self.dropout.p > 0:
            raise NotImplementedError("ResnetBlock dropout > 0 in train mode (the first stage's config has dropout 0)")
        _check_no_grad(self)
        rows, n, c, h, w = _rows(x)
        sc, packs = self._shortcut(), self._packs()
        hid = _gn(self.norm1, rows, True, tile_stats=_tagged_gn_stats(x))
        if (h * w) % 128 == 0:
            hid, st = ops.conv_igemm(hid, packs[0][0], packs[0][1], n, h, w, 9, want_stats=True)
        else:
            hid, st = ops.conv_igemm(hid, packs[0][0], packs[0][1], n, h, w, 9), None
        hid = _gn(self.norm2, hid, True, tile_stats=st, out=hid)
        skip = rows
        if sc is not None:
            skip = ops.conv_igemm(rows, packs[2][0], packs[2][1], n, h, w, 1 if sc.kernel_size == (1, 1) else 9)
        return _nchw(ops.conv_igemm(hid, packs[1][0], packs[1][1], n, h, w, 9, res=skip), n, h, w)


class _SingleHeadAttn(nn.Module):
    """AttnBlock / MemoryEfficientAttnBlock: the same arithmetic (single-head softmax(q k^T / sqrt(C)) v over all pixels) and kernels."""

    def __init__(self, in_channels):
        super().__init__()
        self.in_channels = in_channels

        self.norm = Normalize(in_channels)
        self.q = torch.nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.k = torch.nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.v = torch.nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.proj_out = torch.nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)

    def _pack(self):
        def make():
            wqkv, bqkv = ops.pack_attn_qkv(self.q.weight, self.q.bias, self.k.weight, self.k.bias, self.v.weight, self.v.bias)
            return wqkv, bqkv, self.proj_out.weight.detach().reshape(self.in_channels, -1).to(torch.bfloat16).contiguous(), \
                ops.bias_f32(self.proj_out.bias).clone()
        return derived(self, "_cd360_pack", [p for m in (self.q, self.k, self.v, self.proj_out) for p in (m.weight, m.bias)], make)

    def forward(self, x, **kwargs):
        _check_no_grad(self)
        rows, n, c, h, w = _rows(x)
        wqkv, bqkv, wp, bp = self._pack()
        hid = _gn(self.norm, rows, False)
        qkv = ops.conv_igemm(hid, wqkv, bqkv, n, h, w, 1)  # [n, h w, 3 c]
        att = ops.attention_single(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:])
        return _nchw(ops.conv_igemm(att, wp, bp, n, h, w, 1, res=rows), n, h, w)


class AttnBlock(_SingleHeadAttn):
    pass


class MemoryEfficientAttnBlock(_SingleHeadAttn):
    """The reference's xformers block (model.py:204-265); here the same kernels as AttnBlock."""

    def __init__(self, in_channels):
        super().__init__(in_channels)
        self.attention_op = None


def make_attn(in_channels, attn_type="vanilla", attn_kwargs=None):
    assert attn_type in ["vanilla", "vanilla-xformers", "memory-efficient-cross-attn", "linear", "none"], f"attn_type {attn_type} unknown"
    if attn_type == "vanilla":
        assert attn_kwargs is None
        return AttnBlock(in_channels)
    if attn_type == "vanilla-xformers":
        return MemoryEfficientAttnBlock(in_channels)
    if attn_type == "none":
        return nn.Identity(in_channels)
    raise NotImplementedError(f"attn_type {attn_type!r} is not used by the first stage's config (vanilla-xformers); not implemented")


# ----------------------------------------------------------------------------------------------- encoder / decoder
class Encoder(nn.Module):
    def __init__(self, *, ch, out_ch, ch_mult=(1, 2, 4, 8), num_res_blocks, attn_resolutions, dropout=0.0, resamp_with_conv=True,
                 in_channels, resolution, z_channels, double_z=True, use_linear_attn=False, attn_type="vanilla", **ignore_kwargs):
        super().__init__()
        if use_linear_attn:
            attn_type = "linear"
        self.ch = ch
        self.temb_ch = 0
        self.num_resolutions = len(ch_mult)
        self.num_res_blocks = num_res_blocks
        self.resolution = resolution
        self.in_channels = in_channels

        self.conv_in = torch.nn.Conv2d(in_channels, self.ch, kernel_size=3, stride=1, padding=1)

        curr_res = resolution
        in_ch_mult = (1,) + tuple(ch_mult)
        self.in_ch_mult = in_ch_mult
        self.down = nn.ModuleList()
        for i_level in range(self.num_resolutions):
            block = nn.ModuleList()
            attn = nn.ModuleList()
            block_in = ch * in_ch_mult[i_level]
            block_out = ch * ch_mult[i_level]
            for i_block in range(self.num_res_blocks):
                block.append(ResnetBlock(in_channels=block_in, out_channels=block_out, temb_channels=self.temb_ch, dropout=dropout))
                block_in = block_out
                if curr_res in attn_resolutions:
                    attn.append(make_attn(block_in, attn_type=attn_type))
            down = nn.Module()
            down.block = block
            down.attn = attn
            if i_level != self.num_resolutions - 1:
                down.downsample = Downsample(block_in, resamp_with_conv)
                curr_res = curr_res // 2
            self.down.append(down)

        self.mid = nn.Module()
        self.mid.block_1 = ResnetBlock(in_channels=block_in, out_channels=block_in, temb_channels=self.temb_ch, dropout=dropout)
        self.mid.attn_1 = make_attn(block_in, attn_type=attn_type)
        self.mid.block_2 = ResnetBlock(in_channels=block_in, out_channels=block_in, temb_channels=self.temb_ch, dropout=dropout)

        self.norm_out = Normalize(block_in)
        self.conv_out = torch.nn.Conv2d(block_in, 2 * z_channels if double_z else z_channels, kernel_size=3, stride=1, padding=1)

    def pass_bytes(self, h: int, w: int) -> int:
        """Largest tensor the convolution cores address for one h x w image (every block input / output, each q|k|v projection); it must
        stay below 2^31 bytes.  At the SDXL ddconfig that is the level-0 activation, h w 128 channels of bf16."""
        hw = h * w
        biggest = hw * self.conv_in.out_channels * 2
        for i_level in range(self.num_resolutions):
            down = self.down[i_level]
            for blk in down.block:
                biggest = max(biggest, hw * max(blk.in_channels, blk.out_channels) * 2)
                if len(down.attn) > 0:
                    biggest = max(biggest, hw * 3 * blk.out_channels * 2)
            if i_level != self.num_resolutions - 1:
                h, w = h // 2, w // 2
                hw = h * w
        return max(biggest, hw * 3 * self.mid.block_1.out_channels * 2)

    def forward(self, x):
        if not x.is_cuda:
            raise NotImplementedError("Encoder.forward runs on the HIP kernels only; got a host tensor")
        _check_no_grad(self)
        # one image per pass, as in Decoder.forward: an image encodes to the same bits in a batch of any size (the target x and the
        # references xr of shared_step call this with different batch sizes)
        if x.shape[0] == 1:
            return self._encode_pass(x)
        return torch.cat([self._encode_pass(x[i:i + 1]) for i in range(x.shape[0])], 0)

    def _encode_pass(self, x):
        n, cin, h, w = x.shape
        if self.pass_bytes(h, w) >= _INT32_BYTES:
            raise ops.Cd360Error(f"an image of {h} x {w} exceeds the 32-bit offsets of the convolution cores")
        temb = None

        win, bin_, wout, bout = _ends_pack(self, ops.pack_vae_enc_conv_out_weight)
        x32 = x.float().contiguous()
        if (h * w) % 64 == 0:
            rows, st = ops.vae_conv_in(x32, win, bin_, want_stats=True)
        else:
            rows, st = ops.vae_conv_in(x32, win, bin_), None
        hid = tag_gn_stats(_nchw(rows, n, h, w), st)

        # the reference keeps every level's output in a list `hs`; only its last entry is ever read
        for i_level in range(self.num_resolutions):
            for i_block in range(self.num_res_blocks):
                hid = self.down[i_level].block[i_block](hid, temb)
                if len(self.down[i_level].attn) > 0:
                    hid = self.down[i_level].attn[i_block](hid)
            if i_level != self.num_resolutions - 1:
                hid = self.down[i_level].downsample(hid)

        hid = self.mid.block_1(hid, temb)
        hid = self.mid.attn_1(hid)
        hid = self.mid.block_2(hid, temb)

        rows, n, c, hh, ww = _rows(hid)
        act = _gn(self.norm_out, rows, True)
        out = ops.vae_enc_conv_out(act, wout, bout, n, hh, ww, self.conv_out.out_channels)
        return out.to(self.conv_out.weight.dtype)


class Decoder(nn.Module):
    def __init__(self, *, ch, out_ch, ch_mult=(1, 2, 4, 8), num_res_blocks, attn_resolutions, dropout=0.0, resamp_with_conv=True,
                 in_channels, resolution, z_channels, give_pre_end=False, tanh_out=False, use_linear_attn=False, attn_type="vanilla",
                 **ignorekwargs):
        super().__init__()
        if use_linear_attn:
            attn_type = "linear"
        self.ch = ch
        self.temb_ch = 0
        self.num_resolutions = len(ch_mult)
        self.num_res_blocks = num_res_blocks
        self.resolution = resolution
        self.in_channels = in_channels
        self.give_pre_end = give_pre_end
        self.tanh_out = tanh_out

        block_in = ch * ch_mult[self.num_resolutions - 1]
        curr_res = resolution // 2 ** (self.num_resolutions - 1)
        self.z_shape = (1, z_channels, curr_res, curr_res)

        make_attn_cls = self._make_attn()
        make_resblock_cls = self._make_resblock()
        make_conv_cls = self._make_conv()
        self.conv_in = torch.nn.Conv2d(z_channels, block_in, kernel_size=3, stride=1, padding=1)

        self.mid = nn.Module()
        self.mid.block_1 = make_resblock_cls(in_channels=block_in, out_channels=block_in, temb_channels=self.temb_ch, dropout=dropout)
        self.mid.attn_1 = make_attn_cls(block_in, attn_type=attn_type)
        self.mid.block_2 = make_resblock_cls(in_channels=block_in, out_channels=block_in, temb_channels=self.temb_ch, dropout=dropout)

        self.up = nn.ModuleList()
        for i_level in reversed(range(self.num_resolutions)):
            block = nn.ModuleList()
            attn = nn.ModuleList()
            block_out = ch * ch_mult[i_level]
            for i_block in range(self.num_res_blocks + 1):
                block.append(make_resblock_cls(in_channels=block_in, out_channels=block_out, temb_channels=self.temb_ch, dropout=dropout))
                block_in = block_out
                if curr_res in attn_resolutions:
                    attn.append(make_attn_cls(block_in, attn_type=attn_type))
            up = nn.Module()
            up.block = block
            up.attn = attn
            if i_level != 0:
                up.upsample = Upsample(block_in, resamp_with_conv)
                curr_res = curr_res * 2
            self.up.insert(0, up)  # prepend to get consistent order

        self.norm_out = Normalize(block_in)
        self.conv_out = make_conv_cls(block_in, out_ch, kernel_size=3, stride=1, padding=1)

    def _make_attn(self):
        return make_attn

    def _make_resblock(self):
        return ResnetBlock

    def _make_conv(self):
        return torch.nn.Conv2d

    def get_last_layer(self, **kwargs):
        return self.conv_out.weight

    def max_batch(self, h: int, w: int) -> int:
        """Images of an h x w latent that could share one pass: every activation the convolution cores read (and every q|k|v
        projection / Upsample output they write) stays below 2^31 bytes.  forward() decodes one image per pass (see there)."""
        hw, biggest = h * w, 0
        c = self.conv_in.out_channels

        def see(pixels, channels):
            nonlocal biggest
            biggest = max(biggest, pixels * channels * 2)

        see(hw, c)
        see(hw, 3 * c)  # mid.attn_1's q|k|v
        for i_level in reversed(range(self.num_resolutions)):
            up = self.up[i_level]
            for i_block, blk in enumerate(up.block):
                see(hw, blk.in_channels)
                see(hw, blk.out_channels)
                if len(up.attn) > 0:
                    see(hw, 3 * blk.out_channels)
            if i_level != 0:
                hw *= 4
                see(hw, up.upsample.conv.out_channels)
        return max(1, (_INT32_BYTES - 1) // biggest)

    def forward(self, z, **kwargs):
        self.last_z_shape = z.shape
        if self.give_pre_end or self.tanh_out:
            raise NotImplementedError("Decoder(give_pre_end=True | tanh_out=True) is not used by the first stage; not implemented")
        _check_no_grad(self)
        if not z.is_cuda:
            raise ops.Cd360Error("the first-stage HIP modules run only on the GPU; got a CPU tensor")
        # one image per pass: an image decodes to the same bits in a batch of any size.  A batch-folded pass (_decode_pass on the whole
        # batch, legal up to max_batch(h, w) images) lets the convolution cores pick their tiling from the batch's pixel count, which
        # changes fp32 summation orders and so the bf16 roundings downstream; at a 1024^2 image one image already fills the chip
        if z.shape[0] == 1:
            return self._decode_pass(z, **kwargs)
        return torch.cat([self._decode_pass(z[i:i + 1], **kwargs) for i in range(z.shape[0])], 0)

    @torch.no_grad()
    def forward_u8(self, z, **kwargs):
        """forward(z) with the image epilogue of sample.py:346 in the last kernel: [N, H, W, out_ch] uint8 (channels last, what
        Image.fromarray takes) = (clip(forward(z) * 0.5 + 0.5, 0, 1) * 255).to(uint8) bit for bit when the parameters are fp32, without the
        fp32 image ever reaching memory (cd360_vae_conv_out_u8).  One image per pass, as forward."""
        self.last_z_shape = z.shape
        if self.give_pre_end or self.tanh_out:
            raise NotImplementedError("Decoder(give_pre_end=True | tanh_out=True) is not used by the first stage; not implemented")
        if not z.is_cuda:
            raise ops.Cd360Error("the first-stage HIP modules run only on the GPU; got a CPU tensor")
        outs = []
        for i in range(z.shape[0]):
            act, n, hh, ww, wout, bout = self._decode_trunk(z[i:i + 1], **kwargs)
            outs.append(ops.vae_conv_out_u8(act, wout, bout, n, hh, ww, self.conv_out.out_channels))
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)

    def _decode_pass(self, z, **kwargs):
        """One pass of the decoder over the whole batch z (at most max_batch(h, w) images)."""
        act, n, hh, ww, wout, bout = self._decode_trunk(z, **kwargs)
        out = ops.vae_conv_out(act, wout, bout, n, hh, ww, self.conv_out.out_channels)
        return out.to(self.conv_out.weight.dtype)

    def _decode_trunk(self, z, **kwargs):
        """Everything of one pass in front of conv_out: -> (norm_out + SiLU rows [n, H W, C] bf16, n, H, W, conv_out's packed weight, bias)."""
        n, cz, h, w = z.shape
        if n > self.max_batch(h, w):
            raise ops.Cd360Error(f"{n} images of {h} x {w} exceed the 32-bit offsets of the convolution cores in one pass")
        temb = None

        win, bin_, wout, bout = _ends_pack(self, ops.pack_vae_conv_out_weight)
        z32 = z.float().contiguous()
        if (h * w) % 64 == 0:
            rows, st = ops.vae_conv_in(z32, win, bin_, want_stats=True)
        else:
            rows, st = ops.vae_conv_in(z32, win, bin_), None
        hid = tag_gn_stats(_nchw(rows, n, h, w), st)

        hid = self.mid.block_1(hid, temb, **kwargs)
        hid = self.mid.attn_1(hid, **kwargs)
        hid = self.mid.block_2(hid, temb, **kwargs)

        for i_level in reversed(range(self.num_resolutions)):
            for i_block in range(self.num_res_blocks + 1):
                hid = self.up[i_level].block[i_block](hid, temb, **kwargs)
                if len(self.up[i_level].attn) > 0:
                    hid = self.up[i_level].attn[i_block](hid, **kwargs)
            if i_level != 0:
                hid = self.up[i_level].upsample(hid)

        rows, n, c, hh, ww = _rows(hid)
        return _gn(self.norm_out, rows, True), n, hh, ww, wout, bout
