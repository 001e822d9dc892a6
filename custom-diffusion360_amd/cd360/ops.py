"""Torch-tensor front end of the C ABI.  torch owns memory and the stream; every call goes to libcd360_hip.so.

No operator here has a PyTorch/CPU implementation: a CPU tensor (or a missing library) raises."""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple, Optional

import torch

from . import _host, _lib, routes
from ._lib import Cd360Error, check

_I64x3 = ctypes.c_int64 * 3


# ----------------------------------------------------------------------------------------------- per-kernel timing
# bench.py brackets every C-ABI launch with HIP events ON THE LAUNCH STREAM (torch's current stream is the stream every
# kernel here is enqueued on) and reads them back after the timed region; off by default (zero overhead).
_PROF = None
_PROF_SHAPES = False


def profile_start(shapes: bool = False) -> None:
    """shapes=True: the GEMM entries are keyed per problem shape ("gemm8p[MxNxK]", "gemm_tn[MxNxK]") instead of per kernel."""
    global _PROF, _PROF_SHAPES
    _PROF, _PROF_SHAPES = [], bool(shapes)


def _shape_tag(name: str, M: int, N: int, K: int) -> str:
    return f"{name}[{M}x{N}x{K}]" if _PROF_SHAPES else name


def profile_stop() -> dict:
    """-> {kernel: {"ms": total, "n": launches, "flops": algorithmic flops, "bytes": algorithmic HBM bytes}} (synchronises)."""
    global _PROF
    rec, _PROF = _PROF or [], None
    torch.cuda.synchronize()
    out = {}
    for name, e0, e1, flops, nbytes in rec:
        d = out.setdefault(name, {"ms": 0.0, "n": 0, "flops": 0.0, "bytes": 0.0})
        d["ms"] += e0.elapsed_time(e1)
        d["n"] += 1
        d["flops"] += flops
        d["bytes"] += nbytes
    return out


class _timed:
    __slots__ = ("name", "flops", "nbytes", "e0")

    def __init__(self, name, flops=0.0, nbytes=0.0):
        self.name, self.flops, self.nbytes = name, flops, nbytes

    def __enter__(self):
        if _PROF is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *a):
        if _PROF is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            _PROF.append((self.name, self.e0, e1, self.flops, self.nbytes))
        return False


# Both helpers return plain Python ints (None for a null pointer): every pointer / stream parameter of the C ABI is typed c_void_p in
# cd360/_lib.py, and ctypes converts an int itself -- building a c_void_p object per argument cost 1.5 us each, 13 000 times per eagerly
# launched fine-tuning step, and `torch.cuda.current_stream().cuda_stream` 9 us per launch (tools/probe/train_host_profile.py: 20 + 21 ms
# of a 147 ms step).  The raw-stream query below is what torch's own extensions use; it follows `torch.cuda.stream(...)` contexts and
# graph captures exactly like current_stream().
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _need_gpu(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise Cd360Error("cd360 operators run only on the GPU (HIP extension); got a CPU tensor")
        if t.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("this cd360 HIP operator has no backward; call it under torch.no_grad()")


def _wants_grad(*ts) -> bool:
    """True when the call must be recorded by autograd: the differentiable operators then go through cd360/grad.py
    (torch.autograd.Function around the forward and backward HIP kernels)."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


# ----------------------------------------------------------------------------------------------- attention
ATTN_PRESCALE = 64 ** -0.5 * 1.4426950408889634  # softmax scale x log2(e): what attention(..., prescaled=True) expects folded into q


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, nk: Optional[int] = None,
              out: Optional[torch.Tensor] = None, want_lse: bool = False, prescaled: bool = False):
    """softmax(q k^T / 8) v per head, projection layouts consumed in place.
    q [b, Nq, H*64], k, v [b, >=Nk, H*64] (last dim contiguous; row / batch strides free, e.g. slices of one merged q|k|v
    projection) -> [b, Nq, H*64].  `nk` limits the keys when k / v are padded.  want_lse=True returns (out, lse [b*H, Nq] fp32),
    the training forward (cd360_attn_fwd_lse_bf16).  Differentiable: under autograd the call is recorded (grad.AttentionFn).
    prescaled=True: q already carries ATTN_PRESCALE (folded into the q projection by the caller; cd360_attn_fwd_prescaled_bf16) --
    forward only."""
    if _wants_grad(q, k, v):
        from . import grad
        assert out is None and not want_lse and not prescaled
        return grad.AttentionFn.apply(q, k, v, heads, nk)
    _need_gpu(q, k, v)
    b, nq, inner = q.shape
    assert inner == heads * 64 and q.dtype == torch.bfloat16 and k.dtype == torch.bfloat16 and v.dtype == torch.bfloat16
    assert q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1 and k.shape[-1] == inner and v.shape[-1] == inner
    nk = k.shape[1] if nk is None else nk
    assert v.shape[1] >= nk and k.shape[1] >= nk
    if out is None:
        out = torch.empty(b, nq, inner, dtype=torch.bfloat16, device=q.device)
    lib = _lib.load()
    strides = (_I64x3(q.stride(0), 64, q.stride(1)), _I64x3(k.stride(0), 64, k.stride(1)),
               _I64x3(v.stride(0), 64, v.stride(1)), _I64x3(out.stride(0), 64, out.stride(1)))
    # self-attention (tiled kernel) and the <= 96-key cross-attention (register-resident kernel) are different kernels: timed apart
    with _timed("attn_self" if nk > 96 else "attn_smallk", 4.0 * b * heads * nq * nk * 64, 2.0 * (2 * b * nq * inner + 2 * b * nk * inner)):
        if prescaled:
            assert not want_lse
            check(lib.cd360_attn_fwd_prescaled_bf16(_ptr(q), _ptr(k), _ptr(v), _ptr(out), b, heads, nq, nk, *strides, _stream()),
                  "cd360_attn_fwd_prescaled_bf16")
            return out
        if want_lse:
            lse = torch.empty(b * heads, nq, dtype=torch.float32, device=q.device)
            check(lib.cd360_attn_fwd_lse_bf16(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(lse), b, heads, nq, nk, *strides, 64 ** -0.5, _stream()),
                  "cd360_attn_fwd_lse_bf16")
            return out, lse
        check(lib.cd360_attn_fwd_bf16(_ptr(q), _ptr(k), _ptr(v), _ptr(out), b, heads, nq, nk, *strides, 64 ** -0.5, _stream()),
              "cd360_attn_fwd_bf16")
    return out


def attention_bwd(q, k, v, o, dout, lse, heads: int, nk: Optional[int] = None, need_dq: bool = True, need_dkv: bool = True, out=None):
    """Backward of attention(..., want_lse=True): (dq | None, dk | None, dv | None), bf16, contiguous, rows >= nk of dk / dv zero.
    out = (dq, dk, dv) writes into caller-provided (possibly strided, last dim contiguous) tensors instead, e.g. the three column
    slices of one d(q|k|v) buffer."""
    _need_gpu(q, k, v, o, dout, lse)
    b, nq, inner = q.shape
    nk = k.shape[1] if nk is None else nk
    if dout.stride(2) != 1 or dout.stride(0) % 8 or dout.stride(1) % 8 or dout.data_ptr() % 16:
        dout = dout.contiguous()
    assert dout.dtype == torch.bfloat16 and dout.shape == q.shape and lse.shape == (b * heads, nq) and lse.dtype == torch.float32
    if out is not None:
        dq, dk, dv = out
        assert all(t.dtype == torch.bfloat16 and t.stride(2) == 1 and t.stride(0) % 4 == 0 and t.stride(1) % 4 == 0 for t in out)
        assert dq.shape == q.shape and dk.shape[1] >= nk and dv.shape[1] >= nk
    else:
        dq = torch.empty(b, nq, inner, dtype=torch.bfloat16, device=q.device) if need_dq else None
        dk = torch.zeros(b, k.shape[1], inner, dtype=torch.bfloat16, device=q.device) if need_dkv else None
        dv = torch.zeros(b, v.shape[1], inner, dtype=torch.bfloat16, device=q.device) if need_dkv else None
    ws = torch.empty(b * heads * nq, dtype=torch.float32, device=q.device)
    s3 = lambda t: None if t is None else _I64x3(t.stride(0), 64, t.stride(1))
    flops = 4.0 * b * heads * nq * nk * 64 * ((1.5 if need_dq else 0.0) + (2.0 if need_dkv else 0.0))
    with _timed("attn_bwd", flops, 2.0 * (4 * b * nq * inner + 4 * b * nk * inner)):
        check(_lib.load().cd360_attn_bwd_bf16(_ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(dout), _ptr(lse), _ptr(dq), _ptr(dk), _ptr(dv), _ptr(ws),
                                             b, heads, nq, nk, s3(q), s3(k), s3(v), s3(o), s3(dout), s3(dq), s3(dk), s3(dv), 64 ** -0.5, _stream()),
              "cd360_attn_bwd_bf16")
    return dq, dk, dv


def self_attention_qkv(qkv: torch.Tensor, heads: int) -> torch.Tensor:
    """Self-attention on the merged projection output qkv [b, N, 3*H*64] (q | k | v column slices, read in place).  Under autograd
    the backward kernel writes dq, dk, dv straight into the three slices of ONE d(qkv) buffer (grad.SelfAttentionFn), so the
    projection's backward is a single GEMM and no slice-gradient fills / adds are launched."""
    inner = heads * 64
    assert qkv.shape[-1] == 3 * inner
    if _wants_grad(qkv):
        from . import grad
        return grad.SelfAttentionFn.apply(qkv, heads)
    return attention(qkv[..., :inner], qkv[..., inner:2 * inner], qkv[..., 2 * inner:], heads, qkv.shape[1])


def attention_fp8mfma(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, nk: Optional[int] = None, amax=None) -> torch.Tensor:
    """`attention` with both contractions on fp8 (e4m3) MFMA -- BASELINE configs[4], Nk <= 96 only.  Same bf16 tensors; the
    per-tensor scales come from `amax` = (max|q|, max|k|, max|v|), measured here (one host sync) when not given."""
    _need_gpu(q, k, v)
    b, nq, inner = q.shape
    assert inner == heads * 64 and q.dtype == k.dtype == v.dtype == torch.bfloat16
    assert q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1
    nk = k.shape[1] if nk is None else nk
    if amax is None:
        amax = torch.stack([q.abs().amax(), k[:, :nk].abs().amax(), v[:, :nk].abs().amax()]).float().tolist()
    out = torch.empty(b, nq, inner, dtype=torch.bfloat16, device=q.device)
    arr = (ctypes.c_float * 3)(*[float(a) for a in amax])
    with _timed("attn_fp8mfma", 4.0 * b * heads * nq * nk * 64, 2.0 * (2 * b * nq * inner + 2 * b * nk * inner)):
      check(
        _lib.load().cd360_attn_fwd_fp8mfma_bf16(
            _ptr(q), _ptr(k), _ptr(v), _ptr(out), b, heads, nq, nk,
            _I64x3(q.stride(0), 64, q.stride(1)), _I64x3(k.stride(0), 64, k.stride(1)),
            _I64x3(v.stride(0), 64, v.stride(1)), _I64x3(out.stride(0), 64, out.stride(1)),
            64 ** -0.5, arr, _stream()),
        "cd360_attn_fwd_fp8mfma_bf16")
    return out


def memory_efficient_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, attn_bias=None, op=None) -> torch.Tensor:
    """Same contract as xformers.ops.memory_efficient_attention for the layout the reference uses:
    q, k, v contiguous [B*H, N, 64] (sgm/modules/attention.py:393-408)."""
    if attn_bias is not None:
        raise NotImplementedError("attn_bias is not used on this path (attention.py:403)")
    _need_gpu(q, k, v)
    bh, nq, d = q.shape
    nk = k.shape[1]
    if d != 64 and d % 64 == 0 and d <= 512 and nk == nq:
        # the first stage's single-head attention (sgm/modules/diffusionmodules/model.py:248-250: [B, H W, C], C = 512 at SDXL widths)
        dt = q.dtype
        q, k, v = (t.to(torch.bfloat16).contiguous() for t in (q, k, v))
        return attention_single(q, k, v, qscale=d ** -0.5 * 1.4426950408889634).to(dt)
    if d != 64:
        raise Cd360Error(f"head dim {d} unsupported (SDXL uses 64; single-head self-attention takes 128 .. 512 in steps of 64)")
    dt = q.dtype
    q, k, v = (t.to(torch.bfloat16).contiguous() for t in (q, k, v))
    out = torch.empty_like(q)
    check(_lib.load().cd360_attn_fwd_xformers_bf16(_ptr(q), _ptr(k), _ptr(v), _ptr(out), bh, nq, nk, 64 ** -0.5, _stream()),
          "cd360_attn_fwd_xformers_bf16")
    return out.to(dt)


_I64x2 = ctypes.c_int64 * 2


def attention_single_splits(b: int, n: int) -> int:
    """Key splits cd360_attn_single_bf16 uses for b images of n pixels (1: one launch, no combine)."""
    return _lib.load().cd360_attn_single_splits(b, n)


def attention_single(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, qscale: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Single-head self-attention at head dim C (the first stage's mid-block attention, model.py:204-265): q, k, v [b, N, C] bf16
    (C % 64 == 0, C <= 512; last dim contiguous, row / batch strides free: e.g. the column slices of one merged q|k|v projection) ->
    [b, N, C] = softmax_2(qscale q k^T) v.  qscale = 1: q already carries C^-0.5 log2 e (pack_attn_qkv_weight).  Forward only."""
    _need_gpu(q, k, v)
    b, n, c = q.shape
    assert q.dtype == k.dtype == v.dtype == torch.bfloat16 and k.shape == q.shape and v.shape == q.shape
    assert q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1
    if out is None:
        out = torch.empty(b, n, c, dtype=torch.bfloat16, device=q.device)
    lib = _lib.load()
    nbytes = lib.cd360_attn_single_workspace_bytes(b, n, c)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device) if nbytes > 0 else None
    st = lambda t: _I64x2(t.stride(0), t.stride(1))
    with _timed("attn_single", 4.0 * b * n * n * c, 2.0 * 4 * b * n * c):
        check(lib.cd360_attn_single_bf16(_ptr(q), _ptr(k), _ptr(v), _ptr(out), b, n, c, st(q), st(k), st(v), st(out), float(qscale), _ptr(ws),
                                         _stream()), "cd360_attn_single_bf16")
    return out


# ----------------------------------------------------------------------------------------------- rays / projection
def patch_rays(cams: torch.Tensor, xs: torch.Tensor, ys: torch.Tensor) -> torch.Tensor:
    _need_gpu(cams, xs, ys)
    b, n1, _ = cams.shape
    r = xs.numel()
    rays = torch.empty(b, n1, r * r, 6, dtype=torch.float32, device=cams.device)
    check(_lib.load().cd360_patch_rays(_ptr(cams), _ptr(xs), _ptr(ys), _ptr(rays), b, n1 - 1, r, _stream()), "cd360_patch_rays")
    return rays


def ray_project_index(cams, xs, ys, t, want_points=True, want_grid=True, want_index=True):
    """t: [S] or [hw, S] fp32.  Returns dict(points, grid, x0, y0, mask)."""
    _need_gpu(cams, xs, ys, t)
    b, n1, _ = cams.shape
    n, r = n1 - 1, xs.numel()
    hw, S = r * r, t.shape[-1]
    stride = 0 if t.dim() == 1 else S
    dev = cams.device
    pts = torch.empty(b, hw, S, 3, dtype=torch.float32, device=dev) if want_points else None
    grid = torch.empty(b, n, hw, S, 2, dtype=torch.float32, device=dev) if want_grid else None
    x0 = torch.empty(b, n, hw, S, dtype=torch.int32, device=dev) if want_index else None
    y0 = torch.empty_like(x0) if want_index else None
    mask = torch.empty_like(x0) if want_index else None
    check(_lib.load().cd360_ray_project_index(_ptr(cams), _ptr(xs), _ptr(ys), _ptr(t.contiguous()), stride, b, n, r, S, _ptr(pts), _ptr(grid),
                                             _ptr(x0), _ptr(y0), _ptr(mask), _stream()), "cd360_ray_project_index")
    return dict(points=pts, grid=grid, x0=x0, y0=y0, mask=mask)


def sample_pdf(bins: torch.Tensor, weights: torch.Tensor, u: torch.Tensor, eps: float = 1e-5, want_dists: bool = False, inplace: bool = False):
    """Inverse-CDF depth sampling (cd360_sample_pdf; replaces pytorch3d._C.sample_pdf at nerfsd_pytorch3d.py:300-305).
    bins [..., n_bins + 1], weights [..., n_bins], u [..., n_samples] in [0, 1), fp32 -> samples [..., n_samples]
    (inplace=True writes them over u, as pytorch3d does) and, with want_dists, the gaps to the next sample (:306)."""
    _need_gpu(bins, weights, u)
    n_bins, n_samples = weights.shape[-1], u.shape[-1]
    rows = weights.numel() // n_bins
    assert bins.shape[-1] == n_bins + 1 and bins.numel() == rows * (n_bins + 1) and u.numel() == rows * n_samples
    assert bins.dtype == weights.dtype == u.dtype == torch.float32
    if inplace and (want_dists or not u.is_contiguous()):
        raise ValueError("sample_pdf(inplace=True) needs a contiguous u and cannot return dists")
    bins, weights, uc = bins.contiguous(), weights.contiguous(), u.contiguous()
    out = uc if inplace else torch.empty_like(uc)
    dists = torch.empty_like(uc) if want_dists else None
    check(_lib.load().cd360_sample_pdf(_ptr(bins), _ptr(weights), _ptr(uc), _ptr(out), _ptr(dists), float(eps), rows, n_bins, n_samples,
                                       _stream()), "cd360_sample_pdf")
    return (out, dists) if want_dists else out


def feature_gather(xref: torch.Tensor, grid: torch.Tensor) -> torch.Tensor:
    """xref [n_img, r*r, C] (fp32|bf16), grid [n_img, P, 2] fp32 -> [n_img, P, C]."""
    _need_gpu(xref, grid)
    n_img, hw, C = xref.shape
    r = int(round(hw ** 0.5))
    assert r * r == hw and grid.dtype == torch.float32
    xref, grid = xref.contiguous(), grid.contiguous()
    P = grid.shape[1]
    out = torch.empty(n_img, P, C, dtype=xref.dtype, device=xref.device)
    dt = {torch.float32: 0, torch.bfloat16: 1}[xref.dtype]
    check(_lib.load().cd360_feature_gather(_ptr(xref), _ptr(grid), _ptr(out), n_img, P, r, C, dt, _stream()), "cd360_feature_gather")
    return out


# ----------------------------------------------------------------------------------------------- FeatureNeRF
def plucker_features(cams, xs, ys) -> torch.Tensor:
    _need_gpu(cams, xs, ys)
    b, n1, _ = cams.shape
    r = xs.numel()
    out = torch.empty(b, n1 - 1, r * r, 104, dtype=torch.float32, device=cams.device)
    with _timed("plucker_features", 0.0, 4.0 * 104 * b * (n1 - 1) * r * r):
      check(_lib.load().cd360_plucker_features(_ptr(cams), _ptr(xs), _ptr(ys), _ptr(out), b, n1 - 1, r, _stream()), "cd360_plucker_features")
    return out


def plucker_features_bf16(cams, xs, ys) -> torch.Tensor:
    """plucker_features as bf16 rows of 128 (99 values + zero pad): the A operand of the zP table GEMM on gemm()."""
    _need_gpu(cams, xs, ys)
    b, n1, _ = cams.shape
    r = xs.numel()
    out = torch.empty(b, n1 - 1, r * r, 128, dtype=torch.bfloat16, device=cams.device)
    with _timed("plucker_features", 0.0, 2.0 * 128 * b * (n1 - 1) * r * r):
        check(_lib.load().cd360_plucker_features_bf16(_ptr(cams), _ptr(xs), _ptr(ys), _ptr(out), b, n1 - 1, r, _stream()), "cd360_plucker_features_bf16")
    return out


def nerf_k_padded() -> int:
    return _lib.load().cd360_nerf_k_padded()


def nerf_mlp_aggregate(cams, xs, ys, t, Y, zP, lv, cview, Wk, want_logits=False, img_map=None):
    """img_map (int32 [b*n], optional): Y / lv hold only distinct table images [n_tab, hw, ...]; (batch, view) reads image img_map[b*n_idx].
    Differentiable with respect to Y, zP, lv, cview and Wk (grad.NerfAggregateFn; logits and lse are then always returned)."""
    if _wants_grad(Y, zP, lv, cview, Wk):
        from . import grad
        return grad.NerfAggregateFn.apply(cams, xs, ys, t, Y, zP, lv, cview, Wk, img_map)
    _need_gpu(cams, xs, ys, t, Y, zP, lv, cview, Wk, img_map)
    b, n1, _ = cams.shape
    n, r = n1 - 1, xs.numel()
    hw, S = r * r, t.shape[-1]
    C = Y.shape[-1]
    ntab = b * n if img_map is None else Y.shape[0]
    assert Y.shape == (ntab, hw, C) and zP.shape == (b * n, hw, C) and Y.dtype == torch.bfloat16 and zP.dtype == torch.bfloat16
    assert lv.shape == (ntab, hw) and lv.dtype == torch.float32 and cview.shape == (b, n) and cview.dtype == torch.float32
    assert img_map is None or (img_map.dtype == torch.int32 and img_map.numel() == b * n and img_map.is_contiguous())
    assert Wk.shape == (C, nerf_k_padded()) and Wk.dtype == torch.bfloat16
    for x in (Y, zP, lv, cview, Wk):
        assert x.is_contiguous()
    stride = 0 if t.dim() == 1 else S
    g = torch.empty(b, hw * S, C, dtype=torch.bfloat16, device=Y.device)
    logits = torch.empty(b, n, hw * S, dtype=torch.float32, device=Y.device) if want_logits else None
    lse = torch.empty(b, hw * S, 2, dtype=torch.float32, device=Y.device) if want_logits else None
    # two passes (cd360_nerf_mlp_aggregate_ws): the per-(view, sample) geometry, view logit and softmax statistics once, into `ws`, then
    # the per-channel-slice gather / MLP / aggregate reading 32-byte records (the library falls back to the one-pass kernels outside the
    # two-pass envelope or under cd360_tuning.nerf_kernel = 0 | 1)
    lib = _lib.load()
    ws = torch.empty(int(lib.cd360_nerf_ws_bytes(b, n, r, S)), dtype=torch.uint8, device=Y.device)
    with _timed("nerf_mlp_aggregate", 2.0 * b * n * hw * S * 99 * C, 2.0 * C * (2 * b * n * hw + b * hw * S)):
      check(lib.cd360_nerf_mlp_aggregate_ws(_ptr(cams), _ptr(xs), _ptr(ys), _ptr(t.contiguous()), stride, _ptr(Y), _ptr(zP), _ptr(lv),
                                            _ptr(cview), _ptr(Wk), _ptr(img_map), _ptr(g), _ptr(logits), _ptr(lse), b, n, r, S, C, ntab,
                                            _ptr(ws), ws.numel(), _stream()),
          "cd360_nerf_mlp_aggregate_ws")
    return g, logits, lse


def nerf_mlp_aggregate_bwd(cams, xs, ys, t, Y, zP, lv, cview, Wk, img_map, g, lse, dg, scatter: bool = True):
    """Backward kernel of nerf_mlp_aggregate -> (dz [b,n,hw*S,C] bf16, F [b,n,hw*S,112] bf16, dY [tables,hw,C] fp32,
    dlv [tables,hw] fp32, dcview [b,n] fp32, dlogit [b,n,hw*S] fp32).  scatter=False skips the atomic table scatters (dY, dlv and
    dcview come back None; the caller reduces dz / dlogit itself)."""
    _need_gpu(cams, xs, ys, t, Y, zP, lv, cview, Wk, img_map, g, lse, dg)
    b, n1, _ = cams.shape
    n, r = n1 - 1, xs.numel()
    hw, S = r * r, t.shape[-1]
    C = Y.shape[-1]
    dev = Y.device
    dg = dg.contiguous()
    assert dg.dtype == torch.bfloat16 and dg.shape == (b, hw * S, C) and g.shape == dg.shape and lse.shape == (b, hw * S, 2)
    kp = nerf_k_padded()
    dz = torch.empty(b, n, hw * S, C, dtype=torch.bfloat16, device=dev)
    F = torch.empty(b, n, hw * S, kp, dtype=torch.bfloat16, device=dev)
    dY = torch.zeros(Y.shape, dtype=torch.float32, device=dev) if scatter else None
    # dlogit: every 64-channel chunk stores its term into `parts`, the library sums them in chunk order -- no atomics, so the view-logit
    # gradients (and with them a whole fine-tuning step) are bit-reproducible run to run (cd360_nerf_mlp_aggregate_bwd_det)
    dlogit = torch.empty(b, n, hw * S, dtype=torch.float32, device=dev)
    parts = torch.empty(C // 64, b, n, hw * S, dtype=torch.float32, device=dev)
    dlv = torch.zeros(lv.shape, dtype=torch.float32, device=dev) if scatter else None
    dcview = torch.zeros(b, n, dtype=torch.float32, device=dev) if scatter else None
    stride = 0 if t.dim() == 1 else S
    with _timed("nerf_mlp_aggregate_bwd", 2.0 * b * n * hw * S * 99 * C, 2.0 * C * (2 * b * n * hw + (2 + n) * b * hw * S)):
        check(_lib.load().cd360_nerf_mlp_aggregate_bwd_det(_ptr(cams), _ptr(xs), _ptr(ys), _ptr(t.contiguous()), stride, _ptr(Y), _ptr(zP), _ptr(lv),
                                                          _ptr(cview), _ptr(Wk), _ptr(img_map), _ptr(g), _ptr(lse), _ptr(dg), _ptr(dz), _ptr(F),
                                                          _ptr(dY), _ptr(dlogit), _ptr(parts), _ptr(dlv), _ptr(dcview), b, n, r, S, C, _stream()),
              "cd360_nerf_mlp_aggregate_bwd_det")
    return dz, F, dY, dlv, dcview, dlogit


# ----------------------------------------------------------------------------------------------- volume rendering
def volrender(feats, sigma_raw, dists, rgb_raw=None, want_weights=False, sigma_is_raw=True, rgb_is_raw=True):
    """feats [b,hw,S,C] (fp32|bf16), sigma_raw [b,hw,S] fp32, dists [S] or [hw,S] fp32, rgb_raw [b,hw,S,3] fp32|None.
    Differentiable with respect to feats, sigma_raw and rgb_raw (grad.VolRenderFn)."""
    if _wants_grad(feats, sigma_raw, rgb_raw):
        from . import grad
        return grad.VolRenderFn.apply(feats, sigma_raw, dists, rgb_raw, want_weights, sigma_is_raw, rgb_is_raw)
    _need_gpu(feats, sigma_raw, dists, rgb_raw)
    b, hw, S, C = feats.shape
    feats, sigma_raw, dists = feats.contiguous(), sigma_raw.contiguous().float(), dists.contiguous().float()
    if rgb_raw is not None:
        rgb_raw = rgb_raw.contiguous().float()
    dev = feats.device
    rendered = torch.empty(b, hw, C, dtype=feats.dtype, device=dev)
    fg = torch.empty(b, hw, 1, dtype=torch.float32, device=dev)
    alphas = torch.empty(b, hw, S, 1, dtype=torch.float32, device=dev)
    weights = torch.empty(b, hw, S, 1, dtype=torch.float32, device=dev) if want_weights else None
    rgb = torch.empty(b, hw, 3, dtype=torch.float32, device=dev) if rgb_raw is not None else None
    dt = {torch.float32: 0, torch.bfloat16: 1}[feats.dtype]
    stride = 0 if dists.dim() == 1 else S
    with _timed("volrender", 0.0, feats.element_size() * C * b * hw * (S + 1.0)):
      check(_lib.load().cd360_volrender(_ptr(feats), _ptr(sigma_raw), _ptr(rgb_raw), _ptr(dists), stride, _ptr(rendered), _ptr(fg),
                                     _ptr(alphas), _ptr(weights), _ptr(rgb), b, hw, S, C, dt, (0 if sigma_is_raw else 1) | (0 if rgb_is_raw else 2),
                                     _stream()), "cd360_volrender")
    return rendered, fg, alphas, weights, rgb


def volrender_bwd(feats, sigma_raw, dists, rgb_raw, d_rendered, d_fg, d_alphas, d_weights, d_rgb, sigma_is_raw=True, rgb_is_raw=True):
    """Backward of volrender: (d_feats [b,hw,S,C], d_sigma_raw [b,hw,S] fp32, d_rgb_raw [b,hw,S,3] fp32 | None).  Gradients that
    did not arrive are None."""
    _need_gpu(feats, sigma_raw, dists, rgb_raw, d_rendered, d_fg, d_alphas, d_weights, d_rgb)
    b, hw, S, C = feats.shape
    f32 = lambda t, shape: None if t is None else t.reshape(shape).contiguous().float()
    feats, sigma_raw, dists = feats.contiguous(), sigma_raw.contiguous().float(), dists.contiguous().float()
    rgb_raw = None if rgb_raw is None else rgb_raw.contiguous().float()
    if d_rendered is None:
        d_rendered = torch.zeros(b, hw, C, dtype=feats.dtype, device=feats.device)
    d_rendered = d_rendered.contiguous().to(feats.dtype)
    d_fg, d_alphas, d_weights, d_rgb = f32(d_fg, (b, hw)), f32(d_alphas, (b, hw, S)), f32(d_weights, (b, hw, S)), f32(d_rgb, (b, hw, 3))
    d_feats = torch.empty_like(feats)
    d_sigma = torch.empty(b, hw, S, dtype=torch.float32, device=feats.device)
    d_rgb_raw = torch.empty(b, hw, S, 3, dtype=torch.float32, device=feats.device) if rgb_raw is not None else None
    dt = {torch.float32: 0, torch.bfloat16: 1}[feats.dtype]
    stride = 0 if dists.dim() == 1 else S
    with _timed("volrender_bwd", 0.0, feats.element_size() * C * b * hw * (2.0 * S + 1.0)):
        check(_lib.load().cd360_volrender_bwd(_ptr(feats), _ptr(sigma_raw), _ptr(rgb_raw), _ptr(dists), stride, _ptr(d_rendered), _ptr(d_fg),
                                             _ptr(d_alphas), _ptr(d_weights), _ptr(d_rgb), _ptr(d_feats), _ptr(d_sigma), _ptr(d_rgb_raw), b, hw, S, C,
                                             dt, (0 if sigma_is_raw else 1) | (0 if rgb_is_raw else 2), _stream()), "cd360_volrender_bwd")
    return d_feats, d_sigma, d_rgb_raw


def rowdot4(h: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """h [..., C] bf16, w [4, C] fp32 -> [..., 4] fp32 (FeatureNeRF decoder).  Differentiable (grad.RowDot4Fn)."""
    if _wants_grad(h, w):
        from . import grad
        return grad.RowDot4Fn.apply(h, w)
    _need_gpu(h, w)
    C = h.shape[-1]
    assert h.dtype == torch.bfloat16 and h.is_contiguous() and w.shape == (4, C) and w.dtype == torch.float32 and w.is_contiguous()
    rows = h.numel() // C
    out = torch.empty(*h.shape[:-1], 4, dtype=torch.float32, device=h.device)
    with _timed("rowdot4", 0.0, 2.0 * rows * C):
      check(_lib.load().cd360_rowdot4_bf16(_ptr(h), _ptr(w), _ptr(out), rows, C, _stream()), "cd360_rowdot4_bf16")
    return out


def rowdot1(h: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """h [..., C] bf16, w [C] fp32 -> [...] fp32 (cd360_rowdot1_bf16: the view-logit column lv = xref . vf of the reference tables).
    Not differentiable: the training path differentiates vf through grad.NerfRenderFn's own reductions."""
    _need_gpu(h, w)
    C = h.shape[-1]
    assert h.dtype == torch.bfloat16 and h.is_contiguous() and w.shape == (C,) and w.dtype == torch.float32 and w.is_contiguous()
    rows = h.numel() // C
    out = torch.empty(h.shape[:-1], dtype=torch.float32, device=h.device)
    with _timed("rowdot1", 0.0, 2.0 * rows * C):
        check(_lib.load().cd360_rowdot1_bf16(_ptr(h), _ptr(w), _ptr(out), rows, C, _stream()), "cd360_rowdot1_bf16")
    return out


def render_loss_ok(fg, alphas, rgb, op, mask_, want) -> bool:
    """Can cd360_render_loss_f32 serve these tensors (fp32, on the GPU, a one-channel mask)?"""
    ts = [t for t in (fg, alphas, rgb, op, mask_, want) if t is not None]
    from . import routes
    return (not routes.no_train_fusions and all(t.is_cuda and t.dtype == torch.float32 for t in ts) and (mask_ is None or mask_.shape[1] == 1)
            and (rgb is None or (mask_ is not None and want is not None)))


def render_loss(fg, alphas, rgb, op, bgw, mask_, want, den) -> torch.Tensor:
    """The fg / bg / rgb loss terms of one pose block (loss.py:188-207 of the reference) -> [b, 3] fp32; differentiable with respect
    to fg [b, hw, 1], alphas [b, hw, S, 1] and rgb [b, hw, 3] | None (grad.RenderLossFn).  op, bgw [b, hw]; mask_ [b, 1, r, r];
    want [b, 3, r, r]; den [b]."""
    if _wants_grad(fg, alphas, rgb):
        from . import grad
        return grad.RenderLossFn.apply(fg, alphas, rgb, op, bgw, mask_, want, den)
    return _render_loss_fwd(fg, alphas, rgb, op, bgw, mask_, want, den)


def _render_loss_fwd(fg, alphas, rgb, op, bgw, mask_, want, den):
    _need_gpu(fg, alphas, rgb, op, bgw, mask_, want, den)
    b, hw = op.shape
    S = alphas.numel() // (b * hw)
    c = lambda t: None if t is None else t.detach().contiguous()
    fg, alphas, rgb, op, bgw, mask_, want, den = map(c, (fg, alphas, rgb, op, bgw, mask_, want, den))
    assert fg.numel() == b * hw and (rgb is None or rgb.numel() == b * hw * 3)
    out = torch.empty(b, 3, dtype=torch.float32, device=op.device)
    check(_lib.load().cd360_render_loss_f32(_ptr(fg), _ptr(alphas), _ptr(rgb), _ptr(op), _ptr(bgw), _ptr(mask_), _ptr(want), _ptr(den), _ptr(out),
                                            b, hw, S, _stream()), "cd360_render_loss_f32")
    return out


def render_loss_bwd(fg, alphas, rgb, op, bgw, mask_, want, den, g):
    """-> (d_fg, d_alphas, d_rgb | None) in the shapes of fg, alphas, rgb."""
    _need_gpu(fg, alphas, rgb, op, bgw, mask_, want, den, g)
    b, hw = op.shape
    S = alphas.numel() // (b * hw)
    c = lambda t: None if t is None else t.detach().contiguous()
    fgc, alc, rgbc, op, bgw, mask_, want, den = map(c, (fg, alphas, rgb, op, bgw, mask_, want, den))
    d_fg, d_al = torch.empty_like(fgc), torch.empty_like(alc)
    d_rgb = None if rgbc is None else torch.empty_like(rgbc)
    check(_lib.load().cd360_render_loss_bwd_f32(_ptr(fgc), _ptr(alc), _ptr(rgbc), _ptr(op), _ptr(bgw), _ptr(mask_), _ptr(want), _ptr(den),
                                                _ptr(g.contiguous().float()), _ptr(d_fg), _ptr(d_al), _ptr(d_rgb), b, hw, S, _stream()),
          "cd360_render_loss_bwd_f32")
    return d_fg, d_al, d_rgb


def nerf_pack_weights(W1, b1, b2, wv, bv, Wd, kcol):
    """cd360_nerf_pack_weights_bf16: bf16 parameters of one FeatureNeRFEncoding -> (bf16 arena Wf | Wk | Wp, fp32 arena b1 | b2 | vf |
    v_cam | bv | Wd); the caller slices (see the header)."""
    _need_gpu(W1, b1, b2, wv, bv, Wd, kcol)
    C, NK = W1.shape[0], kcol.numel()
    assert all(t.dtype == torch.bfloat16 and t.is_contiguous() for t in (W1, b1, b2, wv, bv, Wd)) and kcol.dtype == torch.int32
    assert W1.shape == (C, C + 198) and wv.numel() == C + 198 and Wd.shape == (4, C) and b1.numel() == C and b2.numel() == C
    wb = torch.empty(C * (C + NK + 128), dtype=torch.bfloat16, device=W1.device)
    wf = torch.empty(7 * C + 104, dtype=torch.float32, device=W1.device)
    check(_lib.load().cd360_nerf_pack_weights_bf16(_ptr(W1), _ptr(b1), _ptr(b2), _ptr(wv), _ptr(bv), _ptr(Wd), _ptr(kcol), _ptr(wb), _ptr(wf),
                                                   C, NK, _stream()), "cd360_nerf_pack_weights_bf16")
    return wb, wf


def nerf_unpack_grads(grads, kpos, C: int, NK: int):
    """cd360_nerf_unpack_grads_bf16: the nine gradients of the packed operands (None = none arrived) -> (dW1 [C, C + 198] bf16, small
    bf16 arena db1 | db2 | dwv | dbv | dWd)."""
    import ctypes
    some = next(g for g in grads if g is not None)
    gs = [None if g is None else g.contiguous() for g in grads]
    _need_gpu(kpos, *gs)
    for g, n_ in zip(gs, (C * C, C * NK, C * 128, C, C, C, 99, 1, 4 * C)):
        assert g is None or (g.numel() == n_ and g.dtype in (torch.float32, torch.bfloat16)), "nerf_unpack_grads: unexpected gradient"
    ptrs = (ctypes.c_void_p * 9)(*[None if g is None else g.data_ptr() for g in gs])
    dts = (ctypes.c_int * 9)(*[1 if (g is not None and g.dtype == torch.bfloat16) else 0 for g in gs])
    dW1 = torch.empty(C, C + 198, dtype=torch.bfloat16, device=some.device)
    small = torch.empty(7 * C + 200, dtype=torch.bfloat16, device=some.device)
    check(_lib.load().cd360_nerf_unpack_grads_bf16(ptrs, dts, _ptr(kpos), _ptr(dW1), _ptr(small), C, NK, _stream()), "cd360_nerf_unpack_grads_bf16")
    return dW1, small


def rowdot4_bwd(d_out: torch.Tensor, h: torch.Tensor, w: torch.Tensor, need_dh: bool = True, need_dw: bool = True):
    """Backward of rowdot4: d_out [..., 4] fp32 -> (dh [..., C] bf16 | None, dw [4, C] fp32 | None) (cd360_rowdot4_bwd_bf16)."""
    _need_gpu(d_out, h, w)
    C = h.shape[-1]
    rows = h.numel() // C
    d2 = d_out.reshape(rows, 4).float().contiguous()
    assert h.dtype == torch.bfloat16 and h.is_contiguous() and w.shape == (4, C) and w.dtype == torch.float32 and w.is_contiguous()
    lib = _lib.load()
    dh = torch.empty_like(h) if need_dh else None
    part = torch.empty(lib.cd360_rowdot4_bwd_slabs(rows), 4, C, dtype=torch.float32, device=h.device) if need_dw else None
    with _timed("rowdot4_bwd", 0.0, 2.0 * rows * C * (int(need_dh) + int(need_dw))):
        check(lib.cd360_rowdot4_bwd_bf16(_ptr(d2), _ptr(h), _ptr(w), _ptr(dh), _ptr(part), rows, C, _stream()), "cd360_rowdot4_bwd_bf16")
    return dh, (None if part is None else part.sum(0))


# ----------------------------------------------------------------------------------------------- GroupNorm (+SiLU)
def gn_silu(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float, silu: bool,
            out: Optional[torch.Tensor] = None, tile_stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x: channels-last bf16 viewed as [N, P, C] (contiguous).  gamma/beta fp32 [C].
    tile_stats: the fp32 [N, slabs, C, 2] per-slab channel sums conv_igemm(..., want_stats=True) returned for this very tensor
    (the statistics read pass is skipped).  Differentiable with respect to x (grad.GroupNormSiluFn)."""
    if _wants_grad(x, gamma, beta):
        from . import grad
        assert out is None
        return grad.GroupNormSiluFn.apply(x, gamma, beta, groups, eps, silu, tile_stats)
    _need_gpu(x, gamma, beta, tile_stats)
    N, P, C = x.shape
    slabs = 0
    if tile_stats is not None:
        assert tile_stats.dtype == torch.float32 and tile_stats.is_contiguous() and tile_stats.shape[0] == N and tile_stats.shape[2:] == (C, 2)
        slabs = tile_stats.shape[1]
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and gamma.dtype == torch.float32 and beta.dtype == torch.float32
    lib = _lib.load()
    ws = torch.empty(lib.cd360_gn_workspace_bytes(N, P, C), dtype=torch.uint8, device=x.device)
    if out is None:
        out = torch.empty_like(x)
    with _timed("gn_silu", 0.0, 2.0 * (3 if tile_stats is None else 2) * N * P * C):
      check(lib.cd360_gn_silu_bf16(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(out), _ptr(ws), N, P, C, groups, float(eps), int(silu),
                                   _ptr(tile_stats), slabs, _stream()), "cd360_gn_silu_bf16")
    return out


def gn_silu_bwd(x: torch.Tensor, dy: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float, silu: bool) -> torch.Tensor:
    """Backward of gn_silu with respect to x: x, dy [N, P, C] bf16 -> dx."""
    _need_gpu(x, dy, gamma, beta)
    N, P, C = x.shape
    dy = dy.contiguous()
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and dy.dtype == torch.bfloat16 and dy.shape == x.shape
    lib = _lib.load()
    ws = torch.empty(lib.cd360_gn_bwd_workspace_bytes(N, P, C), dtype=torch.uint8, device=x.device)
    dx = torch.empty_like(x)
    with _timed("gn_silu_bwd", 0.0, 2.0 * 6 * N * P * C):
        check(lib.cd360_gn_silu_bwd_bf16(_ptr(x), _ptr(dy), _ptr(gamma), _ptr(beta), _ptr(dx), _ptr(ws), N, P, C, groups, float(eps), int(silu),
                                         _stream()), "cd360_gn_silu_bwd_bf16")
    return dx


# ----------------------------------------------------------------------------------------------- epilogues
def geglu(proj: torch.Tensor) -> torch.Tensor:
    """proj [..., 2*inner] bf16 = [x | gate] -> [..., inner] = x * gelu(gate).  Differentiable (grad.GegluFn)."""
    if _wants_grad(proj):
        from . import grad
        return grad.GegluFn.apply(proj)
    _need_gpu(proj)
    inner = proj.shape[-1] // 2
    assert proj.dtype == torch.bfloat16 and proj.is_contiguous()
    rows = proj.numel() // (2 * inner)
    out = torch.empty(*proj.shape[:-1], inner, dtype=torch.bfloat16, device=proj.device)
    with _timed("geglu", 0.0, 2.0 * 3 * rows * inner):
        check(_lib.load().cd360_geglu_bf16(_ptr(proj), _ptr(out), rows, inner, _stream()), "cd360_geglu_bf16")
    return out


def geglu_bwd(proj: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """Backward of geglu: d(proj) [..., 2*inner] = [dy gelu(gate) | dy x gelu'(gate)]."""
    _need_gpu(proj, dy)
    inner = proj.shape[-1] // 2
    dy = dy.contiguous()
    assert proj.dtype == torch.bfloat16 and proj.is_contiguous() and dy.dtype == torch.bfloat16 and dy.shape == (*proj.shape[:-1], inner)
    rows = proj.numel() // (2 * inner)
    din = torch.empty_like(proj)
    with _timed("geglu_bwd", 0.0, 2.0 * 5 * rows * inner):
        check(_lib.load().cd360_geglu_bwd_bf16(_ptr(proj), _ptr(dy), _ptr(din), rows, inner, _stream()), "cd360_geglu_bwd_bf16")
    return din


def concat_channels(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """torch.cat([a, b], dim=1) for channels-last bf16 images [N, C, H, W]; returns a channels-last [N, Ca+Cb, H, W].
    Differentiable (grad.ConcatChannelsFn: the backward is two channel slices)."""
    if _wants_grad(a, b):
        from . import grad
        return grad.ConcatChannelsFn.apply(a, b)
    _need_gpu(a, b)
    N, ca, H, W = a.shape
    cb = b.shape[1]
    at, bt = a.permute(0, 2, 3, 1), b.permute(0, 2, 3, 1)
    assert a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16 and at.is_contiguous() and bt.is_contiguous() and b.shape[0] == N
    out = torch.empty(N, H, W, ca + cb, dtype=torch.bfloat16, device=a.device)
    with _timed("concat_channels", 0.0, 2.0 * 2 * N * H * W * (ca + cb)):
        check(_lib.load().cd360_concat_channels_bf16(_ptr(at), _ptr(bt), _ptr(out), N * H * W, ca, cb, _stream()), "cd360_concat_channels_bf16")
    return out.permute(0, 3, 1, 2)


def concat_gn_stats(sa: torch.Tensor, sb: torch.Tensor) -> torch.Tensor:
    """torch.cat([sa, sb], dim=2) of two GroupNorm slab-statistics tensors [N, slabs, C, 2] fp32 (the statistics of a channel concatenation
    are the concatenated per-channel statistics) on cd360_concat_channels_bf16: a row of C (sum, sumsq) pairs is a row of 4 C bf16 words
    to that kernel -- no torch-issued cat kernel inside a captured step."""
    _need_gpu(sa, sb)
    N, slabs, ca, two = sa.shape
    cb = sb.shape[2]
    assert two == 2 and sb.shape == (N, slabs, cb, 2) and sa.dtype == sb.dtype == torch.float32 and sa.is_contiguous() and sb.is_contiguous()
    out = torch.empty(N, slabs, ca + cb, 2, dtype=torch.float32, device=sa.device)
    check(_lib.load().cd360_concat_channels_bf16(_ptr(sa), _ptr(sb), _ptr(out), N * slabs, 4 * ca, 4 * cb, _stream()), "cd360_concat_channels_bf16")
    return out


# ----------------------------------------------------------------------------------------------- conv3x3 / GEMM (implicit GEMM)
def pack_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """nn.Conv2d weight [Cout, Cin, k, k] (k = 3 | 1) or a Linear weight [Cout, Cin] -> the bf16 [Cout, taps*Cin] matrix
    cd360_conv_igemm_bf16 reads.  K order: G = cd360_conv_k_order(Cin, taps) 64-channel chunks per group; group outer, tap middle,
    chunk-in-group inner: k = ((cg*taps + ky*3+kx)*G + j)*64 + ci%64 with ci//64 = cg*G + j."""
    if w.dim() == 2:
        return w.detach().to(torch.bfloat16).contiguous()
    cout, cin, kh, kw = w.shape
    assert cin % 64 == 0 and kh == kw and kh in (1, 3)
    g = _lib.load().cd360_conv_k_order(cin, kh * kw)
    wp = w.detach().reshape(cout, cin // (64 * g), g, 64, kh * kw).permute(0, 1, 4, 2, 3)  # [co, group, tap, chunk-in-group, 64]
    return wp.reshape(cout, -1).to(torch.bfloat16).contiguous()


def conv_igemm(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], N: int, H: int, W: int, taps: int = 9,
               emb: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None, want_stats: bool = False, stride: int = 1,
               alg_channels: Optional[tuple] = None, w_dgrad=None):
    """x [N*H*W, Cin] (or [N, H*W, Cin]) channels-last bf16; w_packed [Cout, taps*Cin] bf16; bias fp32 [Cout]; emb bf16 [N, Cout];
    res bf16 [N*Ho*Wo, Cout] -> [N, Ho*Wo, Cout] bf16 = conv3x3 (taps=9; stride 1, or 2 with Ho = H/2, Wo = W/2) or x @ w^T (taps=1)
    + bias + emb[n] + res.
    want_stats=True (H*W % 128 == 0): returns (out, tile_stats) with tile_stats fp32 [N, slabs, Cout, 2] = per pixel slab the channel
    sums / sums of squares of `out`, for gn_silu(out, ..., tile_stats=tile_stats).
    Differentiable with respect to x, emb and res (grad.ConvIgemmFn) when `w_dgrad` is given: a callable returning the packed weight
    of the data-gradient convolution (taps flipped, channels transposed: sgm...util.packed_conv_dgrad).  No weight gradient."""
    if _wants_grad(x, emb, res, w_packed, bias):
        from . import grad
        return grad.conv_igemm(x, w_packed, bias, N, H, W, taps, emb, res, want_stats, stride, alg_channels, w_dgrad)
    _need_gpu(x, w_packed, bias, emb, res)
    cin = x.shape[-1]
    cout = w_packed.shape[0]
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and x.numel() == N * H * W * cin
    assert w_packed.dtype == torch.bfloat16 and w_packed.is_contiguous() and w_packed.shape[1] == taps * cin
    assert bias is None or (bias.dtype == torch.float32 and bias.is_contiguous())
    assert emb is None or (emb.dtype == torch.bfloat16 and emb.shape == (N, cout) and emb.stride(1) == 1)  # rows may be strided
    ho, wo = H // stride, W // stride
    assert res is None or (res.dtype == torch.bfloat16 and res.is_contiguous() and res.numel() == N * ho * wo * cout)
    out = torch.empty(N, ho * wo, cout, dtype=torch.bfloat16, device=x.device)
    m = N * ho * wo
    lib = _lib.load()
    stats = None
    if want_stats:
        _lib.query_stream(_stream())
        rows = lib.cd360_conv_stats_rows(N, H, W, cin, cout, taps, stride)  # pixels per slab: the kernel serving this shape decides
        if rows <= 0 or (ho * wo) % rows or (rows < 64 and (ho * wo) % 128):  # slabs must not straddle images (register-staged kernel: 128-pixel tiles)
            raise Cd360Error(f"conv_igemm(want_stats=True): Ho*Wo = {ho * wo} is not a whole number of the kernel's {rows}-pixel slabs")
        stats = torch.empty(N, (ho * wo) // rows, cout, 2, dtype=torch.float32, device=x.device)
    acin, acout = alg_channels or (cin, cout)  # un-padded channel counts for the algorithmic FLOP / byte accounting
    with _timed("conv_igemm", 2.0 * m * taps * acin * acout, 2.0 * (N * H * W * acin + m * acout + taps * acin * acout)):
        check(lib.cd360_conv_igemm_bf16(_ptr(x), _ptr(w_packed), _ptr(bias), _ptr(emb), 0 if emb is None else emb.stride(0), _ptr(res), _ptr(out),
                                       N, H, W, cin, cout, taps, stride, _ptr(stats), _stream()), "cd360_conv_igemm_bf16")
    return (out, stats) if want_stats else out


class ConvRoute(NamedTuple):
    """The kernel a convolution launch runs (cd360_conv_route): family "register" (the register-staged kernel), "dma" (the LDS-DMA
    core: `tiling` 1..6, `halo` = the halo form, `slab_rows` = pixels per tile_stats slab) or "gemm" (1 x 1 on cd360_gemm_bf16)."""
    family: str
    tiling: int
    halo: bool
    slab_rows: int


_ROUTE_TILING_MASK, _ROUTE_HALO, _ROUTE_GEMM, _ROUTE_SLAB_SHIFT = 15, 16, 32, 8  # include/cd360_hip.h: CD360_ROUTE_*


def decode_conv_route(route: int) -> ConvRoute:
    if route == _ROUTE_GEMM:
        return ConvRoute("gemm", 0, False, 0)
    if route == 0:
        return ConvRoute("register", 0, False, 0)
    return ConvRoute("dma", route & _ROUTE_TILING_MASK, bool(route & _ROUTE_HALO), route >> _ROUTE_SLAB_SHIFT)


def conv_route(N: int, H: int, W: int, cin: int, cout: int, taps: int = 9, stride: int = 1) -> ConvRoute:
    """What conv_igemm launches for this shape on the current stream (its per-stream tuning included)."""
    _lib.query_stream(_stream())
    return decode_conv_route(_lib.load().cd360_conv_route(N, H, W, cin, cout, taps, stride))


def conv3x3_dma_route(N: int, H: int, W: int, cin: int, cout: int) -> ConvRoute:
    """What cd360_conv3x3_dma_bf16 itself launches for this shape on the current stream (family "register": outside its envelope)."""
    _lib.query_stream(_stream())
    return decode_conv_route(_lib.load().cd360_conv3x3_dma_route(N, H, W, cin, cout))


def conv_up2x_tiling(N: int, H: int, W: int, cin: int, cout: int) -> int:
    """The tiling (1..6) conv_up2x launches for this source image on the current stream."""
    _lib.query_stream(_stream())
    t = _lib.load().cd360_conv_up2x_route(N, H, W, cin, cout)
    check(min(t, 0), "cd360_conv_up2x_route")
    return t


def pack_upsample_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """nn.Conv2d weight [Cout, Cin, 3, 3] of an Upsample block -> [4, Cout, 4*Cin] bf16 for conv_up2x: phase (a, b) = (row, column parity of
    the output pixel) sees the source rows {i + a - 1, i + a}; of the three kernel rows ky, those that land on the same source row are
    summed (a = 0: {0}, {1, 2}; a = 1: {0, 1}, {2}), likewise the columns -- fp32 sums, one rounding.  K order as pack_conv_weight with
    tap slot t = 2 ty + tx."""
    cout, cin, kh, kw = w.shape
    assert kh == 3 and kw == 3 and cin % 64 == 0
    w32 = w.detach().float()
    sets = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}
    g = _lib.load().cd360_conv_k_order(cin, 9)
    phases = []
    for a in (0, 1):
        for b in (0, 1):
            taps = [sum(w32[:, :, ky, kx] for ky in sets[a][ty] for kx in sets[b][tx]) for ty in (0, 1) for tx in (0, 1)]  # 4 x [Cout, Cin]
            we = torch.stack(taps, -1)  # [Cout, Cin, 4]
            wp = we.reshape(cout, cin // (64 * g), g, 64, 4).permute(0, 1, 4, 2, 3)  # [co, group, tap, chunk-in-group, 64]
            phases.append(wp.reshape(cout, -1))
    return torch.stack(phases, 0).to(torch.bfloat16).contiguous()


def conv_up2x(x: torch.Tensor, w_phases: torch.Tensor, bias: Optional[torch.Tensor], N: int, H: int, W: int) -> torch.Tensor:
    """Upsample.forward: nearest 2x + conv3x3 in one launch (cd360_conv_up2x_bf16).  x [N, H*W, Cin] channels-last bf16 (the SOURCE
    image), w_phases from pack_upsample_conv_weight -> [N, 4*H*W, Cout] (the 2H x 2W image).  Forward only."""
    _need_gpu(x, w_phases, bias)
    cin = x.shape[-1]
    cout = w_phases.shape[1]
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and x.numel() == N * H * W * cin
    assert w_phases.dtype == torch.bfloat16 and w_phases.is_contiguous() and w_phases.shape == (4, cout, 4 * cin)
    assert bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == cout)
    out = torch.empty(N, 4 * H * W, cout, dtype=torch.bfloat16, device=x.device)
    m = N * H * W
    # algorithmic accounting = the operator replaced: a 3 x 3 convolution over the 2H x 2W image (what the reference computes)
    with _timed("conv_igemm", 2.0 * 4 * m * 9 * cin * cout, 2.0 * (m * cin + 4 * m * cout + 9 * cin * cout)):
        check(_lib.load().cd360_conv_up2x_bf16(_ptr(x), _ptr(w_phases), _ptr(bias), _ptr(out), N, H, W, cin, cout, _stream()), "cd360_conv_up2x_bf16")
    return out


# ----------------------------------------------------------------------------------------------- Linear layers (cd360_gemm_bf16)
def _rows2d(t: torch.Tensor):
    """(rows, row stride) of a bf16 tensor [..., C] whose leading dims collapse to uniformly strided rows (last dim contiguous)."""
    assert t.dtype == torch.bfloat16 and t.stride(-1) == 1, "bf16 with a contiguous last dim"
    rows, ld = 1, None
    for size, stride in zip(reversed(t.shape[:-1]), reversed(t.stride()[:-1])):
        if size == 1:
            continue
        if ld is None:
            ld = stride
        elif stride != rows * ld:
            raise Cd360Error("cd360 gemm: the leading dims do not collapse to uniformly strided rows")
        rows *= size
    return rows, (t.shape[-1] if ld is None else ld)


def gemm_tile_n(M: int, N: int) -> int:
    _lib.query_stream(_stream())
    return _lib.load().cd360_gemm_tile_n(M, N)


def pack_ln_linear(weight: torch.Tensor, bias: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor):
    """LayerNorm(gamma, beta) followed by Linear(weight, bias), folded for gemm(..., ln=...): -> (w' bf16 = weight * gamma,
    wsum fp32 = rowsum(w') of the ROUNDED w', cb fp32 = weight @ beta + bias)."""
    w32 = weight.detach().float()
    wp = (w32 * gamma.detach().float()[None, :]).to(torch.bfloat16).contiguous()
    cb = w32 @ beta.detach().float()
    if bias is not None:
        cb = cb + bias.detach().float()
    return wp, wp.float().sum(1).contiguous(), cb.contiguous()


def geglu_row_order(inner: int, device=None) -> torch.Tensor:
    """Row permutation of a GEGLU projection [2*inner, K] (value rows | gate rows) for gemm(..., geglu=True): per 32 output columns
    the 32 value rows then the 32 gate rows."""
    assert inner % 32 == 0
    g = torch.arange(inner // 32, device=device)[:, None] * 32 + torch.arange(32, device=device)[None, :]
    return torch.cat([g, g + inner], 1).reshape(-1)


def row_stats(x: torch.Tensor) -> torch.Tensor:
    """x [..., C] bf16 -> fp32 [rows, 1, 2] (sum, sum of squares) per row: LayerNorm statistics input of gemm(..., ln=...)."""
    _need_gpu(x)
    rows, ld = _rows2d(x)
    C = x.shape[-1]
    st = torch.empty(rows, 1, 2, dtype=torch.float32, device=x.device)
    with _timed("row_stats", 0.0, 2.0 * rows * C):
        check(_lib.load().cd360_row_stats_bf16(_ptr(x), _ptr(st), rows, C, ld, _stream()), "cd360_row_stats_bf16")
    return st


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None, ln=None,
         want_stats: bool = False, geglu: bool = False, out: Optional[torch.Tensor] = None):
    """a [..., K] @ w[N, K]^T with the fused epilogues of cd360_gemm_bf16 -> out [..., N] (N / 2 with geglu), bf16.
    bias fp32 [N]; res bf16 [..., N]; ln = (stats fp32 [rows, parts, 2], wsum fp32 [N], eps) with w / bias from pack_ln_linear;
    want_stats=True returns (out, stats fp32 [rows, parts_out, 2]) for the next LayerNorm fold.  Not recorded by autograd: the
    differentiable form is linear() (grad.LinearFn)."""
    _need_gpu(a, w, bias, res)
    M, lda = _rows2d(a)
    K = a.shape[-1]
    N = w.shape[0]
    assert w.dtype == torch.bfloat16 and w.dim() == 2 and w.shape[1] == K and w.stride(1) == 1
    assert bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == N)
    nout = N // 2 if geglu else N
    if out is None:
        out = torch.empty(*a.shape[:-1], nout, dtype=torch.bfloat16, device=a.device)
    mo, ldo = _rows2d(out)
    assert mo == M and out.shape[-1] == nout
    ldr = 0
    if res is not None:
        mr, ldr = _rows2d(res)
        assert mr == M and res.shape[-1] == N
    stats_in = wsum = None
    parts = ln_dim = 0
    eps = 0.0
    if ln is not None:
        stats_in, wsum, eps = ln
        assert stats_in.dtype == torch.float32 and stats_in.is_contiguous() and stats_in.shape[0] == M and stats_in.shape[2] == 2
        assert wsum.dtype == torch.float32 and wsum.is_contiguous() and wsum.numel() == N
        parts, ln_dim = stats_in.shape[1], K
    lib = _lib.load()
    stats_out = None
    if want_stats:
        _lib.query_stream(_stream())
        tn = lib.cd360_gemm_tile_n(M, N)
        stats_out = torch.empty(M, (N + tn - 1) // tn, 2, dtype=torch.float32, device=a.device)
    with _timed(_shape_tag("gemm8p", M, N, K), 2.0 * M * N * K, 2.0 * (M * K + N * K + M * nout + (M * N if res is not None else 0))):
        check(lib.cd360_gemm_bf16(_ptr(a), _ptr(w), _ptr(out), M, N, K, lda, w.stride(0), ldo, _ptr(bias), _ptr(res), ldr, _ptr(stats_in), parts,
                                  ln_dim, float(eps), _ptr(wsum), _ptr(stats_out), 1 if geglu else 0, _stream()), "cd360_gemm_bf16")
    return (out, stats_out) if want_stats else out


def gemm_ok(M: int, N: int, K: int, lda: Optional[int] = None, ldw: Optional[int] = None) -> bool:
    """Shape envelope of cd360_gemm_bf16 (K % 64, N % 16, 32-bit buffer offsets): callers outside it keep their tensors on torch."""
    lda, ldw = (K if lda is None else lda), (K if ldw is None else ldw)
    return (M > 0 and K > 0 and N > 0 and K % 64 == 0 and N % 16 == 0 and lda % 8 == 0 and ldw % 8 == 0 and M < 2 ** 31
            and (M + 256) * lda * 2 < 2 ** 32 and (N + 256) * ldw * 2 < 2 ** 32)


_F32_CACHE = {}  # id(tensor) -> (weakref, version, data_ptr, dtype, fp32 copy): biases of frozen Linears as the fp32 vectors the GEMM epilogue reads
_WT_CACHE = {}   # id(weight) -> (weakref, version, data_ptr, dtype, weight^T contiguous): the data-gradient GEMM's operand


def _cached(cache: dict, t: torch.Tensor, make):
    import weakref
    # a view (`w[:, :c]` of pose_emb_layers is a fresh tensor object on every call) or a trainable tensor gains nothing from an id-keyed
    # cache and would leave one dead entry per call behind: compute directly
    if t.requires_grad or t._base is not None:
        return make(t)
    ent = cache.get(id(t))
    if ent is not None and ent[0]() is t and ent[1] == t._version and ent[2] == t.data_ptr() and ent[3] == t.dtype:  # the rule of cd360.derived
        return ent[4]
    if len(cache) > 4096:  # entries of tensors that died (ids are reused): drop them
        for k in [k for k, e in cache.items() if e[0]() is None]:
            del cache[k]
    val = make(t)
    cache[id(t)] = (weakref.ref(t), t._version, t.data_ptr(), t.dtype, val)
    return val


def bias_f32(b: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if b is None or (b.dtype == torch.float32 and b.is_contiguous() and not b.requires_grad):
        return b
    return _cached(_F32_CACHE, b, lambda t: t.detach().float().contiguous())


def weight_t(w: torch.Tensor) -> torch.Tensor:
    """w [N, K] -> w^T [K, N] contiguous bf16, cached per (tensor, version): dX = dY W is cd360_gemm_bf16(dY, W^T)."""
    return _cached(_WT_CACHE, w, lambda t: t.detach().t().contiguous())


def linear_ok(x: torch.Tensor, weight: torch.Tensor) -> bool:
    """True when F.linear(x, weight) can run on cd360_gemm_bf16 (bf16 on the GPU, inside the kernel's shape envelope)."""
    if not (x.is_cuda and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and weight.dim() == 2 and x.shape[-1] == weight.shape[1]):
        return False
    N, K = weight.shape
    M = x.numel() // max(K, 1)
    return gemm_ok(M, N, K)


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.linear(x, weight, bias) (+ res) on the hand-written MFMA GEMM, in every mode: no tape -> one cd360_gemm_bf16 launch; under
    autograd -> grad.LinearFn (forward the same launch; data gradient the same kernel on W^T; weight gradient cd360_gemm_tn_bf16).
    The one Linear of every route: the fused inference blocks, the plain module route (sample.py's patched forwards, hooks) and the
    fine-tuning step all end here.  x [..., K] bf16, weight [N, K] bf16 (nn.Linear layout); bias any float dtype."""
    assert linear_ok(x, weight), "cd360 linear: bf16 GPU tensors with K % 64 == 0 and N % 16 == 0 (use linear_ok() to test)"
    if x.stride(-1) != 1:
        x = x.contiguous()
    try:
        _rows2d(x)
    except Cd360Error:
        x = x.contiguous()
    if res is not None and (res.dtype != torch.bfloat16 or res.stride(-1) != 1):
        res = res.to(torch.bfloat16).contiguous()
    if _wants_grad(x, weight, bias, res):
        # the autograd node in C++ (cd360/_host.py: the same launches without ~90 us of interpreter time per Linear forward + backward);
        # the Python node serves profiling runs (per-launch events), the A/B switch, and trees where the glue was not built
        if _PROF is None and not routes.no_host_glue:
            host = _host.get()
            if host is not None:
                return host.linear(x, weight, bias, res)
        from . import grad
        return grad.LinearFn.apply(x, weight, bias, res)
    w = weight.detach()
    if w.stride(1) != 1 or w.stride(0) % 8:
        w = w.contiguous()
    return gemm(x.detach(), w, bias=bias_f32(bias), res=None if res is None else res.detach())


def gemm_tn(a: torch.Tensor, b: torch.Tensor, out_dtype=torch.bfloat16) -> torch.Tensor:
    """a [M, N]^T @ b [M, K] -> [N, K] (fp32 accumulation; cd360_gemm_tn_bf16): the weight gradient dW = dY^T X of a Linear.
    a, b bf16 with contiguous last dims and uniform row strides (multiples of 8); N, K multiples of 8.  Deterministic."""
    _need_gpu(a, b)
    M, lda = _rows2d(a)
    Mb, ldb = _rows2d(b)
    N, K = a.shape[-1], b.shape[-1]
    assert M == Mb and out_dtype in (torch.bfloat16, torch.float32)
    lib = _lib.load()
    out = torch.empty(N, K, dtype=out_dtype, device=a.device)
    ws = torch.empty(max(16, lib.cd360_gemm_tn_workspace_bytes(M, N, K)), dtype=torch.uint8, device=a.device)
    with _timed(_shape_tag("gemm_tn", M, N, K), 2.0 * M * N * K, 2.0 * (M * N + M * K) + out.element_size() * N * K):
        check(lib.cd360_gemm_tn_bf16(_ptr(a), _ptr(b), _ptr(out), M, N, K, lda, ldb, 1 if out_dtype == torch.bfloat16 else 0, _ptr(ws), _stream()),
              "cd360_gemm_tn_bf16")
    return out


ADAMW_MAX_TENSORS = 64  # CD360_ADAMW_MAX_TENSORS of include/cd360_hip.h


class AdamwPlan:
    """Host-side argument arrays of cd360_adamw_bf16 for a fixed list of bf16 parameters whose fp32 master / exp_avg / exp_avg_sq live
    at offsets `begin` of three flat buffers: offsets, sizes, learning rates and decays are built once; the gradient AND parameter
    pointers are refreshed on every step (a parameter whose storage was replaced -- `p.data = ...` -- must not be written through a
    stale address)."""

    def __init__(self, params, begin, lr, wd):
        self.n = len(params)
        self.params = list(params)
        assert all(p.dtype == torch.bfloat16 and p.is_contiguous() for p in self.params)
        self.chunks = []
        for c0 in range(0, self.n, ADAMW_MAX_TENSORS):
            idx = list(range(c0, min(self.n, c0 + ADAMW_MAX_TENSORS)))
            k = len(idx)
            self.chunks.append(dict(
                idx=idx, k=k, grads=(ctypes.c_void_p * k)(), params=(ctypes.c_void_p * k)(*[params[i].data_ptr() for i in idx]),
                begin=(ctypes.c_int64 * k)(*[int(begin[i]) for i in idx]), numel=(ctypes.c_int64 * k)(*[params[i].numel() for i in idx]),
                lr=(ctypes.c_float * k)(*[float(lr[i]) for i in idx]), wd=(ctypes.c_float * k)(*[float(wd[i]) for i in idx])))


def adamw_step(plan: AdamwPlan, grads, master: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, step: torch.Tensor,
               beta1: float, beta2: float, eps: float) -> None:
    """One AdamW step of every tensor of `plan` (cd360_adamw_tick + cd360_adamw_bf16): `grads` are the bf16 gradients in plan order
    (contiguous), `step` the fp32 device scalar holding the number of steps taken so far."""
    _need_gpu(master, exp_avg, exp_avg_sq, step, *grads)
    lib = _lib.load()
    assert len(grads) == plan.n and all(g.dtype == torch.bfloat16 and g.is_contiguous() for g in grads)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (master, exp_avg, exp_avg_sq, step))
    check(lib.cd360_adamw_tick(_ptr(step), _stream()), "cd360_adamw_tick")
    total = sum(g.numel() for g in grads)
    with _timed("adamw", 0.0, 28.0 * total):
        for c in plan.chunks:
            for j, i in enumerate(c["idx"]):
                c["grads"][j] = grads[i].data_ptr()
                c["params"][j] = plan.params[i].data_ptr()
                assert grads[i].numel() == c["numel"][j] == plan.params[i].numel()
            check(lib.cd360_adamw_bf16(c["k"], c["grads"], c["params"], c["begin"], c["numel"], c["lr"], c["wd"], _ptr(master), _ptr(exp_avg),
                                       _ptr(exp_avg_sq), _ptr(step), beta1, beta2, eps, _stream()), "cd360_adamw_bf16")


# ----------------------------------------------------------------------------------------------- live optimiser step (include/optim/cd360_optim.h)
# libcd360_optim.so through cd360/_optim.py: AdamwPlan / adamw_step above stay what they were.
OPTIM_SUMSQ_VECS = 2048  # CD360_OPTIM_SUMSQ_VECS of include/optim/cd360_optim.h: 8-value vectors per workgroup, one partial each
OPTIM_SUMSQ_TERMS = 64  # CD360_OPTIM_SUMSQ_TERMS: squares one thread adds before the workgroup's tree
OPTIM_SUMSQ_DEPTH = 6  # CD360_OPTIM_SUMSQ_DEPTH: additions a square passes through inside its thread (a balanced tree)


def sumsq_partials(numels) -> int:
    """Partials one cd360_grad_sumsq_bf16 launch over tensors of these sizes writes (the header's formula)."""
    return (sum((int(n) + 7) // 8 for n in numels) + OPTIM_SUMSQ_VECS - 1) // OPTIM_SUMSQ_VECS


class LiveAdamwPlan:
    """Host-side argument arrays of cd360_grad_sumsq_bf16 / cd360_adamw_live_bf16 for a fixed list of bf16 parameters: what AdamwPlan holds,
    with each tensor's row of the device (lr, weight decay) table in place of the values, and each chunk's slice of the partial sums
    (`part0`, `parts`; `npartials` in all).  Gradient and parameter pointers are refreshed on every step, as there."""

    def __init__(self, params, begin, rows):
        self.n = len(params)
        self.params = list(params)
        assert all(p.dtype == torch.bfloat16 and p.is_contiguous() for p in self.params)
        self.chunks, self.npartials = [], 0
        for c0 in range(0, self.n, ADAMW_MAX_TENSORS):
            idx = list(range(c0, min(self.n, c0 + ADAMW_MAX_TENSORS)))
            k = len(idx)
            parts = sumsq_partials(params[i].numel() for i in idx)
            self.chunks.append(dict(
                idx=idx, k=k, grads=(ctypes.c_void_p * k)(), params=(ctypes.c_void_p * k)(*[params[i].data_ptr() for i in idx]),
                begin=(ctypes.c_int64 * k)(*[int(begin[i]) for i in idx]), numel=(ctypes.c_int64 * k)(*[params[i].numel() for i in idx]),
                row=(ctypes.c_int32 * k)(*[int(rows[i]) for i in idx]), part0=self.npartials, parts=parts))
            self.npartials += parts

    def refresh(self, grads) -> None:
        assert len(grads) == self.n and all(g.dtype == torch.bfloat16 and g.is_contiguous() for g in grads)
        for c in self.chunks:
            for j, i in enumerate(c["idx"]):
                c["grads"][j] = grads[i].data_ptr()
                c["params"][j] = self.params[i].data_ptr()
                assert grads[i].numel() == c["numel"][j] == self.params[i].numel()


def grad_clip_coef(plan: LiveAdamwPlan, grads, partials: torch.Tensor, max_norm: float, out: torch.Tensor) -> torch.Tensor:
    """out[4] fp32 <- (sumsq, norm, coef, 0) of the bf16 gradients `grads` (plan order, contiguous): cd360_grad_sumsq_bf16 per chunk into
    its slice of `partials` (fp32, at least plan.npartials entries; every entry read is written first), then cd360_grad_clip_f32 with
    coef = min(1, max_norm / (norm + 1e-6)), torch.nn.utils.clip_grad_norm_'s rule.  No host read; bit-reproducible."""
    from . import _optim
    _refuse(not (float(max_norm) >= 0.0), f"max_norm must be >= 0, got {max_norm}")
    _refuse(partials.dtype != torch.float32 or not partials.is_contiguous() or partials.numel() < plan.npartials,
            f"partials: contiguous fp32 with at least {plan.npartials} entries is needed")
    _refuse(out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != 4 or out.data_ptr() % 16 != 0, "out: 4 contiguous fp32 values, 16-byte aligned")
    _refuse(_overlaps(out, partials), "out overlaps partials")
    _need_gpu(partials, out, *grads)
    lib = _optim.load()
    plan.refresh(grads)
    with _timed("grad_sumsq", 0.0, 2.0 * sum(g.numel() for g in grads)):
        for c in plan.chunks:
            check(lib.cd360_grad_sumsq_bf16(c["k"], c["grads"], c["numel"], partials.data_ptr() + 4 * c["part0"], _stream()), "cd360_grad_sumsq_bf16")
    check(lib.cd360_grad_clip_f32(_ptr(partials), plan.npartials, float(max_norm), _ptr(out), _stream()), "cd360_grad_clip_f32")
    return out


def adamw_live_step(plan: LiveAdamwPlan, grads, hyper: torch.Tensor, master: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
                    step: torch.Tensor, beta1: float, beta2: float, eps: float, coef: Optional[torch.Tensor] = None,
                    ema: Optional[torch.Tensor] = None, ema_decay: float = 0.0) -> None:
    """One AdamW step of every tensor of `plan` (cd360_adamw_tick + cd360_adamw_live_bf16): adamw_step with lr / weight decay read on the
    device from `hyper` [rows, 2] fp32, the gradient scaled by the device scalar `coef` (None: as it is) and `ema` (flat fp32 like
    `master`; None: none) moved towards the new master with decay min(ema_decay, (1 + t) / (10 + t)), t = the step count after the tick."""
    from . import _optim
    flat = (master, exp_avg, exp_avg_sq) + (() if ema is None else (ema,))
    _refuse(any(t.dtype != torch.float32 or not t.is_contiguous() for t in flat + (step, hyper) + (() if coef is None else (coef,))),
            "master, exp_avg, exp_avg_sq, ema, step, hyper and coef must be contiguous fp32 tensors")
    _refuse(hyper.ndim != 2 or hyper.shape[1] != 2 or hyper.shape[0] < 1, f"hyper: [rows, 2] is needed, got {tuple(hyper.shape)}")
    _refuse(any(t.numel() != master.numel() for t in flat), "master, exp_avg, exp_avg_sq and ema must have one length")
    _refuse(coef is not None and coef.numel() != 1, "coef: one fp32 value")
    _refuse(ema is not None and any(_overlaps(ema, t) for t in (master, exp_avg, exp_avg_sq)), "ema overlaps master or a moment")
    _need_gpu(*flat, step, hyper, coef, *grads)
    first, lib = _lib.load(), _optim.load()
    plan.refresh(grads)
    check(first.cd360_adamw_tick(_ptr(step), _stream()), "cd360_adamw_tick")
    total = sum(g.numel() for g in grads)
    with _timed("adamw_live", 0.0, (28.0 if ema is None else 36.0) * total):
        for c in plan.chunks:
            check(lib.cd360_adamw_live_bf16(c["k"], c["grads"], c["params"], c["begin"], c["numel"], c["row"], _ptr(hyper), hyper.shape[0], _ptr(coef),
                                            _ptr(master), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(ema), float(ema_decay), _ptr(step), beta1, beta2,
                                            eps, _stream()), "cd360_adamw_live_bf16")


def gemm_tn_ok(a: torch.Tensor, b: torch.Tensor) -> bool:
    if not (a.is_cuda and a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16 and a.stride(-1) == 1 and b.stride(-1) == 1):
        return False
    try:
        M, lda = _rows2d(a)
        Mb, ldb = _rows2d(b)
    except Cd360Error:
        return False
    N, K = a.shape[-1], b.shape[-1]
    return (M == Mb and N % 8 == 0 and K % 8 == 0 and lda % 8 == 0 and ldb % 8 == 0 and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
            and (M + 64) * lda * 2 < 2 ** 31 and (M + 64) * ldb * 2 < 2 ** 31)


def gemm_cstats(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None):
    """gemm(a, w, bias, res) for an output a GroupNorm reads next: -> (out, cstats) with cstats fp32 [rows / S, N, 2] = per slab of S = 64
    or 32 rows (cd360_gemm_cstats_rows: the tiling decides) and channel the (sum, sum of squares) of the stored outputs (gn_silu's
    tile_stats after a reshape to [images, slabs, N, 2]); cstats is None when the tiling chosen for this shape writes no slabs or
    rows % 64 != 0 (plain gemm then)."""
    _need_gpu(a, w, bias, res)
    M, lda = _rows2d(a)
    K, N = a.shape[-1], w.shape[0]
    lib = _lib.load()
    _lib.query_stream(_stream())
    slab = lib.cd360_gemm_cstats_rows(M, N)
    if M % 64 or slab <= 0:
        return gemm(a, w, bias=bias, res=res), None
    assert w.dtype == torch.bfloat16 and w.dim() == 2 and w.shape[1] == K and w.stride(1) == 1
    assert bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == N)
    out = torch.empty(*a.shape[:-1], N, dtype=torch.bfloat16, device=a.device)
    ldr = 0
    if res is not None:
        mr, ldr = _rows2d(res)
        assert mr == M and res.shape[-1] == N
    cstats = torch.empty(M // slab, N, 2, dtype=torch.float32, device=a.device)
    with _timed(_shape_tag("gemm8p", M, N, K), 2.0 * M * N * K, 2.0 * (M * K + N * K + M * N + (M * N if res is not None else 0))):
        check(lib.cd360_gemm_cstats_bf16(_ptr(a), _ptr(w), _ptr(out), M, N, K, lda, w.stride(0), N, _ptr(bias), _ptr(res), ldr, _ptr(cstats), _stream()),
              "cd360_gemm_cstats_bf16")
    return out, cstats


def qproj_attention_ok(a: torch.Tensor, nk: int) -> bool:
    """Shape envelope of qproj_attention: [b, Nq, K] queries with Nq % 128 == 0 (a token tile stays inside one batch element),
    K % 64 == 0, at most 96 keys."""
    return a.dim() == 3 and a.shape[1] % 128 == 0 and a.shape[2] % 64 == 0 and nk <= 96


def kv_pack_fp8(k: torch.Tensor, v: torch.Tensor, nk: int, heads: int, out=None):
    """k, v bf16 [B, >= nk, heads*64] (last dim contiguous) -> (kv8 uint8 [B, heads, 14336], scales fp32 [B, heads, 2]): the OCP e4m3
    image of K and V^T that cd360_qproj_attn_fp8_bf16 copies into its LDS (cd360_kv_pack_fp8; BASELINE configs[4]).  Once per image:
    the text context is constant over a trajectory.  `out` = (kv8, scales) buffers to write into."""
    _need_gpu(k, v)
    B = k.shape[0]
    assert k.dtype == torch.bfloat16 and v.dtype == torch.bfloat16 and k.shape[-1] == heads * 64 and v.shape[-1] == heads * 64
    assert k.stride(2) == 1 and v.stride(2) == 1 and k.shape[1] >= nk and v.shape[1] >= nk and v.shape[0] == B and nk <= 96
    if out is None:
        kv8 = torch.empty(B, heads, 96 * 64 + 64 * 128, dtype=torch.uint8, device=k.device)
        scales = torch.empty(B, heads, 2, dtype=torch.float32, device=k.device)
    else:  # buffers that stay put (a captured graph re-packs into them on every replay of the render step)
        kv8, scales = out
        assert kv8.shape == (B, heads, 96 * 64 + 64 * 128) and kv8.dtype == torch.uint8 and scales.shape == (B, heads, 2) and scales.dtype == torch.float32
    assert kv8.numel() == _lib.load().cd360_kv_fp8_bytes(B, heads)
    check(_lib.load().cd360_kv_pack_fp8(_ptr(k), _ptr(v), _ptr(kv8), _ptr(scales), B, heads, nk, k.stride(0), k.stride(1), v.stride(0), v.stride(1),
                                        _stream()), "cd360_kv_pack_fp8")
    return kv8, scales


def qproj_attention(a: torch.Tensor, w: torch.Tensor, k: torch.Tensor, v: torch.Tensor, nk: int, heads: int,
                    bias: Optional[torch.Tensor] = None, ln=None, dup: int = 0, tag: str = "qproj_attn", fp8=None) -> torch.Tensor:
    """softmax((a w^T [+ LayerNorm fold, + bias]) k^T / 8) v per head with the query projection and the attention in ONE kernel
    (cd360_qproj_attn_bf16): a [b, Nq, K] bf16, w [heads*64, K] bf16, k / v [b, >= nk, heads*64] (last dim contiguous, e.g. the two
    halves of the merged k|v projection), nk <= 96 -> [b, Nq, heads*64].  bias / ln as gemm().  Forward only.
    dup > 0 (cd360_qproj_attn_dedup_bf16): k / v hold b + dup batch elements; the last `dup` query elements attend to the keys of their own
    batch index AND of index + dup -> [b + dup, Nq, heads*64] (the de-duplicated third of a 3-way CFG batch: q projected once)."""
    _need_gpu(a, w, bias)
    b, nq, K = a.shape
    N = heads * 64
    M, lda = _rows2d(a)
    assert w.dtype == torch.bfloat16 and w.shape == (N, K) and w.stride(1) == 1
    assert 0 <= dup <= b and qproj_attention_ok(a, nk)
    if fp8 is None:
        _need_gpu(k, v)
        assert k.dtype == torch.bfloat16 and v.dtype == torch.bfloat16 and k.shape[0] == b + dup and v.shape[0] == b + dup and k.shape[-1] == N and v.shape[-1] == N
        assert k.stride(2) == 1 and v.stride(2) == 1 and k.shape[1] >= nk and v.shape[1] >= nk
    else:  # (kv8, scales) of kv_pack_fp8: both attention contractions on fp8 MFMA (cd360_qproj_attn_fp8_bf16); k, v are not read
        kv8, kvs = fp8
        _need_gpu(kv8, kvs)
        assert kv8.dtype == torch.uint8 and kv8.is_contiguous() and kv8.shape == (b + dup, heads, 96 * 64 + 64 * 128)
        assert kvs.dtype == torch.float32 and kvs.is_contiguous() and kvs.shape == (b + dup, heads, 2)
    assert bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == N)
    stats_in = wsum = None
    parts = ln_dim = 0
    eps = 0.0
    if ln is not None:
        stats_in, wsum, eps = ln
        assert stats_in.dtype == torch.float32 and stats_in.is_contiguous() and stats_in.shape[0] == M and stats_in.shape[2] == 2
        assert wsum.dtype == torch.float32 and wsum.is_contiguous() and wsum.numel() == N
        parts, ln_dim = stats_in.shape[1], K
    out = torch.empty(b + dup, nq, N, dtype=torch.bfloat16, device=a.device)
    flops = 2.0 * M * N * K + 4.0 * (M + dup * nq) * nk * N
    if fp8 is not None:
        with _timed(tag, flops, 2.0 * (M * K + N * K + M * N) + 2.0 * b * nk * N):
            check(_lib.load().cd360_qproj_attn_fp8_bf16(_ptr(a), _ptr(w), _ptr(out), M, N, K, lda, w.stride(0), N, _ptr(bias), _ptr(stats_in), parts,
                                                       ln_dim, float(eps), _ptr(wsum), _ptr(fp8[0]), _ptr(fp8[1]), nq, nk, 64 ** -0.5, dup,
                                                       _stream()), "cd360_qproj_attn_fp8_bf16")
        return out
    with _timed(tag, flops, 2.0 * (M * K + N * K + M * N + 2 * b * nk * N)):  # per-kernel timing name: A3 "qproj_attn", A2 "qproj_attn_text"
        check(_lib.load().cd360_qproj_attn_dedup_bf16(_ptr(a), _ptr(w), _ptr(out), M, N, K, lda, w.stride(0), N, _ptr(bias), _ptr(stats_in), parts,
                                                     ln_dim, float(eps), _ptr(wsum), _ptr(k), _ptr(v), k.stride(0), k.stride(1), v.stride(0),
                                                     v.stride(1), nq, nk, 64 ** -0.5, dup, _stream()), "cd360_qproj_attn_dedup_bf16")
    return out


def pose_embed(x: torch.Tensor, xref: torch.Tensor, wa: torch.Tensor, wb: torch.Tensor) -> torch.Tensor:
    """pose_emb_layers(cat[x, xref]) (attention.py:634) as x wa^T + xref wb^T through the C ABI (cd360_pose_embed_bf16); wa = W[:, :C],
    wb = W[:, C:], contiguous.  Forward-only operator-level entry (the modules run the same two products on the library GEMM, which
    torch differentiates)."""
    _need_gpu(x, xref, wa, wb)
    C = x.shape[-1]
    for t in (x, xref, wa, wb):
        assert t.dtype == torch.bfloat16 and t.is_contiguous()
    assert xref.shape == x.shape and wa.shape == (C, C) and wb.shape == (C, C)
    out = torch.empty_like(x)
    rows = x.numel() // C
    with _timed("pose_embed", 4.0 * rows * C * C, 2.0 * (3 * rows * C + 2 * C * C)):
        check(_lib.load().cd360_pose_embed_bf16(_ptr(x), _ptr(xref), _ptr(wa), _ptr(wb), _ptr(out), rows, C, _stream()), "cd360_pose_embed_bf16")
    return out


def add_layernorm(a: torch.Tensor, b: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor, eps: float, want_sum: bool = True,
                  alias: bool = False):
    """(a + b, LayerNorm(a + b) * gamma + beta) in one pass; b None -> (None, LayerNorm(a)).  All bf16, last dim C.
    Differentiable with respect to a and b (grad.AddLayerNormFn).  alias (only with b None): the first result is `a` again -- under
    autograd an alias whose gradient the LayerNorm backward kernel adds in its own pass; use it as the residual stream from here on."""
    if _wants_grad(a, b, gamma, beta):
        from . import grad
        return grad.add_layernorm(a, b, gamma, beta, eps, want_sum, alias)
    _need_gpu(a, b, gamma, beta)
    C = a.shape[-1]
    assert a.dtype == torch.bfloat16 and a.is_contiguous() and gamma.dtype == torch.bfloat16 and beta.dtype == torch.bfloat16
    assert b is None or (b.dtype == torch.bfloat16 and b.is_contiguous() and b.shape == a.shape)
    rows = a.numel() // C
    s = torch.empty_like(a) if (b is not None and want_sum) else None
    ln = torch.empty_like(a)
    with _timed("add_layernorm", 0.0, 2.0 * rows * C * (2 + (b is not None) + (s is not None))):
        check(_lib.load().cd360_add_layernorm_bf16(_ptr(a), _ptr(b), _ptr(gamma), _ptr(beta), _ptr(s), _ptr(ln), rows, C, float(eps), _stream()),
              "cd360_add_layernorm_bf16")
    return (a if (alias and b is None) else s), ln


def add_layernorm_bwd(x: torch.Tensor, gamma: torch.Tensor, d_ln: torch.Tensor, d_sum: Optional[torch.Tensor], eps: float) -> torch.Tensor:
    """Backward of add_layernorm with respect to the summed input x (= a + b): LayerNorm backward of d_ln plus d_sum."""
    _need_gpu(x, gamma, d_ln, d_sum)
    C = x.shape[-1]
    d_ln = d_ln.contiguous()
    d_sum = None if d_sum is None else d_sum.contiguous()
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and gamma.dtype == torch.bfloat16 and d_ln.dtype == torch.bfloat16 and d_ln.shape == x.shape
    assert d_sum is None or (d_sum.dtype == torch.bfloat16 and d_sum.shape == x.shape)
    rows = x.numel() // C
    dx = torch.empty_like(x)
    with _timed("add_layernorm_bwd", 0.0, 2.0 * rows * C * (3 + (d_sum is not None))):
        check(_lib.load().cd360_add_layernorm_bwd_bf16(_ptr(x), _ptr(gamma), _ptr(d_ln), _ptr(d_sum), _ptr(dx), rows, C, float(eps), _stream()),
              "cd360_add_layernorm_bwd_bf16")
    return dx


def _cfg_branches(scale_im: Optional[float]) -> int:
    """3 (ScheduledCFGImgTextRef: u | ic | c) or, for scale_im=None, 2 (VanillaCFGImgRef: u | c).  The C entry points take the two-branch
    request as a NaN scale_im (include/cd360_hip.h), so a NaN handed in as a NUMBER is refused here rather than read as that request."""
    if scale_im is None:
        return 2
    if math.isnan(float(scale_im)):
        raise ValueError("scale_im is NaN; pass scale_im=None for the two-branch (VanillaCFGImgRef) step")
    return 3


def _cfg_flat_args(x: torch.Tensor, eps: torch.Tensor, scale_im: Optional[float]) -> float:
    """What the flat fp32 tails share: x [n,...] and eps [NB n,...] fp32 contiguous, NB from scale_im -> scale_im as the C ABI takes it."""
    nb = _cfg_branches(scale_im)
    if eps.shape[0] != nb * x.shape[0] or eps.numel() != nb * x.numel():
        raise ValueError(f"eps holds {eps.shape[0]} rows of {tuple(eps.shape[1:])}; the {nb}-branch step on x {tuple(x.shape)} needs {nb * x.shape[0]}")
    assert x.dtype == torch.float32 and eps.dtype == torch.float32 and x.is_contiguous() and eps.is_contiguous()
    return float("nan") if nb == 2 else float(scale_im)


def _cfg_cl_args(x: torch.Tensor, eps_cl: torch.Tensor, step_tab: torch.Tensor, step: torch.Tensor, scale_im: Optional[float]):
    """What the channels-last tails share: x [bs, 4, H, W] fp32 contiguous, eps_cl [NB bs, H W, >= 4] bf16 rows of unit channel stride,
    step_tab [nsteps, 4] fp32, step int32 -> (bs, H W, the row stride of eps_cl, scale_im as the C ABI takes it)."""
    nb = _cfg_branches(scale_im)
    bs = x.shape[0]
    hw = x.shape[2] * x.shape[3]
    if eps_cl.shape[0] != nb * bs:
        raise ValueError(f"eps_cl holds {eps_cl.shape[0]} images; the {nb}-branch step on {bs} latents needs {nb * bs}")
    assert x.dtype == torch.float32 and x.is_contiguous() and x.shape[1] == 4 and eps_cl.dtype == torch.bfloat16
    assert eps_cl.shape[1] == hw and eps_cl.shape[2] >= 4 and eps_cl.stride(2) == 1
    assert step.dtype == torch.int32 and step_tab.dtype == torch.float32 and step_tab.is_contiguous() and step_tab.shape[1] == 4
    ld = eps_cl.stride(1)
    assert eps_cl.stride(0) == hw * ld
    return bs, hw, ld, float("nan") if nb == 2 else float(scale_im)


def _like(x: torch.Tensor, *ts: torch.Tensor):  # fp32 contiguous, shaped like x
    assert all(t.dtype == torch.float32 and t.shape == x.shape and t.is_contiguous() for t in ts)


def _tab_like(ref: torch.Tensor, *tabs: torch.Tensor):  # a solver's table beside the table `ref` the step's row is picked from
    assert all(t.dtype == torch.float32 and t.is_contiguous() and t.shape == ref.shape for t in tabs)


def _row4(*rows: torch.Tensor):  # one 4-float row of a table
    assert all(row.dtype == torch.float32 and row.numel() == 4 and row.is_contiguous() for row in rows)


def _scalar(*ts: torch.Tensor):  # a 1-element fp32 tensor (sigma)
    assert all(t.dtype == torch.float32 and t.numel() == 1 for t in ts)


def cfg_euler_step(x: torch.Tensor, eps: torch.Tensor, sigma: torch.Tensor, sigma_next: torch.Tensor, scale: float, scale_im: Optional[float]):
    """x [n,...] fp32, eps [3n,...] fp32 (u | ic | c) or, with scale_im=None, [2n,...] (u | c), sigma / sigma_next 0-d fp32 device tensors
    -> Euler-updated x (one kernel)."""
    _need_gpu(x, eps, sigma, sigma_next)
    sim = _cfg_flat_args(x, eps, scale_im)
    _scalar(sigma, sigma_next)
    out = torch.empty_like(x)
    check(_lib.load().cd360_cfg_euler_step_f32(_ptr(x), _ptr(eps), _ptr(sigma), _ptr(sigma_next), float(scale), sim, _ptr(out), x.numel(),
                                              _stream()), "cd360_cfg_euler_step_f32")
    return out


def unet_stage_in(x: torch.Tensor, step_tab: torch.Tensor, step: torch.Tensor, w_k36: torch.Tensor, bias: torch.Tensor, temb_tab: torch.Tensor,
                  lab: torch.Tensor, h: torch.Tensor, emb_act: torch.Tensor):
    """Head of a captured sampling step (cd360_unet_stage_in): x [bs, 4, H, W] fp32 -> h [rep bs, H W, Cout] bf16 = the UNet's input
    convolution of bf16(c_in x) written to every CFG branch, emb_act [rep bs, E] bf16 = silu(temb_tab[step] + lab); c_in = step_tab[step][2]."""
    _need_gpu(x, step_tab, step, w_k36, bias, temb_tab, lab, h, emb_act)
    bs, four, H, W = x.shape
    rep = lab.shape[0] // bs
    cout, E = w_k36.shape[1], temb_tab.shape[1]
    assert four == 4 and x.dtype == torch.float32 and x.is_contiguous() and step.dtype == torch.int32 and step_tab.dtype == torch.float32
    assert w_k36.shape[0] == 36 and w_k36.dtype == torch.float32 and bias.dtype == torch.float32 and w_k36.is_contiguous()
    assert temb_tab.dtype == lab.dtype == h.dtype == emb_act.dtype == torch.bfloat16 and lab.shape == emb_act.shape == (rep * bs, E)
    assert h.shape == (rep * bs, H * W, cout) and h.is_contiguous() and temb_tab.is_contiguous() and lab.is_contiguous() and emb_act.is_contiguous()
    check(_lib.load().cd360_unet_stage_in(_ptr(x), _ptr(step_tab), _ptr(step), _ptr(w_k36), _ptr(bias), _ptr(h), _ptr(temb_tab), _ptr(lab),
                                         _ptr(emb_act), bs, rep, H, W, cout, E, _stream()), "cd360_unet_stage_in")
    return h, emb_act


def cfg_euler_step_cl(x: torch.Tensor, eps_cl: torch.Tensor, step_tab: torch.Tensor, step: torch.Tensor, scale: float, scale_im: Optional[float]):
    """Tail of a captured sampling step, IN PLACE on x [bs, 4, H, W] fp32: eps_cl [3 bs, H W, >= 4] bf16 channels-last rows (a channel slice
    of wider rows is fine: the row stride is passed) or, with scale_im=None, [2 bs, H W, >= 4] (u | c), sigma / sigma_next =
    step_tab[step][0 / 1]  (cd360_cfg_euler_step_cl)."""
    _need_gpu(x, eps_cl, step_tab, step)
    bs, hw, ld, sim = _cfg_cl_args(x, eps_cl, step_tab, step, scale_im)
    check(_lib.load().cd360_cfg_euler_step_cl(_ptr(x), _ptr(eps_cl), _ptr(step_tab), _ptr(step), float(scale), sim, bs, hw, ld, _stream()),
          "cd360_cfg_euler_step_cl")
    return x


def cfg_dpmpp2m_step(x: torch.Tensor, eps: torch.Tensor, old: torch.Tensor, sigma: torch.Tensor, mult: torch.Tensor, scale: float,
                     scale_im: Optional[float]):
    """One DPM++ 2M tail (cd360_cfg_dpmpp2m_step_f32, include/cd360_solvers.h): x, old [n,...] fp32, eps [3n,...] fp32 (u | ic | c) or, with
    scale_im=None, [2n,...] (u | c), sigma a 1-element and mult = (m1, m2, m3, m4) a 4-element fp32 device tensor -> (x', d0), both new
    tensors.  `old` is not read when m4 == 0."""
    _need_gpu(x, eps, old, sigma, mult)
    sim = _cfg_flat_args(x, eps, scale_im)
    _like(x, old)
    _scalar(sigma)
    _row4(mult)
    out, old_out = torch.empty_like(x), torch.empty_like(x)
    check(_lib.load().cd360_cfg_dpmpp2m_step_f32(_ptr(x), _ptr(eps), _ptr(old), _ptr(sigma), _ptr(mult), float(scale), sim, _ptr(out),
                                                _ptr(old_out), x.numel(), _stream()), "cd360_cfg_dpmpp2m_step_f32")
    return out, old_out


def cfg_dpmpp2m_step_cl(x: torch.Tensor, old: torch.Tensor, eps_cl: torch.Tensor, step_tab: torch.Tensor, mult_tab: torch.Tensor,
                        step: torch.Tensor, scale: float, scale_im: Optional[float]):
    """DPM++ 2M tail of a captured sampling step, IN PLACE on x and old [bs, 4, H, W] fp32 (cd360_cfg_dpmpp2m_step_cl): eps_cl as for
    cfg_euler_step_cl, sigma = step_tab[step][0], (m1, m2, m3, m4) = mult_tab[step]; x <- m1 x - m2 dd, old <- d0.  `old` is not read
    when m4 == 0."""
    _need_gpu(x, old, eps_cl, step_tab, mult_tab, step)
    bs, hw, ld, sim = _cfg_cl_args(x, eps_cl, step_tab, step, scale_im)
    _like(x, old)
    _tab_like(step_tab, mult_tab)
    check(_lib.load().cd360_cfg_dpmpp2m_step_cl(_ptr(x), _ptr(old), _ptr(eps_cl), _ptr(step_tab), _ptr(mult_tab), _ptr(step), float(scale), sim,
                                               bs, hw, ld, _stream()), "cd360_cfg_dpmpp2m_step_cl")
    return x


def _noise_args(seed: torch.Tensor, streams: Optional[torch.Tensor], step: torch.Tensor, bs: int):
    assert seed.dtype == torch.int64 and seed.numel() == 1 and step.dtype == torch.int32 and step.numel() == 1
    assert streams is None or (streams.dtype == torch.int32 and streams.numel() == bs and streams.is_contiguous())


def sampler_noise(seed: torch.Tensor, streams: Optional[torch.Tensor], step: torch.Tensor, bs: int, H: int, W: int) -> torch.Tensor:
    """Standard normals [bs, 4, H, W] fp32 as a pure function of (seed, streams[row], step, channel, pixel): Philox4x32-10 + Box-Muller
    (cd360_sampler_noise_f32, include/cd360_stochastic.h).  seed: device int64[1], step: device int32[1], streams: device int32[bs] or None
    (stream 0 for every row).  Rows of equal stream id hold equal bits whatever bs is."""
    _need_gpu(seed, streams, step)
    _noise_args(seed, streams, step, bs)
    out = torch.empty((bs, 4, H, W), dtype=torch.float32, device=seed.device)
    check(_lib.load().cd360_sampler_noise_f32(_ptr(out), _ptr(seed), _ptr(streams), _ptr(step), bs, H * W, _stream()), "cd360_sampler_noise_f32")
    return out


def cfg_euler_ancestral_step(x: torch.Tensor, eps: torch.Tensor, sigma: torch.Tensor, anc: torch.Tensor, seed: torch.Tensor,
                             streams: Optional[torch.Tensor], step: torch.Tensor, scale: float, scale_im: Optional[float]):
    """One ancestral Euler tail (cd360_cfg_euler_ancestral_step_f32, include/cd360_stochastic.h): x [bs, 4, H, W] fp32, eps [3 bs, 4, H, W]
    fp32 (u | ic | c) or, with scale_im=None, [2 bs, ...] (u | c), sigma a 1-element and anc = (sigma_down, sigma_up, s_noise, 0) a
    4-element fp32 device tensor; the noise is sampler_noise(seed, streams, step, ...), drawn inside the kernel (none when sigma_up == 0)
    -> x', a new tensor."""
    _need_gpu(x, eps, sigma, anc, seed, streams, step)
    sim = _cfg_flat_args(x, eps, scale_im)
    assert x.ndim == 4 and x.shape[1] == 4
    _scalar(sigma)
    _row4(anc)
    bs = x.shape[0]
    _noise_args(seed, streams, step, bs)
    out = torch.empty_like(x)
    check(_lib.load().cd360_cfg_euler_ancestral_step_f32(_ptr(x), _ptr(eps), _ptr(sigma), _ptr(anc), _ptr(seed), _ptr(streams), _ptr(step),
                                                        float(scale), sim, _ptr(out), bs, x.shape[2] * x.shape[3], _stream()),
          "cd360_cfg_euler_ancestral_step_f32")
    return out


def cfg_euler_ancestral_step_cl(x: torch.Tensor, eps_cl: torch.Tensor, step_tab: torch.Tensor, anc_tab: torch.Tensor, step: torch.Tensor,
                                seed: torch.Tensor, streams: Optional[torch.Tensor], scale: float, scale_im: Optional[float]):
    """Ancestral Euler tail of a captured sampling step, IN PLACE on x [bs, 4, H, W] fp32 (cd360_cfg_euler_ancestral_step_cl): eps_cl as
    for cfg_euler_step_cl, sigma = step_tab[step][0], (sigma_down, sigma_up, s_noise, 0) = anc_tab[step], the noise =
    sampler_noise(seed, streams, step, ...) drawn inside the kernel (none when sigma_up == 0)."""
    _need_gpu(x, eps_cl, step_tab, anc_tab, step, seed, streams)
    bs, hw, ld, sim = _cfg_cl_args(x, eps_cl, step_tab, step, scale_im)
    _tab_like(step_tab, anc_tab)
    _noise_args(seed, streams, step, bs)
    check(_lib.load().cd360_cfg_euler_ancestral_step_cl(_ptr(x), _ptr(eps_cl), _ptr(step_tab), _ptr(anc_tab), _ptr(step), _ptr(seed),
                                                       _ptr(streams), float(scale), sim, bs, hw, ld, _stream()),
          "cd360_cfg_euler_ancestral_step_cl")
    return x


def edm_churn(x: torch.Tensor, churn_tab: torch.Tensor, step: torch.Tensor, seed: torch.Tensor, streams: Optional[torch.Tensor]):
    """The churn of an EDM step, IN PLACE on x [bs, 4, H, W] fp32 (cd360_edm_churn_f32, include/cd360_edm.h): x <- x + (z * s_noise) *
    noise_std with (gamma, noise_std, s_noise, 0) = churn_tab[step] and z = sampler_noise(seed, streams, step, ...) drawn inside the kernel;
    x is neither read nor written on a noise_std == 0 row."""
    _need_gpu(x, churn_tab, step, seed, streams)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.ndim == 4 and x.shape[1] == 4
    assert churn_tab.dtype == torch.float32 and churn_tab.is_contiguous() and churn_tab.ndim == 2 and churn_tab.shape[1] == 4
    bs = x.shape[0]
    _noise_args(seed, streams, step, bs)
    check(_lib.load().cd360_edm_churn_f32(_ptr(x), _ptr(churn_tab), _ptr(step), _ptr(seed), _ptr(streams), bs, x.shape[2] * x.shape[3], _stream()),
          "cd360_edm_churn_f32")
    return x


def cfg_edm_predict(x: torch.Tensor, eps: torch.Tensor, row: torch.Tensor, scale: float, scale_im: Optional[float], want_dir: bool = True):
    """The predictor tail of an EDM step (cd360_cfg_edm_predict_f32, include/cd360_edm.h): x [n,...] fp32, eps [3n,...] fp32 (u | ic | c) or,
    with scale_im=None, [2n,...] (u | c), row = (sigma_hat, sigma_next, c_in, sq) a 4-element fp32 device tensor -> (xe, d), both new
    tensors: d = (x - d0) / sigma_hat with d0 combined at sq, xe = x + d (sigma_next - sigma_hat).  want_dir=False: d is not written (None)."""
    _need_gpu(x, eps, row)
    sim = _cfg_flat_args(x, eps, scale_im)
    _row4(row)
    xe = torch.empty_like(x)
    d = torch.empty_like(x) if want_dir else None
    check(_lib.load().cd360_cfg_edm_predict_f32(_ptr(x), _ptr(eps), _ptr(row), float(scale), sim, _ptr(xe), _ptr(d), x.numel(), _stream()),
          "cd360_cfg_edm_predict_f32")
    return xe, d


def cfg_edm_predict_cl(x: torch.Tensor, eps_cl: torch.Tensor, edm_tab: torch.Tensor, step: torch.Tensor, scale: float, scale_im: Optional[float],
                       xe: torch.Tensor, d: Optional[torch.Tensor] = None):
    """Predictor tail of a captured EDM step (cd360_cfg_edm_predict_cl): x [bs, 4, H, W] fp32 read, eps_cl as for cfg_euler_step_cl,
    (sigma_hat, sigma_next, -, sq) = edm_tab[step]; xe (may BE x: the in-place, churned Euler tail) and d (or None) are written."""
    _need_gpu(x, eps_cl, edm_tab, step, xe, d)
    bs, hw, ld, sim = _cfg_cl_args(x, eps_cl, edm_tab, step, scale_im)
    _like(x, xe, *(() if d is None else (d,)))
    check(_lib.load().cd360_cfg_edm_predict_cl(_ptr(x), _ptr(eps_cl), _ptr(edm_tab), _ptr(step), float(scale), sim, _ptr(xe), _ptr(d), bs, hw, ld,
                                              _stream()), "cd360_cfg_edm_predict_cl")
    return xe


def cfg_edm_correct(x: torch.Tensor, xe: torch.Tensor, d: torch.Tensor, eps2: torch.Tensor, row: torch.Tensor, corr_row: torch.Tensor, scale: float,
                    scale_im: Optional[float]):
    """The Heun corrector tail (cd360_cfg_edm_correct_f32, include/cd360_edm.h): x (the latent the predictor read), xe, d [n,...] fp32, eps2
    = the network at (xe, sigma_next) [3n,...] or [2n,...] fp32, row / corr_row = one row of edm_tab / corr_tab -> x' = x + (d + d_new) / 2
    (sigma_next - sigma_hat), a new tensor; xe where sigma_next is not > 0 (eps2 and d are then not read)."""
    _need_gpu(x, xe, d, eps2, row, corr_row)
    sim = _cfg_flat_args(x, eps2, scale_im)
    _row4(row, corr_row)
    _like(x, xe, d)
    out = torch.empty_like(x)
    check(_lib.load().cd360_cfg_edm_correct_f32(_ptr(x), _ptr(xe), _ptr(d), _ptr(eps2), _ptr(row), _ptr(corr_row), float(scale), sim, _ptr(out),
                                               x.numel(), _stream()), "cd360_cfg_edm_correct_f32")
    return out


def cfg_edm_correct_cl(x: torch.Tensor, xe: torch.Tensor, d: torch.Tensor, eps2_cl: torch.Tensor, edm_tab: torch.Tensor, corr_tab: torch.Tensor,
                       step: torch.Tensor, scale: float, scale_im: Optional[float]):
    """Corrector tail of a captured Heun step, IN PLACE on x [bs, 4, H, W] fp32 (cd360_cfg_edm_correct_cl): xe, d read, eps2_cl as for
    cfg_euler_step_cl, (sigma_hat, sigma_next) = edm_tab[step][0 / 1], sq' = corr_tab[step][3]; x <- xe where sigma_next is not > 0."""
    _need_gpu(x, xe, d, eps2_cl, edm_tab, corr_tab, step)
    bs, hw, ld, sim = _cfg_cl_args(x, eps2_cl, edm_tab, step, scale_im)
    _like(x, xe, d)
    _tab_like(edm_tab, corr_tab)
    check(_lib.load().cd360_cfg_edm_correct_cl(_ptr(x), _ptr(xe), _ptr(d), _ptr(eps2_cl), _ptr(edm_tab), _ptr(corr_tab), _ptr(step), float(scale), sim,
                                              bs, hw, ld, _stream()), "cd360_cfg_edm_correct_cl")
    return x


def cfg_dpmpp2s_mid(x: torch.Tensor, eps: torch.Tensor, sigma: torch.Tensor, mult: torch.Tensor, scale: float, scale_im: Optional[float]):
    """The midpoint tail of a DPM++ 2S step (cd360_cfg_dpmpp2s_mid_f32, include/cd360_highorder.h): x [n,...] fp32, eps [3n,...] fp32 (u | ic |
    c) or, with scale_im=None, [2n,...] (u | c), sigma a 1-element and mult = (m1, m2, m3, m4) a 4-element fp32 device tensor -> x2 = m1 x -
    m2 d0, a new tensor."""
    _need_gpu(x, eps, sigma, mult)
    sim = _cfg_flat_args(x, eps, scale_im)
    _scalar(sigma)
    _row4(mult)
    x2 = torch.empty_like(x)
    check(_lib.load().cd360_cfg_dpmpp2s_mid_f32(_ptr(x), _ptr(eps), _ptr(sigma), _ptr(mult), float(scale), sim, _ptr(x2), x.numel(), _stream()),
          "cd360_cfg_dpmpp2s_mid_f32")
    return x2


def cfg_dpmpp2s_mid_cl(x: torch.Tensor, eps_cl: torch.Tensor, step_tab: torch.Tensor, mult2s_tab: torch.Tensor, step: torch.Tensor, scale: float,
                       scale_im: Optional[float], x2: torch.Tensor):
    """Midpoint tail of a captured DPM++ 2S step (cd360_cfg_dpmpp2s_mid_cl): x [bs, 4, H, W] fp32 READ, eps_cl as for cfg_euler_step_cl, sigma =
    step_tab[step][0], (m1, m2) = mult2s_tab[step][0 / 1]; x2 (a buffer of its own) is written."""
    _need_gpu(x, eps_cl, step_tab, mult2s_tab, step, x2)
    bs, hw, ld, sim = _cfg_cl_args(x, eps_cl, step_tab, step, scale_im)
    _like(x, x2)
    _tab_like(step_tab, mult2s_tab)
    check(_lib.load().cd360_cfg_dpmpp2s_mid_cl(_ptr(x), _ptr(eps_cl), _ptr(step_tab), _ptr(mult2s_tab), _ptr(step), float(scale), sim, _ptr(x2), bs,
                                              hw, ld, _stream()), "cd360_cfg_dpmpp2s_mid_cl")
    return x2


def cfg_dpmpp2s_step(x: torch.Tensor, x2: torch.Tensor, eps2: torch.Tensor, mid_row: torch.Tensor, mult: torch.Tensor, anc: torch.Tensor,
                     seed: torch.Tensor, streams: Optional[torch.Tensor], step: torch.Tensor, scale: float, scale_im: Optional[float]):
    """The second tail of a DPM++ 2S step (cd360_cfg_dpmpp2s_step_f32): x, x2 [bs, 4, H, W] fp32, eps2 = the network at (x2, sigma_mid) [3 bs,
    ...] or [2 bs, ...] fp32, mid_row / mult / anc = one row of mid_tab / mult2s_tab / anc_tab -> x' = m3 x - m4 d0' (d0' combined from x2 at
    sq_mid), plus (z s_noise) sigma_up where sigma_up != 0, z = sampler_noise(seed, streams, step, ...) drawn inside the kernel; a new tensor."""
    _need_gpu(x, x2, eps2, mid_row, mult, anc, seed, streams, step)
    sim = _cfg_flat_args(x, eps2, scale_im)
    assert x.ndim == 4 and x.shape[1] == 4
    _like(x, x2)
    _row4(mid_row, mult, anc)
    bs = x.shape[0]
    _noise_args(seed, streams, step, bs)
    out = torch.empty_like(x)
    check(_lib.load().cd360_cfg_dpmpp2s_step_f32(_ptr(x), _ptr(x2), _ptr(eps2), _ptr(mid_row), _ptr(mult), _ptr(anc), _ptr(seed), _ptr(streams),
                                                _ptr(step), float(scale), sim, _ptr(out), bs, x.shape[2] * x.shape[3], _stream()),
          "cd360_cfg_dpmpp2s_step_f32")
    return out


def cfg_dpmpp2s_step_cl(x: torch.Tensor, x2: torch.Tensor, eps2_cl: torch.Tensor, mid_tab: torch.Tensor, mult2s_tab: torch.Tensor,
                        anc_tab: torch.Tensor, step: torch.Tensor, seed: torch.Tensor, streams: Optional[torch.Tensor], scale: float,
                        scale_im: Optional[float]):
    """Second tail of a captured DPM++ 2S step, IN PLACE on x [bs, 4, H, W] fp32 (cd360_cfg_dpmpp2s_step_cl): x2 read, eps2_cl as for
    cfg_euler_step_cl, sq_mid = mid_tab[step][3], (m3, m4) = mult2s_tab[step][2 / 3], (sigma_up, s_noise) = anc_tab[step][1 / 2]; the noise is
    drawn inside the kernel (none when sigma_up == 0)."""
    _need_gpu(x, x2, eps2_cl, mid_tab, mult2s_tab, anc_tab, step, seed, streams)
    bs, hw, ld, sim = _cfg_cl_args(x, eps2_cl, mid_tab, step, scale_im)
    _like(x, x2)
    _tab_like(mid_tab, mult2s_tab, anc_tab)
    _noise_args(seed, streams, step, bs)
    check(_lib.load().cd360_cfg_dpmpp2s_step_cl(_ptr(x), _ptr(x2), _ptr(eps2_cl), _ptr(mid_tab), _ptr(mult2s_tab), _ptr(anc_tab), _ptr(step),
                                               _ptr(seed), _ptr(streams), float(scale), sim, bs, hw, ld, _stream()), "cd360_cfg_dpmpp2s_step_cl")
    return x


def _lms_ring(x: torch.Tensor, ring: torch.Tensor) -> int:
    assert ring.dtype == torch.float32 and ring.is_contiguous() and ring.ndim == x.ndim + 1 and tuple(ring.shape[1:]) == tuple(x.shape)
    return ring.shape[0]


def cfg_lms_step(x: torch.Tensor, eps: torch.Tensor, ring: torch.Tensor, sigma: torch.Tensor, row: torch.Tensor, step: torch.Tensor, scale: float,
                 scale_im: Optional[float]):
    """One linear multistep tail (cd360_cfg_lms_step_f32, include/cd360_highorder.h): x [n,...] fp32, eps [3n,...] or [2n,...] fp32, ring
    [order, n,...] fp32 (order 1..4), sigma a 1-element and row = (c_0 .. c_3) a 4-element fp32 device tensor, step a device int32 = the
    index i of the step -> x' = x + sum_j c_j d_(i - j), a new tensor; d_i = (x - d0) / sigma is stored into ring[i % order], and only the
    min(i + 1, order) - 1 slots before it are read."""
    _need_gpu(x, eps, ring, sigma, row, step)
    sim = _cfg_flat_args(x, eps, scale_im)
    order = _lms_ring(x, ring)
    _scalar(sigma)
    assert step.dtype == torch.int32 and step.numel() == 1
    _row4(row)
    out = torch.empty_like(x)
    check(_lib.load().cd360_cfg_lms_step_f32(_ptr(x), _ptr(eps), _ptr(ring), _ptr(sigma), _ptr(row), _ptr(step), float(scale), sim, order, _ptr(out),
                                            x.numel(), _stream()), "cd360_cfg_lms_step_f32")
    return out


def cfg_lms_step_cl(x: torch.Tensor, ring: torch.Tensor, eps_cl: torch.Tensor, step_tab: torch.Tensor, lms_tab: torch.Tensor, step: torch.Tensor,
                    scale: float, scale_im: Optional[float]):
    """Linear multistep tail of a captured sampling step, IN PLACE on x [bs, 4, H, W] fp32 and on ring [order, bs, 4, H, W] fp32
    (cd360_cfg_lms_step_cl): eps_cl as for cfg_euler_step_cl, sigma = step_tab[step][0], (c_0 .. c_3) = lms_tab[step]."""
    _need_gpu(x, ring, eps_cl, step_tab, lms_tab, step)
    bs, hw, ld, sim = _cfg_cl_args(x, eps_cl, step_tab, step, scale_im)
    order = _lms_ring(x, ring)
    _tab_like(step_tab, lms_tab)
    check(_lib.load().cd360_cfg_lms_step_cl(_ptr(x), _ptr(ring), _ptr(eps_cl), _ptr(step_tab), _ptr(lms_tab), _ptr(step), float(scale), sim, order,
                                           bs, hw, ld, _stream()), "cd360_cfg_lms_step_cl")
    return x


def out_conv4_ok(H: int, W: int, cin: int) -> bool:
    return W in (32, 64, 128) and H % 2 == 0 and cin % 64 == 0 and H * W * cin * 2 < 2 ** 31


def pack_out_conv4_weight(w: torch.Tensor) -> torch.Tensor:
    """nn.Conv2d weight [4, Cin, 3, 3] -> [64, Cin] bf16, row tap * 4 + co (tap = 3 ky + kx), rows 36 .. 63 zero (cd360_out_conv4_bf16)."""
    co, cin, kh, kw = w.shape
    assert co == 4 and kh == 3 and kw == 3
    out = torch.zeros(64, cin, dtype=torch.bfloat16, device=w.device)
    out[:36] = w.detach().permute(2, 3, 0, 1).reshape(36, cin).to(torch.bfloat16)
    return out.contiguous()


def out_conv4(x: torch.Tensor, w36: torch.Tensor, bias: torch.Tensor, N: int, H: int, W: int) -> torch.Tensor:
    """The UNet's 3 x 3 output convolution to FOUR channels: x [N, H W, Cin] bf16 channels-last -> [N, H W, 4] bf16 (cd360_out_conv4_bf16)."""
    _need_gpu(x, w36, bias)
    cin = x.shape[-1]
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and x.numel() == N * H * W * cin and out_conv4_ok(H, W, cin)
    assert w36.shape == (64, cin) and w36.dtype == torch.bfloat16 and w36.is_contiguous() and bias.dtype == torch.float32 and bias.numel() == 4
    out = torch.empty(N, H * W, 4, dtype=torch.bfloat16, device=x.device)
    with _timed("conv_igemm", 2.0 * N * H * W * 9 * cin * 4, 2.0 * (N * H * W * (cin + 4) + 36 * cin)):
        check(_lib.load().cd360_out_conv4_bf16(_ptr(x), _ptr(w36), _ptr(bias), _ptr(out), N, H, W, cin, _stream()), "cd360_out_conv4_bf16")
    return out


# ----------------------------------------------------------------------------------------------- the first stage's two ends (Decoder)
def pack_vae_conv_in_weight(w: torch.Tensor) -> torch.Tensor:
    """Decoder.conv_in weight [Cout, Cz, 3, 3] -> fp32 [Cz * 9, Cout], row ci * 9 + 3 ky + kx (cd360_vae_conv_in_f32)."""
    cout, cz, kh, kw = w.shape
    assert kh == 3 and kw == 3
    return w.detach().float().permute(1, 2, 3, 0).reshape(cz * 9, cout).contiguous()


def pack_vae_conv_out_weight(w: torch.Tensor) -> torch.Tensor:
    """Decoder.conv_out weight [Cout <= 4, Cin, 3, 3] -> fp32 [9, Cin, 4] (tap 3 ky + kx, channel, output channel; columns >= Cout zero)
    (cd360_vae_conv_out_bf16)."""
    cout, cin, kh, kw = w.shape
    assert kh == 3 and kw == 3 and cout <= 4
    out = torch.zeros(9, cin, 4, dtype=torch.float32, device=w.device)
    out[:, :, :cout] = w.detach().float().permute(2, 3, 1, 0).reshape(9, cin, cout)
    return out


def pack_attn_qkv(qw: torch.Tensor, qb: torch.Tensor, kw: torch.Tensor, kb: torch.Tensor, vw: torch.Tensor, vb: torch.Tensor):
    """The q, k, v 1 x 1 convolutions of a first-stage attention block ([C, C, 1, 1] weights, [C] biases) -> (w bf16 [3 C, C], bias fp32
    [3 C]) of ONE merged projection whose q rows and q bias carry C^-0.5 log2 e (multiplied in fp32, one bf16 rounding of the weight):
    the prescaled q of attention_single(..., qscale=1)."""
    c = qw.shape[0]
    s = c ** -0.5 * 1.4426950408889634
    w = torch.cat([qw.detach().float().reshape(c, c) * s, kw.detach().float().reshape(c, c), vw.detach().float().reshape(c, c)], 0)
    b = torch.cat([qb.detach().float() * s, kb.detach().float(), vb.detach().float()], 0)
    return w.to(torch.bfloat16).contiguous(), b.contiguous()


def vae_conv_in(z: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], want_stats: bool = False):
    """Decoder.conv_in: z fp32 NCHW [B, Cz, H, W] -> bf16 channels-last [B, H W, Cout] (cd360_vae_conv_in_f32).  want_stats=True
    (H W % 64 == 0): returns (out, tile_stats [B, slabs, Cout, 2] fp32) for gn_silu(out, ..., tile_stats=tile_stats)."""
    _need_gpu(z, w_packed, bias)
    B, cz, H, W = z.shape
    cout = w_packed.shape[1]
    assert z.dtype == torch.float32 and z.is_contiguous() and w_packed.dtype == torch.float32 and w_packed.shape == (cz * 9, cout)
    assert w_packed.is_contiguous() and (bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == cout))
    lib = _lib.load()
    out = torch.empty(B, H * W, cout, dtype=torch.bfloat16, device=z.device)
    stats = torch.empty(B, lib.cd360_vae_conv_in_stats_slabs(H, W), cout, 2, dtype=torch.float32, device=z.device) if want_stats else None
    with _timed("vae_conv_in", 2.0 * B * H * W * 9 * cz * cout, 4.0 * B * H * W * cz + 2.0 * B * H * W * cout):
        check(lib.cd360_vae_conv_in_f32(_ptr(z), _ptr(w_packed), _ptr(bias), _ptr(out), _ptr(stats), B, cz, H, W, cout, _stream()),
              "cd360_vae_conv_in_f32")
    return (out, stats) if want_stats else out


def vae_conv_out(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], N: int, H: int, W: int, cout: int) -> torch.Tensor:
    """Decoder.conv_out: x bf16 channels-last [N, H W, Cin] (after norm_out + SiLU) -> fp32 NCHW [N, cout, H, W] (cd360_vae_conv_out_bf16)."""
    _need_gpu(x, w_packed, bias)
    cin = x.shape[-1]
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and x.numel() == N * H * W * cin and 1 <= cout <= 4
    assert w_packed.dtype == torch.float32 and w_packed.is_contiguous() and w_packed.shape == (9, cin, 4)
    assert bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == cout)
    out = torch.empty(N, cout, H, W, dtype=torch.float32, device=x.device)
    with _timed("vae_conv_out", 2.0 * N * H * W * 9 * cin * cout, 2.0 * N * H * W * cin + 4.0 * N * H * W * cout):
        check(_lib.load().cd360_vae_conv_out_bf16(_ptr(x), _ptr(w_packed), _ptr(bias), _ptr(out), N, H, W, cin, cout, _stream()),
              "cd360_vae_conv_out_bf16")
    return out


# ----------------------------------------------------------------------------------------------- the first stage's encoder
def vae_downsample_stats_rows(N: int, H: int, W: int, C: int) -> int:
    """Pixels per tile_stats slab of vae_downsample for this shape on the current stream (0: the output has no slabs)."""
    _lib.query_stream(_stream())
    return _lib.load().cd360_vae_downsample_stats_rows(N, H, W, C)


def vae_downsample(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], N: int, H: int, W: int, want_stats: bool = True):
    """Encoder Downsample (with_conv=True): x bf16 channels-last [N, H W, C], w_packed = pack_conv_weight(conv.weight) -> (out bf16
    [N, (H // 2) (W // 2), C], tile_stats) = conv3x3 / stride 2 of F.pad(x, (0, 1, 0, 1)) (cd360_vae_downsample_bf16).  tile_stats: fp32
    [N, slabs, C, 2] for gn_silu(out, ..., tile_stats=tile_stats) when want_stats and the shape has slabs
    (cd360_vae_downsample_stats_rows), else None."""
    _need_gpu(x, w_packed, bias)
    c = x.shape[-1]
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and x.numel() == N * H * W * c
    assert w_packed.dtype == torch.bfloat16 and w_packed.is_contiguous() and w_packed.shape == (c, 9 * c)
    assert bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == c)
    ho, wo = H // 2, W // 2
    lib = _lib.load()
    out = torch.empty(N, ho * wo, c, dtype=torch.bfloat16, device=x.device)
    rows = vae_downsample_stats_rows(N, H, W, c) if want_stats else 0
    stats = torch.empty(N, (ho * wo) // rows, c, 2, dtype=torch.float32, device=x.device) if rows > 0 else None
    m = N * ho * wo
    with _timed("vae_downsample", 2.0 * m * 9 * c * c, 2.0 * (N * H * W * c + m * c + 9 * c * c)):
        check(lib.cd360_vae_downsample_bf16(_ptr(x), _ptr(w_packed), _ptr(bias), _ptr(out), _ptr(stats), N, H, W, c, _stream()),
              "cd360_vae_downsample_bf16")
    return out, stats


def pack_vae_enc_conv_out_weight(w: torch.Tensor) -> torch.Tensor:
    """Encoder.conv_out weight [Cout <= 8, Cin, 3, 3] -> fp32 [9, Cin, 8] (tap 3 ky + kx, channel, output channel; columns >= Cout zero)
    (cd360_vae_enc_conv_out_bf16)."""
    cout, cin, kh, kw = w.shape
    assert kh == 3 and kw == 3 and cout <= 8
    out = torch.zeros(9, cin, 8, dtype=torch.float32, device=w.device)
    out[:, :, :cout] = w.detach().float().permute(2, 3, 1, 0).reshape(9, cin, cout)
    return out


def vae_enc_conv_out(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], N: int, H: int, W: int, cout: int) -> torch.Tensor:
    """Encoder.conv_out: x bf16 channels-last [N, H W, Cin] (after norm_out + SiLU) -> fp32 NCHW [N, cout, H, W]
    (cd360_vae_enc_conv_out_bf16)."""
    _need_gpu(x, w_packed, bias)
    cin = x.shape[-1]
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and x.numel() == N * H * W * cin and 1 <= cout <= 8
    assert w_packed.dtype == torch.float32 and w_packed.is_contiguous() and w_packed.shape == (9, cin, 8)
    assert bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == cout)
    out = torch.empty(N, cout, H, W, dtype=torch.float32, device=x.device)
    with _timed("vae_enc_conv_out", 2.0 * N * H * W * 9 * cin * cout, 2.0 * N * H * W * cin + 4.0 * N * H * W * cout):
        check(_lib.load().cd360_vae_enc_conv_out_bf16(_ptr(x), _ptr(w_packed), _ptr(bias), _ptr(out), N, H, W, cin, cout, _stream()),
              "cd360_vae_enc_conv_out_bf16")
    return out


# ----------------------------------------------------------------------------------------------- sampler <-> first stage (include/cd360_image.h)
# These four refuse a bad argument with ValueError BEFORE the device check and before the library is loaded, so a refusal is the same on a
# machine without a GPU (tests/test_images_cpu.py); a CPU tensor that passes them raises Cd360Error in _need_gpu, as everywhere above.
def _refuse(bad: bool, what: str) -> None:
    if bad:
        raise ValueError(what)


def _f32_tensor(t: torch.Tensor, shape, name: str) -> None:
    _refuse(not isinstance(t, torch.Tensor) or t.dtype != torch.float32, f"{name}: an fp32 tensor is needed, got {getattr(t, 'dtype', type(t))}")
    _refuse(tuple(t.shape) != tuple(shape) or not t.is_contiguous(), f"{name}: a contiguous tensor of shape {tuple(shape)} is needed, got {tuple(t.shape)}")


def _seed_args(seed: torch.Tensor, streams: Optional[torch.Tensor], rows: int) -> None:
    _refuse(seed.dtype != torch.int64 or seed.numel() != 1, f"seed: a 1-element int64 tensor is needed, got {seed.dtype} x {seed.numel()}")
    _refuse(streams is not None and (streams.dtype != torch.int32 or streams.numel() != rows or not streams.is_contiguous()),
            f"streams: None or a contiguous int32 tensor of {rows} ids is needed")


def _overlaps(a: torch.Tensor, b: torch.Tensor) -> bool:
    pa, pb = a.data_ptr(), b.data_ptr()
    return pa < pb + b.numel() * b.element_size() and pb < pa + a.numel() * a.element_size()


def _out_arg(out: Optional[torch.Tensor], shape, dtype, like: torch.Tensor, name: str) -> torch.Tensor:
    """The result buffer: the caller's `out` (checked: dtype, shape, contiguous, not overlapping `like`) or a fresh one beside `like`."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=like.device)
    _refuse(out.dtype != dtype or tuple(out.shape) != tuple(shape) or not out.is_contiguous(),
            f"out: a contiguous {dtype} tensor of shape {tuple(shape)} is needed, got {out.dtype} {tuple(out.shape)}")
    _refuse(out.device != like.device, f"out is on {out.device}, {name} on {like.device}")
    _refuse(_overlaps(out, like), f"out overlaps {name}")
    return out


def start_noise(seed: torch.Tensor, streams: Optional[torch.Tensor], scale: torch.Tensor, bs: int, H: int, W: int) -> torch.Tensor:
    """The start latent of a trajectory, [bs, 4, H, W] fp32 = z * scale (cd360_start_noise_f32, include/cd360_image.h): z = the noise of
    sampler_noise in counter domain 1 (step word 0), a pure function of (seed, streams[row], channel, pixel).  seed: device int64[1];
    streams: device int32[bs] or None (stream 0 for every row); scale: a 1-element fp32 device tensor, sqrt(1 + sigma_0^2)."""
    _refuse(bs <= 0 or H <= 0 or W <= 0, f"bs, H, W must be positive, got {bs}, {H}, {W}")
    _seed_args(seed, streams, bs)
    _refuse(scale.dtype != torch.float32 or scale.numel() != 1, f"scale: a 1-element fp32 tensor is needed, got {scale.dtype} x {scale.numel()}")
    _need_gpu(seed, streams, scale)
    out = torch.empty((bs, 4, H, W), dtype=torch.float32, device=seed.device)
    check(_lib.load().cd360_start_noise_f32(_ptr(out), _ptr(seed), _ptr(streams), _ptr(scale), bs, H * W, _stream()), "cd360_start_noise_f32")
    return out


def posterior_sample(moments: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, seed: Optional[torch.Tensor], streams: Optional[torch.Tensor],
                     draw: Optional[torch.Tensor], scale_factor: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """quant_conv + DiagonalGaussianDistribution.sample() + scale_factor * z in one kernel (cd360_posterior_sample_f32): moments [B, 8, H, W]
    fp32 (Encoder.forward's output), w [8, 8] / bias [8] fp32 = quant_conv's weight (output, input) and bias -> [B, 4, H, W] fp32 =
    (mean + exp(0.5 clamp(logvar, -30, 20)) z) * scale_factor, z in counter domain 2 at (pixel, draw, streams[b]).  seed: device int64[1],
    draw: device int32[1], streams: device int32[B] or None.  seed=None is mode(): mean * scale_factor, streams / draw ignored."""
    _refuse(moments.ndim != 4 or moments.shape[1] != 8, f"moments: [B, 8, H, W] is needed (z_channels = 4, double_z), got {tuple(moments.shape)}")
    B, _, H, W = moments.shape
    _refuse(B <= 0 or H * W <= 0, f"moments is empty: {tuple(moments.shape)}")
    _f32_tensor(moments, moments.shape, "moments")
    _f32_tensor(w, (8, 8), "w")
    _f32_tensor(bias, (8,), "bias")
    if seed is not None:
        _seed_args(seed, streams, B)
        _refuse(draw is None or draw.dtype != torch.int32 or draw.numel() != 1, "draw: a 1-element int32 tensor is needed with a seed")
    else:
        streams = draw = None
    out = _out_arg(out, (B, 4, H, W), torch.float32, moments, "moments")
    _need_gpu(moments, w, bias, seed, streams, draw, out)
    with _timed("posterior_sample", 2.0 * B * H * W * 72, 4.0 * B * H * W * 12):
        check(_lib.load().cd360_posterior_sample_f32(_ptr(moments), _ptr(w), _ptr(bias), _ptr(seed), _ptr(streams), _ptr(draw), float(scale_factor),
                                                    _ptr(out), B, H * W, _stream()), "cd360_posterior_sample_f32")
    return out


def post_quant(z: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, inv_scale: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """1 / scale_factor * z + post_quant_conv in one kernel (cd360_post_quant_f32): z [B, 4, H, W] fp32, w [4, 4] / bias [4] fp32 = the 1 x 1
    convolution's weight (output, input) and bias -> [B, 4, H, W] fp32, the Decoder's input."""
    _refuse(z.ndim != 4 or z.shape[1] != 4, f"z: [B, 4, H, W] is needed, got {tuple(z.shape)}")
    B, _, H, W = z.shape
    _refuse(B <= 0 or H * W <= 0, f"z is empty: {tuple(z.shape)}")
    _f32_tensor(z, z.shape, "z")
    _f32_tensor(w, (4, 4), "w")
    _f32_tensor(bias, (4,), "bias")
    out = _out_arg(out, z.shape, torch.float32, z, "z")
    _need_gpu(z, w, bias, out)
    with _timed("post_quant", 2.0 * B * H * W * 20, 4.0 * B * H * W * 8):
        check(_lib.load().cd360_post_quant_f32(_ptr(z), _ptr(w), _ptr(bias), float(inv_scale), _ptr(out), B, H * W, _stream()), "cd360_post_quant_f32")
    return out


def vae_conv_out_u8(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], N: int, H: int, W: int, cout: int,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Decoder.conv_out with the image epilogue (cd360_vae_conv_out_u8): x, w_packed, bias as for vae_conv_out -> uint8 [N, H, W, cout]
    (channels last) = (clip(v * 0.5 + 0.5, 0, 1) * 255).to(uint8) of the fp32 value v vae_conv_out writes, bit for bit; a NaN writes 0."""
    _refuse(not 1 <= cout <= 4, f"cout = {cout}: the output convolution serves 1..4 channels")
    _refuse(N <= 0 or H <= 0 or W <= 0, f"N, H, W must be positive, got {N}, {H}, {W}")
    _refuse(x.dtype != torch.bfloat16 or not x.is_contiguous(), f"x: a contiguous bf16 tensor is needed, got {x.dtype}")
    cin = x.shape[-1]
    _refuse(x.numel() != N * H * W * cin or cin % 64 != 0, f"x: [{N}, {H * W}, Cin % 64 == 0] is needed, got {tuple(x.shape)}")
    _f32_tensor(w_packed, (9, cin, 4), "w_packed")
    _refuse(bias is not None and (bias.dtype != torch.float32 or bias.numel() != cout or not bias.is_contiguous()),
            f"bias: None or {cout} contiguous fp32 values are needed")
    out = _out_arg(out, (N, H, W, cout), torch.uint8, x, "x")
    _need_gpu(x, w_packed, bias, out)
    with _timed("vae_conv_out_u8", 2.0 * N * H * W * 9 * cin * cout, 2.0 * N * H * W * cin + 1.0 * N * H * W * cout):
        check(_lib.load().cd360_vae_conv_out_u8(_ptr(x), _ptr(w_packed), _ptr(bias), _ptr(out), N, H, W, cin, cout, _stream()),
              "cd360_vae_conv_out_u8")
    return out


# ----------------------------------------------------------------------------------------------- masked sampling (include/edit/cd360_edit.h)
# libcd360_edit.so through cd360/_edit.py.  Refusals as above: ValueError before the device check and before the library is loaded.
def _step_arg(step: torch.Tensor) -> None:
    _refuse(not isinstance(step, torch.Tensor) or step.dtype != torch.int32 or step.numel() != 1,
            f"step: a 1-element int32 tensor is needed, got {getattr(step, 'dtype', type(step))}")


def edit_noise(seed: torch.Tensor, streams: Optional[torch.Tensor], step: torch.Tensor, bs: int, H: int, W: int) -> torch.Tensor:
    """Standard normals [bs, 4, H, W] fp32 of counter domain 3 (cd360_edit_noise_f32, include/edit/cd360_edit.h): the noise mask_blend adds
    to the known latent, a pure function of (seed, streams[row], step, channel, pixel) unrelated to sampler_noise / start_noise under the
    same seed.  seed: device int64[1], step: device int32[1], streams: device int32[bs] or None (stream 0 for every row)."""
    from . import _edit
    _refuse(bs <= 0 or H <= 0 or W <= 0, f"bs, H, W must be positive, got {bs}, {H}, {W}")
    _seed_args(seed, streams, bs)
    _step_arg(step)
    _need_gpu(seed, streams, step)
    out = torch.empty((bs, 4, H, W), dtype=torch.float32, device=seed.device)
    check(_edit.load().cd360_edit_noise_f32(_ptr(out), _ptr(seed), _ptr(streams), _ptr(step), bs, H * W, _stream()), "cd360_edit_noise_f32")
    return out


def mask_blend(x: torch.Tensor, known: torch.Tensor, mask: torch.Tensor, sigma_next: torch.Tensor, step: torch.Tensor, seed: torch.Tensor,
               streams: Optional[torch.Tensor]) -> torch.Tensor:
    """The end of a masked sampling step, IN PLACE on x [bs, 4, H, W] fp32 (cd360_mask_blend_f32): x <- m x + (1 - m) kn with
    kn = known + z s' (known itself where s' == 0), z = edit_noise(seed, streams, step, ...) drawn inside the kernel.  known [bs, 4, H, W]
    fp32; mask [bs or 1, 1, H, W] fp32, 1 = generate, 0 = keep.  sigma_next: a step table [nsteps, 4] fp32 (s' = its column 1 in row
    `step`: the staged step) or a 1-element fp32 tensor (s' itself: the un-staged step).  step: device int32[1]."""
    from . import _edit
    _refuse(not isinstance(x, torch.Tensor) or x.ndim != 4 or x.shape[1] != 4, f"x: [bs, 4, H, W] is needed, got {tuple(getattr(x, 'shape', ()))}")
    bs, _, H, W = x.shape
    _refuse(bs <= 0 or H * W <= 0, f"x is empty: {tuple(x.shape)}")
    _f32_tensor(x, x.shape, "x")
    _f32_tensor(known, x.shape, "known")
    _refuse(not isinstance(mask, torch.Tensor) or mask.ndim != 4 or mask.shape[0] not in (1, bs),
            f"mask: [{bs} or 1, 1, {H}, {W}] is needed, got {tuple(getattr(mask, 'shape', ()))}")
    _f32_tensor(mask, (mask.shape[0], 1, H, W), "mask")
    _refuse(not isinstance(sigma_next, torch.Tensor) or sigma_next.dtype != torch.float32 or not sigma_next.is_contiguous()
            or not (sigma_next.numel() == 1 or (sigma_next.ndim == 2 and sigma_next.shape[1] == 4)),
            "sigma_next: a contiguous fp32 step table [nsteps, 4] or a 1-element fp32 tensor is needed")
    _seed_args(seed, streams, bs)
    _step_arg(step)
    _refuse(len({t.device for t in (x, known, mask, sigma_next, step, seed)} | ({streams.device} if streams is not None else set())) != 1,
            "x, known, mask, sigma_next, step, seed and streams must be on one device")
    _refuse(_overlaps(x, known) or _overlaps(x, mask), "x overlaps known or mask")
    _need_gpu(x, known, mask, sigma_next, step, seed, streams)
    table = sigma_next.numel() != 1
    ptr = sigma_next.data_ptr() + (4 if table else 0)  # column 1 of the table's rows
    check(_edit.load().cd360_mask_blend_f32(_ptr(x), _ptr(known), _ptr(mask), mask.shape[0], ptr, 4 if table else 0, _ptr(step), _ptr(seed),
                                           _ptr(streams), bs, H * W, _stream()), "cd360_mask_blend_f32")
    return x


# ----------------------------------------------------------------------------------------------- the ends of a training step (include/train/cd360_train.h)
# libcd360_train.so through cd360/_train.py.  Refusals as above: ValueError before the device check and before the library is loaded.
TRAIN_ROW = 12  # CD360_TRAIN_ROW
TRAIN_CUBIC, TRAIN_DISCRETE = 0, 1


def _sigma_table(t: torch.Tensor, name: str) -> None:
    _refuse(not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.ndim != 1 or t.numel() == 0 or not t.is_contiguous(),
            f"{name}: a contiguous fp32 vector of sigmas is needed")


def _sampler_args(kind: int, start: int, table: torch.Tensor, name: str) -> None:
    _refuse(kind not in (TRAIN_CUBIC, TRAIN_DISCRETE), f"{name}: kind {kind} is neither cubic (0) nor discrete (1)")
    _refuse(kind == TRAIN_DISCRETE and not 0 <= start < table.numel(), f"{name}: num_idx_start {start} outside [0, {table.numel()})")


def train_sigmas(table: torch.Tensor, tgt_table: torch.Tensor, tgt_kind: int, tgt_start: int, ref_table: torch.Tensor, ref_kind: int, ref_start: int,
                 seed: torch.Tensor, streams: Optional[torch.Tensor], step: torch.Tensor, B: int, advance: bool = False, out=None):
    """The per-sample draws and scalars of a training step (cd360_train_sigmas_f32) -> (rows [B, TRAIN_ROW] fp32, timesteps int64 [B],
    sigmas_ref_idx int64 [B], step_used int32 [1]).  table: the denoiser's sigmas; tgt_table / ref_table: the samplers' tables with their
    kind (TRAIN_CUBIC / TRAIN_DISCRETE) and num_idx_start; seed device int64[1]; streams device int32[B] or None; step device int32[1],
    incremented on the device when `advance`.  A row holds sigma, w, c_skip, c_out, c_in, sigma_ref, c_in_ref, off_tgt, off_ref (cd360._train).
    out: the four result buffers to write instead of fresh ones."""
    from . import _train
    _refuse(B <= 0, f"B must be positive, got {B}")
    for t, name in ((table, "table"), (tgt_table, "tgt_table"), (ref_table, "ref_table")):
        _sigma_table(t, name)
    _sampler_args(tgt_kind, tgt_start, tgt_table, "sigma_sampler")
    _sampler_args(ref_kind, ref_start, ref_table, "sigma_sampler_ref")
    _seed_args(seed, streams, B)
    _step_arg(step)
    _need_gpu(table, tgt_table, ref_table, seed, streams, step)
    dev = seed.device
    if out is None:
        out = (torch.empty((B, TRAIN_ROW), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.int64, device=dev),
               torch.empty((B,), dtype=torch.int64, device=dev), torch.empty((1,), dtype=torch.int32, device=dev))
    rows, timesteps, ref_idx, step_used = out
    _f32_tensor(rows, (B, TRAIN_ROW), "rows")
    _refuse(any(t.dtype != torch.int64 or tuple(t.shape) != (B,) or not t.is_contiguous() for t in (timesteps, ref_idx)),
            f"timesteps, sigmas_ref_idx: contiguous int64 [{B}] are needed")
    _step_arg(step_used)
    _need_gpu(rows, timesteps, ref_idx, step_used)
    check(_train.load().cd360_train_sigmas_f32(_ptr(table), table.numel(), _ptr(tgt_table), tgt_table.numel(), tgt_kind, tgt_start, _ptr(ref_table),
                                               ref_table.numel(), ref_kind, ref_start, _ptr(seed), _ptr(streams), _ptr(step), int(bool(advance)),
                                               _ptr(rows), _ptr(timesteps), _ptr(ref_idx), _ptr(step_used), B, _stream()), "cd360_train_sigmas_f32")
    return rows, timesteps, ref_idx, step_used


def train_noise(x0: torch.Tensor, x_ref: Optional[torch.Tensor], drop_im: Optional[torch.Tensor], rows: torch.Tensor, seed: torch.Tensor,
                streams: Optional[torch.Tensor], step_used: torch.Tensor, level: float, dtype=torch.float32, out=None):
    """Noise the target latent and the reference views and scale them for the network (cd360_train_noise_f32) -> (x_t fp32, x_in, xr_in |
    None), x_in and xr_in in `dtype` (fp32 or bf16).  x0 [B, 4, H, W] fp32; x_ref [B, n, 4, H, W] fp32 or None; drop_im [B] fp32 or None;
    rows, step_used as train_sigmas returned them; level = offset_noise_level.  out: (x_t, x_in, xr_in) to write instead of fresh ones."""
    from . import _train
    _refuse(not isinstance(x0, torch.Tensor) or x0.ndim != 4 or x0.shape[1] != 4, f"x0: [B, 4, H, W] is needed, got {tuple(getattr(x0, 'shape', ()))}")
    B, _, H, W = x0.shape
    _refuse(B <= 0 or H * W <= 0, f"x0 is empty: {tuple(x0.shape)}")
    _f32_tensor(x0, x0.shape, "x0")
    n = 0
    if x_ref is not None:
        _refuse(x_ref.ndim != 5 or x_ref.shape[0] != B or x_ref.shape[1] <= 0 or tuple(x_ref.shape[2:]) != (4, H, W),
                f"x_ref: [{B}, n, 4, {H}, {W}] is needed, got {tuple(x_ref.shape)}")
        n = x_ref.shape[1]
        _refuse(n * H * W > 1 << 32, f"x_ref: n * H * W = {n * H * W} > 2^32 (the pixel is one 32-bit counter word)")
        _f32_tensor(x_ref, x_ref.shape, "x_ref")
    _refuse(H * W > 1 << 32, f"x0: H * W = {H * W} > 2^32")
    if drop_im is not None:
        _f32_tensor(drop_im, (B,), "drop_im")
    _f32_tensor(rows, (B, TRAIN_ROW), "rows")
    _seed_args(seed, streams, B)
    _step_arg(step_used)
    _refuse(dtype not in (torch.float32, torch.bfloat16), f"dtype: fp32 or bf16, got {dtype}")
    _refuse(not (0.0 <= float(level) < float("inf")), f"level = {level}: a finite value >= 0 is needed")
    _need_gpu(x0, x_ref, drop_im, rows, seed, streams, step_used)
    if out is None:
        out = (torch.empty(x0.shape, dtype=torch.float32, device=x0.device), torch.empty(x0.shape, dtype=dtype, device=x0.device),
               None if x_ref is None else torch.empty(x_ref.shape, dtype=dtype, device=x0.device))
    x_t, x_in, xr_in = out
    _f32_tensor(x_t, x0.shape, "x_t")
    _refuse(x_in.dtype != dtype or tuple(x_in.shape) != tuple(x0.shape) or not x_in.is_contiguous(), f"x_in: contiguous {dtype} {tuple(x0.shape)} is needed")
    if x_ref is not None:
        _refuse(xr_in is None or xr_in.dtype != dtype or tuple(xr_in.shape) != tuple(x_ref.shape) or not xr_in.is_contiguous(),
                f"xr_in: contiguous {dtype} {tuple(x_ref.shape)} is needed")
    _need_gpu(x_t, x_in, xr_in)
    check(_train.load().cd360_train_noise_f32(_ptr(x0), _ptr(x_ref), _ptr(drop_im), _ptr(rows), _ptr(seed), _ptr(streams), _ptr(step_used), float(level),
                                              _ptr(x_t), _ptr(x_in), _ptr(xr_in) if x_ref is not None else None, int(dtype == torch.bfloat16), B, n,
                                              H * W, _stream()), "cd360_train_noise_f32")
    return x_t, x_in, (xr_in if x_ref is not None else None)


def _train_l2_args(eps, x_t, x0, rows, mask):
    _refuse(not isinstance(eps, torch.Tensor) or eps.ndim != 4 or eps.shape[1] != 4, f"eps: [B, 4, H, W] is needed, got {tuple(getattr(eps, 'shape', ()))}")
    _refuse(eps.dtype not in (torch.float32, torch.bfloat16), f"eps: fp32 or bf16, got {eps.dtype}")
    B, _, H, W = eps.shape
    _refuse(B <= 0 or H * W <= 0, f"eps is empty: {tuple(eps.shape)}")
    _refuse(any(s < 0 for s in eps.stride()), "eps: negative strides")
    _f32_tensor(x_t, eps.shape, "x_t")
    _f32_tensor(x0, eps.shape, "x0")
    _f32_tensor(rows, (B, TRAIN_ROW), "rows")
    if mask is not None:
        _f32_tensor(mask, (B, 1, H, W), "mask")
    return B, H, W


def _strides4(t: torch.Tensor):
    return (ctypes.c_int64 * 4)(*t.stride())


def train_l2(eps: torch.Tensor, x_t: torch.Tensor, x0: torch.Tensor, rows: torch.Tensor, mask: Optional[torch.Tensor]) -> torch.Tensor:
    """The l2 term of the loss from the network's output -> [B] fp32 (cd360_train_l2_f32): D = eps c_out + x_t c_skip, w (D - x0)^2 summed
    over the mask and divided by sum(mask) + 1e-6, or the mean without a mask (loss.py:183-187 of the reference).  eps [B, 4, H, W] fp32 or
    bf16 in ANY layout (read by its strides, no copy); x_t, x0 fp32 contiguous; rows as train_sigmas returned them; mask [B, 1, H, W] fp32
    or None.  Differentiable with respect to eps (grad.TrainL2Fn); the same bits on every run."""
    if _wants_grad(eps):
        from . import grad
        return grad.TrainL2Fn.apply(eps, x_t, x0, rows, mask)
    return _train_l2_fwd(eps, x_t, x0, rows, mask)[0]


def _train_l2_fwd(eps, x_t, x0, rows, mask):
    """-> (loss [B], den [B]): den is what the backward divides by."""
    from . import _train
    B, H, W = _train_l2_args(eps, x_t, x0, rows, mask)
    eps = eps.detach()
    _need_gpu(eps, x_t, x0, rows, mask)
    loss = torch.empty((B,), dtype=torch.float32, device=eps.device)
    den = torch.empty((B,), dtype=torch.float32, device=eps.device)
    check(_train.load().cd360_train_l2_f32(_ptr(eps), int(eps.dtype == torch.bfloat16), _strides4(eps), _ptr(x_t), _ptr(x0), _ptr(rows), _ptr(mask),
                                           _ptr(loss), _ptr(den), B, H, W, _stream()), "cd360_train_l2_f32")
    return loss, den


def train_l2_bwd(eps, x_t, x0, rows, mask, den, g) -> torch.Tensor:
    """-> d_eps in eps's dtype and layout: g[b] 2 w err c_out [mask] / den[b], an exact 0 where g[b] == 0 (cd360_train_l2_bwd_f32)."""
    from . import _train
    B, H, W = _train_l2_args(eps, x_t, x0, rows, mask)
    eps = eps.detach()
    _f32_tensor(den, (B,), "den")
    g = g.detach().float().contiguous()
    _refuse(tuple(g.shape) != (B,), f"g: [{B}] is needed, got {tuple(g.shape)}")
    _need_gpu(eps, x_t, x0, rows, mask, den, g)
    d_eps = torch.empty_like(eps)
    check(_train.load().cd360_train_l2_bwd_f32(_ptr(eps), int(eps.dtype == torch.bfloat16), _strides4(eps), _ptr(x_t), _ptr(x0), _ptr(rows), _ptr(mask),
                                               _ptr(den), _ptr(g), _ptr(d_eps), _strides4(d_eps), B, H, W, _stream()), "cd360_train_l2_bwd_f32")
    return d_eps


# ----------------------------------------------------------------------------------------------- pictures in (include/picture/cd360_picture.h)
# libcd360_picture.so through cd360/_picture.py.  Refusals as above: ValueError before the device check and before the library is loaded.
PICTURE_MAX_TAPS = 64  # CD360_PICTURE_MAX_TAPS
PICTURE_MAX_DILATE = 31  # CD360_PICTURE_MAX_DILATE


def _window_arg(window):
    _refuse(len(window) != 4, f"window: (left, top, w, h) is needed, got {tuple(window)}")
    left, top, w, h = (int(v) for v in window)
    _refuse(w <= 0 or h <= 0, f"window: an empty crop, w = {w}, h = {h}")
    _refuse(max(abs(left), abs(top), w, h) > 1 << 30, f"window {(left, top, w, h)}: a coordinate beyond 2^30")
    return left, top, w, h


def _u8_picture(src: torch.Tensor, name: str, channels) -> int:
    _refuse(not isinstance(src, torch.Tensor) or src.dtype != torch.uint8 or src.ndim not in (2, 3),
            f"{name}: a uint8 [H, W] or [H, W, C] tensor is needed, got {getattr(src, 'dtype', type(src))} {tuple(getattr(src, 'shape', ()))}")
    C = 1 if src.ndim == 2 else src.shape[2]
    _refuse(C not in channels, f"{name}: {C} channels, served: {tuple(channels)}")
    H, W = src.shape[:2]
    _refuse(H <= 0 or W <= 0, f"{name} is empty: {tuple(src.shape)}")
    _refuse(src.stride(1) != C or (src.ndim == 3 and C > 1 and src.stride(2) != 1) or src.stride(0) < W * C,
            f"{name}: pixels of {C} neighbouring bytes in rows at least {W * C} bytes apart are needed, got strides {tuple(src.stride())}")
    _refuse(H * src.stride(0) >= 1 << 31, f"{name}: {H} rows of {src.stride(0)} bytes do not fit 32-bit offsets")
    return C


def _tap_table(tab, n_out: int, name: str) -> int:
    _refuse(not isinstance(tab, (tuple, list)) or len(tab) != 3, f"{name}: (xmin int32 [n], size int32 [n], weights fp32 [n, T]) is needed")
    lo, size, wt = tab
    _refuse(any(not isinstance(t, torch.Tensor) or not t.is_contiguous() for t in tab) or lo.dtype != torch.int32 or size.dtype != torch.int32
            or wt.dtype != torch.float32 or wt.ndim != 2 or tuple(lo.shape) != (n_out,) or tuple(size.shape) != (n_out,) or wt.shape[0] != n_out,
            f"{name}: contiguous int32 [{n_out}], int32 [{n_out}] and fp32 [{n_out}, T] are needed")
    T = wt.shape[1]
    _refuse(not 1 <= T <= PICTURE_MAX_TAPS, f"{name}: rows of {T} taps, served: 1..{PICTURE_MAX_TAPS} (CD360_PICTURE_MAX_TAPS)")
    return T


def picture_resample(src: torch.Tensor, window, xtab, ytab, oh: int, ow: int, fill: int = 0, round_u8: bool = True, div: float = 255.0,
                     mul: float = 2.0, add: float = -1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Crop + separable resize of one uint8 picture into fp32 planes [C, oh, ow] (cd360_picture_resample_u8): src uint8 [H, W, C] (C = 1 or
    3; [H, W] is one channel) with any row stride; window = (left, top, w, h) in picture pixels, which may leave the picture (`fill`
    there); xtab / ytab = (xmin, size, weights) device tensors resizing w -> ow and h -> oh (cd360.pictures.device_taps).  Horizontal
    pass, then vertical, the taps in rising order in fp32; round_u8: round and clamp to 0..255 after each pass (the image library's uint8
    storage); last (v / div) * mul + add.  out: a contiguous fp32 [C, oh, ow] view to write, e.g. one slot of a batch tensor."""
    from . import _picture
    C = _u8_picture(src, "src", (1, 3))
    H, W = src.shape[:2]
    left, top, w, h = _window_arg(window)
    _refuse(oh <= 0 or ow <= 0, f"oh, ow must be positive, got {oh}, {ow}")
    tx, ty = _tap_table(xtab, ow, "xtab"), _tap_table(ytab, oh, "ytab")
    _refuse(not 0 <= int(fill) <= 255, f"fill = {fill}: a byte is needed")
    _refuse(not all(math.isfinite(float(v)) for v in (div, mul, add)) or float(div) == 0.0, f"div, mul, add = {div}, {mul}, {add}: finite values, div != 0")
    _refuse(C * h * ow >= 1 << 31 or C * oh * ow >= 1 << 31, f"{C} planes of {h} x {ow} or {oh} x {ow} do not fit 32-bit offsets")
    out = _out_arg(out, (C, oh, ow), torch.float32, src, "src")
    _need_gpu(src, *xtab, *ytab, out)
    work = torch.empty((C, h, ow), dtype=torch.float32, device=src.device)
    check(_picture.load().cd360_picture_resample_u8(_ptr(src), H, W, C, src.stride(0), left, top, w, h, int(fill), _ptr(xtab[0]), _ptr(xtab[1]),
                                                    _ptr(xtab[2]), tx, _ptr(ytab[0]), _ptr(ytab[1]), _ptr(ytab[2]), ty, oh, ow, int(bool(round_u8)),
                                                    float(div), float(mul), float(add), _ptr(work), _ptr(out), _stream()),
          "cd360_picture_resample_u8")
    return out


def picture_mask(src: torch.Tensor, window, oh: int, ow: int, thr: int = 125, k: int = 7, want=(True, True, True), out=None):
    """The maps of one uint8 mask [H, W] (cd360_picture_mask_u8) -> (opacity, mask, inside), fp32 [oh, ow] each, None where `want` says so:
    opacity = (src > thr) through the crop `window` (0 outside the picture) and the nearest resize of a boolean image; mask = its k x k
    dilation with zero padding, clamp(conv2d(opacity, ones), 0, 1); inside = the all-ones picture through the same crop and resize.  out:
    three contiguous fp32 [oh, ow] views (or None) to write instead of fresh tensors."""
    from . import _picture
    _u8_picture(src, "src", (1,))
    H, W = src.shape[:2]
    left, top, w, h = _window_arg(window)
    _refuse(oh <= 0 or ow <= 0 or oh * ow >= 1 << 31, f"oh, ow must be positive with oh * ow < 2^31, got {oh}, {ow}")
    _refuse(not 0 <= int(thr) <= 255, f"thr = {thr}: a byte is needed")
    _refuse(k < 1 or k % 2 == 0 or k > PICTURE_MAX_DILATE, f"k = {k}: an odd window of 1..{PICTURE_MAX_DILATE} is needed")
    out = (None, None, None) if out is None else tuple(out)
    _refuse(len(want) != 3 or len(out) != 3 or not any(want), "want, out: three entries (opacity, mask, inside), one wanted at the least")
    outs = [_out_arg(o, (oh, ow), torch.float32, src, "src") if wanted else None for o, wanted in zip(out, want)]
    live = [o for o in outs if o is not None]
    _refuse(any(_overlaps(a, b) for n, a in enumerate(live) for b in live[n + 1:]), "out: two outputs overlap")
    _need_gpu(src, *live)
    check(_picture.load().cd360_picture_mask_u8(_ptr(src), H, W, src.stride(0), int(thr), left, top, w, h, oh, ow, k, _ptr(outs[0]), _ptr(outs[1]),
                                                _ptr(outs[2]), _stream()), "cd360_picture_mask_u8")
    return tuple(outs)


# ----------------------------------------------------------------------------------------------- rank-r adapters (add_lora=True)
LOWRANK_RANKS = (8, 16, 32, 64)
_DROPOUT_STATE = {}  # device -> int64 [2] (seed, offset) read by the mask of cd360_lowrank_add_bf16 / cd360_dropout_apply_bf16
_DROPOUT_DRAW = [0]  # host-side draw index of the current step: every mask drawn in a step gets its own site


def dropout_state(device) -> torch.Tensor:
    """The (seed, offset) pair of the adapter dropout masks on `device` (int64 [2] in device memory).  The seed is drawn once from
    torch's CPU generator (so torch.manual_seed decides it); the offset advances through dropout_tick()."""
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    st = _DROPOUT_STATE.get(dev)
    if st is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        st = _DROPOUT_STATE[dev] = torch.tensor([seed, 0], dtype=torch.int64, device=dev)
    return st


def dropout_tick(device=None) -> None:
    """Once per training step (finetune.train_step): advance the mask offset on the device (cd360_dropout_tick: a captured step draws
    new masks on every replay) and restart the host-side draw index, so eager and replayed steps see the same site sequence."""
    st = dropout_state(torch.device("cuda") if device is None else device)
    check(_lib.load().cd360_dropout_tick(_ptr(st), _stream()), "cd360_dropout_tick")
    _DROPOUT_DRAW[0] = 0


def dropout_site(site: int) -> int:
    """`site` (block x 8 + {attn1, attn2} x 4 + {q, k, v, o}) combined with the next draw index of the step."""
    d = _DROPOUT_DRAW[0]
    _DROPOUT_DRAW[0] = d + 1
    return int(site) + (d << 24)


def _aligned_rows(t: torch.Tensor) -> bool:
    if not (t.is_cuda and t.dtype == torch.bfloat16 and t.dim() >= 1 and t.stride(-1) == 1 and t.data_ptr() % 16 == 0):
        return False
    try:
        _, ld = _rows2d(t)
    except Cd360Error:
        return False
    return ld % 8 == 0


def lowrank_add_ok(t: torch.Tensor, u: torch.Tensor, base: Optional[torch.Tensor] = None) -> bool:
    """Shape envelope of cd360_lowrank_add_bf16: t [..., r] with r in LOWRANK_RANKS, u [N, r] with N % 16 == 0, base [..., N]; bf16 on the GPU,
    16-byte aligned rows (strided column slices of a wider buffer are fine)."""
    if not (u.dim() == 2 and t.shape[-1] in LOWRANK_RANKS and u.shape[1] == t.shape[-1] and u.shape[0] % 16 == 0):
        return False
    if not (_aligned_rows(t) and _aligned_rows(u)):
        return False
    return base is None or (_aligned_rows(base) and base.shape[-1] == u.shape[0] and base.shape[:-1] == t.shape[:-1])


def lowrank_add(t: torch.Tensor, u: torch.Tensor, base: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, p: float = 0.0,
                site: int = 0, key: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out [..., N] = base + s * keep * (t [..., r] @ u [N, r]^T) on cd360_lowrank_add_bf16 (fp32 MFMA, one bf16 rounding).  base None reads
    as zero; out may be base (in place) or any view with the same rows.  p > 0 applies the adapter dropout (keep drawn from `key`, an int64
    (seed, offset) pair on the device -- dropout_state() by default -- and `site`; s = 1 / (1 - p)).  Not recorded by autograd (grad.LoraFn)."""
    _need_gpu(t, u, base, out)
    assert lowrank_add_ok(t, u, base), "cd360 lowrank_add: see lowrank_add_ok()"
    M, ldt = _rows2d(t)
    N, r = u.shape
    if out is None:
        out = torch.empty(*t.shape[:-1], N, dtype=torch.bfloat16, device=t.device)
    assert _aligned_rows(out) and out.shape[-1] == N
    mo, ldo = _rows2d(out)
    ldb = 0
    if base is not None:
        mb, ldb = _rows2d(base)
        assert mb == M
    assert mo == M
    if p > 0 and key is None:
        key = dropout_state(t.device)
    with _timed(_shape_tag("lowrank_add", M, N, r), 2.0 * M * N * r, 2.0 * (M * N * (2 if base is not None else 1) + M * r + N * r)):
        check(_lib.load().cd360_lowrank_add_bf16(_ptr(base), ldb, _ptr(t), ldt, _ptr(u), u.stride(0), _ptr(out), ldo, M, N, r, float(p),
                                                 _ptr(key) if p > 0 else None, int(site), _stream()), "cd360_lowrank_add_bf16")
    return out


def dropout_apply_ok(dy: torch.Tensor) -> bool:
    return _aligned_rows(dy) and dy.shape[-1] % 8 == 0


def dropout_apply(dy: torch.Tensor, p: float, site: int, key: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """s * keep * dy with the mask lowrank_add draws for the same (key, site, element) (cd360_dropout_apply_bf16): the adapter dropout's
    backward."""
    _need_gpu(dy, out)
    assert dropout_apply_ok(dy) and 0.0 <= p < 1.0
    M, ldd = _rows2d(dy)
    N = dy.shape[-1]
    if out is None:
        out = torch.empty(*dy.shape[:-1], N, dtype=torch.bfloat16, device=dy.device)
    mo, ldo = _rows2d(out)
    assert mo == M and _aligned_rows(out)
    if key is None:
        key = dropout_state(dy.device)
    with _timed("dropout_apply", 0.0, 4.0 * M * N):
        check(_lib.load().cd360_dropout_apply_bf16(_ptr(dy), ldd, _ptr(out), ldo, M, N, float(p), _ptr(key), int(site), _stream()),
              "cd360_dropout_apply_bf16")
    return out


def lora_ok(x: torch.Tensor, base_out: torch.Tensor, down: torch.Tensor, up: torch.Tensor) -> bool:
    """grad.LoraFn can serve base_out + drop(x down^T up^T): the down GEMM (cd360_gemm_bf16, K = in % 64), the adapter add, and in the
    backward the up-weight transpose GEMM (K = out % 64)."""
    if not (x.is_cuda and x.dtype == torch.bfloat16 and down.dtype == torch.bfloat16 and up.dtype == torch.bfloat16 and base_out.dtype == torch.bfloat16):
        return False
    r, K = down.shape
    N = up.shape[0]
    if up.shape[1] != r or r not in LOWRANK_RANKS or x.shape[-1] != K or base_out.shape[-1] != N:
        return False
    M = x.numel() // max(K, 1)
    return gemm_ok(M, r, K) and gemm_ok(M, r, N) and N % 16 == 0 and base_out.stride(-1) == 1


# ----------------------------------------------------------------------------------------------- prompt encoders (include/text/cd360_text.h)
# libcd360_text.so through cd360/_text.py.  Forward only: a tensor on a tape raises (_need_gpu).
TEXT_MAX_TOKENS = 128  # CD360_TEXT_MAX_TOKENS
ACT_QUICK_GELU, ACT_GELU = 0, 1


def text_embed(ids: torch.Tensor, tok: torch.Tensor, pos: torch.Tensor, want_stats: bool = False, ids_host: Optional[torch.Tensor] = None):
    """bf16(fp32(tok[ids]) + fp32(pos[n])) -> [B, N, D] bf16 (cd360_text_embed_bf16); want_stats=True returns (out, stats fp32 [B*N, 1, 2]),
    the row statistics gemm(..., ln=...) reads.  ids int64 [B, N] on the GPU; tok [V, D], pos [>= N, D] bf16 contiguous.  `ids_host`: the same
    ids where they came from (a CPU tensor): checked against [0, V) here, before the launch -- the kernel itself writes a zero row for an id
    outside the table and reads nothing out of bounds."""
    _need_gpu(ids, tok, pos)
    assert ids.dtype == torch.int64 and ids.dim() == 2 and ids.is_contiguous()
    assert tok.dtype == torch.bfloat16 and pos.dtype == torch.bfloat16 and tok.dim() == 2 and pos.dim() == 2 and tok.is_contiguous() and pos.is_contiguous()
    B, N = ids.shape
    V, D = tok.shape
    assert pos.shape[0] >= N and pos.shape[1] == D
    if ids_host is not None and ids_host.numel() and (int(ids_host.min()) < 0 or int(ids_host.max()) >= V):
        raise ValueError(f"token ids outside the table: [{int(ids_host.min())}, {int(ids_host.max())}] for {V} rows")
    out = torch.empty(B, N, D, dtype=torch.bfloat16, device=ids.device)
    stats = torch.empty(B * N, 1, 2, dtype=torch.float32, device=ids.device) if want_stats else None
    from . import _text
    with _timed("text_embed", 0.0, 2.0 * 3 * B * N * D):
        check(_text.load().cd360_text_embed_bf16(_ptr(ids), _ptr(tok), _ptr(pos), _ptr(out), B, N, V, D, D, _ptr(stats), _stream()),
              "cd360_text_embed_bf16")
    return (out, stats) if want_stats else out


def causal_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: float = 64 ** -0.5, n: Optional[int] = None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Causal softmax(scale q k^T) v per head, head dim 64, at most TEXT_MAX_TOKENS tokens (cd360_text_causal_attn_bf16).  q, k, v
    [b, >= n, H*64] with a contiguous last dim and free row / batch strides (the three column slices of one merged q|k|v projection are
    consumed in place) -> [b, n, H*64].  `n` limits the tokens when the buffers hold more rows: rows >= n are never read."""
    _need_gpu(q, k, v)
    b, rows, inner = q.shape
    n = rows if n is None else n
    assert inner == heads * 64 and q.dtype == torch.bfloat16 and k.dtype == torch.bfloat16 and v.dtype == torch.bfloat16
    assert q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1 and k.shape[-1] == inner and v.shape[-1] == inner
    assert 1 <= n <= TEXT_MAX_TOKENS and rows >= n and k.shape[1] >= n and v.shape[1] >= n and k.shape[0] == b and v.shape[0] == b
    if out is None:
        out = torch.empty(b, n, inner, dtype=torch.bfloat16, device=q.device)
    assert out.shape == (b, n, inner) and out.dtype == torch.bfloat16 and out.stride(2) == 1
    strides = (_I64x3(q.stride(0), 64, q.stride(1)), _I64x3(k.stride(0), 64, k.stride(1)),
               _I64x3(v.stride(0), 64, v.stride(1)), _I64x3(out.stride(0), 64, out.stride(1)))
    from . import _text
    with _timed("text_causal_attn", 2.0 * b * heads * n * (n + 1) * 64, 2.0 * 4 * b * n * inner):
        check(_text.load().cd360_text_causal_attn_bf16(_ptr(q), _ptr(k), _ptr(v), _ptr(out), b, heads, n, *strides, float(scale), _stream()),
              "cd360_text_causal_attn_bf16")
    return out


def text_activation(x: torch.Tensor, kind: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """kind ACT_QUICK_GELU: x * sigmoid(1.702 x); ACT_GELU: exact (erf) GELU -- fp32 inside, bf16 in and out (cd360_text_act_bf16).
    x [..., n] bf16 whose leading dims collapse to uniformly strided rows; out like x (default: a fresh contiguous tensor; out=x: in place)."""
    _need_gpu(x)
    rows, ld = _rows2d(x)
    n = x.shape[-1]
    if out is None:
        out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    ro, ldo = _rows2d(out)
    assert ro == rows and out.shape[-1] == n
    from . import _text
    with _timed("text_act", 0.0, 2.0 * 2 * rows * n):
        check(_text.load().cd360_text_act_bf16(_ptr(x), _ptr(out), rows, n, ld, ldo, int(kind), _stream()), "cd360_text_act_bf16")
    return out


def eot_pool(x: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """x [B, N, D] bf16, ids int64 [B, N] on the GPU -> [B, D]: row argmax_n ids[b, n] of every prompt, the lowest index on ties; the argmax
    runs on the device (cd360_text_eot_pool_bf16)."""
    _need_gpu(x, ids)
    assert x.dtype == torch.bfloat16 and x.dim() == 3 and x.stride(2) == 1 and x.stride(0) == x.shape[1] * x.stride(1)
    assert ids.dtype == torch.int64 and ids.is_contiguous() and tuple(ids.shape) == tuple(x.shape[:2])
    B, N, D = x.shape
    out = torch.empty(B, D, dtype=torch.bfloat16, device=x.device)
    from . import _text
    with _timed("text_eot_pool", 0.0, 2.0 * 2 * B * D):
        check(_text.load().cd360_text_eot_pool_bf16(_ptr(x), _ptr(ids), _ptr(out), B, N, D, x.stride(1), D, _stream()), "cd360_text_eot_pool_bf16")
    return out


# ----------------------------------------------------------------------------------------------- prompt encoders, backward (include/textgrad/cd360_textgrad.h)
# libcd360_textgrad.so through cd360/_textgrad.py: what grad.TextTowerFn launches beside gemm() and add_layernorm_bwd().
TEXTGRAD_MAX_MODIFIERS = 3  # CD360_TEXTGRAD_MAX_MODIFIERS


def _head_strides(t: torch.Tensor):
    return _I64x3(t.stride(0), 64, t.stride(1))


def causal_attention_bwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, d_o: torch.Tensor, heads: int, scale: float = 64 ** -0.5,
                         n: Optional[int] = None, out=None):
    """Backward of causal_attention (cd360_textgrad_causal_attn_bwd_bf16): q, k, v as there (the three column slices of the saved merged
    projection are consumed in place), d_o [b, >= n, H*64] -> (dq, dk, dv), the three column slices of ONE fresh [b, n, 3*H*64] buffer, or
    the three tensors of `out`.  The probabilities are recomputed in fp32; no atomics: the same bits on every run.  Rows >= n are neither
    read nor written."""
    _need_gpu(q, k, v, d_o)
    b, rows, inner = q.shape
    n = rows if n is None else n
    assert inner == heads * 64 and all(t.dtype == torch.bfloat16 and t.dim() == 3 and t.stride(2) == 1 and t.shape[2] == inner and t.shape[0] == b
                                       and t.shape[1] >= n for t in (q, k, v, d_o))
    assert 1 <= n <= TEXT_MAX_TOKENS
    if out is None:
        buf = torch.empty(b, n, 3 * inner, dtype=torch.bfloat16, device=q.device)
        out = (buf[..., :inner], buf[..., inner:2 * inner], buf[..., 2 * inner:])
    dq, dk, dv = out
    assert all(t.dtype == torch.bfloat16 and t.dim() == 3 and t.stride(2) == 1 and t.shape[2] == inner and t.shape[0] == b and t.shape[1] >= n
               for t in out)
    from . import _textgrad
    with _timed("textgrad_causal_attn_bwd", 5 * 2.0 * b * heads * n * (n + 1) / 2 * 64, 2.0 * 7 * b * n * inner):
        check(_textgrad.load().cd360_textgrad_causal_attn_bwd_bf16(_ptr(q), _ptr(k), _ptr(v), _ptr(d_o), _ptr(dq), _ptr(dk), _ptr(dv), b, heads, n,
                                                                   *(_head_strides(t) for t in (q, k, v, d_o, dq, dk, dv)), float(scale), _stream()),
              "cd360_textgrad_causal_attn_bwd_bf16")
    return dq, dk, dv


def text_activation_bwd(x: torch.Tensor, dy: torch.Tensor, kind: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dy * f'(x) for the activation `kind` of text_activation, x the saved pre-activation (cd360_textgrad_act_bwd_bf16): fp32 inside, bf16 in
    and out.  x, dy [..., n] bf16 whose leading dims collapse to uniformly strided rows; out like dy (default: fresh; out=dy: in place)."""
    _need_gpu(x, dy)
    rows, ld = _rows2d(x)
    rd, ldd = _rows2d(dy)
    n = x.shape[-1]
    if out is None:
        out = torch.empty(dy.shape, dtype=torch.bfloat16, device=dy.device)
    ro, ldo = _rows2d(out)
    assert rd == rows and ro == rows and dy.shape[-1] == n and out.shape[-1] == n
    from . import _textgrad
    with _timed("textgrad_act_bwd", 0.0, 2.0 * 3 * rows * n):
        check(_textgrad.load().cd360_textgrad_act_bwd_bf16(_ptr(x), _ptr(dy), _ptr(out), rows, n, ld, ldd, ldo, int(kind), _stream()),
              "cd360_textgrad_act_bwd_bf16")
    return out


def eot_scatter(d_pooled: torch.Tensor, ids: torch.Tensor, dx: torch.Tensor) -> torch.Tensor:
    """Backward of eot_pool, IN PLACE on dx [B, N, D] bf16: row argmax_n ids[b, n] of prompt b (the lowest index on ties, found on the device)
    becomes bf16(fp32(row) + fp32(d_pooled[b])); every other row stays (cd360_textgrad_eot_scatter_bf16).  -> dx."""
    _need_gpu(d_pooled, ids, dx)
    assert dx.dtype == torch.bfloat16 and dx.dim() == 3 and dx.stride(2) == 1 and dx.stride(0) == dx.shape[1] * dx.stride(1)
    assert ids.dtype == torch.int64 and ids.is_contiguous() and tuple(ids.shape) == tuple(dx.shape[:2])
    B, N, D = dx.shape
    assert d_pooled.dtype == torch.bfloat16 and tuple(d_pooled.shape) == (B, D) and d_pooled.stride(1) == 1
    from . import _textgrad
    with _timed("textgrad_eot_scatter", 0.0, 2.0 * 3 * B * D):
        check(_textgrad.load().cd360_textgrad_eot_scatter_bf16(_ptr(d_pooled), _ptr(ids), _ptr(dx), B, N, D, d_pooled.stride(0) if B > 1 else D,
                                                               dx.stride(1), _stream()), "cd360_textgrad_eot_scatter_bf16")
    return dx


def token_rows_grad(d_x0: torch.Tensor, ids: torch.Tensor, modifier_ids) -> torch.Tensor:
    """d_x0 [B, N, D] bf16 (the gradient at the embedding's output), ids int64 [B, N] on the GPU, modifier_ids: up to TEXTGRAD_MAX_MODIFIERS
    host ints -> fp32 [k, D]: for every modifier id the sum of the rows of d_x0 at the positions that hold it, in rising (b, n) order; a zero
    row for a modifier that occurs nowhere (cd360_textgrad_token_rows_f32).  No atomics: the same bits on every run."""
    _need_gpu(d_x0, ids)
    assert d_x0.dtype == torch.bfloat16 and d_x0.dim() == 3 and d_x0.stride(2) == 1 and d_x0.stride(0) == d_x0.shape[1] * d_x0.stride(1)
    assert ids.dtype == torch.int64 and ids.is_contiguous() and tuple(ids.shape) == tuple(d_x0.shape[:2])
    mods = [int(m) for m in modifier_ids]
    k = len(mods)
    assert 1 <= k <= TEXTGRAD_MAX_MODIFIERS
    B, N, D = d_x0.shape
    out = torch.empty(k, D, dtype=torch.float32, device=d_x0.device)
    from . import _textgrad
    with _timed("textgrad_token_rows", 0.0, 2.0 * B * N * D + 4.0 * k * D):
        check(_textgrad.load().cd360_textgrad_token_rows_f32(_ptr(d_x0), _ptr(ids), (ctypes.c_int64 * k)(*mods), _ptr(out), B, N, D, k, d_x0.stride(1),
                                                             _stream()), "cd360_textgrad_token_rows_f32")
    return out
