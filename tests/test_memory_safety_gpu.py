"""Every launching entry point of the C ABI under tests/guarded.py: where did the kernel write, and what did it read?

Each case runs twice (poison 0xFF, then 0x7F) with every output and workspace of the binding allocated between canary guards:
P1 no guard byte changed, P2 results bit-equal between the runs and finite, P3 operands unchanged, P4 the declared entry points ran.
Parity is NOT re-asserted here (the shapes are those the parity tests already trust).  No tolerance: canary and bit equality only.
The weight prefetcher stays disarmed (its side-stream kernel: tests/test_prefetch_gpu.py); captured paths are out of scope."""
import ctypes
import os
import re
import sys
from collections import namedtuple

import pytest
import torch

import guarded as G
import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

DEV = "cuda"
BF = torch.bfloat16

Case = namedtuple("Case", "name build declares inout valid bit_equal tuning grad")
CASES = []


def add(name, build, declares, inout=(), valid=None, bit_equal=True, tuning=None, grad=False):
    assert all(c.name != name for c in CASES), name
    CASES.append(Case(name, build, tuple(declares), tuple(inout), valid, bit_equal, tuning or {}, grad))


def R(*shape, seed=0, scale=1.0, dtype=BF):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(dtype)


def guardfn(fn):
    fn.wants_guard = True
    return fn


def _ops():
    from cd360 import ops
    return ops


# ================================================================================================ GEMM family
def gemm_case(M, N, K, epi="", lda=None, seed=0):
    def build():
        from bench_gemm import rnd
        ops = _ops()
        af = rnd(M, lda or K, seed=seed + 1).to(BF)
        d = dict(a=af[:, :K], a_full=af, w=rnd(N, K, seed=seed + 2, scale=K ** -0.5).to(BF), bias=None, res=None, stats=None, wsum=None)
        if "bias" in epi:
            d["bias"] = rnd(N, seed=seed + 3)
        if "res" in epi:
            d["res"] = rnd(M, N, seed=seed + 4).to(BF)
        if "ln" in epi:
            d["w"], d["wsum"], d["bias"] = ops.pack_ln_linear(d["w"], None, 1 + 0.2 * rnd(K, seed=5), 0.1 * rnd(K, seed=6))
            d["stats"] = ops.row_stats(d["a"])

        def fn(a, a_full, w, bias, res, stats, wsum):
            return ops.gemm(a, w, bias=bias, res=res, ln=None if stats is None else (stats, wsum, 1e-5), want_stats="stats" in epi,
                            geglu="geglu" in epi)
        return fn, d
    return build


for cfg in range(1, 10):  # every forced tiling, a ragged and a product-like shape
    for M, N, K in ((300, 272, 320), (777, 1280, 640)):
        add(f"gemm-cfg{cfg}-{M}x{N}x{K}", gemm_case(M, N, K, "bias res stats"), ["cd360_gemm_bf16"], tuning=dict(gemm_cfg=cfg))
for name, M, N, K, epi in (("L1 qkv", 12288, 1920, 640, "ln"), ("L1 out", 12288, 640, 640, "res"), ("L1 ff1", 12288, 5120, 640, "geglu"),
                           ("L1 ff2", 12288, 640, 2560, "res"), ("L2 qkv", 3072, 3840, 1280, "ln"), ("L2 out", 3072, 1280, 1280, "res"),
                           ("L2 ff1", 3072, 10240, 1280, "geglu"), ("L2 ff2", 3072, 1280, 5120, "res"), ("A3 q L1", 98304 * 3, 640, 640, "ln"),
                           ("A3 q L2", 24576 * 3, 1280, 1280, "ln"), ("4k cube", 4096, 4096, 4096, "")):
    add(f"gemm-auto-{name.replace(' ', '-')}", gemm_case(M, N, K, epi + " bias" if epi in ("res", "geglu") else epi), ["cd360_gemm_bf16"])
for epi in ("bias", "res", "ln", "geglu bias", "stats", "ln stats", "bias res stats"):
    for M, N, K in ((300, 272, 320), (3072, 1280, 1280)):
        if "geglu" in epi and N % 64:
            N = 320
        add(f"gemm-epi-{epi.replace(' ', '+')}-{M}x{N}x{K}", gemm_case(M, N, K, epi, seed=7), ["cd360_gemm_bf16"])
add("gemm-lda-gt-K-300x272x320", gemm_case(300, 272, 320, "bias", lda=392), ["cd360_gemm_bf16"])
add("gemm-lda-gt-K-3072x1280x1280", gemm_case(3072, 1280, 1280, "res", lda=1288), ["cd360_gemm_bf16"])


def test_shapes_match_bench_gemm():
    """The auto-dispatch cases above are bench_gemm.SHAPES (the step's GEMMs), name by name."""
    from bench_gemm import SHAPES
    names = {c.name for c in CASES}
    for name, M, N, K, _ in SHAPES:
        assert f"gemm-auto-{name.replace(' ', '-')}" in names, name


def cstats_case(M, N, K):
    def build():
        from bench_gemm import rnd
        ops = _ops()
        d = dict(a=rnd(M, K, seed=31).to(BF), w=rnd(N, K, seed=32, scale=K ** -0.5).to(BF), b=rnd(N, seed=33), r=rnd(M, N, seed=34).to(BF))
        return (lambda a, w, b, r: ops.gemm_cstats(a, w, bias=b, res=r)), d
    return build


for ks in (0, 1):
    add(f"gemm-cstats-ksplit{ks}-3072x1280x1280", cstats_case(3072, 1280, 1280), ["cd360_gemm_cstats_bf16"], tuning=dict(gemm_ksplit=ks))
add("gemm-cstats-small-batch-1024x1280x1280", cstats_case(1024, 1280, 1280), ["cd360_gemm_cstats_bf16"])
add("gemm-cstats-12288x640x640", cstats_case(12288, 640, 640), ["cd360_gemm_cstats_bf16"])


def row_stats_case(rows, C, ld):
    def build():
        xf = R(rows, ld, seed=rows)
        return (lambda x, x_full: _ops().row_stats(x)), dict(x=xf[:, :C], x_full=xf)
    return build


add("row-stats-37x320", row_stats_case(37, 320, 320), ["cd360_row_stats_bf16"])
add("row-stats-strided-3072x1280", row_stats_case(3072, 1280, 1288), ["cd360_row_stats_bf16"])


def gemm_tn_case(M, N, K, out_dtype, lda=None, ldb=None):
    def build():
        af, bfull = R(M, lda or N, seed=M), R(M, ldb or K, seed=M + 1)
        return (lambda a, b, a_full, b_full: _ops().gemm_tn(a, b, out_dtype=out_dtype)), dict(a=af[:, :N], b=bfull[:, :K], a_full=af, b_full=bfull)
    return build


add("gemm-tn-bf16-333x136x72", gemm_tn_case(333, 136, 72, BF), ["cd360_gemm_tn_bf16"])
add("gemm-tn-fp32-strided-333x136x72", gemm_tn_case(333, 136, 72, torch.float32, lda=144, ldb=80), ["cd360_gemm_tn_bf16"])
add("gemm-tn-bf16-12288x640x640", gemm_tn_case(12288, 640, 640, BF), ["cd360_gemm_tn_bf16"])
add("gemm-tn-fp32-strided-3072x1280x32", gemm_tn_case(3072, 1280, 32, torch.float32, lda=3840, ldb=40), ["cd360_gemm_tn_bf16"])


def lowrank_case(M, N, r, p, base=True):
    def build():
        d = dict(t=R(M, r, seed=1), u=R(N, r, seed=2, scale=0.1), base=R(M, N, seed=3) if base else None,
                 key=torch.tensor([1234, 5], dtype=torch.int64, device=DEV))
        return (lambda t, u, base, key: _ops().lowrank_add(t, u, base=base, p=p, site=3, key=key)), d
    return build


add("lowrank-add-333x640-r32", lowrank_case(333, 640, 32, 0.0), ["cd360_lowrank_add_bf16"])
add("lowrank-add-dropout-3072x1280-r32", lowrank_case(3072, 1280, 32, 0.1), ["cd360_lowrank_add_bf16"])
add("lowrank-add-nobase-77x640-r16", lowrank_case(77, 640, 16, 0.0, base=False), ["cd360_lowrank_add_bf16"])
add("lowrank-add-r64-1000x320", lowrank_case(1000, 320, 64, 0.0), ["cd360_lowrank_add_bf16"])


def pose_embed_case(rows, C):
    def build():
        d = dict(x=R(rows, C, seed=1), xref=R(rows, C, seed=2), wa=R(C, C, seed=3, scale=C ** -0.5), wb=R(C, C, seed=4, scale=C ** -0.5))
        return _ops().pose_embed, d
    return build


add("pose-embed-333x320", pose_embed_case(333, 320), ["cd360_pose_embed_bf16"])
add("pose-embed-3072x1280", pose_embed_case(3072, 1280), ["cd360_pose_embed_bf16"])


# ================================================================================================ fused attention
def qattn_inputs(b, nq, C, K, nk, dup=0):
    ops = _ops()
    a = (R(b, nq, K, seed=11).float() * (0.5 + R(b, nq, 1, seed=12).float().abs()) + 0.5 * R(b, nq, 1, seed=13).float()).to(BF)
    w = R(C, K, seed=14, scale=K ** -0.5, dtype=torch.float32)
    kv = R(b + dup, max(80, nk), 2 * C, seed=15)
    wp, wsum, cb = ops.pack_ln_linear(w, None, 1 + 0.2 * R(K, seed=5, dtype=torch.float32), 0.1 * R(K, seed=6, dtype=torch.float32))
    return dict(a=a, w=wp, kv=kv, bias=cb, stats=ops.row_stats(a), wsum=wsum)


def qattn_case(b, nq, C, K, nk, form, dup=0):
    heads = C // 64

    def build():
        ops = _ops()
        d = qattn_inputs(b, nq, C, K, nk, dup)

        def dedup(a, w, kv, bias, stats, wsum):
            return ops.qproj_attention(a, w, kv[..., :C], kv[..., C:], nk, heads, bias=bias, ln=(stats, wsum, 1e-5), dup=dup)

        def fp8(a, w, kv, bias, stats, wsum):
            packed = ops.kv_pack_fp8(kv[..., :C], kv[..., C:], nk, heads)
            return ops.qproj_attention(a, w, None, None, nk, heads, bias=bias, ln=(stats, wsum, 1e-5), dup=dup, fp8=packed), packed

        @guardfn
        def plain(a, w, kv, bias, stats, wsum, guard):  # cd360_qproj_attn_bf16: the entry without the CFG de-duplication (not wrapped by ops)
            out = guard.torch.empty(b, nq, C, dtype=BF, device=DEV)
            k, v = kv[..., :C], kv[..., C:]
            ops.check(guard.lib.cd360_qproj_attn_bf16(a.data_ptr(), w.data_ptr(), out.data_ptr(), b * nq, C, K, K, w.stride(0), C, bias.data_ptr(),
                                                      stats.data_ptr(), stats.shape[1], K, 1e-5, wsum.data_ptr(), k.data_ptr(), v.data_ptr(),
                                                      k.stride(0), k.stride(1), v.stride(0), v.stride(1), nq, nk, 64 ** -0.5, ops._stream()),
                      "cd360_qproj_attn_bf16")
            return out
        return dict(dedup=dedup, fp8=fp8, plain=plain)[form], d
    return build


for q in (1, 2, 3, 4):
    for nk in (20, 50, 77):
        for b, nq in ((2, 128), (1, 384)):
            tag = f"qcfg{q}-b{b}-nq{nq}-nk{nk}"
            add(f"qproj-attn-{tag}", qattn_case(b, nq, 640, 640, nk, "plain"), ["cd360_qproj_attn_bf16"], tuning=dict(qattn_cfg=q))
            add(f"qproj-attn-dedup-{tag}", qattn_case(b, nq, 640, 640, nk, "dedup", dup=1), ["cd360_qproj_attn_dedup_bf16"], tuning=dict(qattn_cfg=q))
    add(f"qproj-attn-fp8-qcfg{q}-nk77", qattn_case(2, 256, 640, 640, 77, "fp8", dup=1), ["cd360_qproj_attn_fp8_bf16", "cd360_kv_pack_fp8"],
        tuning=dict(qattn_cfg=q))


def kv_pack_case(B, heads, nk):
    """cd360_kv_pack_fp8 alone: it takes any Nk <= 96, while cd360_qproj_attn_fp8_bf16 takes 65 <= Nk <= 96 only (include/cd360_hip.h:500-504:
    "65 <= Nk <= 96 (CD360_ERR_SHAPE otherwise ...)"), so the fused fp8 cases above run at nk = 77 alone.  kv8 is compared whole: the header
    leaves no part of it unspecified."""
    def build():
        C = heads * 64
        return (lambda kv: _ops().kv_pack_fp8(kv[..., :C], kv[..., C:], nk, heads)), dict(kv=R(B, max(80, nk), 2 * C, seed=nk))
    return build


for nk in (1, 20, 50, 77, 96):
    add(f"kv-pack-fp8-b3-h10-nk{nk}", kv_pack_case(3, 10, nk), ["cd360_kv_pack_fp8"])
for nk in (65, 96):  # the two ends of the fused fp8 form's key envelope
    add(f"qproj-attn-fp8-auto-nk{nk}", qattn_case(2, 256, 640, 640, nk, "fp8", dup=1), ["cd360_qproj_attn_fp8_bf16", "cd360_kv_pack_fp8"])
add("qproj-attn-dedup-product-b3-nq4096-nk77", qattn_case(3, 4096, 640, 640, 77, "dedup", dup=1), ["cd360_qproj_attn_dedup_bf16"])
add("qproj-attn-fp8-product-b2-nq4096-nk77", qattn_case(2, 4096, 1280, 1280, 77, "fp8", dup=1), ["cd360_qproj_attn_fp8_bf16", "cd360_kv_pack_fp8"])


def attn_inputs(B, H, Nq, Nk, merged=False):
    if merged:
        qkv = R(B, Nq, 3 * H * 64, seed=Nq)
        return dict(qkv=qkv)
    nkp = (Nk + 7) // 8 * 8
    kv = R(B, nkp, 2 * H * 64 + 64, seed=Nq + Nk)  # k and v: column slices of one wider tensor, rows padded to 8
    return dict(q=R(B, Nq, H * 64, seed=B * 1000 + Nq + Nk), kv=kv)


def attn_case(B, H, Nq, Nk, form):
    def build():
        ops = _ops()
        inner = H * 64
        d = attn_inputs(B, H, Nq, Nk)
        kw = dict(plain={}, lse=dict(want_lse=True), prescaled=dict(prescaled=True))
        if form == "fp8mfma":
            return (lambda q, kv: ops.attention_fp8mfma(q, kv[..., :inner], kv[..., inner + 64:], H, nk=Nk)), d  # amax measured by the binding, as in the parity test
        if form == "xformers":
            d = dict(q=R(B * H, Nq, 64, seed=1), k=R(B * H, Nk, 64, seed=2), v=R(B * H, Nk, 64, seed=3))
            return ops.memory_efficient_attention, d
        return (lambda q, kv: ops.attention(q, kv[..., :inner], kv[..., inner + 64:], H, nk=Nk, **kw[form])), d
    return build


ATTN_SHAPES = ((1, 2, 333, 333), (1, 3, 200, 77), (2, 3, 1024, 1024))
for B, H, Nq, Nk in ATTN_SHAPES:
    s = f"{B}x{H}x{Nq}x{Nk}"
    add(f"attn-fwd-strided-{s}", attn_case(B, H, Nq, Nk, "plain"), ["cd360_attn_fwd_bf16"])
    add(f"attn-fwd-lse-{s}", attn_case(B, H, Nq, Nk, "lse"), ["cd360_attn_fwd_lse_bf16"])
    add(f"attn-fwd-prescaled-{s}", attn_case(B, H, Nq, Nk, "prescaled"), ["cd360_attn_fwd_prescaled_bf16"])
    add(f"attn-fwd-xformers-{s}", attn_case(B, H, Nq, Nk, "xformers"), ["cd360_attn_fwd_xformers_bf16"])
    if Nk <= 96:
        add(f"attn-fwd-fp8mfma-{s}", attn_case(B, H, Nq, Nk, "fp8mfma"), ["cd360_attn_fwd_fp8mfma_bf16"])
add("attn-fwd-fp8mfma-2x2x96x40", attn_case(2, 2, 96, 40, "fp8mfma"), ["cd360_attn_fwd_fp8mfma_bf16"])


def self_attn_case(B, H, N, prescaled):
    def build():
        ops = _ops()
        inner = H * 64

        def fn(qkv):
            if prescaled:
                return ops.attention(qkv[..., :inner], qkv[..., inner:2 * inner], qkv[..., 2 * inner:], H, N, prescaled=True)
            return ops.self_attention_qkv(qkv, H)
        return fn, attn_inputs(B, H, N, N, merged=True)
    return build


for gen in (0, 1, 2):
    for B, H, N in ((1, 2, 333), (2, 3, 1024)):
        add(f"self-attn-gen{gen}-{B}x{H}x{N}", self_attn_case(B, H, N, False), ["cd360_attn_fwd_bf16"], tuning=dict(attn_self=gen))
        add(f"self-attn-prescaled-gen{gen}-{B}x{H}x{N}", self_attn_case(B, H, N, True), ["cd360_attn_fwd_prescaled_bf16"], tuning=dict(attn_self=gen))


def attn_single_case(b, n, c=512):
    def build():
        qkv = R(b * n, 3 * c, seed=n + b, dtype=torch.float32)
        qkv[:, :c] *= 3.0 / c ** 0.5
        qkv = qkv.to(BF).view(b, n, 3 * c)
        return (lambda qkv: _ops().attention_single(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:])), dict(qkv=qkv)
    return build


# N -> key splits (cd360_attn_single_splits, a function of N alone): 1 .. 16, each at the first N that takes it (a ragged last key tile), plus the
# shapes of tests/test_vae_gpu.py (N = 1, 33 and 500 ragged; 4096 and 16384 = the 64^2 and 128^2 latents)
ATTN_SINGLE_SPLITS = {1: 1, 33: 1, 256: 1, 480: 1, 481: 2, 500: 2, 737: 3, 993: 4, 1249: 5, 1505: 6, 1761: 7, 2017: 8, 2273: 9, 2529: 10, 2785: 11,
                      3041: 12, 3297: 13, 3553: 14, 3809: 15, 4065: 16, 4096: 16, 4100: 15, 16384: 4}
for n in sorted(ATTN_SINGLE_SPLITS):
    add(f"attn-single-n{n}", attn_single_case(1, n), ["cd360_attn_single_bf16"])
add("attn-single-b2-n500", attn_single_case(2, 500), ["cd360_attn_single_bf16"])


def test_attn_single_cases_cover_every_split_count():
    """Host only (no gpu mark), but like tests/test_conv_routes_cpu.py it asks the built library: 70 000 calls of the host-side query
    cd360_attn_single_splits, well under a second.  Without the built library it fails with Cd360Error, as every test of the C ABI does."""
    from cd360 import ops
    assert all(ops.attention_single_splits(1, n) == s for n, s in ATTN_SINGLE_SPLITS.items())
    assert {ops.attention_single_splits(1, n) for n in range(1, 70000)} == set(ATTN_SINGLE_SPLITS.values())  # no split count without a case


def attn_bwd_case(B, H, Nq, Nk, form):
    def build():
        ops = _ops()
        inner = H * 64
        if form == "merged":
            qkv = R(B, Nq, 3 * inner, seed=Nq)
            q, k, v = qkv[..., :inner], qkv[..., inner:2 * inner], qkv[..., 2 * inner:]
        else:
            q, k, v = R(B, Nq, inner, seed=1), R(B, Nk, inner, seed=2), R(B, Nk, inner, seed=3)
        o, lse = ops.attention(q, k, v, H, Nk, want_lse=True)
        d = dict(q=q, k=k, v=v, o=o, dout=R(B, Nq, inner, seed=4), lse=lse)
        if form == "merged":  # dq | dk | dv: the three column slices (row stride 3 H 64) of ONE buffer, allocated poisoned between guards
            @guardfn
            def fn(q, k, v, o, dout, lse, guard):
                dqkv = guard.torch.empty(B, Nq, 3 * inner, dtype=BF, device=DEV)
                ops.attention_bwd(q, k, v, o, dout, lse, H, Nk, out=(dqkv[..., :inner], dqkv[..., inner:2 * inner], dqkv[..., 2 * inner:]))
                return dqkv
            return fn, d
        return (lambda q, k, v, o, dout, lse: ops.attention_bwd(q, k, v, o, dout, lse, H, Nk, need_dkv=form == "kv")), d
    return build


def self_attn_autograd_case(B, H, N):
    """The product route of the merged form: ops.self_attention_qkv under autograd, so that the d(q|k|v) buffer is grad.SelfAttentionFn's own
    torch.empty_like(qkv) -- the allocation that relies on the kernel writing every element."""
    def build():
        ops = _ops()

        def fn(qkv, dout):
            x = qkv.detach().clone().requires_grad_(True)
            y = ops.self_attention_qkv(x, H)
            y.backward(dout)
            return y.detach(), x.grad
        return fn, dict(qkv=R(B, N, 3 * H * 64, seed=N), dout=R(B, N, H * 64, seed=N + 1))
    return build


for B, H, Nq, Nk in ATTN_SHAPES:
    s = f"{B}x{H}x{Nq}x{Nk}"
    add(f"attn-bwd-kvgrad-{s}", attn_bwd_case(B, H, Nq, Nk, "kv"), ["cd360_attn_bwd_bf16"])
    add(f"attn-bwd-dq-only-{s}", attn_bwd_case(B, H, Nq, Nk, "q"), ["cd360_attn_bwd_bf16"])
    if Nq == Nk:
        add(f"attn-bwd-merged-qkv-{s}", attn_bwd_case(B, H, Nq, Nk, "merged"), ["cd360_attn_bwd_bf16"])
        add(f"attn-bwd-merged-qkv-autograd-{s}", self_attn_autograd_case(B, H, Nq), ["cd360_attn_fwd_lse_bf16", "cd360_attn_bwd_bf16"], grad=True)


# ================================================================================================ convolutions
def conv_inputs(N, H, W, Cin, Cout, extras, stride=1, seed=0):
    ops = _ops()
    w = R(Cout, Cin, 3, 3, seed=seed + 1, scale=(9 * Cin) ** -0.5, dtype=torch.float32)
    ho, wo = H // stride, W // stride
    return dict(x=R(N * H * W, Cin, seed=seed + 2), wp=ops.pack_conv_weight(w), bias=R(Cout, seed=seed + 3, dtype=torch.float32),
                emb=R(N, Cout, seed=seed + 4) if extras else None, res=R(N * ho * wo, Cout, seed=seed + 5) if extras else None)


def conv_dma_case(N, H, W, Cin, Cout, want_stats, extras=True):
    def build():
        ops = _ops()

        @guardfn
        def fn(x, wp, bias, emb, res, guard):  # cd360_conv3x3_dma_bf16 itself (ops.conv_igemm reaches it only through the dispatcher)
            out = guard.torch.empty(N * H * W, Cout, dtype=BF, device=DEV)
            stats = None
            route = ops.conv3x3_dma_route(N, H, W, Cin, Cout)
            assert route.family == "dma", route
            if want_stats:
                assert (H * W) % route.slab_rows == 0
                stats = guard.torch.empty(N * H * W // route.slab_rows, Cout, 2, dtype=torch.float32, device=DEV)
            ops.check(guard.lib.cd360_conv3x3_dma_bf16(x.data_ptr(), wp.data_ptr(), bias.data_ptr(), ops._ptr(emb), 0 if emb is None else emb.stride(0),
                                                       ops._ptr(res), out.data_ptr(), N, H, W, Cin, Cout, ops._ptr(stats), ops._stream()),
                      "cd360_conv3x3_dma_bf16")
            return out, stats
        return fn, conv_inputs(N, H, W, Cin, Cout, extras)
    return build


for cfg in range(1, 7):
    for halo in (-1, 1):
        h = "halo" if halo == 1 else "default"
        add(f"conv-dma-cfg{cfg}-{h}-stats-3x32x32x320x640", conv_dma_case(3, 32, 32, 320, 640, True), ["cd360_conv3x3_dma_bf16"],
            tuning=dict(conv_cfg=cfg, conv_halo=halo))
        add(f"conv-dma-cfg{cfg}-{h}-ragged-2x9x7x128x320", conv_dma_case(2, 9, 7, 128, 320, False), ["cd360_conv3x3_dma_bf16"],
            tuning=dict(conv_cfg=cfg, conv_halo=halo))
    add(f"conv-dma-cfg{cfg}-nostats-3x16x8x64x320", conv_dma_case(3, 16, 8, 64, 320, False, extras=False), ["cd360_conv3x3_dma_bf16"],
        tuning=dict(conv_cfg=cfg))
# the advisor's shape: tiling 3, M = 24576, Cout = 1280 at the 32^2 level (the halo form wrote twice the promised statistics rows), and a
# tiling-6 shape (half of the slabs stayed unwritten there)
for halo in (-1, 1):
    h = "halo" if halo == 1 else "default"
    add(f"conv-dma-cfg3-{h}-stats-24x32x32x1280x1280", conv_dma_case(24, 32, 32, 1280, 1280, True), ["cd360_conv3x3_dma_bf16"],
        tuning=dict(conv_cfg=3, conv_halo=halo))
    add(f"conv-dma-cfg6-{h}-stats-3x128x128x320x320", conv_dma_case(3, 128, 128, 320, 320, True), ["cd360_conv3x3_dma_bf16"],
        tuning=dict(conv_cfg=6, conv_halo=halo))
    add(f"conv-dma-auto-{h}-stats-3x32x32x1280x1280", conv_dma_case(3, 32, 32, 1280, 1280, True), ["cd360_conv3x3_dma_bf16"], tuning=dict(conv_halo=halo))
# the data gradient's channel counts (tests/conv_shapes.py UNET_DGRAD: Cout' = the forward Cin): three and six 320-channel tiles on tilings
# 1 and 6, 3.75 and 7.5 256-channel tiles on tiling 3, each also on the halo form
for cout in (960, 1920):
    for cfg in (1, 3, 6):
        for halo in (0, 1):
            add(f"conv-dma-cfg{cfg}-{'halo' if halo else 'taps'}-stats-2x16x8x64x{cout}", conv_dma_case(2, 16, 8, 64, cout, True),
                ["cd360_conv3x3_dma_bf16"], tuning=dict(conv_cfg=cfg, conv_halo=halo))


def conv_igemm_case(N, H, W, Cin, Cout, extras, want_stats, stride=1):
    def build():
        ops = _ops()
        return (lambda x, wp, bias, emb, res: ops.conv_igemm(x, wp, bias, N, H, W, 9, emb, res, want_stats=want_stats, stride=stride)), \
            conv_inputs(N, H, W, Cin, Cout, extras, stride)
    return build


for split in (-1, 1, 2):
    t = dict(conv_split=split, conv_dma=0)
    s = "auto" if split < 0 else split
    add(f"conv-igemm-split{s}-ragged-2x9x7x64x48", conv_igemm_case(2, 9, 7, 64, 48, False, False), ["cd360_conv_igemm_bf16"], tuning=t)
    add(f"conv-igemm-split{s}-stats-3x32x32x320x640", conv_igemm_case(3, 32, 32, 320, 640, True, True), ["cd360_conv_igemm_bf16"], tuning=t)
    add(f"conv-igemm-split{s}-stride2-3x32x32x320x320", conv_igemm_case(3, 32, 32, 320, 320, True, False, stride=2), ["cd360_conv_igemm_bf16"], tuning=t)
add("conv-igemm-dispatch-stats-3x64x64x640x640", conv_igemm_case(3, 64, 64, 640, 640, True, True), ["cd360_conv_igemm_bf16"])
add("conv-igemm-dispatch-stride2-1x8x12x128x160", conv_igemm_case(1, 8, 12, 128, 160, False, False, stride=2), ["cd360_conv_igemm_bf16"])


def conv_module_case(N, H, W, cin, cout, stride, backward):
    """The module wrapper (sgm...util.conv_tokens): channel padding 4 -> 320 / 320 -> 4, and under autograd the data-gradient route of
    tests/test_backward_gpu.py::test_conv_data_gradient."""
    def build():
        import torch.nn as nn
        from sgm.modules.diffusionmodules.util import conv_tokens
        g = torch.Generator().manual_seed(cin + cout)
        conv = nn.Conv2d(cin, cout, 3, stride=stride, padding=1)
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / (cin * 9) ** 0.5)
        conv.requires_grad_(False)
        conv = conv.to(DEV, BF)
        d = dict(x=R(N, H * W, cin, seed=1), dy=R(N, (H // stride) * (W // stride), cout, seed=2))

        def fn(x, dy):
            if not backward:
                return conv_tokens(conv, x, N, H, W)
            xd = x.detach().clone().requires_grad_(True)
            y = conv_tokens(conv, xd, N, H, W)
            y.backward(dy)
            return y.detach(), xd.grad
        return fn, d
    return build


add("conv-module-padded-4-to-320", conv_module_case(2, 16, 16, 4, 320, 1, False), ["cd360_conv_igemm_bf16"])
add("conv-module-padded-320-to-4", conv_module_case(2, 16, 16, 320, 4, 1, False), ["cd360_conv_igemm_bf16"])
for N, H, Wd, cin, cout, stride in ((2, 16, 16, 64, 64, 1), (3, 32, 32, 320, 320, 2), (2, 16, 16, 320, 4, 1)):
    add(f"conv-data-gradient-{N}x{H}x{Wd}x{cin}x{cout}-s{stride}", conv_module_case(N, H, Wd, cin, cout, stride, True), ["cd360_conv_igemm_bf16"],
        grad=True)
add("conv-data-gradient-2x16x8x1920x128-s1", conv_module_case(2, 16, 8, 1920, 128, 1, True), ["cd360_conv_igemm_bf16"], grad=True)  # Cout' = 1920


def conv_up2x_case(N, H, W, Cin, Cout):
    def build():
        ops = _ops()
        w = R(Cout, Cin, 3, 3, seed=1, scale=(9 * Cin) ** -0.5, dtype=torch.float32)
        d = dict(x=R(N, H * W, Cin, seed=2), wp=ops.pack_upsample_conv_weight(w), bias=R(Cout, seed=3, dtype=torch.float32))
        return (lambda x, wp, bias: ops.conv_up2x(x, wp, bias, N, H, W)), d
    return build


add("conv-up2x-ragged-1x5x7x128x320", conv_up2x_case(1, 5, 7, 128, 320), ["cd360_conv_up2x_bf16"])
add("conv-up2x-ragged-2x16x12x192x80", conv_up2x_case(2, 16, 12, 192, 80), ["cd360_conv_up2x_bf16"])
add("conv-up2x-3x32x32x1280x1280", conv_up2x_case(3, 32, 32, 1280, 1280), ["cd360_conv_up2x_bf16"])
for cfg in range(1, 7):
    add(f"conv-up2x-cfg{cfg}-2x8x8x64x320", conv_up2x_case(2, 8, 8, 64, 320), ["cd360_conv_up2x_bf16"], tuning=dict(conv_cfg=cfg))


def out_conv4_case(N, H, W, Cin):
    def build():
        ops = _ops()
        d = dict(x=R(N, H * W, Cin, seed=1), w36=ops.pack_out_conv4_weight(R(4, Cin, 3, 3, seed=2, scale=0.05)), bias=R(4, seed=3, dtype=torch.float32))
        return (lambda x, w36, bias: ops.out_conv4(x, w36, bias, N, H, W)), d
    return build


add("out-conv4-ragged-2x6x32x192", out_conv4_case(2, 6, 32, 192), ["cd360_out_conv4_bf16"])
add("out-conv4-3x128x128x320", out_conv4_case(3, 128, 128, 320), ["cd360_out_conv4_bf16"])


# ---- the first stage's own entry points (tests/conv_shapes.py VAE_*: one decoder and one encoder shape, downscaled from 1024^2)
def vae_case(which, *a):
    def build():
        ops = _ops()
        if which == "conv_in":
            B, cz, H, Wd, cout, stats = a
            w = ops.pack_vae_conv_in_weight(R(cout, cz, 3, 3, seed=1, scale=0.2, dtype=torch.float32))
            return (lambda z, w, bias: ops.vae_conv_in(z, w, bias, want_stats=stats)), dict(z=R(B, cz, H, Wd, seed=2, dtype=torch.float32), w=w,
                                                                                          bias=R(cout, seed=3, dtype=torch.float32))
        if which in ("conv_out", "enc_conv_out"):
            N, H, Wd, cin, cout = a
            pack, run = ((ops.pack_vae_conv_out_weight, ops.vae_conv_out) if which == "conv_out" else (ops.pack_vae_enc_conv_out_weight, ops.vae_enc_conv_out))
            w = pack(R(cout, cin, 3, 3, seed=1, scale=0.05, dtype=torch.float32))
            return (lambda x, w, bias: run(x, w, bias, N, H, Wd, cout)), dict(x=R(N, H * Wd, cin, seed=2), w=w, bias=R(cout, seed=3, dtype=torch.float32))
        N, H, Wd, c = a
        wp = ops.pack_conv_weight(R(c, c, 3, 3, seed=1, scale=(9 * c) ** -0.5, dtype=torch.float32))
        return (lambda x, wp, bias: ops.vae_downsample(x, wp, bias, N, H, Wd)), dict(x=R(N, H * Wd, c, seed=2), wp=wp, bias=R(c, seed=3, dtype=torch.float32))
    return build


add("vae-conv-in-decoder-1x4x128x128-512-stats", vae_case("conv_in", 1, 4, 128, 128, 512, True), ["cd360_vae_conv_in_f32"])
add("vae-conv-in-encoder-1x3x256x256-128-stats", vae_case("conv_in", 1, 3, 256, 256, 128, True), ["cd360_vae_conv_in_f32"])
add("vae-conv-in-ragged-2x4x17x23-512", vae_case("conv_in", 2, 4, 17, 23, 512, False), ["cd360_vae_conv_in_f32"])
add("vae-conv-out-1x256x256x128-3", vae_case("conv_out", 1, 256, 256, 128, 3), ["cd360_vae_conv_out_bf16"])
add("vae-conv-out-ragged-1x33x40x320-3", vae_case("conv_out", 1, 33, 40, 320, 3), ["cd360_vae_conv_out_bf16"])
add("vae-enc-conv-out-1x64x64x512-8", vae_case("enc_conv_out", 1, 64, 64, 512, 8), ["cd360_vae_enc_conv_out_bf16"])
add("vae-enc-conv-out-ragged-2x17x23x128-8", vae_case("enc_conv_out", 2, 17, 23, 128, 8), ["cd360_vae_enc_conv_out_bf16"])
add("vae-downsample-1x256x256x128", vae_case("downsample", 1, 256, 256, 128), ["cd360_vae_downsample_bf16"])
add("vae-downsample-1x64x64x512", vae_case("downsample", 1, 64, 64, 512), ["cd360_vae_downsample_bf16"])
add("vae-downsample-odd-2x17x23x128", vae_case("downsample", 2, 17, 23, 128), ["cd360_vae_downsample_bf16"])


# ================================================================================================ render
def render_inputs(C, r, n, S, b):
    from cd360 import nerf
    from test_kernels_gpu import cams_for, nerf_weights
    w = nerf_weights(C, seed=C + n)
    cams = cams_for(b, n, seed=C).to(DEV)
    xref = W.tensor("xref", (b, n, r * r, C), seed=C).to(DEV, BF)
    fw = nerf.FusedNerfWeights(*(w[k].to(DEV) for k in ("plane_coefs.0.weight", "plane_coefs.0.bias", "plane_coefs.2.weight", "plane_coefs.2.bias",
                                                        "nviews.weight", "nviews.bias", "decoder.weight")))
    xs = nerf.patch_positions(r, DEV)
    t, _ = nerf.depth_samples(S, 2.0, 0.0, DEV, r * r)
    Y, lv = nerf.reference_tables(fw, xref)
    return dict(cams=cams, xs=xs, t=t, Y=Y, zP=R(b * n, r * r, C, seed=C), lv=lv, cview=nerf.view_constants(fw, cams), Wk=fw.Wk)


def nerf_fwd_case(C, r, n, S, b, want_logits, direct):
    def build():
        ops = _ops()
        if not direct:
            return (lambda cams, xs, t, Y, zP, lv, cview, Wk: ops.nerf_mlp_aggregate(cams, xs, xs, t, Y, zP, lv, cview, Wk, want_logits=want_logits)), \
                render_inputs(C, r, n, S, b)

        @guardfn
        def fn(cams, xs, t, Y, zP, lv, cview, Wk, guard):  # cd360_nerf_mlp_aggregate: the one-pass entry (the binding calls the _ws form)
            T = guard.torch
            hw = r * r
            g = T.empty(b, hw * S, C, dtype=BF, device=DEV)
            logits = T.empty(b, n, hw * S, dtype=torch.float32, device=DEV) if want_logits else None
            lse = T.empty(b, hw * S, 2, dtype=torch.float32, device=DEV) if want_logits else None
            tc = t.contiguous()
            ops.check(guard.lib.cd360_nerf_mlp_aggregate(cams.data_ptr(), xs.data_ptr(), xs.data_ptr(), tc.data_ptr(), 0 if t.dim() == 1 else S,
                                                         Y.data_ptr(), zP.data_ptr(), lv.data_ptr(), cview.data_ptr(), Wk.data_ptr(), None, g.data_ptr(),
                                                         ops._ptr(logits), ops._ptr(lse), b, n, r, S, C, ops._stream()), "cd360_nerf_mlp_aggregate")
            return g, logits, lse
        return fn, render_inputs(C, r, n, S, b)
    return build


RENDER_SHAPES = ((64, 8, 2, 4, 2), (640, 16, 5, 24, 1), (1280, 8, 7, 6, 2), (128, 7, 3, 3, 1), (64, 8, 1, 4, 1))  # test_render_two_pass_equals_one_pass
HEADLINE = (1280, 32, 50, 24, 1)
for shape in RENDER_SHAPES + (HEADLINE,):
    s = "C{}-r{}-n{}-S{}-b{}".format(*shape)
    for logits in (False, True):
        lg = "logits" if logits else "nologits"
        for k in (0, 1):
            add(f"nerf-onepass-kernel{k}-{lg}-{s}", nerf_fwd_case(*shape, logits, True), ["cd360_nerf_mlp_aggregate"], tuning=dict(nerf_kernel=k))
        for k in (3, 4):
            add(f"nerf-twopass-kernel{k}-{lg}-{s}", nerf_fwd_case(*shape, logits, False), ["cd360_nerf_mlp_aggregate_ws"], tuning=dict(nerf_kernel=k))


def nerf_bwd_case(C, r, n, S, b, form):
    def build():
        ops = _ops()
        d = render_inputs(C, r, n, S, b)
        g, _, lse = ops.nerf_mlp_aggregate(d["cams"], d["xs"], d["xs"], d["t"], d["Y"], d["zP"], d["lv"], d["cview"], d["Wk"], want_logits=True)
        d.update(g=g, lse=lse, dg=R(*g.shape, seed=5))
        if form != "atomic":
            return (lambda cams, xs, t, Y, zP, lv, cview, Wk, g, lse, dg:
                    ops.nerf_mlp_aggregate_bwd(cams, xs, xs, t, Y, zP, lv, cview, Wk, None, g, lse, dg, scatter=form == "det-scatter")), d

        @guardfn
        def fn(cams, xs, t, Y, zP, lv, cview, Wk, g, lse, dg, guard):  # the fp32-atomic scatter form: caller-zeroed accumulators
            T = guard.torch
            hw, kp = r * r, ops.nerf_k_padded()
            dz, F = T.empty(b, n, hw * S, C, dtype=BF, device=DEV), T.empty(b, n, hw * S, kp, dtype=BF, device=DEV)
            dY, dlogit = T.zeros(Y.shape, dtype=torch.float32, device=DEV), T.zeros(b, n, hw * S, dtype=torch.float32, device=DEV)
            dlv, dcview = T.zeros(lv.shape, dtype=torch.float32, device=DEV), T.zeros(b, n, dtype=torch.float32, device=DEV)
            tc = t.contiguous()
            ops.check(guard.lib.cd360_nerf_mlp_aggregate_bwd(
                cams.data_ptr(), xs.data_ptr(), xs.data_ptr(), tc.data_ptr(), 0 if t.dim() == 1 else S, Y.data_ptr(), zP.data_ptr(), lv.data_ptr(),
                cview.data_ptr(), Wk.data_ptr(), None, g.data_ptr(), lse.data_ptr(), dg.data_ptr(), dz.data_ptr(), F.data_ptr(), dY.data_ptr(),
                dlogit.data_ptr(), dlv.data_ptr(), dcview.data_ptr(), b, n, r, S, C, ops._stream()), "cd360_nerf_mlp_aggregate_bwd")
            return dz, F, dY, dlogit, dlv, dcview
        return fn, d
    return build


for shape in ((64, 8, 2, 4, 2), (128, 7, 3, 3, 1), (640, 16, 5, 24, 1)):
    s = "C{}-r{}-n{}-S{}-b{}".format(*shape)
    add(f"nerf-bwd-det-scatter-{s}", nerf_bwd_case(*shape, "det-scatter"), ["cd360_nerf_mlp_aggregate_bwd_det"],
        valid=lambda res: res[:2] + res[5:])  # dY / dlv / dcview (res[2:5]) accumulate with fp32 atomics: finiteness is asserted below
    add(f"nerf-bwd-det-noscatter-{s}", nerf_bwd_case(*shape, "det-noscatter"), ["cd360_nerf_mlp_aggregate_bwd_det"])
    add(f"nerf-bwd-atomic-{s}", nerf_bwd_case(*shape, "atomic"), ["cd360_nerf_mlp_aggregate_bwd"], bit_equal=False)


def rays_case(b, n, r, S, per_ray_t):
    def build():
        from cd360 import nerf
        from test_kernels_gpu import cams_for
        ops = _ops()
        cams = cams_for(b, n, seed=21).to(DEV)
        xs = nerf.patch_positions(r, DEV)
        t, _ = nerf.depth_samples(S, 2.0, 0.0, DEV, r * r)
        if per_ray_t:
            t = (t.reshape(1, -1)[:, -S:] + 0.01 * torch.rand(r * r, S, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))).contiguous()

        def fn(cams, xs, t):
            return (ops.patch_rays(cams, xs, xs), ops.ray_project_index(cams, xs, xs, t), ops.plucker_features(cams, xs, xs),
                    ops.plucker_features_bf16(cams, xs, xs))
        return fn, dict(cams=cams, xs=xs, t=t)
    return build


RAY_ENTRIES = ["cd360_patch_rays", "cd360_ray_project_index", "cd360_plucker_features", "cd360_plucker_features_bf16"]
add("rays-project-plucker-b2-n3-r7-S3", rays_case(2, 3, 7, 3, False), RAY_ENTRIES)
add("rays-project-plucker-per-ray-t-b2-n2-r16-S24", rays_case(2, 2, 16, 24, True), RAY_ENTRIES)
add("rays-project-plucker-b1-n8-r64-S24", rays_case(1, 8, 64, 24, False), RAY_ENTRIES)


def gather_case(n_img, r, P, C, dtype):
    def build():
        grid = (torch.rand(n_img, P, 2, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)) * 2.6 - 1.3)
        return _ops().feature_gather, dict(xref=R(n_img, r * r, C, seed=1, dtype=dtype), grid=grid)
    return build


add("feature-gather-fp32-ragged-3x7x101x72", gather_case(3, 7, 101, 72, torch.float32), ["cd360_feature_gather"])
add("feature-gather-bf16-5x32x24576x1280", gather_case(5, 32, 24576, 1280, BF), ["cd360_feature_gather"])


def sample_pdf_case(rows, n_bins, n_samples, dists):
    def build():
        g = torch.Generator(device=DEV).manual_seed(rows)
        bins = torch.sort(torch.rand(rows, n_bins + 1, device=DEV, generator=g), -1).values
        d = dict(bins=bins, weights=torch.rand(rows, n_bins, device=DEV, generator=g), u=torch.rand(rows, n_samples, device=DEV, generator=g))
        return (lambda bins, weights, u: _ops().sample_pdf(bins, weights, u, want_dists=dists)), d
    return build


add("sample-pdf-ragged-333x8x20-dists", sample_pdf_case(333, 8, 20, True), ["cd360_sample_pdf"])
add("sample-pdf-1024x24x24", sample_pdf_case(1024, 24, 24, False), ["cd360_sample_pdf"])


def sample_pdf_inplace():
    g = torch.Generator(device=DEV).manual_seed(9)
    d = dict(bins=torch.sort(torch.rand(77, 33, device=DEV, generator=g), -1).values, weights=torch.rand(77, 32, device=DEV, generator=g),
             u=torch.rand(77, 32, device=DEV, generator=g))
    return (lambda bins, weights, u: _ops().sample_pdf(bins, weights, u, inplace=True)), d


add("sample-pdf-inplace-77x32x32", sample_pdf_inplace, ["cd360_sample_pdf"], inout=("u",))  # `samples` may alias u (include/cd360_hip.h: sample_pdf)


def nerf_pack_case(C):
    def build():
        from cd360 import nerf
        ops = _ops()
        cols = nerf.xyz_k_columns(C)
        NK = len(cols)
        kcol = torch.tensor(cols, dtype=torch.int32, device=DEV)
        kpos = torch.tensor([cols.index(c) if c in cols else -1 for c in range(C + 198)], dtype=torch.int32, device=DEV)
        d = dict(W1=R(C, C + 198, seed=1, scale=0.05), b1=R(C, seed=2), b2=R(C, seed=3), wv=R(C + 198, seed=4), bv=R(1, seed=5), Wd=R(4, C, seed=6),
                 kcol=kcol, kpos=kpos, gb=R(C * (C + NK + 128), seed=7), gf=R(7 * C + 104, seed=8, dtype=torch.float32))

        def fn(W1, b1, b2, wv, bv, Wd, kcol, kpos, gb, gf):
            wb, wf = ops.nerf_pack_weights(W1, b1, b2, wv, bv, Wd, kcol)
            nWf, nWk = C * C, C * NK
            grads = [gb[:nWf], gb[nWf:nWf + nWk], gb[nWf + nWk:], gf[:C], gf[C:2 * C], gf[2 * C:3 * C], gf[3 * C:3 * C + 99], gf[3 * C + 100:3 * C + 101],
                     gf[3 * C + 104:]]
            dW1, small = ops.nerf_unpack_grads(grads, kpos, C, NK)
            dW1b, smallb = ops.nerf_unpack_grads([None, grads[1], None, None, grads[4], None, grads[6], None, None], kpos, C, NK)
            return wb, wf, dW1, small, dW1b, smallb

        def valid(res):
            wb, wf, dW1, small, dW1b, smallb = res
            # include/cd360_hip.h (pack / unpack): out_f32 = b1 | b2 | vf | v_cam [99], 1 pad | bv, 3 pad | Wd;  small = db1 | db2 | dwv [C + 198] |
            # dbv, 1 pad | dWd -- the pad words are not specified
            f = [wf[:3 * C + 99], wf[3 * C + 100:3 * C + 101], wf[3 * C + 104:]]
            s = lambda t: [t[:3 * C + 199], t[3 * C + 200:]]
            return [wb, dW1, dW1b] + f + s(small) + s(smallb)
        fn.valid = valid
        return fn, d
    return build


for C in (64, 1280):
    add(f"nerf-pack-unpack-C{C}", nerf_pack_case(C), ["cd360_nerf_pack_weights_bf16", "cd360_nerf_unpack_grads_bf16"], valid="fn")


def volrender_case(b, hw, S, C, dtype, want_weights, rgb=True, per_ray=False):
    def build():
        ops = _ops()
        d = dict(feats=R(b, hw, S, C, seed=1, dtype=dtype), sigma=R(b, hw, S, seed=2, dtype=torch.float32),
                 dists=(R(hw, S, seed=3, dtype=torch.float32).abs() + 0.01) if per_ray else (R(S, seed=3, dtype=torch.float32).abs() + 0.01),
                 rgb_raw=R(b, hw, S, 3, seed=4, dtype=torch.float32) if rgb else None,
                 d_r=R(b, hw, C, seed=5, dtype=dtype), d_fg=R(b, hw, seed=6, dtype=torch.float32), d_a=R(b, hw, S, seed=7, dtype=torch.float32),
                 d_w=R(b, hw, S, seed=8, dtype=torch.float32), d_rgb=R(b, hw, 3, seed=9, dtype=torch.float32) if rgb else None)

        def fn(feats, sigma, dists, rgb_raw, d_r, d_fg, d_a, d_w, d_rgb):
            fwd = ops.volrender(feats, sigma, dists, rgb_raw, want_weights=want_weights)
            bwd = ops.volrender_bwd(feats, sigma, dists, rgb_raw, d_r, d_fg, d_a, d_w if want_weights else None, d_rgb)
            return fwd, bwd
        return fn, d
    return build


VOL = ["cd360_volrender", "cd360_volrender_bwd"]
add("volrender-fp32-weights-ragged-2x49x3x72", volrender_case(2, 49, 3, 72, torch.float32, True), VOL)
add("volrender-bf16-ragged-1x63x6x640-norgb", volrender_case(1, 63, 6, 640, BF, False, rgb=False, per_ray=True), VOL)
add("volrender-bf16-weights-1x1024x24x1280", volrender_case(1, 1024, 24, 1280, BF, True), VOL)
add("volrender-fp32-3x1024x24x320", volrender_case(3, 1024, 24, 320, torch.float32, False, per_ray=True), VOL)


def render_loss_case(b, r, S, rgb):
    def build():
        ops = _ops()
        hw = r * r
        u = lambda *s, seed: torch.rand(*s, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
        d = dict(fg=u(b, hw, 1, seed=1) * 1.2 - 0.1, alphas=u(b, hw, S, 1, seed=2), rgb=u(b, hw, 3, seed=3) if rgb else None, op=u(b, hw, seed=4),
                 bgw=u(b, hw, seed=5), mask_=(u(b, 1, r, r, seed=6) > 0.5).float(), want=u(b, 3, r, r, seed=7), den=u(b, seed=8) * hw + 1e-6,
                 g=R(b, 3, seed=9, dtype=torch.float32))

        def fn(fg, alphas, rgb, op, bgw, mask_, want, den, g):
            return ops.render_loss(fg, alphas, rgb, op, bgw, mask_, want, den), ops.render_loss_bwd(fg, alphas, rgb, op, bgw, mask_, want, den, g)
        return fn, d
    return build


RL = ["cd360_render_loss_f32", "cd360_render_loss_bwd_f32"]
add("render-loss-ragged-b3-r7-S3", render_loss_case(3, 7, 3, True), RL)
add("render-loss-norgb-b1-r9-S5", render_loss_case(1, 9, 5, False), RL)
add("render-loss-b2-r32-S24", render_loss_case(2, 32, 24, True), RL)


# ================================================================================================ normalisation and elementwise
def gn_case(N, P, C, silu, stats=False):
    def build():
        ops = _ops()
        groups = 32
        d = dict(x=R(N, P, C, seed=C), dy=R(N, P, C, seed=C + 1), gamma=R(C, seed=2, dtype=torch.float32), beta=R(C, seed=3, dtype=torch.float32))

        def fn(x, dy, gamma, beta):
            return ops.gn_silu(x, gamma, beta, groups, 1e-5, silu), ops.gn_silu_bwd(x, dy, gamma, beta, groups, 1e-5, silu)
        return fn, d
    return build


for N, P, C, silu in ((2, 64, 64, True), (3, 1024, 320, True), (1, 4096, 640, False), (2, 256, 2560, True), (1, 100, 960, False)):  # test_gn_silu
    add(f"gn-silu-{N}x{P}x{C}", gn_case(N, P, C, silu), ["cd360_gn_silu_bf16", "cd360_gn_silu_bwd_bf16"])


def gn_with_conv_stats():
    """gn_silu fed the convolution epilogue's slab statistics (the statistics read pass over x is skipped)."""
    ops = _ops()
    N, H, Wd, Cin, Cout = 3, 32, 32, 320, 640
    d = conv_inputs(N, H, Wd, Cin, Cout, True)
    d.update(gamma=R(Cout, seed=8, dtype=torch.float32), beta=R(Cout, seed=9, dtype=torch.float32))

    def fn(x, wp, bias, emb, res, gamma, beta):
        out, st = ops.conv_igemm(x, wp, bias, N, H, Wd, 9, emb, res, want_stats=True)
        return out, st, ops.gn_silu(out, gamma, beta, 32, 1e-5, True, tile_stats=st)
    return fn, d


add("gn-silu-on-conv-statistics-3x32x32x320x640", gn_with_conv_stats, ["cd360_conv_igemm_bf16", "cd360_gn_silu_bf16"])


def ln_case(rows, C):
    def build():
        ops = _ops()
        d = dict(a=R(rows, C, seed=1), b=R(rows, C, seed=2), gamma=R(C, seed=3), beta=R(C, seed=4), d_ln=R(rows, C, seed=5), d_sum=R(rows, C, seed=6))

        def fn(a, b, gamma, beta, d_ln, d_sum):
            s, ln = ops.add_layernorm(a, b, gamma, beta, 1e-5)
            _, ln1 = ops.add_layernorm(a, None, gamma, beta, 1e-5)
            return s, ln, ln1, ops.add_layernorm_bwd(s, gamma, d_ln, d_sum, 1e-5), ops.add_layernorm_bwd(a, gamma, d_ln, None, 1e-5)
        return fn, d
    return build


for rows, C in ((5, 2048), (37, 64), (513, 1280), (12288, 640)):
    add(f"add-layernorm-{rows}x{C}", ln_case(rows, C), ["cd360_add_layernorm_bf16", "cd360_add_layernorm_bwd_bf16"])


def geglu_case(rows, inner):
    def build():
        ops = _ops()
        return (lambda proj, dy: (ops.geglu(proj), ops.geglu_bwd(proj, dy))), dict(proj=R(rows, 2 * inner, seed=1), dy=R(rows, inner, seed=2))
    return build


add("geglu-ragged-37x72", geglu_case(37, 72), ["cd360_geglu_bf16", "cd360_geglu_bwd_bf16"])
add("geglu-3072x5120", geglu_case(3072, 5120), ["cd360_geglu_bf16", "cd360_geglu_bwd_bf16"])


def concat_case(N, H, Wd, ca, cb):
    def build():
        ops = _ops()
        cl = lambda c, seed: R(N, H, Wd, c, seed=seed).permute(0, 3, 1, 2)
        d = dict(a=cl(ca, 1), b=cl(cb, 2), sa=R(N, 4, ca, 2, seed=3, dtype=torch.float32), sb=R(N, 4, cb, 2, seed=4, dtype=torch.float32))
        return (lambda a, b, sa, sb: (ops.concat_channels(a, b), ops.concat_gn_stats(sa, sb))), d
    return build


add("concat-channels-ragged-2x5x7x72x8", concat_case(2, 5, 7, 72, 8), ["cd360_concat_channels_bf16"])
add("concat-channels-3x32x32x1280x640", concat_case(3, 32, 32, 1280, 640), ["cd360_concat_channels_bf16"])


def rowdot_case(rows, C):
    def build():
        ops = _ops()
        d = dict(h=R(rows, C, seed=1), w4=R(4, C, seed=2, dtype=torch.float32), w1=R(C, seed=3, dtype=torch.float32), d4=R(rows, 4, seed=4, dtype=torch.float32))

        def fn(h, w4, w1, d4):
            return (ops.rowdot4(h, w4), ops.rowdot1(h, w1), ops.rowdot4_bwd(d4, h, w4), ops.rowdot4_bwd(d4, h, w4, need_dw=False),
                    ops.rowdot4_bwd(d4, h, w4, need_dh=False))
        return fn, d
    return build


for rows, C in ((257, 520), (111, 2048), (24576, 1280)):
    add(f"rowdot-{rows}x{C}", rowdot_case(rows, C), ["cd360_rowdot4_bf16", "cd360_rowdot1_bf16", "cd360_rowdot4_bwd_bf16"])


def dropout_case(M, N, ld):
    def build():
        dyf = R(M, ld, seed=1)
        d = dict(dy=dyf[:, :N], dy_full=dyf, key=torch.tensor([99, 7], dtype=torch.int64, device=DEV))
        return (lambda dy, dy_full, key: _ops().dropout_apply(dy, 0.1, 5, key=key)), d
    return build


add("dropout-apply-ragged-333x72", dropout_case(333, 72, 72), ["cd360_dropout_apply_bf16"])
add("dropout-apply-strided-3072x1280", dropout_case(3072, 1280, 3840), ["cd360_dropout_apply_bf16"])


def euler_case(bs, H, Wd):
    def build():
        ops = _ops()
        d = dict(x=R(bs, 4, H, Wd, seed=1, dtype=torch.float32), eps=R(3 * bs, 4, H, Wd, seed=2, dtype=torch.float32),
                 s0=torch.tensor([1.7], device=DEV), s1=torch.tensor([1.1], device=DEV))
        return (lambda x, eps, s0, s1: ops.cfg_euler_step(x, eps, s0, s1, 7.5, 3.5)), d
    return build


add("cfg-euler-step-f32-ragged-1x4x5x7", euler_case(1, 5, 7), ["cd360_cfg_euler_step_f32"])
add("cfg-euler-step-f32-2x4x128x128", euler_case(2, 128, 128), ["cd360_cfg_euler_step_f32"])


def stage_case(bs, rep, H, Wd, cout, E):
    """The two ends of a sampling step (tests/test_f_rows_gpu.py): cd360_unet_stage_in writes h / emb_act, cd360_cfg_euler_step_cl updates x in place."""
    def build():
        ops = _ops()
        nsteps = 5
        d = dict(x=R(bs, 4, H, Wd, seed=1, dtype=torch.float32), tab=R(nsteps, 4, seed=2, dtype=torch.float32).abs() + 0.5,
                 step=torch.tensor([3], dtype=torch.int32, device=DEV), w=R(36, cout, seed=3, scale=0.2, dtype=torch.float32),
                 bias=R(cout, seed=4, dtype=torch.float32), temb=R(nsteps, E, seed=5), lab=R(rep * bs, E, seed=6), eps16=R(3 * bs, H * Wd, 16, seed=7))

        @guardfn
        def fn(x, tab, step, w, bias, temb, lab, eps16, guard):
            h = guard.torch.empty(rep * bs, H * Wd, cout, dtype=BF, device=DEV)
            act = guard.torch.empty_like(lab)
            ops.unet_stage_in(x, tab, step, w, bias, temb, lab, h, act)
            ops.cfg_euler_step_cl(x, eps16[..., :4], tab, step, 7.5, 3.5)
            return h, act
        return fn, d
    return build


STAGE = ["cd360_unet_stage_in", "cd360_cfg_euler_step_cl"]
add("unet-stage-in-and-euler-cl-ragged-2x3x24x40", stage_case(2, 3, 24, 40, 320, 1280), STAGE, inout=("x",))  # cd360_cfg_euler_step_cl: x IN PLACE
add("unet-stage-in-and-euler-cl-1x3x128x128", stage_case(1, 3, 128, 128, 320, 1280), STAGE, inout=("x",))


def adamw_case(sizes):
    def build():
        ops = _ops()
        begin, off = [], 0
        for s in sizes:
            begin.append(off)
            off += (s + 7) // 8 * 8
        d = {f"p{i}": R(s, seed=i) for i, s in enumerate(sizes)}
        d.update({f"g{i}": R(s, seed=100 + i, scale=0.01) for i, s in enumerate(sizes)})
        master = torch.zeros(off, dtype=torch.float32, device=DEV)
        for i, s in enumerate(sizes):
            master[begin[i]:begin[i] + s] = d[f"p{i}"].float()
        d.update(master=master, m=torch.zeros_like(master), v=torch.zeros_like(master), step=torch.zeros(1, dtype=torch.float32, device=DEV))

        def fn(master, m, v, step, **t):
            k = len(sizes)
            plan = ops.AdamwPlan([t[f"p{i}"] for i in range(k)], begin, [1e-3] * k, [0.01] * k)
            ops.adamw_step(plan, [t[f"g{i}"] for i in range(k)], master, m, v, step, 0.9, 0.999, 1e-8)
        return fn, d
    return build


def dropout_tick_case():
    """cd360_dropout_tick adds 1 to the offset of the (seed, offset) pair in device memory; the mask drawn after the tick must follow it."""
    ops = _ops()
    st = ops.dropout_state(torch.device(DEV))
    d = dict(state=st, dy=R(333, 72, seed=1))

    saved = st.clone()

    def fn(state, dy):
        ops.dropout_tick(state.device)
        return ops.dropout_apply(dy, 0.1, 5)
    fn.cleanup = lambda: st.copy_(saved)  # the process-wide mask state is other tests' too: leave it as it was found
    return fn, d


# AdamW's parameters, master weights, moments and the tick's step count are the header's in/out arguments
ADAMW = ["cd360_adamw_tick", "cd360_adamw_bf16"]
add("adamw-odd-sizes-1001-185-4096-3", adamw_case((1001, 185, 4096, 3)), ADAMW, inout=("p0", "p1", "p2", "p3", "master", "m", "v", "step"))
add("adamw-1638400", adamw_case((1280 * 1280,)), ADAMW, inout=("p0", "master", "m", "v", "step"))
add("dropout-tick-then-mask", dropout_tick_case, ["cd360_dropout_tick", "cd360_dropout_apply_bf16"], inout=("state",))  # the tick's rng state: in/out


# ================================================================================================ the tests
BY_NAME = {c.name: c for c in CASES}


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_guarded(name, tune):
    c = BY_NAME[name]
    with torch.no_grad():
        fn, inputs = c.build()
    if c.tuning:
        tune(**c.tuning)
    valid = getattr(fn, "valid", None) if c.valid == "fn" else c.valid
    try:
        with torch.set_grad_enabled(c.grad):
            r1, _ = G.run_twice(fn, inputs, declares=c.declares, inout=c.inout, valid=valid, bit_equal=c.bit_equal)
    finally:
        getattr(fn, "cleanup", lambda: None)()
    for path, t in G._flatten(r1):  # whatever P2's valid region or bit_equal=False left out is still finite where it is floating point
        if c.valid != "fn" and t.is_floating_point():  # ("fn": the header's unspecified pad words are not looked at)
            assert bool(torch.isfinite(t).all()), path


# Functions of include/cd360_hip.h that launch nothing (host-only): size queries, route / shape queries, tuning, and the prefetcher's arm / disarm
# (they only register streams; the touch kernel the armed launches enqueue has tests/test_prefetch_gpu.py).  cd360_adamw_tick and cd360_dropout_tick
# launch a one-thread kernel each and are therefore NOT here: they have cases above.
SIZE_QUERIES = {"cd360_attn_single_workspace_bytes", "cd360_gn_workspace_bytes", "cd360_gn_bwd_workspace_bytes", "cd360_gemm_tn_workspace_bytes",
                "cd360_nerf_ws_bytes", "cd360_kv_fp8_bytes", "cd360_conv_dma_slab_rows", "cd360_conv_stats_rows", "cd360_vae_downsample_stats_rows",
                "cd360_conv_stats_slabs", "cd360_vae_conv_in_stats_slabs", "cd360_gemm_cstats_rows", "cd360_rowdot4_bwd_slabs"}
LAUNCH_NOTHING = SIZE_QUERIES | {
    "cd360_gemm_tile_n", "cd360_conv_route", "cd360_conv3x3_dma_route", "cd360_conv_up2x_route", "cd360_conv_k_order", "cd360_nerf_k_padded",
    "cd360_attn_single_splits",
    "cd360_set_tuning", "cd360_get_tuning", "cd360_set_stream_tuning", "cd360_get_stream_tuning", "cd360_query_stream", "cd360_whatif_build",
    "cd360_prefetch_arm_on", "cd360_prefetch_disarm_on", "cd360_prefetch_arm", "cd360_prefetch_disarm"}


def exported_names():
    """The functions include/cd360_hip.h DECLARES (comments stripped; `return type name(`), not every cd360_ word in it."""
    src = open(os.path.join(ROOT, "include", "cd360_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return set(re.findall(r"\b(?:int|int64_t)\s+(cd360_\w+)\s*\(", src))


def test_every_launching_entry_point_has_a_case():
    """Runs without a GPU: the coverage condition is a property of the case table.  P4 proves at run time that a case reached what it declares."""
    from cd360 import _lib
    names = exported_names()
    assert names == set(_lib.SIGNATURES), names ^ set(_lib.SIGNATURES)  # declarations, not words: no cd360_hip, no cd360_qproj_attn
    assert LAUNCH_NOTHING <= names
    declared = {e for c in CASES for e in c.declares}
    assert declared <= names - LAUNCH_NOTHING, declared - (names - LAUNCH_NOTHING)
    missing = names - LAUNCH_NOTHING - declared
    print(f"\n{len(declared)} launching entry points under guards in {len(CASES)} cases; {len(LAUNCH_NOTHING)} host-only functions subtracted")
    assert not missing, f"launching entry points without a guarded case: {sorted(missing)}"
