"""Every attention kernel that streams its keys in tiles, on inputs where float64 softmax attention is its exact answer up to the one bf16
rounding of the output (tests/attn_tile_cases.py: K, V integers in [-7, 7] times a power of two per batch and head, integer logits in
exp2 units through scale * log2(e) = 1.0f, so every p and every alpha of a moving maximum is a power of two).  Needs an MI355X.

What runs, each under its own test id, B = 2 and H = 2 with q, k, v read in place from one merged [B, N + 8, 3 H 64] projection (Nq != Nk:
k | v merged, q inside a 3 C wide row; 8 attractive padding rows behind the real keys), both families (mix: band / stair-up / stair-down
/ half rows interleaved; onehot) per id, and cd360_attn_fwd_lse_bf16 again under the same tuning on every forward case:
  attn_fwd_kernel               attn_self = 0 x attn_fast = 1, 0 x (Nq, Nk) = (200, 97), (200, 200), (333, 333), (256, 256)
  attn_self_kernel<1, 4>        attn_self = 1, N = 256 (the ring filled once), 640 (the ring wraps, five query tiles)
  attn_self_kernel<1, 8>        attn_self = 3, N = 256, 768
  attn_self_kernel<2, 8>        attn_self = 2, N = 512, 1024
  cd360_attn_fwd_prescaled_bf16 attn_self unset: N = 256, 512 (by shape: <1, 4>), N = 200 (first generation)
  cd360_attn_fwd_xformers_bf16  BH = 4, N = 200
  cd360_attn_single_bf16        (b, n, D) = (2, 256, 512) one split, (1, 520, 320) two, (1, 1024, 128) four, (1, 600, 512) two; the split
                                count held against cd360_attn_single_splits; qscale = 0.5 with q doubled; ops.memory_efficient_attention
  cd360_attn_bwd_bf16           the bwd one-hot family at (Nq, Nk) = (200, 200), (256, 256), (200, 97): dQ + dK/dV roles, need_dq = False
                                (the stand-alone delta kernel), and writing into the slices of one d(q|k|v) buffer
Each case first asserts, from the dispatch conditions restated in attn_tile_cases.route, that it reaches the kernel it is named for.

Bar, per element, 100 % of every output: |got - ref| <= 2^-8 |ref| + 2^-10 A, A = the softmax-weighted mean of |v| (2^-9 is the bf16
rounding of the output; the rest covers 1 / l, the fp32 sums of the rows that are not band rows, and for the single-head kernel the
per-split normalisation, log2f(l) and the combine).  One-hot rows equal bf16(v_winner) bit for bit.  lse: |got - ref| <= LSE_REL
(|ref| + 1) with LSE_REL = 7.2e-7, 4 x the worst error of the fp32 restatement (m c + log2f(l)) ln 2 (1.77e-7, tests/test_attn_tile_cpu.py).
Backward: dV equals the bf16 sum of the dO rows each key wins bit for bit, rows of dK / dV at or beyond Nk stay zero, dQ and dK within
the same bar with A the weighted mean of the magnitudes of their own products (attn_tile_cases.RefBwd).  tests/test_attn_tile_cpu.py holds
fp32 emulations of the three forward pipelines and of the backward to a tenth of the bar in front of the output rounding and shows
that each fault model breaks it.  Each test prints ATTN-TILE <route> <case> worst=<err / bar> before it asserts.

Measured on an MI355X, worst err / bar over the cases of a route, mix family (the one-hot family is bit-exact on every route: ratio 0), and
the worst lse error / lse bar of the route's cd360_attn_fwd_lse_bf16 runs:
  attn_fwd_kernel, attn_fast = 1 (4 shapes)   0.767   lse 0.188      attn_fwd_kernel, attn_fast = 0 (4 shapes)   0.767   lse 0.188
  attn_self_kernel<1, 4>, N = 256, 640        0.692   lse 0.207      attn_self_kernel<1, 8>, N = 256, 768        0.694   lse 0.382
  attn_self_kernel<2, 8>, N = 512, 1024       0.715   lse 0.464      prescaled entry, N = 256, 512 / N = 200     0.701 / 0.767
  xformers entry, BH = 4, N = 200             0.767   lse 0.154      cd360_attn_single_bf16, 1 / 2 / 4 splits    0.764 / 0.782 / 0.699
  cd360_attn_single_bf16, qscale = 0.5        0.782 (bit-equal to qscale = 1)       ops.memory_efficient_attention at head dim 512: bit-exact
  cd360_attn_bwd_bf16, three shapes x three forms: dQ, dK 5.1e-7 of the bar (float64 dQ, dK themselves: ~2^-30 of their products' size), dV
  bit-equal to the per-key sums of dO, rows at and beyond Nk zero, dK / dV of the need_dq = False form bit-equal to the full form's
(every figure is the output's own bf16 rounding, at most 2^-9 / (2^-8 + 2^-10) = 0.797; the fp32 emulations of tests/test_attn_tile_cpu.py
give the same figures to three digits, 8e-4 of the bar at most in front of the output rounding.  The lse bar is 7.2e-7 (|lse| + 1): the
device's worst is 0.464 of it, 3.3e-7 (|lse| + 1).)

What these cases found: nothing to fix.  Every tiled forward kernel in every tiling and under both entries, the single-head kernel with
its combine, and both roles of the backward with the stand-alone delta kernel pass at the bar as first stated, bit for bit where that
is asked.  Two things the code says that the cases had to follow: TileMax's halves are not the lower and upper 32 keys of a tile
but the keys held by lanes 0-31 and 32-63 of the S^T accumulator (key % 8 < 4 and >= 4), so the stair alternates over both splits of the
tile; and the ragged tile of attn_fwd_kernel is masked twice (tile_load zero-fills keys >= Nk, consume_tile sets their scores to
-inf), so an unmasked padding key would arrive as zeros -- the rows with every logit below zero -- while the attractive rows behind Nk
guard against a kernel that reads them."""
import ctypes
import functools

import pytest
import torch

import attn_tile_cases as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
_I64x3 = ctypes.c_int64 * 3
_I64x2 = ctypes.c_int64 * 2


def _lib():
    from cd360 import _lib
    return _lib.load()


def _ok(code, what):
    from cd360 import _lib
    _lib.check(code, what)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def s3(t):
    return _I64x3(t.stride(0), 64, t.stride(1))


def aligned(o):
    return o.data_ptr() % 16 == 0 and o.stride(0) % 8 == 0 and o.stride(1) % 8 == 0


@functools.lru_cache(maxsize=2)
def device_qkv(sp):
    """q, k, v as column slices of the merged projection: [B, N + 8, 3 C] for self-attention (the rows >= N hold the padding keys); for
    Nq != Nk k | v of [B, Nk + 8, 2 C] and q the middle third of a [B, Nq, 3 C] row.  Whatever is not q, k or v is 5."""
    case = T.make_case(sp)
    C = sp.H * sp.D
    kf, vf = case.k.reshape(sp.B, case.rows, C), case.v.reshape(sp.B, case.rows, C)
    qf = case.q.reshape(sp.B, sp.Nq, C)
    if sp.Nq == sp.Nk:
        m = torch.full((sp.B, case.rows, 3 * C), 5.0, dtype=torch.float64)
        m[:, :sp.Nq, :C], m[..., C:2 * C], m[..., 2 * C:] = qf, kf, vf
        m = m.to(DEV, BF)
        return m[:, :sp.Nq, :C], m[..., C:2 * C], m[..., 2 * C:]
    wide = torch.full((sp.B, sp.Nq, 3 * C), 5.0, dtype=torch.float64)
    wide[..., C:2 * C] = qf
    wide, kv = wide.to(DEV, BF), torch.cat([kf, vf], -1).to(DEV, BF)
    return wide[..., C:2 * C], kv[..., :C], kv[..., C:]


def check(route, case, got, lse=None):
    ref = T.reference(case)
    got = got.float().cpu()
    worst = T.worst_ratio(got, ref)
    exact = None
    if case.spec.family == "onehot":
        exact = bool(torch.equal(got.bfloat16(), T.onehot_target(case).bfloat16()))
    lr = None if lse is None else T.lse_ratio(lse.float().cpu(), ref)
    print(f"ATTN-TILE {route} {T.spec_id(case.spec)} worst={worst:.3e}/1 winner_rows_bit_exact={exact}" + ("" if lr is None else f" lse={lr:.3e}/1"))
    assert worst <= 1.0
    assert exact is not False
    assert lr is None or lr <= 1.0


def forward(entry, sp, q, k, v, want_lse=False):
    """One of the tiled forward entries through the C ABI with explicit strides; softmax scale T.SCALE.  -> (o, lse | None)"""
    out = torch.full((sp.B, sp.Nq, sp.H * 64), float("nan"), dtype=BF, device=DEV)
    lse = torch.full((sp.B * sp.H, sp.Nq), float("nan"), dtype=torch.float32, device=DEV) if want_lse else None
    args = (sp.B, sp.H, sp.Nq, sp.Nk, s3(q), s3(k), s3(v), s3(out))
    if want_lse:
        _ok(_lib().cd360_attn_fwd_lse_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), *args, T.SCALE, _stream()),
            "cd360_attn_fwd_lse_bf16")
    elif entry == "prescaled":
        _ok(_lib().cd360_attn_fwd_prescaled_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), *args, _stream()), "cd360_attn_fwd_prescaled_bf16")
    else:
        _ok(_lib().cd360_attn_fwd_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), *args, T.SCALE, _stream()), "cd360_attn_fwd_bf16")
    return out, lse


@pytest.mark.parametrize("name,entry,tuning,nq,nk,kernel", [pytest.param(*c, id=c[0]) for c in T.FORWARD])
def test_tiled_forward(name, entry, tuning, nq, nk, kernel, tune):
    """The entry under its tuning, then cd360_attn_fwd_lse_bf16 under the same tuning (o as before, and lse), both families."""
    if tuning:
        tune(**tuning)
    for family in T.FAMILIES:
        sp = T.tiled_spec(family, nq, nk)
        case = T.make_case(sp)
        q, k, v = device_qkv(sp)
        if entry == "xformers":   # q, k, v, o contiguous [BH, N, 64]; the keys of the next head, or 8 padding rows, follow each head's
            heads = lambda x, n: x[:, :n].reshape(sp.B, n, sp.H, 64).permute(0, 2, 1, 3).reshape(sp.B * sp.H, n, 64)
            xq = heads(q, nq).contiguous()
            xk, xv = (torch.cat([heads(x, nk).reshape(-1, 64), heads(x, nk + T.PAD)[-1, nk:]], 0).contiguous() for x in (k, v))
            out = torch.full((sp.B * sp.H, nq, 64), float("nan"), dtype=BF, device=DEV)
            assert T.route(entry, 1, sp.B * sp.H, nq, nk, aligned=aligned(out), k_row_stride=64, **tuning) == kernel
            _ok(_lib().cd360_attn_fwd_xformers_bf16(xq.data_ptr(), xk.data_ptr(), xv.data_ptr(), out.data_ptr(), sp.B * sp.H, nq, nk, T.SCALE, _stream()),
                "cd360_attn_fwd_xformers_bf16")
            merge = lambda x: x.reshape(sp.B, sp.H, nq, 64).permute(0, 2, 1, 3).reshape(sp.B, nq, sp.H * 64)
            check(f"{entry}:{kernel}", case, merge(out))
            out2 = torch.full_like(out, float("nan"))   # the lse entry on the same layout: one batch element of BH heads
            lse = torch.full((sp.B * sp.H, nq), float("nan"), dtype=torch.float32, device=DEV)
            qs, ks = _I64x3(0, nq * 64, 64), _I64x3(0, nk * 64, 64)
            _ok(_lib().cd360_attn_fwd_lse_bf16(xq.data_ptr(), xk.data_ptr(), xv.data_ptr(), out2.data_ptr(), lse.data_ptr(), 1, sp.B * sp.H, nq, nk,
                                               qs, ks, ks, qs, T.SCALE, _stream()), "cd360_attn_fwd_lse_bf16")
            check(f"lse:{kernel}", case, merge(out2), lse)
            continue
        probe = torch.empty((sp.B, nq, sp.H * 64), dtype=BF, device=DEV)
        got = T.route(entry, sp.B, sp.H, nq, nk, aligned=aligned(probe), k_row_stride=k.stride(1), **tuning)
        if tuning.get("attn_self", 0) > 0 and got != kernel:
            pytest.skip(f"{nq} x {nk} cannot take attn_self = {tuning['attn_self']}")
        assert got == kernel, (got, kernel)
        out, _ = forward(entry, sp, q, k, v)
        check(f"{entry}:{kernel}", case, out)
        lse_kernel = T.route("lse", sp.B, sp.H, nq, nk, aligned=aligned(probe), k_row_stride=k.stride(1), **tuning)
        out, lse = forward(entry, sp, q, k, v, want_lse=True)
        check(f"lse:{lse_kernel}", case, out, lse)


def single(sp, q, k, v, qscale=1.0):
    b, n, d = sp.B, sp.Nq, sp.D
    out = torch.full((b, n, d), float("nan"), dtype=BF, device=DEV)
    nbytes = _lib().cd360_attn_single_workspace_bytes(b, n, d)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
    st = lambda t: _I64x2(t.stride(0), t.stride(1))
    _ok(_lib().cd360_attn_single_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), b, n, d, st(q), st(k), st(v), st(out), qscale,
                                      ws.data_ptr() if nbytes else None, _stream()), "cd360_attn_single_bf16")
    return out


@pytest.mark.parametrize("b,n,d", T.SINGLE, ids=[f"b{b}-n{n}-d{d}" for b, n, d in T.SINGLE])
def test_single_head(b, n, d):
    """attn_single_kernel (+ attn_single_combine_kernel where the keys are split) with q, k, v the column slices of one merged buffer."""
    assert _lib().cd360_attn_single_splits(b, n) == T.SINGLE_SPLITS[n]
    for family in T.FAMILIES:
        sp = T.single_spec(family, b, n, d)
        case = T.make_case(sp)
        q, k, v = device_qkv(sp)
        check(f"single-splits{T.SINGLE_SPLITS[n]}", case, single(sp, q, k, v))
        if (b, n, d) == (1, 520, 320):
            check("single-qscale0.5", case, single(sp, (q * 2).contiguous(), k, v, qscale=0.5))


def test_single_head_through_memory_efficient_attention():
    """ops.memory_efficient_attention at head dim 512 (qscale = 512^-0.5 log2 e inside): the one-hot family, whose winner keeps a margin
    of >= 24 units under that factor, bit for bit."""
    from cd360 import ops
    sp = T.single_spec("onehot", 2, 256, 512)
    case = T.make_case(sp)
    s = T.reference(case).logits * (512 ** -0.5 * 1.4426950408889634)
    top2 = s.topk(2, -1).values
    assert float((top2[..., 0] - top2[..., 1]).min()) >= 24
    q, k, v = device_qkv(sp)
    out = ops.memory_efficient_attention(q.contiguous(), k[:, :sp.Nk].contiguous(), v[:, :sp.Nk].contiguous())
    exact = bool(torch.equal(out.cpu(), T.onehot_target(case).bfloat16()))
    print(f"ATTN-TILE single-ops {T.spec_id(sp)} winner_rows_bit_exact={exact}")
    assert exact


def backward(sp, q, k, v, o, do, lse, dq, dk, dv):
    ws = torch.full((sp.B * sp.H * sp.Nq,), float("nan"), dtype=torch.float32, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()
    st = lambda t: None if t is None else s3(t)
    _ok(_lib().cd360_attn_bwd_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), p(dq), p(dk), p(dv),
                                   ws.data_ptr(), sp.B, sp.H, sp.Nq, sp.Nk, s3(q), s3(k), s3(v), s3(o), s3(do), st(dq), st(dk), st(dv), T.SCALE,
                                   _stream()), "cd360_attn_bwd_bf16")


@pytest.mark.parametrize("nq,nk", T.BWD_SHAPES, ids=[f"{nq}x{nk}" for nq, nk in T.BWD_SHAPES])
def test_backward(nq, nk):
    """o and lse from cd360_attn_fwd_lse_bf16, then cd360_attn_bwd_bf16 three ways: dQ + dK/dV into tensors of their own; need_dq = False
    (the stand-alone delta kernel; dK, dV bit-equal to the first call's); into the slices of one d(q|k|v) (Nq != Nk: d(k|v)) buffer."""
    sp = T.bwd_spec(nq, nk)
    case = T.make_case(sp)
    g = T.reference_bwd(case)
    C = sp.H * 64
    q, k, v = device_qkv(sp)
    o, lse = forward("plain", sp, q, k, v, want_lse=True)
    assert torch.equal(o.cpu(), T.onehot_target(case).bfloat16())
    do = case.do.reshape(sp.B, nq, C).to(DEV, BF)
    rows = case.rows

    def fresh():   # NaN where the kernel has to write, zero in the rows at and beyond Nk
        d = torch.full((sp.B, rows, C), float("nan"), dtype=BF, device=DEV)
        d[:, nk:] = 0
        return d

    def verdict(route, dq, dk, dv):
        if dq is None:
            rq = 0.0
            _, rk, exact = T.bwd_ratios(g.dq, dk[:, :nk].float().cpu(), dv[:, :nk].float().cpu(), g)
        else:
            rq, rk, exact = T.bwd_ratios(dq.float().cpu(), dk[:, :nk].float().cpu(), dv[:, :nk].float().cpu(), g)
        tail = not bool(dk[:, nk:].any()) and not bool(dv[:, nk:].any())
        print(f"ATTN-TILE bwd-{route} {T.spec_id(sp)} worst={max(rq, rk):.3e}/1 dq={rq:.3e} dk={rk:.3e} dv_bit_exact={exact} rows_beyond_nk_zero={tail}")
        assert rq <= 1.0 and rk <= 1.0 and exact and tail

    dq = torch.full((sp.B, nq, C), float("nan"), dtype=BF, device=DEV)
    dk, dv = fresh(), fresh()
    backward(sp, q, k, v, o, do, lse, dq, dk, dv)
    verdict("dq+dkv", dq, dk, dv)
    dk2, dv2 = fresh(), fresh()
    backward(sp, q, k, v, o, do, lse, None, dk2, dv2)
    verdict("dkv-only", None, dk2, dv2)
    assert torch.equal(dk2[:, :nk].view(torch.int16), dk[:, :nk].view(torch.int16)) and torch.equal(dv2[:, :nk].view(torch.int16), dv[:, :nk].view(torch.int16))
    if nq == nk:
        m = torch.full((sp.B, rows, 3 * C), float("nan"), dtype=BF, device=DEV)
        m[:, nk:] = 0
        dq3, dk3, dv3 = m[:, :nq, :C], m[..., C:2 * C], m[..., 2 * C:]
    else:
        m = torch.full((sp.B, rows, 2 * C), float("nan"), dtype=BF, device=DEV)
        m[:, nk:] = 0
        dq3, dk3, dv3 = torch.full((sp.B, nq, C), float("nan"), dtype=BF, device=DEV), m[..., :C], m[..., C:]
    backward(sp, q, k, v, o, do, lse, dq3, dk3, dv3)
    verdict("slices", dq3, dk3, dv3)
