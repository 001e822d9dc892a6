"""Every attention kernel that rounds P (the backward: and dS) to bf16 in front of an MFMA, OFF the power-of-two grid: bf16 `randn` inputs
at the ordinary softmax scale 1 / 8, against float64 emulations that round where the kernel source rounds (tests/attn_round_cases.py,
which states the method, the flip allowance and how its constants were fixed; tests/test_attn_round_cpu.py checks it).  Needs an MI355X.

Three families per case -- spread (q gain 1), peaked (q gain 3), positive (peaked, v > 0 and dO > 0) -- and per output element, nothing
excluded:   |got - emu| <= 2^-8 |emu| + EPS A + F.   On the positive family also the signed bias T = mean((got - exact64) / A) against
float64 attention with no P rounding at all: |T| <= |T_trunc| / 4, T_trunc from the emulation with P truncated on the same inputs.
K and V rows at and beyond Nk are NaN.  What runs, each under its own test id:

  cd360_attn_fwd_bf16, Nk <= 96     B = 2, H = 2, Nq = 160, Nk = 24, 64, 77 (attn_smallk_kernel<1 .. 3>)
  cd360_attn_fwd_lse_bf16           again on every case of the three tiled routes above and below (smallk, attn_fwd_kernel, attn_self_kernel): o as
                                    before and lse within LSE_REL (|lse| + 1) of the emulation's -- where l summed from the rounded P would show
  cd360_qproj_attn_dedup_bf16       the signed selection of attn_grid_cases as the projection (q exact), N = K = 128, Nq = 256, Nk = 40, 77, 96 x
                                    qattn_cfg 1 .. 4 x qattn_keys16 0 / default x dup 0, 1
  attn_fwd_kernel                   Nq = 200, Nk = 97, 200, 333 x attn_fast 1, 0
  attn_self_kernel                  B H = 2, Nq = 512, Nk = 256: plain entry (q~ = bf16(fp32(q c)) formed in the kernel) and pre-scaled entry (q~
                                    handed over) x attn_self 1, 2, 3; the two entries bit-equal
  cd360_attn_single_bf16            N = 256, 512, 1024 at head dim 128 (1, 2, 4 splits), N = 512 at head dim 512; N = 512 again with qscale / 2
                                    against a doubled q, bit-equal
  cd360_attn_bwd_bf16               (Nq, Nk) = (128, 128), (200, 77), (256, 333), B = 1, H = 2: dQ + dK/dV, need_dq = False (the stand-alone delta
                                    kernel), and the merged d(q|k|v) buffer at 128 x 128; o (bf16) and lse (fp32) computed on the host in float64
Each case first asserts, from the dispatch restated in attn_tile_cases.route, that it reaches the kernel it is named for (the fused
projection and the single-head entry have one kernel each; the single-head split count is held against cd360_attn_single_splits).
Each test prints ATTN-ROUND <route> <case> worst=<err / bar> flagged=<share> T=<T>/<bar> before it asserts."""
import ctypes
import functools

import pytest
import torch

import attn_round_cases as RC
import attn_tile_cases as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")
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


@functools.lru_cache(maxsize=4)
def emulation(pipeline, sp):
    """(emulation, the lazy pipeline's alternative or None, T_trunc or None) of a forward case."""
    case = RC.make_case(sp)
    if pipeline == "lazy":
        emu, alt, _ = RC.lazy_pair(case)
    else:
        emu, alt = RC.PIPELINES[pipeline](case), None
    t_trunc = None
    if sp.family == "positive":
        ex = RC.exact(case)
        t_trunc = RC.bias(RC.PIPELINES[pipeline](case, "p_trunc").out(), RC.flat(ex.out), RC.flat(ex.A))
    return emu, alt, t_trunc


def check(route, pipeline, sp, got, lse=None):
    """got [B, Nq, H * D] from the device; lse [B * H, Nq] where the entry returns it."""
    case = RC.make_case(sp)
    ex = RC.exact(case)
    emu, alt, t_trunc = emulation(pipeline, sp)
    got = got.float().cpu().double()
    worst = float(RC.forward_ratios(got, emu, ex.A, alt).max())
    t = RC.bias(got, RC.flat(ex.out), RC.flat(ex.A))
    bar = "-" if t_trunc is None else f"{abs(t_trunc) / 4:.2e}"
    lr = None if lse is None else float(RC.lse_ratios(lse.float().cpu(), emu, alt).max())
    print(f"ATTN-ROUND {route} {RC.spec_id(sp)} worst={worst:.3f}/1 flagged={emu.flagged:.5f} T={t:.2e}/{bar}" + ("" if lr is None else f" lse={lr:.3f}/1"))
    assert worst <= 1.0
    assert lr is None or lr <= 1.0
    assert t_trunc is None or abs(t) <= abs(t_trunc) / 4


@functools.lru_cache(maxsize=4)
def device_qkv(sp):
    """q the middle third of a [B, Nq, 3 C] row, k | v the halves of one [B, Nk + 8, 2 C] buffer whose rows >= Nk are NaN."""
    case = RC.make_case(sp)
    C = sp.H * sp.D
    wide = torch.full((sp.B, sp.Nq, 3 * C), 5.0, dtype=torch.float64)
    wide[..., C:2 * C] = RC.flat(case.q)
    kv = torch.full((sp.B, sp.Nk + RC.PAD, 2 * C), NAN, dtype=torch.float64)
    kv[:, :sp.Nk, :C], kv[:, :sp.Nk, C:] = RC.flat(case.k), RC.flat(case.v)
    wide, kv = wide.to(DEV, BF), kv.to(DEV, BF)
    return wide[..., C:2 * C], kv[..., :C], kv[..., C:]


def forward(entry, sp, q, k, v):
    """-> o, or (o, lse) of cd360_attn_fwd_lse_bf16 for entry "lse"."""
    out = torch.full((sp.B, sp.Nq, sp.H * 64), NAN, dtype=BF, device=DEV)
    args = (sp.B, sp.H, sp.Nq, sp.Nk, s3(q), s3(k), s3(v), s3(out))
    if entry == "lse":
        lse = torch.full((sp.B * sp.H, sp.Nq), NAN, dtype=torch.float32, device=DEV)
        _ok(_lib().cd360_attn_fwd_lse_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), *args, RC.SCALE, _stream()),
            "cd360_attn_fwd_lse_bf16")
        return out, lse
    if entry == "prescaled":
        _ok(_lib().cd360_attn_fwd_prescaled_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), *args, _stream()), "cd360_attn_fwd_prescaled_bf16")
    else:
        _ok(_lib().cd360_attn_fwd_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), *args, RC.SCALE, _stream()), "cd360_attn_fwd_bf16")
    return out


def routed(entry, sp, k, **tuning):
    probe = torch.empty((sp.B, sp.Nq, sp.H * 64), dtype=BF, device=DEV)
    return T.route(entry, sp.B, sp.H, sp.Nq, sp.Nk, aligned=aligned(probe), k_row_stride=k.stride(1), **tuning)


@pytest.mark.parametrize("nk", RC.ROW_NK)
def test_small_key_attention(nk):
    """attn_smallk_kernel<NKB, false>, NKB = ceil(Nk / 32) = 1, 2, 3; Nq = 160: five 32-query blocks."""
    assert -(-nk // 32) == RC.ROW_NK.index(nk) + 1
    for family in RC.FAMILIES:
        sp = RC.row_spec(family, nk)
        q, k, v = device_qkv(sp)
        assert routed("plain", sp, k) == "smallk"
        check(f"smallk<{-(-nk // 32)}>", "row", sp, forward("plain", sp, q, k, v))
        assert routed("lse", sp, k) == "smallk"
        check(f"lse:smallk<{-(-nk // 32)}>", "row", sp, *forward("lse", sp, q, k, v))


QPROJ = [pytest.param(nk, dup, cfg, keys16, id=f"nk{nk}-dup{dup}-qcfg{cfg}-keys16{'off' if keys16 == 0 else 'default'}")
         for nk in RC.QPROJ_NK for dup in (0, 1) for cfg in (1, 2, 3, 4) for keys16 in (0, None)]


@functools.lru_cache(maxsize=4)
def qproj_inputs(sp):
    """a [B - dup, Nq, K] with a W^T = q exactly, W [N, K], k | v as one [B, Nk + 8, 2 N] buffer with NaN rows behind the keys."""
    case = RC.make_case(sp)
    w, pi, sigma = RC.selection()
    g = torch.Generator().manual_seed(sp.Nk)
    a = RC.bf(torch.randn(sp.B - sp.dup, sp.Nq, RC.QPROJ_K, generator=g)).double()
    a[..., pi] = RC.flat(case.q)[:sp.B - sp.dup] * sigma
    assert torch.equal(a @ w.T, RC.flat(case.q)[:sp.B - sp.dup])
    N = RC.QPROJ_N
    kv = torch.full((sp.B, sp.Nk + RC.PAD, 2 * N), NAN, dtype=torch.float64)
    kv[:, :sp.Nk, :N], kv[:, :sp.Nk, N:] = RC.flat(case.k), RC.flat(case.v)
    return a.to(DEV, BF), w.to(DEV, BF), kv.to(DEV, BF)


@pytest.mark.parametrize("nk,dup,cfg,keys16", QPROJ)
def test_fused_projection_attention(nk, dup, cfg, keys16, tune):
    """The <= 96-key epilogues of cd360_qproj_attn_dedup_bf16 behind an exact projection: only the epilogue's P rounding is under test.
    dup = 1: one query batch element, served on the keys of batch 0 and of batch 1."""
    tune(**(dict(qattn_cfg=cfg) if keys16 is None else dict(qattn_cfg=cfg, qattn_keys16=keys16)))
    N, Kd, nq = RC.QPROJ_N, RC.QPROJ_K, RC.QPROJ_NQ
    for family in RC.FAMILIES:
        sp = RC.row_spec(family, nk, nq, dup)
        a, w, kv = qproj_inputs(sp)
        b = a.shape[0]
        out = torch.full((b + dup, nq, N), NAN, dtype=BF, device=DEV)
        k, v = kv[..., :N], kv[..., N:]
        _ok(_lib().cd360_qproj_attn_dedup_bf16(a.data_ptr(), w.data_ptr(), out.data_ptr(), b * nq, N, Kd, Kd, Kd, N, None, None, 0, 0, 0.0, None,
                                               k.data_ptr(), v.data_ptr(), k.stride(0), k.stride(1), v.stride(0), v.stride(1), nq, nk,
                                               RC.SCALE, dup, _stream()), "cd360_qproj_attn_dedup_bf16")
        check("qproj-bf16", "row", sp, out)


EAGER = [pytest.param(nq, nk, fast, id=f"{nq}x{nk}-fast{fast}") for nq, nk in RC.EAGER_SHAPES for fast in (1, 0)]


@pytest.mark.parametrize("nq,nk,fast", EAGER)
def test_eager_tiles(nq, nk, fast, tune):
    """attn_fwd_kernel: one ragged tile beside a full one, four tiles with a ragged query block, six tiles."""
    tune(attn_self=0, attn_fast=fast)
    kernel = "gen1-fast" if fast else "gen1-guarded"
    for family in RC.FAMILIES:
        sp = RC.eager_spec(family, nq, nk)
        q, k, v = device_qkv(sp)
        assert routed("plain", sp, k, attn_self=0, attn_fast=fast) == kernel
        check(kernel, "eager", sp, forward("plain", sp, q, k, v))
        assert routed("lse", sp, k, attn_self=0, attn_fast=fast) == kernel
        check(f"lse:{kernel}", "eager", sp, *forward("lse", sp, q, k, v))


@pytest.mark.parametrize("pick", (1, 2, 3))
def test_lazy_tiles(pick, tune):
    """attn_self_kernel in its three tilings, on the plain entry and on the pre-scaled one with q~ = bf16(fp32(q c)) handed over: the same
    fragments, so the same bits."""
    tune(attn_self=pick)
    for family in RC.FAMILIES:
        sp = RC.lazy_spec(family)
        case = RC.make_case(sp)
        q, k, v = device_qkv(sp)
        qt = torch.full((sp.B, sp.Nq, 3 * sp.H * 64), 5.0, dtype=BF, device=DEV)[..., 128:256]
        qt.copy_(RC.flat(RC.q_tilde(case.q)).to(DEV, BF))
        outs = {}
        for entry, qq in (("plain", q), ("prescaled", qt)):
            assert routed(entry, sp, k, attn_self=pick) == T.FORCED[pick]
            outs[entry] = forward(entry, sp, qq, k, v)
            check(f"{entry}:{T.FORCED[pick]}", "lazy", sp, outs[entry])
        assert torch.equal(outs["plain"].view(torch.int16), outs["prescaled"].view(torch.int16)), "the two entries differ"
        assert routed("lse", sp, k, attn_self=pick) == T.FORCED[pick]
        check(f"lse:{T.FORCED[pick]}", "lazy", sp, *forward("lse", sp, q, k, v))


def single(sp, q, k, v, qscale):
    b, n, d = sp.B, sp.Nq, sp.D
    out = torch.full((b, n, d), NAN, dtype=BF, device=DEV)
    nbytes = _lib().cd360_attn_single_workspace_bytes(b, n, d)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
    st = lambda t: _I64x2(t.stride(0), t.stride(1))
    _ok(_lib().cd360_attn_single_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), b, n, d, st(q), st(k), st(v), st(out), qscale,
                                      ws.data_ptr() if nbytes else None, _stream()), "cd360_attn_single_bf16")
    return out


@pytest.mark.parametrize("n,d", RC.SINGLE, ids=[f"n{n}-d{d}" for n, d in RC.SINGLE])
def test_single_head(n, d):
    """attn_single_kernel (+ attn_single_combine_kernel where the keys are split); q, k, v the column slices of one [1, N + 8, 3 D] buffer
    whose rows >= N are NaN."""
    assert _lib().cd360_attn_single_splits(1, n) == RC.SINGLE_SPLITS[n] == RC.single_splits(n)[0]
    for family in RC.FAMILIES:
        sp = RC.single_spec(family, n, d)
        case = RC.make_case(sp)
        m = torch.full((1, n + RC.PAD, 3 * d), NAN, dtype=torch.float64)
        m[:, :n, :d], m[:, :n, d:2 * d], m[:, :n, 2 * d:] = RC.flat(case.q), RC.flat(case.k), RC.flat(case.v)
        m = m.to(DEV, BF)
        q, k, v = m[:, :n, :d], m[..., d:2 * d], m[..., 2 * d:]
        out = single(sp, q, k, v, RC.C)
        check(f"single-splits{RC.SINGLE_SPLITS[n]}", "single", sp, out)
        if (n, d) == (512, 128):
            half = single(sp, (q * 2).contiguous(), k, v, RC.C / 2)
            check("single-qscale/2", "single", sp, half)
            assert torch.equal(half.view(torch.int16), out.view(torch.int16)), "qscale / 2 on a doubled q differs"


def backward(sp, q, k, v, o, do, lse, dq, dk, dv):
    ws = torch.full((sp.B * sp.H * sp.Nq,), NAN, dtype=torch.float32, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()
    st = lambda t: None if t is None else s3(t)
    _ok(_lib().cd360_attn_bwd_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), p(dq), p(dk), p(dv),
                                   ws.data_ptr(), sp.B, sp.H, sp.Nq, sp.Nk, s3(q), s3(k), s3(v), s3(o), s3(do), st(dq), st(dk), st(dv), RC.SCALE,
                                   _stream()), "cd360_attn_bwd_bf16")


@pytest.mark.parametrize("nq,nk", RC.BWD_SHAPES, ids=[f"{nq}x{nk}" for nq, nk in RC.BWD_SHAPES])
def test_backward(nq, nk):
    """cd360_attn_bwd_bf16 from the host's o and lse: dQ + dK/dV into tensors of their own; need_dq = False (the stand-alone delta kernel;
    dK, dV bit-equal to the first call's); at 128 x 128 into the slices of one d(q|k|v) buffer."""
    for family in RC.FAMILIES:
        sp = RC.bwd_spec(family, nq, nk)
        case = RC.make_case(sp)
        g = RC.bwd_ref(case)
        emu = RC.emulate_bwd(case)
        t_trunc = None
        if family == "positive":
            t_trunc = RC.bias(RC.emulate_bwd(case, "p_trunc").outs()[2], RC.flat(g.dv), RC.flat(g.A_dv))
        C = sp.H * 64
        q, k, v = device_qkv(sp)
        o, do = RC.flat(g.o).to(DEV, BF), RC.flat(case.do).to(DEV, BF)
        lse = g.lse.reshape(sp.B * sp.H, nq).to(DEV, torch.float32)
        rows = nk + RC.PAD

        def fresh():   # NaN where the kernel has to write, zero in the rows at and beyond Nk
            d = torch.full((sp.B, rows, C), NAN, dtype=BF, device=DEV)
            d[:, nk:] = 0
            return d

        def verdict(route, dq, dk, dv):
            got = (None if dq is None else dq.float().cpu().double(), dk[:, :nk].float().cpu().double(), dv[:, :nk].float().cpu().double())
            rq, rk, rv = RC.bwd_ratios(got, emu, g)
            worst = [0.0 if r is None else float(r.max()) for r in (rq, rk, rv)]
            t = RC.bias(got[2], RC.flat(g.dv), RC.flat(g.A_dv))
            tail = not bool(dk[:, nk:].any()) and not bool(dv[:, nk:].any())
            bar = "-" if t_trunc is None else f"{abs(t_trunc) / 4:.2e}"
            print(f"ATTN-ROUND bwd-{route} {RC.spec_id(sp)} worst={max(worst):.3f}/1 dq={worst[0]:.3f} dk={worst[1]:.3f} dv={worst[2]:.3f} "
                  f"flagged=P {emu.flagged_p:.5f} dS {emu.flagged_ds:.5f} T={t:.2e}/{bar} rows_beyond_nk_zero={tail}")
            assert max(worst) <= 1.0 and tail
            assert t_trunc is None or abs(t) <= abs(t_trunc) / 4

        dq = torch.full((sp.B, nq, C), NAN, dtype=BF, device=DEV)
        dk, dv = fresh(), fresh()
        backward(sp, q, k, v, o, do, lse, dq, dk, dv)
        verdict("dq+dkv", dq, dk, dv)
        dk2, dv2 = fresh(), fresh()
        backward(sp, q, k, v, o, do, lse, None, dk2, dv2)
        verdict("dkv-only", None, dk2, dv2)
        assert torch.equal(dk2[:, :nk].view(torch.int16), dk[:, :nk].view(torch.int16)) and torch.equal(dv2[:, :nk].view(torch.int16), dv[:, :nk].view(torch.int16))
        if (nq, nk) == (128, 128):
            m = torch.full((sp.B, rows, 3 * C), NAN, dtype=BF, device=DEV)
            m[:, nk:] = 0
            dq3, dk3, dv3 = m[:, :nq, :C], m[..., C:2 * C], m[..., 2 * C:]
            backward(sp, q, k, v, o, do, lse, dq3, dk3, dv3)
            verdict("slices", dq3, dk3, dv3)
