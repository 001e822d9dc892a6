"""The <= 96-key attention kernels, bf16 and fp8, on inputs where float64 softmax attention is their exact answer up to the one bf16
rounding of the output (tests/attn_grid_cases.py: K, V integers in [-7, 7] times a power of two per batch and head, q sparse with
power-of-two maxima, a signed selection as the projection, scale * log2(e) = 1.0f through the C ABI, so every p is a power of two;
and a dense one-hot family whose output is the winning key's v row bit for bit).  Needs an MI355X.

What runs, each under its own test id:
  cd360_qproj_attn_dedup_bf16   qattn_cfg 1 .. 4 x Nk in 16 .. 96 (key-group epilogues of 2, 4, 5, 6 groups) x dup 0, 1 x N = 128 (K = 192)
                                and N = 384 (K = 384: 256 + 128 columns); Nk 65, 77, 80 again under qattn_keys16 = 0; N = 384,
                                qattn_cfg 1 again under qattn_split = 1; dup = 1 bit-equal to the expanded batch
  cd360_kv_pack_fp8 + cd360_qproj_attn_fp8_bf16   qattn_cfg 1 .. 4 x Nk in 65, 77, 80, 81, 96 x dup x the same widths
  cd360_attn_fwd_bf16, cd360_attn_fwd_fp8mfma_bf16   Nk in 20 .. 96 (NKB 1, 2, 3) x Nq 256, 200, q inside a 3 C wide row, k | v merged
  cd360_kv_pack_fp8 alone       image and scales torch.equal to the host restatement of the layout; a randn case within half an e4m3 step

Bar, per element, both families, bf16 and fp8 alike: |got - ref| <= 2^-8 |ref| + 2^-10 A, A = the softmax-weighted mean of |v|
(2^-9 is the bf16 rounding of the output; the rest covers 1 / l, the fp32 sums and the mass fp8 drops below 2^-17).  One-hot rows equal
bf16(v_winner) bit for bit.  tests/test_attn_grid_cpu.py holds fp32 emulations of both pipelines to a tenth of the bar in front of the
output rounding, and shows that each fault model (two K channels swapped, V^T keys permuted inside a group of four, a scale from the
neighbouring head / batch element / 32-token block, an unmasked padding key, the key count rounded up to 16, the wrong batch for dup)
breaks the bar on every case listed for it.  Each test prints ATTN-GRID <route> <case> worst=<err / bar> before it asserts.

Measured on an MI355X, worst err / bar over the cases of a route, grid family (the one-hot family is bit-exact on every route: ratio 0):
  cd360_qproj_attn_dedup_bf16, all tiles, epilogues, keys16 = 0, split (264 runs)   0.797      cd360_attn_fwd_bf16 (14 runs)           0.797
  cd360_kv_pack_fp8 + cd360_qproj_attn_fp8_bf16, all tiles (80 runs)                0.809      cd360_attn_fwd_fp8mfma_bf16 (14 runs)   0.809
  cd360_kv_pack_fp8: 0 of 258048 image bytes differ, scales equal (Nk 1, 31, 64, 77, 96); randn 1.000000 half steps (a value on a tie)
(0.797 = 2^-9 / (2^-8 + 2^-10): the output's own bf16 rounding on an element with A = |ref|; the fp8 routes add the mass below 2^-17.
The fp32 emulations of tests/test_attn_grid_cpu.py give the same two figures, 0.797 and 0.798 .. 0.81, and 0.036 at most in front of the
output rounding; the weakest fault model on any case, an unmasked all-zero fp8 padding key, reaches 173.)

What these cases found: nothing to fix.  Every tile, key-group epilogue, the split launch, the de-duplicated form, both fp8 forms and the
packed image pass at the bar as first stated, and the layout comment above kv_pack_fp8_kernel describes the image the kernel writes.  The
bf16 epilogue masks a padding key twice (rows >= Nk lie past the end of the K / V buffer descriptors and arrive as zeros, and the
accumulator of the last key block starts at -1e30), so with the mask gone a padding key would arrive as zeros, not as its attractive row:
that is what the rows with every logit below zero are for.  The fp8 form has the mask alone (its padding slots are zero bytes)."""
import ctypes
import functools

import pytest
import torch

import attn_grid_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
_I64x3 = ctypes.c_int64 * 3


def _lib():
    from cd360 import _lib
    return _lib.load()


def _ok(code, what):
    from cd360 import _lib
    _lib.check(code, what)


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=4)
def device_inputs(sp):
    """a [B, Nq, K], w [N, K], and k | v merged as one [B + dup, rows, 2 N] buffer (the layout of the merged k | v projection)."""
    case = G.make_case(sp)
    nb = sp.B + sp.dup
    kv = torch.cat([case.k.reshape(nb, case.rows, sp.N), case.v.reshape(nb, case.rows, sp.N)], -1).to(DEV, BF)
    return case.a.to(DEV, BF), case.w.to(DEV, BF), kv


def check(route, case, got):
    ref = G.reference(case)
    got = got.float().cpu()
    assert got.shape == ref.out.shape, (got.shape, ref.out.shape)
    worst = G.worst_ratio(got, ref)
    same = float((got.bfloat16() == ref.out.bfloat16()).double().mean())   # (reported only: elements equal to bf16(ref) itself)
    exact = None
    if case.spec.family == "onehot":
        exact = bool(torch.equal(got.bfloat16(), G.onehot_target(case).bfloat16()))
    print(f"ATTN-GRID {route} {G.spec_id(case.spec)} worst={worst:.3e}/1 equal_bf16_ref={same:.5f} winner_rows_bit_exact={exact}")
    assert worst <= 1.0
    assert exact is not False


def qproj(sp, a, w, kv, dup, packed=None):
    """The fused projection + attention through the C entry points, softmax scale G.SCALE; packed = (kv8, scales) takes the fp8 form."""
    N, Kd, nq = sp.N, sp.K, sp.Nq
    b = a.shape[0]
    out = torch.full((b + dup, nq, N), float("nan"), dtype=BF, device=DEV)
    k, v = kv[..., :N], kv[..., N:]
    if packed is None:
        _ok(_lib().cd360_qproj_attn_dedup_bf16(a.data_ptr(), w.data_ptr(), out.data_ptr(), b * nq, N, Kd, Kd, Kd, N, None, None, 0, 0, 0.0, None,
                                               k.data_ptr(), v.data_ptr(), k.stride(0), k.stride(1), v.stride(0), v.stride(1), nq, sp.Nk,
                                               G.SCALE, dup, _stream()), "cd360_qproj_attn_dedup_bf16")
    else:
        _ok(_lib().cd360_qproj_attn_fp8_bf16(a.data_ptr(), w.data_ptr(), out.data_ptr(), b * nq, N, Kd, Kd, Kd, N, None, None, 0, 0, 0.0, None,
                                             packed[0].data_ptr(), packed[1].data_ptr(), nq, sp.Nk, G.SCALE, dup, _stream()),
            "cd360_qproj_attn_fp8_bf16")
    return out


def kv_pack(kv, N, nk):
    nb, H = kv.shape[0], N // 64
    k, v = kv[..., :N], kv[..., N:]
    img = torch.full((nb, H, G.IMAGE_BYTES), 0xAB, dtype=torch.uint8, device=DEV)
    scales = torch.full((nb, H, 2), float("nan"), dtype=torch.float32, device=DEV)
    assert img.numel() == _lib().cd360_kv_fp8_bytes(nb, H)
    _ok(_lib().cd360_kv_pack_fp8(k.data_ptr(), v.data_ptr(), img.data_ptr(), scales.data_ptr(), nb, H, nk, k.stride(0), k.stride(1), v.stride(0),
                                 v.stride(1), _stream()), "cd360_kv_pack_fp8")
    return img, scales


def _variants(n, nk):
    v = [(f"bf16-qcfg{q}", dict(qattn_cfg=q), False) for q in G.QCFGS]
    if nk in G.NK_KEYS16:
        v += [(f"bf16-keys16off-qcfg{q}", dict(qattn_cfg=q, qattn_keys16=0), False) for q in G.QCFGS]
    if n == 384:
        v.append(("bf16-split-qcfg1", dict(qattn_cfg=1, qattn_split=1), False))
    if nk in G.NK_FP8:
        v += [(f"fp8-qcfg{q}", dict(qattn_cfg=q), True) for q in G.QCFGS]
    return v


# case-major order: the cases and their device copies are built once and shared by the variants that follow
QPROJ = [pytest.param(n, kdim, nk, dup, tuning, fp8, id=f"{name}-N{n}-nk{nk}-dup{dup}")
         for n, kdim in G.WIDTHS for nk in G.NK_BF16 for dup in (0, 1) for name, tuning, fp8 in _variants(n, nk)]


@pytest.mark.parametrize("n,kdim,nk,dup,tuning,fp8", QPROJ)
def test_fused_projection_attention(n, kdim, nk, dup, tuning, fp8, tune):
    """Both families on one (tile, key-group epilogue, bf16 / fp8, dup, keys16, split) combination; b = 2, Nq = 256, so the 256-row tiles
    are taken as asked.  dup = 1: also bit-equal to the plain form on the batch with its last element repeated."""
    tune(**tuning)
    route = "qproj-fp8" if fp8 else "qproj-bf16"
    for sp in G.qproj_specs(nk, n, kdim, dup):
        case = G.make_case(sp)
        a, w, kv = device_inputs(sp)
        packed = kv_pack(kv, n, nk) if fp8 else None
        out = qproj(sp, a, w, kv, dup, packed)
        check(route, case, out)
        if dup:
            wide = qproj(sp, torch.cat([a, a[sp.B - dup:]], 0).contiguous(), w, kv, 0, packed)
            assert torch.equal(out.view(torch.int16), wide.view(torch.int16)), "dup form differs from the expanded batch"


CORE = [pytest.param(kind, nk, nq, id=f"{kind}-nk{nk}-nq{nq}") for nk in G.NK_CORE for nq in G.NQ_CORE for kind in ("bf16", "fp8mfma")]


@pytest.mark.parametrize("kind,nk,nq", CORE)
def test_small_key_attention_entries(kind, nk, nq):
    """cd360_attn_fwd_bf16 / cd360_attn_fwd_fp8mfma_bf16 (attn_smallk_kernel, NKB 1, 2, 3; Nq = 200: a ragged last 32-query block) with q
    read out of a 3 C wide row and k | v out of the merged buffer.  The fp8 form scales per tensor: amax = (7 2^i, 7 2^j, 7 2^j)."""
    for sp in G.core_specs(nk, nq):
        case = G.make_case(sp)
        C, H = sp.N, case.H
        _, _, kv = device_inputs(sp)
        wide = torch.full((sp.B, nq, 3 * C), 5.0, dtype=BF, device=DEV)
        wide[..., C:2 * C] = case.q.reshape(sp.B, nq, C).to(DEV, BF)
        q, k, v = wide[..., C:2 * C], kv[..., :C], kv[..., C:]
        out = torch.full((sp.B, nq, C), float("nan"), dtype=BF, device=DEV)
        s3 = [_I64x3(t.stride(0), 64, t.stride(1)) for t in (q, k, v, out)]
        args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), sp.B, H, nq, nk, *s3, G.SCALE)
        if kind == "bf16":
            _ok(_lib().cd360_attn_fwd_bf16(*args, _stream()), "cd360_attn_fwd_bf16")
        else:
            amax = (ctypes.c_float * 3)(*G.core_amax(sp))
            _ok(_lib().cd360_attn_fwd_fp8mfma_bf16(*args, amax, _stream()), "cd360_attn_fwd_fp8mfma_bf16")
        check(f"core-{kind}", case, out)


@pytest.mark.parametrize("nk", G.NK_PACK)
def test_kv_pack_image_on_grid_cases(nk):
    """Every byte of the 14336-byte image per (batch, head) and both scales against the host restatement of the layout (the comment above
    kv_pack_fp8_kernel); slots of keys >= Nk are zero bytes although the k / v rows behind them are not."""
    sp = G.pack_spec(nk)
    case = G.make_case(sp)
    _, _, kv = device_inputs(sp)
    img, scales = kv_pack(kv, sp.N, nk)
    want_img, want_scales = G.kv_image(case.k, case.v, nk)
    img, scales = img.cpu(), scales.cpu()
    wrong = int((img != want_img).sum())
    print(f"ATTN-GRID kv-pack {G.spec_id(sp)} bytes_wrong={wrong}/{img.numel()} scales_equal={torch.equal(scales, want_scales)}")
    assert torch.equal(scales, want_scales)
    assert torch.equal(img, want_img)
    k8, v8 = G.decode_image(img)
    assert not k8[:, nk:].any() and not v8[:, nk:].any() and bool(case.k[:, nk:G.SLOTS].any() or nk == G.SLOTS)


def test_kv_pack_image_on_randn():
    """Off the grid: every decoded byte times its scale within half an e4m3 step of x, times (1 + 2^-20); scales = amax / 448."""
    nb, H, nk, rows = 2, 3, 77, 100
    g = torch.Generator().manual_seed(77)
    kv = (torch.randn(nb, rows, 2 * H * 64, generator=g) * 1.7).to(BF)
    img, scales = kv_pack(kv.to(DEV), H * 64, nk)
    img, scales = img.cpu(), scales.cpu().double()
    dec = G.decode_image(img)
    worst = 0.0
    for t, x in enumerate((kv[..., :H * 64], kv[..., H * 64:])):
        x = x.double().reshape(nb, rows, H, 64)
        s = scales[..., t]
        amax = x[:, :nk].abs().amax((1, 3))
        assert float(((s - amax / 448).abs() / s).max()) <= 2.0 ** -20
        y = x[:, :nk] / s[:, None, :, None]
        step = 2.0 ** (torch.floor(torch.log2(y.abs().clamp_min(2.0 ** -6))) - 3)     # e4m3 spacing in y's binade (2^-9 below 2^-6)
        err = (dec[t][:, :nk].double() - y).abs() / (step / 2)
        worst = max(worst, float(err.max()))
        assert not dec[t][:, nk:].any()
    k_bytes, v_bytes = img[..., :96 * 64].reshape(nb, H, 96, 64), img[..., 96 * 64:].reshape(nb, H, 64, 128)
    zero_k = not k_bytes[:, :, nk:].any()
    zero_v = not v_bytes[:, :, torch.from_numpy(G.V_INDEX >= nk)].any()
    print(f"ATTN-GRID kv-pack randn worst={worst:.6f}/{1 + 2.0 ** -20:.6f} half steps, padding slots zero: K {zero_k} V {zero_v}")
    assert worst <= 1 + 2.0 ** -20
    assert zero_k and zero_v
