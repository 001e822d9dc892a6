"""cd360_qproj_attn_dedup_bf16 on DENSE weights, per output element: integer a and W (times one power of two) make the projection exact in
fp32 whatever the tile, ring, wave group or mover schedule does, so q = bf16(a W^T + bias) is one deterministic rounding and the row
pipeline of attn_round_cases judges the output (tests/qproj_cases.py states the method, tests/test_qproj_cases_cpu.py checks it).
Needs an MI355X.

  family A   bias, no LayerNorm: q exact
  family B   the LayerNorm fold of the attention epilogue (ln_stats in 1 or K / 128 partials, wsum, bias), plain rows and rows with
             |mean| / std of 16 .. 20; q elements within their fp32 unit of a bf16 midpoint widen the bar of their row (flagged_q)

K = 64, 192, 640, 1280 x N = 128, 384 (qattn_split 0 / 1), 640 x Nk = 20, 40, 77, 96 (EPI 2, 3, 7 -- 4 with qattn_keys16 = 0 --, 4) x
qattn_cfg 1 .. 4 x dup 0 / 1, as the covering lists qproj_cases.launches("A" / "B") of about 50 launches each; B = 2 query batch elements,
Nq = 256 (384 once, on the 128-row tiles).  Per element, nothing excluded: |got - emu| <= 2^-8 |emu| + EPS A + F + Fq, and on the
positive family |T| <= |T_trunc| / 4.  K / V rows >= Nk and the rows behind a's M rows are NaN.  Each case first asserts from the
restated dispatch (qproj_cases.route) that it reaches the instantiation(s) it is named for; each launch runs twice and must be bit-equal.
Each test prints QPROJ-EXACT <instantiation> <case> worst=<err / bar> flagged_q=<share> flagged_p=<share> T=<T>/<bar> before it asserts."""
import functools

import pytest
import torch

import attn_round_cases as RC
import qproj_cases as QC

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")


def _lib():
    from cd360 import _lib
    return _lib.load()


def _ok(code, what):
    from cd360 import _lib
    _lib.check(code, what)


@functools.lru_cache(maxsize=2)
def device_inputs(d):
    """a [M + 8, K] (the last 8 rows NaN), W [N, K], bias / wsum fp32 [N], ln_stats fp32 [M, parts, 2], k | v the halves of one
    [BQ + dup, Nk + 8, 2 N] buffer whose rows >= Nk are NaN."""
    b = QC.build(d)
    a = torch.full((d.M + RC.PAD, d.K), NAN, dtype=torch.float64)
    a[:d.M] = b.a.reshape(d.M, d.K)
    kv = torch.full((QC.BQ + d.dup, d.Nk + RC.PAD, 2 * d.N), NAN, dtype=torch.float64)
    kv[:, :d.Nk, :d.N], kv[:, :d.Nk, d.N:] = RC.flat(b.k), RC.flat(b.v)
    f32 = lambda x: None if x is None else x.to(DEV, torch.float32).contiguous()
    return a.to(DEV, BF), b.w.to(DEV, BF).contiguous(), f32(b.bias), f32(b.wsum), f32(b.stats), kv.to(DEV, BF)


def run(l):
    d = l.data
    a, w, bias, wsum, stats, kv = device_inputs(d)
    k, v = kv[..., :d.N], kv[..., d.N:]
    out = torch.full((QC.BQ + d.dup, d.Nq, d.N), NAN, dtype=BF, device=DEV)
    p = lambda x: None if x is None else x.data_ptr()
    _ok(_lib().cd360_qproj_attn_dedup_bf16(a.data_ptr(), w.data_ptr(), out.data_ptr(), d.M, d.N, d.K, d.K, d.K, d.N, p(bias), p(stats),
                                           d.parts if stats is not None else 0, d.K if stats is not None else 0, 1e-5 if stats is not None else 0.0,
                                           p(wsum), k.data_ptr(), v.data_ptr(), k.stride(0), k.stride(1), v.stride(0), v.stride(1), d.Nq, d.Nk,
                                           RC.SCALE, d.dup, torch.cuda.current_stream().cuda_stream), "cd360_qproj_attn_dedup_bf16")
    return out


def check(l):
    d = l.data
    e = QC.emulate(d)
    first, second = run(l), run(l)
    got = first.float().cpu().double()
    worst = float(QC.ratios(got, e).max())
    t = RC.bias(got, RC.flat(e.ex.out), RC.flat(e.ex.A))
    bar = "-" if e.t_trunc is None else f"{abs(e.t_trunc) / 4:.2e}"
    print(f"QPROJ-EXACT {'+'.join(l.inst)} {QC.launch_id(l)} worst={worst:.3f}/1 flagged_q={e.flagged_q:.5f} flagged_p={e.flagged_p:.5f} "
          f"rows_q={e.rows_q:.4f} T={t:.2e}/{bar}")
    assert worst <= 1.0
    assert e.t_trunc is None or abs(t) <= abs(e.t_trunc) / 4
    assert torch.equal(first.view(torch.int16), second.view(torch.int16)), "two runs of one launch differ"


def launch_test(l, tune):
    from cd360 import _lib
    d = l.data
    assert _lib.get_tuning()["gemm_movers"] < 0      # the mover waves are named as launch_ks decides them by default
    tune(qattn_cfg=l.cfg, qattn_split=l.split, **({} if l.keys16 is None else dict(qattn_keys16=l.keys16)))
    r = QC.route(d.M, d.N, d.Nq, d.Nk, l.cfg, l.split, l.keys16)
    assert r is not None and tuple(x[0] for x in r) == l.inst and QC.forced_ok(d, l.cfg)
    check(l)


LA, LB = QC.launches("A"), QC.launches("B")


@pytest.mark.parametrize("l", LA, ids=[QC.launch_id(l) for l in LA])
def test_dense_projection_with_bias(l, tune):
    """Family A: q = bf16(a W^T + bias), exact."""
    launch_test(l, tune)


@pytest.mark.parametrize("l", LB, ids=[QC.launch_id(l) for l in LB])
def test_layernorm_fold(l, tune):
    """Family B: q = bf16(fma(acc, rstd, fma(-rstd mean, wsum, bias))), judged with the flip allowance of qproj_cases."""
    launch_test(l, tune)
