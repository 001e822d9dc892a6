"""Every forward softmax kernel on its rescale paths and at extreme logits: the cases of tests/softmax_cases.py (crafted rows in every
(wave, query block) slot; the dominating key in the first / an interior / the last tile, in both halves of a tile, on the last real
key, in the first / an interior / the last key split) against float64 softmax attention on the same bf16 inputs.  Needs an MI355X.

Bars (tests/test_softmax_cases_cpu.py holds the fp32 oracle to a tenth of each against the same reference):
  tensor-wide    max |got - want| / max |want| < 1e-2; 1.5e-2 on the plain entry forced to attn_self_kernel (its in-kernel q * c costs one
                 more bf16 rounding) -- the bars of tests/test_kernels_gpu.py, unchanged;
  crafted rows   the same bar on the crafted rows alone (error over them, divided by the whole tensor's max |want|);
  dominated rows (winner >= 40 units above every other key; tie: two winners; uniform) every element within 2^-7 relative of the
                 winning v / (v_a + v_b) / 2 / mean v: P is rounded to bf16 once and the output once, each <= 2^-9, losers weigh < 2^-40;
  lse            |lse - want| <= 2^-9 where q is not re-rounded (first generation, small-key); the looser bar of
                 test_self_attention_generations_agree_with_oracle where it is (attn_self = 1, 2, 3 on the plain entry).
Each test prints its figures (SOFTMAX-EDGE ...) before it asserts.

Measured on an MI355X, worst over shapes and families (tensor-wide / crafted rows / dominated rows / lse):
  attn_fwd_kernel, plain entry      3.7e-3 / 3.7e-3 / 3.9e-3 / 1.8e-5      ragged, attn_fast 1 and 0   3.0e-3 / 3.0e-3 / 3.9e-3 / 1.8e-5
  attn_self_kernel <1,4> <2,8> <1,8>, plain entry (bar 1.5e-2, lse bar 0.2-0.26)           6.7e-3 / 6.7e-3 / 3.9e-3 / 1.3e-1
  prescaled entry, by shape and attn_self = 2, 3                                            3.9e-3 / 3.6e-3 / 3.9e-3 / -
  attn_smallk_kernel 3.3e-3 / 3.3e-3 / 3.9e-3 / 2.2e-5    qproj epilogue 3.3e-3 / 3.3e-3 / 3.9e-3 / -
  attn_single (+ combine) 3.4e-3 / 3.2e-3 / 3.9e-3 / -      xformers entry 3.4e-3 / 3.4e-3 / 3.9e-3 / -
(3.9e-3 = 2^-8 is the tie / uniform rows: one bf16 rounding of the mean; late-spike and stair-down rows come out bit-exact.)

What these cases found: attn_self_kernel exchanged its tile maximum between the two key halves of a tile through
__builtin_amdgcn_permlane32_swap, and the compiled code read only the first result: every lane kept the maximum of lanes 0-31 (key
rows 0-3, 8-11, ... of each 32-key block).  A dominating key in the other rows never moved m_ref; up to 128 units above it the result
was still right (p < 2^128), beyond that exp2 overflowed: inf in l and lse, NaN in the row.  All three tilings, both entries."""
import pytest
import torch

import softmax_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
LSE_TIGHT = 2.0 ** -9


def check(label, sp, case, out, bar, lse=None, lse_tight=True):
    ref = S.reference(case)
    got = out.float().cpu().double()
    assert got.shape == ref.out.shape, (got.shape, ref.out.shape)
    finite = bool(torch.isfinite(got).all()) and (lse is None or bool(torch.isfinite(lse).all()))
    scale = ref.out.abs().max().item()
    err = (got - ref.out).abs()
    tensor = err.max().item() / scale
    crafted = S.q_rows(case, err).max().item() / scale if case.rows else 0.0
    dom = 0.0
    for r in case.rows:
        if r.target is not None:
            e = ((S.row_of(case, got, r.b, r.h, r.i) - r.target).abs() / r.target.abs()).max().item()
            dom = max(dom, e if e == e else float("inf"))  # a NaN row must not drop out of the maximum
    lse_err = lse_bar = None
    if lse is not None:
        lse_err = (lse.cpu().double() - ref.lse).abs().max().item()
        lse_bar = LSE_TIGHT if lse_tight else 2e-2 * max(1.0, ref.lse.abs().max().item() / 10)
    print(f"SOFTMAX-EDGE {label} {S.spec_id(sp)} finite={finite} tensor={tensor:.3e}/{bar:g} crafted={crafted:.3e}/{bar:g} "
          f"dominated={dom:.3e}/{2.0 ** -7:.3e} lse={lse_err if lse_err is None else format(lse_err, '.3e')}/{lse_bar}")
    assert finite
    assert tensor < bar and crafted < bar
    assert dom <= 2.0 ** -7
    if lse is not None:
        assert lse_err <= lse_bar if lse_tight else lse_err < lse_bar


def gens_for(sp, gens):
    nq = sp[3]
    return [g for g in gens if g in (None, 0, 1) or (g == 2 and nq % 512 == 0) or (g == 3 and nq % 256 == 0)]


PLAIN = [pytest.param(g, sp, id=f"attn_self{g}-{S.spec_id(sp)}") for sp in S.SELF_CASES for g in gens_for(sp, (0, 1, 2, 3))]


@pytest.mark.parametrize("gen,sp", PLAIN)
def test_plain_entry_forced_to_each_generation(gen, sp, tune):
    """ops.attention(want_lse=True) under tune(attn_self = 0 .. 3): attn_fwd_kernel and attn_self_kernel <1,4>, <2,8>, <1,8>, square
    (2 .. 16 tiles) and cross-shaped (2, 3, 5 tiles: below, at and beyond one lap of the four-slot ring)."""
    from cd360 import ops
    case = S.make_case(*sp)
    tune(attn_self=gen)
    q, k, v = S.device_inputs(case)
    out, lse = ops.attention(q, k, v, case.H, nk=case.Nk, want_lse=True)
    check(f"plain-gen{gen}", sp, case, out, 1e-2 if gen == 0 else 1.5e-2, lse, lse_tight=gen == 0)


PRESCALED = [pytest.param(g, sp, id=f"attn_self{'-by-shape' if g is None else g}-{S.spec_id(sp)}") for sp in S.PRESCALED_CASES
             for g in (gens_for(sp, (None, 2, 3)) if sp[3] % 128 == 0 else [None])]


@pytest.mark.parametrize("gen,sp", PRESCALED)
def test_prescaled_entry(gen, sp, tune):
    """ops.attention(prescaled=True), what the transformer blocks call when sampling: the kernel picked by shape (<1,4> here; the ragged
    N = 200 takes the first generation) and the two other tilings by override.  q is not re-rounded: the 1e-2 bar, and the offset family."""
    from cd360 import ops
    case = S.make_case(*sp)
    if gen is not None:
        tune(attn_self=gen)
    q, k, v = S.device_inputs(case)
    out = ops.attention(q, k, v, case.H, nk=case.Nk, prescaled=True)
    check(f"prescaled-gen{gen}", sp, case, out, 1e-2)


@pytest.mark.parametrize("fast", [1, 0])
@pytest.mark.parametrize("sp", S.RAGGED_CASES, ids=S.spec_id)
def test_first_generation_ragged(sp, fast, tune):
    """attn_fwd_kernel on ragged tiles, buffer-load path and guarded path, k / v NaN-padded: a spike on key Nk - 1 is the neighbour of
    the masked tail."""
    from cd360 import ops
    case = S.make_case(*sp)
    tune(attn_fast=fast)
    q, k, v = S.device_inputs(case, pad=True)
    out, lse = ops.attention(q, k, v, case.H, nk=case.Nk, want_lse=True)
    check(f"gen0-ragged-fast{fast}", sp, case, out, 1e-2, lse)


@pytest.mark.parametrize("sp", S.SMALLK_CASES, ids=S.spec_id)
def test_small_key_kernel(sp):
    """attn_smallk_kernel, one Nk per NKB: spikes on key 0 and on key Nk - 1 (next to the -1e30 padding), offset with every real logit near
    -60 units (still far above the padding), uniform."""
    from cd360 import ops
    case = S.make_case(*sp)
    q, k, v = S.device_inputs(case, pad=True)
    out, lse = ops.attention(q, k, v, case.H, nk=case.Nk, want_lse=True)
    check("smallk", sp, case, out, 1e-2, lse)


@pytest.mark.parametrize("sp", [s for s in S.SMALLK_CASES if s[3] % 128 == 0], ids=S.spec_id)
def test_qproj_attention_epilogue(sp):
    """The attention epilogue of the fused q-projection kernel on the same cases (those with Nq % 128 == 0, its envelope): identity projection
    (w = I in bf16, C = K = 128, no LayerNorm fold, no bias), so q is exactly a; and bit for bit against the dup = 1 form on the repeated batch."""
    from cd360 import ops
    case = S.make_case(*sp)
    C = case.H * case.D
    a, k, v = S.device_inputs(case, pad=True)
    w = torch.eye(C, dtype=BF, device=DEV)
    out = ops.qproj_attention(a, w, k, v, case.Nk, case.H)
    check("qproj", sp, case, out, 1e-2)
    b = case.B
    k3, v3 = torch.cat([k, k[:1]], 0), torch.cat([v, v[:1]], 0)  # the last query element also meets the keys of batch element 0
    got = ops.qproj_attention(a, w, k3, v3, case.Nk, case.H, dup=1)
    want = ops.qproj_attention(torch.cat([a, a[b - 1:]], 0).contiguous(), w, k3, v3, case.Nk, case.H)
    assert got.shape == (b + 1, case.Nq, C) and torch.equal(got, want) and torch.equal(got[:b], out)


@pytest.mark.parametrize("sp", S.SINGLE_CASES, ids=S.spec_id)
def test_single_head_kernel_and_its_combine(sp):
    """attn_single_kernel (+ attn_single_combine_kernel) at 1, 2 and 15 key splits: the winner in the first, an interior and the last
    split's ragged final tile, a tie across two splits, a first split that makes every other split's combine weight underflow."""
    from cd360 import ops
    case = S.make_case(*sp)
    n = case.Nq
    assert ops.attention_single_splits(1, n) == S.single_splits(n)[0] == {33: 1, 500: 2, 4100: 15}[n]
    q, k, v = S.device_inputs(case)
    out = ops.attention_single(q, k, v, qscale=case.c)
    check("single", sp, case, out, 1e-2)


@pytest.mark.parametrize("sp", S.XFORMERS_CASES, ids=S.spec_id)
def test_xformers_layout_entry(sp):
    from cd360 import ops
    case = S.make_case(*sp)
    out = ops.memory_efficient_attention(case.q.to(DEV, BF), case.k.to(DEV, BF), case.v.to(DEV, BF))
    check("xformers", sp, case, out, 1e-2)
