"""The text conditioner on the MI355X: the four entry points of include/text/cd360_text.h against torch (bit-equal where the arithmetic is
exact, the suite's bounds elsewhere), the whole towers and the conditioner on the HIP route against tests/text_fp32.py under the rule

    rel(HIP route, fp32 reference)  <=  2 x rel(torch's own bf16 arithmetic on the CPU, fp32 reference)

measured in the same test (nothing is fixed in advance: the factor covers another summation order and the algebraic LayerNorm fold), the
conditioner's rows through a tiny job.Sampler, and every entry point under tests/guarded.py.  `rel` is the max-norm relative error."""
import copy
import ctypes

import pytest
import torch

import guarded as G
import sampler_cases as SC
import text_cases as TC
import text_fp32 as T32

DEV, BF = SC.DEV, SC.BF
rel = T32.rel


def _bf(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ================================================================================================ 1: embedding
@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [1, 77])
@pytest.mark.parametrize("D", [128, 768])
def test_embedding_is_one_rounding_and_its_statistics_are_the_stored_rows(B, N, D):
    """out == (tok[ids].float() + pos.float()).bfloat16() bit for bit; the (sum, sum of squares) of every STORED row against float64 sums at
    rel < 1e-5; the host refuses an id outside the table before the launch."""
    from cd360 import ops
    V = 96
    tok, pos = _bf(V, D, seed=1), _bf(N, D, seed=2, scale=0.5)
    ids = torch.randint(0, V, (B, N), generator=torch.Generator().manual_seed(3))
    ids[0, 0], ids[-1, -1] = 0, V - 1
    out, stats = ops.text_embed(ids.to(DEV), tok, pos, want_stats=True, ids_host=ids)
    want = (tok[ids.to(DEV)].float() + pos.float()[None]).bfloat16()
    assert out.shape == (B, N, D) and torch.equal(out, want)
    assert torch.equal(ops.text_embed(ids.to(DEV), tok, pos), want)  # without the statistics: the same rows
    rows = out.double().reshape(B * N, D)
    assert stats.shape == (B * N, 1, 2) and stats.dtype == torch.float32
    e1, e2 = rel(stats[:, 0, 0], rows.sum(1)), rel(stats[:, 0, 1], (rows * rows).sum(1))
    print("embedding statistics rel", e1, e2)
    assert e1 < 1e-5 and e2 < 1e-5
    bad = ids.clone()
    bad[0, 0] = V
    with pytest.raises(ValueError):
        ops.text_embed(bad.to(DEV), tok, pos, ids_host=bad)


@pytest.mark.gpu
def test_embedding_writes_a_zero_row_for_an_id_outside_the_table():
    """The binding called directly (the host check bypassed): ids V, -1 and 2^40 give rows of zeros with statistics (0, 0); their neighbours
    are what they are without them."""
    from cd360 import _text
    B, N, V, D = 3, 77, 96, 128
    tok, pos = _bf(V, D, seed=4), _bf(N, D, seed=5)
    ids = torch.randint(0, V, (B, N), generator=torch.Generator().manual_seed(6))
    hit = [(0, 0, V), (1, 40, -1), (2, 76, 1 << 40)]
    for b, n, v in hit:
        ids[b, n] = v
    d_ids = ids.to(DEV)
    out = torch.full((B, N, D), 7.0, dtype=BF, device=DEV)
    stats = torch.full((B * N, 1, 2), 7.0, device=DEV)
    rc = _text.load().cd360_text_embed_bf16(d_ids.data_ptr(), tok.data_ptr(), pos.data_ptr(), out.data_ptr(), B, N, V, D, D, stats.data_ptr(), _stream())
    assert rc == 0
    safe = ids.clamp(0, V - 1).to(DEV)
    want = (tok[safe].float() + pos.float()[None]).bfloat16()
    for b, n, _ in hit:
        want[b, n] = 0
        assert not out[b, n].any() and not stats[b * N + n].any()
    assert torch.equal(out, want)


# ================================================================================================ 2: causal attention
def _attn_ref(q, k, v, H, scale=0.125):
    """fp32 masked softmax attention on the same bf16 inputs, on the CPU.  q, k, v [B, N, H * 64] -> [B, N, H * 64] fp32."""
    B, N, _ = q.shape
    q, k, v = (t.float().cpu().reshape(B, N, H, 64).transpose(1, 2) for t in (q, k, v))
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(torch.ones(N, N, dtype=torch.bool).triu(1), float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, N, H * 64)


def _qkv(B, N, H, layout, seed, rows=None):
    """-> q, k, v [B, N, H * 64] bf16 on the GPU: the three column slices of one merged [B, rows, 3 * H * 64] buffer, or three contiguous tensors."""
    D = H * 64
    rows = N if rows is None else rows
    buf = _bf(B, rows, 3 * D, seed=seed)
    q, k, v = buf[:, :N, :D], buf[:, :N, D:2 * D], buf[:, :N, 2 * D:]
    return (q, k, v) if layout == "merged" else (q.contiguous(), k.contiguous(), v.contiguous())


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["merged", "contiguous"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H", [1, 2])
@pytest.mark.parametrize("N", [1, 8, 32, 33, 64, 65, 77, 128])
def test_causal_attention_against_fp32_masked_softmax(N, H, B, layout):
    """rel < 1e-2 against fp32 masked softmax attention on the same bf16 inputs (the bound the suite holds cd360_attn_fwd_bf16 to), and
    row 0 of every head is v[0] bit for bit."""
    from cd360 import ops
    q, k, v = _qkv(B, N, H, layout, seed=N + H)
    out = ops.causal_attention(q, k, v, H)
    assert out.shape == (B, N, H * 64) and out.is_contiguous()
    assert torch.equal(out[:, 0], v[:, 0])
    err = rel(out, _attn_ref(q, k, v, H))
    print("causal attention rel", err)
    assert err < 1e-2


@pytest.mark.gpu
def test_causal_attention_of_constant_values_is_the_constant():
    """q = 0 and every column of v constant at a bf16-representable value: the probabilities of row i are 1 / (i + 1) each and every output
    row is that value, bit for bit (n c / n in fp32)."""
    from cd360 import ops
    B, N, H = 2, 77, 2
    q = torch.zeros(B, N, H * 64, dtype=BF, device=DEV)
    k = _bf(B, N, H * 64, seed=9)
    col = (torch.arange(H * 64) - 50).to(BF) / 8  # multiples of 1 / 8 up to 9.6: exact in bf16
    v = col.to(DEV)[None, None].expand(B, N, H * 64).contiguous()
    out = ops.causal_attention(q, k, v, H)
    assert torch.equal(out, v)


@pytest.mark.gpu
def test_causal_attention_does_not_leak_from_later_keys():
    """Run once; then overwrite the keys and values at positions > i with finite values of magnitude 1e4 (finite: 0 * NaN is NaN in the
    reference as well): rows <= i are bit-identical to the first run.  An unmasked or off-by-one kernel fails this."""
    from cd360 import ops
    B, N, H = 2, 77, 2
    q, k, v = _qkv(B, N, H, "merged", seed=21)
    first = ops.causal_attention(q, k, v, H)
    for i in (0, 31, 32, 63, 76):
        k2, v2 = k.clone(), v.clone()
        big = torch.where(_bf(B, N - 1 - i, H * 64, seed=i).float() < 0, -1e4, 1e4).to(BF)
        k2[:, i + 1:], v2[:, i + 1:] = big, -big
        out = ops.causal_attention(q, k2, v2, H)
        assert torch.equal(out[:, :i + 1], first[:, :i + 1]), i
        if i + 1 < N:
            assert not torch.equal(out[:, i + 1:], first[:, i + 1:]), i  # the later rows do see them


# ================================================================================================ 3: activation
def _act_ref(x, kind):
    x = x.float()
    return x * torch.sigmoid(1.702 * x) if kind == 0 else torch.nn.functional.gelu(x)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1])
def test_activation_against_torch_fp32(kind):
    """QuickGELU (0) and exact GELU (1) on [77, 5120] and on a ragged [5, 48] with a row stride: rel < 8e-3 against torch fp32 on the same bf16
    input (the suite's bound for geglu); the columns behind the ragged rows are not touched; in place gives the same bits."""
    from cd360 import ops
    x = _bf(77, 5120, seed=31, scale=3.0)
    out = ops.text_activation(x, kind)
    err = rel(out, _act_ref(x, kind))
    print("activation kind", kind, "rel", err)
    assert err < 8e-3
    wide = _bf(5, 64, seed=32, scale=3.0)
    dst = torch.full((5, 64), 7.0, dtype=BF, device=DEV)
    got = ops.text_activation(wide[:, :48], kind, out=dst[:, :48])
    assert rel(got, _act_ref(wide[:, :48], kind)) < 8e-3 and bool((dst[:, 48:] == 7).all())
    assert torch.equal(ops.text_activation(wide[:, :48], kind), got) and torch.equal(ops.text_activation(x.clone(), kind, out=None), out)
    y = x.clone()
    assert ops.text_activation(y, kind, out=y) is y and torch.equal(y, out)
    with pytest.raises(Exception):
        ops.text_activation(x, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1])
def test_activation_at_zero_infinity_and_large_arguments(kind):
    """x = 0 -> 0; x = +inf -> +inf; every value is finite where torch's fp32 result (rounded to bf16) is, and equal to it there up to the
    suite's bound."""
    from cd360 import ops
    vals = [0.0, -0.0, float("inf"), float("-inf"), 1e4, -1e4, 3e38, -3e38, 88.0, -88.0, 60.0, -60.0, 1e-30, -1e-30, 5.0, -5.0]
    x = torch.tensor(vals, dtype=BF, device=DEV).reshape(1, 16)
    got = ops.text_activation(x, kind).float().cpu().flatten()
    want = _act_ref(x, kind).bfloat16().float().cpu().flatten()
    print("activation specials kind", kind, got.tolist(), want.tolist())
    assert got[0] == 0 and got[1] == 0 and got[2] == float("inf")
    fin = torch.isfinite(want)
    assert bool(torch.isfinite(got[fin]).all())
    # the geglu bound relative to the ARGUMENT: the negative tail is x times a difference of nearly equal numbers in torch's fp32 as well
    mag = x.float().cpu().flatten().abs()[fin]
    assert bool(((got[fin] - want[fin]).abs() <= 8e-3 * mag).all())


# ================================================================================================ 4: pooling
@pytest.mark.gpu
@pytest.mark.parametrize("B,N,D", [(3, 77, 128), (1, 1, 128), (2, 128, 1280), (5, 65, 768)])
def test_eot_pool_is_the_gather_at_the_first_maximum(B, N, D):
    """Bit-equal to x[b, argmax_n ids[b, n]]; among equal maxima the lowest index wins (in the first 64 ids, behind them, and across the two)."""
    from cd360 import ops
    x = _bf(B, N, D, seed=41)
    ids = torch.randint(0, 90, (B, N), generator=torch.Generator().manual_seed(42))
    if N > 1:
        ids[0, N // 2] = ids[0, N - 1] = 95  # a tie: the earlier one
    if N > 70 and B > 1:
        ids[1, 3] = ids[1, 70] = 94  # a tie across the lanes' second trip
    at = [int((row == row.max()).nonzero()[0]) for row in ids]
    assert at == ids.argmax(-1).tolist()  # torch.argmax: the first maximal value
    got = ops.eot_pool(x, ids.to(DEV))
    assert got.shape == (B, D) and torch.equal(got, x[torch.arange(B), torch.tensor(at)])


# ================================================================================================ 5: whole towers
def _yardstick(ref, ids, want=None):
    """torch's own bf16 arithmetic: text_fp32's module cast to bf16, on the CPU -> its result(s), the yardstick _check measures."""
    with torch.no_grad():
        return copy.deepcopy(ref).bfloat16()(ids)


def _check(name, got, low, want):
    ours, yard = rel(got.float(), want), rel(low.float(), want)
    print(f"{name}: HIP route rel {ours:.3e}, torch bf16 rel {yard:.3e}, ratio {ours / max(yard, 1e-30):.2f}")
    assert torch.isfinite(got.float()).all()
    assert ours <= 2 * yard, (name, ours, yard)


TOWERS = [("small", TC.SMALL, 3), ("clip-l-width", TC.CLIP_L, 1), ("bigg-width", TC.BIG_G, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,arch,B", TOWERS, ids=[t[0] for t in TOWERS])
def test_clip_tower_on_the_hip_route(name, arch, B):
    """FrozenCLIPEmbedder in bf16 on the GPU against text_fp32's HF tower in fp32, within 2 x torch's bf16 run; hidden[:, :i + 1] is bit-identical
    when the ids behind position i change (causality through the whole stack: GEMM rows are independent); a tape raises."""
    emb, ref, _ = TC.clip_pair(None, seed=51, arch=arch)
    ids = T32.token_ids(B, arch["vocab"], seed=52)
    with torch.no_grad():
        want = ref(ids)
    low = _yardstick(ref, ids, want)
    emb = emb.to(DEV, BF)
    with torch.no_grad():
        got = emb(ids)
    assert got.dtype == BF and got.shape == (B, 77, arch["width"])
    _check(f"clip {name}", got, low, want)
    for i in (0, 31, 63):
        other = ids.clone()
        other[:, i + 1:] = torch.randint(0, arch["vocab"], (B, 76 - i), generator=torch.Generator().manual_seed(i))
        with torch.no_grad():
            again = emb(other)
        assert torch.equal(again[:, :i + 1], got[:, :i + 1]), i
        assert not torch.equal(again[:, i + 1:], got[:, i + 1:]), i
    emb.transformer.text_model.embeddings.token_embedding.weight.requires_grad = True
    with pytest.raises(NotImplementedError, match="no_grad"):
        emb(ids)


@pytest.mark.gpu
@pytest.mark.parametrize("name,arch,B", TOWERS, ids=[t[0] for t in TOWERS])
def test_openclip_tower_on_the_hip_route(name, arch, B):
    """FrozenOpenCLIPEmbedder in bf16 on the GPU against text_fp32's nn.MultiheadAttention tower in fp32: penultimate, last and pooled each
    within 2 x torch's bf16 run; with a modifier id above EOT's the pooled row is the modifier's; causality through the stack."""
    V = arch["vocab"]
    emb, ref, _ = TC.openclip_pair("<new1>", seed=61, arch=arch)
    ids = T32.token_ids(B, V, seed=62, modifier=(V, 3))
    with torch.no_grad():
        want = ref(ids)
    low = _yardstick(ref, ids, want)
    emb = emb.to(DEV, BF)
    with torch.no_grad():
        z = emb.encode_with_transformer(ids.to(DEV))
        pen, pooled = emb(ids)
    assert torch.equal(pen, z["penultimate"]) and torch.equal(pooled, z["pooled"])
    for key in ("penultimate", "last", "pooled"):
        _check(f"openclip {name} {key}", z[key], low[key], want[key])
    other = ids.clone()
    other[:, 40:] = torch.randint(0, V, (B, 37), generator=torch.Generator().manual_seed(7))
    with torch.no_grad():
        again = emb.encode_with_transformer(other.to(DEV))
    assert torch.equal(again["last"][:, :40], z["last"][:, :40]) and torch.equal(again["penultimate"][:, :40], z["penultimate"][:, :40])
    with pytest.raises(NotImplementedError, match="no_grad"):
        emb(ids)  # the modifier row keeps the token table trainable: a tape


# ================================================================================================ 6: the LayerNorm fold on an offset stream
def _offset_tables(sd, tok_key, pos_key, seed):
    """Tables whose sum is EXACT in bf16, so the fp32 reference, torch's bf16 run and the HIP route see the same layer input: token values
    are multiples of 1 / 2 in [-4, 4], every position row is 64 with channel 5 at 512 (the token table is 0 there)."""
    V, D = sd[tok_key].shape
    tok = torch.randint(-8, 9, (V, D), generator=torch.Generator().manual_seed(seed)).float() / 2
    tok[:, 5] = 0
    pos = torch.full_like(sd[pos_key], 64.0)
    pos[:, 5] = 512.0
    sd[tok_key], sd[pos_key] = tok, pos
    return sd


@pytest.mark.gpu
@pytest.mark.parametrize("tower", ["clip", "openclip"])
def test_layernorm_fold_on_a_stream_with_an_offset_and_a_massive_channel(tower):
    """One layer of each tower at its real width on an input whose rows carry a common offset of 64 and one channel at 512 -- the
    massive-activation channels real CLIP weights are known for (real weights cannot be tested: nothing may be downloaded).  The folded
    LayerNorm works from (sum, sum of squares); the same 2 x rule against torch's bf16 run."""
    if tower == "clip":
        arch = TC.CLIP_L
        emb, ref, sd = TC.clip_pair(None, seed=71, arch=arch)
        p = "transformer.text_model.embeddings."
        sd = _offset_tables(dict(sd), p + "token_embedding.weight", p + "position_embedding.weight", 72)
    else:
        arch = TC.BIG_G
        emb, ref, sd = TC.openclip_pair(None, seed=73, arch=arch)
        sd = _offset_tables(dict(sd), "model.token_embedding.weight", "model.positional_embedding", 74)
    ref.load_state_dict(sd, strict=True)
    emb.load_state_dict(sd, strict=True)
    ids = T32.token_ids(2, arch["vocab"], seed=75)
    with torch.no_grad():
        want = ref(ids)
    low = _yardstick(ref, ids, want)
    emb = emb.to(DEV, BF)
    with torch.no_grad():
        if tower == "clip":
            _check("offset clip", emb(ids), low, want)
        else:
            z = emb.encode_with_transformer(ids.to(DEV))
            assert torch.equal(z["penultimate"].float().cpu(), want["penultimate"])  # the layer input is exact in bf16
            for key in ("last", "pooled"):
                _check(f"offset openclip {key}", z[key], low[key], want[key])


# ================================================================================================ 7: the conditioner, and into the job
@pytest.mark.gpu
def test_conditioner_on_the_hip_route_and_into_the_sampler():
    """The shipped emb_models (one layer each at the real widths, so that crossattn is 2048 and vector 2816 wide -- what the UNet takes) on the
    GPU: (c, uc) against the CPU torch route in fp32 under the tower rule (yardstick: the CPU torch route in bf16); uc is all zeros.  Then
    cd360.text.sampler_rows' rows into the tiny job.Sampler for two steps: finite, and bit-equal to the same sampler fed rows built by hand."""
    from cd360 import job as J
    from cd360 import text
    cond = TC.conditioner(arches=(TC.CLIP_L, TC.BIG_G))
    batch = TC.batch(1, 0)
    keys = [e.input_keys for e in cond.embedders]
    call = lambda m, b: m.get_unconditional_conditioning(b, force_uc_zero_embeddings=keys, force_ref_zero_embeddings=True)
    with torch.no_grad():
        c32, uc32 = call(cond, batch)
        clow, _ = call(copy.deepcopy(cond).bfloat16(), batch)
    gpu = cond.to(DEV, BF)
    dbatch = {k: (v if k.startswith("txt") else v.to(DEV)) for k, v in batch.items()}
    # modifier_token: the conditioner calls the encoders outside no_grad, as the reference does -- but with `is_trainable: False` its
    # constructor has cleared every requires_grad, the token table's included, so no tape exists and the HIP route serves the call
    assert not any(p.requires_grad for p in gpu.parameters())
    c, uc = call(gpu, dbatch)
    with torch.no_grad():
        again, _ = call(gpu, dbatch)
    assert all(torch.equal(c[k], again[k]) and not c[k].requires_grad for k in c)
    assert c["crossattn"].shape == (1, 77, 2048) and c["vector"].shape == (1, 2816)
    for key in ("crossattn", "vector"):
        _check(f"conditioner {key}", c[key], clow[key], c32[key])
        assert not uc[key].any() and uc[key].shape == c[key].shape
    pose, _, _, x0 = SC.job(0, nb=3)
    ctx, y = text.sampler_rows(c, uc, 3)
    assert ctx.shape == (3, 77, 2048) and y.shape == (3, 2816) and ctx.dtype == BF
    hand_ctx = torch.cat([uc["crossattn"], uc["crossattn"], c["crossattn"]]).to(BF)
    hand_y = torch.cat([uc["vector"], uc["vector"], c["vector"]]).to(BF)
    assert torch.equal(ctx, hand_ctx) and torch.equal(y, hand_y)
    try:
        with torch.no_grad():
            a = J.sample_assigned(SC.sampler(pose, ctx, y, use_graph=False), [(pose, ctx, y, x0)], 2)[0]
            b = J.sample_assigned(SC.sampler(pose, hand_ctx, hand_y, use_graph=False), [(pose, hand_ctx, hand_y, x0)], 2)[0]
        assert torch.isfinite(a).all() and torch.equal(a, b)
    finally:
        SC.release()


# ================================================================================================ 8: guarded memory
def _guarded_case(case):
    from cd360 import _text, ops
    g = torch.Generator().manual_seed(81)
    if case == "embed-stats":
        inputs = dict(ids=torch.randint(0, 96, (3, 77), generator=g).to(DEV), tok=_bf(96, 128, seed=82), pos=_bf(77, 128, seed=83))

        @SC.guardfn
        def fn(guard, ids, tok, pos):
            with G.recorded(guard, _text):
                out, stats = ops.text_embed(ids, tok, pos, want_stats=True)
            return dict(out=out, stats=stats)
    elif case == "causal-attn-merged":
        B, N, H, rows = 2, 77, 2, 96  # 19 rows of every prompt's buffer behind the tokens hold the poison and are never read
        inputs = dict(qkv=_bf(B, N, 3 * H * 64, seed=84))

        @SC.guardfn
        def fn(guard, qkv):
            D = H * 64
            buf = guard.torch.empty((B, rows, 3 * D), dtype=BF, device=DEV)
            buf[:, :N].copy_(qkv)
            with G.recorded(guard, _text):
                out = ops.causal_attention(buf[..., :D], buf[..., D:2 * D], buf[..., 2 * D:], H, n=N)
            assert torch.equal(out, ops_attn_plain(qkv, H))
            return dict(out=out)

        def ops_attn_plain(qkv, H):
            D = H * 64
            return ops.causal_attention(qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:], H)
    elif case == "act-both-kinds":
        inputs = dict(x=_bf(5, 48, seed=85, scale=3.0), big=_bf(77, 512, seed=86))

        @SC.guardfn
        def fn(guard, x, big):
            wide = guard.torch.empty((5, 64), dtype=BF, device=DEV)  # the 16 columns behind every ragged row stay poison
            wide[:, :48].copy_(x)
            with G.recorded(guard, _text):
                outs = [ops.text_activation(wide[:, :48], kind) for kind in (0, 1)] + [ops.text_activation(big, kind) for kind in (0, 1)]
            return dict(outs=outs)
    else:
        assert case == "eot-pool"
        inputs = dict(x=_bf(3, 77, 128, seed=87), ids=torch.randint(0, 96, (3, 77), generator=g).to(DEV))

        @SC.guardfn
        def fn(guard, x, ids):
            with G.recorded(guard, _text):
                return dict(out=ops.eot_pool(x, ids))
    return fn, inputs


@pytest.mark.gpu
@pytest.mark.parametrize("case,declares", TC.GUARDED, ids=[c[0] for c in TC.GUARDED])
def test_text_entry_points_write_their_outputs_only(case, declares):
    """Every launching entry point under tests/guarded.py, both poison patterns: outputs (and the padded operand buffers of the attention and
    the activation) live in arena blocks between canaries, so no guard byte changes; the results are finite and bit-equal between the
    poisons -- for the attention with the rows behind the tokens holding the poison -- and the operands are unchanged."""
    fn, inputs = _guarded_case(case)
    G.run_twice(fn, inputs, declares=declares)
