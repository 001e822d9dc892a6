"""Training the modifier-token embeddings on the MI355X: the four entry points of include/textgrad/cd360_textgrad.h against torch (bit-equal
where the arithmetic is exact), the whole towers' backward (cd360.grad.TextTowerFn) and the conditioner joint against tests/text_fp32.py
under the rule the forward is held to,

    rel(HIP route, fp32 autograd)  <=  2 x rel(torch's own bf16 autograd on the CPU, fp32 autograd)

measured in the same test (nothing is fixed in advance), and every entry point under tests/guarded.py.  `rel` is the max-norm relative
error."""
import copy

import pytest
import torch

import guarded as G
import sampler_cases as SC
import text_cases as TC
import text_fp32 as T32
import textgrad_cases as TG

DEV, BF = SC.DEV, SC.BF
rel = T32.rel


def _bf(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(DEV)


def _check(name, got, low, want):
    ours, yard = rel(got.float(), want), rel(low.float(), want)
    print(f"{name}: HIP route rel {ours:.3e}, torch bf16 rel {yard:.3e}, ratio {ours / max(yard, 1e-30):.2f}")
    assert torch.isfinite(got.float()).all()
    assert ours <= 2 * yard, (name, ours, yard)


# ================================================================================================ 1: attention backward
def _attn(q, k, v, H, scale=0.125):
    """Causal attention in the tensors' own dtype (fp32: the reference; bf16 on the CPU: torch's own bf16 arithmetic).  [B, N, H * 64]."""
    B, N, _ = q.shape
    q, k, v = (t.reshape(B, N, H, 64).transpose(1, 2) for t in (q, k, v))
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(torch.ones(N, N, dtype=torch.bool).triu(1), float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, N, H * 64)


def _attn_grads(q, k, v, d_o, H, dtype):
    leaves = [t.float().cpu().to(dtype).requires_grad_(True) for t in (q, k, v)]
    _attn(*leaves, H).backward(d_o.float().cpu().to(dtype))
    return [t.grad.float() for t in leaves]


def _operands(B, N, H, layout, seed, rows=None):
    """q, k, v, d_o [B, N, H * 64] bf16 on the GPU: the three column slices of one merged [B, rows, 3 * H * 64] buffer or three contiguous
    tensors; d_o contiguous."""
    D = H * 64
    rows = N if rows is None else rows
    buf = _bf(B, rows, 3 * D, seed=seed)
    q, k, v = buf[:, :N, :D], buf[:, :N, D:2 * D], buf[:, :N, 2 * D:]
    if layout != "merged":
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    return q, k, v, _bf(B, N, D, seed=seed + 1000)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["merged", "separate"])
@pytest.mark.parametrize("B,H", [(1, 1), (3, 2)])
@pytest.mark.parametrize("N", [1, 2, 33, 64, 65, 77, 128])
def test_attention_backward_against_fp32_autograd(N, B, H, layout):
    """dq, dk, dv against fp32 autograd of the same causal attention on the same bf16 values, each within 2 x the error of torch's bf16
    autograd on the CPU; merged-projection strides (outputs the three column slices of one buffer) and separate buffers."""
    from cd360 import ops
    q, k, v, d_o = _operands(B, N, H, layout, seed=N + H)
    if layout == "merged":
        dq, dk, dv = ops.causal_attention_bwd(q, k, v, d_o, H)
        inner = H * 64  # the three column slices of ONE [B, N, 3 * H * 64] buffer
        assert dq.stride(1) == 3 * inner and dk.data_ptr() == dq.data_ptr() + 2 * inner and dv.data_ptr() == dq.data_ptr() + 4 * inner
    else:
        out = tuple(torch.empty(B, N, H * 64, dtype=BF, device=DEV) for _ in range(3))
        dq, dk, dv = ops.causal_attention_bwd(q, k, v, d_o, H, out=out)
    want = _attn_grads(q, k, v, d_o, H, torch.float32)
    low = _attn_grads(q, k, v, d_o, H, torch.bfloat16)
    for name, g, l, w in zip(("dq", "dk", "dv"), (dq, dk, dv), low, want):
        _check(f"attention backward N={N} B*H={B * H} {layout} {name}", g, l, w)


@pytest.mark.gpu
def test_attention_backward_exact_properties():
    """dq[0] is exactly zero (row 0 has one key: P = 1, dS = P (dP - dP)); two launches give identical bits; dq[: i + 1] does not change by
    a bit when the k, v rows behind i are overwritten with +-1e4; dk[j :] and dv[j :] do not change by a bit when the q and dO rows before j
    change; rows >= N of every output buffer are untouched.
    dv[N - 1] = P[N - 1][N - 1] dO[N - 1] is bf16(dO[N - 1]) bit for bit exactly when that probability is 1: at N = 1, and at N = 77 with a
    last key that dominates its row (every other term of the row's softmax underflows to 0, so the row sum is 1 in fp32)."""
    from cd360 import ops
    B, N, H = 2, 77, 2
    D = H * 64
    q, k, v, d_o = _operands(B, N, H, "merged", seed=21)
    dq, dk, dv = ops.causal_attention_bwd(q, k, v, d_o, H)
    assert not dq[:, 0].any()
    again = ops.causal_attention_bwd(q, k, v, d_o, H)
    assert all(torch.equal(a, b) for a, b in zip(again, (dq, dk, dv)))
    for i in (0, 31, 32, 63, 76):
        k2, v2 = k.clone(), v.clone()
        big = torch.where(_bf(B, N - 1 - i, D, seed=i).float() < 0, -1e4, 1e4).to(BF)
        k2[:, i + 1:], v2[:, i + 1:] = big, -big
        dq2 = ops.causal_attention_bwd(q, k2, v2, d_o, H)[0]
        assert torch.equal(dq2[:, :i + 1], dq[:, :i + 1]), i
        if i + 1 < N:
            assert not torch.equal(dq2[:, i + 1:], dq[:, i + 1:]), i  # the later rows do see them
    for j in (1, 32, 33, 64, 76):
        q2, g2 = q.clone(), d_o.clone()
        q2[:, :j], g2[:, :j] = _bf(B, j, D, seed=100 + j), _bf(B, j, D, seed=200 + j)
        _, dk2, dv2 = ops.causal_attention_bwd(q2, k, v, g2, H)
        assert torch.equal(dk2[:, j:], dk[:, j:]) and torch.equal(dv2[:, j:], dv[:, j:]), j
        assert not torch.equal(dv2[:, :j], dv[:, :j]), j  # the earlier keys do see them ...
        assert torch.equal(dk2[:, :j], dk[:, :j]) == (j == 1), j  # ... except dk[0] of query 0 alone, whose dS is exactly 0 whatever q[0], dO[0] are
    # ---- rows >= N: operands hold 96 rows, the outputs too; only the first N are read and written
    rows = 96
    qr, kr, vr, _ = _operands(B, rows, H, "merged", seed=21)
    qr[:, :N], kr[:, :N], vr[:, :N] = q, k, v
    gr = torch.full((B, rows, D), 3.0, dtype=BF, device=DEV)
    gr[:, :N] = d_o
    buf = torch.full((B, rows, 3 * D), 7.0, dtype=BF, device=DEV)
    out = ops.causal_attention_bwd(qr, kr, vr, gr, H, n=N, out=(buf[..., :D], buf[..., D:2 * D], buf[..., 2 * D:]))
    assert bool((buf[:, N:] == 7).all()) and all(torch.equal(a[:, :N], b) for a, b in zip(out, (dq, dk, dv)))
    # ---- dv[N - 1] == bf16(dO[N - 1]) where P[N - 1][N - 1] is exactly 1
    q1, k1, v1, g1 = _operands(B, 1, H, "separate", seed=22)
    d1 = ops.causal_attention_bwd(q1, k1, v1, g1, H)
    assert torch.equal(d1[2], g1) and not d1[0].any() and not d1[1].any()
    qd, kd = q.clone(), k.clone()
    qd[:, N - 1] = 8.0
    kd[:, N - 1] = 8.0  # s = 0.125 * 64 * 64 = 512 for the last key, |s| < 0.125 * 64 * 8 * 5 for every other: exp(s_j - 512) = 0 in fp32
    dvd = ops.causal_attention_bwd(qd, kd, v, d_o, H)[2]
    assert torch.equal(dvd[:, N - 1], d_o[:, N - 1])


# ================================================================================================ 2: activation backward
def _act_grad_ref(x, dy, kind):
    x = x.float().cpu().double().requires_grad_(True)
    y = x * torch.sigmoid(1.702 * x) if kind == 0 else torch.nn.functional.gelu(x)
    y.backward(dy.float().cpu().double())
    return x.grad


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1])
def test_activation_backward_against_autograd(kind):
    """dy * f'(x) for QuickGELU (0) and exact GELU (1) on [77, 5120] and on a ragged, strided [5, 48]: rel < 8e-3 against torch autograd on the
    same bf16 values (the suite's bound for the forward activation: one bf16 rounding of the result is 3.9e-3); the columns behind the
    ragged rows are not touched; in place (dx == dy) gives the bits of out of place.  For |x| up to 30 nothing is NaN and the derivative is
    0 or 1 up to one bf16 rounding of the reference."""
    from cd360 import ops
    x, dy = _bf(77, 5120, seed=31, scale=3.0), _bf(77, 5120, seed=32)
    out = ops.text_activation_bwd(x, dy, kind)
    err = rel(out, _act_grad_ref(x, dy, kind))
    print("activation backward kind", kind, "rel", err)
    assert err < 8e-3
    wide, gwide = _bf(5, 64, seed=33, scale=3.0), _bf(5, 56, seed=34)
    dst = torch.full((5, 64), 7.0, dtype=BF, device=DEV)
    got = ops.text_activation_bwd(wide[:, :48], gwide[:, :48], kind, out=dst[:, :48])
    assert rel(got, _act_grad_ref(wide[:, :48], gwide[:, :48], kind)) < 8e-3 and bool((dst[:, 48:] == 7).all())
    assert torch.equal(ops.text_activation_bwd(wide[:, :48], gwide[:, :48], kind), got)
    y = dy.clone()
    assert ops.text_activation_bwd(x, y, kind, out=y) is y and torch.equal(y, out)
    vals = [0.0, -0.0, 30.0, -30.0, 29.5, -29.5, 20.0, -20.0, 12.0, -12.0, 8.0, -8.0, 5.0, -5.0, 1.0, -1.0]
    xs = torch.tensor(vals, dtype=BF, device=DEV).reshape(1, 16)
    ones = torch.ones_like(xs)
    d = ops.text_activation_bwd(xs, ones, kind).float().cpu().flatten()
    want = _act_grad_ref(xs, ones, kind).float().flatten()
    print("activation backward specials kind", kind, d.tolist())
    assert bool(torch.isfinite(d).all()) and d[0] == 0.5 and d[1] == 0.5
    assert bool(((d - want).abs() <= 4e-3 * want.abs().clamp_min(1e-3)).all())
    far = torch.tensor(vals, dtype=BF).abs() >= 20
    assert bool(((d[far] - (torch.tensor(vals)[far] > 0).float()).abs() < 1e-6).all())  # derivative -> 0 or 1
    with pytest.raises(Exception):
        ops.text_activation_bwd(x, dy, 2)


# ================================================================================================ 3: scatter and token rows
def _ints(*shape, seed, lo=-8, hi=9):
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed)).to(BF).to(DEV)


def _tied_ids(B, N, seed):
    ids = torch.randint(0, 90, (B, N), generator=torch.Generator().manual_seed(seed))
    if N > 1:
        ids[0, N // 2] = ids[0, N - 1] = 95  # a tie: the earlier one
    if N > 70 and B > 1:
        ids[1, 3] = ids[1, 70] = 94  # a tie across the lanes' second trip
    return ids


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,D", [(3, 77, 128), (1, 1, 128), (2, 128, 1280), (1, 77, 768)])
def test_eot_scatter_is_index_add_at_the_first_maximum(B, N, D):
    """Small integers (every sum exact in bf16): bit-equal to torch's index_add in fp32 at argmax_n ids (the lowest index among equal
    maxima); every other row keeps its bits; two runs give the same bits."""
    from cd360 import ops
    dx0, dp = _ints(B, N, D, seed=41), _ints(B, D, seed=42)
    ids = _tied_ids(B, N, seed=43)
    at = ids.argmax(-1)
    assert at.tolist() == [int((row == row.max()).nonzero()[0]) for row in ids]
    want = dx0.float().reshape(B * N, D).index_add(0, (torch.arange(B) * N + at).to(DEV), dp.float()).reshape(B, N, D).to(BF)
    got = ops.eot_scatter(dp, ids.to(DEV), dx0.clone())
    assert torch.equal(got, want) and torch.equal(ops.eot_scatter(dp, ids.to(DEV), dx0.clone()), got)
    untouched = torch.ones(B, N, dtype=torch.bool)
    untouched[torch.arange(B), at] = False
    assert torch.equal(got[untouched.to(DEV)], dx0[untouched.to(DEV)])


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("D,k", [(128, 3), (1280, 2), (768, 1)])
def test_token_rows_is_the_masked_index_add(B, D, k):
    """Small integers: bit-equal to torch's index_add in fp32 over the positions that hold each modifier id; a modifier that occurs nowhere
    gives a zero row; no other id contributes; two runs give the same bits, and the rows of prompt 0 alone (B = 1) are the B = 3 rows with
    the later prompts' occurrences removed."""
    from cd360 import ops
    N, V = 77, 96
    g = torch.Generator().manual_seed(51)
    ids = torch.randint(0, V, (3, N), generator=g)
    mods = list(range(V, V + k))
    ids[0, 5] = ids[0, 70] = ids[2, 0] = mods[-1]  # twice in one prompt, and in two of three
    if k > 1:
        ids[1, 76] = mods[0]
    ids = ids[:B].contiguous()
    dx = _ints(B, N, D, seed=52 + B)
    want = torch.zeros(V + 3, D).index_add(0, ids.flatten(), dx.float().cpu().reshape(B * N, D))[V:V + k]
    got = ops.token_rows_grad(dx, ids.to(DEV), mods)
    assert got.dtype == torch.float32 and got.shape == (k, D) and torch.equal(got.cpu(), want)
    assert torch.equal(ops.token_rows_grad(dx, ids.to(DEV), mods), got)
    if k == 3:
        assert not got[1].any() and bool(got[2].any())  # the middle modifier occurs nowhere
    if k > 1 and B == 1:
        assert not got[0].any()  # ... and the first one only in prompt 1


# ================================================================================================ 4: whole towers
TOWERS = [("small", TC.SMALL, 3), ("clip-l-width", TC.CLIP_L, 1), ("bigg-width", TC.BIG_G, 1)]


def _tower_case(tower, arch, B, k, seed, sd_edit=None, **kw):
    modifier = "+".join(f"<new{i + 1}>" for i in range(k))
    emb, ref, sd = (TC.clip_pair if tower == "clip" else TC.openclip_pair)(modifier, seed=seed, arch=arch, **kw)
    if sd_edit is not None:
        sd = sd_edit(dict(sd))
        ref.load_state_dict(sd, strict=True)
        emb.load_state_dict(sd, strict=True)
    V = arch["vocab"]
    ids = TG.prompt_ids("two-of-three" if B > 1 else "twice-in-one", V, k, seed=seed + 1, B=B)
    return emb.to(DEV, BF), ref, ids, V


def _names(tower, emb, ids):
    """The embedder's results under TextTowerFn's names, and its no_grad results in the same order."""
    if tower == "clip":
        return {"last_ln": emb(ids)}
    z = emb.encode_with_transformer(ids.to(DEV))
    return {"pen": z["penultimate"], "last_ln": z["last"], "pooled": z["pooled"]}


def _tower_grads(tower, arch, B, k, seed, sources, sd_edit=None):
    """-> (name, HIP rows.grad, torch-bf16 rows.grad, fp32 rows.grad) for every set of gradient sources."""
    from cd360 import finetune
    emb, ref, ids, V = _tower_case(tower, arch, B, k, seed, sd_edit)
    with torch.no_grad():
        plain = _names(tower, emb, ids)
    tr = finetune.train_tokens(TG.holder(emb))
    assert tr.rows[0].dtype == BF and tr.rows[0].is_cuda and not emb._tables()[0].requires_grad
    out = []
    for names in sources:
        tr.rows[0].grad = None
        outs = _names(tower, emb, ids)
        for n, t in outs.items():
            assert t.requires_grad and torch.equal(t, plain[n]), n  # the training forward: the no_grad route's bits
        cots = TG.cotangents({n: outs[n].shape for n in names}, seed=seed + 2)
        TG.functional({n: outs[n] for n in names}, cots).backward()
        got = tr.rows[0].grad
        assert got.dtype == BF and got.shape == (k, arch["width"])
        want = TG.reference_grad(ref, ids, k, cots)
        assert not want[:V].any()
        low = TG.reference_grad(ref, ids, k, cots, torch.bfloat16)
        out.append(("+".join(names), got, low[V:], want[V:]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,arch,B", TOWERS, ids=[t[0] for t in TOWERS])
def test_clip_tower_backward_on_the_hip_route(name, arch, B):
    """FrozenCLIPEmbedder (k = 3 modifier rows) in bf16 on the GPU, marked by train_tokens: the training forward returns the bits of the
    no_grad route; rows.grad of a random linear functional against the fp32 tower's masked gradient, within 2 x torch's bf16 autograd."""
    for what, got, low, want in _tower_grads("clip", arch, B, 3, 81, [("last_ln",)]):
        _check(f"clip {name} rows.grad [{what}]", got, low, want)


@pytest.mark.gpu
@pytest.mark.parametrize("name,arch,B", TOWERS, ids=[t[0] for t in TOWERS])
def test_openclip_tower_backward_on_the_hip_route(name, arch, B):
    """FrozenOpenCLIPEmbedder (k = 2) with the shipped `layer: penultimate`, pooled, legacy=False: gradients arriving on penultimate only, on
    pooled only (through text_projection, the scatter to the modifier's position -- the reference's argmax quirk --, ln_final and the last
    layer) and on penultimate, last and pooled together."""
    for what, got, low, want in _tower_grads("openclip", arch, B, 2, 91, [("pen",), ("pooled",), ("pen", "last_ln", "pooled")]):
        _check(f"openclip {name} rows.grad [{what}]", got, low, want)


@pytest.mark.gpu
def test_openclip_last_layer_and_legacy_routes_on_the_hip_route():
    """layer="last" without pooled, and legacy=True on both layers (the final LayerNorm of the chosen layer): forward bits and rows.grad."""
    from cd360 import finetune
    V, k = TC.SMALL["vocab"], 1
    for layer, legacy, name in (("last", False, "last_ln"), ("last", True, "last_ln"), ("penultimate", True, "pen_ln")):
        emb, ref, ids, _ = _tower_case("openclip", TC.SMALL, 3, k, 101, layer=layer, always_return_pooled=False, legacy=legacy)
        with torch.no_grad():
            plain = emb(ids)
        tr = finetune.train_tokens(TG.holder(emb))
        out = emb(ids)
        assert out.requires_grad and torch.equal(out, plain)
        cots = TG.cotangents({name: out.shape}, seed=102)
        TG.functional({name: out}, cots).backward()
        _check(f"openclip layer={layer} legacy={legacy} rows.grad", tr.rows[0].grad, TG.reference_grad(ref, ids, k, cots, torch.bfloat16)[V:],
               TG.reference_grad(ref, ids, k, cots)[V:])


@pytest.mark.gpu
@pytest.mark.parametrize("tower", ["clip", "openclip"])
def test_tower_backward_on_a_stream_with_an_offset_and_a_massive_channel(tower):
    """One layer of each tower at its real width on the offset-stream tables of the forward's test (rows with a common offset of 64 and one
    channel at 512): both LayerNorm backwards work on that stream; the same 2 x rule."""
    if tower == "clip":
        p = "transformer.text_model.embeddings."
        edit = lambda sd: TG.offset_tables(sd, p + "token_embedding.weight", p + "position_embedding.weight", 112)
        cases = _tower_grads("clip", TC.CLIP_L, 2, 1, 111, [("last_ln",)], sd_edit=edit)
    else:
        edit = lambda sd: TG.offset_tables(sd, "model.token_embedding.weight", "model.positional_embedding", 114)
        cases = _tower_grads("openclip", TC.BIG_G, 2, 1, 113, [("pen", "last_ln", "pooled")], sd_edit=edit)
    for what, got, low, want in cases:
        _check(f"offset {tower} rows.grad [{what}]", got, low, want)


@pytest.mark.gpu
def test_unmarked_embedder_with_a_trainable_table_still_refuses_a_tape():
    """The opt-in is the mark: a HIP-route embedder whose token table requires grad raises NotImplementedError ("no_grad") under a tape, as
    before; the same embedder after train_tokens serves the tape; one without modifier tokens cannot be marked and keeps refusing."""
    from cd360 import finetune
    emb, _, _ = TC.openclip_pair("<new1>", seed=121)
    emb = emb.to(DEV, BF)
    assert emb._tables()[0].requires_grad and "token_rows" not in emb.__dict__
    ids = T32.token_ids(1, TC.SMALL["vocab"], seed=122, modifier=(TC.SMALL["vocab"], 3))
    with pytest.raises(NotImplementedError, match="no_grad"):
        emb(ids)
    finetune.train_tokens(TG.holder(emb))
    assert all(t.requires_grad for t in emb(ids))
    clip, _, _ = TC.clip_pair(None, seed=123)
    clip = clip.to(DEV, BF)
    clip._tables()[0].requires_grad = True
    with pytest.raises(NotImplementedError, match="no_grad"):
        clip(ids.clamp(max=TC.SMALL["vocab"] - 1))


# ================================================================================================ 5: the conditioner joint
def _cross_attend(x, ctx, wq, wk, wv, wo, bo, heads):
    """MemoryEfficientCrossAttention's arithmetic in plain torch, in the tensors' dtype: softmax(q k^T / 8) v, then to_out."""
    B, n, _ = x.shape
    split = lambda t: t.reshape(B, t.shape[1], heads, 64).transpose(1, 2)
    q, k, v = split(x @ wq.t()), split(ctx @ wk.t()), split(ctx @ wv.t())
    o = torch.softmax((q @ k.transpose(-1, -2)) * 0.125, -1) @ v
    return o.transpose(1, 2).reshape(B, n, heads * 64) @ wo.t() + bo


@pytest.mark.gpu
def test_conditioner_joint_carries_the_gradient_into_both_rows():
    """The shipped emb_models at small widths on the GPU in bf16: train_tokens, c = cond(batch) carries the tape; c["crossattn"] feeds a
    MemoryEfficientCrossAttention (the smallest module of sgm/modules/attention.py that cross-attends to the text), c["vector"] a Linear on
    grad.LinearFn; both rows.grad against the same graph on the CPU in fp32, within 2 x the same graph on the CPU in bf16.  Then one fused
    MasterAdamW step with max_grad_norm changes the rows and, after sync(), the tables' last rows; no other row changes by a bit."""
    from cd360 import finetune, ops
    from sgm.modules.attention import MemoryEfficientCrossAttention
    heads, qd = 2, 128
    cond = TC.conditioner("<new1>")
    batch = TC.batch(2, 1)
    cd, vd = 2 * TC.SMALL["width"], TC.SMALL["proj"] + 3 * 512
    attn = MemoryEfficientCrossAttention(qd, context_dim=cd, heads=heads, dim_head=64)
    sd = T32.synth_weights(attn, seed=131)
    attn.load_state_dict(sd, strict=True)
    for p in attn.parameters():
        p.requires_grad = False
    g = torch.Generator().manual_seed(132)
    x = torch.randn(3, 16, qd, generator=g).bfloat16().float()
    wl = (torch.randn(64, vd, generator=g) * 0.05).bfloat16().float()
    cots = TG.cotangents({"attn": (3, 16, qd), "lin": (3, 64)}, seed=133)
    grads = {}
    for dtype in (torch.float32, torch.bfloat16):
        cpu = copy.deepcopy(cond).to(dtype)
        tr = finetune.train_tokens(cpu)
        c = cpu(batch)
        w = {k_: v_.to(dtype) for k_, v_ in sd.items()}
        outs = {"attn": _cross_attend(x.to(dtype), c["crossattn"], w["to_q.weight"], w["to_k.weight"], w["to_v.weight"], w["to_out.0.weight"],
                                      w["to_out.0.bias"], heads),
                "lin": c["vector"].to(dtype) @ wl.to(dtype).t()}
        TG.functional(outs, cots).backward()
        grads[dtype] = [r.grad.float() for r in tr.rows]
    gpu = cond.to(DEV, BF)
    attn = attn.to(DEV, BF)
    dbatch = {k_: (v_ if k_.startswith("txt") else v_.to(DEV)) for k_, v_ in batch.items()}
    tr = finetune.train_tokens(gpu)
    assert not any(p.requires_grad for p in gpu.parameters()) and all(r.is_cuda and r.dtype == BF for r in tr.rows)
    c = gpu(dbatch)
    assert c["crossattn"].requires_grad and c["vector"].requires_grad and c["crossattn"].shape == (3, 77, cd) and c["vector"].shape == (3, vd)
    outs = {"attn": attn(x.to(DEV, BF), context=c["crossattn"]), "lin": ops.linear(c["vector"].to(BF), wl.to(DEV, BF))}
    TG.functional(outs, cots).backward()
    for i, r in enumerate(tr.rows):
        _check(f"conditioner joint rows.grad of embedder {i}", r.grad, grads[torch.bfloat16][i], grads[torch.float32][i])
    V = TC.SMALL["vocab"]
    tables = [e._tables()[0].detach().clone() for e in gpu.embedders[:2]]
    start = [r.detach().clone() for r in tr.rows]
    opt = finetune.MasterAdamW([{"params": list(tr.parameters()), "lr": 1e-2}], max_grad_norm=1.0)
    assert opt.fused and opt.live
    opt.step()
    torch.cuda.synchronize()
    assert all(not torch.equal(r.detach(), s) and torch.isfinite(r.detach().float()).all() for r, s in zip(tr.rows, start))
    for e, t, s in zip(gpu.embedders[:2], tables, start):
        assert torch.equal(e._tables()[0].detach(), t) and torch.equal(t[V:], s)  # the step wrote the rows, not the tables
    tr.sync()
    for e, t, r in zip(gpu.embedders[:2], tables, tr.rows):
        now = e._tables()[0].detach()
        assert torch.equal(now[:V], t[:V]) and torch.equal(now[V:], r.detach())


# ================================================================================================ 6: guarded memory
def _guarded_case(case):
    from cd360 import _textgrad, ops
    g = torch.Generator().manual_seed(141)
    if case == "attn-bwd-merged":
        B, N, H, rows = 2, 77, 2, 96  # 19 rows of every prompt's buffers behind the tokens hold the poison and are never read
        D = H * 64
        inputs = dict(qkv=_bf(B, N, 3 * D, seed=142), d_o=_bf(B, N, D, seed=143))

        @SC.guardfn
        def fn(guard, qkv, d_o):
            buf = guard.torch.empty((B, rows, 3 * D), dtype=BF, device=DEV)
            buf[:, :N].copy_(qkv)
            gbuf = guard.torch.empty((B, rows, D), dtype=BF, device=DEV)
            gbuf[:, :N].copy_(d_o)
            with G.recorded(guard, _textgrad):
                dq, dk, dv = ops.causal_attention_bwd(buf[..., :D], buf[..., D:2 * D], buf[..., 2 * D:], gbuf, H, n=N)
                plain = ops.causal_attention_bwd(qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:], d_o, H)
            assert all(torch.equal(a, b) for a, b in zip((dq, dk, dv), plain))
            return dict(dq=dq, dk=dk, dv=dv)
    elif case == "act-bwd-both-kinds":
        inputs = dict(x=_bf(5, 48, seed=144, scale=3.0), dy=_bf(5, 48, seed=145), big=_bf(77, 512, seed=146), dbig=_bf(77, 512, seed=147))

        @SC.guardfn
        def fn(guard, x, dy, big, dbig):
            wide = guard.torch.empty((5, 64), dtype=BF, device=DEV)  # the 16 columns behind every ragged row stay poison
            wide[:, :48].copy_(x)
            gwide = guard.torch.empty((5, 56), dtype=BF, device=DEV)
            gwide[:, :48].copy_(dy)
            with G.recorded(guard, _textgrad):
                outs = [ops.text_activation_bwd(wide[:, :48], gwide[:, :48], kind) for kind in (0, 1)]
                outs += [ops.text_activation_bwd(big, dbig, kind) for kind in (0, 1)]
            return dict(outs=outs)
    elif case == "eot-scatter":
        inputs = dict(dp=_bf(3, 128, seed=148), ids=torch.randint(0, 96, (3, 77), generator=g).to(DEV), dx0=_bf(3, 77, 128, seed=149))

        @SC.guardfn
        def fn(guard, dp, ids, dx0):
            dx = guard.torch.empty((3, 77, 128), dtype=BF, device=DEV)
            dx.copy_(dx0)
            with G.recorded(guard, _textgrad):
                return dict(dx=ops.eot_scatter(dp, ids, dx))
    else:
        assert case == "token-rows"
        ids = torch.randint(0, 96, (3, 77), generator=g)
        ids[0, 4] = ids[2, 9] = 97
        inputs = dict(dx=_bf(3, 77, 128, seed=150), ids=ids.to(DEV))

        @SC.guardfn
        def fn(guard, dx, ids):
            with G.recorded(guard, _textgrad):
                return dict(rows=ops.token_rows_grad(dx, ids, [96, 97, 98]))
    return fn, inputs


@pytest.mark.gpu
@pytest.mark.parametrize("case,declares", TG.GUARDED, ids=[c[0] for c in TG.GUARDED])
def test_textgrad_entry_points_write_their_outputs_only(case, declares):
    """Every entry point under tests/guarded.py, both poison patterns: outputs (and the padded operand buffers of the attention backward and
    the activation backward) live in arena blocks between canaries, so no guard byte changes; the results are finite and bit-equal between
    the poisons -- for the attention with the rows behind the tokens holding the poison -- and the operands are unchanged."""
    fn, inputs = _guarded_case(case)
    G.run_twice(fn, inputs, declares=declares)
