"""Training the modifier-token embeddings, without a GPU: the fifth library's header <=> table <=> exports, its host-side refusals and
its resource record; finetune.train_tokens on the torch route (CPU, fp32) against the reference's masked embedding restated on the
tests/text_fp32.py towers; the routing of marked and unmarked embedders; the rows through the optimiser and the delta checkpoint."""
import ctypes
import importlib.util
import json
import os

import pytest
import torch

import sampler_cases as SC
import text_cases as TC
import text_fp32 as T32
import textgrad_cases as TG


# ================================================================================================ 1: header, table, library
def test_textgrad_header_matches_its_table_and_the_older_libraries_are_closed():
    """include/textgrad/cd360_textgrad.h <=> cd360._textgrad.TEXTGRAD_SIGNATURES <=> libcd360_textgrad.so by the rule of
    sampler_cases._header_table_library (every `cd360_...(` word, comments included), with EVERY library of sampler_cases.LIBRARIES as an
    older one: no new name is in one of their tables or headers or exported by them.  The binding and the source read no environment,
    the source never synchronises, and the build table ends with this library's row behind the four older rows."""
    from cd360 import _textgrad, ops
    tables, headers, libs = TG.older_libraries()
    assert len(tables) >= 9 and len(libs) == len(SC.LIBRARIES) and any(h.endswith("cd360_text.h") for h in headers)
    mismatch, in_tables, in_headers, mistyped, lib = SC._header_table_library(_textgrad.HEADER, _textgrad.TEXTGRAD_SIGNATURES, TG.NEW, tables,
                                                                             headers, _textgrad.load())
    assert not mismatch, mismatch
    assert not in_tables, in_tables
    assert not in_headers, in_headers
    assert not mistyped, mistyped
    assert _textgrad.HEADER == TG.HEADER and all(n.startswith("cd360_textgrad_") for n in TG.NEW)
    for older in libs:
        for name in TG.NEW:
            assert not hasattr(older, name), name
    src = open(_textgrad.__file__).read()
    assert "os.environ" not in src and "getenv" not in src
    hip = open(os.path.join(SC.ROOT, "custom-diffusion360_amd", "csrc_textgrad", "text_backward.hip")).read()
    assert "getenv" not in hip and "Synchronize" not in hip and "atomic" not in hip.replace("no atomics", "")
    assert SC.header_constant(TG.HEADER, "CD360_TEXTGRAD_MAX_MODIFIERS") == ops.TEXTGRAD_MAX_MODIFIERS == _textgrad.MAX_MODIFIERS == 3
    spec = importlib.util.spec_from_file_location("_graft_entry_for_textgrad", os.path.join(SC.ROOT, "__graft_entry__.py"))
    entry = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(entry)
    assert tuple(entry.LIBRARIES[-1]) == TG.BUILD_ROW and len(entry.LIBRARIES) == len(SC.LIBRARIES) + 1
    assert [row[3] for row in entry.LIBRARIES[:-1]] == [m for _, m, _, _ in SC.LIBRARIES]


def test_textgrad_entry_points_refuse_bad_arguments_on_the_host():
    """Fabricated non-null pointers: every call below returns CD360_ERR_ARG (-1) or CD360_ERR_SHAPE (-2) before anything launches."""
    from cd360 import _textgrad
    lib = _textgrad.load()
    nul, P = ctypes.c_void_p(None), ctypes.c_void_p
    a, b, c, d, e, f, g = (P(0x1000000 * i) for i in range(1, 8))
    S = lambda *v: (ctypes.c_int64 * 3)(*v)
    good = S(77 * 384, 64, 384)
    # ---- cd360_textgrad_causal_attn_bwd_bf16(q, k, v, d_o, dq, dk, dv, B, H, N, 7 stride arrays, scale, stream)
    bwd = lib.cd360_textgrad_causal_attn_bwd_bf16
    ptrs = ("q", "k", "v", "d_o", "dq", "dk", "dv")
    strides = ("qs", "ks", "vs", "dos", "dqs", "dks", "dvs")

    def call(B=2, H=2, N=77, scale=0.125, **kw):
        args = dict(zip(ptrs, (a, b, c, d, e, f, g)), **{s: good for s in strides})
        args["dos"] = S(77 * 128, 64, 128)
        args.update(kw)
        return bwd(*(args[n] for n in ptrs), B, H, N, *(args[s] for s in strides), scale, nul)

    for name in ptrs:
        assert call(**{name: nul}) == -1, name
        assert call(**{name: P(0x1000008)}) == -1, name  # 8-byte aligned only
    for name in strides:
        assert call(**{name: None}) == -1, name
        assert call(**{name: S(77 * 384, 64, 388)}) == -2 and call(**{name: S(77 * 384 + 4, 64, 384)}) == -2, name  # multiples of 4 only
        assert call(**{name: S(77 * 384, 64, -384)}) == -2, name
    assert call(B=0) == -1 and call(H=0) == -1 and call(H=-1) == -1 and call(B=-2) == -1
    assert call(scale=float("nan")) == -1 and call(scale=float("inf")) == -1
    assert call(N=0) == -2 and call(N=129) == -2 and call(N=-1) == -2
    assert call(B=1 << 16, H=1 << 15) == -2
    # ---- cd360_textgrad_act_bwd_bf16(x, dy, dx, rows, n, ld_x, ld_dy, ld_dx, kind, stream)
    act = lib.cd360_textgrad_act_bwd_bf16

    def call(x=a, dy=b, dx=c, rows=5, n=48, ldx=64, ldy=48, ldo=56, kind=0):
        return act(x, dy, dx, rows, n, ldx, ldy, ldo, kind, nul)

    assert call(x=nul) == -1 and call(dy=nul) == -1 and call(dx=nul) == -1
    assert call(rows=0) == -1 and call(n=0) == -1 and call(rows=-1) == -1 and call(kind=2) == -1 and call(kind=-1) == -1
    assert call(x=P(0x1000008)) == -1 and call(dy=P(0x2000002)) == -1 and call(dx=P(0x3000008)) == -1
    assert call(n=44, ldx=48) == -2
    for name in ("ldx", "ldy", "ldo"):
        assert call(**{name: 52}) == -2 and call(**{name: 40}) == -2, name
    # ---- cd360_textgrad_eot_scatter_bf16(d_pooled, ids, dx, B, N, D, ld_dp, ld_dx, stream)
    sc = lib.cd360_textgrad_eot_scatter_bf16

    def call(dp=a, ids=b, dx=c, B=3, N=77, D=128, ldp=128, ldx=128):
        return sc(dp, ids, dx, B, N, D, ldp, ldx, nul)

    assert call(dp=nul) == -1 and call(ids=nul) == -1 and call(dx=nul) == -1
    for name in ("B", "N", "D"):
        assert call(**{name: 0}) == -1 and call(**{name: -1}) == -1, name
    assert call(dp=P(0x1000008)) == -1 and call(dx=P(0x3000008)) == -1 and call(ids=P(0x2000004)) == -1
    assert call(D=132, ldp=136, ldx=136) == -2 and call(ldp=132) == -2 and call(ldx=132) == -2 and call(ldp=120) == -2 and call(ldx=64) == -2
    assert call(B=1 << 16, N=1 << 15) == -2
    # ---- cd360_textgrad_token_rows_f32(d_x0, ids, mod_ids (host), out, B, N, D, k, ld_dx, stream)
    tr = lib.cd360_textgrad_token_rows_f32
    mods = (ctypes.c_int64 * 3)(96, 97, 98)

    def call(dx=a, ids=b, mod=mods, out=c, B=3, N=77, D=128, k=2, ld=128):
        return tr(dx, ids, mod, out, B, N, D, k, ld, nul)

    assert call(dx=nul) == -1 and call(ids=nul) == -1 and call(mod=None) == -1 and call(out=nul) == -1
    for name in ("B", "N", "D"):
        assert call(**{name: 0}) == -1 and call(**{name: -1}) == -1, name
    assert call(dx=P(0x1000008)) == -1 and call(out=P(0x3000008)) == -1 and call(ids=P(0x2000004)) == -1
    assert call(k=0) == -2 and call(k=4) == -2 and call(k=-1) == -2
    assert call(D=132, ld=136) == -2 and call(ld=132) == -2 and call(ld=120) == -2
    assert call(B=1 << 16, N=1 << 15) == -2


def test_every_textgrad_entry_point_has_a_guarded_case():
    """Every function include/textgrad/cd360_textgrad.h declares is in a guarded case's `declares` (tests/test_textgrad_gpu.py runs them)
    and is typed in TEXTGRAD_SIGNATURES."""
    from cd360 import _textgrad
    untyped, unknown, uncovered = SC.check_guarded_cover(TG.HEADER, _textgrad.TEXTGRAD_SIGNATURES, TG.GUARDED)
    assert not untyped, untyped
    assert not unknown, unknown
    assert not uncovered, f"launching entry points without a guarded case: {sorted(uncovered)}"


def test_textgrad_kernels_are_recorded_without_scratch():
    """The record of text_backward.o: every kernel is there, with zero scratch and zero spills."""
    rec = json.load(open(os.path.join(SC.ROOT, "custom-diffusion360_amd", "lib", "obj", "text_backward.o.resources.json")))
    assert all(any(k in name for name in rec) for k in TG.KERNELS), sorted(rec)
    for name, r in rec.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)


# ================================================================================================ 2: masking, torch route
def _pair(tower, k, seed):
    modifier = "+".join(f"<new{i + 1}>" for i in range(k))
    return (TC.clip_pair if tower == "clip" else TC.openclip_pair)(modifier, seed=seed)


def _outputs(tower, emb, ids):
    if tower == "clip":
        return {"last_ln": emb(ids)}
    z = emb.encode_with_transformer(ids)
    return {"pen": z["penultimate"], "last_ln": z["last"], "pooled": z["pooled"]}


@pytest.mark.parametrize("kind", TG.PROMPTS)
@pytest.mark.parametrize("tower,k", [("clip", 3), ("openclip", 2)])
def test_train_tokens_gradient_is_the_references_masked_one(tower, k, kind):
    """fp32 SMALL towers on the CPU route: train_tokens, then the backward of a random linear functional of the outputs (CLIP: the final
    LayerNorm's output; OpenCLIP: penultimate, last and pooled together).  rows.grad equals the modifier rows of table.grad of the
    reference's formulation -- (1 - ind) * x.detach() + ind * x restated on the text_fp32 tower with the WHOLE table trainable -- at
    rel < 1e-5 (fp32 noise: the bound of this suite's check against HF), and that reference gradient is zero in every other row.  The
    token table of the marked embedder receives no gradient."""
    from cd360 import finetune
    emb, ref, _ = _pair(tower, k, seed=31)
    V, D = TC.SMALL["vocab"], TC.SMALL["width"]
    ids = TG.prompt_ids(kind, V, k, seed=32)
    counts = [int((ids == V + i).sum()) for i in range(k)]
    assert counts[-1] == {"once": 1, "twice-in-one": 2, "two-of-three": 2, "absent": 0}[kind]
    tr = finetune.train_tokens(TG.holder(emb))
    rows = list(tr.parameters())
    assert len(rows) == 1 and rows[0].shape == (k, D) and rows[0].requires_grad and rows[0].is_leaf and rows[0].dtype == torch.float32
    table = emb._tables()[0]
    assert not table.requires_grad and torch.equal(rows[0].detach(), table.detach()[V:])
    outs = _outputs(tower, emb, ids)
    cots = TG.cotangents({n: o.shape for n, o in outs.items()}, seed=33)
    TG.functional(outs, cots).backward()
    want = TG.reference_grad(ref, ids, k, cots)
    assert want.shape == (V + k, D) and not want[:V].any()  # no other token row receives anything
    got = rows[0].grad
    assert got is not None and table.grad is None
    for i, n in enumerate(counts):
        assert bool(want[V + i].any()) == (n > 0) and bool(got[i].any()) == (n > 0), (i, n)
    err = T32.rel(got, want[V:])
    print(f"{tower} {kind}: rows.grad against the masked reference, rel {err:.3e}")
    assert err < 1e-5


def test_openclip_legacy_and_last_layer_routes_carry_the_gradient_too():
    """layer="last" (not pooled) and legacy=True (final LayerNorm of the chosen layer, no pooled vector) on the torch route: rows.grad
    against the masked reference at rel < 1e-5."""
    from cd360 import finetune
    V, k = TC.SMALL["vocab"], 1
    ids = TG.prompt_ids("two-of-three", V, k, seed=41)
    for layer, legacy, name in (("last", False, "last_ln"), ("last", True, "last_ln"), ("penultimate", True, "pen_ln")):
        emb, ref, _ = TC.openclip_pair("<new1>", seed=42, layer=layer, always_return_pooled=False, legacy=legacy)
        tr = finetune.train_tokens(TG.holder(emb))
        out = emb(ids)
        cots = TG.cotangents({name: out.shape}, seed=43)
        TG.functional({name: out}, cots).backward()
        err = T32.rel(tr.rows[0].grad, TG.reference_grad(ref, ids, k, cots)[V:])
        print(f"openclip layer={layer} legacy={legacy}: rel {err:.3e}")
        assert err < 1e-5


# ================================================================================================ 3: routing, optimiser, checkpoint
def test_unmarked_embedders_and_no_grad_calls_behave_as_before():
    """An unmarked embedder with a trainable table still sends the gradient into the whole table (every token row a prompt uses); a marked
    one called under no_grad returns the bits it returned before it was marked and touches nothing; with grad enabled it first copies
    the rows into the table's last rows (the version counter moves)."""
    from cd360 import finetune
    V = TC.SMALL["vocab"]
    emb, _, _ = TC.clip_pair("<new1>", seed=51)
    ids = TG.prompt_ids("once", V, 1, seed=52)
    table = emb._tables()[0]
    assert table.requires_grad and "token_rows" not in emb.__dict__
    out = emb(ids)
    TG.functional({"last_ln": out}, TG.cotangents({"last_ln": out.shape}, seed=53)).backward()
    assert table.grad is not None and bool(table.grad[int(ids[0, 1])].any()) and bool(table.grad[V].any())
    table.grad = None
    with torch.no_grad():
        before = emb(ids)
    keys = set(emb.state_dict())
    tr = finetune.train_tokens(TG.holder(emb))
    assert set(emb.state_dict()) == keys and all(p is not tr.rows[0] for p in emb.parameters())  # the mark is no parameter of the embedder
    version = table._version
    with torch.no_grad():
        assert torch.equal(emb(ids), before) and table._version == version
        tr.rows[0].add_(1.0)
        assert torch.equal(emb(ids), before)  # the table is what a no_grad call reads
    out = emb(ids)
    assert out.requires_grad and table._version > version and torch.equal(table.detach()[V:], tr.rows[0].detach())
    assert not torch.equal(out.detach(), before)


def test_train_tokens_needs_a_modifier_and_skips_embedders_without():
    from cd360 import finetune
    with pytest.raises(ValueError, match="modifier"):
        finetune.train_tokens(TC.conditioner(modifier=None))
    with_mod, _, _ = TC.clip_pair("<new1>", seed=61)
    without, _, _ = TC.openclip_pair(None, seed=62)
    tr = finetune.train_tokens(TG.holder(without, with_mod))
    assert len(tr.rows) == 1 and tr.embedders == [with_mod] and "token_rows" not in without.__dict__


def test_rows_round_trip_through_the_delta_checkpoint_and_the_torch_optimiser():
    """The conditioner of the shipped config at small widths, on the CPU: train_tokens marks both prompt encoders; c = cond(batch) carries the
    tape; one MasterAdamW step (its torch fall-back: fp32 on the CPU) with max_grad_norm moves the rows; sync() writes them into the
    tables' last rows and no other row changes by a bit; embeds() -> delta_state_dict -> load_delta_embeddings on a fresh conditioner
    reproduces them bit for bit."""
    from cd360 import finetune
    cond = TC.conditioner("<new1>")
    V = TC.SMALL["vocab"]
    tr = finetune.train_tokens(cond)
    assert len(tr.rows) == 2 and [tuple(r.shape) for r in tr.rows] == [(1, TC.SMALL["width"])] * 2
    assert not any(p.requires_grad for p in cond.parameters())
    tables = [e._tables()[0].detach().clone() for e in cond.embedders[:2]]
    opt = finetune.MasterAdamW([{"params": list(tr.parameters()), "lr": 1e-2}], max_grad_norm=1.0)
    assert not opt.fused and len(opt.params) == 2
    c = cond(TC.batch(2, 1))
    assert c["crossattn"].requires_grad and c["vector"].requires_grad
    TG.functional(c, TG.cotangents({n: t.shape for n, t in c.items()}, seed=71)).backward()
    assert all(r.grad is not None and bool(r.grad.any()) for r in tr.rows)
    start = [r.detach().clone() for r in tr.rows]
    opt.step()
    assert all(not torch.equal(r.detach(), s) for r, s in zip(tr.rows, start))
    tr.sync()
    for e, t, r in zip(cond.embedders[:2], tables, tr.rows):
        now = e._tables()[0].detach()
        assert torch.equal(now[:V], t[:V]) and torch.equal(now[V:], r.detach())
    delta = finetune.delta_state_dict({}, embeds=tr.embeds())
    assert set(delta) == {"embed"} and all(torch.equal(a, r.detach()) and a is not r for a, r in zip(delta["embed"], tr.rows))
    fresh = TC.conditioner("<new1>")
    finetune.load_delta_embeddings(fresh, delta["embed"])
    for e, r in zip(fresh.embedders[:2], tr.rows):
        assert torch.equal(e._tables()[0].detach()[V:], r.detach())
