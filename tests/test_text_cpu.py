"""The text conditioner without a GPU: the fourth library's header <=> table <=> exports and its host-side refusals, its resource record,
tests/text_fp32.py against HF transformers' own CLIP text model, the embedders' torch route against text_fp32, the conditioner's routing on
the shipped config's five embedders, the checkpoint layouts, the delta embeddings and the joint to the sampling job."""
import ctypes
import json
import os
import re

import pytest
import torch

import sampler_cases as SC
import text_cases as TC
import text_fp32 as T32


# ================================================================================================ 1: header, table, library
def test_text_header_matches_its_table_and_the_older_libraries_are_closed():
    """include/text/cd360_text.h <=> cd360._text.TEXT_SIGNATURES <=> libcd360_text.so (every `cd360_...(` word, comments included); no new
    name is in a table or a header of the three older libraries or exported by them; the binding reads no environment variable."""
    from cd360 import _edit, _lib, _optim, _text
    mismatch, in_tables, in_headers, mistyped, lib = SC.check_library_matches_table(TC.LIBRARY)
    assert not mismatch, mismatch
    assert not in_tables, in_tables
    assert not in_headers, in_headers
    assert not mistyped, mistyped
    for older in (_lib.load(check_symbols=True), _edit.load(), _optim.load()):
        for name in TC.NEW:
            assert not hasattr(older, name), name
    src = open(_text.__file__).read()
    assert "os.environ" not in src and "getenv" not in src
    hip = open(os.path.join(SC.ROOT, "custom-diffusion360_amd", "csrc_text", "text_encoder.hip")).read()
    assert "getenv" not in hip and "Synchronize" not in hip
    from cd360 import ops
    assert SC.header_constant(TC.HEADER, "CD360_TEXT_MAX_TOKENS") == ops.TEXT_MAX_TOKENS == _text.MAX_TOKENS == 128


def test_text_entry_points_refuse_bad_arguments_on_the_host():
    """Fabricated non-null pointers: every call below returns CD360_ERR_ARG (-1) or CD360_ERR_SHAPE (-2) before anything launches."""
    from cd360 import _text
    lib = _text.load()
    nul, P = ctypes.c_void_p(None), ctypes.c_void_p
    a, b, c, d, e = (P(0x1000000 * i) for i in range(1, 6))
    # ---- cd360_text_embed_bf16(ids, tok, pos, out, B, N, V, D, ld_out, stats, stream)
    emb = lib.cd360_text_embed_bf16

    def call(ids=a, tok=b, pos=c, out=d, B=2, N=77, V=96, D=128, ld=128, stats=e):
        return emb(ids, tok, pos, out, B, N, V, D, ld, stats, nul)

    for name in ("ids", "tok", "pos", "out"):
        assert call(**{name: nul}) == -1, name
    for name in ("B", "N", "V", "D"):
        assert call(**{name: 0}) == -1 and call(**{name: -3}) == -1, name
    assert call(tok=P(0x2000008)) == -1 and call(pos=P(0x3000002)) == -1 and call(out=P(0x4000008)) == -1
    assert call(ids=P(0x1000004)) == -1 and call(stats=P(0x5000004)) == -1
    assert call(D=132, ld=136) == -2 and call(ld=132) == -2 and call(ld=120) == -2
    assert call(B=1 << 16, N=1 << 15) == -2
    # ---- cd360_text_causal_attn_bf16(q, k, v, o, B, H, N, qs, ks, vs, os, scale, stream)
    att = lib.cd360_text_causal_attn_bf16
    S = lambda *v: (ctypes.c_int64 * 3)(*v)
    good = S(77 * 384, 64, 384)

    def call(q=a, k=b, v=c, o=d, B=2, H=2, N=77, qs=good, ks=good, vs=good, os_=S(77 * 128, 64, 128), scale=0.125):
        return att(q, k, v, o, B, H, N, qs, ks, vs, os_, scale, nul)

    for name in ("q", "k", "v", "o", "qs", "ks", "vs", "os_"):
        assert call(**{name: None if name.endswith("s") or name == "os_" else nul}) == -1, name
    assert call(B=0) == -1 and call(H=0) == -1 and call(H=-1) == -1
    assert call(q=P(0x1000008)) == -1 and call(k=P(0x2000002)) == -1 and call(v=P(0x3000008)) == -1 and call(o=P(0x4000004)) == -1
    assert call(scale=float("nan")) == -1 and call(scale=float("inf")) == -1
    assert call(N=0) == -2 and call(N=129) == -2 and call(N=-1) == -2
    for name in ("qs", "ks", "vs"):
        assert call(**{name: S(77 * 384, 64, 388)}) == -2 and call(**{name: S(77 * 384 + 4, 64, 384)}) == -2, name  # multiples of 4 only
        assert call(**{name: S(77 * 384, 64, -384)}) == -2, name
    assert call(os_=S(77 * 128, 64, 130)) == -2 and call(os_=S(77 * 128 + 2, 64, 128)) == -2
    assert call(B=1 << 16, H=1 << 15) == -2
    # ---- cd360_text_act_bf16(in, out, rows, n, ld_in, ld_out, kind, stream)
    act = lib.cd360_text_act_bf16

    def call(x=a, out=b, rows=5, n=48, ldi=64, ldo=48, kind=0):
        return act(x, out, rows, n, ldi, ldo, kind, nul)

    assert call(x=nul) == -1 and call(out=nul) == -1 and call(rows=0) == -1 and call(n=0) == -1 and call(rows=-1) == -1
    assert call(kind=2) == -1 and call(kind=-1) == -1
    assert call(x=P(0x1000008)) == -1 and call(out=P(0x2000002)) == -1
    assert call(n=44, ldi=48) == -2 and call(ldi=52) == -2 and call(ldo=52) == -2 and call(ldi=40) == -2 and call(ldo=40) == -2
    # ---- cd360_text_eot_pool_bf16(x, ids, out, B, N, D, ld_x, ld_out, stream)
    pool = lib.cd360_text_eot_pool_bf16

    def call(x=a, ids=b, out=c, B=3, N=77, D=128, ldx=128, ldo=128):
        return pool(x, ids, out, B, N, D, ldx, ldo, nul)

    assert call(x=nul) == -1 and call(ids=nul) == -1 and call(out=nul) == -1
    for name in ("B", "N", "D"):
        assert call(**{name: 0}) == -1, name
    assert call(x=P(0x1000008)) == -1 and call(out=P(0x3000008)) == -1 and call(ids=P(0x2000004)) == -1
    assert call(D=132, ldx=136, ldo=136) == -2 and call(ldx=132) == -2 and call(ldo=132) == -2 and call(ldx=120) == -2 and call(ldo=64) == -2
    assert call(B=1 << 16, N=1 << 15) == -2


def test_every_text_entry_point_has_a_guarded_case():
    """Every `int cd360_...(` include/text/cd360_text.h declares is in a guarded case's `declares` (tests/test_text_gpu.py runs them) and is
    typed in TEXT_SIGNATURES."""
    from cd360 import _text
    untyped, unknown, uncovered = SC.check_guarded_cover(TC.HEADER, _text.TEXT_SIGNATURES, TC.GUARDED)
    assert not untyped, untyped
    assert not unknown, unknown
    assert not uncovered, f"launching entry points without a guarded case: {sorted(uncovered)}"


def test_text_kernels_are_recorded_without_scratch():
    """build() leaves the new object's resource record where test_no_kernel_keeps_a_stack_object_in_scratch_memory reads it."""
    rec = json.load(open(os.path.join(SC.ROOT, "custom-diffusion360_amd", "lib", "obj", "text_encoder.o.resources.json")))
    assert all(any(k in name for name in rec) for k in TC.KERNELS), sorted(rec)
    for name, r in rec.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)


def test_importing_sgm_modules_loads_no_library():
    """`import sgm.modules` in a fresh interpreter imports no encoder module and dlopens nothing; the name resolves on first use."""
    import subprocess
    import sys
    code = ("import sys; sys.path[:0] = %r\n"
            "import sgm.modules\n"
            "assert 'sgm.modules.encoders.modules' not in sys.modules and 'cd360._text' not in sys.modules\n"
            "maps = open('/proc/self/maps').read()\n"
            "assert 'libcd360' not in maps, 'a cd360 library was loaded'\n"
            "from sgm.util import get_obj_from_str\n"
            "assert get_obj_from_str('sgm.modules.GeneralConditioner').__name__ == 'GeneralConditioner'\n"
            "assert 'libcd360' not in open('/proc/self/maps').read()\n" % [os.path.join(SC.ROOT, "custom-diffusion360_amd")])
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


# ================================================================================================ 2: the fp32 reference against HF's own model
def test_text_fp32_hf_tower_equals_transformers_clip_text_model():
    """tests/text_fp32.py's HF tower against transformers.CLIPTextModel built from a CLIPTextConfig (never from a name), same random weights
    and ids: last_hidden_state at rel < 1e-5.  The model's key names are ours without `transformer.` and, depending on the transformers
    version, without `text_model.`; `position_ids` is the model's own buffer."""
    tr = pytest.importorskip("transformers")
    V, D, H, L, MLP = TC.SMALL["vocab"], TC.SMALL["width"], TC.SMALL["heads"], TC.SMALL["layers"], TC.SMALL["mlp"]
    cfg = tr.CLIPTextConfig(vocab_size=V, hidden_size=D, intermediate_size=MLP, num_hidden_layers=L, num_attention_heads=H,
                            max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, pad_token_id=0, bos_token_id=V - 2,
                            eos_token_id=V - 1, projection_dim=D)
    model = tr.CLIPTextModel(cfg).eval()
    ours = T32.HFTextTower(V, D, H, L, MLP).eval()
    sd = T32.synth_weights(ours, seed=5)
    ours.load_state_dict(sd, strict=True)
    theirs = model.state_dict()
    mapped = {}
    for k, v in sd.items():
        short = k[len("transformer."):]
        name = short if short in theirs else short[len("text_model."):]
        assert name in theirs, (k, sorted(theirs)[:6])
        mapped[name] = v
    left = [k for k in theirs if k not in mapped and not k.endswith("position_ids")]
    assert not left, left
    model.load_state_dict(mapped, strict=False)
    ids = T32.token_ids(3, V, seed=1)
    with torch.no_grad():
        want = model(input_ids=ids).last_hidden_state
        got = ours(ids)
    err = T32.rel(got, want)
    print("HF tower against transformers", tr.__version__, "rel", err)
    assert err < 1e-5


# ================================================================================================ 3: the module's torch route
@pytest.mark.parametrize("modifier", [None, "<new1>", "<new1>+<new2>"])
def test_clip_embedder_torch_route_equals_text_fp32(modifier):
    """FrozenCLIPEmbedder on the CPU in fp32 against text_fp32's HF tower on the same state dict: final_layer_norm of the last layer whatever
    `layer` / `layer_idx` say; with modifier tokens the table has grown by their count, their ids are V, V + 1 and prompts that hold them
    encode like the reference tower on the grown table."""
    emb, ref, sd = TC.clip_pair(modifier, seed=11)
    V = TC.SMALL["vocab"]
    k = 0 if modifier is None else modifier.count("+") + 1
    assert emb.transformer.text_model.embeddings.token_embedding.weight.shape[0] == V + k
    if k:
        assert emb.modifier_token_id == list(range(V, V + k)) and emb.modifier_token == modifier.split("+")
        assert emb.transformer.text_model.embeddings.token_embedding.weight.requires_grad
    ids = T32.token_ids(3, V, seed=2, modifier=(V + k - 1, 4) if k else None)
    with torch.no_grad():
        got, want = emb(ids), ref(ids)
    assert got.shape == (3, 77, TC.SMALL["width"]) and got.dtype == torch.float32
    assert T32.rel(got, want) < 1e-5
    other = TC.clip_embedder(modifier, layer="last", layer_idx=None)
    other.load_state_dict(sd, strict=True)
    with torch.no_grad():
        assert torch.equal(other(ids), got)  # `layer: hidden, layer_idx: 11` selects nothing
    with pytest.raises(AssertionError):
        TC.clip_embedder(None, layer="hidden", layer_idx=None)
    with pytest.raises(ValueError, match="tokenizer"):
        emb(["a photo of a <new1> cat"])
    with pytest.raises(ValueError):
        emb(torch.full((1, 77), V + k, dtype=torch.int64))  # an id behind the table: refused on the host
    with pytest.raises(ValueError):
        emb(torch.zeros(1, 76, dtype=torch.int64))
    tok = TC.clip_embedder(modifier, tokenizer=lambda texts: ids[:len(texts)])
    tok.load_state_dict(sd, strict=True)
    with torch.no_grad():
        assert torch.equal(tok(["a", "b", "c"]), got)


@pytest.mark.parametrize("modifier", [None, "<new1>"])
def test_openclip_embedder_torch_route_equals_text_fp32(modifier):
    """FrozenOpenCLIPEmbedder on the CPU in fp32 against text_fp32's OpenCLIP tower (nn.MultiheadAttention): `penultimate` is the input of the
    last block without ln_final, `last` is ln_final of the output, `pooled` the argmax row of `last` times text_projection -- with a modifier
    id above EOT's placed before EOT that row is the MODIFIER's, and differs from the EOT row's projection (the reference's quirk, kept)."""
    V, D = TC.SMALL["vocab"], TC.SMALL["width"]
    k = 0 if modifier is None else 1
    ids = T32.token_ids(3, V, seed=3, modifier=(V, 2) if k else None)
    ref, sd = None, None
    for layer in ("penultimate", "last"):
        emb, ref, sd = TC.openclip_pair(modifier, seed=13, layer=layer, always_return_pooled=True, legacy=False)
        with torch.no_grad():
            z, pooled = emb(ids)
            want = ref(ids)
        assert z.shape == (3, 77, D) and pooled.shape == (3, TC.SMALL["proj"])
        assert T32.rel(z, want[layer]) < 1e-5 and T32.rel(pooled, want["pooled"]) < 1e-5
        plain = TC.openclip_embedder(modifier, layer=layer, always_return_pooled=False, legacy=False)
        plain.load_state_dict(sd, strict=True)
        with torch.no_grad():
            assert torch.equal(plain(ids), z)
    if k:
        assert bool((ids.argmax(-1) == 2).all()) and bool((ids[:, 2] == V).all())
        eot_rows = (ids == V - 1).int().argmax(-1)
        at_eot = want["last"][torch.arange(3), eot_rows] @ sd["model.text_projection"]
        assert T32.rel(want["pooled"], at_eot) > 1e-2  # pooled at the modifier, not at EOT
    legacy = TC.openclip_embedder(modifier, layer="penultimate", always_return_pooled=False, legacy=True)
    legacy.load_state_dict(sd, strict=True)
    with torch.no_grad():
        got = legacy(ids)
    lnf = torch.nn.functional.layer_norm(want["penultimate"], (D,), sd["model.ln_final.weight"], sd["model.ln_final.bias"], 1e-5)
    assert T32.rel(got, lnf) < 1e-5
    from sgm.modules.encoders.modules import FrozenOpenCLIPEmbedder2
    two = FrozenOpenCLIPEmbedder2(layer="last", legacy=False, always_return_pooled=True, **TC.openclip_arch())
    assert two.modifier_token is None and set(two.state_dict()) == set(TC.openclip_embedder(None).state_dict())
    with pytest.raises(ValueError, match="tokenizer"):
        two(["a prompt"])


def test_modifier_rows_start_as_copies_of_the_reference_rows():
    """The appended rows are copies of rows 42170 / 47629 / 43514 (last new token first); min(row, V - 1) only for a smaller table."""
    from sgm.modules.encoders import modules as M
    e = torch.nn.Embedding(47700, 8)
    old = e.weight.detach().clone()
    assert M._append_modifier_rows(e, 2) == [47700, 47701]
    assert torch.equal(e.weight[47701], old[42170]) and torch.equal(e.weight[47700], old[47629]) and torch.equal(e.weight[:47700], old)
    e = torch.nn.Embedding(96, 8)
    old = e.weight.detach().clone()
    assert M._append_modifier_rows(e, 3) == [96, 97, 98] and all(torch.equal(e.weight[96 + i], old[95]) for i in range(3))
    with pytest.raises(ValueError):
        TC.openclip_embedder("<a>+<b>+<c>")
    with pytest.raises(ValueError):
        TC.clip_embedder("<a>+<b>+<c>+<d>")


# ================================================================================================ 4: checkpoint layouts
def test_state_dict_keys_are_the_checkpoint_layouts():
    """state_dict() keys are exactly the SDXL checkpoint's names for both embedders; load_state_dict(strict=True) accepts the layout with and
    without `position_ids`."""
    L = TC.SMALL["layers"]
    clip = TC.clip_embedder(None)
    p = "transformer.text_model."
    want = {p + "embeddings.token_embedding.weight", p + "embeddings.position_embedding.weight", p + "final_layer_norm.weight", p + "final_layer_norm.bias"}
    for i in range(L):
        q = f"{p}encoder.layers.{i}."
        want |= {q + f"{n}.{w}" for n in ("layer_norm1", "layer_norm2", "self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj",
                                          "self_attn.out_proj", "mlp.fc1", "mlp.fc2") for w in ("weight", "bias")}
    assert set(clip.state_dict()) == want
    sd = {k: v.clone() for k, v in clip.state_dict().items()}
    clip.load_state_dict(sd, strict=True)
    sd[p + "embeddings.position_ids"] = torch.arange(77)[None]
    clip.load_state_dict(sd, strict=True)
    assert p + "embeddings.position_ids" in sd  # (the caller's dict is its own business: only the copy torch hands the hook is edited)
    oc = TC.openclip_embedder(None)
    want = {"model.token_embedding.weight", "model.positional_embedding", "model.ln_final.weight", "model.ln_final.bias", "model.text_projection",
            "model.logit_scale"}
    for i in range(L):
        q = f"model.transformer.resblocks.{i}."
        want |= {q + "attn.in_proj_weight", q + "attn.in_proj_bias"}
        want |= {q + f"{n}.{w}" for n in ("ln_1", "ln_2", "attn.out_proj", "mlp.c_fc", "mlp.c_proj") for w in ("weight", "bias")}
    assert set(oc.state_dict()) == want
    oc.load_state_dict({k: v.clone() for k, v in oc.state_dict().items()}, strict=True)
    # a checkpoint table without the modifier rows (the SDXL checkpoint's) loads into the first rows of a grown table; the caller's dict stays
    for grown, plain, key in ((TC.clip_embedder("<new1>+<new2>"), clip, p + "embeddings.token_embedding.weight"),
                              (TC.openclip_embedder("<new1>"), oc, "model.token_embedding.weight")):
        base = {k: v.clone() + 1 for k, v in plain.state_dict().items()}
        kept, V = grown._tables()[0].detach().clone(), base[key].shape[0]
        grown.load_state_dict(base, strict=True)
        assert base[key].shape[0] == V and torch.equal(grown._tables()[0][:V], base[key]) and torch.equal(grown._tables()[0][V:], kept[V:])
        with pytest.raises(RuntimeError):
            grown.load_state_dict({**base, key: base[key][:V - 1]}, strict=True)  # any other row count is the size mismatch it was


# ================================================================================================ 5: the conditioner
def test_general_conditioner_routes_the_shipped_embedders():
    """configs/train_co3d_concept.yaml:56-96's five emb_models (tests/golden/conditioner_emb_models.json: the settings alone) at small widths,
    resolved through sgm.modules.GeneralConditioner: crossattn [., 77, D1 + D2], vector [., D2 + 3 * 512]; target rows before `_ref` rows;
    force_ref_zero_embeddings=True encodes input_keys[0] only; sample.py:151-161's call returns an all-zero uc; ucg_rate is restored."""
    cond = TC.conditioner()
    D1, D2 = TC.SMALL["width"], TC.SMALL["width"]
    assert [type(e).__name__ for e in cond.embedders] == ["FrozenCLIPEmbedder", "FrozenOpenCLIPEmbedder"] + ["ConcatTimestepEmbedderND"] * 3
    assert cond.embedders[0].input_keys == ["txt", "txt_ref"] and cond.embedders[0].input_key is None and cond.embedders[0].is_trainable is False
    assert cond.embedders[0].legacy_ucg_val is None and cond.OUTPUT_DIM2KEYS[3] == "crossattn" and cond.KEY2CATDIM["crossattn"] == 2
    batch = TC.batch(2, 4)
    with torch.no_grad():
        out = cond(batch)
        only = cond({k: v for k, v in batch.items() if not k.endswith("_ref")}, force_ref_zero_embeddings=True)
    assert out["crossattn"].shape == (2 + 4, 77, D1 + D2) and out["vector"].shape == (2 + 4, TC.SMALL["proj"] + 3 * 512)
    assert set(out) == {"crossattn", "vector"}
    assert only["crossattn"].shape == (2, 77, D1 + D2) and only["vector"].shape == (2, TC.SMALL["proj"] + 3 * 512)
    assert torch.equal(out["crossattn"][:2], only["crossattn"]) and torch.equal(out["vector"][:2], only["vector"])  # target rows first
    with torch.no_grad():
        refs = cond({k[:-4]: v for k, v in batch.items() if k.endswith("_ref")}, force_ref_zero_embeddings=True)
    assert torch.equal(out["crossattn"][2:], refs["crossattn"]) and torch.equal(out["vector"][2:], refs["vector"])  # ... `_ref` rows after
    with torch.no_grad():
        z0 = cond.embedders[0](batch["txt"])
        z1, pooled = cond.embedders[1](batch["txt"])
    assert torch.equal(only["crossattn"], torch.cat([z0, z1], 2))
    sizes = [cond.embedders[i](batch[k]) for i, k in ((2, "original_size_as_tuple"), (3, "crop_coords_top_left"), (4, "target_size_as_tuple"))]
    assert torch.equal(only["vector"], torch.cat([pooled] + sizes, 1))
    # ---- sample.py:151-161, unchanged
    for e, r in zip(cond.embedders, (0.1, 0.2, 0.0, 0.3, 0.0)):
        e.ucg_rate = r
    keys = [e.input_keys for e in cond.embedders]
    with torch.no_grad():
        c, uc = cond.get_unconditional_conditioning(batch, force_uc_zero_embeddings=keys if len(cond.embedders) > 0 else [],
                                                    force_ref_zero_embeddings=True)
    assert [e.ucg_rate for e in cond.embedders] == [0.1, 0.2, 0.0, 0.3, 0.0]
    assert torch.equal(c["crossattn"], only["crossattn"]) and torch.equal(c["vector"], only["vector"])  # ucg_rate was 0 inside
    assert uc["crossattn"].shape == c["crossattn"].shape and uc["vector"].shape == c["vector"].shape
    assert not uc["crossattn"].any() and not uc["vector"].any()
    with pytest.raises(KeyError):
        cond.get_unconditional_conditioning({})
    assert [e.ucg_rate for e in cond.embedders] == [0.1, 0.2, 0.0, 0.3, 0.0]  # restored when a pass raises, too


def test_concat_timestep_embedder_sits_on_timestep_embedding():
    from sgm.modules.diffusionmodules.util import timestep_embedding
    from sgm.modules.encoders.modules import ConcatTimestepEmbedderND
    e = ConcatTimestepEmbedderND(256)
    x = torch.tensor([[512.0, 384.0], [0.0, 17.0], [1024.0, 1.0]])
    got = e(x)
    assert got.shape == (3, 512) and e.modifier_token is None and e.outdim == 256
    assert torch.equal(got, torch.cat([timestep_embedding(x[:, 0], 256), timestep_embedding(x[:, 1], 256)], 1))
    assert torch.equal(e(x[:, 0]), timestep_embedding(x[:, 0], 256))


# ================================================================================================ 6: delta embeddings, the joint to the job
def test_load_delta_embeddings_reproduces_the_concatenation():
    """cd360.finetune.load_delta_embeddings against torch.cat([table without the modifier row, trained row]) (sgm/util.py:216-230), for
    embedders that hold the row already (overwrite) and embedders built without modifier_token (append); the input is untouched."""
    from cd360 import finetune
    for modifier in ("<new1>", None):
        cond = TC.conditioner(modifier=modifier)
        V, D = TC.SMALL["vocab"], TC.SMALL["width"]
        tables = [cond.embedders[i]._tables()[0].detach().clone()[:V] for i in range(2)]
        embed = [torch.randn(1, D, generator=torch.Generator().manual_seed(i)) for i in range(2)]
        kept = [e.clone() for e in embed]
        sd_delta = {"embed": embed, "other": torch.zeros(1)}
        finetune.load_delta_embeddings(cond, sd_delta["embed"])
        assert set(sd_delta) == {"embed", "other"} and all(torch.equal(a, b) for a, b in zip(sd_delta["embed"], kept))
        for i in range(2):
            got = cond.embedders[i]._tables()[0]
            assert torch.equal(got.detach(), torch.cat([tables[i], embed[i]], 0)) and cond.embedders[i].modifier_token_id == [V]
        ids = T32.token_ids(1, V, seed=4, modifier=(V, 3))
        with torch.no_grad():
            assert torch.isfinite(cond.embedders[0](ids)).all()
    with pytest.raises(ValueError):
        finetune.load_delta_embeddings(cond, [torch.zeros(1, D + 8), torch.zeros(1, D)])
    with pytest.raises(ValueError):
        finetune.load_delta_embeddings(TC.conditioner(modifier="<new1>"), [torch.zeros(2, D), torch.zeros(2, D)])


def test_sampler_rows_are_the_guiders_own():
    """cd360.text.sampler_rows: [uc | uc | c] for three branches, [uc | c] for two -- and what job.Sampler's _cond_batch makes of them is
    what the guider makes of (c, uc) directly."""
    from cd360 import sampler as S
    from cd360 import text
    g = torch.Generator().manual_seed(0)
    c = {"crossattn": torch.randn(2, 77, 16, generator=g), "vector": torch.randn(2, 24, generator=g)}
    uc = {k: torch.zeros_like(v) for k, v in c.items()}
    ctx, y = text.sampler_rows(c, uc, 3, dtype=torch.float32)
    assert torch.equal(ctx, torch.cat([uc["crossattn"], uc["crossattn"], c["crossattn"]])) and torch.equal(y, torch.cat([uc["vector"]] * 2 + [c["vector"]]))
    ctx, y = text.sampler_rows(c, uc, 2, dtype=torch.float32)
    assert torch.equal(ctx, torch.cat([uc["crossattn"], c["crossattn"]])) and torch.equal(y, torch.cat([uc["vector"], c["vector"]]))
    assert text.sampler_rows(c, uc, 2)[0].dtype == torch.bfloat16
    with pytest.raises(ValueError):
        text.sampler_rows(c, uc, 1)
    with pytest.raises(ValueError):
        text.sampler_rows(c, {"crossattn": uc["crossattn"]}, 3)
