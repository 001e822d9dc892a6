"""What tests/test_textgrad_cpu.py and tests/test_textgrad_gpu.py share (plain helper module, like text_cases.py; no tests, no fixtures): the
names include/textgrad/cd360_textgrad.h adds, the prompts with modifier tokens, the reference's masked embedding restated on the
tests/text_fp32.py towers (the whole token table trainable, the gradient let through at the modifier positions only), and linear
functionals of a tower's outputs."""
import importlib
import os
import types

import torch

import sampler_cases as SC
import text_cases as TC
import text_fp32 as T32

HEADER = os.path.join("textgrad", "cd360_textgrad.h")
NEW = ["cd360_textgrad_causal_attn_bwd_bf16", "cd360_textgrad_act_bwd_bf16", "cd360_textgrad_eot_scatter_bf16", "cd360_textgrad_token_rows_f32"]
KERNELS = ("textgrad_causal_attn_bwd_kernel", "textgrad_act_bwd_kernel", "textgrad_eot_scatter_kernel", "textgrad_token_rows_kernel")
# the guarded cases of tests/test_textgrad_gpu.py::test_textgrad_entry_points_write_their_outputs_only: (id, entry points the case must reach)
GUARDED = [("attn-bwd-merged", ["cd360_textgrad_causal_attn_bwd_bf16"]), ("act-bwd-both-kinds", ["cd360_textgrad_act_bwd_bf16"]),
           ("eot-scatter", ["cd360_textgrad_eot_scatter_bf16"]), ("token-rows", ["cd360_textgrad_token_rows_f32"])]
# the build row this library adds behind the four older ones (__graft_entry__.LIBRARIES)
BUILD_ROW = ("libcd360_textgrad.so", "csrc_textgrad", ["text_backward.hip"], "_textgrad")


def older_libraries():
    """-> (tables, headers, loaded libraries) of EVERY library of sampler_cases.LIBRARIES: all of them are older than this one."""
    from cd360 import _lib
    mods = [importlib.import_module("cd360." + m) for _, m, _, _ in SC.LIBRARIES[1:]]
    tables = list(_lib.ABI.values()) + [getattr(mod, a) for mod, (_, _, a, _) in zip(mods, SC.LIBRARIES[1:])]
    inc = os.path.join(SC.ROOT, "include")
    headers = [os.path.join(d, f) for d, _, _, _ in SC.LIBRARIES for f in sorted(os.listdir(os.path.join(inc, d))) if f.endswith(".h")]
    return tables, headers, [_lib.load(check_symbols=True)] + [mod.load() for mod in mods]


# ------------------------------------------------------------------------------------------------ prompts
PROMPTS = ("once", "twice-in-one", "two-of-three", "absent")


def prompt_ids(kind, V, k, seed=0, B=3):
    """Three prompts of T32.token_ids with the modifier ids V .. V + k - 1 placed by hand.  `kind`: the LAST modifier (id V + k - 1, the one
    every prompt set is about) once / twice in one prompt / in two of three prompts / absent; the other modifiers, where k > 1, sit once each
    in prompt 1 (except for "absent": no modifier anywhere)."""
    ids = T32.token_ids(B, V, seed=seed)
    m = V + k - 1
    if kind == "once":
        ids[0, 2] = m
    elif kind == "twice-in-one":
        ids[0, 1] = ids[0, 6] = m
    elif kind == "two-of-three":
        ids[0, 2] = ids[B - 1, 1] = m
    else:
        assert kind == "absent"
        return ids
    for other in range(k - 1):
        ids[min(1, B - 1), 3 + other] = V + other
    return ids


# ------------------------------------------------------------------------------------------------ the reference's masked embedding
def masked(x, ids, modifier_ids):
    """(1 - indices) * x.detach() + indices * x (modules.py:499-511, 724-730): the token embeddings with the gradient let through at the
    modifier positions only."""
    ind = torch.isin(ids, torch.as_tensor(list(modifier_ids), device=ids.device))[..., None].to(x.dtype)
    return (1 - ind) * x.detach() + ind * x


def hf_masked(ref, ids, modifier_ids):
    """T32.HFTextTower.forward with the masked embedding -> {"last_ln"}."""
    tm = ref.transformer.text_model
    e = tm.embeddings
    x = masked(e.token_embedding(ids), ids, modifier_ids) + e.position_embedding(torch.arange(ids.shape[1], device=ids.device))[None]
    for b in tm.encoder.layers:
        x = ref.layer(b, x)
    return {"last_ln": tm.final_layer_norm(x)}


def openclip_masked(ref, ids, modifier_ids):
    """T32.OpenCLIPTextTower.forward with the masked embedding -> {"pen", "last_ln", "pen_ln", "pooled"}."""
    m = ref.model
    x = (masked(m.token_embedding(ids), ids, modifier_ids) + m.positional_embedding[:ids.shape[1]]).permute(1, 0, 2)
    N = x.shape[0]
    mask = torch.full((N, N), float("-inf"), dtype=x.dtype, device=x.device).triu_(1)
    blocks = m.transformer.resblocks
    out = {}
    for i, b in enumerate(blocks):
        if i == len(blocks) - 1:
            out["pen"] = x.permute(1, 0, 2)
        x = ref.layer(b, x, mask)
    out["last_ln"] = m.ln_final(x.permute(1, 0, 2))
    out["pen_ln"] = m.ln_final(out["pen"])
    out["pooled"] = out["last_ln"][torch.arange(ids.shape[0], device=ids.device), ids.argmax(dim=-1)] @ m.text_projection
    return out


def table_of(ref):
    return (ref.transformer.text_model.embeddings.token_embedding if hasattr(ref, "transformer") else ref.model.token_embedding).weight


def reference_grad(ref, ids, k, cots, dtype=torch.float32):
    """The gradient of sum_name <outputs[name], cots[name]> with respect to the WHOLE token table of a copy of `ref` cast to `dtype`, by
    torch autograd through the masked embedding -> [V + k, D] in fp32."""
    import copy
    ref = copy.deepcopy(ref).to(dtype)
    for p in ref.parameters():
        p.requires_grad = False
    tab = table_of(ref)
    tab.requires_grad = True
    V = tab.shape[0]
    outs = (hf_masked if hasattr(ref, "transformer") else openclip_masked)(ref, ids, range(V - k, V))
    total = sum((outs[name].float() * c.float()).sum() for name, c in cots.items())
    total.backward()
    return tab.grad.float()


def cotangents(shapes, seed):
    """{name: random cotangent, bf16-representable} for {name: shape}: a random linear functional of the outputs."""
    g = torch.Generator().manual_seed(seed)
    return {name: torch.randn(*shape, generator=g).bfloat16().float() for name, shape in shapes.items()}


def functional(outs, cots):
    return sum((outs[name].float() * c.to(outs[name].device)).sum() for name, c in cots.items())


def holder(*embedders):
    """What finetune.train_tokens reads of a conditioner, around embedders that stand alone."""
    return types.SimpleNamespace(embedders=list(embedders))


def offset_tables(sd, tok_key, pos_key, seed):
    """The tables of tests/test_text_gpu.py's offset-stream test: token values multiples of 1 / 2 in [-4, 4], every position row 64 with
    channel 5 at 512 (the token table is 0 there) -- the sum is exact in bf16, the stream carries an offset and a massive channel."""
    V, D = sd[tok_key].shape
    tok = torch.randint(-8, 9, (V, D), generator=torch.Generator().manual_seed(seed)).float() / 2
    tok[:, 5] = 0
    pos = torch.full_like(sd[pos_key], 64.0)
    pos[:, 5] = 512.0
    sd[tok_key], sd[pos_key] = tok, pos
    return sd
