"""The conditioner (reference sgm/modules/encoders/modules.py): GeneralConditioner and the embedders the shipped config names
(configs/train_co3d_concept.yaml:56-96) -- FrozenCLIPEmbedder (CLIP ViT-L/14's text model), FrozenOpenCLIPEmbedder / FrozenOpenCLIPEmbedder2
(OpenCLIP ViT-bigG-14's text tower) and ConcatTimestepEmbedderND.  Forward only; inference.

The two prompt encoders are plain nn.Module holders of nn.Parameters under the checkpoint's own names (the SDXL layout: HF
transformers 4.x for the first, open_clip for the second), with no dependency on transformers or open_clip, and nothing here looks for a
file: weights arrive through load_state_dict.  Two routes, as everywhere in this package:

  bf16 parameters on the GPU, no tape    the HIP route.  Per layer six launches: q|k|v GEMM with LayerNorm 1 folded in front
                                         (ops.pack_ln_linear; CLIP-L's three projections packed into one weight) -> causal attention on
                                         the merged projection in place (ops.causal_attention) -> out-proj GEMM + bias + residual + row
                                         statistics -> FC1 GEMM with LayerNorm 2 folded -> activation (ops.text_activation) -> FC2 GEMM +
                                         bias + residual + row statistics.  In front: ops.text_embed (with the first statistics); behind:
                                         ops.add_layernorm for the final LayerNorm, ops.eot_pool + one GEMM for the pooled vector.
  anything else (CPU, fp32, ...)         a plain torch restatement of the same computation, in the parameters' dtype.

A HIP-route embedder under a tape (grad enabled and a parameter that requires grad -- with `modifier_token` the token table does) raises
NotImplementedError: there is no backward for the tower's own parameters.  The one backward that exists is opt-in: an embedder that
cd360.finetune.train_tokens marked (`token_rows`: its k modifier rows as a leaf parameter of their own, the table itself frozen) runs, with
grad enabled, through cd360.grad.TextTowerFn on the HIP route (the same forward launches; the backward on libcd360_textgrad.so) and embeds
from torch.cat([table[:-k].detach(), rows]) on the torch route.  Packed weights go through cd360.derived.derived and follow its one
invalidation rule.

Text input: no tokenizer vocabulary ships with this package.  `text` is an int64 tensor [B, max_length] of token ids, or a list of strings
together with a `tokenizer=` callable (constructor argument) that returns such a tensor."""
from __future__ import annotations

from contextlib import nullcontext
from typing import Dict, List, Optional, Union

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from cd360 import ops
from cd360.derived import derived

from ...util import count_params, instantiate_from_config
from ..diffusionmodules.util import timestep_embedding

LN_EPS = 1e-5  # both towers (CLIPTextConfig.layer_norm_eps, open_clip's LayerNorm)
# rows the reference copies into the appended modifier rows: the last token, the one before it, the one before that (modules.py:417-431,678-691)
MODIFIER_INIT_ROWS = (42170, 47629, 43514)
NO_TAPE = "the text-encoder HIP modules have no backward; call them under torch.no_grad() (forward only)"


def disabled_train(self, mode=True):
    """Installed as `.train` of an embedder that is not trainable: train / eval mode does not change any more."""
    return self


def expand_dims_like(x, y):
    while x.dim() != y.dim():
        x = x.unsqueeze(-1)
    return x


class AbstractEmbModel(nn.Module):
    def __init__(self):
        super().__init__()
        self._is_trainable = None
        self._ucg_rate = None
        self._input_key = None

    @property
    def is_trainable(self) -> bool:
        return self._is_trainable

    @is_trainable.setter
    def is_trainable(self, value: bool):
        self._is_trainable = value

    @is_trainable.deleter
    def is_trainable(self):
        del self._is_trainable

    @property
    def ucg_rate(self) -> Union[float, torch.Tensor]:
        return self._ucg_rate

    @ucg_rate.setter
    def ucg_rate(self, value: Union[float, torch.Tensor]):
        self._ucg_rate = value

    @ucg_rate.deleter
    def ucg_rate(self):
        del self._ucg_rate

    @property
    def input_key(self) -> str:
        return self._input_key

    @input_key.setter
    def input_key(self, value: str):
        self._input_key = value

    @input_key.deleter
    def input_key(self):
        del self._input_key


class GeneralConditioner(nn.Module):
    """modules.py:73-230.  Every embedder's output is routed by its rank (OUTPUT_DIM2KEYS) and concatenated along KEY2CATDIM.  An embedder
    configured with `input_keys: a,a_ref` encodes both keys: the target's rows come first in every output, the `_ref` rows after them
    (force_ref_zero_embeddings=True: only input_keys[0] is encoded and there are no `_ref` rows).  `force_zero_embeddings` is matched
    against `input_key` (a string) and `input_keys` (the list itself, as sample.py:151-161 passes them)."""

    OUTPUT_DIM2KEYS = {2: "vector", 3: "crossattn", 4: "concat", 5: "concat"}
    KEY2CATDIM = {"vector": 1, "crossattn": 2, "concat": 1}

    def __init__(self, emb_models):
        super().__init__()
        embedders = []
        for n, cfg in enumerate(emb_models):
            embedder = instantiate_from_config(cfg)
            assert isinstance(embedder, AbstractEmbModel), f"embedder model {embedder.__class__.__name__} has to inherit from AbstractEmbModel"
            embedder.is_trainable = cfg.get("is_trainable", False)
            embedder.ucg_rate = cfg.get("ucg_rate", 0.0)
            if not embedder.is_trainable:
                embedder.train = disabled_train
                for p in embedder.parameters():
                    p.requires_grad = False
                embedder.eval()
            print(f"Initialized embedder #{n}: {embedder.__class__.__name__} with {count_params(embedder, False)} params. "
                  f"Trainable: {embedder.is_trainable}")
            if "input_key" in cfg:
                embedder.input_key = cfg["input_key"]
            elif "input_keys" in cfg:
                embedder.input_keys = cfg["input_keys"].split(",")
            else:
                raise KeyError(f"need either 'input_key' or 'input_keys' for embedder {embedder.__class__.__name__}")
            embedder.legacy_ucg_val = cfg.get("legacy_ucg_value", None)
            if embedder.legacy_ucg_val is not None:
                embedder.ucg_prng = np.random.RandomState()
            embedders.append(embedder)
        self.embedders = nn.ModuleList(embedders)

    def possibly_get_ucg_val(self, embedder: AbstractEmbModel, batch: Dict) -> Dict:
        assert embedder.legacy_ucg_val is not None
        p, val = embedder.ucg_rate, embedder.legacy_ucg_val
        for i in range(len(batch[embedder.input_key])):
            if embedder.ucg_prng.choice(2, p=[1 - p, p]):
                batch[embedder.input_key][i] = val
        return batch

    @staticmethod
    def _single_key(embedder) -> bool:
        return getattr(embedder, "input_key", None) is not None

    def forward(self, batch: Dict, force_zero_embeddings: Optional[List] = None, force_ref_zero_embeddings: bool = False) -> Dict:
        output = {}
        force_zero_embeddings = [] if force_zero_embeddings is None else force_zero_embeddings
        for embedder in self.embedders:
            single, multi = self._single_key(embedder), hasattr(embedder, "input_keys")
            tape = embedder.is_trainable or getattr(embedder, "modifier_token", None) is not None
            with (nullcontext() if tape else torch.no_grad()):
                if single:
                    if embedder.legacy_ucg_val is not None:
                        batch = self.possibly_get_ucg_val(embedder, batch)
                    emb_out = embedder(batch[embedder.input_key])
                elif multi:
                    if force_ref_zero_embeddings:
                        emb_out = embedder(batch[embedder.input_keys[0]])
                    else:
                        per_key = [embedder(batch[k]) for k in embedder.input_keys]
                        if isinstance(per_key[0], tuple):
                            emb_out = [torch.cat([e[i] for e in per_key]) for i in range(2)]
                        else:
                            emb_out = torch.cat(per_key)
                else:
                    raise KeyError(f"embedder {embedder.__class__.__name__} has neither input_key nor input_keys")
            assert isinstance(emb_out, (torch.Tensor, list, tuple)), f"encoder outputs must be tensors or a sequence, but got {type(emb_out)}"
            if not isinstance(emb_out, (list, tuple)):
                emb_out = [emb_out]
            for emb in emb_out:
                key = self.OUTPUT_DIM2KEYS[emb.dim()]
                if embedder.ucg_rate > 0.0 and embedder.legacy_ucg_val is None:
                    keep = torch.bernoulli((1.0 - embedder.ucg_rate) * torch.ones(emb.shape[0], device=emb.device))
                    emb = expand_dims_like(keep, emb) * emb
                if (single and embedder.input_key in force_zero_embeddings) or (multi and embedder.input_keys in force_zero_embeddings):
                    emb = torch.zeros_like(emb)
                if multi:
                    catdim = 1 if "pose" in embedder.input_keys else self.KEY2CATDIM[key]
                    parts = {key: emb} if force_ref_zero_embeddings else dict(zip((key, key + "_ref"), emb.chunk(2)))
                else:
                    catdim = 1 if ("pose" in embedder.input_key and emb.size(1) != 77) else self.KEY2CATDIM[key]
                    parts = {key: emb}
                fresh = key not in output
                for k, part in parts.items():
                    output[k] = part if fresh else torch.cat((output[k], part), catdim)
        for key in self.OUTPUT_DIM2KEYS.values():
            if key + "_ref" in output and not force_ref_zero_embeddings:
                output[key] = torch.cat([output[key], output.pop(key + "_ref")], 0)
        return output

    def get_unconditional_conditioning(self, batch_c: Dict, batch_uc: Optional[Dict] = None, force_uc_zero_embeddings: Optional[List] = None,
                                       force_ref_zero_embeddings: bool = False):
        """(c, uc) with every ucg_rate held at 0 for the two passes and restored afterwards (also when a pass raises)."""
        force_uc_zero_embeddings = [] if force_uc_zero_embeddings is None else force_uc_zero_embeddings
        rates = [e.ucg_rate for e in self.embedders]
        try:
            for e in self.embedders:
                e.ucg_rate = 0.0
            c = self(batch_c, force_ref_zero_embeddings=force_ref_zero_embeddings)
            uc = self(batch_c if batch_uc is None else batch_uc, force_uc_zero_embeddings, force_ref_zero_embeddings)
        finally:
            for e, r in zip(self.embedders, rates):
                e.ucg_rate = r
        return c, uc


# ------------------------------------------------------------------------------------------------ what both towers share
def _modifier_list(modifier_token, limit: int):
    if modifier_token is None:
        return None
    toks = modifier_token.split("+") if "+" in modifier_token else [modifier_token]
    if not 1 <= len(toks) <= limit:
        raise ValueError(f"modifier_token names {len(toks)} tokens; the reference initialises at most {limit}")
    return toks


def _append_modifier_rows(emb: nn.Embedding, count: int) -> List[int]:
    """Append `count` rows to the token table; -> their ids V, V + 1, ...  The LAST new row is a copy of row 42170, the one before it of
    47629, the one before that of 43514 (min(row, V - 1) only where the table is smaller than that: the small tables of the tests)."""
    old = emb.weight.data
    V = old.shape[0]
    new = torch.cat([old, old.new_zeros(count, old.shape[1])], 0)
    for back in range(count):
        new[V + count - 1 - back] = old[min(MODIFIER_INIT_ROWS[back], V - 1)]
    emb.weight = nn.Parameter(new)
    emb.num_embeddings = V + count
    return list(range(V, V + count))


class _Holder(nn.Module):
    """A named container of sub-modules and parameters; the computation lives in the embedder."""


class _Layer:
    """One transformer layer's tensors under the names the routes below use, whichever checkpoint layout holds them."""

    __slots__ = ("owner", "ln1", "ln2", "qkv", "out", "fc1", "fc2")

    def __init__(self, owner, ln1, ln2, qkv, out, fc1, fc2):
        self.owner, self.ln1, self.ln2, self.qkv, self.out, self.fc1, self.fc2 = owner, ln1, ln2, qkv, out, fc1, fc2

    def merged_qkv(self):
        """(weight [3D, D], bias [3D]) of the q|k|v projection: `qkv` holds one merged tensor each (open_clip) or three (HF)."""
        ws, bs = self.qkv
        return (ws[0], bs[0]) if len(ws) == 1 else (torch.cat(list(ws), 0), torch.cat(list(bs), 0))


def _act_torch(x, kind):
    return x * torch.sigmoid(1.702 * x) if kind == ops.ACT_QUICK_GELU else F.gelu(x)


def _layer_torch(x, L: _Layer, heads: int, kind: int):
    """x [B, N, D] -> the layer's output, in x's dtype: pre-LayerNorm attention under the causal mask, then the MLP."""
    B, N, D = x.shape
    hd = D // heads
    w, b = L.merged_qkv()
    qkv = F.linear(F.layer_norm(x, (D,), L.ln1.weight, L.ln1.bias, LN_EPS), w, b)
    q, k, v = (t.reshape(B, N, heads, hd).transpose(1, 2) for t in qkv.chunk(3, dim=-1))
    s = (q * hd ** -0.5) @ k.transpose(-1, -2)
    hidden = torch.ones(N, N, dtype=torch.bool, device=x.device).triu(1)
    p = torch.softmax(s.float().masked_fill(hidden, float("-inf")), dim=-1).to(x.dtype)
    o = (p @ v).transpose(1, 2).reshape(B, N, D)
    x = x + F.linear(o, L.out.weight, L.out.bias)
    h = F.linear(F.layer_norm(x, (D,), L.ln2.weight, L.ln2.bias, LN_EPS), L.fc1.weight, L.fc1.bias)
    return x + F.linear(_act_torch(h, kind), L.fc2.weight, L.fc2.bias)


def _layer_hip(x, stats, L: _Layer, heads: int, kind: int, want_stats: bool, tape: Optional[list] = None):
    """The six launches of a layer.  x [B, N, D] bf16 and its row statistics -> (x', statistics of x' | None).  `tape` (the training
    forward of cd360.grad.TextTowerFn): the same launches with the activation written beside its input, not over it, and what the
    backward reads -- the layer's input, the merged q|k|v projection, the stream behind the attention, the pre-activation -- appended."""
    D = x.shape[-1]
    ws, bs = L.qkv
    wq, wsq, cbq = derived(L.owner, "_cd360_qkv", (*ws, *bs, L.ln1.weight, L.ln1.bias),
                           lambda: ops.pack_ln_linear(*L.merged_qkv(), L.ln1.weight, L.ln1.bias))
    w1, ws1, cb1 = derived(L.owner, "_cd360_fc1", (L.fc1.weight, L.fc1.bias, L.ln2.weight, L.ln2.bias),
                           lambda: ops.pack_ln_linear(L.fc1.weight, L.fc1.bias, L.ln2.weight, L.ln2.bias))
    wo, bo, w2, b2 = derived(L.owner, "_cd360_plain", (L.out.weight, L.out.bias, L.fc2.weight, L.fc2.bias),
                             lambda: (L.out.weight.detach().contiguous(), L.out.bias.detach().float().contiguous(),
                                      L.fc2.weight.detach().contiguous(), L.fc2.bias.detach().float().contiguous()))
    qkv = ops.gemm(x, wq, bias=cbq, ln=(stats, wsq, LN_EPS))
    o = ops.causal_attention(qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:], heads)
    x_in = x
    x, stats = ops.gemm(o, wo, bias=bo, res=x, want_stats=True)
    h = ops.gemm(x, w1, bias=cb1, ln=(stats, ws1, LN_EPS))
    if tape is None:
        ops.text_activation(h, kind, out=h)
    else:
        tape.append((x_in, qkv, x, h))
        h = ops.text_activation(h, kind)
    if want_stats:
        return ops.gemm(h, w2, bias=b2, res=x, want_stats=True)
    return ops.gemm(h, w2, bias=b2, res=x), None


class _TextTower(AbstractEmbModel):
    """What the two prompt encoders share: token handling, the route decision and the walk over the layers.  A subclass provides
    _tables() -> (token table [V, D], position table [N, D]), _layers() -> [_Layer], _final_ln() -> nn.LayerNorm, `heads`, `act_kind`."""

    max_length = 77
    tokenizer = None
    modifier_token = None

    def _tokens(self, text):
        """-> (ids on the host, ids on the parameters' device), int64 [B, max_length]."""
        if not isinstance(text, torch.Tensor):
            if isinstance(text, str):
                text = [text]
            if self.tokenizer is None:
                raise ValueError(f"{type(self).__name__} got strings but no tokenizer: no tokenizer vocabulary ships with this package -- pass "
                                 f"int64 token ids [B, {self.max_length}] or construct the embedder with tokenizer=<callable: list of str -> ids>")
            text = self.tokenizer(list(text))
            if not isinstance(text, torch.Tensor):
                text = torch.as_tensor(text)
        if text.dim() == 1:
            text = text[None]
        if text.dtype not in (torch.int64, torch.int32) or text.dim() != 2 or text.shape[1] != self.max_length:
            raise ValueError(f"token ids must be an integer tensor [B, {self.max_length}], got {tuple(text.shape)} {text.dtype}")
        host = text.detach().to("cpu", torch.int64).contiguous()
        V = self._tables()[0].shape[0]
        if host.numel() and (int(host.min()) < 0 or int(host.max()) >= V):
            raise ValueError(f"token ids outside the table: [{int(host.min())}, {int(host.max())}] for {V} rows")
        return host, host.to(self._tables()[0].device)

    def _pad_token_table(self, state_dict, prefix, *args):
        """load_state_dict pre-hook: a checkpoint token table WITHOUT the modifier rows (the SDXL checkpoint's 49408 against this module's
        49408 + k) loads into the first rows; the modifier rows keep what they hold (finetune.load_delta_embeddings fills them)."""
        key = prefix + self.TOKEN_KEY
        have, k = self._tables()[0], len(getattr(self, "modifier_token_id", None) or ())
        got = state_dict.get(key)
        if k and got is not None and got.dim() == 2 and got.shape[0] == have.shape[0] - k and got.shape[1] == have.shape[1]:
            state_dict[key] = torch.cat([got, have.detach()[have.shape[0] - k:].to(got.device, got.dtype)], 0)

    def _hip_route(self) -> bool:
        tok = self._tables()[0]
        if not (tok.is_cuda and all(p.dtype == torch.bfloat16 for p in self.parameters())):
            return False
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError(NO_TAPE)
        D = tok.shape[1]
        if D != self.heads * 64 or self.max_length > ops.TEXT_MAX_TOKENS:
            raise ops.Cd360Error(f"the text-encoder HIP route serves head dim 64 and at most {ops.TEXT_MAX_TOKENS} tokens; got width {D}, "
                                 f"{self.heads} heads, {self.max_length} tokens")
        return True

    def _train_rows(self):
        """The trainable modifier rows of an embedder that cd360.finetune.train_tokens marked, when a tape is wanted (grad enabled); else
        None and nothing changes.  The rows are first copied into the last k rows of the token table (no_grad, in place: the version
        counter moves), so the table every route reads holds what the optimiser last wrote."""
        rows = self.__dict__.get("token_rows")
        if rows is None or not (torch.is_grad_enabled() and rows.requires_grad):
            return None
        tok = self._tables()[0]
        with torch.no_grad():
            tok[tok.shape[0] - rows.shape[0]:].copy_(rows)
        return rows

    def _hip_outputs(self, ids, wants, tape: Optional[list] = None):
        """The HIP route's results by name, in the order of `wants`: "pen" (input of the last layer), "last_ln" / "pen_ln" (final LayerNorm
        of the last layer's output / input), "pooled".  One walk; with `tape` it is the training forward of cd360.grad.TextTowerFn, and
        the output of the last layer (before the final LayerNorm) is appended behind the layers' entries."""
        last, pen, hip = self._run(ids, want_penultimate=True, tape=tape)
        assert hip
        if tape is not None:
            tape.append(last)
        out = {"pen": pen}
        if "last_ln" in wants or "pooled" in wants:
            out["last_ln"] = self._ln(last, True)
        if "pen_ln" in wants:
            out["pen_ln"] = self._ln(pen, True)
        if "pooled" in wants:
            out["pooled"] = self.pool(out["last_ln"], ids, True)
        return [out[w] for w in wants]

    def _run(self, ids, want_penultimate: bool = False, rows=None, tape: Optional[list] = None):
        """ids on the device -> (output of the last layer, input of the last layer | None, hip) -- before any final LayerNorm.  `rows`
        (torch route of a marked embedder): the trainable modifier rows, embedded from torch.cat([table[:-k].detach(), rows]), which is
        the reference's (1 - indices) * x.detach() + indices * x."""
        tok, pos = self._tables()
        layers = self._layers()
        hip = self._hip_route()
        pen = None
        if hip:
            assert rows is None
            x, stats = ops.text_embed(ids, tok.detach(), pos.detach()[:ids.shape[1]].contiguous(), want_stats=True)
            for i, L in enumerate(layers):
                if i == len(layers) - 1:
                    pen = x
                x, stats = _layer_hip(x, stats, L, self.heads, self.act_kind, want_stats=i < len(layers) - 1, tape=tape)
        else:
            if rows is not None:
                tok = torch.cat([tok.detach()[:tok.shape[0] - rows.shape[0]], rows.to(tok.dtype)], 0)
            x = F.embedding(ids, tok) + pos[:ids.shape[1]]
            for i, L in enumerate(layers):
                if i == len(layers) - 1:
                    pen = x
                x = _layer_torch(x, L, self.heads, self.act_kind)
        return x, (pen if want_penultimate else None), hip

    def _ln(self, x, hip: bool):
        ln = self._final_ln()
        if hip:
            return ops.add_layernorm(x.contiguous(), None, ln.weight.detach(), ln.bias.detach(), LN_EPS)[1]
        return F.layer_norm(x, (x.shape[-1],), ln.weight, ln.bias, LN_EPS)

    def encode(self, text):
        return self(text)


def _ln_module(D):
    return nn.LayerNorm(D, eps=LN_EPS)


def _init_(module: nn.Module, std: float = 0.02):
    """Small deterministic-in-shape random weights so that a freshly built tower is finite: real weights come from load_state_dict."""
    with torch.no_grad():
        for name, p in module.named_parameters():
            if p.dim() >= 2:
                p.normal_(0.0, std)
            elif name.endswith("bias"):
                p.zero_()


# ------------------------------------------------------------------------------------------------ CLIP ViT-L/14 text model (HF layout)
class FrozenCLIPEmbedder(_TextTower):
    """modules.py:375-516: the CLIP text model under HF transformers' (4.x) parameter names,
    `transformer.text_model.{embeddings, encoder.layers.i.{layer_norm1, self_attn.{q,k,v,out}_proj, layer_norm2, mlp.{fc1,fc2}}, final_layer_norm}`.
    A `...embeddings.position_ids` entry of a loaded state dict is accepted and ignored; its absence is not an error.

    What forward returns is what the reference's forward returns: ALL layers run under the causal mask and the result is
    final_layer_norm(last_hidden_state) [B, 77, D] (modules.py:487-513 never reads `layer` / `layer_idx`; the shipped config's
    `layer: hidden, layer_idx: 11` therefore selects nothing).  `layer`, `layer_idx` and `always_return_pooled` are accepted and validated as
    there, and do not change the result.  `version` names the checkpoint the weights are expected from; nothing is fetched.
    Architecture arguments default to ViT-L/14: 49408 tokens, width 768, 12 heads, 12 layers, MLP 3072, QuickGELU.
    `modifier_token` ("<new1>" or "<new1>+<new2>+...", at most three): every token appends a row to the token table, ids V, V + 1, ...
    (`modifier_token_id`), initialised as _append_modifier_rows says; with it the token table stays trainable after freeze(), as in the
    reference, and the conditioner calls this embedder outside no_grad.  A stand-alone embedder on the HIP route then needs a no_grad of
    the caller's; inside a GeneralConditioner with `is_trainable: False` (the shipped config) the conditioner's constructor clears every
    requires_grad, as the reference's does, and no tape exists."""

    LAYERS = ["last", "pooled", "hidden"]
    TOKEN_KEY = "transformer.text_model.embeddings.token_embedding.weight"

    def __init__(self, modifier_token=None, version="openai/clip-vit-large-patch14", device="cuda", max_length=77, freeze=True, layer="last",
                 layer_idx=None, always_return_pooled=False, tokenizer=None, vocab_size=49408, width=768, heads=12, layers=12, mlp_width=3072):
        super().__init__()
        assert layer in self.LAYERS
        self.version, self.device, self.max_length, self.tokenizer = version, device, max_length, tokenizer
        self.heads, self.act_kind = heads, ops.ACT_QUICK_GELU
        tm = _Holder()
        tm.embeddings = _Holder()
        tm.embeddings.token_embedding = nn.Embedding(vocab_size, width)
        tm.embeddings.position_embedding = nn.Embedding(max_length, width)
        tm.encoder = _Holder()
        blocks = []
        for _ in range(layers):
            blk = _Holder()
            blk.self_attn = _Holder()
            for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
                setattr(blk.self_attn, n, nn.Linear(width, width))
            blk.layer_norm1 = _ln_module(width)
            blk.mlp = _Holder()
            blk.mlp.fc1 = nn.Linear(width, mlp_width)
            blk.mlp.fc2 = nn.Linear(mlp_width, width)
            blk.layer_norm2 = _ln_module(width)
            blocks.append(blk)
        tm.encoder.layers = nn.ModuleList(blocks)
        tm.final_layer_norm = _ln_module(width)
        self.transformer = _Holder()
        self.transformer.text_model = tm
        _init_(self.transformer)
        self.modifier_token = _modifier_list(modifier_token, 3)
        if self.modifier_token is not None:
            self.modifier_token_id = _append_modifier_rows(tm.embeddings.token_embedding, len(self.modifier_token))
        if freeze:
            self.freeze()
        self.layer, self.layer_idx, self.return_pooled = layer, layer_idx, always_return_pooled
        if layer == "hidden":
            assert layer_idx is not None
            assert 0 <= abs(layer_idx) <= 12
        self._register_load_state_dict_pre_hook(self._drop_position_ids)
        self._register_load_state_dict_pre_hook(self._pad_token_table)

    @staticmethod
    def _drop_position_ids(state_dict, prefix, *args):
        state_dict.pop(prefix + "transformer.text_model.embeddings.position_ids", None)

    def freeze(self):
        self.transformer.eval()
        for p in self.parameters():
            p.requires_grad = False
        if self.modifier_token is not None:
            self.transformer.text_model.embeddings.token_embedding.weight.requires_grad = True

    def _tables(self):
        e = self.transformer.text_model.embeddings
        return e.token_embedding.weight, e.position_embedding.weight

    def _layers(self):
        out = []
        for b in self.transformer.text_model.encoder.layers:
            a = b.self_attn
            out.append(_Layer(b, b.layer_norm1, b.layer_norm2, ((a.q_proj.weight, a.k_proj.weight, a.v_proj.weight),
                                                                (a.q_proj.bias, a.k_proj.bias, a.v_proj.bias)), a.out_proj, b.mlp.fc1, b.mlp.fc2))
        return out

    def _final_ln(self):
        return self.transformer.text_model.final_layer_norm

    def forward(self, text):
        _, ids = self._tokens(text)
        rows = self._train_rows()
        if rows is not None and self._hip_route():
            from cd360 import grad
            return grad.TextTowerFn.apply(rows, self, ids, ("last_ln",))[0]
        x, _, hip = self._run(ids, rows=rows)
        return self._ln(x, hip)


# ------------------------------------------------------------------------------------------------ OpenCLIP ViT-bigG-14 text tower
class FrozenOpenCLIPEmbedder(_TextTower):
    """modules.py:618-771: OpenCLIP's text tower under open_clip's parameter names, `model.{token_embedding.weight, positional_embedding,
    transformer.resblocks.i.{ln_1, attn.{in_proj_weight, in_proj_bias, out_proj}, ln_2, mlp.{c_fc, c_proj}}, ln_final, text_projection,
    logit_scale}` (logit_scale is kept for the checkpoint and unused).

    `layer`: "penultimate" is the INPUT of the last resblock with no ln_final; "last" is ln_final of the output.  With
    always_return_pooled the result is (z[layer], pooled), pooled = ln_final(last)[b, argmax_n ids[b, n]] @ text_projection.  The pooling row is
    the argmax of the ids exactly as the reference has it (modules.py:747-753, "eot_token is the highest number in each sequence"): a
    modifier token's id (49408 and up) exceeds EOT's 49407, so a prompt that holds one is pooled at the MODIFIER's first position, not at
    EOT.  The quirk is the reference's and is kept.  legacy=True returns ln_final(z[layer]) and no pooled vector.
    `arch` / `version` name the checkpoint the weights are expected from; nothing is fetched.  Architecture arguments default to
    ViT-bigG-14's text tower: 49408 tokens, width 1280, 20 heads, 32 layers, MLP 5120, projection 1280, exact GELU.
    `modifier_token`: as FrozenCLIPEmbedder, at most two (the reference initialises two)."""

    LAYERS = ["last", "penultimate"]
    MODIFIER_LIMIT = 2
    TOKEN_KEY = "model.token_embedding.weight"

    def __init__(self, arch="ViT-bigG-14", version="laion2b_s39b_b160k", modifier_token=None, device="cuda", max_length=77, freeze=True,
                 layer="last", always_return_pooled=False, legacy=True, tokenizer=None, vocab_size=49408, width=1280, heads=20, layers=32,
                 mlp_width=5120, proj_dim=1280):
        super().__init__()
        assert layer in self.LAYERS
        self.arch, self.version, self.device, self.max_length, self.tokenizer = arch, version, device, max_length, tokenizer
        self.heads, self.act_kind = heads, ops.ACT_GELU
        m = _Holder()
        m.token_embedding = nn.Embedding(vocab_size, width)
        m.positional_embedding = nn.Parameter(torch.empty(max_length, width))
        m.transformer = _Holder()
        blocks = []
        for _ in range(layers):
            blk = _Holder()
            blk.ln_1 = _ln_module(width)
            blk.attn = _Holder()
            blk.attn.in_proj_weight = nn.Parameter(torch.empty(3 * width, width))
            blk.attn.in_proj_bias = nn.Parameter(torch.zeros(3 * width))
            blk.attn.out_proj = nn.Linear(width, width)
            blk.ln_2 = _ln_module(width)
            blk.mlp = _Holder()
            blk.mlp.c_fc = nn.Linear(width, mlp_width)
            blk.mlp.c_proj = nn.Linear(mlp_width, width)
            blocks.append(blk)
        m.transformer.resblocks = nn.ModuleList(blocks)
        m.ln_final = _ln_module(width)
        m.text_projection = nn.Parameter(torch.empty(width, proj_dim))
        m.logit_scale = nn.Parameter(torch.ones([]) * np.log(1 / 0.07))
        self.model = m
        _init_(m)
        self.modifier_token = _modifier_list(modifier_token, self.MODIFIER_LIMIT)
        self.return_pooled = always_return_pooled
        if self.modifier_token is not None:
            self.modifier_token_id = _append_modifier_rows(m.token_embedding, len(self.modifier_token))
        if freeze:
            self.freeze()
        self.layer = layer
        self.layer_idx = 0 if layer == "last" else 1
        self.legacy = legacy
        self._register_load_state_dict_pre_hook(self._pad_token_table)

    def freeze(self):
        self.model.eval()
        for p in self.parameters():
            p.requires_grad = False
        if self.modifier_token is not None:
            self.model.token_embedding.weight.requires_grad = True

    def _tables(self):
        return self.model.token_embedding.weight, self.model.positional_embedding

    def _layers(self):
        return [_Layer(b, b.ln_1, b.ln_2, ((b.attn.in_proj_weight,), (b.attn.in_proj_bias,)), b.attn.out_proj, b.mlp.c_fc, b.mlp.c_proj)
                for b in self.model.transformer.resblocks]

    def _final_ln(self):
        return self.model.ln_final

    def pool(self, x, ids, hip: bool):
        """x = ln_final(last) [B, N, D] -> [B, proj_dim]: the row at argmax_n ids (lowest index on ties), times text_projection."""
        proj = self.model.text_projection
        if hip:
            wt = derived(self.model, "_cd360_proj_t", (proj,), lambda: proj.detach().t().contiguous())
            return ops.gemm(ops.eot_pool(x, ids), wt)
        return x[torch.arange(x.shape[0], device=x.device), ids.argmax(dim=-1)] @ proj

    def encode_with_transformer(self, ids):
        rows = self._train_rows()
        if rows is not None and self._hip_route():
            from cd360 import grad
            if self.legacy:
                return grad.TextTowerFn.apply(rows, self, ids, ("last_ln" if self.layer == "last" else "pen_ln",))[0]
            return dict(zip(("penultimate", "last", "pooled"), grad.TextTowerFn.apply(rows, self, ids, ("pen", "last_ln", "pooled"))))
        last, pen, hip = self._run(ids, want_penultimate=True, rows=rows)
        if self.legacy:
            return self._ln(last if self.layer == "last" else pen, hip)
        z = {"penultimate": pen, "last": self._ln(last, hip)}
        z["pooled"] = self.pool(z["last"], ids, hip)
        return z

    def forward(self, text):
        _, ids = self._tokens(text)
        if self.return_pooled:
            assert not self.legacy
        z = self.encode_with_transformer(ids)
        if self.legacy:
            return z
        return (z[self.layer], z["pooled"]) if self.return_pooled else z[self.layer]


class FrozenOpenCLIPEmbedder2(FrozenOpenCLIPEmbedder):
    """modules.py:519-616: the same forward without modifier tokens (legacy defaults as there)."""

    def __init__(self, arch="ViT-H-14", version="laion2b_s32b_b79k", device="cuda", max_length=77, freeze=True, layer="last",
                 always_return_pooled=False, legacy=True, **arch_args):
        super().__init__(arch=arch, version=version, modifier_token=None, device=device, max_length=max_length, freeze=freeze, layer=layer,
                         always_return_pooled=always_return_pooled, legacy=legacy, **arch_args)


# ------------------------------------------------------------------------------------------------ size / crop embedders
class Timestep(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.dim = dim

    def forward(self, t):
        return timestep_embedding(t, self.dim)


class ConcatTimestepEmbedderND(AbstractEmbModel):
    """modules.py:1117-1134: embeds each dimension independently and concatenates them.  x [B] or [B, dims] -> [B, dims * outdim] fp32, in
    torch on x's device (a few hundred values: no kernel of its own, no host read)."""

    def __init__(self, outdim):
        super().__init__()
        self.timestep = Timestep(outdim)
        self.outdim = outdim
        self.modifier_token = None

    def forward(self, x):
        if x.ndim == 1:
            x = x[:, None]
        assert x.ndim == 2
        b, dims = x.shape
        return self.timestep(x.reshape(b * dims)).reshape(b, dims * self.outdim)
