"""Framework restatement of the two prompt encoders of the reference's conditioner (sgm/modules/encoders/modules.py:377-516, 618-771) as
plain torch modules that load the checkpoint layouts of the product's embedders: the yardstick of tests/test_text_cpu.py and
tests/test_text_gpu.py and the baseline column of tools/bench_text.py.  Not part of the product, and written against torch alone:

  HFTextTower        HF transformers' CLIPTextModel as the reference drives it: separate q / k / v Linears, q * head_dim^-0.5, the additive
                     mask of modules.py:451-458 (finfo.min above the diagonal), softmax, QuickGELU, final_layer_norm of the last layer.
  OpenCLIPTextTower  open_clip's text tower: nn.MultiheadAttention + nn.LayerNorm + nn.GELU under the additive -inf mask, sequence first;
                     -> {"penultimate", "last", "pooled"} as FrozenOpenCLIPEmbedder.encode_with_transformer (legacy=False) has them.

torch's own attention is the oracle of the second tower, torch's matmul + softmax of the first.  Both run in whatever dtype they are cast
to (fp32: the reference; `.bfloat16()` on the CPU: torch's own bf16 arithmetic, the yardstick of the tolerance rule)."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

import weights as W  # tests/golden/weights.py

EPS = 1e-5


class _Box(nn.Module):
    pass


def rel(got, want):
    """The suite's max-norm relative error."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def synth_weights(module_or_shapes, seed):
    """Deterministic fp32 weights for a state-dict layout (tests/golden/weights.py); LayerNorm gains are 1 + 0.1 n under every name the two
    layouts use for them (the generator knows `norm` in a name, not open_clip's `ln_`)."""
    shapes = module_or_shapes if isinstance(module_or_shapes, dict) else {k: v.shape for k, v in module_or_shapes.state_dict().items()}
    sd = W.synth_state_dict({k: s for k, s in shapes.items() if len(s)}, seed)
    for k, s in shapes.items():
        if not len(s):  # open_clip's logit_scale, the one 0-d entry (kept for the checkpoint, unused)
            sd[k] = W.tensor(k, (1,), seed).reshape(())
    for k in sd:
        part = k.split(".")[-2] if "." in k else ""
        if k.endswith(".weight") and part.startswith("ln_"):
            sd[k] = 1.0 + W.tensor(k, shapes[k], seed, 0.1)
    return sd


class HFTextTower(nn.Module):
    def __init__(self, vocab, width, heads, layers, mlp, n_ctx=77):
        super().__init__()
        self.heads = heads
        tm = _Box()
        tm.embeddings = _Box()
        tm.embeddings.token_embedding = nn.Embedding(vocab, width)
        tm.embeddings.position_embedding = nn.Embedding(n_ctx, width)
        tm.encoder = _Box()
        tm.encoder.layers = nn.ModuleList()
        for _ in range(layers):
            b = _Box()
            b.layer_norm1, b.layer_norm2 = nn.LayerNorm(width, eps=EPS), nn.LayerNorm(width, eps=EPS)
            b.self_attn = _Box()
            for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
                setattr(b.self_attn, n, nn.Linear(width, width))
            b.mlp = _Box()
            b.mlp.fc1, b.mlp.fc2 = nn.Linear(width, mlp), nn.Linear(mlp, width)
            tm.encoder.layers.append(b)
        tm.final_layer_norm = nn.LayerNorm(width, eps=EPS)
        self.transformer = _Box()
        self.transformer.text_model = tm

    def layer(self, b, x):
        B, N, D = x.shape
        hd = D // self.heads
        a = b.self_attn
        h = b.layer_norm1(x)
        split = lambda t: t.view(B, N, self.heads, hd).transpose(1, 2)
        q, k, v = split(a.q_proj(h) * hd ** -0.5), split(a.k_proj(h)), split(a.v_proj(h))
        mask = torch.full((N, N), torch.finfo(x.dtype).min, dtype=x.dtype, device=x.device).triu_(1)
        p = F.softmax(q @ k.transpose(-1, -2) + mask, dim=-1)
        x = x + a.out_proj((p @ v).transpose(1, 2).reshape(B, N, D))
        h = b.mlp.fc1(b.layer_norm2(x))
        return x + b.mlp.fc2(h * torch.sigmoid(1.702 * h))

    def embed(self, ids):
        e = self.transformer.text_model.embeddings
        return e.token_embedding(ids) + e.position_embedding(torch.arange(ids.shape[1], device=ids.device))[None]

    def forward(self, ids):
        x = self.embed(ids)
        for b in self.transformer.text_model.encoder.layers:
            x = self.layer(b, x)
        return self.transformer.text_model.final_layer_norm(x)


class OpenCLIPTextTower(nn.Module):
    def __init__(self, vocab, width, heads, layers, mlp, proj, n_ctx=77):
        super().__init__()
        m = _Box()
        m.token_embedding = nn.Embedding(vocab, width)
        m.positional_embedding = nn.Parameter(torch.zeros(n_ctx, width))
        m.transformer = _Box()
        m.transformer.resblocks = nn.ModuleList()
        for _ in range(layers):
            b = _Box()
            b.ln_1, b.ln_2 = nn.LayerNorm(width, eps=EPS), nn.LayerNorm(width, eps=EPS)
            b.attn = nn.MultiheadAttention(width, heads)
            b.mlp = _Box()
            b.mlp.c_fc, b.mlp.c_proj = nn.Linear(width, mlp), nn.Linear(mlp, width)
            b.gelu = nn.GELU()
            m.transformer.resblocks.append(b)
        m.ln_final = nn.LayerNorm(width, eps=EPS)
        m.text_projection = nn.Parameter(torch.zeros(width, proj))
        m.logit_scale = nn.Parameter(torch.zeros([]))
        self.model = m

    def layer(self, b, x, mask):
        """x [N, B, D], sequence first."""
        h = b.ln_1(x)
        x = x + b.attn(h, h, h, need_weights=False, attn_mask=mask)[0]
        return x + b.mlp.c_proj(b.gelu(b.mlp.c_fc(b.ln_2(x))))

    def forward(self, ids):
        m = self.model
        x = (m.token_embedding(ids) + m.positional_embedding[:ids.shape[1]]).permute(1, 0, 2)
        N = x.shape[0]
        mask = torch.full((N, N), float("-inf"), dtype=x.dtype, device=x.device).triu_(1)
        out = {}
        blocks = m.transformer.resblocks
        for i, b in enumerate(blocks):
            if i == len(blocks) - 1:
                out["penultimate"] = x.permute(1, 0, 2)
            x = self.layer(b, x, mask)
        out["last"] = m.ln_final(x.permute(1, 0, 2))
        out["pooled"] = out["last"][torch.arange(ids.shape[0], device=ids.device), ids.argmax(dim=-1)] @ m.text_projection
        return out


def token_ids(B, V, n_ctx=77, seed=0, eot=None, modifier=None):
    """Prompts as a tokenizer pads them: BOS (id V_base - 2), a few word ids, EOT (the highest base id), then padding with 0 -- every row of
    its own length.  `modifier` = (id, position): that id placed inside the words of every prompt (it exceeds EOT's id: the argmax quirk)."""
    g = torch.Generator().manual_seed(seed)
    eot = V - 1 if eot is None else eot
    ids = torch.zeros(B, n_ctx, dtype=torch.int64)
    for b in range(B):
        n = 3 + int(torch.randint(0, n_ctx - 6, (1,), generator=g))
        ids[b, 0] = eot - 1
        ids[b, 1:n] = torch.randint(1, eot - 1, (n - 1,), generator=g)
        ids[b, n] = eot
        if modifier is not None:
            ids[b, min(modifier[1], n - 1)] = modifier[0]
    return ids
