"""Training the modifier-token rows on the MI355X, for the record (no threshold anywhere): forward + backward of the full prompt encoders
-- FrozenCLIPEmbedder (ViT-L/14: 768 wide, 12 heads, 12 layers, k = 1 modifier row) and FrozenOpenCLIPEmbedder (ViT-bigG-14: 1280 wide, 20
heads, 32 layers; penultimate + pooled) -- marked by cd360.finetune.train_tokens on the HIP route (cd360.grad.TextTowerFn), against torch's
bf16 eager autograd of tests/text_fp32.py's modules with the reference's masked embedding on the same GPU; random weights, 1 and 3 prompts
of 77 tokens, the gradient of a fixed random linear functional of the outputs.

    python tools/bench_text_grad.py [--rounds 7] [--min-seconds 0.3] [--vocab 49408] [--json out.json]

Both columns are timed in ONE process, interleaved, exactly as tools/bench_text.py does: after a warm-up of every shape, `--rounds` rounds,
each timing the HIP route and then the torch module (device events around enough repeated forward + backward passes for --min-seconds of
work); the figure is the MEDIAN of the rounds' milliseconds per pass, the spread their (min, max).  Also printed: the HIP route's
per-launch-family event times of one pass (cd360.ops.profile_start) and both columns' max relative error of rows.grad against fp32."""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "custom-diffusion360_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import text_fp32 as T32  # noqa: E402
import textgrad_cases as TG  # noqa: E402
from bench_text import window  # noqa: E402
from cd360 import finetune, ops  # noqa: E402
from sgm.modules.encoders.modules import FrozenCLIPEmbedder, FrozenOpenCLIPEmbedder  # noqa: E402

PROMPTS = (1, 3)


def towers(vocab, dev):
    """[(name, marked HIP-route embedder in bf16, its TokenRows, text_fp32 module in fp32 on the device, output names)], one set of weights."""
    out = []
    clip = FrozenCLIPEmbedder(modifier_token="<new1>", vocab_size=vocab)
    ref = T32.HFTextTower(vocab + 1, 768, 12, 12, 3072).eval()
    ref.load_state_dict(clip.state_dict(), strict=True)
    out.append(("clip-l", clip, ref, ("last_ln",)))
    big = FrozenOpenCLIPEmbedder(modifier_token="<new1>", vocab_size=vocab, layer="penultimate", always_return_pooled=True, legacy=False)
    ref = T32.OpenCLIPTextTower(vocab + 1, 1280, 20, 32, 5120, 1280).eval()
    ref.load_state_dict(big.state_dict(), strict=True)
    out.append(("openclip-bigg", big, ref, ("pen", "pooled")))
    res = []
    for name, emb, ref, names in out:
        emb = emb.to(dev, torch.bfloat16)
        res.append((name, emb, finetune.train_tokens(TG.holder(emb)), ref.to(dev), names))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--vocab", type=int, default=49408)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_text_grad.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    rows = []
    for name, emb, tr, ref32, names in towers(a.vocab, dev):
        ref16 = copy.deepcopy(ref32).to(torch.bfloat16)
        masked_fn = TG.hf_masked if name == "clip-l" else TG.openclip_masked
        for r_ in (ref32, ref16):
            for p in r_.parameters():
                p.requires_grad = False
            TG.table_of(r_).requires_grad = True
        for b in PROMPTS:
            ids = TG.prompt_ids("once", a.vocab, 1, seed=b, B=b)
            d_ids = ids.to(dev)
            mods = [a.vocab]
            shapes = {"last_ln": (b, 77, 768)} if name == "clip-l" else {"pen": (b, 77, 1280), "pooled": (b, 1280)}
            cots = {n: c.to(dev) for n, c in TG.cotangents(shapes, seed=7).items()}

            def hip():
                tr.rows[0].grad = None
                z = emb(ids)  # ids from the host, as a tokenizer hands them
                outs = {"last_ln": z} if name == "clip-l" else {"pen": z[0], "pooled": z[1]}
                TG.functional(outs, cots).backward()
                return tr.rows[0].grad

            def base(ref=ref16):
                tab = TG.table_of(ref)
                tab.grad = None
                outs = masked_fn(ref, d_ids, mods)
                TG.functional({n: outs[n] for n in names}, cots).backward()
                return tab.grad[a.vocab:]

            for _ in range(3):  # warm-up of both columns at this shape
                hip()
                base()
            torch.cuda.synchronize()
            h, t = [], []
            for _ in range(a.rounds):
                h.append(window(hip, a.min_seconds))
                t.append(window(base, a.min_seconds))
            ops.profile_start()
            got = hip().float()
            prof = ops.profile_stop()
            want = base(ref32).float()
            r = {"tower": name, "prompts": b, "hip_ms": statistics.median(h), "hip_ms_min_max": [min(h), max(h)],
                 "torch_bf16_ms": statistics.median(t), "torch_bf16_ms_min_max": [min(t), max(t)], "rounds": a.rounds,
                 "hip_rel_err_vs_fp32": T32.rel(got, want), "torch_bf16_rel_err_vs_fp32": T32.rel(base().float(), want),
                 "hip_event_ms": {k: [round(v["ms"], 4), v["n"]] for k, v in sorted(prof.items())}}
            rows.append(r)
            print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
