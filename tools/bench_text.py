"""The two prompt encoders on the MI355X, for the record (no threshold anywhere): FrozenCLIPEmbedder (ViT-L/14: 768 wide, 12 heads, 12
layers) and FrozenOpenCLIPEmbedder (ViT-bigG-14: 1280 wide, 20 heads, 32 layers) on the HIP route against tests/text_fp32.py's modules
cast to bf16 on the same GPU (torch's own bf16 kernels), random weights, 1 and 3 prompts of 77 tokens.

    python tools/bench_text.py [--rounds 7] [--min-seconds 0.3] [--vocab 49408] [--json out.json]

Both columns are timed in ONE process, interleaved: after a warm-up of every shape, `--rounds` rounds, each round timing the HIP route and
then the torch modules (device events around enough repeated encodes for --min-seconds of work); the figure is the MEDIAN of the rounds'
milliseconds per encode, the spread their (min, max).  Also printed: the HIP route's per-launch-family event times of one encode
(cd360.ops.profile_start) and its max relative error against the fp32 module.  Kernel times proper come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/bench_text.py --profile-only`."""
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
from cd360 import ops  # noqa: E402
from sgm.modules.encoders.modules import FrozenCLIPEmbedder, FrozenOpenCLIPEmbedder  # noqa: E402

PROMPTS = (1, 3)


def window(fn, min_seconds):
    """ms per call over enough calls for `min_seconds` of device work (one call sizes the window)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    reps = max(3, int(min_seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def towers(vocab, dev):
    """[(name, HIP-route embedder in bf16, text_fp32 module in fp32 on the device, its bf16 copy, result picker)] on one set of weights."""
    out = []
    clip = FrozenCLIPEmbedder(vocab_size=vocab)
    ref = T32.HFTextTower(vocab, 768, 12, 12, 3072).eval()
    ref.load_state_dict(clip.state_dict(), strict=True)
    out.append(("clip-l", clip, ref, lambda z: z, lambda z: z))
    big = FrozenOpenCLIPEmbedder(vocab_size=vocab, layer="penultimate", always_return_pooled=True, legacy=False)
    ref = T32.OpenCLIPTextTower(vocab, 1280, 20, 32, 5120, 1280).eval()
    ref.load_state_dict(big.state_dict(), strict=True)
    out.append(("openclip-bigg", big, ref, lambda z: z[1], lambda z: z["pooled"]))
    return [(n, e.to(dev, torch.bfloat16), r.to(dev), copy.deepcopy(r).to(dev, torch.bfloat16), pe, pr) for n, e, r, pe, pr in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--vocab", type=int, default=49408)
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile-only", action="store_true", help="one encode per case, HIP route only (for rocprofv3)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_text.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    rows = []
    with torch.no_grad():
        for name, emb, ref32, ref16, pick_e, pick_r in towers(a.vocab, dev):
            for b in PROMPTS:
                ids = T32.token_ids(b, a.vocab, seed=b)
                d_ids = ids.to(dev)
                hip = lambda: emb(ids)          # ids from the host, as a tokenizer hands them: the host check and the copy are part of the call
                base = lambda: ref16(d_ids)
                if a.profile_only:
                    hip()
                    torch.cuda.synchronize()
                    continue
                for _ in range(3):  # warm-up of both columns at this shape
                    hip()
                    base()
                torch.cuda.synchronize()
                h, t = [], []
                for _ in range(a.rounds):
                    h.append(window(hip, a.min_seconds))
                    t.append(window(base, a.min_seconds))
                ops.profile_start()
                got = hip()
                prof = ops.profile_stop()
                want = pick_r(ref32(d_ids))
                r = {"tower": name, "prompts": b, "hip_ms": statistics.median(h), "hip_ms_min_max": [min(h), max(h)],
                     "torch_bf16_ms": statistics.median(t), "torch_bf16_ms_min_max": [min(t), max(t)], "rounds": a.rounds,
                     "hip_rel_err_vs_fp32": T32.rel(pick_e(got).float(), want), "torch_bf16_rel_err_vs_fp32": T32.rel(pick_r(base()).float(), want),
                     "hip_event_ms": {k: round(v["ms"], 4) for k, v in sorted(prof.items())}}
                rows.append(r)
                print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
