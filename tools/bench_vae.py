"""First-stage decode (Decoder.forward, reference sgm/modules/diffusionmodules/model.py:604-733) on the MI355X: the HIP decoder against
the fp32 framework restatement (tests/vae_fp32.py) on the same seeded synthetic weights at the SDXL ddconfig.

    python tools/bench_vae.py [--min-seconds 1.0] [--json out.json]

Per case (latent 64^2 / 128^2 = image 512^2 / 1024^2, batch 1 / 2): ms per image of both decoders (device events around repeated
decodes, warm-up first, at least --min-seconds of timed work per column) and the mid-block attention kernel's ms and FLOP/s
(FLOP = 4 N^2 C B) from the HIP path's per-launch events (cd360.ops.profile_start: attention kernel + combine kernel).  For batch 2
also the max relative error of the per-image decode and of the batch-folded pass against the fp32 restatement.  Kernel times proper come
from a separate `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_vae.py --profile-only` (one decode per case):
the new kernels are attn_single_kernel<512>, attn_single_combine_kernel, vae_conv_in_kernel and vae_conv_out_kernel.

Encoder section (Encoder.forward, model.py:487-601, against tests/vae_enc_fp32.py): image 512^2 / 1024^2, batch 1 / 5 (the target x and the
b*n reference images of shared_step): ms per image of both encoders and the max relative error of the HIP encoder against fp32.  Its
kernels in the rocprofv3 run: conv_igemm_kernel (the Downsamples among the other convolutions), vae_enc_conv_out_kernel and
vae_conv_in_kernel (here reading the 3-channel image).  --section decoder | encoder | all (default)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "custom-diffusion360_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import vae_enc_fp32  # noqa: E402
import vae_fp32  # noqa: E402
import weights as W  # noqa: E402
from cd360 import ops  # noqa: E402
from sgm.modules.diffusionmodules.model import Decoder, Encoder  # noqa: E402

DDCONFIG = dict(attn_type="vanilla-xformers", double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128,
                ch_mult=[1, 2, 4, 4], num_res_blocks=2, attn_resolutions=[], dropout=0.0)
CASES = [(64, 1), (64, 2), (128, 1), (128, 2)]
ENC_CASES = [(512, 1), (512, 5), (1024, 1), (1024, 5)]


def timed(fn, min_seconds):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    reps = max(2, int(min_seconds / max(time.perf_counter() - t0, 1e-4)) + 1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile-only", action="store_true", help="one decode per case, HIP path only (for rocprofv3)")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--section", choices=("decoder", "encoder", "all"), default="all")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    if a.section in ("decoder", "all"):
        rows += bench_decoder(a, dev)
    if a.section in ("encoder", "all"):
        rows += bench_encoder(a, dev)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


def bench_encoder(a, dev):
    enc = Encoder(**DDCONFIG).eval()
    sd = W.load_into(enc, 3)
    enc = enc.to(dev)
    sd = {k: v.to(dev) for k, v in sd.items()}
    rows = []
    with torch.no_grad():
        for hw, b in ENC_CASES:
            x = W.tensor(f"x{hw}", (b, 3, hw, hw), seed=1).to(dev)
            if a.profile_only:
                enc(x)
                torch.cuda.synchronize()
                continue
            ms = timed(lambda: enc(x), a.min_seconds)
            ops.profile_start()
            enc(x)
            prof = ops.profile_stop()
            r = {"section": "encoder", "image": hw, "batch": b, "hip_ms_per_image": ms / b,
                 "hip_event_ms_per_image": {k: v["ms"] / b for k, v in sorted(prof.items())}}
            if not a.no_baseline:
                torch.backends.cuda.matmul.allow_tf32 = torch.backends.cudnn.allow_tf32 = False
                base = timed(lambda: vae_enc_fp32.encode(sd, x, DDCONFIG["ch_mult"], 2), a.min_seconds)
                want = vae_enc_fp32.encode(sd, x, DDCONFIG["ch_mult"], 2)
                got = enc(x)
                r["fp32_framework_ms_per_image"] = base / b
                r["max_rel_err_vs_fp32"] = ((got - want).abs().max() / want.abs().max()).item()
            rows.append(r)
            print(json.dumps(r), flush=True)
    return rows


def bench_decoder(a, dev):
    dec = Decoder(**DDCONFIG).eval()
    sd = W.load_into(dec, 3)
    dec = dec.to(dev)
    sd = {k: v.to(dev) for k, v in sd.items()}
    rows = []
    with torch.no_grad():
        for hw, b in CASES:
            z = W.tensor(f"z{hw}", (b, 4, hw, hw), seed=1).to(dev)
            if a.profile_only:
                dec(z)
                torch.cuda.synchronize()
                continue
            ms = timed(lambda: dec(z), a.min_seconds)
            ops.profile_start()
            dec(z)
            prof = ops.profile_stop()
            att = prof.get("attn_single", {"ms": float("nan"), "flops": 0.0})
            base = None if a.no_baseline else timed(lambda: vae_fp32.decode(sd, z, DDCONFIG["ch_mult"], 2), a.min_seconds)
            acc = {}
            if b > 1 and not a.no_baseline:
                # forward() decodes one image per pass; the batch-folded pass (_decode_pass on the whole batch) for comparison: each
                # path's max relative error against the fp32 restatement, and the two paths against each other
                want = vae_fp32.decode(sd, z, DDCONFIG["ch_mult"], 2)
                per, folded = dec(z), dec._decode_pass(z)
                rel = lambda x, y: ((x - y).abs().max() / y.abs().max()).item()
                acc = {"per_image_err_vs_fp32": rel(per, want), "folded_err_vs_fp32": rel(folded, want), "folded_vs_per_image": rel(folded, per)}
            r = {"section": "decoder", "image": 8 * hw, "batch": b, "hip_ms_per_image": ms / b, "fp32_framework_ms_per_image": None if base is None else base / b,
                 "attn_ms": att["ms"], "attn_tflops": att["flops"] / att["ms"] / 1e9 if att["ms"] > 0 else None,
                 "attn_splits": ops.attention_single_splits(b, hw * hw), "max_batch_per_pass_computed": dec.max_batch(hw, hw), **acc}
            rows.append(r)
            print(json.dumps(r), flush=True)
    return rows


if __name__ == "__main__":
    main()
