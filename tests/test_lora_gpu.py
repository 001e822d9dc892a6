"""add_lora=True on the MI355X: cd360_lowrank_add_bf16 / cd360_dropout_apply_bf16 / cd360_dropout_tick against fp32 torch, grad.LoraFn
against torch autograd, the pose block with adapters against the reference's goldens (tests/golden/make_golden_lora.py), the fused route's
folded weights, and a fine-tuning step with adapters."""
import os

import numpy as np
import pytest
import torch

import weights as W
from cd360 import grad, ops
from cd360.cameras import unpack_cameras

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# Bars of tests/test_modules_gpu.py and tests/test_backward_gpu.py.  With every adapter randomised (up weights included) the projections
# carry roughly twice the signal and the attention logits sharpen: one block measures 1.17e-2 against the reference (the adapter-free
# block measures 7.9e-3 under TOL_BLOCK = 1e-2), so the block comparisons take the next bar, TOL_DEEP; the train-mode gradients measure
# <= 4.4e-2 and take the bar of the train-mode gradient golden (test_backward_gpu.py::test_pose_block_mask_ref_train_mode_gradients).
TOL_DEEP = 1.6e-2
TOL = 2.5e-2
TOL_GRAD = 5e-2


def load(name):
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLD, name + ".npz")).items()}


def rel(got, want):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert torch.isfinite(got).all()
    return (got - want).abs().max().item() / max(want.abs().max().item(), 1e-12)


def one_rounding(got, want32):
    """Every element of `got` (bf16) within one bf16 rounding of the fp32 value (plus fp32 summation-order slack)."""
    got, want32 = got.float(), want32.float()
    return bool(((got - want32).abs() <= want32.abs() * 2.0 ** -8 + 1e-6).all())


def rnd(*s, g, scale=1.0):
    return (torch.randn(*s, generator=g, device=DEV) * scale).to(BF)


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("r", [16, 32, 64])
@pytest.mark.parametrize("M,N", [(3072, 3840), (1001, 640), (77, 1280)])
def test_lowrank_add_matches_fp32(r, M, N):
    g = torch.Generator(device=DEV).manual_seed(r + M + N)
    t, u, base = rnd(M, r, g=g), rnd(N, r, g=g, scale=0.1), rnd(M, N, g=g)
    want = base.float() + t.float() @ u.float().t()
    got = ops.lowrank_add(t, u, base=base)
    assert one_rounding(got, want)
    got0 = ops.lowrank_add(t, u)  # base = NULL
    assert one_rounding(got0, t.float() @ u.float().t())


@pytest.mark.parametrize("r", [16, 32, 64])
def test_lowrank_add_on_strided_slices_in_place(r):
    """q|k|v column slices of one buffer (row stride 3 N), T a slice of a wider buffer, out aliasing base; the neighbours stay untouched."""
    g = torch.Generator(device=DEV).manual_seed(7 + r)
    M, N = 1030, 1280
    qkv = rnd(M, 3 * N, g=g)
    tt = rnd(M, 3 * r + 8, g=g)
    us = [rnd(N, r, g=g, scale=0.1) for _ in range(3)]
    before = qkv.clone()
    for i in range(3):
        sl = qkv[:, i * N:(i + 1) * N]
        ops.lowrank_add(tt[:, i * r:(i + 1) * r], us[i], base=sl, out=sl)
    for i in range(3):
        want = before[:, i * N:(i + 1) * N].float() + tt[:, i * r:(i + 1) * r].float() @ us[i].float().t()
        assert one_rounding(qkv[:, i * N:(i + 1) * N], want), i


def _mask(M, N, p, site, key=None, r=16):
    """s * keep of cd360_lowrank_add_bf16 recovered with T U^T = 1 (T = e_0, U = e_0)."""
    t = torch.zeros(M, r, dtype=BF, device=DEV)
    t[:, 0] = 1
    u = torch.zeros(N, r, dtype=BF, device=DEV)
    u[:, 0] = 1
    return ops.lowrank_add(t, u, p=p, site=site, key=key)


def test_dropout_mask_is_shared_by_forward_and_backward_and_keyed():
    M, N, p = 2048, 2560, 0.1  # 5.2 M elements
    key = torch.tensor([1234567, 5], dtype=torch.int64, device=DEV)
    fwd = _mask(M, N, p, 3, key)
    bwd = ops.dropout_apply(torch.ones(M, N, dtype=BF, device=DEV), p, 3, key=key)
    assert torch.equal(fwd, bwd)
    s = torch.tensor(1 / 0.9, dtype=BF).item()
    assert set(torch.unique(fwd.float()).tolist()) <= {0.0, s}
    keep = (fwd != 0).float().mean().item()
    assert abs(keep - 0.9) < 0.005, keep
    assert not torch.equal(fwd, _mask(M, N, p, 4, key))                      # another site
    key2 = key.clone()
    key2[1] += 1
    assert not torch.equal(fwd, _mask(M, N, p, 3, key2))                     # another offset
    assert torch.equal(_mask(M, N, 0.0, 3, key), torch.ones(M, N, dtype=BF, device=DEV))  # p = 0: no mask, s = 1
    # no row / column structure: per-row and per-column keep fractions stay near 0.9
    k = (fwd != 0).float()
    assert (k.mean(1) - 0.9).abs().max() < 0.05 and (k.mean(0) - 0.9).abs().max() < 0.05


def test_dropout_tick_gives_new_masks_on_every_graph_replay():
    M, N, p = 256, 640, 0.1
    key = torch.tensor([99, 0], dtype=torch.int64, device=DEV)
    ones = torch.ones(M, N, dtype=BF, device=DEV)
    out = torch.empty(M, N, dtype=BF, device=DEV)
    lib = __import__("cd360._lib", fromlist=["load"]).load()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.dropout_apply(ones, p, 1, key=key, out=out)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one stream: tick, then the mask (no parallel branches)
        ops.check(lib.cd360_dropout_tick(key.data_ptr(), ops._stream()), "cd360_dropout_tick")
        ops.dropout_apply(ones, p, 1, key=key, out=out)
    seen = []
    for i in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert int(key[1]) == i + 1  # the capture itself executes nothing
        seen.append(out.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    k2 = key.clone()
    k2[1] = 2
    assert torch.equal(seen[1], ops.dropout_apply(ones, p, 1, key=k2))


# ------------------------------------------------------------------------------------------------ autograd
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_lora_fn_gradients_match_torch_autograd(p):
    g = torch.Generator(device=DEV).manual_seed(5)
    M, K, N = 2 * 333, 640, 1280
    x, base = rnd(2, 333, K, g=g), rnd(2, 333, N, g=g)
    D, U = rnd(32, K, g=g, scale=1 / 32), rnd(N, 32, g=g, scale=0.05)
    cot = rnd(2, 333, N, g=g)
    leaves = [t.clone().requires_grad_(True) for t in (x, base, D, U)]
    site = 17
    out = grad.lora(*leaves, p, site)
    out.backward(cot)
    key = ops.dropout_state(DEV)
    mask = ops.dropout_apply(torch.ones(M, N, dtype=BF, device=DEV), p, site, key=key).float().reshape(2, 333, N) if p > 0 else 1.0
    ref = [t.float().clone().requires_grad_(True) for t in (x, base, D, U)]
    want = ref[1] + mask * ((ref[0] @ ref[2].t()) @ ref[3].t())
    want.backward(cot.float())
    assert rel(out, want) < 1e-2
    for a, b_, name in zip(leaves, ref, ("x", "base", "D", "U")):
        assert rel(a.grad, b_.grad) < 2e-2, name


# ------------------------------------------------------------------------------------------------ modules
def _block(seed=2, C=64, heads=1, cd=32, train=False):
    from sgm.modules.attention import BasicTransformerBlock
    blk = BasicTransformerBlock(C, heads, 64, context_dim=cd, checkpoint=False, attn_mode="softmax-xformers", image_cross=True, far=2, num_samples=4,
                                rgb_predict=True, mode="feature-nerf", stratified=True, add_lora=True).train(train)
    W.load_into(blk, seed=seed)
    return blk.to(DEV, BF)


def _b16(t):
    return t.to(DEV, BF)


@torch.no_grad()
def test_pose_block_with_adapters_eval_matches_reference_golden():
    g = load("block_lora_eval")
    blk = _block()
    x = _b16(g["x"])
    assert blk.fused_ready(x)
    out, fg, wts, alphas, rgb = blk(x, context=_b16(g["ctx"]), context_ref=_b16(g["cref"]), pose=unpack_cameras(g["cams"]))
    assert wts is None
    errs = [rel(out, g["out"]), rel(fg, g["fg"]), rel(alphas, g["alphas"]), rel(rgb, g["rgb"]), rel(blk(x, context=_b16(g["ctx"]))[0], g["plain"])]
    print("eval, adapters folded:", errs)
    assert max(errs) < TOL_DEEP
    # the adapters matter: the reference's block without them is far off
    assert rel(g["out"], load("block_eval")["out"]) > 10 * TOL_DEEP


def test_pose_block_with_adapters_train_matches_reference_golden(monkeypatch):
    """Train mode on the autograd route (adapter dropout p = 0 as in the generator), output and every poseattn gradient."""
    from sgm.modules.nerfsd_pytorch3d import Raymarcher
    g = load("block_lora_train")
    blk = _block(train=True)
    for a in (blk.attn1, blk.attn2):
        for w in "qkvo":
            getattr(a, f"dropout{w}").p = 0.0
    names = [k[len("grad."):] for k in g if k.startswith("grad.")]
    assert sum("_attn3_" in k for k in names) == 16
    for k, p_ in blk.named_parameters():
        p_.requires_grad = k in names or "pose" in k or k.startswith(("attn1.", "attn2."))
    monkeypatch.setattr(Raymarcher, "jitter", lambda self, resolution, device: ((g["jit_x"], g["jit_y"]), g["jit_d"].to(device)))
    out, fg, _, alphas, rgb = blk(_b16(g["x"]), context=_b16(g["ctx"]), context_ref=_b16(g["cref"]), pose=unpack_cameras(g["cams"]))
    errs = [rel(out, g["out"]), rel(fg, g["fg"]), rel(alphas, g["alphas"]), rel(rgb, g["rgb"])]
    print("train forward:", errs)
    assert max(errs) < TOL
    cot = W.tensor("cot", tuple(out.shape), seed=2).to(DEV)
    ((out.float() * cot).sum() + fg.float().sum() + rgb.float().sum()).backward()
    params = dict(blk.named_parameters())
    worst = {}
    for k in names:
        assert params[k].grad is not None, k
        if k.endswith("nviews.bias"):  # mathematically zero (softmax shift invariance)
            continue
        worst[k] = rel(params[k].grad, g["grad." + k])
    print("worst gradients:", sorted(worst.items(), key=lambda kv: -kv[1])[:6])
    assert max(worst.values()) < TOL_GRAD, {k: v for k, v in worst.items() if v >= TOL_GRAD}


@torch.no_grad()
@pytest.mark.parametrize("C,heads,cd", [(64, 1, 32), (640, 10, 2048)])
def test_fused_route_with_folded_adapters_equals_module_route(C, heads, cd):
    """Eval: the fused route (adapters folded into the packs, the cached K / V) against the module route with the adapters as branches
    (p = 0), both bf16 on the GPU; then an update of one adapter weight must reach the next fused forward (the packs are keyed on it)."""
    from cd360 import routes
    from make_golden_params import sdxl_block_inputs
    if C == 64:
        gi = load("block_lora_eval")
        x, ctx, cref, pose = _b16(gi["x"]), _b16(gi["ctx"]), _b16(gi["cref"]), unpack_cameras(gi["cams"])
    else:
        x, ctx, cref, pose = sdxl_block_inputs(C)
        x, ctx, cref = _b16(x), _b16(ctx), _b16(cref)
    blk = _block(seed=6, C=C, heads=heads, cd=cd)
    assert blk.fused_ready(x)
    fused = blk(x, context=ctx, context_ref=cref, pose=pose)[0]
    for n_, p_ in blk.named_parameters():
        p_.requires_grad_("_attn3_" in n_)
    lora = [p_ for p_ in blk.parameters() if p_.requires_grad]
    with torch.enable_grad():  # a tape over the adapters: the module route, adapters as grad.LoraFn branches on the HIP kernels
        assert not blk.fused_ready(x) and not blk.attn1.lora_merge()
        module = blk(x, context=ctx, context_ref=cref, pose=pose)[0].detach()
    for p_ in lora:
        p_.requires_grad_(False)
    err = rel(fused, module)
    print(f"C = {C}: fused (folded) vs module route (branches): {err:.3e}")
    assert err < TOL_DEEP
    with routes.override(library_linear=True):  # and the module route on the library GEMM with torch's adapter arithmetic
        assert not blk.fused_ready(x)
        assert rel(fused, blk(x, context=ctx, context_ref=cref, pose=pose)[0]) < TOL_DEEP
    blk.attn2.cache_context_kv = True
    a = blk(x, context=ctx, context_ref=cref, pose=pose)[0]
    for name in ("attn1.to_v_attn3_up", "attn2.to_k_attn3_up", "attn2.to_q_attn3_down"):
        w = blk.get_submodule(name).weight
        w.add_(torch.full_like(w, 0.05))  # what an optimizer step does (in place: same storage, new version)
        b = blk(x, context=ctx, context_ref=cref, pose=pose)[0]
        assert rel(b, a) > 1e-3, name
        a = b
    blk.attn2.cache_context_kv = False


@torch.no_grad()
def test_steady_sampling_step_with_adapters_launches_no_extra_kernels():
    """The merge is paid once, not per step: after a warm-up forward, a steady fused forward of the block launches the same cd360 kernels
    with add_lora as without, and neither the packs nor the cached text K / V are rebuilt."""
    gi = load("block_lora_eval")
    x, ctx, cref, pose = _b16(gi["x"]), _b16(gi["ctx"]), _b16(gi["cref"]), unpack_cameras(gi["cams"])
    launches = []
    for lora in (False, True):
        from sgm.modules.attention import BasicTransformerBlock
        blk = BasicTransformerBlock(64, 1, 64, context_dim=32, checkpoint=False, attn_mode="softmax-xformers", image_cross=True, far=2, num_samples=4,
                                    rgb_predict=True, mode="feature-nerf", stratified=True, add_lora=lora).eval()
        W.load_into(blk, seed=2)
        blk = blk.to(DEV, BF)
        blk.attn2.cache_context_kv = True
        blk(x, context=ctx, context_ref=cref, pose=pose)
        pack, kv = blk._pack, blk.attn2._kv_cache
        ops.profile_start()
        blk(x, context=ctx, context_ref=cref, pose=pose)
        prof = ops.profile_stop()
        assert blk._pack is pack and blk.attn2._kv_cache is kv
        launches.append({k: v["n"] for k, v in prof.items()})
    assert launches[0] == launches[1], launches
    assert not any("lowrank" in k for k in launches[1])


# ------------------------------------------------------------------------------------------------ fine-tuning
def _tiny(lora=True):
    from make_golden_params import UNET_TINY
    from sgm.modules.diffusionmodules.openaimodel import UNetModel
    torch.manual_seed(3)
    net = UNetModel(**{**UNET_TINY, "add_lora": lora, "use_prev_weights_imp_sample": False})
    W.load_into(net, seed=4)
    return net.to(DEV, BF)


def _batch(seed=5, b=2, n=2, L=16):
    from cd360 import synth
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)
    return dict(noised=rn(b, 4, L, L), timesteps=torch.full((b,), 500.0, device=DEV), context=rn(b + b * n, 77, 32), y=rn(b + b * n, 16),
                pose=synth.pose_batch(b, n, seed=3), input_ref=rn(b, n, 4, L, L), sigmas_ref=torch.full((b,), 3.0, device=DEV),
                target=rn(b, 4, L, L), target_rgb=rn(b, 3, 8 * L, 8 * L).clamp(-1, 1), w=torch.full((b, 1, 1, 1), 0.7, device=DEV),
                mask=torch.ones(b, 1, L, L, device=DEV), opacity=torch.sigmoid(3 * rn(b, 1, 8 * L, 8 * L)))


def _loss_fn():
    from make_golden_params import LOSS_CFG
    from sgm.util import instantiate_from_config
    return instantiate_from_config({"target": "sgm.modules.diffusionmodules.loss.StandardDiffusionLossImgRef", "params": LOSS_CFG})


def test_train_step_with_adapters_trains_them_and_replays_like_eager():
    import copy
    from cd360 import finetune
    net = _tiny()
    net.train()
    names = finetune.select_trainable(net, "poseattn")
    adapters = [k for k in names if "_attn3_" in k]
    assert len(adapters) == 16 * len([m for m in net.modules() if getattr(m, "add_lora", False) and hasattr(m, "pose_emb_layers")])
    loss_fn, batch = _loss_fn(), _batch()
    params = dict(net.named_parameters())
    before = {k: params[k].detach().clone() for k in adapters}
    opt = finetune.MasterAdamW(finetune.optimizer_param_groups(net, "poseattn", lr=1e-3), lr=1e-3)
    assert opt.fused
    loss = float(finetune.train_step(net, loss_fn, opt, **batch)[0])  # adapter dropout p = 0.1, masks drawn in the kernel
    assert np.isfinite(loss)
    assert all(params[k].grad is not None and torch.isfinite(params[k].grad.float()).all() for k in adapters)
    assert all(not torch.equal(params[k], before[k]) for k in adapters if "_up" in k)  # the zero-init up weights move first
    # eager vs graph replay with p = 0 (eval-mode raymarchers: no jitter)
    net.eval()
    for m in net.modules():
        if hasattr(m, "dropouto"):
            for w in "qkvo":
                getattr(m, f"dropout{w}").p = 0.0
    start = copy.deepcopy({k: v for k, v in net.state_dict().items() if "pose" in k or "attn" in k})
    opt = finetune.MasterAdamW(finetune.optimizer_param_groups(net, "poseattn", lr=1e-4), lr=1e-4)
    eager = [float(finetune.train_step(net, loss_fn, opt, **batch)[0]) for _ in range(4)]
    net.load_state_dict(start, strict=False)
    opt = finetune.MasterAdamW(finetune.optimizer_param_groups(net, "poseattn", lr=1e-4), lr=1e-4)
    step = finetune.GraphedTrainStep(net, loss_fn, opt, batch, warmup=2)
    graphed = [float(step()[0]) for _ in range(2)]
    print("eager:", eager, "graph (steps 3-4):", graphed)
    assert all(abs(a - e) <= 1e-3 * abs(e) for a, e in zip(graphed, eager[2:]))


def test_lowrank_add_bandwidth_report():
    """Reported, not asserted against a target: time and achieved bytes/s of the q|k|v adapter add of a 32^2-level (M = 3 x 1024,
    N = 3 x 1280) and a 64^2-level (M = 3 x 4096, N = 3 x 640) pose block of a CFG x 3 batch, r = 32, in place."""
    g = torch.Generator(device=DEV).manual_seed(1)
    for M, N in ((3 * 1024, 3 * 1280), (3 * 4096, 3 * 640)):
        t, u, base = rnd(M, 32, g=g), rnd(N, 32, g=g, scale=0.1), rnd(M, N, g=g)
        for _ in range(3):
            ops.lowrank_add(t, u, base=base, out=base)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 50
        e0.record()
        for _ in range(reps):
            ops.lowrank_add(t, u, base=base, out=base)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / reps
        nbytes = 2 * (2 * M * N + M * 32 + N * 32)
        print(f"lowrank_add M={M} N={N} r=32: {us:.1f} us, {nbytes / us / 1e6:.2f} TB/s")
        assert us > 0
