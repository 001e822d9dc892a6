"""Fine-tuning glue around the pose path: what the reference's Lightning engine and callbacks do to the UNet between training
steps and the sampling path.  pytorch_lightning is not part of the drop-in; these are plain functions on the
UNet module that an engine (or a test) calls.

  select_trainable          diffusion.py:117-150   which parameters train for trainkeys in {poseattn, pose, all}
  combine_losses            diffusion.py:226-241   lambda-weighted total of the four loss terms, gated by drop_im
  register_reference_hooks  diffusion.py:28-41,151-163   forward hooks that keep the pose blocks' outputs on reference images
  harvest_references        main.py:596-607        concatenate, all-gather over ranks (RCCL `nccl` / gloo), interleave, register
                                                   the `references` buffer the sampling path reads (sample.py:91)
  delta_state_dict          main.py:611-624        the delta checkpoint: pose parameters (no raymarcher buffers) + references
  load_delta_state_dict     sgm/util.py:227-240    its inverse on a freshly built UNet
  optimizer_param_groups    diffusion.py:310-361   the optimiser groups (pose parameters at lr, attention / remaining weights at multiplier * lr)
  MasterAdamW / train_step  diffusion.py:226-262   one optimisation step of the fine-tuning loop: UNet forward (HIP kernels), the four
                                                   loss terms, backward (HIP backward kernels via cd360/grad.py), AdamW on fp32 master
                                                   copies of the trainable (bf16) parameters
  NoiseStage / train_step_latents / encode_batch   loss.py:146-168, denoiser.py:22-44, diffusion.py:238-249   the same step from CLEAN
                                                   latents and a seed: sigma draws, noising and scaling in front of the UNet and the l2
                                                   term behind it as HIP launches (include/train/cd360_train.h), graph-safe

The all-gather in harvest_references is the one exchange step of the training side: each rank holds the features of its share
of the reference images ([N_local, hw, C] per pose block, 12 blocks) and every rank needs all of them in dataset order
(DistributedSampler gives sample i to rank i % world, hence the transpose before flattening).  It is issued once per
validation epoch on ~2 GB of bf16 features at 1024^2, as ONE collective per block over xGMI.
"""
from __future__ import annotations

import collections
import contextlib
from typing import Dict, List, Optional

import torch
import torch.distributed as dist

from .sampling import pose_blocks


# ---------------------------------------------------------------- which parameters train
def select_trainable(unet: torch.nn.Module, trainkeys: str = "pose") -> List[str]:
    """Sets requires_grad exactly as diffusion.py:117-150 and returns the names left trainable.  Call it BEFORE any grad-enabled forward:
    freshly constructed modules have every parameter trainable, and the HIP path refuses (NotImplementedError) to run a trainable
    convolution / norm affine it cannot differentiate."""
    named = list(unet.named_parameters())
    if trainkeys == "poseattn":
        blocks = []
        for name, p in named:
            if not ("pose" in name or "transformer_blocks" in name):
                p.requires_grad = False
            elif "pose" in name:
                p.requires_grad = True
                blocks.append(name.split(".pose")[0])
        blocks = set(blocks)
        for name, p in named:
            if "transformer_blocks" in name:
                hit = any(b in name and ("attn1" in name or "attn2" in name or "pose" in name) for b in blocks)
                p.requires_grad = bool(hit)
    elif trainkeys == "pose":
        for name, p in named:
            p.requires_grad = "pose" in name
    elif trainkeys == "all":
        # the reference accepts it (diffusion.py:117-150) and so does this function -- off the hand-written path: trainable convolutions
        # run on torch's own convolution, the GroupNorm / LayerNorm affine gradients are fp32 torch reductions
        import warnings
        warnings.warn("trainkeys='all': convolution weights train through torch's convolution and the GroupNorm / LayerNorm affine gradients "
                      "through torch reductions -- correct, but not the hand-written path the shipped configs ('pose' / 'poseattn') run on",
                      stacklevel=2)
        for _, p in named:
            p.requires_grad = True
    else:
        raise ValueError(f"unknown trainkeys {trainkeys!r}")
    return [n for n, p in named if p.requires_grad]


def optimizer_param_groups(unet: torch.nn.Module, trainkeys: str = "pose", lr: float = 1e-4, multiplier: float = 0.05) -> List[dict]:
    """The optimiser groups of DiffusionEngine.configure_optimizers (diffusion.py:310-361) for the UNet: the pose parameters at
    `lr`; for 'poseattn' the attn1 / attn2 weights of the pose blocks, and for 'all' every other parameter, at `multiplier * lr`
    (configs/train_co3d_concept.yaml:2,7-8: lr 1e-4, multiplier 0.05).  Each group also lists its parameter `names`."""
    named = list(unet.named_parameters())
    main = [(n, p) for n, p in named if "pose" in n]
    low = []
    if trainkeys == "poseattn":
        blocks = {n.split(".pose")[0] for n, _ in main}
        low = [(n, p) for n, p in named if "transformer_blocks" in n and "pose" not in n and ("attn1" in n or "attn2" in n)
               and any(b in n for b in blocks)]
    elif trainkeys == "all":
        low = [(n, p) for n, p in named if "pose" not in n]
    elif trainkeys != "pose":
        raise ValueError(f"unknown trainkeys {trainkeys!r}")
    groups = [{"params": [p for _, p in main], "lr": lr, "names": [n for n, _ in main]}]
    if low:
        groups.append({"params": [p for _, p in low], "lr": multiplier * lr, "names": [n for n, _ in low]})
    return groups


# ---------------------------------------------------------------- loss weighting
def combine_losses(loss, loss_fg, loss_bg, loss_rgb, drop_im, *, rgb: bool = True, rgb_predict: bool = True, global_step: int = 1,
                   loss_fg_lambda: float = 10.0, loss_bg_lambda: float = 10.0, loss_rgb_lambda: float = 5.0, as_tensors: bool = False):
    """DiffusionEngine.forward (diffusion.py:226-241).  `drop_im` [b] is 1 where the sample kept its reference images; the
    render losses only count those samples.  Defaults are configs/train_co3d_concept.yaml:9-11.
    as_tensors=True: the logged terms stay 0-d device tensors and the `loss_rgb.mean() > 0` test of the reference becomes a device-side
    select (torch.where: a zero or NaN rgb term contributes nothing to the total, as skipping it does) -- no host synchronisation between
    the forward and the backward pass, and the step can be captured into a hipGraph.  The skipped term's GRADIENT is an exact zero on the
    product route too: `cd360_render_loss_bwd_f32` writes 0 (not 0 * NaN) where the upstream gradient of the rgb term is 0
    (tests/test_backward_gpu.py::test_render_loss_skipped_rgb_term_has_zero_gradient).  The op-by-op torch route kept for A/B
    (`routes.no_train_fusions`) has torch's semantics there: 0 * NaN = NaN."""
    total = loss.mean()
    out = {"loss": total.detach()}
    den = drop_im.sum() + 1e-12
    if rgb and global_step > 0:
        fg = (loss_fg.mean(1) * drop_im.reshape(-1)).sum() / den
        bg = (loss_bg.mean(1) * drop_im.reshape(-1)).sum() / den
        total = total + loss_fg_lambda * fg + loss_bg_lambda * bg
        out["loss_fg"], out["loss_bg"] = fg.detach(), bg.detach()
    if rgb_predict and (as_tensors or loss_rgb.mean() > 0):
        lr = (loss_rgb.mean(1) * drop_im.reshape(-1)).sum() / den
        if as_tensors:  # the reference's `if loss_rgb.mean() > 0` without a host read: a NaN (or zero) rgb term is skipped, not added
            lr = torch.where(loss_rgb.mean() > 0, lr, torch.zeros_like(lr))
        total = total + loss_rgb_lambda * lr
        out["loss_rgb"] = lr.detach()
    if not as_tensors:
        out = {k: float(v) for k, v in out.items()}
    return total, out


# ---------------------------------------------------------------- references harvest
def _is_pose_block_name(name: str) -> bool:
    parts = name.split(".")
    return len(parts) > 1 and parts[-2] == "transformer_blocks"


def register_reference_hooks(unet: torch.nn.Module):
    """-> (activations, handles).  A pose block called WITHOUT a pose (the `onlyref` validation pass over the reference images)
    returns `(x, None, None, None, None)`; the hook keeps `x` (diffusion.py:28-41: only when out[1] is None)."""
    activations: Dict[str, list] = collections.defaultdict(list)
    handles = []

    def hook(name, _module, _inp, out):
        if isinstance(out, tuple) and out[1] is None:
            activations[name].append(out[0].detach())

    for name, module in unet.named_modules():
        if _is_pose_block_name(name) and hasattr(module, "pose_emb_layers"):
            handles.append(module.register_forward_hook(lambda m, i, o, name=name: hook(name, m, i, o)))
    return activations, handles


def remove_hooks(handles) -> None:
    for h in handles:
        h.remove()


def harvest_references(unet: torch.nn.Module, activations: Dict[str, list], group: Optional[dist.ProcessGroup] = None) -> Dict[str, torch.Tensor]:
    """main.py:596-607.  Every rank must have run the same number of reference images.  Returns {block name: references}."""
    world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
    out = {}
    for name, module in unet.named_modules():
        if not (_is_pose_block_name(name) and hasattr(module, "pose_emb_layers")):
            continue
        if not activations.get(name):
            raise RuntimeError(f"no reference activations were recorded for {name} (run the reference images with pose=None first)")
        local = torch.cat(activations[name]).contiguous()
        if world > 1:
            gathered = [torch.empty_like(local) for _ in range(world)]
            dist.all_gather(gathered, local, group=group)
            refs = torch.stack(gathered).transpose(0, 1).reshape(-1, *local.shape[1:])  # "(b n) ..." with n = rank
        else:
            refs = local
        if "references" in module._buffers:
            module._buffers["references"] = refs
        else:
            module.register_buffer("references", refs)
        out[name] = refs
    return out


# ---------------------------------------------------------------- delta checkpoint
def delta_state_dict(state_dict: Dict[str, torch.Tensor], embeds: Optional[list] = None) -> Dict[str, object]:
    """main.py:611-624: keys containing 'pose' (but not the raymarcher buffers) and the `references` buffers; `embed` carries
    the two new-token embedding rows of the text encoders when the caller has them (they live outside the UNet)."""
    delta = {k: v for k, v in state_dict.items() if ("pose" in k and "raymarcher" not in k) or "references" in k}
    if embeds is not None:
        delta["embed"] = list(embeds)
    return delta


def load_delta_state_dict(unet: torch.nn.Module, sd_delta: Dict[str, object], prefix: str = "model.diffusion_model.") -> List[str]:
    """sgm/util.py:227-240 for the UNet part: registers each pose block's `references` buffer, loads the pose parameters,
    returns the unexpected keys.  `sd_delta` is not modified."""
    sd = {k: v for k, v in sd_delta.items() if k != "embed"}
    for name, module in unet.named_modules():
        if _is_pose_block_name(name) and hasattr(module, "pose_emb_layers"):
            key = f"{prefix}{name}.references"
            if key not in sd:
                raise KeyError(f"delta checkpoint has no {key}")
            ref = sd.pop(key).to(next(module.parameters()).device)
            if "references" in module._buffers:
                module._buffers["references"] = ref
            else:
                module.register_buffer("references", ref)
    stripped = {k[len(prefix):] if k.startswith(prefix) else k: v for k, v in sd.items()}
    _missing, unexpected = unet.load_state_dict(stripped, strict=False)
    return list(unexpected)


def load_delta_embeddings(conditioner: torch.nn.Module, embed) -> None:
    """sgm/util.py:216-230 for the conditioner part: `embed` = sd_delta["embed"], the trained modifier rows of the two prompt encoders
    (embed[0] for conditioner.embedders[0], FrozenCLIPEmbedder; embed[1] for embedders[1], FrozenOpenCLIPEmbedder; each [k, D]).  The
    reference sets every token table to torch.cat([checkpoint table without modifier rows, embed[i]]).  Here the embedder already holds
    its k modifier rows (appended at construction): the LAST k rows of its table are overwritten; a table that holds none yet (an embedder
    built without modifier_token) gets them appended.  `embed` and its tensors are not modified."""
    for emb, rows in zip(conditioner.embedders[:2], embed):
        table = emb._tables()[0]
        rows = rows.detach().to(table.device, table.dtype)
        if rows.dim() != 2 or rows.shape[1] != table.shape[1]:
            raise ValueError(f"delta embedding rows {tuple(rows.shape)} for a token table of width {table.shape[1]}")
        k = rows.shape[0]
        held = len(getattr(emb, "modifier_token_id", None) or ())
        if held not in (0, k):
            raise ValueError(f"{type(emb).__name__} holds {held} modifier rows, the delta checkpoint {k}")
        with torch.no_grad():
            if held:
                table[table.shape[0] - k:].copy_(rows)  # in place: the version counter moves and cd360.derived rebuilds what was packed
            else:
                holder = emb.transformer.text_model.embeddings.token_embedding if hasattr(emb, "transformer") else emb.model.token_embedding
                V = table.shape[0]
                holder.weight = torch.nn.Parameter(torch.cat([table.detach(), rows], 0), requires_grad=table.requires_grad)
                holder.num_embeddings = V + k
                emb.modifier_token_id = list(range(V, V + k))


class TokenRows(torch.nn.Module):
    """The trainable modifier-token rows of a conditioner's prompt encoders (train_tokens): `parameters()` are the rows, one [k, D] leaf per
    marked embedder in the order of conditioner.embedders -- one more optimiser group for MasterAdamW (bf16 on the GPU: its fused path).
    The embedders are held, not owned: they stay the conditioner's sub-modules."""

    def __init__(self, embedders, rows):
        super().__init__()
        self.rows = torch.nn.ParameterList(rows)
        self.__dict__["embedders"] = list(embedders)

    def embeds(self) -> List[torch.Tensor]:
        """Copies of the rows, the list delta_state_dict(embeds=) stores and load_delta_embeddings reads."""
        return [r.detach().clone() for r in self.rows]

    @torch.no_grad()
    def sync(self) -> None:
        """Write the rows into the last k rows of the embedders' token tables, in place (the version counter moves): for sampling under
        no_grad after training.  A grad-enabled forward of a marked embedder does the same on its own."""
        for emb, r in zip(self.embedders, self.rows):
            table = emb._tables()[0]
            table[table.shape[0] - r.shape[0]:].copy_(r)


def train_tokens(conditioner: torch.nn.Module) -> TokenRows:
    """Opt in to training the modifier-token embeddings (sgm/models/diffusion.py:342-355 hands both token tables to the optimiser;
    modules.py:499-511, 724-730 lets the gradient through at the modifier positions only; the delta checkpoint keeps exactly those rows).
    For each of conditioner.embedders[:2] with `modifier_token_id`: a leaf parameter [k, D] holding the last k rows of its token table, in the
    table's dtype and on its device (call this AFTER moving the conditioner), requires_grad=True; the table itself is set to
    requires_grad=False and the embedder is marked (`embedder.token_rows`, kept out of its parameters and its state dict).  A marked
    embedder called with grad enabled runs cd360.grad.TextTowerFn on the HIP route, the masked embedding on the torch route.  An embedder
    without modifier tokens is skipped; ValueError if none has any.  Unlike the reference, only these k rows are optimiser parameters (its
    whole 49409-row tables are, their other rows receiving zero gradient and weight decay only, and the delta checkpoint drops them)."""
    marked, rows = [], []
    for emb in list(conditioner.embedders)[:2]:
        k = len(getattr(emb, "modifier_token_id", None) or ())
        if not k:
            continue
        table = emb._tables()[0]
        r = torch.nn.Parameter(table.detach()[table.shape[0] - k:].clone().contiguous(), requires_grad=True)
        table.requires_grad = False
        emb.__dict__["token_rows"] = r
        marked.append(emb)
        rows.append(r)
    if not rows:
        raise ValueError("train_tokens: no prompt encoder of this conditioner has modifier tokens (modifier_token is None)")
    return TokenRows(marked, rows)


# ---------------------------------------------------------------- one optimisation step
class MasterAdamW:
    """AdamW (configs/train_co3d_concept.yaml: optimizer_config AdamW) on fp32 master copies of the trainable parameters: the HIP
    path keeps the UNet in bf16, and a bf16 parameter cannot absorb updates of lr ~ 1e-5 (its spacing near 1 is 8e-3), so the
    optimiser state and the accumulated weights live in fp32 and the bf16 parameters are refreshed from them after every step.
    bf16 parameters on the GPU take the fused path: masters and both moments in three flat fp32 buffers, the whole update (gradient
    read, decay, moments, bias-corrected step, bf16 write-back) in one pass of cd360_adamw_bf16 with the step count on the device
    (graph-capturable as it is).  Anything else (CPU, fp32 parameters, amsgrad / maximize) runs torch.optim.AdamW on the masters.

    max_grad_norm / ema_decay / live (all None: the object above, launch for launch).  Any of them set selects, on the fused path, the
    LIVE step of include/optim/cd360_optim.h: lr and weight decay are read by the kernel from a device table that `sync_hyper()` refreshes
    from `param_groups` (so a schedule reaches the replays of a captured step), `max_grad_norm` clips the global L2 norm of the gradients
    as torch.nn.utils.clip_grad_norm_ does (one read-only pass for the norm, the factor applied inside the update; `grad_norm` and
    `clip_coef` are 0-d device views, never read on the host), and `ema_decay` keeps LitEma's moving average (sgm/modules/ema.py,
    use_num_upates=True) of the weights inside the same pass.  The shadows are fp32 where LitEma keeps the parameter dtype, for the reason
    the masters exist: one EMA update moves a weight by (1 - decay) * delta ~ 1e-4 * delta, far below bf16's spacing, so a bf16 shadow
    would never move.  `ema_scope()` swaps the averaged weights in, `ema_state_dict()` returns them.  Tensors without a gradient in a step
    are skipped by that step, their shadows included.  The torch fall-back honours max_grad_norm (clip_grad_norm_ on the fp32 master
    gradients) and ema_decay (the same formula in torch) too."""

    def __init__(self, params, lr: float = 1e-5, fused: Optional[bool] = None, max_grad_norm: Optional[float] = None,
                 ema_decay: Optional[float] = None, live: Optional[bool] = None, **kw):
        """`params`: an iterable of parameters, or optimiser groups as returned by optimizer_param_groups (per-group `lr`)."""
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f"max_grad_norm must be >= 0, got {max_grad_norm}")
        if ema_decay is not None and not 0.0 <= float(ema_decay) <= 1.0:
            raise ValueError("Decay must be between 0 and 1")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.live, self.ema, self._ema = False, None, None
        params = list(params)
        if params and isinstance(params[0], dict):
            groups = [{**{k: v for k, v in g.items() if k not in ("params", "names")}, "params": [p for p in g["params"] if p.requires_grad]}
                      for g in params]
        else:
            groups = [{"params": [p for p in params if p.requires_grad]}]
        self.params = [p for g in groups for p in g["params"]]
        can_fuse = (bool(self.params) and all(p.is_cuda and p.dtype == torch.bfloat16 and p.is_contiguous() for p in self.params)
                    and not kw.get("amsgrad") and not kw.get("maximize") and not (set(kw) - {"betas", "eps", "weight_decay", "capturable", "amsgrad",
                                                                                            "maximize", "foreach"}))
        if fused and not can_fuse:
            raise ValueError("MasterAdamW(fused=True) needs bf16 parameters on the GPU and plain AdamW options")
        self.fused = can_fuse if fused is None else bool(fused)
        if self.fused:
            from . import ops
            dev = self.params[0].device
            begin, total = [], 0
            for p in self.params:
                begin.append(total)
                total += (p.numel() + 7) // 8 * 8  # every tensor starts on a 32-byte boundary of the flat buffers
            self._master = torch.zeros(total, dtype=torch.float32, device=dev)
            self.exp_avg, self.exp_avg_sq = torch.zeros_like(self._master), torch.zeros_like(self._master)
            self.steps = torch.zeros((), dtype=torch.float32, device=dev)  # steps taken; on the device so that graph replays advance it
            self.master = [self._master[b:b + p.numel()].view(p.shape) for b, p in zip(begin, self.params)]
            for m, p in zip(self.master, self.params):
                m.copy_(p.detach())
            self.betas, self.eps = tuple(kw.get("betas", (0.9, 0.999))), float(kw.get("eps", 1e-8))
            self.param_groups = [{"lr": g.get("lr", lr), "weight_decay": g.get("weight_decay", kw.get("weight_decay", 1e-2)), "n": len(g["params"])}
                                 for g in groups]  # edit lr / weight_decay here (a captured graph keeps the values it was captured with)
            self._begin, self._plan, self._plan_key, self.opt, self.capturable = begin, None, None, None, True
            self._ops = ops
            if self.max_grad_norm is not None or self.ema_decay is not None or live:
                self._init_live(dev, begin, total)
            return
        self.master = [p.detach().float().clone() for p in self.params]
        it = iter(self.master)
        kw.pop("foreach", None)
        self.opt = torch.optim.AdamW([{**g, "params": [next(it) for _ in g["params"]]} for g in groups], lr=lr, **kw)
        self.param_groups = self.opt.param_groups
        self.capturable = all(g.get("capturable") for g in self.opt.param_groups)
        if self.ema_decay is not None:
            self.ema = [m.clone() for m in self.master]  # LitEma.__init__ clones the parameters
            self._ema_updates = torch.zeros((), dtype=torch.float32, device=self.master[0].device) if self.master else None
        if self.max_grad_norm is not None:
            self.grad_norm = self.clip_coef = None  # set by step()

    def _init_live(self, dev, begin, total) -> None:
        """State of the live step: the (lr, weight decay) table, one row per tensor, in pinned host memory and on the device; the partial
        sums and the 4 values (sumsq, norm, coef, 0) of the clip kernels; the flat fp32 EMA, initialised from the masters."""
        self.live = True
        n = len(self.params)
        self._hyper_host = torch.zeros(n, 2, dtype=torch.float32).pin_memory()
        self._hyper_dev = torch.zeros(n, 2, dtype=torch.float32, device=dev)
        self._hyper_vals, self._hyper_event = None, None
        chunks = (n + self._ops.ADAMW_MAX_TENSORS - 1) // self._ops.ADAMW_MAX_TENSORS
        self._partials = torch.zeros(self._ops.sumsq_partials([total]) + chunks, dtype=torch.float32, device=dev)  # enough for any subset of the tensors
        self._clip_out = torch.zeros(4, dtype=torch.float32, device=dev)
        self.grad_norm, self.clip_coef = self._clip_out[1], self._clip_out[2]  # written by step() when max_grad_norm is set
        if self.ema_decay is not None:
            self._ema = self._master.clone()
            self.ema = [self._ema[b:b + p.numel()].view(p.shape) for b, p in zip(begin, self.params)]
        self.sync_hyper()

    def sync_hyper(self) -> bool:
        """The live step reads lr and weight decay from a device table: compare `param_groups` with the table's host copy and, on a change,
        rewrite it and queue ONE non-blocking copy on the current stream.  Called by the eager step() and by GraphedTrainStep before every
        replay; never captured.  Returns whether a copy was queued (always False for an optimiser that is not live)."""
        if not self.live:
            return False
        vals = [(float(g["lr"]), float(g["weight_decay"])) for g in self.param_groups for _ in range(g["n"])]
        if vals == self._hyper_vals:
            return False
        if self._hyper_event is not None:
            self._hyper_event.synchronize()  # the previous copy has read the pinned rows before they are rewritten
        self._hyper_host.copy_(torch.tensor(vals, dtype=torch.float32).view(-1, 2))
        self._hyper_dev.copy_(self._hyper_host, non_blocking=True)
        self._hyper_event = torch.cuda.Event()
        self._hyper_event.record()
        self._hyper_vals = vals
        return True

    @contextlib.contextmanager
    def ema_scope(self):
        """The engine's ema_scope (sgm/models/diffusion.py:291-303): inside, the parameters hold the averaged weights (rounded to the
        parameter dtype); on exit they hold the masters again.  Every weight cache keyed on `_version` is invalidated both times."""
        if self.ema is None:
            raise ValueError("ema_scope: this optimiser was built without ema_decay")
        with torch.no_grad():
            for p, e in zip(self.params, self.ema):
                p.copy_(e)
            self.bump_versions()
        try:
            yield self
        finally:
            with torch.no_grad():
                for p, m in zip(self.params, self.master):
                    p.copy_(m)
                self.bump_versions()

    def ema_state_dict(self, names) -> Dict[str, torch.Tensor]:
        """{name: fp32 shadow} for a checkpoint; `names` in the order of the optimiser's parameters."""
        names = list(names)
        if self.ema is None:
            raise ValueError("ema_state_dict: this optimiser was built without ema_decay")
        if len(names) != len(self.ema):
            raise ValueError(f"ema_state_dict: {len(names)} names for {len(self.ema)} tensors")
        return {k: e.detach().clone() for k, e in zip(names, self.ema)}

    def _live_plan(self, active):
        key = tuple(active)
        if self._plan_key != key:
            self._plan = self._ops.LiveAdamwPlan([self.params[i] for i in active], [self._begin[i] for i in active], list(active))
            self._plan_key = key
        return self._plan

    def bump_versions(self, active=None) -> None:
        """The fused kernel (and a hipGraph replay of it) writes the bf16 parameters through raw pointers, which torch's version counter
        does not see.  Every derived-weight cache of the package (LayerNorm-folded packs, W^T copies, fp32 biases, the FeatureNeRF's fused
        weights, the pose-projection split) is keyed on `_version`, so the update is made visible here -- no kernel is launched."""
        for i in (range(len(self.params)) if active is None else active):
            torch.autograd.graph.increment_version(self.params[i])

    allreduce_single = False  # True: run the gradient all-reduce even in a group of one (tests of the collective path on a 1-GPU box)

    def zero_grad(self) -> None:
        for p in self.params:
            p.grad = None

    @torch.no_grad()
    def allreduce_grads(self, group: Optional[dist.ProcessGroup] = None) -> None:
        """Data-parallel fine-tuning (the reference trains under Lightning DDP, main.py): average the gradients of the trainable
        parameters over the ranks as ONE flat fp32 all-reduce (66.7 M values = 267 MB at SDXL size: a single RCCL ring over xGMI,
        per-link bound, instead of 96 small collectives).  No-op without an initialised process group."""
        if not (dist.is_available() and dist.is_initialized()) or (dist.get_world_size(group) == 1 and not self.allreduce_single):
            return
        grads = [p.grad for p in self.params]
        if any(g is None for g in grads):
            raise RuntimeError("allreduce_grads: a trainable parameter has no gradient on this rank (ranks would disagree on the buffer layout)")
        flat = torch.cat([g.reshape(-1).float() for g in grads])
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
        flat.div_(dist.get_world_size(group))
        off = 0
        for p, g in zip(self.params, grads):
            n = g.numel()
            p.grad = flat[off:off + n].reshape(g.shape).to(g.dtype)
            off += n

    def _fused_plan(self, active):
        lrs = [g["lr"] for g in self.param_groups for _ in range(g["n"])]
        wds = [g["weight_decay"] for g in self.param_groups for _ in range(g["n"])]
        key = (tuple(active), tuple(lrs), tuple(wds))
        if self._plan_key != key:
            self._plan = self._ops.AdamwPlan([self.params[i] for i in active], [self._begin[i] for i in active], [lrs[i] for i in active],
                                             [wds[i] for i in active])
            self._plan_key = key
        return self._plan

    @torch.no_grad()
    def step(self, group: Optional[dist.ProcessGroup] = None) -> None:
        self.allreduce_grads(group)
        if self.fused:
            # parameters without a gradient are skipped as torch does; the step count is one per optimiser, not one per tensor
            active = [i for i, p in enumerate(self.params) if p.grad is not None]
            if active and self.live:
                if not torch.cuda.is_current_stream_capturing():
                    self.sync_hyper()
                grads = [self.params[i].grad if self.params[i].grad.is_contiguous() else self.params[i].grad.contiguous() for i in active]
                plan, coef = self._live_plan(active), None
                if self.max_grad_norm is not None:
                    coef = self._ops.grad_clip_coef(plan, grads, self._partials, self.max_grad_norm, self._clip_out)[2]
                self._ops.adamw_live_step(plan, grads, self._hyper_dev, self._master, self.exp_avg, self.exp_avg_sq, self.steps, self.betas[0],
                                          self.betas[1], self.eps, coef=coef, ema=self._ema, ema_decay=self.ema_decay or 0.0)
                self.bump_versions(active)
            elif active:
                grads = [self.params[i].grad if self.params[i].grad.is_contiguous() else self.params[i].grad.contiguous() for i in active]
                self._ops.adamw_step(self._fused_plan(active), grads, self._master, self.exp_avg, self.exp_avg_sq, self.steps, self.betas[0],
                                     self.betas[1], self.eps)
                self.bump_versions(active)
            return
        for m, p in zip(self.master, self.params):
            m.grad = None if p.grad is None else p.grad.float()
        if self.max_grad_norm is not None:
            with_grad = [m for m in self.master if m.grad is not None]
            if with_grad:
                self.grad_norm = torch.nn.utils.clip_grad_norm_(with_grad, self.max_grad_norm)
                self.clip_coef = torch.clamp(self.max_grad_norm / (self.grad_norm + 1e-6), max=1.0)
        self.opt.step()
        if self.ema is not None and any(m.grad is not None for m in self.master):
            t = self._ema_updates.add_(1.0)  # LitEma.forward with use_num_upates=True, one fp32 operation at a time
            omd = 1.0 - torch.clamp((1.0 + t) / (10.0 + t), max=self.ema_decay)
            for e, m in zip(self.ema, self.master):
                if m.grad is not None:
                    e.sub_(omd * (e - m))
        for m, p in zip(self.master, self.params):
            p.copy_(m)


class LRSchedule:
    """torch.optim.lr_scheduler.LambdaLR's rule, lr = initial_lr * schedule(n), on the `param_groups` of a MasterAdamW (which LambdaLR
    rejects: the class is not a torch Optimizer): applied at construction with n = 0 and at every step().  `schedule`: a callable of the
    step number, e.g. one of sgm/lr_scheduler.py (DiffusionEngine.configure_optimizers, sgm/models/diffusion.py:362-374)."""

    def __init__(self, optimizer, schedule):
        self.optimizer, self.schedule, self.n = optimizer, schedule, 0
        for g in optimizer.param_groups:
            g.setdefault("initial_lr", g["lr"])
        self.base_lrs = [g["initial_lr"] for g in optimizer.param_groups]
        self._apply()

    def _apply(self) -> None:
        for g, base in zip(self.optimizer.param_groups, self.base_lrs):
            g["lr"] = base * self.schedule(self.n)

    def step(self) -> None:
        self.n += 1
        self._apply()

    def get_last_lr(self) -> List[float]:
        return [g["lr"] for g in self.optimizer.param_groups]


_ADAPTERS = {}  # id(unet) -> (module epoch, whether any attention module carries add_lora adapters)


def _has_adapters(unet: torch.nn.Module) -> bool:
    from sgm.modules.attention import _module_epoch
    ent = _ADAPTERS.get(id(unet))
    if ent is None or ent[0] != _module_epoch[0]:
        ent = _ADAPTERS[id(unet)] = (_module_epoch[0], any(getattr(m, "add_lora", False) for m in unet.modules()))
    return ent[1]


def train_step(unet: torch.nn.Module, loss_fn, optimizer, *, noised, timesteps, context, y, pose, input_ref, sigmas_ref, target, target_rgb,
               w, mask, opacity, drop_im=None, mask_ref=None, as_tensors: bool = False, **loss_kw):
    """One step of the fine-tuning loop on already-noised inputs (the engine's denoiser / conditioner / data loading stay outside
    the path): forward, StandardDiffusionLossImgRef.get_loss (loss.py:177-209), the lambda-weighted total
    (diffusion.py:226-241), backward, optimiser step.  Returns (total loss tensor, dict of logged terms).
    The logged terms are read back AFTER the optimiser step has been queued (one host synchronisation per step, at its end, instead of
    four between the forward and the backward pass); as_tensors=True leaves them on the device (no synchronisation at all)."""
    optimizer.zero_grad()
    if _has_adapters(unet):  # new adapter-dropout masks for this step (a captured step advances the offset on every replay)
        from . import ops
        ops.dropout_tick(noised.device)
    out, fgs, alphas, rgbs = unet(noised, timesteps=timesteps, context=context, y=y, pose=pose, input_ref=input_ref, sigmas_ref=sigmas_ref,
                                  mask_ref=mask_ref)
    l2, lfg, lbg, lrgb = loss_fn.get_loss(out, fgs, rgbs, target, target_rgb, w, mask, mask_ref, opacity, alphas)
    if drop_im is None:
        drop_im = torch.ones(noised.shape[0], device=noised.device)
    total, logged = combine_losses(l2, lfg, lbg, lrgb, drop_im, as_tensors=True, **loss_kw)
    total.backward()
    optimizer.step()
    if not as_tensors:
        logged = {k: float(v) for k, v in logged.items()}
    return total.detach(), logged


# ---------------------------------------------------------------- a step from clean latents
class Staged:
    """What NoiseStage.__call__ returns: views of the stage's buffers, valid until its next call.  x_t [B, 4, H, W] fp32 (the noised
    target); x_in (x_t * c_in) and input_ref ([B, n, 4, H, W] or None: the twice-noised reference views * c_in_ref) in the stage's dtype;
    timesteps / sigmas_ref int64 [B] (sigma_to_idx of sigma / sigma_ref: what the UNet embeds); scalars [B, 12] fp32 (cd360._train: sigma,
    w, c_skip, c_out, c_in, sigma_ref, c_in_ref, off_tgt, off_ref); step_used int32 [1]."""

    def __init__(self, stage, x_t, x_in, timesteps, input_ref, sigmas_ref, scalars, step_used):
        self.stage, self.x_t, self.x_in, self.timesteps, self.input_ref, self.sigmas_ref = stage, x_t, x_in, timesteps, input_ref, sigmas_ref
        self.scalars, self.step_used = scalars, step_used

    def l2(self, eps, x0, mask=None):
        from . import ops
        return ops.train_l2(eps, self.x_t, x0, self.scalars, mask)


class NoiseStage:
    """The front and the l2 tail of a training step on the device (include/train/cd360_train.h): what StandardDiffusionLossImgRef.__call__
    and DiscreteDenoiser do around the network -- the sigma draws, the target and offset noise, the two noisings of the reference views,
    c_in / c_out / w, the drop_im zeroing of shared_step -- in two launches in front of the UNet and one (plus one backward) behind it.
    Every random number is a pure function of (seed, stream id of the sample, step, channel, pixel): a hipGraph replay, an eager call and
    any split of the samples over ranks draw the same bits (give each sample its global index as stream id).

    Reads loss_fn.sigma_sampler, loss_fn.sigma_sampler_ref, loss_fn.offset_noise_level and denoiser.sigmas (whose device is the stage's).
    ValueError for anything but CubicSampling / DiscreteSampling, EpsScaling, EpsWeighting and type "l2", and for a loss without a reference sampler:
    a reference index is always drawn.  The reference's denoiser snaps the target sigma to its own table before c_in / c_out; the kernels
    take the sampler's sigma as it is, so a target sampler whose table does not lie ON the denoiser's (possibly_quantize_sigma(s) != s for
    an entry; the shipped config uses the same 1000-entry table for both) is refused too.  sigma_ref is not snapped by the reference either.

    The stage owns the device seed, the stream ids, the step counter and every output buffer (allocated on the first call of a shape, then
    reused), so a captured call keeps reading and writing the same memory: set_step / reseed / set_streams rewrite them in place and reach
    the replays.  A call draws at the step counter's value and, with advance=True (the default), leaves it one higher -- on the device, so
    a replay advances it too.  dtype: what x_in and input_ref are written in -- the dtype UNetModel.forward casts its inputs to."""

    def __init__(self, denoiser, loss_fn, seed: int, streams=None, dtype=torch.bfloat16):
        from sgm.modules.diffusionmodules.sigma_sampling import CubicSampling, DiscreteSampling
        from . import ops
        from .sampler import EpsScaling, EpsWeighting, seed_words

        def named(obj, cls):  # the package's class, or the class of that name an engine instantiated from the YAML target
            return isinstance(obj, cls) or type(obj).__name__ == cls.__name__

        def sampler(s, what):
            if s is None:
                raise ValueError(f"NoiseStage: the loss has no {what} (sigma_sampler_config_ref = None): a reference index is always drawn")
            if named(s, CubicSampling):
                return ops.TRAIN_CUBIC, 0
            if named(s, DiscreteSampling):
                return ops.TRAIN_DISCRETE, int(s.num_idx_start)
            raise ValueError(f"NoiseStage: {what} is a {type(s).__name__}; CubicSampling and DiscreteSampling are served")

        if not named(getattr(denoiser, "scaling", None), EpsScaling):
            raise ValueError(f"NoiseStage: the denoiser's scaling is a {type(getattr(denoiser, 'scaling', None)).__name__}; EpsScaling is served")
        if not named(getattr(denoiser, "weighting", None), EpsWeighting):
            raise ValueError(f"NoiseStage: the denoiser's weighting is a {type(getattr(denoiser, 'weighting', None)).__name__}; EpsWeighting is served")
        if getattr(loss_fn, "type", "l2") != "l2":
            raise ValueError(f"NoiseStage: the loss is of type {loss_fn.type!r}; the stage's tail is the l2 term (stage.l2 stands in for get_loss)")
        self.tgt_kind, self.tgt_start = sampler(loss_fn.sigma_sampler, "sigma_sampler")
        self.ref_kind, self.ref_start = sampler(getattr(loss_fn, "sigma_sampler_ref", None), "sigma_sampler_ref")
        self.level = float(loss_fn.offset_noise_level)
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"NoiseStage: dtype {dtype}; fp32 and bf16 are served")
        self.dtype = dtype
        table = denoiser.sigmas.detach()
        tgt = loss_fn.sigma_sampler.sigmas.detach().to("cpu", torch.float32)
        grid = table.to("cpu", torch.float32)
        if not torch.equal(grid[(tgt[None, :] - grid[:, None]).abs().argmin(0)], tgt):
            raise ValueError("NoiseStage: the target sampler's sigmas do not lie on the denoiser's table (the reference would snap them before c_in / c_out)")
        if not table.is_cuda:
            raise ops.Cd360Error("the training stage runs only on the GPU; the denoiser's sigmas are a CPU tensor")
        dev = self.device = table.device
        f32 = lambda t: t.detach().to(dev, torch.float32).contiguous().clone()
        self.table, self.tgt_table, self.ref_table = f32(table), f32(loss_fn.sigma_sampler.sigmas), f32(loss_fn.sigma_sampler_ref.sigmas)
        self._seed_words = seed_words
        self.seed = torch.tensor([seed_words(seed)], dtype=torch.int64, device=dev)
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)
        self.streams = None if streams is None else torch.tensor([int(v) for v in streams], dtype=torch.int32, device=dev)
        self._buffers, self._last = {}, None

    # ---- the state a captured call reads: rewritten in place
    def set_step(self, k: int) -> None:
        self.step.fill_(((int(k) + 2 ** 31) % 2 ** 32) - 2 ** 31)  # the counter's word is the low 32 bits

    def reseed(self, seed: int) -> None:
        self.seed.fill_(self._seed_words(seed))

    def set_streams(self, ids) -> None:
        ids = [int(v) for v in ids]
        if self.streams is None or self.streams.numel() != len(ids):
            raise ValueError("set_streams: the stage was built with "
                             f"{'no stream ids' if self.streams is None else f'{self.streams.numel()} stream ids'}, got {len(ids)} (a new stage is needed)")
        self.streams.copy_(torch.tensor(ids, dtype=torch.int32))

    def _gpu(self, *ts):
        from . import ops
        for t in ts:
            if t is not None and not t.is_cuda:
                raise ops.Cd360Error("the training stage runs only on the GPU; got a CPU tensor")

    def __call__(self, x0, x_ref=None, drop_im=None, advance: bool = True) -> Staged:
        """x0 [B, 4, H, W] fp32 clean latents; x_ref [B, n, 4, H, W] fp32 clean reference latents or None; drop_im [B] fp32 or None (1 = the
        sample keeps its reference views, 0 = they are zeroed before the noising)."""
        from . import ops
        self._gpu(x0, x_ref, drop_im)
        B = x0.shape[0]
        if self.streams is not None and self.streams.numel() != B:
            raise ValueError(f"{self.streams.numel()} noise stream ids for {B} samples")
        key = (tuple(x0.shape), None if x_ref is None else tuple(x_ref.shape))
        buf = self._buffers.get(key)
        if buf is None:
            dev = self.device
            buf = self._buffers[key] = dict(
                scalars=(torch.zeros((B, ops.TRAIN_ROW), dtype=torch.float32, device=dev), torch.zeros((B,), dtype=torch.int64, device=dev),
                         torch.zeros((B,), dtype=torch.int64, device=dev), torch.zeros((1,), dtype=torch.int32, device=dev)),
                noised=(torch.zeros(x0.shape, dtype=torch.float32, device=dev), torch.zeros(x0.shape, dtype=self.dtype, device=dev),
                        None if x_ref is None else torch.zeros(x_ref.shape, dtype=self.dtype, device=dev)))
        rows, timesteps, ref_idx, step_used = ops.train_sigmas(self.table, self.tgt_table, self.tgt_kind, self.tgt_start, self.ref_table, self.ref_kind,
                                                               self.ref_start, self.seed, self.streams, self.step, B, advance=advance, out=buf["scalars"])
        drop = None if drop_im is None else drop_im.detach().float().contiguous()
        x_t, x_in, xr_in = ops.train_noise(x0.detach(), None if x_ref is None else x_ref.detach(), drop, rows, self.seed, self.streams, step_used,
                                           self.level, dtype=self.dtype, out=buf["noised"])
        self._last = Staged(self, x_t, x_in, timesteps, xr_in, ref_idx, rows, step_used)
        return self._last

    def l2(self, eps, x0, mask=None):
        """The l2 term [B] of the LAST call's noising from the network's output eps (any layout, fp32 or bf16); differentiable in eps."""
        if self._last is None:
            raise ValueError("NoiseStage.l2: the stage has not been called yet")
        self._gpu(eps, x0, mask)
        return self._last.l2(eps, x0, mask)


def encode_batch(first_stage, x, x_ref, seed: int, step: int, streams=None):
    """The two encode_first_stage calls of shared_step (sgm/models/diffusion.py:241-245) on cd360.images.FirstStage: x [B, 3, H, W] ->
    x0 [B, 4, H / 8, W / 8]; x_ref [B, n, 3, H, W] or None -> [B, n, 4, H / 8, W / 8].  The posterior samples are drawn at draw = step.
    streams: one id per sample, the ids NoiseStage is given (the sample's index in the data set, so that the encoder's noise too is the
    sample's own on any split of the batch over ranks); None = the row's index in THIS batch, which is right for one process only: ranks
    that pass None draw the same noise for different images.  Sample s encodes its target in noise stream s (1 + n) and its view v in
    stream s (1 + n) + 1 + v, so no two images of a step share their noise.  Runs outside a captured step: the encoder allocates."""
    B = x.shape[0]
    n = 0 if x_ref is None else x_ref.shape[1]
    ids = list(range(B)) if streams is None else [int(s) for s in streams]
    if len(ids) != B:
        raise ValueError(f"{len(ids)} noise stream ids for {B} samples")
    x0 = first_stage.encode(x, seed, step, streams=[s * (1 + n) for s in ids])
    if x_ref is None:
        return x0, None
    z = first_stage.encode(x_ref.reshape(B * n, *x_ref.shape[2:]), seed, step, streams=[s * (1 + n) + 1 + v for s in ids for v in range(n)])
    return x0, z.reshape(B, n, *z.shape[1:])


def encode_pictures(first_stage, front, pictures, masks, boxes, n_ref: int, seed: int, step: int, streams=None):
    """From decoded frames to clean latents: cd360.pictures.PictureFront.batch (crop, resize, masks: the loader's per-picture arithmetic, on
    the device) and then encode_batch -> (x0, x_ref, batch).  pictures / masks: uint8 device frames [H, W, 3] / [H, W], sample by sample
    with the target first and its n_ref views behind it; boxes: front.boxes(...).  batch["jpg"] is also the loss's target_rgb,
    batch["mask"], batch["depth"] and batch["mask_ref"] are train_step_latents' mask, opacity and mask_ref."""
    batch = front.batch(pictures, masks, boxes, n_ref)
    x0, x_ref = encode_batch(first_stage, batch["jpg"], batch["jpg_ref"] if n_ref else None, seed, step, streams=streams)
    return x0, x_ref, batch


def train_step_latents(unet: torch.nn.Module, loss_fn, optimizer, stage: NoiseStage, *, x0, x_ref, context, y, pose, target_rgb, mask, opacity,
                       drop_im=None, mask_ref=None, as_tensors: bool = False, **loss_kw):
    """One step of the fine-tuning loop from CLEAN latents: stage (sigma draws, noising, scaling: NoiseStage) -> UNet -> the l2 term
    (stage.l2) and the render terms (StandardDiffusionLossImgRef.render_terms) -> the lambda-weighted total -> backward -> optimiser step.
    With FirstStage.encode (encode_batch) and train_tokens this is training_step of the reference's engine.  The step counter of the stage
    advances by one.  Returns as train_step does."""
    optimizer.zero_grad()
    if _has_adapters(unet):
        from . import ops
        ops.dropout_tick(x0.device)
    st = stage(x0, x_ref, drop_im)
    out, fgs, alphas, rgbs = unet(st.x_in, timesteps=st.timesteps, context=context, y=y, pose=pose, input_ref=st.input_ref, sigmas_ref=st.sigmas_ref,
                                  mask_ref=mask_ref)
    l2 = stage.l2(out, x0, mask)
    lfg, lbg, lrgb = loss_fn.render_terms(fgs, rgbs, target_rgb, mask, opacity, alphas)
    if drop_im is None:
        drop_im = torch.ones(x0.shape[0], device=x0.device)
    total, logged = combine_losses(l2, lfg, lbg, lrgb, drop_im, as_tensors=True, **loss_kw)
    total.backward()
    optimizer.step()
    if not as_tensors:
        logged = {k: float(v) for k, v in logged.items()}
    return total.detach(), logged


class GraphedTrainStep:
    """train_step captured ONCE into a hipGraph and replayed: forward, loss, backward and the optimiser step of BASELINE config 4 are
    ~6400 kernel launches and ~16000 torch operator calls per step -- host work that takes longer than the kernels run;
    a replay costs one launch.  Conditions: fixed shapes (the batch is copied into static buffers), a MasterAdamW on its fused
    path (or built with capturable=True), the raymarchers on device_rng=True (the stratified jitter of patch x / y is then drawn by the device generator, which
    a graph advances on every replay; the reference draws those two on the CPU generator).  Under an initialised process group the
    gradient all-reduce is part of the graph (RCCL collectives capture; tools/probe/rccl_graph_probe.py).  The returned loss terms are 0-d device tensors that the next replay overwrites.
    Side effects of construction, all deliberate: (1) `warmup` REAL optimisation steps run on the construction batch before the capture
    (weights, moments and the device step counter advance by `warmup`; pass warmup_restore=True to snapshot and restore parameters,
    masters, moments and the step counter around them); (2) `device_rng = True` stays set on every raymarcher, so later eager steps draw
    their patch jitter from the device generator too; (3) unless the optimiser is LIVE (MasterAdamW(max_grad_norm= / ema_decay= / live=True)),
    lr and weight_decay are frozen into the graph at capture time -- an LR scheduler that edits `optimizer.param_groups` then has no effect
    on replays (re-capture to change them).  A live optimiser reads both from a device table that __call__ refreshes (sync_hyper, outside
    the graph) before every replay: schedules reach the replays.
    stage=NoiseStage(...): the captured step is train_step_latents -- `batch` then holds ITS keywords (x0, x_ref, context, y, pose,
    target_rgb, mask, opacity, drop_im, mask_ref: clean latents instead of noised ones) and the stage's launches are graph nodes, the sigma
    draw with advance on: replay k after the capture draws at step counter + k, with no host work, and stage.set_step / reseed /
    set_streams between replays reach the next one.  Every warm-up step is a real step and advances the stage's step counter by one (the
    capture itself only records: it draws nothing and advances nothing), so after construction the counter stands `warmup` higher than
    before; warmup_restore=True puts it back to its value from before the warm-up.  stage=None (the default) changes nothing:
    no buffer, no launch, no graph node."""

    def __init__(self, unet: torch.nn.Module, loss_fn, optimizer: "MasterAdamW", batch: dict, warmup: int = 3, warmup_restore: bool = False,
                 weight_prefetch: bool = False, stage: Optional["NoiseStage"] = None, **loss_kw):
        if not optimizer.capturable:
            raise ValueError("GraphedTrainStep: the torch fall-back of MasterAdamW must be built with capturable=True (the fused path is as it is)")
        self.unet, self.loss_fn, self.optimizer, self.loss_kw, self.stage = unet, loss_fn, optimizer, loss_kw, stage
        if stage is None:
            step_fn = train_step
        else:
            step_fn = lambda unet, loss_fn, optimizer, **kw: train_step_latents(unet, loss_fn, optimizer, stage, **kw)
        for m in unet.modules():
            if hasattr(m, "device_rng"):
                m.device_rng = True
        clone = lambda v: v.clone() if torch.is_tensor(v) else ({k: clone(x) for k, x in v.items()} if isinstance(v, dict) else v)
        self.static = {k: clone(v) for k, v in batch.items()}
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # allocator, library workspaces, weight packs, optimiser state: all settled before the capture
            saved = None
            if warmup_restore and optimizer.fused:
                saved = ([p.detach().clone() for p in optimizer.params], optimizer._master.clone(), optimizer.exp_avg.clone(),
                         optimizer.exp_avg_sq.clone(), optimizer.steps.clone(), None if optimizer._ema is None else optimizer._ema.clone())
            stage_step = stage.step.clone() if warmup_restore and stage is not None else None
            for _ in range(warmup):
                step_fn(unet, loss_fn, optimizer, as_tensors=True, **self.static, **loss_kw)
            if stage_step is not None:
                stage.step.copy_(stage_step)
            if saved is not None:
                with torch.no_grad():
                    for p, q in zip(optimizer.params, saved[0]):
                        p.copy_(q)
                    optimizer._master.copy_(saved[1]); optimizer.exp_avg.copy_(saved[2]); optimizer.exp_avg_sq.copy_(saved[3]); optimizer.steps.copy_(saved[4])
                    if saved[5] is not None:
                        optimizer._ema.copy_(saved[5])
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        from . import memo
        memo.new_epoch()  # nothing memoised before this point -- by the warm-up steps or by an earlier capture -- may feed this graph
        # with a process group the gradient all-reduce (one flat RCCL all-reduce, MasterAdamW.allreduce_grads) is captured with the step; the
        # group's watchdog thread polls events meanwhile, which only the thread-local capture mode tolerates.  Every rank captures the same
        # sequence and must replay in lock-step, as with any collective.
        mode = "thread_local" if dist.is_available() and dist.is_initialized() else "global"
        import contextlib
        pf = contextlib.nullcontext()
        if weight_prefetch:  # (cd360/prefetch.py; measured SLOWER here, 121.3 vs 117.9 ms: 3400 short launches leave the touches no room -- off)
            from .prefetch import WeightPrefetcher
            pf = WeightPrefetcher(next(unet.parameters()).device)
        with torch.cuda.graph(self.graph, capture_error_mode=mode):
            with pf:
                self.total, self.logged = step_fn(unet, loss_fn, optimizer, as_tensors=True, **self.static, **loss_kw)
        memo.new_epoch()

    @staticmethod
    def _load(dst, src):
        if torch.is_tensor(dst):
            dst.copy_(src)
        elif isinstance(dst, dict):
            for k in dst:
                GraphedTrainStep._load(dst[k], src[k])

    def __call__(self, **batch):
        """Copies `batch` (same keys and shapes as at construction; omitted keys keep their values) into the static buffers, replays."""
        for k, v in batch.items():
            self._load(self.static[k], v)
        if hasattr(self.optimizer, "sync_hyper"):
            self.optimizer.sync_hyper()  # a live optimiser: this step's lr / weight decay into the table the captured kernels read
        self.graph.replay()
        self.optimizer.bump_versions()  # the replay rewrote the parameters behind torch's back: invalidate every cache keyed on their version
        return self.total, self.logged
