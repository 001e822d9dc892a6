"""What tests/test_optim_cpu.py and tests/test_optim_gpu.py share (plain helper module, like edit_cases.py; no tests, no fixtures): the
names include/optim/cd360_optim.h adds (the library's entry in sampler_cases.LIBRARIES, where the header / table / library rule is
stated), the small ragged tensor set of the GPU tests and the torch restatement of the EMA update, one fp32 operation at a time."""
import os

import torch

import sampler_cases as SC

LIBRARY = 2  # in SC.LIBRARIES
NEW = SC.LIBRARIES[LIBRARY][3]
HEADER = os.path.join("optim", "cd360_optim.h")
KERNELS = ("grad_sumsq_kernel", "grad_clip_kernel", "adamw_live_kernel")
# the ragged set of test_fused_adamw_matches_torch_adamw_on_fp32_masters scaled down: tails of fewer than 8 values (1, 3 x 5 = 15, 77), a few
# thousand values so that several workgroups take part (20000 values = 2500 vectors: 10 blocks of the update, 2 of the sum of squares), and
# 70 one-vector tensors so that two chunks launch.  Index 5 becomes a 2-byte-aligned view (tensors()).
SHAPES = [(160, 125), (3,), (3, 5), (1,), (4, 24), (77,), (13, 40)] + [(1 + i % 8,) for i in range(70)]
UNALIGNED = 5


def tensors(seed, shapes=SHAPES, scale=0.1, device="cuda"):
    """bf16 tensors of `shapes`, index UNALIGNED a view that starts 2 bytes into its storage (the kernels' scalar path)."""
    g = torch.Generator(device=device).manual_seed(seed)
    out = [torch.randn(*s, generator=g, device=device).mul_(scale).to(torch.bfloat16) for s in shapes]
    if len(shapes) > UNALIGNED:
        n = out[UNALIGNED].numel()
        out[UNALIGNED] = torch.randn(n + 1, generator=g, device=device).mul_(scale).to(torch.bfloat16)[1:]
    return out


def parameters(base):
    """Fresh Parameters holding `base`'s values, each in its own storage, the misaligned one misaligned again."""
    ps = []
    for b in base:
        if b.storage_offset():
            ps.append(torch.nn.Parameter(torch.cat([b[:1], b])[1:]))
        else:
            ps.append(torch.nn.Parameter(b.clone()))
    return ps


def groups(ps):
    return [{"params": ps[:4], "lr": 1e-3, "weight_decay": 0.1}, {"params": ps[4:], "lr": 3e-4}]


def ema_update(ema, master, t, decay):
    """LitEma.forward with use_num_upates=True restated one fp32 operation at a time: ema, master fp32 tensors, t the step count after the
    tick (a python number), decay the cap.  -> the new ema.  The three scalar operations run on the CPU (IEEE fp32), the two per element
    on the tensors' device, each a torch operation of its own (nothing is fused)."""
    t = torch.tensor(float(t), dtype=torch.float32)
    warm = (1.0 + t) / (10.0 + t)
    d = torch.minimum(torch.tensor(decay, dtype=torch.float32), warm)
    omd = (1.0 - d).to(ema.device)
    return ema - omd * (ema - master)
