"""What tests/test_optim_cpu.py and tests/test_optim_gpu.py share (plain helper module, like edit_cases.py; no tests, no fixtures): the
names include/optim/cd360_optim.h adds, the header / table / library rule of edit_cases.check_header_matches_table restated for the THIRD
library, a recorder for libcd360_optim.so under tests/guarded.py, the small ragged tensor set of the GPU tests and the torch restatement of
the EMA update, one fp32 operation at a time."""
import contextlib
import ctypes
import os
import re

import torch

import sampler_cases as SC

NEW = ["cd360_grad_sumsq_bf16", "cd360_grad_clip_f32", "cd360_adamw_live_bf16"]
HEADER = os.path.join("optim", "cd360_optim.h")
KERNELS = ("grad_sumsq_kernel", "grad_clip_kernel", "adamw_live_kernel")
# the ragged set of test_fused_adamw_matches_torch_adamw_on_fp32_masters scaled down: tails of fewer than 8 values (1, 3 x 5 = 15, 77), a few
# thousand values so that several workgroups take part (20000 values = 2500 vectors: 10 blocks of the update, 2 of the sum of squares), and
# 70 one-vector tensors so that two chunks launch.  Index 5 becomes a 2-byte-aligned view (tensors()).
SHAPES = [(160, 125), (3,), (3, 5), (1,), (4, 24), (77,), (13, 40)] + [(1 + i % 8,) for i in range(70)]
UNALIGNED = 5


def check_header_matches_table():
    """include/optim/cd360_optim.h <=> cd360._optim.OPTIM_SIGNATURES <=> the loaded libcd360_optim.so, by the rule of
    sampler_cases.check_header_matches_table (every `cd360_...(` word of the header, comments included).  -> (mismatch, in_tables,
    in_headers, mistyped, lib): the names on which header, table and NEW disagree; the new names a table of cd360._lib.ABI or
    EDIT_SIGNATURES holds; the headers of the first two libraries that name one; the new names the library does not export as typed; the
    library.  The first four must be empty."""
    from cd360 import _edit, _lib, _optim
    table = _optim.OPTIM_SIGNATURES
    assert all(t is not table for t in _lib.ABI.values()) and _edit.EDIT_SIGNATURES is not table
    new = set(NEW)
    declared = set(re.findall(r"\b(cd360_[a-z0-9_]+)\s*\(", SC.header_text(HEADER)))
    mismatch = (declared ^ set(table)) | (declared ^ new)
    in_tables = ({n for t in _lib.ABI.values() for n in t} | set(_edit.EDIT_SIGNATURES)) & new
    inc = os.path.join(SC.ROOT, "include")
    older = [f for f in os.listdir(inc) if f.endswith(".h")] + [os.path.join("edit", f) for f in os.listdir(os.path.join(inc, "edit")) if f.endswith(".h")]
    in_headers = [h for h in older if any(n in SC.header_text(h) for n in new)]
    lib = _optim.load()
    mistyped = [n for n in NEW if not (isinstance(getattr(lib, n), ctypes._CFuncPtr) and getattr(lib, n).restype is ctypes.c_int
                                       and list(getattr(lib, n).argtypes) == table[n][1])]
    return mismatch, in_tables, in_headers, mistyped, lib


def header_constant(name):
    m = re.search(r"#define\s+%s\s+(\d+)" % name, SC.header_text(HEADER))
    assert m, name
    return int(m.group(1))


@contextlib.contextmanager
def recorded(guard):
    """Inside tests/guarded.py's context: record the entry points of libcd360_optim.so as well (guarded() records cd360._lib.load()'s
    library; cd360.ops reaches the third library through cd360._optim.load()), into the same list P4 reads."""
    import guarded as G
    from cd360 import _optim
    rec = G.Recorder(_optim.load())
    saved = _optim.load
    _optim.load = lambda: rec
    try:
        yield rec
    finally:
        _optim.load = saved
        guard.lib.called.extend(rec.called)


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
