"""What the sampler test files share (plain helper module, like guarded.py, philox_ref.py and gemm_cases.py; no tests, no fixtures): the
device-tensor builders, ONE torch restatement of the CFG combine in the kernels' order, the header / signature-table / guarded-case checks,
the tiny job every GPU file samples (latent 32, 6 views, n_train 50, 4 steps, 3 poses, seed 360) and the walk through the un-captured
sampler classes.  A file keeps what is its own: the restatement of its solver's update, its tables, GUARDED list, bars and constants."""
import ctypes
import functools
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
BF = torch.bfloat16
LATENT, REFS, N_TRAIN, STEPS, POSES, SEED = 32, 6, 50, 4, 3, 360


# ------------------------------------------------------------------------------------------------ device tensors
def seed_t(seed):
    from cd360.sampler import seed_words
    return torch.tensor([seed_words(seed)], dtype=torch.int64, device=DEV)


def step_t(step):
    return torch.tensor([step], dtype=torch.int32, device=DEV)


def streams_t(ids):
    return None if ids is None else torch.tensor(ids, dtype=torch.int32, device=DEV)


def R(*shape, seed=0, dtype=torch.float32):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV).to(dtype)


def cl_to_nchw(e16, n, H, Wd):
    """Channels 0..3 of channels-last bf16 rows [n, H W, >= 4] as the NCHW fp32 tensor the flat kernels take."""
    return e16[..., :4].float().reshape(n, H, Wd, 4).permute(0, 3, 1, 2).contiguous()


def eps_forms(nb, bs, H, Wd, seed):
    """Two channels-last eps of the SAME values: ld = 4 (rows of their own) and ld = 8 (channels 0..3 of 8-wide rows); and their NCHW fp32."""
    e8 = R(nb * bs, H * Wd, 8, seed=seed, dtype=BF)
    e4 = e8[..., :4].contiguous()
    assert e4.stride(1) == 4 and e8[..., :4].stride(1) == 8
    return (e4, e8[..., :4]), cl_to_nchw(e8, nb * bs, H, Wd)


def guardfn(fn):
    """Mark a callable for guarded.run_twice: it takes the guard as its last argument."""
    fn.wants_guard = True
    return fn


# ------------------------------------------------------------------------------------------------ the CFG combine
def combine(x, e, s, scale, scale_im):
    """d0 of every tail in the kernels' order, one fp32 rounding per operation (torch's elementwise kernels do not contract): den_b = x - s
    e_b, then the guider's expression; scale_im=None is the two-branch form.  Independent of cd360.sampler.cfg_combine, which it checks."""
    if scale_im is None:
        e_u, e_c = e.chunk(2)
        du, dc = x - s * e_u, x - s * e_c
        return du + scale * (dc - du)
    e_u, e_i, e_c = e.chunk(3)
    du, dic, dc = x - s * e_u, x - s * e_i, x - s * e_c
    return du + scale * (dc - dic) + scale_im * (dic - du)


# ------------------------------------------------------------------------------------------------ headers, tables, guarded cases
def header_text(header):
    return open(os.path.join(ROOT, "include", header)).read()


def declared_functions(header):
    """The functions include/<header> declares: every `int cd360_...(` / `int64_t cd360_...(` outside comments."""
    src = re.sub(r"/\*.*?\*/", " ", header_text(header), flags=re.S)
    return set(re.findall(r"\b(?:int|int64_t)\s+(cd360_\w+)\s*\(", src))


def header_constant(header, name):
    m = re.search(r"#define\s+%s\s+(\d+)" % name, header_text(header))
    assert m, name
    return int(m.group(1))


def _header_table_library(header, table, new_names, older_tables, older_headers, lib):
    """The rule itself: -> (mismatch, in_older_tables, in_older_headers, mistyped, lib), the first four empty when it holds."""
    new = set(new_names)
    declared = set(re.findall(r"\b(cd360_[a-z0-9_]+)\s*\(", header_text(header)))
    mismatch = (declared ^ set(table)) | (declared ^ new)
    in_older_tables = {n for t in older_tables for n in t} & new
    in_older_headers = [h for h in older_headers if any(n in header_text(h) for n in new)]
    mistyped = [n for n in new_names if not (isinstance(getattr(lib, n), ctypes._CFuncPtr) and getattr(lib, n).restype is ctypes.c_int
                                             and list(getattr(lib, n).argtypes) == table[n][1])]
    return mismatch, in_older_tables, in_older_headers, mistyped, lib


def check_header_matches_table(header, table, new_names, older_headers):
    """include/<header> <=> its signature table, by the rule test_library_exports_every_declared_symbol holds cd360_hip.h to (every
    `cd360_...(` word, comments included).  -> (mismatch, in_older_tables, in_older_headers, mistyped, lib): the names on which header,
    table and `new_names` disagree; the new names an older header's table holds; the older headers that name one; the new names the loaded
    library does not export as typed; and the library itself (loaded with check_symbols=True).  The first four must be empty."""
    from cd360 import _lib
    assert _lib.ABI[header] is table and all(h in _lib.ABI for h in older_headers)
    return _header_table_library(header, table, new_names, [_lib.ABI[h] for h in older_headers], older_headers, _lib.load(check_symbols=True))


# every library in the order it was added: (header folder under include/, binding module of cd360, its table there, the names its header
# declares).  The first library's tables are cd360._lib.ABI, its headers include/*.h; a new library enters itself at the end.
LIBRARIES = [
    ("", "_lib", None, None),
    ("edit", "_edit", "EDIT_SIGNATURES", ["cd360_edit_noise_f32", "cd360_mask_blend_f32"]),
    ("optim", "_optim", "OPTIM_SIGNATURES", ["cd360_grad_sumsq_bf16", "cd360_grad_clip_f32", "cd360_adamw_live_bf16"]),
    ("text", "_text", "TEXT_SIGNATURES", ["cd360_text_embed_bf16", "cd360_text_causal_attn_bf16", "cd360_text_act_bf16", "cd360_text_eot_pool_bf16"]),
]


def check_library_matches_table(position):
    """LIBRARIES[position], a library beside the first: its header <=> its table <=> the loaded library, by the rule of
    check_header_matches_table, and every older library closed to it.  -> (mismatch, in_tables, in_headers, mistyped, lib): the names on
    which header, table and the entry's names disagree; the new names a table of cd360._lib.ABI or of an earlier entry holds; the headers
    in the folders of the earlier entries (listed from include/, bound or not) that name one; the new names the library does not export as
    typed; the library.  The first four must be empty."""
    import importlib
    from cd360 import _lib
    assert 0 < position < len(LIBRARIES)
    folder, module, attr, new_names = LIBRARIES[position]
    mod = importlib.import_module("cd360." + module)
    table = getattr(mod, attr)
    assert mod.HEADER == os.path.join(folder, os.path.basename(mod.HEADER))
    older_tables = list(_lib.ABI.values()) + [getattr(importlib.import_module("cd360." + m), a) for _, m, a, _ in LIBRARIES[1:position]]
    assert all(t is not table for t in older_tables)
    inc = os.path.join(ROOT, "include")
    older_headers = [os.path.join(d, f) for d, _, _, _ in LIBRARIES[:position] for f in os.listdir(os.path.join(inc, d)) if f.endswith(".h")]
    return _header_table_library(mod.HEADER, table, new_names, older_tables, older_headers, mod.load())


def check_guarded_cover(header, table, guarded_cases):
    """Every function include/<header> declares is typed in `table` and in some guarded case's `declares` (a case = (id, declares, ...)).
    -> (untyped, unknown, uncovered): names header and table disagree on; declared by a case but not by the header; launching entry points
    without a guarded case.  All three must be empty."""
    names = declared_functions(header)
    assert names, header
    declared = {e for c in guarded_cases for e in c[1]}
    return names ^ set(table), declared - names, names - declared


# ------------------------------------------------------------------------------------------------ the tiny job
@functools.lru_cache(maxsize=1)
def net():
    import bench
    return bench.build_model(LATENT, REFS, N_TRAIN, DEV)


def job(p, nb=3):
    """Target pose p in one replay: nb camera batches, ctx / y = [uc | (uc) | c], start latent."""
    from cd360 import synth
    cam = synth.pose_batch(1, REFS, seed=100 + p, n_train=N_TRAIN)[0]
    g = torch.Generator(device=DEV).manual_seed(7 + p)
    ctx = torch.randn(2, 77, 2048, generator=g, device=DEV).to(BF)
    y = torch.randn(2, 2816, generator=g, device=DEV).to(BF)
    x = torch.randn(1, 4, LATENT, LATENT, generator=g, device=DEV)
    return [cam] * nb, torch.cat([ctx[0:1]] * (nb - 1) + [ctx[1:2]]), torch.cat([y[0:1]] * (nb - 1) + [y[1:2]]), x


def sampler(pose, ctx, y, n_steps=STEPS, **kw):
    """job.Sampler on the shared net; graph mode and seed 360 unless `kw` says otherwise."""
    from cd360 import job as J
    return J.Sampler(net(), pose, ctx, y, n_steps, **dict(dict(use_graph=True, seed=SEED), **kw))


_WALKS = {}


def walk(**kw):
    """3 poses x all 4 steps of a 4-step schedule through ONE graph-mode sampler(**kw) (job.sample_poses) -> (latents, the sampler); built
    once per `kw` and kept until release()."""
    from cd360 import job as J
    key = tuple(sorted(kw.items()))
    if key not in _WALKS:
        held = {}

        def make_sampler(pose, ctx, y):
            held["smp"] = sampler(pose, ctx, y, **kw)
            return held["smp"]

        with torch.no_grad():
            latents, mine = J.sample_poses(make_sampler, job, POSES, STEPS, world=1, rank=0)
        assert mine == list(range(POSES))
        _WALKS[key] = latents, held["smp"]
    return _WALKS[key]


def release():
    """Let go of the UNet and the captured samplers a file built through net() / walk()."""
    _WALKS.clear()
    net.cache_clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ the un-captured classes
def guider_config(nb):
    """The YAML guider of `nb` branches at the scales the job's defaults hold."""
    if nb == 2:
        return {"target": "sgm.modules.diffusionmodules.guiders.VanillaCFGImgRef", "params": {"scale": 7.5}}
    return {"target": "sgm.modules.diffusionmodules.guiders.ScheduledCFGImgTextRef", "params": {"scale": 7.5, "scale_im": 3.5}}


def module_route(net, mod, solver, nb, pose, ctx, y, x0, steps, order=None):
    """The un-captured module route: `mod`, an instance of cd360.sampler's class for `solver`, + its guider + DiscreteDenoiser around the
    same UNet, eager, over the first `steps` steps of mod.num_steps, each class by its own sampler_step convention.  -> the latent."""
    from cd360 import sampler as S
    from cd360 import sampling
    den = S.DiscreteDenoiser().to(DEV)
    sampling.set_cfg_branches(net, nb)
    sampling.clear_rendered_feat(net)
    c, uc = {"crossattn": ctx[nb - 1:], "vector": y[nb - 1:]}, {"crossattn": ctx[:1], "vector": y[:1]}
    network = lambda x_in, t, cond: (net(x_in, timesteps=t, context=cond["crossattn"], y=cond["vector"], pose=pose)[0], None, None, None)  # noqa: E731
    denoiser = lambda inp, s, cond: den(network, inp, s, cond)  # noqa: E731
    sig = mod.discretization(mod.num_steps, device=DEV)
    table = S.lms_coefficients(sig, order) if solver == "lms" else None
    x, old, ds = x0.clone(), None, []
    for i in range(steps):
        s, sn = sig[i].reshape(1), sig[i + 1].reshape(1)
        if solver in ("euler", "heun"):
            x, _ = mod.sampler_step(s, sn, denoiser, x, c, uc, mod.gamma_of(sig[i], mod.num_steps))
        elif solver == "dpmpp2m":
            x, old = mod.sampler_step(old, None if i == 0 else sig[i - 1].reshape(1), s, sn, denoiser, x, c, uc)
        elif solver == "lms":
            x = mod.sampler_step(ds, [float(table[i, j]) for j in range(min(i + 1, mod.order))], s, denoiser, x, c, uc)
        else:  # "euler_a", "dpmpp2s_a"
            x = mod.sampler_step(s, sn, denoiser, x, c, uc)
    sampling.clear_rendered_feat(net)
    return x
