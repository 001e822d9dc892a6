"""The two ends of a training step, without a GPU: the sixth library's header <=> table <=> exports, its host-side refusals and its
resource record; the numpy restatement of tests/train_cases.py against the reference's own arithmetic (tests/golden/train_stage.npz,
tests/golden/make_train_stage_golden.py); what makes exact index comparison safe; NoiseStage's refusals; render_terms against get_loss."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import sampler_cases as SC
import textgrad_cases as TG
import train_cases as TR
from make_golden_params import LOSS_CFG, loss_inputs
from sgm.util import instantiate_from_config

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TARGET = "sgm.modules.diffusionmodules.loss.StandardDiffusionLossImgRef"


# ================================================================================================ 1: header, table, library
def test_train_header_matches_its_table_and_the_older_libraries_are_closed():
    """include/train/cd360_train.h <=> cd360._train.TRAIN_SIGNATURES <=> libcd360_train.so by the rule of
    sampler_cases._header_table_library, with all five older libraries closed to the new names.  The binding and the source read no
    environment, the source never synchronises and accumulates nowhere across workgroups; __graft_entry__.LIBRARIES keeps its five rows and
    the new row is the second table's."""
    from cd360 import _textgrad, _train, ops
    tables, headers, libs = TG.older_libraries()
    tables, libs = tables + [_textgrad.TEXTGRAD_SIGNATURES], libs + [_textgrad.load()]
    headers = headers + [TG.HEADER]
    mismatch, in_tables, in_headers, mistyped, lib = SC._header_table_library(_train.HEADER, _train.TRAIN_SIGNATURES, TR.NEW, tables, headers, _train.load())
    assert not mismatch, mismatch
    assert not in_tables, in_tables
    assert not in_headers, in_headers
    assert not mistyped, mistyped
    assert _train.HEADER == TR.HEADER and all(n.startswith("cd360_train_") for n in TR.NEW) and len(libs) == 5
    for older in libs:
        for name in TR.NEW:
            assert not hasattr(older, name), name
    src = open(_train.__file__).read()
    assert "os.environ" not in src and "getenv" not in src
    hip = open(os.path.join(SC.ROOT, "custom-diffusion360_amd", "csrc_train", "train_stage.hip")).read()
    assert "getenv" not in hip and "Synchronize" not in hip and "atomic" not in hip
    for name, py in (("CD360_TRAIN_ROW", (ops.TRAIN_ROW, _train.ROW, TR.ROW)), ("CD360_TRAIN_CUBIC", (ops.TRAIN_CUBIC, _train.CUBIC, TR.CUBIC)),
                     ("CD360_TRAIN_DISCRETE", (ops.TRAIN_DISCRETE, _train.DISCRETE, TR.DISCRETE))):
        value = SC.header_constant(TR.HEADER, name)
        assert all(v == value for v in py), name
        assert f"#define {name} {value}\n" in hip, name
    philox = open(os.path.join(SC.ROOT, "custom-diffusion360_amd", "csrc", "cd360_philox.h")).read()
    for name, value in (("SIGMA", 4), ("TARGET", 5), ("REF_A", 6), ("REF_B", 7)):
        assert f"CD360_NOISE_TRAIN_{name} = {value}u;" in philox, name
    assert (_train.DOMAIN_SIGMA, _train.DOMAIN_TARGET, _train.DOMAIN_REF_A, _train.DOMAIN_REF_B) == (4, 5, 6, 7)
    spec = importlib.util.spec_from_file_location("_graft_entry_for_train", os.path.join(SC.ROOT, "__graft_entry__.py"))
    entry = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(entry)
    assert tuple(entry.LIBRARIES[-1]) == TG.BUILD_ROW and len(entry.LIBRARIES) == len(SC.LIBRARIES) + 1
    assert [tuple(r) for r in entry.LATER_LIBRARIES] == [TR.BUILD_ROW]


def test_every_train_entry_point_has_a_guarded_case():
    from cd360 import _train
    untyped, unknown, uncovered = SC.check_guarded_cover(TR.HEADER, _train.TRAIN_SIGNATURES, TR.GUARDED)
    assert not untyped, untyped
    assert not unknown, unknown
    assert not uncovered, f"launching entry points without a guarded case: {sorted(uncovered)}"


def test_train_kernels_are_recorded_without_scratch():
    """The record of train_stage.o: every kernel is there, with zero scratch and no vector-register spill."""
    rec = json.load(open(os.path.join(SC.ROOT, "custom-diffusion360_amd", "lib", "obj", "train_stage.o.resources.json")))
    assert all(any(k in name for name in rec) for k in TR.KERNELS), sorted(rec)
    for name, r in rec.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)


# ================================================================================================ 2: refusals on the host
def test_train_entry_points_refuse_bad_arguments_on_the_host():
    """Fabricated non-null pointers: every call below returns CD360_ERR_ARG (-1) or CD360_ERR_SHAPE (-2) before anything launches."""
    from cd360 import _train
    lib = _train.load()
    nul, P = ctypes.c_void_p(None), ctypes.c_void_p
    p = [P(0x1000000 * i) for i in range(1, 16)]
    odd = lambda q, by: P(q.value + by)
    # ---- cd360_train_sigmas_f32
    names = ("table", "tgt", "ref", "seed", "streams", "step", "rows", "timesteps", "ref_idx", "step_used")

    def sig(n_table=1000, n_tgt=1000, tgt_kind=0, tgt_start=0, n_ref=50, ref_kind=1, ref_start=0, advance=1, B=3, **kw):
        a = dict(zip(names, p))
        a.update(kw)
        return lib.cd360_train_sigmas_f32(a["table"], n_table, a["tgt"], n_tgt, tgt_kind, tgt_start, a["ref"], n_ref, ref_kind, ref_start, a["seed"],
                                          a["streams"], a["step"], advance, a["rows"], a["timesteps"], a["ref_idx"], a["step_used"], B, nul)

    for name in names:
        if name != "streams":
            assert sig(**{name: nul}) == -1, name
        assert sig(**{name: odd(dict(zip(names, p))[name], 2)}) == -1, name
    assert sig(seed=odd(p[3], 4)) == -1 and sig(timesteps=odd(p[7], 4)) == -1 and sig(ref_idx=odd(p[8], 4)) == -1  # 8-byte words
    assert sig(B=0) == -1 and sig(B=-1) == -1 and sig(n_table=0) == -1 and sig(n_tgt=0) == -1 and sig(n_ref=-3) == -1
    assert sig(tgt_kind=2) == -1 and sig(ref_kind=-1) == -1
    for name in ("step_used", "rows", "timesteps", "ref_idx", "seed", "streams"):  # the counter is rewritten: it may alias nothing else
        assert sig(step=dict(zip(names, p))[name]) == -1, name
    assert sig(ref_start=50) == -2 and sig(ref_start=-1) == -2 and sig(ref_start=77) == -2
    assert sig(tgt_kind=1, tgt_start=1000) == -2 and sig(ref_kind=0, n_ref=(1 << 24) + 1) == -2
    # ---- cd360_train_noise_f32
    names = ("x0", "xr", "drop", "rows", "seed", "streams", "step_used", "x_t", "x_in", "xr_in")

    def noise(level=0.1, dtype=1, B=3, n=2, HW=64, **kw):
        a = dict(zip(names, p))
        a.update(kw)
        return lib.cd360_train_noise_f32(a["x0"], a["xr"], a["drop"], a["rows"], a["seed"], a["streams"], a["step_used"], level, a["x_t"], a["x_in"],
                                         a["xr_in"], dtype, B, n, HW, nul)

    for name in names:
        if name not in ("xr", "drop", "streams"):
            assert noise(**{name: nul}) == -1, name
        assert noise(**{name: odd(dict(zip(names, p))[name], 1)}) == -1, name
    assert noise(seed=odd(p[4], 4)) == -1 and noise(x_in=odd(p[8], 2), dtype=0) == -1
    assert noise(B=0) == -1 and noise(HW=0) == -1 and noise(n=0) == -1 and noise(dtype=2) == -1 and noise(dtype=-1) == -1
    assert noise(level=-0.1) == -1 and noise(level=float("nan")) == -1 and noise(level=float("inf")) == -1
    assert noise(HW=(1 << 32) + 4, B=1, n=1) == -2 and noise(HW=1 << 31, n=3, B=1) == -2 and noise(HW=1 << 20, n=4097, B=1) == -2
    assert noise(x_t=p[0]) == -1 and noise(x_in=P(p[0].value + 64)) == -1 and noise(xr_in=p[1]) == -1  # an output over an input
    # ---- cd360_train_l2_f32 / cd360_train_l2_bwd_f32
    S = lambda *v: (ctypes.c_int64 * 4)(*v)
    cl, planes = S(256, 1, 32, 4), S(256, 64, 8, 1)
    names = ("eps", "x_t", "x0", "rows", "mask", "loss", "den")

    def l2(dtype=1, st=cl, B=3, H=8, W=8, **kw):
        a = dict(zip(names, p))
        a.update(kw)
        return lib.cd360_train_l2_f32(a["eps"], dtype, st, a["x_t"], a["x0"], a["rows"], a["mask"], a["loss"], a["den"], B, H, W, nul)

    for name in names:
        if name != "mask":
            assert l2(**{name: nul}) == -1, name
        assert l2(**{name: odd(dict(zip(names, p))[name], 1)}) == -1, name
    assert l2(st=None) == -1 and l2(dtype=2) == -1 and l2(B=0) == -1 and l2(H=0) == -1 and l2(W=-1) == -1 and l2(eps=odd(p[0], 2), dtype=0) == -1
    assert l2(st=S(256, 1, -32, 4)) == -2 and l2(st=S(-1, 64, 8, 1)) == -2 and l2(H=1 << 15, W=1 << 14) == -2
    names = ("eps", "x_t", "x0", "rows", "mask", "den", "g", "d_eps")

    def bwd(dtype=1, st=cl, ds=cl, B=3, H=8, W=8, **kw):
        a = dict(zip(names, p))
        a.update(kw)
        return lib.cd360_train_l2_bwd_f32(a["eps"], dtype, st, a["x_t"], a["x0"], a["rows"], a["mask"], a["den"], a["g"], a["d_eps"], ds, B, H, W, nul)

    for name in names:
        if name != "mask":
            assert bwd(**{name: nul}) == -1, name
        assert bwd(**{name: odd(dict(zip(names, p))[name], 1)}) == -1, name
    assert bwd(st=None) == -1 and bwd(ds=None) == -1 and bwd(dtype=3) == -1 and bwd(B=0) == -1 and bwd(H=0) == -1 and bwd(W=0) == -1
    assert bwd(st=S(256, 64, 8, -1)) == -2 and bwd(ds=S(256, -64, 8, 1), st=planes) == -2 and bwd(H=1 << 15, W=1 << 14) == -2


# ================================================================================================ 3: the restatement is the reference's arithmetic
@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLD, "train_stage.npz")))


@pytest.mark.parametrize("tag,level", [("l0", 0.0), ("l1", 0.1)])
def test_restatement_reproduces_the_reference(gold, tag, level):
    """tests/golden/train_stage.npz holds what the reference's loss and denoiser hand their network, w and loss_l2, on the documented draws.
    The fp32 restatement: both index vectors exactly; every float -- x_in, input_ref and w per element, and loss_l2, with and without the
    mask -- within 2 ulp of the recorded fp32 value."""
    g = gold
    kw = dict(seed=int(g["seed"]), streams=[int(s) for s in g["streams"]], step=int(g["step"]), x0=g["x0"], xr=g["xr"], drop=g["drop_im"],
              eps=g["eps"], **TR.shipped(level))
    assert g["x0"].shape == (3, 4, 8, 8) and g["xr"].shape == (3, 2, 4, 8, 8) and g["drop_im"].tolist() == [1.0, 0.0, 1.0]
    r = TR.restate(np.float32, mask=g["mask"], **kw)
    assert np.array_equal(r["timesteps"], g[f"{tag}.timesteps"]) and np.array_equal(r["sigmas_ref_idx"], g[f"{tag}.sigmas_ref"])
    assert np.array_equal(r["timesteps"], r["tgt_idx"])  # the target sampler's table IS the denoiser's
    figures = {k: TR.ulps(r[mine], g[f"{tag}.{k}"]) for k, mine in (("x_in", "x_in"), ("input_ref", "xr_in"))}
    figures["w"] = TR.ulps(r["rows"][:, TR.W], g[f"{tag}.w"].reshape(-1))
    figures["loss_l2.m"] = TR.ulps(r["loss"], g[f"{tag}.loss_l2.m"])
    figures["loss_l2.n"] = TR.ulps(TR.restate(np.float32, mask=None, **kw)["loss"], g[f"{tag}.loss_l2.n"])
    print(f"{tag}: fp32 restatement against the reference, ulp: {figures}")
    assert figures["x_in"] <= 2 and figures["input_ref"] <= 2 and figures["w"] <= 2
    assert figures["loss_l2.m"] <= 2 and figures["loss_l2.n"] <= 2
    if level > 0:
        assert not np.array_equal(g["l0.x_in"], g["l1.x_in"]) and np.array_equal(g["l0.timesteps"], g["l1.timesteps"])
    r64 = TR.restate(np.float64, mask=g["mask"], **kw)
    assert np.array_equal(r64["timesteps"], r["timesteps"]) and np.abs(r64["x_in"] - r["x_in"]).max() < 1e-5


def test_exact_index_comparison_is_safe():
    """What lets the tests of cd360._train's library compare indices exactly, in the binding's own constants (its sampler kinds and its
    counter domain of the per-sample draw).  Over all 2^24 values u = k 2^-24 that the draw can take: torch's u ** 3 is u * u * u bit for bit, and the reference's cubic index
    ((1 - u ** 3) * 999).long() is the restatement's.  On the tables: sigma ** -2.0 is 1 / (s * s) bit for bit, 1 / (sigma ** 2 + 1) ** 0.5
    is 1 / sqrt(s * s + 1) to 2 ulp (this is a float, not an index), and every entry of the 50-entry table has ONE nearest entry of the 1000-entry one (no tie; the two
    nearest differ in distance by more than 1e-3), itself where the two tables meet."""
    from cd360 import _train
    assert (_train.CUBIC, _train.DISCRETE, _train.DOMAIN_SIGMA, _train.ROW) == (TR.CUBIC, TR.DISCRETE, TR.DOMAIN_SIGMA, TR.ROW)
    k = np.arange(1 << 24, dtype=np.uint32)
    u = (k.astype(np.float64) * 2.0 ** -24).astype(np.float32)
    assert np.array_equal(TR.uniform24(k << np.uint32(8)), u)
    tu = torch.from_numpy(u)
    assert torch.equal(tu ** 3, tu * tu * tu) and np.array_equal((tu ** 3).numpy(), u * u * u)
    assert np.array_equal(((1 - tu ** 3) * 999).long().numpy(), TR.sample_index(_train.CUBIC, k << np.uint32(8), 1000, 0))
    t1000, t50 = TR.legacy_table(1000), TR.legacy_table(50)
    for tab in (t1000, t50):
        s = torch.from_numpy(tab)
        one = np.float32(1.0)
        assert np.array_equal((s ** -2.0).numpy(), one / (tab * tab))
        c_in = TR.ulps((1 / (s ** 2 + 1.0) ** 0.5).numpy(), one / np.sqrt(tab * tab + one))
        print(f"{len(tab)} entries: torch's 1 / (s ** 2 + 1) ** 0.5 against the correctly rounded 1 / sqrt(s * s + 1): {c_in} ulp")
        assert c_in <= 2  # torch's vectorised pow is not correctly rounded everywhere; the kernels' sqrtf and division are
    d = np.sort(np.abs(t50[None, :] - t1000[:, None]), axis=0)
    gap = float((d[1] - d[0]).min())
    print(f"50 -> 1000 entries: the smallest lead of the nearest entry over the second nearest is {gap:.3e}")
    assert gap > 1e-3 and float(d[0].max()) == 0.0
    from cd360 import sampler as S
    den = S.DiscreteDenoiser()
    assert np.array_equal(den.sigma_to_idx(torch.from_numpy(t50)).numpy(), TR.sigma_to_idx(t50, t1000))


# ================================================================================================ 4: the Python layer
def _loss_fn(**kw):
    return instantiate_from_config({"target": TARGET, "params": dict(LOSS_CFG, **kw)})


def test_noise_stage_refuses_what_it_does_not_serve():
    from cd360 import finetune, ops, sampler as S
    den = S.DiscreteDenoiser()
    edm = {"target": "sgm.modules.diffusionmodules.sigma_sampling.EDMSampling"}
    with pytest.raises(ValueError, match="EDMSampling"):
        finetune.NoiseStage(den, _loss_fn(sigma_sampler_config=edm), 1)
    with pytest.raises(ValueError, match="EDMSampling"):
        finetune.NoiseStage(den, _loss_fn(sigma_sampler_config_ref=edm), 1)
    with pytest.raises(ValueError, match="reference"):
        finetune.NoiseStage(den, _loss_fn(sigma_sampler_config_ref=None), 1)

    class VScaling:
        pass

    class EDMWeighting:
        pass

    other = S.DiscreteDenoiser()
    other.scaling = VScaling()
    with pytest.raises(ValueError, match="VScaling"):
        finetune.NoiseStage(other, _loss_fn(), 1)
    other = S.DiscreteDenoiser()
    other.weighting = EDMWeighting()
    with pytest.raises(ValueError, match="EDMWeighting"):
        finetune.NoiseStage(other, _loss_fn(), 1)
    off_grid = _loss_fn(sigma_sampler_config=dict(LOSS_CFG["sigma_sampler_config"], params=dict(LOSS_CFG["sigma_sampler_config"]["params"], num_idx=1000)))
    off_grid.sigma_sampler.sigmas = off_grid.sigma_sampler.sigmas * 1.01
    with pytest.raises(ValueError, match="denoiser's table"):
        finetune.NoiseStage(den, off_grid, 1)
    with pytest.raises(ValueError, match="l1"):
        finetune.NoiseStage(den, _loss_fn(type="l1"), 1)
    with pytest.raises(ValueError, match="dtype"):
        finetune.NoiseStage(den, _loss_fn(), 1, dtype=torch.float16)
    with pytest.raises(ops.Cd360Error, match="GPU"):  # a denoiser on the CPU: no fallback
        finetune.NoiseStage(den, _loss_fn(), 1)
    # the operators under it: CPU tensors that pass every shape check
    t = torch.from_numpy(TR.legacy_table(1000))
    seed, step = torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ops.Cd360Error, match="GPU"):
        ops.train_sigmas(t, t, 0, 0, t[:50].contiguous(), 1, 0, seed, None, step, 3)
    rows, x0 = torch.zeros(3, ops.TRAIN_ROW), torch.zeros(3, 4, 8, 8)
    with pytest.raises(ops.Cd360Error, match="GPU"):
        ops.train_noise(x0, None, None, rows, seed, None, step, 0.0)
    with pytest.raises(ops.Cd360Error, match="GPU"):
        ops.train_l2(x0.bfloat16(), x0, x0, rows, None)
    with pytest.raises(ValueError, match="start"):
        ops.train_sigmas(t, t, 0, 0, t[:50].contiguous(), 1, 50, seed, None, step, 3)
    with pytest.raises(ValueError, match="2\\^32"):
        ops.train_noise(torch.zeros(1, 4, 8, 8), torch.zeros(1, 1, 4, 8, 8).expand(1, 1 << 27, 4, 8, 8), None, torch.zeros(1, ops.TRAIN_ROW), seed, None, step, 0.0)


def test_render_terms_are_get_loss_without_the_l2_term():
    """get_loss = (l2,) + render_terms, bit for bit, on the inputs of tests/golden/loss.npz, whose fg / bg / rgb terms they reproduce; and
    the l2 term the stage computes -- the restatement of cd360_train_l2_f32 -- is get_loss's on D = eps c_out + x_t c_skip."""
    g = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLD, "loss.npz")).items()}
    d = loss_inputs()
    loss_fn = _loss_fn()
    fgs, als, rgbs = [d["fg0"], d["fg1"]], [d["alphas0"], d["alphas1"]], [d["rgb0"], d["rgb1"]]
    w = torch.tensor([0.5, 2.0, 1.0]).view(-1, 1, 1, 1)
    mo = d["x0"] * 0.9
    whole = loss_fn.get_loss(mo, fgs, rgbs, d["x0"], d["x_rgb"], w, d["mask"], None, d["opacity"], als)
    part = loss_fn.render_terms(fgs, rgbs, d["x_rgb"], d["mask"], d["opacity"], als)
    assert len(whole) == 4 and len(part) == 3 and all(torch.equal(a, b) for a, b in zip(whole[1:], part))
    for got, key in zip(part, ("lfg", "lbg", "lrgb")):
        assert torch.allclose(got, g[key], rtol=1e-5, atol=1e-7), key
    assert loss_fn.render_terms([], [], d["x_rgb"], None, d["opacity"], []) == ([], [], [])
    # the l2 term
    gs = dict(np.load(os.path.join(GOLD, "train_stage.npz")))
    for mask in (gs["mask"], None):
        r = TR.restate(np.float32, seed=9, streams=None, step=2, x0=gs["x0"], eps=gs["eps"], mask=mask, **TR.shipped(0.1))
        rows = torch.from_numpy(r["rows"])
        D = torch.from_numpy(gs["eps"]) * rows[:, TR.C_OUT].view(-1, 1, 1, 1) + torch.from_numpy(r["x_t"]) * rows[:, TR.C_SKIP].view(-1, 1, 1, 1)
        l2 = loss_fn.get_loss(D, [], [], torch.from_numpy(gs["x0"]), None, rows[:, TR.W].view(-1, 1, 1, 1), None if mask is None else torch.from_numpy(mask),
                              None, None, [])[0]
        u = TR.ulps(r["loss"], l2.numpy())
        print(f"l2 term, {'masked' if mask is not None else 'mean'}: restatement against get_loss, {u} ulp")
        assert u <= 2


def test_encode_batch_is_the_two_encode_calls_of_shared_step():
    """finetune.encode_batch on a first stage that records its calls: the targets, then the views flattened "(b n)", both at draw = step and
    in disjoint noise streams derived from the samples' ids; the views come back as [b, n, ...] in the order they went in; without views there is one call."""
    from cd360 import finetune

    class Recording:
        def __init__(self):
            self.calls = []

        def encode(self, x, seed, draw, streams=None):
            self.calls.append((tuple(x.shape), seed, draw, list(streams)))
            return x[:, :1, ::8, ::8].repeat(1, 4, 1, 1) + 100.0 * len(self.calls)

    fs = Recording()
    x = torch.arange(2 * 3 * 16 * 16, dtype=torch.float32).reshape(2, 3, 16, 16)
    xr = torch.arange(2 * 3 * 3 * 16 * 16, dtype=torch.float32).reshape(2, 3, 3, 16, 16)
    x0, z = finetune.encode_batch(fs, x, xr, seed=5, step=9)
    assert fs.calls == [((2, 3, 16, 16), 5, 9, [0, 4]), ((6, 3, 16, 16), 5, 9, [1, 2, 3, 5, 6, 7])]
    assert x0.shape == (2, 4, 2, 2) and z.shape == (2, 3, 4, 2, 2)
    assert torch.equal(z[1, 2], xr[1, 2, :1, ::8, ::8].repeat(4, 1, 1) + 200.0) and torch.equal(x0[1], x[1, :1, ::8, ::8].repeat(4, 1, 1) + 100.0)
    x0b, none = finetune.encode_batch(fs, x, None, seed=5, step=10)
    assert none is None and len(fs.calls) == 3 and fs.calls[2][2:] == (10, [0, 1])
    # the samples' own ids: what rank 1 of two draws for samples 2 and 3 is what one process draws for them
    fs2 = Recording()
    finetune.encode_batch(fs2, x, xr, seed=5, step=9, streams=[2, 3])
    whole = Recording()
    finetune.encode_batch(whole, torch.cat([x, x]), torch.cat([xr, xr]), seed=5, step=9, streams=[0, 1, 2, 3])
    assert fs2.calls[0][3] == whole.calls[0][3][2:] == [8, 12] and fs2.calls[1][3] == whole.calls[1][3][6:] == [9, 10, 11, 13, 14, 15]
    with pytest.raises(ValueError):
        finetune.encode_batch(fs2, x, xr, seed=5, step=9, streams=[1])
