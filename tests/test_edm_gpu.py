"""The EDM family on the captured HIP step: the churn kernel against the device noise and its float64 restatement (tests/philox_ref.py), the
predictor / corrector tails bit for bit against a torch restatement, their memory safety, the GPU trajectories against the reference's
goldens, and the sampling job with solver="heun" and with s_churn > 0.  Needs an MI355X."""
import functools

import numpy as np
import pytest
import torch

import guarded as G
import philox_ref as P
import sampler_cases as SC
from sampler_cases import BF, DEV, LATENT, POSES, SEED, STEPS, R, seed_t, step_t, streams_t

NEW = ["cd360_edm_churn_f32", "cd360_cfg_edm_predict_cl", "cd360_cfg_edm_predict_f32", "cd360_cfg_edm_correct_cl", "cd360_cfg_edm_correct_f32"]
BIG_SEED = 2 ** 63 + 12345
ALL = dict(s_churn=40.0, s_noise=1.003)  # every row churned, clamped to sqrt 2 - 1: row 0's sigma_hat lies above the grid
CW = dict(s_churn=40.0, s_tmin=0.05, s_tmax=10.0, s_noise=1.0)  # the golden's windowed setting: row 0 un-churned
C1 = dict(s_churn=1.0, s_noise=1.003)  # the golden's un-clamped setting

# test 13's yardstick: the SAME comparison (captured job sampler against the un-captured module route, n_steps = 4, all 4 steps, latent 32 /
# 6 views, bs = 1) under plain EULER on the parent commit, measured with tools/solver_report.py --solver euler --repo <parent checkout> on
# the box and in the session of this change, per branch count: three branches 5.488e-2 of the latent's maximum, two branches 6.147e-2.
PARENT_EULER_JOB_VS_MODULE_REL = {3: 0.05488, 2: 0.06147}
BAR_FACTOR = {"euler": 2, "heun": 4}  # churned Euler: the margin the ancestral test grants a larger step; Heun: two evaluations per step


@functools.lru_cache(maxsize=None)
def _tables(tag):
    """A 4-step schedule's own tables on the device: (edm_tab, corr_tab, churn_tab)."""
    from cd360 import sampler as S
    return tuple(t.to(DEV) for t in S.edm_tables(S.LegacyDDPMDiscretization()(4), S.DiscreteDenoiser(), **{"all": ALL, "cw": CW}[tag]))


# ================================================================================================ 6: the churn kernel
@pytest.mark.gpu
@pytest.mark.parametrize("bs,H,Wd", [(1, 5, 7), (2, 24, 40)])
def test_churn_kernel_adds_the_documented_noise(bs, H, Wd):
    """cd360_edm_churn_f32 on a churned row: x' is bit-equal to x + (z * s_noise) * noise_std evaluated in fp32 with z from
    ops.sampler_noise (the same seed, streams and step word), for null, all-zero and distinct streams; null streams are stream 0; rows of
    different streams receive different noise.  From x = 0 the result is the noise term itself, held to the float64 restatement of
    tests/philox_ref.py: the bar of test_noise_kernel_equals_the_float64_restatement on z (4 x the float32 evaluation's own error) scaled
    by s_noise noise_std, plus the term's two fp32 products (2^-23 relative)."""
    from cd360 import ops
    _, _, churn = _tables("all")
    hw = H * Wd
    x = torch.randn(bs, 4, H, Wd, generator=torch.Generator(device=DEV).manual_seed(4), device=DEV)
    for seed in (0, BIG_SEED):
        for row in (0, 2):
            std, s_noise = churn[row, 1], churn[row, 2]
            assert float(std) > 0 and float(s_noise) == float(torch.tensor(1.003))
            got = {}
            for name, ids in (("null", None), ("zero", [0] * bs), ("distinct", list(range(3, 3 + bs)))):
                z = ops.sampler_noise(seed_t(seed), streams_t(ids), step_t(row), bs, H, Wd)
                x2 = x.clone()
                assert ops.edm_churn(x2, churn, step_t(row), seed_t(seed), streams_t(ids)) is x2
                assert torch.equal(x2, x + (z * s_noise) * std), (seed, row, name)
                x0 = torch.zeros_like(x)
                ops.edm_churn(x0, churn, step_t(row), seed_t(seed), streams_t(ids))
                rows = [0] * bs if ids is None else ids
                scale = float(s_noise.double() * std.double())
                want = P.batch(seed, rows, row, hw) * scale
                zbar = 4 * float(np.abs(P.batch(seed, rows, row, hw, np.float32) - P.batch(seed, rows, row, hw)).max())
                bar = zbar * scale + 2.0 ** -23 * float(np.abs(want).max())
                err = float(np.abs(x0.cpu().numpy().reshape(bs, 4, hw).astype(np.float64) - want).max())
                print(f"churn {bs}x4x{H}x{Wd} seed {seed} row {row} streams {name}: max |kernel - float64| {err:.3e} | bar {bar:.3e}")
                assert err <= bar, (seed, row, name, err, bar)
                got[name] = x2
            assert torch.equal(got["null"], got["zero"]) and not torch.equal(got["null"], got["distinct"])
            if bs == 2:
                assert not torch.equal(got["distinct"][0] - x[0], got["distinct"][1] - x[1])
    _, _, cw = _tables("cw")
    assert float(cw[0, 1]) == 0.0
    x2 = x.clone()
    ops.edm_churn(x2, cw, step_t(0), seed_t(1), None)
    assert torch.equal(x2, x)


# ================================================================================================ 7: predictor and corrector, bit for bit
def _predict(x, e, row, scale, scale_im):
    """The predictor in the kernels' order, one fp32 rounding per operation (torch's elementwise kernels do not contract) -> (x_e, d)."""
    sh, sn, _, sq = row.unbind()
    d = (x - SC.combine(x, e, sq, scale, scale_im)) / sh
    return x + d * (sn - sh), d


def _correct(x, xe, d, e2, row, crow, scale, scale_im):
    sh, sn = row[0], row[1]
    if not float(sn) > 0.0:
        return xe.clone()
    d_new = (xe - SC.combine(xe, e2, crow[3], scale, scale_im)) / sn
    return x + (d + d_new) / 2.0 * (sn - sh)


ROWS = {"first-row": ("all", 0), "middle-row": ("all", 2), "last-row": ("all", 3), "unchurned-row": ("cw", 0)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(ROWS))
@pytest.mark.parametrize("scale_im", [3.5, 0.0, -1.25, None])
def test_predict_and_correct_equal_a_torch_restatement_in_the_kernels_order(scale_im, case):
    """cd360_cfg_edm_predict_f32 / _cl and cd360_cfg_edm_correct_f32 / _cl, three branches (any finite scale_im) and two: bit-equal to the
    documented expressions evaluated operation by operation in fp32, at a ragged size (W = 40), eps sliced from 16-wide rows; the
    channels-last kernels equal the fp32 kernels on the same values.  Rows: the first (clamped: sq != sigma_hat), a middle one, the last
    (sigma_next = 0: the predictor is defined, the corrector hands back x_e and reads neither eps2 nor d -- both NaN here), and an
    un-churned one, where the in-place predictor without d holds the bits of cfg_euler_step_cl / cfg_euler_step."""
    from cd360 import ops
    tag, row = ROWS[case]
    edm, corr, _ = _tables(tag)
    nb = 2 if scale_im is None else 3
    g = torch.Generator(device=DEV).manual_seed(11)
    bs, H, Wd = 2, 24, 40
    x = torch.randn(bs, 4, H, Wd, generator=g, device=DEV)
    eps16 = torch.randn(nb * bs, H * Wd, 16, generator=g, device=DEV).to(BF)
    eps16b = torch.randn(nb * bs, H * Wd, 16, generator=g, device=DEV).to(BF)
    e, e2 = SC.cl_to_nchw(eps16, nb * bs, H, Wd), SC.cl_to_nchw(eps16b, nb * bs, H, Wd)
    gi, r, cr = step_t(row), edm[row].contiguous(), corr[row].contiguous()
    assert (float(r[3]) != float(r[0])) == (case != "unchurned-row") and (float(r[1]) == 0.0) == (case == "last-row")
    want_e, want_d = _predict(x, e, r, 7.5, scale_im)
    assert torch.isfinite(want_e).all()
    # ---- predictor
    xe, d = ops.cfg_edm_predict(x, e, r, 7.5, scale_im)
    assert torch.equal(xe, want_e) and torch.equal(d, want_d), float((xe - want_e).abs().max())
    xe_only, none = ops.cfg_edm_predict(x, e, r, 7.5, scale_im, want_dir=False)
    assert none is None and torch.equal(xe_only, xe)
    keep, xe2, d2 = x.clone(), torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    assert ops.cfg_edm_predict_cl(x, eps16[..., :4], edm, gi, 7.5, scale_im, xe2, d2) is xe2
    assert torch.equal(xe2, xe) and torch.equal(d2, d) and torch.equal(x, keep)
    x3 = x.clone()
    ops.cfg_edm_predict_cl(x3, eps16[..., :4], edm, gi, 7.5, scale_im, x3)  # in place, no d: the churned Euler tail
    assert torch.equal(x3, xe) and not torch.equal(x3, x)
    if case == "unchurned-row":
        assert torch.equal(ops.cfg_euler_step_cl(x.clone(), eps16[..., :4], edm, gi, 7.5, scale_im), xe)
        assert torch.equal(ops.cfg_euler_step(x, e, r[0:1].contiguous(), r[1:2].contiguous(), 7.5, scale_im), xe)
    # ---- corrector
    want = _correct(x, xe, d, e2, r, cr, 7.5, scale_im)
    nan = float("nan")
    dd, ee2, ee16 = (d, e2, eps16b) if case != "last-row" else (torch.full_like(d, nan), torch.full_like(e2, nan), torch.full_like(eps16b, nan))
    got = ops.cfg_edm_correct(x, xe, dd, ee2, r, cr, 7.5, scale_im)
    assert torch.equal(got, want), float((got - want).abs().max())
    xc = x.clone()
    assert ops.cfg_edm_correct_cl(xc, xe, dd, ee16[..., :4], edm, corr, gi, 7.5, scale_im) is xc
    assert torch.equal(xc, want)
    assert torch.equal(got, xe) == (case == "last-row")


# ================================================================================================ 8: host refusals
@pytest.mark.gpu
def test_host_refuses_bad_arguments():
    """CD360_ERR_ARG before anything is launched: null pointers, bs <= 0, HW <= 0, n <= 0, HW > 2^32 (churn), a bad ld, a misaligned eps, and
    every overlap of x / xe / dir / out that is not allowed; xe == x is accepted by the staged predictor, `dir` and `streams` may be null.  A
    wrong branch count and a NaN scale_im handed in as a number raise ValueError in the wrapper."""
    from cd360 import _lib, ops
    g = torch.Generator(device=DEV).manual_seed(5)
    bs, H, Wd = 1, 4, 8
    n = bs * 4 * H * Wd
    x, xe, d, out = (torch.randn(bs, 4, H, Wd, generator=g, device=DEV) for _ in range(4))
    eps16 = torch.randn(3 * bs, H * Wd, 16, generator=g, device=DEV).to(BF)
    e = torch.randn(3 * bs, 4, H, Wd, generator=g, device=DEV)
    edm, corr, churn = _tables("all")
    seed, gi = seed_t(9), step_t(0)
    r, cr = edm[0].contiguous(), corr[0].contiguous()
    lib, Q = _lib.load(), lambda t: t.data_ptr()  # noqa: E731
    big = 2 ** 32 + 1

    def caller(fn, *defaults):
        return lambda **k: fn(*[k.get(name, dflt) for name, dflt in defaults])

    ch = caller(lib.cd360_edm_churn_f32, ("x", Q(out)), ("tab", Q(churn)), ("step", Q(gi)), ("seed", Q(seed)), ("streams", None), ("bs", 1),
                ("HW", 32), ("stream", None))
    for bad in (dict(x=None), dict(tab=None), dict(step=None), dict(seed=None), dict(bs=0), dict(HW=0), dict(HW=big), dict(seed=Q(seed) + 4)):
        assert ch(**bad) == -1, bad
    pcl = caller(lib.cd360_cfg_edm_predict_cl, ("x", Q(x)), ("eps", Q(eps16)), ("tab", Q(edm)), ("step", Q(gi)), ("scale", 7.5), ("scale_im", 3.5),
                 ("xe", Q(xe)), ("dir", Q(d)), ("bs", 1), ("HW", 32), ("ld", 16), ("stream", None))
    for bad in (dict(x=None), dict(eps=None), dict(tab=None), dict(step=None), dict(xe=None), dict(bs=0), dict(HW=0), dict(ld=2), dict(ld=6),
                dict(eps=Q(eps16) + 4), dict(xe=Q(x) + 16), dict(dir=Q(x)), dict(dir=Q(xe)), dict(dir=Q(xe) + 4 * (n - 1)), dict(xe=Q(x), dir=Q(x))):
        assert pcl(**bad) == -1, bad
    assert pcl(xe=Q(out), dir=None) == 0 and pcl(x=Q(out), xe=Q(out), dir=None) == 0 and pcl(x=Q(out), xe=Q(out)) == 0
    pf = caller(lib.cd360_cfg_edm_predict_f32, ("x", Q(x)), ("eps", Q(e)), ("row", Q(r)), ("scale", 7.5), ("scale_im", 3.5), ("xe", Q(xe)),
                ("dir", Q(d)), ("n", n), ("stream", None))
    for bad in (dict(x=None), dict(eps=None), dict(row=None), dict(xe=None), dict(n=0), dict(xe=Q(x)), dict(xe=Q(e) + 2 * n * 4), dict(dir=Q(x)),
                dict(dir=Q(xe)), dict(dir=Q(e))):
        assert pf(**bad) == -1, bad
    assert pf(xe=Q(out), dir=None) == 0
    assert pf(xe=Q(e) + 2 * n * 4, dir=None, scale_im=float("nan")) == 0  # two branches: the third slab is not an input
    ccl = caller(lib.cd360_cfg_edm_correct_cl, ("x", Q(out)), ("xe", Q(xe)), ("dir", Q(d)), ("eps", Q(eps16)), ("tab", Q(edm)), ("corr", Q(corr)),
                 ("step", Q(gi)), ("scale", 7.5), ("scale_im", 3.5), ("bs", 1), ("HW", 32), ("ld", 16), ("stream", None))
    for bad in (dict(x=None), dict(xe=None), dict(dir=None), dict(eps=None), dict(tab=None), dict(corr=None), dict(step=None), dict(bs=0), dict(HW=0),
                dict(ld=2), dict(ld=6), dict(eps=Q(eps16) + 4), dict(xe=Q(out)), dict(dir=Q(out)), dict(dir=Q(xe)), dict(xe=Q(out) + 16)):
        assert ccl(**bad) == -1, bad
    cf = caller(lib.cd360_cfg_edm_correct_f32, ("x", Q(x)), ("xe", Q(xe)), ("dir", Q(d)), ("eps", Q(e)), ("row", Q(r)), ("crow", Q(cr)), ("scale", 7.5),
                ("scale_im", 3.5), ("out", Q(out)), ("n", n), ("stream", None))
    for bad in (dict(x=None), dict(xe=None), dict(dir=None), dict(eps=None), dict(row=None), dict(crow=None), dict(out=None), dict(n=0),
                dict(out=Q(x)), dict(out=Q(xe)), dict(out=Q(d)), dict(out=Q(e) + 2 * n * 4)):
        assert cf(**bad) == -1, bad
    assert cf(out=Q(e) + 2 * n * 4, scale_im=float("nan")) == 0
    torch.cuda.synchronize()
    with pytest.raises(_lib.Cd360Error):  # channels 2..5 of the 16-wide rows: 4 bytes off the 8-byte alignment
        ops.cfg_edm_predict_cl(x, eps16[..., 2:6], edm, gi, 7.5, 3.5, xe)
    with pytest.raises(ValueError):
        ops.cfg_edm_predict_cl(x, eps16[..., :4], edm, gi, 7.5, None, xe)  # three images, two-branch request
    with pytest.raises(ValueError):
        ops.cfg_edm_predict(x, e, r, 7.5, None)
    with pytest.raises(ValueError):
        ops.cfg_edm_correct(x, xe, d, e, r, cr, 7.5, float("nan"))
    with pytest.raises(_lib.Cd360Error):
        ops.edm_churn(x.clone(), churn.cpu(), gi, seed, None)


# ================================================================================================ 9: guarded runs
GUARDED = []  # (id, declares, bs, H, W, nb, tag, row): what test_every_edm_entry_point_has_a_guarded_case reads
for _bs, _H, _W in ((1, 5, 7), (2, 24, 40)):
    for _nb in (3, 2):
        for _name, _tag, _row in (("middle", "all", 2), ("last", "all", 3), ("unchurned", "cw", 0)):
            GUARDED.append((f"{_nb}-branch-{_name}-row-{_bs}x4x{_H}x{_W}", NEW, _bs, _H, _W, _nb, _tag, _row))


@pytest.mark.gpu
@pytest.mark.parametrize("declares,bs,H,Wd,nb,tag,row", [c[1:] for c in GUARDED], ids=[c[0] for c in GUARDED])
def test_churn_predict_and_correct_write_their_outputs_only(declares, bs, H, Wd, nb, tag, row):
    """All five entry points under tests/guarded.py, both poison patterns: a middle row, the sigma_next = 0 row (the corrector's d and eps2
    are then left POISONED: not read) and an un-churned row (the churn kernel's x is then left POISONED and must still hold the poison:
    neither read nor written).  x, eps and the outputs live in arena blocks between canaries: no guard byte changes; the inputs and tables
    are unchanged; the results are finite and bit-equal between the poisons.  In two-branch form a poisoned third branch sits behind the
    two."""
    from cd360 import ops
    scale_im = 3.5 if nb == 3 else None
    edm, corr, churn = _tables(tag)
    d = dict(x=R(bs, 4, H, Wd, seed=1), e=R(nb * bs, 4, H, Wd, seed=2), e2=R(nb * bs, 4, H, Wd, seed=3), e16=R(nb * bs, H * Wd, 16, seed=7, dtype=BF),
             e16b=R(nb * bs, H * Wd, 16, seed=8, dtype=BF), edm=edm, corr=corr, churn=churn, step=step_t(row), seed=seed_t(BIG_SEED),
             streams=streams_t(list(range(1, bs + 1))))
    tail = bs if nb == 2 else 0
    last, quiet = float(edm[row, 1]) == 0.0, float(churn[row, 1]) == 0.0

    @SC.guardfn
    def fn(x, e, e2, e16, e16b, edm, corr, churn, step, seed, streams, guard):
        T = guard.torch

        def arena(src, rows=None, fill=True):
            t = T.empty(((rows or src.shape[0]),) + tuple(src.shape[1:]), dtype=src.dtype, device=DEV)
            if fill:
                t[:src.shape[0]].copy_(src)
            return t

        ge, ge16 = arena(e, nb * bs + tail), arena(e16, nb * bs + tail)
        ge2, ge16b = arena(e2, nb * bs + tail, fill=not last), arena(e16b, nb * bs + tail, fill=not last)  # the last row reads no eps2
        r, cr = edm[row].contiguous(), corr[row].contiguous()
        # churn: on the un-churned row x stays poisoned and untouched
        gx = arena(x, fill=not quiet)
        assert ops.edm_churn(gx, churn, step, seed, streams) is gx
        if quiet:
            assert bool((gx.view(torch.uint8) == guard.arena.poison).all()), "the churn kernel touched x on a noise_std == 0 row"
            gx.copy_(x)
        # predictor: fp32 form into the binding's arena blocks, staged form into this case's
        xe, dv = ops.cfg_edm_predict(gx, ge[:nb * bs], r, 7.5, scale_im)
        gxe, gd = arena(x, fill=False), arena(x, fill=False)
        ops.cfg_edm_predict_cl(gx, ge16[:nb * bs, :, :4], edm, step, 7.5, scale_im, gxe, gd)
        gin = arena(gx)
        ops.cfg_edm_predict_cl(gin, ge16[:nb * bs, :, :4], edm, step, 7.5, scale_im, gin)
        assert torch.equal(gin, gxe)
        # corrector: on the last row d is a poisoned block of its own
        dpo = arena(x, fill=False) if last else dv
        out = ops.cfg_edm_correct(gx, xe, dpo, ge2[:nb * bs], r, cr, 7.5, scale_im)
        gxc = arena(gx)
        ops.cfg_edm_correct_cl(gxc, gxe, arena(x, fill=False) if last else gd, ge16b[:nb * bs, :, :4], edm, corr, step, 7.5, scale_im)
        assert torch.equal(ge[:nb * bs], e) and torch.equal(ge16[:nb * bs], e16), "eps was written"
        return gx.clone(), xe, (xe if last else dv), gxe, out, gxc

    (xh, xe, dv, gxe, out, gxc), _ = G.run_twice(fn, d, declares=declares)
    r, cr = edm[row], corr[row]
    want_e, want_d = _predict(xh, d["e"], r, 7.5, scale_im)
    assert torch.equal(xe, want_e) and (last or torch.equal(dv, want_d))
    assert torch.equal(xh, d["x"]) == quiet
    assert torch.equal(out, _correct(xh, xe, want_d, d["e2"], r, cr, 7.5, scale_im))
    e_cl, e2_cl = SC.cl_to_nchw(d["e16"], nb * bs, H, Wd), SC.cl_to_nchw(d["e16b"], nb * bs, H, Wd)
    cl_e, cl_d = _predict(xh, e_cl, r, 7.5, scale_im)
    assert torch.equal(gxe, cl_e) and torch.equal(gxc, _correct(xh, cl_e, cl_d, e2_cl, r, cr, 7.5, scale_im))


def test_every_edm_entry_point_has_a_guarded_case():
    """The twin of test_every_stochastic_entry_point_has_a_guarded_case for include/cd360_edm.h (runs without a GPU): every
    `int cd360_...(` the header declares is in some guarded case's `declares` in this file, and is typed in EDM_SIGNATURES."""
    from cd360 import _lib
    untyped, unknown, uncovered = SC.check_guarded_cover("cd360_edm.h", _lib.EDM_SIGNATURES, GUARDED)
    assert not untyped, untyped
    assert not unknown, unknown
    assert not uncovered, f"launching entry points without a guarded case: {sorted(uncovered)}"


# ================================================================================================ 10: the GPU trajectories
@pytest.mark.gpu
@torch.no_grad()
@pytest.mark.parametrize("solver,tag", [("euler", "c1"), ("euler", "cw"), ("heun", "c0"), ("heun", "cw")])
@pytest.mark.parametrize("name", ["cfg3", "cfg2"])
def test_fused_steps_on_the_gpu_walk_the_reference_trajectory(name, solver, tag):
    """The product's step functions (cd360.sampler.fused_cfg_edm_euler_step / fused_cfg_heun_step, the tails on cd360_cfg_edm_predict_f32 /
    cd360_cfg_edm_correct_f32, the golden's stored z handed in as the noise) ON THE GPU over the 12-step trajectories of
    tests/golden/sampler_edm.npz, written by the REFERENCE's own classes; the bar of the CPU twins."""
    from test_edm_cpu import load, run_product_steps
    g = load()
    got, xs = run_product_steps(g, solver, name, DEV, fused=True, tag=tag)
    assert got.is_cuda
    key = f"{solver}_{name}_12_{tag}"
    err = float((got.cpu() - g[key]).abs().max())
    print(f"{key}: fused GPU trajectory vs the reference's golden, max abs:", err, "of max", float(g[key].abs().max()))
    assert torch.allclose(got.cpu(), g[key], atol=2e-5, rtol=1e-5), err
    for i in range(12):
        assert torch.allclose(xs[i].cpu(), g[key + "_x"][i], atol=2e-5, rtol=1e-5), i


# ================================================================================================ 11 - 13: the job
JOBS = {"heun-c0": dict(solver="heun"), "heun-cw": dict(solver="heun", **CW), "euler-c1": dict(solver="euler", **C1)}


def _edm_job(which):
    """SC.walk for a key of JOBS, or for "euler": the plain solver the others are told apart from."""
    return SC.walk(**JOBS.get(which, {}))


@pytest.fixture(scope="module", autouse=True)
def _release_the_shared_job():
    yield
    SC.release()


@pytest.mark.gpu
@torch.no_grad()
@pytest.mark.parametrize("which", list(JOBS))
def test_edm_job_through_its_captured_graphs(which):
    """Sampler(n_steps=4, use_graph=True) over 3 poses x all 4 steps for un-churned Heun, Heun with the windowed churn and churned Euler.
    All graphs captured and staged -- Heun holds three (steady: two evaluations; render; the one-evaluation sigma_next = 0 step) and
    smp.gxe / smp.gdir.  Every pose bit-identical to a fresh graph-mode sampler's (the render graph's corrector evaluation must read THIS
    step's render, pose after pose) and to use_graph=False, and a step replayed twice from the same x gives the same bits.  Each differs
    from plain Euler by more than 1e-3 of the maximum."""
    from cd360 import job, solvers
    kw = JOBS[which]
    latents, smp = _edm_job(which)
    assert latents.shape == (POSES, 4, LATENT, LATENT) and torch.isfinite(latents).all()
    assert smp.solver == kw["solver"] and smp._solver is solvers.EDM_SOLVERS[kw["solver"]] and smp.staged and smp.branches == 3
    assert smp.graph is not None and smp.rgraph is not None
    for tab in (smp.edm_tab, smp.corr_tab, smp.churn_tab):
        assert tab.shape == (STEPS, 4) and tab.dtype == torch.float32 and tab.is_cuda
    assert smp.corr_tab[-1, 0] == 0 and torch.equal(smp.edm_tab[:, 1], smp.sigmas[1:])
    if kw["solver"] == "heun":
        assert smp.lgraph is not None and smp.gxe.shape == smp.gx.shape == smp.gdir.shape
    else:
        assert smp.lgraph is None
    if which == "heun-c0":
        assert not smp.churned and torch.equal(smp.edm_tab[:, 3], smp.edm_tab[:, 0]) and not hasattr(smp, "seed_buf")
    else:
        assert smp.churned and smp.seed_buf.tolist() == [SEED] and smp.streams_buf.tolist() == [0]
        assert (smp.churn_tab[:, 1] > 0).tolist() == ([False, True, True, True] if which == "heun-cw" else [True] * 4)
    for p in range(POSES):
        pose, ctx, y, x0 = SC.job(p)
        fresh = job.sample_assigned(SC.sampler(pose, ctx, y, **kw), [(pose, ctx, y, x0)], STEPS)[0]
        assert torch.equal(fresh, latents[p:p + 1]), (p, float((fresh - latents[p:p + 1]).abs().max()))
        eager = job.sample_assigned(SC.sampler(pose, ctx, y, use_graph=False, **kw), [(pose, ctx, y, x0)], STEPS)[0]
        assert torch.equal(eager, latents[p:p + 1]), (p, float((eager - latents[p:p + 1]).abs().max()))
    pose, ctx, y, x0 = SC.job(0)
    smp.retarget(pose, ctx, y)
    x1 = smp.step(x0.clone(), 0)
    for i in (1, 2, 3):  # step i twice from the same x: the same bits
        a, b = smp.step(x1, i), smp.step(x1, i)
        assert torch.equal(a, b) and not torch.equal(a, x1), i
    assert torch.equal(smp.step(x0.clone(), 0), x1)
    eul, esmp = _edm_job("euler")
    assert esmp._solver is solvers.SOLVERS["euler"] and esmp.lgraph is None
    for p in range(POSES):
        d = float((eul[p] - latents[p]).abs().max() / latents[p].abs().max())
        print(f"{which} pose {p}: vs plain Euler, 4 steps: rel", d)
        assert d > 1e-3, (p, d)


@pytest.mark.gpu
@torch.no_grad()
def test_one_step_heun_is_one_step_euler():
    """n_steps = 1: the only step is the sigma_next = 0 row, Heun's corrector is skipped and the predictor on the EDM tables must hold the
    Euler step's bits -- graph mode (Heun launches this step un-captured) and eager."""
    pose, ctx, y, x0 = SC.job(0)
    for use_graph in (True, False):
        h = SC.sampler(pose, ctx, y, n_steps=1, solver="heun", use_graph=use_graph)
        e = SC.sampler(pose, ctx, y, n_steps=1, solver="euler", use_graph=use_graph)
        a, b = h.step(x0.clone(), 0), e.step(x0.clone(), 0)
        assert torch.isfinite(a).all() and torch.equal(a, b), float((a - b).abs().max())
        assert torch.equal(h.edm_tab[0, :3], e.step_tab[0, :3])


@pytest.mark.gpu
@torch.no_grad()
def test_unstaged_route_serves_heun_and_churn():
    """With routes.no_stage the un-staged route carries both: finite, graph mode equal to its own eager run, and not the Euler result."""
    from cd360 import job, routes
    pose, ctx, y, x0 = SC.job(0)
    with routes.override(no_stage=True):
        u_eul = job.sample_assigned(SC.sampler(pose, ctx, y, use_graph=False, solver="euler"), [(pose, ctx, y, x0)], STEPS)[0]
        for which in ("heun-cw", "euler-c1"):
            g_smp = SC.sampler(pose, ctx, y, **JOBS[which])
            e_smp = SC.sampler(pose, ctx, y, use_graph=False, **JOBS[which])
            assert not g_smp.staged and not e_smp.staged
            got_g = job.sample_assigned(g_smp, [(pose, ctx, y, x0)], STEPS)[0]
            got_e = job.sample_assigned(e_smp, [(pose, ctx, y, x0)], STEPS)[0]
            assert g_smp.graph is not None and torch.isfinite(got_g).all()
            assert torch.equal(got_g, got_e), (which, float((got_g - got_e).abs().max()))
            assert float((got_g - u_eul).abs().max() / u_eul.abs().max()) > 1e-3, which


@pytest.mark.gpu
@torch.no_grad()
def test_captured_churn_follows_seed_and_streams():
    """The captured churn isolated: from ONE snapshot of gx, step 1 of churned Euler replayed under seed A and under seed B (reseed: no
    re-capture) differs; set_noise_streams changes the result and restoring it restores the bits.  On a gamma = 0 row -- row 0 of the
    windowed setting, under Heun's render graph -- the two seeds give bit-equal x.  (The noise passes through the UNet here: the
    difference term itself is held at the kernel level, test_churn_kernel_adds_the_documented_noise.)"""
    _, smp = _edm_job("euler-c1")
    pose, ctx, y, x0 = SC.job(0)
    smp.retarget(pose, ctx, y)
    snap = smp.step(x0.clone(), 0)
    graph, res = smp.graph, {}
    for seed in (SEED, SEED + 1):
        smp.reseed(seed)
        res[seed] = smp.step(snap, 1)
    assert smp.graph is graph and smp.seed_buf.tolist() == [SEED + 1]
    assert not torch.equal(res[SEED], res[SEED + 1]) and torch.isfinite(res[SEED + 1]).all()
    smp.set_noise_streams([1])
    moved = smp.step(snap, 1)
    assert smp.streams_buf.tolist() == [1] and not torch.equal(moved, res[SEED + 1])
    smp.set_noise_streams([0])
    assert torch.equal(smp.step(snap, 1), res[SEED + 1])
    smp.reseed(SEED)  # (ends on the fixture's seed)
    assert torch.equal(smp.step(snap, 1), res[SEED])
    _, win = _edm_job("heun-cw")
    win.retarget(pose, ctx, y)
    first = {}
    for seed in (SEED + 1, SEED):
        win.reseed(seed)
        first[seed] = win.step(x0.clone(), 0)
    assert float(win.churn_tab[0, 1]) == 0.0 and torch.equal(first[SEED], first[SEED + 1])
    later = {}
    for seed in (SEED + 1, SEED):
        win.reseed(seed)
        later[seed] = win.step(first[SEED], 1)
    assert not torch.equal(later[SEED], later[SEED + 1])


@pytest.mark.gpu
@torch.no_grad()
@pytest.mark.parametrize("which", ["euler-c1", "heun-c0", "heun-cw"])
@pytest.mark.parametrize("nb", [3, 2])
def test_edm_job_agrees_with_the_uncaptured_module_route(nb, which):
    """Whole trajectory, n_steps = 4, all 4 steps, the same seed: the same UNet under cd360.sampler.EulerEDMSampler / HeunEDMSampler(seed=...)
    + the guider + DiscreteDenoiser (the YAML's classes, eager, the implicit-GEMM input convolution) against the job sampler (captured,
    staged, the tables).  Both routes draw the same noise (the class's step word is the step index, like the kernels'), so they differ as
    under plain Euler -- by the staged input convolution rounding a few bf16 values to the other neighbour, amplified by 70 random-init
    blocks.
    Bar: what the SAME comparison gives under plain EULER on the parent commit at the same branch count, measured on the same box in the
    same session (tools/solver_report.py), times 2 for churned Euler (the margin the ancestral test grants a larger step) and times 4 for
    Heun (two evaluations per step, each contributing that rounding).  Measured figures: DESIGN.md section 6.3."""
    from cd360 import job
    from cd360 import sampler as S
    kw = dict(JOBS[which])
    solver = kw.pop("solver")
    net = SC.net()
    pose, ctx, y, x0 = SC.job(0, nb)
    got = job.sample_assigned(SC.sampler(pose, ctx, y, scale_im=3.5 if nb == 3 else 0, solver=solver, **kw), [(pose, ctx, y, x0)], STEPS)[0]
    mod = (S.HeunEDMSampler if solver == "heun" else S.EulerEDMSampler)(num_steps=STEPS, guider_config=SC.guider_config(nb), device=DEV, seed=SEED, **kw)
    x = SC.module_route(net, mod, solver, nb, pose, ctx, y, x0, STEPS)
    dev = float((got - x).abs().max() / x.abs().max())
    bar = BAR_FACTOR[solver] * PARENT_EULER_JOB_VS_MODULE_REL[nb]
    print(f"{which} {nb}-branch job vs module route, 4 steps: max abs", float((got - x).abs().max()), "rel", dev, "| bar", bar)
    assert torch.isfinite(got).all() and dev <= bar, (dev, bar)
