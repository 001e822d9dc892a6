"""DPM++ 2S ancestral and linear multistep on the captured HIP step: the six tails of include/cd360_highorder.h bit for bit against a torch
restatement, the noise term against the float64 restatement of the device noise (tests/philox_ref.py), host refusals, memory safety, the
GPU trajectories against the reference's goldens, and the sampling job with solver="dpmpp2s_a" and solver="lms".  Needs an MI355X."""
import functools

import numpy as np
import pytest
import torch

import guarded as G
import philox_ref as P
import sampler_cases as SC
from sampler_cases import BF, DEV, LATENT, POSES, SEED, STEPS, R, seed_t, step_t, streams_t

NEW = ["cd360_cfg_dpmpp2s_mid_cl", "cd360_cfg_dpmpp2s_mid_f32", "cd360_cfg_dpmpp2s_step_cl", "cd360_cfg_dpmpp2s_step_f32", "cd360_cfg_lms_step_cl",
       "cd360_cfg_lms_step_f32"]
BIG_SEED = 2 ** 63 + 12345
SHAPES = [(1, 5, 7), (2, 24, 40)]
SCALE_IMS = [3.5, 0.0, -1.25, None]

# The module-route test's yardstick: the SAME comparison (captured job sampler against the un-captured module route, n_steps = 4, all 4
# steps, latent 32 / 6 views, bs = 1) under plain EULER on the parent commit, measured with tools/solver_report.py --solver euler --repo
# <parent checkout> on the box and in the session of this change, per branch count: three branches 5.488e-2 of the latent's maximum, two
# branches 6.147e-2.
PARENT_EULER_JOB_VS_MODULE_REL = {3: 0.05488, 2: 0.06147}
BAR_FACTOR = {"lms": 2, "dpmpp2s_a": 4}  # one evaluation per step, as DPM++ 2M is granted; two evaluations per step, as Heun is granted


@functools.lru_cache(maxsize=None)
def _tables(eta, s_noise=1.05):
    """A 4-step schedule's own tables on the device: (step_tab, anc_tab, mid_tab, mult2s_tab)."""
    from cd360 import sampler as S
    sig = S.LegacyDDPMDiscretization()(4)
    anc, mid, mult = S.dpmpp2s_tables(sig, S.DiscreteDenoiser(), eta, s_noise)
    tab = torch.stack([sig[:-1], sig[1:], torch.ones(4), torch.zeros(4)], 1).contiguous()
    return tuple(t.to(DEV) for t in (tab, anc, mid, mult))


@functools.lru_cache(maxsize=None)
def _lms_tables(order, steps=6):
    from cd360 import sampler as S
    sig = S.LegacyDDPMDiscretization()(steps)
    tab = torch.stack([sig[:-1], sig[1:], torch.ones(steps), torch.zeros(steps)], 1).contiguous()
    return tab.to(DEV), S.lms_coefficients(sig, order).to(DEV)


# ================================================================================================ 6: the kernels, bit for bit
def _mid(x, e, s, mult, scale, scale_im):
    """The midpoint in the kernels' order, one fp32 rounding per operation (torch's elementwise kernels do not contract)."""
    return mult[0] * x - mult[1] * SC.combine(x, e, s, scale, scale_im)


def _step2s(x, x2, e2, midrow, mult, anc, z, scale, scale_im):
    xn = mult[2] * x - mult[3] * SC.combine(x2, e2, midrow[3], scale, scale_im)
    return xn if float(anc[1]) == 0.0 else xn + (z * anc[2]) * anc[1]


def _lms(x, e, ring, s, coef, i, scale, scale_im):
    """-> x'; ring [order, ...] updated in place, slot i % order"""
    order = ring.shape[0]
    d = (x - SC.combine(x, e, s, scale, scale_im)) / s
    ring[i % order] = d
    acc = coef[0] * d
    for j in range(1, min(i + 1, order)):
        acc = acc + coef[j] * ring[(i - j) % order]
    return x + acc


ROWS = {"first-row": (1.0, 0), "middle-row": (1.0, 2), "last-row": (1.0, 3), "single-row": (1.5, 1)}  # (eta, row of the 4-step schedule)


@pytest.mark.gpu
@pytest.mark.parametrize("bs,H,Wd", SHAPES)
@pytest.mark.parametrize("scale_im", SCALE_IMS)
def test_dpmpp2s_kernels_equal_a_torch_restatement_in_the_kernels_order(scale_im, bs, H, Wd):
    """cd360_cfg_dpmpp2s_mid_f32 / _cl and cd360_cfg_dpmpp2s_step_f32 / _cl, three branches (any finite scale_im) and two, eps at ld 4 and
    8: bit-equal to the documented expressions evaluated operation by operation in fp32 with z taken from cd360_sampler_noise_f32; the
    channels-last kernels equal the fp32 kernels on the same values.  Rows of a 4-step schedule: first, middle, last (sigma_down = 0: the
    filler row, m = 0 and sigma_up = 0: finite, nothing drawn) and a one-evaluation row of eta 1.5 (filler with sigma_up != 0).  x stays
    untouched by the midpoint; sq_mid differs from sigma_mid on the two-evaluation rows."""
    from cd360 import ops
    nb = 2 if scale_im is None else 3
    x = R(bs, 4, H, Wd, seed=11)
    (cl_forms, e), (cl2_forms, e2) = SC.eps_forms(nb, bs, H, Wd, 12), SC.eps_forms(nb, bs, H, Wd, 13)
    seed, streams = seed_t(BIG_SEED), streams_t(list(range(3, 3 + bs)))
    for case, (eta, row) in ROWS.items():
        tab, anc, mid, mult = _tables(eta)
        gi = step_t(row)
        s, a, m, mu = tab[row, 0:1].contiguous(), anc[row].contiguous(), mid[row].contiguous(), mult[row].contiguous()
        single = case in ("last-row", "single-row")
        assert (float(a[0]) == 0.0) == single and (float(m[3]) != float(m[0])) == (not single) and (float(a[1]) == 0.0) == (case == "last-row")
        want2 = _mid(x, e, s, mu, 7.5, scale_im)
        x2 = ops.cfg_dpmpp2s_mid(x, e, s, mu, 7.5, scale_im)
        assert torch.equal(x2, want2) and torch.isfinite(x2).all(), (case, float((x2 - want2).abs().max()))
        for ecl in cl_forms:
            keep, x2c = x.clone(), torch.full_like(x, float("nan"))
            assert ops.cfg_dpmpp2s_mid_cl(x, ecl, tab, mult, gi, 7.5, scale_im, x2c) is x2c
            assert torch.equal(x2c, x2) and torch.equal(x, keep), (case, ecl.stride(1))
        z = ops.sampler_noise(seed, streams, gi, bs, H, Wd)
        want = _step2s(x, x2, e2, m, mu, a, z, 7.5, scale_im)
        got = ops.cfg_dpmpp2s_step(x, x2, e2, m, mu, a, seed, streams, gi, 7.5, scale_im)
        assert torch.equal(got, want) and torch.isfinite(got).all(), (case, float((got - want).abs().max()))
        for ecl in cl2_forms:
            xc = x.clone()
            assert ops.cfg_dpmpp2s_step_cl(xc, x2, ecl, mid, mult, anc, gi, seed, streams, 7.5, scale_im) is xc
            assert torch.equal(xc, got), (case, ecl.stride(1))
        if not single:
            assert not torch.equal(got, x) and not torch.equal(x2, x)
            null = ops.cfg_dpmpp2s_step(x, x2, e2, m, mu, a, seed, None, gi, 7.5, scale_im)  # null streams = stream 0 for every row
            zero = ops.cfg_dpmpp2s_step(x, x2, e2, m, mu, a, seed, streams_t([0] * bs), gi, 7.5, scale_im)
            assert torch.equal(null, zero) and not torch.equal(null, got)
        if case == "last-row":  # no noise: the seed does not matter
            assert torch.equal(ops.cfg_dpmpp2s_step(x, x2, e2, m, mu, a, seed_t(1), None, gi, 7.5, scale_im), got)


@pytest.mark.gpu
@pytest.mark.parametrize("order", [4, 3])
@pytest.mark.parametrize("bs,H,Wd", SHAPES)
@pytest.mark.parametrize("scale_im", SCALE_IMS)
def test_lms_kernels_equal_a_torch_restatement_in_the_kernels_order(scale_im, bs, H, Wd, order):
    """cd360_cfg_lms_step_f32 / _cl over steps 0..5 of a 6-step schedule, the ring carried from step to step and PRE-FILLED WITH NaN: every
    result is finite and bit-equal to the documented expression evaluated operation by operation in fp32; step i writes slot i % order --
    the ring wraps at step 4 (order 4) resp. 3 (order 3) -- and every other slot keeps its bits, the NaN of the slots not yet written
    included; the channels-last kernel (ld 4 and 8) equals the fp32 kernel."""
    from cd360 import ops
    nb = 2 if scale_im is None else 3
    tab, lms = _lms_tables(order)
    nan = float("nan")
    ring_ref = torch.full((order, bs, 4, H, Wd), nan, device=DEV)
    rings = [ring_ref.clone() for _ in range(3)]  # fp32 form, ld 4, ld 8
    wrapped = False
    for i in range(6):
        x = R(bs, 4, H, Wd, seed=20 + i)
        cl_forms, e = SC.eps_forms(nb, bs, H, Wd, 40 + i)
        s, coef, gi = tab[i, 0:1].contiguous(), lms[i].contiguous(), step_t(i)
        before = ring_ref.clone()
        want = _lms(x, e, ring_ref, s, coef, i, 7.5, scale_im)
        assert torch.isfinite(want).all() and not torch.equal(want, x)
        got = ops.cfg_lms_step(x, e, rings[0], s, coef, gi, 7.5, scale_im)
        assert torch.equal(got, want), (i, float((got - want).abs().max()))
        for ring, ecl in zip(rings[1:], cl_forms):
            xc = x.clone()
            assert ops.cfg_lms_step_cl(xc, ring, ecl, tab, lms, gi, 7.5, scale_im) is xc
            assert torch.equal(xc, want), (i, ecl.stride(1))
        slot = i % order
        wrapped |= i >= order and slot == i - order
        for ring in rings:
            assert torch.equal(ring[slot], ring_ref[slot]) and torch.isfinite(ring[slot]).all(), i
            for other in range(order):
                if other != slot:  # bits, not values: unwritten slots hold NaN
                    assert torch.equal(ring[other].view(torch.int32), before[other].view(torch.int32)), (i, other)
        assert bool(torch.isnan(ring_ref[i + 1:]).all())  # slots no step has reached yet
    assert wrapped and torch.isfinite(ring_ref).all()


# ================================================================================================ 7: the 2S noise term
@pytest.mark.gpu
@pytest.mark.parametrize("bs,H,Wd", SHAPES)
def test_dpmpp2s_step_adds_the_documented_noise(bs, H, Wd):
    """cd360_cfg_dpmpp2s_step_f32 on a noisy row minus the same call on the row with sigma_up = 0 equals (z * s_noise) * sigma_up with z
    from the float64 restatement of tests/philox_ref.py (step word = the step index, tag word 0, the row's stream).  Bar: that of
    test_noise_kernel_equals_the_float64_restatement on z (4 x the float32 evaluation's own error) scaled by s_noise sigma_up, plus the
    term's two fp32 products (2^-23 of the term) and the one fp32 rounding between the term and the difference -- the sum x_n + term, at the
    result's magnitude (2^-24 of max |out|); the difference itself is formed in float64, where it is exact."""
    from cd360 import ops
    tab, anc, mid, mult = _tables(1.0)
    hw = H * Wd
    x, x2, e2 = R(bs, 4, H, Wd, seed=1), R(bs, 4, H, Wd, seed=2), R(3 * bs, 4, H, Wd, seed=3)
    for seed in (0, BIG_SEED):
        for row in (0, 2):
            a, m, mu = anc[row].contiguous(), mid[row].contiguous(), mult[row].contiguous()
            quiet_row = torch.stack([a[0], torch.zeros_like(a[1]), a[2], a[3]])
            assert float(a[1]) > 0 and float(a[2]) == float(torch.tensor(1.05))
            for ids in (None, list(range(3, 3 + bs))):
                noisy = ops.cfg_dpmpp2s_step(x, x2, e2, m, mu, a, seed_t(seed), streams_t(ids), step_t(row), 7.5, 3.5)
                quiet = ops.cfg_dpmpp2s_step(x, x2, e2, m, mu, quiet_row, seed_t(seed), streams_t(ids), step_t(row), 7.5, 3.5)
                rows = [0] * bs if ids is None else ids
                scale = float(a[2].double() * a[1].double())
                want = P.batch(seed, rows, row, hw) * scale
                zbar = 4 * float(np.abs(P.batch(seed, rows, row, hw, np.float32) - P.batch(seed, rows, row, hw)).max())
                bar = zbar * scale + 2.0 ** -23 * float(np.abs(want).max()) + 2.0 ** -24 * float(noisy.abs().max())
                err = float(np.abs((noisy.double() - quiet.double()).cpu().numpy().reshape(bs, 4, hw) - want).max())
                print(f"2s noise term {bs}x4x{H}x{Wd} seed {seed} row {row} streams {ids}: max |kernel - float64| {err:.3e} | bar {bar:.3e}")
                assert float(np.abs(want).max()) > 0.1 and err <= bar, (seed, row, ids, err, bar)


# ================================================================================================ 8: host refusals
@pytest.mark.gpu
def test_host_refuses_bad_arguments():
    """CD360_ERR_ARG before anything is launched, one assertion per case: a null pointer, an overlap among x / x2 / ring / out, a misaligned
    eps, ld < 4 or ld % 4, bs <= 0, HW <= 0, n <= 0, HW > 2^32 where noise is drawn, order outside 1..4; `streams` may be null.  A wrong branch
    count and a NaN scale_im handed in as a number raise ValueError in the wrapper."""
    from cd360 import _lib, ops
    bs, H, Wd = 1, 4, 8
    n = bs * 4 * H * Wd
    x, x2, out = (R(bs, 4, H, Wd, seed=s) for s in (1, 2, 3))
    ring = R(4, bs, 4, H, Wd, seed=4)
    eps16 = R(3 * bs, H * Wd, 16, seed=5, dtype=BF)
    e = R(3 * bs, 4, H, Wd, seed=6)
    tab, anc, mid, mult = _tables(1.0)
    ltab, lms = _lms_tables(4)
    seed, gi = seed_t(9), step_t(0)
    s, a, m, mu, lr = tab[0, 0:1].contiguous(), anc[0].contiguous(), mid[0].contiguous(), mult[0].contiguous(), lms[0].contiguous()
    lib, Q = _lib.load(), lambda t: t.data_ptr()  # noqa: E731
    big = 2 ** 32 + 1

    def caller(fn, *defaults):
        return lambda **k: fn(*[k.get(name, dflt) for name, dflt in defaults])

    mcl = caller(lib.cd360_cfg_dpmpp2s_mid_cl, ("x", Q(x)), ("eps", Q(eps16)), ("tab", Q(tab)), ("mult", Q(mult)), ("step", Q(gi)), ("scale", 7.5),
                 ("scale_im", 3.5), ("x2", Q(x2)), ("bs", 1), ("HW", 32), ("ld", 16), ("stream", None))
    for bad in (dict(x=None), dict(eps=None), dict(tab=None), dict(mult=None), dict(step=None), dict(x2=None), dict(bs=0), dict(HW=0), dict(ld=2),
                dict(ld=6), dict(eps=Q(eps16) + 4), dict(x2=Q(x)), dict(x2=Q(x) + 16), dict(x2=Q(x) + 4 * (n - 1))):
        assert mcl(**bad) == -1, bad
    assert mcl(x2=Q(out)) == 0
    mf = caller(lib.cd360_cfg_dpmpp2s_mid_f32, ("x", Q(x)), ("eps", Q(e)), ("sigma", Q(s)), ("mult", Q(mu)), ("scale", 7.5), ("scale_im", 3.5),
                ("x2", Q(x2)), ("n", n), ("stream", None))
    for bad in (dict(x=None), dict(eps=None), dict(sigma=None), dict(mult=None), dict(x2=None), dict(n=0), dict(x2=Q(x)), dict(x2=Q(e)),
                dict(x2=Q(e) + 2 * n * 4)):
        assert mf(**bad) == -1, bad
    assert mf(x2=Q(out)) == 0
    assert mf(x2=Q(e) + 2 * n * 4, scale_im=float("nan")) == 0  # two branches: the third slab is not an input
    scl = caller(lib.cd360_cfg_dpmpp2s_step_cl, ("x", Q(out)), ("x2", Q(x2)), ("eps", Q(eps16)), ("mid", Q(mid)), ("mult", Q(mult)), ("anc", Q(anc)),
                 ("step", Q(gi)), ("seed", Q(seed)), ("streams", None), ("scale", 7.5), ("scale_im", 3.5), ("bs", 1), ("HW", 32), ("ld", 16),
                 ("stream", None))
    for bad in (dict(x=None), dict(x2=None), dict(eps=None), dict(mid=None), dict(mult=None), dict(anc=None), dict(step=None), dict(seed=None),
                dict(bs=0), dict(HW=0), dict(HW=big), dict(ld=2), dict(ld=6), dict(eps=Q(eps16) + 4), dict(seed=Q(seed) + 4), dict(x2=Q(out)),
                dict(x2=Q(out) + 16)):
        assert scl(**bad) == -1, bad
    assert scl() == 0
    sf = caller(lib.cd360_cfg_dpmpp2s_step_f32, ("x", Q(x)), ("x2", Q(x2)), ("eps", Q(e)), ("mid", Q(m)), ("mult", Q(mu)), ("anc", Q(a)),
                ("seed", Q(seed)), ("streams", None), ("step", Q(gi)), ("scale", 7.5), ("scale_im", 3.5), ("out", Q(out)), ("bs", 1), ("HW", 32),
                ("stream", None))
    for bad in (dict(x=None), dict(x2=None), dict(eps=None), dict(mid=None), dict(mult=None), dict(anc=None), dict(seed=None), dict(step=None),
                dict(out=None), dict(bs=0), dict(HW=0), dict(HW=big), dict(out=Q(x)), dict(out=Q(x2)), dict(out=Q(e) + 2 * n * 4)):
        assert sf(**bad) == -1, bad
    assert sf() == 0 and sf(out=Q(e) + 2 * n * 4, scale_im=float("nan")) == 0
    lcl = caller(lib.cd360_cfg_lms_step_cl, ("x", Q(out)), ("ring", Q(ring)), ("eps", Q(eps16)), ("tab", Q(ltab)), ("lms", Q(lms)), ("step", Q(gi)),
                 ("scale", 7.5), ("scale_im", 3.5), ("order", 4), ("bs", 1), ("HW", 32), ("ld", 16), ("stream", None))
    for bad in (dict(x=None), dict(ring=None), dict(eps=None), dict(tab=None), dict(lms=None), dict(step=None), dict(order=0), dict(order=5),
                dict(bs=0), dict(HW=0), dict(ld=2), dict(ld=6), dict(eps=Q(eps16) + 4), dict(x=Q(ring)), dict(x=Q(ring) + 3 * n * 4),
                dict(ring=Q(out) + 16)):
        assert lcl(**bad) == -1, bad
    assert lcl() == 0 and lcl(x=Q(ring) + 3 * n * 4, order=3) == 0  # the fourth slot is not part of an order-3 ring
    lf = caller(lib.cd360_cfg_lms_step_f32, ("x", Q(x)), ("eps", Q(e)), ("ring", Q(ring)), ("sigma", Q(s)), ("row", Q(lr)), ("step", Q(gi)),
                ("scale", 7.5), ("scale_im", 3.5), ("order", 4), ("out", Q(out)), ("n", n), ("stream", None))
    for bad in (dict(x=None), dict(eps=None), dict(ring=None), dict(sigma=None), dict(row=None), dict(step=None), dict(out=None), dict(n=0),
                dict(order=0), dict(order=5), dict(out=Q(x)), dict(out=Q(e) + 2 * n * 4), dict(out=Q(ring) + 3 * n * 4), dict(ring=Q(x)),
                dict(x=Q(ring) + 3 * n * 4), dict(ring=Q(e))):
        assert lf(**bad) == -1, bad
    assert lf() == 0 and lf(out=Q(ring) + 3 * n * 4, order=3) == 0
    torch.cuda.synchronize()
    with pytest.raises(_lib.Cd360Error):  # channels 2..5 of the 16-wide rows: 4 bytes off the 8-byte alignment
        ops.cfg_lms_step_cl(x.clone(), ring, eps16[..., 2:6], ltab, lms, gi, 7.5, 3.5)
    with pytest.raises(ValueError):
        ops.cfg_dpmpp2s_mid_cl(x, eps16[..., :4], tab, mult, gi, 7.5, None, x2)  # three images, two-branch request
    with pytest.raises(ValueError):
        ops.cfg_dpmpp2s_mid(x, e, s, mu, 7.5, None)
    with pytest.raises(ValueError):
        ops.cfg_lms_step(x, e, ring, s, lr, gi, 7.5, float("nan"))
    with pytest.raises(_lib.Cd360Error):
        ops.cfg_dpmpp2s_step(x, x2, e, m.cpu(), mu, a, seed, None, gi, 7.5, 3.5)


# ================================================================================================ 9: guarded runs
GUARDED = []  # (id, declares, bs, H, W, nb, eta, row): what test_every_highorder_entry_point_has_a_guarded_case reads
for _bs, _H, _W in SHAPES:
    for _nb in (3, 2):
        for _name, _eta, _row in (("middle", 1.0, 2), ("last", 1.0, 3), ("single", 1.5, 1)):
            GUARDED.append((f"{_nb}-branch-{_name}-row-{_bs}x4x{_H}x{_W}", NEW, _bs, _H, _W, _nb, _eta, _row))


@pytest.mark.gpu
@pytest.mark.parametrize("declares,bs,H,Wd,nb,eta,row", [c[1:] for c in GUARDED], ids=[c[0] for c in GUARDED])
def test_highorder_tails_write_their_outputs_only(declares, bs, H, Wd, nb, eta, row):
    """All six entry points under tests/guarded.py, both poison patterns: a middle row, the last row and a one-evaluation row of eta 1.5
    (linear multistep: steps `row` and `row` + 3 of a 7-step schedule at order 3, the second of which wraps; the slots a step does not
    read are left POISONED and must still hold the poison).  x, eps, x2, the ring and the outputs live in arena blocks between canaries: no
    guard byte changes; the inputs and tables are unchanged; the results are finite and bit-equal between the poisons.  In two-branch form
    a poisoned third branch sits behind the two."""
    from cd360 import ops
    scale_im = 3.5 if nb == 3 else None
    tab, anc, mid, mult = _tables(eta)
    ltab, lms = _lms_tables(3, 7)
    d = dict(x=R(bs, 4, H, Wd, seed=1), e=R(nb * bs, 4, H, Wd, seed=2), e2=R(nb * bs, 4, H, Wd, seed=3), e16=R(nb * bs, H * Wd, 16, seed=7, dtype=BF),
             e16b=R(nb * bs, H * Wd, 16, seed=8, dtype=BF), hist=R(3, bs, 4, H, Wd, seed=9), tab=tab, anc=anc, mid=mid, mult=mult, ltab=ltab, lms=lms,
             step=step_t(row), step3=step_t(row + 3), seed=seed_t(BIG_SEED), streams=streams_t(list(range(1, bs + 1))))
    tail = bs if nb == 2 else 0

    @SC.guardfn
    def fn(x, e, e2, e16, e16b, hist, tab, anc, mid, mult, ltab, lms, step, step3, seed, streams, guard):
        T = guard.torch

        def arena(src, rows=None, fill=True):
            t = T.empty(((rows or src.shape[0]),) + tuple(src.shape[1:]), dtype=src.dtype, device=DEV)
            if fill:
                t[:src.shape[0]].copy_(src)
            return t

        ge, ge16, ge2, ge16b = (arena(t, nb * bs + tail) for t in (e, e16, e2, e16b))
        gx = arena(x)
        s, a, m, mu = tab[row, 0:1].contiguous(), anc[row].contiguous(), mid[row].contiguous(), mult[row].contiguous()
        # DPM++ 2S: fp32 forms into the binding's arena blocks, staged forms into this case's
        x2 = ops.cfg_dpmpp2s_mid(gx, ge[:nb * bs], s, mu, 7.5, scale_im)
        gx2 = arena(x, fill=False)
        ops.cfg_dpmpp2s_mid_cl(gx, ge16[:nb * bs, :, :4], tab, mult, step, 7.5, scale_im, gx2)
        out = ops.cfg_dpmpp2s_step(gx, x2, ge2[:nb * bs], m, mu, a, seed, streams, step, 7.5, scale_im)
        gxs = arena(x)
        ops.cfg_dpmpp2s_step_cl(gxs, gx2, ge16b[:nb * bs, :, :4], mid, mult, anc, step, seed, streams, 7.5, scale_im)
        # linear multistep at order 3, steps row and row + 3: only the slots a step reads are filled
        res = []
        for i, st in ((row, step), (row + 3, step3)):
            cur = min(i + 1, 3)
            for form in ("f32", "cl"):
                ring = arena(hist, fill=False)
                for j in range(1, cur):
                    ring[(i - j) % 3].copy_(hist[(i - j) % 3])
                if form == "f32":
                    o = ops.cfg_lms_step(gx, ge[:nb * bs], ring, ltab[i, 0:1].contiguous(), lms[i].contiguous(), st, 7.5, scale_im)
                else:
                    o = arena(x)
                    ops.cfg_lms_step_cl(o, ring, ge16[:nb * bs, :, :4], ltab, lms, st, 7.5, scale_im)
                for other in range(3):
                    if other != i % 3 and not 1 <= (i - other) % 3 < cur:
                        assert bool((ring[other].view(torch.uint8) == guard.arena.poison).all()), f"step {i} touched slot {other}"
                    elif other != i % 3:
                        assert torch.equal(ring[other], hist[other]), f"step {i} wrote slot {other}"
                res += [o, ring[i % 3].clone()]
        assert torch.equal(ge[:nb * bs], e) and torch.equal(ge16[:nb * bs], e16) and torch.equal(gx, x), "an input was written"
        return x2, gx2, out, gxs, res

    (x2, gx2, out, gxs, res), _ = G.run_twice(fn, d, declares=declares)
    x, s, a, m, mu = d["x"], tab[row, 0:1], anc[row], mid[row], mult[row]
    e_cl, e2_cl = SC.cl_to_nchw(d["e16"], nb * bs, H, Wd), SC.cl_to_nchw(d["e16b"], nb * bs, H, Wd)
    z = ops.sampler_noise(d["seed"], d["streams"], d["step"], bs, H, Wd)
    assert torch.equal(x2, _mid(x, d["e"], s, mu, 7.5, scale_im)) and torch.equal(gx2, _mid(x, e_cl, s, mu, 7.5, scale_im))
    assert torch.equal(out, _step2s(x, x2, d["e2"], m, mu, a, z, 7.5, scale_im))
    assert torch.equal(gxs, _step2s(x, gx2, e2_cl, m, mu, a, z, 7.5, scale_im))
    k = 0
    for i in (row, row + 3):
        for e_form in (d["e"], e_cl):
            ring = d["hist"].clone()
            want = _lms(x, e_form, ring, ltab[i, 0:1], lms[i], i, 7.5, scale_im)
            assert torch.equal(res[k], want) and torch.equal(res[k + 1], ring[i % 3]), (i, k)
            k += 2


def test_every_highorder_entry_point_has_a_guarded_case():
    """The twin of test_every_edm_entry_point_has_a_guarded_case for include/cd360_highorder.h (runs without a GPU): every `int cd360_...(`
    the header declares is in some guarded case's `declares` in this file, and is typed in HIGHORDER_SIGNATURES."""
    from cd360 import _lib
    untyped, unknown, uncovered = SC.check_guarded_cover("cd360_highorder.h", _lib.HIGHORDER_SIGNATURES, GUARDED)
    assert not untyped, untyped
    assert not unknown, unknown
    assert not uncovered, f"launching entry points without a guarded case: {sorted(uncovered)}"


# ================================================================================================ 10: the GPU trajectories
@pytest.mark.gpu
@torch.no_grad()
@pytest.mark.parametrize("solver,tag", [("2s", "e10"), ("2s", "e06"), ("2s", "e15"), ("lms", 4), ("lms", 3), ("lms", 1)])
@pytest.mark.parametrize("name", ["cfg3", "cfg2"])
def test_fused_steps_on_the_gpu_walk_the_reference_trajectory(name, solver, tag):
    """The product's step functions (cd360.sampler.fused_cfg_dpmpp2s_step / fused_cfg_lms_step, the tails on the `_f32` kernels, the golden's
    stored z handed in as the noise, the linear multistep ring pre-filled with NaN) ON THE GPU over the 12-step trajectories of
    tests/golden/sampler_highorder.npz, written by the REFERENCE's own classes; the bar of the CPU twins."""
    from test_highorder_cpu import golden_key, load, run_product_steps
    g = load()
    got, xs = run_product_steps(g, solver, name, DEV, fused=True, tag=tag)
    assert got.is_cuda
    key = golden_key(solver, name, tag)
    err = float((got.cpu() - g[key]).abs().max())
    print(f"{key}: fused GPU trajectory vs the reference's golden, max abs:", err, "of max", float(g[key].abs().max()))
    assert torch.allclose(got.cpu(), g[key], atol=2e-5, rtol=1e-5), err
    for i in range(12):
        assert torch.allclose(xs[i].cpu(), g[key + "_x"][i], atol=2e-5, rtol=1e-5), i


# ================================================================================================ 11 - 13: the job
JOBS = {"dpmpp2s_a": dict(solver="dpmpp2s_a", eta=1.0), "lms": dict(solver="lms", order=3)}  # order 3: the ring wraps at step 3


def _ho_job(which):
    """SC.walk for a key of JOBS, or for "euler": the plain solver the others are told apart from."""
    return SC.walk(**JOBS.get(which, {}))


@pytest.fixture(scope="module", autouse=True)
def _release_the_shared_job():
    yield
    SC.release()


@pytest.mark.gpu
@torch.no_grad()
@pytest.mark.parametrize("which", list(JOBS))
def test_highorder_job_through_its_captured_graphs(which):
    """Sampler(n_steps=4, use_graph=True) over 3 poses x all 4 steps for DPM++ 2S ancestral (eta 1.0) and the linear multistep solver
    (order 3).  All graphs captured and staged -- DPM++ 2S holds three (steady: two evaluations; render; the one-evaluation sigma_down = 0
    step) and smp.gx2, linear multistep two and the ring smp.gds.  Every pose bit-identical to a fresh graph-mode sampler's (the ring and
    gx2 carry nothing from pose to pose) and to use_graph=False, and a step replayed twice from the same x gives the same bits.  Each
    differs from plain Euler by more than 1e-3 of the maximum."""
    from cd360 import job, solvers
    kw = JOBS[which]
    latents, smp = _ho_job(which)
    assert latents.shape == (POSES, 4, LATENT, LATENT) and torch.isfinite(latents).all()
    assert smp.solver == which and smp._solver is solvers.HIGHORDER_SOLVERS[which] and smp.staged and smp.branches == 3
    assert smp.graph is not None and smp.rgraph is not None
    if which == "dpmpp2s_a":
        assert smp.lgraph is not None and smp.gx2.shape == smp.gx.shape and smp.single_rows == [False, False, False, True]
        for tab in (smp.anc_tab, smp.mid_tab, smp.mult2s_tab):
            assert tab.shape == (STEPS, 4) and tab.dtype == torch.float32 and tab.is_cuda
        assert smp.mid_temb.shape == smp.temb_tab.shape and smp.seed_buf.tolist() == [SEED] and smp.streams_buf.tolist() == [0]
    else:
        assert smp.lgraph is None and smp.gds.shape == (3,) + tuple(smp.gx.shape) and smp.lms_tab.shape == (STEPS, 4) and smp.order == 3
        assert bool((smp.lms_tab[3, :3] != 0).all()) and float(smp.lms_tab[3, 3]) == 0.0
    for p in range(POSES):
        pose, ctx, y, x0 = SC.job(p)
        fresh = job.sample_assigned(SC.sampler(pose, ctx, y, **kw), [(pose, ctx, y, x0)], STEPS)[0]
        assert torch.equal(fresh, latents[p:p + 1]), (p, float((fresh - latents[p:p + 1]).abs().max()))
        eager = job.sample_assigned(SC.sampler(pose, ctx, y, use_graph=False, **kw), [(pose, ctx, y, x0)], STEPS)[0]
        assert torch.equal(eager, latents[p:p + 1]), (p, float((eager - latents[p:p + 1]).abs().max()))
    pose, ctx, y, x0 = SC.job(0)
    smp.retarget(pose, ctx, y)
    x1 = smp.step(x0.clone(), 0)
    for i in (1, 2, 3):  # step i twice from the same x: the same bits (the ring's slot i % order is rewritten with the same direction)
        a, b = smp.step(x1, i), smp.step(x1, i)
        assert torch.equal(a, b) and not torch.equal(a, x1), i
    assert torch.equal(smp.step(x0.clone(), 0), x1)
    eul, esmp = _ho_job("euler")
    assert esmp._solver is solvers.SOLVERS["euler"] and esmp.lgraph is None
    for p in range(POSES):
        d = float((eul[p] - latents[p]).abs().max() / latents[p].abs().max())
        print(f"{which} pose {p}: vs plain Euler, 4 steps: rel", d)
        assert d > 1e-3, (p, d)


@pytest.mark.gpu
@torch.no_grad()
def test_one_step_dpmpp2s_is_one_step_euler_ancestral():
    """n_steps = 1: the only step is the sigma_down = 0 row, DPM++ 2S takes one evaluation and must hold the ancestral Euler step's bits at
    the same seed and eta -- graph mode (this step is launched un-captured) and eager."""
    pose, ctx, y, x0 = SC.job(0)
    for use_graph in (True, False):
        s2 = SC.sampler(pose, ctx, y, n_steps=1, solver="dpmpp2s_a", eta=1.0, use_graph=use_graph)
        ea = SC.sampler(pose, ctx, y, n_steps=1, solver="euler_a", eta=1.0, use_graph=use_graph)
        a, b = s2.step(x0.clone(), 0), ea.step(x0.clone(), 0)
        assert torch.isfinite(a).all() and torch.equal(a, b), float((a - b).abs().max())
        assert s2.single_rows == [True] and s2.graph is None and torch.equal(s2.anc_tab, ea.anc_tab)


@pytest.mark.gpu
@torch.no_grad()
def test_interior_single_rows_run_on_the_one_evaluation_graph():
    """eta = 1.5, n_steps = 12: rows 0-4 and 8-11 take one evaluation (sigma_up is clamped to sigma_next there), rows 5-7 two.  One pose
    through the captured sampler -- row 0 renders un-captured, the other single rows replay the one-evaluation graph -- equals the eager
    run bit for bit, and is finite."""
    from cd360 import job
    pose, ctx, y, x0 = SC.job(0)
    g_smp = SC.sampler(pose, ctx, y, n_steps=12, solver="dpmpp2s_a", eta=1.5)
    got = job.sample_assigned(g_smp, [(pose, ctx, y, x0)], 12)[0]
    assert g_smp.single_rows == [i in (0, 1, 2, 3, 4, 8, 9, 10, 11) for i in range(12)]
    assert g_smp.graph is not None and g_smp.lgraph is not None and g_smp.rgraph is None and torch.isfinite(got).all()
    eager = job.sample_assigned(SC.sampler(pose, ctx, y, n_steps=12, solver="dpmpp2s_a", eta=1.5, use_graph=False), [(pose, ctx, y, x0)], 12)[0]
    assert torch.equal(got, eager), float((got - eager).abs().max())


@pytest.mark.gpu
@torch.no_grad()
def test_captured_dpmpp2s_follows_seed_and_streams():
    """From ONE snapshot of gx, step 1 replayed under seed A and under seed B (reseed: no re-capture) differs, and restoring the seed
    restores the bits; set_noise_streams changes the result and restoring it restores the bits.  On the last step (sigma_up = 0) the two
    seeds give bit-equal x.  (The difference term itself is held at the kernel level, test_dpmpp2s_step_adds_the_documented_noise.)"""
    _, smp = _ho_job("dpmpp2s_a")
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
    last = {}
    for seed in (SEED + 1, SEED):  # (ends on the fixture's seed)
        smp.reseed(seed)
        last[seed] = smp.step(snap, STEPS - 1)
    assert torch.equal(last[SEED], last[SEED + 1]) and smp.graph is graph
    assert torch.equal(smp.step(snap, 1), res[SEED])


@pytest.mark.gpu
@torch.no_grad()
def test_unstaged_route_serves_both_solvers():
    """With routes.no_stage the un-staged route carries both: finite, graph mode equal to its own eager run, and not the Euler result."""
    from cd360 import job, routes
    pose, ctx, y, x0 = SC.job(0)
    with routes.override(no_stage=True):
        u_eul = job.sample_assigned(SC.sampler(pose, ctx, y, use_graph=False, solver="euler"), [(pose, ctx, y, x0)], STEPS)[0]
        for which in JOBS:
            g_smp = SC.sampler(pose, ctx, y, **JOBS[which])
            e_smp = SC.sampler(pose, ctx, y, use_graph=False, **JOBS[which])
            assert not g_smp.staged and not e_smp.staged
            got_g = job.sample_assigned(g_smp, [(pose, ctx, y, x0)], STEPS)[0]
            got_e = job.sample_assigned(e_smp, [(pose, ctx, y, x0)], STEPS)[0]
            assert g_smp.graph is not None and torch.isfinite(got_g).all()
            assert torch.equal(got_g, got_e), (which, float((got_g - got_e).abs().max()))
            assert float((got_g - u_eul).abs().max() / u_eul.abs().max()) > 1e-3, which


def module_route(net, which, nb, pose, ctx, y, x0, steps=STEPS):
    """SC.module_route under this file's class for JOBS[which]."""
    from cd360 import sampler as S
    kw = dict(JOBS[which])
    kw.pop("solver")
    if which == "dpmpp2s_a":
        mod = S.DPMPP2SAncestralSampler(num_steps=steps, guider_config=SC.guider_config(nb), device=DEV, seed=SEED, **kw)
    else:
        mod = S.LinearMultistepSampler(num_steps=steps, guider_config=SC.guider_config(nb), device=DEV, **kw)
    return SC.module_route(net, mod, which, nb, pose, ctx, y, x0, steps, order=kw.get("order"))


@pytest.mark.gpu
@torch.no_grad()
@pytest.mark.parametrize("which", list(JOBS))
@pytest.mark.parametrize("nb", [3, 2])
def test_highorder_job_agrees_with_the_uncaptured_module_route(nb, which):
    """Whole trajectory, n_steps = 4, all 4 steps, the same seed: the same UNet under cd360.sampler.DPMPP2SAncestralSampler(seed=...) /
    LinearMultistepSampler + the guider + DiscreteDenoiser (the YAML's classes, eager, the implicit-GEMM input convolution) against the job
    sampler (captured, staged, the tables).  Both routes draw the same noise (one draw per step: the class's step word is the step index,
    like the kernels'), so they differ as under plain Euler -- by the staged input convolution rounding a few bf16 values to the other
    neighbour, amplified by 70 random-init blocks.
    Bar: what the SAME comparison gives under plain EULER on the parent commit at the same branch count, measured on the same box in the
    same session (tools/solver_report.py), times 2 for the linear multistep solver (one evaluation per step, as DPM++ 2M is granted) and
    times 4 for DPM++ 2S (two evaluations per step, as Heun is granted).  Measured figures: DESIGN.md section 6.4."""
    from cd360 import job
    net = SC.net()
    pose, ctx, y, x0 = SC.job(0, nb)
    got = job.sample_assigned(SC.sampler(pose, ctx, y, scale_im=3.5 if nb == 3 else 0, **JOBS[which]), [(pose, ctx, y, x0)], STEPS)[0]
    x = module_route(net, which, nb, pose, ctx, y, x0)
    dev = float((got - x).abs().max() / x.abs().max())
    bar = BAR_FACTOR[which] * PARENT_EULER_JOB_VS_MODULE_REL[nb]
    print(f"{which} {nb}-branch job vs module route, 4 steps: max abs", float((got - x).abs().max()), "rel", dev, "| bar", bar)
    assert torch.isfinite(got).all() and dev <= bar, (dev, bar)
