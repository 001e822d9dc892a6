"""Masked and image-to-image sampling on the GPU: the domain-3 noise kernel against the float64 restatement, the blend kernel bit for bit
against cd360.sampler.masked_blend, both under the guarded allocator, the blend inside the captured step of every solver, the partial
start and the job down to images.  Needs an MI355X; the job tests run on the tiny job of sampler_cases."""
import numpy as np
import pytest
import torch

import edit_cases as EC
import guarded as G
import philox_ref as P
import sampler_cases as SC
from sampler_cases import DEV, LATENT, POSES, SEED, STEPS, R, seed_t, step_t, streams_t

BIG_SEED = 2 ** 63 + 12345
SHAPES = [(1, 5, 7), (3, 5, 7), (1, 1, 257), (3, 1, 257)]  # HW = 35 and 257: odd, no multiple of a wave; 257 takes two workgroups


# ================================================================================================ 1: the noise kernel
@pytest.mark.gpu
@pytest.mark.parametrize("bs,H,Wd", SHAPES)
def test_edit_noise_equals_the_float64_restatement(bs, H, Wd):
    """cd360_edit_noise_f32 against image_cases.normals(..., domain 3) in float64.  Bar, as tests/test_euler_a_gpu.py holds
    cd360_sampler_noise_f32 to: 4 x what the SAME expression evaluated in float32 by numpy gives against float64 on the same inputs (a few
    ulp between the device's and the host's logf / sinf / cosf at radius <= 5.8).  Rows of equal stream id are bit-equal, rows of
    different ids differ, a row does not depend on bs or on its position, and the draw is not domain 0's."""
    from cd360 import ops
    hw = H * Wd
    for seed in (0, BIG_SEED):
        for step in (0, 3):
            for ids in (None, list(range(bs)), [5] * bs):
                got = ops.edit_noise(seed_t(seed), streams_t(ids), step_t(step), bs, H, Wd)
                assert got.shape == (bs, 4, H, Wd) and got.dtype == torch.float32
                rows = [0] * bs if ids is None else ids
                want = EC.batch(seed, rows, step, hw)
                bar = 4 * float(np.abs(EC.batch(seed, rows, step, hw, np.float32) - want).max())
                err = float(np.abs(got.cpu().numpy().reshape(bs, 4, hw).astype(np.float64) - want).max())
                print(f"edit noise {bs}x4x{H}x{Wd} seed {seed} step {step} streams {ids}: max |kernel - float64| {err:.3e} | bar {bar:.3e}")
                assert err <= bar, (seed, step, ids, err, bar)
                assert not torch.equal(got, ops.sampler_noise(seed_t(seed), streams_t(ids), step_t(step), bs, H, Wd))
                if bs == 3:
                    assert torch.equal(got[0], got[2]) == (rows[0] == rows[2]) and torch.equal(got[0], got[1]) == (rows[0] == rows[1])
                    for r in (0, 2):  # the matching row of bs = 1, and of the reversed batch
                        one = ops.edit_noise(seed_t(seed), streams_t([rows[r]]), step_t(step), 1, H, Wd)
                        assert torch.equal(one[0], got[r]), (seed, step, ids, r)
                    rev = ops.edit_noise(seed_t(seed), streams_t(rows[::-1]), step_t(step), bs, H, Wd)
                    assert torch.equal(rev[0], got[2]) and torch.equal(rev[2], got[0])


# ================================================================================================ 2: the blend, bit for bit
def _table():
    """A 4-step schedule's step table: column 1 = sigma_next, row 3 the sigma_next = 0 row."""
    from cd360 import sampler as S
    sig = S.LegacyDDPMDiscretization()(4)
    return torch.stack([sig[:-1], sig[1:], torch.ones(4), torch.zeros(4)], 1).contiguous().to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ["one-row", "bs-rows"])
@pytest.mark.parametrize("bs,H,Wd", SHAPES)
def test_mask_blend_equals_masked_blend_bit_for_bit(bs, H, Wd, rows):
    """cd360_mask_blend_f32 == cd360.sampler.masked_blend(x, known, m, s', ops.edit_noise(...)) under torch.equal for a fractional mask, on
    a noisy row and on the s' = 0 row; m = 1 returns x, m = 0 returns kn, s' = 0 returns m x + (1 - m) known with NaN-free bits whatever
    the seed; known, mask and the table are unchanged; the stride-4 form (the table) and the stride-0 form (a device scalar) agree; a
    tensor that wants a gradient is refused."""
    from cd360 import ops
    from cd360.sampler import masked_blend
    mr = 1 if rows == "one-row" else bs
    x, known = R(bs, 4, H, Wd, seed=1), R(bs, 4, H, Wd, seed=2)
    m = torch.rand(mr, 1, H, Wd, generator=torch.Generator(device=DEV).manual_seed(3), device=DEV)
    m[..., 0] = 1.0
    m[..., -1] = 0.0
    tab, seed, ids = _table(), seed_t(BIG_SEED), streams_t(list(range(bs)))
    keep = [t.clone() for t in (known, m, tab)]
    for row in (2, 3, 0):
        s = tab[row, 1:2].clone()
        z = ops.edit_noise(seed, ids, step_t(row), bs, H, Wd)
        want = masked_blend(x, known, m, s, z)
        got = ops.mask_blend(x.clone(), known, m, tab, step_t(row), seed, ids)
        assert torch.equal(got, want), (row, float((got - want).abs().max()))
        assert torch.equal(ops.mask_blend(x.clone(), known, m, s, step_t(row), seed, ids), got), row  # stride 0
        assert torch.equal(ops.mask_blend(x.clone(), known, torch.ones_like(m), tab, step_t(row), seed, ids), x)
        kn = ops.mask_blend(x.clone(), known, torch.zeros_like(m), tab, step_t(row), seed, ids)
        assert torch.equal(kn, known if row == 3 else known + z * s), row
        if row == 3:
            assert float(s) == 0.0 and torch.equal(got, m * x + (1.0 - m) * known)
            assert torch.equal(ops.mask_blend(x.clone(), known, m, tab, step_t(row), seed_t(1), None), got)  # no noise term
        else:
            assert not torch.equal(ops.mask_blend(x.clone(), known, m, tab, step_t(row), seed_t(1), ids), got)
            if bs == 3:  # streams null = stream 0 for every row
                null = ops.mask_blend(x.clone(), known, m, tab, step_t(row), seed, None)
                assert torch.equal(null, ops.mask_blend(x.clone(), known, m, tab, step_t(row), seed, streams_t([0] * bs)))
                assert torch.equal(null[0], got[0]) and not torch.equal(null[1], got[1])
    for t, k in zip((known, m, tab), keep):
        assert torch.equal(t, k)
    with pytest.raises(NotImplementedError), torch.enable_grad():
        ops.mask_blend(x.clone().requires_grad_(True), known, m, tab, step_t(0), seed, ids)


# ================================================================================================ 3: guarded runs
GUARDED = [(f"{rows}-mask-rows-{name}-row-3x4x5x7", EC.NEW, rows, row) for rows in (1, 3) for name, row in (("middle", 2), ("last", 3))]


@pytest.mark.gpu
@pytest.mark.parametrize("declares,mask_rows,row", [c[1:] for c in GUARDED], ids=[c[0] for c in GUARDED])
def test_edit_entry_points_write_their_outputs_only(declares, mask_rows, row):
    """Both entry points under tests/guarded.py at HW = 35, bs = 3, both poison patterns: x, known and the mask live in arena blocks between
    canaries, so no guard byte changes; the results are finite and bit-equal between the poisons; the operands are unchanged; both entry
    points ran."""
    from cd360 import _edit, ops
    bs, H, Wd = 3, 5, 7
    inputs = dict(x=R(bs, 4, H, Wd, seed=4), known=R(bs, 4, H, Wd, seed=5), mask=torch.rand(mask_rows, 1, H, Wd, device=DEV), tab=_table(),
                  step=step_t(row), seed=seed_t(BIG_SEED), streams=streams_t([0, 3, 0]))

    @SC.guardfn
    def fn(x, known, mask, tab, step, seed, streams, guard):
        T = guard.torch
        gx, gk, gm = (T.empty(tuple(t.shape), dtype=t.dtype, device=DEV) for t in (x, known, mask))
        for g, t in ((gx, x), (gk, known), (gm, mask)):
            g.copy_(t)
        with G.recorded(guard, _edit):
            z = ops.edit_noise(seed, streams, step, bs, H, Wd)
            out = ops.mask_blend(gx, gk, gm, tab, step, seed, streams)
        assert out is gx and torch.equal(gk, known) and torch.equal(gm, mask)
        return z, out

    (z, out), _ = G.run_twice(fn, inputs, declares=declares)
    from cd360.sampler import masked_blend
    assert torch.equal(out, masked_blend(inputs["x"], inputs["known"], inputs["mask"], inputs["tab"][row, 1:2], z))


def test_every_edit_entry_point_has_a_guarded_case():
    """Runs without a GPU: every `int cd360_...(` include/edit/cd360_edit.h declares is in a guarded case's `declares` above, and is typed in
    EDIT_SIGNATURES."""
    from cd360 import _edit
    untyped, unknown, uncovered = SC.check_guarded_cover(EC.HEADER, _edit.EDIT_SIGNATURES, GUARDED)
    assert not untyped, untyped
    assert not unknown, unknown
    assert not uncovered, f"launching entry points without a guarded case: {sorted(uncovered)}"


# ================================================================================================ 4: every solver's captured step
@pytest.fixture(scope="module", autouse=True)
def _release_the_shared_job():
    yield
    SC.release()


def _karras():
    from cd360 import sampler as S
    return S.EDMDiscretization(sigma_min=0.0292, sigma_max=14.6146, rho=3.0)  # inside the denoiser's table, every sigma off its grid


CASES = {"euler": (3, dict(solver="euler")), "euler-cfg2": (2, dict(solver="euler", scale_im=None)), "euler-karras": (3, dict(solver="euler")),
         "dpmpp2m": (3, dict(solver="dpmpp2m")), "euler_a": (3, dict(solver="euler_a")), "heun": (3, dict(solver="heun")),
         "dpmpp2s_a": (3, dict(solver="dpmpp2s_a")), "lms": (3, dict(solver="lms"))}
DETERMINISTIC = ("euler", "euler-cfg2", "euler-karras", "dpmpp2m", "heun", "lms")
TOP = LATENT // 2 - 1  # rows 0 .. TOP - 1 are kept, two fractional rows follow, the rest is generated


def _known(seed=21):
    return R(1, 4, LATENT, LATENT, seed=seed) * 0.8


def _half_mask():
    m = torch.ones(1, 1, LATENT, LATENT, device=DEV)
    m[..., :TOP, :] = 0.0
    m[..., TOP, :], m[..., TOP + 1, :] = 0.25, 0.75
    return m


def _walk(smp, x0, first_step=0):
    x, xs = x0.clone(), []
    for i in range(first_step, STEPS):
        x = smp.step(x, i, first=i == first_step)
        xs.append(x)
    return xs


@pytest.mark.gpu
@torch.no_grad()
@pytest.mark.parametrize("case", list(CASES))
def test_masked_step_of_every_solver(case):
    """Sampler(known=, mask=) on the tiny job, 4 steps.  A mask of ones gives the unmasked sampler's latents bit for bit, step by step.
    With a half mask (set_known on the SAME captured sampler: the graph objects stay) graph, eager and a fresh graph-mode sampler are
    bit-equal step by step, the final latent equals `known` exactly where the mask is 0 (the last sigma_next is 0) and differs from it
    where the mask is 1; set_known with another picture changes the result and nothing is re-captured.  A masked sampler owns the seed
    buffer under a deterministic solver too (reseed moves an intermediate latent); an unmasked one keeps refusing reseed."""
    nb, kw = CASES[case]
    if case == "euler-karras":
        kw = dict(kw, discretization=_karras())
    pose, ctx, y, x0 = SC.job(0, nb)
    known, ones, half = _known(), torch.ones(1, 1, LATENT, LATENT, device=DEV), _half_mask()
    plain = SC.sampler(pose, ctx, y, use_graph=False, **kw)
    xs_plain = _walk(plain, x0)
    assert not plain.masked and plain.known_buf is None
    if case in DETERMINISTIC:
        assert getattr(plain, "seed_buf", None) is None
        with pytest.raises(ValueError):
            plain.reseed(SEED + 1)
        with pytest.raises(ValueError):
            plain.set_noise_streams([1])
    with pytest.raises(ValueError):
        plain.set_known(known, half)
    g = SC.sampler(pose, ctx, y, known=known, mask=ones, **kw)
    xs_ones = _walk(g, x0)
    for i in range(STEPS):
        assert torch.equal(xs_ones[i], xs_plain[i]), (i, float((xs_ones[i] - xs_plain[i]).abs().max()))
    graphs = (g.graph, g.lgraph, g.rgraph)
    assert g.masked and g.staged and g.graph is not None and g.seed_buf.tolist() == [SEED] and g.streams_buf.tolist() == [0]
    assert g.rgraph is not None and g.known_buf.shape == x0.shape and g.mask_buf.shape == (1, 1, LATENT, LATENT)
    g.set_known(known, half)
    xs_half = _walk(g, x0)
    e = SC.sampler(pose, ctx, y, use_graph=False, known=known, mask=half, **kw)
    xs_eager = _walk(e, x0)
    f = SC.sampler(pose, ctx, y, known=known, mask=half, **kw)
    xs_fresh = _walk(f, x0)
    for i in range(STEPS):
        assert torch.equal(xs_half[i], xs_eager[i]), (i, float((xs_half[i] - xs_eager[i]).abs().max()))
        assert torch.equal(xs_half[i], xs_fresh[i]), (i, float((xs_half[i] - xs_fresh[i]).abs().max()))
    final = xs_half[-1]
    assert torch.isfinite(final).all() and torch.equal(final[..., :TOP, :], known[..., :TOP, :])
    inside = final[..., TOP + 2:, :]
    assert not torch.equal(inside, known[..., TOP + 2:, :]) and float((inside - known[..., TOP + 2:, :]).abs().max()) > 1e-3
    assert not torch.equal(xs_half[0][..., :TOP, :], known[..., :TOP, :])  # before the last row the kept region is known + sigma_next z
    other = _known(seed=22)
    g.set_known(other, half)
    xs_other = _walk(g, x0)
    assert torch.equal(xs_other[-1][..., :TOP, :], other[..., :TOP, :]) and not torch.equal(xs_other[-1], final)
    g.set_known(known, half)
    g.reseed(SEED + 1)
    moved = g.step(x0.clone(), 0)
    g.reseed(SEED)
    assert not torch.equal(moved[..., :TOP, :], xs_half[0][..., :TOP, :]) and torch.equal(g.step(x0.clone(), 0), xs_half[0])
    assert (g.graph, g.lgraph, g.rgraph) == graphs and all(a is b for a, b in zip((g.graph, g.lgraph, g.rgraph), graphs))
    with pytest.raises(ValueError):
        g.set_known(known, None)
    with pytest.raises(ValueError):
        g.set_known(known[..., :8], half[..., :8])


@pytest.mark.gpu
@torch.no_grad()
def test_unstaged_route_serves_the_masked_step():
    """With routes.no_stage the blend reads the schedule's own sigma_next as a device scalar (stride 0) and the step index the sampler
    itself advances: graph mode equals its own eager run, the kept region ends as `known`, and a mask of ones is the unmasked run."""
    from cd360 import routes
    pose, ctx, y, x0 = SC.job(0)
    known, half = _known(), _half_mask()
    with routes.override(no_stage=True):
        for solver in ("euler", "euler_a"):
            plain = _walk(SC.sampler(pose, ctx, y, use_graph=False, solver=solver), x0)
            ones = SC.sampler(pose, ctx, y, use_graph=False, solver=solver, known=known, mask=torch.ones_like(half))
            assert not ones.staged and torch.equal(_walk(ones, x0)[-1], plain[-1])
            g_smp = SC.sampler(pose, ctx, y, solver=solver, known=known, mask=half)
            e_smp = SC.sampler(pose, ctx, y, use_graph=False, solver=solver, known=known, mask=half)
            got_g, got_e = _walk(g_smp, x0), _walk(e_smp, x0)
            assert not g_smp.staged and g_smp.graph is not None
            for i in range(STEPS):
                assert torch.equal(got_g[i], got_e[i]), (solver, i)
            assert torch.equal(got_g[-1][..., :TOP, :], known[..., :TOP, :]) and not torch.equal(got_g[-1], plain[-1])


# ================================================================================================ 5: the partial start
@pytest.mark.gpu
@torch.no_grad()
@pytest.mark.parametrize("solver", ["euler", "heun", "euler_a", "dpmpp2s_a"])
def test_partial_start_runs_the_tail_of_the_schedule(solver):
    """A full trajectory with the mask 0 everywhere holds, after step k - 1, exactly start_from(sampler, known, k, seed).  Rows k .. n - 1
    run from that latent with step(., k, first=True), unmasked, in graph mode are bit-equal to the same rows launched eagerly (k = 2: a
    row of the captured shape, through the render graph; k = 3: the one-evaluation last row of the two-evaluation solvers).  The render
    runs on row k and on no later row: the first pose block's cached render is refreshed for another pose there, and stays."""
    from cd360 import job as J
    from cd360 import sampling
    pose, ctx, y, x0 = SC.job(0)
    known = _known()
    kept = SC.sampler(pose, ctx, y, solver=solver, known=known, mask=torch.zeros(1, 1, LATENT, LATENT, device=DEV))
    xs_kept = _walk(kept, x0)
    assert torch.equal(xs_kept[-1], known)
    u = SC.sampler(pose, ctx, y, solver=solver)
    v = SC.sampler(pose, ctx, y, solver=solver, use_graph=False)
    blk = sampling.pose_blocks(SC.net())[0][1]
    for k in (2, 3):
        start = J.start_from(kept, known, k, SEED)
        assert torch.equal(xs_kept[k - 1], start), (k, float((xs_kept[k - 1] - start).abs().max()))
        assert torch.equal(J.start_from(u, known, k, SEED, streams=[0]), start) and not torch.equal(J.start_from(u, known, k, SEED + 1), start)
        assert float((start - known).std() / kept.sigmas[k]) == pytest.approx(1.0, abs=0.05)
        got = _walk(u, start, first_step=k)
        assert len(got) == STEPS - k
        want = _walk(v, start, first_step=k)
        for a, b in zip(got, want):
            assert torch.isfinite(a).all() and torch.equal(a, b), (k, float((a - b).abs().max()))
    assert u.graph is not None and u.rgraph is not None
    # another pose: the render of row 2 refreshes the cached render, row 3 leaves it
    pose1, ctx1, y1, _ = SC.job(1)
    start = J.start_from(u, known, 2, SEED)
    u.retarget(pose, ctx, y)
    x = u.step(start, 2, first=True)
    r0 = blk.rendered_feat.clone()
    u.retarget(pose1, ctx1, y1)
    x = u.step(start, 2, first=True)
    r1 = blk.rendered_feat.clone()
    assert not torch.equal(r1, r0)
    u.step(x, 3)
    assert torch.equal(blk.rendered_feat, r1)
    u.retarget(pose, ctx, y)
    u.step(x, 3)  # (not first: the render of pose 1 stays)
    assert torch.equal(blk.rendered_feat, r1)
    for bad in ("dpmpp2m", "lms"):
        with pytest.raises(ValueError):
            SC.sampler(pose, ctx, y, solver=bad, use_graph=False).step(start, 2, first=True)


# ================================================================================================ 6: down to images
@pytest.mark.gpu
@torch.no_grad()
def test_sample_images_keeps_and_starts_from_given_latents():
    """sample_images(init_latents=, masks=, first_step=) on one rank, the narrow first stage of tests/test_images_gpu.py: uint8 images of
    the right shape; with masks of zeros they are exactly first_stage.decode_u8(init_latents), pose by pose; with a half mask they are
    not, and a whole-schedule masked run from the start latent differs from the partial one."""
    from cd360 import job as J
    from test_images_gpu import _first_stage
    fs, _ = _first_stage()
    init = torch.cat([_known(seed=30 + p) for p in range(POSES)])
    half = _half_mask()
    held = {}

    def make_sampler(pose, ctx, y):
        if "smp" not in held:
            held["smp"] = SC.sampler(pose, ctx, y, known=init[:1], mask=half)
        else:
            held["smp"].retarget(pose, ctx, y)
        return held["smp"]

    no_x0 = lambda p: SC.job(p)[:3] + (None,)  # noqa: E731
    shape = (POSES, 4 * LATENT, 4 * LATENT, 3)
    kept, mine = J.sample_images(make_sampler, no_x0, POSES, STEPS, fs, seed=SEED, first_step=2, init_latents=init, masks=torch.zeros_like(half))
    assert mine == list(range(POSES)) and kept.shape == shape and kept.dtype == torch.uint8
    assert torch.equal(kept, fs.decode_u8(init)) and not torch.equal(kept[0], kept[1])
    part, _ = J.sample_images(make_sampler, no_x0, POSES, STEPS, fs, seed=SEED, first_step=2, init_latents=init, masks=half)
    assert part.shape == shape and part.dtype == torch.uint8 and not torch.equal(part, kept)
    whole, _ = J.sample_images(make_sampler, no_x0, POSES, STEPS, fs, seed=SEED, latent_hw=(LATENT, LATENT), init_latents=init, masks=half)
    assert whole.shape == shape and not torch.equal(whole, part)
    rows = 4 * TOP - 8  # image rows well inside the kept region (the decoder's receptive field reaches across the border)
    assert float((whole[:, :rows].float() - kept[:, :rows].float()).abs().mean()) < float((whole[:, -rows:].float() - kept[:, -rows:].float()).abs().mean())
