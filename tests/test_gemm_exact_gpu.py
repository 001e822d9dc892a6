"""Every tiling of the MFMA GEMM core, the TN GEMM and the low-rank add on exact-integer inputs, bit for bit against float64 (`-m gpu`).

The cases of tests/gemm_cases.py: small-integer operands, so every product and every partial sum is an integer below 2^24 and the fp32
accumulator is exact on any schedule; the one rounding left, fp32 -> bf16 to nearest even, has a single right answer.  The assertions
are torch.equal -- one lost, doubled or misplaced product, truncation, or a second rounding in front of the residual changes bits
(tests/test_gemm_cases_cpu.py holds every case to that).  Launches are repeated and must agree; strided runs put the operands, the
residual and the output inside wider tensors whose padding holds 32768 and must neither leak into a result nor be written.

The one place without bit equality is the GEGLU epilogue (an erf approximation): there every element must lie between
bf16(want - delta) and bf16(want + delta), delta = c |v| max(|g|, 1) with c = 3.13e-7 derived in gemm_cases.GEGLU_C, want = v gelu(g)
in float64 on exact integer pre-activations (measured on an MI355X: 0.034 of delta at the worst, see test_geglu_pairs_values_with_gates)."""
import pytest
import torch

import gemm_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
PAD = 32768.0
CFG_BN = {1: 128, 2: 128, 3: 256, 4: 128, 5: 128, 6: 192, 7: 256, 8: 128, 9: 256}  # columns per tile of gemm_cfg (gemm8p.hip)


def widen(t):
    """t [R, C] -> (wide, view): the same values as a column slice of a wider tensor filled with PAD (row stride C + 24, 16-byte aligned)."""
    R, C = t.shape
    wide = torch.full((R, C + 24), PAD, dtype=t.dtype, device=t.device)
    wide[:, 8:8 + C] = t
    return wide, wide[:, 8:8 + C]


def padding_intact(wide, C):
    return bool((wide[:, :8] == PAD).all()) and bool((wide[:, 8 + C:] == PAD).all())


def describe(got, want):
    """Where and by how much two tensors differ (for the assertion message: the cause is to be found from one run)."""
    g, w = got.double().cpu(), want.double().cpu()
    ne = (g != w).nonzero()
    first = [(tuple(i.tolist()), g[tuple(i)].item(), w[tuple(i)].item()) for i in ne[:4]]
    rows, cols = sorted(set(ne[:, 0].tolist())), sorted(set(ne[:, 1].tolist())) if ne.shape[1] > 1 else []
    return (f"{ne.shape[0]} of {g.numel()} differ, max |d| {(g - w).abs().max().item():g}, rows {rows[:3]}..{rows[-1:]}, "
            f"cols {cols[:3]}..{cols[-1:]}, first (index, got, want) {first}")


_LINEAR = {}  # the small cases stay on the device for the routes that follow; the two multi-million-output ones are rebuilt per test


def linear_on_device(M, N, K, family="main"):
    key = (family, M, N, K)
    if (M, N, K) in G.BIG_SHAPES:
        _LINEAR.pop(key, None)
    if key not in _LINEAR:
        c = G.linear_case(M, N, K, family)
        d = dict(a=c.a.to(DEV, BF), w=c.w.to(DEV, BF), bias=c.bias.to(DEV, torch.float32), res=c.res.to(DEV, BF))
        for k in ("a", "w", "res"):
            d[k + "_wide"], d[k + "_s"] = widen(d[k])
        d["want"] = {e: c.want(e).to(DEV) for e in G.EPILOGUES}
        if (M, N, K) in G.BIG_SHAPES:
            return d
        _LINEAR[key] = d
    return _LINEAR[key]


def launch_linear(ops, d, epilogue, strided, N):
    kw = {}
    if epilogue != "none":
        kw["bias"] = d["bias"]
    if epilogue in ("bias_res", "bias_res_stats"):
        kw["res"] = d["res_s"] if strided else d["res"]
    if epilogue == "bias_res_stats":
        kw["want_stats"] = True
    wide = None
    if strided:
        wide, kw["out"] = widen(torch.zeros(d["a"].shape[0], N, dtype=BF, device=DEV))
    o = ops.gemm(d["a_s"] if strided else d["a"], d["w_s"] if strided else d["w"], **kw)
    out, stats = o if isinstance(o, tuple) else (o, None)
    return out, stats, wide


def run_linear_cases(ops, cases, epilogues, family="main"):
    bad = []
    for M, N, K in cases:
        d = linear_on_device(M, N, K, family)
        tile_n = ops.gemm_tile_n(M, N)
        for e in epilogues:
            want = d["want"][e]
            for strided in (False, True):
                tag = f"{family} {M}x{N}x{K} {e}{' strided' if strided else ''}"
                out, stats, wide = launch_linear(ops, d, e, strided, N)
                out2, stats2, _ = launch_linear(ops, d, e, strided, N)
                if not torch.equal(out, want):
                    bad.append(f"{tag}: {describe(out, want)}")
                if not torch.equal(out, out2) or (stats is not None and not torch.equal(stats, stats2)):
                    bad.append(f"{tag}: repeated launches differ")
                if strided and not (padding_intact(wide, N) and padding_intact(d["a_wide"], K) and padding_intact(d["res_wide"], N)):
                    bad.append(f"{tag}: padding written")
                if stats is not None and family == "stats":
                    ws = G.row_stats(want, tile_n).float()
                    if stats.shape != ws.shape:
                        bad.append(f"{tag}: stats_out shape {tuple(stats.shape)}, want {tuple(ws.shape)} (tile_n {tile_n})")
                    elif not torch.equal(stats, ws):
                        bad.append(f"{tag}: stats_out (tile_n {tile_n}) {describe(stats.reshape(M, -1), ws.reshape(M, -1))}")
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:12])


def set_route(tune, ops, fields):
    tune(**fields)
    cfg = fields.get("gemm_cfg", -1)
    if cfg >= 1:
        assert ops.gemm_tile_n(300, 272) == CFG_BN[cfg]  # the forced tiling is the one the launch takes


@pytest.mark.parametrize("route", G.GEMM_ROUTES, ids=[r[0] for r in G.GEMM_ROUTES])
def test_gemm_bit_equal_on_every_route(tune, route):
    """cd360_gemm_bf16 under every forced tiling (cfg 9 = the generated four-wave loop), k-step mode and mover setting, and the default dispatch:
    one row to ragged multi-tile shapes, one to twelve K-tiles, no epilogue / bias / bias + residual / + row statistics, contiguous and
    strided -- bit-equal to RNE(float64)."""
    from cd360 import ops
    set_route(tune, ops, route[1])
    run_linear_cases(ops, [(M, N, 64 * t) for M, N in G.GEMM_SHAPES for t in G.K_TILES], G.EPILOGUES)


@pytest.mark.parametrize("route", G.GEMM_ROUTES_LONG, ids=[r[0] for r in G.GEMM_ROUTES_LONG])
def test_gemm_bit_equal_on_long_k_loops(tune, route):
    """K = 1280, 3072 (where the k-step groups switch on by default) and 5120."""
    from cd360 import ops
    set_route(tune, ops, route[1])
    run_linear_cases(ops, [(M, N, 64 * t) for M, N in G.GEMM_SHAPES for t in G.K_TILES_LONG], G.EPILOGUES)


@pytest.mark.parametrize("route", G.GEMM_ROUTES, ids=[r[0] for r in G.GEMM_ROUTES])
def test_gemm_row_statistics_bit_equal(tune, route):
    """stats_out = per-row, per-N-tile (sum, sum of squares) of the STORED outputs: on the stats family (sums below 2^24, part of the
    outputs rounds) bit-equal to the float64 sums, on every route."""
    from cd360 import ops
    set_route(tune, ops, route[1])
    run_linear_cases(ops, [(M, N, 64 * t) for M, N in G.GEMM_SHAPES for t in G.STATS_K_TILES], ("bias_res_stats",), family="stats")


@pytest.mark.parametrize("small", [-1, 0], ids=["switch-to-cfg5", "gemm_small-off"])
def test_gemm_default_dispatch_at_the_cfg2_to_cfg5_switch(tune, small):
    """4096 x 1280 x 1280: 320 tiles of 128 x 128 (cfg 2), which cd360_gemm_bf16 moves to 256 x 128 tiles with three buffers (cfg 5) for
    K >= 1280; with gemm_small = 0 it stays on cfg 2."""
    from cd360 import ops
    tune(gemm_small=small)
    M, N, K = G.SWITCH_SHAPE
    assert ops.gemm_tile_n(M, N) == 128
    run_linear_cases(ops, [G.SWITCH_SHAPE], ("bias_res", "bias_res_stats"))


def test_gemm_asm4_switch_moves_a_256x256_launch_onto_the_generated_loop(tune):
    """gemm_asm4 = 1 with gemm_cfg = -1: cd360_gemm_bf16 reads the switch only where the default dispatch chose 256 x 256 tiles, which none
    of the small shapes reaches -- 4096 x 4096 does (pick_cfg's efficiency rule, restated and checked in tests/test_gemm_cases_cpu.py).
    Bit-equal to float64 with the switch on (cfg 9) and off (cfg 3)."""
    from cd360 import ops
    M, N, K = G.ASM4_SHAPE
    for asm4 in (1, 0):
        tune(gemm_cfg=-1, gemm_asm4=asm4)
        assert ops.gemm_tile_n(M, N) == 256
        run_linear_cases(ops, [G.ASM4_SHAPE], ("bias_res", "bias_res_stats"))


@pytest.mark.parametrize("route", G.CSTATS_ROUTES, ids=[r[0] for r in G.CSTATS_ROUTES])
def test_gemm_cstats_output_and_slab_statistics_bit_equal(tune, route):
    """cd360_gemm_cstats_bf16 on the 64-row tilings (cfg 2, cfg 4 in both wave arrangements), the 32-row tiling (cfg 8, both) and the
    default dispatch: output and per-slab channel (sum, sum of squares) bit-equal to float64."""
    from cd360 import ops
    tune(**route[1])
    bad = []
    for M in G.CSTATS_M:
        for N, K in G.CSTATS_NK:
            d = linear_on_device(M, N, K, "stats")
            want = d["want"]["bias_res"]
            for strided in (False, True):
                tag = f"{M}x{N}x{K}{' strided' if strided else ''}"
                sfx = "_s" if strided else ""
                runs = [ops.gemm_cstats(d["a" + sfx], d["w" + sfx], bias=d["bias"], res=d["res" + sfx]) for _ in range(2)]
                out, cst = runs[0]
                assert cst is not None, f"{tag}: no slab statistics on this route"
                slab = M // cst.shape[0]
                assert slab == (route[2] or slab) and slab in (32, 64) and cst.shape == (M // slab, N, 2)
                if not torch.equal(out, want):
                    bad.append(f"{tag}: out {describe(out, want)}")
                ws = G.slab_stats(want, slab).float()
                if not torch.equal(cst, ws):
                    bad.append(f"{tag}: cstats (slab {slab}) {describe(cst.reshape(-1, 2 * N), ws.reshape(-1, 2 * N))}")
                if not (torch.equal(out, runs[1][0]) and torch.equal(cst, runs[1][1])):
                    bad.append(f"{tag}: repeated launches differ")
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:12])


@pytest.mark.parametrize("route", G.GEGLU_ROUTES, ids=[r[0] for r in G.GEGLU_ROUTES])
def test_geglu_pairs_values_with_gates(tune, route):
    """Flag bit 0 on cfg 1, 3, 5, 7, 9, the default (cfg 7) and gemm_asm4 = 1 (which moves the default to cfg 9): operands in {-1, 0, 1} and an integer bias make the value and gate
    pre-activations exact integers (gates within [-6, 6]); every output element -- the value / gate pairing, the geglu_row_order packing,
    the N / 2 indexing -- must lie between bf16(want - delta) and bf16(want + delta), want = v gelu(g) in float64,
    delta = 3.13e-7 |v| max(|g|, 1) (gemm_cases.GEGLU_C: half of Abramowitz-Stegun 7.1.26's 1.5e-7 + four fp32 roundings).
    Measured on an MI355X, worst error relative to delta over all shapes: 0.034 on every route (the epilogue's arithmetic does not depend
    on the tiling), no element outside its band.  The figure is a lower bound on the fp32 error -- the distance from want to the bf16
    rounding boundary the kernel's value crossed -- and a clean fp32 evaluation of the exact formula on the CPU crosses the same one.
    The test prints it (GEMM-EXACT geglu ...)."""
    from cd360 import ops
    tune(**route[1])
    bad, worst = [], 0.0
    for M, N in G.GEGLU_SHAPES:
        for K in G.GEGLU_K:
            c = G.geglu_case(M, N, K)
            perm = ops.geglu_row_order(N // 2, DEV)
            assert torch.equal(perm.cpu(), G.geglu_row_order(N // 2))
            a, w, b = c.a.to(DEV, BF), c.w.to(DEV, BF)[perm].contiguous(), c.bias.to(DEV, torch.float32)[perm].contiguous()
            for strided in (False, True):
                tag = f"{M}x{N}x{K}{' strided' if strided else ''}"
                if strided:
                    wide, view = widen(torch.zeros(M, N // 2, dtype=BF, device=DEV))
                    outs = [ops.gemm(widen(a)[1], widen(w)[1], bias=b, geglu=True, out=view).clone() for _ in range(2)]
                    if not padding_intact(wide, N // 2):
                        bad.append(f"{tag}: padding written")
                else:
                    outs = [ops.gemm(a, w, bias=b, geglu=True) for _ in range(2)]
                ok, ratio = G.geglu_accepts(c, outs[0])
                worst = max(worst, ratio)
                if not ok:
                    lo, hi, _ = G.geglu_band(c)
                    g = outs[0].cpu().double()
                    out_of = ((g < lo.double()) | (g > hi.double())).nonzero()
                    i = tuple(out_of[0].tolist())
                    bad.append(f"{tag}: {out_of.shape[0]} of {g.numel()} outside the band, error / delta {ratio:.3g}, first {i}: got {g[i].item()!r} "
                               f"want {c.want[i].item()!r} v {c.v[i].item()} g {c.g[i].item()}")
                if not torch.equal(outs[0], outs[1]):
                    bad.append(f"{tag}: repeated launches differ")
    print(f"GEMM-EXACT geglu {route[0]}: worst error / delta = {worst:.4f}")
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:12])


@pytest.mark.parametrize("M", G.TN_M)
def test_gemm_tn_bit_equal(M):
    """cd360_gemm_tn_bf16 (the weight gradient): fewer rows than one 64-row tile, ragged last tiles, one slab and several slabs with a
    ragged last one; the fp32 output equals the float64 product (an exact integer: no rounding at all), the bf16 output its RNE;
    contiguous and strided operands."""
    from cd360 import ops
    bad = []
    for N, K in G.TN_NK:
        c = G.tn_case(M, N, K)
        a, b = c.a.to(DEV, BF), c.b.to(DEV, BF)
        want = {torch.float32: c.out.float().to(DEV), BF: G.rne(c.out).to(DEV)}
        for strided in (False, True):
            (aw, av), (bw, bv) = (widen(a), widen(b)) if strided else ((a, a), (b, b))
            assert ops.gemm_tn_ok(av, bv)
            for dt in (torch.float32, BF):
                tag = f"{M}x{N}x{K} {str(dt)[6:]}{' strided' if strided else ''}"
                outs = [ops.gemm_tn(av, bv, out_dtype=dt) for _ in range(2)]
                if not torch.equal(outs[0], want[dt]):
                    bad.append(f"{tag}: {describe(outs[0], want[dt])}")
                if not torch.equal(outs[0], outs[1]):
                    bad.append(f"{tag}: repeated launches differ")
            if strided and not (padding_intact(aw, N) and padding_intact(bw, K)):
                bad.append(f"{M}x{N}x{K}: operand padding written")
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:12])


@pytest.mark.parametrize("r", G.LOWRANK_R)
def test_lowrank_add_bit_equal(r):
    """cd360_lowrank_add_bf16 at p = 0: RNE(base + T U^T) bit for bit, with and without base, into a fresh output and in place on a
    column slice of a wider tensor (strided t and u as well)."""
    from cd360 import ops
    bad = []
    for M in G.LOWRANK_M:
        for N in G.LOWRANK_N:
            c = G.lowrank_case(M, N, r)
            t, u, base = c.t.to(DEV, BF), c.u.to(DEV, BF), c.base.to(DEV, BF)
            assert ops.lowrank_add_ok(t, u, base)
            for with_base in (False, True):
                want = c.want(with_base).to(DEV)
                tag = f"{M}x{N} r={r}{' base' if with_base else ''}"
                outs = [ops.lowrank_add(t, u, base=base if with_base else None) for _ in range(2)]
                if not torch.equal(outs[0], want):
                    bad.append(f"{tag}: {describe(outs[0], want)}")
                if not torch.equal(outs[0], outs[1]):
                    bad.append(f"{tag}: repeated launches differ")
                # strided: t, u column slices; the output a column slice of a wider tensor that holds base and is updated in place
                wide, view = widen(base if with_base else torch.full_like(base, PAD))
                got = ops.lowrank_add(widen(t)[1], widen(u)[1], base=view if with_base else None, out=view)
                if got.data_ptr() != view.data_ptr() or not torch.equal(view, want):
                    bad.append(f"{tag} in place, strided: {describe(view, want)}")
                if not padding_intact(wide, N):
                    bad.append(f"{tag} in place, strided: padding written")
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:12])


@pytest.mark.parametrize("r", G.LOWRANK_R)
def test_lowrank_add_with_dropout_bit_equal(r):
    """The masked form at p = 0.5, where s = 1 / (1 - p) = 2 keeps the arithmetic exact: RNE(base + 2 keep (T U^T)) bit for bit, with the
    mask read from cd360_dropout_apply_bf16 on ones (the same (key, site, element) function)."""
    from cd360 import ops
    M, N = 77, 320
    c = G.lowrank_case(M, N, r)
    t, u, base = c.t.to(DEV, BF), c.u.to(DEV, BF), c.base.to(DEV, BF)
    key = torch.tensor([20240607, 3], dtype=torch.int64, device=DEV)
    mask = ops.dropout_apply(torch.ones(M, N, dtype=BF, device=DEV), 0.5, 5, key=key).cpu().double()
    assert set(mask.unique().tolist()) == {0.0, 2.0} and 0.4 < (mask != 0).double().mean().item() < 0.6
    for with_base in (False, True):
        want = G.rne(mask * c.prod + (c.base if with_base else 0)).to(DEV)
        outs = [ops.lowrank_add(t, u, base=base if with_base else None, p=0.5, site=5, key=key) for _ in range(2)]
        assert torch.equal(outs[0], want), describe(outs[0], want)
        assert torch.equal(outs[0], outs[1])
