"""The exact-integer cases of tests/gemm_cases.py, validated without a GPU: every case the GPU tests build meets the conditions its
exactness rests on (operands representable, every partial sum below 2^24), is not exact merely because nothing rounds, and would
expose every defect of the fault models that applies to it -- one product dropped, a K-tile added twice, truncation, a rounding in front
of the residual, a shifted bias slice, a misplaced ragged column group, statistics of unrounded values, a TN partial tile left out,
rows past M read as data.  So a bit-equal GPU result says something, and a case list that drifts is caught here, not on the GPU."""
import pytest
import torch

import gemm_cases as G

LINEAR = sorted(set(G.linear_cases()))


def test_rounding_helpers_against_hand_values():
    # 257 lies halfway between 256 and 258: RNE -> 256 (even mantissa), 259 -> 260 (tie, odd mantissa below), truncation drops towards zero
    x = torch.tensor([257.0, 259.0, 258.0, -257.0, -259.0, 513.0, 515.0, 100.0], dtype=torch.float64)
    assert G.rne(x).tolist() == [256.0, 260.0, 258.0, -256.0, -260.0, 512.0, 516.0, 100.0]
    assert G.truncate(x).tolist() == [256.0, 258.0, 258.0, -256.0, -258.0, 512.0, 512.0, 100.0]
    inexact, ties, differ = G.rounding_shares(x)
    assert (inexact, ties, differ) == (6 / 8, 4 / 8, 3 / 8)
    with pytest.raises(AssertionError):
        G.rne(torch.tensor([2.0 ** 24 + 1], dtype=torch.float64))


def test_issue_reference_ranges_meet_the_floors():
    """A in [-16, 16], W in [-8, 8], bias in [-64, 64], res in [-128, 128] at 300 x 272: at K = 64 and 1280 at least 25 % of the outputs need
    rounding, 5 % are exact ties, and the worst sum stays far below 2^24."""
    for K in (64, 1280):
        c = G.linear_case(300, 272, K)
        bound = (c.a.abs() @ c.w.abs().t()).max().item() + 64 + 128
        inexact, ties, differ = G.rounding_shares(c.pre("bias_res"))
        print(f"GEMM-CASES K={K}: bound {bound:.0f}, inexact {inexact:.3f}, ties {ties:.3f}, truncation != RNE {differ:.3f}")
        assert bound < 2 ** 20 and inexact >= 0.25 and ties >= 0.05 and differ >= 0.10


@pytest.mark.parametrize("family,M,N,K", LINEAR, ids=[f"{f}-{m}x{n}x{k}" for f, m, n, k in LINEAR])
def test_linear_case_is_exact_nontrivial_and_detects_every_fault(family, M, N, K):
    c = G.linear_case(M, N, K, family)
    G.check_linear(c)
    assert G.nontrivial_linear(c)
    if family == "main":
        for e in ("none", "bias", "bias_res"):
            inexact, ties, _ = G.rounding_shares(c.pre(e))
            assert inexact >= G.MIN_INEXACT and ties >= G.MIN_TIES, (e, inexact, ties)
    big = (M, N, K) in G.BIG_SHAPES  # (their defects on one epilogue: 5 M and 17 M outputs)
    for e in (("bias_res",) if big else G.EPILOGUES):
        want = c.want(e)
        names = []
        for name, rounding, bad in G.linear_faults(c, e):
            moved = (bad != want).double().mean().item()
            assert moved > 0, f"{e}: {name} changes no output bit"
            assert not rounding or moved >= G.MIN_ROUNDING_FAULT, f"{e}: {name} moves only {moved:.4f} of the outputs"
            names.append(name)
        assert {"k-index-dropped-in-one-block", "k-tile-added-twice"} <= set(names)
        assert family != "main" or "truncation" in names
    if family == "stats":
        for tile_n in (128, 192, 256):
            for name, right, bad in G.stats_faults(c, tile_n):
                assert right.abs().max().item() < G.TWO24 and not torch.equal(right, bad), f"{name} at tile_n={tile_n} goes unseen"
        if M * N >= G.STATS_MIN_OUTPUTS:
            assert G.rounding_shares(c.pre("bias_res"))[0] >= G.MIN_STATS_INEXACT and G.stats_blocks_round(c)
            # ... so every partial notices: each 128-column tile of the row statistics, each 64-row slab of the slab statistics
            faults = {name: (right, bad) for name, right, bad in G.stats_faults(c, 128, 64)}
            right, bad = faults["row-stats-of-unrounded"]
            assert all(not torch.equal(right[:, q], bad[:, q]) for q in range(right.shape[1]))
            if M % 64 == 0:
                right, bad = faults["slab-stats-of-unrounded"]
                assert all(not torch.equal(right[q], bad[q]) for q in range(right.shape[0]))


def test_linear_case_lists_cover_what_the_routes_need():
    ks = {K for _, _, _, K in LINEAR}
    assert {64 * t for t in range(1, 13)} | {1280, 3072, 5120} <= ks
    ids = [r[0] for r in G.GEMM_ROUTES]
    assert len(set(ids)) == len(ids)
    cfgs = {r[1].get("gemm_cfg") for r in G.GEMM_ROUTES}
    assert set(range(1, 10)) <= cfgs and {"default", "small-off"} <= set(ids)
    assert {f"cfg4-ksplit{k}" for k in (0, 1, 2)} | {f"cfg8-ksplit{k}" for k in (0, 1)} <= set(ids)
    assert all(f"cfg{c}-movers{m}" in ids for c in G.MOVER_CFGS for m in (0, 4))
    M, N, K = G.SWITCH_SHAPE
    tiles = -(-M // 128) * -(-N // 128)
    assert 256 < tiles <= 512 and K >= 1280 and N <= 1536 and M < 65536  # pick_cfg: cfg 2; cd360_gemm_bf16 then moves it to cfg 5
    # gemm_asm4 is read only after the default dispatch chose 256 x 256 tiles: its shape does, none of the small shapes would
    assert G.default_picks_256x256(*G.ASM4_SHAPE[:2]) and not any(G.default_picks_256x256(M, N) for M, N in G.GEMM_SHAPES + [G.SWITCH_SHAPE[:2]])
    assert ("asm4", dict(gemm_cfg=-1, gemm_asm4=1)) in G.GEGLU_ROUTES  # GEGLU: the default is cfg 7, which the switch moves as well


@pytest.mark.parametrize("M,N", G.GEGLU_SHAPES)
@pytest.mark.parametrize("K", G.GEGLU_K)
def test_geglu_case_and_band_rule(M, N, K):
    c = G.geglu_case(M, N, K)
    G.check_geglu(c)
    # the packing restated here is a permutation that puts value and gate of a column 32 rows apart
    perm = G.geglu_row_order(N // 2)
    assert sorted(perm.tolist()) == list(range(N))
    assert all(perm[64 * q + 32 + j] - perm[64 * q + j] == N // 2 for q in range(N // 64) for j in (0, 31))
    ok, worst = G.geglu_accepts(c, c.want.to(G.BF))
    assert ok and worst == 0.0
    # a clean fp32 evaluation of the exact formula sits well inside the band ...
    g32, v32 = c.g.float(), c.v.float()
    ok, worst = G.geglu_accepts(c, (v32 * (0.5 * g32 * (1 + torch.erf(g32 * 0.70710678118654752)))).to(G.BF))
    print(f"GEMM-CASES geglu {M}x{N}x{K}: fp32 evaluation at {worst:.3f} of delta")
    assert ok and worst < 0.5
    # ... and every defect outside it
    for name, bad in G.geglu_faults(c):
        assert not G.geglu_accepts(c, bad)[0], f"{name} is accepted"
    assert abs(G.GEGLU_C - 3.13e-7) < 0.01e-7


@pytest.mark.parametrize("M", G.TN_M)
@pytest.mark.parametrize("N,K", G.TN_NK)
def test_tn_case_is_exact_and_detects_every_fault(M, N, K):
    c = G.tn_case(M, N, K)
    G.check_tn(c)
    if M >= 63:
        inexact, ties, _ = G.rounding_shares(c.out)
        assert inexact >= G.MIN_INEXACT and ties >= G.MIN_TIES  # the bf16 output rounds
    names = []
    for name, bad in G.tn_faults(c):
        assert not torch.equal(bad, c.out) and not torch.equal(G.rne(bad), G.rne(c.out)), name
        names.append(name)
    assert ("partial-tile-left-out" in names) == (M > 64) and ("rows-past-M-read-as-data" in names) == (M % 64 != 0)


@pytest.mark.parametrize("r", G.LOWRANK_R)
@pytest.mark.parametrize("M", G.LOWRANK_M)
@pytest.mark.parametrize("N", G.LOWRANK_N)
def test_lowrank_case_is_exact_nontrivial_and_detects_every_fault(M, N, r):
    c = G.lowrank_case(M, N, r)
    G.check_lowrank(c)
    for with_base in (False, True):
        want = c.want(with_base)
        inexact, ties, _ = G.rounding_shares(c.prod + c.base if with_base else c.prod)
        assert inexact >= G.MIN_INEXACT and ties >= G.MIN_TIES
        for name, rounding, bad in G.lowrank_faults(c, with_base):
            moved = (bad != want).double().mean().item()
            assert moved > 0 and (not rounding or moved >= G.MIN_ROUNDING_FAULT), (name, moved)
