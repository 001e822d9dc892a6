"""The cases of tests/attn_tile_cases.py, checked without a GPU, for every case tests/test_attn_tile_gpu.py runs:
  * the builder conditions that make float64 the exact answer hold (integer logits, band width and bit budget, the stair's rises on both
    sides of the 8-unit slack and in both key halves, winner margins, padding inside the allocation and attractive);
  * an fp32 torch emulation of each pipeline -- eager maximum per 64-key tile (attn_fwd_kernel), lazy maximum with slack 8 starting at 0
    and P packed to bf16 (attn_self_kernel), 32-key tiles with normalised per-split parts and the lse2 merge (attn_single) -- stays, in
    two different summation orders, within a TENTH of the GPU bar (2^-8 |ref| + 2^-10 A) of the float64 reference in front of the one
    bf16 rounding of the output, and within the bar behind it; the same for dQ / dK of the backward with their own weighted means;
  * every fault model a case is listed for (attn_tile_cases.faults_for), applied to the emulation, breaks the bar;
  * the lazy cases take move_ref and catch_up after tile 0;
  * the restated dispatch names, for every case of the GPU file, the kernel the case is named for;
  * the lse bar: 4 x the worst error of the fp32 restatement."""
import numpy as np
import pytest
import torch

import attn_tile_cases as T
from softmax_cases import single_splits

FWD = T.forward_specs()
SINGLE = [T.single_spec(f, b, n, d) for b, n, d in T.SINGLE for f in T.FAMILIES]
BWD = [T.bwd_spec(nq, nk) for nq, nk in T.BWD_SHAPES]
EMU = {"eager": T.emulate_eager, "lazy": T.emulate_lazy, "single": T.emulate_single}


def test_scale_times_log2e_is_one_in_fp32():
    assert np.float32(T.SCALE) * np.float32(1.4426950408889634) == np.float32(1.0)


def test_lists_hold_what_the_gpu_file_names():
    assert T.GEN1_SHAPES == ((200, 97), (200, 200), (333, 333), (256, 256))
    assert T.SELF_SHAPES == {1: (256, 640), 3: (256, 768), 2: (512, 1024)}
    assert T.SINGLE == ((2, 256, 512), (1, 520, 320), (1, 1024, 128), (1, 600, 512)) and T.BWD_SHAPES == ((200, 200), (256, 256), (200, 97))
    assert {n: single_splits(n)[0] for _, n, _ in T.SINGLE} == T.SINGLE_SPLITS
    ids = [c[0] for c in T.FORWARD]
    assert len(set(ids)) == len(ids) == 18


@pytest.mark.parametrize("sp", sorted({s for s, _ in FWD}, key=T.spec_id) + SINGLE + BWD, ids=T.spec_id)
def test_builder_conditions(sp):
    T.check_conditions(T.make_case(sp))


def test_digits_and_level_plan():
    x = np.arange(-1687, 1688)
    d = T.digits15(x)
    assert all(np.abs(di).max() <= 7 for di in d) and np.array_equal(d[0] + 15 * d[1] + 225 * d[2], x)
    for nk, tile in ((97, 64), (200, 64), (1024, 64), (520, 32), (1024, 32)):
        lv, tops = T.level_plan(nk, tile)
        rise = np.diff(tops)
        assert set(rise.tolist()) <= set(range(3, 13)) | {20} and lv.max() == tops[-1] and len(lv) == nk
        for t in range(len(tops)):
            assert lv[t * tile:(t + 1) * tile].max() == tops[t]


def _check_forward(sp, pipeline, **kw):
    case = T.make_case(sp)
    ref = T.reference(case)
    emu = EMU[pipeline]
    for order in (0, 1):
        exact = T.worst_ratio(emu(case, order=order, round_out=False, **kw), ref)
        rounded = T.worst_ratio(emu(case, order=order, **kw), ref)
        print(f"ATTN-TILE-EMU {pipeline} {T.spec_id(sp)} order={order} unrounded={exact:.3e}/0.1 rounded={rounded:.3e}/1")
        assert exact <= 0.1 and rounded <= 1.0
        if sp.family == "onehot":
            assert torch.equal(emu(case, order=order, **kw), T.onehot_target(case).bfloat16())
    for fault in T.faults_for(sp, pipeline):
        r = T.worst_ratio(emu(case, fault=fault, **kw), ref)
        print(f"ATTN-TILE-FAULT {pipeline} {T.spec_id(sp)} {fault} {r:.3e}")
        assert r > 1.0, f"{T.spec_id(sp)} does not expose {fault} on the {pipeline} pipeline"


@pytest.mark.parametrize("sp,pipeline", FWD, ids=[f"{p}-{T.spec_id(s)}" for s, p in FWD])
def test_tiled_emulations_agree_and_fault_models_break_the_bar(sp, pipeline):
    _check_forward(sp, pipeline)
    if pipeline == "lazy" and sp.family == "mix":
        count = {}
        T.emulate_lazy(T.make_case(sp), count=count)
        print(f"ATTN-TILE-EMU lazy {T.spec_id(sp)} rows x tiles that moved m_ref after tile 0: {count}")
        assert count["moves"] > 0 and count["catch_ups"] > 0


@pytest.mark.parametrize("sp", SINGLE, ids=T.spec_id)
def test_single_head_emulation_agrees_and_fault_models_break_the_bar(sp):
    _check_forward(sp, "single")


def test_single_head_qscale():
    """qscale = 0.5 with q doubled is the same case; with qscale ignored it is not."""
    sp = T.single_spec("mix", 1, 520, 320)
    case = T.make_case(sp)
    ref = T.reference(case)
    assert T.worst_ratio(T.emulate_single(case, qscale=0.5, qmul=2.0, round_out=False), ref) <= 0.1
    assert T.worst_ratio(T.emulate_single(case, qscale=0.5, qmul=2.0, fault="qscale_ignored"), ref) > 1.0


def test_every_fault_model_is_listed_somewhere():
    listed = {"eager": set(), "lazy": set(), "single": set()}
    for sp, pipeline in FWD:
        listed[pipeline] |= set(T.faults_for(sp, pipeline))
    for sp in SINGLE:
        listed["single"] |= set(T.faults_for(sp, "single"))
    kv, tile, pads = set(T.KV_FAULTS), set(T.TILE_FAULTS), {"pad_zero", "pad_rows"}
    assert listed["eager"] == kv | tile
    assert listed["lazy"] == kv | tile - pads | set(T.LAZY_FAULTS)   # (whole tiles only)
    assert listed["single"] == kv - {"k_head", "v_head"} | tile | set(T.SINGLE_FAULTS) - {"qscale_ignored"}   # (one head; qscale: above)


def test_single_head_cases_reach_every_split_and_the_ragged_tile():
    for b, n, d in T.SINGLE:
        ns, per = single_splits(n)
        lv, tops = T.level_plan(n, T.SINGLE_KT)
        winners = T.make_case(T.single_spec("onehot", b, n, d)).winner.numpy()
        for s in range(ns):
            lo, hi = s * per, min((s + 1) * per, n)
            assert len(set(tops[lo // T.SINGLE_KT:-(-hi // T.SINGLE_KT)].tolist())) == -(-hi // T.SINGLE_KT) - lo // T.SINGLE_KT >= 1
            assert set(range(lo, hi)) <= set(winners.tolist())
        last = (n - 1) // T.SINGLE_KT * T.SINGLE_KT
        assert lv[last:].max() == tops[-1] == lv.max() and set(range(last, n)) <= set(winners.tolist())


@pytest.mark.parametrize("sp", BWD, ids=T.spec_id)
def test_backward_emulation_agrees_and_fault_models_break_the_bar(sp):
    case = T.make_case(sp)
    g = T.reference_bwd(case)
    rq, rk, _ = T.bwd_ratios(*T.emulate_bwd(case, round_out=False), g)
    bq, bk, dv_exact = T.bwd_ratios(*T.emulate_bwd(case), g)
    print(f"ATTN-TILE-EMU bwd {T.spec_id(sp)} dq={rq:.3e}/0.1 dk={rk:.3e}/0.1 rounded dq={bq:.3e}/1 dk={bk:.3e}/1 dv_exact={dv_exact}")
    assert rq <= 0.1 and rk <= 0.1 and bq <= 1.0 and bk <= 1.0 and dv_exact
    fq, fk, _ = T.bwd_ratios(*T.emulate_bwd(case, fault="delta_neighbour"), g)
    _, _, fv = T.bwd_ratios(*T.emulate_bwd(case, fault="dv_perm4"), g)
    print(f"ATTN-TILE-FAULT bwd {T.spec_id(sp)} delta_neighbour dq={fq:.3e} dk={fk:.3e} dv_perm4 exact={fv}")
    assert fq > 1.0 and fk > 1.0 and not fv


def test_route_restatement_names_every_case():
    for name, entry, tuning, nq, nk, kernel in T.FORWARD:
        b, h = (1, 4) if entry == "xformers" else (2, 2)
        assert T.route(entry, b, h, nq, nk, **tuning) == kernel, name
    # what the restatement says of shapes that cannot take a forced variant (such a case would be skipped, never run under that name)
    assert T.route("plain", 2, 2, 256, 256, attn_self=2) == "self<1,4>" and T.route("plain", 2, 2, 640, 640, attn_self=3) == "self<1,4>"
    assert T.route("plain", 2, 2, 200, 200, attn_self=1) == "gen1-fast" and T.route("plain", 2, 2, 256, 256, attn_self=1, aligned=False) == "gen1-fast"
    assert T.route("plain", 2, 2, 256, 96) == "smallk" and T.route("plain", 2, 2, 200, 97) == "gen1-fast"
    assert T.route("prescaled", 60, 10, 1024, 1024) == "self<2,8>" and T.route("lse", 2, 2, 256, 256) == "gen1-fast"


def test_lse_bar_is_four_times_the_fp32_restatement():
    """The fp32 restatement of what the kernels write: (m c + log2f(l)) ln 2 (eager) and (log2f(l) + m_ref) ln 2 (lazy)."""
    worst = 0.0
    for sp, pipeline in FWD:
        case = T.make_case(sp)
        _, lse = EMU[pipeline](case, want_lse=True)
        worst = max(worst, T.lse_ratio(lse, T.reference(case), rel=1.0))
    print(f"ATTN-TILE-EMU lse worst |fp32 - float64| / (|lse| + 1) = {worst:.3e}; bar = 4 x = {4 * worst:.3e}; LSE_REL = {T.LSE_REL:.3e}")
    assert 4 * worst <= T.LSE_REL <= 8 * worst
