"""The cases of tests/attn_grid_cases.py, checked without a GPU, for every case tests/test_attn_grid_gpu.py runs:
  * the builder conditions that make float64 the exact answer hold;
  * an fp32 torch emulation of the bf16 and of the fp8 pipeline stays within a TENTH of the GPU bar (2^-8 |ref| + 2^-10 A) of the float64
    reference in front of the one bf16 rounding of the output, and within the bar behind it;
  * every fault model the case is listed for (attn_grid_cases.faults_for), applied to the emulation, breaks the bar.  A case that does
    not expose one of its fault models fails here;
  * the host restatement of the packed e4m3 image is a bijection of the 96 x 64 + 64 x 96 values and keeps keys >= Nk zero."""
import numpy as np
import pytest
import torch

import attn_grid_cases as G

ALL = G.all_specs()


def test_scale_times_log2e_is_one_in_fp32():
    assert np.float32(G.SCALE) * np.float32(1.4426950408889634) == np.float32(1.0)
    assert float(G.c_f32()) == 1.0


def test_lists_hold_what_the_gpu_file_names():
    assert G.NK_BF16 == (16, 17, 32, 33, 48, 64, 65, 77, 80, 81, 95, 96) and G.NK_FP8 == (65, 77, 80, 81, 96)
    assert G.NK_CORE == (20, 32, 33, 64, 65, 77, 96) and G.NQ_CORE == (256, 200) and G.NK_PACK == (1, 31, 64, 77, 96)
    assert {(sp.N, sp.K) for sp, _, _ in ALL if sp.imode == "vary"} == {(128, 192), (384, 384)}
    assert {sp.imode for sp, _, _ in ALL} == {"vary", 0, 1, 2}


@pytest.mark.parametrize("sp", [a[0] for a in ALL] + [G.pack_spec(nk) for nk in G.NK_PACK], ids=G.spec_id)
def test_builder_conditions(sp):
    G.check_conditions(G.make_case(sp))


def _emulations(sp, bf16, fp8):
    core = sp.imode != "vary"
    runs = []
    if bf16:
        runs.append(("bf16", lambda c, **kw: G.emulate_bf16(c, **kw)))
    if fp8:
        amax = G.core_amax(sp) if core else None
        runs.append(("fp8core" if core else "fp8", lambda c, **kw: G.emulate_fp8(c, per_tensor_amax=amax, **kw)))
    return runs


@pytest.mark.parametrize("sp,bf16,fp8", ALL, ids=[G.spec_id(a[0]) for a in ALL])
def test_emulations_agree_and_fault_models_break_the_bar(sp, bf16, fp8):
    case = G.make_case(sp)
    ref = G.reference(case)
    for route, emu in _emulations(sp, bf16, fp8):
        exact = G.worst_ratio(emu(case, round_out=False), ref)
        rounded = G.worst_ratio(emu(case), ref)
        print(f"ATTN-GRID-EMU {route} {G.spec_id(sp)} unrounded={exact:.3e}/0.1 rounded={rounded:.3e}/1")
        assert exact <= 0.1 and rounded <= 1.0
        if sp.family == "onehot":
            assert torch.equal(emu(case), G.onehot_target(case).bfloat16())
        for fault in G.faults_for(sp, route):
            r = G.worst_ratio(emu(case, fault=fault), ref)
            print(f"ATTN-GRID-FAULT {route} {G.spec_id(sp)} {fault} {r:.3e}")
            assert r > 1.0, f"{G.spec_id(sp)} does not expose {fault} on the {route} route"


def test_every_fault_model_is_listed_somewhere():
    listed = {"bf16": set(), "fp8": set(), "fp8core": set()}
    for sp, bf16, fp8 in ALL:
        for route, _ in _emulations(sp, bf16, fp8):
            listed[route] |= set(G.faults_for(sp, route))
    assert listed["bf16"] == set(G.FAULTS_BF16) and listed["fp8"] == set(G.FAULTS_FP8)
    assert listed["fp8core"] == {"k_chan_swap", "v_key_perm", "pad_unmasked", "nk_round16"}


@pytest.mark.parametrize("nk", G.NK_PACK)
def test_image_layout_is_a_bijection(nk):
    case = G.make_case(G.pack_spec(nk))
    img, scales = G.kv_image(case.k, case.v, nk)
    nb, H = case.k.shape[0], case.H
    assert img.shape == (nb, H, G.IMAGE_BYTES) and img.dtype == torch.uint8 and scales.shape == (nb, H, 2)
    for row in G.K_INDEX:
        assert sorted(row.tolist()) == list(range(64))
    for row in G.V_INDEX:
        assert sorted(row.tolist()) == list(range(128))
    k8, v8 = G.decode_image(img)
    qk, sk = G.quantise(case.k, nk)
    qv, sv = G.quantise(case.v, nk)
    assert torch.equal(k8, qk) and torch.equal(v8, qv) and torch.equal(scales[..., 0], sk) and torch.equal(scales[..., 1], sv)
    assert not k8[:, nk:].any() and not v8[:, nk:].any()
    for b in range(nb):
        for h in range(H):
            assert float(sk[b, h]) == 2.0 ** (G.jk_of(b, h) - 6) and float(sv[b, h]) == 2.0 ** (G.jv_of(b, h) - 6)
    # lossless on the grid: decoded value times scale is k, v itself
    assert torch.equal(k8[:, :nk].double() * sk.double()[:, None, :, None], case.k[:, :nk])
    assert torch.equal(v8[:, :nk].double() * sv.double()[:, None, :, None], case.v[:, :nk])
    # two spot values straight from the comment: K byte 0 of row 4 is chunk 0 ^ 1 -> logical byte 16 -> channel 32; V^T byte 0 of
    # row 2 is chunk 0 ^ 1 -> slot 16 -> key 32
    assert G.K_INDEX[4, 0] == 32 and G.K_INDEX[0, 16] == 32 and G.K_INDEX[0, 32] == 16
    assert G.V_INDEX[2, 0] == 32 and G.V_INDEX[0, 1] == 1 and G.V_INDEX[0, 4] == 8 and G.V_INDEX[0, 32] == 4 and G.V_INDEX[0, 64] == 64
