"""The claims of tests/softmax_cases.py, proved from its float64 reference alone for every case the GPU tests run: margins, stair
steps, offsets, placement, the share of crafted rows, the scale of the uncrafted rows and gradients, and the fp32 oracle's distance
from the float64 reference (one tenth of every bar of tests/test_softmax_edges_gpu.py / test_softmax_edges_bwd_gpu.py)."""
import pytest
import torch

import softmax_cases as S
from oracle import pose_path as O

ALL = S.FORWARD_CASES + S.BWD_CASES
BAR_OUT, BAR_DOM, BAR_GRAD = 1e-2, 2.0 ** -7, 2e-2  # the tightest tensor-wide forward bar, the dominated-row bar, the gradient bar


def tiles(case):
    return S.SINGLE_KT if case.geometry == "single" else 64


@pytest.mark.parametrize("sp", ALL, ids=S.spec_id)
def test_case_claims(sp):
    case = S.make_case(*sp)
    assert S.make_case(*sp) is case and torch.equal(case.q, S.bf(case.q)) and torch.equal(case.k, S.bf(case.k))  # deterministic, bf16 values
    assert torch.equal(case.v, S.bf(case.v)) and torch.equal(case.do, S.bf(case.do))
    units, p = S.logits(case)
    assert units.abs().max().item() <= 200.0  # fp32 score arithmetic is not what is being tested
    B, H, Nq, Nk = case.B, case.H, case.Nq, case.Nk
    qmask = case.crafted_q_mask().permute(0, 2, 1)  # [B, H, Nq]
    if case.family == "uniform":
        # the family is a whole (batch, head) by definition: the shares below are stated for the other families
        (b, h), = case.uniform_heads
        assert torch.equal(case.k.reshape(B, Nk, H, -1)[b, :, h], case.k.reshape(B, Nk, H, -1)[b, :1, h].expand(Nk, -1))
        assert (case.v.reshape(B, Nk, H, -1)[b, :, h] >= 0).all()
        row = units[b, h]
        assert (row == row[:, :1]).all()
        ref = S.reference(case)
        want = row[:, 0] * S.LN2 + torch.log(torch.tensor(float(Nk), dtype=torch.float64))
        assert (ref.lse.reshape(B, H, Nq)[b, h] - want).abs().max().item() < 1e-9
    else:
        assert len(case.rows) * 8 <= B * H * Nq and len(case.crafted_keys) * 8 <= B * H * Nk
        assert len(set((r.b, r.h, r.i) for r in case.rows)) == len(case.rows)
    if not (B * H == 1 and case.family == "uniform"):
        w = p.amax(-1)[~qmask].mean().item()
        assert 0.01 < w < 0.9, w

    # placement: every 32-query block of a crafted head holds a crafted row, all four lane offsets occur, more than one workgroup
    heads = sorted(set((r.b, r.h) for r in case.rows))
    if case.family != "uniform":
        for b, h in heads:
            blocks = set(r.i // 32 for r in case.rows if (r.b, r.h) == (b, h))
            assert blocks == set(range(-(-Nq // 32)))
        if Nq >= 128:
            assert set(r.i % 32 for r in case.rows) >= set(S.LANE_OFFSETS)
        assert len(heads) >= 2 or len(set(r.i // 128 for r in case.rows)) >= 2 or case.family == "cold-start" or Nq < 128

    t = tiles(case)
    for r in case.rows:
        row = units[r.b, r.h, r.i]
        others = torch.ones(Nk, dtype=torch.bool)
        others[list(r.keys)] = False
        if r.family in ("late-spike", "tie", "stair-down"):
            win = row[list(r.keys)]
            assert (win == win[0]).all() and win[0].item() > 128.0 + 8.0
            assert win[0].item() - row[others].max().item() >= r.margin >= 40.0
            assert len(r.keys) == (2 if r.family == "tie" else 1) and r.target is not None
        if r.family == "stair-down":
            assert r.keys[0] < t and (Nk <= t or row[t:].max().item() <= row[r.keys[0]].item() - 40.0)
            if case.geometry == "single" and S.single_splits(Nk)[0] > 1:  # every other split's weight 2^(lse2 - max) leaves fp32's normal range
                per = S.single_splits(Nk)[1]
                assert torch.logsumexp(row[per:] * S.LN2, 0).item() / S.LN2 <= row[r.keys[0]].item() - 126.0
        if r.family == "stair-up":
            mx = torch.stack([row[64 * j:64 * j + 64].max() for j in range(-(-Nk // 64))])
            step = mx[1:] - mx[:-1]
            assert ((step > 11.0) & (step < 13.0)).all() and row.argmax().item() == r.keys[0] >= 64 * (len(mx) - 1)
        if r.family == "cold-start":
            assert row[:t].max().item() < -128.0 and row[t:].max().item() > -30.0
        if r.family == "offset":
            assert (torch.sign(row) == torch.sign(row[0])).all() and (row.abs() - abs(case.L)).abs().max().item() <= 35.0
    if case.family == "offset":
        signs = set(torch.sign(units[r.b, r.h, r.i, 0]).item() for r in case.rows)
        assert signs == ({-1.0, 1.0} if sp[-1] == "both" else {-1.0})

    # where the dominating keys sit: every position class of the geometry, in every crafted head
    if case.family == "late-spike":
        classes = S.key_classes(case.geometry, Nk)
        for b, h in heads:
            got = set(r.where for r in case.rows if (r.b, r.h) == (b, h))
            assert got == set(c[0] for c in classes[:len(set(r.group for r in case.rows))])
        for r in case.rows:
            lo, hi = next((c[1], c[2]) for c in classes if c[0] == r.where)
            assert lo <= r.keys[0] < hi or hi - lo < 2
    if case.family == "tie" and case.geometry == "single" and S.single_splits(Nk)[0] > 1:
        per = S.single_splits(Nk)[1]
        assert all(r.keys[0] // per != r.keys[1] // per for r in case.rows)
    if case.family == "tie":
        assert all(r.keys[0] < t and r.keys[1] >= (Nk - 1) // t * t for r in case.rows) or case.geometry in ("smallk", "bwd")


@pytest.mark.parametrize("sp", ALL, ids=S.spec_id)
def test_fp32_oracle_is_within_a_tenth_of_every_bar(sp):
    case = S.make_case(*sp)
    grads = sp in S.BWD_CASES
    ref = S.reference(case, grads=grads)
    B, H, D = case.B, case.H, case.D
    qs = case.q * (case.c / (D ** -0.5 * S.LOG2E))  # the oracle's scale is D^-0.5: what is left of c goes into q (exact or one fp32 rounding)

    def split(x):
        return case.heads4(x).reshape(B * H, x.shape[1], D)

    q, k, v = (x.clone().requires_grad_(grads) for x in (qs, case.k, case.v))
    out = O.attention_core(split(q), split(k), split(v)).reshape(B, H, case.Nq, D).permute(0, 2, 1, 3).reshape(B, case.Nq, H * D)
    scale = ref.out.abs().max().item()
    assert (out.detach().double() - ref.out).abs().max().item() / scale < BAR_OUT / 10
    for r in case.rows:
        if r.target is not None:
            got = S.row_of(case, out.detach().double(), r.b, r.h, r.i)
            assert ((got - r.target).abs() <= BAR_DOM / 10 * r.target.abs()).all()
            assert ((S.row_of(case, ref.out, r.b, r.h, r.i) - r.target).abs() <= BAR_DOM / 10 * r.target.abs()).all()
    if grads:
        got = torch.autograd.grad(out, (q, k, v), case.do)
        got = (got[0] * (case.c / (D ** -0.5 * S.LOG2E)), got[1], got[2])
        for g, w in zip(got, (ref.dq, ref.dk, ref.dv)):
            assert (g.double() - w).abs().max().item() / w.abs().max().item() < BAR_GRAD / 10


@pytest.mark.parametrize("sp", S.BWD_CASES, ids=S.spec_id)
def test_backward_case_claims(sp):
    case = S.make_case(*sp)
    ref = S.reference(case, grads=True)
    B, H, Nq, Nk, D = case.B, case.H, case.Nq, case.Nk, case.D
    qm, km = case.crafted_q_mask(), case.crafted_k_mask()
    # the largest gradient of each tensor belongs to an uncrafted row / key: the max-normalised bars are set by ordinary rows
    for g, m in ((ref.dq, qm), (ref.dk, km), (ref.dv, km)):
        a = g.reshape(B, g.shape[1], H, D).abs().amax(-1)
        assert not m.any() or a[~m].max().item() > a[m].max().item()
    if case.family in ("late-spike", "tie"):
        p = S.logits(case)[1]
        for b, h, j, won in case.dominating:  # a won row enters dv_j with P = 1 (1 / 2 on a tie) exactly, to 2^-40
            assert (p[b, h, list(won), j] - (0.5 if case.family == "tie" else 1.0)).abs().max().item() < 2.0 ** -40
        classes = S.key_classes("bwd", Nk)
        n64 = -(-Nq // 64)
        for b, h, j, won in case.dominating:
            assert len(won) >= 8 and (Nq - 1) // 64 in set(i // 64 for i in won) and len(set(i // 64 for i in won)) >= min(n64, 4)
        for b in range(B):
            for h in range(H):
                keys = [j for bb, hh, j, _ in case.dominating if (bb, hh) == (b, h)]
                for _, lo, hi in classes if case.family == "late-spike" else ():  # every wave of a 128-key tile, and the ragged last tile where there is one
                    assert any(lo <= j < hi for j in keys)
        # every wave of a 128-query tile of the dQ role holds crafted queries
        assert set((r.i // 32) for r in case.rows) == set(range(-(-Nq // 32)))
