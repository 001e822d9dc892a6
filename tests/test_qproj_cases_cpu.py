"""The method of tests/qproj_cases.py, checked without a GPU: the fp32 restatements of the whole chain (exact projection, LayerNorm fold in
the source's expression order, row epilogue in two summation orders) stay inside half of the fp32 parts of the bars and the flagged
shares under their caps; every fault model is caught in every case listed for it; the builders' assertions fire; the covering list
covers what it states.  Prints QPROJ-CPU lines with the measured use of every constant."""
import itertools

import pytest
import torch

import attn_round_cases as RC
import qproj_cases as QC

DATA = QC._data_cases("A") + QC._data_cases("B")
IDS = [QC.data_id(d) for d in DATA]


@pytest.mark.parametrize("d", DATA, ids=IDS)
def test_fp32_restatements(d):
    e = QC.emulate(d)
    b = e.b
    A = e.ex.A
    unit_use = 0.0
    if d.kind == "B":
        for variant, ulp in itertools.product((0, 1, 2), (-1, 1)):
            t32 = QC.project(b, f32=(variant, ulp))
            unit_use = max(unit_use, float(((t32 - b.t).abs() / b.unit).max()))
        # C_T is the SMALLEST power of two that holds: half of it does not, somewhere on the list (test_unit_is_minimal)
    else:
        assert torch.equal(QC.project(b, f32=(0, 0)), b.t)
    figs = []
    for order, f32 in ((0, (0, 1)), (1, (1, -1))):
        t32 = QC.project(b, f32=f32)
        e32 = RC.emulate_row(QC.case_of(b, t32), f32=True, order=order)
        eps_use = float((((e32.o - e.fwd.o).abs() - e.F) / (RC.EPS * A)).max())
        worst = float(QC.ratios(e32.out(), e).max())
        figs.append((eps_use, worst))
    t_rne = RC.bias(e.fwd.out(), RC.flat(e.ex.out), RC.flat(A))
    print(f"QPROJ-CPU {QC.data_id(d)} j={b.j} q std={float(RC.rnd(b.t).std()):.2f} rounded={b.rounded:.3f} ties={b.ties:.3f} unit use={unit_use:.3f} "
          f"flagged_q={e.flagged_q:.5f} flagged_p={e.flagged_p:.5f} rows_q={e.rows_q:.4f} fp32 (eps use, worst err/bar) " + " ".join(f"{x:.3f}/{y:.3f}" for x, y in figs)
          + f" T_rne={t_rne:.2e} T_trunc={e.t_trunc if e.t_trunc is None else format(e.t_trunc, '.2e')}")
    assert unit_use <= 0.5
    assert e.flagged_q <= QC.FLAG_CAP_Q and e.flagged_p <= RC.FLAG_CAP_P and e.rows_q <= 64 * QC.FLAG_CAP_Q
    for eps_use, worst in figs:
        assert eps_use <= 0.5 and worst <= 1.0
    if d.family == "positive":
        assert abs(e.t_trunc) > 5e-4 and abs(t_rne) <= abs(e.t_trunc) / 20


def test_unit_is_minimal():
    """C_T / 2 would not hold half of itself on the offset rows at the longest K."""
    worst = 0.0
    for d in QC._data_cases("B"):
        b = QC.build(d)
        for variant, ulp in itertools.product((0, 1, 2), (-1, 1)):
            worst = max(worst, float(((QC.project(b, f32=(variant, ulp)) - b.t).abs() / b.unit).max()))
    print(f"QPROJ-CPU worst use of the fold's unit over family B: {worst:.3f}")
    assert 0.25 < worst <= 0.5


@pytest.mark.parametrize("d", DATA, ids=IDS)
def test_fault_models_are_caught(d):
    e = QC.emulate(d)
    want, A = RC.flat(e.ex.out), RC.flat(e.ex.A)
    for fault in QC.faults_for(d):
        out = QC.faulty_out(e, fault)
        reg = QC.region(d, fault)
        share = float((QC.ratios(out, e)[reg] > 1).double().mean())
        t = RC.bias(out, want, A)
        biased = d.family == "positive" and abs(t) > abs(e.t_trunc) / 4
        print(f"QPROJ-CPU {QC.data_id(d)} fault {fault}: outside the bar {share:.3f} of {int(reg.sum())}, T={t:.2e}" + (" (T bar broken)" if biased else ""))
        assert share >= 0.10 or biased, fault


def test_every_fault_model_is_listed_somewhere():
    listed = set(f for d in DATA for f in QC.faults_for(d))
    assert listed == set(QC.Q_FAULTS)


def test_builder_assertions_fire(monkeypatch):
    QC.build.cache_clear()
    try:
        with pytest.raises(AssertionError, match="changes under the bf16 rounding"):     # |t| below 256 units: nothing to round
            QC.build(QC.Data("A", "peaked", 64, 128, 20, amax=1))
        monkeypatch.setattr(QC, "W_LO", 200)
        monkeypatch.setattr(QC, "W_HI", 255)
        with pytest.raises(AssertionError, match="fp32 integers"):
            QC.build(QC.Data("A", "spread", 1280, 128, 20, amax=127))
        monkeypatch.undo()
        with pytest.raises(AssertionError):      # a plain row kind asked of data that is not: the ratio assertion
            monkeypatch.setattr(QC, "_rows", lambda d, g, n: QC._ints(g, (n, d.Nq, d.K), 20, 24) + QC._ints(g, (n, d.Nq, 1), 0, 9))
            QC.build(QC.Data("B", "spread", 64, 128, 20, rows="plain"))
        monkeypatch.undo()
        monkeypatch.setattr(QC, "C_T", 2.0 ** -14)
        QC.build.cache_clear()
        QC.emulate.cache_clear()
        with pytest.raises(AssertionError, match="within their unit of a bf16 midpoint"):
            QC.emulate(QC._data_cases("B")[1])
    finally:
        monkeypatch.undo()
        QC.build.cache_clear()
        QC.emulate.cache_clear()


@pytest.mark.parametrize("kind", "AB")
def test_covering_list(kind):
    ls = QC.launches(kind)
    assert 45 <= len(ls) <= 70 and len(set(QC.launch_id(l) for l in ls)) == len(ls)
    for l in ls:
        d = l.data
        r = QC.route(d.M, d.N, d.Nq, d.Nk, l.cfg, l.split, l.keys16)
        assert r is not None and tuple(x[0] for x in r) == l.inst, QC.launch_id(l)
        assert sum(x[2] for x in r) == d.N and QC.forced_ok(d, l.cfg)
    epis = (2, 3, 4, 7)
    for cfg in (1, 2, 3, 4):
        for e in epis:
            for K in (64, 1280):
                assert any(l.cfg == cfg and l.data.K == K and l.inst[0] == QC.inst_name(cfg, e) for l in ls), (cfg, e, K)
        assert any(l.cfg == cfg and l.data.dup for l in ls)
        assert any(l.cfg == cfg and l.data.Nk == 77 and l.keys16 == 0 and l.inst[0] == QC.inst_name(cfg, 4) for l in ls)
        if kind == "B":
            for rows in ("plain", "offset"):
                assert any(l.cfg == cfg and l.data.rows == rows for l in ls)
    for N in (128, 384, 640):
        for cfg in (1, 4):
            assert any(l.cfg == cfg and l.data.N == N for l in ls)
        if N > 256:
            assert {l.split for l in ls if l.data.N == N and l.cfg == 1} == {0, 1}
    assert {l.data.K for l in ls} == {64, 192, 640, 1280}
    assert {l.cfg for l in ls if l.data.Nq == 384} == {2, 3}
    if kind == "B":
        assert any(l.data.free_wsum for l in ls) and {l.data.parts for l in ls} >= {1, 5, 10}
    # the restated dispatch falls back where a forced tile cannot run, so such a launch could not carry that tile's name
    assert QC.route(768, 128, 384, 96, 1)[0][0] == QC.inst_name(2, 4) and QC.route(768, 128, 384, 96, 4)[0][0] == QC.inst_name(2, 4)
