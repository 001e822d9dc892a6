"""The exact cases of tests/thin_cases.py, validated without a GPU: every case tests/test_thin_exact_gpu.py builds meets the conditions its
exactness rests on (operands representable, every partial sum below 2^24, statistics of the stored values below 2^24), meets the
rounding floors where the output is bf16 (15 % of the outputs round, 5 % are exact ties), and changes at least one output bit under
EVERY defect of its family's fault model -- a dropped tap, a column shift that wraps into the neighbouring row, a missing or foreign
halo row, a K chunk dropped or doubled, a zero tile-edge column, c_in from the wrong row, an omitted rounding, an unwritten branch copy,
a skipped ragged block, statistics of unrounded values or of the neighbouring slab, a K slice left out of the LDS sum, a skipped tail
chunk, channels >= Cout written, a wave's second row stale or skipped, a read past C, elements beyond the first grid trip, truncation,
a shifted bias slice.  Where a defect is tied to a position the changed elements must include it.  So a bit-equal GPU result says
something, and a case list that drifts (a shape shrunk until a path is no longer taken) is caught here, not on the GPU."""
import pytest
import torch

import thin_cases as T
from gemm_cases import rounding_shares


def hold(want, faults, need=()):
    """Every (name, bad, where) changes an output, at `where` if given; the names in `need` are among them."""
    names = []
    for name, bad, where in faults:
        d = T.differs(bad, want)
        assert bool(d.any()), f"{name} changes no output bit"
        assert where is None or bool((d & where).any()), f"{name} changes nothing at its position"
        names.append(name)
    missing = [n for n in need if not any(m.startswith(n) for m in names)]
    assert not missing, f"faults that should apply but were not generated: {missing}"
    return names


def floors(pre):
    inexact, ties, _ = rounding_shares(pre)
    assert inexact >= T.MIN_INEXACT and ties >= T.MIN_TIES, (inexact, ties)


def ids(cases):
    return ["-".join(str(v) for v in k) for k in cases]


def test_issue_reference_figures():
    """The figures the case ranges were chosen by: out_conv4 at Cin = 320 stays below a bound of 92,224 (= 9 x 320 x 8 x 4 + 64); the
    uint8 family at Cin = 128 on 17 x 23 shows most byte values with both ends of the clip; a 64-pixel slab of vae_conv_in at Cz = 4
    keeps sum v^2 below 2^24."""
    c = T.out_conv4_case(3, 6, 128, 320)
    assert T.conv_bound(c.x, c.w, c.bias) <= 92224
    g = torch.Generator().manual_seed(5)
    x, w, b = T._ints(g, (2, 17, 23, 128), 4), T._ints(g, (4, 128, 3, 3), 4) / 256, T._ints(g, (4,), 64) / 256
    by = T.image_bytes(T.conv3x3(x, w) + b)
    share0, share255 = (by == 0).double().mean().item(), (by == 255).double().mean().item()
    print(f"THIN-CASES u8 Cin=128 17x23: {by.unique().numel()} byte values, {share0:.3f} at 0, {share255:.3f} at 255")
    assert by.unique().numel() >= 200 and share0 > 0.02 and share255 > 0.02
    c = T.vae_conv_in_case(1, 4, 512, 8, 8)
    v = c.want.double().reshape(1, 1, 64, 512)
    print(f"THIN-CASES vae_conv_in Cz=4: worst slab sum v^2 {(v * v).sum(2).max().item():.3g}")


def test_bf16_of_rounds_once():
    x = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -30, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -257.0, 0.0, 1e-20], dtype=torch.float64)
    assert T.bf16_of(x).double().tolist()[:5] == [1.0 + 2.0 ** -7, 1.0, 1.0 + 2.0 ** -6, -256.0, 0.0]
    assert x.to(T.BF).double()[0].item() == 1.0  # (the cast through fp32 loses the 2^-30 and then takes the tie to even)


def test_tap_terms_against_torch_conv2d():
    g = torch.Generator().manual_seed(1)
    x, w = T._ints(g, (2, 5, 7, 6), 8), T._ints(g, (3, 6, 3, 3), 4)
    ref = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1)
    assert torch.equal(T.conv3x3(x, w), ref)
    # the wrapped forms differ from the right one exactly at the border they name
    d = (T.tap_terms(x, w, wrap_cols=True) != T.tap_terms(x, w)).any(0).any(-1)
    assert bool(d[:, :, 0].any()) and bool(d[:, :, -1].any()) and not bool(d[:, :, 1:-1].any())
    d = (T.tap_terms(x, w, wrap_rows=True) != T.tap_terms(x, w)).any(0).any(-1)
    assert bool(d[1, 0].any()) and bool(d[0, -1].any()) and not bool(d[:, 1:-1].any()) and not bool(d[0, 0].any()) and not bool(d[1, -1].any())


@pytest.mark.parametrize("key", T.out_conv4_cases(), ids=ids(T.out_conv4_cases()))
def test_out_conv4_case(key):
    images, H, W, cin = key
    c = T.out_conv4_case(*key)
    T.check_out_conv4(c)
    floors(c.pre)
    need = ["tap-8-partial", "truncation", "bias-slice", "column-shift-wraps-at-x=0", "column-shift-wraps-at-x=W-1"]
    need += [f"k-chunk-{i}-dropped" for i in range(cin // 64)] + [f"k-chunk-{i}-added-twice" for i in range(cin // 64)]
    need += ["upper-halo-row-missing", "lower-halo-row-missing"] if H > 2 else []
    need += ["first-band-halo-from", "last-band-halo-from"] if images > 1 else []
    names = hold(c.want, T.out_conv4_faults(c), need)
    assert sum(n.startswith("tap-") and n.endswith("-dropped") for n in names) == 10


def test_out_conv4_case_list_reaches_every_ring_path():
    chunks = {cin // 64 for _, _, _, cin in T.out_conv4_cases()}
    assert {1, 2, 3} <= chunks and max(chunks) >= 5        # a single issue; both stages, no re-issue; issue(c + 2); several re-issues
    assert {W for _, _, W, _ in T.out_conv4_cases()} == {32, 64, 128} and {1, 3} == {n for n, _, _, _ in T.out_conv4_cases()}
    assert any(H == 2 for _, H, _, _ in T.out_conv4_cases()) and any(H > 4 for _, H, _, _ in T.out_conv4_cases())  # one band; interior bands


@pytest.mark.parametrize("key", T.stage_in_cases(), ids=ids(T.stage_in_cases()))
def test_stage_in_case(key):
    kind, bs, rep, cout, H, W = key
    c = T.stage_in_case(*key)
    T.check_stage_in(c)
    floors(c.pre)
    need = ["truncation", "bias-slice-shifted-8", "c_in-from-row-0", "upper-halo-row-missing", "lower-halo-row-missing", "column-shift-wraps"]
    need += [f"branch-copy-{r}-not-written" for r in range(1, rep)]
    need += ["bf16-rounding-of-c_in-x-omitted"] if kind == "round" else []
    need += ["tile-edge-halo-column-zero-at-x=64"] if W > 64 else []
    need += ["tile-edge-halo-column-zero-at-x=128"] if W > 128 else []
    need += ["ragged-last-tile-skipped"] if W % 64 else []
    need += ["first-band-halo-from", "last-band-halo-from"] if bs > 1 else []
    hold(T.stage_full(c, c.want), T.stage_in_faults(c), need)


def test_stage_in_case_list_covers_the_tile_geometry():
    ws = {W for *_, W in T.stage_in_cases()}
    assert any(W < 64 for W in ws) and 64 in ws and 128 in ws and any(64 < W < 128 for W in ws) and any(0 < W - 128 < 8 for W in ws)
    assert {T.stage_in_case(*k).extra["idx"] for k in T.stage_in_cases()} == {1, 2}


@pytest.mark.parametrize("key", T.emb_cases(), ids=ids(T.emb_cases()))
def test_emb_case_and_bar(key):
    c = T.emb_case(*key)
    assert T.is_bf16(c.temb) and T.is_bf16(c.lab) and T.is_bf16(c.ssum) and c.idx in (1, 2)
    assert (c.ssum != c.temb[c.idx] + c.lab).double().mean().item() > 0.2   # the sum rounds
    assert bool(T.emb_accepts(c, c.want.to(T.BF)).all())
    # an fp32 evaluation with the kernel's formula lands inside the bar, both bf16 neighbours of the reference do, the next ones do not
    s = c.ssum.float()
    assert bool(T.emb_accepts(c, (s / (1 + torch.exp(-s))).to(T.BF)).all())
    near = c.want.to(T.BF).double()
    other = torch.where(near > c.want, near - T.bf16_spacing(near), near + T.bf16_spacing(near))
    m, e = torch.frexp(near)
    live = (c.want.abs() > 1e-30) & (near != c.want) & (m.abs() != 0.5) & (e == torch.frexp(c.want)[1])  # (away from a change of spacing)
    assert bool(T.emb_accepts(c, other)[live].all())
    far = torch.where(near > c.want, near + 2 * T.bf16_spacing(near), near - 2 * T.bf16_spacing(near))
    assert not bool(T.emb_accepts(c, far)[live].any())
    for name, bad in T.emb_faults(c):
        assert not bool(T.emb_accepts(c, bad).all()), f"{name} is accepted"


@pytest.mark.parametrize("key", T.vae_conv_in_cases(), ids=ids(T.vae_conv_in_cases()))
def test_vae_conv_in_case(key):
    B, cz, cout, H, W = key
    c = T.vae_conv_in_case(*key)
    T.check_vae_conv_in(c)
    floors(c.pre)
    assert c.extra["stats"] == ((H * W) % 64 == 0)
    need = ["truncation", "bias-slice-shifted-2", "column-shift-wraps"] + (["ragged-last-pixel-block-skipped"] if (H * W) % 64 else [])
    hold(c.want, T.vae_conv_in_faults(c), need)
    if c.extra["stats"]:
        right = T.pixel_slab_stats(c.want)
        T.exact_f32(right)
        names = hold(right, T.vae_conv_in_stats_faults(c), ["statistics-of-the-unrounded-values"])
        assert ("statistics-slabs-shifted-by-one" in names) == (H * W > 64)
        # every slab holds an output that rounded: each slab's statistics tell stored from unrounded values
        pre_stats = T.pixel_slab_stats(c.pre)
        assert all(not torch.equal(right[b, s], pre_stats[b, s]) for b in range(B) for s in range(right.shape[1]))


def test_vae_conv_in_case_list():
    hw = {H * W for *_, H, W in T.vae_conv_in_cases()}
    assert 391 in hw and 64 in hw and any(p % 64 == 0 and p > 64 for p in hw)  # a ragged 7-pixel slab; one slab; several slabs with statistics


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("key", T.vae_conv_out_cases(), ids=ids(T.vae_conv_out_cases()))
def test_vae_conv_out_case(key, u8):
    B, cout, cin, H, W = key
    c = T.vae_conv_out_case(*key, u8=u8)
    T.check_vae_conv_out(c)
    need = [f"k-chunk-{i}" for i in range(-(-cin // 256))] + (["ragged-last-pixel-block-skipped"] if (H * W) % 256 else [])
    need += ["k-chunk-1-the-tail-dropped"] if cin == 320 else []
    need += ["output-channels->=Cout-written"] if cout < 4 and (u8 or B > 1) else []
    need += ["column-shift-wraps"] if H > 1 else []
    hold(c.want, T.vae_conv_out_faults(c), need)


@pytest.mark.parametrize("key", T.enc_conv_out_cases(), ids=ids(T.enc_conv_out_cases()))
def test_enc_conv_out_case(key):
    B, cout, cin, H, W = key
    c = T.enc_conv_out_case(*key)
    T.check_conv(c, "bf16", "f32")
    need = [f"k-chunk-{i}" for i in range(-(-cin // 128))] + [f"k-slice-{s}-left-out" for s in (0, 7, 15)]
    need += ["k-chunk-1-the-tail-dropped"] if cin == 192 else []
    need += ["ragged-last-pixel-block-skipped"] if (H * W) % 16 else []
    need += ["output-channels->=Cout-written"] if cout < 8 and B > 1 else []
    hold(c.want, T.enc_conv_out_faults(c), need)
    # the slices of 16 partition the weight
    assert torch.equal(sum(T.slice_weight(c, s) for s in range(T.EO_SLICES)), c.w)


def test_enc_conv_out_slices_are_uneven_at_64_channels():
    c = T.enc_conv_out_case(1, 5, 64, 4, 4)   # 72 units over 16 slices: slices 0 .. 7 take five, the rest four
    counts = [int((T.slice_weight(c, s) != 0).any(0).sum().item()) // 8 for s in range(16)]
    assert sum(counts) <= 72 and max(counts) == 5 and min(counts) >= 3


ROWDOT = T.ROWDOT_SMALL + T.ROWDOT_MULTI


@pytest.mark.parametrize("nw", [1, 4])
@pytest.mark.parametrize("rows,C", ROWDOT, ids=[f"{r}x{c}" for r, c in ROWDOT])
def test_rowdot_case(nw, rows, C):
    c = T.rowdot_case(nw, rows, C)
    T.check_rowdot(c)
    nwaves = T.rowdot_waves(rows)
    need = ["last-8-channels-dropped"]
    need += ["second-row-reuses", "second-row-skipped"] if rows > nwaves else []
    need += ["third-row-sees"] if rows > 2 * nwaves else []
    need += ["lane-of-the-last-group-reads-past-C"] if C % 512 and nw == 4 and rows > 1 else []
    hold(c.out, T.rowdot_faults(c), need)


def test_rowdot_case_list_reaches_the_row_loop():
    assert T.rowdot_waves(37) == 40 and T.rowdot_waves(3072) == 3072 and T.rowdot_waves(10 ** 6) == 3072
    per_wave = {rows: -(-rows // T.rowdot_waves(rows)) for rows, _ in ROWDOT}
    assert per_wave[3072] == 1 and per_wave[3073] == 2 and per_wave[6149] == 3 and 6149 - 2 * 3072 < 3072  # a remainder: some waves take a third row
    assert {-(-C // 512) for _, C in ROWDOT} == {1, 2, 3, 4} and any(C % 512 for _, C in T.ROWDOT_MULTI)


BWD = T.ROWDOT_BWD + [T.ROWDOT_BWD_BIG]


@pytest.mark.parametrize("amp", T.ROWDOT_BWD_D)
@pytest.mark.parametrize("rows,C", BWD, ids=[f"{r}x{c}" for r, c in BWD])
def test_rowdot_bwd_case(rows, C, amp):
    """d in [-16, 16] cannot reach the floors (dh is a sum of four products): measured 4 .. 14 % of the outputs round.  Those cases are held
    to exactness and the fault models, the same shapes on d in [-32, 32] to the floors as well."""
    c = T.rowdot_bwd_case(rows, C, amp)
    T.check_rowdot_bwd(c)
    assert c.d.abs().max().item() <= amp
    if amp == 32:
        floors(c.dh_pre)
    names = []
    for name, which, bad, where in T.rowdot_bwd_faults(c):
        hold(c.dh if which == "dh" else c.dw, [(name, bad, where)])
        names.append(name)
    assert ("last-slab-skipped" in names) == (rows > 256) and ("elements-beyond-the-first-grid-trip-unwritten" in names) == ((rows, C) == T.ROWDOT_BWD_BIG)
    assert "truncation" in names or rows * C < T.ROWDOT_BWD_MIN_ROUNDING_OUTPUTS


CONCAT = T.CONCAT_SMALL + [T.CONCAT_BIG]


@pytest.mark.parametrize("ca,cb,pixels", CONCAT, ids=ids(CONCAT))
def test_concat_case(ca, cb, pixels):
    T.check_concat(ca, cb, pixels)
    _, _, want = T.concat_case(ca, cb, pixels)
    names = hold(want, T.concat_faults(ca, cb, pixels))
    assert ("elements-beyond-the-first-grid-trip-unwritten" in names) == ((ca, cb, pixels) == T.CONCAT_BIG)


def test_big_cases_pass_the_grid_caps():
    ca, cb, px = T.CONCAT_BIG
    assert px * (ca + cb) // 8 == 1_050_000 > T.GRID_VECTORS
    assert T.GEGLU_BIG[0] * T.GEGLU_BIG[1] // 8 == 1_049_600 > T.GRID_VECTORS
    assert T.ROWDOT_BWD_BIG[0] * T.ROWDOT_BWD_BIG[1] // 8 == 2_099_200 > T.DH_GRID_VECTORS
    assert all(r * i // 8 < T.GRID_VECTORS for r, i in T.GEGLU_SMALL) and all(p * (a + b) // 8 < T.GRID_VECTORS for a, b, p in T.CONCAT_SMALL)


GEGLU = T.GEGLU_SMALL + [T.GEGLU_BIG]


@pytest.mark.parametrize("rows,inner", GEGLU, ids=[f"{r}x{i}" for r, i in GEGLU])
def test_geglu_case_and_band_rule(rows, inner):
    c = T.geglu_case(rows, inner)
    T.check_geglu(c)
    ref = T.geglu_reference(c)
    # the yardstick: a plain fp32 evaluation on this host stays within half of c (c = 4 x the figure measured when the cases were made)
    units = T.fp32_error_units(c)
    print(f"THIN-CASES geglu {rows}x{inner}: fp32 CPU error in units of 2^-24 scale {units}")
    assert max(units.values()) <= T.GEGLU_C / 2 and abs(T.GEGLU_C - 4 * max(T.GEGLU_MEASURED.values())) < 0.05
    fp32 = T.geglu_fp32(c)
    for k, (want, scale) in ref.items():
        assert bool(T.band_accepts(T.bf16_of(want), want, scale).all()) and T.band_error(T.bf16_of(want), want, scale) == 0.0
        assert bool(T.band_accepts(fp32[k].to(T.BF), want, scale).all())
        assert T.band_error(fp32[k].to(T.BF), want, scale) <= 0.5
    names = set()
    for name, k, bad in T.geglu_faults(c):
        assert not bool(T.band_accepts(bad, *ref[k]).all()), f"{name} ({k}) is accepted"
        names.add(name)
    assert ("elements-beyond-the-first-grid-trip-unwritten" in names) == ((rows, inner) == T.GEGLU_BIG)


def test_case_counts():
    n = T.case_counts()
    print(f"THIN-CASES counts {n}, total {sum(n.values())}")
    assert n == dict(out_conv4=32, stage_in=80, emb_act=8, vae_conv_in=36, vae_conv_out=48, vae_conv_out_u8=48, vae_enc_conv_out=48, rowdot1=24,
                     rowdot4=24, rowdot4_bwd=42, concat_channels=4, geglu=5, geglu_bwd=5)
