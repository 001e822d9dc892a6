"""The thin kernels around the GEMM core on exact inputs, bit for bit against float64 (`-m gpu`): cd360_out_conv4_bf16,
cd360_unet_stage_in, cd360_vae_conv_in_f32 with its slab statistics, cd360_vae_conv_out_bf16 / _u8, cd360_vae_enc_conv_out_bf16,
cd360_rowdot1 / 4_bf16 (several rows per wave), cd360_rowdot4_bwd_bf16, cd360_concat_channels_bf16 and the GEGLU pair past their grid caps.

The cases of tests/thin_cases.py: small-integer operands (or integers times one power of two), so every product and every partial sum
is exact in the fp32 accumulators on any schedule; an fp32 output has one right value, a bf16 output one rounding with one right answer,
the uint8 image one truncation of an exact value.  The assertions are torch.equal -- one wrong tap, halo, chunk, slice, slab or row
changes bits (tests/test_thin_cases_cpu.py holds every case to that).  Every launch runs twice and must give identical bits; outputs
the wrapper takes from the caller are pre-filled (NaN, or two different byte patterns for the uint8 image), so an element left unwritten
shows.  The two places without bit equality: GEGLU (an erf, an exp) is held to the band [bf16(want - delta), bf16(want + delta)] of
thin_cases (c = 10.5; measured on an MI355X: 0.12 of delta at the worst, see the tests), and emb_act (an exp) to one bf16 spacing of the float64 reference."""
import pytest
import torch

import thin_cases as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
F32 = torch.float32
INT_OF = {BF: torch.int16, F32: torch.int32, torch.uint8: torch.uint8, torch.int16: torch.int16}


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(INT_OF[a.dtype]), b.contiguous().view(INT_OF[b.dtype]))


def describe(got, want):
    """Count, first indices, got and want (the cause is to be found from one run)."""
    g, w = got.double().cpu(), want.double().cpu()
    if g.shape != w.shape:
        return f"shape {tuple(g.shape)}, want {tuple(w.shape)}"
    ne = (g != w).nonzero()
    first = [(tuple(i.tolist()), g[tuple(i)].item(), w[tuple(i)].item()) for i in ne[:4]]
    last = tuple(ne[-1].tolist()) if ne.shape[0] else ()
    return f"{ne.shape[0]} of {g.numel()} differ, first (index, got, want) {first}, last index {last}"


def check(bad, tag, runs, want):
    """runs: the outputs of two launches; want on the device in the output's dtype."""
    if not torch.equal(runs[0], want):
        bad.append(f"{tag}: {describe(runs[0], want)}")
    if not same_bits(runs[0], runs[1]):
        bad.append(f"{tag}: repeated launches differ")


def finish(bad):
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:12])


def rows_of(t):
    """[B, H, W, C] -> [B, H W, C] (channels-last rows, as the kernels take and write them)"""
    return t.reshape(t.shape[0], -1, t.shape[-1])


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("cin", T.OUT_CONV4_CIN)
def test_out_conv4_bit_equal(cin):
    """ops.out_conv4: one, two, three and five K chunks of the LDS-DMA ring, one band and interior bands, W = 32 / 64 / 128, one image
    and three with distinct data -- bit-equal to RNE(float64)."""
    from cd360 import ops
    bad = []
    for key in [k for k in T.out_conv4_cases() if k[3] == cin]:
        n, H, W, _ = key
        c = T.out_conv4_case(*key)
        x, bias = rows_of(c.x).to(DEV, BF), c.bias.to(DEV, F32)
        w36 = ops.pack_out_conv4_weight(c.w.to(DEV, F32))
        assert ops.out_conv4_ok(H, W, cin)
        runs = [ops.out_conv4(x, w36, bias, n, H, W) for _ in range(2)]
        check(bad, f"{key}", runs, rows_of(c.want).to(DEV))
    finish(bad)


def launch_stage(ops, c, e):
    """One cd360_unet_stage_in launch of the conv case c and the emb case e into NaN-filled outputs -> (h, emb_act)."""
    bs, H, W, _ = c.x.shape
    rep, cout = c.extra["rep"], c.w.shape[0]
    h = torch.full((rep * bs, H * W, cout), T.NAN, dtype=BF, device=DEV)
    emb = torch.full((rep * bs, e.E), T.NAN, dtype=BF, device=DEV)
    return ops.unet_stage_in(nchw(c.extra["lat"]).to(DEV, F32), c.extra["tab"].to(DEV, F32), torch.tensor([c.extra["idx"]], dtype=torch.int32, device=DEV),
                             c.w.permute(2, 3, 1, 0).reshape(36, cout).contiguous().to(DEV, F32), c.bias.to(DEV, F32), e.temb.to(DEV, BF),
                             e.lab.to(DEV, BF), h, emb)


@pytest.mark.parametrize("cout", T.STAGE_COUT)
@pytest.mark.parametrize("kind", list(T.STAGE_TABLES))
def test_stage_in_convolution_bit_equal(kind, cout):
    """ops.unet_stage_in: less than a 64-pixel tile, one tile, a ragged second, two tiles, a third of two pixels; c_in from step row 1 or
    2 of three; c_in x exact in bf16 (`exact`) or rounding (`round`: the convolution of the rounded values is still exact); EVERY one of
    the rep branch copies equals the expected rows."""
    from cd360 import ops
    bad = []
    for key in [k for k in T.stage_in_cases() if k[0] == kind and k[3] == cout]:
        _, bs, rep, _, H, W = key
        c = T.stage_in_case(*key)
        e = T.emb_case(bs, rep, 64)
        want = rows_of(c.want).to(DEV)
        runs = [launch_stage(ops, c, e)[0] for _ in range(2)]
        for r in range(rep):
            if not torch.equal(runs[0][r * bs:(r + 1) * bs], want):
                bad.append(f"{key} branch copy {r}: {describe(runs[0][r * bs:(r + 1) * bs], want)}")
        if not same_bits(runs[0], runs[1]):
            bad.append(f"{key}: repeated launches differ")
    finish(bad)


@pytest.mark.parametrize("E", T.STAGE_E)
def test_stage_in_emb_act_within_one_bf16_spacing(E):
    """emb_act = bf16(silu(bf16(temb[step] + lab[row]))): every row of rep x bs within one bf16 spacing of the float64 reference on the
    rounded sum (the fp32 evaluation error is far below half a spacing, so only the reference's two bf16 neighbours qualify)."""
    from cd360 import ops
    bad = []
    for bs, rep, _ in [k for k in T.emb_cases() if k[2] == E]:
        e = T.emb_case(bs, rep, E)
        c = T.stage_in_case(*T.emb_launch(bs, rep))
        assert c.extra["idx"] == e.idx
        runs = [launch_stage(ops, c, e)[1] for _ in range(2)]
        ok = T.emb_accepts(e, runs[0])
        if not bool(ok.all()):
            i = tuple((~ok).nonzero()[0].tolist())
            bad.append(f"bs={bs} rep={rep}: {int((~ok).sum())} of {ok.numel()} beyond one spacing, first {i}: got {runs[0][i].item()!r} want {e.want[i].item()!r}")
        if not same_bits(runs[0], runs[1]):
            bad.append(f"bs={bs} rep={rep}: repeated launches differ")
    finish(bad)


@pytest.mark.parametrize("cout", T.VAE_IN_COUT)
def test_vae_conv_in_and_slab_statistics_bit_equal(cout):
    """ops.vae_conv_in: 391 pixels (a ragged 7-pixel slab), one slab, three slabs; Cz = 4 and 8; the bf16 output bit-equal to
    RNE(float64), and where H W % 64 == 0 the statistics torch.equal to the float64 (sum, sum of squares) of the ROUNDED outputs per slab."""
    from cd360 import ops
    bad = []
    for key in [k for k in T.vae_conv_in_cases() if k[2] == cout]:
        c = T.vae_conv_in_case(*key)
        z, bias = nchw(c.x).to(DEV, F32), c.bias.to(DEV, F32)
        wp = ops.pack_vae_conv_in_weight(c.w.to(DEV, F32))
        stats = c.extra["stats"]
        runs = [ops.vae_conv_in(z, wp, bias, want_stats=stats) for _ in range(2)]
        check(bad, f"{key}", [r[0] if stats else r for r in runs], rows_of(c.want).to(DEV))
        if stats:
            check(bad, f"{key} statistics", [r[1] for r in runs], T.pixel_slab_stats(c.want).to(DEV, F32))
    finish(bad)


@pytest.mark.parametrize("cin", T.VAE_OUT_CIN)
def test_vae_conv_out_f32_bit_equal(cin):
    """ops.vae_conv_out: one channel chunk of the LDS, a tail chunk of 64 behind a full one (Cin = 320), two full chunks; 5 pixels, one
    256-pixel block, a ragged second block; Cout = 3 and 4 -- the fp32 output torch.equal to the float64 convolution."""
    from cd360 import ops
    bad = []
    for key in [k for k in T.vae_conv_out_cases() if k[2] == cin]:
        B, cout, _, H, W = key
        c = T.vae_conv_out_case(*key)
        wp = ops.pack_vae_conv_out_weight(c.w.to(DEV, F32))
        runs = [ops.vae_conv_out(rows_of(c.x).to(DEV, BF), wp, c.bias.to(DEV, F32), B, H, W, cout) for _ in range(2)]
        check(bad, f"{key}", runs, nchw(c.want).to(DEV, F32))
    finish(bad)


@pytest.mark.parametrize("cin", T.VAE_OUT_CIN)
def test_vae_conv_out_u8_against_float64(cin):
    """ops.vae_conv_out_u8 held to float64 alone, not to cd360_vae_conv_out_bf16 (both run the same accumulation): x integers, w and bias
    multiples of 1 / 256, so f and clip(f 0.5 + 0.5, 0, 1) 255 are exact in fp32 and the truncation to a byte has one right answer.  The
    output is pre-filled with 0x5a, then with 0xa5: a byte left unwritten differs from `want` in one of the two."""
    from cd360 import ops
    bad = []
    for key in [k for k in T.vae_conv_out_cases() if k[2] == cin]:
        B, cout, _, H, W = key
        c = T.vae_conv_out_case(*key, u8=True)
        wp = ops.pack_vae_conv_out_weight(c.w.to(DEV, F32))
        runs = []
        for fill in (0x5A, 0xA5):
            out = torch.full((B, H, W, cout), fill, dtype=torch.uint8, device=DEV)
            got = ops.vae_conv_out_u8(rows_of(c.x).to(DEV, BF), wp, c.bias.to(DEV, F32), B, H, W, cout, out=out)
            assert got.data_ptr() == out.data_ptr()
            runs.append(got)
        check(bad, f"{key}", runs, c.want.to(DEV))
    finish(bad)


@pytest.mark.parametrize("cin", T.ENC_OUT_CIN)
def test_vae_enc_conv_out_bit_equal(cin):
    """ops.vae_enc_conv_out: 72 units over the 16 K slices (uneven), one chunk of 128, 128 + 64, four chunks; 3 pixels, one 16-pixel block,
    a ragged 25th; Cout = 5 and 8 -- the fp32 output torch.equal to the float64 convolution."""
    from cd360 import ops
    bad = []
    for key in [k for k in T.enc_conv_out_cases() if k[2] == cin]:
        B, cout, _, H, W = key
        c = T.enc_conv_out_case(*key)
        wp = ops.pack_vae_enc_conv_out_weight(c.w.to(DEV, F32))
        runs = [ops.vae_enc_conv_out(rows_of(c.x).to(DEV, BF), wp, c.bias.to(DEV, F32), B, H, W, cout) for _ in range(2)]
        check(bad, f"{key}", runs, nchw(c.want).to(DEV, F32))
    finish(bad)


@pytest.mark.parametrize("shapes", ["small", "multi-row"])
@pytest.mark.parametrize("nw", [1, 4])
def test_rowdot_bit_equal(nw, shapes):
    """ops.rowdot1 / rowdot4.  small: every number of 512-channel chunks, ragged last chunks, one row and 37.  multi-row: 3072 rows (one
    per wave), 3073 (one wave takes a second row: the prefetch hand-over vn -> v) and 6149 (two rows for every wave, a third for five) --
    the fp32 output torch.equal to the float64 product."""
    from cd360 import ops
    bad = []
    for rows, C in (T.ROWDOT_SMALL if shapes == "small" else T.ROWDOT_MULTI):
        c = T.rowdot_case(nw, rows, C)
        h = c.h.to(DEV, BF)
        if nw == 4:
            runs, want = [ops.rowdot4(h, c.w.to(DEV, F32)) for _ in range(2)], c.out
        else:
            runs, want = [ops.rowdot1(h, c.w[0].contiguous().to(DEV, F32)) for _ in range(2)], c.out[:, 0]
        check(bad, f"rowdot{nw} {rows}x{C}", runs, want.to(DEV, F32))
    finish(bad)


def run_rowdot_bwd(ops, bad, rows, C, amp):
    c = T.rowdot_bwd_case(rows, C, amp)
    d, h, w = c.d.to(DEV, F32), c.h.to(DEV, BF), c.w.to(DEV, F32)
    runs = [ops.rowdot4_bwd(d, h, w) for _ in range(2)]
    check(bad, f"{rows}x{C} |d|<={amp} dh", [r[0] for r in runs], c.dh.to(DEV))
    check(bad, f"{rows}x{C} |d|<={amp} dw", [r[1] for r in runs], c.dw.to(DEV, F32))
    dh, dw = ops.rowdot4_bwd(d, h, w, need_dh=False)
    if dh is not None or not torch.equal(dw, c.dw.to(DEV, F32)):
        bad.append(f"{rows}x{C} need_dh=False: {'dh returned' if dh is not None else describe(dw, c.dw)}")
    dh, dw = ops.rowdot4_bwd(d, h, w, need_dw=False)
    if dw is not None or not torch.equal(dh, c.dh.to(DEV)):
        bad.append(f"{rows}x{C} need_dw=False: {'dw returned' if dw is not None else describe(dh, c.dh)}")


@pytest.mark.parametrize("C", sorted({C for _, C in T.ROWDOT_BWD}))
def test_rowdot4_bwd_bit_equal(C):
    """ops.rowdot4_bwd: one row, 255 / 256 / 257 (one slab short, full, one row over) and 1000 rows: dh bit-equal to RNE of the exact
    sum_j d_j w_jc, dw torch.equal to the float64 product; need_dh=False and need_dw=False give the same.  d in [-16, 16] and in
    [-32, 32] (on the wider range at least 15 % of dh rounds and 5 % are ties)."""
    from cd360 import ops
    bad = []
    for rows in sorted({r for r, _ in T.ROWDOT_BWD}):
        for amp in T.ROWDOT_BWD_D:
            run_rowdot_bwd(ops, bad, rows, C, amp)
    finish(bad)


@pytest.mark.parametrize("amp", T.ROWDOT_BWD_D)
def test_rowdot4_bwd_beyond_the_dh_grid_cap(amp):
    """16,400 rows x 1024 channels = 2,099,200 vectors, above the 8192 x 256 threads of the dh grid: the second trip of its grid-stride loop."""
    from cd360 import ops
    bad = []
    run_rowdot_bwd(ops, bad, *T.ROWDOT_BWD_BIG, amp)
    finish(bad)


@pytest.mark.parametrize("ca,cb,pixels", T.CONCAT_SMALL + [T.CONCAT_BIG], ids=[f"{a}+{b}x{p}" for a, b, p in T.CONCAT_SMALL + [T.CONCAT_BIG]])
def test_concat_channels_bit_equal(ca, cb, pixels):
    """ops.concat_channels on inputs whose every 16-byte vector is distinct (within and across the two): a copy from the wrong place
    changes bits.  (320, 640) x 8,750 pixels is 1,050,000 vectors: past the 4096-workgroup cap, the loop's second trip."""
    from cd360 import ops
    a, b, want = T.concat_case(ca, cb, pixels)
    as_image = lambda t: t.to(DEV).view(BF).reshape(1, pixels, 1, -1).permute(0, 3, 1, 2)  # [1, C, pixels, 1], channels last in memory
    runs = [ops.concat_channels(as_image(a), as_image(b)).permute(0, 2, 3, 1).reshape(pixels, ca + cb).contiguous().view(torch.int16) for _ in range(2)]
    bad = []
    check(bad, f"{ca}+{cb} x {pixels}", runs, want.to(DEV))
    finish(bad)


def geglu_check(bad, tag, got, want, scale):
    """-> worst error / delta of this output; a failure line into `bad` if an element is outside its band."""
    want, scale = want.to(DEV), scale.to(DEV)
    ok = T.band_accepts(got, want, scale)
    ratio = T.band_error(got, want, scale)
    if not bool(ok.all()):
        i = tuple((~ok).nonzero()[0].tolist())
        bad.append(f"{tag}: {int((~ok).sum())} of {ok.numel()} outside the band, error / delta {ratio:.3g}, first {i}: got {got[i].item()!r} "
                   f"want {want[i].item()!r} scale {scale[i].item()!r}")
    return ratio


GEGLU = T.GEGLU_SMALL + [T.GEGLU_BIG]


@pytest.mark.parametrize("rows,inner", GEGLU, ids=[f"{r}x{i}" for r, i in GEGLU])
def test_geglu_within_the_band(rows, inner):
    """ops.geglu: y = x gelu(g) with the gate grid -8 .. 8 among the gates, every element in [bf16(want - delta), bf16(want + delta)],
    delta = 10.5 x 2^-24 |x| max(|g|, 1) (thin_cases.GEGLU_C).  4100 x 2048 is 1,049,600 vectors: the second trip of the grid-stride loop.
    Measured on an MI355X, worst error / delta: 0.0016, 0.017, 0.017, 0.061, 0.061 over the five cases, no element outside its band.
    The test prints it (THIN-EXACT geglu ...)."""
    from cd360 import ops
    c = T.geglu_case(rows, inner)
    want, scale = T.geglu_reference(c)["y"]
    proj = c.proj.to(DEV, BF)
    runs = [ops.geglu(proj) for _ in range(2)]
    bad = []
    worst = geglu_check(bad, f"{rows}x{inner} y", runs[0], want, scale)
    if not same_bits(runs[0], runs[1]):
        bad.append("repeated launches differ")
    print(f"THIN-EXACT geglu {rows}x{inner}: worst error / delta = {worst:.4f}")
    finish(bad)


@pytest.mark.parametrize("rows,inner", GEGLU, ids=[f"{r}x{i}" for r, i in GEGLU])
def test_geglu_bwd_within_the_band(rows, inner):
    """ops.geglu_bwd: dx = dy gelu(g) and dg = dy x gelu'(g), each element in its band (delta = 10.5 x 2^-24 |dy| max(|g|, 1) and
    10.5 x 2^-24 |dy||x| max(|g|, 1)); the large case takes the loop's second trip.  Measured on an MI355X, worst error / delta: dx 0.061, dg 0.123 (both at
    4100 x 2048), no element outside its band.  Prints the worst error / delta per output (THIN-EXACT geglu_bwd ...)."""
    from cd360 import ops
    c = T.geglu_case(rows, inner)
    ref = T.geglu_reference(c)
    proj, dy = c.proj.to(DEV, BF), c.dy.to(DEV, BF)
    runs = [ops.geglu_bwd(proj, dy) for _ in range(2)]
    bad = []
    worst = {k: geglu_check(bad, f"{rows}x{inner} {k}", got.contiguous(), *ref[k]) for k, got in (("dx", runs[0][:, :inner]), ("dg", runs[0][:, inner:]))}
    if not same_bits(runs[0], runs[1]):
        bad.append("repeated launches differ")
    print(f"THIN-EXACT geglu_bwd {rows}x{inner}: worst error / delta dx = {worst['dx']:.4f}, dg = {worst['dg']:.4f}")
    finish(bad)
