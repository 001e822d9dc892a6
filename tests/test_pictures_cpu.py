"""Pictures in, without a GPU: the seventh library's header <=> table <=> exports, its build row, host-side refusals and resource record;
the tap tables of cd360.pictures against the rule restated in tests/picture_cases.py and against torch's antialiased interpolate; the
restatement with the two uint8 roundings against what the image library returns (tests/golden/pictures.npz, written by
tests/golden/make_picture_golden.py); the mask rule against that fixture and torch's nearest-exact; the crop boxes by hand; the
refusals of the Python layer."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import picture_cases as PC
import sampler_cases as SC
import textgrad_cases as TG
import train_cases as TR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TORCH_MODE = {"bilinear": "bilinear", "bicubic": "bicubic"}


# ================================================================================================ 1: header, table, library
def test_picture_header_matches_its_table_and_the_older_libraries_are_closed():
    """include/picture/cd360_picture.h <=> cd360._picture.PICTURE_SIGNATURES <=> libcd360_picture.so by the rule of
    sampler_cases._header_table_library, with all six older libraries closed to the new names.  The binding and the source read no
    environment, the source never synchronises and has no atomics; the two caps are one value in the header, the source and the binding."""
    from cd360 import _picture, _textgrad, _train, ops
    tables, headers, libs = TG.older_libraries()
    tables, libs = tables + [_textgrad.TEXTGRAD_SIGNATURES, _train.TRAIN_SIGNATURES], libs + [_textgrad.load(), _train.load()]
    headers = headers + [TG.HEADER, TR.HEADER]
    mismatch, in_tables, in_headers, mistyped, lib = SC._header_table_library(_picture.HEADER, _picture.PICTURE_SIGNATURES, PC.NEW, tables, headers,
                                                                              _picture.load())
    assert not mismatch, mismatch
    assert not in_tables, in_tables
    assert not in_headers, in_headers
    assert not mistyped, mistyped
    assert _picture.HEADER == PC.HEADER and all(n.startswith("cd360_picture_") for n in PC.NEW) and len(libs) == 6
    for older in libs:
        for name in PC.NEW:
            assert not hasattr(older, name), name
    src = open(_picture.__file__).read()
    assert "os.environ" not in src and "getenv" not in src
    hip = open(os.path.join(SC.ROOT, "custom-diffusion360_amd", "csrc_picture", "picture_stage.hip")).read()
    assert "getenv" not in hip and "Synchronize" not in hip and "atomic" not in hip
    for name, py in (("CD360_PICTURE_MAX_TAPS", (ops.PICTURE_MAX_TAPS, _picture.MAX_TAPS, PC.MAX_TAPS)),
                     ("CD360_PICTURE_MAX_DILATE", (ops.PICTURE_MAX_DILATE, _picture.MAX_DILATE, PC.MAX_DILATE))):
        value = SC.header_constant(PC.HEADER, name)
        assert all(v == value for v in py), name
        assert f"#define {name} {value}\n" in hip, name


def test_the_build_row_is_in_the_third_table_and_the_older_tables_are_unchanged():
    spec = importlib.util.spec_from_file_location("_graft_entry_for_pictures", os.path.join(SC.ROOT, "__graft_entry__.py"))
    entry = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(entry)
    assert PC.BUILD_ROW in [tuple(r) for r in entry.MORE_LIBRARIES]
    assert tuple(entry.LIBRARIES[-1]) == TG.BUILD_ROW and len(entry.LIBRARIES) == len(SC.LIBRARIES) + 1
    assert [r[3] for r in entry.LIBRARIES] == ["_lib", "_edit", "_optim", "_text", "_textgrad"]
    assert [tuple(r) for r in entry.LATER_LIBRARIES] == [TR.BUILD_ROW]
    assert entry.ALL_LIBRARIES == entry.LIBRARIES + entry.LATER_LIBRARIES + entry.MORE_LIBRARIES
    assert len({r[0] for r in entry.ALL_LIBRARIES}) == len(entry.ALL_LIBRARIES)


def test_every_picture_entry_point_has_a_guarded_case():
    from cd360 import _picture
    untyped, unknown, uncovered = SC.check_guarded_cover(PC.HEADER, _picture.PICTURE_SIGNATURES, PC.GUARDED)
    assert not untyped, untyped
    assert not unknown, unknown
    assert not uncovered, f"launching entry points without a guarded case: {sorted(uncovered)}"


def test_picture_kernels_are_recorded_without_scratch():
    """The record of picture_stage.o: every kernel is there, with zero scratch and no register spill."""
    rec = json.load(open(os.path.join(SC.ROOT, "custom-diffusion360_amd", "lib", "obj", "picture_stage.o.resources.json")))
    assert all(any(k in name for name in rec) for k in PC.KERNELS), sorted(rec)
    for name, r in rec.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)


# ================================================================================================ 2: refusals on the host
def test_picture_entry_points_refuse_bad_arguments_on_the_host():
    """Fabricated non-null pointers: every call below returns CD360_ERR_ARG (-1) or CD360_ERR_SHAPE (-2) before anything launches."""
    from cd360 import _picture
    lib = _picture.load()
    nul, P = ctypes.c_void_p(None), ctypes.c_void_p
    p = [P(0x10000000 * i) for i in range(1, 12)]
    odd = lambda q, by: P(q.value + by)
    # ---- cd360_picture_resample_u8
    names = ("src", "x_min", "x_size", "x_w", "y_min", "y_size", "y_w", "work", "out")

    def res(H=60, W=80, C=3, stride=240, left=-3, top=2, w=70, h=70, fill=0, x_taps=8, y_taps=8, oh=32, ow=32, rnd=1, div=255.0, mul=2.0, add=-1.0, **kw):
        a = dict(zip(names, p))
        a.update(kw)
        return lib.cd360_picture_resample_u8(a["src"], H, W, C, stride, left, top, w, h, fill, a["x_min"], a["x_size"], a["x_w"], x_taps, a["y_min"],
                                             a["y_size"], a["y_w"], y_taps, oh, ow, rnd, div, mul, add, a["work"], a["out"], nul)

    for name in names:
        assert res(**{name: nul}) == -1, name
        if name != "src":
            assert res(**{name: odd(dict(zip(names, p))[name], 2)}) == -1, name
    assert res(work=odd(p[7], 8)) == -1  # the work planes are read as 16-byte vectors
    assert res(C=2) == -1 and res(C=4) == -1 and res(C=0) == -1
    assert res(w=0) == -1 and res(h=0) == -1 and res(w=-5) == -1  # an empty crop
    assert res(H=0) == -1 and res(W=-1) == -1 and res(oh=0) == -1 and res(ow=0) == -1 and res(x_taps=0) == -1 and res(y_taps=-1) == -1
    assert res(stride=239) == -1 and res(fill=256) == -1 and res(fill=-1) == -1
    assert res(div=0.0) == -1 and res(div=float("nan")) == -1 and res(mul=float("inf")) == -1 and res(add=float("nan")) == -1
    assert res(out=p[0]) == -1 and res(work=p[0]) == -1 and res(out=P(p[7].value + 64)) == -1  # an output over an input
    assert res(x_taps=PC.MAX_TAPS + 1) == -2 and res(y_taps=PC.MAX_TAPS + 1) == -2
    assert res(H=1 << 16, stride=1 << 15, W=80) == -2 and res(H=3, stride=1 << 31) == -2  # the picture's offsets past 32 bits
    assert res(h=1 << 20, ow=1 << 10) == -2 and res(oh=1 << 15, ow=1 << 15) == -2  # the crop's, the result's
    assert res(left=(1 << 30) + 1) == -2 and res(top=-(1 << 30) - 1) == -2 and res(w=(1 << 30) + 1, ow=1) == -2
    # ---- cd360_picture_mask_u8
    names = ("src", "opacity", "mask", "inside")

    def msk(H=60, W=80, stride=80, thr=125, left=-3, top=2, w=70, h=70, oh=8, ow=8, k=7, **kw):
        a = dict(zip(names, p))
        a.update(kw)
        return lib.cd360_picture_mask_u8(a["src"], H, W, stride, thr, left, top, w, h, oh, ow, k, a["opacity"], a["mask"], a["inside"], nul)

    assert msk(src=nul) == -1 and msk(opacity=nul, mask=nul, inside=nul) == -1
    for name in names[1:]:
        assert msk(**{name: odd(dict(zip(names, p))[name], 2)}) == -1, name
    for k in (0, 2, 4, 6, -1, -3):
        assert msk(k=k) == -1, k
    assert msk(k=PC.MAX_DILATE + 2) == -2
    assert msk(w=0) == -1 and msk(h=-1) == -1 and msk(H=0) == -1 and msk(W=0) == -1 and msk(oh=0) == -1 and msk(ow=-2) == -1
    assert msk(stride=79) == -1 and msk(thr=256) == -1 and msk(thr=-1) == -1
    assert msk(mask=p[1]) == -1 and msk(inside=P(p[2].value + 4)) == -1 and msk(opacity=p[0]) == -1
    assert msk(H=1 << 16, stride=1 << 15) == -2 and msk(oh=1 << 16, ow=1 << 15) == -2 and msk(left=-(1 << 30) - 1) == -2


# ================================================================================================ 3: the tables against torch
def _float_picture(H, W, seed):
    return PC.picture(H, W, 0, seed, "noise").astype(np.float64) / 255.0


@pytest.mark.parametrize("kind", PC.KINDS)
@pytest.mark.parametrize("shape", PC.SHAPES, ids=[f"{h}x{w}-{oh}x{ow}" for (h, w), (oh, ow) in PC.SHAPES])
def test_tap_tables_against_torch(shape, kind):
    """cd360.pictures.taps is the rule of tests/picture_cases.py in fp32 bit for bit and picks the taps an fp64 table picks.  Resizing a
    noise picture with values in [0, 1] with the fp64 table equals F.interpolate(double, antialias=True) to 1e-13.  The fp32
    restatement's distance from that fp64 result is at most twice torch-fp32's own plus one ulp of the largest value: both are fp32 sums
    of the same terms in different orders.  The identity case returns the input bits.

    Measured, max |x - torch fp64| on values in [0, 1], as (fp64 restatement | fp32 restatement | torch fp32):
      37x53->8x8    bilinear 1.1e-16 | 1.15e-07 | 1.15e-07    bicubic 4.4e-16 | 1.90e-07 | 1.89e-07
      64x64->32x16  bilinear 2.2e-16 | 1.02e-07 | 1.00e-07    bicubic 2.2e-16 | 1.36e-07 | 1.19e-07
      19x23->40x31  bilinear 2.2e-16 | 1.01e-06 | 1.01e-06    bicubic 1.3e-15 | 1.04e-06 | 8.58e-07
      90x70->64x64  bilinear 2.2e-16 | 1.95e-07 | 1.75e-07    bicubic 7.8e-16 | 4.78e-07 | 5.56e-07
      16x16->16x16  0 | 2.95e-08 | 2.95e-08 for both: the rounding of the input itself
      5x7->3x2      bilinear 1.1e-16 | 7.58e-08 | 4.66e-08    bicubic 2.2e-16 | 9.32e-08 | 4.80e-08"""
    from cd360 import pictures
    (H, W), (oh, ow) = shape
    a = _float_picture(H, W, seed=H * 100 + W)
    t64 = F.interpolate(torch.from_numpy(a)[None, None], size=(oh, ow), mode=TORCH_MODE[kind], antialias=True, align_corners=False)[0, 0].numpy()
    t32 = F.interpolate(torch.from_numpy(a.astype(np.float32))[None, None], size=(oh, ow), mode=TORCH_MODE[kind], antialias=True,
                        align_corners=False)[0, 0].numpy()
    got = {}
    for n_in, n_out in ((W, ow), (H, oh)):
        mine, want, wide = pictures.taps(n_in, n_out, kind), PC.tap_table(n_in, n_out, kind, np.float32), PC.tap_table(n_in, n_out, kind, np.float64)
        assert all(m.dtype == w.dtype and np.array_equal(m, w) for m, w in zip(mine, want)), (n_in, n_out)
        assert np.array_equal(mine[0], wide[0]) and np.array_equal(mine[1], wide[1]), (n_in, n_out)
        assert pictures.taps(n_in, n_out, kind) is mine and mine[2].shape[1] <= PC.MAX_TAPS  # cached
        assert np.abs(mine[2].astype(np.float64).sum(1) - 1).max() < 1e-6 and (mine[1] >= 1).all() and (mine[0] + mine[1] <= n_in).all()
        got[n_in, n_out] = (mine, wide)
    r64 = PC.apply_taps(PC.apply_taps(a, got[W, ow][1], 1), got[H, oh][1], 0)
    r32 = PC.apply_taps(PC.apply_taps(a.astype(np.float32), got[W, ow][0], 1), got[H, oh][0], 0)
    assert r32.dtype == np.float32 and r64.dtype == np.float64
    d64, d32, dt = (float(np.abs(x.astype(np.float64) - t64).max()) for x in (r64, r32, t32))
    ulp = float(np.spacing(np.float32(np.abs(t64).max())))
    print(f"{H}x{W}->{oh}x{ow} {kind}: fp64 restatement {d64:.2e} | fp32 restatement {d32:.2e} | torch fp32 {dt:.2e} | ulp {ulp:.2e}")
    assert d64 <= 1e-13
    assert d32 <= 2 * dt + ulp, (d32, dt)
    if (H, W) == (oh, ow):
        assert np.array_equal(r32, a.astype(np.float32)) and np.array_equal(r64, a)


def test_tables_refuse_what_the_kernel_does_not_serve():
    from cd360 import pictures
    with pytest.raises(ValueError, match="taps"):
        pictures.taps(4000, 100, "bicubic")
    with pytest.raises(ValueError, match="kind"):
        pictures.taps(10, 10, "lanczos")
    with pytest.raises(ValueError):
        pictures.taps(0, 10)
    assert pictures.taps(992, 64, "bicubic")[2].shape[1] <= PC.MAX_TAPS  # down-scaling by 15.5


# ================================================================================================ 4: the image library's bits
@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLD, "pictures.npz")))


def test_the_rounded_restatement_is_the_image_library_within_one_level(gold):
    """tests/golden/pictures.npz: crop + resize(BICUBIC) of the image library on seeded pictures, windows leaving the picture, fill 0 and
    255, three channels and one.  The fp32 restatement with the two uint8 roundings, on cd360.pictures' tables: no value differs by more
    than one level, at most 1 % of a case's values differ at all, and the share is the one recorded when the fixture was written.
    Without the roundings the noise cases differ by several levels: the roundings are part of what is reproduced."""
    from cd360 import pictures
    tags = [str(t) for t in gold["pictures"]]
    assert {"leaves-noise", "tall-smooth", "up-noise", "wide-white"} <= set(tags)
    worst_unrounded = 0.0
    for tag in tags:
        src, window, fill, want = gold[f"{tag}.src"], tuple(int(v) for v in gold[f"{tag}.window"]), int(gold[f"{tag}.fill"]), gold[f"{tag}.out"]
        assert src.dtype == np.uint8 and max(src.shape[:2]) <= 128 and min(src.shape[:2]) <= 96 and want.shape[1] <= 64
        S = want.shape[0]
        xt, yt = pictures.taps(window[2], S, "bicubic"), pictures.taps(window[3], S, "bicubic")
        mine = PC.levels(src, window, xt, yt, fill)
        d = np.abs(mine.astype(np.int64) - want.astype(np.int64))
        share = float((d > 0).mean())
        print(f"{tag}: {int((d > 0).sum())} of {d.size} values differ, max {int(d.max())}, share {share:.5f} (recorded {float(gold[f'{tag}.share']):.5f})")
        assert d.max() <= 1 and share <= 0.01 and share == float(gold[f"{tag}.share"]), tag
        plain = np.moveaxis(PC.resample(src, window, xt, yt, fill, False, 1.0, 1.0, 0.0), 0, 2).reshape(want.shape)
        if "noise" in tag:
            worst_unrounded = max(worst_unrounded, float(np.abs(np.clip(np.floor(plain + 0.5), 0, 255) - want).max()))
    print(f"without the roundings, noise cases: up to {worst_unrounded:.0f} levels from the image library")
    assert worst_unrounded >= 2
    assert gold["leaves-noise.window"].tolist() == [-5, -9, 61, 61] and gold["tall-noise.window"].tolist() == [-8, 0, 80, 80]


def test_the_mask_rule_is_the_image_library_and_nearest_exact(gold):
    """A boolean picture is resized by the nearest rule floor((2 i + 1) n_in / (2 n_out)) whatever filter is asked for: the restatement of
    cd360_picture_mask_u8's opacity equals the fixture, and torch's mode="nearest-exact" on the cropped mask, with no differing pixel;
    inside is 1 exactly where the source pixel lies in the picture; mask is clamp(conv2d(opacity, ones(k, k), padding="same"), 0, 1)."""
    tags = [str(t) for t in gold["masks"]]
    assert "mask-100" in tags and gold["mask-100.src"].shape == (100, 100) and gold["mask-100.out"].shape == (64, 64)
    for tag in tags:
        src, window, want = gold[f"{tag}.src"], tuple(int(v) for v in gold[f"{tag}.window"]), gold[f"{tag}.out"]
        s = want.shape[0]
        for k in (1, 3, 7):
            opacity, mask, inside = PC.mask_maps(src, window, s, s, 125, k)
            assert np.array_equal(opacity, want.astype(np.float32)), tag
            cropped = torch.from_numpy(PC.crop((src > 125).astype(np.float32), window, 0))[None, None]
            assert torch.equal(F.interpolate(cropped, size=(s, s), mode="nearest-exact")[0, 0], torch.from_numpy(opacity)), tag
            ones = torch.from_numpy(PC.crop(np.ones(src.shape, np.float32), window, 0))[None, None]
            assert torch.equal(F.interpolate(ones, size=(s, s), mode="nearest-exact")[0, 0], torch.from_numpy(inside)), tag
            conv = torch.clamp(F.conv2d(torch.from_numpy(opacity)[None, None], torch.ones(1, 1, k, k), padding="same"), 0, 1)[0, 0]
            assert torch.equal(conv, torch.from_numpy(mask)), (tag, k)
        assert 0 < want.sum() < want.size


# ================================================================================================ 5: crop boxes, by hand
def test_boxes_are_the_loaders_square_boxes():
    """data_co3d.py:373-390 worked by hand.  _padded_bbox of a (w, h) picture: centre (rint(w / 2), rint(h / 2)) with halves to even, half
    side rint(max(w, h) / 2).  Wide 80 x 64: centre (40, 32), half 40 -> (0, -8, 80, 72).  Tall 64 x 80: (-8, 0, 72, 80).  53 x 37: centre
    (26, 18) (26.5 and 18.5 round to even), half 26 -> (0, -8, 52, 44).  _crop_bbox of (70, 10, 120, 50) in a 100 x 60 picture: centre
    (95, 30), half 25 -> (70, 5, 120, 55), 20 columns outside the picture.  Of (10.5, 3, 31, 40): centre (rint(20.75), rint(21.5)) = (21,
    22), half rint(18.5) = 18 -> (3, 4, 39, 40)."""
    from cd360.pictures import PictureFront
    got = PictureFront.boxes([(80, 64), (64, 80), (53, 37)])
    assert got.dtype == np.int64 and got.tolist() == [[0, -8, 80, 72], [-8, 0, 72, 80], [0, -8, 52, 44]]
    got = PictureFront.boxes([(100, 60), (64, 48), (80, 64)], [[70, 10, 120, 50], [10.5, 3, 31, 40], None])
    assert got.tolist() == [[70, 5, 120, 55], [3, 4, 39, 40], [0, -8, 80, 72]]
    assert PictureFront._windows(got, 3) == [(70, 5, 50, 50), (3, 4, 36, 36), (0, -8, 80, 80)]
    with pytest.raises(ValueError):
        PictureFront.boxes([(80, 64)], [None, None])
    with pytest.raises(ValueError):
        PictureFront.boxes([(0, 64)])


# ================================================================================================ 6: the Python layer's refusals
def test_the_python_layer_refuses_before_the_device():
    """ValueError from the arguments alone, Cd360Error for a CPU tensor that passes them: there is no fallback."""
    from cd360 import finetune, ops, pictures
    tabs = lambda n_in, n_out: tuple(torch.from_numpy(np.array(a)) for a in pictures.taps(n_in, n_out, "bicubic"))
    src, m = torch.zeros(40, 60, 3, dtype=torch.uint8), torch.zeros(40, 60, dtype=torch.uint8)
    win = (-2, 3, 50, 50)
    with pytest.raises(ops.Cd360Error, match="GPU"):
        ops.picture_resample(src, win, tabs(50, 16), tabs(50, 16), 16, 16)
    with pytest.raises(ops.Cd360Error, match="GPU"):
        ops.picture_mask(m, win, 8, 8)
    for bad in (dict(src=src.float()), dict(src=torch.zeros(40, 60, 2, dtype=torch.uint8)), dict(src=src.permute(1, 0, 2)), dict(window=(0, 0, 0, 5)),
                dict(window=(0, 0, 5)), dict(fill=256), dict(div=0.0), dict(xtab=tabs(50, 15)), dict(oh=0),
                dict(xtab=(tabs(50, 16)[0], tabs(50, 16)[1], torch.zeros(16, PC.MAX_TAPS + 1))), dict(out=torch.zeros(3, 16, 15))):
        kw = dict(src=src, window=win, xtab=tabs(50, 16), ytab=tabs(50, 16), oh=16, ow=16)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.picture_resample(**kw)
    for bad in (dict(k=4), dict(k=0), dict(k=PC.MAX_DILATE + 2), dict(thr=300), dict(src=src), dict(want=(False, False, False)), dict(window=(0, 0, 5, -1)),
                dict(out=(torch.zeros(8, 8), torch.zeros(8, 7), None))):
        kw = dict(src=m, window=win, oh=8, ow=8)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.picture_mask(**kw)
    shared = torch.zeros(8, 8)
    with pytest.raises(ValueError, match="overlap"):
        ops.picture_mask(m, win, 8, 8, out=(shared, shared, None))
    for kw in (dict(img_size=30), dict(kind="lanczos"), dict(dilate=4), dict(fill=300), dict(img_size=0)):
        with pytest.raises(ValueError):
            pictures.PictureFront(**kw)
    front = pictures.PictureFront(img_size=32)
    boxes = front.boxes([(60, 40)] * 2)
    with pytest.raises(ops.Cd360Error, match="GPU"):
        front.images([src, src], boxes)
    with pytest.raises(ops.Cd360Error, match="GPU"):
        front.masks([m, m], boxes)
    with pytest.raises(ValueError, match="mask"):  # a mask of another size than its picture
        front.batch([src, src], [m, m[:30]], boxes, 1)
    with pytest.raises(ValueError):
        front.batch([src, src], [m, m], boxes, 2)
    with pytest.raises(ValueError):
        front.images([src, src], boxes[:1])
    with pytest.raises(ops.Cd360Error, match="GPU"):
        finetune.encode_pictures(None, front, [src, src], [m, m], boxes, 1, seed=1, step=0)
    with pytest.raises(ops.Cd360Error, match="GPU"):
        pictures.init_from_pictures(None, front, [src], boxes[:1], [m])
