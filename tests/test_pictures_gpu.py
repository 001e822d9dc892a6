"""Pictures in, on the GPU: the two entry points of include/picture/cd360_picture.h against the numpy restatement of
tests/picture_cases.py with the SAME tap tables, bit for bit (every operation is one IEEE fp32 operation in a fixed order, and the kernels
evaluate no filter); against what the image library returns (tests/golden/pictures.npz) under the cap of tests/test_pictures_cpu.py;
their memory safety under tests/guarded.py with the output a slot in the middle of a batch tensor; PictureFront.batch,
finetune.encode_pictures and pictures.init_from_pictures against the per-picture calls and the restatement."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guarded as G
import picture_cases as PC
import sampler_cases as SC
import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NARROW_DDCONFIG = dict(attn_type="vanilla-xformers", double_z=True, z_channels=4, resolution=64, in_channels=3, out_ch=3, ch=64, ch_mult=[1, 2, 2],
                       num_res_blocks=1, attn_resolutions=[16], dropout=0.0)  # the narrow first stage of tests/test_images_gpu.py: 4 x down


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _padded(a, pad):
    """The picture `a` on the device in rows `pad` bytes longer than its pixels."""
    a = a if a.ndim == 3 else a[:, :, None]
    H, Wd, C = a.shape
    buf = torch.full((H, Wd * C + pad), 99, dtype=torch.uint8, device=DEV)
    buf[:, :Wd * C] = _dev(a.reshape(H, Wd * C))
    view = buf[:, :Wd * C].unflatten(1, (Wd, C))
    assert view.stride() == (Wd * C + pad, C, 1) and view.data_ptr() == buf.data_ptr()
    return view


def _tabs(n_in, n_out, kind):
    from cd360 import pictures
    return pictures.taps(n_in, n_out, kind), pictures.device_taps(n_in, n_out, kind, DEV)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _same_bits(got, want):
    want = np.ascontiguousarray(want, np.float32)
    return got.dtype == torch.float32 and tuple(got.shape) == want.shape and np.array_equal(_bits(got), want.view(np.uint32))


# ================================================================================================ 1: the resample entry, bit for bit
WHOLE = [(shape, kind) for shape in PC.SHAPES for kind in PC.KINDS]
# on a 40 x 56 picture: inside it; leaving it on the left, the top, the right, the bottom; around it; wholly outside
WINDOWS = [("inside", (10, 8, 30, 25)), ("left", (-7, 5, 30, 30)), ("top", (5, -6, 30, 30)), ("right", (35, 5, 30, 30)), ("bottom", (5, 25, 30, 30)),
           ("around", (-4, -5, 70, 50)), ("outside", (100, 90, 10, 12))]
RESAMPLE = [(f"{h}x{w}-{oh}x{ow}-{kind}", (h, w), (0, 0, w, h), (oh, ow), kind) for ((h, w), (oh, ow)), kind in WHOLE] + \
           [(f"window-{tag}-{kind}", (40, 56), win, out, kind) for tag, win in WINDOWS for out, kind in (((24, 20), "bicubic"), ((13, 13), "bilinear"))]


@pytest.mark.parametrize("tag,hw,window,out_hw,kind", RESAMPLE, ids=[c[0] for c in RESAMPLE])
def test_resample_equals_the_restatement_bit_for_bit(tag, hw, window, out_hw, kind):
    """cd360_picture_resample_u8 through ops.picture_resample against picture_cases.resample with the same tables, bits compared.  The six
    shapes of the table test, bilinear and bicubic, with the whole picture as the window; and on a 40 x 56 picture a window inside it,
    windows leaving it on each side, one around it and one wholly outside (all fill), to 24 x 20 (16-byte stores) and 13 x 13 (ow % 4 !=
    0: the scalar form).  Rotating over the cases: 3 channels and 1, rows padded by 5 bytes, fill 0 and 255, the uint8 roundings on and
    off, image scaling (/ 255, * 2, - 1) and none, the current and a second stream."""
    from cd360 import ops
    i = [c[0] for c in RESAMPLE].index(tag)
    C, pad, fill, rnd, side = (3, 1)[i % 2], (0, 5)[(i // 2) % 2], (255 if i % 3 == 0 else 0), i % 3 != 2, i % 5 == 1
    scale = (255.0, 2.0, -1.0) if i % 4 else (1.0, 1.0, 0.0)
    (H, Wd), (oh, ow) = hw, out_hw
    src = PC.picture(H, Wd, C if C == 3 else 0, seed=500 + i, kind=("noise", "smooth")[i % 2])
    (xt, xd), (yt, yd) = _tabs(window[2], ow, kind), _tabs(window[3], oh, kind)
    want = PC.resample(src, window, xt, yt, fill, rnd, *scale)
    dsrc = _padded(src, pad) if pad else _dev(src)
    kw = dict(fill=fill, round_u8=rnd, div=scale[0], mul=scale[1], add=scale[2])
    if side:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            got = ops.picture_resample(dsrc, window, xd, yd, oh, ow, **kw)
        s.synchronize()
    else:
        got = ops.picture_resample(dsrc, window, xd, yd, oh, ow, **kw)
    assert tuple(got.shape) == (C, oh, ow) and want.shape == (C, oh, ow)
    if not _same_bits(got, want):
        d = np.abs(got.cpu().numpy().astype(np.float64) - want)
        raise AssertionError(f"{tag}: C {C} pad {pad} fill {fill} round {rnd} scale {scale}: {int((d > 0).sum())} of {d.size} values differ, max {d.max():.3e}")
    if tag.startswith("window-outside"):
        assert len(np.unique(want)) == 1  # nothing of the picture: one value everywhere
    if window == (0, 0, Wd, H) and (H, Wd) == (oh, ow) and scale[0] == 1.0:
        assert np.array_equal(want, np.moveaxis(src.reshape(H, Wd, -1), 2, 0).astype(np.float32))  # the identity returns the input


def test_resample_is_the_image_library_within_one_level():
    """The same entry on the pictures of tests/golden/pictures.npz, as levels (div 1, mul 1, add 0): no value more than one level from
    what the image library returned, at most 1 % of a case's values differing at all -- the cap tests/test_pictures_cpu.py holds the
    restatement to, whose bits the kernel's are."""
    from cd360 import ops
    gold = dict(np.load(os.path.join(GOLD, "pictures.npz")))
    for tag in (str(t) for t in gold["pictures"]):
        src, window, fill, want = gold[f"{tag}.src"], tuple(int(v) for v in gold[f"{tag}.window"]), int(gold[f"{tag}.fill"]), gold[f"{tag}.out"]
        S = want.shape[0]
        (xt, xd), (yt, yd) = _tabs(window[2], S, "bicubic"), _tabs(window[3], S, "bicubic")
        got = ops.picture_resample(_dev(src), window, xd, yd, S, S, fill=fill, round_u8=True, div=1.0, mul=1.0, add=0.0)
        assert _same_bits(got, PC.resample(src, window, xt, yt, fill, True, 1.0, 1.0, 0.0)), tag
        lv = got.permute(1, 2, 0).cpu().numpy().reshape(want.shape)
        assert np.array_equal(lv, np.floor(lv)) and lv.min() >= 0 and lv.max() <= 255
        d = np.abs(lv.astype(np.int64) - want.astype(np.int64))
        share = float((d > 0).mean())
        print(f"{tag}: {int((d > 0).sum())} of {d.size} values differ from the image library, max {int(d.max())}, share {share:.5f}")
        assert d.max() <= 1 and share <= 0.01, tag


# ================================================================================================ 2: the mask entry
MASKS = [("8x8-k7", (37, 53), (0, -8, 52, 52), (8, 8), 7), ("k1", (37, 53), (0, -8, 52, 52), (8, 8), 1), ("leaves", (40, 56), (-9, 12, 60, 60), (16, 16), 3),
         ("ragged", (40, 56), (30, -20, 45, 50), (11, 7), 5), ("inside", (96, 128), (30, 10, 70, 70), (64, 64), 7), ("widest", (40, 56), (0, 0, 56, 40), (9, 13), PC.MAX_DILATE)]


@pytest.mark.parametrize("tag,hw,window,out_hw,k", MASKS, ids=[c[0] for c in MASKS])
def test_mask_maps_equal_the_restatement_and_conv2d(tag, hw, window, out_hw, k):
    """cd360_picture_mask_u8 against picture_cases.mask_maps and against clamp(conv2d(opacity, ones(k, k), padding="same"), 0, 1) on torch
    CPU, bit for bit: an 8 x 8 map with k = 7 (the window reaches past every border from every pixel), k = 1 (mask = opacity), crops that
    leave the picture, a non-square map, the largest window; every output left out in turn gives the other two the same bits."""
    from cd360 import ops
    (H, Wd), (oh, ow) = hw, out_hw
    src = PC.blob_mask(H, Wd, seed=700 + len(tag))
    opacity, mask, inside = PC.mask_maps(src, window, oh, ow, 125, k)
    dsrc = _padded(src, 3)[:, :, 0] if k == 3 else _dev(src)
    got = ops.picture_mask(dsrc, window, oh, ow, thr=125, k=k)
    for name, g, w in zip(("opacity", "mask", "inside"), got, (opacity, mask, inside)):
        assert _same_bits(g, w), (tag, name)
    conv = torch.clamp(F.conv2d(torch.from_numpy(opacity)[None, None], torch.ones(1, 1, k, k), padding="same"), 0, 1)[0, 0]
    assert torch.equal(got[1].cpu(), conv)
    assert 0 < opacity.sum() < opacity.size and (k == 1 or mask.sum() > opacity.sum()) and (window[0] >= 0 or inside.min() == 0)
    for skip in range(3):
        want = tuple(j != skip for j in range(3))
        part = ops.picture_mask(dsrc, window, oh, ow, thr=125, k=k, want=want)
        assert part[skip] is None and all(torch.equal(part[j], got[j]) for j in range(3) if j != skip), (tag, skip)
    other = ops.picture_mask(dsrc, window, oh, ow, thr=200, k=k)[0]
    assert _same_bits(other, PC.mask_maps(src, window, oh, ow, 200, k)[0]) and other.sum() < got[0].sum()


# ================================================================================================ 3: memory safety
def _guarded_case(case):
    from cd360 import _picture, ops
    src = PC.picture(40, 56, 3, seed=31, kind="noise")
    window = (-7, -6, 66, 52)
    if case == "resample-slot":
        tabs, host = {}, {}
        for name, n_in, n_out in (("xa", 66, 20), ("ya", 52, 24), ("xb", 66, 13), ("yb", 52, 13)):
            host[name], dev = _tabs(n_in, n_out, "bicubic")
            tabs.update({f"{name}{j}": t for j, t in enumerate(dev)})
        inputs = dict(src=_padded(src, 5), grey=_dev(src[:, :, 1]), batch_a=torch.full((3, 3, 24, 20), 7.0, device=DEV), batch_b=torch.full((3, 3, 13, 13), 7.0, device=DEV),
                      batch_c=torch.full((3, 1, 13, 13), 7.0, device=DEV), **tabs)

        @SC.guardfn
        def fn(guard, src, grey, batch_a, batch_b, batch_c, **t):
            tab = lambda n: tuple(t[f"{n}{j}"] for j in range(3))
            with G.recorded(guard, _picture):
                ops.picture_resample(src, window, tab("xa"), tab("ya"), 24, 20, out=batch_a[1])
                ops.picture_resample(src, window, tab("xb"), tab("yb"), 13, 13, fill=255, out=batch_b[1])
                ops.picture_resample(grey, window, tab("xb"), tab("yb"), 13, 13, round_u8=False, out=batch_c[1])
                fresh = [ops.picture_resample(src, window, tab("xa"), tab("ya"), 24, 20), ops.picture_resample(src, window, tab("xb"), tab("yb"), 13, 13, fill=255),
                         ops.picture_resample(grey, window, tab("xb"), tab("yb"), 13, 13, round_u8=False)]
            return dict(fresh=fresh)
        want = [PC.resample(src, window, host["xa"], host["ya"], 0), PC.resample(src, window, host["xb"], host["yb"], 255),
                PC.resample(src[:, :, 1], window, host["xb"], host["yb"], 0, False)]
        return fn, inputs, ("batch_a", "batch_b", "batch_c"), want
    assert case == "mask-slots"
    m = PC.blob_mask(40, 56, seed=32)
    inputs = dict(src=_dev(m), opa=torch.full((3, 1, 11, 7), 7.0, device=DEV), dil=torch.full((3, 1, 11, 7), 7.0, device=DEV), ins=torch.full((3, 1, 11, 7), 7.0, device=DEV))

    @SC.guardfn
    def fn(guard, src, opa, dil, ins):
        with G.recorded(guard, _picture):
            ops.picture_mask(src, window, 11, 7, k=5, out=(opa[1, 0], dil[1, 0], ins[1, 0]))
            fresh = [[t for t in ops.picture_mask(src, window, 11, 7, k=5, want=tuple(j != skip for j in range(3))) if t is not None] for skip in (0, 1, 2, 3)]
        return dict(fresh=fresh)
    return fn, inputs, ("opa", "dil", "ins"), list(PC.mask_maps(m, window, 11, 7, 125, 5))


@pytest.mark.parametrize("case,declares", PC.GUARDED, ids=[c[0] for c in PC.GUARDED])
def test_picture_entry_points_write_their_slot_only(case, declares):
    """Both entry points under tests/guarded.py, both poison patterns.  The output is slot 1 of a three-slot batch tensor filled with 7:
    after the call slot 1 holds the restatement's bits and slots 0 and 2 still hold 7; the source and the tables are unchanged (P3); the
    work planes and the fresh outputs are arena blocks between canaries (P1), fully written (P2: finite and bit-equal under both poisons)."""
    fn, inputs, inout, want = _guarded_case(case)
    first, _ = G.run_twice(fn, inputs, declares=declares, inout=inout)
    for name, w in zip(inout, want):
        slots = inputs[name]
        assert bool((slots[0] == 7).all()) and bool((slots[2] == 7).all()), name
        assert _same_bits(slots[1].reshape(w.shape), w), name
    if case == "resample-slot":
        assert all(_same_bits(f, w) for f, w in zip(first["fresh"], want))
    else:
        assert [len(f) for f in first["fresh"]] == [2, 2, 2, 3] and all(_same_bits(f, w) for f, w in zip(first["fresh"][3], want))


# ================================================================================================ 4: the front
def _frames(sizes, seed):
    pics = [PC.picture(h, w, 3, seed + 2 * j, kind=("smooth", "noise")[j % 2]) for j, (w, h) in enumerate(sizes)]
    masks = [PC.blob_mask(h, w, seed + 2 * j + 1) for j, (w, h) in enumerate(sizes)]
    return pics, masks


def _restated_batch(front, pics, masks, boxes, n_ref):
    """What PictureFront.batch must return, from the restatement alone."""
    from cd360 import pictures
    S, s, per = front.img_size, front.img_size // front.factor, 1 + n_ref
    wins = [(int(b[0]), int(b[1]), int(b[2] - b[0]), int(b[3] - b[1])) for b in boxes]
    x = np.stack([PC.resample(p, w, pictures.taps(w[2], S, front.kind), pictures.taps(w[3], S, front.kind), front.fill, front.round_u8) for p, w in zip(pics, wins)])
    maps = [PC.mask_maps(m, w, s, s, pictures.THRESHOLD, front.dilate) for m, w in zip(masks, wins)]
    opa, dil, ins = (np.stack([mp[j] for mp in maps])[:, None] for j in range(3))
    B = len(pics) // per
    r = lambda a: a.reshape(B, per, *a.shape[1:])
    return dict(jpg=r(x)[:, 0], jpg_ref=r(x)[:, 1:], mask=r(dil)[:, 0], depth=r(opa)[:, 0], mask_ref=r(ins)[:, 1:]), wins


SIZES = [(56, 40), (40, 56), (33, 47), (64, 64), (80, 64), (50, 30)]  # (w, h) of 2 samples x (1 + 2) pictures
BBOXES = [None, [10, 5, 50, 45], [-4, 3, 30, 44], None, [30, 20, 90, 60], [5.5, 2, 40, 29]]


def test_front_batch_is_the_per_picture_calls_under_the_loaders_names():
    """PictureFront.batch on 2 samples of 1 + 2 pictures of six sizes, boxes from front.boxes (whole pictures and boxes partly outside):
    every tensor equals the restatement bit for bit, under the loader's keys and shapes; images() and masks() alone give the same bits;
    data_co3d.make_cameras takes crop_coords and original_size_as_tuple row by row."""
    from cd360 import pictures
    from sgm.data.data_co3d import make_cameras
    front = pictures.PictureFront(img_size=32, factor=4, dilate=3)
    pics, masks = _frames(SIZES, seed=40)
    boxes = front.boxes(SIZES, BBOXES)
    want, wins = _restated_batch(front, pics, masks, boxes, 2)
    dp, dm = [_dev(p) for p in pics], [_dev(m) for m in masks]
    got = front.batch(dp, dm, boxes, 2)
    assert set(got) == {"jpg", "jpg_ref", "mask", "depth", "mask_ref", "crop_coords", "original_size_as_tuple"}
    shapes = dict(jpg=(2, 3, 32, 32), jpg_ref=(2, 2, 3, 32, 32), mask=(2, 1, 8, 8), depth=(2, 1, 8, 8), mask_ref=(2, 2, 1, 8, 8))
    for key, shape in shapes.items():
        assert tuple(got[key].shape) == shape and got[key].device.type == DEV and got[key].is_contiguous() and _same_bits(got[key], want[key]), key
    assert float(got["jpg"].min()) >= -1 and float(got["jpg"].max()) <= 1 and float(got["mask_ref"].min()) == 0  # a view's box leaves its picture
    assert got["crop_coords"].dtype == torch.int32 and got["crop_coords"].reshape(-1, 4).tolist() == [list(w) for w in wins]
    assert got["original_size_as_tuple"].reshape(-1, 4).tolist() == [[w, h, win[2], win[3]] for (w, h), win in zip(SIZES, wins)]
    x, (dil, opa, ins) = front.images(dp, boxes), front.masks(dm, boxes)
    assert torch.equal(x.reshape(2, 3, 3, 32, 32)[:, 0], got["jpg"]) and torch.equal(x.reshape(2, 3, 3, 32, 32)[:, 1:], got["jpg_ref"])
    assert torch.equal(dil.reshape(2, 3, 1, 8, 8)[:, 0], got["mask"]) and torch.equal(opa.reshape(2, 3, 1, 8, 8)[:, 0], got["depth"])
    assert torch.equal(ins.reshape(2, 3, 1, 8, 8)[:, 1:], got["mask_ref"])
    soft = pictures.PictureFront(img_size=32, factor=4, round_u8=False, kind="bilinear", fill=255)
    want_soft = np.stack([PC.resample(p, w, pictures.taps(w[2], 32, "bilinear"), pictures.taps(w[3], 32, "bilinear"), 255, False) for p, w in zip(pics, wins)])
    assert _same_bits(soft.images(dp, boxes), want_soft)
    for b in range(2):
        R, T = torch.eye(3)[None].repeat(3, 1, 1), torch.tensor([[0.0, 0.0, 3.0]]).repeat(3, 1)
        cams = make_cameras(R, T, torch.full((3, 2), 2.0), torch.zeros(3, 2), got["original_size_as_tuple"][b], got["crop_coords"][b], 32)
        assert len(cams) == 3 and all(torch.isfinite(c.focal_length).all() and torch.isfinite(c.principal_point).all() for c in cams)


@pytest.fixture(scope="module")
def first_stage():
    """FirstStage on the narrow first stage of tests/test_images_gpu.py (tests/golden/weights.py weights, fp32 parameters)."""
    from cd360 import images
    from sgm.modules.diffusionmodules.model import Decoder, Encoder
    enc, dec = Encoder(**NARROW_DDCONFIG).eval(), Decoder(**NARROW_DDCONFIG).eval()
    W.load_into(enc, 3)
    W.load_into(dec, 3)
    qc, pqc = torch.nn.Conv2d(8, 8, 1), torch.nn.Conv2d(4, 4, 1)
    with torch.no_grad():
        qc.weight.copy_(W.tensor("qc.w", (8, 8, 1, 1), seed=3) * 0.35)
        qc.bias.copy_(W.tensor("qc.b", (8,), seed=3) * 0.05)
        pqc.weight.copy_(W.tensor("pqc.w", (4, 4, 1, 1), seed=3) * 0.5)
        pqc.bias.copy_(W.tensor("pqc.b", (4,), seed=3) * 0.05)
    mods = [m.to(DEV) for m in (enc, dec, qc, pqc)]
    for m in mods:
        for p in m.parameters():
            p.requires_grad_(False)
    return images.FirstStage(*mods)


def test_encode_pictures_is_encode_batch_on_the_restated_tensors(first_stage):
    """finetune.encode_pictures at img_size 32 on the narrow first stage: x0 and x_ref are, bit for bit, finetune.encode_batch on the jpg /
    jpg_ref tensors made by the restatement on the host, with the same seed, step and stream ids; the batch it returns is front.batch's."""
    from cd360 import finetune, pictures
    front = pictures.PictureFront(img_size=32, factor=4, dilate=3)
    pics, masks = _frames(SIZES, seed=60)
    boxes = front.boxes(SIZES, BBOXES)
    want, _ = _restated_batch(front, pics, masks, boxes, 2)
    x0, x_ref, batch = finetune.encode_pictures(first_stage, front, [_dev(p) for p in pics], [_dev(m) for m in masks], boxes, 2, seed=77, step=5, streams=[3, 9])
    w0, w_ref = finetune.encode_batch(first_stage, _dev(want["jpg"]), _dev(want["jpg_ref"]), seed=77, step=5, streams=[3, 9])
    assert tuple(x0.shape) == (2, 4, 8, 8) and tuple(x_ref.shape) == (2, 2, 4, 8, 8) and bool(torch.isfinite(x0).all())
    assert torch.equal(x0, w0) and torch.equal(x_ref, w_ref)
    assert all(_same_bits(batch[k], want[k]) for k in want)
    other = finetune.encode_pictures(first_stage, front, [_dev(p) for p in pics], [_dev(m) for m in masks], boxes, 2, seed=77, step=6, streams=[3, 9])[0]
    assert not torch.equal(other, x0)
    alone, none, _ = finetune.encode_pictures(first_stage, front, [_dev(pics[0]), _dev(pics[3])], [_dev(masks[0]), _dev(masks[3])], boxes[[0, 3]], 0, seed=77, step=5)
    assert none is None and tuple(alone.shape) == (2, 4, 8, 8)


def test_init_from_pictures_is_encode_mode_and_latent_mask_on_the_restated_tensors(first_stage):
    """pictures.init_from_pictures: the latents are first_stage.encode_mode of the restated pictures; the masks are images.latent_mask of
    the regions through the crop and the nearest rule at img_size (0 outside the picture: kept), [N, 1, 8, 8] with values between 0 and 1."""
    from cd360 import images, pictures
    front = pictures.PictureFront(img_size=32, factor=4)
    pics, regions = _frames(SIZES[:3], seed=80)
    regions = [(r > 125).astype(np.uint8) * 255 for r in regions]
    boxes = front.boxes(SIZES[:3], BBOXES[:3])
    want, wins = _restated_batch(front, pics, regions, boxes, 0)
    init, lm = pictures.init_from_pictures(first_stage, front, [_dev(p) for p in pics], boxes, [_dev(r) for r in regions])
    assert torch.equal(init, first_stage.encode_mode(_dev(want["jpg"]))) and tuple(init.shape) == (3, 4, 8, 8)
    full = np.stack([PC.mask_maps(r, w, 32, 32, 0, 1)[0] for r, w in zip(regions, wins)])[:, None]
    assert torch.equal(lm, images.latent_mask(_dev(full), 4)) and tuple(lm.shape) == (3, 1, 8, 8)
    assert 0 < float(lm.sum()) < lm.numel() and float(lm.min()) >= 0 and float(lm.max()) <= 1 and bool(((lm > 0) & (lm < 1)).any())
    init2, none = pictures.init_from_pictures(first_stage, front, [_dev(p) for p in pics], boxes)
    assert none is None and torch.equal(init2, init)
