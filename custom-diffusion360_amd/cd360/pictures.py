"""Pictures in: from decoded uint8 frames to the tensors `finetune.encode_batch`, `train_step_latents` and `job.sample_images` take.

What the reference's data loader does per picture on the host between a decoded frame and the first stage (sgm/data/data_co3d.py:332-352,
373-390, 518-555, 469-471) -- the square crop window that may leave the picture, `Resize(img_size, BICUBIC)` -> `ToTensor` -> `x * 2 - 1`,
the thresholded mask cropped and resized to `img_size // 8`, its 7 x 7 dilation, the all-ones "padding" mask -- as launches of
include/picture/cd360_picture.h on frames that are already on the device.  File reading and decoding stay with the caller.

The resize is the separable antialiased filter the reference's image library and `F.interpolate(..., antialias=True)` share.  With
n_in the crop's side, n_out the target side and isz the filter size (2: bilinear, 4: bicubic with a = -0.5):

    scale = n_in / n_out;  support = isz / 2 * scale if scale >= 1 else isz / 2;  inv = 1 / scale if scale >= 1 else 1
    output i:  c = scale * (i + 0.5);  xmin = max(0, int(c - support + 0.5));  xsize = min(n_in, int(c + support + 0.5)) - xmin
               w_j = filter((j + xmin - c + 0.5) * inv), divided by the sum of the w_j

`taps` evaluates that once per (n_in, n_out, kind) on the host in numpy fp32 and `device_taps` keeps a device copy: the kernels evaluate
no filter, so a host restatement with the same table gives the same bits (tests/picture_cases.py).  `round_u8=True` adds the two uint8
roundings of the image library (it stores the horizontal pass and the result in uint8), which is what the reference's loader yields to
within one grey level on a few pixels in ten thousand ("Pictures in"); `round_u8=False` is torch's float `antialias=True`.

    front = PictureFront(img_size=512)
    boxes = front.boxes([(W, H), ...], bboxes)                               the loader's _padded_bbox / _crop_bbox
    batch = front.batch(pictures, masks, boxes, n_ref)                       jpg, jpg_ref, mask, depth, mask_ref, crop_coords, ...
    x0, x_ref, batch = finetune.encode_pictures(first_stage, front, pictures, masks, boxes, n_ref, seed, step)
    init, masks = init_from_pictures(first_stage, front, pictures, boxes, regions)        for job.sample_images(init_latents=, masks=)"""
from __future__ import annotations

import functools

import numpy as np
import torch

from . import ops
from .images import latent_mask

KINDS = {"bilinear": 2, "bicubic": 4}  # kind -> filter size
THRESHOLD = 125  # a mask pixel counts where it is > THRESHOLD (data_co3d.py:534)
_F32 = np.float32


def _bilinear(x):
    x = np.abs(x)
    return np.where(x < 1, 1 - x, 0).astype(x.dtype)


def _bicubic(x):
    a = x.dtype.type(-0.5)
    x = np.abs(x)
    near = ((a + 2) * x - (a + 3)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1, near, np.where(x < 2, far, 0)).astype(x.dtype)


_FILTERS = {"bilinear": _bilinear, "bicubic": _bicubic}


@functools.lru_cache(maxsize=None)
def taps(n_in: int, n_out: int, kind: str = "bicubic"):
    """The tap table that resizes an axis of n_in pixels to n_out -> (xmin int32 [n_out], size int32 [n_out], weights fp32 [n_out, T]),
    by the rule above in numpy fp32; row i holds size[i] weights that sum to 1, then zeros.  Cached: treat the arrays as read-only."""
    if kind not in KINDS:
        raise ValueError(f"kind = {kind!r}: served are {sorted(KINDS)}")
    if n_in <= 0 or n_out <= 0:
        raise ValueError(f"n_in, n_out must be positive, got {n_in}, {n_out}")
    half = _F32(KINDS[kind] / 2)
    scale = _F32(n_in) / _F32(n_out)
    support = half * scale if scale >= 1 else half
    inv = _F32(1) / scale if scale >= 1 else _F32(1)
    c = scale * (np.arange(n_out, dtype=_F32) + _F32(0.5))
    xmin = np.maximum(0, (c - support + _F32(0.5)).astype(np.int64))
    size = np.minimum(n_in, (c + support + _F32(0.5)).astype(np.int64)) - xmin
    T = int(size.max())
    if T > ops.PICTURE_MAX_TAPS:
        raise ValueError(f"{n_in} -> {n_out} ({kind}) needs {T} taps per pixel, served: {ops.PICTURE_MAX_TAPS} (CD360_PICTURE_MAX_TAPS)")
    j = np.arange(T, dtype=np.int64)[None, :]
    w = _FILTERS[kind](((j + xmin[:, None]).astype(_F32) - c[:, None] + _F32(0.5)) * inv)
    w = np.where(j < size[:, None], w, _F32(0)).astype(_F32)
    total = np.zeros(n_out, _F32)
    for t in range(T):  # the sum in rising order, one rounding per term
        total = total + w[:, t]
    table = (xmin.astype(np.int32), size.astype(np.int32), (w / total[:, None]).astype(_F32))
    for a in table:
        a.setflags(write=False)
    return table


_DEVICE_TAPS = {}


def device_taps(n_in: int, n_out: int, kind: str, device):
    """`taps` as three device tensors, copied once per (n_in, n_out, kind, device)."""
    key = (n_in, n_out, kind, str(torch.device(device)))
    tab = _DEVICE_TAPS.get(key)
    if tab is None:
        tab = _DEVICE_TAPS[key] = tuple(torch.from_numpy(np.array(a)).to(device) for a in taps(n_in, n_out, kind))
    return tab


def _gpu(t: torch.Tensor) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ops.Cd360Error("the picture kernels run only on the GPU; got a CPU tensor")
    return t


class PictureFront:
    """The loader's per-picture arithmetic on device frames.  img_size: the training size S; factor: the first stage's down-sampling (the
    masks are S / factor); dilate: the odd dilation window of `mask`; kind: "bicubic" (the loader) or "bilinear"; round_u8: the image
    library's uint8 roundings (True: what the loader yields) or torch's float antialias result (False); fill: 0, or 255 for the
    white-background crop."""

    def __init__(self, img_size: int = 512, factor: int = 8, dilate: int = 7, kind: str = "bicubic", round_u8: bool = True, fill: int = 0):
        if img_size <= 0 or factor <= 0 or img_size % factor:
            raise ValueError(f"img_size = {img_size} must be a positive multiple of factor = {factor}")
        if kind not in KINDS:
            raise ValueError(f"kind = {kind!r}: served are {sorted(KINDS)}")
        if dilate < 1 or dilate % 2 == 0 or dilate > ops.PICTURE_MAX_DILATE:
            raise ValueError(f"dilate = {dilate}: an odd window of 1..{ops.PICTURE_MAX_DILATE} is needed")
        if not 0 <= fill <= 255:
            raise ValueError(f"fill = {fill}: a byte is needed")
        self.img_size, self.factor, self.dilate, self.kind, self.round_u8, self.fill = img_size, factor, dilate, kind, bool(round_u8), fill

    # ------------------------------------------------------------------------------------------------ crop windows
    @staticmethod
    def boxes(sizes_wh, bboxes=None) -> np.ndarray:
        """The loader's square crop boxes, int64 [N, 4] as (x0, y0, x1, y1), which may leave the picture: for a picture of (w, h) without a
        box, _padded_bbox = the square around the whole picture (data_co3d.py:373-378); with an xyxy box, _crop_bbox = the square around
        the box, its corners rounded (data_co3d.py:380-390).  bboxes: None, or one entry per picture, each None or a box."""
        from sgm.data.data_co3d import square_bbox
        sizes = [tuple(int(v) for v in s) for s in sizes_wh]
        bboxes = [None] * len(sizes) if bboxes is None else list(bboxes)
        if len(bboxes) != len(sizes):
            raise ValueError(f"{len(bboxes)} boxes for {len(sizes)} pictures")
        out = []
        for (w, h), box in zip(sizes, bboxes):
            if w <= 0 or h <= 0:
                raise ValueError(f"a picture of {w} x {h}")
            if box is None:
                out.append(square_bbox(np.array([0, 0, w, h]).astype(np.float32)).astype(np.int64))
                continue
            b = square_bbox(np.asarray(box).astype(np.float32))
            side = b[2] - b[0]
            center = (b[:2] + b[2:]) / 2
            extent = side / 2
            ul = (center - extent).round().astype(int)
            lr = ul + np.round(2 * extent).astype(int)
            out.append(np.concatenate((ul, lr)).astype(np.int64))
        return np.stack(out) if out else np.zeros((0, 4), np.int64)

    @staticmethod
    def _windows(boxes, n: int):
        boxes = np.asarray(boxes)
        if boxes.shape != (n, 4):
            raise ValueError(f"boxes: [{n}, 4] (x0, y0, x1, y1) is needed, got {boxes.shape}")
        return [(int(b[0]), int(b[1]), int(b[2] - b[0]), int(b[3] - b[1])) for b in boxes]

    # ------------------------------------------------------------------------------------------------ pictures and masks
    def images(self, pictures, boxes) -> torch.Tensor:
        """uint8 [H, W, 3] device frames of any sizes, each through its crop box and the resize -> fp32 [N, 3, S, S] in [-1, 1]: the bits
        of ToTensor and x * 2 - 1 on the resized uint8 picture (round_u8), the layout Encoder.forward reads."""
        pictures = list(pictures)
        ops._refuse(not pictures, "no pictures")
        wins = self._windows(boxes, len(pictures))
        for p in pictures:
            ops._refuse(not isinstance(p, torch.Tensor) or p.ndim != 3 or p.shape[2] != 3, f"a picture: uint8 [H, W, 3] is needed, got {tuple(getattr(p, 'shape', ()))}")
            _gpu(p)
        S = self.img_size
        out = torch.empty((len(pictures), 3, S, S), dtype=torch.float32, device=pictures[0].device)
        for i, (p, win) in enumerate(zip(pictures, wins)):
            xt, yt = device_taps(win[2], S, self.kind, p.device), device_taps(win[3], S, self.kind, p.device)
            ops.picture_resample(p, win, xt, yt, S, S, fill=self.fill, round_u8=self.round_u8, out=out[i])
        return out

    def masks(self, masks, boxes):
        """uint8 [H, W] device masks -> (mask, opacity, inside), fp32 [N, 1, S / factor, S / factor] each: opacity = the loader's `depth`
        (the thresholded mask through the crop and the nearest resize), mask = its dilation (the loader's `mask`), inside = the all-ones
        picture through the same crop and resize (the loader's `masks_padding`, which becomes `mask_ref`)."""
        masks = list(masks)
        ops._refuse(not masks, "no masks")
        wins = self._windows(boxes, len(masks))
        for m in masks:
            ops._refuse(not isinstance(m, torch.Tensor) or m.ndim != 2, f"a mask: uint8 [H, W] is needed, got {tuple(getattr(m, 'shape', ()))}")
            _gpu(m)
        s = self.img_size // self.factor
        dil, opa, ins = (torch.empty((len(masks), 1, s, s), dtype=torch.float32, device=masks[0].device) for _ in range(3))
        for i, (m, win) in enumerate(zip(masks, wins)):
            ops.picture_mask(m, win, s, s, thr=THRESHOLD, k=self.dilate, out=(opa[i, 0], dil[i, 0], ins[i, 0]))
        return dil, opa, ins

    def batch(self, pictures, masks, boxes, n_ref: int) -> dict:
        """B samples of 1 + n_ref pictures each, sample by sample with the target first -> the loader's batch: jpg [B, 3, S, S], jpg_ref
        [B, n_ref, 3, S, S], mask / depth [B, 1, s, s] of the targets, mask_ref [B, n_ref, 1, s, s] of the views (s = S / factor), and per
        sample and picture the rows data_co3d.make_cameras takes: crop_coords int32 [B, 1 + n_ref, 4] = (x, y, w, h) and
        original_size_as_tuple int64 [B, 1 + n_ref, 4] = (W, H, crop w, crop h), both on the host."""
        pictures, masks = list(pictures), list(masks)
        per = 1 + int(n_ref)
        if n_ref < 0 or not pictures or len(pictures) % per or len(masks) != len(pictures):
            raise ValueError(f"{len(pictures)} pictures and {len(masks)} masks for samples of 1 + {n_ref} pictures")
        for p, m in zip(pictures, masks):
            if tuple(m.shape[:2]) != tuple(p.shape[:2]):
                raise ValueError(f"a mask of {tuple(m.shape)} for a picture of {tuple(p.shape)}: resize the mask to its picture first")
        B = len(pictures) // per
        S, s = self.img_size, self.img_size // self.factor
        wins = self._windows(boxes, len(pictures))
        x = self.images(pictures, boxes).reshape(B, per, 3, S, S)
        dil, opa, ins = (t.reshape(B, per, 1, s, s) for t in self.masks(masks, boxes))
        crop = torch.tensor(wins, dtype=torch.int32).reshape(B, per, 4)
        orig = torch.tensor([[p.shape[1], p.shape[0], w[2], w[3]] for p, w in zip(pictures, wins)], dtype=torch.int64).reshape(B, per, 4)
        return {"jpg": x[:, 0].contiguous(), "jpg_ref": x[:, 1:].contiguous(), "mask": dil[:, 0].contiguous(), "depth": opa[:, 0].contiguous(),
                "mask_ref": ins[:, 1:].contiguous(), "crop_coords": crop, "original_size_as_tuple": orig}


def init_from_pictures(first_stage, front: PictureFront, pictures, boxes, regions=None):
    """Pictures the caller owns -> (init_latents, masks) for job.sample_images(init_latents=, masks=): init_latents [N, 4, S / 8, S / 8] =
    first_stage.encode_mode of front.images; masks = None without regions, else the regions (uint8 [H, W] device tensors of their
    pictures' sizes, nonzero = generate) through the same crop and a nearest resize to S, then images.latent_mask."""
    pictures = list(pictures)
    x = front.images(pictures, boxes)
    init = first_stage.encode_mode(x)
    if regions is None:
        return init, None
    regions = list(regions)
    if len(regions) != len(pictures):
        raise ValueError(f"{len(regions)} regions for {len(pictures)} pictures")
    wins = front._windows(boxes, len(pictures))
    S = front.img_size
    full = torch.empty((len(regions), 1, S, S), dtype=torch.float32, device=init.device)
    for i, (r, p, win) in enumerate(zip(regions, pictures, wins)):
        if tuple(r.shape) != tuple(p.shape[:2]):
            raise ValueError(f"a region of {tuple(r.shape)} for a picture of {tuple(p.shape)}")
        ops.picture_mask(_gpu(r), win, S, S, thr=0, k=1, want=(True, False, False), out=(full[i, 0], None, None))
    return init, latent_mask(full, front.factor)
