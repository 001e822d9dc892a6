"""Golden pictures of the image library the reference's data loader resizes with (Pillow; written with 12.2.0).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_picture_golden.py

Writes tests/golden/pictures.npz.  Seeded small pictures (tests/picture_cases.py: smooth and noise, at most 96 x 128) go through what the
loader does to a frame (sgm/data/data_co3d.py:392-407, 332-352): `crop` to a window that may leave the picture (filled with 0), or the
white-background variant (a white image the frame is pasted into, fill 255), then `resize((S, S), BICUBIC)`; and seeded masks through
`> 125`, a mode-"1" image, the same crop and a resize to (s, s), which the library does by NEAREST for a boolean image whatever filter is
asked for.  Stored per case: the source, the window, the fill, the library's result, and `share`: the share of the pixels on which the
fp32 restatement with the two uint8 roundings (tests/picture_cases.py) differs from it -- by one grey level at the most, asserted here.
The library resamples uint8 pictures with 22-bit fixed-point weights made from float64 ones; the restatement's weights are fp32: a value
that lands within about 1e-5 of a rounding boundary can go either way, which is the whole difference.  The seeds below were kept
because every case stays at or below one pixel in 256; the test caps a case at 1 %."""
from __future__ import annotations

import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE)]
import picture_cases as PC  # noqa: E402

# (tag, H, W, C (0: one channel, 2-d), picture kind, seed, window (left, top, w, h), S, fill)
PICTURES = [
    ("leaves-smooth", 37, 53, 3, "smooth", 1, (-5, -9, 61, 61), 16, 0),
    ("leaves-noise", 37, 53, 3, "noise", 2, (-5, -9, 61, 61), 16, 0),
    ("tall-smooth", 80, 64, 3, "smooth", 3, (-8, 0, 80, 80), 32, 0),
    ("tall-noise", 80, 64, 3, "noise", 4, (-8, 0, 80, 80), 32, 0),
    ("up-smooth", 48, 48, 3, "smooth", 5, (0, 0, 48, 48), 64, 0),
    ("up-noise", 48, 48, 3, "noise", 6, (0, 0, 48, 48), 64, 0),
    ("wide-white", 96, 128, 3, "smooth", 7, (0, -16, 128, 128), 64, 255),
    ("wide-white-noise", 96, 128, 3, "noise", 8, (0, -16, 128, 128), 64, 255),
    ("inside-grey", 64, 90, 0, "noise", 9, (20, 7, 50, 50), 24, 0),
    ("corner-grey", 40, 40, 0, "smooth", 10, (25, 22, 30, 30), 20, 255),
]
# (tag, H, W, seed, window, s)
MASKS = [
    ("mask-100", 100, 100, 21, (0, 0, 100, 100), 64),
    ("mask-tall", 80, 64, 22, (-8, 0, 80, 80), 16),
    ("mask-leaves", 37, 53, 23, (-5, -9, 61, 61), 8),
    ("mask-inside", 96, 128, 24, (30, 10, 70, 70), 12),
]


def library_crop(img, window, fill):
    left, top, w, h = window
    if fill == 0:
        return img.crop((left, top, left + w, top + h))
    white = Image.new(img.mode, (w, h), (fill,) * len(img.getbands()) if len(img.getbands()) > 1 else fill)
    white.paste(img, (-left, -top))
    return white


def main():
    out = {"pictures": np.array([p[0] for p in PICTURES]), "masks": np.array([m[0] for m in MASKS])}
    for tag, H, W, C, kind, seed, window, S, fill in PICTURES:
        src = PC.picture(H, W, C, seed, kind)
        got = np.array(library_crop(Image.fromarray(src), window, fill).resize((S, S), Image.BICUBIC))
        mine = PC.levels(src, window, PC.tap_table(window[2], S, "bicubic"), PC.tap_table(window[3], S, "bicubic"), fill)
        d = np.abs(mine.astype(np.int64) - got.astype(np.int64))
        share = float((d > 0).mean())
        print(f"{tag}: {src.shape} window {window} -> {S}, fill {fill}: {int((d > 0).sum())} of {d.size} values differ, max {int(d.max())}, share {share:.5f}")
        assert d.max() <= 1 and share <= 1 / 256 + 1e-12, tag
        out.update({f"{tag}.src": src, f"{tag}.window": np.asarray(window, np.int64), f"{tag}.fill": np.int64(fill), f"{tag}.out": got,
                    f"{tag}.share": np.float64(share)})
    for tag, H, W, seed, window, s in MASKS:
        src = PC.blob_mask(H, W, seed)
        got = np.array(library_crop(Image.fromarray(src > 125), window, 0).resize((s, s), Image.BICUBIC))
        assert got.dtype == np.bool_ and 0 < got.sum() < got.size, tag
        assert np.array_equal(PC.mask_maps(src, window, s, s, 125, 1)[0], got.astype(np.float32)), tag
        out.update({f"{tag}.src": src, f"{tag}.window": np.asarray(window, np.int64), f"{tag}.out": got})
    path = os.path.join(HERE, "pictures.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
