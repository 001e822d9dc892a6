"""What tests/test_pictures_cpu.py, tests/test_pictures_gpu.py and tests/golden/make_picture_golden.py share (plain helper module, like
train_cases.py; no tests, no fixtures): the names include/picture/cd360_picture.h adds, and numpy restatements of its two entry points by
the rules of DESIGN.md ("Pictures in"), independent of cd360.pictures: the tap table of the antialiased separable filter in the dtype the
caller names (np.float32: what cd360.pictures.taps must return bit for bit; np.float64: the yardstick against torch), the crop that may
leave the picture, the two passes in rising tap order with one rounding per operation, the uint8 roundings, and the integer nearest
rule, threshold and dilation of the mask entry."""
import os

import numpy as np

HEADER = os.path.join("picture", "cd360_picture.h")
NEW = ["cd360_picture_resample_u8", "cd360_picture_mask_u8"]
KERNELS = ("picture_rows_kernel", "picture_cols_kernel", "picture_mask_kernel")
BUILD_ROW = ("libcd360_picture.so", "csrc_picture", ["picture_stage.hip"], "_picture")
# the guarded cases of tests/test_pictures_gpu.py::test_picture_entry_points_write_their_slot_only: (id, entry points the case must reach)
GUARDED = [("resample-slot", ["cd360_picture_resample_u8"]), ("mask-slots", ["cd360_picture_mask_u8"])]
MAX_TAPS, MAX_DILATE = 64, 31
F32 = np.float32
# (H, W) -> (oh, ow): down-scaling by non-integers, anisotropic, up-scaling, a near-identity scale, the identity, a tiny one
SHAPES = [((37, 53), (8, 8)), ((64, 64), (32, 16)), ((19, 23), (40, 31)), ((90, 70), (64, 64)), ((16, 16), (16, 16)), ((5, 7), (3, 2))]
KINDS = ("bilinear", "bicubic")


# ------------------------------------------------------------------------------------------------ the tap table
def filter_of(kind):
    def bilinear(x):
        x = np.abs(x)
        return np.where(x < 1, 1 - x, 0 * x)

    def bicubic(x):
        a = x.dtype.type(-0.5)
        x = np.abs(x)
        return np.where(x < 1, ((a + 2) * x - (a + 3)) * x * x + 1, np.where(x < 2, (((x - 5) * x + 8) * x - 4) * a, 0 * x))
    return {"bilinear": (bilinear, 2), "bicubic": (bicubic, 4)}[kind]


def tap_table(n_in, n_out, kind, dtype=F32):
    """(xmin int32 [n_out], size int32 [n_out], weights `dtype` [n_out, T]) by the rule, every scalar and array in `dtype`."""
    dt = np.dtype(dtype).type
    filt, isz = filter_of(kind)
    scale = dt(n_in) / dt(n_out)
    support = dt(isz / 2) * scale if scale >= 1 else dt(isz / 2)
    inv = dt(1) / scale if scale >= 1 else dt(1)
    xmin, size, rows = [], [], []
    for i in range(n_out):
        c = scale * (dt(i) + dt(0.5))
        lo = max(0, int(c - support + dt(0.5)))
        n = min(n_in, int(c + support + dt(0.5))) - lo
        w = filt((np.arange(n).astype(dt) + dt(lo) - c + dt(0.5)) * inv).astype(dt)
        total = dt(0)
        for v in w:
            total = total + v
        xmin.append(lo), size.append(n), rows.append(w / total)
    T = max(size)
    wt = np.zeros((n_out, T), dt)
    for i, w in enumerate(rows):
        wt[i, :len(w)] = w
    return np.asarray(xmin, np.int32), np.asarray(size, np.int32), wt


# ------------------------------------------------------------------------------------------------ crop, passes, roundings
def crop(src, window, fill):
    """src [H, W] or [H, W, C] through the window (left, top, w, h) that may leave it: the pixels outside are `fill`."""
    left, top, w, h = window
    H, W = src.shape[:2]
    out = np.full((h, w) + src.shape[2:], fill, src.dtype)
    x0, x1, y0, y1 = max(left, 0), min(left + w, W), max(top, 0), min(top + h, H)
    if x1 > x0 and y1 > y0:
        out[y0 - top:y1 - top, x0 - left:x1 - left] = src[y0:y1, x0:x1]
    return out


def apply_taps(a, table, axis):
    """The pass of one axis: out[i] = sum over j < size[i] in rising order of w[i, j] * a[xmin[i] + j], one multiply and one add each,
    in the table's dtype."""
    xmin, size, wt = table
    dt = wt.dtype.type
    a = np.moveaxis(np.asarray(a, wt.dtype), axis, 0)
    out = np.zeros((len(xmin),) + a.shape[1:], wt.dtype)
    for i in range(len(xmin)):
        acc = np.zeros(a.shape[1:], wt.dtype)
        for j in range(int(size[i])):
            acc = acc + dt(wt[i, j]) * a[int(xmin[i]) + j]
        out[i] = acc
    return np.moveaxis(out, 0, axis)


def round_level(v):
    return np.minimum(v.dtype.type(255), np.maximum(v.dtype.type(0), np.floor(v + v.dtype.type(0.5))))


def resample(src, window, xtab, ytab, fill=0, round_u8=True, div=255.0, mul=2.0, add=-1.0):
    """cd360_picture_resample_u8 -> [C, oh, ow] in the tables' dtype: horizontal pass over every row of the crop, then the vertical one,
    the uint8 roundings after each with round_u8, then (v / div) * mul + add as three operations."""
    dt = xtab[2].dtype.type
    c = crop(src if src.ndim == 3 else src[:, :, None], window, fill)
    t = apply_taps(c, xtab, 1)
    if round_u8:
        t = round_level(t)
    v = apply_taps(t, ytab, 0)
    if round_u8:
        v = round_level(v)
    v = v / dt(div)
    v = v * dt(mul)
    v = v + dt(add)
    return np.ascontiguousarray(np.moveaxis(v, 2, 0))


def levels(src, window, xtab, ytab, fill=0):
    """The round_u8 restatement as grey levels, uint8 [oh, ow, C] (or [oh, ow] for a 2-d source): what is compared with the image
    library's picture."""
    out = np.moveaxis(resample(src, window, xtab, ytab, fill, True, 1.0, 1.0, 0.0), 0, 2).astype(np.uint8)
    return out if src.ndim == 3 else out[:, :, 0]


# ------------------------------------------------------------------------------------------------ the mask's maps
def nearest_index(n_in, n_out):
    i = np.arange(n_out, dtype=np.int64)
    return ((2 * i + 1) * n_in) // (2 * n_out)


def mask_maps(src, window, oh, ow, thr=125, k=7):
    """cd360_picture_mask_u8 -> (opacity, mask, inside), fp32 [oh, ow] each."""
    left, top, w, h = window
    on = crop((src > thr).astype(np.uint8), window, 0)
    ins = crop(np.ones(src.shape, np.uint8), window, 0)
    sy, sx = nearest_index(h, oh), nearest_index(w, ow)
    opacity, inside = on[sy][:, sx].astype(F32), ins[sy][:, sx].astype(F32)
    r = (k - 1) // 2
    pad = np.zeros((oh + 2 * r, ow + 2 * r), F32)
    pad[r:r + oh, r:r + ow] = opacity
    mask = np.zeros((oh, ow), F32)
    for a in range(k):
        for b in range(k):
            mask = np.maximum(mask, pad[a:a + oh, b:b + ow])
    return opacity, mask, inside


# ------------------------------------------------------------------------------------------------ seeded pictures
def picture(H, W, C, seed, kind="noise"):
    """A uint8 picture [H, W, C] ([H, W] for C = 0): uniform noise, or a smooth one (low-frequency waves) with every level in reach."""
    g = np.random.default_rng(seed)
    shape = (H, W) if C == 0 else (H, W, C)
    if kind == "noise":
        return g.integers(0, 256, shape, dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    ph = g.uniform(0, 2 * np.pi, (max(C, 1), 3))
    planes = [127.5 + 127.5 * np.sin(x / W * 5 + p[0]) * np.cos(y / H * 4 + p[1]) * np.sin((x + y) / (H + W) * 3 + p[2]) for p in ph]
    out = np.clip(np.rint(np.stack(planes, -1)), 0, 255).astype(np.uint8)
    return out[:, :, 0] if C == 0 else out


def blob_mask(H, W, seed):
    """A uint8 mask [H, W]: soft blobs around the middle, values across the threshold."""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    v = np.zeros((H, W))
    for _ in range(3):
        cy, cx, s = g.uniform(0.2, 0.8) * H, g.uniform(0.2, 0.8) * W, g.uniform(0.1, 0.25) * min(H, W)
        v = np.maximum(v, np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s)))
    return np.clip(np.rint(v * 255 + g.normal(0, 6, (H, W))), 0, 255).astype(np.uint8)
