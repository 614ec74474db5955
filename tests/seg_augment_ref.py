"""The augmentation of include/ivln_seg_augment.h restated in numpy, in a dtype of the caller's choice (float64: the
reference; float32: the arithmetic's own noise, operation for operation what csrc/seg_augment.hip does).  Every index is a
Python integer, exactly as the header defines it; only the rgb values pass through `dtype`.  Not a test file."""
import numpy as np

ONE = 4096
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def scaled_size(n, q):
    return (n * q + ONE // 2) // ONE


def offset_range(n, q):
    d = scaled_size(n, q) - n
    return (0, d) if d >= 0 else (d, 0)


def geometry(H, W, geom):
    """{q, oy, ox, flip} -> dict(ty (H,), tx (W,): the scaled coordinates; ys (H,), xs (W,): the nearest source indices (0
    where outside); inside (H, W) bool), all from Python integers."""
    q, oy, ox, flip = (int(v) for v in geom)
    Hs, Ws = scaled_size(H, q), scaled_size(W, q)
    ty = [y + oy for y in range(H)]
    tx = [((W - 1 - x) if flip else x) + ox for x in range(W)]
    in_y = [0 <= t < Hs for t in ty]
    in_x = [0 <= t < Ws for t in tx]
    ys = [min(((2 * t + 1) * ONE) // (2 * q), H - 1) if ok else 0 for t, ok in zip(ty, in_y)]
    xs = [min(((2 * t + 1) * ONE) // (2 * q), W - 1) if ok else 0 for t, ok in zip(tx, in_x)]
    return dict(q=q, ty=np.array(ty, dtype=np.int64), tx=np.array(tx, dtype=np.int64), ys=np.array(ys, dtype=np.int64),
                xs=np.array(xs, dtype=np.int64), inside=np.outer(np.array(in_y), np.array(in_x)))


def _taps(t, q, n_out, n_rgb, dt):
    """scaled integer coordinates t -> (i0, i1, l): the two edge-clamped taps and the weight of the second, in dt"""
    r = dt(2048) / dt(q)
    f = (2 * t + 1).astype(dt) * r - dt(0.5)
    g = (f + dt(0.5)) * (dt(n_rgb) / dt(n_out)) - dt(0.5)
    g = np.minimum(np.maximum(g, dt(0)), dt(n_rgb - 1))
    i0 = g.astype(np.int64)  # (g >= 0: truncation is the floor)
    i1 = np.minimum(i0 + 1, n_rgb - 1)
    return i0, i1, g - i0.astype(dt)


def augment_image(rgb, depth, labels, geom, photo, ignore_label, dtype=np.float64):
    """rgb u8 (h, w, 3), depth f32 (H, W), labels u8 (H, W), one record -> dict(rgb_n (3, H, W) dtype, depth_n (H, W) dtype,
    depth_src (H, W) f32: the gathered depth with 0 outside, labels_a (H, W) u8, inside (H, W) bool)."""
    dt = np.dtype(dtype).type
    h, w, _ = rgb.shape
    H, W = depth.shape
    geo = geometry(H, W, geom)
    inside = geo["inside"]
    if not inside.all() and ignore_label is None:
        raise ValueError("a record that pads needs an ignore label")
    ks, kv, dv = (dt(np.float32(v)) for v in photo[:3])  # (the kernel's f32 values, promoted)
    src = depth[geo["ys"][:, None], geo["xs"][None, :]]
    depth_src = np.where(inside, src, np.float32(0)).astype(np.float32)
    labels_a = np.where(inside, labels[geo["ys"][:, None], geo["xs"][None, :]], 0 if ignore_label is None else ignore_label)
    depth_n = (depth_src.astype(dt) - dt(0.213)) / dt(0.285)
    # rgb: one bilinear sampling of the original image at the scaled coordinate (outside coordinates computed too, then masked)
    ty, tx = np.maximum(geo["ty"], 0), np.maximum(geo["tx"], 0)
    y0, y1, ly = _taps(ty, geo["q"], H, h, dt)
    x0, x1, lx = _taps(tx, geo["q"], W, w, dt)
    ly, lx = ly[:, None, None], lx[None, :, None]
    p = rgb.astype(dt)
    one = dt(1)
    c = ((one - ly) * ((one - lx) * p[y0[:, None], x0[None, :]] + lx * p[y0[:, None], x1[None, :]])
         + ly * ((one - lx) * p[y1[:, None], x0[None, :]] + lx * p[y1[:, None], x1[None, :]]))  # (H, W, 3)
    v = c.max(axis=2, keepdims=True)
    j = np.minimum(np.maximum(kv * np.maximum(v - ks * (v - c), dt(0)) + dv, dt(0)), dt(255))
    mean, std = np.array(MEAN, dtype=dt), np.array(STD, dtype=dt)
    out = (j / dt(255) - mean) / std
    out = np.where(inside[:, :, None], out, dt(0))
    assert out.dtype == np.dtype(dtype) and depth_n.dtype == np.dtype(dtype)
    return dict(rgb_n=np.ascontiguousarray(out.transpose(2, 0, 1)), depth_n=depth_n, depth_src=depth_src,
                labels_a=labels_a.astype(np.uint8), inside=inside, ys=geo["ys"], xs=geo["xs"])


def augment_batch(rgb, depth, labels, geom, photo, ignore_label, dtype=np.float64):
    """The batch form: rgb (B, h, w, 3), depth (B, H, W), labels (B, H, W), geom (B, 4), photo (B, 4) -> the stacked dict."""
    per = [augment_image(rgb[b], depth[b], labels[b], geom[b], photo[b], ignore_label, dtype) for b in range(len(rgb))]
    return {k: np.stack([p[k] for p in per]) for k in ("rgb_n", "depth_n", "depth_src", "labels_a", "inside")}
