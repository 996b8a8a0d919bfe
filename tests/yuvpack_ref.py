"""The numpy model of the packed YUV word formats (include/hmgpu.h "packed YUV"), written from the table of that section and from
nothing in the library: pack() lays planes of D-bit values out as bytes, unpack() reads them back.

  format  cf     D   memory, per unit
  uyvy    4:2:2  8   bytes Cb Y0 Cr Y1 per two pixels
  yuy2    4:2:2  8   bytes Y0 Cb Y1 Cr per two pixels
  y210    4:2:2  10  little-endian uint16 Y0 Cb Y1 Cr, each v << 6
  y216    4:2:2  16  little-endian uint16 Y0 Cb Y1 Cr
  v210    4:2:2  10  six pixels in four little-endian uint32, three 10-bit values per word from bit 0, bits 30-31 zero
  ayuv    4:4:4  8   bytes Cr Cb Y A per pixel
  y410    4:4:4  10  little-endian uint32 Cb | Y << 10 | Cr << 20 | A << 30 per pixel
  y416    4:4:4  16  little-endian uint16 Cb Y Cr A per pixel
"""
import numpy as np

FORMATS = ("uyvy", "yuy2", "y210", "y216", "v210", "ayuv", "y410", "y416")
CHROMA = {"uyvy": 2, "yuy2": 2, "y210": 2, "y216": 2, "v210": 2, "ayuv": 3, "y410": 3, "y416": 3}
DEPTH = {"uyvy": 8, "yuy2": 8, "y210": 10, "y216": 16, "v210": 10, "ayuv": 8, "y410": 10, "y416": 16}
ALPHA_MAX = {"uyvy": 0, "yuy2": 0, "y210": 0, "y216": 0, "v210": 0, "ayuv": 255, "y410": 3, "y416": 65535}
ELEMENT = {"uyvy": 1, "yuy2": 1, "y210": 2, "y216": 2, "v210": 4, "ayuv": 1, "y410": 4, "y416": 2}      # bytes of the unit of alignment
# v210: (plane, index inside the group) of the three fields of each of the four words, from bit 0: Y 0, Cb 1, Cr 2
V210 = (((1, 0), (0, 0), (2, 0)), ((0, 1), (1, 1), (0, 2)), ((2, 1), (0, 3), (1, 2)), ((0, 4), (2, 2), (0, 5)))


def row_bytes(fmt, w):
    """the bytes of one row of w pixels: the least pitch"""
    if fmt == "v210":
        return (w + 5) // 6 * 16
    return {"uyvy": 2, "yuy2": 2, "y210": 4, "y216": 4, "ayuv": 4, "y410": 4, "y416": 8}[fmt] * w


def _le(values, nbytes):
    """[..., K] unsigned integers as [..., K * nbytes] little-endian bytes"""
    v = np.asarray(values, np.uint64)
    out = np.stack([(v >> np.uint64(8 * b)) & np.uint64(0xff) for b in range(nbytes)], axis=-1).astype(np.uint8)
    return out.reshape(v.shape[:-1] + (v.shape[-1] * nbytes,))


def _from_le(b, nbytes):
    """[..., K * nbytes] bytes as [..., K] integers"""
    b = np.asarray(b, np.uint8).astype(np.int64)
    b = b.reshape(b.shape[:-1] + (b.shape[-1] // nbytes, nbytes))
    return sum(b[..., k] << (8 * k) for k in range(nbytes))


def pack(fmt, y, cb, cr, alpha=0, pitch=None, canary=None):
    """planes of DEPTH[fmt]-bit values -- y [H, W]; cb, cr [H, W / 2] (4:2:2) or [H, W] (4:4:4) -- as a uint8 array [H, pitch] (pitch
    None: row_bytes).  Bytes the format does not write hold `canary` (None: 0)"""
    y, cb, cr = (np.asarray(p).astype(np.int64) for p in (y, cb, cr))
    h, w = y.shape
    rb = row_bytes(fmt, w)
    pitch = rb if pitch is None else pitch
    assert pitch >= rb and cb.shape == cr.shape == (h, w // 2 if CHROMA[fmt] == 2 else w) and 0 <= alpha <= ALPHA_MAX[fmt]
    assert all(p.min() >= 0 and p.max() < (1 << DEPTH[fmt]) for p in (y, cb, cr))
    out = np.full((h, pitch), 0 if canary is None else canary, np.uint8)
    a = np.full_like(y, alpha)
    if fmt == "uyvy":
        row = np.stack([cb, y[:, 0::2], cr, y[:, 1::2]], axis=-1).reshape(h, -1)
    elif fmt == "yuy2":
        row = np.stack([y[:, 0::2], cb, y[:, 1::2], cr], axis=-1).reshape(h, -1)
    elif fmt in ("y210", "y216"):
        s = 6 if fmt == "y210" else 0
        row = _le(np.stack([y[:, 0::2], cb, y[:, 1::2], cr], axis=-1).reshape(h, -1) << s, 2)
    elif fmt == "ayuv":
        row = np.stack([cr, cb, y, a], axis=-1).reshape(h, -1)
    elif fmt == "y410":
        row = _le(cb | y << 10 | cr << 20 | a << 30, 4)
    elif fmt == "y416":
        row = _le(np.stack([cb, y, cr, a], axis=-1).reshape(h, -1), 2)
    else:
        groups = (w + 5) // 6
        planes = [np.zeros((h, 6 * groups), np.int64), np.zeros((h, 3 * groups), np.int64), np.zeros((h, 3 * groups), np.int64)]
        planes[0][:, :w], planes[1][:, :w // 2], planes[2][:, :w // 2] = y, cb, cr          # values beyond the width: 0
        words = np.zeros((h, groups, 4), np.int64)
        for k, fields in enumerate(V210):
            for pos, (plane, i) in enumerate(fields):
                per = 6 if plane == 0 else 3
                words[:, :, k] |= planes[plane][:, i::per] << (10 * pos)
        row = _le(words.reshape(h, -1), 4)
    out[:, :rb] = row
    return out


def unpack(fmt, buf, w, h):
    """(y, cb, cr) int64 planes from a uint8 array [H, pitch]: A, bits 30-31 of v210 words and the low six bits of y210 elements are
    read over, and so is everything beyond a row's bytes"""
    b = np.asarray(buf, np.uint8)[:h, :row_bytes(fmt, w)]
    if fmt in ("uyvy", "yuy2"):
        u = b.astype(np.int64).reshape(h, w // 2, 4)
        o = (1, 0, 3, 2) if fmt == "uyvy" else (0, 1, 2, 3)           # positions of Y0, Cb, Y1, Cr
        y = np.stack([u[..., o[0]], u[..., o[2]]], axis=-1).reshape(h, w)
        return y, u[..., o[1]], u[..., o[3]]
    if fmt in ("y210", "y216"):
        u = (_from_le(b, 2) >> (6 if fmt == "y210" else 0)).reshape(h, w // 2, 4)
        return np.stack([u[..., 0], u[..., 2]], axis=-1).reshape(h, w), u[..., 1], u[..., 3]
    if fmt == "ayuv":
        u = b.astype(np.int64).reshape(h, w, 4)
        return u[..., 2], u[..., 1], u[..., 0]
    if fmt == "y410":
        u = _from_le(b, 4)
        return (u >> 10) & 0x3ff, u & 0x3ff, (u >> 20) & 0x3ff
    if fmt == "y416":
        u = _from_le(b, 2).reshape(h, w, 4)
        return u[..., 1], u[..., 0], u[..., 2]
    groups = (w + 5) // 6
    words = _from_le(b, 4).reshape(h, groups, 4)
    planes = [np.zeros((h, 6 * groups), np.int64), np.zeros((h, 3 * groups), np.int64), np.zeros((h, 3 * groups), np.int64)]
    for k, fields in enumerate(V210):
        for pos, (plane, i) in enumerate(fields):
            per = 6 if plane == 0 else 3
            planes[plane][:, i::per] = (words[:, :, k] >> (10 * pos)) & 0x3ff
    return planes[0][:, :w], planes[1][:, :w // 2], planes[2][:, :w // 2]


def mask(fmt, w, h, pitch=None):
    """uint8 [H, pitch]: 1 where pack() writes a byte"""
    rb = row_bytes(fmt, w)
    m = np.zeros((h, rb if pitch is None else pitch), np.uint8)
    m[:, :rb] = 1
    return m
