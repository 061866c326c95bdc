"""NumPy model of the JPEG pixel arithmetic and the small host-side helpers the JPEG tests share.

The model is written from libjpeg's definition of its default decoder, whole planes at a time: dequantise, the slow-integer inverse
DCT (jidctint.c: 13-bit constants, column pass keeping 2 extra bits, row pass), level shift and range limit, "fancy" triangle
upsampling (jdsample.c) and the 16-bit fixed-point YCbCr -> RGB of jdcolor.c.  It knows nothing of how csrc/jpeg.hip maps the work
to threads; the GPU tests require the kernel's bytes to equal its output exactly, the CPU tests require its output to be within
5 LSB of Pillow's decode of the same file."""
import ctypes
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg")
REC = 16
PIL_CEILING = 5   # LSB: two conforming IDCTs differ by <= 1 per sample, fancy upsampling rounding adds <= 1 on chroma, the colour
#                   transform amplifies chroma by at most 1.772: 1 + 2 * 1.772 = 4.54


def manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


def fixture_names():
    return [e["name"] for e in manifest()["fixtures"]]


def fixture_bytes(name):
    with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as f:
        return f.read()


def fixture_pixels(name):
    return np.load(os.path.join(GOLDEN, name + ".npy"))


def entropy_decode(data, guard=0, fill=0x5A5A):
    """bsclip_jpeg_entropy_decode of one stream through ctypes -> (rc, coef int16 [coef_count], qtab uint16 [3, 64], rec int32 [16]).
    With ``guard`` > 0 the coefficient buffer sits between two bands of that many int16 filled with ``fill`` and the function
    asserts that the call left them alone."""
    from bioscanclip.hip import lib
    h = lib.load()
    src = np.frombuffer(bytes(data), dtype=np.uint8)
    info = lib.JpegInfo()
    prc = h.bsclip_jpeg_probe(ctypes.c_void_p(src.ctypes.data), src.size, ctypes.byref(info))
    count = int(info.coef_count) if prc == 0 else 64
    buf = np.full(count + 2 * guard, fill, dtype=np.uint16).view(np.int16)
    qtab = np.zeros((3, 64), dtype=np.uint16)
    rec = np.zeros(REC, dtype=np.int32)
    rc = h.bsclip_jpeg_entropy_decode(ctypes.c_void_p(src.ctypes.data), src.size, ctypes.c_void_p(buf.ctypes.data + 2 * guard), count,
                                      ctypes.c_void_p(qtab.ctypes.data), ctypes.c_void_p(rec.ctypes.data))
    if guard:
        g = buf.view(np.uint16)
        assert (g[:guard] == fill).all() and (g[guard + count:] == fill).all(), "entropy decode wrote outside coef_out"
    assert rc == prc or prc == 0, (rc, prc)       # whatever the probe refuses, the decode refuses the same way
    return rc, buf[guard:guard + count], qtab, rec


# ---- the arithmetic -------------------------------------------------------------------------------------------------------
_C = {k: np.int32(v) for k, v in dict(c0298=2446, c0390=3196, c0541=4433, c0765=6270, c0899=7373, c1175=9633, c1501=12299, c1847=15137, c1961=16069, c2053=16819,
          c2562=20995, c3072=25172).items()}


def _idct_1d(v, shift):
    """jpeg_idct_islow's 8-point butterfly along the last axis of an int32 array, descaled by ``shift`` bits with rounding.  NumPy's
    int32 array arithmetic wraps modulo 2^32, which is what the kernel defines for values no 8-bit image encodes; for every other
    stream nothing wraps and this is libjpeg's arithmetic."""
    x = [v[..., i] for i in range(8)]
    z1 = (x[2] + x[6]) * _C["c0541"]
    t2, t3 = z1 - x[6] * _C["c1847"], z1 + x[2] * _C["c0765"]
    t0, t1 = (x[0] + x[4]) * np.int32(8192), (x[0] - x[4]) * np.int32(8192)
    e = [t0 + t3, t1 + t2, t1 - t2, t0 - t3]
    o0, o1, o2, o3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * _C["c1175"]
    z3, z4 = z5 - z3 * _C["c1961"], z5 - z4 * _C["c0390"]
    z1, z2 = -z1 * _C["c0899"], -z2 * _C["c2562"]
    o0 = o0 * _C["c0298"] + z1 + z3
    o1 = o1 * _C["c2053"] + z2 + z4
    o2 = o2 * _C["c3072"] + z2 + z3
    o3 = o3 * _C["c1501"] + z1 + z4
    odd = [o3, o2, o1, o0]
    r = np.int32(1 << (shift - 1))
    out = [(e[i] + odd[i] + r) >> shift for i in range(4)] + [(e[3 - i] - odd[3 - i] + r) >> shift for i in range(4)]
    return np.stack(out, axis=-1)


def _range_limit(v):
    x = v & 1023                                   # libjpeg's wrap-around table: clamp(v + 128) for every legitimate value
    return np.where(x < 128, x + 128, np.where(x < 512, 255, np.where(x < 896, 0, x - 896)))


def _plane(blocks, q, bw, bh):
    """blocks int16 [bh * bw, 64], q uint16 [64] -> uint8-valued int64 plane [bh * 8, bw * 8]."""
    w = (blocks.astype(np.int64).reshape(-1, 8, 8) * q.astype(np.int64).reshape(8, 8)).astype(np.int32)   # |.| < 2^31: exact
    w = np.swapaxes(_idct_1d(np.swapaxes(w, 1, 2), 11), 1, 2)        # columns, 13 - 2 bits
    w = _range_limit(_idct_1d(w, 18).astype(np.int64))                                # rows, 13 + 2 + 3 bits
    return w.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _upsample(pl, hs, vs, W, H):
    """Chroma plane (padded) -> [H, W]: libjpeg's fancy upsampling at the real downsampled size, replication where it falls back."""
    dw, dh = -(-W // hs), -(-H // vs)
    pl = pl[:dh, :dw]
    x, y = np.arange(W), np.arange(H)
    cx, cy = (x >> 1, y >> 1) if (hs, vs) == (2, 2) else (x >> 1, y) if hs == 2 else (x, y >> 1) if vs == 2 else (x, y)
    nx = np.where(x & 1, np.minimum(cx + 1, dw - 1), np.maximum(cx - 1, 0))
    ny = np.where(y & 1, np.minimum(cy + 1, dh - 1), np.maximum(cy - 1, 0))
    if hs == 2 and dw <= 2:                        # jinit_upsampler: fancy h2v1 / h2v2 only when downsampled_width > 2
        return pl[np.ix_(cy, cx)]
    if (hs, vs) == (1, 1):
        return pl[np.ix_(cy, cx)]
    if (hs, vs) == (2, 1):
        return (3 * pl[np.ix_(cy, cx)] + pl[np.ix_(cy, nx)] + np.where(x & 1, 2, 1)[None, :]) >> 2
    if (hs, vs) == (1, 2):
        return (3 * pl[np.ix_(cy, cx)] + pl[np.ix_(ny, cx)] + np.where(y & 1, 2, 1)[:, None]) >> 2
    here = 3 * pl[np.ix_(cy, cx)] + pl[np.ix_(ny, cx)]
    side = 3 * pl[np.ix_(cy, nx)] + pl[np.ix_(ny, nx)]
    return (3 * here + side + np.where(x & 1, 7, 8)[None, :]) >> 4


def model_pixels(coef, qtab, rec):
    """uint8 [H, W, 3] from one image's coefficients, tables and record (as bsclip_jpeg_entropy_decode wrote them)."""
    W, H, nc, hs, vs = (int(rec[i]) for i in (4, 5, 6, 7, 8))
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    grids = [(mx * hs, my * vs)] + [(mx, my)] * (nc - 1)
    planes, off = [], 0
    for c, (bw, bh) in enumerate(grids):
        n = bw * bh
        planes.append(_plane(np.asarray(coef[off:off + 64 * n]).reshape(n, 64), qtab[c], bw, bh))
        off += 64 * n
    assert off == 64 * int(rec[12]) == len(coef)
    Y = planes[0][:H, :W]
    if nc == 1:
        return np.repeat(Y[..., None], 3, axis=2).astype(np.uint8)
    cb, cr = (_upsample(p, hs, vs, W, H) - 128 for p in planes[1:])
    R = Y + ((91881 * cr + 32768) >> 16)
    G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    B = Y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([R, G, B], axis=2), 0, 255).astype(np.uint8)


def decode_all(names=None):
    """[(name, coef, qtab, rec)] of the committed fixtures (every entropy decode must succeed)."""
    out = []
    for name in names or fixture_names():
        rc, coef, qtab, rec = entropy_decode(fixture_bytes(name))
        assert rc == 0, (name, rc)
        out.append((name, coef, qtab, rec))
    return out
