"""What the sync-index tests share: a plain-Python decoder of ONE segment of a baseline JPEG scan, written from the JPEG
specification (ITU-T T.81: B.2 marker segments, C the canonical code construction, F.2.2 the decoding procedures), and the host-side
preparation of a batch for ``bsclip_jpeg_entropy_device``.  The decoder knows nothing of csrc/jpeg_segment.h: it reads bits one at
a time and looks codes up in a dictionary."""
import ctypes

import numpy as np

import jpeg_model as jm

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]

# three damaged streams that tools/jpeg_segments_check.cpp flags on the host under the sanitisers (its "flagged" lines; the CPU test
# asserts that they are printed): (fixture, scan byte, value, status at sync_mcus = 2)
FLAGGED = [("c37x29_420_q75", 0, 0xFF, 4), ("c17x9_444_opt", 0, 0xF7, 1), ("c48x40_420_rst", 0, 0x00, 24)]


def parse_headers(data):
    """{'scan': first entropy-coded byte, 'restart', 'comps': [(h, v, dc id, ac id)], 'mcus_x', 'mcus_y', 'dc' / 'ac': {id: {(len, code): symbol}}}"""
    assert data[:2] == b"\xff\xd8"
    pos, out = 2, {"restart": 0, "dc": {}, "ac": {}}
    while True:
        assert data[pos] == 0xFF
        m, L = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        body = data[pos + 4:pos + 2 + L]
        if m == 0xC4:
            q = 0
            while q < len(body):
                tc, th = body[q] >> 4, body[q] & 15
                counts = list(body[q + 1:q + 17])
                syms = body[q + 17:q + 17 + sum(counts)]
                table, code, k = {}, 0, 0
                for ln in range(1, 17):              # C.2: codes of each length are consecutive, then the code doubles
                    for _ in range(counts[ln - 1]):
                        table[(ln, code)] = syms[k]
                        code, k = code + 1, k + 1
                    code <<= 1
                out["ac" if tc else "dc"][th] = table
                q += 17 + sum(counts)
        elif m == 0xDD:
            out["restart"] = (body[0] << 8) | body[1]
        elif m == 0xC0:
            out["height"], out["width"] = (body[1] << 8) | body[2], (body[3] << 8) | body[4]
            frame = [(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15) for c in range(body[5])]
        elif m == 0xDA:
            sel = {body[1 + 2 * c]: (body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15) for c in range(body[0])}
            out["scan"] = pos + 2 + L
            break
        pos += 2 + L
    if len(frame) == 1:
        frame = [(frame[0][0], 1, 1)]
    out["comps"] = [(h, v, *sel[cid]) for cid, h, v in frame]
    hmax, vmax = max(c[0] for c in out["comps"]), max(c[1] for c in out["comps"])
    out["mcus_x"], out["mcus_y"] = -(-out["width"] // (8 * hmax)), -(-out["height"] // (8 * vmax))
    return out


class _Bits:
    """One bit at a time from (byte, bit); a 0xFF is data only when 0x00 follows, which is then skipped (F.2.2.5)."""

    def __init__(self, data, bitpos):
        self.d, self.pos, self.bit = data, bitpos >> 3, bitpos & 7

    def get(self):
        b = self.d[self.pos]
        if b == 0xFF:
            assert self.d[self.pos + 1] == 0x00, "marker inside a segment"
        v = (b >> (7 - self.bit)) & 1
        self.bit += 1
        if self.bit == 8:
            self.bit, self.pos = 0, self.pos + (2 if b == 0xFF else 1)
        return v

    def receive(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.get()
        return v

    def symbol(self, table):
        code = 0
        for ln in range(1, 17):
            code = (code << 1) | self.get()
            if (ln, code) in table:
                return table[(ln, code)]
        raise AssertionError("unassigned code")

    def where(self):
        return 8 * self.pos + self.bit


def _extend(v, t):
    return v if t == 0 or v >= (1 << (t - 1)) else v - (1 << t) + 1


def decode_segment(data, hdr, entry, count):
    """MCUs [entry[1], entry[1] + count) from the entry alone -> ({(component, block row, block column): int list [64] natural order},
    end bit position, end predictors)."""
    bits = _Bits(data, int(entry[0]))
    cb, cr = int(entry[3]) & 0xFFFF, (int(entry[3]) >> 16) & 0xFFFF
    pred = [int(entry[2]), cb - 65536 if cb >= 32768 else cb, cr - 65536 if cr >= 32768 else cr]
    blocks = {}
    for m in range(int(entry[1]), int(entry[1]) + count):
        my, mx = divmod(m, hdr["mcus_x"])
        for c, (h, v, dcid, acid) in enumerate(hdr["comps"]):
            for y in range(v):
                for x in range(h):
                    zz = [0] * 64
                    t = bits.symbol(hdr["dc"][dcid])
                    pred[c] += _extend(bits.receive(t), t)
                    zz[0] = pred[c]
                    k = 1
                    while k < 64:
                        rs = bits.symbol(hdr["ac"][acid])
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            k += 16
                            continue
                        k += r
                        zz[k] = _extend(bits.receive(s), s)
                        k += 1
                    nat = [0] * 64
                    for i, val in enumerate(zz):
                        nat[ZIGZAG[i]] = val
                    blocks[(c, my * v + y, mx * h + x)] = nat
    return blocks, bits.where(), pred


def raster(hdr, coef):
    """The host decoder's coefficient raster as {(component, block row, block column): int list [64]}."""
    out, off = {}, 0
    for c, (h, v, _, _) in enumerate(hdr["comps"]):
        bw, bh = hdr["mcus_x"] * h, hdr["mcus_y"] * v
        plane = np.asarray(coef[off:off + 64 * bw * bh]).reshape(bh, bw, 64)
        for by in range(bh):
            for bx in range(bw):
                out[(c, by, bx)] = [int(t) for t in plane[by, bx]]
        off += 64 * bw * bh
    assert off == len(coef)
    return out


def segment_firsts(nmcu, restart, sync_mcus):
    """First MCU of every segment: MCU 0, the first MCU of every restart interval, every sync_mcus MCUs inside an interval."""
    R = restart if 0 < restart <= nmcu else nmcu
    return [lo + k for lo in range(0, nmcu, R) for k in range(0, min(R, nmcu - lo), sync_mcus)]


# ---- a batch for bsclip_jpeg_entropy_device ------------------------------------------------------------------------------
def device_tables(data):
    """bsclip_jpeg_device_tables of one stream -> (huff uint8 [4 * JPEG_HUFF_BYTES], qtab uint16 [3, 64], rec int32 [16])."""
    from bioscanclip.hip import lib, ops
    src = np.frombuffer(bytes(data), dtype=np.uint8)
    huff = np.zeros(4 * lib.JPEG_HUFF_BYTES, dtype=np.uint8)
    qtab, rec = np.zeros((3, 64), dtype=np.uint16), np.zeros(lib.JPEG_REC, dtype=np.int32)
    ops.jpeg_device_tables(src.ctypes.data, src.size, huff.ctypes.data, qtab.ctypes.data, rec.ctypes.data)
    return huff, qtab, rec


def batch(streams, sync_mcus, index_from=None, gap=3):
    """Host arrays of one launch over ``streams``: bytes back to back with ``gap`` stray 0xFF bytes between them, index entries,
    tables, records and segment records.  ``index_from``: the (intact) streams the index and tables are made from, when ``streams``
    are damaged copies."""
    from bioscanclip.hip import ops
    clean = streams if index_from is None else index_from
    B = len(streams)
    idx = [ops.jpeg_sync_index(s, sync_mcus) for s in clean]
    tabs = [device_tables(s) for s in clean]
    rec = np.stack([t[2] for t in tabs]).astype(np.int32)
    counts = 64 * rec[:, 12].astype(np.int64)
    coef_off = np.concatenate([[0], np.cumsum(counts)])
    rec[:, 0] = coef_off[:B]
    seg = np.zeros((B, 8), dtype=np.int32)
    blob, eo = bytearray(), 0
    for k, s in enumerate(streams):
        blob += b"\xff" * gap
        seg[k] = (len(blob), len(s), eo, len(idx[k]), sync_mcus, k, 0, 0)
        blob += bytes(s)
        eo += len(idx[k])
    return {"bytes": np.frombuffer(bytes(blob), dtype=np.uint8).copy(), "sync": np.concatenate(idx).astype(np.int32),
            "huff": np.stack([t[0] for t in tabs]), "qtab": np.concatenate([t[1] for t in tabs]), "rec": rec, "seg": seg,
            "coef_off": coef_off, "ncoef": int(coef_off[-1])}


def ptr(a):
    return ctypes.c_void_p(a.ctypes.data)
