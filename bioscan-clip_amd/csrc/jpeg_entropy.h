// Host half of the JPEG decode: marker parsing and Huffman decoding of baseline sequential 8-bit streams into quantised
// coefficients.  Plain C++ (no HIP headers), no allocation (all state lives in a Decoder on the caller's stack), no globals:
// safe to call from any number of loader threads at once.  The data-parallel half (dequantise, inverse DCT, upsampling,
// colour) is csrc/jpeg.hip.  At the end of this file: the sync index and the device-ready tables with which the same coefficients
// are decoded on the device instead (csrc/jpeg_segment.h, csrc/jpeg_entropy.hip); the decoder itself does not use them.
//
// Accepted: SOF0, 8-bit, one component (grey) or three (YCbCr) with luma sampling H, V in {1, 2} and chroma 1x1 (4:4:4, 4:2:2,
// 4:4:0, 4:2:0), one interleaved scan, restart intervals, any size up to 4096 x 4096.  Everything else is refused with a code
// of its own before a single coefficient is written.
//
// Coefficient layout (what jpeg.hip reads): per component, in frame order, a raster of 8x8 blocks padded to whole MCUs --
// component c has bw_c = mcus_x * h_c blocks per row and bh_c = mcus_y * v_c block rows -- each block 64 int16 in natural
// (de-zigzagged) order, DC prediction undone.  Quantisation tables: one uint16[64] per component, natural order.
//
// Damage policy: a stream that ends early, runs into a marker before its last MCU, holds a code no table assigns, an
// out-of-range run length or a missing / out-of-order restart marker is an ERROR (ERR_TRUNCATED / ERR_CORRUPT); nothing is
// zero-filled and the caller must not use the coefficient buffer.  Every read is bounded by the input length, every write by
// the caller's capacity (checked once, before decoding, against the size the frame header implies).
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "jpeg_segment.h"

namespace bsclip_jpeg {

enum : int {
    OK = 0,
    ERR_ARGS = -1,            // null pointer / buffer too small (BSCLIP_ERR_INVALID)
    ERR_TRUNCATED = -10,      // the bytes end (or a marker arrives) before the headers / the last MCU
    ERR_CORRUPT = -11,        // malformed segment, unassigned Huffman code, bad run length, wrong restart marker
    ERR_SOF = -12,            // any frame type but SOF0 at 8 bits: extended, progressive, lossless, arithmetic, 12-bit
    ERR_COMPONENTS = -13,     // component count other than 1 or 3
    ERR_SAMPLING = -14,       // sampling factors outside luma {1,2}x{1,2}, chroma 1x1
    ERR_MULTISCAN = -15,      // the first scan does not carry every component
    ERR_MISSING_TABLE = -16,  // a quantisation or Huffman table the scan refers to was never defined
    ERR_SIZE = -17,           // zero or > 4096 in a dimension
    ERR_COLORSPACE = -18,     // three components that are not YCbCr (Adobe transform 0 / component ids R, G, B)
};

constexpr int MAX_DIM = 4096;
constexpr int REC = 16;  // int32 per image record, see Frame::write_record

static const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
    bool defined;
    uint16_t look[512];    // 9-bit prefix -> (length << 8) | symbol, 0 = longer than 9 bits (or unassigned)
    int32_t maxcode[18];   // largest code of each length, -1 if none
    int32_t valoff[17];    // index of the first symbol of a length minus its first code
    uint8_t vals[256];
    int nvals;
};

struct Frame {
    int width, height, ncomp, hs, vs;    // hs, vs: luma sampling factors (1 x 1 for grey)
    int mcus_x, mcus_y, restart;
    int qsel[3], dcsel[3], acsel[3];
    int bw[3], bh[3];                    // block grid of each component, padded to whole MCUs
    int64_t comp_off[3];                 // first coefficient of each component
    int64_t coef_count;                  // int16 coefficients of the image = bytes of planar scratch jpeg.hip needs
    int64_t pixel_bytes;                 // width * height * 3
    size_t scan_pos;                     // first entropy-coded byte
};

struct Decoder {
    const uint8_t* p;
    size_t n;
    uint16_t qt[4][64];   // natural order
    bool qt_defined[4];
    Huff dc[4], ac[4];
    Frame f;
    char msg[160];

    int fail(int code, const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, sizeof(msg), fmt, ap);
        va_end(ap);
        return code;
    }

    // ---- tables ----------------------------------------------------------------------------------------------------
    int read_dqt(size_t pos, size_t end) {
        while (pos < end) {
            const int pq = p[pos] >> 4, tq = p[pos] & 15;
            ++pos;
            if (pq > 1 || tq > 3) return fail(ERR_CORRUPT, "corrupt stream: DQT precision %d table %d", pq, tq);
            const size_t need = pq ? 128 : 64;
            if (end - pos < need) return fail(ERR_CORRUPT, "corrupt stream: DQT segment shorter than its table");
            for (int k = 0; k < 64; ++k) {
                const unsigned v = pq ? (unsigned)((p[pos + 2 * k] << 8) | p[pos + 2 * k + 1]) : p[pos + k];
                qt[tq][ZIGZAG[k]] = (uint16_t)v;
            }
            qt_defined[tq] = true;
            pos += need;
        }
        return OK;
    }

    int read_dht(size_t pos, size_t end) {
        while (pos < end) {
            const int tc = p[pos] >> 4, th = p[pos] & 15;
            ++pos;
            if (tc > 1 || th > 3) return fail(ERR_CORRUPT, "corrupt stream: DHT class %d table %d", tc, th);
            if (end - pos < 16) return fail(ERR_CORRUPT, "corrupt stream: DHT segment shorter than its counts");
            const uint8_t* bits = p + pos;
            int total = 0;
            for (int i = 0; i < 16; ++i) total += bits[i];
            pos += 16;
            if (total > 256 || end - pos < (size_t)total) return fail(ERR_CORRUPT, "corrupt stream: DHT with %d symbols", total);
            Huff& h = tc ? ac[th] : dc[th];
            h.defined = false;
            memset(h.look, 0, sizeof(h.look));
            memcpy(h.vals, p + pos, (size_t)total);
            h.nvals = total;
            pos += (size_t)total;
            int code = 0, k = 0;
            for (int len = 1; len <= 16; ++len) {
                const int cnt = bits[len - 1];
                h.valoff[len] = k - code;
                if (code + cnt > (1 << len)) return fail(ERR_CORRUPT, "corrupt stream: DHT codes overflow length %d", len);
                for (int i = 0; i < cnt; ++i, ++k, ++code) {
                    if (len <= 9) {
                        const int lo = code << (9 - len), span = 1 << (9 - len);
                        for (int j = 0; j < span; ++j) h.look[lo + j] = (uint16_t)((len << 8) | h.vals[k]);
                    }
                }
                h.maxcode[len] = cnt ? code - 1 : -1;
                code <<= 1;
            }
            h.maxcode[17] = 0x7fffffff;
            h.defined = true;
        }
        return OK;
    }

    // ---- headers: everything up to and including the SOS header -----------------------------------------------------
    int parse(const uint8_t* bytes, size_t len) {
        p = bytes;
        n = len;
        msg[0] = 0;
        memset(qt_defined, 0, sizeof(qt_defined));
        for (int i = 0; i < 4; ++i) dc[i].defined = ac[i].defined = false;
        memset(&f, 0, sizeof(f));
        if (!bytes) return fail(ERR_ARGS, "null input");
        if (n < 4 || p[0] != 0xFF || p[1] != 0xD8) return fail(n < 4 ? ERR_TRUNCATED : ERR_CORRUPT, "not a JPEG stream (no SOI)");
        size_t pos = 2;
        bool have_sof = false, adobe_rgb = false;
        int cid[3] = {0, 0, 0};
        for (;;) {
            if (pos + 2 > n) return fail(ERR_TRUNCATED, "truncated stream: headers end at byte %zu", n);
            if (p[pos] != 0xFF) return fail(ERR_CORRUPT, "corrupt stream: byte 0x%02X at %zu where a marker belongs", p[pos], pos);
            while (pos < n && p[pos] == 0xFF) ++pos;      // fill bytes
            if (pos >= n) return fail(ERR_TRUNCATED, "truncated stream: headers end at byte %zu", n);
            const int m = p[pos++];
            if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;   // TEM / stray RSTn: no payload
            if (m == 0xD8) return fail(ERR_CORRUPT, "corrupt stream: second SOI");
            if (m == 0xD9) return fail(ERR_TRUNCATED, "truncated stream: EOI before any scan");
            if (m == 0x00) return fail(ERR_CORRUPT, "corrupt stream: stuffed byte among the headers");
            if (pos + 2 > n) return fail(ERR_TRUNCATED, "truncated stream: marker 0x%02X has no length", m);
            const size_t L = (size_t)((p[pos] << 8) | p[pos + 1]);
            if (L < 2) return fail(ERR_CORRUPT, "corrupt stream: marker 0x%02X with length %zu", m, L);
            if (L > n - pos) return fail(ERR_TRUNCATED, "truncated stream: marker 0x%02X runs past the end", m);
            const size_t body = pos + 2, end = pos + L;
            if (m == 0xDB) {
                const int rc = read_dqt(body, end);
                if (rc) return rc;
            } else if (m == 0xC4) {
                const int rc = read_dht(body, end);
                if (rc) return rc;
            } else if (m == 0xDD) {
                if (L != 4) return fail(ERR_CORRUPT, "corrupt stream: DRI length %zu", L);
                f.restart = (p[body] << 8) | p[body + 1];
            } else if (m == 0xEE) {   // Adobe: transform 0 with three components means RGB
                if (L >= 14 && memcmp(p + body, "Adobe", 5) == 0 && p[body + 11] == 0) adobe_rgb = true;
            } else if (m == 0xC0) {
                if (have_sof) return fail(ERR_CORRUPT, "corrupt stream: second frame header");
                if (L < 8) return fail(ERR_CORRUPT, "corrupt stream: SOF0 length %zu", L);
                const int prec = p[body];
                f.height = (p[body + 1] << 8) | p[body + 2];
                f.width = (p[body + 3] << 8) | p[body + 4];
                f.ncomp = p[body + 5];
                if (prec != 8) return fail(ERR_SOF, "unsupported JPEG: %d-bit samples (only 8-bit baseline)", prec);
                if (f.ncomp != 1 && f.ncomp != 3)
                    return fail(ERR_COMPONENTS, "unsupported JPEG: %d components (only grey and YCbCr)", f.ncomp);
                if (L != (size_t)(8 + 3 * f.ncomp)) return fail(ERR_CORRUPT, "corrupt stream: SOF0 length %zu for %d components", L, f.ncomp);
                if (f.width < 1 || f.height < 1 || f.width > MAX_DIM || f.height > MAX_DIM)
                    return fail(ERR_SIZE, "unsupported JPEG: %d x %d (1..%d per side)", f.width, f.height, MAX_DIM);
                int h[3], v[3];
                for (int c = 0; c < f.ncomp; ++c) {
                    cid[c] = p[body + 6 + 3 * c];
                    h[c] = p[body + 7 + 3 * c] >> 4;
                    v[c] = p[body + 7 + 3 * c] & 15;
                    f.qsel[c] = p[body + 8 + 3 * c];
                    if (f.qsel[c] > 3) return fail(ERR_CORRUPT, "corrupt stream: quantisation table %d", f.qsel[c]);
                    if (h[c] < 1 || h[c] > 4 || v[c] < 1 || v[c] > 4) return fail(ERR_CORRUPT, "corrupt stream: sampling %dx%d", h[c], v[c]);
                }
                if (f.ncomp == 1) {
                    f.hs = f.vs = 1;   // a one-component scan is never interleaved: its MCU is one block whatever the factors say
                } else {
                    if (h[0] > 2 || v[0] > 2 || h[1] != 1 || v[1] != 1 || h[2] != 1 || v[2] != 1)
                        return fail(ERR_SAMPLING, "unsupported JPEG: sampling %dx%d,%dx%d,%dx%d (luma 1 or 2 per axis, chroma 1x1)",
                                    h[0], v[0], h[1], v[1], h[2], v[2]);
                    f.hs = h[0];
                    f.vs = v[0];
                }
                have_sof = true;
            } else if ((m >= 0xC1 && m <= 0xCF) && m != 0xC4 && m != 0xC8) {
                static const char* const kind[16] = {"", "extended sequential", "progressive", "lossless", "", "differential sequential",
                                                     "differential progressive", "differential lossless", "", "arithmetic sequential",
                                                     "arithmetic progressive", "arithmetic lossless", "arithmetic-coding tables",
                                                     "arithmetic differential", "arithmetic differential progressive",
                                                     "arithmetic differential lossless"};
                return fail(ERR_SOF, "unsupported JPEG: SOF%d (%s); only baseline SOF0 is decoded", m - 0xC0, kind[m - 0xC0]);
            } else if (m == 0xDA) {
                if (!have_sof) return fail(ERR_CORRUPT, "corrupt stream: scan before the frame header");
                if (L < 3) return fail(ERR_CORRUPT, "corrupt stream: SOS length %zu", L);
                const int ns = p[body];
                if (L != (size_t)(6 + 2 * ns)) return fail(ERR_CORRUPT, "corrupt stream: SOS length %zu for %d components", L, ns);
                if (ns != f.ncomp)
                    return fail(ERR_MULTISCAN, "unsupported JPEG: first scan carries %d of %d components (multi-scan file)", ns, f.ncomp);
                for (int c = 0; c < ns; ++c) {
                    if (p[body + 1 + 2 * c] != cid[c]) return fail(ERR_MULTISCAN, "unsupported JPEG: scan components out of frame order");
                    f.dcsel[c] = p[body + 2 + 2 * c] >> 4;
                    f.acsel[c] = p[body + 2 + 2 * c] & 15;
                    if (f.dcsel[c] > 3 || f.acsel[c] > 3) return fail(ERR_CORRUPT, "corrupt stream: Huffman table selector");
                    if (!dc[f.dcsel[c]].defined || !ac[f.acsel[c]].defined)
                        return fail(ERR_MISSING_TABLE, "missing table: Huffman table DC %d / AC %d is not defined", f.dcsel[c], f.acsel[c]);
                    if (!qt_defined[f.qsel[c]]) return fail(ERR_MISSING_TABLE, "missing table: quantisation table %d is not defined", f.qsel[c]);
                }
                if (p[body + 1 + 2 * ns] != 0 || p[body + 2 + 2 * ns] != 63 || p[body + 3 + 2 * ns] != 0)
                    return fail(ERR_SOF, "unsupported JPEG: scan with spectral selection / successive approximation");
                if (f.ncomp == 3 && (adobe_rgb || (cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B')))
                    return fail(ERR_COLORSPACE, "unsupported JPEG: three components that are RGB, not YCbCr");
                f.scan_pos = end;
                break;
            }
            pos = end;
        }
        f.mcus_x = (f.width + 8 * f.hs - 1) / (8 * f.hs);
        f.mcus_y = (f.height + 8 * f.vs - 1) / (8 * f.vs);
        int64_t off = 0;
        for (int c = 0; c < f.ncomp; ++c) {
            f.bw[c] = f.mcus_x * (c == 0 ? f.hs : 1);
            f.bh[c] = f.mcus_y * (c == 0 ? f.vs : 1);
            f.comp_off[c] = off;
            off += (int64_t)f.bw[c] * f.bh[c] * 64;
        }
        f.coef_count = off;
        f.pixel_bytes = (int64_t)f.width * f.height * 3;
        return OK;
    }

    // ---- entropy-coded segment ------------------------------------------------------------------------------------
    // Bit reader: a 64-bit window refilled a byte at a time; 0xFF00 is one 0xFF data byte; at a marker or the end of the input it
    // feeds zeros and counts them, and a block that consumed any of them is an error.
    struct Bits {
        const uint8_t* p;
        size_t pos, n;
        uint64_t acc;
        int cnt, fake;   // bits in acc; how many of them (the newest) are made-up zeros
        void fill() {
            while (cnt <= 56) {
                unsigned b = 0;
                bool real = false;
                if (fake == 0 && pos < n) {
                    b = p[pos];
                    if (b != 0xFF) {
                        ++pos;
                        real = true;
                    } else if (pos + 1 < n && p[pos + 1] == 0x00) {
                        pos += 2;
                        real = true;
                    }
                }
                if (!real) {
                    b = 0;
                    fake += 8;
                }
                acc = (acc << 8) | b;
                cnt += 8;
            }
        }
        unsigned peek(int k) const { return (unsigned)((acc >> (cnt - k)) & ((1u << k) - 1)); }
        void skip(int k) { cnt -= k; }
        bool overran() const { return cnt < fake; }
    };

    static int decode_symbol(Bits& b, const Huff& h) {   // >= 0: symbol, -1: no such code
        const unsigned e = h.look[b.peek(9)];
        if (e) {
            b.skip(e >> 8);
            return e & 0xff;
        }
        int code = (int)b.peek(9);
        for (int len = 10; len <= 16; ++len) {
            code = (int)b.peek(len);
            if (h.maxcode[len] >= 0 && code <= h.maxcode[len]) {
                const int idx = code + h.valoff[len];
                if (idx < 0 || idx >= h.nvals) return -1;
                b.skip(len);
                return h.vals[idx];
            }
        }
        return -1;
    }

    static int extend(unsigned v, int s) { return v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

    int decode_block(Bits& b, const Huff& hd, const Huff& ha, int& pred, int16_t* blk) {
        memset(blk, 0, 64 * sizeof(int16_t));
        b.fill();
        int s = decode_symbol(b, hd);
        if (s < 0 || s > 15) return fail(ERR_CORRUPT, "corrupt stream: unassigned DC code near byte %zu", b.pos);
        int diff = 0;
        if (s) {
            diff = extend(b.peek(s), s);
            b.skip(s);
        }
        pred = (int16_t)(pred + diff);   // legitimate DC values span 12 bits; a corrupt stream wraps instead of overflowing
        blk[0] = (int16_t)pred;
        for (int k = 1; k < 64;) {
            b.fill();                    // >= 57 bits: enough for a 16-bit code and its 15 value bits
            const int rs = decode_symbol(b, ha);
            if (rs < 0) return fail(ERR_CORRUPT, "corrupt stream: unassigned AC code near byte %zu", b.pos);
            const int r = rs >> 4;
            s = rs & 15;
            if (s == 0) {
                if (r != 15) break;      // end of block
                k += 16;
                continue;
            }
            k += r;
            if (k > 63) return fail(ERR_CORRUPT, "corrupt stream: run length past the block near byte %zu", b.pos);
            blk[ZIGZAG[k]] = (int16_t)extend(b.peek(s), s);
            b.skip(s);
            ++k;
        }
        if (b.overran()) return fail(ERR_TRUNCATED, "truncated stream: entropy data ends at byte %zu before the last block", b.pos);
        return OK;
    }

    // coef: f.coef_count int16 (the caller checked its capacity)
    int decode_scan(int16_t* coef) {
        Bits b{p, f.scan_pos, n, 0, 0, 0};
        int pred[3] = {0, 0, 0};
        int todo = f.restart, next_rst = 0;
        for (int my = 0; my < f.mcus_y; ++my) {
            for (int mx = 0; mx < f.mcus_x; ++mx) {
                if (f.restart && todo == 0) {
                    // byte-align: the window may still hold the interval's padding bits (fewer than 8 real ones; the reader never
                    // takes marker bytes in), then the marker itself is at pos
                    size_t at = b.pos;
                    if (b.cnt - b.fake >= 8) return fail(ERR_CORRUPT, "corrupt stream: data where RST%d belongs near byte %zu", next_rst, at);
                    while (at < n && p[at] == 0xFF && at + 1 < n && p[at + 1] == 0xFF) ++at;
                    if (at + 2 > n) return fail(ERR_TRUNCATED, "truncated stream: ends where RST%d belongs", next_rst);
                    if (p[at] != 0xFF || p[at + 1] != 0xD0 + next_rst)
                        return fail(ERR_CORRUPT, "corrupt stream: 0x%02X%02X where RST%d belongs at byte %zu", p[at], p[at + 1], next_rst, at);
                    b = Bits{p, at + 2, n, 0, 0, 0};
                    next_rst = (next_rst + 1) & 7;
                    pred[0] = pred[1] = pred[2] = 0;
                    todo = f.restart;
                }
                for (int c = 0; c < f.ncomp; ++c) {
                    const int hc = c == 0 ? f.hs : 1, vc = c == 0 ? f.vs : 1;
                    for (int v = 0; v < vc; ++v)
                        for (int h = 0; h < hc; ++h) {
                            const int64_t blk = (int64_t)(my * vc + v) * f.bw[c] + (mx * hc + h);
                            const int rc = decode_block(b, dc[f.dcsel[c]], ac[f.acsel[c]], pred[c], coef + f.comp_off[c] + blk * 64);
                            if (rc) return rc;
                        }
                }
                --todo;
            }
        }
        return OK;
    }

    // The 16-int record jpeg.hip reads.  The decoder fills in the image's own fields; the three batch fields (where its
    // coefficients and pixels live, and which table slots are its) start at zero / 0,1,2 and are the caller's to place.
    //   0,1 coefficient offset (int16 elements, low / high word; also the image's byte offset in the planar scratch)
    //   2,3 output offset (bytes, low / high)     4 W   5 H   6 components   7 luma h   8 luma v
    //   9,10,11 quantisation-table slot of each component     12 blocks of all components (= coefficients / 64)
    //   13 restart interval (informative)   14, 15 zero
    void write_record(int32_t* rec) const {
        memset(rec, 0, REC * sizeof(int32_t));
        rec[4] = f.width;
        rec[5] = f.height;
        rec[6] = f.ncomp;
        rec[7] = f.hs;
        rec[8] = f.vs;
        rec[9] = 0;
        rec[10] = f.ncomp == 3 ? 1 : 0;
        rec[11] = f.ncomp == 3 ? 2 : 0;
        rec[12] = (int32_t)(f.coef_count / 64);
        rec[13] = f.restart;
    }
};

// blocks (of all components) that a record's W, H, components and sampling imply; 0 if they are outside what is decoded
inline int64_t record_blocks(int W, int H, int ncomp, int hs, int vs) {
    if (W < 1 || H < 1 || W > MAX_DIM || H > MAX_DIM || (ncomp != 1 && ncomp != 3) || hs < 1 || hs > 2 || vs < 1 || vs > 2) return 0;
    if (ncomp == 1 && (hs != 1 || vs != 1)) return 0;
    const int64_t mx = (W + 8 * hs - 1) / (8 * hs), my = (H + 8 * vs - 1) / (8 * vs);
    return mx * my * (hs * vs + (ncomp == 3 ? 2 : 0));
}

// Decode one image.  coef_out: coef_capacity int16; qtab_out: 3 x 64 uint16 (one table per component, unused ones zero);
// record_out: REC int32.  Returns OK or an error code, with text in `msg` (msg_len bytes, may be null).
inline int entropy_decode(const uint8_t* bytes, size_t n, int16_t* coef_out, int64_t coef_capacity, uint16_t* qtab_out,
                          int32_t* record_out, char* msg, size_t msg_len) {
    Decoder d;
    int rc;
    if (!bytes || !coef_out || !qtab_out || !record_out) rc = d.fail(ERR_ARGS, "null pointer");
    else rc = d.parse(bytes, n);
    if (rc == OK && d.f.coef_count > coef_capacity)
        rc = d.fail(ERR_ARGS, "coefficient buffer holds %lld int16 but the image needs %lld", (long long)coef_capacity, (long long)d.f.coef_count);
    if (rc == OK) rc = d.decode_scan(coef_out);
    if (rc == OK) {
        memset(qtab_out, 0, 3 * 64 * sizeof(uint16_t));
        for (int c = 0; c < d.f.ncomp; ++c) memcpy(qtab_out + 64 * c, d.qt[d.f.qsel[c]], 64 * sizeof(uint16_t));
        d.write_record(record_out);
    }
    if (rc != OK && msg && msg_len) snprintf(msg, msg_len, "%s", d.msg);
    return rc;
}

// ---- the sync index and the device-ready tables ("entropy decode on the device") -----------------------------------
// The four tables a scan selects, in the segment decoder's form, and the selector word that says which each component uses.  A scan
// whose components select more than two DC or more than two AC tables (baseline allows two of each) is refused.
inline void seg_huff_from(const Huff& h, SegHuff* o) {
    memset(o, 0, sizeof(*o));
    memcpy(o->look, h.look, sizeof(o->look));
    for (int len = 1; len <= 16; ++len) o->maxcode[len] = h.maxcode[len], o->valoff[len] = h.valoff[len];
    o->maxcode[0] = -1;
    o->nvals = h.nvals;
    memcpy(o->vals, h.vals, sizeof(o->vals));
}

inline int seg_tables(Decoder& d, SegHuff* tabs, int* sel_out) {
    int dcid[2] = {-1, -1}, acid[2] = {-1, -1}, sel = 0;
    for (int c = 0; c < d.f.ncomp; ++c) {
        int sd = -1, sa = -1;
        for (int k = 0; k < 2 && sd < 0; ++k)
            if (dcid[k] < 0 || dcid[k] == d.f.dcsel[c]) dcid[k] = d.f.dcsel[c], sd = k;
        for (int k = 0; k < 2 && sa < 0; ++k)
            if (acid[k] < 0 || acid[k] == d.f.acsel[c]) acid[k] = d.f.acsel[c], sa = k;
        if (sd < 0 || sa < 0) return d.fail(ERR_SOF, "unsupported JPEG: the scan selects more than two DC or two AC Huffman tables");
        sel |= (sd << c) | (sa << (4 + c));
    }
    for (int k = 0; k < 2; ++k) {
        seg_huff_from(d.dc[dcid[k] < 0 ? dcid[0] : dcid[k]], tabs + k);
        seg_huff_from(d.ac[acid[k] < 0 ? acid[0] : acid[k]], tabs + 2 + k);
    }
    *sel_out = sel;
    return OK;
}

inline SegGeom seg_geom(const Frame& f, int sel) { return SegGeom{f.ncomp, f.hs, f.vs, f.mcus_x, f.mcus_x * f.mcus_y, sel}; }

// Headers of one stream -> SEG_TABLES device-ready Huffman tables, the quantisation tables (3 x 64 uint16) and the 16-int record
// with word 14 = the selector word (the pixel kernels ignore it).  Decodes nothing.
inline int device_tables(const uint8_t* bytes, size_t n, SegHuff* huff_out, uint16_t* qtab_out, int32_t* record_out, char* msg,
                         size_t msg_len) {
    Decoder d;
    int rc, sel = 0;
    if (!bytes || !huff_out || !qtab_out || !record_out) rc = d.fail(ERR_ARGS, "null pointer");
    else rc = d.parse(bytes, n);
    if (rc == OK) rc = seg_tables(d, huff_out, &sel);
    if (rc == OK) {
        memset(qtab_out, 0, 3 * 64 * sizeof(uint16_t));
        for (int c = 0; c < d.f.ncomp; ++c) memcpy(qtab_out + 64 * c, d.qt[d.f.qsel[c]], 64 * sizeof(uint16_t));
        d.write_record(record_out);
        record_out[14] = sel;
    }
    if (rc != OK && msg && msg_len) snprintf(msg, msg_len, "%s", d.msg);
    return rc;
}

// The sync index of one stream: SYNC_ENTRY int32 per segment (segment_range says which MCUs each covers).  Walks the scan with the
// segment decoder itself, storing nothing, so an indexed stream is one the device decodes with status 0.  out == null: returns the
// entry count, which the frame, the restart interval and sync_mcus fix.  Otherwise returns the count written or an error code: the
// decoder's own for everything the decoder refuses, ERR_ARGS for a stream of 2^28 bytes or more, sync_mcus < 1 or a short buffer,
// ERR_CORRUPT for data bytes between the last MCU and the marker that ends an interval or the scan.
inline int64_t sync_index(const uint8_t* bytes, size_t n, int sync_mcus, int32_t* out, int64_t capacity, char* msg, size_t msg_len) {
    Decoder d;
    SegHuff tabs[SEG_TABLES];
    int rc, sel = 0;
    int64_t count = 0;
    if (!bytes) rc = d.fail(ERR_ARGS, "null input");
    else if (n >= (size_t)MAX_STREAM) rc = d.fail(ERR_ARGS, "stream of %zu bytes: the index holds bit positions of streams below 2^28 bytes", n);
    else if (sync_mcus < 1) rc = d.fail(ERR_ARGS, "sync_mcus=%d must be at least 1", sync_mcus);
    else rc = d.parse(bytes, n);
    if (rc == OK) rc = seg_tables(d, tabs, &sel);
    if (rc == OK) {
        const SegGeom g = seg_geom(d.f, sel);
        count = segment_count(g.nmcu, d.f.restart, sync_mcus);
        if (out && capacity < count) rc = d.fail(ERR_ARGS, "index buffer holds %lld entries but the stream needs %lld", (long long)capacity, (long long)count);
        if (out && rc == OK) {
            int32_t e[SYNC_ENTRY] = {(int32_t)(d.f.scan_pos * 8), 0, 0, 0};
            int next_rst = 0;
            for (int j = 0; j < (int)count && rc == OK; ++j) {
                int first, cnt;
                bool chained;
                segment_range(j, g.nmcu, d.f.restart, sync_mcus, &first, &cnt, &chained);
                e[1] = first;
                memcpy(out + (size_t)j * SYNC_ENTRY, e, sizeof(e));
                SegEnd end;
                const int st = decode_segment<false>(bytes, (uint32_t)n, e, first, cnt, g, tabs, nullptr, &end);
                if (st & SEG_OVERRUN) rc = d.fail(ERR_TRUNCATED, "truncated stream: entropy data ends before MCU %d", first + cnt);
                else if (st) rc = d.fail(ERR_CORRUPT, "corrupt stream: unassigned code or run length past the block in MCUs %d..%d", first, first + cnt - 1);
                else if (chained) {
                    e[0] = end.bitpos, e[2] = end.pred[0];
                    e[3] = g.ncomp == 3 ? pack_chroma(end.pred[1], end.pred[2]) : 0;
                } else {
                    if (end.real >= 8) rc = d.fail(ERR_CORRUPT, "corrupt stream: data where a marker belongs near byte %u", end.fetch);
                    if (rc == OK && first + cnt < g.nmcu) {   // the restart marker, found as the decoder finds it
                        size_t at = end.fetch;
                        while (at < n && bytes[at] == 0xFF && at + 1 < n && bytes[at + 1] == 0xFF) ++at;
                        if (at + 2 > n) rc = d.fail(ERR_TRUNCATED, "truncated stream: ends where RST%d belongs", next_rst);
                        else if (bytes[at] != 0xFF || bytes[at + 1] != 0xD0 + next_rst)
                            rc = d.fail(ERR_CORRUPT, "corrupt stream: 0x%02X%02X where RST%d belongs at byte %zu", bytes[at], bytes[at + 1], next_rst, at);
                        else if (at + 2 >= n) rc = d.fail(ERR_TRUNCATED, "truncated stream: ends after RST%d", next_rst);
                        next_rst = (next_rst + 1) & 7;
                        e[0] = (int32_t)((at + 2) * 8), e[2] = e[3] = 0;
                    }
                }
            }
        }
    }
    if (rc != OK && msg && msg_len) snprintf(msg, msg_len, "%s", d.msg);
    return rc != OK ? rc : count;
}

}  // namespace bsclip_jpeg
