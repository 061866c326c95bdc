// One SEGMENT of a baseline JPEG scan, decoded from a sync-index entry alone.  The same routine runs on the host (the index
// builder in jpeg_entropy.h, tools/jpeg_segments_check.cpp) and inside the kernel of jpeg_entropy.hip, one lane per segment: plain
// C++, no allocation, no globals, no library call.
//
// A segment is a run of whole MCUs inside one restart interval.  Its index entry (int32[4], include/bsclip.h) says where its first
// bit is and what the DC predictors are there; which MCUs it covers follows from the frame, the restart interval and sync_mcus alone
// (segment_range), never from the data, so every address written is known before a byte is read:
//   reads   p[0, n) only -- the image's own byte range; past its end, or at a marker, the reader feeds zeros and counts them;
//   writes  whole blocks of the segment's MCUs: each is zero-filled and then takes its non-zero coefficients, in the host decoder's
//           layout (jpeg_entropy.h).  After a fault the rest of the segment is still zero-filled, so the range is always defined;
//   loops   MCUs of the segment x blocks of an MCU x at most 64 AC symbols x at most 7 code lengths past the 9-bit look-up; a
//           symbol and its value bits take at most 31 of the >= 57 bits a refill leaves, whatever the tables hold.
// The status is 0 only if no code was unassigned, no run left its block, no made-up bit was consumed, and the segment ended where
// the next entry begins with the predictors it records (or, at the end of a restart interval or of the scan, inside the padding
// of the last data byte).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BSCLIP_HD __host__ __device__ __forceinline__
#else
#define BSCLIP_HD inline
#endif

namespace bsclip_jpeg {

enum : int {
    SEG_BAD_CODE = 1,    // a code no table assigns (or a DC size above 15)
    SEG_BAD_RUN = 2,     // a zero run that leaves the block
    SEG_OVERRUN = 4,     // bits consumed past the byte range or past a marker
    SEG_END_POS = 8,     // the segment did not end where the next one starts / in the padding of the interval's last byte
    SEG_END_PRED = 16,   // DC predictors at the end differ from the next entry's
    SEG_BAD_ENTRY = 32,  // the entry's first MCU or bit position is not this segment's / not inside the byte range
};

constexpr int SYNC_ENTRY = 4;           // int32 per index entry: bit position, first MCU, Y predictor, Cb | Cr << 16
constexpr int64_t MAX_STREAM = 1 << 28;  // bytes: 8 * byte + bit fits an int32

// A Huffman table in the form the segment decoder reads (host memory, device memory and LDS alike): 1420 bytes, dword aligned.
struct SegHuff {
    uint16_t look[512];    // 9-bit prefix -> (length << 8) | symbol, 0 = longer than 9 bits or unassigned
    int32_t maxcode[17];   // [len] largest code of that length, -1 if none (index 0 unused)
    int32_t valoff[17];    // [len] index of the first symbol of that length minus its first code
    int32_t nvals;
    uint8_t vals[256];
};
static_assert(sizeof(SegHuff) == 1420, "SegHuff is part of the C ABI (BSCLIP_JPEG_HUFF_BYTES)");
constexpr int SEG_TABLES = 4;   // per image: DC 0, DC 1, AC 0, AC 1 (the slots the record's selector word names)

struct SegGeom {
    int ncomp, hs, vs, mcus_x, nmcu;
    int sel;   // bit c: DC slot of component c; bit 4 + c: AC slot of component c
};

struct SegEnd {
    int32_t bitpos;   // position of the next unread bit (8 * byte + bit)
    int32_t pred[3];
    uint32_t fetch;   // the reader's next byte: where a restart marker is looked for
    int32_t real;     // real (not made-up) bits left in the window
};

BSCLIP_HD int32_t pack_chroma(int cb, int cr) { return (int32_t)(((uint32_t)cb & 0xFFFFu) | ((uint32_t)cr << 16)); }

// ---- which MCUs a segment covers: from the frame and sync_mcus alone -------------------------------------------------------
BSCLIP_HD int interval_len(int nmcu, int restart) { return (restart <= 0 || restart > nmcu) ? nmcu : restart; }
BSCLIP_HD int segment_count(int nmcu, int restart, int sync_mcus) {
    const int R = interval_len(nmcu, restart);
    return (nmcu / R) * ((R + sync_mcus - 1) / sync_mcus) + (nmcu % R + sync_mcus - 1) / sync_mcus;
}
// segment j -> [first, first + count); *chained: another segment of the same restart interval follows it
BSCLIP_HD void segment_range(int j, int nmcu, int restart, int sync_mcus, int* first, int* count, bool* chained) {
    const int R = interval_len(nmcu, restart);
    const int spi = (R + sync_mcus - 1) / sync_mcus;
    const int i = j / spi, k = j - i * spi;
    const int64_t lo = (int64_t)i * R + (int64_t)k * sync_mcus;
    int64_t stop = (int64_t)(i + 1) * R;
    stop = stop < nmcu ? stop : nmcu;
    int64_t hi = lo + sync_mcus;
    hi = hi < stop ? hi : stop;
    *first = (int)lo;
    *count = (int)(hi - lo);
    *chained = hi < stop;
}

// ---- bit reader ---------------------------------------------------------------------------------------------------------
// A 64-bit window refilled a byte at a time, like the host decoder's: 0xFF00 is one 0xFF data byte; at a marker or at the end of the
// range it feeds zeros and counts them (`fake`).  `stuffed` keeps one flag per byte of the window (newest in bit 0): the byte
// was followed by a stuffed 0x00.  That is what turns "bits left in the window" back into a position in the stream.
struct SegBits {
    const uint8_t* p;
    uint32_t pos, n;
    uint64_t acc;
    int cnt, fake;
    uint32_t stuffed;

    BSCLIP_HD void fill() {
        while (cnt <= 56) {
            unsigned b = 0, st = 0;
            bool real = false;
            if (fake == 0 && pos < n) {
                b = p[pos];
                if (b != 0xFF) {
                    ++pos;
                    real = true;
                } else if (pos + 1 < n && p[pos + 1] == 0x00) {
                    pos += 2;
                    real = true;
                    st = 1;
                }
            }
            if (!real) {
                b = 0;
                fake += 8;
            }
            acc = (acc << 8) | b;
            stuffed = (stuffed << 1) | st;
            cnt += 8;
        }
    }
    BSCLIP_HD unsigned peek(int k) const { return (unsigned)((acc >> (cnt - k)) & ((1u << k) - 1)); }
    BSCLIP_HD void skip(int k) { cnt -= k; }
    BSCLIP_HD bool overran() const { return cnt < fake; }
    // position of the next unread bit; only meaningful while !overran()
    BSCLIP_HD void where(int32_t* bitpos, int32_t* real_left) const {
        const int real = cnt - fake;                 // real bits left: whole bytes and perhaps the tail of one
        const int nb = (real + 7) >> 3;              // bytes they live in, the newest `fake / 8` window bytes being made up
        const uint32_t flags = (stuffed >> (fake >> 3)) & ((1u << nb) - 1u);
        const uint32_t byte = pos - (uint32_t)nb - (uint32_t)__builtin_popcount(flags);
        *bitpos = (int32_t)(byte * 8u + (uint32_t)((8 - (real & 7)) & 7));
        *real_left = real;
    }
};

BSCLIP_HD int seg_symbol(SegBits& b, const SegHuff& h) {   // >= 0: symbol, -1: no such code
    const unsigned e = h.look[b.peek(9)];
    const int len9 = (int)((e >> 8) & 15);
    if (len9) {
        b.skip(len9);
        return (int)(e & 0xff);
    }
    const unsigned nv = (unsigned)h.nvals < 256u ? (unsigned)h.nvals : 256u;   // a table from anywhere: never past vals[]
    for (int len = 10; len <= 16; ++len) {
        const int code = (int)b.peek(len);
        const int mc = h.maxcode[len];
        if (mc >= 0 && code <= mc) {
            const unsigned idx = (unsigned)code + (unsigned)h.valoff[len];
            if (idx >= nv) return -1;
            b.skip(len);
            return h.vals[idx];
        }
    }
    return -1;
}

BSCLIP_HD int seg_extend(unsigned v, int s) { return v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

// one block; blk: 64 int16 (STORE) or unused.  Returns status bits (0 = fine).
template <bool STORE>
BSCLIP_HD int seg_block(SegBits& b, const SegHuff& hd, const SegHuff& ha, int& pred, int16_t* blk) {
    constexpr uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    b.fill();
    int s = seg_symbol(b, hd);
    if (s < 0 || s > 15) return SEG_BAD_CODE;
    int diff = 0;
    if (s) {
        diff = seg_extend(b.peek(s), s);
        b.skip(s);
    }
    pred = (int16_t)(pred + diff);   // the host decoder's wrap
    if (STORE) blk[0] = (int16_t)pred;
    for (int k = 1; k < 64;) {       // every pass ends the block or advances k: at most 63 passes
        b.fill();
        const int rs = seg_symbol(b, ha);
        if (rs < 0) return SEG_BAD_CODE;
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r != 15) break;
            k += 16;
            continue;
        }
        k += r;
        if (k > 63) return SEG_BAD_RUN;
        const int v = seg_extend(b.peek(s), s);
        b.skip(s);
        if (STORE) blk[zz[k]] = (int16_t)v;
        ++k;
    }
    return b.overran() ? SEG_OVERRUN : 0;
}

// Decode MCUs [first, first + count) of the image whose coefficients start at `coef` (STORE = false: walk only, nothing is
// written and `coef` may be null).  The caller guarantees 0 <= first, count >= 1, first + count <= g.nmcu -- segment_range does.
template <bool STORE>
BSCLIP_HD int decode_segment(const uint8_t* p, uint32_t n, const int32_t* entry, int first, int count, const SegGeom& g,
                             const SegHuff* tabs, int16_t* coef, SegEnd* end) {
    int st = 0;
    const uint32_t bit0 = (uint32_t)entry[0];
    if (entry[1] != first || entry[0] < 0 || (bit0 >> 3) >= n) st = SEG_BAD_ENTRY;
    SegBits b{p, st ? n : (bit0 >> 3), n, 0, 0, 0, 0};
    if (!st) {
        b.fill();
        b.skip((int)(bit0 & 7));
    }
    int pred[3] = {entry[2], (int16_t)(entry[3] & 0xFFFF), (int16_t)((uint32_t)entry[3] >> 16)};
    const int n0 = g.nmcu * g.hs * g.vs;   // blocks of the luma plane; a chroma plane has g.nmcu
    int my = first / g.mcus_x, mx = first - my * g.mcus_x;
    for (int m = 0; m < count; ++m) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c >= g.ncomp) break;
            const int hc = c == 0 ? g.hs : 1, nb = c == 0 ? g.hs * g.vs : 1;
            const int64_t plane = c == 0 ? 0 : (int64_t)(n0 + (c - 1) * g.nmcu) * 64;
            const SegHuff& hd = tabs[(g.sel >> c) & 1];
            const SegHuff& ha = tabs[2 + ((g.sel >> (4 + c)) & 1)];
            for (int j = 0; j < nb; ++j) {
                const int v = j / hc, h = j - v * hc;
                int16_t* blk = nullptr;
                if (STORE) {
                    const int vc = c == 0 ? g.vs : 1;
                    blk = coef + plane + ((int64_t)(my * vc + v) * (g.mcus_x * hc) + (mx * hc + h)) * 64;
                    __builtin_memset(__builtin_assume_aligned(blk, 16), 0, 64 * sizeof(int16_t));   // coef is 16-byte aligned
                }
                if (!st) st = seg_block<STORE>(b, hd, ha, pred[c], blk);
            }
        }
        if (++mx == g.mcus_x) mx = 0, ++my;
    }
    end->bitpos = 0, end->real = 0;
    if (!st) b.where(&end->bitpos, &end->real);
    end->pred[0] = pred[0], end->pred[1] = pred[1], end->pred[2] = pred[2];
    end->fetch = b.pos;
    return st;
}

// The end-of-segment check.  chained: `next` is the following entry of the same restart interval; otherwise the segment ends an
// interval or the scan and `next` is not read.
BSCLIP_HD int segment_end_status(const SegEnd& e, const SegGeom& g, const int32_t* next, bool chained) {
    if (!chained) return e.real < 8 ? 0 : SEG_END_POS;   // only padding bits of the last data byte may be left before the marker
    int st = e.bitpos == next[0] ? 0 : SEG_END_POS;
    const int32_t chroma = g.ncomp == 3 ? pack_chroma(e.pred[1], e.pred[2]) : 0;
    if (e.pred[0] != next[2] || chroma != next[3]) st |= SEG_END_PRED;
    return st;
}

template <bool STORE>
BSCLIP_HD int decode_segment_checked(const uint8_t* p, uint32_t n, const int32_t* entry, int first, int count, const SegGeom& g,
                                     const SegHuff* tabs, int16_t* coef, const int32_t* next, bool chained) {
    SegEnd e;
    const int st = decode_segment<STORE>(p, n, entry, first, count, g, tabs, coef, &e);
    return st ? st : segment_end_status(e, g, next, chained);
}

}  // namespace bsclip_jpeg
