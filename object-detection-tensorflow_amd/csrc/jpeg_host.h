// Host half of the JPEG decoder (include/odtk.h, "JPEG"): marker parsing and baseline Huffman decoding.  Plain C++17 with no HIP in it, so that
// csrc/jpeg.hip includes it for libodtk and tests/jpeg_fuzz_host.cpp compiles it with g++ under the address / undefined-behaviour sanitizers.
// The bytes come from files the user did not write: every length field is checked against the buffer before it is used, every Huffman table against
// the code space, every coefficient index against the block.  No state outside the arguments: callable from several threads at once.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/odtk.h"

namespace odtk_jpeg {

static const unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                          41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                          30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
    bool defined = false;
    unsigned char vals[256];
    int maxcode[17];      // largest code of each length, -1 where the length has none
    int valoff[17];       // vals index of a length's first code minus that code
    int total = 0;
    uint16_t look[512];   // 9-bit prefix -> (length << 8) | symbol, 0 where the code is longer
};

struct Header {
    struct odtk_jpeg_info info;
    uint16_t qt[4][64];   // natural order
    bool qt_defined[4] = {false, false, false, false};
    Huff dc[4], ac[4];
    int td[3], ta[3];
    int restart_interval = 0;
    size_t scan_pos = 0;  // first byte of the entropy-coded segment
};

#define ODTK_JPEG_FAIL(...)                       \
    do {                                          \
        snprintf(err, errn, __VA_ARGS__);         \
        return ODTK_ERR_ARG;                      \
    } while (0)

inline int build_huff(Huff& h, const unsigned char* counts, const unsigned char* syms, int total, char* err, size_t errn) {
    int code = 0, k = 0;
    memset(h.look, 0, sizeof(h.look));
    for (int l = 1; l <= 16; ++l) {
        const int n = counts[l - 1];
        if (code + n > (1 << l)) ODTK_JPEG_FAIL("jpeg: corrupt DHT (more codes of length %d than the code space holds)", l);
        h.valoff[l] = k - code;
        if (n && l <= 9)
            for (int i = 0; i < n; ++i) {
                const int first = (code + i) << (9 - l);
                for (int j = 0; j < (1 << (9 - l)); ++j) h.look[first + j] = (uint16_t)((l << 8) | syms[k + i]);
            }
        code += n;
        k += n;
        h.maxcode[l] = n ? code - 1 : -1;
        code <<= 1;
    }
    memcpy(h.vals, syms, (size_t)total);
    h.total = total;
    h.defined = true;
    return ODTK_OK;
}

// Markers up to and including SOS: geometry, tables, restart interval, the scan's table selectors.
inline int parse_header(const unsigned char* d, size_t n, Header& H, char* err, size_t errn) {
    if (d == nullptr) ODTK_JPEG_FAIL("jpeg: null data");
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) ODTK_JPEG_FAIL("jpeg: not a JPEG stream (no SOI marker)");
    memset(&H.info, 0, sizeof(H.info));
    bool have_sof = false, saw_jfif = false;
    int adobe_transform = -1;          // APP14 "Adobe": 0 = the components are RGB (or CMYK), 1 = YCbCr, 2 = YCCK
    int comp_id[3] = {0, 0, 0};
    size_t pos = 2;
    for (;;) {
        if (pos + 2 > n) ODTK_JPEG_FAIL("jpeg: truncated stream (no SOS marker before the end, offset %zu)", pos);
        if (d[pos] != 0xFF) ODTK_JPEG_FAIL("jpeg: corrupt stream (0x%02x where a marker should start, offset %zu)", d[pos], pos);
        while (pos < n && d[pos] == 0xFF) ++pos;      // fill bytes
        if (pos >= n) ODTK_JPEG_FAIL("jpeg: truncated stream (ends inside a marker)");
        const int m = d[pos++];
        if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD8)) ODTK_JPEG_FAIL("jpeg: corrupt stream (marker 0xff%02x before SOS, offset %zu)", m, pos - 2);
        if (m == 0xD9) ODTK_JPEG_FAIL("jpeg: corrupt stream (EOI before SOS)");
        if (pos + 2 > n) ODTK_JPEG_FAIL("jpeg: truncated stream (segment length cut off, offset %zu)", pos);
        const size_t L = ((size_t)d[pos] << 8) | d[pos + 1];
        if (L < 2 || L > n - pos) ODTK_JPEG_FAIL("jpeg: truncated or corrupt stream (segment 0xff%02x of length %zu at offset %zu, %zu bytes left)", m, L, pos, n - pos);
        const unsigned char* s = d + pos + 2;
        const size_t sl = L - 2;
        pos += L;
        if (m == 0xC2) ODTK_JPEG_FAIL("jpeg: progressive JPEG (SOF2) is not supported: baseline sequential only");
        if (m == 0xC9 || m == 0xCA || m == 0xCB || m == 0xCD || m == 0xCE || m == 0xCF || m == 0xCC)
            ODTK_JPEG_FAIL("jpeg: arithmetic coding (marker 0xff%02x) is not supported: baseline Huffman only", m);
        if (m == 0xC3 || m == 0xC5 || m == 0xC6 || m == 0xC7) ODTK_JPEG_FAIL("jpeg: lossless / hierarchical JPEG (SOF%d) is not supported", m - 0xC0);
        if (m == 0xC0 || m == 0xC1) {
            if (have_sof) ODTK_JPEG_FAIL("jpeg: corrupt stream (second frame header)");
            if (sl < 6) ODTK_JPEG_FAIL("jpeg: corrupt frame header (length %zu)", L);
            if (s[0] == 12) ODTK_JPEG_FAIL("jpeg: 12-bit samples are not supported: 8-bit only");
            if (s[0] != 8) ODTK_JPEG_FAIL("jpeg: sample precision %d is not supported: 8-bit only", s[0]);
            const int h = (s[1] << 8) | s[2], w = (s[3] << 8) | s[4], nc = s[5];
            if (nc == 4) ODTK_JPEG_FAIL("jpeg: 4 components (CMYK / YCCK) are not supported: grayscale or YCbCr only");
            if (nc != 1 && nc != 3) ODTK_JPEG_FAIL("jpeg: %d components are not supported: 1 or 3 only", nc);
            if (w == 0 || h == 0) ODTK_JPEG_FAIL("jpeg: picture size %d x %d is not supported (a height of 0, DNL, included)", w, h);
            if (sl != (size_t)(6 + 3 * nc)) ODTK_JPEG_FAIL("jpeg: corrupt frame header (length %zu for %d components)", L, nc);
            struct odtk_jpeg_info& I = H.info;
            I.width = w; I.height = h; I.ncomp = nc;
            for (int c = 0; c < nc; ++c) {
                comp_id[c] = s[6 + 3 * c];
                I.hsamp[c] = s[7 + 3 * c] >> 4;
                I.vsamp[c] = s[7 + 3 * c] & 15;
                I.tq[c] = s[8 + 3 * c];
                if (I.tq[c] > 3) ODTK_JPEG_FAIL("jpeg: corrupt frame header (quantisation table %d)", I.tq[c]);
                if (I.hsamp[c] < 1 || I.hsamp[c] > 4 || I.vsamp[c] < 1 || I.vsamp[c] > 4) ODTK_JPEG_FAIL("jpeg: corrupt frame header (sampling factors %d x %d)", I.hsamp[c], I.vsamp[c]);
            }
            if (nc == 1) {
                I.hsamp[0] = I.vsamp[0] = 1;          // one component: the scan is not interleaved, its MCU is one block whatever the factors say
            } else {
                const int hs = I.hsamp[0], vs = I.vsamp[0];
                const bool luma_ok = (hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2);
                if (!luma_ok || I.hsamp[1] != 1 || I.vsamp[1] != 1 || I.hsamp[2] != 1 || I.vsamp[2] != 1)
                    ODTK_JPEG_FAIL("jpeg: sampling %dx%d,%dx%d,%dx%d is not supported: 1x1, 2x1 or 2x2 luma over 1x1 chroma only", hs, vs, I.hsamp[1], I.vsamp[1],
                                   I.hsamp[2], I.vsamp[2]);
            }
            I.mcu_w = (w + 8 * I.hsamp[0] - 1) / (8 * I.hsamp[0]);
            I.mcu_h = (h + 8 * I.vsamp[0] - 1) / (8 * I.vsamp[0]);
            I.coef_count = 0;
            for (int c = 0; c < nc; ++c) {
                I.blocks_w[c] = I.mcu_w * I.hsamp[c];
                I.blocks_h[c] = I.mcu_h * I.vsamp[c];
                I.blocks[c] = I.blocks_w[c] * I.blocks_h[c];          // <= 8192 * 8192: fits an int
                I.coef_offset[c] = I.coef_count;
                I.coef_count += 64ll * I.blocks[c];
            }
            have_sof = true;
        } else if (m == 0xDB) {
            size_t p = 0;
            while (p < sl) {
                const int pq = s[p] >> 4, tq = s[p] & 15;
                if (pq > 1 || tq > 3) ODTK_JPEG_FAIL("jpeg: corrupt DQT (precision %d, table %d)", pq, tq);
                const size_t need = pq ? 128 : 64;
                if (sl - p - 1 < need) ODTK_JPEG_FAIL("jpeg: corrupt DQT (table cut off)");
                for (int i = 0; i < 64; ++i)
                    H.qt[tq][kZigzag[i]] = pq ? (uint16_t)((s[p + 1 + 2 * i] << 8) | s[p + 2 + 2 * i]) : (uint16_t)s[p + 1 + i];
                H.qt_defined[tq] = true;
                p += 1 + need;
            }
        } else if (m == 0xC4) {
            size_t p = 0;
            while (p < sl) {
                const int tc = s[p] >> 4, th = s[p] & 15;
                if (tc > 1 || th > 3) ODTK_JPEG_FAIL("jpeg: corrupt DHT (class %d, table %d)", tc, th);
                if (sl - p - 1 < 16) ODTK_JPEG_FAIL("jpeg: corrupt DHT (counts cut off)");
                int total = 0;
                for (int i = 0; i < 16; ++i) total += s[p + 1 + i];
                if (total > 256 || sl - p - 17 < (size_t)total) ODTK_JPEG_FAIL("jpeg: corrupt DHT (%d symbols)", total);
                const int rc = build_huff(tc ? H.ac[th] : H.dc[th], s + p + 1, s + p + 17, total, err, errn);
                if (rc) return rc;
                p += 17 + (size_t)total;
            }
        } else if (m == 0xE0) {
            if (sl >= 5 && memcmp(s, "JFIF", 5) == 0) saw_jfif = true;
        } else if (m == 0xEE) {
            if (sl >= 12 && memcmp(s, "Adobe", 5) == 0) adobe_transform = s[11];
        } else if (m == 0xDD) {
            if (sl != 2) ODTK_JPEG_FAIL("jpeg: corrupt DRI (length %zu)", L);
            H.restart_interval = (s[0] << 8) | s[1];
        } else if (m == 0xDA) {
            if (!have_sof) ODTK_JPEG_FAIL("jpeg: corrupt stream (SOS before the frame header)");
            const int nc = H.info.ncomp;
            if (sl < 1) ODTK_JPEG_FAIL("jpeg: corrupt SOS");
            const int ns = s[0];
            if (ns != nc) ODTK_JPEG_FAIL("jpeg: a scan with %d of %d components is not supported: one interleaved scan only", ns, nc);
            if (sl != (size_t)(4 + 2 * ns)) ODTK_JPEG_FAIL("jpeg: corrupt SOS (length %zu for %d components)", L, ns);
            for (int c = 0; c < nc; ++c) {
                if (s[1 + 2 * c] != comp_id[c]) ODTK_JPEG_FAIL("jpeg: scan component %d does not follow the frame's order: not supported", s[1 + 2 * c]);
                H.td[c] = s[2 + 2 * c] >> 4;
                H.ta[c] = s[2 + 2 * c] & 15;
                if (H.td[c] > 3 || H.ta[c] > 3) ODTK_JPEG_FAIL("jpeg: corrupt SOS (Huffman table %d / %d)", H.td[c], H.ta[c]);
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) ODTK_JPEG_FAIL("jpeg: spectral selection / successive approximation is not supported: baseline only");
            // the colour space of three components, by libjpeg's rules: JFIF says YCbCr; else Adobe's transform flag; else the component ids
            if (nc == 3 && !saw_jfif &&
                (adobe_transform == 0 || (adobe_transform < 0 && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B')))
                ODTK_JPEG_FAIL("jpeg: RGB-coded JPEG (%s) is not supported: YCbCr or grayscale only", adobe_transform == 0 ? "Adobe transform 0" : "component ids R, G, B");
            H.info.restart_interval = H.restart_interval;
            H.scan_pos = pos;
            return ODTK_OK;
        }
        // APPn, COM and everything else: skipped by its length
    }
}

struct Bits {
    const unsigned char* d;
    size_t n, pos;
    uint64_t buf = 0;     // the next bits, left-aligned from bit (count - 1) down
    int count = 0;        // bits in buf (zero padding included)
    long long real = 0;   // of these, bits that came from the stream; negative: the decoder has read past a marker or the end
    inline void fill() {
        while (count <= 56) {
            unsigned b = 0;
            if (pos < n) {
                const unsigned c = d[pos];
                if (c != 0xFF) { b = c; ++pos; real += 8; }
                else if (pos + 1 < n && d[pos + 1] == 0x00) { b = 0xFF; pos += 2; real += 8; }
                // else a marker (or a cut-off 0xff): stay on it and feed zeros
            }
            buf = (buf << 8) | b;
            count += 8;
        }
    }
    inline unsigned peek(int k) const { return (unsigned)((buf >> (count - k)) & ((1u << k) - 1u)); }      // 1 <= k <= 16 <= count
    inline void skip(int k) { count -= k; real -= k; }
};

inline int decode_symbol(Bits& b, const Huff& h) {
    const unsigned e = h.look[b.peek(9)];
    if (e) { b.skip((int)(e >> 8)); return (int)(e & 255u); }
    for (int l = 10; l <= 16; ++l) {
        const int code = (int)b.peek(l);
        if (code <= h.maxcode[l]) {
            const int i = h.valoff[l] + code;
            if (i < 0 || i >= h.total) return -1;
            b.skip(l);
            return h.vals[i];
        }
    }
    return -1;
}

inline int receive_extend(Bits& b, int s) {      // 1 <= s <= 15
    const int v = (int)b.peek(s);
    b.skip(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

inline int info(const unsigned char* d, size_t n, struct odtk_jpeg_info* out, char* err, size_t errn) {
    if (out == nullptr) ODTK_JPEG_FAIL("jpeg: null info");
    Header H;
    const int rc = parse_header(d, n, H, err, errn);
    if (rc) return rc;
    *out = H.info;
    return ODTK_OK;
}

inline int entropy_decode(const unsigned char* d, size_t n, int16_t* coef, size_t coef_capacity, uint16_t* qtables, char* err, size_t errn) {
    if (coef == nullptr || qtables == nullptr) ODTK_JPEG_FAIL("jpeg: null output");
    Header H;
    const int rc = parse_header(d, n, H, err, errn);
    if (rc) return rc;
    const struct odtk_jpeg_info& I = H.info;
    if ((unsigned long long)I.coef_count > (unsigned long long)coef_capacity)
        ODTK_JPEG_FAIL("jpeg: coefficient buffer too small (%zu, the picture needs %lld)", coef_capacity, I.coef_count);
    for (int c = 0; c < I.ncomp; ++c) {
        if (!H.qt_defined[I.tq[c]]) ODTK_JPEG_FAIL("jpeg: missing quantisation table %d", I.tq[c]);
        if (!H.dc[H.td[c]].defined) ODTK_JPEG_FAIL("jpeg: missing DC Huffman table %d", H.td[c]);
        if (!H.ac[H.ta[c]].defined) ODTK_JPEG_FAIL("jpeg: missing AC Huffman table %d", H.ta[c]);
    }
    for (int t = 0; t < 4; ++t)
        for (int i = 0; i < 64; ++i) qtables[t * 64 + i] = H.qt_defined[t] ? H.qt[t][i] : (uint16_t)1;
    memset(coef, 0, (size_t)I.coef_count * sizeof(int16_t));
    Bits b{d, n, H.scan_pos};
    int pred[3] = {0, 0, 0};
    long long mcu = 0;
    for (int my = 0; my < I.mcu_h; ++my)
        for (int mx = 0; mx < I.mcu_w; ++mx, ++mcu) {
            if (H.restart_interval && mcu && mcu % H.restart_interval == 0) {
                // the bits left in the buffer are the padding of the interval's last byte; the reader stopped on the marker
                if (b.pos + 1 >= n || d[b.pos] != 0xFF || d[b.pos + 1] < 0xD0 || d[b.pos + 1] > 0xD7)
                    ODTK_JPEG_FAIL("jpeg: corrupt stream (no restart marker at offset %zu, MCU %lld)", b.pos, mcu);
                b.pos += 2;
                b.buf = 0; b.count = 0; b.real = 0;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < I.ncomp; ++c) {
                const Huff& hd = H.dc[H.td[c]];
                const Huff& ha = H.ac[H.ta[c]];
                for (int v = 0; v < I.vsamp[c]; ++v)
                    for (int h = 0; h < I.hsamp[c]; ++h) {
                        const long long blk = (long long)(my * I.vsamp[c] + v) * I.blocks_w[c] + (mx * I.hsamp[c] + h);
                        int16_t* out = coef + I.coef_offset[c] + 64 * blk;
                        b.fill();
                        int s = decode_symbol(b, hd);
                        if (s < 0 || s > 11) ODTK_JPEG_FAIL("jpeg: corrupt stream (bad DC code, MCU %lld)", mcu);
                        if (s) pred[c] = (int)(int16_t)(uint16_t)(pred[c] + receive_extend(b, s));      // (a hostile stream wraps, it does not overflow)
                        out[0] = (int16_t)pred[c];
                        for (int k = 1; k < 64;) {
                            b.fill();
                            const int rs = decode_symbol(b, ha);
                            if (rs < 0) ODTK_JPEG_FAIL("jpeg: corrupt stream (bad AC code, MCU %lld)", mcu);
                            const int r = rs >> 4;
                            s = rs & 15;
                            if (s == 0) {
                                if (r != 15) break;
                                k += 16;
                                continue;
                            }
                            k += r;
                            if (k > 63) ODTK_JPEG_FAIL("jpeg: corrupt stream (coefficient index %d past the block, MCU %lld)", k, mcu);
                            out[kZigzag[k]] = (int16_t)receive_extend(b, s);
                            ++k;
                        }
                        if (b.real < 0) ODTK_JPEG_FAIL("jpeg: truncated or corrupt stream (entropy data ends in MCU %lld of %lld)", mcu, (long long)I.mcu_w * I.mcu_h);
                    }
            }
        }
    return ODTK_OK;
}

}  // namespace odtk_jpeg
