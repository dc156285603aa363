// The host half of the JPEG decoder (include/mvldm.h, "JPEG frames"): the marker parser, the Huffman decoder of a baseline scan and the
// plain C++ restatement of the device half.  No HIP call, no global or static state: every table lives in the caller's frame, so any
// number of threads may decode at once.  Every read of the stream goes through an index checked against `len`.
#include <string.h>

#include <vector>

#include "jpeg_common.h"
#include "jpeg_huff_common.h"

namespace mvldm {

int set_error(int code, const char* fmt, ...);      // api.cpp (thread-local text)

namespace {

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {                   // one DHT table: canonical codes by length, and the codes of up to kLook bits by direct lookup
    static constexpr int kLook = 9;
    bool defined = false;
    uint8_t vals[256];
    int32_t maxcode[18];        // largest code of length l, -1 if none; [17] a sentinel above every 16-bit code
    int32_t valoff[17];         // vals index of the first code of length l, minus that code
    uint16_t look[1 << kLook];  // (length << 8) | symbol, 0 for a longer code
};

// DHT payload at p[0 .. n): counts[16], symbols.  false: the counts do not describe a prefix code
bool huff_build(Huff* t, const uint8_t* counts, const uint8_t* syms, int nsyms) {
    memset(t->look, 0, sizeof(t->look));
    memset(t->vals, 0, sizeof(t->vals));        // the table blob of the device path copies all 256
    memcpy(t->vals, syms, (size_t)nsyms);
    int32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = counts[l - 1];
        t->valoff[l] = k - code;
        if (n) {
            if (code + n > (1 << l)) return false;
            for (int i = 0; i < n; ++i, ++k, ++code)
                if (l <= Huff::kLook) {
                    const int first = code << (Huff::kLook - l);
                    for (int j = 0; j < (1 << (Huff::kLook - l)); ++j) t->look[first + j] = (uint16_t)((l << 8) | t->vals[k]);
                }
            t->maxcode[l] = code - 1;
        } else {
            t->maxcode[l] = -1;
        }
        code <<= 1;
    }
    t->maxcode[17] = 0x7FFFFFFF;
    t->defined = true;
    return true;
}

struct Component {
    int id, hs, vs, tq, td, ta;
};

struct Header {                 // what the markers in front of the scan say
    int h = 0, w = 0, sampling = -1, ncomp = 0;
    Component comp[3];
    uint16_t qt[4][64];         // natural order
    bool qt_defined[4] = {false, false, false, false};
    Huff dc[4], ac[4];
    int restart = 0;            // MCUs per restart interval, 0: none
    bool jfif = false, adobe = false;
    size_t scan = 0;            // index of the first byte of entropy-coded data
};

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Walks the markers from SOI to the first SOS.  Returns a MVLDM_JPEG_* reason; hd->h / w are set once a frame header was read.
int parse_header(const uint8_t* d, size_t len, Header* hd) {
    if (len < 2 || d[0] != 0xFF || d[1] != 0xD8) return MVLDM_JPEG_NOT_JPEG;
    size_t pos = 2;
    bool sof = false;
    int reason = MVLDM_JPEG_OK;                 // the first thing that makes the frame unsupported; parsing goes on to the size
    auto refuse = [&](int r) {
        if (reason == MVLDM_JPEG_OK) reason = r;
    };
    while (true) {
        // a marker: 0xFF, any number of fill 0xFF, the code
        if (pos >= len) return MVLDM_JPEG_TRUNCATED;
        if (d[pos] != 0xFF) return MVLDM_JPEG_CORRUPT;
        while (pos < len && d[pos] == 0xFF) ++pos;
        if (pos >= len) return MVLDM_JPEG_TRUNCATED;
        const int m = d[pos++];
        if (m == 0x00 || m == 0xD8 || (m >= 0xD0 && m <= 0xD7)) return MVLDM_JPEG_CORRUPT;
        if (m == 0xD9) return MVLDM_JPEG_TRUNCATED;     // EOI before any scan
        if (m == 0x01) continue;                        // TEM: no payload
        if (len - pos < 2) return MVLDM_JPEG_TRUNCATED;
        const size_t seg = (size_t)be16(d + pos);
        if (seg < 2) return MVLDM_JPEG_CORRUPT;
        if (len - pos < seg) return MVLDM_JPEG_TRUNCATED;
        const uint8_t* p = d + pos + 2;
        const size_t n = seg - 2;
        pos += seg;
        if (m == 0xE0) {
            if (n >= 5 && memcmp(p, "JFIF", 5) == 0) hd->jfif = true;
        } else if (m == 0xEE) {
            if (n >= 12 && memcmp(p, "Adobe", 5) == 0) hd->adobe = true;
        } else if (m == 0xDB) {                 // DQT: any number of tables
            size_t at = 0;
            while (at < n) {
                const int pq = p[at] >> 4, tq = p[at] & 15;
                if (tq > 3 || pq > 1) return MVLDM_JPEG_CORRUPT;
                const size_t need = 1 + (pq ? 128 : 64);
                if (n - at < need) return MVLDM_JPEG_CORRUPT;
                if (pq) {
                    refuse(MVLDM_JPEG_PRECISION);
                } else {
                    for (int k = 0; k < 64; ++k) hd->qt[tq][kZigzag[k]] = p[at + 1 + k];
                    hd->qt_defined[tq] = true;
                }
                at += need;
            }
        } else if (m == 0xC4) {                 // DHT: any number of tables
            size_t at = 0;
            while (at < n) {
                if (n - at < 17) return MVLDM_JPEG_CORRUPT;
                const int tc = p[at] >> 4, th = p[at] & 15;
                if (tc > 1 || th > 3) return MVLDM_JPEG_CORRUPT;
                int total = 0;
                for (int l = 0; l < 16; ++l) total += p[at + 1 + l];
                if (total > 256 || n - at - 17 < (size_t)total) return MVLDM_JPEG_CORRUPT;
                if (!huff_build(tc ? &hd->ac[th] : &hd->dc[th], p + at + 1, p + at + 17, total)) return MVLDM_JPEG_CORRUPT;
                at += 17 + (size_t)total;
            }
        } else if (m == 0xDD) {                 // DRI
            if (n != 2) return MVLDM_JPEG_CORRUPT;
            hd->restart = be16(p);
        } else if (m >= 0xC0 && m <= 0xCF && m != 0xC8 && m != 0xCC) {      // a frame header
            if (sof) return MVLDM_JPEG_CORRUPT;
            sof = true;
            if (n < 6) return MVLDM_JPEG_CORRUPT;
            hd->h = be16(p + 1);
            hd->w = be16(p + 3);
            hd->ncomp = p[5];
            if (n != 6 + 3 * (size_t)hd->ncomp) return MVLDM_JPEG_CORRUPT;
            if (m == 0xC2) refuse(MVLDM_JPEG_PROGRESSIVE);
            else if (m != 0xC0) refuse(MVLDM_JPEG_CODING);
            if (p[0] != 8) refuse(MVLDM_JPEG_PRECISION);
            if (hd->h < 1 || hd->w < 1 || hd->h > kJpegMaxDim || hd->w > kJpegMaxDim) refuse(MVLDM_JPEG_SIZE);
            if (hd->ncomp != 1 && hd->ncomp != 3) {
                refuse(MVLDM_JPEG_COMPONENTS);
            } else {
                for (int c = 0; c < hd->ncomp; ++c) {
                    const uint8_t* q = p + 6 + 3 * c;
                    hd->comp[c] = Component{q[0], q[1] >> 4, q[1] & 15, q[2], 0, 0};
                    if (q[2] > 3) return MVLDM_JPEG_CORRUPT;
                }
                const Component* cc = hd->comp;
                if (hd->ncomp == 1) {
                    if (cc[0].hs == 1 && cc[0].vs == 1) hd->sampling = MVLDM_JPEG_GRAY;
                } else if (cc[1].hs == 1 && cc[1].vs == 1 && cc[2].hs == 1 && cc[2].vs == 1) {
                    if (cc[0].hs == 1 && cc[0].vs == 1) hd->sampling = MVLDM_JPEG_444;
                    if (cc[0].hs == 2 && cc[0].vs == 1) hd->sampling = MVLDM_JPEG_422;
                    if (cc[0].hs == 2 && cc[0].vs == 2) hd->sampling = MVLDM_JPEG_420;
                }
                if (hd->sampling < 0) refuse(MVLDM_JPEG_SAMPLING);
            }
        } else if (m == 0xDA) {                 // SOS
            if (!sof) return MVLDM_JPEG_CORRUPT;
            if (reason != MVLDM_JPEG_OK) return reason;
            if (n < 1) return MVLDM_JPEG_CORRUPT;
            const int ns = p[0];
            if (ns < 1 || ns > 4 || n != 4 + 2 * (size_t)ns) return MVLDM_JPEG_CORRUPT;
            if (ns != hd->ncomp) return MVLDM_JPEG_SCANS;
            for (int c = 0; c < ns; ++c) {      // in the frame's order, as an interleaved scan must list them
                if (p[1 + 2 * c] != hd->comp[c].id) return MVLDM_JPEG_SCANS;
                hd->comp[c].td = p[2 + 2 * c] >> 4;
                hd->comp[c].ta = p[2 + 2 * c] & 15;
                if (hd->comp[c].td > 3 || hd->comp[c].ta > 3) return MVLDM_JPEG_CORRUPT;
                if (!hd->dc[hd->comp[c].td].defined || !hd->ac[hd->comp[c].ta].defined || !hd->qt_defined[hd->comp[c].tq]) return MVLDM_JPEG_CORRUPT;
            }
            if (p[1 + 2 * ns] != 0 || p[2 + 2 * ns] != 63 || p[3 + 2 * ns] != 0) return MVLDM_JPEG_CORRUPT;      // Ss, Se, Ah / Al of a sequential scan
            if (hd->ncomp == 3 && !hd->jfif) {  // jdapimin.c default_decompress_parms
                if (hd->adobe) return MVLDM_JPEG_COLORSPACE;
                if (hd->comp[0].id != 1 || hd->comp[1].id != 2 || hd->comp[2].id != 3) return MVLDM_JPEG_COLORSPACE;
            }
            hd->scan = pos;
            return MVLDM_JPEG_OK;
        }
        // APPn, COM and anything else with a length: skipped
    }
}

struct Bits {                   // the scan's bit stream: byte stuffing removed, stops in front of a marker
    const uint8_t* d;
    size_t pos, len;
    uint64_t acc = 0;           // the low `n` bits are the unread bits, oldest highest
    int n = 0;
    bool stop = false;          // a marker or the end of the data lies at pos
    void fill() {
        while (n <= 56 && !stop) {
            if (pos >= len) {
                stop = true;
                break;
            }
            const uint8_t b = d[pos];
            if (b == 0xFF) {
                if (pos + 1 >= len) {           // the data ends inside a stuffed pair or a marker
                    pos = len;
                    stop = true;
                    break;
                }
                if (d[pos + 1] != 0x00) {       // a marker: stay in front of it
                    stop = true;
                    break;
                }
                pos += 2;
            } else {
                ++pos;
            }
            acc = (acc << 8) | b;
            n += 8;
        }
    }
    // the next k <= 16 bits, zero-padded past the end, not consumed
    int peek(int k) {
        if (n < k) fill();
        return n >= k ? (int)((acc >> (n - k)) & ((1u << k) - 1)) : (int)((acc << (k - n)) & ((1u << k) - 1));
    }
    bool skip(int k) {
        if (k > n) return false;
        n -= k;
        return true;
    }
};

// one Huffman symbol, or -1 (a code that does not exist, or the data ran out)
inline int huff_decode(Bits* b, const Huff& t) {
    const int v = b->peek(16);
    const int e = t.look[v >> (16 - Huff::kLook)];
    if (e) return b->skip(e >> 8) ? (e & 255) : -1;
    for (int l = Huff::kLook + 1; l <= 16; ++l) {
        const int code = v >> (16 - l);
        if (code <= t.maxcode[l]) return b->skip(l) ? t.vals[(code + t.valoff[l]) & 255] : -1;
    }
    return -1;
}
// s >= 1 magnitude bits, sign-extended as in F.2.2.1; false when the data ran out
inline bool receive_extend(Bits* b, int s, int* out) {
    const int v = b->peek(s);
    if (!b->skip(s)) return false;
    *out = v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
    return true;
}

// What follows the entropy-coded bytes, at d[p]: fill bytes (FF), then EOI.  Returns a reason: running off the end is TRUNCATED; no
// marker at all at p, or another marker (more scans, tables or restart markers than the frame has MCUs for), is CORRUPT.
int expect_eoi(const uint8_t* d, size_t len, size_t p) {
    const size_t at = p;
    while (p < len && d[p] == 0xFF) ++p;
    if (p >= len) return MVLDM_JPEG_TRUNCATED;
    return p == at || d[p] != 0xD9 ? MVLDM_JPEG_CORRUPT : MVLDM_JPEG_OK;
}

// The three components' quantisation rows (natural order, zeros for a component the frame does not have) as the device half takes them
void quant_rows(const Header& hd, const JpegLayout& L, uint16_t* qt) {
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 64; ++k) qt[c * 64 + k] = c < L.ncomp ? hd.qt[hd.comp[c].tq][k] : 0;
}

// The scan.  coef: room for L.blocks * 64 values (checked by the caller).  Returns a reason.  kStore false: the reason alone, coef is
// not touched (mvldm_jpeg_rst_prepare names a broken marker structure with this decoder's own code).
template <bool kStore>
int decode_scan(const uint8_t* d, size_t len, const Header& hd, const JpegLayout& L, int16_t* coef, int32_t* max_s) {
    Bits b{d, hd.scan, len};
    int pred[3] = {0, 0, 0};
    int32_t worst = 0;
    const int mcus = L.mcux * L.mcuy;
    int next_rst = 0, until_rst = hd.restart;
    if (kStore) memset(coef, 0, (size_t)L.blocks * 64 * sizeof(int16_t));
    for (int m = 0; m < mcus; ++m) {
        if (hd.restart && until_rst == 0) {     // byte-align, RSTn, predictors back to 0
            b.fill();
            if (!b.stop || b.n >= 8) return MVLDM_JPEG_CORRUPT;
            size_t p = b.pos;
            if (p >= len) return MVLDM_JPEG_TRUNCATED;
            while (p < len && d[p] == 0xFF) ++p;
            if (p >= len) return MVLDM_JPEG_TRUNCATED;
            if (d[p] != 0xD0 + next_rst) return d[p] == 0xD9 ? MVLDM_JPEG_TRUNCATED : MVLDM_JPEG_CORRUPT;
            b.pos = p + 1;
            b.acc = 0;
            b.n = 0;
            b.stop = false;
            next_rst = (next_rst + 1) & 7;
            until_rst = hd.restart;
            pred[0] = pred[1] = pred[2] = 0;
        }
        --until_rst;
        const int my = m / L.mcux, mx = m % L.mcux;
        for (int c = 0; c < L.ncomp; ++c) {
            const int hs = c == 0 ? L.hmax : 1, vs = c == 0 ? L.vmax : 1;
            const Huff& dc = hd.dc[hd.comp[c].td];
            const Huff& ac = hd.ac[hd.comp[c].ta];
            const uint16_t* q = hd.qt[hd.comp[c].tq];
            for (int by = 0; by < vs; ++by)
                for (int bx = 0; bx < hs; ++bx) {
                    int16_t* blk = kStore ? coef + ((size_t)L.off[c] + (size_t)(my * vs + by) * L.bw[c] + (mx * hs + bx)) * 64 : nullptr;
                    int s = huff_decode(&b, dc);
                    if (s < 0) return b.stop && b.pos >= len ? MVLDM_JPEG_TRUNCATED : MVLDM_JPEG_CORRUPT;
                    if (s > 15) return MVLDM_JPEG_CORRUPT;
                    int diff = 0;
                    if (s && !receive_extend(&b, s, &diff)) return b.pos >= len ? MVLDM_JPEG_TRUNCATED : MVLDM_JPEG_CORRUPT;
                    pred[c] += diff;
                    if (pred[c] < -32768 || pred[c] > 32767) return MVLDM_JPEG_CORRUPT;
                    if (kStore) blk[0] = (int16_t)pred[c];
                    int32_t sum = (pred[c] < 0 ? -pred[c] : pred[c]) * (int32_t)q[0];
                    for (int k = 1; k < 64; ++k) {
                        const int rs = huff_decode(&b, ac);
                        if (rs < 0) return b.stop && b.pos >= len ? MVLDM_JPEG_TRUNCATED : MVLDM_JPEG_CORRUPT;
                        const int r = rs >> 4;
                        s = rs & 15;
                        if (s == 0) {
                            if (r != 15) break;             // EOB
                            k += 15;                        // ZRL
                            continue;
                        }
                        k += r;
                        if (k > 63) return MVLDM_JPEG_CORRUPT;
                        int v = 0;
                        if (!receive_extend(&b, s, &v)) return b.pos >= len ? MVLDM_JPEG_TRUNCATED : MVLDM_JPEG_CORRUPT;
                        const int nat = kZigzag[k];
                        if (kStore) blk[nat] = (int16_t)v;  // |v| < 2^15
                        sum += (v < 0 ? -v : v) * (int32_t)q[nat];     // <= 64 * 32767 * 255 < 2^31
                    }
                    if (sum > worst) worst = sum;
                }
        }
    }
    // what follows the last MCU: padding bits, then EOI
    b.fill();
    if (!b.stop || b.n >= 8) return MVLDM_JPEG_CORRUPT;
    const int tail = expect_eoi(d, len, b.pos);
    if (tail != MVLDM_JPEG_OK) return tail;
    if (max_s) *max_s = worst;
    return worst > kJpegGuard ? MVLDM_JPEG_RANGE : MVLDM_JPEG_OK;
}

// info[0..7] of mvldm_jpeg_probe
void fill_info(const Header& hd, int reason, int32_t* info) {
    for (int i = 0; i < 8; ++i) info[i] = 0;
    info[0] = hd.h;
    info[1] = hd.w;
    info[2] = -1;
    info[3] = reason;
    JpegLayout L;
    if (reason == MVLDM_JPEG_OK && jpeg_layout(hd.h, hd.w, hd.sampling, &L)) {
        info[2] = hd.sampling;
        info[4] = L.bw[0] * L.bh[0];
        info[5] = L.bw[1] * L.bh[1];
        info[6] = L.mcux;
        info[7] = L.mcuy;
    }
}

// one table of the device path's blob (include/mvldm.h): look | maxcode[18] | valoff[18] | vals
void huff_blob(const Huff& t, uint8_t* out) {
    int32_t words[36];
    for (int l = 0; l < 18; ++l) {
        words[l] = l >= 1 ? t.maxcode[l] : -1;
        words[18 + l] = l >= 1 && l <= 16 ? t.valoff[l] : 0;
    }
    memcpy(out + kHuffLookOff, t.look, sizeof(t.look));
    memcpy(out + kHuffMaxOff, words, sizeof(words));
    memcpy(out + kHuffValsOff, t.vals, sizeof(t.vals));
}
static_assert(sizeof(Huff::look) == 1024 && sizeof(Huff::vals) == 256, "table blob layout");

// the frame's MVLDM_JPEG_TABLE_BYTES: the six tables as the scan header selects them, then the quantisation rows
void tables_blob(const Header& hd, const JpegLayout& L, uint8_t* tables) {
    memset(tables, 0, (size_t)kHuffBlobBytes);
    for (int c = 0; c < L.ncomp; ++c) {
        huff_blob(hd.dc[hd.comp[c].td], tables + (size_t)(2 * c) * kHuffTabBytes);
        huff_blob(hd.ac[hd.comp[c].ta], tables + (size_t)(2 * c + 1) * kHuffTabBytes);
    }
    uint16_t qt[192];
    quant_rows(hd, L, qt);
    memcpy(tables + kHuffTabsBytes, qt, sizeof(qt));
}

}  // namespace

size_t jpeg_coef_count(int h, int w, int sampling) {
    JpegLayout L;
    return jpeg_layout(h, w, sampling, &L) ? (size_t)L.blocks * 64 : 0;
}

}  // namespace mvldm

using namespace mvldm;

extern "C" int mvldm_jpeg_probe(const uint8_t* data, size_t len, int32_t* info) {
    if (data == nullptr || info == nullptr) return set_error(MVLDM_ERR_ARG, "jpeg_probe: null pointer");
    Header hd;
    const int reason = parse_header(data, len, &hd);
    fill_info(hd, reason, info);
    return reason;
}

extern "C" size_t mvldm_jpeg_coef_count(int h, int w, int sampling) { return jpeg_coef_count(h, w, sampling); }

extern "C" int mvldm_jpeg_entropy(const uint8_t* data, size_t len, int16_t* coef, size_t coef_len, uint16_t* qt, int32_t* max_s) {
    if (data == nullptr || coef == nullptr || qt == nullptr) return set_error(MVLDM_ERR_ARG, "jpeg_entropy: null pointer");
    if (max_s) *max_s = 0;
    Header hd;
    const int reason = parse_header(data, len, &hd);
    if (reason != MVLDM_JPEG_OK) return reason;
    JpegLayout L;
    if (!jpeg_layout(hd.h, hd.w, hd.sampling, &L)) return MVLDM_JPEG_SIZE;
    if (coef_len < (size_t)L.blocks * 64)
        return set_error(MVLDM_ERR_ARG, "jpeg_entropy: room for %zu coefficients, the %d x %d frame has %zu", coef_len, hd.h, hd.w, (size_t)L.blocks * 64);
    quant_rows(hd, L, qt);
    return decode_scan<true>(data, len, hd, L, coef, max_s);
}

extern "C" int mvldm_jpeg_idct_host(const int16_t* coef, const uint16_t* qt, uint8_t* dst, int h, int w, int sampling) {
    if (coef == nullptr || qt == nullptr || dst == nullptr) return set_error(MVLDM_ERR_ARG, "jpeg_idct_host: null pointer");
    JpegLayout L;
    if (!jpeg_layout(h, w, sampling, &L)) return set_error(MVLDM_ERR_ARG, "jpeg_idct_host: frame %d x %d, sampling %d", h, w, sampling);
    uint8_t* planes = new uint8_t[(size_t)L.blocks * 64];
    for (int c = 0; c < L.ncomp; ++c) {
        const int ld = L.bw[c] * 8;
        uint8_t* plane = planes + (size_t)L.off[c] * 64;
        for (int by = 0; by < L.bh[c]; ++by)
            for (int bx = 0; bx < L.bw[c]; ++bx) {
                const int16_t* blk = coef + ((size_t)L.off[c] + (size_t)by * L.bw[c] + bx) * 64;
                int32_t ws[8][8], v[8];
                for (int x = 0; x < 8; ++x) {           // columns
                    for (int k = 0; k < 8; ++k) v[k] = (int32_t)blk[k * 8 + x] * (int32_t)qt[c * 64 + k * 8 + x];
                    jpeg_idct_1d(v, 11);
                    for (int k = 0; k < 8; ++k) ws[k][x] = v[k];
                }
                for (int y = 0; y < 8; ++y) {           // rows
                    jpeg_idct_1d(ws[y], 18);
                    for (int x = 0; x < 8; ++x) plane[(size_t)(by * 8 + y) * ld + bx * 8 + x] = (uint8_t)jpeg_sample(ws[y][x]);
                }
            }
    }
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const uint32_t px = jpeg_pixel(planes, L, y, x);
            uint8_t* o = dst + ((size_t)y * w + x) * 3;
            o[0] = (uint8_t)px;
            o[1] = (uint8_t)(px >> 8);
            o[2] = (uint8_t)(px >> 16);
        }
    delete[] planes;
    return MVLDM_OK;
}

// ---- the scan on the device: what the host still does, and the emulations of jpeg_huff.hip's two forms ----------------------------------
namespace mvldm {
namespace {

// The front of the two prepares: the argument checks (at least min_room bytes behind the offset), the header into *hd and `info`, the
// descriptor reset and the layout.  false: *rc is the prepare's answer.
bool prepare_front(const char* name, const uint8_t* data, size_t len, uint8_t* scan, size_t scan_off, size_t scan_room, size_t min_room, int32_t* desc,
                   uint8_t* tables, int32_t* info, Header* hd, JpegLayout* L, int* rc) {
    *rc = MVLDM_JPEG_OK;
    if (data == nullptr || scan == nullptr || desc == nullptr || tables == nullptr) {
        *rc = set_error(MVLDM_ERR_ARG, "%s: null pointer", name);
    } else if ((scan_off & 15) || len >= ((size_t)1 << 28) || scan_room > 0x7FFFFFFFu || scan_room < scan_off || scan_room - scan_off < min_room) {
        *rc = set_error(MVLDM_ERR_ARG, "%s: offset %zu of %zu bytes for a frame of %zu (a multiple of 16, %zu bytes or more behind it, below 2^31)", name, scan_off,
                        scan_room, len, min_room);
    } else {
        *rc = parse_header(data, len, hd);
        if (info) fill_info(*hd, *rc, info);
        desc[0] = (int32_t)scan_off;
        desc[1] = desc[2] = desc[3] = 0;
        if (*rc == MVLDM_JPEG_OK && !jpeg_layout(hd->h, hd->w, hd->sampling, L)) *rc = MVLDM_JPEG_SIZE;
    }
    return *rc == MVLDM_JPEG_OK;
}

// intervals of the frame, MCUs to an interval (a frame without DRI, or with one at or above its MCUs, is one interval), and the bytes
// its region can occupy: at most huff_rst_room(len)
size_t rst_plan(const Header& hd, const JpegLayout& L, size_t len, uint32_t* n_int, uint32_t* ri, size_t* table_bytes) {
    const uint32_t mcus = (uint32_t)(L.mcux * L.mcuy);
    *ri = hd.restart != 0 && (uint32_t)hd.restart < mcus ? (uint32_t)hd.restart : mcus;
    *n_int = (mcus + *ri - 1) / *ri;
    const size_t scan_len = len - hd.scan, most = huff_rst_max_intervals(scan_len), cap = *n_int < most ? (size_t)*n_int : most;
    *table_bytes = huff_rst_table_bytes(cap);           // a stream too short for its markers is refused before entry `cap` is written
    return huff_rst_need(scan_len, cap);
}

// a marker structure prepare cannot lay down: decode_scan's own reason for the stream
int rst_refusal(const uint8_t* data, size_t len, const Header& hd, const JpegLayout& L) {
    const int reason = decode_scan<false>(data, len, hd, L, nullptr, nullptr);
    return reason == MVLDM_JPEG_OK || reason == MVLDM_JPEG_RANGE ? MVLDM_JPEG_CORRUPT : reason;
}

struct HuffEmul {               // what a kernel keeps in LDS and in its threads' registers, one entry per thread of a chunk
    std::vector<HuffState> buf[2], entry;       // the exit states twice: the barrier of a round is the swap of the two
    std::vector<uint32_t> done, ex, pre;
    std::vector<HuffRstLane> lane;
    uint32_t sb, T;             // bits of a subsequence, subsequences of a chunk
    HuffGeom G;
    size_t count;               // coefficients of a frame
    uint8_t zigzag[64];
};

// The emulations' argument checks and buffers.
int emul_open(const char* name, const void* scan, const void* desc, const void* tables, int n_img, int h, int w, int sampling, const void* coef, const void* qt,
              const void* status, int subseq_bits, int chunk_subseqs, HuffEmul* E) {
    if (scan == nullptr || desc == nullptr || tables == nullptr || coef == nullptr || qt == nullptr || status == nullptr)
        return set_error(MVLDM_ERR_ARG, "%s: null pointer", name);
    JpegLayout L;
    if (n_img < 0 || !jpeg_layout(h, w, sampling, &L)) return set_error(MVLDM_ERR_ARG, "%s: %d frames of %d x %d, sampling %d", name, n_img, h, w, sampling);
    if (!huff_bits_ok(subseq_bits) || chunk_subseqs < 0 || chunk_subseqs > (1 << 20))
        return set_error(MVLDM_ERR_ARG, "%s: subseq_bits %d (0, or a multiple of 32 in 32 .. %d), chunk of %d", name, subseq_bits, kHuffMaxBits, chunk_subseqs);
    E->sb = subseq_bits ? (uint32_t)subseq_bits : (uint32_t)kHuffDefaultBits;
    E->T = chunk_subseqs ? (uint32_t)chunk_subseqs : (uint32_t)kHuffChunk;
    E->G = huff_geom(L);
    E->count = (size_t)L.blocks * 64;
    for (auto* v : {&E->buf[0], &E->buf[1], &E->entry}) v->resize(E->T);
    for (auto* v : {&E->done, &E->ex, &E->pre}) v->resize(E->T);
    E->lane.resize(E->T);
    for (uint32_t i = 0; i < 64; ++i) E->zigzag[i] = huff_zigzag(i);
    return MVLDM_OK;
}

// One chunk of n_act subsequences described by E.lane: cold pass, rounds, segmented scan of the completed blocks, write pass.
// Returns the blocks the chunk completed; *carry is the last thread's exit.
uint32_t huff_chunk(HuffEmul& E, uint32_t n_act, const uint8_t* tab, int16_t* cf, uint32_t* bad, uint32_t* ended, HuffState* carry, uint32_t* rounds_max) {
    const HuffGeom& G = E.G;
    const uint32_t sb = E.sb;
    HuffNoSink none;
    for (uint32_t i = 0; i < n_act; ++i) {              // cold pass
        const HuffRstLane& ln = E.lane[i];
        HuffState st = E.entry[i] = huff_rst_cold(ln, sb);
        huff_run(ln.sc, ln.bits, tab, G.nl, G.nb, huff_rst_end(ln, sb), sb, &st, &E.done[i], &none);
        E.buf[0][i] = st;
    }
    int cur = 0;
    uint32_t rounds = 0;
    for (uint32_t r = 0; r < n_act; ++r) {
        bool any = false;
        for (uint32_t i = 0; i < n_act; ++i) {
            const HuffRstLane& ln = E.lane[i];
            HuffState st = E.buf[cur][i];
            if (!ln.first && !huff_same(E.buf[cur][i - 1], E.entry[i])) {
                E.entry[i] = st = E.buf[cur][i - 1];
                huff_run(ln.sc, ln.bits, tab, G.nl, G.nb, huff_rst_end(ln, sb), sb, &st, &E.done[i], &none);
                any = true;
            }
            E.buf[cur ^ 1][i] = st;
        }
        cur ^= 1;
        ++rounds;
        if (!any) break;
    }
    if (rounds > *rounds_max) *rounds_max = rounds;
    uint32_t blocks = 0;
    for (uint32_t i = 0; i < n_act; ++i) {
        E.ex[i] = blocks;
        blocks += E.done[i];
    }
    for (uint32_t i = 0; i < n_act; ++i) {              // write pass
        const HuffRstLane& ln = E.lane[i];
        HuffCoefSink sink{cf, E.zigzag, G, ln.base + E.ex[i] - E.ex[ln.start], ln.limit, ln.bits, 0u, bad, nullptr};
        sink.open();
        HuffState st = E.entry[i];
        uint32_t again = 0;
        huff_run(ln.sc, ln.bits, tab, G.nl, G.nb, huff_rst_end(ln, sb), sb, &st, &again, &sink);
        *ended += sink.ended;
    }
    *carry = E.buf[cur][n_act - 1];
    return blocks;
}

// One stream (a frame without intervals, or an interval of more than a chunk) of `bits` bits whose blocks are base .. limit: its
// chunks in order, the first lane of each entering with the carry of the chunk before.
void huff_stream(HuffEmul& E, const uint8_t* sc, uint32_t bits, uint32_t base, uint32_t limit, const uint8_t* tab, int16_t* cf, uint32_t* bad, uint32_t* ended,
                 uint32_t* rounds_max) {
    const uint32_t cnt = huff_rst_count(bits, E.sb);
    HuffState carry = {0u, 0u};
    for (uint32_t ch0 = 0; ch0 < cnt; ch0 += E.T) {
        const uint32_t n_act = cnt - ch0 < E.T ? cnt - ch0 : E.T;
        for (uint32_t i = 0; i < n_act; ++i) E.lane[i] = HuffRstLane{sc, bits, ch0 + i, 0u, base, limit, carry, i == 0};
        base += huff_chunk(E, n_act, tab, cf, bad, ended, &carry, rounds_max);
    }
}

// A frame's slot and tables before its scan is decoded.
const uint8_t* emul_frame(const HuffEmul& E, int img, const uint8_t* tables, int16_t* coef, uint16_t* qt, int16_t** cf) {
    const uint8_t* tab = tables + (size_t)img * kHuffBlobBytes;
    *cf = coef + (size_t)img * E.count;
    memset(*cf, 0, E.count * sizeof(int16_t));
    memcpy(qt + (size_t)img * 192, tab + kHuffTabsBytes, 192 * sizeof(uint16_t));
    return tab;
}

// The second launch and the status words of a frame whose scan gave `reason`: DC prefixes per interval of ri MCUs in scan order (a
// frame without intervals: ri = its MCUs), S of every block.
void emul_finish(const HuffGeom& G, uint32_t ri, int16_t* cf, const uint16_t* q, int reason, uint32_t rounds_max, uint32_t n_int, int32_t* status) {
    int32_t worst = 0;
    if (reason == MVLDM_JPEG_OK) {
        bool bad = false;
        for (uint32_t c = 0; c < G.ncomp; ++c) {
            const uint32_t per = c == 0 ? G.nl : 1u, nc = G.mcus * per, period = ri * per;
            long long pred = 0;
            for (uint32_t j = 0; j < nc; ++j) {
                const uint32_t m = c == 0 ? j / G.nl : j, b = c == 0 ? j - m * G.nl : G.nl + c - 1;
                int16_t* blk = cf + (size_t)huff_block_index(G, m, b) * 64;
                bool f = j % period == 0;
                long long v = blk[0];
                huff_rst_join(false, pred, &f, &v);
                pred = v;
                if (pred < -32768 || pred > 32767) {
                    bad = true;
                    continue;
                }
                blk[0] = (int16_t)pred;
                int32_t sum = 0;
                for (int k = 0; k < 64; ++k) sum += (blk[k] < 0 ? -(int32_t)blk[k] : (int32_t)blk[k]) * (int32_t)q[c * 64 + k];
                if (sum > worst) worst = sum;
            }
        }
        reason = bad ? MVLDM_JPEG_CORRUPT : worst > kJpegGuard ? MVLDM_JPEG_RANGE : MVLDM_JPEG_OK;
        if (bad) worst = 0;
    }
    status[0] = reason;
    status[1] = worst;
    status[2] = (int32_t)rounds_max;
    status[3] = (int32_t)n_int;
}

inline int32_t rst_word(const uint8_t* region, size_t i) {          // the host's packed buffer need not be aligned
    int32_t v;
    memcpy(&v, region + 4 * i, 4);
    return v;
}

}  // namespace
}  // namespace mvldm

extern "C" size_t mvldm_jpeg_scan_room(size_t len) { return huff_scan_room(len); }

extern "C" int mvldm_jpeg_scan_prepare(const uint8_t* data, size_t len, uint8_t* scan, size_t scan_off, size_t scan_room, int32_t* desc, uint8_t* tables,
                                       int32_t* info) {
    Header hd;
    JpegLayout L;
    int rc;
    if (!prepare_front("jpeg_scan_prepare", data, len, scan, scan_off, scan_room, huff_scan_room(len), desc, tables, info, &hd, &L, &rc)) return rc;
    if (hd.restart != 0) return MVLDM_JPEG_RESTART;
    // the entropy-coded bytes up to the first marker, FF 00 -> FF
    uint8_t* out = scan + scan_off;
    size_t n = 0, i = hd.scan;
    while (true) {
        if (i >= len) return MVLDM_JPEG_TRUNCATED;
        const uint8_t b = data[i];
        if (b == 0xFF) {
            if (i + 1 >= len) return MVLDM_JPEG_TRUNCATED;
            if (data[i + 1] != 0x00) break;
            i += 2;
        } else {
            ++i;
        }
        out[n++] = b;                           // n <= i - hd.scan < len
    }
    const int tail = expect_eoi(data, len, i);  // i sits on the marker's FF
    if (tail != MVLDM_JPEG_OK) return tail;
    const size_t room = huff_scan_room(n);      // <= huff_scan_room(len)
    memset(out + n, 0, room - n);
    desc[1] = (int32_t)(n * 8);
    desc[2] = (int32_t)room;
    tables_blob(hd, L, tables);
    return MVLDM_JPEG_OK;
}

extern "C" int mvldm_jpeg_entropy_chunk_subseqs(void) { return kHuffChunk; }

extern "C" int mvldm_jpeg_entropy_emul_host(const uint8_t* scan, size_t scan_bytes, const int32_t* desc, const uint8_t* tables, int n_img, int h, int w,
                                            int sampling, int16_t* coef, uint16_t* qt, int32_t* status, int subseq_bits, int chunk_subseqs) {
    HuffEmul E;
    const int rc = emul_open("jpeg_entropy_emul_host", scan, desc, tables, n_img, h, w, sampling, coef, qt, status, subseq_bits, chunk_subseqs, &E);
    if (rc != MVLDM_OK) return rc;
    for (int img = 0; img < n_img; ++img) {
        int16_t* cf;
        const uint8_t* tab = emul_frame(E, img, tables, coef, qt, &cf);
        const int32_t* d = desc + (size_t)img * 4;
        uint32_t rounds_max = 0, bad = 0, ended = 0;
        if (huff_desc_ok(d, scan_bytes)) huff_stream(E, scan + d[0], (uint32_t)d[1], 0u, E.G.total, tab, cf, &bad, &ended, &rounds_max);      // the frame: one interval
        emul_finish(E.G, E.G.mcus, cf, qt + (size_t)img * 192, !bad && ended == 1u ? MVLDM_JPEG_OK : MVLDM_JPEG_CORRUPT, rounds_max, 0u, status + (size_t)img * 4);
    }
    return MVLDM_OK;
}

extern "C" size_t mvldm_jpeg_rst_room(size_t len) { return huff_rst_room(len); }

extern "C" size_t mvldm_jpeg_rst_need(const uint8_t* data, size_t len) {
    if (data == nullptr) return 0;
    Header hd;
    JpegLayout L;
    if (parse_header(data, len, &hd) != MVLDM_JPEG_OK || !jpeg_layout(hd.h, hd.w, hd.sampling, &L)) return 0;
    uint32_t n_int, ri;
    size_t table_bytes;
    return rst_plan(hd, L, len, &n_int, &ri, &table_bytes);
}

extern "C" int mvldm_jpeg_rst_prepare(const uint8_t* data, size_t len, uint8_t* scan, size_t scan_off, size_t scan_room, int32_t* desc, uint8_t* tables,
                                      int32_t* info) {
    Header hd;
    JpegLayout L;
    int rc;
    if (!prepare_front("jpeg_rst_prepare", data, len, scan, scan_off, scan_room, 0, desc, tables, info, &hd, &L, &rc)) return rc;
    uint32_t n_int, ri;
    size_t T;
    const size_t need = rst_plan(hd, L, len, &n_int, &ri, &T);
    if (scan_room - scan_off < need)
        return set_error(MVLDM_ERR_ARG, "jpeg_rst_prepare: %zu bytes behind offset %zu, the frame can need %zu (mvldm_jpeg_rst_need; at most mvldm_jpeg_rst_room)",
                         scan_room - scan_off, scan_off, need);
    // one walk of the scan: FF 00 -> FF, fill bytes and RSTn dropped, every interval at a 4-byte aligned offset, its pair into the table
    uint8_t* out = scan + scan_off;
    memset(out, 0, T);
    size_t w = T, first = T, i = hd.scan;
    uint32_t g = 0;
    int next_rst = 0;
    auto close = [&]() {
        const int32_t pair[2] = {(int32_t)first, (int32_t)((w - first) * 8)};
        memcpy(out + 8 * (size_t)g, pair, 8);           // g < cap: every interval in front of this one ended at a marker of two bytes
        ++g;
    };
    while (true) {
        if (i >= len) return rst_refusal(data, len, hd, L);
        const uint8_t b = data[i];
        if (b != 0xFF) {
            out[w++] = b;                               // w - T <= bytes read - 2 markers' + 3 of padding an interval: below need - 16
            ++i;
            continue;
        }
        if (i + 1 >= len) return rst_refusal(data, len, hd, L);
        if (data[i + 1] == 0x00) {
            out[w++] = 0xFF;
            i += 2;
            continue;
        }
        if (g + 1 < n_int) {                            // RSTn, counted 0 .. 7, after any number of fill bytes
            size_t p = i;
            while (p < len && data[p] == 0xFF) ++p;
            if (p >= len || data[p] != 0xD0 + next_rst) return rst_refusal(data, len, hd, L);
            close();
            next_rst = (next_rst + 1) & 7;
            while (w & 3) out[w++] = 0;
            first = w;
            i = p + 1;
        } else {                                        // behind the last interval: EOI
            if (expect_eoi(data, len, i) != MVLDM_JPEG_OK) return rst_refusal(data, len, hd, L);
            close();
            break;
        }
    }
    const size_t total = T + huff_scan_room(w - T);     // <= need
    memset(out + w, 0, total - w);
    desc[1] = (int32_t)n_int;
    desc[2] = (int32_t)total;
    desc[3] = (int32_t)ri;
    tables_blob(hd, L, tables);
    return MVLDM_JPEG_OK;
}

extern "C" int mvldm_jpeg_rst_entropy_emul_host(const uint8_t* scan, size_t scan_bytes, const int32_t* desc, const uint8_t* tables, int n_img, int h, int w,
                                                int sampling, int16_t* coef, uint16_t* qt, int32_t* status, int subseq_bits, int chunk_subseqs) {
    HuffEmul E;
    const int rc = emul_open("jpeg_rst_entropy_emul_host", scan, desc, tables, n_img, h, w, sampling, coef, qt, status, subseq_bits, chunk_subseqs, &E);
    if (rc != MVLDM_OK) return rc;
    const HuffGeom& G = E.G;
    const uint32_t sb = E.sb, T = E.T;
    for (int img = 0; img < n_img; ++img) {
        int16_t* cf;
        const uint8_t* tab = emul_frame(E, img, tables, coef, qt, &cf);
        const int32_t* d = desc + (size_t)img * 4;
        int reason = MVLDM_JPEG_CORRUPT;
        uint32_t rounds_max = 0, n_int = 0, ri = 1;
        if (huff_rst_desc_ok(d, scan_bytes, G.mcus)) {
            const uint8_t* region = scan + d[0];
            n_int = (uint32_t)d[1];
            ri = (uint32_t)d[3];
            bool wrong = false;                         // the whole table against the descriptor before any scan bit is read
            for (uint32_t g = 0; g < n_int; ++g) wrong = wrong || !huff_rst_entry_ok(rst_word(region, 2 * (size_t)g), rst_word(region, 2 * (size_t)g + 1), d);
            uint32_t bad = 0, ended = 0;
            for (uint32_t g0 = 0; g0 < n_int && !wrong;) {
                // the batch: the longest run of whole intervals from g0 whose subsequences fit a chunk
                uint32_t nbi = 0, sum = 0;
                for (uint32_t j = 0; j < T && g0 + j < n_int; ++j) {
                    sum += huff_rst_count_capped((uint32_t)rst_word(region, 2 * (size_t)(g0 + j) + 1), sb, T);
                    E.pre[j] = sum;
                    if (sum > T) break;                 // the sums only grow: the batch ends here
                    nbi = j + 1;
                }
                if (nbi == 0) {                         // an interval of more than a chunk: walked alone
                    uint32_t base, limit;
                    huff_rst_blocks(G, g0, ri, &base, &limit);
                    huff_stream(E, region + rst_word(region, 2 * (size_t)g0), (uint32_t)rst_word(region, 2 * (size_t)g0 + 1), base, limit, tab, cf, &bad, &ended,
                                &rounds_max);
                    g0 += 1;
                } else {
                    const uint32_t n_act = E.pre[nbi - 1];
                    for (uint32_t i = 0; i < n_act; ++i) {
                        const uint32_t j = huff_rst_find(E.pre.data(), nbi, i), start = j ? E.pre[j - 1] : 0u;
                        uint32_t base, limit;
                        huff_rst_blocks(G, g0 + j, ri, &base, &limit);
                        E.lane[i] = HuffRstLane{region + rst_word(region, 2 * (size_t)(g0 + j)), (uint32_t)rst_word(region, 2 * (size_t)(g0 + j) + 1), i - start, start, base,
                                                limit, HuffState{0u, 0u}, i == start};
                    }
                    HuffState carry;
                    huff_chunk(E, n_act, tab, cf, &bad, &ended, &carry, &rounds_max);
                    g0 += nbi;
                }
            }
            if (!wrong && !bad && ended == n_int) reason = MVLDM_JPEG_OK;
        }
        emul_finish(G, ri, cf, qt + (size_t)img * 192, reason, rounds_max, n_int, status + (size_t)img * 4);
    }
    return MVLDM_OK;
}
