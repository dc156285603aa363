// What the device entropy decoders (jpeg_huff.hip: the plain and the restart form) and their host emulations (jpeg_host.cpp,
// mvldm_jpeg_entropy_emul_host and mvldm_jpeg_rst_entropy_emul_host) share: the bit window, the one-symbol step of the decoder state
// (p, b, k), the address of a block, the store of a coefficient and a lane's description of its subsequence -- written once, so that the
// kernels and the emulations run the same statements (include/mvldm.h, "JPEG frames: the scan on the device").
// No HIP call and no other header of the library.
#pragma once
#include "jpeg_common.h"

namespace mvldm {

// ---- the prepared frame ------------------------------------------------------------------------------------------------------------
// Scan: the destuffed bytes in STREAM order at a 16-byte aligned offset, zero padding up to huff_scan_room(bytes).  A lane reads aligned
// dwords and swaps their bytes (v_perm), so that bit 31 of a word is the oldest bit: the choice keeps prepare a plain byte copy.
// The decoder holds three consecutive words; the furthest it touches for a symbol that starts at bit p < bit_len is word (p >> 5) + 2,
// i.e. a byte below bytes + 12: the padding is 16 bytes and more.
constexpr int kHuffTabBytes = MVLDM_JPEG_HUFF_TABLE_BYTES;         // look u16[512] | maxcode i32[18] | valoff i32[18] | vals u8[256]
constexpr int kHuffLookOff = 0, kHuffMaxOff = 1024, kHuffValOff = 1096, kHuffValsOff = 1168;
constexpr int kHuffTabsBytes = 6 * kHuffTabBytes;                  // [component][DC, AC]
constexpr int kHuffBlobBytes = MVLDM_JPEG_TABLE_BYTES;             // the six tables, then qt u16[3][64]
constexpr int kHuffLook = 9;
constexpr int kHuffChunk = 1024;                                   // subsequences of a chunk on the device: one per thread of the workgroup
constexpr int kHuffDefaultBits = 512;                              // measured on the MI355X against 128, 256 and 1024: DESIGN.md 3.7
constexpr int kHuffMaxBits = 1 << 16;
static_assert(kHuffValsOff + 256 == kHuffTabBytes && kHuffTabsBytes + 384 == kHuffBlobBytes, "table blob layout");

MVLDM_HD size_t huff_scan_room(size_t bytes) { return ((bytes + 15) & ~(size_t)15) + 16; }
MVLDM_HD bool huff_bits_ok(int subseq_bits) { return subseq_bits == 0 || (subseq_bits >= 32 && subseq_bits <= kHuffMaxBits && subseq_bits % 32 == 0); }

// desc[0..3] = offset of the scan in the packed buffer, bit_len, bytes occupied (padding included), 0.  false: the frame is not read.
MVLDM_HD bool huff_desc_ok(const int32_t* d, size_t scan_bytes) {
    if (d[0] < 0 || d[1] < 0 || (d[0] & 15)) return false;
    const size_t need = huff_scan_room(((size_t)d[1] + 7) >> 3);
    return (size_t)d[0] <= scan_bytes && scan_bytes - (size_t)d[0] >= need;
}

// ---- geometry: the scalar fields of a JpegLayout the decoder needs (selects instead of runtime indices into a kernel argument) -------
struct HuffGeom {
    uint32_t nl, nb;            // luma blocks and all blocks of an MCU
    uint32_t hmax, mcux, mcus;
    uint32_t bw0, bw1;          // blocks per row of the luma and of a chroma grid
    uint32_t off1, off2;        // first block of Cb and Cr
    uint32_t total;             // blocks of the frame = mcus * nb
    uint32_t vmax, ncomp;
};
MVLDM_HD HuffGeom huff_geom(const JpegLayout& L) {
    HuffGeom G;
    G.nl = (uint32_t)(L.hmax * L.vmax);
    G.nb = L.ncomp == 3 ? G.nl + 2 : 1;
    G.hmax = (uint32_t)L.hmax;
    G.vmax = (uint32_t)L.vmax;
    G.mcux = (uint32_t)L.mcux;
    G.mcus = (uint32_t)(L.mcux * L.mcuy);
    G.bw0 = (uint32_t)L.bw[0];
    G.bw1 = (uint32_t)L.bw[1];
    G.off1 = (uint32_t)L.off[1];
    G.off2 = (uint32_t)L.off[2];
    G.total = (uint32_t)L.blocks;
    G.ncomp = (uint32_t)L.ncomp;
    return G;
}
// block b of MCU m -> its index in the frame's coefficient slot: the host decoder's address (component, by, bx)
MVLDM_HD uint32_t huff_block_index(const HuffGeom& G, uint32_t m, uint32_t b) {
    const uint32_t my = m / G.mcux, mx = m - my * G.mcux;
    if (b < G.nl) {
        const uint32_t by = b / G.hmax, bx = b - by * G.hmax;
        return (my * G.vmax + by) * G.bw0 + mx * G.hmax + bx;
    }
    return (b == G.nl ? G.off1 : G.off2) + my * G.bw1 + mx;
}

// zigzag position -> natural (row-major) index; the kernel copies the 64 bytes into LDS, the emulation into a local table
MVLDM_HD uint8_t huff_zigzag(uint32_t i) {
    constexpr uint8_t z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return z[i & 63];
}

// ---- the bit window ----------------------------------------------------------------------------------------------------------------
MVLDM_HD uint32_t huff_word(const uint8_t* scan, uint32_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bswap32(((const uint32_t*)scan)[i]);
#else
    const uint8_t* q = scan + 4 * (size_t)i;
    return ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | (uint32_t)q[3];
#endif
}
struct HuffWin {
    uint32_t wi, w0, w1, w2;    // words wi, wi + 1, wi + 2 of the scan; w2 is loaded one word ahead of its first use
};
MVLDM_HD void huff_seek(HuffWin* W, const uint8_t* scan, uint32_t p) {
    W->wi = p >> 5;
    W->w0 = huff_word(scan, W->wi);
    W->w1 = huff_word(scan, W->wi + 1);
    W->w2 = huff_word(scan, W->wi + 2);
}
// the 32 bits that start at bit p, oldest highest
MVLDM_HD uint32_t huff_peek32(HuffWin* W, const uint8_t* scan, uint32_t p) {
    const uint32_t i = p >> 5;
    if (i != W->wi) {
        if (i == W->wi + 1) {   // a symbol is at most 31 bits long: the common case
            W->wi = i;
            W->w0 = W->w1;
            W->w1 = W->w2;
            W->w2 = huff_word(scan, i + 2);
        } else {
            huff_seek(W, scan, p);
        }
    }
    const uint32_t s = p & 31;
    return s ? (W->w0 << s) | (W->w1 >> (32 - s)) : W->w0;
}

// ---- the state and its step ----------------------------------------------------------------------------------------------------------
// p: bit position.  bk = b | k << 8: b the block of the MCU the next symbol belongs to, k its zigzag position (0: a DC category).
// The step is a total function of (state, bits): what decode_scan (jpeg_host.cpp) refuses is a FAULT here -- reported to the sink, and
// the decode goes on by a fixed rule: a code that does not exist skips one bit; a DC category above 15 counts as 0; a coefficient index
// above 63 consumes its bits and ends the block; a symbol whose bits run past bit_len gives DEAD = (bit_len, kHuffDead), which passes
// through every later subsequence unchanged (p = bit_len is at or beyond every end).  A decoder that started at a wrong bit faults all
// the time; had the first fault been absorbing, no cold start would ever meet the true sequence of states and every chunk would need its
// full count of rounds (measured: 1020 of 1024).  Only the write pass, whose entries are true, listens: its first fault in front of the
// frame's last block is the one decode_scan returns at, so acceptance is the same.  A run of sixteen zeros that passes index 63 ends
// the block without a fault, as in decode_scan.  Every rule advances p by at least one bit.
struct HuffState {
    uint32_t p, bk;
};
constexpr uint32_t kHuffDead = 0x80000000u;
MVLDM_HD bool huff_same(const HuffState& a, const HuffState& b) { return a.p == b.p && a.bk == b.bk; }

struct HuffNoSink {
    MVLDM_HD void put(uint32_t, int) {}
    MVLDM_HD void done(uint32_t) {}
    MVLDM_HD void fault() {}
};
// The write pass's sink, of the plain and of the restart form: n is the absolute index (scan order) of the block being decoded, limit the
// end of the blocks this lane's stream may fill -- the frame's (G.total) on the plain path, the interval's on the restart path -- and bits
// the length of that stream.  Every store is guarded by n < limit <= blocks of the frame, so the padding bits of one interval never write
// into the next.  `ended`: block limit - 1 completed in this subsequence; decode_scan stops there and wants fewer than 8 bits of the
// stream to remain (in front of a marker and at the end), so 8 or more set *bad.  A fault in front of that point sets *bad too: the write
// pass decodes from true entries, so its first fault is the stream's.  A stream is accepted when *bad == 0 and exactly one of its lanes
// reports `ended`.  For the plain path this is the test it had with a shared end position end_p (written where n reached G.total):
// end_p != sentinel && bit_len - end_p < 8 && !bad.  n reaches limit in at most one lane, because the lanes' n continue each other, so
// "one lane ended" is "end_p was written", and bit_len - end_p >= 8 is the case that now sets *bad.
struct HuffCoefSink {
    int16_t* coef;              // the frame's slot
    const uint8_t* zigzag;
    HuffGeom G;
    uint32_t n, limit, bits, ended;
    uint32_t* bad;
    int16_t* blk;
    MVLDM_HD void fault() {
        if (blk != nullptr) *bad = 1u;
    }
    MVLDM_HD void open() {
        if (n < limit) {
            const uint32_t m = n / G.nb;
            blk = coef + (size_t)huff_block_index(G, m, n - m * G.nb) * 64;
        } else {
            blk = nullptr;
        }
    }
    MVLDM_HD void put(uint32_t k, int v) {
        if (blk != nullptr) blk[zigzag[k & 63]] = (int16_t)v;
    }
    MVLDM_HD void done(uint32_t p) {
        ++n;
        if (n == limit) {
            ended = 1u;
            if (bits - p >= 8u) *bad = 1u;
        }
        open();
    }
};

// Decodes from *st while the next symbol starts below `end` (<= bit_len): at most max_steps symbols (every symbol is at least one bit
// long, so end - p bounds them).  *blocks receives the number of blocks completed.  tab: the six tables of the frame (LDS on the device).
template <class Sink>
MVLDM_HD void huff_run(const uint8_t* scan, uint32_t bit_len, const uint8_t* tab, uint32_t nl, uint32_t nb, uint32_t end, uint32_t max_steps, HuffState* st,
                       uint32_t* blocks, Sink* sink) {
    uint32_t p = st->p, bk = st->bk, nblk = 0;
    if (!(bk & kHuffDead) && p < end) {
        HuffWin W;
        huff_seek(&W, scan, p);
        for (uint32_t it = 0; it < max_steps && p < end; ++it) {
            uint32_t b = bk & 255u, k = bk >> 8;
            const uint32_t w = huff_peek32(&W, scan, p);
            const uint32_t c = b < nl ? 0u : b - nl + 1u;
            const uint8_t* t = tab + (2u * c + (k != 0u ? 1u : 0u)) * (uint32_t)kHuffTabBytes;
            const uint32_t v16 = w >> 16;
            const uint32_t e = ((const uint16_t*)(t + kHuffLookOff))[v16 >> (16 - kHuffLook)];
            uint32_t l = e >> 8, sym = e & 255u;
            if (e == 0u) {
                const int32_t* maxcode = (const int32_t*)(t + kHuffMaxOff);
                const int32_t* valoff = (const int32_t*)(t + kHuffValOff);
                for (uint32_t ll = kHuffLook + 1; ll <= 16u; ++ll) {
                    const int32_t code = (int32_t)(v16 >> (16u - ll));
                    if (code <= maxcode[ll]) {
                        l = ll;
                        sym = (t + kHuffValsOff)[(uint32_t)(code + valoff[ll]) & 255u];
                        break;
                    }
                }
            }
            if (l == 0u) {                      // a code that does not exist: a fault; try the next bit
                sink->fault();
                ++p;
                continue;
            }
            bool done = false, skip = false;
            uint32_t s;
            if (k == 0u) {
                s = sym;
                if (s > 15u) {                  // a DC category that does not exist: a fault; taken as category 0
                    sink->fault();
                    s = 0u;
                }
            } else {
                s = sym & 15u;
                const uint32_t r = sym >> 4;
                if (s == 0u) {
                    if (r == 15u) {
                        k += 16u;
                        done = k >= 64u;
                    } else {
                        done = true;
                    }
                } else {
                    k += r;
                    if (k > 63u) {              // a coefficient behind the last: a fault; its bits are consumed and the block ends
                        sink->fault();
                        done = skip = true;
                    }
                }
            }
            if (l + s > bit_len - p) {          // the symbol's bits run past the end: a fault, and the end of every decode (DEAD)
                sink->fault();
                p = bit_len;
                bk = kHuffDead;
                break;
            }
            if (s != 0u && !skip) {
                const int bits = (int)((w << l) >> (32u - s));
                sink->put(k, bits < (1 << (s - 1u)) ? bits - (1 << s) + 1 : bits);
            }
            if (!done && (s != 0u || k == 0u)) {
                ++k;
                done = k >= 64u;
            }
            p += l + s;
            if (done) {
                ++nblk;
                sink->done(p);
                b = b + 1u == nb ? 0u : b + 1u;
                k = 0u;
            }
            bk = b | (k << 8);
        }
    }
    st->p = p;
    st->bk = bk;
    *blocks = nblk;
}

// ---- restart intervals (jpeg_huff.hip jpeg_rst_*_kernel, mvldm_jpeg_rst_entropy_emul_host) -------------------------------------------
// A frame's region of the packed buffer: the interval table -- int32 pairs (byte offset inside the region, exact bit length), n of them,
// rounded up to 16 bytes -- then the destuffed intervals, each at a 4-byte aligned offset (huff_word reads aligned dwords relative to the
// interval's first byte), and zeros up to huff_scan_room behind the last.  A bit position is relative to its interval, bit_len is the
// interval's: DEAD stays inside it.  desc[0..3] = offset of the region (a multiple of 16), intervals, bytes occupied, MCUs per interval.
MVLDM_HD size_t huff_rst_table_bytes(size_t n) { return (n * 8 + 15) & ~(size_t)15; }
// what a frame with `scan_len` bytes behind its scan header and at most n intervals can occupy: a marker takes two bytes away and the
// alignment in front of the next interval gives at most three back
MVLDM_HD size_t huff_rst_need(size_t scan_len, size_t n) { return huff_rst_table_bytes(n) + huff_scan_room(scan_len + n); }
MVLDM_HD size_t huff_rst_max_intervals(size_t scan_len) { return scan_len / 2 + 1; }
MVLDM_HD size_t huff_rst_room(size_t len) { return huff_rst_need(len, huff_rst_max_intervals(len)); }

// false: nothing of the frame is read
MVLDM_HD bool huff_rst_desc_ok(const int32_t* d, size_t scan_bytes, uint32_t mcus) {
    if (d[0] < 0 || d[1] < 1 || d[2] < 0 || d[3] < 1 || (d[0] & 15) || (uint32_t)d[3] > mcus) return false;
    if ((mcus + (uint32_t)d[3] - 1) / (uint32_t)d[3] != (uint32_t)d[1]) return false;
    if ((size_t)d[2] < huff_rst_table_bytes((size_t)d[1]) + 16) return false;
    return (size_t)d[0] <= scan_bytes && scan_bytes - (size_t)d[0] >= (size_t)d[2];
}
// one pair of the table against the region's descriptor: behind the table, aligned, not empty, and the widest read of a symbol that
// starts at its last bit (12 bytes past its bytes) inside the bytes occupied.  false: no scan bit of the frame is read
MVLDM_HD bool huff_rst_entry_ok(int32_t off, int32_t bits, const int32_t* d) {
    if (off < 0 || bits < 1 || (off & 3) || (size_t)off < huff_rst_table_bytes((size_t)d[1])) return false;
    return (size_t)off + (((size_t)bits + 7) >> 3) + 12 <= (size_t)d[2];
}
// subsequences of an interval; `cap` + 1 stands for anything above cap, so that the sum over a chunk's worth of intervals fits 32 bits
MVLDM_HD uint32_t huff_rst_count(uint32_t bits, uint32_t sb) { return (uint32_t)(((uint64_t)bits + sb - 1) / sb); }
MVLDM_HD uint32_t huff_rst_count_capped(uint32_t bits, uint32_t sb, uint32_t cap) {
    const uint32_t c = huff_rst_count(bits, sb);
    return c > cap ? cap + 1 : c;
}
// pre[0 .. n): inclusive sums of the counts of a batch's intervals (every count >= 1).  The interval of the batch's subsequence t <
// pre[n - 1]: the first j with pre[j] > t
MVLDM_HD uint32_t huff_rst_find(const uint32_t* pre, uint32_t n, uint32_t t) {
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (pre[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// What one thread of a chunk knows about its subsequence: subsequence s of the interval at sc (bits long), whose first subsequence of
// this chunk is thread `start`.  first: the thread does not take its neighbour's exit -- its entry entry0 is true (the interval's
// start, or the carry of the chunk before when an interval is longer than a chunk).  base: the block at which thread `start` begins,
// limit: the end of the interval's blocks, at most the frame's.
struct HuffRstLane {
    const uint8_t* sc;
    uint32_t bits, s, start, base, limit;
    HuffState entry0;
    bool first;
};
MVLDM_HD uint32_t huff_rst_end(const HuffRstLane& ln, uint32_t sb) {
    const uint64_t e = ((uint64_t)ln.s + 1) * sb;
    return e < ln.bits ? (uint32_t)e : ln.bits;
}
MVLDM_HD HuffState huff_rst_cold(const HuffRstLane& ln, uint32_t sb) { return ln.first ? ln.entry0 : HuffState{ln.s * sb, 0u}; }
// interval g of a frame whose intervals hold ri MCUs: its first block and the end of its blocks
MVLDM_HD void huff_rst_blocks(const HuffGeom& G, uint32_t g, uint32_t ri, uint32_t* base, uint32_t* limit) {
    const uint64_t b = (uint64_t)g * ri * G.nb, e = b + (uint64_t)ri * G.nb;
    *base = b < G.total ? (uint32_t)b : G.total;
    *limit = e < G.total ? (uint32_t)e : G.total;
}

// The DC differences of a component in scan order become predictions by a SEGMENTED sum: a block that opens a restart interval (head)
// starts from 0.  (f, v) is the pair of the scan: f says a head lies in the range summed so far.  later after earlier:
MVLDM_HD void huff_rst_join(bool ef, long long ev, bool* f, long long* v) {
    if (!*f) *v += ev;
    *f = *f || ef;
}

}  // namespace mvldm
