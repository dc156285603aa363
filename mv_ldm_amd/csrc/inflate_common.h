// What the device inflate (inflate.hip) and its host twin (inflate_host.cpp, mvldm_png_inflate_host) share: the descriptor check, the bit
// buffer, the canonical-Huffman tables, the sequential step of the decoder and the per-lane halves of what the wave does together --
// written once, so that the kernel and the twin run the same statements (include/mvldm.h, "PNG frames: IDAT inflated on the device").
// A zlib stream (RFC 1950 around RFC 1951) comes from an untrusted file: every function here is total in its state and the bits it is
// given, reads the stream only through inf_word and inf_copy_stored (both bounded by the padded stream) and writes the output only below
// `need`.  No HIP call and no other header of the library.
#pragma once
#include "png_common.h"

namespace mvldm {

constexpr int kInfZdescInts = MVLDM_PNG_ZDESC_INTS;
constexpr int kInfLanes = 64;                   // the lanes of the kernel's wave = the trip count of the twin's lane loops
constexpr int kInfLook = 9;                     // bits of the first-level lookup: codes up to 9 bits take one LDS read
constexpr int kInfBatch = 64;                   // symbols the decoding lane queues before the wave writes them
constexpr uint32_t kInfWindow = 32768;          // the sliding window: DEFLATE's largest distance
constexpr uint32_t kInfMatch = 65536;           // a queue word at or above this is a match (length | distance << 16), below it a literal
constexpr uint32_t kAdlerMod = 65521;

MVLDM_HD size_t inflate_room(size_t bytes) { return ((bytes + 15) & ~(size_t)15) + 16; }
// zdesc[0..3] = offset of the zlib stream in the packed buffer (a multiple of 16), its bytes, 0, 0.  false: the frame is not read.
MVLDM_HD bool inflate_zdesc_ok(const int32_t* zd, size_t z_bytes) {
    if (zd[0] < 0 || zd[1] < 0 || (zd[0] & 15)) return false;
    return (size_t)zd[0] <= z_bytes && z_bytes - (size_t)zd[0] >= inflate_room((size_t)zd[1]);
}

// ---- the bit buffer ---------------------------------------------------------------------------------------------------------------
// DEFLATE packs bits from bit 0 of each byte up, so the little-endian dword i holds stream bits 32 i .. 32 i + 31 in place.  The buffer
// holds 32 .. 63 bits after a refill; a step takes at most 28 (a 15-bit code and 13 extra bits) between two refills.  Words behind the
// padded stream read as 0; the step refuses as soon as more bits were taken than the stream has.
struct InfBits {
    uint64_t buf;
    uint32_t cnt, next, words;          // bits in buf; the next word to load; words of the padded stream
};
MVLDM_HD uint32_t inf_word(const uint8_t* z, uint32_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
    return ((const uint32_t*)z)[i];
#else
    const uint8_t* q = z + 4 * (size_t)i;
    return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
#endif
}
MVLDM_HD void inf_refill(InfBits& B, const uint8_t* z) {
    if (B.cnt < 32) {
        const uint32_t w = B.next < B.words ? inf_word(z, B.next) : 0u;
        B.buf |= (uint64_t)w << B.cnt;
        B.cnt += 32;
        B.next += 1;
    }
}
MVLDM_HD uint32_t inf_take(InfBits& B, int n) {     // n <= 24 (inf_seek; a step takes at most 16 at once), n <= cnt, no more than 28 bits between two refills
    const uint32_t v = (uint32_t)B.buf & ((1u << n) - 1u);
    B.buf >>= n;
    B.cnt -= (uint32_t)n;
    return v;
}
MVLDM_HD uint64_t inf_used(const InfBits& B) { return (uint64_t)B.next * 32 - B.cnt; }
MVLDM_HD void inf_seek(InfBits& B, const uint8_t* z, uint32_t byte) {
    B.next = byte >> 2;
    B.buf = 0;
    B.cnt = 0;
    inf_refill(B, z);
    inf_take(B, (int)(8 * (byte & 3)));
}
MVLDM_HD void inf_byte_align(InfBits& B) { inf_take(B, (int)(B.cnt & 7)); }     // 32 * next is a multiple of 8: the bits used so far are -cnt mod 8

// ---- tables -----------------------------------------------------------------------------------------------------------------------
// A canonical code from its lengths: the symbols sorted by (length, symbol) with the count per length (the bit-by-bit walk for codes
// above kInfLook bits and for patterns no code uses), and a first-level lookup indexed by the next kInfLook stream bits -- the code
// reversed, since a code's first bit is the stream's lowest.  look: symbol | length << 12, 0 where no code of up to kInfLook bits fits.
struct InfTable {
    uint16_t look[1 << kInfLook];
    uint16_t sym[320];
    uint16_t count[16], offs[16], first[16];
    int32_t left, maxlen;               // the code space left over (0: complete, below 0: over-subscribed); the longest length used
};
// the wave clears the lookup and lane L counts the codes of length L
MVLDM_HD void inf_build_count(InfTable& T, const uint8_t* lens, int n, int lane) {
#pragma unroll 1
    for (int i = lane; i < (1 << kInfLook); i += kInfLanes) T.look[i] = 0;
    if (lane < 16) {
        int c = 0;
#pragma unroll 1
        for (int s = 0; s < n; ++s) c += lens[s] == lane ? 1 : 0;
        T.count[lane] = (uint16_t)c;
    }
}
// one lane: where each length starts in `sym`, its first code, and how much of the code space is used
MVLDM_HD void inf_build_offsets(InfTable& T) {
    int left = 1, code = 0, off = 0, maxlen = 0;
    T.offs[0] = 0;
    T.first[0] = 0;
#pragma unroll 1
    for (int L = 1; L < 16; ++L) {
        const int c = T.count[L];
        left = left * 2 - c;
        if (left < -(1 << 20)) left = -(1 << 20);
        T.offs[L] = (uint16_t)off;
        T.first[L] = (uint16_t)code;
        off += c;
        code = ((code + c) * 2) & 0xFFFF;
        if (c) maxlen = L;
    }
    T.left = left;
    T.maxlen = maxlen;
}
MVLDM_HD uint32_t inf_reverse(uint32_t code, int bits) {
    uint32_t r = 0;
    for (int i = 0; i < bits; ++i) r |= ((code >> i) & 1u) << (bits - 1 - i);
    return r;
}
// lane L (1 .. 15) places the symbols of length L in symbol order and fills their lookup entries.  Nothing for an over-subscribed
// set (its codes would not fit their lengths): the step refuses it before a symbol is decoded.
MVLDM_HD void inf_build_place(InfTable& T, const uint8_t* lens, int n, int lane) {
    if (lane < 1 || lane > 15 || T.left < 0) return;
    const int L = lane;
    int r = 0;
#pragma unroll 1
    for (int s = 0; s < n; ++s) {
        if (lens[s] != L) continue;
        T.sym[T.offs[L] + r] = (uint16_t)s;
        if (L <= kInfLook) {
            const uint32_t rev = inf_reverse((uint32_t)T.first[L] + (uint32_t)r, L);
#pragma unroll 1
            for (uint32_t j = rev; j < (1u << kInfLook); j += 1u << L) T.look[j] = (uint16_t)(s | (L << 12));
        }
        ++r;
    }
}
// the next symbol, or -1 where the bits match no code.  Takes at most 15 bits.
MVLDM_HD int inf_decode(const InfTable& T, InfBits& B) {
    const uint32_t e = T.look[(uint32_t)B.buf & ((1u << kInfLook) - 1u)];
    if (e) {
        inf_take(B, (int)(e >> 12));
        return (int)(e & 0xFFFu);
    }
    int code = 0, first = 0, index = 0;
#pragma unroll 1
    for (int L = 1; L < 16; ++L) {
        code |= (int)((B.buf >> (L - 1)) & 1u);
        const int c = T.count[L];
        if (code - c < first) {
            inf_take(B, L);
            return T.sym[index + (code - first)];
        }
        index += c;
        first = (first + c) * 2;
        code *= 2;
    }
    return -1;
}

// ---- what the wave shares ---------------------------------------------------------------------------------------------------------
enum { INF_ACT_NONE = 0, INF_ACT_BUILD_CL, INF_ACT_BUILD, INF_ACT_STORED, INF_ACT_BATCH, INF_ACT_FINISH, INF_ACT_DONE };
struct InfShared {
    uint8_t window[kInfWindow];         // the last 32 KiB of output, byte p at p & 32767: what a match reads
    InfTable lit, dst;                  // dst is the code-length code's table while a dynamic block's lengths are read
    uint8_t lens[320];                  // literal/length lengths, then the distance lengths
    uint8_t cl[20];
    uint32_t q_val[kInfBatch], q_pos[kInfBatch], q_flag[kInfBatch];     // the queue; the lanes' partial sums at the end
    int32_t act, status, n_lit, n_dst;
    uint32_t a0, a1, a2, adler;
};
enum { INF_HEADER = 0, INF_BLOCK, INF_LENS, INF_CHECK, INF_SYMBOLS, INF_TRAILER, INF_END };
struct InfState {                       // the decoding lane's registers
    InfBits B;
    uint32_t pos, need, len;            // bytes written; bytes of the frame's slot; bytes of the zlib stream
    int32_t mode, last;
};
MVLDM_HD void inf_init(InfState& st, uint32_t len, uint32_t need) {
    st.B.buf = 0;
    st.B.cnt = 0;
    st.B.next = 0;
    st.B.words = (uint32_t)(inflate_room(len) >> 2);
    st.pos = 0;
    st.need = need;
    st.len = len;
    st.mode = INF_HEADER;
    st.last = 0;
}
MVLDM_HD int inf_refuse(InfShared& S, int status) {
    S.status = status;
    S.act = INF_ACT_DONE;
    return INF_ACT_DONE;
}
MVLDM_HD uint8_t inf_cl_order(int i) {
    constexpr uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return order[i];
}

// One step of the sequential decoder: runs until the wave has something to do and says what (S.act).  Every step takes at least one
// bit or ends the frame, and refuses once more bits were taken than the stream holds, so 8 * len + 16 steps bound any input.
MVLDM_HD int inf_step(InfState& st, InfShared& S, const uint8_t* z) {
    InfBits& B = st.B;
    const uint64_t bits = (uint64_t)st.len * 8;
    if (inf_used(B) > bits) return inf_refuse(S, MVLDM_PNG_INFLATE);
    S.act = INF_ACT_NONE;
    if (st.mode == INF_HEADER) {
        inf_refill(B, z);
        const uint32_t cmf = inf_take(B, 8), flg = inf_take(B, 8);
        if (st.len < 6 || (cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 32u)) return inf_refuse(S, MVLDM_PNG_INFLATE);
        st.mode = INF_BLOCK;
        return INF_ACT_NONE;
    }
    if (st.mode == INF_BLOCK) {
        inf_refill(B, z);
        st.last = (int32_t)inf_take(B, 1);
        const uint32_t type = inf_take(B, 2);
        if (type == 0) {
            inf_byte_align(B);
            inf_refill(B, z);
            const uint32_t n = inf_take(B, 16), inv = inf_take(B, 16);
            if ((n ^ 0xFFFFu) != inv) return inf_refuse(S, MVLDM_PNG_INFLATE);
            const uint64_t start = inf_used(B) >> 3;
            if (start + n > st.len) return inf_refuse(S, MVLDM_PNG_INFLATE);        // the block's bytes lie inside the stream
            if (n > st.need - st.pos) return inf_refuse(S, MVLDM_PNG_LENGTH);
            S.a0 = (uint32_t)start;
            S.a1 = n;
            S.a2 = st.pos;
            st.pos += n;
            inf_seek(B, z, (uint32_t)start + n);
            st.mode = st.last ? INF_TRAILER : INF_BLOCK;
            S.act = INF_ACT_STORED;
            return INF_ACT_STORED;
        }
        if (type == 1) {
#pragma unroll 1
            for (int s = 0; s < 288; ++s) S.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
#pragma unroll 1
            for (int s = 288; s < 320; ++s) S.lens[s] = 5;      // 32 distance codes: 30 and 31 are part of the code and refused when met
            S.n_lit = 288;
            S.n_dst = 32;
            st.mode = INF_CHECK;
            S.act = INF_ACT_BUILD;
            return INF_ACT_BUILD;
        }
        if (type == 3) return inf_refuse(S, MVLDM_PNG_INFLATE);
        const int nlen = (int)inf_take(B, 5) + 257, ndist = (int)inf_take(B, 5) + 1, ncl = (int)inf_take(B, 4) + 4;
        if (nlen > 286 || ndist > 30) return inf_refuse(S, MVLDM_PNG_INFLATE);
#pragma unroll 1
        for (int i = 0; i < 19; ++i) S.cl[i] = 0;
#pragma unroll 1
        for (int i = 0; i < ncl; ++i) {
            inf_refill(B, z);
            S.cl[inf_cl_order(i)] = (uint8_t)inf_take(B, 3);
        }
        S.n_lit = nlen;
        S.n_dst = ndist;
        st.mode = INF_LENS;
        S.act = INF_ACT_BUILD_CL;
        return INF_ACT_BUILD_CL;
    }
    if (st.mode == INF_LENS) {
        if (S.dst.left != 0) return inf_refuse(S, MVLDM_PNG_INFLATE);              // the code-length code is complete, as zlib asks
        const int total = S.n_lit + S.n_dst;
        int i = 0;
        while (i < total) {
            inf_refill(B, z);
            const int sym = inf_decode(S.dst, B);
            if (sym < 0 || sym > 18) return inf_refuse(S, MVLDM_PNG_INFLATE);
            if (sym < 16) {
                S.lens[i++] = (uint8_t)sym;
                continue;
            }
            int prev = 0, rep;
            if (sym == 16) {
                if (i == 0) return inf_refuse(S, MVLDM_PNG_INFLATE);
                prev = S.lens[i - 1];
                rep = 3 + (int)inf_take(B, 2);
            } else if (sym == 17) {
                rep = 3 + (int)inf_take(B, 3);
            } else {
                rep = 11 + (int)inf_take(B, 7);
            }
            if (i + rep > total) return inf_refuse(S, MVLDM_PNG_INFLATE);
#pragma unroll 1
            for (int k = 0; k < rep; ++k) S.lens[i++] = (uint8_t)prev;
        }
        if (inf_used(B) > bits || S.lens[256] == 0) return inf_refuse(S, MVLDM_PNG_INFLATE);    // no end-of-block code
        st.mode = INF_CHECK;
        S.act = INF_ACT_BUILD;
        return INF_ACT_BUILD;
    }
    if (st.mode == INF_CHECK) {
        // zlib's rule: no over-subscribed set; an incomplete one only where its longest code has one bit (a single code), or for
        // distances where no code is used at all
        if (S.lit.left < 0 || (S.lit.left > 0 && S.lit.maxlen != 1)) return inf_refuse(S, MVLDM_PNG_INFLATE);
        if (S.dst.left < 0 || (S.dst.left > 0 && S.dst.maxlen > 1)) return inf_refuse(S, MVLDM_PNG_INFLATE);
        st.mode = INF_SYMBOLS;
    }
    if (st.mode == INF_SYMBOLS) {
        uint32_t n = 0;
        while (n < (uint32_t)kInfBatch) {
            inf_refill(B, z);
            int sym = inf_decode(S.lit, B);
            if (sym < 0 || inf_used(B) > bits) return inf_refuse(S, MVLDM_PNG_INFLATE);        // bits from behind the stream decide nothing
            if (sym < 256) {
                if (st.pos >= st.need) return inf_refuse(S, MVLDM_PNG_LENGTH);
                S.q_val[n] = (uint32_t)sym;
                S.q_pos[n] = st.pos;
                st.pos += 1;
                n += 1;
            } else if (sym == 256) {
                st.mode = st.last ? INF_TRAILER : INF_BLOCK;
                break;
            } else {
                sym -= 257;
                if (sym >= 29) return inf_refuse(S, MVLDM_PNG_INFLATE);
                const int le = sym < 8 || sym == 28 ? 0 : (sym - 4) >> 2;
                const uint32_t length = (sym < 8 ? 3u + (uint32_t)sym : sym == 28 ? 258u : 3u + ((4u + ((uint32_t)sym & 3u)) << le)) + inf_take(B, le);
                inf_refill(B, z);
                const int ds = inf_decode(S.dst, B);
                if (ds < 0 || ds >= 30) return inf_refuse(S, MVLDM_PNG_INFLATE);
                const int de = ds < 4 ? 0 : (ds - 2) >> 1;
                const uint32_t dist = (ds < 4 ? 1u + (uint32_t)ds : 1u + ((2u + ((uint32_t)ds & 1u)) << de)) + inf_take(B, de);
                if (inf_used(B) > bits) return inf_refuse(S, MVLDM_PNG_INFLATE);
                if (dist > st.pos) return inf_refuse(S, MVLDM_PNG_INFLATE);       // zlib's non-strict rule: no distance beyond what was written
                if (length > st.need - st.pos) return inf_refuse(S, MVLDM_PNG_LENGTH);
                S.q_val[n] = length | (dist << 16);
                S.q_pos[n] = st.pos;
                st.pos += length;
                n += 1;
            }
        }
        S.a0 = n;
        S.act = INF_ACT_BATCH;
        return INF_ACT_BATCH;
    }
    if (st.mode == INF_TRAILER) {
        inf_byte_align(B);
        inf_refill(B, z);
        uint32_t want = inf_take(B, 8) << 24;
        want |= inf_take(B, 8) << 16;
        inf_refill(B, z);
        want |= inf_take(B, 8) << 8;
        want |= inf_take(B, 8);
        if (inf_used(B) != bits) return inf_refuse(S, MVLDM_PNG_INFLATE);          // the trailer cut short, or bytes behind it
        S.adler = want;
        S.a0 = st.pos;
        st.mode = INF_END;
        S.act = INF_ACT_FINISH;
        return INF_ACT_FINISH;
    }
    return inf_refuse(S, MVLDM_PNG_INFLATE);
}

// ---- what each lane does of the wave's work -------------------------------------------------------------------------------------------
// Every byte goes to the window and, below `need`, to the frame's slot.  The step has checked pos + length <= need already; the guard
// stands on its own.
MVLDM_HD void inf_put(InfShared& S, uint8_t* out, uint32_t need, uint32_t p, uint8_t v) {
    S.window[p & (kInfWindow - 1)] = v;
    if (p < need) out[p] = v;
}
// a stored block: a1 bytes from byte a0 of the stream (inside it: the step checked) to position a2
MVLDM_HD void inf_copy_stored(InfShared& S, const uint8_t* z, uint32_t len, uint8_t* out, uint32_t need, int lane) {
#pragma unroll 1
    for (uint32_t k = (uint32_t)lane; k < S.a1; k += kInfLanes) {
        const uint32_t src = S.a0 + k;
        inf_put(S, out, need, S.a2 + k, src < len ? z[src] : (uint8_t)0);
    }
}
// queue entries [i, j): literals, one per lane
MVLDM_HD void inf_put_literals(InfShared& S, uint8_t* out, uint32_t need, uint32_t i, uint32_t j, int lane) {
    const uint32_t e = i + (uint32_t)lane;
    if (e < j && e < (uint32_t)kInfBatch) inf_put(S, out, need, S.q_pos[e], (uint8_t)S.q_val[e]);
}
// a match: byte k of it is byte k mod dist of the dist bytes in front of it, which were all written before this call -- so the lanes
// copy in parallel whether or not the match overlaps itself.  Two halves with a barrier between them: at distances near 32768 the
// window byte one lane writes is the byte another lane reads.  A lane carries its up to five bytes (258 / 64) in one 64-bit word.
MVLDM_HD bool inf_match_ok(uint32_t start, uint32_t length, uint32_t dist) { return dist >= 1 && dist <= start && dist <= kInfWindow && length <= 5u * kInfLanes; }
MVLDM_HD uint64_t inf_match_read(const InfShared& S, uint32_t start, uint32_t length, uint32_t dist, int lane) {
    uint64_t v = 0;
    if (!inf_match_ok(start, length, dist)) return v;
    for (uint32_t j = 0; j < 5; ++j) {
        const uint32_t k = (uint32_t)lane + j * kInfLanes;
        if (k < length) {
            const uint32_t r = k < dist ? k : k % dist;
            v |= (uint64_t)S.window[(start - dist + r) & (kInfWindow - 1)] << (8 * j);
        }
    }
    return v;
}
MVLDM_HD void inf_match_write(InfShared& S, uint8_t* out, uint32_t need, uint32_t start, uint32_t length, uint32_t dist, int lane, uint64_t v) {
    if (!inf_match_ok(start, length, dist)) return;
    for (uint32_t j = 0; j < 5; ++j) {
        const uint32_t k = (uint32_t)lane + j * kInfLanes;
        if (k < length) inf_put(S, out, need, start + k, (uint8_t)(v >> (8 * j)));
    }
}
// Adler-32 of out[0, n) as 64 interleaved sums: a = 1 + sum d_i, b = n + sum (n - i) d_i (mod 65521); and the filter bytes of the rows
MVLDM_HD void inf_sum_lane(InfShared& S, const uint8_t* out, uint32_t n, uint32_t need, uint32_t row, int lane) {
    uint64_t sa = 0, sb = 0;
    uint32_t wgt = (uint32_t)lane < n ? (n - (uint32_t)lane) % kAdlerMod : 0u;     // (n - i) mod 65521 at i = lane
    for (uint32_t i = (uint32_t)lane; i < n; i += kInfLanes) {
        const uint32_t d = out[i];
        sa += d;
        sb += wgt * d;
        wgt = wgt >= (uint32_t)kInfLanes ? wgt - kInfLanes : wgt + kAdlerMod - kInfLanes;
    }
    uint32_t bad = 0;
    if (n == need)
        for (uint32_t p = (uint32_t)lane * row; p < need; p += kInfLanes * row) bad |= out[p] > 4 ? 1u : 0u;
    S.q_val[lane] = (uint32_t)(sa % kAdlerMod);
    S.q_pos[lane] = (uint32_t)(sb % kAdlerMod);
    S.q_flag[lane] = bad;
}
// one lane: the verdict
MVLDM_HD int inf_verdict(const InfShared& S, uint32_t n, uint32_t need) {
    uint64_t a = 1, b = n % kAdlerMod;
    uint32_t bad = 0;
#pragma unroll 1
    for (int l = 0; l < kInfLanes; ++l) {
        a += S.q_val[l];
        b += S.q_pos[l];
        bad |= S.q_flag[l];
    }
    const uint32_t adler = ((uint32_t)(b % kAdlerMod) << 16) | (uint32_t)(a % kAdlerMod);
    if (adler != S.adler) return MVLDM_PNG_INFLATE;
    if (n != need) return MVLDM_PNG_LENGTH;
    return bad ? MVLDM_PNG_FILTER : MVLDM_PNG_OK;
}

}  // namespace mvldm
