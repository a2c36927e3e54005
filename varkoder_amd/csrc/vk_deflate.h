// vk_deflate.h -- BGZF compressor: the texts of clean_reads/ and split_fastqs/ become .fq.gz files where they lie in HBM.
//
// A text is cut into members of at most kDfMemberText bytes (0xff00, bgzip's figure: a member whose block is STORED,
// 18 + 5 + 65280 + 8 bytes, still fits the 65,536 that BSIZE can state).  One workgroup of 256 lanes compresses one
// member, everything in LDS:
//   1. the text is staged, and its CRC-32 taken: every lane runs the byte table over its 1/256 of the text, and a tree
//      of eight levels joins the pieces with a polynomial product (x^(8 C s) mod P, squared from level to level);
//      no combine matrices.
//   2. LZ77 in rounds of 256 consecutive positions, one per lane.  A lane hashes its 4 bytes into a table of earlier
//      positions (the table holds what the rounds BEFORE put there: a lookup never sees a position of its own round, so
//      what it finds does not depend on the order lanes run in), measures the match there and the match at distance 1,
//      and keeps the longer.  The round's candidates are resolved into tokens greedily from where the last token ended,
//      by pointer jumping: next[j] = j + length, eight doublings mark every position the chain from the carry reaches.
//      Tokens go to a byte stream (literal: the byte; match: length - 3, distance - 1 in three bytes) with one bit per
//      stream byte that marks a match's first byte.
//   3. histogram of the tokens, two Huffman codes limited to 15 bits (minimum-redundancy lengths in place, then the
//      Kraft sum repaired from the longest codes), and ONE dynamic block.  Before step 2 the block of the LITERALS ALONE
//      is priced the same way (greedy matches can cost more than the bytes they stand for): the member is the cheaper
//      of the two dynamic blocks, or a stored block when neither is smaller than the text.
//      The code-length alphabet is fixed (length 0: one bit, lengths 1..15: five bits, no run-length symbols).
//   4. a prefix sum of the tokens' bit lengths, every lane ORs its tokens' bits into the output (which takes the text's
//      place in LDS), and the member -- header with the BC field, block, CRC-32, ISIZE -- is copied to its slot.
// Then vk_cl_scan_* runs over the members' sizes and vk_df_gather_kernel packs every file's members and bgzip's empty
// EOF member contiguously, every file at a multiple of 16 bytes.
//
// Steps 2 to 4 up to the block's last bit are df_block, which takes the bit offset at which the block starts and
// BFINAL: the member (df_member) is staging, CRC-32 and the gzip/BGZF header and trailer around it, and vk_png.h frames
// the same block as a piece of a PNG's zlib stream.
//
// The member compressor is written in PHASES: DF_LANES(t) ... DF_END is "every lane t runs this, then all wait".  No
// value lives in a register across a phase: what one phase hands to the next lies in DfLds.  For the GPU a phase is
// the lane's own code and a barrier; for the host (tests/emul/deflate_emul.cpp) it is a loop over the lanes, one after
// another, so the CPU suite runs this very arithmetic with zlib as the judge.
#ifndef VK_DEFLATE_H
#define VK_DEFLATE_H

#include <stdint.h>

#include "vk_lane.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define DF_LANES(t) { const uint32_t t = threadIdx.x;
#define DF_END } __syncthreads();
#define DF_FN __device__ __forceinline__
#elif defined(__HIPCC__)
#define DF_LANES(t) for (uint32_t t = 0; t < kDfThreads; ++t) {
#define DF_END }
#define DF_FN __device__ __forceinline__
#else
#define DF_LANES(t) for (uint32_t t = 0; t < kDfThreads; ++t) {
#define DF_END }
#define DF_FN inline
#endif

constexpr uint32_t kDfThreads = 256;
constexpr uint32_t kDfMemberText = 65280;          // text bytes of a member at most
constexpr uint32_t kDfSlot = 65536;                // a member's slot in the workspace
constexpr uint32_t kDfHeader = 18, kDfTrailer = 8; // gzip header with the BC extra field; CRC-32 and ISIZE
constexpr uint32_t kDfEofBytes = 28;
constexpr uint32_t kDfTextWords = kDfMemberText / 4 + 16;
constexpr uint32_t kDfHashBits = 12;
constexpr uint32_t kDfMaxMatch = 258, kDfMinMatch = 3, kDfMaxDist = 32768, kDfFar = 4096;
constexpr uint32_t kDfLL = 286, kDfD = 30, kDfDBase = 288, kDfSyms = 320, kDfMaxBits = 15;
constexpr uint32_t kDfPreamble = 3 + 5 + 5 + 4 + 19 * 3;   // block header, HLIT, HDIST, HCLEN, the code-length code's lengths

struct DfMember {
    uint64_t off;   // of the member's text in the caller's buffer
    uint32_t len;
    uint32_t file;
};

struct DfFile {
    uint64_t m0;    // first member
    uint64_t nmem;
};

// uniform values of a member (DfLds::u)
enum { kDfCarry0 = 0, kDfCarry1, kDfSlen0, kDfSlen1, kDfCrc, kDfFixed = 7, kDfRes = 8, kDfU = 20 };   // kDfRes: three result slots of df_codes

struct DfLds {
    uint32_t text[kDfTextWords];          // the member's text (zero behind its end); later the member as it is written
    uint8_t stream[kDfMemberText + 16];   // the tokens
    uint32_t mbits[kDfMemberText / 32 + 1];  // bit o: stream byte o is a match's first byte
    uint32_t head[1u << kDfHashBits];     // hash -> position + 1 of its latest occurrence in an earlier round (0: none); first the CRC table
    uint32_t freq[kDfSyms];               // literal/length symbols at 0, distance symbols at kDfDBase
    uint32_t sorted[kDfSyms];             // (frequency << 9 | symbol), ascending, per alphabet; before and after the codes are built: a scan's values
    uint32_t work[kDfSyms];               // the code builders' lengths; the scan's other buffer
    uint16_t code[kDfSyms];               // bit-reversed
    uint8_t clen[kDfSyms];
    uint16_t rlen[kDfThreads], rdist[kDfThreads];   // the round's candidates
    uint16_t jump[2][kDfThreads];
    uint8_t mark[kDfThreads];
    uint32_t rm[8], rmm[8];               // the round's token starts / match starts as bit masks
    uint32_t hc[2][32];                   // per alphabet: codes of each length, the next code of each length
    uint32_t u[kDfU];
};
static_assert(sizeof(DfLds) <= 160 * 1024, "one member's state fits the CU's LDS");

DF_FN void df_or(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(p, v);
#else
    *p |= v;
#endif
}
DF_FN void df_max(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax(p, v);
#else
    if (*p < v) *p = v;
#endif
}
DF_FN void df_add(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}
DF_FN uint32_t df_log2(uint32_t x) {   // x > 0
#if defined(__HIP_DEVICE_COMPILE__)
    return 31u - static_cast<uint32_t>(__clz(static_cast<int>(x)));
#else
    return 31u - static_cast<uint32_t>(__builtin_clz(x));
#endif
}

// ---- CRC-32 (reflected, polynomial 0xEDB88320) as polynomials over GF(2): bit 31 is x^0 ---------------------
constexpr uint32_t kDfPoly = 0xEDB88320u;

DF_FN uint32_t df_mulmod(uint32_t a, uint32_t b) {   // a(x) b(x) mod P
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kDfPoly : b >> 1;
    }
    return p;
}

DF_FN uint32_t df_xpow8(uint32_t bytes) {   // x^(8 bytes) mod P
    uint32_t r = 0x80000000u, sq = 0x00800000u;   // 1, x^8
    for (; bytes; bytes >>= 1) {
        if (bytes & 1u) r = df_mulmod(r, sq);
        sq = df_mulmod(sq, sq);
    }
    return r;
}

// ---- symbols ----------------------------------------------------------------------------------------------
DF_FN void df_len_symbol(uint32_t len, uint32_t& sym, uint32_t& eb, uint32_t& extra) {   // len 3..258
    const uint32_t l = len - 3u;
    if (l < 8u) { sym = 257u + l; eb = 0; extra = 0; return; }
    if (len == kDfMaxMatch) { sym = 285u; eb = 0; extra = 0; return; }
    eb = df_log2(l) - 2u;
    sym = 261u + 4u * eb + ((l >> eb) & 3u);
    extra = l & ((1u << eb) - 1u);
}
DF_FN void df_dist_symbol(uint32_t d, uint32_t& sym, uint32_t& eb, uint32_t& extra) {   // d = distance - 1, 0..32767
    if (d < 4u) { sym = d; eb = 0; extra = 0; return; }
    const uint32_t msb = df_log2(d);
    eb = msb - 1u;
    sym = 2u * msb + ((d >> eb) & 1u);
    extra = d & ((1u << eb) - 1u);
}
DF_FN uint32_t df_ll_extra_bits(uint32_t sym) { return sym < 265u || sym == 285u ? 0u : (sym - 261u) >> 2; }
DF_FN uint32_t df_d_extra_bits(uint32_t sym) { return sym < 4u ? 0u : (sym >> 1) - 1u; }

DF_FN uint32_t df_load4(const uint32_t* text, uint32_t i) {   // bytes i .. i+3, little endian
    return vkl::alignbit(text[(i >> 2) + 1u], text[i >> 2], (i & 3u) * 8u);
}
DF_FN uint32_t df_hash(uint32_t v) { return (v * 0x9E3779B1u) >> (32u - kDfHashBits); }

DF_FN uint32_t df_match_len(const uint32_t* text, uint32_t p, uint32_t q, uint32_t maxlen) {
    uint32_t k = 0;
    for (; k < maxlen; k += 4u) {
        const uint32_t x = df_load4(text, p + k) ^ df_load4(text, q + k);
        if (x) { k += vkl::ffbl(x) >> 3; break; }
    }
    return k < maxlen ? k : maxlen;
}

DF_FN uint32_t df_mbit(const uint32_t* mbits, uint32_t o) { return (mbits[o >> 5] >> (o & 31u)) & 1u; }
// stream byte o: 0 literal, 1 a match's first byte, 2 inside a match token
DF_FN uint32_t df_kind(const uint32_t* mbits, uint32_t o) {
    if (df_mbit(mbits, o)) return 1u;
    if ((o >= 1u && df_mbit(mbits, o - 1u)) || (o >= 2u && df_mbit(mbits, o - 2u))) return 2u;
    return 0u;
}

DF_FN void df_put(uint32_t* out, uint32_t bitpos, uint64_t v, uint32_t nbits) {   // nbits <= 48, v below 2^nbits
    const uint32_t w = bitpos >> 5, sh = bitpos & 31u;
    df_or(out + w, static_cast<uint32_t>(v << sh));
    if (sh + nbits > 32u) df_or(out + w + 1u, static_cast<uint32_t>(v >> (32u - sh)));
    if (sh + nbits > 64u) df_or(out + w + 2u, static_cast<uint32_t>(v >> (64u - sh)));
}

// the first 16 bytes of a member: 1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, 'B' 'C' 2 0 (BSIZE follows)
DF_FN uint32_t df_head_word(uint32_t i) { return i == 0u ? 0x04088b1fu : i == 1u ? 0u : i == 2u ? 0x0006ff00u : 0x00024342u; }
// bgzip's empty last member, 28 bytes as 7 words
DF_FN uint32_t df_eof_word(uint32_t i) { return i < 4u ? df_head_word(i) : i == 4u ? 0x0003001bu : 0u; }

DF_FN uint32_t df_rev(uint32_t code, uint32_t len) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1u - i);
    return r;
}

// DEFLATE's fixed literal/length code (RFC 1951, 3.2.6); the fixed distance code is the symbol in 5 bits
DF_FN uint32_t df_fixed_len(uint32_t s) { return s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : 8u; }
DF_FN uint32_t df_fixed_code(uint32_t s) { return s < 144u ? 0x30u + s : s < 256u ? 0x190u + (s - 144u) : s < 280u ? s - 256u : 0xC0u + (s - 280u); }

// One alphabet's code, by one lane: S.sorted[base .. base+nsym) ascending -> S.clen / S.code[base ..).  An alphabet
// with fewer than two used symbols gets two codes of one bit (a complete code, whatever reads it).
DF_FN void df_build_code(DfLds& S, uint32_t base, uint32_t nsym) {
    uint32_t* A = S.work + base;
    uint32_t* cnt = S.hc[base ? 1 : 0];
    uint32_t* nextc = cnt + 16;
    const uint32_t* K = S.sorted + base;
    uint32_t first = 0;
    while (first < nsym && (K[first] >> 9) == 0u) ++first;
    const uint32_t n = nsym - first;
    for (uint32_t i = 0; i < nsym; ++i) S.clen[base + i] = 0;
    if (n < 2u) {
        const uint32_t s = n ? (K[first] & 511u) : 0u;
        S.clen[base + s] = 1;
        S.clen[base + (s ? 0u : 1u)] = 1;
    } else {
        // minimum-redundancy code lengths in place (Moffat and Katajainen 1995)
        for (uint32_t i = 0; i < n; ++i) A[i] = K[first + i] >> 9;
        A[0] += A[1];
        uint32_t root = 0, leaf = 2;
        for (uint32_t next = 1; next + 1u < n; ++next) {
            if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = next; } else A[next] = A[leaf++];
            if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = next; } else A[next] += A[leaf++];
        }
        A[n - 2u] = 0;
        for (uint32_t next = n - 2u; next-- > 0u;) A[next] = A[A[next]] + 1u;
        int32_t avbl = 1, used = 0, dpth = 0, rt = static_cast<int32_t>(n) - 2, nx = static_cast<int32_t>(n) - 1;
        while (avbl > 0) {
            while (rt >= 0 && static_cast<int32_t>(A[rt]) == dpth) { ++used; --rt; }
            while (avbl > used) { A[nx--] = static_cast<uint32_t>(dpth); --avbl; }
            avbl = 2 * used; ++dpth; used = 0;
        }
        // A[i]: the length of the i-th rarest symbol.  Limit to 15 bits: fold the longer ones, then repair the Kraft sum.
        for (uint32_t l = 0; l <= kDfMaxBits; ++l) cnt[l] = 0;
        for (uint32_t i = 0; i < n; ++i) ++cnt[A[i] < kDfMaxBits ? A[i] : kDfMaxBits];
        uint32_t total = 0;
        for (uint32_t l = 1; l <= kDfMaxBits; ++l) total += cnt[l] << (kDfMaxBits - l);
        while (total > (1u << kDfMaxBits)) {
            --cnt[kDfMaxBits];
            for (uint32_t l = kDfMaxBits - 1u; l > 0u; --l)
                if (cnt[l]) { --cnt[l]; cnt[l + 1u] += 2u; break; }
            --total;
        }
        uint32_t i = 0;
        for (uint32_t l = kDfMaxBits; l > 0u; --l)
            for (uint32_t c = cnt[l]; c > 0u; --c) S.clen[base + (K[first + i++] & 511u)] = static_cast<uint8_t>(l);
    }
    // canonical codes
    for (uint32_t l = 0; l <= kDfMaxBits; ++l) cnt[l] = 0;
    for (uint32_t i = 0; i < nsym; ++i) ++cnt[S.clen[base + i]];
    cnt[0] = 0;
    uint32_t c = 0;
    for (uint32_t l = 1; l <= kDfMaxBits; ++l) { c = (c + cnt[l - 1u]) << 1; nextc[l] = c; }
    for (uint32_t i = 0; i < nsym; ++i) {
        const uint32_t l = S.clen[base + i];
        S.code[base + i] = l ? static_cast<uint16_t>(df_rev(nextc[l]++, l)) : 0;
    }
}

// A token's bits: the value and how many.
DF_FN uint32_t df_token_bits(const DfLds& S, uint32_t o, uint32_t kind, uint64_t& v) {
    if (kind == 0u) {
        const uint32_t b = S.stream[o];
        v = S.code[b];
        return S.clen[b];
    }
    const uint32_t len = S.stream[o] + 3u, d = S.stream[o + 1u] | (static_cast<uint32_t>(S.stream[o + 2u]) << 8);
    uint32_t ls, leb, lx, ds, deb, dx;
    df_len_symbol(len, ls, leb, lx);
    df_dist_symbol(d, ds, deb, dx);
    uint32_t nb = S.clen[ls];
    v = S.code[ls];
    v |= static_cast<uint64_t>(lx) << nb; nb += leb;
    v |= static_cast<uint64_t>(S.code[kDfDBase + ds]) << nb; nb += S.clen[kDfDBase + ds];
    v |= static_cast<uint64_t>(dx) << nb; nb += deb;
    return nb;
}

// The codes of a token stream of slen bytes and what they cost, into the result slots `which` of S.u (bits of the tokens
// and the end of block, the lengths table's bits beyond one per symbol sent, HLIT + 257, HDIST + 1).  A call has slots
// of its own: what uniform code has read is never written again.
DF_FN void df_codes(DfLds& S, uint32_t slen, uint32_t which) {
    const uint32_t SC = (slen + kDfThreads - 1u) / kDfThreads;
    DF_LANES(t)
        for (uint32_t i = t; i < kDfSyms; i += kDfThreads) S.freq[i] = 0;
    DF_END
    // -- histogram
    DF_LANES(t)
        const uint32_t o1 = (t + 1u) * SC < slen ? (t + 1u) * SC : slen;
        for (uint32_t o = t * SC; o < o1; ++o) {
            const uint32_t kind = df_kind(S.mbits, o);
            if (kind == 0u) df_add(&S.freq[S.stream[o]], 1u);
            else if (kind == 1u) {
                uint32_t sym, eb, ex;
                df_len_symbol(S.stream[o] + 3u, sym, eb, ex);
                df_add(&S.freq[sym], 1u);
                df_dist_symbol(S.stream[o + 1u] | (static_cast<uint32_t>(S.stream[o + 2u]) << 8), sym, eb, ex);
                df_add(&S.freq[kDfDBase + sym], 1u);
            }
        }
        if (t == 0u) df_add(&S.freq[256], 1u);   // end of block
    DF_END
    // -- the two codes: rank the symbols by (frequency, symbol), then one lane each builds its alphabet's lengths
    DF_LANES(t)
        for (uint32_t i = t; i < kDfSyms; i += kDfThreads) {
            const uint32_t b = i < kDfDBase ? 0u : kDfDBase, ns = i < kDfDBase ? kDfLL : kDfD;
            if (i - b >= ns) continue;
            const uint32_t key = (S.freq[i] << 9) | (i - b);
            uint32_t rank = 0;
            for (uint32_t j = 0; j < ns; ++j) rank += ((S.freq[b + j] << 9) | j) < key;
            S.sorted[b + rank] = key;
        }
    DF_END
    DF_LANES(t)
        if (t == 0u) df_build_code(S, 0u, kDfLL);
        if (t == 64u) df_build_code(S, kDfDBase, kDfD);
    DF_END
    // -- sizes: the lengths table, the tokens
    DF_LANES(t)
        uint32_t bits = 0, tab = 0, hl = 0, hd = 0;
        for (uint32_t i = t; i < kDfSyms; i += kDfThreads) {
            const bool ll = i < kDfDBase;
            const uint32_t s = ll ? i : i - kDfDBase;
            if (s >= (ll ? kDfLL : kDfD) || !S.clen[i]) continue;
            bits += S.freq[i] * (S.clen[i] + (ll ? df_ll_extra_bits(s) : df_d_extra_bits(s)));
            tab += 4u;   // a length that is not 0 takes 5 bits, 0 takes 1: 1 per symbol sent is added below
            if (ll) hl = s + 1u; else hd = s + 1u;
        }
        if (bits) df_add(&S.u[kDfRes + 4u * which], bits);
        if (tab) df_add(&S.u[kDfRes + 4u * which + 1u], tab);
        if (hl) df_max(&S.u[kDfRes + 4u * which + 2u], hl);
        if (hd) df_max(&S.u[kDfRes + 4u * which + 3u], hd);
    DF_END
}

DF_FN uint32_t df_code_bits(const DfLds& S, uint32_t which) {   // of the dynamic block
    return kDfPreamble + S.u[kDfRes + 4u * which + 1u] + S.u[kDfRes + 4u * which + 2u] + S.u[kDfRes + 4u * which + 3u] +
           S.u[kDfRes + 4u * which];
}

// the stream that says the text byte by byte
DF_FN void df_all_literals(DfLds& S, uint32_t n) {
    DF_LANES(t)
        const uint8_t* tb = reinterpret_cast<const uint8_t*>(S.text);
        for (uint32_t i = t; i < n; i += kDfThreads) S.stream[i] = tb[i];
        for (uint32_t i = t; i < kDfMemberText / 32u + 1u; i += kDfThreads) S.mbits[i] = 0;
    DF_END
}

// The CRC-32 register after bytes [0, m) of S.text, started from `init`, into S.sorted[0] (not inverted); the byte table
// lies in S.head[0 .. 256).  Lane t takes bytes [t C - pad, (t + 1) C - pad): zero bytes in front of a register that
// is 0 change nothing, and the register of the lane that holds byte 0 starts at `init`.
DF_FN void df_crc_lanes(DfLds& S, uint32_t m, uint32_t init) {
    uint32_t* const scan0 = S.sorted;
    const uint32_t C = (m + kDfThreads - 1u) / kDfThreads, pad = kDfThreads * C - m;
    DF_LANES(t)
        const uint8_t* tb = reinterpret_cast<const uint8_t*>(S.text);
        uint32_t c = 0;
        for (uint32_t v = t * C; v < (t + 1u) * C; ++v) {
            if (v < pad) continue;
            if (v == pad) c = init;
            c = S.head[(c ^ tb[v - pad]) & 0xFFu] ^ (c >> 8);
        }
        scan0[t] = c;
    DF_END
    {
        uint32_t f = df_xpow8(C);   // what moves a register over the s C bytes of the right-hand piece
        for (uint32_t s = 1; s < kDfThreads; s <<= 1) {
            DF_LANES(t)
                if ((t & (2u * s - 1u)) == 0u) scan0[t] = df_mulmod(f, scan0[t]) ^ scan0[t + s];
            DF_END
            f = df_mulmod(f, f);
        }
    }
}

// One DEFLATE block of the text staged in S.text[0 .. n) (zero behind its end), 1 <= n <= kDfMemberText, with S.head and
// S.u's carries, stream lengths and result slots zero.  The block is the cheaper of the tokens' and the literals'
// dynamic blocks; its bits are ORed into S.text (which they replace) from bit `bit0` on, with `bfinal` in its first
// bit, everything else zero up to `tail` bytes behind the block's last byte: the caller's framing goes there and in
// front of bit0.  Returns the bit behind the block's last one -- or 0 when no code pays: then S.text still holds the
// text and the caller writes it as a stored block.  (bit0 / 8 + tail <= 26: the output fits S.text.)
// fixed != 0: the chosen tokens are also priced with DEFLATE's fixed codes (BTYPE 1) and written with them where that
// is smaller -- a text of a few hundred bytes, where the lengths table is most of a dynamic block; S.u[kDfFixed] zero.
// above != 0: a third candidate beside the hash table's and distance 1, the position `above` bytes back (an image's
// row above; the table only knows earlier rounds, and a small image's first round is half of it).
// The BGZF members ask for neither: their bytes are recorded.
DF_FN uint32_t df_block(DfLds& S, uint32_t n, uint32_t bit0, uint32_t bfinal, uint32_t tail, uint32_t fixed, uint32_t above) {
    uint32_t* const scan0 = S.sorted;
    uint32_t* const scan1 = S.work;
    // -- what the literals alone would cost (greedy matches can cost more than the bytes they stand for)
    df_all_literals(S, n);
    df_codes(S, n, 0u);
    const uint32_t litbits = df_code_bits(S, 0u);
    // -- LZ77, 256 positions a round
    const uint32_t rounds = (n + kDfThreads - 1u) / kDfThreads;
    for (uint32_t r = 0; r < rounds; ++r) {
        const uint32_t base = r * kDfThreads, par = r & 1u;
        DF_LANES(t)
            const uint32_t p = base + t;
            uint32_t len = 0, dist = 0;
            if (p < n) {
                const uint32_t maxlen = n - p < kDfMaxMatch ? n - p : kDfMaxMatch;
                if (maxlen >= kDfMinMatch) {
                    const uint32_t cand = S.head[df_hash(df_load4(S.text, p))];
                    if (cand && p - (cand - 1u) <= kDfMaxDist) {
                        len = df_match_len(S.text, p, cand - 1u, maxlen);
                        dist = p - (cand - 1u);
                    }
                    if (p >= 1u && dist != 1u) {
                        const uint32_t l1 = df_match_len(S.text, p, p - 1u, maxlen);
                        if (l1 >= len) { len = l1; dist = 1u; }
                    }
                    if (above && p >= above && dist != above) {   // (the text itself: the same whatever order lanes run in)
                        const uint32_t l2 = df_match_len(S.text, p, p - above, maxlen);
                        if (l2 > len) { len = l2; dist = above; }
                    }
                    if (len < kDfMinMatch || (len == kDfMinMatch && dist > kDfFar)) len = 0;
                }
            }
            S.rlen[t] = static_cast<uint16_t>(len);
            S.rdist[t] = static_cast<uint16_t>(dist - 1u);
            const uint32_t nx = p < n ? t + (len ? len : 1u) : kDfThreads;
            S.jump[0][t] = static_cast<uint16_t>(nx < kDfThreads ? nx : kDfThreads);
            S.mark[t] = p < n && t == S.u[kDfCarry0 + par];
            if (t < 8u) S.rm[t] = S.rmm[t] = 0;
        DF_END
        for (uint32_t k = 0; k < 8u; ++k) {   // after doubling k every position within 2^k tokens of the carry is marked
            DF_LANES(t)
                const uint32_t j = S.jump[k & 1u][t];
                if (j < kDfThreads) {
                    if (S.mark[t]) S.mark[j] = 1;
                    S.jump[(k & 1u) ^ 1u][t] = S.jump[k & 1u][j];
                } else {
                    S.jump[(k & 1u) ^ 1u][t] = static_cast<uint16_t>(kDfThreads);
                }
            DF_END
        }
        DF_LANES(t)
            const uint32_t p = base + t;
            if (S.mark[t] && p < n) {   // (the chain also marks the position behind the text's last token)
                df_or(&S.rm[t >> 5], 1u << (t & 31u));
                if (S.rlen[t]) df_or(&S.rmm[t >> 5], 1u << (t & 31u));
            }
            if (p < n) df_max(&S.head[df_hash(df_load4(S.text, p))], p + 1u);   // seen from the next round on
        DF_END
        DF_LANES(t)
            const uint32_t slen = S.u[kDfSlen0 + par];
            if (S.mark[t] && base + t < n) {
                uint32_t o = slen;
                for (uint32_t w = 0; w < (t >> 5); ++w) o += vkl::popc(S.rm[w]) + 2u * vkl::popc(S.rmm[w]);
                const uint32_t below = (1u << (t & 31u)) - 1u;
                o += vkl::popc(S.rm[t >> 5] & below) + 2u * vkl::popc(S.rmm[t >> 5] & below);
                const uint32_t len = S.rlen[t];
                if (len) {
                    S.stream[o] = static_cast<uint8_t>(len - 3u);
                    S.stream[o + 1u] = static_cast<uint8_t>(S.rdist[t] & 0xFFu);
                    S.stream[o + 2u] = static_cast<uint8_t>(S.rdist[t] >> 8);
                    df_or(&S.mbits[o >> 5], 1u << (o & 31u));
                } else {
                    S.stream[o] = reinterpret_cast<const uint8_t*>(S.text)[base + t];
                }
                const uint32_t end = t + (len ? len : 1u);
                if (end >= kDfThreads || base + end >= n) {   // the round's last token
                    S.u[kDfCarry0 + (par ^ 1u)] = end >= kDfThreads ? end - kDfThreads : 0u;
                    S.u[kDfSlen0 + (par ^ 1u)] = o + (len ? 3u : 1u);
                }
            } else if (t == 0u && !(S.rm[0] | S.rm[1] | S.rm[2] | S.rm[3] | S.rm[4] | S.rm[5] | S.rm[6] | S.rm[7])) {
                // a match of an earlier round covers this one
                S.u[kDfCarry0 + (par ^ 1u)] = S.u[kDfCarry0 + par] - kDfThreads;
                S.u[kDfSlen0 + (par ^ 1u)] = slen;
            }
        DF_END
    }
    const uint32_t mslen = S.u[kDfSlen0 + (rounds & 1u)];
    df_codes(S, mslen, 1u);
    // -- the block: the tokens, the literals alone when the matches do not pay, the text as it is when no code pays
    const uint32_t use = df_code_bits(S, 1u) < litbits ? 1u : 0u;   // the result slots that hold: 1 the tokens', 0 the literals'
    if (use == 0u && (litbits + 7u) / 8u < n + 5u) {   // the literals' codes again (slot 2 takes the same figures)
        df_all_literals(S, n);
        df_codes(S, n, 2u);
    }
    const uint32_t slen = use == 1u ? mslen : n;
    const uint32_t SC = (slen + kDfThreads - 1u) / kDfThreads;   // stream bytes a lane walks
    const uint32_t hlit = S.u[kDfRes + 4u * use + 2u], hdist = S.u[kDfRes + 4u * use + 3u];
    // S.freq and the codes are the chosen stream's, unless the literals were chosen and not coded again (stored follows)
    const bool coded = use == 1u || (litbits + 7u) / 8u < n + 5u;
    if (fixed && coded) {
        DF_LANES(t)
            uint32_t bits = 0;
            for (uint32_t i = t; i < kDfSyms; i += kDfThreads) {
                const bool ll = i < kDfDBase;
                const uint32_t s = ll ? i : i - kDfDBase;
                if (s < (ll ? kDfLL : kDfD)) bits += S.freq[i] * (ll ? df_fixed_len(s) + df_ll_extra_bits(s) : 5u + df_d_extra_bits(s));
            }
            if (bits) df_add(&S.u[kDfFixed], bits);
        DF_END
    }
    const bool fix = fixed && coded && 3u + S.u[kDfFixed] < df_code_bits(S, use);
    if (fix) {
        DF_LANES(t)
            for (uint32_t i = t; i < kDfSyms; i += kDfThreads) {
                const bool ll = i < kDfDBase;
                const uint32_t s = ll ? i : i - kDfDBase;
                S.clen[i] = static_cast<uint8_t>(ll ? df_fixed_len(s) : 5u);
                S.code[i] = static_cast<uint16_t>(ll ? df_rev(df_fixed_code(s), df_fixed_len(s)) : df_rev(s, 5u));
            }
        DF_END
    }
    const uint32_t tabbits = fix ? 0u : S.u[kDfRes + 4u * use + 1u] + hlit + hdist;
    const uint32_t preamble = fix ? 3u : kDfPreamble;
    const uint32_t dynbits = fix ? 3u + S.u[kDfFixed] : df_code_bits(S, use);
    const uint32_t dynbytes = (dynbits + 7u) / 8u;
    if (dynbytes >= n + 5u) return 0u;   // a stored block is no larger
    // -- dynamic block: every lane's first bit, then the bits
    const uint32_t owords = (bit0 / 8u + dynbytes + tail + 3u) / 4u;
    DF_LANES(t)
        const uint32_t o1 = (t + 1u) * SC < slen ? (t + 1u) * SC : slen;
        uint32_t bits = 0;
        for (uint32_t o = t * SC; o < o1; ++o) {
            const uint32_t kind = df_kind(S.mbits, o);
            uint64_t v;
            if (kind != 2u) bits += df_token_bits(S, o, kind, v);
        }
        scan0[t] = bits;
        for (uint32_t i = t; i < owords + 2u; i += kDfThreads) S.text[i] = 0;   // (dynbytes < n + 5: owords + 2 <= kDfTextWords)
    DF_END
    for (uint32_t k = 0; k < 8u; ++k) {   // inclusive scan, doubling
        DF_LANES(t)
            const uint32_t d = 1u << k;
            (k & 1u ? scan0 : scan1)[t] = (k & 1u ? scan1 : scan0)[t] + (t >= d ? (k & 1u ? scan1 : scan0)[t - d] : 0u);
        DF_END
    }
    const uint32_t tok0 = bit0 + preamble + tabbits;   // of the first token
    DF_LANES(t)
        uint32_t* out = S.text;
        const uint32_t o1 = (t + 1u) * SC < slen ? (t + 1u) * SC : slen;
        uint32_t at = tok0 + (t ? scan0[t - 1u] : 0u);
        for (uint32_t o = t * SC; o < o1; ++o) {
            const uint32_t kind = df_kind(S.mbits, o);
            if (kind == 2u) continue;
            uint64_t v;
            const uint32_t nb = df_token_bits(S, o, kind, v);
            df_put(out, at, v, nb);
            at += nb;
        }
        if (t == kDfThreads - 1u) {   // block preamble, the lengths, end of block
            uint32_t b = bit0;
            df_put(out, b, bfinal | ((fix ? 1u : 2u) << 1), 3u); b += 3u;      // BFINAL, BTYPE 2 (1: the fixed codes, no table)
            if (!fix) {
                df_put(out, b, hlit - 257u, 5u); b += 5u;
                df_put(out, b, hdist - 1u, 5u); b += 5u;
                df_put(out, b, 15u, 4u); b += 4u;                     // all 19 lengths of the code-length code
                // in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15: symbol 0 one bit, 1..16 five bits, 17 and 18 unused
                for (uint32_t i = 0; i < 19u; ++i) { df_put(out, b, i == 3u ? 1u : (i == 1u || i == 2u ? 0u : 5u), 3u); b += 3u; }
                for (uint32_t i = 0; i < hlit + hdist; ++i) {
                    const uint32_t l = S.clen[i < hlit ? i : kDfDBase + (i - hlit)];
                    if (l) { df_put(out, b, df_rev(15u + l, 5u), 5u); b += 5u; } else b += 1u;   // (code 0, one bit)
                }
            }
            df_put(out, at, S.code[256], S.clen[256]);
        }
    DF_END
    return bit0 + dynbits;
}

// One member: text[0 .. n) (global, at a multiple of 4 bytes), 1 <= n <= kDfMemberText -> slot[0 .. *size), *size <= 65,311.
DF_FN void df_member(DfLds& S, const uint8_t* text, uint32_t n, uint8_t* slot, uint64_t* size) {
    const uint32_t words = n >> 2;
    // -- stage the text; the CRC's byte table
    DF_LANES(t)
        const uint32_t* src = reinterpret_cast<const uint32_t*>(text);
        for (uint32_t i = t; i < kDfTextWords; i += kDfThreads) {
            uint32_t w = 0;
            if (i < words) w = src[i];
            else if (i == words)
                for (uint32_t b = 0; b < (n & 3u); ++b) w |= static_cast<uint32_t>(text[4u * i + b]) << (8u * b);
            S.text[i] = w;
        }
        uint32_t c = t;
        for (uint32_t k = 0; k < 8u; ++k) c = (c & 1u) ? (c >> 1) ^ kDfPoly : c >> 1;
        S.head[t] = c;
        if (t < kDfU) S.u[t] = 0;
    DF_END
    df_crc_lanes(S, n, 0xFFFFFFFFu);
    DF_LANES(t)
        if (t == 0u) S.u[kDfCrc] = ~S.sorted[0];
        for (uint32_t i = t; i < (1u << kDfHashBits); i += kDfThreads) S.head[i] = 0;
    DF_END
    // -- the block, behind the header
    const uint32_t end = df_block(S, n, kDfHeader * 8u, 1u, kDfTrailer, 0u, 0u);
    const uint32_t crc = S.u[kDfCrc];
    if (end == 0u) {
        // -- stored block
        const uint32_t total = kDfHeader + 5u + n + kDfTrailer;
        DF_LANES(t)
            const uint8_t* tb = reinterpret_cast<const uint8_t*>(S.text);
            for (uint32_t i = t; i < n; i += kDfThreads) slot[kDfHeader + 5u + i] = tb[i];
            if (t == 0u) {
                for (uint32_t i = 0; i < 4u; ++i) reinterpret_cast<uint32_t*>(slot)[i] = df_head_word(i);
                slot[16] = static_cast<uint8_t>((total - 1u) & 0xFFu);
                slot[17] = static_cast<uint8_t>((total - 1u) >> 8);
                slot[18] = 1;   // BFINAL, BTYPE 0
                slot[19] = static_cast<uint8_t>(n & 0xFFu);
                slot[20] = static_cast<uint8_t>(n >> 8);
                slot[21] = static_cast<uint8_t>(~n & 0xFFu);
                slot[22] = static_cast<uint8_t>((~n >> 8) & 0xFFu);
                uint8_t* tr = slot + kDfHeader + 5u + n;
                for (uint32_t i = 0; i < 4u; ++i) {
                    tr[i] = static_cast<uint8_t>(crc >> (8u * i));
                    tr[4u + i] = static_cast<uint8_t>(n >> (8u * i));
                }
                *size = total;
            }
        DF_END
        return;
    }
    // -- dynamic block: the header and the trailer around it
    const uint32_t dynbytes = (end - kDfHeader * 8u + 7u) / 8u;
    const uint32_t total = kDfHeader + dynbytes + kDfTrailer, owords = (total + 3u) / 4u;
    DF_LANES(t)
        if (t == 0u) {
            uint32_t* out = S.text;
            for (uint32_t i = 0; i < 4u; ++i) df_put(out, 32u * i, df_head_word(i), 32u);
            df_put(out, 128u, total - 1u, 16u);
            const uint32_t tr = (kDfHeader + dynbytes) * 8u;
            df_put(out, tr, crc, 32u);
            df_put(out, tr + 32u, n, 32u);
            *size = total;
        }
    DF_END
    DF_LANES(t)
        uint32_t* dst = reinterpret_cast<uint32_t*>(slot);
        for (uint32_t i = t; i < owords; i += kDfThreads) dst[i] = S.text[i];
    DF_END
}

#if defined(__HIPCC__)

__global__ void __launch_bounds__(kDfThreads) vk_df_member_kernel(const uint8_t* __restrict__ text, const DfMember* __restrict__ mem,
                                                                  uint8_t* __restrict__ slots, uint64_t* __restrict__ sizes) {
    extern __shared__ uint32_t vk_df_lds[];
    DfLds& S = *reinterpret_cast<DfLds*>(vk_df_lds);
    const DfMember m = mem[blockIdx.x];
    df_member(S, text + m.off, m.len, slots + static_cast<uint64_t>(blockIdx.x) * kDfSlot, sizes + blockIdx.x);
}

// a file's bytes: its members and the EOF member; fsizes: rounded up to 16, what the scan lays the files out by
__global__ void __launch_bounds__(kDfThreads) vk_df_files_kernel(const DfFile* __restrict__ files, uint32_t nfiles,
                                                                 const uint64_t* __restrict__ mprefix, uint64_t* __restrict__ flens,
                                                                 uint64_t* __restrict__ fsizes) {
    const uint32_t f = blockIdx.x * kDfThreads + threadIdx.x;
    if (f >= nfiles) return;
    const uint64_t len = mprefix[files[f].m0 + files[f].nmem] - mprefix[files[f].m0] + kDfEofBytes;
    flens[f] = len;
    fsizes[f] = (len + 15u) / 16u * 16u;
}

// blocks [0, nmem): member b's slot to its place in its file; blocks [nmem, nmem + nfiles): a file's EOF member and the
// zero bytes up to its 16-byte rounded end
__global__ void __launch_bounds__(kDfThreads) vk_df_gather_kernel(const DfMember* __restrict__ mem, uint64_t nmem,
                                                                  const DfFile* __restrict__ files, const uint8_t* __restrict__ slots,
                                                                  const uint64_t* __restrict__ mprefix, const uint64_t* __restrict__ flens,
                                                                  const uint64_t* __restrict__ fprefix, uint8_t* __restrict__ out) {
    const uint64_t b = blockIdx.x;
    if (b >= nmem) {
        const uint64_t f = b - nmem;
        uint8_t* dst = out + fprefix[f] + flens[f] - kDfEofBytes;
        const uint32_t span = static_cast<uint32_t>(fprefix[f + 1] - fprefix[f] - flens[f]) + kDfEofBytes;
        if (threadIdx.x < span) dst[threadIdx.x] = threadIdx.x < kDfEofBytes ? static_cast<uint8_t>(df_eof_word(threadIdx.x >> 2) >> (8u * (threadIdx.x & 3u))) : 0;
        return;
    }
    const DfFile fl = files[mem[b].file];
    const uint32_t n = static_cast<uint32_t>(mprefix[b + 1] - mprefix[b]);
    uint8_t* dst = out + fprefix[mem[b].file] + (mprefix[b] - mprefix[fl.m0]);
    const uint8_t* src = slots + b * kDfSlot;
    // bytes up to the destination's first dword, whole dwords (the slot read as two aligned dwords each), the rest
    const uint32_t lead = static_cast<uint32_t>((4u - (reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u);
    const uint32_t h = lead < n ? lead : n, body = (n - h) / 4u;
    if (threadIdx.x < h) dst[threadIdx.x] = src[threadIdx.x];
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(src);
    uint32_t* dw = reinterpret_cast<uint32_t*>(dst + h);
    for (uint32_t i = threadIdx.x; i < body; i += kDfThreads) {
        const uint32_t at = h + 4u * i;
        dw[i] = vkl::alignbit(sw[(at >> 2) + 1u], sw[at >> 2], (at & 3u) * 8u);
    }
    const uint32_t done = h + 4u * body;
    if (threadIdx.x < n - done) dst[done + threadIdx.x] = src[done + threadIdx.x];
}

#endif  // __HIPCC__
#endif  // VK_DEFLATE_H
