// vk_png.h -- PNG encoder: the images of a batch become IDAT chunks where they lie in HBM.
//
// An image [side][side] of bytes has the raw stream of side rows of 1 + side bytes: the filter byte 0 ("None"), then the
// row's pixels.  The stream is cut into pieces of at most kDfMemberText bytes, and one workgroup of 256 lanes makes one
// piece's bytes with vk_deflate.h's block compressor, everything in LDS (a DfLds):
//   1. staging reads the image itself and puts the filter bytes in on the way: raw position r is row r / (side + 1),
//      column r % (side + 1) - 1.  No raw copy exists in HBM.
//   2. Adler-32 of the piece, from 1, 0 replaced by 0, 0 (the part that is linear in the bytes): every lane sums its
//      1/256 of the piece, a = sum of the bytes, b = sum of (bytes behind it in the piece + 1) * byte, joined with LDS adds.
//   3. df_block: the piece as ONE block (with the fixed codes where they are smaller: images of k = 5 and 6; with the
//      byte of the row above, side + 1 back, as a match candidate of every position).  The first piece starts behind the zlib header 78 01; a piece that is not the
//      image's last has BFINAL 0 and is brought to a byte boundary by an empty stored block (three zero bits, padding,
//      00 00 ff ff) unless it is a stored block itself; the last has BFINAL 1 and is padded to a byte.
//   4. CRC-32 of the piece's bytes from register 0 (again the linear part), by df_crc_lanes over the bytes in LDS.
// Then vk_cl_scan_* runs over the pieces' sizes, vk_png_image_kernel joins an image's pieces -- Adler-32 by the combine
// rule mod 65521, the chunk's CRC-32 from the register after "IDAT" carried over every piece by a polynomial product
// (x^(8 n) mod P) and then over the four Adler bytes -- a second scan lays the chunks out at multiples of 16, and
// vk_png_gather_kernel writes every chunk: length, "IDAT", the pieces, Adler-32, CRC-32.
//
// The file's rules are vk_deflate.h's: phases, nothing in a register across a phase but values that every lane reads
// from LDS alike, plain stores and LDS atomics.  tests/emul/png_emul.cpp runs png_piece and png_join on the host.
#ifndef VK_PNG_H
#define VK_PNG_H

#include "vk_deflate.h"

constexpr uint32_t kPngMaxSide = 512;
constexpr uint32_t kPngAdler = 65521;
constexpr uint32_t kPngFrame = 16;       // of a chunk: length, "IDAT" in front, Adler-32 and CRC-32 behind
constexpr uint32_t kPngPieceExtra = 9;   // a dynamic block has at most n + 4 bytes, the empty stored block behind it at most 5
constexpr uint32_t kPngZlibHeader = 0x0178;   // 78 01: deflate, 32 KiB window, no dictionary, fastest

enum { kPngA = 5, kPngB = 6 };   // DfLds::u: the piece's Adler sums (slots that df_block leaves alone)
static_assert(static_cast<uint32_t>(kPngB) < static_cast<uint32_t>(kDfFixed), "the Adler sums and the fixed price share DfLds::u");

// what a piece hands to the join
struct PngPiece {
    uint32_t crc;    // the CRC-32 register after the piece's bytes, from register 0
    uint32_t a, b;   // Adler-32 of the piece's raw bytes from (0, 0), each below 65521
    uint32_t raw;    // raw bytes
};

constexpr uint32_t png_raw(uint32_t side) { return side * (side + 1u); }
constexpr uint32_t png_pieces(uint32_t side) { return (png_raw(side) + kDfMemberText - 1u) / kDfMemberText; }
constexpr uint32_t png_piece_len(uint32_t side, uint32_t piece) {
    return png_raw(side) - piece * kDfMemberText < kDfMemberText ? png_raw(side) - piece * kDfMemberText : kDfMemberText;
}
// bytes of a piece at most: the zlib header in front of the first, the text, a stored block's 5 or kPngPieceExtra
constexpr uint32_t png_piece_bound(uint32_t n, bool first) { return n + kPngPieceExtra + (first ? 2u : 0u); }
// a piece's workspace slot: the first piece's bound (no piece is longer), rounded up to 16
constexpr uint32_t png_slot(uint32_t side) { return (png_piece_bound(png_piece_len(side, 0u), true) + 15u) / 16u * 16u; }
// bytes of an image's chunk at most, rounded up to 16
constexpr uint64_t png_chunk_bound(uint32_t side) {
    return (kPngFrame + 2u + png_raw(side) + static_cast<uint64_t>(kPngPieceExtra) * png_pieces(side) + 15u) / 16u * 16u;
}

DF_FN uint32_t png_crc_byte(uint32_t reg, uint32_t byte) {
    reg ^= byte;
    for (uint32_t k = 0; k < 8u; ++k) reg = (reg & 1u) ? (reg >> 1) ^ kDfPoly : reg >> 1;
    return reg;
}

// Piece `piece` of image img[side][side] -> slot[0 .. *size), *size <= png_piece_bound, and the piece's sums.
DF_FN void png_piece(DfLds& S, const uint8_t* img, uint32_t side, uint32_t piece, uint8_t* slot, uint64_t* size, PngPiece* sums) {
    const uint32_t r0 = piece * kDfMemberText, n = png_piece_len(side, piece);
    const uint32_t first = piece == 0u ? 1u : 0u, last = r0 + n == png_raw(side) ? 1u : 0u;
    const uint32_t head = first ? 2u : 0u;   // bytes in front of the block
    // -- stage the raw bytes
    DF_LANES(t)
        for (uint32_t i = t; i < kDfTextWords; i += kDfThreads) {
            uint32_t w = 0;
            if (4u * i < n) {
                uint32_t row = (r0 + 4u * i) / (side + 1u), col = (r0 + 4u * i) - row * (side + 1u);   // col 0: the filter byte
                for (uint32_t b = 0; b < 4u && 4u * i + b < n; ++b) {
                    if (col) w |= static_cast<uint32_t>(img[row * side + col - 1u]) << (8u * b);
                    if (++col > side) { col = 0; ++row; }
                }
            }
            S.text[i] = w;
        }
        for (uint32_t i = t; i < (1u << kDfHashBits); i += kDfThreads) S.head[i] = 0;
        if (t < kDfU) S.u[t] = 0;
    DF_END
    // -- Adler-32: lane t takes bytes [t C, (t + 1) C) of the piece
    const uint32_t C = (n + kDfThreads - 1u) / kDfThreads;   // <= 255: a below 65521, b below 2^24
    DF_LANES(t)
        const uint8_t* tb = reinterpret_cast<const uint8_t*>(S.text);
        const uint32_t lo = t * C < n ? t * C : n, hi = (t + 1u) * C < n ? (t + 1u) * C : n;
        uint32_t a = 0, b = 0;
        for (uint32_t i = lo; i < hi; ++i) { a += tb[i]; b += a; }
        if (a) {   // the n - hi bytes behind the lane's add a to b once each
            df_add(&S.u[kPngA], a);
            df_add(&S.u[kPngB], b % kPngAdler + ((n - hi) * a) % kPngAdler);
        }
    DF_END
    // -- the block
    const uint32_t end = df_block(S, n, head * 8u, last, 5u, 1u, side + 1u);
    uint32_t total, pre = 0;   // bytes of the piece; of them in front of S.text's (a stored block's)
    if (end == 0u) {
        pre = head + 5u;
        total = pre + n;
        DF_LANES(t)
            const uint8_t* tb = reinterpret_cast<const uint8_t*>(S.text);
            for (uint32_t i = t; i < n; i += kDfThreads) slot[pre + i] = tb[i];
            if (t == 0u) {
                if (first) { slot[0] = kPngZlibHeader & 0xFFu; slot[1] = kPngZlibHeader >> 8; }
                slot[head] = static_cast<uint8_t>(last);   // BFINAL, BTYPE 0
                slot[head + 1u] = static_cast<uint8_t>(n & 0xFFu);
                slot[head + 2u] = static_cast<uint8_t>(n >> 8);
                slot[head + 3u] = static_cast<uint8_t>(~n & 0xFFu);
                slot[head + 4u] = static_cast<uint8_t>((~n >> 8) & 0xFFu);
            }
        DF_END
    } else {
        total = ((last ? end : end + 3u) + 7u) / 8u + (last ? 0u : 4u);
        DF_LANES(t)
            if (t == 0u) {
                if (first) df_put(S.text, 0u, kPngZlibHeader, 16u);
                if (!last) df_put(S.text, (total - 4u) * 8u, 0xFFFF0000u, 32u);   // the empty stored block's LEN, NLEN
            }
        DF_END
        DF_LANES(t)
            uint32_t* dst = reinterpret_cast<uint32_t*>(slot);
            for (uint32_t i = t; i < (total + 3u) / 4u; i += kDfThreads) dst[i] = S.text[i];
        DF_END
    }
    // -- CRC-32 of the piece's bytes: those in S.text by the lanes, a stored block's `pre` bytes in front by one
    DF_LANES(t)
        uint32_t c = t;
        for (uint32_t k = 0; k < 8u; ++k) c = (c & 1u) ? (c >> 1) ^ kDfPoly : c >> 1;
        S.head[t] = c;
    DF_END
    df_crc_lanes(S, total - pre, 0u);
    DF_LANES(t)
        if (t == 0u) {
            uint32_t reg = 0;
            if (pre) {
                if (first) { reg = png_crc_byte(reg, kPngZlibHeader & 0xFFu); reg = png_crc_byte(reg, kPngZlibHeader >> 8); }
                reg = png_crc_byte(reg, last);
                reg = png_crc_byte(reg, n & 0xFFu);
                reg = png_crc_byte(reg, n >> 8);
                reg = png_crc_byte(reg, ~n & 0xFFu);
                reg = png_crc_byte(reg, (~n >> 8) & 0xFFu);
                reg = df_mulmod(df_xpow8(n), reg);
            }
            sums->crc = reg ^ S.sorted[0];
            sums->a = S.u[kPngA] % kPngAdler;
            sums->b = S.u[kPngB] % kPngAdler;
            sums->raw = n;
            *size = total;
        }
    DF_END
}

// An image's pieces joined: the Adler-32 of its raw stream and the CRC-32 of its chunk ("IDAT", the pieces' bytes, the
// Adler-32).  sizes: the pieces' bytes.
DF_FN void png_join(const PngPiece* sums, const uint64_t* sizes, uint32_t npieces, uint32_t& adler, uint32_t& crc) {
    uint32_t a = 1, b = 0, reg = 0xFFFFFFFFu;
    reg = png_crc_byte(reg, 'I'); reg = png_crc_byte(reg, 'D'); reg = png_crc_byte(reg, 'A'); reg = png_crc_byte(reg, 'T');
    for (uint32_t p = 0; p < npieces; ++p) {
        b = static_cast<uint32_t>((b + static_cast<uint64_t>(sums[p].raw % kPngAdler) * a + sums[p].b) % kPngAdler);
        a = (a + sums[p].a) % kPngAdler;
        reg = df_mulmod(df_xpow8(static_cast<uint32_t>(sizes[p])), reg) ^ sums[p].crc;
    }
    adler = (b << 16) | a;
    for (uint32_t i = 0; i < 4u; ++i) reg = png_crc_byte(reg, (adler >> (24u - 8u * i)) & 0xFFu);
    crc = ~reg;
}

// byte i of a chunk's 8 bytes in front (length of the data: all but 12 of the chunk's bytes; "IDAT") or, from 8 on, of its 8 behind (Adler-32, CRC-32)
DF_FN uint32_t png_frame_byte(uint32_t i, uint32_t datalen, uint32_t adler, uint32_t crc) {
    const uint32_t w = i < 4u ? datalen : i < 8u ? 0x49444154u : i < 12u ? adler : crc;
    return (w >> (24u - 8u * (i & 3u))) & 0xFFu;
}

#if defined(__HIPCC__)

__global__ void __launch_bounds__(kDfThreads) vk_png_piece_kernel(const uint8_t* __restrict__ img, uint32_t side, uint32_t ppi,
                                                                  uint32_t slot, uint8_t* __restrict__ slots,
                                                                  uint64_t* __restrict__ sizes, PngPiece* __restrict__ sums) {
    extern __shared__ uint32_t vk_png_lds[];
    DfLds& S = *reinterpret_cast<DfLds*>(vk_png_lds);
    const uint32_t image = blockIdx.x / ppi, piece = blockIdx.x - image * ppi;
    png_piece(S, img + static_cast<uint64_t>(image) * side * side, side, piece, slots + static_cast<uint64_t>(blockIdx.x) * slot,
              sizes + blockIdx.x, sums + blockIdx.x);
}

// an image's chunk: its bytes, their number rounded up to 16 (what the scan lays the chunks out by), Adler-32 and CRC-32
__global__ void __launch_bounds__(kDfThreads) vk_png_image_kernel(uint32_t nimg, uint32_t ppi, const PngPiece* __restrict__ sums,
                                                                  const uint64_t* __restrict__ sizes,
                                                                  const uint64_t* __restrict__ pprefix, uint64_t* __restrict__ ilens,
                                                                  uint64_t* __restrict__ isizes, uint32_t* __restrict__ itail) {
    const uint32_t im = blockIdx.x * kDfThreads + threadIdx.x;
    if (im >= nimg) return;
    const uint64_t p0 = static_cast<uint64_t>(im) * ppi;
    const uint64_t len = pprefix[p0 + ppi] - pprefix[p0] + kPngFrame;
    uint32_t adler, crc;
    png_join(sums + p0, sizes + p0, ppi, adler, crc);
    ilens[im] = len;
    isizes[im] = (len + 15u) / 16u * 16u;
    itail[2ull * im] = adler;
    itail[2ull * im + 1u] = crc;
}

// blocks [0, npieces): piece b's slot to its place in its chunk (vk_df_gather_kernel's copy: dword stores aligned to the
// destination); blocks [npieces, npieces + nimg): a chunk's 8 bytes in front, its 8 behind and the zero bytes up to its
// 16-byte rounded end
__global__ void __launch_bounds__(kDfThreads) vk_png_gather_kernel(uint64_t npieces, uint32_t ppi, uint32_t slot,
                                                                   const uint8_t* __restrict__ slots,
                                                                   const uint64_t* __restrict__ pprefix,
                                                                   const uint64_t* __restrict__ ilens,
                                                                   const uint64_t* __restrict__ iprefix,
                                                                   const uint32_t* __restrict__ itail, uint8_t* __restrict__ out) {
    const uint64_t b = blockIdx.x;
    if (b >= npieces) {
        const uint64_t im = b - npieces;
        const uint32_t len = static_cast<uint32_t>(ilens[im]);
        const uint32_t span = static_cast<uint32_t>(iprefix[im + 1] - iprefix[im]) - len + 8u;   // < 24
        uint8_t* dst = out + iprefix[im];
        const uint32_t t = threadIdx.x;
        if (t < 8u) dst[t] = static_cast<uint8_t>(png_frame_byte(t, len - 12u, 0u, 0u));
        else if (t < 8u + span)
            dst[len - 16u + t] = t < 16u ? static_cast<uint8_t>(png_frame_byte(t, 0u, itail[2ull * im], itail[2ull * im + 1u])) : 0;
        return;
    }
    const uint64_t im = b / ppi;
    const uint32_t n = static_cast<uint32_t>(pprefix[b + 1] - pprefix[b]);
    uint8_t* dst = out + iprefix[im] + 8u + (pprefix[b] - pprefix[im * ppi]);
    const uint8_t* src = slots + b * slot;
    const uint32_t lead = static_cast<uint32_t>((4u - (reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u);
    const uint32_t h = lead < n ? lead : n, body = (n - h) / 4u;
    if (threadIdx.x < h) dst[threadIdx.x] = src[threadIdx.x];
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(src);
    uint32_t* dw = reinterpret_cast<uint32_t*>(dst + h);
    for (uint32_t i = threadIdx.x; i < body; i += kDfThreads) {
        const uint32_t at = h + 4u * i;   // (at & 3) != 0: the second dword holds byte at + 3 < n, inside the slot
        dw[i] = (at & 3u) ? vkl::alignbit(sw[(at >> 2) + 1u], sw[at >> 2], (at & 3u) * 8u) : sw[at >> 2];
    }
    const uint32_t done = h + 4u * body;
    if (threadIdx.x < n - done) dst[done + threadIdx.x] = src[done + threadIdx.x];
}

#endif  // __HIPCC__
#endif  // VK_PNG_H
