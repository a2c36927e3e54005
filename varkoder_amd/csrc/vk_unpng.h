// vk_unpng.h -- PNG decoder: the zlib streams of a batch of image files become images [side][side] in HBM.
//
// An 8-bit greyscale file of side x side pixels holds ONE zlib stream (its IDAT payloads, joined) whose text is the raw
// stream: side rows of 1 + side bytes, a filter byte and the row's filtered pixels.  Two kernels, each one wavefront
// per image:
//   1. vk_unpng_inflate_kernel: vk_inflate.h's decoder as it is, entered behind the two bytes of the zlib header
//      (gz_wave<false>, at_header = false, start_bit = 16).  After the final block the decoder wants a gzip trailer:
//      eight bytes, of which it hands back the first four (here: the stream's Adler-32, big-endian) and checks the last
//      four, a little-endian u32, against the text's length.  So the host puts side * (side + 1) as four bytes behind
//      every stream's Adler-32, and the raw-DEFLATE decode, the size check and the Adler word come without a change to
//      the decoder.  The text goes to the image's slot of the workspace, side * (side + 1) bytes rounded up to 16; the
//      slot's raw size is the decoder's `cap`.
//   2. vk_unpng_unfilter_kernel: the raw stream -> pixels.  Pixel (r, c) needs (r, c - 1), (r - 1, c), (r - 1, c - 1),
//      so the rows are taken in BANDS of 64: lane j owns row 64 * band + j and runs one column behind lane j - 1, which
//      gives side + 63 steps a band, a wave-uniform count.  A band lies in LDS as 65 rows of `stride` bytes: row 0 is
//      the last row of the band before (zeros for the first), rows 1 .. 64 the band's, column 0 of every row is 0
//      (where the filter byte was: it is "the pixel left of column 1") -- so left, up and up-left are plain reads one
//      byte and one row back, and a row is un-filtered in place.  In a step lane j reads what lane j - 1 wrote a step
//      EARLIER and writes where nobody reads in this step: the order the lanes run in within a step does not matter.
//      The filter type is a per-lane select over one formula.  stride - 1 is 4 * an odd number: the lanes of a step,
//      stride - 1 bytes apart, fall into different banks.
//      A band is staged with 16-byte loads (the slot is aligned), and the stream's Adler-32 is taken from those very
//      bytes: lane j sums row j (a = sum of the bytes, b = sum of (bytes behind and itself) * byte: below 2^26), and
//      one lane joins the rows in order by vk_png.h's combine rule mod 65521 -- no sum over more than one row is ever
//      held unreduced, so nothing overflows at 262,656 bytes.
//
// The file's rules are vk_deflate.h's: phases (UP_LANES(t) ... UP_END, 64 lanes), nothing in a register across a phase
// but values that every lane reads alike, plain stores.  tests/emul/unpng_emul.cpp runs unpng_image on the host.
#ifndef VK_UNPNG_H
#define VK_UNPNG_H

#include "vk_png.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define UP_LANES(t) { const uint32_t t = threadIdx.x;
#define UP_END } __syncthreads();
#else
#define UP_LANES(t) for (uint32_t t = 0; t < kUpLanes; ++t) {
#define UP_END }
#endif

constexpr uint32_t kUpLanes = 64;   // one wavefront: a band's rows
constexpr uint32_t kUpBadStream = 1u, kUpTruncated = 2u, kUpBadSize = 4u, kUpBadAdler = 8u, kUpBadFilter = 16u;   // VK_UNPNG_*
constexpr uint32_t kUpStreamMin = 2u + 4u + 4u;   // zlib header, Adler-32, the appended length

enum { kUpA = 0, kUpB, kUpSt, kUpU = 4 };   // UpLds::u: the Adler sums so far, status bits

// an image's slot in the workspace
constexpr uint32_t unpng_slot(uint32_t side) { return (png_raw(side) + 15u) / 16u * 16u; }
// bytes between two rows of a band in LDS: at least side + 1, and stride - 1 = 4 * odd
constexpr uint32_t unpng_stride(uint32_t side) { return (side + 7u) / 8u * 8u + 5u; }
static_assert(unpng_stride(1) >= 2 && unpng_stride(4) >= 5 && unpng_stride(5) >= 6 && unpng_stride(512) == 517, "a row fits its stride");
// dwords of LDS: ra, rb (a row's Adler sums), u, flt (a row's filter byte), the band's 65 rows
constexpr uint32_t unpng_lds_words(uint32_t side) { return 2u * kUpLanes + kUpU + kUpLanes / 4u + ((kUpLanes + 1u) * unpng_stride(side) + 3u) / 4u; }

struct alignas(16) UpQuad { uint32_t w[4]; };

// The raw stream raw[0 .. side * (side + 1)) (16-byte aligned, readable up to unpng_slot(side)) -> img[side][side].
// *status = st_in | kUpBadFilter | kUpBadAdler as found; with st_in != 0 nothing is read or written but *status.
// want: the stream's Adler-32 as the four bytes behind the data read as a little-endian word.
DF_FN void unpng_image(uint32_t* lds, const uint8_t* raw, uint32_t side, uint32_t want, uint32_t st_in, uint8_t* img, uint32_t* status) {
    uint32_t* ra = lds;
    uint32_t* rb = ra + kUpLanes;
    uint32_t* u = rb + kUpLanes;
    uint8_t* flt = reinterpret_cast<uint8_t*>(u + kUpU);
    uint8_t* rows = flt + kUpLanes;
    const uint32_t L = side + 1u, S = unpng_stride(side);
    if (st_in) {   // (alike for every lane)
        UP_LANES(t)
            if (t == 0u) *status = st_in;
        UP_END
        return;
    }
    UP_LANES(t)
        for (uint32_t c = t; c < S; c += kUpLanes) rows[c] = 0;
        if (t == 0u) { u[kUpA] = 1u; u[kUpB] = 0u; u[kUpSt] = 0u; }
    UP_END
    for (uint32_t r0 = 0; r0 < side; r0 += kUpLanes) {
        const uint32_t nrows = side - r0 < kUpLanes ? side - r0 : kUpLanes;
        const uint32_t b0 = r0 * L, b1 = b0 + nrows * L;
        // -- stage the band's raw bytes: 16 at a time, each to its row and column
        UP_LANES(t)
            const UpQuad* quads = reinterpret_cast<const UpQuad*>(raw);
            for (uint32_t q = b0 / 16u + t; 16u * q < b1; q += kUpLanes) {
                const UpQuad v = quads[q];
                const uint32_t first = 16u * q < b0 ? b0 - 16u * q : 0u;   // the quad's first byte of this band
                uint32_t r = (16u * q + first - b0) / L, c = (16u * q + first - b0) - r * L;
                for (uint32_t k = 0; k < 16u; ++k) {   // (a constant trip count: v stays in registers)
                    if (k >= first && 16u * q + k < b1) {
                        rows[(1u + r) * S + c] = static_cast<uint8_t>(v.w[k >> 2] >> (8u * (k & 3u)));
                        if (++c == L) { c = 0; ++r; }
                    }
                }
            }
        UP_END
        // -- Adler-32 of the rows, the filter bytes aside
        UP_LANES(t)
            if (t < nrows) {
                uint8_t* row = rows + (1u + t) * S;
                uint32_t a = 0, b = 0;
                for (uint32_t c = 0; c < L; ++c) { a += row[c]; b += a; }   // a <= 255 * 513, b <= 255 * 513 * 514 / 2
                ra[t] = a;
                rb[t] = b;
                flt[t] = row[0];
                row[0] = 0;
                if (flt[t] > 4u) df_or(&u[kUpSt], kUpBadFilter);
            }
        UP_END
        UP_LANES(t)
            if (t == 0u) {   // the rows joined in stream order: every term below 2^26
                uint32_t a = u[kUpA], b = u[kUpB];
                for (uint32_t r = 0; r < nrows; ++r) {
                    b = (b + L * a + rb[r]) % kPngAdler;
                    a = (a + ra[r]) % kPngAdler;
                }
                u[kUpA] = a;
                u[kUpB] = b;
            }
        UP_END
        // -- un-filter: in step s lane t does column s - t of its row
        for (uint32_t s = 0; s < side + kUpLanes - 1u; ++s) {
            UP_LANES(t)
                const uint32_t c = s - t;   // (wraps for s < t: not below side then)
                if (t < nrows && c < side) {
                    uint8_t* row = rows + (1u + t) * S + c;   // row[0]: left, row[1]: this pixel; S back: the row above
                    const uint32_t ft = flt[t];
                    const int32_t x = row[1], a = row[0], b = row[1 - static_cast<int32_t>(S)], cc = row[-static_cast<int32_t>(S)];
                    const int32_t pa = b > cc ? b - cc : cc - b, pb = a > cc ? a - cc : cc - a;
                    const int32_t pc = a + b > 2 * cc ? a + b - 2 * cc : 2 * cc - a - b;
                    const int32_t paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : cc);
                    const int32_t pred = ft == 1u ? a : ft == 2u ? b : ft == 3u ? (a + b) >> 1 : ft == 4u ? paeth : 0;
                    row[1] = static_cast<uint8_t>(x + pred);
                }
            UP_END
        }
        // -- the band's pixels out: dword stores aligned to the destination; then its last row becomes row 0
        UP_LANES(t)
            uint8_t* dst = img + r0 * side;
            const uint32_t n = nrows * side;
            const uint32_t lead = static_cast<uint32_t>((4u - (reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u);
            const uint32_t h = lead < n ? lead : n, body = (n - h) / 4u;
            if (t < h) dst[t] = rows[(1u + t / side) * S + 1u + t % side];
            uint32_t* dw = reinterpret_cast<uint32_t*>(dst + h);
            for (uint32_t i = t; i < body; i += kUpLanes) {
                uint32_t r = (h + 4u * i) / side, c = (h + 4u * i) - r * side, w = 0;
                for (uint32_t k = 0; k < 4u; ++k) {
                    w |= static_cast<uint32_t>(rows[(1u + r) * S + 1u + c]) << (8u * k);
                    if (++c == side) { c = 0; ++r; }
                }
                dw[i] = w;
            }
            const uint32_t done = h + 4u * body;
            if (t < n - done) dst[done + t] = rows[(1u + (done + t) / side) * S + 1u + (done + t) % side];
        UP_END
        UP_LANES(t)
            for (uint32_t c = 1u + t; c < L; c += kUpLanes) rows[c] = rows[nrows * S + c];
        UP_END
    }
    UP_LANES(t)
        if (t == 0u) {
            const uint32_t adler = (u[kUpB] << 16) | u[kUpA];
            const uint32_t stored = (want >> 24) | ((want >> 8) & 0xFF00u) | ((want << 8) & 0xFF0000u) | (want << 24);
            *status = u[kUpSt] | (adler != stored ? kUpBadAdler : 0u);
        }
    UP_END
}

#if defined(__HIPCC__)

// gz_wave's status bits as VK_UNPNG_*: text that does not end where the slot does is a bad size either way
__device__ __forceinline__ uint32_t unpng_status(uint32_t gz) {
    return ((gz & (kGzBadData | kGzBadHeader)) ? kUpBadStream : 0u) | ((gz & kGzTruncated) ? kUpTruncated : 0u) |
           ((gz & (kGzOverflow | kGzBadSize)) ? kUpBadSize : 0u);
}

// stream i: streams[offsets[i] .. +lengths[i]) = zlib header, blocks, Adler-32, side * (side + 1) as a little-endian u32
__global__ __launch_bounds__(64) void vk_unpng_inflate_kernel(const uint8_t* __restrict__ streams, const uint64_t* __restrict__ offsets,
                                                               const uint64_t* __restrict__ lengths, uint32_t nimg, uint32_t side,
                                                               uint8_t* __restrict__ slots, uint32_t* __restrict__ st,
                                                               uint32_t* __restrict__ adler) {
    __shared__ GzLds L;
    __shared__ uint16_t hist[kGzHist];
    const uint32_t im = blockIdx.x;
    if (im >= nimg) return;
#if VK_GZ_SYMTAB
    gz_lds_init(L);
#endif
    uint64_t n = 0, endbit = 0;
    uint32_t gz = 0, next = 0, isum = 0, nm = 0, cr = 0;
    gz_wave<false>(L, hist, streams + offsets[im], lengths[im], slots + static_cast<uint64_t>(im) * unpng_slot(side), nullptr,
                   png_raw(side), 16, false, nullptr, 0, 0, n, gz, next, endbit, isum, nm, cr, nullptr);
    if ((threadIdx.x & 63) == 0) {
        st[im] = unpng_status(gz);
        adler[im] = cr;
    }
}

__global__ __launch_bounds__(kUpLanes) void vk_unpng_unfilter_kernel(const uint8_t* __restrict__ slots, uint32_t nimg, uint32_t side,
                                                                     const uint32_t* __restrict__ st, const uint32_t* __restrict__ adler,
                                                                     uint8_t* __restrict__ img, uint32_t* __restrict__ status) {
    extern __shared__ uint32_t vk_unpng_lds[];
    const uint32_t im = blockIdx.x;
    if (im >= nimg) return;
    unpng_image(vk_unpng_lds, slots + static_cast<uint64_t>(im) * unpng_slot(side), side, adler[im], st[im],
                img + static_cast<uint64_t>(im) * side * side, status + im);
}

#endif  // __HIPCC__
#endif  // VK_UNPNG_H
