// png_emul.cpp -- CPU emulation of the PNG encoder's piece kernel and join (test only).
//
// Compiles the product's own csrc/vk_png.h (and through it vk_deflate.h) for the host: png_piece() and png_join() run as
// they are, every phase as a loop over the 256 lanes, one after another, on a DfLds in ordinary memory.  Lets the CPU
// suite check the encoder's arithmetic -- staging with the filter bytes, the Adler-32 sums and their joining, the
// pieces' framing, the CRC-32 carried over the pieces -- with zlib and PIL as the judges.
//
// It checks vk_png.h's arithmetic ONLY.  The packing of the chunks (every chunk at a multiple of 16, zero bytes up to
// the next) is restated here the way vk_png_image_kernel, the scans and vk_png_gather_kernel do it; barriers and LDS
// atomics are not exercised at all, and only the GPU tests (tests/test_gpu_png.py) run the real ones.
//
// With PNG_EMUL_MAIN the file is a program: `png_emul FILE...` reads FILE (side as 4 bytes little-endian, then
// images of side * side bytes) and writes the chunks one behind the other to FILE.idat.  That is the form a sanitizer
// build runs in (tests/test_png_emulation.py).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "vk_png.h"

extern "C" uint32_t emul_png_pieces(uint32_t side) { return png_pieces(side); }

extern "C" uint64_t emul_png_bound(uint32_t side, uint32_t nimg) {
    const uint64_t raw = static_cast<uint64_t>(side) * (side + 1), pieces = (raw + 65279) / 65280;
    return (16 + 2 + raw + 9 * pieces + 15) / 16 * 16 * nimg;
}

// img[nimg][side][side] -> chunks at out[offsets[i] .. +lengths[i]); piece_sizes[nimg * pieces] (may be null): the bytes
// of every piece.  Returns 1 (VK_EINVAL) or 6 (VK_ENOSPC) without writing.
extern "C" int emul_png(const uint8_t* img, uint32_t nimg, uint32_t side, uint8_t* out, uint64_t cap, uint64_t* offsets,
                        uint64_t* lengths, uint64_t* piece_sizes) {
    if (!img || !out || !offsets || !lengths || nimg == 0 || side == 0 || side > kPngMaxSide) return 1;
    if (cap < emul_png_bound(side, nimg)) return 6;
    auto lds = std::make_unique<DfLds>();
    const uint32_t ppi = png_pieces(side);
    std::vector<std::vector<uint32_t>> slots(ppi, std::vector<uint32_t>(png_slot(side) / 4));
    std::vector<uint64_t> sizes(ppi);
    std::vector<PngPiece> sums(ppi);
    uint64_t at = 0;
    for (uint32_t im = 0; im < nimg; ++im) {
        uint64_t len = kPngFrame;
        for (uint32_t p = 0; p < ppi; ++p) {
            png_piece(*lds, img + static_cast<uint64_t>(im) * side * side, side, p, reinterpret_cast<uint8_t*>(slots[p].data()),
                      &sizes[p], &sums[p]);
            if (sizes[p] > png_piece_bound(png_piece_len(side, p), p == 0)) return 100;
            if (piece_sizes) piece_sizes[static_cast<uint64_t>(im) * ppi + p] = sizes[p];
            len += sizes[p];
        }
        uint32_t adler, crc;
        png_join(sums.data(), sizes.data(), ppi, adler, crc);
        uint8_t* dst = out + at;
        for (uint32_t i = 0; i < 8; ++i) dst[i] = static_cast<uint8_t>(png_frame_byte(i, static_cast<uint32_t>(len) - 12, 0, 0));
        uint64_t o = 8;
        for (uint32_t p = 0; p < ppi; ++p) {
            memcpy(dst + o, slots[p].data(), sizes[p]);
            o += sizes[p];
        }
        for (uint32_t i = 8; i < 16; ++i) dst[o + i - 8] = static_cast<uint8_t>(png_frame_byte(i, 0, adler, crc));
        const uint64_t rounded = (len + 15) / 16 * 16;
        for (uint64_t i = len; i < rounded; ++i) dst[i] = 0;
        offsets[im] = at;
        lengths[im] = len;
        at += rounded;
    }
    return 0;
}

#ifdef PNG_EMUL_MAIN
int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) return 2;
        std::vector<uint8_t> data;
        uint8_t buf[65536];
        for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) data.insert(data.end(), buf, buf + got);
        fclose(f);
        if (data.size() < 4) return 2;
        uint32_t side;
        memcpy(&side, data.data(), 4);
        if (side == 0 || side > kPngMaxSide || (data.size() - 4) % (static_cast<size_t>(side) * side)) return 2;
        const uint32_t nimg = static_cast<uint32_t>((data.size() - 4) / (static_cast<size_t>(side) * side));
        std::vector<uint8_t> img(data.begin() + 4, data.end());   // (a buffer of exactly the images: a read behind them is seen)
        std::vector<uint8_t> out(emul_png_bound(side, nimg));
        std::vector<uint64_t> offs(nimg), lens(nimg);
        if (emul_png(img.data(), nimg, side, out.data(), out.size(), offs.data(), lens.data(), nullptr)) return 3;
        const std::string name = std::string(argv[a]) + ".idat";
        FILE* g = fopen(name.c_str(), "wb");
        if (!g) return 4;
        for (uint32_t i = 0; i < nimg; ++i)
            if (fwrite(out.data() + offs[i], 1, lens[i], g) != lens[i]) return 4;
        fclose(g);
    }
    return 0;
}
#endif
