// unpng_emul.cpp -- CPU emulation of the PNG decoder's un-filter and Adler-32 function (test only).
//
// Compiles the product's own csrc/vk_unpng.h for the host: unpng_image() runs as it is, every phase as a loop over the
// 64 lanes, one after another, on LDS words in ordinary memory.  Lets the CPU suite check the decoder's arithmetic --
// staging a band from 16-byte loads, the rows' Adler sums and their joining, the five filters in the order of the
// band's steps, the seam between two bands, the aligned stores of the pixels -- with PIL as the judge.
//
// It checks unpng_image ONLY.  The inflate kernel is vk_inflate.h's decoder, which has no host build: the raw stream
// is zlib's here.  Barriers and the LDS atomic are not exercised, and only the GPU tests (tests/test_gpu_unpng.py) run
// the real ones.
//
// With UNPNG_EMUL_MAIN the file is a program: `unpng_emul FILE...` reads FILE (side, then the number of images, as 4
// bytes little-endian each; per image the Adler word as it lies behind the stream read as a little-endian u32, then
// side * (side + 1) raw bytes) and writes the statuses and then the images to FILE.img.  That is the form a sanitizer
// build runs in (tests/test_unpng_emulation.py).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "vk_unpng.h"

extern "C" uint32_t emul_unpng_slot(uint32_t side) { return unpng_slot(side); }
extern "C" uint32_t emul_unpng_stride(uint32_t side) { return unpng_stride(side); }

// raw[nimg][side * (side + 1)] (packed), want[nimg], st_in[nimg] (may be null: zeros) -> img[nimg][side][side],
// status[nimg].  Every image is staged from a buffer of exactly its slot, so that a read behind it is seen by a sanitizer.
extern "C" int emul_unpng(const uint8_t* raw, uint32_t nimg, uint32_t side, const uint32_t* want, const uint32_t* st_in, uint8_t* img,
                          uint32_t* status) {
    if (!raw || !want || !img || !status || nimg == 0 || side == 0 || side > kPngMaxSide) return 1;
    const size_t n = png_raw(side), px = static_cast<size_t>(side) * side;
    for (uint32_t im = 0; im < nimg; ++im) {
        std::vector<UpQuad> slot(unpng_slot(side) / 16);
        std::vector<uint32_t> lds(unpng_lds_words(side));
        memcpy(slot.data(), raw + im * n, n);
        unpng_image(lds.data(), reinterpret_cast<const uint8_t*>(slot.data()), side, want[im], st_in ? st_in[im] : 0u, img + im * px,
                    status + im);   // (images packed: with an odd side every alignment of the stores occurs)
    }
    return 0;
}

#ifdef UNPNG_EMUL_MAIN
int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) return 2;
        std::vector<uint8_t> data;
        uint8_t buf[65536];
        for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) data.insert(data.end(), buf, buf + got);
        fclose(f);
        if (data.size() < 8) return 2;
        uint32_t side, nimg;
        memcpy(&side, data.data(), 4);
        memcpy(&nimg, data.data() + 4, 4);
        if (side == 0 || side > kPngMaxSide || nimg == 0) return 2;
        const size_t n = png_raw(side), px = static_cast<size_t>(side) * side;
        if (data.size() != 8 + nimg * (4 + n)) return 2;
        std::vector<uint8_t> raw(nimg * n), img(nimg * px);
        std::vector<uint32_t> want(nimg), status(nimg);
        for (uint32_t i = 0; i < nimg; ++i) {
            memcpy(&want[i], data.data() + 8 + i * (4 + n), 4);
            memcpy(raw.data() + i * n, data.data() + 8 + i * (4 + n) + 4, n);
        }
        if (emul_unpng(raw.data(), nimg, side, want.data(), nullptr, img.data(), status.data())) return 3;
        const std::string name = std::string(argv[a]) + ".img";
        FILE* g = fopen(name.c_str(), "wb");
        if (!g) return 4;
        if (fwrite(status.data(), 4, nimg, g) != nimg || fwrite(img.data(), 1, img.size(), g) != img.size()) return 4;
        fclose(g);
    }
    return 0;
}
#endif
