// deflate_emul.cpp -- CPU emulation of the BGZF compressor's member kernel (test only).
//
// Compiles the product's own csrc/vk_deflate.h for the host: df_member() runs as it is, every phase as a loop over the
// 256 lanes, one after another (the header's DF_LANES / DF_END), on a DfLds that lies in ordinary memory.  Lets the CPU
// suite check the compressor's arithmetic -- CRC-32 pieces and their joining, match finding and token resolution, the
// two Huffman codes and their 15-bit limit, block choice, bit packing, member framing -- with zlib as the judge.
//
// It checks vk_deflate.h's arithmetic ONLY.  The cutting of a text into members, the layout of a file (members, then
// the EOF member) and vk_deflate_bound's formula are restated here the way vkimg.hip and vk_df_gather_kernel do them:
// a change to those does not reach this file, barriers and LDS atomics are not exercised at all, and only the GPU tests
// (tests/test_gpu_deflate.py) run the real ones.
//
// With DEFLATE_EMUL_MAIN the file is a program: `deflate_emul FILE...` writes FILE.gz for every FILE.  That is the
// form a sanitizer build runs in (tests/test_deflate_emulation.py).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "vk_deflate.h"

extern "C" uint64_t emul_deflate_bound(uint64_t len) {
    const uint64_t members = (len + kDfMemberText - 1) / kDfMemberText;
    return (members * 31 + len + kDfEofBytes + 15) / 16 * 16;
}

// One text -> one BGZF file at out[0 .. *out_len).  Returns 6 (VK_ENOSPC) without writing when cap is below the bound.
extern "C" int emul_deflate(const uint8_t* text, uint64_t len, uint8_t* out, uint64_t cap, uint64_t* out_len) {
    if (cap < emul_deflate_bound(len)) return 6;
    auto lds = std::make_unique<DfLds>();
    std::vector<uint32_t> staged(kDfMemberText / 4 + 1);   // (the kernel reads a member's text as dwords)
    std::vector<uint32_t> slot(kDfSlot / 4);
    uint64_t at = 0;
    for (uint64_t off = 0; off < len; off += kDfMemberText) {
        const uint32_t n = static_cast<uint32_t>(len - off < kDfMemberText ? len - off : kDfMemberText);
        memcpy(staged.data(), text + off, n);
        uint64_t size = 0;
        df_member(*lds, reinterpret_cast<const uint8_t*>(staged.data()), n, reinterpret_cast<uint8_t*>(slot.data()), &size);
        memcpy(out + at, slot.data(), size);
        at += size;
    }
    for (uint32_t i = 0; i < kDfEofBytes; ++i) out[at + i] = static_cast<uint8_t>(df_eof_word(i >> 2) >> (8 * (i & 3)));
    *out_len = at + kDfEofBytes;
    return 0;
}

#ifdef DEFLATE_EMUL_MAIN
int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) return 2;
        std::vector<uint8_t> text;
        uint8_t buf[65536];
        for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) text.insert(text.end(), buf, buf + got);
        fclose(f);
        std::vector<uint8_t> out(emul_deflate_bound(text.size()));
        uint64_t n = 0;
        if (emul_deflate(text.data(), text.size(), out.data(), out.size(), &n)) return 3;
        const std::string name = std::string(argv[a]) + ".gz";
        FILE* g = fopen(name.c_str(), "wb");
        if (!g || fwrite(out.data(), 1, n, g) != n) return 4;
        fclose(g);
    }
    return 0;
}
#endif
