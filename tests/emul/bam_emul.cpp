// bam_emul.cpp -- CPU emulation of the lane-local device code of the BAM to FASTQ conversion (test only).
//
// Compiles the product's own csrc/vk_bam.h for the host (VK_BAM_LANE_ONLY: bam_read, bam_plausible, bam_guess_ok,
// bam_class, bam_text_size, bam_walk, bam_emit_of, bam_text_byte, bam_emit_range, bam_items, bam_emit_item) and runs a file
// the way the kernels cut it: segment after segment.  Every segment but the first takes as its guess the smallest offset
// among its bytes that bam_guess_ok accepts (what the ballot over the lanes' candidates finds) and is walked from there;
// then the segments are linked in order from first_record -- a guess that equals the true entry stands, any other segment
// is walked again or starts no record -- and every stream's text is written segment by segment, record by record from the
// starts the walks noted, item by item, each read at the place the tallies of the segments before it give.  The file, every
// segment's starts and every text lie in heap blocks of exactly their size: under the address sanitizer a byte read past
// the file, a start noted past its segment's share or a byte written past a text is an error.
//
// What it does NOT cover: the kernels themselves.  The ballot and the 64-at-a-step run of the link pass (here: one segment
// at a time, which is what they compute), the wave prefix sums over tallies, record sizes and items (here: running sums),
// the search of an item's record in LDS, the split of a workgroup's threads over the items and the stores' order exist
// only on the GPU: tests/test_gpu_bam.py.
//
// A stand-alone program:  bam_emul IN OUT SEG_BYTES NO_GUESS EXCLUDE
//   IN:  cases, each u32 length, u64 first_record, i32 n_ref and the bytes.
//   OUT: per case u32 status, u64 segments, u64 rewalked, then for ALL, READ1, READ2, SINGLE a u64 length and the text.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define __device__
#define VK_BAM_LANE_ONLY
#include "vk_bam.h"

namespace {

struct Seg {
    uint64_t entry = kBamNone, exit = 0, base[3] = {0, 0, 0};
    BamTally t{};
    uint32_t status = 0, nrec = 0;
    bool guessed = false;
    std::vector<uint16_t> starts;   // bam_starts_cap entries, as the kernels' workspace holds per segment
};

uint64_t pick(const uint64_t* v, uint32_t select) { return select == kBamAll ? v[0] + v[1] + v[2] : v[select - 1]; }

struct Result {
    uint32_t status = 0;
    uint64_t segments = 0, rewalked = 0;
    std::vector<uint8_t> text[4];
};

Result convert(const uint8_t* p, uint64_t len, uint64_t first, int32_t n_ref, uint64_t seg_bytes, bool no_guess, uint32_t exclude) {
    Result res;
    uint64_t nseg = (len + seg_bytes - 1) / seg_bytes;
    if (nseg == 0) nseg = 1;
    std::vector<Seg> segs(nseg);
    const uint32_t cap = bam_starts_cap(static_cast<uint32_t>(seg_bytes));
    for (Seg& s : segs) s.starts.assign(cap, 0xFFFF);
    auto seg_end = [&](uint64_t j) { return (j + 1) * seg_bytes < len ? (j + 1) * seg_bytes : len; };
    // segment pass
    for (uint64_t j = 0; j < nseg; ++j) {
        Seg& s = segs[j];
        const uint64_t start = j * seg_bytes, end = seg_end(j);
        if (j == 0) s.entry = first;
        else if (!no_guess)
            for (uint64_t c = start; c < end; ++c)
                if (bam_guess_ok(p, len, n_ref, c)) {
                    s.entry = c;
                    break;
                }
        s.guessed = s.entry != kBamNone;
        s.exit = s.entry;
        if (s.guessed) s.status = bam_walk(p, len, s.entry, end, exclude, &s.t, &s.exit, start, s.starts.data(), cap, &s.nrec);
    }
    // link pass
    uint64_t truth = first, carry_b[3] = {0, 0, 0};
    uint32_t status = 0;
    for (uint64_t j = 0; j < nseg && !status; ++j) {
        Seg& s = segs[j];
        if (!(s.guessed && s.entry == truth)) {
            s = Seg();
            s.starts.assign(cap, 0xFFFF);
            s.entry = s.exit = truth;
            s.guessed = true;
            if (truth < seg_end(j)) {
                s.status = bam_walk(p, len, truth, seg_end(j), exclude, &s.t, &s.exit, j * seg_bytes, s.starts.data(), cap, &s.nrec);
                ++res.rewalked;
            }
        }
        status = s.status;
        for (int c = 0; c < 3; ++c) {
            s.base[c] = carry_b[c];
            carry_b[c] += s.t.bytes[c];
        }
        truth = s.exit;
    }
    if (!status && truth != len) status = kBamTruncated;
    res.status = status;
    res.segments = nseg;
    if (status) return res;
    // emit pass
    for (uint32_t select = 0; select < 4; ++select) {
        std::vector<uint8_t>& out = res.text[select];
        out.assign(pick(carry_b, select), 0xEE);
        std::vector<uint8_t> written(out.size(), 0);
        for (uint64_t j = 0; j < nseg; ++j) {
            const Seg& s = segs[j];
            uint64_t pos = pick(s.base, select);
            for (uint32_t i = 0; i < s.nrec && i < cap; ++i) {   // from the noted starts, as the emit kernel
                BamRec r;
                const uint64_t here = j * seg_bytes + s.starts[i];
                if (bam_read(p, len, here, &r) || !bam_takes(select, bam_class(r, exclude))) continue;
                const uint64_t size = bam_text_size(r);
                if (pos + size > out.size()) {
                    fprintf(stderr, "a read past its stream's text\n");
                    exit(3);
                }
                const BamEmit e = bam_emit_of(p, r);
                uint8_t* dst = out.data() + pos;
                const uint64_t items = bam_items(dst, size);
                for (uint64_t it = items; it-- > 0;) bam_emit_item(e, dst, size, it);   // (any order: the items are disjoint)
                for (uint64_t i = 0; i < size; ++i) ++written[pos + i];
                pos += size;
            }
        }
        for (uint8_t w : written)
            if (w != 1) {
                fprintf(stderr, "a text byte written %u times\n", w);
                exit(3);
            }
    }
    return res;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 6) {
        fprintf(stderr, "usage: bam_emul IN OUT SEG_BYTES NO_GUESS EXCLUDE\n");
        return 2;
    }
    const uint64_t seg_bytes = strtoull(argv[3], nullptr, 10);
    const bool no_guess = atoi(argv[4]) != 0;
    const uint32_t exclude = static_cast<uint32_t>(strtoul(argv[5], nullptr, 0));
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out || seg_bytes < 64 || seg_bytes > kBamSegBytes) return 2;
    for (;;) {
        uint32_t len;
        uint64_t first;
        int32_t n_ref;
        if (fread(&len, 4, 1, in) != 1) break;
        if (fread(&first, 8, 1, in) != 1 || fread(&n_ref, 4, 1, in) != 1) return 2;
        uint8_t* data = static_cast<uint8_t*>(malloc(len ? len : 1));   // exactly the file: nothing behind it may be read
        if (len && fread(data, 1, len, in) != len) return 2;
        const Result r = convert(data, len, first, n_ref, seg_bytes, no_guess, exclude);
        fwrite(&r.status, 4, 1, out);
        fwrite(&r.segments, 8, 1, out);
        fwrite(&r.rewalked, 8, 1, out);
        for (const auto& t : r.text) {
            const uint64_t n = t.size();
            fwrite(&n, 8, 1, out);
            if (n) fwrite(t.data(), 1, n, out);
        }
        free(data);
    }
    fclose(in);
    fclose(out);
    return 0;
}
