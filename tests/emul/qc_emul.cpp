// qc_emul.cpp -- CPU emulation of the lane-local device code of `--qc-report` (test only).
//
// Compiles the product's own csrc/vk_qc.h for the host (VK_QC_LANE_ONLY: qc_class, qc_phred, qc_lane_chunk, qc_merge,
// QcTile, QcLane and the row's layout) and runs a stream the way vk_qc_count_kernel cuts it: the budgeted records in
// workgroups of VK_QC_MERGE records (a compile-time constant: the test builds this program at the product's value and
// at 3), a workgroup's tile zeroed, its records dealt to 8 wavefronts (record j to wavefront j % 8), a record's cycles
// taken 256 at a time by 64 lanes calling qc_lane_chunk, the tile merged into the row by 512 threads calling qc_merge.
// qc_class and qc_phred are first held against a plain restatement for every byte value.
// After every workgroup the tile's cells are checked against the widths vk_qc.h claims for them (a count below 2^10, a
// quality sum below 2^22 and neither carried into the other: the cell must equal the two tallied apart).
// Every stream's text lies in a heap block of exactly its size and the tile in one of exactly sizeof(QcTile), so under the
// address sanitizer a byte read past a stream's end or a cell addressed past the tile is an error.
//
// What it does NOT cover: the kernels themselves -- the record index (the line ends are found here by a plain walk), the
// status and finish kernels, the atomic additions of concurrent lanes and workgroups, the wave-wide sums of the quality,
// GC, other and invalid counts (summed here over the lanes one by one), VKIMG_QC_MERGE: tests/test_gpu_qc.py.
//
// A stand-alone program:  qc_emul IN OUT
//   IN:  streams, each u32 records, u32 length, the text.
//   OUT: per stream u32 status, then VK_QC_NSTAT u64.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#define __device__
#define __host__
// what vk_qc.h takes from HIP: the additions to the tile and to the row
#define QC_ADD32(p, v) (*(p) += (v))
#define QC_ADD64(p, v) (*(p) += (v))
#define VK_QC_LANE_ONLY
#include "vk_qc.h"

namespace {

[[noreturn]] void die(const char* what) {
    fprintf(stderr, "qc_emul: %s\n", what);
    exit(2);
}

struct Rec {   // a record's sequence and quality lines without their '\r'
    uint64_t h, p, s, q;
    uint64_t ls, lq;
};

uint64_t line_len(const uint8_t* text, uint64_t a, uint64_t e) {   // [a, e) without one trailing '\r'
    return e > a && text[e - 1] == '\r' ? e - a - 1 : e - a;
}

// One stream: false when it has a status.
bool run_stream(const uint8_t* text, uint64_t len, uint64_t records, uint32_t* status, uint64_t* row) {
    std::vector<uint64_t> ends;
    for (uint64_t i = 0; i < len; ++i)
        if (text[i] == '\n') ends.push_back(i);
    if (len && text[len - 1] != '\n') ends.push_back(len);
    if (ends.size() < 4 * records) {
        *status = 8u;   // VK_EM_BAD_RECORDS
        return false;
    }
    std::vector<Rec> recs(records);
    for (uint64_t r = 0; r < records; ++r) {
        Rec& g = recs[r];
        g.h = r ? ends[4 * r - 1] + 1 : 0;
        g.s = ends[4 * r] + 1;
        g.p = ends[4 * r + 1] + 1;
        g.q = ends[4 * r + 2] + 1;
        g.ls = line_len(text, g.s, ends[4 * r + 1]);
        g.lq = line_len(text, g.q, ends[4 * r + 3]);
        if (text[g.h] != '@' || text[g.p] != '+') {
            *status = kQcBadFraming;
            return false;
        }
    }
    uint64_t minlen = ~0ull, maxlen = 0;
    std::unique_ptr<QcTile> tile(new QcTile);
    for (uint64_t r0 = 0; r0 < records; r0 += kQcMerge) {
        memset(tile.get(), 0, sizeof(QcTile));
        const uint32_t n = static_cast<uint32_t>(std::min<uint64_t>(kQcMerge, records - r0));
        std::vector<uint32_t> cnt(kQcClasses * kQcCycles, 0), sum(kQcClasses * kQcCycles, 0);   // the cells, tallied apart
        for (uint32_t wave = 0; wave < kQcThreads / 64; ++wave) {
            QcLane lanes[64];
            for (uint32_t j = wave; j < n; j += kQcThreads / 64) {
                const Rec& g = recs[r0 + j];
                ++row[kQcRecords];
                if (g.ls != g.lq) {
                    ++row[kQcRagged];
                    continue;
                }
                uint64_t qsum = 0;
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    lanes[lane].qsum = 0;
                    for (uint64_t c0 = 0; c0 < g.ls; c0 += kQcChunk) qc_lane_chunk(text + g.s, text + g.q, c0, g.ls, lane, tile.get(), &lanes[lane]);
                    qsum += lanes[lane].qsum;
                }
                for (uint64_t c = 0; c < std::min<uint64_t>(g.ls, kQcCycles); ++c) {
                    uint32_t bad;
                    const uint32_t cell = qc_class(text[g.s + c]) * kQcCycles + static_cast<uint32_t>(c);
                    ++cnt[cell];
                    sum[cell] += qc_phred(text[g.q + c], &bad);
                }
                row[kQcBases] += g.ls;
                minlen = std::min(minlen, g.ls);
                maxlen = std::max(maxlen, g.ls);
                tile->maxc = std::max<uint32_t>(tile->maxc, static_cast<uint32_t>(std::min<uint64_t>(g.ls, kQcCycles)));
                ++tile->len[std::min<uint64_t>(g.ls, kQcLenBins - 1)];
                if (g.ls) ++tile->readq[qsum / g.ls];
            }
            for (const QcLane& a : lanes) {
                row[kQcGc] += a.gc;
                row[kQcOther] += a.other;
                row[kQcInvalid] += a.invalid;
            }
        }
        for (uint32_t i = 0; i < kQcClasses * kQcCycles; ++i) {
            if (cnt[i] >= (1u << (32 - kQcSumBits)) || sum[i] >= (1u << kQcSumBits)) die("a cycle cell's field is too narrow");
            if (tile->cyc[i] != ((cnt[i] << kQcSumBits) | sum[i])) die("a cycle cell is not its count and its sum");
        }
        for (uint32_t t = 0; t < kQcThreads; ++t) qc_merge(tile.get(), row, t, kQcThreads);
    }
    row[kQcMinLen] = minlen == ~0ull ? 0 : minlen;
    row[kQcMaxLen] = maxlen;
    return true;
}

uint32_t get32(const std::vector<uint8_t>& in, size_t* at) {
    if (*at + 4 > in.size()) die("short input");
    uint32_t v;
    memcpy(&v, in.data() + *at, 4);
    *at += 4;
    return v;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) die("usage: qc_emul IN OUT");
    for (uint32_t b = 0; b < 256; ++b) {   // every byte: the class and the phred against a plain restatement
        const char* at = strchr("ACGTacgt", static_cast<int>(b));
        const uint32_t cls = b && at ? static_cast<uint32_t>(at - "ACGTacgt") % 4u : 4u;
        uint32_t bad;
        if (qc_class(b) != cls) die("qc_class differs");
        if (qc_phred(b, &bad) != (b < 33 ? 0u : b > 126 ? 93u : b - 33u) || bad != (b < 33 || b > 126 ? 1u : 0u)) die("qc_phred differs");
    }
    std::vector<uint8_t> in;
    {
        FILE* f = fopen(argv[1], "rb");
        if (!f) die("cannot read IN");
        static uint8_t buf[1 << 20];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + n);
        fclose(f);
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) die("cannot write OUT");
    size_t at = 0;
    std::vector<uint64_t> row(kQcNstat);
    while (at < in.size()) {
        const uint32_t records = get32(in, &at), len = get32(in, &at);
        if (at + len > in.size()) die("bad stream");
        std::unique_ptr<uint8_t[]> text(new uint8_t[len ? len : 1]);   // a heap block of exactly the stream's size
        memcpy(text.get(), in.data() + at, len);
        at += len;
        uint32_t status = 0;
        std::fill(row.begin(), row.end(), 0);
        if (!run_stream(text.get(), len, records, &status, row.data())) std::fill(row.begin(), row.end(), 0);
        if (fwrite(&status, 4, 1, out) != 1 || fwrite(row.data(), 8, row.size(), out) != row.size()) die("cannot write OUT");
    }
    fclose(out);
    return 0;
}
