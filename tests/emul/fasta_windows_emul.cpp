// fasta_windows_emul.cpp -- CPU emulation of the lane-local device code of the per-window FASTA count (test only).
//
// Compiles the product's own csrc/vk_fasta_windows.h for the host (VK_FASTA_LANE_ONLY: FawPos, faw_step, faw_lane_count
// on top of vk_fasta.h's FaWalk, vk_fasta_records.h's fa_lane_headers and vk_fasta_ladder.h's fa_lane_bases) and runs a
// sample the way the kernels cut it: unit after unit (a workgroup per unit, as with VKIMG_FASTA_UNIT_BYTES set), lane
// after lane, each lane with the 64 bytes it would have loaded, the header state, the header count and the ordinal of
// its first sequence byte, its walk over its own bytes and its read forward past them.  Tiles are counted and m of them
// summed into every window, as the kernels do.  For k <= 7 the unit's table stands in for the LDS table: it belongs to
// the (record, tile) that enters the unit and is added to that tile's row at the unit's end, or never used when that
// tile has no row.
//
// What it does NOT cover: the kernels themselves.  fa_load's bounds, the scans (here running sums in lane order, which
// is what they compute), vk_faw_plan_kernel's clipping of rows to a range, the skipping of workgroups and lanes, the
// wave vote, the atomics and vk_faw_sum_kernel exist only on the GPU: tests/test_gpu_fasta_windows.py.
//
// A stand-alone program:  fasta_windows_emul IN OUT K UNIT_BYTES N S
//   IN:  cases, each a u32 length and the bytes.
//   OUT: per case u32 status, u32 nrec, and per record u64 bases, u32 nwin and per window u32 nnz and nnz pairs (u32
//        code, u32 count) in code order.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define __device__
#define VK_FASTA_LANE_ONLY
#include "vk_fasta_windows.h"

namespace {

typedef std::vector<std::vector<uint32_t>> Rows;

// FawAdd's host twin: the unit's table while in the (record, tile) it belongs to, else the tile's row, else nowhere.
struct HostAdd {
    uint32_t* unit_table;
    std::vector<Rows>* tiles;   // of every record: the tiles its windows need
    uint32_t own_ord;           // kFaNoSlot: the table is not in use
    uint64_t own_tile;
    uint32_t ord = kFaNoSlot;
    bool to_table = false;
    uint32_t* row = nullptr;
    void tile(uint64_t t) {
        to_table = ord == own_ord && t == own_tile;
        row = nullptr;
        if (to_table || ord >= tiles->size()) return;
        if (t < (*tiles)[ord].size()) row = (*tiles)[ord][t].data();
    }
    void enter(uint32_t o, uint64_t t) {
        ord = o;
        tile(t);
    }
    void operator()(uint32_t code, uint32_t n) {
        if (to_table) unit_table[code] += n;
        else if (row) row[code] += n;
    }
};

struct Sample {
    uint32_t status = 0;
    std::vector<uint64_t> bases;
    std::vector<Rows> windows;
};

struct LaneState {
    uint32_t hdr, hb;   // header state at its first byte, header lines that start before it
    uint64_t q;         // ordinal of its first sequence byte in the sample
};

// the passes in front of the count: the state of every lane, and the bases of every record
void index(const uint8_t* text, uint64_t len, std::vector<LaneState>* lanes, std::vector<uint64_t>* bases) {
    uint32_t hdr = 0, hb = 0;
    uint64_t q = 0;
    for (uint64_t c0 = 0; c0 < len; c0 += kFaLaneBytes) {
        const uint32_t n = len - c0 < kFaLaneBytes ? static_cast<uint32_t>(len - c0) : kFaLaneBytes;
        uint32_t w[kFaLaneBytes / 4];
        memset(w, 0xA5, sizeof w);   // (bytes past n are whatever the 16-byte loads bring)
        memcpy(w, text + c0, n);
        const bool first_ls = c0 == 0 || text[c0 - 1] == '\n';
        lanes->push_back(LaneState{hdr, hb, q});
        struct {
            std::vector<uint64_t>* v;
            void header(uint32_t ord, uint32_t) { if (v->size() <= ord) v->resize(ord + 1, 0); }
            void bases(uint32_t ord, uint32_t nb) { if (ord < v->size()) (*v)[ord] += nb; }
        } sink{bases};
        const uint32_t next = c0 + n < len ? text[c0 + n] : '\n';
        far_lane_table(w, n, hdr, first_ls, next, hb, sink);
        q += fa_lane_bases(w, n, hdr, first_ls, next);
        hb += fa_lane_headers(w, n, first_ls);
        const uint32_t lk = fa_lane_key(w, n, first_ls);
        if (lk) hdr = lk & 1u;
    }
}

template <int K>
void run(const uint8_t* text, uint64_t len, uint32_t unit, uint32_t N, uint32_t S, Sample* out) {
    constexpr uint32_t NCODE = 1u << (2 * K);
    const uint32_t m = N / S;
    out->status = len && text[0] != '>' ? 1u : 0u;
    if (out->status || len == 0) return;
    std::vector<LaneState> lanes;
    index(text, len, &lanes, &out->bases);
    const uint32_t nrec = static_cast<uint32_t>(out->bases.size());
    std::vector<uint64_t> ord0(nrec + 1, 0);
    std::vector<Rows> tiles(nrec);
    for (uint32_t r = 0; r < nrec; ++r) {
        ord0[r + 1] = ord0[r] + out->bases[r];
        const uint64_t nwin = out->bases[r] >= N ? (out->bases[r] - N) / S + 1 : 0;
        if (nwin) tiles[r].assign(nwin + m - 1, std::vector<uint32_t>(NCODE, 0u));
    }
    std::vector<uint32_t> unit_table(NCODE);
    const uint32_t per_unit = unit / kFaLaneBytes;
    for (size_t l0 = 0; l0 < lanes.size(); l0 += per_unit) {
        // the (record, tile) that enters the unit
        const LaneState& e = lanes[l0];
        const uint32_t own_ord = e.hb ? e.hb - 1u : 0u;
        FawPos p0;
        p0.start<K>(own_ord < nrec ? e.q - ord0[own_ord] : 0, S);
        const bool table_on = K <= 7 && own_ord < nrec && p0.tile < tiles[own_ord].size();
        if (table_on) std::fill(unit_table.begin(), unit_table.end(), 0u);
        for (size_t l = l0; l < l0 + per_unit && l < lanes.size(); ++l) {
            const uint64_t c0 = static_cast<uint64_t>(l) * kFaLaneBytes;
            const uint32_t n = len - c0 < kFaLaneBytes ? static_cast<uint32_t>(len - c0) : kFaLaneBytes;
            uint32_t w[kFaLaneBytes / 4];
            memset(w, 0xA5, sizeof w);
            memcpy(w, text + c0, n);
            const LaneState& ls = lanes[l];
            FaWalk wk;
            wk.hdr = ls.hdr;
            wk.ls = c0 == 0 || text[c0 - 1] == '\n' ? 1u : 0u;
            HostAdd add{unit_table.data(), &tiles, table_on ? own_ord : kFaNoSlot, p0.tile};
            FawPos ps;
            ps.S = S;
            if (ls.hb) {
                const uint32_t cur = ls.hb - 1u;
                ps.start<K>(cur < nrec ? ls.q - ord0[cur] : 0, S);
                add.enter(cur, ps.tile);
            }
            const uint32_t after = faw_lane_count<K>(w, n, wk, ps, ls.hb, add);
            if (after != (l + 1 < lanes.size() ? lanes[l + 1].hb : nrec)) abort();
            for (uint64_t p = c0 + n; p < len && wk.more<K>(); ++p) faw_step<K>(wk, ps, text[p], false, add);
            wk.flush(add);
        }
        if (table_on)
            for (uint32_t i = 0; i < NCODE; ++i) tiles[own_ord][p0.tile][i] += unit_table[i];
    }
    out->windows.resize(nrec);
    for (uint32_t r = 0; r < nrec; ++r) {
        if (tiles[r].empty()) continue;
        const size_t nwin = tiles[r].size() - (m - 1);
        out->windows[r].assign(nwin, std::vector<uint32_t>(NCODE, 0u));
        for (size_t w = 0; w < nwin; ++w)
            for (uint32_t t = 0; t < m; ++t)
                for (uint32_t c = 0; c < NCODE; ++c) out->windows[r][w][c] += tiles[r][w + t][c];
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 7) {
        fprintf(stderr, "usage: fasta_windows_emul IN OUT K UNIT_BYTES N S\n");
        return 2;
    }
    const int k = atoi(argv[3]);
    const uint32_t unit = static_cast<uint32_t>(strtoul(argv[4], nullptr, 10));
    const uint32_t N = static_cast<uint32_t>(strtoul(argv[5], nullptr, 10)), S = static_cast<uint32_t>(strtoul(argv[6], nullptr, 10));
    if (k < 5 || k > 9 || unit < kFaLaneBytes || unit % kFaLaneBytes || unit > kFaUnitBytes) return 2;
    if (S < static_cast<uint32_t>(k) || N < S || N % S || N / S > kFaMaxSteps) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t len;
    while (fread(&len, 4, 1, in) == 1) {
        std::vector<uint8_t> text(len);   // exactly len bytes: a read past the sample is the sanitizer's to find
        if (len && fread(text.data(), 1, len, in) != len) return 3;
        Sample s;
        switch (k) {
            case 5: run<5>(text.data(), len, unit, N, S, &s); break;
            case 6: run<6>(text.data(), len, unit, N, S, &s); break;
            case 7: run<7>(text.data(), len, unit, N, S, &s); break;
            case 8: run<8>(text.data(), len, unit, N, S, &s); break;
            default: run<9>(text.data(), len, unit, N, S, &s); break;
        }
        const uint32_t nrec = static_cast<uint32_t>(s.bases.size());
        fwrite(&s.status, 4, 1, out);
        fwrite(&nrec, 4, 1, out);
        for (uint32_t r = 0; r < nrec; ++r) {
            const uint32_t nwin = static_cast<uint32_t>(s.windows[r].size());
            fwrite(&s.bases[r], 8, 1, out);
            fwrite(&nwin, 4, 1, out);
            for (uint32_t w = 0; w < nwin; ++w) {
                std::vector<uint32_t> pairs;
                const std::vector<uint32_t>& row = s.windows[r][w];
                for (uint32_t c = 0; c < row.size(); ++c)
                    if (row[c]) {
                        pairs.push_back(c);
                        pairs.push_back(row[c]);
                    }
                const uint32_t nnz = static_cast<uint32_t>(pairs.size() / 2);
                fwrite(&nnz, 4, 1, out);
                if (nnz) fwrite(pairs.data(), 4, pairs.size(), out);
            }
        }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 3;
}
