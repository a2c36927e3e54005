// fasta_records_emul.cpp -- CPU emulation of the lane-local device code of the per-record FASTA count (test only).
//
// Compiles the product's own csrc/vk_fasta_records.h for the host (VK_FASTA_LANE_ONLY: fa_lane_headers, far_lane_table,
// far_lane_count on top of vk_fasta.h's FaWalk, fa_lane_key) and runs a sample the way the kernels cut it: unit after
// unit (a workgroup per unit, as with VKIMG_FASTA_UNIT_BYTES set), lane after lane, each lane with the 64 bytes it would
// have loaded, the header state and header count that enter it, its walk over its own bytes and its read forward past
// them.  For k <= 7 the unit's table stands in for the LDS table: it belongs to the record that enters the unit and is
// added to that record's row at the unit's end, or never used when that record has no slot.
//
// What it does NOT cover: the kernels themselves.  fa_load's bounds, the scans (fa_block_excl_max_sum,
// vk_far_scan_kernel; here a running maximum and a running sum in lane order, which is what they compute), fa_locate,
// the skipping of workgroups, the atomics and the wave vote exist only on the GPU: tests/test_gpu_fasta_records.py.
//
// A stand-alone program:  fasta_records_emul IN OUT K UNIT_BYTES SEL
//   IN:  cases, each a u32 length and the bytes.  SEL: 0 = every record has a slot (its ordinal), 1 = only the records of
//        even ordinal (slot = ordinal / 2).
//   OUT: per case u32 status, u32 nrec, and per record u64 start, u64 bases, u8 name[128], u32 slot, u32 nnz and nnz
//        pairs (u32 code, u32 count) in code order.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define __device__
#define VK_FASTA_LANE_ONLY
#include "vk_fasta_records.h"

namespace {

struct Table {
    const uint8_t* text;
    uint64_t len, c0;
    std::vector<uint64_t>* v_start;
    std::vector<uint64_t>* v_bases;
    std::vector<uint8_t>* v_name;
    void header(uint32_t ord, uint32_t i) {
        if (ord >= v_start->size()) return;
        (*v_start)[ord] = c0 + i;
        uint64_t p = c0 + i + 1;
        for (uint32_t j = 0; j < kFaNameBytes && p < len; ++j, ++p) {
            if (text[p] == '\n') break;
            (*v_name)[static_cast<size_t>(ord) * kFaNameBytes + j] = text[p];
        }
    }
    void bases(uint32_t ord, uint32_t nb) {
        if (ord < v_bases->size()) (*v_bases)[ord] += nb;
    }
};

// FarAdd's host twin: the unit's table while in the record it belongs to, else the record's row, else nowhere.
struct HostAdd {
    uint32_t* unit_table;
    std::vector<std::vector<uint32_t>>* rows;
    const std::vector<uint32_t>* slot;
    uint32_t own;
    bool to_table = false;
    uint32_t* row = nullptr;
    void enter(uint32_t ord) {
        to_table = ord == own;
        row = nullptr;
        if (to_table || ord >= slot->size()) return;
        const uint32_t sl = (*slot)[ord];
        if (sl < rows->size()) row = (*rows)[sl].data();
    }
    void operator()(uint32_t code, uint32_t n) {
        if (to_table) unit_table[code] += n;
        else if (row) row[code] += n;
    }
};

struct Sample {
    uint32_t status = 0;
    std::vector<uint64_t> start, bases;
    std::vector<uint8_t> name;
    std::vector<uint32_t> slot;
    std::vector<std::vector<uint32_t>> rows;
};

// the pass that vk_far_summary_kernel and vk_far_scan_kernel make: the records of the sample
uint32_t count_records(const uint8_t* text, uint64_t len) {
    uint32_t nrec = 0;
    for (uint64_t c0 = 0; c0 < len; c0 += kFaLaneBytes) {
        const uint32_t n = len - c0 < kFaLaneBytes ? static_cast<uint32_t>(len - c0) : kFaLaneBytes;
        uint32_t w[kFaLaneBytes / 4];
        memset(w, 0xA5, sizeof w);   // (bytes past n are whatever the 16-byte loads bring)
        memcpy(w, text + c0, n);
        nrec += fa_lane_headers(w, n, c0 == 0 || text[c0 - 1] == '\n');
    }
    return nrec;
}

template <int K>
void run(const uint8_t* text, uint64_t len, uint32_t unit, int sel, Sample* out) {
    constexpr uint32_t NCODE = 1u << (2 * K);
    out->status = len && text[0] != '>' ? 1u : 0u;
    if (out->status || len == 0) return;
    const uint32_t nrec = count_records(text, len);
    out->start.assign(nrec, 0);
    out->bases.assign(nrec, 0);
    out->name.assign(static_cast<size_t>(nrec) * kFaNameBytes, 0);
    out->slot.assign(nrec, kFaNoSlot);
    uint32_t nslots = 0;
    for (uint32_t r = 0; r < nrec; ++r)
        if (sel == 0 || r % 2 == 0) out->slot[r] = nslots++;
    out->rows.assign(nslots, std::vector<uint32_t>(NCODE, 0u));
    std::vector<uint32_t> unit_table(NCODE);
    uint32_t carry = 0;      // the header state that enters the unit
    uint32_t unit_hb = 0;    // header lines that start before the unit
    for (uint64_t ub = 0; ub < len; ub += unit) {
        const uint32_t own_ord = unit_hb ? unit_hb - 1u : 0u;
        const uint32_t own_slot = own_ord < nrec ? out->slot[own_ord] : kFaNoSlot;
        const bool table_on = K <= 7 && own_slot < nslots;
        if (table_on) std::fill(unit_table.begin(), unit_table.end(), 0u);
        uint32_t excl = 0;   // running maximum of the lanes' keys before this lane
        uint32_t hb = unit_hb;
        for (uint32_t lane = 0; lane * kFaLaneBytes < unit; ++lane) {
            const uint64_t c0 = ub + static_cast<uint64_t>(lane) * kFaLaneBytes;
            if (c0 >= len) break;
            const uint32_t n = len - c0 < kFaLaneBytes ? static_cast<uint32_t>(len - c0) : kFaLaneBytes;
            uint32_t w[kFaLaneBytes / 4];
            memset(w, 0xA5, sizeof w);
            memcpy(w, text + c0, n);
            const bool first_ls = c0 == 0 || text[c0 - 1] == '\n';
            const uint32_t lk = fa_lane_key(w, n, first_ls);
            const uint32_t nh = fa_lane_headers(w, n, first_ls);
            const uint32_t hdr = excl ? excl & 1u : carry;
            // the table
            Table sink{text, len, c0, &out->start, &out->bases, &out->name};
            far_lane_table(w, n, hdr, first_ls, c0 + n < len ? text[c0 + n] : '\n', hb, sink);
            // the count
            FaWalk wk;
            wk.hdr = hdr;
            wk.ls = first_ls ? 1u : 0u;
            HostAdd add{unit_table.data(), &out->rows, &out->slot, table_on ? own_ord : kFaNoSlot};
            if (hb) add.enter(hb - 1u);
            const uint32_t after = far_lane_count<K>(w, n, wk, hb, add);
            if (after != hb + nh) abort();
            for (uint64_t p = c0 + n; p < len && wk.more<K>(); ++p) wk.step<K>(text[p], false, add);
            wk.flush(add);
            hb = after;
            if (lk) excl = ((lane + 1u) << 1) | (lk & 1u);
        }
        if (table_on)
            for (uint32_t i = 0; i < NCODE; ++i) out->rows[own_slot][i] += unit_table[i];
        if (excl) carry = excl & 1u;
        unit_hb = hb;
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 6) {
        fprintf(stderr, "usage: fasta_records_emul IN OUT K UNIT_BYTES SEL\n");
        return 2;
    }
    const int k = atoi(argv[3]), sel = atoi(argv[5]);
    const uint32_t unit = static_cast<uint32_t>(strtoul(argv[4], nullptr, 10));
    if (k < 5 || k > 9 || unit < kFaLaneBytes || unit % kFaLaneBytes || unit > kFaUnitBytes || sel < 0 || sel > 1) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t len;
    while (fread(&len, 4, 1, in) == 1) {
        std::vector<uint8_t> text(len);   // exactly len bytes: a read past the sample is the sanitizer's to find
        if (len && fread(text.data(), 1, len, in) != len) return 3;
        Sample s;
        switch (k) {
            case 5: run<5>(text.data(), len, unit, sel, &s); break;
            case 6: run<6>(text.data(), len, unit, sel, &s); break;
            case 7: run<7>(text.data(), len, unit, sel, &s); break;
            case 8: run<8>(text.data(), len, unit, sel, &s); break;
            default: run<9>(text.data(), len, unit, sel, &s); break;
        }
        const uint32_t nrec = static_cast<uint32_t>(s.start.size());
        fwrite(&s.status, 4, 1, out);
        fwrite(&nrec, 4, 1, out);
        for (uint32_t r = 0; r < nrec; ++r) {
            fwrite(&s.start[r], 8, 1, out);
            fwrite(&s.bases[r], 8, 1, out);
            fwrite(s.name.data() + static_cast<size_t>(r) * kFaNameBytes, 1, kFaNameBytes, out);
            fwrite(&s.slot[r], 4, 1, out);
            std::vector<uint32_t> pairs;
            if (s.slot[r] != kFaNoSlot) {
                const std::vector<uint32_t>& row = s.rows[s.slot[r]];
                for (uint32_t c = 0; c < row.size(); ++c)
                    if (row[c]) {
                        pairs.push_back(c);
                        pairs.push_back(row[c]);
                    }
            }
            const uint32_t nnz = static_cast<uint32_t>(pairs.size() / 2);
            fwrite(&nnz, 4, 1, out);
            if (nnz) fwrite(pairs.data(), 4, pairs.size(), out);
        }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 3;
}
