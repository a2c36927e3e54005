// bam_groups_emul.cpp -- CPU emulation of the lane-local device code of the read-group split of BAM files (test only).
//
// Compiles the product's own csrc/vk_bam.h and csrc/vk_bam_groups.h for the host (VK_BAM_LANE_ONLY: bam_aux_fixed,
// bam_aux_elem, bam_group_of, bam_probe, bam_hash_step, bam_table_slots, bam_map_at, bam_note_of on top of vk_bam.h's
// bam_read, bam_walk, bam_class, bam_emit_item ...) and runs a file the way the kernels cut it.  The framing is the link
// pass's result -- every segment walked from its true entry, its starts noted -- and then, as the three kernels do: the
// count pass takes panel after panel, notes every record's stream beside its start and fills the panel's row; the scan
// turns the rows into the places where a panel's reads begin; the emit pass takes a panel's records 64 at a time, places
// each read at its stream's cursor plus the sizes of the earlier lanes of the same stream, lets the last lane of every
// stream move the cursor on, and writes item by item.  The hash table and the map are the product's: csrc/vk_bamplan.h's
// bg_describe builds them, and the pieces the lanes read are copied out of its block.  The file, the ID bytes, the hash table, the map, every segment's
// starts and notes and every text lie in heap blocks of exactly their size: under the address sanitizer a byte read past
// the file (an aux length followed without a check), a probe past the table or a byte written past a text is an error.
//
// What it does NOT cover: the kernels themselves -- the LDS tables and their atomics, the shuffles of the placement, the
// search of an item's record, the split of a workgroup's threads over records and items: tests/test_gpu_bam_groups.py.
//
// A stand-alone program:  bam_groups_emul IN OUT SEG_BYTES PANEL_SEGS EXCLUDE
//   IN:  cases, each u32 length, u64 first_record, u32 groups, per group u32 length and the ID, u32 streams, per stream u32
//        select and u32 group, then the file's bytes.
//   OUT: per case u32 status, u64 records, a u16 note per record (the stream's index, 0xFFFF: none), u64 records walked,
//        u64 panels, then per stream a u64 length and the text.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#define __device__
#define __host__
#define VK_BAM_LANE_ONLY
#include "vk_bam.h"
#include "vk_bam_groups.h"
#include "vk_bamplan.h"

namespace {

struct Stream {
    uint32_t select, group;
};

struct Result {
    uint32_t status = 0;
    std::vector<uint16_t> notes;
    uint64_t walked = 0, panels = 0;
    std::vector<std::vector<uint8_t>> text;
};

template <class T>
std::unique_ptr<T[]> exact(const T* v, size_t n) {   // a heap block of exactly n elements
    std::unique_ptr<T[]> p(new T[n]);
    for (size_t i = 0; i < n; ++i) p[i] = v[i];
    return p;
}

Result convert(const uint8_t* p, uint64_t len, uint64_t first, const std::vector<std::vector<uint8_t>>& ids,
               const std::vector<Stream>& streams, uint64_t seg_bytes, uint64_t panel, uint32_t exclude) {
    Result res;
    res.text.resize(streams.size());
    uint64_t nseg = (len + seg_bytes - 1) / seg_bytes;
    if (nseg == 0) nseg = 1;
    const uint32_t cap = bam_starts_cap(static_cast<uint32_t>(seg_bytes));
    // the framing, as the link pass leaves it
    std::vector<std::unique_ptr<uint16_t[]>> starts(nseg), notes(nseg);
    std::vector<uint32_t> nrec(nseg, 0);
    uint64_t truth = first;
    uint32_t status = 0;
    for (uint64_t j = 0; j < nseg && !status; ++j) {
        starts[j].reset(new uint16_t[cap]);
        notes[j].reset(new uint16_t[cap]);
        const uint64_t end = (j + 1) * seg_bytes < len ? (j + 1) * seg_bytes : len;
        if (truth < end) {
            BamTally t;
            status = bam_walk(p, len, truth, end, exclude, &t, &truth, j * seg_bytes, starts[j].get(), cap, &nrec[j]);
        }
    }
    if (!status && truth != len) status = kBamTruncated;
    res.status = status;
    if (status) return res;
    // the tables: the host layer's own (bg_describe), as a call with this one file makes them
    const uint32_t ng = static_cast<uint32_t>(ids.size()), nslots = bam_table_slots(ng);
    std::vector<uint8_t> id_bytes;
    std::vector<uint32_t> id_first(1, 0), stream_file(streams.size(), 0), select, group;
    for (const auto& id : ids) {
        id_bytes.insert(id_bytes.end(), id.begin(), id.end());
        id_first.push_back(static_cast<uint32_t>(id_bytes.size()));
    }
    for (const Stream& s : streams) {
        select.push_back(s.select);
        group.push_back(s.group);
    }
    const uint32_t group_first[2] = {0, ng};
    BamCall c{};
    c.lengths = &len;
    c.nfiles = 1;
    c.group_first = group_first;
    c.id_first = id_first.data();
    c.id_bytes = id_bytes.data();
    c.stream_file = stream_file.data();
    c.stream_select = select.data();
    c.stream_group = group.data();
    c.nstreams = static_cast<uint32_t>(streams.size());
    c.grouped = true;
    std::vector<uint8_t> desc;
    const BgPieces h = bg_describe(c, bg_counts(c, static_cast<uint32_t>(seg_bytes), static_cast<uint32_t>(panel)), desc);
    const auto x_ids = exact(h.ids, id_bytes.size());
    const auto x_first = exact(h.id_first, ng + 1);
    const auto x_slots = exact(h.slots, nslots);
    const auto x_map = exact(h.map, 3 * (ng + 1));
    const BamGroupTable T{x_ids.get(), x_first.get(), x_slots.get(), nslots - 1, ng};
    // count pass: a row per panel
    const uint64_t npan = (nseg + panel - 1) / panel;
    const size_t nls = streams.size();
    std::vector<uint64_t> row_recs(npan * nls, 0), row_bytes(npan * nls, 0);
    uint32_t bad = 0;
    for (uint64_t j = 0; j < nseg; ++j)
        for (uint32_t i = 0; i < nrec[j]; ++i) {
            BamRec r;
            uint16_t note = kBamNoStream;
            if (bam_read(p, len, j * seg_bytes + starts[j][i], &r) == 0) {
                const uint32_t cls = bam_class(r, exclude);
                if (cls) {
                    note = bam_note_of(p, r, cls, T, x_map.get(), &bad);
                    ++res.walked;
                    if (note != kBamNoStream) {
                        row_recs[(j / panel) * nls + note] += 1;
                        row_bytes[(j / panel) * nls + note] += bam_text_size(r);
                    }
                }
            }
            notes[j][i] = note;
            res.notes.push_back(note);
        }
    res.panels = npan;
    if (bad) {
        res.status = kBamBadAux;
        res.notes.clear();
        return res;
    }
    // scan: a panel's entry becomes where its reads begin
    std::vector<uint64_t> total(nls, 0);
    for (size_t s = 0; s < nls; ++s)
        for (uint64_t q = 0; q < npan; ++q) {
            const uint64_t here = row_bytes[q * nls + s];
            row_bytes[q * nls + s] = total[s];
            total[s] += here;
        }
    std::vector<std::vector<uint8_t>> written(nls);
    for (size_t s = 0; s < nls; ++s) {
        res.text[s].assign(total[s], 0xEE);
        written[s].assign(total[s], 0);
    }
    // emit pass: panels in any order (here: the last first), the records of a panel 64 at a time
    for (uint64_t q = npan; q-- > 0;) {
        std::vector<uint64_t> cursor(row_bytes.begin() + q * nls, row_bytes.begin() + (q + 1) * nls);
        for (uint64_t j = q * panel; j < nseg && j < (q + 1) * panel; ++j)
            for (uint32_t r0 = 0; r0 < nrec[j]; r0 += 64) {
                uint32_t note[64];
                uint64_t size[64], at[64];
                BamRec rec[64];
                for (uint32_t l = 0; l < 64; ++l) {
                    note[l] = kBamNoStream;
                    size[l] = 0;
                    if (r0 + l < nrec[j] && notes[j][r0 + l] != kBamNoStream && bam_read(p, len, j * seg_bytes + starts[j][r0 + l], &rec[l]) == 0) {
                        note[l] = notes[j][r0 + l];
                        size[l] = bam_text_size(rec[l]);
                    }
                }
                for (uint32_t l = 0; l < 64; ++l) {   // (every lane reads the cursors before any moves one)
                    uint64_t before = 0;
                    for (uint32_t k = 0; k < l; ++k)
                        if (note[k] == note[l]) before += size[k];
                    at[l] = note[l] != kBamNoStream ? cursor[note[l]] + before : 0;
                }
                for (uint32_t l = 0; l < 64; ++l) {
                    bool last = true;
                    for (uint32_t k = l + 1; k < 64; ++k)
                        if (note[k] == note[l]) last = false;
                    if (note[l] != kBamNoStream && last) cursor[note[l]] = at[l] + size[l];
                }
                for (uint32_t l = 0; l < 64; ++l) {
                    if (note[l] == kBamNoStream) continue;
                    std::vector<uint8_t>& out = res.text[note[l]];
                    if (at[l] + size[l] > out.size()) {
                        fprintf(stderr, "a read past its stream's text\n");
                        exit(3);
                    }
                    const BamEmit e = bam_emit_of(p, rec[l]);
                    uint8_t* dst = out.data() + at[l];
                    for (uint64_t it = bam_items(dst, size[l]); it-- > 0;) bam_emit_item(e, dst, size[l], it);
                    for (uint64_t i = 0; i < size[l]; ++i) ++written[note[l]][at[l] + i];
                }
            }
    }
    for (const auto& w : written)
        for (uint8_t c : w)
            if (c != 1) {
                fprintf(stderr, "a text byte written %u times\n", c);
                exit(3);
            }
    return res;
}

bool get(FILE* in, void* dst, size_t n) { return fread(dst, 1, n, in) == n; }

}  // namespace

int main(int argc, char** argv) {
    if (argc != 6) {
        fprintf(stderr, "usage: bam_groups_emul IN OUT SEG_BYTES PANEL_SEGS EXCLUDE\n");
        return 2;
    }
    const uint64_t seg_bytes = strtoull(argv[3], nullptr, 10), panel = strtoull(argv[4], nullptr, 10);
    const uint32_t exclude = static_cast<uint32_t>(strtoul(argv[5], nullptr, 0));
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out || seg_bytes < 64 || seg_bytes > kBamSegBytes || panel < 1) return 2;
    for (;;) {
        uint32_t len, ng, ns;
        uint64_t first;
        if (!get(in, &len, 4)) break;
        if (!get(in, &first, 8) || !get(in, &ng, 4)) return 2;
        std::vector<std::vector<uint8_t>> ids(ng);
        for (auto& id : ids) {
            uint32_t n;
            if (!get(in, &n, 4)) return 2;
            id.resize(n);
            if (n && !get(in, id.data(), n)) return 2;
        }
        if (!get(in, &ns, 4)) return 2;
        std::vector<Stream> streams(ns);
        if (ns && !get(in, streams.data(), ns * sizeof(Stream))) return 2;
        uint8_t* data = static_cast<uint8_t*>(malloc(len ? len : 1));   // exactly the file: nothing behind it may be read
        if (len && !get(in, data, len)) return 2;
        const Result r = convert(data, len, first, ids, streams, seg_bytes, panel, exclude);
        const uint64_t nnotes = r.notes.size();
        fwrite(&r.status, 4, 1, out);
        fwrite(&nnotes, 8, 1, out);
        if (nnotes) fwrite(r.notes.data(), 2, nnotes, out);
        fwrite(&r.walked, 8, 1, out);
        fwrite(&r.panels, 8, 1, out);
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
