// Host build of the BAM calls' host rules (csrc/vk_bamplan.h): the argument rules, the framing's plan, a grouped call's
// sizes, pieces and descriptor block, the result rules -- and the product's probe (csrc/vk_bam_groups.h's bam_probe) over
// the tables the block holds.  The header is plain C++; this file gives it a C ABI for ctypes (tests/bamplan_emul_lib.py)
// and, with -DBAMPLAN_EMUL_MAIN, a main() for the sanitizer build.  A case is one flat array of u64 words and is answered
// with one, so that the library and the program run the very same code on the very same bytes.  Every array a rule reads
// lies in a heap block of exactly its size: under the address sanitizer a read past one is an error.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "vk_bamplan.h"

namespace {

// the words of a case, read in order; `ok` goes false on a read past the end
struct Words {
    const uint64_t* p;
    uint64_t n, at = 0;
    bool ok = true;
    uint64_t one() {
        if (at >= n) { ok = false; return 0; }
        return p[at++];
    }
    // `count` words as a heap block of exactly that many T
    template <class T> std::unique_ptr<T[]> many(uint64_t count) {
        if (count > n - at) { ok = false; count = 0; }
        std::unique_ptr<T[]> v(new T[count]);
        for (uint64_t i = 0; i < count; ++i) v[i] = static_cast<T>(p[at++]);
        return v;
    }
};

template <class T>
std::unique_ptr<T[]> exact(const T* v, size_t n) {   // a heap block of exactly n elements
    std::unique_ptr<T[]> p(new T[n]);
    for (size_t i = 0; i < n; ++i) p[i] = v[i];
    return p;
}

// A call: nfiles | nstreams | flags | grouped | text | lengths[nfiles] | stream_file[ns] | stream_select[ns] |
// grouped: stream_group[ns] | group_first[nfiles + 1] | nid | id_first[nid] | nbytes | the ID bytes, a word each |
// text: out_offsets[ns] | out_caps[ns].  offsets, first_record and n_ref are zeros: no rule reads their values.
struct Case {
    BamCall c{};
    std::unique_ptr<uint64_t[]> offsets, lengths, first, out_offsets, out_caps;
    std::unique_ptr<int32_t[]> n_ref;
    std::unique_ptr<uint32_t[]> stream_file, stream_select, stream_group, group_first, id_first;
    std::unique_ptr<uint8_t[]> id_bytes;
    uint64_t nid = 0, nbytes = 0;
};

bool read_call(Words& w, Case& k) {
    BamCall& c = k.c;
    c.nfiles = static_cast<uint32_t>(w.one());
    c.nstreams = static_cast<uint32_t>(w.one());
    c.flags = static_cast<uint32_t>(w.one());
    c.grouped = w.one() != 0;
    c.text = w.one() != 0;
    if (!w.ok || c.nfiles > (1u << 16) || c.nstreams > (1u << 16)) return false;
    k.offsets.reset(new uint64_t[c.nfiles]());
    k.first.reset(new uint64_t[c.nfiles]());
    k.n_ref.reset(new int32_t[c.nfiles]());
    k.lengths = w.many<uint64_t>(c.nfiles);
    k.stream_file = w.many<uint32_t>(c.nstreams);
    k.stream_select = w.many<uint32_t>(c.nstreams);
    c.offsets = k.offsets.get();
    c.lengths = k.lengths.get();
    c.first_record = k.first.get();
    c.n_ref = k.n_ref.get();
    c.stream_file = k.stream_file.get();
    c.stream_select = k.stream_select.get();
    if (c.grouped) {
        k.stream_group = w.many<uint32_t>(c.nstreams);
        k.group_first = w.many<uint32_t>(c.nfiles + 1ull);
        k.nid = w.one();
        k.id_first = w.many<uint32_t>(k.nid);
        k.nbytes = w.one();
        k.id_bytes = w.many<uint8_t>(k.nbytes);
        c.stream_group = k.stream_group.get();
        c.group_first = k.group_first.get();
        c.id_first = k.id_first.get();
        c.id_bytes = k.id_bytes.get();
    }
    if (c.text) {
        k.out_offsets = w.many<uint64_t>(c.nstreams);
        k.out_caps = w.many<uint64_t>(c.nstreams);
        c.out_offsets = k.out_offsets.get();
        c.out_caps = k.out_caps.get();
    }
    return w.ok;
}

template <class T>
void put(std::vector<uint64_t>& out, const T* v, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) out.push_back(v[i]);
}

// 1 | call  ->  bam_args_ok | bg_args_ok (0 for a call that is not grouped, or that bam_args_ok refuses)
bool run_args(Words& w, std::vector<uint64_t>& out) {
    Case k;
    if (!read_call(w, k)) return false;
    const bool ok = bam_args_ok(k.c);
    out.push_back(ok);
    out.push_back(ok && k.c.grouped && bg_args_ok(k.c));
    return true;
}

// 2 | seg_bytes | call (one the rules accept)  ->  ok | seg | streams of the framing | segs | stream_segs |
// seg_first[nfiles + 1] | sseg_first[streams + 1] | out_offs[streams] | out_caps[streams]
bool run_plan(Words& w, std::vector<uint64_t>& out) {
    const uint32_t seg_bytes = static_cast<uint32_t>(w.one());
    Case k;
    if (!read_call(w, k) || !bam_args_ok(k.c)) return false;
    const BamPlan p = bam_plan(k.c, seg_bytes);
    if (p.seg_first.size() != k.c.nfiles + 1ull || p.sseg_first.size() != p.nstreams + 1ull || p.out_offs.size() != p.nstreams ||
        p.out_caps.size() != p.nstreams)
        return false;
    const uint64_t head[5] = {p.ok, p.seg, p.nstreams, p.segs, p.stream_segs};
    put(out, head, 5);
    put(out, p.seg_first.data(), p.seg_first.size());
    put(out, p.sseg_first.data(), p.sseg_first.size());
    put(out, p.out_offs.data(), p.nstreams);
    put(out, p.out_caps.data(), p.nstreams);
    return true;
}

// 3 | seg | panel | call (grouped, one the rules accept) | nq | per query: file, n, n bytes (a word each)  ->
// workspace bytes | desc_bytes | back_bytes | the 15 pieces of the block in bg_take's order, each: offset, count, values |
// per query: bam_probe's answer over the file's table, its pieces copied out of the block
bool run_describe(Words& w, std::vector<uint64_t>& out) {
    const uint32_t seg = static_cast<uint32_t>(w.one()), panel = static_cast<uint32_t>(w.one());
    Case k;
    if (!read_call(w, k) || seg < 64 || panel < 1 || !k.c.grouped || !bam_args_ok(k.c) || !bg_args_ok(k.c)) return false;
    const BamCall& c = k.c;
    const BgCounts n = bg_counts(c, seg, panel);
    std::vector<uint8_t> host;
    const BgPieces h = bg_describe(c, n, host);
    if (host.size() != h.desc_bytes) return false;
    out.push_back(bg_workspace_bytes(c, seg, panel));
    out.push_back(h.desc_bytes);
    out.push_back(h.back_bytes);
    const auto piece = [&](const auto* v, uint64_t count) {
        out.push_back(static_cast<uint64_t>(reinterpret_cast<const uint8_t*>(v) - host.data()));
        out.push_back(count);
        const auto x = exact(v, count);
        put(out, x.get(), count);
    };
    const uint64_t nf = c.nfiles, ns = c.nstreams;
    piece(h.ids, n.id_bytes);
    piece(h.group_first, nf + 1);
    piece(h.id_first, n.groups + 1);
    piece(h.slots, n.slots);
    piece(h.slot_first, nf);
    piece(h.map_first, nf);
    piece(h.ls_first, nf + 1);
    piece(h.ls_stream, ns);
    piece(h.stream_file, ns);
    piece(h.stream_local, ns);
    piece(h.map, n.map);
    piece(h.pan_first, nf + 1);
    piece(h.row_first, nf);
    piece(h.out_offs, ns);
    piece(h.out_caps, ns);
    const uint64_t nq = w.one();
    for (uint64_t q = 0; q < nq && w.ok; ++q) {
        const uint64_t f = w.one(), len = w.one();
        const auto v = w.many<uint8_t>(len);
        if (!w.ok || f >= nf) return false;
        // the file's table as bam_table_of hands it to the lanes
        const uint32_t g0 = h.group_first[f], ng = h.group_first[f + 1] - g0, nslots = bam_table_slots(ng);
        const auto x_ids = exact(h.ids, n.id_bytes);
        const auto x_first = exact(h.id_first + g0, ng + 1ull);
        const auto x_slots = exact(h.slots + h.slot_first[f], nslots);
        const BamGroupTable T{x_ids.get(), x_first.get(), x_slots.get(), nslots - 1, ng};
        uint32_t hash = kBamHashSeed;
        for (uint64_t i = 0; i < len; ++i) hash = bam_hash_step(hash, v[i]);
        out.push_back(bam_probe(T, v.get(), static_cast<uint32_t>(len), hash));
    }
    return w.ok;
}

// 4 | 0 | v[3] | select -> bam_host_pick;  4 | 1 | a file's status | its aux_bad -> bam_status_of;
// 4 | 2 | n | cap -> fits | length (bam_slot_fits)
bool run_result(Words& w, std::vector<uint64_t>& out) {
    switch (w.one()) {
        case 0: {
            const auto v = w.many<uint64_t>(3);
            const uint32_t select = static_cast<uint32_t>(w.one());
            if (!w.ok || select > kBamSingle) return false;
            out.push_back(bam_host_pick(v.get(), select));
            return true;
        }
        case 1: {
            const uint32_t status = static_cast<uint32_t>(w.one()), bad = static_cast<uint32_t>(w.one());
            out.push_back(bam_status_of(status, bad));
            return w.ok;
        }
        case 2: {
            const uint64_t n = w.one(), cap = w.one();
            uint64_t length = ~0ull;
            out.push_back(bam_slot_fits(n, cap, &length));
            out.push_back(length);
            return w.ok;
        }
        default: return false;
    }
}

bool run_case(const uint64_t* in, uint64_t nin, std::vector<uint64_t>& out) {
    Words w{in, nin};
    switch (w.one()) {
        case 1: return run_args(w, out) && w.at == nin;
        case 2: return run_plan(w, out) && w.at == nin;
        case 3: return run_describe(w, out) && w.at == nin;
        case 4: return run_result(w, out) && w.at == nin;
        default: return false;
    }
}

}  // namespace

extern "C" {

// A case (see run_*): the words of the answer, -1 for a malformed case or too small an `out`.
int64_t bamplan_run(const uint64_t* in, uint64_t nin, uint64_t* out, uint64_t cap) {
    std::vector<uint64_t> w;
    if (!run_case(in, nin, w) || w.size() > cap) return -1;
    for (size_t i = 0; i < w.size(); ++i) out[i] = w[i];
    return static_cast<int64_t>(w.size());
}

}  // extern "C"

#ifdef BAMPLAN_EMUL_MAIN
// bamplan_emul_san CASES ANSWERS: CASES holds cases as (count, words...), ANSWERS receives (count, words...) for each.
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 2;
    uint64_t n = 0;
    while (fread(&n, 8, 1, f) == 1) {
        if (n > (1u << 24)) return 3;
        std::vector<uint64_t> in(n);   // (sized exactly: a read past the case is a read past the allocation)
        if (n && fread(in.data(), 8, n, f) != n) return 3;
        std::vector<uint64_t> out;
        if (!run_case(in.data(), n, out)) return 4;
        const uint64_t m = out.size();
        fwrite(&m, 8, 1, g);
        if (m) fwrite(out.data(), 8, m, g);
    }
    fclose(f);
    return fclose(g) == 0 ? 0 : 5;
}
#endif
