// Host build of the inflate's plans (csrc/vk_gzplan.h): chunk size, chunk table, chain walk, member checks, CRC operators.
// The header is plain C++; this file gives it a C ABI for ctypes (tests/gzplan_emul_lib.py) and, with -DGZPLAN_EMUL_MAIN,
// a main() for the sanitizer build.  The walk and the member checks take their case as one flat array of u64 words and
// answer with one, so that the library and the program run the very same code on the very same bytes.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "vk_gzplan.h"

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
    template <class T> std::vector<T> many(uint64_t count) {
        std::vector<T> v;
        if (count > n - at) { ok = false; return v; }
        v.reserve(count);
        for (uint64_t i = 0; i < count; ++i) v.push_back(static_cast<T>(p[at++]));
        return v;
    }
};

void put_checks(std::vector<uint64_t>& out, const GzChecks& ck) {
    out.push_back(ck.jobs.size());
    for (size_t j = 0; j < ck.jobs.size(); ++j) {
        out.push_back(ck.jobs[j].text_off);
        out.push_back(ck.jobs[j].text_len);
        out.push_back(ck.file[j]);
        out.push_back(ck.want[j]);
    }
}

std::vector<GzTrailer> trailers(Words& w, uint64_t count) {
    const std::vector<uint32_t> flat = w.many<uint32_t>(2 * count);
    std::vector<GzTrailer> rec(flat.size() / 2);
    for (size_t i = 0; i < rec.size(); ++i) rec[i] = GzTrailer{flat[2 * i], flat[2 * i + 1]};
    return rec;
}

// 1 | nc | nbig | chunks (7 words each) | chunk0[nbig] | len[nc] | status[nc] | next[nc] | isize[nc] | nmem[nc] |
// records (end, crc) [nc * kGzMemRec] | out_offsets[nbig] | out_caps[nbig]; file b of the call is big file b
bool run_walk(Words& w, std::vector<uint64_t>& out) {
    const uint64_t nc = w.one(), nbig = w.one();
    if (!w.ok || nc > (1u << 20) || nbig > (1u << 20)) return false;
    GzChunkPlan plan;
    for (uint64_t c = 0; c < nc; ++c) {
        const std::vector<uint64_t> f = w.many<uint64_t>(7);
        if (!w.ok) return false;
        plan.chunks.push_back(GzChunk{f[0], f[1], f[2], f[3], static_cast<uint32_t>(f[4]), static_cast<uint32_t>(f[5]), static_cast<uint32_t>(f[6]), 0});
    }
    plan.chunk0 = w.many<uint32_t>(nbig);
    std::vector<unsigned long long> len = w.many<unsigned long long>(nc);
    std::vector<uint32_t> st = w.many<uint32_t>(nc), next = w.many<uint32_t>(nc), isize = w.many<uint32_t>(nc), nmem = w.many<uint32_t>(nc);
    std::vector<GzTrailer> rec = trailers(w, nc * kGzMemRec);
    const std::vector<uint64_t> out_offsets = w.many<uint64_t>(nbig), out_caps = w.many<uint64_t>(nbig);
    if (!w.ok) return false;
    std::vector<uint32_t> big(nbig);
    for (uint32_t b = 0; b < nbig; ++b) big[b] = b;
    const GzChunkResults r{len.data(), st.data(), next.data(), isize.data(), nmem.data(), rec.data()};
    GzChecks ck;
    const GzChains ch = gz_walk_chains(plan, r, big, out_offsets.data(), out_caps.data(), ck);
    for (const GzVerdict& v : ch.verdict) {
        out.push_back(v.kind);
        out.push_back(v.status);
        out.push_back(v.total);
    }
    out.push_back(ch.items.size());
    for (const GzItem& it : ch.items) {
        out.push_back(it.sym_off);
        out.push_back(it.len);
        out.push_back(it.text_off);
    }
    out.push_back(ch.okfile.size());
    for (size_t k = 0; k < ch.okfile.size(); ++k) {
        out.push_back(ch.first[k]);
        out.push_back(ch.count[k]);
        out.push_back(ch.okfile[k]);
    }
    put_checks(out, ck);
    return true;
}

// 2 | file | n | text_off | text_len | (end, crc) [n]
bool run_members(Words& w, std::vector<uint64_t>& out) {
    const uint64_t file = w.one(), n = w.one(), text_off = w.one(), text_len = w.one();
    if (!w.ok || n > (1u << 20)) return false;
    std::vector<GzMember> members;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t end = w.one(), crc = w.one();
        members.push_back(GzMember{end, static_cast<uint32_t>(crc)});
    }
    if (!w.ok) return false;
    GzChecks ck;
    out.push_back(gz_member_checks(ck, static_cast<uint32_t>(file), members, text_off, text_len));
    put_checks(out, ck);
    return true;
}

// 3 | file | status | nmem | text_off | text_len | nrec | (end, crc) [nrec]: the one-wavefront path's file
bool run_direct(Words& w, std::vector<uint64_t>& out) {
    const uint64_t file = w.one(), status = w.one(), nmem = w.one(), text_off = w.one(), text_len = w.one(), nrec = w.one();
    if (!w.ok || nrec > kGzMemRec) return false;
    const std::vector<GzTrailer> rec = trailers(w, nrec);
    if (!w.ok) return false;
    GzChecks ck;
    std::vector<GzMember> members;
    out.push_back(gz_direct_checks(ck, static_cast<uint32_t>(file), static_cast<uint32_t>(status), static_cast<uint32_t>(nmem), rec.data(),
                                   text_off, text_len, members));
    put_checks(out, ck);
    return true;
}

bool run_case(const uint64_t* in, uint64_t nin, std::vector<uint64_t>& out) {
    Words w{in, nin};
    switch (w.one()) {
        case 1: return run_walk(w, out) && w.at == nin;
        case 2: return run_members(w, out) && w.at == nin;
        case 3: return run_direct(w, out) && w.at == nin;
        default: return false;
    }
}

}  // namespace

extern "C" {

uint32_t gzplan_mem_rec() { return kGzMemRec; }
uint32_t gzplan_chunk_min() { return kGzChunkMin; }
uint32_t gzplan_big_file() { return kGzBigFile; }

uint32_t gzplan_fit(const uint64_t* lengths, uint32_t n, uint64_t slots, uint32_t forced, uint32_t fill_pct) {
    std::vector<uint32_t> big(n);
    for (uint32_t i = 0; i < n; ++i) big[i] = i;
    return gz_fit_chunk_bytes(lengths, big, slots, forced, fill_pct);
}

// out: sym_total | nchunks | chunk0[n] | per chunk: in_off in_len out_off out_cap file_chunk0 nchunks chunk_bytes.
// Returns the words written, -1 when `cap` words do not hold them.
int64_t gzplan_table(uint32_t chunk_bytes, const uint64_t* offsets, const uint64_t* lengths, const uint64_t* caps, uint32_t n,
                     uint64_t* out, uint64_t cap) {
    std::vector<uint32_t> big(n);
    for (uint32_t i = 0; i < n; ++i) big[i] = i;
    const GzChunkPlan p = gz_chunk_table(chunk_bytes, offsets, lengths, caps, big);
    std::vector<uint64_t> w{p.sym_total, p.chunks.size()};
    w.insert(w.end(), p.chunk0.begin(), p.chunk0.end());
    for (const GzChunk& c : p.chunks) {
        const uint64_t f[7] = {c.in_off, c.in_len, c.out_off, c.out_cap, c.file_chunk0, c.nchunks, c.chunk_bytes};
        w.insert(w.end(), f, f + 7);
    }
    if (w.size() > cap) return -1;
    for (size_t i = 0; i < w.size(); ++i) out[i] = w[i];
    return static_cast<int64_t>(w.size());
}

// CRC-32 of n zero bytes, the way gz_text_crc finishes a job: the preset shifted over the text, inverted
uint32_t gzplan_crc_zeros(uint64_t n) { return gz_crc_ops().shift(0xFFFFFFFFu, n) ^ 0xFFFFFFFFu; }

// A walk, member or direct case (see run_*): the words of the answer, -1 for a malformed case or too small an `out`.
int64_t gzplan_run(const uint64_t* in, uint64_t nin, uint64_t* out, uint64_t cap) {
    std::vector<uint64_t> w;
    if (!run_case(in, nin, w) || w.size() > cap) return -1;
    for (size_t i = 0; i < w.size(); ++i) out[i] = w[i];
    return static_cast<int64_t>(w.size());
}

}  // extern "C"

#ifdef GZPLAN_EMUL_MAIN
// gzplan_emul_san CASES ANSWERS: CASES holds cases as (count, words...), ANSWERS receives (count, words...) for each.
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
