// textplan_emul.cpp -- the host rules of the calls on record text (csrc/vk_textplan.h) for the CPU suite (test only).
//
// Compiles the product's own header for the host and answers cases, each a flat list of u64 words:
//   1 size   fn, then the size function's arrays -> total, pieces, then per piece in the order the layout states them
//            (offset, bytes).  The pieces' element counts are restated here, so a piece that the header sizes otherwise shows.
//            fn: 0 ladder emit (nsamples, nsteps, lengths, records, step_sample), 1 screen build (length), 2 screen,
//            3 spectrum, 5 depth, 6 qc (nsamples, lengths, records), 4 spectrum from FASTA (nsamples, lengths)
//   2 index  nsamples, offsets, lengths, records -> nchunks, nrec, per sample (off, len, rec0, nrec, chunk0, chunk1),
//            rec_base[nsamples + 1], per file (off, len, nrec, rec0, chunk0), fchunk[nsamples]
//   3 check  call, then its arguments (textplan_emul_lib.py: check_case) -> status, words of block_base, block_base
// The layouts are carved from a heap block of exactly their size, so under the address sanitizer a piece past the total
// would be an error were it touched; every piece's first and last byte is touched.
//
// What it does NOT cover: vkimg.hip's entry points (the null checks, the workspace's size against ws_bytes, the order of
// the runtime calls) and the kernels: tests/test_gpu_text_host_path.py runs those.
//
// A library (tests/textplan_emul_lib.py) and, with -DTEXTPLAN_EMUL_MAIN, a stand-alone program: textplan_emul IN OUT, IN
// cases each led by its word count, OUT the answers each led by theirs.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// what vk_spectrum.h's lane code names from HIP (vk_textplan.h takes constants and plain structs only)
inline unsigned long long atomicCAS(unsigned long long* p, unsigned long long cmp, unsigned long long val) {
    const unsigned long long old = *p;
    if (old == cmp) *p = val;
    return old;
}
inline void sp_add(uint32_t* p, uint32_t n) { *p += n; }
#include "vk_textplan.h"

namespace {

struct In {
    const uint64_t* w;
    uint64_t n, at = 0;
    bool bad = false;
    uint64_t one() {
        if (at >= n) {
            bad = true;
            return 0;
        }
        return w[at++];
    }
    std::vector<uint64_t> many(uint64_t count) {
        if (count > n - at) {
            bad = true;
            return {};
        }
        std::vector<uint64_t> v(w + at, w + at + count);
        at += count;
        return v;
    }
    std::vector<uint32_t> many32(uint64_t count) {
        const std::vector<uint64_t> v = many(count);
        return std::vector<uint32_t>(v.begin(), v.end());
    }
};

struct Pieces {
    uint8_t* base;
    std::vector<uint64_t> out;
    template <class T> void operator()(T* p, uint64_t count) {
        const uint64_t bytes = count * sizeof(T);
        out.push_back(static_cast<uint64_t>(reinterpret_cast<uint8_t*>(p) - base));
        out.push_back(bytes);
        if (bytes) {
            reinterpret_cast<uint8_t*>(p)[0] = 1;
            reinterpret_cast<uint8_t*>(p)[bytes - 1] = 1;
        }
    }
};

uint64_t chunks_of(const std::vector<uint64_t>& lengths) {
    uint64_t n = 0;
    for (uint64_t l : lengths) n += (l + kClChunk - 1) / kClChunk;
    return n;
}

uint64_t sum_of(const std::vector<uint64_t>& v) {
    uint64_t n = 0;
    for (uint64_t x : v) n += x;
    return n;
}

uint64_t scan_blocks(uint64_t items) { return (items + kClScanBlock - 1) / kClScanBlock; }

void index_pieces(Pieces& P, const ClLayout& c, uint64_t n, uint64_t nchunks, uint64_t nrec, uint64_t scanned) {
    P(c.files, n);
    P(c.fchunk, n);
    P(c.ccount, nchunks);
    P(c.cprefix, nchunks + 1);
    P(c.sums, scan_blocks(std::max(nchunks, scanned)) + 1);
    P(c.recs, nrec);
}

void fasta_pieces(Pieces& P, const FaStatePieces& f, const std::vector<uint64_t>& lengths) {
    uint64_t units = 0;
    for (uint64_t l : lengths) units += (l + 63) / 64;
    P(f.meta, 4 * lengths.size() + 2);
    P(f.ukey, units + 1);
    P(f.carry, units + 1);
}

bool size_case(In& in, std::vector<uint64_t>& out) {
    const uint64_t fn = in.one();
    uint64_t length = 0, n = 0, nsteps = 0;
    std::vector<uint64_t> lengths, records;
    std::vector<uint32_t> step_sample;
    if (fn == 1) {
        length = in.one();
    } else {
        n = in.one();
        if (fn == 0) nsteps = in.one();
        lengths = in.many(n);
        if (fn != 4) records = in.many(n);
        if (fn == 0) step_sample = in.many32(nsteps);
    }
    if (in.bad || fn > 6) return false;
    const uint32_t ns = static_cast<uint32_t>(n);
    const uint64_t nchunks = chunks_of(lengths), nrec = sum_of(records);
    // the total first (no base), then the pieces carved from a block of exactly that size
    uint64_t total = 0;
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<uint8_t> block(pass ? std::max<uint64_t>(total, 1) : 0);
        void* ws = pass ? block.data() : nullptr;
        Pieces P{block.data(), {}};
        uint64_t got = 0;
        if (fn == 0) {
            const EmLayout L = em_layout(ws, records.data(), ns, lengths.data(), step_sample.data(), static_cast<uint32_t>(nsteps));
            got = L.total;
            if (pass) {
                uint64_t nitems = 0;
                for (uint32_t s : step_sample) nitems += s < n ? records[s] : 0;
                index_pieces(P, L.c, n, nchunks, nrec, nitems);
                P(L.samples, n), P(L.status, n), P(L.steps, nsteps), P(L.step_base, nsteps + 1), P(L.sizes, nsteps);
                P(L.obytes, nitems), P(L.oprefix, nitems + 1);
            }
        } else if (fn == 1) {
            const ScBuildLayout L = sc_build_layout(ws, length);
            got = L.total;
            if (pass) fasta_pieces(P, L.f, {length}), P(L.out, 1), P(L.status, 1);
        } else if (fn == 2 || fn == 5) {
            const DpLayout D = fn == 5 ? dp_layout(ws, records.data(), ns, lengths.data()) : DpLayout{};
            const ScLayout L = fn == 5 ? D.s : sc_layout(ws, records.data(), ns, lengths.data());
            got = fn == 5 ? D.total : L.total;
            if (pass) {
                index_pieces(P, L.c, n, nchunks, nrec, nrec);
                P(L.samples, n), P(L.rec_base, n + 1), P(L.out_offs, n), P(L.obytes, nrec), P(L.oprefix, nrec + 1);
                if (fn == 5) P(D.slot_base, n), P(D.nslots, n), P(D.lo, n), P(D.hi, n);
            }
        } else if (fn == 3) {
            const SpLayout L = sp_layout(ws, records.data(), ns, lengths.data());
            got = L.total;
            if (pass) {
                index_pieces(P, L.c, n, nchunks, nrec, 0);
                P(L.samples, n), P(L.rec_base, n + 1), P(L.t.block_base, n + 1), P(L.t.slot_base, n), P(L.t.nslots, n);
            }
        } else if (fn == 4) {
            const FsLayout L = fs_layout(ws, lengths.data(), ns);
            got = L.total;
            if (pass) fasta_pieces(P, L.f, lengths), P(L.t.block_base, n + 1), P(L.t.slot_base, n), P(L.t.nslots, n);
        } else {
            const QcLayout L = qc_layout(ws, records.data(), lengths.data(), ns);
            got = L.total;
            if (pass) {
                index_pieces(P, L.c, n, nchunks, nrec, 0);
                P(L.streams, n), P(L.block_base, n + 1), P(L.bad, n);
            }
        }
        if (!pass) {
            total = got;
            continue;
        }
        if (got != total) return false;
        out.push_back(total);
        out.push_back(P.out.size() / 2);
        out.insert(out.end(), P.out.begin(), P.out.end());
    }
    return true;
}

bool index_case(In& in, std::vector<uint64_t>& out) {
    const uint64_t n = in.one();
    const std::vector<uint64_t> offsets = in.many(n), lengths = in.many(n), records = in.many(n);
    if (in.bad) return false;
    const TextIndex t = text_index(offsets.data(), lengths.data(), records.data(), static_cast<uint32_t>(n));
    out.push_back(t.ix.nchunks);
    out.push_back(t.ix.nrec);
    for (const EmSample& s : t.rows) out.insert(out.end(), {s.off, s.len, s.rec0, s.nrec, s.chunk0, s.chunk1});
    out.insert(out.end(), t.rec_base.begin(), t.rec_base.end());
    for (const ClFile& f : t.ix.files) out.insert(out.end(), {f.off, f.len, f.nrec, f.rec0, f.chunk0});
    out.insert(out.end(), t.ix.fchunk.begin(), t.ix.fchunk.end());
    return true;
}

// call: 0 ladder emit, 1 screen build, 2 screen, 3 spectrum, 4 spectrum from FASTA, 5 depth, 6 qc
bool check_case(In& in, std::vector<uint64_t>& out) {
    const uint64_t call = in.one();
    std::vector<uint64_t> block_base;
    int status;
    if (call == 1) {
        const uint64_t length = in.one(), k = in.one(), table = in.one(), nslots = in.one();
        if (in.bad) return false;
        status = screen_build_check(length, static_cast<int>(static_cast<int64_t>(k)), table != 0, nslots);
    } else {
        const uint64_t n = in.one(), k = in.one(), every = in.one(), min_hits = in.one(), cap = in.one(), extra = in.one();
        const std::vector<uint64_t> offsets = in.many(n), lengths = in.many(n), records = in.many(n), nslots = in.many(n),
                                    out_offsets = in.many(n);
        const std::vector<uint32_t> lo = in.many32(n), hi = in.many32(n);
        const uint64_t nsteps = call == 0 ? in.one() : 0;
        const std::vector<uint32_t> step_sample = in.many32(nsteps);
        const std::vector<uint64_t> step_threshold = in.many(nsteps);
        if (in.bad || call > 6) return false;
        TextCall c{};
        c.offsets = offsets.data(), c.lengths = lengths.data(), c.records = call == 4 ? nullptr : records.data();
        c.nsamples = static_cast<uint32_t>(n);
        c.nslots = nslots.data(), c.out_offsets = out_offsets.data(), c.out_capacity = cap, c.lo = lo.data(), c.hi = hi.data();
        c.k = static_cast<int>(static_cast<int64_t>(k)), c.every = static_cast<uint32_t>(every), c.min_hits = static_cast<uint32_t>(min_hits);
        status = call == 0   ? emit_check(c, step_sample.data(), step_threshold.data(), static_cast<uint32_t>(nsteps))
                 : call == 2 ? screen_check(c, extra)
                 : call == 5 ? depth_check(c)
                 : call == 6 ? qc_check(c, static_cast<uint32_t>(extra), &block_base)
                             : spectrum_check(c, &block_base);
    }
    out.push_back(static_cast<uint64_t>(status));
    out.push_back(status ? 0 : block_base.size());
    if (!status) out.insert(out.end(), block_base.begin(), block_base.end());
    return true;
}

int64_t answer(const uint64_t* w, uint64_t n, std::vector<uint64_t>& out) {
    In in{w, n};
    const uint64_t kind = in.one();
    const bool ok = kind == 1 ? size_case(in, out) : kind == 2 ? index_case(in, out) : kind == 3 ? check_case(in, out) : false;
    return ok && !in.bad && in.at == n ? static_cast<int64_t>(out.size()) : -1;
}

}  // namespace

extern "C" int64_t textplan_run(const uint64_t* w, uint64_t n, uint64_t* out, uint64_t cap) {
    std::vector<uint64_t> v;
    const int64_t got = answer(w, n, v);
    if (got < 0 || static_cast<uint64_t>(got) > cap) return -1;
    std::copy(v.begin(), v.end(), out);
    return got;
}

#ifdef TEXTPLAN_EMUL_MAIN
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint64_t> in;
    uint64_t word;
    while (std::fread(&word, 8, 1, f) == 1) in.push_back(word);
    std::fclose(f);
    std::vector<uint64_t> all;
    for (uint64_t at = 0; at < in.size();) {
        const uint64_t n = in[at];
        if (n > in.size() - at - 1) return 3;
        std::vector<uint64_t> v;
        if (answer(in.data() + at + 1, n, v) < 0) return 3;
        all.push_back(v.size());
        all.insert(all.end(), v.begin(), v.end());
        at += 1 + n;
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    if (!all.empty() && std::fwrite(all.data(), 8, all.size(), f) != all.size()) return 2;
    return std::fclose(f) ? 2 : 0;
}
#endif
