// faplan_emul.cpp -- the host rules of the FASTA calls (csrc/vk_faplan.h) for the CPU suite (test only).
//
// Compiles the product's own header for the host and answers cases, each a flat list of u64 words:
//   1 clamp   env -> fa_unit_clamp(env)
//   2 plan    override, nsamples, offsets, lengths -> status, unit, span, nwg, nunits, words of meta, meta (a refused plan:
//             the status alone)
//   3 pairs   override, nsamples, offsets, lengths, npairs, pair_sample, seeds, thresholds, shifts -> status of the pair
//             plan (the samples' plan must hold), pair_nwg, words of the table, the table, then the FaPairs view with
//             frag_len 77: the five arrays' byte offsets from the table's start, npairs, frag_len
//   4 first   nsamples, rec_first[nsamples + 1] -> far_rec_first_ok
//   5 check   call, then its arguments (faplan_emul_lib.py: check_case) -> status, stage, steps, sum_wgs.  The rules in
//             the order the entry point applies them, and how far the call came: stage 0 refused by the call's rules (the
//             *_check function), 1 by the offsets or the sum's grid behind d_fasta (the two per-row counting calls), 2 by
//             the plan or the pair plan, 3 accepted.  The two per-row counting calls have reset d_hist when they reach
//             stage 2.
//   6 layout  fn, override, nsamples, lengths, npairs, total, steps, tile_rows, k -> total bytes, pieces, then per piece in
//             the order the layout states them (offset, bytes).  fn: 0 count, 1 sampled, 2 records, 3 windows (the plan's
//             units), 4 the header state of a caller's workspace (a unit per lane).  The pieces' element counts are
//             restated here, so a piece that the header sizes otherwise shows.
// The layouts are carved from a heap block of exactly their size, so under the address sanitizer a piece past the total
// would be an error were it touched; every piece's first and last byte is touched.
//
// What it does NOT cover: vkimg.hip's entry points (the null checks, d_fasta's alignment, the order of the runtime calls)
// and the kernels: tests/test_gpu_fasta_host_path.py runs those.
//
// A library (tests/faplan_emul_lib.py) and, with -DFAPLAN_EMUL_MAIN, a stand-alone program: faplan_emul IN OUT, IN cases
// each led by its word count, OUT the answers each led by theirs.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vk_faplan.h"

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

bool plan_case(In& in, std::vector<uint64_t>& out) {
    const uint64_t override = in.one(), n = in.one();
    const std::vector<uint64_t> offsets = in.many(n), lengths = in.many(n);
    if (in.bad) return false;
    FaPlan pl;
    const int status = fa_plan(static_cast<uint32_t>(override), offsets.data(), lengths.data(), static_cast<uint32_t>(n), &pl);
    out.push_back(static_cast<uint64_t>(status));
    if (status) return true;
    if (pl.wg_first() != pl.meta.data() + 2 * n) return false;
    out.insert(out.end(), {pl.unit, pl.span, pl.nwg, pl.nunits, pl.meta.size()});
    out.insert(out.end(), pl.meta.begin(), pl.meta.end());
    return true;
}

bool pairs_case(In& in, std::vector<uint64_t>& out) {
    const uint64_t override = in.one(), n = in.one();
    const std::vector<uint64_t> offsets = in.many(n), lengths = in.many(n);
    const uint64_t npairs = in.one();
    const std::vector<uint32_t> pair_sample = in.many32(npairs);
    const std::vector<uint64_t> seeds = in.many(npairs), thresholds = in.many(npairs), shifts = in.many(npairs);
    if (in.bad) return false;
    FaCall c{};
    c.offsets = offsets.data(), c.lengths = lengths.data(), c.nsamples = static_cast<uint32_t>(n), c.k = 5, c.frag_len = 77;
    c.npairs = static_cast<uint32_t>(npairs), c.pair_sample = pair_sample.data(), c.seeds = seeds.data();
    c.thresholds = thresholds.data(), c.shifts = shifts.data();
    FaPlan pl;
    if (count_fasta_sampled_check(c) || fa_plan(static_cast<uint32_t>(override), c.offsets, c.lengths, c.nsamples, &pl)) return false;
    FaPairPlan pp;
    const int status = fa_pair_plan(c, pl, &pp);
    out.insert(out.end(), {static_cast<uint64_t>(status), pp.pair_nwg, pp.words.size()});
    out.insert(out.end(), pp.words.begin(), pp.words.end());
    const std::vector<uint64_t> dev(pp.words.size());
    const FaPairs v = pp.pairs_on_device(dev.data(), c.frag_len);
    for (const uint64_t* p : {v.sample, v.seed, v.threshold, v.shift, v.wg_first}) out.push_back(8ull * (p - dev.data()));
    out.insert(out.end(), {v.npairs, v.frag_len});
    return true;
}

bool first_case(In& in, std::vector<uint64_t>& out) {
    const uint64_t n = in.one();
    const std::vector<uint64_t> rec_first = in.many(n + 1);
    if (in.bad) return false;
    out.push_back(far_rec_first_ok(rec_first.data(), static_cast<uint32_t>(n)) ? 1 : 0);
    return true;
}

// call: 0 count, 1 sampled, 2 records count, 3 records, 4 count records, 5 count windows
bool check_case(In& in, std::vector<uint64_t>& out) {
    const uint64_t call = in.one(), override = in.one(), n = in.one(), k = in.one();
    const std::vector<uint64_t> offsets = in.many(n), lengths = in.many(n), rec_first = in.many(n + 1);
    const uint64_t nslots = in.one(), npairs = in.one();
    const std::vector<uint32_t> pair_sample = in.many32(npairs);
    const std::vector<uint64_t> seeds = in.many(npairs), thresholds = in.many(npairs), shifts = in.many(npairs);
    const uint64_t frag_len = in.one(), win_len = in.one(), win_step = in.one(), nrows = in.one(), tile_rows = in.one();
    if (in.bad || call > 5) return false;
    FaCall c{};
    c.offsets = offsets.data(), c.lengths = lengths.data(), c.nsamples = static_cast<uint32_t>(n);
    c.k = static_cast<int>(static_cast<int64_t>(k)), c.rec_first = rec_first.data(), c.nslots = static_cast<uint32_t>(nslots);
    c.npairs = static_cast<uint32_t>(npairs), c.pair_sample = pair_sample.data(), c.seeds = seeds.data();
    c.thresholds = thresholds.data(), c.shifts = shifts.data(), c.frag_len = static_cast<uint32_t>(frag_len);
    c.win_len = static_cast<uint32_t>(win_len), c.win_step = static_cast<uint32_t>(win_step);
    c.nrows = static_cast<uint32_t>(nrows), c.tile_rows = static_cast<uint32_t>(tile_rows);
    uint32_t steps = 0;
    uint64_t sum_wgs = 0, stage = 0;
    int status = call == 0   ? count_fasta_check(c)
                 : call == 1 ? count_fasta_sampled_check(c)
                 : call == 2 ? fasta_records_count_check(c)
                 : call == 3 ? fasta_records_check(c)
                 : call == 4 ? count_fasta_records_check(c)
                             : count_fasta_windows_check(c, &steps);
    if (!status && call >= 4) {
        stage = 1;
        if (!fa_offsets_ok(c.offsets, c.nsamples)) status = VK_EINVAL;
        if (!status && call == 5) status = faw_sum_check(c, steps, &sum_wgs);
    }
    // (the four calls that write nothing answer VK_OK to no sample here; the two others make no plan without a record)
    const bool planned = call < 4 ? n != 0 : n != 0 && rec_first[n] != 0;
    if (!status && planned) {
        stage = 2;
        FaPlan pl;
        FaPairPlan pp;
        status = fa_plan(static_cast<uint32_t>(override), c.offsets, c.lengths, c.nsamples, &pl);
        if (!status && call == 1) status = fa_pair_plan(c, pl, &pp);
    }
    if (!status) stage = 3;
    out.insert(out.end(), {static_cast<uint64_t>(status), stage, steps, sum_wgs});
    return true;
}

bool layout_case(In& in, std::vector<uint64_t>& out) {
    const uint64_t fn = in.one(), override = in.one(), n = in.one();
    const std::vector<uint64_t> lengths = in.many(n);
    const uint64_t npairs = in.one(), total_recs = in.one(), steps = in.one(), tile_rows = in.one(), k = in.one();
    if (in.bad || fn > 4 || k < 5 || k > 9) return false;
    const uint32_t ns = static_cast<uint32_t>(n);
    const std::vector<uint64_t> offsets(n, 0);
    FaPlan pl;
    if (fa_plan(static_cast<uint32_t>(override), offsets.data(), lengths.data(), ns, &pl)) return false;
    // the units and the lanes restated: a unit is the override's bytes or 16,384, a lane 64
    const uint64_t unit = override ? override : 16384;
    uint64_t units = 0, lane_units = 0;
    for (uint64_t l : lengths) units += (l + unit - 1) / unit, lane_units += (l + 63) / 64;
    const uint64_t lane_words = units * (unit / 64) + 1;
    // the total first (no base), then the pieces carved from a block of exactly that size
    uint64_t total = 0;
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<uint8_t> block(pass ? std::max<uint64_t>(total, 1) : 0);
        WsTake take{pass ? block.data() : nullptr, 0};
        Pieces P{block.data(), {}};
        if (fn == 0 || fn == 4) {
            FaStatePieces f{};
            if (fn == 0) fa_state_take(take, f, ns, pl.nunits);
            else fa_state_take(take, f, lengths.data(), ns);
            const uint64_t u = fn == 0 ? units : lane_units;
            if (pass) P(f.meta, 4 * n + 2), P(f.ukey, u + 1), P(f.carry, u + 1);
        } else if (fn == 1) {
            FaSampledPieces p{};
            fa_sampled_take(take, p, pl, static_cast<uint32_t>(npairs));
            if (pass) {
                P(p.f.meta, 4 * n + 2), P(p.pairs, 5 * npairs + 1), P(p.f.ukey, units + 1), P(p.f.carry, units + 1);
                P(p.unit_ord, units + 1), P(p.lane, lane_words);
            }
        } else if (fn == 2) {
            FarPieces p{};
            far_take(take, p, pl);
            if (pass) {
                P(p.meta, 4 * n + 2), P(p.rec_first, n + 1), P(p.ukey, units + 1), P(p.carry, units + 1), P(p.uhdr, units + 1);
                P(p.status, n), P(p.nrec, n);
            }
        } else {
            FawPieces p{};
            faw_take(take, p, pl, total_recs, static_cast<uint32_t>(steps), static_cast<uint32_t>(tile_rows), static_cast<int>(k));
            if (pass) {
                P(p.lane, lane_words), P(p.unit_ord, units + 1), P(p.bases, n), P(p.recs, total_recs + 1), P(p.used, 1);
                P(p.tiles, steps > 1 ? tile_rows << (2 * k) : 1);
            }
        }
        if (!pass) {
            total = take.at;
            continue;
        }
        if (take.at != total) return false;
        out.push_back(total);
        out.push_back(P.out.size() / 2);
        out.insert(out.end(), P.out.begin(), P.out.end());
    }
    return true;
}

int64_t answer(const uint64_t* w, uint64_t n, std::vector<uint64_t>& out) {
    In in{w, n};
    const uint64_t kind = in.one();
    bool ok = false;
    if (kind == 1) {
        out.push_back(fa_unit_clamp(static_cast<uint32_t>(in.one())));
        ok = true;
    } else if (kind >= 2 && kind <= 6) {
        ok = kind == 2 ? plan_case(in, out) : kind == 3 ? pairs_case(in, out) : kind == 4 ? first_case(in, out)
             : kind == 5 ? check_case(in, out) : layout_case(in, out);
    }
    return ok && !in.bad && in.at == n ? static_cast<int64_t>(out.size()) : -1;
}

}  // namespace

extern "C" int64_t faplan_run(const uint64_t* w, uint64_t n, uint64_t* out, uint64_t cap) {
    std::vector<uint64_t> v;
    const int64_t got = answer(w, n, v);
    if (got < 0 || static_cast<uint64_t>(got) > cap) return -1;
    std::copy(v.begin(), v.end(), out);
    return got;
}

#ifdef FAPLAN_EMUL_MAIN
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
