// vk_gzplan.h -- the host's side of the gzip inflate (vk_inflate.h): the plain structs host and device share, and the
// decisions vk_inflate_device takes on what the kernels report -- how large a chunk is, which chunks a file is cut into,
// whether a file's chain of chunks is sound, which stretches of text get which check word.  They run on untrusted input and
// are plain functions of a few integer arrays: no HIP here, so that a host compiler and a CPU test reach them
// (tests/emul/gzplan_emul.cpp).
#ifndef VK_GZPLAN_H
#define VK_GZPLAN_H

#include <cstddef>
#include <cstdint>
#include <vector>

namespace {

// status bits of one gzip file
constexpr uint32_t kGzBadHeader = 1u, kGzBadData = 2u, kGzTruncated = 4u, kGzOverflow = 8u, kGzBadSize = 16u, kGzBadCrc = 32u;

struct GzJob {
    uint64_t in_off, in_len;     // compressed bytes in the input buffer
    uint64_t out_off, out_cap;   // where the text goes, and how much room there is
};

// A CHUNK of a large gzip file (the chunked path, below): one wavefront decodes the DEFLATE blocks
// from the block start `start_bit` (found by vk_gzfind_kernel; chunk 0: the gzip header at bit 0)
// up to the block start of a later chunk.
struct GzChunk {
    uint64_t in_off, in_len;     // the whole FILE's compressed bytes
    uint64_t out_off, out_cap;   // this chunk's u16 elements in the symbolic buffer (offset and room, in elements)
    uint32_t file_chunk0;        // index of the file's chunk 0 in the chunk arrays
    uint32_t nchunks;            // chunks of the file
    uint32_t chunk_bytes;        // compressed bytes per chunk (chosen per call, vk_inflate_device)
    uint32_t pad_;
};
constexpr uint64_t kGzNone = ~0ull;       // start_bit of a chunk in which no block start was found
constexpr uint64_t kGzPending = 0xFEFEFEFEFEFEFEFEull;   // ... of a chunk whose wavefront has not looked yet (the host's memset; vk_gzchunk_kernel)
constexpr uint32_t kGzEnd = 0xFFFFFFFFu;  // next[] of the chunk that decoded the file's last member
constexpr uint32_t kGzMemRec = 62;         // member trailers a wavefront records (end of the member's text in ITS output, CRC-32 word); a file with more in one chunk goes unchecked

constexpr uint32_t kGzChunkMin = 1u << 17;                            // compressed bytes per chunk: this, or twice this
constexpr uint32_t kGzBigFile = 1u << 19;                             // files at least this large are cut into chunks

// items: {chunk's element offset, its length}; first/count: the file's slice of them (vk_gzwin_kernel, vk_gzfinal_kernel).
struct GzItem {
    uint64_t sym_off, len, text_off;
};

struct GzCrcJob {
    uint64_t text_off, text_len;
    uint32_t seg0, nseg;  // this file's slice of the segment array
};

// A member trailer as a wavefront records it (the kernels' uint2: cast at the launch).
struct GzTrailer {
    uint32_t end, crc;   // end of the member's text in the wavefront's own output, CRC-32 word
};
static_assert(sizeof(GzTrailer) == 8, "a member record is the kernels' uint2");

// Operators of the CRC-32 (reflected polynomial 0xEDB88320) over GF(2), as zlib's crc32_combine builds them:
// op[k] advances a remainder over 2^k zero BYTES; 32 columns each.
struct GzCrcOps {
    uint32_t op[34][32];  // [33]: 4032 bytes, the step between a lane's pieces in vk_crc32_seg_kernel
    GzCrcOps() {
        uint32_t bit1[32], bit2[32], bit4[32];
        bit1[0] = 0xEDB88320u;  // one zero bit
        for (int n = 1; n < 32; ++n) bit1[n] = 1u << (n - 1);
        square(bit2, bit1);
        square(bit4, bit2);
        square(op[0], bit4);  // eight zero bits
        for (int k = 1; k <= 32; ++k) square(op[k], op[k - 1]);
        for (int n = 0; n < 32; ++n) op[33][n] = shift(1u << n, 4032);
    }
    static uint32_t times(const uint32_t* m, uint32_t v) {
        uint32_t r = 0;
        for (int i = 0; v; v >>= 1, ++i)
            if (v & 1u) r ^= m[i];
        return r;
    }
    static void square(uint32_t* sq, const uint32_t* m) {
        for (int n = 0; n < 32; ++n) sq[n] = times(m, m[n]);
    }
    uint32_t shift(uint32_t v, uint64_t nbytes) const {
        for (int k = 0; nbytes; nbytes >>= 1, ++k)
            if (nbytes & 1u) v = times(op[k], v);
        return v;
    }
};
inline const GzCrcOps& gz_crc_ops() {
    static const GzCrcOps ops;
    return ops;
}

// ---- the chunked path's plan: chunk size and chunk table ---------------------------------------------
// `big` names the files of a call that are cut into chunks (indices into the call's arrays), `slots` is the number of
// wavefronts of vk_gzchunk_kernel the device holds at a time (CUs x kGzChunkWaves, vk_inflate.h).

// Chunk size: 128 KiB gives a small call the most wavefronts (8 files of 24 MB: 48 ms against 72 ms with
// 256 KiB); once there are more chunks than the device holds wavefronts, throughput no longer
// depends on it (measured flat from 128 to 320 KiB) and 256 KiB halves the per-chunk work of the finder.
// Round 6: the chunk decoder's wavefronts are all resident from the start when there are no more of them than the device
// holds (slots), and a launch of 1.26 rounds is the worst there is (64 files of 24 MB, level 1: 96.9 ms at 192 KiB = 1.26
// rounds, 88.0 at 128 KiB = 1.9, 80.9 at 256 KiB = 0.95, 86.4 at 320 KiB = 0.76): the size is fitted so that the chunks
// fill 0.99 of the slots a whole number of times, the fewest times that keep a chunk under 352 KiB -- by the exact count
// (every file's length is known), so that a SIMD holds six wavefronts or, here and there, five: at 0.96 a quarter of the
// SIMDs held five and were done a sixth early (64 files of 33 MB: 113.5 ms at 0.96, 102.1 at 0.99 and at 1.00; 0.90: 115.9).
// forced: VKIMG_GZ_CHUNK_BYTES (0 = fitted); fill_pct: VKIMG_GZ_FILL (0 = 99).
inline uint32_t gz_fit_chunk_bytes(const uint64_t* gz_lengths, const std::vector<uint32_t>& big, uint64_t slots, uint32_t forced,
                                   uint32_t fill_pct) {
    uint32_t chunk_bytes = forced;
    if (chunk_bytes == 0) {
        uint64_t big_total = 0;
        for (uint32_t i : big) big_total += gz_lengths[i];
        chunk_bytes = kGzChunkMin;
        if (big_total / kGzChunkMin > slots) {
            for (uint64_t rounds = 1; rounds <= 64; ++rounds) {
                // (every file ends in a part of a chunk: half a chunk per file goes off the count)
                const double fill = fill_pct ? 0.01 * fill_pct : 0.99;
                const double want = fill * static_cast<double>(slots * rounds) - 0.5 * static_cast<double>(big.size());
                if (want < 1.0) continue;
                uint64_t cb = (static_cast<uint64_t>(static_cast<double>(big_total) / want) + 4095u) & ~4095ull;
                if (cb < kGzChunkMin) cb = kGzChunkMin;
                // (the count is known exactly: never one chunk more than the rounds hold)
                for (;;) {
                    uint64_t count = 0;
                    for (uint32_t i : big) count += (gz_lengths[i] + cb - 1) / cb;
                    if (count <= static_cast<uint64_t>(fill * static_cast<double>(slots * rounds)) || cb > 352u * 1024u) break;
                    cb += 4096;
                }
                if (cb <= 352u * 1024u) {
                    chunk_bytes = cb < kGzChunkMin ? kGzChunkMin : static_cast<uint32_t>(cb);
                    break;
                }
                chunk_bytes = 2 * kGzChunkMin;   // (never reached by a sane input: a thousand rounds)
            }
        }
    }
    if (chunk_bytes < 65536u) chunk_bytes = 65536u;
    return chunk_bytes;
}

struct GzChunkPlan {
    std::vector<GzChunk> chunks;    // of every file of `big`, file after file
    std::vector<uint32_t> chunk0;   // per file of `big`: its first chunk
    uint64_t sym_total = 0;         // u16 elements of all chunks together
};

inline GzChunkPlan gz_chunk_table(uint32_t chunk_bytes, const uint64_t* gz_offsets, const uint64_t* gz_lengths, const uint64_t* out_caps,
                                  const std::vector<uint32_t>& big) {
    GzChunkPlan p;
    p.chunk0.resize(big.size());
    for (size_t b = 0; b < big.size(); ++b) {
        const uint32_t i = big[b];
        const uint32_t nch = static_cast<uint32_t>((gz_lengths[i] + chunk_bytes - 1) / chunk_bytes);
        // room per chunk (u16 elements): twice what the file's overall ratio predicts for a chunk, at least 8x
        double ratio = static_cast<double>(out_caps[i]) / static_cast<double>(gz_lengths[i]);
        if (ratio < 4.0) ratio = 4.0;
        uint64_t cap = static_cast<uint64_t>(2.0 * ratio * chunk_bytes) + 65536;
        if (cap > (1ull << 25)) cap = 1ull << 25;
        p.chunk0[b] = static_cast<uint32_t>(p.chunks.size());
        for (uint32_t j = 0; j < nch; ++j) {
            p.chunks.push_back(GzChunk{gz_offsets[i], gz_lengths[i], p.sym_total, cap, p.chunk0[b], nch, chunk_bytes, 0});
            p.sym_total += cap;
        }
    }
    return p;
}

// ---- member checks -----------------------------------------------------------------------------------
struct GzMember {
    uint64_t end;   // end of the member's text in the file's text
    uint32_t crc;   // the CRC-32 word of its trailer
};

// one job per gzip member with text: its CRC-32 is checked against the member's trailer
struct GzChecks {
    std::vector<GzCrcJob> jobs;
    std::vector<uint32_t> file, want;   // per job: the file it belongs to, the check word it must have
};

// every member of file `file` (text at text_off, text_len bytes; `members` in order) gets a check of its own;
// an empty member's check word must be that of no bytes.  Returns the status bits the list itself earns the file.
inline uint32_t gz_member_checks(GzChecks& ck, uint32_t file, const std::vector<GzMember>& members, uint64_t text_off, uint64_t text_len) {
    uint32_t bits = 0;
    uint64_t from = 0;
    for (const GzMember& mb : members) {
        if (mb.end < from || mb.end > text_len) return bits;  // (cannot happen for a file whose sizes added up)
        if (mb.end == from) {
            if (mb.crc != 0u) bits |= kGzBadCrc;
        } else {
            ck.jobs.push_back(GzCrcJob{text_off + from, mb.end - from, 0, 0});
            ck.file.push_back(file);
            ck.want.push_back(mb.crc);
        }
        from = mb.end;
    }
    return bits;
}

// The one-wavefront path: a file's members are checked when it inflated without a fault, every trailer is on record and
// the text is below 4 GiB (the records' ends are 32-bit).  The chunked path has no such bound on the length: a chunk's
// records are relative to the chunk, and its files are checked at any size.
inline uint32_t gz_direct_checks(GzChecks& ck, uint32_t file, uint32_t status, uint32_t nmem, const GzTrailer* rec, uint64_t text_off,
                                 uint64_t text_len, std::vector<GzMember>& members) {
    if (status != 0 || nmem < 1 || nmem > kGzMemRec || text_len >= (1ull << 32)) return 0;
    members.clear();
    for (uint32_t r = 0; r < nmem; ++r) members.push_back({rec[r].end, rec[r].crc});
    return gz_member_checks(ck, file, members, text_off, text_len);
}

// ---- the chain walk ----------------------------------------------------------------------------------
// What vk_gzchunk_kernel reports per chunk, as host arrays (kGzMemRec records per chunk).
struct GzChunkResults {
    unsigned long long* len;   // u16 elements (= bytes of text) the chunk decoded
    uint32_t* status;
    uint32_t* next;            // the chunk whose start this one decoded up to, kGzEnd behind the file's last member
    uint32_t* isize;           // sum of the size words of the members that ended here
    uint32_t* nmem;            // members that ended here
    GzTrailer* rec;
};

constexpr uint32_t kGzInflated = 0;    // the chain is sound and the text fits: `total` bytes
constexpr uint32_t kGzTooLarge = 1;    // the chain is sound and the text does not fit: it needs `total` bytes
constexpr uint32_t kGzGoDirect = 2;    // anything odd: the file goes through the one-wavefront kernel
struct GzVerdict {
    uint32_t kind, status;   // status: the file's status word (kGzGoDirect: none yet)
    uint64_t total;
};

struct GzChains {
    std::vector<GzVerdict> verdict;              // per file of `big`
    std::vector<GzItem> items;                   // the accepted files' chunks in chain order
    std::vector<uint32_t> first, count, okfile;  // per accepted file: its slice of items, the file
};

// The chain of the file whose chunks begin at c0 and whose text goes to text_off (room: out_cap): its items are appended
// (and taken back unless it is accepted), `members` holds its trailers, *checkable says whether every one is on record.
inline GzVerdict gz_walk_file(const GzChunk* chunks, uint32_t c0, const GzChunkResults& r, uint64_t text_off, uint64_t out_cap,
                              std::vector<GzItem>& items, std::vector<GzMember>& members, bool* checkable) {
    const size_t mark = items.size();
    uint64_t total = 0;
    uint32_t isum = 0, nmem = 0;
    bool ok = true;
    uint32_t c = c0;
    members.clear();
    bool members_known = true;   // every trailer's (end of text, check word) on record?
    for (;;) {
        if (r.status[c] != 0) { ok = false; break; }
        items.push_back(GzItem{chunks[c].out_off, r.len[c], text_off + total});
        if (r.nmem[c] > kGzMemRec) members_known = false;
        for (uint32_t k = 0; k < r.nmem[c] && k < kGzMemRec; ++k) {
            const GzTrailer rec = r.rec[static_cast<size_t>(c) * kGzMemRec + k];
            members.push_back({total + rec.end, rec.crc});
        }
        total += r.len[c];
        isum += r.isize[c];
        nmem += r.nmem[c];
        const uint32_t nx = r.next[c];
        if (nx == kGzEnd) break;
        if (nx <= c || nx >= c0 + chunks[c].nchunks) { ok = false; break; }
        c = nx;
    }
    if (ok && isum != static_cast<uint32_t>(total)) ok = false;  // the members' size words do not add up to the text
    if (ok && total > out_cap) {  // e.g. several members and a caller who knew only the last one's size
        items.resize(mark);
        return GzVerdict{kGzTooLarge, kGzOverflow, total};   // ... who now learns the size a second call needs
    }
    if (!ok) {
        items.resize(mark);
        return GzVerdict{kGzGoDirect, 0, 0};
    }
    *checkable = members_known && members.size() == nmem;
    return GzVerdict{kGzInflated, 0, total};
}

// follow every file's chain of chunks; a file with anything odd in it goes the direct way instead
inline GzChains gz_walk_chains(const GzChunkPlan& plan, const GzChunkResults& r, const std::vector<uint32_t>& big,
                               const uint64_t* out_offsets, const uint64_t* out_caps, GzChecks& ck) {
    GzChains ch;
    ch.verdict.resize(big.size());
    std::vector<GzMember> members;
    for (size_t b = 0; b < big.size(); ++b) {
        const uint32_t i = big[b];
        const size_t mark = ch.items.size();
        bool checkable = false;
        GzVerdict& v = ch.verdict[b];
        v = gz_walk_file(plan.chunks.data(), plan.chunk0[b], r, out_offsets[i], out_caps[i], ch.items, members, &checkable);
        if (v.kind != kGzInflated) continue;
        ch.first.push_back(static_cast<uint32_t>(mark));
        ch.count.push_back(static_cast<uint32_t>(ch.items.size() - mark));
        ch.okfile.push_back(i);
        if (checkable) v.status |= gz_member_checks(ck, i, members, out_offsets[i], v.total);
    }
    return ch;
}

}  // namespace

#endif  // VK_GZPLAN_H
