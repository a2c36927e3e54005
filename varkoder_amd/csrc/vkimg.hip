// vkimg.hip -- HIP kernels (gfx950 / CDNA4) and the C ABI of include/vkimg.h.
//
// Hot path of varKoder's `image` command (reference: varKoder/commands/image.py
// count_kmers :727-806 -> dsk, make_image :808-936 -> dsk2ascii + pandas/NumPy):
//
//   K1  vk_count_kernel   FASTQ text in HBM -> forward-strand k-mer histogram u32[4^k]
//   K1c vk_check_kernel   line-phase consistency of the byte ranges -> status word
//   K2  vk_image_kernel   strand merge + pixel scatter (count+1) + sort + 256-quantile
//                         rank binning -> uint8 image
//   vk_synth_kernel       synthetic FASTQ generator of BASELINE.md section 4
//
// The kernels live in vk_count.h (K1), vk_image.h (K2) and vk_aux.h, included below.
// Design notes live in DESIGN.md; the short version for K1:
//   * one 1024-thread workgroup per (sample, byte-range part);
//     its 16 wavefronts run WITHOUT workgroup barriers in steady state: every
//     wave streams its own contiguous byte range in 4 KiB pieces (every lane loads its
//     own 64 contiguous bytes, four 16-B loads, prefetched one piece ahead)
//     and classifies them with 32-bit SWAR arithmetic (vk_lane.h);
//   * FASTQ line phase (header/sequence/plus/quality) comes from a wave-level
//     prefix sum of newline counts; the phase at a range start is recovered
//     locally from the '@' / '+' framing, so byte ranges are independent;
//   * k-mer windows are counted forward-strand only into an LDS histogram
//     (ds_add_u32); the strand merge happens once per sample in K2;
//   * 4^k u32 > LDS for k = 8, 9: QUADS of neighbouring windows are bucketed through workgroup-shared LDS
//     queues into 256 streams per sample in HBM (half a byte per window) and replayed into LDS tables
//     (vk_bucket_kernel<K, 3>, vk_quad_count_kernel, vk_quad_merge_kernel); subsampled launches: pairs of
//     windows through wave-private queues into 16 streams (vk_bucket_kernel<K, 1>, vk_bucket_count_kernel).
//   vk_remap_kernel / vk_preprocess_kernel: `convert`'s remap and the input side of `query`.
//   vk_fa_*_kernel (vk_fasta.h): the count straight from FASTA text (`--from-fasta`): cut by bytes, header state by a scan.
//   vk_far_*_kernel (vk_fasta_records.h): the same per FASTA record (`--per-record`): record ordinal by a second scan.
//   vk_faw_*_kernel (vk_fasta_windows.h): the same per window of a record (`--windows`): tiles by start, summed to windows.
//   vk_bam_*_kernel (vk_bam.h): BAM records to FASTQ text (`--from-bam`): record starts guessed per segment, verified in order.
//   vk_bam_groups_*_kernel (vk_bam_groups.h): the same split by read group (`--bam-read-groups`): one emit workgroup per panel.
//   vk_dist_*_kernel (vk_dist.h): exact distances between images and nearest neighbours (`compare`): centred i8 rows, tiles on the i8 matrix cores, a workgroup's selection per row.
//   vk_qc_*_kernel (vk_qc.h): quality profiles of FASTQ streams (`--qc-report`): wave per record, lanes on cycles, counters in LDS merged per workgroup.
//   vk_sp_*_kernel (vk_spectrum.h): the k-mer spectrum of cleaned reads (`--kmer-spectrum`): wave per record, scattered atomics into a counting table in HBM, its histogram.
//   vk_fs_count_kernel (vk_fasta_spectrum.h): the k-mer spectrum of assemblies (`--genome-spectrum`): the same tables filled straight from FASTA text, lane per 64 bytes, windows rolled from registers.
//   vk_sk_*_kernel (vk_sketch.h): bottom-s MinHash sketches from the spectrum's tables (`--spectrum-sketch`: radix select, compaction, LDS runs, merge path) and all pairs of sketches compared (`distance`: a wavefront per pair).
//   vk_tr_*_kernel (vk_tree.h): neighbour-joining trees of a batch of distance matrices (`tree`): per step a search of the upper triangle by tiles and strips, then a workgroup per tree that joins.
//   vk_sc_*_kernel (vk_screen.h): reads screened against a reference's k-mer set (`--exclude-fasta`, `--keep-fasta`): wave per record, probes of a table in HBM.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "vkimg.h"
#include "vk_lane.h"
#include "vk_ws.h"

#include "vk_count.h"
#include "vk_pack.h"
#include "vk_countplan.h"
#include "vk_ladder.h"
#include "vk_image.h"
#include "vk_inflate.h"
#include "vk_aux.h"
#include "vk_train.h"
#include "vk_clean.h"
#include "vk_adapter.h"
#include "vk_emit.h"
#include "vk_deflate.h"
#include "vk_png.h"
#include "vk_unpng.h"
#include "vk_fasta.h"
#include "vk_fasta_ladder.h"
#include "vk_fasta_records.h"
#include "vk_fasta_windows.h"
#include "vk_faplan.h"
#include "vk_bam.h"
#include "vk_bam_groups.h"
#include "vk_bamplan.h"
#include "vk_screen.h"
#include "vk_spectrum.h"
#include "vk_fasta_spectrum.h"
#include "vk_sketch.h"
#include "vk_depth.h"
#include "vk_qc.h"
#include "vk_textplan.h"
#include "vk_dist.h"
#include "vk_tree.h"

// ---------------------------------------------------------------- C ABI ------

struct vk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipError_t last = hipSuccess;
    uint32_t* d_pix[10] = {};
    uint32_t npix[10] = {};
    // workspaces (grown on demand, never inside a timed launch after warm-up)
    uint64_t* d_desc = nullptr;   // offsets | lengths
    size_t desc_cap = 0;
    uint64_t* h_desc = nullptr;   // pinned mirror of d_desc (descriptor cache): the copy uploaded last
    size_t h_desc_cap = 0;
    uint64_t* h_desc_alt = nullptr;  // the other of the two mirrors: a batch with new descriptors is staged here
    size_t h_desc_alt_cap = 0;       // while the previous batch's copy may still be reading h_desc
    hipEvent_t desc_ev = nullptr, desc_ev_alt = nullptr;  // recorded behind the copy out of each mirror
    uint32_t desc_n = 0;
    uint32_t* d_wavephase = nullptr;
    size_t wavephase_cap = 0;
    // read index of a batch (vk_read_index_device): anchors | sample bases | segment counts | sites | overflow flags
    uint8_t* d_index = nullptr;
    size_t index_cap = 0;
    IndexParams ix{};
    const void* ix_fastq = nullptr;
    uint32_t ix_parts = 0;
    std::map<std::pair<uint64_t, uint64_t>, uint32_t> ix_sample;   // (offset, length) -> sample of the index
    std::vector<uint32_t> ix_status, ix_overflow;                  // per indexed sample (host copies)
    uint32_t* d_walk = nullptr;   // per-pair arrays of a walker launch
    size_t walk_cap = 0;
    uint32_t* d_aside = nullptr;  // k <= 7: the waves' lists of lanes set aside
    size_t aside_cap = 0;
    uint32_t* d_scratch = nullptr;
    size_t scratch_cap = 0;
    uint32_t* d_spill = nullptr;  // k >= 8: bucket cursors + bucket streams
    size_t spill_cap = 0;
    size_t spill_budget = 96ull << 30;  // bytes of HBM the spill path may use at a time (VKIMG_SPILL_BUDGET=n: tests force several sub-batches)
    // host-call staging
    uint64_t* d_sub = nullptr;    // subsampling launches: seeds | thresholds
    uint8_t* d_gzjobs = nullptr;  // vk_inflate_device: jobs | check words | what the kernel reports (gz_direct_stage)
    size_t gzjobs_cap = 0;
    uint8_t* d_gzmeta = nullptr;  // ... chunked path: chunk table and results, then the chain items
    size_t gzmeta_cap = 0;
    uint8_t* d_gzsym = nullptr;   // ... u16 elements of every chunk
    size_t gzsym_cap = 0;
    uint8_t* d_gzwin = nullptr;   // ... the 32 KiB window every chunk of a chain starts with
    size_t gzwin_cap = 0;
    uint8_t* d_gzcrc = nullptr;   // ... CRC-32 jobs, operators, segment values
    size_t gzcrc_cap = 0;
    bool gz_no_chunks = false;    // VKIMG_GZ_NO_CHUNKS=1: every file through the one-wavefront kernel (tests, A/B timing)
    uint32_t gz_chunk_bytes = 0;  // VKIMG_GZ_CHUNK_BYTES: fixed chunk size of the chunked inflate (0 = fitted to the device)
    bool gz_split_find = false;   // VKIMG_GZ_SPLIT_FIND=1: the chunks' block starts by a launch of its own (vk_gzfind_kernel; rounds 2-5) instead of by the chunk decoder's wavefronts themselves (tests, A/B timing)
    uint32_t gz_fill_pct = 0;     // VKIMG_GZ_FILL: per cent of the device's chunk-wavefront slots a round of chunks is fitted to (0 = 99; A/B timing)
    uint32_t gz_lds_pad = 0;      // VKIMG_GZ_LDS_PAD: bytes of LDS a chunk wavefront asks for on top of its own (A/B timing: fewer wavefronts per CU)
    int num_cus = 256;
    size_t sub_cap = 0;
    uint8_t* d_stage = nullptr;
    size_t stage_cap = 0;
    uint32_t* d_synth = nullptr;       // vk_synth_shaped_*: record offsets of a slab of samples
    size_t synth_cap = 0;
    uint64_t* d_synth_offs = nullptr;  // ... and the slab's sample offsets
    size_t synth_offs_cap = 0;
    uint32_t* d_hist1 = nullptr;
    uint32_t* d_status1 = nullptr;
    size_t status1_cap = 0;
    uint8_t* d_img1 = nullptr;
    uint32_t last_grid = 0, last_block = 0, last_lds = 0;
    uint64_t last_waves = 0, last_bytes = 0;   // of the last count call: wave slots in d_wavephase, FASTQ bytes
    bool image_sort_only = false;  // VKIMG_IMAGE_SORT_ONLY=1: always take the sort kernel (tests, A/B timing)
    uint32_t spill_misc_cap = 0;   // VKIMG_SPILL_MISC_CAP=n: log2 of the entries per (workgroup, bucket) region of the quad route's listed quads (tests)
    uint32_t spill_runs_cap = 0;   // VKIMG_SPILL_RUNS_CAP=n: runs per sample arena of the k = 8, 9 path (tests)
    bool spill_packed = false;     // VKIMG_SPILL_PACKED=1: k = 8, 9 pass A in two kernels, vk_pack_kernel + the partition of the packed stream (measured slower than the one kernel that classifies every byte: 21.1 against 16.3 ms per 100 samples; tests, A/B timing)
    bool spill_pairs = false;      // VKIMG_SPILL_PAIRS=1: a plain k = 8, 9 count through the pair route of rounds 1-4 (u16 per two windows, wave-private queues; what subsampled and packed launches still use) instead of the quad route (tests, A/B timing)
    bool spill_force_wide = false; // VKIMG_SPILL_FORCE_WIDE=1: every k = 8, 9 replay job through the u32 window counters (tests)
    uint8_t* d_clines = nullptr;   // vk_clean_lines_device: files | chunk bases | line counters (vk_clean_heads_device: see there)
    size_t clines_cap = 0;
    uint8_t* d_cladapt = nullptr;  // vk_clean_adapters_device: the adapter table (ClAdapter per sample and group)
    size_t cladapt_cap = 0;
    uint8_t* d_cldetect = nullptr; // vk_clean_detect_device: a slice's seed occurrences and their states
    size_t cldetect_cap = 0;
    uint32_t clean_hash_bits = 64; // VKIMG_CLEAN_HASH_BITS=n: vk_clean_device's dedup keeps n bits of its 64-bit hash (tests: collisions on purpose)
    bool no_read_index = false;    // VKIMG_NO_READ_INDEX=1: subsampled counts always stream the text, whatever index the context holds (tests, A/B timing)
    uint8_t* d_fasta = nullptr;    // vk_count_fasta_device: descriptors | unit summaries | the state that enters every unit
    size_t fasta_cap = 0;
    uint8_t* d_fawin = nullptr;    // vk_count_fasta_windows_device: ordinal index | record table | tile rows (beside d_fasta, which far_prepare carves)
    size_t fawin_cap = 0;
    uint32_t fasta_unit_bytes = 0; // VKIMG_FASTA_UNIT_BYTES=n: bytes of a unit of the FASTA count, a multiple of 64 up to 16384, one unit per workgroup (tests: many seams in little text; 0 = 16384, 32 units per workgroup)
    uint8_t* d_bamws = nullptr;    // vk_bam_frame_device, vk_bam_fastq_device: descriptors | segments | per-file results | link counters
    size_t bamws_cap = 0;
    uint32_t bam_seg_bytes = 0;    // VKIMG_BAM_SEG_BYTES=n: bytes of a segment of the BAM framing, 64 .. 65536 (tests: many seams in little data; 0 = 65536)
    uint64_t bam_segments = 0, bam_rewalked = 0;   // of the last of those calls (vk_last_bam_frame)
    uint8_t* d_bamgws = nullptr;   // vk_bam_groups_frame_device, vk_bam_groups_fastq_device: what vk_bam_groups_workspace_size states (beside d_bamws)
    size_t bamgws_cap = 0;
    uint32_t bam_panel_segs = 0;   // VKIMG_BAM_PANEL_SEGS=n: segments of a panel of the grouped BAM calls, 1 .. 4096 (tests: many panels in little data; 0 = 4)
    uint64_t bam_groups_wgs = 0, bam_groups_walked = 0;   // of the last of those calls (vk_last_bam_groups)
    uint32_t qc_merge = 0;         // VKIMG_QC_MERGE=n: records per workgroup of the QC count kernel, 1 to VK_QC_MERGE (tests: many merges in small cases; 0 = VK_QC_MERGE)
    uint32_t dist_strip = 0;       // VKIMG_DIST_STRIP=n: query rows of a strip of vk_dist_device, from 1 up to what the workspace holds (tests: strip seams in small inputs; 0 = what the workspace holds)
    uint32_t screen_tile = 0;      // VKIMG_SCREEN_TILE=n: bases of a wavefront's tile of the screen's match kernel, a multiple of 64 from 64 to 4096 (tests: tile seams in short reads; 0 = 4096)
    uint32_t spectrum_tile = 0;    // VKIMG_SPECTRUM_TILE=n: the same for the spectrum's count kernel
    uint32_t spectrum_merge = kSpMergeDefault;   // VKIMG_SPECTRUM_MERGE=0|1|2: how the count kernel merges equal keys of a wave instruction (SpParams::merge; tools/spectrum_time.py)
    uint32_t depth_merge = kDpMergeDefault;   // VKIMG_DEPTH_MERGE=0|1: how the depth filter's match kernel adds to its LDS histogram (DpParams::merge; tools/depth_time.py)
    uint32_t* d_pull = nullptr;    // k <= 7, the launch whose workgroups pull their work: its words (vk_count.h, PullParams; ct_pull)
    size_t pull_cap = 0;
    bool k1_static = false;        // VKIMG_K1_STATIC=1: the k <= 7 count as one workgroup per (sample, part), each wavefront its fixed range, instead of resident workgroups that pull chunks (tests, A/B timing)
    uint32_t k1_helpers = 0xFFFFFFFFu;   // VKIMG_K1_HELPERS=n: workgroups that may join a sample beside its owner, in place of pull_plan's figure; samples of one part then pull as well (tests, A/B timing)
    uint32_t last_helpers = 0, last_pull_samples = 0;   // of the last count call: its bound on helpers and its samples (0: no pulling launch; vk_last_count_pull)
    bool k1_classic = false;       // VKIMG_K1_CLASSIC=1: k <= 7 through vk_count_kernel (every byte through the heavy stage) instead of vk_count_dense_kernel (tests, A/B timing)
};

#define VK_HIP(ctx, call)                     \
    do {                                      \
        hipError_t e_ = (call);               \
        if (e_ != hipSuccess) {               \
            (ctx)->last = e_;                 \
            return VK_EHIP;                   \
        }                                     \
    } while (0)

namespace {

int ensure(vk_ctx* ctx, void** p, size_t* cap, size_t need) {
    if (*cap >= need) return VK_OK;
    if (*p) VK_HIP(ctx, hipFree(*p));
    *p = nullptr;
    *cap = 0;
    size_t n = need + need / 4 + 256;
    VK_HIP(ctx, hipMalloc(p, n));
    *cap = n;
    return VK_OK;
}

// A workspace of the context (*p, *cap: grown on demand) in the pieces `pieces(take)` states: once for the size, once for the pointers.
template <class P, class F>
int ws_carve(vk_ctx* ctx, P** p, size_t* cap, F&& pieces) {
    WsTake size{nullptr, 0};
    pieces(size);
    int rc = ensure(ctx, reinterpret_cast<void**>(p), cap, size.at);
    if (rc) return rc;
    WsTake take{reinterpret_cast<uint8_t*>(*p), 0};
    pieces(take);
    return VK_OK;
}

// environment switches, read when a context is made: NAME=1, NAME=<number>
bool env_flag(const char* name) {
    const char* e = getenv(name);
    return e && e[0] == '1';
}
template <class T>
void env_uint(const char* name, T* dst) {
    const char* e = getenv(name);
    if (e && e[0]) *dst = static_cast<T>(strtoull(e, nullptr, 10));
}

// The runtime k (5..9, checked by the caller) as the template argument of f: f(std::integral_constant<int, K>{}).
template <class F>
int with_k(int k, F&& f) {
    switch (k) {
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 7: return f(std::integral_constant<int, 7>{});
        case 8: return f(std::integral_constant<int, 8>{});
        default: return f(std::integral_constant<int, 9>{});
    }
}

// Sample descriptors go through a pinned host mirror; an unchanged batch (the
// steady state of a pipeline that recycles its buffers) is not uploaded again.
int upload_desc(vk_ctx* ctx, const uint64_t* offsets, const uint64_t* lengths, uint32_t n) {
    const size_t bytes = static_cast<size_t>(n) * sizeof(uint64_t);
    if (ctx->desc_n == n && ctx->h_desc && memcmp(ctx->h_desc, offsets, bytes) == 0 &&
        memcmp(ctx->h_desc + n, lengths, bytes) == 0)
        return VK_OK;
    // Two pinned mirrors take turns: the new descriptors go into the one that was NOT uploaded last, and
    // the host waits only for the copy that read that mirror two batches ago (an event behind it) -- not,
    // as a stream synchronise would, for every kernel queued since (a pipeline's batches all differ).
    uint64_t* m = ctx->h_desc_alt;
    size_t cap = ctx->h_desc_alt_cap;
    hipEvent_t ev = ctx->desc_ev_alt;
    if (ev) VK_HIP(ctx, hipEventSynchronize(ev));
    if (cap < 2 * bytes) {
        if (m) VK_HIP(ctx, hipHostFree(m));
        m = nullptr;
        cap = 0;
        ctx->h_desc_alt = nullptr;
        ctx->h_desc_alt_cap = 0;
        VK_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&m), 2 * bytes + 4096, hipHostMallocDefault));
        cap = 2 * bytes + 4096;
    }
    if (!ev) VK_HIP(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    memcpy(m, offsets, bytes);
    memcpy(m + n, lengths, bytes);
    VK_HIP(ctx, hipMemcpyAsync(ctx->d_desc, m, 2 * bytes, hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipEventRecord(ev, ctx->stream));
    // swap: what was uploaded just now becomes the cache the next call compares against
    ctx->h_desc_alt = ctx->h_desc;
    ctx->h_desc_alt_cap = ctx->h_desc_cap;
    ctx->desc_ev_alt = ctx->desc_ev;
    ctx->h_desc = m;
    ctx->h_desc_cap = cap;
    ctx->desc_ev = ev;
    ctx->desc_n = n;
    return VK_OK;
}

uint32_t npad_of(uint32_t npix) {
    uint32_t p = 1;
    while (p < npix) p <<= 1;
    return p;
}

// The samples of a count / index call and how its launches split them.
struct CtPlan {
    const uint8_t* fq;
    uint32_t nsamples, parts;    // workgroups per sample
    uint64_t maxlen;             // the longest sample
    size_t nwaves;               // nsamples * parts * kWaves: a slot each in d_wavephase
    const uint64_t *d_offs, *d_lens;   // the descriptors on the device
};

// The arguments every such call checks alike (nsamples > 0), and the longest sample.
int ct_check(vk_ctx* ctx, const void* d_fastq, const uint64_t* offsets, const uint64_t* lengths, uint32_t nsamples, CtPlan* p) {
    if (!d_fastq || (reinterpret_cast<uintptr_t>(d_fastq) & 15u) != 0) return VK_EINVAL;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    *p = CtPlan{static_cast<const uint8_t*>(d_fastq), nsamples, 0, 0, 0, nullptr, nullptr};
    for (uint32_t i = 0; i < nsamples; ++i) {
        if ((offsets[i] & 15u) != 0) return VK_EINVAL;
        if (lengths[i] > p->maxlen) p->maxlen = lengths[i];
    }
    return VK_OK;
}

// The split is settled (at least `parts` workgroups per sample): the descriptors and a phase word per wave on the device.
int ct_split(vk_ctx* ctx, const uint64_t* offsets, const uint64_t* lengths, uint32_t parts, CtPlan* p) {
    // a wavefront addresses its byte range through a 32-bit buffer descriptor (vk_count.h, wave_stream):
    // keep every range below 2 GiB, whatever the caller asked for
    while (p->maxlen / (static_cast<uint64_t>(parts) * kWaves) >= (1ull << 31)) parts *= 2;
    if (static_cast<uint64_t>(p->nsamples) * parts > (1u << 24)) return VK_EINVAL;
    p->parts = parts;
    p->nwaves = static_cast<size_t>(p->nsamples) * parts * kWaves;
    if (ctx->desc_cap < 2ull * p->nsamples * sizeof(uint64_t)) ctx->desc_n = 0;  // realloc drops the cached copy
    int rc = ensure(ctx, reinterpret_cast<void**>(&ctx->d_desc), &ctx->desc_cap, 2ull * p->nsamples * sizeof(uint64_t));
    if (rc) return rc;
    rc = ensure(ctx, reinterpret_cast<void**>(&ctx->d_wavephase), &ctx->wavephase_cap, p->nwaves * sizeof(uint32_t));
    if (rc) return rc;
    p->d_offs = ctx->d_desc;
    p->d_lens = ctx->d_desc + p->nsamples;
    return upload_desc(ctx, offsets, lengths, p->nsamples);
}

// What a launch over the plan's samples ends with: the line-phase check of the byte ranges into d_status.  With `lengths`
// (a count) the figures vk_last_count_general reads are kept.
int ct_finish(vk_ctx* ctx, const CtPlan& p, const uint64_t* lengths, uint32_t* d_status) {
    if (lengths) {
        ctx->last_waves = p.nwaves;
        ctx->last_bytes = 0;
        for (uint32_t i = 0; i < p.nsamples; ++i) ctx->last_bytes += lengths[i];
    }
    hipLaunchKernelGGL(vk_check_kernel, dim3((p.nsamples + 255) / 256), dim3(256), 0, ctx->stream, p.fq, p.d_offs, p.d_lens,
                       p.nsamples, p.parts, ctx->d_wavephase, d_status);
    VK_HIP(ctx, hipGetLastError());
    return VK_OK;
}

// The waves' lists of lanes set aside (vk_count.h): room for one lane per piece of the longest range (fastp-shaped
// reads need 0.45), at least 64 entries; a wave whose list is full sends its pieces down the general path instead.
// ctx->d_aside holds the lists of `nwaves` waves, *d_aside_n their lengths.
int aside_lists(vk_ctx* ctx, const CtPlan& p, size_t nwaves, uint32_t* cap_out, uint32_t** d_aside_n) {
    const uint64_t wave_bytes = p.maxlen / (static_cast<uint64_t>(p.parts) * kWaves) + 64;
    uint64_t cap = wave_bytes / kPiece + 64;
    if (cap > (1u << 20)) cap = 1u << 20;
    int rc = ensure(ctx, reinterpret_cast<void**>(&ctx->d_aside), &ctx->aside_cap, nwaves * (cap + 1) * sizeof(uint32_t));   // lists, then their lengths
    if (rc) return rc;
    *cap_out = static_cast<uint32_t>(cap);
    *d_aside_n = ctx->d_aside + nwaves * cap;
    return VK_OK;
}

// The words of a launch whose workgroups pull their work (vk_count.h, PullParams), zeroed; its grid in *grid.  The count
// kernels keep two workgroups of kCountThreads per CU resident.
int ct_pull(vk_ctx* ctx, const CtPlan& p, PullParams* pp, uint32_t* grid) {
    const PullPlan pl = pull_plan(2u * static_cast<uint32_t>(ctx->num_cus), p.nsamples, p.parts, ctx->k1_helpers);
    *grid = pl.grid;
    if (pl.grid == 0) return VK_OK;   // (the rule keeps the static launch for this batch)
    int rc = ws_carve(ctx, &ctx->d_pull, &ctx->pull_cap, [&](WsTake& take) { take(pp->words, pull_words(p.nsamples)); });
    if (rc) return rc;
    VK_HIP(ctx, hipMemsetAsync(pp->words, 0, pull_words(p.nsamples) * sizeof(uint32_t), ctx->stream));
    pp->helpers = pl.helpers;
    ctx->last_helpers = pl.helpers;
    ctx->last_pull_samples = p.nsamples;
    return VK_OK;
}

template <int K>
int launch_count(vk_ctx* ctx, const CtPlan& p, uint32_t* d_hist, const SubParams* sub, const IndexParams* index = nullptr) {
    const uint32_t nsamples = p.nsamples, parts = p.parts;
    bool pulling = !sub && !index && !ctx->k1_classic && !ctx->k1_static;
    uint32_t grid = nsamples * parts;
    ctx->last_pull_samples = 0;
    PullParams pp{};
    if (pulling) {
        const int rc = ct_pull(ctx, p, &pp, &grid);
        if (rc) return rc;
        pulling = grid != 0;
        if (!pulling) grid = nsamples * parts;
    }
    // (pulling: owner and helpers flush into the same zeroed row; a sample nobody may help is stored by its owner alone)
    const int atomic_flush = (pulling ? pp.helpers > 0 : parts > 1) ? 1 : 0;
    if (atomic_flush)
        VK_HIP(ctx, hipMemsetAsync(d_hist, 0, static_cast<size_t>(nsamples) * (1u << (2 * K)) * sizeof(uint32_t),
                                   ctx->stream));
    ctx->last_grid = grid;
    ctx->last_block = kCountThreads;
    ctx->last_lds = (1u << (2 * K)) * 4u + kWaves * 64 + 2 * 66 * 16;
    if (sub)
        hipLaunchKernelGGL((vk_count_kernel<K, true>), dim3(grid), dim3(kCountThreads), 0, ctx->stream, p.fq,
                           p.d_offs, p.d_lens, nsamples, parts, d_hist, ctx->d_wavephase, atomic_flush, *sub);
    else if (ctx->k1_classic && !index)
        hipLaunchKernelGGL((vk_count_kernel<K, false>), dim3(grid), dim3(kCountThreads), 0, ctx->stream, p.fq,
                           p.d_offs, p.d_lens, nsamples, parts, d_hist, ctx->d_wavephase, atomic_flush, SubParams{});
    else {
        ctx->last_lds = (1u << (2 * K)) * 4u + kWaves * 1024;
        uint32_t cap = 0, *d_aside_n = nullptr;
        int rc = aside_lists(ctx, p, p.nwaves, &cap, &d_aside_n);
        if (rc) return rc;
        // vk_aside_kernel: about a thousand workgroups, each serving `upb` workgroups of the count launch (of one sample)
        const uint32_t awant = nsamples >= 1024u ? 1u : (1024u + nsamples - 1u) / nsamples;
        const uint32_t upb = (parts + (awant < parts ? awant : parts) - 1u) / (awant < parts ? awant : parts);
        const uint32_t ablocks = (parts + upb - 1u) / upb;
        if (index) {   // the count and the read index of the samples in one pass (vk_count_index_device)
            hipLaunchKernelGGL((vk_count_dense_kernel<K, true>), dim3(grid), dim3(kCountThreads), 0, ctx->stream, p.fq,
                               p.d_offs, p.d_lens, nsamples, parts, d_hist, ctx->d_wavephase, atomic_flush, ctx->d_aside,
                               cap, d_aside_n, *index, PullParams{});
            VK_HIP(ctx, hipGetLastError());
            hipLaunchKernelGGL((vk_aside_kernel<K, true>), dim3(nsamples * ablocks), dim3(kCountThreads), 0, ctx->stream, p.fq,
                               p.d_offs, p.d_lens, nsamples, parts, d_hist, ctx->d_aside, cap, d_aside_n, *index, upb);
        } else {
            if (pulling) {   // resident workgroups that own samples and pull their chunks (vk_count.h, PullParams)
                hipLaunchKernelGGL((vk_count_dense_kernel<K, false, true>), dim3(grid), dim3(kCountThreads), 0, ctx->stream, p.fq,
                                   p.d_offs, p.d_lens, nsamples, parts, d_hist, ctx->d_wavephase, atomic_flush, ctx->d_aside,
                                   cap, d_aside_n, IndexParams{}, pp);
            } else {
                hipLaunchKernelGGL((vk_count_dense_kernel<K, false>), dim3(grid), dim3(kCountThreads), 0, ctx->stream, p.fq,
                                   p.d_offs, p.d_lens, nsamples, parts, d_hist, ctx->d_wavephase, atomic_flush, ctx->d_aside,
                                   cap, d_aside_n, IndexParams{}, PullParams{});
            }
            VK_HIP(ctx, hipGetLastError());
#ifndef VK_DIAG_ASIDE_INLINE   // (diagnostic: the count kernel counts its own lists, vk_count.h)
            hipLaunchKernelGGL((vk_aside_kernel<K, false>), dim3(nsamples * ablocks), dim3(kCountThreads), 0, ctx->stream, p.fq,
                               p.d_offs, p.d_lens, nsamples, parts, d_hist, ctx->d_aside, cap, d_aside_n, IndexParams{}, upb);
#endif
        }
    }
    VK_HIP(ctx, hipGetLastError());
    return VK_OK;
}

// k = 8, 9: how many 4 KiB runs a sample's arena gets (*runs: in, what the route wants for its entries and open runs) and
// how many samples a sub-batch holds.  `run_bytes`: a run with its header words, `fixed_bytes`: the rest of a sample's share.
int spill_plan(vk_ctx* ctx, uint32_t nsamples, size_t run_bytes, size_t fixed_bytes, size_t* runs, size_t* batch_out) {
    if (ctx->spill_runs_cap) *runs = ctx->spill_runs_cap;  // VKIMG_SPILL_RUNS_CAP: tests force the arena-full fallback
    if (*runs >= (1u << 24)) return VK_EINVAL;             // a run number travels in 24 bits (64 GiB of entries per sample)
    const size_t per_sample = *runs * run_bytes + fixed_bytes + 64;
    // never plan for more than three quarters of what is free (plus what this context already holds)
    size_t free_b = 0, total_b = 0;
    VK_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
    size_t budget = ctx->spill_budget;
    const size_t avail = free_b / 4 * 3 + ctx->spill_cap;
    if (budget > avail) budget = avail;
    uint32_t batch = static_cast<uint32_t>(budget / per_sample);
    if (batch == 0) batch = 1;
    if (batch > nsamples) batch = nsamples;
    *batch_out = batch;
    return VK_OK;
}

// The sub-batches of a k = 8, 9 count, `batch` samples at a time: the head of the workspace (cursors and run headers)
// zeroed, then body(s0, n, hist0, wph0) for samples s0 .. s0 + n with their rows of d_hist and d_wavephase.
template <int K, class F>
int spill_batches(vk_ctx* ctx, const CtPlan& p, size_t batch, size_t head_bytes, uint32_t* d_hist, F&& body) {
    constexpr uint32_t NCODE = 1u << (2 * K);
    VK_HIP(ctx, hipMemsetAsync(d_hist, 0, static_cast<size_t>(p.nsamples) * NCODE * sizeof(uint32_t), ctx->stream));
    ctx->last_block = kCountThreads;
    ctx->last_lds = kLdsBucketBytes;
    for (uint32_t s0 = 0; s0 < p.nsamples; s0 += batch) {
        const uint32_t n = p.nsamples - s0 < batch ? p.nsamples - s0 : static_cast<uint32_t>(batch);
        VK_HIP(ctx, hipMemsetAsync(ctx->d_spill, 0, head_bytes, ctx->stream));
        ctx->last_grid = n * p.parts;
        const int rc = body(s0, n, d_hist + static_cast<size_t>(s0) * NCODE, ctx->d_wavephase + static_cast<size_t>(s0) * p.parts * kWaves);
        if (rc) return rc;
    }
    return VK_OK;
}

// k = 8, 9, the quad route (vk_count.h: vk_bucket_kernel<K, 3>, vk_quad_list / _count / _merge_kernel),
// in sub-batches that fit the spill budget.
template <int K>
int launch_spill_quad(vk_ctx* ctx, const CtPlan& p, uint32_t* d_hist) {
    constexpr uint32_t NCODE = 1u << (2 * K);
    constexpr size_t kOutWords = 4u << (2 * K - 8);   // what a pass B job stores: four window arrays of 4^(K-4) counters
    const uint32_t parts = p.parts;
    // the regions of quads of which only some windows count, one per (workgroup of pass A, bucket): ~1 per 215 bytes of
    // 150-base reads over 256 buckets; room for four times that (uniform bases), at least 64
    const uint64_t wg_bytes = p.maxlen / parts + 64 * kWaves;
    uint32_t pshift = 6;                                   // (a power of two: the place is a shift and an or)
    while (pshift < 21 && (1ull << pshift) < wg_bytes / 16384 + 64) ++pshift;   // (at most 2^21: a workgroup's 256 regions stay below 2^31 bytes, the size a buffer descriptor takes as an int; what does not fit is counted directly)
    if (ctx->spill_misc_cap) pshift = ctx->spill_misc_cap < 21 ? ctx->spill_misc_cap : 21;   // VKIMG_SPILL_MISC_CAP (log2): tests force the region-full fallback
    const uint64_t pcap = 1ull << pshift;
    const size_t preg_words = static_cast<size_t>(parts) * kQuadBuckets * (pcap + 1);   // per sample: regions, populations
    // Arena of one sample, in 4 KiB runs: a quad entry is 2 bytes and a FASTQ holds at most len / 8 quads (sequence
    // lines are less than half of the text), so len / 4 bytes however they spread over the 256 buckets; plus the
    // blocks a drain may leave unused at the end of a run, one open run per (workgroup, queue), one reserve per wave.
    // A run has a header and a place in qlist; per sample on top: qfirst, job sizes and order, a cursor, pass B's tables, the regions.
    size_t runs = (p.maxlen / 4 + p.maxlen / 32) / kRunBytes + 16 + static_cast<uint64_t>(parts) * (kQuadBuckets + kWaves * kPoolRuns), batch = 0;
    int rc = spill_plan(ctx, p.nsamples, kRunBytes + 2 * sizeof(uint32_t),
                        (3 * kQuadBuckets + 2) * sizeof(uint32_t) + kQuadBuckets * kOutWords * sizeof(uint32_t) + preg_words * sizeof(uint32_t), &runs, &batch);
    if (rc) return rc;
    BucketParams bp{};
    size_t head_bytes = 0;
    rc = ws_carve(ctx, &ctx->d_spill, &ctx->spill_cap, [&](WsTake& take) {
        take(bp.cursors, batch);
        take(bp.hdrs, batch * runs);
        head_bytes = take.at;   // zeroed per sub-batch: the cursors and run headers
        take(bp.qfirst, batch * (kQuadBuckets + 1));
        take(bp.qlist, batch * runs);
        take(bp.bsize, batch * kQuadBuckets);   // job sizes
        take(bp.order, batch * kQuadBuckets);   // job order
        take(bp.preg_n, batch * parts * kQuadBuckets);
        take(bp.preg, batch * parts * kQuadBuckets * pcap);
        take(bp.bucket_hist, batch * kQuadBuckets * kOutWords);   // window arrays [batch][256][4][4^(K-4)]
        take(bp.arena, batch * runs * kRunBytes);
    });
    if (rc) return rc;
    bp.preg_shift = pshift;
    bp.parts = parts;
    bp.runs_cap = static_cast<uint32_t>(runs);
    return spill_batches<K>(ctx, p, batch, head_bytes, d_hist, [&](uint32_t s0, uint32_t n, uint32_t* hist0, uint32_t* wph0) {
        hipLaunchKernelGGL((vk_bucket_kernel<K, 3>), dim3(n * parts), dim3(kCountThreads), 0, ctx->stream,
                           p.fq, p.d_offs + s0, p.d_lens + s0, n, parts, hist0, wph0, bp, SubParams{}, PackParams{});
        VK_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(vk_quad_list_kernel, dim3(n), dim3(1024), 0, ctx->stream, bp);
        VK_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(vk_bucket_order_kernel, dim3(1), dim3(1024), 0, ctx->stream, bp, n * kQuadBuckets);
        VK_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL((vk_quad_count_kernel<K>), dim3(n * kQuadBuckets), dim3(512), 0, ctx->stream, bp);
        VK_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL((vk_quad_merge_kernel<K>), dim3(n * (NCODE / kMergeTile)), dim3(256), 0, ctx->stream, bp, hist0);
        VK_HIP(ctx, hipGetLastError());
        return VK_OK;
    });
}

// k = 8, 9: bucket pass + replay pass, in sub-batches that fit the spill budget.
template <int K>
int launch_spill(vk_ctx* ctx, const CtPlan& p, uint32_t* d_hist, const SubParams* sub) {
    constexpr uint32_t NCODE = 1u << (2 * K);
    if (sub == nullptr && !ctx->spill_packed && !ctx->spill_pairs) return launch_spill_quad<K>(ctx, p, d_hist);
    const uint32_t parts = p.parts;
    constexpr size_t kBucketHistWords = static_cast<size_t>(kQueues) * (2u << (2 * K - 4));  // pass B -> merge
    // the packed stream of a sample (vk_pack.h): a record per 16 bytes of text at most, a few per wavefront on top
    const bool packed = sub == nullptr && ctx->spill_packed;
    const uint64_t pack_recs = packed ? ((p.maxlen + 15) / 16 + 8ull * parts * kWaves + 16 + 3) / 4 * 4 : 0;
    // Arena of one sample, in 4 KiB runs: a pair entry is 2 bytes and a FASTQ holds at most len / 4
    // pairs (sequence lines are less than half of the text), so len / 2 bytes however the pairs spread
    // over the 16 buckets; plus the blocks a drain may leave unused at the end of a run (at most 3 of
    // 64), plus one open run per (workgroup, wave, queue) and one reserve per wave.
    // A run has a header; per sample on top: a cursor, job sizes, order and wide flags, pass B's tables, the packed stream.
    size_t runs = (p.maxlen / 2 + p.maxlen / 16) / kRunBytes + 16 + static_cast<uint64_t>(parts) * kWaves * (kQueues + kPoolRuns), batch = 0;
    int rc = spill_plan(ctx, p.nsamples, kRunBytes + sizeof(uint32_t),
                        sizeof(uint32_t) + 3 * kQueues * sizeof(uint32_t) + kBucketHistWords * sizeof(uint32_t) + pack_recs * 8, &runs, &batch);
    if (rc) return rc;
    BucketParams bp{};
    PackParams pk{};
    uint64_t* d_base = nullptr;
    size_t head_bytes = 0;
    rc = ws_carve(ctx, &ctx->d_spill, &ctx->spill_cap, [&](WsTake& take) {
        take(bp.cursors, batch);
        take(bp.hdrs, batch * runs);
        take(bp.bsize, batch * kQueues);   // bucket sizes
        take(bp.order, batch * kQueues);   // job order
        take(bp.wide, batch * kQueues);    // wide flags
        head_bytes = take.at;   // zeroed per sub-batch: all of the above
        take(bp.bucket_hist, batch * kBucketHistWords);   // [batch][16][2 * 4^K / 16]
        take(bp.arena, batch * runs * kRunBytes);
        if (!packed) return;
        // packed stream: codes | masks (+ a block of slack: the last wavefront's loads run to the end of its last block) | sample bases | counts
        take(pk.c, batch * pack_recs + kPackBlock);
        take(pk.m, batch * pack_recs + kPackBlock);
        take(d_base, batch);
        take(pk.count, batch * parts * kWaves);
    });
    if (rc) return rc;
    bp.force_wide = ctx->spill_force_wide ? 1u : 0u;
    bp.runs_cap = static_cast<uint32_t>(runs);
    uint32_t aside_cap = 0, *d_aside_n = nullptr;
    if (packed) {
        pk.base = d_base;
        std::vector<uint64_t> base(batch);
        for (uint32_t i = 0; i < batch; ++i) base[i] = static_cast<uint64_t>(i) * pack_recs;
        VK_HIP(ctx, hipMemcpyAsync(d_base, base.data(), batch * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
        VK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (base is a temporary; once per call)
        rc = aside_lists(ctx, p, batch * parts * kWaves, &aside_cap, &d_aside_n);   // as for the k <= 7 kernel
        if (rc) return rc;
    }
    return spill_batches<K>(ctx, p, batch, head_bytes, d_hist, [&](uint32_t s0, uint32_t n, uint32_t* hist0, uint32_t* wph0) {
        const uint64_t *const d_offs = p.d_offs + s0, *const d_lens = p.d_lens + s0;
        if (sub) {
            SubParams ss = *sub;  // this sub-batch's slice of the per-sample arrays
            ss.seeds += s0;
            ss.thresholds += s0;
            if (ss.sites) ss.sites += 2ull * s0;
            hipLaunchKernelGGL((vk_bucket_kernel<K, 1>), dim3(n * parts), dim3(kCountThreads), 0, ctx->stream,
                               p.fq, d_offs, d_lens, n, parts, hist0, wph0, bp, ss, PackParams{});
        } else if (packed) {
            // pass A in two kernels: the text packed once (the k <= 7 kernel's front end), the stream partitioned
            hipLaunchKernelGGL(vk_pack_kernel, dim3(n * parts), dim3(kCountThreads), 0, ctx->stream, p.fq, d_offs,
                               d_lens, n, parts, pk, wph0, ctx->d_aside, aside_cap, d_aside_n);
            VK_HIP(ctx, hipGetLastError());
            hipLaunchKernelGGL((vk_aside_kernel<K, false>), dim3(n * parts), dim3(kCountThreads), 0, ctx->stream, p.fq,
                               d_offs, d_lens, n, parts, hist0, ctx->d_aside, aside_cap, d_aside_n, IndexParams{}, 1u);
            VK_HIP(ctx, hipGetLastError());
            hipLaunchKernelGGL((vk_bucket_kernel<K, 2>), dim3(n * parts), dim3(kCountThreads), 0, ctx->stream,
                               p.fq, d_offs, d_lens, n, parts, hist0, wph0, bp, SubParams{}, pk);
        } else {
            hipLaunchKernelGGL((vk_bucket_kernel<K, 0>), dim3(n * parts), dim3(kCountThreads), 0, ctx->stream,
                               p.fq, d_offs, d_lens, n, parts, hist0, wph0, bp, SubParams{}, PackParams{});
        }
        VK_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(vk_bucket_order_kernel, dim3(1), dim3(1024), 0, ctx->stream, bp, n * kQueues);
        VK_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL((vk_bucket_count_kernel<K>), dim3(n * kQueues), dim3(kCountThreads), 0, ctx->stream, bp);
        VK_HIP(ctx, hipGetLastError());
        // (jobs whose u16 pair counters wrapped: replayed into u32 window counters; every other workgroup leaves at once)
        hipLaunchKernelGGL((vk_bucket_count_wide_kernel<K>), dim3(n * kQueues), dim3(kCountThreads), 0, ctx->stream, bp);
        VK_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL((vk_bucket_merge_kernel<K>), dim3(n * (NCODE / 256)), dim3(256), 0, ctx->stream, bp, hist0);
        VK_HIP(ctx, hipGetLastError());
        return VK_OK;
    });
}

uint32_t choose_parts(uint32_t nsamples, uint64_t maxlen, int k) {
    // The count kernels keep two workgroups per CU resident: 512 slots on the 256 CUs.
    constexpr uint64_t kSlots = 512;
    if (k <= 7) {
        // Round 6: MANY more workgroups than slots.  Rounds 2-5 launched 1000 samples as 1000 workgroups of 320 MB -- two
        // "rounds" of the chip in lock-step -- and the wave-cycle counter read 85 % of the launch (profiles/r05a): a
        // workgroup's slot is held until its slowest wavefront is through its sixteenth of the sample, and a CU that runs
        // a few per cent behind (another XCD's L2, a busier memory channel) ends the launch alone.  In workgroups of
        // 10-27 MB (20 MiB is the rule) the dispatcher hands the faster CUs more of them: 65.6 -> 62.6 ms for 1000 samples, 7.13 -> 6.63 for 100,
        // 74.1 -> 71.1 on fastp-shaped reads (profiles/ab/r06_parts.txt; flat from 12 to 32 parts, slower again from 64:
        // every workgroup zeroes and flushes a 64 KB histogram and every wavefront finds its line phase).  At least four
        // rounds of the chip where that leaves workgroups of 4 MiB.
        const uint64_t cap4 = maxlen / (4ull << 20) > 1 ? maxlen / (4ull << 20) : 1;
        uint64_t parts = (maxlen + (10ull << 20)) / (20ull << 20);
        if (parts < 1) parts = 1;
        const uint64_t want = (4 * kSlots + nsamples - 1) / nsamples;
        if (parts < want) parts = want < cap4 ? want : cap4;
        if (parts > 512) parts = 512;
        if (nsamples * parts >= 4 * kSlots) return static_cast<uint32_t>(parts);
    } else if (nsamples >= 4 * kSlots) {
        return 1;
    }
    // Few workgroups after all (a handful of samples; k = 8, 9, whose workspace is sized by the workgroup): a launch of G equal
    // workgroups runs in ceil(G / 512) rounds, so G just below a multiple of 512 wastes the least (100 samples: 5 parts = 500
    // workgroups, not 8 = 800 in two rounds).  Parts never get so small (< 1 MiB) that the per-wave range sync shows.
    uint32_t best = 1;
    double best_eff = 0.0;
    for (uint32_t parts = 1; parts <= 512; ++parts) {
        if (parts > 1 && maxlen / parts < (1u << 20)) break;
        const uint64_t g = static_cast<uint64_t>(nsamples) * parts;
        const double eff = static_cast<double>(g) / static_cast<double>((g + kSlots - 1) / kSlots * kSlots);
        if (eff > best_eff) {
            best_eff = eff;
            best = parts;
        }
        if (eff >= 0.95) break;  // good enough: more parts only add range syncs, flushes and open runs
    }
    return best;
}

}  // namespace

extern "C" {

int vk_abi_version(void) { return 1; }

const char* vk_strerror(int status) {
    switch (status) {
        case VK_OK: return "ok";
        case VK_EINVAL: return "invalid argument";
        case VK_EHIP: return "HIP runtime error";
        case VK_ENOMAP: return "no k-mer mapping installed for this k";
        case VK_EFORMAT: return "inconsistent FASTQ framing";
        case VK_ENOMEM: return "out of memory";
        case VK_ENOSPC: return "the output does not fit the buffer";
        default: return "unknown status";
    }
}

const char* vk_last_hip_error(const vk_ctx* ctx) {
    if (!ctx || ctx->last == hipSuccess) return "";
    return hipGetErrorString(ctx->last);
}

int vk_ctx_create(int device, void* stream, int own_stream, vk_ctx** out) {
    if (!out) return VK_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return VK_EHIP;
    vk_ctx* ctx = new (std::nothrow) vk_ctx();
    if (!ctx) return VK_ENOMEM;
    ctx->device = device;
    ctx->image_sort_only = env_flag("VKIMG_IMAGE_SORT_ONLY");
    ctx->gz_no_chunks = env_flag("VKIMG_GZ_NO_CHUNKS");
    env_uint("VKIMG_GZ_CHUNK_BYTES", &ctx->gz_chunk_bytes);
    ctx->gz_split_find = env_flag("VKIMG_GZ_SPLIT_FIND");
    env_uint("VKIMG_GZ_FILL", &ctx->gz_fill_pct);
    env_uint("VKIMG_GZ_LDS_PAD", &ctx->gz_lds_pad);
    env_uint("VKIMG_SPILL_RUNS_CAP", &ctx->spill_runs_cap);
    env_uint("VKIMG_SPILL_BUDGET", &ctx->spill_budget);
    ctx->spill_packed = env_flag("VKIMG_SPILL_PACKED");
    env_uint("VKIMG_SPILL_MISC_CAP", &ctx->spill_misc_cap);
    ctx->spill_pairs = env_flag("VKIMG_SPILL_PAIRS");
    ctx->spill_force_wide = env_flag("VKIMG_SPILL_FORCE_WIDE");
    uint64_t hash_bits = 64;
    env_uint("VKIMG_CLEAN_HASH_BITS", &hash_bits);
    ctx->clean_hash_bits = hash_bits >= 1 && hash_bits <= 64 ? static_cast<uint32_t>(hash_bits) : 64u;
    ctx->k1_classic = env_flag("VKIMG_K1_CLASSIC");
    ctx->k1_static = env_flag("VKIMG_K1_STATIC");
    env_uint("VKIMG_K1_HELPERS", &ctx->k1_helpers);
    env_uint("VKIMG_FASTA_UNIT_BYTES", &ctx->fasta_unit_bytes);
    ctx->fasta_unit_bytes = fa_unit_clamp(ctx->fasta_unit_bytes);
    env_uint("VKIMG_BAM_SEG_BYTES", &ctx->bam_seg_bytes);
    if (ctx->bam_seg_bytes && ctx->bam_seg_bytes < 64) ctx->bam_seg_bytes = 64;
    if (ctx->bam_seg_bytes > kBamSegBytes) ctx->bam_seg_bytes = kBamSegBytes;
    env_uint("VKIMG_SCREEN_TILE", &ctx->screen_tile);
    if (ctx->screen_tile) {
        ctx->screen_tile = ctx->screen_tile / 64 * 64;
        if (ctx->screen_tile < 64) ctx->screen_tile = 64;
        if (ctx->screen_tile > kScMaxTile) ctx->screen_tile = kScMaxTile;
    }
    env_uint("VKIMG_SPECTRUM_TILE", &ctx->spectrum_tile);
    if (ctx->spectrum_tile) {
        ctx->spectrum_tile = ctx->spectrum_tile / 64 * 64;
        if (ctx->spectrum_tile < 64) ctx->spectrum_tile = 64;
        if (ctx->spectrum_tile > kScMaxTile) ctx->spectrum_tile = kScMaxTile;
    }
    env_uint("VKIMG_SPECTRUM_MERGE", &ctx->spectrum_merge);
    if (ctx->spectrum_merge > 2) ctx->spectrum_merge = kSpMergeDefault;
    env_uint("VKIMG_DEPTH_MERGE", &ctx->depth_merge);
    if (ctx->depth_merge > 1) ctx->depth_merge = kDpMergeDefault;
    env_uint("VKIMG_QC_MERGE", &ctx->qc_merge);
    if (ctx->qc_merge > kQcMerge) ctx->qc_merge = kQcMerge;
    env_uint("VKIMG_DIST_STRIP", &ctx->dist_strip);
    env_uint("VKIMG_BAM_PANEL_SEGS", &ctx->bam_panel_segs);
    if (ctx->bam_panel_segs > 4096) ctx->bam_panel_segs = 4096;
    ctx->no_read_index = getenv("VKIMG_NO_READ_INDEX") != nullptr;   // (set at all, as ever)
    if (hipSetDevice(device) != hipSuccess) { delete ctx; return VK_EHIP; }
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) ctx->num_cus = cus;
    }
    if (!own_stream) {
        ctx->stream = static_cast<hipStream_t>(stream);  // NULL = the device's default stream
    } else {
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return VK_EHIP; }
        ctx->own_stream = true;
    }
    *out = ctx;
    return VK_OK;
}

void vk_ctx_destroy(vk_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (int k = 0; k < 10; ++k)
        if (ctx->d_pix[k]) (void)hipFree(ctx->d_pix[k]);
    void* ptrs[] = {ctx->d_desc, ctx->d_wavephase, ctx->d_scratch, ctx->d_spill, ctx->d_stage, ctx->d_hist1, ctx->d_status1, ctx->d_img1, ctx->d_sub, ctx->d_gzjobs, ctx->d_gzmeta, ctx->d_gzsym, ctx->d_gzwin, ctx->d_gzcrc, ctx->d_synth, ctx->d_synth_offs, ctx->d_aside, ctx->d_pull, ctx->d_index, ctx->d_walk, ctx->d_clines, ctx->d_cladapt, ctx->d_cldetect, ctx->d_fasta, ctx->d_fawin, ctx->d_bamws, ctx->d_bamgws};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (ctx->h_desc) (void)hipHostFree(ctx->h_desc);
    if (ctx->h_desc_alt) (void)hipHostFree(ctx->h_desc_alt);
    if (ctx->desc_ev) (void)hipEventDestroy(ctx->desc_ev);
    if (ctx->desc_ev_alt) (void)hipEventDestroy(ctx->desc_ev_alt);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int vk_ctx_sync(vk_ctx* ctx) {
    if (!ctx) return VK_EINVAL;
    VK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VK_OK;
}

int vk_host_register(vk_ctx* ctx, const void* p, uint64_t nbytes) {
    if (!ctx || !p || nbytes == 0) return VK_EINVAL;
    if (hipSetDevice(ctx->device) != hipSuccess) return VK_EHIP;   // (the calling thread may be an I/O thread that never chose a device)
    const hipError_t e = hipHostRegister(const_cast<void*>(p), nbytes, hipHostRegisterDefault);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return VK_EHIP;   // (ctx->last is left alone: this may run beside the context's own thread)
    }
    return VK_OK;
}

int vk_host_unregister(vk_ctx* ctx, const void* p) {
    if (!ctx || !p) return VK_EINVAL;
    if (hipSetDevice(ctx->device) != hipSuccess) return VK_EHIP;
    return hipHostUnregister(const_cast<void*>(p)) == hipSuccess ? VK_OK : VK_EHIP;
}

int vk_upload_mapped(vk_ctx* ctx, void* d_dst, const uint64_t* dst_offsets, const void* const* h_src,
                     const uint64_t* nbytes, const uint8_t* registered, uint32_t nfiles, uint32_t* status) {
    if (!ctx || !d_dst || (nfiles && (!dst_offsets || !h_src || !nbytes || !status))) return VK_EINVAL;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<char> reg(nfiles, 0), mine(nfiles, 0);
    auto pin = [&](uint32_t i) {   // the file's page-cache pages, pinned and mapped for the DMA engines
        status[i] = 0u;
        if (nbytes[i] == 0) return;
        if (registered && registered[i]) {
            reg[i] = 1;
            return;
        }
        mine[i] = 1;
        if (!h_src[i] || hipHostRegister(const_cast<void*>(h_src[i]), nbytes[i], hipHostRegisterDefault) != hipSuccess) {
            (void)hipGetLastError();
            status[i] = 1u;
            mine[i] = 0;
        } else {
            reg[i] = 1;
        }
    };
    if (nfiles) pin(0);
    int rc = VK_OK;
    for (uint32_t i = 0; i < nfiles; ++i) {
        if (reg[i]) {
            const hipError_t e = hipMemcpyAsync(static_cast<uint8_t*>(d_dst) + dst_offsets[i], h_src[i], nbytes[i],
                                                hipMemcpyHostToDevice, ctx->stream);
            if (e != hipSuccess) {
                ctx->last = e;
                status[i] = 2u;
                rc = VK_EHIP;
            }
        }
        if (i + 1 < nfiles) pin(i + 1);   // while file i is in flight
    }
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    for (uint32_t i = 0; i < nfiles; ++i)
        if (mine[i]) (void)hipHostUnregister(const_cast<void*>(h_src[i]));
    if (es != hipSuccess) {
        ctx->last = es;
        return VK_EHIP;
    }
    return rc;
}

int vk_set_mapping(vk_ctx* ctx, int k, const uint32_t* pix, uint32_t npix) {
    if (!ctx || k < 5 || k > 9) return VK_EINVAL;
    const uint32_t ncode = 1u << (2 * k);
    VK_HIP(ctx, hipSetDevice(ctx->device));
    if (!pix) {
        if (npix != ncode) return VK_EINVAL;
    } else {
        for (uint32_t c = 0; c < ncode; ++c)
            if (pix[c] >= npix) return VK_EINVAL;
    }
    if (!ctx->d_pix[k]) VK_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->d_pix[k]), ncode * sizeof(uint32_t)));
    if (pix) {
        VK_HIP(ctx, hipMemcpyAsync(ctx->d_pix[k], pix, ncode * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        VK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // pix may be a temporary
    } else {
        hipLaunchKernelGGL(vk_cgr_lut_kernel, dim3((ncode + 255) / 256), dim3(256), 0, ctx->stream, k, ctx->d_pix[k]);
        VK_HIP(ctx, hipGetLastError());
    }
    ctx->npix[k] = npix;
    return VK_OK;
}

}  // extern "C"

// Subsampled counts through the read index (vk_ladder.h): every (offset, length) of the call is a sample the context
// holds an index of.  Returns VK_OK with *done = true when the walker ran.
constexpr uint64_t kWalkMaxThresholdSpill = (1ull << 32) / 32;   // k = 8, 9: largest fraction of the reads (as a threshold) the walker takes

static int count_walk(vk_ctx* ctx, const void* d_fastq, const uint64_t* offsets, const uint64_t* lengths, uint32_t nsamples, int k,
                      uint32_t* d_hist, uint32_t* d_status, const uint64_t* seeds, const uint64_t* thresholds, uint64_t* d_sites,
                      bool* done) {
    *done = false;
    if (ctx->ix_fastq != d_fastq || ctx->ix_sample.empty() || ctx->no_read_index) return VK_OK;
    std::vector<uint32_t> isample(nsamples), status(nsamples);
    for (uint32_t i = 0; i < nsamples; ++i) {
        // k = 8, 9: the walker counts into the subsample's row in HBM, one atomic per window (~28 G/s measured): it beats a
        // streamed pass of the spill path only for subsamples of a few per cent of the reads
        if (k > 7 && thresholds[i] > kWalkMaxThresholdSpill) return VK_OK;
        const auto it = ctx->ix_sample.find(std::make_pair(offsets[i], lengths[i]));
        if (it == ctx->ix_sample.end() || ctx->ix_overflow[it->second]) return VK_OK;   // not indexed: the streaming kernels
        if (lengths[i] >= (1ull << 32) - 4096) return VK_OK;                             // (the walker's offsets are 32-bit)
        isample[i] = it->second;
        status[i] = ctx->ix_status[it->second];
    }
    const uint32_t parts = ctx->ix_parts;
    if (static_cast<uint64_t>(nsamples) * parts > (1u << 24)) return VK_OK;
    // per-pair arrays
    uint64_t *d_offs = nullptr, *d_lens = nullptr, *d_seeds = nullptr, *d_thr = nullptr;
    uint32_t* d_is = nullptr;
    int rc = ws_carve(ctx, &ctx->d_walk, &ctx->walk_cap, [&](WsTake& take) {
        take(d_offs, nsamples);
        take(d_lens, nsamples);
        take(d_seeds, nsamples);
        take(d_thr, nsamples);
        take(d_is, nsamples);
    });
    if (rc) return rc;
    VK_HIP(ctx, hipMemcpyAsync(d_offs, offsets, nsamples * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(d_lens, lengths, nsamples * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(d_seeds, seeds, nsamples * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(d_thr, thresholds, nsamples * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(d_is, isample.data(), nsamples * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(d_status, status.data(), nsamples * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the host vectors are temporaries)
    if (d_sites) VK_HIP(ctx, hipMemsetAsync(d_sites, 0, 2ull * nsamples * sizeof(uint64_t), ctx->stream));
    const int atomic_flush = (parts > 1 || k > 7) ? 1 : 0;
    if (atomic_flush)
        VK_HIP(ctx, hipMemsetAsync(d_hist, 0, static_cast<size_t>(nsamples) * (1ull << (2 * k)) * sizeof(uint32_t), ctx->stream));
    const WalkParams wp{d_is, d_seeds, d_thr, reinterpret_cast<unsigned long long*>(d_sites), parts};
    ctx->last_grid = nsamples * parts;
    ctx->last_block = kCountThreads;
    ctx->last_lds = (k <= 7 ? (1u << (2 * k)) * 4u : 4u) + kWaves * kWalkQueue * 4u;
    with_k(k, [&](auto kc) {
        hipLaunchKernelGGL((vk_walk_kernel<decltype(kc)::value>), dim3(nsamples * parts), dim3(kCountThreads), 0, ctx->stream,
                           static_cast<const uint8_t*>(d_fastq), d_offs, d_lens, nsamples, ctx->ix, wp, d_hist, atomic_flush);
        return VK_OK;
    });
    VK_HIP(ctx, hipGetLastError());
    *done = true;
    return VK_OK;
}

extern "C" {

static int count_impl(vk_ctx* ctx, const void* d_fastq, const uint64_t* offsets, const uint64_t* lengths,
                      uint32_t nsamples, int k, uint32_t parts_per_sample, uint32_t* d_hist, uint32_t* d_status,
                      const uint64_t* seeds, const uint64_t* thresholds, uint64_t* d_sites) {
    if (!ctx || !offsets || !lengths || !d_hist || !d_status || k < 5 || k > 9) return VK_EINVAL;
    if (nsamples == 0) return VK_OK;
    CtPlan p;
    int rc = ct_check(ctx, d_fastq, offsets, lengths, nsamples, &p);
    if (rc) return rc;
    if (seeds) {   // subsamples of samples the context holds a read index of: the walker (vk_ladder.h)
        bool done = false;
        const int rcw = count_walk(ctx, d_fastq, offsets, lengths, nsamples, k, d_hist, d_status, seeds, thresholds, d_sites, &done);
        if (rcw || done) return rcw;
    }
    uint32_t parts = parts_per_sample ? parts_per_sample : choose_parts(nsamples, p.maxlen, k);
    if (!parts_per_sample && k >= 8 && seeds == nullptr && !ctx->spill_pairs && !ctx->spill_packed) {
        // The quad route's workgroups meet at barriers: twice as many, half as long, when that fills the chip's 512 slots as
        // well (100 samples: 5 -> 10 parts, 500 -> 1000 workgroups), ends a launch with less of a tail: 13.09 against 13.18 ms.
        const uint64_t g1 = static_cast<uint64_t>(nsamples) * parts, g2 = 2 * g1;
        const double e1 = static_cast<double>(g1) / static_cast<double>((g1 + 511) / 512 * 512);
        const double e2 = static_cast<double>(g2) / static_cast<double>((g2 + 511) / 512 * 512);
        if (g2 <= 2048 && e2 >= e1 - 0.005 && p.maxlen / (2ull * parts) >= (1u << 20)) parts *= 2;
    }
    rc = ct_split(ctx, offsets, lengths, parts, &p);
    if (rc) return rc;
    SubParams sp{};
    const SubParams* sub = nullptr;
    if (seeds) {
        // seeds | thresholds travel like the descriptors (pageable source: the copy has read it on return)
        rc = ensure(ctx, reinterpret_cast<void**>(&ctx->d_sub), &ctx->sub_cap, 2ull * nsamples * sizeof(uint64_t));
        if (rc) return rc;
        VK_HIP(ctx, hipMemcpyAsync(ctx->d_sub, seeds, nsamples * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
        VK_HIP(ctx, hipMemcpyAsync(ctx->d_sub + nsamples, thresholds, nsamples * sizeof(uint64_t),
                                   hipMemcpyHostToDevice, ctx->stream));
        if (d_sites) VK_HIP(ctx, hipMemsetAsync(d_sites, 0, 2ull * nsamples * sizeof(uint64_t), ctx->stream));
        sp.seeds = ctx->d_sub;
        sp.thresholds = ctx->d_sub + nsamples;
        sp.sites = reinterpret_cast<unsigned long long*>(d_sites);
        sub = &sp;
    }
    rc = with_k(k, [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        if constexpr (K <= 7) return launch_count<K>(ctx, p, d_hist, sub);
        else return launch_spill<K>(ctx, p, d_hist, sub);
    });
    return rc ? rc : ct_finish(ctx, p, lengths, d_status);
}

int vk_count_device(vk_ctx* ctx, const void* d_fastq, const uint64_t* offsets, const uint64_t* lengths,
                    uint32_t nsamples, int k, uint32_t parts_per_sample, uint32_t* d_hist, uint32_t* d_status) {
    return count_impl(ctx, d_fastq, offsets, lengths, nsamples, k, parts_per_sample, d_hist, d_status, nullptr,
                      nullptr, nullptr);
}

int vk_count_sampled_device(vk_ctx* ctx, const void* d_fastq, const uint64_t* offsets, const uint64_t* lengths,
                            uint32_t nsamples, int k, uint32_t parts_per_sample, const uint64_t* seeds,
                            const uint64_t* thresholds, uint32_t* d_hist, uint32_t* d_status, uint64_t* d_sites) {
    if (!seeds || !thresholds) return VK_EINVAL;
    for (uint32_t i = 0; i < nsamples; ++i)
        if (thresholds[i] > (1ull << 32)) return VK_EINVAL;
    return count_impl(ctx, d_fastq, offsets, lengths, nsamples, k, parts_per_sample, d_hist, d_status, seeds,
                      thresholds, d_sites);
}

}  // extern "C"

namespace {

// Workspace and descriptors of a read index over the samples of a call (vk_ladder.h): *ip describes it, *p is the split
// the index is laid out for.  The samples' descriptors are on the device (ctx->d_desc) on return.
int index_prepare(vk_ctx* ctx, const void* d_fastq, const uint64_t* offsets, const uint64_t* lengths, uint32_t nsamples,
                  uint32_t parts_per_sample, IndexParams* ip, CtPlan* p) {
    ctx->ix_fastq = nullptr;
    ctx->ix_sample.clear();
    int rc = ct_check(ctx, d_fastq, offsets, lengths, nsamples, p);
    if (rc) return rc;
    // (the walker runs a workgroup per (subsample, part) of this split: the rule of rounds 2-5, one round of the chip)
    rc = ct_split(ctx, offsets, lengths, parts_per_sample ? parts_per_sample : choose_parts(nsamples, p->maxlen, 9), p);
    if (rc) return rc;
    // anchors: a sample's region holds one per 32 bytes of text, and eight per wavefront on top
    std::vector<uint64_t> base(nsamples);
    uint64_t total = 0;
    for (uint32_t i = 0; i < nsamples; ++i) {
        base[i] = total;
        total += lengths[i] / 32 + 8ull * p->parts * kWaves + 16;
    }
    uint64_t* d_base = nullptr;
    size_t zeroed = 0, end = 0;
    rc = ws_carve(ctx, &ctx->d_index, &ctx->index_cap, [&](WsTake& take) {
        take(ip->anchors, total);
        take(d_base, nsamples);
        take(ip->count, p->nwaves);
        zeroed = take.at;   // cleared per call: the site counters and overflow flags
        take(ip->sites, nsamples);
        take(ip->overflow, nsamples);
        end = take.at;
    });
    if (rc) return rc;
    ip->base = d_base;
    VK_HIP(ctx, hipMemcpyAsync(d_base, base.data(), nsamples * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (base is a temporary)
    VK_HIP(ctx, hipMemsetAsync(ctx->d_index + zeroed, 0, end - zeroed, ctx->stream));
    return VK_OK;
}

// The index is filled and d_status holds the samples' status words: bring sites, overflow flags and status to the host and
// remember which samples the index covers.
int index_finish(vk_ctx* ctx, const void* d_fastq, const uint64_t* offsets, const uint64_t* lengths, uint32_t nsamples,
                 const IndexParams& ip, uint32_t parts, const uint32_t* d_status, uint64_t* sites, uint32_t* status) {
    ctx->ix_status.assign(nsamples, 0u);
    ctx->ix_overflow.assign(nsamples, 0u);
    VK_HIP(ctx, hipMemcpyAsync(sites, ip.sites, nsamples * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(ctx->ix_overflow.data(), ip.overflow, nsamples * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(ctx->ix_status.data(), d_status, nsamples * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t i = 0; i < nsamples; ++i) {
        status[i] = ctx->ix_status[i];
        ctx->ix_sample[std::make_pair(offsets[i], lengths[i])] = i;
    }
    ctx->ix = ip;
    ctx->ix_fastq = d_fastq;
    ctx->ix_parts = parts;
    return VK_OK;
}

}  // namespace

extern "C" {

int vk_read_index_device(vk_ctx* ctx, const void* d_fastq, const uint64_t* offsets, const uint64_t* lengths, uint32_t nsamples,
                         uint32_t parts_per_sample, uint64_t* sites, uint32_t* status) {
    if (!ctx || !offsets || !lengths || !sites || !status) return VK_EINVAL;
    ctx->ix_fastq = nullptr;
    ctx->ix_sample.clear();
    if (nsamples == 0) return VK_OK;
    IndexParams ip;
    CtPlan p;
    int rc = index_prepare(ctx, d_fastq, offsets, lengths, nsamples, parts_per_sample, &ip, &p);
    if (rc) return rc;
    rc = ensure(ctx, reinterpret_cast<void**>(&ctx->d_status1), &ctx->status1_cap, nsamples * sizeof(uint32_t) + 64);
    if (rc) return rc;
    hipLaunchKernelGGL(vk_index_kernel, dim3(nsamples * p.parts), dim3(kCountThreads), 0, ctx->stream, p.fq, p.d_offs, p.d_lens,
                       nsamples, p.parts, ip, ctx->d_wavephase);
    VK_HIP(ctx, hipGetLastError());
    rc = ct_finish(ctx, p, nullptr, ctx->d_status1);
    if (rc) return rc;
    return index_finish(ctx, d_fastq, offsets, lengths, nsamples, ip, p.parts, ctx->d_status1, sites, status);
}

int vk_count_index_device(vk_ctx* ctx, const void* d_fastq, const uint64_t* offsets, const uint64_t* lengths, uint32_t nsamples, int k,
                          uint32_t parts_per_sample, uint32_t* d_hist, uint32_t* d_status, uint64_t* sites, uint32_t* status) {
    if (!ctx || !offsets || !lengths || !d_hist || !d_status || !sites || !status || k < 5 || k > 9) return VK_EINVAL;
    ctx->ix_fastq = nullptr;
    ctx->ix_sample.clear();
    if (nsamples == 0) return VK_OK;
    if (k > 7) {   // the spill path has no index mode: the index in a pass of its own, then the count
        int rc = vk_read_index_device(ctx, d_fastq, offsets, lengths, nsamples, parts_per_sample, sites, status);
        if (rc) return rc;
        return vk_count_device(ctx, d_fastq, offsets, lengths, nsamples, k, parts_per_sample, d_hist, d_status);
    }
    IndexParams ip;
    CtPlan p;
    int rc = index_prepare(ctx, d_fastq, offsets, lengths, nsamples, parts_per_sample, &ip, &p);
    if (rc) return rc;
    rc = with_k(k, [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        if constexpr (K <= 7) return launch_count<K>(ctx, p, d_hist, nullptr, &ip);
        else return VK_EINVAL;   // (handled above)
    });
    if (rc) return rc;
    rc = ct_finish(ctx, p, lengths, d_status);
    if (rc) return rc;
    return index_finish(ctx, d_fastq, offsets, lengths, nsamples, ip, p.parts, d_status, sites, status);
}

int vk_image_device(vk_ctx* ctx, const uint32_t* d_hist, uint32_t nsamples, int k, uint8_t* d_img) {
    if (!ctx || !d_hist || !d_img || k < 5 || k > 9) return VK_EINVAL;
    if (!ctx->d_pix[k]) return VK_ENOMAP;
    if (nsamples == 0) return VK_OK;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t npix = ctx->npix[k];
    const uint32_t npad = npad_of(npix);
    const size_t work = static_cast<size_t>(nsamples) * 2u * npad * sizeof(uint32_t);
    int rc = ensure(ctx, reinterpret_cast<void**>(&ctx->d_scratch), &ctx->scratch_cap,
                    work + static_cast<size_t>(nsamples) * sizeof(uint32_t));
    if (rc) return rc;
    const uint32_t* gate = nullptr;
#ifndef VK_IMAGE_COUNT_FROM
#define VK_IMAGE_COUNT_FROM 8192u   // padded pixels from which the order statistics are counted instead of sorted: k >= 7 (round 5: k = 7 too -- 1000 images 0.84 -> 0.23 ms)
#endif
    if (npad >= VK_IMAGE_COUNT_FROM && !ctx->image_sort_only) {
        // order statistics by counting; samples it cannot finish are flagged for the sort
        uint32_t* flags = ctx->d_scratch + work / sizeof(uint32_t);
        // the scatter first, spread over the device (vk_image.h); a batch too large for one grid keeps it in the kernel
        const int scattered = nsamples <= 65535u ? 1 : 0;
        if (scattered) {
            VK_HIP(ctx, hipMemsetAsync(ctx->d_scratch, 0, work, ctx->stream));
            hipLaunchKernelGGL(vk_image_scatter_kernel, dim3((1u << (2 * k)) / 256u, nsamples), dim3(256), 0, ctx->stream, d_hist,
                               ctx->d_pix[k], k, npad, ctx->d_scratch);
            VK_HIP(ctx, hipGetLastError());
        }
        hipLaunchKernelGGL(vk_image_count_kernel, dim3(nsamples), dim3(kImgThreads), 0, ctx->stream, d_hist,
                           ctx->d_pix[k], k, npix, npad, ctx->d_scratch, d_img, flags, scattered);
        VK_HIP(ctx, hipGetLastError());
        gate = flags;
    }
    hipLaunchKernelGGL(vk_image_kernel, dim3(nsamples), dim3(kImgThreads), 0, ctx->stream, d_hist, ctx->d_pix[k], k,
                       npix, npad, ctx->d_scratch, d_img, gate);
    VK_HIP(ctx, hipGetLastError());
    return VK_OK;
}

int vk_fastq_to_image_device(vk_ctx* ctx, const void* d_fastq, const uint64_t* offsets, const uint64_t* lengths,
                             uint32_t nsamples, int k, uint32_t parts_per_sample, uint32_t* d_hist,
                             uint32_t* d_status, uint8_t* d_img) {
    if (!ctx || k < 5 || k > 9) return VK_EINVAL;
    if (!ctx->d_pix[k]) return VK_ENOMAP;
    int rc = vk_count_device(ctx, d_fastq, offsets, lengths, nsamples, k, parts_per_sample, d_hist, d_status);
    if (rc) return rc;
    return vk_image_device(ctx, d_hist, nsamples, k, d_img);
}

int vk_count_host(vk_ctx* ctx, const uint8_t* fastq, size_t nbytes, int k, uint32_t* hist, uint32_t* status) {
    if (!ctx || !hist || k < 5 || k > 9 || (nbytes && !fastq)) return VK_EINVAL;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ncode = static_cast<size_t>(1) << (2 * k);
    int rc = ensure(ctx, reinterpret_cast<void**>(&ctx->d_stage), &ctx->stage_cap, nbytes + 64);
    if (rc) return rc;
    if (!ctx->d_hist1) VK_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->d_hist1), (1u << 18) * sizeof(uint32_t)));
    {
        const int rcs = ensure(ctx, reinterpret_cast<void**>(&ctx->d_status1), &ctx->status1_cap, 64);
        if (rcs) return rcs;
    }
    if (nbytes)
        VK_HIP(ctx, hipMemcpyAsync(ctx->d_stage, fastq, nbytes, hipMemcpyHostToDevice, ctx->stream));
    uint64_t off = 0, len = nbytes;
    rc = vk_count_device(ctx, ctx->d_stage, &off, &len, 1, k, 0, ctx->d_hist1, ctx->d_status1);
    if (rc) return rc;
    uint32_t st = 0;
    VK_HIP(ctx, hipMemcpyAsync(hist, ctx->d_hist1, ncode * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(&st, ctx->d_status1, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (status) *status = st;
    return st ? VK_EFORMAT : VK_OK;
}

int vk_image_host(vk_ctx* ctx, const uint32_t* hist, int k, uint8_t* img) {
    if (!ctx || !hist || !img || k < 5 || k > 9) return VK_EINVAL;
    if (!ctx->d_pix[k]) return VK_ENOMAP;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ncode = static_cast<size_t>(1) << (2 * k);
    if (!ctx->d_hist1) VK_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->d_hist1), (1u << 18) * sizeof(uint32_t)));
    if (!ctx->d_img1) VK_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->d_img1), 1u << 18));
    VK_HIP(ctx, hipMemcpyAsync(ctx->d_hist1, hist, ncode * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    int rc = vk_image_device(ctx, ctx->d_hist1, 1, k, ctx->d_img1);
    if (rc) return rc;
    VK_HIP(ctx, hipMemcpyAsync(img, ctx->d_img1, ctx->npix[k], hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VK_OK;
}

}  // extern "C"

// ---- vk_inflate_device: the plans and decisions are vk_gzplan.h's, the workspaces and launches are here ----
namespace {

static_assert(kGzOverflow == VK_GZ_OVERFLOW && kGzBadCrc == VK_GZ_BAD_CRC, "vk_gzplan.h sets the status bits of vkimg.h");

// d_gzcrc
struct GzCrcLayout {
    GzCrcJob* jobs;
    uint32_t* seg_job;   // per segment: its job
    uint32_t* ops;       // GzCrcOps::op
    uint32_t* seg;       // per segment: its remainder
    uint32_t* raw;       // per job: the zero-preset remainder of its text
};

// CRC-32 of texts resident on the device (vk_inflate.h, "CRC-32 of the inflated text"): crc[i] for every job.
int gz_text_crc(vk_ctx* ctx, const uint8_t* text, const std::vector<GzCrcJob>& jobs_in, std::vector<uint32_t>& crc) {
    std::vector<GzCrcJob> jobs = jobs_in;
    std::vector<uint32_t> seg_job;
    for (size_t j = 0; j < jobs.size(); ++j) {
        jobs[j].seg0 = static_cast<uint32_t>(seg_job.size());
        jobs[j].nseg = static_cast<uint32_t>((jobs[j].text_len + 65535) / 65536);
        seg_job.insert(seg_job.end(), jobs[j].nseg, static_cast<uint32_t>(j));
    }
    const uint32_t nj = static_cast<uint32_t>(jobs.size()), ns = static_cast<uint32_t>(seg_job.size());
    crc.assign(nj, 0u);
    const GzCrcOps& ops = gz_crc_ops();
    if (ns != 0) {
        GzCrcLayout L{};
        int rc = ws_carve(ctx, &ctx->d_gzcrc, &ctx->gzcrc_cap, [&](WsTake& take) {
            take(L.jobs, nj);
            take(L.seg_job, ns);
            take(L.ops, sizeof(ops.op) / sizeof(uint32_t));
            take(L.seg, ns);
            take(L.raw, nj);
        });
        if (rc) return rc;
        VK_HIP(ctx, hipMemcpyAsync(L.jobs, jobs.data(), nj * sizeof(GzCrcJob), hipMemcpyHostToDevice, ctx->stream));
        VK_HIP(ctx, hipMemcpyAsync(L.seg_job, seg_job.data(), ns * 4ull, hipMemcpyHostToDevice, ctx->stream));
        VK_HIP(ctx, hipMemcpyAsync(L.ops, ops.op, sizeof(ops.op), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(vk_crc32_seg_kernel, dim3((ns + 3) / 4), dim3(256), 0, ctx->stream, text, L.jobs, nj, L.seg_job, ns, L.ops, L.seg);
        VK_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(vk_crc32_fold_kernel, dim3(nj), dim3(64), 0, ctx->stream, L.jobs, nj, L.ops, L.seg, L.raw);
        VK_HIP(ctx, hipGetLastError());
        VK_HIP(ctx, hipMemcpyAsync(crc.data(), L.raw, nj * 4ull, hipMemcpyDeviceToHost, ctx->stream));
        VK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (also keeps jobs and seg_job alive until the copies have read them)
    }
    // zero-preset remainder -> CRC-32: the preset 0xFFFFFFFF shifted over the text, and the final inversion
    for (uint32_t j = 0; j < nj; ++j) crc[j] ^= ops.shift(0xFFFFFFFFu, jobs[j].text_len) ^ 0xFFFFFFFFu;
    return VK_OK;
}

// The arguments of a vk_inflate_device call.
struct GzCall {
    const uint8_t* gz;
    uint8_t* out;
    const uint64_t *gz_offsets, *gz_lengths, *out_offsets, *out_caps;
    uint64_t* out_lengths;
    uint32_t* status;
};

// What a stage's kernel reports is ONE run of pieces, so that one copy brings it back: the same statement of pieces lays out
// the run in the device's workspace and, over a host buffer, its mirror.
void gz_chunk_results(WsTake& take, GzChunkResults& r, size_t nc) {
    take(r.len, nc);
    take(r.status, nc);
    take(r.next, nc);
    take(r.isize, nc);
    take(r.nmem, nc);
    take(r.rec, nc * kGzMemRec);
}

// The chunked path, steps (1) and (2): the chunks of `plan` decoded into d_gzsym, what they report on the host (h: pointers
// into `mirror`).  d_gzmeta holds the chunk table and the results here; no pointer into it leaves this function, because
// gz_chunks_write carves the buffer anew.
int gz_chunks_decode(vk_ctx* ctx, const uint8_t* gz, const GzChunkPlan& plan, std::vector<uint8_t>& mirror, GzChunkResults& h) {
    const uint32_t nc = static_cast<uint32_t>(plan.chunks.size());
    GzChunk* d_chunks = nullptr;
    uint64_t* d_starts = nullptr;
    uint32_t* d_crc = nullptr;   // the last member's check word per chunk: written by the kernel, not read by the host
    GzChunkResults d{};
    size_t res_at = 0, res_bytes = 0;
    int rc = ws_carve(ctx, &ctx->d_gzmeta, &ctx->gzmeta_cap, [&](WsTake& take) {
        take(d_chunks, nc);
        take(d_starts, nc);
        take(d_crc, nc);
        res_at = take.at;
        gz_chunk_results(take, d, nc);
        res_bytes = take.at - res_at;
    });
    if (rc) return rc;
    uint16_t* d_sym = nullptr;
    rc = ws_carve(ctx, &ctx->d_gzsym, &ctx->gzsym_cap, [&](WsTake& take) { take(d_sym, plan.sym_total + 128); });   // (256 bytes to spare)
    if (rc) return rc;
    mirror.resize(res_bytes);
    WsTake host{mirror.data(), 0};
    gz_chunk_results(host, h, nc);
    VK_HIP(ctx, hipMemcpyAsync(d_chunks, plan.chunks.data(), nc * sizeof(GzChunk), hipMemcpyHostToDevice, ctx->stream));
    if (ctx->gz_split_find) {
        hipLaunchKernelGGL(vk_gzfind_kernel, dim3(nc), dim3(64), 0, ctx->stream, gz, d_chunks, nc, d_starts);
        VK_HIP(ctx, hipGetLastError());
    } else {
        VK_HIP(ctx, hipMemsetAsync(d_starts, 0xFE, nc * 8ull, ctx->stream));   // kGzPending: the chunks' wavefronts find their own starts
    }
    hipLaunchKernelGGL(vk_gzchunk_kernel, dim3(nc), dim3(64), ctx->gz_lds_pad, ctx->stream, gz, d_sym, d_chunks, nc, d_starts, d.len,
                       d.status, d.next, d.isize, d.nmem, d_crc, reinterpret_cast<uint2*>(d.rec), ctx->gz_split_find ? 0u : 1u);
    VK_HIP(ctx, hipGetLastError());
    VK_HIP(ctx, hipMemcpyAsync(mirror.data(), ctx->d_gzmeta + res_at, res_bytes, hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the chunk table is read by the copy: the plan is the caller's)
    return VK_OK;
}

// The chunked path, steps (3) and (4): the accepted files' windows handed on and their text written.  The chunk metadata
// has been read back and the stream synchronised (gz_chunks_decode): d_gzmeta now carries the items.
int gz_chunks_write(vk_ctx* ctx, uint8_t* out, const GzChains& ch) {
    const uint32_t ni = static_cast<uint32_t>(ch.items.size()), nf = static_cast<uint32_t>(ch.okfile.size());
    GzItem* d_items = nullptr;
    uint32_t *d_first = nullptr, *d_count = nullptr;
    int rc = ws_carve(ctx, &ctx->d_gzmeta, &ctx->gzmeta_cap, [&](WsTake& take) {
        take(d_items, ni);
        take(d_first, nf);
        take(d_count, nf);
    });
    if (rc) return rc;
    uint8_t* d_win = nullptr;
    rc = ws_carve(ctx, &ctx->d_gzwin, &ctx->gzwin_cap, [&](WsTake& take) { take(d_win, static_cast<size_t>(ni) * 32768 + 256); });
    if (rc) return rc;
    const uint16_t* d_sym = reinterpret_cast<const uint16_t*>(ctx->d_gzsym);
    VK_HIP(ctx, hipMemcpyAsync(d_items, ch.items.data(), ni * sizeof(GzItem), hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(d_first, ch.first.data(), nf * 4ull, hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(d_count, ch.count.data(), nf * 4ull, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(vk_gzwin_kernel, dim3(nf), dim3(1024), 0, ctx->stream, d_sym, d_items, d_first, d_count, d_win);
    VK_HIP(ctx, hipGetLastError());
    for (uint32_t i0 = 0; i0 < ni; i0 += 65535u) {  // (gridDim.y holds 65535 at most: 8 GiB of 128 KiB chunks)
        const uint32_t n = ni - i0 < 65535u ? ni - i0 : 65535u;
        hipLaunchKernelGGL(vk_gzfinal_kernel, dim3(32, n), dim3(256), 0, ctx->stream, d_sym, d_items + i0, n,
                           d_win + static_cast<size_t>(i0) * 32768, out);
        VK_HIP(ctx, hipGetLastError());
    }
    VK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (items / first / count are read by the kernels)
    return VK_OK;
}

// Large files: many wavefronts per file (vk_inflate.h, "the chunked path").  A file whose chain of chunks is sound gets its
// text, or learns the room it needs; the others join `direct`.
int gz_chunked_stage(vk_ctx* ctx, const GzCall& f, const std::vector<uint32_t>& big, std::vector<uint32_t>& direct, GzChecks& checks) {
    const uint32_t chunk_bytes = gz_fit_chunk_bytes(f.gz_lengths, big, static_cast<uint64_t>(ctx->num_cus) * kGzChunkWaves,
                                                    ctx->gz_chunk_bytes, ctx->gz_fill_pct);
    const GzChunkPlan plan = gz_chunk_table(chunk_bytes, f.gz_offsets, f.gz_lengths, f.out_caps, big);
    std::vector<uint8_t> mirror;
    GzChunkResults res{};
    int rc = gz_chunks_decode(ctx, f.gz, plan, mirror, res);
    if (rc) return rc;
    const GzChains ch = gz_walk_chains(plan, res, big, f.out_offsets, f.out_caps, checks);
    for (size_t b = 0; b < big.size(); ++b) {
        const GzVerdict& v = ch.verdict[b];
        if (v.kind == kGzGoDirect) {
            direct.push_back(big[b]);
        } else {
            f.status[big[b]] = v.status;
            f.out_lengths[big[b]] = v.total;
        }
    }
    return ch.okfile.empty() ? VK_OK : gz_chunks_write(ctx, f.out, ch);
}

// what vk_inflate_kernel reports per file: one run, as above
struct GzDirectResults {
    unsigned long long* len;
    uint32_t *status, *nmem;
    GzTrailer* rec;
};
void gz_direct_results(WsTake& take, GzDirectResults& r, size_t nd) {
    take(r.len, nd);
    take(r.status, nd);
    take(r.nmem, nd);
    take(r.rec, nd * kGzMemRec);
}

// Small files, and large ones the chunked path gave up on: one wavefront per file.
int gz_direct_stage(vk_ctx* ctx, const GzCall& f, const std::vector<uint32_t>& direct, GzChecks& checks) {
    const uint32_t nd = static_cast<uint32_t>(direct.size());
    GzJob* d_jobs = nullptr;
    uint32_t* d_crc = nullptr;   // (written by the kernel, not read by the host)
    GzDirectResults d{}, h{};
    size_t res_at = 0, res_bytes = 0;
    int rc = ws_carve(ctx, &ctx->d_gzjobs, &ctx->gzjobs_cap, [&](WsTake& take) {
        take(d_jobs, nd);
        take(d_crc, nd);
        res_at = take.at;
        gz_direct_results(take, d, nd);
        res_bytes = take.at - res_at;
    });
    if (rc) return rc;
    std::vector<uint8_t> mirror(res_bytes);
    WsTake host{mirror.data(), 0};
    gz_direct_results(host, h, nd);
    std::vector<GzJob> jobs(nd);
    for (uint32_t j = 0; j < nd; ++j) {
        const uint32_t i = direct[j];
        jobs[j] = GzJob{f.gz_offsets[i], f.gz_lengths[i], f.out_offsets[i], f.out_caps[i]};
    }
    VK_HIP(ctx, hipMemcpyAsync(d_jobs, jobs.data(), nd * sizeof(GzJob), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(vk_inflate_kernel, dim3(nd), dim3(64), 0, ctx->stream, f.gz, f.out, d_jobs, nd, d.len, d.status, d.nmem, d_crc,
                       reinterpret_cast<uint2*>(d.rec));
    VK_HIP(ctx, hipGetLastError());
    VK_HIP(ctx, hipMemcpyAsync(mirror.data(), ctx->d_gzjobs + res_at, res_bytes, hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (also keeps `jobs` alive until the copy has read it)
    std::vector<GzMember> members;
    for (uint32_t j = 0; j < nd; ++j) {
        const uint32_t i = direct[j];
        f.out_lengths[i] = h.len[j];
        f.status[i] = h.status[j] | gz_direct_checks(checks, i, h.status[j], h.nmem[j], h.rec + static_cast<size_t>(j) * kGzMemRec,
                                                     f.out_offsets[i], h.len[j], members);
    }
    return VK_OK;
}

}  // namespace

extern "C" {

int vk_inflate_device(vk_ctx* ctx, const void* d_gz, const uint64_t* gz_offsets, const uint64_t* gz_lengths,
                      uint32_t nfiles, void* d_out, const uint64_t* out_offsets, const uint64_t* out_caps,
                      uint64_t* out_lengths, uint32_t* status) {
    if (!ctx || !gz_offsets || !gz_lengths || !out_offsets || !out_caps || !out_lengths || !status) return VK_EINVAL;
    if (nfiles == 0) return VK_OK;
    if (!d_gz || !d_out) return VK_EINVAL;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    const GzCall f{static_cast<const uint8_t*>(d_gz), static_cast<uint8_t*>(d_out), gz_offsets, gz_lengths, out_offsets, out_caps,
                   out_lengths, status};
    std::vector<uint32_t> big, direct;  // files that are cut into chunks, files that go through the one-wavefront-per-file kernel
    for (uint32_t i = 0; i < nfiles; ++i) {
        out_lengths[i] = 0;
        status[i] = 0;
        if (!ctx->gz_no_chunks && gz_lengths[i] >= kGzBigFile) big.push_back(i);
        else direct.push_back(i);
    }
    GzChecks checks;
    int rc = big.empty() ? VK_OK : gz_chunked_stage(ctx, f, big, direct, checks);
    if (rc) return rc;
    rc = direct.empty() ? VK_OK : gz_direct_stage(ctx, f, direct, checks);
    if (rc) return rc;
    // the check word of every member against the CRC-32 of the text it inflated to
    if (!checks.jobs.empty()) {
        std::vector<uint32_t> got;
        rc = gz_text_crc(ctx, f.out, checks.jobs, got);
        if (rc) return rc;
        for (size_t j = 0; j < checks.jobs.size(); ++j)
            if (got[j] != checks.want[j]) status[checks.file[j]] |= VK_GZ_BAD_CRC;
    }
    return VK_OK;
}

int vk_synth_fastq_device(vk_ctx* ctx, void* d_out, uint32_t sample0, uint32_t nsamples, uint32_t reads,
                          uint32_t readlen, uint64_t seed, int dist) {
    if (!ctx || !d_out || readlen == 0 || reads == 0 || reads > 10000000u || (dist != 0 && dist != 1)) return VK_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_out) & 15u) != 0) return VK_EINVAL;
    if (nsamples == 0) return VK_OK;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t rec = 2ull * readlen + 20ull;
    const uint64_t total = rec * reads * nsamples;
    const uint64_t total16 = (total + 15) / 16;
    uint64_t blocks = (total16 + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(vk_synth_kernel, dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, ctx->stream,
                       static_cast<uint8_t*>(d_out), sample0, nsamples, reads, readlen, seed, dist, total16);
    VK_HIP(ctx, hipGetLastError());
    return VK_OK;
}

// dist 2 (vk_aux.h, "reads shaped like what step B hands to step D"): the record offsets of `n` samples in the
// context's workspace, n * (reads + 1) u32
static int synth_shapes(vk_ctx* ctx, uint32_t sample0, uint32_t n, uint32_t reads, uint32_t readlen, uint64_t seed) {
    int rc = ensure(ctx, reinterpret_cast<void**>(&ctx->d_synth), &ctx->synth_cap, static_cast<size_t>(n) * (reads + 1ull) * sizeof(uint32_t));
    if (rc) return rc;
    hipLaunchKernelGGL(vk_synth_shape_kernel, dim3(n), dim3(1024), 0, ctx->stream, ctx->d_synth, sample0, reads, readlen, seed);
    VK_HIP(ctx, hipGetLastError());
    return VK_OK;
}

int vk_synth_shaped_lengths(vk_ctx* ctx, uint32_t sample0, uint32_t nsamples, uint32_t reads, uint32_t readlen,
                            uint64_t seed, uint64_t* lengths) {
    if (!ctx || !lengths || readlen < 64 || readlen > 1000 || reads == 0 || reads > 4000000u) return VK_EINVAL;
    if (static_cast<uint64_t>(reads) * (74ull + 4ull * readlen) >= (1ull << 32)) return VK_EINVAL;   // record offsets are u32
    VK_HIP(ctx, hipSetDevice(ctx->device));
    constexpr uint32_t kSlab = 64;
    std::vector<uint32_t> tot(kSlab);
    for (uint32_t s0 = 0; s0 < nsamples; s0 += kSlab) {
        const uint32_t n = nsamples - s0 < kSlab ? nsamples - s0 : kSlab;
        int rc = synth_shapes(ctx, sample0 + s0, n, reads, readlen, seed);
        if (rc) return rc;
        VK_HIP(ctx, hipMemcpy2DAsync(tot.data(), sizeof(uint32_t), ctx->d_synth + reads, (reads + 1ull) * sizeof(uint32_t),
                                     sizeof(uint32_t), n, hipMemcpyDeviceToHost, ctx->stream));
        VK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (uint32_t i = 0; i < n; ++i) lengths[s0 + i] = tot[i];
    }
    return VK_OK;
}

int vk_synth_shaped_device(vk_ctx* ctx, void* d_out, const uint64_t* offsets, uint32_t sample0, uint32_t nsamples,
                           uint32_t reads, uint32_t readlen, uint64_t seed) {
    if (!ctx || !d_out || !offsets || readlen < 64 || readlen > 1000 || reads == 0 || reads > 4000000u) return VK_EINVAL;
    if (static_cast<uint64_t>(reads) * (74ull + 4ull * readlen) >= (1ull << 32)) return VK_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_out) & 15u) != 0) return VK_EINVAL;
    for (uint32_t i = 0; i < nsamples; ++i)
        if (offsets[i] & 15u) return VK_EINVAL;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    constexpr uint32_t kSlab = 64;
    const uint32_t chunks = (reads + 255u) / 256u;
    for (uint32_t s0 = 0; s0 < nsamples; s0 += kSlab) {
        const uint32_t n = nsamples - s0 < kSlab ? nsamples - s0 : kSlab;
        int rc = synth_shapes(ctx, sample0 + s0, n, reads, readlen, seed);
        if (rc) return rc;
        rc = ensure(ctx, reinterpret_cast<void**>(&ctx->d_synth_offs), &ctx->synth_offs_cap, kSlab * sizeof(uint64_t));
        if (rc) return rc;
        // (pageable source: the copy has read it on return)
        VK_HIP(ctx, hipMemcpyAsync(ctx->d_synth_offs, offsets + s0, n * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(vk_synth_shaped_kernel, dim3(n * chunks), dim3(256), 0, ctx->stream, static_cast<uint8_t*>(d_out),
                           ctx->d_synth_offs, ctx->d_synth, sample0 + s0, reads, readlen, seed);
        VK_HIP(ctx, hipGetLastError());
        VK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the workspaces are reused by the next slab
    }
    return VK_OK;
}

int vk_remap_host(vk_ctx* ctx, const uint8_t* img_in, uint32_t nimg, uint32_t npix_in, uint32_t npix_out,
                  const uint32_t* src0, const uint32_t* src1, const uint8_t* w0, const uint8_t* w1, int sum_rc,
                  uint8_t* img_out) {
    if (!ctx || !img_in || !img_out || !src0 || npix_in == 0 || npix_out == 0) return VK_EINVAL;
    if (sum_rc && (!src1 || !w0 || !w1)) return VK_EINVAL;
    if (nimg == 0) return VK_OK;
    for (uint32_t p = 0; p < npix_out; ++p) {
        if (src0[p] != 0xFFFFFFFFu && src0[p] >= npix_in) return VK_EINVAL;
        if (sum_rc && src1[p] != 0xFFFFFFFFu && src1[p] >= npix_in) return VK_EINVAL;
    }
    VK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t in_b = static_cast<size_t>(nimg) * npix_in, out_b = static_cast<size_t>(nimg) * npix_out;
    const size_t lut_b = static_cast<size_t>(npix_out) * 4;
    const size_t need = in_b + out_b + 2 * lut_b + 2 * npix_out + 256;
    int rc = ensure(ctx, reinterpret_cast<void**>(&ctx->d_stage), &ctx->stage_cap, need);
    if (rc) return rc;
    uint8_t* base = ctx->d_stage;
    uint32_t* d_s0 = reinterpret_cast<uint32_t*>(base);
    uint32_t* d_s1 = d_s0 + npix_out;
    uint8_t* d_w0 = reinterpret_cast<uint8_t*>(d_s1 + npix_out);
    uint8_t* d_w1 = d_w0 + npix_out;
    uint8_t* d_in = d_w1 + npix_out;
    uint8_t* d_out = d_in + in_b;
    VK_HIP(ctx, hipMemcpyAsync(d_s0, src0, lut_b, hipMemcpyHostToDevice, ctx->stream));
    if (sum_rc) {
        VK_HIP(ctx, hipMemcpyAsync(d_s1, src1, lut_b, hipMemcpyHostToDevice, ctx->stream));
        VK_HIP(ctx, hipMemcpyAsync(d_w0, w0, npix_out, hipMemcpyHostToDevice, ctx->stream));
        VK_HIP(ctx, hipMemcpyAsync(d_w1, w1, npix_out, hipMemcpyHostToDevice, ctx->stream));
    }
    VK_HIP(ctx, hipMemcpyAsync(d_in, img_in, in_b, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(vk_remap_kernel, dim3(nimg), dim3(256), 0, ctx->stream, d_in, npix_in, npix_out, d_s0, d_s1,
                       d_w0, d_w1, sum_rc, d_out);
    VK_HIP(ctx, hipGetLastError());
    VK_HIP(ctx, hipMemcpyAsync(img_out, d_out, out_b, hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VK_OK;
}

#ifdef VK_GZ_STAMPS
int vk_debug_read_gz_find(unsigned long long* out, uint32_t nchunks) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_gz_find), static_cast<size_t>(nchunks) * 8 * sizeof(unsigned long long)) == hipSuccess ? 0 : 2;
}
int vk_debug_read_gz_res(unsigned long long* out, uint32_t nchunks, int clear) {
    if (clear) {
        static unsigned long long zeros[16384 * 4];
        return hipMemcpyToSymbol(HIP_SYMBOL(g_gz_res), zeros, sizeof(zeros)) == hipSuccess ? 0 : 2;
    }
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_gz_res), static_cast<size_t>(nchunks) * 4 * sizeof(unsigned long long)) == hipSuccess ? 0 : 2;
}
int vk_debug_read_gz_stamps(unsigned long long* out, uint32_t nchunks) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_gz_stamps), static_cast<size_t>(nchunks) * 8 * sizeof(unsigned long long)) == hipSuccess ? 0 : 2;
}
#endif

#ifdef VK_STAMPS
int vk_debug_read_stamps(unsigned long long* out8) {
    return hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_vk_stamps), 8 * sizeof(unsigned long long)) == hipSuccess ? 0 : 2;
}
#endif

int vk_preprocess_device(vk_ctx* ctx, const uint8_t* d_img, uint32_t nimg, uint32_t side, uint32_t out,
                         const int32_t* bounds, const int32_t* coef, uint32_t kmax, float mean, float stdv,
                         float* d_out) {
    if (!ctx || !d_img || !d_out || !bounds || !coef || side == 0 || out == 0 || kmax == 0 || stdv == 0.0f)
        return VK_EINVAL;
    if (static_cast<size_t>(side) * out > 160u * 1024u - 1024u) return VK_EINVAL;  // LDS intermediate
    for (uint32_t i = 0; i < out; ++i) {
        const int32_t x0 = bounds[2 * i], n = bounds[2 * i + 1];
        if (x0 < 0 || n < 0 || static_cast<uint32_t>(n) > kmax || static_cast<uint32_t>(x0 + n) > side) return VK_EINVAL;
    }
    if (nimg == 0) return VK_OK;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t tb = static_cast<size_t>(out) * 2 * sizeof(int32_t), cb = static_cast<size_t>(out) * kmax * sizeof(int32_t);
    int rc = ensure(ctx, reinterpret_cast<void**>(&ctx->d_stage), &ctx->stage_cap, tb + cb + 256);
    if (rc) return rc;
    int32_t* d_bounds = reinterpret_cast<int32_t*>(ctx->d_stage);
    int32_t* d_coef = d_bounds + out * 2;
    VK_HIP(ctx, hipMemcpyAsync(d_bounds, bounds, tb, hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(d_coef, coef, cb, hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the host tables may be temporaries
    const size_t lds = static_cast<size_t>(side) * out;
    VK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(vk_preprocess_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
    hipLaunchKernelGGL(vk_preprocess_kernel, dim3(nimg), dim3(256), lds, ctx->stream, d_img, side, out, d_bounds,
                       d_coef, kmax, mean, stdv, d_out);
    VK_HIP(ctx, hipGetLastError());
    return VK_OK;
}

int vk_train_batch_device(vk_ctx* ctx, const uint8_t* d_img, uint32_t nset, uint32_t side, uint32_t out,
                          const int32_t* bounds, const int32_t* coef, uint32_t kmax, float mean, float stdv,
                          uint32_t batch, const uint32_t* idx, const uint32_t* partner, const float* lam,
                          const float* bshift, const float* cscale, uint32_t x1, uint32_t y1, uint32_t x2,
                          uint32_t y2, int mode, float* d_out) {
    if (!ctx || !d_img || !d_out || !bounds || !coef || side == 0 || out == 0 || kmax == 0 || stdv == 0.0f)
        return VK_EINVAL;
    if (!idx || !partner || !lam || !bshift || !cscale || nset == 0 || mode < 0 || mode > 2) return VK_EINVAL;
    if (side > 32768u || out > 32768u) return VK_EINVAL;   // (pixel counts stay below 2^31)
    const bool resize = out != side;
    if (resize && static_cast<size_t>(side) * out + kTrainLutBytes > 160u * 1024u) return VK_EINVAL;  // LDS intermediate
    for (uint32_t i = 0; i < out; ++i) {
        const int32_t x0 = bounds[2 * i], n = bounds[2 * i + 1];
        if (x0 < 0 || n < 0 || static_cast<uint32_t>(n) > kmax || static_cast<uint32_t>(x0 + n) > side) return VK_EINVAL;
        // out == side: the kernel reads the source pixels themselves, so the tables must say exactly that
        if (!resize && (static_cast<uint32_t>(x0) != i || n != 1 || coef[static_cast<size_t>(i) * kmax] != (1 << 22)))
            return VK_EINVAL;
    }
    if (x1 > x2 || x2 > out || y1 > y2 || y2 > out) return VK_EINVAL;
    for (uint32_t i = 0; i < batch; ++i) {
        if (idx[i] >= nset || partner[i] >= batch) return VK_EINVAL;
        if (!(lam[i] >= 0.0f && lam[i] <= 1.0f)) return VK_EINVAL;   // (refuses NaN too)
        if (!std::isfinite(bshift[i]) || !std::isfinite(cscale[i])) return VK_EINVAL;
    }
    if (batch == 0) return VK_OK;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    // one host block, one copy: [bounds | coef | idx | partner | lam | bshift | cscale], all 4-byte words
    const size_t nb = static_cast<size_t>(out) * 2, nc = static_cast<size_t>(out) * kmax;
    std::vector<uint32_t> h(nb + nc + 5 * static_cast<size_t>(batch));
    uint32_t* w = h.data();
    memcpy(w, bounds, nb * 4);
    memcpy(w += nb, coef, nc * 4);
    memcpy(w += nc, idx, batch * 4u);
    memcpy(w += batch, partner, batch * 4u);
    memcpy(w += batch, lam, batch * 4u);
    memcpy(w += batch, bshift, batch * 4u);
    memcpy(w += batch, cscale, batch * 4u);
    int rc = ensure(ctx, reinterpret_cast<void**>(&ctx->d_stage), &ctx->stage_cap, h.size() * 4 + 256);
    if (rc) return rc;
    VK_HIP(ctx, hipMemcpyAsync(ctx->d_stage, h.data(), h.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the host block goes away
    const int32_t* d_bounds = reinterpret_cast<const int32_t*>(ctx->d_stage);
    const int32_t* d_coef = d_bounds + nb;
    const uint32_t* d_idx = reinterpret_cast<const uint32_t*>(d_coef + nc);
    const uint32_t* d_partner = d_idx + batch;
    const float* d_lam = reinterpret_cast<const float*>(d_partner + batch);
    const float* d_bshift = d_lam + batch;
    const float* d_cscale = d_bshift + batch;
    const size_t lds = kTrainLutBytes + (resize ? (static_cast<size_t>(side) * out + 15) / 16 * 16 : 0);
    // four pixels per thread where every uchar4 / float4 access is aligned
    const bool wide = out % 4 == 0 && reinterpret_cast<uintptr_t>(d_out) % 16 == 0 &&
                      (resize || reinterpret_cast<uintptr_t>(d_img) % 4 == 0);
    auto kernel = wide ? vk_train_batch_kernel<4> : vk_train_batch_kernel<1>;
    VK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    static_cast<int>(lds)));
    hipLaunchKernelGGL(kernel, dim3(batch), dim3(256), lds, ctx->stream, d_img, side, out, d_bounds, d_coef, kmax, mean,
                       stdv, d_idx, d_partner, d_lam, d_bshift, d_cscale, x1, y1, x2, y2, mode, d_out);
    VK_HIP(ctx, hipGetLastError());
    return VK_OK;
}

int vk_last_count_general(vk_ctx* ctx, uint64_t* general_pieces, uint64_t* pieces) {
    if (!ctx || !general_pieces || !pieces) return VK_EINVAL;
    *general_pieces = 0;
    *pieces = 0;
    if (ctx->last_waves == 0) return VK_OK;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint32_t> w(ctx->last_waves);
    VK_HIP(ctx, hipMemcpyAsync(w.data(), ctx->d_wavephase, w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t g = 0, active = 0;
    for (uint32_t v : w) {
        if (v & 0x80u) continue;
        ++active;
        g += v >> 8;
    }
    *general_pieces = g;
    // every wave's range starts one 64-byte block early and ends with a partial piece: about one piece per wave on top
    *pieces = (ctx->last_bytes + kPiece - 1) / kPiece + active;
    return VK_OK;
}

int vk_last_count_pull(vk_ctx* ctx, uint32_t* helpers, uint32_t* flushes, uint32_t nsamples) {
    if (!ctx || !helpers || (nsamples && !flushes)) return VK_EINVAL;
    *helpers = 0;
    for (uint32_t i = 0; i < nsamples; ++i) flushes[i] = 0;
    if (ctx->last_pull_samples == 0) return VK_OK;
    if (nsamples > ctx->last_pull_samples) return VK_EINVAL;
    *helpers = ctx->last_helpers;
    if (nsamples == 0) return VK_OK;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t* d_flushes = ctx->d_pull + 2 + ctx->last_pull_samples;   // (vk_count.h, PullParams)
    VK_HIP(ctx, hipMemcpyAsync(flushes, d_flushes, nsamples * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VK_OK;
}

int vk_last_count_launch(const vk_ctx* ctx, uint32_t* grid, uint32_t* block, uint32_t* lds_bytes) {
    if (!ctx) return VK_EINVAL;
    if (grid) *grid = ctx->last_grid;
    if (block) *block = ctx->last_block;
    if (lds_bytes) *lds_bytes = ctx->last_lds;
    return VK_OK;
}

}  // extern "C"

// ------------------------------------------------------------- step B ---------

namespace {

// the pieces of a vk_clean_device workspace (ClLayout: vk_textplan.h)
ClLayout cl_layout(void* d_ws, const uint64_t* lengths, const uint64_t* records, uint32_t nfiles, uint32_t nsamples) {
    ClLayout L{};
    for (uint32_t i = 0; i < nfiles; ++i) {
        L.nchunks += (lengths[i] + kClChunk - 1) / kClChunk;
        L.nrec += records[i];
    }
    L.nslots = 1024;
    while (L.nslots < 2 * L.nrec) L.nslots <<= 1;
    const uint64_t nb = std::max((L.nchunks + kClScanBlock - 1) / kClScanBlock, (L.nrec + kClScanBlock - 1) / kClScanBlock);
    WsTake take{static_cast<uint8_t*>(d_ws), 0};
    take(L.files, nfiles);
    take(L.fchunk, nfiles);
    take(L.samples, nsamples);
    take(L.unit_base, nsamples + 1ull);
    take(L.ccount, L.nchunks);
    take(L.cprefix, L.nchunks + 1);
    take(L.sums, nb + 1);
    take(L.recs, L.nrec);
    take(L.hashes, L.nrec);
    take(L.slot_of, L.nrec);
    take(L.plans, L.nrec);
    take(L.obytes, L.nrec);
    take(L.oprefix, L.nrec + 1);
    take(L.table, 2 * L.nslots);   // (a slot is two words)
    L.total = take.at;
    return L;
}

// the pieces of a vk_clean_detect_device workspace: the record index of vk_clean_device's layout, then a slice's tables
struct AdLayout {
    ClLayout c;
    uint32_t *hist, *counts;
    AdGroup* groups;
    uint64_t *gbase, *ranked, *totals;
    AdCand* cands;
    AdExt* ext;
    size_t total;
    uint32_t slice;
};

AdLayout ad_layout(void* d_ws, const uint64_t* lengths, const uint64_t* records, uint32_t nfiles, uint32_t nsamples) {
    AdLayout L{};
    L.c = cl_layout(d_ws, lengths, records, nfiles, nsamples);
    L.slice = static_cast<uint32_t>(std::min<uint64_t>(kAdSlice, 3ull * nsamples));
    WsTake take{static_cast<uint8_t*>(d_ws), L.c.total};
    take(L.hist, static_cast<size_t>(L.slice) * kAdKeys);
    take(L.groups, L.slice);
    take(L.gbase, L.slice + 1ull);
    take(L.ranked, L.slice * kAdTop);
    take(L.totals, L.slice);
    take(L.cands, L.slice * kAdTop);
    take(L.counts, L.slice * kAdTop);
    take(L.ext, L.slice * kAdTop);
    L.total = take.at;
    return L;
}

int cl_scan(vk_ctx* ctx, const uint64_t* in, uint64_t n, uint64_t* sums, uint64_t* out) {
    VK_HIP(ctx, hipMemsetAsync(out, 0, sizeof(uint64_t), ctx->stream));   // (n = 0: out[0] = 0)
    if (n == 0) return VK_OK;
    const uint64_t nb = (n + kClScanBlock - 1) / kClScanBlock;
    hipLaunchKernelGGL(vk_cl_scan_reduce_kernel, dim3(nb), dim3(kClThreads), 0, ctx->stream, in, n, sums);
    hipLaunchKernelGGL(vk_cl_scan_top_kernel, dim3(1), dim3(kClThreads), 0, ctx->stream, sums, nb);
    hipLaunchKernelGGL(vk_cl_scan_apply_kernel, dim3(nb), dim3(kClThreads), 0, ctx->stream, in, n, sums, out);
    VK_HIP(ctx, hipGetLastError());
    return VK_OK;
}

// (cl_rank, cl_order, ClIndex and cl_index, the host's statement of the record index: vk_textplan.h)

// Uploads the index's tables and has the GPU find every record's line ends.  The sample rows and the stats and status
// words that the init kernel resets are vk_clean_device's; detection has none (nulls, nsamples 0).
int cl_index_run(vk_ctx* ctx, const uint8_t* text, const ClIndex& ix, const ClLayout& L, const ClSample* dsmp, uint32_t nsamples,
                 uint64_t* d_stats, uint32_t* d_status) {
    const uint32_t nfiles = static_cast<uint32_t>(ix.files.size());
    if (nfiles) {
        VK_HIP(ctx, hipMemcpyAsync(L.files, ix.files.data(), nfiles * sizeof(ClFile), hipMemcpyHostToDevice, ctx->stream));
        VK_HIP(ctx, hipMemcpyAsync(L.fchunk, ix.fchunk.data(), nfiles * 8ull, hipMemcpyHostToDevice, ctx->stream));
    }
    if (ix.nrec) VK_HIP(ctx, hipMemsetAsync(L.recs, 0xFF, ix.nrec * sizeof(ClRec), ctx->stream));
    const uint32_t ninit = std::max(nsamples, nfiles);
    hipLaunchKernelGGL(vk_cl_init_kernel, dim3((ninit + kClThreads - 1) / kClThreads), dim3(kClThreads), 0, ctx->stream, dsmp,
                       nsamples, L.files, nfiles, L.recs, d_stats, d_stats ? static_cast<uint32_t>(VK_CL_NSTAT) : 0u, d_status);
    if (ix.nchunks) {
        hipLaunchKernelGGL(vk_cl_nl_count_kernel, dim3(ix.nchunks), dim3(kClThreads), 0, ctx->stream, text, L.files, L.fchunk,
                           nfiles, L.ccount);
        int rc = cl_scan(ctx, L.ccount, ix.nchunks, L.sums, L.cprefix);
        if (rc) return rc;
        hipLaunchKernelGGL(vk_cl_nl_write_kernel, dim3(ix.nchunks), dim3(kClThreads), 0, ctx->stream, text, L.files, L.fchunk,
                           nfiles, L.cprefix, L.recs);
    }
    VK_HIP(ctx, hipGetLastError());
    return VK_OK;
}

// what vk_clean_device and vk_clean_detect_device ask of the arguments they share
int cl_check(const vk_ctx* ctx, const void* d_text, const uint64_t* offsets, const uint64_t* lengths, const uint64_t* records,
             const uint32_t* roles, const uint32_t* samples, uint32_t nfiles, uint32_t nsamples, uint32_t trim_tail,
             const void* d_ws) {
    if (!ctx || nsamples == 0 || !d_ws || trim_tail > (1u << 30)) return VK_EINVAL;
    if (nfiles && (!d_text || !offsets || !lengths || !records || !roles || !samples)) return VK_EINVAL;
    uint64_t nrec = 0;
    for (uint32_t i = 0; i < nfiles; ++i) {
        if (samples[i] >= nsamples || roles[i] > VK_CL_ROLE_R2 || offsets[i] % 16) return VK_EINVAL;
        nrec += records[i];
    }
    return nrec >= kClEmpty ? VK_EINVAL : VK_OK;   // (the dedup table holds unit ordinals as 32-bit words, kClEmpty for a free slot)
}

// an adapter triple table as the clean kernel reads it: each sequence's bytes, 2-bit codes and non-ACGT marks
std::vector<ClAdapter> ad_pack(const uint32_t* ad_lengths, const uint8_t* ad_seqs, uint64_t ngroups) {
    std::vector<ClAdapter> ads(ngroups);
    for (uint64_t g = 0; g < ngroups; ++g) {
        ClAdapter& d = ads[g];
        d = ClAdapter{};
        d.len = ad_lengths[g];
        for (uint32_t i = 0; i < d.len; ++i) {
            const uint8_t b = ad_seqs[g * kAdMaxAdapter + i];
            const uint64_t c = (b >> 1) & 3u, bad = (b == 'A' || b == 'C' || b == 'G' || b == 'T') ? 0u : 1u;
            d.seq[i] = b;
            (i < 32 ? d.lo : d.hi) |= c << (2 * (i % 32));
            (i < 32 ? d.nlo : d.nhi) |= bad << (2 * (i % 32));
        }
    }
    return ads;
}

// A slice's candidates: ranked keys with count * 4^10 / total > 20; each gets room for `count` occurrences (the
// extension's positions are a part of the counted ones).  Returns the room of all.
uint64_t ad_candidates(const std::vector<uint64_t>& ranked, const std::vector<uint64_t>& totals, std::vector<AdCand>& cand) {
    uint64_t nocc = 0;
    for (size_t k = 0; k < totals.size(); ++k)
        for (uint32_t c = 0; c < kAdTop; ++c) {
            const uint64_t v = ranked[k * kAdTop + c], cnt = v >> 20;
            AdCand& d = cand[k * kAdTop + c];
            d = AdCand{static_cast<uint32_t>(kAdKeys - 1 - (v & (kAdKeys - 1))), 0, nocc};
            if (v && totals[k] && cnt * kAdKeys / totals[k] > kAdFold) {
                d.cap = static_cast<uint32_t>(cnt);
                nocc += cnt;
            }
        }
    return nocc;
}

// D = reverse(backward) + seed + forward, its first kAdMaxLen bytes
std::string ad_detected(const AdExt& e, uint32_t key) {
    std::string d;
    const uint32_t nb = std::min(e.nb, kAdMaxLen);
    for (uint32_t i = 0; i < nb; ++i) d += static_cast<char>(e.back[(e.nb - 1 - i) % kAdKeep]);
    for (uint32_t i = 0; i < kAdK; ++i) d += "ACGT"[(key >> (2 * (kAdK - 1 - i))) & 3u];
    for (uint32_t i = 0; i < std::min(e.nf, kAdKeep); ++i) d += static_cast<char>(e.fwd[i]);
    if (d.size() > kAdMaxLen) d.resize(kAdMaxLen);
    return d;
}

// what an extension is accepted as: the listed adapter D snaps to, else D when both directions ran out, else nothing
std::string ad_accept(const AdExt& e, uint32_t key) {
    const std::string D = ad_detected(e, key);
    for (const char* known : kAdKnown) {
        const std::string ad(known);
        if (D.find(ad.substr(0, kAdSnap)) != std::string::npos) return ad;
    }
    return (e.flags & 3u) == 3u ? D : std::string();
}

// vk_clean_device, and with ad_lengths vk_clean_adapters_device
int cl_clean(vk_ctx* ctx, const void* d_text, const uint64_t* offsets, const uint64_t* lengths, const uint64_t* records,
             const uint32_t* roles, const uint32_t* samples, uint32_t nfiles, uint32_t nsamples, uint32_t trim_front,
             uint32_t trim_tail, uint32_t flags, void* d_ws, uint64_t ws_bytes, uint8_t* d_out, const uint64_t* out_offsets,
             uint64_t out_bytes, uint64_t* d_out_lengths, uint64_t* d_stats, uint32_t* d_status, const uint32_t* ad_lengths,
             const uint8_t* ad_seqs, uint64_t* d_ad_stats) {
    if (!out_offsets || !d_out || !d_out_lengths || !d_stats || !d_status) return VK_EINVAL;
    if ((flags & ~(VK_CL_ADAPTER | VK_CL_MERGE | VK_CL_DEDUP)) || trim_front > (1u << 30)) return VK_EINVAL;
    int rc = cl_check(ctx, d_text, offsets, lengths, records, roles, samples, nfiles, nsamples, trim_tail, d_ws);
    if (rc) return rc;
    const ClLayout L = cl_layout(d_ws, lengths, records, nfiles, nsamples);
    if (ws_bytes < L.total) return VK_EINVAL;
    const ClIndex ix = cl_index(offsets, lengths, records, roles, samples, nfiles, nsamples, ~0ull);
    std::vector<uint64_t> cap(nsamples, 0), unit_base(nsamples + 1ull, 0);
    for (uint32_t i = 0; i < nfiles; ++i) cap[samples[i]] += lengths[i];
    std::vector<ClSample> smp(nsamples);
    for (uint32_t s = 0; s < nsamples; ++s) {
        const uint64_t *first = &ix.first[3ull * s], *cnt = &ix.count[3ull * s];
        ClSample& d = smp[s];
        d.r1 = first[0];
        d.r2 = first[1];
        d.se = first[2];
        d.flags = cnt[0] != cnt[1] ? VK_CL_RAGGED : 0u;
        d.npairs = d.flags ? 0 : cnt[0];
        d.nse = d.flags ? 0 : cnt[2];
        d.out_off = out_offsets[s];
        d.out_cap = cap[s];
        if (out_offsets[s] % 16 || out_offsets[s] + (cap[s] + 15) / 16 * 16 > out_bytes) return VK_EINVAL;
        unit_base[s + 1] = unit_base[s] + d.npairs + d.nse;
    }
    const uint64_t nunits = unit_base[nsamples];
    VK_HIP(ctx, hipSetDevice(ctx->device));
    const ClAdapter* dads = nullptr;
    if (ad_lengths) {   // the adapter table in a buffer of the context
        const std::vector<ClAdapter> ads = ad_pack(ad_lengths, ad_seqs, 3ull * nsamples);
        rc = ensure(ctx, reinterpret_cast<void**>(&ctx->d_cladapt), &ctx->cladapt_cap, ads.size() * sizeof(ClAdapter));
        if (rc) return rc;
        VK_HIP(ctx, hipMemcpyAsync(ctx->d_cladapt, ads.data(), ads.size() * sizeof(ClAdapter), hipMemcpyHostToDevice, ctx->stream));
        VK_HIP(ctx, hipMemsetAsync(d_ad_stats, 0, 2ull * nsamples * sizeof(uint64_t), ctx->stream));
        dads = reinterpret_cast<const ClAdapter*>(ctx->d_cladapt);
    }
    const auto* text = static_cast<const uint8_t*>(d_text);
    VK_HIP(ctx, hipMemcpyAsync(L.samples, smp.data(), nsamples * sizeof(ClSample), hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(L.unit_base, unit_base.data(), (nsamples + 1ull) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (flags & VK_CL_DEDUP) VK_HIP(ctx, hipMemsetAsync(L.table, 0xFF, L.nslots * 8, ctx->stream));
    rc = cl_index_run(ctx, text, ix, L, L.samples, nsamples, d_stats, d_status);
    if (rc) return rc;
    const uint64_t ug = (nunits + kClThreads - 1) / kClThreads;
    const uint64_t hash_mask = ctx->clean_hash_bits >= 64 ? ~0ull : ((1ull << ctx->clean_hash_bits) - 1);
    if (nunits) {
        hipLaunchKernelGGL(vk_cl_hash_kernel, dim3(ug), dim3(kClThreads), 0, ctx->stream, text, L.samples, L.unit_base, nsamples,
                           nunits, L.recs, hash_mask, L.hashes, d_status);
        if (flags & VK_CL_DEDUP)
            hipLaunchKernelGGL(vk_cl_dedup_kernel, dim3(ug), dim3(kClThreads), 0, ctx->stream, text, L.samples, L.unit_base,
                               nsamples, nunits, L.recs, L.hashes, d_status, L.table, L.nslots - 1, L.slot_of);
        if (dads)
            hipLaunchKernelGGL(vk_cl_clean_kernel<true>, dim3(ug), dim3(kClThreads), 0, ctx->stream, text, L.samples, L.unit_base,
                               nsamples, nunits, L.recs, d_status, L.table, L.slot_of, trim_front, trim_tail, flags, L.plans,
                               L.obytes, dads, d_ad_stats);
        else
            hipLaunchKernelGGL(vk_cl_clean_kernel<false>, dim3(ug), dim3(kClThreads), 0, ctx->stream, text, L.samples, L.unit_base,
                               nsamples, nunits, L.recs, d_status, L.table, L.slot_of, trim_front, trim_tail, flags, L.plans,
                               L.obytes, static_cast<const ClAdapter*>(nullptr), static_cast<uint64_t*>(nullptr));
    }
    VK_HIP(ctx, hipGetLastError());
    rc = cl_scan(ctx, L.obytes, nunits, L.sums, L.oprefix);
    if (rc) return rc;
    if (nunits)
        hipLaunchKernelGGL(vk_cl_write_kernel, dim3((nunits + kClUnitsPerBlock - 1) / kClUnitsPerBlock), dim3(kClThreads), 0,
                           ctx->stream, text, L.samples, L.unit_base, nsamples, nunits, L.recs, L.plans, L.oprefix, d_out,
                           d_stats, static_cast<uint32_t>(VK_CL_NSTAT));
    hipLaunchKernelGGL(vk_cl_finish_kernel, dim3(nsamples), dim3(kClThreads), 0, ctx->stream, L.samples, L.unit_base, nsamples,
                       L.oprefix, d_status, d_out, d_out_lengths);
    VK_HIP(ctx, hipGetLastError());
    return VK_OK;
}

}  // namespace

extern "C" {

int vk_clean_lines_device(vk_ctx* ctx, const void* d_text, const uint64_t* offsets, const uint64_t* lengths,
                          uint32_t nfiles, uint64_t* lines) {
    if (!ctx || !offsets || !lengths || !lines || (nfiles && !d_text)) return VK_EINVAL;
    if (nfiles == 0) return VK_OK;
    for (uint32_t i = 0; i < nfiles; ++i)
        if (offsets[i] % 16) return VK_EINVAL;
    const ClIndex ix = cl_index(offsets, lengths, nullptr, nullptr, nullptr, nfiles, 0, 0);
    VK_HIP(ctx, hipSetDevice(ctx->device));
    ClFile* d_files = nullptr;
    uint64_t* d_fchunk = nullptr;
    unsigned long long* d_lines = nullptr;
    int rc = ws_carve(ctx, &ctx->d_clines, &ctx->clines_cap, [&](WsTake& take) {
        take(d_files, nfiles);
        take(d_fchunk, nfiles);
        take(d_lines, nfiles);
    });
    if (rc) return rc;
    VK_HIP(ctx, hipMemcpyAsync(d_files, ix.files.data(), nfiles * sizeof(ClFile), hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(d_fchunk, ix.fchunk.data(), nfiles * 8ull, hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipMemsetAsync(d_lines, 0, nfiles * 8ull, ctx->stream));
    if (ix.nchunks)
        hipLaunchKernelGGL(vk_cl_lines_kernel, dim3(ix.nchunks), dim3(kClThreads), 0, ctx->stream,
                           static_cast<const uint8_t*>(d_text), d_files, d_fchunk, nfiles, d_lines);
    VK_HIP(ctx, hipGetLastError());
    VK_HIP(ctx, hipMemcpyAsync(lines, d_lines, nfiles * 8ull, hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VK_OK;
}

int vk_clean_heads_device(vk_ctx* ctx, const void* d_text, const uint64_t* offsets, const uint64_t* lengths,
                          uint32_t nfiles, uint32_t sample_size, uint64_t* totals, uint64_t* counted) {
    if (!ctx || !offsets || !lengths || !totals || !counted || (nfiles && !d_text)) return VK_EINVAL;
    if (sample_size == 0 || sample_size > (1u << 30)) return VK_EINVAL;
    if (nfiles == 0) return VK_OK;
    for (uint32_t i = 0; i < nfiles; ++i)
        if (offsets[i] % 16) return VK_EINVAL;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    // offsets | lengths | totals | counted, nfiles u64 words each, in the buffer of vk_clean_lines_device
    const size_t row = nfiles * 8ull;
    uint64_t *d_offs = nullptr, *d_lens = nullptr, *d_totals = nullptr, *d_counted = nullptr;
    int rc = ws_carve(ctx, &ctx->d_clines, &ctx->clines_cap, [&](WsTake& take) {
        take(d_offs, nfiles);
        take(d_lens, nfiles);
        take(d_totals, nfiles);
        take(d_counted, nfiles);
    });
    if (rc) return rc;
    VK_HIP(ctx, hipMemcpyAsync(d_offs, offsets, row, hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(d_lens, lengths, row, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(vk_cl_heads_kernel, dim3(nfiles), dim3(kClThreads), 0, ctx->stream, static_cast<const uint8_t*>(d_text),
                       d_offs, d_lens, sample_size, d_totals, d_counted);
    VK_HIP(ctx, hipGetLastError());
    VK_HIP(ctx, hipMemcpyAsync(totals, d_totals, row, hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(counted, d_counted, row, hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VK_OK;
}

int vk_clean_workspace_size(const uint64_t* lengths, const uint64_t* records, uint32_t nfiles, uint32_t nsamples,
                            uint64_t* bytes) {
    if (!bytes || (nfiles && (!lengths || !records))) return VK_EINVAL;
    *bytes = cl_layout(nullptr, lengths, records, nfiles, nsamples).total;
    return VK_OK;
}

int vk_clean_device(vk_ctx* ctx, const void* d_text, const uint64_t* offsets, const uint64_t* lengths,
                    const uint64_t* records, const uint32_t* roles, const uint32_t* samples, uint32_t nfiles,
                    uint32_t nsamples, uint32_t trim_front, uint32_t trim_tail, uint32_t flags, void* d_ws,
                    uint64_t ws_bytes, uint8_t* d_out, const uint64_t* out_offsets, uint64_t out_bytes,
                    uint64_t* d_out_lengths, uint64_t* d_stats, uint32_t* d_status) {
    return cl_clean(ctx, d_text, offsets, lengths, records, roles, samples, nfiles, nsamples, trim_front, trim_tail, flags,
                    d_ws, ws_bytes, d_out, out_offsets, out_bytes, d_out_lengths, d_stats, d_status, nullptr, nullptr, nullptr);
}

int vk_clean_adapters_device(vk_ctx* ctx, const void* d_text, const uint64_t* offsets, const uint64_t* lengths,
                             const uint64_t* records, const uint32_t* roles, const uint32_t* samples, uint32_t nfiles,
                             uint32_t nsamples, uint32_t trim_front, uint32_t trim_tail, uint32_t flags, void* d_ws,
                             uint64_t ws_bytes, uint8_t* d_out, const uint64_t* out_offsets, uint64_t out_bytes,
                             uint64_t* d_out_lengths, uint64_t* d_stats, uint32_t* d_status, const uint32_t* adapter_lengths,
                             const uint8_t* adapter_seqs, uint64_t* d_adapter_stats) {
    if (!adapter_lengths || !adapter_seqs || !d_adapter_stats) return VK_EINVAL;
    for (uint64_t g = 0; g < 3ull * nsamples; ++g)
        if (adapter_lengths[g] > kAdMaxAdapter) return VK_EINVAL;
    return cl_clean(ctx, d_text, offsets, lengths, records, roles, samples, nfiles, nsamples, trim_front, trim_tail, flags,
                    d_ws, ws_bytes, d_out, out_offsets, out_bytes, d_out_lengths, d_stats, d_status, adapter_lengths,
                    adapter_seqs, d_adapter_stats);
}

int vk_clean_detect_workspace_size(const uint64_t* lengths, const uint64_t* records, uint32_t nfiles, uint32_t nsamples,
                                   uint64_t* bytes) {
    if (!bytes || (nfiles && (!lengths || !records))) return VK_EINVAL;
    *bytes = ad_layout(nullptr, lengths, records, nfiles, nsamples).total;
    return VK_OK;
}

int vk_clean_detect_device(vk_ctx* ctx, const void* d_text, const uint64_t* offsets, const uint64_t* lengths,
                           const uint64_t* records, const uint32_t* roles, const uint32_t* samples, uint32_t nfiles,
                           uint32_t nsamples, uint32_t trim_tail, void* d_ws, uint64_t ws_bytes, uint32_t* adapter_lengths,
                           uint8_t* adapter_seqs) {
    if (!adapter_lengths || !adapter_seqs) return VK_EINVAL;
    int rc = cl_check(ctx, d_text, offsets, lengths, records, roles, samples, nfiles, nsamples, trim_tail, d_ws);
    if (rc) return rc;
    const AdLayout L = ad_layout(d_ws, lengths, records, nfiles, nsamples);
    if (ws_bytes < L.total) return VK_EINVAL;
    const uint64_t ngroups = 3ull * nsamples;
    std::fill(adapter_lengths, adapter_lengths + ngroups, 0u);
    std::fill(adapter_seqs, adapter_seqs + ngroups * kAdMaxAdapter, uint8_t{0});
    // the index holds each group's evaluation set: its first kAdEval records, in the order of its files
    const ClIndex ix = cl_index(offsets, lengths, records, roles, samples, nfiles, nsamples, kAdEval);
    std::vector<uint64_t> active;   // groups with records
    for (uint64_t g = 0; g < ngroups; ++g)
        if (ix.count[g]) active.push_back(g);
    if (active.empty()) return VK_OK;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    const auto* text = static_cast<const uint8_t*>(d_text);
    rc = cl_index_run(ctx, text, ix, L.c, nullptr, 0, nullptr, nullptr);
    if (rc) return rc;
    const uint32_t shift_tail = std::max(1u, trim_tail);
    for (size_t g0 = 0; g0 < active.size(); g0 += L.slice) {
        const uint32_t ng = static_cast<uint32_t>(std::min<size_t>(L.slice, active.size() - g0));
        std::vector<AdGroup> grp(ng);
        std::vector<uint64_t> base(ng + 1ull, 0);
        for (uint32_t k = 0; k < ng; ++k) {
            grp[k] = AdGroup{ix.first[active[g0 + k]], ix.count[active[g0 + k]]};
            base[k + 1] = base[k] + grp[k].n;
        }
        const uint64_t nrec = base[ng];
        VK_HIP(ctx, hipMemcpyAsync(L.groups, grp.data(), ng * sizeof(AdGroup), hipMemcpyHostToDevice, ctx->stream));
        VK_HIP(ctx, hipMemcpyAsync(L.gbase, base.data(), (ng + 1ull) * 8, hipMemcpyHostToDevice, ctx->stream));
        VK_HIP(ctx, hipMemsetAsync(L.hist, 0, static_cast<size_t>(ng) * kAdKeys * 4, ctx->stream));
        hipLaunchKernelGGL(vk_ad_hist_kernel, dim3((nrec + kClThreads - 1) / kClThreads), dim3(kClThreads), 0, ctx->stream,
                           text, L.c.recs, L.groups, L.gbase, ng, L.hist);
        hipLaunchKernelGGL(vk_ad_top_kernel, dim3(ng), dim3(kAdThreads), 0, ctx->stream, L.hist, L.ranked, L.totals);
        VK_HIP(ctx, hipGetLastError());
        std::vector<uint64_t> rk(ng * kAdTop), tot(ng);
        VK_HIP(ctx, hipMemcpyAsync(rk.data(), L.ranked, rk.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        VK_HIP(ctx, hipMemcpyAsync(tot.data(), L.totals, tot.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        VK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        std::vector<AdCand> cand(ng * kAdTop);
        const uint64_t nocc = ad_candidates(rk, tot, cand);
        if (nocc == 0) continue;
        rc = ensure(ctx, reinterpret_cast<void**>(&ctx->d_cldetect), &ctx->cldetect_cap,
                    ws_align(nocc * sizeof(AdOcc)) + nocc * sizeof(uint16_t));
        if (rc) return rc;
        auto* occ = reinterpret_cast<AdOcc*>(ctx->d_cldetect);
        auto* state = reinterpret_cast<uint16_t*>(ctx->d_cldetect + ws_align(nocc * sizeof(AdOcc)));
        VK_HIP(ctx, hipMemcpyAsync(L.cands, cand.data(), cand.size() * sizeof(AdCand), hipMemcpyHostToDevice, ctx->stream));
        VK_HIP(ctx, hipMemsetAsync(L.counts, 0, cand.size() * 4, ctx->stream));
        hipLaunchKernelGGL(vk_ad_collect_kernel, dim3((nrec + kClThreads - 1) / kClThreads), dim3(kClThreads), 0, ctx->stream,
                           text, L.c.recs, L.groups, L.gbase, ng, L.cands, shift_tail, L.counts, occ);
        hipLaunchKernelGGL(vk_ad_extend_kernel, dim3(ng * kAdTop), dim3(kAdThreads), 0, ctx->stream, text, L.cands, L.counts, occ,
                           state, L.ext);
        VK_HIP(ctx, hipGetLastError());
        std::vector<AdExt> ext(ng * kAdTop);
        VK_HIP(ctx, hipMemcpyAsync(ext.data(), L.ext, ext.size() * sizeof(AdExt), hipMemcpyDeviceToHost, ctx->stream));
        VK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (uint32_t k = 0; k < ng; ++k)   // a group takes the first of its candidates that is accepted
            for (uint32_t c = 0; c < kAdTop; ++c) {
                const AdExt& e = ext[k * kAdTop + c];
                if (!cand[k * kAdTop + c].cap || e.nocc < kAdMinVotes) continue;   // (no evidence either way)
                const std::string got = ad_accept(e, cand[k * kAdTop + c].key);
                if (got.empty()) continue;
                const uint64_t g = active[g0 + k];
                adapter_lengths[g] = static_cast<uint32_t>(got.size());
                memcpy(adapter_seqs + g * kAdMaxAdapter, got.data(), got.size());
                break;
            }
    }
    return VK_OK;
}

}  // extern "C"

// ------------------------------------------------------------- step C's files --

namespace {

// What the calls on record text share (the plans, rules and layouts: vk_textplan.h).
//
// Their head: the samples' rows and, where the call has the piece, rec_base go up; then the call's own uploads and resets
// (`more`); the record index is found; vk_em_status_kernel states every sample's framing (no d_status: vk_qc_device, which
// has a status kernel of its own).
template <class F>
int text_index_run(vk_ctx* ctx, const uint8_t* text, const TextIndex& t, const ClLayout& c, EmSample* d_rows, uint64_t* d_rec_base,
                   uint32_t* d_status, F&& more) {
    const uint32_t nsamples = static_cast<uint32_t>(t.rows.size());
    VK_HIP(ctx, hipSetDevice(ctx->device));
    // (pageable sources: a copy has read its source on return)
    VK_HIP(ctx, hipMemcpyAsync(d_rows, t.rows.data(), nsamples * sizeof(EmSample), hipMemcpyHostToDevice, ctx->stream));
    if (d_rec_base) VK_HIP(ctx, hipMemcpyAsync(d_rec_base, t.rec_base.data(), t.rec_base.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    int rc = more();
    if (rc) return rc;
    rc = cl_index_run(ctx, text, t.ix, c, nullptr, 0, nullptr, nullptr);
    if (rc) return rc;
    if (d_status)
        hipLaunchKernelGGL(vk_em_status_kernel, dim3((nsamples + kClThreads - 1) / kClThreads), dim3(kClThreads), 0, ctx->stream, text,
                           d_rows, nsamples, c.recs, c.cprefix, d_status);
    return VK_OK;
}

}  // namespace

extern "C" {

int vk_ladder_emit_workspace_size(const uint64_t* records, uint32_t nsamples, const uint64_t* lengths,
                                  const uint32_t* step_sample, uint32_t nsteps, uint64_t* bytes) {
    if (!bytes || (nsamples && (!records || !lengths)) || (nsteps && !step_sample)) return VK_EINVAL;
    *bytes = em_layout(nullptr, records, nsamples, lengths, step_sample, nsteps).total;
    return VK_OK;
}

int vk_ladder_emit_device(vk_ctx* ctx, const void* d_fastq, const uint64_t* offsets, const uint64_t* lengths,
                          const uint64_t* records, uint32_t nsamples, const uint32_t* step_sample,
                          const uint64_t* step_seed, const uint64_t* step_threshold, const uint8_t* step_whole,
                          uint32_t nsteps, uint8_t* d_out, uint64_t out_capacity, uint64_t* out_offsets,
                          uint64_t* out_lengths, uint32_t* status, void* d_ws, uint64_t ws_bytes) {
    if (!ctx || nsamples == 0 || !d_fastq || !offsets || !lengths || !records || !status || !d_ws) return VK_EINVAL;
    if (nsteps && (!step_sample || !step_seed || !step_threshold || !step_whole || !out_offsets || !out_lengths)) return VK_EINVAL;
    if (!d_out && out_capacity) return VK_EINVAL;
    TextCall c{};
    c.offsets = offsets, c.lengths = lengths, c.records = records, c.nsamples = nsamples;
    if (int rc = emit_check(c, step_sample, step_threshold, nsteps)) return rc;
    const EmLayout L = em_layout(d_ws, records, nsamples, lengths, step_sample, nsteps);
    if (ws_bytes < L.total) return VK_EINVAL;
    const TextIndex t = text_index(offsets, lengths, records, nsamples);
    std::vector<EmStep> steps(nsteps);
    std::vector<uint64_t> step_base(nsteps + 1ull, 0);
    for (uint32_t j = 0; j < nsteps; ++j) {
        steps[j] = EmStep{step_seed[j], step_threshold[j], 0, step_sample[j], step_whole[j] ? 1u : 0u};
        step_base[j + 1] = step_base[j] + records[step_sample[j]];
    }
    const uint64_t nitems = step_base[nsteps];
    const auto* text = static_cast<const uint8_t*>(d_fastq);
    int rc = text_index_run(ctx, text, t, L.c, L.samples, nullptr, L.status, [&] {
        VK_HIP(ctx, hipMemcpyAsync(L.step_base, step_base.data(), step_base.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        if (nsteps) VK_HIP(ctx, hipMemcpyAsync(L.steps, steps.data(), nsteps * sizeof(EmStep), hipMemcpyHostToDevice, ctx->stream));
        return VK_OK;
    });
    if (rc) return rc;
    if (nitems)
        hipLaunchKernelGGL(vk_em_plan_kernel, dim3((nitems + kClThreads - 1) / kClThreads), dim3(kClThreads), 0, ctx->stream, text,
                           L.samples, L.steps, L.step_base, nsteps, nitems, L.c.recs, L.status, L.obytes);
    VK_HIP(ctx, hipGetLastError());
    rc = cl_scan(ctx, L.obytes, nitems, L.c.sums, L.oprefix);
    if (rc) return rc;
    if (nsteps)
        hipLaunchKernelGGL(vk_em_sizes_kernel, dim3((nsteps + kClThreads - 1) / kClThreads), dim3(kClThreads), 0, ctx->stream,
                           L.step_base, nsteps, L.oprefix, L.sizes);
    VK_HIP(ctx, hipGetLastError());
    VK_HIP(ctx, hipMemcpyAsync(status, L.status, nsamples * 4ull, hipMemcpyDeviceToHost, ctx->stream));
    if (nsteps) VK_HIP(ctx, hipMemcpyAsync(out_lengths, L.sizes, nsteps * 8ull, hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // the files one after another, each at a multiple of 16 bytes
    uint64_t at = 0;
    for (uint32_t j = 0; j < nsteps; ++j) {
        out_offsets[j] = steps[j].out_off = at;
        at += (out_lengths[j] + 15) / 16 * 16;
    }
    if (at > out_capacity) return VK_ENOSPC;
    if (at == 0) return VK_OK;
    VK_HIP(ctx, hipMemcpyAsync(L.steps, steps.data(), nsteps * sizeof(EmStep), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(vk_em_write_kernel, dim3((nitems + kEmItemsPerBlock - 1) / kEmItemsPerBlock), dim3(kClThreads), 0,
                       ctx->stream, text, L.samples, L.steps, L.step_base, nsteps, nitems, L.c.recs, L.oprefix, d_out);
    hipLaunchKernelGGL(vk_em_pad_kernel, dim3((nsteps + kClThreads - 1) / kClThreads), dim3(kClThreads), 0, ctx->stream, L.steps,
                       nsteps, L.sizes, d_out);
    VK_HIP(ctx, hipGetLastError());
    VK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the tables above are the host's)
    return VK_OK;
}

}  // extern "C"

// ------------------------------------------------------- .fq.gz files (BGZF) --

namespace {

// the pieces of a vk_deflate_device workspace
struct DfLayout {
    uint8_t* slots;
    DfMember* mem;
    DfFile* files;
    uint64_t *sizes, *mprefix, *sums, *flens, *fsizes, *fprefix;
    size_t total;
    uint64_t nmem;
};

uint64_t df_members(uint64_t len) { return (len + kDfMemberText - 1) / kDfMemberText; }
uint64_t df_file_bound(uint64_t len) { return (df_members(len) * 31 + len + kDfEofBytes + 15) / 16 * 16; }

DfLayout df_layout(void* d_work, const uint64_t* lengths, uint32_t nfiles) {
    DfLayout L{};
    for (uint32_t i = 0; i < nfiles; ++i) L.nmem += df_members(lengths[i]);
    const uint64_t nb = (std::max<uint64_t>(L.nmem, nfiles) + kClScanBlock - 1) / kClScanBlock;
    WsTake take{static_cast<uint8_t*>(d_work), 0};
    take(L.slots, L.nmem * kDfSlot);
    take(L.mem, L.nmem);
    take(L.files, nfiles);
    take(L.sizes, L.nmem);
    take(L.mprefix, L.nmem + 1);
    take(L.sums, nb + 1);
    take(L.flens, nfiles);
    take(L.fsizes, nfiles);
    take(L.fprefix, nfiles + 1ull);
    L.total = take.at;
    return L;
}

}  // namespace

extern "C" {

int vk_deflate_bound(const uint64_t* lengths, uint32_t nfiles, uint64_t* out_bound) {
    if (!out_bound || (nfiles && !lengths)) return VK_EINVAL;
    uint64_t b = 0;
    for (uint32_t i = 0; i < nfiles; ++i) b += df_file_bound(lengths[i]);
    *out_bound = b;
    return VK_OK;
}

int vk_deflate_workspace_size(const uint64_t* lengths, uint32_t nfiles, uint64_t* out_bytes) {
    if (!out_bytes || (nfiles && !lengths)) return VK_EINVAL;
    *out_bytes = df_layout(nullptr, lengths, nfiles).total;
    return VK_OK;
}

int vk_deflate_device(vk_ctx* ctx, const void* d_text, const uint64_t* offsets, const uint64_t* lengths, uint32_t nfiles,
                      uint8_t* d_out, uint64_t out_capacity, void* d_work, uint64_t work_bytes, uint64_t* out_offsets,
                      uint64_t* out_lengths) {
    if (!ctx || nfiles == 0 || !d_text || !offsets || !lengths || !d_out || !d_work || !out_offsets || !out_lengths) return VK_EINVAL;
    for (uint32_t i = 0; i < nfiles; ++i)
        if (offsets[i] % 16) return VK_EINVAL;
    const DfLayout L = df_layout(d_work, lengths, nfiles);
    if (work_bytes < L.total || L.nmem + nfiles > 0x7FFFFFFFull) return VK_EINVAL;
    uint64_t bound = 0;
    for (uint32_t i = 0; i < nfiles; ++i) bound += df_file_bound(lengths[i]);
    if (out_capacity < bound) return VK_ENOSPC;
    std::vector<DfMember> mem(L.nmem);
    std::vector<DfFile> files(nfiles);
    uint64_t m = 0;
    for (uint32_t i = 0; i < nfiles; ++i) {
        files[i] = DfFile{m, df_members(lengths[i])};
        for (uint64_t at = 0; at < lengths[i]; at += kDfMemberText)
            mem[m++] = DfMember{offsets[i] + at, static_cast<uint32_t>(std::min<uint64_t>(kDfMemberText, lengths[i] - at)), i};
    }
    VK_HIP(ctx, hipSetDevice(ctx->device));
    VK_HIP(ctx, hipMemcpyAsync(L.files, files.data(), nfiles * sizeof(DfFile), hipMemcpyHostToDevice, ctx->stream));
    if (L.nmem) {
        VK_HIP(ctx, hipMemcpyAsync(L.mem, mem.data(), L.nmem * sizeof(DfMember), hipMemcpyHostToDevice, ctx->stream));
        VK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(vk_df_member_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        static_cast<int>(sizeof(DfLds))));
        hipLaunchKernelGGL(vk_df_member_kernel, dim3(static_cast<uint32_t>(L.nmem)), dim3(kDfThreads), sizeof(DfLds), ctx->stream,
                           static_cast<const uint8_t*>(d_text), L.mem, L.slots, L.sizes);
        VK_HIP(ctx, hipGetLastError());
    }
    int rc = cl_scan(ctx, L.sizes, L.nmem, L.sums, L.mprefix);
    if (rc) return rc;
    hipLaunchKernelGGL(vk_df_files_kernel, dim3((nfiles + kDfThreads - 1) / kDfThreads), dim3(kDfThreads), 0, ctx->stream, L.files,
                       nfiles, L.mprefix, L.flens, L.fsizes);
    VK_HIP(ctx, hipGetLastError());
    rc = cl_scan(ctx, L.fsizes, nfiles, L.sums, L.fprefix);
    if (rc) return rc;
    hipLaunchKernelGGL(vk_df_gather_kernel, dim3(static_cast<uint32_t>(L.nmem + nfiles)), dim3(kDfThreads), 0, ctx->stream, L.mem,
                       L.nmem, L.files, L.slots, L.mprefix, L.flens, L.fprefix, d_out);
    VK_HIP(ctx, hipGetLastError());
    VK_HIP(ctx, hipMemcpyAsync(out_offsets, L.fprefix, nfiles * 8ull, hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(out_lengths, L.flens, nfiles * 8ull, hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the tables above are the host's)
    return VK_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- IDAT chunks (vk_png.h) ------

namespace {

// the pieces of a vk_png_device workspace
struct PngLayout {
    uint8_t* slots;
    PngPiece* psums;
    uint64_t *sizes, *pprefix, *sums, *ilens, *isizes, *iprefix;
    uint32_t* itail;
    size_t total;
    uint64_t npieces;
    uint32_t ppi, slot;
};

PngLayout png_layout(void* d_work, uint32_t side, uint32_t nimg) {
    PngLayout L{};
    L.ppi = png_pieces(side);
    L.slot = png_slot(side);
    L.npieces = static_cast<uint64_t>(nimg) * L.ppi;
    const uint64_t nb = (L.npieces + kClScanBlock - 1) / kClScanBlock;
    WsTake take{static_cast<uint8_t*>(d_work), 0};
    take(L.slots, L.npieces * L.slot);
    take(L.psums, L.npieces);
    take(L.sizes, L.npieces);
    take(L.pprefix, L.npieces + 1);
    take(L.sums, nb + 1);
    take(L.ilens, nimg);
    take(L.isizes, nimg);
    take(L.iprefix, nimg + 1ull);
    take(L.itail, 2ull * nimg);
    L.total = take.at;
    return L;
}

bool png_shape_ok(uint32_t side, uint32_t nimg) { return nimg != 0 && side != 0 && side <= kPngMaxSide; }

}  // namespace

extern "C" {

int vk_png_bound(uint32_t side, uint32_t nimg, uint64_t* out_bound) {
    if (!out_bound || !png_shape_ok(side, nimg)) return VK_EINVAL;
    *out_bound = png_chunk_bound(side) * nimg;
    return VK_OK;
}

int vk_png_workspace_size(uint32_t side, uint32_t nimg, uint64_t* out_bytes) {
    if (!out_bytes || !png_shape_ok(side, nimg)) return VK_EINVAL;
    *out_bytes = png_layout(nullptr, side, nimg).total;
    return VK_OK;
}

int vk_png_device(vk_ctx* ctx, const void* d_img, uint32_t nimg, uint32_t side, uint8_t* d_out, uint64_t out_capacity, void* d_work,
                  uint64_t work_bytes, uint64_t* out_offsets, uint64_t* out_lengths) {
    if (!ctx || !d_img || !d_out || !d_work || !out_offsets || !out_lengths || !png_shape_ok(side, nimg)) return VK_EINVAL;
    const PngLayout L = png_layout(d_work, side, nimg);
    if (work_bytes < L.total || L.npieces + nimg > 0x7FFFFFFFull) return VK_EINVAL;
    if (out_capacity < png_chunk_bound(side) * nimg) return VK_ENOSPC;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    VK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(vk_png_piece_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    static_cast<int>(sizeof(DfLds))));
    hipLaunchKernelGGL(vk_png_piece_kernel, dim3(static_cast<uint32_t>(L.npieces)), dim3(kDfThreads), sizeof(DfLds), ctx->stream,
                       static_cast<const uint8_t*>(d_img), side, L.ppi, L.slot, L.slots, L.sizes, L.psums);
    VK_HIP(ctx, hipGetLastError());
    int rc = cl_scan(ctx, L.sizes, L.npieces, L.sums, L.pprefix);
    if (rc) return rc;
    hipLaunchKernelGGL(vk_png_image_kernel, dim3((nimg + kDfThreads - 1) / kDfThreads), dim3(kDfThreads), 0, ctx->stream, nimg, L.ppi,
                       L.psums, L.sizes, L.pprefix, L.ilens, L.isizes, L.itail);
    VK_HIP(ctx, hipGetLastError());
    rc = cl_scan(ctx, L.isizes, nimg, L.sums, L.iprefix);
    if (rc) return rc;
    hipLaunchKernelGGL(vk_png_gather_kernel, dim3(static_cast<uint32_t>(L.npieces + nimg)), dim3(kDfThreads), 0, ctx->stream,
                       L.npieces, L.ppi, L.slot, L.slots, L.pprefix, L.ilens, L.iprefix, L.itail, d_out);
    VK_HIP(ctx, hipGetLastError());
    VK_HIP(ctx, hipMemcpyAsync(out_offsets, L.iprefix, nimg * 8ull, hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(out_lengths, L.ilens, nimg * 8ull, hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the tables above are the host's)
    return VK_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- PNG files read (vk_unpng.h) ------

namespace {

// the pieces of a vk_unpng_device workspace
struct UnpngLayout {
    uint8_t* slots;
    uint64_t *offs, *lens;
    uint32_t *st, *adler, *status;
    size_t total;
};

UnpngLayout unpng_layout(void* d_work, uint32_t side, uint32_t nimg) {
    UnpngLayout L{};
    WsTake take{static_cast<uint8_t*>(d_work), 0};
    take(L.slots, static_cast<size_t>(nimg) * unpng_slot(side));
    take(L.offs, nimg);
    take(L.lens, nimg);
    take(L.st, nimg);
    take(L.adler, nimg);
    take(L.status, nimg);
    L.total = take.at;
    return L;
}

}  // namespace

extern "C" {

int vk_unpng_workspace_size(uint32_t side, uint32_t nimg, uint64_t* out_bytes) {
    if (!out_bytes || !png_shape_ok(side, nimg)) return VK_EINVAL;
    *out_bytes = unpng_layout(nullptr, side, nimg).total;
    return VK_OK;
}

int vk_unpng_device(vk_ctx* ctx, const void* d_streams, const uint64_t* offsets, const uint64_t* lengths, uint32_t nimg, uint32_t side,
                    uint8_t* d_img, uint32_t* status, void* d_work, uint64_t work_bytes) {
    if (!ctx || !d_streams || !offsets || !lengths || !d_img || !status || !d_work || !png_shape_ok(side, nimg)) return VK_EINVAL;
    for (uint32_t i = 0; i < nimg; ++i)
        if ((offsets[i] & 15u) || lengths[i] < kUpStreamMin) return VK_EINVAL;
    const UnpngLayout L = unpng_layout(d_work, side, nimg);
    if (work_bytes < L.total) return VK_EINVAL;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    VK_HIP(ctx, hipMemcpyAsync(L.offs, offsets, nimg * 8ull, hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(L.lens, lengths, nimg * 8ull, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(vk_unpng_inflate_kernel, dim3(nimg), dim3(64), 0, ctx->stream, static_cast<const uint8_t*>(d_streams), L.offs,
                       L.lens, nimg, side, L.slots, L.st, L.adler);
    VK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(vk_unpng_unfilter_kernel, dim3(nimg), dim3(kUpLanes), unpng_lds_words(side) * 4u, ctx->stream, L.slots, nimg, side,
                       L.st, L.adler, d_img, L.status);
    VK_HIP(ctx, hipGetLastError());
    VK_HIP(ctx, hipMemcpyAsync(status, L.status, nimg * 4ull, hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (status is the host's)
    return VK_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- FASTA count (vk_fasta.h, vk_fasta_ladder.h) ------
// What a call carries, the rules of its arguments, the plan, the pair table and the workspaces' pieces are vk_faplan.h's
// (with the warts kept); the entry points, the copies and the launches are here, one sequence per shared stage.

namespace {

bool fa_text_ok(const void* d_fasta) { return d_fasta && (reinterpret_cast<uintptr_t>(d_fasta) & 15u) == 0; }

// Behind a call's rules: the text where a lane may load it -- looked at only when there is a sample --, then the device.
// (vk_count_fasta_windows_device has rules between the two and states them itself.)
int fa_enter(vk_ctx* ctx, const void* d_fasta, uint32_t nsamples) {
    if (nsamples && !fa_text_ok(d_fasta)) return VK_EINVAL;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    return VK_OK;
}

// The header state that enters every unit (f.carry) and the samples' status words: the plan goes up, then the call's own
// uploads and resets (`more`), then the two kernels.  *m: the plan as the kernels read it.
template <class F>
int fa_state_run(vk_ctx* ctx, const uint8_t* text, const FaPlan& pl, const FaStatePieces& f, uint32_t* d_status, FaMeta* m, F&& more) {
    // (pageable source: the copy has read it on return)
    VK_HIP(ctx, hipMemcpyAsync(f.meta, pl.meta.data(), pl.meta.size() * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    int rc = more();
    if (rc) return rc;
    *m = pl.on_device(f.meta);
    if (pl.nwg) {
        hipLaunchKernelGGL(vk_fa_summary_kernel, dim3(static_cast<uint32_t>(pl.nwg)), dim3(kFaThreads), 0, ctx->stream, text, *m, f.ukey);
        VK_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(vk_fa_scan_kernel, dim3(pl.nsamples), dim3(kFaThreads), 0, ctx->stream, text, *m, f.ukey, f.carry, d_status);
    VK_HIP(ctx, hipGetLastError());
    return VK_OK;
}

// The lanes' index and the ordinal of every unit's first sequence byte (d_lane, d_unit_ord), the samples' sequence bytes.
int fa_ord_run(vk_ctx* ctx, const uint8_t* text, const FaPlan& pl, const FaMeta& m, const uint32_t* d_carry, uint32_t* d_lane,
               unsigned long long* d_unit_ord, unsigned long long* d_bases) {
    if (pl.nwg) {
        hipLaunchKernelGGL(vk_fa_ord_kernel, dim3(static_cast<uint32_t>(pl.nwg)), dim3(kFaThreads), 0, ctx->stream, text, m, d_carry,
                           d_lane, d_unit_ord);
        VK_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(vk_fa_ordscan_kernel, dim3(pl.nsamples), dim3(kFaThreads), 0, ctx->stream, text, m, d_unit_ord, d_bases);
    VK_HIP(ctx, hipGetLastError());
    return VK_OK;
}

// One kernel templated on K for the runtime k (5..9, checked by the caller), nwg workgroups of kFaThreads, its error
// checked.  pick(std::integral_constant<int, K>{}) names the kernel: FA_KERNEL(vk_fa_count_kernel).
#define FA_KERNEL(name) [](auto kc) { return name<decltype(kc)::value>; }
template <class Pick, class... Args>
int launch_k(vk_ctx* ctx, int k, uint64_t nwg, Pick pick, Args... args) {
    return with_k(k, [&](auto kc) {
        hipLaunchKernelGGL(pick(kc), dim3(static_cast<uint32_t>(nwg)), dim3(kFaThreads), 0, ctx->stream, args...);
        VK_HIP(ctx, hipGetLastError());
        return VK_OK;
    });
}

}  // namespace

extern "C" {

int vk_count_fasta_device(vk_ctx* ctx, const void* d_fasta, const uint64_t* offsets, const uint64_t* lengths, uint32_t nsamples,
                          int k, uint32_t* d_hist, uint32_t* d_status, uint64_t* d_bases) {
    if (!ctx || !offsets || !lengths || !d_hist || !d_status || !d_bases) return VK_EINVAL;
    FaCall c{};
    c.offsets = offsets, c.lengths = lengths, c.nsamples = nsamples, c.k = k;
    if (int rc = count_fasta_check(c)) return rc;
    if (nsamples == 0) return VK_OK;
    int rc = fa_enter(ctx, d_fasta, nsamples);
    if (rc) return rc;
    FaPlan pl;
    rc = fa_plan(ctx->fasta_unit_bytes, offsets, lengths, nsamples, &pl);
    if (rc) return rc;
    FaStatePieces f{};
    rc = ws_carve(ctx, &ctx->d_fasta, &ctx->fasta_cap, [&](WsTake& take) { fa_state_take(take, f, nsamples, pl.nunits); });
    if (rc) return rc;
    const size_t ncode = static_cast<size_t>(1) << (2 * k);
    const uint8_t* text = static_cast<const uint8_t*>(d_fasta);
    FaMeta m;
    rc = fa_state_run(ctx, text, pl, f, d_status, &m, [&] {
        VK_HIP(ctx, hipMemsetAsync(d_hist, 0, nsamples * ncode * sizeof(uint32_t), ctx->stream));
        VK_HIP(ctx, hipMemsetAsync(d_bases, 0, nsamples * sizeof(uint64_t), ctx->stream));
        return VK_OK;
    });
    if (rc || !pl.nwg) return rc;
    return launch_k(ctx, k, pl.nwg, FA_KERNEL(vk_fa_count_kernel), text, m, f.carry, d_hist, reinterpret_cast<unsigned long long*>(d_bases));
}

int vk_count_fasta_sampled_device(vk_ctx* ctx, const void* d_fasta, const uint64_t* offsets, const uint64_t* lengths,
                                  uint32_t nsamples, int k, uint32_t frag_len, uint32_t npairs, const uint32_t* pair_sample,
                                  const uint64_t* seeds, const uint64_t* thresholds, const uint64_t* shifts, uint32_t* d_hist,
                                  uint32_t* d_status, uint64_t* d_bases, uint64_t* d_taken) {
    if (!ctx || !offsets || !lengths || !d_status || !d_bases) return VK_EINVAL;
    if (npairs && (!pair_sample || !seeds || !thresholds || !shifts || !d_hist || !d_taken)) return VK_EINVAL;
    FaCall c{};
    c.offsets = offsets, c.lengths = lengths, c.nsamples = nsamples, c.k = k, c.frag_len = frag_len;
    c.npairs = npairs, c.pair_sample = pair_sample, c.seeds = seeds, c.thresholds = thresholds, c.shifts = shifts;
    if (int rc = count_fasta_sampled_check(c)) return rc;
    if (nsamples == 0) return VK_OK;
    int rc = fa_enter(ctx, d_fasta, nsamples);
    if (rc) return rc;
    FaPlan pl;
    rc = fa_plan(ctx->fasta_unit_bytes, offsets, lengths, nsamples, &pl);
    if (rc) return rc;
    FaPairPlan pp;
    rc = fa_pair_plan(c, pl, &pp);
    if (rc) return rc;
    FaSampledPieces p{};
    rc = ws_carve(ctx, &ctx->d_fasta, &ctx->fasta_cap, [&](WsTake& take) { fa_sampled_take(take, p, pl, npairs); });
    if (rc) return rc;
    const size_t ncode = static_cast<size_t>(1) << (2 * k);
    const uint8_t* text = static_cast<const uint8_t*>(d_fasta);
    FaMeta m;
    rc = fa_state_run(ctx, text, pl, p.f, d_status, &m, [&] {
        // (pageable source: the copy has read it on return)
        VK_HIP(ctx, hipMemcpyAsync(p.pairs, pp.words.data(), pp.words.size() * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
        if (npairs) {
            VK_HIP(ctx, hipMemsetAsync(d_hist, 0, npairs * ncode * sizeof(uint32_t), ctx->stream));
            VK_HIP(ctx, hipMemsetAsync(d_taken, 0, npairs * sizeof(uint64_t), ctx->stream));
        }
        return VK_OK;
    });
    if (rc) return rc;
    rc = fa_ord_run(ctx, text, pl, m, p.f.carry, p.lane, p.unit_ord, reinterpret_cast<unsigned long long*>(d_bases));
    if (rc || !pp.pair_nwg) return rc;
    return launch_k(ctx, k, pp.pair_nwg, FA_KERNEL(vk_fa_frag_count_kernel), text, m, pp.pairs_on_device(p.pairs, frag_len), p.lane,
                    p.unit_ord, d_hist, reinterpret_cast<unsigned long long*>(d_taken));
}

int vk_count_fasta_host(vk_ctx* ctx, const uint8_t* fasta, size_t nbytes, int k, uint32_t* hist, uint32_t* status, uint64_t* bases) {
    if (!ctx || !hist || k < 5 || k > 9 || (nbytes && !fasta)) return VK_EINVAL;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ncode = static_cast<size_t>(1) << (2 * k);
    int rc = ensure(ctx, reinterpret_cast<void**>(&ctx->d_stage), &ctx->stage_cap, nbytes + 64);
    if (rc) return rc;
    if (!ctx->d_hist1) VK_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->d_hist1), (1u << 18) * sizeof(uint32_t)));
    rc = ensure(ctx, reinterpret_cast<void**>(&ctx->d_status1), &ctx->status1_cap, 64);   // status word, then the bases at byte 8
    if (rc) return rc;
    if (nbytes) VK_HIP(ctx, hipMemcpyAsync(ctx->d_stage, fasta, nbytes, hipMemcpyHostToDevice, ctx->stream));
    uint64_t off = 0, len = nbytes;
    uint64_t* d_bases = reinterpret_cast<uint64_t*>(ctx->d_status1 + 2);
    rc = vk_count_fasta_device(ctx, ctx->d_stage, &off, &len, 1, k, ctx->d_hist1, ctx->d_status1, d_bases);
    if (rc) return rc;
    uint32_t st = 0;
    uint64_t nb = 0;
    VK_HIP(ctx, hipMemcpyAsync(hist, ctx->d_hist1, ncode * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(&st, ctx->d_status1, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(&nb, d_bases, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (status) *status = st;
    if (bases) *bases = nb;
    return st ? VK_EFORMAT : VK_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- FASTA records (vk_fasta_records.h) ---------------

namespace {

// What the three per-record calls and the windows share: the plan on the device, the header state and the header count
// that enter every unit (p.carry, p.uhdr), the samples' status words and record counts.
struct FarState {
    FaPlan pl;
    FaMeta m;
    FarPieces p;
    uint32_t *d_status = nullptr, *d_nrec = nullptr;   // the caller's, or p's
};

// rec_first: null (the counting call) or host u64[nsamples + 1], checked by the caller.  d_status, d_nrec: the caller's,
// or null for pieces of the workspace.
int far_prepare(vk_ctx* ctx, const uint8_t* text, const uint64_t* offsets, const uint64_t* lengths, uint32_t nsamples,
                const uint64_t* rec_first, uint32_t* d_status, uint32_t* d_nrec, FarState* st) {
    int rc = fa_plan(ctx->fasta_unit_bytes, offsets, lengths, nsamples, &st->pl);
    if (rc) return rc;
    const FaPlan& pl = st->pl;
    FarPieces& p = st->p;
    rc = ws_carve(ctx, &ctx->d_fasta, &ctx->fasta_cap, [&](WsTake& take) { far_take(take, p, pl); });
    if (rc) return rc;
    st->d_status = d_status ? d_status : p.status;
    st->d_nrec = d_nrec ? d_nrec : p.nrec;
    // (pageable sources: the copies have read them on return)
    VK_HIP(ctx, hipMemcpyAsync(p.meta, pl.meta.data(), pl.meta.size() * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    if (rec_first)
        VK_HIP(ctx, hipMemcpyAsync(p.rec_first, rec_first, (nsamples + 1ull) * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    st->m = pl.on_device(p.meta);
    if (pl.nwg) {
        hipLaunchKernelGGL(vk_far_summary_kernel, dim3(static_cast<uint32_t>(pl.nwg)), dim3(kFaThreads), 0, ctx->stream, text, st->m,
                           p.ukey, p.uhdr);
        VK_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(vk_far_scan_kernel, dim3(nsamples), dim3(kFaThreads), 0, ctx->stream, text, st->m, p.ukey, p.carry, p.uhdr,
                       st->d_status, st->d_nrec);
    VK_HIP(ctx, hipGetLastError());
    return VK_OK;
}

}  // namespace

extern "C" {

int vk_fasta_records_count_device(vk_ctx* ctx, const void* d_fasta, const uint64_t* offsets, const uint64_t* lengths, uint32_t nsamples,
                                  uint32_t* d_nrec, uint32_t* d_status) {
    if (!ctx || !offsets || !lengths || !d_nrec || !d_status) return VK_EINVAL;
    FaCall c{};
    c.offsets = offsets, c.lengths = lengths, c.nsamples = nsamples;
    if (int rc = fasta_records_count_check(c)) return rc;
    if (nsamples == 0) return VK_OK;
    if (int rc = fa_enter(ctx, d_fasta, nsamples)) return rc;
    FarState st;
    return far_prepare(ctx, static_cast<const uint8_t*>(d_fasta), offsets, lengths, nsamples, nullptr, d_status, d_nrec, &st);
}

int vk_fasta_records_device(vk_ctx* ctx, const void* d_fasta, const uint64_t* offsets, const uint64_t* lengths, uint32_t nsamples,
                            const uint64_t* rec_first, uint64_t* d_rec_start, uint64_t* d_rec_bases, uint8_t* d_rec_name) {
    if (!ctx || !offsets || !lengths || !rec_first || !d_rec_start || !d_rec_bases || !d_rec_name) return VK_EINVAL;
    FaCall c{};
    c.offsets = offsets, c.lengths = lengths, c.nsamples = nsamples, c.rec_first = rec_first;
    if (int rc = fasta_records_check(c)) return rc;
    if (nsamples == 0) return VK_OK;
    int rc = fa_enter(ctx, d_fasta, nsamples);
    if (rc) return rc;
    const uint8_t* text = static_cast<const uint8_t*>(d_fasta);
    FarState st;
    rc = far_prepare(ctx, text, offsets, lengths, nsamples, rec_first, nullptr, nullptr, &st);
    if (rc) return rc;
    const uint64_t total = rec_first[nsamples];
    if (total == 0) return VK_OK;
    VK_HIP(ctx, hipMemsetAsync(d_rec_start, 0, total * sizeof(uint64_t), ctx->stream));
    VK_HIP(ctx, hipMemsetAsync(d_rec_bases, 0, total * sizeof(uint64_t), ctx->stream));
    VK_HIP(ctx, hipMemsetAsync(d_rec_name, 0, total * kFaNameBytes, ctx->stream));
    if (st.pl.nwg) {
        hipLaunchKernelGGL(vk_far_table_kernel, dim3(static_cast<uint32_t>(st.pl.nwg)), dim3(kFaThreads), 0, ctx->stream, text, st.m,
                           st.p.carry, st.p.uhdr, FaRecs{st.p.rec_first}, reinterpret_cast<unsigned long long*>(d_rec_start),
                           reinterpret_cast<unsigned long long*>(d_rec_bases), d_rec_name);
        VK_HIP(ctx, hipGetLastError());
    }
    return VK_OK;
}

int vk_count_fasta_records_device(vk_ctx* ctx, const void* d_fasta, const uint64_t* offsets, const uint64_t* lengths, uint32_t nsamples,
                                  int k, const uint64_t* rec_first, const uint32_t* d_slot, uint32_t nslots, uint32_t* d_hist) {
    if (!ctx || !offsets || !lengths || !rec_first || !d_slot || !d_hist) return VK_EINVAL;
    FaCall c{};
    c.offsets = offsets, c.lengths = lengths, c.nsamples = nsamples, c.k = k, c.rec_first = rec_first, c.nslots = nslots;
    if (int rc = count_fasta_records_check(c)) return rc;
    int rc = fa_enter(ctx, d_fasta, nsamples);
    if (rc) return rc;
    const size_t ncode = static_cast<size_t>(1) << (2 * k);
    // (the wart: the offsets before the reset, the rest of the plan's rules behind it)
    if (!fa_offsets_ok(offsets, nsamples)) return VK_EINVAL;
    VK_HIP(ctx, hipMemsetAsync(d_hist, 0, nslots * ncode * sizeof(uint32_t), ctx->stream));
    if (nsamples == 0 || rec_first[nsamples] == 0) return VK_OK;
    const uint8_t* text = static_cast<const uint8_t*>(d_fasta);
    FarState st;
    rc = far_prepare(ctx, text, offsets, lengths, nsamples, rec_first, nullptr, nullptr, &st);
    if (rc || !st.pl.nwg) return rc;
    return launch_k(ctx, k, st.pl.nwg, FA_KERNEL(vk_far_count_kernel), text, st.m, st.p.carry, st.p.uhdr, st.d_nrec,
                    FaRecs{st.p.rec_first}, d_slot, nslots, d_hist);
}

int vk_count_fasta_windows_device(vk_ctx* ctx, const void* d_fasta, const uint64_t* offsets, const uint64_t* lengths, uint32_t nsamples,
                                  int k, const uint64_t* rec_first, const uint64_t* d_rec_bases, const uint64_t* d_win_first,
                                  uint32_t win_len, uint32_t win_step, uint64_t row_lo, uint32_t nrows, uint32_t tile_rows,
                                  uint32_t* d_hist) {
    if (!ctx || !offsets || !lengths || !rec_first || !d_rec_bases || !d_win_first || !d_hist) return VK_EINVAL;
    FaCall c{};
    c.offsets = offsets, c.lengths = lengths, c.nsamples = nsamples, c.k = k, c.rec_first = rec_first;
    c.win_len = win_len, c.win_step = win_step, c.nrows = nrows, c.tile_rows = tile_rows;
    uint32_t steps = 0;
    uint64_t sum_wgs = 0;
    if (int rc = count_fasta_windows_check(c, &steps)) return rc;
    if (nsamples && !fa_text_ok(d_fasta)) return VK_EINVAL;
    // (the wart: the offsets before the reset, the rest of the plan's rules behind it)
    if (!fa_offsets_ok(offsets, nsamples)) return VK_EINVAL;
    if (int rc = faw_sum_check(c, steps, &sum_wgs)) return rc;
    const size_t ncode = static_cast<size_t>(1) << (2 * k);
    VK_HIP(ctx, hipSetDevice(ctx->device));
    VK_HIP(ctx, hipMemsetAsync(d_hist, 0, nrows * ncode * sizeof(uint32_t), ctx->stream));
    const uint64_t total = nsamples ? rec_first[nsamples] : 0;
    if (total == 0) return VK_OK;
    const uint8_t* text = static_cast<const uint8_t*>(d_fasta);
    FarState st;
    int rc = far_prepare(ctx, text, offsets, lengths, nsamples, rec_first, nullptr, nullptr, &st);
    if (rc) return rc;
    const FaPlan& pl = st.pl;
    if (pl.nwg == 0) return VK_OK;
    FawPieces w{};
    rc = ws_carve(ctx, &ctx->d_fawin, &ctx->fawin_cap, [&](WsTake& take) { faw_take(take, w, pl, total, steps, tile_rows, k); });
    if (rc) return rc;
    if (steps > 1) VK_HIP(ctx, hipMemsetAsync(w.tiles, 0, tile_rows * ncode * sizeof(uint32_t), ctx->stream));
    rc = fa_ord_run(ctx, text, pl, st.m, st.p.carry, w.lane, w.unit_ord, w.bases);
    if (rc) return rc;
    const uint32_t cap = steps > 1 ? tile_rows : nrows;
    hipLaunchKernelGGL(vk_faw_plan_kernel, dim3(1), dim3(kFaThreads), 0, ctx->stream, reinterpret_cast<const unsigned long long*>(d_rec_bases),
                       reinterpret_cast<const unsigned long long*>(d_win_first), total, win_len, win_step, row_lo, nrows, cap, w.recs, w.used);
    VK_HIP(ctx, hipGetLastError());
    rc = launch_k(ctx, k, pl.nwg, FA_KERNEL(vk_faw_count_kernel), text, st.m, st.p.carry, st.p.uhdr, st.d_nrec, FaRecs{st.p.rec_first},
                  w.lane, w.unit_ord, w.recs, win_step, steps > 1 ? w.tiles : d_hist, cap);
    if (rc) return rc;
    if (steps > 1) {
        hipLaunchKernelGGL(vk_faw_sum_kernel, dim3(static_cast<uint32_t>(sum_wgs)), dim3(kFaThreads), 0, ctx->stream, w.recs,
                           reinterpret_cast<const unsigned long long*>(d_win_first), total, w.used, w.tiles, static_cast<uint32_t>(ncode),
                           steps, row_lo, nrows, d_hist);
        VK_HIP(ctx, hipGetLastError());
    }
    return VK_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- BAM to FASTQ (vk_bam.h, vk_bam_groups.h) ---------
// The four calls are one sequence (bam_run): what a call carries, the rules of its arguments, the plans and the host's
// tables and what is made of the results are vk_bamplan.h's; the workspaces, copies and launches are here.

namespace {

// What the link pass reports is ONE run of pieces, so that one copy brings it back: the same statement lays out the run in
// the device's workspace and, over a host buffer, its mirror.
struct BamBack {
    BamFile* files;
    unsigned long long* link;   // segments, segments walked again
};
void bam_back(WsTake& take, BamBack& b, uint32_t nfiles) {
    take(b.files, nfiles);
    take(b.link, 2);
}

// d_bamws: the descriptors (made on the host, uploaded as one block) and the device-only pieces of the framing.
struct BamPieces {
    uint64_t *offs, *lens, *first, *seg_first, *sseg_first, *out_offs, *out_caps;
    int32_t* n_ref;
    uint32_t *stream_file, *stream_select;
    size_t desc_bytes;
    BamSeg* segs;
    uint16_t* starts;   // bam_starts_cap per segment
    BamBack back;
    size_t back_bytes;
};

void bam_take(WsTake& take, BamPieces& p, uint32_t nfiles, const BamPlan& pl) {
    take(p.offs, nfiles);
    take(p.lens, nfiles);
    take(p.first, nfiles);
    take(p.seg_first, nfiles + 1ull);
    take(p.sseg_first, pl.nstreams + 1ull);
    take(p.out_offs, pl.nstreams);
    take(p.out_caps, pl.nstreams);
    take(p.n_ref, nfiles);
    take(p.stream_file, pl.nstreams);
    take(p.stream_select, pl.nstreams);
    p.desc_bytes = take.at;
    take(p.segs, pl.segs);
    take(p.starts, pl.segs * bam_starts_cap(pl.seg));
    const size_t at = take.at;
    bam_back(take, p.back, nfiles);
    p.back_bytes = take.at - at;
}

template <class T>
void bam_put(T* dst, const T* src, size_t n) {
    if (n) memcpy(dst, src, n * sizeof(T));
}

// What the calls share: the descriptors on the device, the plan, the link pass's results on the host.
struct BamState {
    BamPieces d{};
    BamPlan plan;
    BamMeta m;
    BamStreams ss;
    std::vector<uint8_t> mirror;   // (host) of d.back, once bam_finish has run: `h` points into it
    BamBack h{};
};

// Segment pass and link pass.
int bam_frame(vk_ctx* ctx, const BamCall& c, BamState* st) {
    st->plan = bam_plan(c, ctx->bam_seg_bytes);
    const BamPlan& pl = st->plan;
    if (!pl.ok) return VK_EINVAL;
    const uint32_t nfiles = c.nfiles;
    BamPieces h{};
    WsTake size{nullptr, 0};
    bam_take(size, h, nfiles, pl);
    std::vector<uint8_t> host(h.desc_bytes, 0);
    WsTake on_host{host.data(), 0};
    bam_take(on_host, h, nfiles, pl);
    bam_put(h.offs, c.offsets, nfiles);
    bam_put(h.lens, c.lengths, nfiles);
    bam_put(h.first, c.first_record, nfiles);
    bam_put(h.seg_first, pl.seg_first.data(), pl.seg_first.size());
    bam_put(h.sseg_first, pl.sseg_first.data(), pl.sseg_first.size());
    bam_put(h.out_offs, pl.out_offs.data(), pl.nstreams);
    bam_put(h.out_caps, pl.out_caps.data(), pl.nstreams);
    bam_put(h.n_ref, c.n_ref, nfiles);
    bam_put(h.stream_file, c.stream_file, pl.nstreams);
    bam_put(h.stream_select, c.stream_select, pl.nstreams);
    int rc = ws_carve(ctx, &ctx->d_bamws, &ctx->bamws_cap, [&](WsTake& take) { bam_take(take, st->d, nfiles, pl); });
    if (rc) return rc;
    const BamPieces& d = st->d;
    // (a pageable source: the copy has read it on return)
    VK_HIP(ctx, hipMemcpyAsync(ctx->d_bamws, host.data(), host.size(), hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipMemsetAsync(d.back.link, 0, 2 * sizeof(unsigned long long), ctx->stream));
    st->m = BamMeta{d.offs, d.lens, d.first, d.seg_first, d.n_ref, nfiles, pl.seg};
    st->ss = BamStreams{d.stream_file, d.stream_select, d.sseg_first, d.out_offs, d.out_caps, pl.nstreams};
    hipLaunchKernelGGL(vk_bam_segment_kernel, dim3(static_cast<uint32_t>(pl.segs)), dim3(64), 0, ctx->stream, c.d_bam, st->m, c.exclude,
                       c.flags, d.segs, d.starts);
    VK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(vk_bam_link_kernel, dim3(nfiles), dim3(64), 0, ctx->stream, c.d_bam, st->m, c.exclude, d.segs, d.starts,
                       d.back.files, d.back.link);
    VK_HIP(ctx, hipGetLastError());
    return VK_OK;
}

int bam_emit(vk_ctx* ctx, const BamCall& c, const BamState& st) {
    if (st.plan.stream_segs == 0) return VK_OK;
    hipLaunchKernelGGL(vk_bam_emit_kernel, dim3(static_cast<uint32_t>(st.plan.stream_segs)), dim3(kBamEmitThreads), 0, ctx->stream,
                       c.d_bam, st.m, st.ss, c.exclude, st.d.segs, st.d.starts, st.d.back.files, c.d_out);
    VK_HIP(ctx, hipGetLastError());
    return VK_OK;
}

// The link pass's results on the host (st->h); synchronises.
int bam_finish(vk_ctx* ctx, uint32_t nfiles, BamState* st) {
    st->mirror.resize(st->d.back_bytes);
    WsTake on_host{st->mirror.data(), 0};
    bam_back(on_host, st->h, nfiles);
    VK_HIP(ctx, hipMemcpyAsync(st->mirror.data(), st->d.back.files, st->d.back_bytes, hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->bam_segments = st->h.link[0];
    ctx->bam_rewalked = st->h.link[1];
    return VK_OK;
}

struct BgState {
    BgPieces d{};
    BgCounts n;
    BamGroupsMeta G{};
};

// Behind bam_frame, for a grouped call: the tables, the count pass and the scan.
int bg_count(vk_ctx* ctx, const BamCall& c, const BamState& st, BgState* bg) {
    const uint32_t panel = ctx->bam_panel_segs ? ctx->bam_panel_segs : kBamPanelSegs;
    bg->n = bg_counts(c, st.plan.seg, panel);
    const BgCounts& n = bg->n;
    std::vector<uint8_t> host;
    bg_describe(c, n, host);
    int rc = ws_carve(ctx, &ctx->d_bamgws, &ctx->bamgws_cap, [&](WsTake& take) { bg_take(take, bg->d, c.nfiles, c.nstreams, n); });
    if (rc) return rc;
    const BgPieces& d = bg->d;
    // (a pageable source: the copy has read it on return)
    VK_HIP(ctx, hipMemcpyAsync(ctx->d_bamgws, host.data(), host.size(), hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipMemsetAsync(d.aux_bad, 0, c.nfiles * sizeof(uint32_t), ctx->stream));
    VK_HIP(ctx, hipMemsetAsync(d.counters, 0, sizeof(unsigned long long), ctx->stream));
    bg->G = BamGroupsMeta{d.ids, d.group_first, d.id_first, d.slots, d.slot_first, d.map, d.map_first, d.ls_first, d.ls_stream,
                          d.pan_first, d.row_first, panel};
    hipLaunchKernelGGL(vk_bam_groups_count_kernel, dim3(static_cast<uint32_t>(n.panels)), dim3(kBamCountThreads),
                       n.max_ls * 2 * sizeof(unsigned long long), ctx->stream, c.d_bam, st.m, bg->G, c.exclude, st.d.segs, st.d.starts,
                       st.d.back.files, d.notes, d.rows, d.aux_bad, d.counters);
    VK_HIP(ctx, hipGetLastError());
    if (c.nstreams) {
        hipLaunchKernelGGL(vk_bam_groups_scan_kernel, dim3((c.nstreams + 3) / 4), dim3(256), 0, ctx->stream, st.m, bg->G, d.stream_file,
                           d.stream_local, c.nstreams, st.d.back.files, d.aux_bad, d.rows, d.totals);
        VK_HIP(ctx, hipGetLastError());
    }
    return VK_OK;
}

int bg_emit(vk_ctx* ctx, const BamCall& c, const BamState& st, const BgState& bg) {
    if (c.nstreams == 0) return VK_OK;
    // a workgroup per panel: the grid does not depend on the streams
    hipLaunchKernelGGL(vk_bam_groups_emit_kernel, dim3(static_cast<uint32_t>(bg.n.panels)), dim3(kBamEmitThreads),
                       bg.n.max_ls * sizeof(unsigned long long), ctx->stream, c.d_bam, st.m, bg.G, bg.d.out_offs, bg.d.out_caps,
                       st.d.segs, st.d.starts, bg.d.notes, st.d.back.files, bg.d.aux_bad, bg.d.rows, bg.d.totals, c.d_out);
    VK_HIP(ctx, hipGetLastError());
    ctx->bam_groups_wgs = bg.n.panels;
    return VK_OK;
}

// The results of a grouped call on the host: totals[nstreams], aux_bad[nfiles], and bam_finish's; synchronises.
int bg_finish(vk_ctx* ctx, const BamCall& c, BamState* st, const BgState& bg, std::vector<BamRow>* totals, std::vector<uint32_t>* aux_bad) {
    totals->assign(c.nstreams, BamRow{0, 0});
    std::vector<uint8_t> mirror(bg.d.back_bytes);
    uint32_t* h_bad = nullptr;
    unsigned long long* h_walked = nullptr;
    WsTake on_host{mirror.data(), 0};
    bg_back(on_host, h_bad, h_walked, c.nfiles);
    if (c.nstreams)
        VK_HIP(ctx, hipMemcpyAsync(totals->data(), bg.d.totals, c.nstreams * sizeof(BamRow), hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(mirror.data(), bg.d.aux_bad, mirror.size(), hipMemcpyDeviceToHost, ctx->stream));
    int rc = bam_finish(ctx, c.nfiles, st);
    if (rc) return rc;
    ctx->bam_groups_walked = *h_walked;
    aux_bad->assign(h_bad, h_bad + c.nfiles);
    return VK_OK;
}

// What a call wants back: per stream the reads and text bytes (a framing call) or the text's length (a text call), per
// file the status.
struct BamWant {
    uint64_t *records, *bytes, *lengths;
    uint32_t* status;
};

// The one sequence of the four calls: check, reset the counters of the last call, frame, (grouped: count and scan),
// (text: emit), finish, write the results.
int bam_run(vk_ctx* ctx, const BamCall& c, const BamWant& w) {
    if (!ctx || !bam_args_ok(c) || (c.nfiles && (!c.d_bam || !w.status))) return VK_EINVAL;
    if (c.nstreams && (c.text ? !c.d_out || !c.out_offsets || !c.out_caps || !w.lengths : !w.records || !w.bytes)) return VK_EINVAL;
    if (c.grouped && !bg_args_ok(c)) return VK_EINVAL;
    ctx->bam_segments = ctx->bam_rewalked = 0;
    if (c.grouped) ctx->bam_groups_wgs = ctx->bam_groups_walked = 0;
    if (c.nfiles == 0) return VK_OK;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    BamState st;
    BgState bg;
    std::vector<BamRow> totals;      // a grouped call's streams
    std::vector<uint32_t> aux_bad;   // ... and files
    int rc = bam_frame(ctx, c, &st);
    if (rc == VK_OK && c.grouped) rc = bg_count(ctx, c, st, &bg);
    if (rc == VK_OK && c.text) rc = c.grouped ? bg_emit(ctx, c, st, bg) : bam_emit(ctx, c, st);
    if (rc == VK_OK) rc = c.grouped ? bg_finish(ctx, c, &st, bg, &totals, &aux_bad) : bam_finish(ctx, c.nfiles, &st);
    if (rc) return rc;
    const BamFile* files = st.h.files;
    for (uint32_t i = 0; i < c.nfiles; ++i) w.status[i] = bam_status_of(files[i].status, c.grouped ? aux_bad[i] : 0u);
    for (uint32_t s = 0; s < c.nstreams; ++s) {
        const BamFile& f = files[c.stream_file[s]];
        const BamRow got = c.grouped ? totals[s] : BamRow{bam_host_pick(f.recs, c.stream_select[s]), bam_host_pick(f.bytes, c.stream_select[s])};
        if (!c.text) {
            w.records[s] = got.recs;
            w.bytes[s] = got.bytes;
        } else if (!bam_slot_fits(got.bytes, c.out_caps[s], &w.lengths[s])) {
            rc = VK_ENOSPC;
        }
    }
    return rc;
}

}  // namespace

extern "C" {

int vk_bam_frame_device(vk_ctx* ctx, const void* d_bam, const uint64_t* offsets, const uint64_t* lengths, const uint64_t* first_record,
                        const int32_t* n_ref, uint32_t nfiles, const uint32_t* stream_file, const uint32_t* stream_select,
                        uint32_t nstreams, uint32_t exclude, uint32_t flags, uint64_t* out_records, uint64_t* out_bytes,
                        uint32_t* status) {
    const BamCall c{static_cast<const uint8_t*>(d_bam), offsets, lengths, first_record, n_ref, nfiles, nullptr, nullptr, nullptr,
                    stream_file, stream_select, nullptr, nstreams, nullptr, nullptr, nullptr, exclude, flags, false, false};
    return bam_run(ctx, c, BamWant{out_records, out_bytes, nullptr, status});
}

int vk_bam_fastq_device(vk_ctx* ctx, const void* d_bam, const uint64_t* offsets, const uint64_t* lengths, const uint64_t* first_record,
                        const int32_t* n_ref, uint32_t nfiles, const uint32_t* stream_file, const uint32_t* stream_select,
                        uint32_t nstreams, uint32_t exclude, uint32_t flags, void* d_out, const uint64_t* out_offsets,
                        const uint64_t* out_caps, uint64_t* out_lengths, uint32_t* status) {
    const BamCall c{static_cast<const uint8_t*>(d_bam), offsets, lengths, first_record, n_ref, nfiles, nullptr, nullptr, nullptr,
                    stream_file, stream_select, nullptr, nstreams, static_cast<uint8_t*>(d_out), out_offsets, out_caps, exclude, flags,
                    false, true};
    return bam_run(ctx, c, BamWant{nullptr, nullptr, out_lengths, status});
}

int vk_last_bam_frame(const vk_ctx* ctx, uint64_t* segments, uint64_t* rewalked) {
    if (!ctx || !segments || !rewalked) return VK_EINVAL;
    *segments = ctx->bam_segments;
    *rewalked = ctx->bam_rewalked;
    return VK_OK;
}

int vk_bam_groups_workspace_size(const uint64_t* lengths, uint32_t nfiles, const uint32_t* group_first, const uint32_t* id_first,
                                 const uint32_t* stream_file, uint32_t nstreams, uint32_t seg_bytes, uint32_t panel_segs,
                                 uint64_t* bytes) {
    if (!bytes || (nfiles && (!lengths || !group_first || !id_first)) || (nstreams && !stream_file)) return VK_EINVAL;
    if ((seg_bytes && (seg_bytes < 64 || seg_bytes > kBamSegBytes)) || panel_segs > 4096) return VK_EINVAL;
    for (uint32_t s = 0; s < nstreams; ++s)
        if (stream_file[s] >= nfiles) return VK_EINVAL;
    BamCall c{};
    c.lengths = lengths;
    c.nfiles = nfiles;
    c.group_first = group_first;
    c.id_first = id_first;
    c.stream_file = stream_file;
    c.nstreams = nstreams;
    *bytes = bg_workspace_bytes(c, seg_bytes ? seg_bytes : kBamSegBytes, panel_segs ? panel_segs : kBamPanelSegs);
    return VK_OK;
}

int vk_bam_groups_frame_device(vk_ctx* ctx, const void* d_bam, const uint64_t* offsets, const uint64_t* lengths,
                               const uint64_t* first_record, const int32_t* n_ref, uint32_t nfiles, const uint32_t* group_first,
                               const uint32_t* id_first, const uint8_t* id_bytes, const uint32_t* stream_file,
                               const uint32_t* stream_select, const uint32_t* stream_group, uint32_t nstreams, uint32_t exclude,
                               uint32_t flags, uint64_t* out_records, uint64_t* out_bytes, uint32_t* status) {
    const BamCall c{static_cast<const uint8_t*>(d_bam), offsets, lengths, first_record, n_ref, nfiles, group_first, id_first, id_bytes,
                    stream_file, stream_select, stream_group, nstreams, nullptr, nullptr, nullptr, exclude, flags, true, false};
    return bam_run(ctx, c, BamWant{out_records, out_bytes, nullptr, status});
}

int vk_bam_groups_fastq_device(vk_ctx* ctx, const void* d_bam, const uint64_t* offsets, const uint64_t* lengths,
                               const uint64_t* first_record, const int32_t* n_ref, uint32_t nfiles, const uint32_t* group_first,
                               const uint32_t* id_first, const uint8_t* id_bytes, const uint32_t* stream_file,
                               const uint32_t* stream_select, const uint32_t* stream_group, uint32_t nstreams, uint32_t exclude,
                               uint32_t flags, void* d_out, const uint64_t* out_offsets, const uint64_t* out_caps, uint64_t* out_lengths,
                               uint32_t* status) {
    const BamCall c{static_cast<const uint8_t*>(d_bam), offsets, lengths, first_record, n_ref, nfiles, group_first, id_first, id_bytes,
                    stream_file, stream_select, stream_group, nstreams, static_cast<uint8_t*>(d_out), out_offsets, out_caps, exclude,
                    flags, true, true};
    return bam_run(ctx, c, BamWant{nullptr, nullptr, out_lengths, status});
}

int vk_last_bam_groups(const vk_ctx* ctx, uint64_t* emit_workgroups, uint64_t* walked) {
    if (!ctx || !emit_workgroups || !walked) return VK_EINVAL;
    *emit_workgroups = ctx->bam_groups_wgs;
    *walked = ctx->bam_groups_walked;
    return VK_OK;
}

}  // extern "C"

// ------------------------------------------- reads screened against a reference (vk_screen.h) ------

namespace {

// (the rules, sc_build_layout and sc_layout: vk_textplan.h)

// The tail of the calls that keep records (screen, depth filter): the scan of the records' kept bytes, the text, and per
// sample its length and the zeros up to its 16-byte rounded end.
int kept_text_run(vk_ctx* ctx, const uint8_t* text, const ScLayout& L, uint32_t nsamples, uint64_t nrec, uint8_t* d_out,
                  uint64_t* d_out_lengths) {
    int rc = cl_scan(ctx, L.obytes, nrec, L.c.sums, L.oprefix);
    if (rc) return rc;
    if (nrec)
        hipLaunchKernelGGL(vk_sc_write_kernel, dim3(static_cast<uint32_t>(text_record_blocks(nrec))), dim3(kClThreads), 0, ctx->stream,
                           text, L.rec_base, L.out_offs, nsamples, nrec, L.c.recs, L.oprefix, d_out);
    hipLaunchKernelGGL(vk_sc_pad_kernel, dim3((nsamples + kClThreads - 1) / kClThreads), dim3(kClThreads), 0, ctx->stream, L.rec_base,
                       L.out_offs, nsamples, L.oprefix, d_out, d_out_lengths);
    VK_HIP(ctx, hipGetLastError());
    return VK_OK;
}

}  // namespace

extern "C" {

int vk_screen_build_workspace_size(uint64_t length, uint64_t* bytes) {
    if (!bytes || length > VK_SCREEN_MAX_REF) return VK_EINVAL;
    *bytes = sc_build_layout(nullptr, length).total;
    return VK_OK;
}

int vk_screen_build_device(vk_ctx* ctx, const void* d_fasta, uint64_t length, int k, uint64_t* d_table, uint64_t nslots,
                           void* d_ws, uint64_t ws_bytes, uint64_t* windows, uint64_t* distinct, uint32_t* status) {
    if (!ctx || !d_ws || !windows || !distinct || !status) return VK_EINVAL;
    // (a reference too long is refused here: before anything is allocated or uploaded)
    if (int rc = screen_build_check(length, k, d_table != nullptr, nslots)) return rc;
    if (!d_fasta || (reinterpret_cast<uintptr_t>(d_fasta) & 15u) != 0) return VK_EINVAL;
    const ScBuildLayout L = sc_build_layout(d_ws, length);
    if (ws_bytes < L.total) return VK_EINVAL;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    FaPlan pl;
    const uint64_t zero = 0;
    int rc = fa_plan(ctx->fasta_unit_bytes, &zero, &length, 1, &pl);
    if (rc) return rc;
    const uint8_t* text = static_cast<const uint8_t*>(d_fasta);
    FaMeta m;
    rc = fa_state_run(ctx, text, pl, L.f, L.status, &m, [&] {
        VK_HIP(ctx, hipMemsetAsync(L.out, 0, sizeof(ScBuildOut), ctx->stream));
        if (d_table) VK_HIP(ctx, hipMemsetAsync(d_table, 0xFF, nslots * sizeof(uint64_t), ctx->stream));
        return VK_OK;
    });
    if (rc) return rc;
    if (pl.nwg) {
        const dim3 grid(static_cast<uint32_t>(pl.nwg)), block(kFaThreads);
        if (d_table)
            hipLaunchKernelGGL(vk_sc_build_kernel<true>, grid, block, 0, ctx->stream, text, m, L.f.carry, static_cast<uint32_t>(k), d_table,
                               nslots, L.out);
        else
            hipLaunchKernelGGL(vk_sc_build_kernel<false>, grid, block, 0, ctx->stream, text, m, L.f.carry, static_cast<uint32_t>(k), d_table,
                               nslots, L.out);
        VK_HIP(ctx, hipGetLastError());
    }
    ScBuildOut out{};
    VK_HIP(ctx, hipMemcpyAsync(&out, L.out, sizeof(out), hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(status, L.status, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *windows = out.windows;
    *distinct = out.distinct;
    // (a table without a free slot would be no table: a probe for an absent key ends at one)
    return d_table && (out.full || out.distinct >= nslots) ? VK_ENOSPC : VK_OK;
}

int vk_screen_workspace_size(const uint64_t* records, uint32_t nsamples, const uint64_t* lengths, uint64_t* bytes) {
    if (!bytes || (nsamples && (!records || !lengths))) return VK_EINVAL;
    *bytes = sc_layout(nullptr, records, nsamples, lengths).total;
    return VK_OK;
}

int vk_screen_device(vk_ctx* ctx, const void* d_fastq, const uint64_t* offsets, const uint64_t* lengths, const uint64_t* records,
                     uint32_t nsamples, const uint64_t* d_table, uint64_t nslots, int k, uint32_t min_hits, int keep,
                     uint8_t* d_out, const uint64_t* out_offsets, uint64_t out_capacity, uint64_t* d_out_lengths,
                     uint64_t* d_stats, uint32_t* d_status, void* d_ws, uint64_t ws_bytes) {
    if (!ctx || nsamples == 0 || !d_fastq || !offsets || !lengths || !records || !d_table || !d_out || !out_offsets ||
        !d_out_lengths || !d_stats || !d_status || !d_ws)
        return VK_EINVAL;
    TextCall c{};
    c.offsets = offsets, c.lengths = lengths, c.records = records, c.nsamples = nsamples;
    c.out_offsets = out_offsets, c.out_capacity = out_capacity, c.k = k, c.min_hits = min_hits;
    if (int rc = screen_check(c, nslots)) return rc;
    const ScLayout L = sc_layout(d_ws, records, nsamples, lengths);
    if (ws_bytes < L.total) return VK_EINVAL;
    const TextIndex t = text_index(offsets, lengths, records, nsamples);
    const uint64_t nrec = t.rec_base[nsamples];
    const auto* text = static_cast<const uint8_t*>(d_fastq);
    int rc = text_index_run(ctx, text, t, L.c, L.samples, L.rec_base, d_status, [&] {
        VK_HIP(ctx, hipMemcpyAsync(L.out_offs, out_offsets, nsamples * 8ull, hipMemcpyHostToDevice, ctx->stream));
        VK_HIP(ctx, hipMemsetAsync(d_stats, 0, nsamples * 4ull * sizeof(uint64_t), ctx->stream));
        return VK_OK;
    });
    if (rc) return rc;
    if (nrec) {
        const ScParams P{d_table, nslots, static_cast<uint32_t>(k), min_hits, keep ? 1u : 0u,
                         ctx->screen_tile ? ctx->screen_tile : kScMaxTile};
        hipLaunchKernelGGL(vk_sc_match_kernel, dim3(static_cast<uint32_t>(text_record_blocks(nrec))), dim3(kClThreads), 0, ctx->stream,
                           text, L.samples, L.rec_base, nsamples, nrec, L.c.recs, d_status, P, L.obytes,
                           reinterpret_cast<unsigned long long*>(d_stats));
    }
    VK_HIP(ctx, hipGetLastError());
    return kept_text_run(ctx, text, L, nsamples, nrec, d_out, d_out_lengths);
}

}  // extern "C"

// ------------------------------------------- the k-mer spectrum of cleaned reads (vk_spectrum.h) ------

namespace {

// (the rules, the table plan and sp_layout: vk_textplan.h)

// The samples' tables, for the spectrum of reads and of assemblies alike: their descriptors go up and the rows are reset ...
int sp_tables_put(vk_ctx* ctx, const SpTablePieces& T, const std::vector<uint64_t>& block_base, const uint64_t* slot_base,
                  const uint64_t* nslots, uint32_t nsamples, uint64_t* d_rows) {
    VK_HIP(ctx, hipMemcpyAsync(T.block_base, block_base.data(), block_base.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(T.slot_base, slot_base, nsamples * 8ull, hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(T.nslots, nslots, nsamples * 8ull, hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipMemsetAsync(d_rows, 0, static_cast<size_t>(nsamples) * kSpNstat * sizeof(uint64_t), ctx->stream));
    return VK_OK;
}

// ... and the table sequence: every slot freed, the call's count step (`count`, given the rows), the histogram, the rows
// finished.  nblocks: the table plan's workgroups (block_base[nsamples]).
template <class F>
int sp_tables_run(vk_ctx* ctx, const SpTablePieces& T, uint64_t nblocks, uint32_t nsamples, uint64_t* d_keys, uint32_t* d_counts,
                  uint32_t* d_status, uint64_t* d_rows, F&& count) {
    const dim3 tgrid(static_cast<uint32_t>(nblocks));
    auto* rows = reinterpret_cast<unsigned long long*>(d_rows);
    hipLaunchKernelGGL(vk_sp_init_kernel, tgrid, dim3(kClThreads), 0, ctx->stream, T.block_base, nsamples, T.slot_base, T.nslots, d_keys,
                       d_counts);
    count(rows);
    hipLaunchKernelGGL(vk_sp_hist_kernel, tgrid, dim3(kClThreads), 0, ctx->stream, T.block_base, nsamples, T.slot_base, T.nslots,
                       d_counts, d_status, rows);
    hipLaunchKernelGGL(vk_sp_finish_kernel, dim3(nsamples), dim3(kClThreads), 0, ctx->stream, d_status, rows);
    VK_HIP(ctx, hipGetLastError());
    return VK_OK;
}

}  // namespace

extern "C" {

int vk_spectrum_workspace_size(const uint64_t* records, uint32_t nsamples, const uint64_t* lengths, uint64_t* bytes) {
    if (!bytes || (nsamples && (!records || !lengths))) return VK_EINVAL;
    *bytes = sp_layout(nullptr, records, nsamples, lengths).total;
    return VK_OK;
}

int vk_spectrum_device(vk_ctx* ctx, const void* d_text, const uint64_t* offsets, const uint64_t* lengths, const uint64_t* records,
                       uint32_t nsamples, int k, uint32_t every, uint64_t* d_keys, uint32_t* d_counts, const uint64_t* slot_base,
                       const uint64_t* nslots, uint64_t* d_rows, uint32_t* d_status, void* d_ws, uint64_t ws_bytes) {
    if (!ctx || nsamples == 0 || !d_text || !offsets || !lengths || !records || !d_keys || !d_counts || !slot_base || !nslots ||
        !d_rows || !d_status || !d_ws)
        return VK_EINVAL;
    TextCall c{};
    c.offsets = offsets, c.lengths = lengths, c.records = records, c.nsamples = nsamples;
    c.nslots = nslots, c.slot_base = slot_base, c.k = k, c.every = every;
    std::vector<uint64_t> block_base;
    if (int rc = spectrum_check(c, &block_base)) return rc;
    const SpLayout L = sp_layout(d_ws, records, nsamples, lengths);
    if (ws_bytes < L.total) return VK_EINVAL;
    const TextIndex t = text_index(offsets, lengths, records, nsamples);
    const uint64_t nrec = t.rec_base[nsamples];
    const auto* text = static_cast<const uint8_t*>(d_text);
    int rc = text_index_run(ctx, text, t, L.c, L.samples, L.rec_base, d_status,
                            [&] { return sp_tables_put(ctx, L.t, block_base, slot_base, nslots, nsamples, d_rows); });
    if (rc) return rc;
    return sp_tables_run(ctx, L.t, block_base[nsamples], nsamples, d_keys, d_counts, d_status, d_rows, [&](unsigned long long* rows) {
        if (!nrec) return;
        const SpParams P{d_keys, d_counts, L.t.slot_base, L.t.nslots, static_cast<uint32_t>(k), every,
                         ctx->spectrum_tile ? ctx->spectrum_tile : kScMaxTile, ctx->spectrum_merge};
        hipLaunchKernelGGL(vk_sp_count_kernel, dim3(static_cast<uint32_t>(text_record_blocks(nrec))), dim3(kClThreads), 0, ctx->stream,
                           text, L.rec_base, nsamples, nrec, L.c.recs, d_status, P, rows);
    });
}

}  // extern "C"

// ------------------------------------------- the k-mer spectrum of assemblies, from FASTA text (vk_fasta_spectrum.h) ------

// (the rules and fs_layout: vk_textplan.h; the table sequence is the spectrum's, above)

extern "C" {

int vk_spectrum_fasta_workspace_size(const uint64_t* lengths, uint32_t nsamples, uint64_t* bytes) {
    if (!bytes || (nsamples && !lengths)) return VK_EINVAL;
    *bytes = fs_layout(nullptr, lengths, nsamples).total;
    return VK_OK;
}

int vk_spectrum_fasta_device(vk_ctx* ctx, const void* d_fasta, const uint64_t* offsets, const uint64_t* lengths, uint32_t nsamples,
                             int k, uint32_t every, uint64_t* d_keys, uint32_t* d_counts, const uint64_t* slot_base,
                             const uint64_t* nslots, uint64_t* d_rows, uint32_t* d_status, void* d_ws, uint64_t ws_bytes) {
    if (!ctx || nsamples == 0 || !d_fasta || !offsets || !lengths || !d_keys || !d_counts || !slot_base || !nslots || !d_rows ||
        !d_status || !d_ws)
        return VK_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_fasta) & 15u) != 0) return VK_EINVAL;
    TextCall c{};
    c.offsets = offsets, c.lengths = lengths, c.nsamples = nsamples;
    c.nslots = nslots, c.slot_base = slot_base, c.k = k, c.every = every;
    std::vector<uint64_t> block_base;
    if (int rc = spectrum_check(c, &block_base)) return rc;
    const FsLayout L = fs_layout(d_ws, lengths, nsamples);
    if (ws_bytes < L.total) return VK_EINVAL;
    FaPlan pl;
    int rc = fa_plan(ctx->fasta_unit_bytes, offsets, lengths, nsamples, &pl);
    if (rc) return rc;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    const auto* text = static_cast<const uint8_t*>(d_fasta);
    FaMeta m;
    rc = fa_state_run(ctx, text, pl, L.f, d_status, &m,
                      [&] { return sp_tables_put(ctx, L.t, block_base, slot_base, nslots, nsamples, d_rows); });
    if (rc) return rc;
    return sp_tables_run(ctx, L.t, block_base[nsamples], nsamples, d_keys, d_counts, d_status, d_rows, [&](unsigned long long* rows) {
        if (!pl.nwg) return;
        const SpParams P{d_keys, d_counts, L.t.slot_base, L.t.nslots, static_cast<uint32_t>(k), every, 0u, 0u};
        hipLaunchKernelGGL(vk_fs_count_kernel, dim3(static_cast<uint32_t>(pl.nwg)), dim3(kFaThreads), 0, ctx->stream, text, m, L.f.carry,
                           P, d_status, rows);
    });
}

}  // extern "C"

// ------------------------------------------- reads kept by their k-mers' depth in the spectrum's tables (vk_depth.h) ------

// (the rules and dp_layout: vk_textplan.h; the kept-text tail is the screen's)

extern "C" {

int vk_depth_workspace_size(const uint64_t* records, uint32_t nsamples, const uint64_t* lengths, uint64_t* bytes) {
    if (!bytes || (nsamples && (!records || !lengths))) return VK_EINVAL;
    *bytes = dp_layout(nullptr, records, nsamples, lengths).total;
    return VK_OK;
}

int vk_depth_device(vk_ctx* ctx, const void* d_text, const uint64_t* offsets, const uint64_t* lengths, const uint64_t* records,
                    uint32_t nsamples, int k, uint32_t every, const uint64_t* d_keys, const uint32_t* d_counts,
                    const uint64_t* slot_base, const uint64_t* nslots, const uint32_t* d_table_status, const uint32_t* lo,
                    const uint32_t* hi, uint8_t* d_out, const uint64_t* out_offsets, uint64_t out_capacity, uint64_t* d_out_lengths,
                    uint64_t* d_rows, uint32_t* d_status, void* d_ws, uint64_t ws_bytes) {
    if (!ctx || nsamples == 0 || !d_text || !offsets || !lengths || !records || !d_keys || !d_counts || !slot_base || !nslots ||
        !d_table_status || !lo || !hi || !d_out || !out_offsets || !d_out_lengths || !d_rows || !d_status || !d_ws)
        return VK_EINVAL;
    TextCall c{};
    c.offsets = offsets, c.lengths = lengths, c.records = records, c.nsamples = nsamples;
    c.nslots = nslots, c.slot_base = slot_base, c.out_offsets = out_offsets, c.out_capacity = out_capacity;
    c.lo = lo, c.hi = hi, c.k = k, c.every = every;
    if (int rc = depth_check(c)) return rc;
    const DpLayout L = dp_layout(d_ws, records, nsamples, lengths);
    if (ws_bytes < L.total) return VK_EINVAL;
    const TextIndex t = text_index(offsets, lengths, records, nsamples);
    const uint64_t nrec = t.rec_base[nsamples];
    const auto* text = static_cast<const uint8_t*>(d_text);
    int rc = text_index_run(ctx, text, t, L.s.c, L.s.samples, L.s.rec_base, d_status, [&] {
        VK_HIP(ctx, hipMemcpyAsync(L.s.out_offs, out_offsets, nsamples * 8ull, hipMemcpyHostToDevice, ctx->stream));
        VK_HIP(ctx, hipMemcpyAsync(L.slot_base, slot_base, nsamples * 8ull, hipMemcpyHostToDevice, ctx->stream));
        VK_HIP(ctx, hipMemcpyAsync(L.nslots, nslots, nsamples * 8ull, hipMemcpyHostToDevice, ctx->stream));
        VK_HIP(ctx, hipMemcpyAsync(L.lo, lo, nsamples * 4ull, hipMemcpyHostToDevice, ctx->stream));
        VK_HIP(ctx, hipMemcpyAsync(L.hi, hi, nsamples * 4ull, hipMemcpyHostToDevice, ctx->stream));
        VK_HIP(ctx, hipMemsetAsync(d_rows, 0, static_cast<size_t>(nsamples) * kDpNstat * sizeof(uint64_t), ctx->stream));
        return VK_OK;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(vk_dp_status_kernel, dim3((nsamples + kClThreads - 1) / kClThreads), dim3(kClThreads), 0, ctx->stream,
                       d_table_status, nsamples, d_status);
    if (nrec) {
        const DpParams P{d_keys, d_counts, L.slot_base, L.nslots, L.lo, L.hi, static_cast<uint32_t>(k), every,
                         ctx->spectrum_tile ? ctx->spectrum_tile : kScMaxTile, ctx->depth_merge};
        hipLaunchKernelGGL(vk_dp_match_kernel, dim3(static_cast<uint32_t>(text_record_blocks(nrec))), dim3(kClThreads), 0, ctx->stream,
                           text, L.s.samples, L.s.rec_base, nsamples, nrec, L.s.c.recs, d_status, P, L.s.obytes,
                           reinterpret_cast<unsigned long long*>(d_rows));
    }
    VK_HIP(ctx, hipGetLastError());
    return kept_text_run(ctx, text, L.s, nsamples, nrec, d_out, d_out_lengths);
}

}  // extern "C"

// ------------------------------------------- sketches from the spectrum's tables, and their pairs (vk_sketch.h) ------

namespace {

// the pieces of a vk_sketch_device workspace
struct SkLayout {
    uint64_t *block_base, *slot_base, *nslots;
    SkState* state;
    uint32_t* hist;
    uint64_t *cand, *cand2;   // the candidates, and the merges' other buffer
    uint64_t ncand;           // hashes of all the samples' buffers
    uint64_t max_cap;
    size_t total;
};

uint64_t sk_cap(uint64_t nslots, uint32_t s) {
    return (s + std::max(kSkMinSlack, nslots >> kSkDigitBits) + kSkRun - 1) / kSkRun * kSkRun;
}

uint64_t sk_per_block(uint64_t nslots) {
    return std::max(kSkMinPerBlock, (nslots + kSkMaxBlocksPerSample - 1) / kSkMaxBlocksPerSample);
}

bool sk_args_ok(const uint64_t* nslots, uint32_t nsamples, uint32_t s) {
    if (!nslots || nsamples == 0 || s < kSkMinS || s > kSkMaxS) return false;
    for (uint32_t i = 0; i < nsamples; ++i)
        if (nslots[i] < 1 || nslots[i] > kSkMaxSlots) return false;
    return true;
}

SkLayout sk_layout(void* d_ws, const uint64_t* nslots, uint32_t nsamples, uint32_t s) {
    SkLayout L{};
    for (uint32_t i = 0; i < nsamples; ++i) {
        L.ncand += sk_cap(nslots[i], s);
        L.max_cap = std::max(L.max_cap, sk_cap(nslots[i], s));
    }
    WsTake take{static_cast<uint8_t*>(d_ws), 0};
    take(L.block_base, nsamples + 1ull);
    take(L.slot_base, nsamples);
    take(L.nslots, nsamples);
    take(L.state, nsamples);
    take(L.hist, static_cast<size_t>(nsamples) * kSkBins);
    take(L.cand, L.ncand);
    take(L.cand2, L.ncand);
    L.total = take.at;
    return L;
}

}  // namespace

extern "C" {

int vk_sketch_workspace_size(const uint64_t* nslots, uint32_t nsamples, uint32_t s, uint64_t* bytes) {
    if (!bytes || !sk_args_ok(nslots, nsamples, s)) return VK_EINVAL;
    *bytes = sk_layout(nullptr, nslots, nsamples, s).total;
    return VK_OK;
}

int vk_sketch_device(vk_ctx* ctx, const uint64_t* d_keys, const uint32_t* d_counts, const uint64_t* slot_base, const uint64_t* nslots,
                     uint32_t nsamples, const uint32_t* d_status, uint32_t min_count, uint32_t s, uint64_t* d_hashes, uint64_t* d_info,
                     void* d_ws, uint64_t ws_bytes) {
    if (!ctx || !d_keys || !d_counts || !slot_base || !d_status || !d_hashes || !d_info || !d_ws || min_count < 1 ||
        !sk_args_ok(nslots, nsamples, s))
        return VK_EINVAL;
    const SkLayout L = sk_layout(d_ws, nslots, nsamples, s);
    if (ws_bytes < L.total) return VK_EINVAL;
    std::vector<uint64_t> block_base(nsamples + 1ull, 0);
    std::vector<SkState> state(nsamples);
    uint64_t at = 0;
    for (uint32_t i = 0; i < nsamples; ++i) {
        SkState S{};
        S.cand_base = at;
        S.per_block = sk_per_block(nslots[i]);
        S.mode = kSkAll;
        S.cap = static_cast<uint32_t>(sk_cap(nslots[i], s));
        at += S.cap;
        state[i] = S;
        block_base[i + 1] = block_base[i] + (nslots[i] + S.per_block - 1) / S.per_block;
    }
    // the sort's and the row's workgroups: a sample's chunks of kSkRun candidates, of kClThreads row entries
    const uint64_t chunks = L.max_cap / kSkRun, row_blocks = (s + kClThreads - 1) / kClThreads;
    if (block_base[nsamples] >= (1ull << 31) || chunks * nsamples >= (1ull << 31) || row_blocks * nsamples >= (1ull << 31))
        return VK_EINVAL;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    // (pageable sources: a copy has read its source on return)
    VK_HIP(ctx, hipMemcpyAsync(L.block_base, block_base.data(), block_base.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(L.slot_base, slot_base, nsamples * 8ull, hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(L.nslots, nslots, nsamples * 8ull, hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipMemcpyAsync(L.state, state.data(), nsamples * sizeof(SkState), hipMemcpyHostToDevice, ctx->stream));
    VK_HIP(ctx, hipMemsetAsync(L.hist, 0, static_cast<size_t>(nsamples) * kSkBins * sizeof(uint32_t), ctx->stream));
    const dim3 tgrid(static_cast<uint32_t>(block_base[nsamples]));
    for (uint32_t round = 0; round < kSkRounds; ++round) {
        hipLaunchKernelGGL(vk_sk_hist_kernel, tgrid, dim3(kClThreads), 0, ctx->stream, L.block_base, nsamples, L.slot_base, L.nslots,
                           d_keys, d_counts, d_status, min_count, round, L.state, L.hist);
        hipLaunchKernelGGL(vk_sk_pick_kernel, dim3(nsamples), dim3(kClThreads), 0, ctx->stream, d_status, round, s, L.state, L.hist);
    }
    hipLaunchKernelGGL(vk_sk_compact_kernel, tgrid, dim3(kClThreads), 0, ctx->stream, L.block_base, nsamples, L.slot_base, L.nslots,
                       d_keys, d_counts, d_status, min_count, L.state, L.cand);
    const dim3 sgrid(static_cast<uint32_t>(chunks * nsamples));
    hipLaunchKernelGGL(vk_sk_run_kernel, sgrid, dim3(kClThreads), 0, ctx->stream, d_status, L.state, static_cast<uint32_t>(chunks),
                       L.cand);
    uint64_t *src = L.cand, *dst = L.cand2;
    for (uint64_t width = kSkRun; width < L.max_cap; width *= 2) {
        hipLaunchKernelGGL(vk_sk_merge_kernel, sgrid, dim3(kClThreads), 0, ctx->stream, d_status, L.state,
                           static_cast<uint32_t>(chunks), static_cast<uint32_t>(width), src, dst);
        std::swap(src, dst);
    }
    hipLaunchKernelGGL(vk_sk_finish_kernel, dim3(static_cast<uint32_t>(row_blocks * nsamples)), dim3(kClThreads), 0, ctx->stream,
                       d_status, L.state, static_cast<uint32_t>(row_blocks), s, src, d_hashes, d_info);
    VK_HIP(ctx, hipGetLastError());
    return VK_OK;
}

int vk_sketch_pairs_device(vk_ctx* ctx, const uint64_t* d_q, const uint64_t* d_qlen, uint64_t nq, const uint64_t* d_r,
                           const uint64_t* d_rlen, uint64_t nr, uint32_t s, uint32_t* d_shared, uint32_t* d_seen) {
    if (!ctx || !d_q || !d_qlen || !d_r || !d_rlen || !d_shared || !d_seen || s < kSkMinS || s > kSkMaxS) return VK_EINVAL;
    if (nq < 1 || nr < 1 || nq > kSkMaxSide || nr > kSkMaxSide || nq * nr > kSkMaxPairs) return VK_EINVAL;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t blocks = (nq * nr + kSkPairsPerBlock - 1) / kSkPairsPerBlock;   // (2^30 at most)
    hipLaunchKernelGGL(vk_sk_pairs_kernel, dim3(static_cast<uint32_t>(blocks)), dim3(kClThreads), 0, ctx->stream, d_q, d_qlen,
                       static_cast<uint32_t>(nq), d_r, d_rlen, static_cast<uint32_t>(nr), s, d_shared, d_seen);
    VK_HIP(ctx, hipGetLastError());
    return VK_OK;
}

int vk_sketch_pair_blocks_device(vk_ctx* ctx, const uint64_t* d_q, const uint64_t* d_qlen, uint64_t nq, const uint64_t* d_r,
                                 const uint64_t* d_rlen, uint64_t nr, uint32_t s, uint32_t* d_shared, uint32_t* d_seen) {
    if (!ctx || !d_q || !d_qlen || !d_r || !d_rlen || !d_shared || !d_seen || s < kSkMinS || s > kSkMaxS) return VK_EINVAL;
    if (nq < 1 || nr < 1 || nq > kSkMaxSide || nr > kSkMaxSide || nq * nr > kSkMaxBlockPairs) return VK_EINVAL;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t blocks = (nq * nr + kSkPairsPerBlock - 1) / kSkPairsPerBlock;   // (2^24 at most)
    hipLaunchKernelGGL(vk_sk_pair_blocks_kernel, dim3(static_cast<uint32_t>(blocks)), dim3(kClThreads), 0, ctx->stream, d_q, d_qlen,
                       static_cast<uint32_t>(nq), d_r, d_rlen, static_cast<uint32_t>(nr), s, d_shared, d_seen);
    VK_HIP(ctx, hipGetLastError());
    return VK_OK;
}

}  // extern "C"

// ------------------------------------------- quality profiles of FASTQ streams (vk_qc.h) ------

// (the rules and qc_layout: vk_textplan.h)

extern "C" {

int vk_qc_workspace_size(const uint64_t* records, const uint64_t* lengths, uint32_t nstreams, uint64_t* bytes) {
    if (!bytes || (nstreams && (!records || !lengths))) return VK_EINVAL;
    *bytes = qc_layout(nullptr, records, lengths, nstreams).total;
    return VK_OK;
}

int vk_qc_device(vk_ctx* ctx, const void* d_text, const uint64_t* offsets, const uint64_t* lengths, const uint64_t* records,
                 uint32_t nstreams, uint64_t* d_rows, uint32_t* d_status, void* d_ws, uint64_t ws_bytes) {
    if (!ctx || nstreams == 0 || !d_text || !offsets || !lengths || !records || !d_rows || !d_status || !d_ws) return VK_EINVAL;
    const uint32_t per_block = ctx->qc_merge ? ctx->qc_merge : kQcMerge;
    TextCall c{};
    c.offsets = offsets, c.lengths = lengths, c.records = records, c.nsamples = nstreams;
    std::vector<uint64_t> block_base;
    if (int rc = qc_check(c, per_block, &block_base)) return rc;
    const uint64_t nblocks = block_base[nstreams];
    const QcLayout L = qc_layout(d_ws, records, lengths, nstreams);
    if (ws_bytes < L.total) return VK_EINVAL;
    const TextIndex t = text_index(offsets, lengths, records, nstreams);   // a stream is one file of the record index
    const auto* text = static_cast<const uint8_t*>(d_text);
    int rc = text_index_run(ctx, text, t, L.c, L.streams, nullptr, nullptr, [&] {
        VK_HIP(ctx, hipMemcpyAsync(L.block_base, block_base.data(), block_base.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        VK_HIP(ctx, hipMemsetAsync(L.bad, 0, nstreams * sizeof(uint32_t), ctx->stream));
        VK_HIP(ctx, hipMemsetAsync(d_rows, 0, static_cast<size_t>(nstreams) * kQcNstat * sizeof(uint64_t), ctx->stream));
        return VK_OK;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(vk_qc_status_kernel, dim3((nstreams + kClThreads - 1) / kClThreads), dim3(kClThreads), 0, ctx->stream, text,
                       L.streams, nstreams, L.c.cprefix, d_rows, d_status);
    if (nblocks)
        hipLaunchKernelGGL(vk_qc_count_kernel, dim3(static_cast<uint32_t>(nblocks)), dim3(kQcThreads), 0, ctx->stream, text, L.streams,
                           L.block_base, nstreams, per_block, L.c.recs, d_rows, d_status, L.bad);
    hipLaunchKernelGGL(vk_qc_finish_kernel, dim3(nstreams), dim3(kClThreads), 0, ctx->stream, d_rows, d_status, L.bad);
    VK_HIP(ctx, hipGetLastError());
    return VK_OK;
}

}  // extern "C"

// ------------------------------------------- distances and nearest neighbours of images (vk_dist.h) ------

namespace {

// the pieces of a vk_dist_device workspace
struct DistLayout {
    int8_t *q, *r;            // the prepared rows
    uint64_t *qnorm, *rnorm;
    uint64_t* strip;
    uint64_t strip_rows;
    size_t total;
};

DistLayout dist_layout(void* d_ws, uint64_t nq, uint64_t nr, uint64_t npix) {
    DistLayout L{};
    const uint64_t padded = dist_padded(npix);
    L.strip_rows = dist_strip_rows(nq, nr, VK_DIST_STRIP);
    WsTake take{static_cast<uint8_t*>(d_ws), 0};
    take(L.q, nq * padded);
    take(L.r, nr * padded);
    take(L.qnorm, nq);
    take(L.rnorm, nr);
    take(L.strip, L.strip_rows * nr);
    L.total = take.at;
    return L;
}

bool dist_args_ok(uint64_t nq, uint64_t nr, uint64_t npix, uint32_t nn) {
    return nq >= 1 && nq < (1ull << 31) && nr >= 1 && nr <= kDistMaxRefs && npix >= 1 && npix <= kDistMaxPix && nn >= 1 &&
           nn <= kDistMaxN && dist_key_fits(npix, dist_idx_bits(nr));
}

}  // namespace

extern "C" {

int vk_dist_workspace_size(uint64_t nq, uint64_t nr, uint64_t npix, uint32_t n_neighbours, int want_matrix, uint64_t* bytes) {
    (void)want_matrix;   // (the matrix goes to the caller's buffer)
    if (!bytes || !dist_args_ok(nq, nr, npix, n_neighbours)) return VK_EINVAL;
    *bytes = dist_layout(nullptr, nq, nr, npix).total;
    return VK_OK;
}

int vk_dist_device(vk_ctx* ctx, const void* d_q, uint64_t nq, const void* d_r, uint64_t nr, uint64_t npix, const uint32_t* d_qgroup,
                   const uint32_t* d_rgroup, uint32_t n_neighbours, uint32_t* d_idx, uint64_t* d_d2, uint64_t* d_matrix, void* d_ws,
                   uint64_t ws_bytes) {
    if (!ctx || !d_q || !d_r || !d_idx || !d_d2 || !d_ws || !dist_args_ok(nq, nr, npix, n_neighbours)) return VK_EINVAL;
    if ((d_qgroup == nullptr) != (d_rgroup == nullptr)) return VK_EINVAL;
    const DistLayout L = dist_layout(d_ws, nq, nr, npix);
    if (ws_bytes < L.total) return VK_EINVAL;
    const uint64_t padded = dist_padded(npix);
    const uint32_t bits = dist_idx_bits(nr);
    const bool self = d_q == d_r && nq == nr;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(vk_dist_prep_kernel, dim3(static_cast<uint32_t>(nq)), dim3(kDistThreads), 0, ctx->stream,
                       static_cast<const uint8_t*>(d_q), L.q, L.qnorm, npix, padded);
    if (!self)
        hipLaunchKernelGGL(vk_dist_prep_kernel, dim3(static_cast<uint32_t>(nr)), dim3(kDistThreads), 0, ctx->stream,
                           static_cast<const uint8_t*>(d_r), L.r, L.rnorm, npix, padded);
    const int8_t* refs = self ? L.q : L.r;
    const uint64_t* rnorm = self ? L.qnorm : L.rnorm;
    const uint64_t strip = dist_strip_rows(nq, nr, ctx->dist_strip && ctx->dist_strip < L.strip_rows ? ctx->dist_strip : L.strip_rows);
    const uint32_t jtiles = static_cast<uint32_t>((nr + kDistTile - 1) / kDistTile);
    for (uint64_t q0 = 0; q0 < nq; q0 += strip) {
        const uint32_t rows = static_cast<uint32_t>(std::min(strip, nq - q0));
        const uint64_t tiles = static_cast<uint64_t>((rows + kDistTile - 1) / kDistTile) * jtiles;
        if (tiles >= (1ull << 31)) return VK_EINVAL;
        hipLaunchKernelGGL(vk_dist_tile_kernel, dim3(static_cast<uint32_t>(tiles)), dim3(kDistThreads), 0, ctx->stream, L.q, refs, L.qnorm,
                           rnorm, q0, rows, static_cast<uint32_t>(nr), jtiles, padded, L.strip, d_matrix);
        hipLaunchKernelGGL(vk_dist_select_kernel, dim3(rows), dim3(kDistSelThreads), 0, ctx->stream, L.strip, q0,
                           static_cast<uint32_t>(nr), d_qgroup, d_rgroup, n_neighbours, bits, d_idx, d_d2);
    }
    VK_HIP(ctx, hipGetLastError());
    return VK_OK;
}

}  // extern "C"

// ------------------------------------------- neighbour-joining trees of distance matrices (vk_tree.h) ------

namespace {

// the pieces of a vk_tree_nj_device workspace
struct TrLayout {
    double* R;          // [ntrees][n], -inf for a retired slot
    TrBest* parts;      // [ntrees][strips][tiles]: the search workgroups' candidates
    uint32_t tiles, strips;
    size_t total;
};

bool tr_args_ok(uint32_t n, uint32_t ntrees) {
    return n >= kTrMinLeaves && n <= kTrMaxLeaves && ntrees >= 1 && ntrees <= kTrMaxTrees;
}

TrLayout tr_layout(void* d_ws, uint32_t n, uint32_t ntrees) {
    TrLayout L{};
    L.tiles = (n + kTrTile) / kTrTile;   // (columns 0 .. n: a lane's pair of an odd row begins one column early)
    L.strips = (n - 1 + kTrStrip - 1) / kTrStrip;
    WsTake take{static_cast<uint8_t*>(d_ws), 0};
    take(L.R, static_cast<size_t>(ntrees) * n);
    take(L.parts, static_cast<size_t>(ntrees) * L.tiles * L.strips);
    L.total = take.at;
    return L;
}

}  // namespace

extern "C" {

int vk_tree_workspace_size(uint32_t n, uint32_t ntrees, uint64_t* bytes) {
    if (!bytes || !tr_args_ok(n, ntrees)) return VK_EINVAL;
    *bytes = tr_layout(nullptr, n, ntrees).total;
    return VK_OK;
}

int vk_tree_nj_device(vk_ctx* ctx, double* d_dist, uint32_t n, uint32_t ntrees, uint32_t* d_nodes, double* d_lengths,
                      uint32_t* d_status, void* d_ws, uint64_t ws_bytes) {
    if (!ctx || !d_dist || !d_nodes || !d_lengths || !d_status || !d_ws || !tr_args_ok(n, ntrees)) return VK_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_dist) & 7u) || (reinterpret_cast<uintptr_t>(d_ws) & 15u)) return VK_EINVAL;
    const TrLayout L = tr_layout(d_ws, n, ntrees);
    if (ws_bytes < L.total) return VK_EINVAL;
    const size_t rec = static_cast<size_t>(ntrees) * tr_record_len(n);
    VK_HIP(ctx, hipSetDevice(ctx->device));
    VK_HIP(ctx, hipMemsetAsync(d_status, 0, static_cast<size_t>(ntrees) * sizeof(uint32_t), ctx->stream));
    VK_HIP(ctx, hipMemsetAsync(d_nodes, 0, rec * sizeof(uint32_t), ctx->stream));
    VK_HIP(ctx, hipMemsetAsync(d_lengths, 0, rec * sizeof(double), ctx->stream));
    hipLaunchKernelGGL(vk_tr_init_kernel, dim3(n, ntrees), dim3(kClThreads), 0, ctx->stream, d_dist, n, L.R, d_status);
    const dim3 sgrid(L.tiles, L.strips, ntrees);
    for (uint32_t step = 0; step + 3 < n; ++step) {   // m = n - step active slots
        hipLaunchKernelGGL(vk_tr_search_kernel, sgrid, dim3(kClThreads), 0, ctx->stream, d_dist, n, n - step, L.R, d_status, L.R,
                           L.parts);
        hipLaunchKernelGGL(vk_tr_join_kernel, dim3(ntrees), dim3(kClThreads), 0, ctx->stream, d_dist, n, n - step, step, L.R, d_status,
                           L.parts, L.tiles * L.strips, d_nodes, d_lengths);
    }
    hipLaunchKernelGGL(vk_tr_close_kernel, dim3(ntrees), dim3(kClThreads), 0, ctx->stream, d_dist, n, L.R, d_status, d_nodes, d_lengths);
    VK_HIP(ctx, hipGetLastError());
    return VK_OK;
}

int vk_tree_search_probe_device(vk_ctx* ctx, const double* d_dist, uint32_t n, uint32_t ntrees, uint32_t launches, uint32_t* d_status,
                                void* d_ws, uint64_t ws_bytes) {
    if (!ctx || !d_dist || !d_status || !d_ws || !tr_args_ok(n, ntrees) || n < 4) return VK_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_dist) & 7u) || (reinterpret_cast<uintptr_t>(d_ws) & 15u)) return VK_EINVAL;
    const TrLayout L = tr_layout(d_ws, n, ntrees);
    if (ws_bytes < L.total) return VK_EINVAL;
    VK_HIP(ctx, hipSetDevice(ctx->device));
    VK_HIP(ctx, hipMemsetAsync(d_status, 0, static_cast<size_t>(ntrees) * sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(vk_tr_init_kernel, dim3(n, ntrees), dim3(kClThreads), 0, ctx->stream, d_dist, n, L.R, d_status);
    for (uint32_t i = 0; i < launches; ++i)
        hipLaunchKernelGGL(vk_tr_search_kernel, dim3(L.tiles, L.strips, ntrees), dim3(kClThreads), 0, ctx->stream, d_dist, n, n, L.R,
                           d_status, L.R, L.parts);
    VK_HIP(ctx, hipGetLastError());
    return VK_OK;
}

}  // extern "C"
