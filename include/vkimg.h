/*
 * vkimg.h -- C ABI of libvkimg_hip.so: varKoder's `image` hot path on MI355X (gfx950).
 *
 * The reference (brunoasm/varKoder) has no FFI layer: the path sits behind two
 * Python functions that shell out to `dsk` / `dsk2ascii`.  Each
 * entry point below names the reference interface it replaces.  Plain pointers
 * and sizes only; status codes, never exceptions; caller-allocated buffers.
 *
 * Conventions
 *   - k in [5, 9]  (varKoder/commands/image.py:1209-1210).
 *   - k-mer code: bases A0 C1 G2 T3, code = sum_i b_i * 4^(k-1-i) (first base
 *     most significant), so codes sort like the k-mer strings.
 *   - hist[4^k] (u32): FORWARD-strand window counts.  The canonical class count
 *     dsk reports for {s, rc(s)} is hist[s] + hist[rc(s)] (hist[s] for a
 *     palindrome); vk_image_* performs that merge.
 *   - pix[4^k] (u32): image pixel index (row-major, row 0 on top) of every code,
 *     i.e. (side-1-y)*side + x of the reference's mapping table
 *     (core/utils.py:152-217, image.py:906-913).
 *   - "d_" pointers are device (HBM) addresses of the context's GPU; the others
 *     are host addresses.  FASTQ samples on the device must start at 16-byte
 *     aligned addresses and the buffer must be readable up to the 16-byte
 *     rounded end of the last sample.
 *   - All work is enqueued on the context's stream; *_host calls synchronise
 *     before returning, *_device calls do not.
 *   - A context owns device workspaces that grow on demand and is NOT re-entrant: use it
 *     from one thread at a time (one context per worker thread / process is the intended
 *     model: the reference runs one sample per pool worker, image.py:1281-1284).
 *   - k = 8, 9 count through a bucketed two-pass path whose workspace is about half the
 *     FASTQ bytes of the samples in flight (subsampled counts: about the FASTQ bytes); large
 *     batches are processed in sub-batches.
 */
#ifndef VKIMG_H
#define VKIMG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VK_OK 0
#define VK_EINVAL 1      /* bad argument (k, null pointer, alignment) */
#define VK_EHIP 2        /* a HIP runtime call failed; see vk_last_hip_error */
#define VK_ENOMAP 3      /* vk_set_mapping not called for this k */
#define VK_EFORMAT 4     /* FASTQ framing inconsistent (per-sample status word) */
#define VK_ENOMEM 5

/* per-file status bits of vk_inflate_device */
#define VK_GZ_BAD_HEADER 1u    /* not a gzip member (magic, method, reserved flags) */
#define VK_GZ_BAD_DATA 2u      /* invalid DEFLATE data (block type, code set, distance too far back) */
#define VK_GZ_TRUNCATED 4u     /* the stream ends before its last block / trailer */
#define VK_GZ_OVERFLOW 8u      /* the text does not fit out_caps[i]: call again with more room */
#define VK_GZ_BAD_SIZE 16u     /* a member's ISIZE differs from the bytes it inflated to */
#define VK_GZ_BAD_CRC 32u      /* single-member file: the trailer's CRC-32 is not the CRC-32 of the inflated text */

/* per-sample status bits written by the count stage */
#define VK_ST_BAD_START 1u     /* first record malformed: no leading '@', or third line not '+' */
#define VK_ST_BAD_PHASE 2u     /* line count mod 4 inconsistent between byte ranges / at EOF */

typedef struct vk_ctx vk_ctx;

int vk_abi_version(void);
const char* vk_strerror(int status);
/* hipGetErrorString of the last failing HIP call on this context ("" if none) */
const char* vk_last_hip_error(const vk_ctx* ctx);

/* Context: one per process per GPU.  own_stream != 0: the library creates its own
 * non-blocking stream (`stream` ignored); own_stream == 0: all work is enqueued on the
 * caller's hipStream_t `stream` (NULL = the device's default stream), so that it
 * orders with the caller's other work, e.g. a PyTorch stream. */
int vk_ctx_create(int device, void* stream, int own_stream, vk_ctx** out);
void vk_ctx_destroy(vk_ctx* ctx);
int vk_ctx_sync(vk_ctx* ctx);

/* Replaces get_kmer_mapping(k, method) (core/utils.py:152-171): installs the
 * code->pixel table for k.  pix == NULL selects the CGR closed form of
 * get_cgr (core/utils.py:174-217; npix must be 4^k); otherwise pix[4^k] is a
 * host table (varKode LUT) with every entry < npix. */
int vk_set_mapping(vk_ctx* ctx, int k, const uint32_t* pix, uint32_t npix);

/* Replaces count_kmers() = `dsk -kmer-size k -abundance-min 1 -file IN`
 * (commands/image.py:727-806, argv :771-790) for a batch of samples resident in
 * HBM.  Sample i is the FASTQ text d_fastq[offsets[i] .. offsets[i]+lengths[i]).
 * d_hist[nsamples][4^k] receives forward-strand counts, d_status[nsamples] the
 * VK_ST_* bits.  parts_per_sample = 0 lets the library choose how many
 * workgroups split one sample. */
int vk_count_device(vk_ctx* ctx, const void* d_fastq, const uint64_t* offsets,
                    const uint64_t* lengths, uint32_t nsamples, int k,
                    uint32_t parts_per_sample, uint32_t* d_hist, uint32_t* d_status);

/* vk_count_device restricted to a pseudo-random subset of each sample's reads: stands where the
 * reference runs `reformat.sh samplebasestarget=N sampleseed=S` once per output size before dsk
 * (split_fastq / run_parallel_reformats, commands/image.py:577-725).  Not bit-compatible with
 * BBTools' sampler (statistical equivalent, opt-in): read r of sample i is counted iff
 * hash32(seeds[i], offset of the newline ending r's header line) < thresholds[i], thresholds in
 * [0, 2^32] (2^32 = every read) -- a pure function of the file's bytes, independent of how the
 * library splits the sample.  seeds/thresholds are host arrays.  d_sites[nsamples][2] (device,
 * may be NULL) receives the bytes of all sequence lines (the reference's `nsites`, :669-675) and
 * of the sequence lines of the reads taken. */
int vk_count_sampled_device(vk_ctx* ctx, const void* d_fastq, const uint64_t* offsets,
                            const uint64_t* lengths, uint32_t nsamples, int k,
                            uint32_t parts_per_sample, const uint64_t* seeds,
                            const uint64_t* thresholds, uint32_t* d_hist, uint32_t* d_status,
                            uint64_t* d_sites);

/* The read index of a batch of samples resident in HBM: one streaming pass per sample that lists every read's
 * anchor (the newline that ends its header line) and adds up the bytes of all sequence lines -- `nsites`, which
 * split_fastq computes before it derives its ladder of subsample sizes (commands/image.py:663-675).  sites[i]
 * and status[i] (VK_ST_* bits) are HOST arrays; the call synchronises.  The context keeps the index until the
 * next call: vk_count_sampled_device calls whose samples (same d_fastq, same offsets and lengths, in any order
 * and any number of times) are all in it then WALK the reads each subsample takes instead of streaming the text
 * once per subsample (the reference runs reformat.sh + dsk once per subsample, :577-627, :682-695) -- same
 * counts, same sites.  A sample with more than one read per 32 bytes of text, or of 4 GiB and more, gets no index
 * (such calls stream as before).  VKIMG_NO_READ_INDEX=1 disables the walker. */
int vk_read_index_device(vk_ctx* ctx, const void* d_fastq, const uint64_t* offsets, const uint64_t* lengths,
                         uint32_t nsamples, uint32_t parts_per_sample, uint64_t* sites, uint32_t* status);

/* vk_count_device and vk_read_index_device in ONE pass over the text (k <= 7: the count kernel lists the anchors and
 * adds up the sites on its way; k = 8, 9: the two passes, one after the other): what a ladder whose first step takes
 * every read wants (split_fastq when the file holds less than --max-bp, commands/image.py:677-680).  d_hist /
 * d_status as vk_count_device; sites / status (host) as vk_read_index_device; the call synchronises. */
int vk_count_index_device(vk_ctx* ctx, const void* d_fastq, const uint64_t* offsets, const uint64_t* lengths,
                          uint32_t nsamples, int k, uint32_t parts_per_sample, uint32_t* d_hist, uint32_t* d_status,
                          uint64_t* sites, uint32_t* status);

/* Replaces make_image()'s arithmetic = `dsk2ascii` dump + join/groupby +
 * count+1 scatter + 256-quantile rank binning (commands/image.py:864-919) for a
 * batch of histograms.  d_img[nsamples][npix] receives the uint8 pixels. */
int vk_image_device(vk_ctx* ctx, const uint32_t* d_hist, uint32_t nsamples, int k,
                    uint8_t* d_img);

/* Both stages back to back (run_clean2img steps D+E, commands/image.py:1054-1127). */
int vk_fastq_to_image_device(vk_ctx* ctx, const void* d_fastq, const uint64_t* offsets,
                             const uint64_t* lengths, uint32_t nsamples, int k,
                             uint32_t parts_per_sample, uint32_t* d_hist,
                             uint32_t* d_status, uint8_t* d_img);

/* Replaces the gzip reader inside dsk (`-file IN.fq.gz`, commands/image.py:771-790; the files are
 * written by split_fastq, :696-708): inflates nfiles gzip files,
 * d_gz[gz_offsets[i] .. +gz_lengths[i]), into d_out[out_offsets[i] ..), at most out_caps[i] bytes each.
 * d_gz is memory the device can read: HBM, or pinned host memory (hipHostMalloc) -- the kernels then read the
 * compressed bytes over PCIe where they lie (twice: block-start finder and decoder) and no copy is needed
 * (single-member files: the little-endian u32 in the file's last four bytes is the text length).
 * Multi-member files are accepted; after a complete member, zero padding or bytes that are not a gzip
 * header end the data (as for zlib's gzread, which is how dsk reads a .gz).  out_lengths[i] (host)
 * receives the bytes written and status[i] (host) the VK_GZ_* bits; the call synchronises.  A file whose
 * text does not fit out_caps[i] gets VK_GZ_OVERFLOW and no text; where the whole file was decoded before the
 * slot was looked at (files of 512 KiB and more) out_lengths[i] then holds the size a second call needs
 * (> out_caps[i]), otherwise the bytes that fitted.
 * Integrity: structure and every member's ISIZE are checked, and every member's CRC-32 word is verified (on the
 * GPU) against the stretch of text the member inflated to (VK_GZ_BAD_CRC) -- as zlib's gzread, which dsk reads
 * through, does; only a file with more than 62 members inside one 128 KiB stretch of compressed bytes goes
 * unchecked. */
int vk_inflate_device(vk_ctx* ctx, const void* d_gz, const uint64_t* gz_offsets, const uint64_t* gz_lengths,
                      uint32_t nfiles, void* d_out, const uint64_t* out_offsets, const uint64_t* out_caps,
                      uint64_t* out_lengths, uint32_t* status);

/* Host-buffer conveniences (one sample): H2D copy, kernels, D2H copy, sync.
 * vk_count_host returns VK_EFORMAT when the sample's status word is non-zero
 * (hist is still written). */
int vk_count_host(vk_ctx* ctx, const uint8_t* fastq, size_t nbytes, int k, uint32_t* hist,
                  uint32_t* status);
int vk_image_host(vk_ctx* ctx, const uint32_t* hist, int k, uint8_t* img);

/* Synthetic FASTQ of BASELINE.md section 4, written straight into HBM: samples
 * sample0 .. sample0+nsamples-1, `reads` reads of `readlen` bases each, record =
 * "@sSSSSS.RRRRRRR\n" + bases + "\n+\n" + 'I'*readlen + "\n" (2*readlen+20 bytes;
 * 320 at readlen 150).  dist 0 = uniform ACGT, 1 = GC-skewed + homopolymer
 * reads; N injected at ~1e-3 per base.  Sample j starts at j*reads*(2*readlen+20).
 * varkoder_amd/synth.py is the bit-identical host generator. */
int vk_synth_fastq_device(vk_ctx* ctx, void* d_out, uint32_t sample0, uint32_t nsamples,
                          uint32_t reads, uint32_t readlen, uint64_t seed, int dist);

/* Synthetic FASTQ shaped like the files step B of the reference hands to step D: fastp runs with --merge
 * --include_unmerged and --disable_length_filtering (commands/image.py:405,426-427,494-495), so a cleaned file
 * holds reads of every length from 0 to about 2 x readlen under long headers.  Per read: 65 % readlen bases,
 * 20 % merged pairs (readlen+1 .. 2*readlen-10), 10 % trimmed (45 .. readlen-1), 5 % of 0 .. 44 bases (empty
 * reads included); header lines of 40 .. 70 bytes; quality characters '!' .. 'I' ('@' and '+' among them).
 * Samples differ in size: vk_synth_shaped_lengths fills lengths[nsamples] (host; synchronises), the caller lays
 * the samples out at 16-byte aligned offsets[] and vk_synth_shaped_device writes them (bytes up to each
 * sample's 16-byte rounded end are zeroed; synchronises).  64 <= readlen <= 1000.
 * varkoder_amd/synth.py (dist=2) is the bit-identical host generator. */
int vk_synth_shaped_lengths(vk_ctx* ctx, uint32_t sample0, uint32_t nsamples, uint32_t reads, uint32_t readlen,
                            uint64_t seed, uint64_t* lengths);
int vk_synth_shaped_device(vk_ctx* ctx, void* d_out, const uint64_t* offsets, uint32_t sample0, uint32_t nsamples,
                           uint32_t reads, uint32_t readlen, uint64_t seed);

/* Replaces remap() of `varKoder convert` (commands/convert.py:34-77) for a batch of host
 * images: out[p] = in[src0[p]] (src 0xFFFFFFFF = pixel without a k-mer -> 0); with sum_rc the
 * uint8-wrapping sum w0[p]*in[src0[p]] + w1[p]*in[src1[p]] followed by the reference's
 * (v - min) / max * 255 rescale in float64.  The source maps are built by
 * varkoder_amd/convert.py from the two k-mer mappings. */
int vk_remap_host(vk_ctx* ctx, const uint8_t* img_in, uint32_t nimg, uint32_t npix_in,
                  uint32_t npix_out, const uint32_t* src0, const uint32_t* src1,
                  const uint8_t* w0, const uint8_t* w1, int sum_rc, uint8_t* img_out);

/* Input side of `varKoder query` (commands/query.py:283-324 with the item transform of
 * commands/train.py:236-245): uint8 images d_img[nimg][side*side] (device) -> float32
 * d_out[nimg][3][out][out] = ((PIL BOX-resampled pixel)/255 - mean)/std, grey replicated to three
 * channels.  bounds[out][2] = (first source index, count) and coef[out][kmax] = PIL's 22-bit
 * fixed-point BOX coefficients of one axis (host tables, built by varkoder_amd/query.py). */
int vk_preprocess_device(vk_ctx* ctx, const uint8_t* d_img, uint32_t nimg, uint32_t side,
                         uint32_t out, const int32_t* bounds, const int32_t* coef, uint32_t kmax,
                         float mean, float stdv, float* d_out);

/* The training-time counterpart of vk_preprocess_device: one launch turns `batch` indices into a resident image
 * set d_img[nset][side*side] (device) into the model's input d_out[batch][3][out][out] (device, float32).
 * Row i: BOX-resample image idx[i] as vk_preprocess_device does (out == side: the tables must be the identity
 * and no intermediate is needed, so any side goes), /255, lighting where bshift[i] != 0 or cscale[i] != 1
 * (x = sigmoid((logit(clamp(x, 1e-7, 1 - 1e-7)) + bshift[i]) * cscale[i])), (x - mean) / std = s_i; then
 * mode 0: s_i;  mode 1 (MixUp): lam[i] * s_i + (1 - lam[i]) * s_partner[i];  mode 2 (CutMix): s_partner[i] for
 * x1 <= x < x2 and y1 <= y < y2, else s_i -- s_partner[i] being the same steps for row partner[i] (a position in
 * the batch) with that row's lighting.  A row with partner[i] == i, lam[i] == 1 (mode 1) or an empty rectangle
 * (mode 2) is s_i itself.  idx, partner, lam, bshift, cscale: host arrays of length batch.  VK_EINVAL, with nothing
 * launched, for idx[i] >= nset, partner[i] >= batch, lam[i] outside [0, 1], lighting parameters that are not finite,
 * a rectangle that is not 0 <= x1 <= x2 <= out (y alike), a mode other than 0, 1, 2, and what vk_preprocess_device
 * refuses.  The rule in full: INTEGRATION.md, "train". */
int vk_train_batch_device(vk_ctx* ctx, const uint8_t* d_img, uint32_t nset, uint32_t side, uint32_t out,
                          const int32_t* bounds, const int32_t* coef, uint32_t kmax, float mean, float stdv,
                          uint32_t batch, const uint32_t* idx, const uint32_t* partner, const float* lam,
                          const float* bshift, const float* cscale, uint32_t x1, uint32_t y1, uint32_t x2,
                          uint32_t y2, int mode, float* d_out);

/* Replaces: dsk opening and reading `-file <sample>.fq` (commands/image.py:771-796), for plain-text files: nfiles
 * host regions -- each a page-aligned, read-only MAP_SHARED mapping of a whole file -- are copied to
 * d_dst + dst_offsets[i] by DMA from the page-cache pages where they lie: no read() into a staging buffer (a copy
 * that costs a core per ~3 GB/s; ranks that share a host's cores cannot feed a 57 GB/s link with it).
 * registered (may be NULL): registered[i] != 0 says the caller has pinned region i with vk_host_register -- ahead of
 * time, on another thread -- and will release it; any other region is registered for the duration of its copy
 * (file i + 1 while file i is in flight) and released before the call returns.  The call synchronises.
 * status[i] (host): 0 copied, 1 the pages could not be registered (the caller copies that file through its own
 * buffer), 2 the copy failed.  Regions of 0 bytes are skipped. */
int vk_upload_mapped(vk_ctx* ctx, void* d_dst, const uint64_t* dst_offsets, const void* const* h_src,
                     const uint64_t* nbytes, const uint8_t* registered, uint32_t nfiles, uint32_t* status);

/* Pin / release a host region for vk_upload_mapped (hipHostRegister / hipHostUnregister: the pages stay where they
 * are, in the page cache).  Thread-safe; VK_EHIP if the platform refuses (the caller then leaves the flag 0). */
int vk_host_register(vk_ctx* ctx, const void* p, uint64_t nbytes);
int vk_host_unregister(vk_ctx* ctx, const void* p);

/* Step B: replaces clean_reads (commands/image.py:317-575: concatenate_reads, then fastp with --dedup,
 * --trim_front1/--trim_tail1, --trim_poly_g, --detect_adapter_for_pe, --merge --include_unmerged, no quality or
 * length filter) for a batch of samples whose raw FASTQ files are resident in HBM.  The rules are this project's
 * restatement of those options ("Step B", and tests/clean_ref.py), not fastp bit for bit.
 *
 * vk_clean_lines_device: lines[i] (host) = the '\n' bytes of file i, d_text[offsets[i] .. +lengths[i]) -- `wc -l`
 * of count_total_reads (:117-160), whose // 4 is the file's read count.  Synchronises.
 *
 * vk_clean_heads_device: replaces estimate_read_lengths (:90-115) reading each file's first sample_size records on
 * the host.  totals[i] and counted[i] (host) = the sum of the lengths and the number of the sequence lines that it
 * samples in file i: of the pieces between '\n' bytes (the last one ends with the file), pieces 1, 5, 9, ... up to
 * sample_size (>= 1) of them, each without the space, \t, \n, \v, \f and \r bytes at its ends.  The mean read length
 * is totals[i] / counted[i].  A file is read from its start only as far as its last sampled line.  Synchronises once.
 *
 * vk_clean_device: file i belongs to sample samples[i] as roles[i] (VK_CL_ROLE_*) and gives its first records[i]
 * records (the read budget of calculate_reads_needed, :164-221; the caller computes it).  A sample's R1 records,
 * in the order its R1 files are listed, pair up with its R2 records in the order of its R2 files.  flags:
 * VK_CL_* options.  d_ws: caller-allocated device workspace of vk_clean_workspace_size bytes (same lengths /
 * records).  Output: sample s's cleaned FASTQ text goes to d_out + out_offsets[s] (host array, 16-byte aligned;
 * the region must hold the sum of the sample's file lengths rounded up to 16, and d_out is out_bytes long), its
 * length to d_out_lengths[s] (the bytes up to the 16-byte rounded end are zeroed), its stats to
 * d_stats[s][VK_CL_NSTAT] (u64: output sequence bases, output records, then for cycles c = 0..39 of the first
 * group's output reads the counts of A C G T at [2 + 4c + 0..3] and the reads that reach c at [162 + c]) and its
 * VK_CL_* status bits to d_status[s] (a sample with a non-zero status gets no text).  No allocation, no
 * synchronisation: everything is enqueued on the context's stream. */
#define VK_CL_ROLE_UNPAIRED 0u
#define VK_CL_ROLE_R1 1u
#define VK_CL_ROLE_R2 2u
#define VK_CL_ADAPTER 1u       /* adapter trimming by pair overlap (not -a) */
#define VK_CL_MERGE 2u         /* merge overlapping pairs, keep the others (not -r) */
#define VK_CL_DEDUP 4u         /* drop exact duplicate reads / pairs (not -D) */
#define VK_CL_BAD_FRAMING 1u   /* a budgeted record lacks lines, its header is not '@', its third line not '+', or quality and sequence lengths differ */
#define VK_CL_RAGGED 2u        /* the sample's R1 files and R2 files give different numbers of records */
#define VK_CL_NSTAT 202
int vk_clean_lines_device(vk_ctx* ctx, const void* d_text, const uint64_t* offsets, const uint64_t* lengths,
                          uint32_t nfiles, uint64_t* lines);
int vk_clean_heads_device(vk_ctx* ctx, const void* d_text, const uint64_t* offsets, const uint64_t* lengths,
                          uint32_t nfiles, uint32_t sample_size, uint64_t* totals, uint64_t* counted);
int vk_clean_workspace_size(const uint64_t* lengths, const uint64_t* records, uint32_t nfiles, uint32_t nsamples,
                            uint64_t* bytes);
int vk_clean_device(vk_ctx* ctx, const void* d_text, const uint64_t* offsets, const uint64_t* lengths,
                    const uint64_t* records, const uint32_t* roles, const uint32_t* samples, uint32_t nfiles,
                    uint32_t nsamples, uint32_t trim_front, uint32_t trim_tail, uint32_t flags, void* d_ws,
                    uint64_t ws_bytes, uint8_t* d_out, const uint64_t* out_offsets, uint64_t out_bytes,
                    uint64_t* d_out_lengths, uint64_t* d_stats, uint32_t* d_status);

/* Step B's adapters by sequence ("Step B"; tests/adapter_ref.py).  A sample has three groups: its
 * R1 records, its R2 records and its single reads; group g of sample s is entry 3 s + g (0 R1, 1 R2, 2 unpaired) of
 * the adapter arrays, which hold a length (0: none) and VK_CL_MAX_ADAPTER bytes per group.
 *
 * vk_clean_detect_device: the same files, records, roles and samples as vk_clean_device, and -T's tail value.
 * Detects each group's adapter from its first VK_CL_DETECT_RECORDS budgeted records and writes it to the host arrays
 * adapter_lengths[3 nsamples] / adapter_seqs[3 nsamples][VK_CL_MAX_ADAPTER].  d_ws: device workspace of
 * vk_clean_detect_workspace_size bytes.  May grow a buffer of the context; synchronises.
 *
 * vk_clean_adapters_device: vk_clean_device, and with VK_CL_ADAPTER each read is also trimmed by its group's adapter
 * (host arrays as above, 0..VK_CL_MAX_ADAPTER bytes, compared as they are).  d_adapter_stats[s][2] (u64): reads and
 * bases of sample s cut by sequence.  May grow a buffer of the context; no synchronisation. */
#define VK_CL_MAX_ADAPTER 64
#define VK_CL_DETECT_RECORDS 262144
int vk_clean_detect_workspace_size(const uint64_t* lengths, const uint64_t* records, uint32_t nfiles, uint32_t nsamples,
                                   uint64_t* bytes);
int vk_clean_detect_device(vk_ctx* ctx, const void* d_text, const uint64_t* offsets, const uint64_t* lengths,
                           const uint64_t* records, const uint32_t* roles, const uint32_t* samples, uint32_t nfiles,
                           uint32_t nsamples, uint32_t trim_tail, void* d_ws, uint64_t ws_bytes, uint32_t* adapter_lengths,
                           uint8_t* adapter_seqs);
int vk_clean_adapters_device(vk_ctx* ctx, const void* d_text, const uint64_t* offsets, const uint64_t* lengths,
                             const uint64_t* records, const uint32_t* roles, const uint32_t* samples, uint32_t nfiles,
                             uint32_t nsamples, uint32_t trim_front, uint32_t trim_tail, uint32_t flags, void* d_ws,
                             uint64_t ws_bytes, uint8_t* d_out, const uint64_t* out_offsets, uint64_t out_bytes,
                             uint64_t* d_out_lengths, uint64_t* d_stats, uint32_t* d_status, const uint32_t* adapter_lengths,
                             const uint8_t* adapter_seqs, uint64_t* d_adapter_stats);

/* Step C's files: replaces run_parallel_reformats / run_reformat (commands/image.py:577-627: one `reformat.sh
 * samplebasestarget=N sampleseed=S breaklength=500 iupacToN=t` per subsample) for the steps of a batch of cleaned
 * samples resident in HBM.  The rule is this project's ("Step C", and tests/ladder_emit_ref.py), not
 * BBTools byte for byte: step j writes, in input order, the records of sample step_sample[j] that
 * vk_count_sampled_device counts with seed step_seed[j] and threshold step_threshold[j] (in [0, 2^32]) -- a read of
 * more than 500 bases as records of 500, named `<header>_<n>` -- or, with step_whole[j] != 0, every record uncut
 * (what vk_count_device counts).  A record is four lines ended by '\n' (a trailing '\r' dropped, the third line a
 * bare '+'); sequence bytes outside ACGTacgt are written as 'N'.  Counting a step's text gives the step's histogram.
 *
 * Samples as for vk_count_device: offsets[i] is a multiple of 16 (the newline passes load 16 bytes at a time from the
 * sample's start), any other offset returns VK_EINVAL before anything is read; the records inside a sample, its end and
 * the records of its files lie at any residue.  records[i] (host) = the lines of sample i over 4, a last line without '\n'
 * counted: (vk_clean_lines_device's lines[i] + 1) / 4.  d_ws: caller-allocated device workspace of
 * vk_ladder_emit_workspace_size bytes (same records and step_sample).  Host arrays out: out_lengths[nsteps] the bytes
 * of each step's file, out_offsets[nsteps] where it starts in d_out (a multiple of 16; the bytes up to its 16-byte
 * rounded end are zeroed) and status[nsamples]: VK_ST_* as vk_read_index_device reports them, VK_EM_TOO_LARGE for a
 * sample of 4 GiB or more, VK_EM_BAD_RECORDS when records[i] is not the sample's.  A sample with a non-zero status
 * gives its steps no text.  The files lie one after another and take the sum of their rounded lengths: when that is
 * more than out_capacity the call returns VK_ENOSPC with out_lengths and status filled and d_out untouched (d_out
 * NULL with out_capacity 0 asks for the sizes only).  The call synchronises. */
#define VK_ENOSPC 6            /* the output does not fit the caller's buffer */
#define VK_EM_TOO_LARGE 4u
#define VK_EM_BAD_RECORDS 8u
int vk_ladder_emit_workspace_size(const uint64_t* records, uint32_t nsamples, const uint64_t* lengths,
                                  const uint32_t* step_sample, uint32_t nsteps, uint64_t* bytes);
int vk_ladder_emit_device(vk_ctx* ctx, const void* d_fastq, const uint64_t* offsets, const uint64_t* lengths,
                          const uint64_t* records, uint32_t nsamples, const uint32_t* step_sample,
                          const uint64_t* step_seed, const uint64_t* step_threshold, const uint8_t* step_whole,
                          uint32_t nsteps, uint8_t* d_out, uint64_t out_capacity, uint64_t* out_offsets,
                          uint64_t* out_lengths, uint32_t* status, void* d_ws, uint64_t ws_bytes);

/* The .fq.gz files of the intermediates: replaces `pigz` behind clean_reads (commands/image.py:529-540) and
 * reformat.sh's own .fq.gz output in split_fastq (:696-708) for a batch of texts resident in HBM.  Text i is
 * d_text[offsets[i] .. +lengths[i]) (offsets[i] a multiple of 16, any other returns VK_EINVAL before anything is launched;
 * a length of 0 is a file).  Each becomes one BGZF file, the format BBTools writes through `bgzip`: gzip members of at
 * most 65,280 bytes of text, each with the 6-byte `BC` extra field (BSIZE = the member's size - 1), CRC-32 and ISIZE,
 * then bgzip's 28-byte empty member; an empty text is that member alone.  A member is one dynamic-Huffman DEFLATE block
 * over LZ77 tokens (matches of 3..258 bytes at distances up to 32,768, none reaching before the member), over the
 * literals alone when that is smaller, or a stored block when no code pays.  The same texts give the same bytes.
 * Any gzip reader reads the files (vk_inflate_device inflates their members in parallel); they are NOT the
 * single-member files pigz writes, and their bytes are not pinned between versions -- only the text they inflate to.
 *
 * vk_deflate_bound: *out_bound = the bytes d_out must hold: per file members * 31 + length + 28 rounded up to 16,
 * members = ceil(length / 65280).  Host arithmetic.  vk_deflate_workspace_size: the bytes of d_work (a 65,536-byte
 * slot per member, and tables).
 * vk_deflate_device: every argument is checked before anything is launched: VK_EINVAL for a null pointer, nfiles 0, an
 * unaligned offset or a workspace that is too small; VK_ENOSPC when out_capacity is below the bound (d_out untouched).
 * File i is written to d_out[out_offsets[i] .. +out_lengths[i]) (host arrays out; offsets multiples of 16, the files in
 * the order given, packed: the last one ends below the bound; the bytes up to a file's 16-byte rounded end are zeroed).
 * The number of launches does not depend on the files or their sizes.  The call synchronises. */
int vk_deflate_bound(const uint64_t* lengths, uint32_t nfiles, uint64_t* out_bound);
int vk_deflate_workspace_size(const uint64_t* lengths, uint32_t nfiles, uint64_t* out_bytes);
int vk_deflate_device(vk_ctx* ctx, const void* d_text, const uint64_t* offsets, const uint64_t* lengths, uint32_t nfiles,
                      uint8_t* d_out, uint64_t out_capacity, void* d_work, uint64_t work_bytes, uint64_t* out_offsets,
                      uint64_t* out_lengths);

/* The PNG files' image data: replaces PIL's zlib pass behind every image file (commands/image.py: `img.save(..., optimize=True)`)
 * for a batch of images resident in HBM, d_img[nimg][side][side] bytes (8-bit greyscale).  Image i becomes one complete
 * IDAT chunk: the data's length (big-endian), "IDAT", a zlib stream, the chunk's CRC-32.  The stream's text is the
 * image's rows with the filter byte 0 in front of each, side * (side + 1) bytes, cut into pieces of at most 65,280; each
 * piece is one DEFLATE block as vk_deflate_device makes them (LZ77 tokens, the literals alone when that is smaller, stored
 * when no code pays) with two additions: the byte one row up (side + 1 back) is a match candidate of every position, and
 * the block takes RFC 1951's fixed codes where they are smaller than a lengths table and its codes.  A piece that is not
 * the last is followed by an empty stored block where it does not end on a byte;
 * the header is 78 01, the trailer the Adler-32 of the text.  Pixels are what any PNG reader gives back; the bytes are
 * not PIL's and are not pinned between versions.  The same images give the same bytes.
 *
 * vk_png_bound: *out_bound = nimg * (16 + 2 + side * (side + 1) + 9 * pieces, rounded up to 16), pieces =
 * ceil(side * (side + 1) / 65280): the bytes d_out must hold.  Host arithmetic.  vk_png_workspace_size: the bytes of
 * d_work (per piece a slot of min(side * (side + 1), 65280) + 11 bytes rounded up to 16, and tables).
 * vk_png_device: every argument is checked before anything is launched: VK_EINVAL for a null pointer, nimg 0, side 0 or
 * above 512, or a workspace that is too small; VK_ENOSPC when out_capacity is below the bound (d_out untouched).  Chunk i
 * is written to d_out[out_offsets[i] .. +out_lengths[i]) (host arrays out; offsets multiples of 16, the chunks in image
 * order, packed: the last one ends below the bound; the bytes up to a chunk's 16-byte rounded end are zeroed).  The
 * number of launches does not depend on nimg.  The call synchronises. */
int vk_png_bound(uint32_t side, uint32_t nimg, uint64_t* out_bound);
int vk_png_workspace_size(uint32_t side, uint32_t nimg, uint64_t* out_bytes);
int vk_png_device(vk_ctx* ctx, const void* d_img, uint32_t nimg, uint32_t side, uint8_t* d_out, uint64_t out_capacity,
                  void* d_work, uint64_t work_bytes, uint64_t* out_offsets, uint64_t* out_lengths);

/* PNG files read back: replaces PIL's decode behind `Image.open` where a command starts from a folder of images
 * (commands/train.py and commands/query.py: `np.array(Image.open(p))`, one host thread) for 8-bit greyscale files of
 * side x side pixels.  Stream i is d_streams[offsets[i] .. +lengths[i]): the file's zlib stream (its IDAT payloads joined
 * in file order) from its 2-byte header to its Adler-32, and behind that four bytes more that the caller appends:
 * side * (side + 1), the bytes the stream must inflate to, as a little-endian u32.  offsets are multiples of 16; offsets and
 * lengths are host arrays.  The header's two bytes are the caller's to judge (CM 8, no dictionary) and are skipped here.
 * Image i is inflated by one wavefront (the decoder of vk_inflate_device) and un-filtered by one (filters 0 None, 1 Sub,
 * 2 Up, 3 Average, 4 Paeth of the PNG specification, per row) into d_img[i][side][side]; the stream's Adler-32 is
 * taken on the way and compared.  status[i] (a host array, out) is 0 or a sum of the bits below.  An image whose status
 * is not 0 has unspecified pixels inside its own side * side bytes; nothing outside them is written.
 *
 * vk_unpng_workspace_size: the bytes of d_work (per image a slot of side * (side + 1) bytes rounded up to 16, and tables).
 * vk_unpng_device: every argument is checked before anything is launched: VK_EINVAL for a null pointer, nimg 0, side 0 or
 * above 512, an offset that is not a multiple of 16, a length below 2 + 4 + 4, or a workspace that is too small (d_img
 * untouched).  The number of launches does not depend on nimg.  The call synchronises. */
#define VK_UNPNG_BAD_STREAM 1u   /* a block the decoder refuses */
#define VK_UNPNG_TRUNCATED  2u
#define VK_UNPNG_BAD_SIZE   4u   /* does not inflate to side * (side + 1) bytes */
#define VK_UNPNG_BAD_ADLER  8u
#define VK_UNPNG_BAD_FILTER 16u  /* a row's filter byte above 4 */
int vk_unpng_workspace_size(uint32_t side, uint32_t nimg, uint64_t* out_bytes);
int vk_unpng_device(vk_ctx* ctx, const void* d_streams, const uint64_t* offsets, const uint64_t* lengths, uint32_t nimg,
                    uint32_t side, uint8_t* d_img, uint32_t* status, void* d_work, uint64_t work_bytes);

/* Replaces: dsk on a FASTA input,`dsk -kmer-size k -abundance-min 1 -file IN.fa` (commands/image.py:771-796; the real dsk
 * reads FASTA as well as FASTQ), for a batch of samples resident in HBM, laid out as for vk_count_device (offsets multiples
 * of 16, readable up to the last sample's 16-byte rounded end).  The rule is this project's ("--from-fasta";
 * tests/fasta_ref.py): a line ends at '\n', a '\r' directly before it or as the sample's last byte belongs to the line end;
 * a line whose first byte is '>' is a header line and starts a record, none of its bytes are sequence; the other lines,
 * their ends removed, join into the record (empty lines vanish).  d_hist[nsamples][4^k] (u32, wrapping) = what
 * vk_count_device gives for the FASTQ text with one read per record: windows of ACGTacgt run across line ends, never
 * across records or any other byte.  d_status[nsamples]: VK_ST_BAD_START for a non-empty sample whose first byte is not
 * '>' (its histogram is not used); an empty sample has status 0 and a zero histogram.  d_bases[nsamples] (u64, device) =
 * the sequence bytes of the sample (joined bytes, every class).  A sample is cut by bytes, not records, so a record may be
 * of any length.  VKIMG_FASTA_UNIT_BYTES (tests) shrinks the bytes a workgroup owns.  No synchronisation. */
int vk_count_fasta_device(vk_ctx* ctx, const void* d_fasta, const uint64_t* offsets, const uint64_t* lengths,
                          uint32_t nsamples, int k, uint32_t* d_hist, uint32_t* d_status, uint64_t* d_bases);

/* Replaces: split_fastq + dsk on its files (commands/image.py:629-725, 771-796) for an ASSEMBLY -- the subsample ladder of
 * `image --from-fasta --fragments`: (sample, step) pairs of a batch of FASTA samples (laid out as for
 * vk_count_fasta_device), every pair counted over the fragments its step takes.  The rule is this project's
 * ("--from-fasta --fragments"; tests/fasta_ladder_ref.py): the joined bytes of a sample's records, in
 * order, have ordinals 0 .. bases - 1; the fragment of ordinal q is (q + shifts[i]) div frag_len; fragment f is taken iff
 * sample_hash(seeds[i], f) < thresholds[i] (thresholds in [0, 2^32]; 2^32 takes every fragment).  A window of k bytes
 * counts for pair i iff it counts in vk_count_fasta_device, its first and last byte lie in one fragment, and that one is
 * taken -- so even at 2^32 the windows across a fragment seam are dropped.  pair_sample[npairs] (host): the sample of each
 * pair, in any order, a sample any number of times.  d_hist[npairs][4^k] (u32); d_taken[npairs] (u64, device) = the
 * ordinals whose fragment is taken; d_status[nsamples], d_bases[nsamples] as vk_count_fasta_device's (a sample with
 * VK_ST_BAD_START: zero histograms, zero bases, nothing taken).  The call builds an index of the text (a u32 per 64
 * bytes, a u64 per unit) in the context's workspace; a lane none of whose fragments is taken reads its index word and
 * not its text.  VK_EINVAL, before anything is launched, for frag_len < k, frag_len >= 2^31, pair_sample[i] >= nsamples,
 * a threshold above 2^32 or a shift of 2^63 or more.  VKIMG_FASTA_UNIT_BYTES shrinks the units here as well.  No
 * synchronisation. */
int vk_count_fasta_sampled_device(vk_ctx* ctx, const void* d_fasta, const uint64_t* offsets, const uint64_t* lengths,
                                  uint32_t nsamples, int k, uint32_t frag_len, uint32_t npairs, const uint32_t* pair_sample,
                                  const uint64_t* seeds, const uint64_t* thresholds, const uint64_t* shifts, uint32_t* d_hist,
                                  uint32_t* d_status, uint64_t* d_bases, uint64_t* d_taken);

/* One host sample: H2D copy, vk_count_fasta_device, D2H copies, sync.  VK_EFORMAT when the status word is non-zero. */
int vk_count_fasta_host(vk_ctx* ctx, const uint8_t* fasta, size_t nbytes, int k, uint32_t* hist, uint32_t* status,
                        uint64_t* bases);

#define VK_FA_NAME_BYTES 128u        /* bytes kept of a record's name, zero-padded */
#define VK_FA_NO_SLOT 0xFFFFFFFFu    /* a record without a row: not counted */

/* Replaces: dsk on a FASTA input (commands/image.py:771-796), once per RECORD instead of once per file -- `image / query
 * --from-fasta --per-record`.  The rule is this project's ("--from-fasta --per-record";
 * tests/fasta_records_ref.py); lines, headers and bases are vk_count_fasta_device's.  A sample without VK_ST_BAD_START has
 * one record per header line, in order, those without sequence bytes included; a sample with it, or an empty one, has
 * none.  d_nrec[nsamples] (u32, device) = the records of each sample; d_status[nsamples] as vk_count_fasta_device's.  The
 * batch is laid out as for vk_count_fasta_device.  VKIMG_FASTA_UNIT_BYTES shrinks the units here as well.  No
 * synchronisation. */
int vk_fasta_records_count_device(vk_ctx* ctx, const void* d_fasta, const uint64_t* offsets, const uint64_t* lengths,
                                  uint32_t nsamples, uint32_t* d_nrec, uint32_t* d_status);

/* Replaces: the sequence names and lengths dsk's FASTA reader sees (commands/image.py:771-796) -- the record table of a
 * batch whose record counts the caller has read back: rec_first[nsamples + 1] (host) = prefix sums of d_nrec, total =
 * rec_first[nsamples].  Record g = rec_first[s] + r (r: its ordinal in sample s): d_rec_start[g] (u64) = the offset of its
 * '>' within the sample; d_rec_bases[g] (u64) = its joined bytes, every class (their sum over a sample is
 * vk_count_fasta_device's d_bases); d_rec_name[g][VK_FA_NAME_BYTES] = the bytes of its header line behind the '>' up to,
 * not including, the '\n' or the sample's end, at most VK_FA_NAME_BYTES of them, zero-padded (a trailing '\r' is kept).
 * All three are zeroed by the call; a record past rec_first's count is not written.  VK_EINVAL, before anything is
 * launched, for a null pointer or a rec_first that does not start at 0 or decreases.  No synchronisation. */
int vk_fasta_records_device(vk_ctx* ctx, const void* d_fasta, const uint64_t* offsets, const uint64_t* lengths,
                            uint32_t nsamples, const uint64_t* rec_first, uint64_t* d_rec_start, uint64_t* d_rec_bases,
                            uint8_t* d_rec_name);

/* Replaces: dsk on one FASTA file per record (commands/image.py:771-796).  d_slot[total] (u32, device): the row of every
 * record of the batch, or VK_FA_NO_SLOT; the slots are distinct, in [0, nslots), and increase with the record's position
 * in the batch.  d_hist[nslots][4^k] (u32, wrapping; zeroed by the call): the row of record g's slot = what
 * vk_count_fasta_device gives for a sample that holds this record alone; the rows of a sample's records sum to its
 * vk_count_fasta_device row.  A record without a slot is not counted and touches no row; a row no record names comes back
 * zero; a workgroup none of whose records has a slot does not read its text.  VK_EINVAL, before anything is launched,
 * for a null pointer, k outside 5..9, nslots == 0, or a rec_first that does not start at 0 or decreases.  No
 * synchronisation. */
int vk_count_fasta_records_device(vk_ctx* ctx, const void* d_fasta, const uint64_t* offsets, const uint64_t* lengths,
                                  uint32_t nsamples, int k, const uint64_t* rec_first, const uint32_t* d_slot, uint32_t nslots,
                                  uint32_t* d_hist);

#define VK_FA_NO_WINDOW 0xFFFFFFFFFFFFFFFFull   /* a record without rows: none of its windows is counted */

/* Replaces: dsk on one FASTA file per WINDOW of a record (commands/image.py:771-796, once per window) -- `image / query
 * --from-fasta --windows`.  The rule is this project's ("--from-fasta --windows";
 * tests/fasta_windows_ref.py); lines, headers, records and bases are vk_count_fasta_records_device's.  rec_first (host) and
 * d_rec_bases[total] (u64, device) are what vk_fasta_records_device takes and returns.  A window has win_len bytes and the
 * next one starts win_step behind it: win_step | win_len, m = win_len / win_step <= 64.  Window w of a record covers its
 * ordinals [w * win_step, w * win_step + win_len), exists iff it lies within the record, and holds the record's counted
 * k-mers whose FIRST byte lies in it (a k-mer may reach k - 1 bytes past the window's end, never past the record): what
 * vk_count_fasta_device gives for a record made of the window's bytes and the k - 1 behind them.  d_win_first[total]
 * (u64, device): the row of every record's window 0, or VK_FA_NO_WINDOW; window w has row d_win_first[g] + w; the rows of
 * different records are disjoint and increase with the record's position in the batch.  The call counts the rows of
 * [row_lo, row_lo + nrows) into d_hist[nrows][4^k] (u32, wrapping; zeroed by the call), row R at d_hist[R - row_lo];
 * every other window touches nothing, a row of the range no window names comes back zero, and a workgroup none of whose
 * bytes falls in a row of the range does not read its text.  m > 1: the call counts tiles of win_step bytes into
 * tile_rows rows of 4^k u32 in the context's workspace and sums m of them into each window; the caller states
 * tile_rows, at least the sum, over the records with a row in the range, of (their rows in the range + m - 1) (rows
 * whose tiles do not fit come back zero); m == 1: tile_rows is not used.  Ordinals, d_win_first and row numbers are
 * bounds-checked on the device.  VK_EINVAL, before anything is launched, for a null pointer, k outside 5..9, win_step < k,
 * win_len % win_step != 0, win_len / win_step > 64, win_len >= 2^31, nrows == 0, tile_rows == 0 with m > 1, or a rec_first
 * that does not start at 0 or decreases.  VKIMG_FASTA_UNIT_BYTES shrinks the units here as well.  No synchronisation. */
int vk_count_fasta_windows_device(vk_ctx* ctx, const void* d_fasta, const uint64_t* offsets, const uint64_t* lengths,
                                  uint32_t nsamples, int k, const uint64_t* rec_first, const uint64_t* d_rec_bases,
                                  const uint64_t* d_win_first, uint32_t win_len, uint32_t win_step, uint64_t row_lo,
                                  uint32_t nrows, uint32_t tile_rows, uint32_t* d_hist);

#define VK_BAM_BAD_RECORD 1u   /* a record's block_size is too small for its fields, its name is empty or not NUL-terminated */
#define VK_BAM_TRUNCATED 2u    /* a record runs past the file's end (or first_record lies behind it) */
#define VK_BAM_ALL 0u          /* a stream's `select`: every read of the file ... */
#define VK_BAM_READ1 1u        /* ... those with flag & 0xC1 == 0x41 (paired, first of the pair) ... */
#define VK_BAM_READ2 2u        /* ... with flag & 0xC1 == 0x81 (paired, second of the pair) ... */
#define VK_BAM_SINGLE 3u       /* ... every other read */
#define VK_BAM_NO_GUESS 1u     /* `flags`: no segment guesses its entry, the whole chain of records is walked in order */

/* Replaces: `samtools fastq` on the host before varKoder sees a read (varKoder has no BAM input; the rule is this
 * project's: INTEGRATION.md, "--from-bam: the rule"; tests/bam_ref.py) -- the framing of BAM files whose INFLATED bytes
 * lie in HBM (a .bam is BGZF: vk_inflate_device).  File i is d_bam + offsets[i], lengths[i] bytes (no alignment is asked:
 * every field is read by bytes); first_record[i] = the offset of its first record and n_ref[i] its reference count, as
 * the caller parsed them from the header (SAM spec 4.2: magic, l_text, text, n_ref, references).  A record (SAM spec
 * 4.2, "alignments") is a block_size word and block_size bytes; it is a read when l_seq > 0 and flag & exclude == 0
 * (flag: SAM spec 1.4.2), of l_read_name + 2 * l_seq + 5 bytes of FASTQ text.  Stream s takes the reads
 * stream_select[s] (VK_BAM_*) of file stream_file[s]; any number of streams may name a file.  out_records[nstreams],
 * out_bytes[nstreams] (host) = the reads and text bytes of every stream; status[nfiles] (host) = 0 or VK_BAM_BAD_RECORD /
 * VK_BAM_TRUNCATED, and the streams of such a file have neither reads nor bytes.  The files are cut into segments of
 * VKIMG_BAM_SEG_BYTES (read when the context is made; 64 to 65536, the default), every segment guesses where its first record starts and the
 * guesses are verified in order (vk_bam.h): the result does not depend on them, nor on VK_BAM_NO_GUESS in `flags`.
 * Nothing is read outside a file's bytes.  VK_EINVAL, before anything is launched, for a null pointer, a stream_file of
 * nfiles or more, a stream_select above VK_BAM_SINGLE or flags other than VK_BAM_NO_GUESS.  Synchronises. */
int vk_bam_frame_device(vk_ctx* ctx, const void* d_bam, const uint64_t* offsets, const uint64_t* lengths,
                        const uint64_t* first_record, const int32_t* n_ref, uint32_t nfiles, const uint32_t* stream_file,
                        const uint32_t* stream_select, uint32_t nstreams, uint32_t exclude, uint32_t flags,
                        uint64_t* out_records, uint64_t* out_bytes, uint32_t* status);

/* Replaces: `samtools fastq` (as above) -- the text.  The inputs are vk_bam_frame_device's; stream s is written to d_out +
 * out_offsets[s], at most out_caps[s] bytes (host arrays; the caller sizes them from out_bytes).  A read's text (SAM spec
 * 4.2 for the fields, 4.2.3 / 4.2.4 for bases and qualities): '@', read_name without its NUL, '\n', the bases ("=ACMGRSVTWYHKDBN",
 * '=' written as N), "\n+\n", min(q, 93) + 33 per quality -- 'I' for every base when the first quality byte is 0xFF --
 * and '\n'; with flag & 0x10 the bases are reverse-complemented (IUPAC codes included) and the qualities reversed.
 * out_lengths[nstreams], status[nfiles] (host) as the framing call's bytes and status.  Nothing is written outside a
 * stream's slot: a stream whose text does not fit gets none, out_lengths[s] = 0, and the call returns VK_ENOSPC once the
 * other streams are written.  Synchronises. */
int vk_bam_fastq_device(vk_ctx* ctx, const void* d_bam, const uint64_t* offsets, const uint64_t* lengths,
                        const uint64_t* first_record, const int32_t* n_ref, uint32_t nfiles, const uint32_t* stream_file,
                        const uint32_t* stream_select, uint32_t nstreams, uint32_t exclude, uint32_t flags, void* d_out,
                        const uint64_t* out_offsets, const uint64_t* out_caps, uint64_t* out_lengths, uint32_t* status);

/* Introspection (tests, tools/bam_time.py): of the last vk_bam_frame_device / vk_bam_fastq_device call, the segments its
 * files (SAM spec 4.2) were cut into and how many of them the link pass walked again because their guess was wrong or
 * missing. */
int vk_last_bam_frame(const vk_ctx* ctx, uint64_t* segments, uint64_t* rewalked);

#define VK_BAM_BAD_AUX 3u               /* an aux field in front of a read's RG field does not parse (the grouped calls only) */
#define VK_BAM_UNGROUPED 0xFFFFFFFFu    /* a stream's `group`: the reads that belong to no group of their file's table */
#define VK_BAM_MAX_GROUPS 1024u         /* groups of one file */

/* Replaces: `samtools split` (or `dorado demux`) and then `samtools fastq` on the host (the rule is this project's:
 * INTEGRATION.md, "--from-bam --bam-read-groups: the rule"; tests/bam_groups_ref.py) -- vk_bam_frame_device with the reads
 * of a file split by read group (SAM spec 1.3 for @RG, 4.2.4 for the aux fields).  The arguments of vk_bam_frame_device, and:
 * file i has the groups group_first[i] .. group_first[i + 1] (at most VK_BAM_MAX_GROUPS) of the call's table, group g's ID
 * is id_bytes[id_first[g] .. id_first[g + 1]) (1 to 255 bytes, no two equal within a file; all host arrays).  A read's
 * group is the one whose ID equals, byte for byte, the value of the FIRST aux field with tag RG when its type is Z; a read
 * whose first RG field has another type or a value that is no ID of the file (or runs to the block's end without NUL), or
 * that has no RG field, is ungrouped.  The fields are walked in order from the end of the qualities (types A c C s S i I
 * f Z H B, B's subtypes c C s S i I f); nothing behind the deciding field is looked at.  A field in front of it with
 * another type or subtype, whose value or NUL lies past the block's end, or fewer than 3 bytes left over, give the file
 * the status VK_BAM_BAD_AUX -- only when the framing is good (VK_BAM_BAD_RECORD and VK_BAM_TRUNCATED come first), and
 * only for reads: a record that is no read is not walked.  Stream s takes the reads stream_select[s] of group
 * stream_group[s] (an index into the file's groups, or VK_BAM_UNGROUPED) of file stream_file[s]; a read goes to at most
 * one stream, and reads that no stream takes are passed over.  VK_EINVAL, before anything is launched, for what
 * vk_bam_frame_device refuses, a stream_group at or past the file's count, a file of more than VK_BAM_MAX_GROUPS groups,
 * an ID of 0 or more than 255 bytes or twice in a file, a (file, select, group) named twice, and a file whose streams mix
 * VK_BAM_ALL with the class selects.  Nothing is read outside a file's bytes: every aux length is checked against the
 * block's end before it is followed.  Synchronises. */
int vk_bam_groups_frame_device(vk_ctx* ctx, const void* d_bam, const uint64_t* offsets, const uint64_t* lengths,
                               const uint64_t* first_record, const int32_t* n_ref, uint32_t nfiles,
                               const uint32_t* group_first, const uint32_t* id_first, const uint8_t* id_bytes,
                               const uint32_t* stream_file, const uint32_t* stream_select, const uint32_t* stream_group,
                               uint32_t nstreams, uint32_t exclude, uint32_t flags, uint64_t* out_records,
                               uint64_t* out_bytes, uint32_t* status);

/* Replaces: `samtools split` and `samtools fastq` (as above) -- the text, as vk_bam_fastq_device writes it and under its
 * slot rules: nothing is written outside a stream's slot, a stream whose text does not fit gets none (out_lengths[s] =
 * 0), and VK_ENOSPC is returned once the other streams are written.  Reads keep the file's order within a stream.  The
 * files are cut into PANELS of VKIMG_BAM_PANEL_SEGS segments (read when the context is made; 1 to 4096, 4 by default);
 * the emit pass runs one workgroup per panel, whatever the number of streams (vk_bam_groups.h).  Synchronises. */
int vk_bam_groups_fastq_device(vk_ctx* ctx, const void* d_bam, const uint64_t* offsets, const uint64_t* lengths,
                               const uint64_t* first_record, const int32_t* n_ref, uint32_t nfiles,
                               const uint32_t* group_first, const uint32_t* id_first, const uint8_t* id_bytes,
                               const uint32_t* stream_file, const uint32_t* stream_select, const uint32_t* stream_group,
                               uint32_t nstreams, uint32_t exclude, uint32_t flags, void* d_out,
                               const uint64_t* out_offsets, const uint64_t* out_caps, uint64_t* out_lengths,
                               uint32_t* status);

/* Host only: the bytes of workspace a grouped call takes beyond those of the ungrouped calls, for segments of seg_bytes
 * and panels of panel_segs segments (0: the defaults, 65536 and 4).  With S_i = max(1, ceil(lengths[i] / seg_bytes))
 * segments, P_i = ceil(S_i / panel_segs) panels, G_i groups and L_i streams of file i, and every piece rounded up to 256
 * bytes:
 *     the ID bytes + 4 (4 nfiles + 2 + sum G_i + 1 + sum T_i + 3 nstreams) + 2 sum 3 (G_i + 1)
 *     + 8 (2 nfiles + 1) + 16 nstreams          (tables; T_i = the power of two >= max(2, 2 G_i): the hash table)
 *     + 4 nfiles + 8                            (aux statuses, counters)
 *     + 2 (seg_bytes / 37 + 2) sum S_i          (a u16 note per record start)
 *     + 16 sum P_i L_i + 16 nstreams            (a row of two u64 per panel and stream; the totals)
 * A file of 1 GiB with 1024 groups x 3 classes: 16384 segments, 4096 panels, 3072 streams -- 58 MB of notes and 201 MB of
 * rows; with 96 groups, 6 MB of rows.  VK_EINVAL for a null pointer, a stream_file of nfiles or more, seg_bytes outside 64 .. 65536, panel_segs above
 * 4096. */
int vk_bam_groups_workspace_size(const uint64_t* lengths, uint32_t nfiles, const uint32_t* group_first,
                                 const uint32_t* id_first, const uint32_t* stream_file, uint32_t nstreams,
                                 uint32_t seg_bytes, uint32_t panel_segs, uint64_t* bytes);

/* Introspection (tests, tools/bam_time.py): of the last vk_bam_groups_frame_device / vk_bam_groups_fastq_device call,
 * the workgroups of its emit launch (0 for the framing call) and the records whose aux fields (SAM spec 4.2.4) were
 * walked. */
int vk_last_bam_groups(const vk_ctx* ctx, uint64_t* emit_workgroups, uint64_t* walked);

/* `image / query --exclude-fasta / --keep-fasta`: the k-mer set of a reference FASTA, built in HBM.  The rule is this
 * project's ("--exclude-fasta / --keep-fasta: the rule", and tests/screen_ref.py): lines, headers and
 * records as vk_count_fasta_device reads them; a base is ACGT of either case coded 0 1 2 3; every other sequence byte and
 * every record boundary breaks the sequence; every window of k (16 .. 31) unbroken bases gives a key, the smaller of the
 * window and its reverse complement read as 2k-bit integers, first base most significant; the set is the distinct keys.
 *
 * d_fasta[0 .. length) is the text (16-byte aligned, readable up to its 16-byte rounded end); a text of more than
 * VK_SCREEN_MAX_REF bytes -- it cannot hold more sequence bytes than that -- returns VK_EINVAL before anything is
 * touched.  d_table[nslots] is the caller's: open addressing over the keys, a free slot all ones (no key of 62 bits
 * equals it); nslots is a power of two of at least VK_SCREEN_MIN_SLOTS.  The call with d_table NULL and nslots 0 only
 * counts: *windows = the windows of k unbroken bases, from which a caller sizes the table (the engine takes the smallest
 * power of two that is at least twice the windows).  With a table the call fills it and returns *windows and *distinct,
 * the number of distinct keys; VK_ENOSPC when the keys do not leave one slot free (the table is then not to be used).
 * *status: VK_ST_BAD_START for a non-empty text whose first byte is not '>' (no windows, an empty table).  Where a key
 * lies in the table depends on a hash function that is the library's own; no result does.  d_ws: caller-allocated device
 * workspace of vk_screen_build_workspace_size(length) bytes.  VK_EINVAL for a null pointer, k outside 16 .. 31, a
 * misaligned text, a bad nslots or a workspace that is too small.  The call allocates no device memory and synchronises. */
#define VK_SCREEN_MAX_REF (1ull << 30)
#define VK_SCREEN_MIN_SLOTS 1024u
int vk_screen_build_workspace_size(uint64_t length, uint64_t* bytes);
int vk_screen_build_device(vk_ctx* ctx, const void* d_fasta, uint64_t length, int k, uint64_t* d_table, uint64_t nslots,
                           void* d_ws, uint64_t ws_bytes, uint64_t* windows, uint64_t* distinct, uint32_t* status);

/* The screen: cleaned FASTQ samples in HBM (what vk_clean_device wrote, or an upload) record by record against a table of
 * vk_screen_build_device.  A read's windows are taken from its sequence line as the set's are from the reference (a
 * trailing '\r' is no part of the line); its hits are the window POSITIONS whose key is in the table; it matches when
 * hits >= min_hits (>= 1); a read of fewer than k bases never matches.  keep == 0 keeps the records that do not match
 * (--exclude-fasta), keep != 0 those that do (--keep-fasta).  A kept record is copied byte for byte -- four lines as
 * they stand, a '\r' included, a last line without '\n' as it is -- and kept records stay in input order.
 *
 * Samples as for vk_ladder_emit_device: offsets[i] a multiple of 16 (any other returns VK_EINVAL before anything is
 * read), records[i] the lines of sample i over 4.  Sample i's text is written at d_out + out_offsets[i] (host array,
 * multiples of 16), zeroed up to its 16-byte rounded end; its region is as large as its input, lengths[i] rounded up to
 * 16, as vk_clean_device lays its output out, and must end within out_capacity (else VK_ENOSPC, nothing touched).  Device
 * arrays out: d_out_lengths[nsamples]; d_stats[nsamples][4] = records in, records kept, sequence bases in, sequence
 * bases kept; d_status[nsamples] = VK_ST_*, VK_EM_TOO_LARGE, VK_EM_BAD_RECORDS as vk_ladder_emit_device reports them: a
 * sample with a status gets no text and zero stats.  d_ws: caller-allocated device workspace of
 * vk_screen_workspace_size bytes (same records and lengths).  The call allocates no device memory and does not synchronise: it is
 * enqueued on the context's stream (its host arrays have been read when it returns). */
int vk_screen_workspace_size(const uint64_t* records, uint32_t nsamples, const uint64_t* lengths, uint64_t* bytes);
int vk_screen_device(vk_ctx* ctx, const void* d_fastq, const uint64_t* offsets, const uint64_t* lengths,
                     const uint64_t* records, uint32_t nsamples, const uint64_t* d_table, uint64_t nslots, int k,
                     uint32_t min_hits, int keep, uint8_t* d_out, const uint64_t* out_offsets, uint64_t out_capacity,
                     uint64_t* d_out_lengths, uint64_t* d_stats, uint32_t* d_status, void* d_ws, uint64_t ws_bytes);

/* `image / query --qc-report`: the quality profile of FASTQ streams in HBM -- what fastp's report states about the reads
 * before and after filtering (the reference copies `*_fastp_*.json` and `*.html` next to the cleaned reads,
 * commands/image.py:545-547, and users read them).  The rule is this project's ("--qc-report: the rule",
 * and tests/qc_ref.py).
 *
 * Stream i is d_text[offsets[i] .. + lengths[i]) (offsets[i] a multiple of 16, any other returns VK_EINVAL before anything
 * is read; readable up to its 16-byte rounded end; shorter than 4 GiB) and only its first records[i] records count: a read
 * budget, as vk_clean_device takes it.  A record is four lines as vk_ladder_emit_device frames them (a trailing '\r' no
 * part of a line, the last line with or without '\n').  With ls and lq the lengths of its sequence and quality lines:
 * a record with ls != lq adds 1 to records and to ragged_records and nothing else.  Every other record counts its bases by
 * class (A C G T of either case 0 1 2 3, every other byte 4) and its quality bytes b as q = min(max(b - 33, 0), 93), a byte
 * outside 33..126 also once in invalid_quality_bytes.
 *
 * d_rows[nstreams][VK_QC_NSTAT], u64 in this order:
 *     0 records   1 ragged_records   2 bases   3 gc_bases   4 other_bases   5 min_length   6 max_length
 *     7 invalid_quality_bytes        (min_length is 0 in a row without counted records)
 *     VK_QC_QUAL_HIST   94: bases of quality q (their sum is bases)
 *     VK_QC_READQ_HIST  94: reads of mean quality floor(sum q / ls), ls > 0
 *     VK_QC_LEN_HIST    1025: reads of length min(ls, 1024)
 *     VK_QC_CYCLE_BASE  [VK_QC_CYCLES][5]: bases of each class at cycle c < VK_QC_CYCLES
 *     VK_QC_CYCLE_QSUM  [VK_QC_CYCLES][5]: their qualities summed
 * d_status[nstreams]: VK_QC_BAD_FRAMING when a budgeted record's header does not start with '@' or its third line not
 * with '+'; VK_EM_BAD_RECORDS (alone) when the text holds fewer than 4 records[i] lines.  A stream with a status gets an
 * all-zero row and disturbs no other; a defect behind the budget is not seen.  Results are integers and do not depend on
 * the launch.  d_ws: caller-allocated device workspace of vk_qc_workspace_size bytes (same records and lengths).
 * VK_EINVAL for a null pointer, nstreams 0, an unaligned offset, a stream of 4 GiB or more, a workspace that is too small.
 * offsets, lengths and records are host arrays (read when the call returns).  The call allocates no device memory and
 * does not synchronise: it is enqueued on the context's stream. */
#define VK_QC_BAD_FRAMING 16u
#define VK_QC_CYCLES 1024u
#define VK_QC_QUAL_HIST 8u
#define VK_QC_READQ_HIST 102u
#define VK_QC_LEN_HIST 196u
#define VK_QC_CYCLE_BASE 1221u
#define VK_QC_CYCLE_QSUM 6341u
#define VK_QC_NSTAT 11461u
int vk_qc_workspace_size(const uint64_t* records, const uint64_t* lengths, uint32_t nstreams, uint64_t* bytes);
int vk_qc_device(vk_ctx* ctx, const void* d_text, const uint64_t* offsets, const uint64_t* lengths, const uint64_t* records,
                 uint32_t nstreams, uint64_t* d_rows, uint32_t* d_status, void* d_ws, uint64_t ws_bytes);

/* `image / query --kmer-spectrum`: the k-mer spectrum of cleaned FASTQ samples in HBM -- how many distinct canonical
 * k-mers occur once, twice, ... -- from which depth, genome size and error rate are estimated (varkoder_amd/spectrum.py).
 * The rule is this project's ("`--kmer-spectrum`: the rule", and tests/spectrum_ref.py); neither the
 * reference nor any other call here counts k-mers of this size.
 *
 * Samples as for vk_screen_device: sample i is d_text[offsets[i] .. + lengths[i]) (offsets[i] a multiple of 16, any other
 * returns VK_EINVAL before anything is read), records[i] its lines over 4.  A read's windows are taken from its sequence
 * line as the screen takes them (a base is ACGT of either case, a trailing '\r' is no part of the line, the quality line
 * is not looked at): every window of k (16 .. 31) unbroken bases gives a key, the smaller of the window and its reverse
 * complement as 2k-bit integers.  A key is taken when the high half of the library's 64-bit mix of it is a multiple of
 * `every` (>= 1; 1 takes every key and is exact): selection is by key, so every occurrence of a taken key counts and the
 * taken keys' spectrum is a 1/every sample of the whole.
 *
 * Tables: sample i owns slots slot_base[i] .. + nslots[i] of d_keys (u64) and d_counts (u32), both caller-allocated;
 * nslots[i] is a power of two of at least VK_SCREEN_MIN_SLOTS, the samples' ranges do not overlap, and the call
 * initialises them.  slot_base and nslots are host arrays.
 *
 * d_rows[nsamples][VK_SPEC_NSTAT], u64 in this order:
 *     0 reads   1 bases (sequence bytes, '\r' excluded)   2 windows   3 taken_windows   4 distinct (taken keys)
 *     VK_SPEC_HIST  256: hist[c - 1] = distinct taken keys of multiplicity c = 1 .. 255, hist[255] those of 256 and more
 * sum(hist) == distinct; the sum over c <= 255 of c hist[c - 1] <= taken_windows, equal when hist[255] == 0.
 * d_status[nsamples]: VK_ST_*, VK_EM_TOO_LARGE, VK_EM_BAD_RECORDS as vk_ladder_emit_device reports them, and
 * VK_SPEC_TABLE_FULL when a key of the sample found no slot (the probe ends after nslots[i] slots; it never spins).  A
 * sample with a status gets an all-zero row and disturbs no other.  Results are integers and do not depend on the launch.
 * d_ws: caller-allocated device workspace of vk_spectrum_workspace_size bytes (same records and lengths).  VK_EINVAL for a
 * null pointer, nsamples 0, k outside 16 .. 31, every 0, an nslots[i] that is no power of two or below 1,024, an
 * unaligned offset, a sample of more than 2^33 bytes (a multiplicity is 32-bit) or a workspace that is too small.  The
 * call allocates no device memory and does not synchronise: it is enqueued on the context's stream (its host arrays
 * have been read when it returns). */
#define VK_SPEC_NSTAT 261u
#define VK_SPEC_HIST 5u
#define VK_SPEC_TABLE_FULL 32u
int vk_spectrum_workspace_size(const uint64_t* records, uint32_t nsamples, const uint64_t* lengths, uint64_t* bytes);
int vk_spectrum_device(vk_ctx* ctx, const void* d_text, const uint64_t* offsets, const uint64_t* lengths,
                       const uint64_t* records, uint32_t nsamples, int k, uint32_t every, uint64_t* d_keys,
                       uint32_t* d_counts, const uint64_t* slot_base, const uint64_t* nslots, uint64_t* d_rows,
                       uint32_t* d_status, void* d_ws, uint64_t ws_bytes);

/* `image / query --from-fasta --genome-spectrum`: the k-mer spectrum of assemblies, counted straight from FASTA text in
 * HBM into tables of vk_spectrum_device's layout, so that vk_sketch_device takes them as they stand.  The rule is this
 * project's ("`--genome-spectrum`: the rule", and tests/fasta_spectrum_ref.py).
 *
 * The batch is laid out as for vk_count_fasta_device: sample i is d_fasta[offsets[i] .. + lengths[i]) (offsets[i] a
 * multiple of 16, the buffer readable up to each sample's 16-byte rounded end); lines, header lines and records are read
 * exactly as there.  Bases, windows and keys are the screen's (vk_screen_build_device): ACGT of either case, every window
 * of k (16 .. 31) unbroken bases -- across line ends, never across a header line or any other byte -- gives a key, the
 * smaller of the window and its reverse complement as 2k-bit integers.  A key is taken as in vk_spectrum_device, and every
 * occurrence of a taken key counts.  Tables (d_keys, d_counts, slot_base, nslots) as for vk_spectrum_device: the caller
 * allocates them, the call initialises them.
 *
 * d_rows[nsamples][VK_SPEC_NSTAT], u64, in vk_spectrum_device's layout:
 *     0 records (header lines)   1 bases (vk_count_fasta_device's d_bases: joined sequence bytes of every class)
 *     2 windows   3 taken_windows   4 distinct (taken keys)   VK_SPEC_HIST  256: hist[c - 1] as there
 * A multiplicity is a copy number here, not a depth.
 * d_status[nsamples]: VK_ST_BAD_START for a non-empty sample that does not begin with '>', VK_SPEC_TABLE_FULL when a key
 * of the sample found no slot (the probe ends after nslots[i] slots; it never spins).  A sample with a status gets an
 * all-zero row and disturbs no other; an empty sample has status 0 and a zero row.  Results are integers and do not depend
 * on the launch.
 * d_ws: caller-allocated device workspace of vk_spectrum_fasta_workspace_size bytes (same lengths).  VK_EINVAL, before
 * anything is launched, for a null pointer, nsamples 0, k outside 16 .. 31, every 0, an nslots[i] that is no power of two
 * or below 1,024, an unaligned offset, a sample of more than 2^33 bytes (a multiplicity is 32-bit) or a workspace that is
 * too small.  The call allocates no device memory and does not synchronise: it is enqueued on the context's stream (its
 * host arrays have been read when it returns).  VKIMG_FASTA_UNIT_BYTES shrinks the units as in the other FASTA calls. */
int vk_spectrum_fasta_workspace_size(const uint64_t* lengths, uint32_t nsamples, uint64_t* bytes);
int vk_spectrum_fasta_device(vk_ctx* ctx, const void* d_fasta, const uint64_t* offsets, const uint64_t* lengths,
                             uint32_t nsamples, int k, uint32_t every, uint64_t* d_keys, uint32_t* d_counts,
                             const uint64_t* slot_base, const uint64_t* nslots, uint64_t* d_rows, uint32_t* d_status,
                             void* d_ws, uint64_t ws_bytes);

/* `image / query --spectrum-sketch` and `distance`: a bottom-s MinHash sketch of each sample, taken from its spectrum
 * table while that lies in HBM, and every pair of sketches compared.  The rule is this project's (INTEGRATION.md,
 * "`--spectrum-sketch` and `distance`: the rule", and tests/sketch_ref.py); the reference has no such command.
 *
 * vk_sketch_device, after vk_spectrum_device and with its table arguments: sample i owns slots slot_base[i] .. +
 * nslots[i] of d_keys (u64, a free slot all ones) and d_counts (u32); slot_base and nslots are host arrays, d_status
 * u32[nsamples] is the spectrum's status array on the device.  (On tables made otherwise nslots[i] is any number from
 * 1 to 2^31.)  A held slot is eligible when its count is at least min_count (>= 1).  d_hashes[nsamples][s], u64: the
 * min(s, eligible) smallest values of the library's 64-bit mix (splitmix64's finaliser, a bijection) over the eligible
 * keys, ascending, the rest of the row all ones.  d_info[nsamples][2], u64: eligible and length = min(s, eligible).  A
 * sample with a status has eligible = length = 0 and disturbs no other.  The held keys of a table are distinct; if a
 * key lies in several eligible slots its hash counts once per slot.  Results are integers and do not depend on the
 * launch; the number of passes over a table does depend on its contents (two for spread hashes, at most seven) and is
 * bounded.  d_ws: caller-allocated device workspace of vk_sketch_workspace_size bytes (same nslots, nsamples and s).
 * VK_EINVAL for a null pointer, nsamples 0, min_count 0, s outside VK_SKETCH_MIN .. VK_SKETCH_MAX, an nslots[i] of 0 or
 * above 2^31, or a workspace that is too small.  The call allocates no device memory and does not synchronise: it is
 * enqueued on the context's stream (its host arrays have been read when it returns).
 *
 * vk_sketch_pairs_device: d_q u64[nq][s] with d_qlen u64[nq] (a length above s counts as s), d_r and d_rlen likewise
 * (d_q == d_r is allowed); every row strictly ascending in its first length entries, all made with the same s.  For
 * query i and reference j, with Sa and Sb their sketches: d_seen[i][j] = min(s, |Sa u Sb|) and d_shared[i][j] = the
 * number of values among the d_seen[i][j] smallest of Sa u Sb that lie in both, u32 each; empty against empty gives 0
 * and 0.  VK_EINVAL for a null pointer, s outside VK_SKETCH_MIN .. VK_SKETCH_MAX, nq or nr of 0 or above 2^20, or
 * nq * nr above 2^32.  Allocates nothing and does not synchronise.
 *
 * vk_sketch_pair_blocks_device: the same arguments and the same pair, its two counts split by BLOCK for `tree
 * --replicates` ("`tree`: the rule").  A value h belongs to block h & 63 (the values are outputs of the
 * mix, so their low bits are uniform).  d_seen[i][j][b] and d_shared[i][j][b], u32 [nq][nr][VK_SKETCH_BLOCKS]: among the
 * min(s, |Sa u Sb|) smallest values of Sa u Sb, those of block b, and those of block b that lie in both; over b they sum
 * to vk_sketch_pairs_device's d_seen[i][j] and d_shared[i][j].  VK_EINVAL as there, and for nq * nr above 2^26. */
#define VK_SKETCH_BLOCKS 64u
#define VK_SKETCH_MIN 64u
#define VK_SKETCH_MAX (1u << 20)
int vk_sketch_workspace_size(const uint64_t* nslots, uint32_t nsamples, uint32_t s, uint64_t* bytes);
int vk_sketch_device(vk_ctx* ctx, const uint64_t* d_keys, const uint32_t* d_counts, const uint64_t* slot_base,
                     const uint64_t* nslots, uint32_t nsamples, const uint32_t* d_status, uint32_t min_count, uint32_t s,
                     uint64_t* d_hashes, uint64_t* d_info, void* d_ws, uint64_t ws_bytes);
int vk_sketch_pairs_device(vk_ctx* ctx, const uint64_t* d_q, const uint64_t* d_qlen, uint64_t nq, const uint64_t* d_r,
                           const uint64_t* d_rlen, uint64_t nr, uint32_t s, uint32_t* d_shared, uint32_t* d_seen);
int vk_sketch_pair_blocks_device(vk_ctx* ctx, const uint64_t* d_q, const uint64_t* d_qlen, uint64_t nq, const uint64_t* d_r,
                                 const uint64_t* d_rlen, uint64_t nr, uint32_t s, uint32_t* d_shared, uint32_t* d_seen);

/* `image / query --kmer-spectrum --depth-filter`: cleaned reads kept by the depth of their own k-mers in their sample's
 * spectrum table, while that lies in HBM.  The rule is this project's ("`--depth-filter`: the rule", and
 * tests/depth_ref.py); neither the reference nor any other call here filters reads by depth.
 *
 * vk_depth_device, after vk_spectrum_device on the same text and with its arguments: samples, k and every as there;
 * sample i owns slots slot_base[i] .. + nslots[i] of d_keys and d_counts as that call left them (they are only read);
 * d_table_status u32[nsamples] is the spectrum's status array on the device.  A read's windows and keys are the
 * spectrum's; the depth of a taken window is the count in the slot that holds its key, 0 when none does (the probe stops
 * at a free slot or after nslots[i] slots; it never spins and never writes).  With n the taken windows of a record, its
 * depth m is 0 for n == 0 and else the lower median of their depths, the element at index (n - 1) / 2 of the sorted
 * depths.  The record is kept when lo[i] <= m <= hi[i] (host arrays, u32, both ends included; 2^32 - 1 is an open upper
 * end); the decision is exact for any bounds.  A kept record is copied byte for byte and kept records stay in input
 * order; the output is laid out as vk_screen_device lays it out (d_out, out_offsets, out_capacity, d_out_lengths as
 * there).
 *
 * d_rows[nsamples][VK_DEPTH_NSTAT], u64 in this order:
 *     0 records in   1 records kept   2 sequence bases in   3 sequence bases kept   4 records without a taken window
 *     VK_DEPTH_HIST  256: hist[min(m, 255)] over all records in, kept or not
 * d_status[nsamples]: VK_ST_*, VK_EM_TOO_LARGE, VK_EM_BAD_RECORDS as vk_ladder_emit_device reports them, joined with
 * d_table_status[i] (VK_SPEC_TABLE_FULL: a table that filled is no table).  A sample with a status gets no text and an
 * all-zero row and disturbs no other.  Results are integers and do not depend on the launch.  d_ws: caller-allocated
 * device workspace of vk_depth_workspace_size bytes (same records and lengths).  VK_EINVAL, before anything is read or
 * written, for a null pointer, nsamples 0, k outside 16 .. 31, every 0, an nslots[i] that is no power of two or below
 * 1,024, an unaligned offset or output offset, a sample of more than 2^33 bytes, lo[i] > hi[i], an output region that
 * does not end within out_capacity, or a workspace that is too small.  The call allocates no device memory and does not
 * synchronise: it is enqueued on the context's stream (its host arrays have been read when it returns). */
#define VK_DEPTH_NSTAT 261u
#define VK_DEPTH_HIST 5u
int vk_depth_workspace_size(const uint64_t* records, uint32_t nsamples, const uint64_t* lengths, uint64_t* bytes);
int vk_depth_device(vk_ctx* ctx, const void* d_text, const uint64_t* offsets, const uint64_t* lengths,
                    const uint64_t* records, uint32_t nsamples, int k, uint32_t every, const uint64_t* d_keys,
                    const uint32_t* d_counts, const uint64_t* slot_base, const uint64_t* nslots,
                    const uint32_t* d_table_status, const uint32_t* lo, const uint32_t* hi, uint8_t* d_out,
                    const uint64_t* out_offsets, uint64_t out_capacity, uint64_t* d_out_lengths, uint64_t* d_rows,
                    uint32_t* d_status, void* d_ws, uint64_t ws_bytes);

/* `compare`: exact squared Euclidean distances between images and the nearest neighbours of every query among the
 * references (the rule: INTEGRATION.md, "`compare`: the rule", and tests/dist_ref.py).  Neither the reference nor any
 * other call here compares images.
 *
 * d_q: u8 [nq][npix], d_r: u8 [nr][npix], pixels of any count (no side is assumed); d_q == d_r with nq == nr is allowed
 * (self mode: the rows are prepared once).  d2(i, j) = sum over p of (q[i][p] - r[j][p])^2, an exact integer.
 * d_qgroup u32[nq], d_rgroup u32[nr]: group ids, both or neither (null: no groups); reference j is eligible for query i
 * if d_qgroup[i] == VK_DIST_NO_GROUP or d_rgroup[j] != d_qgroup[i].  The neighbours of i are its n_neighbours eligible
 * references with the smallest (d2, j) -- d2 first, then the lower j -- written in that order to d_idx u32[nq][n] and
 * d_d2 u64[nq][n]; slots without an eligible reference hold VK_DIST_NO_IDX and VK_DIST_NO_D2.  d_matrix, if not null:
 * u64 [nq][nr], every d2 (eligibility does not apply).
 *
 * Limits: 1 <= n_neighbours <= VK_DIST_MAX_NEIGHBOURS, 1 <= npix <= VK_DIST_MAX_PIXELS, 1 <= nr <= VK_DIST_MAX_REFS,
 * 1 <= nq < 2^31, and 65025 npix + 1 < 2^(64 - b) with b the bits of nr - 1 (1 at least): a distance and an index share a
 * 64-bit key.  Up to 264,208 pixels (512 x 512 included) that holds for every nr; an input it refuses would not fit
 * the device's memory.  VK_EINVAL for anything else, a null pointer, one group array without the other, a workspace
 * smaller than vk_dist_workspace_size states (same nq, nr, npix; n_neighbours and want_matrix do not change it).
 * Results are integers and do not depend on the launch or on VKIMG_DIST_STRIP.  The call allocates no device memory and
 * does not synchronise: it is enqueued on the context's stream. */
#define VK_DIST_NO_GROUP 0xFFFFFFFFu
#define VK_DIST_NO_IDX 0xFFFFFFFFu
#define VK_DIST_NO_D2 0xFFFFFFFFFFFFFFFFull
#define VK_DIST_MAX_NEIGHBOURS 64u
#define VK_DIST_MAX_PIXELS (1u << 20)
#define VK_DIST_MAX_REFS (1u << 30)
int vk_dist_workspace_size(uint64_t nq, uint64_t nr, uint64_t npix, uint32_t n_neighbours, int want_matrix, uint64_t* bytes);
int vk_dist_device(vk_ctx* ctx, const void* d_q, uint64_t nq, const void* d_r, uint64_t nr, uint64_t npix, const uint32_t* d_qgroup,
                   const uint32_t* d_rgroup, uint32_t n_neighbours, uint32_t* d_idx, uint64_t* d_d2, uint64_t* d_matrix, void* d_ws,
                   uint64_t ws_bytes);

/* `tree`: neighbour joining of a batch of distance matrices, one record of joins and branch lengths per matrix.  There is
 * no reference interface: neither the reference nor any other call here builds a tree, and the rule is this project's
 * ("`tree`: the rule", and tests/tree_ref.py).
 *
 * d_dist: f64 [ntrees][n][n], 8-byte aligned; the call OVERWRITES it.  All arithmetic is IEEE double, one operation at a
 * time in the order written below, never a fused multiply-add, so a record does not depend on the launch.  A matrix is
 * valid when every entry is finite, >= 0 and <= 1e100, the diagonal is 0 and D[i][j] equals D[j][i] bit for bit; an
 * invalid matrix gets d_status[t] = VK_TREE_BAD_VALUE and an all-zero record and disturbs no other tree of the call.
 * Slots are 0 .. n - 1, all active at the start.  R[i] is the sum of D[i][k] over active k != i, taken as 256 partial
 * sums -- partial p adds the entries with k % 256 == p in rising k, starting from +0.0 -- folded by p[t] += p[t + s] for
 * s = 128, 64, .., 1.  A step with m > 3 active slots: over active i < j, Q = ((double)(m - 2) * D[i][j] - R[i]) - R[j];
 * the joined pair has the smallest Q, ties going to the smaller i, then the smaller j.  Li = 0.5 * D[i][j] + (R[i] - R[j])
 * / (2.0 * (double)(m - 2)) and Lj = D[i][j] - Li.  For every active k other than i and j, Du[k] = 0.5 * ((D[i][k] +
 * D[j][k]) - D[i][j]) and R[k] = ((R[k] - D[i][k]) - D[j][k]) + Du[k].  The new node takes slot i (Du becomes its row and
 * column, the diagonal stays 0), slot j goes inactive, and R[i] is taken afresh by the 256-partial rule.
 *
 * d_nodes u32 and d_lengths f64, [ntrees][2 (n - 3) + 3]: step t writes i and j at 2t and 2t + 1 of d_nodes and Li and Lj
 * at the same places of d_lengths; the last three active slots a < b < c close the record with La = 0.5 * ((D[a][b] +
 * D[a][c]) - D[b][c]), Lb = 0.5 * ((D[a][b] + D[b][c]) - D[a][c]), Lc = 0.5 * ((D[a][c] + D[b][c]) - D[a][b]).  Lengths are
 * recorded as computed, negative ones included.  n = 3 has no step: the record is the closing three.
 *
 * d_ws: caller-allocated device workspace of vk_tree_workspace_size bytes (same n and ntrees), 16-byte aligned.
 * VK_EINVAL for a null pointer, n outside VK_TREE_MIN_LEAVES .. VK_TREE_MAX_LEAVES, ntrees of 0 or above
 * VK_TREE_MAX_TREES, a misaligned d_dist or d_ws, or a workspace that is too small.  The call is 2 (n - 3) + 2 launches
 * enqueued on the context's stream; it allocates nothing, reads no device value on the host and does not synchronise. */
#define VK_TREE_MIN_LEAVES 3u
#define VK_TREE_MAX_LEAVES 16384u
#define VK_TREE_MAX_TREES 4096u
#define VK_TREE_BAD_VALUE 1u
int vk_tree_workspace_size(uint32_t n, uint32_t ntrees, uint64_t* bytes);
int vk_tree_nj_device(vk_ctx* ctx, double* d_dist /* [ntrees][n][n], overwritten */, uint32_t n, uint32_t ntrees,
                      uint32_t* d_nodes /* [ntrees][2(n-3)+3] */, double* d_lengths /* [ntrees][2(n-3)+3] */,
                      uint32_t* d_status /* [ntrees] */, void* d_ws, uint64_t ws_bytes);

/* Measurement (tools/tree_time.py): vk_tree_nj_device's first launch, which checks the matrices and sums their rows, and
 * then `launches` times the search launch of its first step (all n >= 4 slots active), nothing else; d_dist is only
 * read.  The time of a call with many launches less that of a call with few, over the difference, is the search alone.
 * Arguments and VK_EINVAL as there.  Does not synchronise. */
int vk_tree_search_probe_device(vk_ctx* ctx, const double* d_dist, uint32_t n, uint32_t ntrees, uint32_t launches,
                                uint32_t* d_status, void* d_ws, uint64_t ws_bytes);

/* Introspection used by bench.py / tests: workgroups and LDS bytes of the last
 * vk_count_device launch. */
int vk_last_count_launch(const vk_ctx* ctx, uint32_t* grid, uint32_t* block, uint32_t* lds_bytes);

/* Introspection (bench.py): of the last vk_count_device call with k <= 7, how many 4 KiB pieces of text left the
 * sequence-only fast path for the general one (reads under ~45 bases, non-ASCII bytes, low complexity, the first
 * and last piece of every wavefront's range), and about how many pieces there were.  Synchronises. */
int vk_last_count_general(vk_ctx* ctx, uint64_t* general_pieces, uint64_t* pieces);

/* Introspection (tests): the last vk_count_device call with k <= 7 ran as resident workgroups that own samples and pull
 * their byte ranges (the default; VKIMG_K1_STATIC=1 keeps one workgroup per sample and part).  *helpers: how many
 * workgroups may join a sample beside its owner; flushes[i], i < nsamples: how many workgroups added their histogram
 * to sample i's row, between 1 and 1 + *helpers (all 0, like *helpers: the call was no such launch).  Synchronises. */
int vk_last_count_pull(vk_ctx* ctx, uint32_t* helpers, uint32_t* flushes, uint32_t nsamples);

#ifdef __cplusplus
}
#endif
#endif /* VKIMG_H */
