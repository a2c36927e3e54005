"""ctypes binding of include/vkimg.h (libvkimg_hip.so).  No CPU fallback: if the
HIP library is missing or a call fails, the caller gets an exception."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VKIMG_LIB") or os.path.join(HERE, "libvkimg_hip.so")  # (VKIMG_LIB: A/B timing of experimental builds)

VK_OK, VK_EINVAL, VK_EHIP, VK_ENOMAP, VK_EFORMAT, VK_ENOMEM, VK_ENOSPC = 0, 1, 2, 3, 4, 5, 6
VK_ST_BAD_START, VK_ST_BAD_PHASE = 1, 2
VK_EM_TOO_LARGE, VK_EM_BAD_RECORDS = 4, 8
VK_CL_ROLE_UNPAIRED, VK_CL_ROLE_R1, VK_CL_ROLE_R2 = 0, 1, 2
VK_CL_ADAPTER, VK_CL_MERGE, VK_CL_DEDUP = 1, 2, 4
VK_CL_BAD_FRAMING, VK_CL_RAGGED = 1, 2
VK_CL_NSTAT = 202
VK_CL_MAX_ADAPTER, VK_CL_DETECT_RECORDS = 64, 262144
VK_FA_NAME_BYTES, VK_FA_NO_SLOT = 128, 0xFFFFFFFF
VK_FA_NO_WINDOW = 0xFFFFFFFFFFFFFFFF
VK_BAM_BAD_RECORD, VK_BAM_TRUNCATED = 1, 2
VK_BAM_ALL, VK_BAM_READ1, VK_BAM_READ2, VK_BAM_SINGLE = 0, 1, 2, 3
VK_BAM_NO_GUESS = 1
VK_BAM_BAD_AUX, VK_BAM_UNGROUPED, VK_BAM_MAX_GROUPS = 3, 0xFFFFFFFF, 1024
VK_SCREEN_MAX_REF, VK_SCREEN_MIN_SLOTS, VK_SCREEN_MIN_K, VK_SCREEN_MAX_K = 1 << 30, 1024, 16, 31
VK_QC_BAD_FRAMING, VK_QC_CYCLES, VK_QC_NSTAT = 16, 1024, 11461
VK_QC_QUAL_HIST, VK_QC_READQ_HIST, VK_QC_LEN_HIST, VK_QC_CYCLE_BASE, VK_QC_CYCLE_QSUM = 8, 102, 196, 1221, 6341
VK_SPEC_NSTAT, VK_SPEC_HIST, VK_SPEC_TABLE_FULL = 261, 5, 32
VK_SKETCH_MIN, VK_SKETCH_MAX, VK_SKETCH_BLOCKS = 64, 1 << 20, 64
VK_TREE_MIN_LEAVES, VK_TREE_MAX_LEAVES, VK_TREE_MAX_TREES, VK_TREE_BAD_VALUE = 3, 16384, 4096, 1
VK_DEPTH_NSTAT, VK_DEPTH_HIST = 261, 5
VK_DIST_NO_GROUP, VK_DIST_NO_IDX, VK_DIST_NO_D2, VK_DIST_MAX_NEIGHBOURS = 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 64
VK_UNPNG_BAD_STREAM,VK_UNPNG_TRUNCATED, VK_UNPNG_BAD_SIZE, VK_UNPNG_BAD_ADLER, VK_UNPNG_BAD_FILTER = 1, 2, 4, 8, 16
VK_GZ_BAD_HEADER, VK_GZ_BAD_DATA, VK_GZ_TRUNCATED, VK_GZ_OVERFLOW, VK_GZ_BAD_SIZE, VK_GZ_BAD_CRC = 1, 2, 4, 8, 16, 32

# every symbol include/vkimg.h declares
SYMBOLS = ("vk_abi_version", "vk_strerror", "vk_last_hip_error", "vk_ctx_create", "vk_ctx_destroy",
           "vk_ctx_sync", "vk_set_mapping", "vk_count_device", "vk_image_device",
           "vk_fastq_to_image_device", "vk_count_host", "vk_image_host", "vk_synth_fastq_device", "vk_remap_host", "vk_preprocess_device",
           "vk_last_count_launch", "vk_count_sampled_device", "vk_inflate_device", "vk_upload_mapped", "vk_host_register", "vk_host_unregister",
           "vk_synth_shaped_lengths", "vk_synth_shaped_device", "vk_last_count_general", "vk_read_index_device", "vk_count_index_device",
           "vk_clean_lines_device", "vk_clean_workspace_size", "vk_clean_device", "vk_clean_detect_workspace_size",
           "vk_clean_detect_device", "vk_clean_adapters_device", "vk_clean_heads_device", "vk_ladder_emit_workspace_size",
           "vk_ladder_emit_device", "vk_train_batch_device", "vk_deflate_bound", "vk_deflate_workspace_size", "vk_deflate_device",
           "vk_count_fasta_device", "vk_count_fasta_host", "vk_count_fasta_sampled_device", "vk_fasta_records_count_device",
           "vk_fasta_records_device", "vk_count_fasta_records_device", "vk_count_fasta_windows_device", "vk_bam_frame_device",
           "vk_bam_fastq_device", "vk_last_bam_frame", "vk_png_bound", "vk_png_workspace_size", "vk_png_device",
           "vk_unpng_workspace_size", "vk_unpng_device", "vk_bam_groups_frame_device", "vk_bam_groups_fastq_device",
           "vk_bam_groups_workspace_size", "vk_last_bam_groups", "vk_screen_build_workspace_size", "vk_screen_build_device",
           "vk_screen_workspace_size", "vk_screen_device", "vk_qc_workspace_size", "vk_qc_device",
           "vk_spectrum_workspace_size", "vk_spectrum_device",
           "vk_spectrum_fasta_workspace_size", "vk_spectrum_fasta_device",
           "vk_sketch_workspace_size", "vk_sketch_device", "vk_sketch_pairs_device", "vk_sketch_pair_blocks_device",
           "vk_tree_workspace_size", "vk_tree_nj_device", "vk_tree_search_probe_device",
           "vk_depth_workspace_size", "vk_depth_device",
           "vk_dist_workspace_size", "vk_dist_device", "vk_last_count_pull")

_lib = None


class VkError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(msg)
        self.status = status


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VkError(VK_EHIP, f"HIP extension not built: {LIB_PATH} is missing "
                               "(run `python -m varkoder_amd.build`); there is no CPU fallback")
    # PyTorch carries its own HIP runtime (libamdhip64 under torch/lib): it must be the process's one before this library is
    # loaded, else the loader resolves the library's dependency to the system copy, PyTorch later brings its own, and a
    # context created here on a stream PyTorch made fails with a HIP runtime error (seen: `build()` then `smoke()` in one process).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, u32p, u64p, u8p = C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
    L.vk_abi_version.restype = C.c_int
    L.vk_strerror.restype = C.c_char_p
    L.vk_strerror.argtypes = [C.c_int]
    L.vk_last_hip_error.restype = C.c_char_p
    L.vk_last_hip_error.argtypes = [vp]
    L.vk_ctx_create.argtypes = [C.c_int, vp, C.c_int, C.POINTER(vp)]
    L.vk_ctx_destroy.restype = None
    L.vk_ctx_destroy.argtypes = [vp]
    L.vk_ctx_sync.argtypes = [vp]
    L.vk_set_mapping.argtypes = [vp, C.c_int, u32p, C.c_uint32]
    L.vk_count_device.argtypes = [vp, vp, u64p, u64p, C.c_uint32, C.c_int, C.c_uint32, vp, vp]
    L.vk_count_sampled_device.argtypes = [vp, vp, u64p, u64p, C.c_uint32, C.c_int, C.c_uint32, u64p, u64p, vp, vp, vp]
    L.vk_image_device.argtypes = [vp, vp, C.c_uint32, C.c_int, vp]
    L.vk_fastq_to_image_device.argtypes = [vp, vp, u64p, u64p, C.c_uint32, C.c_int, C.c_uint32, vp, vp, vp]
    L.vk_count_host.argtypes = [vp, vp, C.c_size_t, C.c_int, u32p, u32p]
    L.vk_image_host.argtypes = [vp, u32p, C.c_int, u8p]
    L.vk_synth_fastq_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int]
    L.vk_synth_shaped_lengths.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, u64p]
    L.vk_synth_shaped_device.argtypes = [vp, vp, u64p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64]
    L.vk_read_index_device.argtypes = [vp, vp, u64p, u64p, C.c_uint32, C.c_uint32, u64p, u32p]
    L.vk_count_index_device.argtypes = [vp, vp, u64p, u64p, C.c_uint32, C.c_int, C.c_uint32, vp, vp, u64p, u32p]
    L.vk_clean_lines_device.argtypes = [vp, vp, u64p, u64p, C.c_uint32, u64p]
    L.vk_clean_heads_device.argtypes = [vp, vp, u64p, u64p, C.c_uint32, C.c_uint32, u64p, u64p]
    L.vk_clean_workspace_size.argtypes = [u64p, u64p, C.c_uint32, C.c_uint32, u64p]
    L.vk_clean_device.argtypes = [vp, vp, u64p, u64p, u64p, u32p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                  C.c_uint32, vp, C.c_uint64, vp, u64p, C.c_uint64, vp, vp, vp]
    L.vk_clean_detect_workspace_size.argtypes = [u64p, u64p, C.c_uint32, C.c_uint32, u64p]
    L.vk_clean_detect_device.argtypes = [vp, vp, u64p, u64p, u64p, u32p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, vp,
                                         C.c_uint64, u32p, u8p]
    L.vk_clean_adapters_device.argtypes = [vp, vp, u64p, u64p, u64p, u32p, u32p, C.c_uint32, C.c_uint32, C.c_uint32,
                                           C.c_uint32, C.c_uint32, vp, C.c_uint64, vp, u64p, C.c_uint64, vp, vp, vp, u32p,
                                           u8p, vp]
    L.vk_ladder_emit_workspace_size.argtypes = [u64p, C.c_uint32, u64p, u32p, C.c_uint32, u64p]
    L.vk_ladder_emit_device.argtypes = [vp, vp, u64p, u64p, u64p, C.c_uint32, u32p, u64p, u64p, u8p, C.c_uint32, vp, C.c_uint64,
                                        u64p, u64p, u32p, vp, C.c_uint64]
    L.vk_deflate_bound.argtypes = [u64p, C.c_uint32, u64p]
    L.vk_deflate_workspace_size.argtypes = [u64p, C.c_uint32, u64p]
    L.vk_deflate_device.argtypes = [vp, vp, u64p, u64p, C.c_uint32, vp, C.c_uint64, vp, C.c_uint64, u64p, u64p]
    L.vk_png_bound.argtypes = [C.c_uint32, C.c_uint32, u64p]
    L.vk_png_workspace_size.argtypes = [C.c_uint32, C.c_uint32, u64p]
    L.vk_png_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, C.c_uint64, vp, C.c_uint64, u64p, u64p]
    L.vk_unpng_workspace_size.argtypes = [C.c_uint32, C.c_uint32, u64p]
    L.vk_unpng_device.argtypes = [vp, vp, u64p, u64p, C.c_uint32, C.c_uint32, vp, u32p, vp, C.c_uint64]
    L.vk_count_fasta_device.argtypes = [vp, vp, u64p, u64p, C.c_uint32, C.c_int, vp, vp, vp]
    L.vk_count_fasta_sampled_device.argtypes = [vp, vp, u64p, u64p, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, u32p, u64p, u64p, u64p,
                                                vp, vp, vp, vp]
    L.vk_count_fasta_host.argtypes = [vp, vp, C.c_size_t, C.c_int, u32p, u32p, u64p]
    L.vk_fasta_records_count_device.argtypes = [vp, vp, u64p, u64p, C.c_uint32, vp, vp]
    L.vk_fasta_records_device.argtypes = [vp, vp, u64p, u64p, C.c_uint32, u64p, vp, vp, vp]
    L.vk_count_fasta_records_device.argtypes = [vp, vp, u64p, u64p, C.c_uint32, C.c_int, u64p, vp, C.c_uint32, vp]
    L.vk_count_fasta_windows_device.argtypes = [vp, vp, u64p, u64p, C.c_uint32, C.c_int, u64p, vp, vp, C.c_uint32, C.c_uint32,
                                                C.c_uint64, C.c_uint32, C.c_uint32, vp]
    i32p = C.POINTER(C.c_int32)
    L.vk_bam_frame_device.argtypes = [vp, vp, u64p, u64p, u64p, i32p, C.c_uint32, u32p, u32p, C.c_uint32, C.c_uint32, C.c_uint32,
                                      u64p, u64p, u32p]
    L.vk_bam_fastq_device.argtypes = [vp, vp, u64p, u64p, u64p, i32p, C.c_uint32, u32p, u32p, C.c_uint32, C.c_uint32, C.c_uint32,
                                      vp, u64p, u64p, u64p, u32p]
    L.vk_last_bam_frame.argtypes = [vp, u64p, u64p]
    L.vk_bam_groups_frame_device.argtypes = [vp, vp, u64p, u64p, u64p, i32p, C.c_uint32, u32p, u32p, u8p, u32p, u32p, u32p, C.c_uint32,
                                             C.c_uint32, C.c_uint32, u64p, u64p, u32p]
    L.vk_bam_groups_fastq_device.argtypes = [vp, vp, u64p, u64p, u64p, i32p, C.c_uint32, u32p, u32p, u8p, u32p, u32p, u32p, C.c_uint32,
                                             C.c_uint32, C.c_uint32, vp, u64p, u64p, u64p, u32p]
    L.vk_bam_groups_workspace_size.argtypes = [u64p, C.c_uint32, u32p, u32p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, u64p]
    L.vk_last_bam_groups.argtypes = [vp, u64p, u64p]
    L.vk_screen_build_workspace_size.argtypes = [C.c_uint64, u64p]
    L.vk_screen_build_device.argtypes = [vp, vp, C.c_uint64, C.c_int, vp, C.c_uint64, vp, C.c_uint64, u64p, u64p, u32p]
    L.vk_screen_workspace_size.argtypes = [u64p, C.c_uint32, u64p, u64p]
    L.vk_screen_device.argtypes = [vp, vp, u64p, u64p, u64p, C.c_uint32, vp, C.c_uint64, C.c_int, C.c_uint32, C.c_int, vp, u64p,
                                   C.c_uint64, vp, vp, vp, vp, C.c_uint64]
    L.vk_qc_workspace_size.argtypes = [u64p, u64p, C.c_uint32, u64p]
    L.vk_qc_device.argtypes = [vp, vp, u64p, u64p, u64p, C.c_uint32, vp, vp, vp, C.c_uint64]
    L.vk_spectrum_workspace_size.argtypes = [u64p, C.c_uint32, u64p, u64p]
    L.vk_spectrum_device.argtypes = [vp, vp, u64p, u64p, u64p, C.c_uint32, C.c_int, C.c_uint32, vp, vp, u64p, u64p, vp, vp, vp,
                                     C.c_uint64]
    L.vk_spectrum_fasta_workspace_size.argtypes = [u64p, C.c_uint32, u64p]
    L.vk_spectrum_fasta_device.argtypes = [vp, vp, u64p, u64p, C.c_uint32, C.c_int, C.c_uint32, vp, vp, u64p, u64p, vp, vp, vp,
                                           C.c_uint64]
    L.vk_sketch_workspace_size.argtypes = [u64p, C.c_uint32, C.c_uint32, u64p]
    L.vk_sketch_device.argtypes = [vp, vp, vp, u64p, u64p, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint64]
    L.vk_sketch_pairs_device.argtypes = [vp, vp, vp, C.c_uint64, vp, vp, C.c_uint64, C.c_uint32, vp, vp]
    L.vk_sketch_pair_blocks_device.argtypes = [vp, vp, vp, C.c_uint64, vp, vp, C.c_uint64, C.c_uint32, vp, vp]
    L.vk_tree_workspace_size.argtypes = [C.c_uint32, C.c_uint32, u64p]
    L.vk_tree_nj_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.c_uint64]
    L.vk_tree_search_probe_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, C.c_uint64]
    L.vk_depth_workspace_size.argtypes = [u64p, C.c_uint32, u64p, u64p]
    L.vk_depth_device.argtypes = [vp, vp, u64p, u64p, u64p, C.c_uint32, C.c_int, C.c_uint32, vp, vp, u64p, u64p, vp, u32p, u32p, vp,
                                  u64p, C.c_uint64, vp, vp, vp, vp, C.c_uint64]
    L.vk_dist_workspace_size.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, u64p]
    L.vk_dist_device.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, C.c_uint64, vp, vp, C.c_uint32, vp, vp, vp, vp, C.c_uint64]
    L.vk_last_count_general.argtypes = [vp, u64p, u64p]
    L.vk_last_count_launch.argtypes = [vp, u32p, u32p, u32p]
    if hasattr(L, "vk_last_count_pull"):   # (tools/k1_ab.py also loads libraries built from older trees)
        L.vk_last_count_pull.argtypes = [vp, u32p, u32p, C.c_uint32]
    L.vk_preprocess_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, C.c_float, C.c_float, vp]
    L.vk_train_batch_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, C.c_float, C.c_float,
                                        C.c_uint32, u32p, u32p, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                        C.c_int, vp]
    L.vk_remap_host.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.c_int, vp]
    L.vk_inflate_device.argtypes = [vp, vp, u64p, u64p, C.c_uint32, vp, u64p, u64p, u64p, u32p]
    L.vk_upload_mapped.argtypes = [vp, vp, u64p, C.POINTER(vp), u64p, u8p, C.c_uint32, u32p]
    L.vk_host_register.argtypes = [vp, vp, C.c_uint64]
    L.vk_host_unregister.argtypes = [vp, vp]
    _lib = L
    return L


def check(ctx, status, what):
    if status == VK_OK:
        return
    L = lib()
    msg = L.vk_strerror(status).decode()
    if status == VK_EHIP and ctx:
        msg += ": " + L.vk_last_hip_error(ctx).decode()
    raise VkError(status, f"{what}: {msg}")
