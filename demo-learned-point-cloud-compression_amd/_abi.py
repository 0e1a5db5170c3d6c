"""ctypes binding of libpcc_hip.so (include/pcc.h).

This is the only place the package touches native code.  There is no CPU
fallback: if the shared library is missing or a GPU entry point fails, the
error propagates (RuntimeError / PccError) — a product path that silently ran
elsewhere would void every parity claim.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libpcc_hip.so")

PCC_OK = 0
PCC_E_ARG, PCC_E_HIP, PCC_E_RANGE, PCC_E_DUP, PCC_E_STREAM, PCC_E_NOMEM = -1, -2, -3, -4, -5, -6


class PccError(RuntimeError):
    def __init__(self, code, where, text):
        super().__init__(f"{where} failed ({code}): {text}")
        self.code = code


vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_float
pi64, pi32, pf32 = C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_float)

class PccBuf(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_uint8)), ("len", C.c_int64)]


class PccCloudInfo(C.Structure):
    _fields_ = [("n_points", C.c_int64), ("n_frames", C.c_int32), ("n_offsets", C.c_int32),
                ("h_offsets", C.POINTER(C.c_int64)), ("d_coords", C.c_void_p), ("d_colors", C.c_void_p),
                ("q_g", C.c_double), ("q_a", C.c_double)]


# what every attribute encode entry point begins with: ctx, values, value offsets, formats, row offsets, points, n_frames,
# perm, run starts, n_unique; _AEV with the blob version behind ctx
_AE = [vp, vp, pi64, pi32, pi64, pi64, i32, vp, vp, i64]
_AEV = _AE[:1] + [i32] + _AE[1:]

# name -> (restype, argtypes); every symbol declared in include/pcc.h
PROTOTYPES = {
    "pcc_codec_create": (vp, [vp, C.c_size_t, i32, vp]),
    "pcc_codec_destroy": (None, [vp]),
    "pcc_codec_ctx": (vp, [vp]),
    "pcc_codec_set_container_version": (i32, [vp, i32]),
    "pcc_codec_set_seek_points": (i32, [vp, i32]),
    "pcc_encode_gop": (i32, [vp, vp, vp, i64, i32, C.POINTER(C.c_double), i32, C.POINTER(PccBuf), pi64,
                             C.POINTER(C.c_double)]),
    "pcc_encode_gop_frames": (i32, [vp, C.POINTER(C.c_void_p), i32, C.POINTER(C.c_void_p), i32, pi64, i32,
                                    C.POINTER(C.c_double), i32, C.POINTER(PccBuf), pi64, C.POINTER(C.c_double)]),
    "pcc_encode_gop_host_frames": (i32, [vp, C.POINTER(C.c_void_p), i32, C.POINTER(C.c_void_p), i32, pi64, i32,
                                         C.POINTER(C.c_double), i32, C.POINTER(PccBuf), pi64, C.POINTER(C.c_double)]),
    "pcc_decode_gop": (i32, [vp, vp, i64, C.POINTER(PccCloudInfo), C.POINTER(C.c_double)]),
    "pcc_decode_fetch": (i32, [vp, vp, vp]),
    "pcc_decode_fetch_packed": (i32, [vp, vp, vp]),
    "pcc_container_points": (i32, [vp, i64, vp, vp]),
    "pcc_decode_gop_packed": (i32, [vp, vp, i64, vp, vp, i64, vp, vp]),
    "pcc_sparse_conv_head_up": (i32, [vp, vp, i64, vp, i64, vp, vp, i32, vp, vp, vp, vp]),
    "pcc_gaussian_quant_dev": (i32, [vp, vp, vp, i64, i32, vp, i32, vp, i32, vp, vp]),
    "pcc_rans_dev_create": (vp, [vp, i32, vp, vp, i32]),
    "pcc_rans_dev_destroy": (None, [vp]),
    "pcc_rans_dev_bound": (i64, [i64]),
    "pcc_rans_encode_dev": (i32, [vp, vp, vp, vp, i64, i64, i32, vp, i64, pi64]),
    "pcc_rans_stream_info": (i32, [vp, i64, pi64, pi64, pi64]),
    "pcc_rans_decode_dev": (i32, [vp, vp, vp, i64, i64, i64, i64, vp, i64, vp, vp]),
    "pcc_conv_prepare": (i32, [vp, vp, i32, i32, i32]),
    "pcc_conv_kernel_name": (C.c_char_p, [i32, i32, i32, i32]),
    "pcc_conv_forget": (i32, [vp, vp]),
    "pcc_level_counts": (i32, [vp, vp, i64, i32, i32, pi64, C.POINTER(C.c_int)]),
    "pcc_down_coords_known": (i32, [vp, vp, i64, i32, vp, vp, i64, vp, i64]),
    "pcc_exclusive_scan_u32": (i32, [vp, vp, vp, i64, vp]),
    "pcc_convT_gen_gather": (i32, [vp, vp, vp, i64, vp, vp, i32, vp]),
    "pcc_linear_gather": (i32, [vp, vp, vp, i64, vp, vp, i32, i32, vp]),
    "pcc_gather_map_columns": (i32, [vp, vp, i32, i64, vp, i64, vp, vp]),
    "pcc_subset_map_up": (i32, [vp, vp, i64, vp, vp, i64, vp]),
    "pcc_octree_encode": (i32, [vp, vp, i64, i32, vp, i64, pi64]),
    "pcc_octree_decode": (i32, [vp, i64, vp, i64, pi64]),
    "pcc_octree_encode_version": (i32, [vp, vp, i64, i32, i32, vp, i64, pi64]),
    "pcc_octree_blob_version": (i32, [vp, i64]),
    "pcc_octree_decode_ctx": (i32, [vp, vp, i64, vp, i64, pi64]),
    "pcc_octree_decode_dev": (i32, [vp, vp, i64, vp, i64, pi64, pi64]),
    "pcc_morton_keys_frames": (i32, [vp, vp, i32, i64, vp, i32, vp, vp]),
    "pcc_morton_keys_frames_f32": (i32, [vp, vp, i64, vp, i32, f32, pf32, i32, vp, vp]),
    "pcc_rows_index": (i32, [vp, vp, i64, i64, vp, i64, vp, vp, i32, vp]),
    "pcc_points_to_metric": (i32, [vp, vp, i64, i32, f32, pf32, vp]),
    "pcc_attr_encode_frames_kept": (i32, _AEV + [i64, vp, i32, vp, i64, pi64]),
    "pcc_octree_encode_frames": (i32, [vp, vp, i64, i32, i32, vp, i64, pi64]),
    "pcc_octree_decode_frames": (i32, [vp, C.POINTER(C.c_void_p), pi64, i32, vp, vp, i64, pi64]),
    "pcc_octree_decode_frames_lod": (i32, [vp, C.POINTER(C.c_void_p), pi64, i32, i32, vp, vp, i64, pi64]),
    "pcc_octree_encode_frames_inter": (i32, [vp, vp, i64, i32, i32, i32, i32, vp, i64, pi64]),
    "pcc_octree_decode_frames_ref": (i32, [vp, C.POINTER(C.c_void_p), pi64, i32, vp, i64, vp, vp, i64, pi64]),
    "pcc_octree_inter_info": (i32, [vp, i64, C.POINTER(C.c_int), pi64, C.POINTER(C.c_int), pi64]),
    "pcc_octree_encode_frames_inter_hist": (i32, [vp, vp, i64, i32, i32, i32, i32, i32, vp, i64, pi64]),
    "pcc_octree_decode_frames_refs": (i32, [vp, C.POINTER(C.c_void_p), pi64, i32, C.POINTER(C.c_void_p), pi64, i32, vp, vp, i64, pi64]),
    "pcc_octree_decode_frames_refs_lod": (i32, [vp, C.POINTER(C.c_void_p), pi64, i32, C.POINTER(C.c_void_p), pi64, i32, i32, vp, vp, i64,
                                                pi64]),
    "pcc_merge_keys": (i32, [vp, C.POINTER(C.c_void_p), pi64, i32, i32, vp, i64, pi64]),
    "pcc_octree_encode_frames_inter_best": (i32, [vp, vp, i64, i32, i32, i32, i32, i32, vp, i64, pi64]),
    "pcc_merge_keys_nested": (i32, [vp, C.POINTER(C.c_void_p), pi64, i32, i32, vp, i64, pi64]),
    "pcc_octree_lod_info": (i32, [vp, i64, i32, pi64, pi64]),
    "pcc_attr_encode_frames": (i32, _AE + [vp, i64, pi64]),
    "pcc_attr_decode_frames": (i32, [vp, C.POINTER(C.c_void_p), pi64, i32, pi64, vp, vp, i64, pi64, pi32]),
    "pcc_attr_lod_info": (i32, [vp, i64, i32, pi64, pi64]),
    "pcc_attr_encode_frames_v2": (i32, _AE + [vp, i32, vp, i64, pi64]),
    "pcc_attr_decode_frames_lod": (i32, [vp, C.POINTER(C.c_void_p), pi64, i32, i32, vp, pi64, vp, vp, i64, pi64, pi32]),
    "pcc_attr_encode_frames_nl": (i32, _AEV + [i64, vp, i32, i32, vp, i64, pi64]),
    "pcc_attr_info": (i32, [vp, i64, pi32, pi32, pi32, pi64, pi32, pi32, pi32]),
    "pcc_attr_encode_frames_cross": (i32, _AEV + [i64, vp, i32, i32, pi32, vp, i64, pi64]),
    "pcc_attr_cross_mask": (i32, [vp, i64, pi32]),
    "pcc_attr_encode_frames_nbr": (i32, _AE + [i64, vp, i32, pi32, vp, i64, pi64]),
    "pcc_attr_encode_frames_nbr_nl": (i32, _AE + [i64, vp, i32, i32, pi32, vp, i64, pi64]),
    "pcc_attr_encode_frames_transform": (i32, _AE + [i64, vp, i32, i32, vp, i64, pi64]),
    "pcc_attr_qstep": (i32, [vp, i64, pi32]),
    "pcc_attr_encode_frames_transform2": (i32, _AE + [i64, vp, i32, pi32, i32, vp, i64, pi64]),
    "pcc_attr_transform_info": (i32, [vp, i64, pi32, pi32]),
    "pcc_attr_encode_frames_transform3": (i32, _AE + [i64, vp, i32, pi32, i32, i32, vp, i64, pi64]),
    "pcc_attr_scalable_to": (i32, [vp, i64, pi32]),
    "pcc_attr_rate_ladder": (i32, [pi32, i32, i32, pi32, pi32]),
    "pcc_attr_encode_frames_rate": (i32, _AE + [i64, vp, i32, pi32, i32, i32, pi64, i64, vp, i64, pi64, pi32]),
    "pcc_nn_frames": (i32, [vp, vp, i64, vp, i64, i32, vp, vp, vp]),
    "pcc_nn_attr_sse_frames": (i32, [vp, vp, vp, i64, vp, vp, i64, i32, i32, i32, vp]),
    "pcc_nn_replay_host": (i32, [vp, i64, vp, i64, vp, vp, vp]),
    "pcc_knn_frames": (i32, [vp, vp, i64, i32, i32, vp, vp, vp, vp, pi32]),
    "pcc_nn_d2_frames": (i32, [vp, vp, vp, i64, vp, i64, vp, vp, i32, vp, vp]),
    "pcc_knn_replay_host": (i32, [vp, i64, i32, vp, vp, vp, vp, vp]),
    "pcc_outlier_scores_frames": (i32, [vp, vp, i64, i32, i32, vp, vp]),
    "pcc_outlier_mask_frames": (i32, [vp, vp, i64, i32, vp, vp, vp, vp]),
    "pcc_outlier_radius_frames": (i32, [vp, vp, i64, i32, i32, C.c_uint64, vp, vp]),
    "pcc_outlier_compact_rows": (i32, [vp, vp, i64, vp, i64, vp, i32, vp, vp, vp]),
    "pcc_gather_rows_pitched": (i32, [vp, vp, i64, i64, vp, i64, i32, vp]),
    "pcc_outlier_isqrt_host": (C.c_uint64, [C.c_uint64]),
    "pcc_outlier_replay_host": (i32, [vp, i64, i32, i32, i32, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "pcc_cluster_frames": (i32, [vp, vp, i64, i32, i32, C.c_uint64, i64, vp, vp, vp]),
    "pcc_cluster_replay_host": (i32, [vp, i64, i32, i32, C.c_uint64, i64, vp, vp, vp, vp, vp, vp]),
    "pcc_cluster_replay_host_reversed": (i32, [vp, i64, i32, i32, C.c_uint64, i64, vp, vp, vp, vp, vp, vp]),
    "pcc_attr_transfer_frames": (i32, [vp, vp, i64, vp, i64, vp, vp, vp, i64, i32, i32, i32, vp, vp]),
    "pcc_attr_stage_frames": (i32, [vp, vp, vp, vp, vp, i32, C.c_double, i32, i32, vp, vp, i64, vp]),
    "pcc_abi_version": (i32, []),
    "pcc_last_error": (C.c_char_p, []),
    "pcc_create": (vp, [i32, vp]),
    "pcc_destroy": (None, [vp]),
    "pcc_set_stream": (i32, [vp, vp]),
    "pcc_sync": (i32, [vp]),
    "pcc_timer_start": (i32, [vp]),
    "pcc_timer_stop": (i32, [vp]),
    "pcc_timer_elapsed_ms": (i32, [vp, pf32]),
    "pcc_prof_enable": (i32, [vp, i32]),
    "pcc_prof_only": (i32, [vp, C.c_char_p, i64]),
    "pcc_prof_count": (i32, [vp]),
    "pcc_prof_get": (i32, [vp, i32, C.c_char_p, i32, pf32, pi64]),
    "pcc_count_nonneg": (i32, [vp, vp, i64, pi64]),
    "pcc_morton_keys": (i32, [vp, vp, i64, vp, vp]),
    "pcc_keys_to_coords": (i32, [vp, vp, i64, vp]),
    "pcc_linear_keys": (i32, [vp, vp, i64, vp]),
    "pcc_sort_pairs": (i32, [vp, vp, vp, i64, i32]),
    "pcc_sort_coords": (i32, [vp, vp, i64, vp]),
    "pcc_gather_rows": (i32, [vp, vp, vp, i64, i32, vp]),
    "pcc_check_unique": (i32, [vp, vp, i64, pi32]),
    "pcc_batch_offsets": (i32, [vp, vp, i64, i32, pi64]),
    "pcc_down_coords": (i32, [vp, vp, i64, i32, vp, vp, i64, vp, pi64]),
    "pcc_derive_map_up": (i32, [vp, vp, i64, vp, vp, i64, vp]),
    "pcc_derive_map_down": (i32, [vp, vp, i64, vp, vp, vp, i64, i32, vp]),
    "pcc_inverse_rows": (i32, [vp, vp, i64, i64, vp]),
    "pcc_up_coords": (i32, [vp, vp, i64, i32, vp]),
    "pcc_up_coords_rows": (i32, [vp, vp, i64, i32, vp, i64, vp]),
    "pcc_build_map": (i32, [vp, vp, i64, i32, vp]),
    "pcc_lookup": (i32, [vp, vp, i64, vp, i64, vp]),
    "pcc_gather_rows_or_zero": (i32, [vp, vp, vp, i64, i32, vp]),
    "pcc_sparse_conv": (i32, [vp, vp, i64, vp, i32, i64, i64, vp, vp, i32, i32, i32, vp]),
    "pcc_sparse_conv_head": (i32, [vp, vp, i64, vp, i32, i64, i64, vp, vp, i32, i32, i32, vp, vp, vp, vp]),
    "pcc_convT_gen": (i32, [vp, vp, i64, vp, vp, i32, i32, i32, vp]),
    "pcc_linear": (i32, [vp, vp, i64, vp, vp, i32, i32, i32, vp]),
    "pcc_topk_prune": (i32, [vp, vp, i64, i32, pi64, pi64, vp, pi64]),
    "pcc_topk_prune_map": (i32, [vp, vp, i64, i32, pi64, pi64, vp, pi64, vp]),
    "pcc_factorized_quant": (i32, [vp, vp, i64, i32, vp, vp, vp]),
    "pcc_factorized_dequant": (i32, [vp, vp, i64, i32, vp, vp]),
    "pcc_gaussian_quant": (i32, [vp, vp, vp, i64, i32, vp, i32, vp, i32, vp, vp]),
    "pcc_gaussian_indexes": (i32, [vp, vp, i64, i32, vp, vp, i32, vp]),
    "pcc_build_indexes": (i32, [vp, vp, i64, vp, i32, vp]),
    "pcc_quantize_symbols": (i32, [vp, vp, vp, i64, vp]),
    "pcc_gaussian_quant16": (i32, [vp, vp, vp, i64, i32, vp, i32, vp, i32, vp, vp, vp]),
    "pcc_gaussian_indexes8": (i32, [vp, vp, i64, i32, vp, vp, i32, vp]),
    "pcc_rans_encode_multi16": (i32, [vp, vp, i64, i32, vp, i32, vp, vp, i32, vp, i64, pi64]),
    "pcc_rans_decode8": (i32, [vp, i64, vp, i64, vp, i32, vp, vp, i32, vp]),
    "pcc_rans_encode_seek": (i32, [vp, vp, i64, vp, i32, vp, vp, i32, vp, i64, pi64, vp, i32, vp, vp]),
    "pcc_rans_decode_range": (i32, [vp, i64, vp, i64, vp, i32, vp, vp, i32, vp, i64, i64, C.c_uint64, i64, vp, pi64]),
    "pcc_gaussian_dequant": (i32, [vp, vp, vp, i64, i32, vp, f32, f32, f32, vp]),
    "pcc_rans_encode": (i32, [vp, vp, i64, vp, i32, vp, vp, i32, vp, i64, pi64]),
    "pcc_rans_decode": (i32, [vp, i64, vp, i64, vp, i32, vp, vp, i32, vp]),
    "pcc_rans_encode_multi": (i32, [vp, vp, i64, i32, vp, i32, vp, vp, i32, vp, i64, pi64]),
    "pcc_octree_levels": (i32, [vp, vp, i64, i32, i32, vp, i64, pi64]),
    "pcc_octree_pack": (i32, [vp, pi64, i32, i64, pi32, vp, i64, pi64]),
    "pcc_octree_peek": (i32, [vp, i64, pi64, pi32, pi32]),
    "pcc_octree_unpack": (i32, [vp, i64, vp, i64]),
    "pcc_octree_unpack_levels": (i32, [vp, i64, vp, i64, pi64]),
    "pcc_vox_valid": (i32, [vp, vp, i64, f32, vp, pf32, pi64]),
    "pcc_vox_keys": (i32, [vp, vp, vp, i64, C.POINTER(C.c_double), C.c_double, vp, vp]),
    "pcc_vox_mean": (i32, [vp, vp, vp, vp, i64, C.c_double, vp, vp, i64, pi64]),
    "pcc_unique_rows": (i32, [vp, vp, i64, vp, pi64]),
}

def host_cpu_budget():
    """CPUs this process may actually use: min(visible cores, cgroup quota).  On the GPU boxes
    256 cores are visible but the cgroup grants 16; thread pools sized by os.cpu_count()
    (torch intra-op, OpenMP) then spin 256 threads, exhaust the quota and the whole process is
    throttled for tens of ms at a time."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as f:
                txt = f.read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]))))
            else:
                quota = int(txt[0])
                if quota > 0:
                    with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                        n = min(n, max(1, quota // int(f.read().split()[0])))
            break
        except (OSError, ValueError, IndexError):
            continue
    # one process per GPU (torch.distributed.run): the ranks of a node share its cores and, usually, one cgroup
    try:
        n //= max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1")))
    except ValueError:
        pass
    return max(1, n)


_lib = None


def lib():
    """Load libpcc_hip.so once; fail loudly if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C demo-learned-point-cloud-compression_amd/csrc`). There is no CPU fallback.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(handle, name)          # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if handle.pcc_abi_version() != 1:
            raise RuntimeError("libpcc_hip.so ABI version mismatch")
        _lib = handle
    return _lib


def check(code, where):
    if code != PCC_OK:
        raise PccError(code, where, lib().pcc_last_error().decode(errors="replace"))
