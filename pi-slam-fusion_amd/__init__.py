"""pi-slam-fusion_amd -- ctypes host binding of libpifusion.so.

Mirrors the reference's Map2D interface (Map2DFusion/Map2D.h:79-98:
create / prepare / feed / save / queueSize) and the MultiBandMap2DCPU::Ele tile
surface (MultiBandMap2DCPU.h:32-51).  The arithmetic lives in the HIP library;
this module only marshals pointers.  There is no CPU fallback: creating a map
without a HIP device (or without the built library) raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PF_LIB") or os.path.join(_HERE, "libpifusion.so")      # PF_LIB: another build of the same library (A/B runs)
ELE_PIXELS = 256

# Map2D::Map2DType (Map2D.h:83)
NoType, TypeCPU, TypeGPU, TypeMultiBandCPU, TypeRender = 0, 1, 2, 3, 4
PF_8UC3, PF_8UC4, PF_16SC3, PF_32FC3 = 16, 24, 19, 21
# raw frame formats (include/pifusion.h, DESIGN.md "Raw frames"); Bayer formats are named by the first two pixels of row 0
RAW_GREY, RAW_NV12, RAW_NV21, RAW_I420 = 1, 2, 3, 4
RAW_BAYER_RGGB, RAW_BAYER_BGGR, RAW_BAYER_GRBG, RAW_BAYER_GBRG = 8, 9, 10, 11


def host_array(shape, dtype=np.uint8):
    """numpy array over page-locked host memory (pf_host_alloc); freed with the array."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = lib().pf_host_alloc(n)
    if not p:
        raise MemoryError("pf_host_alloc(%d)" % n)
    buf = (C.c_uint8 * n).from_address(p)
    a = np.frombuffer(buf, dtype=dtype).reshape(shape)
    import weakref
    weakref.finalize(buf, lib().pf_host_free, p)
    return a


class Options(C.Structure):
    _fields_ = [("band_number", C.c_int), ("force_float", C.c_int), ("high_quality_show", C.c_int),
                ("weight_type", C.c_int), ("bg_color", C.c_int), ("resolution", C.c_double),
                ("scale", C.c_double), ("device", C.c_int), ("shard_rank", C.c_int),
                ("shard_count", C.c_int), ("shard_block", C.c_int), ("max_queue", C.c_int), ("fused", C.c_int),
                ("lookahead", C.c_int)]


class Image(C.Structure):
    _fields_ = [("rows", C.c_int), ("cols", C.c_int), ("type", C.c_int), ("data", C.c_void_p),
                ("step", C.c_size_t)]


class RawFrame(C.Structure):
    """pf_raw_frame: rows, cols of the image; up to three planes with their row steps (0 = packed)"""
    _fields_ = [("format", C.c_int), ("rows", C.c_int), ("cols", C.c_int), ("plane", C.c_void_p * 3), ("step", C.c_size_t * 3)]


class DistStats(C.Structure):
    _fields_ = [("bytes_sent", C.c_ulonglong), ("bytes_received", C.c_ulonglong), ("strips_sent", C.c_ulonglong),
                ("strips_received", C.c_ulonglong), ("tiles", C.c_ulonglong), ("peers", C.c_ulonglong),
                ("plan_ms", C.c_double), ("pack_ms", C.c_double), ("exchange_ms", C.c_double), ("compute_ms", C.c_double),
                ("verified", C.c_ulonglong)]


# pf_exchange_fn: all-to-all-v over host buffers (include/pifusion.h)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p),
                          C.POINTER(C.c_size_t), C.c_int)


class WebTile(C.Structure):
    """pf_webtile: one map tile on its way through a sink"""
    _fields_ = [("z", C.c_int), ("x", C.c_int), ("y", C.c_int), ("cover", C.c_int), ("jpeg", C.POINTER(C.c_uint8)), ("jpeg_len", C.c_size_t),
                ("mask8192", C.POINTER(C.c_uint8)), ("bgr", C.POINTER(C.c_uint8))]


WEBTILE_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(WebTile))


class ViewInfo(C.Structure):
    """pf_view_info: the plan of a view (include/pifusion.h)"""
    _fields_ = [("level", C.c_int), ("rect", C.c_int * 4), ("window", C.c_int * 4), ("M0", C.c_double * 9), ("Minv", C.c_double * 9),
                ("empty", C.c_int), ("tiles", C.c_int)]

    def as_dict(self):
        return {"level": self.level, "rect": tuple(self.rect), "window": tuple(self.window), "M0": np.array(self.M0).reshape(3, 3),
                "Minv": np.array(self.Minv).reshape(3, 3), "empty": bool(self.empty), "tiles": self.tiles}

_lib = None


def build(verbose=False):
    """Compile libpifusion.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc")]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libpifusion.so is not built (run __graft_entry__.build()); there is no CPU fallback")
    # PyTorch-ROCm wheels bundle their own libamdhip64 (same SONAME, different file name).
    # Loading torch first makes the dynamic linker hand that one runtime to this library
    # too; the other order ends with two HIP runtimes in the process and torch blind.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, ip, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)
    L.pf_default_options.argtypes = [C.POINTER(Options)]; L.pf_default_options.restype = None
    L.pf_options_set.argtypes = [C.POINTER(Options), C.c_char_p, C.c_char_p]
    L.pf_create.argtypes = [C.c_int, C.c_int, C.POINTER(Options)]; L.pf_create.restype = vp
    L.pf_destroy.argtypes = [vp]; L.pf_destroy.restype = None
    L.pf_last_error.restype = C.c_char_p
    L.pf_prepare.argtypes = [vp, dp, dp, C.c_int, C.POINTER(Image), dp]
    L.pf_feed.argtypes = [vp, C.POINTER(Image), dp]
    L.pf_feed_device.argtypes = [vp, C.POINTER(Image), dp]
    L.pf_queue_size.argtypes = [vp]; L.pf_queue_size.restype = C.c_uint
    L.pf_debug_read_last_frame.argtypes = [vp, vp, C.c_size_t]; L.pf_debug_read_last_frame.restype = C.c_long
    L.pf_sync.argtypes = [vp]
    L.pf_save.argtypes = [vp, C.c_char_p]
    L.pf_save_to_memory.argtypes = [vp, vp, ip, ip, ip, ip]
    L.pf_write_image.argtypes = [C.c_char_p, vp, C.c_int, C.c_int]
    L.pf_image_info.argtypes = [C.c_char_p, ip, ip]
    L.pf_read_image.argtypes = [C.c_char_p, vp, C.c_int, C.c_int]
    L.pf_jpeg_info.argtypes = [C.c_char_p, C.c_size_t, ip, ip, ip]
    L.pf_jpeg_decode_bgr.argtypes = [C.c_char_p, C.c_size_t, vp, C.c_int, C.c_int]
    L.pf_jpeg_decode_device.argtypes = [C.c_char_p, C.c_size_t, vp, C.c_int, C.c_int, vp]
    L.pf_feed_jpeg.argtypes = [vp, C.c_char_p, C.c_size_t, dp]
    if hasattr(L, "pf_jpeg_encode_bgr") or not os.environ.get("PF_LIB"):
        L.pf_jpeg_encode_bgr.argtypes = [vp, C.c_int, C.c_int, C.c_size_t, C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.pf_jpeg_encode_device.argtypes = [vp, C.c_int, C.c_int, C.c_size_t, C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t), vp]
        L.pf_blend_tiles_jpeg.argtypes = [vp, ip, C.c_int, C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    if hasattr(L, "pf_tiff_write_bgr") or not os.environ.get("PF_LIB"):
        L.pf_tiff_write_bgr.argtypes = [C.c_char_p, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, dp, C.c_int]
        L.pf_tiff_write_device.argtypes = [C.c_char_p, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, dp, C.c_int, vp]
        L.pf_save_tiff.argtypes = [vp, C.c_char_p, C.c_int, C.c_int]
    if hasattr(L, "pf_tiff_write_bgr_masked") or not os.environ.get("PF_LIB"):
        L.pf_tiff_write_bgr_masked.argtypes = [C.c_char_p, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int, dp, C.c_int]
        L.pf_tiff_write_device_masked.argtypes = [C.c_char_p, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int, dp, C.c_int, vp]
        L.pf_save_tiff_masked.argtypes = [vp, C.c_char_p, C.c_int, C.c_int]
        L.pf_save_to_memory_mask.argtypes = [vp, vp, vp, ip, ip, ip, ip]
    if hasattr(L, "pf_deflate_tile_bgr") or not os.environ.get("PF_LIB"):
        L.pf_deflate_tile_bgr.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.pf_deflate_tiles_device.argtypes = [vp, C.c_int, vp, C.c_size_t, vp, C.c_size_t, vp, vp]
        L.pf_deflate_code_lengths.argtypes = [vp, C.c_int, C.c_int, vp]
        L.pf_tiff_write_bgr_lossless.argtypes = [C.c_char_p, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_size_t, C.c_int, dp, C.c_int]
        L.pf_tiff_write_device_lossless.argtypes = [C.c_char_p, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_size_t, C.c_int, dp, C.c_int, vp]
        L.pf_save_tiff_lossless.argtypes = [vp, C.c_char_p, C.c_int, C.c_int]
        L.pf_debug_tiff_counts.argtypes = [vp, C.POINTER(C.c_longlong)]; L.pf_debug_tiff_counts.restype = None
    if hasattr(L, "pf_png_encode_bgr") or not os.environ.get("PF_LIB"):
        L.pf_png_encode_bgr.argtypes = [vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.pf_png_encode_device.argtypes = [vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t), vp]
        L.pf_png_crc32.argtypes = [C.c_uint32, vp, C.c_size_t]; L.pf_png_crc32.restype = C.c_uint32
        L.pf_png_crc32_combine.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64]; L.pf_png_crc32_combine.restype = C.c_uint32
        L.pf_png_adler32.argtypes = [vp, C.c_size_t]; L.pf_png_adler32.restype = C.c_uint32
        L.pf_png_adler32_combine.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64]; L.pf_png_adler32_combine.restype = C.c_uint32
        L.pf_save_png.argtypes = [vp, C.c_char_p, C.c_int]
    if hasattr(L, "pf_webtiles") or not os.environ.get("PF_LIB"):
        L.pf_webtiles_georef.argtypes = [vp, dp, dp, ip, ip]
        L.pf_webtiles_georef_compose.argtypes = [dp, dp, dp, dp]
        L.pf_webtiles_plan.argtypes = [dp, C.c_int, C.c_int, C.c_int, ip, dp, dp, dp, dp, C.c_longlong, C.c_longlong]
        L.pf_webtiles_native_zoom.argtypes = [dp, C.c_int, C.c_int]
        L.pf_webtiles_device.argtypes = [vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_size_t, dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, WEBTILE_SINK, vp, vp]
        L.pf_webtiles.argtypes = [vp, dp, C.c_int, C.c_int, C.c_int, C.c_int, WEBTILE_SINK, vp]
        L.pf_save_webtiles.argtypes = [vp, C.c_char_p, dp, C.c_int, C.c_int, C.c_int]
        L.pf_debug_webtiles_batch.argtypes = [C.c_int]
        L.pf_debug_webtiles_timing.argtypes = [C.c_int]; L.pf_debug_webtiles_timing.restype = None
        L.pf_debug_webtiles_timing_read.argtypes = [dp]; L.pf_debug_webtiles_timing_read.restype = None
    if hasattr(L, "pf_view_plan"):
        vi = C.POINTER(ViewInfo)
        L.pf_view_plan.argtypes = [dp, C.c_int, C.c_int, C.c_int, ip, dp, C.c_int, ip, vi]
        L.pf_render_view.argtypes = [vp, dp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, vi]
        L.pf_render_view_device.argtypes = [vp, dp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, vp, vi]
        L.pf_render_view_jpeg.argtypes = [vp, dp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t), vi]
        L.pf_view_of_extent.argtypes = [vp, C.c_int, C.c_int, dp]
        L.pf_view_from_pose.argtypes = [vp, dp, dp, dp]
        L.pf_view_from_lnglat.argtypes = [vp, dp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, dp]
        L.pf_debug_view_timing.argtypes = [vp, C.c_int]; L.pf_debug_view_timing.restype = None
        L.pf_debug_view_timing_read.argtypes = [vp, dp]; L.pf_debug_view_timing_read.restype = None
    L.pf_debug_jpeg_huffman.argtypes = [vp, C.POINTER(C.c_longlong)]; L.pf_debug_jpeg_huffman.restype = None
    L.pf_feed_jpeg_batch.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), dp, C.c_int, ip]
    L.pf_num_levels.argtypes = [vp]
    L.pf_pyramid_type.argtypes = [vp]
    L.pf_grid.argtypes = [vp, ip, dp]
    L.pf_tile_count.argtypes = [vp]
    L.pf_tile_coords.argtypes = [vp, ip, C.c_int]
    L.pf_get_tile_level.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp]
    L.pf_get_tile_bgra.argtypes = [vp, C.c_int, C.c_int, vp]
    L.pf_blend_tile_raw.argtypes = [vp, C.c_int, C.c_int, vp]
    L.pf_blend_tile.argtypes = [vp, C.c_int, C.c_int, vp]
    L.pf_blend_changed.argtypes = [vp, ip, vp, C.c_int]
    if hasattr(L, "pf_blend_tiles") or not os.environ.get("PF_LIB"):
        L.pf_blend_tiles.argtypes = [vp, ip, C.c_int, vp]
        L.pf_host_alloc.argtypes = [C.c_size_t]; L.pf_host_alloc.restype = vp
        L.pf_host_free.argtypes = [vp]; L.pf_host_free.restype = None
    if hasattr(L, "pf_blend_tiles_level") or not os.environ.get("PF_LIB"):
        L.pf_blend_tiles_level.argtypes = [vp, ip, C.c_int, C.c_int, vp, vp]
        L.pf_blend_changed_level.argtypes = [vp, C.c_int, ip, vp, C.c_int]
        L.pf_save_to_memory_level.argtypes = [vp, C.c_int, vp, ip, ip, ip, ip]
    L.pf_format_map_update.argtypes = [dp, dp, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_char_p, C.c_int]
    L.pf_map_update_command.argtypes = [vp, C.c_int, C.c_int, dp, C.c_char_p, C.c_int]
    L.pf_lnglat_from_distance.argtypes = [C.c_double, C.c_double, C.c_double, C.c_double, dp, dp]; L.pf_lnglat_from_distance.restype = None
    L.pf_normalize_using_weight_map.argtypes = [vp, vp, C.c_size_t]
    L.pf_mul_weight_map.argtypes = [vp, vp, C.c_size_t]
    L.pf_tile_owner.argtypes = [C.POINTER(Options), C.c_int, C.c_int]
    L.pf_halo_bytes.argtypes = [vp, C.c_int, C.c_int]; L.pf_halo_bytes.restype = C.c_size_t
    L.pf_halo_pack.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.pf_blend_tile_halo.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp), vp, vp]
    L.pf_tile_bytes.argtypes = [vp]; L.pf_tile_bytes.restype = C.c_size_t
    L.pf_tile_export.argtypes = [vp, C.c_int, C.c_int, vp]
    L.pf_tile_import.argtypes = [vp, C.c_int, C.c_int, vp]
    if hasattr(L, "pf_merge") or not os.environ.get("PF_LIB"):
        L.pf_merge.argtypes = [vp, vp]
        L.pf_merge_tiles.argtypes = [vp, C.c_int, ip, C.POINTER(vp), C.POINTER(C.c_float)]
        L.pf_tile_bounds.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_float)]
        L.pf_save_state.argtypes = [vp, C.c_char_p]
        L.pf_load_state.argtypes = [vp, C.c_char_p]
        L.pf_merge_state.argtypes = [vp, C.c_char_p]
        L.pf_state_info.argtypes = [C.c_char_p, ip, dp, dp, dp]
        L.pf_debug_merge_stats.argtypes = [vp, C.c_int, dp]; L.pf_debug_merge_stats.restype = None
    if hasattr(L, "pf_set_input_camera") or not os.environ.get("PF_LIB"):
        fp, llp = C.POINTER(C.c_float), C.POINTER(C.c_longlong)
        L.pf_undistort_table.argtypes = [dp, C.c_int, dp, fp, fp, llp]
        L.pf_undistort_fit_camera.argtypes = [dp, C.c_int, dp]
        L.pf_undistort_bgr.argtypes = [dp, C.c_int, dp, C.POINTER(Image), vp, C.c_size_t]
        L.pf_undistort_device.argtypes = [dp, C.c_int, dp, C.POINTER(Image), vp, C.c_size_t, vp]
        L.pf_set_input_camera.argtypes = [vp, dp, C.c_int]
        L.pf_input_camera_info.argtypes = [vp, ip, ip, llp]
    if hasattr(L, "pf_feed_raw") or not os.environ.get("PF_LIB"):
        rf = C.POINTER(RawFrame)
        L.pf_raw_to_bgr.argtypes = [rf, vp, C.c_size_t]
        L.pf_raw_to_bgr_device.argtypes = [rf, vp, C.c_size_t, vp]
        L.pf_feed_raw.argtypes = [vp, rf, dp]
        L.pf_feed_raw_device.argtypes = [vp, rf, dp]
    L.pf_dist_unique_id.argtypes = [vp]
    L.pf_dist_init_rccl.argtypes = [vp, vp, C.c_int, C.c_int]; L.pf_dist_init_rccl.restype = vp
    L.pf_dist_init_host.argtypes = [vp, C.c_int, C.c_int, EXCHANGE_FN, vp]; L.pf_dist_init_host.restype = vp
    L.pf_dist_destroy.argtypes = [vp]; L.pf_dist_destroy.restype = None
    L.pf_dist_blend_changed.argtypes = [vp, ip, vp, C.c_int]
    L.pf_dist_feed.argtypes = [vp, C.POINTER(Image), dp, C.c_int]
    L.pf_dist_feed_jpeg.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_int, dp, C.c_int]
    L.pf_dist_save.argtypes = [vp, C.c_char_p]
    if hasattr(L, "pf_dist_save_tiff_lossless") or not os.environ.get("PF_LIB"):
        L.pf_dist_save_tiff_lossless.argtypes = [vp, C.c_char_p, C.c_int, C.c_int]
    L.pf_dist_save_to_memory.argtypes = [vp, vp, ip, ip, ip, ip]
    L.pf_dist_last_stats.argtypes = [vp, C.POINTER(DistStats)]
    L.pf_dist_info.argtypes = [vp, ip, ip, C.POINTER(C.c_char_p)]
    L.pf_dist_set_verify.argtypes = [vp, C.c_int]
    L.pf_dist_plan_blend.argtypes = [C.c_int, C.c_int, ip, ip, C.POINTER(C.c_longlong), C.c_int, C.POINTER(C.c_size_t), vp, C.c_int, ip,
                                     vp, C.c_int, ip, ip, C.c_int, ip]
    if hasattr(L, "pf_debug_compact_launches") or not os.environ.get("PF_LIB"):
        L.pf_debug_compact_launches.argtypes = []; L.pf_debug_compact_launches.restype = C.c_longlong
    L.pf_profile_enable.argtypes = [vp, C.c_int]
    L.pf_profile_read.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), dp, C.POINTER(C.c_longlong), dp]
    # (PF_LIB may name an older build of the library for an A/B round, tools/ab.sh: it lacks this round's entry points)
    if hasattr(L, "pf_profile_read_run") or not os.environ.get("PF_LIB"):
        L.pf_profile_read_run.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), dp, C.POINTER(C.c_longlong), dp, dp]
    L.pf_profile_reset.argtypes = [vp]
    L.pf_stats.argtypes = [vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.pf_reserve_tiles.argtypes = [vp, C.c_longlong]
    L.pf_debug_culled_tiles.argtypes = [vp]; L.pf_debug_culled_tiles.restype = C.c_longlong
    L.pf_set_cull.argtypes = [vp, C.c_int]; L.pf_set_cull.restype = None
    if hasattr(L, "pf_debug_render_log") or not os.environ.get("PF_LIB"):
        L.pf_debug_render_log.argtypes = [vp, C.POINTER(C.c_longlong), C.c_int]
    L.pf_debug_culled_cells.argtypes = [vp]; L.pf_debug_culled_cells.restype = C.c_longlong
    if hasattr(L, "pf_debug_next_homography"):          # the experiments library alone has it (csrc/c_api.cpp)
        L.pf_debug_next_homography.argtypes = [vp, dp]; L.pf_debug_next_homography.restype = None
    if hasattr(L, "pf_debug_tile_store"):               # likewise
        L.pf_debug_tile_store.argtypes = [vp, C.c_int, C.c_int, C.c_int]; L.pf_debug_tile_store.restype = None
        L.pf_debug_fail_workspace.argtypes = [vp, C.c_int]; L.pf_debug_fail_workspace.restype = None
    if hasattr(L, "pf_stats_failed") or not os.environ.get("PF_LIB"):
        L.pf_stats_failed.argtypes = [vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.pf_debug_level0_exact_px.argtypes = [vp]; L.pf_debug_level0_exact_px.restype = C.c_double
    L.pf_render_stats.argtypes = [vp, dp]
    L.pf_timer_read.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_longlong), dp, dp, dp]
    L.pf_timer_reset.argtypes = [vp]
    _lib = L
    return L


POSE7 = C.c_double * 7


def _pose(p):
    if isinstance(p, POSE7):          # a caller that feeds thousands of poses a second converts them once (bench.py)
        return p, p
    a = np.ascontiguousarray(p, dtype=np.float64).reshape(-1)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def default_options(**kw):
    o = Options()
    lib().pf_default_options(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def se3_inverse(a):
    a, pa = _pose(a); o = np.zeros(7); lib().pf_se3_inverse(pa, o.ctypes.data_as(C.POINTER(C.c_double))); return o


def format_map_update(plane, gps_origin, min_x, min_y, ele_size, x, y):
    """pf_format_map_update: the reference's Map2DUpdate text for dense tile index (x, y) (C implementation)."""
    _, pp = _pose(plane)
    buf = C.create_string_buffer(256)
    g = (C.c_double * 3)(*[float(v) for v in gps_origin])
    n = lib().pf_format_map_update(pp, g, float(min_x), float(min_y), float(ele_size), int(x), int(y), buf, 256)
    return buf.value.decode() if n > 0 else None


def lnglat_from_distance(lng1, lat1, dx, dy):
    a, b = C.c_double(), C.c_double()
    lib().pf_lnglat_from_distance(float(lng1), float(lat1), float(dx), float(dy), C.byref(a), C.byref(b))
    return a.value, b.value


def se3_mul(a, b):
    a, pa = _pose(a); b, pb = _pose(b); o = np.zeros(7)
    lib().pf_se3_mul(pa, pb, o.ctypes.data_as(C.POINTER(C.c_double))); return o


def so3_rotate(q, p):
    q, pq = _pose(q); p, pp = _pose(p); o = np.zeros(3)
    lib().pf_so3_rotate(pq, pp, o.ctypes.data_as(C.POINTER(C.c_double))); return o


def footprint(cam, pose_plane):
    c, pc = _pose(cam); p, pp = _pose(pose_plane); o = np.zeros(8)
    ok = lib().pf_footprint(pc, pp, o.ctypes.data_as(C.POINTER(C.c_double)))
    return o.reshape(4, 2) if ok else None


def perspective_transform(src, dst):
    s = np.ascontiguousarray(src, dtype=np.float32).reshape(8); d = np.ascontiguousarray(dst, dtype=np.float32).reshape(8)
    M = np.zeros(9)
    lib().pf_perspective_transform(s.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), M.ctypes.data_as(C.c_void_p))
    return M.reshape(3, 3)


def write_image(filename, bgr):
    """cv::imwrite leg of save() (MultiBandMap2DCPU.cpp:841): HxWx3 BGR uint8 -> .png / .jpg, .jpeg (quality 95, 4:2:0) / .ppm"""
    a = np.ascontiguousarray(bgr, dtype=np.uint8)
    return bool(lib().pf_write_image(filename.encode(), a.ctypes.data, a.shape[0], a.shape[1]))


def read_image(filename):
    """cv::imread(filename) of the file driver (backup/map2dfusion.cpp:129-132): JPEG or binary PPM -> HxWx3 BGR uint8.
    Raises on a file the library cannot read (there is no other decoder behind it)."""
    L = lib(); r = C.c_int(); c = C.c_int()
    if not L.pf_image_info(filename.encode(), C.byref(r), C.byref(c)):
        raise RuntimeError("read_image: %s" % L.pf_last_error().decode())
    out = np.empty((r.value, c.value, 3), np.uint8)
    if not L.pf_read_image(filename.encode(), out.ctypes.data, r.value, c.value):
        raise RuntimeError("read_image: %s" % L.pf_last_error().decode())
    return out


def decode_jpeg(data):
    """cv::imdecode-style entry: the bytes of a JPEG stream -> HxWx3 BGR uint8 (libjpeg's default decode, byte for byte)."""
    L = lib(); b = bytes(data); r = C.c_int(); c = C.c_int(); k = C.c_int()
    if not L.pf_jpeg_info(b, len(b), C.byref(r), C.byref(c), C.byref(k)):
        raise ValueError("decode_jpeg: %s" % L.pf_last_error().decode())
    out = np.empty((r.value, c.value, 3), np.uint8)
    if not L.pf_jpeg_decode_bgr(b, len(b), out.ctypes.data, r.value, c.value):
        raise ValueError("decode_jpeg: %s" % L.pf_last_error().decode())
    return out


def jpeg_info(data):
    """(rows, cols, components) of a JPEG stream"""
    L = lib(); b = bytes(data); r = C.c_int(); c = C.c_int(); k = C.c_int()
    if not L.pf_jpeg_info(b, len(b), C.byref(r), C.byref(c), C.byref(k)):
        raise ValueError("jpeg_info: %s" % L.pf_last_error().decode())
    return r.value, c.value, k.value


def decode_jpeg_device(data, dev_ptr, rows, cols, stream=None):
    """The same decode with its back end on the GPU (csrc/jpeg_device.hip): BGR8, rows*cols*3 bytes at the device address `dev_ptr`,
    complete in the order of `stream` (a hipStream_t handle; None = the default stream).  Returns once the work is queued."""
    L = lib(); b = bytes(data)
    if not L.pf_jpeg_decode_device(b, len(b), dev_ptr, rows, cols, stream):
        raise ValueError("decode_jpeg_device: %s" % L.pf_last_error().decode())


def jpeg_encode(bgr, quality=95):
    """cv::imencode(".jpg")-style entry: HxWx3 BGR uint8 (rows may be padded: any array whose pixels are contiguous) -> the bytes
    of the baseline JPEG stream libjpeg writes for it (4:2:0, Annex K tables, quality as jpeg_set_quality takes it), byte for byte."""
    a = np.asarray(bgr)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.strides[2] != 1 or a.strides[1] != 3 or a.strides[0] < 3 * a.shape[1]:
        a = np.ascontiguousarray(bgr, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("jpeg_encode: HxWx3 expected")
    L = lib(); n = C.c_size_t(0)
    if not L.pf_jpeg_encode_bgr(a.ctypes.data, a.shape[0], a.shape[1], a.strides[0], quality, None, 0, C.byref(n)):
        raise ValueError("jpeg_encode: %s" % L.pf_last_error().decode())
    out = np.empty(n.value, np.uint8)
    if not L.pf_jpeg_encode_bgr(a.ctypes.data, a.shape[0], a.shape[1], a.strides[0], quality, out.ctypes.data, out.size, C.byref(n)):
        raise ValueError("jpeg_encode: %s" % L.pf_last_error().decode())
    return out[:n.value].tobytes()


def jpeg_encode_device(dev_ptr, rows, cols, quality=95, step=0, stream=None):
    """The same encoder on the GPU (csrc/jpeg_encode.hip) for rows x cols BGR8 pixels at the device address `dev_ptr`, `step` bytes
    per row (0 = packed), its passes in the order of `stream` (a hipStream_t handle; None = the default stream).  Returns the bytes
    of the stream: byte-equal to jpeg_encode."""
    L = lib(); n = C.c_size_t(0)
    if not L.pf_jpeg_encode_device(dev_ptr, rows, cols, step, quality, None, 0, C.byref(n), stream):
        raise ValueError("jpeg_encode_device: %s" % L.pf_last_error().decode())
    out = np.empty(n.value, np.uint8)
    if not L.pf_jpeg_encode_device(dev_ptr, rows, cols, step, quality, out.ctypes.data, out.size, C.byref(n), stream):
        raise ValueError("jpeg_encode_device: %s" % L.pf_last_error().decode())
    return out[:n.value].tobytes()


def _transform16(model_transform):
    if model_transform is None:
        return None, None
    a = np.ascontiguousarray(model_transform, dtype=np.float64).reshape(16)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def tiff_write(filename, bgr, quality=95, bg=0, model_transform=None, force_bigtiff=False):
    """HxWx3 BGR uint8 (rows may be padded) -> the tiled pyramid TIFF of pf_tiff_write_bgr (include/pifusion.h): JPEG tiles of 256 x 256,
    2 x 2-mean overviews down to one tile, all-background tiles stored once, geo tags when the 16 doubles are given.  Host code."""
    a = np.asarray(bgr)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.strides[2] != 1 or a.strides[1] != 3 or a.strides[0] < 3 * a.shape[1]:
        a = np.ascontiguousarray(bgr, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("tiff_write: HxWx3 expected")
    keep, xf = _transform16(model_transform)
    return bool(lib().pf_tiff_write_bgr(filename.encode(), a.ctypes.data, a.shape[0], a.shape[1], a.strides[0], quality, bg, xf, int(force_bigtiff)))


def tiff_write_device(filename, dev_ptr, rows, cols, quality=95, bg=0, model_transform=None, force_bigtiff=False, step=0, stream=None):
    """The same file, byte for byte, from rows x cols BGR8 pixels at the device address `dev_ptr` (csrc/overview.hip + jpeg_encode.hip)."""
    keep, xf = _transform16(model_transform)
    return bool(lib().pf_tiff_write_device(filename.encode(), dev_ptr, rows, cols, step, quality, bg, xf, int(force_bigtiff), stream))


def tiff_write_masked(filename, bgr, mask, quality=95, bg=0, model_transform=None, force_bigtiff=False):
    """tiff_write with a transparency mask behind every image (pf_tiff_write_bgr_masked): mask is HxW, non-zero = covered (rows may be
    padded); every overview's mask is the OR of the 2 x 2 blocks of the one above.  Host code."""
    a = np.asarray(bgr)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.strides[2] != 1 or a.strides[1] != 3 or a.strides[0] < 3 * a.shape[1]:
        a = np.ascontiguousarray(bgr, dtype=np.uint8)
    m = np.asarray(mask)
    if m.dtype == np.bool_:
        m = m.astype(np.uint8)
    if m.dtype != np.uint8 or m.ndim != 2 or m.strides[1] != 1 or m.strides[0] < m.shape[1]:
        m = np.ascontiguousarray(m, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 3 or m.shape != a.shape[:2]:
        raise ValueError("tiff_write_masked: HxWx3 and HxW expected")
    keep, xf = _transform16(model_transform)
    return bool(lib().pf_tiff_write_bgr_masked(filename.encode(), a.ctypes.data, a.shape[0], a.shape[1], a.strides[0], m.ctypes.data, m.strides[0],
                                               quality, bg, xf, int(force_bigtiff)))


def tiff_write_device_masked(filename, dev_ptr, rows, cols, dev_mask, quality=95, bg=0, model_transform=None, force_bigtiff=False, step=0, mask_step=0, stream=None):
    """The same file, byte for byte, from pixels and a byte-per-pixel mask at device addresses (csrc/coverage.hip beside overview.hip)."""
    keep, xf = _transform16(model_transform)
    return bool(lib().pf_tiff_write_device_masked(filename.encode(), dev_ptr, rows, cols, step, dev_mask, mask_step, quality, bg, xf, int(force_bigtiff), stream))


DEFLATE_TILE_BOUND = 196608 + 5 * 16 + 6          # no tile stream is longer (include/pifusion.h)


def deflate_tile(tile):
    """256x256x3 BGR uint8 (rows may be padded) -> the tile's zlib stream of pf_deflate_tile_bgr (include/pifusion.h): Predictor 2,
    run-length tokens at distance 1, 16 blocks, dynamic Huffman or stored.  Host code."""
    a = np.asarray(tile)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.strides[2] != 1 or a.strides[1] != 3 or a.strides[0] < 3 * a.shape[1]:
        a = np.ascontiguousarray(tile, dtype=np.uint8)
    if a.shape != (256, 256, 3):
        raise ValueError("deflate_tile: 256x256x3 expected")
    out = np.empty(DEFLATE_TILE_BOUND, np.uint8)
    n = C.c_size_t(0)
    if not lib().pf_deflate_tile_bgr(a.ctypes.data, a.strides[0], out.ctypes.data, out.size, C.byref(n)):
        raise RuntimeError("pf_deflate_tile_bgr failed: %s" % lib().pf_last_error().decode())
    return out[:n.value].tobytes()


def deflate_code_lengths(freq, max_len):
    """the codec's length builder (pf_deflate_code_lengths): counts -> code lengths, none above max_len"""
    f = np.ascontiguousarray(freq, dtype=np.uint32)
    out = np.zeros(f.size, np.uint8)
    if not lib().pf_deflate_code_lengths(f.ctypes.data, f.size, max_len, out.ctypes.data):
        raise ValueError("pf_deflate_code_lengths failed: %s" % lib().pf_last_error().decode())
    return out


def deflate_tiles_device(dev_ptr, byte_offsets, step, stream=None):
    """The streams of the tiles that begin byte_offsets[i] bytes behind the device address `dev_ptr` (rows of `step` bytes), encoded on
    the GPU (csrc/deflate_encode.hip): a list of bytes objects, each equal to deflate_tile of the same pixels."""
    w = np.ascontiguousarray(byte_offsets, dtype=np.int64)
    n = int(w.size)
    off = np.zeros(n + 1, np.uint64)
    out = np.empty(n * DEFLATE_TILE_BOUND, np.uint8)
    if not lib().pf_deflate_tiles_device(dev_ptr, n, w.ctypes.data, step, out.ctypes.data, out.size, off.ctypes.data, stream):
        raise RuntimeError("pf_deflate_tiles_device failed: %s" % lib().pf_last_error().decode())
    return [out[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)]


def tiff_write_lossless(filename, bgr, mask=None, bg=0, model_transform=None, force_bigtiff=False):
    """tiff_write / tiff_write_masked with lossless tiles (pf_tiff_write_bgr_lossless): Compression 8, Predictor 2, every tile the
    stream of deflate_tile.  mask None: the unmasked file.  Host code."""
    a = np.asarray(bgr)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.strides[2] != 1 or a.strides[1] != 3 or a.strides[0] < 3 * a.shape[1]:
        a = np.ascontiguousarray(bgr, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("tiff_write_lossless: HxWx3 expected")
    mp, ms = None, 0
    if mask is not None:
        m = np.asarray(mask)
        if m.dtype == np.bool_:
            m = m.astype(np.uint8)
        if m.dtype != np.uint8 or m.ndim != 2 or m.strides[1] != 1 or m.strides[0] < m.shape[1]:
            m = np.ascontiguousarray(m, dtype=np.uint8)
        if m.shape != a.shape[:2]:
            raise ValueError("tiff_write_lossless: HxWx3 and HxW expected")
        mp, ms = m.ctypes.data, m.strides[0]
    keep, xf = _transform16(model_transform)
    return bool(lib().pf_tiff_write_bgr_lossless(filename.encode(), a.ctypes.data, a.shape[0], a.shape[1], a.strides[0], mp, ms, bg, xf, int(force_bigtiff)))


def tiff_write_device_lossless(filename, dev_ptr, rows, cols, dev_mask=None, bg=0, model_transform=None, force_bigtiff=False, step=0, mask_step=0, stream=None):
    """The same file, byte for byte, from pixels (and a byte-per-pixel mask, or None) at device addresses (csrc/overview.hip + deflate_encode.hip)."""
    keep, xf = _transform16(model_transform)
    return bool(lib().pf_tiff_write_device_lossless(filename.encode(), dev_ptr, rows, cols, step, dev_mask, mask_step, bg, xf, int(force_bigtiff), stream))


def _png_mask(mask, shape, who):
    if mask is None:
        return None, None, 0
    m = np.asarray(mask)
    if m.dtype == np.bool_:
        m = m.astype(np.uint8)
    if m.dtype != np.uint8 or m.ndim != 2 or m.strides[1] != 1 or m.strides[0] < m.shape[1]:
        m = np.ascontiguousarray(m, dtype=np.uint8)
    if m.shape != shape:
        raise ValueError("%s: HxWx3 and HxW expected" % who)
    return m, m.ctypes.data, m.strides[0]


def png_encode(bgr, mask=None):
    """HxWx3 BGR uint8 (rows may be padded) and, optionally, an HxW mask (non-zero = covered) -> the bytes of the PNG file of
    pf_png_encode_bgr (include/pifusion.h): RGB, or RGBA with alpha 255 where covered; Sub filter, run-length deflate.  Host code."""
    a = np.asarray(bgr)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.strides[2] != 1 or a.strides[1] != 3 or a.strides[0] < 3 * a.shape[1]:
        a = np.ascontiguousarray(bgr, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("png_encode: HxWx3 expected")
    keep, mp, ms = _png_mask(mask, a.shape[:2], "png_encode")
    L = lib(); n = C.c_size_t(0)
    if not L.pf_png_encode_bgr(a.ctypes.data, a.shape[0], a.shape[1], a.strides[0], mp, ms, None, 0, C.byref(n)):
        raise ValueError("png_encode: %s" % L.pf_last_error().decode())
    out = np.empty(n.value, np.uint8)
    if not L.pf_png_encode_bgr(a.ctypes.data, a.shape[0], a.shape[1], a.strides[0], mp, ms, out.ctypes.data, out.size, C.byref(n)):
        raise ValueError("png_encode: %s" % L.pf_last_error().decode())
    return out[:n.value].tobytes()


def png_encode_device(dev_ptr, rows, cols, dev_mask=None, step=0, mask_step=0, stream=None):
    """The same file, byte for byte, made on the GPU (csrc/png_encode.hip) from rows x cols BGR8 pixels at the device address `dev_ptr`
    (`step` bytes per row, 0 = packed) and a byte-per-pixel mask at `dev_mask` (or None), its passes in the order of `stream`."""
    L = lib(); n = C.c_size_t(0)
    if not L.pf_png_encode_device(dev_ptr, rows, cols, step, dev_mask, mask_step, None, 0, C.byref(n), stream):
        raise ValueError("png_encode_device: %s" % L.pf_last_error().decode())
    out = np.empty(n.value, np.uint8)
    if not L.pf_png_encode_device(dev_ptr, rows, cols, step, dev_mask, mask_step, out.ctypes.data, out.size, C.byref(n), stream):
        raise ValueError("png_encode_device: %s" % L.pf_last_error().decode())
    return out[:n.value].tobytes()


def tiff_counts(map2d=None):
    """(tiles of all images, the empty ones among them, bytes of device memory held for levels and flags) of the last pyramid TIFF the
    map -- or, map2d None, the process-wide writer behind tiff_write_device* on the current device -- made on the GPU (pf_debug_tiff_counts)"""
    out = (C.c_longlong * 3)()
    lib().pf_debug_tiff_counts(map2d._h if map2d is not None else None, out)
    return tuple(int(v) for v in out)


def jpeg_huffman_counts(map2d=None):
    """(frames whose Huffman pass ran on the GPU, frames that fell back to the host after trying, rounds of the most recent GPU pass) of a map's
    decoder, or of decode_jpeg_device's when map2d is None"""
    out = (C.c_longlong * 3)()
    lib().pf_debug_jpeg_huffman(map2d._h if map2d is not None else None, out)
    return tuple(out)


def _d(values, n):
    a = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    if a.size != n:
        raise ValueError("%d doubles expected" % n)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def webtiles_georef_compose(model_transform, plane, gps_origin):
    """px2ll (6 doubles: lng = P0 + P1 col + P2 row, lat = P3 + P4 col + P5 row) of a mosaic whose TIFF would carry model_transform (16
    doubles, pixel -> plane metres), on the plane `plane` around gps_origin (pf_webtiles_georef_compose); None for a singular affine"""
    (_, t), (_, p), (_, g) = _d(model_transform, 16), _d(plane, 7), _d(gps_origin, 3)
    out = np.zeros(6)
    return out if lib().pf_webtiles_georef_compose(t, p, g, out.ctypes.data_as(C.POINTER(C.c_double))) else None


def webtiles_native_zoom(px2ll, rows, cols):
    """the smallest zoom at which a source pixel spans at least 1 / sqrt 2 output pixel (pf_webtiles_native_zoom); -1: no such plan"""
    _, p = _d(px2ll, 6)
    return int(lib().pf_webtiles_native_zoom(p, rows, cols))


def webtiles_plan(px2ll, rows, cols, z):
    """((tx0, ty0, tx1, ty1), UX, UY, VX, VY) of pf_webtiles_plan: the inclusive tile range of zoom z and the tables over its global
    columns and rows -- output pixel (c, r) samples the source at (UX[c] + VX[r], UY[c] + VY[r]).  Raises ValueError on a refusal"""
    L = lib(); _, p = _d(px2ll, 6)
    rg = (C.c_int * 4)(-1, -1, -1, -1)
    if not L.pf_webtiles_plan(p, rows, cols, z, rg, None, None, None, None, 0, 0):          # without tables: the range alone, which says what is needed
        raise ValueError(L.pf_last_error().decode())
    nc, nr = 256 * (rg[2] - rg[0] + 1), 256 * (rg[3] - rg[1] + 1)
    ux, uy, vx, vy = np.empty(nc), np.empty(nc), np.empty(nr), np.empty(nr)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    if not L.pf_webtiles_plan(p, rows, cols, z, rg, ptr(ux), ptr(uy), ptr(vx), ptr(vy), nc, nr):
        raise ValueError(L.pf_last_error().decode())
    return tuple(rg), ux, uy, vx, vy


def _matrix9(V):
    a = np.ascontiguousarray(V, dtype=np.float64).reshape(9)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def view_plan(V, width, height, level, dims, geo, num_levels, extent):
    """pf_view_plan: the plan of a view without a map (host code).  dims, geo as Map2D.grid() gives them, extent = (first tile x, y, tiles
    across, tiles down) of the content.  Returns the ViewInfo as a dict; raises ValueError with the reason where a view is refused."""
    _, pv = _matrix9(V)
    d = (C.c_int * 4)(*[int(v) for v in dims]); e = (C.c_int * 4)(*[int(v) for v in extent])
    _, g = _d(geo, 6)
    info = ViewInfo()
    if not lib().pf_view_plan(pv, int(width), int(height), int(level), d, g, int(num_levels), e, C.byref(info)):
        raise ValueError(lib().pf_last_error().decode())
    return info.as_dict()


def _collect_webtiles(call, pixels):
    """runs call(sink) and returns the records the sink saw: dicts z, x, y, cover (1 partial, 2 full), jpeg (bytes), mask (256 x 256 bool,
    None for a fully covered tile), and bgr (256 x 256 x 3) when pixels were asked for"""
    out = []

    def sink(user, t):
        t = t.contents
        rec = {"z": t.z, "x": t.x, "y": t.y, "cover": t.cover, "jpeg": C.string_at(t.jpeg, t.jpeg_len), "mask": None}
        if t.mask8192:
            rec["mask"] = np.unpackbits(np.frombuffer(C.string_at(t.mask8192, 8192), np.uint8)).reshape(256, 256).astype(bool)
        if pixels and t.bgr:
            rec["bgr"] = np.frombuffer(C.string_at(t.bgr, 256 * 256 * 3), np.uint8).reshape(256, 256, 3).copy()
        out.append(rec)
        return 1

    cb = WEBTILE_SINK(sink)
    if not call(cb):
        raise RuntimeError(lib().pf_last_error().decode())
    return out


def webtiles_device(dev_ptr, rows, cols, dev_mask, px2ll, zmin=None, zmax=None, quality=95, bg=0, pixels=False, step=0, mask_step=0, stream=None):
    """North-up Web-Mercator map tiles (z/x/y, 256 x 256) of rows x cols BGR8 pixels and a byte-per-pixel coverage at device addresses,
    placed by px2ll (pf_webtiles_device, csrc/webtiles.hip): the list of records of every tile with a covered pixel, zmax (None: the
    native zoom) down to zmin (None: the zoom at which one tile holds the image)."""
    _, p = _d(px2ll, 6)
    return _collect_webtiles(lambda cb: lib().pf_webtiles_device(dev_ptr, rows, cols, step, dev_mask, mask_step, p, -1 if zmin is None else zmin, -1 if zmax is None else zmax,
                                                                 quality, bg, int(pixels), cb, None, stream), pixels)


def _image_of(array):
    """(Image, keepalive) of a host frame as Map2D.feed and Map2D.prepare(images=...) hand it over: the type from the shape -- HxWx3
    uint8 is PF_8UC3 (BGR), HxWx4 uint8 PF_8UC4 (BGRA as the tracker holds it, TrackerOpt.cpp:376), anything else -1, which the library
    rejects -- and the row step of a row-padded view (cv::Mat::step) carried over.  No cast: an array of another dtype is not a frame."""
    img = np.asarray(array)
    step = 0
    if img.ndim == 3 and img.dtype == np.uint8 and img.strides[2] == 1 and img.strides[1] == img.shape[2] and img.strides[0] >= img.shape[1] * img.shape[2]:
        step = img.strides[0]                       # row-padded view: handed over as is
    else:
        img = np.ascontiguousarray(img)
    typ = -1
    if img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] in (3, 4):
        typ = PF_8UC3 if img.shape[2] == 3 else PF_8UC4
    rows, cols = (img.shape[0], img.shape[1]) if img.ndim >= 2 else (0, 0)
    return Image(rows, cols, typ, img.ctypes.data, step), img


def state_info(path):
    """What a map state file holds (pf_state_info; host code, no device): a dict with type, pyramid_type, band_number, weight_type,
    tiles, w, h (the grid in tiles), version, plane (7), cam (6) and geo (6, as grid() gives it) -- or None, with the reason in
    pf_last_error(), for a file load_state would refuse on sight."""
    info = (C.c_int * 8)(); plane = (C.c_double * 7)(); cam = (C.c_double * 6)(); geo = (C.c_double * 6)()
    if not lib().pf_state_info(os.fsencode(path), info, plane, cam, geo):
        return None
    keys = ("type", "pyramid_type", "band_number", "weight_type", "tiles", "w", "h", "version")
    out = {k: int(v) for k, v in zip(keys, info)}
    out.update(plane=list(plane), cam=list(cam), geo=list(geo))
    return out


def tile_owner(opt, ix, iy):
    return lib().pf_tile_owner(C.byref(opt), ix, iy)


# ---- undistortion (pf_undistort_*; DESIGN.md "Undistortion").  camera_in: a GSLAM parameter vector of 6 (PinHole), 7 (ATAN) or 11
# (OpenCV) numbers; camera_out: the six of a pinhole camera
def _cameras(camera_in, camera_out):
    ci = (C.c_double * len(camera_in))(*[float(v) for v in camera_in])
    co = (C.c_double * 6)(*[float(v) for v in np.asarray(camera_out, dtype=np.float64).reshape(-1)])
    return ci, co


def undistort_table(camera_in, camera_out):
    """The remap table on the host (no GPU): (x, y, uncovered) -- two float32 arrays of the output camera's h x w, (-1, -1) where the
    output pixel looks past the input image, and the number of such pixels.  None, with the reason in pf_last_error(), for a camera
    that is not valid."""
    ci, co = _cameras(camera_in, camera_out)
    if not (int(co[0]) >= 1 and int(co[1]) >= 1 and co[0] < 65536 and co[1] < 65536):
        return None
    x = np.empty((int(co[1]), int(co[0])), np.float32); y = np.empty_like(x)
    unc = C.c_longlong(0)
    fp = C.POINTER(C.c_float)
    if not lib().pf_undistort_table(ci, len(camera_in), co, x.ctypes.data_as(fp), y.ctypes.data_as(fp), C.byref(unc)):
        return None
    return x, y, int(unc.value)


def fit_camera(camera_in, camera_out):
    """camera_out with (fx, fy) multiplied by the smallest s = k / 4096 >= 1 at which the whole border of the output image is covered by
    the input camera (pf_undistort_fit_camera; host only), as a list of six -- or None when there is none up to s = 64."""
    ci, co = _cameras(camera_in, camera_out)
    if not lib().pf_undistort_fit_camera(ci, len(camera_in), co):
        return None
    return list(co)


def undistort(img, camera_in, camera_out):
    """One host frame (HxWx3 BGR or HxWx4 BGRA uint8, of camera_in's size) undistorted on the GPU into camera_out: an h x w x 3 array."""
    ci, co = _cameras(camera_in, camera_out)
    im, keep = _image_of(img)
    out = np.empty((max(int(co[1]), 0), max(int(co[0]), 0), 3), np.uint8)
    if not lib().pf_undistort_bgr(ci, len(camera_in), co, C.byref(im), out.ctypes.data, 0):
        raise RuntimeError("pf_undistort_bgr failed: %s" % lib().pf_last_error().decode())
    return out


def undistort_device(src_ptr, camera_in, camera_out, dst_ptr, channels=3, src_step=0, dst_step=0, stream=None):
    """The same on device pointers (pf_undistort_device), queued on `stream`: src_ptr holds camera_in's h rows of w BGR / BGRA pixels,
    dst_ptr takes camera_out's packed BGR rows."""
    ci, co = _cameras(camera_in, camera_out)
    im = Image(int(camera_in[1]), int(camera_in[0]), PF_8UC3 if channels == 3 else PF_8UC4, src_ptr, src_step)
    return bool(lib().pf_undistort_device(ci, len(camera_in), co, C.byref(im), dst_ptr, dst_step, stream))


# ---- raw frames (pf_raw_*; DESIGN.md "Raw frames")
def _raw_planes(planes, format, rows, cols):
    """(list of 2-D uint8 arrays with contiguous rows, rows, cols) from one array in the usual packed layout (NV12 / NV21: rows * 3 / 2 x cols,
    I420: the same bytes, Y then U then V; grey and Bayer: rows x cols) or from a tuple of planes (any row stride)."""
    n = 3 if format == RAW_I420 else 2 if format in (RAW_NV12, RAW_NV21) else 1
    if isinstance(planes, np.ndarray):
        a = np.ascontiguousarray(planes, dtype=np.uint8)
        if n == 1:
            if a.ndim != 2:
                raise ValueError("raw frame: a grey or Bayer frame is a rows x cols array")
            planes = (a,)
        else:
            if cols is None:
                if a.ndim != 2:
                    raise ValueError("raw frame: a packed YUV frame is a (rows * 3 / 2) x cols array, or give rows and cols")
                cols = a.shape[1]
            if rows is None:
                rows = a.size // cols * 2 // 3
            if rows < 0 or cols < 0 or rows % 2 or cols % 2 or a.size != rows * cols * 3 // 2:
                raise ValueError("raw frame: a packed YUV 4:2:0 frame has even rows and cols and rows * cols * 3 / 2 bytes")
            flat = a.reshape(-1)
            y = flat[:rows * cols].reshape(rows, cols)
            if n == 2:
                planes = (y, flat[rows * cols:].reshape(rows // 2, cols))
            else:
                q = rows * cols // 4
                planes = (y, flat[rows * cols:rows * cols + q].reshape(rows // 2, cols // 2), flat[rows * cols + q:].reshape(rows // 2, cols // 2))
    planes = list(planes)
    if len(planes) != n:
        raise ValueError("raw frame: format %d has %d plane(s)" % (format, n))
    out = []
    for p in planes:
        p = np.asarray(p)
        if p.dtype != np.uint8 or p.ndim != 2:
            raise ValueError("raw frame: planes are 2-D uint8 arrays")
        if p.shape[1] > 1 and p.strides[1] != 1 or (p.shape[0] > 1 and p.strides[0] < p.shape[1]):
            p = np.ascontiguousarray(p)
        out.append(p)
    if rows is None:
        rows = out[0].shape[0]
    if cols is None:
        cols = out[0].shape[1]
    return out, int(rows), int(cols)


def _raw_frame(planes, format, rows, cols):
    f = RawFrame(int(format), rows, cols)
    for k, p in enumerate(planes):
        f.plane[k] = p.ctypes.data
        f.step[k] = p.strides[0] if p.shape[0] > 1 else p.shape[1]
    return f


class RawImage:
    """A raw frame on its way to Map2D.feed (the file driver's <name>.nv12): planes as raw_to_bgr takes them, and the RAW_* format."""

    def __init__(self, planes, format, rows=None, cols=None):
        self.planes, self.format, self.rows, self.cols = planes, format, rows, cols

    def to_bgr(self):
        return raw_to_bgr(self.planes, self.format, self.rows, self.cols)


def raw_to_bgr(planes, format, rows=None, cols=None):
    """A raw frame (one packed array or a tuple of planes; RAW_* format) converted on the host (pf_raw_to_bgr, no GPU): rows x cols x 3 BGR."""
    ps, rows, cols = _raw_planes(planes, format, rows, cols)
    f = _raw_frame(ps, format, rows, cols)
    out = np.empty((max(rows, 0), max(cols, 0), 3), np.uint8)
    if not lib().pf_raw_to_bgr(C.byref(f), out.ctypes.data, 0):
        raise ValueError("pf_raw_to_bgr: %s" % lib().pf_last_error().decode())
    return out


def raw_to_bgr_device(ptrs, steps, format, rows, cols, dst_ptr, dst_step=0, stream=None):
    """The same on device pointers (pf_raw_to_bgr_device), queued on `stream`: ptrs / steps of the format's planes, dst_ptr takes BGR rows."""
    f = RawFrame(int(format), int(rows), int(cols))
    for k, (p, s) in enumerate(zip(ptrs, steps)):
        f.plane[k] = p
        f.step[k] = s
    return bool(lib().pf_raw_to_bgr_device(C.byref(f), dst_ptr, dst_step, stream))


class Map2D:
    """Map2D::create(type, thread) -> object with prepare/feed/save/queueSize."""

    def __init__(self, handle, opt):
        self._h = handle
        self.opt = opt

    @staticmethod
    def create(type=TypeMultiBandCPU, thread=False, options=None, **kw):
        opt = options if options is not None else default_options(**kw)
        h = lib().pf_create(type, 1 if thread else 0, C.byref(opt))
        if not h:
            if type in (NoType, TypeRender):
                return None
            raise RuntimeError("pf_create failed: %s" % lib().pf_last_error().decode())
        return Map2D(h, opt)

    def close(self):
        if self._h:
            lib().pf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- Map2D virtuals
    def prepare(self, plane, camera, poses, images=None):
        """plane: 7 doubles; camera: [w h fx fy cx cy]; poses: n x 7 camera-to-world."""
        pl, ppl = _pose(plane); cam, pc = _pose(camera)
        ps = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
        imgs = None
        keep = []
        if images is not None:
            imgs = (Image * len(images))()
            for i, im in enumerate(images):
                imgs[i], k = _image_of(im); keep.append(k)
        return bool(lib().pf_prepare(self._h, ppl, pc, ps.shape[0], imgs, ps.ctypes.data_as(C.POINTER(C.c_double))))

    def feed(self, img, pose):
        """img: HxWx3 (BGR) or HxWx4 (BGRA) uint8 numpy array (host), None for a geometry-only frame, or the bytes of a .jpg
        file (decoded by the map: feed_jpeg), or a RawImage (converted by the map: feed_raw)."""
        if isinstance(img, (bytes, bytearray, memoryview)):
            return self.feed_jpeg(img, pose)
        if isinstance(img, RawImage):
            return self.feed_raw(img.planes, img.format, pose, img.rows, img.cols)
        p, pp = _pose(pose)
        if img is None:
            return bool(lib().pf_feed(self._h, None, pp))
        im, keep = _image_of(img)
        return bool(lib().pf_feed(self._h, C.byref(im), pp))

    def feed_device(self, data_ptr, rows, cols, pose, step=0, channels=3):
        """Frame already resident in HBM (e.g. torch tensor .data_ptr()): BGR, or BGRA with channels=4 (pf_feed_device takes both)."""
        if channels not in (3, 4):
            raise ValueError("feed_device: 3 (BGR) or 4 (BGRA) channels")
        p, pp = _pose(pose)
        im = Image(rows, cols, PF_8UC3 if channels == 3 else PF_8UC4, data_ptr, step)
        return bool(lib().pf_feed_device(self._h, C.byref(im), pp))

    def feed_jpeg(self, data, pose):
        """feed(cv::imread(file), pose) in one call: the JPEG stream is decoded into HBM on the map's stream (Huffman on this thread,
        IDCT / upsampling / colour on the GPU) and rendered from there."""
        p, pp = _pose(pose)
        b = bytes(data)
        return bool(lib().pf_feed_jpeg(self._h, b, len(b), pp))

    def feed_raw(self, planes, format, pose, rows=None, cols=None):
        """feed() of the BGR picture a raw frame converts to (pf_feed_raw): the planes cross to HBM as they are -- 1 or 1.5 bytes a pixel --
        and are converted there.  planes: one contiguous array in the usual packed layout (NV12: rows * 3 / 2 x cols) or a tuple of planes."""
        ps, rows, cols = _raw_planes(planes, format, rows, cols)
        f = _raw_frame(ps, format, rows, cols)
        p, pp = _pose(pose)
        return bool(lib().pf_feed_raw(self._h, C.byref(f), pp))

    def feed_raw_device(self, ptrs, steps, format, rows, cols, pose):
        """The same from planes that lie in HBM (pf_feed_raw_device; thread=False maps): converted on the map's stream inside the call; the
        planes must stay valid and unchanged until sync()."""
        f = RawFrame(int(format), int(rows), int(cols))
        for k, (q, s) in enumerate(zip(ptrs, steps)):
            f.plane[k] = q
            f.step[k] = s
        p, pp = _pose(pose)
        return bool(lib().pf_feed_raw_device(self._h, C.byref(f), pp))

    def feed_jpeg_batch(self, streams, poses, threads=0):
        """n .jpg keyframes at once: Huffman passes on `threads` host threads (0: one per frame), the rest on the GPU, fed in order.
        Returns the list of per-frame results (what feed_jpeg returns)."""
        n = len(streams)
        keep = [bytes(s) for s in streams]
        data = (C.c_char_p * n)(*keep); lens = (C.c_size_t * n)(*[len(s) for s in keep])
        pp = (C.c_double * (7 * n))(*[float(v) for p in poses for v in p])
        res = (C.c_int * n)()
        lib().pf_feed_jpeg_batch(self._h, n, data, lens, pp, threads, res)
        return [bool(r) for r in res]

    # ---- input camera (pf_set_input_camera; DESIGN.md "Undistortion")
    def set_input_camera(self, camera_in):
        """From now on every frame fed is a frame of camera_in (GSLAM parameters: 6 PinHole, 7 ATAN, 11 OpenCV; its own width and height)
        and is undistorted on the GPU into the camera of prepare().  None or () clears it.  Survives prepare(), not load_state()."""
        vals = [] if camera_in is None else [float(v) for v in camera_in]
        ci = (C.c_double * max(len(vals), 1))(*vals)
        return bool(lib().pf_set_input_camera(self._h, ci, len(vals)))

    def input_camera_info(self):
        """None without an input camera, else (rows_in, cols_in, uncovered): the frame size the map expects and the output pixels the
        input camera does not cover (-1 before prepare())."""
        r = C.c_int(0); c = C.c_int(0); u = C.c_longlong(0)
        if not lib().pf_input_camera_info(self._h, C.byref(r), C.byref(c), C.byref(u)):
            return None
        return r.value, c.value, int(u.value)

    undistort = staticmethod(undistort)
    undistort_table = staticmethod(undistort_table)
    fit_camera = staticmethod(fit_camera)

    def read_last_frame(self):
        """test hook: bytes of the most recently uploaded host frame as they lie in HBM"""
        n = lib().pf_debug_read_last_frame(self._h, None, 0)
        if n < 0:
            return None
        out = np.empty(n, np.uint8)
        return out if lib().pf_debug_read_last_frame(self._h, out.ctypes.data, n) == n else None

    def queueSize(self):
        return int(lib().pf_queue_size(self._h))

    def sync(self):
        return bool(lib().pf_sync(self._h))

    def save(self, filename):
        return bool(lib().pf_save(self._h, filename.encode()))

    def save_tiff(self, filename, quality=95, force_bigtiff=False):
        """save("x.tif") with the tiles' JPEG quality and the flag that forces BigTIFF (pf_save_tiff)"""
        return bool(lib().pf_save_tiff(self._h, filename.encode(), quality, int(force_bigtiff)))

    def save_tiff_masked(self, filename, quality=95, force_bigtiff=False):
        """save_tiff with a transparency mask behind every image: covered where the level-0 weight is not 0 (pf_save_tiff_masked)"""
        return bool(lib().pf_save_tiff_masked(self._h, filename.encode(), quality, int(force_bigtiff)))

    def save_tiff_lossless(self, filename, masked=False, force_bigtiff=False):
        """the mosaic as a pyramid TIFF with lossless (Deflate) tiles, with or without the transparency masks (pf_save_tiff_lossless)"""
        return bool(lib().pf_save_tiff_lossless(self._h, filename.encode(), int(masked), int(force_bigtiff)))

    def save_png(self, filename, masked=False):
        """the mosaic as a PNG encoded on the GPU, under any name (pf_save_png); masked: RGBA, alpha 0 where save() paints the background"""
        return bool(lib().pf_save_png(self._h, filename.encode(), int(masked)))

    def save_to_memory_mask(self):
        """(mosaic BGR8, coverage HxW uint8: 255 where the level-0 weight is not 0, (tile x0, tile y0)) of one moment"""
        r, c, x0, y0 = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        if not lib().pf_save_to_memory_mask(self._h, None, None, C.byref(r), C.byref(c), C.byref(x0), C.byref(y0)):
            return None
        # (the extent may have grown between the two calls: the second call fills what it reports, so it is asked until it fits)
        while True:
            out = np.empty((r.value, c.value, 3), np.uint8); mask = np.empty((r.value, c.value), np.uint8)
            want = (r.value, c.value)
            if not lib().pf_save_to_memory_mask(self._h, out.ctypes.data, mask.ctypes.data, C.byref(r), C.byref(c), C.byref(x0), C.byref(y0)):
                return None
            if (r.value, c.value) == want:
                return out, mask, (x0.value, y0.value)

    def webtiles_georef(self, gps_origin):
        """(px2ll, rows, cols) of the mosaic save_to_memory would return now, around gps_origin = (lng, lat, alt) (pf_webtiles_georef);
        None for an empty or sharded map or a vertical plane"""
        _, g = _d(gps_origin, 3)
        out = np.zeros(6); r, c = C.c_int(), C.c_int()
        if not lib().pf_webtiles_georef(self._h, g, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(r), C.byref(c)):
            return None
        return out, r.value, c.value

    def webtiles(self, gps_origin, zmin=None, zmax=None, quality=95, pixels=False):
        """The mosaic of this moment as north-up Web-Mercator map tiles (pf_webtiles): yields the records of webtiles_device"""
        _, g = _d(gps_origin, 3)
        for rec in _collect_webtiles(lambda cb: lib().pf_webtiles(self._h, g, -1 if zmin is None else zmin, -1 if zmax is None else zmax, quality, int(pixels), cb, None), pixels):
            yield rec

    def save_webtiles(self, dir, gps_origin, zmin=None, zmax=None, quality=95):
        """dir/z/x/y.jpg, dir/z/x/y.pbm (coverage of the partly covered tiles) and dir/tiles.json (pf_save_webtiles)"""
        _, g = _d(gps_origin, 3)
        return bool(lib().pf_save_webtiles(self._h, str(dir).encode(), g, -1 if zmin is None else zmin, -1 if zmax is None else zmax, quality))

    def export_mbtiles(self, path, gps_origin, zmin=None, zmax=None, quality=95, name="mosaic"):
        """The same tiles as an MBTiles file (sqlite3): tables tiles (TMS rows: tile_row = 2^z - 1 - y) and metadata (format jpg, bounds,
        minzoom, maxzoom).  Returns the number of tiles written"""
        import sqlite3
        geo = self.webtiles_georef(gps_origin)
        if geo is None:
            raise RuntimeError(lib().pf_last_error().decode())
        recs = list(self.webtiles(gps_origin, zmin, zmax, quality))
        p, rows, cols = geo
        lng = [p[0] + p[1] * c + p[2] * r for c in (0, cols) for r in (0, rows)]
        lat = [p[3] + p[4] * c + p[5] * r for c in (0, cols) for r in (0, rows)]
        db = sqlite3.connect(str(path))
        try:
            db.execute("CREATE TABLE tiles (zoom_level INTEGER, tile_column INTEGER, tile_row INTEGER, tile_data BLOB)")
            db.execute("CREATE UNIQUE INDEX tile_index ON tiles (zoom_level, tile_column, tile_row)")
            db.execute("CREATE TABLE metadata (name TEXT, value TEXT)")
            db.executemany("INSERT INTO tiles VALUES (?, ?, ?, ?)", [(t["z"], t["x"], (1 << t["z"]) - 1 - t["y"], t["jpeg"]) for t in recs])
            zs = [t["z"] for t in recs]
            meta = {"name": name, "format": "jpg", "type": "overlay", "version": "1", "bounds": "%.8f,%.8f,%.8f,%.8f" % (min(lng), min(lat), max(lng), max(lat)),
                    "minzoom": str(min(zs)), "maxzoom": str(max(zs))}
            db.executemany("INSERT INTO metadata VALUES (?, ?)", sorted(meta.items()))
            db.commit()
        finally:
            db.close()
        return len(recs)

    def save_to_memory(self, alloc=None, level=0):
        """(mosaic BGR8, (tile x0, tile y0)); alloc(shape) -> uint8 array supplies the buffer (e.g. host_array).  level=k: the
        mosaic collapsed down to pyramid level k, (256 >> k) pixels a tile (pf_save_to_memory_level); None where the map has no
        such view."""
        r, c, x0, y0 = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        if hasattr(lib(), "pf_save_to_memory_level"):          # (PF_LIB = an older build: level 0 through its own entry point)
            call = lambda p: lib().pf_save_to_memory_level(self._h, level, p, C.byref(r), C.byref(c), C.byref(x0), C.byref(y0))
        elif level == 0:
            call = lambda p: lib().pf_save_to_memory(self._h, p, C.byref(r), C.byref(c), C.byref(x0), C.byref(y0))
        else:
            raise RuntimeError("this build of the library has no level views")
        if not call(None):
            return None
        out = alloc((r.value, c.value, 3)) if alloc else np.empty((r.value, c.value, 3), np.uint8)
        if not call(out.ctypes.data):
            return None
        return out, (x0.value, y0.value)

    # ---- views (pf_render_view*; DESIGN.md "Views")
    def render_view(self, V, width, height, level=-1, channels=4, out=None):
        """The mosaic under V (3 x 3, plane metres -> view pixels) as a height x width x channels uint8 image, warped on the GPU from the
        tiles the view depends on: B G R and, with channels=4, the coverage.  level=-1: the pyramid level that fits the view's scale.
        out: a caller's array of that shape (its rows may be padded; host_array(): page-locked, filled straight from HBM).  Returns
        (array, info dict); raises ValueError with the reason where the view is refused (out keeps its bytes)."""
        _, pv = _matrix9(V)
        if out is None:
            out = np.empty((max(height, 1), max(width, 1), channels), np.uint8)          # (a size the map refuses still gets a buffer to refuse)
        elif out.dtype != np.uint8 or out.shape != (height, width, channels) or out.strides[2] != 1 or out.strides[1] != channels or out.strides[0] < width * channels:
            raise ValueError("render_view: out must be height x width x channels uint8 with contiguous pixels")
        info = ViewInfo()
        if not lib().pf_render_view(self._h, pv, width, height, level, channels, out.ctypes.data, out.strides[0], C.byref(info)):
            raise ValueError(lib().pf_last_error().decode())
        return out, info.as_dict()

    def render_view_device(self, V, width, height, dev_ptr, level=-1, channels=4, step=0, stream=None):
        """render_view into device memory (e.g. a torch tensor's .data_ptr()): the view stays in HBM.  stream: a hipStream_t handle the
        work is ordered into (the call returns once it is queued); None: complete on return.  Returns the info dict."""
        _, pv = _matrix9(V)
        info = ViewInfo()
        if not lib().pf_render_view_device(self._h, pv, width, height, level, channels, dev_ptr, step, stream, C.byref(info)):
            raise ValueError(lib().pf_last_error().decode())
        return info.as_dict()

    def render_view_jpeg(self, V, width, height, level=-1, quality=95, cap=None):
        """The 3-channel view as one JPEG stream, encoded on the GPU (only the stream crosses to the host): (bytes, info dict)."""
        _, pv = _matrix9(V)
        L = lib(); n = C.c_size_t(0)
        if cap is None:
            if not L.pf_render_view_jpeg(self._h, pv, width, height, level, quality, None, 0, C.byref(n), None):
                raise ValueError(L.pf_last_error().decode())
            cap = n.value
        out = np.empty(max(cap, 1), np.uint8)
        info = ViewInfo()
        if not L.pf_render_view_jpeg(self._h, pv, width, height, level, quality, out.ctypes.data, cap, C.byref(n), C.byref(info)):
            raise ValueError(L.pf_last_error().decode())
        return out[:n.value].tobytes(), info.as_dict()

    def view_of_extent(self, width, height):
        """V of the whole content fitted into width x height: axes as the map's, aspect kept, centred; None for a map without content"""
        V = np.zeros(9)
        return V.reshape(3, 3) if lib().pf_view_of_extent(self._h, width, height, V.ctypes.data_as(C.POINTER(C.c_double))) else None

    def view_from_pose(self, pose_world, camera=None):
        """V of what a camera at pose_world (7 doubles, camera-to-world) sees; camera: [w h fx fy cx cy], None = the camera of prepare().
        None for a pose feed() would reject as oblique"""
        _, pp = _pose(pose_world)
        pc = None
        if camera is not None:
            _, pc = _d(camera, 6)
        V = np.zeros(9)
        return V.reshape(3, 3) if lib().pf_view_from_pose(self._h, pp, pc, V.ctypes.data_as(C.POINTER(C.c_double))) else None

    def view_from_lnglat(self, gps_origin, lng_w, lat_n, lng_e, lat_s, width, height):
        """V of a north-up window linear in degrees, (lng_w, lat_n) at the view's top left corner and (lng_e, lat_s) at its bottom right,
        placed as webtiles() places the mosaic around gps_origin = (lng, lat, alt)"""
        _, g = _d(gps_origin, 3)
        V = np.zeros(9)
        ok = lib().pf_view_from_lnglat(self._h, g, float(lng_w), float(lat_n), float(lng_e), float(lat_s), width, height, V.ctypes.data_as(C.POINTER(C.c_double)))
        return V.reshape(3, 3) if ok else None

    def view_timing(self, on=None):
        """measurement hook: on=True/False switches the HIP events around a view's collapse, coverage pass and view kernel; on=None reads
        (collapse ms, coverage ms, view kernel ms, tiles collapsed) of the most recent view"""
        if on is not None:
            lib().pf_debug_view_timing(self._h, int(on)); return None
        o = np.zeros(4)
        lib().pf_debug_view_timing_read(self._h, o.ctypes.data_as(C.POINTER(C.c_double)))
        return tuple(o)

    # ---- Ele surface
    @property
    def num_levels(self):
        return lib().pf_num_levels(self._h)

    @property
    def dtype(self):
        return np.float32 if lib().pf_pyramid_type(self._h) == PF_32FC3 else np.int16

    def grid(self):
        dims = (C.c_int * 4)(); geo = (C.c_double * 6)()
        if not lib().pf_grid(self._h, dims, geo):
            return None
        return list(dims), list(geo)

    def tiles(self):
        n = lib().pf_tile_count(self._h)
        xy = (C.c_int * (2 * max(n, 1)))()
        lib().pf_tile_coords(self._h, xy, n)
        return [(xy[2 * i], xy[2 * i + 1]) for i in range(n)]

    def tile_level(self, ix, iy, level):
        s = ELE_PIXELS >> level
        lap = np.empty((s, s, 3), self.dtype); w = np.empty((s, s), np.float32)
        ok = lib().pf_get_tile_level(self._h, ix, iy, level, lap.ctypes.data, w.ctypes.data)
        return (lap, w) if ok else None

    def tile_bgra(self, ix, iy):
        out = np.empty((ELE_PIXELS, ELE_PIXELS, 4), np.uint8)
        return out if lib().pf_get_tile_bgra(self._h, ix, iy, out.ctypes.data) else None

    def blend_tile_raw(self, ix, iy):
        out = np.empty((ELE_PIXELS, ELE_PIXELS, 3), self.dtype)
        return out if lib().pf_blend_tile_raw(self._h, ix, iy, out.ctypes.data) else None

    def blend_tile(self, ix, iy):
        out = np.empty((ELE_PIXELS, ELE_PIXELS, 3), np.uint8)
        return out if lib().pf_blend_tile(self._h, ix, iy, out.ctypes.data) else None

    def map_update_command(self, ix, iy, gps_origin):
        """draw()'s "Map2DUpdate LastTexMat ..." text for tile (ix, iy), or None under the reference's gate
        `updated && !inborder` (MultiBandMap2DCPU.cpp:744); Fuse2Google is the caller's flag."""
        buf = C.create_string_buffer(256)
        g = (C.c_double * 3)(*[float(v) for v in gps_origin])
        n = lib().pf_map_update_command(self._h, ix, iy, g, buf, 256)
        return buf.value.decode() if n > 0 else None

    def blend_changed(self, cap=4096, out=None, level=0):
        """draw()'s texture refresh: ([(ix, iy)...], n x E x E x 3 uint8), E = 256 >> level (level=k: the tiles as views of pyramid
        level k, pf_blend_changed_level).  out: a caller-owned buffer of at least cap tiles (e.g. host_array(): page-locked, filled
        straight from HBM)."""
        e = ELE_PIXELS >> level if 0 <= level <= 8 else 1          # (a level the map refuses: nothing is written)
        xy = (C.c_int * (2 * cap))()
        if out is None:
            out = np.empty((cap, e, e, 3), np.uint8)
        if hasattr(lib(), "pf_blend_changed_level"):
            n = lib().pf_blend_changed_level(self._h, level, xy, out.ctypes.data, cap)
        elif level == 0:
            n = lib().pf_blend_changed(self._h, xy, out.ctypes.data, cap)
        else:
            raise RuntimeError("this build of the library has no level views")
        return [(xy[2 * i], xy[2 * i + 1]) for i in range(n)], out[:n]

    def blend_tiles(self, tiles, out=None, level=0):
        """Ele::blend + 8U view of the listed tiles (Ischanged untouched); tiles without pyramid keep out's bytes.  level=k: the views
        of pyramid level k, n x E x E x 3 with E = 256 >> k (pf_blend_tiles_level); None where the map has no such view."""
        n = len(tiles)
        e = ELE_PIXELS >> level if 0 <= level <= 8 else 1
        xy = (C.c_int * (2 * n))(*[v for t in tiles for v in t])
        if out is None:
            out = np.zeros((n, e, e, 3), np.uint8)
        if hasattr(lib(), "pf_blend_tiles_level"):
            ok = lib().pf_blend_tiles_level(self._h, xy, n, level, out.ctypes.data, None)
        elif level == 0:
            ok = lib().pf_blend_tiles(self._h, xy, n, out.ctypes.data)
        else:
            raise RuntimeError("this build of the library has no level views")
        return out[:n] if ok else None

    def blend_tiles_raw(self, tiles, level=0, out=None):
        """Ele::blend of the listed tiles in the pyramid type, before the 8U view: n x E x E x 3 of self.dtype, E = 256 >> level
        (a TypeCPU / TypeGPU map, level 0 only: n x 256 x 256 x 4 uint8, tile_bgra's).  Tiles without pyramid keep out's bytes."""
        n = len(tiles)
        e = ELE_PIXELS >> level if 0 <= level <= 8 else 1
        xy = (C.c_int * (2 * n))(*[v for t in tiles for v in t])
        if out is None:
            out = np.zeros((n, e, e, 4), np.uint8) if lib().pf_pyramid_type(self._h) == PF_8UC4 else np.zeros((n, e, e, 3), self.dtype)
        return out[:n] if lib().pf_blend_tiles_level(self._h, xy, n, level, None, out.ctypes.data) else None

    def blend_tiles_jpeg(self, tiles, quality=95, cap=None):
        """blend_tiles whose results leave as JPEG streams (256 x 256 each, encoded on the GPU from where the blend left them):
        a list of bytes, one per tile, empty for a tile without pyramid; None on failure.  cap: bytes of the buffer the
        streams are packed into (default: the bound for any content)."""
        n = len(tiles)
        xy = (C.c_int * (2 * n))(*[v for t in tiles for v in t])
        L = lib()
        if cap is None:
            b = C.c_size_t(0); one = np.zeros(3, np.uint8)
            L.pf_jpeg_encode_bgr(one.ctypes.data, ELE_PIXELS, ELE_PIXELS, 0, quality, None, 0, C.byref(b))
            cap = b.value * n
        out = np.empty(cap + 1, np.uint8); out[cap] = 0xA5
        off = (C.c_size_t * (n + 1))()
        if not L.pf_blend_tiles_jpeg(self._h, xy, n, quality, out.ctypes.data, cap, off):
            return None
        assert out[cap] == 0xA5
        return [out[off[i]:off[i + 1]].tobytes() for i in range(n)]

    # ---- multi-GPU seam exchange
    def halo_bytes(self, dx, dy):
        return int(lib().pf_halo_bytes(self._h, dx, dy))

    def halo_pack(self, ix, iy, dx, dy, dev_ptr):
        return bool(lib().pf_halo_pack(self._h, ix, iy, dx, dy, dev_ptr))

    def blend_tile_halo(self, ix, iy, halo_ptrs, raw=False):
        arr = (C.c_void_p * 9)(*[(p if p else None) for p in halo_ptrs])
        if raw:
            out = np.empty((ELE_PIXELS, ELE_PIXELS, 3), self.dtype)
            ok = lib().pf_blend_tile_halo(self._h, ix, iy, arr, None, out.ctypes.data)
        else:
            out = np.empty((ELE_PIXELS, ELE_PIXELS, 3), np.uint8)
            ok = lib().pf_blend_tile_halo(self._h, ix, iy, arr, out.ctypes.data, None)
        return out if ok else None

    def tile_bytes(self):
        return int(lib().pf_tile_bytes(self._h))

    def tile_export(self, ix, iy, dev_ptr):
        return bool(lib().pf_tile_export(self._h, ix, iy, dev_ptr))

    def tile_import(self, ix, iy, dev_ptr):
        return bool(lib().pf_tile_import(self._h, ix, iy, dev_ptr))

    # ---- merging maps, saving and resuming a map's state
    def merge(self, other):
        """other's tiles merged into this map's on the GPU (pf_merge): this map ends as the map fed its own keyframes and then other's,
        bit for bit; other is not modified.  False, with the reason in pf_last_error(), for maps that are not compatible."""
        return bool(lib().pf_merge(self._h, other._h))

    def merge_tiles(self, tiles, dev_ptrs, wlb=None):
        """pf_merge_tiles: the same merge from slot images in this device's memory (tile_export's; tile_bytes() each, 16-byte aligned),
        tiles = [(ix, iy)...], dev_ptrs their addresses; wlb: n x 16 float32 cull bounds of the exporting map, None: nothing known."""
        n = len(tiles)
        xy = (C.c_int * (2 * max(n, 1)))(*[v for t in tiles for v in t])
        ptrs = (C.c_void_p * max(n, 1))(*[int(p) for p in dev_ptrs])
        w = None
        if wlb is not None:
            keep = np.ascontiguousarray(wlb, dtype=np.float32).reshape(n, 16)
            w = keep.ctypes.data_as(C.POINTER(C.c_float))
        return bool(lib().pf_merge_tiles(self._h, n, xy, ptrs, w))

    def tile_bounds(self, ix, iy):
        """the 16 cull bounds of a tile (pf_tile_bounds): what merge_tiles takes as wlb beside tile_export's image; None: no such tile"""
        out = np.empty(16, np.float32)
        return out if lib().pf_tile_bounds(self._h, ix, iy, out.ctypes.data_as(C.POINTER(C.c_float))) else None

    def save_state(self, path):
        """the map's whole state into one file (pf_save_state); two saves of one state are the same bytes"""
        return bool(lib().pf_save_state(self._h, os.fsencode(path)))

    def load_state(self, path):
        """prepare from a state file (pf_load_state): this map, created with the file's options, becomes the map that wrote it"""
        return bool(lib().pf_load_state(self._h, os.fsencode(path)))

    def merge_state(self, path):
        """a state file merged into this prepared map as merge() would merge the map that wrote it (pf_merge_state)"""
        return bool(lib().pf_merge_state(self._h, os.fsencode(path)))

    def merge_stats(self, count_stores=-1):
        """diagnostics of the most recent merge (pf_debug_merge_stats): pairs, fresh pairs, ms between HIP events around the launches,
        pixel-levels the other map won (-1: not counted), slot bytes.  count_stores=True / False switches the counting for later merges."""
        o = (C.c_double * 6)()
        lib().pf_debug_merge_stats(self._h, int(count_stores), o)
        return {"pairs": int(o[0]), "fresh": int(o[1]), "ms": o[2], "won": int(o[3]), "slot_bytes": int(o[4])}

    # ---- measurement
    def profile_enable(self, mode=1):
        lib().pf_profile_enable(self._h, mode)

    def profile_reset(self):
        lib().pf_profile_reset(self._h)

    def profile_read(self):
        cap = 32
        names = (C.c_char_p * cap)(); ms = (C.c_double * cap)(); n = (C.c_longlong * cap)(); by = (C.c_double * cap)(); br = (C.c_double * cap)()
        if not hasattr(lib(), "pf_profile_read_run"):          # PF_LIB = an older build (A/B rounds)
            k = lib().pf_profile_read(self._h, cap, names, ms, n, by)
            return {names[i].decode(): {"ms": ms[i], "launches": n[i], "alg_bytes": by[i], "alg_bytes_run": by[i]} for i in range(k)}
        k = lib().pf_profile_read_run(self._h, cap, names, ms, n, by, br)
        # alg_bytes: SURVEY 8d's bytes for every tile of every canvas; alg_bytes_run: for the part of the canvases the launches' blocks processed
        return {names[i].decode(): {"ms": ms[i], "launches": n[i], "alg_bytes": by[i], "alg_bytes_run": br[i]} for i in range(k)}

    def reserve_tiles(self, n_tiles):
        """Allocator hint: HBM for n_tiles more tiles now (see pf_reserve_tiles)."""
        return bool(lib().pf_reserve_tiles(self._h, int(n_tiles)))

    def render_stats(self):
        o = (C.c_double * 4)()
        lib().pf_render_stats(self._h, o)
        return {"frames_with_pixels": int(o[0]), "level0_px": o[1], "owned_px": o[2], "tiles_held": int(o[3])}

    def timers(self):
        """host section timers under the reference's section names (pi::timer): {name: {calls, mean_s, min_s, max_s}}"""
        cap = 16
        names = (C.c_char_p * cap)(); calls = (C.c_longlong * cap)(); mean = (C.c_double * cap)(); mn = (C.c_double * cap)(); mx = (C.c_double * cap)()
        k = lib().pf_timer_read(self._h, cap, names, calls, mean, mn, mx)
        return {names[i].decode(): {"calls": calls[i], "mean_s": mean[i], "min_s": mn[i], "max_s": mx[i]} for i in range(k)}

    def timer_reset(self):
        lib().pf_timer_reset(self._h)

    def set_cull(self, on):
        """the cull of render_frame on / off (off: every tile of every canvas rendered, as the reference does; same mosaic)"""
        lib().pf_set_cull(self._h, 1 if on else 0)

    def next_homography(self, M0):
        """test hook of the experiments library (PF_LIB): the next accepted keyframe is warped with the 3 x 3 frame -> canvas matrix M0
        instead of the one its pose gives; one matrix per keyframe, in the order of the calls (pf_debug_next_homography)"""
        if not hasattr(lib(), "pf_debug_next_homography"):
            raise RuntimeError("pf_debug_next_homography: only the experiments library has it (PF_LIB=.../libpifusion_exp.so)")
        a = np.ascontiguousarray(M0, dtype=np.float64).reshape(9)
        lib().pf_debug_next_homography(self._h, a.ctypes.data_as(C.POINTER(C.c_double)))

    def debug_tile_store(self, slab_slots, fail_from=0, fail_count=0):
        """test hook of the experiments library (PF_LIB): tile slabs of slab_slots tiles from now on (0: the default size), and of the slabs
        asked for from this call on those numbered fail_from .. fail_from + fail_count - 1 are refused by hipMalloc (pf_debug_tile_store)"""
        if not hasattr(lib(), "pf_debug_tile_store"):
            raise RuntimeError("pf_debug_tile_store: only the experiments library has it (PF_LIB=.../libpifusion_exp.so)")
        lib().pf_debug_tile_store(self._h, int(slab_slots), int(fail_from), int(fail_count))

    def debug_fail_workspace(self, n):
        """test hook of the experiments library: the next n calls that size the frame workspace meet a hipMalloc that refuses"""
        if not hasattr(lib(), "pf_debug_fail_workspace"):
            raise RuntimeError("pf_debug_fail_workspace: only the experiments library has it (PF_LIB=.../libpifusion_exp.so)")
        lib().pf_debug_fail_workspace(self._h, int(n))

    def failed(self):
        """keyframes accepted and then lost to an allocation or launch failure (pf_stats_failed)"""
        n = C.c_longlong()
        lib().pf_stats_failed(self._h, None, None, None, C.byref(n))
        return n.value

    def render_log(self):
        """test hook: indices of the feed() calls whose keyframes were rendered, in render order (pf_debug_render_log)"""
        n = lib().pf_debug_render_log(self._h, None, 0)
        out = (C.c_longlong * max(n, 1))()
        k = lib().pf_debug_render_log(self._h, out, n)
        return [int(out[i]) for i in range(min(n, k))]

    def culled_tiles(self):
        """tiles left out of launches because the keyframe could not win the select anywhere in them (diagnostics)"""
        return int(lib().pf_debug_culled_tiles(self._h))

    def culled_cells(self):
        """64 x 64 cells switched off inside tiles that were rendered (diagnostics)"""
        return int(lib().pf_debug_culled_cells(self._h))

    def stats(self):
        a, b, c = C.c_longlong(), C.c_longlong(), C.c_longlong()
        lib().pf_stats(self._h, C.byref(a), C.byref(b), C.byref(c))
        return {"rendered": a.value, "rejected": b.value, "dropped": c.value}
