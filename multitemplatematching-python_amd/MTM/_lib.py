"""
ctypes binding of libmtm_hip.so (C ABI: include/mtm_hip.h).

There is NO CPU fallback: if the library cannot be loaded, or no GPU is visible when a context is
requested, the call fails loudly.  The oracle under oracle/ is test infrastructure and is never
imported from here.
"""
import ctypes
import struct
import os
import threading
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MTM_LIB_PATH: a differently built libmtm_hip.so (kernel timing experiments, tools/probes); never a fallback
LIB_PATH = os.environ.get("MTM_LIB_PATH") or os.path.join(_HERE, "libmtm_hip.so")

MTM_U8, MTM_F32, MTM_U16 = 0, 1, 2
GROUP_EXCHANGE_HOST, GROUP_EXCHANGE_RCCL = 0, 1
PEAKS_LOCAL, PEAKS_GLOBAL = 0, 1
BORDER_CONSTANT, BORDER_NEAREST = 0, 1
KERNEL_AUTO, KERNEL_NAIVE, KERNEL_DOT4, KERNEL_MFMA = 0, 1, 2, 3
OPT_KERNEL, OPT_PEAK_BORDER, OPT_HIT_CAPACITY, OPT_DOT4_VARIANT, OPT_EXACT_DIV, OPT_HITS_ONLY, OPT_F32_MFMA = 1, 2, 3, 4, 5, 6, 7
OPT_BATCH_MAX_ROWS = 8
OPT_BOXES_MAX_FLOATS = 9
ALL_OPTIONS = (OPT_KERNEL, OPT_PEAK_BORDER, OPT_HIT_CAPACITY, OPT_DOT4_VARIANT, OPT_EXACT_DIV, OPT_HITS_ONLY, OPT_F32_MFMA,
               OPT_BATCH_MAX_ROWS, OPT_BOXES_MAX_FLOATS)
BATCH_MAX_ROWS = 65535      # the default (and largest) MTM_OPT_BATCH_MAX_ROWS: stacked rows of one mtm_find_matches_batch chunk
POISON_SCRATCH, POISON_LDS, POISON_ARENAS = 1, 2, 4
E_OVERFLOW = -5
E_HIP = -2
COMM_ID_BYTES = 128
ABI_VERSION = 9


class MtmTempl(ctypes.Structure):
    _fields_ = [("px", ctypes.c_void_p), ("mask", ctypes.c_void_p),
                ("rows", ctypes.c_int32), ("cols", ctypes.c_int32),
                ("chans", ctypes.c_int32), ("dtype", ctypes.c_int32),
                ("row_stride", ctypes.c_int64), ("mask_row_stride", ctypes.c_int64)]


class MtmHit(ctypes.Structure):
    _fields_ = [("templ_idx", ctypes.c_int32), ("x", ctypes.c_int32), ("y", ctypes.c_int32),
                ("w", ctypes.c_int32), ("h", ctypes.c_int32), ("score", ctypes.c_float)]


class MtmTiming(ctypes.Structure):
    _fields_ = [("total_ms", ctypes.c_float), ("score_ms", ctypes.c_float),
                ("peaks_ms", ctypes.c_float), ("ncc_kernel_ms", ctypes.c_float),
                ("ncc_launches", ctypes.c_int32), ("kernel_used", ctypes.c_int32),
                ("n_hits", ctypes.c_int64), ("hits_only", ctypes.c_int32), ("sclk_mhz", ctypes.c_float),
                ("ncc_sum_ms", ctypes.c_float), ("f32_route", ctypes.c_int32),
                ("sq_launches", ctypes.c_int32), ("masked_stat_ms", ctypes.c_float),
                ("f32_pieces", ctypes.c_int32)]


HIT_DTYPE = np.dtype([("templ_idx", "<i4"), ("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4"),
                      ("score", "<f4")])
# mtm_box_unit: a template index and the region (y0, x0, rows, cols) it is searched in
BOX_UNIT_DTYPE = np.dtype([("templ_idx", "<i4"), ("y0", "<i4"), ("x0", "<i4"), ("rows", "<i4"), ("cols", "<i4")])
# mtm_point: a template index and the window (x, y) at the centre of a 3 x 3 neighbourhood (mtm_hit_neighbourhoods)
# one mtm_block of mtm_match_blocks: a block (x, y, w, h) of the reference image
BLOCK_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4")])
# one mtm_block_pass of mtm_match_blocks_passes: a grid of bw x bh blocks at stride (sx, sy), searched with `margin`
BLOCK_PASS_DTYPE = np.dtype([("bw", "<i4"), ("bh", "<i4"), ("sx", "<i4"), ("sy", "<i4"), ("margin", "<i4")])
POINT_DTYPE = np.dtype([("templ_idx", "<i4"), ("x", "<i4"), ("y", "<i4")])
assert HIT_DTYPE.itemsize == ctypes.sizeof(MtmHit) == 24
# mtm_templ as a numpy record: a whole template list is filled column-wise instead of field by field
TEMPL_DTYPE = np.dtype([("px", "<u8"), ("mask", "<u8"), ("rows", "<i4"), ("cols", "<i4"), ("chans", "<i4"),
                        ("dtype", "<i4"), ("row_stride", "<i8"), ("mask_row_stride", "<i8")])
assert TEMPL_DTYPE.itemsize == ctypes.sizeof(MtmTempl) == 48
# mtm_variant: one augmentation of a base template (mtm_set_templates_augmented)
VARIANT_DTYPE = np.dtype([("rot90", "<i4"), ("flip_lr", "<i4"), ("flip_ud", "<i4"), ("rows", "<i4"), ("cols", "<i4"),
                          ("down", "<i4")])

# mtm_debug_peak_pass: the routes of the peak pass, and its argument block (mtm_peak_pass)
PEAK_SCAN, PEAK_SCAN_BATCH, PEAK_SEGMENTS, PEAK_VERIFY_MAPS, PEAK_VERIFY_HASH, PEAK_EXTREMUM, PEAK_EXTREMUM_BATCH = range(7)
PEAK_INFO_FIELDS = ("grid_x", "grid_y", "grid_z", "list_cap", "n_lists", "verify_blocks", "hash_slots", "extremum_blocks")


class MtmPeakPass(ctypes.Structure):
    _fields_ = [("n_maps", ctypes.c_int32), ("route", ctypes.c_int32), ("mode_min", ctypes.c_int32), ("border", ctypes.c_int32),
                ("thr", ctypes.c_float), ("thr_q", ctypes.c_float),
                ("img_rows", ctypes.c_int32), ("holes", ctypes.c_int32), ("pattern_byte", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("hit_cap", ctypes.c_int64),
                ("dims", ctypes.c_void_p), ("maps", ctypes.c_void_p), ("flags", ctypes.c_void_p), ("cands", ctypes.c_void_p),
                ("n_cands", ctypes.c_int64), ("cand_count", ctypes.c_int64), ("cand_cap", ctypes.c_int64),
                ("records", ctypes.c_void_p), ("capacity", ctypes.c_int64), ("count", ctypes.c_void_p),
                ("raw", ctypes.c_void_p), ("trivial", ctypes.c_void_p), ("n_ints", ctypes.c_int64),
                ("keys", ctypes.c_void_p), ("ext_hits", ctypes.c_void_p), ("list_counts", ctypes.c_void_p),
                ("list_cap", ctypes.c_int64), ("info", ctypes.c_void_p)]


# mtm_debug_window_stats: the forms of the fused uint8 statistics kernel (output rows per work-group; numbered from 1) and the argument block (mtm_window_stats)
STATS_FORMS = (8, 4)
STATS_INFO_FIELDS = ("st_pitch", "blk_pitch", "pitch", "form", "grid_x", "grid_y", "n_cus", "kernel_ns")


class MtmWindowStats(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_int32), ("cols", ctypes.c_int32), ("h", ctypes.c_int32), ("w", ctypes.c_int32),
                ("num_type", ctypes.c_int32), ("form", ctypes.c_int32),
                ("tail_s", ctypes.c_int32), ("sb0", ctypes.c_int32), ("sb1", ctypes.c_int32), ("lay_r0", ctypes.c_int32),
                ("lay_r1", ctypes.c_int32), ("pattern_byte", ctypes.c_int32), ("zero_header", ctypes.c_int32),
                ("reserved", ctypes.c_int32),
                ("image", ctypes.c_void_p), ("t0", ctypes.c_void_p), ("sum2", ctypes.c_void_p), ("sq", ctypes.c_void_p),
                ("rsq", ctypes.c_void_p), ("blk", ctypes.c_void_p), ("blkq", ctypes.c_void_p), ("u8", ctypes.c_void_p),
                ("u8b", ctypes.c_void_p), ("header", ctypes.c_void_p), ("info", ctypes.c_void_p)]


# mtm_debug_window_stats_route: the kernel chains of csrc/mtm_stats_route.h (MTM_STATS_ROUTE_*), the bits of `want` and the
# argument block (mtm_window_stats_route)
STATS_ROUTES = ("U8", "U8MC", "U16", "U8_2P", "U8_2P_WIDE", "F64_LDS", "F64")
STATS_ROUTE_WANT = {"t": 1, "sum2": 2, "sq": 4, "blk": 8, "nulls": 16}
STATS_ROUTE_INFO_FIELDS = ("route", "st_pitch", "blk_pitch", "pitch", "grid1_x", "grid1_y", "grid1_z", "grid2_x", "grid2_y",
                           "hs_pitch", "lds_bytes", "kernel_ns")


class MtmWindowStatsRoute(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_int32), ("cols", ctypes.c_int32), ("chans", ctypes.c_int32), ("dtype", ctypes.c_int32),
                ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("num_type", ctypes.c_int32), ("route", ctypes.c_int32),
                ("want", ctypes.c_int32), ("sb0", ctypes.c_int32), ("sb1", ctypes.c_int32), ("lay_r0", ctypes.c_int32),
                ("lay_r1", ctypes.c_int32), ("pattern_byte", ctypes.c_int32),
                ("image", ctypes.c_void_p), ("t0", ctypes.c_void_p), ("t1", ctypes.c_void_p), ("t2", ctypes.c_void_p),
                ("t3", ctypes.c_void_p), ("sum2", ctypes.c_void_p), ("sq", ctypes.c_void_p), ("blk", ctypes.c_void_p),
                ("info", ctypes.c_void_p)]


# mtm_debug_maskf32_screen: the argument block (mtm_maskf32_screen) and the names of info[]
MASKF32_SCREEN_INFO_FIELDS = ("n_templ", "h", "w", "oh", "ow", "nyb", "nseg", "mb", "cap_production", "cap", "count", "rescored")
MASKF32_CANARY = 8          # records behind the list's capacity, filled with the byte 0xC5 before the listing pass


class MtmMaskF32Screen(ctypes.Structure):
    _fields_ = [("pieces", ctypes.c_int32), ("mode", ctypes.c_int32), ("rescore", ctypes.c_int32), ("set_cap", ctypes.c_int32),
                ("thr", ctypes.c_float), ("reserved", ctypes.c_int32),
                ("list_cap", ctypes.c_int64),
                ("n_templ", ctypes.c_int64), ("oh", ctypes.c_int64), ("ow", ctypes.c_int64), ("tiles", ctypes.c_int64),
                ("c1", ctypes.c_void_p), ("c2", ctypes.c_void_p), ("lb", ctypes.c_void_p), ("ub", ctypes.c_void_p),
                ("map_listed", ctypes.c_void_p), ("map_rescored", ctypes.c_void_p), ("mu_i", ctypes.c_void_p),
                ("mu_j", ctypes.c_void_p), ("records", ctypes.c_void_p), ("capacity", ctypes.c_int64),
                ("best", ctypes.c_void_p), ("info", ctypes.c_void_p)]


# every symbol include/mtm_hip.h declares: (restype, argtypes)
_P = ctypes.POINTER
SYMBOLS = {
    "mtm_abi_version": (ctypes.c_int, []),
    "mtm_device_count": (ctypes.c_int, []),
    "mtm_last_error": (ctypes.c_char_p, []),
    "mtm_ctx_create": (ctypes.c_int, [_P(ctypes.c_void_p), ctypes.c_int]),
    "mtm_ctx_destroy": (None, [ctypes.c_void_p]),
    "mtm_set_option": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64]),
    "mtm_get_option": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _P(ctypes.c_int64)]),
    "mtm_debug_poison": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    "mtm_debug_quotient_check": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, _P(ctypes.c_uint64)]),
    "mtm_debug_tail_split": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_double]),
    "mtm_debug_class_tilings": (ctypes.c_int, [ctypes.c_void_p, _P(ctypes.c_int32), ctypes.c_int]),
    "mtm_debug_tail_consts": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _P(ctypes.c_double), ctypes.c_int64]),
    "mtm_debug_templ_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_int, _P(ctypes.c_double)]),
    "mtm_debug_device_nms": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_int64,
                                            ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, _P(ctypes.c_int64),
                                            _P(ctypes.c_int64)]),
    "mtm_debug_peak_pass": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "mtm_debug_window_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "mtm_debug_window_stats_route": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "mtm_debug_maskf32_screen": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "mtm_set_image": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_int64]),
    "mtm_set_image_downscaled": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_int, ctypes.c_int64, ctypes.c_int]),
    "mtm_set_templates": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    "mtm_set_templates_augmented": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                   ctypes.c_int]),
    "mtm_score_map": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64]),
    "mtm_find_matches": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_void_p,
                                        ctypes.c_int64, _P(ctypes.c_int64)]),
    "mtm_find_matches_image": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_void_p,
                                              ctypes.c_int64, _P(ctypes.c_int64)]),
    "mtm_find_matches_image_nms": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                  ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_double, ctypes.c_int64,
                                                  ctypes.c_void_p, ctypes.c_int64, _P(ctypes.c_int64)]),
    "mtm_find_matches_image_sharded_nms": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                          ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_double,
                                                          ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                          ctypes.c_void_p, ctypes.c_int64, _P(ctypes.c_int64)]),
    "mtm_find_matches_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_double,
                                              ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, _P(ctypes.c_int64)]),
    "mtm_find_matches_pyramid": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                                ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                                _P(ctypes.c_int64)]),
    "mtm_find_matches_boxes": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_double, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                              _P(ctypes.c_int64)]),
    "mtm_track_boxes": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_double, ctypes.c_void_p]),
    "mtm_track_boxes_nbhd": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]),
    "mtm_track_boxes_adapt": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "mtm_track_boxes_reacquire": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                 ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int,
                                                 ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_void_p,
                                                 ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "mtm_track_boxes_sets": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                            ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "mtm_match_blocks": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "mtm_debug_plan_blocks": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                             ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                             _P(ctypes.c_int64), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "mtm_match_blocks_stack": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p]),
    "mtm_match_blocks_stack_at": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                 ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                 ctypes.c_void_p, ctypes.c_void_p]),
    "mtm_match_blocks_stack_passes": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                     ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int,
                                                     ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                     ctypes.c_void_p]),
    "mtm_debug_plane_peaks": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                             ctypes.c_void_p]),
    "mtm_debug_plan_blocks_stack": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                                   _P(ctypes.c_int64), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                   ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "mtm_match_blocks_at": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                           ctypes.c_void_p]),
    "mtm_match_blocks_passes": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                               ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "mtm_debug_plan_blocks_passes": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                    ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.c_int64, _P(ctypes.c_int64), ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "mtm_match_blocks_passes_validated": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                         ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                         ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                                         ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "mtm_debug_validate_blocks": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                 ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_void_p,
                                                 ctypes.c_void_p]),
    "mtm_match_blocks_second": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                               ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "mtm_match_blocks_masked": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                               ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                               ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p]),
    "mtm_match_blocks_passes_second": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                      ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                      ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                                      ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                      ctypes.c_int, ctypes.c_void_p]),
    "mtm_debug_second_peaks": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "mtm_deform_image": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    "mtm_match_blocks_passes_deformed": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                        ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                        ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                                        ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                        ctypes.c_void_p]),
    "mtm_match_blocks_passes_steered": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                       ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                       ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                                       ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                       ctypes.c_void_p, ctypes.c_int]),
    "mtm_deform_image_q8": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    "mtm_debug_steer_q8": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_void_p]),
    "mtm_hit_neighbourhoods": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "mtm_find_matches_next": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_void_p,
                                             ctypes.c_int64, _P(ctypes.c_int64), ctypes.c_void_p, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64]),
    "mtm_find_matches_async": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_double]),
    "mtm_find_matches_wait": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    "mtm_last_hits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, _P(ctypes.c_int64)]),
    "mtm_last_score_map": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64]),
    "mtm_get_timing": (ctypes.c_int, [ctypes.c_void_p, _P(MtmTiming)]),
    "mtm_nms": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_int,
                               ctypes.c_int64, ctypes.c_double, ctypes.c_void_p, _P(ctypes.c_int64)]),
    "mtm_nms_segments": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_int,
                                        ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]),
    "mtm_group_create": (ctypes.c_int, [_P(ctypes.c_void_p), _P(ctypes.c_int), ctypes.c_int]),
    "mtm_group_destroy": (None, [ctypes.c_void_p]),
    "mtm_group_size": (ctypes.c_int, [ctypes.c_void_p]),
    "mtm_group_ctx": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_int]),
    "mtm_group_set_option": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64]),
    "mtm_group_shards": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_void_p]),
    "mtm_group_find_matches": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                              ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_int64,
                                              _P(ctypes.c_int64)]),
    "mtm_group_find_matches_nms": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                  ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                                  ctypes.c_double, ctypes.c_double, ctypes.c_int64, ctypes.c_void_p,
                                                  ctypes.c_int64, _P(ctypes.c_int64)]),
    "mtm_group_last_hits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, _P(ctypes.c_int64)]),
    "mtm_group_comm_init": (ctypes.c_int, [ctypes.c_void_p]),
    "mtm_group_comm_ranks": (ctypes.c_int, [ctypes.c_void_p]),
    "mtm_group_set_exchange": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "mtm_group_exchange_used": (ctypes.c_int, [ctypes.c_void_p]),
    "mtm_host_alloc": (ctypes.c_void_p, [ctypes.c_size_t]),
    "mtm_host_free": (None, [ctypes.c_void_p]),
    "mtm_comm_unique_id": (ctypes.c_int, [ctypes.c_void_p]),
    "mtm_comm_init": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    "mtm_comm_allgather_hits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                               ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                               _P(ctypes.c_int64)]),
    "mtm_comm_last_gather": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                            _P(ctypes.c_int64)]),
    "mtm_comm_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "mtm_comm_init_all": (ctypes.c_int, [_P(ctypes.c_void_p), ctypes.c_int]),
    "mtm_comm_count": (ctypes.c_int, [ctypes.c_void_p]),
    "mtm_comm_allgather_hits_all": (ctypes.c_int, [_P(ctypes.c_void_p), ctypes.c_int, _P(ctypes.c_void_p), _P(ctypes.c_int64),
                                                   ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, _P(ctypes.c_int64)]),
}

_lib = None
_lib_lock = threading.Lock()


class MtmError(RuntimeError):
    """A libmtm_hip call failed (message from mtm_last_error)."""


def load():
    """Load libmtm_hip.so and declare every prototype.  Raises if the library is missing."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise MtmError(
                "libmtm_hip.so is not built (%s). Build it with "
                "`python multitemplatematching-python_amd/build.py` (needs hipcc); this package has "
                "no CPU fallback." % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)       # ctypes releases the GIL during every call
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)       # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        if lib.mtm_abi_version() != ABI_VERSION:
            raise MtmError("libmtm_hip.so ABI version mismatch")
        _lib = lib
        return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().mtm_last_error()
        raise MtmError("%s failed (%d): %s" % (what or "libmtm_hip call", rc, (msg or b"").decode()))


def _hits_call(fn, fetch, name, handle, *args, cap=4096, counts=None, tail=()):
    """fn(handle, *args, out, cap[, counts], &n, *tail) into a `cap`-record buffer: the hit records.  On E_OVERFLOW the
    result stays in the native object (counts are filled): it is fetched with fetch(handle, out, n, &n), not recomputed."""
    out = np.empty(cap, dtype=HIT_DTYPE)
    n = ctypes.c_int64(0)
    mid = () if counts is None else (counts.ctypes.data,)
    rc = fn(handle, *args, out.ctypes.data, cap, *mid, ctypes.byref(n), *tail)
    if rc == E_OVERFLOW:
        cap = int(n.value)
        out = np.empty(cap, dtype=HIT_DTYPE)
        rc = fetch(handle, out.ctypes.data, cap, ctypes.byref(n))
    check(rc, name)
    return out[:n.value]


def _pixel_rows(a):
    """Return (array_kept_alive, pointer, row_stride_bytes) for a (rows, cols[, C]) array whose
    rows have contiguous pixels; anything else (e.g. a transposed view) is copied."""
    ai = a.__array_interface__
    if ai["strides"] is None:           # C-contiguous (the usual case): one dictionary look-up, no checks needed
        shp = ai["shape"]
        return a, ai["data"][0], (shp[1] * shp[2] if len(shp) == 3 else shp[1]) * a.itemsize
    item = a.itemsize
    ok = a.strides[-1] == item and (a.ndim == 2 or a.strides[1] == a.shape[2] * item)
    if a.ndim == 3 and a.shape[2] == 1:
        ok = ok or a.strides[1] == item
    if not ok or a.strides[0] < a.shape[1] * (a.shape[2] if a.ndim == 3 else 1) * item or not a.flags.aligned:
        a = np.ascontiguousarray(a)
    return a, a.ctypes.data, a.strides[0]


def _dtype_code(a):
    if a.dtype == np.uint8:
        return MTM_U8
    if a.dtype == np.float32:
        return MTM_F32
    if a.dtype == np.uint16:
        return MTM_U16
    raise MtmError("libmtm_hip takes uint8, uint16 or float32 pixels (got %s)" % a.dtype)


_DT_CODES = {np.dtype(np.uint8): MTM_U8, np.dtype(np.float32): MTM_F32, np.dtype(np.uint16): MTM_U16}


_PACK_TEMPL = struct.Struct("<QQiiiiqq").pack_into      # one mtm_templ record (TEMPL_DTYPE)
_TYPESTR_CODES = {"|u1": MTM_U8, "<u2": MTM_U16, "<f4": MTM_F32}


def templ_records(templates):
    """[(template, mask or None), ...] (pixel policy already applied) -> (mtm_templ records, arrays kept alive).
    On the path of every call whose template objects are new (32 templates: 40 us; 78 us as field-wise numpy assignments)."""
    n = len(templates)
    buf = bytearray(48 * max(n, 1))
    keep = []
    off = 0
    for t, m in templates:
        ai = t.__array_interface__
        if ai["strides"] is None:           # C-contiguous (the usual case)
            shp = ai["shape"]
            tp = ai["data"][0]
            c = shp[2] if len(shp) == 3 else 1
            ts = shp[1] * c * t.itemsize
            code = _TYPESTR_CODES.get(ai["typestr"])
        else:
            t, tp, ts = _pixel_rows(t)
            shp = t.shape
            c = shp[2] if len(shp) == 3 else 1
            code = _DT_CODES.get(t.dtype)
        if code is None:
            raise MtmError("libmtm_hip takes uint8, uint16 or float32 pixels (got %s)" % t.dtype)
        keep.append(t)
        if m is not None:
            m, mp, mst = _pixel_rows(m)
            keep.append(m)
        else:
            mp = mst = 0
        _PACK_TEMPL(buf, off, tp, mp, shp[0], shp[1], c, code, ts, mst)
        off += 48
    return np.frombuffer(buf, dtype=TEMPL_DTYPE), keep


class FrozenUnits(list):
    """A list of (template, mask) units that its owner promises never to mutate (MTM._ListMemo)."""
    __slots__ = ()


def _zero_copy(templates, keep):
    """True if templ_records handed the caller's own buffers to the library (no array had to be copied)."""
    it = iter(keep)
    for t, m in templates:
        if next(it) is not t or (m is not None and next(it) is not m):
            return False
    return True


class _PinnedBlock:
    """Owner of one mtm_host_alloc block (freed with the last numpy view of it)."""

    def __init__(self, nbytes):
        lib = load()
        self.ptr = lib.mtm_host_alloc(int(nbytes))
        if not self.ptr:
            check(E_HIP, "mtm_host_alloc")
        self.nbytes = int(nbytes)
        self.__array_interface__ = {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.ptr, False), "version": 3}

    def __del__(self):
        ptr, self.ptr = getattr(self, "ptr", None), None
        if ptr and _lib is not None:
            _lib.mtm_host_free(ptr)


def pinned_empty(shape, dtype=np.uint8):
    """An uninitialised numpy array in page-locked host memory (mtm_host_alloc): images kept in such arrays are
    uploaded by plain DMA transfers, without the staging copy pageable memory needs."""
    dtype = np.dtype(dtype)
    shape = (int(shape),) if np.isscalar(shape) else tuple(int(v) for v in shape)
    n = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
    block = _PinnedBlock(max(n, 1))
    return np.asarray(block)[:n].view(dtype).reshape(shape)       # the views keep `block` alive


class _RecordMemo:
    """Marshalled template lists, memoised (shared by Context and Group)."""
    _rec_key = _rec = _rec_keep = _rec_src = None

    def _records(self, templates):
        """templ_records(templates), memoised on the identity (and shape) of the arrays: a caller that passes the same
        template objects call after call - the usual loop over images - pays for the marshalling once.  The arrays are
        kept referenced, so an id cannot be recycled; changed PIXELS are the library's business (it compares the bytes
        with the copy it packed from in every mtm_set_templates)."""
        # (a unit list MTM's own memo hands over again - never mutated, shapes re-checked by the caller in this very call)
        if type(templates) is FrozenUnits and templates is self._rec_src and self._rec_key is not None:
            return self._rec
        key = [(id(t), t.shape, id(m)) for t, m in templates]
        if key != self._rec_key:
            self._rec, keep = templ_records(templates)
            self._rec_keep = (keep, [t for t, _ in templates], [m for _, m in templates])
            # Only records that point at the caller's own buffers may be reused: a template that had to be copied
            # (np.rot90(base), base[:, ::-1], base.T ...) would otherwise be matched from the copy of the FIRST call
            # for ever, even after the caller edited the array in place - the reference re-reads it on every call.
            self._rec_key = key if _zero_copy(templates, keep) else None
        self._rec_src = templates
        return self._rec


_LIVE = weakref.WeakSet()          # contexts that exist right now (test support: live_contexts)


def live_contexts():
    return [c for c in list(_LIVE) if c._h]


# the fields of one mtm_debug_class_tilings record (MTM_CLASS_TILING_FIELDS of them)
CLASS_TILING_FIELDS = ("h", "w", "n_templates", "kernel", "rm_nt", "rm_R", "kp_nseg", "r2", "tail_ok", "tail_split", "n_slabs",
                       "slab_nt", "dot_variant")


# the doubles of one mtm_debug_tail_consts record (MTM_TAIL_CONST_FIELDS of them)
TAIL_CONST_FIELDS = ("k0", "k1", "d0", "d1", "g0", "g1", "valid_split")


def debug_tail_split(h, w, thr):
    """Test support (mtm_debug_tail_split; needs no GPU): the K steps after which the two-row score kernel of an h x w
    class screens its waves at the candidate threshold `thr`, 0 = unscreened."""
    return int(load().mtm_debug_tail_split(int(h), int(w), float(thr)))


# the doubles of one mtm_debug_templ_stats / mtm_track_boxes_adapt statistics record
TEMPL_STATS_FIELDS = ("mean0", "mean1", "mean2", "mean3", "templ_norm", "templ_sum2", "all_ones")


def block_records(blocks):
    """BLOCK_DTYPE records from such records or from an (N, 4) integer array of (x, y, w, h)."""
    b = np.asarray(blocks)
    if b.dtype == BLOCK_DTYPE:
        return np.ascontiguousarray(b)
    b = b.reshape(-1, 4)
    rec = np.empty(len(b), dtype=BLOCK_DTYPE)
    rec["x"], rec["y"], rec["w"], rec["h"] = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    return rec


def debug_plan_blocks(shape, chans, dtype, blocks, margin, budget_bytes):
    """The host plan of a mtm_match_blocks call for images of `shape` (rows, cols), no GPU needed (mtm_debug_plan_blocks):
    (tiles (n, 3) int32 of (block, ty0, tx0); chunk_of (N,) int32; toff (N,) int64; maps (N, 4) int32 of (x0, y0, ow, oh))."""
    lib = load()
    blocks = block_records(blocks)
    n = len(blocks)
    code = _DT_CODES[np.dtype(dtype)]
    n_tiles = ctypes.c_int64(0)
    chunk_of = np.zeros(n, dtype=np.int32)
    toff = np.zeros(n, dtype=np.int64)
    maps = np.zeros((n, 4), dtype=np.int32)
    args = (int(shape[0]), int(shape[1]), int(chans), code, blocks.ctypes.data, n, int(margin), int(budget_bytes))
    check(lib.mtm_debug_plan_blocks(*args, None, 0, ctypes.byref(n_tiles), chunk_of.ctypes.data, toff.ctypes.data,
                                    maps.ctypes.data), "mtm_debug_plan_blocks")
    tiles = np.zeros((n_tiles.value, 3), dtype=np.int32)
    check(lib.mtm_debug_plan_blocks(*args, tiles.ctypes.data, n_tiles.value, ctypes.byref(n_tiles), None, None, None),
          "mtm_debug_plan_blocks")
    return tiles, chunk_of, toff, maps


# mtm_match_blocks_stack: the reference of pair p is frames[p] / frames[0]
BLOCKS_REF_PREVIOUS, BLOCKS_REF_FIRST = 0, 1


def debug_plan_blocks_stack(n_frames, frames_per_chunk, mode, shape=None, chans=1, dtype=np.uint8, blocks=None, margin=0):
    """The host plan of a mtm_match_blocks_stack call, no GPU needed (mtm_debug_plan_blocks_stack): (chunks (n, 4) int32 of
    (f0, nf, carried, p0) - a chunk uploads the stack [frame carried, frames f0 .. f0 + nf - 1] and runs the pairs p0 ..
    p0 + nf - 1 -; clip (N, 2) int32 of every block's (ox, oy), how far its search box in frames of `shape` was clipped at
    the left and at the top, or None without blocks)."""
    lib = load()
    n_chunks = ctypes.c_int64(0)
    head = (int(n_frames), int(frames_per_chunk), int(mode))
    none = (1, 1, 1, MTM_U8, None, 0, 0, None)
    check(lib.mtm_debug_plan_blocks_stack(*head, None, 0, ctypes.byref(n_chunks), *none), "mtm_debug_plan_blocks_stack")
    chunks = np.zeros((n_chunks.value, 4), dtype=np.int32)
    clip, tail = None, none
    if blocks is not None:
        blocks = block_records(blocks)
        clip = np.zeros((len(blocks), 2), dtype=np.int32)
        tail = (int(shape[0]), int(shape[1]), int(chans), _DT_CODES[np.dtype(dtype)], blocks.ctypes.data, len(blocks),
                int(margin), clip.ctypes.data)
    check(lib.mtm_debug_plan_blocks_stack(*head, chunks.ctypes.data, n_chunks.value, ctypes.byref(n_chunks), *tail),
          "mtm_debug_plan_blocks_stack")
    return chunks, clip


def block_pass_records(passes):
    """BLOCK_PASS_DTYPE records from such records or from an (P, 5) integer array of (bw, bh, sx, sy, margin)."""
    a = np.asarray(passes)
    if a.dtype == BLOCK_PASS_DTYPE:
        return np.ascontiguousarray(a)
    a = a.reshape(-1, 5)
    rec = np.empty(len(a), dtype=BLOCK_PASS_DTYPE)
    for i, name in enumerate(BLOCK_PASS_DTYPE.names):
        rec[name] = a[:, i]
    return rec


def debug_plan_blocks_passes(shape, chans, dtype, passes, budget_bytes, coarse=None, at_pass=0):
    """The host plan of a mtm_match_blocks_passes call for images of `shape` (rows, cols), no GPU needed
    (mtm_debug_plan_blocks_passes): (counts (P,) int64, the blocks of every pass; tiles (n, 4) int32 of (pass, block, ty0,
    tx0), the fixed tile table; chunk_of int32, pass-major, every block's chunk within its pass).  With `coarse` - the
    positions (Nc, 2) of pass at_pass - 1's blocks - two more: pred (Nf, 2) int32, the (dx, dy) predicted for every block of
    pass `at_pass`, and maps (Nf, 4) int32 of (x0, y0, ow, oh), the units searched - the functions the kernel runs."""
    lib = load()
    passes = block_pass_records(passes)
    n_passes = len(passes)
    code = _DT_CODES[np.dtype(dtype)]
    head = (int(shape[0]), int(shape[1]), int(chans), code, passes.ctypes.data, n_passes, int(budget_bytes))
    counts = np.zeros(n_passes, dtype=np.int64)
    n_tiles = ctypes.c_int64(0)
    check(lib.mtm_debug_plan_blocks_passes(*head, counts.ctypes.data, None, 0, ctypes.byref(n_tiles), None, None, 0, None, None),
          "mtm_debug_plan_blocks_passes")
    tiles = np.zeros((n_tiles.value, 4), dtype=np.int32)
    chunk_of = np.zeros(int(counts.sum()), dtype=np.int32)
    rec = pred = maps = None
    if coarse is not None:
        pos = np.asarray(coarse, dtype=np.int64).reshape(-1, 2)
        if not 1 <= at_pass < n_passes or len(pos) != counts[at_pass - 1]:
            raise ValueError("debug_plan_blocks_passes: coarse needs one position per block of pass at_pass - 1")
        rec = np.zeros(len(pos), dtype=HIT_DTYPE)
        rec["x"], rec["y"] = pos[:, 0], pos[:, 1]
        pred = np.zeros((int(counts[at_pass]), 2), dtype=np.int32)
        maps = np.zeros((int(counts[at_pass]), 4), dtype=np.int32)
    check(lib.mtm_debug_plan_blocks_passes(*head, None, tiles.ctypes.data, n_tiles.value, ctypes.byref(n_tiles),
                                           chunk_of.ctypes.data, rec.ctypes.data if rec is not None else None, int(at_pass),
                                           pred.ctypes.data if rec is not None else None,
                                           maps.ctypes.data if rec is not None else None), "mtm_debug_plan_blocks_passes")
    return (counts, tiles, chunk_of) if coarse is None else (counts, tiles, chunk_of, pred, maps)


def debug_validate_blocks(positions, grid_shape, step, threshold=2.0, epsilon=0.5, context=None):
    """Test support (mtm_debug_validate_blocks): the median test of mtm_match_blocks_passes_validated over one grid of
    records.  `positions`: the (ny * nx, 2) integer (x, y) found for the blocks of a `grid_shape` = (ny, nx) grid in
    row-major order, block (iy, ix) at (ix * sx, iy * sy) with `step` = (sx, sy).  Returns (valid (N,) bool, steer (N, 2)
    int64): the flags and the positions that steer a next pass (an outlier's: block position + the neighbours' median
    displacement).  `context=None` runs the rule in the library's host code, no GPU needed; with a Context the records go
    through blocks_validate_kernel."""
    ny, nx = (int(v) for v in grid_shape)
    sx, sy = (int(v) for v in step)
    pos = np.asarray(positions).reshape(-1, 2)
    if len(pos) != nx * ny:
        raise ValueError("debug_validate_blocks: %d positions for a grid of %d x %d blocks" % (len(pos), ny, nx))
    rec = np.zeros(len(pos), dtype=HIT_DTYPE)
    rec["templ_idx"] = np.arange(len(pos))
    rec["x"], rec["y"] = pos[:, 0], pos[:, 1]
    valid = np.zeros(len(pos), dtype=np.uint8)
    steer = np.zeros(len(pos), dtype=HIT_DTYPE)
    lib = load() if context is None else context._lib
    check(lib.mtm_debug_validate_blocks(None if context is None else context._h, rec.ctypes.data, nx, ny, sx, sy,
                                        float(threshold), float(epsilon), valid.ctypes.data, steer.ctypes.data),
          "mtm_debug_validate_blocks")
    return valid.astype(bool), np.stack((steer["x"], steer["y"]), axis=1).astype(np.int64)


def deform_image(image, grid, displacements, context=None, q8=False):
    """The warp of mtm_deform_image: `image` (uint8 with 1 or 3 channels, or single-channel uint16) by the field of
    `displacements` - (N, 2) integers (dx, dy), each within +-2^22 - over the coarse `grid` = (bw, bh, sx, sy); the warped
    image, of the image's shape.  `context=None` runs the rule in the library's host code, no GPU needed; with a Context
    the image goes through deform_image_kernel.  `q8`: the displacements are in Q8, each within +-2^30
    (mtm_deform_image_q8)."""
    a, ptr, stride = _pixel_rows(image)
    chans = 1 if a.ndim == 2 else a.shape[2]
    d = np.ascontiguousarray(displacements, dtype=np.int32).reshape(-1, 2)
    out = np.empty(a.shape, dtype=a.dtype)
    lib = load() if context is None else context._lib
    name = "mtm_deform_image_q8" if q8 else "mtm_deform_image"
    check(getattr(lib, name)(None if context is None else context._h, ptr, stride, a.shape[0], a.shape[1], chans,
                             _dtype_code(a), *(int(v) for v in grid), d.ctypes.data, out.ctypes.data, out.strides[0]), name)
    return out


def debug_steer_q8(positions, nbhd, predicted, grid_shape, step, mode_min, smooth, valid=None, steer_positions=None,
                   context=None):
    """Test support (mtm_debug_steer_q8): the Q8 steering displacements of one pass of a steered call.  `positions`: the
    (ny * nx, 2) integer record positions of a `grid_shape` = (ny, nx) grid in row-major order, block (iy, ix) at (ix * sx,
    iy * sy) with `step` = (sx, sy); `nbhd`: (N, 3, 3) float32; `predicted`: (N, 2) integers, the pass's field in Q8;
    `valid` / `steer_positions`: both None, or the median test's flags and the (N, 2) positions that steer.  Returns (N, 2)
    int32: D8, or with `smooth` the filtered S8.  `context=None` runs the rule in the library's host code, no GPU needed;
    with a Context the records go through blocks_steer_q8_kernel and blocks_smooth_q8_kernel."""
    ny, nx = (int(v) for v in grid_shape)
    sx, sy = (int(v) for v in step)
    pos = np.asarray(positions).reshape(-1, 2)
    n = len(pos)
    nb = np.ascontiguousarray(nbhd, dtype=np.float32).reshape(-1, 9)
    pred = np.ascontiguousarray(predicted, dtype=np.int32).reshape(-1, 2)
    if n != nx * ny or len(nb) != n or len(pred) != n or (valid is None) != (steer_positions is None):
        raise ValueError("debug_steer_q8: one position, neighbourhood and field per block of the %d x %d grid" % (ny, nx))

    def records(p):
        rec = np.zeros(n, dtype=HIT_DTYPE)
        rec["templ_idx"] = np.arange(n)
        rec["x"], rec["y"] = p[:, 0], p[:, 1]
        return rec

    rec = records(pos)
    flags = steer = None
    if valid is not None:
        flags = np.ascontiguousarray(valid, dtype=np.uint8).reshape(n)
        steer = records(np.asarray(steer_positions).reshape(n, 2))
    out = np.zeros((n, 2), dtype=np.int32)
    lib = load() if context is None else context._lib
    check(lib.mtm_debug_steer_q8(None if context is None else context._h, rec.ctypes.data, nb.ctypes.data, pred.ctypes.data,
                                 None if flags is None else flags.ctypes.data, None if steer is None else steer.ctypes.data,
                                 nx, ny, sx, sy, int(mode_min), int(bool(smooth)), out.ctypes.data), "mtm_debug_steer_q8")
    return out


def debug_plane_peaks(acc, clip, oh, ow, pairs, method, context=None):
    """Test support (mtm_debug_plane_peaks): the means and peaks of constructed planes of sums.  `acc`: an (N, side, side)
    float64 array; block k's clipped box covers the cells oy <= cy < oy + oh[k], ox <= cx < ox + ow[k], (ox, oy) = clip[k].
    Returns (planes (N, side, side) float32 - (float)(acc / pairs) inside the box, NaN outside -, records: x = dx, y = dy
    of the peak, (-1, -1) and NaN for a plane without a number).  `context` None: the same rule on the host, no GPU."""
    a = np.ascontiguousarray(acc, dtype=np.float64)
    if a.ndim != 3 or a.shape[1] != a.shape[2]:
        raise ValueError("debug_plane_peaks: acc must be (N, side, side)")
    n, side = a.shape[0], a.shape[1]
    clip = np.ascontiguousarray(clip, dtype=np.int32).reshape(n, 2)
    oh = np.ascontiguousarray(oh, dtype=np.int32).reshape(n)
    ow = np.ascontiguousarray(ow, dtype=np.int32).reshape(n)
    planes = np.empty((n, side, side), dtype=np.float32)
    recs = np.zeros(n, dtype=HIT_DTYPE)
    lib = load() if context is None else context._lib
    check(lib.mtm_debug_plane_peaks(None if context is None else context._h, a.ctypes.data, n, side, clip.ctypes.data,
                                    oh.ctypes.data, ow.ctypes.data, int(pairs), int(method), planes.ctypes.data,
                                    recs.ctypes.data), "mtm_debug_plane_peaks")
    return planes, recs


def debug_second_peaks(planes, mode_min, exclusion, firsts=None, context=None):
    """Test support (mtm_debug_second_peaks): the second peaks of constructed maps.  `planes`: a sequence of 2-D float32
    maps (any sizes); `firsts`: the row-major index of every map's first peak, or None - the map's best cell.  Returns
    (positions (N, 2) int64 of (x, y) in the map's own coordinates, (-1, -1) where there is none; scores (N,) float32, NaN
    there).  `context=None` runs the rule in the library's host code, no GPU needed; with a Context the maps go through
    blocks_second_kernel, launched once over all of them."""
    maps = [np.ascontiguousarray(p, dtype=np.float32) for p in planes]
    if any(m.ndim != 2 for m in maps):
        raise ValueError("debug_second_peaks: every plane is a 2-D map")
    n = len(maps)
    oh = np.array([m.shape[0] for m in maps], dtype=np.int32)
    ow = np.array([m.shape[1] for m in maps], dtype=np.int32)
    flat = np.concatenate([m.reshape(-1) for m in maps]) if n else np.zeros(0, np.float32)
    at = None if firsts is None else np.ascontiguousarray(firsts, dtype=np.int32).reshape(n)
    out = np.zeros(n, dtype=HIT_DTYPE)
    lib = load() if context is None else context._lib
    check(lib.mtm_debug_second_peaks(None if context is None else context._h, flat.ctypes.data, n, oh.ctypes.data,
                                     ow.ctypes.data, None if at is None else at.ctypes.data, int(mode_min), int(exclusion),
                                     out.ctypes.data), "mtm_debug_second_peaks")
    return np.stack((out["x"], out["y"]), axis=1).astype(np.int64), out["score"].astype(np.float32)


def debug_templ_stats(template, method):
    """Test support (mtm_debug_templ_stats; needs no GPU): the constants mtm_set_templates computes for an unmasked
    template (H x W or H x W x C; uint8, uint16 or float32) under `method` - a float64 array of TEMPL_STATS_FIELDS."""
    a = np.ascontiguousarray(template)
    chans = 1 if a.ndim == 2 else a.shape[2]
    out = (ctypes.c_double * len(TEMPL_STATS_FIELDS))()
    check(load().mtm_debug_templ_stats(a.ctypes.data, a.shape[0], a.shape[1], chans, _dtype_code(a), int(method), out),
          "mtm_debug_templ_stats")
    return np.array(out[:], dtype=np.float64)


class Context(_RecordMemo):
    """One GPU context (single caller: guarded by a lock)."""

    def __init__(self, device=None):
        lib = load()
        if device is None:
            device = int(os.environ.get("MTM_DEVICE", os.environ.get("LOCAL_RANK", "0")))
            n = lib.mtm_device_count()
            if n > 0:
                device %= n
        h = ctypes.c_void_p()
        check(lib.mtm_ctx_create(ctypes.byref(h), int(device)), "mtm_ctx_create")
        self._lib = lib
        self._h = h
        self.device = device
        self.lock = threading.RLock()
        self._keep = []
        self._rec_key, self._rec, self._rec_keep = None, None, None
        _LIVE.add(self)
        k = os.environ.get("MTM_KERNEL")
        if k:
            self.set_option(OPT_KERNEL, {"auto": 0, "naive": 1, "dot4": 2, "mfma": 3}[k.lower()])
        b = os.environ.get("MTM_PEAK_BORDER")
        if b:
            self.set_option(OPT_PEAK_BORDER, {"constant": 0, "nearest": 1}[b.lower()])

    def close(self):
        _LIVE.discard(self)
        if self._h:
            self._lib.mtm_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    def set_option(self, opt, value):
        check(self._lib.mtm_set_option(self._h, int(opt), int(value)), "mtm_set_option")

    def get_option(self, opt):
        v = ctypes.c_int64(0)
        check(self._lib.mtm_get_option(self._h, int(opt), ctypes.byref(v)), "mtm_get_option")
        return int(v.value)

    def options(self):
        """{option: value} of every MTM_OPT_* option (what a fresh context starts with is `DEFAULT_OPTIONS` after the
        environment switches have been applied: compare with Context(...).options())."""
        return {o: self.get_option(o) for o in ALL_OPTIONS}

    def debug_poison(self, pattern=0xFF, what=7):
        """Test support (mtm_debug_poison): a byte pattern into every wave slot's scratch memory (1), every CU's LDS (2) and
        the context's per-call work buffers (4) - memory no result may depend on."""
        check(self._lib.mtm_debug_poison(self._h, int(pattern), int(what)), "mtm_debug_poison")

    def class_tilings(self):
        """Test support (mtm_debug_class_tilings): the tiling placement chose for every size class of the template set
        placed on the context, in placement order -> a list of dicts (CLASS_TILING_FIELDS; tail_split is the split of the
        class's last score launch, 0 = unscreened)."""
        nf = len(CLASS_TILING_FIELDS)
        n = self._lib.mtm_debug_class_tilings(self._h, None, 0)
        check(min(n, 0), "mtm_debug_class_tilings")
        buf = (ctypes.c_int32 * (nf * max(n, 1)))()
        check(min(self._lib.mtm_debug_class_tilings(self._h, buf, n), 0), "mtm_debug_class_tilings")
        return [dict(zip(CLASS_TILING_FIELDS, buf[k * nf:(k + 1) * nf])) for k in range(n)]

    def debug_tail_consts(self, split=0):
        """Test support (mtm_debug_tail_consts): the tail screen's constants of every template of the set placed on the
        context, as the device holds them -> an (n_templ, 7) float64 array of TAIL_CONST_FIELDS (k, d, g of the wave's first
        and second output row; valid_split: the split the context takes them to hold for).  split > 0 first re-derives them
        for that split (clamped to [6, h - 2]) in every class that can screen, as a search call with that split would;
        split == 0 launches nothing.  Templates of classes without a screen: NaN, valid_split -1."""
        nf = len(TAIL_CONST_FIELDS)
        n = sum(r["n_templates"] for r in self.class_tilings())
        out = np.zeros((n, nf), dtype=np.float64)
        check(self._lib.mtm_debug_tail_consts(self._h, int(split), out.ctypes.data_as(_P(ctypes.c_double)), out.size),
              "mtm_debug_tail_consts")
        return out

    def debug_quotient_check(self, n_cases=1 << 28, seed=1):
        """Test support (mtm_debug_quotient_check): the epilogue's division-free quotient against the IEEE division on
        n_cases operand triples -> dict(cases, mismatches, took_division, max_ulp_distance)."""
        out = (ctypes.c_uint64 * 4)()
        check(self._lib.mtm_debug_quotient_check(self._h, int(n_cases), int(seed), out), "mtm_debug_quotient_check")
        return {"cases": int(out[0]), "mismatches": int(out[1]), "took_division": int(out[2]), "max_ulp_distance": int(out[3])}

    def debug_device_nms(self, hits, rows, cols, max_side, score_threshold, max_overlap, ascending=False, n_min=0,
                         n_max=1 << 18, out=None):
        """Test support (mtm_debug_device_nms): the device's share of the suppression - counting sort by grid cell, champion
        pass, prune pass - on the hit list `hits`, on the grid of a rows x cols image with boxes of at most max_side a side
        -> (champions, undecided): the hits kept for certain and the ones the host's pass still has to decide about (views
        of `out`, a HIT_DTYPE array of at least len(hits) records, when one is given).  A list shorter than n_min or longer
        than n_max returns two empty arrays and leaves `out` as it is."""
        hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        n = len(hits)
        if out is None:
            out = np.empty(max(n, 1), dtype=HIT_DTYPE)
        assert out.dtype == HIT_DTYPE and out.flags.c_contiguous
        nc, nu = ctypes.c_int64(0), ctypes.c_int64(0)
        check(self._lib.mtm_debug_device_nms(self._h, hits.ctypes.data, n, int(rows), int(cols), int(max_side),
                                             float(score_threshold), int(bool(ascending)), float(max_overlap), int(n_min),
                                             int(n_max), out.ctypes.data, len(out), ctypes.byref(nc), ctypes.byref(nu)),
              "mtm_debug_device_nms")
        return out[:nc.value], out[nc.value:nc.value + nu.value]

    def debug_peak_pass(self, maps, route, thr, mode_min=False, border=BORDER_NEAREST, hit_cap=4096, templ_hw=None, img_rows=0,
                        flags=None, holes=False, cands=None, cand_count=None, cand_cap=None, thr_q=None, pattern=0xFF,
                        records=None):
        """Test support (mtm_debug_peak_pass): the peak pass of the search calls - the kernels of `route` (PEAK_*), with the
        grids and capacities the search call derives - on the float32 score maps `maps` (a list of 2-D arrays; templ_hw: the
        (h, w) of each map's template, (1, 1) by default).  flags (PEAK_SEGMENTS): uint8 [map][row][strip column of 256],
        padded to the largest map.  cands (the verify routes): HIT_DTYPE records, cand_count the length the device counter
        holds (len(cands) by default), cand_cap the list's capacity (max(len, 1) by default), thr_q the quality a hit exceeds
        (the threshold's by default).  records: a HIT_DTYPE array of at least hit_cap records that the device's list starts
        from (what the kernels do not write stays) - it comes back as 'records'.
        -> dict(records, count, raw, trivial, keys, ext_hits, list_counts, info); raw / trivial / keys are per (image, map) for
        the batch routes."""
        maps = [np.ascontiguousarray(m, dtype=np.float32) for m in maps]
        n = len(maps)
        assert n >= 1 and all(m.ndim == 2 for m in maps)
        templ_hw = [(1, 1)] * n if templ_hw is None else list(templ_hw)
        dims = np.array([[m.shape[0], m.shape[1], hw[0], hw[1]] for m, hw in zip(maps, templ_hw)], dtype=np.int32)
        packed = np.concatenate([m.ravel() for m in maps])
        batch = route in (PEAK_SCAN_BATCH, PEAK_EXTREMUM_BATCH)
        n_img = (int(dims[0, 0]) + int(dims[0, 2]) - 1) // int(img_rows) if batch and img_rows > 0 else 1
        n_ints = n * max(n_img, 1)
        max_oh, max_ow = int(dims[:, 0].max()), int(dims[:, 1].max())
        n_sx = (max_ow + 255) // 256
        a = MtmPeakPass()
        a.n_maps, a.route, a.mode_min, a.border = n, int(route), int(bool(mode_min)), int(border)
        a.thr = float(thr)
        a.thr_q = float(thr_q) if thr_q is not None else float(np.float32(-np.float32(thr)) if mode_min else np.float32(thr))
        a.img_rows, a.holes, a.pattern_byte, a.hit_cap = int(img_rows), int(bool(holes)), int(pattern), int(hit_cap)
        a.dims, a.maps = dims.ctypes.data, packed.ctypes.data
        if flags is not None:
            flags = np.ascontiguousarray(flags, dtype=np.uint8)
            assert flags.shape == (n, max_oh, n_sx), (flags.shape, (n, max_oh, n_sx))
            a.flags = flags.ctypes.data
        if cands is not None:
            cands = np.ascontiguousarray(cands, dtype=HIT_DTYPE)
            a.cands = cands.ctypes.data if len(cands) else None
            a.n_cands = len(cands)
            a.cand_count = len(cands) if cand_count is None else int(cand_count)
            a.cand_cap = max(len(cands), 1) if cand_cap is None else int(cand_cap)
        if records is None:
            records = np.zeros(int(hit_cap), dtype=HIT_DTYPE)
        assert records.dtype == HIT_DTYPE and records.flags.c_contiguous and records.flags.writeable
        count = np.zeros(1, dtype=np.uint64)
        raw, trivial = np.zeros(n_ints, dtype=np.int32), np.zeros(n_ints, dtype=np.int32)
        keys, ext_hits = np.zeros(2 * n_ints, dtype=np.uint64), np.zeros(2 * n_ints, dtype=HIT_DTYPE)
        list_counts = np.zeros(n * n_sx, dtype=np.uint64)
        info = np.zeros(8, dtype=np.int64)
        a.records, a.capacity, a.count = records.ctypes.data, len(records), count.ctypes.data
        a.raw, a.trivial, a.n_ints = raw.ctypes.data, trivial.ctypes.data, n_ints
        a.keys, a.ext_hits = keys.ctypes.data, ext_hits.ctypes.data
        a.list_counts, a.list_cap, a.info = list_counts.ctypes.data, len(list_counts), info.ctypes.data
        check(self._lib.mtm_debug_peak_pass(self._h, ctypes.byref(a)), "mtm_debug_peak_pass")
        shape = (n_img, n) if batch else (n,)
        return {"records": records, "count": int(count[0]), "raw": raw.reshape(shape), "trivial": trivial.reshape(shape),
                "keys": keys.reshape(shape + (2,)), "ext_hits": ext_hits.reshape(shape + (2,)), "list_counts": list_counts,
                "info": dict(zip(PEAK_INFO_FIELDS, (int(v) for v in info)))}

    def debug_window_stats(self, image, h, w, num_type, form=0, planes=("t0", "sum2", "sq", "rsq", "blk"), tail_s=0, units=None,
                           convert_rows=None, zero_header=True, pattern=0xA5):
        """Test support (mtm_debug_window_stats): the fused window statistics of single-channel uint8 images on the 2-D uint8
        array `image`, window h x w, num_type 0 / 1 / 2, launched the way the search calls launch them - in form `form` (1 ..
        len(STATS_FORMS); 0: the launcher's choice).  planes: which of t0, sum2, sq, rsq, blk the kernel is asked for (tail_s
        > 0 adds blkq, the tail boxes of that split); units: the (first, end) range of 8-row units, all by default;
        convert_rows: (r0, r1) image rows the launch converts from the raw copy on the way.  Every buffer starts out as the
        byte `pattern`.
        -> dict: the wanted planes ((oh, st_pitch) float64; blk / blkq (oh, blk_pitch, 4)), u8 / u8b ((rows, pitch) uint8),
        header (2 uint64), info (STATS_INFO_FIELDS)."""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        assert image.ndim == 2
        rows, cols = image.shape
        oh, ow = rows - h + 1, cols - w + 1
        st_pitch = (ow + 3) // 4 * 4
        blk_pitch = (st_pitch + 15) // 16
        pitch = (cols + 512 + 63) // 64 * 64
        a = MtmWindowStats()
        a.rows, a.cols, a.h, a.w, a.num_type, a.form = rows, cols, int(h), int(w), int(num_type), int(form)
        a.tail_s, a.pattern_byte, a.zero_header = int(tail_s), int(pattern), int(bool(zero_header))
        a.sb0, a.sb1 = (0, -1) if units is None else (int(units[0]), int(units[1]))
        a.lay_r0, a.lay_r1 = (0, 0) if convert_rows is None else (int(convert_rows[0]), int(convert_rows[1]))
        a.image = image.ctypes.data
        out = {}
        for name in tuple(planes) + (("blkq",) if tail_s else ()):
            shape = (max(oh, 0), blk_pitch, 4) if name in ("blk", "blkq") else (max(oh, 0), st_pitch)
            out[name] = np.zeros(shape, dtype=np.float64)
            setattr(a, name, out[name].ctypes.data)
        out["u8"], out["u8b"] = np.zeros((rows, pitch), dtype=np.uint8), np.zeros((rows, pitch), dtype=np.uint8)
        out["header"] = np.zeros(2, dtype=np.uint64)
        info = np.zeros(8, dtype=np.int64)
        a.u8, a.u8b, a.header, a.info = out["u8"].ctypes.data, out["u8b"].ctypes.data, out["header"].ctypes.data, info.ctypes.data
        check(self._lib.mtm_debug_window_stats(self._h, ctypes.byref(a)), "mtm_debug_window_stats")
        out["info"] = dict(zip(STATS_INFO_FIELDS, (int(v) for v in info)))
        assert (out["info"]["st_pitch"], out["info"]["blk_pitch"], out["info"]["pitch"]) == (st_pitch, blk_pitch, pitch)
        return out

    def debug_window_stats_route(self, image, h, w, num_type, route=0, want=("t", "sum2", "sq"), units=None, rows_in=None,
                                 pattern=0xA5):
        """Test support (mtm_debug_window_stats_route): the window statistics of `image` ((rows, cols) or (rows, cols, chans);
        uint8, uint16 or float32) on one of the kernel chains of STATS_ROUTES - route 0: the one the library's rule gives
        it, else its index, forced.  want: which of t, sum2, sq, blk the kernels are asked for ("nulls": planes not wanted
        are handed over as NULL); units: the (first, end) range of 8-row units (U16, or F64_LDS with rows_in: the (r0, r1)
        image rows whose row sums the launch makes).  Every buffer starts out as the byte `pattern`.
        -> dict: t (chans planes), sum2, sq ((oh, st_pitch) float64), blk ((oh, blk_pitch, 4)) - all of them, wanted or not -
        and info (STATS_ROUTE_INFO_FIELDS)."""
        image = np.ascontiguousarray(image)
        code = _dtype_code(image)
        assert image.ndim in (2, 3)
        rows, cols = image.shape[:2]
        chans = 1 if image.ndim == 2 else image.shape[2]
        oh, ow = rows - h + 1, cols - w + 1
        st_pitch = (ow + 3) // 4 * 4
        blk_pitch = (st_pitch + 15) // 16
        a = MtmWindowStatsRoute()
        a.rows, a.cols, a.chans, a.dtype, a.h, a.w = rows, cols, chans, code, int(h), int(w)
        a.num_type, a.route, a.pattern_byte = int(num_type), int(route), int(pattern)
        a.want = sum(STATS_ROUTE_WANT[k] for k in want)
        a.sb0, a.sb1 = (0, -1) if units is None else (int(units[0]), int(units[1]))
        a.lay_r0, a.lay_r1 = (0, 0) if rows_in is None else (int(rows_in[0]), int(rows_in[1]))
        a.image = image.ctypes.data
        out = {"t": np.zeros((4, max(oh, 0), max(st_pitch, 0)), dtype=np.float64)}
        for k in range(4):
            setattr(a, "t%d" % k, out["t"][k].ctypes.data)
        for name in ("sum2", "sq", "blk"):
            shape = (max(oh, 0), max(blk_pitch, 0), 4) if name == "blk" else (max(oh, 0), max(st_pitch, 0))
            out[name] = np.zeros(shape, dtype=np.float64)
            setattr(a, name, out[name].ctypes.data)
        info = np.zeros(len(STATS_ROUTE_INFO_FIELDS), dtype=np.int64)
        a.info = info.ctypes.data
        check(self._lib.mtm_debug_window_stats_route(self._h, ctypes.byref(a)), "mtm_debug_window_stats_route")
        out["info"] = dict(zip(STATS_ROUTE_INFO_FIELDS, (int(v) for v in info)))
        assert (out["info"]["st_pitch"], out["info"]["blk_pitch"]) == (st_pitch, blk_pitch)
        return out

    def debug_maskf32_screen(self, n_templ, out_shape, pieces, mode, thr=0.0, rescore=True, list_cap=0):
        """Test support (mtm_debug_maskf32_screen): the screen of the context's ONE masked float32 size class (after set_image
        and set_templates), stage by stage: `pieces` piece products in the two raw launches, the listing pass of `mode`
        (PEAKS_LOCAL against the score threshold `thr`, PEAKS_GLOBAL against the templates' best lower bounds), the exact
        re-scoring; list_cap: 0 = a search call's capacity of the list, else a smaller one.
        -> dict: c1, c2 (float32), lb, ub (float64), map_listed, map_rescored (float32): (n_templ, oh, ow); mu_i, mu_j
        (nyb, nseg) float32; records (HIT_DTYPE: what was written), canary (the bytes of the 8 records behind the list's
        capacity, set to 0xC5 before the listing pass), best (uint32 keys, PEAKS_GLOBAL) and info
        (MASKF32_SCREEN_INFO_FIELDS)."""
        oh, ow = int(out_shape[0]), int(out_shape[1])
        n = int(n_templ)
        a = MtmMaskF32Screen()
        a.pieces, a.mode, a.rescore, a.set_cap = int(pieces), int(mode), 1 if rescore else 0, 0
        a.thr, a.list_cap = float(thr), int(list_cap)
        a.n_templ, a.oh, a.ow = n, oh, ow
        nyb, nseg = (oh + 3) // 4, (ow + 127) // 128
        a.tiles = nyb * nseg
        out = {}
        for name, dt in (("c1", np.float32), ("c2", np.float32), ("lb", np.float64), ("ub", np.float64),
                         ("map_listed", np.float32), ("map_rescored", np.float32)):
            out[name] = np.zeros((n, oh, ow), dtype=dt)
            setattr(a, name, out[name].ctypes.data)
        for name in ("mu_i", "mu_j"):
            out[name] = np.zeros((nyb, nseg), dtype=np.float32)
            setattr(a, name, out[name].ctypes.data)
        rec = np.zeros(n * oh * ow + MASKF32_CANARY, dtype=HIT_DTYPE)
        a.records, a.capacity = rec.ctypes.data, len(rec)
        out["best"] = np.zeros(n, dtype=np.uint32)
        a.best = out["best"].ctypes.data
        info = np.zeros(len(MASKF32_SCREEN_INFO_FIELDS), dtype=np.int64)
        a.info = info.ctypes.data
        check(self._lib.mtm_debug_maskf32_screen(self._h, ctypes.byref(a)), "mtm_debug_maskf32_screen")
        out["info"] = dict(zip(MASKF32_SCREEN_INFO_FIELDS, (int(v) for v in info)))
        assert (out["info"]["nyb"], out["info"]["nseg"]) == (nyb, nseg), out["info"]
        n_rec = min(out["info"]["count"], out["info"]["cap"])
        out["records"] = rec[:n_rec].copy()
        out["canary"] = rec[n_rec:n_rec + MASKF32_CANARY].view(np.uint8).copy()
        return out

    def debug_maskf32_list_cap(self, list_cap):
        """Test support: the capacity the NEXT search calls of this context give the masked float32 screen's list (0: their
        own again) - what shows the ladder one piece product -> three -> the float64 kernel on a small map."""
        a = MtmMaskF32Screen()
        a.set_cap, a.list_cap = 1, int(list_cap)
        check(self._lib.mtm_debug_maskf32_screen(self._h, ctypes.byref(a)), "mtm_debug_maskf32_screen")

    def set_image(self, image, downscale=1):
        """Upload the search image; `downscale` > 1 area-averages it by that integer factor on the
        device (mtm_set_image_downscaled)."""
        a, ptr, stride = _pixel_rows(image)
        chans = 1 if a.ndim == 2 else a.shape[2]
        check(self._lib.mtm_set_image_downscaled(self._h, ptr, a.shape[0], a.shape[1], chans, _dtype_code(a), stride,
                                                 int(downscale)), "mtm_set_image")


    def set_templates(self, templates, method):
        """templates: list of (array, mask_or_None) with identical dtype policy already applied."""
        rec = self._records(templates)
        check(self._lib.mtm_set_templates(self._h, rec.ctypes.data, len(templates), int(method)), "mtm_set_templates")

    def set_templates_augmented(self, bases, variants, method):
        """bases: list of (uint8 array, uint8 mask or None); variants: VARIANT_DTYPE records.  Units are
        base-major: unit index = base * len(variants) + variant (mtm_set_templates_augmented)."""
        rec, keep = templ_records(bases)
        var = np.ascontiguousarray(variants, dtype=VARIANT_DTYPE)
        check(self._lib.mtm_set_templates_augmented(self._h, rec.ctypes.data, len(bases), var.ctypes.data, len(var),
                                                    int(method)), "mtm_set_templates_augmented")

    def search(self, templates, image, method, mode, score_threshold):
        """One search = templates + image in, hit records out (the engine interface shared with Group)."""
        self.set_templates(templates, method)
        return self.find_matches_image(image, mode, score_threshold)

    def score_map(self, idx, shape):
        out = np.empty(shape, dtype=np.float32)
        check(self._lib.mtm_score_map(self._h, int(idx), out.ctypes.data, out.strides[0]), "mtm_score_map")
        return out

    def find_matches(self, mode, score_threshold, next_image=None):
        """Hits of the current image.  With `next_image`, that image is uploaded while the kernels run
        and is the current image when the call returns (mtm_find_matches_next)."""
        if next_image is None:
            return _hits_call(self._lib.mtm_find_matches, self._lib.mtm_last_hits, "mtm_find_matches", self._h, int(mode),
                              float(score_threshold))
        a, ptr, stride = _pixel_rows(next_image)
        chans = 1 if a.ndim == 2 else a.shape[2]
        next_args = (ptr, a.shape[0], a.shape[1], chans, _dtype_code(a), stride)
        return _hits_call(self._lib.mtm_find_matches_next, self._lib.mtm_last_hits, "mtm_find_matches", self._h, int(mode),
                          float(score_threshold), tail=next_args)

    def find_matches_image(self, image, mode, score_threshold):
        """set_image + find_matches in one native call (mtm_find_matches_image): no round trip in between, the
        image crosses PCIe in row bands under the score kernel where the layout allows."""
        a, ptr, stride = _pixel_rows(image)
        chans = 1 if a.ndim == 2 else a.shape[2]
        return _hits_call(self._lib.mtm_find_matches_image, self._lib.mtm_last_hits, "mtm_find_matches_image", self._h, ptr,
                          a.shape[0], a.shape[1], chans, _dtype_code(a), stride, int(mode), float(score_threshold))

    def find_matches_pyramid(self, image, factor, mode, coarse_threshold, score_threshold, radius, max_candidates):
        """Coarse-to-fine search of the current templates in one native call (mtm_find_matches_pyramid): candidates from
        the image downscaled by `factor`, exact full-resolution scores in windows of +-`radius` around them."""
        a, ptr, stride = _pixel_rows(image)
        chans = 1 if a.ndim == 2 else a.shape[2]
        return _hits_call(self._lib.mtm_find_matches_pyramid, self._lib.mtm_last_hits, "mtm_find_matches_pyramid", self._h,
                          ptr, a.shape[0], a.shape[1], chans, _dtype_code(a), stride, int(factor), int(mode),
                          float(coarse_threshold), float(score_threshold), int(radius), int(max_candidates))

    def find_matches_boxes(self, image, units, mode, score_threshold):
        """The current templates searched in many regions of one image in one native call (mtm_find_matches_boxes).
        `units`: BOX_UNIT_DTYPE records.  Returns (hits, counts): the records grouped by unit (full-image coordinates,
        templ_idx = the unit's template) and the number of records of each unit."""
        a, ptr, stride = _pixel_rows(image)
        chans = 1 if a.ndim == 2 else a.shape[2]
        units = np.ascontiguousarray(units, dtype=BOX_UNIT_DTYPE)
        n = len(units)
        counts = np.zeros(n, dtype=np.int64)
        hits = _hits_call(self._lib.mtm_find_matches_boxes, self._lib.mtm_last_hits, "mtm_find_matches_boxes", self._h,
                          ptr, a.shape[0], a.shape[1], chans, _dtype_code(a), stride, units.ctypes.data, n, int(mode),
                          float(score_threshold), cap=max(4096, 16 * n), counts=counts)
        return hits, counts

    def track_boxes(self, frames, units, margin, min_score=None):
        """The current templates tracked through frames of one shape and dtype in one native call (mtm_track_boxes).
        `units`: BOX_UNIT_DTYPE records, each track's template and frame-0 region.  Returns the len(frames) * len(units)
        records, frame-major (frame coordinates, templ_idx = the track's template)."""
        return self._track_boxes(frames, units, margin, min_score, False)[0]

    def track_boxes_nbhd(self, frames, units, margin, min_score=None):
        """track_boxes with every record's 3 x 3 score neighbourhood in its own frame's map, in the same native call
        (mtm_track_boxes_nbhd): (records, (len(frames) * len(units), 3, 3) float32 array, element [i, 1 + dy, 1 + dx] the
        score at window (x + dx, y + dy) of record i, NaN outside the map) - hit_neighbourhoods of each frame's records."""
        return self._track_boxes(frames, units, margin, min_score, True)

    def _track_boxes(self, frames, units, margin, min_score, with_nbhd):
        n, nt = len(frames), len(units)
        if n == 0 or nt == 0:
            return np.zeros(0, dtype=HIT_DTYPE), (np.zeros((0, 3, 3), dtype=np.float32) if with_nbhd else None)
        rows = [_pixel_rows(a) for a in frames]
        if len({r[2] for r in rows}) > 1:       # (one row stride for every frame)
            rows = [_pixel_rows(np.ascontiguousarray(a)) for a in frames]
        a0, _, stride = rows[0]
        chans = 1 if a0.ndim == 2 else a0.shape[2]
        ptrs = (ctypes.c_void_p * n)(*[r[1] for r in rows])
        units = np.ascontiguousarray(units, dtype=BOX_UNIT_DTYPE)
        out = np.empty(n * nt, dtype=HIT_DTYPE)
        use_min = min_score is not None
        args = (self._h, ptrs, n, a0.shape[0], a0.shape[1], chans, _dtype_code(a0), stride, units.ctypes.data, nt,
                int(margin), int(use_min), float(min_score) if use_min else 0.0, out.ctypes.data)
        if not with_nbhd:
            check(self._lib.mtm_track_boxes(*args), "mtm_track_boxes")
            return out, None
        nbhd = np.empty((n * nt, 3, 3), dtype=np.float32)
        check(self._lib.mtm_track_boxes_nbhd(*args, nbhd.ctypes.data), "mtm_track_boxes_nbhd")
        return out, nbhd

    def track_boxes_adapt(self, frames, units, margin, min_score, blend_a, templates, with_nbhd=False):
        """track_boxes / track_boxes_nbhd with a template per track that is blended with each passing hit's window
        (mtm_track_boxes_adapt; the window's weight is blend_a / 256).  `templates`: the pixel arrays of the current
        templates, in their order (for the shapes of the result).  Returns (records, neighbourhoods or None, every
        track's template after the last frame, (len(units), 7) float64 array of their TEMPL_STATS_FIELDS)."""
        return self._track_boxes_adapt("mtm_track_boxes_adapt", frames, units, margin, min_score, blend_a, templates,
                                       with_nbhd)

    def track_boxes_reacquire(self, frames, units, margin, min_score, blend_a, templates, with_nbhd=False):
        """track_boxes_adapt's arguments and result with lost tracks searched again over the whole frame, in the same
        native call (mtm_track_boxes_reacquire): a track whose hit does not pass `min_score` (required) gets the
        extremum of its template's whole-frame map as the frame's record.  blend_a == 0: no adaptation - the templates
        and their statistics are then returned as None."""
        return self._track_boxes_adapt("mtm_track_boxes_reacquire", frames, units, margin, min_score, blend_a, templates,
                                       with_nbhd)

    def _track_boxes_adapt(self, name, frames, units, margin, min_score, blend_a, templates, with_nbhd):
        n, nt = len(frames), len(units)
        adapt = int(blend_a) != 0
        units = np.ascontiguousarray(units, dtype=BOX_UNIT_DTYPE)
        like = [templates[j] for j in units["templ_idx"].tolist()]
        if n == 0 or nt == 0:
            return (np.zeros(0, dtype=HIT_DTYPE), (np.zeros((0, 3, 3), dtype=np.float32) if with_nbhd else None),
                    [np.array(t) for t in like] if adapt else None,
                    np.zeros((nt, len(TEMPL_STATS_FIELDS))) if adapt else None)
        rows = [_pixel_rows(a) for a in frames]
        if len({r[2] for r in rows}) > 1:       # (one row stride for every frame)
            rows = [_pixel_rows(np.ascontiguousarray(a)) for a in frames]
        a0, _, stride = rows[0]
        chans = 1 if a0.ndim == 2 else a0.shape[2]
        ptrs = (ctypes.c_void_p * n)(*[r[1] for r in rows])
        out = np.empty(n * nt, dtype=HIT_DTYPE)
        nbhd = np.empty((n * nt, 3, 3), dtype=np.float32) if with_nbhd else None
        sizes = [int(np.prod(t.shape)) for t in like]          # (tightly packed, in the frames' pixel type)
        packed = np.empty(sum(sizes), dtype=a0.dtype) if adapt else None
        stats = np.empty((nt, len(TEMPL_STATS_FIELDS)), dtype=np.float64) if adapt else None
        use_min = min_score is not None
        check(getattr(self._lib, name)(self._h, ptrs, n, a0.shape[0], a0.shape[1], chans, _dtype_code(a0), stride,
                                       units.ctypes.data, nt, int(margin), int(use_min),
                                       float(min_score) if use_min else 0.0, out.ctypes.data,
                                       nbhd.ctypes.data if with_nbhd else None, int(blend_a),
                                       packed.ctypes.data if adapt else None, stats.ctypes.data if adapt else None), name)
        if not adapt:
            return out, nbhd, None, None
        ends = np.cumsum(sizes)
        last = [packed[e - s:e].reshape(t.shape).copy() for s, e, t in zip(sizes, ends.tolist(), like)]
        return out, nbhd, last, stats

    def track_boxes_sets(self, frames, start, set_off, set_idx, margin, min_score=None, reacquire=False, with_nbhd=False):
        """track_boxes / track_boxes_nbhd / track_boxes_reacquire for tracks that carry a set of templates of one shape, in
        one native call (mtm_track_boxes_sets).  `start`: BOX_UNIT_DTYPE records, each track's frame-0 region and the first
        template of its set; track k's set is set_idx[set_off[k]:set_off[k + 1]] (int32 arrays, len(start) + 1 offsets).
        Returns (records, neighbourhoods or None): a record's templ_idx is the template of the set that won its frame."""
        n, nt = len(frames), len(start)
        if n == 0 or nt == 0:
            return np.zeros(0, dtype=HIT_DTYPE), (np.zeros((0, 3, 3), dtype=np.float32) if with_nbhd else None)
        rows = [_pixel_rows(a) for a in frames]
        if len({r[2] for r in rows}) > 1:       # (one row stride for every frame)
            rows = [_pixel_rows(np.ascontiguousarray(a)) for a in frames]
        a0, _, stride = rows[0]
        chans = 1 if a0.ndim == 2 else a0.shape[2]
        ptrs = (ctypes.c_void_p * n)(*[r[1] for r in rows])
        start = np.ascontiguousarray(start, dtype=BOX_UNIT_DTYPE)
        set_off = np.ascontiguousarray(set_off, dtype=np.int32)
        set_idx = np.ascontiguousarray(set_idx, dtype=np.int32)
        if len(set_off) != nt + 1 or len(set_idx) != int(set_off[-1]):
            raise ValueError("track_boxes_sets: set_off holds len(start) + 1 offsets into set_idx")
        out = np.empty(n * nt, dtype=HIT_DTYPE)
        nbhd = np.empty((n * nt, 3, 3), dtype=np.float32) if with_nbhd else None
        use_min = min_score is not None
        check(self._lib.mtm_track_boxes_sets(self._h, ptrs, n, a0.shape[0], a0.shape[1], chans, _dtype_code(a0), stride,
                                             start.ctypes.data, nt, set_off.ctypes.data, set_idx.ctypes.data, int(margin),
                                             int(use_min), float(min_score) if use_min else 0.0, int(bool(reacquire)),
                                             out.ctypes.data, nbhd.ctypes.data if with_nbhd else None),
              "mtm_track_boxes_sets")
        return out, nbhd

    def _pair_args(self, reference, image):
        """(args, keep): the nine leading arguments of the mtm_match_blocks* pair entry points - the context, both images'
        rows and row strides, the shape and pixel kind they share - and the arrays the pointers point into, for the
        caller to hold until its call returns."""
        r, rptr, rstride = _pixel_rows(reference)
        a, aptr, astride = _pixel_rows(image)
        chans = 1 if a.ndim == 2 else a.shape[2]
        return (self._h, rptr, rstride, aptr, astride, a.shape[0], a.shape[1], chans, _dtype_code(a)), (r, a)

    def match_blocks(self, reference, image, blocks, margin, method, with_nbhd=False):
        """Every block of `reference` (BLOCK_DTYPE records) searched in `image` - same shape and pixel type, row strides of
        their own - inside its box widened by `margin`, in one native call (mtm_match_blocks).  Returns (records, one per
        block with templ_idx = the block's index, image coordinates; (len(blocks), 3, 3) float32 neighbourhoods of the
        records in the whole image's map - hit_neighbourhoods' values -, or None).  The templates set on the context are
        not touched."""
        blocks = block_records(blocks)
        n = len(blocks)
        out = np.empty(n, dtype=HIT_DTYPE)
        nbhd = np.empty((n, 3, 3), dtype=np.float32) if with_nbhd else None
        if n == 0:
            return out, nbhd
        pair, keep = self._pair_args(reference, image)
        check(self._lib.mtm_match_blocks(*pair, blocks.ctypes.data, n, int(margin), int(method), out.ctypes.data,
                                         nbhd.ctypes.data if with_nbhd else None), "mtm_match_blocks")
        return out, nbhd

    def match_blocks_at(self, reference, image, blocks, offsets, margin, method, with_nbhd=False, second=None):
        """match_blocks with a displacement per block (mtm_match_blocks_at): `offsets` an (N, 2) int32 array of (dx, dy);
        block k's box is that of the block moved by its offset and clamped into the image, widened by `margin`.
        `second` = the exclusion radius: every block's second peak too (mtm_match_blocks_second; `offsets` may then be
        None, mtm_match_blocks' boxes) - a third element is returned, the second peaks' records: x = y = -1 and a NaN
        score where a map has no cell outside the exclusion."""
        blocks = block_records(blocks)
        n = len(blocks)
        if offsets is not None:
            offsets = np.ascontiguousarray(offsets, dtype=np.int32).reshape(n, 2)
        out = np.empty(n, dtype=HIT_DTYPE)
        nbhd = np.empty((n, 3, 3), dtype=np.float32) if with_nbhd else None
        if second is not None:
            out2 = np.empty(n, dtype=HIT_DTYPE)
            if n:
                pair, keep = self._pair_args(reference, image)
                check(self._lib.mtm_match_blocks_second(*pair, blocks.ctypes.data,
                                                        None if offsets is None else offsets.ctypes.data, n, int(margin),
                                                        int(method), out.ctypes.data, nbhd.ctypes.data if with_nbhd else None,
                                                        int(second), out2.ctypes.data), "mtm_match_blocks_second")
            return out, nbhd, out2
        if n == 0:
            return out, nbhd
        pair, keep = self._pair_args(reference, image)
        check(self._lib.mtm_match_blocks_at(*pair, blocks.ctypes.data, offsets.ctypes.data, n, int(margin), int(method),
                                            out.ctypes.data, nbhd.ctypes.data if with_nbhd else None), "mtm_match_blocks_at")
        return out, nbhd

    def match_blocks_masked(self, reference, image, mask, blocks, offsets, margin, method, with_nbhd=False, second=None):
        """match_blocks_at with a static mask over the reference (mtm_match_blocks_masked): `mask` an (H, W) uint8 array,
        non-zero = the pixel takes part, for every channel; uint8 images, methods 0 and 3.  `offsets` may be None
        (match_blocks' boxes); `second` = the exclusion radius, or None.  Returns (records, neighbourhoods or None) and,
        with `second`, the second peaks' records: x = y = -1 and a NaN score mean "none" - in the records, a block whose
        mask keeps no pixel or whose map holds only NaNs."""
        blocks = block_records(blocks)
        n = len(blocks)
        if offsets is not None:
            offsets = np.ascontiguousarray(offsets, dtype=np.int32).reshape(n, 2)
        out = np.empty(n, dtype=HIT_DTYPE)
        nbhd = np.empty((n, 3, 3), dtype=np.float32) if with_nbhd else None
        out2 = np.empty(n, dtype=HIT_DTYPE) if second is not None else None
        if n:
            pair, keep = self._pair_args(reference, image)
            m = np.asarray(mask)
            if m.dtype != np.uint8 or m.ndim != 2 or m.strides[1] != 1 or m.strides[0] < m.shape[1]:
                m = np.ascontiguousarray(m, dtype=np.uint8)
            check(self._lib.mtm_match_blocks_masked(*pair[:5], m.ctypes.data, m.strides[0], *pair[5:], blocks.ctypes.data, n,
                                                    None if offsets is None else offsets.ctypes.data, int(margin), int(method),
                                                    -1 if second is None else int(second), out.ctypes.data,
                                                    nbhd.ctypes.data if with_nbhd else None,
                                                    None if second is None else out2.ctypes.data), "mtm_match_blocks_masked")
        return (out, nbhd) if second is None else (out, nbhd, out2)

    def debug_second_peaks(self, planes, mode_min, exclusion, firsts=None):
        """Test support: the module's debug_second_peaks on this context - blocks_second_kernel, launched once."""
        return debug_second_peaks(planes, mode_min, exclusion, firsts, context=self)

    def debug_validate_blocks(self, positions, grid_shape, step, threshold=2.0, epsilon=0.5):
        """Test support: the module's debug_validate_blocks on this context - blocks_validate_kernel, launched once."""
        return debug_validate_blocks(positions, grid_shape, step, threshold, epsilon, context=self)

    def deform_image(self, image, grid, displacements, q8=False):
        """The module's deform_image on this context: one upload, deform_image_kernel, the warped image back."""
        return deform_image(image, grid, displacements, context=self, q8=q8)

    def debug_steer_q8(self, positions, nbhd, predicted, grid_shape, step, mode_min, smooth, valid=None, steer_positions=None):
        """Test support: the module's debug_steer_q8 on this context - the steer and filter kernels, launched once each."""
        return debug_steer_q8(positions, nbhd, predicted, grid_shape, step, mode_min, smooth, valid, steer_positions, context=self)

    def match_blocks_passes(self, reference, image, passes, counts, method, with_nbhd=False, validate=None, second=None,
                            deform=False, steer=0):
        """Coarse-to-fine block matching in one native call (mtm_match_blocks_passes): `passes` BLOCK_PASS_DTYPE records,
        `counts` the blocks of every pass's grid.  Returns (records, pass-major, sum(counts) of them; neighbourhoods in
        the same order, or None).  The templates set on the context are not touched.
        `validate` = (threshold, epsilon): the median test between the passes (mtm_match_blocks_passes_validated); a third
        element is returned, the (sum(counts),) bool flags of the records in the same order.
        `second` = the exclusion radius (mtm_match_blocks_passes_second): the second peaks' records of every pass, in the
        same order, are returned as the last element.
        `deform` (not with `second`): window deformation between the passes (mtm_match_blocks_passes_deformed); the last
        element returned is then the (sum(counts), 2) int32 field at every block's centre in Q8, zero for pass 0.
        `steer` (with `deform`): 1 - refined positions, filtered, steer the deformed passes
        (mtm_match_blocks_passes_steered); 0 is the deformed call as it is."""
        passes = block_pass_records(passes)
        n = int(sum(counts))
        out = np.empty(n, dtype=HIT_DTYPE)
        nbhd = np.empty((n, 3, 3), dtype=np.float32) if with_nbhd else None
        pair, keep = self._pair_args(reference, image)
        if steer and not deform:
            raise ValueError("match_blocks_passes: steer needs deform")
        if deform and second is not None:
            raise ValueError("match_blocks_passes: deform does not go with second")
        threshold, epsilon = validate if validate is not None else (0.0, 0.0)
        valid = np.zeros(n, dtype=np.uint8) if validate is not None else None
        last = np.zeros((n, 2), dtype=np.int32) if deform else np.empty(n, dtype=HIT_DTYPE) if second is not None else None
        ptr = lambda a: None if a is None else a.ctypes.data     # noqa: E731
        # the native entry, the first that applies: (asked for, its suffix, what follows `valid` in its arguments; None: the
        # plain entry, which takes no median test either)
        suffix, tail = next((s, t) for on, s, t in ((steer, "_steered", lambda: (ptr(last), int(steer))),
                                                    (deform, "_deformed", lambda: (ptr(last),)),
                                                    (second is not None, "_second", lambda: (int(second), ptr(last))),
                                                    (validate is not None, "_validated", tuple),
                                                    (True, "", None)) if on)
        name = "mtm_match_blocks_passes" + suffix
        args = pair + (passes.ctypes.data, len(passes), int(method))
        if tail is None:
            args += (ptr(out), ptr(nbhd))
        else:
            args += (float(threshold), float(epsilon), ptr(out), ptr(nbhd), ptr(valid)) + tail()
        check(getattr(self._lib, name)(*args), name)
        # out, nbhd, [valid], [second | predicted]
        return (out, nbhd) + (() if valid is None else (valid.astype(bool),)) + (() if last is None else (last,))

    def match_blocks_stack(self, frames, blocks, margin, method, mode, with_nbhd=False, planes=False):
        """matchBlocks over the pairs of a frame stack in one native call (mtm_match_blocks_stack): pair p searches
        frames[p + 1] for the blocks (BLOCK_DTYPE records) of frames[p] (`mode` BLOCKS_REF_PREVIOUS) or frames[0]
        (BLOCKS_REF_FIRST).  Frames of one shape and pixel type as track_boxes takes them.  Returns (records, pair-major:
        (len(frames) - 1) * len(blocks); neighbourhoods as match_blocks' in the same order, or None) or, `planes`, the
        (len(blocks), 2 margin + 1, 2 margin + 1) float32 array of every block's score plane averaged over the pairs, NaN
        where the clipped search box has no output.  The templates set on the context are not touched."""
        blocks = block_records(blocks)
        n, npairs, side = len(blocks), len(frames) - 1, 2 * int(margin) + 1
        if planes:
            if npairs < 1:
                raise ValueError("match_blocks_stack: planes need at least two frames")
            out = np.empty((n, side, side), dtype=np.float32)
            if n == 0:
                return out
        else:
            out = np.empty(max(npairs, 0) * n, dtype=HIT_DTYPE)
            nbhd = np.empty((len(out), 3, 3), dtype=np.float32) if with_nbhd else None
            if len(out) == 0:
                return out, nbhd
        rows = [_pixel_rows(a) for a in frames]
        if len({r[2] for r in rows}) > 1:       # (one row stride for every frame)
            rows = [_pixel_rows(np.ascontiguousarray(a)) for a in frames]
        a0, _, stride = rows[0]
        chans = 1 if a0.ndim == 2 else a0.shape[2]
        ptrs = (ctypes.c_void_p * len(rows))(*[r[1] for r in rows])
        args = (self._h, ptrs, len(rows), a0.shape[0], a0.shape[1], chans, _dtype_code(a0), stride, blocks.ctypes.data, n,
                int(margin), int(method), int(mode))
        if planes:
            check(self._lib.mtm_match_blocks_stack(*args, None, None, out.ctypes.data), "mtm_match_blocks_stack")
            return out
        check(self._lib.mtm_match_blocks_stack(*args, out.ctypes.data, nbhd.ctypes.data if with_nbhd else None, None),
              "mtm_match_blocks_stack")
        return out, nbhd

    def _frames_args(self, frames):
        """(args, keep): the eight leading arguments of the mtm_match_blocks_stack_at / _passes entry points - the context,
        the frames' pointers, their number, the shape, pixel kind and row stride they share - and what the pointers point
        into, for the caller to hold until its call returns."""
        rows = [_pixel_rows(a) for a in frames]
        if len({r[2] for r in rows}) > 1:       # (one row stride for every frame)
            rows = [_pixel_rows(np.ascontiguousarray(a)) for a in frames]
        a0, _, stride = rows[0]
        chans = 1 if a0.ndim == 2 else a0.shape[2]
        ptrs = (ctypes.c_void_p * len(rows))(*[r[1] for r in rows])
        return (self._h, ptrs, len(rows), a0.shape[0], a0.shape[1], chans, _dtype_code(a0), stride), (rows, ptrs)

    def match_blocks_stack_at(self, frames, blocks, offsets, margin, method, mode, with_nbhd=False, planes=False):
        """match_blocks_stack with a displacement per block, shared by the pairs (mtm_match_blocks_stack_at): `offsets` an
        (N, 2) int32 array of (dx, dy), block k's box that of match_blocks_at.  Returns (records, neighbourhoods or None) as
        match_blocks_stack does or, `planes`, (the (N, 2 margin + 1, 2 margin + 1) float32 planes of means around every
        block's moved position, the N records of their peaks) - both computed on the device."""
        blocks = block_records(blocks)
        n, npairs, side = len(blocks), len(frames) - 1, 2 * int(margin) + 1
        offsets = np.ascontiguousarray(offsets, dtype=np.int32).reshape(n, 2)
        if planes:
            if npairs < 1:
                raise ValueError("match_blocks_stack_at: planes need at least two frames")
            out, recs = np.empty((n, side, side), dtype=np.float32), np.empty(n, dtype=HIT_DTYPE)
            if n == 0:
                return out, recs
        else:
            out = np.empty(max(npairs, 0) * n, dtype=HIT_DTYPE)
            nbhd = np.empty((len(out), 3, 3), dtype=np.float32) if with_nbhd else None
            if len(out) == 0:
                return out, nbhd
        head, keep = self._frames_args(frames)
        args = head + (blocks.ctypes.data, offsets.ctypes.data, n, int(margin), int(method), int(mode))
        if planes:
            check(self._lib.mtm_match_blocks_stack_at(*args, recs.ctypes.data, None, out.ctypes.data), "mtm_match_blocks_stack_at")
            return out, recs
        check(self._lib.mtm_match_blocks_stack_at(*args, out.ctypes.data, nbhd.ctypes.data if with_nbhd else None, None),
              "mtm_match_blocks_stack_at")
        return out, nbhd

    def match_blocks_stack_passes(self, frames, passes, counts, method, mode, with_nbhd=False, planes=False):
        """match_blocks_passes over the pairs of a frame stack in one native call (mtm_match_blocks_stack_passes): `passes`
        BLOCK_PASS_DTYPE records, `counts` the blocks of every pass's grid.  Returns (records, pair-major and pass-major
        within a pair: (len(frames) - 1) * sum(counts); neighbourhoods in the same order, or None) or, `planes`, (a flat
        float32 array of every pass's planes of means, pass after pass - counts[p] * (2 margin_p + 1)^2 floats each -, the
        sum(counts) records of their peaks, pass-major)."""
        passes = block_pass_records(passes)
        n, npairs = int(sum(counts)), len(frames) - 1
        if npairs < 1:
            raise ValueError("match_blocks_stack_passes: needs at least two frames")
        head, keep = self._frames_args(frames)
        args = head + (passes.ctypes.data, len(passes), int(method), int(mode))
        name = "mtm_match_blocks_stack_passes"
        if planes:
            out = np.empty(int(sum(int(k) * (2 * int(a["margin"]) + 1) ** 2 for k, a in zip(counts, passes))), dtype=np.float32)
            recs = np.empty(n, dtype=HIT_DTYPE)
            check(self._lib.mtm_match_blocks_stack_passes(*args, recs.ctypes.data, None, out.ctypes.data), name)
            return out, recs
        out = np.empty(npairs * n, dtype=HIT_DTYPE)
        nbhd = np.empty((len(out), 3, 3), dtype=np.float32) if with_nbhd else None
        check(self._lib.mtm_match_blocks_stack_passes(*args, out.ctypes.data, nbhd.ctypes.data if with_nbhd else None, None), name)
        return out, nbhd

    def debug_plane_peaks(self, acc, clip, oh, ow, pairs, method):
        """Test support: the module's debug_plane_peaks on this context - blocks_plane_peak_kernel, launched once."""
        return debug_plane_peaks(acc, clip, oh, ow, pairs, method, context=self)

    def hit_neighbourhoods(self, image, points):
        """The 3 x 3 score neighbourhoods of `points` (POINT_DTYPE records: a template of the current set and a window of
        its map over `image`) in one native call (mtm_hit_neighbourhoods): a (len(points), 3, 3) float32 array, element
        [k, 1 + dy, 1 + dx] the score at window (x + dx, y + dy), NaN outside the map."""
        a, ptr, stride = _pixel_rows(image)
        chans = 1 if a.ndim == 2 else a.shape[2]
        points = np.ascontiguousarray(points, dtype=POINT_DTYPE)
        n = len(points)
        out = np.empty((n, 3, 3), dtype=np.float32)
        check(self._lib.mtm_hit_neighbourhoods(self._h, ptr, a.shape[0], a.shape[1], chans, _dtype_code(a), stride,
                                               points.ctypes.data, n, out.ctypes.data), "mtm_hit_neighbourhoods")
        return out

    def find_matches_batch(self, images, mode, score_threshold):
        """Images of one shape and dtype against the current templates in one native call (mtm_find_matches_batch): a list
        of hit arrays, one per image, each what find_matches_image returns for that image alone.  uint8 / uint16 only."""
        n = len(images)
        if n == 0:
            return []
        rows = [_pixel_rows(a) for a in images]
        if len({r[2] for r in rows}) > 1:       # (one row stride for the whole batch)
            rows = [_pixel_rows(np.ascontiguousarray(a)) for a in images]
        a0, _, stride = rows[0]
        chans = 1 if a0.ndim == 2 else a0.shape[2]
        ptrs = (ctypes.c_void_p * n)(*[r[1] for r in rows])
        counts = np.zeros(n, dtype=np.int64)
        hits = _hits_call(self._lib.mtm_find_matches_batch, self._lib.mtm_last_hits, "mtm_find_matches_batch", self._h,
                          ptrs, n, a0.shape[0], a0.shape[1], chans, _dtype_code(a0), stride, int(mode),
                          float(score_threshold), cap=max(4096, 64 * n), counts=counts)
        return np.split(hits, np.cumsum(counts)[:-1])

    def search_nms(self, templates, image, method, score_threshold, max_overlap, n_object=-1):
        """search() + MTM's non-maxima suppression in one native call (mtm_find_matches_image_nms): the kept hits, best
        first.  Dense images leave thousands of peaks on the device; most of the suppressed ones never leave it."""
        self.set_templates(templates, method)
        a, ptr, stride = _pixel_rows(image)
        chans = 1 if a.ndim == 2 else a.shape[2]
        return _hits_call(self._lib.mtm_find_matches_image_nms, self._lib.mtm_last_hits, "mtm_find_matches_image_nms",
                          self._h, ptr, a.shape[0], a.shape[1], chans, _dtype_code(a), stride, float(score_threshold),
                          float(max_overlap), int(n_object))

    def search_sharded_nms(self, templates, image, method, score_threshold, max_overlap, n_object, global_idx):
        """This rank's step of a sharded matchTemplates in one native call (mtm_find_matches_image_sharded_nms): search
        `templates` (this rank's shard; global_idx = their positions in the whole list), all-gather the ranks' hits over
        the context's communicator, merge, suppress.  Collective: every rank calls it; every rank gets the same list."""
        gidx = np.ascontiguousarray(global_idx, dtype=np.int32)
        n_t = len(templates)
        if n_t:
            self.set_templates(templates, method)
            a, ptr, stride = _pixel_rows(image)
            chans = 1 if a.ndim == 2 else a.shape[2]
            shape, code = a.shape, _dtype_code(a)
        else:
            ptr, stride, chans, shape, code = None, 0, 1, (0, 0), MTM_U8
        return _hits_call(self._lib.mtm_find_matches_image_sharded_nms, self._lib.mtm_last_hits,
                          "mtm_find_matches_image_sharded_nms", self._h, ptr, shape[0], shape[1], chans, code, stride,
                          float(score_threshold), float(max_overlap), int(n_object), int(method), gidx.ctypes.data, n_t)

    def find_matches_async(self, mode, score_threshold):
        """Start mtm_find_matches on the context's worker thread and return at once; collect the hits with
        find_matches_wait().  Nothing else may use the context in between."""
        check(self._lib.mtm_find_matches_async(self._h, int(mode), float(score_threshold)), "mtm_find_matches_async")

    def find_matches_wait(self):
        return _hits_call(self._lib.mtm_find_matches_wait, self._lib.mtm_last_hits, "mtm_find_matches_wait", self._h)

    def last_score_map(self, idx, shape):
        """Score map of template `idx` as the last find_matches computed it (map mode only)."""
        out = np.empty(shape, dtype=np.float32)
        check(self._lib.mtm_last_score_map(self._h, int(idx), out.ctypes.data, out.strides[0]), "mtm_last_score_map")
        return out

    def timing(self):
        t = MtmTiming()
        check(self._lib.mtm_get_timing(self._h, ctypes.byref(t)), "mtm_get_timing")
        return {f: getattr(t, f) for f, _ in MtmTiming._fields_}

    # ---- RCCL hit exchange ------------------------------------------------------------------
    def comm_init(self, uid, n_ranks, rank):
        buf = (ctypes.c_char * COMM_ID_BYTES).from_buffer_copy(bytes(uid))
        check(self._lib.mtm_comm_init(self._h, buf, int(n_ranks), int(rank)), "mtm_comm_init")
        self.n_ranks = n_ranks

    def allgather_hits(self, local):
        """RCCL all-gather of hit records.  Collective: exactly ONE exchange per call on every rank - when the
        output buffer turns out too small (a local matter: the buffers are sized per rank) the gathered
        records are fetched from the context with mtm_comm_last_gather, the collective is not repeated."""
        local = np.ascontiguousarray(local, dtype=HIT_DTYPE)
        cap = 4096
        out = np.empty(cap, dtype=HIT_DTYPE)
        counts = np.zeros(self.n_ranks, dtype=np.int64)
        n = ctypes.c_int64(0)
        rc = self._lib.mtm_comm_allgather_hits(self._h, local.ctypes.data, len(local), out.ctypes.data, cap,
                                               counts.ctypes.data, ctypes.byref(n))
        if rc == E_OVERFLOW:
            cap = int(n.value)
            out = np.empty(cap, dtype=HIT_DTYPE)
            rc = self._lib.mtm_comm_last_gather(self._h, out.ctypes.data, cap, counts.ctypes.data, ctypes.byref(n))
        check(rc, "mtm_comm_allgather_hits")
        return out[:n.value], counts


class Group(_RecordMemo):
    """Several GPUs in one process (mtm_group): units sharded over the devices (LPT on their MAC cost), the image
    uploaded and searched on every device concurrently by native worker threads, hit lists merged on the host in
    template order.  Same ``search`` interface and results as a single Context."""

    def __init__(self, devices):
        lib = load()
        devices = [int(d) for d in devices]
        if not devices:
            raise MtmError("Group needs at least one device")
        arr = (ctypes.c_int * len(devices))(*devices)
        h = ctypes.c_void_p()
        check(lib.mtm_group_create(ctypes.byref(h), arr, len(devices)), "mtm_group_create")
        self._lib, self._h, self.devices = lib, h, devices
        self.lock = threading.RLock()
        for env, opt, table in (("MTM_KERNEL", OPT_KERNEL, {"auto": 0, "naive": 1, "dot4": 2, "mfma": 3}),
                                ("MTM_PEAK_BORDER", OPT_PEAK_BORDER, {"constant": 0, "nearest": 1})):
            v = os.environ.get(env)
            if v:
                self.set_option(opt, table[v.lower()])

    def close(self):
        if self._h:
            self._lib.mtm_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    def __len__(self):
        return len(self.devices)

    def set_option(self, opt, value):
        check(self._lib.mtm_group_set_option(self._h, int(opt), int(value)), "mtm_group_set_option")

    # ---- hit exchange: host merge (default) or the in-process RCCL all-gather ------
    def comm_init(self, strict=True):
        """ncclCommInitAll over the group's devices and the RCCL exchange for the searches that follow.  Returns the
        number of ranks of the communicator (ncclCommCount); with strict=False a failure (RCCL missing, a device listed
        twice) leaves the host merge in place and returns 0 instead of raising."""
        rc = self._lib.mtm_group_comm_init(self._h)
        if rc != 0:
            if strict:
                check(rc, "mtm_group_comm_init")
            return 0
        return self.comm_ranks()

    def comm_ranks(self):
        return int(self._lib.mtm_group_comm_ranks(self._h))

    def set_exchange(self, kind):
        """"host" | "rccl" """
        check(self._lib.mtm_group_set_exchange(self._h, {"host": GROUP_EXCHANGE_HOST, "rccl": GROUP_EXCHANGE_RCCL}[kind]),
              "mtm_group_set_exchange")

    def exchange_used(self):
        return {GROUP_EXCHANGE_HOST: "host", GROUP_EXCHANGE_RCCL: "rccl"}[int(self._lib.mtm_group_exchange_used(self._h))]

    def shards(self, templates, image_shape, method):
        """device index of every unit, as a search over an image of this shape would assign them"""
        rec, keep = templ_records(templates)
        dev = np.zeros(max(len(templates), 1), dtype=np.int32)
        check(self._lib.mtm_group_shards(self._h, rec.ctypes.data, len(templates), int(method), int(image_shape[0]),
                                         int(image_shape[1]), dev.ctypes.data), "mtm_group_shards")
        return dev[:len(templates)]

    def timing(self, i):
        t = MtmTiming()
        check(self._lib.mtm_get_timing(self._lib.mtm_group_ctx(self._h, int(i)), ctypes.byref(t)), "mtm_get_timing")
        return {f: getattr(t, f) for f, _ in MtmTiming._fields_}

    def search(self, templates, image, method, mode, score_threshold):
        rec = self._records(templates)
        a, ptr, stride = _pixel_rows(image)
        chans = 1 if a.ndim == 2 else a.shape[2]
        return _hits_call(self._lib.mtm_group_find_matches, self._lib.mtm_group_last_hits, "mtm_group_find_matches",
                          self._h, rec.ctypes.data, len(templates), int(method), ptr, a.shape[0], a.shape[1], chans,
                          _dtype_code(a), stride, int(mode), float(score_threshold))


    def search_nms(self, templates, image, method, score_threshold, max_overlap, n_object=-1):
        """search() + MTM's non-maxima suppression on the merged list in one native call (mtm_group_find_matches_nms)."""
        rec = self._records(templates)
        a, ptr, stride = _pixel_rows(image)
        chans = 1 if a.ndim == 2 else a.shape[2]
        return _hits_call(self._lib.mtm_group_find_matches_nms, self._lib.mtm_group_last_hits,
                          "mtm_group_find_matches_nms", self._h, rec.ctypes.data, len(templates), int(method), ptr,
                          a.shape[0], a.shape[1], chans, _dtype_code(a), stride, float(score_threshold), float(max_overlap),
                          int(n_object))


def parse_devices(spec):
    """"all" | "0,1,2" | iterable of ints | int -> list of device ids (validated against the visible devices)."""
    n = load().mtm_device_count()
    if isinstance(spec, str):
        spec = spec.strip().lower()
        ids = list(range(n)) if spec == "all" else [int(x) for x in spec.split(",") if x.strip() != ""]
    elif isinstance(spec, int):
        ids = [spec]
    else:
        ids = [int(x) for x in spec]
    if not ids:
        raise MtmError("no HIP device visible (libmtm_hip has no CPU fallback)")
    for d in ids:
        if d < 0 or d >= n:
            raise MtmError("device %d is not visible (%d device(s))" % (d, n))
    return ids


_engines = {}


def engine_for(devices=None):
    """The search engine of a matchTemplates / findMatches call: the default single-GPU context, or a device
    group when several devices are asked for (argument, or the MTM_DEVICES environment variable: "all" or a
    comma-separated list).  Engines are created once per device list and reused."""
    if devices is None:
        devices = os.environ.get("MTM_DEVICES")
    if devices is None or devices == "":
        return default_context()
    ids = tuple(parse_devices(devices))
    if len(ids) == 1 and "MTM_DEVICES_FORCE_GROUP" not in os.environ:
        key = ("ctx", ids[0])
        with _default_lock:
            if key not in _engines:
                _engines[key] = Context(ids[0])
            return _engines[key]
    with _default_lock:
        if ids not in _engines:
            _engines[ids] = Group(ids)
        return _engines[ids]


def comm_unique_id():
    buf = (ctypes.c_char * COMM_ID_BYTES)()
    check(load().mtm_comm_unique_id(buf), "mtm_comm_unique_id")
    return bytes(buf)


def nms_indices(boxes, scores, score_threshold, max_overlap, ascending=False, n_object=-1):
    """cv2.dnn.NMSBoxes through the C ABI (host code, works without a GPU)."""
    n = len(boxes)
    hits = np.zeros(n, dtype=HIT_DTYPE)
    if n:
        b = np.asarray(boxes, dtype=np.int64).reshape(n, 4)
        hits["x"], hits["y"], hits["w"], hits["h"] = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
        hits["score"] = np.asarray(scores, dtype=np.float32)
    keep = np.empty(max(n, 1), dtype=np.int32)
    m = ctypes.c_int64(0)
    check(load().mtm_nms(hits.ctypes.data, n, float(score_threshold), int(bool(ascending)), int(n_object),
                         float(max_overlap), keep.ctypes.data, ctypes.byref(m)), "mtm_nms")
    return keep[:m.value]


def nms_hits(hits, score_threshold, max_overlap, ascending=False):
    """Same as nms_indices, on a structured hit array (boxes and float32 scores are taken from it)."""
    n = len(hits)
    if hits.dtype != HIT_DTYPE or not hits.flags.c_contiguous:
        hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    keep = np.empty(max(n, 1), dtype=np.int32)
    m = ctypes.c_int64(0)
    check(load().mtm_nms(hits.ctypes.data, n, float(score_threshold), int(bool(ascending)), -1, float(max_overlap),
                         keep.ctypes.data, ctypes.byref(m)), "mtm_nms")
    return keep[:m.value]


def nms_segments(hits, counts, score_threshold, max_overlap, ascending=False):
    """nms_hits on each of the consecutive segments of `hits` (counts[s] records each) as matchTemplates applies it to one
    search's list (a segment of at most one hit is kept as it is), in one native call (mtm_nms_segments).  Returns the
    kept records' indices into `hits`, segment after segment, and the number kept per segment."""
    if hits.dtype != HIT_DTYPE or not hits.flags.c_contiguous:
        hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    keep = np.empty(max(len(hits), 1), dtype=np.int32)
    kept = np.zeros(max(len(counts), 1), dtype=np.int64)
    check(load().mtm_nms_segments(hits.ctypes.data, counts.ctypes.data, len(counts), float(score_threshold),
                                  int(bool(ascending)), float(max_overlap), keep.ctypes.data, kept.ctypes.data),
          "mtm_nms_segments")
    kept = kept[:len(counts)]
    return keep[:int(kept.sum())], kept


_default_ctx = None
_default_lock = threading.Lock()


def default_context():
    global _default_ctx
    with _default_lock:
        if _default_ctx is None:
            _default_ctx = Context()
        return _default_ctx
