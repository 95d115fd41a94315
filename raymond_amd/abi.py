"""ctypes mirror of include/raymond_hip.h (POD structs and enums only).

Field order, names and widths follow the header one-to-one; the header in turn cites the
reference types it stands for (core/src/scene.rs, core/src/lib.rs, src/trace.rs:32-55,
core/src/tile.rs:7-14).  tests/test_abi_layout.py checks sizes/offsets against the
compiled library.
"""
import ctypes as C

RMD_ABI_VERSION = 6

RMD_OK = 0
RMD_ERR_INVALID_ARGUMENT = 1
RMD_ERR_NO_DEVICE = 2
RMD_ERR_HIP = 3
RMD_ERR_OUT_OF_MEMORY = 4
RMD_ERR_GRID_INDEX = 5
RMD_ERR_UNSUPPORTED = 6
RMD_ERR_RCCL = 7
RMD_ERR_DEVICE_FAULT = 8

STATUS_NAMES = {
    0: "RMD_OK",
    1: "RMD_ERR_INVALID_ARGUMENT",
    2: "RMD_ERR_NO_DEVICE",
    3: "RMD_ERR_HIP",
    4: "RMD_ERR_OUT_OF_MEMORY",
    5: "RMD_ERR_GRID_INDEX",
    6: "RMD_ERR_UNSUPPORTED",
    7: "RMD_ERR_RCCL",
    8: "RMD_ERR_DEVICE_FAULT",
}

# enum Geometry { Plane, Sphere, Grid } — core/src/scene.rs:9-13
RMD_GEOM_PLANE, RMD_GEOM_SPHERE, RMD_GEOM_GRID = 0, 1, 2
# enum Material { Diffuse, Metal, Emission } — core/src/lib.rs:21-26
RMD_MAT_DIFFUSE, RMD_MAT_METAL, RMD_MAT_EMISSION = 0, 1, 2

RMD_MAX_BOUNCE_LIMIT = 16
RMD_FEATURE_CHANNELS = 7  # first-hit feature buffers: 0..2 normal xyz, 3..5 albedo rgb, 6 depth
RMD_ID_SLOTS, RMD_ID_WORDS, RMD_ID_MISS = 4, 10, 0xFFFFFFFF  # ID buffers: key_0 count_0 .. key_3 count_3 other samples; the key of a miss
RMD_AO_WORDS = 4  # AO buffers: occluded open none samples
RMD_RAY_DOUBLES = 6  # a caller-supplied ray: origin xyz, direction xyz
RMD_HIT_DOUBLES = 5  # rmd_ray_hit, 40 bytes: a hit buffer is 5 * n doubles to the framebuffer helpers
RMD_MAX_RAYS = 1 << 30  # rmd_intersect_rays, rmd_camera_rays: the most rays of one call
RMD_ATROUS_MAX_LEVELS = 8  # rmd_denoise_atrous: the most levels a call may ask for
RMD_RENDER_DOF = 1  # rmd_settings.flags
RMD_RENDER_TRACE_BLACK_PATHS = 2  # never end a zero-throughput path early
RMD_RENDER_END_BLACK_PATHS = 4  # end them in scenes with grids too (flags 0: only where provably exact, i.e. scenes without grids)
(RMD_TUNE_SAMPLE_SPLIT, RMD_TUNE_WALK_BATCH, RMD_TUNE_MASK_BUDGET, RMD_TUNE_LAUNCH_FORM, RMD_TUNE_SCRATCH_CAP_MB, RMD_TUNE_WALK_CUT,
 RMD_TUNE_SPLIT_MIN_SAMPLES, RMD_TUNE_CHAIN_ITEMS, RMD_TUNE_AXIS_PAIRS, RMD_TUNE_PATH_QUEUES) = range(10)
RMD_LAUNCH_AUTO, RMD_LAUNCH_PER_ITEM, RMD_LAUNCH_PERSISTENT = range(3)
RMD_COMM_ID_BYTES = 128


class Material(C.Structure):
    _fields_ = [
        ("kind", C.c_uint32),
        ("_pad", C.c_uint32),
        ("color", C.c_double * 3),
        ("roughness", C.c_double),
        ("emission_aux", C.c_double * 5),
    ]


class Object(C.Structure):
    _fields_ = [
        ("geometry_kind", C.c_uint32),
        ("grid_index", C.c_uint32),
        ("origin", C.c_double * 3),
        ("normal", C.c_double * 3),
        ("radius", C.c_double),
        ("material", Material),
    ]


class GridDesc(C.Structure):
    _fields_ = [
        ("bbox_min", C.c_double * 3),
        ("bbox_max", C.c_double * 3),
        ("resolution", C.c_uint32 * 3),
        ("_pad", C.c_uint32),
        ("cell_size", C.c_double * 3),
        ("cells", C.POINTER(C.c_uint32)),
        ("n_cells", C.c_uint64),
        ("mapping_table", C.POINTER(C.c_uint32)),
        ("n_mapping", C.c_uint64),
        ("tri_pos", C.POINTER(C.c_double)),
        ("tri_nrm", C.POINTER(C.c_double)),
        ("n_tris", C.c_uint64),
        ("built", C.c_void_p),
    ]


class Camera(C.Structure):
    _fields_ = [
        ("backbuffer_width", C.c_uint32),
        ("backbuffer_height", C.c_uint32),
        ("fov_vert", C.c_double),
        ("position", C.c_double * 3),
        ("focal_length", C.c_double),
        ("aperture_radius", C.c_double),
    ]


class Settings(C.Structure):
    _fields_ = [
        ("bounce_limit", C.c_uint32),
        ("sample_begin", C.c_uint32),
        ("sample_count", C.c_uint32),
        ("flags", C.c_uint32),
        ("seed", C.c_uint64),
    ]


class TileRect(C.Structure):
    _fields_ = [
        ("left", C.c_uint32),
        ("top", C.c_uint32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
    ]


class RayHit(C.Structure):  # rmd_ray_hit: rmd_intersect_rays' record for one ray, 40 bytes
    _fields_ = [
        ("t", C.c_double),
        ("normal", C.c_double * 3),
        ("object", C.c_int32),
        ("triangle", C.c_uint32),
    ]


class DenoiseCandidate(C.Structure):  # rmd_denoise_candidate
    _fields_ = [
        ("k", C.c_double),
        ("alpha", C.c_double),
        ("k_f", C.c_double),
        ("tau", C.c_double),
        ("guided", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


DENOISE_MAX_CANDIDATES = 4  # RMD_DENOISE_MAX_CANDIDATES

RMD_LUMA_BINS = 256  # rmd_luma_histogram: four bins an octave over 2^-32 .. 2^32

DESPIKE_MAX_RADIUS = 3  # rmd_despike: 1 <= radius <= 3, rank <= (2 * radius + 1)^2 - 2


class TileLuma(C.Structure):  # rmd_tile_luma: rmd_tile_luma_error's result for one rect, 48 bytes
    _fields_ = [
        ("tile_rms", C.c_double),
        ("pixel_rms", C.c_double),
        ("mean_luma", C.c_double),
        ("mean_variance", C.c_double),
        ("mean_rel_variance", C.c_double),
        ("valid", C.c_uint32),
        ("invalid", C.c_uint32),
    ]


LUMA_WEIGHTS = 260  # RMD_LUMA_WEIGHTS: rmd_tile_weighted_error's table, one weight per counter of rmd_luma_histogram without not_finite


class TileWeighted(C.Structure):  # rmd_tile_weighted: rmd_tile_weighted_error's and rmd_tile_weighted_error_dual's result for one rect, 40 bytes
    _fields_ = [
        ("rms", C.c_double),
        ("mean_weighted_variance", C.c_double),
        ("mean_luma", C.c_double),
        ("mean_variance", C.c_double),
        ("valid", C.c_uint32),
        ("invalid", C.c_uint32),
    ]


ADAPTIVE_MEASURES = ("channel_max", "luma_tile", "luma_pixel")  # Settings.adaptive_measure: rmd_tile_error, rmd_tile_luma_error's tile_rms, its pixel_rms


class LumaHistogram(C.Structure):  # rmd_luma_histogram
    _fields_ = [
        ("bins", C.c_uint64 * RMD_LUMA_BINS),
        ("below", C.c_uint64),
        ("above", C.c_uint64),
        ("zero", C.c_uint64),
        ("negative", C.c_uint64),
        ("not_finite", C.c_uint64),
        ("pixels", C.c_uint64),
    ]


class LaunchInfo(C.Structure):  # rmd_launch_info
    _fields_ = [
        ("passes", C.c_uint32),
        ("split_k", C.c_uint32),
        ("persistent", C.c_uint32),
        ("end_black_paths", C.c_uint32),
        ("has_grid", C.c_uint32),
        ("waves_per_workgroup", C.c_uint32),
        ("buffered", C.c_uint32),
        ("chained", C.c_uint32),
        ("queued", C.c_uint32),
    ]
