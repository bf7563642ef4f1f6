"""ctypes binding of the C ABI declared in include/mpt.h (libmpt_hip.so).

The HIP library is the product; there is no CPU fallback.  Loading fails loudly when the
library has not been built, and creating a context fails loudly when no GPU is present.
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MPT_LIB") or os.path.join(_PKG, "lib", "libmpt_hip.so")

RNG_LITERAL, RNG_PHILOX = 0, 1
BSDF_LAMBERT, BSDF_SCATTER, BSDF_SCATTER_ALL = 0, 1, 2
PIPE_WAVEFRONT, PIPE_MEGAKERNEL, PIPE_WAVELOCAL, PIPE_ORDERED, PIPE_AUTO = 0, 1, 2, 3, 4
REFERENCE_ORDER_PIPELINES = (PIPE_WAVEFRONT, PIPE_MEGAKERNEL, PIPE_WAVELOCAL)  # walk the BVH in the reference's own order
DEFAULT_PIPELINE = PIPE_AUTO  # closest-first for big scenes, reference-order wave-local below 8192 primitives
FLAG_COUNT_WORK = 1
FLAG_MOMENTS = 2

STATUS = {0: "MPT_OK", 1: "MPT_ERR_INVALID_ARG", 2: "MPT_ERR_NO_DEVICE", 3: "MPT_ERR_HIP",
          4: "MPT_ERR_BAD_SCENE", 5: "MPT_ERR_NOT_READY", 6: "MPT_ERR_OVERFLOW"}

# every symbol include/mpt.h declares (tests/test_capi_symbols.py checks header <-> library <-> this list)
SYMBOLS = (
    "mpt_create", "mpt_destroy", "mpt_last_error", "mpt_status_string", "mpt_upload_scene", "mpt_set_uniforms",
    "mpt_resize", "mpt_draw", "mpt_render", "mpt_render_async", "mpt_wait", "mpt_async_info", "mpt_sum_buffer", "mpt_set_sum_buffer", "mpt_clear_sum",
    "mpt_read_frame", "mpt_read_sum", "mpt_write_sum", "mpt_get_stats", "mpt_reset_stats", "mpt_stream", "mpt_synchronize",
    "mpt_trace_rays", "mpt_trace_rays_ordered", "mpt_accel_info", "mpt_kat_pcg", "mpt_kat_philox", "mpt_kat_sincos", "mpt_kat_rcp",
    "mpt_build_bvh", "mpt_build_and_upload", "mpt_download_bvh", "mpt_gpu_leaf_max", "mpt_build_info", "mpt_scene_digest", "mpt_read_scene_array", "mpt_read_lean_tile_classes", "mpt_comm_unique_id", "mpt_comm_create_all", "mpt_comm_create_rank", "mpt_reduce_sum", "mpt_comm_destroy",
    "mpt_comm_last_error", "mpt_read_aovs", "mpt_denoise", "mpt_read_denoised", "mpt_denoised_buffer", "mpt_denoise_image",
    "mpt_read_moments", "mpt_render_adaptive", "mpt_read_tile_samples",
    "mpt_temporal_accumulate", "mpt_read_temporal", "mpt_temporal_buffer", "mpt_temporal_reset", "mpt_denoise_temporal",
    "mpt_temporal_image",
    "mpt_svgf_accumulate", "mpt_read_svgf", "mpt_svgf_buffer", "mpt_read_svgf_state", "mpt_svgf_reset", "mpt_svgf_image",
    "mpt_display", "mpt_read_display", "mpt_display_buffer", "mpt_read_display_histogram", "mpt_display_reset", "mpt_display_table",
    "mpt_display_image",
    "mpt_trace_occluded", "mpt_time_trace", "mpt_ambient_occlusion", "mpt_read_ao", "mpt_ao_buffer", "mpt_ao_image",
    "mpt_light_info", "mpt_read_lights", "mpt_direct_lighting", "mpt_read_direct", "mpt_direct_buffer", "mpt_direct_image",
    "mpt_render_nee", "mpt_set_light_sampling", "mpt_get_light_sampling", "mpt_render_nee_adaptive",
    "mpt_set_light_candidates", "mpt_get_light_candidates",
    "mpt_direct_restir", "mpt_read_restir", "mpt_restir_buffer", "mpt_restir_image", "mpt_read_restir_reservoirs",
    "mpt_direct_restir_temporal", "mpt_read_restir_temporal", "mpt_restir_temporal_buffer", "mpt_read_restir_temporal_reservoirs",
    "mpt_restir_temporal_reset", "mpt_restir_temporal_image",
)

# mpt_scene_digest's words: the nine device arrays (mpt_read_scene_array's `which`), then the seven counts
SCENE_ARRAYS = ("nodes", "prims", "mats", "own", "refleaf", "refbox", "always", "ref_bvh", "ref_idx")
SCENE_COUNTS = ("n_nodes", "n_prims", "n_mats", "n_own", "n_leaves", "n_always", "depth")

DENOISE_SUM, DENOISE_FRAME = 0, 1
DENOISE_MAX_ITERATIONS = 8
# include/mpt.h MPT_DENOISE_DEFAULT_* (a sigma <= 0 / iterations < 0 selects them on the device too)
DENOISE_DEFAULTS = dict(iterations=3, sigma_luminance=8.0, sigma_normal=32.0, sigma_depth=0.25)
# include/mpt.h MPT_ADAPTIVE_DEFAULT_* (0 / a floor <= 0 selects them)
ADAPTIVE_DEFAULTS = dict(min_samples=16, batch_samples=16, luminance_floor=0.05)
# include/mpt.h MPT_TEMPORAL_DEFAULT_* (0 / a tolerance <= 0 selects them)
TEMPORAL_DEFAULTS = dict(max_history=32, depth_tolerance=0.05, normal_threshold=0.5, min_weight=0.05)
# include/mpt.h MPT_SVGF_DEFAULT_* (iterations / feedback < 0 and a sigma <= 0 select them; step A's are the TEMPORAL_DEFAULTS)
SVGF_DEFAULTS = dict(iterations=2, sigma_luminance=2.0, sigma_normal=32.0, sigma_depth=0.25, feedback=0)
SVGF_EPSILON = 1e-4
DISPLAY_SUM, DISPLAY_FRAME, DISPLAY_DENOISED, DISPLAY_TEMPORAL, DISPLAY_SVGF, DISPLAY_ADAPTIVE = 0, 1, 2, 3, 4, 5
TONE_CLAMP, TONE_REINHARD, TONE_ACES = 0, 1, 2
TRANSFER_SRGB, TRANSFER_GAMMA22, TRANSFER_LINEAR = 0, 1, 2
# include/mpt.h MPT_DISPLAY_DEFAULT_* (a value <= 0 / percentile 0 selects them; exposure <= 0 selects 1)
DISPLAY_DEFAULTS = dict(white=4.0, percentile=50, key=0.18)
DISPLAY_NO_BIN = 0xFFFFFFFF
WALK_REFERENCE, WALK_OWN, WALK_AUTO = 0, 1, 2
AO_MAX_SAMPLES = 1024
DIRECT_MAX_SAMPLES = 1024
LIGHTS_MAX = 65536
LIGHT_SAMPLING_AREA, LIGHT_SAMPLING_CONE = 0, 1
LIGHT_CANDIDATES_MAX = 32
RESTIR_UNBIASED, RESTIR_BIASED = 0, 1
RESTIR_MAX_NEIGHBOURS, RESTIR_MAX_RADIUS = 16, 64
# include/mpt.h MPT_RESTIR_DEFAULT_* (radius 0 / a threshold <= 0 selects them)
RESTIR_DEFAULTS = dict(radius=4, normal_threshold=0.5, depth_tolerance=0.05)
# include/mpt.h MPT_RESTIR_TEMPORAL_* (max_history 0 / a threshold <= 0 selects the defaults)
RESTIR_TEMPORAL_MAX_HISTORY = 1024
RESTIR_TEMPORAL_DEFAULTS = dict(max_history=20, normal_threshold=0.5, depth_tolerance=0.05)


class MptError(RuntimeError):
    def __init__(self, status, where, detail=""):
        self.status = status
        super().__init__("%s failed: %s%s" % (where, STATUS.get(status, status), (" — " + detail) if detail else ""))


class Uniforms(C.Structure):
    """mpt_uniforms == UniformsData, 144 bytes (R/Renderer/Shaders/Structs.h:23-41)."""
    _fields_ = [
        ("primitiveIndex", C.c_int32), ("_pad0", C.c_int32 * 3),
        ("cameraPosition", C.c_float * 4),
        ("screenSize", C.c_float * 2), ("_pad1", C.c_float * 2),
        ("viewportU", C.c_float * 4),
        ("viewportV", C.c_float * 4),
        ("firstPixelPosition", C.c_float * 4),
        ("randomSeed", C.c_float * 4),
        ("primitiveCount", C.c_uint64),
        ("triangleCount", C.c_uint64),
        ("frameCount", C.c_uint64),
        ("totalPrimitiveCount", C.c_uint64),
    ]


assert C.sizeof(Uniforms) == 144


class RenderParams(C.Structure):
    _fields_ = [
        ("rng_mode", C.c_int32), ("bsdf_mode", C.c_int32), ("max_depth", C.c_int32), ("pipeline", C.c_int32),
        ("sample_begin", C.c_uint32), ("sample_count", C.c_uint32),
        ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32),
        ("shard_rank", C.c_int32), ("shard_count", C.c_int32),
        ("slots_per_iter", C.c_uint32), ("flags", C.c_uint32),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("paths", C.c_uint64), ("rays", C.c_uint64), ("node_visits", C.c_uint64), ("aabb_hits", C.c_uint64),
        ("prim_tests", C.c_uint64), ("iterations", C.c_uint64),
        ("trace_kernel_ms", C.c_double), ("total_ms", C.c_double), ("trace_launches", C.c_uint64),
        ("wave_node_iters", C.c_uint64), ("wave_prim_iters", C.c_uint64), ("wave_leaf_phases", C.c_uint64),
        ("exact_retraces", C.c_uint64), ("tree_parked", C.c_uint64),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DenoiseParams(C.Structure):
    _fields_ = [("source", C.c_int32), ("samples", C.c_uint32), ("iterations", C.c_int32),
                ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float)]


def denoise_params(source=DENOISE_SUM, samples=0, iterations=-1, sigma_luminance=0.0, sigma_normal=0.0, sigma_depth=0.0):
    """mpt_denoise_params; iterations < 0 and sigmas <= 0 mean the defaults of include/mpt.h."""
    return DenoiseParams(int(source), int(samples), int(iterations), float(sigma_luminance), float(sigma_normal),
                         float(sigma_depth))


class AdaptiveParams(C.Structure):
    _fields_ = [("min_samples", C.c_uint32), ("batch_samples", C.c_uint32), ("threshold", C.c_float),
                ("luminance_floor", C.c_float)]


class AdaptiveInfo(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("passes", C.c_uint32), ("tiles_converged", C.c_uint32),
                ("tiles_at_max", C.c_uint32), ("_pad", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "_pad"}


class TemporalParams(C.Structure):
    _fields_ = [("source", C.c_int32), ("samples", C.c_uint32), ("max_history", C.c_uint32),
                ("depth_tolerance", C.c_float), ("normal_threshold", C.c_float), ("min_weight", C.c_float)]


class TemporalInfo(C.Structure):
    _fields_ = [("pixels_reprojected", C.c_uint64), ("pixels_reset", C.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


def temporal_params(source=DENOISE_SUM, samples=0, max_history=0, depth_tolerance=0.0, normal_threshold=0.0, min_weight=0.0):
    """mpt_temporal_params; max_history = 0 and tolerances <= 0 mean the defaults of include/mpt.h."""
    return TemporalParams(int(source), int(samples), int(max_history), float(depth_tolerance), float(normal_threshold),
                          float(min_weight))


class SvgfParams(C.Structure):
    _fields_ = [("source", C.c_int32), ("samples", C.c_uint32), ("max_history", C.c_uint32),
                ("depth_tolerance", C.c_float), ("normal_threshold", C.c_float), ("min_weight", C.c_float),
                ("iterations", C.c_int32), ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float),
                ("feedback", C.c_int32)]


class SvgfInfo(C.Structure):
    _fields_ = [("pixels_reprojected", C.c_uint64), ("pixels_reset", C.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


def svgf_params(source=DENOISE_SUM, samples=0, max_history=0, depth_tolerance=0.0, normal_threshold=0.0, min_weight=0.0, iterations=-1,
                sigma_luminance=0.0, sigma_normal=0.0, sigma_depth=0.0, feedback=-1):
    """mpt_svgf_params; 0 / <= 0 / < 0 mean the defaults of include/mpt.h."""
    return SvgfParams(int(source), int(samples), int(max_history), float(depth_tolerance), float(normal_threshold), float(min_weight),
                      int(iterations), float(sigma_luminance), float(sigma_normal), float(sigma_depth), int(feedback))


class DisplayParams(C.Structure):
    _fields_ = [("source", C.c_int32), ("samples", C.c_uint32), ("tone", C.c_int32), ("transfer", C.c_int32),
                ("exposure", C.c_float), ("white", C.c_float), ("auto_exposure", C.c_int32), ("percentile", C.c_uint32),
                ("key", C.c_float), ("adaptation", C.c_float)]


class DisplayInfo(C.Structure):
    _fields_ = [("scale", C.c_float), ("auto_scale", C.c_float), ("key_bin", C.c_uint32), ("_pad", C.c_uint32),
                ("pixels_counted", C.c_uint64), ("pixels_clipped", C.c_uint64)]

    def as_dict(self):
        """scale / auto_scale as numpy float32 (their bits matter to the tests), the rest as int."""
        return dict(scale=np.float32(self.scale), auto_scale=np.float32(self.auto_scale), key_bin=int(self.key_bin),
                    pixels_counted=int(self.pixels_counted), pixels_clipped=int(self.pixels_clipped))


assert C.sizeof(DisplayParams) == 40 and C.sizeof(DisplayInfo) == 32


def display_params(source=DISPLAY_SUM, samples=0, tone=TONE_CLAMP, transfer=TRANSFER_SRGB, exposure=0.0, white=0.0, auto_exposure=False,
                   percentile=0, key=0.0, adaptation=0.0):
    """mpt_display_params; exposure / white / key <= 0 and percentile = 0 mean the defaults of include/mpt.h."""
    return DisplayParams(int(source), int(samples), int(tone), int(transfer), float(exposure), float(white), int(bool(auto_exposure)),
                         int(percentile), float(key), float(adaptation))


class AoParams(C.Structure):
    _fields_ = [("sample_begin", C.c_uint32), ("sample_count", C.c_uint32), ("radius", C.c_float), ("seed_lo", C.c_uint32),
                ("seed_hi", C.c_uint32), ("walk", C.c_int32)]


class AoInfo(C.Structure):
    _fields_ = [("pixels_surface", C.c_uint64), ("rays", C.c_uint64), ("rays_occluded", C.c_uint64), ("device_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def ao_params(samples=16, radius=0.0, sample_begin=0, seed=(0, 0), walk=WALK_AUTO):
    """mpt_ao_params: `samples` rays per surface pixel, numbered from sample_begin; radius <= 0 means no limit."""
    return AoParams(int(sample_begin), int(samples), float(radius), int(seed[0]) & 0xFFFFFFFF, int(seed[1]) & 0xFFFFFFFF, int(walk))


class DirectParams(C.Structure):
    _fields_ = [("sample_begin", C.c_uint32), ("sample_count", C.c_uint32), ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32),
                ("walk", C.c_int32)]


class DirectInfo(C.Structure):
    _fields_ = [("pixels_surface", C.c_uint64), ("rays", C.c_uint64), ("rays_occluded", C.c_uint64), ("lights", C.c_uint64),
                ("device_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def direct_params(samples=16, sample_begin=0, seed=(0, 0), walk=WALK_AUTO):
    """mpt_direct_params: `samples` light samples per surface pixel, numbered from sample_begin."""
    return DirectParams(int(sample_begin), int(samples), int(seed[0]) & 0xFFFFFFFF, int(seed[1]) & 0xFFFFFFFF, int(walk))


class RestirParams(C.Structure):
    _fields_ = [("sample_begin", C.c_uint32), ("sample_count", C.c_uint32), ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32),
                ("walk", C.c_int32), ("neighbours", C.c_uint32), ("radius", C.c_uint32), ("mode", C.c_int32),
                ("normal_threshold", C.c_float), ("depth_tolerance", C.c_float)]


class RestirInfo(C.Structure):
    _fields_ = [("pixels_surface", C.c_uint64), ("rays_initial", C.c_uint64), ("rays_final", C.c_uint64), ("rays_correction", C.c_uint64),
                ("rays_occluded", C.c_uint64), ("neighbours_accepted", C.c_uint64), ("samples_from_neighbours", C.c_uint64),
                ("lights", C.c_uint64), ("device_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def restir_params(samples=16, sample_begin=0, seed=(0, 0), walk=WALK_AUTO, neighbours=0, radius=0, mode=RESTIR_UNBIASED, normal_threshold=0.0,
                  depth_tolerance=0.0):
    """mpt_restir_params: `samples` rounds per surface pixel, numbered from sample_begin, each merged with `neighbours` reservoirs from
    within `radius` pixels (0: the default radius; a threshold <= 0: its default)."""
    return RestirParams(int(sample_begin), int(samples), int(seed[0]) & 0xFFFFFFFF, int(seed[1]) & 0xFFFFFFFF, int(walk), int(neighbours),
                        int(radius), int(mode), float(normal_threshold), float(depth_tolerance))


class RestirTemporalParams(C.Structure):
    _fields_ = [("frame", C.c_uint32), ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("walk", C.c_int32), ("mode", C.c_int32),
                ("max_history", C.c_uint32), ("normal_threshold", C.c_float), ("depth_tolerance", C.c_float)]


class RestirTemporalInfo(C.Structure):
    _fields_ = [("pixels_surface", C.c_uint64), ("rays_initial", C.c_uint64), ("rays_final", C.c_uint64), ("rays_correction", C.c_uint64),
                ("rays_occluded", C.c_uint64), ("history_accepted", C.c_uint64), ("samples_from_history", C.c_uint64),
                ("pixels_reset", C.c_uint64), ("lights", C.c_uint64), ("device_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def restir_temporal_params(frame=0, seed=(0, 0), walk=WALK_AUTO, mode=RESTIR_UNBIASED, max_history=0, normal_threshold=0.0, depth_tolerance=0.0):
    """mpt_restir_temporal_params: frame number `frame` of a camera path, its reservoirs merged with the previous frame's, which count
    for at most `max_history` frames' candidates (0: the default; a threshold <= 0: its default)."""
    return RestirTemporalParams(int(frame) & 0xFFFFFFFF, int(seed[0]) & 0xFFFFFFFF, int(seed[1]) & 0xFFFFFFFF, int(walk), int(mode),
                                int(max_history), float(normal_threshold), float(depth_tolerance))


class NeeParams(C.Structure):
    _fields_ = [("walk", C.c_int32), ("clamp", C.c_float)]


class NeeInfo(C.Structure):
    _fields_ = [("paths", C.c_uint64), ("rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("shadow_rays_occluded", C.c_uint64),
                ("lights", C.c_uint64), ("device_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def display_table(transfer):
    """mpt_display_table: the 255 float32 thresholds T[1..255] of a transfer function (index k - 1); needs no context."""
    out = np.empty(255, np.float32)
    rc = load().mpt_display_table(int(transfer), _fp(out))
    if rc:
        raise MptError(rc, "mpt_display_table")
    return out


def expand_tile_counts(counts, H, W):
    """(tiles_y, tiles_x) per-tile counts -> (H, W) per-pixel counts (8x8 tiles, the edge tiles cut at the image border)."""
    return np.repeat(np.repeat(np.asarray(counts), 8, axis=0), 8, axis=1)[:H, :W]


_lib = None


def knob_env():
    """The MPT_* environment knobs that change what the device runs, i.e. part of a measured workload."""
    return {k: v for k, v in sorted(os.environ.items())
            if k.startswith("MPT_") and k != "MPT_LIB" and not k.startswith("MPT_BENCH_") and k != "MPT_CPU_THREADS"}


def build_id():
    """What ties a committed counter profile (profiles/*.json) to the build it was taken from: the sha256 of the library that
    is loaded and the sha256 of the sources it is built from (kernels, host side, ABI header, compiler flags) — the second
    survives a rebuild on another machine."""
    import hashlib
    import re
    root = os.path.dirname(_PKG)
    h = hashlib.sha256()
    csrc = os.path.join(_PKG, "csrc")
    files = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".hip")))
    files.append(os.path.join(root, "include", "mpt.h"))
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0" + open(f, "rb").read())
    m = re.search(r"^HIPFLAGS\s*\?=.*$", open(os.path.join(root, "Makefile")).read(), flags=re.M)
    h.update((m.group(0) if m else "").encode())
    lib = hashlib.sha256(open(LIB_PATH, "rb").read()).hexdigest() if os.path.exists(LIB_PATH) else None
    return {"lib_sha256": lib, "source_sha256": h.hexdigest()}


def load():
    """dlopen libmpt_hip.so and declare prototypes.  Raises if the library is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libmpt_hip.so is not built (%s). Run `make` or __graft_entry__.build(); "
                          "there is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, fp, ip, up = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
    L.mpt_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.mpt_destroy.argtypes = [vp]
    L.mpt_last_error.argtypes = [vp]
    L.mpt_last_error.restype = C.c_char_p
    L.mpt_status_string.argtypes = [C.c_int]
    L.mpt_status_string.restype = C.c_char_p
    L.mpt_upload_scene.argtypes = [vp, fp, C.c_uint64, fp, fp, ip, C.c_uint64]
    L.mpt_set_uniforms.argtypes = [vp, C.POINTER(Uniforms)]
    L.mpt_resize.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.mpt_draw.argtypes = [vp, C.POINTER(RenderParams)]
    L.mpt_render.argtypes = [vp, C.POINTER(RenderParams)]
    L.mpt_render_async.argtypes = [vp, C.POINTER(RenderParams)]
    L.mpt_wait.argtypes = [vp]
    L.mpt_sum_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.mpt_set_sum_buffer.argtypes = [vp, vp]
    L.mpt_clear_sum.argtypes = [vp]
    L.mpt_read_frame.argtypes = [vp, fp]
    L.mpt_read_sum.argtypes = [vp, fp]
    L.mpt_write_sum.argtypes = [vp, fp]
    L.mpt_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.mpt_reset_stats.argtypes = [vp]
    L.mpt_stream.argtypes = [vp]
    L.mpt_stream.restype = vp
    L.mpt_synchronize.argtypes = [vp]
    L.mpt_trace_rays.argtypes = [vp, fp, fp, C.c_uint64, fp, ip, fp, ip]
    L.mpt_trace_rays_ordered.argtypes = [vp, fp, fp, C.c_uint64, fp, ip, fp, ip, up]
    L.mpt_accel_info.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.mpt_build_bvh.argtypes = [vp, fp, C.c_uint64, fp, C.c_uint64, C.POINTER(C.c_uint64), ip, C.POINTER(C.c_double)]
    L.mpt_build_and_upload.argtypes = [vp, fp, fp, C.c_uint64, C.POINTER(C.c_double)]
    L.mpt_download_bvh.argtypes = [vp, fp, C.c_uint64, C.POINTER(C.c_uint64), ip]
    L.mpt_gpu_leaf_max.argtypes = [C.c_uint64]
    L.mpt_build_info.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.mpt_scene_digest.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.mpt_read_scene_array.argtypes = [vp, C.c_int, up, C.c_uint64, C.POINTER(C.c_uint64)]
    if hasattr(L, "mpt_read_lean_tile_classes"):   # (MPT_LIB may name a build from before the entry point)
        L.mpt_read_lean_tile_classes.argtypes = [vp, C.c_int, up, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.mpt_comm_unique_id.argtypes = [vp]
    L.mpt_comm_create_all.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(vp)]
    L.mpt_comm_create_rank.argtypes = [vp, C.c_int, C.c_int, vp, C.POINTER(vp)]
    L.mpt_reduce_sum.argtypes = [vp, C.c_int]
    L.mpt_comm_destroy.argtypes = [vp]
    L.mpt_comm_last_error.argtypes = [vp]
    L.mpt_comm_last_error.restype = C.c_char_p
    L.mpt_kat_pcg.argtypes = [vp, up, C.c_uint64, up, fp]
    L.mpt_kat_philox.argtypes = [vp, up, up, C.c_uint64, up]
    L.mpt_kat_sincos.argtypes = [vp, fp, C.c_uint64, fp, fp]
    L.mpt_kat_rcp.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.mpt_async_info.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.mpt_read_aovs.argtypes = [vp, fp, fp, ip]
    L.mpt_denoise.argtypes = [vp, C.POINTER(DenoiseParams)]
    L.mpt_read_denoised.argtypes = [vp, fp]
    L.mpt_denoised_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.mpt_denoise_image.argtypes = [vp, C.c_uint32, C.c_uint32, fp, fp, fp, C.POINTER(DenoiseParams), fp]
    L.mpt_read_moments.argtypes = [vp, fp]
    L.mpt_render_adaptive.argtypes = [vp, C.POINTER(RenderParams), C.POINTER(AdaptiveParams), C.POINTER(AdaptiveInfo)]
    L.mpt_read_tile_samples.argtypes = [vp, up]
    L.mpt_temporal_accumulate.argtypes = [vp, C.POINTER(TemporalParams), C.POINTER(TemporalInfo)]
    L.mpt_read_temporal.argtypes = [vp, fp]
    L.mpt_temporal_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.mpt_temporal_reset.argtypes = [vp]
    L.mpt_denoise_temporal.argtypes = [vp, C.POINTER(DenoiseParams)]
    L.mpt_temporal_image.argtypes = [vp, C.c_uint32, C.c_uint32, fp, fp, fp, C.POINTER(Uniforms), fp, fp, fp, C.POINTER(Uniforms),
                                     C.POINTER(TemporalParams), fp, C.POINTER(TemporalInfo)]
    L.mpt_svgf_accumulate.argtypes = [vp, C.POINTER(SvgfParams), C.POINTER(SvgfInfo)]
    L.mpt_read_svgf.argtypes = [vp, fp]
    L.mpt_svgf_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.mpt_read_svgf_state.argtypes = [vp, fp, fp]
    L.mpt_svgf_reset.argtypes = [vp]
    L.mpt_svgf_image.argtypes = [vp, C.c_uint32, C.c_uint32, fp, fp, fp, C.POINTER(Uniforms), fp, fp, fp, fp, C.POINTER(Uniforms),
                                 C.POINTER(SvgfParams), fp, fp, fp, C.POINTER(SvgfInfo)]
    u8p = C.POINTER(C.c_uint8)
    L.mpt_display.argtypes = [vp, C.POINTER(DisplayParams), C.POINTER(DisplayInfo)]
    L.mpt_read_display.argtypes = [vp, u8p]
    L.mpt_display_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.mpt_read_display_histogram.argtypes = [vp, up]
    L.mpt_display_reset.argtypes = [vp]
    L.mpt_display_table.argtypes = [C.c_int, fp]
    L.mpt_display_image.argtypes = [vp, C.c_uint32, C.c_uint32, fp, C.POINTER(DisplayParams), fp, u8p, up, C.POINTER(DisplayInfo)]
    L.mpt_trace_occluded.argtypes = [vp, fp, fp, fp, C.c_uint64, C.c_int32, u8p, up]
    L.mpt_time_trace.argtypes = [vp, fp, fp, fp, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]
    L.mpt_ambient_occlusion.argtypes = [vp, C.POINTER(AoParams), C.POINTER(AoInfo)]
    L.mpt_read_ao.argtypes = [vp, fp, up]
    L.mpt_ao_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.mpt_ao_image.argtypes = [vp, C.c_uint32, C.c_uint32, fp, fp, C.POINTER(Uniforms), C.POINTER(AoParams), fp, up]
    L.mpt_light_info.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.mpt_read_lights.argtypes = [vp, C.c_uint32, ip, fp, fp, up]
    L.mpt_direct_lighting.argtypes = [vp, C.POINTER(DirectParams), C.POINTER(DirectInfo)]
    L.mpt_read_direct.argtypes = [vp, fp, up, up]
    L.mpt_direct_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.mpt_direct_image.argtypes = [vp, C.c_uint32, C.c_uint32, fp, fp, C.POINTER(Uniforms), C.POINTER(DirectParams), fp, up, up]
    L.mpt_direct_restir.argtypes = [vp, C.POINTER(RestirParams), C.POINTER(RestirInfo)]
    L.mpt_read_restir.argtypes = [vp, fp, up, up]
    L.mpt_restir_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.mpt_restir_image.argtypes = [vp, C.c_uint32, C.c_uint32, fp, fp, C.POINTER(Uniforms), C.POINTER(RestirParams), fp, up, up]
    L.mpt_read_restir_reservoirs.argtypes = [vp, C.c_int32, up]
    L.mpt_direct_restir_temporal.argtypes = [vp, C.POINTER(RestirTemporalParams), C.POINTER(RestirTemporalInfo)]
    L.mpt_read_restir_temporal.argtypes = [vp, fp, up, up]
    L.mpt_restir_temporal_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.mpt_read_restir_temporal_reservoirs.argtypes = [vp, up]
    L.mpt_restir_temporal_reset.argtypes = [vp]
    L.mpt_restir_temporal_image.argtypes = [vp, C.c_uint32, C.c_uint32, fp, fp, C.POINTER(Uniforms), fp, fp, C.POINTER(Uniforms), up,
                                            C.POINTER(RestirTemporalParams), fp, up, up, up, C.POINTER(RestirTemporalInfo)]
    L.mpt_render_nee.argtypes = [vp, C.POINTER(RenderParams), C.POINTER(NeeParams), C.POINTER(NeeInfo)]
    L.mpt_render_nee_adaptive.argtypes = [vp, C.POINTER(RenderParams), C.POINTER(NeeParams), C.POINTER(AdaptiveParams),
                                          C.POINTER(AdaptiveInfo), C.POINTER(NeeInfo)]
    L.mpt_set_light_sampling.argtypes = [vp, C.c_int32]
    L.mpt_get_light_sampling.argtypes = [vp, C.POINTER(C.c_int32)]
    L.mpt_set_light_candidates.argtypes = [vp, C.c_uint32]
    L.mpt_get_light_candidates.argtypes = [vp, C.POINTER(C.c_uint32)]
    _lib = L
    return L


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _up(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def _ray_batch(origins, directions, tmax=None):
    """What the ray queries pass on: contiguous float32 origins, directions [n, 3], tmax [n] (broadcast; None = no limit), and n."""
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
    n = o.shape[0]
    t = None if tmax is None else np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, np.float32), (n,)))
    return o, d, t, n


def gpu_leaf_max(n_prims):
    """mpt_gpu_leaf_max: the leaf limit of the GPU builders for a scene of n_prims primitives (6 below 8192, 2 from there on)."""
    return int(load().mpt_gpu_leaf_max(int(n_prims)))


class Comm:
    """RCCL communicator over the C ABI (mpt_comm_*): `Comm.all([ctx0, ctx1, ...])` for N contexts driven by this
    process, or `Comm.rank(ctx, rank, nranks, id_bytes)` with `Comm.unique_id()` from rank 0 for one process per GPU."""

    def __init__(self, handle, ctxs):
        self.L = load()
        self.h = handle
        self.ctxs = ctxs

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        rc = load().mpt_comm_unique_id(buf)
        if rc:
            raise MptError(rc, "mpt_comm_unique_id")
        return buf.raw

    @classmethod
    def all(cls, ctxs):
        L = load()
        arr = (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])
        h = C.c_void_p()
        rc = L.mpt_comm_create_all(arr, len(ctxs), C.byref(h))
        if rc:
            raise MptError(rc, "mpt_comm_create_all", (L.mpt_last_error(ctxs[0].h) or b"").decode())
        return cls(h, list(ctxs))

    @classmethod
    def rank(cls, ctx, rank, nranks, id_bytes=None):
        L = load()
        h = C.c_void_p()
        buf = C.create_string_buffer(id_bytes, 128) if id_bytes else None
        rc = L.mpt_comm_create_rank(ctx.h, int(rank), int(nranks), buf, C.byref(h))
        if rc:
            raise MptError(rc, "mpt_comm_create_rank", (L.mpt_last_error(ctx.h) or b"").decode())
        return cls(h, [ctx])

    def reduce_sum(self, root=0):
        rc = self.L.mpt_reduce_sum(self.h, int(root))
        if rc:
            raise MptError(rc, "mpt_reduce_sum", (self.L.mpt_comm_last_error(self.h) or b"").decode())

    def close(self):
        if self.h:
            self.L.mpt_comm_destroy(self.h)
            self.h = None


class Context:
    """Owns one mpt_ctx (one GPU, one stream).  Not thread-safe, like the reference Renderer."""

    def __init__(self, device=0):
        self.L = load()
        self.h = C.c_void_p()
        rc = self.L.mpt_create(int(device), C.byref(self.h))
        if rc:
            raise MptError(rc, "mpt_create", "a MI355X GPU is required; there is no CPU fallback")
        self.width = self.height = 0

    def close(self):
        if getattr(self, "h", None):
            self.L.mpt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, where):
        if rc:
            raise MptError(rc, where, (self.L.mpt_last_error(self.h) or b"").decode())

    def upload_scene(self, bvh, prims, mats, prim_idx):
        bvh = np.ascontiguousarray(bvh, np.float32)
        prims = np.ascontiguousarray(prims, np.float32)
        mats = np.ascontiguousarray(mats, np.float32)
        prim_idx = np.ascontiguousarray(prim_idx, np.int32)
        n_nodes = bvh.size // 8
        n_prims = prims.size // 12
        if mats.size != n_prims * 8 or prim_idx.size != n_prims:
            raise ValueError("scene arrays disagree on the primitive count")
        self._chk(self.L.mpt_upload_scene(self.h, _fp(bvh), n_nodes, _fp(prims), _fp(mats), _ip(prim_idx), n_prims),
                  "mpt_upload_scene")

    def set_uniforms(self, u):
        self._chk(self.L.mpt_set_uniforms(self.h, C.byref(u)), "mpt_set_uniforms")

    def resize(self, w, h):
        self._chk(self.L.mpt_resize(self.h, int(w), int(h)), "mpt_resize")
        self.width, self.height = int(w), int(h)

    @staticmethod
    def params(rng_mode=RNG_PHILOX, bsdf_mode=BSDF_LAMBERT, max_depth=32, pipeline=DEFAULT_PIPELINE, sample_begin=0,
               sample_count=1, seed=(1, 0), shard_rank=0, shard_count=1, slots_per_iter=0, flags=0):
        return RenderParams(rng_mode, bsdf_mode, max_depth, pipeline, sample_begin, sample_count, seed[0], seed[1],
                            shard_rank, shard_count, slots_per_iter, flags)

    def draw(self, **kw):
        p = self.params(**kw)
        self._chk(self.L.mpt_draw(self.h, C.byref(p)), "mpt_draw")

    def render(self, **kw):
        p = self.params(**kw)
        self._chk(self.L.mpt_render(self.h, C.byref(p)), "mpt_render")

    def render_async(self, **kw):
        """Enqueue a render and return; up to two overlap on the device.  wait() collects them (and their stats)."""
        p = self.params(**kw)
        self._chk(self.L.mpt_render_async(self.h, C.byref(p)), "mpt_render_async")

    def wait(self):
        self._chk(self.L.mpt_wait(self.h), "mpt_wait")

    def async_info(self):
        out = (C.c_uint64 * 4)()
        self._chk(self.L.mpt_async_info(self.h, out), "mpt_async_info")
        return dict(zip(("submitted", "gate_resident", "gate_timeout", "call_us_max"), [int(v) for v in out]))

    def clear_sum(self):
        self._chk(self.L.mpt_clear_sum(self.h), "mpt_clear_sum")

    def sum_buffer(self):
        p, n = C.c_void_p(), C.c_uint64()
        self._chk(self.L.mpt_sum_buffer(self.h, C.byref(p), C.byref(n)), "mpt_sum_buffer")
        return p.value, n.value

    def set_sum_buffer(self, device_ptr):
        self._chk(self.L.mpt_set_sum_buffer(self.h, C.c_void_p(device_ptr)), "mpt_set_sum_buffer")

    def read_frame(self):
        out = np.empty((self.height, self.width, 4), np.float32)
        self._chk(self.L.mpt_read_frame(self.h, _fp(out)), "mpt_read_frame")
        return out

    def read_sum(self):
        out = np.empty((self.height, self.width, 4), np.float32)
        self._chk(self.L.mpt_read_sum(self.h, _fp(out)), "mpt_read_sum")
        return out

    def write_sum(self, rgba):
        """Put an HDR sum back (checkpoint / resume): the inverse of read_sum."""
        a = np.ascontiguousarray(rgba, np.float32)
        if a.shape != (self.height, self.width, 4):
            raise ValueError("write_sum: expected an array of shape (%d, %d, 4)" % (self.height, self.width))
        self._chk(self.L.mpt_write_sum(self.h, _fp(a)), "mpt_write_sum")

    def stats(self):
        s = Stats()
        self._chk(self.L.mpt_get_stats(self.h, C.byref(s)), "mpt_get_stats")
        return s.as_dict()

    def reset_stats(self):
        self._chk(self.L.mpt_reset_stats(self.h), "mpt_reset_stats")

    def synchronize(self):
        self._chk(self.L.mpt_synchronize(self.h), "mpt_synchronize")

    def stream(self):
        return self.L.mpt_stream(self.h)

    def trace_rays(self, origins, directions):
        o, d, _, n = _ray_batch(origins, directions)
        t = np.empty(n, np.float32)
        prim = np.empty(n, np.int32)
        nrm = np.empty((n, 3), np.float32)
        front = np.empty(n, np.int32)
        self._chk(self.L.mpt_trace_rays(self.h, _fp(o), _fp(d), n, _fp(t), _ip(prim), _fp(nrm), _ip(front)),
                  "mpt_trace_rays")
        return t, prim, nrm, front

    def trace_rays_ordered(self, origins, directions):
        """Closest hit through the closest-first walk of PIPE_ORDERED; also returns the per-ray re-trace flags."""
        o, d, _, n = _ray_batch(origins, directions)
        t = np.empty(n, np.float32)
        prim = np.empty(n, np.int32)
        nrm = np.empty((n, 3), np.float32)
        front = np.empty(n, np.int32)
        flags = np.empty(n, np.uint32)
        self._chk(self.L.mpt_trace_rays_ordered(self.h, _fp(o), _fp(d), n, _fp(t), _ip(prim), _fp(nrm), _ip(front),
                                                _up(flags)), "mpt_trace_rays_ordered")
        return t, prim, nrm, front, flags

    def trace_occluded(self, origins, directions, tmax=None, walk=WALK_AUTO):
        """mpt_trace_occluded: is anything in the way before tmax (per ray; None = no limit)?  Returns (occluded [n] bool,
        flags [n] uint32 as trace_rays_ordered's)."""
        o, d, t, n = _ray_batch(origins, directions, tmax)
        occ = np.empty(n, np.uint8)
        flags = np.empty(n, np.uint32)
        self._chk(self.L.mpt_trace_occluded(self.h, _fp(o), _fp(d), None if t is None else _fp(t), n, int(walk),
                                            occ.ctypes.data_as(C.POINTER(C.c_uint8)), _up(flags)), "mpt_trace_occluded")
        return occ.astype(bool), flags

    def time_trace(self, origins, directions, tmax=None, warmup=3, reps=20):
        """mpt_time_trace: HIP-event ms per launch, [reps, 4] = (closest reference, any-hit reference, closest own, any-hit own)."""
        o, d, t, n = _ray_batch(origins, directions, tmax)
        ms = np.zeros((int(reps), 4), np.float64)
        self._chk(self.L.mpt_time_trace(self.h, _fp(o), _fp(d), None if t is None else _fp(t), n, int(warmup), int(reps),
                                        ms.ctypes.data_as(C.POINTER(C.c_double))), "mpt_time_trace")
        return ms

    def ambient_occlusion(self, **kw):
        """mpt_ambient_occlusion over the context's guide buffers (ao_params' keywords); returns the info dict."""
        p = ao_params(**kw)
        info = AoInfo()
        self._chk(self.L.mpt_ambient_occlusion(self.h, C.byref(p), C.byref(info)), "mpt_ambient_occlusion")
        return info.as_dict()

    def read_ao(self):
        """(ao [H,W] float32, occluded [H,W] uint32) of the last ambient_occlusion."""
        ao = np.empty((self.height, self.width), np.float32)
        occ = np.empty((self.height, self.width), np.uint32)
        self._chk(self.L.mpt_read_ao(self.h, _fp(ao), _up(occ)), "mpt_read_ao")
        return ao, occ

    def ao_buffer(self):
        """(device pointer, bytes) of the last ambient_occlusion's ao image (float32, W * H)."""
        p, n = C.c_void_p(), C.c_uint64()
        self._chk(self.L.mpt_ao_buffer(self.h, C.byref(p), C.byref(n)), "mpt_ao_buffer")
        return p.value, n.value

    def ao_image(self, albedo_depth, normal_class, cam, **kw):
        """The AO kernel on caller guides [H,W,4] with the camera of `cam` (Uniforms); needs a scene, touches no context state."""
        ad = np.ascontiguousarray(albedo_depth, np.float32)
        nc = np.ascontiguousarray(normal_class, np.float32)
        if ad.ndim != 3 or ad.shape[2] != 4 or nc.shape != ad.shape:
            raise ValueError("ao_image: albedo_depth and normal_class must be [H, W, 4] arrays of one shape")
        H, W = ad.shape[:2]
        ao = np.empty((H, W), np.float32)
        occ = np.empty((H, W), np.uint32)
        p = ao_params(**kw)
        self._chk(self.L.mpt_ao_image(self.h, W, H, _fp(ad), _fp(nc), C.byref(cam), C.byref(p), _fp(ao), _up(occ)), "mpt_ao_image")
        return ao, occ

    def light_info(self):
        """mpt_light_info: the light table of the scene in place (built if stale) as a dict of counts."""
        out = (C.c_uint64 * 4)()
        self._chk(self.L.mpt_light_info(self.h, out), "mpt_light_info")
        return dict(lights=out[0], emissive_prims=out[1], triangle_lights=out[2], sphere_lights=out[3])

    def read_lights(self):
        """mpt_read_lights: (prim_id [n] int32, records [n, 4, 4] float32, cdf [n] float32) of the light table."""
        n = C.c_uint32()
        self._chk(self.L.mpt_read_lights(self.h, 0, None, None, None, C.byref(n)), "mpt_read_lights")
        ids = np.empty(n.value, np.int32)
        rec = np.empty((n.value, 4, 4), np.float32)
        cdf = np.empty(n.value, np.float32)
        if n.value:
            self._chk(self.L.mpt_read_lights(self.h, n.value, _ip(ids), _fp(rec), _fp(cdf), C.byref(n)), "mpt_read_lights")
        return ids, rec, cdf

    def direct_lighting(self, **kw):
        """mpt_direct_lighting over the context's guide buffers (direct_params' keywords); returns the info dict."""
        p = direct_params(**kw)
        info = DirectInfo()
        self._chk(self.L.mpt_direct_lighting(self.h, C.byref(p), C.byref(info)), "mpt_direct_lighting")
        return info.as_dict()

    def read_direct(self):
        """(rgba [H,W,4] float32, traced [H,W] uint32, unoccluded [H,W] uint32) of the last direct_lighting."""
        rgba = np.empty((self.height, self.width, 4), np.float32)
        traced = np.empty((self.height, self.width), np.uint32)
        unocc = np.empty((self.height, self.width), np.uint32)
        self._chk(self.L.mpt_read_direct(self.h, _fp(rgba), _up(traced), _up(unocc)), "mpt_read_direct")
        return rgba, traced, unocc

    def direct_buffer(self):
        """(device pointer, bytes) of the last direct_lighting's RGBA32F image."""
        p, n = C.c_void_p(), C.c_uint64()
        self._chk(self.L.mpt_direct_buffer(self.h, C.byref(p), C.byref(n)), "mpt_direct_buffer")
        return p.value, n.value

    def direct_image(self, albedo_depth, normal_class, cam, **kw):
        """The direct-lighting kernel on caller guides [H,W,4] with the camera of `cam` (Uniforms); needs a scene."""
        ad = np.ascontiguousarray(albedo_depth, np.float32)
        nc = np.ascontiguousarray(normal_class, np.float32)
        if ad.ndim != 3 or ad.shape[2] != 4 or nc.shape != ad.shape:
            raise ValueError("direct_image: albedo_depth and normal_class must be [H, W, 4] arrays of one shape")
        H, W = ad.shape[:2]
        rgba = np.empty((H, W, 4), np.float32)
        traced = np.empty((H, W), np.uint32)
        unocc = np.empty((H, W), np.uint32)
        p = direct_params(**kw)
        self._chk(self.L.mpt_direct_image(self.h, W, H, _fp(ad), _fp(nc), C.byref(cam), C.byref(p), _fp(rgba), _up(traced), _up(unocc)),
                  "mpt_direct_image")
        return rgba, traced, unocc

    def direct_restir(self, **kw):
        """mpt_direct_restir over the context's guide buffers (restir_params' keywords): the direct pass with spatial reservoir reuse;
        returns the info dict."""
        p = restir_params(**kw)
        info = RestirInfo()
        self._chk(self.L.mpt_direct_restir(self.h, C.byref(p), C.byref(info)), "mpt_direct_restir")
        return info.as_dict()

    def read_restir(self):
        """(rgba [H,W,4] float32, traced [H,W] uint32, unoccluded [H,W] uint32) of the last direct_restir."""
        rgba = np.empty((self.height, self.width, 4), np.float32)
        traced = np.empty((self.height, self.width), np.uint32)
        unocc = np.empty((self.height, self.width), np.uint32)
        self._chk(self.L.mpt_read_restir(self.h, _fp(rgba), _up(traced), _up(unocc)), "mpt_read_restir")
        return rgba, traced, unocc

    def restir_buffer(self):
        """(device pointer, bytes) of the last direct_restir's RGBA32F image."""
        p, n = C.c_void_p(), C.c_uint64()
        self._chk(self.L.mpt_restir_buffer(self.h, C.byref(p), C.byref(n)), "mpt_restir_buffer")
        return p.value, n.value

    def read_restir_reservoirs(self, which):
        """The last round's reservoirs of the last direct_restir, [H,W,6] uint32: k, the bits of ua, ub, wsum, fac, flags (bit 0 holds,
        bit 1 own).  which = 0: after step A; 1: the pick after step B."""
        out = np.empty((self.height, self.width, 6), np.uint32)
        self._chk(self.L.mpt_read_restir_reservoirs(self.h, int(which), _up(out)), "mpt_read_restir_reservoirs")
        return out

    def restir_image(self, albedo_depth, normal_class, cam, **kw):
        """The kernels of direct_restir on caller guides [H,W,4] with the camera of `cam` (Uniforms); needs a scene."""
        ad = np.ascontiguousarray(albedo_depth, np.float32)
        nc = np.ascontiguousarray(normal_class, np.float32)
        if ad.ndim != 3 or ad.shape[2] != 4 or nc.shape != ad.shape:
            raise ValueError("restir_image: albedo_depth and normal_class must be [H, W, 4] arrays of one shape")
        H, W = ad.shape[:2]
        rgba = np.empty((H, W, 4), np.float32)
        traced = np.empty((H, W), np.uint32)
        unocc = np.empty((H, W), np.uint32)
        p = restir_params(**kw)
        self._chk(self.L.mpt_restir_image(self.h, W, H, _fp(ad), _fp(nc), C.byref(cam), C.byref(p), _fp(rgba), _up(traced), _up(unocc)),
                  "mpt_restir_image")
        return rgba, traced, unocc

    def direct_restir_temporal(self, **kw):
        """mpt_direct_restir_temporal over the context's guide buffers (restir_temporal_params' keywords): one frame of the direct pass
        whose reservoirs are merged with the previous frame's; returns the info dict."""
        p = restir_temporal_params(**kw)
        info = RestirTemporalInfo()
        self._chk(self.L.mpt_direct_restir_temporal(self.h, C.byref(p), C.byref(info)), "mpt_direct_restir_temporal")
        return info.as_dict()

    def read_restir_temporal(self):
        """(rgba [H,W,4] float32, traced [H,W] uint32, unoccluded [H,W] uint32) of the last direct_restir_temporal."""
        rgba = np.empty((self.height, self.width, 4), np.float32)
        traced = np.empty((self.height, self.width), np.uint32)
        unocc = np.empty((self.height, self.width), np.uint32)
        self._chk(self.L.mpt_read_restir_temporal(self.h, _fp(rgba), _up(traced), _up(unocc)), "mpt_read_restir_temporal")
        return rgba, traced, unocc

    def restir_temporal_buffer(self):
        """(device pointer, bytes) of the last direct_restir_temporal's RGBA32F image."""
        p, n = C.c_void_p(), C.c_uint64()
        self._chk(self.L.mpt_restir_temporal_buffer(self.h, C.byref(p), C.byref(n)), "mpt_restir_temporal_buffer")
        return p.value, n.value

    def read_restir_temporal_reservoirs(self):
        """The reservoirs the last direct_restir_temporal left for the next frame, [H,W,7] uint32: k, the bits of ua, ub, wsum, fac, flags
        (bit 0 holds, bit 1 own) and the count Mh."""
        out = np.empty((self.height, self.width, 7), np.uint32)
        self._chk(self.L.mpt_read_restir_temporal_reservoirs(self.h, _up(out)), "mpt_read_restir_temporal_reservoirs")
        return out

    def restir_temporal_reset(self):
        """mpt_restir_temporal_reset: the next direct_restir_temporal starts without a history."""
        self._chk(self.L.mpt_restir_temporal_reset(self.h), "mpt_restir_temporal_reset")

    def restir_temporal_image(self, albedo_depth, normal_class, cam, prev=None, **kw):
        """The kernels of direct_restir_temporal on caller guides [H,W,4] with the camera of `cam` (Uniforms); needs a scene.  prev: None
        (no history) or (albedo_depth, normal_class, cam, reservoirs [H,W,7]) of the previous frame.  Returns (rgba, traced, unoccluded,
        reservoirs [H,W,7], info dict)."""
        ad = np.ascontiguousarray(albedo_depth, np.float32)
        nc = np.ascontiguousarray(normal_class, np.float32)
        if ad.ndim != 3 or ad.shape[2] != 4 or nc.shape != ad.shape:
            raise ValueError("restir_temporal_image: albedo_depth and normal_class must be [H, W, 4] arrays of one shape")
        H, W = ad.shape[:2]
        args_prev = (None, None, None, None)
        if prev is not None:
            ad_h = np.ascontiguousarray(prev[0], np.float32)
            nc_h = np.ascontiguousarray(prev[1], np.float32)
            res_h = np.ascontiguousarray(prev[3], np.uint32)
            if ad_h.shape != ad.shape or nc_h.shape != ad.shape or res_h.shape != (H, W, 7):
                raise ValueError("restir_temporal_image: the previous frame's arrays must be [H, W, 4], [H, W, 4] and [H, W, 7]")
            args_prev = (_fp(ad_h), _fp(nc_h), C.byref(prev[2]), _up(res_h))
        rgba = np.empty((H, W, 4), np.float32)
        traced = np.empty((H, W), np.uint32)
        unocc = np.empty((H, W), np.uint32)
        res = np.empty((H, W, 7), np.uint32)
        p = restir_temporal_params(**kw)
        info = RestirTemporalInfo()
        self._chk(self.L.mpt_restir_temporal_image(self.h, W, H, _fp(ad), _fp(nc), C.byref(cam), *args_prev, C.byref(p), _fp(rgba), _up(traced),
                                                   _up(unocc), _up(res), C.byref(info)), "mpt_restir_temporal_image")
        return rgba, traced, unocc, res, info.as_dict()

    def render_nee(self, walk=WALK_AUTO, clamp=0.0, **params):
        """mpt_render_nee: the samples of `params` (the keywords of render) with a light sample and MIS at every Lambert vertex, added
        to the HDR sum; clamp <= 0 = no per-sample clamp, 1 = mpt_render's.  Returns the mpt_nee_info as a dict."""
        p = self.params(**params)
        n = NeeParams(int(walk), float(clamp))
        info = NeeInfo()
        self._chk(self.L.mpt_render_nee(self.h, C.byref(p), C.byref(n), C.byref(info)), "mpt_render_nee")
        return info.as_dict()

    def render_nee_adaptive(self, threshold, min_samples=0, batch_samples=0, luminance_floor=0.0, walk=WALK_AUTO, clamp=0.0, **params):
        """mpt_render_nee_adaptive: render_nee's estimator with render_adaptive's allocation, every 8x8 tile deciding on the device in
        one launch; sample_count (params) is the most samples a tile gets.  Clears the sum, the moments and the tile counts first.
        Returns {"adaptive": the mpt_adaptive_info, "nee": the mpt_nee_info}, each as a dict."""
        p = self.params(**params)
        n = NeeParams(int(walk), float(clamp))
        a = AdaptiveParams(int(min_samples), int(batch_samples), float(threshold), float(luminance_floor))
        info, nee = AdaptiveInfo(), NeeInfo()
        self._chk(self.L.mpt_render_nee_adaptive(self.h, C.byref(p), C.byref(n), C.byref(a), C.byref(info), C.byref(nee)),
                  "mpt_render_nee_adaptive")
        return {"adaptive": info.as_dict(), "nee": nee.as_dict()}

    def set_light_sampling(self, mode):
        """mpt_set_light_sampling: LIGHT_SAMPLING_AREA (the default) or LIGHT_SAMPLING_CONE — how direct_lighting, direct_image and
        render_nee sample a sphere light."""
        self._chk(self.L.mpt_set_light_sampling(self.h, int(mode)), "mpt_set_light_sampling")

    @property
    def light_sampling(self):
        mode = C.c_int32(-1)
        self._chk(self.L.mpt_get_light_sampling(self.h, C.byref(mode)), "mpt_get_light_sampling")
        return mode.value

    def set_light_candidates(self, m):
        """mpt_set_light_candidates: from how many candidates (1..LIGHT_CANDIDATES_MAX; 1, the default, is no resampling) a light
        sample of direct_lighting, direct_image and render_nee is resampled."""
        self._chk(self.L.mpt_set_light_candidates(self.h, int(m)), "mpt_set_light_candidates")

    def get_light_candidates(self):
        m = C.c_uint32(0)
        self._chk(self.L.mpt_get_light_candidates(self.h, C.byref(m)), "mpt_get_light_candidates")
        return m.value

    def build_bvh(self, prims):
        """GPU LBVH over the packed primitive array (12 floats each) -> (bvh [N, 8] f32, prim_idx [P] i32, device ms)."""
        prims = np.ascontiguousarray(prims, np.float32).reshape(-1, 12)
        n = prims.shape[0]
        bvh = np.zeros((2 * n - 1, 8), np.float32)
        idx = np.zeros(n, np.int32)
        nn, ms = C.c_uint64(), C.c_double()
        self._chk(self.L.mpt_build_bvh(self.h, _fp(prims), n, _fp(bvh), 2 * n - 1, C.byref(nn), _ip(idx), C.byref(ms)),
                  "mpt_build_bvh")
        return bvh[: nn.value].copy(), idx, ms.value

    def build_and_upload(self, prims, mats):
        """Build the BVH on the device and make it the scene, without a host round trip.  Returns the device ms."""
        prims = np.ascontiguousarray(prims, np.float32).reshape(-1, 12)
        mats = np.ascontiguousarray(mats, np.float32).reshape(-1, 8)
        assert prims.shape[0] == mats.shape[0]
        ms = C.c_double()
        self._chk(self.L.mpt_build_and_upload(self.h, _fp(prims), _fp(mats), prims.shape[0], C.byref(ms)), "mpt_build_and_upload")
        return ms.value

    def build_info(self):
        """mpt_build_info: what the last scene call left on the device (sizes come from the C API, not from this object)."""
        out = (C.c_uint64 * 8)()
        self._chk(self.L.mpt_build_info(self.h, out), "mpt_build_info")
        keys = ("built_prims", "built_nodes", "built_leaf_max", "auto_ordered_prims", "prims", "threaded_nodes", "materials", "unquantised_nodes")
        return dict(zip(keys, [int(v) for v in out]))

    def download_bvh(self):
        """The tree of the last build_and_upload in the reference's buffer format: (bvh [N, 2, 4] f32, prim_idx [P] i32).
        MPT_ERR_NOT_READY when the scene on the device did not come from build_and_upload."""
        info = self.build_info()
        n, nodes = info["built_prims"], max(1, info["built_nodes"])
        bvh = np.zeros((nodes, 2, 4), np.float32)
        idx = np.zeros(max(1, n), np.int32)
        nn = C.c_uint64()
        self._chk(self.L.mpt_download_bvh(self.h, _fp(bvh), nodes, C.byref(nn), _ip(idx)), "mpt_download_bvh")
        return bvh[: nn.value].copy(), idx[:n]

    def scene_digest(self):
        """16 words: digests of the scene's nine device arrays, then seven counts (include/mpt.h)"""
        out = (C.c_uint64 * 16)()
        self._chk(self.L.mpt_scene_digest(self.h, out), "mpt_scene_digest")
        return [int(v) for v in out]

    def read_scene_array(self, which):
        """mpt_read_scene_array: device array `which` (0..8, the order of SCENE_ARRAYS) as uint32 words; empty where the scene has none."""
        n = C.c_uint64()
        self._chk(self.L.mpt_read_scene_array(self.h, int(which), None, 0, C.byref(n)), "mpt_read_scene_array")
        out = np.zeros(n.value, np.uint32)
        if n.value:
            self._chk(self.L.mpt_read_scene_array(self.h, int(which), _up(out), n.value, C.byref(n)), "mpt_read_scene_array")
        return out

    def read_lean_tile_classes(self, lane=-1):
        """mpt_read_lean_tile_classes: (the class words of render lane `lane` (-1: the last one that traced) as uint32, row-major by tile; tables built by this context so far)."""
        n, builds = C.c_uint64(), C.c_uint64()
        self._chk(self.L.mpt_read_lean_tile_classes(self.h, int(lane), None, 0, C.byref(n), C.byref(builds)), "mpt_read_lean_tile_classes")
        out = np.zeros(n.value, np.uint32)
        if n.value:
            self._chk(self.L.mpt_read_lean_tile_classes(self.h, int(lane), _up(out), n.value, C.byref(n), C.byref(builds)), "mpt_read_lean_tile_classes")
        return out, builds.value

    def read_scene(self):
        """Every device array of the scene and the counts: ({name: uint32 words} over SCENE_ARRAYS, {name: int} over SCENE_COUNTS)."""
        arrays = {name: self.read_scene_array(k) for k, name in enumerate(SCENE_ARRAYS)}
        return arrays, dict(zip(SCENE_COUNTS, self.scene_digest()[9:]))

    def accel_info(self):
        out = (C.c_uint64 * 8)()
        self._chk(self.L.mpt_accel_info(self.h, out), "mpt_accel_info")
        keys = ("ordered_ok", "nodes", "depth", "lds_nodes", "always_spheres", "reference_leaves", "lds_prims", "auto_pipeline")
        return dict(zip(keys, [int(v) for v in out]))

    def read_aovs(self):
        """First-hit guide buffers (traced on the device if stale): (albedo_depth [H,W,4], normal_class [H,W,4], prim [H,W])."""
        ad = np.empty((self.height, self.width, 4), np.float32)
        nc = np.empty((self.height, self.width, 4), np.float32)
        prim = np.empty((self.height, self.width), np.int32)
        self._chk(self.L.mpt_read_aovs(self.h, _fp(ad), _fp(nc), _ip(prim)), "mpt_read_aovs")
        return ad, nc, prim

    def denoise(self, **kw):
        """mpt_denoise: filter the sum (source=DENOISE_SUM, samples=spp) or the draw target (DENOISE_FRAME) on the device."""
        p = denoise_params(**kw)
        self._chk(self.L.mpt_denoise(self.h, C.byref(p)), "mpt_denoise")

    def read_denoised(self):
        out = np.empty((self.height, self.width, 4), np.float32)
        self._chk(self.L.mpt_read_denoised(self.h, _fp(out)), "mpt_read_denoised")
        return out

    def denoised_buffer(self):
        """(device pointer, bytes) of the last denoise result, for zero-copy use after synchronize()."""
        p, n = C.c_void_p(), C.c_uint64()
        self._chk(self.L.mpt_denoised_buffer(self.h, C.byref(p), C.byref(n)), "mpt_denoised_buffer")
        return p.value, n.value

    def denoise_image(self, color, albedo_depth, normal_class, **kw):
        """The filter kernels on caller arrays [H,W,4] (color is filtered as given; source / samples are ignored)."""
        c = np.ascontiguousarray(color, np.float32)
        ad = np.ascontiguousarray(albedo_depth, np.float32)
        nc = np.ascontiguousarray(normal_class, np.float32)
        if c.ndim != 3 or c.shape[2] != 4 or ad.shape != c.shape or nc.shape != c.shape:
            raise ValueError("denoise_image: color, albedo_depth and normal_class must be [H, W, 4] arrays of one shape")
        H, W = c.shape[:2]
        out = np.empty_like(c)
        p = denoise_params(**kw)
        self._chk(self.L.mpt_denoise_image(self.h, W, H, _fp(c), _fp(ad), _fp(nc), C.byref(p), _fp(out)), "mpt_denoise_image")
        return out

    def read_moments(self):
        """Per-pixel second moments of the renders with FLAG_MOMENTS since the last clear: (sum v.x^2, v.y^2, v.z^2, lum^2) [H,W,4]."""
        out = np.empty((self.height, self.width, 4), np.float32)
        self._chk(self.L.mpt_read_moments(self.h, _fp(out)), "mpt_read_moments")
        return out

    def render_adaptive(self, threshold, min_samples=0, batch_samples=0, luminance_floor=0.0, **params):
        """mpt_render_adaptive: sample_count (params) is the most samples a tile gets; returns the mpt_adaptive_info as a dict."""
        p = self.params(**params)
        a = AdaptiveParams(int(min_samples), int(batch_samples), float(threshold), float(luminance_floor))
        info = AdaptiveInfo()
        self._chk(self.L.mpt_render_adaptive(self.h, C.byref(p), C.byref(a), C.byref(info)), "mpt_render_adaptive")
        return info.as_dict()

    def read_tile_samples(self):
        """Samples per 8x8 tile of the last adaptive render: (tiles_y, tiles_x) uint32."""
        out = np.empty(((self.height + 7) // 8, (self.width + 7) // 8), np.uint32)
        self._chk(self.L.mpt_read_tile_samples(self.h, _up(out)), "mpt_read_tile_samples")
        return out

    def read_adaptive_mean(self):
        """The per-pixel estimate of the last adaptive render: the HDR sum divided by its tile's sample count, in float32."""
        n = expand_tile_counts(self.read_tile_samples(), self.height, self.width).astype(np.float32)
        return self.read_sum() / n[..., None]

    def temporal_accumulate(self, **kw):
        """mpt_temporal_accumulate: blend this frame's colour (source=DENOISE_SUM, samples=spp, or DENOISE_FRAME) into the history
        reprojected from the previous camera; returns the mpt_temporal_info as a dict."""
        p = temporal_params(**kw)
        info = TemporalInfo()
        self._chk(self.L.mpt_temporal_accumulate(self.h, C.byref(p), C.byref(info)), "mpt_temporal_accumulate")
        return info.as_dict()

    def read_temporal(self):
        """The history: rgb = accumulated colour, a = history length n, [H,W,4]."""
        out = np.empty((self.height, self.width, 4), np.float32)
        self._chk(self.L.mpt_read_temporal(self.h, _fp(out)), "mpt_read_temporal")
        return out

    def temporal_buffer(self):
        """(device pointer, bytes) of the history, for zero-copy use after synchronize()."""
        p, n = C.c_void_p(), C.c_uint64()
        self._chk(self.L.mpt_temporal_buffer(self.h, C.byref(p), C.byref(n)), "mpt_temporal_buffer")
        return p.value, n.value

    def temporal_reset(self):
        self._chk(self.L.mpt_temporal_reset(self.h), "mpt_temporal_reset")

    def denoise_temporal(self, **kw):
        """mpt_denoise_temporal: the a-trous filter over the history with the current guides (read_denoised has the result)."""
        p = denoise_params(**kw)
        self._chk(self.L.mpt_denoise_temporal(self.h, C.byref(p)), "mpt_denoise_temporal")

    def temporal_image(self, color, albedo_depth, normal_class, cam, history=None, albedo_depth_prev=None, normal_class_prev=None,
                       cam_prev=None, **kw):
        """The temporal kernels on caller arrays [H,W,4] with the two cameras as Uniforms; history=None: no history.
        Returns (new history [H,W,4], info dict)."""
        c = np.ascontiguousarray(color, np.float32)
        ad = np.ascontiguousarray(albedo_depth, np.float32)
        nc = np.ascontiguousarray(normal_class, np.float32)
        if c.ndim != 3 or c.shape[2] != 4 or ad.shape != c.shape or nc.shape != c.shape:
            raise ValueError("temporal_image: color, albedo_depth and normal_class must be [H, W, 4] arrays of one shape")
        H, W = c.shape[:2]
        null = C.POINTER(C.c_float)()
        hp = adp = ncp = null
        camp = None
        if history is not None:
            h = np.ascontiguousarray(history, np.float32)
            a2 = np.ascontiguousarray(albedo_depth_prev, np.float32)
            n2 = np.ascontiguousarray(normal_class_prev, np.float32)
            if h.shape != c.shape or a2.shape != c.shape or n2.shape != c.shape or cam_prev is None:
                raise ValueError("temporal_image: the history, its guides and its camera go together, in the shape of color")
            hp, adp, ncp, camp = _fp(h), _fp(a2), _fp(n2), C.byref(cam_prev)
        out = np.empty_like(c)
        p = temporal_params(**kw)
        info = TemporalInfo()
        self._chk(self.L.mpt_temporal_image(self.h, W, H, _fp(c), _fp(ad), _fp(nc), C.byref(cam), hp, adp, ncp, camp, C.byref(p),
                                            _fp(out), C.byref(info)), "mpt_temporal_image")
        return out, info.as_dict()

    def svgf_accumulate(self, **kw):
        """mpt_svgf_accumulate: step A (reproject the illumination and its moments, blend this frame in), step B (variance) and the
        variance-guided a-trous levels; returns the mpt_svgf_info as a dict.  read_svgf() has the frame."""
        p = svgf_params(**kw)
        info = SvgfInfo()
        self._chk(self.L.mpt_svgf_accumulate(self.h, C.byref(p), C.byref(info)), "mpt_svgf_accumulate")
        return info.as_dict()

    def read_svgf(self):
        """The filtered frame: rgb, a = history length n, [H,W,4]."""
        out = np.empty((self.height, self.width, 4), np.float32)
        self._chk(self.L.mpt_read_svgf(self.h, _fp(out)), "mpt_read_svgf")
        return out

    def svgf_buffer(self):
        """(device pointer, bytes) of the filtered frame, for zero-copy use after synchronize()."""
        p, n = C.c_void_p(), C.c_uint64()
        self._chk(self.L.mpt_svgf_buffer(self.h, C.byref(p), C.byref(n)), "mpt_svgf_buffer")
        return p.value, n.value

    def read_svgf_state(self):
        """(illumination history (X, n) [H,W,4], (M1, M2, V_0, 0) [H,W,4])."""
        h = np.empty((self.height, self.width, 4), np.float32)
        mv = np.empty((self.height, self.width, 4), np.float32)
        self._chk(self.L.mpt_read_svgf_state(self.h, _fp(h), _fp(mv)), "mpt_read_svgf_state")
        return h, mv

    def svgf_reset(self):
        self._chk(self.L.mpt_svgf_reset(self.h), "mpt_svgf_reset")

    def svgf_image(self, color, albedo_depth, normal_class, cam, history=None, moments=None, albedo_depth_prev=None,
                   normal_class_prev=None, cam_prev=None, **kw):
        """The SVGF kernels on caller arrays [H,W,4] (moments [H,W,2]) with the two cameras as Uniforms; history=None: no history.
        Returns (history [H,W,4], (M1, M2, V_0, 0) [H,W,4], filtered frame [H,W,4], info dict)."""
        c = np.ascontiguousarray(color, np.float32)
        ad = np.ascontiguousarray(albedo_depth, np.float32)
        nc = np.ascontiguousarray(normal_class, np.float32)
        if c.ndim != 3 or c.shape[2] != 4 or ad.shape != c.shape or nc.shape != c.shape:
            raise ValueError("svgf_image: color, albedo_depth and normal_class must be [H, W, 4] arrays of one shape")
        H, W = c.shape[:2]
        null = C.POINTER(C.c_float)()
        hp = mp = adp = ncp = null
        camp = None
        if history is not None:
            h = np.ascontiguousarray(history, np.float32)
            m = np.ascontiguousarray(moments, np.float32)
            a2 = np.ascontiguousarray(albedo_depth_prev, np.float32)
            n2 = np.ascontiguousarray(normal_class_prev, np.float32)
            if h.shape != c.shape or m.shape != (H, W, 2) or a2.shape != c.shape or n2.shape != c.shape or cam_prev is None:
                raise ValueError("svgf_image: the history, its moments [H, W, 2], its guides and its camera go together")
            hp, mp, adp, ncp, camp = _fp(h), _fp(m), _fp(a2), _fp(n2), C.byref(cam_prev)
        ho, mv, out = np.empty_like(c), np.empty_like(c), np.empty_like(c)
        p = svgf_params(**kw)
        info = SvgfInfo()
        self._chk(self.L.mpt_svgf_image(self.h, W, H, _fp(c), _fp(ad), _fp(nc), C.byref(cam), hp, mp, adp, ncp, camp, C.byref(p),
                                        _fp(ho), _fp(mv), _fp(out), C.byref(info)), "mpt_svgf_image")
        return ho, mv, out, info.as_dict()

    def display(self, **kw):
        """mpt_display: exposure, tone curve and 8-bit encoding of a source on the device; returns the mpt_display_info as a dict.
        read_display() has the bytes."""
        p = display_params(**kw)
        info = DisplayInfo()
        self._chk(self.L.mpt_display(self.h, C.byref(p), C.byref(info)), "mpt_display")
        return info.as_dict()

    def read_display(self):
        """The finished frame: [H, W, 4] uint8 (r, g, b, 255)."""
        out = np.empty((self.height, self.width, 4), np.uint8)
        self._chk(self.L.mpt_read_display(self.h, out.ctypes.data_as(C.POINTER(C.c_uint8))), "mpt_read_display")
        return out

    def display_buffer(self):
        """(device pointer, bytes) of the finished frame, for zero-copy use after synchronize()."""
        p, n = C.c_void_p(), C.c_uint64()
        self._chk(self.L.mpt_display_buffer(self.h, C.byref(p), C.byref(n)), "mpt_display_buffer")
        return p.value, n.value

    def read_display_histogram(self):
        """The 256 luminance bins of the last display() with auto_exposure."""
        out = np.empty(256, np.uint32)
        self._chk(self.L.mpt_read_display_histogram(self.h, _up(out)), "mpt_read_display_histogram")
        return out

    def display_reset(self):
        self._chk(self.L.mpt_display_reset(self.h), "mpt_display_reset")

    def display_image(self, color, prev_auto_scale=None, **kw):
        """The display kernels on a caller array [H,W,4] (source / samples are ignored); prev_auto_scale: the auto scale kept from an
        earlier call, or None.  Returns (bytes [H,W,4] uint8, histogram [256] uint32, info dict)."""
        c = np.ascontiguousarray(color, np.float32)
        if c.ndim != 3 or c.shape[2] != 4:
            raise ValueError("display_image: color must be an [H, W, 4] array")
        H, W = c.shape[:2]
        out = np.empty((H, W, 4), np.uint8)
        hist = np.empty(256, np.uint32)
        prev = None if prev_auto_scale is None else C.byref(C.c_float(float(prev_auto_scale)))
        p = display_params(**kw)
        info = DisplayInfo()
        self._chk(self.L.mpt_display_image(self.h, W, H, _fp(c), C.byref(p), prev, out.ctypes.data_as(C.POINTER(C.c_uint8)), _up(hist),
                                           C.byref(info)), "mpt_display_image")
        return out, hist, info.as_dict()

    def kat_pcg(self, seeds):
        s = np.ascontiguousarray(seeds, np.uint32)
        h = np.empty_like(s)
        f = np.empty(s.shape, np.float32)
        self._chk(self.L.mpt_kat_pcg(self.h, _up(s), s.size, _up(h), _fp(f)), "mpt_kat_pcg")
        return h, f

    def kat_philox(self, ctr, key):
        c = np.ascontiguousarray(ctr, np.uint32).reshape(-1, 4)
        k = np.ascontiguousarray(key, np.uint32).reshape(-1, 2)
        o = np.empty_like(c)
        self._chk(self.L.mpt_kat_philox(self.h, _up(c), _up(k), c.shape[0], _up(o)), "mpt_kat_philox")
        return o

    def kat_sincos(self, u):
        u = np.ascontiguousarray(u, np.float32)
        s = np.empty_like(u)
        c = np.empty_like(u)
        self._chk(self.L.mpt_kat_sincos(self.h, _fp(u), u.size, _fp(s), _fp(c)), "mpt_kat_sincos")
        return s, c

    def kat_rcp(self):
        """rcp_chain(x) vs the correctly rounded 1.0f / x over all 2^32 operands, on the device:
        (mismatches inside the range the kernels use the chain in, operands in it, mismatches outside, operands outside)."""
        out = (C.c_uint64 * 4)()
        self._chk(self.L.mpt_kat_rcp(self.h, out), "mpt_kat_rcp")
        return tuple(int(v) for v in out)
