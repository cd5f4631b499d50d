"""raytracer_rs_amd — host-side mirror of raytracer-rs's `raytracer_lib` API over libmi355rt.so.

The names, argument meaning and error behaviour follow the reference's public surface
(/root/reference/raytracer_lib/src):

    create_raytracer(collada_doc, triangles_per_leaf, width, height)        lib.rs:15-20
    create_raytracer_from_file(collada_filename, triangles_per_leaf, w, h)   lib.rs:22-27
    RayTracer.trace_frame_additive() -> int                                  raytracer/mod.rs:80-117
    RayTracer.get_tonemapped_pixels() -> uint32[w*h] (0xAARRGGBB)            raytracer/mod.rs:120-128
    RayTracer.camera.move_rel / add_x_angle / add_y_angle                    scene/camera.rs:63-78
    RayTracer.film.clear / get_pixels / get_estimated_variances              raytracer/film.rs:37-67
    stats.Stats                                                              stats.rs:3-40
    DEFAULT_TRIANGLES_PER_LEAF = 70                                          lib.rs:7

Everything that computes runs in the HIP library through its C ABI (include/mi355rt.h).  There is
no CPU fallback here: if the shared library is missing, importing `lib()` raises, and without a GPU
`create_*` raises RuntimeError carrying the library's error text (the reference's
`Result<_, String>` error becomes the exception message).
"""
import ctypes as C
import os
import sys
import time
import weakref

import numpy as np

DEFAULT_TRIANGLES_PER_LEAF = 70

FLAG_FIX_ROW_INDEX = 1
FLAG_COUNT_STEPS = 2
FLAG_TIME_KERNELS = 4
FLAG_OCTREE_SEMANTICS = 8
FLAG_GROUP_SHARES_DEVICE = 16
FLAG_TRUE_CLOSEST_HIT = 32
FLAG_DEVICE_LBVH = 64
FLAG_DIRECT_FILM = 128
FLAG_LIGHT_FILMS = 256        # create-time: a film per light (include/mi355rt.h, "LIGHT FILMS")
LIGHT_FILMS_MAX_LIGHTS = 8

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MI355RT_LIB") or os.path.join(_HERE, "libmi355rt.so")     # MI355RT_LIB: an A/B build of the library
_lib = None


class Material(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("rgb", C.c_float * 3), ("tex_id", C.c_uint32)]


class Light(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("color", C.c_float * 3)]


class Texture(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("rgb", C.POINTER(C.c_float))]


class SceneDesc(C.Structure):
    _fields_ = [
        ("tri_verts", C.POINTER(C.c_float)), ("tri_geom", C.POINTER(C.c_uint32)), ("ntri", C.c_uint32),
        ("materials", C.POINTER(Material)), ("nmaterials", C.c_uint32),
        ("lights", C.POINTER(Light)), ("nlights", C.c_uint32),
        ("textures", C.POINTER(Texture)), ("ntextures", C.c_uint32),
        ("camera_orientation", C.c_float * 16), ("camera_fov_deg", C.c_float),
    ]


class Config(C.Structure):
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32), ("triangles_per_leaf", C.c_uint32),
        ("recursions", C.c_uint32), ("spread", C.c_uint32), ("flags", C.c_uint32),
        ("seed", C.c_uint64), ("device", C.c_int32),
        ("stripe_rows", C.c_uint32), ("stripe_rank", C.c_uint32), ("stripe_world", C.c_uint32),
        ("samples_per_pass", C.c_uint32), ("device_count", C.c_uint32),
    ]


class RayCounts(C.Structure):
    _fields_ = [
        ("primary", C.c_uint64), ("bounce", C.c_uint64), ("shadow", C.c_uint64), ("primary_hits", C.c_uint64),
        ("primary_culled", C.c_uint64),
        ("nodes_visited", C.c_uint64), ("tris_tested", C.c_uint64), ("trace_launches", C.c_uint64),
        ("inner_execs", C.c_uint64), ("leaf_execs", C.c_uint64),
        ("trace_ms", C.c_double), ("total_ms", C.c_double),
        ("trace_secondary_ms", C.c_double), ("trace_secondary_launches", C.c_uint64), ("shader_clock_mhz", C.c_double),
        ("shadow_skipped", C.c_uint64),
        ("bounce_skipped", C.c_uint64),
    ]

    def as_dict(self):
        d = {name: getattr(self, name) for name, _ in self._fields_}
        d["total_rays"] = self.primary + self.bounce + self.shadow
        d["traced_rays"] = d["total_rays"] - self.primary_culled - self.shadow_skipped - self.bounce_skipped
        return d


ADAPTIVE_TILE = 8          # MI355RT_ADAPTIVE_TILE: adaptive sampling decides per image tile of 8 x 8 pixels


class AdaptiveConfig(C.Structure):
    _fields_ = [("min_spp", C.c_uint32), ("max_spp", C.c_uint32), ("batch_spp", C.c_uint32), ("max_rounds", C.c_uint32),
                ("rel_error", C.c_float), ("abs_floor", C.c_float)]


class AdaptiveStats(C.Structure):
    _fields_ = [("rounds", C.c_uint32), ("tiles", C.c_uint32), ("tiles_active_first", C.c_uint32), ("tiles_active_last", C.c_uint32),
                ("samples_added", C.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class DenoiseConfig(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("normal_power_log2", C.c_uint32),
                ("sigma_luminance", C.c_float), ("sigma_depth", C.c_float), ("sigma_albedo", C.c_float)]


HIST_BINS = 256            # MI355RT_HIST_BINS
DISPLAY_SOURCE_FILM, DISPLAY_SOURCE_DENOISED, DISPLAY_SOURCE_DENOISED_SPLIT = 0, 1, 2
CURVE_REINHARD, CURVE_REINHARD_WHITE, CURVE_ACES, CURVE_CLAMP = 0, 1, 2, 3
TRANSFER_REFERENCE, TRANSFER_SRGB = 0, 1


class LuminanceHistogram(C.Structure):
    _fields_ = [("bins", C.c_uint32 * HIST_BINS), ("empty", C.c_uint32), ("nan", C.c_uint32), ("nonpositive", C.c_uint32), ("max_bits", C.c_uint32)]

    def as_dict(self):
        """the layout of display.histogram(): dict(bins uint32[256], empty, nan, nonpositive, max_bits)"""
        return dict(bins=np.array(self.bins, np.uint32), empty=int(self.empty), nan=int(self.nan), nonpositive=int(self.nonpositive), max_bits=int(self.max_bits))

    @classmethod
    def from_dict(cls, d):
        h = cls()
        bins = np.ascontiguousarray(d["bins"], np.uint32).reshape(HIST_BINS)
        C.memmove(h.bins, bins.ctypes.data, HIST_BINS * 4)
        h.empty, h.nan, h.nonpositive, h.max_bits = (int(d.get(k, 0)) for k in ("empty", "nan", "nonpositive", "max_bits"))
        return h


class DisplayConfig(C.Structure):
    _fields_ = [("source", C.c_uint32), ("curve", C.c_uint32), ("transfer", C.c_uint32), ("auto_exposure", C.c_uint32),
                ("exposure", C.c_float), ("white", C.c_float), ("key", C.c_float), ("low", C.c_float), ("high", C.c_float)]


RAYS_HOST, RAYS_DEVICE = 0, 1      # MI355RT_RAYS_*: where the pointers of mi355rt_trace_rays / mi355rt_render_rays live


class RayOutputs(C.Structure):
    """mi355rt_ray_outputs: any pointer may be NULL, not all of them (void pointers here: host arrays or device addresses)"""
    _fields_ = [("rgb", C.c_void_p), ("direct", C.c_void_p), ("tuv", C.c_void_p), ("prim", C.c_void_p)]


RAY_OUTPUTS = ("rgb", "direct", "tuv", "prim")

GATHER_MEAN, GATHER_COSINE = 0, 1      # MI355RT_GATHER_*
GATHER_WEIGHTS = {"mean": GATHER_MEAN, "cosine": GATHER_COSINE}


class GatherConfig(C.Structure):
    """mi355rt_gather_config (include/mi355rt.h, "GATHER")"""
    _fields_ = [("spp", C.c_uint32), ("first_sample", C.c_uint32), ("weight", C.c_uint32), ("accumulate", C.c_uint32), ("near_distance", C.c_float)]


class GatherOutputs(C.Structure):
    """mi355rt_gather_outputs: any pointer may be NULL, not all of them (void pointers here: host arrays or device addresses)"""
    _fields_ = [("n", C.c_void_p), ("hits", C.c_void_p), ("near", C.c_void_p), ("sum", C.c_void_p), ("sumsq", C.c_void_p), ("direct", C.c_void_p)]


GATHER_OUTPUTS = ("n", "hits", "near", "sum", "sumsq", "direct")

class BakeTexelOutputs(C.Structure):
    """mi355rt_bake_texel_outputs: any pointer may be NULL (void pointers here: host arrays or device addresses)"""
    _fields_ = [("owner", C.c_void_p), ("bary", C.c_void_p), ("ids", C.c_void_p), ("points", C.c_void_p), ("normals", C.c_void_p), ("albedo", C.c_void_p)]


BAKE_TEXEL_OUTPUTS = ("owner", "bary", "ids", "points", "normals", "albedo")

SH_RADIANCE, SH_IRRADIANCE = 0, 1      # MI355RT_SH_*
SH_MODES = {"radiance": SH_RADIANCE, "irradiance": SH_IRRADIANCE}


class ProbeConfig(C.Structure):
    """mi355rt_probe_config (include/mi355rt.h, "PROBES")"""
    _fields_ = [("spp", C.c_uint32), ("first_sample", C.c_uint32), ("accumulate", C.c_uint32), ("near_distance", C.c_float)]


class ProbeOutputs(C.Structure):
    """mi355rt_probe_outputs: any pointer may be NULL, not all of them (void pointers here: host arrays or device addresses); sh is npoints x 9 x 3"""
    _fields_ = [("n", C.c_void_p), ("hits", C.c_void_p), ("near", C.c_void_p), ("sh", C.c_void_p)]


class ProbeGrid(C.Structure):
    """mi355rt_probe_grid: probe (ix, iy, iz) has index (iz * ny + iy) * nx + ix and sits at origin + float(i) * spacing"""
    _fields_ = [("origin", C.c_float * 3), ("spacing", C.c_float * 3), ("counts", C.c_uint32 * 3)]

    @classmethod
    def from_dict(cls, d):
        """from the dict raytracer_rs_amd.probes uses: origin, spacing (3 floats each), counts (3 ints)"""
        g = cls()
        for a in range(3):
            g.origin[a], g.spacing[a], g.counts[a] = float(np.float32(d["origin"][a])), float(np.float32(d["spacing"][a])), int(d["counts"][a])
        return g


PROBE_OUTPUTS = ("n", "hits", "near", "sh")

VIS_CHEBYSHEV, VIS_FACING = 1, 2      # MI355RT_VIS_*


class ProbeDepth(C.Structure):
    """mi355rt_probe_depth (include/mi355rt.h, "PROBE VISIBILITY"): count is nprobes x res * res uint32, moments nprobes x res * res x 2 float32 (void pointers
    here: host arrays or device addresses)"""
    _fields_ = [("res", C.c_uint32), ("max_distance", C.c_float), ("count", C.c_void_p), ("moments", C.c_void_p)]


class ProbeVisConfig(C.Structure):
    """mi355rt_probe_vis_config: flags VIS_CHEBYSHEV | VIS_FACING, normal_bias"""
    _fields_ = [("flags", C.c_uint32), ("normal_bias", C.c_float)]


PROBE_DEPTH_OUTPUTS = PROBE_OUTPUTS + ("count", "moments")

LENS_PINHOLE, LENS_THIN, LENS_ORTHO = 0, 1, 2      # MI355RT_LENS_*
LENS_MODELS = {"pinhole": LENS_PINHOLE, "thin": LENS_THIN, "ortho": LENS_ORTHO}


GUIDES_CENTRE, GUIDES_FEATURES = 0, 1      # MI355RT_GUIDES_*: where the denoised and display read-outs take their guides from
GUIDE_SOURCES = {"centre": GUIDES_CENTRE, "features": GUIDES_FEATURES}


class Lens(C.Structure):
    """mi355rt_lens: the ray generator of render() (include/mi355rt.h, "lens models"): model LENS_*, radius and focus (THIN), width_world (ORTHO)"""
    _fields_ = [("model", C.c_uint32), ("radius", C.c_float), ("focus", C.c_float), ("width_world", C.c_float)]

    def as_dict(self):
        return dict(model={v: k for k, v in LENS_MODELS.items()}.get(self.model, self.model), radius=self.radius, focus=self.focus, width_world=self.width_world)


# every symbol include/mi355rt.h declares: (name, restype, argtypes)
_H = C.c_void_p
_F = C.POINTER(C.c_float)
_U = C.POINTER(C.c_uint32)
ABI = [
    ("mi355rt_default_config", None, [C.POINTER(Config)]),
    ("mi355rt_create", C.c_int, [C.POINTER(SceneDesc), C.POINTER(Config), C.POINTER(_H)]),
    ("mi355rt_create_from_collada_str", C.c_int, [C.c_char_p, C.c_size_t, C.c_char_p, C.POINTER(Config), C.POINTER(_H)]),
    ("mi355rt_create_from_collada_file", C.c_int, [C.c_char_p, C.POINTER(Config), C.POINTER(_H)]),
    ("mi355rt_create_from_scene_file", C.c_int, [C.c_char_p, C.POINTER(Config), C.POINTER(_H)]),
    ("mi355rt_destroy", None, [_H]),
    ("mi355rt_last_error", C.c_char_p, [_H]),
    ("mi355rt_trace_frame_additive", C.c_uint32, [_H]),
    ("mi355rt_render", C.c_int, [_H, C.c_uint32, C.POINTER(RayCounts)]),
    ("mi355rt_render_async", C.c_int, [_H, C.c_uint32]),
    ("mi355rt_last_counts", C.c_int, [_H, C.POINTER(RayCounts)]),
    ("mi355rt_adaptive_default_config", None, [C.POINTER(AdaptiveConfig)]),
    ("mi355rt_render_adaptive", C.c_int, [_H, C.POINTER(AdaptiveConfig), C.POINTER(AdaptiveStats)]),
    ("mi355rt_adaptive_tile_mask", C.c_int, [_H, C.POINTER(AdaptiveConfig), C.POINTER(C.c_uint8), C.c_size_t]),
    ("mi355rt_denoise_default_config", None, [C.POINTER(DenoiseConfig)]),
    ("mi355rt_get_denoised_pixels", C.c_int, [_H, C.POINTER(DenoiseConfig), _F, _U, C.c_size_t]),
    ("mi355rt_film_get_direct", C.c_int, [_H, _F]),
    ("mi355rt_get_denoised_pixels_split", C.c_int, [_H, C.POINTER(DenoiseConfig), _F, _U, C.c_size_t]),
    ("mi355rt_get_guides", C.c_int, [_H, _F, _F, _F, _U, C.c_size_t]),
    ("mi355rt_display_default_config", None, [C.POINTER(DisplayConfig)]),
    ("mi355rt_display_histogram", C.c_int, [_H, C.c_uint32, C.POINTER(DenoiseConfig), C.POINTER(LuminanceHistogram)]),
    ("mi355rt_display_auto_exposure", C.c_int, [C.POINTER(LuminanceHistogram), C.c_float, C.c_float, C.c_float, _F]),
    ("mi355rt_display_srgb_thresholds", C.c_int, [_F]),
    ("mi355rt_get_display_pixels", C.c_int, [_H, C.POINTER(DisplayConfig), C.POINTER(DenoiseConfig), _U, C.c_size_t, _F]),
    ("mi355rt_display_image", C.c_int, [_H, _F, C.c_size_t, C.POINTER(DisplayConfig), _U]),
    ("mi355rt_get_tonemapped_pixels", C.c_int, [_H, _U, C.c_size_t]),
    ("mi355rt_tonemap_owned_rows_device", C.c_int, [_H, C.c_void_p, C.c_size_t]),
    ("mi355rt_tonemap_owned_rows_device_on_stream", C.c_int, [_H, C.c_void_p, C.c_size_t, C.c_void_p]),
    ("mi355rt_owned_rows", C.c_uint32, [_H]),
    ("mi355rt_owned_row_list", C.c_int, [_H, _U, C.c_size_t]),
    ("mi355rt_film_get", C.c_int, [_H, _F, _F, _U]),
    ("mi355rt_film_clear", C.c_int, [_H]),
    ("mi355rt_film_set", C.c_int, [_H, _F, _F, _U, _F, C.c_size_t]),
    ("mi355rt_film_add", C.c_int, [_H, _F, _F, _U, _F, C.c_size_t]),
    ("mi355rt_film_save", C.c_int, [_H, C.c_char_p]),
    ("mi355rt_film_load", C.c_int, [_H, C.c_char_p, C.c_int]),
    ("mi355rt_film_file_info", C.c_int, [C.c_char_p, _U]),
    ("mi355rt_film_get_pixels", C.c_int, [_H, _F]),
    ("mi355rt_film_get_estimated_variances", C.c_int, [_H, _F]),
    ("mi355rt_camera_move_rel", C.c_int, [_H, C.c_float, C.c_float, C.c_float]),
    ("mi355rt_camera_add_x_angle", C.c_int, [_H, C.c_float]),
    ("mi355rt_camera_add_y_angle", C.c_int, [_H, C.c_float]),
    ("mi355rt_camera_get", C.c_int, [_H, _F, _F, _F]),
    ("mi355rt_camera_get_ray", C.c_int, [_H, C.c_uint32, C.c_uint32, C.c_float, C.c_float, _F]),
    ("mi355rt_set_seed", C.c_int, [_H, C.c_uint64]),
    ("mi355rt_set_flags", C.c_int, [_H, C.c_uint32]),
    ("mi355rt_set_slices", C.c_int, [_H, C.c_uint32]),
    ("mi355rt_get_slices", C.c_uint32, [_H]),
    ("mi355rt_intersect_rays", C.c_int, [_H, _F, C.c_size_t, _F, _U]),
    ("mi355rt_occluded_rays", C.c_int, [_H, _F, C.c_size_t, C.POINTER(C.c_uint8)]),
    ("mi355rt_trace_rays", C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(RayOutputs)]),
    ("mi355rt_render_rays", C.c_int, [_H, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(RayCounts)]),
    ("mi355rt_gather_default_config", None, [C.POINTER(GatherConfig)]),
    ("mi355rt_gather", C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(GatherConfig), C.c_uint32, C.POINTER(GatherOutputs)]),
    ("mi355rt_gather_ray", C.c_int, [_F, C.c_uint32, _F, _F, C.c_uint32, C.c_uint32, _F, _U]),
    ("mi355rt_bake_texels", C.c_int, [_H, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(BakeTexelOutputs), _U]),
    ("mi355rt_bake_atlas", C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("mi355rt_bake_texel", C.c_int, [_F, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _U, _F]),
    ("mi355rt_bake_point", C.c_float, [C.c_float, C.c_float, C.c_float, C.c_float, C.c_float]),
    ("mi355rt_bake_dilate_texel", C.c_uint32, [_F, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _F]),
    ("mi355rt_bake_auto_atlas", C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _F, _U]),
    ("mi355rt_probes_default_config", None, [C.POINTER(ProbeConfig)]),
    ("mi355rt_probes_gather", C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(ProbeConfig), C.c_uint32, C.POINTER(ProbeOutputs)]),
    ("mi355rt_probes_lookup", C.c_int, [_H, C.POINTER(ProbeGrid), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32,
                                        C.c_void_p, C.c_void_p]),
    ("mi355rt_sh9_basis", C.c_int, [_F, _F]),
    ("mi355rt_probes_lookup_one", C.c_int, [C.POINTER(ProbeGrid), _U, _F, C.POINTER(C.c_uint8), _F, _F, C.c_uint32, _F, _U]),
    ("mi355rt_probe_grid_points", C.c_int, [C.POINTER(ProbeGrid), _F]),
    ("mi355rt_probes_vis_default_config", None, [C.POINTER(ProbeVisConfig)]),
    ("mi355rt_probes_gather_depth", C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(ProbeConfig), C.c_uint32, C.POINTER(ProbeOutputs), C.POINTER(ProbeDepth)]),
    ("mi355rt_probes_lookup_vis", C.c_int, [_H, C.POINTER(ProbeGrid), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ProbeDepth), C.POINTER(ProbeVisConfig), C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("mi355rt_oct_encode", C.c_int, [_F, _F]),
    ("mi355rt_oct_texel", C.c_int, [_F, C.c_uint32, _U]),
    ("mi355rt_probe_visibility_one", C.c_int, [C.POINTER(ProbeDepth), _F, _F]),
    ("mi355rt_probes_lookup_vis_one", C.c_int, [C.POINTER(ProbeGrid), _U, _F, C.POINTER(C.c_uint8), C.POINTER(ProbeDepth), C.POINTER(ProbeVisConfig), _F, _F, _F, C.c_uint32, _F, _U]),
    ("mi355rt_lens_default", None, [C.POINTER(Lens)]),
    ("mi355rt_set_lens", C.c_int, [_H, C.POINTER(Lens)]),
    ("mi355rt_get_lens", C.c_int, [_H, C.POINTER(Lens)]),
    ("mi355rt_lens_ray", C.c_int, [_F, _F, _F, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Lens), C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_float, _F]),
    ("mi355rt_lens_rays", C.c_int, [_H, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t]),
    ("mi355rt_render_tiles", C.c_int, [_H, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(RayCounts)]),
    ("mi355rt_features_render", C.c_int, [_H, C.c_uint32]),
    ("mi355rt_features_render_rays", C.c_int, [_H, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32]),
    ("mi355rt_features_get", C.c_int, [_H, _U, _U, _F, _F, _F, C.c_size_t]),
    ("mi355rt_features_clear", C.c_int, [_H]),
    ("mi355rt_features_alpha", C.c_int, [_H, _F, C.c_size_t]),
    ("mi355rt_light_count", C.c_uint32, [_H]),
    ("mi355rt_light_films_get", C.c_int, [_H, _F, C.c_size_t, C.c_size_t]),
    ("mi355rt_light_films_set", C.c_int, [_H, _F, C.c_size_t, C.c_size_t]),
    ("mi355rt_light_films_add", C.c_int, [_H, _F, C.c_size_t, C.c_size_t]),
    ("mi355rt_get_relit_pixels", C.c_int, [_H, _F, C.c_size_t, C.c_void_p, _F, _U, C.c_size_t, _F]),
    ("mi355rt_set_guide_source", C.c_int, [_H, C.c_uint32]),
    ("mi355rt_get_guide_source", C.c_uint32, [_H]),
    ("mi355rt_get_sample_table", C.c_int, [_H, _F]),
    ("mi355rt_debug_sample", C.c_int, [_H, C.c_uint32, C.c_uint32, _F, _F, C.c_size_t]),
    ("mi355rt_debug_numerics", C.c_int, [_H, _F, _F, C.c_size_t, _F, _F, _F]),
    ("mi355rt_debug_slab", C.c_int, [_H, _F, _F, C.c_size_t, C.POINTER(C.c_uint8), _F]),
    ("mi355rt_tree_nodes", C.c_uint32, [_H]),
    ("mi355rt_debug_speculation", C.c_int, [_H, C.POINTER(C.c_uint64)]),
    ("mi355rt_debug_light_map", C.c_int, [_F, C.c_uint32, _F, C.c_double, C.c_uint32, _F, C.POINTER(C.c_double)]),
    ("mi355rt_debug_reflect_mask", C.c_int, [_F, C.c_uint32, C.c_double, C.c_uint32, C.c_uint64, _U, C.POINTER(C.c_double)]),
    ("mi355rt_reflect_mask_info", C.c_int, [_H, C.POINTER(C.c_double)]),
    ("mi355rt_debug_rays_read", C.c_int, [_H, C.POINTER(C.c_uint64)]),
    ("mi355rt_debug_wide_bvh", C.c_int, [_F, C.c_uint32, _U]),
    ("mi355rt_debug_octree", C.c_int, [_F, C.c_uint32, C.c_uint32, _U, _F, C.POINTER(C.c_int32), _U, _U, _U, C.c_size_t, _U, C.c_size_t]),
    ("mi355rt_debug_bvh_read", C.c_int, [_H, _F, _U, C.c_uint32, _U, _F, _U, C.c_size_t, _U, C.c_size_t]),
    ("mi355rt_accel_stats", C.c_int, [_H, _U]),
    ("mi355rt_octree_stats", C.c_int, [_H, _U]),
    ("mi355rt_bvh_build_info", C.c_int, [_H, _U]),
    ("mi355rt_device_count", C.c_uint32, [_H]),
    ("mi355rt_synchronize", C.c_int, [_H]),
    ("mi355rt_comm_unique_id", C.c_int, [C.POINTER(C.c_uint8)]),
    ("mi355rt_comm_available", C.c_int, [_H]),
    ("mi355rt_comm_init", C.c_int, [_H, C.POINTER(C.c_uint8)]),
    ("mi355rt_comm_gather_frame", C.c_int, [_H, C.c_uint32, _U, C.c_size_t]),
    ("mi355rt_comm_destroy", C.c_int, [_H]),
    ("mi355rt_comm_ranks", C.c_uint32, [_H]),
    ("mi355rt_hbm_allocated_bytes", C.c_uint64, [_H]),
    ("mi355rt_debug_check_guards", C.c_int64, [_H]),
    ("mi355rt_debug_gather_rate", C.c_int, [_H, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]),
    ("mi355rt_width", C.c_uint32, [_H]),
    ("mi355rt_height", C.c_uint32, [_H]),
    ("mi355rt_triangle_count", C.c_uint32, [_H]),
    ("mi355rt_current_row", C.c_uint32, [_H]),
]


def lib():
    """Load libmi355rt.so (built by `make -C raytracer-rs_amd` / __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "libmi355rt.so is not built (%s); run __graft_entry__.build() — there is no CPU fallback" % LIB_PATH)
        # PyTorch ships its own copy of the HIP runtime.  A process that uses both (tests, bench.py: torch buffers and streams are
        # handed to the library) must have torch's copy loaded FIRST, so that libmi355rt.so's libamdhip64 dependency resolves to
        # the runtime already in the process instead of bringing /opt/rocm's as a second one.  Done here, once, for whoever has
        # torch imported already; a host without torch (the C++ CLI, a Rust binary) never meets the question.
        if "torch" in sys.modules:
            try:
                sys.modules["torch"].cuda.is_available()
            except Exception:       # noqa: BLE001 — a CPU-only torch build
                pass
        L = C.CDLL(LIB_PATH)
        for name, res, args in ABI:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _fp(a):
    return a.ctypes.data_as(_F)


def _up(a):
    return a.ctypes.data_as(_U)


def _is_tensor(a):
    """a torch tensor (without importing torch for callers that never hand one in)"""
    t = sys.modules.get("torch")
    return t is not None and isinstance(a, t.Tensor)


def _ray_array(a, name, cols, dtype, rows=None):
    """Check one array argument of trace_rays / render_rays BEFORE any library call: a C-contiguous numpy array (host) or torch tensor on a GPU
    (device) of exactly this dtype and shape (rows, cols); a uint32 argument may be a torch.int32 tensor holding the same bits (torch has little uint32
    support).  Returns (address, rows, is_device)."""
    want = np.dtype(dtype).name
    if _is_tensor(a):
        if a.device.type != "cuda":
            raise ValueError("%s: a torch tensor must live on the handle's GPU (it is on %s); pass a numpy array for host memory" % (name, a.device))
        if str(a.dtype).replace("torch.", "") not in ((want, "int32") if want == "uint32" else (want,)):
            raise TypeError("%s: dtype must be %s, not %s" % (name, want, a.dtype))
        shape, contiguous, addr, dev = tuple(a.shape), a.is_contiguous(), a.data_ptr(), True
    elif isinstance(a, np.ndarray):
        if a.dtype != np.dtype(dtype):
            raise TypeError("%s: dtype must be %s, not %s" % (name, want, a.dtype))
        shape, contiguous, addr, dev = a.shape, a.flags["C_CONTIGUOUS"], a.ctypes.data, False
    else:
        raise TypeError("%s: a numpy array or a torch tensor, not %s" % (name, type(a).__name__))
    if len(shape) != 2 or shape[1] != cols or (rows is not None and shape[0] != rows):
        raise ValueError("%s: shape must be (%s, %d), not %s" % (name, "n" if rows is None else rows, cols, tuple(shape)))
    if not contiguous:
        raise ValueError("%s: must be C-contiguous" % name)
    return addr, shape[0], dev


def _ray_vector(a, name, dtype, rows):
    """_ray_array for a one-dimensional argument (rows,): checked as the (rows, 1) view of the same memory"""
    if (_is_tensor(a) and a.dim() == 1 and a.is_contiguous()) or (isinstance(a, np.ndarray) and a.ndim == 1 and a.flags["C_CONTIGUOUS"]):
        return _ray_array(a.reshape(-1, 1), name, 1, dtype, rows=rows)
    if _is_tensor(a) or isinstance(a, np.ndarray):
        raise ValueError("%s: shape must be (%d,) and C-contiguous, not %s" % (name, rows, tuple(a.shape)))
    raise TypeError("%s: a numpy array or a torch tensor, not %s" % (name, type(a).__name__))


def _film_array(a, name, shape, dtype):
    """_ray_array for an argument of exactly this shape (rows, ...): checked as the (rows, rest) view of the same memory"""
    if not (_is_tensor(a) or isinstance(a, np.ndarray)):
        raise TypeError("%s: a numpy array or a torch tensor, not %s" % (name, type(a).__name__))
    if tuple(a.shape) != tuple(shape):
        raise ValueError("%s: shape must be %s, not %s" % (name, tuple(shape), tuple(a.shape)))
    if not (a.is_contiguous() if _is_tensor(a) else a.flags["C_CONTIGUOUS"]):
        raise ValueError("%s: must be C-contiguous" % name)                 # before the reshape, which would copy
    rest = int(np.prod(shape[1:], dtype=np.int64))
    return _ray_array(a.reshape(shape[0], rest), name, rest, dtype, rows=shape[0])


# ---- what the array-taking methods share: the checks of want / into / max_distance and the making of outputs, host or device ----
def _check_want(want, allowed, empty_ok=False):
    """want as a tuple: a selection of `allowed` without repeats, non-empty unless empty_ok"""
    want = tuple(want)
    if (not want and not empty_ok) or any(w not in allowed for w in want) or len(set(want)) != len(want):
        raise ValueError("want: a %sselection of %s without repeats, not %r" % ("" if empty_ok else "non-empty ", allowed, want))
    return want


def _input_beside(a, name, dtype, rows, cols, dev, anchor, optional=True):
    """The address of an input that goes with an anchor input: (rows, cols), or with cols None (rows,), checked, and in the anchor's place (dev: the anchor's
    is_device; anchor: "points live").  optional: None is accepted and gives None"""
    if a is None and optional:
        return None
    addr, _, adev = _ray_vector(a, name, dtype, rows) if cols is None else _ray_array(a, name, cols, dtype, rows=rows)
    if adev != dev:
        raise ValueError("%s must live where %s (both numpy arrays, or both tensors on the GPU)" % (name, anchor))
    return addr


def _device_of(a):
    """where outputs for the input `a` go: its torch device, None for host memory"""
    return a.device if _is_tensor(a) else None


def _sync(device):
    """torch's stream on `device` has finished what it was given (inputs, zero fills): the library's stream knows nothing of torch's.  None: host memory, nothing to do"""
    if device is not None:
        import torch
        torch.cuda.current_stream(device).synchronize()


def _new_output(shape, dtype, device=None):
    """A zeroed output of dtype uint32, uint8 or float32: a numpy array, or on a torch device a tensor there (uint32 as torch.int32 holding the same bits)"""
    if device is None:
        return np.zeros(shape, dtype)
    import torch
    return torch.zeros(shape, dtype={"uint32": torch.int32, "uint8": torch.uint8, "float32": torch.float32}[np.dtype(dtype).name], device=device)


def _address(a):
    return a.data_ptr() if _is_tensor(a) else a.ctypes.data


def _output(struct, field, shape, dtype, device, into=None, misplaced=None):
    """The output `field` of a call: into[field], checked (shape, dtype, contiguous, host or device as `device` says), or with into None a new one.  Its address
    goes into struct.field; returns the array.  misplaced: the message for an into entry in the wrong place"""
    if into is None:
        a = _new_output(shape, dtype, device)
        addr = _address(a)
    else:
        if field not in into:
            raise ValueError("into: holds no %r" % field)
        a, label = into[field], "into[%r]" % field
        if len(shape) == 1:
            addr, _, adev = _ray_vector(a, label, dtype, shape[0])
        elif len(shape) == 2 and shape[1] == 3:                             # rows of three: checked as gather and probe_lit_rays always did, the dtype first
            addr, _, adev = _ray_array(a, label, 3, dtype, rows=shape[0])
        else:
            addr, _, adev = _film_array(a, label, shape, dtype)
        if adev != (device is not None):
            raise ValueError(misplaced or "into[%r] must live where points live" % field)
    setattr(struct, field, addr)
    return a


def _rgb_ok(m, want_ok, device):
    """(rgb, ok, their addresses): the float32 (m, 3) and, with want_ok, uint8 (m,) outputs of a read-out, with _sync behind the zero fills"""
    rgb, ok = _new_output((m, 3), np.float32, device), _new_output((m,), np.uint8, device) if want_ok else None
    _sync(device)
    return rgb, ok, _address(rgb), _address(ok) if want_ok else None


def _reconcile_max_distance(max_distance, into, res=None):
    """max_distance as the f32 value the library takes: finite, > 0, <= 1e12.  into: the dict of the call that is continued (or None): it holds max_distance —
    with res its depth film's depth_res too — which must agree; a max_distance of None takes into's"""
    if into is not None:
        if "max_distance" not in into or (res is not None and "depth_res" not in into):
            raise ValueError("into: holds no depth film (depth_res, max_distance)" if res is not None else "into: holds no max_distance")
        if max_distance is None:
            max_distance = into["max_distance"]
        same = float(np.float32(into["max_distance"])) == float(np.float32(max_distance))
        if res is not None and (int(into["depth_res"]) != res or not same):
            raise ValueError("into: its depth film has res %r and max_distance %r, not %r and %r" % (into["depth_res"], into["max_distance"], res, max_distance))
        if not same:
            raise ValueError("into: its survey has max_distance %r, not %r" % (into["max_distance"], max_distance))
    if max_distance is None:
        raise ValueError("max_distance: give one (probes.grid_max_distance(grid) is the usual choice)")
    max_distance = float(np.float32(max_distance))
    if res is not None and not 2 <= res <= 16:
        raise ValueError("res: 2 .. 16, not %r" % res)
    if not (np.isfinite(max_distance) and 0.0 < max_distance <= 1e12):
        raise ValueError("max_distance: finite, > 0 and <= 1e12, not %r" % max_distance)
    return max_distance


def default_config(width=1024, height=768, **kw):
    cfg = Config()
    lib().mi355rt_default_config(C.byref(cfg))
    cfg.width, cfg.height = int(width), int(height)
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise TypeError("unknown config field %r" % k)
        setattr(cfg, k, v)
    return cfg


def adaptive_config(**kw):
    """mi355rt_adaptive_default_config with the given fields replaced (min_spp, max_spp, batch_spp, max_rounds, rel_error, abs_floor)"""
    cfg = AdaptiveConfig()
    lib().mi355rt_adaptive_default_config(C.byref(cfg))
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise TypeError("unknown adaptive config field %r" % k)
        setattr(cfg, k, v)
    return cfg


def denoise_config(**kw):
    """mi355rt_denoise_default_config with the given fields replaced (iterations, normal_power_log2, sigma_luminance, sigma_depth, sigma_albedo)"""
    cfg = DenoiseConfig()
    lib().mi355rt_denoise_default_config(C.byref(cfg))
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise TypeError("unknown denoise config field %r" % k)
        setattr(cfg, k, v)
    return cfg


def display_config(**kw):
    """mi355rt_display_default_config with the given fields replaced (source, curve, transfer, auto_exposure, exposure, white, key, low, high)"""
    cfg = DisplayConfig()
    lib().mi355rt_display_default_config(C.byref(cfg))
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise TypeError("unknown display config field %r" % k)
        setattr(cfg, k, v)
    return cfg


def make_lens(model="pinhole", radius=None, focus=None, width_world=None):
    """A Lens: mi355rt_lens_default with the given fields replaced; model: "pinhole", "thin", "ortho" or a LENS_* number.  Not validated here."""
    l = Lens()
    lib().mi355rt_lens_default(C.byref(l))
    l.model = LENS_MODELS[model] if isinstance(model, str) else int(model)
    for k, v in (("radius", radius), ("focus", focus), ("width_world", width_world)):
        if v is not None:
            setattr(l, k, v)
    return l


def lens_ray(cam, width, height, lens, pixel, xi1=0.5, xi2=0.5, l1=0.5, l2=0.5, flags=0):
    """mi355rt_lens_ray (host code, no device): float32[6] (pos3, dir3), the ray of `pixel` under `lens` (a Lens, see make_lens) for the jitter
    (xi1, xi2) and the lens sample (l1, l2); cam = (rot16, orient16, max_xy) as RayTracer.camera.matrices() returns them; flags bit 0:
    FLAG_FIX_ROW_INDEX.  The defaults give the guide ray of the pixel.  Raises RuntimeError naming the argument for an invalid one."""
    rot, orient, mx = (np.ascontiguousarray(a, np.float32).reshape(-1) for a in cam)
    if rot.size != 16 or orient.size != 16 or mx.size != 2:
        raise ValueError("cam must be (rot16, orient16, max_xy) as RayTracer.camera.matrices() returns them")
    out = np.zeros(6, np.float32)
    if lib().mi355rt_lens_ray(_fp(rot), _fp(orient), _fp(mx), int(width), int(height), int(flags), C.byref(lens), int(pixel), xi1, xi2, l1, l2, _fp(out)) != 0:
        raise RuntimeError((lib().mi355rt_last_error(None) or b"").decode() or "mi355rt_lens_ray failed")
    return out


def display_auto_exposure(hist, key=0.18, low=0.0, high=1.0):
    """mi355rt_display_auto_exposure (host code, no device): the exposure (numpy float32) a luminance histogram gives; hist: a LuminanceHistogram,
    or the dict RayTracer.display_histogram() / display.histogram() return.  Raises RuntimeError naming the field for an invalid key, low or high."""
    h = hist if isinstance(hist, LuminanceHistogram) else LuminanceHistogram.from_dict(hist)
    out = C.c_float(0.0)
    if lib().mi355rt_display_auto_exposure(C.byref(h), key, low, high, C.byref(out)) != 0:
        raise RuntimeError((lib().mi355rt_last_error(None) or b"").decode() or "mi355rt_display_auto_exposure failed")
    return np.float32(out.value)


def display_srgb_thresholds():
    """mi355rt_display_srgb_thresholds (host code, no device): float32[255], T[1..255] of the sRGB transfer"""
    out = np.zeros(255, np.float32)
    if lib().mi355rt_display_srgb_thresholds(_fp(out)) != 0:
        raise RuntimeError((lib().mi355rt_last_error(None) or b"").decode() or "mi355rt_display_srgb_thresholds failed")
    return out


class Camera:
    """scene/camera.rs — the `pub camera` field of RayTracer (mod.rs:38)."""

    def __init__(self, rt):
        self._rt = rt

    def move_rel(self, x, y, z):
        self._rt._check(lib().mi355rt_camera_move_rel(self._rt._h, x, y, z))

    def add_x_angle(self, radians):
        self._rt._check(lib().mi355rt_camera_add_x_angle(self._rt._h, radians))

    def add_y_angle(self, radians):
        self._rt._check(lib().mi355rt_camera_add_y_angle(self._rt._h, radians))

    def matrices(self):
        rot = np.zeros(16, np.float32); orient = np.zeros(16, np.float32); mx = np.zeros(2, np.float32)
        self._rt._check(lib().mi355rt_camera_get(self._rt._h, _fp(rot), _fp(orient), _fp(mx)))
        return rot, orient, mx

    def get_ray(self, u, v, xi1, xi2):
        ray = np.zeros(6, np.float32)
        self._rt._check(lib().mi355rt_camera_get_ray(self._rt._h, u, v, xi1, xi2, _fp(ray)))
        return ray


class Film:
    """raytracer/film.rs — the `pub film` field of RayTracer (mod.rs:41)."""

    def __init__(self, rt):
        self._rt = rt

    def clear(self):
        self._rt._check(lib().mi355rt_film_clear(self._rt._h))

    def pixel_datas(self):
        """(pixel_sum[n,3], pixel_sum_squared[n,3], num_samples[n]) — film.rs:3-8"""
        n = self._rt.width * self._rt.height
        s = np.zeros((n, 3), np.float32); q = np.zeros((n, 3), np.float32); c = np.zeros(n, np.uint32)
        self._rt._check(lib().mi355rt_film_get(self._rt._h, _fp(s), _fp(q), _up(c)))
        return s, q, c

    def direct_sums(self):
        """direct[n,3]: per pixel, the sum of its samples' root light terms (a handle created with FLAG_DIRECT_FILM; mi355rt_film_get_direct)"""
        d = np.zeros((self._rt.width * self._rt.height, 3), np.float32)
        self._rt._check(lib().mi355rt_film_get_direct(self._rt._h, _fp(d)))
        return d

    def _put(self, fn, sum, sumsq, n, direct):
        s = np.ascontiguousarray(sum, np.float32); q = np.ascontiguousarray(sumsq, np.float32); c = np.ascontiguousarray(n, np.uint32)
        d = None if direct is None else np.ascontiguousarray(direct, np.float32)
        if s.size != 3 * c.size or q.size != 3 * c.size or (d is not None and d.size != 3 * c.size):
            raise ValueError("film planes: sum, sumsq and direct hold 3 floats per entry of n")
        self._rt._check(fn(self._rt._h, _fp(s), _fp(q), _up(c), None if d is None else _fp(d), c.size))

    def set(self, sum, sumsq, n, direct=None):
        """mi355rt_film_set: the film becomes these planes (the layout of pixel_datas() / direct_sums()), bits unchanged, on the rows the handle
        owns.  direct: required exactly when the handle was created with FLAG_DIRECT_FILM."""
        self._put(lib().mi355rt_film_set, sum, sumsq, n, direct)

    def add(self, sum, sumsq, n, direct=None):
        """mi355rt_film_add: film = film + planes, one f32 addition per value (u32 for n), on the rows the handle owns"""
        self._put(lib().mi355rt_film_add, sum, sumsq, n, direct)

    def save(self, path):
        """mi355rt_film_save: the film as a film file (include/mi355rt.h; raytracer_rs_amd.film_io reads and writes the same format)"""
        self._rt._check(lib().mi355rt_film_save(self._rt._h, os.fsencode(path)))

    def load(self, path, add=False):
        """mi355rt_film_load: set (or, add=True, add) the planes of a film file; the file is checked whole before the film is touched"""
        self._rt._check(lib().mi355rt_film_load(self._rt._h, os.fsencode(path), 1 if add else 0))

    def get_pixels(self):
        out = np.zeros((self._rt.width * self._rt.height, 3), np.float32)
        self._rt._check(lib().mi355rt_film_get_pixels(self._rt._h, _fp(out)))
        return out

    def get_estimated_variances(self):
        out = np.zeros((self._rt.width * self._rt.height, 3), np.float32)
        self._rt._check(lib().mi355rt_film_get_estimated_variances(self._rt._h, _fp(out)))
        return out


class Features:
    """The feature film of a RayTracer (include/mi355rt.h, "FEATURE FILM"): per pixel, the primary hits' depth, normal and albedo summed
    over jittered samples, and how many samples hit.  raytracer_rs_amd.features states the arithmetic in numpy."""

    def __init__(self, rt):
        self._rt = rt

    def render(self, spp):
        """mi355rt_features_render: spp samples per owned pixel under the handle's lens, keys (p, feat_n[p] + s): the rays a cleared film's render(spp) takes"""
        spp = int(spp)
        if spp < 0:
            raise ValueError("spp must be >= 1")
        self._rt._check(lib().mi355rt_features_render(self._rt._h, spp))

    def render_rays(self, rays6, spp):
        """mi355rt_features_render_rays: the same accumulation along the caller's rays; rays6 and spp as RayTracer.render_rays takes them (a numpy array,
        or a torch tensor on the handle's GPU, which is read in place)"""
        spp = int(spp)
        if spp < 0:
            raise ValueError("spp must be >= 1")
        addr, n, dev = _ray_array(rays6, "rays6", 6, np.float32)
        if dev:
            import torch
            torch.cuda.current_stream(rays6.device).synchronize()
        self._rt._check(lib().mi355rt_features_render_rays(self._rt._h, addr, n, spp, RAYS_DEVICE if dev else RAYS_HOST))

    def get(self):
        """mi355rt_features_get: dict(n uint32[npix], hits uint32[npix], depth float32[npix], normal float32[npix, 3], albedo float32[npix, 3])"""
        n = self._rt.width * self._rt.height
        p = dict(n=np.zeros(n, np.uint32), hits=np.zeros(n, np.uint32), depth=np.zeros(n, np.float32),
                 normal=np.zeros((n, 3), np.float32), albedo=np.zeros((n, 3), np.float32))
        self._rt._check(lib().mi355rt_features_get(self._rt._h, _up(p["n"]), _up(p["hits"]), _fp(p["depth"]), _fp(p["normal"]), _fp(p["albedo"]), n))
        return p

    def alpha(self):
        """mi355rt_features_alpha: float32[npix], hits / n (0 where n == 0): the share of a pixel's samples that hit the scene"""
        out = np.zeros(self._rt.width * self._rt.height, np.float32)
        self._rt._check(lib().mi355rt_features_alpha(self._rt._h, _fp(out), out.size))
        return out

    def clear(self):
        """mi355rt_features_clear: zero planes (owned rows), no view stamp"""
        self._rt._check(lib().mi355rt_features_clear(self._rt._h))


class LightFilms:
    """The light films of a RayTracer created with FLAG_LIGHT_FILMS (include/mi355rt.h, "LIGHT FILMS"): per light, a plane of the film's
    shape that holds the sum of every sample's light radiance — the sample's colour with every other light black.  Arrays are float32[nlights, npix, 3].
    raytracer_rs_amd.relight states the relit read-out in numpy."""

    def __init__(self, rt):
        self._rt = rt

    def _planes(self, a):
        a = np.ascontiguousarray(a, np.float32)
        nl, n = self._rt.nlights, self._rt.width * self._rt.height
        if a.shape != (nl, n, 3):
            raise ValueError("light films: shape must be (%d, %d, 3), not %s" % (nl, n, a.shape))
        return a

    def get(self):
        """mi355rt_light_films_get: float32[nlights, npix, 3]"""
        nl, n = self._rt.nlights, self._rt.width * self._rt.height
        out = np.zeros((nl, n, 3), np.float32)
        self._rt._check(lib().mi355rt_light_films_get(self._rt._h, _fp(out) if nl else None, nl, n))
        return out

    def set(self, a):
        """mi355rt_light_films_set: the planes' bits as they are, on the rows the handle owns"""
        a = self._planes(a)
        self._rt._check(lib().mi355rt_light_films_set(self._rt._h, _fp(a) if a.size else None, a.shape[0], a.shape[1]))

    def add(self, a):
        """mi355rt_light_films_add: handle + a, one f32 addition per value, on the rows the handle owns"""
        a = self._planes(a)
        self._rt._check(lib().mi355rt_light_films_add(self._rt._h, _fp(a) if a.size else None, a.shape[0], a.shape[1]))


class RayTracer:
    """raytracer/mod.rs:32-47.  Construct through create_raytracer* below."""

    def __init__(self, handle, keepalive=None, device_index=0):
        self._h = C.c_void_p(handle)
        self._keep = keepalive
        self.device_index = int(device_index)     # config.device: the HIP device of the handle (of device 0 of a group)
        L = lib()
        self.width = L.mi355rt_width(self._h)
        self.height = L.mi355rt_height(self._h)
        # weak back-references: no reference cycle, so dropping the last reference to a RayTracer destroys the handle (and
        # frees its tens of GB of pass buffers) at once instead of whenever the cycle collector runs
        self.camera = Camera(weakref.proxy(self))
        self.film = Film(weakref.proxy(self))
        self.features = Features(weakref.proxy(self))
        self.nlights = int(L.mi355rt_light_count(self._h))
        self.light_films = LightFilms(weakref.proxy(self))

    def close(self):
        if self._h:
            lib().mi355rt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, code):
        if code != 0:
            raise RuntimeError((lib().mi355rt_last_error(self._h) or b"").decode() or "mi355rt error %d" % code)

    # --- the reference's methods
    def trace_frame_additive(self):
        n = lib().mi355rt_trace_frame_additive(self._h)
        if n == 0:
            self._check(-4)
        return n

    def get_tonemapped_pixels(self, out=None):
        """width*height u32 0xAARRGGBB; `out` (uint32[width*height]) is reused when given"""
        if out is None:
            out = np.empty(self.width * self.height, np.uint32)
        self._check(lib().mi355rt_get_tonemapped_pixels(self._h, _up(out), out.size))
        return out

    # --- additions (no reference counterpart)
    def render(self, spp, wait=True):
        """whole frame (owned stripes) x spp; wait=False only queues it (mi355rt_render_async) and returns None: last_counts() waits"""
        if not wait:
            self._check(lib().mi355rt_render_async(self._h, int(spp)))
            return None
        rc = RayCounts()
        self._check(lib().mi355rt_render(self._h, int(spp), C.byref(rc)))
        return rc

    def last_counts(self):
        rc = RayCounts()
        self._check(lib().mi355rt_last_counts(self._h, C.byref(rc)))
        return rc

    def render_adaptive(self, **cfg):
        """Adaptive sampling (include/mi355rt.h, mi355rt_render_adaptive): rounds of batch_spp samples in the tiles whose noise is above the
        target until none is left.  Fields not given keep mi355rt_adaptive_default_config's values.  Returns the stats as a dict;
        last_counts() holds the call's ray counters."""
        c = adaptive_config(**cfg)
        st = AdaptiveStats()
        self._check(lib().mi355rt_render_adaptive(self._h, C.byref(c), C.byref(st)))
        return st.as_dict()

    def adaptive_tile_mask(self, **cfg):
        """the verdict the next adaptive round would use: uint8[tiles_y, tiles_x], 1 = active"""
        c = adaptive_config(**cfg)
        tx = (self.width + ADAPTIVE_TILE - 1) // ADAPTIVE_TILE
        ty = (self.height + ADAPTIVE_TILE - 1) // ADAPTIVE_TILE
        out = np.zeros((ty, tx), np.uint8)
        rc = lib().mi355rt_adaptive_tile_mask(self._h, C.byref(c), out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size)
        if rc < 0:
            self._check(rc)
        assert rc == int(out.sum())
        return out

    def render_tiles(self, mask, spp):
        """mi355rt_render_tiles: spp samples into the tiles of `mask`, under whatever lens the handle has.  mask: uint8[tiles_y, tiles_x] or flat — a numpy
        array (host), or a torch uint8 tensor on the handle's GPU, which is read in place.  Non-zero selects a tile.  Returns the call's counters."""
        tx = (self.width + ADAPTIVE_TILE - 1) // ADAPTIVE_TILE
        ty = (self.height + ADAPTIVE_TILE - 1) // ADAPTIVE_TILE
        if _is_tensor(mask):
            if mask.device.type != "cuda":
                raise ValueError("mask: a torch tensor must live on the handle's GPU (it is on %s); pass a numpy array for host memory" % (mask.device,))
            if mask.device.index not in (None, self.device_index):
                raise ValueError("mask: the tensor lives on GPU %d, the handle on GPU %d" % (mask.device.index, self.device_index))
            if str(mask.dtype) != "torch.uint8":
                raise TypeError("mask: dtype must be uint8, not %s" % (mask.dtype,))
            if not mask.is_contiguous():
                raise ValueError("mask: must be C-contiguous")
            shape, addr, where, keep = tuple(mask.shape), mask.data_ptr(), RAYS_DEVICE, mask
        else:
            keep = np.ascontiguousarray(mask)
            if keep.dtype != np.uint8:
                raise TypeError("mask: dtype must be uint8, not %s" % keep.dtype)
            shape, addr, where = keep.shape, keep.ctypes.data, RAYS_HOST
        if shape not in ((ty, tx), (ty * tx,)):
            raise ValueError("mask: shape must be (%d, %d) or (%d,), not %s" % (ty, tx, ty * tx, tuple(shape)))
        rc = RayCounts()
        self._check(lib().mi355rt_render_tiles(self._h, C.c_void_p(addr), ty * tx, int(spp), where, C.byref(rc)))
        return rc

    def refine(self, **cfg):
        """The adaptive loop on the caller's side (adaptive.refine): adaptive_tile_mask, then render_tiles, until no tile is active — under any lens."""
        from . import adaptive
        return adaptive.refine(self, **cfg)

    def get_denoised_pixels(self, rgb=True, packed=True, split=False, **cfg):
        """The denoised read-out of the film (include/mi355rt.h, mi355rt_get_denoised_pixels).  Fields not given keep
        mi355rt_denoise_default_config's values.  Returns (rgb float32[npix, 3] or None, packed uint32[npix] or None).
        split=True (a handle created with FLAG_DIRECT_FILM): mi355rt_get_denoised_pixels_split, which filters the indirect part only."""
        c = denoise_config(**cfg)
        n = self.width * self.height
        out_rgb = np.zeros((n, 3), np.float32) if rgb else None
        out_packed = np.zeros(n, np.uint32) if packed else None
        fn = lib().mi355rt_get_denoised_pixels_split if split else lib().mi355rt_get_denoised_pixels
        self._check(fn(self._h, C.byref(c), _fp(out_rgb) if rgb else None, _up(out_packed) if packed else None, n))
        return out_rgb, out_packed

    def display_histogram(self, source=0, **dn):
        """The luminance histogram of a source image (include/mi355rt.h, mi355rt_display_histogram): dict(bins uint32[256], empty, nan, nonpositive,
        max_bits).  source: DISPLAY_SOURCE_*; dn: denoise config fields for the denoised sources (none given: the default config)."""
        hist = LuminanceHistogram()
        c = denoise_config(**dn) if dn else None
        self._check(lib().mi355rt_display_histogram(self._h, int(source), C.byref(c) if c is not None else None, C.byref(hist)))
        return hist.as_dict()

    def get_display_pixels(self, denoise=None, out=None, **cfg):
        """The display read-out (include/mi355rt.h, mi355rt_get_display_pixels): exposure, tone curve and transfer on the film or on a denoised image.
        cfg: display config fields (not given: mi355rt_display_default_config's values); denoise: dict of denoise config fields for sources 1 and 2
        (None: the default config).  Returns (packed uint32[npix] 0xAARRGGBB, exposure_used as numpy float32); `out` is filled when given."""
        c = display_config(**cfg)
        d = denoise_config(**denoise) if denoise is not None else None
        if out is None:
            out = np.zeros(self.width * self.height, np.uint32)
        used = C.c_float(0.0)
        self._check(lib().mi355rt_get_display_pixels(self._h, C.byref(c), C.byref(d) if d is not None else None, _up(out), out.size, C.byref(used)))
        return out, np.float32(used.value)

    def display_image(self, rgb, **cfg):
        """mi355rt_display_image: the display mapping of an image that is no film (a baked atlas).  rgb: float32 (npix, 3), a numpy array; cfg: display config
        fields (exposure, curve, transfer, white; auto_exposure is refused); none given: the reference's tone map, as get_tonemapped_pixels.  Returns packed
        uint32[npix] 0xAARRGGBB."""
        rgb = np.ascontiguousarray(rgb, np.float32)
        if rgb.ndim != 2 or rgb.shape[1] != 3:
            raise ValueError("rgb: shape must be (npix, 3), not %s" % (rgb.shape,))
        c = display_config(**cfg) if cfg else None
        out = np.zeros(rgb.shape[0], np.uint32)
        self._check(lib().mi355rt_display_image(self._h, _fp(rgb), rgb.shape[0], C.byref(c) if c is not None else None, _up(out)))
        return out

    def get_relit_pixels(self, weights, rgb=False, **display_cfg):
        """mi355rt_get_relit_pixels (a handle created with FLAG_LIGHT_FILMS): the frame with light li's colour scaled by weights[li], mixed from the light
        films without tracing.  weights: [nlights] scalars or [nlights, 3] RGB factors.  display_cfg: display config fields (source stays the film); none
        given: the reference's tone map, as get_tonemapped_pixels.  Returns (packed uint32[npix], exposure_used as numpy float32), with rgb=True
        (rgb float32[npix, 3], packed, exposure_used)."""
        w = np.asarray(weights, np.float32)
        if w.ndim == 1:
            w = np.repeat(w[:, None], 3, axis=1)
        w = np.ascontiguousarray(w, np.float32)
        if w.ndim != 2 or w.shape[1] != 3:
            raise ValueError("weights: shape must be (nlights,) or (nlights, 3), not %s" % (w.shape,))
        c = display_config(**display_cfg) if display_cfg else None
        n = self.width * self.height
        out_rgb = np.zeros((n, 3), np.float32) if rgb else None
        packed = np.zeros(n, np.uint32)
        used = C.c_float(0.0)
        self._check(lib().mi355rt_get_relit_pixels(self._h, _fp(w) if w.size else None, w.size, C.byref(c) if c is not None else None,
                                                   _fp(out_rgb) if rgb else None, _up(packed), n, C.byref(used)))
        if rgb:
            return out_rgb, packed, np.float32(used.value)
        return packed, np.float32(used.value)

    def guides(self):
        """the denoiser's guide buffers: dict(depth float32[npix], normal float32[npix, 3], albedo float32[npix, 3], prim uint32[npix])"""
        n = self.width * self.height
        g = dict(depth=np.zeros(n, np.float32), normal=np.zeros((n, 3), np.float32), albedo=np.zeros((n, 3), np.float32), prim=np.zeros(n, np.uint32))
        self._check(lib().mi355rt_get_guides(self._h, _fp(g["depth"]), _fp(g["normal"]), _fp(g["albedo"]), _up(g["prim"]), n))
        return g

    def set_guide_source(self, source):
        """mi355rt_set_guide_source: "centre" (one centre ray per pixel, the state at creation) or "features" (the feature film's means); a GUIDES_* number is
        accepted in place of the name.  Under "features", guides() and the denoised and display read-outs take their guides from rt.features."""
        self._check(lib().mi355rt_set_guide_source(self._h, GUIDE_SOURCES[source] if isinstance(source, str) else int(source)))

    @property
    def guide_source(self):
        """mi355rt_get_guide_source by name: "centre" or "features" (the keys of GUIDE_SOURCES)"""
        s = int(lib().mi355rt_get_guide_source(self._h))
        return {v: k for k, v in GUIDE_SOURCES.items()}.get(s, s)

    def set_seed(self, seed):
        self._check(lib().mi355rt_set_seed(self._h, seed))

    def set_flags(self, flags):
        self._check(lib().mi355rt_set_flags(self._h, flags))

    def set_slices(self, slices):
        """Concurrent frame slices of render() (1..8); results do not depend on it."""
        self._check(lib().mi355rt_set_slices(self._h, slices))

    def get_slices(self):
        return int(lib().mi355rt_get_slices(self._h))

    def synchronize(self):
        self._check(lib().mi355rt_synchronize(self._h))

    @property
    def device_count(self):
        return int(lib().mi355rt_device_count(self._h))

    # --- one process per GPU: RCCL gather inside the library (include/mi355rt.h, mi355rt_comm_*)
    def comm_available(self):
        """(ok, error text): the local pre-check of comm_init; no communication"""
        rc = lib().mi355rt_comm_available(self._h)
        return rc == 0, "" if rc == 0 else (lib().mi355rt_last_error(self._h) or b"").decode()

    def comm_init(self, id128):
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(id128))
        self._check(lib().mi355rt_comm_init(self._h, buf))

    def comm_gather_frame(self, root=0, out=None):
        """collective; `out` (uint32[width*height], root only) receives the frame, None only queues the transfers"""
        if out is None:
            self._check(lib().mi355rt_comm_gather_frame(self._h, root, None, 0))
        else:
            self._check(lib().mi355rt_comm_gather_frame(self._h, root, _up(out), out.size))
        return out

    def comm_destroy(self):
        self._check(lib().mi355rt_comm_destroy(self._h))

    def comm_ranks(self):
        """ranks of the live RCCL communicator as RCCL counts them (ncclCommCount); 0 without one"""
        return int(lib().mi355rt_comm_ranks(self._h))

    def debug_gather_rate(self, table_nodes=48000, steps=2000):
        """the device's divergent-gather rate (kernels.hip, gather_rate_kernel): dict(line_accesses_per_s, ms, node_fetches_per_s)"""
        out = (C.c_double * 3)()
        self._check(lib().mi355rt_debug_gather_rate(self._h, table_nodes, steps, out))
        return {"line_accesses_per_s": out[0], "ms": out[1], "node_fetches_per_s": out[2]}

    def debug_speculation(self):
        """(50-row frames launched ahead of their call, how many the next call took over)"""
        out = (C.c_uint64 * 2)()
        self._check(lib().mi355rt_debug_speculation(self._h, out))
        return int(out[0]), int(out[1])

    def debug_check_guards(self):
        """MI355RT_DEBUG_GUARD: overwritten guard bytes behind the pass buffers (0 = clean)"""
        return int(lib().mi355rt_debug_check_guards(self._h))

    def hbm_allocated_bytes(self):
        """device memory the handle holds right now (scene, film, pass buffers, gather slots)"""
        return int(lib().mi355rt_hbm_allocated_bytes(self._h))

    def owned_rows(self):
        n = lib().mi355rt_owned_rows(self._h)
        rows = np.zeros(n, np.uint32)
        if n:
            self._check(lib().mi355rt_owned_row_list(self._h, _up(rows), n))
        return rows

    def tonemap_owned_rows_device(self, device_ptr, n, stream=None):
        """Packed owned rows into device memory.  stream (a hipStream_t as int, e.g.
        torch.cuda.current_stream().cuda_stream): asynchronous, ordered on that stream; None: synchronous."""
        if stream:
            self._check(lib().mi355rt_tonemap_owned_rows_device_on_stream(self._h, C.c_void_p(device_ptr), n, C.c_void_p(stream)))
        else:
            self._check(lib().mi355rt_tonemap_owned_rows_device(self._h, C.c_void_p(device_ptr), n))

    def intersect_rays(self, rays6):
        rays6 = np.ascontiguousarray(rays6, np.float32).reshape(-1, 6)
        n = rays6.shape[0]
        tuv = np.zeros((n, 3), np.float32); prim = np.zeros(n, np.uint32)
        self._check(lib().mi355rt_intersect_rays(self._h, _fp(rays6), n, _fp(tuv), _up(prim)))
        return tuv, prim

    def trace_rays(self, rays6, keys=None, want=("rgb",)):
        """mi355rt_trace_rays: the radiance of arbitrary rays; no film is touched.  rays6: float32 (n, 6) rows (pos3, dir3), used as given; keys: uint32
        (n, 2) rows (pixel, sampleno) for the sample's random numbers, None: (i, 0); want: any of "rgb", "direct", "tuv", "prim".  numpy arrays are host
        memory and the results come back as numpy arrays; torch tensors on the handle's GPU are read in place (MI355RT_RAYS_DEVICE) and the results are
        tensors on that device.  Returns a dict name -> array: rgb, direct, tuv (n, 3) float32; prim (n,) uint32 (as a tensor: torch.int32 holding the
        same bits, a miss is -1)."""
        want = _check_want(want, RAY_OUTPUTS)
        addr, n, dev = _ray_array(rays6, "rays6", 6, np.float32)
        kaddr = _input_beside(keys, "keys", np.uint32, n, 2, dev, "rays6 lives")
        o, device = RayOutputs(), _device_of(rays6)
        _sync(device)                                                       # what produced the rays has finished
        res = {w: _output(o, w, (n,) if w == "prim" else (n, 3), np.uint32 if w == "prim" else np.float32, device) for w in want}
        _sync(device)                                                       # ... and so has the zero fill
        self._check(lib().mi355rt_trace_rays(self._h, addr, kaddr, n, RAYS_DEVICE if dev else RAYS_HOST, C.byref(o)))
        return res

    def gather(self, points, normals=None, ids=None, spp=16, first_sample=0, weight="mean", near_distance=float("inf"), want=("n", "sum"), into=None):
        """mi355rt_gather: the light arriving at caller-given points, sampled on the device with the renderer's own hemisphere sampler (raytracer_rs_amd.gather
        is the statement).  points: float32 (n, 3); normals: float32 (n, 3) unit normals, None: the whole sphere (probes); ids: uint32 (n,) keys of the points'
        random numbers, None: i; weight "mean" (the reference's bounce estimator) or "cosine" (mean = irradiance / pi); want: any of "n", "hits", "near", "sum",
        "sumsq", "direct".  numpy arrays are host memory and the results numpy arrays; torch tensors on the handle's GPU are read in place and the results are
        tensors there (uint32 as torch.int32 holding the same bits), under trace_rays' rules.  into: the dict of an earlier call; its arrays are added to and
        returned (accumulate): gather(spp=3) then gather(spp=5, first_sample=3, into=res) is gather(spp=8) bit for bit.  `direct` is always overwritten.
        Returns a dict name -> array.  No film, camera or lens state changes."""
        want = _check_want(want, GATHER_OUTPUTS)
        if weight not in GATHER_WEIGHTS:
            raise ValueError("weight: one of %s, not %r" % (tuple(GATHER_WEIGHTS), weight))
        addr, n, dev = _ray_array(points, "points", 3, np.float32)
        naddr = _input_beside(normals, "normals", np.float32, n, 3, dev, "points live")
        iaddr = _input_beside(ids, "ids", np.uint32, n, None, dev, "points live")
        cfg = GatherConfig()
        lib().mi355rt_gather_default_config(C.byref(cfg))
        cfg.spp, cfg.first_sample, cfg.weight, cfg.accumulate, cfg.near_distance = int(spp), int(first_sample), GATHER_WEIGHTS[weight], 1 if into is not None else 0, float(near_distance)
        res, o, device = {}, GatherOutputs(), _device_of(points)
        for w in want:
            f32 = w in ("sum", "sumsq", "direct")
            res[w] = _output(o, w, (n, 3) if f32 else (n,), np.float32 if f32 else np.uint32, device, None if w == "direct" else into)
        _sync(device)                                                       # what produced the inputs (and the zero fill) has finished
        self._check(lib().mi355rt_gather(self._h, addr, naddr, iaddr, n, C.byref(cfg), RAYS_DEVICE if dev else RAYS_HOST, C.byref(o)))
        return res

    def probes_gather(self, points, ids=None, spp=64, first_sample=0, near_distance=float("inf"), want=("n", "sh"), into=None):
        """mi355rt_probes_gather: the light arriving at probes from the whole sphere, projected onto the nine real spherical harmonics up to band 2
        (raytracer_rs_amd.probes is the statement).  The samples are gather's sphere-mode samples.  points: float32 (n, 3); ids: uint32 (n,) keys of the
        points' random numbers, None: i; want: any of "n", "hits", "near", "sh" (float32 (n, 9, 3) sums).  numpy arrays or torch tensors on the handle's GPU,
        under gather's rules.  into: the dict of an earlier call; its arrays are added to and returned: probes_gather(spp=3) then probes_gather(spp=5,
        first_sample=3, into=res) is probes_gather(spp=8) bit for bit.  Returns a dict name -> array.  No film, camera or lens state changes."""
        want = _check_want(want, PROBE_OUTPUTS)
        addr, n, dev = _ray_array(points, "points", 3, np.float32)
        iaddr = _input_beside(ids, "ids", np.uint32, n, None, dev, "points live")
        cfg = ProbeConfig()
        lib().mi355rt_probes_default_config(C.byref(cfg))
        cfg.spp, cfg.first_sample, cfg.accumulate, cfg.near_distance = int(spp), int(first_sample), 1 if into is not None else 0, float(near_distance)
        o, device = ProbeOutputs(), _device_of(points)
        res = {w: _output(o, w, (n, 9, 3) if w == "sh" else (n,), np.float32 if w == "sh" else np.uint32, device, into) for w in want}
        _sync(device)                                                       # what produced the inputs (and the zero fill) has finished
        self._check(lib().mi355rt_probes_gather(self._h, addr, iaddr, n, C.byref(cfg), RAYS_DEVICE if dev else RAYS_HOST, C.byref(o)))
        return res

    def probes_lookup(self, grid, res, points, dirs, mode="irradiance", usable=None, want_ok=False):
        """mi355rt_probes_lookup: a probe grid interpolated at points and evaluated for dirs (raytracer_rs_amd.probes.lookup is the statement); traces nothing.
        grid: dict(origin, spacing, counts) (probes.grid_over makes one); res: a dict with n uint32 (nprobes,) and sh float32 (nprobes, 9, 3) as probes_gather
        returns them at probes.grid_points(grid); points, dirs: float32 (m, 3); mode "irradiance" (dirs are normals) or "radiance" (arriving from dirs);
        usable: uint8 (nprobes,) or None.  numpy arrays or torch tensors on the handle's GPU, all alike.  Returns rgb float32 (m, 3), with want_ok
        (rgb, ok uint8 (m,)): ok 0 and rgb 0 where no probe around the point could be used.  Nothing is clamped."""
        return self._lookup("probes_lookup", grid, res, points, dirs, mode, usable, want_ok)

    def _lookup(self, entry, grid, res, points, dirs, mode, usable, want_ok, normals=None, weights=None, offsets=None):
        """The one body of probes_lookup, probes_lookup_vis and probes_lookup_placed; entry names which, and the call ends in the library entry of that name.
        weights: (chebyshev, facing, normal_bias) for the two that read depth films, which res then holds; offsets: probes_lookup_placed's."""
        weighted, placed = weights is not None, entry == "probes_lookup_placed"
        if mode not in SH_MODES:
            raise ValueError("mode: one of %s, not %r" % (tuple(SH_MODES), mode))
        for k in ("n", "sh", "count", "moments", "depth_res", "max_distance") if weighted else ():
            if k not in res:
                raise ValueError("res: holds no %r (probes_gather_depth returns it)" % k)
        g = grid if isinstance(grid, ProbeGrid) else ProbeGrid.from_dict(grid)
        nprobes = int(g.counts[0]) * int(g.counts[1]) * int(g.counts[2])
        R = int(res["depth_res"]) if weighted else 0
        if weighted and not 2 <= R <= 16:
            raise ValueError('res["depth_res"]: 2 .. 16, not %r' % R)
        addr, m, dev = _ray_array(points, "points", 3, np.float32)
        daddr, _, ddev = _ray_array(dirs, "dirs", 3, np.float32, rows=m)
        naddr, _, ndev = _ray_vector(res["n"], 'res["n"]', np.uint32, nprobes)
        saddr, _, sdev = _film_array(res["sh"], 'res["sh"]', (nprobes, 9, 3), np.float32)
        uaddr = nraddr = oaddr = None
        devs, films = {dev, ddev, ndev, sdev}, []
        if weighted:
            caddr, _, cdev = _film_array(res["count"], 'res["count"]', (nprobes, R * R), np.uint32)
            maddr, _, mdev = _film_array(res["moments"], 'res["moments"]', (nprobes, R * R, 2), np.float32)
            devs |= {cdev, mdev}
        if usable is not None:
            uaddr, _, udev = _ray_vector(usable, "usable", np.uint8, nprobes)
            devs.add(udev)
        if normals is not None:
            nraddr, _, nrdev = _ray_array(normals, "normals", 3, np.float32, rows=m)
            devs.add(nrdev)
        if offsets is not None:
            oaddr, _, odev = _ray_array(offsets, "offsets", 3, np.float32, rows=nprobes)
            devs.add(odev)
        if len(devs) != 1:
            names = ["dirs"] + ["normals"] * weighted + ["res", "usable"] + ["offsets"] * placed
            raise ValueError("%s and %s must live where points live (all numpy arrays, or all tensors on the GPU)" % (", ".join(names[:-1]), names[-1]))
        if weighted:
            d = ProbeDepth(R, float(np.float32(res["max_distance"])), caddr, maddr)
            vc = ProbeVisConfig((VIS_CHEBYSHEV if weights[0] else 0) | (VIS_FACING if weights[1] and normals is not None else 0), float(weights[2]))
            films = [C.byref(d), C.byref(vc)]
        rgb, ok, raddr, okaddr = _rgb_ok(m, want_ok, _device_of(points))
        args = [self._h, C.byref(g), naddr, saddr, uaddr] + films + [oaddr] * placed + [addr, daddr] + [nraddr] * weighted
        self._check(getattr(lib(), "mi355rt_" + entry)(*args, m, SH_MODES[mode], RAYS_DEVICE if dev else RAYS_HOST, raddr, okaddr))
        return (rgb, ok) if want_ok else rgb

    def probes_gather_depth(self, points, ids=None, spp=64, first_sample=0, near_distance=float("inf"), res=8, max_distance=None,
                            want=("n", "sh", "count", "moments"), into=None):
        """mi355rt_probes_gather_depth: probes_gather, and from the same traced samples each probe's depth film over an octahedral map of res x res texels
        (raytracer_rs_amd.probes.project_depth is the statement): count uint32 (n, res * res) and moments float32 (n, res * res, 2), the sums of dist and
        dist^2 with dist = min(t, max_distance) and max_distance for a miss.  res: 2 .. 16; max_distance: finite, > 0, <= 1e12 (probes.grid_max_distance(grid)
        is the usual choice; None: that of `into`).  want: any of "n", "hits", "near", "sh", "count", "moments"; count and moments come together.  numpy
        arrays or torch tensors on the handle's GPU, under probes_gather's rules.  into: the dict of an earlier call with the same res and max_distance; its
        arrays are added to and returned.  Returns a dict name -> array, with "depth_res" and "max_distance" when it holds a depth film.  No film, camera or
        lens state changes."""
        want = _check_want(want, PROBE_DEPTH_OUTPUTS)
        if ("count" in want) != ("moments" in want):
            raise ValueError('want: "count" and "moments" come together')
        if "count" not in want:
            return self.probes_gather(points, ids, spp, first_sample, near_distance, want, into)
        res = int(res)
        max_distance = _reconcile_max_distance(max_distance, into, res)
        addr, n, dev = _ray_array(points, "points", 3, np.float32)
        iaddr = _input_beside(ids, "ids", np.uint32, n, None, dev, "points live")
        cfg = ProbeConfig()
        lib().mi355rt_probes_default_config(C.byref(cfg))
        cfg.spp, cfg.first_sample, cfg.accumulate, cfg.near_distance = int(spp), int(first_sample), 1 if into is not None else 0, float(near_distance)
        shapes = {"sh": (n, 9, 3), "count": (n, res * res), "moments": (n, res * res, 2)}
        o, d, device = ProbeOutputs(), ProbeDepth(res, max_distance, None, None), _device_of(points)
        out = {w: _output(d if w in ("count", "moments") else o, w, shapes.get(w, (n,)), np.float32 if w in ("sh", "moments") else np.uint32, device, into) for w in want}
        out["depth_res"], out["max_distance"] = res, max_distance
        _sync(device)                                                       # what produced the inputs (and the zero fill) has finished
        only_depth = all(w in ("count", "moments") for w in want)
        self._check(lib().mi355rt_probes_gather_depth(self._h, addr, iaddr, n, C.byref(cfg), RAYS_DEVICE if dev else RAYS_HOST, None if only_depth else C.byref(o), C.byref(d)))
        return out

    def probes_lookup_vis(self, grid, res, points, dirs, normals=None, mode="irradiance", usable=None, chebyshev=True, facing=True, normal_bias=0.0, want_ok=False):
        """mi355rt_probes_lookup_vis: probes_lookup with each corner's trilinear weight multiplied by the probe's visibility of the query (Chebyshev's bound on
        its depth film) and by how much the surface faces the probe (raytracer_rs_amd.probes.lookup_vis is the statement); traces nothing.  res: the dict
        probes_gather_depth returned at probes.grid_points(grid), with n, sh, count, moments, depth_res and max_distance.  normals: float32 (m, 3) unit normals
        of the surface at the points, or None: then facing has no effect and normal_bias must be 0.  With chebyshev=False, facing=False and normal_bias=0 the
        result is probes_lookup's on every bit.  numpy arrays or torch tensors on the handle's GPU, all alike.  Returns rgb float32 (m, 3), with want_ok
        (rgb, ok uint8 (m,))."""
        return self._lookup("probes_lookup_vis", grid, res, points, dirs, mode, usable, want_ok, normals=normals, weights=(chebyshev, facing, normal_bias))

    def bake_texels(self, uv, width, height, flip=False, want=BAKE_TEXEL_OUTPUTS):
        """mi355rt_bake_texels: the UV charts of the scene's triangles rasterised into an atlas of width x height texels (raytracer_rs_amd.bake.texels is the
        statement).  uv: float32 (ntri, 3, 2), one UV triangle per scene triangle, u to the right and v downwards; a numpy array (host, results numpy arrays)
        or a torch tensor on the handle's GPU (read in place, results tensors there, uint32 as torch.int32 holding the same bits).  flip: the lists' normals
        negated.  want: any of "owner", "bary", "ids", "points", "normals", "albedo".  Returns a dict: owner uint32 (width * height,), the lowest triangle
        index covering the texel's centre or 0xFFFFFFFF; bary float32 (width * height, 2), 0 where uncovered; the compact lists of the covered texels in
        ascending texel index, ids uint32 (n,) (the texel index: the key gather should sample under), points / normals / albedo float32 (n, 3); "ncovered".
        No film, camera or lens state changes."""
        want = _check_want(want, BAKE_TEXEL_OUTPUTS, empty_ok=True)
        width, height = int(width), int(height)
        if not (1 <= width <= 16384 and 1 <= height <= 16384):
            raise ValueError("width and height must be 1 .. 16384")
        if (_is_tensor(uv) or isinstance(uv, np.ndarray)) and len(uv.shape) == 3 and tuple(uv.shape[1:]) == (3, 2):
            if not (uv.is_contiguous() if _is_tensor(uv) else uv.flags["C_CONTIGUOUS"]):
                raise ValueError("uv: must be C-contiguous")             # before the reshape, which would copy
            addr, _, dev = _ray_array(uv.reshape(-1, 6), "uv", 6, np.float32, rows=int(self.triangle_count))
        elif _is_tensor(uv) or isinstance(uv, np.ndarray):
            raise ValueError("uv: shape must be (%d, 3, 2), not %s" % (int(self.triangle_count), tuple(uv.shape)))
        else:
            raise TypeError("uv: a numpy array or a torch tensor, not %s" % type(uv).__name__)
        nt = width * height
        shapes = {"owner": ((nt,), np.uint32), "bary": ((nt, 2), np.float32), "ids": ((nt,), np.uint32), "points": ((nt, 3), np.float32),
                  "normals": ((nt, 3), np.float32), "albedo": ((nt, 3), np.float32)}
        o, device = BakeTexelOutputs(), _device_of(uv)
        res = {w: _output(o, w, shapes[w][0], shapes[w][1], device) for w in want}
        _sync(device)                                                       # what produced uv (and the zero fill) has finished
        n = C.c_uint32(0)
        self._check(lib().mi355rt_bake_texels(self._h, addr, width, height, 1 if flip else 0, RAYS_DEVICE if dev else RAYS_HOST, C.byref(o), C.byref(n)))
        for w in ("ids", "points", "normals", "albedo"):
            if w in res:
                res[w] = res[w][:n.value]
        res["ncovered"] = int(n.value)
        return res

    def bake_atlas(self, ids, values, width, height, dilate=2):
        """mi355rt_bake_atlas: per-texel values back into an image, chart borders filled (raytracer_rs_amd.bake.atlas is the statement).  ids: uint32 (n,) texel
        indices; values: float32 (n, 3); numpy arrays or torch tensors on the handle's GPU, both alike.  dilate: iterations in which an empty texel takes the
        mean of its non-empty 8-neighbours.  Returns (atlas float32 (width * height, 3), valid uint8 (width * height,)): valid 0 empty, 1 given, 1 + k filled
        in iteration k.  Ids outside the atlas and repeated ids are refused with nothing written."""
        width, height, dilate = int(width), int(height), int(dilate)
        if not (1 <= width <= 16384 and 1 <= height <= 16384):
            raise ValueError("width and height must be 1 .. 16384")
        if not 0 <= dilate <= 0xFFFFFFFF:
            raise ValueError("dilate must be 0 .. 2^32 - 1")
        vaddr, n, dev = _ray_array(values, "values", 3, np.float32)
        iaddr = _input_beside(ids, "ids", np.uint32, n, None, dev, "values live", optional=False)
        atlas, valid, aaddr, daddr = _rgb_ok(width * height, True, _device_of(values))
        self._check(lib().mi355rt_bake_atlas(self._h, iaddr, vaddr, n, width, height, dilate, RAYS_DEVICE if dev else RAYS_HOST, aaddr, daddr))
        return atlas, valid

    def bake(self, uv, width, height, spp=16, weight="mean", dilate=2, first_sample=0, into=None, flip=False):
        """A lightmap bake: bake_texels, then gather(points, normals, ids, spp, first_sample, weight, want=("n", "sum", "sumsq", "direct")) at the covered
        texels' points under the texel index as the key, then bake_atlas of three per-texel values (raytracer_rs_amd.bake states each):
            direct     the unshadowed point-light term
            indirect   sum / n
            radiance   albedo * direct + indirect (f32, elementwise): under weight "mean" what the reference's compute_radiance shows at the point without
                       the view-dependent highlight
        into: the dict an earlier bake of the same charts returned; its gather sums are added to, so bake(spp=3) then bake(spp=5, first_sample=3, into=...)
        is bake(spp=8) bit for bit.  Returns dict(texels=..., gather=..., direct=, indirect=, radiance= (atlas, valid) pairs)."""
        tex = self.bake_texels(uv, width, height, flip=flip)
        prev = None if into is None else into["gather"]
        g = self.gather(tex["points"], tex["normals"], tex["ids"], spp=spp, first_sample=first_sample, weight=weight, want=("n", "sum", "sumsq", "direct"), into=prev)
        if _is_tensor(uv):
            import torch
            ind = g["sum"] / g["n"].to(torch.float32)[:, None]             # n as int32 bits: counts stay far below 2^31
            rad = tex["albedo"] * g["direct"] + ind
        else:
            with np.errstate(all="ignore"):
                ind = (g["sum"] / g["n"].astype(np.float32)[:, None]).astype(np.float32)
                rad = (tex["albedo"] * g["direct"] + ind).astype(np.float32)
        out = dict(texels=tex, gather=g)
        for name, val in (("direct", g["direct"]), ("indirect", ind), ("radiance", rad)):
            out[name] = self.bake_atlas(tex["ids"], val.contiguous() if _is_tensor(val) else np.ascontiguousarray(val), width, height, dilate=dilate)
        return out

    def render_rays(self, rays6, spp):
        """mi355rt_render_rays: mi355rt_render with the caller's rays.  rays6: float32 (width * height * spp, 6), row s * npix + p = the ray of the call's
        sample s of film pixel p (raytracer_rs_amd.cameras builds such arrays); a numpy array (host) or a torch tensor on the handle's GPU.  Returns
        the call's counters.  Afterwards the film holds caller-ray samples: the denoised read-outs and render_adaptive refuse it until film.clear() /
        film.set()."""
        spp = int(spp)
        if spp < 1:
            raise ValueError("spp must be >= 1")
        addr, n, dev = _ray_array(rays6, "rays6", 6, np.float32, rows=self.width * self.height * spp)
        if dev:
            import torch
            torch.cuda.current_stream(rays6.device).synchronize()
        rc = RayCounts()
        self._check(lib().mi355rt_render_rays(self._h, addr, n, spp, RAYS_DEVICE if dev else RAYS_HOST, C.byref(rc)))
        return rc

    # --- lens models (include/mi355rt.h, "lens models")
    def set_lens(self, model="pinhole", radius=None, focus=None, width_world=None):
        """mi355rt_set_lens: the ray generator of render().  "thin" (radius, focus): depth of field, cameras.thin_lens made on the device; "ortho"
        (width_world): cameras.orthographic; "pinhole": the reference's camera, the state at creation.  A Lens is accepted in place of the model name.
        Keeps the film.  Under a lens the guides, and so the denoised and display read-outs, describe the lens's view; render_adaptive and
        trace_frame_additive refuse.  Raises RuntimeError naming the field for an invalid lens (nothing changes then)."""
        l = model if isinstance(model, Lens) else make_lens(model, radius, focus, width_world)
        self._check(lib().mi355rt_set_lens(self._h, C.byref(l)))

    @property
    def lens(self):
        """mi355rt_get_lens: the handle's Lens"""
        l = Lens()
        self._check(lib().mi355rt_get_lens(self._h, C.byref(l)))
        return l

    def lens_rays(self, spp, device=False):
        """mi355rt_lens_rays: float32 (width * height * spp, 6), the rays the next render(spp) would take under the handle's lens, in render_rays layout
        (row s * npix + p: key (p, film_n[p] + s)).  device=False: a numpy array; device=True (or a torch device): a torch tensor on the handle's GPU,
        as render_rays accepts one — the start of a caller's own ray generator (distortion, stereo offsets) without a host array."""
        spp = int(spp)
        if spp < 1:
            raise ValueError("spp must be >= 1")
        n = self.width * self.height * spp
        dev = None
        if not (device is False or device is None):
            import torch
            dev = torch.device("cuda", self.device_index) if device is True else torch.device(device)
        out = _new_output((n, 6), np.float32, dev)
        _sync(dev)                                                          # the zero fill has finished
        self._check(lib().mi355rt_lens_rays(self._h, spp, RAYS_HOST if dev is None else RAYS_DEVICE, _address(out), n))
        return out

    def occluded_rays(self, rays6):
        rays6 = np.ascontiguousarray(rays6, np.float32).reshape(-1, 6)
        n = rays6.shape[0]
        out = np.zeros(n, np.uint8)
        self._check(lib().mi355rt_occluded_rays(self._h, _fp(rays6), n, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def sample_table(self):
        out = np.zeros((65536, 3), np.float32)
        self._check(lib().mi355rt_get_sample_table(self._h, _fp(out)))
        return out

    def debug_sample(self, pixel, sampleno):
        nodes = lib().mi355rt_tree_nodes(self._h)
        color = np.zeros(3, np.float32); node_l = np.zeros((nodes, 3), np.float32)
        self._check(lib().mi355rt_debug_sample(self._h, pixel, sampleno, _fp(color), _fp(node_l), nodes))
        return color, node_l

    def debug_numerics(self, a, b):
        a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
        q = np.zeros_like(a); r = np.zeros_like(a); p = np.zeros_like(a)
        self._check(lib().mi355rt_debug_numerics(self._h, _fp(a), _fp(b), a.size, _fp(q), _fp(r), _fp(p)))
        return q, r, p

    def debug_slab(self, inv_rays6, cubes6):
        """intersect_cube_inverse_ray on the device: (hit[n] bool, tmin[n])"""
        r = np.ascontiguousarray(inv_rays6, np.float32).reshape(-1, 6); c = np.ascontiguousarray(cubes6, np.float32).reshape(-1, 6)
        assert r.shape == c.shape
        hit = np.zeros(r.shape[0], np.uint8); tmin = np.zeros(r.shape[0], np.float32)
        self._check(lib().mi355rt_debug_slab(self._h, _fp(r), _fp(c), r.shape[0], hit.ctypes.data_as(C.POINTER(C.c_uint8)), _fp(tmin)))
        return hit.astype(bool), tmin

    def accel_stats(self):
        out = np.zeros(8, np.uint32)
        self._check(lib().mi355rt_accel_stats(self._h, _up(out)))
        return dict(nodes=int(out[0]), leaves=int(out[1]), max_depth=int(out[2]), max_leaf=int(out[3]),
                    node_bytes=int(out[4]), tri_bytes=int(out[5]), bvh_build_ms=int(out[6]) / 1000.0, octree_build_ms=int(out[7]) / 1000.0)

    def reflect_mask_info(self):
        """the direction masks that prove reflection rays free: bins per cube-face edge (0: none), build time, share of clear bits, device bytes"""
        out = (C.c_double * 4)()
        self._check(lib().mi355rt_reflect_mask_info(self._h, out))
        return dict(bins=int(out[0]), build_ms=float(out[1]), clear_share=float(out[2]), bytes=int(out[3]))

    def debug_rays_read(self):
        """FLAG_COUNT_STEPS: rays the trace launches of the last call took from their queues, counted by the trace kernels"""
        out = C.c_uint64(0)
        self._check(lib().mi355rt_debug_rays_read(self._h, C.byref(out)))
        return int(out.value)

    def bvh_build_info(self):
        out = np.zeros(2, np.uint32)
        self._check(lib().mi355rt_bvh_build_info(self._h, _up(out)))
        return dict(on_device=bool(out[0]), device_ms=int(out[1]) / 1000.0)

    def bvh_read(self):
        """the binary BVH the handle's kernels were given, word for word, whichever builder made it (include/mi355rt.h, mi355rt_debug_bvh_read)"""
        return _bvh_read(self._h, None, None, 0)

    def octree_stats(self):
        out = np.zeros(8, np.uint32)
        self._check(lib().mi355rt_octree_stats(self._h, _up(out)))
        return dict(nodes=int(out[0]), inner=int(out[1]), leaves=int(out[2]), empty=int(out[3]), depth=int(out[4]), tri_refs=int(out[5]))

    @property
    def triangle_count(self):
        return lib().mi355rt_triangle_count(self._h)

    @property
    def current_row(self):
        return lib().mi355rt_current_row(self._h)


def _finish(code, handle, keep=None, cfg=None):
    if code != 0:
        raise RuntimeError((lib().mi355rt_last_error(None) or b"").decode() or "mi355rt error %d" % code)
    return RayTracer(handle.value, keep, cfg.device if cfg is not None else 0)


def create_raytracer(collada_doc, triangles_per_leaf, width, height, data_dir=None, **cfg_kw):
    """lib.rs:15-20.  Raises RuntimeError(message) where the reference returns Err(String)."""
    cfg = default_config(width, height, triangles_per_leaf=triangles_per_leaf, **cfg_kw)
    doc = collada_doc.encode() if isinstance(collada_doc, str) else bytes(collada_doc)
    h = C.c_void_p()
    code = lib().mi355rt_create_from_collada_str(doc, len(doc), data_dir.encode() if data_dir else None, C.byref(cfg), C.byref(h))
    return _finish(code, h, None, cfg)


def create_raytracer_from_file(collada_filename, triangles_per_leaf, width, height, **cfg_kw):
    """lib.rs:22-27"""
    cfg = default_config(width, height, triangles_per_leaf=triangles_per_leaf, **cfg_kw)
    h = C.c_void_p()
    code = lib().mi355rt_create_from_collada_file(str(collada_filename).encode(), C.byref(cfg), C.byref(h))
    return _finish(code, h, None, cfg)


def create_raytracer_from_scene_file(scene_filename, triangles_per_leaf, width, height, **cfg_kw):
    cfg = default_config(width, height, triangles_per_leaf=triangles_per_leaf, **cfg_kw)
    h = C.c_void_p()
    code = lib().mi355rt_create_from_scene_file(str(scene_filename).encode(), C.byref(cfg), C.byref(h))
    return _finish(code, h, None, cfg)


def scene_desc(scene):
    """(SceneDesc, keepalive): the parsed arrays of scene_io.load_scene_file() as mi355rt_create takes them.  A texture is a float array of shape
    (height, width, 3); any other shape is refused here (RuntimeError), because the C struct carries no length the library could check."""
    verts = np.ascontiguousarray(scene["tri_verts"], np.float32).reshape(-1)
    geom = np.ascontiguousarray(scene["tri_geom"], np.uint32)
    nm = len(scene["mat_kind"])
    mats = (Material * max(nm, 1))()
    for i in range(nm):
        mats[i].kind = int(scene["mat_kind"][i]); mats[i].tex_id = int(scene["mat_tex"][i])
        for c in range(3):
            mats[i].rgb[c] = float(scene["mat_rgb"][i][c])
    nl = len(scene["lights"])
    lights = (Light * max(nl, 1))()
    for i in range(nl):
        for c in range(3):
            lights[i].pos[c] = float(scene["lights"][i][c]); lights[i].color[c] = float(scene["lights"][i][3 + c])
    nt = len(scene["textures"])
    texs = (Texture * max(nt, 1))()
    keep = [verts, geom, mats, lights, texs]
    for i, t in enumerate(scene["textures"]):
        arr = np.ascontiguousarray(t, np.float32)
        if arr.ndim != 3 or arr.shape[2] != 3:
            raise RuntimeError("texture size mismatch: texture %d has shape %r, not (height, width, 3)" % (i, arr.shape))
        keep.append(arr)
        texs[i].height, texs[i].width = arr.shape[0], arr.shape[1]
        texs[i].rgb = _fp(arr)
    sd = SceneDesc()
    sd.tri_verts = _fp(verts); sd.tri_geom = _up(geom); sd.ntri = geom.size
    sd.materials = mats; sd.nmaterials = nm; sd.lights = lights; sd.nlights = nl
    sd.textures = texs; sd.ntextures = nt
    for i in range(16):
        sd.camera_orientation[i] = float(scene["camera_matrix"][i])
    sd.camera_fov_deg = float(scene["camera_fov"])
    return sd, keep


def create_raytracer_from_arrays(scene, triangles_per_leaf, width, height, **cfg_kw):
    """build_raytracer (lib.rs:29-44) from parsed arrays — what a Rust shim would marshal.
    `scene` is the dict produced by scene_io.load_scene_file()."""
    cfg = default_config(width, height, triangles_per_leaf=triangles_per_leaf, **cfg_kw)
    sd, keep = scene_desc(scene)
    h = C.c_void_p()
    code = lib().mi355rt_create(C.byref(sd), C.byref(cfg), C.byref(h))
    return _finish(code, h, keep, cfg)


def film_file_info(path):
    """mi355rt_film_file_info (host code, no device): dict(version, width, height, planes, seed, flags) of a film file; raises RuntimeError
    with the library's reason for a malformed file"""
    out = (C.c_uint32 * 8)()
    if lib().mi355rt_film_file_info(os.fsencode(path), out) != 0:
        raise RuntimeError((lib().mi355rt_last_error(None) or b"").decode() or "mi355rt_film_file_info failed")
    return dict(version=int(out[0]), width=int(out[1]), height=int(out[2]), planes=int(out[3]), seed=int(out[4]) | int(out[5]) << 32, flags=int(out[6]))


def debug_light_map(tri_verts, light, pad, res):
    """(dist2[6, res, res], nearest): the depth cube map the library builds around a point light (host code; include/mi355rt.h)"""
    v = np.ascontiguousarray(tri_verts, np.float32).reshape(-1, 9)
    l = np.ascontiguousarray(light, np.float32).reshape(3)
    out = np.zeros((6, res, res), np.float32); nearest = C.c_double(0.0)
    code = lib().mi355rt_debug_light_map(_fp(v), v.shape[0], _fp(l), float(pad), int(res), _fp(out), C.byref(nearest))
    if code != 0:
        raise RuntimeError("mi355rt_debug_light_map failed: %d" % code)
    return out, nearest.value


def debug_reflect_mask(tri_verts, pad, bins=8, work_budget=0, min_cos=0.0, pad_angle=0.0):
    """(words[ntri, stride] or None, info): the per-triangle direction masks the library builds for the reflection rays (host code; include/mi355rt.h).
    info: stride, build_ms, work, clear_bits, min_cos, pad_angle, bary_margin, built"""
    v = np.ascontiguousarray(tri_verts, np.float32).reshape(-1, 9)
    info = (C.c_double * 8)()
    info[4], info[5] = float(min_cos), float(pad_angle)          # 0: the library's own margins
    stride = 6 * bins * bins // 32 + 4
    out = np.zeros((v.shape[0], stride), np.uint32)
    code = lib().mi355rt_debug_reflect_mask(_fp(v), v.shape[0], float(pad), int(bins), int(work_budget), _up(out), info)
    if code != 0:
        raise RuntimeError("mi355rt_debug_reflect_mask failed: %d" % code)
    d = dict(stride=int(info[0]), build_ms=float(info[1]), work=int(info[2]), clear_bits=int(info[3]), min_cos=float(info[4]), pad_angle=float(info[5]),
             bary_margin=float(info[6]), built=bool(info[7]))
    return (out if d["built"] else None), d


def debug_wide_bvh(tri_verts):
    """facts about the 4-wide tree of 48-byte nodes the MI355RT_WIDE experiment builds walk, checked by a host walk (include/mi355rt.h)"""
    v = np.ascontiguousarray(tri_verts, np.float32).reshape(-1, 9)
    out = (C.c_uint32 * 8)()
    code = lib().mi355rt_debug_wide_bvh(_fp(v), v.shape[0], out)
    if code != 0:
        raise RuntimeError("mi355rt_debug_wide_bvh failed: %d" % code)
    keys = ("wide_nodes", "binary_nodes", "stack_need", "binary_depth", "children", "tris_once_wide", "bad_boxes", "tris_once_binary")
    return dict(zip(keys, (int(x) for x in out)))


def debug_octree(tri_verts, tris_per_leaf):
    """the reference's octree as mi355rt_create builds it, by node index (host code; include/mi355rt.h): dict(cubes (n, 6), first_child (n,) int32,
    tri_first, tri_count, parent (n,), leaf_tris, stats: the dict of RayTracer.octree_stats)"""
    v = np.ascontiguousarray(tri_verts, np.float32).reshape(-1, 9)
    counts = np.zeros(8, np.uint32)
    code = lib().mi355rt_debug_octree(_fp(v), v.shape[0], int(tris_per_leaf), _up(counts), None, None, None, None, None, 0, None, 0)
    if code != 0:
        raise RuntimeError("mi355rt_debug_octree failed: %d" % code)
    n, refs = int(counts[0]), int(counts[5])
    cubes = np.zeros((n, 6), np.float32); first_child = np.zeros(n, np.int32)
    tri_first = np.zeros(n, np.uint32); tri_count = np.zeros(n, np.uint32); parent = np.zeros(n, np.uint32); leaf_tris = np.zeros(max(refs, 1), np.uint32)
    code = lib().mi355rt_debug_octree(_fp(v), v.shape[0], int(tris_per_leaf), _up(counts), _fp(cubes), first_child.ctypes.data_as(C.POINTER(C.c_int32)),
                                      _up(tri_first), _up(tri_count), _up(parent), n, _up(leaf_tris), refs)
    if code != 0:
        raise RuntimeError("mi355rt_debug_octree failed: %d" % code)
    stats = dict(nodes=int(counts[0]), inner=int(counts[1]), leaves=int(counts[2]), empty=int(counts[3]), depth=int(counts[4]), tri_refs=int(counts[5]))
    return dict(cubes=cubes, first_child=first_child, tri_first=tri_first, tri_count=tri_count, parent=parent, leaf_tris=leaf_tris[:refs], stats=stats)


def _bvh_read(handle, verts, geom, ntri):
    info = np.zeros(8, np.uint32); bounds = np.zeros(6, np.float32)
    vp = _fp(verts) if verts is not None else None; gp = _up(geom) if geom is not None else None
    code = lib().mi355rt_debug_bvh_read(handle, vp, gp, ntri, _up(info), _fp(bounds), None, 0, None, 0)
    if code != 0:
        raise RuntimeError("mi355rt_debug_bvh_read failed: %d" % code)
    nn, nt = int(info[0]), int(info[1])
    nodes = np.zeros((max(nn, 1), 8), np.uint32); tris = np.zeros((max(nt, 1), 12), np.uint32)
    code = lib().mi355rt_debug_bvh_read(handle, vp, gp, ntri, _up(info), _fp(bounds), _up(nodes), nn, _up(tris), nt)
    if code != 0:
        raise RuntimeError("mi355rt_debug_bvh_read failed: %d" % code)
    return dict(nodes=nodes[:nn], tris=tris[:nt], root=int(info[2:3].view(np.int32)[0]), leaves=int(info[3]), max_depth=int(info[4]), max_leaf=int(info[5]),
                scene_min=bounds[:3].copy(), scene_max=bounds[3:].copy())


def debug_bvh(tri_verts, tri_geom=None):
    """the binary BVH the host builder makes of these triangles, as mi355rt_create would (host code, no device; include/mi355rt.h,
    mi355rt_debug_bvh_read): dict(nodes (k, 8) uint32, tris (n, 12) uint32, root, leaves, max_depth, max_leaf, scene_min, scene_max)"""
    v = np.ascontiguousarray(tri_verts, np.float32).reshape(-1, 9)
    g = None if tri_geom is None else np.ascontiguousarray(tri_geom, np.uint32).reshape(-1)
    if g is not None and g.shape[0] != v.shape[0]:
        raise ValueError("tri_geom has %d entries for %d triangles" % (g.shape[0], v.shape[0]))
    return _bvh_read(None, v, g, v.shape[0])


def comm_unique_id():
    """128-byte RCCL id (rank 0 creates it, the host application hands it to the other ranks)"""
    buf = (C.c_uint8 * 128)()
    if lib().mi355rt_comm_unique_id(buf) != 0:
        raise RuntimeError((lib().mi355rt_last_error(None) or b"").decode() or "mi355rt_comm_unique_id failed")
    return bytes(buf)


class Stats:
    """stats.rs:3-40 — fps and primary rays/s per call and running mean."""

    def __init__(self):
        self.last_iteration = time.perf_counter()
        self.fps_sum = 0.0
        self.primrays_per_sec_sum = 0.0
        self.num_measurements = 0

    def stats(self, num_primary_rays):
        now = time.perf_counter()
        dt = now - self.last_iteration
        self.last_iteration = now
        fps = 1.0 / dt
        self.fps_sum += fps
        prs = num_primary_rays / dt
        self.primrays_per_sec_sum += prs
        self.num_measurements += 1
        return "fps: %s  primary rays/s: %d" % (fps, int(prs))

    def mean_stats(self):
        return "mean fps: %s  mean primary rays/s: %s" % (
            self.fps_sum / self.num_measurements, self.primrays_per_sec_sum / self.num_measurements)


class stats:  # namespace alias: raytracer_lib::stats::Stats
    Stats = Stats


# ---- probe placement (include/mi355rt.h, "PROBE PLACEMENT"): the structs, the symbols and the RayTracer methods --------------------------------
SURVEY_FLIP = 1                                                 # MI355RT_SURVEY_FLIP
PROBE_UNKNOWN, PROBE_BURIED, PROBE_IDLE, PROBE_ACTIVE = 0, 1, 2, 3      # MI355RT_PROBE_*
PLACE_UNSAMPLED, PLACE_THROUGH, PLACE_AWAY, PLACE_STAY, PLACE_BACK, PLACE_REST, PLACE_REFUSED = 0, 1, 2, 3, 4, 5, 8      # MI355RT_PLACE_*
PROBE_SURVEY_OUTPUTS = ("n", "back", "front", "near_back", "near_front", "far")
PROBE_PLACE_OUTPUTS = ("offsets", "verdict", "state")


class ProbeSurveyConfig(C.Structure):
    """mi355rt_probe_survey_config: flags SURVEY_FLIP; max_distance finite, > 0, <= 1e12"""
    _fields_ = [("spp", C.c_uint32), ("first_sample", C.c_uint32), ("accumulate", C.c_uint32), ("flags", C.c_uint32), ("max_distance", C.c_float)]


class ProbeSurvey(C.Structure):
    """mi355rt_probe_survey: n, back, front uint32 (npoints,); near_back, near_front, far float32 (npoints, 4) rows (dist, dx, dy, dz) (void pointers here:
    host arrays or device addresses)"""
    _fields_ = [("n", C.c_void_p), ("back", C.c_void_p), ("front", C.c_void_p), ("near_back", C.c_void_p), ("near_front", C.c_void_p), ("far", C.c_void_p)]


class ProbePlaceConfig(C.Structure):
    """mi355rt_probe_place_config: back_share 0.25 and max_offset 0.45 by default; min_front and max_distance are the caller's to set"""
    _fields_ = [("back_share", C.c_float), ("max_offset", C.c_float), ("min_front", C.c_float), ("max_distance", C.c_float)]


ABI += [
    ("mi355rt_probes_survey_default_config", None, [C.POINTER(ProbeSurveyConfig)]),
    ("mi355rt_probes_place_default_config", None, [C.POINTER(ProbePlaceConfig)]),
    ("mi355rt_probes_survey", C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(ProbeSurveyConfig), C.c_uint32, C.POINTER(ProbeSurvey)]),
    ("mi355rt_probes_place", C.c_int, [_H, C.POINTER(ProbeGrid), C.POINTER(ProbeSurvey), C.POINTER(ProbePlaceConfig), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("mi355rt_probe_place_one", C.c_int, [C.POINTER(ProbeGrid), C.POINTER(ProbePlaceConfig), _U, _F, _F, _F, _U, _U]),
    ("mi355rt_probes_lookup_placed", C.c_int, [_H, C.POINTER(ProbeGrid), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ProbeDepth), C.POINTER(ProbeVisConfig), C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("mi355rt_probes_lookup_placed_one", C.c_int, [C.POINTER(ProbeGrid), _U, _F, C.POINTER(C.c_uint8), C.POINTER(ProbeDepth), C.POINTER(ProbeVisConfig), _F, _F, _F, _F,
                                                   C.c_uint32, _F, _U]),
]


def _survey_pointers(sv, nprobes, name):
    """(ProbeSurvey, is_device) over the six arrays of a survey dict, each checked"""
    s, devs = ProbeSurvey(), []
    for k in PROBE_SURVEY_OUTPUTS:
        if k not in sv:
            raise ValueError("%s: holds no %r (probes_survey returns it)" % (name, k))
        label = "%s[%r]" % (name, k)
        addr, _, dev = _ray_vector(sv[k], label, np.uint32, nprobes) if k in ("n", "back", "front") else _ray_array(sv[k], label, 4, np.float32, rows=nprobes)
        setattr(s, k, addr)
        devs.append(dev)
    if len(set(devs)) != 1:
        raise ValueError("%s: its arrays must all live in one place (all numpy arrays, or all tensors on the GPU)" % name)
    return s, devs[0]


def _probes_survey(self, points, ids=None, spp=64, first_sample=0, max_distance=None, flip=False, into=None):
    """mi355rt_probes_survey: what each point sees around itself, from the closest hits of probes_gather's samples (raytracer_rs_amd.probes.survey is the
    statement): n, back, front uint32 (n,) and the records near_back, near_front, far float32 (n, 4) rows (dist, dx, dy, dz).  A back hit is one whose ray runs
    along the hit triangle's normal (flip: against it).  max_distance: finite, > 0, <= 1e12 (None: that of `into`).  numpy arrays or torch tensors on the
    handle's GPU, under probes_gather's rules.  into: the dict of an earlier call with the same max_distance; its arrays are continued and returned:
    probes_survey(spp=3) then probes_survey(spp=5, first_sample=3, into=res) is probes_survey(spp=8) bit for bit.  Returns a dict name -> array, with
    "max_distance".  Only closest hits are traced: last_counts() reports n * spp primary rays, no bounce and no shadow ray."""
    max_distance = _reconcile_max_distance(max_distance, into)
    addr, n, dev = _ray_array(points, "points", 3, np.float32)
    iaddr = _input_beside(ids, "ids", np.uint32, n, None, dev, "points live")
    cfg = ProbeSurveyConfig()
    lib().mi355rt_probes_survey_default_config(C.byref(cfg))
    cfg.spp, cfg.first_sample, cfg.accumulate, cfg.flags, cfg.max_distance = int(spp), int(first_sample), 1 if into is not None else 0, SURVEY_FLIP if flip else 0, max_distance
    if into is not None:
        o, odev = _survey_pointers(into, n, "into")
        if odev != dev:
            raise ValueError("into must live where points live")
        out = {k: into[k] for k in PROBE_SURVEY_OUTPUTS}
    else:
        o = ProbeSurvey()
        out = {k: _output(o, k, *(((n,), np.uint32) if k in ("n", "back", "front") else ((n, 4), np.float32)), _device_of(points)) for k in PROBE_SURVEY_OUTPUTS}
    out["max_distance"] = max_distance
    _sync(_device_of(points))                                           # what produced the inputs (and the zero fill) has finished
    self._check(lib().mi355rt_probes_survey(self._h, addr, iaddr, n, C.byref(cfg), RAYS_DEVICE if dev else RAYS_HOST, C.byref(o)))
    return out


def _probes_place(self, grid, survey, offsets=None, back_share=0.25, max_offset=0.45, min_front=None, want=PROBE_PLACE_OUTPUTS):
    """mi355rt_probes_place: where every probe of a grid goes and the state it gets (raytracer_rs_amd.probes.place and probes.classify are the statement);
    traces nothing.  survey: the dict probes_survey returned at probes.grid_points(grid) + offsets; offsets: float32 (nprobes, 3) or None (zero); min_front: a
    length, None: probes.grid_min_front(grid); want: any of "offsets" (float32 (nprobes, 3), new arrays), "verdict" (uint8, PLACE_*), "state" (uint8, PROBE_*).
    numpy arrays or torch tensors on the handle's GPU, all alike.  Returns a tuple in the order of want."""
    want = _check_want(want, PROBE_PLACE_OUTPUTS)
    g = grid if isinstance(grid, ProbeGrid) else ProbeGrid.from_dict(grid)
    nprobes = int(g.counts[0]) * int(g.counts[1]) * int(g.counts[2])
    s, dev = _survey_pointers(survey, nprobes, "survey")
    oaddr = None
    if offsets is not None:
        oaddr, _, odev = _ray_array(offsets, "offsets", 3, np.float32, rows=nprobes)
        if odev != dev:
            raise ValueError("offsets must live where the survey lives (all numpy arrays, or all tensors on the GPU)")
    if min_front is None:
        from . import probes as _probes
        min_front = _probes.grid_min_front(dict(origin=list(g.origin), spacing=list(g.spacing), counts=list(g.counts)))
    cfg = ProbePlaceConfig()
    lib().mi355rt_probes_place_default_config(C.byref(cfg))
    cfg.back_share, cfg.max_offset, cfg.min_front, cfg.max_distance = float(back_share), float(max_offset), float(min_front), float(np.float32(survey.get("max_distance", 0.0)))
    device = _device_of(survey["n"])
    res = {w: _new_output(*(((nprobes, 3), np.float32) if w == "offsets" else ((nprobes,), np.uint8)), device) for w in want}
    addrs = {w: _address(res[w]) if w in res else None for w in PROBE_PLACE_OUTPUTS}
    _sync(device)
    self._check(lib().mi355rt_probes_place(self._h, C.byref(g), C.byref(s), C.byref(cfg), oaddr, RAYS_DEVICE if dev else RAYS_HOST, addrs["offsets"], addrs["verdict"],
                                           addrs["state"]))
    return tuple(res[w] for w in want)


def _probes_lookup_placed(self, grid, res, points, dirs, normals=None, mode="irradiance", usable=None, chebyshev=True, facing=True, normal_bias=0.0, offsets=None,
                          want_ok=False):
    """mi355rt_probes_lookup_placed: probes_lookup_vis for probes that have moved (raytracer_rs_amd.probes.lookup_placed is the statement); traces nothing.
    offsets: float32 (nprobes, 3), the probes' offsets from their grid points, under which `res` was gathered; None: probes_lookup_vis on every bit.  The
    weights use the moved positions, the cell and the trilinear factor the grid.  Everything else as probes_lookup_vis."""
    return self._lookup("probes_lookup_placed", grid, res, points, dirs, mode, usable, want_ok, normals=normals, weights=(chebyshev, facing, normal_bias), offsets=offsets)


def _probes_relocate(self, grid, rounds=4, spp=64, **kw):
    """raytracer_rs_amd.probes.relocate(self, grid, ...): rounds of probes_survey and probes_place from zero offsets, then a last survey and the states.
    device=torch.device("cuda", i): everything stays on the GPU.  Returns dict(offsets, state, usable, points, verdict, survey)."""
    from . import probes as _probes
    return _probes.relocate(self, grid, rounds=rounds, spp=spp, **kw)


RayTracer.probes_survey = _probes_survey
RayTracer.probes_place = _probes_place
RayTracer.probes_lookup_placed = _probes_lookup_placed
RayTracer.probes_relocate = _probes_relocate


# ---- probe-lit shading (include/mi355rt.h, "PROBE-LIT"): the structs, the symbols and the RayTracer methods -----------------------------------
PROBE_LIT_CLAMP = 1                                             # MI355RT_PROBE_LIT_CLAMP
PROBE_LIT_OUTPUTS = ("rgb", "light", "indirect", "tuv", "prim", "ok")


class ProbeVolume(C.Structure):
    """mi355rt_probe_volume: grid, n, sh, usable (may be null), depth with vc (both null, or neither), offsets (may be null; null without depth)"""
    _fields_ = [("grid", C.POINTER(ProbeGrid)), ("n", C.c_void_p), ("sh", C.c_void_p), ("usable", C.c_void_p), ("depth", C.POINTER(ProbeDepth)),
                ("vc", C.POINTER(ProbeVisConfig)), ("offsets", C.c_void_p)]


class ProbeLitOutputs(C.Structure):
    """mi355rt_probe_lit_outputs: rgb, light, indirect, tuv float32 (n, 3); prim uint32 (n,); ok uint8 (n,); any may be null, not all"""
    _fields_ = [("rgb", C.c_void_p), ("light", C.c_void_p), ("indirect", C.c_void_p), ("tuv", C.c_void_p), ("prim", C.c_void_p), ("ok", C.c_void_p)]


ABI += [
    ("mi355rt_probe_lit_points", C.c_int, [_H, C.POINTER(ProbeVolume), C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("mi355rt_probe_lit_rays", C.c_int, [_H, C.POINTER(ProbeVolume), C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(ProbeLitOutputs)]),
    ("mi355rt_probe_lit_one", C.c_int, [C.POINTER(ProbeVolume), _F, _F, C.c_uint32, _F, _U]),
]


def _probe_volume(self, vol):
    """(ProbeVolume, is_device, keep) over the arrays of a probe_lit.volume dict, each checked; keep: what the struct points to"""
    for k in ("grid", "n", "sh", "usable", "depth", "offsets", "chebyshev", "facing", "normal_bias"):
        if k not in vol:
            raise ValueError("volume: holds no %r (probe_lit.volume makes one)" % k)
    g = vol["grid"] if isinstance(vol["grid"], ProbeGrid) else ProbeGrid.from_dict(vol["grid"])
    nprobes = int(g.counts[0]) * int(g.counts[1]) * int(g.counts[2])
    v, devs, keep = ProbeVolume(), [], [g]
    v.grid = C.pointer(g)
    v.n, _, dev = _ray_vector(vol["n"], 'volume["n"]', np.uint32, nprobes)
    devs.append(dev)
    v.sh, _, dev = _film_array(vol["sh"], 'volume["sh"]', (nprobes, 9, 3), np.float32)
    devs.append(dev)
    if vol["usable"] is not None:
        v.usable, _, dev = _ray_vector(vol["usable"], 'volume["usable"]', np.uint8, nprobes)
        devs.append(dev)
    depth = vol["depth"]
    if depth is None:
        if vol["offsets"] is not None:
            raise ValueError('volume["offsets"]: given without volume["depth"]')
    else:
        R = int(depth["res"])
        if not 2 <= R <= 16:
            raise ValueError('volume["depth"]["res"]: 2 .. 16, not %r' % R)
        caddr, _, dev = _film_array(depth["count"], 'volume["depth"]["count"]', (nprobes, R * R), np.uint32)
        devs.append(dev)
        maddr, _, dev = _film_array(depth["moments"], 'volume["depth"]["moments"]', (nprobes, R * R, 2), np.float32)
        devs.append(dev)
        d = ProbeDepth(R, float(np.float32(depth.get("max_distance", 1.0))), caddr, maddr)
        vc = ProbeVisConfig((VIS_CHEBYSHEV if vol["chebyshev"] else 0) | (VIS_FACING if vol["facing"] else 0), float(vol["normal_bias"]))
        keep += [d, vc]
        v.depth, v.vc = C.pointer(d), C.pointer(vc)
        if vol["offsets"] is not None:
            v.offsets, _, dev = _ray_array(vol["offsets"], 'volume["offsets"]', 3, np.float32, rows=nprobes)
            devs.append(dev)
    if len(set(devs)) != 1:
        raise ValueError("volume: its arrays must all live in one place (all numpy arrays, or all tensors on the GPU)")
    return v, devs[0], keep


def _probe_lit_points(self, volume, points, normals, clamp=True, want_ok=False):
    """mi355rt_probe_lit_points: the uniform mean over the hemisphere of each normal of the light a probe volume holds, at surface points
    (raytracer_rs_amd.probe_lit.hemi is the statement): the reference's bounce term, read from the probes without tracing a ray.  volume: what
    probe_lit.volume makes; points, normals: float32 (m, 3).  numpy arrays or torch tensors on the handle's GPU, the volume's arrays alike.  clamp: a negative
    (or NaN) value becomes 0.  Returns indirect float32 (m, 3), with want_ok (indirect, ok uint8 (m,))."""
    v, vdev, _keep = _probe_volume(self, volume)
    addr, m, dev = _ray_array(points, "points", 3, np.float32)
    naddr, _, ndev = _ray_array(normals, "normals", 3, np.float32, rows=m)
    if not (vdev == ndev == dev):
        raise ValueError("normals and the volume must live where points live (all numpy arrays, or all tensors on the GPU)")
    ind, ok, iaddr, okaddr = _rgb_ok(m, want_ok, _device_of(points))
    self._check(lib().mi355rt_probe_lit_points(self._h, C.byref(v), addr, naddr, m, PROBE_LIT_CLAMP if clamp else 0, RAYS_DEVICE if dev else RAYS_HOST, iaddr, okaddr))
    return (ind, ok) if want_ok else ind


def _probe_lit_rays(self, volume, rays6, want=("rgb",), clamp=True, into=None):
    """mi355rt_probe_lit_rays: the radiance along caller-given rays with the bounce tree replaced by one lookup in a probe volume
    (raytracer_rs_amd.probe_lit.rays is the statement): closest hit, the reference's shade() there with shadow rays (`light`: trace_rays' `direct` bit for
    bit), the hemisphere mean of the volume (`indirect`, `ok`), and their sum (`rgb`).  rays6: float32 (n, 6) rows (pos3, dir3), used as given; want: any of
    "rgb", "light", "indirect", "tuv", "prim", "ok".  numpy arrays or torch tensors on the handle's GPU, the volume's arrays alike, under trace_rays' rules.
    into: a dict of arrays to write into (tuv of a miss stays as it was).  Returns a dict name -> array.  No film, camera or lens state changes;
    last_counts() reports n primary rays."""
    want = _check_want(want, PROBE_LIT_OUTPUTS)
    v, vdev, _keep = _probe_volume(self, volume)
    addr, n, dev = _ray_array(rays6, "rays6", 6, np.float32)
    if vdev != dev:
        raise ValueError("the volume must live where rays6 lives (all numpy arrays, or all tensors on the GPU)")
    o, device = ProbeLitOutputs(), _device_of(rays6)
    res = {w: _output(o, w, (n,) if w in ("prim", "ok") else (n, 3), np.uint32 if w == "prim" else np.uint8 if w == "ok" else np.float32, device,
                      into if into is not None and w in into else None, "into must live where rays6 lives") for w in want}
    _sync(device)                                                       # what produced the inputs (and the zero fill) has finished
    self._check(lib().mi355rt_probe_lit_rays(self._h, C.byref(v), addr, n, PROBE_LIT_CLAMP if clamp else 0, RAYS_DEVICE if dev else RAYS_HOST, C.byref(o)))
    return res


def _render_probe_lit(self, volume, spp=1, device=None):
    """A probe-lit frame: lens_rays(spp) under the handle's lens (layout s * npix + p), probe_lit_rays along them, probe_lit.frame_mean over each pixel's
    samples.  It does none of render()'s bounce rounds and touches no film.  device: None — numpy arrays, the volume's too; a torch device (or True) of the
    handle's GPU — tensors there.  Returns dict(mean, light, indirect float32 (height, width, 3); ok_share float32 (height, width): the share of a pixel's samples
    whose lookup used a probe).  display_image(result["mean"]) puts it on the screen."""
    from . import probe_lit as _probe_lit
    spp = int(spp)
    rays6 = self.lens_rays(spp, device=False if device is None else device)
    r = self.probe_lit_rays(volume, rays6, want=("rgb", "light", "indirect", "ok"))
    npix, h, w = self.width * self.height, self.height, self.width
    ok = r["ok"].astype(np.float32) if device is None else r["ok"].float()
    out = {k: _probe_lit.frame_mean(r[s], npix).reshape(h, w, 3) for k, s in (("mean", "rgb"), ("light", "light"), ("indirect", "indirect"))}
    out["ok_share"] = _probe_lit.frame_mean(ok.reshape(-1, 1), npix).reshape(h, w)
    return out


RayTracer.probe_lit_points = _probe_lit_points
RayTracer.probe_lit_rays = _probe_lit_rays
RayTracer.render_probe_lit = _render_probe_lit
