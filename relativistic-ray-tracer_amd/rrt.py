"""ctypes binding of librrt.so (include/rrt.h) -- the host-side mirror of the reference's
PathTracer hot-path interface for Python callers (tests, bench, smoke).

The product path is native: librrt.so (HIP kernels + C ABI).  This module only marshals
arguments; it never computes radiance itself and raises if the library is missing.

Reference correspondence (pathtracer.h / pathtracer.cpp):
    Renderer(device)                  PathTracer ctor (pathtracer.cpp:32-85)
    .set_scene(SceneFile)             PathTracer::set_scene + build_accel (:95-117, :304-328)
    .set_camera(camera)               PathTracer::set_camera (:119-134)
    .set_black_hole(c, r_s, dtheta)   the `-B` override of global_black_hole (main.cpp:139-145)
    .render(params, x0, y0, w, h)     raytrace_tile / raytrace_cell over a region (:549-609)
    .trace_rays(o, d) / .trace_camera BVHAccel::intersect itself, one first-hit record per ray (bvh.cpp:103-113)
    .env_eval(dirs)                   EnvironmentLight::sample_dir (environment_light.cpp:146-148)
    RenderParams(...)                 AppConfig fields (application.h:41-85)
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RRT_LIB") or os.path.join(HERE, "librrt.so")  # RRT_LIB: A/B of builds

RRT_OK, RRT_E_INVALID, RRT_E_HIP, RRT_E_CANCELLED, RRT_E_NO_DEVICE, RRT_E_IO = 0, -1, -2, -3, -4, -5
RRT_RENDER_COUNTERS, RRT_RENDER_DRAWS, RRT_RENDER_WAVEFRONT, RRT_RENDER_EXACT_DIV = 1, 2, 4, 8
RRT_RENDER_PIXEL_LOOP, RRT_RENDER_NO_SKIP, RRT_RENDER_NO_CLEAN, RRT_RENDER_PER_PIXEL = 16, 32, 64, 128
RRT_RENDER_COUNT_EXECUTED, RRT_RENDER_ORDERED, RRT_RENDER_NO_FIRST = 256, 512, 1024
RRT_RENDER_ONE_QUEUE, RRT_RENDER_XCD_QUEUES, RRT_RENDER_NO_MISS_PROOF, RRT_RENDER_PREPASS = 2048, 4096, 8192, 16384
RRT_RENDER_STRIPED_QUEUES, RRT_RENDER_NO_SHADOW_PROOF, RRT_RENDER_NO_PIXEL_PROOF = 1 << 15, 1 << 16, 1 << 17
RRT_RENDER_NO_SEARCH_TREE, RRT_RENDER_DEEP_SAMPLE, RRT_RENDER_NO_HEAVY, RRT_RENDER_HEAVY = 1 << 18, 1 << 19, 1 << 20, 1 << 21
RRT_RENDER_DIAG_NO_TRAVERSE, RRT_RENDER_DIAG_CLEAR_STATS = 1 << 30, 1 << 31
# the reference's compile-time switches (pathtracer.h:4-6, environment_light.h:4, bsdf.h:4) as flags
RRT_RENDER_THIN_LENS, RRT_RENDER_NO_ADAPTIVE, RRT_RENDER_ENV_HEMI, RRT_RENDER_MICROFACET_HEMI = 1 << 22, 1 << 23, 1 << 24, 1 << 25


def RRT_RENDER_ILLUM(n):
    """ILLUM n (pathtracer.h:4) as flag bits 26..27 (ILLUM 2, the default: 0)."""
    return ((n ^ 2) & 3) << 26


class RRTError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"rrt error {code}: {msg}")
        self.code = code


class DeviceCfg(C.Structure):
    _fields_ = [("device", C.c_int), ("free_grid_res", C.c_uint32), ("reserved", C.c_uint32 * 6)]


class CameraDesc(C.Structure):
    _fields_ = [("hFov", C.c_double), ("vFov", C.c_double), ("nClip", C.c_double), ("fClip", C.c_double),
                ("pos", C.c_double * 3), ("c2w", C.c_double * 9), ("lensRadius", C.c_double),
                ("focalDistance", C.c_double)]


class CameraState(C.Structure):
    """The full CGL::Camera record (Camera::dump_settings order; the .rrtc payload)."""
    _fields_ = [("hFov", C.c_double), ("vFov", C.c_double), ("ar", C.c_double), ("nClip", C.c_double),
                ("fClip", C.c_double), ("pos", C.c_double * 3), ("targetPos", C.c_double * 3), ("phi", C.c_double),
                ("theta", C.c_double), ("r", C.c_double), ("minR", C.c_double), ("maxR", C.c_double),
                ("c2w", C.c_double * 9), ("screenW", C.c_double), ("screenH", C.c_double),
                ("screenDist", C.c_double), ("focalDistance", C.c_double), ("lensRadius", C.c_double)]

    def to_array(self):
        return np.frombuffer(bytes(self), np.float64).copy()


class ColladaOptions(C.Structure):
    _fields_ = [("screen_w", C.c_uint32), ("screen_h", C.c_uint32), ("lens_radius", C.c_double),
                ("focal_distance", C.c_double), ("reserved", C.c_uint32 * 4)]


class EnvmapDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("texels", C.c_void_p)]


RRT_METRIC_SCHWARZSCHILD, RRT_METRIC_KERR = 0, 1
RRT_SPACETIME_LENSED_SKY = 1  # rrt_spacetime_desc.flags
RRT_SKY_FAR_M = 1000.0


class SpacetimeDesc(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("flags", C.c_uint32), ("center", C.c_double * 3), ("r_s", C.c_double),
                ("delta_theta", C.c_double), ("spin", C.c_double), ("axis", C.c_double * 3)]


RRT_DISK_NO_REDSHIFT = 1  # rrt_disk_desc.flags
RRT_DISK_BLACKBODY = 4    # the blackbody disk; bit 1 is unassigned and rejected
RRT_DISK_LIGHT = 16       # the disk importance-sampled as a light; bit 3 is unassigned and rejected
RRT_DISK_PROFILE_POWER, RRT_DISK_PROFILE_ZERO_TORQUE = 0, 1  # rrt_disk_desc.profile
RRT_DISK_PROFILE_PAGE_THORNE = 3  # the Page-Thorne flux of the spin in force; 2 is unassigned and rejected
DISK_PROFILES = {"power": RRT_DISK_PROFILE_POWER, "zero-torque": RRT_DISK_PROFILE_ZERO_TORQUE,
                 "page-thorne": RRT_DISK_PROFILE_PAGE_THORNE}


class DiskDesc(C.Structure):  # rrt_disk_desc
    _fields_ = [("r_in", C.c_double), ("r_out", C.c_double), ("emission", C.c_float * 3), ("flags", C.c_uint32),
                ("temperature", C.c_float), ("profile", C.c_uint32), ("reserved", C.c_uint32 * 2)]


RRT_OBSERVER_FRAME_STATIC, RRT_OBSERVER_FRAME_COORDINATE = 0, 1  # rrt_observer_desc.frame
RRT_OBSERVER_NO_BEAMING = 1  # rrt_observer_desc.flags: every factor 1, aberration alone
OBSERVER_FRAMES = {"static": RRT_OBSERVER_FRAME_STATIC, "coordinate": RRT_OBSERVER_FRAME_COORDINATE}
OBSERVER_RESOLVED = ("f", "sg", "alpha", "D_g", "ig", "gamma", "kappa", "l_w", "b2", "identity")


class ObserverDesc(C.Structure):  # rrt_observer_desc
    _fields_ = [("velocity", C.c_double * 3), ("frame", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 4)]


class RenderParams(C.Structure):
    _fields_ = [("ns_aa", C.c_uint32), ("max_ray_depth", C.c_uint32), ("ns_area_light", C.c_uint32),
                ("samples_per_batch", C.c_uint32), ("max_tolerance", C.c_float),
                ("direct_hemisphere", C.c_uint32), ("seed", C.c_uint64), ("frame_w", C.c_uint32),
                ("frame_h", C.c_uint32), ("flags", C.c_uint32), ("variant", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("n_prims", C.c_uint32), ("n_nodes", C.c_uint32), ("n_leaf_refs", C.c_uint32),
                ("max_depth", C.c_uint32), ("device_bytes", C.c_uint64), ("grid_n", C.c_uint32 * 3),
                ("n_clean", C.c_uint32), ("n_big", C.c_uint32),
                ("grid_free_frac", C.c_float), ("last_kernel_ms", C.c_float), ("grid_blocks", C.c_uint32),
                ("block_threads", C.c_uint32), ("kernel", C.c_char * 64), ("last_main_kernel_ms", C.c_float),
                ("last_heavy_pixels", C.c_uint32), ("last_cont_pixels", C.c_uint32)]


# ray queries (include/rrt.h "ray queries")
RRT_RAY_MISS, RRT_RAY_HIT, RRT_RAY_CAPTURED, RRT_RAY_ESCAPED = 0, 1, 2, 3
RRT_RAY_DISK = 4  # with a disk set (set_disk) only
RRT_TRACE_ANY_HIT, RRT_TRACE_EXIT = 1, 4  # (bit 1 is unassigned)
RRT_TRACE_AUTO, RRT_TRACE_LANE_PER_RAY, RRT_TRACE_WAVE_PER_RAY = 0, 1, 2
TRACE_MODES = {"auto": RRT_TRACE_AUTO, "lane": RRT_TRACE_LANE_PER_RAY, "wave": RRT_TRACE_WAVE_PER_RAY}
RAY_DTYPE = np.dtype([("o", np.float64, 3), ("d", np.float64, 3)])  # rrt_ray, 48 bytes
HIT_DTYPE = np.dtype([("hit_p", np.float64, 3), ("n", np.float64, 3), ("w_out", np.float64, 3), ("t", np.float64),
                      ("status", np.uint32), ("prim", np.int32), ("bsdf", np.int32), ("steps", np.uint32)])  # rrt_hit, 96


class TraceParams(C.Structure):  # rrt_trace_params
    _fields_ = [("flags", C.c_uint32), ("mode", C.c_uint32), ("reserved", C.c_uint32 * 6)]


def trace_params(any_hit=False, mode="auto", exit=False):
    p = TraceParams()
    p.flags = (RRT_TRACE_ANY_HIT if any_hit else 0) | (RRT_TRACE_EXIT if exit else 0)
    p.mode = TRACE_MODES[mode] if isinstance(mode, str) else int(mode)
    return p


# every symbol include/rrt.h declares (checked by tests/test_capi_host.py)
EXPORTS = ["rrt_abi_version", "rrt_create", "rrt_destroy", "rrt_last_error", "rrt_set_scene", "rrt_set_camera",
           "rrt_set_spacetime", "rrt_render_params_default", "rrt_render", "rrt_render_tiles_device",
           "rrt_unpack_tiles_device", "rrt_tonemap_device", "rrt_partition_tiles", "rrt_region_tiles", "rrt_get_stats", "rrt_get_launch_times", "rrt_get_bvh", "rrt_get_free_grid", "rrt_get_clean_tree", "rrt_get_search_tree", "rrt_proof_envelope",
           "rrt_scene_file_load", "rrt_scene_file_desc", "rrt_scene_file_free", "rrt_camera_file_load",
           "rrt_scene_file_save", "rrt_collada_options_default", "rrt_collada_load", "rrt_camera_settings_load",
           "rrt_camera_settings_save", "rrt_camera_state_file_load", "rrt_camera_state_file_save",
           "rrt_camera_state_desc", "rrt_set_envmap", "rrt_tonemap_pixel", "rrt_write_png",
           "rrt_exr_load", "rrt_exr_free", "rrt_exr_save", "rrt_kerr_frame", "rrt_get_big_masks",
           "rrt_get_occluders", "rrt_group_create", "rrt_group_render", "rrt_group_destroy", "rrt_libm_eval",
           "rrt_set_proof_audit", "rrt_get_proof_audit", "rrt_get_search_tree4", "rrt_trace_rays",
           "rrt_trace_rays_device", "rrt_trace_camera", "rrt_trace_camera_device", "rrt_env_eval", "rrt_set_disk",
           "rrt_get_disk", "rrt_disk_eval", "rrt_blackbody_tint", "rrt_disk_sample",
           "rrt_plan_prove_first", "rrt_set_observer", "rrt_get_observer", "rrt_observer_eval"]
AUDIT_KINDS = ("camera", "shadow", "pixel", "strip", "kerr", "zero")  # include/rrt.h RRT_AUDIT_*

_lib = None


def build_id():
    """First 16 hex digits of the sha256 of the librrt.so this process loads (ties measured
    profiles -- PMC counters, traffic -- to the exact kernel build they were taken on)."""
    import hashlib
    with open(LIB_PATH, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def lib():
    """Load librrt.so (fails loudly if it was not built: there is no fallback path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RRTError(RRT_E_IO, f"{LIB_PATH} not built (run `make -C relativistic-ray-tracer_amd`)")
        L = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        L.rrt_create.argtypes = [C.POINTER(vp), C.POINTER(DeviceCfg)]
        L.rrt_destroy.argtypes = [vp]
        L.rrt_last_error.restype = C.c_char_p
        L.rrt_last_error.argtypes = [vp]
        L.rrt_set_scene.argtypes = [vp, vp]
        L.rrt_set_camera.argtypes = [vp, C.POINTER(CameraDesc)]
        L.rrt_set_spacetime.argtypes = [vp, C.POINTER(SpacetimeDesc)]
        if hasattr(L, "rrt_kerr_frame"):
            L.rrt_kerr_frame.argtypes = [vp, vp, vp, vp]
            L.rrt_kerr_frame.restype = None
        if hasattr(L, "rrt_set_envmap"):
            L.rrt_set_envmap.argtypes = [vp, C.POINTER(EnvmapDesc)]
            L.rrt_exr_load.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_uint32),
                                       C.POINTER(C.c_uint32)]
            L.rrt_exr_free.argtypes = [vp]
        L.rrt_render_params_default.argtypes = [C.POINTER(RenderParams)]
        L.rrt_render.argtypes = [vp, C.POINTER(RenderParams), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp,
                                 vp, vp, vp]
        L.rrt_render_tiles_device.argtypes = [vp, C.POINTER(RenderParams), vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
        L.rrt_unpack_tiles_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp,
                                              vp]
        L.rrt_tonemap_device.argtypes = [vp, C.c_uint32, vp, vp, vp]
        L.rrt_partition_tiles.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint32]
        if hasattr(L, "rrt_region_tiles"):  # absent from older builds loaded through RRT_LIB
            L.rrt_region_tiles.argtypes = [C.c_uint32] * 7 + [vp, C.c_uint32]
        L.rrt_get_stats.argtypes = [vp, C.POINTER(Stats)]
        if hasattr(L, "rrt_plan_prove_first"):  # absent from older builds loaded through RRT_LIB
            L.rrt_plan_prove_first.argtypes = []
            L.rrt_plan_prove_first.restype = C.c_uint32
        L.rrt_get_launch_times.argtypes = [vp, C.c_uint32, vp, vp]
        L.rrt_libm_eval.argtypes = [vp, C.c_int, vp, vp, vp, C.c_uint64]
        if hasattr(L, "rrt_env_eval"):  # absent from older builds loaded through RRT_LIB
            L.rrt_env_eval.argtypes = [vp, vp, C.c_uint64, vp]
        if hasattr(L, "rrt_set_disk"):  # absent from older builds loaded through RRT_LIB
            L.rrt_set_disk.argtypes = [vp, C.POINTER(DiskDesc)]
            L.rrt_get_disk.argtypes = [vp, C.POINTER(DiskDesc)]
        if hasattr(L, "rrt_disk_eval"):  # absent from older builds loaded through RRT_LIB
            L.rrt_disk_eval.argtypes = [vp, vp, vp, C.c_uint64, vp]
            L.rrt_blackbody_tint.argtypes = [C.c_double, C.POINTER(C.c_float * 3)]
        if hasattr(L, "rrt_disk_sample"):  # absent from older builds loaded through RRT_LIB
            L.rrt_disk_sample.argtypes = [vp, vp, vp, C.c_uint64, vp, vp]
        if hasattr(L, "rrt_set_observer"):  # absent from older builds loaded through RRT_LIB
            L.rrt_set_observer.argtypes = [vp, C.POINTER(ObserverDesc)]
            L.rrt_get_observer.argtypes = [vp, C.POINTER(ObserverDesc), vp]
            L.rrt_observer_eval.argtypes = [vp, vp, C.c_uint64, vp, vp, vp]
        if hasattr(L, "rrt_set_proof_audit"):  # absent from older builds loaded through RRT_LIB
            L.rrt_set_proof_audit.argtypes = [vp, C.c_int]
            L.rrt_get_proof_audit.argtypes = [vp, vp]
        L.rrt_proof_envelope.argtypes = [vp]
        if hasattr(L, "rrt_trace_rays"):  # absent from older builds loaded through RRT_LIB
            tp = C.POINTER(TraceParams)
            L.rrt_trace_rays.argtypes = [vp, tp, vp, C.c_uint32, vp]
            L.rrt_trace_rays_device.argtypes = [vp, tp, vp, C.c_uint32, vp, vp]
            L.rrt_trace_camera.argtypes = [vp, tp] + [C.c_uint32] * 6 + [vp]
            L.rrt_trace_camera_device.argtypes = [vp, tp] + [C.c_uint32] * 6 + [vp, vp]
        L.rrt_get_bvh.argtypes = [vp, vp, vp, vp]
        for name, n_args in (("rrt_get_free_grid", 4), ("rrt_get_clean_tree", 5), ("rrt_get_search_tree", 3),
                             ("rrt_get_search_tree4", 3),
                             ("rrt_get_big_masks", 3),
                             ("rrt_get_occluders", 3)):
            if hasattr(L, name):  # absent from older builds loaded through RRT_LIB
                getattr(L, name).argtypes = [vp] * n_args
        L.rrt_scene_file_load.argtypes = [C.c_char_p, C.POINTER(vp)]
        L.rrt_scene_file_desc.restype = vp
        L.rrt_scene_file_desc.argtypes = [vp]
        L.rrt_scene_file_free.argtypes = [vp]
        L.rrt_camera_file_load.argtypes = [C.c_char_p, C.POINTER(CameraDesc)]
        if hasattr(L, "rrt_collada_load"):  # absent from older builds loaded through RRT_LIB
            L.rrt_scene_file_save.argtypes = [C.c_char_p, vp]
            L.rrt_collada_options_default.argtypes = [C.POINTER(ColladaOptions)]
            L.rrt_collada_load.argtypes = [C.c_char_p, C.POINTER(ColladaOptions), C.POINTER(vp),
                                           C.POINTER(CameraState), C.c_char_p, C.c_size_t]
            for name in ("rrt_camera_settings_load", "rrt_camera_state_file_load"):
                getattr(L, name).argtypes = [C.c_char_p, C.POINTER(CameraState)]
            for name in ("rrt_camera_settings_save", "rrt_camera_state_file_save"):
                getattr(L, name).argtypes = [C.c_char_p, C.POINTER(CameraState)]
            L.rrt_camera_state_desc.argtypes = [C.POINTER(CameraState), C.POINTER(CameraDesc)]
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data


class ObjectDesc(C.Structure):  # rrt_object_desc
    _fields_ = [("kind", C.c_uint32), ("bsdf", C.c_uint32), ("n_vertices", C.c_uint32), ("n_triangles", C.c_uint32),
                ("positions", C.POINTER(C.c_double)), ("normals", C.POINTER(C.c_double)),
                ("indices", C.POINTER(C.c_uint32)), ("center", C.c_double * 3), ("radius", C.c_double)]


class LightDesc(C.Structure):  # rrt_light_desc
    _fields_ = [("type", C.c_uint32), ("is_delta", C.c_uint32), ("radiance", C.c_float * 3), ("area", C.c_float),
                ("v", (C.c_double * 3) * 4)]


class SceneDesc(C.Structure):  # rrt_scene_desc
    _fields_ = [("n_objects", C.c_uint32), ("n_bsdfs", C.c_uint32), ("n_lights", C.c_uint32), ("reserved", C.c_uint32),
                ("objects", C.POINTER(ObjectDesc)), ("bsdfs", C.c_void_p), ("lights", C.POINTER(LightDesc))]


class SceneFile:
    """A flattened static scene (.rrts, include/rrt_scene_format.h) loaded by librrt."""

    def __init__(self, path=None, handle=None):
        if handle is None:
            h = C.c_void_p()
            rc = lib().rrt_scene_file_load(path.encode(), C.byref(h))
            if rc != RRT_OK:
                raise RRTError(rc, f"cannot load scene {path}")
            handle = h
        self.h = handle

    def desc(self):
        return lib().rrt_scene_file_desc(self.h)

    def triangles(self):
        """[n, 3, 3] vertex positions of every mesh triangle, in object / BVH build order."""
        d = SceneDesc.from_address(self.desc())
        out = []
        for i in range(d.n_objects):
            o = d.objects[i]
            if o.kind != 0 or o.n_triangles == 0:
                continue
            P = np.ctypeslib.as_array(o.positions, shape=(o.n_vertices * 3,)).reshape(-1, 3)
            idx = np.ctypeslib.as_array(o.indices, shape=(o.n_triangles * 3,)).reshape(-1, 3)
            out.append(P[idx])
        return np.concatenate(out) if out else np.zeros((0, 3, 3))

    def lights(self):
        """[(type, is_delta, v [4][3])] of the scene's lights."""
        d = SceneDesc.from_address(self.desc())
        return [(d.lights[i].type, d.lights[i].is_delta, np.array(d.lights[i].v, np.float64))
                for i in range(d.n_lights)]

    def save(self, path):
        rc = lib().rrt_scene_file_save(path.encode(), self.desc())
        if rc != RRT_OK:
            raise RRTError(rc, f"cannot write {path}")

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.rrt_scene_file_free(self.h)
            self.h = None


def load_collada(path, screen_w=800, screen_h=600, lens_radius=0.25, focal_distance=4.7):
    """Native COLLADA ingest: (SceneFile, CameraState) as the reference's loader + Application::load
    produce them for a `-r screen_w screen_h` render (include/rrt.h rrt_collada_load)."""
    o = ColladaOptions()
    lib().rrt_collada_options_default(C.byref(o))
    o.screen_w, o.screen_h, o.lens_radius, o.focal_distance = screen_w, screen_h, lens_radius, focal_distance
    h = C.c_void_p()
    cam = CameraState()
    err = C.create_string_buffer(512)
    rc = lib().rrt_collada_load(path.encode(), C.byref(o), C.byref(h), C.byref(cam), err, len(err))
    if rc != RRT_OK:
        raise RRTError(rc, err.value.decode(errors="replace"))
    return SceneFile(handle=h), cam


def camera_desc(state):
    """The rrt_set_camera subset of a CameraState."""
    cam = CameraDesc()
    rc = lib().rrt_camera_state_desc(C.byref(state), C.byref(cam))
    if rc != RRT_OK:
        raise RRTError(rc, "bad camera state")
    return cam


def load_camera_settings(path):
    """Camera::load_settings text file (the `-c` flag)."""
    st = CameraState()
    rc = lib().rrt_camera_settings_load(path.encode(), C.byref(st))
    if rc != RRT_OK:
        raise RRTError(rc, f"cannot read camera settings {path}")
    return st


def load_camera_state(path):
    """.rrtc record as a CameraState."""
    st = CameraState()
    rc = lib().rrt_camera_state_file_load(path.encode(), C.byref(st))
    if rc != RRT_OK:
        raise RRTError(rc, f"cannot load camera {path}")
    return st


def load_camera(path):
    cam = CameraDesc()
    rc = lib().rrt_camera_file_load(path.encode(), C.byref(cam))
    if rc != RRT_OK:
        raise RRTError(rc, f"cannot load camera {path}")
    return cam


def kerr_frame(axis=(0.0, 1.0, 0.0)):
    """(ex, ey, ez) of the Kerr local frame the library uses for this spin axis."""
    a = np.ascontiguousarray(axis, np.float64)
    out = np.zeros((3, 3), np.float64)
    lib().rrt_kerr_frame(a.ctypes.data, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data)
    return out


def blackbody_tint(temperature):
    """The three-wavelength Planck colour of a blackbody at `temperature` Kelvin (1000..1e6) normalised to
    G = 1, a float tuple (rrt_blackbody_tint): the physical emission of a blackbody disk."""
    out = (C.c_float * 3)()
    rc = lib().rrt_blackbody_tint(float(temperature), C.byref(out))
    if rc != RRT_OK:
        raise RRTError(rc, "blackbody_tint: the temperature must lie in [1000, 1e6] K")
    return tuple(out)


def load_exr(path):
    """Environment map texels [h][w][3] float32 (rrt_exr_load: main.cpp's load_exr)."""
    t = C.POINTER(C.c_float)()
    w, h = C.c_uint32(), C.c_uint32()
    rc = lib().rrt_exr_load(path.encode(), C.byref(t), C.byref(w), C.byref(h))
    if rc != RRT_OK:
        raise RRTError(rc, f"cannot load {path}")
    arr = np.ctypeslib.as_array(t, shape=(h.value, w.value, 3)).copy()
    lib().rrt_exr_free(t)
    return arr


def render_params(frame_w, frame_h, ns_aa=1, max_ray_depth=1, ns_area_light=1, samples_per_batch=32,
                  max_tolerance=0.05, direct_hemisphere=False, seed=0, flags=0, variant=0):
    p = RenderParams()
    lib().rrt_render_params_default(C.byref(p))
    p.ns_aa, p.max_ray_depth, p.ns_area_light = ns_aa, max_ray_depth, ns_area_light
    p.samples_per_batch, p.max_tolerance, p.direct_hemisphere = samples_per_batch, max_tolerance, int(direct_hemisphere)
    p.seed, p.frame_w, p.frame_h, p.flags, p.variant = seed, frame_w, frame_h, flags, variant
    return p


def partition_tiles(frame_w, frame_h, tile_size, rank, world):
    n = lib().rrt_partition_tiles(frame_w, frame_h, tile_size, rank, world, None, 0)
    if n < 0:
        raise RRTError(n, "bad partition arguments")
    out = np.zeros((max(n, 1), 2), np.uint32)
    lib().rrt_partition_tiles(frame_w, frame_h, tile_size, rank, world, out.ctypes.data, n)
    return out[:n]


def region_tiles(x0, y0, w, h, tile_size, rank, world):
    """rrt_region_tiles: rank's tiles of the region's lattice deal (rrt_group_render's split)."""
    n = lib().rrt_region_tiles(x0, y0, w, h, tile_size, rank, world, None, 0)
    if n < 0:
        raise RRTError(n, "bad partition arguments")
    out = np.zeros((max(n, 1), 2), np.uint32)
    lib().rrt_region_tiles(x0, y0, w, h, tile_size, rank, world, out.ctypes.data, n)
    return out[:n]


class Renderer:
    """One rendering context on one HIP device (device=-1: host-only, for BVH/host tests)."""

    def __init__(self, device=0, free_grid_res=0):
        cfg = DeviceCfg()
        cfg.device = device
        cfg.free_grid_res = free_grid_res
        h = C.c_void_p()
        rc = lib().rrt_create(C.byref(h), C.byref(cfg))
        if rc != RRT_OK:
            raise RRTError(rc, f"rrt_create(device={device}) failed")
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.rrt_destroy(self.h)
            self.h = None

    __del__ = close

    def _chk(self, rc):
        if rc != RRT_OK:
            raise RRTError(rc, lib().rrt_last_error(self.h).decode())

    def set_scene(self, scene_file):
        self._scene = scene_file
        self._chk(lib().rrt_set_scene(self.h, scene_file.desc()))

    def set_camera(self, cam):
        self._chk(lib().rrt_set_camera(self.h, C.byref(cam)))

    def set_black_hole(self, center=(0.0, 1.0, 0.0), r_s=0.1, delta_theta=0.1, spin=None, axis=(0.0, 1.0, 0.0),
                       lensed_sky=False):
        """The global black hole (-B).  spin=None: Schwarzschild (the reference's stepper);
        spin=a/M in [0, 1): the Kerr integrator (build-defined) about `axis`.
        lensed_sky: escaping rays take the environment map along their exit direction and the
        hole's shadow is black (RRT_SPACETIME_LENSED_SKY)."""
        st = SpacetimeDesc()
        st.flags = RRT_SPACETIME_LENSED_SKY if lensed_sky else 0
        st.kind = RRT_METRIC_SCHWARZSCHILD if spin is None else RRT_METRIC_KERR
        st.center[0], st.center[1], st.center[2] = center
        st.r_s, st.delta_theta = r_s, delta_theta
        if spin is not None:
            st.spin = spin
            st.axis[0], st.axis[1], st.axis[2] = axis
        self._chk(lib().rrt_set_spacetime(self.h, C.byref(st)))

    def set_envmap(self, texels):
        """Environment map ([h][w][3] float32) or None (the PathTracer ctor's envmap argument)."""
        if texels is None:
            self._chk(lib().rrt_set_envmap(self.h, None))
            return
        t = np.ascontiguousarray(texels, np.float32)
        d = EnvmapDesc()
        d.width, d.height, d.texels = t.shape[1], t.shape[0], t.ctypes.data
        self._chk(lib().rrt_set_envmap(self.h, C.byref(d)))

    LIBM_FN = {"sin": 0, "cos": 1, "acos": 2, "atan2": 3, "sinf": 4, "cosf": 5, "exp": 6, "log": 7, "erf": 8,
               "atan": 9, "tan": 10}

    def set_disk(self, r_in=0.0, r_out=None, emission=None, redshift=True, temperature=None, profile="power",
                 light=False):
        """The thin accretion disk of a Kerr hole (rrt_set_disk): the annulus r_in..r_out
        (in M; r_in=0: the prograde ISCO of the spin in force) of the equatorial plane, radiance
        emission x (r_in / r)^3 x g^4; redshift=False: g = 1.  set_disk(None) removes it.
        temperature (Kelvin, 1000..1e6): the blackbody disk with the temperature profile
        "power" (T ~ r^-3/4, `temperature` at r_in), "zero-torque" (`temperature` at its peak,
        r = 49/36 r_in) or "page-thorne" (T^4 follows the Page-Thorne flux of the spin in
        force, `temperature` at its peak, the inner edge black); emission is then the colour of gas at `temperature` seen at g = 1.
        emission=None: (1, 1, 1), with a temperature blackbody_tint(temperature).
        light=True (RRT_DISK_LIGHT): importance-sampled direct light samples the disk too,
        ns_area_light points of its flat image, after the listed lights."""
        if r_in is None:
            self._chk(lib().rrt_set_disk(self.h, None))
            return
        if r_out is None:
            raise ValueError("set_disk needs r_out")
        d = DiskDesc()
        d.r_in, d.r_out = r_in, r_out
        d.flags = (0 if redshift else RRT_DISK_NO_REDSHIFT) | (RRT_DISK_LIGHT if light else 0)
        if temperature is not None:
            d.flags |= RRT_DISK_BLACKBODY
            d.temperature = temperature
            d.profile = DISK_PROFILES[profile] if isinstance(profile, str) else profile
            if emission is None and 1000.0 <= d.temperature <= 1e6:  # (else rrt_set_disk rejects the descriptor)
                emission = blackbody_tint(d.temperature)  # of the float the descriptor holds
        d.emission[0], d.emission[1], d.emission[2] = (1.0, 1.0, 1.0) if emission is None else emission
        self._chk(lib().rrt_set_disk(self.h, C.byref(d)))

    def get_disk(self):
        """The disk in force as a dict (r_in resolved: 0 -> the ISCO of a Kerr spacetime), or None.
        "temperature" and "profile" are there for a blackbody disk, "light": True for a disk light."""
        d = DiskDesc()
        if not lib().rrt_get_disk(self.h, C.byref(d)):
            return None
        out = {"r_in": d.r_in, "r_out": d.r_out, "emission": tuple(d.emission),
               "redshift": not (d.flags & RRT_DISK_NO_REDSHIFT)}
        if d.flags & RRT_DISK_BLACKBODY:
            out["temperature"] = d.temperature
            out["profile"] = {v: k for k, v in DISK_PROFILES.items()}[d.profile]
        if d.flags & RRT_DISK_LIGHT:
            out["light"] = True
        return out

    def disk_sample(self, p, uv):
        """The device's sampler of the disk light (rrt_disk_sample) for the disk in force,
        at the world points p [n, 3] with the draws uv [n, 2]: (wi float64 [n, 3], pdf float32 [n]); an
        invalid sample has pdf 0."""
        p = np.ascontiguousarray(np.asarray(p, np.float64).reshape(-1, 3))
        uv = np.ascontiguousarray(np.asarray(uv, np.float64).reshape(-1, 2))
        if len(p) != len(uv):
            raise ValueError("disk_sample needs as many draws as points")
        wi = np.zeros((len(p), 3), np.float64)
        pdf = np.zeros(len(p), np.float32)
        self._chk(lib().rrt_disk_sample(self.h, _p(p), _p(uv), len(p), _p(wi), _p(pdf)))
        return wi, pdf

    def disk_eval(self, r_m, g):
        """The device's colour rule of the disk in force (rrt_disk_eval) at the
        Boyer-Lindquist radii r_m [n] (in M) and redshifts g [n]: float32 [n, 3]."""
        r_m = np.ascontiguousarray(np.asarray(r_m, np.float64).ravel())
        g = np.ascontiguousarray(np.asarray(g, np.float64).ravel())
        if len(r_m) != len(g):
            raise ValueError("disk_eval needs as many redshifts as radii")
        out = np.zeros((len(r_m), 3), np.float32)
        self._chk(lib().rrt_disk_eval(self.h, _p(r_m), _p(g), len(r_m), _p(out)))
        return out

    def set_observer(self, velocity=None, frame="static", beaming=True):
        """The moving observer of a Kerr hole (rrt_set_observer): the camera moves with
        `velocity` (beta, in units of c; world components read in the static observer's triad at the
        camera), so its rays are aberrated and every camera sample is scaled by the photon's energy in
        its frame.  frame="coordinate" reads the coordinate axes as the static frame (with a zero
        velocity: the identity, bit for bit the render without an observer).  beaming=False
        (RRT_OBSERVER_NO_BEAMING): aberration alone.  set_observer(None) removes it."""
        if velocity is None:
            self._chk(lib().rrt_set_observer(self.h, None))
            return
        d = ObserverDesc()
        d.velocity[0], d.velocity[1], d.velocity[2] = (float(v) for v in velocity)
        d.frame = OBSERVER_FRAMES[frame] if isinstance(frame, str) else frame
        d.flags = 0 if beaming else RRT_OBSERVER_NO_BEAMING
        self._chk(lib().rrt_set_observer(self.h, C.byref(d)))

    def get_observer(self):
        """The observer in force as a dict ("velocity", "frame", "beaming") or None.  With a camera and a
        Kerr spacetime set, "resolved" holds the constants a launch would resolve now (OBSERVER_RESOLVED:
        f, sg, alpha, D_g, ig, gamma, kappa, l_w (3), b2, identity)."""
        d = ObserverDesc()
        res = np.full(12, np.nan, np.float64)
        if not lib().rrt_get_observer(self.h, C.byref(d), _p(res)):
            return None
        out = {"velocity": tuple(d.velocity), "frame": {v: k for k, v in OBSERVER_FRAMES.items()}[d.frame],
               "beaming": not (d.flags & RRT_OBSERVER_NO_BEAMING)}
        if not np.isnan(res[11]):
            out["resolved"] = {"f": res[0], "sg": res[1], "alpha": res[2], "D_g": res[3], "ig": res[4], "gamma": res[5],
                               "kappa": res[6], "l_w": res[7:10].copy(), "b2": res[10], "identity": bool(res[11])}
        return out

    def observer_eval(self, dirs):
        """The device's observer rule (rrt_observer_eval) on the unit directions dirs [n, 3]
        of the moving camera's rest frame: (d_eff float64 [n, 3], D_v float64 [n], D float64 [n])."""
        dirs = np.ascontiguousarray(np.asarray(dirs, np.float64).reshape(-1, 3))
        d_eff = np.zeros((len(dirs), 3), np.float64)
        dv = np.zeros(len(dirs), np.float64)
        dd = np.zeros(len(dirs), np.float64)
        self._chk(lib().rrt_observer_eval(self.h, _p(dirs), len(dirs), _p(d_eff), _p(dv), _p(dd)))
        return d_eff, dv, dd

    def libm_eval(self, fn, a, b=None):
        """The device's restated host-libm function `fn` (rrt_glibm.h) on float64 arrays a (, b)."""
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
        out = np.empty_like(a)
        self._chk(lib().rrt_libm_eval(self.h, self.LIBM_FN[fn], _p(a), _p(b), _p(out), a.size))
        return out

    def env_eval(self, dirs):
        """The device's EnvironmentLight::sample_dir on directions dirs [n, 3]: float32 [n, 3] (rrt_env_eval)."""
        dirs = np.ascontiguousarray(np.asarray(dirs, np.float64).reshape(-1, 3))
        out = np.zeros((len(dirs), 3), np.float32)
        self._chk(lib().rrt_env_eval(self.h, _p(dirs), len(dirs), _p(out)))
        return out

    def render(self, params, x0, y0, w, h, draws=False, counters=False):
        rgb = np.zeros((h, w, 3), np.float32)
        cnt = np.zeros((h, w), np.int32)
        dr = np.zeros((h, w), np.uint32) if draws else None
        ct = np.zeros((h, w, 4), np.uint32) if counters else None
        self._chk(lib().rrt_render(self.h, C.byref(params), x0, y0, w, h, _p(rgb), _p(cnt), _p(dr), _p(ct), None))
        return rgb, cnt, dr, ct

    def render_tiles_device(self, params, tiles, tile_size, d_rgb, d_count, d_counters=None, stream=None):
        tiles = np.ascontiguousarray(tiles, dtype=np.uint32)
        self._chk(lib().rrt_render_tiles_device(self.h, C.byref(params), _p(tiles), len(tiles), tile_size, d_rgb,
                                                d_count, d_counters, stream))

    def unpack_tiles_device(self, tiles, tile_size, frame_w, frame_h, rgb_p, cnt_p, rgb, cnt, stream=None):
        tiles = np.ascontiguousarray(tiles, dtype=np.uint32)
        self._chk(lib().rrt_unpack_tiles_device(self.h, _p(tiles), len(tiles), tile_size, frame_w, frame_h, rgb_p,
                                                cnt_p, rgb, cnt, stream))

    def tonemap_device(self, n, d_rgb, d_rgba, stream=None):
        self._chk(lib().rrt_tonemap_device(self.h, n, d_rgb, d_rgba, stream))

    def trace_rays(self, o, d, any_hit=False, mode="auto", exit=False):
        """BVHAccel::intersect (bvh.cpp:103-113) of the rays (o [n, 3], d [n, 3]) under the context's
        spacetime: a structured array [n] with the layout of rrt_hit (HIT_DTYPE).  any_hit: the
        shadow query (status and steps only).  mode: "auto", "lane" or "wave" (RRT_TRACE_*).
        exit: exit mode (RRT_TRACE_EXIT): an escaping ray's record is RRT_RAY_ESCAPED, w_out minus
        its exit direction."""
        o = np.asarray(o, np.float64).reshape(-1, 3)
        d = np.asarray(d, np.float64).reshape(-1, 3)
        if len(o) != len(d):
            raise ValueError("o and d differ in length")
        rays = np.empty(len(o), RAY_DTYPE)
        rays["o"], rays["d"] = o, d
        hits = np.zeros(len(o), HIT_DTYPE)
        self._chk(lib().rrt_trace_rays(self.h, C.byref(trace_params(any_hit, mode, exit)), _p(rays), len(rays), _p(hits)))
        return hits

    def trace_camera(self, frame_w, frame_h, x0, y0, w, h, any_hit=False, mode="auto", exit=False):
        """The same query for the pixel-centre camera rays of a region of a frame_w x frame_h frame
        (raytrace_pixel's ray with ns_aa == 1): a structured array [h, w], y = 0 at the bottom."""
        hits = np.zeros((h, w), HIT_DTYPE)
        self._chk(lib().rrt_trace_camera(self.h, C.byref(trace_params(any_hit, mode, exit)), frame_w, frame_h, x0, y0, w, h,
                                         _p(hits)))
        return hits

    def trace_rays_device(self, d_rays, n, d_hits, any_hit=False, mode="auto", stream=None, exit=False):
        """Asynchronous form on device buffers (rrt_ray [n] -> rrt_hit [n], 16-byte aligned), like
        render_tiles_device."""
        self._chk(lib().rrt_trace_rays_device(self.h, C.byref(trace_params(any_hit, mode, exit)), d_rays, n, d_hits, stream))

    def trace_camera_device(self, frame_w, frame_h, x0, y0, w, h, d_hits, any_hit=False, mode="auto", stream=None,
                            exit=False):
        self._chk(lib().rrt_trace_camera_device(self.h, C.byref(trace_params(any_hit, mode, exit)), frame_w, frame_h, x0, y0,
                                                w, h, d_hits, stream))

    def stats(self):
        s = Stats()
        self._chk(lib().rrt_get_stats(self.h, C.byref(s)))
        return s

    def set_proof_audit(self, every_log2):
        """Counting launches (RRT_RENDER_COUNTERS | RRT_RENDER_COUNT_EXECUTED) re-march every
        2^every_log2-th proven ray exactly (rrt_set_proof_audit); every_log2 < 0 turns it off."""
        self._chk(lib().rrt_set_proof_audit(self.h, every_log2))

    def proof_audit(self):
        """{proof: {"checked": n, "violations": m}} since the last call (rrt_get_proof_audit; resets)."""
        out = np.zeros(2 * len(AUDIT_KINDS), np.uint64)
        self._chk(lib().rrt_get_proof_audit(self.h, _p(out)))
        return {k: {"checked": int(out[2 * i]), "violations": int(out[2 * i + 1])} for i, k in enumerate(AUDIT_KINDS)}

    def launch_times(self, n):
        """HIP-event ms of the last n (<= 32) launches, oldest first: (whole launch, main kernel)."""
        tot, main = np.zeros(n, np.float32), np.zeros(n, np.float32)
        k = lib().rrt_get_launch_times(self.h, n, _p(tot), _p(main))
        if k < 0:
            self._chk(k)
        return tot[:k], main[:k]

    def search_tree4(self):
        """(boxes [n, 4, 6] f32, kids [n, 4, 3] = child, first, count) of the 4-wide walk's nodes."""
        n = lib().rrt_get_search_tree4(self.h, None, None)
        if n < 0:
            self._chk(n)
        b = np.zeros((max(n, 1), 4, 6), np.float32)
        k = np.zeros((max(n, 1), 4, 3), np.int32)
        lib().rrt_get_search_tree4(self.h, _p(b), _p(k))
        return b[:n], k[:n]

    def free_grid(self):
        """(k [nz][ny][nx] uint8, g0 (3,), inv_h, h_free) of the empty-space grid, or None."""
        n = np.zeros(3, np.int32)
        cells = lib().rrt_get_free_grid(self.h, None, None, _p(n))
        if cells < 0:
            raise RRTError(cells, "no scene")
        if cells == 0:
            return None
        k = np.zeros((n[2], n[1], n[0]), np.uint8)
        geom = np.zeros(5, np.float64)
        self._chk(0 if lib().rrt_get_free_grid(self.h, _p(k), _p(geom), _p(n)) > 0 else RRT_E_INVALID)
        return k, geom[:3].copy(), float(geom[3]), float(geom[4])

    def big_masks(self):
        """(mask [nz][ny][nx] uint32 over the free grid's cells, reach) of the oversized-leaf masks, or None."""
        cells = lib().rrt_get_big_masks(self.h, None, None)
        if cells < 0:
            raise RRTError(cells, "no scene")
        if cells == 0:
            return None
        g = self.free_grid()
        m = np.zeros(g[0].shape, np.uint32)
        reach = np.zeros(1, np.float64)
        lib().rrt_get_big_masks(self.h, _p(m), _p(reach))
        return m, float(reach[0])

    def occluders(self):
        """(tris [6][4][16] = plane n (3), d, in-plane edge normals en [3][3], offsets eo [3];
        counts [6]) of the shadow-ray occlusion proof's root-box face triangles (include/rrt.h
        rrt_get_occluders)."""
        tris = np.zeros((6, 4, 16), np.float64)
        counts = np.zeros(6, np.uint32)
        n = lib().rrt_get_occluders(self.h, _p(tris), _p(counts))
        if n < 0:
            raise RRTError(n, "no scene")
        return tris, counts

    def clean_tree(self):
        """(boxes [n,6], nodes [n,4] (skip, first, count, ordinal), big_boxes [nb,6], big [nb,3]
        (first, count, ordinal)) of the clean tree, or None."""
        s = self.stats()
        if s.n_clean == 0:
            return None
        boxes = np.zeros((s.n_clean, 6), np.float64)
        nodes = np.zeros((s.n_clean, 4), np.int32)
        bb = np.zeros((max(s.n_big, 1), 6), np.float64)
        big = np.zeros((max(s.n_big, 1), 3), np.int32)
        self._chk(0 if lib().rrt_get_clean_tree(self.h, _p(boxes), _p(nodes), _p(bb), _p(big)) > 0 else RRT_E_INVALID)
        return boxes, nodes, bb[:s.n_big], big[:s.n_big]

    def proof_envelope(self):
        """True if the scene and hole lie in the proofs' validated envelope (rrt_proof_envelope)."""
        return lib().rrt_proof_envelope(self.h) == 1

    def search_tree(self):
        """(boxes [n,6], nodes [n,4] (skip, first, count, ordinal)) of the search tree, or None."""
        n = lib().rrt_get_search_tree(self.h, None, None)
        if n <= 0:
            return None
        boxes = np.zeros((n, 6), np.float64)
        nodes = np.zeros((n, 4), np.int32)
        lib().rrt_get_search_tree(self.h, _p(boxes), _p(nodes))
        return boxes, nodes

    def bvh(self):
        s = self.stats()
        boxes = np.zeros((s.n_nodes, 6), np.float64)
        nodes = np.zeros((s.n_nodes, 4), np.int32)
        prims = np.zeros(s.n_leaf_refs, np.uint32)
        self._chk(lib().rrt_get_bvh(self.h, _p(boxes), _p(nodes), _p(prims)))
        return boxes, nodes, prims
