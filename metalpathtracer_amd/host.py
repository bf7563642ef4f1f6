"""Python mirror of the host layer (include/mpt_host.h, libmpt_host.so).

Class and method names follow the reference's C++ interface (R/Scene/Scene.h, R/Scene/SceneLoader.h,
R/Renderer/Renderer.h, R/Renderer/Camera.h) so the tests read like code written against the reference.
All work happens in the C++ library; nothing here computes.
"""
import ctypes as C
import os

import numpy as np

from . import capi

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libmpt_host.so")

BVH_REFERENCE_SWEEP, BVH_BINNED_CENTROID, BVH_GPU_LBVH = 0, 1, 2

SYMBOLS = (
    "mpt_scene_create", "mpt_scene_destroy", "mpt_scene_clear", "mpt_scene_load_xml", "mpt_scene_add_primitive",
    "mpt_scene_build_bvh", "mpt_scene_sort_primitives", "mpt_scene_counts", "mpt_scene_copy_buffers", "mpt_camera_reset_values",
    "mpt_camera_viewport", "mpt_host_random_float", "mpt_renderer_create", "mpt_renderer_destroy",
    "mpt_renderer_drawable_size_will_change", "mpt_renderer_set_params", "mpt_renderer_draw", "mpt_renderer_input",
    "mpt_renderer_read_frame", "mpt_renderer_render_batch", "mpt_renderer_read_sum", "mpt_renderer_clear_sum",
    "mpt_renderer_uniforms", "mpt_renderer_stats", "mpt_renderer_context", "mpt_renderer_scene", "mpt_write_pfm",
    "mpt_write_ppm", "mpt_renderer_denoise", "mpt_renderer_render_adaptive",
    "mpt_renderer_draw_temporal", "mpt_renderer_read_temporal", "mpt_renderer_denoise_temporal",
    "mpt_renderer_draw_svgf", "mpt_renderer_read_svgf", "mpt_renderer_display", "mpt_write_ppm8",
    "mpt_renderer_ambient_occlusion", "mpt_renderer_direct_lighting", "mpt_renderer_direct_restir", "mpt_renderer_direct_restir_temporal", "mpt_renderer_render_nee", "mpt_renderer_set_light_sampling",
    "mpt_renderer_render_nee_adaptive", "mpt_renderer_set_light_candidates", "mpt_renderer_get_light_candidates",
)

_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libmpt_host.so is not built (%s). Run `make` or __graft_entry__.build()." % LIB_PATH)
    capi.load()  # libmpt_host.so links libmpt_hip.so
    L = C.CDLL(LIB_PATH)
    vp, fp, ip = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32)
    L.mpt_scene_create.argtypes = [C.POINTER(vp)]
    L.mpt_scene_destroy.argtypes = [vp]
    L.mpt_scene_clear.argtypes = [vp]
    L.mpt_scene_load_xml.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]
    L.mpt_scene_add_primitive.argtypes = [vp, C.c_int, fp, fp, fp, fp]
    L.mpt_scene_build_bvh.argtypes = [vp, C.c_int]
    L.mpt_scene_sort_primitives.argtypes = [vp]
    L.mpt_scene_counts.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                   C.POINTER(C.c_int32)]
    L.mpt_scene_copy_buffers.argtypes = [vp, fp, fp, fp, ip]
    L.mpt_camera_reset_values.argtypes = [fp, fp, fp, fp]
    L.mpt_camera_viewport.argtypes = [fp, fp, fp, C.c_float, C.c_float, C.c_float, C.POINTER(capi.Uniforms)]
    L.mpt_host_random_float.argtypes = [C.POINTER(C.c_uint32)]
    L.mpt_host_random_float.restype = C.c_float
    L.mpt_renderer_create.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.POINTER(vp), C.c_char_p, C.c_size_t]
    L.mpt_renderer_destroy.argtypes = [vp]
    L.mpt_renderer_drawable_size_will_change.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.mpt_renderer_set_params.argtypes = [vp, C.POINTER(capi.RenderParams)]
    L.mpt_renderer_draw.argtypes = [vp]
    L.mpt_renderer_input.argtypes = [vp, fp, fp, C.c_float, C.c_int]
    L.mpt_renderer_read_frame.argtypes = [vp, fp]
    L.mpt_renderer_render_batch.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.mpt_renderer_read_sum.argtypes = [vp, fp]
    L.mpt_renderer_clear_sum.argtypes = [vp]
    L.mpt_renderer_uniforms.argtypes = [vp, C.POINTER(capi.Uniforms)]
    L.mpt_renderer_stats.argtypes = [vp, C.POINTER(capi.Stats)]
    L.mpt_renderer_denoise.argtypes = [vp, C.POINTER(capi.DenoiseParams), fp]
    L.mpt_renderer_render_adaptive.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(capi.AdaptiveParams),
                                               C.POINTER(capi.AdaptiveInfo)]
    L.mpt_renderer_draw_temporal.argtypes = [vp, C.c_uint32, C.POINTER(capi.TemporalParams), C.POINTER(capi.TemporalInfo)]
    L.mpt_renderer_read_temporal.argtypes = [vp, fp]
    L.mpt_renderer_denoise_temporal.argtypes = [vp, C.POINTER(capi.DenoiseParams), fp]
    L.mpt_renderer_draw_svgf.argtypes = [vp, C.c_uint32, C.POINTER(capi.SvgfParams), C.POINTER(capi.SvgfInfo)]
    L.mpt_renderer_read_svgf.argtypes = [vp, fp]
    L.mpt_renderer_context.argtypes = [vp]
    L.mpt_renderer_context.restype = vp
    L.mpt_renderer_scene.argtypes = [vp]
    L.mpt_renderer_scene.restype = vp
    L.mpt_write_pfm.argtypes = [C.c_char_p, fp, C.c_uint32, C.c_uint32, C.c_float]
    L.mpt_write_ppm.argtypes = [C.c_char_p, fp, C.c_uint32, C.c_uint32, C.c_float, C.c_float]
    L.mpt_renderer_display.argtypes = [vp, C.POINTER(capi.DisplayParams), C.POINTER(C.c_uint8), C.POINTER(capi.DisplayInfo)]
    L.mpt_write_ppm8.argtypes = [C.c_char_p, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32]
    L.mpt_renderer_ambient_occlusion.argtypes = [vp, C.c_uint32, C.c_float, C.POINTER(C.c_float), C.POINTER(capi.AoInfo)]
    L.mpt_renderer_direct_lighting.argtypes = [vp, C.c_uint32, C.c_int32, C.POINTER(C.c_float), C.POINTER(capi.DirectInfo)]
    L.mpt_renderer_direct_restir.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.POINTER(C.c_float),
                                             C.POINTER(capi.RestirInfo)]
    L.mpt_renderer_direct_restir_temporal.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.POINTER(C.c_float),
                                                      C.POINTER(capi.RestirTemporalInfo)]
    L.mpt_renderer_render_nee.argtypes = [vp, C.c_uint32, C.c_int32, C.c_int32, C.c_float, C.POINTER(capi.NeeInfo)]
    L.mpt_renderer_set_light_sampling.argtypes = [vp, C.c_int32]
    L.mpt_renderer_set_light_candidates.argtypes = [vp, C.c_uint32]
    L.mpt_renderer_get_light_candidates.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.mpt_renderer_render_nee_adaptive.argtypes = [vp, C.c_uint32, C.c_int32, C.c_int32, C.c_float, C.POINTER(capi.AdaptiveParams),
                                                   C.POINTER(capi.AdaptiveInfo), C.POINTER(capi.NeeInfo)]
    _lib = L
    return L


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


class Scene:
    """class Scene (R/Scene/Scene.h:34-188)."""

    def __init__(self, _borrowed=None):
        self.L = load()
        self._owned = _borrowed is None
        if self._owned:
            self.h = C.c_void_p()
            self.L.mpt_scene_create(C.byref(self.h))
        else:
            self.h = C.c_void_p(_borrowed)

    def __del__(self):
        try:
            if self._owned and self.h:
                self.L.mpt_scene_destroy(self.h)
        except Exception:
            pass

    def clear(self):
        self.L.mpt_scene_clear(self.h)

    def addPrimitive(self, type_, d0, d1, d2, albedo=(0.8, 0.8, 0.8), materialType=0.0, emission=(0, 0, 0),
                     emissionPower=0.0):
        mat = (C.c_float * 8)(*albedo, materialType, *emission, emissionPower)
        rc = self.L.mpt_scene_add_primitive(self.h, int(type_), _f3(d0), _f3(d1), _f3(d2), mat)
        if rc:
            raise ValueError("mpt_scene_add_primitive: %d" % rc)

    def addSphere(self, center, radius, **kw):
        self.addPrimitive(0, center, (radius, 0, 0), (0, 0, 0), **kw)

    def addTriangle(self, v0, v1, v2, **kw):
        self.addPrimitive(1, v0, v1, v2, **kw)

    def buildBVH(self, mode=BVH_REFERENCE_SWEEP):
        rc = self.L.mpt_scene_build_bvh(self.h, int(mode))
        if rc:
            raise ValueError("mpt_scene_build_bvh: %d" % rc)

    def sortPrimitives(self):
        """Scene::sortPrimitives: spheres first, stable — all that mpt_build_and_upload needs of buildBVH."""
        rc = self.L.mpt_scene_sort_primitives(self.h)
        if rc:
            raise ValueError("mpt_scene_sort_primitives: %d" % rc)

    def _counts(self):
        p, t, n, d = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int32()
        self.L.mpt_scene_counts(self.h, C.byref(p), C.byref(t), C.byref(n), C.byref(d))
        return p.value, t.value, n.value, d.value

    def getPrimitiveCount(self):
        return self._counts()[0]

    def getTriangleCount(self):
        return self._counts()[1]

    def getSphereCount(self):
        c = self._counts()
        return c[0] - c[1]

    def getBVHNodeCount(self):
        return self._counts()[2]

    def getBVHDepth(self):
        return self._counts()[3]

    def packed_primitives(self):
        """(prims [P,3,4], mats [P,2,4]) without a tree: what mpt_build_and_upload takes (createTransformsBuffer /
        createMaterialsBuffer, R/Scene/Scene.h:99-133)."""
        P = self._counts()[0]
        prims = np.zeros((P, 3, 4), np.float32)
        mats = np.zeros((P, 2, 4), np.float32)
        self.L.mpt_scene_copy_buffers(self.h, None, _fp(prims), _fp(mats), None)
        return prims, mats

    def buffers(self):
        """(bvh [N,2,4], prims [P,3,4], mats [P,2,4], prim_idx [P]) — createBVHBuffer / createTransformsBuffer /
        createMaterialsBuffer / createPrimitiveIndexBuffer (R/Scene/Scene.h:99-167)."""
        P, _, N, _ = self._counts()
        bvh = np.zeros((N, 2, 4), np.float32)
        prims = np.zeros((P, 3, 4), np.float32)
        mats = np.zeros((P, 2, 4), np.float32)
        idx = np.zeros((P,), np.int32)
        self.L.mpt_scene_copy_buffers(self.h, _fp(bvh), _fp(prims), _fp(mats), idx.ctypes.data_as(C.POINTER(C.c_int32)))
        return bvh, prims, mats, idx


class SceneLoader:
    """SceneLoader::LoadSceneFromXML (R/Scene/SceneLoader.h:11)."""

    @staticmethod
    def LoadSceneFromXML(path, scene, asset_root=None):
        log = C.create_string_buffer(1 << 16)
        st = load().mpt_scene_load_xml(scene.h, path.encode(), asset_root.encode() if asset_root else None, log,
                                       len(log))
        return st, log.value.decode(errors="replace")


BVH_DEVICE = 3   # make_ready only: build -> render on the device (mpt_build_and_upload); 0..2 are Scene::buildBVH's modes


def make_ready(ctx, scene, bvh=BVH_REFERENCE_SWEEP):
    """The scene ready to render on `ctx` with the tree builder `bvh`: Scene::buildBVH + mpt_upload_scene for the host
    builders (0 reference sweep, 1 binned SAH, 2 GPU tree copied through the host), mpt_build_and_upload for BVH_DEVICE.
    Returns the (bvh, prims, mats, prim_idx) arrays in the reference's buffer format — for BVH_DEVICE the tree comes back
    from the device (mpt_download_bvh): what the oracle walks to render the same image."""
    if bvh == BVH_DEVICE:
        scene.sortPrimitives()                       # spheres first, as every builder does; no host tree is built
        prims, mats = scene.packed_primitives()
        ctx.build_and_upload(prims, mats)
        tree, idx = ctx.download_bvh()
        return tree, prims, mats, idx
    scene.buildBVH(bvh)
    buffers = scene.buffers()
    ctx.upload_scene(*buffers)
    return buffers


def camera_reset():
    """Camera::reset() (R/Renderer/Camera.h:24-32)."""
    pos, fwd, up = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 3)()
    fov = C.c_float()
    load().mpt_camera_reset_values(pos, fwd, up, C.byref(fov))
    return dict(pos=tuple(pos), fwd=tuple(fwd), up=tuple(up), vfov=fov.value)


def make_uniforms(W, H, prim_count, tri_count=0, cam=None, random_seed=(0.0, 0.0, 0.0), frame_count=1):
    """Uniforms as Renderer::recalculateViewport + updateUniforms fill them (R/Renderer/Renderer.cpp:153-182,251-267)."""
    cam = cam or camera_reset()
    u = capi.Uniforms()
    rc = load().mpt_camera_viewport(_f3(cam["pos"]), _f3(cam["fwd"]), _f3(cam["up"]), float(cam["vfov"]), float(W),
                                    float(H), C.byref(u))
    if rc:
        raise ValueError("mpt_camera_viewport: %d" % rc)
    for i in range(3):
        u.randomSeed[i] = float(random_seed[i])
    u.primitiveCount = prim_count
    u.triangleCount = tri_count
    u.frameCount = frame_count
    return u


def host_seed_sequence(n=3, state=92407235):
    st = C.c_uint32(state)
    return [float(load().mpt_host_random_float(C.byref(st))) for _ in range(n)]


class Renderer:
    """class Renderer (R/Renderer/Renderer.h:16-29) over an offscreen target."""

    def __init__(self, device=0, scene_xml=None, asset_root=None):
        self.L = load()
        self.h = C.c_void_p()
        err = C.create_string_buffer(1024)
        rc = self.L.mpt_renderer_create(int(device), scene_xml.encode() if scene_xml else None,
                                        asset_root.encode() if asset_root else None, C.byref(self.h), err, len(err))
        if rc:
            raise capi.MptError(rc, "Renderer", err.value.decode(errors="replace"))
        self.width, self.height = 1280, 720  # R/Renderer/Renderer.cpp:49

    def close(self):
        if getattr(self, "h", None):
            self.L.mpt_renderer_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, where):
        if rc:
            raise capi.MptError(rc, where)

    def drawableSizeWillChange(self, width, height):
        self._chk(self.L.mpt_renderer_drawable_size_will_change(self.h, int(width), int(height)),
                  "drawableSizeWillChange")
        self.width, self.height = int(width), int(height)

    def setRenderParams(self, **kw):
        p = capi.Context.params(**kw)
        self._chk(self.L.mpt_renderer_set_params(self.h, C.byref(p)), "setRenderParams")

    def draw(self):
        self._chk(self.L.mpt_renderer_draw(self.h), "draw")

    def input(self, move=(0, 0, 0), rotate=(0, 0), zoom=0.0, reset=False):
        """InputSystem state for the next draw (movementInput, rotationInput, zoomInput, resetInput)."""
        self._chk(self.L.mpt_renderer_input(self.h, _f3(move), (C.c_float * 2)(*[float(x) for x in rotate]), float(zoom),
                                            int(bool(reset))), "input")

    def readFrame(self):
        out = np.empty((self.height, self.width, 4), np.float32)
        self._chk(self.L.mpt_renderer_read_frame(self.h, _fp(out)), "readFrame")
        return out

    def renderBatch(self, sample_begin, sample_count):
        self._chk(self.L.mpt_renderer_render_batch(self.h, int(sample_begin), int(sample_count)), "renderBatch")

    def renderAdaptive(self, sample_begin, max_samples, threshold, min_samples=0, batch_samples=0, luminance_floor=0.0):
        """mpt_renderer_render_adaptive: the mpt_adaptive_info as a dict (counts per tile: capi's read_tile_samples on context())."""
        a = capi.AdaptiveParams(int(min_samples), int(batch_samples), float(threshold), float(luminance_floor))
        info = capi.AdaptiveInfo()
        self._chk(self.L.mpt_renderer_render_adaptive(self.h, int(sample_begin), int(max_samples), C.byref(a), C.byref(info)),
                  "renderAdaptive")
        return info.as_dict()

    def readTileSamples(self):
        """Samples per 8x8 tile of the last renderAdaptive: (tiles_y, tiles_x) uint32 (mpt_read_tile_samples on the context)."""
        out = np.empty(((self.height + 7) // 8, (self.width + 7) // 8), np.uint32)
        ctx = self.L.mpt_renderer_context(self.h)
        self._chk(capi.load().mpt_read_tile_samples(ctx, out.ctypes.data_as(C.POINTER(C.c_uint32))), "readTileSamples")
        return out

    def readSum(self):
        out = np.empty((self.height, self.width, 4), np.float32)
        self._chk(self.L.mpt_renderer_read_sum(self.h, _fp(out)), "readSum")
        return out

    def clearSum(self):
        self._chk(self.L.mpt_renderer_clear_sum(self.h), "clearSum")

    def uniforms(self):
        u = capi.Uniforms()
        self._chk(self.L.mpt_renderer_uniforms(self.h, C.byref(u)), "uniforms")
        return u

    def stats(self):
        s = capi.Stats()
        self._chk(self.L.mpt_renderer_stats(self.h, C.byref(s)), "stats")
        return s.as_dict()

    def denoise(self, **kw):
        """mpt_renderer_denoise: the draw() target after draw(), the sum after renderBatch() (samples=0: all rendered since the
        last clearSum()); the denoised [H, W, 4] image."""
        u = self.uniforms()
        out = np.empty((int(u.screenSize[1]), int(u.screenSize[0]), 4), np.float32)
        p = capi.denoise_params(**kw)
        self._chk(self.L.mpt_renderer_denoise(self.h, C.byref(p), _fp(out)), "denoise")
        return out

    def drawTemporal(self, samples_per_frame=1, **kw):
        """mpt_renderer_draw_temporal: one frame of temporal accumulation with the pending input(); kw: max_history, depth_tolerance,
        normal_threshold, min_weight (none: keep the renderer's).  Returns the mpt_temporal_info as a dict."""
        p = capi.temporal_params(**kw) if kw else None
        info = capi.TemporalInfo()
        self._chk(self.L.mpt_renderer_draw_temporal(self.h, int(samples_per_frame), C.byref(p) if p is not None else None,
                                                    C.byref(info)), "drawTemporal")
        return info.as_dict()

    def readTemporal(self):
        u = self.uniforms()
        out = np.empty((int(u.screenSize[1]), int(u.screenSize[0]), 4), np.float32)
        self._chk(self.L.mpt_renderer_read_temporal(self.h, _fp(out)), "readTemporal")
        return out

    def denoiseTemporal(self, **kw):
        """mpt_renderer_denoise_temporal: the a-trous filter over the history with the current guides; the [H, W, 4] image."""
        u = self.uniforms()
        out = np.empty((int(u.screenSize[1]), int(u.screenSize[0]), 4), np.float32)
        p = capi.denoise_params(**kw)
        self._chk(self.L.mpt_renderer_denoise_temporal(self.h, C.byref(p), _fp(out)), "denoiseTemporal")
        return out

    def drawSvgf(self, samples_per_frame=1, **kw):
        """mpt_renderer_draw_svgf: one frame of SVGF with the pending input(); kw: the fields of mpt_svgf_params but source / samples
        (none: keep the renderer's).  Returns the mpt_svgf_info as a dict; readSvgf() has the frame."""
        p = capi.svgf_params(**kw) if kw else None
        info = capi.SvgfInfo()
        self._chk(self.L.mpt_renderer_draw_svgf(self.h, int(samples_per_frame), C.byref(p) if p is not None else None, C.byref(info)),
                  "drawSvgf")
        return info.as_dict()

    def readSvgf(self):
        u = self.uniforms()
        out = np.empty((int(u.screenSize[1]), int(u.screenSize[0]), 4), np.float32)
        self._chk(self.L.mpt_renderer_read_svgf(self.h, _fp(out)), "readSvgf")
        return out

    def display(self, **kw):
        """mpt_renderer_display: mpt_display + mpt_read_display of `source` (DISPLAY_SUM with samples=0: all rendered since the last
        clearSum()).  Returns (bytes [H, W, 4] uint8, the mpt_display_info as a dict)."""
        u = self.uniforms()
        out = np.empty((int(u.screenSize[1]), int(u.screenSize[0]), 4), np.uint8)
        p = capi.display_params(**kw)
        info = capi.DisplayInfo()
        self._chk(self.L.mpt_renderer_display(self.h, C.byref(p), out.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(info)), "display")
        return out, info.as_dict()

    def renderAmbientOcclusion(self, samples, radius=0.0):
        """mpt_renderer_ambient_occlusion: `samples` shadow rays per surface pixel of the current camera's first hits, no farther than
        `radius` (<= 0: no limit).  Returns (ao [H, W] float32, 1 = open; the mpt_ao_info as a dict)."""
        u = self.uniforms()
        out = np.empty((int(u.screenSize[1]), int(u.screenSize[0])), np.float32)
        info = capi.AoInfo()
        self._chk(self.L.mpt_renderer_ambient_occlusion(self.h, int(samples), float(radius), _fp(out), C.byref(info)), "renderAmbientOcclusion")
        return out, info.as_dict()

    def renderDirectLighting(self, samples, walk=capi.WALK_AUTO):
        """mpt_renderer_direct_lighting: `samples` light samples per surface pixel of the current camera's first hits, one shadow ray
        each.  Returns (rgba [H, W, 4] float32: the direct lighting of a Lambert surface, emitters black; the mpt_direct_info as a dict)."""
        u = self.uniforms()
        out = np.empty((int(u.screenSize[1]), int(u.screenSize[0]), 4), np.float32)
        info = capi.DirectInfo()
        self._chk(self.L.mpt_renderer_direct_lighting(self.h, int(samples), int(walk), _fp(out), C.byref(info)), "renderDirectLighting")
        return out, info.as_dict()

    def renderDirectRestir(self, samples, neighbours, radius=0, mode=capi.RESTIR_UNBIASED, walk=capi.WALK_AUTO):
        """mpt_renderer_direct_restir: renderDirectLighting with spatial reservoir reuse — every round merges a pixel's reservoir with
        `neighbours` from within `radius` pixels (0: the default).  Returns (rgba [H, W, 4] float32; the mpt_restir_info as a dict)."""
        u = self.uniforms()
        out = np.empty((int(u.screenSize[1]), int(u.screenSize[0]), 4), np.float32)
        info = capi.RestirInfo()
        self._chk(self.L.mpt_renderer_direct_restir(self.h, int(samples), int(neighbours), int(radius), int(mode), int(walk), _fp(out),
                                                    C.byref(info)), "renderDirectRestir")
        return out, info.as_dict()

    def drawDirectRestirTemporal(self, frame, max_history=0, mode=capi.RESTIR_UNBIASED, walk=capi.WALK_AUTO):
        """mpt_renderer_direct_restir_temporal: frame number `frame` of a camera path with the pending input() — one round of the direct
        pass whose reservoirs are merged with the previous frame's, which count for at most `max_history` frames' candidates (0: the
        default).  Returns (rgba [H, W, 4] float32; the mpt_restir_temporal_info as a dict)."""
        u = self.uniforms()
        out = np.empty((int(u.screenSize[1]), int(u.screenSize[0]), 4), np.float32)
        info = capi.RestirTemporalInfo()
        self._chk(self.L.mpt_renderer_direct_restir_temporal(self.h, int(frame), int(max_history), int(mode), int(walk), _fp(out), C.byref(info)),
                  "drawDirectRestirTemporal")
        return out, info.as_dict()

    def renderNee(self, spp, depth, walk=capi.WALK_AUTO, clamp=0.0):
        """mpt_renderer_render_nee: samples [0, spp) onto the HDR sum (readSum) with a light sample and MIS at every Lambert vertex, at
        max_depth `depth`; clamp <= 0 = no per-sample clamp.  Returns the mpt_nee_info as a dict."""
        info = capi.NeeInfo()
        self._chk(self.L.mpt_renderer_render_nee(self.h, int(spp), int(depth), int(walk), float(clamp), C.byref(info)), "renderNee")
        return info.as_dict()

    def renderNeeAdaptive(self, max_samples, depth, threshold, min_samples=0, batch_samples=0, luminance_floor=0.0, walk=capi.WALK_AUTO,
                          clamp=0.0):
        """mpt_renderer_render_nee_adaptive: renderNee's estimator, at most max_samples per 8x8 tile, every tile stopped on the device by
        renderAdaptive's rule (counts per tile: readTileSamples).  Returns {"adaptive": ..., "nee": ...}, the two infos as dicts."""
        a = capi.AdaptiveParams(int(min_samples), int(batch_samples), float(threshold), float(luminance_floor))
        info, nee = capi.AdaptiveInfo(), capi.NeeInfo()
        self._chk(self.L.mpt_renderer_render_nee_adaptive(self.h, int(max_samples), int(depth), int(walk), float(clamp), C.byref(a),
                                                          C.byref(info), C.byref(nee)), "renderNeeAdaptive")
        return {"adaptive": info.as_dict(), "nee": nee.as_dict()}

    def setLightSampling(self, mode):
        """mpt_renderer_set_light_sampling: capi.LIGHT_SAMPLING_AREA (the default) or capi.LIGHT_SAMPLING_CONE for renderDirectLighting
        and renderNee."""
        self._chk(self.L.mpt_renderer_set_light_sampling(self.h, int(mode)), "setLightSampling")

    def setLightCandidates(self, m):
        """mpt_renderer_set_light_candidates: from how many candidates (1..capi.LIGHT_CANDIDATES_MAX; 1, the default, is no resampling)
        a light sample of renderDirectLighting and renderNee is resampled."""
        self._chk(self.L.mpt_renderer_set_light_candidates(self.h, int(m)), "setLightCandidates")

    def lightCandidates(self):
        m = C.c_uint32(0)
        self._chk(self.L.mpt_renderer_get_light_candidates(self.h, C.byref(m)), "lightCandidates")
        return m.value

    def scene(self):
        return Scene(_borrowed=self.L.mpt_renderer_scene(self.h))


def write_pfm(path, rgba, scale=1.0):
    a = np.ascontiguousarray(rgba, np.float32)
    return load().mpt_write_pfm(path.encode(), _fp(a), a.shape[1], a.shape[0], float(scale))


def write_ppm(path, rgba, scale=1.0, gamma=2.2):
    a = np.ascontiguousarray(rgba, np.float32)
    return load().mpt_write_ppm(path.encode(), _fp(a), a.shape[1], a.shape[0], float(scale), float(gamma))


def write_ppm8(path, rgba8):
    """mpt_write_ppm8: the r, g, b of finished bytes [H, W, 4] uint8 (Context.read_display) as a binary PPM; no arithmetic."""
    a = np.ascontiguousarray(rgba8, np.uint8)
    return load().mpt_write_ppm8(path.encode(), a.ctypes.data_as(C.POINTER(C.c_uint8)), a.shape[1], a.shape[0])
