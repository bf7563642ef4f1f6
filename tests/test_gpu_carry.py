"""Carried hits of the wave-local kernel (wavelocal_body, mpt_kernels.h): when the step after a step is going to pop ring 0, the hits
just found stay in their lanes instead of being pushed and popped.  The schedule, the counts and every result bit must be what they
are without the carry, so the wave-local pipeline (2) is compared with the megakernel (1), which has no rings at all: every float of
the HDR sum and the `rays` / `paths` counts must be equal.

Three regimes of the carry rule, by camera:
  ground  every primary ray hits the ground sphere: all 64 lanes of a primary step carry, step after step;
  sky     no primary ray hits anything: nothing is ever carried (and nothing pushed);
  scene   scene.xml's own view: tiles of sky, of ground and of the mesh, partial carries topped up from the ring.
Sizes that are not multiples of the 8x8 tile, spp 1 / 3 / 17, depth 1 / 2 / 8 / 32, a non-zero sample_begin, eight shards, both RNG
modes, the counting instantiation, and three pipelined render_async calls (k_wavelocal_corun) against serial renders."""
import numpy as np
import pytest

from conftest import host_scene

pytestmark = pytest.mark.gpu

# looking straight down at the ground from beside the mesh / straight up from a spot with nothing overhead
# (scene.xml: the ground sphere's top is y = 0, the large sphere spans x, z in [-40, 40], the light [-10, 10])
VIEWS = {
    "ground": dict(pos=(300.0, 60.0, 300.0), fwd=(0.0, -1.0, 0.0), up=(0.0, 0.0, -1.0), vfov=40.0),
    "sky": dict(pos=(300.0, 60.0, 300.0), fwd=(0.0, 1.0, 0.0), up=(0.0, 0.0, -1.0), vfov=40.0),
    "scene": None,
}
SIZES = ((67, 45), (130, 75))
SPPS = (1, 3, 17)
DEPTHS = (1, 2, 8, 32)


def _setup(ctx, view, W, H):
    from metalpathtracer_amd import host
    sc, buf = host_scene("scene.xml")
    ctx.upload_scene(*buf)
    ctx.resize(W, H)
    ctx.set_uniforms(host.make_uniforms(W, H, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=VIEWS[view]))


def _render(ctx, pipeline, shards=1, issue=None, **kw):
    ctx.clear_sum()
    ctx.reset_stats()
    fn = issue or ctx.render
    for r in range(shards):
        fn(pipeline=pipeline, shard_rank=r, shard_count=shards, **kw)
    ctx.wait()
    st = ctx.stats()
    return ctx.read_sum(), st["rays"], st["paths"]


def _same(a, b, what):
    print(what, "rays", a[1], b[1], "paths", a[2], b[2], "floats that differ", int((a[0].view(np.uint32) != b[0].view(np.uint32)).sum()))
    assert (a[1], a[2]) == (b[1], b[2]), what
    np.testing.assert_array_equal(a[0].view(np.uint32), b[0].view(np.uint32), err_msg=str(what))


@pytest.mark.parametrize("rng", ("philox", "literal"))
@pytest.mark.parametrize("view", tuple(VIEWS))
def test_wavelocal_equals_the_megakernel_in_every_regime_of_the_carry(gpu_ctx, view, rng):
    from metalpathtracer_amd import capi
    rng_mode = capi.RNG_PHILOX if rng == "philox" else capi.RNG_LITERAL
    n = 0
    for W, H in SIZES:
        _setup(gpu_ctx, view, W, H)
        for spp in SPPS:
            for depth in DEPTHS:
                n += 1
                kw = dict(rng_mode=rng_mode, max_depth=depth, sample_count=spp, seed=(11, 3),
                          sample_begin=(0, 1000, 37)[n % 3], shards=8 if n % 4 == 1 else 1)
                if n % 5 == 0:
                    kw["flags"] = capi.FLAG_COUNT_WORK      # (the counting instantiation of the kernel)
                mega = _render(gpu_ctx, capi.PIPE_MEGAKERNEL, **kw)
                wave = _render(gpu_ctx, capi.PIPE_WAVELOCAL, **kw)
                _same(wave, mega, (view, rng, W, H, kw))
                assert mega[2] == W * H * spp
                if view == "sky":
                    assert mega[1] == mega[2]               # one ray per path: no primary ray hits
                if view == "ground" and depth >= 2:
                    assert mega[1] >= 2 * mega[2]           # every primary ray hits a diffuse surface and bounces
    assert n == len(SIZES) * len(SPPS) * len(DEPTHS)


@pytest.mark.parametrize("view", tuple(VIEWS))
def test_three_pipelined_renders_equal_serial_ones_and_the_megakernel(gpu_ctx, view):
    from metalpathtracer_amd import capi
    W, H = 483, 271
    _setup(gpu_ctx, view, W, H)

    def three(fn, pipeline):
        gpu_ctx.clear_sum()
        gpu_ctx.reset_stats()
        for k in range(3):
            fn(pipeline=pipeline, rng_mode=capi.RNG_PHILOX, max_depth=8, sample_begin=5 + 6 * k, sample_count=6, seed=(2, 9))
        gpu_ctx.wait()
        st = gpu_ctx.stats()
        return gpu_ctx.read_sum(), st["rays"], st["paths"]

    mega = three(gpu_ctx.render, capi.PIPE_MEGAKERNEL)
    serial = three(gpu_ctx.render, capi.PIPE_WAVELOCAL)
    piped = three(gpu_ctx.render_async, capi.PIPE_WAVELOCAL)
    _same(serial, mega, (view, "serial"))
    _same(piped, mega, (view, "render_async"))
    assert mega[2] == 3 * 6 * W * H


def test_larger_scene_whose_tree_is_not_all_in_lds(gpu_ctx):
    """bunny20.xml: the other product instantiation of k_wavelocal (nodes fetched through L2), deep walks, many parked rays."""
    from metalpathtracer_amd import capi, host
    sc, buf = host_scene("bunny20.xml")
    gpu_ctx.upload_scene(*buf)
    W, H = 93, 61
    gpu_ctx.resize(W, H)
    gpu_ctx.set_uniforms(host.make_uniforms(W, H, sc.getPrimitiveCount(), sc.getTriangleCount()))
    kw = dict(rng_mode=capi.RNG_PHILOX, max_depth=8, sample_count=3, sample_begin=2, seed=(4, 4))
    _same(_render(gpu_ctx, capi.PIPE_WAVELOCAL, **kw), _render(gpu_ctx, capi.PIPE_MEGAKERNEL, **kw), ("bunny20", kw))
    _same(_render(gpu_ctx, capi.PIPE_WAVELOCAL, issue=gpu_ctx.render_async, **kw), _render(gpu_ctx, capi.PIPE_MEGAKERNEL, **kw),
          ("bunny20 render_async", kw))
