"""Workload for the denoiser's timing profile (profiles/r06_denoise.txt): scene.xml at 1920x1080 and 1280x720, a 4-spp render,
then REPS x (guide pass + N = 5 filter levels) — the camera alternates between two positions so that every repetition traces the
guides again.  Run under `rocprofv3 --kernel-trace --stats`; tools/denoise_prof.py turns the kernel trace into per-kernel times."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metalpathtracer_amd import capi, host  # noqa: E402

REPS = 20


def main():
    sc = host.Scene()
    st, log = host.SceneLoader.LoadSceneFromXML(os.path.join(ROOT, "assets", "scene.xml"), sc)
    assert st == 0, log
    sc.buildBVH()
    buf = sc.buffers()
    ctx = capi.Context(0)
    ctx.upload_scene(*buf)
    for W, H in ((1920, 1080), (1280, 720)):
        ctx.resize(W, H)
        cams = []
        for dx in (0.0, 0.5):
            cam = host.camera_reset()
            cam["pos"] = (cam["pos"][0] + dx, cam["pos"][1], cam["pos"][2])
            cams.append(host.make_uniforms(W, H, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=cam))
        ctx.set_uniforms(cams[0])
        ctx.render(sample_count=4, max_depth=8)
        for r in range(REPS):
            ctx.set_uniforms(cams[r & 1])
            ctx.denoise(source=capi.DENOISE_SUM, samples=4, iterations=5)
        ctx.synchronize()
        print("done %dx%d" % (W, H))
    ctx.close()


if __name__ == "__main__":
    main()
