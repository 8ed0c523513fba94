"""Shaded ray batches, milliseconds per call: vx_trace_rays over the C3 view's 1920 x 1080 camera rays, handed over as a device batch, beside
vx_render of the same view.

    python profiles/trace_rays_bench.py [--out profiles/trace_rays/results.json] [--formats esvo,csvo]

On the depth-12 bench world with the bench camera (shadows on, shadow distance 500), per node format:
  trace_rgba32f_ms, trace_rgba8_ms   vx_trace_rays(VX_MEM_DEVICE), colours only, the 2,073,600 rays as packed [N,3] device arrays
  trace_rgba32f_hits_ms              the same with vx_hit records as well
  render_default_ms                  vx_render into device memory, RGBA32F, the default (persistent, traversal image) kernel
  render_per_pixel_ms                the same in a context created with VX_RENDER_KERNEL=1: the one-thread-per-pixel kernel on the world's own
                                     bytes -- the path vx_trace_rays' kernel shares
Every figure is the host clock around a queue of calls that ends in vx_sync, divided by the calls: 5 rounds after a warm-up round, the median
with the smallest and largest round beside it. The rays are primary_ray's arithmetic restated in float32 NumPy; `records_identical` says how
many of the batch's vx_hit records are byte for byte those of vx_render(want_hits) of the view (a check that the two did the same work, not a
test). Each (format, kernel) runs in a child process of its own under `timeout`; the driver stops at the first that fails."""
import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
W, H = 1920, 1080
ROUNDS = 5


def camera_rays(u, np):
    """world.glsl:110-129 for every pixel, in primary_ray's order of operations (an affine view: no perspective divide); index y * W + x."""
    f = np.float32
    m = np.array(list(u.view), dtype=f)
    t = f(np.tan(f(u.fovy) * f(0.5)))
    x, y = np.meshgrid(np.arange(W, dtype=f), np.arange(H, dtype=f))
    uvx = (x / f(W)) * f(2) - f(1)
    uvy = (y / f(H)) * f(2) - f(1)
    uvx = uvx * f(u.aspect) * t
    uvy = uvy * t
    ro = np.array([m[12], m[13], m[14]], dtype=f)
    d = np.stack([(m[r] * uvx + m[4 + r] * uvy + m[8 + r] * f(-1) + m[12 + r] * f(1)) - ro[r] for r in range(3)], axis=-1).astype(f)
    length = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]).astype(f)).astype(f)
    d = (d / length[..., None]).astype(f)
    return np.ascontiguousarray(np.broadcast_to(ro, (W * H, 3))), np.ascontiguousarray(d.reshape(-1, 3))


def case(fmt, kernel):
    sys.path.insert(0, str(ROOT))
    import numpy as np
    import torch

    from _pkg import load_package

    vra = load_package()
    from voxel_rs_amd import hip, scenes

    svo_type = vra.SVO_ESVO if fmt == "esvo" else vra.SVO_CSVO
    world = vra.World(svo_type)
    st = world.build_heightfield(12)
    svo = hip.Svo(svo_type, world.size_in_bytes + (4 << 20))
    svo.set_materials(scenes.synthetic_materials())
    svo.set_textures(scenes.synthetic_textures(), 6)
    svo.update(world)
    u = scenes.bench_camera(12, st["h_max"], W, H)
    n = W * H

    def timed(fn, calls):
        per_call = []
        for _ in range(ROUNDS + 1):
            svo.sync()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            svo.sync()
            per_call.append((time.perf_counter() - t0) * 1e3 / calls)
        v = per_call[1:]
        return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4), "calls_per_round": calls}

    frame = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    out = {"format": fmt, "rays": n}
    key = "render_per_pixel_ms" if kernel == 1 else "render_default_ms"
    out[key] = timed(lambda: svo.render_device(u, W, H, frame.data_ptr()), 50 if kernel == 2 else 10)
    if kernel == 2:
        o, d = camera_rays(u, np)
        d_o, d_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
        rgba = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        rgba8 = torch.empty((n, 4), dtype=torch.uint8, device="cuda")
        hits = torch.empty((n, 12), dtype=torch.int32, device="cuda")
        # the same work? records of the batch against those of the view
        svo.trace_rays(u, d_o, d_d, want_hits=True, out=(rgba, hits))
        svo.sync()
        _, rhits = svo.render(u, W, H, want_hits=True)
        got = hip.trace_hits_to_numpy(hits)
        same = (got.view(np.uint8).reshape(n, 48) == rhits.reshape(-1).view(np.uint8).reshape(n, 48)).all(axis=1)
        out["records_identical"] = int(same.sum())
        out["primary_hits"] = int((got["flags"] & 1).sum())
        out["shadow_rays"] = int(((got["flags"] >> 1) & 1).sum())
        out["loop_iterations"] = int(got["steps"].sum())
        out["trace_rgba32f_ms"] = timed(lambda: svo.trace_rays(u, d_o, d_d, out=(rgba, None)), 5)
        out["trace_rgba8_ms"] = timed(lambda: svo.trace_rays(u, d_o, d_d, fmt=hip.VX_FORMAT_RGBA8, out=(rgba8, None)), 5)
        out["trace_rgba32f_hits_ms"] = timed(lambda: svo.trace_rays(u, d_o, d_d, want_hits=True, out=(rgba, hits)), 5)
    print(json.dumps(out), flush=True)
    svo.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", metavar="FORMAT")
    ap.add_argument("--kernel", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "trace_rays" / "results.json"))
    ap.add_argument("--formats", default="esvo,csvo")
    ap.add_argument("--timeout", type=int, default=240)
    args = ap.parse_args()
    if args.case:
        case(args.case, args.kernel)
        return 0
    results = {}
    for fmt in args.formats.split(","):
        for kernel in (2, 1):
            env = dict(os.environ, VX_RENDER_KERNEL=str(kernel))
            r = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, __file__, "--case", fmt, "--kernel", str(kernel)], stdout=subprocess.PIPE,
                               text=True, env=env)
            if r.returncode != 0:
                print(f"format {fmt}, kernel {kernel} ended with status {r.returncode}: stopping", file=sys.stderr)
                return r.returncode
            line = r.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            results.setdefault(fmt, {}).update(json.loads(line))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": "MI355X (gfx950)", "scene": f"heightfield depth 12, bench camera, {W}x{H}, shadows on", "unit": "milliseconds per call",
                                          "method": f"host clock around a queue of calls ending in vx_sync; median of {ROUNDS} rounds after one warm-up round",
                                          "cases": list(results.values())}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
