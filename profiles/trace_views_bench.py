"""Many small views, milliseconds per batch: one vx_trace_views against N vx_render calls and against one vx_trace_rays over the same rays.

    python profiles/trace_views_bench.py [--out profiles/trace_views/results.json] [--formats esvo,csvo]

On the depth-12 bench world (bench.py's C3 scene), N views of 64 x 64 pixels on a ring around the middle of the terrain, each looking inwards
and down, N = 1 / 16 / 256 / 1024, and one view of 1920 x 1080; RGBA32F pixels in device memory, no records. Per N, each ended by one vx_sync
and timed with the host clock from the first call to the return of the sync:
    trace_views_ms   one vx_trace_views
    render_ms        N vx_render calls into the N images, at the default frames in flight
    trace_rays_ms    one vx_trace_rays over the N * W * H primary rays, generated beforehand and resident in device memory
Medians of 25 repetitions after 5 warm-ups, with the 10th and 90th percentiles beside them; the three are measured in turn, repetition by
repetition, so that a drift of the device's clock meets all three. Each format runs in a child process of its own under `timeout`; the driver
stops at the first that fails."""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CASES = [(1, 64, 64), (16, 64, 64), (256, 64, 64), (1024, 64, 64), (1, 1920, 1080)]
REPS, WARMUP = 25, 5


def ring_views(n, size, h_max, width, height):
    import numpy as np

    from voxel_rs_amd import hip, scenes

    centre = np.float64([0.5 * size, h_max + 0.05 * size, 0.5 * size])
    views = []
    for k in range(n):
        a = 2.0 * np.pi * k / n
        eye = centre + 0.15 * size * np.float64([np.cos(a), 0.0, np.sin(a)])
        fwd = (-np.cos(a), -0.35, -np.sin(a))
        views.append(hip.make_uniforms(scenes.view_matrix(eye, fwd, (0.0, 1.0, 0.0)), np.radians(72.0), width / height, 0.3,
                                       scenes._normalize((-1.0, -1.0, -1.0)), eye, True, 500.0))
    return views


def primary_rays(views, width, height):
    """world.glsl:110-129 for every pixel of every view, in float32 (timing only: the last bit may differ from the library's)."""
    import numpy as np

    x = ((np.arange(width, dtype=np.float32) / np.float32(width)) * 2 - 1)[None, :]
    y = ((np.arange(height, dtype=np.float32) / np.float32(height)) * 2 - 1)[:, None]
    o, d = [], []
    for u in views:
        m = np.float32(list(u.view)).reshape(4, 4)  # m[c] = column c
        t = np.float32(np.tan(np.float32(u.fovy) * np.float32(0.5)))
        ux, uy = x * np.float32(u.aspect) * t, y * t
        look = m[0][None, None, :3] * ux[..., None] + m[1][None, None, :3] * uy[..., None] - m[2][None, None, :3] + m[3][None, None, :3]
        v = look - m[3][None, None, :3]
        v /= np.linalg.norm(v, axis=2, keepdims=True)
        d.append(v.reshape(-1, 3).astype(np.float32))
        o.append(np.broadcast_to(m[3][:3], (width * height, 3)))
    return np.ascontiguousarray(np.concatenate(o), dtype=np.float32), np.ascontiguousarray(np.concatenate(d), dtype=np.float32)


def case(fmt):
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
    L, h = hip.lib(), svo._h
    _vp = hip._vp

    def stats(v):
        v = np.asarray(v) * 1e3
        return {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4), "p90": round(float(np.percentile(v, 90)), 4)}

    for n, w, hgt in CASES:
        views = ring_views(n, float(1 << 12), st["h_max"], w, hgt)
        table = (hip.Uniforms * n)(*views)
        o, d = primary_rays(views, w, hgt)
        d_o, d_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
        batch = hip.RayBatch(d_o.data_ptr(), d_d.data_ptr(), None, 12, 12, 0, -1.0, 0)
        out = torch.zeros((n, hgt, w, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        px = w * hgt * 16
        targets = [hip.Target(out.data_ptr() + k * px, None, hip.VX_MEM_DEVICE, 0, 1, hip.VX_FORMAT_RGBA32F) for k in range(n)]

        def trace_views():
            assert L.vx_trace_views(h, table, n, w, hgt, hip.VX_MEM_DEVICE, _vp(out.data_ptr()), hip.VX_FORMAT_RGBA32F, None) == 0

        def renders():
            for k in range(n):
                assert L.vx_render(h, hip.C.byref(table[k]), w, hgt, hip.C.byref(targets[k])) == 0

        def trace_rays():
            assert L.vx_trace_rays(h, hip.C.byref(table[0]), hip.C.byref(batch), n * w * hgt, hip.VX_MEM_DEVICE, _vp(out.data_ptr()), hip.VX_FORMAT_RGBA32F, None) == 0

        ways = {"trace_views_ms": trace_views, "render_ms": renders, "trace_rays_ms": trace_rays}
        times = {k: [] for k in ways}
        images = {}
        for i in range(REPS + WARMUP):
            for name, fn in ways.items():
                assert L.vx_sync(h) == 0
                t0 = time.perf_counter()
                fn()
                assert L.vx_sync(h) == 0
                t1 = time.perf_counter()
                if i >= WARMUP:
                    times[name].append(t1 - t0)
                if i == 0:
                    images[name] = out.cpu().numpy().copy()
        worst = float(np.abs(images["trace_views_ms"] - images["render_ms"]).max())
        row = {"format": fmt, "views": n, "width": w, "height": hgt, "repeats": REPS, "views_vs_render_max_colour_difference": worst}
        row.update({k: stats(v) for k, v in times.items()})
        row["render_over_trace_views"] = round(row["render_ms"]["median"] / row["trace_views_ms"]["median"], 3)
        print(json.dumps(row), flush=True)
        del out, d_o, d_d
    svo.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", metavar="FORMAT")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "trace_views" / "results.json"))
    ap.add_argument("--formats", default="esvo,csvo")
    ap.add_argument("--timeout", type=int, default=300)
    args = ap.parse_args()
    if args.case:
        case(args.case)
        return 0
    results = []
    for fmt in args.formats.split(","):
        r = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, __file__, "--case", fmt], stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print(f"format {fmt} ended with status {r.returncode}: stopping", file=sys.stderr)
            return r.returncode
        for line in r.stdout.strip().splitlines():
            print(line, flush=True)
            results.append(json.loads(line))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": "MI355X (gfx950)", "scene": "heightfield depth 12", "unit": "milliseconds per batch, one vx_sync included",
                                          "cases": results}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
