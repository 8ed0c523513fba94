"""Plain picker rays, microseconds per call: vx_raycast over vx_picker_task records against vx_raycast_batch.

    python profiles/raycast_batch_bench.py [--out profiles/raycast_batch/results.json] [--formats esvo,csvo]

On the depth-12 bench world, rays of a 256 x 256 look fan from above the terrain (the 1-ray and 80-ray batches are spread over it):
  host arrays, synchronous, the host clock around the call, for 1 / 80 / 65,536 rays:
    raycast_us, raycast_again_us   vx_raycast, measured before and after the batch calls: their difference is the session's spread
    batch_us                       vx_raycast_batch on packed [N,3] arrays
  device tensors, for the same counts and for 4,096 look rays whose origins are the positions inside vx_entity records (stride 64, one
  direction for all):
    device_return_us               the call alone (it returns after enqueueing); vx_sync follows outside the timed region
    device_event_us                HIP-event time per call over a queue of 100 calls on the context's stream
Each format runs in a child process of its own under `timeout`; the driver stops at the first that fails. Medians over at least 200
calls after 20 of warm-up, with the 10th and 90th percentiles beside them."""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
COUNTS = [1, 80, 65536]
REPS, WARMUP = 200, 20


def look_fan(eye, n):
    """n x n unit directions of a 72-degree pinhole looking forward and down from `eye`."""
    import numpy as np

    f = np.float64([0.6, -0.35, 0.7])
    f /= np.linalg.norm(f)
    r = np.cross(f, [0.0, 1.0, 0.0])
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    s = np.tan(np.radians(36.0)) * (2.0 * (np.arange(n) + 0.5) / n - 1.0)
    d = f[None, None, :] + s[None, :, None] * r[None, None, :] + s[:, None, None] * u[None, None, :]
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    return np.ascontiguousarray(d.reshape(-1, 3).astype(np.float32))


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
    size = float(1 << 12)
    eye = np.float32([0.5 * size, st["h_max"] + 0.05 * size, 0.5 * size])
    fan = look_fan(eye, 256)

    def stats(v):
        v = np.asarray(v) * 1e6
        return {"median": round(float(np.median(v)), 2), "p10": round(float(np.percentile(v, 10)), 2), "p90": round(float(np.percentile(v, 90)), 2)}

    def timed(fn, after=None):
        out = []
        for i in range(REPS + WARMUP):
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            if after:
                after()
            if i >= WARMUP:
                out.append(t1 - t0)
        return stats(out)

    stream = torch.cuda.ExternalStream(svo.stream)

    def event_us(fn, queue=100, rounds=5):
        per_call = []
        for _ in range(rounds + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(queue):
                fn()
            e1.record(stream)
            L.vx_sync(h)
            per_call.append(e0.elapsed_time(e1) * 1e-3 / queue)
        return stats(per_call[1:])

    _vp = hip._vp
    results = []
    for n in COUNTS:
        idx = np.linspace(0, len(fan) - 1, n).astype(np.int64) if n < len(fan) else np.arange(n)
        d = np.ascontiguousarray(fan[idx])
        o = np.ascontiguousarray(np.tile(eye, (n, 1)))
        m = np.full(n, -1.0, dtype=np.float32)
        tasks = np.zeros(n, dtype=hip.PICKER_TASK_DTYPE)
        tasks["pos"], tasks["dir"], tasks["max_dst"] = o, d, m
        res, hits = np.zeros(n, dtype=hip.PICKER_RESULT_DTYPE), np.zeros(n, dtype=hip.RAY_HIT_DTYPE)
        b = hip.RayBatch(o.ctypes.data, d.ctypes.data, m.ctypes.data, 12, 12, 4, -1.0, 0)
        rc = lambda: L.vx_raycast(h, tasks.ctypes.data_as(_vp), n, res.ctypes.data_as(_vp))  # noqa: E731
        rb = lambda: L.vx_raycast_batch(h, hip.C.byref(b), n, hip.VX_MEM_HOST, hits.ctypes.data_as(_vp))  # noqa: E731
        assert rc() == 0 and rb() == 0
        assert hits["dst"].tobytes() == res["dst"].tobytes() and hits["pos"].tobytes() == res["pos"].tobytes(), "vx_raycast_batch and vx_raycast disagree"
        first, batch, again = timed(rc), timed(rb), timed(rc)
        d_o, d_d, d_m = (torch.from_numpy(a).cuda() for a in (o, d, m))
        d_hits = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        db = hip.RayBatch(d_o.data_ptr(), d_d.data_ptr(), d_m.data_ptr(), 12, 12, 4, -1.0, 0)
        dv = lambda: L.vx_raycast_batch(h, hip.C.byref(db), n, hip.VX_MEM_DEVICE, _vp(d_hits.data_ptr()))  # noqa: E731
        assert dv() == 0 and L.vx_sync(h) == 0
        assert hip.ray_hits_to_numpy(d_hits).tobytes() == hits.tobytes(), "device and host hits disagree"
        results.append({"format": fmt, "rays": n, "hits": int((hits["dst"] > 0).sum()), "repeats": REPS, "raycast_us": first, "batch_us": batch,
                        "raycast_again_us": again, "device_return_us": timed(dv, after=lambda: L.vx_sync(h)), "device_event_us": event_us(dv)})
        print(json.dumps(results[-1]), flush=True)

    # 4,096 look rays from the positions inside vx_entity records
    n = 4096
    rng = np.random.default_rng(3)
    e = np.zeros(n, dtype=hip.ENTITY_DTYPE)
    e["position"] = np.stack([rng.uniform(0.3, 0.7, n) * size, np.full(n, st["h_max"] + 2.0), rng.uniform(0.3, 0.7, n) * size], axis=1)
    d_e = torch.from_numpy(e.view(np.uint8).copy()).cuda()
    look = torch.from_numpy(fan[len(fan) // 2 + 128].copy()).cuda()
    d_hits = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    eb = hip.RayBatch(hip.entity_positions(d_e).data_ptr(), look.data_ptr(), None, 64, 0, 0, 100.0, 0)
    ev = lambda: L.vx_raycast_batch(h, hip.C.byref(eb), n, hip.VX_MEM_DEVICE, _vp(d_hits.data_ptr()))  # noqa: E731
    assert ev() == 0 and L.vx_sync(h) == 0
    exp = svo.raycast_batch(hip.entity_positions(e), fan[len(fan) // 2 + 128], 100.0)
    assert hip.ray_hits_to_numpy(d_hits).tobytes() == exp.tobytes(), "entity-record rays: device and host hits disagree"
    results.append({"format": fmt, "rays": n, "source": "vx_entity records, stride 64, one direction", "hits": int((exp["dst"] > 0).sum()), "repeats": REPS,
                    "device_return_us": timed(ev, after=lambda: L.vx_sync(h)), "device_event_us": event_us(ev)})
    print(json.dumps(results[-1]), flush=True)
    svo.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", metavar="FORMAT")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "raycast_batch" / "results.json"))
    ap.add_argument("--formats", default="esvo,csvo")
    ap.add_argument("--timeout", type=int, default=240)
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
    Path(args.out).write_text(json.dumps({"device": "MI355X (gfx950)", "scene": "heightfield depth 12", "unit": "microseconds per call", "cases": results}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
