"""Entity physics, microseconds per call: the path over vx_raycast against vx_physics_step.

    python profiles/physics_bench.py [--out profiles/physics/results.json] [--formats esvo,csvo]

For N entities x K steps in {1x1, 1x4, 48x1, 48x8, 4096x4}, on the depth-7 heightfield with the entities settled on the ground:
  (a) step_many_us        vxh_physics_step_many: Physics::step_many over vx_raycast, K blocking picker round trips (the existing path)
  (b) host_us             vx_physics_step on host records: one launch, one wait
  (c) device_enqueue_us   vx_physics_step on device records: the call alone (it returns after enqueueing) ...
      device_synced_us    ... and the call plus vx_sync
Every case runs in a child process of its own under `timeout`; the driver stops at the first that fails. Medians over the repeats, with
the 10th and 90th percentiles beside them."""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CASES = [(1, 1), (1, 4), (48, 1), (48, 8), (4096, 4)]


def case(fmt, n, k):
    sys.path.insert(0, str(ROOT))
    import numpy as np
    import torch

    from _pkg import load_package

    vra = load_package()
    from voxel_rs_amd import hip, host, scenes

    svo_type = vra.SVO_ESVO if fmt == "esvo" else vra.SVO_CSVO
    world = vra.World(svo_type)
    st = world.build_heightfield(7, threads=4)
    svo = hip.Svo(svo_type, world.size_in_bytes + (1 << 20))
    svo.set_materials(scenes.synthetic_materials())
    svo.set_textures(scenes.synthetic_textures(), 6)
    svo.update(world)
    rng = np.random.default_rng(3)
    pos = np.stack([rng.uniform(8, 120, n), np.full(n, st["h_max"] + 2.0), rng.uniform(8, 120, n)], axis=1).astype(np.float32)
    rows = host.make_entities(pos)
    rows[:, 3], rows[:, 5] = rng.uniform(-6, 6, n), rng.uniform(-6, 6, n)
    dt = np.float32(1.0 / 250.0)
    settled = hip.entities_from_rows(rows)
    svo.physics_step(settled, dt, 400)  # 1.6 s: everybody stands, or walks, on the ground
    reps = 30 if n * k > 10000 else 300

    def timed(fn, after=None):
        out = []
        for i in range(reps + 20):
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            if after:
                after()
            t2 = time.perf_counter()
            if i >= 20:
                out.append((t1 - t0, t2 - t0))
        return np.array(out) * 1e6

    def stats(v):
        return {"median": round(float(np.median(v)), 2), "p10": round(float(np.percentile(v, 10)), 2), "p90": round(float(np.percentile(v, 90)), 2)}

    a_rows = hip.entities_to_rows(settled)
    a = timed(lambda: host.lib().vxh_physics_step_many(svo._h, dt, k, a_rows.ctypes.data, n))[:, 0]
    b_e = settled.copy()
    b_ptr = b_e.ctypes.data
    b = timed(lambda: hip.lib().vx_physics_step(svo._h, b_ptr, n, hip.VX_MEM_HOST, dt, k, None))[:, 0]
    d = torch.from_numpy(settled.view(np.uint8).copy()).cuda()
    d_ptr = d.data_ptr()
    c = timed(lambda: hip.lib().vx_physics_step(svo._h, d_ptr, n, hip.VX_MEM_DEVICE, dt, k, None), after=lambda: hip.lib().vx_sync(svo._h))
    # the three ran the same entities: they must still agree
    assert hip.entities_to_rows(b_e).tobytes() == a_rows.tobytes(), "vx_physics_step and step_many over vx_raycast disagree"
    assert d.cpu().numpy().tobytes() == b_e.tobytes(), "device and host records disagree"
    print(json.dumps({"format": fmt, "entities": n, "steps": k, "repeats": reps, "step_many_us": stats(a), "host_us": stats(b),
                      "device_enqueue_us": stats(c[:, 0]), "device_synced_us": stats(c[:, 1])}))
    svo.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", nargs=3, metavar=("FORMAT", "N", "K"))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "physics" / "results.json"))
    ap.add_argument("--formats", default="esvo,csvo")
    ap.add_argument("--timeout", type=int, default=120)
    args = ap.parse_args()
    if args.case:
        case(args.case[0], int(args.case[1]), int(args.case[2]))
        return 0
    results = []
    for fmt in args.formats.split(","):
        for n, k in CASES:
            r = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, __file__, "--case", fmt, str(n), str(k)], stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:
                print(f"case {fmt} {n}x{k} ended with status {r.returncode}: stopping", file=sys.stderr)
                return r.returncode
            line = r.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            results.append(json.loads(line))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": "MI355X (gfx950)", "scene": "heightfield depth 7", "unit": "microseconds per call", "cases": results}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
