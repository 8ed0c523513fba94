"""Block ids read from the device, microseconds per call: vx_block_points and vx_read_region.

    python profiles/blocks_bench.py [--out profiles/blocks/results.json] [--formats esvo,csvo]

On the depth-12 bench world (bench.py's C3 scene), device memory throughout:
  vx_block_points for 1 / 4,096 / 1,048,576 points spread through the terrain's layer around the camera (packed [N,3]; the 4,096 also as the
  positions inside vx_entity records, stride 64). The world is a heightfield's shell, so nearly all of them lie in air (`solid`: how many do not);
  vx_read_region for boxes of 64^3, 128^3 and 256^3 voxels centred on the C3 camera's look-at point in the terrain (`terrain`) and high
  above it (`sky`: every brick ends in empty space), on the brick grid and one voxel off it (masked edge bricks); `solid`: the blocks in the box.
    call_sync_us      the host clock around the call and the vx_sync behind it
    device_event_us   HIP-event time per call over a queue of calls on the context's stream
    output_gbs        regions: the box's 4 bytes a voxel over device_event_us; for scale, the device's HBM takes 8.0 TB/s by its
                      specification and 6.3 TB/s in a copy kernel
Each format runs in a child process of its own under `timeout`; the driver stops at the first that fails. Medians over at least 20 calls
after warm-up, with the 10th and 90th percentiles beside them. There is no threshold."""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
POINT_COUNTS = [1, 4096, 1 << 20]
BOXES = [64, 128, 256]
REPS, WARMUP = 40, 10


def case(fmt):
    sys.path.insert(0, str(ROOT))
    import numpy as np
    import torch

    from _pkg import load_package

    vra = load_package()
    from voxel_rs_amd import hip, scenes

    depth = 12
    svo_type = vra.SVO_ESVO if fmt == "esvo" else vra.SVO_CSVO
    world = vra.World(svo_type)
    st = world.build_heightfield(depth)
    svo = hip.Svo(svo_type, world.size_in_bytes + (4 << 20))
    svo.set_materials(scenes.synthetic_materials())
    svo.set_textures(scenes.synthetic_textures(), 6)
    svo.update(world)
    L, h, _vp, C = hip.lib(), svo._h, hip._vp, hip.C
    size = float(1 << depth)
    h_max = float(st["h_max"])
    eye = np.float64([0.5 * size, h_max + 0.05 * size, 0.5 * size])
    stream = torch.cuda.ExternalStream(svo.stream)

    def stats(v):
        v = np.asarray(v) * 1e6
        return {"median": round(float(np.median(v)), 2), "p10": round(float(np.percentile(v, 10)), 2), "p90": round(float(np.percentile(v, 90)), 2)}

    def call_sync(fn):
        out = []
        for i in range(REPS + WARMUP):
            t0 = time.perf_counter()
            fn()
            L.vx_sync(h)
            if i >= WARMUP:
                out.append(time.perf_counter() - t0)
        return stats(out)

    def event(fn, queue, rounds=20):
        per_call = []
        for _ in range(rounds + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(queue):
                fn()
            e1.record(stream)
            L.vx_sync(h)
            per_call.append(e0.elapsed_time(e1) * 1e-3 / queue)
        return stats(per_call[2:])

    rng = np.random.default_rng(5)
    for n in POINT_COUNTS:
        p = np.stack([rng.uniform(0.25, 0.75, n) * size, rng.uniform(0.0, h_max + 8.0, n), rng.uniform(0.25, 0.75, n) * size], axis=1).astype(np.float32)
        d_p = torch.from_numpy(np.ascontiguousarray(p)).cuda()
        d_out = torch.empty((n, 2), dtype=torch.int32, device="cuda")
        fn = lambda: L.vx_block_points(h, _vp(d_p.data_ptr()), 12, n, hip.VX_MEM_DEVICE, _vp(d_out.data_ptr()))  # noqa: E731
        assert fn() == 0 and L.vx_sync(h) == 0
        cells = hip.block_cells_to_numpy(d_out)
        check = svo.block_points(p[:4096])
        assert cells[:4096].tobytes() == check.tobytes(), "device and host records disagree"
        row = {"format": fmt, "call": "vx_block_points", "points": n, "solid": int((cells["value"] != 0).sum()), "call_sync_us": call_sync(fn),
               "device_event_us": event(fn, 50 if n < (1 << 20) else 10)}
        print(json.dumps(row), flush=True)
        if n == 4096:
            e = np.zeros(n, dtype=hip.ENTITY_DTYPE)
            e["position"] = p
            d_e = torch.from_numpy(e.view(np.uint8).copy()).cuda()
            fe = lambda: L.vx_block_points(h, _vp(hip.entity_positions(d_e).data_ptr()), 64, n, hip.VX_MEM_DEVICE, _vp(d_out.data_ptr()))  # noqa: E731
            assert fe() == 0 and L.vx_sync(h) == 0 and hip.block_cells_to_numpy(d_out).tobytes() == cells.tobytes()
            print(json.dumps({"format": fmt, "call": "vx_block_points", "points": n, "source": "vx_entity records, stride 64", "call_sync_us": call_sync(fe),
                              "device_event_us": event(fe, 50)}), flush=True)

    # where the C3 camera looks: along (0.6, -0.35, 0.7) from the eye down to the terrain's layer
    look = np.float64([0.6, -0.35, 0.7])
    ground = eye + look * ((eye[1] - 0.5 * h_max) / 0.35)
    for where, centre in (("terrain", ground), ("sky", np.float64([ground[0], min(h_max + 600.0, size - 200.0), ground[2]]))):
        for s in BOXES:
            for odd in (0, 1):
                lo = tuple(int(v) // 8 * 8 - s // 2 + odd for v in centre)
                lo3, size3 = (C.c_int32 * 3)(*lo), (C.c_uint32 * 3)(s, s, s)
                d_out = torch.empty((s, s, s), dtype=torch.int32, device="cuda")
                fn = lambda: L.vx_read_region(h, C.byref(lo3), C.byref(size3), hip.VX_MEM_DEVICE, _vp(d_out.data_ptr()))  # noqa: E731
                assert fn() == 0 and L.vx_sync(h) == 0
                ids = d_out.cpu().numpy().view(np.uint32)
                if s == 64:  # the region's voxels are the points at their centres
                    z, y, x = np.meshgrid(np.arange(s), np.arange(s), np.arange(s), indexing="ij")
                    c = np.ascontiguousarray(np.stack([x + lo[0] + 0.5, y + lo[1] + 0.5, z + lo[2] + 0.5], axis=-1).reshape(-1, 3).astype(np.float32))
                    assert (svo.block_points(c)["value"] == ids.reshape(-1)).all(), "region and points disagree"
                ev = event(fn, 20 if s < 256 else 5)
                row = {"format": fmt, "call": "vx_read_region", "where": where, "box": s, "lo": list(lo), "on_brick_grid": not odd, "solid": int((ids != 0).sum()),
                       "call_sync_us": call_sync(fn), "device_event_us": ev, "output_gbs": round(4.0 * s ** 3 / (ev["median"] * 1e-6) / 1e9, 1)}
                print(json.dumps(row), flush=True)
    svo.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", metavar="FORMAT")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "blocks" / "results.json"))
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
    Path(args.out).write_text(json.dumps({"device": "MI355X (gfx950)", "scene": "heightfield depth 12 (bench.py's C3 world)", "unit": "microseconds per call",
                                          "hbm_peak_tbs": {"specification": 8.0, "copy_kernel": 6.3}, "repeats": REPS, "cases": results}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
