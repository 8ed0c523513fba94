"""The first block along an axis, microseconds per call: vx_scan_points and vx_scan_columns, beside the two things a caller did before them.

    python profiles/scan_bench.py [--out profiles/scan/results.json] [--formats esvo,csvo]

On the depth-12 bench world (bench.py's C3 scene), device memory throughout:
  vx_scan_points downwards (VX_DIR_NEG_Y, VX_SCAN_TO_EDGE) for 1 / 4,096 / 1,048,576 positions spread through the air above the terrain
  around the camera (packed [N,3]; the 4,096 and the 1,048,576 also as the positions inside vx_entity records, stride 64); `found`: how many
  have ground below them;
  vx_scan_columns: top-down heightmaps (VX_DIR_NEG_Y over the world's whole height) of 64^2, 256^2 and 1,024^2 columns over the terrain
  where the C3 camera looks, on the tile grid, the 256^2 one also one voxel off it; 256^2 over open sky (a box 512 voxels high that starts
  600 above the terrain: every tile ends in empty space); one side elevation (VX_DIR_POS_X through the whole world, 256 x 256 columns of y
  and z).
Beside each heightmap, what a caller did at this commit's parent:
  rays        vx_raycast_batch of the same columns as downward rays from the cell centres at the top of the scanned extent;
  region      vx_read_region of the largest sub-box of the same footprint that call accepts (2^24 voxels: 4,096 / 256 / 16 voxels high
              from the top of the terrain's layer), which the caller would then have to reduce, and to repeat for the rest of the height.
    call_sync_us      the host clock around the call and the vx_sync behind it
    device_event_us   HIP-event time per call over a queue of calls on the context's stream
    rays_over_scan, region_over_scan    the ratios of the device_event_us medians
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
MAPS = [64, 256, 1024]
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
    size = 1 << depth
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

    def timed(fn, queue):
        assert fn() == 0 and L.vx_sync(h) == 0, L.vx_last_error()
        return {"call_sync_us": call_sync(fn), "device_event_us": event(fn, queue)}

    rng = np.random.default_rng(5)
    for n in POINT_COUNTS:
        p = np.stack([rng.uniform(0.25, 0.75, n) * size, rng.uniform(0.0, h_max + 64.0, n), rng.uniform(0.25, 0.75, n) * size], axis=1).astype(np.float32)
        d_p = torch.from_numpy(np.ascontiguousarray(p)).cuda()
        d_out = torch.empty((n, 4), dtype=torch.int32, device="cuda")
        fn = lambda: L.vx_scan_points(h, _vp(d_p.data_ptr()), 12, n, hip.VX_DIR_NEG_Y, hip.VX_SCAN_TO_EDGE, hip.VX_MEM_DEVICE, _vp(d_out.data_ptr()))  # noqa: E731
        row = {"format": fmt, "call": "vx_scan_points", "points": n, **timed(fn, 50 if n < (1 << 20) else 10)}
        hits = hip.scan_hits_to_numpy(d_out)
        assert hits[:4096].tobytes() == svo.scan_points(p[:4096], hip.VX_DIR_NEG_Y).tobytes(), "device and host records disagree"
        row["found"] = int((hits["coord"] != hip.VX_SCAN_NONE).sum())
        print(json.dumps(row), flush=True)
        if n >= 4096:
            e = np.zeros(n, dtype=hip.ENTITY_DTYPE)
            e["position"] = p
            d_e = torch.from_numpy(e.view(np.uint8).copy()).cuda()
            fe = lambda: L.vx_scan_points(h, _vp(hip.entity_positions(d_e).data_ptr()), 64, n, hip.VX_DIR_NEG_Y, hip.VX_SCAN_TO_EDGE, hip.VX_MEM_DEVICE, _vp(d_out.data_ptr()))  # noqa: E731
            row = {"format": fmt, "call": "vx_scan_points", "points": n, "source": "vx_entity records, stride 64", **timed(fe, 50 if n < (1 << 20) else 10)}
            assert hip.scan_hits_to_numpy(d_out).tobytes() == hits.tobytes()
            print(json.dumps(row), flush=True)

    # where the C3 camera looks: along (0.6, -0.35, 0.7) from the eye down to the terrain's layer
    look = np.float64([0.6, -0.35, 0.7])
    ground = eye + look * ((eye[1] - 0.5 * h_max) / 0.35)
    layer_top = (int(h_max) + 8) // 8 * 8  # above every block of the terrain

    def scan_row(what, lo, box, direction, queue, compare):
        a = direction >> 1
        u, v = (1 if a == 0 else 0), (1 if a == 2 else 2)
        lo3, size3 = (C.c_int32 * 3)(*lo), (C.c_uint32 * 3)(*box)
        d_out = torch.empty((box[v], box[u], 4), dtype=torch.int32, device="cuda")
        fn = lambda: L.vx_scan_columns(h, C.byref(lo3), C.byref(size3), direction, hip.VX_MEM_DEVICE, _vp(d_out.data_ptr()))  # noqa: E731
        row = {"format": fmt, "call": "vx_scan_columns", "what": what, "lo": list(lo), "size": list(box), "direction": direction, **timed(fn, queue)}
        hits = hip.scan_hits_to_numpy(d_out)
        row["found"] = int((hits["coord"] != hip.VX_SCAN_NONE).sum())
        if compare:
            # the same columns as downward rays from the cell centres at the top of the extent
            z, x = np.meshgrid(np.arange(box[2]), np.arange(box[0]), indexing="ij")
            top = min(lo[1] + box[1], size)
            o = np.ascontiguousarray(np.stack([x + lo[0] + 0.5, np.full(x.shape, top - 0.5), z + lo[2] + 0.5], axis=-1).reshape(-1, 3).astype(np.float32))
            d_o, d_d = torch.from_numpy(o).cuda(), torch.from_numpy(np.float32([0.0, -1.0, 0.0])).cuda()
            d_hits = torch.empty((len(o), 8), dtype=torch.int32, device="cuda")
            batch = hip.RayBatch()
            batch.origin, batch.origin_stride, batch.dir, batch.dir_stride = d_o.data_ptr(), 12, d_d.data_ptr(), 0
            batch.max_dst, batch.max_dst_stride, batch.max_dst_all, batch.flags = None, 0, -1.0, 0
            fr = lambda: L.vx_raycast_batch(h, C.byref(batch), len(o), hip.VX_MEM_DEVICE, _vp(d_hits.data_ptr()))  # noqa: E731
            row["rays"] = timed(fr, queue)
            ray_hits = hip.ray_hits_to_numpy(d_hits)
            row["rays"]["hit"] = int((ray_hits["dst"] > 0).sum())
            row["rays"]["same_value"] = int((ray_hits["value"] == hits["value"].reshape(-1)).sum())
            # the largest sub-box vx_read_region accepts over this footprint, from the top of the terrain's layer down
            tall = min((1 << 24) // (box[0] * box[2]), size)
            rlo3, rsize3 = (C.c_int32 * 3)(lo[0], max(layer_top - tall, 0), lo[2]), (C.c_uint32 * 3)(box[0], tall, box[2])
            d_ids = torch.empty((box[2], tall, box[0]), dtype=torch.int32, device="cuda")
            fg = lambda: L.vx_read_region(h, C.byref(rlo3), C.byref(rsize3), hip.VX_MEM_DEVICE, _vp(d_ids.data_ptr()))  # noqa: E731
            row["region"] = {"size": [box[0], tall, box[2]], **timed(fg, max(queue // 4, 2))}
            row["rays_over_scan"] = round(row["rays"]["device_event_us"]["median"] / row["device_event_us"]["median"], 2)
            row["region_over_scan"] = round(row["region"]["device_event_us"]["median"] / row["device_event_us"]["median"], 2)
        print(json.dumps(row), flush=True)

    for s in MAPS:
        corner = tuple(int(v) // 8 * 8 - s // 2 for v in (ground[0], ground[2]))
        scan_row("heightmap over the terrain", (corner[0], 0, corner[1]), (s, size, s), hip.VX_DIR_NEG_Y, 20 if s < 1024 else 5, True)
        if s == 256:
            scan_row("heightmap one voxel off the tile grid", (corner[0] + 1, 0, corner[1] + 1), (s, size, s), hip.VX_DIR_NEG_Y, 20, True)
            scan_row("heightmap over open sky", (corner[0], min(layer_top + 600, size - 512), corner[1]), (s, 512, s), hip.VX_DIR_NEG_Y, 20, True)
            scan_row("side elevation", (0, layer_top - 256, corner[1]), (size, 256, s), hip.VX_DIR_POS_X, 20, False)
    svo.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", metavar="FORMAT")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "scan" / "results.json"))
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
                                          "repeats": REPS, "cases": results}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
