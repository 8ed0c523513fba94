"""What a batch of float boxes holds, microseconds per call: vx_overlap_boxes beside what a caller did before it.

    python profiles/boxes_bench.py [--out profiles/boxes/results.json] [--formats esvo,csvo]

On the depth-12 bench world (bench.py's C3 scene), device memory throughout. The workloads:
    standing  N = 1, 4,096 and 262,144 boxes of extents (0.8, 1.8, 0.8) standing on the terrain's surface around the C3 camera's look-at
              point: the surface comes from vx_scan_columns (VX_DIR_NEG_Y) over 512 x 512 columns, one box a column, every second one sunk
              by 0.5 into the ground
    cube16    4,096 boxes of 16^3 centred on points of that surface
    cube64    256 boxes of 64^3 centred on points of it (the largest a call takes: nine bricks an axis)
    sky       4,096 boxes of (0.8, 1.8, 0.8) in open sky high above it: every brick ends in empty space
Beside each:
    boxes     vx_overlap_boxes: one launch, one wave a box
    points    the batch without it: vx_block_points over the centres of all voxels of every cover (as many calls as 2^24 points a call
              need), then a segmented sum of value != 0 by torch.index_add_. The centres are worked out once, OUTSIDE the timing (a caller
              would have to build them every time): the time is the lookups' and the sum's alone, and it yields the counts only, neither
              the first block nor the bounds.
    list      the per-box way, N = 1 and 256 (the first 256 boxes of standing, and cube64): vx_list_region with capacity 0 for each box's
              cover, three launches a box, the totals into a device array.
    call_sync_us      the host clock around one call (points, list: all its steps) and the vx_sync behind it
    device_event_us   HIP-event time per call over a queue of calls on the context's stream
    points_over_boxes, list_over_boxes   the other way's median over this call's, per clock: above 1 this call wins, below 1 it loses
The counts of the three ways are compared box for box before anything is timed. At N = 1 every figure is the latency of one launch and one
wait, not throughput. Each format runs in a child process of its own under `timeout`; the driver stops at the first that fails. Medians
after warm-up, with the 10th and 90th percentiles beside them. There is no threshold."""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REPS, WARMUP = 20, 5
POINTS_A_CALL = 1 << 24


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

    def event(fn, queue, rounds=10):
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

    look = np.float64([0.6, -0.35, 0.7])
    ground = eye + look * ((eye[1] - 0.5 * h_max) / 0.35)
    gx, gz = int(ground[0]), int(ground[2])
    rng = np.random.default_rng(5)

    # the surface under 512 x 512 columns: a heightmap [z][x] from the device
    side = 512
    height = svo.scan_columns((gx - side // 2, 0, gz - side // 2), (side, 1 << depth, side), hip.VX_DIR_NEG_Y, device=True)
    svo.sync()
    top = height[:, :, 0].clamp(min=-1).to(torch.float32) + 1.0  # (no block: y = 0)
    zz, xx = torch.meshgrid(torch.arange(side, device="cuda"), torch.arange(side, device="cuda"), indexing="ij")
    sunk = ((xx + zz) % 2).to(torch.float32) * 0.5
    standing = torch.stack([xx.to(torch.float32) + (gx - side // 2) + 0.1, top - sunk, zz.to(torch.float32) + (gz - side // 2) + 0.1], dim=-1).reshape(-1, 3)
    standing = standing[torch.from_numpy(rng.permutation(side * side)).cuda()].contiguous()
    person = torch.tensor([0.8, 1.8, 0.8], dtype=torch.float32, device="cuda")

    def scattered(n, s):
        """n cubes of side s centred on points of that surface (off the voxel grid by the standing boxes' 0.1)"""
        return (standing[8192:8192 + n] - s / 2).contiguous()

    sky = torch.from_numpy((np.float64([ground[0], min(h_max + 600.0, size - 200.0), ground[2]]) + rng.uniform(-50.0, 50.0, (4096, 3))).astype(np.float32)).cuda()
    workloads = [("standing", standing[:1].contiguous(), person, True), ("standing", standing[:4096].contiguous(), person, False),
                 ("standing", standing, person, False), ("cube16", scattered(4096, 16.0), torch.full((3,), 16.0, device="cuda"), False),
                 ("cube64", scattered(256, 64.0), torch.full((3,), 64.0, device="cuda"), True), ("sky", sky, person, False)]
    workloads.insert(2, ("standing", standing[:256].contiguous(), person, True))

    for name, origin, extents, with_list in workloads:
        n = int(origin.shape[0])
        out = torch.empty((n, 8), dtype=torch.int32, device="cuda")

        def boxes():
            svo.overlap_boxes(origin, extents, out=out)

        # the covers, as a caller would work them out, and the centre of every voxel of them
        world_edge = float(1 << depth)
        first = torch.floor(origin).clamp(min=0.0)
        last = (torch.ceil(origin + extents).clamp(max=world_edge) - 1.0)
        width = (last - first + 1.0).clamp(min=0.0).to(torch.int64)
        per_box = width.prod(dim=1)
        owner = torch.repeat_interleave(torch.arange(n, device="cuda"), per_box)
        local = torch.arange(int(per_box.sum().item()), device="cuda") - torch.repeat_interleave(torch.cumsum(per_box, 0) - per_box, per_box)
        w = width[owner]
        centres = torch.stack([local % w[:, 0], local // w[:, 0] % w[:, 1], local // (w[:, 0] * w[:, 1])], dim=1).to(torch.float32) + first[owner] + 0.5
        centres = centres.contiguous()
        n_points = int(centres.shape[0])
        cells = torch.empty((n_points, 2), dtype=torch.int32, device="cuda")
        counts = torch.zeros(n, dtype=torch.int32, device="cuda")

        def points():
            for at in range(0, n_points, POINTS_A_CALL):
                svo.block_points(centres[at:at + POINTS_A_CALL], out=cells[at:at + POINTS_A_CALL])
            with torch.cuda.stream(stream):
                counts.zero_()
                counts.index_add_(0, owner, (cells[:, 0] != 0).to(torch.int32))

        totals = torch.zeros(n, dtype=torch.int32, device="cuda")
        lo_h, size_h = first.to(torch.int32).cpu().numpy(), width.to(torch.int32).cpu().numpy()
        regions = [((C.c_int32 * 3)(*(int(v) for v in lo_h[i])), (C.c_uint32 * 3)(*(int(v) for v in size_h[i]))) for i in range(n)] if with_list else []

        def listed():
            for i, (lo3, size3) in enumerate(regions):
                assert L.vx_list_region(h, C.byref(lo3), C.byref(size3), 0, hip.VX_MEM_DEVICE, None, 0, _vp(totals.data_ptr() + 4 * i)) == 0

        torch.cuda.synchronize()  # (what torch has prepared on its own stream is there before the context's stream reads it)
        boxes()
        points()
        listed()
        svo.sync()
        got = out[:, 0]
        assert torch.equal(got, counts), "vx_overlap_boxes and the sum over vx_block_points disagree"
        if with_list:
            assert torch.equal(got, totals), "vx_overlap_boxes and vx_list_region's totals disagree"
        queue = 20 if n_points < (1 << 22) else 3
        rows = {"boxes": boxes, "points": points}
        if with_list:
            rows["list"] = listed
        timed = {k: {"call_sync_us": call_sync(fn), "device_event_us": event(fn, queue)} for k, fn in rows.items()}
        row = {"format": fmt, "call": "vx_overlap_boxes", "workload": name, "boxes_n": n, "extents": [float(v) for v in extents.cpu()], "cover_voxels": n_points,
               "with_blocks": int((got > 0).sum().item()), "blocks": int(got.to(torch.int64).sum().item()), **timed}
        for k in rows:
            if k != "boxes":
                row[f"{k}_over_boxes"] = {c: round(timed[k][c]["median"] / timed["boxes"][c]["median"], 2) for c in ("call_sync_us", "device_event_us")}
        print(json.dumps(row), flush=True)
    svo.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", metavar="FORMAT")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "boxes" / "results.json"))
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
