"""Walking distances and paths for ground agents around many positions, microseconds per batch: vx_walk_points beside what a caller did
before it, and beside vx_flood_points of the same box.

    python profiles/walk_bench.py [--out profiles/walk/results.json] [--formats esvo,csvo]

On the depth-12 bench world (bench.py's C3 scene), device memory throughout. The seeds stand on the terrain's surface around the C3 camera's
look-at point (the surface comes from vx_scan_columns, VX_DIR_NEG_Y, over 512 x 512 columns), the seed in the middle of the box; each goal is
the surface cell three columns along x and two along z from its seed. An agent two cells high that climbs one block and drops up to three;
max_steps 250.
    counts    1, 64 and 4,096 positions
    shapes    9 x 8 x 9, 17 x 12 x 17 and 32 x 28 x 32 cells
    outputs   fields and records; records only; paths only (capacity 8) under VX_WALK_STOP_AT_GOAL
Beside each:
    walk      vx_walk_points: one workgroup a query; as many calls as 2^24 bytes of fields a call need (otherwise one call)
    torch     the batch without it: one vx_read_region into device memory per box -- of the box with the layer below it and the two above --,
              then the same walk as a batched torch iteration on the context's stream: standable cells and the up and drop masks from
              shifted slices, both seeds and goals settled, then shifted ORs over [N, z, y, x] bool tensors with the three edge kinds,
              stepping until no frontier is left (one flag read back a step) or max_steps, the step counts written into a uint8 field or --
              records only -- the reached cells counted. For the paths row it steps until every goal that can be has been reached and keeps
              the goals' step counts: the back-trace itself is left out of its time, which favours it. Measured where N * voxels <= 2^25;
              elsewhere the row says so.
    flood     vx_flood_points of the same box and positions with the same outputs (fields and records, or records): the floor a bit-row flood
              costs. (Not the same question: it floods the air above the terrain.)
    call_sync_us      the host clock around one batch (all its calls) and the vx_sync behind it
    device_event_us   walk only: HIP-event time per batch over a queue of batches on the context's stream
    torch_over_walk   torch's median call_sync_us over the walk's: above 1 vx_walk_points wins, below 1 it loses
    walk_over_flood   the walk's median call_sync_us over the flood's
The fields (records only: the reached counts; paths: the goals' step counts) of the two ways are compared query for query before anything is
timed. At N = 1 every figure is the latency of one launch and one wait, not throughput. Each format runs in a child process of its own under
`timeout`; the driver stops at the first that fails. Medians after warm-up, with the 10th and 90th percentiles beside them. There is no
threshold."""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REPS, WARMUP = 10, 3
TORCH_REPS, TORCH_WARMUP = 4, 1
FIELD_BYTES_A_CALL = 1 << 24
TORCH_CELLS = 1 << 25
HEIGHT, CLIMB, DROP, MAX_STEPS, CAPACITY = 2, 1, 3, 250, 8


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
    L, h, C = hip.lib(), svo._h, hip.C
    size = float(1 << depth)
    h_max = float(st["h_max"])
    eye = np.float64([0.5 * size, h_max + 0.05 * size, 0.5 * size])
    stream = torch.cuda.ExternalStream(svo.stream)

    def stats(v):
        v = np.asarray(v) * 1e6
        return {"median": round(float(np.median(v)), 2), "p10": round(float(np.percentile(v, 10)), 2), "p90": round(float(np.percentile(v, 90)), 2)}

    def call_sync(fn, reps=REPS, warmup=WARMUP):
        out = []
        for i in range(reps + warmup):
            t0 = time.perf_counter()
            fn()
            L.vx_sync(h)
            if i >= warmup:
                out.append(time.perf_counter() - t0)
        return stats(out)

    def event(fn, queue, rounds=6):
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
    rng = np.random.default_rng(7)
    side = 512
    height = svo.scan_columns((gx - side // 2, 0, gz - side // 2), (side, 1 << depth, side), hip.VX_DIR_NEG_Y, device=True)
    svo.sync()
    top = height[:, :, 0].clamp(min=-1).to(torch.float32) + 1.0  # [z][x]: the first air cell of the column
    zz, xx = torch.meshgrid(torch.arange(side, device="cuda"), torch.arange(side, device="cuda"), indexing="ij")
    fx, fz = xx.to(torch.float32) + (gx - side // 2) + 0.5, zz.to(torch.float32) + (gz - side // 2) + 0.5
    standing = torch.stack([fx, top + 0.5, fz], dim=-1).reshape(-1, 3)
    aims = torch.stack([fx + 3.0, torch.roll(top, shifts=(-2, -3), dims=(0, 1)) + 0.5, fz + 2.0], dim=-1).reshape(-1, 3)
    inner = ((xx < side - 4) & (zz < side - 4)).reshape(-1).cpu().numpy()
    chosen = torch.from_numpy(rng.permutation(np.flatnonzero(inner))[:4096]).cuda()
    standing, aims = standing[chosen].contiguous(), aims[chosen].contiguous()

    def beside(a):
        out = torch.zeros_like(a)
        out[..., 1:] |= a[..., :-1]
        out[..., :-1] |= a[..., 1:]
        out[:, 1:] |= a[:, :-1]
        out[:, :-1] |= a[:, 1:]
        return out

    def settled(column, e, rows):
        """The layer on which agents put into layer e of passable columns [N, layers] come to stand, and whether they stand at all: headroom
        where they are put, then down to the highest layer below them that does not pass."""
        ok = torch.ones(len(e), dtype=torch.bool, device="cuda")
        for j in range(HEIGHT):
            ok &= column[rows, e + j]
        layer = torch.arange(column.shape[1], device="cuda")
        below = ~column & (layer[None, :] < e[:, None])
        floor = torch.where(below, layer[None, :], -1).max(dim=1).values
        return floor + 1, ok & (floor >= 0)

    for shape in ((9, 8, 9), (17, 12, 17), (32, 28, 32)):
        sx, sy, sz = shape
        ax, ay, az = seed_at = (sx // 2, sy // 2, sz // 2)
        voxels = sx * sy * sz
        stride = (voxels + 15) // 16 * 16
        for n in (1, 64, 4096):
            pos, goal = standing[:n].contiguous(), aims[:n].contiguous()
            a_call = max(FIELD_BYTES_A_CALL // stride, 1)
            fields = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
            info = torch.empty((n, 8), dtype=torch.int32, device="cuda")
            paths = torch.empty((n, CAPACITY), dtype=torch.int32, device="cuda")
            flood_info = torch.empty((n, 4), dtype=torch.int32, device="cuda")
            los = torch.floor(pos).to(torch.int32).cpu().numpy() - np.int32(seed_at)
            with_torch = n * voxels <= TORCH_CELLS
            regions = torch.empty((n, sz, sy + HEIGHT, sx), dtype=torch.int32, device="cuda") if with_torch else None
            lo3s = [(C.c_int32 * 3)(int(los[i][0]), int(los[i][1]) - 1, int(los[i][2])) for i in range(n)] if with_torch else []
            size3 = (C.c_uint32 * 3)(sx, sy + HEIGHT, sz)
            goal_cell = torch.floor(goal).to(torch.int64) - torch.from_numpy(los.astype(np.int64)).cuda()
            goal_in = ((goal_cell >= 0) & (goal_cell < torch.tensor(shape, device="cuda"))).all(dim=1)  # (the terrain may put it above or below the box)
            goal_cell = torch.where(goal_in[:, None], goal_cell, 0)
            rows = torch.arange(n, device="cuda")
            for outputs in ("fields+info", "info", "paths+stop"):
                flags = hip.VX_WALK_STOP_AT_GOAL if outputs == "paths+stop" else 0

                def walk():
                    kw = dict(seed_at=seed_at, max_steps=MAX_STEPS, height=HEIGHT, climb=CLIMB, drop=DROP, flags=flags)
                    if outputs == "info":
                        svo.walk_points(pos, shape, goal, fields=None, info=info, paths=False, **kw)
                    elif outputs == "paths+stop":
                        svo.walk_points(pos, shape, goal, fields=None, info=None, paths=paths, path_capacity=CAPACITY, **kw)
                    else:
                        for at in range(0, n, a_call):
                            svo.walk_points(pos[at:at + a_call], shape, goal[at:at + a_call], fields=fields[at:at + a_call], info=info[at:at + a_call], paths=False, **kw)

                def flood():
                    if outputs == "info":
                        svo.flood_points(pos, shape, seed_at, MAX_STEPS, fields=None, info=flood_info)
                        return
                    for at in range(0, n, a_call):
                        svo.flood_points(pos[at:at + a_call], shape, seed_at, MAX_STEPS, fields=fields[at:at + a_call], info=flood_info[at:at + a_call])

                result = {}

                def by_torch():
                    for i in range(n):
                        assert L.vx_read_region(h, C.byref(lo3s[i]), C.byref(size3), hip.VX_MEM_DEVICE, hip._vp(regions[i].data_ptr())) == 0
                    with torch.cuda.stream(stream):
                        passable = regions == 0
                        stand = ~passable[:, :, 0:sy]
                        for j in range(HEIGHT):
                            stand = stand & passable[:, :, 1 + j:1 + j + sy]
                        up_ok = torch.zeros_like(stand)
                        up_ok[:, :, :sy - 1] = passable[:, :, 1 + HEIGHT:HEIGHT + sy]
                        clear, free = [], torch.ones_like(stand)
                        for d in range(1, DROP + 1):
                            now = torch.zeros_like(stand)
                            now[:, :, :sy - d] = free[:, :, :sy - d] & passable[:, :, HEIGHT + d:HEIGHT + sy]
                            free = now
                            clear.append(now)
                        e, ok = settled(passable[:, az, :, ax], torch.full((n,), ay + 1, dtype=torch.int64, device="cuda"), rows)
                        frontier = torch.zeros_like(stand)
                        frontier[rows[ok], az, e[ok] - 1, ax] = True
                        reached = frontier.clone()
                        want_goal, want_field = outputs == "paths+stop", outputs == "fields+info"
                        if want_goal:
                            ge, gok = settled(passable[rows, goal_cell[:, 2], :, goal_cell[:, 0]], goal_cell[:, 1] + 1, rows)
                            gok, gy = gok & goal_in, (ge - 1).clamp(min=0)
                            goal_steps = torch.where(gok & frontier[rows, goal_cell[:, 2], gy, goal_cell[:, 0]], 0, -1)
                            pending = gok & (goal_steps < 0)
                        field = None
                        if want_field:
                            field = torch.where(stand, 0xFE, 0xFF).to(torch.uint8)
                            field[frontier] = 0
                        for step in range(1, MAX_STEPS + 1):
                            near = beside(frontier)
                            grow = near.clone()
                            grow[:, :, 1:] |= beside(frontier & up_ok)[:, :, :-1]
                            for d, free_above in enumerate(clear, start=1):
                                grow[:, :, :-d] |= near[:, :, d:] & free_above[:, :, :-d]
                            grow &= stand & ~reached
                            if want_goal:  # (a query whose goal has been reached goes on with the others: only its goal's step count is kept)
                                found = pending & grow[rows, goal_cell[:, 2], gy, goal_cell[:, 0]]
                                goal_steps = torch.where(found, step, goal_steps)
                                pending = pending & ~found
                                go_on = grow.any() & pending.any()
                            else:
                                go_on = grow.any()
                            reached |= grow
                            if want_field:
                                field.masked_fill_(grow, step)
                            frontier = grow
                            if not bool(go_on):  # (reads one byte back: the stream is waited for)
                                break
                        result["reached"] = reached.sum(dim=(1, 2, 3), dtype=torch.int32)
                        result["field"] = field
                        result["goal_steps"] = goal_steps if want_goal else None

                info.fill_(-1)
                torch.cuda.synchronize()  # (what torch has prepared on its own stream is there before the context's stream reads it)
                walk()
                if outputs == "paths+stop":  # (the records of the same call, for the comparison and the row)
                    svo.walk_points(pos, shape, goal, seed_at=seed_at, max_steps=MAX_STEPS, height=HEIGHT, climb=CLIMB, drop=DROP, flags=flags, fields=None, info=info, paths=False)
                svo.sync()
                got = info.clone()
                if with_torch:
                    by_torch()
                    svo.sync()
                    if outputs == "paths+stop":
                        assert torch.equal(got[:, 6], result["goal_steps"].to(torch.int32)), "vx_walk_points and the torch walk disagree on a goal's step count"
                        steps = got[:, 6].clamp(max=CAPACITY)
                        assert torch.equal((paths != -1).sum(dim=1), torch.where(got[:, 6] < 0, 0, steps).to(torch.int64)), "a path's length is not its goal's step count"
                    else:
                        assert torch.equal(got[:, 0], result["reached"]), "vx_walk_points and the torch walk disagree on the reached cells"
                    if outputs == "fields+info":
                        assert torch.equal(fields[:, :voxels], result["field"].reshape(n, -1)), "vx_walk_points and the torch walk disagree on a field"
                calls = (n + a_call - 1) // a_call if outputs == "fields+info" else 1
                queue = 20 if n * voxels < (1 << 24) else 3
                routed = got[:, 6] >= 0
                row = {"format": fmt, "call": "vx_walk_points", "queries": n, "shape": list(shape), "max_steps": MAX_STEPS, "outputs": outputs, "calls_a_batch": calls,
                       "reached_mean": round(float(got[:, 0].to(torch.float64).mean().item()), 1), "farthest_max": int(got[:, 1].max().item()),
                       "goals_reached": int(routed.sum().item()), "path_steps_mean": round(float(got[:, 6][routed].to(torch.float64).mean().item()), 1) if bool(routed.any()) else None,
                       "walk": {"call_sync_us": call_sync(walk), "device_event_us": event(walk, queue)}}
                if with_torch:
                    row["torch"] = {"call_sync_us": call_sync(by_torch, TORCH_REPS, TORCH_WARMUP)}
                    row["torch_over_walk"] = round(row["torch"]["call_sync_us"]["median"] / row["walk"]["call_sync_us"]["median"], 2)
                else:
                    row["torch"] = "not measured: N * voxels exceeds 2^25"
                if outputs != "paths+stop":
                    row["flood"] = {"call_sync_us": call_sync(flood)}
                    row["walk_over_flood"] = round(row["walk"]["call_sync_us"]["median"] / row["flood"]["call_sync_us"]["median"], 2)
                print(json.dumps(row), flush=True)
    svo.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", metavar="FORMAT")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "walk" / "results.json"))
    ap.add_argument("--formats", default="esvo,csvo")
    ap.add_argument("--timeout", type=int, default=420)
    args = ap.parse_args()
    if args.case:
        case(args.case)
        return 0
    results = []
    for fmt in args.formats.split(","):
        r = subprocess.Popen(["timeout", "-k", "10", str(args.timeout), sys.executable, __file__, "--case", fmt], stdout=subprocess.PIPE, text=True)
        for line in r.stdout:  # (row by row as they come)
            print(line.strip(), flush=True)
            results.append(json.loads(line))
        if r.wait() != 0:
            print(f"format {fmt} ended with status {r.returncode}: stopping", file=sys.stderr)
            return r.returncode
    kernel = {"with_field_or_path": {"vgprs": {"esvo": 66, "csvo": 88, "esvo_big": 68}, "sgprs": {"esvo": 99, "csvo": 106, "esvo_big": 101},
                                     "sgprs_spilled_to_vgpr_lanes": {"esvo": 0, "csvo": 2, "esvo_big": 0}, "scratch_bytes": 0, "lds_bytes": 53536, "workgroups_a_cu_by_lds": 3},
              "records_only": {"vgprs": {"esvo": 67, "csvo": 88, "esvo_big": 70}, "sgprs": {"esvo": 91, "csvo": 106, "esvo_big": 93}, "sgprs_spilled_to_vgpr_lanes": 0,
                               "scratch_bytes": 0, "lds_bytes": 20816},
              "source": "hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage on csrc/blocks/kernels_walk.hip"}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": "MI355X (gfx950)", "scene": "heightfield depth 12 (bench.py's C3 world)", "unit": "microseconds per batch",
                                          "agent": {"height": HEIGHT, "climb": CLIMB, "drop": DROP}, "repeats": REPS, "torch_repeats": TORCH_REPS,
                                          "kernel_resource_usage": kernel, "cases": results}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
