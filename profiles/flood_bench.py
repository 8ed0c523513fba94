"""Step distances through air around many positions, microseconds per batch: vx_flood_points beside what a caller did before it.

    python profiles/flood_bench.py [--out profiles/flood/results.json] [--formats esvo,csvo]

On the depth-12 bench world (bench.py's C3 scene), device memory throughout. The positions stand 1.5 voxels above the terrain's surface around
the C3 camera's look-at point (the surface comes from vx_scan_columns, VX_DIR_NEG_Y, over 512 x 512 columns), the seed in the middle of the box.
    counts    1, 64, 4,096 and 65,536 positions
    shapes    9^3, 17^3 and 32^3 cells
    steps     max_steps 15 and 250
    outputs   fields and records, or records only
Beside each:
    flood     vx_flood_points: one workgroup a query; as many calls as 2^24 bytes of fields a call need (records only: one call)
    torch     the batch without it: one vx_read_region into device memory per box, then a batched flood in torch on the context's stream --
              shifted ORs over an [N, z, y, x] bool tensor, stepping until no frontier is left (one .any() read back a step) or max_steps --
              with the step counts written into a uint8 field, or -- records only -- the reached cells counted. Measured where N * voxels
              <= 2^25 (the bool tensors of a larger batch, and its thousands of vx_read_region calls, are not what a caller would do in one
              go); elsewhere the row says so.
    call_sync_us      the host clock around one batch (all its calls) and the vx_sync behind it
    device_event_us   flood only: HIP-event time per batch over a queue of batches on the context's stream
    torch_over_flood  torch's median call_sync_us over the flood's: above 1 vx_flood_points wins, below 1 it loses
The fields (records only: the reached counts) of the two ways are compared query for query before anything is timed. At N = 1 every figure is
the latency of one launch and one wait, not throughput. Each format runs in a child process of its own under `timeout`; the driver stops at
the first that fails. Medians after warm-up, with the 10th and 90th percentiles beside them. There is no threshold."""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REPS, WARMUP = 10, 3
TORCH_REPS, TORCH_WARMUP = 5, 2
FIELD_BYTES_A_CALL = 1 << 24
TORCH_CELLS = 1 << 25


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
    rng = np.random.default_rng(6)
    side = 512
    height = svo.scan_columns((gx - side // 2, 0, gz - side // 2), (side, 1 << depth, side), hip.VX_DIR_NEG_Y, device=True)
    svo.sync()
    top = height[:, :, 0].clamp(min=-1).to(torch.float32) + 1.0
    zz, xx = torch.meshgrid(torch.arange(side, device="cuda"), torch.arange(side, device="cuda"), indexing="ij")
    standing = torch.stack([xx.to(torch.float32) + (gx - side // 2) + 0.5, top + 1.5, zz.to(torch.float32) + (gz - side // 2) + 0.5], dim=-1).reshape(-1, 3)
    standing = standing[torch.from_numpy(rng.permutation(side * side)[:65536]).cuda()].contiguous()

    for side_cells in (9, 17, 32):
        shape = (side_cells,) * 3
        seed_at = (side_cells // 2,) * 3
        voxels = side_cells ** 3
        stride = (voxels + 15) // 16 * 16
        for n in (1, 64, 4096, 65536):
            pos = standing[:n].contiguous()
            a_call = max(FIELD_BYTES_A_CALL // stride, 1)
            fields = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
            info = torch.empty((n, 4), dtype=torch.int32, device="cuda")
            seeds = torch.floor(pos).to(torch.int32).cpu().numpy() - np.int32(seed_at)
            with_torch = n * voxels <= TORCH_CELLS
            regions = torch.empty((n,) + shape, dtype=torch.int32, device="cuda") if with_torch else None
            lo3s = [(C.c_int32 * 3)(*(int(v) for v in seeds[i])) for i in range(n)] if with_torch else []
            size3 = (C.c_uint32 * 3)(*shape)
            for max_steps in (15, 250):
                for want_fields in (True, False):
                    def flood():
                        if not want_fields:
                            svo.flood_points(pos, shape, seed_at, max_steps, fields=None, info=info)
                            return
                        for at in range(0, n, a_call):
                            svo.flood_points(pos[at:at + a_call], shape, seed_at, max_steps, fields=fields[at:at + a_call], info=info[at:at + a_call])

                    result = {}

                    def by_torch():
                        for i in range(n):
                            assert L.vx_read_region(h, C.byref(lo3s[i]), C.byref(size3), hip.VX_MEM_DEVICE, hip._vp(regions[i].data_ptr())) == 0
                        with torch.cuda.stream(stream):
                            passable = regions == 0
                            frontier = torch.zeros_like(passable)
                            frontier[:, seed_at[2], seed_at[1], seed_at[0]] = passable[:, seed_at[2], seed_at[1], seed_at[0]]
                            reached = frontier.clone()
                            field = None
                            if want_fields:
                                field = torch.where(passable, 0xFE, 0xFF).to(torch.uint8)
                                field[frontier] = 0
                            for step in range(1, max_steps + 1):
                                grow = torch.zeros_like(frontier)
                                grow[:, 1:] |= frontier[:, :-1]
                                grow[:, :-1] |= frontier[:, 1:]
                                grow[:, :, 1:] |= frontier[:, :, :-1]
                                grow[:, :, :-1] |= frontier[:, :, 1:]
                                grow[:, :, :, 1:] |= frontier[:, :, :, :-1]
                                grow[:, :, :, :-1] |= frontier[:, :, :, 1:]
                                grow &= passable & ~reached
                                if not bool(grow.any()):  # (reads one byte back: the stream is waited for)
                                    break
                                reached |= grow
                                if want_fields:
                                    field.masked_fill_(grow, step)
                                frontier = grow
                            result["reached"] = reached.sum(dim=(1, 2, 3), dtype=torch.int32)
                            result["field"] = field

                    torch.cuda.synchronize()  # (what torch has prepared on its own stream is there before the context's stream reads it)
                    flood()
                    svo.sync()
                    got_reached = info[:, 0].clone()
                    if with_torch:
                        by_torch()
                        svo.sync()
                        assert torch.equal(got_reached, result["reached"]), "vx_flood_points and the torch flood disagree on the reached cells"
                        if want_fields:
                            assert torch.equal(fields[:, :voxels], result["field"].reshape(n, -1)), "vx_flood_points and the torch flood disagree on a field"
                    calls = (n + a_call - 1) // a_call if want_fields else 1
                    queue = 20 if n * voxels < (1 << 24) else 3
                    row = {"format": fmt, "call": "vx_flood_points", "queries": n, "shape": list(shape), "max_steps": max_steps, "outputs": "fields+info" if want_fields else "info",
                           "calls_a_batch": calls, "reached_mean": round(float(got_reached.to(torch.float64).mean().item()), 1),
                           "farthest_max": int(info[:, 1].max().item()), "flood": {"call_sync_us": call_sync(flood), "device_event_us": event(flood, queue)}}
                    if with_torch:
                        row["torch"] = {"call_sync_us": call_sync(by_torch, TORCH_REPS, TORCH_WARMUP)}
                        row["torch_over_flood"] = round(row["torch"]["call_sync_us"]["median"] / row["flood"]["call_sync_us"]["median"], 2)
                    else:
                        row["torch"] = "not measured: N * voxels exceeds 2^25"
                    print(json.dumps(row), flush=True)
    svo.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", metavar="FORMAT")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "flood" / "results.json"))
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
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": "MI355X (gfx950)", "scene": "heightfield depth 12 (bench.py's C3 world)", "unit": "microseconds per batch",
                                          "repeats": REPS, "torch_repeats": TORCH_REPS, "cases": results}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
