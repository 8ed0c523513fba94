"""Sky and block light levels for many boxes, microseconds per batch: vx_light_boxes beside what a caller could do before it.

    python profiles/light_bench.py [--out profiles/light/results.json] [--formats esvo,csvo]

On the depth-12 bench world (bench.py's C3 scene), device memory throughout. The boxes are centred on the terrain's surface around the C3
camera's look-at point (the surface comes from vx_scan_columns, VX_DIR_NEG_Y, over 512 x 512 columns). The props: grass (1) opaque and dark,
dirt (2) emits 12, stone (3) opaque and dark -- no transparent block, so that the baseline's one scan a box is the whole exposure test.
    counts    1, 64 and 151 boxes (151 boxes of 48^3 are what one call may write of fields; 46^3 is a 16^3 section with its margin of 15)
    shapes    16^3, 32^3 and 46^3 cells
    outputs   fields and records, or records only
Beside each:
    light     vx_light_boxes: one call, one workgroup a box
    torch     the batch without it: per box one vx_read_region into device memory and one vx_scan_columns (VX_DIR_POS_Y) over the box's
              footprint from its top to the world's top, then on the context's stream a batched fixed-point iteration in torch over
              [2, N, z, y, x] levels -- both channels at once, 14 times "the largest of the six neighbours less one, or the cell's own source
              level", with no read-back -- and the bytes put together. Three launches a box plus a few hundred of torch's.
    call_sync_us      the host clock around one batch and the vx_sync behind it
    device_event_us   light only: HIP-event time per batch over a queue of batches on the context's stream
    torch_over_light  torch's median call_sync_us over the light call's: above 1 vx_light_boxes wins, below 1 it loses
The fields of the two ways are compared box for box before anything is timed. At N = 1 every figure is the latency of one launch and one
wait, not throughput. Each format runs in a child process of its own under `timeout`; the driver stops at the first that fails. Medians after
warm-up, with the 10th and 90th percentiles beside them. There is no threshold."""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REPS, WARMUP = 10, 3
TORCH_REPS, TORCH_WARMUP = 5, 2
PROPS = [0, 0, 12, 0]


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
    top = height[:, :, 0].clamp(min=-1).cpu().numpy().astype(np.int64) + 1  # [z][x]: the first air cell of each column
    picks = rng.permutation(side * side)[:151]
    centres = np.stack([picks % side + (gx - side // 2), top.reshape(-1)[picks], picks // side + (gz - side // 2)], axis=1)
    props = np.array(PROPS, dtype=np.uint8)
    emits = torch.tensor([p & 15 for p in PROPS], dtype=torch.int16, device="cuda")
    world_top = 1 << depth

    for side_cells in (16, 32, 46):
        shape = (side_cells,) * 3
        voxels = side_cells ** 3
        stride = (voxels + 15) // 16 * 16
        for n in (1, 64, 151):
            los = (centres[:n] - side_cells // 2).astype(np.int32)
            lo = torch.from_numpy(los).cuda()
            fields = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
            info = torch.empty((n, 4), dtype=torch.int32, device="cuda")
            regions = torch.empty((n,) + shape, dtype=torch.int32, device="cuda")
            above = torch.empty((n, side_cells, side_cells, 4), dtype=torch.int32, device="cuda")  # vx_scan_hit records, [z][x]
            lo3s = [(C.c_int32 * 3)(*(int(v) for v in los[i])) for i in range(n)]
            up3s = [(C.c_int32 * 3)(int(los[i][0]), int(los[i][1]) + side_cells, int(los[i][2])) for i in range(n)]
            up_sizes = [(C.c_uint32 * 3)(side_cells, world_top - (int(los[i][1]) + side_cells), side_cells) for i in range(n)]
            size3 = (C.c_uint32 * 3)(*shape)
            result = {}

            def by_torch():
                for i in range(n):
                    assert L.vx_read_region(h, C.byref(lo3s[i]), C.byref(size3), hip.VX_MEM_DEVICE, hip._vp(regions[i].data_ptr())) == 0
                    assert L.vx_scan_columns(h, C.byref(up3s[i]), C.byref(up_sizes[i]), hip.VX_DIR_POS_Y, hip.VX_MEM_DEVICE, hip._vp(above[i].data_ptr())) == 0
                with torch.cuda.stream(stream):
                    passable = regions == 0  # [N, z, y, x]
                    open_above = above[:, :, :, 0] == hip.VX_SCAN_NONE  # [N, z, x]
                    closed = (~passable).flip(2).cumsum(2).flip(2) > 0  # an impassable cell at or above, inside the box
                    exposed = passable & ~closed & open_above[:, :, None, :]
                    own = torch.stack([torch.where(exposed, 15, 0).to(torch.int16), emits[regions.clamp(max=len(PROPS) - 1).long()]])  # [2, N, z, y, x]
                    level = own.clone()
                    for _ in range(14):
                        around = torch.zeros_like(level)
                        around[:, :, 1:] = torch.maximum(around[:, :, 1:], level[:, :, :-1])
                        around[:, :, :-1] = torch.maximum(around[:, :, :-1], level[:, :, 1:])
                        around[:, :, :, 1:] = torch.maximum(around[:, :, :, 1:], level[:, :, :, :-1])
                        around[:, :, :, :-1] = torch.maximum(around[:, :, :, :-1], level[:, :, :, 1:])
                        around[:, :, :, :, 1:] = torch.maximum(around[:, :, :, :, 1:], level[:, :, :, :, :-1])
                        around[:, :, :, :, :-1] = torch.maximum(around[:, :, :, :, :-1], level[:, :, :, :, 1:])
                        level = torch.where(passable[None], torch.maximum(own, (around - 1).clamp(min=0)), own)
                    result["field"] = (level[0] << 4 | level[1]).to(torch.uint8)

            for want_fields in (True, False):
                def light():
                    svo.light_boxes(lo, shape, props, fields=fields if want_fields else False, info=info)

                torch.cuda.synchronize()  # (what torch has prepared on its own stream is there before the context's stream reads it)
                light()
                svo.sync()
                row = {"format": fmt, "call": "vx_light_boxes", "boxes": n, "shape": list(shape), "outputs": "fields+info" if want_fields else "info",
                       "lit_mean": round(float(info[:, 0].to(torch.float64).mean().item()), 1), "sources_mean": round(float(info[:, 1].to(torch.float64).mean().item()), 1),
                       "open_columns_mean": round(float(info[:, 2].to(torch.float64).mean().item()), 1)}
                if want_fields:
                    by_torch()
                    svo.sync()
                    assert torch.equal(fields[:, :voxels], result["field"].reshape(n, -1)), "vx_light_boxes and the torch iteration disagree on a field"
                row["light"] = {"call_sync_us": call_sync(light), "device_event_us": event(light, 20 if n * voxels < (1 << 22) else 4)}
                if want_fields:
                    row["torch"] = {"call_sync_us": call_sync(by_torch, TORCH_REPS, TORCH_WARMUP)}
                    row["torch_over_light"] = round(row["torch"]["call_sync_us"]["median"] / row["light"]["call_sync_us"]["median"], 2)
                else:
                    row["torch"] = "not measured: the baseline computes the fields whatever is wanted of them"
                print(json.dumps(row), flush=True)
    svo.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", metavar="FORMAT")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "light" / "results.json"))
    ap.add_argument("--formats", default="esvo,csvo")
    ap.add_argument("--timeout", type=int, default=240)
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
                                          "repeats": REPS, "torch_repeats": TORCH_REPS, "props": PROPS, "cases": results}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
