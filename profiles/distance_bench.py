"""The squared distance to the nearest block, per cell, in many boxes, microseconds per batch: vx_distance_boxes beside what a caller could do
before it.

    python profiles/distance_bench.py [--out profiles/distance/results.json] [--formats esvo,csvo]

On the depth-12 bench world (bench.py's C3 scene), device memory throughout. The boxes are centred on the terrain's surface around the C3
camera's look-at point (the surface comes from vx_scan_columns, VX_DIR_NEG_Y, over 512 x 512 columns). Every solid cell is a target, no pass
value, no flag.
    shapes    9^3, 17^3 and 32^3 cells
    counts    with fields 1, 64 and as many boxes as one call may write (2^24 bytes): 11,397 of 9^3, 1,705 of 17^3, 256 of 32^3; records only
              1, 64 and 4,096
    outputs   fields and records, or records only
Beside each:
    distance  vx_distance_boxes: one call, one workgroup a box
    torch     the batch without it: per box one vx_read_region into device memory, then on the context's stream the same separable
              transform as batched torch operations over [N, z, y, x]: 0 at a target and a large number elsewhere, then along x, y and z
              the minimum over j of d[j] + (i - j)^2 as one broadcast add and one amin, a few boxes at a time where the broadcast would
              not fit. A launch a box plus torch's.
    call_sync_us      the host clock around one batch and the vx_sync behind it
    device_event_us   distance only: HIP-event time per batch over a queue of batches on the context's stream
    torch_over_distance  torch's median call_sync_us over the distance call's: above 1 vx_distance_boxes wins, below 1 it loses
The two ways' fields are compared box for box before anything is timed. At N = 1 every figure is the latency of one launch and one wait, not
throughput. Each format runs in a child process of its own under `timeout`; the driver stops at the first that fails. Medians after warm-up,
with the 10th and 90th percentiles beside them. There is no threshold."""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REPS, WARMUP = 10, 3
TORCH_REPS, TORCH_WARMUP = 5, 2
MOST = 4096
LARGEST = (1 << 24) // ((2 * 9 ** 3 + 15) // 16 * 16)  # boxes of 9^3 with fields: the most a row asks for


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
    picks = rng.permutation(side * side)[:LARGEST]
    centres = np.stack([picks % side + (gx - side // 2), top.reshape(-1)[picks], picks // side + (gz - side // 2)], axis=1)
    info_all = torch.empty((LARGEST, 4), dtype=torch.int32, device="cuda")
    FAR = 1 << 20
    ramp = torch.arange(32, dtype=torch.int32, device="cuda")
    squares = (ramp[:, None] - ramp[None, :]) ** 2  # [i, j]

    def min_plus(d, axis):
        """out[.., i, ..] = min_j(d[.., j, ..] + (i - j)^2) along `axis` of [N, z, y, x]; at most 2^26 sums at a time"""
        d = d.movedim(axis, -1)
        n = d.shape[-1]
        out = torch.empty_like(d)
        step = max(1, (1 << 26) // (d[0].numel() * n))
        for k in range(0, d.shape[0], step):
            out[k:k + step] = (d[k:k + step].unsqueeze(-2) + squares[:n, :n]).amin(dim=-1)
        return out.movedim(-1, axis)

    for side_cells in (9, 17, 32):
        shape = (side_cells,) * 3
        voxels = side_cells ** 3
        stride = (2 * voxels + 15) // 16 * 16
        for want_fields in (True, False):
            for asked in (1, 64, MOST):
                n = (1 << 24) // stride if want_fields and asked == MOST else asked
                los = (centres[:n] - side_cells // 2).astype(np.int32)
                lo = torch.from_numpy(los).cuda()
                fields = torch.empty((n, stride // 2), dtype=torch.int16, device="cuda") if want_fields else False
                info = info_all[:n]
                result = {}

                def distance():
                    svo.distance_boxes(lo, shape, fields=fields, info=info)

                torch.cuda.synchronize()  # (what torch has prepared on its own stream is there before the context's stream reads it)
                distance()
                svo.sync()
                records = hip.distance_infos_to_numpy(info)
                row = {"format": fmt, "call": "vx_distance_boxes", "boxes": n, "shape": list(shape), "outputs": "fields+info" if want_fields else "info",
                       "targets_mean": round(float(records["targets"].mean()), 1), "farthest_mean": round(float(records["farthest"].mean()), 1),
                       "no_target": int((records["targets"] == 0).sum())}
                if want_fields:
                    regions = torch.empty((n,) + shape, dtype=torch.int32, device="cuda")
                    lo3s = [(C.c_int32 * 3)(*(int(v) for v in los[i])) for i in range(n)]
                    size3 = (C.c_uint32 * 3)(*shape)

                    def by_torch():
                        for i in range(n):
                            assert L.vx_read_region(h, C.byref(lo3s[i]), C.byref(size3), hip.VX_MEM_DEVICE, hip._vp(regions[i].data_ptr())) == 0
                        with torch.cuda.stream(stream):
                            d = torch.where(regions != 0, 0, FAR).to(torch.int32)  # [N, z, y, x]
                            for axis in (3, 2, 1):
                                d = min_plus(d, axis)
                            result["field"] = torch.where(d >= FAR, hip.VX_DISTANCE_NONE, d)

                    by_torch()
                    svo.sync()
                    cells = fields[:, :voxels].to(torch.int32) & 0xFFFF
                    assert torch.equal(cells.reshape((n,) + shape), result["field"].to(torch.int32)), "the two ways disagree on a field"
                row["distance"] = {"call_sync_us": call_sync(distance), "device_event_us": event(distance, 20 if n * voxels < (1 << 22) else 4)}
                if want_fields:
                    row["torch"] = {"call_sync_us": call_sync(by_torch, TORCH_REPS, TORCH_WARMUP)}
                    row["torch_over_distance"] = round(row["torch"]["call_sync_us"]["median"] / row["distance"]["call_sync_us"]["median"], 2)
                else:
                    row["torch"] = "not measured: the baseline computes every cell whatever is wanted of the field"
                print(json.dumps(row), flush=True)
    svo.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", metavar="FORMAT")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "distance" / "results.json"))
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
                                          "repeats": REPS, "torch_repeats": TORCH_REPS, "pass_value": 0, "match_value": 0, "flags": 0, "cases": results},
                                         indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
