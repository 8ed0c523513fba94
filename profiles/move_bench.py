"""A batch of float boxes moved through the world, microseconds per call: vx_move_boxes beside what a caller did before it.

    python profiles/move_bench.py [--out profiles/move/results.json] [--formats esvo,csvo]

On the depth-12 bench world (bench.py's C3 scene), device memory throughout. The workloads:
    step      N = 1, 256, 4,096 and 262,144 boxes of extents (0.8, 1.8, 0.8) standing on the terrain's surface around the C3 camera's
              look-at point (the surface from vx_scan_columns, as profiles/boxes_bench.py takes it), each with a motion of (0.1, -0.2, 0.05)
    far       the same boxes with a motion of length 8
    cube8     4,096 boxes of 8^3 centred on points of that surface, moving 16
    sky       4,096 boxes of (0.8, 1.8, 0.8) in open sky high above it: every brick ends in empty space
Beside each:
    move      vx_move_boxes: one launch, one wave a box, order y, x, z, skin 2^-10
    overlap   the batch without it, three passes: per pass the swept box (from the integer plane at or beyond the leading face to the face's
              end position plus the skin) by torch arithmetic on the context's stream, one vx_overlap_boxes, then `moved` from its lo / hi and
              the box's new position by torch arithmetic again: three launches of the kernel and the launches of torch between them. It
              yields moved and the contacts, not the stopping voxel's value.
    call_sync_us      the host clock around one call (overlap: all its steps) and the vx_sync behind it
    device_event_us   HIP-event time per call over a queue of calls on the context's stream
    overlap_over_move   the other way's median over this call's, per clock: above 1 this call wins, below 1 it loses
`moved` and `contacts` of the two ways are compared box for box before anything is timed. At N = 1 every figure is the latency of one launch
and one wait, not throughput. Each format runs in a child process of its own under `timeout`; the driver stops at the first that fails.
Medians after warm-up, with the 10th and 90th percentiles beside them. There is no threshold."""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REPS, WARMUP = 20, 5
SKIN = 2.0 ** -10
ORDER_AXES = (1, 0, 2)  # VX_MOVE_ORDER_YXZ


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
    L, h = hip.lib(), svo._h
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
    standing = torch.stack([xx.to(torch.float32) + (gx - side // 2) + 0.1, top, zz.to(torch.float32) + (gz - side // 2) + 0.1], dim=-1).reshape(-1, 3)
    standing = standing[torch.from_numpy(rng.permutation(side * side)).cuda()].contiguous()
    dev = lambda v: torch.tensor(v, dtype=torch.float32, device="cuda")
    person, step = dev([0.8, 1.8, 0.8]), dev([0.1, -0.2, 0.05])
    far = dev((np.float64([0.5, -0.6, 0.62]) / np.linalg.norm([0.5, -0.6, 0.62]) * 8.0).tolist())
    sixteen = dev((np.float64([0.55, -0.6, 0.58]) / np.linalg.norm([0.55, -0.6, 0.58]) * 16.0).tolist())
    sky = torch.from_numpy((np.float64([ground[0], min(h_max + 600.0, size - 200.0), ground[2]]) + rng.uniform(-50.0, 50.0, (4096, 3))).astype(np.float32)).cuda()
    workloads = [("step", standing[:n].contiguous(), person, step) for n in (1, 256, 4096, side * side)]
    workloads += [("far", standing[:n].contiguous(), person, far) for n in (1, 256, 4096, side * side)]
    workloads += [("cube8", (standing[8192:8192 + 4096] - 4.0).contiguous(), dev([8.0, 8.0, 8.0]), sixteen), ("sky", sky, person, step)]

    for name, origin, extents, motion in workloads:
        n = int(origin.shape[0])
        out = torch.empty((n, 12), dtype=torch.int32, device="cuda")
        hits = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        swept_mn, swept_ext = torch.empty((n, 3), dtype=torch.float32, device="cuda"), torch.empty((n, 3), dtype=torch.float32, device="cuda")
        mn, moved, contacts = origin.clone(), torch.zeros((n, 3), dtype=torch.float32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
        d3 = [float(v) for v in motion.cpu()]

        def move():
            svo.move_boxes(origin, extents, motion, skin=SKIN, out=out)

        def overlap():
            with torch.cuda.stream(stream):
                mn.copy_(origin)
                moved.zero_()
                contacts.zero_()
            for a in ORDER_AXES:
                d = d3[a]
                if d == 0.0:
                    continue
                with torch.cuda.stream(stream):
                    face = mn[:, a] + extents[a] if d > 0 else mn[:, a]
                    end = face + ((d + SKIN) if d > 0 else (d - SKIN))
                    plane = torch.ceil(face) if d > 0 else torch.floor(face)
                    swept_mn.copy_(mn)
                    swept_ext.copy_(extents.expand(n, 3))
                    swept_mn[:, a] = plane if d > 0 else end
                    reach = end - plane if d > 0 else plane - end  # (not above 0: no layer ahead, no box, nothing found)
                    if d < 0:  # end + reach may round to just above the plane, and the layer the box stands in would count: one step shorter then
                        reach = torch.where(end + reach > plane, torch.nextafter(reach, torch.zeros_like(reach)), reach)
                    swept_ext[:, a] = reach
                svo.overlap_boxes(swept_mn, swept_ext, out=hits)
                with torch.cuda.stream(stream):
                    found = (hits[:, 0] > 0) & (hits[:, 0] != -1)
                    gap = (hits[:, 2 + a].to(torch.float32) - face) if d > 0 else (face - hits[:, 5 + a].to(torch.float32))
                    room = torch.clamp(gap - SKIN, min=0.0)
                    m = torch.where(found, torch.clamp(room, max=abs(d)) * (1.0 if d > 0 else -1.0), torch.full_like(room, d))
                    moved[:, a] = m
                    mn[:, a] += m
                    contacts.bitwise_or_(found.to(torch.int32) << (2 * a + (1 if d > 0 else 0)))

        torch.cuda.synchronize()  # (what torch has prepared on its own stream is there before the context's stream reads it)
        move()
        overlap()
        svo.sync()
        rec = out.view(torch.float32)
        assert torch.equal(rec[:, 3:6], moved), "vx_move_boxes and the three passes of vx_overlap_boxes disagree on `moved`"
        assert torch.equal(out[:, 6], contacts), "vx_move_boxes and the three passes of vx_overlap_boxes disagree on `contacts`"
        queue = 20 if n <= 4096 else 3
        rows = {"move": move, "overlap": overlap}
        timed = {k: {"call_sync_us": call_sync(fn), "device_event_us": event(fn, queue)} for k, fn in rows.items()}
        row = {"format": fmt, "call": "vx_move_boxes", "workload": name, "boxes_n": n, "extents": [float(v) for v in extents.cpu()], "motion": [round(v, 4) for v in d3],
               "with_contact": int((contacts != 0).sum().item()), "stopped_short": int((moved != motion).any(dim=1).sum().item()), **timed}
        row["overlap_over_move"] = {c: round(timed["overlap"][c]["median"] / timed["move"][c]["median"], 2) for c in ("call_sync_us", "device_event_us")}
        print(json.dumps(row), flush=True)
    svo.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", metavar="FORMAT")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "move" / "results.json"))
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
