"""The blocks of a box as a compact list, microseconds per call: vx_list_region beside what a caller did before it.

    python profiles/list_bench.py [--out profiles/list/results.json] [--formats esvo,csvo]

On the depth-12 bench world (bench.py's C3 scene), device memory throughout: boxes of 64^3, 128^3 and 256^3 voxels centred on the C3 camera's
look-at point in the terrain (`terrain`), and 256^3 of open sky high above it (`sky`: every brick ends in empty space, the list is empty), on
the brick grid; flags 0 and VX_LIST_EXPOSED.
    list      vx_list_region into a buffer of exactly the list's length (counted by a call with capacity 0 beforehand, outside the timing):
              three launches.
    dense     the same answer without it: vx_read_region into device memory, torch.nonzero and a gather of the ids (torch.nonzero waits for
              the device to learn its result's length: that wait is part of what the caller pays, in both clocks). For VX_LIST_EXPOSED:
              vx_read_region of the box padded by one voxel -- 258^3 exceeds a call's 2^24 voxels, so two calls, one z-slab each --, six
              shifted compares for the face bits, then nonzero and the gathers.
    call_sync_us      the host clock around one call (dense: all its steps) and the vx_sync behind it
    device_event_us   HIP-event time per call over a queue of calls on the context's stream
    out_bytes         what the caller is left holding: 8 bytes a record and the count; for dense the box's 4 bytes a voxel (padded box
                      for VX_LIST_EXPOSED) besides the compacted index and id arrays
    dense_over_list   dense's median over the list's, per clock: above 1 the list wins
The two answers are compared record for record (sorted by index) before anything is timed. Each format runs in a child process of its own
under `timeout`; the driver stops at the first that fails. Medians after warm-up, with the 10th and 90th percentiles beside them. There is
no threshold."""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REPS, WARMUP = 20, 5


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

    def read_into(t, lo, shape):
        """vx_read_region of the box into the dense tensor t ([z][y][x]), a z-slab a call where the box exceeds 2^24 voxels"""
        sz, sy, sx = shape
        slab = max(1, min(sz, (1 << 24) // (sy * sx)))
        for z0 in range(0, sz, slab):
            n = min(slab, sz - z0)
            lo3, size3 = (C.c_int32 * 3)(lo[0], lo[1], lo[2] + z0), (C.c_uint32 * 3)(sx, sy, n)
            assert L.vx_read_region(h, C.byref(lo3), C.byref(size3), hip.VX_MEM_DEVICE, _vp(t[z0].data_ptr())) == 0

    look = np.float64([0.6, -0.35, 0.7])
    ground = eye + look * ((eye[1] - 0.5 * h_max) / 0.35)
    sky = np.float64([ground[0], min(h_max + 600.0, size - 200.0), ground[2]])
    for where, centre, s in (("terrain", ground, 64), ("terrain", ground, 128), ("terrain", ground, 256), ("sky", sky, 256)):
        lo = tuple(int(v) // 8 * 8 - s // 2 for v in centre)
        lo3, size3 = (C.c_int32 * 3)(*lo), (C.c_uint32 * 3)(s, s, s)
        dense = torch.empty((s, s, s), dtype=torch.int32, device="cuda")
        padded = torch.empty((s + 2, s + 2, s + 2), dtype=torch.int32, device="cuda")
        for flags in (0, hip.VX_LIST_EXPOSED):
            d_total = torch.zeros(1, dtype=torch.int32, device="cuda")
            assert L.vx_list_region(h, C.byref(lo3), C.byref(size3), flags, hip.VX_MEM_DEVICE, None, 0, _vp(d_total.data_ptr())) == 0 and L.vx_sync(h) == 0
            total = int(d_total.item())
            d_out = torch.empty((max(total, 1), 2), dtype=torch.int32, device="cuda")

            def listed():
                assert L.vx_list_region(h, C.byref(lo3), C.byref(size3), flags, hip.VX_MEM_DEVICE, _vp(d_out.data_ptr()), total, _vp(d_total.data_ptr())) == 0

            def by_hand():
                with torch.cuda.stream(stream):
                    if not flags:
                        read_into(dense, lo, (s, s, s))
                        flat = dense.reshape(-1)
                        at = torch.nonzero(flat).reshape(-1)
                        return at, flat[at]
                    read_into(padded, tuple(v - 1 for v in lo), (s + 2, s + 2, s + 2))
                    air = padded == 0
                    m = slice(1, -1)
                    faces = torch.zeros((s, s, s), dtype=torch.int32, device="cuda")
                    for f, side in enumerate((air[m, m, :-2], air[m, m, 2:], air[m, :-2, m], air[m, 2:, m], air[:-2, m, m], air[2:, m, m])):
                        faces |= side.to(torch.int32) << f
                    core = padded[m, m, m]
                    at = torch.nonzero(((core != 0) & (faces != 0)).reshape(-1)).reshape(-1)
                    return at | (faces.reshape(-1)[at].long() << 24), core.reshape(-1)[at]

            listed()
            L.vx_sync(h)
            want_where, want_value = by_hand()
            L.vx_sync(h)
            assert int(d_total.item()) == total == len(want_where), "the list's length and the dense answer's disagree"
            if total:
                got_where, got_value = d_out[:total, 0].long(), d_out[:total, 1]
                order = torch.argsort(got_where & 0xFFFFFF)
                assert torch.equal(got_where[order], want_where) and torch.equal(got_value[order], want_value), "the list and the dense answer disagree"
            queue = 20 if s < 256 else 5
            rows = {"list": (listed, 8 * total + 4), "dense": (by_hand, 4 * (s + 2 * bool(flags)) ** 3 + 12 * total)}
            timed = {k: {"call_sync_us": call_sync(fn), "device_event_us": event(fn, queue), "out_bytes": nbytes} for k, (fn, nbytes) in rows.items()}
            row = {"format": fmt, "call": "vx_list_region", "where": where, "box": s, "lo": list(lo), "flags": flags, "records": total, "voxels": s ** 3, **timed,
                   "dense_over_list": {k: round(timed["dense"][k]["median"] / timed["list"][k]["median"], 2) for k in ("call_sync_us", "device_event_us")}}
            print(json.dumps(row), flush=True)
    svo.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", metavar="FORMAT")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "list" / "results.json"))
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
