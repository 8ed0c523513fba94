"""The loose pieces of the blocks in many boxes, microseconds per batch: vx_label_boxes beside what a caller could do before it.

    python profiles/label_bench.py [--out profiles/label/results.json] [--formats esvo,csvo]

On the depth-12 bench world (bench.py's C3 scene), device memory throughout. The boxes are centred on the terrain's surface around the C3
camera's look-at point (the surface comes from vx_scan_columns, VX_DIR_NEG_Y, over 512 x 512 columns). Every face anchors, max_pieces 250,
max_steps 4,096, no pass value.
    shapes    9^3, 17^3 and 32^3 cells
    counts    1, 64 and 4,096 boxes -- with fields as many of the 4,096 as one call may write (2^24 bytes): 3,404 boxes of 17^3, 512 of 32^3
    outputs   fields, piece records and records, or piece records and records only
Beside each:
    label     vx_label_boxes: one call, one workgroup a box
    torch     the batch without it: per box one vx_read_region into device memory, then on the context's stream a batched labelling in torch
              over [N, z, y, x]: every solid cell starts with its own number, the cells on the anchor faces with 0, and "the least of the cell
              and its six neighbours" over shifted views is repeated to the fixed point (looked for every 8 rounds, with a read-back). A launch a
              box plus torch's.
    call_sync_us      the host clock around one batch and the vx_sync behind it
    device_event_us   label only: HIP-event time per batch over a queue of batches on the context's stream
    torch_over_label  torch's median call_sync_us over the label call's: above 1 vx_label_boxes wins, below 1 it loses
The two ways' held / loose partition is compared cell for cell, and the sizes of the pieces box for box, before anything is timed. At N = 1
every figure is the latency of one launch and one wait, not throughput. Each format runs in a child process of its own under `timeout`; the
driver stops at the first that fails. Medians after warm-up, with the 10th and 90th percentiles beside them. There is no threshold."""
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
    picks = rng.permutation(side * side)[:MOST]
    centres = np.stack([picks % side + (gx - side // 2), top.reshape(-1)[picks], picks // side + (gz - side // 2)], axis=1)
    pieces_all = torch.empty((MOST, hip.VX_LABEL_MAX_PIECES, 4), dtype=torch.int32, device="cuda")
    info_all = torch.empty((MOST, 8), dtype=torch.int32, device="cuda")
    INF = 1 << 30

    for side_cells in (9, 17, 32):
        shape = (side_cells,) * 3
        voxels = side_cells ** 3
        stride = (voxels + 15) // 16 * 16
        on_face = torch.zeros(shape, dtype=torch.bool, device="cuda")
        on_face[0] = on_face[-1] = on_face[:, 0] = on_face[:, -1] = on_face[:, :, 0] = on_face[:, :, -1] = True
        own = torch.arange(1, voxels + 1, dtype=torch.int32, device="cuda").reshape(shape)
        for want_fields in (True, False):
            for asked in (1, 64, MOST):
                n = min(asked, (1 << 24) // stride) if want_fields else asked
                los = (centres[:n] - side_cells // 2).astype(np.int32)
                lo = torch.from_numpy(los).cuda()
                fields = torch.empty((n, stride), dtype=torch.uint8, device="cuda") if want_fields else False
                pieces, info = pieces_all[:n], info_all[:n]
                result = {}

                def label():
                    svo.label_boxes(lo, shape, fields=fields, pieces=pieces, info=info)

                torch.cuda.synchronize()  # (what torch has prepared on its own stream is there before the context's stream reads it)
                label()
                svo.sync()
                records = hip.label_infos_to_numpy(info)
                row = {"format": fmt, "call": "vx_label_boxes", "boxes": n, "shape": list(shape), "outputs": "fields+pieces+info" if want_fields else "pieces+info",
                       "solid_mean": round(float(records["solid"].mean()), 1), "held_mean": round(float(records["held"].mean()), 1),
                       "pieces_mean": round(float(records["pieces"].mean()), 3), "steps_mean": round(float(records["steps"].mean()), 1),
                       "cut": int((records["flags"] & hip.VX_LABEL_CUT != 0).sum())}
                if want_fields:
                    regions = torch.empty((n,) + shape, dtype=torch.int32, device="cuda")
                    lo3s = [(C.c_int32 * 3)(*(int(v) for v in los[i])) for i in range(n)]
                    size3 = (C.c_uint32 * 3)(*shape)

                    def by_torch():
                        for i in range(n):
                            assert L.vx_read_region(h, C.byref(lo3s[i]), C.byref(size3), hip.VX_MEM_DEVICE, hip._vp(regions[i].data_ptr())) == 0
                        with torch.cuda.stream(stream):
                            solid = regions != 0  # [N, z, y, x]
                            lab = torch.where(solid, torch.where(on_face, 0, own), INF)
                            for rounds in range(1, 1 << 15):
                                least = lab.clone()
                                least[:, 1:] = torch.minimum(least[:, 1:], lab[:, :-1])
                                least[:, :-1] = torch.minimum(least[:, :-1], lab[:, 1:])
                                least[:, :, 1:] = torch.minimum(least[:, :, 1:], lab[:, :, :-1])
                                least[:, :, :-1] = torch.minimum(least[:, :, :-1], lab[:, :, 1:])
                                least[:, :, :, 1:] = torch.minimum(least[:, :, :, 1:], lab[:, :, :, :-1])
                                least[:, :, :, :-1] = torch.minimum(least[:, :, :, :-1], lab[:, :, :, 1:])
                                least = torch.where(solid, least, INF)
                                done = rounds % 8 == 0 and torch.equal(least, lab)  # (a read-back: the fixed point is looked for every 8 rounds)
                                lab = least
                                if done:
                                    break
                            result["label"], result["solid"], result["rounds"] = lab, solid, rounds

                    by_torch()
                    svo.sync()
                    cells = fields[:, :voxels].reshape((n,) + shape)
                    assert torch.equal(cells == hip.VX_LABEL_HELD, result["solid"] & (result["label"] == 0)), "the two ways disagree on the held cells"
                    assert torch.equal(cells != hip.VX_LABEL_AIR, result["solid"]), "the two ways disagree on the solid cells"
                    labels, got = result["label"].cpu().numpy().reshape(n, -1), hip.label_pieces_to_numpy(pieces)
                    for k in np.flatnonzero(records["more"] == 0):  # (every piece of the box has a record: the sizes can be compared)
                        loose = labels[k][(labels[k] > 0) & (labels[k] < INF)]
                        sizes = sorted(np.unique(loose, return_counts=True)[1].tolist())
                        assert sizes == sorted(got[k]["cells"][got[k]["cells"] > 0].tolist()), f"the two ways disagree on the pieces of box {k}"
                    row["torch_rounds"] = result["rounds"]
                row["label"] = {"call_sync_us": call_sync(label), "device_event_us": event(label, 20 if n * voxels < (1 << 22) else 4)}
                if want_fields:
                    row["torch"] = {"call_sync_us": call_sync(by_torch, TORCH_REPS, TORCH_WARMUP)}
                    row["torch_over_label"] = round(row["torch"]["call_sync_us"]["median"] / row["label"]["call_sync_us"]["median"], 2)
                else:
                    row["torch"] = "not measured: the baseline labels every cell whatever is wanted of the labels"
                print(json.dumps(row), flush=True)
    svo.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", metavar="FORMAT")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "label" / "results.json"))
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
                                          "repeats": REPS, "torch_repeats": TORCH_REPS, "anchor_faces": 0x3F, "max_pieces": 250, "max_steps": 4096, "cases": results},
                                         indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
