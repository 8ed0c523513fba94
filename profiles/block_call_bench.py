"""The host cost of a block entry point's call, microseconds: two builds of the libraries side by side, for a change to blocks_runtime.cpp
that leaves the kernels alone.

    python profiles/block_call_bench.py --parent-lib DIR [--branch-lib voxel-rs_amd/lib] [--rounds 4] [--out profiles/block_call/results.json]

DIR holds libvoxelhip.so and libvoxelhost.so built from the commit to compare against (make -C voxel-rs_amd hip host in a checkout of it).
The two builds take turns, `--rounds` times each, every turn a fresh child process under `timeout` that loads its build through VX_LIB_DIR;
the driver stops at the first child that fails. On a depth-9 heightfield, per child:
    vx_block_points, vx_overlap_boxes, vx_move_boxes, vx_flood_points (a box of 8 x 8 x 8 cells, fields and records)
    host memory, 1 and 4,096 items; device memory, 1 item
    the host clock around the call and the vx_sync behind it (profiles/boxes_bench.py's call_sync): REPS samples after WARMUP calls
A row pools a build's samples over its rounds: median, p10, p90, and the median of each round. `inside_parent_band`: the branch's median lies
within the parent's p10..p90 of that same run -- the margin is the parent's own spread, there is no other threshold. At 1 item every figure
is the latency of one launch and one wait.

    python profiles/block_call_bench.py --parent-tree DIR [--out profiles/block_call/binding.json]

For a change to the Python binding instead: the parent's children run DIR/profiles/block_call_bench.py --case, a checkout of the commit to
compare against, with the branch's libraries (or --parent-lib), so that the two sides differ only in voxel-rs_amd/hip.py."""
import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REPS, WARMUP = 40, 10
CALLS = ("vx_block_points", "vx_overlap_boxes", "vx_move_boxes", "vx_flood_points")
ROWS = (("host", 1), ("host", 4096), ("device", 1))


def case():
    sys.path.insert(0, str(ROOT))
    import numpy as np
    import torch

    from _pkg import load_package

    vra = load_package()
    from voxel_rs_amd import hip, scenes

    depth = 9
    world = vra.World(vra.SVO_ESVO)
    st = world.build_heightfield(depth)
    svo = hip.Svo(vra.SVO_ESVO, world.size_in_bytes + (4 << 20))
    svo.set_materials(scenes.synthetic_materials())
    svo.set_textures(scenes.synthetic_textures(), 6)
    svo.update(world)
    L, h = hip.lib(), svo._h
    size, h_max = float(1 << depth), float(st["h_max"])
    rng = np.random.default_rng(11)
    pts = np.stack([rng.uniform(0.3 * size, 0.7 * size, 4096), rng.uniform(0.0, h_max, 4096), rng.uniform(0.3 * size, 0.7 * size, 4096)], axis=1).astype(np.float32)
    extents, motion, cells = np.float32([0.8, 1.8, 0.8]), np.float32([0.3, -0.5, 0.2]), (8, 8, 8)

    def call_sync(fn):
        out = []
        for i in range(REPS + WARMUP):
            t0 = time.perf_counter()
            fn()
            L.vx_sync(h)
            if i >= WARMUP:
                out.append(round((time.perf_counter() - t0) * 1e6, 2))
        return out

    for memory, n in ROWS:
        if memory == "host":
            p, e, m = pts[:n].copy(), extents, motion
            cell_out, box_out, move_out = np.zeros(n, dtype=hip.BLOCK_CELL_DTYPE), np.zeros(n, dtype=hip.BOX_HIT_DTYPE), np.zeros(n, dtype=hip.MOVE_HIT_DTYPE)
            fields, info = np.zeros((n, 512), dtype=np.uint8), np.zeros(n, dtype=hip.FLOOD_INFO_DTYPE)
        else:
            p, e, m = torch.from_numpy(pts[:n].copy()).cuda(), torch.from_numpy(extents).cuda(), torch.from_numpy(motion).cuda()
            cell_out, box_out, move_out = (torch.empty((n, w), dtype=torch.int32, device="cuda") for w in (2, 8, 12))
            fields, info = torch.empty((n, 512), dtype=torch.uint8, device="cuda"), torch.empty((n, 4), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()  # (what torch has prepared on its own stream is there before the context's stream reads it)
        fns = {"vx_block_points": lambda: svo.block_points(p, out=cell_out), "vx_overlap_boxes": lambda: svo.overlap_boxes(p, e, out=box_out),
               "vx_move_boxes": lambda: svo.move_boxes(p, e, m, out=move_out), "vx_flood_points": lambda: svo.flood_points(p, cells, fields=fields, info=info)}
        for call in CALLS:
            print(json.dumps({"call": call, "memory": memory, "items": n, "samples_us": call_sync(fns[call])}), flush=True)
    svo.close()


def stats(v):
    import numpy as np

    return {"median": round(float(np.median(v)), 2), "p10": round(float(np.percentile(v, 10)), 2), "p90": round(float(np.percentile(v, 90)), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--parent-tree")
    ap.add_argument("--branch-lib", default=str(ROOT / "voxel-rs_amd" / "lib"))
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "block_call" / "results.json"))
    ap.add_argument("--timeout", type=int, default=150)
    args = ap.parse_args()
    if args.case:
        case()
        return 0
    if not args.parent_lib and not args.parent_tree:
        ap.error("--parent-lib or --parent-tree is required")
    args.parent_lib = args.parent_lib or args.branch_lib  # (a tree alone: one build of the libraries under both)
    libs = {"parent": str(Path(args.parent_lib).resolve()), "branch": str(Path(args.branch_lib).resolve())}
    scripts = {"parent": str(Path(args.parent_tree).resolve() / "profiles" / "block_call_bench.py") if args.parent_tree else __file__, "branch": __file__}
    samples = {}  # (call, memory, items) -> build -> one list a round
    for rnd in range(args.rounds):
        for build, lib in libs.items():
            r = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, scripts[build], "--case"], stdout=subprocess.PIPE, text=True,
                               env=dict(os.environ, VX_LIB_DIR=lib))
            if r.returncode != 0:
                print(f"round {rnd}, build {build} ended with status {r.returncode}: stopping", file=sys.stderr)
                return r.returncode
            for line in r.stdout.strip().splitlines():
                row = json.loads(line)
                samples.setdefault((row["call"], row["memory"], row["items"]), {}).setdefault(build, []).append(row["samples_us"])
            print(f"round {rnd}, build {build}: done", flush=True)
    cases = []
    for (call, memory, items), by_build in samples.items():
        row = {"call": call, "memory": memory, "items": items}
        for build, rounds in by_build.items():
            row[build] = dict(stats([v for r in rounds for v in r]), round_medians=[stats(r)["median"] for r in rounds])
        row["branch_over_parent"] = round(row["branch"]["median"] / row["parent"]["median"], 3)
        row["inside_parent_band"] = row["parent"]["p10"] <= row["branch"]["median"] <= row["parent"]["p90"]
        row["above_parent_band"] = row["branch"]["median"] > row["parent"]["p90"]  # (below the band is fine)
        print(json.dumps(row), flush=True)
        cases.append(row)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": "MI355X (gfx950)", "scene": "heightfield depth 9, ESVO", "unit": "microseconds per call and vx_sync, host clock",
                                          "rounds": args.rounds, "samples_a_round": REPS, "cases": cases}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
