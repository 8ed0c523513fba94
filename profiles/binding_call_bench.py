"""The Python cost of a batch or block method's call, microseconds: voxel-rs_amd/hip.py of two trees side by side, for a change to the binding that
leaves the library alone. No GPU and no library: hip.lib is replaced by a stand-in whose every vx_* returns VX_OK (tests/test_binding_calls.py's
recorder, recording nothing), so a figure is the argument handling alone.

    python profiles/binding_call_bench.py --parent-tree DIR [--rounds 5] [--out profiles/binding_call/results.json]

DIR is a checkout of the commit to compare against (git archive of it is enough; nothing is built). The two trees take turns, `--rounds`
times each, every turn a fresh child process that loads the package from its tree; the driver stops at the first child that fails. Per child:
    every method from Svo.raycast_batch to Svo.physics_step, host arrays, outputs supplied, 1 and 4,096 items
    BATCHES samples a row after WARMUP calls, a sample the mean of CALLS calls in a row (20,000 calls a row and child)
A row pools a tree's samples over its rounds: median, p10, p90, and the median of each round. `above_parent_band`: the branch's median lies
above the parent's p90 of that same run -- the margin is the parent's own spread, there is no other threshold; below the band is fine. The
driver's status is 1 when a row lies above its band."""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
BATCHES, CALLS, WARMUP = 100, 200, 200
ITEMS = (1, 4096)


class Nothing:
    """Stands in for the library: every vx_* returns VX_OK."""

    def __getattr__(self, name):
        if not name.startswith("vx_"):
            raise AttributeError(name)
        setattr(self, name, lambda *args: 0)
        return getattr(self, name)


def case(tree):
    sys.path.insert(0, tree)
    import ctypes as C

    import numpy as np

    from _pkg import load_package

    load_package()
    from voxel_rs_amd import hip

    assert Path(hip.__file__).resolve().parent.parent == Path(tree).resolve(), hip.__file__
    nothing = Nothing()
    hip.lib = lambda: nothing
    svo = hip.Svo.__new__(hip.Svo)
    svo._h, svo.svo_type = C.c_void_p(1), 0
    u = hip.Uniforms()
    for n in ITEMS:
        f32 = lambda: np.zeros((n, 3), dtype=np.float32)  # noqa: E731
        rec = lambda dtype, *shape: np.zeros(shape or n, dtype=dtype)  # noqa: E731
        p, e, m, g, lo = f32(), f32(), f32(), f32(), np.zeros((n, 3), dtype=np.int32)
        fields, ents, views = np.zeros((n, 64), dtype=np.uint8), np.zeros(n, dtype=hip.ENTITY_DTYPE), (hip.Uniforms * n)()
        hits, cells, scans, boxes, moves = (rec(d) for d in (hip.RAY_HIT_DTYPE, hip.BLOCK_CELL_DTYPE, hip.SCAN_HIT_DTYPE, hip.BOX_HIT_DTYPE, hip.MOVE_HIT_DTYPE))
        flood, light, label, walk = (rec(d) for d in (hip.FLOOD_INFO_DTYPE, hip.LIGHT_INFO_DTYPE, hip.LABEL_INFO_DTYPE, hip.WALK_INFO_DTYPE))
        pixels, records, ats = np.zeros((n, 4), dtype=np.float32), rec(hip.HIT_DTYPE), rec(hip.BLOCK_AT_DTYPE)
        ids, columns, pieces, paths = np.zeros((4, 4, n), dtype=np.uint32), rec(hip.SCAN_HIT_DTYPE, 4, n), rec(hip.LABEL_PIECE_DTYPE, n, 2), np.zeros((n, 4), dtype=np.uint32)
        fns = {
            "raycast_batch": lambda: svo.raycast_batch(p, e, out=hits),
            "trace_rays": lambda: svo.trace_rays(u, p, e, want_hits=True, out=(pixels, records)),
            "trace_views": lambda: svo.trace_views(views, 1, 1, want_hits=True, out=(pixels, records)),
            "block_points": lambda: svo.block_points(p, out=cells),
            "read_region": lambda: svo.read_region((1, 2, 3), (n, 4, 4), out=ids),
            "list_region": lambda: svo.list_region((1, 2, 3), (n, 4, 4), out=ats),
            "scan_points": lambda: svo.scan_points(p, hip.VX_DIR_NEG_Y, out=scans),
            "scan_columns": lambda: svo.scan_columns((1, 2, 3), (n, 4, 4), hip.VX_DIR_NEG_Y, out=columns),
            "overlap_boxes": lambda: svo.overlap_boxes(p, e, out=boxes),
            "move_boxes": lambda: svo.move_boxes(p, e, m, out=moves),
            "flood_points": lambda: svo.flood_points(p, (4, 4, 4), fields=fields, info=flood),
            "light_boxes": lambda: svo.light_boxes(lo, (4, 4, 4), (0x10, 0x1F), fields=fields, info=light),
            "label_boxes": lambda: svo.label_boxes(lo, (4, 4, 4), max_pieces=2, fields=fields, pieces=pieces, info=label),
            "walk_points": lambda: svo.walk_points(p, (4, 4, 4), goals=g, path_capacity=4, fields=fields, info=walk, paths=paths),
            "physics_step": lambda: svo.physics_step(ents, 0.05),
        }
        for method, fn in fns.items():
            for _ in range(WARMUP):
                fn()
            samples = []
            for _ in range(BATCHES):
                t0 = time.perf_counter()
                for _ in range(CALLS):
                    fn()
                samples.append(round((time.perf_counter() - t0) / CALLS * 1e6, 3))
            print(json.dumps({"method": method, "items": n, "samples_us": samples}), flush=True)
    svo._h = None  # (close would call the stand-in)


def stats(v):
    import numpy as np

    return {"median": round(float(np.median(v)), 3), "p10": round(float(np.percentile(v, 10)), 3), "p90": round(float(np.percentile(v, 90)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", metavar="TREE")
    ap.add_argument("--parent-tree")
    ap.add_argument("--branch-tree", default=str(ROOT))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "binding_call" / "results.json"))
    ap.add_argument("--timeout", type=int, default=300)
    args = ap.parse_args()
    if args.case:
        case(args.case)
        return 0
    if not args.parent_tree:
        ap.error("--parent-tree is required")
    trees = {"parent": str(Path(args.parent_tree).resolve()), "branch": str(Path(args.branch_tree).resolve())}
    samples = {}  # (method, items) -> tree -> one list a round
    for rnd in range(args.rounds):
        for name, tree in trees.items():
            r = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, __file__, "--case", tree], stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:
                print(f"round {rnd}, tree {name} ended with status {r.returncode}: stopping", file=sys.stderr)
                return r.returncode
            for line in r.stdout.strip().splitlines():
                row = json.loads(line)
                samples.setdefault((row["method"], row["items"]), {}).setdefault(name, []).append(row["samples_us"])
            print(f"round {rnd}, tree {name}: done", flush=True)
    cases = []
    for (method, items), by_tree in samples.items():
        row = {"method": method, "items": items}
        for name, rounds in by_tree.items():
            row[name] = dict(stats([v for r in rounds for v in r]), round_medians=[stats(r)["median"] for r in rounds])
        row["branch_over_parent"] = round(row["branch"]["median"] / row["parent"]["median"], 3)
        row["above_parent_band"] = row["branch"]["median"] > row["parent"]["p90"]
        print(json.dumps(row), flush=True)
        cases.append(row)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"what": "Python argument handling of one call, the library replaced by a stand-in; host arrays, outputs supplied",
                                          "unit": "microseconds a call, host clock, mean of %d calls a sample" % CALLS, "rounds": args.rounds,
                                          "samples_a_round": BATCHES, "cases": cases}, indent=1) + "\n")
    return 1 if any(c["above_parent_band"] for c in cases) else 0


if __name__ == "__main__":
    sys.exit(main())
