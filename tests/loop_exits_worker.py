"""Worker of tests/test_loop_exits.py: one process, one setting of the library's knobs (they are read when a context is created: hence a process
per leg). Renders, under the environment it was started with, three views of four small worlds -- the views at which the hand-scheduled traversal
loop's exits matter (vx_loop_gfx950.hpp): lanes that park at a leaf, whole waves whose rays start inside a voxel -- each view
as a whole frame in device memory (the frames in flight the context was given), on the context's own stream, and with hit records. Prints the
frames' digests and the context's knobs as one JSON line; the frames and hit records go to an .npz file.

    VX_SERVICE_MIN=33 python tests/loop_exits_worker.py /tmp/leg.npz
"""
import hashlib
import json
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

W, H = 200, 120  # edge tiles, and no multiple of 8
WORLDS = [("csvo", 6), ("csvo", 9), ("esvo", 6), ("esvo", 9)]
VIEWS = ("inside a voxel", "along the surface", "frame 7")
SEED = 0x5EED0001


def views_of(scenes, host, depth, h_max):
    """the three views of a world of this depth, in VIEWS' order"""
    import bench

    n = float(1 << depth)
    x, z = 0.5 * n + 0.3, 0.5 * n + 0.6
    ground = float(host.scene_height(depth, SEED, int(x), int(z)))
    # the eye inside the column's top voxel: every primary ray starts inside a solid voxel
    inside = scenes.render_params_to_uniforms((x, ground + 0.5, z), (0.6, 0.15, 0.7), (0.0, 1.0, 0.0), math.radians(72.0), W / H, 0.3, (-1.0, -1.0, -1.0), True, 3.0e38)
    # the eye in air, one block above the highest of the columns around it, looking along the surface: hits, misses, shadow rays that start inside their voxel
    top = float(host.scene_heights(depth, SEED, int(x) - 1, int(z) - 1, 3, 3).max())
    along = scenes.render_params_to_uniforms((x, top + 2.0, z), (0.6, -0.05, 0.7), (0.0, 1.0, 0.0), math.radians(72.0), W / H, 0.3, (-1.0, -1.0, -1.0), True, 3.0e38)
    return [inside, along, bench.moving_uniforms(scenes, depth, h_max, W, H, 7)]


def main():
    dump = sys.argv[1]
    import numpy as np
    import torch

    from _pkg import load_package

    vra = load_package()
    from voxel_rs_amd import hip, host, scenes

    sha = lambda b: hashlib.sha256(b).hexdigest()
    out, arrays = {}, {}
    for fmt_name, depth in WORLDS:
        fmt = vra.SVO_ESVO if fmt_name == "esvo" else vra.SVO_CSVO
        world = vra.World(fmt)
        st = world.build_heightfield(depth, seed=SEED, threads=2)  # (six workers at a time)
        svo = hip.Svo(fmt, world.size_in_bytes + (1 << 20))
        svo.set_materials(scenes.synthetic_materials())
        svo.set_textures(scenes.synthetic_textures(), 6)
        svo.update_full(world)
        us = views_of(scenes, host, depth, st["h_max"])
        key = "%s %d" % (fmt_name, depth)
        out["knobs"] = svo.knobs()
        # whole frames in device memory, one behind the other: the launches the whole-frame build serves where two frames are in flight
        frames = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in us]
        torch.cuda.synchronize()
        for u, f in zip(us, frames):
            svo.render_device(u, W, H, f.data_ptr())
        svo.sync()
        device = [f.cpu().numpy() for f in frames]
        row = {"device": [sha(f.tobytes()) for f in device], "own": [], "with hits": [], "hits": []}
        for i, u in enumerate(us):
            img, hits = svo.render(u, W, H, want_hits=True)
            row["with hits"].append(sha(img.tobytes()))
            row["hits"].append(sha(hits.tobytes()))
            row["own"].append(sha(svo.render(u, W, H)[0].tobytes()))
            arrays["%s|%d|image" % (key, i)] = device[i]
            arrays["%s|%d|hits" % (key, i)] = hits
        # how many rays the first view's frame lists (CSVO worlds) or walks inside their voxels
        svo.excursion_counters(reset=True)
        torch.cuda.synchronize()  # (the reset zeroes the counters with a memset on the default stream, which the render's stream does not wait for)
        svo.render(us[0], W, H)
        torch.cuda.synchronize()
        row["excursions"] = svo.excursion_counters(reset=True)  # rays listed or walked, the walks' service phases and iterations on the world's bytes
        row["inside-voxel rays"] = row["excursions"]["rays"]
        svo.excursion_counters(stop=True)
        out[key] = row
        svo.close()
    np.savez(dump, **arrays)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
