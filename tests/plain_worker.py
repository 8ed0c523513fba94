"""Worker of tests/test_plain_frame.py: one process, one context (VX_PLAIN_FRAME and VX_FOREIGN_RERUN are read when a context is created: hence a
process per setting). Renders, under the environment it was started with, what the test compares between the whole-frame build of the render kernel
and the general one, and prints the frames' digests and the context's knobs as one JSON line; the first frame of the moving camera goes to a file.

    VX_PLAIN_FRAME=0 python tests/plain_worker.py csvo 333 227 /tmp/frame0.npy
"""
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

DEPTH = 8
VIEWS = 6


def moving_uniforms(scenes, h_max, w, h, i):
    """bench.py's own moving camera (moving_uniforms), on this worker's world"""
    import bench

    return bench.moving_uniforms(scenes, DEPTH, h_max, w, h, i)


def main():
    fmt_name, w, h, dump = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    import numpy as np
    import torch

    from _pkg import load_package

    vra = load_package()
    from voxel_rs_amd import hip, scenes

    fmt = vra.SVO_ESVO if fmt_name == "esvo" else vra.SVO_CSVO
    world = vra.World(fmt)
    st = world.build_heightfield(DEPTH, threads=4)
    svo = hip.Svo(fmt, world.size_in_bytes + (1 << 20))
    svo.set_materials(scenes.synthetic_materials())
    svo.set_textures(scenes.synthetic_textures(), 6)
    svo.update_full(world)
    sha = lambda b: hashlib.sha256(b).hexdigest()
    us = [moving_uniforms(scenes, st["h_max"], w, h, i) for i in range(VIEWS)]
    out = {"knobs": svo.knobs(), "h_max": st["h_max"]}

    # whole frames, RGBA32F, two frames in flight: the launches the whole-frame build serves
    frames = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(VIEWS)]
    torch.cuda.synchronize()
    svo.set_frames_in_flight(2)
    for i in range(VIEWS):
        svo.render_device(us[i], w, h, frames[i].data_ptr())
    svo.sync()
    host = [f.cpu().numpy() for f in frames]
    out["views"] = [sha(f.tobytes()) for f in host]
    np.save(dump, host[0])

    # launches it must not serve: an RGBA8 target, a tile list, the context's own stream (cost notes, then the cost-ordered table)
    rgba8 = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    n = hip.local_tile_count(w, h, 1, 3)
    lst = torch.zeros((n * 1024, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    svo.render_device(us[0], w, h, rgba8.data_ptr(), fmt=hip.VX_FORMAT_RGBA8)
    svo.render_device(us[0], w, h, lst.data_ptr(), tile_rank=1, tile_count=3)
    svo.sync()
    out["rgba8"] = sha(rgba8.cpu().numpy().tobytes())
    out["rank 1 of 3"] = sha(lst.cpu().numpy().tobytes())
    out["own"] = [sha(svo.render(us[0], w, h)[0].tobytes()) for _ in range(7)]
    svo.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
