"""bench.py as the driver runs it, on one GPU at a small size: a plain run times exactly --steps frames in one block and prints the headline
fields (none of --full's); --dump-outputs writes the frame of the last timed step, which is the oracle's frame of that view and the same
from run to run."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
STEPS, DEPTH, W, H = 7, 9, 640, 360
ARGS = ["--gpus", "1", "--steps", str(STEPS), "--warmup", "2", "--depth", str(DEPTH), "--width", str(W), "--height", str(H), "--format", "csvo",
        "--textures", "procedural"]


def run_bench(extra, timeout=300):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py")] + ARGS + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert lines, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(lines[-1])


def test_plain_run_and_its_dumped_frame(tmp_path):
    d = run_bench(["--dump-outputs", str(tmp_path / "a")])
    assert d["unit"] == "Mrays/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["metric"].startswith("Mrays/sec")
    assert d["steps"] == STEPS and d["repeats"] == 1 and d["value_source"] == f"one timed block of {STEPS} frames"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert d["roofline"] is None and d["cpu_baseline"] is None and not {"sustained", "configs", "forced_sharded", "still_view", "picker"} & set(d)
    img = np.load(tmp_path / "a" / "image.npy")
    assert img.dtype == np.float32 and img.shape == (H, W, 4)

    # the last timed step renders view STEPS - 1 of the camera's path: the oracle's frame of that view
    import bench
    from _pkg import load_package
    from oracle import oracle as orc

    vra = load_package()
    from voxel_rs_amd import scenes

    world = vra.World(vra.SVO_CSVO)
    st = world.build_heightfield(DEPTH)
    scene = orc.OracleScene(vra.SVO_CSVO, world.frame(), scenes.synthetic_materials().view(orc.MATERIAL_DTYPE), scenes.synthetic_textures(), 6)
    u = bench.moving_uniforms(scenes, DEPTH, st["h_max"], W, H, STEPS - 1)
    cimg, _ = scene.render(orc.Uniforms.from_buffer_copy(bytes(u)), W, H)
    assert np.array_equal(np.isnan(img), np.isnan(cimg)) and np.nanmax(np.abs(img - cimg)) <= 5e-6

    # the same arguments, the same frame
    run_bench(["--dump-outputs", str(tmp_path / "b")])
    assert np.load(tmp_path / "b" / "image.npy").tobytes() == img.tobytes()
