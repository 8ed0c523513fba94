"""The render kernel's whole-frame builds (render_persistent's PLAIN flag; launch_render takes one where vxk::plain_frame holds and VX_PLAIN_FRAME is
not 0) against the general builds: the same frames, bit for bit, on the three image-only kernels a small world reaches -- the ESVO world's, the
CSVO world's that lists its inside-voxel rays (default) and the one that walks them (VX_FOREIGN_RERUN=0) --, at a size with edge tiles and a
narrower last strip (333x227) and at one with fewer sub-tiles than resident waves (64x40); against the CPU oracle; and the launches that must
not take a whole-frame build. A worker process per setting (tests/plain_worker.py): the knobs are read when a context is created."""
import functools
import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

from helpers import ROOT, SVO_TYPES, orc, vra

COLOR_TOL = 5e-6  # tests/test_hip_parity.py's, for image-only frames against the oracle

# leg -> (world format, environment)
LEGS = {"esvo": ("esvo", {}), "csvo listed": ("csvo", {}), "csvo walked": ("csvo", {"VX_FOREIGN_RERUN": "0"})}
SIZES = [(333, 227), (64, 40)]


@functools.lru_cache(maxsize=None)
def worker(leg, w, h, plain):
    fmt, env = LEGS[leg]
    e = {k: v for k, v in os.environ.items() if not k.startswith("VX_")}
    e.update(env)
    e["VX_PLAIN_FRAME"] = str(plain)
    dump = Path(tempfile.mkdtemp(prefix="plain_frame_")) / "frame0.npy"
    r = subprocess.run([sys.executable, str(Path(ROOT) / "tests" / "plain_worker.py"), fmt, str(w), str(h), str(dump)], env=e, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    out["frame0"] = np.load(dump)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("leg", list(LEGS))
def test_the_whole_frame_build_renders_the_same_frames(leg, size):
    """Six views of bench.py's moving camera, RGBA32F, two frames in flight: every frame's SHA-256 under VX_PLAIN_FRAME=1 is the one under =0, and
    the context says which build its whole frames run."""
    plain, general = worker(leg, *size, 1), worker(leg, *size, 0)
    assert plain["knobs"]["plain_frame"] == 1 and general["knobs"]["plain_frame"] == 0
    assert len(plain["views"]) == 6 and len(set(plain["views"])) == 6  # (the camera moves: six different frames)
    assert plain["views"] == general["views"]


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("leg", list(LEGS))
def test_launches_that_are_no_whole_frame_are_untouched(leg, size):
    """An RGBA8 target, rank 1 of 3 as a tile list, the context's own stream through seven frames (cost notes, then the cost-ordered table): none may
    take the whole-frame build, and all give the same digests under both settings."""
    plain, general = worker(leg, *size, 1), worker(leg, *size, 0)
    for key in ("rgba8", "rank 1 of 3", "own"):
        assert plain[key] == general[key], key
    assert len(plain["own"]) == 7 and len(set(plain["own"])) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("leg", list(LEGS))
def test_the_whole_frame_build_against_the_oracle(leg):
    """The moving camera's first view from the whole-frame build within test_hip_parity's colour tolerance of the CPU oracle's frame."""
    import bench
    from voxel_rs_amd import scenes

    w, h = SIZES[0]
    got = worker(leg, w, h, 1)
    fmt = LEGS[leg][0]
    world = vra.World(SVO_TYPES[fmt])
    st = world.build_heightfield(8, threads=4)
    assert st["h_max"] == got["h_max"]
    tex, mats = scenes.synthetic_textures(), scenes.synthetic_materials()
    scene = orc.OracleScene(SVO_TYPES[fmt], world.frame(), mats.view(orc.MATERIAL_DTYPE), tex, 6)
    u = bench.moving_uniforms(scenes, 8, st["h_max"], w, h, 0)
    cimg, _ = scene.render(orc.Uniforms.from_buffer_copy(bytes(u)), w, h)
    img = got["frame0"]
    assert img.shape == cimg.shape and np.array_equal(np.isnan(img), np.isnan(cimg))
    assert np.nanmax(np.abs(img - cimg)) <= COLOR_TOL


def test_the_predicate_needs_every_condition():
    """vxk::plain_frame (vx_args.hpp), compiled for the host: true for a whole RGBA32F frame with a target, plain ticket order, no cost notes, no
    excursion counters and an affine view; each of the seven conditions flipped alone turns it off."""
    build = Path(ROOT) / "tests" / "_build"
    build.mkdir(exist_ok=True)
    exe = build / "plain_frame_on_host"
    src = Path(ROOT) / "tests" / "cpp" / "plain_frame_on_host.cpp"
    inc = [Path(ROOT) / "include", Path(ROOT) / "tests" / "cpp" / "shims", Path(ROOT) / "voxel-rs_amd" / "csrc" / "hip"]
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *[f"-I{d}" for d in inc], str(src), "-o", str(exe)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = dict((ln.split()[0], int(ln.split()[1])) for ln in r.stdout.splitlines())
    assert got == {"plain": 1, "tile_count": 0, "rgba8": 0, "out": 0, "order": 0, "cost_cur": 0, "excursions": 0, "affine_view": 0}
