"""The hand-scheduled traversal loop's exits (vx_loop_gfx950.hpp): the listed build's single leaf exit, which leaves telling a ray at a leaf from one
led into the voxel it started in to render_persistent, beside the ESVO world's and the walk's exits, which stay as they were. Small CSVO and ESVO heightfields of depth 6 and 9 at 200x120
(edge tiles, no multiple of 8), three views -- the eye inside a solid voxel (whole waves of rays that park in their first trip with t_min <= 0), the
eye in air one block above the surface looking along it (hits, misses, shadow rays that start inside their voxel), frame 7 of bench.py's moving
camera -- and six settings of the library, a worker process each (tests/loop_exits_worker.py: the knobs are read when a context is created), all
started together. With VX_SERVICE_MIN=48 and =33 a wave leaves the loop and comes back in mid-batch: parked lanes wait across calls of the loop.

The rule is the sibling tests': between the legs those hold identical (test_plain_frame: the whole-frame build and the general one; test_hip_parity,
test_kernel_versions_agree: a leg's image-only frames and its frame with hit records; every leg's hit records) the same bytes, and every leg within
test_hip_parity's tolerance of the CPU oracle -- hit records bit for bit, colours within COLOR_TOL."""
import functools
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import pytest

from helpers import ROOT, SVO_TYPES, orc, vra
from loop_exits_worker import H, SEED, VIEWS, W, WORLDS, views_of

COLOR_TOL = 5e-6  # tests/test_hip_parity.py's

# leg -> environment
LEGS = {
    "two frames in flight": {},                         # the whole-frame build
    "one frame in flight": {"VX_FRAMES_IN_FLIGHT": "1"},  # the general build
    "walked": {"VX_FOREIGN_RERUN": "0"},                # the loop variant with the second exit
    "service at 48": {"VX_SERVICE_MIN": "48"},
    "service at 33": {"VX_SERVICE_MIN": "33"},
    "world's bytes": {"VX_TRAVERSAL_IMAGE": "0"},       # the compiler's loop, the reference's cursor
}
WORLD_KEYS = ["%s %d" % w for w in WORLDS]


@functools.lru_cache(maxsize=None)
def legs():
    """every leg's worker, started together (two host threads each); leg -> its JSON line, with "arrays" = the frames and hit records it wrote. The
    first worker that fails ends the others."""
    tmp = Path(tempfile.mkdtemp(prefix="loop_exits_"))
    base = {k: v for k, v in os.environ.items() if not k.startswith("VX_")}
    procs, out = {}, {}
    try:
        for leg, env in LEGS.items():
            dump = tmp / (leg.replace(" ", "_").replace("'", "") + ".npz")
            procs[leg] = (subprocess.Popen([sys.executable, str(Path(ROOT) / "tests" / "loop_exits_worker.py"), str(dump)], env={**base, **env},
                                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True), dump)
        waiting, deadline = dict(procs), time.monotonic() + 300
        while waiting:
            for leg, (p, dump) in list(waiting.items()):
                try:
                    so, se = p.communicate(timeout=0.2)
                except subprocess.TimeoutExpired:
                    assert time.monotonic() < deadline, (leg, "still running")
                    continue
                del waiting[leg]
                assert p.returncode == 0, (leg, p.returncode, se[-2000:])
                out[leg] = json.loads([ln for ln in so.splitlines() if ln.startswith("{")][-1])
                out[leg]["arrays"] = dict(np.load(dump))
    finally:
        for p, _ in procs.values():
            if p.poll() is None:
                p.kill()
                p.communicate()
        shutil.rmtree(tmp, ignore_errors=True)
    return out


@functools.lru_cache(maxsize=None)
def oracle_frames(world_key):
    """the CPU oracle's frame and hit records of the world's three views"""
    from voxel_rs_amd import host, scenes

    fmt, depth = world_key.split()
    world = vra.World(SVO_TYPES[fmt])
    st = world.build_heightfield(int(depth), seed=SEED, threads=4)
    tex, mats = scenes.synthetic_textures(), scenes.synthetic_materials()
    scene = orc.OracleScene(SVO_TYPES[fmt], world.frame(), mats.view(orc.MATERIAL_DTYPE), tex, 6)
    return [scene.render(orc.Uniforms.from_buffer_copy(bytes(u)), W, H) for u in views_of(scenes, host, int(depth), st["h_max"])]


@pytest.mark.gpu
def test_the_settings_took():
    """The knobs the context reports, and what the inside-voxel view's frame of a CSVO world did with its rays: listed (no walk phases) by default,
    walked in service phases with VX_FOREIGN_RERUN=0, neither on the world's own bytes (no image cursor is ever led into a voxel)."""
    got = legs()
    assert got["two frames in flight"]["knobs"]["plain_frame"] == 1
    assert got["service at 48"]["knobs"]["service_min"] == 48 and got["service at 33"]["knobs"]["service_min"] == 33
    assert got["two frames in flight"]["knobs"]["service_min"] not in (33, 48)
    for world_key in WORLD_KEYS:
        if not world_key.startswith("csvo"):
            continue
        listed, walked, on_bytes = (got[leg][world_key]["excursions"] for leg in ("two frames in flight", "walked", "world's bytes"))
        assert listed["rays"] >= W * H and listed["service_phases"] == 0, (world_key, listed)
        assert walked["rays"] > 0 and walked["service_phases"] > 0 and walked["iterations_on_bytes"] > 0, (world_key, walked)
        assert on_bytes["rays"] == 0 and on_bytes["service_phases"] == 0, (world_key, on_bytes)


@pytest.mark.gpu
@pytest.mark.parametrize("world_key", WORLD_KEYS)
@pytest.mark.parametrize("leg", list(LEGS))
def test_a_legs_frames_are_one_frame(leg, world_key):
    """A view's whole frame in device memory, its frame on the context's own stream and its frame with hit records: the same bytes."""
    row = legs()[leg][world_key]
    assert len(row["device"]) == len(VIEWS) and len(set(row["device"])) == len(VIEWS)  # (three different views)
    assert row["device"] == row["own"] == row["with hits"]


@pytest.mark.gpu
@pytest.mark.parametrize("world_key", WORLD_KEYS)
def test_the_legs_agree(world_key):
    """The whole-frame build and the general one: the same frames; every leg: the same hit records."""
    got = legs()
    assert got["two frames in flight"][world_key]["device"] == got["one frame in flight"][world_key]["device"]
    for leg in LEGS:
        assert got[leg][world_key]["hits"] == got["two frames in flight"][world_key]["hits"], leg


@pytest.mark.gpu
@pytest.mark.parametrize("world_key", WORLD_KEYS)
@pytest.mark.parametrize("leg", list(LEGS))
def test_against_the_oracle(leg, world_key):
    """Hit records bit for bit, colours within COLOR_TOL. (Hit records come from the builds with hit records, which never list a ray: the listed build's
    single leaf exit is held by the image's bytes -- test_a_legs_frames_are_one_frame -- and by the colours here, its iteration count by nothing.)"""
    arrays = legs()[leg]["arrays"]
    for i, (cimg, chits) in enumerate(oracle_frames(world_key)):
        img, hits = arrays["%s|%d|image" % (world_key, i)], arrays["%s|%d|hits" % (world_key, i)]
        assert hits.tobytes() == chits.tobytes(), (VIEWS[i], "hit records")
        assert img.shape == cimg.shape and np.array_equal(np.isnan(img), np.isnan(cimg)), VIEWS[i]
        assert np.nanmax(np.abs(img - cimg)) <= COLOR_TOL, (VIEWS[i], float(np.nanmax(np.abs(img - cimg))))


@pytest.mark.gpu
def test_the_views_are_what_they_are_meant_to_be():
    """The eye inside a voxel: every primary ray of the frame is led into the voxel it started in, so a CSVO world's frame lists at least a ray a
    pixel (whole waves park in one trip); along the surface: hits, misses and shadow rays in one frame."""
    for world_key in WORLD_KEYS:
        flags = oracle_frames(world_key)[1][1]["flags"]
        hit, shadow = (flags & 1) != 0, ((flags >> 1) & 1) != 0
        assert 0.05 < hit.mean() < 0.95 and shadow.sum() > 100, world_key
        if world_key.startswith("csvo"):
            assert legs()["two frames in flight"][world_key]["inside-voxel rays"] >= W * H, world_key
