"""vx_trace_rays without a GPU: its per-ray device code (voxel-rs_amd/csrc/trace/vx_trace.hpp), compiled for the host by the test-only harness
tests/cpp/trace_on_host.cpp over the shims of tests/cpp/shims, against the oracle on the camera-ray and free-ray cases of tests/trace_cases.py --
records byte for byte, colours within 5e-6 -- and, from the oracle's results alone, that those cases hold every kind of pixel and ray they
were specified to hold. test_trace_rays.py runs the same cases through the kernel on the GPU."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import trace_cases as tc
from helpers import ROOT
from voxel_rs_amd import hip

BUILD = Path(ROOT) / "tests" / "_build"
_vp = C.c_void_p
CAMERA = [(n, f) for n in ("heightfield", "glasshouse", "far_chunks") for f in ("esvo", "csvo")]
FREE = [(n, f) for n in ("heightfield", "far_chunks") for f in ("esvo", "csvo")]


@pytest.fixture(scope="module")
def tracehost():
    BUILD.mkdir(exist_ok=True)
    so = BUILD / "libtrace_on_host.so"
    csrc = Path(ROOT) / "voxel-rs_amd" / "csrc"
    deps = [Path(ROOT) / "tests" / "cpp" / "trace_on_host.cpp", csrc / "trace" / "vx_trace.hpp", csrc / "hip" / "vx_device.hpp", csrc / "hip" / "vx_args.hpp",
            Path(ROOT) / "tests" / "cpp" / "shims" / "vx_platform.hpp", Path(ROOT) / "tests" / "cpp" / "shims" / "hip_on_host.hpp",
            Path(ROOT) / "include" / "voxel_hip.h"]
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in deps):
        # tests/cpp/shims comes first: its vx_platform.hpp (plain C++) is found instead of the product's (gfx950 built-ins)
        cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", f"-I{ROOT}/include", f"-I{ROOT}/tests/cpp/shims",
               f"-I{csrc}/hip", f"-I{csrc}/trace", str(deps[0]), "-o", str(so)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    return C.CDLL(str(so))


def trace_on_host(lib, c, u, o, d, m):
    """(rgba32f [N,4], rgba8 [N,4] uint8, vx_hit records) of the harness."""
    frame, mats, chain, n_levels, level_offset = tc.scene_arguments(c)
    o, d, m = (np.array(a, dtype=np.float32, order="C") for a in (o, d, m))
    n = len(o)
    rgba, rgba8, hits = np.zeros((n, 4), dtype=np.float32), np.zeros((n, 4), dtype=np.uint8), np.zeros(n, dtype=hip.HIT_DTYPE)
    lib.tracehost_trace_rays(c.svo_type, frame.ctypes.data_as(_vp), C.c_uint64(frame.size * 4), mats.ctypes.data_as(_vp), len(mats), chain.ctypes.data_as(_vp),
                             c.tex.shape[2], c.tex.shape[1], c.tex.shape[0], n_levels, level_offset, C.byref(u), o.ctypes.data_as(_vp), d.ctypes.data_as(_vp),
                             m.ctypes.data_as(_vp), n, rgba.ctypes.data_as(_vp), rgba8.ctypes.data_as(_vp), hits.ctypes.data_as(_vp))
    return rgba, rgba8, hits


@pytest.mark.parametrize("name,fmt", CAMERA)
def test_the_views_hold_every_kind_of_pixel(name, fmt):
    """Counted on the oracle's records; a view that misses a condition is changed, never the threshold."""
    c = tc.camera_case(name, fmt)
    print(f"\n{name}-{fmt}: {c.counts}")
    k = c.counts
    assert k["sky"] >= 100 and k["lit"] >= 100 and k["shadow"] >= 50 and k["beyond"] >= 50 and k["outline"] >= 4, k
    if name != "heightfield":
        assert k["through"] >= 30, k


@pytest.mark.parametrize("name,fmt", FREE)
def test_the_free_rays_hold_every_kind(name, fmt):
    c = tc.free_case(name, fmt)
    hit = c.exp["t"] != -1.0
    assert len(c.o) == tc.N_FREE == 19 * 64 + 21 and (c.d[:tc.N_GRID] == c.d[0]).all()
    assert (~hit).sum() >= 100 and c.cut >= 40, (int((~hit).sum()), c.cut)
    assert (np.signbit(c.d) & (c.d == 0)).any() and (c.kinds == "inside").sum() == 53
    assert not np.isnan(c.color).any()
    if name == "far_chunks":
        a, b = c.lod_box
        lod = hit & (c.exp["pos"] >= a - 1e-3).all(axis=1) & (c.exp["pos"] <= b + 1e-3).all(axis=1)
        assert (lod | (hit & c.inside)).sum() >= 20


@pytest.mark.parametrize("name,fmt", CAMERA)
def test_camera_rays_on_the_host_are_the_oracles_render(tracehost, name, fmt):
    """Case 1 (and, on the heightfield, case 2: cam_pos 20 blocks from the rays' origin) through vx_trace.hpp on the host."""
    c = tc.camera_case(name, fmt)
    m = np.full(len(c.o), -1.0, dtype=np.float32)
    rgba, rgba8, hits = trace_on_host(tracehost, c, c.u, c.o, c.d, m)
    tc.assert_records(hits, c.hits, f"{name}-{fmt} on the host")
    tc.assert_colors(rgba, c.img, f"{name}-{fmt} on the host")
    assert (rgba8 == tc.pack_rgba8(rgba)).all()
    if name == "heightfield":
        moved, _, moved_hits = trace_on_host(tracehost, c, c.u_moved, c.o, c.d, m)
        tc.assert_records(moved_hits, c.hits_moved, "cam_pos moved, on the host")
        tc.assert_colors(moved, c.img_moved, "cam_pos moved, on the host")
        assert c.hits_moved.tobytes() == c.hits.tobytes()  # (the oracle: cam_pos moves no ray)
        assert (np.abs(c.img_moved - c.img).max(axis=2) > 0).sum() >= 20


@pytest.mark.parametrize("name,fmt", FREE)
def test_free_rays_on_the_host_are_the_oracles_casts(tracehost, name, fmt):
    """Case 3 through vx_trace.hpp on the host: every record field against OracleScene.intersect, the pixel against Result.color or the sky."""
    c = tc.free_case(name, fmt)
    rgba, rgba8, hits = trace_on_host(tracehost, c, c.u, c.o, c.d, c.m)
    tc.assert_records(hits, c.exp, f"{name}-{fmt} free rays on the host")
    tc.assert_colors(rgba, c.color, f"{name}-{fmt} free rays on the host")
    assert (rgba8 == tc.pack_rgba8(rgba)).all()
