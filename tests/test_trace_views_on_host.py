"""vx_trace_views without a GPU: its per-lane device code (voxel-rs_amd/csrc/trace/vx_views.hpp), compiled for the host by the test-only harness
tests/cpp/views_on_host.cpp over the shims of tests/cpp/shims, run for every lane of every workgroup of the kernel's grid on the cases of
tests/views_cases.py and held against the oracle -- records byte for byte, colours within 5e-6, RGBA8 as the packing, every output index
written exactly once and nothing by the lanes outside the image -- and, from the oracle's results alone, that those cases hold what they were
specified to hold. test_trace_views.py runs the same cases through the kernel on the GPU."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import trace_cases as tc
import views_cases as vc
from helpers import ROOT
from voxel_rs_amd import hip

BUILD = Path(ROOT) / "tests" / "_build"
_vp = C.c_void_p
WORLDS = [(n, f) for n in ("heightfield", "glasshouse", "far_chunks") for f in ("esvo", "csvo")]
FORMATS = [hip.VX_FORMAT_RGBA32F, hip.VX_FORMAT_RGBA8]
FORMAT_IDS = ["rgba32f", "rgba8"]


@pytest.fixture(scope="module")
def viewshost():
    BUILD.mkdir(exist_ok=True)
    so = BUILD / "libviews_on_host.so"
    csrc = Path(ROOT) / "voxel-rs_amd" / "csrc"
    deps = [Path(ROOT) / "tests" / "cpp" / "views_on_host.cpp", csrc / "trace" / "vx_views.hpp", csrc / "trace" / "vx_trace.hpp", csrc / "trace" / "vx_view_params.hpp", csrc / "hip" / "vx_device.hpp",
            csrc / "hip" / "vx_args.hpp", Path(ROOT) / "tests" / "cpp" / "shims" / "vx_platform.hpp", Path(ROOT) / "tests" / "cpp" / "shims" / "hip_on_host.hpp",
            Path(ROOT) / "include" / "voxel_hip.h"]
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in deps):
        # tests/cpp/shims comes first: its vx_platform.hpp (plain C++) is found instead of the product's (gfx950 built-ins)
        cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", f"-I{ROOT}/include", f"-I{ROOT}/tests/cpp/shims",
               f"-I{csrc}/hip", f"-I{csrc}/trace", str(deps[0]), "-o", str(so)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    return C.CDLL(str(so))


def views_on_host(lib, c, pixel_format):
    """(rgba32f [N, H, W, 4], rgba8 [N, H, W, 4] uint8, records [N, H * W], writes per index, (lanes that left, stray stores, workgroups))."""
    frame, mats, chain, n_levels, level_offset = tc.scene_arguments(c)
    n, w, h = len(c.views), c.width, c.height
    rgba, rgba8, hits = np.zeros((n, h, w, 4), dtype=np.float32), np.zeros((n, h, w, 4), dtype=np.uint8), np.zeros((n, h * w), dtype=hip.HIT_DTYPE)
    writes, tally = np.zeros(n * h * w, dtype=np.uint32), np.zeros(3, dtype=np.uint64)
    lib.viewshost_trace_views(c.svo_type, frame.ctypes.data_as(_vp), C.c_uint64(frame.size * 4), mats.ctypes.data_as(_vp), len(mats), chain.ctypes.data_as(_vp),
                              c.tex.shape[2], c.tex.shape[1], c.tex.shape[0], n_levels, level_offset, vc.uniforms_array(c.views), n, w, h,
                              1 if pixel_format == hip.VX_FORMAT_RGBA8 else 0, rgba.ctypes.data_as(_vp), rgba8.ctypes.data_as(_vp), hits.ctypes.data_as(_vp),
                              writes.ctypes.data_as(_vp), tally.ctypes.data_as(_vp))
    return rgba, rgba8, hits, writes, tuple(int(v) for v in tally)


def check_against_the_oracle(lib, c, pixel_format, what):
    rgba, rgba8, hits, writes, (left, stray, groups) = views_on_host(lib, c, pixel_format)
    n, w, h = len(c.views), c.width, c.height
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    assert groups == n * tiles and stray == 0
    assert (writes == 1).all(), f"{what}: {(writes != 1).sum()} output indices are not written exactly once"
    assert left == groups * 64 - n * w * h  # every lane either stores once or leaves
    exp_img, exp_hits = vc.expected(c, pixel_format)
    for k in range(n):
        tc.assert_records(hits[k], exp_hits[k], f"{what}, view {k}")
        tc.assert_colors(rgba[k], exp_img[k], f"{what}, view {k}")
    assert (rgba8.reshape(-1, 4) == tc.pack_rgba8(rgba.reshape(-1, 4))).all()


@pytest.mark.parametrize("name,fmt", WORLDS)
def test_the_small_views_hold_what_they_should(name, fmt):
    """Counted on the oracle's records; a view that misses a condition is changed, never the threshold."""
    c = vc.small_views(name, fmt)
    print(f"\n{name}-{fmt}: {c.counts}")
    assert (c.width, c.height, len(c.views)) == (20, 13, 5)
    total = {k: sum(v[k] for v in c.counts) for k in c.counts[0]}
    assert total["sky"] >= 100 and total["lit"] >= 100 and total["shadow"] >= 30, total
    assert all(v["sky"] >= 1 and v["hit"] >= 1 for v in c.counts), c.counts
    assert c.counts[3]["outline"] >= 1
    assert c.counts[1]["lit"] == 0 and c.counts[1]["shadow"] == 0  # (shadows off: no shadow ray is cast)
    for a in range(5):
        for b in range(a + 1, 5):
            assert c.hits[a].tobytes() != c.hits[b].tobytes(), (a, b)
    # the cameras: five eyes, five forward vectors, three values of fovy, one aspect that is not W / H, one projective matrix
    assert len({bytes(u)[48:64] for u in c.views}) == 5 and len({bytes(u)[32:44] for u in c.views}) == 5
    assert len({u.fovy for u in c.views}) == 3 and sum(u.aspect != np.float32(20 / 13) for u in c.views) == 1
    assert [tuple(u.view)[3::4] != (0.0, 0.0, 0.0, 1.0) for u in c.views] == [False, False, False, False, True]
    assert c.views[0].render_shadows and np.isfinite(c.views[0].shadow_distance) and not c.views[1].render_shadows
    assert tuple(c.views[2].light_dir) != tuple(c.views[0].light_dir) and c.views[2].ambient != c.views[0].ambient
    assert not np.isnan(c.views[3].highlight_pos[0]) and all(np.isnan(u.highlight_pos[0]) for k, u in enumerate(c.views) if k != 3)


@pytest.mark.parametrize("pixel_format", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("name,fmt", WORLDS)
def test_small_views_on_the_host_are_the_oracles_renders(viewshost, name, fmt, pixel_format):
    """Case (a): 5 views x 6 workgroups x 64 lanes, 260 of each view's 384 lanes inside the image."""
    check_against_the_oracle(viewshost, vc.small_views(name, fmt), pixel_format, f"{name}-{fmt} small views on the host")


@pytest.mark.parametrize("pixel_format", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("fmt", ["esvo", "csvo"])
def test_the_camera_batch_on_the_host_is_the_oracles_renders(viewshost, fmt, pixel_format):
    """Case (b): the heightfield's three 64 x 48 views (whole tiles only) as one batch."""
    c = vc.camera_batch(fmt)
    check_against_the_oracle(viewshost, c, pixel_format, f"heightfield-{fmt} camera batch on the host")
    assert c.hits[0].tobytes() == c.hits[1].tobytes() and (c.hits[2]["flags"] & 8).sum() == 0 and (c.hits[0]["flags"] & 8).sum() >= 4
