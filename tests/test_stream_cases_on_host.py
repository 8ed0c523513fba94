"""The streamed world of tests/stream_cases.py without a GPU: the path streamed with pump(None, 400), both formats, and at each of its four
settled states -- that the resident chunks are the restated truth's (645 = 69 / 161 / 298 / 117 and 830 = 137 / 202 / 368 / 123 at LOD 5 / 4 / 3
/ 2), that every input set holds every kind it was specified to hold (by the truth and the oracle alone), that the host harness's points and
regions, its scans (tests/cpp/scan_on_host.cpp) and its lists (tests/cpp/list_on_host.cpp) on the streamer's frame equal the dense truth, and
that the device headers compiled for the host (batch, trace, views, physics) agree with the oracle on that frame for the ray, view and entity
sets. test_stream_batch.py runs the same sets through the nine entry points on the GPU, between ranged commits."""
import ctypes as C

import numpy as np
import pytest

import list_cases as lc
import scan_cases as scn
import stream_cases as sc
import trace_cases as tc
from batch_cases import first_difference
from blocks_cases import harness, host_points, host_region
from physics_cases import DT
from test_device_on_host import devhost  # noqa: F401  (the fixtures that build the harnesses)
from test_physics_device_on_host import host_step, physhost  # noqa: F401
from test_trace_rays_on_host import trace_on_host, tracehost  # noqa: F401
from test_trace_views_on_host import views_on_host, viewshost  # noqa: F401
from voxel_rs_amd import hip

_vp = C.c_void_p


@pytest.fixture(scope="module", params=["esvo", "csvo"])
def states(request):
    return sc.dry_run(request.param)


@pytest.fixture(scope="module")
def exe():
    return harness()


def test_the_bulk_heights_are_the_per_column_ones():
    from voxel_rs_amd import host

    rect = host.scene_heights(sc.SCENE_DEPTH, sc.SEED, 37, 901, 19, 23)
    assert rect.shape == (23, 19) and rect.dtype == np.uint32
    for z in range(23):
        for x in range(19):
            assert rect[z, x] == host.scene_height(sc.SCENE_DEPTH, sc.SEED, 37 + x, 901 + z)
    assert 54 <= sc.heights().min() and sc.heights().max() <= 216


def test_the_resident_chunks_are_the_restated_ones(states):
    """s.resident_chunks against the truth's count at every settled state; the four tables; at least 50 chunks of each LOD; the offset by the
    rule of SvoCoordSpace; the path's totals of events."""
    for x in states:
        t, lod = sc.truth(x.centre)
        counts = sc.chunk_counts(lod)
        print(f"\nstate {x.index}: centre {x.centre}, offset {x.off.tolist()}, {x.resident} chunks, by LOD {counts[1:]}, arena {x.arena_bytes} bytes, {x.totals}")
        assert x.resident == counts[0]
        assert counts == sc.CHUNKS[(x.centre[0], x.centre[2])]
        assert min(counts[1:]) >= 50
        assert (x.off == sc.offset_of(x.centre)).all()
        assert x.scene.oracle is not None and int(x.scene.words[0:1].view(np.float32)[0] * (1 << sc.SVO_DEPTH)) == 1  # (scale = 2^-11)
    assert [x.resident for x in states] == [645, 830, 830, 645]
    assert states[2].off.tolist() == [608, 608, 640] and states[1].off.tolist() == [608, 672, 640]
    assert states[2].totals["loads"] == states[1].totals["loads"] and states[2].totals["lod_changes"] == states[1].totals["lod_changes"]  # (a move in y alone: no events)
    total = states[-1].totals
    assert (total["loads"], total["unloads"], total["lod_changes"]) == (14680, 2544, 7840)
    assert states[-1].arena_bytes < (16 << 20) - (1 << 20)


def test_every_set_holds_every_kind(states):
    """The thresholds the sets were specified with, from the truth and the oracle alone."""
    for x in states:
        print(f"\nstate {x.index} ({x.scene.fmt}): {x.counts}")
        sc.assert_kinds(x.counts)
        p = x.inputs.pts
        size = np.float32(1 << sc.SVO_DEPTH)
        assert np.isnan(p).any() and (p == np.inf).any() and (p == -np.inf).any() and (p == size).any() and ((p == 0) & np.signbit(p)).any()
        assert x.inputs.rows.shape == (24, 17) and len(x.inputs.views) == 2 and all(u.render_shadows for u in x.inputs.views)


def test_points_and_regions_on_the_host_are_the_dense_truth(states, exe):
    """tests/cpp/blocks_on_host.cpp on s.frame(): every value, cell_log2 = 5 - lod on blocks; every region voxel for voxel."""
    for x in states:
        t, lod = sc.truth(x.centre)
        cells = host_points(exe, x.scene, x.inputs.pts, 12, len(x.inputs.pts))
        assert len(cells) == len(x.inputs.pts)
        sc.check_cells(t, lod, x.off, x.inputs.pts, cells, f"state {x.index} {x.scene.fmt}")
        for name, (lo, size) in x.inputs.regions.items():
            if 0 in size:
                continue
            got = host_region(exe, x.scene, lo, size)
            exp = sc.dense_region(t, x.off, lo, size)
            assert (got == exp).all(), (x.index, name, lo, size, np.argwhere(got != exp)[:8])


def test_the_scans_on_the_host_are_the_dense_truth(states):
    """tests/cpp/scan_on_host.cpp on s.frame(): the point set (NaN, +-inf, outside and integer positions among it) in all six directions at
    reaches 1, 7 and VX_SCAN_TO_EDGE, and every scan box -- each footprint along each axis over the whole octree and beyond, so that side
    elevations cross every LOD ring --, record for record against scan_cases' numpy truth over the dense arrays."""
    for x in states:
        what = f"state {x.index} {x.scene.fmt}"
        scans = scn.HostScans(scn.harness(), x.case)
        try:
            for (d, reach), exp in x.blocks.points.items():
                got = scans.points(x.inputs.pts, d, reach)
                assert scn.differing(got, exp) is None, f"{what} points {scn.DIR_NAMES[d]} reach {reach}: {scn.differing(got, exp)}"
            for (name, d), (lo, size) in x.inputs.scan_boxes.items():
                got = scans.columns(lo, size, d)
                assert scn.differing(got, x.blocks.columns[name, d]) is None, f"{what} columns {name} {scn.DIR_NAMES[d]} {lo} {size}: {scn.differing(got, x.blocks.columns[name, d])}"
        finally:
            scans.close()


def test_the_lists_on_the_host_are_the_dense_truth(states):
    """tests/cpp/list_on_host.cpp on s.frame(): every list box under every flag set against list_cases' numpy truth, and the list of the
    LOD 4 / LOD 3 box cut by a capacity of 1,000 records: the total stays, the records are the first 1,000."""
    for x in states:
        what = f"state {x.index} {x.scene.fmt}"
        lists = lc.HostLists(lc.harness(), x.case)
        try:
            for (name, flags), exp in x.blocks.lists.items():
                got, total = lists.list(*x.inputs.list_boxes[name], flags)
                assert total == len(exp) and lc.differing(got, exp) is None, f"{what} {name} flags {flags}: total {total} of {len(exp)}; {lc.differing(got, exp)}"
            exp = x.blocks.lists[sc.CUT_BOX, sc.EXPOSED_FACES]
            got, total, _ = lists.buffer(*x.inputs.list_boxes[sc.CUT_BOX], sc.EXPOSED_FACES, sc.CUT)
            assert len(exp) > sc.CUT and total == len(exp) and lc.differing(got, exp[:sc.CUT]) is None, f"{what} cut: {lc.differing(got, exp[:sc.CUT])}"
        finally:
            lists.close()


def test_the_ray_set_on_the_host_is_the_oracles(states, devhost, tracehost):  # noqa: F811
    """vxd::intersect (vx_device.hpp) and vx_trace.hpp on the host over the ray set: vx_ray_hit and vx_hit records byte for byte, colours within
    trace_cases.TOL."""
    for x in states:
        c, inp, exp = x.scene, x.inputs, x.expected
        frame, mats, chain, n_levels, level_offset = tc.scene_arguments(c)
        o, d, m = (np.array(a, order="C") for a in (inp.o, inp.d, inp.m))
        got = np.zeros(len(o), dtype=hip.RAY_HIT_DTYPE)
        devhost.devhost_ray_batch(c.svo_type, frame.ctypes.data_as(_vp), C.c_uint64(frame.size * 4), mats.ctypes.data_as(_vp), len(mats), chain.ctypes.data_as(_vp),
                                  c.tex.shape[2], c.tex.shape[1], c.tex.shape[0], n_levels, level_offset, o.ctypes.data_as(_vp), d.ctypes.data_as(_vp),
                                  m.ctypes.data_as(_vp), len(o), 0, got.ctypes.data_as(_vp))
        what = f"state {x.index} {c.fmt}"
        first_difference(got, exp.hits, what + " ray batch on the host", lambda i: f"ray {i} ({inp.kinds[i]}): origin {inp.o[i]!r} dir {inp.d[i]!r} max_dst {inp.m[i]!r}")
        rgba, rgba8, hits = trace_on_host(tracehost, c, inp.free_u, inp.o, inp.d, inp.m)
        tc.assert_records(hits, exp.trace, what + " trace_rays on the host")
        tc.assert_colors(rgba, exp.color, what + " trace_rays on the host")
        assert (rgba8 == tc.pack_rgba8(rgba)).all()


class _Views:
    def __init__(self, scene, inp):
        self.svo_type, self.world, self.tex, self.mats = scene.svo_type, scene.world, scene.tex, scene.mats
        self.views, self.width, self.height = inp.views, sc.W, sc.H


def test_the_views_on_the_host_are_the_oracles_renders(states, viewshost):  # noqa: F811
    for x in states:
        rgba, rgba8, hits, writes, (left, stray, groups) = views_on_host(viewshost, _Views(x.scene, x.inputs), hip.VX_FORMAT_RGBA32F)
        assert stray == 0 and (writes == 1).all() and left == 0  # (64 x 48: whole tiles only)
        for k in range(2):
            tc.assert_records(hits[k], x.expected.view_hits[k].reshape(-1), f"state {x.index} {x.scene.fmt} view {k} on the host")
            tc.assert_colors(rgba[k], x.expected.imgs[k], f"state {x.index} {x.scene.fmt} view {k} on the host")


def test_the_entities_on_the_host_step_as_the_oracle_steps_them(states, physhost):  # noqa: F811
    """vx_physics.hpp on the host: 8 single steps, records and contacts after every one; 8 steps in one call."""
    for x in states:
        c, inp, exp = x.scene, x.inputs, x.expected
        frame, mats, chain, n_levels, level_offset = tc.scene_arguments(c)
        what = f"state {x.index} {c.fmt}"
        describe = lambda i: f"entity {i} ({next(r for r, idx in inp.roles.items() if i in idx)}): start {inp.rows[i]!r}"  # noqa: E731
        e = hip.entities_from_rows(inp.rows)
        for step, (rows, contacts) in enumerate(exp.run):
            got = np.zeros(len(e), dtype=hip.AABB_RESULT_DTYPE)
            host_step(physhost, c.svo_type, frame, mats, chain, c.tex, n_levels, level_offset, e, DT, 1, got)
            first_difference(got.view(np.float32).reshape(-1, 6), contacts, f"{what} contacts of step {step}", describe)
            first_difference(hip.entities_to_rows(e), rows, f"{what} records after step {step}", describe)
        many = hip.entities_from_rows(inp.rows)
        got = np.zeros(len(many), dtype=hip.AABB_RESULT_DTYPE)
        host_step(physhost, c.svo_type, frame, mats, chain, c.tex, n_levels, level_offset, many, DT, sc.STEPS, got)
        first_difference(hip.entities_to_rows(many), exp.run[-1][0], f"{what} records after {sc.STEPS} steps in one call", describe)
        first_difference(got.view(np.float32).reshape(-1, 6), exp.run[-1][1], f"{what} contacts of {sc.STEPS} steps in one call", describe)
