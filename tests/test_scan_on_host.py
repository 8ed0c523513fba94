"""vx_scan_points' and vx_scan_columns' walk without a GPU: voxel-rs_amd/csrc/blocks/vx_scan.hpp compiled for the host by the stand-alone
harness tests/cpp/scan_on_host.cpp, against the numpy truth of tests/scan_cases.py over the dense arrays the worlds were built from -- all
three worlds, both formats, all six directions, every point and box. test_scan.py holds the GPU's records against the harness's, byte for
byte."""
import subprocess

import numpy as np
import pytest

import blocks_cases
from scan_cases import (DIR_NAMES, DIRECTIONS, GAP, NONE, OUTSIDE, REACHES, SCAN_CASES, TO_EDGE, axes_of, boxes_for, columns_truth, differing, first_of_region,
                        harness, host_scan_columns, host_scan_points, make_scan_case, points_truth, skipping_box)
from voxel_rs_amd import hip


@pytest.fixture(scope="module")
def exe():
    return harness()


@pytest.fixture(scope="module", params=SCAN_CASES, ids=[f"{n}-{f}" for n, f in SCAN_CASES])
def case(request):
    return make_scan_case(*request.param)


def same_fields(got, exp, what):
    """Field for field -- coord, value, cell_log2, _pad == 0 --, then the bytes."""
    for f in ("coord", "value", "cell_log2"):
        bad = np.argwhere(got[f] != exp[f])
        assert not len(bad), f"{what}: {len(bad)} records differ in {f}, first at {tuple(bad[0])}: got {got[tuple(bad[0])]} expected {exp[tuple(bad[0])]}"
    assert not got["_pad"].any(), what
    assert differing(got, exp) is None, what


def test_the_point_set_holds_every_kind(case):
    """By the dense arrays alone. A seed that misses a threshold is changed; the threshold never is."""
    g, p = case.groups, case.pts
    counts = {k: len(v) for k, v in g.items()}
    print(f"\n{case.name}-{case.fmt}: {len(p)} points, {counts}")
    assert 1200 <= len(p) <= 1800
    for name, least in (("above", 300), ("solid", 260), ("covered", 200), ("space", 150), ("outside", 120), ("integral", 100), ("special", 72)):
        assert counts[name] >= least, name
    if case.name != "glasshouse":
        assert counts["lod_inner"] >= 200 and counts["lod"] >= 100
    assert np.isnan(p).any() and (p == np.inf).any() and (p == -np.inf).any() and (p == np.float32(3e38)).any() and (p == np.float32(-3e38)).any()
    assert ((p == 0) & np.signbit(p)).any()
    down, up = points_truth(case, p, hip.VX_DIR_NEG_Y, TO_EDGE), points_truth(case, p, hip.VX_DIR_POS_Y, TO_EDGE)
    floor_y = np.floor(p[:, 1].astype(np.float64))
    assert (down["coord"][g["above"]] < floor_y[g["above"]]).all() and (down["value"][g["above"]] != 0).all()  # the ground lies below them
    assert (down["coord"][g["solid"]] == floor_y[g["solid"]]).all() and (down["cell_log2"][g["solid"]] == 0).all()  # the start voxel counts
    assert (up["coord"][g["covered"]] > floor_y[g["covered"]]).all()  # something lies above them
    if "lod_inner" in g:
        assert (down["coord"][g["lod_inner"]] == floor_y[g["lod_inner"]]).all() and (down["cell_log2"][g["lod_inner"]] >= 2).all()
    entering = sum(int((points_truth(case, p[g["outside"]], d, TO_EDGE)["coord"] != NONE).sum()) for d in DIRECTIONS)
    assert entering >= 20, entering  # scans that start outside the world and find a block in it
    assert (down["cell_log2"][~np.isfinite(p).all(axis=1)] == OUTSIDE).all() and (down["cell_log2"][np.isfinite(p).all(axis=1)] != OUTSIDE).all()


@pytest.mark.parametrize("direction", DIRECTIONS, ids=DIR_NAMES)
def test_points_against_the_dense_array(case, exe, direction):
    """Every point at reaches 1, 2 and VX_SCAN_TO_EDGE; the gap points at a reach that ends one voxel short of the block (none) and on it."""
    for reach in REACHES:
        got, trips = host_scan_points(exe, case, case.pts, 12, len(case.pts), direction, reach)
        same_fields(got, points_truth(case, case.pts, direction, reach), f"{DIR_NAMES[direction]} reach {reach}")
        assert trips.max() <= (4 if reach <= 2 else 64)
    gaps = case.gaps[direction]
    short, _ = host_scan_points(exe, case, gaps, 12, len(gaps), direction, GAP)
    exact, _ = host_scan_points(exe, case, gaps, 12, len(gaps), direction, GAP + 1)
    same_fields(short, points_truth(case, gaps, direction, GAP), "one voxel short")
    same_fields(exact, points_truth(case, gaps, direction, GAP + 1), "exactly on the block")
    a, _, _, positive = axes_of(direction)
    assert (short["coord"] == NONE).all() and (exact["coord"] == np.floor(gaps[:, a]) + (GAP if positive else -GAP)).all() and (exact["value"] != 0).all()


def test_strided_points_are_the_packed_ones(case, exe):
    """The same points inside vx_entity records (stride 64) and inside vx_ray_hit records (pos at offset 16, stride 32): the same records."""
    n = len(case.pts)
    plain, _ = host_scan_points(exe, case, case.pts, 12, n, hip.VX_DIR_NEG_Y, TO_EDGE)
    e = np.zeros(n, dtype=hip.ENTITY_DTYPE)
    e["position"], e["velocity"] = case.pts, 3.0
    assert host_scan_points(exe, case, e, 64, n, hip.VX_DIR_NEG_Y, TO_EDGE)[0].tobytes() == plain.tobytes()
    h = np.full(n, 0x5a, dtype=np.uint8).repeat(32).view(hip.RAY_HIT_DTYPE)
    h["pos"] = case.pts
    assert host_scan_points(exe, case, h.view(np.uint8)[16:], 32, n, hip.VX_DIR_NEG_Y, TO_EDGE)[0].tobytes() == plain.tobytes()


@pytest.mark.parametrize("direction", DIRECTIONS, ids=DIR_NAMES)
def test_boxes_against_the_dense_array(case, exe, direction):
    """The columns routine, tile by tile as the kernel runs it, on every box of scan_cases.boxes_for."""
    boxes = boxes_for(case, direction)
    assert len(boxes) == (9 if (case.cell >= 2).any() else 8)
    seen = {}
    for name, lo, size in boxes:
        got, _ = host_scan_columns(exe, case, lo, size, direction)
        exp = columns_truth(case, lo, size, direction)
        same_fields(got, exp, f"{name} {lo} {size} {DIR_NAMES[direction]}")
        seen[name] = exp
    assert (seen["1x1"]["coord"] != NONE).all() and (seen["9x1"]["coord"] != NONE).any()
    assert (seen["outside"]["coord"] == NONE).all() and (seen["beside"]["coord"] == NONE).all()
    assert seen["short"][2, 2]["coord"] == NONE and seen["exact"][2, 2]["coord"] != NONE
    if "in_lod" in seen:
        inside = seen["in_lod"]["cell_log2"] >= 2
        a, _, _, positive = axes_of(direction)
        lo, size = next((lo, size) for name, lo, size in boxes if name == "in_lod")
        start = lo[a] if positive else lo[a] + size[a] - 1
        assert (seen["in_lod"]["coord"][inside] == start).any()  # a scan that starts inside a LOD voxel answers with its start
    assert any((seen[n]["cell_log2"] > 0).any() for n in seen) == bool((case.cell > 0).any())


@pytest.mark.parametrize("direction", DIRECTIONS, ids=DIR_NAMES)
def test_the_truth_is_the_first_block_of_the_region(case, direction):
    """The numpy truth against code that is already trusted: the first non-zero, in travel order, of the block harness's host_region
    (tests/cpp/blocks_on_host.cpp) over the same box."""
    _, lo, size = boxes_for(case, direction)[2]
    block_case = blocks_cases.BlockCase()
    block_case.frame, block_case.svo_type = case.frame, case.svo_type
    region = blocks_cases.host_region(blocks_cases.harness(), block_case, lo, size)
    coord, value = first_of_region(region, lo, direction)
    exp = columns_truth(case, lo, size, direction)
    assert (exp["coord"] == coord).all() and (exp["value"] == value).all() and (exp["coord"] != NONE).any()


@pytest.mark.parametrize("fmt", ["esvo", "csvo"])
def test_empty_space_is_stepped_over(exe, fmt):
    """far_chunks, depth 14: a full-height VX_DIR_NEG_Y scan of the four chunks' footprint plus a margin of 8 -- as one box, and as one point a
    column at the world's top -- takes no more than 64 loop trips in any tile and any column; voxel by voxel it would take 16,384. The cap
    is a condition that keeps a linear walk from passing, not a measurement. Measured on the CPU, both formats: at most 11 trips a tile (mean 9.9) and 25 a column (mean 12.8)."""
    c = make_scan_case("far_chunks", fmt)
    lo, size = skipping_box(c)
    got, tile_trips = host_scan_columns(exe, c, lo, size, hip.VX_DIR_NEG_Y)
    same_fields(got, columns_truth(c, lo, size, hip.VX_DIR_NEG_Y), "the footprint")
    z, x = np.meshgrid(np.arange(size[2]), np.arange(size[0]), indexing="ij")
    tops = np.ascontiguousarray(np.stack([x + lo[0] + 0.5, np.full(x.shape, c.size - 0.5), z + lo[2] + 0.5], axis=-1).reshape(-1, 3).astype(np.float32))
    per_point, point_trips = host_scan_points(exe, c, tops, 12, len(tops), hip.VX_DIR_NEG_Y, TO_EDGE)
    assert per_point.tobytes() == got.tobytes()  # (the same columns, asked both ways)
    print(f"\nfar_chunks-{fmt}: loop trips a tile: max {tile_trips.max()}, mean {tile_trips.mean():.1f}; a column: max {point_trips.max()}, mean {point_trips.mean():.1f}")
    assert len(tile_trips) == 10 * 10 and (got["coord"] != NONE).sum() == 64 * 64
    assert 1 <= tile_trips.max() <= 64 and 1 <= point_trips.max() <= 64


def test_the_rules_refuse_what_the_abi_lists(exe):
    """vx_scan.hpp's argument rules on their own: each bad value named by its field, what is allowed allowed."""
    out = subprocess.run([str(exe), "rules"], stdout=subprocess.PIPE, text=True, check=True).stdout
    said = dict(ln.split(": ", 1) for ln in out.splitlines())
    for ok in ("packed", "entity", "nothing", "nothing at a bad stride", "columns", "columns none", "columns flat"):
        assert said[ok] == "ok", (ok, said[ok])
    for stride in (0, 4, 8, 13, 14, 18):
        assert "pos_stride" in said[f"stride {stride}"]
    assert "pos must be aligned" in said["misaligned"] and said["null pos"] == "null pos" and said["null out"] == "null out" and "count" in said["too many"]
    assert "reach" in said["no reach"] and "direction" in said["nothing in no direction"]
    for d in (-1, 6, 255):
        assert "direction" in said[f"points direction {d}"] and "direction" in said[f"columns direction {d}"]
    for name in ("columns wide", "columns wide along x", "columns deep across"):
        assert said[name].startswith("size") and "columns" in said[name], name
    assert said["columns deep"].startswith("size") and "along the scan axis" in said["columns deep"]
    assert said["null lo"] == "null lo" and said["null size"] == "null size"
