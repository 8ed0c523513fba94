"""vx_block_points' and vx_read_region's lookup without a GPU: voxel-rs_amd/csrc/blocks/vx_blocks.hpp compiled for the host by the stand-alone
harness tests/cpp/blocks_on_host.cpp, against the dense arrays the worlds of tests/blocks_cases.py were built from -- both worlds, both formats.
test_blocks.py holds the GPU's records against the harness's, byte for byte."""
import numpy as np
import pytest

from batch_cases import CASES
from blocks_cases import OUTSIDE, REGIONS, check_cells, classify, dense_region, harness, host_points, host_region, lod_voxel, make_block_case
from voxel_rs_amd import hip


@pytest.fixture(scope="module")
def exe():
    return harness()


@pytest.fixture(scope="module", params=CASES, ids=[f"{n}-{f}" for n, f in CASES])
def case(request):
    return make_block_case(*request.param)


def test_the_lod_rule_as_stated():
    """lod_voxel on hand-made cells: the sub-octant order [2,3,6,7,0,1,4,5] with the child index x | y << 1 | z << 2, then the same order inside."""
    cell = np.zeros((4, 4, 4), dtype=np.uint32)
    assert lod_voxel(cell) == 0
    cell[0, 0, 0] = 7  # sub-octant 0, child 0
    assert lod_voxel(cell) == 7
    cell[1, 1, 0] = 8  # sub-octant 0, child 3: before child 0
    assert lod_voxel(cell) == 8
    cell[3, 0, 3] = 9  # sub-octant 5: after sub-octant 0
    assert lod_voxel(cell) == 8
    cell[0, 2, 3] = 4  # sub-octant 6 (y high, z high), child 4: before sub-octant 0
    assert lod_voxel(cell) == 4
    cell[1, 3, 0] = 5  # sub-octant 2 (y high), child 3: the first of all
    assert lod_voxel(cell) == 5
    cell[0, 3, 0] = 6  # sub-octant 2, child 2: before child 3
    assert lod_voxel(cell) == 6


def test_the_point_set_holds_every_kind(case):
    """By the dense array alone. A seed that misses a threshold is changed; the threshold never is."""
    k, p = case.kinds, case.pts
    counts = {name: int(k[name].sum()) for name in ("solid", "air", "lod", "space", "outside", "integral")}
    print(f"\n{case.name}-{case.fmt}: {len(p)} points, {counts}, ids {sorted(int(v) for v in np.unique(k['value'][k['solid']]))}")
    assert 1500 <= len(p) <= 2500
    assert counts["solid"] >= 300 and len(np.unique(k["value"][k["solid"]])) >= 4
    assert counts["air"] >= 300
    if case.name == "far_chunks":
        assert counts["lod"] >= 100 and (k["lod"] & (k["value"] != 0)).sum() >= 30 and (k["lod"] & (k["value"] == 0)).sum() >= 30
    assert counts["space"] >= 100
    assert counts["outside"] >= 60
    size = np.float32(case.info["size"])
    assert np.isnan(p).any() and (p == np.inf).any() and (p == -np.inf).any() and (p == np.float32(-1e-30)).any() and (p == size).any()
    assert ((p == 0) & np.signbit(p)).any()
    assert not k["outside"][((p == 0) & np.signbit(p)).any(axis=1) & np.isfinite(p).all(axis=1) & (p >= 0).all(axis=1) & (p < size).all(axis=1)].any()
    assert counts["integral"] >= 60


def test_points_against_the_dense_array(case, exe):
    """Every point's value; cell_log2 0 / 2 / VX_CELL_OUTSIDE; an empty cell is aligned, holds the point and is all air."""
    cells = host_points(exe, case, case.pts, 12, len(case.pts))
    assert len(cells) == len(case.pts)
    check_cells(case, cells)
    k = case.kinds
    assert (cells["value"][k["outside"]] == 0).all() and (cells["cell_log2"][k["outside"]] == OUTSIDE).all()
    if case.name == "far_chunks":  # the empty space of a deep world ends high above the voxels
        assert cells["cell_log2"][k["space"]].max() >= 10


def test_strided_points_are_the_packed_ones(case, exe):
    """The same points inside vx_entity records (stride 64) and inside vx_ray_hit records (pos at offset 16, stride 32): the same records."""
    n = len(case.pts)
    plain = host_points(exe, case, case.pts, 12, n)
    e = np.zeros(n, dtype=hip.ENTITY_DTYPE)
    e["position"], e["velocity"] = case.pts, 3.0
    assert host_points(exe, case, e, 64, n).tobytes() == plain.tobytes()
    h = np.full(n, 0x5a, dtype=np.uint8).repeat(32).view(hip.RAY_HIT_DTYPE)
    h["pos"] = case.pts
    assert host_points(exe, case, h.view(np.uint8)[16:], 32, n).tobytes() == plain.tobytes()


def test_regions_against_the_dense_array(case, exe):
    """The region routine, brick by brick as the kernel runs it: glasshouse's whole world with a margin of 3 (lo = -3, 70^3); the 75 x 37 x 77 box
    at an odd corner over all four far chunks; and small boxes: one voxel, a row across a brick boundary, a box wholly outside the world."""
    lo, size = REGIONS[case.name]
    got = host_region(exe, case, lo, size)
    exp = dense_region(case.info, case.truth, lo, size)
    assert exp.any() and (got == exp).all(), np.argwhere(got != exp)[:8]
    if case.name == "glasshouse":
        assert (got[3:67, 3:67, 3:67] == np.pad(case.truth, ((0, 32),) * 3).transpose(2, 1, 0)).all() and not got[:3].any() and not got[:, :, 67:].any()
    solid = np.argwhere(case.truth != 0)[0] + case.info["lo"]
    for blo, bsize in ((tuple(solid), (1, 1, 1)), ((int(solid[0]) // 8 * 8 - 4, int(solid[1]), int(solid[2])), (9, 1, 1)), ((-40, -9, 3), (8, 9, 3)),
                       ((int(case.info["size"]), 0, 0), (5, 4, 3))):
        got = host_region(exe, case, blo, bsize)
        assert (got == dense_region(case.info, case.truth, blo, bsize)).all(), (blo, bsize)
    assert host_region(exe, case, tuple(solid), (1, 1, 1))[0, 0, 0] == case.truth[tuple(solid - case.info["lo"])] != 0


def test_a_regions_voxels_are_the_points_at_their_centres(case, exe):
    """Every voxel of a box around the chunks' corner, asked as a point at its centre, gives the region's value."""
    lo = tuple(int(v) - 5 for v in case.info["lo"] + (np.asarray(case.truth.shape) // 2 if case.name == "far_chunks" else 0))
    size = (13, 11, 9)
    region = host_region(exe, case, lo, size)
    z, y, x = np.meshgrid(np.arange(size[2]), np.arange(size[1]), np.arange(size[0]), indexing="ij")
    centres = np.ascontiguousarray(np.stack([x + lo[0] + 0.5, y + lo[1] + 0.5, z + lo[2] + 0.5], axis=-1).reshape(-1, 3).astype(np.float32))
    cells = host_points(exe, case, centres, 12, len(centres))
    inside = ~classify(case.info, case.truth, centres)["outside"]
    assert (cells["value"] == region.reshape(-1)).all() and not region.reshape(-1)[~inside].any()


def test_the_rules_refuse_what_the_abi_lists(exe):
    """vx_blocks.hpp's argument rules on their own: each bad value named by its field, what is allowed allowed."""
    import subprocess

    out = subprocess.run([str(exe), "rules"], stdout=subprocess.PIPE, text=True, check=True).stdout
    said = dict(ln.split(": ", 1) for ln in out.splitlines())
    for ok in ("packed", "entity", "nothing", "nothing at a bad stride", "region", "region none"):
        assert said[ok] == "ok", (ok, said[ok])
    for stride in (0, 4, 8, 13, 14, 18):
        assert "pos_stride" in said[f"stride {stride}"]
    assert "pos must be aligned" in said["misaligned"] and said["null pos"] == "null pos" and said["null out"] == "null out" and "count" in said["too many"]
    assert "size.x * size.y * size.z" in said["region big"] and "size.x * size.y * size.z" in said["region huge"]
    assert said["null lo"] == "null lo" and said["null size"] == "null size"
