"""vx_list_region's list without a GPU: voxel-rs_amd/csrc/blocks/vx_list.hpp compiled for the host by the stand-alone harness
tests/cpp/list_on_host.cpp -- count, prefix and write, brick by brick as the kernels run it -- against the numpy lists of tests/list_cases.py
over the dense arrays the worlds were built from: all three worlds, both formats, every box and flag set, byte for byte. test_list.py holds
the GPU's records against the harness's."""
import subprocess

import numpy as np
import pytest

import blocks_cases
from list_cases import (EXPOSED, FACES, FLAG_SETS, MAIN_BOXES, SCAN_CASES, HostLists, boxes_for, differing, expected_list, expected_parts, harness, make_scan_case,
                        merged, rebased, split_at)
from voxel_rs_amd import hip


@pytest.fixture(scope="module")
def exe():
    return harness()


@pytest.fixture(scope="module", params=SCAN_CASES, ids=[f"{n}-{f}" for n, f in SCAN_CASES])
def case(request, exe):
    c = make_scan_case(*request.param)
    c.host = HostLists(exe, c)
    yield c
    c.host.close()


def test_the_boxes_hold_what_the_tests_need(case):
    """By the dense arrays alone. A box that misses a threshold is changed; the threshold never is."""
    boxes = {name: (lo, size) for name, lo, size in boxes_for(case)}
    lo, size = boxes["main"]
    assert (lo, size) == MAIN_BOXES[case.name]
    plain, faced, seen = (expected_list(case, lo, size, f) for f in FLAG_SETS)
    _, faces = hip.split_where(faced["where"])
    per_face = [int(((faces >> f) & 1).sum()) for f in range(6)]
    buried = int((faces == 0).sum())
    print(f"\n{case.name}-{case.fmt}: {len(plain)} records, {len(seen)} exposed, {buried} buried, per face {per_face}, {len(np.unique(plain['value']))} ids")
    assert len(plain) == len(faced) >= 1500 and len(seen) >= 1500 and len(seen) == len(plain) - buried
    assert min(per_face) >= 80
    if case.name != "glasshouse":
        assert buried >= 20000 and len(np.unique(plain["value"])) >= 8
    assert (plain["value"] != 0).all() and (plain["where"] >> 24 == 0).all() and (faced["where"] >> 30 == 0).all()
    # the small boxes catch what they are named for
    assert len(expected_list(case, *boxes["one_voxel"], 0)) == 1 and len(expected_list(case, *boxes["9x1x1"], 0)) >= 1
    assert not len(expected_list(case, *boxes["outside"], 0)) and not len(expected_list(case, *boxes["outside_negative"], 0))
    for name in ("grid8", "grid16", "grid24", "off_grid", "inner"):
        assert len(expected_list(case, *boxes[name], 0)) >= 50, name
    # inner: a record on each of the box's x sides whose neighbour beyond that side, outside the box, holds a block
    ilo, isize = boxes["inner"]
    x, _, _, _, f, _ = expected_parts(case, ilo, isize, FACES)
    assert ((x == ilo[0]) & (f & 1 == 0)).any() and ((x == ilo[0] + isize[0] - 1) & (f & 2 == 0)).any()
    if case.name != "far_chunks":  # blocks at the world's edge: the side towards it is open
        x, y, z, _, f, _ = expected_parts(case, *boxes["world_edge"], FACES)
        assert ((x == 0) & (f & 1 != 0)).sum() >= 10 and ((y == 0) & (f & 4 != 0)).sum() >= 10 and ((z == 0) & (f & 16 != 0)).sum() >= 10
    if case.name == "tower":
        _, _, z, _, f, _ = expected_parts(case, *boxes["lod_seam"], FACES)
        assert (z == 31).sum() >= 50 and (z == 32).sum() >= 50 and ((z == 31) & (f & 32 == 0)).any() and ((z == 32) & (f & 16 == 0)).any()
        x, y, z, _, f, _ = expected_parts(case, *boxes["lod1_chunk"], FACES)
        assert len(x) >= 1000 and (f == 0).any() and ((y == 127) & (f & 8 != 0)).sum() == (y == 127).sum()


@pytest.mark.parametrize("flags", FLAG_SETS, ids=["plain", "faces", "exposed"])
def test_every_box_against_the_dense_array(case, flags):
    for name, lo, size in boxes_for(case):
        got, total = case.host.list(lo, size, flags)
        exp = expected_list(case, lo, size, flags)
        assert total == len(exp), (name, total, len(exp))
        assert differing(got, exp) is None, f"{name} {lo} {size}: {differing(got, exp)}"


def test_exposed_alone_implies_faces(case):
    for name, lo, size in boxes_for(case)[:3]:
        alone, both = case.host.list(lo, size, EXPOSED), case.host.list(lo, size, EXPOSED | FACES)
        assert alone[1] == both[1] and alone[0].tobytes() == both[0].tobytes(), name


def test_capacity_cuts_the_list_and_nothing_else(case):
    """capacity 0, 1, total - 1, total and total + 7: the prefix is written, the rest of the buffer left alone, the total the same."""
    for name, lo, size in boxes_for(case):
        for flags in (0, EXPOSED):
            whole, total = case.host.list(lo, size, flags)
            for capacity in sorted({0, 1, max(total - 1, 0), total, total + 7}):
                buf, again, _ = case.host.buffer(lo, size, flags, capacity)
                n = min(total, capacity)
                assert again == total and buf[:n].tobytes() == whole[:n].tobytes(), (name, flags, capacity)
                assert (buf[n:].view(np.uint8) == 0x5a).all(), (name, flags, capacity)


def test_the_plain_list_scattered_is_the_region(case):
    """Against code that is already trusted: the block harness's host_region (tests/cpp/blocks_on_host.cpp) over the same box."""
    block_case = blocks_cases.BlockCase()
    block_case.frame, block_case.svo_type = case.frame, case.svo_type
    for name, lo, size in boxes_for(case):
        got, _ = case.host.list(lo, size, 0)
        dense = np.zeros(size[0] * size[1] * size[2], dtype=np.uint32)
        dense[got["where"]] = got["value"]
        assert len(np.unique(got["where"])) == len(got)
        assert dense.tobytes() == blocks_cases.host_region(blocks_cases.harness(), block_case, lo, size).tobytes(), name


@pytest.mark.parametrize("axis", [0, 1, 2], ids=["x", "y", "z"])
def test_two_boxes_that_tile_a_third_give_its_list(case, axis):
    """The main box split at a plane that is no multiple of 8: the two lists, re-based and merged by the key, are the whole box's -- the face
    bits of the voxels at the seam included, which each part judges by the world beyond its own box."""
    lo, size = MAIN_BOXES[case.name]
    cut = int(np.median(expected_parts(case, lo, size, 0)[axis]))  # through the middle of the blocks (the dense array's), off the brick grid
    cut += 1 if cut % 8 == 0 else 0
    assert cut % 8 and lo[axis] < cut < lo[axis] + size[axis]
    for flags in FLAG_SETS:
        whole, _ = case.host.list(lo, size, flags)
        parts = [rebased(case.host.list(plo, psize, flags)[0], plo, psize, lo, size) for plo, psize in split_at(lo, size, axis, cut)]
        assert all(len(p[0]) for p in parts)
        assert differing(merged(parts), whole) is None, (flags, differing(merged(parts), whole))


def test_the_rules_refuse_what_the_abi_lists(exe):
    """vx_list.hpp's argument rules on their own: each bad value named by its field, what is allowed allowed."""
    out = subprocess.run([str(exe), "rules"], stdout=subprocess.PIPE, text=True, check=True).stdout
    said = dict(ln.split(": ", 1) for ln in out.splitlines())
    for ok in ("plain", "faces", "exposed", "exposed faces", "count only", "no voxel"):
        assert said[ok] == "ok", (ok, said[ok])
    for flags in (4, 8, 7, 0x80000000, 0xFFFFFFFF):
        assert said[f"flags {flags}"].startswith("flags"), flags
    assert said["no voxel, bad flags"].startswith("flags")
    assert said["too large"].startswith("size.x * size.y * size.z")
    assert said["null lo"] == "null lo" and said["null size"] == "null size"
    assert said["null total"] == "null total" and said["null total, count only"] == "null total"
    assert said["null out"].startswith("null out")
