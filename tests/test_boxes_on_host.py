"""vx_overlap_boxes' answer without a GPU: voxel-rs_amd/csrc/blocks/vx_boxes.hpp compiled for the host by the stand-alone harness
tests/cpp/boxes_on_host.cpp -- box by box and brick by brick as the kernel runs it -- against the numpy records of tests/boxes_cases.py over
the dense arrays the worlds were built from: all three worlds, both formats, every box in every form, byte for byte; and the same program built
with AddressSanitizer and UndefinedBehaviorSanitizer (with the float-to-integer conversion check) on the named boxes and the seeded set of
`tower`. test_boxes.py holds the GPU's records against the harness's."""
import subprocess

import numpy as np
import pytest

from boxes_cases import (INVALID, SCAN_CASES, SEEDED, Boxes, HostBoxes, absent_id, boxes_truth, calls_for, commonest_id, cover_of, differing, harness,
                         make_boxes, make_scan_case)
from voxel_rs_amd import hip


@pytest.fixture(scope="module")
def exe():
    return harness()


@pytest.fixture(scope="module", params=SCAN_CASES, ids=[f"{n}-{f}" for n, f in SCAN_CASES])
def case(request, exe):
    c = make_scan_case(*request.param)
    c.host = HostBoxes(exe, c)
    c.boxes = make_boxes(c)
    c.expected = boxes_truth(c, c.boxes)
    c.expected.setflags(write=False)
    yield c
    c.host.close()


def test_the_boxes_hold_what_the_tests_need(case):
    """By the dense arrays alone. A set that misses a threshold is changed (its seed, the grown box); the threshold never is."""
    b, exp = case.boxes, case.expected
    seeded = exp[b.seeded]
    some, none = float((seeded["blocks"] > 0).mean()), float((seeded["blocks"] == 0).mean())
    print(f"\n{case.name}-{case.fmt}: seeded set {some:.1%} with blocks, {none:.1%} without; largest count {int(seeded['blocks'].max())}")
    assert len(seeded) == SEEDED and (seeded["blocks"] != INVALID).all()
    assert some >= 0.5 and none >= 0.1
    named = {name: exp[i] for name, i in b.names.items()}
    # resting on a block is no overlap; 2^-10 lower is
    assert float(b.origin[b.names["resting"]][1]).is_integer() and named["resting"]["blocks"] == 0
    assert named["sunk"]["blocks"] == 1 and named["sunk"]["value"] != 0
    assert list(named["sunk"]["hi"] - named["sunk"]["lo"]) == [1, 1, 1] and named["sunk"]["hi"][1] == int(b.origin[b.names["resting"]][1])
    assert named["one_voxel"]["blocks"] == 1
    first, last = cover_of(case, b.origin[b.names["eight_bricks"]], b.offset[b.names["eight_bricks"]], b.extents[b.names["eight_bricks"]])
    assert [h - l + 1 for l, h in zip(first, last)] == [9, 9, 9] and all(l % 8 == 4 for l in first)  # two bricks on every axis
    print({name: int(r["blocks"]) for name, r in named.items() if r["blocks"] != INVALID})
    assert named["widest"]["blocks"] >= 1000
    assert named["world_edge_near"]["blocks"] >= 1 and list(named["world_edge_near"]["lo"]) == [0, 0, 0] if case.name != "far_chunks" else named["world_edge_near"]["blocks"] == 0
    for name in ("outside_below", "outside_above", "outside_one_axis", "touching_edge", "far_x", "far_negative", "far_huge", "far_all", "far_max"):
        assert named[name].tobytes() == bytes(32), name
    if case.name == "tower":
        assert named["lod_seam"]["lo"][2] < 32 < named["lod_seam"]["hi"][2] and named["lod_leaves"]["blocks"] >= 1000
    assert len(b.invalid) >= 45
    for i in b.invalid:
        assert exp[i]["blocks"] == INVALID and exp[i].tobytes()[4:] == bytes(28), i
    assert commonest_id(case) != 0 and not (case.truth == absent_id(case)).any()


def test_every_box_in_every_form_against_the_dense_array(case):
    """Every form, and the packed form with only_value the commonest id and an id that occurs nowhere."""
    for name, boxes, only_value in calls_for(case, case.boxes):
        exp = case.expected if (boxes.form, only_value) == ("packed", 0) else boxes_truth(case, boxes, only_value)
        got = case.host.records(boxes, only_value)
        assert differing(got, exp) is None, f"{name}: {differing(got, exp)}"
        valid = exp["blocks"] != INVALID
        if name == "absent":
            assert (exp["blocks"][valid] == 0).all() and valid.sum() == (case.expected["blocks"] != INVALID).sum()
        if name == "commonest":
            assert (exp["value"][valid & (exp["blocks"] > 0)] == only_value).all() and (exp["blocks"][valid] > 0).mean() >= 0.1
            assert (exp["blocks"][valid] <= case.expected["blocks"][valid]).all() and (exp["blocks"][valid] < case.expected["blocks"][valid]).any()
        if name == "entities":
            assert exp.tobytes() == case.expected.tobytes()


def test_one_box_and_no_box(case):
    b = case.boxes
    one = Boxes(b.origin[7:8], b.offset[7:8], b.extents[7:8], "packed")
    assert case.host.records(one).tobytes() == case.expected[7:8].tobytes()
    none = Boxes(b.origin[:0], b.offset[:0], b.extents[:0], "entities")
    assert len(case.host.records(none)) == 0


def test_the_bounds_hold_the_count(case):
    """What the record says of itself: the counted voxels lie within [lo, hi), which lies within the cover and the world; a count of 1 is a
    box of one voxel; the first value is a block's."""
    exp = case.host.records(case.boxes)
    some = (exp["blocks"] != INVALID) & (exp["blocks"] > 0)
    ext = (exp["hi"] - exp["lo"]).astype(np.int64)
    assert (ext[some] >= 1).all() and (ext[some].prod(axis=1) >= exp["blocks"][some]).all()
    assert (exp["lo"][some] >= 0).all() and (exp["hi"][some] <= case.size).all()
    assert (ext[some & (exp["blocks"] == 1)] == 1).all() and (exp["value"][some] != 0).all()
    assert (exp["value"][~some] == 0).all() and (ext[~some] == 0).all()


def test_the_sanitized_program_on_tower(exe):
    """The same program under -fsanitize=address,undefined -fsanitize=float-cast-overflow -fno-sanitize-recover=all, run directly: the named
    boxes -- 3e9, -3e9, 1e30 and FLT_MAX among them --, the records that are no box and the seeded set of `tower`, both formats, every form. A
    finding ends the program with a non-zero status; its records are the plain program's."""
    san = harness(sanitize=True)
    for fmt in ("esvo", "csvo"):
        c = make_scan_case("tower", fmt)
        plain, checked = HostBoxes(exe, c), HostBoxes(san, c)
        try:
            boxes = make_boxes(c)
            for name, b, only_value in calls_for(c, boxes):
                assert checked.records(b, only_value).tobytes() == plain.records(b, only_value).tobytes(), (fmt, name)
        finally:
            plain.close()
            checked.close()


def test_the_rules_refuse_what_the_abi_lists(exe):
    """vx_boxes.hpp's argument rules on their own: each bad value named by its field, what is allowed allowed."""
    out = subprocess.run([str(exe), "rules"], stdout=subprocess.PIPE, text=True, check=True).stdout
    said = dict(ln.split(": ", 1) for ln in out.splitlines())
    for ok in ("packed", "no offset", "one offset, one extents", "entities", "count 0"):
        assert said[ok] == "ok", (ok, said[ok])
    assert said["too many"].startswith("count exceeds 16777216")
    assert said["null boxes"] == "null boxes" and said["null out"] == "null out" and said["null origin"] == "null origin" and said["null extents"] == "null extents"
    for stride in (0, 4, 8, 13, 14):
        assert said[f"origin_stride {stride}"].startswith("origin_stride"), stride
    for stride in (4, 8, 13, 18):
        assert said[f"offset_stride {stride}"].startswith("offset_stride") and said[f"extents_stride {stride}"].startswith("extents_stride"), stride
    for off in (1, 2, 3):
        for field in ("origin", "offset", "extents"):
            assert said[f"{field} + {off}"].startswith(f"{field} must be aligned"), (field, off)
    assert hip.BOX_HIT_DTYPE.itemsize == 32
