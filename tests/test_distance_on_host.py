"""vx_distance_boxes' answer without a GPU: voxel-rs_amd/csrc/blocks/vx_distance.hpp compiled for the host by the stand-alone harness
tests/cpp/distance_on_host.cpp -- box by box, the bricks, rows and the two passes the kernel's workgroup runs -- against the numpy fields and
records of tests/distance_cases.py, which come from the dense arrays the worlds were built from: five worlds, both formats, every shape, flag,
pass_value, match_value and stride, entry for entry and record for record; the truth's two ways against one another and against scipy; the
margin rule; and the same program built with AddressSanitizer and UndefinedBehaviorSanitizer. test_distance.py holds the GPU's bytes against
the harness's."""
import subprocess

import numpy as np
import pytest

from distance_cases import (ABSENT, BRUTE_CELLS, DISTANCE_CASES, NONE, SEVENTEEN, SHAPE, SHAPES, SMALL_PICK, TO_AIR, HostDistance, Shape, boxes_for, brute_force, calls_for, cells, derive,
                            differing, distance_field, distance_truth, harness, make_distance_case, match_id, named_at, pick_for, targets_of, the_call, truth_for, unpack)
from label_cases import RUBBLE_AT, SEEDED, SOLID_ROCK, regions_of
from voxel_rs_amd import hip


@pytest.fixture(scope="module")
def exe():
    return harness()


@pytest.fixture(scope="module", params=DISTANCE_CASES, ids=[f"{n}-{f}" for n, f in DISTANCE_CASES])
def case(request, exe):
    c = make_distance_case(*request.param)
    c.host = HostDistance(exe, c)
    yield c
    c.host.close()


@pytest.fixture(scope="module", params=["esvo", "csvo"])
def rubble(request, exe):
    c = make_distance_case("rubble", request.param)
    c.host = HostDistance(exe, c)
    yield c
    c.host.close()


def test_the_bit_function_and_the_pass(exe):
    """distance_row_x against a loop over the bits and distance_pass against its definition, on seeded words and lines of every length,
    with "none" entries: none stays none, nothing overflows, nothing beyond the line is written."""
    r = subprocess.run([str(exe), "lines"], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


def test_the_two_truths_agree(case):
    """The separable passes and the minimum over all target cells, for every call on a box of at most 12^3 cells, and on the corner of 12^3
    cells of the 17^3 boxes' regions."""
    seen = 0
    for call in calls_for(case):
        name, shape, pass_value, match_value, flags, _, _ = call
        if shape.voxels > BRUTE_CELLS:
            continue
        fields = cells(truth_for(case, call)[0], shape)
        target = targets_of(regions_of(case, boxes_for(case, shape)[pick_for(case, shape)], shape.size), pass_value, match_value, flags)
        for k in range(0, len(target), 3):
            assert (brute_force(target[k]) == fields[k]).all(), (name, k)
            seen += 1
    values = regions_of(case, case.boxes[:SEEDED:8], SEVENTEEN.size)[:, :12, :12, :12]
    for flags in (0, TO_AIR):
        target = targets_of(values, flags=flags)
        field = distance_field(target)
        for k in range(len(target)):
            assert (brute_force(target[k]) == field[k]).all(), (flags, k)
    assert seen >= 100


def test_the_boxes_hold_what_the_tests_need(case):
    """By the truth alone, among the seeded boxes at 17^3: boxes with a target, values above 2 -- a cell whose nearest target lies on no axis
    through it --, and records whose `where` is not cell 0; boxes without a target are among the named ones. (The conditions are `rubble`'s:
    the other worlds' figures are printed.)"""
    fields, info = truth_for(case, the_call(case, "17-solid"))
    fields, info = fields[:SMALL_PICK], info[:SMALL_PICK]
    inner = fields[:, :SEVENTEEN.voxels]
    figures = (int((info["targets"] > 0).sum()), int((info["targets"] == 0).sum()), int(((inner > 2) & (inner != NONE)).any(axis=1).sum()), int((info["where"] != 0).sum()))
    print(f"\n{case.name}-{case.fmt}: {figures[0]} boxes with a target, {figures[1]} without, {figures[2]} with a value above 2, {figures[3]} with where != 0")
    if case.name == "rubble":
        assert figures[0] >= SMALL_PICK // 2 and figures[2] >= SMALL_PICK // 4 and figures[3] >= SMALL_PICK // 4


def test_every_call_against_the_dense_array(case):
    """Every shape under the four kinds of target set and the strides in turn; the absent id and the complements at 17^3."""
    for call in calls_for(case):
        name, shape, pass_value, match_value, flags, lo_stride, field_stride = call
        expected = truth_for(case, call)
        got = case.host.call(case, call)
        assert differing(got, expected) is None, f"{name} (pass {pass_value}, match {match_value}, flags {flags}, strides {lo_stride}, {field_stride}): {differing(got, expected)}"
        fields, info = expected
        inner = fields[:, :shape.voxels]
        assert (fields[:, shape.voxels:] == NONE).all()
        assert ((inner == 0).sum(axis=1) == info["targets"]).all() and (inner.max(axis=1) == info["farthest"]).all()
        none = info["targets"] == 0
        assert (inner[none] == NONE).all() and (info["farthest"][none] == NONE).all() and (info["where"][none] == 0).all() and (info["faces"][none] == 0).all()
        assert (inner[~none] <= 3 * 31 ** 2).all()
    absent, absent_air = truth_for(case, the_call(case, "17-absent")), truth_for(case, the_call(case, "17-absent-air"))
    assert (absent[1]["targets"] == 0).all() and (absent[0] == NONE).all()
    assert (absent_air[1]["targets"] == SEVENTEEN.voxels).all() and (absent_air[0][:, :SEVENTEEN.voxels] == 0).all() and (absent_air[1]["faces"] == 63).all()
    # the complement's targets are the other cells; a pass value that occurs makes cells air: never more targets than without
    solid, air = truth_for(case, the_call(case, "17-solid"))[1], truth_for(case, the_call(case, "17-air"))[1]
    assert (solid["targets"] + air["targets"] == SEVENTEEN.voxels).all()
    passing, matching = truth_for(case, the_call(case, "17-pass"))[1], truth_for(case, the_call(case, "17-match"))[1]
    assert (passing["targets"] + matching["targets"] == solid["targets"]).all() and (matching["targets"] > 0).any()


def one(c, lo, size, **kw):
    """One box by the harness, held against the truth: (field [z, y, x], the record)."""
    boxes = np.array([lo], dtype=np.int32)
    got = c.host.distance(boxes, size, **kw)
    expected = distance_truth(c, boxes, size, kw.get("pass_value", 0), kw.get("match_value", 0), kw.get("flags", 0))
    assert differing(got, expected) is None, differing(got, expected)
    return got[0][0, :size[0] * size[1] * size[2]].reshape(size[2], size[1], size[0]), got[1][0]


def test_the_named_boxes(case):
    """The boxes around the world, by the truth (which the harness equals, above)."""
    names = {name: named_at(case, SEVENTEEN, name) for name in case.names}
    fields, info = truth_for(case, the_call(case, "17-solid"))
    for name in ("outside", "wrapping"):
        assert tuple(info[names[name]]) == (0, NONE, 0, 0) and (fields[names[name]] == NONE).all(), name
    for face in range(6):  # half of the box lies outside the world: no target there
        assert not info[names[f"world_face_{face}"]]["faces"] >> face & 1, face
    if case.name == "tower":
        assert info[names["lod_seam"]]["targets"] > 0 and info[names["lod_leaf"]]["targets"] > 0


def test_the_named_blocks(rubble):
    """Rock all through; the world's last cell in the corner of a box of nothing; single blocks in the hollow of `rubble`."""
    c = rubble
    f, i = one(c, SOLID_ROCK, (32, 32, 32))
    assert tuple(i) == (32768, 0, 0, 63) and (f == 0).all()
    f, i = one(c, SOLID_ROCK, (32, 32, 32), flags=TO_AIR)
    assert tuple(i) == (0, NONE, 0, 0) and (f == NONE).all()
    # the world ends at 128: of a box at 127 only cell 0 lies inside it, the corner of the chunk of rock -- a single block in a 32^3 box of air
    f, i = one(c, (127, 127, 127), (32, 32, 32))
    assert tuple(i) == (1, 3 * 31 ** 2, 31 | 31 << 8 | 31 << 16, 1 | 4 | 16) and f[0, 0, 0] == 0 and f[31, 31, 31] == 2883 and f[0, 0, 31] == 961
    # the single block at (4, 4, 4) of the chunk: in the corner of its box, only in the last plane, only in the last row
    at = np.array((4, 4, 4)) + RUBBLE_AT
    f, i = one(c, at, (3, 3, 3))
    assert tuple(i) == (1, 12, 2 | 2 << 8 | 2 << 16, 1 | 4 | 16)
    f, i = one(c, at - (0, 0, 2), (3, 3, 3))
    assert tuple(i) == (1, 12, 2 | 2 << 8, 1 | 4 | 32) and f[2, 0, 0] == 0 and f[0, 0, 0] == 4
    f, i = one(c, at - (0, 2, 0), (3, 3, 1))
    assert tuple(i) == (1, 8, 2, 1 | 8 | 16 | 32) and f[0, 2, 0] == 0
    # two blocks, (24, 12, 23) and (20, 10, 25), mirror images through the box's centre: a tie for the farthest cell, and `where` is the first
    # in the field's order
    f, i = one(c, np.array((20, 10, 23)) + RUBBLE_AT, (5, 3, 3))
    assert i["targets"] == 2 and (f == i["farthest"]).sum() >= 2 and unpack(i["where"]) == tuple(int(v) for v in np.argwhere(f == i["farthest"])[0][::-1])
    # depth inside rock: the chunk's wall is two cells thick and the box ends at the chunk's face
    f, i = one(c, (RUBBLE_AT, RUBBLE_AT + 16, RUBBLE_AT + 16), (8, 4, 4), flags=TO_AIR)
    assert list(f[0, 0]) == [4, 1, 0, 0, 0, 0, 0, 0] and i["targets"] == 6 * 16 and i["farthest"] == 4 and i["where"] == 0


def test_outputs_and_strides(case):
    """Fields only, records only, every form of lo, a stride larger than the field (the bytes beyond it keep their sentinel), one box, none."""
    shape = SHAPE["31x3x17"]
    boxes = boxes_for(case, shape)[:40]
    expected = distance_truth(case, boxes, shape)
    for stride in (12, 16, 20, 64):  # packed, padded to 16 and 20 bytes, inside a larger record
        assert differing(case.host.distance(boxes, shape.size, lo_stride=stride), expected) is None, stride
    f, i = case.host.distance(boxes, shape.size, info=False)
    assert i is None and (f == expected[0]).all()
    f, i = case.host.distance(boxes, shape.size, fields=False)
    assert f is None and i.tobytes() == expected[1].tobytes()
    f, i = case.host.distance(boxes, shape.size, field_stride=shape.bytes + 32)
    assert (f[:, :shape.entries] == expected[0]).all() and (f[:, shape.entries:] == 0x5A5A).all() and i.tobytes() == expected[1].tobytes()
    f, i = case.host.distance(boxes[7:8], shape.size)
    assert (f == expected[0][7:8]).all() and i.tobytes() == expected[1][7:8].tobytes()
    f, i = case.host.distance(boxes[:0], shape.size)
    assert f.size == 0 and i.size == 0


def test_a_second_opinion_on_the_field():
    """scipy.ndimage.distance_transform_edt over the same cells, squared and rounded, on the seeded boxes."""
    ndimage = pytest.importorskip("scipy.ndimage")
    c = make_distance_case("rubble", "esvo")
    for flags in (0, TO_AIR):
        fields, info = truth_for(c, the_call(c, "17-air" if flags else "17-solid"))
        target = targets_of(regions_of(c, c.boxes[pick_for(c, SEVENTEEN)], SEVENTEEN.size), flags=flags)
        f = cells(fields, SEVENTEEN)
        for k in range(len(f)):
            if not target[k].any():
                assert (f[k] == NONE).all()
                continue
            edt = ndimage.distance_transform_edt(~target[k])
            assert (np.rint(edt ** 2).astype(np.int64) == f[k]).all(), (flags, k)


def test_the_margin_rule():
    """A value v <= g^2, g the cell's distance in cells to the outside of the box, is the value a larger box gives: seeded 16^3 sections inside
    32^3 boxes, at every offset of a seeded set."""
    rng = np.random.default_rng(131)
    checked = 0
    for name, fmt in (("rubble", "esvo"), ("glasshouse", "esvo"), ("tower", "csvo")):
        c = make_distance_case(name, fmt)
        boxes = c.boxes[rng.integers(0, SEEDED, 12)].astype(np.int64) - 8
        for flags in (0, TO_AIR):
            large = cells(distance_truth(c, boxes, (32, 32, 32), flags=flags)[0], SHAPE["32"])
            off = rng.integers(0, 17, (len(boxes), 3))
            small = cells(distance_truth(c, boxes + off, (16, 16, 16), flags=flags)[0], Shape("16", (16, 16, 16)))
            r = np.arange(16)
            g1 = np.minimum(r + 1, 16 - r)
            g = np.minimum(np.minimum(g1[:, None, None], g1[None, :, None]), g1[None, None, :])
            for k, (ox, oy, oz) in enumerate(off):
                inside = large[k, oz:oz + 16, oy:oy + 16, ox:ox + 16]
                sure = small[k].astype(np.int64) <= g ** 2
                assert (small[k][sure] == inside[sure]).all(), (name, flags, k)
                assert (small[k] >= inside).all()  # (a larger box can only bring a target nearer)
                checked += int(sure.sum())
    assert checked > 10000


@pytest.mark.parametrize("name", ["rubble", "burrow", "tower"])
def test_the_sanitized_program(exe, name):
    """The same program under -fsanitize=address,undefined -fno-sanitize-recover=all, run directly: every call of `rubble`, `burrow` and
    `tower`, both formats, on six seeded boxes and every named one -- negative, overhanging and wrapping coordinates among them --,
    and its own check of the bit function and the pass. A finding ends the program with a non-zero status; its bytes are the plain program's."""
    san = harness(sanitize=True)
    r = subprocess.run([str(san), "lines"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout
    for fmt in ("esvo", "csvo"):
        c = make_distance_case(name, fmt)
        plain, checked = HostDistance(exe, c), HostDistance(san, c)
        try:
            for call in calls_for(c):
                n = len(pick_for(c, call[1]))
                named = len(c.boxes) - SEEDED
                pick = np.concatenate([np.arange(6), np.arange(n - named, n)])
                assert differing(plain.call(c, call, pick), checked.call(c, call, pick)) is None, (fmt, call[0])
        finally:
            plain.close()
            checked.close()


def test_the_rules_refuse_what_the_abi_lists(exe):
    """vx_distance.hpp's argument rules on their own: each bad value named by its field, what is allowed allowed."""
    out = subprocess.run([str(exe), "rules"], stdout=subprocess.PIPE, text=True, check=True).stdout
    said = dict(ln.split(": ", 1) for ln in out.splitlines())
    for ok in ("packed", "stride 64", "fields only", "info only", "info only, any stride", "count 0", "count 2^20", "largest box", "smallest box", "flags 1", "any pass_value",
               "any match_value", "match_value to air", "any padding", "field_stride 8192", "field_stride 8208", "field_stride 16384", "field bytes 2^24",
               "records only beyond 2^24", "fields beside lo", "info beside lo", "side by side"):
        assert said[ok] == "ok", (ok, said[ok])
    assert said["too many"] == "count exceeds 1048576 (2^20)"
    assert said["null shape"] == "null shape" and said["null lo"] == "null lo" and said["no output"] == "fields and info are both null"
    for stride in (0, 4, 8, 13, 14):
        assert said[f"lo_stride {stride}"].startswith("lo_stride"), stride
    for off in (1, 2, 3):
        assert said[f"lo + {off}"].startswith("lo must be aligned"), off
    for a in range(3):
        for side in (0, 33, 0xFFFFFFFF):
            assert said[f"size[{a}] {side}"] == "size: every component must be 1..32", (a, side)
    for flags in (2, 3, 0x80000000):
        assert said[f"flags {flags}"].startswith("flags"), flags
    assert said["match_value with pass_value"].startswith("pass_value")
    for stride in (8193, 8200, 8176, 4096, 16):  # (4,096: the voxel count, half of what the entries need)
        assert said[f"field_stride {stride}"].startswith("field_stride"), stride
    assert said["field bytes 2^24 + 8192"].startswith("count * field_stride")
    for what, word in (("fields on lo", "fields overlaps lo"), ("info on lo", "info overlaps lo"), ("fields on info", "fields overlaps info"),
                       ("strided fields between", "fields overlaps info")):
        assert said[what] == word, what
    assert hip.DISTANCE_INFO_DTYPE.itemsize == 16 and len(SHAPES) == 12 and SHAPE["32"].voxels == 32768 and ABSENT and match_id and derive
