"""vx_label_boxes' answer without a GPU: voxel-rs_amd/csrc/blocks/vx_label.hpp compiled for the host by the stand-alone harness
tests/cpp/label_on_host.cpp -- box by box, the bricks, rows, steps and floods the kernel's workgroup walks -- against the numpy fields, piece
records and records of tests/label_cases.py, which come from breadth-first floods over the dense arrays the worlds were built from: five
worlds, both formats, every shape, anchor_faces, piece limit, step budget, pass value and stride, byte for byte and record for record; the
named boxes for what each was made to catch; and the same program built with AddressSanitizer and UndefinedBehaviorSanitizer.
test_label.py holds the GPU's bytes against the harness's."""
import subprocess

import numpy as np
import pytest

from label_cases import (AIR, ALL_FACES, CUT, HELD, LABEL_CASES, MAX_PIECES, MAX_STEPS, MORE, RUBBLE_AT, RUBBLE_NAMED, SEEDED, SEVENTEEN, SHAPE, SHAPES, SOLID_ROCK,
                         HostLabel, anchor_cells, boxes_for, calls_for, cells, derive, differing, full_for, harness, label_truth, make_label_case, regions_of,
                         the_call, truth_for)
from voxel_rs_amd import hip


@pytest.fixture(scope="module")
def exe():
    return harness()


@pytest.fixture(scope="module", params=LABEL_CASES, ids=[f"{n}-{f}" for n, f in LABEL_CASES])
def case(request, exe):
    c = make_label_case(*request.param)
    c.host = HostLabel(exe, c)
    yield c
    c.host.close()


@pytest.fixture(scope="module", params=["esvo", "csvo"])
def rubble(request, exe):
    c = make_label_case("rubble", request.param)
    c.host = HostLabel(exe, c)
    yield c
    c.host.close()


def test_the_boxes_hold_what_the_tests_need(case):
    """By the truth alone, among the seeded boxes at 17^3 with every face anchored. A set that misses a condition gets another seed; the
    condition is never loosened. (The conditions are `rubble`'s: the other worlds' figures are printed.)"""
    full = full_for(case, SEVENTEEN, ALL_FACES, 0)
    whole = derive(full, SEVENTEEN, MAX_PIECES, MAX_STEPS)[2][:SEEDED]
    four = derive(full, SEVENTEEN, 4, MAX_STEPS)[2][:SEEDED]
    short = derive(full, SEVENTEEN, MAX_PIECES, 24)[2][:SEEDED]
    figures = (int((whole["pieces"] >= 1).sum()), int((whole["pieces"] >= 2).sum()), int((four["more"] > 0).sum()), int((short["flags"] & CUT != 0).sum()))
    print(f"\n{case.name}-{case.fmt}: {figures[0]} boxes with a piece, {figures[1]} with two or more, {figures[2]} with more > 0 at max_pieces 4, {figures[3]} cut at max_steps 24")
    assert not (whole["flags"] & CUT).any() and len(case.boxes) <= 200 + 16
    if case.name == "rubble":
        assert figures[0] >= SEEDED // 4 and figures[1] >= 20 and figures[2] >= 10 and figures[3] >= 5


def test_every_call_against_the_dense_array(case):
    """Every shape under every anchor_faces, the piece limits, step budgets, pass values and strides in turn; 17^3 under every budget."""
    for call in calls_for(case):
        name, shape, faces, most, steps, pass_value, stride = call
        expected = truth_for(case, call)
        got = case.host.call(case, call)
        assert differing(got, expected) is None, f"{name} (pieces {most}, steps {steps}, pass {pass_value}, stride {stride}): {differing(got, expected)}"
        fields, pieces, info = expected
        assert (fields[:, shape.voxels:] == AIR).all()
        assert (info["solid"] == info["held"] + info["loose"] + info["more"]).all() and (info["pieces"] <= most).all() and (info["steps"] <= steps).all()
        assert (info["loose"] == pieces["cells"].sum(axis=1)).all() and ((pieces["cells"] > 0).sum(axis=1) == info["pieces"]).all()
        f = cells(fields, shape)
        assert ((f == HELD).sum(axis=(1, 2, 3)) == info["held"]).all() and ((f == MORE).sum(axis=(1, 2, 3)) == info["more"]).all()
        if faces == 0:
            assert (info["held"] == 0).all()
        if most == 0:
            assert (info["loose"] == 0).all() and pieces.shape[1] == 0
    # a pass value that occurs makes cells air: never more solid cells than without
    plain, passing = truth_for(case, the_call(case, "17-250-4096"))[2], truth_for(case, the_call(case, "17-250-4096-pass"))[2]
    assert (passing["solid"] <= plain["solid"]).all() and (passing["solid"] < plain["solid"]).any()


def test_the_labels_come_in_the_fields_order(case):
    """Label k's first cell in the field's order lies before label k + 1's, and is the piece record's `where`."""
    call = the_call(case, "32-0x0") if case.name != "burrow" else the_call(case, "17-250-4096")
    shape = call[1]
    got = case.host.label(boxes_for(case, shape), shape.size, call[2], MAX_PIECES, MAX_STEPS, 0)
    fields, pieces, info = got
    assert differing(got, label_truth(case, boxes_for(case, shape), shape, call[2])) is None
    seen = 0
    for k in np.flatnonzero(info["pieces"] >= 2)[:40]:
        first = [int(np.flatnonzero(fields[k, :shape.voxels] == label)[0]) for label in range(1, int(info["pieces"][k]) + 1)]
        assert first == sorted(first)
        where = pieces["where"][k, :len(first)] & 0xFFFFFF
        assert [int(w & 0xFF) + shape.size[0] * (int(w >> 8 & 0xFF) + shape.size[1] * int(w >> 16)) for w in where] == first
        seen += 1
    assert seen or case.name in ("burrow", "glasshouse")


def one(c, lo, size, faces=ALL_FACES, most=MAX_PIECES, steps=MAX_STEPS, pass_value=0):
    """One box by the harness, held against the truth: (field [z, y, x], the pieces that exist, the record)."""
    boxes = np.array([lo], dtype=np.int32)
    got = c.host.label(boxes, size, faces, most, steps, pass_value, pieces=True if most else None)
    got = (got[0], np.zeros((1, 0), dtype=hip.LABEL_PIECE_DTYPE) if got[1] is None else got[1], got[2])
    expected = label_truth(c, boxes, size, faces, most, steps, pass_value)
    assert differing(got, expected) is None, differing(got, expected)
    fields, pieces, info = got
    return fields[0, :size[0] * size[1] * size[2]].reshape(size[2], size[1], size[0]), pieces[0][pieces[0]["cells"] > 0], info[0]


def named(c, name, **over):
    at, size, faces, pass_value = RUBBLE_NAMED[name]
    return one(c, np.array(at) + RUBBLE_AT, size, over.pop("faces", faces), pass_value=over.pop("pass_value", pass_value), **over)


def unpack(word):
    return int(word & 0xFF), int(word >> 8 & 0xFF), int(word >> 16 & 0xFF)


def test_the_named_pieces(rubble):
    """What each piece of `rubble` was made to catch, in a box around it (which the harness answers as the truth does)."""
    c = rubble
    f, p, i = named(c, "single")
    assert tuple(i) == (1, 0, 1, 1, 0, 0, 0, 0) and tuple(p[0]) == (1, 2 | 2 << 8 | 2 << 16, 2 | 2 << 8 | 2 << 16, 2 | 2 << 8 | 2 << 16) and f[2, 2, 2] == 1
    f, p, i = named(c, "cube")
    assert tuple(i) == (8, 0, 1, 8, 0, 3, 0, 0) and unpack(p[0]["lo"]) == (1, 1, 1) and unpack(p[0]["hi"]) == (2, 2, 2)
    for pair in ("edge_pair", "corner_pair"):  # contact along an edge or at a corner does not connect
        f, p, i = named(c, pair)
        assert (i["solid"], i["pieces"], i["loose"], i["steps"]) == (2, 2, 2, 0) and list(p["cells"]) == [1, 1], pair
    f, p, i = named(c, "ring")
    assert (i["solid"], i["pieces"], i["loose"], i["steps"]) == (16, 1, 16, 8) and unpack(p[0]["lo"]) == (1, 1, 1) and unpack(p[0]["hi"]) == (5, 1, 5)
    f, p, i = named(c, "checkerboard")
    assert (i["solid"], i["pieces"], i["loose"], i["more"], i["steps"]) == (108, 108, 108, 0, 0) and (p["cells"] == 1).all()
    assert sorted(np.unique(f)) == list(range(109))
    f, p, i = named(c, "checkerboard", most=4)
    assert (i["pieces"], i["loose"], i["more"]) == (4, 4, 104) and (f == MORE).sum() == 104
    f, p, i = named(c, "checkerboard", most=0)
    assert (i["pieces"], i["loose"], i["more"]) == (0, 0, 108)  # the cheap "does anything hang loose, and how much"
    # the blob hangs from the ceiling by a cell of id 9: held -- and loose once 9 counts as air
    f, p, i = named(c, "blob_held")
    assert i["pieces"] == 0 and i["more"] == 0 and f[8, 12, 8] == HELD and f[8, 14, 8] == HELD
    f, p, i = named(c, "blob_loose")
    assert (i["pieces"], i["loose"]) == (1, 27) and f[8, 12, 8] == 1 and f[8, 14, 8] == AIR and unpack(p[0]["lo"]) == (7, 11, 7) and unpack(p[0]["hi"]) == (9, 13, 9)
    # the wire: 269 cells, 268 steps from its first cell; a budget of 267 cuts it and labels nothing
    f, p, i = named(c, "wire")
    assert (i["solid"], i["pieces"], i["loose"], i["steps"], i["flags"]) == (269, 1, 269, 268, 0)
    f, p, i = named(c, "wire", steps=267)
    assert (i["pieces"], i["loose"], i["more"], i["steps"], i["flags"]) == (0, 0, 269, 267, CUT) and (f == MORE).sum() == 269 and len(p) == 0
    # the U: two pieces in the box that cuts its base off, one in the larger box
    f, p, i = named(c, "u_cut")
    assert (i["pieces"], i["loose"]) == (2, 10) and list(p["cells"]) == [5, 5] and (p["where"] >> 24 == 4).all()  # (both touch the box's floor)
    f, p, i = named(c, "u_whole")
    assert (i["pieces"], i["loose"], i["steps"]) == (1, 15, 9)  # (from the base's corner to the far prong's tip)
    f, p, i = named(c, "u_cut", faces=0x04)  # the floor anchored: the prongs stand on it
    assert (i["held"], i["pieces"]) == (10, 0)
    # the order is z, then y, then x: the block with the smaller z is piece 1 though the other has the smaller x and the smaller y
    f, p, i = named(c, "order")
    assert i["pieces"] == 2 and unpack(p[0]["where"]) == (6, 4, 1) and unpack(p[1]["where"]) == (2, 2, 3)
    f, p, i = named(c, "straddle")
    assert (i["pieces"], i["loose"], i["steps"]) == (1, 8, 3) and unpack(p[0]["lo"]) == (3, 3, 3) and unpack(p[0]["hi"]) == (4, 4, 4)


def test_the_budget_is_spent_by_depth(rubble):
    """used + depth == max_steps exactly: complete. One step fewer: cut. The coil (no anchor in its box, one piece of depth 38); the chunk of
    solid rock with no face anchored (one piece of 32^3 cells whose depth, 93, is far below its size: the budget counts steps, not cells);
    and a held flood and a piece that share a budget."""
    c = rubble
    f, p, i = named(c, "coil", steps=38)
    assert (i["held"], i["pieces"], i["loose"], i["steps"], i["flags"]) == (0, 1, 39, 38, 0)
    f, p, i = named(c, "coil", steps=37)
    assert (i["held"], i["pieces"], i["loose"], i["more"], i["steps"], i["flags"]) == (0, 0, 0, 39, 37, CUT)
    f, p, i = one(c, SOLID_ROCK, (32, 32, 32), faces=0, steps=93)
    assert tuple(i) == (32768, 0, 1, 32768, 0, 93, 63, 0) and (f == 1).all() and tuple(p[0]) == (32768, 0, 31 | 31 << 8 | 31 << 16, 63 << 24)
    f, p, i = one(c, SOLID_ROCK, (32, 32, 32), faces=0, steps=92)
    assert tuple(i) == (32768, 0, 0, 0, 32768, 92, 63, CUT) and (f == MORE).all()
    f, p, i = one(c, SOLID_ROCK, (32, 32, 32), faces=0x01, steps=31)  # held from the -x face: 31 steps to the far side
    assert tuple(i) == (32768, 32768, 0, 0, 0, 31, 63, 0) and (f == HELD).all()
    f, p, i = one(c, SOLID_ROCK, (32, 32, 32), faces=0x01, steps=30)  # cut: the 31 layers the budget covered stay held
    assert tuple(i) == (32768, 31 * 1024, 0, 0, 1024, 30, 63, CUT) and (f[:, :, :31] == HELD).all() and (f[:, :, 31] == MORE).all()
    # the coil's box grown to the chunk's ceiling: the rock is held in 1 step (two layers of it), then the coil needs its 38
    lo, size = np.array((17, 23, 17)) + RUBBLE_AT, (11, 9, 9)
    f, p, i = one(c, lo, size, steps=39)
    assert (i["held"], i["pieces"], i["loose"], i["steps"], i["flags"]) == (2 * 11 * 9, 1, 39, 39, 0)
    f, p, i = one(c, lo, size, steps=38)
    assert (i["held"], i["pieces"], i["loose"], i["more"], i["steps"], i["flags"]) == (2 * 11 * 9, 0, 0, 39, 38, CUT)
    f, p, i = one(c, lo, size, steps=0)  # no step at all: the anchors themselves -- the top layer, the rim of the one below -- are held
    assert (i["held"], i["more"], i["steps"], i["flags"]) == (11 * 9 + 36, 11 * 9 - 36 + 39, 0, CUT)


def test_the_named_boxes(case):
    """The boxes around the world, by the truth (which the harness equals, above)."""
    names = case.names
    fields, pieces, info = truth_for(case, the_call(case, "17-250-4096"))
    for name in ("outside", "wrapping"):
        assert tuple(info[names[name]]) == (0,) * 8 and (fields[names[name]] == AIR).all(), name
    f = cells(fields, SEVENTEEN)
    for face in range(6):  # half of the box lies outside the world: air there
        k = names[f"world_face_{face}"]
        outside = anchor_cells((17, 17, 17), 1 << face)
        assert (f[k][outside] == AIR).all() and not info[k]["faces"] >> face & 1, face
    if case.name == "tower":
        assert info[names["lod_seam"]]["solid"] > 0 and info[names["lod_leaf"]]["solid"] > 0
    if case.name == "rubble":
        assert tuple(info[names["in_rock"]]) == (17 ** 3, 17 ** 3, 0, 0, 0, 8, 63, 0)


def test_outputs_and_strides(case):
    """Fields only, pieces only, records only, a stride larger than the box (the bytes beyond the rounded voxel count keep their sentinel),
    one box, none."""
    shape, most = SHAPE["31x3x17"], 4
    boxes = boxes_for(case, shape)
    exp_fields, exp_pieces, exp_info = label_truth(case, boxes, shape, max_pieces=most)
    for stride in (12, 16, 64):  # packed, at stride 16, inside a larger record
        f, p, i = case.host.label(boxes, shape.size, max_pieces=most, lo_stride=stride)
        assert differing((f, p, i), (exp_fields, exp_pieces, exp_info)) is None, stride
    f, p, i = case.host.label(boxes, shape.size, max_pieces=most, fields=True, pieces=False, info=False)
    assert p is None and i is None and (f == exp_fields).all()
    f, p, i = case.host.label(boxes, shape.size, max_pieces=most, fields=False, pieces=True, info=False)
    assert f is None and i is None and p.tobytes() == exp_pieces.tobytes()
    f, p, i = case.host.label(boxes, shape.size, max_pieces=most, fields=False, pieces=False, info=True)
    assert f is None and p is None and i.tobytes() == exp_info.tobytes()
    f, p, i = case.host.label(boxes, shape.size, max_pieces=most, field_stride=shape.padded + 32)
    assert (f[:, :shape.padded] == exp_fields).all() and (f[:, shape.padded:] == 0x5a).all() and p.tobytes() == exp_pieces.tobytes() and i.tobytes() == exp_info.tobytes()
    f, p, i = case.host.label(boxes[7:8], shape.size, max_pieces=most)
    assert (f == exp_fields[7:8]).all() and p.tobytes() == exp_pieces[7:8].tobytes() and i.tobytes() == exp_info[7:8].tobytes()
    f, p, i = case.host.label(boxes[:0], shape.size, max_pieces=most)
    assert f.size == 0 and p.size == 0 and i.size == 0


def test_a_second_opinion_on_the_partition():
    """scipy.ndimage.label on the same solid cells: the components that touch no anchor face are the truth's pieces, cell for cell."""
    ndimage = pytest.importorskip("scipy.ndimage")
    c = make_label_case("rubble", "esvo")
    boxes = boxes_for(c, SEVENTEEN)[:60]
    fields, pieces, info = label_truth(c, boxes, SEVENTEEN)
    solid = regions_of(c, boxes, SEVENTEEN.size) != 0
    on_face = anchor_cells((17, 17, 17), ALL_FACES)
    for k in range(len(boxes)):
        labels, n = ndimage.label(solid[k])  # (6-connected by default)
        held = np.isin(labels, np.unique(labels[on_face & solid[k]])) & solid[k]
        f = cells(fields[k:k + 1], SEVENTEEN)[0]
        assert ((f == HELD) == held).all() and info[k]["pieces"] == n - len(np.unique(labels[on_face & solid[k]]))
        for piece in range(1, int(info[k]["pieces"]) + 1):
            mine = f == piece
            assert len(np.unique(labels[mine])) == 1 and (labels == labels[mine][0]).sum() == mine.sum()


@pytest.mark.parametrize("name", ["rubble", "burrow", "tower"])
def test_the_sanitized_program(exe, name):
    """The same program under -fsanitize=address,undefined -fno-sanitize-recover=all, run directly: every call of `rubble`, `burrow` and
    `tower`, both formats, on the first 20 seeded boxes and every named one -- negative, overhanging and wrapping coordinates among them. A
    finding ends the program with a non-zero status; its bytes are the plain program's."""
    san = harness(sanitize=True)
    for fmt in ("esvo", "csvo"):
        c = make_label_case(name, fmt)
        plain, checked = HostLabel(exe, c), HostLabel(san, c)
        pick = np.concatenate([np.arange(20), np.arange(SEEDED, len(c.boxes))])
        try:
            for call in calls_for(c):
                assert differing(plain.call(c, call, pick), checked.call(c, call, pick)) is None, (fmt, call[0])
        finally:
            plain.close()
            checked.close()


def test_the_rules_refuse_what_the_abi_lists(exe):
    """vx_label.hpp's argument rules on their own: each bad value named by its field, what is allowed allowed."""
    out = subprocess.run([str(exe), "rules"], stdout=subprocess.PIPE, text=True, check=True).stdout
    said = dict(ln.split(": ", 1) for ln in out.splitlines())
    for ok in ("packed", "stride 64", "fields only", "pieces only", "info only", "info only, any stride", "count 0", "count 2^20", "largest box", "smallest box",
               "anchor_faces 0", "anchor_faces 4", "anchor_faces 63", "max_pieces 0", "max_pieces 250", "max_steps 0", "max_steps 4096", "any pass_value", "field_stride 4096",
               "field_stride 4112", "field_stride 8192", "field bytes 2^24", "piece bytes 2^24", "fields beside lo", "info beside lo", "all side by side"):
        assert said[ok] == "ok", (ok, said[ok])
    assert said["too many"] == "count exceeds 1048576 (2^20)"
    assert said["null shape"] == "null shape" and said["null lo"] == "null lo" and said["no output"] == "fields, pieces and info are all null"
    for stride in (0, 4, 8, 13, 14):
        assert said[f"lo_stride {stride}"].startswith("lo_stride"), stride
    for off in (1, 2, 3):
        assert said[f"lo + {off}"].startswith("lo must be aligned"), off
    for a in range(3):
        for side in (0, 33, 0xFFFFFFFF):
            assert said[f"size[{a}] {side}"] == "size: every component must be 1..32", (a, side)
    for faces in (0x40, 0x80000000):
        assert said[f"anchor_faces {faces}"].startswith("anchor_faces"), faces
    assert said["max_pieces 251"].startswith("max_pieces exceeds") and said["max_steps 4097"].startswith("max_steps exceeds")
    assert said["pieces with max_pieces 0"] == "pieces with max_pieces == 0"
    for flags in (1, 0x80000000):
        assert said[f"flags {flags}"].startswith("flags"), flags
    for stride in (4097, 4104, 4080, 16):
        assert said[f"field_stride {stride}"].startswith("field_stride"), stride
    assert said["field bytes 2^24 + 8192"].startswith("count * field_stride") and said["piece bytes 2^24 + 2784"].startswith("count * max_pieces * 16")
    for what, word in (("fields on lo", "fields overlaps lo"), ("pieces on lo", "pieces overlaps lo"), ("info on lo", "info overlaps lo"), ("fields on pieces", "fields overlaps pieces"),
                       ("fields on info", "fields overlaps info"), ("pieces on info", "pieces overlaps info"), ("strided fields between", "fields overlaps pieces")):
        assert said[what] == word, what
    assert hip.LABEL_INFO_DTYPE.itemsize == 32 and hip.LABEL_PIECE_DTYPE.itemsize == 16 and len(SHAPES) == 7 and SHAPE["32"].voxels == 32768
