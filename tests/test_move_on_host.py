"""vx_move_boxes' answer without a GPU: voxel-rs_amd/csrc/blocks/vx_move.hpp compiled for the host by the stand-alone harness
tests/cpp/move_on_host.cpp -- box by box, pass by pass and brick by brick as the kernel runs it -- against the numpy records of
tests/move_cases.py over the dense arrays the worlds were built from: all three worlds, both formats, every box in every form, order, skin
and only_value, byte for byte; a property of the truth that does not depend on the rule's arithmetic; the argument rules; and the same
program built with AddressSanitizer and UndefinedBehaviorSanitizer (with the float-to-integer conversion check) on the named boxes and every
tenth seeded one of `tower`. test_move.py holds the GPU's records against the harness's."""
import subprocess

import numpy as np
import pytest

from blocks_cases import dense_region
from boxes_cases import cover_of
from move_cases import (INVALID, SCAN_CASES, SEEDED, SKIN, XYZ, YXZ, HostMoves, absent_id, calls_for, differing, harness, make_moves, make_scan_case, moves_truth,
                        overlaps_at)
from voxel_rs_amd import hip


@pytest.fixture(scope="module")
def exe():
    return harness()


@pytest.fixture(scope="module", params=SCAN_CASES, ids=[f"{n}-{f}" for n, f in SCAN_CASES])
def case(request, exe):
    c = make_scan_case(*request.param)
    c.host = HostMoves(exe, c)
    c.moves = make_moves(c)
    c.expected = moves_truth(c, c.moves)
    yield c
    c.host.close()


def axis_bits(contacts):
    """[N, 3]: the two contact bits of each axis"""
    return np.stack([(contacts >> (2 * a)) & 3 for a in range(3)], axis=1)


def test_the_moves_hold_what_the_tests_need(case):
    """By the dense arrays alone. A set that misses a threshold is changed (its seed, the way of drawing); the threshold never is."""
    mv, exp = case.moves, case.expected
    seeded, motion = exp[mv.seeded], mv.motion[mv.seeded]
    assert len(seeded) == SEEDED and (seeded["contacts"] != INVALID).all()
    contact = float((seeded["contacts"] != 0).mean())
    sides = [int(((seeded["contacts"] >> s) & 1).sum()) for s in range(6)]
    two_axes = int(((axis_bits(seeded["contacts"]) != 0).sum(axis=1) >= 2).sum())
    other = moves_truth(case, mv, order=XYZ)[mv.seeded]
    by_order = int((seeded.view(np.uint32).reshape(-1, 12) != other.view(np.uint32).reshape(-1, 12)).any(axis=1).sum())
    stuck = overlaps_at(case, mv.picked(mv.seeded), mv.boxes.origin[mv.seeded]) > 0
    stuck_moving = int((stuck & (seeded["moved"] != 0).any(axis=1)).sum())
    partly = int(((np.abs(seeded["moved"]) > 0) & (np.abs(seeded["moved"]) < np.abs(motion))).any(axis=1).sum())
    stopped = int(((seeded["moved"] == 0) & (motion != 0)).any(axis=1).sum())
    print(f"\n{case.name}-{case.fmt}: {contact:.1%} with a contact, by side {sides}, {two_axes} on two axes or more, {by_order} differ by order, "
          f"{stuck_moving} start inside a block and move, {partly} stopped part of the way, {stopped} not moving at all")
    assert contact >= 0.25 and min(sides) >= 50 and two_axes >= 20 and by_order >= 20 and stuck_moving >= 20 and partly >= 20 and stopped >= 20
    named = {name: exp[i] for name, i in mv.names.items()}
    skin, zero = np.float32(SKIN), np.float32(0)
    # resting exactly on a block's top, moving down: gap 0, a contact below, -0.0 moved
    r = named["resting_down"]
    assert r["contacts"] == 1 << 2 and r["value"][1] != 0 and r["moved"][1] == 0 and np.signbit(r["moved"][1]) and r["origin"][1] == mv.boxes.origin[mv.names["resting_down"]][1]
    assert named["hover_down"]["moved"][1] == 0 and named["hover_down"]["contacts"] == 1 << 2
    assert named["hover_quarter"]["moved"][1] == -(np.float32(0.25) - skin) and named["hover_quarter"]["contacts"] == 1 << 2
    assert named["sunk_up"]["moved"][1] == np.float32(0.5) and named["sunk_up"]["contacts"] == 0
    assert named["sunk_down"]["moved"][1] < 0  # the block it stands in does not hold it
    assert named["minus_zero"].tobytes() == named["resting_down"].tobytes()
    for name in ("minus_zero_all", "still"):
        i = mv.names[name]
        assert named[name]["contacts"] == 0 and named[name]["moved"].tobytes() == bytes(12) and named[name]["origin"].tobytes() == mv.boxes.origin[i].tobytes()
    # past a block's edge: y first, the box comes down beside the block and is stopped by its side; x first, it lands on its top
    x_first = moves_truth(case, mv, order=XYZ)[mv.names["diagonal"]]
    assert named["diagonal"]["contacts"] == 1 << 0 and x_first["contacts"] == 1 << 2 and x_first.tobytes() != named["diagonal"].tobytes()
    assert named["diagonal"]["moved"][1] == np.float32(-0.5) and x_first["moved"][0] == np.float32(-0.5)
    assert named["travel_64"]["contacts"] != INVALID and named["travel_above_64"]["contacts"] == INVALID and named["travel_above_64_z"]["contacts"] == INVALID
    for name in ("far_x", "far_negative", "far_huge", "far_all", "into_the_world", "out_of_the_world", "in_from_the_top", "widest", "widest_diagonal"):
        assert named[name]["contacts"] != INVALID, name
    assert named["far_x"]["moved"][0] == 1 and named["far_negative"]["moved"][1] == 1 and named["far_huge"]["moved"][2] == -1
    assert named["out_of_the_top"]["moved"][1] == 9 and named["below_the_world"]["moved"][1] == -3 and named["below_the_world"]["contacts"] == 0
    for name, r in named.items():
        if name.startswith("motion_"):
            assert r["contacts"] == INVALID and r.tobytes()[:24] == bytes(24) and r.tobytes()[28:] == bytes(20), name
    assert len(mv.no_box) >= 45
    for i in mv.no_box:
        assert exp[i]["contacts"] == INVALID and exp[i].tobytes()[:24] == bytes(24), i
    # a skin larger than the gap: no move, and a contact; a skin of 0: the whole gap
    half, none = moves_truth(case, mv, skin=0.5), moves_truth(case, mv, skin=0.0)
    assert half[mv.names["hover_quarter"]]["moved"][1] == 0 and half[mv.names["hover_quarter"]]["contacts"] == 1 << 2
    assert none[mv.names["hover_down"]]["moved"][1] == -skin and named["hover_down"]["moved"][1] == zero
    # an id that occurs nowhere: the box falls through everything
    absent = moves_truth(case, mv, only_value=absent_id(case))
    valid = absent["contacts"] != INVALID
    assert (absent["contacts"][valid] == 0).all() and named["fall_through"]["contacts"] == 1 << 2 and absent[mv.names["fall_through"]]["moved"][1] == -6
    if case.name == "tower":
        assert named["lod_seam"]["contacts"] != INVALID and named["lod_leaf_16"]["contacts"] & (1 << 2)


def test_every_call_against_the_dense_array(case):
    """Every form of the boxes and of the motion, the three orders, three skins, two scales and only_value."""
    for name, mv, how in calls_for(case, case.moves):
        exp = moves_truth(case, mv, **how)
        got = case.host.records(mv, **how)
        assert differing(got, exp) is None, f"{name}: {differing(got, exp)}"
        if name in ("entities", "motion_stride16", "motion_velocity"):
            assert exp.tobytes() == case.expected.tobytes(), name
        if name == "motion_one":
            assert exp.tobytes() != case.expected.tobytes()


def test_one_box_and_no_box(case):
    mv = case.moves
    for i in (7, int(mv.names["diagonal"]), int(mv.no_box[0])):
        assert case.host.records(mv.picked(np.array([i]))).tobytes() == case.expected[i:i + 1].tobytes(), i
    none = mv.picked(np.array([], dtype=np.int64))
    assert len(case.host.records(none)) == 0


def test_a_move_never_puts_a_box_into_a_block(case):
    """What the truth says of itself, by the cover and the dense array alone. With a skin of 2^-10 and every coordinate below 4096 in
    magnitude a box's three roundings after a pass (origin + m, + offset, + extents) stay under 1.5 * 2^-12 together, less than the skin: so
    the box at its new origin overlaps no block it did not overlap where it started. And a box with no contact has moved by d exactly."""
    mv, exp = case.moves, case.expected
    b = mv.boxes
    checked = 0
    for i in mv.seeded:
        before, after = cover_of(case, b.origin[i], b.offset[i], b.extents[i]), cover_of(case, exp["origin"][i], b.offset[i], b.extents[i])
        corners = np.abs(np.concatenate([b.origin[i] + b.offset[i], b.origin[i] + b.offset[i] + b.extents[i], b.origin[i], exp["origin"][i],
                                         exp["origin"][i] + b.offset[i] + b.extents[i], exp["origin"][i] + b.offset[i]]))
        if exp["contacts"][i] == 0:
            assert (exp["moved"][i] == mv.motion[i]).all(), i  # (scale 1: d is the motion)
        if corners.max() >= 4096:
            continue
        checked += 1
        (f0, l0), (f1, l1) = before, after
        if any(lo > hi for lo, hi in zip(f1, l1)):
            continue
        region = dense_region(case.info, case.truth, f1, [hi - lo + 1 for lo, hi in zip(f1, l1)])
        for z, y, x in np.argwhere(region != 0):
            p = (f1[0] + int(x), f1[1] + int(y), f1[2] + int(z))
            assert all(f0[k] <= p[k] <= l0[k] for k in range(3)), f"box {i} ends in the block at {p}, which it did not start in: {exp[i]}"
    assert checked >= (1900 if case.size <= 4096 else 0)


def test_the_sanitized_program_on_tower(exe):
    """The same program under -fsanitize=address,undefined -fsanitize=float-cast-overflow -fno-sanitize-recover=all, run directly: the named
    boxes -- 3e9, -3e9, 1e30, the travel of 64 and the largest slab among them --, the records that are no box and every tenth seeded box of
    `tower`, both formats, every call. A finding ends the program with a non-zero status; its records are the plain program's."""
    san = harness(sanitize=True)
    for fmt in ("esvo", "csvo"):
        c = make_scan_case("tower", fmt)
        plain, checked = HostMoves(exe, c), HostMoves(san, c)
        try:
            mv = make_moves(c)
            keep = np.concatenate([mv.seeded[::10], mv.named, mv.no_box])
            part = mv.picked(keep)
            for name, m, how in calls_for(c, part):
                assert checked.records(m, **how).tobytes() == plain.records(m, **how).tobytes(), (fmt, name)
        finally:
            plain.close()
            checked.close()


def test_the_rules_refuse_what_the_abi_lists(exe):
    """vx_move.hpp's argument rules on their own: each bad value named by its field, what is allowed allowed."""
    out = subprocess.run([str(exe), "rules"], stdout=subprocess.PIPE, text=True, check=True).stdout
    said = dict(ln.split(": ", 1) for ln in out.splitlines())
    for ok in ("packed", "one motion", "entities", "count 0", "motion_stride 12", "motion_stride 16", "motion_stride 64", "scale 0", "scale -1", "scale 1e30",
               "skin 0", "skin -0", "skin 1", "skin 0.5"):
        assert said[ok] == "ok", (ok, said[ok])
    assert said["count 0, null shape"] == "null shape" and said["null shape"] == "null shape" and said["null motion"] == "null motion"
    assert said["null boxes"] == "null boxes" and said["null out"] == "null out" and said["too many"].startswith("count exceeds 16777216")
    assert said["origin_stride 8"].startswith("origin_stride")
    for stride in (4, 8, 13, 18):
        assert said[f"motion_stride {stride}"].startswith("motion_stride"), stride
    for off in (1, 2, 3):
        assert said[f"motion + {off}"].startswith("motion must be aligned"), off
    for bad in ("scale inf", "scale -inf", "scale nan"):
        assert said[bad].startswith("scale"), bad
    for bad in ("skin -1e-6", "skin 1.0000001", "skin inf", "skin nan"):
        assert said[bad].startswith("skin"), bad
    permutations = {a | b << 2 | c << 4 for a in range(3) for b in range(3) for c in range(3) if len({a, b, c}) == 3}
    assert {YXZ, XYZ, hip.VX_MOVE_ORDER_ZYX} <= permutations and len(permutations) == 6
    for order in range(64):
        assert (said[f"order {order}"] == "ok") == (order in permutations), order
    for order in (0x21 | 0x40, 0x21 | 0x80000000):
        assert said[f"order {order}"].startswith("order"), order
    assert said["flags 1"].startswith("flags") and said[f"flags {0x80000000}"].startswith("flags")
    assert hip.MOVE_HIT_DTYPE.itemsize == 48
