"""vx_walk_points' answer without a GPU: voxel-rs_amd/csrc/blocks/vx_walk.hpp compiled for the host by the stand-alone harness
tests/cpp/walk_on_host.cpp -- query by query, the bricks, rows, steps and back-trace candidates the kernel's workgroup walks -- against the
numpy fields, records and paths of tests/walk_cases.py over the dense arrays the worlds were built from: five worlds, both formats, every
shape at every step limit, the path capacities, the forms and the flag, byte for byte; the named positions for what each was made to catch;
and the same program built with AddressSanitizer and UndefinedBehaviorSanitizer on `steps`, `burrow` and `tower`. test_walk.py holds the GPU's
bytes against the harness's."""
import subprocess

import numpy as np
import pytest

from flood_cases import BURROW_AT
from walk_cases import (INVALID, MAX_STEPS, NO_POSITION, NO_STAND, NONE, PATH_CAPACITIES, SEEDED, SHAPE, SHAPES, STEP_LIMITS, STEPS_AT, STOP, UNREACHED, WALK_CASES, HostWalk,
                        Shape, answers, calls_for, differing, edge_kinds, full_truth, harness, in_form, make_walk_case, points_truth, positions_for, truth_for)
from scan_cases import start_of
from voxel_rs_amd import hip


@pytest.fixture(scope="module")
def exe():
    return harness()


@pytest.fixture(scope="module", params=WALK_CASES, ids=[f"{n}-{f}" for n, f in WALK_CASES])
def case(request, exe):
    c = make_walk_case(*request.param)
    c.host = HostWalk(exe, c)
    yield c
    c.host.close()


def test_the_positions_hold_what_the_tests_need(case):
    """By the dense arrays alone, at 17 x 12 x 17 and VX_WALK_MAX_STEPS. A set that misses a condition gets another seed; the condition is
    never loosened."""
    shape = SHAPE["17"]
    full = full_truth(case, shape)
    fields, info, _ = answers(full, shape, MAX_STEPS)
    seeded = info[:SEEDED]
    assert (seeded["reached"] != INVALID).all()
    walks, settles = float((seeded["reached"] >= 2).mean()), sum(1 for k in range(SEEDED) if full["start"][k] is not None and full["start"][k][1] != shape.seed_at[1])
    routes = sum(1 for d in full["goal_steps"][:SEEDED] if d)
    kinds = edge_kinds(full, shape)
    print(f"\n{case.name}-{case.fmt}: {walks:.1%} reach 2 cells or more, {settles} seeds fall before they stand, {routes} goals reached, edges by dy {kinds}")
    assert walks >= 0.25 and settles >= 20 and routes >= 20
    if case.name == "steps":
        assert all(kinds.get(dy, 0) >= 1 for dy in (1, -1, -2, -3)), kinds


def test_every_call_against_the_dense_array(case):
    """Every shape at every step limit with the path capacities, the flag and the forms in turn; a pass_value."""
    for call in calls_for(case):
        name, shape, max_steps, cap, flags, pass_value, form = call
        exp = truth_for(case, shape, max_steps, cap, flags, pass_value)
        got = case.host.call(case, call)
        assert differing(got, exp) is None, f"{name} ({form}): {differing(got, exp)}"
        fields, info, paths = exp
        has = info["reached"] != INVALID
        assert (info["farthest"][has] <= max_steps).all() and (fields[~has][:, :shape.voxels] == NO_POSITION).all() and (fields[:, shape.voxels:] == NO_STAND).all()
        assert (info["_pad"] == 0).all()
        routed = has & (info["path_steps"] != NONE)
        assert (info["path_steps"][routed] <= max_steps).all()
        if cap:
            written = (paths != NONE).sum(axis=1)
            assert (written[routed] == np.minimum(info["path_steps"][routed], cap)).all() and (written[~routed] == 0).all()
        if flags & STOP:
            assert (info["farthest"][routed] == info["path_steps"][routed]).all()


def test_the_named_positions(case):
    """What each named position was made to catch, by the truth (which the harness equals, above)."""
    names, shape = case.names, SHAPE["17"]
    fields, info, paths = truth_for(case, shape, MAX_STEPS, 252)
    at = lambda name: info[names[name]]
    for name, i in names.items():
        if name.startswith(("nan", "inf", "-inf")):
            assert tuple(info[i]) == (INVALID, 0, 0, 0, NONE, NONE, NONE, 0) and (fields[i, :shape.voxels] == NO_POSITION).all() and (paths[i] == NONE).all(), name
    assert sum(name.startswith(("nan", "inf", "-inf")) for name in names) == 10
    # far away all is air: nothing is a floor, nobody stands
    for name in ("far_all", "beyond_int32"):
        assert tuple(at(name)) == (0, 0, 0, 0, NONE, NONE, NONE, 0) and (fields[names[name], :shape.voxels] == NO_STAND).all(), name
    assert start_of(case.positions[names["minus_zero"]]) == [0, 0, 0] and at("minus_zero")["reached"] != INVALID
    for name in ("goal_inf", "goal_-inf"):  # no goal, not an error
        assert at(name)["reached"] != INVALID and at(name)["goal_ry"] == NONE and at(name)["path_steps"] == NONE and (paths[names[name]] == NONE).all()
    if case.name == "tower":
        r = at("lod_seam")
        assert r["reached"] >= 20 and r["path_steps"] != NONE and (fields[names["lod_seam"], :shape.voxels] <= MAX_STEPS).sum() == r["reached"]
    if case.name == "burrow":
        # the serpentine, one cell high, under a box that covers the chunk: 250 of its 463 steps for an agent one cell high
        named = np.arange(SEEDED, len(case.positions))
        pts, goals = case.positions[named], case.goals[named]
        serpent = Shape("serpent", (32, 31, 32), (1, 4, 1), height=1)
        (raw, stride, _), (graw, gstride, _) = in_form(pts, "packed"), in_form(goals, "packed")
        got = case.host.walk(raw, stride, graw, gstride, len(pts), serpent, MAX_STEPS, 252)
        i, j = names["serpentine_start"] - SEEDED, names["serpentine_near"] - SEEDED
        assert start_of(pts[i]) == [BURROW_AT + 1, BURROW_AT + 4, BURROW_AT + 1]
        assert tuple(got[1][i]) == (251, 250, 0, 0, 4, 4, NONE, 0) and (got[2][i] == NONE).all()      # the far end lies 463 steps off
        assert tuple(got[1][j])[:7] == (251, 250, 0, 0, 4, 4, 31) and (got[2][j][:31] != NONE).all() and (got[2][j][31:] == NONE).all()
        k = names["serpentine_far"] - SEEDED  # (eight rows of 29 steps and their links of 2, then 2 more: the last step there is)
        assert tuple(got[1][k])[:7] == (251, 250, 0, 0, 4, 4, 250) and (got[2][k][:250] != NONE).all() and (got[2][k][250:] == NONE).all() and got[2][k][249] == (3 | 4 << 8 | 17 << 16)
        assert got[2][j][0] == (2 | 4 << 8 | 1 << 16) and got[2][j][30] == (30 | 4 << 8 | 3 << 16)  # (29 along z = 1, 2 through the link at x = 30)
        assert differing(got, points_truth(case, pts, goals, serpent, MAX_STEPS, 252)) is None
        stop = case.host.walk(raw, stride, graw, gstride, len(pts), serpent, MAX_STEPS, 4, STOP)
        assert tuple(stop[1][j])[:7] == (32, 31, 0, 0, 4, 4, 31) and tuple(stop[1][i])[:2] == (251, 250)
        assert differing(stop, points_truth(case, pts, goals, serpent, MAX_STEPS, 4, STOP)) is None
        # two cells high, nobody walks the serpentine; the sealed room's floor is nine cells
        assert tuple(at("serpentine_start"))[:5] == (0, 0, 0, 0, NONE) and tuple(at("room")) == (9, 2, 0, 0, 5, 5, 2, 0) and at("on_top")["reached"] >= 100
    if case.name != "steps":
        return
    h1, h4 = SHAPE["32x31_h1"], SHAPE["32x28_h4"]
    one, four, flat = truth_for(case, h1, MAX_STEPS, 252), truth_for(case, h4, MAX_STEPS, 252), truth_for(case, SHAPE["17_flat"], MAX_STEPS, 252)
    dys = lambda answer, name, start_ry: np.diff(np.concatenate([[start_ry], (answer[2][names[name]][:answer[1][names[name]]["path_steps"]] >> 8) & 0xFF]).astype(np.int64)).tolist()
    # the staircase is climbed a step at a time; the 2-high step is not; without climb neither
    assert at("stairs_up")["path_steps"] == 7 and dys((fields, info, paths), "stairs_up", 6) == [0, 1, 1, 1, 1, 0, 0]
    assert at("two_high_step")["path_steps"] == NONE and at("two_high_step")["goal_ry"] == 8
    assert flat[1][names["stairs_up"]]["path_steps"] == NONE and flat[1][names["stairs_up"]]["reached"] == 8  # (the lane's ground before the first step)
    # ledges: 1, 2 and 3 down are edges, one way where they are higher than a step; 4 down is none
    assert at("ledges_down")["path_steps"] == 8 and dys((fields, info, paths), "ledges_down", 6) == [-1, 0, 0, 0, -2, 0, 0, 0]
    assert at("ledge_three")["path_steps"] == 5 and dys((fields, info, paths), "ledge_three", 6) == [0, 0, -3, 0, 0]
    assert at("ledge_four")["path_steps"] == NONE and at("ledge_four")["goal_ry"] == 2
    assert at("ledges_back_up")["path_steps"] == 4 and dys((fields, info, paths), "ledges_back_up", 6) == [0, 0, 1, 0]
    assert flat[1][names["ledges_down"]]["path_steps"] == NONE
    # corridors: one cell high takes an agent of height 1, two cells high one of height 2, neither one of height 4
    assert one[1][names["corridor_1"]]["path_steps"] == 8 and at("corridor_1")["path_steps"] == NONE and at("corridor_1")["goal_ry"] == NONE
    assert at("corridor_2")["path_steps"] == 8 and one[1][names["corridor_2"]]["path_steps"] == 8
    assert four[1][names["corridor_2"]]["path_steps"] == NONE and four[1][names["corridor_2"]]["start_ry"] == h4.seed_at[1]
    # a ceiling over the source column stops the step up at height 2, not at height 1; a lintel over the destination column the drop
    assert at("low_ceiling")["path_steps"] == NONE and at("low_ceiling")["goal_ry"] != NONE and one[1][names["low_ceiling"]]["path_steps"] == 5
    assert at("lintel")["path_steps"] == NONE and at("lintel")["goal_ry"] != NONE and one[1][names["lintel"]]["path_steps"] == 5
    # a floor of pass_value blocks: one walks over it without pass_value, and a layer lower with it
    passing = truth_for(case, shape, MAX_STEPS, 252, 0, 9)
    assert at("pass_floor")["path_steps"] == 8 and dys((fields, info, paths), "pass_floor", 6) == [0] * 8
    assert passing[1][names["pass_floor"]]["path_steps"] == 8 and dys(passing, "pass_floor", 6) == [0, -1, 0, 0, 0, 0, 1, 0]
    # settling
    assert tuple(at("in_air"))[3:7] == (0, 4, 4, 2) and at("in_air")["reached"] >= 10
    assert tuple(at("over_hole")) == (0, 0, 0, 0, NONE, 5, NONE, 0) and tuple(at("in_rock")) == (0, 0, 0, 3, NONE, 11, NONE, 0)  # (ry counts from the box's bottom)
    assert (fields[names["over_hole"], :shape.voxels] == UNREACHED).any()  # (its field still tells standable from not)
    assert tuple(at("goal_is_seed"))[4:7] == (6, 6, 0) and (paths[names["goal_is_seed"]] == NONE).all()
    assert tuple(at("goal_outside"))[4:7] == (6, NONE, NONE) and tuple(at("goal_nan"))[4:7] == (6, NONE, NONE)
    assert tuple(at("goal_in_air"))[4:7] == (6, 6, 3)
    stop = truth_for(case, shape, MAX_STEPS, 4, STOP)
    assert tuple(stop[1][names["goal_is_seed"]])[:2] == (1, 0) and tuple(stop[1][names["goal_in_air"]])[1] == 3 and stop[1][names["goal_nan"]]["farthest"] > 3
    # the world's floor: one stands on y = 0's blocks at y = 1, with no world beneath them
    r = at("world_floor")
    assert start_of(case.positions[names["world_floor"]])[1] == 1 and tuple(r)[:2] == (14, 5) and tuple(r)[4:7] == (6, 6, 4) and STEPS_AT[1] == 0


def test_outputs_and_strides(case):
    """Fields only, records only, paths only, no goal, one goal for all, a stride larger than the box (the bytes beyond the rounded voxel count
    keep their sentinel), one query, none."""
    shape = SHAPE["9_two_bricks"]
    pts, goals = positions_for(case, shape)
    (raw, stride, _), (graw, gstride, _) = in_form(pts, "stride16"), in_form(goals, "entities")
    exp = truth_for(case, shape, 24, 4)
    n = len(pts)
    f, i, p = case.host.walk(raw, stride, graw, gstride, n, shape, 24, 4, info=False, paths=False)
    assert i is None and p is None and (f == exp[0]).all()
    f, i, p = case.host.walk(raw, stride, graw, gstride, n, shape, 24, 4, fields=False, paths=False)
    assert f is None and p is None and i.tobytes() == exp[1].tobytes()
    f, i, p = case.host.walk(raw, stride, graw, gstride, n, shape, 24, 4, fields=False, info=False)
    assert f is None and i is None and (p == exp[2]).all()
    got = case.host.walk(raw, stride, None, 0, n, shape, 24, 4, paths=False)
    assert (got[0] == exp[0]).all() and got[1].tobytes() == truth_for(case, shape, 24, 0, 0, 0, with_goal=False)[1].tobytes()
    one_goal = np.ascontiguousarray(goals[SEEDED // 2 + 3])
    got = case.host.walk(raw, stride, one_goal.view(np.uint8), 0, n, shape, 24, 4)
    assert differing(got, points_truth(case, pts, np.tile(one_goal, (n, 1)), shape, 24, 4)) is None
    f, i, p = case.host.walk(raw, stride, graw, gstride, n, shape, 24, 4, field_stride=shape.padded + 32)
    assert (f[:, :shape.padded] == exp[0]).all() and (f[:, shape.padded:] == 0x5a).all() and i.tobytes() == exp[1].tobytes() and (p == exp[2]).all()
    f, i, p = case.host.walk(raw[7 * 16:], stride, graw[7 * 64:], gstride, 1, shape, 24, 4)
    assert (f == exp[0][7:8]).all() and i.tobytes() == exp[1][7:8].tobytes() and (p == exp[2][7:8]).all()
    f, i, p = case.host.walk(raw[:0], stride, graw[:0], gstride, 0, shape, 24, 4)
    assert f.size == 0 and i.size == 0 and p.size == 0


@pytest.mark.parametrize("name", ["steps", "burrow", "tower"])
def test_the_sanitized_program(exe, name):
    """The same program under -fsanitize=address,undefined -fno-sanitize-recover=all, run directly: every call of `steps`, `burrow` and
    `tower`, both formats, on 60 seeded positions and every named one -- 3e9, -3e9, 1e30 and the positions beyond int32 among them. A finding
    ends the program with a non-zero status; its bytes are the plain program's."""
    san = harness(sanitize=True)
    for fmt in ("esvo", "csvo"):
        c = make_walk_case(name, fmt)
        plain, checked = HostWalk(exe, c), HostWalk(san, c)
        pick = np.concatenate([np.arange(0, SEEDED, 5), np.arange(SEEDED, len(c.positions))])
        try:
            for call in calls_for(c):
                a, b = plain.call(c, call, pick), checked.call(c, call, pick)
                assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), (fmt, call[0])
        finally:
            plain.close()
            checked.close()


def test_the_rules_refuse_what_the_abi_lists(exe):
    """vx_walk.hpp's argument rules on their own: each bad value named by its field, what is allowed allowed."""
    out = subprocess.run([str(exe), "rules"], stdout=subprocess.PIPE, text=True, check=True).stdout
    said = dict(ln.split(": ", 1) for ln in out.splitlines())
    for ok in ("packed", "entities", "one goal", "no goal", "no goal, any goal_stride", "fields only", "info only", "paths only", "info only, any stride", "count 0",
               "largest box", "smallest box", "31 layers and 1", "28 layers and 4", "height 1", "height 4", "climb 0", "climb 1", "drop 0", "drop 3", "path_capacity 0",
               "path_capacity 4", "path_capacity 252", "flags 1", "any pass_value", "field_stride 3472", "field_stride 4096", "field bytes 2^24",
               "field bytes by the default stride, one fewer", "path bytes 2^24"):
        assert said[ok] == "ok", (ok, said[ok])
    assert said["too many"].startswith("count exceeds 16777216")
    assert said["null shape"] == "null shape" and said["null pos"] == "null pos" and said["no output"] == "fields, info and paths are all null"
    assert said["paths without goal"] == "paths without goal"
    for stride in (0, 4, 8, 13, 14):
        assert said[f"pos_stride {stride}"].startswith("pos_stride"), stride
    for stride in (4, 8, 13, 14):
        assert said[f"goal_stride {stride}"].startswith("goal_stride"), stride
    assert said["goal_stride 16"] == "ok"
    for off in (1, 2, 3):
        assert said[f"pos + {off}"].startswith("pos must be aligned") and said[f"goal + {off}"].startswith("goal must be aligned"), off
    for a in range(3):
        for side in (0, 33, 0xFFFFFFFF):
            assert said[f"size[{a}] {side}"].startswith("size"), (a, side)
        assert said[f"seed_at[{a}] 17"].startswith("seed_at"), a
    for h in (0, 5, 0xFFFFFFFF):
        assert said[f"height {h}"].startswith("height"), h
    assert said["31 layers and 2"].startswith("size[1] + height") and said["32 layers and 1"].startswith("size[1] + height")
    assert said["max_steps 251"].startswith("max_steps")
    for v in (2, 0xFFFFFFFF):
        assert said[f"climb {v}"].startswith("climb"), v
    for v in (4, 0xFFFFFFFF):
        assert said[f"drop {v}"].startswith("drop"), v
    for v in (6, 253, 256):
        assert said[f"path_capacity {v}"].startswith("path_capacity"), v
    for flags in (2, 3, 0x80000000):
        assert said[f"flags {flags}"].startswith("flags"), flags
    for stride in (3468, 3470, 3456, 16):
        assert said[f"field_stride {stride}"].startswith("field_stride"), stride
    assert said["field bytes 2^24 + 4096"].startswith("count * field_stride") and said["field bytes by the default stride"].startswith("count * field_stride")
    assert said["path bytes beyond 2^24"].startswith("count * path_capacity * 4")
    assert hip.WALK_INFO_DTYPE.itemsize == 32 and len(SHAPES) == 8 and STEP_LIMITS == (0, 1, 24, 250) and PATH_CAPACITIES == (0, 4, 252)
