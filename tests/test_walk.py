"""vx_walk_points on the GPU (voxel-rs_amd/csrc/blocks/kernels_walk.hip): walking distances and paths for ground agents around a batch of
positions, against the host harness's bytes (tests/cpp/walk_on_host.cpp: the same header on the host), which are held against numpy over the dense
arrays here and in tests/test_walk_on_host.py, and against numpy directly where the world or the positions change. Five worlds, both formats; every
comparison is byte for byte. A case -- every third seeded position and every named one, every call of walk_cases.calls_for -- is computed
once and left unchanged."""
import ctypes as C

import numpy as np
import pytest

from batch_cases import _chunk_of
from gpu_harness import (SENTINEL, big_esvo_context, field_rows, flying_entities, leaves_the_outputs_alone, make_context, records_head, sentinel_bytes, sentinel_words,
                         shared_cases)
from helpers import vra  # noqa: F401
from physics_cases import DT
from voxel_rs_amd import hip
from walk_cases import (INVALID, MAX_STEPS, NONE, SEEDED, SHAPE, STEPS_AT, STOP, WALK_CASES, HostWalk, Shape, calls_for, differing, harness, in_form, make_walk_case, points_truth,
                        positions_for, steps_blocks, torch_positions, truth_for)

pytestmark = pytest.mark.gpu
filled_fields = sentinel_bytes  # (count, stride): the fields at their stride and the tail
filled_words = sentinel_words  # (count, width): records are 8 words wide; a path is its capacity, or 4 where that is 0


def walk(svo, pos, goals, shape, max_steps, cap=0, flags=0, pass_value=0, **outputs):
    return svo.walk_points(pos, shape.size, goals, shape.seed_at, max_steps, pass_value, shape.height, shape.climb, shape.drop, cap, flags, **outputs)


def check_device(got, count, stride, cap, exp, what):
    """Buffers longer than the call needs: the fields at their stride with the sentinel between and behind them, the records and two more,
    the paths and two rows more. An output that is None was not asked for."""
    fields, info, paths = got
    exp_fields, exp_info, exp_paths = exp
    got_fields = exp_fields if fields is None else field_rows(fields, count, stride, exp_fields.shape[1], what)
    got_info = exp_info if info is None else records_head(hip.walk_infos_to_numpy(info), count, what)
    got_paths = exp_paths if paths is None else records_head(paths.reshape(-1), count * cap, what).view(np.uint32).reshape(count, cap)
    d = differing((got_fields, got_info, got_paths), exp)
    assert d is None, f"{what}: {d}"


def build(name, fmt):
    """The world, a context that has it, the positions the GPU is asked about and the harness's bytes for every call; shared by the tests."""
    c = make_walk_case(name, fmt)
    c.pick = np.concatenate([np.arange(0, SEEDED, 3), np.arange(SEEDED, len(c.positions))])
    c.calls = calls_for(c)
    host = HostWalk(harness(), c)
    c.expected = {call[0]: host.call(c, call, c.pick) for call in c.calls}
    host.close()
    for call, shape, max_steps, cap, flags, pass_value, _ in c.calls:  # (the harness's bytes are numpy's)
        truth = tuple(a[c.pick] for a in truth_for(c, shape, max_steps, cap, flags, pass_value))
        assert differing(c.expected[call], truth) is None, f"{call}: the harness differs from the dense truth: {differing(c.expected[call], truth)}"
    c.svo = make_context(c)
    return c


the_case, _contexts, case = shared_cases(build, WALK_CASES)


def queue_calls(svo, c):
    """Every call of the case into device memory, in buffers longer than it needs; [(positions, goals, host views, outputs)]."""
    n, queued = len(c.pick), []
    for name, shape, max_steps, cap, flags, pass_value, form in c.calls:
        pts, goals = positions_for(c, shape)
        (raw, stride, view), (graw, gstride, gview) = in_form(pts[c.pick], form), in_form(goals[c.pick], form)
        pos, goal = torch_positions(raw, stride, n), torch_positions(graw, gstride, n)
        got = walk(svo, pos, goal, shape, max_steps, cap, flags, pass_value, fields=filled_fields(n, shape.padded), info=filled_words(n, 8), paths=filled_words(n, cap or 4))
        queued.append((pos, goal, view, gview, got))
    return queued


def test_device_and_host_memory_give_the_harness_bytes(case):
    """Every call -- every shape at every step limit, the path capacities, the flag, a pass_value, the forms in turn, vx_entity records among
    them --: the device calls queued together before one vx_sync, each into buffers longer than it needs; then the same positions as
    host-memory calls."""
    svo, n = case.svo, len(case.pick)
    queued = queue_calls(svo, case)
    svo.sync()
    for (name, shape, max_steps, cap, flags, pass_value, form), (_, _, view, gview, got) in zip(case.calls, queued):
        exp = case.expected[name]
        check_device(got, n, shape.padded, cap, exp, f"{case.name}-{case.fmt} {name}")
        hf, hi, hp = walk(svo, view, gview, shape, max_steps, cap, flags, pass_value, paths=True)
        assert hi.dtype == hip.WALK_INFO_DTYPE and differing((hf, hi, hp), exp) is None, f"{name} in host memory: {differing((hf, hi, hp), exp)}"
    full = case.expected["17-250"][1]
    assert (full["reached"] == INVALID).sum() == 10 and (full["reached"][:SEEDED // 3] >= 2).mean() >= 0.25
    print(f"\n{case.name}-{case.fmt}: {2 * n * len(case.calls)} walks")


def test_outputs_and_strides(case):
    """Fields only, records only, paths with and without fields, under VX_WALK_STOP_AT_GOAL, no goal, one goal for all, and a field_stride
    larger than the box (the bytes beyond the rounded voxel count keep their sentinel), in device and in host memory; one query; none."""
    svo, shape, n, cap = case.svo, SHAPE["17"], len(case.pick), 4
    exp = case.expected["17-stop-4"]
    form = [c for c in case.calls if c[0] == "17-stop-4"][0][6]
    pts, goals = positions_for(case, shape)
    (raw, stride, view), (graw, gstride, gview) = in_form(pts[case.pick], form), in_form(goals[case.pick], form)
    pos, goal = torch_positions(raw, stride, n), torch_positions(graw, gstride, n)
    wide = shape.padded + 32
    bufs = lambda count=n, width=shape.padded: dict(fields=filled_fields(count, width), info=filled_words(count, 8), paths=filled_words(count, cap))
    f_only = walk(svo, pos, goal, shape, 250, cap, STOP, **{**bufs(), "info": None, "paths": False})
    i_only = walk(svo, pos, goal, shape, 250, cap, STOP, **{**bufs(), "fields": None, "paths": False})
    p_only = walk(svo, pos, goal, shape, 250, cap, STOP, **{**bufs(), "fields": None, "info": None})
    p_fields = walk(svo, pos, goal, shape, 250, cap, STOP, **{**bufs(), "info": None})
    both = walk(svo, pos, goal, shape, 250, cap, STOP, field_stride=wide, **bufs(n, wide))
    no_goal = walk(svo, pos, None, shape, 250, cap, STOP, **{**bufs(), "paths": False})
    one_goal = walk(svo, pos, goal[40], shape, 250, cap, STOP, **bufs())
    one = walk(svo, pos[7:8], goal[7:8], shape, 250, cap, STOP, **bufs(1))
    none = walk(svo, pos[:0], goal[:0], shape, 250, cap, STOP, **bufs(0))
    svo.sync()
    assert f_only[1] is None and f_only[2] is None and i_only[0] is None and i_only[2] is None and p_only[0] is None and p_only[1] is None and p_fields[1] is None
    check_device(f_only, n, shape.padded, cap, exp, "fields only")
    check_device(i_only, n, shape.padded, cap, exp, "records only")
    check_device(p_only, n, shape.padded, cap, exp, "paths only")
    check_device(p_fields, n, shape.padded, cap, exp, "paths and fields")
    check_device(both, n, wide, cap, exp, "a stride larger than the box")
    exp_no_goal = points_truth(case, pts[case.pick], None, shape, 250, 0, STOP)
    assert no_goal[2] is None
    check_device(no_goal, n, shape.padded, 0, exp_no_goal, "no goal")
    assert (exp_no_goal[1]["goal_ry"] == NONE).all() and (exp_no_goal[1]["path_steps"] == NONE).all()
    exp_one_goal = points_truth(case, pts[case.pick], np.tile(gview[40], (n, 1)), shape, 250, cap, STOP)
    check_device(one_goal, n, shape.padded, cap, exp_one_goal, "one goal for all")
    check_device(one, 1, shape.padded, cap, tuple(e[7:8] for e in exp), "one query")
    check_device(none, 0, shape.padded, cap, tuple(e[:0] for e in exp), "no query")
    # host memory
    hf, hi, hp = walk(svo, view, gview, shape, 250, cap, STOP, info=None, paths=False)
    assert hi is None and hp is None and (hf == exp[0]).all()
    hf, hi, hp = walk(svo, view, gview, shape, 250, cap, STOP, fields=None, paths=False)
    assert hf is None and hp is None and hi.tobytes() == exp[1].tobytes()
    hf, hi, hp = walk(svo, view, gview, shape, 250, cap, STOP, fields=None, info=None)
    assert hf is None and hi is None and (hp == exp[2]).all()
    out = np.full((n, wide), 0x5A, dtype=np.uint8)
    hf, hi, hp = walk(svo, view, gview, shape, 250, cap, STOP, fields=out, field_stride=wide)
    assert (out[:, :shape.padded] == exp[0]).all() and (out[:, shape.padded:] == 0x5A).all() and hi.tobytes() == exp[1].tobytes() and (hp == exp[2]).all()
    assert differing(walk(svo, view, np.ascontiguousarray(gview[40]), shape, 250, cap, STOP), exp_one_goal) is None
    hf, hi, hp = walk(svo, view, None, shape, 250, cap, STOP)
    assert hp is None and (hf == exp_no_goal[0]).all() and hi.tobytes() == exp_no_goal[1].tobytes()
    assert differing(walk(svo, view[7:8], gview[7:8], shape, 250, cap, STOP), tuple(e[7:8] for e in exp)) is None
    hf, hi, hp = walk(svo, view[:0], gview[:0], shape, 250, cap, STOP)
    assert hf.shape == (0, shape.padded) and hi.shape == (0,) and hp.shape == (0, cap)


@pytest.mark.parametrize("fmt", ["esvo", "csvo"])
def test_the_serpentine(fmt):
    """`burrow`'s corridor one cell high under a box that covers the chunk, for an agent one cell high: the longest search and the longest
    back-trace there are -- 250 steps, a path of 250 entries in a capacity of 252 --, a goal 31 steps off and one 463 steps off, which is not
    reached; with and without VX_WALK_STOP_AT_GOAL, as numpy has them."""
    c = the_case("burrow", fmt)
    named = np.arange(SEEDED, len(c.positions))
    pts, goals = c.positions[named], c.goals[named]
    serpent = Shape("serpent", (32, 31, 32), (1, 4, 1), height=1)
    (raw, stride, view), (graw, gstride, gview) = in_form(pts, "entities"), in_form(goals, "packed")
    pos, goal = torch_positions(raw, stride, len(pts)), torch_positions(graw, gstride, len(pts))
    bufs = lambda: dict(fields=filled_fields(len(pts), serpent.padded), info=filled_words(len(pts), 8), paths=filled_words(len(pts), 252))
    plain, stop = walk(c.svo, pos, goal, serpent, MAX_STEPS, 252, **bufs()), walk(c.svo, pos, goal, serpent, MAX_STEPS, 252, STOP, **bufs())
    c.svo.sync()
    exp, exp_stop = points_truth(c, pts, goals, serpent, MAX_STEPS, 252), points_truth(c, pts, goals, serpent, MAX_STEPS, 252, STOP)
    steps = {name: int(exp[1][c.names[name] - SEEDED]["path_steps"]) for name in ("serpentine_start", "serpentine_near", "serpentine_far")}
    assert steps == {"serpentine_start": NONE, "serpentine_near": 31, "serpentine_far": 250} and exp_stop[1][c.names["serpentine_near"] - SEEDED]["reached"] == 32
    check_device(plain, len(pts), serpent.padded, 252, exp, "the serpentine")
    check_device(stop, len(pts), serpent.padded, 252, exp_stop, "the serpentine, stopping at the goal")
    assert differing(walk(c.svo, view, gview, serpent, MAX_STEPS, 252, STOP), exp_stop) is None


@pytest.mark.parametrize("fmt", ["esvo", "csvo"])
def test_behind_physics_step(fmt):
    """256 flying entities in device memory stepped 8 times (they move 1.28 voxels down and sideways), then vx_walk_points over the same
    records' positions in place with no sync between the two calls; after one vx_sync the entities are read back, and fields, records and
    paths are numpy's for the positions the steps left -- which differ from those of the positions before."""
    import torch

    c = the_case("glasshouse", fmt)
    rng = np.random.default_rng(191)
    e = flying_entities(256, rng.uniform((2.0, 2.0, 2.0), (30.0, 6.0, 30.0), (256, 3)), rng)
    goal = np.array([16.5, 1.5, 6.5], dtype=np.float32)
    shape, cap = SHAPE["17"], 252
    d = torch.from_numpy(e.view(np.uint8).copy()).cuda()
    c.svo.physics_step(d, DT, 8)
    got = walk(c.svo, hip.entity_positions(d), torch.from_numpy(goal).cuda(), shape, 24, cap, fields=filled_fields(256, shape.padded), info=filled_words(256, 8),
               paths=filled_words(256, cap))
    c.svo.sync()
    after = d.cpu().numpy().view(hip.ENTITY_DTYPE)
    assert (after["position"][:, 1] < e["position"][:, 1] - 1.0).all()
    goals = np.tile(goal, (256, 1))
    before = points_truth(c, e["position"], goals, shape, 24, cap)
    exp = points_truth(c, after["position"], goals, shape, 24, cap)
    assert ((before[0] != exp[0]).any(axis=1)).sum() >= 64 and (exp[1]["path_steps"] != NONE).sum() >= 16
    check_device(got, 256, shape.padded, cap, exp, "behind vx_physics_step")
    assert differing(walk(c.svo, hip.entity_positions(after), goal, shape, 24, cap), exp) is None


@pytest.mark.parametrize("fmt", ["esvo", "csvo"])
def test_a_commit_opens_a_wall(fmt):
    """`steps`: a call into device memory, a doorway two cells high cut through the wall between the last two lanes on the host chunk and
    committed with vx_commit_all, the call again into other buffers, one vx_sync: the first buffers show the old world -- the goal in the
    other lane not reached --, the second the new one with the path through the doorway; both exactly as numpy has them (the commit's
    uploads wait for the event mark_world_read records behind the launch)."""
    c = make_walk_case("steps", fmt)
    svo = make_context(c)
    try:
        shape, cap = SHAPE["17"], 252
        pts = (STEPS_AT + np.array([(4, 8, 29), (6, 10, 30), (4, 8, 25)]) + 0.5).astype(np.float32)
        goals = (STEPS_AT + np.array([(4, 8, 25), (6, 8, 26), (4, 8, 29)]) + 0.5).astype(np.float32)
        (raw, stride, _), (graw, gstride, _) = in_form(pts, "packed"), in_form(goals, "stride16")
        pos, goal = torch_positions(raw, stride, len(pts)), torch_positions(graw, gstride, len(pts))
        bufs = lambda: dict(fields=filled_fields(len(pts), shape.padded), info=filled_words(len(pts), 8), paths=filled_words(len(pts), cap))
        old = points_truth(c, pts, goals, shape, MAX_STEPS, cap)
        first = walk(svo, pos, goal, shape, MAX_STEPS, cap, **bufs())
        b = steps_blocks()
        b[4, 8:10, 27:29] = 0  # through the walls at z = 27 and z = 28
        c.world.set_chunk((1, 0, 1), _chunk_of((1, 0, 1), 5, b))
        c.world.serialize()
        svo.update_full(c.world)  # vx_commit_all
        changed = c.truth.copy()
        changed[:32, :32, :32] = b
        new = points_truth(c, pts, goals, shape, MAX_STEPS, cap, truth=changed)
        second = walk(svo, pos, goal, shape, MAX_STEPS, cap, **bufs())
        svo.sync()
        assert (old[1]["path_steps"] == NONE).all() and new[1]["path_steps"].tolist() == [4, 8, 4] and (new[1]["reached"] > old[1]["reached"]).all()
        check_device(first, len(pts), shape.padded, cap, old, "before the commit")
        check_device(second, len(pts), shape.padded, cap, new, "after the commit")
    finally:
        svo.close()


def test_esvo_big():
    """`steps` in an ESVO context of 4 GiB, which selects the VX_SVO_ESVO_BIG build of the kernel: every call."""
    c = the_case("steps", "esvo")
    with big_esvo_context(c) as svo:
        queued = queue_calls(svo, c)
        svo.sync()
        for (name, shape, max_steps, cap, *_), (_, _, _, _, got) in zip(c.calls, queued):
            check_device(got, len(c.pick), shape.padded, cap, c.expected[name], name)
        name, shape, max_steps, cap, flags, pass_value, form = c.calls[-1]
        _, _, view, gview, _ = queued[-1]
        assert differing(walk(svo, view, gview, shape, max_steps, cap, flags, pass_value, paths=True), c.expected[name]) is None


def test_errors_leave_the_output_alone(case):
    """Every invalid argument returns VX_ERR_INVALID_ARGUMENT with the field named and leaves host and device outputs at their sentinels; a
    context without a commit returns VX_ERR_STATE; count == 0 is VX_OK and writes nothing."""
    import torch

    L, h, vp = hip.lib(), case.svo._h, C.c_void_p
    fields = np.full(2 * 3472 + 16, 0x5A, dtype=np.uint8)
    paths = np.full(3 * 252, SENTINEL, dtype=np.uint32)
    info = np.full(3, SENTINEL, dtype=np.uint32).repeat(8)
    d_fields, d_paths, d_info = filled_fields(2, 3472), filled_words(2, 252), filled_words(2, 8)
    v = np.tile(np.array([3.5, 3.5, 3.5], dtype=np.float32), 8)
    d_v = torch.from_numpy(v).cuda()
    assert d_fields.data_ptr() % 16 == 0 and d_paths.data_ptr() % 16 == 0 and d_info.data_ptr() % 16 == 0 and v.ctypes.data % 4 == 0

    def shape(**fields_):
        s = hip.walk_shape((17, 12, 17), (8, 6, 8), 250, path_capacity=252)
        for k, val in fields_.items():
            setattr(s, k, val)
        return s

    u3 = C.c_uint32 * 3
    hb, db = v.ctypes.data, d_v.data_ptr()
    hf, hp, hi = vp(fields.ctypes.data), vp(paths.ctypes.data), vp(info.ctypes.data)
    df, dp, di = vp(d_fields.data_ptr()), vp(d_paths.data_ptr()), vp(d_info.data_ptr())
    H, D = hip.VX_MEM_HOST, hip.VX_MEM_DEVICE

    def host_call(ctx=h, pos=hb, pos_stride=12, goal=hb, goal_stride=12, count=2, s=None, memory=H, f=hf, field_stride=0, p=hp, i=hi, no_shape=False, **shape_fields):
        return L.vx_walk_points(ctx, pos, pos_stride, goal, goal_stride, count, None if no_shape else C.byref(shape(**shape_fields)), memory, f, field_stride, p, i)

    refusals = ((lambda: host_call(ctx=None), b"null context"),
                (lambda: host_call(memory=3), b"VX_MEM"),
                (lambda: host_call(no_shape=True), b"null shape"),
                (lambda: host_call(pos=None), b"null pos"),
                (lambda: host_call(f=None, p=None, i=None), b"fields, info and paths"),
                (lambda: host_call(goal=None), b"paths without goal"),
                (lambda: host_call(pos_stride=8), b"pos_stride"),
                (lambda: host_call(pos=hb + 2), b"pos must be aligned"),
                (lambda: host_call(goal_stride=8), b"goal_stride"),
                (lambda: host_call(goal=hb + 2), b"goal must be aligned"),
                (lambda: host_call(size=u3(17, 0, 17), seed_at=u3(8, 0, 8)), b"size"),
                (lambda: host_call(size=u3(17, 12, 33)), b"size"),
                (lambda: host_call(seed_at=u3(17, 6, 8)), b"seed_at"),
                (lambda: host_call(height=0), b"height"),
                (lambda: host_call(height=5), b"height"),
                (lambda: host_call(size=u3(17, 31, 17)), b"size[1] + height"),
                (lambda: host_call(max_steps=251), b"max_steps"),
                (lambda: host_call(climb=2), b"climb"),
                (lambda: host_call(drop=4), b"drop"),
                (lambda: host_call(path_capacity=6), b"path_capacity"),
                (lambda: host_call(path_capacity=256), b"path_capacity"),
                (lambda: host_call(flags=2), b"flags"),
                (lambda: host_call(field_stride=3456), b"field_stride"),
                (lambda: host_call(field_stride=3480), b"field_stride"),
                (lambda: host_call(count=(1 << 24) + 1, f=None, p=None), b"count exceeds"),
                (lambda: host_call(count=4833), b"count * field_stride"),
                (lambda: host_call(count=16645, f=None), b"count * path_capacity * 4"),
                (lambda: host_call(pos=db, goal=db, memory=D, f=vp(d_fields.data_ptr() + 8), p=dp, i=di), b"fields in device memory"),
                (lambda: host_call(pos=db, goal=db, memory=D, f=df, p=vp(d_paths.data_ptr() + 4), i=di), b"paths in device memory"),
                (lambda: host_call(pos=db, goal=db, memory=D, f=df, p=dp, i=vp(d_info.data_ptr() + 4)), b"info in device memory"),
                (lambda: host_call(pos=db + 1, goal=db, memory=D, f=df, p=dp, i=di), b"pos must be aligned"))
    uncommitted = (lambda ctx: host_call(ctx=ctx), lambda ctx: host_call(ctx=ctx, pos=db, goal=db, memory=D, f=df, p=dp, i=di))
    # count == 0: VX_OK whatever the rest is; nothing is read or written
    nothing_to_do = (lambda: host_call(count=0),
                     lambda: L.vx_walk_points(h, None, 0, None, 0, 0, None, H, None, 0, None, None),
                     lambda: host_call(count=0, pos=db, goal=db, memory=D, f=df, p=dp, i=di))
    leaves_the_outputs_alone(case, [fields, paths, info], [d_fields, d_paths, d_info], refusals, uncommitted, nothing_to_do)
    # and the call still works: two queries at (3.5, 3.5, 3.5) with themselves as the goal, as numpy has them
    assert host_call() == 0
    pts = v[:6].reshape(2, 3)
    exp = points_truth(case, pts, pts, SHAPE["17"], 250, 252)
    assert fields[:2 * 3472].tobytes() == exp[0].tobytes() and (fields[2 * 3472:] == 0x5A).all()
    assert paths[:2 * 252].tobytes() == exp[2].tobytes() and (paths[2 * 252:] == SENTINEL).all()
    assert info[:16].tobytes() == exp[1].tobytes() and (info[16:] == SENTINEL).all()
