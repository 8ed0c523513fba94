"""vx_distance_boxes on the GPU (voxel-rs_amd/csrc/blocks/kernels_distance.hip): the squared distance to the nearest block, per cell, in a
batch of boxes, against the host harness's bytes (tests/cpp/distance_on_host.cpp: the same header on the host, which
tests/test_distance_on_host.py holds against numpy over the dense arrays) and against numpy directly where the world or the boxes change.
Five worlds, both formats; every comparison is entry for entry and record for record. A case -- ten seeded boxes, five of the uniform ones and
five of those around the blocks' surface, and every named one; every call of distance_cases.calls_for -- is computed once and left unchanged."""
import ctypes as C

import numpy as np
import pytest

from batch_cases import _chunk_of
from distance_cases import (ABSENT, DISTANCE_CASES, NONE, SEVENTEEN, SHAPE, TO_AIR, HostDistance, boxes_for, calls_for, differing, distance_truth, harness, in_form,
                            make_distance_case, pick_for, torch_boxes)
from gpu_harness import (SENTINEL, big_esvo_context, field_rows, leaves_the_outputs_alone, make_context, records_head, sentinel_bytes, sentinel_words, shared_cases)
from helpers import vra  # noqa: F401
from label_cases import ROCK, RUBBLE_AT, SEEDED, SOLID_ROCK, rubble_blocks
from voxel_rs_amd import hip

pytestmark = pytest.mark.gpu
filled_fields = sentinel_bytes  # (count, stride in bytes): the fields at their stride and the tail


def filled_info(count):
    return sentinel_words(count, 4)


def check_device(fields, info, count, stride, expected, what):
    """Buffers longer than the call needs: the fields at their stride (bytes) with the sentinel between and behind them, the records and two
    more. None: an output the call was not given."""
    exp_fields, exp_info = expected
    got_fields, got_info = exp_fields, exp_info
    if fields is not None:
        got_fields = np.ascontiguousarray(field_rows(fields, count, stride, 2 * exp_fields.shape[1], what)).view(np.uint16)
    if info is not None:
        got_info = records_head(hip.distance_infos_to_numpy(info), count, what)
    assert differing((got_fields, got_info), expected) is None, f"{what}: {differing((got_fields, got_info), expected)}"


def gpu_pick(c, shape):
    """Of pick_for's boxes: five of each kind of seeded box, and every named one."""
    n, named = len(pick_for(c, shape)), len(c.boxes) - SEEDED
    half = (n - named) // 2
    return np.concatenate([np.arange(5), np.arange(half, half + 5), np.arange(n - named, n)])


def gpu_boxes(c, shape):
    return boxes_for(c, shape)[pick_for(c, shape)][gpu_pick(c, shape)]


def build(name, fmt):
    """The world, a context that has it, the boxes the GPU is asked about and the harness's bytes for every call; shared by the tests."""
    c = make_distance_case(name, fmt)
    c.calls = calls_for(c)
    host = HostDistance(harness(), c)
    c.expected = {call[0]: host.call(c, call, gpu_pick(c, call[1])) for call in c.calls}
    host.close()
    c.svo = make_context(c)
    return c


the_case, _contexts, case = shared_cases(build, DISTANCE_CASES)


def asked(c, call, svo=None):
    """One of the case's calls into device memory, into buffers longer than it needs: (lo, fields, info, the fields' stride in bytes)."""
    _, shape, pass_value, match_value, flags, lo_stride, field_stride = call
    boxes = gpu_boxes(c, shape)
    n, stride = len(boxes), field_stride or shape.bytes
    lo = torch_boxes(in_form(boxes, lo_stride)[0], lo_stride, n)
    f, i = (svo or c.svo).distance_boxes(lo, shape.size, pass_value, match_value, flags, fields=filled_fields(n, stride), info=filled_info(n), field_stride=field_stride)
    return lo, f, i, stride


def test_device_and_host_memory_give_the_harness_bytes(case):
    """Every call -- every shape under every kind of target set, the forms of lo and the field strides in turn --: the device calls queued
    together before one vx_sync, each into buffers longer than it needs; then the same boxes as host-memory calls."""
    svo = case.svo
    queued = [asked(case, call) for call in case.calls]
    svo.sync()
    for call, (_, f, i, stride) in zip(case.calls, queued):
        name, shape, pass_value, match_value, flags, lo_stride, field_stride = call
        boxes = gpu_boxes(case, shape)
        check_device(f, i, len(boxes), stride, case.expected[name], f"{case.name}-{case.fmt} {name}")
        view = in_form(boxes, lo_stride)[1]
        hf, hi = svo.distance_boxes(view, shape.size, pass_value, match_value, flags, field_stride=field_stride)
        assert hf.dtype == np.uint16 and hf.shape == (len(boxes), stride // 2) and hi.dtype == hip.DISTANCE_INFO_DTYPE
        got = (hf[:, :shape.entries], hi)
        assert differing(got, case.expected[name]) is None, f"{name} in host memory: {differing(got, case.expected[name])}"
    absent = case.expected["17-absent"]
    assert (absent[0] == NONE).all() and (absent[1]["farthest"] == NONE).all() and (absent[1]["where"] == 0).all()
    if case.name not in ("burrow", "rubble"):  # (there the id is a single cell's: test_the_named_blocks asks for it where it is)
        assert (case.expected["17-match"][1]["targets"] > 0).any()


def test_outputs_and_strides(case):
    """Fields only, records only, and a field_stride larger than the field (the bytes beyond it keep their sentinel), in device and in host
    memory; fresh outputs; one box (count = 1); none."""
    import torch

    svo, shape = case.svo, SHAPE["31x3x17"]
    boxes = gpu_boxes(case, shape)
    n = len(boxes)
    expected = distance_truth(case, boxes, shape)
    raw, view = in_form(boxes, 20)
    lo = torch_boxes(raw, 20, n)
    wide = shape.bytes + 32
    f_only = svo.distance_boxes(lo, shape.size, fields=filled_fields(n, shape.bytes), info=False)
    i_only = svo.distance_boxes(lo, shape.size, fields=False, info=filled_info(n))
    every = svo.distance_boxes(lo, shape.size, fields=filled_fields(n, wide), info=filled_info(n), field_stride=wide)
    fresh = svo.distance_boxes(lo, shape.size)
    one = svo.distance_boxes(lo[7:8], shape.size, fields=filled_fields(1, shape.bytes), info=filled_info(1))
    none = svo.distance_boxes(lo[:0], shape.size, fields=filled_fields(0, shape.bytes), info=filled_info(0))
    svo.sync()
    assert f_only[1] is None and i_only[0] is None
    check_device(f_only[0], None, n, shape.bytes, expected, "fields only")
    check_device(None, i_only[1], n, shape.bytes, expected, "records only")
    check_device(*every, n, wide, expected, "a stride larger than the field")
    check_device(*one, 1, shape.bytes, tuple(a[7:8] for a in expected), "one box")
    check_device(*none, 0, shape.bytes, tuple(a[:0] for a in expected), "no box")
    assert fresh[0].dtype == torch.int16 and tuple(fresh[0].shape) == (n, shape.entries) and tuple(fresh[1].shape) == (n, 4)
    assert differing((hip.distance_fields_to_numpy(fresh[0]), hip.distance_infos_to_numpy(fresh[1])), expected) is None
    # host memory
    hf, hi = svo.distance_boxes(view, shape.size, info=False)
    assert hi is None and (hf == expected[0]).all()
    hf, hi = svo.distance_boxes(view, shape.size, fields=False)
    assert hf is None and hi.tobytes() == expected[1].tobytes()
    out = np.full((n, wide // 2), 0x5A5A, dtype=np.uint16)
    hf, hi = svo.distance_boxes(view, shape.size, fields=out, field_stride=wide)
    assert hf is out and (out[:, shape.entries:] == 0x5A5A).all() and differing((out[:, :shape.entries], hi), expected) is None
    assert differing(svo.distance_boxes(view[7:8], shape.size), tuple(a[7:8] for a in expected)) is None
    hf, hi = svo.distance_boxes(view[:0], shape.size)
    assert hf.shape == (0, shape.entries) and hi.shape == (0,)


@pytest.mark.parametrize("stride", [16, 64])
def test_lo_gathered_in_place(case, stride):
    """lo read in place from a torch tensor of larger records, through a stride of 16 and of 64 bytes."""
    import torch

    boxes = gpu_boxes(case, SEVENTEEN)
    n = len(boxes)
    records = torch.full((n, stride // 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    records[:, :3] = torch.from_numpy(np.ascontiguousarray(boxes)).cuda()
    lo = records[:, :3]
    assert lo.stride(0) == stride // 4 and lo.data_ptr() == records.data_ptr()
    f, i = case.svo.distance_boxes(lo, SEVENTEEN.size, fields=filled_fields(n, SEVENTEEN.bytes), info=filled_info(n))
    case.svo.sync()
    check_device(f, i, n, SEVENTEEN.bytes, case.expected["17-solid"], f"stride {stride}")
    assert (records[:, 3:].cpu().numpy() == 0x5A5A5A5A).all()


@pytest.mark.parametrize("fmt", ["esvo", "csvo"])
def test_the_named_blocks(fmt):
    """`rubble`, each box in its own shape, as numpy has it (tests/test_distance_on_host.py says what each catches): rock all through and its
    complement; the world's last cell in the corner of a 32^3 box of nothing, 2,883 from the opposite corner; a box wholly outside; a target
    only in the last plane and only in the last row; two blocks and a tie; depth inside the chunk's wall; an id that is absent."""
    c = the_case("rubble", fmt)
    at = np.array((4, 4, 4)) + RUBBLE_AT
    asks = [(SOLID_ROCK, (32, 32, 32), 0, 0, 0), (SOLID_ROCK, (32, 32, 32), 0, 0, TO_AIR), ((127, 127, 127), (32, 32, 32), 0, 0, 0), ((128, 40, 40), (32, 32, 32), 0, 0, 0),
            ((-40, 3, 3), (32, 1, 5), 0, 0, 0), (at, (3, 3, 3), 0, 0, 0), (at - (0, 0, 2), (3, 3, 3), 0, 0, 0), (at - (0, 2, 0), (3, 3, 1), 0, 0, 0),
            (np.array((20, 10, 23)) + RUBBLE_AT, (5, 3, 3), 0, 0, 0), ((RUBBLE_AT, RUBBLE_AT + 16, RUBBLE_AT + 16), (8, 4, 4), 0, 0, TO_AIR),
            ((RUBBLE_AT + 6, RUBBLE_AT + 15, RUBBLE_AT + 6), (17, 17, 17), 0, 9, 0), ((RUBBLE_AT + 6, RUBBLE_AT + 15, RUBBLE_AT + 6), (17, 17, 17), 9, 0, 0),
            (SOLID_ROCK, (1, 32, 32), 0, ABSENT, 0), (SOLID_ROCK, (1, 32, 32), 0, ROCK, 0)]
    queued = []
    for lo, size, pass_value, match_value, flags in asks:
        dev = torch_boxes(in_form(np.array([lo], dtype=np.int32), 12)[0], 12, 1)
        nbytes = (2 * size[0] * size[1] * size[2] + 15) // 16 * 16
        queued.append((dev, nbytes, c.svo.distance_boxes(dev, size, pass_value, match_value, flags, fields=filled_fields(1, nbytes), info=filled_info(1))))
    c.svo.sync()
    records = []
    for (lo, size, pass_value, match_value, flags), (_, nbytes, (f, i)) in zip(asks, queued):
        expected = distance_truth(c, np.array([lo]), size, pass_value, match_value, flags)
        check_device(f, i, 1, nbytes, expected, f"{size} at {lo}, pass {pass_value}, match {match_value}, flags {flags}")
        records.append(tuple(int(v) for v in expected[1][0]))
    assert records[0] == (32768, 0, 0, 63) and records[1] == (0, NONE, 0, 0)
    assert records[2] == (1, 2883, 31 | 31 << 8 | 31 << 16, 1 | 4 | 16) and records[3] == (0, NONE, 0, 0) and records[4] == (0, NONE, 0, 0)
    assert records[5] == (1, 12, 2 | 2 << 8 | 2 << 16, 21) and records[6][:3] == (1, 12, 2 | 2 << 8) and records[7][:3] == (1, 8, 2)
    assert records[8][0] == 2 and records[9][:3] == (96, 4, 0) and records[10][0] == 1 and records[12] == (0, NONE, 0, 0) and records[13][0] == 1024


def test_behind_an_earlier_batch_call(case):
    """A label call and a distance call of the same boxes queued on the context's stream with nothing between them, then one vx_sync: both as
    the harness and numpy have them."""
    from label_cases import label_truth

    boxes = gpu_boxes(case, SEVENTEEN)
    n = len(boxes)
    lo = torch_boxes(in_form(boxes, 12)[0], 12, n)
    _, _, label_info = case.svo.label_boxes(lo, SEVENTEEN.size, fields=False, pieces=False)
    f, i = case.svo.distance_boxes(lo, SEVENTEEN.size, fields=filled_fields(n, SEVENTEEN.bytes), info=filled_info(n))
    again = case.svo.distance_boxes(lo, SEVENTEEN.size, flags=TO_AIR, fields=filled_fields(n, SEVENTEEN.bytes), info=filled_info(n))
    case.svo.sync()
    check_device(f, i, n, SEVENTEEN.bytes, case.expected["17-solid"], "behind a label call")
    check_device(*again, n, SEVENTEEN.bytes, case.expected["17-air"], "behind a distance call")
    assert hip.label_infos_to_numpy(label_info).tobytes() == label_truth(case, boxes, SEVENTEEN.size)[2].tobytes()
    assert (hip.label_infos_to_numpy(label_info)["solid"] == case.expected["17-solid"][1]["targets"]).all()


@pytest.mark.parametrize("fmt", ["esvo", "csvo"])
def test_a_commit_changes_the_field(fmt):
    """`rubble`: a call into device memory; one block put into the hollow and committed; the call again; one vx_sync. Each buffer shows the
    world of its moment exactly as numpy has it (a commit's uploads wait for the event mark_world_read records behind the launch), and the
    two differ."""
    c = make_distance_case("rubble", fmt)
    svo = make_context(c)
    try:
        lo = (np.array([(2, 12, 2), (10, 10, 10)]) + RUBBLE_AT).astype(np.int32)
        dev = torch_boxes(in_form(lo, 12)[0], 12, len(lo))
        b = rubble_blocks()
        assert b[6, 16, 6] == 0
        n, shape = len(lo), SHAPE["9_two_bricks"]
        ask = lambda: svo.distance_boxes(dev, shape.size, fields=filled_fields(n, shape.bytes), info=filled_info(n))
        worlds, calls = [b.copy()], [ask()]
        b[6, 16, 6] = ROCK
        c.world.set_chunk((1, 1, 1), _chunk_of((1, 1, 1), 5, b))
        c.world.serialize()
        svo.update_full(c.world)  # vx_commit_all
        worlds.append(b.copy())
        calls.append(ask())
        svo.sync()
        truths = []
        for w in worlds:
            blocks = c.truth.copy()
            blocks[:32, :32, :32] = w
            truths.append(distance_truth(c, lo, shape, truth=blocks))
        assert truths[0][1]["targets"][0] + 1 == truths[1][1]["targets"][0] and (truths[0][0][0] != truths[1][0][0]).any()
        for k, ((f, i), expected) in enumerate(zip(calls, truths)):
            check_device(f, i, n, shape.bytes, expected, f"after {k} commits")
    finally:
        svo.close()


def test_esvo_big():
    """`rubble` in an ESVO context of 4 GiB, which selects the VX_SVO_ESVO_BIG build of the kernel: every call."""
    c = the_case("rubble", "esvo")
    with big_esvo_context(c) as svo:
        queued = [asked(c, call, svo) for call in c.calls]
        svo.sync()
        for call, (lo, f, i, stride) in zip(c.calls, queued):
            check_device(f, i, len(lo), stride, c.expected[call[0]], call[0])


def test_errors_leave_the_output_alone(case):
    """Every invalid argument returns VX_ERR_INVALID_ARGUMENT with the field named and leaves host and device outputs at their sentinels; a
    context without a commit returns VX_ERR_STATE; count == 0 is VX_OK and writes nothing."""
    import torch

    L, h, vp = hip.lib(), case.svo._h, C.c_void_p
    fields = np.full(2 * 8192 + 16, 0x5A, dtype=np.uint8)
    info = np.full(3, SENTINEL, dtype=np.uint32).repeat(4)
    d_fields, d_info = filled_fields(2, 8192), filled_info(2)
    v = np.tile(np.array([3, 3, 3], dtype=np.int32), 8)
    d_v = torch.from_numpy(v).cuda()
    assert d_fields.data_ptr() % 16 == 0 and d_info.data_ptr() % 16 == 0 and v.ctypes.data % 4 == 0

    def shape(**fields_):
        s = hip.distance_shape((16, 16, 16))
        for k, val in fields_.items():
            setattr(s, k, val)
        return s

    u3 = C.c_uint32 * 3
    hb, db = v.ctypes.data, d_v.data_ptr()
    hf, hi = vp(fields.ctypes.data), vp(info.ctypes.data)
    df, di = vp(d_fields.data_ptr()), vp(d_info.data_ptr())
    H, D = hip.VX_MEM_HOST, hip.VX_MEM_DEVICE
    refusals = ((lambda: L.vx_distance_boxes(None, hb, 12, 2, C.byref(shape()), H, hf, 0, hi), b"null context"),
                (lambda: L.vx_distance_boxes(h, hb, 12, 2, C.byref(shape()), 3, hf, 0, hi), b"VX_MEM"),
                (lambda: L.vx_distance_boxes(h, hb, 12, 2, None, H, hf, 0, hi), b"null shape"),
                (lambda: L.vx_distance_boxes(h, None, 12, 2, C.byref(shape()), H, hf, 0, hi), b"null lo"),
                (lambda: L.vx_distance_boxes(h, hb, 12, 2, C.byref(shape()), H, None, 0, None), b"fields and info are both null"),
                (lambda: L.vx_distance_boxes(h, hb, 8, 2, C.byref(shape()), H, hf, 0, hi), b"lo_stride"),
                (lambda: L.vx_distance_boxes(h, hb + 2, 12, 2, C.byref(shape()), H, hf, 0, hi), b"lo must be aligned"),
                (lambda: L.vx_distance_boxes(h, hb, 12, 2, C.byref(shape(size=u3(16, 0, 16))), H, hf, 0, hi), b"size"),
                (lambda: L.vx_distance_boxes(h, hb, 12, 2, C.byref(shape(size=u3(16, 16, 33))), H, hf, 0, hi), b"size"),
                (lambda: L.vx_distance_boxes(h, db, 12, 2, C.byref(shape(size=u3(33, 16, 16))), D, df, 0, di), b"size"),
                (lambda: L.vx_distance_boxes(h, hb, 12, 2, C.byref(shape(flags=2)), H, hf, 0, hi), b"flags"),
                (lambda: L.vx_distance_boxes(h, db, 12, 2, C.byref(shape(flags=3)), D, df, 0, di), b"flags"),
                (lambda: L.vx_distance_boxes(h, hb, 12, 2, C.byref(shape(pass_value=9, match_value=3)), H, hf, 0, hi), b"pass_value must be 0"),
                (lambda: L.vx_distance_boxes(h, db, 12, 2, C.byref(shape(pass_value=9, match_value=3)), D, df, 0, di), b"pass_value must be 0"),
                (lambda: L.vx_distance_boxes(h, hb, 12, 2, C.byref(shape()), H, hf, 8176, hi), b"field_stride"),
                (lambda: L.vx_distance_boxes(h, hb, 12, 2, C.byref(shape()), H, hf, 8200, hi), b"field_stride"),
                (lambda: L.vx_distance_boxes(h, db, 12, 2, C.byref(shape()), D, df, 4096, di), b"field_stride"),
                (lambda: L.vx_distance_boxes(h, hb, 12, (1 << 20) + 1, C.byref(shape()), H, None, 0, hi), b"count exceeds"),
                (lambda: L.vx_distance_boxes(h, hb, 12, 2049, C.byref(shape()), H, hf, 0, None), b"count * field_stride"),
                (lambda: L.vx_distance_boxes(h, hb, 12, 2, C.byref(shape()), H, hf, 0, vp(fields.ctypes.data + 8192)), b"fields overlaps info"),
                (lambda: L.vx_distance_boxes(h, db, 12, 2, C.byref(shape()), D, df, 0, vp(d_fields.data_ptr() + 64)), b"fields overlaps info"),
                (lambda: L.vx_distance_boxes(h, db, 12, 2, C.byref(shape()), D, None, 0, vp(db)), b"info overlaps lo"),
                (lambda: L.vx_distance_boxes(h, db, 12, 2, C.byref(shape()), D, vp(d_fields.data_ptr() + 8), 0, di), b"fields in device memory"),
                (lambda: L.vx_distance_boxes(h, db, 12, 2, C.byref(shape()), D, df, 0, vp(d_info.data_ptr() + 4)), b"info in device memory"),
                (lambda: L.vx_distance_boxes(h, db + 1, 12, 2, C.byref(shape()), D, df, 0, di), b"lo must be aligned"))
    uncommitted = (lambda ctx: L.vx_distance_boxes(ctx, hb, 12, 2, C.byref(shape()), H, hf, 0, hi), lambda ctx: L.vx_distance_boxes(ctx, db, 12, 2, C.byref(shape()), D, df, 0, di))
    # count == 0: VX_OK whatever the rest is; nothing is read or written
    nothing_to_do = (lambda: L.vx_distance_boxes(h, hb, 12, 0, C.byref(shape()), H, hf, 0, hi),
                     lambda: L.vx_distance_boxes(h, None, 0, 0, None, H, None, 0, None),
                     lambda: L.vx_distance_boxes(h, db, 12, 0, C.byref(shape(flags=7)), D, df, 0, di))
    leaves_the_outputs_alone(case, [fields, info], [d_fields, d_info], refusals, uncommitted, nothing_to_do)
    # and the call still works: two boxes at (3, 3, 3), as numpy has them
    assert L.vx_distance_boxes(h, hb, 12, 2, C.byref(shape()), H, hf, 0, hi) == 0
    exp_fields, exp_info = distance_truth(case, v[:6].reshape(2, 3), (16, 16, 16))
    assert fields[:2 * 8192].tobytes() == exp_fields.tobytes() and (fields[2 * 8192:] == 0x5A).all()
    assert info[:8].tobytes() == exp_info.tobytes() and (info[8:] == SENTINEL).all()
