"""vx_label_boxes on the GPU (voxel-rs_amd/csrc/blocks/kernels_label.hip): the loose pieces of the blocks in a batch of boxes, against the
host harness's bytes (tests/cpp/label_on_host.cpp: the same header on the host, which tests/test_label_on_host.py holds against numpy over
the dense arrays) and against numpy directly where the world or the boxes change. Five worlds, both formats; every comparison is byte for
byte. A case -- 40 seeded boxes, 14 of the uniform ones and 26 of those around the blocks' surface, and every named one; the calls of
gpu_calls -- is computed once and left unchanged."""
import ctypes as C

import numpy as np
import pytest

from batch_cases import _chunk_of
from gpu_harness import (SENTINEL, big_esvo_context, field_rows, leaves_the_outputs_alone, make_context, records_head, sentinel_bytes, sentinel_words, shared_cases)
from helpers import vra  # noqa: F401
from label_cases import (ALL_FACES, CUT, LABEL_CASES, LINK, MAX_PIECES, ROCK, RUBBLE_AT, RUBBLE_NAMED, SEEDED, SEVENTEEN, SHAPE, SOLID_ROCK, HostLabel, boxes_for,
                         calls_for, differing, harness, in_form, label_truth, make_label_case, rubble_blocks, torch_boxes)
from voxel_rs_amd import hip

pytestmark = pytest.mark.gpu
filled_fields = sentinel_bytes  # (count, stride): the fields at their stride and the tail


def filled_pieces(count, most):
    return sentinel_words(count * most, 4)


def filled_info(count):
    return sentinel_words(count, 8)


def check_device(fields, pieces, info, count, stride, most, expected, what):
    """Buffers longer than the call needs: the fields at their stride with the sentinel between and behind them, the piece records and the
    records and two more of each. None: an output the call was not given."""
    exp_fields, exp_pieces, exp_info = expected
    got_fields, got_pieces, got_info = exp_fields, exp_pieces, exp_info
    if fields is not None:
        got_fields = field_rows(fields, count, stride, exp_fields.shape[1], what)
    if pieces is not None:
        got_pieces = np.ascontiguousarray(records_head(pieces, count * most, what)).view(hip.LABEL_PIECE_DTYPE).reshape(count, most)
    if info is not None:
        got_info = records_head(hip.label_infos_to_numpy(info), count, what)
    assert differing((got_fields, got_pieces, got_info), expected) is None, f"{what}: {differing((got_fields, got_pieces, got_info), expected)}"


def gpu_calls(c):
    """Of label_cases.calls_for: every shape under every anchor_faces (the limits, budgets, pass values and strides in turn), and of the
    sweep at 17^3 the calls that pair each piece limit and each step budget once."""
    keep = {"17-0-4096", "17-4-24", "17-250-0", "17-250-1", "17-250-4096", "17-4-4096-pass", "17-250-24-pass", "17-0-1-pass"}
    return [call for call in calls_for(c) if "0x" in call[0] or call[0] in keep]


def build(name, fmt):
    """The world, a context that has it, the boxes the GPU is asked about and the harness's bytes for every call; shared by the tests."""
    c = make_label_case(name, fmt)
    c.pick = np.concatenate([np.arange(14), np.arange(SEEDED - 26, SEEDED), np.arange(SEEDED, len(c.boxes))])
    c.calls = gpu_calls(c)
    host = HostLabel(harness(), c)
    c.expected = {call[0]: host.call(c, call, c.pick) for call in c.calls}
    host.close()
    c.svo = make_context(c)
    return c


the_case, _contexts, case = shared_cases(build, LABEL_CASES)


def asked(c, call, svo=None):
    """One of the case's calls into device memory, into buffers longer than it needs: (lo, fields, pieces, info)."""
    _, shape, faces, most, steps, pass_value, stride = call
    n = len(c.pick)
    lo = torch_boxes(in_form(boxes_for(c, shape)[c.pick], stride)[0], stride, n)
    got = (svo or c.svo).label_boxes(lo, shape.size, faces, most, steps, pass_value, fields=filled_fields(n, shape.padded), pieces=filled_pieces(n, most) if most else False,
                                     info=filled_info(n))
    return (lo,) + got


def test_device_and_host_memory_give_the_harness_bytes(case):
    """Every call -- every shape, anchor_faces, piece limit, step budget and pass value, the strides in turn --: the device calls queued
    together before one vx_sync, each into buffers longer than it needs; then the same boxes as host-memory calls."""
    svo, n = case.svo, len(case.pick)
    queued = [asked(case, call) for call in case.calls]
    svo.sync()
    for call, (_, f, p, i) in zip(case.calls, queued):
        name, shape, faces, most, steps, pass_value, stride = call
        check_device(f, p, i, n, shape.padded, most, case.expected[name], f"{case.name}-{case.fmt} {name}")
        view = in_form(boxes_for(case, shape)[case.pick], stride)[1]
        hf, hp, hi = svo.label_boxes(view, shape.size, faces, most, steps, pass_value)
        hp = np.zeros((n, 0), dtype=hip.LABEL_PIECE_DTYPE) if hp is None else hp
        assert hi.dtype == hip.LABEL_INFO_DTYPE and differing((hf, hp, hi), case.expected[name]) is None, f"{name} in host memory: {differing((hf, hp, hi), case.expected[name])}"
    if case.name == "rubble":
        info = case.expected["17-250-4096"][2]
        assert (info["pieces"] >= 2).sum() >= 5 and (case.expected["17-4-24"][2]["flags"] & CUT).any()


def test_outputs_and_strides(case):
    """Fields only, pieces only, records only, and a field_stride larger than the box (the bytes beyond the rounded voxel count keep their
    sentinel), in device and in host memory; one box (count = 1); none."""
    svo, shape, most, n = case.svo, SHAPE["31x3x17"], 4, len(case.pick)
    boxes = boxes_for(case, shape)[case.pick]
    expected = label_truth(case, boxes, shape, max_pieces=most)
    raw, view = in_form(boxes, 16)
    lo = torch_boxes(raw, 16, n)
    wide = shape.padded + 32
    f_only = svo.label_boxes(lo, shape.size, max_pieces=most, fields=filled_fields(n, shape.padded), pieces=False, info=False)
    p_only = svo.label_boxes(lo, shape.size, max_pieces=most, fields=False, pieces=filled_pieces(n, most), info=False)
    i_only = svo.label_boxes(lo, shape.size, max_pieces=most, fields=False, pieces=False, info=filled_info(n))
    every = svo.label_boxes(lo, shape.size, max_pieces=most, fields=filled_fields(n, wide), pieces=filled_pieces(n, most), info=filled_info(n), field_stride=wide)
    one = svo.label_boxes(lo[7:8], shape.size, max_pieces=most, fields=filled_fields(1, shape.padded), pieces=filled_pieces(1, most), info=filled_info(1))
    none = svo.label_boxes(lo[:0], shape.size, max_pieces=most, fields=filled_fields(0, shape.padded), pieces=filled_pieces(0, most), info=filled_info(0))
    svo.sync()
    assert f_only[1] is None and f_only[2] is None and p_only[0] is None and p_only[2] is None and i_only[0] is None and i_only[1] is None
    check_device(f_only[0], None, None, n, shape.padded, most, expected, "fields only")
    check_device(None, p_only[1], None, n, shape.padded, most, expected, "pieces only")
    check_device(None, None, i_only[2], n, shape.padded, most, expected, "records only")
    check_device(*every, n, wide, most, expected, "a stride larger than the box")
    check_device(*one, 1, shape.padded, most, tuple(a[7:8] for a in expected), "one box")
    check_device(*none, 0, shape.padded, most, tuple(a[:0] for a in expected), "no box")
    # host memory
    hf, hp, hi = svo.label_boxes(view, shape.size, max_pieces=most, pieces=False, info=False)
    assert hp is None and hi is None and (hf == expected[0]).all()
    hf, hp, hi = svo.label_boxes(view, shape.size, max_pieces=most, fields=False, info=False)
    assert hf is None and hi is None and hp.tobytes() == expected[1].tobytes()
    hf, hp, hi = svo.label_boxes(view, shape.size, max_pieces=most, fields=False, pieces=False)
    assert hf is None and hp is None and hi.tobytes() == expected[2].tobytes()
    out = np.full((n, wide), 0x5A, dtype=np.uint8)
    hf, hp, hi = svo.label_boxes(view, shape.size, max_pieces=most, fields=out, field_stride=wide)
    assert (out[:, :shape.padded] == expected[0]).all() and (out[:, shape.padded:] == 0x5A).all() and differing((out[:, :shape.padded], hp, hi), expected) is None
    assert differing(svo.label_boxes(view[7:8], shape.size, max_pieces=most), tuple(a[7:8] for a in expected)) is None
    hf, hp, hi = svo.label_boxes(view[:0], shape.size, max_pieces=most)
    assert hf.shape == (0, shape.padded) and hp.shape == (0, most) and hi.shape == (0,)


@pytest.mark.parametrize("stride", [16, 64])
def test_lo_gathered_in_place(case, stride):
    """lo read in place from a torch tensor of larger records, through a stride of 16 and of 64 bytes."""
    import torch

    n = len(case.pick)
    call = [c for c in case.calls if c[0] == "17-250-4096"][0]
    records = torch.full((n, stride // 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    records[:, :3] = torch.from_numpy(np.ascontiguousarray(case.boxes[case.pick])).cuda()
    lo = records[:, :3]
    assert lo.stride(0) == stride // 4 and lo.data_ptr() == records.data_ptr()
    f, p, i = case.svo.label_boxes(lo, SEVENTEEN.size, fields=filled_fields(n, SEVENTEEN.padded), pieces=filled_pieces(n, MAX_PIECES), info=filled_info(n))
    case.svo.sync()
    check_device(f, p, i, n, SEVENTEEN.padded, MAX_PIECES, case.expected[call[0]], f"stride {stride}")
    assert (records[:, 3:].cpu().numpy() == 0x5A5A5A5A).all()


@pytest.mark.parametrize("fmt", ["esvo", "csvo"])
def test_the_named_pieces_and_the_budget(fmt):
    """`rubble`'s named boxes, each in its own shape, as numpy has them (tests/test_label_on_host.py says what each catches): the wire of
    268 steps whole and cut one step short, the chunk of solid rock as one piece of 32^3 cells at exactly its depth and cut below it, the
    link of id 9 as rock and as air."""
    c = the_case("rubble", fmt)
    asks = [(np.array(at) + RUBBLE_AT, size, faces, MAX_PIECES, hip.VX_LABEL_MAX_STEPS, pass_value) for at, size, faces, pass_value in RUBBLE_NAMED.values()]
    wire = RUBBLE_NAMED["wire"]
    asks += [(np.array(wire[0]) + RUBBLE_AT, wire[1], ALL_FACES, 4, 267, 0), (np.array(RUBBLE_NAMED["coil"][0]) + RUBBLE_AT, RUBBLE_NAMED["coil"][1], ALL_FACES, 4, 38, 0),
             (np.array(RUBBLE_NAMED["coil"][0]) + RUBBLE_AT, RUBBLE_NAMED["coil"][1], ALL_FACES, 4, 37, 0), (np.array(RUBBLE_NAMED["checkerboard"][0]) + RUBBLE_AT, (8, 8, 8), ALL_FACES, 0, 0, 0),
             (SOLID_ROCK, (32, 32, 32), 0, 1, 93, 0), (SOLID_ROCK, (32, 32, 32), 0, 1, 92, 0), (SOLID_ROCK, (32, 32, 32), 1, 1, 30, 0), (SOLID_ROCK, (32, 32, 32), ALL_FACES, 2, 0, LINK)]
    queued = []
    for lo, size, faces, most, steps, pass_value in asks:
        dev = torch_boxes(in_form(np.array([lo], dtype=np.int32), 12)[0], 12, 1)
        padded = (size[0] * size[1] * size[2] + 15) // 16 * 16
        queued.append((dev, padded, c.svo.label_boxes(dev, size, faces, most, steps, pass_value, fields=filled_fields(1, padded), pieces=filled_pieces(1, most) if most else False,
                                                      info=filled_info(1))))
    c.svo.sync()
    for (lo, size, faces, most, steps, pass_value), (_, padded, (f, p, i)) in zip(asks, queued):
        expected = label_truth(c, np.array([lo]), size, faces, most, steps, pass_value)
        check_device(f, p, i, 1, padded, most, expected, f"{size} at {lo}, faces {faces:#x}, {most} pieces, {steps} steps")
    rock = label_truth(c, np.array([SOLID_ROCK]), (32, 32, 32), 0, 1, 93)
    assert tuple(rock[2][0]) == (32768, 0, 1, 32768, 0, 93, 63, 0) and tuple(label_truth(c, np.array([SOLID_ROCK]), (32, 32, 32), 0, 1, 92)[2][0])[2:6] == (0, 0, 32768, 92)


@pytest.mark.parametrize("fmt", ["esvo", "csvo"])
def test_4096_boxes_records_only(fmt):
    """One records-only call of 4,096 boxes -- more workgroups than the device holds at once --: the case's boxes at 17^3 over and over, every
    record and piece record the harness's."""
    c = the_case("rubble", fmt)
    _, pieces, info = c.expected["17-4-24"]
    n, most = len(c.pick), 4
    times = -(-4096 // n)
    boxes = np.tile(boxes_for(c, SEVENTEEN)[c.pick], (times, 1))[:4096]
    lo = torch_boxes(in_form(boxes, 12)[0], 12, 4096)
    f, p, i = c.svo.label_boxes(lo, SEVENTEEN.size, ALL_FACES, most, 24, 0, fields=False, pieces=filled_pieces(4096, most), info=filled_info(4096))
    c.svo.sync()
    assert f is None
    expected = (np.zeros((4096, 0), dtype=np.uint8), np.tile(pieces, (times, 1))[:4096], np.tile(info, times)[:4096])
    check_device(None, p, i, 4096, 0, most, expected, "4,096 boxes")


@pytest.mark.parametrize("fmt", ["esvo", "csvo"])
def test_commits_change_the_pieces(fmt):
    """`rubble`: a call into device memory; the link the blob hangs by removed and committed; the call again; a block put between the two
    blocks that touched along an edge and committed; the call again; one vx_sync. Each buffer shows the world of its moment exactly as numpy
    has it (a commit's uploads wait for the event mark_world_read records behind the launch), and the three differ."""
    c = make_label_case("rubble", fmt)
    svo = make_context(c)
    try:
        lo = (np.array([RUBBLE_NAMED["blob_held"][0], (6, 0, 0)]) + RUBBLE_AT).astype(np.int32)
        dev = torch_boxes(in_form(lo, 12)[0], 12, len(lo))
        b = rubble_blocks()
        assert b[14, 29, 14] == LINK and b[12, 4, 4] == 0
        n, shape = len(lo), SEVENTEEN
        ask = lambda: svo.label_boxes(dev, shape.size, fields=filled_fields(n, shape.padded), pieces=filled_pieces(n, MAX_PIECES), info=filled_info(n))
        worlds, calls = [b.copy()], [ask()]
        for x, y, z, value in ((14, 29, 14, 0), (12, 4, 4, ROCK)):
            b[x, y, z] = value
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
            truths.append(label_truth(c, lo, shape, truth=blocks))
        assert truths[0][2]["pieces"][0] + 1 == truths[1][2]["pieces"][0] and truths[1][2]["pieces"][1] == truths[2][2]["pieces"][1] + 1
        for k, ((f, p, i), expected) in enumerate(zip(calls, truths)):
            check_device(f, p, i, n, shape.padded, MAX_PIECES, expected, f"after {k} commits")
    finally:
        svo.close()


def test_esvo_big():
    """`rubble` in an ESVO context of 4 GiB, which selects the VX_SVO_ESVO_BIG build of the kernel: every call."""
    c = the_case("rubble", "esvo")
    with big_esvo_context(c) as svo:
        n = len(c.pick)
        queued = [asked(c, call, svo) for call in c.calls]
        svo.sync()
        for call, (_, f, p, i) in zip(c.calls, queued):
            check_device(f, p, i, n, call[1].padded, call[3], c.expected[call[0]], call[0])


def test_errors_leave_the_output_alone(case):
    """Every invalid argument returns VX_ERR_INVALID_ARGUMENT with the field named and leaves host and device outputs at their sentinels; a
    context without a commit returns VX_ERR_STATE; count == 0 is VX_OK and writes nothing."""
    import torch

    L, h, vp = hip.lib(), case.svo._h, C.c_void_p
    fields = np.full(2 * 4096 + 16, 0x5A, dtype=np.uint8)
    pieces = np.full(2 * 4 + 1, SENTINEL, dtype=np.uint32).repeat(4)
    info = np.full(3, SENTINEL, dtype=np.uint32).repeat(8)
    d_fields, d_pieces, d_info = filled_fields(2, 4096), filled_pieces(2, 4), filled_info(2)
    v = np.tile(np.array([3, 3, 3], dtype=np.int32), 8)
    d_v = torch.from_numpy(v).cuda()
    assert d_fields.data_ptr() % 16 == 0 and d_pieces.data_ptr() % 16 == 0 and d_info.data_ptr() % 16 == 0 and v.ctypes.data % 4 == 0

    def shape(**fields_):
        s = hip.label_shape((16, 16, 16), max_pieces=4)
        for k, val in fields_.items():
            setattr(s, k, val)
        return s

    u3 = C.c_uint32 * 3
    hb, db = v.ctypes.data, d_v.data_ptr()
    hf, hp, hi = vp(fields.ctypes.data), vp(pieces.ctypes.data), vp(info.ctypes.data)
    df, dp, di = vp(d_fields.data_ptr()), vp(d_pieces.data_ptr()), vp(d_info.data_ptr())
    H, D = hip.VX_MEM_HOST, hip.VX_MEM_DEVICE
    refusals = ((lambda: L.vx_label_boxes(None, hb, 12, 2, C.byref(shape()), H, hf, 0, hp, hi), b"null context"),
                (lambda: L.vx_label_boxes(h, hb, 12, 2, C.byref(shape()), 3, hf, 0, hp, hi), b"VX_MEM"),
                (lambda: L.vx_label_boxes(h, hb, 12, 2, None, H, hf, 0, hp, hi), b"null shape"),
                (lambda: L.vx_label_boxes(h, None, 12, 2, C.byref(shape()), H, hf, 0, hp, hi), b"null lo"),
                (lambda: L.vx_label_boxes(h, hb, 12, 2, C.byref(shape()), H, None, 0, None, None), b"fields, pieces and info"),
                (lambda: L.vx_label_boxes(h, hb, 8, 2, C.byref(shape()), H, hf, 0, hp, hi), b"lo_stride"),
                (lambda: L.vx_label_boxes(h, hb + 2, 12, 2, C.byref(shape()), H, hf, 0, hp, hi), b"lo must be aligned"),
                (lambda: L.vx_label_boxes(h, hb, 12, 2, C.byref(shape(size=u3(16, 0, 16))), H, hf, 0, hp, hi), b"size"),
                (lambda: L.vx_label_boxes(h, hb, 12, 2, C.byref(shape(size=u3(16, 16, 33))), H, hf, 0, hp, hi), b"size"),
                (lambda: L.vx_label_boxes(h, hb, 12, 2, C.byref(shape(anchor_faces=0x40)), H, hf, 0, hp, hi), b"anchor_faces"),
                (lambda: L.vx_label_boxes(h, hb, 12, 2, C.byref(shape(max_pieces=251)), H, hf, 0, hp, hi), b"max_pieces"),
                (lambda: L.vx_label_boxes(h, hb, 12, 2, C.byref(shape(max_pieces=0)), H, hf, 0, hp, hi), b"pieces with max_pieces == 0"),
                (lambda: L.vx_label_boxes(h, db, 12, 2, C.byref(shape(max_pieces=0)), D, df, 0, dp, di), b"pieces with max_pieces == 0"),
                (lambda: L.vx_label_boxes(h, hb, 12, 2, C.byref(shape(max_steps=4097)), H, hf, 0, hp, hi), b"max_steps"),
                (lambda: L.vx_label_boxes(h, db, 12, 2, C.byref(shape(max_steps=4097)), D, df, 0, dp, di), b"max_steps"),
                (lambda: L.vx_label_boxes(h, hb, 12, 2, C.byref(shape(flags=1)), H, hf, 0, hp, hi), b"flags"),
                (lambda: L.vx_label_boxes(h, hb, 12, 2, C.byref(shape()), H, hf, 4080, hp, hi), b"field_stride"),
                (lambda: L.vx_label_boxes(h, hb, 12, 2, C.byref(shape()), H, hf, 4104, hp, hi), b"field_stride"),
                (lambda: L.vx_label_boxes(h, hb, 12, (1 << 20) + 1, C.byref(shape()), H, None, 0, None, hi), b"count exceeds"),
                (lambda: L.vx_label_boxes(h, hb, 12, 4097, C.byref(shape()), H, hf, 0, None, hi), b"count * field_stride"),
                (lambda: L.vx_label_boxes(h, hb, 12, 2, C.byref(shape()), H, hf, 0, vp(fields.ctypes.data + 4096), hi), b"fields overlaps pieces"),
                (lambda: L.vx_label_boxes(h, db, 12, 2, C.byref(shape()), D, df, 0, dp, vp(d_pieces.data_ptr() + 64)), b"pieces overlaps info"),
                (lambda: L.vx_label_boxes(h, db, 12, 2, C.byref(shape()), D, vp(d_fields.data_ptr() + 8), 0, dp, di), b"fields in device memory"),
                (lambda: L.vx_label_boxes(h, db, 12, 2, C.byref(shape()), D, df, 0, vp(d_pieces.data_ptr() + 8), di), b"pieces in device memory"),
                (lambda: L.vx_label_boxes(h, db, 12, 2, C.byref(shape()), D, df, 0, dp, vp(d_info.data_ptr() + 4)), b"info in device memory"),
                (lambda: L.vx_label_boxes(h, db + 1, 12, 2, C.byref(shape()), D, df, 0, dp, di), b"lo must be aligned"))
    uncommitted = (lambda ctx: L.vx_label_boxes(ctx, hb, 12, 2, C.byref(shape()), H, hf, 0, hp, hi), lambda ctx: L.vx_label_boxes(ctx, db, 12, 2, C.byref(shape()), D, df, 0, dp, di))
    # count == 0: VX_OK whatever the rest is; nothing is read or written
    nothing_to_do = (lambda: L.vx_label_boxes(h, hb, 12, 0, C.byref(shape()), H, hf, 0, hp, hi),
                     lambda: L.vx_label_boxes(h, None, 0, 0, None, H, None, 0, None, None),
                     lambda: L.vx_label_boxes(h, db, 12, 0, C.byref(shape(flags=7)), D, df, 0, dp, di))
    leaves_the_outputs_alone(case, [fields, pieces, info], [d_fields, d_pieces, d_info], refusals, uncommitted, nothing_to_do)
    # and the call still works: two boxes at (3, 3, 3), as numpy has them
    assert L.vx_label_boxes(h, hb, 12, 2, C.byref(shape()), H, hf, 0, hp, hi) == 0
    exp_fields, exp_pieces, exp_info = label_truth(case, v[:6].reshape(2, 3), (16, 16, 16), max_pieces=4)
    assert fields[:2 * 4096].tobytes() == exp_fields.tobytes() and (fields[2 * 4096:] == 0x5A).all()
    assert pieces[:32].tobytes() == exp_pieces.tobytes() and (pieces[32:] == SENTINEL).all()
    assert info[:16].tobytes() == exp_info.tobytes() and (info[16:] == SENTINEL).all()
