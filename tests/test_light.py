"""vx_light_boxes on the GPU (voxel-rs_amd/csrc/blocks/kernels_light.hip): sky and block light levels for a batch of boxes, against the host
harness's bytes (tests/cpp/light_on_host.cpp: the same header on the host, which tests/test_light_on_host.py holds against numpy over the
dense arrays) and against numpy directly where the world or the boxes change. Five worlds, both formats; every comparison is byte for byte. A
case -- the first 40 seeded boxes and every named one, every call of light_cases.calls_for -- is computed once and left unchanged."""
import ctypes as C

import numpy as np
import pytest

from batch_cases import _chunk_of
from gpu_harness import (SENTINEL, big_esvo_context, field_rows, leaves_the_outputs_alone, make_context, records_head, sentinel_bytes, sentinel_words, shared_cases)
from helpers import vra  # noqa: F401
from light_cases import (LIGHT_CASES, NO_BLOCKS, NO_SKY, ROCK, SEEDED, SHAPE, SIXTEEN, HostLight, boxes_for, calls_for, differing, harness, in_form, lantern_blocks,
                         light_truth, make_light_case, torch_boxes)
from voxel_rs_amd import hip

pytestmark = pytest.mark.gpu
filled_fields = sentinel_bytes  # (count, stride): the fields at their stride and the tail


def filled_info(count):
    return sentinel_words(count, 4)


def check_device(fields, info, count, stride, exp_fields, exp_info, what):
    """Buffers longer than the call needs: the fields at their stride with the sentinel between and behind them, the records and two more.
    info None: a call that was given no records."""
    got_fields = field_rows(fields, count, stride, exp_fields.shape[1], what)
    got_info = exp_info if info is None else records_head(hip.light_infos_to_numpy(info), count, what)
    assert differing(got_fields, got_info, exp_fields, exp_info) is None, f"{what}: {differing(got_fields, got_info, exp_fields, exp_info)}"


def build(name, fmt):
    """The world, a context that has it, the boxes the GPU is asked about and the harness's bytes for every call; shared by the tests."""
    c = make_light_case(name, fmt)
    c.pick = np.concatenate([np.arange(40), np.arange(SEEDED, len(c.boxes))])
    c.calls = calls_for(c)
    host = HostLight(harness(), c)
    c.expected = {call[0]: host.call(c, call, c.pick) for call in c.calls}
    host.close()
    c.svo = make_context(c)
    return c


the_case, _contexts, case = shared_cases(build, LIGHT_CASES)


def test_device_and_host_memory_give_the_harness_bytes(case):
    """Every call -- every shape, no props, a table cut short, each flag, the strides in turn --: the device calls queued together before one
    vx_sync, each into buffers longer than it needs; then the same boxes as host-memory calls."""
    svo, n = case.svo, len(case.pick)
    queued = []
    for name, shape, props, flags, stride in case.calls:
        raw, view = in_form(boxes_for(case, shape)[case.pick], stride)
        lo = torch_boxes(raw, stride, n)
        table = props.copy()
        f, i = svo.light_boxes(lo, shape.size, table, flags, fields=filled_fields(n, shape.padded), info=filled_info(n))
        table[:] = 0xE0  # (the call has returned: the table is the caller's again)
        queued.append((lo, view, f, i))
    svo.sync()
    for (name, shape, props, flags, stride), (_, view, f, i) in zip(case.calls, queued):
        exp_fields, exp_info = case.expected[name]
        check_device(f, i, n, shape.padded, exp_fields, exp_info, f"{case.name}-{case.fmt} {name}")
        hf, hi = svo.light_boxes(view, shape.size, props, flags)
        assert hi.dtype == hip.LIGHT_INFO_DTYPE and differing(hf, hi, exp_fields, exp_info) is None, f"{name} in host memory: {differing(hf, hi, exp_fields, exp_info)}"
    full = case.expected["16"][1]
    assert (full["lit"] > 0).sum() >= 20


def test_outputs_and_strides(case):
    """Fields only, records only, and a field_stride larger than the box (the bytes beyond the rounded voxel count keep their sentinel), in
    device and in host memory; one box; none."""
    svo, shape, n = case.svo, SHAPE["33x9x17"], len(case.pick)
    _, _, props, flags, stride = [c for c in case.calls if c[0] == "33x9x17"][0]
    exp_fields, exp_info = case.expected["33x9x17"]
    raw, view = in_form(boxes_for(case, shape)[case.pick], stride)
    lo = torch_boxes(raw, stride, n)
    wide = shape.padded + 32
    f_only = svo.light_boxes(lo, shape.size, props, fields=filled_fields(n, shape.padded), info=False)
    i_only = svo.light_boxes(lo, shape.size, props, fields=False, info=filled_info(n))
    both = svo.light_boxes(lo, shape.size, props, fields=filled_fields(n, wide), info=filled_info(n), field_stride=wide)
    one = svo.light_boxes(lo[7:8], shape.size, props, fields=filled_fields(1, shape.padded), info=filled_info(1))
    none = svo.light_boxes(lo[:0], shape.size, props, fields=filled_fields(0, shape.padded), info=filled_info(0))
    svo.sync()
    assert f_only[1] is None and i_only[0] is None
    check_device(f_only[0], None, n, shape.padded, exp_fields, exp_info, "fields only")
    assert records_head(hip.light_infos_to_numpy(i_only[1]), n, "records only").tobytes() == exp_info.tobytes()
    check_device(both[0], both[1], n, wide, exp_fields, exp_info, "a stride larger than the box")
    check_device(one[0], one[1], 1, shape.padded, exp_fields[7:8], exp_info[7:8], "one box")
    check_device(none[0], none[1], 0, shape.padded, exp_fields[:0], exp_info[:0], "no box")
    # host memory
    hf, hi = svo.light_boxes(view, shape.size, props, info=False)
    assert hi is None and (hf == exp_fields).all()
    hf, hi = svo.light_boxes(view, shape.size, props, fields=False)
    assert hf is None and hi.tobytes() == exp_info.tobytes()
    out = np.full((n, wide), 0x5A, dtype=np.uint8)
    hf, hi = svo.light_boxes(view, shape.size, props, fields=out, field_stride=wide)
    assert (out[:, :shape.padded] == exp_fields).all() and (out[:, shape.padded:] == 0x5A).all() and hi.tobytes() == exp_info.tobytes()
    hf, hi = svo.light_boxes(view[7:8], shape.size, props)
    assert (hf == exp_fields[7:8]).all() and hi.tobytes() == exp_info[7:8].tobytes()
    hf, hi = svo.light_boxes(view[:0], shape.size, props)
    assert hf.shape == (0, shape.padded) and hi.shape == (0,)


@pytest.mark.parametrize("stride", [16, 64])
def test_lo_gathered_in_place(case, stride):
    """lo read in place from a torch tensor of larger records, through a stride of 16 and of 64 bytes: the 16^3 boxes as they are."""
    import torch

    n = len(case.pick)
    exp_fields, exp_info = case.expected["16"]
    records = torch.full((n, stride // 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    records[:, :3] = torch.from_numpy(np.ascontiguousarray(case.boxes[case.pick])).cuda()
    lo = records[:, :3]
    assert lo.stride(0) == stride // 4 and lo.data_ptr() == records.data_ptr()
    f, i = case.svo.light_boxes(lo, SIXTEEN.size, case.props, fields=filled_fields(n, SIXTEEN.padded), info=filled_info(n))
    case.svo.sync()
    check_device(f, i, n, SIXTEEN.padded, exp_fields, exp_info, f"stride {stride}")
    assert (records[:, 3:].cpu().numpy() == 0x5A5A5A5A).all()


@pytest.mark.parametrize("fmt", ["esvo", "csvo"])
def test_512_copies_of_one_box(fmt):
    """512 workgroups on one box of 48^3, more than the device has compute units: every field and record is the first one's, the harness's."""
    import torch

    c = the_case("lantern", fmt)
    shape = SHAPE["48"]
    exp_fields, exp_info = c.expected["48"]
    k = int(np.argmax(exp_info["lit"] * (exp_info["sources"] > 0)))
    lo = torch.from_numpy(np.tile(boxes_for(c, shape)[c.pick][k], (512, 1))).cuda()
    f, i = c.svo.light_boxes(lo, shape.size, c.props, fields=False, info=filled_info(512))
    f2, _ = c.svo.light_boxes(lo[:100], shape.size, c.props, fields=filled_fields(100, shape.padded), info=False)
    c.svo.sync()
    assert hip.light_infos_to_numpy(i)[:512].tobytes() == np.tile(exp_info[k:k + 1], 512).tobytes()
    check_device(f2, None, 100, shape.padded, np.tile(exp_fields[k], (100, 1)), np.tile(exp_info[k:k + 1], 100), "100 copies")


@pytest.mark.parametrize("fmt", ["esvo", "csvo"])
def test_commits_change_the_light(fmt):
    """`lantern`: a call into device memory; the roof block over (12, 20, 12) removed and committed; the call again; a lamp added at
    (12, 3, 16) and committed; the call again; one vx_sync. Each buffer shows the world of its moment exactly as numpy has it (a commit's
    uploads wait for the event mark_world_read records behind the launch), and the three differ."""
    c = make_light_case("lantern", fmt)
    svo = make_context(c)
    try:
        lo = np.array([[4, 4, 4], [2, 2, 6]], dtype=np.int32)
        dev = torch_boxes(in_form(lo, 12)[0], 12, len(lo))
        b = lantern_blocks()
        assert b[12, 20, 12] == ROCK and b[12, 3, 16] == 0
        worlds, calls = [b.copy()], []
        calls.append(svo.light_boxes(dev, SIXTEEN.size, c.props, fields=filled_fields(len(lo), SIXTEEN.padded), info=filled_info(len(lo))))
        for x, y, z, value in ((12, 20, 12, 0), (12, 3, 16, 1)):
            b[x, y, z] = value
            c.world.set_chunk((0, 0, 0), _chunk_of((0, 0, 0), 5, b))
            c.world.serialize()
            svo.update_full(c.world)  # vx_commit_all
            worlds.append(b.copy())
            calls.append(svo.light_boxes(dev, SIXTEEN.size, c.props, fields=filled_fields(len(lo), SIXTEEN.padded), info=filled_info(len(lo))))
        svo.sync()
        truths = [light_truth(c, lo, SIXTEEN.size, c.props, truth=w) for w in worlds]
        assert truths[0][1]["open_columns"][0] + 1 == truths[1][1]["open_columns"][0] and truths[1][1]["sources"][1] + 1 == truths[2][1]["sources"][1]
        assert (truths[0][0] != truths[1][0]).any() and (truths[1][0] != truths[2][0]).any()
        for k, ((f, i), (exp_fields, exp_info)) in enumerate(zip(calls, truths)):
            check_device(f, i, len(lo), SIXTEEN.padded, exp_fields, exp_info, f"after {k} commits")
    finally:
        svo.close()


def test_a_section_with_its_margin_does_not_depend_on_the_box(case):
    """The margin rule of the header: the 16^3 section in the middle of a 46^3 box has the levels of the same cells of the 48^3 box one cell
    larger on every side, which numpy gives."""
    lo = np.asarray(case.boxes[[0, 1, 2, case.names["negative_lo"]]], dtype=np.int64)
    f46, _ = case.svo.light_boxes((lo - 15).astype(np.int32), (46, 46, 46), case.props, info=False)
    t48, _ = light_truth(case, lo - 16, (48, 48, 48), case.props)
    inner46 = f46[:, :46 ** 3].reshape(-1, 46, 46, 46)[:, 15:31, 15:31, 15:31]
    inner48 = t48[:, :48 ** 3].reshape(-1, 48, 48, 48)[:, 16:32, 16:32, 16:32]
    assert (inner46 == inner48).all()
    t46, _ = light_truth(case, lo - 15, (46, 46, 46), case.props)
    assert (f46 == t46).all()


def test_esvo_big():
    """The lantern in an ESVO context of 4 GiB, which selects the VX_SVO_ESVO_BIG build of the kernel: every call."""
    c = the_case("lantern", "esvo")
    with big_esvo_context(c) as svo:
        n, queued = len(c.pick), []
        for name, shape, props, flags, stride in c.calls:
            lo = torch_boxes(in_form(boxes_for(c, shape)[c.pick], stride)[0], stride, n)
            queued.append((lo, svo.light_boxes(lo, shape.size, props, flags, fields=filled_fields(n, shape.padded), info=filled_info(n))))
        svo.sync()
        for (name, shape, *_), (_, (f, i)) in zip(c.calls, queued):
            check_device(f, i, n, shape.padded, *c.expected[name], name)


def test_errors_leave_the_output_alone(case):
    """Every invalid argument returns VX_ERR_INVALID_ARGUMENT with the field named and leaves host and device outputs at their sentinels; a
    context without a commit returns VX_ERR_STATE; count == 0 is VX_OK and writes nothing."""
    import torch

    L, h, vp = hip.lib(), case.svo._h, C.c_void_p
    fields = np.full(2 * 4096 + 16, 0x5A, dtype=np.uint8)
    info = np.full(3, SENTINEL, dtype=np.uint32).repeat(4)
    d_fields, d_info = filled_fields(2, 4096), filled_info(2)
    v = np.tile(np.array([3, 3, 3], dtype=np.int32), 8)
    d_v = torch.from_numpy(v).cuda()
    good = case.props.copy()
    bad = good.copy()
    bad[-1] |= 0x40
    assert d_fields.data_ptr() % 16 == 0 and d_info.data_ptr() % 16 == 0 and v.ctypes.data % 4 == 0

    def shape(table=good, **fields_):
        s, keep = hip.light_shape((16, 16, 16), table)
        s.keep = keep
        for k, val in fields_.items():
            setattr(s, k, val)
        return s

    u3 = C.c_uint32 * 3
    hb, db = v.ctypes.data, d_v.data_ptr()
    hf, hi, df, di = vp(fields.ctypes.data), vp(info.ctypes.data), vp(d_fields.data_ptr()), vp(d_info.data_ptr())
    H, D = hip.VX_MEM_HOST, hip.VX_MEM_DEVICE
    refusals = ((lambda: L.vx_light_boxes(None, hb, 12, 2, C.byref(shape()), H, hf, 0, hi), b"null context"),
                (lambda: L.vx_light_boxes(h, hb, 12, 2, C.byref(shape()), 3, hf, 0, hi), b"VX_MEM"),
                (lambda: L.vx_light_boxes(h, hb, 12, 2, None, H, hf, 0, hi), b"null shape"),
                (lambda: L.vx_light_boxes(h, None, 12, 2, C.byref(shape()), H, hf, 0, hi), b"null lo"),
                (lambda: L.vx_light_boxes(h, hb, 12, 2, C.byref(shape()), H, None, 0, None), b"fields and info"),
                (lambda: L.vx_light_boxes(h, hb, 8, 2, C.byref(shape()), H, hf, 0, hi), b"lo_stride"),
                (lambda: L.vx_light_boxes(h, hb + 2, 12, 2, C.byref(shape()), H, hf, 0, hi), b"lo must be aligned"),
                (lambda: L.vx_light_boxes(h, hb, 12, 2, C.byref(shape(size=u3(16, 0, 16))), H, hf, 0, hi), b"size"),
                (lambda: L.vx_light_boxes(h, hb, 12, 2, C.byref(shape(size=u3(16, 16, 49))), H, hf, 0, hi), b"size"),
                (lambda: L.vx_light_boxes(h, hb, 12, 2, C.byref(shape(flags=4)), H, hf, 0, hi), b"flags"),
                (lambda: L.vx_light_boxes(h, hb, 12, 2, C.byref(shape(flags=NO_SKY | NO_BLOCKS)), H, hf, 0, hi), b"flags"),
                (lambda: L.vx_light_boxes(h, hb, 12, 2, C.byref(shape(props_count=4097)), H, hf, 0, hi), b"props_count"),
                (lambda: L.vx_light_boxes(h, hb, 12, 2, C.byref(shape(props=None)), H, hf, 0, hi), b"null props"),
                (lambda: L.vx_light_boxes(h, hb, 12, 2, C.byref(shape(bad)), H, hf, 0, hi), b"props: a byte"),
                (lambda: L.vx_light_boxes(h, db, 12, 2, C.byref(shape(bad)), D, df, 0, di), b"props: a byte"),
                (lambda: L.vx_light_boxes(h, hb, 12, 2, C.byref(shape()), H, hf, 4080, hi), b"field_stride"),
                (lambda: L.vx_light_boxes(h, hb, 12, 2, C.byref(shape()), H, hf, 4104, hi), b"field_stride"),
                (lambda: L.vx_light_boxes(h, hb, 12, (1 << 24) + 1, C.byref(shape()), H, None, 0, hi), b"count exceeds"),
                (lambda: L.vx_light_boxes(h, hb, 12, 4097, C.byref(shape()), H, hf, 0, hi), b"count * field_stride"),
                (lambda: L.vx_light_boxes(h, db, 12, 2, C.byref(shape()), D, vp(d_fields.data_ptr() + 8), 0, di), b"fields in device memory"),
                (lambda: L.vx_light_boxes(h, db, 12, 2, C.byref(shape()), D, df, 0, vp(d_info.data_ptr() + 4)), b"info in device memory"),
                (lambda: L.vx_light_boxes(h, db + 1, 12, 2, C.byref(shape()), D, df, 0, di), b"lo must be aligned"))
    uncommitted = (lambda ctx: L.vx_light_boxes(ctx, hb, 12, 2, C.byref(shape()), H, hf, 0, hi), lambda ctx: L.vx_light_boxes(ctx, db, 12, 2, C.byref(shape()), D, df, 0, di))
    # count == 0: VX_OK whatever the rest is; nothing is read or written
    nothing_to_do = (lambda: L.vx_light_boxes(h, hb, 12, 0, C.byref(shape()), H, hf, 0, hi),
                     lambda: L.vx_light_boxes(h, None, 0, 0, None, H, None, 0, None),
                     lambda: L.vx_light_boxes(h, db, 12, 0, C.byref(shape(bad)), D, df, 0, di))
    leaves_the_outputs_alone(case, [fields, info], [d_fields, d_info], refusals, uncommitted, nothing_to_do)
    # and the call still works: two boxes at (3, 3, 3), as numpy has them
    assert L.vx_light_boxes(h, hb, 12, 2, C.byref(shape()), H, hf, 0, hi) == 0
    exp_fields, exp_info = light_truth(case, v[:6].reshape(2, 3), (16, 16, 16), good)
    assert fields[:2 * 4096].tobytes() == exp_fields.tobytes() and (fields[2 * 4096:] == 0x5A).all()
    assert info[:8].tobytes() == exp_info.tobytes() and (info[8:] == SENTINEL).all()
