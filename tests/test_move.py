"""vx_move_boxes on the GPU (voxel-rs_amd/csrc/blocks/kernels_move.hip): a batch of float boxes moved through the world and stopped by blocks,
against the host harness's records (tests/cpp/move_on_host.cpp: the same header on the host, which tests/test_move_on_host.py holds against
the dense arrays) and against numpy directly where the world or the boxes change. Three worlds, both formats; every comparison is byte for
byte. A case is computed once and left unchanged."""
import types

import numpy as np
import pytest

from batch_cases import _chunk_of
from boxes_cases import Boxes
from gpu_harness import (above_the_blocks, big_esvo_context, flying_entities, leaves_the_outputs_alone, make_context, no_image_context, records_head, sentinel_words,
                         shared_cases)
from helpers import vra  # noqa: F401
from move_cases import (INVALID, SCAN_CASES, SEEDED, SKIN, YXZ, HostMoves, Moves, calls_for, differing, harness, make_moves, make_scan_case, moves_truth)
from physics_cases import DT
from voxel_rs_amd import hip

pytestmark = pytest.mark.gpu


def filled(count):
    """A device buffer two records longer than a batch of `count`, every byte 0x5a."""
    return sentinel_words(count, 12)


def check_buffer(dev, exp, what):
    """A buffer two records longer than the batch: the records, then the untouched tail."""
    raw = hip.move_hits_to_numpy(dev)
    got = records_head(raw, len(exp), what)
    assert differing(got, exp) is None, f"{what}: {differing(got, exp)}"
    assert len(raw) == len(exp) + 2, what


def shape_of(how):
    return dict(scale=how["scale"], skin=how["skin"], order=how["order"], only_value=how["only_value"])


def build(name, fmt):
    """The world, a context that has it, its boxes and motions in every form and the harness's records of each; shared by the tests of this
    module."""
    c = make_scan_case(name, fmt)
    c.moves = make_moves(c)
    c.calls = calls_for(c, c.moves)
    host = HostMoves(harness(), c)
    c.records = {call: host.records(mv, **how) for call, mv, how in c.calls}
    host.close()
    for a in c.records.values():
        a.setflags(write=False)
    c.svo = make_context(c)
    return c


the_case, _contexts, case = shared_cases(build, SCAN_CASES)


def test_device_and_host_memory_give_the_harness_records(case):
    """Every form of the boxes and of the motion, the orders, the skins and only_value: the device calls queued together before one vx_sync,
    each into a buffer two records longer than the batch; then the same as host-memory calls. The named boxes of extents 64 moving 64 walk the
    largest slab a pass can have."""
    svo = case.svo
    queued = []
    for call, mv, how in case.calls:
        args = mv.torch_args()
        queued.append((args, svo.move_boxes(**args, **shape_of(how), out=filled(len(mv)))))
    svo.sync()
    for (call, mv, how), (_, dev) in zip(case.calls, queued):
        check_buffer(dev, case.records[call], f"{case.name}-{case.fmt} {call}")
        host = svo.move_boxes(**mv.numpy_args(), **shape_of(how))
        assert host.dtype == hip.MOVE_HIT_DTYPE and differing(host, case.records[call]) is None, f"{call} in host memory: {differing(host, case.records[call])}"
    packed = case.records["packed"]
    assert (packed["contacts"][:SEEDED] != 0).mean() >= 0.25 and (packed["contacts"] == INVALID).sum() >= 60
    assert case.records["xyz"].tobytes() != packed.tobytes() != case.records["zyx"].tobytes()
    widest = packed[case.moves.names["widest"]]
    assert widest["contacts"] == 1 << 2 and widest["value"][1] != 0


def test_one_box(case):
    """count == 1, device and host: a box that is stopped, a box that is not, a record that is no box."""
    mv, exp = case.moves, case.records["packed"]
    picks = [int(np.flatnonzero(exp["contacts"][:SEEDED] != 0)[0]), int(np.flatnonzero(exp["contacts"][:SEEDED] == 0)[0]), int(mv.no_box[0])]
    queued = []
    for i in picks:
        one = mv.picked(np.array([i]))
        args = one.torch_args()
        queued.append((one, args, case.svo.move_boxes(**args, out=filled(1))))
    case.svo.sync()
    for i, (one, _, dev) in zip(picks, queued):
        check_buffer(dev, exp[i:i + 1], f"box {i}")
        assert case.svo.move_boxes(**one.numpy_args()).tobytes() == exp[i:i + 1].tobytes(), i


@pytest.mark.parametrize("fmt", ["esvo", "csvo"])
def test_a_grid_beyond_65535_workgroups(fmt):
    """count == 70,001: the seeded set of `glasshouse` tiled; box i's record is the set's record i mod 2,000."""
    c = the_case("glasshouse", fmt)
    idx = np.arange(70001) % SEEDED
    many = c.moves.picked(idx)
    exp = c.records["packed"][idx]
    args = many.torch_args()
    dev = c.svo.move_boxes(**args, out=filled(len(many)))
    c.svo.sync()
    check_buffer(dev, exp, "device")
    assert c.svo.move_boxes(**many.numpy_args()).tobytes() == exp.tobytes()


@pytest.mark.parametrize("fmt", ["esvo", "csvo"])
def test_behind_physics_step(fmt):
    """256 flying entities in device memory stepped 8 times, then vx_move_boxes over the same records in place -- positions, boxes and
    velocities, scale = delta_time -- with no sync between the two calls; after one vx_sync the entities are read back, and the records are
    numpy's for the positions and velocities the steps left."""
    import torch

    c = the_case("glasshouse", fmt)
    rng = np.random.default_rng(91)
    e = flying_entities(256, above_the_blocks(c, 256, rng, 1.3, 1.5), rng)  # 1.3 to 1.5 above their column's highest block
    d = torch.from_numpy(e.view(np.uint8).copy()).cuda()
    c.svo.physics_step(d, DT, 8)
    origin, extents, offset = hip.entity_boxes(d)
    dev = c.svo.move_boxes(origin, extents, hip.entity_velocities(d), offset=offset, scale=float(DT), out=filled(len(e)))  # no sync in between
    c.svo.sync()
    after = d.cpu().numpy().view(hip.ENTITY_DTYPE)
    assert (after["position"][:, 1] < e["position"][:, 1] - 1.0).all()
    how = dict(scale=float(DT), skin=SKIN, order=YXZ, only_value=0)
    as_moves = lambda r: Moves(Boxes(r["position"], r["aabb_offset"], r["aabb_extents"], "packed"), r["velocity"])
    exp, before = moves_truth(c, as_moves(after), **how), moves_truth(c, as_moves(e), **how)
    assert (exp["contacts"] != 0).sum() >= 64 and (exp["contacts"] != INVALID).all() and (exp["origin"] != before["origin"]).any(axis=1).sum() >= 200
    check_buffer(dev, exp, "behind vx_physics_step")
    origin, extents, offset = hip.entity_boxes(after)
    assert c.svo.move_boxes(origin, extents, hip.entity_velocities(after), offset=offset, scale=float(DT)).tobytes() == exp.tobytes()


@pytest.mark.parametrize("fmt", ["esvo", "csvo"])
def test_ordered_between_commits(fmt):
    """A call into device memory, a wall set in the way of one box and the floor removed from under another on the host chunk and committed
    with vx_commit_all, the call again into a second buffer, one vx_sync: the first buffer shows the old world and the second the new one,
    both exactly as numpy has them (the commit's uploads wait for the event mark_world_read records behind the last launch)."""
    c = make_scan_case("glasshouse", fmt)
    svo = make_context(c)
    try:
        seeded = make_moves(c)
        extra = [("walled", (14.25, 16.25, 16.25), (1.0, 1.0, 1.0), (4.0, 0.0, 0.0)), ("floorless", (6.1, 1.5, 24.1), (0.8, 0.8, 0.8), (0.0, -3.0, 0.0))]
        b = seeded.boxes
        boxes = Boxes(np.concatenate([b.origin[:SEEDED], np.array([r[1] for r in extra], dtype=np.float32)]),
                      np.concatenate([b.offset[:SEEDED], np.zeros((len(extra), 3), dtype=np.float32)]),
                      np.concatenate([b.extents[:SEEDED], np.array([r[2] for r in extra], dtype=np.float32)]), "packed")
        mv = Moves(boxes, np.concatenate([seeded.motion[:SEEDED], np.array([r[3] for r in extra], dtype=np.float32)]))
        args = mv.torch_args()
        old = moves_truth(c, mv)
        first = svo.move_boxes(**args, out=filled(len(mv)))  # enqueued; the commit below has to wait for it on the device
        blocks = c.info["blocks"].copy()
        assert blocks[6, 0, 24] != 0 and not blocks[16:19, 16:18, 16:18].any()
        blocks[17, 16:18, 16:18], blocks[6, 0, 24] = 12, 0  # a wall in the air, one block of the floor removed
        c.world.set_chunk((0, 0, 0), _chunk_of((0, 0, 0), 5, blocks))
        c.world.serialize()
        svo.update_full(c.world)  # vx_commit_all
        changed = types.SimpleNamespace(name="glasshouse, changed", fmt=fmt, info=c.info, truth=blocks, size=c.size)  # (no LOD chunk here: the world shows its blocks)
        new = moves_truth(changed, mv)
        second = svo.move_boxes(**args, out=filled(len(mv)))  # enqueued behind the commit's upload
        svo.sync()
        assert old.tobytes() != new.tobytes()
        assert old["moved"][SEEDED][0] == 4 and old["contacts"][SEEDED] == 0 and new["moved"][SEEDED][0] == np.float32(1.75) - np.float32(SKIN)
        assert new["contacts"][SEEDED] == 1 << 1 and new["value"][SEEDED][0] == 12
        assert old["contacts"][SEEDED + 1] == 1 << 2 and old["moved"][SEEDED + 1][1] == -(np.float32(0.5) - np.float32(SKIN))
        assert new["contacts"][SEEDED + 1] == 0 and new["moved"][SEEDED + 1][1] == -3
        check_buffer(first, old, "before the commit")
        check_buffer(second, new, "after the commit")
    finally:
        svo.close()


def test_esvo_big():
    """The glasshouse in an ESVO context of 4 GiB, which selects the VX_SVO_ESVO_BIG build of the kernel: every call."""
    c = the_case("glasshouse", "esvo")
    with big_esvo_context(c) as svo:
        queued = []
        for call, mv, how in c.calls:
            args = mv.torch_args()
            queued.append((args, svo.move_boxes(**args, **shape_of(how), out=filled(len(mv)))))
        svo.sync()
        for (call, mv, how), (_, dev) in zip(c.calls, queued):
            check_buffer(dev, c.records[call], call)
            assert svo.move_boxes(**mv.numpy_args(), **shape_of(how)).tobytes() == c.records[call].tobytes(), call


def test_without_a_traversal_image_the_bytes_are_the_same(case, monkeypatch):
    """A context created with VX_TRAVERSAL_IMAGE=0 (read when a context is created) answers with the same bytes."""
    with no_image_context(case, monkeypatch) as svo:
        for call, mv, how in case.calls:
            assert svo.move_boxes(**mv.numpy_args(), **shape_of(how)).tobytes() == case.records[call].tobytes(), call


def test_errors_leave_the_output_alone(case):
    """Every invalid argument returns VX_ERR_INVALID_ARGUMENT with the field named and leaves host and device outputs at their sentinels; a
    context without a commit returns VX_ERR_STATE; count == 0 is VX_OK and writes nothing."""
    import ctypes as C
    import torch

    L, h, vp = hip.lib(), case.svo._h, C.c_void_p
    out = np.full(48 * 4, 0x5a, dtype=np.uint8)
    d_out = filled(2)
    v = np.tile(np.array([3.0, 3.0, 3.0], dtype=np.float32), 32)
    d_v = torch.from_numpy(v).cuda()
    assert d_out.data_ptr() % 16 == 0 and out.ctypes.data % 4 == 0

    def batch(base, **fields):
        b = hip.BoxBatch(base, base + 96, base + 192, 12, 12, 12, 0)
        for k, val in fields.items():
            setattr(b, k, val)
        return b

    def shape(**fields):
        s = hip.MOVE_SHAPE()
        for k, val in fields.items():
            setattr(s, k, val)
        return C.byref(s)

    hb, db = v.ctypes.data, d_v.data_ptr()
    hm, dm = vp(hb + 288), vp(db + 288)
    o, do = vp(out.ctypes.data), vp(d_out.data_ptr())
    H, D = hip.VX_MEM_HOST, hip.VX_MEM_DEVICE
    refusals = ((lambda: L.vx_move_boxes(None, C.byref(batch(hb)), hm, 12, 2, shape(), H, o), b"null context"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(hb)), hm, 12, 2, shape(), 3, o), b"VX_MEM"),
                (lambda: L.vx_move_boxes(h, None, hm, 12, 2, shape(), H, o), b"null boxes"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(hb)), None, 12, 2, shape(), H, o), b"null motion"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(hb)), hm, 12, 2, None, H, o), b"null shape"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(hb)), hm, 12, 2, shape(), H, None), b"null out"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(hb, origin=None)), hm, 12, 2, shape(), H, o), b"null origin"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(hb, extents=None)), hm, 12, 2, shape(), H, o), b"null extents"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(hb, origin_stride=8)), hm, 12, 2, shape(), H, o), b"origin_stride"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(hb, offset_stride=14)), hm, 12, 2, shape(), H, o), b"offset_stride"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(hb, extents_stride=8)), hm, 12, 2, shape(), H, o), b"extents_stride"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(hb)), hm, 8, 2, shape(), H, o), b"motion_stride"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(hb)), hm, 14, 2, shape(), H, o), b"motion_stride"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(hb)), vp(hb + 290), 12, 2, shape(), H, o), b"motion must be aligned"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(hb, origin=hb + 2)), hm, 12, 2, shape(), H, o), b"origin must be aligned"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(hb)), hm, 12, (1 << 24) + 1, shape(), H, o), b"count exceeds"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(hb)), hm, 12, 2, shape(scale=float("nan")), H, o), b"scale"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(hb)), hm, 12, 2, shape(scale=float("inf")), H, o), b"scale"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(hb)), hm, 12, 2, shape(skin=-0.001), H, o), b"skin"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(hb)), hm, 12, 2, shape(skin=1.5), H, o), b"skin"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(hb)), hm, 12, 2, shape(skin=float("nan")), H, o), b"skin"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(hb)), hm, 12, 2, shape(order=0), H, o), b"order"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(hb)), hm, 12, 2, shape(order=0x23), H, o), b"order"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(hb)), hm, 12, 2, shape(order=0x21 | 0x40), H, o), b"order"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(hb)), hm, 12, 2, shape(flags=1), H, o), b"flags"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(db)), dm, 12, 2, shape(), D, vp(d_out.data_ptr() + 8)), b"out in device memory"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(db)), dm, 6, 2, shape(), D, do), b"motion_stride"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(db)), dm, 12, 2, shape(order=0x3f), D, do), b"order"),
                (lambda: L.vx_move_boxes(h, C.byref(batch(db, origin=db + 1)), dm, 12, 2, shape(), D, do), b"origin must be aligned"))
    uncommitted = (lambda ctx: L.vx_move_boxes(ctx, C.byref(batch(hb)), hm, 12, 2, shape(), H, o), lambda ctx: L.vx_move_boxes(ctx, C.byref(batch(db)), dm, 12, 2, shape(), D, do))
    # count == 0: VX_OK whatever the rest is (a shape there must be); nothing is read or written
    nothing_to_do = (lambda: L.vx_move_boxes(h, C.byref(batch(hb)), hm, 12, 0, shape(), H, o),
                     lambda: L.vx_move_boxes(h, None, None, 0, 0, shape(), H, None),
                     lambda: L.vx_move_boxes(h, C.byref(batch(db)), dm, 12, 0, shape(), D, do))
    leaves_the_outputs_alone(case, [out], [d_out], refusals, uncommitted, nothing_to_do)
    # and the call still works: two boxes of 3^3 voxels at (3, 3, 3) moving by (3, 3, 3)
    two = Moves(Boxes(v[:6].reshape(2, 3), v[24:30].reshape(2, 3), v[48:54].reshape(2, 3), "packed"), v[72:78].reshape(2, 3))
    assert L.vx_move_boxes(h, C.byref(batch(hb)), hm, 12, 2, shape(), H, o) == 0
    assert out[:96].tobytes() == moves_truth(case, two).tobytes() and (out[96:] == 0x5a).all()
