"""vx_overlap_boxes on the GPU (voxel-rs_amd/csrc/blocks/kernels_boxes.hip): what a batch of float boxes holds, against the host harness's
records (tests/cpp/boxes_on_host.cpp: the same header on the host, which tests/test_boxes_on_host.py holds against the dense arrays) and
against numpy directly where the world or the boxes change. Three worlds, both formats; every comparison is byte for byte. A case is computed
once and left unchanged."""
import types

import numpy as np
import pytest

from batch_cases import _chunk_of
from boxes_cases import (INVALID, SCAN_CASES, SEEDED, Boxes, HostBoxes, boxes_truth, calls_for, differing, harness, make_boxes, make_scan_case)
from gpu_harness import (above_the_blocks, big_esvo_context, flying_entities, leaves_the_outputs_alone, make_context, no_image_context, records_head, sentinel_words,
                         shared_cases)
from helpers import vra  # noqa: F401
from physics_cases import DT
from voxel_rs_amd import hip

pytestmark = pytest.mark.gpu


def filled(count):
    """A device buffer two records longer than a batch of `count`, every byte 0x5a."""
    return sentinel_words(count, 8)


def check_buffer(dev, exp, what):
    """A buffer two records longer than the batch: the records, then the untouched tail."""
    raw = hip.box_hits_to_numpy(dev)
    got = records_head(raw, len(exp), what)
    assert differing(got, exp) is None, f"{what}: {differing(got, exp)}"
    assert len(raw) == len(exp) + 2, what


def build(name, fmt):
    """The world, a context that has it, its boxes in every form and the harness's records of each; shared by the tests of this module."""
    c = make_scan_case(name, fmt)
    c.boxes = make_boxes(c)
    c.calls = calls_for(c, c.boxes)
    host = HostBoxes(harness(), c)
    c.records = {call: host.records(b, only_value) for call, b, only_value in c.calls}
    host.close()
    for a in c.records.values():
        a.setflags(write=False)
    c.svo = make_context(c)
    return c


the_case, _contexts, case = shared_cases(build, SCAN_CASES)


def test_device_and_host_memory_give_the_harness_records(case):
    """Every form and only_value: the device calls queued together before one vx_sync, each into a buffer two records longer than the batch;
    then the same boxes as host-memory calls."""
    svo = case.svo
    queued = []
    for call, b, only_value in case.calls:
        args = b.torch_args()
        queued.append((args, svo.overlap_boxes(*args, only_value=only_value, out=filled(len(b)))))
    svo.sync()
    for (call, b, only_value), (_, dev) in zip(case.calls, queued):
        check_buffer(dev, case.records[call], f"{case.name}-{case.fmt} {call}")
        host = svo.overlap_boxes(*b.numpy_args(), only_value=only_value)
        assert host.dtype == hip.BOX_HIT_DTYPE and differing(host, case.records[call]) is None, f"{call} in host memory: {differing(host, case.records[call])}"
    packed = case.records["packed"]
    assert (packed["blocks"][:SEEDED] > 0).mean() >= 0.5 and (packed["blocks"] == INVALID).sum() >= 45 and (case.records["absent"]["blocks"] % INVALID == 0).all()


def test_one_box(case):
    """count == 1, device and host: a box with blocks, a box without, a record that is no box."""
    b, exp = case.boxes, case.records["packed"]
    picks = [int(np.flatnonzero(exp["blocks"][:SEEDED] > 0)[0]), int(np.flatnonzero(exp["blocks"][:SEEDED] == 0)[0]), int(b.invalid[0])]
    queued = []
    for i in picks:
        one = Boxes(b.origin[i:i + 1], b.offset[i:i + 1], b.extents[i:i + 1], "packed")
        args = one.torch_args()
        queued.append((one, args, case.svo.overlap_boxes(*args, out=filled(1))))
    case.svo.sync()
    for i, (one, _, dev) in zip(picks, queued):
        check_buffer(dev, exp[i:i + 1], f"box {i}")
        assert case.svo.overlap_boxes(*one.numpy_args()).tobytes() == exp[i:i + 1].tobytes(), i


@pytest.mark.parametrize("fmt", ["esvo", "csvo"])
def test_a_grid_beyond_65535_workgroups(fmt):
    """count == 70,001: the seeded set of `glasshouse` tiled; box i's record is the set's record i mod 2,000."""
    c = the_case("glasshouse", fmt)
    b = c.boxes
    seeded = Boxes(b.origin[:SEEDED], b.offset[:SEEDED], b.extents[:SEEDED], "packed")
    many, idx = seeded.tiled(70001)
    exp = c.records["packed"][:SEEDED][idx]
    args = many.torch_args()
    dev = c.svo.overlap_boxes(*args, out=filled(len(many)))
    c.svo.sync()
    check_buffer(dev, exp, "device")
    assert c.svo.overlap_boxes(*many.numpy_args()).tobytes() == exp.tobytes()


@pytest.mark.parametrize("fmt", ["esvo", "csvo"])
def test_behind_physics_step(fmt):
    """256 flying entities in device memory (no gravity, no collision: they move 1.28 voxels down into the floor) stepped 8 times, then
    vx_overlap_boxes over the same records in place with no sync between the two calls; after one vx_sync the entities are read back, and
    the records are numpy's for the positions the steps left -- which differ from those of the positions before."""
    import torch

    c = the_case("glasshouse", fmt)
    rng = np.random.default_rng(71)
    e = flying_entities(256, above_the_blocks(c, 256, rng, 0.2, 0.9), rng)  # 0.2 to 0.9 above their column's highest block
    d = torch.from_numpy(e.view(np.uint8).copy()).cuda()
    c.svo.physics_step(d, DT, 8)
    dev = c.svo.overlap_boxes(*hip.entity_boxes(d), out=filled(len(e)))  # enqueued behind the steps; no sync in between
    c.svo.sync()
    after = d.cpu().numpy().view(hip.ENTITY_DTYPE)
    assert (after["position"][:, 1] < e["position"][:, 1] - 1.0).all()
    before_truth = boxes_truth(c, Boxes(e["position"], e["aabb_offset"], e["aabb_extents"], "entities"))
    exp = boxes_truth(c, Boxes(after["position"], after["aabb_offset"], after["aabb_extents"], "entities"))
    assert (before_truth["blocks"] != exp["blocks"]).sum() >= 64 and (exp["blocks"] > 0).sum() >= 64
    check_buffer(dev, exp, "behind vx_physics_step")
    assert c.svo.overlap_boxes(*hip.entity_boxes(after)).tobytes() == exp.tobytes()


@pytest.mark.parametrize("fmt", ["esvo", "csvo"])
def test_ordered_between_commits(fmt):
    """A call into device memory, three blocks changed on the host chunk and committed with vx_commit_all, the call again into a second buffer,
    one vx_sync: the first buffer shows the old world and the second the new one, both exactly as numpy has them; a box around the removed
    block loses one from its count (tests/test_list.py::test_ordered_between_commits: the commit's uploads wait for the event
    mark_world_read records behind the last launch)."""
    c = make_scan_case("glasshouse", fmt)
    svo = make_context(c)
    try:
        seeded = make_boxes(c)
        around = [("removed", (5.5, -0.5, 23.5), (0.0, 0.0, 0.0), (2.0, 2.0, 2.0)), ("set", (16.5, 16.5, 16.5), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
                  ("replaced", (-1.0, -1.0, -1.0), (0.0, 0.0, 0.0), (1.5, 1.5, 1.5))]
        boxes = Boxes(np.concatenate([seeded.origin[:SEEDED], np.array([r[1] for r in around], dtype=np.float32)]),
                      np.concatenate([seeded.offset[:SEEDED], np.array([r[2] for r in around], dtype=np.float32)]),
                      np.concatenate([seeded.extents[:SEEDED], np.array([r[3] for r in around], dtype=np.float32)]), "packed")
        args = boxes.torch_args()
        old = boxes_truth(c, boxes)
        first = svo.overlap_boxes(*args, out=filled(len(boxes)))  # enqueued; the commit below has to wait for it on the device
        b = c.info["blocks"].copy()
        b[6, 0, 24], b[17, 17, 17], b[0, 0, 0] = 0, 12, 9  # one block of the floor removed, one set in the air, one replaced
        assert c.info["blocks"][6, 0, 24] != 0 and c.info["blocks"][17, 17, 17] == 0 and c.info["blocks"][0, 0, 0] not in (0, 9)
        c.world.set_chunk((0, 0, 0), _chunk_of((0, 0, 0), 5, b))
        c.world.serialize()
        svo.update_full(c.world)  # vx_commit_all
        changed = types.SimpleNamespace(info=c.info, truth=b, size=c.size)  # (no LOD chunk here: the world shows its blocks)
        new = boxes_truth(changed, boxes)
        second = svo.overlap_boxes(*args, out=filled(len(boxes)))  # enqueued behind the commit's upload
        svo.sync()
        assert old.tobytes() != new.tobytes()
        assert new["blocks"][SEEDED] == old["blocks"][SEEDED] - 1 and (old["blocks"][SEEDED + 1], new["blocks"][SEEDED + 1]) == (0, 1)
        assert new["value"][SEEDED + 1] == 12 and new["blocks"][SEEDED + 2] == old["blocks"][SEEDED + 2] == 1 and new["value"][SEEDED + 2] == 9 != old["value"][SEEDED + 2]
        check_buffer(first, old, "before the commit")
        check_buffer(second, new, "after the commit")
    finally:
        svo.close()


def test_esvo_big():
    """The glasshouse in an ESVO context of 4 GiB, which selects the VX_SVO_ESVO_BIG build of the kernel: every form and only_value."""
    c = the_case("glasshouse", "esvo")
    with big_esvo_context(c) as svo:
        queued = []
        for call, b, only_value in c.calls:
            args = b.torch_args()
            queued.append((args, svo.overlap_boxes(*args, only_value=only_value, out=filled(len(b)))))
        svo.sync()
        for (call, b, only_value), (_, dev) in zip(c.calls, queued):
            check_buffer(dev, c.records[call], call)
            assert svo.overlap_boxes(*b.numpy_args(), only_value=only_value).tobytes() == c.records[call].tobytes(), call


def test_without_a_traversal_image_the_bytes_are_the_same(case, monkeypatch):
    """A context created with VX_TRAVERSAL_IMAGE=0 (read when a context is created) answers with the same bytes."""
    with no_image_context(case, monkeypatch) as svo:
        for call, b, only_value in case.calls:
            assert svo.overlap_boxes(*b.numpy_args(), only_value=only_value).tobytes() == case.records[call].tobytes(), call


def test_errors_leave_the_output_alone(case):
    """Every invalid argument returns VX_ERR_INVALID_ARGUMENT with the field named and leaves host and device outputs at their sentinels; a
    context without a commit returns VX_ERR_STATE; count == 0 is VX_OK and writes nothing."""
    import ctypes as C
    import torch

    L, h, vp = hip.lib(), case.svo._h, C.c_void_p
    out = np.full(32 * 4, 0x5a, dtype=np.uint8)
    d_out = filled(2)
    v = np.tile(np.array([3.0, 3.0, 3.0], dtype=np.float32), 24)
    d_v = torch.from_numpy(v).cuda()
    assert d_out.data_ptr() % 16 == 0 and out.ctypes.data % 4 == 0

    def batch(base, **fields):
        b = hip.BoxBatch(base, base + 96, base + 192, 12, 12, 12, 0)
        for k, val in fields.items():
            setattr(b, k, val)
        return b

    hb, db = v.ctypes.data, d_v.data_ptr()
    o = vp(out.ctypes.data)
    refusals = ((lambda: L.vx_overlap_boxes(None, C.byref(batch(hb)), 2, hip.VX_MEM_HOST, o), b"null context"),
                (lambda: L.vx_overlap_boxes(h, C.byref(batch(hb)), 2, 3, o), b"VX_MEM"),
                (lambda: L.vx_overlap_boxes(h, None, 2, hip.VX_MEM_HOST, o), b"null boxes"),
                (lambda: L.vx_overlap_boxes(h, C.byref(batch(hb)), 2, hip.VX_MEM_HOST, None), b"null out"),
                (lambda: L.vx_overlap_boxes(h, C.byref(batch(hb, origin=None)), 2, hip.VX_MEM_HOST, o), b"null origin"),
                (lambda: L.vx_overlap_boxes(h, C.byref(batch(hb, extents=None)), 2, hip.VX_MEM_HOST, o), b"null extents"),
                (lambda: L.vx_overlap_boxes(h, C.byref(batch(hb, origin_stride=8)), 2, hip.VX_MEM_HOST, o), b"origin_stride"),
                (lambda: L.vx_overlap_boxes(h, C.byref(batch(hb, origin_stride=0)), 2, hip.VX_MEM_HOST, o), b"origin_stride"),
                (lambda: L.vx_overlap_boxes(h, C.byref(batch(hb, offset_stride=14)), 2, hip.VX_MEM_HOST, o), b"offset_stride"),
                (lambda: L.vx_overlap_boxes(h, C.byref(batch(hb, extents_stride=8)), 2, hip.VX_MEM_HOST, o), b"extents_stride"),
                (lambda: L.vx_overlap_boxes(h, C.byref(batch(hb, origin=hb + 2)), 2, hip.VX_MEM_HOST, o), b"origin must be aligned"),
                (lambda: L.vx_overlap_boxes(h, C.byref(batch(hb, offset=hb + 97)), 2, hip.VX_MEM_HOST, o), b"offset must be aligned"),
                (lambda: L.vx_overlap_boxes(h, C.byref(batch(hb, extents=hb + 193)), 2, hip.VX_MEM_HOST, o), b"extents must be aligned"),
                (lambda: L.vx_overlap_boxes(h, C.byref(batch(hb)), (1 << 24) + 1, hip.VX_MEM_HOST, o), b"count exceeds"),
                (lambda: L.vx_overlap_boxes(h, C.byref(batch(db)), 2, hip.VX_MEM_DEVICE, vp(d_out.data_ptr() + 8)), b"out in device memory"),
                (lambda: L.vx_overlap_boxes(h, C.byref(batch(db, extents_stride=6)), 2, hip.VX_MEM_DEVICE, vp(d_out.data_ptr())), b"extents_stride"),
                (lambda: L.vx_overlap_boxes(h, C.byref(batch(db, origin=db + 1)), 2, hip.VX_MEM_DEVICE, vp(d_out.data_ptr())), b"origin must be aligned"))
    uncommitted = (lambda ctx: L.vx_overlap_boxes(ctx, C.byref(batch(hb)), 2, hip.VX_MEM_HOST, o),
                   lambda ctx: L.vx_overlap_boxes(ctx, C.byref(batch(db)), 2, hip.VX_MEM_DEVICE, vp(d_out.data_ptr())))
    # count == 0: VX_OK whatever the rest is; nothing is read or written
    nothing_to_do = (lambda: L.vx_overlap_boxes(h, C.byref(batch(hb)), 0, hip.VX_MEM_HOST, o),
                     lambda: L.vx_overlap_boxes(h, None, 0, hip.VX_MEM_HOST, None),
                     lambda: L.vx_overlap_boxes(h, C.byref(batch(db)), 0, hip.VX_MEM_DEVICE, vp(d_out.data_ptr())))
    leaves_the_outputs_alone(case, [out], [d_out], refusals, uncommitted, nothing_to_do)
    # and the call still works: two boxes of 3^3 voxels at (3, 3, 3), as the harness's program has them
    two = Boxes(v[:6].reshape(2, 3), v[24:30].reshape(2, 3), v[48:54].reshape(2, 3), "packed")
    assert L.vx_overlap_boxes(h, C.byref(batch(hb)), 2, hip.VX_MEM_HOST, o) == 0
    assert out[:64].tobytes() == boxes_truth(case, two).tobytes() and (out[64:] == 0x5a).all()
