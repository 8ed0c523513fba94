"""vx_overlap_boxes on the GPU (voxel-rs_amd/csrc/blocks/kernels_boxes.hip): what a batch of float boxes holds, against the host harness's
records (tests/cpp/boxes_on_host.cpp: the same header on the host, which tests/test_boxes_on_host.py holds against the dense arrays) and
against numpy directly where the world or the boxes change. Three worlds, both formats; every comparison is byte for byte. A case is computed
once and left unchanged."""
import types

import numpy as np
import pytest

from batch_cases import _chunk_of
from boxes_cases import (INVALID, SCAN_CASES, SEEDED, Boxes, HostBoxes, boxes_truth, calls_for, differing, harness, make_boxes, make_scan_case)
from helpers import vra  # noqa: F401
from physics_cases import DT
from voxel_rs_amd import hip

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A


def make_context(c, capacity=None):
    svo = hip.Svo(c.svo_type, c.world.size_in_bytes + (1 << 20) if capacity is None else capacity)
    svo.set_materials(c.mats)
    svo.set_textures(c.tex, 6)
    svo.update_full(c.world)
    return svo


def filled(records):
    """A device buffer of `records` records, every byte 0x5a."""
    import torch

    return torch.full((records, 8), SENTINEL, dtype=torch.int32, device="cuda")


def as_records(t):
    return hip.box_hits_to_numpy(t)


def check_buffer(dev, exp, what):
    """A buffer two records longer than the batch: the records, then the untouched tail."""
    got = as_records(dev)
    assert differing(got[:len(exp)], exp) is None, f"{what}: {differing(got[:len(exp)], exp)}"
    assert len(got) == len(exp) + 2 and (got[len(exp):].view(np.uint32) == SENTINEL).all(), what


_CASES = {}


def the_case(name, fmt):
    """The world, a context that has it, its boxes in every form and the harness's records of each; shared by the tests of this module."""
    if (name, fmt) not in _CASES:
        c = make_scan_case(name, fmt)
        c.boxes = make_boxes(c)
        c.calls = calls_for(c, c.boxes)
        host = HostBoxes(harness(), c)
        c.records = {call: host.records(b, only_value) for call, b, only_value in c.calls}
        host.close()
        for a in c.records.values():
            a.setflags(write=False)
        c.svo = make_context(c)
        _CASES[name, fmt] = c
    return _CASES[name, fmt]


@pytest.fixture(scope="module", autouse=True)
def _contexts():
    yield
    for c in _CASES.values():
        c.svo.close()
    _CASES.clear()


@pytest.fixture(scope="module", params=SCAN_CASES, ids=[f"{n}-{f}" for n, f in SCAN_CASES])
def case(request):
    return the_case(*request.param)


def test_device_and_host_memory_give_the_harness_records(case):
    """Every form and only_value: the device calls queued together before one vx_sync, each into a buffer two records longer than the batch;
    then the same boxes as host-memory calls."""
    svo = case.svo
    queued = []
    for call, b, only_value in case.calls:
        args = b.torch_args()
        queued.append((args, svo.overlap_boxes(*args, only_value=only_value, out=filled(len(b) + 2))))
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
        queued.append((one, args, case.svo.overlap_boxes(*args, out=filled(3))))
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
    dev = c.svo.overlap_boxes(*args, out=filled(len(many) + 2))
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
    t = c.truth
    top = np.where((t != 0).any(axis=1), t.shape[1] - 1 - (t[:, ::-1, :] != 0).argmax(axis=1), -1)  # [x][z]: the highest block
    held = np.argwhere(top >= 0)
    e = np.zeros(256, dtype=hip.ENTITY_DTYPE)
    for k in range(len(e)):
        x, z = (int(v) for v in held[rng.integers(len(held))])
        e["position"][k] = c.info["lo"] + (x + 0.5, top[x, z] + 1 + rng.uniform(0.2, 0.9), z + 0.5)
    e["velocity"] = np.stack([rng.uniform(-30, 30, len(e)), np.full(len(e), -40.0), rng.uniform(-30, 30, len(e))], axis=1)
    e["aabb_offset"], e["aabb_extents"] = (-0.4, 0.0, -0.4), (0.8, 1.8, 0.8)
    e["gravity"], e["max_fall_velocity"], e["flags"] = 20.0, 50.0, hip.ENTITY_FLYING
    d = torch.from_numpy(e.view(np.uint8).copy()).cuda()
    c.svo.physics_step(d, DT, 8)
    dev = c.svo.overlap_boxes(*hip.entity_boxes(d), out=filled(len(e) + 2))  # enqueued behind the steps; no sync in between
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
        first = svo.overlap_boxes(*args, out=filled(len(boxes) + 2))  # enqueued; the commit below has to wait for it on the device
        b = c.info["blocks"].copy()
        b[6, 0, 24], b[17, 17, 17], b[0, 0, 0] = 0, 12, 9  # one block of the floor removed, one set in the air, one replaced
        assert c.info["blocks"][6, 0, 24] != 0 and c.info["blocks"][17, 17, 17] == 0 and c.info["blocks"][0, 0, 0] not in (0, 9)
        c.world.set_chunk((0, 0, 0), _chunk_of((0, 0, 0), 5, b))
        c.world.serialize()
        svo.update_full(c.world)  # vx_commit_all
        changed = types.SimpleNamespace(info=c.info, truth=b, size=c.size)  # (no LOD chunk here: the world shows its blocks)
        new = boxes_truth(changed, boxes)
        second = svo.overlap_boxes(*args, out=filled(len(boxes) + 2))  # enqueued behind the commit's upload
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
    import ctypes as C

    c = the_case("glasshouse", "esvo")
    h = C.c_void_p()
    rc = hip.lib().vx_create(c.svo_type, 1 << 32, 0, C.byref(h))
    if rc == 3:  # VX_ERR_OUT_OF_MEMORY, from vx_create itself: the one reason to skip (as tests/test_blocks.py::test_esvo_big)
        pytest.skip("vx_create: " + hip.lib().vx_last_error().decode())
    assert rc == 0, hip.lib().vx_last_error()
    svo = hip.Svo.__new__(hip.Svo)
    svo._h, svo.svo_type = h, c.svo_type
    try:
        svo.set_materials(c.mats)
        svo.set_textures(c.tex, 6)
        svo.update_full(c.world)
        assert svo.get_stats()["capacity_bytes"] == 1 << 32
        queued = []
        for call, b, only_value in c.calls:
            args = b.torch_args()
            queued.append((args, svo.overlap_boxes(*args, only_value=only_value, out=filled(len(b) + 2))))
        svo.sync()
        for (call, b, only_value), (_, dev) in zip(c.calls, queued):
            check_buffer(dev, c.records[call], call)
            assert svo.overlap_boxes(*b.numpy_args(), only_value=only_value).tobytes() == c.records[call].tobytes(), call
    finally:
        svo.close()


def test_without_a_traversal_image_the_bytes_are_the_same(case, monkeypatch):
    """A context created with VX_TRAVERSAL_IMAGE=0 (read when a context is created) answers with the same bytes."""
    monkeypatch.setenv("VX_TRAVERSAL_IMAGE", "0")
    svo = make_context(case)
    try:
        assert svo.image_info()["layout"] == 0  # (no traversal image in this context)
        for call, b, only_value in case.calls:
            assert svo.overlap_boxes(*b.numpy_args(), only_value=only_value).tobytes() == case.records[call].tobytes(), call
    finally:
        svo.close()


def test_errors_leave_the_output_alone(case):
    """Every invalid argument returns VX_ERR_INVALID_ARGUMENT with the field named and leaves host and device outputs at their sentinels; a
    context without a commit returns VX_ERR_STATE; count == 0 is VX_OK and writes nothing."""
    import ctypes as C
    import torch

    L, h, vp = hip.lib(), case.svo._h, C.c_void_p
    out = np.full(32 * 4, 0x5a, dtype=np.uint8)
    sentinel = out.tobytes()
    d_out = filled(4)
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
    for call, word in ((lambda: L.vx_overlap_boxes(None, C.byref(batch(hb)), 2, hip.VX_MEM_HOST, o), b"null context"),
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
                       (lambda: L.vx_overlap_boxes(h, C.byref(batch(db, origin=db + 1)), 2, hip.VX_MEM_DEVICE, vp(d_out.data_ptr())), b"origin must be aligned")):
        rc = call()
        assert rc == 1 and word in L.vx_last_error(), (rc, word, L.vx_last_error())
        assert out.tobytes() == sentinel
    fresh = hip.Svo(case.svo_type, 1 << 20)
    try:
        assert L.vx_overlap_boxes(fresh._h, C.byref(batch(hb)), 2, hip.VX_MEM_HOST, o) == 6 and b"committed" in L.vx_last_error()
        assert L.vx_overlap_boxes(fresh._h, C.byref(batch(db)), 2, hip.VX_MEM_DEVICE, vp(d_out.data_ptr())) == 6
        assert out.tobytes() == sentinel
    finally:
        fresh.close()
    # count == 0: VX_OK whatever the rest is; nothing is read or written
    assert L.vx_overlap_boxes(h, C.byref(batch(hb)), 0, hip.VX_MEM_HOST, o) == 0
    assert L.vx_overlap_boxes(h, None, 0, hip.VX_MEM_HOST, None) == 0
    assert L.vx_overlap_boxes(h, C.byref(batch(db)), 0, hip.VX_MEM_DEVICE, vp(d_out.data_ptr())) == 0
    case.svo.sync()
    assert out.tobytes() == sentinel and (d_out.cpu().numpy().view(np.uint32) == SENTINEL).all()
    # and the call still works: two boxes of 3^3 voxels at (3, 3, 3), as the harness's program has them
    two = Boxes(v[:6].reshape(2, 3), v[24:30].reshape(2, 3), v[48:54].reshape(2, 3), "packed")
    assert L.vx_overlap_boxes(h, C.byref(batch(hb)), 2, hip.VX_MEM_HOST, o) == 0
    assert out[:64].tobytes() == boxes_truth(case, two).tobytes() and (out[64:] == 0x5a).all()
