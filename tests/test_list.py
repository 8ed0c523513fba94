"""vx_list_region on the GPU (voxel-rs_amd/csrc/blocks/kernels_list.hip): the blocks of a box as a compact list with their open faces, against
the host harness's records (tests/cpp/list_on_host.cpp: the same header on the host, which tests/test_list_on_host.py holds against the dense
arrays) and against numpy directly where the world changes. Three worlds, both formats; every comparison is byte for byte. A case is
computed once and left unchanged."""
import contextlib
import types

import numpy as np
import pytest

from batch_cases import _chunk_of
from blocks_cases import REGIONS
from gpu_harness import SENTINEL, big_esvo_context, leaves_the_outputs_alone, make_context, no_image_context
from helpers import vra  # noqa: F401
from list_cases import EXPOSED, FACES, FLAG_SETS, MAIN_BOXES, SCAN_CASES, HostLists, boxes_for, differing, expected_list, harness, make_scan_case
from voxel_rs_amd import hip

pytestmark = pytest.mark.gpu


def filled(records):
    """A device buffer of exactly `records` records (a capacity is a part of this call), every byte 0x5a."""
    import torch

    return torch.full((records, 2), SENTINEL, dtype=torch.int32, device="cuda")


def as_records(t):
    return hip.block_ats_to_numpy(t)


@pytest.fixture(scope="module", params=SCAN_CASES, ids=[f"{n}-{f}" for n, f in SCAN_CASES])
def case(request):
    """The world, a context that has it, and the harness's list of every box under every flag set."""
    c = make_scan_case(*request.param)
    c.host = HostLists(harness(), c)
    c.boxes = boxes_for(c)
    c.lists = {(name, flags): c.host.list(lo, size, flags)[0] for name, lo, size in c.boxes for flags in FLAG_SETS}
    for a in c.lists.values():
        a.setflags(write=False)
    c.svo = make_context(c)
    yield c
    c.svo.close()
    c.host.close()


def test_device_and_host_memory_give_the_harness_records(case):
    """Every box and flag set: the device calls queued together before one vx_sync, each into a buffer two records longer than its list."""
    svo = case.svo
    calls = [(name, lo, size, flags) for name, lo, size in case.boxes for flags in FLAG_SETS]
    queued = [svo.list_region(lo, size, flags, out=filled(len(case.lists[name, flags]) + 2)) for name, lo, size, flags in calls]
    svo.sync()
    for (name, lo, size, flags), (dev, total) in zip(calls, queued):
        exp = case.lists[name, flags]
        got = as_records(dev)
        assert int(total.item()) == len(exp), (name, flags, int(total.item()), len(exp))
        assert differing(got[:len(exp)], exp) is None, f"{name} {lo} {size} flags {flags}: {differing(got[:len(exp)], exp)}"
        assert (got[len(exp):].view(np.uint32) == SENTINEL).all(), (name, flags)
        host, host_total = svo.list_region(lo, size, flags)
        assert host_total == len(exp) and host.dtype == hip.BLOCK_AT_DTYPE and host.tobytes() == exp.tobytes(), (name, flags)
    assert len(case.lists["main", 0]) >= 1500 and not len(case.lists["outside", 0])


def test_the_plain_list_scattered_is_the_region(case):
    """Flags 0, scattered on the device into zeros: vx_read_region of the same box in the same context."""
    import torch

    svo = case.svo
    for name, lo, size in case.boxes:
        records, total = svo.list_region(lo, size, 0, device=True)
        region = svo.read_region(lo, size, device=True)
        svo.sync()
        n = int(total.item())
        where, value = records[:n, 0].long(), records[:n, 1]
        assert int(where.max().item() if n else 0) < region.numel() and (where >> 24 == 0).all()
        dense = torch.zeros(region.numel(), dtype=torch.int32, device="cuda")
        dense[where] = value
        assert torch.equal(dense, region.reshape(-1)), name
        assert n == int((region != 0).sum().item())


@pytest.mark.parametrize("flags", [0, EXPOSED], ids=["plain", "exposed"])
def test_capacity_cuts_the_list_and_nothing_else(case, flags):
    """capacity = total // 2 into a buffer of `total` records filled with 0x5a: the first half is exact, the second untouched, the total
    unchanged; capacity 0 with no out gives the same total."""
    svo = case.svo
    lo, size = MAIN_BOXES[case.name]
    exp = case.lists["main", flags | (FACES if flags else 0)]
    half = len(exp) // 2
    buf = filled(len(exp))
    _, total = svo.list_region(lo, size, flags, capacity=half, out=buf)
    _, counted = svo.list_region(lo, size, flags, capacity=0, device=True)
    svo.sync()
    got = as_records(buf)
    assert half >= 700 and int(total.item()) == int(counted.item()) == len(exp)
    assert differing(got[:half], exp[:half]) is None and (got[half:].view(np.uint32) == SENTINEL).all()
    host, host_total = svo.list_region(lo, size, flags, capacity=half)
    assert host_total == len(exp) and host.tobytes() == exp[:half].tobytes()
    out = np.frombuffer(bytearray(b"\x5a" * (8 * len(exp))), dtype=hip.BLOCK_AT_DTYPE)
    written, again = svo.list_region(lo, size, flags, capacity=half, out=out)
    assert again == len(exp) and len(written) == half and out[:half].tobytes() == exp[:half].tobytes() and (out[half:].view(np.uint8) == 0x5a).all()
    assert svo.list_region(lo, size, flags, capacity=0)[1] == len(exp)


def test_the_workspace_is_reused_and_grows():
    """A large box and then a small one with no sync between them share the context's workspace in stream order; a second context's first call
    is a tiny box and its second the 134^3 box (5,832 bricks), so its workspace has to grow with a call still queued."""
    c = make_scan_case("tower", "esvo")
    host = HostLists(harness(), c)
    boxes = {name: (lo, size) for name, lo, size in boxes_for(c)}
    flags = EXPOSED | FACES
    exp = {name: host.list(*boxes[name], flags)[0] for name in ("main", "grid8", "one_voxel")}
    first, second = make_context(c), make_context(c)
    try:
        big = first.list_region(*boxes["main"], flags, out=filled(len(exp["main"])))
        small = first.list_region(*boxes["grid8"], flags, out=filled(len(exp["grid8"])))
        tiny = second.list_region(*boxes["one_voxel"], flags, out=filled(len(exp["one_voxel"])))
        grown = second.list_region(*boxes["main"], flags, out=filled(len(exp["main"])))
        after = second.list_region(*boxes["grid8"], flags, out=filled(len(exp["grid8"])))
        first.sync()
        second.sync()
        for name, (dev, total) in (("main", big), ("grid8", small), ("one_voxel", tiny), ("main", grown), ("grid8", after)):
            assert int(total.item()) == len(exp[name]) and differing(as_records(dev), exp[name]) is None, (name, differing(as_records(dev), exp[name]))
        assert len(exp["main"]) >= 20000 and len(exp["grid8"]) >= 50 and len(exp["one_voxel"]) == 1
    finally:
        first.close()
        second.close()
        host.close()


@pytest.mark.parametrize("fmt", ["esvo", "csvo"])
def test_ordered_between_commits(fmt):
    """A list into device memory, three blocks changed on the host chunk and committed with vx_commit_all, the list again into a second
    buffer, one vx_sync: the first buffer shows the old world and the second the new one, both exactly as numpy has them -- the removed
    block's neighbours have gained a face bit (tests/test_blocks.py::test_ordered_between_commits: the commit's uploads wait for the event
    mark_world_read records behind the last launch)."""
    c = make_scan_case("glasshouse", fmt)
    svo = make_context(c)
    try:
        lo, size = REGIONS["glasshouse"]
        old = expected_list(c, lo, size, FACES)
        first = svo.list_region(lo, size, FACES, out=filled(len(old) + 4))  # enqueued; the commit below has to wait for it on the device
        b = c.info["blocks"].copy()
        b[6, 0, 24], b[17, 17, 17], b[0, 0, 0] = 0, 12, 9  # one block of the floor removed, one set in the air, one replaced
        assert c.info["blocks"][6, 0, 24] != 0 and c.info["blocks"][17, 17, 17] == 0 and c.info["blocks"][0, 0, 0] not in (0, 9)
        c.world.set_chunk((0, 0, 0), _chunk_of((0, 0, 0), 5, b))
        c.world.serialize()
        svo.update_full(c.world)  # vx_commit_all
        changed = types.SimpleNamespace(info=c.info, truth=b)  # (no LOD chunk here: the world shows its blocks)
        new = expected_list(changed, lo, size, FACES)
        second = svo.list_region(lo, size, FACES, out=filled(len(new) + 4))  # enqueued behind the commit's upload
        svo.sync()
        assert len(new) == len(old) and old.tobytes() != new.tobytes()
        # the removed block's neighbour in the floor at x - 1 shows its +x face now, and not before
        at = ((24 - lo[2]) * size[1] + (0 - lo[1])) * size[0] + (5 - lo[0])
        faces_at = lambda records: int(hip.split_where(records["where"][hip.split_where(records["where"])[0] == at])[1][0])  # noqa: E731
        assert faces_at(old) & 2 == 0 and faces_at(new) & 2 == 2
        for (dev, total), exp in ((first, old), (second, new)):
            assert int(total.item()) == len(exp) and differing(as_records(dev)[:len(exp)], exp) is None, differing(as_records(dev)[:len(exp)], exp)
    finally:
        svo.close()


def test_esvo_big():
    """The glasshouse in an ESVO context of 4 GiB, which selects the VX_SVO_ESVO_BIG builds of the kernels: every box and flag set."""
    c = make_scan_case("glasshouse", "esvo")
    with big_esvo_context(c) as svo, contextlib.closing(HostLists(harness(), c)) as host:
        calls = [(name, lo, size, flags, host.list(lo, size, flags)[0]) for name, lo, size in boxes_for(c) for flags in FLAG_SETS]
        queued = [svo.list_region(lo, size, flags, out=filled(len(exp) + 1)) for _, lo, size, flags, exp in calls]
        svo.sync()
        for (name, lo, size, flags, exp), (dev, total) in zip(calls, queued):
            assert int(total.item()) == len(exp) and differing(as_records(dev)[:len(exp)], exp) is None, (name, flags)
            assert svo.list_region(lo, size, flags)[0].tobytes() == exp.tobytes(), (name, flags)


def test_without_a_traversal_image_the_bytes_are_the_same(case, monkeypatch):
    """A context created with VX_TRAVERSAL_IMAGE=0 (read when a context is created) answers with the same bytes."""
    with no_image_context(case, monkeypatch) as svo:
        for name, lo, size in case.boxes:
            for flags in FLAG_SETS:
                got, total = svo.list_region(lo, size, flags)
                assert total == len(case.lists[name, flags]) and got.tobytes() == case.lists[name, flags].tobytes(), (name, flags)


def test_errors_leave_the_output_alone(case):
    """Every invalid argument returns VX_ERR_INVALID_ARGUMENT with the field named and leaves out and total at their sentinels; a context
    without a commit returns VX_ERR_STATE; an empty box is VX_OK and writes total = 0, in host and in device memory."""
    import ctypes as C
    import torch

    L, h, vp = hip.lib(), case.svo._h, C.c_void_p
    out = np.full(8 * 8, 0x5a, dtype=np.uint8)
    total = np.full(4, 0x5a, dtype=np.uint8)
    d_out, d_total = filled(8), filled(1)
    sentinel = out.tobytes()
    lo3, size3 = (C.c_int32 * 3)(0, 0, 0), (C.c_uint32 * 3)(2, 2, 2)
    o, t = vp(out.ctypes.data), vp(total.ctypes.data)
    refusals = ((lambda: L.vx_list_region(h, None, C.byref(size3), 0, hip.VX_MEM_HOST, o, 8, t), b"null lo"),
                (lambda: L.vx_list_region(h, C.byref(lo3), None, 0, hip.VX_MEM_HOST, o, 8, t), b"null size"),
                (lambda: L.vx_list_region(h, C.byref(lo3), C.byref(size3), 4, hip.VX_MEM_HOST, o, 8, t), b"flags"),
                (lambda: L.vx_list_region(h, C.byref(lo3), C.byref(size3), 0, 3, o, 8, t), b"VX_MEM"),
                (lambda: L.vx_list_region(h, C.byref(lo3), C.byref(size3), 0, hip.VX_MEM_HOST, o, 8, None), b"null total"),
                (lambda: L.vx_list_region(h, C.byref(lo3), C.byref(size3), 0, hip.VX_MEM_HOST, None, 8, t), b"null out"),
                (lambda: L.vx_list_region(h, C.byref(lo3), C.byref((C.c_uint32 * 3)(256, 256, 257)), 0, hip.VX_MEM_HOST, o, 8, t), b"size.x"),
                (lambda: L.vx_list_region(h, C.byref(lo3), C.byref(size3), 0, hip.VX_MEM_DEVICE, vp(d_out.data_ptr() + 4), 7, vp(d_total.data_ptr())), b"out in device memory"),
                (lambda: L.vx_list_region(h, C.byref(lo3), C.byref(size3), 0, hip.VX_MEM_DEVICE, vp(d_out.data_ptr()), 8, vp(d_total.data_ptr() + 2)), b"total in device memory"))
    uncommitted = (lambda ctx: L.vx_list_region(ctx, C.byref(lo3), C.byref(size3), 0, hip.VX_MEM_HOST, o, 8, t),)
    leaves_the_outputs_alone(case, [out, total], [d_out, d_total], refusals, uncommitted)
    # any size component 0: total = 0, out not touched; with no total, nothing at all
    empty = (C.c_uint32 * 3)(2, 0, 2)
    assert L.vx_list_region(h, C.byref(lo3), C.byref(empty), 3, hip.VX_MEM_HOST, o, 8, t) == 0
    assert out.tobytes() == sentinel and total.view(np.uint32)[0] == 0
    assert L.vx_list_region(h, C.byref(lo3), C.byref(empty), 0, hip.VX_MEM_HOST, None, 8, None) == 0
    assert L.vx_list_region(h, C.byref(lo3), C.byref(empty), 0, hip.VX_MEM_DEVICE, vp(d_out.data_ptr()), 8, vp(d_total.data_ptr())) == 0
    case.svo.sync()
    assert (d_out.cpu().numpy().view(np.uint32) == SENTINEL).all() and int(d_total.cpu()[0, 0]) == 0 and int(d_total.cpu()[0, 1]) == SENTINEL
    assert torch.cuda.is_available()
