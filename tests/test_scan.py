"""vx_scan_points and vx_scan_columns on the GPU (voxel-rs_amd/csrc/blocks): the first block along an axis read from the world the device
holds, against the host harness's records (tests/cpp/scan_on_host.cpp: the same header on the host), which test_scan_on_host.py holds against
the numpy truth of tests/scan_cases.py. Three worlds, both formats, six directions; every comparison is byte for byte. A case is computed
once and left unchanged."""
import numpy as np
import pytest

from batch_cases import TRANSLUCENT_IDS, _chunk_of, oracle_hits
from scan_cases import (DIR_NAMES, DIRECTIONS, GAP, NONE, SCAN_CASES, TO_EDGE, axes_of, boxes_for, columns_truth, differing, first_of_region, harness,
                        host_scan_columns, host_scan_points, make_scan_case, points_truth)
from gpu_harness import SENTINEL, big_esvo_context, leaves_the_outputs_alone, make_context, no_image_context, to_device
from helpers import vra  # noqa: F401
from voxel_rs_amd import hip

pytestmark = pytest.mark.gpu
COUNTS = [1, 63, 64, 65, None]  # None: the whole set


def host_records(c):
    """What the host harness says: the whole point set in all six directions to the world's edge, at reach 2 downwards, the gap points one
    voxel short of their block and on it, and every box."""
    c.exe = harness()
    n = len(c.pts)
    c.exp_points = {d: host_scan_points(c.exe, c, c.pts, 12, n, d, TO_EDGE)[0] for d in DIRECTIONS}
    c.exp_reach2 = host_scan_points(c.exe, c, c.pts, 12, n, hip.VX_DIR_NEG_Y, 2)[0]
    c.exp_gaps = {(d, r): host_scan_points(c.exe, c, c.gaps[d], 12, len(c.gaps[d]), d, r)[0] for d in DIRECTIONS for r in (GAP, GAP + 1)}
    c.boxes = {d: boxes_for(c, d) for d in DIRECTIONS}
    c.exp_boxes = {(d, name): host_scan_columns(c.exe, c, lo, size, d)[0] for d in DIRECTIONS for name, lo, size in c.boxes[d]}
    for a in list(c.exp_points.values()) + list(c.exp_gaps.values()) + list(c.exp_boxes.values()) + [c.exp_reach2]:
        a.setflags(write=False)


@pytest.fixture(scope="module", params=SCAN_CASES, ids=[f"{n}-{f}" for n, f in SCAN_CASES])
def case(request):
    """The world, a context that has it, and the host harness's records of its points and boxes."""
    c = make_scan_case(*request.param)
    host_records(c)
    # (the harness against the truth, where it is cheap: test_scan_on_host.py does all of it)
    assert differing(c.exp_points[hip.VX_DIR_NEG_Y], points_truth(c, c.pts, hip.VX_DIR_NEG_Y, TO_EDGE)) is None
    c.svo = make_context(c)
    yield c
    c.svo.close()


def sentinel_out(shape):
    """A device record tensor of `shape` records inside a larger sentinel-filled one: (the records' view, the whole tensor)."""
    import torch

    records = int(np.prod(shape))
    whole = torch.full(((records + 8) * 4,), SENTINEL, dtype=torch.int32, device="cuda")
    return whole[:records * 4].view(tuple(shape) + (4,)), whole


def tail_untouched(whole, records):
    return bool((whole[records * 4:] == SENTINEL).all().item())


@pytest.mark.parametrize("count", COUNTS, ids=[str(n or "all") for n in COUNTS])
def test_points_from_device_memory(case, count):
    """Device tensors -- packed, inside vx_entity records (stride 64), inside vx_ray_hit records (pos at offset 16, stride 32) -- and host
    arrays give the host harness's records: VX_DIR_NEG_Y and VX_DIR_POS_X on every count, all six directions on the whole set."""
    n = count or len(case.pts)
    pts, svo = case.pts[:n], case.svo
    d_pts = to_device(pts)  # (every device input stays alive until the sync: a call returns after enqueueing)
    e = np.zeros(n, dtype=hip.ENTITY_DTYPE)
    e["position"], e["velocity"] = pts, 3.0
    ents = to_device(e.view(np.uint8))
    h = np.full(n, 0x5a, dtype=np.uint8).repeat(32).view(hip.RAY_HIT_DTYPE)
    h["pos"] = pts
    hits = to_device(h.view(np.uint8))
    got = {}
    for d in DIRECTIONS if count is None else (hip.VX_DIR_NEG_Y, hip.VX_DIR_POS_X):
        out, whole = sentinel_out((n,))
        got[d] = (svo.scan_points(d_pts, d), svo.scan_points(hip.entity_positions(ents), d), svo.scan_points(hip.ray_hit_positions(hits), d, out=out), whole)
    svo.sync()
    for d, (packed, in_entities, in_hits, whole) in got.items():
        exp = case.exp_points[d][:n]
        assert tuple(packed.shape) == (n, 4)
        for name, records in (("packed", packed), ("vx_entity.position", in_entities), ("vx_ray_hit.pos", in_hits)):
            assert differing(hip.scan_hits_to_numpy(records), exp) is None, (DIR_NAMES[d], name, differing(hip.scan_hits_to_numpy(records), exp))
        assert tail_untouched(whole, n)
        assert svo.scan_points(pts, d).tobytes() == exp.tobytes()
        out = np.zeros(n, dtype=hip.SCAN_HIT_DTYPE)
        assert svo.scan_points(hip.entity_positions(e), d, out=out) is out and out.tobytes() == exp.tobytes()
    assert svo.scan_points(hip.ray_hit_positions(h), hip.VX_DIR_NEG_Y).tobytes() == case.exp_points[hip.VX_DIR_NEG_Y][:n].tobytes()
    assert ents.cpu().numpy().tobytes() == e.tobytes() and hits.cpu().numpy().tobytes() == h.tobytes() and d_pts.cpu().numpy().tobytes() == pts.tobytes()  # (inputs are only read)


def test_reaches(case):
    """Reach 2 on the whole set; the gap points at a reach that ends one voxel short of the block (none) and on it, in all six directions."""
    svo = case.svo
    d_pts = to_device(case.pts)
    two = svo.scan_points(d_pts, hip.VX_DIR_NEG_Y, reach=2)
    d_gaps = {d: to_device(case.gaps[d]) for d in DIRECTIONS}
    got = {(d, r): svo.scan_points(d_gaps[d], d, reach=r) for d in DIRECTIONS for r in (GAP, GAP + 1)}
    svo.sync()
    assert differing(hip.scan_hits_to_numpy(two), case.exp_reach2) is None
    for (d, r), records in got.items():
        records = hip.scan_hits_to_numpy(records)
        assert differing(records, case.exp_gaps[d, r]) is None, (DIR_NAMES[d], r)
        assert ((records["coord"] == NONE) == (r == GAP)).all()
        assert svo.scan_points(case.gaps[d], d, reach=r).tobytes() == case.exp_gaps[d, r].tobytes()


@pytest.mark.parametrize("direction", DIRECTIONS, ids=DIR_NAMES)
def test_columns_against_the_host_harness(case, direction):
    """Every box of scan_cases.boxes_for in device and in host memory. Device buffers are pre-filled with a sentinel: the bytes beyond
    size[u] * size[v] records stay as they are."""
    svo = case.svo
    _, u, v, _ = axes_of(direction)
    on_device = []
    for name, lo, size in case.boxes[direction]:
        out, whole = sentinel_out((size[v], size[u]))
        assert svo.scan_columns(lo, size, direction, out=out) is out
        on_device.append((out, whole))
    fresh = svo.scan_columns(*case.boxes[direction][0][1:], direction, device=True)
    svo.sync()
    for (name, lo, size), (out, whole) in zip(case.boxes[direction], on_device):
        exp = case.exp_boxes[direction, name]
        got = hip.scan_hits_to_numpy(out)
        assert differing(got, exp) is None, (name, lo, size, differing(got, exp))
        assert tail_untouched(whole, size[u] * size[v]), name
        on_host = svo.scan_columns(lo, size, direction)
        assert on_host.dtype == hip.SCAN_HIT_DTYPE and differing(on_host, exp) is None, (name, lo, size)
    assert differing(hip.scan_hits_to_numpy(fresh), case.exp_boxes[direction, case.boxes[direction][0][0]]) is None
    # any size component 0: nothing to do, nothing touched
    out, whole = sentinel_out((0, 0))
    assert svo.scan_columns((0, 0, 0), (5, 0, 5), direction).size == 0 and svo.scan_columns((0, 0, 0), (0, 5, 5), direction, out=out) is out
    svo.sync()
    assert tail_untouched(whole, 0)


@pytest.mark.parametrize("direction", DIRECTIONS, ids=DIR_NAMES)
def test_consistent_with_the_lookups_on_the_device(case, direction):
    """One box a world (the world, or the chunks, with a margin of 3): the scan is the first non-zero, in travel order, of vx_read_region of
    the same box, and vx_block_points at the answering voxel's centre gives the same value and cell_log2."""
    svo = case.svo
    _, lo, size = case.boxes[direction][2]
    a, u, v, _ = axes_of(direction)
    scan, region = svo.scan_columns(lo, size, direction, device=True), svo.read_region(lo, size, device=True)
    svo.sync()
    scan, region = hip.scan_hits_to_numpy(scan), region.cpu().numpy().view(np.uint32)
    coord, value = first_of_region(region, lo, direction)
    assert (scan["coord"] == coord).all() and (scan["value"] == value).all() and (scan["coord"] != NONE).any()
    found = np.argwhere(scan["coord"] != NONE)
    centres = np.zeros((len(found), 3), dtype=np.float32)
    centres[:, u], centres[:, v], centres[:, a] = found[:, 1] + lo[u] + 0.5, found[:, 0] + lo[v] + 0.5, scan["coord"][tuple(found.T)] + 0.5
    cells = svo.block_points(to_device(centres))
    svo.sync()
    cells = hip.block_cells_to_numpy(cells)
    assert (cells["value"] == scan["value"][tuple(found.T)]).all() and (cells["cell_log2"] == scan["cell_log2"][tuple(found.T)]).all()


def test_against_rays():
    """glasshouse: the columns whose downward ray from the cell centre at the world's top hits an opaque full-detail block from outside, as
    decided by batch_cases.oracle_hits alone -- 806 of the 34 x 34 = 1,156 columns over the chunk and a margin of 1 (132 miss, 218 end on
    glass or leaves). For those, vx_raycast_batch's value is the scan's, and the hit lies on the top face of the scan's voxel. The reference's
    traversal reports a hit position one quantum of its [1, 2) coordinates, 2^(depth - 23) blocks, inside the face it enters (all 806 of the
    oracle's hits here have pos.y = coord + 1 - 2^-17, none has floor(pos.y) == coord + 1), so the face is pinned exactly:
    coord + 1 - pos.y == 2^(depth - 23), and with it floor(pos.y) == coord. The oracle's own hits meet this against the host harness's records
    (checked here on the CPU, before the device is asked)."""
    from blocks_cases import make_block_case

    c = make_scan_case("glasshouse", "esvo")
    scene = make_block_case("glasshouse", "esvo").scene
    lo, size = (-1, 0, -1), (34, c.size, 34)
    z, x = np.meshgrid(np.arange(size[2]), np.arange(size[0]), indexing="ij")
    o = np.ascontiguousarray(np.stack([x + lo[0] + 0.5, np.full(x.shape, c.size - 0.5), z + lo[2] + 0.5], axis=-1).reshape(-1, 3).astype(np.float32))
    d = np.ascontiguousarray(np.broadcast_to(np.float32([0.0, -1.0, 0.0]), o.shape))
    m = np.full(len(o), -1.0, dtype=np.float32)
    oracle = oracle_hits(scene, o, d, m, False)
    chosen = np.flatnonzero((oracle["dst"] > 0) & (oracle["inside_voxel"] == 0) & ~np.isin(oracle["value"], TRANSLUCENT_IDS))
    print(f"\n{len(chosen)} of {len(o)} columns; {int((oracle['dst'] > 0).sum())} rays hit")
    assert len(chosen) == 806
    quantum = 2.0 ** (c.info["depth"] - 23)

    def on_the_top_face(hits, scan):
        top = scan["coord"][chosen].astype(np.float64) + 1.0
        return bool((hits["value"][chosen] == scan["value"][chosen]).all() and (top - hits["pos"][chosen, 1].astype(np.float64) == quantum).all()
                    and (np.floor(hits["pos"][chosen, 1]) == scan["coord"][chosen]).all())

    exp = host_scan_columns(harness(), c, lo, size, hip.VX_DIR_NEG_Y)[0].reshape(-1)
    assert on_the_top_face(oracle, exp)
    svo = make_context(c)
    try:
        d_o, d_d, d_m = to_device(o), to_device(d), to_device(m)
        hits, scan = svo.raycast_batch(d_o, d_d, d_m), svo.scan_columns(lo, size, hip.VX_DIR_NEG_Y, device=True)
        svo.sync()
        hits, scan = hip.ray_hits_to_numpy(hits), hip.scan_hits_to_numpy(scan).reshape(-1)
        assert differing(scan, exp) is None
        assert on_the_top_face(hits, scan) and (scan["cell_log2"][chosen] == 0).all()
    finally:
        svo.close()


def test_without_a_traversal_image_the_bytes_are_the_same(case, monkeypatch):
    """A context created with VX_TRAVERSAL_IMAGE=0 (read when a context is created) answers with the same bytes."""
    with no_image_context(case, monkeypatch) as svo:
        for d in DIRECTIONS:
            assert svo.scan_points(case.pts, d).tobytes() == case.exp_points[d].tobytes(), DIR_NAMES[d]
            for name, lo, size in case.boxes[d]:
                assert svo.scan_columns(lo, size, d).tobytes() == case.exp_boxes[d, name].tobytes(), (DIR_NAMES[d], name)


def test_esvo_big():
    """The glasshouse in an ESVO context of 4 GiB, which selects the VX_SVO_ESVO_BIG builds of both kernels (runtime.cpp: ctx->big depends on the
    capacity alone; the world is read through a 64-bit address with an explicit range check): points from device and host memory and the
    boxes, against the host harness's records."""
    c = make_scan_case("glasshouse", "esvo")
    with big_esvo_context(c) as svo:
        host_records(c)
        d_pts = to_device(c.pts)
        points = {d: svo.scan_points(d_pts, d) for d in DIRECTIONS}
        boxes = {(d, name): svo.scan_columns(lo, size, d, device=True) for d in DIRECTIONS for name, lo, size in c.boxes[d]}
        svo.sync()
        for d in DIRECTIONS:
            assert differing(hip.scan_hits_to_numpy(points[d]), c.exp_points[d]) is None and svo.scan_points(c.pts, d).tobytes() == c.exp_points[d].tobytes()
            for name, lo, size in c.boxes[d]:
                assert differing(hip.scan_hits_to_numpy(boxes[d, name]), c.exp_boxes[d, name]) is None, (DIR_NAMES[d], name)
                assert svo.scan_columns(lo, size, d).tobytes() == c.exp_boxes[d, name].tobytes(), (DIR_NAMES[d], name)


@pytest.mark.parametrize("fmt", ["esvo", "csvo"])
def test_ordered_between_commits(fmt):
    """A heightmap into device memory; on the host chunk one column's top block removed and one block set in the air above another column;
    vx_commit_all; the heightmap again into a second buffer and a scan of three device points; one vx_sync. The first buffer shows the old
    world and the second the new one, exactly, and exactly two columns differ: the commit's uploads wait for the first scan (the event
    mark_world_read records behind it), and the second scan runs behind them."""
    c = make_scan_case("glasshouse", fmt)
    svo = make_context(c)
    try:
        lo, size = (-3, -3, -3), (70, 70, 70)
        old = columns_truth(c, lo, size, hip.VX_DIR_NEG_Y)
        first = svo.scan_columns(lo, size, hip.VX_DIR_NEG_Y, device=True)  # enqueued; the commit below has to wait for it on the device
        b = c.info["blocks"].copy()
        assert b[28, 15, 28] != 0 and not b[28, 16:, 28].any() and b[20, 0, 5] != 0 and not b[20, 1:, 5].any()
        b[28, 15, 28], b[20, 25, 5] = 0, 12  # the floating block removed (its column's top); a block set in the air above a floor column
        c.world.set_chunk((0, 0, 0), _chunk_of((0, 0, 0), 5, b))
        c.world.serialize()
        svo.update_full(c.world)  # vx_commit_all
        second = svo.scan_columns(lo, size, hip.VX_DIR_NEG_Y, device=True)  # enqueued behind the commit's upload
        probes = to_device(np.float32([[28.5, 40.5, 28.5], [20.5, 40.5, 5.5], [3.5, 40.5, 3.5]]))
        below = svo.scan_points(probes, hip.VX_DIR_NEG_Y)
        svo.sync()
        new = old.copy()
        new[28 + 3, 28 + 3], new[5 + 3, 20 + 3] = (0, b[28, 0, 28], 0, 0), (25, 12, 0, 0)
        assert (old != new).sum() == 2
        first, second = hip.scan_hits_to_numpy(first), hip.scan_hits_to_numpy(second)
        assert differing(first, old) is None, differing(first, old)
        assert differing(second, new) is None, differing(second, new)
        assert hip.scan_hits_to_numpy(below)[["coord", "value"]].tolist() == [(0, int(b[28, 0, 28])), (25, 12), (0, int(b[3, 0, 3]))]
    finally:
        svo.close()


def test_errors_leave_the_output_alone(case):
    """Every invalid argument returns VX_ERR_INVALID_ARGUMENT with the field named and writes nothing; a context without a commit returns
    VX_ERR_STATE; no points and an empty box are VX_OK."""
    import ctypes as C

    L, h, vp = hip.lib(), case.svo._h, C.c_void_p
    pts = np.array(case.pts[:8], order="C")
    out = np.full(8 * 16, 0x5a, dtype=np.uint8)
    lo3, size3 = (C.c_int32 * 3)(0, 0, 0), (C.c_uint32 * 3)(2, 2, 2)
    o, p = vp(out.ctypes.data), vp(pts.ctypes.data)
    refusals = ((lambda: L.vx_scan_points(h, p, 8, 8, 2, 1, hip.VX_MEM_HOST, o), b"pos_stride"),
                (lambda: L.vx_scan_points(h, None, 12, 8, 2, 1, hip.VX_MEM_HOST, o), b"null pos"),
                (lambda: L.vx_scan_points(h, p, 12, 8, 6, 1, hip.VX_MEM_HOST, o), b"direction"),
                (lambda: L.vx_scan_points(h, p, 12, 8, 2, 0, hip.VX_MEM_HOST, o), b"reach"),
                (lambda: L.vx_scan_points(h, p, 12, 8, 2, 1, 3, o), b"VX_MEM"),
                (lambda: L.vx_scan_columns(h, None, C.byref(size3), 2, hip.VX_MEM_HOST, o), b"null lo"),
                (lambda: L.vx_scan_columns(h, C.byref(lo3), C.byref(size3), -1, hip.VX_MEM_HOST, o), b"direction"),
                (lambda: L.vx_scan_columns(h, C.byref(lo3), C.byref((C.c_uint32 * 3)(4097, 1, 4096)), 2, hip.VX_MEM_HOST, o), b"size"),
                (lambda: L.vx_scan_columns(h, C.byref(lo3), C.byref((C.c_uint32 * 3)(1, (1 << 24) + 1, 1)), 2, hip.VX_MEM_HOST, o), b"size"))
    uncommitted = (lambda ctx: L.vx_scan_points(ctx, p, 12, 8, 2, 1, hip.VX_MEM_HOST, o), lambda ctx: L.vx_scan_columns(ctx, C.byref(lo3), C.byref(size3), 2, hip.VX_MEM_HOST, o))
    nothing_to_do = (lambda: L.vx_scan_points(h, None, 12, 0, 2, 1, hip.VX_MEM_HOST, None),
                     lambda: L.vx_scan_points(h, vp(pts.ctypes.data + 1), 5, 0, 0, 0, hip.VX_MEM_DEVICE, vp(out.ctypes.data + 3)),  # (no points: nothing to refuse)
                     lambda: L.vx_scan_columns(h, C.byref(lo3), C.byref((C.c_uint32 * 3)(2, 0, 2)), 2, hip.VX_MEM_DEVICE, None))
    leaves_the_outputs_alone(case, [out], [], refusals, uncommitted, nothing_to_do)
