"""vx_block_points and vx_read_region on the GPU (voxel-rs_amd/csrc/blocks): block ids read from the world the device holds, against the host
harness's records (tests/cpp/blocks_on_host.cpp: the same header on the host) and, with that, against the dense arrays the worlds were built
from (tests/blocks_cases.py). Both worlds, both formats; every comparison is byte for byte. A case is computed once and left unchanged."""
import numpy as np
import pytest

from batch_cases import CASES, RAY_SEED, TRANSLUCENT_IDS, _chunk_of, build_rays_for, oracle_hits
from blocks_cases import REGIONS, check_cells, classify, dense_region, harness, host_points, make_block_case
from gpu_harness import big_esvo_context, leaves_the_outputs_alone, make_context, no_image_context, to_device
from helpers import vra  # noqa: F401
from voxel_rs_amd import hip

pytestmark = pytest.mark.gpu
COUNTS = [1, 63, 64, 65, None]  # None: the whole set


def region_to_numpy(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module", params=CASES, ids=[f"{n}-{f}" for n, f in CASES])
def case(request):
    """The world, a context that has it, the points and what the host harness says of them -- which is the ground truth (asserted here)."""
    c = make_block_case(*request.param)
    c.exe = harness()
    c.host_cells = host_points(c.exe, c, c.pts, 12, len(c.pts))
    check_cells(c, c.host_cells)
    c.host_cells.setflags(write=False)
    c.svo = make_context(c)
    yield c
    c.svo.close()


@pytest.mark.parametrize("count", COUNTS, ids=[str(n or "all") for n in COUNTS])
def test_points_from_device_memory(case, count):
    """1: device tensors -- packed, inside vx_entity records (stride 64), inside vx_ray_hit records (pos at offset 16, stride 32) -- and host
    arrays give the host harness's records."""
    import torch

    n = count or len(case.pts)
    pts, exp = case.pts[:n], case.host_cells[:n]
    svo = case.svo
    d_pts = to_device(pts)  # (every device input stays alive until the sync: a call returns after enqueueing)
    packed = svo.block_points(d_pts)
    e = np.zeros(n, dtype=hip.ENTITY_DTYPE)
    e["position"], e["velocity"] = pts, 3.0
    ents = to_device(e.view(np.uint8))
    in_entities = svo.block_points(hip.entity_positions(ents))
    h = np.full(n, 0x5a, dtype=np.uint8).repeat(32).view(hip.RAY_HIT_DTYPE)
    h["pos"] = pts
    hits = to_device(h.view(np.uint8))
    in_hits = svo.block_points(hip.ray_hit_positions(hits), out=torch.full((n, 2), -7, dtype=torch.int32, device="cuda"))
    svo.sync()
    assert tuple(packed.shape) == (n, 2)
    for name, got in (("packed", packed), ("vx_entity.position", in_entities), ("vx_ray_hit.pos", in_hits)):
        got = hip.block_cells_to_numpy(got)
        bad = np.flatnonzero(got.view(np.uint64) != exp.view(np.uint64))
        assert got.tobytes() == exp.tobytes(), f"{name}: {len(bad)} records differ, first at {bad[0]}: point {pts[bad[0]]!r} got {got[bad[0]]} expected {exp[bad[0]]}"
    assert ents.cpu().numpy().tobytes() == e.tobytes() and hits.cpu().numpy().tobytes() == h.tobytes()  # (inputs are only read)
    assert svo.block_points(pts).tobytes() == exp.tobytes()
    assert svo.block_points(hip.entity_positions(e)).tobytes() == exp.tobytes()
    out = np.zeros(n, dtype=hip.BLOCK_CELL_DTYPE)
    assert svo.block_points(hip.ray_hit_positions(h), out=out) is out and out.tobytes() == exp.tobytes()


def small_regions(case):
    """(lo, size): one voxel; 9 x 1 x 1 across a brick boundary; a box wholly outside the world; boxes of 8, 16 and 24 on the brick grid."""
    solid = np.argwhere(case.truth != 0)[0] + case.info["lo"]
    # on the brick grid, in the terrain at the chunks' middle (for far_chunks: where all four meet, the LOD chunk among them)
    grid = (case.info["lo"] + np.array([case.truth.shape[0] // 2, 8, case.truth.shape[2] // 2])) // 8 * 8
    size = int(case.info["size"])
    return [(tuple(int(v) for v in solid), (1, 1, 1)), ((int(solid[0]) // 8 * 8 - 4, int(solid[1]), int(solid[2])), (9, 1, 1)), ((-40, -9, 3), (8, 9, 3)),
            ((size, 0, 8), (5, 4, 3))] + [(tuple(int(v) - 8 * (s // 16) for v in grid), (s, s, s)) for s in (8, 16, 24)]


def test_regions_against_the_dense_arrays(case):
    """2: the 70^3 glasshouse region / the 75 x 37 x 77 far_chunks region and the small ones, device and host memory."""
    svo = case.svo
    boxes = [REGIONS[case.name]] + small_regions(case)
    on_device = [svo.read_region(lo, size, device=True) for lo, size in boxes]
    svo.sync()
    for (lo, size), dev in zip(boxes, on_device):
        exp = dense_region(case.info, case.truth, lo, size)
        got = region_to_numpy(dev)
        assert got.shape == exp.shape and (got == exp).all(), (lo, size, np.argwhere(got != exp)[:8])
        host = svo.read_region(lo, size)
        assert host.dtype == np.uint32 and host.tobytes() == exp.tobytes(), (lo, size)
    assert dense_region(case.info, case.truth, *boxes[0]).any() and dense_region(case.info, case.truth, *boxes[1]).all()
    assert not dense_region(case.info, case.truth, *boxes[3]).any() and all(dense_region(case.info, case.truth, *b).any() for b in boxes[5:])
    # any size component 0: nothing to do, nothing touched
    assert svo.read_region((0, 0, 0), (5, 0, 5)).size == 0


def test_a_regions_voxels_are_the_points_at_their_centres(case):
    lo, size = small_regions(case)[-1]
    region = case.svo.read_region(lo, size)
    z, y, x = np.meshgrid(np.arange(size[2]), np.arange(size[1]), np.arange(size[0]), indexing="ij")
    centres = np.ascontiguousarray(np.stack([x + lo[0] + 0.5, y + lo[1] + 0.5, z + lo[2] + 0.5], axis=-1).reshape(-1, 3).astype(np.float32))
    assert (case.svo.block_points(centres)["value"] == region.reshape(-1)).all()


def test_without_a_traversal_image_the_bytes_are_the_same(case, monkeypatch):
    """2, last item: a context created with VX_TRAVERSAL_IMAGE=0 (read when a context is created) answers with the same bytes."""
    with no_image_context(case, monkeypatch) as svo:
        assert svo.block_points(case.pts).tobytes() == case.host_cells.tobytes()
        for lo, size in [REGIONS[case.name]] + small_regions(case):
            assert svo.read_region(lo, size).tobytes() == case.svo.read_region(lo, size).tobytes(), (lo, size)


@pytest.mark.parametrize("fmt", ["esvo", "csvo"])
def test_ordered_between_commits(fmt):
    """3: a region read into device memory, three blocks changed on the host chunk and committed with vx_commit_all, the region read again
    into a second buffer, one vx_sync: the first buffer shows the old world and the second the new one, both exactly. What this shows is the
    order the caller sees. A commit's uploads run on a stream of the context's own, which waits for the event mark_world_read records behind
    the read (vx_commit; the read runs on another stream): without that call the first read and the upload would race, which a run of this
    test may or may not catch."""
    c = make_block_case("glasshouse", fmt)
    svo = make_context(c)
    try:
        lo, size = REGIONS["glasshouse"]
        old = dense_region(c.info, c.truth, lo, size)
        first = svo.read_region(lo, size, device=True)  # enqueued; the commit below has to wait for it on the device
        b = c.info["blocks"].copy()
        b[6, 5, 24], b[17, 17, 17], b[0, 0, 0] = 0, 12, 9  # one block removed, one set in the air, one replaced
        assert c.info["blocks"][6, 5, 24] != 0 and c.info["blocks"][17, 17, 17] == 0 and c.info["blocks"][0, 0, 0] not in (0, 9)
        c.world.set_chunk((0, 0, 0), _chunk_of((0, 0, 0), 5, b))
        c.world.serialize()
        svo.update_full(c.world)  # vx_commit_all
        second = svo.read_region(lo, size, device=True)  # enqueued behind the commit's upload
        changed = to_device(np.float32([[6.5, 5.5, 24.5], [17.5, 17.5, 17.5], [0.5, 0.5, 0.5]]))
        cells = svo.block_points(changed)
        svo.sync()
        new = dense_region(c.info, b, lo, size)
        assert (old != new).sum() == 3
        assert (region_to_numpy(first) == old).all(), np.argwhere(region_to_numpy(first) != old)[:8]
        assert (region_to_numpy(second) == new).all(), np.argwhere(region_to_numpy(second) != new)[:8]
        assert hip.block_cells_to_numpy(cells)["value"].tolist() == [0, 12, 9]
    finally:
        svo.close()


def test_esvo_big():
    """The glasshouse in an ESVO context of 4 GiB, which selects the VX_SVO_ESVO_BIG builds of both kernels (runtime.cpp: ctx->big depends on the
    capacity alone; the world is read through a 64-bit address with an explicit range check): points from device and host memory and the
    regions, against the host harness's records and the dense array."""
    c = make_block_case("glasshouse", "esvo")
    with big_esvo_context(c) as svo:
        exp = host_points(harness(), c, c.pts, 12, len(c.pts))
        check_cells(c, exp)
        d_pts = to_device(c.pts)
        cells = svo.block_points(d_pts)
        boxes = [REGIONS["glasshouse"]] + small_regions(c)
        on_device = [svo.read_region(lo, size, device=True) for lo, size in boxes]
        svo.sync()
        assert hip.block_cells_to_numpy(cells).tobytes() == exp.tobytes() == svo.block_points(c.pts).tobytes()
        for (lo, size), dev in zip(boxes, on_device):
            want = dense_region(c.info, c.truth, lo, size)
            assert (region_to_numpy(dev) == want).all() and svo.read_region(lo, size).tobytes() == want.tobytes(), (lo, size)


def test_the_block_behind_a_hit_face_is_the_hits_value(case):
    """4: for the rays of batch_cases that hit a full-detail opaque block from outside (chosen by the oracle's hits), the block at
    pos - 0.5 * normal(face_id) is hits.value. The rays are cast and the points made on the device, with no copy in between. (The shared ray set
    alone holds 171 such rays on glasshouse: a second set from the same builder, with another seed, brings both worlds above 200.)"""
    import torch

    o, d, m = (np.concatenate(a) for a in zip(*(build_rays_for(case.info, seed)[:3] for seed in (RAY_SEED[case.name], RAY_SEED[case.name] + 100))))
    oracle = oracle_hits(case.scene, o, d, m, False)
    inward = oracle["pos"] - np.float32(0.5) * hip.FACE_NORMALS[np.clip(oracle["face_id"], 0, 5)]
    k = classify(case.info, case.truth, inward)
    chosen = (oracle["dst"] > 0) & (oracle["inside_voxel"] == 0) & ~np.isin(oracle["value"], TRANSLUCENT_IDS) & k["solid"]
    assert chosen.sum() >= 200, int(chosen.sum())
    idx = np.flatnonzero(chosen)
    d_o, d_d, d_m, normals = to_device(o[idx]), to_device(d[idx]), to_device(m[idx]), to_device(hip.FACE_NORMALS)  # (alive until the sync)
    hits = case.svo.raycast_batch(d_o, d_d, d_m)
    with torch.cuda.stream(torch.cuda.ExternalStream(case.svo.stream)):  # torch's step of the chain, on the context's stream: behind the cast
        points = (hip.ray_hit_positions(hits) - 0.5 * normals[hits[:, 2].long()]).contiguous()
    cells = case.svo.block_points(points)
    case.svo.sync()
    got, h = hip.block_cells_to_numpy(cells), hip.ray_hits_to_numpy(hits)
    assert h.tobytes() == oracle[idx].tobytes()
    assert (got["value"] == h["value"]).all() and (got["cell_log2"] == 0).all() and (got["value"] == k["value"][idx]).all()


def test_errors_leave_the_output_alone(case):
    """Every invalid argument returns VX_ERR_INVALID_ARGUMENT with the field named and writes nothing; a context without a commit returns
    VX_ERR_STATE; no points and an empty box are VX_OK."""
    import ctypes as C

    L, h, vp = hip.lib(), case.svo._h, C.c_void_p
    pts = np.array(case.pts[:8], order="C")
    out = np.full(8 * 8, 0x5a, dtype=np.uint8)
    lo3, size3 = (C.c_int32 * 3)(0, 0, 0), (C.c_uint32 * 3)(2, 2, 2)
    o = vp(out.ctypes.data)
    refusals = ((lambda: L.vx_block_points(h, vp(pts.ctypes.data), 8, 8, hip.VX_MEM_HOST, o), b"pos_stride"),
                (lambda: L.vx_block_points(h, None, 12, 8, hip.VX_MEM_HOST, o), b"null pos"),
                (lambda: L.vx_block_points(h, vp(pts.ctypes.data), 12, 8, 3, o), b"VX_MEM"),
                (lambda: L.vx_read_region(h, None, C.byref(size3), hip.VX_MEM_HOST, o), b"null lo"),
                (lambda: L.vx_read_region(h, C.byref(lo3), C.byref((C.c_uint32 * 3)(256, 256, 257)), hip.VX_MEM_HOST, o), b"size.x"))
    uncommitted = (lambda ctx: L.vx_block_points(ctx, vp(pts.ctypes.data), 12, 8, hip.VX_MEM_HOST, vp(out.ctypes.data)),
                   lambda ctx: L.vx_read_region(ctx, C.byref(lo3), C.byref(size3), hip.VX_MEM_HOST, vp(out.ctypes.data)))
    nothing_to_do = (lambda: L.vx_block_points(h, None, 12, 0, hip.VX_MEM_HOST, None),
                     lambda: L.vx_block_points(h, vp(pts.ctypes.data + 1), 5, 0, hip.VX_MEM_DEVICE, vp(out.ctypes.data + 3)),  # (no points: nothing to refuse)
                     lambda: L.vx_read_region(h, C.byref(lo3), C.byref((C.c_uint32 * 3)(2, 0, 2)), hip.VX_MEM_DEVICE, None))
    leaves_the_outputs_alone(case, [out], [], refusals, uncommitted, nothing_to_do)
