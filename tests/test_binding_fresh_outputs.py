"""The one path of the batch and block methods that tests/test_binding_calls.py cannot reach without a GPU: device inputs and no outputs
given, so that the binding allocates the tensors itself. For every method: the returned tensors' dtype, shape and device as its docstring
states them and, after sync(), their bytes against the same call on host arrays (record fields that are padding aside: nobody writes them).
The smallest world a case module builds (glasshouse, ESVO), 3 items, boxes of 4 x 4 x 4 cells, max_pieces=2, path_capacity=4."""
import numpy as np
import pytest

from blocks_cases import make_block_case
from helpers import vra  # noqa: F401
from voxel_rs_amd import hip

pytestmark = pytest.mark.gpu
N, SIZE, STRIDE, MOST, PATH = 3, (4, 4, 4), 64, 2, 4
POINTS = np.array([[20.5, 30.5, 20.5], [32.25, 33.75, 31.5], [40.0, 20.0, 44.5]], dtype=np.float32)
LO = np.floor(POINTS).astype(np.int32) - 2
GOALS = POINTS + np.float32([1.0, 0.0, 1.0])
EXTENTS, MOTION, DOWN = np.float32([0.8, 1.8, 0.8]), np.float32([0.3, -0.5, 0.2]), np.float32([0.0, -1.0, 0.0])
PROPS = np.full(256, hip.VX_LIGHT_TRANSPARENT, dtype=np.uint8)


@pytest.fixture(scope="module")
def svo():
    c = make_block_case("glasshouse", "esvo")
    s = hip.Svo(c.svo_type, c.world.size_in_bytes + (1 << 20))
    s.set_materials(c.mats)
    s.set_textures(c.tex, 6)
    s.update_full(c.world)
    yield s
    s.close()


def dev(a):
    import torch

    return torch.from_numpy(a.copy()).cuda()


def tensor(t, dtype, shape, like=None):
    """A fresh output as the docstrings state it: its dtype, its shape, and the device -- of the input, or the current one."""
    import torch

    assert isinstance(t, torch.Tensor) and t.dtype == dtype and tuple(t.shape) == shape and t.is_cuda and t.is_contiguous()
    assert t.device == (like.device if like is not None else torch.device("cuda", torch.cuda.current_device()))


def same(got, expected):
    """Records field by field, but for the padding; plain numbers byte for byte."""
    assert got.dtype == expected.dtype and got.shape == expected.shape
    for name in expected.dtype.names or ():
        if not name.startswith("_"):
            assert got[name].tobytes() == expected[name].tobytes(), name
    if not expected.dtype.names:
        assert got.tobytes() == expected.tobytes()


def test_ray_batches(svo):
    import torch

    o, d = dev(POINTS), dev(DOWN)
    views = [hip.make_uniforms(np.eye(4, dtype=np.float32).ravel(), 1.0, 1.0, 0.3, (0, -1, 0), tuple(p), 0, 1.0) for p in POINTS]
    hits = svo.raycast_batch(o, d, 40.0)
    rgba, records = svo.trace_rays(views[0], o, d, 40.0, want_hits=True)
    rgba8, none = svo.trace_rays(views[0], o, d, 40.0, fmt=hip.VX_FORMAT_RGBA8)
    v_rgba, v_records = svo.trace_views(views, 4, 2, want_hits=True, device=True)
    svo.sync()
    tensor(hits, torch.int32, (N, 8), o)
    tensor(rgba, torch.float32, (N, 4), o)
    tensor(records, torch.int32, (N, 12), o)
    tensor(rgba8, torch.uint8, (N, 4), o)
    tensor(v_rgba, torch.float32, (N, 2, 4, 4))
    tensor(v_records, torch.int32, (N, 8, 12))
    assert none is None
    same(hip.ray_hits_to_numpy(hits), svo.raycast_batch(POINTS, DOWN, 40.0))
    h_rgba, h_records = svo.trace_rays(views[0], POINTS, DOWN, 40.0, want_hits=True)
    same(rgba.cpu().numpy(), h_rgba)
    same(hip.trace_hits_to_numpy(records), h_records)
    same(rgba8.cpu().numpy(), svo.trace_rays(views[0], POINTS, DOWN, 40.0, fmt=hip.VX_FORMAT_RGBA8)[0])
    h_rgba, h_records = svo.trace_views(views, 4, 2, want_hits=True)
    same(v_rgba.cpu().numpy(), h_rgba)
    same(hip.trace_hits_to_numpy(v_records).reshape(N, 8), h_records)


def test_points_and_regions(svo):
    import torch

    p = dev(POINTS)
    lo = tuple(int(v) for v in LO[0])
    cells = svo.block_points(p)
    scans = svo.scan_points(p, hip.VX_DIR_NEG_Y, 16)
    ids = svo.read_region(lo, (4, 3, 2), device=True)
    columns = svo.scan_columns(lo, (4, 3, 2), hip.VX_DIR_NEG_Y, device=True)
    ats, total = svo.list_region(lo, (4, 3, 2), hip.VX_LIST_FACES, device=True)
    some, _ = svo.list_region(lo, (4, 3, 2), capacity=5, device=True)
    svo.sync()
    tensor(cells, torch.int32, (N, 2), p)
    tensor(scans, torch.int32, (N, 4), p)
    tensor(ids, torch.int32, (2, 3, 4))
    tensor(columns, torch.int32, (2, 4, 4))
    tensor(ats, torch.int32, (24, 2))
    tensor(total, torch.int32, (1,))
    tensor(some, torch.int32, (5, 2))
    same(hip.block_cells_to_numpy(cells), svo.block_points(POINTS))
    same(hip.scan_hits_to_numpy(scans), svo.scan_points(POINTS, hip.VX_DIR_NEG_Y, 16))
    same(ids.cpu().numpy().view(np.uint32), svo.read_region(lo, (4, 3, 2)))
    same(hip.scan_hits_to_numpy(columns), svo.scan_columns(lo, (4, 3, 2), hip.VX_DIR_NEG_Y))
    h_ats, h_total = svo.list_region(lo, (4, 3, 2), hip.VX_LIST_FACES)
    assert int(total[0]) == h_total
    same(hip.block_ats_to_numpy(ats)[:h_total], h_ats)


def test_boxes(svo):
    import torch

    o, e, m = dev(POINTS), dev(EXTENTS), dev(MOTION)
    boxes = svo.overlap_boxes(o, e)
    moves = svo.move_boxes(o, e, m)
    svo.sync()
    tensor(boxes, torch.int32, (N, 8), o)
    tensor(moves, torch.int32, (N, 12), o)
    same(hip.box_hits_to_numpy(boxes), svo.overlap_boxes(POINTS, EXTENTS))
    same(hip.move_hits_to_numpy(moves), svo.move_boxes(POINTS, EXTENTS, MOTION))


def test_fields(svo):
    import torch

    p, g, lo = dev(POINTS), dev(GOALS), dev(LO)
    flood = svo.flood_points(p, SIZE)
    light = svo.light_boxes(lo, SIZE, PROPS)
    label = svo.label_boxes(lo, SIZE, max_pieces=MOST)
    walk = svo.walk_points(p, SIZE, goals=g, path_capacity=PATH)
    svo.sync()
    for (fields, info), words, like in ((flood, 4, p), (light, 4, lo), (label[::2], 8, lo), (walk[:2], 8, p)):
        tensor(fields, torch.uint8, (N, STRIDE), like)
        tensor(info, torch.int32, (N, words), like)
    tensor(label[1], torch.int32, (N, MOST, 4), lo)
    tensor(walk[2], torch.int32, (N, PATH), p)
    h_fields, h_info = svo.flood_points(POINTS, SIZE)
    same(flood[0].cpu().numpy(), h_fields)
    same(hip.flood_infos_to_numpy(flood[1]), h_info)
    h_fields, h_info = svo.light_boxes(LO, SIZE, PROPS)
    same(light[0].cpu().numpy(), h_fields)
    same(hip.light_infos_to_numpy(light[1]), h_info)
    h_fields, h_pieces, h_info = svo.label_boxes(LO, SIZE, max_pieces=MOST)
    same(label[0].cpu().numpy(), h_fields)
    same(hip.label_pieces_to_numpy(label[1]), h_pieces)
    same(hip.label_infos_to_numpy(label[2]), h_info)
    h_fields, h_info, h_paths = svo.walk_points(POINTS, SIZE, goals=GOALS, path_capacity=PATH)
    same(walk[0].cpu().numpy(), h_fields)
    same(hip.walk_infos_to_numpy(walk[1]), h_info)
    same(walk[2].cpu().numpy().view(np.uint32), h_paths)


def test_contacts(svo):
    import torch

    e = np.zeros(N, dtype=hip.ENTITY_DTYPE)
    e["position"], e["aabb_extents"], e["gravity"], e["max_fall_velocity"] = POINTS, EXTENTS, 9.8, 50.0
    ents = dev(e.view(np.uint8))
    contacts = svo.physics_step(ents, 0.05, 2, want_contacts=True)
    svo.sync()
    tensor(contacts, torch.float32, (N, 6), ents)
    h_contacts = svo.physics_step(e, 0.05, 2, want_contacts=True)
    same(contacts.cpu().numpy().reshape(-1).view(hip.AABB_RESULT_DTYPE), h_contacts)
    assert ents.cpu().numpy().tobytes() == e.tobytes()
