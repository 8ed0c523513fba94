"""vx_physics_step on the GPU: entity physics stepped by a kernel of its own (voxel-rs_amd/csrc/physics), against the path it replaces --
systems::Physics::step_many over vx_raycast (host.physics_step_many) -- and against the oracle-backed step. Depth-7 heightfield, both
formats; every comparison is byte for byte."""
import ctypes as C

import numpy as np
import pytest

from helpers import orc, vra  # noqa: F401
from physics_cases import DT, ground_under, heightfield, oracle_step, place_entities, touches_a_wall
from voxel_rs_amd import hip, host

pytestmark = pytest.mark.gpu
_vp = C.c_void_p


class Case:
    pass


@pytest.fixture(scope="module", params=[host.SVO_ESVO, host.SVO_CSVO], ids=["esvo", "csvo"])
def case(request):
    """The world, its oracle scene, a context that has it, and 51 entity rows over it: 48 players' boxes (every seventh with wall_clip,
    three flying) and three boxes of other shapes. Shared and left unchanged: the tests step copies."""
    c = Case()
    c.svo_type = request.param
    c.world, c.scene, tex, mats, c.h_max = heightfield(c.svo_type, 7)
    c.svo = hip.Svo(c.svo_type, c.world.size_in_bytes + (1 << 20))
    c.svo.set_materials(mats)
    c.svo.set_textures(tex, 6)
    c.svo.update(c.world)
    rng = np.random.default_rng(3)
    rows = place_entities(c.scene, rng, 48, 8, 120, c.h_max)
    rows[[5, 17, 29], 13] = 1.0  # flying
    extra = []
    for x, z, ext in ((40.3, 50.6, (2.5, 3.2, 1.3)), (70.2, 33.9, (0.3, 0.3, 0.3)), (90.5, 80.5, (1.0, 2.0, 1.0))):  # 180 slots: three trips; a small box; whole blocks
        off = (-ext[0] / 2, 0.0, -ext[2] / 2)
        y = ground_under(c.scene, x, z, c.h_max + 4.0, off, ext) + 1.5
        r = host.make_entities([(x, y, z)], extents=ext, offset=off)
        r[0, 3], r[0, 5] = 5.0, -4.0
        extra.append(r)
    c.rows = np.concatenate([rows] + extra)
    c.rows.setflags(write=False)
    yield c
    c.svo.close()


def aabbs_of(rows):
    return [dict(pos=e[0:3], offset=e[6:9], extents=e[9:12]) for e in rows]


def picker_contacts(svo, rows):
    """The AabbResults of the rows' boxes through vx_raycast: PickerBatch::serialize_tasks -> Svo::raycast -> deserialize_results."""
    a = aabbs_of(rows)
    return host.picker_deserialize([], a, svo.raycast(host.picker_serialize([], a)))[1]


def to_device(array):
    import torch

    return torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).copy()).cuda()


def from_device(tensor, dtype):
    return tensor.cpu().numpy().view(np.uint8).reshape(-1).view(dtype)


def test_one_step_per_call_against_the_existing_path(case):
    """6.3"""
    svo = case.svo
    e = hip.entities_from_rows(case.rows)
    ref = case.rows.copy()
    sub = [0, 1, 2, 3, 5, 6, 7, 8, 14, 48, 49, 50]  # wall_clip, flying and the three other boxes among them
    orc_rows = case.rows[sub].copy()
    wall = False
    for step in range(150):
        ref_contacts = picker_contacts(svo, ref)
        contacts = svo.physics_step(e, DT, 1, want_contacts=True)
        host.physics_step_many(svo._h, DT, 1, ref)
        assert hip.entities_to_rows(e).tobytes() == ref.tobytes(), f"entity states diverge at step {step}"
        assert contacts.tobytes() == np.ascontiguousarray(ref_contacts, dtype=np.float32).tobytes(), f"contacts diverge at step {step}"
        wall = wall or touches_a_wall(ref_contacts, ref)
        if step < 20:
            oracle_step(case.scene, DT, orc_rows)
            assert ref[sub].tobytes() == orc_rows.tobytes(), f"the oracle-backed step diverges at step {step}"
    # the reference side alone: landed, and met a wall
    assert (ref[:, 16] == 1.0).sum() >= len(ref) // 2 and wall
    assert (ref[[5, 17, 29], 16] == 0.0).all() and (ref[[5, 17, 29], 4] == 0.0).all()  # flying: no gravity


def test_many_steps_in_one_call(case):
    """6.4: steps = 25 in one call = 25 calls of one step, in host and in device memory (there: everything enqueued back to back, one
    vx_sync before reading); the contacts are the last single step's."""
    svo = case.svo
    start = hip.entities_from_rows(case.rows)
    one, many = start.copy(), start.copy()
    for _ in range(25):
        last = svo.physics_step(one, DT, 1, want_contacts=True)
    contacts = svo.physics_step(many, DT, 25, want_contacts=True)
    assert many.tobytes() == one.tobytes() and contacts.tobytes() == last.tobytes()
    assert (many["position"] != start["position"]).any()
    d_many, d_one = to_device(start), to_device(start)
    c_many = svo.physics_step(d_many, DT, 25, want_contacts=True)
    for _ in range(25):
        c_one = svo.physics_step(d_one, DT, 1, want_contacts=True)
    svo.sync()
    assert from_device(d_many, hip.ENTITY_DTYPE).tobytes() == one.tobytes() and from_device(d_one, hip.ENTITY_DTYPE).tobytes() == one.tobytes()
    assert from_device(c_many, hip.AABB_RESULT_DTYPE).tobytes() == last.tobytes() and from_device(c_one, hip.AABB_RESULT_DTYPE).tobytes() == last.tobytes()
    # ... and the path it replaces, 25 steps of it
    ref = case.rows.copy()
    host.physics_step_many(svo._h, DT, 25, ref)
    assert hip.entities_to_rows(many).tobytes() == ref.tobytes()


def test_no_steps_is_an_aabb_distance_query(case):
    """6.5"""
    svo = case.svo
    e = hip.entities_from_rows(case.rows)
    svo.physics_step(e, DT, 40)  # (some on the ground, some in the air)
    before = e.copy()
    exp = np.ascontiguousarray(picker_contacts(svo, hip.entities_to_rows(e)), dtype=np.float32)
    contacts = svo.physics_step(e, DT, 0, want_contacts=True)
    assert e.tobytes() == before.tobytes() and contacts.tobytes() == exp.tobytes()
    assert (exp == -1).any() and (exp > 0).any()
    d = to_device(e)
    dc = svo.physics_step(d, DT, 0, want_contacts=True)
    svo.sync()
    assert from_device(d, hip.ENTITY_DTYPE).tobytes() == before.tobytes() and from_device(dc, hip.AABB_RESULT_DTYPE).tobytes() == exp.tobytes()
    # raw device pointers with their count, as an embedder without torch passes them
    import torch

    d2, dc2 = to_device(e), torch.zeros((len(e), 6), dtype=torch.float32, device="cuda")
    assert svo.physics_step(d2.data_ptr(), DT, 3, want_contacts=True, count=len(e), contacts=dc2.data_ptr()) == dc2.data_ptr()
    svo.sync()
    three = e.copy()
    c3 = svo.physics_step(three, DT, 3, want_contacts=True)
    assert from_device(d2, hip.ENTITY_DTYPE).tobytes() == three.tobytes() and from_device(dc2, hip.AABB_RESULT_DTYPE).tobytes() == c3.tobytes()
    with pytest.raises(TypeError):
        svo.physics_step(d2.data_ptr(), DT, 1)  # no count
    with pytest.raises(TypeError):
        svo.physics_step(d2.data_ptr(), DT, 1, want_contacts=True, count=len(e))  # nowhere to put the contacts
    assert svo.physics_step(np.zeros(0, dtype=hip.ENTITY_DTYPE), DT, 3) is None  # count == 0


def test_records_that_cannot_be_stepped(case):
    """6.6"""
    svo = case.svo
    e = hip.entities_from_rows(case.rows[:12])
    bad = {2: 0.0, 6: np.nan, 9: 9.5}
    for i, v in bad.items():
        e["aabb_extents"][i, 1] = v
    good = [i for i in range(len(e)) if i not in bad]
    exp = case.rows[:12][good].copy()
    host.physics_step_many(svo._h, DT, 10, exp)
    d = to_device(e)
    dc = svo.physics_step(d, DT, 10, want_contacts=True)
    svo.sync()
    got, contacts = from_device(d, hip.ENTITY_DTYPE), from_device(dc, hip.AABB_RESULT_DTYPE)
    for i in bad:
        assert got[i].tobytes() == e[i].tobytes(), i
        assert contacts[i].tobytes() == np.full(6, -1, dtype=np.float32).tobytes(), i
    assert hip.entities_to_rows(got[good]).tobytes() == exp.tobytes()
    before = e.copy()
    out = np.full(len(e), 7.0, dtype=hip.AABB_RESULT_DTYPE)
    rc = hip.lib().vx_physics_step(svo._h, e.ctypes.data_as(_vp), len(e), hip.VX_MEM_HOST, float(DT), 10, out.ctypes.data_as(_vp))
    assert rc == 1 and b"entity 2 " in hip.lib().vx_last_error()
    assert e.tobytes() == before.tobytes() and (out["neg"] == 7.0).all() and (out["pos"] == 7.0).all()
    with pytest.raises(hip.VoxelHipError):
        svo.physics_step(e, DT, 1)


def test_a_world_change_between_calls(case):
    """6.7: a step enqueued before a commit sees the world as it was, one enqueued after it the new world -- the ground gone under an
    entity that stood on it. Run last: it edits the module's world."""
    svo, world = case.svo, case.world
    e = hip.entities_from_rows(case.rows)
    svo.physics_step(e, DT, 150)
    rows = hip.entities_to_rows(e)
    inside = lambda v: 3.0 < v % 32.0 < 29.0  # noqa: E731  (the whole box over one chunk)
    g = next(i for i in range(48) if rows[i, 16] == 1.0 and rows[i, 12] == 0.0 and inside(rows[i, 0]) and inside(rows[i, 2]) and rows[i, 1] < 31.0)
    exp_old = rows.copy()
    host.physics_step_many(svo._h, DT, 8, exp_old)
    d_old, d_new = to_device(e), to_device(e)
    svo.physics_step(d_old, DT, 8)  # enqueued; the commit below has to wait for it on the device
    cx, cz = int(rows[g, 0] // 32), int(rows[g, 2] // 32)
    chunk = vra.Chunk(cx, 0, cz, 5)
    chunk.set_block(0, 0, 0, 1)  # (not quite empty)
    chunk.compact()
    world.set_chunk((cx, 0, cz), chunk)
    world.serialize()
    svo.update(world)
    svo.physics_step(d_new, DT, 8)  # enqueued behind the commit's uploads
    svo.sync()
    exp_new = rows.copy()
    host.physics_step_many(svo._h, DT, 8, exp_new)
    assert hip.entities_to_rows(from_device(d_old, hip.ENTITY_DTYPE)).tobytes() == exp_old.tobytes()
    assert hip.entities_to_rows(from_device(d_new, hip.ENTITY_DTYPE)).tobytes() == exp_new.tobytes()
    assert exp_old[g, 16] == 1.0 and exp_new[g, 16] == 0.0 and exp_new[g, 1] < exp_old[g, 1]
