"""vx_physics_step without a GPU: the DEVICE physics header (voxel-rs_amd/csrc/physics/vx_physics.hpp) compiled for the host by a test-only
harness (tests/cpp/physics_on_host.cpp, the shims of tests/cpp/shims/hip_on_host.hpp) -- the fan's slots against PickerBatch::serialize_tasks,
the update against Physics::update_entity, whole steps against the oracle-backed step -- and the entry point's argument checks. Every
comparison is byte for byte."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from helpers import ROOT, orc, vra  # noqa: F401
from physics_cases import DT, heightfield, oracle_step, place_entities, touches_a_wall
from voxel_rs_amd import hip, host

BUILD = Path(ROOT) / "tests" / "_build"
_vp = C.c_void_p


@pytest.fixture(scope="module")
def physhost():
    BUILD.mkdir(exist_ok=True)
    so = BUILD / "libphysics_on_host.so"
    deps = [Path(ROOT) / "tests" / "cpp" / "physics_on_host.cpp", Path(ROOT) / "voxel-rs_amd" / "csrc" / "physics" / "vx_physics.hpp",
            Path(ROOT) / "voxel-rs_amd" / "csrc" / "physics" / "vx_physics_rules.h",
            Path(ROOT) / "voxel-rs_amd" / "csrc" / "hip" / "vx_device.hpp", Path(ROOT) / "voxel-rs_amd" / "csrc" / "hip" / "vx_args.hpp",
            Path(ROOT) / "tests" / "cpp" / "shims" / "vx_platform.hpp", Path(ROOT) / "tests" / "cpp" / "shims" / "hip_on_host.hpp",
            Path(ROOT) / "include" / "voxel_hip.h"]
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        # tests/cpp/shims comes first: its vx_platform.hpp (plain C++) is found instead of the product's (gfx950 built-ins)
        cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", f"-I{ROOT}/include", f"-I{ROOT}/tests/cpp/shims",
               f"-I{ROOT}/voxel-rs_amd/csrc/hip", f"-I{ROOT}/voxel-rs_amd/csrc/physics", str(deps[0]), "-o", str(so)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    lib = C.CDLL(str(so))
    lib.physhost_fan.restype = C.c_uint32
    lib.physhost_sizes.restype = C.c_uint32
    return lib


def fan_of(lib, pos, offset, extents):
    e = hip.entities_from_rows(host.make_entities([pos], extents=extents, offset=offset))
    slots = C.c_uint32(0)
    n = lib.physhost_fan(e.ctypes.data_as(_vp), None, 0, C.byref(slots))
    out = np.zeros(n, dtype=host.PICKER_TASK_DTYPE)
    assert lib.physhost_fan(e.ctypes.data_as(_vp), out.ctypes.data_as(_vp), n, C.byref(slots)) == n
    return out, slots.value


def test_fan_slots_are_the_reference_tasks(physhost):
    """6.1(a): the live slots' (pos, dir, max_dst) are Aabb::generate_picker_tasks' tasks bit for bit, as a multiset."""
    rng = np.random.default_rng(11)
    boxes = [((10.3, 20.7, 30.1), (-0.4, 0.0, -0.4), (0.8, 1.8, 0.8)), ((5.5, 6.25, 7.125), (-0.5, 0.0, -0.5), (1.0, 2.0, 1.0)),
             ((3.1, 4.1, 5.9), (-0.15, 0.0, -0.15), (0.3, 0.3, 0.3)), ((40.7, 9.3, 11.9), (-4.0, 0.0, -4.0), (8.0, 8.0, 8.0)),
             ((17.2, 3.4, 9.9), (-1.25, 0.0, -0.65), (2.5, 3.2, 1.3)), ((1.0, 2.0, 3.0), (0.0, 0.0, 0.0), (2.0, 0.3, 1.0))]
    for _ in range(200):
        ext = rng.uniform(0.05, 4.5, 3)
        if rng.random() < 0.3:
            ext[rng.integers(0, 3)] = float(rng.integers(1, 5))  # whole blocks: ceil(extent) == extent
        boxes.append((tuple(rng.uniform(0, 120, 3)), tuple(-ext / 2 * [1, 0, 1]), tuple(ext)))
    trips = set()
    for pos, offset, extents in boxes:
        got, slots = fan_of(physhost, pos, offset, extents)
        exp = host.picker_serialize([], [dict(pos=np.float32(pos), offset=np.float32(offset), extents=np.float32(extents))])
        b = [int(np.ceil(np.float32(x))) for x in extents]
        assert slots == 3 * (b[0] + 1) * (b[1] + 1) * (b[2] + 1)
        assert len(got) == len(exp), (extents, len(got), len(exp))
        assert sorted(t.tobytes() for t in got) == sorted(t.tobytes() for t in exp), extents
        assert (got["max_dst"] == 10.0).all()
        trips.add((slots + 63) // 64)
    got, slots = fan_of(physhost, (0, 0, 0), (-0.4, 0, -0.4), (0.8, 1.8, 0.8))
    assert (slots, len(got)) == (36, 32)  # the player's box: one trip
    got, slots = fan_of(physhost, (0, 0, 0), (0, 0, 0), (2.5, 3.2, 1.3))
    assert slots == 180
    assert {1, 2, 3} <= trips and max(trips) >= 30  # one trip, several, and the 8.0 limit's 2187 slots


def test_steppable_is_the_documented_rule(physhost):
    """vxp::steppable_extents (vx_physics_rules.h): the one statement of the rule, which the kernel and the runtime's check of host records
    both call."""
    for ext, ok in (((0.8, 1.8, 0.8), 1), ((8.0, 8.0, 8.0), 1), ((0.0, 1.0, 1.0), 0), ((1.0, np.nan, 1.0), 0), ((1.0, 1.0, 9.5), 0), ((1.0, np.inf, 1.0), 0),
                    ((-1.0, 1.0, 1.0), 0), ((1e-30, 1.0, 1.0), 1)):
        e = hip.entities_from_rows(host.make_entities([(1, 2, 3)], extents=ext))
        assert physhost.physhost_steppable(e.ctypes.data_as(_vp)) == ok, ext


def test_update_is_update_entity(physhost):
    """6.1(b): the device update against Physics::update_entity + apply_axial_physics (csrc/host/physics.hpp) on seeded inputs that hold
    every branch."""
    rng = np.random.default_rng(5)
    n = 2000
    rows = host.make_entities(rng.uniform(0, 100, (n, 3)).astype(np.float32))
    rows[:, 3:6] = rng.uniform(-8, 8, (n, 3))
    rows[:, 4] = rng.uniform(-30, 10, n)
    rows[0::9, 3] = 0.0
    rows[1::9, 3] = -0.0
    rows[2::9, 5] = -0.0
    rows[3::9, 4] = 0.24  # gravity * dt takes it to about zero
    rows[4::11, 4] = -rows[4::11, 15]  # already at -max_fall_velocity
    rows[5::11, 15] = 20.0
    rows[5::11, 4] = -20.0
    rows[::7, 12] = 1.0   # wall_clip
    rows[::13, 13] = 1.0  # flying
    contacts = np.empty((n, 6), dtype=np.float32)
    kind = rng.integers(0, 4, (n, 6))
    contacts[...] = np.where(kind == 0, -1.0, np.where(kind == 1, rng.uniform(0, 0.001, (n, 6)), np.where(kind == 2, rng.uniform(0.001, 0.04, (n, 6)),
                                                                                                      rng.uniform(0.04, 10, (n, 6)))))
    dt = DT
    moved = rows[:, 3:6] * dt
    chosen = np.where(moved > 0, contacts[:, 3:6], contacts[:, 0:3])
    # the branches the inputs must hold
    assert (chosen == -1).any() and ((chosen >= 0) & (chosen < 0.001)).any() and ((chosen >= 0.001) & (np.abs(moved) > chosen)).any()
    assert (rows[:, 3].view(np.uint32) == 0).any() and (rows[:, 3].view(np.uint32) == 0x80000000).any()
    assert (rows[:, 13] != 0).any() and (rows[:, 12] != 0).any() and (rows[:, 4] == -rows[:, 15]).any() and (contacts[:, 1] == -1).any()
    exp = rows.copy()
    host.physics_update(dt, exp, contacts)
    e = hip.entities_from_rows(rows)
    c = np.ascontiguousarray(contacts).view(hip.AABB_RESULT_DTYPE).reshape(n)
    physhost.physhost_update(C.c_float(dt), e.ctypes.data_as(_vp), c.ctypes.data_as(_vp), n)
    got = hip.entities_to_rows(e)
    bad = [i for i in range(n) if got[i].tobytes() != exp[i].tobytes()]
    assert not bad, (len(bad), bad[:5], got[bad[0]], exp[bad[0]], contacts[bad[0]])
    assert 0 < (exp[:, 16] == 1.0).sum() < n and (exp[:, 0:3] != rows[:, 0:3]).any()


def host_step(lib, svo_type, frame, mats, tex_chain, tex, levels, level_offset, e, dt, steps, contacts):
    lib.physhost_step(svo_type, frame.ctypes.data_as(_vp), C.c_uint64(frame.size * 4), mats.ctypes.data_as(_vp), len(mats), tex_chain.ctypes.data_as(_vp),
                      tex.shape[2], tex.shape[1], tex.shape[0], levels, level_offset, e.ctypes.data_as(_vp), len(e), C.c_float(dt), steps,
                      contacts.ctypes.data_as(_vp) if contacts is not None else None)


@pytest.mark.parametrize("svo_type", [host.SVO_ESVO, host.SVO_CSVO])
def test_whole_steps_on_the_host_match_the_oracle_backed_step(physhost, svo_type):
    """6.1(c): 16 entities, 60 steps over the depth-6 heightfield; the 64 lanes are played by a loop (every live slot through vxd::intersect,
    the min fold, the butterfly, the update). Records and contacts equal the oracle-backed step's after every step."""
    world, scene, tex, mats, h_max = heightfield(svo_type, 6)
    rng = np.random.default_rng(5)  # (seed 3 lands 6 of the 16 within 60 steps -- a fall of more than 1.7 blocks takes longer --, seed 5 lands 13)
    ref = place_entities(scene, rng, 16, 6, 58, h_max)
    e = hip.entities_from_rows(ref)
    frame = np.concatenate([world.frame(pad_words=0), np.zeros(4, dtype=np.uint32)])  # (the 16 zero bytes a context keeps behind the world buffer)
    levels = orc.mip_chain(tex, 6)
    chain = np.concatenate([lv.ravel() for lv in levels])
    offsets = np.cumsum([0] + [lv.size for lv in levels[:-1]])
    level_offset = (C.c_uint32 * 16)(*[int(o) for o in offsets])
    m = np.ascontiguousarray(mats.view(orc.MATERIAL_DTYPE))
    wall = False
    for step in range(60):
        contacts = np.zeros(len(e), dtype=hip.AABB_RESULT_DTYPE)
        host_step(physhost, svo_type, frame, m, chain, tex, len(levels), level_offset, e, DT, 1, contacts)
        ref_contacts = oracle_step(scene, DT, ref)
        assert contacts.tobytes() == np.ascontiguousarray(ref_contacts, dtype=np.float32).tobytes(), f"contacts diverge at step {step}"
        assert hip.entities_to_rows(e).tobytes() == ref.tobytes(), f"entity states diverge at step {step}"
        wall = wall or touches_a_wall(ref_contacts, ref)
    # the reference run alone: it has to have landed and to have met a wall for the above to mean something
    assert (ref[:, 16] == 1.0).sum() >= 8 and wall
    # steps = 0: nothing moves, the contacts are the fan's at the current position; steps = 5 in one call = five calls
    before = e.copy()
    contacts = np.zeros(len(e), dtype=hip.AABB_RESULT_DTYPE)
    host_step(physhost, svo_type, frame, m, chain, tex, len(levels), level_offset, e, DT, 0, contacts)
    assert e.tobytes() == before.tobytes()
    five = e.copy()
    host_step(physhost, svo_type, frame, m, chain, tex, len(levels), level_offset, five, DT, 5, None)
    for _ in range(5):
        oracle_step(scene, DT, ref)
    assert hip.entities_to_rows(five).tobytes() == ref.tobytes()


def test_abi_without_a_device():
    """6.2: the entry point's argument checks need no device, and the records have the ABI's sizes."""
    L = hip.lib()
    e = np.zeros(2, dtype=hip.ENTITY_DTYPE)
    assert hip.ENTITY_DTYPE.itemsize == 64 and hip.AABB_RESULT_DTYPE.itemsize == 24
    assert L.vx_physics_step(None, e.ctypes.data_as(_vp), 2, hip.VX_MEM_HOST, 0.004, 1, None) == 1 and b"null context" in L.vx_last_error()
    assert L.vx_physics_step(None, e.ctypes.data_as(_vp), 2, hip.VX_MEM_HOST, 0.004, 1025, None) == 1 and b"1024" in L.vx_last_error()
    assert L.vx_physics_step(None, e.ctypes.data_as(_vp), 2, 7, 0.004, 1, None) == 1 and b"VX_MEM" in L.vx_last_error()
    assert L.vx_physics_step(None, e.ctypes.data_as(_vp), (1 << 24) + 1, hip.VX_MEM_HOST, 0.004, 1, None) == 1 and b"16777216" in L.vx_last_error()
    assert L.vx_physics_step(None, e.ctypes.data_as(_vp), 1 << 24, hip.VX_MEM_HOST, 0.004, 1024, None) == 1 and b"null context" in L.vx_last_error()  # (both at their limits)


def test_record_sizes_in_the_device_build(physhost):
    assert physhost.physhost_sizes() == (64 << 16 | 24)


def test_entity_rows_round_trip():
    rows = host.make_entities([(1, 2, 3), (4, 5, 6), (7, 8, 9)], extents=(1.0, 2.0, 1.0))
    rows[0, 12], rows[1, 13], rows[2, 16] = 1.0, 1.0, 1.0
    rows[:, 3:6] = [[1, -2, 3], [-0.0, 0.5, 0], [6, 6, -6]]
    e = hip.entities_from_rows(rows)
    assert list(e["flags"]) == [1, 2, 0] and list(e["grounded"]) == [0, 0, 1]
    assert hip.entities_to_rows(e).tobytes() == rows.tobytes()
