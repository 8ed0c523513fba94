"""The ray and entity sets of tests/batch_cases.py without a GPU: that they hold every kind of case they were built for (by the oracle's
results alone), and that the DEVICE headers, compiled for the host by the test-only harnesses (tests/cpp/device_on_host.cpp,
tests/cpp/physics_on_host.cpp), agree with the oracle on them byte for byte. test_batch_physics_worlds.py runs the same cases through
vx_raycast_batch and vx_physics_step on the GPU."""
import ctypes as C

import numpy as np
import pytest

from batch_cases import CASES, GLASS, STEPS, cut_short, describe_entity, describe_ray, first_difference, make_case, sunk_contact
from helpers import orc
from physics_cases import DT
from test_device_on_host import devhost  # noqa: F401  (the fixture that builds the harness)
from test_physics_device_on_host import host_step, physhost  # noqa: F401
from voxel_rs_amd import hip

_vp = C.c_void_p


@pytest.fixture(scope="module", params=CASES, ids=[f"{n}-{f}" for n, f in CASES])
def case(request):
    return make_case(*request.param)


def test_the_ray_set_holds_every_kind(case):
    """Thresholds as the cases were specified; a seed that misses one is changed, never the threshold."""
    c = case.counts
    cut = {name: cut_short(case.scene, case.o, case.d, case.m, hits, name == "through") for name, hits in (("opaque", case.opaque), ("through", case.through))}
    hits_of = dict(opaque=case.opaque, through=case.through)
    print(f"\n{case.name}-{case.fmt} rays: {c} cut_short={cut}")
    assert 1100 <= c["rays"] <= 1500
    assert c["differ"] >= 150 and c["differ_value"] >= 30 and c["through_glass"] >= 30
    for name in ("opaque", "through"):
        k = c[name]
        assert k["inside_voxel"] >= 100 and k["miss"] >= 100 and k["outside_hit"] >= 60, (name, k)
        assert len(k["values"]) >= 4 and k["faces"] == [0, 1, 2, 3, 4, 5], (name, k)
        odd = (hits_of[name]["dst"] > 0) & ~((hits_of[name]["value"] >= 1) & (hits_of[name]["value"] <= 12))
        assert (hits_of[name]["inside_voxel"][odd] != 0).all() and (case.fmt == "csvo" or not odd.any())  # (ray_counts: the reference's own, from inside voxels)
        assert cut[name] >= 40, (name, cut)
        if case.name == "far_chunks":
            assert k["lod_hits"] >= 20, (name, k)
    assert c["integral"] >= 40
    if case.name == "far_chunks":
        assert c["wander"] >= 100
    # what the builder promises besides: signed zeros, tiny components, every max_dst
    d = case.d
    assert ((d == 0).sum(axis=1) == 1).sum() >= 10 and ((d == 0).sum(axis=1) == 2).sum() >= 10 and (np.signbit(d) & (d == 0)).any()
    assert (np.abs(d) == np.float32(1e-30)).any(axis=1).sum() >= 40
    assert (case.m == -1).sum() >= 100 and (case.m == np.float32(1e-6)).sum() >= 40 and (case.m >= 3e4).sum() >= 40
    size = case.info["size"]
    assert ((case.o == 0) | (case.o == size)).any(axis=1).sum() >= 40
    assert (case.kinds == "between").sum() == 60 and (case.through["dst"][case.kinds == "between"] < 0).all() and (case.opaque["dst"][case.kinds == "between"] > 0).all()


def test_the_entity_set_holds_every_kind(case):
    rows, roles, run = case.rows, case.roles, case.run
    contacts = np.stack([ct for _, ct in run] + [case.final_contacts])  # [step][entity][6]
    kinds = [(int((contacts[:, :, k] >= 0).sum()), int((contacts[:, :, k] == -1).sum())) for k in range(6)]
    last = run[-1][0]
    moved = (last[:, 0:3] != rows[:, 0:3]).any(axis=1)
    print(f"\n{case.name}-{case.fmt} entities: {len(rows)} boxes, roles {roles}, contacts (>= 0, -1) per kind {kinds}, moved {int(moved.sum())}, "
          f"grounded {int((last[:, 16] == 1).sum())}")
    assert all(a >= 1 and b >= 1 for a, b in kinds)
    for i in roles["sunk"]:
        assert sunk_contact(case.info, contacts[0, i]), (i, contacts[0, i])  # (< 2 * 0.0005; at depth 14: one quantum, see sunk_contact)
    a, b = roles["outward"]
    assert case.final_contacts[a, 3] == -1 and case.final_contacts[b, 2] == -1
    assert last[a, 0] > rows[a, 0] and last[b, 2] < rows[b, 2]
    assert all(r[roles["on_glass"][0], 16] == 1.0 for r, _ in run)
    assert (contacts[:4, roles["into_glass"][0], 5] >= 0).all()  # glass is solid for the opaque cast
    assert moved.sum() * 3 >= len(rows)
    assert len(roles["extents"]) == 5 and (rows[:, 12] != 0).sum() >= 2 and (rows[:, 13] != 0).sum() >= 2
    if case.name == "far_chunks":
        assert len(roles["straddle"]) == 1


def scene_arguments(case):
    """The world's frame, the materials and the texture chain as the harnesses' entries take them."""
    frame = np.concatenate([case.world.frame(pad_words=0), np.zeros(4, dtype=np.uint32)])  # (the 16 zero bytes a context keeps behind the world buffer)
    levels = orc.mip_chain(case.tex, 6)
    chain = np.concatenate([lv.ravel() for lv in levels])
    offsets = np.cumsum([0] + [lv.size for lv in levels[:-1]])
    level_offset = (C.c_uint32 * 16)(*[int(v) for v in offsets])
    mats = np.ascontiguousarray(case.mats.view(orc.MATERIAL_DTYPE))
    return frame, mats, chain, len(levels), level_offset


@pytest.mark.parametrize("translucent", [False, True], ids=["opaque", "translucent"])
def test_the_device_traversal_casts_the_rays_as_the_oracle_does(case, devhost, translucent):  # noqa: F811
    """vxd::intersect (vx_device.hpp) on the host over the whole ray set: vx_ray_hit records, byte for byte."""
    frame, mats, chain, n_levels, level_offset = scene_arguments(case)
    o, d, m = (np.array(a, order="C") for a in (case.o, case.d, case.m))
    got = np.zeros(len(o), dtype=hip.RAY_HIT_DTYPE)
    devhost.devhost_ray_batch(case.svo_type, frame.ctypes.data_as(_vp), C.c_uint64(frame.size * 4), mats.ctypes.data_as(_vp), len(mats), chain.ctypes.data_as(_vp),
                              case.tex.shape[2], case.tex.shape[1], case.tex.shape[0], n_levels, level_offset, o.ctypes.data_as(_vp), d.ctypes.data_as(_vp),
                              m.ctypes.data_as(_vp), len(o), int(translucent), got.ctypes.data_as(_vp))
    exp = case.through if translucent else case.opaque
    first_difference(got, exp, f"{case.name}-{case.fmt} translucent={translucent}", lambda i: describe_ray(case, i))


def test_the_device_physics_steps_the_entities_as_the_oracle_does(case, physhost):  # noqa: F811
    """vx_physics.hpp on the host (physhost_step): 12 single steps, records and contacts after every one; 12 steps in one call; no steps."""
    frame, mats, chain, n_levels, level_offset = scene_arguments(case)
    e = hip.entities_from_rows(case.rows)
    what = f"{case.name}-{case.fmt}"
    for step, (rows, contacts) in enumerate(case.run):
        got = np.zeros(len(e), dtype=hip.AABB_RESULT_DTYPE)
        host_step(physhost, case.svo_type, frame, mats, chain, case.tex, n_levels, level_offset, e, DT, 1, got)
        first_difference(got.view(np.float32).reshape(-1, 6), contacts, f"{what} contacts of step {step}", lambda i: describe_entity(case, i))
        first_difference(hip.entities_to_rows(e), rows, f"{what} records after step {step}", lambda i: describe_entity(case, i))
    many = hip.entities_from_rows(case.rows)
    got = np.zeros(len(many), dtype=hip.AABB_RESULT_DTYPE)
    host_step(physhost, case.svo_type, frame, mats, chain, case.tex, n_levels, level_offset, many, DT, STEPS, got)
    first_difference(hip.entities_to_rows(many), case.run[-1][0], f"{what} records after {STEPS} steps in one call", lambda i: describe_entity(case, i))
    first_difference(got.view(np.float32).reshape(-1, 6), case.run[-1][1], f"{what} contacts of {STEPS} steps in one call", lambda i: describe_entity(case, i))
    before = many.copy()
    host_step(physhost, case.svo_type, frame, mats, chain, case.tex, n_levels, level_offset, many, DT, 0, got)
    assert many.tobytes() == before.tobytes()
    first_difference(got.view(np.float32).reshape(-1, 6), case.final_contacts, f"{what} contacts of no steps", lambda i: describe_entity(case, i))


def test_glass_is_in_the_opaque_results(case):
    """(the block id travels with the hit: the opaque cast stops at panes, the translucent cast goes on)"""
    assert (case.opaque["value"] == GLASS).sum() > (case.through["value"] == GLASS).sum()
