"""vx_raycast_batch and vx_physics_step on the GPU beyond the depth-7 heightfield: the worlds, rays and entities of tests/batch_cases.py
(translucent blocks, a deep world far from the origin with an LOD chunk, borders, boxes sunk into the ground, the 8 x 8 x 8 fan), against
the ORACLE's results, which test_batch_cases_on_host.py has checked to hold every kind of case. Both formats, and the ESVO-BIG kernel
builds (a context of 4 GiB). Every comparison is byte for byte."""
import ctypes as C

import numpy as np
import pytest

from batch_cases import CASES, DT, STEPS, describe_entity, describe_ray, first_difference, make_case, oracle_hits
from gpu_harness import make_context
from helpers import orc, vra  # noqa: F401
from test_raycast_batch import assert_is_picker_result, tasks_of
from voxel_rs_amd import hip, host

pytestmark = pytest.mark.gpu


_cases = {}


@pytest.fixture(scope="module")
def contexts():
    """One context per (world, format) for the whole module, opened when a test first asks for it."""
    open_contexts = {}
    yield open_contexts
    for svo in open_contexts.values():
        svo.close()


def with_context(contexts, name, fmt):
    """A world in one format, its rays and entities and the oracle's results for them (computed once, read-only), and the context that has it."""
    if (name, fmt) not in _cases:
        _cases[name, fmt] = make_case(name, fmt)
    c = _cases[name, fmt]
    if (name, fmt) not in contexts:
        contexts[name, fmt] = make_context(c)
    c.svo = contexts[name, fmt]
    return c


@pytest.fixture(scope="module", params=CASES, ids=[f"{n}-{f}" for n, f in CASES])
def case(request, contexts):
    return with_context(contexts, *request.param)


@pytest.fixture(scope="module", params=["esvo", "csvo"])
def glasshouse_case(request, contexts):
    """(the case fixture's glasshouse, for the tests that run in that world only)"""
    return with_context(contexts, "glasshouse", request.param)


@pytest.fixture(scope="module", params=["esvo", "csvo"])
def far_case(request, contexts):
    return with_context(contexts, "far_chunks", request.param)


def to_device(array):
    import torch

    return torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).copy()).cuda()


def floats_to_device(array):
    import torch

    return torch.from_numpy(np.array(array, dtype=np.float32, order="C")).cuda()


def from_device(tensor, dtype):
    return tensor.cpu().numpy().view(np.uint8).reshape(-1).view(dtype)


def same_rays(c, got, exp, what, idx=None):
    first_difference(got, exp, f"{c.name}-{c.fmt} {what}", lambda i: describe_ray(c, i if idx is None else idx[i]))


def same_entities(c, got, exp, what):
    first_difference(got, exp, f"{c.name}-{c.fmt} {what}", lambda i: describe_entity(c, i))


def check_rays_from_host_memory(c, svo):
    opaque = svo.raycast_batch(c.o, c.d, c.m)
    through = svo.raycast_batch(c.o, c.d, c.m, translucent=True)
    same_rays(c, opaque, c.opaque, "host rays, opaque cast")
    same_rays(c, through, c.through, "host rays, translucent cast")
    differ = sum(opaque[i].tobytes() != through[i].tobytes() for i in range(len(opaque)))
    assert differ >= 150 and differ == c.counts["differ"], differ  # the two kernel builds answer differently where the oracle's casts do
    return opaque


def test_ray_batches_against_the_oracle(case):
    """1: both casts, from host and from device memory; the opaque one is also what vx_raycast says."""
    c, svo = case, case.svo
    opaque = check_rays_from_host_memory(c, svo)
    assert_is_picker_result(opaque, svo.raycast(tasks_of(c.o, c.d, c.m)))
    d_o, d_d, d_m = floats_to_device(c.o), floats_to_device(c.d), floats_to_device(c.m)
    d_opaque = svo.raycast_batch(d_o, d_d, d_m)
    d_through = svo.raycast_batch(d_o, d_d, d_m, translucent=True)
    svo.sync()
    same_rays(c, hip.ray_hits_to_numpy(d_opaque), c.opaque, "device rays, opaque cast")
    same_rays(c, hip.ray_hits_to_numpy(d_through), c.through, "device rays, translucent cast")


def physics_rows_against_the_oracle(c, svo, start):
    """12 single steps from host records, contacts asked for: records and contacts are the oracle-backed step's after every step."""
    e = start.copy()
    big = c.roles["extents"][0]
    for step, (rows, contacts) in enumerate(c.run):
        got = svo.physics_step(e, DT, 1, want_contacts=True).view(np.float32).reshape(-1, 6)
        assert got[big].tobytes() == contacts[big].tobytes(), f"the 8 x 8 x 8 box's contacts at step {step}: {got[big]} != {contacts[big]}"
        same_entities(c, got, contacts, f"contacts of step {step} (host records)")
        same_entities(c, hip.entities_to_rows(e), rows, f"records after step {step} (host records)")


def test_counts_around_the_wave_and_the_pool(glasshouse_case):
    """2: counts of 1, 64, 65 and all with the translucent flag; a host batch of 40,000 rays that grows the shared pinned pool, and directly after it
    a host physics step and a batch of 3 rays."""
    c, svo = glasshouse_case, glasshouse_case.svo
    for count in (1, 64, 65, len(c.o)):
        hits = svo.raycast_batch(np.ascontiguousarray(c.o[:count]), np.ascontiguousarray(c.d[:count]), np.ascontiguousarray(c.m[:count]), translucent=True)
        assert len(hits) == count
        same_rays(c, hits, c.through[:count], f"{count} rays, translucent cast")
    idx = np.arange(40000) % len(c.o)
    o, d, m = (np.ascontiguousarray(a[idx]) for a in (c.o, c.d, c.m))
    many = svo.raycast_batch(o, d, m, translucent=True)
    e = hip.entities_from_rows(c.rows)
    contacts = svo.physics_step(e, DT, 1, want_contacts=True).view(np.float32).reshape(-1, 6)
    three = svo.raycast_batch(np.ascontiguousarray(c.o[:3]), np.ascontiguousarray(c.d[:3]), np.ascontiguousarray(c.m[:3]))
    same_rays(c, many, c.through[idx], "40,000 rays, translucent cast", idx)
    same_entities(c, contacts, c.run[0][1], "contacts of a step after the large batch")
    same_entities(c, hip.entities_to_rows(e), c.run[0][0], "records of a step after the large batch")
    same_rays(c, three, c.opaque[:3], "3 rays after the large batch")


def test_physics_against_the_oracle_alone(case):
    """3: 12 single steps from host and from device records, 12 steps in one call, and a call of no steps."""
    c, svo = case, case.svo
    start = hip.entities_from_rows(c.rows)
    big = c.roles["extents"][0]
    physics_rows_against_the_oracle(c, svo, start)
    d = to_device(start)
    for step, (rows, contacts) in enumerate(c.run):
        dc = svo.physics_step(d, DT, 1, want_contacts=True)
        svo.sync()
        got = from_device(dc, np.float32).reshape(-1, 6)
        assert got[big].tobytes() == contacts[big].tobytes(), f"the 8 x 8 x 8 box's contacts at step {step}: {got[big]} != {contacts[big]}"
        same_entities(c, got, contacts, f"contacts of step {step} (device records)")
        same_entities(c, hip.entities_to_rows(from_device(d, hip.ENTITY_DTYPE)), rows, f"records after step {step} (device records)")
    last_rows, last_contacts = c.run[-1]
    many = start.copy()
    got = svo.physics_step(many, DT, STEPS, want_contacts=True).view(np.float32).reshape(-1, 6)
    assert got[big].tobytes() == last_contacts[big].tobytes(), f"the 8 x 8 x 8 box's contacts after {STEPS} steps in one call"
    same_entities(c, hip.entities_to_rows(many), last_rows, f"records after {STEPS} steps in one call")
    same_entities(c, got, last_contacts, f"contacts of {STEPS} steps in one call")
    d_many = to_device(start)
    dc = svo.physics_step(d_many, DT, STEPS, want_contacts=True)
    svo.sync()
    got = from_device(dc, np.float32).reshape(-1, 6)
    assert got[big].tobytes() == last_contacts[big].tobytes(), f"the 8 x 8 x 8 box's contacts after {STEPS} steps in one call (device records)"
    same_entities(c, hip.entities_to_rows(from_device(d_many, hip.ENTITY_DTYPE)), last_rows, f"records after {STEPS} steps in one call (device records)")
    same_entities(c, got, last_contacts, f"contacts of {STEPS} steps in one call (device records)")
    # no steps: the oracle's contacts at the current position, nothing moves -- at the start and where the steps ended
    for where, e, exp in (("start", start.copy(), c.start_contacts), ("end", many.copy(), c.final_contacts)):
        before = e.copy()
        got = svo.physics_step(e, DT, 0, want_contacts=True).view(np.float32).reshape(-1, 6)
        assert e.tobytes() == before.tobytes()
        assert got[big].tobytes() == exp[big].tobytes(), f"the 8 x 8 x 8 box's contacts of no steps at the {where}"
        same_entities(c, got, exp, f"contacts of no steps at the {where}")
        d0 = to_device(before)
        dc = svo.physics_step(d0, DT, 0, want_contacts=True)
        svo.sync()
        assert from_device(d0, hip.ENTITY_DTYPE).tobytes() == before.tobytes()
        got = from_device(dc, np.float32).reshape(-1, 6)
        assert got[big].tobytes() == exp[big].tobytes(), f"the 8 x 8 x 8 box's contacts of no steps at the {where} (device records)"
        same_entities(c, got, exp, f"contacts of no steps at the {where} (device records)")


def test_the_path_it_replaces(case):
    """4: the same 12 steps through Physics::step_many over vx_raycast (host.physics_step_many): a difference between the two GPU paths
    shows here, a difference to the oracle in the tests above."""
    c, svo = case, case.svo
    ref = c.rows.copy()
    for step, (rows, _) in enumerate(c.run):
        host.physics_step_many(svo._h, DT, 1, ref)
        same_entities(c, ref, rows, f"records after step {step} (step_many over vx_raycast)")
    ref = c.rows.copy()
    host.physics_step_many(svo._h, DT, STEPS, ref)
    same_entities(c, ref, c.run[-1][0], f"records after {STEPS} steps (step_many over vx_raycast)")


def test_a_batch_reads_the_stepped_boxes(far_case):
    """6: far_chunks' entities in device memory: 8 steps and, with no synchronisation in between, a translucent batch looking down from the
    records' positions (stride 64). The hits are the oracle's for the oracle-stepped positions."""
    c, svo = far_case, far_case.svo
    ents = to_device(hip.entities_from_rows(c.rows))
    down = np.float32([0, -1, 0])
    svo.physics_step(ents, DT, 8)
    hits = svo.raycast_batch(hip.entity_positions(ents), floats_to_device(down), 20.0, translucent=True)
    svo.sync()
    stepped = c.run[7][0]
    same_entities(c, hip.entities_to_rows(from_device(ents, hip.ENTITY_DTYPE)), stepped, "records after 8 steps (device records)")
    n = len(stepped)
    exp = oracle_hits(c.scene, stepped[:, 0:3], np.tile(down, (n, 1)), np.full(n, 20.0), True)
    same_entities(c, hip.ray_hits_to_numpy(hits), exp, "hits under the stepped boxes")
    assert (exp["dst"] > 0).sum() >= 8
    assert exp.tobytes() != oracle_hits(c.scene, c.rows[:, 0:3], np.tile(down, (n, 1)), np.full(n, 20.0), True).tobytes()  # (a batch that ran first would say this)


def test_esvo_big():
    """5: the glasshouse in an ESVO context of 4 GiB, which selects the VX_SVO_ESVO_BIG builds of both kernels (runtime.cpp: ctx->big depends on
    the capacity alone): both casts from host memory, and 12 single physics steps from host records, against the same oracle results."""
    c = _cases.get(("glasshouse", "esvo")) or make_case("glasshouse", "esvo")
    h = C.c_void_p()
    rc = hip.lib().vx_create(c.svo_type, 1 << 32, 0, C.byref(h))
    if rc == 3:  # VX_ERR_OUT_OF_MEMORY, from vx_create itself: the one reason to skip
        pytest.skip("vx_create: " + hip.lib().vx_last_error().decode())
    assert rc == 0, hip.lib().vx_last_error()
    svo = hip.Svo.__new__(hip.Svo)
    svo._h, svo.svo_type = h, c.svo_type
    try:
        svo.set_materials(c.mats)
        svo.set_textures(c.tex, 6)
        svo.update_full(c.world)
        assert svo.get_stats()["capacity_bytes"] == 1 << 32
        check_rays_from_host_memory(c, svo)
        physics_rows_against_the_oracle(c, svo, hip.entities_from_rows(c.rows))
    finally:
        svo.close()
