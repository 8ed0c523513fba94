"""What the GPU tests of the block entry points (tests/test_blocks.py to tests/test_distance.py) share: the context of a case and the two
special ones (4 GiB; no traversal image), the sentinel-filled device buffers and the two checks of what a call left of them, the cache of a
module's cases, the frame of test_errors_leave_the_output_alone and the entities of test_behind_physics_step. Each module keeps its calls,
its picks, its table of refusals and every assertion about a call's results. torch is imported inside the functions: collection needs no GPU."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from abi_checks import refusing
from voxel_rs_amd import hip

SENTINEL = 0x5A5A5A5A
TAIL = 48  # bytes behind the last field a call may write to, which it has to leave alone


def make_context(c, world=None, capacity=None):
    """A context of the case's format with its materials and textures that holds `world` (default: the case's) whole."""
    world = c.world if world is None else world
    svo = hip.Svo(c.svo_type, world.size_in_bytes + (1 << 20) if capacity is None else capacity)
    svo.set_materials(c.mats)
    svo.set_textures(c.tex, 6)
    svo.update_full(world)
    return svo


@contextlib.contextmanager
def big_esvo_context(c):
    """The case's world in a context of 4 GiB, which selects the VX_SVO_ESVO_BIG builds of the kernels (runtime.cpp: ctx->big depends on the
    capacity alone). VX_ERR_OUT_OF_MEMORY from vx_create itself is the one reason to skip."""
    h = C.c_void_p()
    rc = hip.lib().vx_create(c.svo_type, 1 << 32, 0, C.byref(h))
    if rc == 3:
        pytest.skip("vx_create: " + hip.lib().vx_last_error().decode())
    assert rc == 0, hip.lib().vx_last_error()
    svo = hip.Svo.__new__(hip.Svo)
    svo._h, svo.svo_type = h, c.svo_type
    try:
        svo.set_materials(c.mats)
        svo.set_textures(c.tex, 6)
        svo.update_full(c.world)
        assert svo.get_stats()["capacity_bytes"] == 1 << 32
        yield svo
    finally:
        svo.close()


@contextlib.contextmanager
def no_image_context(c, monkeypatch):
    """A context of the case's world created under VX_TRAVERSAL_IMAGE=0 (read when a context is created): it has no traversal image."""
    monkeypatch.setenv("VX_TRAVERSAL_IMAGE", "0")
    svo = make_context(c)
    try:
        assert svo.image_info()["layout"] == 0
        yield svo
    finally:
        svo.close()


def sentinel_bytes(count, stride, device="cuda"):
    """`count` fields at `stride` bytes and the tail, every byte 0x5a."""
    import torch

    return torch.full((count * stride + TAIL,), 0x5A, dtype=torch.uint8, device=device)


def sentinel_words(rows, width, device="cuda"):
    """`rows` records of `width` sentinel words, and two records more."""
    import torch

    return torch.full((rows + 2, width), SENTINEL, dtype=torch.int32, device=device)


def to_device(array):
    import torch

    return torch.from_numpy(np.array(array, order="C")).cuda()  # (a copy: the shared arrays are read-only)


def field_rows(fields, count, stride, written, what):
    """Of a sentinel_bytes buffer a call has written `count` fields into: the first `written` bytes of each; the rest of every row and all
    that lies behind the last row must still be 0x5a."""
    raw = fields.cpu().numpy()
    rows = raw[:count * stride].reshape(count, stride)
    assert (rows[:, written:] == 0x5A).all() and (raw[count * stride:] == 0x5A).all(), what
    return rows[:, :written]


def records_head(raw_records, count, what):
    """Of a sentinel_words buffer (the tensor, or its records as numpy has them) a call has written `count` records into: those; all that
    lies behind them must still be sentinel words."""
    raw = raw_records.cpu().numpy() if hasattr(raw_records, "cpu") else raw_records
    assert (raw[count:].view(np.uint32) == SENTINEL).all(), what
    return raw[:count]


def shared_cases(build, params):
    """(the_case, _contexts, case) for a module to bind to these names: the_case(name, fmt) is build(name, fmt) -- the world, the picks, the
    host program's bytes and, as c.svo, a context --, made once; _contexts, autouse, closes every context when the module is done; `case` runs
    a test on each of `params`."""
    cases = {}

    def the_case(name, fmt):
        if (name, fmt) not in cases:
            cases[name, fmt] = build(name, fmt)
        return cases[name, fmt]

    @pytest.fixture(scope="module", autouse=True)
    def _contexts():
        yield
        for c in cases.values():
            c.svo.close()
        cases.clear()

    @pytest.fixture(scope="module", params=params, ids=[f"{n}-{f}" for n, f in params])
    def case(request):
        return the_case(*request.param)

    return the_case, _contexts, case


def leaves_the_outputs_alone(case, outputs, device_outputs, refusals, uncommitted, nothing_to_do=()):
    """The frame of test_errors_leave_the_output_alone. Each (call, word) of `refusals` returns VX_ERR_INVALID_ARGUMENT with `word` in the
    message; each call of `uncommitted`, given a context that holds no world, VX_ERR_STATE; each of `nothing_to_do` (count == 0) VX_OK. After
    every one the sentinel-filled `outputs` (numpy) are as they were, and after a vx_sync so are `device_outputs` (torch)."""
    L = hip.lib()
    unchanged = refusing(L, lambda call: call(), outputs)
    for call, word in refusals:
        unchanged(word, call)
    sentinel = b"".join(o.tobytes() for o in outputs)
    fresh = hip.Svo(case.svo_type, 1 << 20)
    try:
        for call in uncommitted:
            assert call(fresh._h) == 6 and b"committed" in L.vx_last_error()
        assert b"".join(o.tobytes() for o in outputs) == sentinel
    finally:
        fresh.close()
    for call in nothing_to_do:
        assert call() == 0
    case.svo.sync()
    assert b"".join(o.tobytes() for o in outputs) == sentinel
    for d in device_outputs:
        assert (d.cpu().numpy().view(np.uint8) == 0x5A).all()


def above_the_blocks(c, count, rng, low, high):
    """`count` positions over columns of the case's dense array that hold a block, `low` to `high` above the column's highest one: `rng`'s
    next draws, a column and a height in turn."""
    t = c.truth
    top = np.where((t != 0).any(axis=1), t.shape[1] - 1 - (t[:, ::-1, :] != 0).argmax(axis=1), -1)  # [x][z]: the highest block
    held = np.argwhere(top >= 0)
    positions = np.zeros((count, 3))
    for k in range(count):
        x, z = (int(v) for v in held[rng.integers(len(held))])
        positions[k] = c.info["lo"] + (x + 0.5, top[x, z] + 1 + rng.uniform(low, high), z + 0.5)
    return positions


def flying_entities(count, positions, rng):
    """`count` vx_entity records at `positions` that fly -- no gravity, no collision -- down at 40 voxels a second and sideways at up to 30;
    the sideways velocities are `rng`'s next draws."""
    e = np.zeros(count, dtype=hip.ENTITY_DTYPE)
    e["position"] = positions
    e["velocity"] = np.stack([rng.uniform(-30, 30, count), np.full(count, -40.0), rng.uniform(-30, 30, count)], axis=1)
    e["aabb_offset"], e["aabb_extents"] = (-0.4, 0.0, -0.4), (0.8, 1.8, 0.8)
    e["gravity"], e["max_fall_velocity"], e["flags"] = 20.0, 50.0, hip.ENTITY_FLYING
    return e
