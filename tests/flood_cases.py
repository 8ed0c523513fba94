"""Shared by the tests of vx_flood_points (test_flood_abi.py, test_flood_on_host.py, test_flood.py): scan_cases.py's three worlds in both
formats and a fourth, `burrow`, built here -- one solid chunk with a serpentine corridor longer than VX_FLOOD_MAX_STEPS, a sealed room, a sealed
single cell and a corridor whose only exit is a block of id 9 --, the positions of each -- a seeded set of 500 and the named ones --, the forms
they are handed over in (packed, at stride 16, vx_entity records), the shapes and step limits, and the expected field and record of every query:
plain numpy over blocks_cases.dense_region of the query's box, a breadth-first flood by shifted ORs of boolean arrays for a whole batch at once
(a query leaves the batch when its frontier is empty), with the record read off the field. The flood is run once per shape and flag to
VX_FLOOD_MAX_STEPS; a smaller step limit's field is that field with the larger step counts turned into VX_FLOOD_UNREACHED -- what a
breadth-first search cut short gives. Nothing of the code under test is used. Also the runner of the host harness
(tests/cpp/flood_on_host.cpp), a stand-alone program, plain and built with sanitizers."""

import numpy as np

from batch_cases import _chunk_of
from blocks_cases import dense_region
from host_harness import HostRunner, build_harness, outputs_differing
from helpers import vra
from scan_cases import SCAN_CASES, ScanCase, make_scan_case, start_of
from voxel_rs_amd import hip, host

NO_POSITION, UNREACHED, BLOCKED, INVALID = hip.VX_FLOOD_NO_POSITION, hip.VX_FLOOD_UNREACHED, hip.VX_FLOOD_BLOCKED, hip.VX_FLOOD_INVALID
MAX_STEPS, SEED_ALWAYS = hip.VX_FLOOD_MAX_STEPS, hip.VX_FLOOD_SEED_ALWAYS
FLOOD_CASES = SCAN_CASES + [("burrow", "esvo"), ("burrow", "csvo")]
FLOOD_SEED = {"glasshouse": 81, "far_chunks": 82, "tower": 83, "burrow": 84}
SEEDED = 500
FORMS = ("packed", "stride16", "entities")
STEP_LIMITS = (0, 1, 24, 250)
STONE, DOOR = 3, 9
BURROW_AT = 32  # the chunk (1, 1, 1) spans [32, 64) on every axis


class Shape:
    """A vx_flood_shape without its step limit, pass_value and flags. snap: the positions are moved to the same place in their 8-cell, so that
    lo % 8 == 4 on every axis whatever the position (9^3: two bricks an axis)."""

    def __init__(self, name, size, seed_at, snap=False):
        self.name, self.size, self.seed_at, self.snap = name, tuple(size), tuple(seed_at), snap
        self.voxels = size[0] * size[1] * size[2]
        self.padded = (self.voxels + 15) // 16 * 16


SHAPES = [Shape("1", (1, 1, 1), (0, 0, 0)), Shape("17", (17, 17, 17), (8, 8, 8)), Shape("9_two_bricks", (9, 9, 9), (4, 4, 4), snap=True),
          Shape("32", (32, 32, 32), (16, 16, 16)), Shape("31x3x17_corner", (31, 3, 17), (30, 2, 0)), Shape("32x1x1", (32, 1, 1), (5, 0, 0))]
SHAPE = {s.name: s for s in SHAPES}


# ---- the fourth world ----------------------------------------------------------------------------------------------------------------------


def burrow_blocks():
    """The chunk's blocks [x][y][z], solid but for: the serpentine on layer y = 4 -- 15 rows of 30 cells along x at z = 1, 3, ..., 29, joined at
    alternating ends: 464 cells, 463 steps end to end --, the room x, y, z in 4..6, 12..14, 4..6, the cell (20, 12, 20), and the corridor at
    y = 20, z = 10: x = 5..9 and x = 11..14 of air with the door, a block of id 9, at x = 10 between them."""
    b = np.full((32, 32, 32), STONE, dtype=np.uint32)
    for k in range(15):
        b[1:31, 4, 1 + 2 * k] = 0
        if k < 14:
            b[30 if k % 2 == 0 else 1, 4, 2 + 2 * k] = 0
    b[4:7, 12:15, 4:7] = 0
    b[20, 12, 20] = 0
    b[5:15, 20, 10] = 0
    b[10, 20, 10] = DOOR
    return b


BURROW_NAMED = {"serpentine_start": (1, 4, 1), "serpentine_end": (30, 4, 29), "room": (5, 13, 5), "cell": (20, 12, 20), "corridor": (7, 20, 10),
                "behind_door": (13, 20, 10), "in_rock": (16, 16, 16)}


def burrow(svo_type):
    from voxel_rs_amd import scenes

    c = ScanCase()
    b = burrow_blocks()
    # (the chunk alone gives the smallest world that holds it: depth 6; the empty far corner chunk of a depth-7 world cannot be stated, so a
    # single block at (3, 3, 3) * 32 makes the world span [0, 128))
    far = np.zeros((32, 32, 32), dtype=np.uint32)
    far[0, 0, 0] = STONE
    c.world = vra.World(svo_type)
    c.world.set_chunk((1, 1, 1), _chunk_of((1, 1, 1), 5, b))
    c.world.set_chunk((3, 3, 3), _chunk_of((3, 3, 3), 5, far))
    c.world.serialize()
    assert c.world.depth == 7
    blocks = np.zeros((96, 96, 96), dtype=np.uint32)
    blocks[:32, :32, :32] = b
    blocks[64, 64, 64] = STONE
    lo = np.full(3, BURROW_AT, dtype=np.int64)
    c.info = dict(name="burrow", svo_type=svo_type, depth=7, size=128.0, lo=lo, hi=lo + 96, blocks=blocks, detail=np.ones(blocks.shape, dtype=bool), lod_box=None)
    c.truth, c.cell = blocks, np.zeros(blocks.shape, dtype=np.uint32)
    c.tex, c.mats = scenes.synthetic_textures(), scenes.synthetic_materials()
    c.frame = np.concatenate([c.world.frame(pad_words=0), np.zeros(4, dtype=np.uint32)])
    return c


def make_flood_case(name, fmt):
    """A world in one format, its dense truth and its positions; computed once, left unchanged."""
    if name == "burrow":
        c = burrow(host.SVO_ESVO if fmt == "esvo" else host.SVO_CSVO)
        c.name, c.fmt, c.svo_type = name, fmt, host.SVO_ESVO if fmt == "esvo" else host.SVO_CSVO
        c.size = 128
        for a in (c.truth, c.frame):
            a.setflags(write=False)
    else:
        c = make_scan_case(name, fmt)
    c.positions, c.names = make_positions(c)
    c.positions.setflags(write=False)
    c.seeded = np.arange(SEEDED)
    return c


# ---- positions and the forms they are handed over in ---------------------------------------------------------------------------------------------


def named_positions(c):
    """[(name, position)], each named for what it catches."""
    lo, hi, size = c.info["lo"], c.info["hi"], float(c.size)
    t = c.truth
    solid = np.argwhere(t != 0)
    # a block with air on top of it: a seed in a block that has somewhere to spread to under VX_FLOOD_SEED_ALWAYS
    open_top = np.argwhere((t[:, :-1, :] != 0) & (t[:, 1:, :] == 0))
    block = lo + (open_top[len(open_top) // 2] if len(open_top) else solid[len(solid) // 2])
    mid = (lo + hi) / 2.0
    out = [("in_block", block + 0.5), ("integral", np.floor(mid)), ("minus_zero", (-0.0, -0.0, -0.0)),
           ("far_x", (3e9, mid[1], mid[2])), ("far_negative", (mid[0], -3e9, mid[2])), ("far_huge", (mid[0], mid[1], 1e30)), ("far_all", (3e9, -3e9, 1e30)),
           ("beyond_int32", (2147483648.0, -2147483904.0, 2147483520.0)), ("above_chunks", (mid[0], float(hi[1]) + 2.5, mid[2]))]
    for a in range(3):  # a seed on each face of the world, the box overhanging it; in line with the chunks where the world is that small
        for far in (0, 1):
            p = np.array(mid, dtype=np.float64)
            p[a] = size - 0.5 if far else 0.5
            out.append((f"world_face_{2 * a + far}", p))
    for a in range(3):
        for bad, word in ((np.nan, "nan"), (np.inf, "inf"), (-np.inf, "-inf")):
            p = np.array(mid, dtype=np.float64)
            p[a] = bad
            out.append((f"{word}_{a}", p))
    out.append(("nan_all", (np.nan, np.nan, np.nan)))
    if c.name == "tower":
        out.append(("lod_seam", (6.5, 14.5, 30.5)))    # z = 32: LOD 5 below, LOD 2 above
        out.append(("lod_leaves", (70.5, 108.5, 40.5)))  # beside leaves of side 8 and 16
    if c.name == "burrow":
        out += [(name, lo + np.array(at) + 0.5) for name, at in BURROW_NAMED.items()]
    return out


def make_positions(c):
    """(float32 [N, 3], name -> index): the seeded set -- uniform over the occupied extent grown by 4 --, then the named ones."""
    rng = np.random.default_rng(FLOOD_SEED[c.name])
    lo, hi = c.info["lo"].astype(np.float64), c.info["hi"].astype(np.float64)
    if c.name == "burrow":
        hi = lo + 32.0  # (the chunk: the single block that sizes the world is not what is flooded)
    seeded = rng.uniform(lo - 4.0, hi + 4.0, (SEEDED, 3))
    named = named_positions(c)
    pts = np.concatenate([seeded, np.array([p for _, p in named], dtype=np.float64)]).astype(np.float32)
    return np.ascontiguousarray(pts), {name: SEEDED + k for k, (name, _) in enumerate(named)}


def positions_for(c, shape):
    """The case's positions as the shape wants them: unchanged, or -- snap -- moved to the first cell of their brick, the fraction kept
    (positions beyond +-2^20 and those that are no position stay: the move would not be exact)."""
    p = c.positions
    if not shape.snap:
        return p
    with np.errstate(invalid="ignore"):
        near = np.isfinite(p) & (np.abs(p) < 2.0 ** 20)
    q = np.where(near, p, 0).astype(np.float64)
    moved = np.floor(q / 8.0) * 8.0 + (q - np.floor(q))
    return np.ascontiguousarray(np.where(near, moved, p).astype(np.float32))


def in_form(pts, form):
    """(raw uint8 bytes, stride, an (N, 3) float32 view of them at that stride) of positions in one form."""
    n = len(pts)
    if form == "entities":
        e = np.zeros(n, dtype=hip.ENTITY_DTYPE)
        e["position"] = pts
        e["velocity"], e["aabb_extents"], e["flags"] = 0.25, 0.8, 0x5a5a5a5a  # (what lies behind the position is not read)
        raw, stride = e.view(np.uint8).copy(), 64
    else:
        stride = 12 if form == "packed" else 16
        padded = np.full((n, stride // 4), 7.0e37, dtype=np.float32)
        padded[:, :3] = pts
        raw = padded.reshape(-1).view(np.uint8).copy()
    view = np.ndarray((n, 3), dtype=np.float32, buffer=raw, offset=0, strides=(stride, 4))
    return raw, stride, view


def torch_positions(raw, stride, n):
    """The same view of a copy of the bytes in device memory."""
    import torch

    floats = torch.from_numpy(raw.copy()).cuda().view(torch.float32)
    return floats.as_strided((n, 3), (stride // 4, 1), 0)


# ---- the truth: plain numpy over the dense arrays ----------------------------------------------------------------------------------------------


def info_of(fields, shape, seed_values):
    """FLOOD_INFO_DTYPE records read off fields [N, voxels] (not fields of no position)."""
    f = fields.reshape(len(fields), shape.size[2], shape.size[1], shape.size[0])
    got = f <= MAX_STEPS
    out = np.zeros(len(fields), dtype=hip.FLOOD_INFO_DTYPE)
    out["reached"] = got.sum(axis=(1, 2, 3))
    out["farthest"] = np.where(got, f, 0).max(axis=(1, 2, 3))
    faces = [got[:, :, :, 0], got[:, :, :, -1], got[:, :, 0, :], got[:, :, -1, :], got[:, 0, :, :], got[:, -1, :, :]]
    out["faces"] = sum(face.any(axis=(1, 2)).astype(np.uint32) << k for k, face in enumerate(faces))
    out["seed_value"] = seed_values
    return out


def flood_batch(passable, seed_at):
    """fields [N, z, y, x] uint8 of the full flood (VX_FLOOD_MAX_STEPS steps) of boolean arrays passable [N, z, y, x] from cell seed_at."""
    n = len(passable)
    fields = np.where(passable, UNREACHED, BLOCKED).astype(np.uint8)
    z, y, x = seed_at[2], seed_at[1], seed_at[0]
    frontier = np.zeros(passable.shape, dtype=bool)
    frontier[:, z, y, x] = passable[:, z, y, x]
    fields[frontier] = 0
    active = np.flatnonzero(frontier.any(axis=(1, 2, 3)))
    frontier, free = frontier[active], (passable & (fields != 0))[active]  # free: passable and not reached yet
    for step in range(1, MAX_STEPS + 1):
        if not len(active):
            break
        grow = np.zeros(frontier.shape, dtype=bool)
        grow[:, 1:] |= frontier[:, :-1]
        grow[:, :-1] |= frontier[:, 1:]
        grow[:, :, 1:] |= frontier[:, :, :-1]
        grow[:, :, :-1] |= frontier[:, :, 1:]
        grow[:, :, :, 1:] |= frontier[:, :, :, :-1]
        grow[:, :, :, :-1] |= frontier[:, :, :, 1:]
        grow &= free
        fields[active] = np.where(grow, step, fields[active])
        free &= ~grow
        going = grow.any(axis=(1, 2, 3))
        active, frontier, free = active[going], grow[going], free[going]
    return fields.reshape(n, -1)


def cut_to(fields, max_steps):
    """The fields of a flood cut short after max_steps."""
    return np.where((fields <= MAX_STEPS) & (fields > max_steps), UNREACHED, fields).astype(np.uint8)


_TRUTHS = {}  # kept for the run: the two formats of a world share their truth (but `tower`'s, whose CSVO form has another chunk)


def _regions(c, shape):
    """(block ids [N, z, y, x] of every query's box, has_position [N]) for the case's positions under `shape`."""
    key = (c.name, c.fmt if c.name == "tower" else "", shape.name)
    if key not in _TRUTHS:
        pts = positions_for(c, shape)
        sx, sy, sz = shape.size
        regions = np.zeros((len(pts), sz, sy, sx), dtype=np.uint32)
        has = np.zeros(len(pts), dtype=bool)
        for k, p in enumerate(pts):
            seed = start_of(p)
            if seed is not None:
                has[k] = True
                regions[k] = dense_region(c.info, c.truth, [s - a for s, a in zip(seed, shape.seed_at)], shape.size)
        _TRUTHS[key] = (regions, has)
    return _TRUTHS[key]


def full_truth(c, shape, pass_value=0, flags=0):
    """(fields [N, voxels] at VX_FLOOD_MAX_STEPS, seed values [N], has_position [N]) for the case's positions under `shape`; kept. Under
    VX_FLOOD_SEED_ALWAYS only the queries whose seed does not pass are flooded again: the flag changes nothing for the others."""
    key = (c.name, c.fmt if c.name == "tower" else "", shape.name, pass_value, flags)
    if key in _TRUTHS:
        return _TRUTHS[key]
    regions, has = _regions(c, shape)
    z, y, x = shape.seed_at[2], shape.seed_at[1], shape.seed_at[0]
    seed_values = np.where(has, regions[:, z, y, x], 0).astype(np.uint32)
    if flags & SEED_ALWAYS:
        fields = full_truth(c, shape, pass_value, 0)[0].copy()
        again = np.flatnonzero(has & (fields[:, (z * shape.size[1] + y) * shape.size[0] + x] == BLOCKED))
    else:
        fields = np.zeros((len(regions), shape.voxels), dtype=np.uint8)
        again = np.arange(len(regions))
    if len(again):
        passable = regions[again] == 0
        if pass_value:
            passable |= regions[again] == pass_value
        if flags & SEED_ALWAYS:
            passable[:, z, y, x] = True
        fields[again] = flood_batch(passable, shape.seed_at)
    fields[~has] = NO_POSITION
    for a in (fields, seed_values):
        a.setflags(write=False)
    _TRUTHS[key] = (fields, seed_values, has)
    return _TRUTHS[key]


def truth_for(c, shape, max_steps, pass_value=0, flags=0):
    """(fields [N, padded]: the voxels, then VX_FLOOD_BLOCKED up to the multiple of 16; FLOOD_INFO_DTYPE records [N])."""
    full, seed_values, has = full_truth(c, shape, pass_value, flags)
    cut = cut_to(full, max_steps)
    info = info_of(np.where(has[:, None], cut, BLOCKED), shape, seed_values)
    info[~has] = np.array((INVALID, 0, 0, 0), dtype=hip.FLOOD_INFO_DTYPE)
    fields = np.full((len(cut), shape.padded), BLOCKED, dtype=np.uint8)
    fields[:, :shape.voxels] = cut
    return fields, info


def batches(count, field_stride):
    """[(first, end)] of `count` queries in calls that each write at most 2^24 bytes of fields."""
    most = max((1 << 24) // field_stride, 1)
    return [(a, min(a + most, count)) for a in range(0, count, most)] or [(0, 0)]


def points_truth(c, pts, shape, max_steps, pass_value=0, flags=0, truth=None):
    """truth_for for any positions (not kept); truth: the dense array to flood instead of the case's (a world that has been changed)."""
    sx, sy, sz = shape.size
    z, y, x = shape.seed_at[2], shape.seed_at[1], shape.seed_at[0]
    regions = np.zeros((len(pts), sz, sy, sx), dtype=np.uint32)
    has = np.zeros(len(pts), dtype=bool)
    for k, p in enumerate(np.asarray(pts, dtype=np.float32)):
        seed = start_of(p)
        if seed is not None:
            has[k] = True
            regions[k] = dense_region(c.info, c.truth if truth is None else truth, [s - a for s, a in zip(seed, shape.seed_at)], shape.size)
    passable = (regions == 0) | ((regions == pass_value) if pass_value else False)
    if flags & SEED_ALWAYS:
        passable[:, z, y, x] = True
    cut = cut_to(flood_batch(passable & has[:, None, None, None], shape.seed_at), max_steps)
    info = info_of(cut, shape, regions[:, z, y, x])
    info[~has] = np.array((INVALID, 0, 0, 0), dtype=hip.FLOOD_INFO_DTYPE)
    fields = np.full((len(cut), shape.padded), BLOCKED, dtype=np.uint8)
    fields[:, :shape.voxels] = np.where(has[:, None], cut, NO_POSITION)
    return fields, info


def calls_for(c):
    """[(name, shape, max_steps, pass_value, flags, form)]: every shape at every step limit, every shape under VX_FLOOD_SEED_ALWAYS, and a
    pass_value that occurs in the world; the forms in turn."""
    out = []
    for i, shape in enumerate(SHAPES):
        for j, max_steps in enumerate(STEP_LIMITS):
            out.append((f"{shape.name}-{max_steps}", shape, max_steps, 0, 0, FORMS[(i + j) % 3]))
        out.append((f"{shape.name}-seed_always", shape, 250, 0, SEED_ALWAYS, FORMS[i % 3]))
    out.append(("17-pass", SHAPE["17"], 250, pass_id(c), 0, "packed"))
    out.append(("17-pass-seed_always", SHAPE["17"], 24, pass_id(c), SEED_ALWAYS, "entities"))
    return out


def pass_id(c):
    """The id that passes in the pass_value calls: the door's in `burrow`, the commonest elsewhere."""
    if c.name == "burrow":
        return DOOR
    ids, counts = np.unique(c.truth[c.truth != 0], return_counts=True)
    return int(ids[counts.argmax()])


# ---- the host harness: a stand-alone program -----------------------------------------------------------------------------------------


def harness(sanitize=False):
    """tests/_build/flood_on_host, or flood_on_host_san: host_harness.build_harness's."""
    return build_harness("flood_on_host", sanitize)


class HostFlood(HostRunner):
    """The harness on one world: the frame is written once, every call is a run of the program."""

    def flood(self, raw, stride, count, shape, max_steps, pass_value=0, flags=0, field_stride=0, fields=True, info=True):
        """(fields [count, field_stride or padded] or None, FLOOD_INFO_DTYPE records or None); more queries than one call may write fields
        for (2^24 bytes) are several runs."""
        parts = batches(count, field_stride or shape.padded) if fields else [(0, count)]
        if len(parts) > 1:
            got = [self.flood(raw[a * stride:], stride, b - a, shape, max_steps, pass_value, flags, field_stride, fields, info) for a, b in parts]
            return np.concatenate([f for f, _ in got]), (np.concatenate([i for _, i in got]) if info else None)
        self.run("flood", self.put("points.bin", raw), stride, count, *shape.size, *shape.seed_at, max_steps, pass_value, flags, field_stride,
                 self.path("fields.bin", fields), self.path("info.bin", info))
        f = self.get("fields.bin", np.uint8, fields, (count, field_stride or shape.padded))
        i = self.get("info.bin", hip.FLOOD_INFO_DTYPE, info)
        assert i is None or len(i) == count
        return f, i

    def call(self, c, call, pick=None):
        """One of calls_for's calls on the case's positions, or on those of them that `pick` indexes."""
        _, shape, max_steps, pass_value, flags, form = call
        pts = positions_for(c, shape)
        pts = pts if pick is None else pts[pick]
        raw, stride, _ = in_form(pts, form)
        return self.flood(raw, stride, len(pts), shape, max_steps, pass_value, flags)


def differing(got_fields, got_info, exp_fields, exp_info):
    """A message naming the first query whose field or record differs, or None."""
    return outputs_differing((got_fields, got_info), (exp_fields, exp_info))
