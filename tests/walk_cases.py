"""Shared by the tests of vx_walk_points (test_walk_abi.py, test_walk_on_host.py, test_walk.py): flood_cases.py's four worlds unchanged and a
fifth, `steps`, built here -- one chunk on the world's floor that holds the named cases: a staircase of 1-high steps and a 2-high step, ledges
of 1, 2, 3 and 4 down, corridors 1 and 2 high, a step up under a low ceiling over the source column, a drop under a lintel over the
destination column, a floor of pass_value blocks, a shaft through the world's bottom and a floor at the world's y = 0 --, the positions and
goals of each -- a seeded set of 300 and the named ones --, the shapes, step limits and path capacities, and the expected field, record and
path of every query: plain numpy over blocks_cases.dense_region of the query's extended box -- a batched breadth-first search by shifted
boolean arrays with the three edge kinds (a query leaves the batch when its frontier is empty), the back-trace as a Python loop. The search is
run once per shape and pass_value to VX_WALK_MAX_STEPS; a smaller step limit's field is that field with the larger step counts turned into
VX_WALK_UNREACHED, and VX_WALK_STOP_AT_GOAL is the step limit min(max_steps, path_steps), as the header states it. Nothing of the code under
test is used. Also the runner of the host harness (tests/cpp/walk_on_host.cpp), a stand-alone program, plain and built with sanitizers."""

import numpy as np

from batch_cases import _chunk_of
from blocks_cases import dense_region
from host_harness import HostRunner, build_harness, outputs_differing
from flood_cases import BURROW_AT, FLOOD_CASES, in_form, make_flood_case, torch_positions  # noqa: F401  (the forms are the flood's)
from helpers import vra
from scan_cases import ScanCase, start_of
from voxel_rs_amd import hip, host

NO_POSITION, UNREACHED, NO_STAND, NONE, INVALID = hip.VX_WALK_NO_POSITION, hip.VX_WALK_UNREACHED, hip.VX_WALK_NO_STAND, hip.VX_WALK_NONE, hip.VX_FLOOD_INVALID
MAX_STEPS, STOP = hip.VX_WALK_MAX_STEPS, hip.VX_WALK_STOP_AT_GOAL
WALK_CASES = FLOOD_CASES + [("steps", "esvo"), ("steps", "csvo")]
WALK_SEED = {"glasshouse": 181, "far_chunks": 182, "tower": 183, "burrow": 184, "steps": 185}
SEEDED = 300
FORMS = ("packed", "stride16", "entities")
STEP_LIMITS = (0, 1, 24, 250)
PATH_CAPACITIES = (0, 4, 252)
STONE, DOOR = 3, 9
STEPS_AT = np.array([32, 0, 32])  # the chunk (1, 0, 1): on the world's floor
SIDES = ((-1, 0), (1, 0), (0, -1), (0, 1))  # (dx, dz) in the back-trace's order


class Shape:
    """A vx_walk_shape without its step limit, pass_value, path capacity and flags. snap: as flood_cases.Shape's."""

    def __init__(self, name, size, seed_at, height=2, climb=1, drop=3, snap=False):
        self.name, self.size, self.seed_at, self.height, self.climb, self.drop, self.snap = name, tuple(size), tuple(seed_at), height, climb, drop, snap
        self.voxels = size[0] * size[1] * size[2]
        self.padded = (self.voxels + 15) // 16 * 16
        assert size[1] + height <= 32


SHAPES = [Shape("1", (1, 1, 1), (0, 0, 0), height=1), Shape("17", (17, 12, 17), (8, 6, 8)), Shape("9_two_bricks", (9, 9, 9), (4, 4, 4), snap=True),
          Shape("32x28_h4", (32, 28, 32), (16, 14, 16), height=4), Shape("32x31_h1", (32, 31, 32), (16, 15, 16), height=1),
          Shape("31x3x17_corner", (31, 3, 17), (30, 2, 0)), Shape("32x1x1", (32, 1, 1), (5, 0, 0), height=1), Shape("17_flat", (17, 12, 17), (8, 6, 8), climb=0, drop=0)]
SHAPE = {s.name: s for s in SHAPES}


# ---- the fifth world ---------------------------------------------------------------------------------------------------------------------------


def steps_blocks():
    """The chunk's blocks [x][y][z]: ground up to y = 7 (one stands at y = 8), cut into lanes two cells wide along x at z = 4 k + 1, 4 k + 2 by
    walls up to y = 27 at z = 4 k and 4 k + 3. Lane 0: a staircase, the ground's top 8, 9, 10, 11 at x = 4..7, 11 up to x = 11, then 13 at
    x = 12..15 -- a 2-high step. Lane 1: ledges, the top 15 at x < 6, 14 at 6..9, 12 at 10..13, 9 at 14..17, 5 from 18 on: 1, 2, 3 and 4 down.
    Lanes 2 and 3: rock at x = 8..24 up to y = 20 with a corridor at z = 9 one cell high and one at z = 13 two cells high. Lane 4: the ground one
    higher from x = 10 on, and a block at (9, 10): a ceiling over the SOURCE column of the step up. Lane 5: the top 10 at x < 10 and 8 from there
    on, and a block at (10, 12): a lintel over the DESTINATION column of the drop. Lane 6: the ground's top layer of id 9 at x = 8..12. Lane 7:
    a shaft through everything at (20, *, 29), and at x = 24..30 nothing but the layer y = 0: a floor with no world beneath it."""
    b = np.zeros((32, 32, 32), dtype=np.uint32)
    b[:, 0:8, :] = STONE
    for k in range(8):
        b[:, 8:28, 4 * k] = STONE
        b[:, 8:28, 4 * k + 3] = STONE
    lane = lambda k: slice(4 * k + 1, 4 * k + 3)
    for x, top in ((4, 8), (5, 9), (6, 10), (7, 11), (8, 11), (9, 11), (10, 11), (11, 11), (12, 13), (13, 13), (14, 13), (15, 13)):
        b[x, 8:top + 1, lane(0)] = STONE
    for x in range(32):
        top = 15 if x < 6 else 14 if x < 10 else 12 if x < 14 else 9 if x < 18 else 5
        b[x, :, lane(1)] = 0
        b[x, 0:top + 1, lane(1)] = STONE
    b[8:25, 8:21, 8:16] = STONE
    b[8:25, 8, 9] = 0
    b[8:25, 8:10, 13] = 0
    b[10:, 8, lane(4)] = STONE
    b[9, 10, lane(4)] = STONE
    b[:10, 8:11, lane(5)] = STONE
    b[10:, 8, lane(5)] = STONE
    b[10, 12, lane(5)] = STONE
    b[8:13, 7, lane(6)] = DOOR
    b[20, :, 29] = 0
    b[24:31, 1:8, lane(7)] = 0
    return b


# name -> (the seed's cell, the goal's cell or None or "nan"), chunk coordinates; the seed's position is the cell's centre
STEPS_NAMED = {"stairs_up": ((2, 8, 1), (9, 12, 1)), "two_high_step": ((10, 12, 1), (13, 14, 1)), "ledges_down": ((5, 16, 5), (13, 13, 5)),
               "ledge_three": ((11, 13, 5), (16, 10, 5)), "ledge_four": ((16, 10, 5), (19, 6, 5)), "ledges_back_up": ((8, 15, 5), (4, 16, 5)), "corridor_1": ((6, 8, 9), (14, 8, 9)),
               "corridor_2": ((6, 8, 13), (14, 8, 13)), "low_ceiling": ((7, 8, 17), (12, 9, 17)), "lintel": ((7, 11, 21), (12, 9, 21)),
               "pass_floor": ((6, 8, 25), (14, 8, 25)), "in_air": ((4, 10, 29), (6, 8, 29)), "over_hole": ((20, 9, 29), (18, 8, 29)), "in_rock": ((4, 3, 29), (6, 8, 29)),
               "goal_is_seed": ((4, 8, 29), (4, 8, 29)), "goal_outside": ((4, 8, 29), (24, 8, 29)), "goal_nan": ((4, 8, 29), "nan"),
               "goal_in_air": ((4, 8, 30), (7, 11, 30)), "world_floor": ((26, 1, 29), (29, 1, 30))}


def steps_world(svo_type):
    from voxel_rs_amd import scenes

    c = ScanCase()
    b = steps_blocks()
    far = np.zeros((32, 32, 32), dtype=np.uint32)  # (a single block at (3, 3, 3) * 32 makes the world span [0, 128), as flood_cases.burrow's)
    far[0, 0, 0] = STONE
    c.world = vra.World(svo_type)
    c.world.set_chunk((1, 0, 1), _chunk_of((1, 0, 1), 5, b))
    c.world.set_chunk((3, 3, 3), _chunk_of((3, 3, 3), 5, far))
    c.world.serialize()
    assert c.world.depth == 7
    blocks = np.zeros((96, 128, 96), dtype=np.uint32)
    blocks[:32, :32, :32] = b
    blocks[64, 96, 64] = STONE
    lo = STEPS_AT.astype(np.int64)
    c.info = dict(name="steps", svo_type=svo_type, depth=7, size=128.0, lo=lo, hi=lo + np.array(blocks.shape), blocks=blocks, detail=np.ones(blocks.shape, dtype=bool), lod_box=None)
    c.truth, c.cell = blocks, np.zeros(blocks.shape, dtype=np.uint32)
    c.tex, c.mats = scenes.synthetic_textures(), scenes.synthetic_materials()
    c.frame = np.concatenate([c.world.frame(pad_words=0), np.zeros(4, dtype=np.uint32)])
    c.name, c.fmt, c.svo_type, c.size = "steps", "esvo" if svo_type == host.SVO_ESVO else "csvo", svo_type, 128
    for a in (c.truth, c.frame):
        a.setflags(write=False)
    return c


def make_walk_case(name, fmt):
    """A world in one format, its dense truth, its positions and goals; computed once, left unchanged."""
    c = steps_world(host.SVO_ESVO if fmt == "esvo" else host.SVO_CSVO) if name == "steps" else make_flood_case(name, fmt)
    c.positions, c.goals, c.names = make_positions(c)
    c.positions.setflags(write=False)
    c.goals.setflags(write=False)
    return c


# ---- positions and goals -------------------------------------------------------------------------------------------------------------------------


def standable_cells(c, height=2):
    """World coordinates of the cells of the dense array with a block below and `height` cells of air (by the dense array alone; its rim is
    left out)."""
    air = np.asarray(c.truth) == 0
    s = ~air[:, :-height, :]
    for j in range(height):
        s = s & air[:, 1 + j:air.shape[1] - height + 1 + j, :]
    cells = np.argwhere(s)
    cells[:, 1] += 1
    return cells + c.info["lo"]


def named_positions(c):
    """[(name, position, goal)], each named for what it catches."""
    lo, hi = c.info["lo"], c.info["hi"]
    mid = (lo + hi) / 2.0
    nan3 = (np.nan, np.nan, np.nan)
    out = [("far_all", (3e9, -3e9, 1e30), (3e9, -3e9, 1e30)), ("beyond_int32", (2147483648.0, -2147483904.0, 2147483520.0), (-2147483904.0, 2147483648.0, 0.0)),
           ("minus_zero", (-0.0, -0.0, -0.0), (0.5, 0.5, 0.5)), ("above_chunks", (mid[0], float(hi[1]) + 2.5, mid[2]), (mid[0] + 1, float(hi[1]) + 0.5, mid[2]))]
    for a in range(3):
        for bad, word in ((np.nan, "nan"), (np.inf, "inf"), (-np.inf, "-inf")):
            p = np.array(mid, dtype=np.float64)
            p[a] = bad
            out.append((f"{word}_{a}", p, mid))
    out.append(("nan_all", nan3, nan3))
    for bad, word in ((np.inf, "goal_inf"), (-np.inf, "goal_-inf")):
        out.append((word, mid, (mid[0], bad, mid[2])))
    if c.name == "tower":
        out.append(("lod_seam", (6.5, 33.5, 34.5), (9.5, 32.5, 38.5)))    # z = 32: LOD 5 below, LOD 2 above, on whose coarse voxels one stands
        out.append(("lod_leaves", (70.5, 108.5, 40.5), (73.5, 108.5, 43.5)))  # beside leaves of side 8 and 16
    if c.name == "burrow":
        at = lambda cell: BURROW_AT + np.array(cell) + 0.5
        out += [("serpentine_start", at((1, 4, 1)), at((30, 4, 29))), ("serpentine_near", at((1, 4, 1)), at((30, 4, 3))), ("serpentine_far", at((1, 4, 1)), at((3, 4, 17))), ("room", at((5, 13, 5)), at((4, 12, 6))),
                ("on_top", at((16, 34, 16)), at((20, 32, 12)))]
    if c.name == "steps":
        for name, (cell, goal) in STEPS_NAMED.items():
            g = nan3 if goal == "nan" else STEPS_AT + np.array(goal) + 0.5
            out.append((name, STEPS_AT + np.array(cell) + 0.5, g))
    return out


def make_positions(c):
    """(positions float32 [N, 3], goals float32 [N, 3], name -> index): 150 positions uniform over the occupied extent grown by 4 with goals up
    to 6 cells off, 150 placed 0..3 cells above a standable cell of the dense array with a goal 0..3 cells above another at most 7 cells
    away, then the named ones."""
    rng = np.random.default_rng(WALK_SEED[c.name])
    lo, hi = c.info["lo"].astype(np.float64), c.info["hi"].astype(np.float64)
    if c.name in ("burrow", "steps"):
        hi = lo + 32.0  # (the chunk: the single block that sizes the world is not what is walked on)
    half = SEEDED // 2
    uniform = rng.uniform(lo - 4.0, hi + 4.0, (half, 3))
    uniform_goals = uniform + rng.uniform(-6.0, 6.0, (half, 3))
    cells = standable_cells(c)
    cells = cells[((cells >= lo) & (cells < hi + 1)).all(axis=1)]
    assert len(cells) >= 8, c.name
    picked = cells[rng.integers(0, len(cells), half)]
    placed = picked + 0.5 + np.stack([np.zeros(half), rng.integers(0, 4, half), np.zeros(half)], axis=1)
    placed_goals = np.zeros((half, 3))
    for k, cell in enumerate(picked):
        near = cells[(np.abs(cells - cell).max(axis=1) <= 7)]
        placed_goals[k] = near[rng.integers(0, len(near))] + 0.5 + (0, rng.integers(0, 4), 0)
    named = named_positions(c)
    pts = np.concatenate([uniform, placed, np.array([p for _, p, _ in named], dtype=np.float64)]).astype(np.float32)
    goals = np.concatenate([uniform_goals, placed_goals, np.array([g for _, _, g in named], dtype=np.float64)]).astype(np.float32)
    return np.ascontiguousarray(pts), np.ascontiguousarray(goals), {name: SEEDED + k for k, (name, _, _) in enumerate(named)}


def snapped(p):
    """flood_cases.positions_for's move: to the first cell of the position's brick, the fraction kept."""
    with np.errstate(invalid="ignore"):
        near = np.isfinite(p) & (np.abs(p) < 2.0 ** 20)
    q = np.where(near, p, 0).astype(np.float64)
    return np.ascontiguousarray(np.where(near, np.floor(q / 8.0) * 8.0 + (q - np.floor(q)), p).astype(np.float32))


def positions_for(c, shape):
    """(positions, goals) as the shape wants them: unchanged, or -- snap -- the positions moved to the first cell of their brick and the goals
    by the same whole number of cells."""
    if not shape.snap:
        return c.positions, c.goals
    p = snapped(c.positions)
    with np.errstate(invalid="ignore"):
        move = np.where(np.isfinite(c.positions) & (np.abs(c.positions) < 2.0 ** 20), p.astype(np.float64) - c.positions, 0.0)
        goals = np.where(np.isfinite(c.goals) & (np.abs(c.goals) < 2.0 ** 20), c.goals + move, c.goals)
    return p, np.ascontiguousarray(goals.astype(np.float32))


# ---- the truth: plain numpy over the dense arrays ----------------------------------------------------------------------------------------------


def beside(a):
    """[N, z, y, x] -> the cells with a set cell at x +- 1 or z +- 1."""
    out = np.zeros(a.shape, dtype=bool)
    out[:, :, :, 1:] |= a[:, :, :, :-1]
    out[:, :, :, :-1] |= a[:, :, :, 1:]
    out[:, 1:] |= a[:, :-1]
    out[:, :-1] |= a[:, 1:]
    return out


def graph_of(passable, shape):
    """(standable [N, z, sy, x], up_ok: the cells whose column is free for a step up, clear[d - 1]: the cells whose column is free for a drop
    of d onto them) of passable [N, z, sy + height, x], whose layer 0 lies below the box."""
    sy, h = shape.size[1], shape.height
    stand = ~passable[:, :, 0:sy]
    for j in range(h):
        stand = stand & passable[:, :, 1 + j:1 + j + sy]
    up_ok = np.zeros(stand.shape, dtype=bool)
    if shape.climb and sy > 1:
        up_ok[:, :, :sy - 1] = passable[:, :, 1 + h:h + sy]   # (x, y + height, z) of a cell that has a layer above it in the box
    clear = []
    free = np.ones(stand.shape, dtype=bool)
    for d in range(1, shape.drop + 1):
        now = np.zeros(stand.shape, dtype=bool)
        if sy > d:
            now[:, :, :sy - d] = free[:, :, :sy - d] & passable[:, :, h + d:h + sy]  # (x', y' + height + d - 1, z') for y' + d inside the box
        free = now
        clear.append(now)
    return stand, up_ok, clear


def walk_batch(stand, up_ok, clear, start):
    """fields [N, z, y, x] uint8 of the full search (VX_WALK_MAX_STEPS steps) from start [N] = (x, y, z) or None."""
    n = len(stand)
    fields = np.where(stand, UNREACHED, NO_STAND).astype(np.uint8)
    frontier = np.zeros(stand.shape, dtype=bool)
    for k, s in enumerate(start):
        if s is not None:
            assert stand[k, s[2], s[1], s[0]]
            frontier[k, s[2], s[1], s[0]] = True
    fields[frontier] = 0
    active = np.flatnonzero(frontier.any(axis=(1, 2, 3)))
    frontier, free = frontier[active], (stand & (fields != 0))[active]
    for step in range(1, MAX_STEPS + 1):
        if not len(active):
            break
        near = beside(frontier)
        grow = near.copy()                                             # level
        grow[:, :, 1:] |= beside(frontier & up_ok[active])[:, :, :-1]  # from below
        for d, free_above in enumerate(clear, start=1):                # from above by d
            grow[:, :, :-d] |= near[:, :, d:] & free_above[active][:, :, :-d]
        grow &= free
        fields[active] = np.where(grow, step, fields[active])
        free &= ~grow
        going = grow.any(axis=(1, 2, 3))
        active, frontier, free = active[going], grow[going], free[going]
    return fields.reshape(n, -1)


def settle(column, e, height):
    """The layer (0: below the box) an agent put into layer e of passable column [layers] comes to stand on, or None."""
    if not column[e:e + height].all():
        return None
    while e >= 1 and column[e - 1]:
        e -= 1
    return e if e >= 1 else None


def trace(field, passable, shape, goal, steps):
    """The cells (rx, ry, rz) after 1..steps steps of the path to `goal`, found backwards by the header's order. field [z, y, x] of step
    counts, passable [z, layers, x]."""
    sx, sy, sz = shape.size
    h = shape.height
    x, y, z = goal
    out = []
    for k in range(steps, 0, -1):
        out.append((x, y, z))
        found = None
        for dx, dz in SIDES:
            px, pz = x + dx, z + dz
            if not (0 <= px < sx and 0 <= pz < sz):
                continue
            kinds = [(y, True)]
            if y >= 1:
                kinds.append((y - 1, bool(shape.climb) and bool(passable[pz, y - 1 + 1 + h, px])))
            else:
                kinds.append((y - 1, False))
            for d in range(1, shape.drop + 1):
                kinds.append((y + d, y + d < sy and bool(passable[z, y + 1 + h:y + 1 + h + d, x].all())))
            for py, edge in kinds:
                if edge and 0 <= py < sy and field[pz, py, px] == k - 1:
                    found = (px, py, pz)
                    break
            if found:
                break
        assert found is not None
        x, y, z = found
    return out[::-1]


_TRUTHS = {}


def _extended(c, pts, shape, truth=None):
    """(block ids [N, z, size.y + height, x] of every query's box with the layer below and those above, lo [N] as Python ints or None)."""
    sx, sy, sz = shape.size
    regions = np.zeros((len(pts), sz, sy + shape.height, sx), dtype=np.uint32)
    los = []
    for k, p in enumerate(pts):
        seed = start_of(p)
        los.append(None if seed is None else [s - a for s, a in zip(seed, shape.seed_at)])
        if seed is not None:
            lo = los[-1]
            regions[k] = dense_region(c.info, c.truth if truth is None else truth, [lo[0], lo[1] - 1, lo[2]], [sx, sy + shape.height, sz])
    return regions, los


def full_of(c, pts, goals, shape, pass_value=0, truth=None):
    """The search run to VX_WALK_MAX_STEPS for any positions: a dict of fields [N, voxels], seed_value, has, start_ry, goal (settled cell or
    None), goal_steps (None: not reached), paths (lists of packed entries)."""
    regions, los = _extended(c, pts, shape, truth)
    n = len(pts)
    passable = (regions == 0) | ((regions == pass_value) if pass_value else False)
    stand, up_ok, clear = graph_of(passable, shape)
    ax, ay, az = shape.seed_at
    has = np.array([lo is not None for lo in los])
    start, goal_cells = [], []
    for k in range(n):
        s = g = None
        if has[k]:
            e = settle(passable[k, az, :, ax], ay + 1, shape.height)
            s = None if e is None else (ax, e - 1, az)
            gs = None if goals is None else start_of(goals[k])
            if gs is not None:
                rel = [a - b for a, b in zip(gs, los[k])]
                if all(0 <= r < m for r, m in zip(rel, shape.size)):
                    e = settle(passable[k, rel[2], :, rel[0]], rel[1] + 1, shape.height)
                    g = None if e is None else (rel[0], e - 1, rel[2])
        start.append(s)
        goal_cells.append(g)
    fields = walk_batch(stand, up_ok, clear, start)
    goal_steps, paths = [], []
    f4 = fields.reshape(n, shape.size[2], shape.size[1], shape.size[0])
    for k in range(n):
        g = goal_cells[k]
        d = None if g is None or f4[k, g[2], g[1], g[0]] > MAX_STEPS else int(f4[k, g[2], g[1], g[0]])
        goal_steps.append(d)
        paths.append([] if d is None else [x | y << 8 | z << 16 for x, y, z in trace(f4[k], passable[k], shape, g, d)])
    fields[~has] = NO_POSITION
    seed_values = np.where(has, regions[:, az, ay + 1, ax], 0).astype(np.uint32)
    return dict(fields=fields, seed_value=seed_values, has=has, start=start, goal=goal_cells, goal_steps=goal_steps, paths=paths)


def full_truth(c, shape, pass_value=0):
    """full_of for the case's own positions and goals under `shape`; kept (the two formats of a world share it, but `tower`'s, whose CSVO form
    has another chunk)."""
    key = (c.name, c.fmt if c.name == "tower" else "", shape.name, pass_value)
    if key not in _TRUTHS:
        pts, goals = positions_for(c, shape)
        _TRUTHS[key] = full_of(c, pts, goals, shape, pass_value)
        _TRUTHS[key]["fields"].setflags(write=False)
    return _TRUTHS[key]


def answers(full, shape, max_steps, path_capacity=0, flags=0, with_goal=True):
    """(fields [N, padded], WALK_INFO_DTYPE records [N], paths uint32 [N, path_capacity]) of a call, read off the full search."""
    n = len(full["fields"])
    limit = np.full(n, max_steps, dtype=np.int64)
    steps = np.array([NONE if (d is None or not with_goal or d > max_steps) else d for d in full["goal_steps"]], dtype=np.int64)
    if flags & STOP:
        limit = np.minimum(limit, steps)
    f = full["fields"]
    cut = np.where((f <= MAX_STEPS) & (f > limit[:, None]), UNREACHED, f).astype(np.uint8)
    has = full["has"]
    info = np.zeros(n, dtype=hip.WALK_INFO_DTYPE)
    cells = np.where(has[:, None], cut, NO_STAND).reshape(n, shape.size[2], shape.size[1], shape.size[0])
    got = cells <= MAX_STEPS
    info["reached"] = got.sum(axis=(1, 2, 3))
    info["farthest"] = np.where(got, cells, 0).max(axis=(1, 2, 3))
    faces = [got[:, :, :, 0], got[:, :, :, -1], got[:, :, 0, :], got[:, :, -1, :], got[:, 0, :, :], got[:, -1, :, :]]
    info["faces"] = sum(face.any(axis=(1, 2)).astype(np.uint32) << k for k, face in enumerate(faces))
    info["seed_value"] = full["seed_value"]
    info["start_ry"] = [NONE if s is None else s[1] for s in full["start"]]
    info["goal_ry"] = [NONE if (g is None or not with_goal) else g[1] for g in full["goal"]]
    info["path_steps"] = steps
    none = np.array((INVALID, 0, 0, 0, NONE, NONE, NONE, 0), dtype=hip.WALK_INFO_DTYPE)
    info[~has] = none
    fields = np.full((n, shape.padded), NO_STAND, dtype=np.uint8)
    fields[:, :shape.voxels] = cut
    paths = np.full((n, path_capacity), NONE, dtype=np.uint32)
    if with_goal and path_capacity:
        for k in range(n):
            if has[k] and steps[k] != NONE:
                m = min(int(steps[k]), path_capacity)
                paths[k, :m] = full["paths"][k][:m]
    return fields, info, paths


def truth_for(c, shape, max_steps, path_capacity=0, flags=0, pass_value=0, with_goal=True):
    return answers(full_truth(c, shape, pass_value), shape, max_steps, path_capacity, flags, with_goal)


def points_truth(c, pts, goals, shape, max_steps, path_capacity=0, flags=0, pass_value=0, truth=None):
    """answers for any positions (not kept); truth: the dense array to walk instead of the case's (a world that has been changed)."""
    return answers(full_of(c, np.asarray(pts, dtype=np.float32), None if goals is None else np.asarray(goals, dtype=np.float32), shape, pass_value, truth), shape, max_steps,
                   path_capacity, flags, goals is not None)


def edge_kinds(full, shape):
    """How often the shortest paths of a full search use a level edge, an up edge and a drop of d: {dy: count}."""
    out = {}
    for k, path in enumerate(full["paths"]):
        if full["start"][k] is None:
            continue
        y = full["start"][k][1]
        for entry in path:
            ny = (entry >> 8) & 0xFF
            out[ny - y] = out.get(ny - y, 0) + 1
            y = ny
    return out


def calls_for(c):
    """[(name, shape, max_steps, path_capacity, flags, pass_value, form)]: every shape at every step limit, the path capacities, the flag and
    the forms in turn; a pass_value that occurs in the world; paths and the flag at every capacity on the main shape."""
    out = []
    for i, shape in enumerate(SHAPES):
        for j, max_steps in enumerate(STEP_LIMITS):
            cap, flags = PATH_CAPACITIES[(i + j) % 3], STOP if (i + j) % 2 else 0
            out.append((f"{shape.name}-{max_steps}", shape, max_steps, cap, flags, 0, FORMS[(i + j) % 3]))
    for cap in PATH_CAPACITIES:
        out.append((f"17-stop-{cap}", SHAPE["17"], 250, cap, STOP, 0, FORMS[cap % 3]))
        out.append((f"17-paths-{cap}", SHAPE["17"], 250, cap, 0, 0, "packed"))
    out.append(("17-pass", SHAPE["17"], 250, 252, 0, pass_id(c), "entities"))
    out.append(("32x31_h1-pass-stop", SHAPE["32x31_h1"], 24, 4, STOP, pass_id(c), "stride16"))
    return out


def pass_id(c):
    """The id that passes in the pass_value calls: the door's in `burrow` and `steps`, the commonest elsewhere."""
    if c.name in ("burrow", "steps"):
        return DOOR
    ids, counts = np.unique(c.truth[c.truth != 0], return_counts=True)
    return int(ids[counts.argmax()])


def batches(count, field_stride):
    most = max((1 << 24) // field_stride, 1)
    return [(a, min(a + most, count)) for a in range(0, count, most)] or [(0, 0)]


# ---- the host harness: a stand-alone program -----------------------------------------------------------------------------------------


def harness(sanitize=False):
    """tests/_build/walk_on_host, or walk_on_host_san: host_harness.build_harness's."""
    return build_harness("walk_on_host", sanitize)


class HostWalk(HostRunner):
    """The harness on one world: the frame is written once, every call is a run of the program."""

    def walk(self, raw, stride, graw, gstride, count, shape, max_steps, path_capacity=0, flags=0, pass_value=0, field_stride=0, fields=True, info=True, paths=None):
        """(fields [count, field_stride or padded] or None, WALK_INFO_DTYPE records or None, paths uint32 [count, path_capacity] or None).
        graw None: no goal; paths None: asked for when there is a goal."""
        paths = graw is not None if paths is None else paths
        self.run("walk", self.put("points.bin", raw), stride, "-" if graw is None else self.put("goals.bin", graw), gstride, count, *shape.size, *shape.seed_at, max_steps,
                 pass_value, shape.height, shape.climb, shape.drop, path_capacity, flags, field_stride, self.path("fields.bin", fields), self.path("paths.bin", paths),
                 self.path("info.bin", info))
        f = self.get("fields.bin", np.uint8, fields, (count, field_stride or shape.padded))
        i = self.get("info.bin", hip.WALK_INFO_DTYPE, info)
        p = self.get("paths.bin", np.uint32, paths, (count, path_capacity))
        assert i is None or len(i) == count
        return f, i, p

    def call(self, c, call, pick=None):
        """One of calls_for's calls on the case's positions, or on those of them that `pick` indexes."""
        _, shape, max_steps, cap, flags, pass_value, form = call
        pts, goals = positions_for(c, shape)
        pts, goals = (pts, goals) if pick is None else (pts[pick], goals[pick])
        raw, stride, _ = in_form(pts, form)
        graw, gstride, _ = in_form(goals, form)
        return self.walk(raw, stride, graw, gstride, len(pts), shape, max_steps, cap, flags, pass_value)


def differing(got, exp):
    """A message naming the first query whose field, record or path differs between two (fields, info, paths), or None."""
    return outputs_differing(got, exp)
