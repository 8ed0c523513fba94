"""Shared by the tests of vx_label_boxes (test_label_abi.py, test_label_on_host.py, test_label.py): flood_cases.py's four worlds in both
formats and a fifth, `rubble`, built here -- solid rock around a hollow that holds loose pieces of every kind the call has to tell apart --;
the boxes of each -- a seeded set of 200 and the named ones --; the shapes, the forms the boxes are handed over in (packed, at stride 16, inside
a larger record) and the expected field, piece records and record of every box.

The truth is plain numpy over blocks_cases.dense_region of each box: breadth-first floods by shifted ORs of boolean arrays for a whole batch
at once (a box leaves the batch when its frontier is empty) -- first from the solid cells on the anchor faces, then from the first unsettled
solid cell in the field's order, again and again until none is left --, recording every flood's depth and every cell's distance. It is run
once per shape, anchor_faces and pass_value with no budget at all; the answer under max_pieces and max_steps is derived from the recorded
depths by the rule of include/voxel_hip.h (a flood is complete when used + depth <= max_steps). Nothing of the code under test is used.
Also the runner of the host harness (tests/cpp/label_on_host.cpp), a stand-alone program, plain and built with sanitizers."""

import numpy as np

from batch_cases import _chunk_of
from blocks_cases import dense_region
from host_harness import HostRunner, build_harness, outputs_differing
from flood_cases import FLOOD_CASES, make_flood_case
from helpers import vra
from light_cases import in_form, torch_boxes  # noqa: F401  (the forms of lo are vx_light_boxes')
from scan_cases import ScanCase
from voxel_rs_amd import hip, host

AIR, MORE, HELD, CUT, ALL_FACES = hip.VX_LABEL_AIR, hip.VX_LABEL_MORE, hip.VX_LABEL_HELD, hip.VX_LABEL_CUT, hip.VX_LABEL_ALL_FACES
MAX_PIECES, MAX_STEPS = hip.VX_LABEL_MAX_PIECES, hip.VX_LABEL_MAX_STEPS
LABEL_CASES = FLOOD_CASES + [("rubble", "esvo"), ("rubble", "csvo")]
LABEL_SEED = {"glasshouse": 121, "far_chunks": 122, "tower": 123, "burrow": 124, "rubble": 125}
SEEDED = 200
FORMS = (12, 16, 64)  # lo_stride
ANCHORS = (ALL_FACES, 0, 0x04, 0x03)  # every face, none, the floor only, the two x faces
PIECES = (0, 4, MAX_PIECES)
STEPS = (0, 1, 24, MAX_STEPS)
ROCK, LINK = 3, 9
RUBBLE_AT = 32  # the chunk (1, 1, 1) spans [32, 64) on every axis


class Shape:
    """The box of a call. snap: None -- the boxes' lo as they are; else every seeded lo is moved down to a multiple of 8 and `snap` added."""

    def __init__(self, name, size, snap=None):
        self.name, self.size, self.snap = name, tuple(size), snap
        self.voxels = size[0] * size[1] * size[2]
        self.padded = (self.voxels + 15) // 16 * 16


SHAPES = [Shape("1", (1, 1, 1)), Shape("9_two_bricks", (9, 9, 9), (4, 4, 4)), Shape("17", (17, 17, 17)), Shape("32", (32, 32, 32)), Shape("31x3x17", (31, 3, 17)),
          Shape("32x1x1", (32, 1, 1)), Shape("1x32x1", (1, 32, 1))]
SHAPE = {s.name: s for s in SHAPES}
SEVENTEEN = SHAPE["17"]  # the named boxes' shape, and the conditions'


# ---- the fifth world --------------------------------------------------------------------------------------------------------------------------


def rubble_blocks():
    """The chunk's blocks [x][y][z]: rock two cells thick around a hollow x, y, z in 2..29, and in the hollow, each a cell of air or more from
    the rock and from the others:
      a single floating block at (4, 4, 4); a floating 2 x 2 x 2 at x 7..8, y 4..5, z 4..5;
      two blocks that touch only along an edge, (11, 4, 4) and (12, 5, 4), and two that touch only at a corner, (15, 4, 4) and (16, 5, 5);
      a ring of 16 cells at y = 4: the border of x 19..23, z 3..7;
      a checkerboard x 4..9, y 8..13, z 10..15: the 108 cells whose coordinates sum to an even number, every one a piece;
      a blob x 13..15, y 26..28, z 13..15 hanging from the ceiling (y = 30) by one cell of id 9 at (14, 29, 14);
      a wire at y = 20, burrow's serpentine inverted: 10 rows of 26 cells along x = 3..28 at z = 3, 5, ..., 21, joined at alternating ends:
      269 cells, 268 steps end to end;
      a U in the plane z = 26: prongs x = 5 and x = 9 over y 4..8, the base y = 3 over x 5..9 -- a box from y = 4 up holds two pieces;
      two single blocks, (24, 12, 23) and (20, 10, 25): the first has the smaller z, the second the smaller x and the smaller y;
      a 2 x 2 x 2 at x 15..16, y 15..16, z 23..24, across a brick boundary on all three axes;
      a coil at y = 24, small enough for a box of 17^3 to hold all of it: 4 rows of 9 cells along x = 18..26 at z = 18, 20, 22, 24, joined at
      alternating ends: 39 cells, 38 steps end to end."""
    b = np.full((32, 32, 32), ROCK, dtype=np.uint32)
    b[2:30, 2:30, 2:30] = 0
    b[4, 4, 4] = ROCK
    b[7:9, 4:6, 4:6] = ROCK
    b[11, 4, 4] = b[12, 5, 4] = ROCK
    b[15, 4, 4] = b[16, 5, 5] = ROCK
    b[19:24, 4, 3:8] = ROCK
    b[20:23, 4, 4:7] = 0
    x, y, z = np.meshgrid(np.arange(4, 10), np.arange(8, 14), np.arange(10, 16), indexing="ij")
    even = (x + y + z) % 2 == 0
    b[x[even], y[even], z[even]] = ROCK
    b[13:16, 26:29, 13:16] = ROCK
    b[14, 29, 14] = LINK
    for k in range(10):
        b[3:29, 20, 3 + 2 * k] = ROCK
        if k < 9:
            b[28 if k % 2 == 0 else 3, 20, 4 + 2 * k] = ROCK
    b[5, 4:9, 26] = b[9, 4:9, 26] = ROCK
    b[5:10, 3, 26] = ROCK
    b[24, 12, 23] = b[20, 10, 25] = ROCK
    b[15:17, 15:17, 23:25] = ROCK
    for k in range(4):
        b[18:27, 24, 18 + 2 * k] = ROCK
        if k < 3:
            b[26 if k % 2 == 0 else 18, 24, 19 + 2 * k] = ROCK
    return b


# what the named tests ask of `rubble`: (lo inside the chunk, size, anchor_faces, pass_value)
RUBBLE_NAMED = {
    "single": ((2, 2, 2), (5, 5, 5), ALL_FACES, 0),
    "cube": ((6, 3, 3), (4, 4, 4), ALL_FACES, 0),
    "edge_pair": ((10, 3, 3), (4, 4, 3), ALL_FACES, 0),
    "corner_pair": ((14, 3, 3), (4, 4, 4), ALL_FACES, 0),
    "ring": ((18, 3, 2), (7, 3, 7), ALL_FACES, 0),
    "checkerboard": ((3, 7, 9), (8, 8, 8), ALL_FACES, 0),
    "blob_held": ((6, 15, 6), (17, 17, 17), ALL_FACES, 0),
    "blob_loose": ((6, 15, 6), (17, 17, 17), ALL_FACES, LINK),
    "wire": ((2, 19, 2), (28, 3, 21), ALL_FACES, 0),
    "u_cut": ((3, 4, 22), (9, 9, 7), 0, 0),
    "u_whole": ((3, 2, 22), (9, 11, 7), 0, 0),
    "order": ((18, 8, 22), (9, 7, 5), ALL_FACES, 0),
    "straddle": ((12, 12, 20), (8, 8, 8), ALL_FACES, 0),
    "coil": ((17, 23, 17), (11, 3, 9), ALL_FACES, 0),
}
SOLID_ROCK = (96, 96, 96)  # rubble's chunk (3, 3, 3), rock all through: as a box of 32^3 one piece of 32,768 cells


def rubble(svo_type):
    """As flood_cases.burrow: the chunk (1, 1, 1), and the chunk (3, 3, 3) -- here rock all through -- that makes the world span [0, 128)."""
    from voxel_rs_amd import scenes

    c = ScanCase()
    b = rubble_blocks()
    far = np.full((32, 32, 32), ROCK, dtype=np.uint32)
    c.world = vra.World(svo_type)
    c.world.set_chunk((1, 1, 1), _chunk_of((1, 1, 1), 5, b))
    c.world.set_chunk((3, 3, 3), _chunk_of((3, 3, 3), 5, far))
    c.world.serialize()
    assert c.world.depth == 7
    blocks = np.zeros((96, 96, 96), dtype=np.uint32)
    blocks[:32, :32, :32] = b
    blocks[64:, 64:, 64:] = ROCK
    lo = np.full(3, RUBBLE_AT, dtype=np.int64)
    c.info = dict(name="rubble", svo_type=svo_type, depth=7, size=128.0, lo=lo, hi=lo + 96, blocks=blocks, detail=np.ones(blocks.shape, dtype=bool), lod_box=None)
    c.truth, c.cell = blocks, np.zeros(blocks.shape, dtype=np.uint32)
    c.tex, c.mats = scenes.synthetic_textures(), scenes.synthetic_materials()
    c.frame = np.concatenate([c.world.frame(pad_words=0), np.zeros(4, dtype=np.uint32)])
    c.size = 128
    for a in (c.truth, c.frame):
        a.setflags(write=False)
    return c


def make_label_case(name, fmt):
    """A world in one format, its dense truth and its boxes; computed once, left unchanged."""
    if name == "rubble":
        c = rubble(host.SVO_ESVO if fmt == "esvo" else host.SVO_CSVO)
        c.name, c.fmt, c.svo_type = name, fmt, host.SVO_ESVO if fmt == "esvo" else host.SVO_CSVO
    else:
        c = make_flood_case(name, fmt)
    c.boxes, c.names = make_boxes(c)
    c.boxes.setflags(write=False)
    return c


# ---- boxes --------------------------------------------------------------------------------------------------------------------------------------


def named_boxes(c):
    """[(name, lo)], each a 17^3 box named for what it catches."""
    lo, hi, size = c.info["lo"], c.info["hi"], int(c.size)
    if c.name in ("burrow", "rubble"):
        hi = lo + 32
    mid = (lo + hi) // 2 - 8
    out = []
    for a in range(3):  # across each face of the world, half of the box outside it; in line with the chunks
        for far in (0, 1):
            p = np.array(mid)
            p[a] = size - 9 if far else -8
            out.append((f"world_face_{2 * a + far}", p))
    out += [("outside", (size + 5, mid[1], mid[2])), ("negative_lo", (-7, -3, -9)), ("wrapping", (2147483647 - 20, -2147483648, 2147483647 - 3)),
            ("chunk_corner", tuple(lo - 8))]
    if c.name == "tower":
        out += [("lod_seam", (0, 6, 24)), ("lod_leaf", (64, 100, 34))]  # z = 32: LOD 5 below, LOD 2 above; beside leaves of side 8 and 16
    if c.name == "rubble":
        out.append(("in_rock", SOLID_ROCK))
    return out


def make_boxes(c):
    """(int32 [N, 3], name -> index): the seeded set, then the named ones. A third of the seeded boxes is uniform over the occupied extent grown
    by 8; two thirds lie around solid cells that have air on at least one side and lie two cells or more inside the extent (by the dense
    array, jittered by up to 6): where pieces and anchors are found. The lo is that of a 17^3 box centred there."""
    rng = np.random.default_rng(LABEL_SEED[c.name])
    lo, hi = c.info["lo"], c.info["hi"]
    if c.name in ("burrow", "rubble"):
        hi = lo + 32
    t = c.truth[:hi[0] - lo[0], :hi[1] - lo[1], :hi[2] - lo[2]] != 0
    open_side = np.zeros(t.shape, dtype=bool)
    for a in range(3):
        air = ~t
        open_side |= np.roll(air, 1, axis=a) | np.roll(air, -1, axis=a)
    surface = np.argwhere(t[2:-2, 2:-2, 2:-2] & open_side[2:-2, 2:-2, 2:-2]) + 2
    third = SEEDED // 3
    seeded = [rng.integers(lo - 8 - 8, hi + 8 - 8, (SEEDED - 2 * third, 3))]
    if len(surface):
        seeded.append(surface[rng.integers(0, len(surface), 2 * third)] + lo - 8 + rng.integers(-6, 7, (2 * third, 3)))
    else:
        seeded.append(rng.integers(lo - 16, hi, (2 * third, 3)))
    named = named_boxes(c)
    boxes = np.concatenate(seeded + [np.array([p for _, p in named], dtype=np.int64)]).astype(np.int32)
    return np.ascontiguousarray(boxes), {name: SEEDED + k for k, (name, _) in enumerate(named)}


def boxes_for(c, shape):
    """The case's boxes as the shape wants them: unchanged, or the seeded ones moved to a multiple of 8 plus shape.snap."""
    if shape.snap is None:
        return c.boxes
    b = c.boxes.copy()
    b[:SEEDED] = (b[:SEEDED] // 8) * 8 + np.array(shape.snap, dtype=np.int32)
    return b


# ---- the truth: plain numpy over the dense arrays ----------------------------------------------------------------------------------------------


def _grow(f):
    """The six neighbours inside the box of the cells of f [M, z, y, x]."""
    g = np.zeros_like(f)
    g[:, 1:] |= f[:, :-1]
    g[:, :-1] |= f[:, 1:]
    g[:, :, 1:] |= f[:, :, :-1]
    g[:, :, :-1] |= f[:, :, 1:]
    g[:, :, :, 1:] |= f[:, :, :, :-1]
    g[:, :, :, :-1] |= f[:, :, :, 1:]
    return g


def _flood(seeds, free):
    """(distance [M, z, y, x] int32, -1 where not reached; depth [M]) of the floods from `seeds` through `free` (seeds lie in free)."""
    dist = np.where(seeds, 0, -1).astype(np.int32)
    depth = np.zeros(len(seeds), dtype=np.int64)
    active = np.flatnonzero(seeds.any(axis=(1, 2, 3)))
    frontier, left = seeds[active], (free & ~seeds)[active]
    k = 0
    while len(active):
        k += 1
        grow = _grow(frontier) & left
        going = grow.any(axis=(1, 2, 3))
        sub = dist[active]
        sub[grow] = k
        dist[active] = sub
        depth[active[going]] = k
        left &= ~grow
        active, frontier, left = active[going], grow[going], left[going]
    return dist, depth


def anchor_cells(shape_zyx, faces):
    """bool [z, y, x]: the cells on the faces of the box that `faces` names."""
    m = np.zeros(shape_zyx, dtype=bool)
    for f, index in enumerate(((..., 0), (..., -1), (slice(None), 0), (slice(None), -1), (0,), (-1,))):
        if faces >> f & 1:
            m[index] = True
    return m


class Full:
    """The floods of a batch of boxes with no budget: solid [N, z, y, x]; held_dist (the distance from the anchors, -1: not held) and
    held_depth [N]; label (the number of the piece in the field's order, 0: none, not cut off at 250) and depths[k], the depth of each piece
    of box k."""


def label_full(values, anchor_faces, pass_value):
    f = Full()
    f.solid = (values != 0) & ((values != pass_value) if pass_value else True)
    n = len(values)
    f.held_dist, f.held_depth = _flood(f.solid & anchor_cells(values.shape[1:], anchor_faces), f.solid)
    settled = f.held_dist >= 0
    f.label = np.zeros(values.shape, dtype=np.int32)
    f.depths = [[] for _ in range(n)]
    number = 0
    while True:
        unsettled = f.solid & ~settled
        has = np.flatnonzero(unsettled.any(axis=(1, 2, 3)))
        if not len(has):
            break
        number += 1
        free = unsettled[has]
        flat = free.reshape(len(has), -1)
        seeds = np.zeros_like(flat)
        seeds[np.arange(len(has)), flat.argmax(axis=1)] = True  # the first in the field's order: least z, then y, then x
        dist, depth = _flood(seeds.reshape(free.shape), free)
        got = dist >= 0
        sub = f.label[has]
        sub[got] = number
        f.label[has] = sub
        settled[has] |= got
        for k, d in zip(has, depth):
            f.depths[k].append(int(d))
    return f


def _pack(x, y, z):
    return int(x) | int(y) << 8 | int(z) << 16


def _faces_of(cells):
    faces = [cells[:, :, 0], cells[:, :, -1], cells[:, 0, :], cells[:, -1, :], cells[0], cells[-1]]
    return sum(int(face.any()) << f for f, face in enumerate(faces))


def derive(full, shape, max_pieces, max_steps):
    """(fields [N, padded], LABEL_PIECE_DTYPE [N, max_pieces], LABEL_INFO_DTYPE [N]) under a budget, by the header's rule."""
    n = len(full.solid)
    fields = np.zeros((n, shape.padded), dtype=np.uint8)
    pieces = np.zeros((n, max_pieces), dtype=hip.LABEL_PIECE_DTYPE)
    info = np.zeros(n, dtype=hip.LABEL_INFO_DTYPE)
    for k in range(n):
        solid, dist = full.solid[k], full.held_dist[k]
        used, flags = 0, 0
        if full.held_depth[k] <= max_steps:
            held, used = dist >= 0, int(full.held_depth[k])
        else:
            held, used, flags = (dist >= 0) & (dist <= max_steps), max_steps, CUT
        field = np.where(solid, MORE, AIR).astype(np.uint8)
        field[held] = HELD
        count = loose = 0
        if not flags:
            for number, depth in enumerate(full.depths[k], 1):
                if count >= max_pieces:
                    break
                if used + depth > max_steps:
                    used, flags = max_steps, CUT
                    break
                used += depth
                cells = full.label[k] == number
                field[cells] = number
                z, y, x = np.nonzero(cells)  # (in the field's order: the first is the seed)
                pieces[k, count] = (len(x), _pack(x.min(), y.min(), z.min()), _pack(x.max(), y.max(), z.max()), _pack(x[0], y[0], z[0]) | _faces_of(cells) << 24)
                count += 1
                loose += len(x)
        fields[k, :shape.voxels] = field.reshape(-1)
        total, n_held = int(solid.sum()), int(held.sum())
        info[k] = (total, n_held, count, loose, total - n_held - loose, used, _faces_of(solid), flags)
    return fields, pieces, info


def regions_of(c, boxes, size, truth=None):
    """Block ids [N, z, y, x] of the boxes."""
    out = np.zeros((len(boxes), size[2], size[1], size[0]), dtype=np.uint32)
    for k, lo in enumerate(np.asarray(boxes, dtype=np.int64)):
        out[k] = dense_region(c.info, c.truth if truth is None else truth, lo, size)
    return out


def label_truth(c, boxes, shape, anchor_faces=ALL_FACES, max_pieces=MAX_PIECES, max_steps=MAX_STEPS, pass_value=0, truth=None):
    """derive() of label_full() for any boxes (not kept); shape: a Shape, or a size; truth: the dense array to label instead of the case's."""
    shape = shape if isinstance(shape, Shape) else Shape("", shape)
    return derive(label_full(regions_of(c, boxes, shape.size, truth), anchor_faces, pass_value), shape, max_pieces, max_steps)


_FULLS = {}  # kept for the run: the two formats of a world share their truth (but `tower`'s, whose CSVO form has another chunk)
_TRUTHS = {}


def pick_for(c, shape):
    """The boxes a call of this shape is made on: all of them."""
    return np.arange(len(c.boxes))


def pass_id(c):
    """The id that counts as air in the pass_value calls: the link's in `rubble` (and the door's in `burrow`, the same 9), the commonest
    elsewhere."""
    if c.name in ("burrow", "rubble"):
        return LINK
    ids, counts = np.unique(c.truth[c.truth != 0], return_counts=True)
    return int(ids[counts.argmax()])


def calls_for(c):
    """[(name, shape, anchor_faces, max_pieces, max_steps, pass_value, lo_stride)]: every shape under every anchor_faces with the piece
    limits, step budgets, pass values and strides in turn; and at 17^3 with every face anchored every piece limit under every step budget,
    without and with the pass value."""
    out = []
    for i, shape in enumerate(SHAPES):
        for j, faces in enumerate(ANCHORS):
            k = i + j
            out.append((f"{shape.name}-{faces:#x}", shape, faces, PIECES[(k + 2) % 3], STEPS[(k + 3) % 4], pass_id(c) if k % 2 else 0, FORMS[k % 3]))
    for j, (most, steps) in enumerate((m, s) for m in PIECES for s in STEPS):
        out.append((f"17-{most}-{steps}", SEVENTEEN, ALL_FACES, most, steps, 0, FORMS[j % 3]))
        out.append((f"17-{most}-{steps}-pass", SEVENTEEN, ALL_FACES, most, steps, pass_id(c), FORMS[(j + 1) % 3]))
    return out


def the_call(c, name):
    return [call for call in calls_for(c) if call[0] == name][0]


def full_for(c, shape, anchor_faces, pass_value):
    key = (c.name, c.fmt if c.name == "tower" else "", shape.name, anchor_faces, pass_value)
    if key not in _FULLS:
        _FULLS[key] = label_full(regions_of(c, boxes_for(c, shape)[pick_for(c, shape)], shape.size), anchor_faces, pass_value)
    return _FULLS[key]


def truth_for(c, call):
    """(fields, pieces, info) of one of calls_for's calls on the boxes pick_for gives; kept."""
    name, shape, faces, most, steps, pass_value, _ = call
    key = (c.name, c.fmt if c.name == "tower" else "", name)
    if key not in _TRUTHS:
        got = derive(full_for(c, shape, faces, pass_value), shape, most, steps)
        for a in got:
            a.setflags(write=False)
        _TRUTHS[key] = got
    return _TRUTHS[key]


def cells(fields, shape):
    """[N, z, y, x] of fields."""
    return fields[:, :shape.voxels].reshape(len(fields), shape.size[2], shape.size[1], shape.size[0])


# ---- the host harness: a stand-alone program -----------------------------------------------------------------------------------------


def harness(sanitize=False):
    """tests/_build/label_on_host, or label_on_host_san: host_harness.build_harness's."""
    return build_harness("label_on_host", sanitize)


class HostLabel(HostRunner):
    """The harness on one world: the frame is written once, every call is a run of the program."""

    def label(self, boxes, size, anchor_faces=ALL_FACES, max_pieces=MAX_PIECES, max_steps=MAX_STEPS, pass_value=0, lo_stride=12, field_stride=0, fields=True, pieces=None,
              info=True):
        """(fields [count, field_stride or padded] or None, LABEL_PIECE_DTYPE [count, max_pieces] or None, LABEL_INFO_DTYPE records or None);
        pieces None: asked for when max_pieces > 0."""
        count = len(boxes)
        voxels = size[0] * size[1] * size[2]
        pieces = max_pieces > 0 if pieces is None else pieces
        lo = self.put("lo.bin", in_form(np.asarray(boxes, dtype=np.int32).reshape(-1, 3), lo_stride)[0])
        self.run("label", lo, lo_stride, count, *size, anchor_faces, max_pieces, max_steps, pass_value, field_stride, self.path("fields.bin", fields),
                 self.path("pieces.bin", pieces), self.path("info.bin", info))
        f = self.get("fields.bin", np.uint8, fields, (count, field_stride or (voxels + 15) // 16 * 16))
        p = self.get("pieces.bin", hip.LABEL_PIECE_DTYPE, pieces, (count, max_pieces))
        i = self.get("info.bin", hip.LABEL_INFO_DTYPE, info)
        assert i is None or len(i) == count
        return f, p, i

    def call(self, c, call, pick=None):
        """One of calls_for's calls on the boxes pick_for gives, or on those of them that `pick` indexes."""
        _, shape, faces, most, steps, pass_value, stride = call
        boxes = boxes_for(c, shape)[pick_for(c, shape)]
        f, p, i = self.label(boxes if pick is None else boxes[pick], shape.size, faces, most, steps, pass_value, stride)
        return f, (np.zeros((len(f), 0), dtype=hip.LABEL_PIECE_DTYPE) if p is None else p), i


def differing(got, expected):
    """A message naming the first box whose field, piece records or record differ between two (fields, pieces, info), or None."""
    return outputs_differing(got, expected)
