"""Shared by the tests of vx_light_boxes (test_light_abi.py, test_light_on_host.py, test_light.py): flood_cases.py's four worlds in both
formats and a fifth, `lantern`, built here; a table of props for each, derived from the ids the world holds; the boxes of each -- a seeded set
of 100 and the named ones --; the shapes, the forms the boxes are handed over in (packed, at stride 16, at stride 64) and the expected field
and record of every box.

The truth is plain numpy over the dense arrays, straight from the per-cell rule of include/voxel_hip.h: the sky exposure from the dense array
of the whole column above each cell, then both channels by iterating "a passable cell takes the largest of its six neighbours less one, or
its own source level" over whole batches until nothing changes. It is no level-ordered flood and uses nothing of the code under test.

The props: the ids of a world sorted by how often they occur (the id breaks ties); the commonest stays opaque and dark, and of the others the
rarest emits 15 and is opaque, the next emits 4 and is opaque, the next is transparent and emits 9, the next is transparent and dark, the
rest are opaque and dark. `burrow` holds two ids only -- rock and the one block of its door --, so there the door emits 15 and nothing is
transparent or emits a low level: `burrow` cannot show a transparent block, a low emitter or overlapping emitters, and its one emitter
lies in a corridor sealed in rock, so none of its seeded boxes has both channels in one cell (0 of 100, against the 10 asked for; it meets
the two other conditions on the seeded boxes: test_light_on_host.py prints the figures). `lantern` carries all of that: a walled hall under a roof with a one-cell hole and a
patch of panes, lamps of 15, an ember of 4, lava (transparent, 12), a lamp sealed in rock and a wall between a lamp and the cells behind it.
Also the runner of the host harness (tests/cpp/light_on_host.cpp), a stand-alone program, plain and built with sanitizers."""

import numpy as np

from batch_cases import _chunk_of
from blocks_cases import dense_region
from host_harness import HostRunner, build_harness, outputs_differing
from flood_cases import FLOOD_CASES, make_flood_case
from helpers import vra
from scan_cases import ScanCase
from voxel_rs_amd import hip, host

TRANSPARENT, NO_SKY, NO_BLOCKS = hip.VX_LIGHT_TRANSPARENT, hip.VX_LIGHT_NO_SKY, hip.VX_LIGHT_NO_BLOCKS
LIGHT_CASES = FLOOD_CASES + [("lantern", "esvo"), ("lantern", "csvo")]
LIGHT_SEED = {"glasshouse": 101, "far_chunks": 102, "tower": 103, "burrow": 104, "lantern": 105}
SEEDED = 100
FORMS = (12, 16, 64)  # lo_stride
LAMP, EMBER, ROCK, PANE, LAVA = 1, 2, 3, 4, 5
LANTERN_PROPS = {LAMP: 15, EMBER: 4, ROCK: 0, PANE: TRANSPARENT, LAVA: TRANSPARENT | 12}


class Shape:
    """The box of a call. snap: None -- the boxes' lo as they are; else every seeded lo is moved down to a multiple of 8 and `snap` added."""

    def __init__(self, name, size, snap=None):
        self.name, self.size, self.snap = name, tuple(size), snap
        self.voxels = size[0] * size[1] * size[2]
        self.padded = (self.voxels + 15) // 16 * 16


SHAPES = [Shape("1", (1, 1, 1)), Shape("16_aligned", (16, 16, 16), (0, 0, 0)), Shape("16_off", (16, 16, 16), (3, 5, 6)), Shape("33x9x17", (33, 9, 17)),
          Shape("48", (48, 48, 48)), Shape("48x1x48", (48, 1, 48)), Shape("1x48x1", (1, 48, 1))]
SHAPE = {s.name: s for s in SHAPES}
SIXTEEN = Shape("16", (16, 16, 16))  # the named boxes' shape, and the conditions'


# ---- the fifth world --------------------------------------------------------------------------------------------------------------------------


def lantern_blocks():
    """The chunk's blocks [x][y][z]: a floor two blocks thick; a hall -- walls at x and z = 2 and 29 up to a roof at y = 20 -- whose roof has a
    one-cell hole at (8, 20, 8) and panes over x, z in 18..23; inside it a lamp at (10, 3, 20) with a wall at x = 13 behind it, a lamp at
    (22, 3, 8) four cells from lava at (26, 3, 8), an ember at (24, 5, 12), a cube of rock x 4..8, y 2..6, z 22..26 with a lamp in its middle;
    outside it a lamp on the roof and lava on the floor."""
    b = np.zeros((32, 32, 32), dtype=np.uint32)
    b[:, 0:2, :] = ROCK
    b[2:30, 20, 2:30] = ROCK
    for at in (2, 29):
        b[at, 2:20, 2:30] = ROCK
        b[2:30, 2:20, at] = ROCK
    b[8, 20, 8] = 0
    b[18:24, 20, 18:24] = PANE
    b[13, 2:12, 14:27] = ROCK
    b[10, 3, 20] = LAMP
    b[22, 3, 8], b[26, 3, 8], b[24, 5, 12] = LAMP, LAVA, EMBER
    b[4:9, 2:7, 22:27] = ROCK
    b[6, 4, 24] = LAMP
    b[16, 21, 12], b[31, 2, 16] = LAMP, LAVA
    return b


def lantern(svo_type):
    from voxel_rs_amd import scenes

    c = ScanCase()
    b = lantern_blocks()
    c.world = vra.World(svo_type)
    c.world.set_chunk((0, 0, 0), _chunk_of((0, 0, 0), 5, b))
    c.world.serialize()
    assert c.world.depth == 6
    lo = np.zeros(3, dtype=np.int64)
    c.info = dict(name="lantern", svo_type=svo_type, depth=6, size=64.0, lo=lo, hi=lo + 32, blocks=b, detail=np.ones(b.shape, dtype=bool), lod_box=None)
    c.truth, c.cell = b, np.zeros(b.shape, dtype=np.uint32)
    c.tex, c.mats = scenes.synthetic_textures(), scenes.synthetic_materials()
    c.frame = np.concatenate([c.world.frame(pad_words=0), np.zeros(4, dtype=np.uint32)])
    c.size = 64
    for a in (c.truth, c.frame):
        a.setflags(write=False)
    return c


def make_light_case(name, fmt):
    """A world in one format, its dense truth, its props and its boxes; computed once, left unchanged."""
    if name == "lantern":
        c = lantern(host.SVO_ESVO if fmt == "esvo" else host.SVO_CSVO)
        c.name, c.fmt, c.svo_type = name, fmt, host.SVO_ESVO if fmt == "esvo" else host.SVO_CSVO
    else:
        c = make_flood_case(name, fmt)
    c.props = props_of(c)
    c.boxes, c.names = make_boxes(c)
    c.boxes.setflags(write=False)
    return c


# ---- props ------------------------------------------------------------------------------------------------------------------------------------


def props_of(c):
    """uint8 [highest id + 1]: see the module's docstring."""
    ids, counts = np.unique(c.truth[c.truth != 0], return_counts=True)
    props = np.zeros(int(ids.max()) + 1, dtype=np.uint8)
    if c.name == "lantern":
        for i, p in LANTERN_PROPS.items():
            props[i] = p
        return props
    order = [int(i) for _, i in sorted(zip(counts.tolist(), ids.tolist()))][:-1]  # rarest first, the commonest left out
    for i, p in zip(order, (15, 4, TRANSPARENT | 9, TRANSPARENT)):
        props[i] = p
    return props


def tables(props):
    """(passes [n] bool, emits [n] uint8) of a props table; id 0 passes and emits nothing whatever props[0] says."""
    passes, emits = (props & TRANSPARENT) != 0, (props & 15).astype(np.uint8)
    if len(props):
        passes[0], emits[0] = True, 0
    return passes, emits


# ---- boxes --------------------------------------------------------------------------------------------------------------------------------------


def named_boxes(c):
    """[(name, lo)], each a 16^3 box named for what it catches."""
    lo, hi, size = c.info["lo"], c.info["hi"], int(c.size)
    if c.name == "burrow":
        hi = lo + 32
    mid = (lo + hi) // 2 - 8
    out = [("above_world", (mid[0], size, mid[2])), ("outside_x", (size + 5, mid[1], mid[2])), ("top_layer", (mid[0], size - 16, mid[2])),
           ("below_zero", (mid[0], -5, mid[2])), ("negative_lo", (-7, -3, -9)), ("far", (2147483647 - 20, -2147483648, 2147483647 - 3))]
    if c.name == "burrow":
        out.append(("in_rock", (48, 48, 48)))
    if c.name == "tower":
        out.append(("lod", (0, 4, 24)))  # z = 32: LOD 5 below, LOD 2 above
    if c.name == "far_chunks":
        a = c.info["lod_box"][0]
        out.append(("lod", (a[0] - 8, a[1] + 2, a[2] - 8)))
    if c.name == "lantern":
        out += [("roof_hole", (2, 4, 2)), ("glass_roof", (14, 6, 14)), ("two_emitters", (16, 2, 2)), ("wall", (6, 2, 14))]
    return out


SEALED = ((4, 2, 22), (5, 5, 5))  # lantern: the cube of rock with the lamp in its middle, as a box of its own


def make_boxes(c):
    """(int32 [N, 3], name -> index): the seeded set, then the named ones. A third of the seeded boxes is uniform over the occupied extent grown
    by 8; a third lies around cells that emit, a third around passable cells with something above them (both by the dense array, jittered by up
    to 6) -- where partly open tops, light around sources and both channels in one cell are found."""
    rng = np.random.default_rng(LIGHT_SEED[c.name])
    lo, hi = c.info["lo"], c.info["hi"]
    if c.name == "burrow":
        hi = lo + 32
    passes, emits = tables(c.props)
    t = c.truth[:hi[0] - lo[0], :hi[1] - lo[1], :hi[2] - lo[2]]
    sources = np.argwhere(emits[t] > 0)
    passable = passes[t]
    covered = np.argwhere(passable & ~np.logical_and.accumulate(passable[:, ::-1, :], axis=1)[:, ::-1, :])
    third = SEEDED // 3
    seeded = [rng.integers(lo - 8 - 8, hi + 8 - 8, (SEEDED - 2 * third, 3))]
    for cells in (sources, covered):
        if len(cells):
            at = cells[rng.integers(0, len(cells), third)] + lo - 8 + rng.integers(-6, 7, (third, 3))
        else:
            at = rng.integers(lo - 16, hi, (third, 3))
        seeded.append(at)
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


def in_form(boxes, stride):
    """(raw uint8 bytes, an (N, 3) int32 view of them at that stride) of boxes at a stride; what lies between them is not read."""
    n = len(boxes)
    padded = np.full((n, stride // 4), 0x5A5A5A5A, dtype=np.int32)
    padded[:, :3] = boxes
    raw = padded.reshape(-1).view(np.uint8).copy()
    view = np.ndarray((n, 3), dtype=np.int32, buffer=raw, offset=0, strides=(stride, 4))
    return raw, view


def torch_boxes(raw, stride, n):
    """The same view of a copy of the bytes in device memory."""
    import torch

    ints = torch.from_numpy(raw.copy()).cuda().view(torch.int32)
    return ints.as_strided((n, 3), (stride // 4, 1), 0)


# ---- the truth: plain numpy over the dense arrays ----------------------------------------------------------------------------------------------


def _around(level):
    """The largest of the six neighbours inside the box, of [N, z, y, x] levels (int16); 0 beyond the box."""
    m = np.zeros_like(level)
    m[:, 1:] = np.maximum(m[:, 1:], level[:, :-1])
    m[:, :-1] = np.maximum(m[:, :-1], level[:, 1:])
    m[:, :, 1:] = np.maximum(m[:, :, 1:], level[:, :, :-1])
    m[:, :, :-1] = np.maximum(m[:, :, :-1], level[:, :, 1:])
    m[:, :, :, 1:] = np.maximum(m[:, :, :, 1:], level[:, :, :, :-1])
    m[:, :, :, :-1] = np.maximum(m[:, :, :, :-1], level[:, :, :, 1:])
    return m


def _fixed_point(own, passable):
    """The per-cell rule iterated until nothing changes: a passable cell has max(own, largest neighbour - 1, 0), an impassable one `own`."""
    level = own.copy()
    for _ in range(64):
        new = np.where(passable, np.maximum(own, np.maximum(_around(level) - 1, 0)), own)
        if (new == level).all():
            return level
        level = new
    raise AssertionError("the light rule did not settle")


def light_truth(c, boxes, size, props, flags=0, truth=None):
    """(fields [N, padded] uint8 -- the voxels, then 0 up to the multiple of 16 --, LIGHT_INFO_DTYPE records [N]) of int boxes [N, 3] of one
    size; truth: the dense array to light instead of the case's (a world that has been changed)."""
    truth = c.truth if truth is None else truth
    sx, sy, sz = size
    n = len(boxes)
    passes, emits = tables(np.asarray(props, dtype=np.uint8))
    values = np.zeros((n, sz, sy, sx), dtype=np.uint32)
    open_above = np.ones((n, sz, sx), dtype=bool)
    top_of_chunks = int(c.info["hi"][1])  # above it, and beside the chunks, the world is air up to its top
    known = lambda v: np.where(v < len(passes), v, 0)
    for k, lo in enumerate(np.asarray(boxes, dtype=np.int64)):
        values[k] = dense_region(c.info, truth, lo, size)
        top = max(int(lo[1]) + sy, int(c.info["lo"][1]))  # (below the chunks is air as well)
        if top < top_of_chunks:
            above = dense_region(c.info, truth, (lo[0], top, lo[2]), (sx, top_of_chunks - top, sz))  # [z][y][x]: the whole column above the box
            open_above[k] = ((above == 0) | ((above < len(passes)) & passes[known(above)] if len(passes) else False)).all(axis=1)
    inside = values < len(passes)
    passable = (values == 0) | (inside & passes[known(values)] if len(passes) else False)
    emission = np.where(inside, emits[known(values)] if len(passes) else 0, 0).astype(np.int16)
    sky = np.zeros(values.shape, dtype=np.int16)
    block = np.zeros(values.shape, dtype=np.int16)
    info = np.zeros(n, dtype=hip.LIGHT_INFO_DTYPE)
    if not flags & NO_SKY:
        exposed = np.zeros(values.shape, dtype=bool)
        still = open_above
        for y in range(sy - 1, -1, -1):
            still = still & passable[:, :, y, :]
            exposed[:, :, y, :] = still
        sky = _fixed_point(np.where(exposed, 15, 0).astype(np.int16), passable)
        info["open_columns"] = exposed[:, :, sy - 1, :].sum(axis=(1, 2))
    if not flags & NO_BLOCKS:
        block = _fixed_point(emission, passable)
        info["sources"] = (emission > 0).sum(axis=(1, 2, 3))
        assert (block[~passable] == emission[~passable]).all()
    assert sky.max(initial=0) <= 15 and block.max(initial=0) <= 15 and (sky[~passable] == 0).all()
    byte = (sky << 4 | block).astype(np.uint8)
    bright = (sky >= 2) | (block >= 2)
    info["lit"] = (byte != 0).sum(axis=(1, 2, 3))
    faces = [bright[:, :, :, 0], bright[:, :, :, -1], bright[:, :, 0, :], bright[:, :, -1, :], bright[:, 0, :, :], bright[:, -1, :, :]]
    info["faces"] = sum(face.any(axis=(1, 2)).astype(np.uint32) << f for f, face in enumerate(faces))
    voxels = sx * sy * sz
    fields = np.zeros((n, (voxels + 15) // 16 * 16), dtype=np.uint8)
    fields[:, :voxels] = byte.reshape(n, -1)
    return fields, info


_TRUTHS = {}  # kept for the run: the two formats of a world share their truth (but `tower`'s, whose CSVO form has another chunk)


def calls_for(c):
    """[(name, shape, props, flags, lo_stride)]: every shape under the world's props, the strides in turn; at 16^3 off the brick grid also no
    props at all, a table that cuts the world's highest id off, and each of the two flags; the named boxes as they are."""
    out = [(shape.name, shape, c.props, 0, FORMS[i % 3]) for i, shape in enumerate(SHAPES)]
    off = SHAPE["16_off"]
    out += [("16_off-no_props", off, c.props[:0], 0, 12), ("16_off-cut", off, c.props[:-1], 0, 16), ("16_off-no_sky", off, c.props, NO_SKY, 64),
            ("16_off-no_blocks", off, c.props, NO_BLOCKS, 12), ("16", SIXTEEN, c.props, 0, 16)]
    return out


def truth_for(c, call):
    """light_truth of one of calls_for's calls on the case's boxes; kept."""
    name, shape, props, flags, _ = call
    key = (c.name, c.fmt if c.name == "tower" else "", name)
    if key not in _TRUTHS:
        fields, info = light_truth(c, boxes_for(c, shape), shape.size, props, flags)
        for a in (fields, info):
            a.setflags(write=False)
        _TRUTHS[key] = (fields, info)
    return _TRUTHS[key]


def cells(fields, shape):
    """(sky, block) [N, z, y, x] of fields."""
    f = fields[:, :shape.voxels].reshape(len(fields), shape.size[2], shape.size[1], shape.size[0])
    return f >> 4, f & 15


# ---- the host harness: a stand-alone program -----------------------------------------------------------------------------------------


def harness(sanitize=False):
    """tests/_build/light_on_host, or light_on_host_san: host_harness.build_harness's."""
    return build_harness("light_on_host", sanitize)


class HostLight(HostRunner):
    """The harness on one world: the frame is written once, every call is a run of the program."""

    def light(self, boxes, size, props, flags=0, lo_stride=12, field_stride=0, fields=True, info=True):
        """(fields [count, field_stride or padded] or None, LIGHT_INFO_DTYPE records or None)."""
        count = len(boxes)
        voxels = size[0] * size[1] * size[2]
        lo = self.put("lo.bin", in_form(np.asarray(boxes, dtype=np.int32).reshape(-1, 3), lo_stride)[0])
        self.put("props.bin", np.asarray(props, dtype=np.uint8))
        self.run("light", lo, lo_stride, count, *size, flags, self.path("props.bin", len(props)), field_stride, self.path("fields.bin", fields), self.path("info.bin", info))
        f = self.get("fields.bin", np.uint8, fields, (count, field_stride or (voxels + 15) // 16 * 16))
        i = self.get("info.bin", hip.LIGHT_INFO_DTYPE, info)
        assert i is None or len(i) == count
        return f, i

    def call(self, c, call, pick=None):
        """One of calls_for's calls on the case's boxes, or on those of them that `pick` indexes."""
        _, shape, props, flags, stride = call
        boxes = boxes_for(c, shape)
        return self.light(boxes if pick is None else boxes[pick], shape.size, props, flags, stride)


def differing(got_fields, got_info, exp_fields, exp_info):
    """A message naming the first box whose field or record differs, or None."""
    return outputs_differing((got_fields, got_info), (exp_fields, exp_info))
