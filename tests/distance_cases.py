"""Shared by the tests of vx_distance_boxes (test_distance_abi.py, test_distance_on_host.py, test_distance.py): label_cases.py's five worlds in
both formats with their boxes -- a pick of the seeded set, half uniform and half around the surface, and the named ones --; the shapes,
the forms the boxes are handed over in (packed, at stride 16 and 20, inside a larger record) and the expected field and record of every box.

The truth is plain numpy over blocks_cases.dense_region of each box, in integers, two ways that must agree: the three separable passes, each
a broadcast minimum over the 32 x 32 matrix of (i - j)^2 (distance_truth), and for a box of at most 12^3 cells the minimum over all target
cells of the squared distance itself (brute_force). `where` and `farthest` come from argmax over the field in its own order. Nothing of the
code under test is used.
Also the runner of the host harness (tests/cpp/distance_on_host.cpp), a stand-alone program, plain and built with sanitizers."""
import numpy as np

from host_harness import HostRunner, build_harness, outputs_differing
from label_cases import LABEL_CASES, SEEDED, _faces_of, make_label_case, pass_id, regions_of
from light_cases import in_form, torch_boxes  # noqa: F401  (the forms of lo are vx_light_boxes')
from voxel_rs_amd import hip

NONE, TO_AIR = hip.VX_DISTANCE_NONE, hip.VX_DISTANCE_TO_AIR
DISTANCE_CASES = LABEL_CASES
FORMS = (12, 16, 20, 64)  # lo_stride
FAR = 1 << 20  # "no target" inside the truth: above every sum of real values and squares, far below an int32's end
SQUARES = (np.arange(32)[:, None] - np.arange(32)[None, :]) ** 2  # [i, j]
BRUTE_CELLS = 12 ** 3
SMALL_PICK, LARGE_PICK = 60, 12  # seeded boxes a call of at most, and of more than, 17^3 cells is made on (and every named one)


class Shape:
    """The box of a call. snap: None -- the boxes' lo as they are; else every seeded lo is moved down to a multiple of 8 and `snap` added."""

    def __init__(self, name, size, snap=None):
        self.name, self.size, self.snap = name, tuple(size), snap
        self.voxels = size[0] * size[1] * size[2]
        self.bytes = (2 * self.voxels + 15) // 16 * 16  # of a field, as written
        self.entries = self.bytes // 2


# sizes 1, 7, 8, 9, 17, 31 and 32 on an axis; on the brick grid, off it by 1, 4 and 7 (at 32: five bricks an axis); not cubic
SHAPES = [Shape("1", (1, 1, 1)), Shape("7", (7, 7, 7)), Shape("8_one_brick", (8, 8, 8), (0, 0, 0)), Shape("9_two_bricks", (9, 9, 9), (4, 4, 4)), Shape("17", (17, 17, 17)),
          Shape("31", (31, 31, 31)), Shape("32", (32, 32, 32)), Shape("32_off_1", (32, 32, 32), (1, 1, 1)), Shape("32_off_7", (32, 32, 32), (7, 7, 7)),
          Shape("32x1x5", (32, 1, 5)), Shape("1x32x32", (1, 32, 32)), Shape("31x3x17", (31, 3, 17))]
SHAPE = {s.name: s for s in SHAPES}
SEVENTEEN = SHAPE["17"]


def make_distance_case(name, fmt):
    """label_cases' world in one format, its dense truth and its boxes; computed once, left unchanged."""
    return make_label_case(name, fmt)


def boxes_for(c, shape):
    """The case's boxes as the shape wants them: unchanged, or the seeded ones moved to a multiple of 8 plus shape.snap."""
    if shape.snap is None:
        return c.boxes
    b = c.boxes.copy()
    b[:SEEDED] = (b[:SEEDED] // 8) * 8 + np.array(shape.snap, dtype=np.int32)
    return b


def pick_for(c, shape):
    """The boxes a call of this shape is made on: SMALL_PICK or LARGE_PICK of the seeded ones, half of them of each kind (uniform, then around
    the surface), and every named one."""
    half = (SMALL_PICK if shape.voxels <= 17 ** 3 else LARGE_PICK) // 2
    uniform = SEEDED - 2 * (SEEDED // 3)
    return np.concatenate([np.arange(half), np.arange(uniform, uniform + half), np.arange(SEEDED, len(c.boxes))])


def named_at(c, shape, name):
    """Where among pick_for's boxes the named box lies."""
    return len(pick_for(c, shape)) - (len(c.boxes) - c.names[name])


# ---- the truth: plain numpy over the dense arrays ----------------------------------------------------------------------------------------------


def targets_of(values, pass_value=0, match_value=0, flags=0):
    """bool, of values' shape: the rule of include/voxel_hip.h."""
    if match_value:
        t = values == match_value
    else:
        t = (values != 0) & ((values != pass_value) if pass_value else True)
    return ~t if flags & TO_AIR else t


def _min_plus(d, axis):
    """out[.., i, ..] = min_j(d[.., j, ..] + (i - j)^2) along `axis`, a few boxes at a time (the broadcast has 32 times the cells)."""
    d = np.moveaxis(d, axis, -1)
    n = d.shape[-1]
    out = np.empty_like(d)
    step = max(1, (1 << 22) // max(1, d[0].size * n))
    for k in range(0, len(d), step):
        out[k:k + step] = (d[k:k + step, ..., None, :] + SQUARES[:n, :n]).min(axis=-1)
    return np.moveaxis(out, -1, axis)


def distance_field(target):
    """uint16 [N, z, y, x]: the squared distance to the nearest True cell of each box; NONE where a box has none."""
    d = np.where(target, 0, FAR).astype(np.int32)
    for axis in (3, 2, 1):
        d = _min_plus(d, axis)
    return np.where(d >= FAR, NONE, d).astype(np.uint16)


def brute_force(target):
    """The same for one box [z, y, x], by the definition: the minimum over all target cells."""
    cells = np.argwhere(np.ones(target.shape, dtype=bool))
    at = np.argwhere(target)
    if not len(at):
        return np.full(target.shape, NONE, dtype=np.uint16)
    return ((cells[:, None, :] - at[None, :, :]) ** 2).sum(axis=-1).min(axis=1).astype(np.uint16).reshape(target.shape)


def derive(target, shape):
    """(fields uint16 [N, shape.entries], DISTANCE_INFO_DTYPE [N]) of target [N, z, y, x]."""
    n = len(target)
    field = distance_field(target)
    fields = np.full((n, shape.entries), NONE, dtype=np.uint16)
    fields[:, :shape.voxels] = field.reshape(n, -1)
    info = np.zeros(n, dtype=hip.DISTANCE_INFO_DTYPE)
    flat = fields[:, :shape.voxels]
    first = flat.argmax(axis=1)  # (the first of the largest, in the field's order)
    sx, sy = shape.size[0], shape.size[1]
    info["targets"] = target.reshape(n, -1).sum(axis=1)
    info["farthest"] = flat[np.arange(n), first] if n else 0
    info["where"] = (first % sx) | (first // sx % sy) << 8 | (first // (sx * sy)) << 16
    info["faces"] = [_faces_of(t) for t in target]
    return fields, info


def distance_truth(c, boxes, shape, pass_value=0, match_value=0, flags=0, truth=None):
    """derive() for any boxes (not kept); shape: a Shape, or a size; truth: the dense array to measure instead of the case's."""
    shape = shape if isinstance(shape, Shape) else Shape("", shape)
    return derive(targets_of(regions_of(c, boxes, shape.size, truth), pass_value, match_value, flags), shape)


def match_id(c):
    """An id that is present: the one pass_id picks (the commonest, or the link's)."""
    return pass_id(c)


ABSENT = 0x7FFF1234  # no world holds it


def calls_for(c):
    """[(name, shape, pass_value, match_value, flags, lo_stride, field_stride)]: every shape under the four kinds of target set -- solid, its
    complement, solid without the pass value, the cells of one id -- with the strides in turn (field_stride 0, or 48 bytes more than a field);
    and at 17^3 an id that is absent, without and with the flag, the complement of one id and of the pass rule."""
    out = []
    kinds = (("solid", 0, 0, 0), ("air", 0, 0, TO_AIR), ("pass", pass_id(c), 0, 0), ("match", 0, match_id(c), 0))
    for i, shape in enumerate(SHAPES):
        for j, (kind, pass_value, match_value, flags) in enumerate(kinds):
            k = i + j
            out.append((f"{shape.name}-{kind}", shape, pass_value, match_value, flags, FORMS[k % 4], shape.bytes + 48 if k % 3 == 1 else 0))
    out.append(("17-absent", SEVENTEEN, 0, ABSENT, 0, 12, 0))
    out.append(("17-absent-air", SEVENTEEN, 0, ABSENT, TO_AIR, 20, 0))
    out.append(("17-match-air", SEVENTEEN, 0, match_id(c), TO_AIR, 16, SEVENTEEN.bytes + 48))
    out.append(("17-pass-air", SEVENTEEN, pass_id(c), 0, TO_AIR, 64, 0))
    return out


def the_call(c, name):
    return [call for call in calls_for(c) if call[0] == name][0]


_TRUTHS = {}  # kept for the run: the two formats of a world share their truth (but `tower`'s, whose CSVO form has another chunk)


def truth_for(c, call):
    """(fields [N, shape.entries], info) of one of calls_for's calls on the boxes pick_for gives; kept."""
    name, shape, pass_value, match_value, flags, _, _ = call
    key = (c.name, c.fmt if c.name == "tower" else "", name)
    if key not in _TRUTHS:
        got = distance_truth(c, boxes_for(c, shape)[pick_for(c, shape)], shape, pass_value, match_value, flags)
        for a in got:
            a.setflags(write=False)
        _TRUTHS[key] = got
    return _TRUTHS[key]


def cells(fields, shape):
    """[N, z, y, x] of fields."""
    return fields[:, :shape.voxels].reshape(len(fields), shape.size[2], shape.size[1], shape.size[0])


def unpack(word):
    return int(word) & 0xFF, int(word) >> 8 & 0xFF, int(word) >> 16 & 0xFF


# ---- the host harness: a stand-alone program -----------------------------------------------------------------------------------------


def harness(sanitize=False):
    """tests/_build/distance_on_host, or distance_on_host_san: host_harness.build_harness's."""
    return build_harness("distance_on_host", sanitize)


class HostDistance(HostRunner):
    """The harness on one world: the frame is written once, every call is a run of the program."""

    def distance(self, boxes, size, pass_value=0, match_value=0, flags=0, lo_stride=12, field_stride=0, fields=True, info=True):
        """(fields uint16 [count, (field_stride or a field's bytes) / 2] or None, DISTANCE_INFO_DTYPE records or None); what the call left
        untouched reads 0x5a5a."""
        count = len(boxes)
        voxels = size[0] * size[1] * size[2]
        lo = self.put("lo.bin", in_form(np.asarray(boxes, dtype=np.int32).reshape(-1, 3), lo_stride)[0])
        self.run("distance", lo, lo_stride, count, *size, pass_value, match_value, flags, field_stride, self.path("fields.bin", fields), self.path("info.bin", info))
        f = self.get("fields.bin", np.uint16, fields, (count, (field_stride or (2 * voxels + 15) // 16 * 16) // 2))
        i = self.get("info.bin", hip.DISTANCE_INFO_DTYPE, info)
        assert i is None or len(i) == count
        return f, i

    def call(self, c, call, pick=None):
        """One of calls_for's calls on the boxes pick_for gives, or on those of them that `pick` indexes: (the fields' written entries, info)."""
        _, shape, pass_value, match_value, flags, lo_stride, field_stride = call
        boxes = boxes_for(c, shape)[pick_for(c, shape)]
        f, i = self.distance(boxes if pick is None else boxes[pick], shape.size, pass_value, match_value, flags, lo_stride, field_stride)
        assert (f[:, shape.entries:] == 0x5A5A).all(), "entries beyond the field were written"
        return f[:, :shape.entries], i


def differing(got, expected):
    """A message naming the first box whose field or record differ between two (fields, info), or None."""
    return outputs_differing(got, expected)
