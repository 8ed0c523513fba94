"""Shared by the tests of vx_move_boxes (test_move_abi.py, test_move_on_host.py, test_move.py): scan_cases.py's three worlds in both formats,
the boxes of each with their motions -- a seeded set of 2,000 and the named ones --, the forms they are handed over in (boxes_cases' five
forms of the box vectors; the motion packed, at stride 16, one for all, and as vx_entity.velocity in place with scale = 1/64), and the
expected record of each: plain numpy over the dense truth -- float32 adds, multiplies and subtractions in the rule's order, floor and ceil
in float64 of those float32 values, the clamps in Python integers, blocks_cases.dense_region of each slab, np.argwhere for the nearest layer
and its first voxel in [z][y][x] order. Nothing of the code under test is used. Also the runner of the host harness
(tests/cpp/move_on_host.cpp), a stand-alone program, plain and built with sanitizers."""
import math

import numpy as np

from blocks_cases import dense_region
from host_harness import HostRunner, build_harness, outputs_differing
from boxes_cases import FORMS, ONE_EXTENTS, Boxes, absent_id, box_truth, commonest_id, cover_of, invalid_boxes, resting_voxel
from list_cases import ANCHOR
from scan_cases import SCAN_CASES, make_scan_case  # noqa: F401  (the tests' parameters)
from voxel_rs_amd import hip

F = np.float32
INVALID = hip.VX_MOVE_INVALID
MOVE_SEED = {"glasshouse": 81, "far_chunks": 82, "tower": 83}
SEEDED = 2000
SKIN = 2.0 ** -10
YXZ, XYZ, ZYX = hip.VX_MOVE_ORDER_YXZ, hip.VX_MOVE_ORDER_XYZ, hip.VX_MOVE_ORDER_ZYX
ORDERS = {"yxz": YXZ, "xyz": XYZ, "zyx": ZYX}
ONE_MOTION = np.array([0.75, -1.5, -0.25], dtype=np.float32)  # the motion every box shares under `one`
VELOCITY_SCALE = 1.0 / 64.0


# ---- the truth: plain numpy over the dense arrays ----------------------------------------------------------------------------------------------


def invalid_record():
    r = np.zeros((), dtype=hip.MOVE_HIT_DTYPE)
    r["contacts"] = INVALID
    return r


def displacement_of(motion, scale):
    """d = motion * scale in float32; None for a record with no motion: a non-finite component of either, or |d| above 64."""
    m = np.asarray(motion, dtype=F)
    with np.errstate(over="ignore", invalid="ignore"):
        d = m * F(scale)
    if not (np.isfinite(m).all() and np.isfinite(d).all()) or (np.abs(d) > F(64)).any():
        return None
    return d


def _cut(first, last, size):
    return max(first, 0), min(last, size - 1)


def pass_truth(c, mn, mx, a, d, skin, only_value):
    """One pass: (m, found, value) for the box [mn, mx) moving by d != 0 along axis a."""
    first, last = [0, 0, 0], [0, 0, 0]
    for k in range(3):
        if k != a:
            first[k], last[k] = _cut(int(math.floor(float(mn[k]))), int(math.ceil(float(mx[k]))) - 1, c.size)
    if d > 0:
        end = mx[a] + (d + skin)
        first[a], last[a] = _cut(int(math.ceil(float(mx[a]))), int(math.ceil(float(end))) - 1, c.size)
    else:
        end = mn[a] + (d - skin)
        first[a], last[a] = _cut(int(math.floor(float(end))), int(math.floor(float(mn[a]))) - 1, c.size)
    if any(lo > hi for lo, hi in zip(first, last)):
        return d, 0, 0
    region = dense_region(c.info, c.truth, first, [hi - lo + 1 for lo, hi in zip(first, last)])  # [z][y][x]
    counted = region == only_value if only_value else region != 0
    ax = 2 - a
    layers = np.flatnonzero(counted.any(axis=tuple(k for k in range(3) if k != ax)))
    if not len(layers):
        return d, 0, 0
    n = int(layers[0] if d > 0 else layers[-1])
    at = tuple(np.argwhere(np.take(counted, n, axis=ax))[0])  # (ascending by z, then y, then x, without the axis)
    value = int(np.take(region, n, axis=ax)[at])
    v = first[a] + n
    zero = F(0)
    if d > 0:
        gap = F(v) - mx[a]
        m = np.minimum(d, np.maximum(zero, gap - skin))
    else:
        gap = mn[a] - F(v + 1)
        m = -np.minimum(-d, np.maximum(zero, gap - skin))
    return F(m), 1, value


def move_truth(c, origin, offset, extents, motion, scale, skin, order, only_value=0):
    """One box's MOVE_HIT_DTYPE record."""
    d3 = displacement_of(motion, scale)
    if cover_of(c, origin, offset, extents) is None or d3 is None:
        return invalid_record()
    o, e = np.array(origin, dtype=F), np.asarray(extents, dtype=F)
    f = None if offset is None else np.asarray(offset, dtype=F)
    skin = F(skin)
    mn = o.copy() if f is None else o + f
    mx = mn + e
    r = np.zeros((), dtype=hip.MOVE_HIT_DTYPE)
    contacts = 0
    for p in range(3):
        a = (order >> (2 * p)) & 3
        d = d3[a]
        m, found, value = (F(0), 0, 0) if d == 0 else pass_truth(c, mn, mx, a, d, skin, only_value)
        o[a] = o[a] + m
        mn[a] = o[a] if f is None else o[a] + f[a]
        mx[a] = mn[a] + e[a]
        r["moved"][a], r["value"][a] = m, value
        contacts |= found << (2 * a + (1 if d > 0 else 0))
    r["origin"], r["contacts"] = o, contacts
    return r


_TRUTHS = {}


def moves_truth(c, mv, scale=1.0, skin=SKIN, order=YXZ, only_value=0):
    """The records of a Moves, by its effective vectors (computed once for equal vectors, whatever form they come in)."""
    b = mv.boxes
    key = (c.name, c.fmt, b.origin.tobytes(), None if b.offset is None else b.offset.tobytes(), b.extents.tobytes(), mv.motion.tobytes(), float(F(scale)),
           float(F(skin)), order, only_value)
    if key not in _TRUTHS:
        out = np.zeros(len(b), dtype=hip.MOVE_HIT_DTYPE)
        for i in range(len(b)):
            out[i] = move_truth(c, b.origin[i], None if b.offset is None else b.offset[i], b.extents[i], mv.motion[i], scale, skin, order, only_value)
        out.setflags(write=False)
        _TRUTHS[key] = out
    return _TRUTHS[key]


# ---- boxes with motions, and the forms they are handed over in -------------------------------------------------------------------------------


class Moves:
    """A Boxes and the motion of each box (float32 [N, 3]) in one form (packed, stride16, one, velocity): the bytes a caller holds them all
    in and where each vector lies in them. `velocity`: the boxes are vx_entity records and .motion becomes their velocity field, 64 times
    the motion given (a call with scale = VELOCITY_SCALE moves the boxes as the motion given does with scale 1)."""

    def __init__(self, boxes, motion, form="packed"):
        self.boxes, self.form = boxes, form
        self.motion = np.ascontiguousarray(motion, dtype=np.float32)
        assert self.motion.shape == (len(boxes), 3)
        self.at = dict(boxes.at)
        if form == "velocity":
            assert boxes.form == "entities"
            e = boxes.raw.copy().view(hip.ENTITY_DTYPE)
            with np.errstate(over="ignore", invalid="ignore"):
                self.motion = self.motion * F(64)  # (exact, or an overflow to inf: no motion either way); .motion is what the call reads
            e["velocity"] = self.motion
            self.raw = e.view(np.uint8)
            self.at["motion"] = (hip.ENTITY_DTYPE.fields["velocity"][1], 64)
        else:
            if form == "one":
                assert len(boxes) == 0 or (self.motion == self.motion[0]).all()
                part = (self.motion[0] if len(boxes) else np.zeros(3, dtype=np.float32)).view(np.uint8)
                stride = 0
            elif form == "stride16":
                wide = np.full((len(boxes), 4), 7.5, dtype=np.float32)  # (what lies between the motions is not read)
                wide[:, :3] = self.motion
                part, stride = wide.reshape(-1).view(np.uint8), 16
            else:
                part, stride = self.motion.reshape(-1).view(np.uint8), 12
            self.at["motion"] = (len(boxes.raw), stride)
            self.raw = np.concatenate([boxes.raw, part])
        self.motion.setflags(write=False)
        self.raw.setflags(write=False)

    def __len__(self):
        return len(self.boxes)

    def _views(self, make):
        """The keyword arguments of Svo.move_boxes: [N, 3] at the form's stride, (3,) for a shared vector."""
        return {name: make(*self.at[name]) for name in ("origin", "extents", "motion", "offset") if name in self.at}

    def numpy_args(self):
        raw = self.raw
        return self._views(lambda at, stride: np.ndarray((len(self), 3) if stride else (3,), dtype=np.float32, buffer=raw, offset=at, strides=(stride, 4) if stride else (4,)))

    def torch_args(self):
        """The same views of a copy of the bytes in device memory (the uint8 tensor is kept alive by the views)."""
        import torch

        floats = torch.from_numpy(self.raw.copy()).cuda().view(torch.float32)
        return self._views(lambda at, stride: floats.as_strided((len(self), 3) if stride else (3,), (stride // 4, 1) if stride else (1,), at // 4))

    def picked(self, idx):
        """The boxes `idx` of this set, packed."""
        b = self.boxes
        return Moves(Boxes(b.origin[idx], None if b.offset is None else b.offset[idx], b.extents[idx], "packed" if b.offset is not None else "no_offset"), self.motion[idx])


def surface_voxels(c):
    """(voxel [x, y, z] in the dense array, face 0..5) of every block face that touches air (beyond the dense array is air)."""
    solid = c.truth != 0
    padded = np.pad(solid, 1)
    out = []
    for face in range(6):
        a, step = face >> 1, (1 if face & 1 else -1)
        beyond = np.roll(padded, -step, axis=a)[1:-1, 1:-1, 1:-1]
        at = np.argwhere(solid & ~beyond)
        out.append(np.concatenate([at, np.full((len(at), 1), face)], axis=1))
    return np.concatenate(out)


def seeded_moves(c, seed):
    """(origin, offset, extents, motion) of 2,000 boxes. Half start resting on or beside the surface: a block face that touches air is drawn,
    the box overlaps it across and its near face lies exactly on it (3 in 10), up to 1.5 in front of it (5 in 10) or up to 0.6 behind it
    (2 in 10); most of them move towards the block. Half are drawn uniformly over the world's populated box grown by 4 voxels. Extents from 0.3
    to 12, small ones more often; displacements from 0 to 20 an axis, 8 in 10 under 2, one component in 10 exactly 0. The origin is the box's
    centre and the offset minus half the extents, as an entity holds them."""
    rng = np.random.default_rng(seed)
    lo, hi = c.info["lo"].astype(np.float64), c.info["hi"].astype(np.float64)
    faces = surface_voxels(c)
    half = SEEDED // 2
    extents = np.where(rng.uniform(size=(SEEDED, 3)) < 0.7, rng.uniform(0.3, 3.0, (SEEDED, 3)), rng.uniform(3.0, 12.0, (SEEDED, 3)))
    extents = extents.astype(np.float32).astype(np.float64)
    size = np.where(rng.uniform(size=(SEEDED, 3)) < 0.8, rng.uniform(0.0, 2.0, (SEEDED, 3)), rng.uniform(2.0, 20.0, (SEEDED, 3)))
    motion = size * rng.choice([-1.0, 1.0], (SEEDED, 3))
    motion[rng.uniform(size=(SEEDED, 3)) < 0.1] = 0.0
    mn = rng.uniform(lo - 4.0, hi + 4.0, (SEEDED, 3)) - extents / 2
    for i in range(half):
        x, y, z, face = (int(v) for v in faces[rng.integers(len(faces))])
        a, out = face >> 1, bool(face & 1)
        voxel = lo + (x, y, z)
        mn[i] = voxel + rng.uniform(0.05 - extents[i], 0.95)
        kind = rng.uniform()
        gap = 0.0 if kind < 0.3 else (rng.uniform(0.0, 1.5) if kind < 0.8 else -rng.uniform(0.0, 0.6))
        mn[i, a] = voxel[a] + 1.0 + gap if out else voxel[a] - gap - extents[i, a]
        if rng.uniform() < 0.85:
            motion[i, a] = -abs(motion[i, a]) if out else abs(motion[i, a])  # towards the block
            if motion[i, a] == 0.0:
                motion[i, a] = -0.5 if out else 0.5
    order = rng.permutation(SEEDED)
    extents32 = extents.astype(np.float32)[order]
    offset = (-extents32 / np.float32(2)).astype(np.float32)
    origin = (mn[order] - offset.astype(np.float64)).astype(np.float32)
    return origin, offset, extents32, motion.astype(np.float32)[order]


def edge_voxel(c):
    """A block with two voxels of air on top whose +x neighbour column is air from one voxel below its top to two above: a box that comes
    down diagonally over that edge lands on the block when x goes first and beside it when y does. World coordinates."""
    t = c.truth
    ok = np.zeros(t.shape, dtype=bool)
    ok[:-1, 1:-2, :] = ((t[:-1, 1:-2, :] != 0) & (t[:-1, 2:-1, :] == 0) & (t[:-1, 3:, :] == 0) & (t[1:, :-3, :] == 0) & (t[1:, 1:-2, :] == 0)
                        & (t[1:, 2:-1, :] == 0) & (t[1:, 3:, :] == 0))
    at = np.argwhere(ok)
    assert len(at), "no block edge of that kind in this world"
    return c.info["lo"] + at[len(at) // 2]


def named_moves(c):
    """[(name, origin, offset, extents, motion)], each named for what it catches."""
    size, lo = float(c.size), c.info["lo"]
    g = np.asarray(ANCHOR[c.name], dtype=np.float64)
    rest = resting_voxel(c).astype(np.float64)
    edge = edge_voxel(c).astype(np.float64)
    zero = (0.0, 0.0, 0.0)
    one = ONE_EXTENTS
    above = float(np.nextafter(np.float32(64), np.float32(65)))
    base = lo.astype(np.float64) if c.name == "far_chunks" else np.zeros(3)
    out = [("resting_down", rest + (0.1, 1.0, 0.1), zero, one, (0.0, -0.5, 0.0)),                     # mn.y exactly the block's top: gap 0
           ("hover_down", rest + (0.1, 1.0 + SKIN, 0.1), zero, one, (0.0, -0.5, 0.0)),              # 2^-10 above it
           ("hover_quarter", rest + (0.1, 1.25, 0.1), zero, one, (0.0, -0.5, 0.0)),                 # a gap of 0.25: a skin of 0.5 is larger
           ("sunk_up", rest + (0.1, 0.5, 0.1), zero, one, (0.0, 0.5, 0.0)),                          # half a voxel in the ground, up and out
           ("sunk_sideways", rest + (0.1, 0.5, 0.1), zero, one, (0.75, 0.0, 0.0)),
           ("sunk_down", rest + (0.1, 0.5, 0.1), zero, one, (0.0, -0.25, 0.0)),                      # the block it is in is no obstacle
           ("diagonal", edge + (1.2, 1.2, 0.1), zero, (0.8, 0.8, 0.8), (-0.5, -0.5, 0.0)),           # past the block's edge: the order decides
           ("travel_64", g + (0.5, 40.5, 0.5), zero, (1.0, 1.0, 1.0), (64.0, -64.0, 64.0)),
           ("travel_above_64", g + (0.5, 40.5, 0.5), zero, (1.0, 1.0, 1.0), (above, 0.0, 0.0)),      # no motion
           ("travel_above_64_z", g + (0.5, 40.5, 0.5), zero, (1.0, 1.0, 1.0), (0.0, 0.0, -above)),
           # the largest slab: a cross-section of 65 x 65 voxels and 65 layers off the brick grid, 9 bricks each (a world of 64: what it has)
           ("widest", base + (np.array([3.5, 67.5, 3.5]) if size >= 128 else np.array([-2.5, 62.5, -2.5])), zero, (64.0, 64.0, 64.0), (0.0, -64.0, 0.0)),
           ("widest_diagonal", base + (np.array([-60.5, 131.5, -60.5]) if size >= 128 else np.array([-60.5, 70.5, -60.5])), zero, (64.0, 64.0, 64.0), (64.0, -64.0, 64.0)),
           ("into_the_world", (-6.5, rest[1] + 1.5, rest[2] + 0.1), zero, one, (12.0, 0.0, 0.0)),
           ("out_of_the_world", (2.5, rest[1] + 1.5, rest[2] + 0.1), zero, one, (-12.0, 0.0, 0.0)),
           ("out_of_the_top", (rest[0] + 0.1, size - 3.5, rest[2] + 0.1), zero, one, (0.0, 9.0, 0.0)),
           ("in_from_the_top", (rest[0] + 0.1, size + 3.5, rest[2] + 0.1), zero, one, (0.0, -9.0, 0.0)),
           ("below_the_world", (rest[0] + 0.1, -9.5, rest[2] + 0.1), zero, one, (0.5, -3.0, 0.5)),
           ("far_x", (3e9, 10.0, 10.0), zero, (2.0, 2.0, 2.0), (1.0, -1.0, 1.0)),
           ("far_negative", (10.0, -3e9, 10.0), zero, (2.0, 2.0, 2.0), (-1.0, 1.0, -1.0)),
           ("far_huge", (10.0, 10.0, 1e30), zero, (2.0, 2.0, 2.0), (1.0, 1.0, -1.0)),
           ("far_all", (3e9, -3e9, 1e30), (1e30, 3e9, -3e9), (64.0, 0.5, 2.0), (-64.0, 64.0, 0.5)),
           ("minus_zero", rest + (0.1, 1.0, 0.1), zero, one, (-0.0, -0.5, 0.0)),
           ("minus_zero_all", rest + (0.1, 1.0, 0.1), zero, one, (-0.0, -0.0, -0.0)),
           ("still", rest + (0.1, 1.0, 0.1), zero, one, zero),
           ("fall_through", rest + (0.1, 1.5, 0.1), zero, one, (0.0, -6.0, 0.0))]                     # (only_value: an id that occurs nowhere)
    for word, bad in (("nan", np.nan), ("inf", np.inf), ("-inf", -np.inf), ("1e30", 1e30), ("-3e38", -3e38)):
        for a in range(3):
            m = np.array([0.25, -0.25, 0.25])
            m[a] = bad
            out.append((f"motion_{word}_{a}", rest + (0.1, 1.5, 0.1), zero, one, m))
    if c.name == "tower":
        out.append(("lod_seam", (4.3, 12.2, 24.5), zero, (3.0, 3.0, 3.0), (0.0, 0.0, 12.0)))        # across z = 32: LOD 5 below, LOD 2 above
        out.append(("lod_seam_back", (4.3, 2.2, 36.5), zero, (3.0, 3.0, 3.0), (0.5, -0.5, -12.0)))
        out.append(("lod_leaf_16", (70.5, 125.5, 40.5), zero, (2.0, 2.0, 2.0), (5.0, -30.0, 5.0)))  # inside the chunk of leaves of side 16 (CSVO: 8)
        out.append(("lod_leaf_16_up", (70.5, 97.5, 40.5), zero, (2.0, 2.0, 2.0), (-20.0, 20.0, -20.0)))
    return out


def make_moves(c):
    """The world's boxes with their motions in the packed form: the seeded set, then the named ones and boxes_cases' records that are no
    box (each with a motion of its own); .names: name -> index; .seeded, .named, .no_box: index arrays."""
    so, sf, se, sm = seeded_moves(c, MOVE_SEED[c.name])
    named = named_moves(c)
    rows = named + [(r[0], r[1], r[2], r[3], (0.25, -0.5, 0.125)) for r in invalid_boxes(c)]
    col = lambda k: np.array([r[k] for r in rows], dtype=np.float64).astype(np.float32)
    with np.errstate(over="ignore"):
        boxes = Boxes(np.concatenate([so, col(1)]), np.concatenate([sf, col(2)]), np.concatenate([se, col(3)]), "packed")
        mv = Moves(boxes, np.concatenate([sm, col(4)]))
    mv.names = {r[0]: SEEDED + k for k, r in enumerate(rows)}
    mv.seeded, mv.named, mv.no_box = np.arange(SEEDED), np.arange(SEEDED, SEEDED + len(named)), np.arange(SEEDED + len(named), len(boxes))
    return mv


def in_forms(mv, box_form, motion_form):
    """The same boxes and motions in other forms; where a form shares a vector among all boxes, or has no offset, they are other boxes and
    motions (boxes_cases.Boxes.in_form; ONE_MOTION)."""
    boxes = mv.boxes if box_form == mv.boxes.form else mv.boxes.in_form(box_form)
    motion = np.broadcast_to(ONE_MOTION, mv.motion.shape) if motion_form == "one" else mv.motion
    return Moves(boxes, motion, motion_form)


def calls_for(c, mv):
    """[(name, Moves, dict(scale, skin, order, only_value))]: every form of the boxes, every form of the motion, the three orders, a skin of 0
    and one of 0.5, the commonest id of the world and an id that occurs nowhere."""
    base = dict(scale=1.0, skin=SKIN, order=YXZ, only_value=0)
    out = [(form, in_forms(mv, form, "packed"), dict(base)) for form in FORMS]
    out += [("motion_" + form, in_forms(mv, "packed", form), dict(base)) for form in ("stride16", "one")]
    out.append(("motion_velocity", in_forms(mv, "entities", "velocity"), dict(base, scale=VELOCITY_SCALE)))
    out += [(name, mv, dict(base, order=order)) for name, order in ORDERS.items() if order != YXZ]
    out += [("skin_0", mv, dict(base, skin=0.0)), ("skin_half", mv, dict(base, skin=0.5)), ("scale_half", mv, dict(base, scale=0.5))]
    out += [("commonest", mv, dict(base, only_value=commonest_id(c))), ("absent", mv, dict(base, only_value=absent_id(c)))]
    return out


def overlaps_at(c, mv, origin):
    """boxes_cases.box_truth's count for each box of `mv` standing at `origin` (INVALID for a record that is no box)."""
    b = mv.boxes
    return np.array([int(box_truth(c, origin[i], None if b.offset is None else b.offset[i], b.extents[i])["blocks"]) for i in range(len(b))], dtype=np.int64)


# ---- the host harness: a stand-alone program -----------------------------------------------------------------------------------------


def harness(sanitize=False):
    """tests/_build/move_on_host, or move_on_host_san: host_harness.build_harness's."""
    return build_harness("move_on_host", sanitize, float_cast=True)


def float_bits(v):
    return f"{int(np.array(v, dtype=np.float32).view(np.uint32)):08x}"


class HostMoves(HostRunner):
    """The harness on one world: the frame is written once, every call is a run of the program."""

    def records(self, mv, scale=1.0, skin=SKIN, order=YXZ, only_value=0):
        at = mv.at
        self.run("move", self.put("raw.bin", mv.raw), len(mv), *at["origin"], *at.get("offset", (-1, 0)), *at["extents"], *at["motion"], only_value, float_bits(scale),
                 float_bits(skin), order, self.path("out.bin"))
        out = self.get("out.bin", hip.MOVE_HIT_DTYPE)
        assert len(out) == len(mv)
        return out


def differing(got, exp):
    """A message naming the first differing record of two MOVE_HIT_DTYPE arrays, or None. (Equal bytes: -0.0 is not 0.0, the padding counts.)"""
    return outputs_differing((got,), (exp,))
