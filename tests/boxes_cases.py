"""Shared by the tests of vx_overlap_boxes (test_boxes_abi.py, test_boxes_on_host.py, test_boxes.py): scan_cases.py's three worlds in both
formats, the boxes of each -- a seeded set of 2,000 and the named ones --, the forms their vectors are handed over in (packed arrays, no
offset, one extents or one offset vector for every box, vx_entity records), and the expected record of each box: plain numpy over the dense
truth -- mn and mx by float32 adds in the call's order, floor and ceil in float64 of those float32 values, the clamp in Python integers,
blocks_cases.dense_region of the cover, the count, np.argwhere for the bounds and the first voxel in [z][y][x] order. Nothing of the code under
test is used. Also the runner of the host harness (tests/cpp/boxes_on_host.cpp), a stand-alone program, plain and built with sanitizers."""
import math

import numpy as np

from blocks_cases import dense_region
from host_harness import HostRunner, build_harness, outputs_differing
from list_cases import ANCHOR
from scan_cases import SCAN_CASES, make_scan_case  # noqa: F401  (the tests' parameters)
from voxel_rs_amd import hip

INVALID = hip.VX_BOX_INVALID
BOX_SEED = {"glasshouse": 61, "far_chunks": 62, "tower": 63}
SEEDED = 2000
FORMS = ("packed", "no_offset", "one_extents", "one_offset", "entities")
ONE_EXTENTS = np.array([0.8, 1.8, 0.8], dtype=np.float32)  # the vector every box shares under one_extents, one_offset
ONE_OFFSET = np.array([-0.4, 0.0, -0.4], dtype=np.float32)
FLT_MAX = float(np.finfo(np.float32).max)


# ---- the truth: plain numpy over the dense arrays ----------------------------------------------------------------------------------------------


def invalid_record():
    r = np.zeros((), dtype=hip.BOX_HIT_DTYPE)
    r["blocks"] = INVALID
    return r


def cover_of(c, origin, offset, extents):
    """(first, last) of the box's cover as Python ints per axis; None for a record that is no box. offset None: mn = origin."""
    o, e = np.asarray(origin, dtype=np.float32), np.asarray(extents, dtype=np.float32)
    f = None if offset is None else np.asarray(offset, dtype=np.float32)
    given = (o, e) if f is None else (o, f, e)
    if not all(np.isfinite(v).all() for v in given) or not ((e > 0) & (e <= 64)).all():
        return None
    with np.errstate(over="ignore", invalid="ignore"):
        mn = o if f is None else o + f  # (float32 adds)
        mx = mn + e
    if not (np.isfinite(mn).all() and np.isfinite(mx).all()):
        return None
    first = [max(int(math.floor(float(v))), 0) for v in mn]
    last = [min(int(math.ceil(float(v))) - 1, c.size - 1) for v in mx]
    return first, last


def box_truth(c, origin, offset, extents, only_value=0):
    """One box's BOX_HIT_DTYPE record."""
    cover = cover_of(c, origin, offset, extents)
    if cover is None:
        return invalid_record()
    r = np.zeros((), dtype=hip.BOX_HIT_DTYPE)
    first, last = cover
    if any(a > b for a, b in zip(first, last)):
        return r
    region = dense_region(c.info, c.truth, first, [b - a + 1 for a, b in zip(first, last)])  # [z][y][x]
    counted = region == only_value if only_value else region != 0
    at = np.argwhere(counted)  # (ascending by z, then y, then x)
    if not len(at):
        return r
    r["blocks"], r["value"] = len(at), region[tuple(at[0])]
    r["lo"] = [first[a] + int(at[:, 2 - a].min()) for a in range(3)]
    r["hi"] = [first[a] + int(at[:, 2 - a].max()) + 1 for a in range(3)]
    return r


def boxes_truth(c, boxes, only_value=0):
    """The records of a Boxes, by its effective vectors."""
    out = np.zeros(len(boxes), dtype=hip.BOX_HIT_DTYPE)
    for i in range(len(boxes)):
        out[i] = box_truth(c, boxes.origin[i], None if boxes.offset is None else boxes.offset[i], boxes.extents[i], only_value)
    return out


# ---- boxes and the forms they are handed over in -------------------------------------------------------------------------------------------------


class Boxes:
    """N boxes by their effective vectors (float32 [N, 3]; offset None: there is none) in one form: the bytes a caller holds them in and
    where each vector lies in them."""

    def __init__(self, origin, offset, extents, form, names=None):
        self.origin, self.extents = (np.ascontiguousarray(v, dtype=np.float32) for v in (origin, extents))
        self.offset = None if offset is None else np.ascontiguousarray(offset, dtype=np.float32)
        self.form, self.names = form, names or {}
        n = len(self.origin)
        assert (form == "no_offset") == (self.offset is None)
        if form == "entities":
            e = np.zeros(n, dtype=hip.ENTITY_DTYPE)
            e["position"], e["aabb_offset"], e["aabb_extents"] = self.origin, self.offset, self.extents
            e["velocity"], e["gravity"], e["flags"] = 0.25, 9.81, 0x5a5a5a5a  # (what lies between the vectors is not read)
            self.raw = e.view(np.uint8).copy()
            self.at = dict(origin=(0, 64), offset=(24, 64), extents=(36, 64))
        else:
            parts, self.at, size = [], {}, 0
            for name, v, shared in (("origin", self.origin, False), ("offset", self.offset, form == "one_offset"), ("extents", self.extents, form == "one_extents")):
                if v is None:
                    continue
                if shared:
                    assert (v == v[0]).all()
                part = (v[0] if shared else v).reshape(-1).view(np.uint8)
                self.at[name] = (size, 0 if shared else 12)
                parts.append(part)
                size += len(part)
            self.raw = np.concatenate(parts)
        for a in (self.origin, self.extents, self.raw) + (() if self.offset is None else (self.offset,)):
            a.setflags(write=False)

    def __len__(self):
        return len(self.origin)

    def _views(self, make):
        """(origin, extents, offset) as Svo.overlap_boxes takes them: [N, 3] at the form's stride, (3,) for a shared vector, None."""
        out = []
        for name in ("origin", "extents", "offset"):
            if name not in self.at:
                out.append(None)
                continue
            at, stride = self.at[name]
            out.append(make(at, stride))
        return tuple(out)

    def numpy_args(self):
        raw = self.raw
        return self._views(lambda at, stride: np.ndarray((len(self), 3) if stride else (3,), dtype=np.float32, buffer=raw, offset=at, strides=(stride, 4) if stride else (4,)))

    def torch_args(self):
        """The same views of a copy of the bytes in device memory (the uint8 tensor is kept alive by the views)."""
        import torch

        floats = torch.from_numpy(self.raw.copy()).cuda().view(torch.float32)
        return self._views(lambda at, stride: floats.as_strided((len(self), 3) if stride else (3,), (stride // 4, 1) if stride else (1,), at // 4))

    def in_form(self, form):
        """The same boxes in another form; where the form shares a vector among all boxes, or has no offset, they are other boxes: every box
        gets ONE_EXTENTS / ONE_OFFSET, or its mn as the origin."""
        o, f, e = self.origin, self.offset, self.extents
        if form == "no_offset":
            with np.errstate(over="ignore", invalid="ignore"):
                o, f = o + f, None
        elif form == "one_extents":
            e = np.broadcast_to(ONE_EXTENTS, e.shape)
        elif form == "one_offset":
            f = np.broadcast_to(ONE_OFFSET, f.shape)
        return Boxes(o, f, e, form, self.names)

    def tiled(self, count):
        idx = np.arange(count) % len(self)
        return Boxes(self.origin[idx], None if self.offset is None else self.offset[idx], self.extents[idx], self.form), idx


def seeded_boxes(c, seed):
    """(origin, offset, extents) of 2,000 boxes: half with their centre inside a solid voxel (centre = voxel + u, u in (0.05, 0.95); extents in
    (0.1, 9)), so that they overlap by construction; half drawn uniformly over the world's populated box grown by 4 voxels. The origin is the
    box's centre and the offset minus half the extents, as an entity holds them."""
    rng = np.random.default_rng(seed)
    lo, hi = c.info["lo"].astype(np.float64), c.info["hi"].astype(np.float64)
    solid = np.argwhere(c.truth != 0)
    half = SEEDED // 2
    centre = np.concatenate([lo + solid[rng.integers(len(solid), size=half)] + rng.uniform(0.05, 0.95, (half, 3)),
                             rng.uniform(lo - 4.0, hi + 4.0, (SEEDED - half, 3))])
    extents = rng.uniform(0.1, 9.0, (SEEDED, 3)).astype(np.float32)
    order = rng.permutation(SEEDED)
    origin, extents = centre.astype(np.float32)[order], extents[order]
    return origin, (-extents / np.float32(2)).astype(np.float32), extents


def resting_voxel(c):
    """A block with two voxels of air on top of it, in world coordinates: a box of ONE_EXTENTS standing on it covers only that air."""
    t = c.truth
    ok = (t[:, :-2, :] != 0) & (t[:, 1:-1, :] == 0) & (t[:, 2:, :] == 0)
    at = np.argwhere(ok)
    return c.info["lo"] + at[len(at) // 2]


def named_boxes(c):
    """[(name, origin, offset, extents)], each named for what it catches."""
    size, lo = float(c.size), c.info["lo"]
    solid = lo + np.argwhere(c.truth != 0)[len(np.argwhere(c.truth != 0)) // 3]
    g = np.asarray(ANCHOR[c.name], dtype=np.float64)
    rest = resting_voxel(c).astype(np.float64)
    zero = (0.0, 0.0, 0.0)
    out = [("resting", rest + (0.1, 1.0, 0.1), zero, ONE_EXTENTS),                       # mn.y exactly the block's top: the block does not count
           ("sunk", rest + (0.1, 1.0 - 2.0 ** -10, 0.1), zero, ONE_EXTENTS),             # 2^-10 lower: it counts
           ("one_voxel", solid + 0.25, zero, (0.5, 0.5, 0.5)),
           ("eight_bricks", g + 4.5, zero, (8.0, 8.0, 8.0)),                            # a cover 9 wide: two bricks on every axis
           ("widest", (lo if c.name == "far_chunks" else 0.0) + np.array([-2.5, -2.5, -2.5]), zero, (64.0, 64.0, 64.0)),  # nine bricks an axis
           ("world_edge_near", (0.0, 0.0, 0.0), (-3.5, -2.5, -1.5), (9.0, 9.0, 9.0)),    # mn negative, mx inside the world
           ("world_edge_far", (size - 5.5, size - 4.5, size - 6.5), zero, (12.0, 12.0, 12.0)),  # mx beyond the far edge
           ("chunks_corner", c.info["hi"] - 3.5, zero, (9.0, 9.0, 9.0)),
           ("outside_below", (-20.0, -20.0, -20.0), zero, (5.0, 5.0, 5.0)),
           ("outside_above", (size + 3.0, size + 3.0, size + 3.0), zero, (5.0, 5.0, 5.0)),
           ("outside_one_axis", (solid[0], size, solid[2]), zero, (3.0, 3.0, 3.0)),       # mn exactly at the world's far edge
           ("touching_edge", (solid[0] + 0.5, -2.0, solid[2] + 0.5), zero, (1.0, 2.0, 1.0)),  # mx.y exactly 0: no voxel
           ("far_x", (3e9, 10.0, 10.0), zero, (2.0, 2.0, 2.0)),
           ("far_negative", (10.0, -3e9, 10.0), zero, (2.0, 2.0, 2.0)),
           ("far_huge", (10.0, 10.0, 1e30), zero, (2.0, 2.0, 2.0)),
           ("far_all", (3e9, -3e9, 1e30), (1e30, 3e9, -3e9), (64.0, 0.5, 2.0)),
           ("far_max", (FLT_MAX, 10.0, 10.0), zero, (64.0, 2.0, 2.0)),                   # (FLT_MAX + 64 rounds to FLT_MAX: mx stays finite)
           ("minus_zero", (-0.0, -0.0, -0.0), (-0.0, 0.0, -0.0), (2.5, 2.5, 2.5))]
    if c.name == "tower":
        out.append(("lod_seam", (4.3, 2.2, 27.5), zero, (10.0, 9.0, 9.5)))                  # across z = 32: LOD 5 below, LOD 2 above
        out.append(("lod_leaves", (60.5, 90.5, 30.5), zero, (40.0, 40.0, 36.0)))            # leaves of side 8 and 16 against the world's edge
    return out


def invalid_boxes(c):
    """[(name, origin, offset, extents)] that describe no box: NaN and +-inf in each component of each of the three vectors, an extent of 0,
    -1, 64.001 (and the next float above 64), and a sum that overflows to inf. (mn + extents itself cannot overflow: an extent is at most 64
    and FLT_MAX + 64 rounds to FLT_MAX -- `far_max` above, a valid box; the add that can is origin + offset.)"""
    base = (c.info["lo"] + (5.0, 3.0, 5.0), (-0.4, 0.0, -0.4), (0.8, 1.8, 0.8))
    out = []
    for v, vector in enumerate(("origin", "offset", "extents")):
        for bad, word in ((np.nan, "nan"), (np.inf, "inf"), (-np.inf, "-inf")):
            for a in range(3):
                vecs = [np.array(x, dtype=np.float64) for x in base]
                vecs[v][a] = bad
                out.append((f"{word}_{vector}_{a}", *vecs))
    for bad in (0.0, -0.0, -1.0, 64.001, float(np.nextafter(np.float32(64), np.float32(65))), 1e30):
        for a in range(3):
            vecs = [np.array(x, dtype=np.float64) for x in base]
            vecs[2][a] = bad
            out.append((f"extent_{bad}_{a}", *vecs))
    out.append(("overflow_mn", (3e38, 1.0, 1.0), (3e38, 0.0, 0.0), (1.0, 1.0, 1.0)))
    out.append(("overflow_mn_negative", (1.0, -3e38, 1.0), (0.0, -3e38, 0.0), (1.0, 1.0, 1.0)))
    out.append(("overflow_mn_z", (1.0, 1.0, FLT_MAX), (0.0, 0.0, FLT_MAX), (64.0, 64.0, 64.0)))
    return out


def make_boxes(c):
    """The world's boxes in the packed form: the seeded set, then the named and the invalid ones; .names: name -> index; .seeded, .named,
    .invalid: index arrays."""
    so, sf, se = seeded_boxes(c, BOX_SEED[c.name])
    rows = named_boxes(c) + invalid_boxes(c)
    origin = np.concatenate([so, np.array([r[1] for r in rows], dtype=np.float64).astype(np.float32)])
    offset = np.concatenate([sf, np.array([r[2] for r in rows], dtype=np.float64).astype(np.float32)])
    extents = np.concatenate([se, np.array([r[3] for r in rows], dtype=np.float64).astype(np.float32)])
    names = {r[0]: SEEDED + k for k, r in enumerate(rows)}
    b = Boxes(origin, offset, extents, "packed", names)
    n_named = len(named_boxes(c))
    b.seeded, b.named, b.invalid = np.arange(SEEDED), np.arange(SEEDED, SEEDED + n_named), np.arange(SEEDED + n_named, len(origin))
    return b


def commonest_id(c):
    ids, counts = np.unique(c.truth[c.truth != 0], return_counts=True)
    return int(ids[counts.argmax()])


def absent_id(c):
    return int(c.truth.max()) + 1000


def calls_for(c, boxes):
    """[(name, Boxes, only_value)]: every form with every block counted, and the packed form with the commonest id of the world and with an id
    that occurs nowhere."""
    out = [(form, boxes.in_form(form), 0) for form in FORMS]
    out.append(("commonest", boxes, commonest_id(c)))
    out.append(("absent", boxes, absent_id(c)))
    return out


# ---- the host harness: a stand-alone program -----------------------------------------------------------------------------------------


def harness(sanitize=False):
    """tests/_build/boxes_on_host, or boxes_on_host_san: host_harness.build_harness's."""
    return build_harness("boxes_on_host", sanitize, float_cast=True)


class HostBoxes(HostRunner):
    """The harness on one world: the frame is written once, every call is a run of the program."""

    def records(self, boxes, only_value=0):
        at = boxes.at
        self.run("boxes", self.put("raw.bin", boxes.raw), len(boxes), *at["origin"], *at.get("offset", (-1, 0)), *at["extents"], only_value, self.path("out.bin"))
        out = self.get("out.bin", hip.BOX_HIT_DTYPE)
        assert len(out) == len(boxes)
        return out


def differing(got, exp):
    """A message naming the first differing record of two BOX_HIT_DTYPE arrays, or None."""
    return outputs_differing((got,), (exp,))
