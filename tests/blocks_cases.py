"""Shared by the tests of vx_block_points and vx_read_region (test_blocks_abi.py, test_blocks_on_host.py, test_blocks.py): batch_cases.py's two
worlds -- `glasshouse`, depth 6, one chunk; `far_chunks`, depth 14, 2 x 2 chunks at (400, 3, 401), one of them at LOD 3 --, a seeded point set
for each, and the ground truth of both: info["blocks"] and info["detail"], the dense copy the worlds were built from, with the LOD chunk's
voxels of 4 x 4 x 4 blocks worked out by the reference's pick_leaf_for_lod rule (internal.rs:461-485) restated here over the dense array.
Nothing of the code under test is used. Also the runner of the host harness (tests/cpp/blocks_on_host.cpp), a stand-alone program."""
import numpy as np

from batch_cases import BUILDERS
from host_harness import HostRunner, build_harness
from voxel_rs_amd import hip, host

OUTSIDE = 0xFFFFFFFF
POINT_SEED = {"glasshouse": 41, "far_chunks": 42}
LOD_ORDER = (2, 3, 6, 7, 0, 1, 4, 5)  # pick_leaf_for_lod's visiting order; a child's index is x | y << 1 | z << 2
REGIONS = {"glasshouse": ((-3, -3, -3), (70, 70, 70)),  # the whole world and a margin of 3 on every side
           "far_chunks": ((12795, 93, 12825), (75, 37, 77))}  # all four chunks (12800..12864, 96..128, 12832..12896) from an odd corner


def pick_octants(a):
    """One level of pick_leaf_for_lod over a dense [x][y][z] array of even sides: per 2 x 2 x 2 cell the first non-zero child in LOD_ORDER."""
    v = a.reshape(a.shape[0] // 2, 2, a.shape[1] // 2, 2, a.shape[2] // 2, 2)
    out = np.zeros((a.shape[0] // 2, a.shape[1] // 2, a.shape[2] // 2), dtype=a.dtype)
    for c in reversed(LOD_ORDER):  # (the first in the order is written last)
        child = v[:, c & 1, :, (c >> 1) & 1, :, c >> 2]
        out = np.where(child != 0, child, out)
    return out


def lod_voxels(cell, levels):
    """What a cell of side 2^levels shows as one voxel, and every aligned cell of that side of a larger array: pick_leaf_for_lod applied
    recursively -- the first sub-octant, in LOD_ORDER, that holds a block, and so on inside it."""
    for _ in range(levels):
        cell = pick_octants(cell)
    return cell


def lod_voxel(cell):
    """The id a 4 x 4 x 4 cell ([x][y][z]) of a LOD-3 chunk shows: the first 2^3 sub-octant, in LOD_ORDER, that holds a block, and in it the
    first block in the same order; 0 for a cell of air. (The LOD-3 case of lod_voxels.)"""
    return int(lod_voxels(np.asarray(cell), 2)[0, 0, 0])


def truth_of(info):
    """info["blocks"] as the serialized world shows it: unchanged where the world has full detail, per 4^3 cell the LOD voxel's id elsewhere."""
    t = info["blocks"].copy()
    if info["lod_box"] is not None:
        a, b = (v - info["lo"] for v in info["lod_box"])
        for x in range(a[0], b[0], 4):
            for y in range(a[1], b[1], 4):
                for z in range(a[2], b[2], 4):
                    t[x:x + 4, y:y + 4, z:z + 4] = lod_voxel(info["blocks"][x:x + 4, y:y + 4, z:z + 4])
    return t


def dense_region(info, truth, lo, size):
    """What vx_read_region has to give for the box: [z][y][x], zeros around the chunks."""
    lo, size = np.asarray(lo, dtype=np.int64), np.asarray(size, dtype=np.int64)
    out = np.zeros((size[2], size[1], size[0]), dtype=np.uint32)
    a, b = np.maximum(lo, info["lo"]), np.minimum(lo + size, info["hi"])
    if (a < b).all():
        src = truth[a[0] - info["lo"][0]:b[0] - info["lo"][0], a[1] - info["lo"][1]:b[1] - info["lo"][1], a[2] - info["lo"][2]:b[2] - info["lo"][2]]
        out[a[2] - lo[2]:b[2] - lo[2], a[1] - lo[1]:b[1] - lo[1], a[0] - lo[0]:b[0] - lo[0]] = src.transpose(2, 1, 0)
    return out


def classify(info, truth, pts):
    """Per point, by the dense arrays alone: the expected value, and the group it falls in -- `outside` the world (a component NaN, infinite,
    below 0 or at or above 2^depth), `space` (inside the world, outside every chunk), `lod` (inside the LOD chunk), `solid` / `air` (inside a
    full-detail chunk) -- and whether all its coordinates are integers."""
    p = np.asarray(pts, dtype=np.float32)
    size = np.float32(info["size"])
    with np.errstate(invalid="ignore"):
        inside = ((p >= 0) & (p < size)).all(axis=1)
    q = np.where(inside[:, None], np.floor(np.where(inside[:, None], p, 0)), 0).astype(np.int64)
    rel = q - info["lo"]
    in_box = inside & (rel >= 0).all(axis=1) & (rel < np.asarray(truth.shape)).all(axis=1)
    r = np.where(in_box[:, None], rel, 0)
    value = np.where(in_box, truth[r[:, 0], r[:, 1], r[:, 2]], 0).astype(np.uint32)
    detail = in_box & info["detail"][r[:, 0], r[:, 1], r[:, 2]]
    with np.errstate(invalid="ignore"):
        integral = inside & (p == np.floor(p)).all(axis=1)
    return dict(value=value, cell=q, outside=~inside, space=inside & ~in_box, lod=in_box & ~detail, solid=detail & (value != 0), air=detail & (value == 0),
                integral=integral)


def build_points(info, truth, seed):
    """About 2,000 float32 positions, shuffled: in solid blocks, in the air of the chunks, in the LOD chunk, in the empty space around the
    chunks near and far, outside the world (with NaN, +-inf, -1e-30 and exactly 2^depth; and -0.0f, which is inside), and on integer
    coordinates."""
    rng = np.random.default_rng(seed)
    lo, hi, size = info["lo"].astype(np.float64), info["hi"].astype(np.float64), info["size"]
    pts = []
    solid = np.argwhere((truth != 0) & info["detail"]) + info["lo"]
    by_id = [solid[truth[tuple((solid - info["lo"]).T)] == v] for v in np.unique(truth[(truth != 0) & info["detail"]])]
    for k in range(520):  # every id in turn, so that the rare ones (single blocks) are there too
        group = by_id[k % len(by_id)]
        pts.append(group[rng.integers(len(group))] + rng.uniform(0.0, 1.0, 3))
    while len(pts) < 520 + 560:  # anywhere in the chunks: mostly air
        pts.append(rng.uniform(lo, hi))
    if info["lod_box"] is not None:
        a, b = (v.astype(np.float64) for v in info["lod_box"])
        for _ in range(150):
            pts.append(rng.uniform(a, [b[0], a[1] + 14.0, b[2]]))  # (the terrain's part of the chunk: voxels and air)
        for _ in range(50):
            pts.append(rng.uniform(a, b))
    for k in range(260):  # empty space: a few blocks around the chunks, and anywhere in the world
        if k % 2:
            pts.append(rng.uniform(0.0, size, 3))
        else:
            p = rng.uniform(lo - 6.0, hi + 6.0)
            p[k % 3] = hi[k % 3] + rng.uniform(0.0, 6.0) if k % 4 else max(lo[k % 3] - rng.uniform(0.0, 6.0), 0.0)
            pts.append(np.clip(p, 0.0, size - 0.5))
    inside_point = lambda: rng.uniform(lo, hi)
    special = [np.nan, np.inf, -np.inf, -1e-30, size, -1.0, -1e-3, size + 0.5, 3.0e38, -3.0e38, float(np.nextafter(np.float32(size), np.float32(np.inf)))]
    for k in range(99):  # outside the world: one component (then two, then all three) beyond it
        p = inside_point()
        for a in range(1 + k // 33):
            p[(k + a) % 3] = special[(k + 5 * a) % len(special)]
        pts.append(p)
    for k in range(30):  # -0.0f is 0; the largest float below 2^depth is inside
        p = inside_point()
        p[k % 3] = -0.0 if k % 2 else float(np.nextafter(np.float32(size), np.float32(0)))
        pts.append(p)
    for k in range(120):  # integer coordinates: blocks' corners, the world's corner and its last voxel
        if k < 80:
            p = solid[rng.integers(len(solid))].astype(np.float64) + rng.integers(-1, 2, 3)
        elif k < 100:
            p = np.floor(inside_point())
        else:
            p = np.array([[0.0, 0.0, 0.0], [size - 1, size - 1, size - 1], [size - 1, 0.0, lo[2]], [lo[0], lo[1], 0.0]][k % 4])
        pts.append(p)
    pts = np.asarray(pts, dtype=np.float32)
    return np.ascontiguousarray(pts[rng.permutation(len(pts))])


class BlockCase:
    pass


def make_block_case(name, fmt):
    """A world in one format, its ground truth, its points and what they have to give; computed once, left unchanged."""
    c = BlockCase()
    c.name, c.fmt, c.svo_type = name, fmt, host.SVO_ESVO if fmt == "esvo" else host.SVO_CSVO
    c.world, c.scene, c.tex, c.mats, c.info = BUILDERS[name](c.svo_type)
    c.truth = truth_of(c.info)
    c.pts = build_points(c.info, c.truth, POINT_SEED[name])
    c.kinds = classify(c.info, c.truth, c.pts)
    c.frame = np.concatenate([c.world.frame(pad_words=0), np.zeros(4, dtype=np.uint32)])  # (with the 16 zero bytes a context keeps behind the world)
    for a in (c.truth, c.pts, c.frame, c.kinds["value"]):
        a.setflags(write=False)
    return c


def check_cells(c, cells, pts=None, kinds=None):
    """vx_block_cell records against the ground truth: every value; cell_log2 = 0 on full-detail blocks, 2 on LOD voxels, VX_CELL_OUTSIDE
    outside; for no block, the reported cell -- aligned to its size, holding floor(p) -- is all air in the dense array."""
    pts = c.pts if pts is None else pts
    k = c.kinds if kinds is None else kinds
    value, log2 = cells["value"], cells["cell_log2"]
    bad = np.flatnonzero(value != k["value"])
    assert not len(bad), f"{c.name}-{c.fmt}: {len(bad)} values differ, first at {bad[0]}: point {pts[bad[0]]!r} got {value[bad[0]]} expected {k['value'][bad[0]]}"
    assert (log2[k["outside"]] == OUTSIDE).all() and (log2[~k["outside"]] <= c.info["depth"]).all()
    assert (log2[k["solid"]] == 0).all()
    assert (log2[k["lod"] & (value != 0)] == 2).all()
    lo, shape = c.info["lo"], np.asarray(c.truth.shape)
    for i in np.flatnonzero(~k["outside"] & (value == 0)):
        side = 1 << int(log2[i])
        corner = k["cell"][i] // side * side  # aligned to its size and holding floor(p)
        a, b = np.maximum(corner - lo, 0), np.minimum(corner + side - lo, shape)
        if (a < b).all():
            assert not c.truth[a[0]:b[0], a[1]:b[1], a[2]:b[2]].any(), (i, pts[i], int(log2[i]))


# ---- the host harness: a stand-alone program -----------------------------------------------------------------------------------------


def harness():
    """tests/_build/blocks_on_host: host_harness.build_harness's."""
    return build_harness("blocks_on_host")


def host_points(exe, c, raw, stride, count):
    """`count` float[3] at `stride` bytes of `raw` (a uint8 array) through the harness: BLOCK_CELL_DTYPE records."""
    h = HostRunner(exe, c)
    h.run("points", h.put("points.bin", raw), stride, count, h.path("out.bin"))
    out = h.get("out.bin", hip.BLOCK_CELL_DTYPE)
    h.close()
    return out


def host_region(exe, c, lo, size):
    """The box through the harness's region routine: uint32 [z][y][x]."""
    h = HostRunner(exe, c)
    h.run("region", *lo, *size, h.path("out.bin"))
    out = h.get("out.bin", np.uint32, shape=(size[2], size[1], size[0]))
    h.close()
    return out
