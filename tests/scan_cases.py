"""Shared by the tests of vx_scan_points and vx_scan_columns (test_scan_abi.py, test_scan_on_host.py, test_scan.py): three worlds --
blocks_cases.py's `glasshouse` (depth 6: a ceiling, floating blocks and walls, so that up, down and sideways differ) and `far_chunks` (depth
14: a scan from the world's top crosses empty cells of 2^13 down to 1; one chunk at LOD 3), and `tower`, built here: five chunks of seeded
random columns with overhangs, one at each of LOD 5, 4, 3, 2 and 1 (leaves of side 1, 2, 4, 8 and 16), in a 3 x 4 x 2 arrangement of chunk
positions with an empty position between two occupied ones along y and along x (an arrangement only two positions wide cannot hold the
latter). A CSVO chunk at LOD 1 is one leaf-mask byte with no depth-2 node above it inside the chunk (csvo.rs:437-463), and read_leaf
(svo.csvo.glsl:119-133) finds a leaf's block id through that node's material section offset: the format holds no readable ids for such a
chunk, for the reference's shader as for vx_block_points, so the CSVO tower has a second chunk at LOD 2 in that place (leaves of side 8,
which still end the descent above the brick) --, a seeded point set and a list of boxes for each, and the ground truth of both: per column the first non-zero of the dense array
along the axis within the range, and the cell size from the chunk's LOD. Plain numpy over the dense arrays the worlds were built from
(blocks_cases.lod_voxels for the LOD chunks); nothing of the code under test is used. Also the runner of the host harness
(tests/cpp/scan_on_host.cpp), a stand-alone program."""
import numpy as np

from batch_cases import _chunk_of
from blocks_cases import dense_region, lod_voxels, make_block_case
from helpers import vra
from host_harness import HostRunner, build_harness
from voxel_rs_amd import hip, host

NONE, OUTSIDE, TO_EDGE = hip.VX_SCAN_NONE, hip.VX_CELL_OUTSIDE, hip.VX_SCAN_TO_EDGE
DIRECTIONS = list(range(6))
DIR_NAMES = ["-x", "+x", "-y", "+y", "-z", "+z"]
WORLDS = ("glasshouse", "far_chunks", "tower")
SCAN_CASES = [(name, fmt) for name in WORLDS for fmt in ("esvo", "csvo")]
POINT_SEED = {"glasshouse": 51, "far_chunks": 52, "tower": 53}
GAP = 5  # the voxels of air, start included, in front of the block of a `gap` point: reach GAP ends one voxel short of it, GAP + 1 on it
REACHES = (1, 2, TO_EDGE)
TOWER_CHUNKS = (((0, 0, 0), 5), ((0, 2, 0), 4), ((2, 0, 0), 3), ((0, 0, 1), 2), ((2, 3, 1), 1))  # (chunk position, LOD); (0, 1, 0), (1, 0, 0) stay empty


def axes_of(direction):
    """(a, u, v, positive): the scan axis, the two other axes u < v, and whether travel is towards larger coordinates."""
    a = direction >> 1
    return a, (1 if a == 0 else 0), (1 if a == 2 else 2), bool(direction & 1)


def tower_blocks(rng):
    """One chunk's blocks [x][y][z]: random columns, a slab that overhangs part of them, scattered single blocks."""
    b = np.zeros((32, 32, 32), dtype=np.uint32)
    for x in range(32):
        for z in range(32):
            b[x, :4 + int(rng.integers(0, 9)), z] = int(rng.choice([1, 2, 3, 7, 9]))
    x0, z0 = (int(v) for v in rng.integers(0, 12, size=2))
    b[x0:x0 + 14, 20:23, z0:z0 + 17] = 4  # the overhang
    b[x0 + 3:x0 + 6, 23:29, z0 + 2] = 12
    for _ in range(60):
        x, y, z = (int(v) for v in rng.integers(0, 32, size=3))
        b[x, y, z] = int(rng.choice([5, 10, 4]))
    return b


def tower(svo_type):
    """(world, info): the tower world, depth 7; info as batch_cases' worlds have it, with the dense truth and the per-voxel cell sizes."""
    rng = np.random.default_rng(17)
    shape = (96, 128, 64)
    blocks, truth, cell = (np.zeros(shape, dtype=np.uint32) for _ in range(3))
    world = vra.World(svo_type)
    for pos, lod in TOWER_CHUNKS:
        b = tower_blocks(rng)
        if lod == 1 and svo_type == host.SVO_CSVO:
            lod = 2  # (see the module's docstring: the CSVO format cannot hold a chunk at LOD 1)
        world.set_chunk(pos, _chunk_of(pos, lod, b))
        k = 5 - lod  # a voxel of the chunk is a cell of side 2^k
        v = lod_voxels(b, k)
        for axis in range(3):
            v = np.repeat(v, 1 << k, axis=axis)
        at = tuple(slice(32 * p, 32 * p + 32) for p in pos)
        blocks[at], truth[at], cell[at] = b, v, k
    world.serialize()
    assert world.depth == 7
    lo = np.zeros(3, dtype=np.int64)
    info = dict(name="tower", svo_type=svo_type, depth=world.depth, size=float(1 << world.depth), lo=lo, hi=lo + np.asarray(shape), blocks=blocks,
                detail=cell == 0, lod_box=None)
    return world, info, truth, cell


class ScanCase:
    pass


def make_scan_case(name, fmt):
    """A world in one format, its dense truth (values and log2 cell sizes), its points and boxes; computed once, left unchanged."""
    from voxel_rs_amd import scenes

    c = ScanCase()
    c.name, c.fmt, c.svo_type = name, fmt, host.SVO_ESVO if fmt == "esvo" else host.SVO_CSVO
    if name == "tower":
        c.world, c.info, c.truth, c.cell = tower(c.svo_type)
        c.tex, c.mats = scenes.synthetic_textures(), scenes.synthetic_materials()
        c.frame = np.concatenate([c.world.frame(pad_words=0), np.zeros(4, dtype=np.uint32)])
    else:
        b = make_block_case(name, fmt)
        c.world, c.info, c.truth, c.tex, c.mats, c.frame = b.world, b.info, b.truth, b.tex, b.mats, b.frame
        c.cell = np.where(c.info["detail"], 0, 2).astype(np.uint32)  # (the one LOD chunk of these worlds is at LOD 3)
    c.size = int(c.info["size"])
    c.pts, c.groups = build_scan_points(c, POINT_SEED[name])
    c.gaps = {d: gap_points(c, d, POINT_SEED[name] + 10 + d) for d in DIRECTIONS}
    for a in (c.truth, c.cell, c.pts, c.frame) + tuple(c.gaps.values()):
        a.setflags(write=False)
    return c


# ---- the truth: plain numpy over the dense arrays ----------------------------------------------------------------------------------------------


def none_records(shape, cell_log2=0):
    r = np.zeros(shape, dtype=hip.SCAN_HIT_DTYPE)
    r["coord"], r["cell_log2"] = NONE, cell_log2
    return r


def column_truth(c, start, direction, reach):
    """One column: the record of the scan from the integer voxel `start` (any Python ints) over `reach` voxels."""
    a, u, v, positive = axes_of(direction)
    rec = none_records(())
    if not (0 <= start[u] < c.size and 0 <= start[v] < c.size):
        return rec
    r0, r1 = (start[a], start[a] + reach - 1) if positive else (start[a] - reach + 1, start[a])
    lo, hi = c.info["lo"], c.info["hi"]
    r0, r1 = max(r0, 0, int(lo[a])), min(r1, c.size - 1, int(hi[a]) - 1)  # (outside the dense array everything is air)
    if r0 > r1 or not (lo[u] <= start[u] < hi[u] and lo[v] <= start[v] < hi[v]):
        return rec
    at = [0, 0, 0]
    at[u], at[v], at[a] = start[u] - lo[u], start[v] - lo[v], slice(r0 - lo[a], r1 + 1 - lo[a])
    col = c.truth[tuple(at)]
    hit = np.flatnonzero(col)
    if len(hit):
        k = int(hit[0] if positive else hit[-1])
        rec["coord"], rec["value"], rec["cell_log2"] = r0 + k, col[k], c.cell[tuple(at)][k]
    return rec


def start_of(p):
    """floor(p) per component saturated to int32, as Python ints; None for a position with a NaN or infinite component."""
    if not np.isfinite(p).all():
        return None
    return [int(min(max(np.floor(np.float64(x)), -2.0 ** 31), 2.0 ** 31 - 1)) for x in p]


def points_truth(c, pts, direction, reach):
    out = none_records(len(pts))
    for i, p in enumerate(pts):
        s = start_of(p)
        out[i] = none_records((), OUTSIDE) if s is None else column_truth(c, s, direction, reach)
    return out


def columns_truth(c, lo, size, direction):
    """The box's records, [v - lo.v][u - lo.u]: the first non-zero of the dense array along the axis, from the face the scan enters."""
    a, u, v, positive = axes_of(direction)
    out = none_records((size[v], size[u]))
    if not all(size):
        return out
    lo, size = list(lo), list(size)
    r0, r1 = max(lo[a], 0, int(c.info["lo"][a])), min(lo[a] + size[a], c.size, int(c.info["hi"][a]))  # (beyond the dense array: air)
    if r0 >= r1:
        return out
    lo[a], size[a] = r0, r1 - r0
    val, cell = (dense_region(c.info, t, lo, size) for t in (c.truth, c.cell))  # [z][y][x]
    ax = 2 - a
    some = (val != 0).any(axis=ax)
    first = (val != 0).argmax(axis=ax) if positive else val.shape[ax] - 1 - (np.flip(val, axis=ax) != 0).argmax(axis=ax)
    pick = lambda t: np.take_along_axis(t, np.expand_dims(first, ax), axis=ax).squeeze(ax)
    # (a column outside the world holds no block in the dense array either)
    out["coord"] = np.where(some, r0 + first, NONE)
    out["value"], out["cell_log2"] = np.where(some, pick(val), 0), np.where(some, pick(cell), 0)
    return out


def first_of_region(region, lo, direction):
    """(coord, value) per column of a vx_read_region array [z][y][x] of the box at `lo`: its first non-zero along the axis in travel order."""
    a, _, _, positive = axes_of(direction)
    ax = 2 - a
    some = (region != 0).any(axis=ax)
    first = (region != 0).argmax(axis=ax) if positive else region.shape[ax] - 1 - (np.flip(region, axis=ax) != 0).argmax(axis=ax)
    value = np.take_along_axis(region, np.expand_dims(first, ax), axis=ax).squeeze(ax)
    return np.where(some, lo[a] + first, NONE), np.where(some, value, 0)


# ---- points ------------------------------------------------------------------------------------------------------------------------------


def build_scan_points(c, seed):
    """(about 1,500 float32 positions, shuffled; group name -> indices): in the air above the terrain, inside solid blocks, inside LOD voxels
    away from the cell's faces, in the air under something (the glasshouse's ceiling, the overhangs), in the empty space beside the chunks,
    outside the world on each side (in line with the chunks and not), on integer coordinates, and with -0.0f, NaN, +-inf and +-3e38."""
    rng = np.random.default_rng(seed)
    lo, hi, size = c.info["lo"].astype(np.float64), c.info["hi"].astype(np.float64), float(c.size)
    truth, cell = c.truth, c.cell
    pts, groups = [], {}

    def add(group, p):
        groups.setdefault(group, []).append(len(pts))
        pts.append(np.asarray(p, dtype=np.float64))

    solid = np.argwhere(truth != 0)
    full = solid[cell[tuple(solid.T)] == 0]
    top = np.where((truth != 0).any(axis=1), truth.shape[1] - 1 - (truth[:, ::-1, :] != 0).argmax(axis=1), -1)  # [x][z]: the highest block
    held = np.argwhere(top >= 0)  # the columns that hold a block
    for _ in range(300):
        x, z = (int(v) for v in held[rng.integers(len(held))])
        add("above", lo + [x + rng.uniform(), top[x, z] + 1 + rng.uniform(0.0, 12.0), z + rng.uniform()])
    for _ in range(260):
        add("solid", lo + full[rng.integers(len(full))] + rng.uniform(0.05, 0.95, 3))
    inner = solid[(cell[tuple(solid.T)] >= 2) & (((solid & ((1 << cell[tuple(solid.T)]) - 1)[:, None]) != 0).all(axis=1))
                  & (((solid + 1) & ((1 << cell[tuple(solid.T)]) - 1)[:, None]) != 0).all(axis=1)]
    for _ in range(200 if len(inner) else 0):
        add("lod_inner", lo + inner[rng.integers(len(inner))] + rng.uniform(0.05, 0.95, 3))
    lod = np.argwhere(cell != 0)
    for _ in range(100 if len(lod) else 0):
        add("lod", lo + lod[rng.integers(len(lod))] + rng.uniform(0.05, 0.95, 3))
    covered = np.argwhere((truth == 0) & (np.flip(np.maximum.accumulate(np.flip(truth != 0, axis=1), axis=1), axis=1)))  # air with a block above it
    if c.name == "glasshouse":
        covered = covered[(covered[:, 0] >= 4) & (covered[:, 0] < 16) & (covered[:, 2] >= 18) & (covered[:, 2] < 30) & (covered[:, 1] < 12)]  # under the ceiling
    for _ in range(200):
        add("covered", lo + covered[rng.integers(len(covered))] + rng.uniform(0.05, 0.95, 3))
    for k in range(150):  # the empty space beside the chunks, inside the world
        p = rng.uniform(lo - 6.0, hi + 6.0)
        p[k % 3] = hi[k % 3] + rng.uniform(0.0, 6.0) if k % 2 else lo[k % 3] - rng.uniform(0.0, 6.0)
        add("space", np.clip(p, 0.0, size - 0.5))
    for k in range(120):  # outside the world: in line with the chunks (a scan along that axis enters it) and not
        axis, far, aligned = k % 3, (k // 3) % 2, (k // 6) % 2
        p = rng.uniform(lo, hi) if aligned else rng.uniform(-8.0, size + 8.0, 3)
        p[axis] = size + rng.uniform(0.0, 8.0) if far else -rng.uniform(0.001, 8.0)
        add("outside", p)
    for k in range(100):  # integer coordinates
        add("integral", np.floor(rng.uniform(lo - 2.0, hi + 2.0)) if k % 2 else lo + solid[rng.integers(len(solid))] + rng.integers(-1, 2, 3))
    special = [-0.0, np.nan, np.inf, -np.inf, 3.0e38, -3.0e38]
    for k in range(72):
        p = rng.uniform(lo, hi)
        for n in range(1 + k // 36):
            p[(k + n) % 3] = special[(k // 3 + 2 * n) % len(special)]
        add("special", p)
    pts = np.asarray(pts, dtype=np.float32)
    order = rng.permutation(len(pts))
    back = np.argsort(order)
    return np.ascontiguousarray(pts[order]), {g: np.sort(back[np.asarray(i)]) for g, i in groups.items()}


def gap_points(c, direction, seed):
    """40 positions with exactly GAP voxels of air, the start included, in front of a block along `direction`."""
    a, _, _, positive = axes_of(direction)
    rng = np.random.default_rng(seed)
    step = np.zeros(3, dtype=np.int64)
    step[a] = 1 if positive else -1
    solid = np.argwhere(c.truth != 0)
    out = []
    for i in rng.permutation(len(solid)):
        b = solid[i]
        before = [b - k * step for k in range(1, GAP + 1)]
        if all((q < 0).any() or (q >= c.truth.shape).any() or c.truth[tuple(q)] == 0 for q in before):
            out.append(c.info["lo"] + before[-1] + rng.uniform(0.05, 0.95, 3))
            if len(out) == 40:
                break
    assert len(out) == 40
    return np.ascontiguousarray(np.asarray(out, dtype=np.float32))


# ---- boxes -------------------------------------------------------------------------------------------------------------------------------


def boxes_for(c, direction):
    """[(name, lo, size)] for one direction: 1 x 1 columns; 9 x 1 across a tile boundary; the whole world with a margin of 3 (a world too wide for one call: the chunks with that margin); a footprint one
    voxel off the tile grid; a box wholly outside the world; a range along the axis that starts inside a LOD voxel (worlds that have one);
    one that ends one voxel before the first block, and one voxel later."""
    a, u, v, positive = axes_of(direction)
    lo, hi, size = c.info["lo"], c.info["hi"], c.size
    solid = np.argwhere(c.truth != 0)
    mid = [int(x) for x in lo + solid[len(solid) // 2]]  # a voxel that holds a block: every column through it finds one

    def box(name, blo, bsize):
        return name, tuple(int(x) for x in blo), tuple(int(x) for x in bsize)

    def through(point, footprint):
        """the box over the whole world along the axis, its footprint starting at `point`"""
        blo, bsize = list(point), [0, 0, 0]
        blo[a], bsize[a], bsize[u], bsize[v] = 0, size, footprint[0], footprint[1]
        return blo, bsize

    out = [box("1x1", *through(mid, (1, 1)))]
    p = list(mid)
    p[u] = p[u] // 8 * 8 + (4 if p[u] % 8 >= 4 else -4)  # (nine columns across a tile boundary, the one through `mid` among them)
    out.append(box("9x1", *through(p, (9, 1))))
    out.append(box("world+3", (-3, -3, -3), (size + 6,) * 3) if size <= 128 else box("chunks+3", lo - 3, hi - lo + 6))
    p = [int(x) // 8 * 8 + 1 for x in lo]
    out.append(box("off_grid", *through(p, (23, 18))))
    out.append(box("outside", (size + 8, -20, size), (9, 10, 11)))
    out.append(box("beside", *through([-24, -24, -24], (17, 9))))
    if (c.cell >= 2).any():  # the extent starts inside a LOD voxel (not at its face in travel order) and covers the footprint of 2 x 2 of them
        s = np.argwhere((c.cell >= 2) & (c.truth != 0))
        s = s[len(s) // 2]
        k = int(c.cell[tuple(s)])
        corner = lo + (s >> k << k)
        blo, bsize = [int(x) for x in corner], [2 << k] * 3
        blo[u] -= 1  # (and a column beside them)
        if positive:
            blo[a] += 1
        bsize[a] = (1 << k) - 1 if not positive else 2 << k
        out.append(box("in_lod", blo, bsize))
    # around the first gap point, GAP voxels of air in front of a block: an extent that stops one voxel before the block, and on it
    g = [int(np.floor(x)) for x in c.gaps[direction][0]]
    for name, extent in (("short", GAP), ("exact", GAP + 1)):
        blo, bsize = [g[0] - 2, g[1] - 2, g[2] - 2], [5, 5, 5]
        blo[a], bsize[a] = (g[a] if positive else g[a] - extent + 1), extent
        out.append(box(name, blo, bsize))
    return out


def skipping_box(c):
    """far_chunks: the four chunks' footprint plus a margin of 8, the world's full height."""
    lo, hi = c.info["lo"], c.info["hi"]
    return (int(lo[0]) - 8, 0, int(lo[2]) - 8), (int(hi[0] - lo[0]) + 16, c.size, int(hi[2] - lo[2]) + 16)


# ---- the host harness: a stand-alone program -----------------------------------------------------------------------------------------


def harness():
    """tests/_build/scan_on_host: host_harness.build_harness's."""
    return build_harness("scan_on_host")


def host_scan_points(exe, c, raw, stride, count, direction, reach):
    """`count` float[3] at `stride` bytes of `raw` through the harness: (SCAN_HIT_DTYPE records, loop trips a point)."""
    h = HostScans(exe, c)
    h.run("points", h.put("points.bin", raw), stride, count, direction, reach, h.path("out.bin"), h.path("trips.bin"))
    out = h.get("out.bin", hip.SCAN_HIT_DTYPE), h.get("trips.bin", np.uint32)
    h.close()
    return out


def host_scan_columns(exe, c, lo, size, direction):
    """The box through the harness's columns routine: (SCAN_HIT_DTYPE records [v][u], loop trips a tile)."""
    h = HostScans(exe, c)
    out = h.columns(lo, size, direction), h.get("trips.bin", np.uint32)
    h.close()
    return out


class HostScans(HostRunner):
    """The harness on one world for many calls (a streamed frame of several MB): the frame is written once, every call is a run of the program.
    The records of host_scan_points and host_scan_columns, without the trips."""

    def points(self, pts, direction, reach):
        pts = np.ascontiguousarray(pts, dtype=np.float32)
        self.run("points", self.put("points.bin", pts), 12, len(pts), direction, reach, self.path("out.bin"), self.path("trips.bin"))
        return self.get("out.bin", hip.SCAN_HIT_DTYPE)

    def columns(self, lo, size, direction):
        _, u, v, _ = axes_of(direction)
        self.run("columns", *lo, *size, direction, self.path("out.bin"), self.path("trips.bin"))
        return self.get("out.bin", hip.SCAN_HIT_DTYPE, shape=(size[v], size[u]))


def differing(got, exp):
    """A message naming the first differing record of two SCAN_HIT_DTYPE arrays, or None. (Equal bytes: the padding too.)"""
    if got.shape != exp.shape:
        return f"shapes differ: {got.shape} vs {exp.shape}"
    if got.tobytes() == exp.tobytes():
        return None
    bad = np.argwhere(got.view(np.uint32).reshape(got.shape + (4,)) != exp.view(np.uint32).reshape(exp.shape + (4,)))
    i = tuple(bad[0][:-1])
    return f"{len(bad)} fields differ, first in record {i}: got {got[i]} expected {exp[i]}"
