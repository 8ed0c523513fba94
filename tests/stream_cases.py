"""Shared by the tests of the batch entry points on a STREAMED world (test_stream_cases_on_host.py, test_stream_batch.py): a depth-10 heightfield
scene streamed at radius 22 along a path of four eyes, so that chunks of LOD 5, 4, 3 and 2 are resident, chunks load, unload and change LOD, freed
ranges are reused and the window re-bases twice in x / z and once in y alone.

The ground truth is restated here from the scene's heights and four rules -- the shell of generate_heightfield_chunk (stream.hpp), the residency
rule of ChunkLoader::update and calculate_lod (chunkloader.hpp), and pick_leaf_for_lod (octree.hpp) applied recursively --, and the seeded input
sets (points, regions, rays, entities, views; the boxes of the lists and of the scans) are made per settled state in WORLD coordinates and
shifted by svo_offset, so that they follow the window as it re-bases. What the sets hold is counted from the truth and the oracle alone. Nothing
of the code under test is used. For vx_scan_points, vx_scan_columns and vx_list_region a settled state is handed to scan_cases.py and
list_cases.py as one of their cases (Case), so that their numpy truths and their host harnesses serve here unchanged."""
import functools
import math

import numpy as np

import list_cases as lc
import scan_cases as scn
import trace_cases as tc
from batch_cases import first_difference, oracle_hits, oracle_run, unit  # noqa: F401
from blocks_cases import LOD_ORDER, lod_voxels, pick_octants  # noqa: F401
from helpers import orc, vra  # noqa: F401
from physics_cases import DT, ground_under, oracle_contacts  # noqa: F401
from voxel_rs_amd import hip, host, scenes

SCENE_DEPTH = 10  # 1024^3 domain, 32 chunks per axis
SEED = 0x5EED0001
RADIUS = 22
LAYERS = (0, 8)
PATH = [(8.5, 60.0, 8.5), (100.5, 60.0, 70.5), (100.5, 100.0, 70.5), (8.5, 60.0, 8.5)]
SVO_DEPTH = 11  # what the window of 45 chunks needs
SVO = {"esvo": host.SVO_ESVO, "csvo": host.SVO_CSVO}
LODS = (5, 4, 3, 2)
N = 1 << SCENE_DEPTH
HEIGHT = 32 * LAYERS[1]
OUTSIDE = 0xFFFFFFFF
W, H = 64, 48
STEPS = 8
# the settled states' chunk counts: total and per LOD 5 / 4 / 3 / 2 (the same for both formats)
CHUNKS = {(0, 0): (645, 69, 161, 298, 117), (3, 2): (830, 137, 202, 368, 123)}
MIN_PITCH = 0.05  # the least |d.y| of a ray (build_rays)
SET_SEED = 7100  # + the state's index (anything random for a set added later: a generator of its own, SET_SEED + 100 + the index)
SIZE = 1 << SVO_DEPTH
LIST_BOXES = ("under_eye", "lod5_lod4", "lod4_lod3", "lod2", "rim", "domain_edge")  # the boxes vx_list_region is asked for
SEAM_BOXES = ("lod5_lod4", "lod4_lod3")
SCAN_FOOTPRINTS = LIST_BOXES + ("half_outside",)  # (half_outside holds no block: the domain starts near 600)
EXPOSED_FACES = lc.EXPOSED | lc.FACES
CUT_BOX, CUT = "lod4_lod3", 1000  # the list that a capacity of 1,000 records cuts
REACHES = (1, 7, scn.TO_EDGE)
SETTLED_SCANS = tuple((d, r) for d in scn.DIRECTIONS for r in REACHES)  # (direction, reach) of vx_scan_points at a settled state
MID_SCANS = ((hip.VX_DIR_NEG_Y, scn.TO_EDGE), (hip.VX_DIR_POS_X, scn.TO_EDGE))  # and at a checkpoint in mid-stream


def centre_of(eye):
    return tuple(int(math.floor(v)) >> 5 for v in eye)


# ---- the ground truth ------------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def heights():
    """[x][z] of the whole domain."""
    h = host.scene_heights(SCENE_DEPTH, SEED, 0, 0, N, N).T.astype(np.int64)
    sample = np.random.default_rng(3).integers(0, N, (50, 2))
    assert all(int(h[x, z]) == host.scene_height(SCENE_DEPTH, SEED, int(x), int(z)) for x, z in sample)  # (the per-column call says the same)
    return h


@functools.lru_cache(maxsize=None)
def full_detail():
    """The scene's shell at full detail, [x][y][z] uint8 over the whole domain: per column the voxels from one above the lowest of the four
    neighbour columns (clamped at the domain's edge) up to the column's own height; grass on top, dirt within 3 below it, stone further down."""
    h = heights().astype(np.int16)
    p = np.pad(h, 1, mode="edge")
    m = np.minimum(np.minimum(p[:-2, 1:-1], p[2:, 1:-1]), np.minimum(p[1:-1, :-2], p[1:-1, 2:]))
    lo = np.minimum(h, m + 1)
    y = np.arange(HEIGHT, dtype=np.int16)[None, :, None]
    c = h[:, None, :]
    ids = np.where(y >= c, np.uint8(1), np.where(y + np.int16(3) >= c, np.uint8(2), np.uint8(3)))
    b = np.where((y >= lo[:, None, :]) & (y <= c), ids, np.uint8(0))
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def shown_at(levels):
    """full_detail() as chunks `levels` below full detail show it: one value per aligned cell of side 2^levels (a chunk is 32 blocks, so cells
    never straddle chunks)."""
    return full_detail() if levels == 0 else pick_octants(shown_at(levels - 1))


@functools.lru_cache(maxsize=None)
def truth(centre_chunk):
    """(blocks, lod): what the streamed world shows once settled around the centre chunk (cx, cy, cz), as a dense [x][y][z] uint8 array over the
    domain in WORLD coordinates, and the LOD of each voxel's chunk, 0 = no chunk -- per CHUNK, [cx][cy][cz]: use lod_at for voxels. A chunk is
    resident if it lies in the domain, within dx^2 + dz^2 <= r^2 of the centre, in a layer within reach, and holds a voxel."""
    cx, cy, cz = centre_chunk
    b = full_detail()
    t = np.zeros_like(b)
    n = N // 32
    lod = np.zeros((n, LAYERS[1], n), dtype=np.uint8)
    y_lo, y_hi = max(LAYERS[0], cy - RADIUS), min(LAYERS[1] - 1, cy + RADIUS)
    for x in range(max(0, cx - RADIUS), min(n, cx + RADIUS + 1)):
        for z in range(max(0, cz - RADIUS), min(n, cz + RADIUS + 1)):
            d2 = (x - cx) ** 2 + (z - cz) ** 2
            if d2 > RADIUS * RADIUS:
                continue
            d = int(math.sqrt(d2))
            level = 5 if d <= 6 else 4 if d <= 12 else 3 if d <= 19 else 2
            col = b[32 * x:32 * x + 32, 32 * y_lo:32 * y_hi + 32, 32 * z:32 * z + 32]
            lod[x, y_lo:y_hi + 1, z] = np.where(col.reshape(32, -1, 32, 32).any(axis=(0, 2, 3)), level, 0)
            side = 1 << (5 - level)
            w = 32 // side
            shown = shown_at(5 - level)[w * x:w * x + w, w * y_lo:w * y_hi + w, w * z:w * z + w]
            t[32 * x:32 * x + 32, 32 * y_lo:32 * y_hi + 32, 32 * z:32 * z + 32] = shown.repeat(side, 0).repeat(side, 1).repeat(side, 2) if side > 1 else shown
    t.setflags(write=False)
    lod.setflags(write=False)
    return t, lod


def chunk_counts(lod):
    return (int((lod != 0).sum()),) + tuple(int((lod == k).sum()) for k in LODS)


def svo_offset(s):
    """s.to_svo((0, 0, 0)) as integers: what is added to a world position to have the SVO's."""
    off = np.asarray(s.to_svo((0.0, 0.0, 0.0)), dtype=np.float64)
    assert (off == np.round(off)).all() and (off % 32 == 0).all()
    return off.astype(np.int64)


def offset_of(centre_chunk):
    """The same by the rule of SvoCoordSpace: a chunk lies at radius + (chunk - centre)."""
    return 32 * (RADIUS - np.asarray(centre_chunk, dtype=np.int64))


def classify(t, lod, off, pts):
    """Per float32 SVO position, by the truth alone: the expected value, the LOD of its chunk (0: none), whether it lies outside the octree (a
    component NaN, infinite, below 0 or at or above 2^depth), and whether all its coordinates are integers."""
    p = np.asarray(pts, dtype=np.float32)
    size = np.float32(1 << SVO_DEPTH)
    with np.errstate(invalid="ignore"):
        inside = ((p >= 0) & (p < size)).all(axis=1)
        integral = inside & (p == np.floor(p)).all(axis=1)
    q = np.where(inside[:, None], np.floor(np.where(inside[:, None], p, 0)), 0).astype(np.int64)
    w = q - off
    in_dom = inside & (w >= 0).all(axis=1) & (w < np.asarray(t.shape)).all(axis=1)
    r = np.where(in_dom[:, None], w, 0)
    value = np.where(in_dom, t[r[:, 0], r[:, 1], r[:, 2]], 0).astype(np.uint32)
    level = np.where(in_dom, lod[r[:, 0] >> 5, r[:, 1] >> 5, r[:, 2] >> 5], 0).astype(np.int64)
    return dict(value=value, lod=level, outside=~inside, integral=integral, cell=q)


def lod_at(lod, off, pos):
    """The LOD of the chunk that holds each SVO position (0: none, or outside the domain)."""
    w = np.floor(np.asarray(pos, dtype=np.float64)).astype(np.int64).reshape(-1, 3) - off
    ok = (w >= 0).all(axis=1) & (w < [N, HEIGHT, N]).all(axis=1)
    r = np.where(ok[:, None], w, 0) >> 5
    return np.where(ok, lod[r[:, 0], r[:, 1], r[:, 2]], 0)


def dense_region(t, off, lo, size):
    """What vx_read_region has to give for the box in SVO coordinates: [z][y][x], zeros around the domain."""
    lo, size = np.asarray(lo, dtype=np.int64), np.asarray(size, dtype=np.int64)
    out = np.zeros((size[2], size[1], size[0]), dtype=np.uint32)
    wlo = lo - off
    a, b = np.maximum(wlo, 0), np.minimum(wlo + size, t.shape)
    if (a < b).all():
        out[a[2] - wlo[2]:b[2] - wlo[2], a[1] - wlo[1]:b[1] - wlo[1], a[0] - wlo[0]:b[0] - wlo[0]] = t[a[0]:b[0], a[1]:b[1], a[2]:b[2]].transpose(2, 1, 0)
    return out


def check_cells(t, lod, off, pts, cells, what):
    """vx_block_cell records against the truth: every value; cell_log2 = 5 - lod on blocks, VX_CELL_OUTSIDE outside the octree; for no block,
    the reported cell -- aligned to its size, holding floor(p) -- is all air in the truth."""
    k = classify(t, lod, off, pts)
    value, log2 = cells["value"], cells["cell_log2"]
    bad = np.flatnonzero(value != k["value"])
    assert not len(bad), f"{what}: {len(bad)} values differ, first at {bad[0]}: point {pts[bad[0]]!r} got {value[bad[0]]} expected {k['value'][bad[0]]} (LOD {k['lod'][bad[0]]})"
    assert (log2[k["outside"]] == OUTSIDE).all() and (log2[~k["outside"]] <= SVO_DEPTH).all(), what
    block = value != 0
    assert (log2[block] == 5 - k["lod"][block]).all(), what
    shape = np.asarray(t.shape)
    for i in np.flatnonzero(~k["outside"] & ~block):
        side = 1 << int(log2[i])
        corner = k["cell"][i] // side * side - off
        a, b = np.maximum(corner, 0), np.minimum(corner + side, shape)
        if (a < b).all():
            assert not t[a[0]:b[0], a[1]:b[1], a[2]:b[2]].any(), (what, i, pts[i], int(log2[i]))


# ---- the input sets of one settled state ----------------------------------------------------------------------------------------------------


class Inputs:
    pass


def _ring_columns(lod, centre, level):
    """The (x, z) chunk columns of the ring of one LOD that hold a chunk."""
    cols = np.argwhere((lod == level).any(axis=1))
    assert len(cols)
    return cols


def build_points(t, lod, off, rng):
    """About 1,200 float32 SVO positions, shuffled: per LOD ring 160 in solid voxels (sampled per ring: the LOD-5 ring is a small part of the
    world), 330 in the air of chunks, 110 inside the octree outside every chunk, 44 outside the octree (NaN, +-inf, -1e-30, exactly 2^depth; and
    -0.0f, which is inside), 64 on integer coordinates."""
    size = float(1 << SVO_DEPTH)
    pts = []
    chunks = {k: np.argwhere(lod == k) for k in LODS}

    def solid_in(level):
        c = chunks[level][rng.integers(len(chunks[level]))] * 32
        v = np.argwhere(t[c[0]:c[0] + 32, c[1]:c[1] + 32, c[2]:c[2] + 32] != 0)
        return c + v[rng.integers(len(v))]

    for level in LODS:
        for _ in range(160):
            pts.append(solid_in(level) + off + rng.uniform(0.0, 1.0, 3))
    n_air = 0
    while n_air < 330:  # the air of resident chunks, every ring in turn, near the terrain as often as anywhere
        level = LODS[n_air % 4]
        c = chunks[level][rng.integers(len(chunks[level]))] * 32
        p = c + rng.uniform(0.0, 32.0, 3)
        if n_air % 2:
            p = solid_in(level) + rng.uniform(0.0, 1.0, 3) + [0.0, rng.uniform(1.0, 9.0), 0.0]
        q = np.floor(p).astype(np.int64)
        if (q < 0).any() or (q >= t.shape).any() or t[q[0], q[1], q[2]] != 0 or lod[q[0] >> 5, q[1] >> 5, q[2] >> 5] == 0:
            continue
        pts.append(p + off)
        n_air += 1
    n_space = 0
    while n_space < 110:  # no chunk there: anywhere in the octree, and just above and beside the window's chunks
        if n_space % 2:
            p = rng.uniform(0.0, size, 3)
        else:
            level = LODS[n_space % 4]
            p = chunks[level][rng.integers(len(chunks[level]))] * 32 + rng.uniform(0.0, 32.0, 3) + off + [0.0, 32.0 * rng.integers(1, 4), 0.0]
        if lod_at(lod, off, p)[0] != 0 or (p < 0).any() or (p >= size).any():
            continue
        pts.append(p)
        n_space += 1
    inside_point = lambda: solid_in(LODS[rng.integers(4)]) + off + rng.uniform(0.0, 1.0, 3)  # noqa: E731
    special = [np.nan, np.inf, -np.inf, -1e-30, size, -1.0, -1e-3, size + 0.5, 3.0e38, -3.0e38, float(np.nextafter(np.float32(size), np.float32(np.inf)))]
    for k in range(44):  # outside the octree: one component (then two, then all three) beyond it
        p = inside_point()
        for a in range(1 + k // 15):
            p[(k + a) % 3] = special[(k + 5 * a) % len(special)]
        pts.append(p)
    for k in range(12):  # -0.0f is 0; the largest float below 2^depth is inside
        p = inside_point()
        p[k % 3] = -0.0 if k % 2 else float(np.nextafter(np.float32(size), np.float32(0)))
        pts.append(p)
    for k in range(64):  # integer coordinates: voxels' corners in every ring
        pts.append((solid_in(LODS[k % 4]) + off + rng.integers(-1, 2, 3)).astype(np.float64))
    pts = np.asarray(pts, dtype=np.float32)
    return np.ascontiguousarray(pts[rng.permutation(len(pts))])


def point_counts(t, lod, off, pts):
    k = classify(t, lod, off, pts)
    c = {f"solid{level}": int(((k["lod"] == level) & (k["value"] != 0)).sum()) for level in LODS}
    c.update(air=int(((k["lod"] != 0) & (k["value"] == 0)).sum()), space=int((~k["outside"] & (k["lod"] == 0)).sum()), outside=int(k["outside"].sum()),
             integral=int(k["integral"].sum()))
    return c


def _odd(v):
    return int(v) | 1


def _across(cz, boundary_chunk):
    """A 45 x 40 x 45 box over the boundary at x = 32 * boundary_chunk, in the eye's row of chunks, in WORLD coordinates (its height from the
    boundary's column, clamped into the domain)."""
    h = heights()
    bx, z0 = 32 * boundary_chunk, 32 * cz + 3
    return (_odd(bx - 22), _odd(int(h[min(max(bx, 0), N - 1), z0 + 20]) - 20), _odd(z0)), (45, 40, 45)


def build_regions(t, lod, off, eye, centre):
    """name -> (lo, size) in SVO coordinates."""
    h = heights()
    cx, _, cz = centre
    ex, ez = int(math.floor(eye[0])), int(math.floor(eye[2]))
    odd = _odd

    def across(boundary_chunk):
        return _across(cz, boundary_chunk)

    x2, z2 = 32 * (cx + 20) + 5, 32 * cz + 3
    regions = {
        "under_eye": ((ex // 8 * 8 - 32, int(h[ex, ez]) // 8 * 8 - 32, ez // 8 * 8 - 32), (64, 64, 64)),
        "lod5_lod4": across(cx + 7),
        "lod4_lod3": across(cx + 13),
        "lod2": ((odd(x2), odd(int(h[x2 + 24, z2 + 24]) - 16), odd(z2)), (48, 32, 48)),
    }
    out = {name: (tuple(int(v) for v in np.asarray(lo) + off), size) for name, (lo, size) in regions.items()}
    out["half_outside"] = ((-20, int(h[ex, ez]) + int(off[1]) - 12, ez + int(off[2]) - 20), (40, 24, 40))
    out["empty_size"] = (out["under_eye"][0], (5, 0, 5))
    return out


def region_counts(t, lod, off, regions):
    """Per region: how many voxels of each LOD it holds, how many are non-empty, and -- for the LOD-2 box -- how many distinct LOD-2 voxels
    (8 x 8 x 8 cells) in it are non-empty."""
    c = {}
    for name, (lo, size) in regions.items():
        if 0 in size:
            c[name] = dict(voxels=0)
            continue
        z, y, x = np.meshgrid(*(np.arange(size[a]) + lo[a] for a in (2, 1, 0)), indexing="ij")
        p = np.stack([x, y, z], axis=-1).reshape(-1, 3)
        level = lod_at(lod, off, p)
        dense = dense_region(t, off, lo, size).reshape(-1)
        c[name] = dict(voxels=len(p), nonzero=int((dense != 0).sum()), in_octree=int(((p >= 0) & (p < 1 << SVO_DEPTH)).all(axis=1).sum()),
                       **{f"lod{k}": int((level == k).sum()) for k in LODS}, **{f"nonzero_lod{k}": int(((level == k) & (dense != 0)).sum()) for k in LODS})
        full = (level == 2) & (dense != 0)
        c[name]["lod2_voxels"] = len(np.unique(p[full] // 8, axis=0)) if full.any() else 0
    return c


def build_rays(t, lod, off, eye, centre, scene, rng):
    """(origins, dirs, max_dst, kinds) of about 800 rays in SVO coordinates: per LOD ring 60 from above and 40 oblique onto its terrain and 32
    origins inside its solid voxels; 80 skimming rays from the eye's chunk outwards across the rings; 40 from outside the octree aimed in and 20
    aimed away; 50 ended by max_dst before their hit; 50 to the sky. No direction has x = z = 0 (the sky term of trace_rays), and none is
    closer to level than |d.y| = 0.05: the shader's sky term takes acos of the cosine of the ray's elevation a in fp32, whose error of about
    1e-7 becomes 1e-7 / sin(a) in the angle and 0.63 times that in the colour (d grad / da = 1.91 at the horizon, horizon - sky <= 0.33) --
    2e-5 at a = 0.003, beyond the 5e-6 that the float64 restatement trace_cases.sky_color is held to, and 1.3e-6 at a = 0.05."""
    h = heights()
    size = float(1 << SVO_DEPTH)
    o, d, m, kinds = [], [], [], []

    def add(kind, p, v, md=-1.0):
        v = np.asarray(v, dtype=np.float32)
        if abs(v[1]) < MIN_PITCH:  # (see above)
            v = unit([v[0], -MIN_PITCH if np.signbit(v[1]) else MIN_PITCH, v[2]])
        assert np.isfinite(v).all() and (v[0] != 0 or v[2] != 0) and abs(v[1]) >= 0.99 * MIN_PITCH
        o.append(np.asarray(p, dtype=np.float64) + off)
        d.append(v)
        m.append(np.float32(md))
        kinds.append(kind)

    def column_in(level):
        cols = _ring_columns(lod, centre, level)
        c = cols[rng.integers(len(cols))]
        x, z = 32 * c[0] + rng.uniform(0.0, 32.0), 32 * c[1] + rng.uniform(0.0, 32.0)
        return x, float(h[int(x), int(z)]), z

    chunks = {k: np.argwhere(lod == k) for k in LODS}
    for level in LODS:
        for k in range(100):
            x, y, z = column_in(level)
            if k < 60:
                v = unit([rng.uniform(-0.15, 0.15), -1.0, rng.uniform(-0.15, 0.15)])
            else:
                v = unit([rng.uniform(-1, 1), rng.uniform(-0.7, -0.25), rng.uniform(-1, 1)])
            target = np.float64([x, y + 0.5, z])
            add(f"onto{level}", target - v.astype(np.float64) * rng.uniform(12.0, 40.0), v)
        for _ in range(32):
            c = chunks[level][rng.integers(len(chunks[level]))] * 32
            vox = np.argwhere(t[c[0]:c[0] + 32, c[1]:c[1] + 32, c[2]:c[2] + 32] != 0)
            add(f"inside{level}", c + vox[rng.integers(len(vox))] + rng.uniform(0.05, 0.95, 3), unit(rng.normal(size=3)))
    ex, ez = eye[0], eye[2]
    mid = np.float64([32 * centre[0] + 16, 32 * centre[2] + 16])
    for k in range(80):  # skimming: nearly level, from just inside a ring boundary outwards over it (the domain lies towards +x, +z)
        a = rng.uniform(0.08, 0.5 * math.pi - 0.08)
        out = np.float64([math.cos(a), math.sin(a)])
        x, z = mid + out * (32.0 * (7, 13, 20)[k % 3] - 16.0 - rng.uniform(2.0, 14.0))
        add("skim", (x, float(h[int(x), int(z)]) + rng.uniform(1.5, 8.0), z), unit([out[0], rng.uniform(-0.12, -MIN_PITCH), out[1]]))
    for k in range(60):  # outside the octree, up to 8 blocks out, aimed at the terrain of some ring / aimed away
        axis, far = k % 3, (k // 3) % 2
        x, y, z = column_in(LODS[k % 4])
        target = np.float64([x, y, z]) + off
        p = target + rng.uniform(-300.0, 300.0, 3)
        p[axis] = size + rng.uniform(0.01, 8.0) if far else -rng.uniform(0.01, 8.0)
        if k < 40:
            add("outside_in", p - off, unit(target - p))
        else:
            v = unit(rng.normal(size=3))
            v[axis] = abs(v[axis]) + np.float32(0.05) if far else -abs(v[axis]) - np.float32(0.05)
            add("outside_away", p - off, unit(v))
    n_cut = 0
    while n_cut < 50:  # ended by max_dst before the hit
        x, y, z = column_in(LODS[n_cut % 4])
        p = np.float64([x, y + rng.uniform(8.0, 30.0), z])
        v = unit([rng.uniform(-0.5, 0.5), -1.0, rng.uniform(-0.5, 0.5)])
        r, _, _ = scene.intersect(np.float32(p + off), v, -1.0, False)
        if r.t > 1.0:
            add("cut", p, v, r.t * rng.uniform(0.2, 0.9))
            n_cut += 1
    for k in range(50):  # to the sky
        x, y, z = column_in(LODS[k % 4])
        add("sky", (x, y + rng.uniform(3.0, 20.0), z), unit([rng.uniform(-1, 1), rng.uniform(0.3, 1.5), rng.uniform(-1, 1)]), -1.0 if k % 2 else 64.0)
    order = rng.permutation(len(o))
    o, d, m = (np.ascontiguousarray(np.asarray(a, dtype=np.float32)[order]) for a in (o, d, m))
    return o, d, m, np.asarray(kinds)[order]


def ray_counts(t, lod, off, o, d, m, kinds, hits, scene):
    """From the oracle's opaque hits and the truth: per ring the `onto` rays that hit terrain of that ring, per ring the origins that lie in
    a solid voxel of it, the skimming rays that hit in another ring than they start over, outside origins that hit / miss, rays that
    max_dst cut before their hit, and misses."""
    hit = hits["dst"] > 0
    hit_lod = lod_at(lod, off, hits["pos"] - 0.01 * hip.FACE_NORMALS[np.clip(hits["face_id"], 0, 5)])
    start = classify(t, lod, off, o)
    c = {}
    for level in LODS:
        c[f"onto{level}"] = int(((kinds == f"onto{level}") & hit & (hit_lod == level)).sum())
        c[f"inside{level}"] = int(((kinds == f"inside{level}") & (start["lod"] == level) & (start["value"] != 0)).sum())
    skim = (kinds == "skim") & hit
    c["skim_crossing"] = int((skim & (hit_lod != lod_at(lod, off, o))).sum())
    c["skim_rings"] = sorted(int(v) for v in np.unique(hit_lod[skim]))
    c["outside_in_hits"] = int(((kinds == "outside_in") & hit).sum())
    c["outside_away_misses"] = int(((kinds == "outside_away") & ~hit).sum())
    c["outside_origins"] = int(start["outside"].sum())
    cut = 0
    for i in np.flatnonzero((kinds == "cut") & ~hit):
        r, _, _ = scene.intersect(o[i], d[i], -1.0, False)
        cut += bool(r.t > m[i])
    c["cut"] = cut
    c["sky_misses"] = int(((kinds == "sky") & ~hit).sum())
    c["rays"] = len(o)
    return c


def build_entities(t, lod, off, eye, centre, scene, rng):
    """(rows of host.make_entities in SVO coordinates, roles: name -> row indices): 15 boxes in the LOD-5 area -- standing on the ground, just
    above it, moving, sunk into it, flying --, 4 standing on LOD-4 terrain, 4 on LOD-3 terrain, one wide box straddling the LOD 5 / LOD 4 boundary."""
    cx, _, cz = centre
    rows, roles = [], {}
    top = float(HEIGHT + off[1])

    def add(role, pos, vel=(0.0, 0.0, 0.0), extents=(0.8, 1.8, 0.8), wall_clip=False, flying=False):
        r = host.make_entities([pos], extents=extents, offset=(-extents[0] / 2, 0.0, -extents[2] / 2))
        r[0, 3:6] = vel
        r[0, 12], r[0, 13] = float(wall_clip), float(flying)
        roles.setdefault(role, []).append(len(rows))
        rows.append(r[0])

    def ground(x, z, extents=(0.8, 1.8, 0.8)):
        return ground_under(scene, x, z, top, (-extents[0] / 2, 0.0, -extents[2] / 2), extents)

    def near_eye():
        return eye[0] + off[0] + rng.uniform(2.0, 90.0), eye[2] + off[2] + rng.uniform(2.0, 90.0)

    def in_ring(level):
        cols = _ring_columns(lod, centre, level)
        c = cols[rng.integers(len(cols))]
        return 32 * c[0] + off[0] + rng.uniform(6.0, 26.0), 32 * c[1] + off[2] + rng.uniform(6.0, 26.0)

    for k in range(4):  # standing: on the ground and a hair above it
        x, z = near_eye()
        add("standing", (x, ground(x, z) + [0.0, 0.0005, 0.01, 0.016][k], z))
    for k in range(6):
        x, z = near_eye()
        add("moving", (x, ground(x, z) + rng.uniform(0.3, 2.5), z), (rng.uniform(-6, 6), 0.0, rng.uniform(-6, 6)), wall_clip=k == 1)
    for depth in (0.3, 0.5, 0.7):
        x, z = near_eye()
        add("sunk", (x, ground(x, z) - depth, z), (rng.uniform(-3, 3), 0.0, rng.uniform(-3, 3)))
    for k in range(2):
        x, z = near_eye()
        add("flying", (x, ground(x, z) + rng.uniform(1.0, 4.0), z), (rng.uniform(-6, 6), rng.uniform(-2, 2), rng.uniform(-6, 6)), flying=True)
    for level in (4, 3):  # standing on the large voxels of a LOD ring (0.016 above: see batch_cases.build_entities_for)
        for _ in range(4):
            x, z = in_ring(level)
            add(f"on_lod{level}", (x, ground(x, z) + 0.016, z))
    ext = (2.6, 1.8, 2.6)
    x, z = float(32 * (cx + 7) + off[0]), 32 * cz + off[2] + 14.3
    add("straddle", (x, ground(x, z, ext) + 0.2, z), (-2.0, 0.0, 1.0), extents=ext)
    return np.ascontiguousarray(np.stack(rows)).astype(np.float32), roles


def entity_counts(t, lod, off, rows, roles, run):
    """From the oracle-backed run and the truth: per LOD the boxes that stand (a contact below of less than 0.05 at the start) over terrain of
    that LOD, boxes that moved, contacts of each kind, and the LODs under the straddling box's footprint."""
    start = run[0][1]
    under = lod_at(lod, off, rows[:, 0:3] - [0.0, 0.5, 0.0])
    standing = (start[:, 1] >= 0) & (start[:, 1] < 0.05)
    c = {f"standing_on_lod{k}": int((standing & (under == k)).sum()) for k in (5, 4, 3)}
    c["moved"] = int((run[-1][0][:, 0:3] != rows[:, 0:3]).any(axis=1).sum())
    c["flying"], c["sunk"] = len(roles["flying"]), len(roles["sunk"])
    c["sunk_inside"] = int(sum(classify(t, lod, off, rows[i:i + 1, 0:3] + [0.0, 0.05, 0.0])["value"][0] != 0 for i in roles["sunk"]))
    i = roles["straddle"][0]
    corners = rows[i, 0:3] + rows[i, 6:9] + [[0.0, -0.5, 0.0], [rows[i, 9], -0.5, rows[i, 11]]]
    c["straddle_lods"] = sorted(int(v) for v in lod_at(lod, off, corners))
    c["boxes"] = len(rows)
    return c


def build_views(t, lod, off, eye, centre):
    """Two 64 x 48 views, shadows on: from above the eye towards the horizon over the domain's diagonal, so that every ring is on screen; and from
    high above the LOD 5 / LOD 4 boundary looking down."""
    h = heights()
    cx, _, cz = centre
    light = scenes._normalize((-1.0, -1.0, -1.0))
    ex, ez = int(eye[0]), int(eye[2])
    eye1 = np.float64([eye[0], float(h[ex, ez]) + 70.0, eye[2]]) + off
    bx, bz = 32 * (cx + 7), 32 * cz + 16
    eye2 = np.float64([bx + 0.5, float(h[bx, bz]) + 90.0, bz + 0.5]) + off
    out = []
    for e, fwd in ((eye1, (0.72, -0.2, 0.66)), (eye2, (0.25, -1.0, 0.15))):
        view = scenes.view_matrix(e, fwd, (0.0, 1.0, 0.0))
        out.append(hip.make_uniforms(view, np.radians(72.0), W / H, 0.3, light, e, True, 300.0))
    return out


def view_counts(lod, off, hits):
    """Per view, from the oracle's records: sky, lit and shadowed pixels and the pixels that show terrain of each LOD."""
    out = []
    for rec in hits:
        f = rec["flags"].ravel()
        level = lod_at(lod, off, rec["pos"].reshape(-1, 3) - 0.01 * hip.FACE_NORMALS[np.clip(rec["face_id"].ravel(), 0, 5)])
        c = dict(sky=int(((f & 1) == 0).sum()), lit=int((((f & 2) != 0) & ((f & 4) == 0)).sum()), shadow=int(((f & 4) != 0).sum()))
        c.update({f"lod{k}": int((((f & 1) != 0) & (level == k)).sum()) for k in LODS})
        out.append(c)
    return out


# ---- the boxes of the lists and the scans, and a state as a case of scan_cases.py / list_cases.py ------------------------------------------------


def build_list_boxes(regions, off, centre):
    """name -> (lo, size) in SVO coordinates: the four regions that hold blocks; `rim`, the box over the boundary at chunk cx + 23, where the
    resident chunks end (LOD-2 voxels face no chunk); `domain_edge`, the box over x = 0 of the scene (inside the octree: the scene's own edge)."""
    cx, _, cz = centre
    boxes = {name: regions[name] for name in LIST_BOXES[:4]}
    for name, chunk in (("rim", cx + 23), ("domain_edge", 0)):
        lo, size = _across(cz, chunk)
        boxes[name] = (tuple(int(v) for v in np.asarray(lo) + off), size)
    return boxes


def build_scan_boxes(list_boxes, regions):
    """(name, direction) -> (lo, size): the footprint of every list box and of `half_outside`, stretched along the direction's axis over the
    whole octree and 5 voxels beyond it on either side."""
    out = {}
    for name in SCAN_FOOTPRINTS:
        lo, size = list_boxes[name] if name in list_boxes else regions[name]
        for d in scn.DIRECTIONS:
            blo, bsize = list(lo), list(size)
            blo[d >> 1], bsize[d >> 1] = -5, SIZE + 10
            out[name, d] = (tuple(blo), tuple(bsize))
    return out


@functools.lru_cache(maxsize=None)
def cells(centre_chunk):
    """Per voxel of truth(centre_chunk): log2 of the side of the cells its chunk shows, 5 - lod; 0 where there is no chunk."""
    _, lod = truth(centre_chunk)
    k = np.where(lod != 0, 5 - lod.astype(np.int16), 0).astype(np.uint8)
    c = k.repeat(32, 0).repeat(32, 1).repeat(32, 2)
    c.setflags(write=False)
    return c


class Case:
    """What scan_cases.py and list_cases.py want of a case, for one frame of the streamed world; the truth only at a settled state."""

    def __init__(self, scene, centre=None, off=None):
        self.fmt, self.svo_type, self.frame, self.size = scene.fmt, scene.svo_type, scene.frame, SIZE
        if centre is not None:
            self.truth, self.cell = truth(centre)[0], cells(centre)
            lo = np.asarray(off, dtype=np.int64)
            self.info = dict(lo=lo, hi=lo + np.asarray(self.truth.shape), size=float(SIZE))


class BlockTruth:
    """By the dense truth alone: points[direction, reach] and columns[name, direction] (SCAN_HIT_DTYPE), lists[name, flags] (BLOCK_AT_DTYPE)."""


_block_truths = {}


def block_truth(case, inp):
    """The numpy truths of scan_cases.py and list_cases.py for a settled state's sets; once per state (the formats share the truth)."""
    key = (inp.index, inp.pts.tobytes())
    if key not in _block_truths:
        b = BlockTruth()
        b.points = {(d, r): scn.points_truth(case, inp.pts, d, r) for d, r in SETTLED_SCANS}
        b.columns = {(name, d): scn.columns_truth(case, lo, size, d) for (name, d), (lo, size) in inp.scan_boxes.items()}
        b.lists = {(name, flags): lc.expected_list(case, lo, size, flags) for name, (lo, size) in inp.list_boxes.items() for flags in lc.FLAG_SETS}
        for a in list(b.points.values()) + list(b.columns.values()) + list(b.lists.values()):
            a.setflags(write=False)
        _block_truths[key] = b
    return _block_truths[key]


def list_counts(case, lod, off, boxes):
    """Per list box, from the truth: its records, how many of them have an open face, how many have none (the inner voxels of LOD cells and
    of the ground), how many show their -x / +x face, and the LODs of the chunks that hold them."""
    c = {}
    for name, (lo, size) in boxes.items():
        x, y, z, _, faces, _ = lc.expected_parts(case, lo, size, lc.FACES)
        exposed = int((faces != 0).sum())
        c[name] = dict(records=len(faces), exposed=exposed, hidden=len(faces) - exposed, open_neg_x=int((faces & 1 != 0).sum()),
                       open_pos_x=int((faces & 2 != 0).sum()), lods=sorted(int(v) for v in np.unique(lod_at(lod, off, np.stack([x, y, z], axis=1)))))
    return c


def scan_counts(columns):
    """From the truth's columns: the cell sizes (log2) that answer the top-down heightmap of each seam box, and under_eye over all six
    directions together and in the direction that sees most; the directions in which half_outside has a column that hits, and none."""
    def sizes(keys):
        return sorted({int(v) for k in keys for v in np.unique(columns[k]["cell_log2"][columns[k]["coord"] != scn.NONE])})

    c = {f"{name}_down": sizes([(name, hip.VX_DIR_NEG_Y)]) for name in SEAM_BOXES}
    c["under_eye"] = sizes([("under_eye", d) for d in scn.DIRECTIONS])
    c["under_eye_most_in_one"] = max(len(sizes([("under_eye", d)])) for d in scn.DIRECTIONS)
    hit = [d for d in scn.DIRECTIONS if (columns["half_outside", d]["coord"] != scn.NONE).any()]
    c["half_outside_hit"], c["half_outside_none"] = hit, [d for d in scn.DIRECTIONS if d not in hit]
    return c


# ---- what the oracle says of a set on one frame ------------------------------------------------------------------------------------------------


class _Frame:
    def __init__(self, words):
        self.words = words

    def frame(self, pad_words=0):  # (trace_cases.scene_arguments asks c.world.frame(pad_words=0))
        return self.words


class Scene:
    """What the on-host harnesses and trace_cases.scene_arguments want of a case: the frame as a context holds it, materials, textures."""

    def __init__(self, fmt, frame_words):
        self.fmt, self.svo_type = fmt, SVO[fmt]
        self.tex, self.mats = scenes.synthetic_textures(), scenes.synthetic_materials()
        self.words = np.ascontiguousarray(frame_words)
        self.oracle = orc.OracleScene(self.svo_type, self.words, self.mats.view(orc.MATERIAL_DTYPE), self.tex, 6)
        self.frame = np.concatenate([self.words, np.zeros(4, dtype=np.uint32)])  # (with the 16 zero bytes a context keeps behind the world)
        self.world = _Frame(self.words)


class Expected:
    pass


def expected(scene, inp, blocks_too=False):
    """The oracle's answers for one input set on one frame: vx_ray_hit records of the opaque cast; vx_hit records and colours of trace_rays under
    trace_cases.free_uniforms; images and records of the views; the entities after 8 steps and the contacts of the last."""
    e = Expected()
    e.hits = oracle_hits(scene.oracle, inp.o, inp.d, inp.m, False)
    n = len(inp.o)
    e.trace = np.zeros(n, dtype=hip.HIT_DTYPE)
    e.color = np.zeros((n, 4), dtype=np.float64)
    sky = tc.sky_color(inp.d)
    for i in range(n):
        ctr = orc.Counters()
        r, _, _ = scene.oracle.intersect(inp.o[i], inp.d[i], float(inp.m[i]), True, counters=ctr)
        x = e.trace[i]
        x["t"], x["value"], x["face_id"], x["pos"], x["lod"], x["uv"] = r.t, r.value, r.face_id, list(r.pos), r.lod, list(r.uv)
        x["flags"], x["shadow_t"], x["steps"] = int(r.t != -1.0), -1.0, ctr.iterations
        e.color[i] = list(r.color) if r.t != -1.0 else sky[i]
    rendered = [scene.oracle.render(tc.as_oracle(u), W, H) for u in inp.views]
    e.imgs, e.view_hits = np.stack([r[0] for r in rendered]), np.stack([r[1] for r in rendered])
    e.run = oracle_run(scene.oracle, inp.rows, STEPS)
    return e


def make_inputs(fmt, index, eye, centre, off, scene):
    t, lod = truth(centre)
    rng = np.random.default_rng(SET_SEED + index)
    inp = Inputs()
    inp.index, inp.eye, inp.centre, inp.off = index, eye, centre, off
    inp.pts = build_points(t, lod, off, rng)
    inp.regions = build_regions(t, lod, off, eye, centre)
    inp.o, inp.d, inp.m, inp.kinds = build_rays(t, lod, off, eye, centre, scene.oracle, rng)
    inp.rows, inp.roles = build_entities(t, lod, off, eye, centre, scene.oracle, rng)
    inp.views = build_views(t, lod, off, eye, centre)
    inp.free_u = tc.free_uniforms()
    inp.list_boxes = build_list_boxes(inp.regions, off, centre)
    inp.scan_boxes = build_scan_boxes(inp.list_boxes, inp.regions)
    for a in (inp.pts, inp.o, inp.d, inp.m, inp.rows):
        a.setflags(write=False)
    return inp


def kind_counts(inp, exp):
    t, lod = truth(inp.centre)
    return dict(points=point_counts(t, lod, inp.off, inp.pts), regions=region_counts(t, lod, inp.off, inp.regions),
                rays=ray_counts(t, lod, inp.off, inp.o, inp.d, inp.m, inp.kinds, exp.hits, exp.scene.oracle),
                entities=entity_counts(t, lod, inp.off, inp.rows, inp.roles, exp.run), views=view_counts(lod, inp.off, exp.view_hits),
                lists=list_counts(exp.case, lod, inp.off, inp.list_boxes), scans=scan_counts(exp.blocks.columns))


def assert_kinds(k):
    """The thresholds the sets were specified with; a seed that misses one is changed, never the threshold."""
    p = k["points"]
    assert all(p[f"solid{level}"] >= 150 for level in LODS) and p["air"] >= 300 and p["space"] >= 100 and p["outside"] >= 40 and p["integral"] >= 60, p
    r = k["regions"]
    assert r["under_eye"]["lod4"] == r["under_eye"]["lod3"] == r["under_eye"]["lod2"] == 0 and r["under_eye"]["nonzero_lod5"] >= 1000, r["under_eye"]
    assert min(r["lod5_lod4"]["nonzero_lod5"], r["lod5_lod4"]["nonzero_lod4"]) >= 500, r["lod5_lod4"]
    assert min(r["lod4_lod3"]["nonzero_lod4"], r["lod4_lod3"]["nonzero_lod3"]) >= 500, r["lod4_lod3"]
    assert r["lod2"]["lod5"] == r["lod2"]["lod4"] == r["lod2"]["lod3"] == 0 and r["lod2"]["lod2_voxels"] >= 20, r["lod2"]
    assert 0 < r["half_outside"]["in_octree"] < r["half_outside"]["voxels"] and r["empty_size"]["voxels"] == 0
    y = k["rays"]
    assert 700 <= y["rays"] <= 900, y
    assert all(y[f"onto{level}"] >= 80 and y[f"inside{level}"] >= 30 for level in LODS), y
    assert y["skim_crossing"] >= 20 and len(y["skim_rings"]) >= 2, y
    assert y["outside_in_hits"] >= 10 and y["outside_away_misses"] == 20 and y["outside_origins"] >= 60 and y["cut"] >= 40 and y["sky_misses"] >= 40, y
    e = k["entities"]
    assert e["boxes"] == 24 and e["standing_on_lod5"] >= 3 and e["standing_on_lod4"] >= 4 and e["standing_on_lod3"] >= 4, e
    assert e["moved"] >= 8 and e["flying"] >= 2 and e["sunk_inside"] >= 2 and e["straddle_lods"] == [4, 5], e
    v = k["views"]
    assert all(v[0][f"lod{level}"] >= 20 for level in LODS) and v[0]["sky"] >= 100 and v[0]["shadow"] >= 20 and v[0]["lit"] >= 100, v[0]
    assert v[1]["lod5"] >= 300 and v[1]["lod4"] >= 300 and v[1]["shadow"] >= 20, v[1]
    b = k["lists"]
    assert b["under_eye"]["records"] >= 1500, b["under_eye"]
    assert b["lod5_lod4"]["records"] >= 3000 and b["lod5_lod4"]["hidden"] >= 300, b["lod5_lod4"]
    assert b["lod4_lod3"]["records"] >= 8000 and b["lod4_lod3"]["hidden"] >= 3000, b["lod4_lod3"]
    assert b["lod2"]["records"] >= 20000 and b["lod2"]["hidden"] >= 15000, b["lod2"]
    assert b["rim"]["lods"] == [2] and b["rim"]["exposed"] >= 1500 and b["rim"]["open_pos_x"] >= 400, b["rim"]
    assert b["domain_edge"]["records"] >= 1000 and b["domain_edge"]["open_neg_x"] >= 300, b["domain_edge"]
    s = k["scans"]
    assert len(s["lod5_lod4_down"]) == 2 and len(s["lod4_lod3_down"]) == 2, s  # the heightmaps over the seams answer with two cell sizes each
    assert s["under_eye"] == [0, 1, 2, 3], s  # side elevations from under the eye cross every ring
    assert s["half_outside_hit"] and s["half_outside_none"], s


# ---- the stream ---------------------------------------------------------------------------------------------------------------------


def new_streamer(fmt):
    return host.WorldStreamer(SVO[fmt], SCENE_DEPTH, RADIUS, LAYERS[0], LAYERS[1], SEED)


class State:
    pass


@functools.lru_cache(maxsize=None)
def dry_run(fmt):
    """The path streamed without a device, pump(None, 400): per settled state its frame, offset, resident chunks, the pump totals so far, the
    input sets and what the oracle says of them. Computed once per format and left unchanged."""
    s = new_streamer(fmt)
    states = []
    totals = dict(loads=0, unloads=0, lod_changes=0, ranges=0, commits=0)
    for index, eye in enumerate(PATH):
        s.move_to(*eye)
        while True:
            st = s.pump(None, 400)
            for k in ("loads", "unloads", "lod_changes", "ranges"):
                totals[k] += st[k]
            totals["commits"] += 1
            if st["pending"] == 0:
                break
        x = State()
        x.index, x.eye, x.centre = index, eye, centre_of(eye)
        x.off = svo_offset(s)
        x.resident, x.arena_bytes, x.totals = s.resident_chunks, st["arena_bytes"], dict(totals)
        x.scene = Scene(fmt, s.frame(pad_words=0))
        x.inputs = make_inputs(fmt, index, eye, x.centre, x.off, x.scene)
        x.expected = expected(x.scene, x.inputs)
        x.expected.scene = x.scene
        x.case = x.expected.case = Case(x.scene, x.centre, x.off)
        x.blocks = x.expected.blocks = block_truth(x.case, x.inputs)
        x.counts = kind_counts(x.inputs, x.expected)
        states.append(x)
    return states
