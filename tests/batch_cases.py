"""Shared by the tests of vx_raycast_batch and vx_physics_step beyond the heightfield (test_batch_cases_on_host.py,
test_batch_physics_worlds.py): two small worlds with translucent blocks -- `glasshouse`, one chunk at the origin, and `far_chunks`,
2 x 2 chunks far from the origin of a depth-14 world, one of them at a lower LOD --, a seeded ray set and an entity set for each, and
what the oracle says of them. Everything is seeded; the builders use the oracle (ground_under, the distance between a pane and what
lies behind it) and nothing of the code under test."""
import numpy as np

from helpers import orc, vra  # noqa: F401
from physics_cases import DT, ground_under, oracle_contacts, oracle_step  # noqa: F401
from voxel_rs_amd import hip, host

AIR, GRASS, DIRT, STONE, BRICKS, GLASS, SAND, LOG, LEAVES, COBBLE = 0, 1, 2, 3, 4, 5, 7, 9, 10, 12
TRANSLUCENT_IDS = (GLASS, LEAVES)
FAR_BASE = (400, 3, 401)  # tests/test_hip_parity.py::test_rays_from_inside_voxels_in_a_deep_world, depth 14
LOD_CHUNK = (1, 1)        # (dx, dz) of the far chunk built at LOD 3: voxels of 4 x 4 x 4 blocks
RAY_SEED = {"glasshouse": 21, "far_chunks": 22}
ENTITY_SEED = {"glasshouse": 31, "far_chunks": 32}
STEPS = 12
SPECIAL_EXTENTS = [(8.0, 8.0, 8.0), (4.2, 1.0, 7.9), (1.0, 2.0, 1.0), (0.05, 0.05, 0.05), (1e-30, 1.0, 1.0)]


def _finish(name, svo_type, world, blocks, lo, lod_box):
    from voxel_rs_amd import scenes

    tex, mats = scenes.synthetic_textures(), scenes.synthetic_materials()
    scene = orc.OracleScene(svo_type, world.frame(), mats.view(orc.MATERIAL_DTYPE), tex, 6)
    lo = np.asarray(lo, dtype=np.int64)
    detail = np.ones(blocks.shape, dtype=bool)  # where `blocks` is what the world holds (not inside the LOD chunk)
    if lod_box is not None:
        a, b = lod_box[0] - lo, lod_box[1] - lo
        detail[a[0]:b[0], a[1]:b[1], a[2]:b[2]] = False
    info = dict(name=name, svo_type=svo_type, depth=world.depth, size=float(1 << world.depth), lo=lo, hi=lo + np.asarray(blocks.shape), blocks=blocks,
                detail=detail, lod_box=lod_box, scene=scene)
    return world, scene, tex, mats, info


def _chunk_of(pos, lod, blocks):
    chunk = vra.Chunk(pos[0], pos[1], pos[2], lod)
    for x, y, z in np.argwhere(blocks != 0):
        chunk.set_block(int(x), int(y), int(z), int(blocks[x, y, z]))
    chunk.compact()
    return chunk


def glasshouse(svo_type):
    """One chunk at (0, 0, 0), in the style of test_hip_parity.py::test_translucent_blocks_frame: a floor of two opaque ids, a glass wall of
    two layers (z = 10, 11), a wall of leaves (z = 14), an opaque pillar behind them, a glass ceiling one block thick over part of the floor
    (y = 12), and single blocks with air on all six sides."""
    b = np.zeros((32, 32, 32), dtype=np.uint32)  # [x][y][z]
    for x in range(32):
        for z in range(32):
            b[x, 0, z] = STONE if (x + z) % 3 else SAND
    b[4:28, 1:9, 10] = GLASS
    b[4:28, 1:9, 11] = GLASS  # second identical layer: skipped as "not first of its kind"
    b[4:28, 1:9, 14] = LEAVES
    b[16, 1:12, 20] = LOG
    b[4:16, 12, 18:30] = GLASS  # the ceiling
    for (x, y, z), v in (((6, 5, 24), BRICKS), ((24, 6, 4), LOG), ((28, 15, 28), GRASS), ((2, 20, 2), COBBLE), ((20, 3, 26), LEAVES), ((10, 4, 5), GLASS),
                         ((22, 20, 16), DIRT)):
        b[x, y, z] = v
    world = vra.World(svo_type)
    world.set_chunk((0, 0, 0), _chunk_of((0, 0, 0), 5, b))
    world.serialize()
    assert world.depth == 6  # (the octree spans [0, 64): the chunk is its lowest octant)
    return _finish("glasshouse", svo_type, world, b, (0, 0, 0), None)


def far_chunks(svo_type):
    """The world of test_hip_parity.py::test_rays_from_inside_voxels_in_a_deep_world at base (400, 3, 401), depth 14: 2 x 2 chunks of random
    columns with scattered glass, leaves and stone bricks; the chunk at LOD_CHUNK is built at LOD 3."""
    rng = np.random.default_rng(11)
    base = FAR_BASE
    b = np.zeros((64, 32, 64), dtype=np.uint32)
    world = vra.World(svo_type)
    for dx in range(2):
        for dz in range(2):
            c = b[32 * dx:32 * dx + 32, :, 32 * dz:32 * dz + 32]
            for x in range(32):
                for z in range(32):
                    top = 6 + int(rng.integers(0, 6))
                    for y in range(top):
                        c[x, y, z] = int(rng.choice([GRASS, DIRT, STONE, SAND, LOG]))
            for _ in range(200):
                x, y, z = (int(v) for v in rng.integers(0, 32, size=3))
                c[x, y, z] = int(rng.choice([GLASS, LEAVES, BRICKS]))
            pos = (base[0] + dx, base[1], base[2] + dz)
            world.set_chunk(pos, _chunk_of(pos, 3 if (dx, dz) == LOD_CHUNK else 5, c))
    world.serialize()
    assert world.depth == 14
    lo = np.array([32 * v for v in base], dtype=np.int64)
    lod_lo = lo + np.array([32 * LOD_CHUNK[0], 0, 32 * LOD_CHUNK[1]])
    return _finish("far_chunks", svo_type, world, b, lo, (lod_lo, lod_lo + 32))


BUILDERS = {"glasshouse": glasshouse, "far_chunks": far_chunks}


# ---- rays -------------------------------------------------------------------------------------------------------------------------


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return (v / np.linalg.norm(v)).astype(np.float32)


def block_at(info, p):
    """The block id the dense copy holds at world position p (air outside it)."""
    q = np.floor(np.asarray(p, dtype=np.float64)).astype(np.int64) - info["lo"]
    if (q < 0).any() or (q >= info["blocks"].shape).any():
        return AIR
    return int(info["blocks"][q[0], q[1], q[2]])


def blocks_of(info, ids):
    """World coordinates of the full-detail blocks whose id is in `ids`."""
    return np.argwhere(np.isin(info["blocks"], ids) & info["detail"]) + info["lo"]


def exposed(info, blocks):
    """Those of `blocks` that have air above them or on two opposite sides: a ray from the air can reach them."""
    def free(b):
        air = [block_at(info, b + np.array(n)) == AIR for n in ((0, 1, 0), (-1, 0, 0), (1, 0, 0), (0, 0, -1), (0, 0, 1))]
        return air[0] or (air[1] and air[2]) or (air[3] and air[4])
    return np.array([b for b in blocks if free(b)])


def random_unit(rng):
    return unit(rng.normal(size=3))


def oracle_hits(scene, o, d, m, translucent=False, steps=None):
    """vx_ray_hit records by the oracle alone (`steps`, if given, receives its iteration counts)."""
    out = np.zeros(len(o), dtype=hip.RAY_HIT_DTYPE)
    for i in range(len(o)):
        ctr = orc.Counters() if steps is not None else None
        r, _, _ = scene.intersect(o[i], d[i], float(m[i]), translucent, counters=ctr)
        if steps is not None:
            steps[i] = ctr.iterations
        if r.t > 0:
            out[i]["dst"], out[i]["value"], out[i]["face_id"], out[i]["inside_voxel"], out[i]["pos"] = r.t, r.value, r.face_id, r.inside_voxel != 0, list(r.pos)
        else:
            out[i]["dst"] = -1.0
    return out


def build_rays_for(info, seed):
    """(origins [N,3], dirs [N,3], max_dst [N], kinds [N]) of 1252 (glasshouse) / 1362 (far_chunks, with the LOD chunk's rays) rays, shuffled; `kinds` names the group each ray was made for.
    No NaN, infinite or all-zero direction."""
    rng = np.random.default_rng(seed)
    scene, lo, hi, size = info["scene"], info["lo"].astype(np.float64), info["hi"].astype(np.float64), info["size"]
    glass, leaves = exposed(info, blocks_of(info, [GLASS])), exposed(info, blocks_of(info, [LEAVES]))
    opaque = blocks_of(info, [GRASS, DIRT, STONE, BRICKS, SAND, LOG, COBBLE])
    top_y = float(lo[1] + (13 if info["name"] == "far_chunks" else 10))  # above the terrain (the glasshouse's walls end at 9)
    o, d, m, kinds = [], [], [], []

    def add(kind, p, v, md=-1.0):
        v = np.asarray(v, dtype=np.float32)
        assert np.isfinite(v).all() and (v != 0).any()
        o.append(np.asarray(p, dtype=np.float32))
        d.append(v)
        m.append(np.float32(md))
        kinds.append(kind)

    def towards(block, dist_lo=1.2, dist_hi=8.0, jitter=0.35):
        """An origin in the air and a direction towards a point in `block`."""
        for _ in range(2000):
            v = random_unit(rng)
            target = block + 0.5 + rng.uniform(-jitter, jitter, 3)
            p = target - v.astype(np.float64) * rng.uniform(dist_lo, dist_hi)
            if block_at(info, p) == AIR and p[1] > lo[1] + 1:
                return np.float32(p), unit(target - np.float32(p).astype(np.float64))
        raise AssertionError("no origin in the air")

    def inside_region():
        return rng.uniform(lo, hi)

    def in_air(y_lo=None):
        for _ in range(200):
            p = inside_region()
            if y_lo is not None:
                p[1] = rng.uniform(y_lo, y_lo + 6.0)
            if block_at(info, p) == AIR:
                return p
        raise AssertionError("no air")

    through = []  # (origin, dir) of the rays aimed at panes and leaves: reused with other max_dst
    for k in range(130):  # through glass
        p, v = towards(glass[rng.integers(len(glass))])
        through.append((p, v))
        add("glass", p, v, -1.0 if k % 4 else 1.0e5)  # (every fourth: a max_dst beyond everything)
    for k in range(100):  # through leaves
        p, v = towards(leaves[rng.integers(len(leaves))])
        through.append((p, v))
        add("leaves", p, v, -1.0 if k % 4 else 3.0e4)
    for _ in range(60):  # along the panes: nearly parallel to x or z, grazing or inside them
        g = glass[rng.integers(len(glass))]
        v = unit([1.0, rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03)])
        if rng.random() < 0.3:
            v = v[[2, 1, 0]]
        v = v * np.float32(rng.choice([-1.0, 1.0]))
        p = g + 0.5 + rng.uniform(-0.6, 0.6, 3) - v.astype(np.float64) * rng.uniform(1.0, 10.0)
        add("along", p, v)
    for name, where, n in (("in_glass", glass, 50), ("in_leaves", leaves, 50), ("in_opaque", opaque, 80)):
        for _ in range(n):
            add(name, where[rng.integers(len(where))] + rng.uniform(0.05, 0.95, 3), random_unit(rng))
    # outside the octree, up to 8 blocks out on every side, aimed at the solid part of the chunks
    for k in range(120):
        axis, far = k % 3, (k // 3) % 2
        target = rng.uniform(lo + [1, 0.5, 1], [hi[0] - 1, lo[1] + 6.0, hi[2] - 1])
        p = target + rng.uniform(-6.0, 6.0, 3)
        p[axis] = size + rng.uniform(0.01, 8.0) if far else -rng.uniform(0.01, 8.0)
        add("outside_in", p, unit(target - p))
    for k in range(40):  # ... and aimed away
        axis, far = k % 3, (k // 3) % 2
        p = inside_region()
        p[axis] = size + rng.uniform(0.01, 8.0) if far else -rng.uniform(0.01, 8.0)
        v = random_unit(rng)
        v[axis] = abs(v[axis]) + np.float32(0.05) if far else -abs(v[axis]) - np.float32(0.05)
        add("outside_away", p, unit(v))
    for k in range(48):  # exactly on the border, at 0 and at 2^depth; a third of them run in the border's own plane
        axis, far = k % 3, (k // 3) % 2
        target = rng.uniform(lo + [1, 0.5, 1], [hi[0] - 1, lo[1] + 6.0, hi[2] - 1])
        p = target + rng.uniform(-3.0, 3.0, 3)
        p[axis] = size if far else 0.0
        v = unit(target - p)
        if k % 3 == 2:
            v[axis] = 0.0
            v = unit(v)
        add("border", p, v)
    for k in range(90):  # integral coordinates: voxel faces, edges and corners
        p = opaque[rng.integers(len(opaque))].astype(np.float64) + rng.integers(-1, 3, 3) + rng.uniform(0.0, 1.0, 3)
        which = [(0,), (1,), (2,), (0, 1), (1, 2), (0, 1, 2)][k % 6]
        for a in which:
            p[a] = np.round(p[a])
        add("integral", p, random_unit(rng) if k % 2 else unit(np.eye(3)[k % 3] * (1.0 if k % 4 else -1.0)))
    axes = [[0, -1, 0], [1, 0, 0], [0, 0, -1], [1, -1, 0], [0, -1, 1], [-1, -1, 0], [1, 0, 1], [0, 1, 0], [-1, 0, 0], [0, -2, -1], [0, 0, 1], [2, 1, 0]]
    for k in range(84):  # one or two components exactly 0.0 or -0.0
        v = unit(axes[k % len(axes)])
        if k % 2:
            v = np.where(v == 0, np.float32(-0.0), v)
        add("zeros", in_air(top_y - 8.0), v, -1.0 if k % 3 else 50.0)
    for k in range(40):  # a component of magnitude 1e-30
        v = random_unit(rng)
        v[k % 3] = np.float32(1e-30 if k % 2 else -1e-30)
        add("tiny_dir", in_air(top_y - 8.0), v)
    for k in range(40):  # max_dst tiny
        p, v = through[rng.integers(len(through))]
        add("tiny_dst", p if k % 2 else opaque[rng.integers(len(opaque))] + rng.uniform(0.05, 0.95, 3), v, 1e-6)
    n_between = 0
    for _ in range(2000):  # max_dst between a pane (or leaves) and what lies behind it
        if n_between == 60:
            break
        p, v = towards(glass[rng.integers(len(glass))] if rng.random() < 0.7 else leaves[rng.integers(len(leaves))])
        near, _, _ = scene.intersect(p, v, -1.0, False)
        behind, _, _ = scene.intersect(p, v, -1.0, True)
        if near.t > 0 and behind.t > near.t + 0.01:
            add("between", p, v, 0.5 * (near.t + behind.t))
            n_between += 1
    assert n_between == 60
    n_cut = 0
    for _ in range(2000):  # ended by max_dst before the hit
        if n_cut == 50:
            break
        p = in_air(top_y)
        v = unit([rng.uniform(-0.5, 0.5), -1.0, rng.uniform(-0.5, 0.5)])
        r, _, _ = scene.intersect(np.float32(p), v, -1.0, False)
        if r.t > 1.0:
            add("cut", p, v, r.t * rng.uniform(0.2, 0.9))
            n_cut += 1
    assert n_cut == 50
    for _ in range(150):  # skimming the terrain, nearly level: a long walk through small empty cells
        p = inside_region()
        edge = int(rng.integers(0, 4))
        p[0 if edge < 2 else 2] = (lo if edge % 2 == 0 else hi)[0 if edge < 2 else 2] + (0.3 if edge % 2 == 0 else -0.3)
        p[1] = lo[1] + (rng.uniform(11.05, 12.5) if info["name"] == "far_chunks" else rng.uniform(1.05, 2.5))
        target = inside_region()
        target[1] = p[1] - rng.uniform(0.0, 1.0)
        target[0 if edge < 2 else 2] = (hi if edge % 2 == 0 else lo)[0 if edge < 2 else 2]
        add("skim", p, unit(target - p))
    for _ in range(60):  # towards the sky
        add("sky", in_air(top_y), unit([rng.uniform(-1, 1), rng.uniform(0.2, 1.5), rng.uniform(-1, 1)]), -1.0 if rng.random() < 0.5 else 64.0)
    if info["lod_box"] is not None:  # the LOD chunk: from above and from the sides, and origins inside its large voxels
        a, b = (v.astype(np.float64) for v in info["lod_box"])
        for _ in range(80):
            target = rng.uniform(a + [1, 0, 1], [b[0] - 1, a[1] + 10.0, b[2] - 1])
            v = unit([rng.uniform(-1, 1), rng.uniform(-1.5, -0.1), rng.uniform(-1, 1)])
            add("lod", target - v.astype(np.float64) * rng.uniform(4.0, 20.0), v)
        for _ in range(30):
            add("in_lod", rng.uniform(a + [0, 0, 0], [b[0], a[1] + 10.0, b[2]]), random_unit(rng))
    order = rng.permutation(len(o))
    o, d, m = (np.ascontiguousarray(np.asarray(x, dtype=np.float32)[order]) for x in (o, d, m))
    kinds = np.asarray(kinds)[order]
    assert o.shape == d.shape == (len(m), 3) and np.isfinite(o).all() and np.isfinite(d).all() and (d != 0).any(axis=1).all()
    return o, d, m, kinds


def ray_counts(info, o, d, m, opaque, through, steps):
    """The figures behind "the ray set holds every kind", from the oracle's results alone. `values` are the block ids hit. `other_values` are
    what the reference itself reports for some rays of a CSVO world that start inside a voxel (inside_voxel = 1: the walk inside the voxel
    reads the leaf's material where there is none): 0, or bytes of the arena read as an id. They are the oracle's, the device code has to
    give the same, and they do not count as block ids."""
    size = info["size"]
    differ = np.array([opaque[i].tobytes() != through[i].tobytes() for i in range(len(o))])
    outside = ((o < 0) | (o > size)).any(axis=1)
    c = dict(rays=len(o), differ=int(differ.sum()), differ_value=int((differ & (opaque["value"] != through["value"])).sum()),
             through_glass=int((differ & (opaque["value"] == GLASS) & (through["dst"] > opaque["dst"]) & (opaque["dst"] > 0)).sum()))
    for name, hits in (("opaque", opaque), ("through", through)):
        hit = hits["dst"] > 0
        c[name] = dict(inside_voxel=int((hits["inside_voxel"] != 0).sum()), miss=int((~hit).sum()), outside_hit=int((outside & hit).sum()),
                       values=sorted(int(v) for v in np.unique(hits["value"][hit]) if 1 <= v <= COBBLE),
                       other_values=sorted(int(v) for v in np.unique(hits["value"][hit & (hits["inside_voxel"] != 0)]) if not 1 <= v <= COBBLE), faces=sorted(int(v) for v in np.unique(hits["face_id"][hit])))
        if info["lod_box"] is not None:
            a, b = info["lod_box"]
            c[name]["lod_hits"] = int((hit & (hits["pos"] >= a - 1e-3).all(axis=1) & (hits["pos"] <= b + 1e-3).all(axis=1)).sum())
    c["integral"] = int((o == np.round(o)).any(axis=1).sum())
    c["wander"] = int((steps > 3 * info["depth"]).sum())
    return c, differ


def cut_short(scene, o, d, m, hits, translucent):
    """How many rays that miss with their max_dst would hit beyond it."""
    n = 0
    for i in np.flatnonzero((hits["dst"] < 0) & (m > 0)):
        r, _, _ = scene.intersect(o[i], d[i], -1.0, translucent)
        n += bool(r.t > m[i])
    return n


# ---- entities ---------------------------------------------------------------------------------------------------------------------


def _free_above(info, b, n):
    return all(block_at(info, b + [0, k, 0]) == AIR for k in range(1, n + 1))


def sunk_contact(info, contacts):
    """A sunk box's contacts hold one below 2 * kPhysicsEpsilon = 0.001, the distance under which Physics::apply_axial_physics stops the box.
    The traversal works on positions scaled to [1, 2), where fp32 has steps of 2^-23: 2^(depth - 23) blocks. An axis-parallel ray's hit
    distance is a multiple of that quantum. At depth 6 the quantum is 7.6e-6 and the bound is met as it stands; at depth 14 it is 2^-9 =
    0.00195 > 0.001, so no fan ray of far_chunks can report a positive distance below 0.001 whatever the seed: there the smallest
    distance the world can express is asked for, one quantum."""
    quantum = info["size"] * 2.0 ** -23
    c = np.asarray(contacts)
    return bool(((c >= 0) & (c < 2 * 0.0005)).any()) if quantum < 2 * 0.0005 else bool((c == np.float32(quantum)).any())


def build_entities_for(info, seed):
    """(rows of host.make_entities, roles: name -> row indices)."""
    rng = np.random.default_rng(seed)
    scene, lo, hi, size = info["scene"], info["lo"].astype(np.float64), info["hi"].astype(np.float64), info["size"]
    far = info["name"] == "far_chunks"
    top = float(lo[1] + 31.0)
    rows, roles = [], {}

    def add(role, pos, vel=(0.0, 0.0, 0.0), extents=(0.8, 1.8, 0.8), wall_clip=False, flying=False):
        off = (-extents[0] / 2, 0.0, -extents[2] / 2)
        r = host.make_entities([pos], extents=extents, offset=off)
        r[0, 3:6] = vel
        r[0, 12], r[0, 13] = float(wall_clip), float(flying)
        roles.setdefault(role, []).append(len(rows))
        rows.append(r[0])

    def ground(x, z, extents=(0.8, 1.8, 0.8)):
        return ground_under(scene, x, z, top, (-extents[0] / 2, 0.0, -extents[2] / 2), extents)

    def detail_xz(margin=2.0):
        for _ in range(100):
            x, z = rng.uniform(lo[0] + margin, hi[0] - margin), rng.uniform(lo[2] + margin, hi[2] - margin)
            if info["lod_box"] is None or not (info["lod_box"][0][0] - 2 <= x <= info["lod_box"][1][0] + 2 and info["lod_box"][0][2] - 2 <= z <= info["lod_box"][1][2] + 2):
                return x, z
        raise AssertionError

    for k in range(8):  # players' boxes on and above the ground
        x, z = detail_xz()
        up = [0.0, 0.0005, 0.01][k] if k < 3 else rng.uniform(0.3, 2.5)
        add("players", (x, ground(x, z) + up, z), (rng.uniform(-6, 6), 0.0, rng.uniform(-6, 6)), wall_clip=k in (1, 5), flying=k in (4,))
    # standing on glass: the ceiling / a glass block with two blocks of air above it
    glass = blocks_of(info, [GLASS])
    if far:
        g = next(b for b in glass if _free_above(info, b, 3) and b[1] > lo[1] + 12)
        wall = next(b for b in glass if b[1] > lo[1] + 12 and all(block_at(info, b + [dx, dy, -1]) == AIR for dx in (-1, 0, 1) for dy in (-1, 0, 1, 2))
                    and all(block_at(info, b + [dx, dy, 0]) == AIR for dx in (-1, 1) for dy in (0, 1, 2)) and _free_above(info, b, 2) and (b != g).any())
    else:
        g, wall = np.array([9, 12, 23]), np.array([12, 1, 10])
    # (0.016 above it: a grounded box still sinks by gravity * dt * dt = 0.00096 a step until its contact falls below 2 * kPhysicsEpsilon, and
    # where the smallest contact the world can express is larger than that -- far_chunks -- it would reach the glass and fall into it)
    add("on_glass", (g[0] + 0.5, g[1] + 1.0 + 0.016, g[2] + 0.5))
    # against the glass wall (its -z side), moving into it
    add("into_glass", (wall[0] + 0.5, wall[1] + 0.02, wall[2] - 0.45), (0.0, 0.0, 3.0))
    for k, ext in enumerate(SPECIAL_EXTENTS):
        x, z = (24.0, 25.0) if (not far and k == 0) else detail_xz(5.0)
        add("extents", (x, ground(x, z, ext) + 0.5, z), (5.0, 0.0, -4.0), extents=ext, wall_clip=k == 1)
    # Sunk into the ground: fan rays start inside voxels. Such a ray hits the NEXT voxel on its way (svo.esvo.glsl:183-185), so the box's -x
    # side is put a hair beyond a block boundary inside the ground: the oracle then reports a contact below 2 * kPhysicsEpsilon there
    # (far_chunks: of one quantum, see sunk_contact).
    for depth in (0.3, 0.5, 0.7):
        for attempt in range(400):
            x, z = detail_xz()
            x = np.floor(x) + 0.4 + (1 + attempt % 8) * 2.0 ** -12  # (quarters of the fp32 spacing at 12,800)
            pos = (x, ground(x, z) - depth, z)
            row = host.make_entities([pos])
            contacts = np.asarray(oracle_contacts(scene, row))[0]
            if sunk_contact(info, contacts):
                break
        else:
            raise AssertionError("no place for a sunk box")
        add("sunk", pos, (rng.uniform(-3, 3), 0.0, rng.uniform(-3, 3)))
    # within 1.5 blocks of the world's border, moving outward
    y = lo[1] + 16.0 if far else 1.0
    add("outward", (size - 1.1, y, 0.5 * (lo[2] + hi[2])), (6.0, 0.0, 0.0))
    add("outward", (0.5 * (lo[0] + hi[0]), y, 1.0), (0.0, 0.0, -6.0), flying=True)
    add("outside", (-5.0, lo[1] + 0.5, 0.5 * (lo[2] + hi[2])), (1.0, 0.0, 0.0), flying=True)
    if info["lod_box"] is not None:  # half over the LOD chunk, half over the full-detail chunk beside it
        a, b = info["lod_box"]
        x, z, ext = float(a[0]), float(a[2]) + 14.3, (2.6, 1.8, 2.6)
        add("straddle", (x, ground(x, z, ext) + 0.2, z), (-2.0, 0.0, 1.0), extents=ext)
    return np.ascontiguousarray(np.stack(rows)).astype(np.float32), roles


def oracle_run(scene, rows, steps=STEPS):
    """`steps` oracle-backed steps of DT: [(rows after step k, the contacts step k was computed from)]."""
    rows = rows.copy()
    out = []
    for _ in range(steps):
        contacts = np.ascontiguousarray(oracle_step(scene, DT, rows), dtype=np.float32)
        out.append((rows.copy(), contacts))
    return out


def first_difference(got, exp, what, describe):
    """tobytes() == with a message: the first differing record, what it belongs to and both records."""
    if got.tobytes() == exp.tobytes():
        return
    assert len(got) == len(exp), (what, len(got), len(exp))
    bad = [i for i in range(len(exp)) if got[i].tobytes() != exp[i].tobytes()]
    i = bad[0]
    raise AssertionError(f"{what}: {len(bad)} of {len(exp)} records differ; first at {i}: {describe(i)}\n  got      {got[i]}\n  expected {exp[i]}")


# ---- a case: one world in one format, its rays and entities, and what the oracle says of them ----------------------------------------


class Case:
    pass


CASES = [(name, fmt) for name in ("glasshouse", "far_chunks") for fmt in ("esvo", "csvo")]


def make_case(name, fmt):
    """Everything the tests share, computed once and left unchanged."""
    c = Case()
    c.name, c.fmt, c.svo_type = name, fmt, host.SVO_ESVO if fmt == "esvo" else host.SVO_CSVO
    c.world, c.scene, c.tex, c.mats, c.info = BUILDERS[name](c.svo_type)
    c.o, c.d, c.m, c.kinds = build_rays_for(c.info, RAY_SEED[name])
    c.steps = np.zeros(len(c.o), dtype=np.uint64)
    c.opaque = oracle_hits(c.scene, c.o, c.d, c.m, False, steps=c.steps)
    c.through = oracle_hits(c.scene, c.o, c.d, c.m, True)
    c.counts, c.differ = ray_counts(c.info, c.o, c.d, c.m, c.opaque, c.through, c.steps)
    c.rows, c.roles = build_entities_for(c.info, ENTITY_SEED[name])
    c.run = oracle_run(c.scene, c.rows)
    c.start_contacts = c.run[0][1]  # (what a call of no steps at the start answers)
    c.final_contacts = np.ascontiguousarray(oracle_contacts(c.scene, c.run[-1][0]), dtype=np.float32)
    for a in (c.o, c.d, c.m, c.opaque, c.through, c.rows, c.final_contacts) + tuple(x for pair in c.run for x in pair):
        a.setflags(write=False)
    return c


def describe_ray(c, i):
    return f"ray {i} ({c.kinds[i]}): origin {c.o[i]!r} dir {c.d[i]!r} max_dst {c.m[i]!r}"


def describe_entity(c, i):
    role = next((r for r, idx in c.roles.items() if i in idx), "?")
    return f"entity {i} ({role}): start {c.rows[i]!r}"
