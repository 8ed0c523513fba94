"""Shared by the tests of vx_trace_rays (test_trace_rays_on_host.py, test_trace_rays.py): a 64 x 48 view of each of three worlds -- the depth-7
heightfield, `glasshouse` and `far_chunks` (batch_cases.py) -- whose camera rays come from the oracle's or_primary_ray and whose expected
pixels and records come from OracleScene.render; 1237 free rays over the heightfield and far_chunks with what OracleScene.intersect says of
them; and a float64 restatement of get_sky_color. Everything is seeded and computed once per (world, format); nothing of the code under test
is used."""
import ctypes as C
import functools

import numpy as np

from batch_cases import far_chunks, glasshouse
from helpers import orc, vra  # noqa: F401
from physics_cases import heightfield
from voxel_rs_amd import hip, host, scenes

W, H = 64, 48
N_FREE, N_GRID = 1237, 1024  # 19 waves + 21 lanes; the first 1024 are a 32 x 32 orthographic grid
GRID_DIR = np.float64([0.3, -0.9, 0.2])
TOL = 5e-6  # the project's stated colour tolerance (include/voxel_hip.h)
SVO = {"esvo": host.SVO_ESVO, "csvo": host.SVO_CSVO}

# eye, forward, shadow_distance and the pixel whose block is highlighted, per world (positions relative to `anchor`, see view_of)
VIEWS = {
    "heightfield": dict(eye=(64.0, 4.6, 64.0), fwd=(0.6, -0.42, 0.7), shadow_distance=30.0, pick=(31, 8)),
    "glasshouse": dict(eye=(15.3, 4.2, 1.7), fwd=(0.12, -0.22, 1.0), shadow_distance=17.0, pick=(10, 0)),
    "far_chunks": dict(eye=(6.3, 14.4, 5.2), fwd=(0.6, -0.36, 0.7), shadow_distance=30.0, pick=(44, 2)),
}


class Case:
    pass


def as_oracle(u):
    return orc.Uniforms.from_buffer_copy(bytes(u))


def build_world(name, fmt):
    """(world, oracle scene, textures, materials, anchor of the view, region (lo, hi) of the blocks, lod box or None)"""
    svo_type = SVO[fmt]
    if name == "heightfield":
        world, scene, tex, mats, h_max = heightfield(svo_type, 7)
        ground, _, _ = scene.intersect(np.float32([64.0, h_max + 2.0, 64.0]), np.float32([0, -1, 0]), -1.0, False)  # under the eye
        return world, scene, tex, mats, np.float64([0, ground.pos[1], 0]), (np.float64([0, 0, 0]), np.float64([128, h_max + 1, 128])), None
    world, scene, tex, mats, info = (glasshouse if name == "glasshouse" else far_chunks)(svo_type)
    lo, hi = info["lo"].astype(np.float64), info["hi"].astype(np.float64)
    return world, scene, tex, mats, lo, (lo, hi), info["lod_box"]


def view_of(name, anchor, cam_shift=(0.0, 0.0, 0.0), highlight=None):
    """The view's uniforms: shadows on, a finite shadow distance. cam_shift moves uniforms.cam_pos alone -- the view matrix, and so every ray,
    stays where it is (world.glsl:118 takes the origin from u_view; u_cam_pos feeds the specular term, :73)."""
    v = VIEWS[name]
    eye = np.float64(v["eye"]) + anchor
    view = scenes.view_matrix(eye, v["fwd"], (0.0, 1.0, 0.0))
    light = scenes._normalize((-1.0, -1.0, -1.0))
    return hip.make_uniforms(view, np.radians(72.0), W / H, 0.3, light, eye + np.float64(cam_shift), True, v["shadow_distance"], highlight)


def camera_rays(u):
    """(origins [W*H, 3], dirs [W*H, 3]) of the view's pixels at y * W + x, by the oracle's or_primary_ray."""
    o, d = np.zeros((W * H, 3), dtype=np.float32), np.zeros((W * H, 3), dtype=np.float32)
    ou = as_oracle(u)
    ro, rd = (C.c_float * 3)(), (C.c_float * 3)()
    for y in range(H):
        for x in range(W):
            orc.lib().or_primary_ray(C.byref(ou), W, H, x, y, C.byref(ro), C.byref(rd))
            o[y * W + x], d[y * W + x] = list(ro), list(rd)
    return o, d


def kind_counts(scene, o, d, hits):
    """How many pixels of each kind the oracle's records hold; `through`: hits whose primary passed through a translucent block (the opaque
    cast of the same ray stops nearer)."""
    f = hits["flags"].ravel()
    c = dict(sky=int(((f & 1) == 0).sum()), lit=int((((f & 2) != 0) & ((f & 4) == 0)).sum()), shadow=int(((f & 4) != 0).sum()),
             beyond=int((((f & 1) != 0) & ((f & 2) == 0) & ((f & 8) == 0)).sum()), outline=int(((f & 8) != 0).sum()))
    through = 0
    t = hits["t"].ravel()
    for i in np.flatnonzero((f & 1) != 0):
        r, _, _ = scene.intersect(o[i], d[i], -1.0, False)
        through += bool(0 < r.t < t[i])
    c["through"] = through
    return c


@functools.lru_cache(maxsize=None)
def camera_case(name, fmt):
    """Case 1 and 2 of one world in one format: uniforms, rays, and the oracle's image and records -- with cam_pos at the eye (`img`, `hits`) and,
    for the heightfield, 20 blocks away from it (`img_moved`, `hits_moved`)."""
    c = Case()
    c.name, c.fmt, c.svo_type = name, fmt, SVO[fmt]
    c.world, c.scene, c.tex, c.mats, c.anchor, c.region, c.lod_box = build_world(name, fmt)
    plain = view_of(name, c.anchor)
    c.o, c.d = camera_rays(plain)
    # the highlighted block: the one the oracle sees at the view's `pick` pixel
    px, py = VIEWS[name]["pick"]
    r, _, _ = c.scene.intersect(c.o[py * W + px], c.d[py * W + px], -1.0, True)
    assert r.t > 0
    c.highlight = tuple(float(np.floor(v)) + 0.5 for v in r.pos)
    c.u = view_of(name, c.anchor, highlight=c.highlight)
    c.img, c.hits = c.scene.render(as_oracle(c.u), W, H)
    c.counts = kind_counts(c.scene, c.o, c.d, c.hits)
    if name == "heightfield":
        c.u_moved = view_of(name, c.anchor, cam_shift=(12.0, 16.0, 0.0), highlight=c.highlight)  # |shift| = 20
        c.img_moved, c.hits_moved = c.scene.render(as_oracle(c.u_moved), W, H)
    for a in (c.o, c.d, c.img, c.hits):
        a.setflags(write=False)
    return c


# ---- free rays ---------------------------------------------------------------------------------------------------------------------


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return (v / np.linalg.norm(v)).astype(np.float32)


def sky_color(rd):
    """world.glsl:92-108 in float64, the acos argument clamped as include/voxel_hip.h states; (N, 3) directions -> (N, 4) pixels."""
    rd = np.asarray(rd, dtype=np.float64).reshape(-1, 3)
    sky = np.float64([135.0, 206.0, 235.0]) / 255.0
    horizon = 1.0 * (1.0 - 0.3) + sky * 0.3
    flat = rd * [1.0, 0.0, 1.0]
    p = flat / np.linalg.norm(flat, axis=1, keepdims=True)
    a = np.arccos(np.clip((rd * p).sum(axis=1) / np.linalg.norm(rd, axis=1) * np.linalg.norm(p, axis=1), -1.0, 1.0))
    grad = a / 1.570796
    grad = 1.0 - (1.0 - grad) ** 3
    out = np.ones((len(rd), 4))
    out[:, :3] = horizon * (1.0 - grad[:, None]) + sky * grad[:, None]
    return out


def build_free_rays(scene, region, top, seed):
    """(origins, dirs, max_dst, kinds) of N_FREE rays. The first N_GRID: a 32 x 32 grid of parallel rays along GRID_DIR from the height `top`
    down onto the region, no limit. Then 213 in the manner of test_raycast_batch.build_rays: 53 origins inside the ground, 50 rays towards the
    sky, 50 with signed-zero direction components, 60 whose max_dst ends them before their hit. No direction has rd.x = rd.z = 0 (the shader's
    sky term is 0/0 there)."""
    rng = np.random.default_rng(seed)
    lo, hi = region
    g = unit(GRID_DIR)
    o, d, m, kinds = [], [], [], []
    drift = g.astype(np.float64) * ((top - lo[1]) / -float(g[1]))  # how far a grid ray travels sideways before it reaches the region's floor
    for iz in range(32):
        for ix in range(32):
            target = np.float64([lo[0] + (ix + 0.37) * (hi[0] - lo[0]) / 32.0, lo[1], lo[2] + (iz + 0.61) * (hi[2] - lo[2]) / 32.0])
            o.append(target - 0.6 * drift + [0.0, 0.0, 0.0])  # (0.6: the outer rays come down beside the region, or leave the octree: misses)
            o[-1][1] = top
            d.append(g)
            m.append(-1.0)
            kinds.append("grid")

    def xz():
        return rng.uniform(lo[0] + 3.0, hi[0] - 3.0), rng.uniform(lo[2] + 3.0, hi[2] - 3.0)

    def surface(x, z):
        r, _, _ = scene.intersect(np.float32([x, top, z]), np.float32([0, -1, 0]), -1.0, False)
        assert r.t > 0
        return np.float64(list(r.pos))

    for _ in range(53):  # from inside the ground
        s = surface(*xz())
        o.append([s[0], s[1] - rng.uniform(0.1, 0.8), s[2]])
        d.append(unit(rng.uniform(-1, 1, 3)))
        m.append(-1.0)
        kinds.append("inside")
    for _ in range(50):  # towards the sky
        x, z = xz()
        o.append([x, top + rng.uniform(1.0, 8.0), z])
        d.append(unit([rng.uniform(-1, 1), rng.uniform(0.2, 1.5), rng.uniform(-1, 1)]))
        m.append(-1.0 if rng.random() < 0.5 else 64.0)
        kinds.append("sky")
    axes = [[1, 0, 0], [0, 0, -1], [1, -1, 0], [0, -1, 1], [-1, -1, 0], [1, 0, 1], [-1, 0, 0], [0, -2, -1], [0, 0, 1], [2, 1, 0]]
    for k in range(50):  # one or two components 0.0 or -0.0
        s = surface(*xz())
        v = unit(axes[k % len(axes)])
        if k % 2:
            v = np.where(v == 0, np.float32(-0.0), v)
        o.append([s[0], s[1] + rng.uniform(0.2, 3.0), s[2]])
        d.append(v)
        m.append(-1.0 if k % 3 else 50.0)
        kinds.append("zeros")
    n_cut = 0
    while n_cut < 60:  # ended by max_dst before the hit
        x, z = xz()
        p = np.float32([x, top + rng.uniform(2.0, 8.0), z])
        v = unit([rng.uniform(-0.5, 0.5), -1.0, rng.uniform(-0.5, 0.5)])
        r, _, _ = scene.intersect(p, v, -1.0, True)
        if r.t > 1.0:
            o.append(p)
            d.append(v)
            m.append(r.t * rng.uniform(0.2, 0.9))
            kinds.append("cut")
            n_cut += 1
    o, d, m = (np.ascontiguousarray(np.asarray(a, dtype=np.float32)) for a in (o, d, m))
    tail = N_GRID + rng.permutation(N_FREE - N_GRID)  # (the grid stays in front: its rays share one direction)
    order = np.concatenate([np.arange(N_GRID), tail])
    o, d, m, kinds = o[order], d[order], m[order], np.asarray(kinds)[order]
    assert o.shape == d.shape == (N_FREE, 3) and m.shape == (N_FREE,) and not ((d[:, 0] == 0) & (d[:, 2] == 0)).any()
    return np.ascontiguousarray(o), np.ascontiguousarray(d), np.ascontiguousarray(m), kinds


def free_uniforms():
    """ambient = 1, no shadows, nothing highlighted: light clamps to 1 and a hit's pixel is OctreeResult.color. cam_pos is anywhere."""
    return hip.make_uniforms(np.eye(4, dtype=np.float32).ravel(), 1.0, 1.0, 1.0, scenes._normalize((-1.0, -1.0, -1.0)), (3.0, 900.0, -5.0), False, 0.0)


@functools.lru_cache(maxsize=None)
def free_case(name, fmt):
    """Case 3 of one world in one format: the rays and, per ray, what OracleScene.intersect(o, d, max_dst, True) says -- the record fields, the
    iteration count and the expected pixel (Result.color, or the sky)."""
    c = Case()
    c.name, c.fmt, c.svo_type = name, fmt, SVO[fmt]
    c.world, c.scene, c.tex, c.mats, c.anchor, c.region, c.lod_box = build_world(name, fmt)
    top = float(c.region[1][1] + (3.0 if name == "heightfield" else -14.0))  # above the terrain (far_chunks: its columns end below y = 12)
    c.o, c.d, c.m, c.kinds = build_free_rays(c.scene, c.region, top, 41 if name == "heightfield" else 42)
    c.u = free_uniforms()
    n = len(c.o)
    c.exp = np.zeros(n, dtype=hip.HIT_DTYPE)
    c.color = np.zeros((n, 4), dtype=np.float64)
    c.inside = np.zeros(n, dtype=bool)
    sky = sky_color(c.d)
    for i in range(n):
        ctr = orc.Counters()
        r, _, _ = c.scene.intersect(c.o[i], c.d[i], float(c.m[i]), True, counters=ctr)
        e = c.exp[i]
        e["t"], e["value"], e["face_id"], e["pos"], e["lod"], e["uv"] = r.t, r.value, r.face_id, list(r.pos), r.lod, list(r.uv)
        e["flags"], e["shadow_t"], e["steps"] = int(r.t != -1.0), -1.0, ctr.iterations
        c.color[i] = list(r.color) if r.t != -1.0 else sky[i]
        c.inside[i] = r.inside_voxel != 0
    c.cut = 0
    for i in np.flatnonzero((c.exp["t"] == -1.0) & (c.m > 0)):
        r, _, _ = c.scene.intersect(c.o[i], c.d[i], -1.0, True)
        c.cut += bool(r.t > c.m[i])
    for a in (c.o, c.d, c.m, c.exp, c.color):
        a.setflags(write=False)
    return c


# ---- what the harness and the contexts are handed -----------------------------------------------------------------------------------------


def scene_arguments(c):
    """The world's frame, the materials and the texture chain as the on-host harnesses' entries take them (test_batch_cases_on_host.py)."""
    frame = np.concatenate([c.world.frame(pad_words=0), np.zeros(4, dtype=np.uint32)])  # (the 16 zero bytes a context keeps behind the world buffer)
    levels = orc.mip_chain(c.tex, 6)
    chain = np.concatenate([lv.ravel() for lv in levels])
    offsets = np.cumsum([0] + [lv.size for lv in levels[:-1]])
    level_offset = (C.c_uint32 * 16)(*[int(v) for v in offsets])
    mats = np.ascontiguousarray(c.mats.view(orc.MATERIAL_DTYPE))
    return frame, mats, chain, len(levels), level_offset


def pack_rgba8(rgba):
    """glReadPixels(RGBA, UNSIGNED_BYTE) of float pixels: clamp to [0, 1], round to the nearest of 255 steps, NaN -> 0; (N, 4) uint8."""
    f = np.asarray(rgba, dtype=np.float32)
    f = np.where(np.isnan(f), np.float32(0), np.clip(f, np.float32(0), np.float32(1)))
    return (f * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)


def assert_records(got, exp, what):
    """vx_hit records byte for byte, with the first difference named."""
    if got.tobytes() == exp.tobytes():
        return
    g, e = got.ravel(), exp.ravel()
    bad = [i for i in range(len(e)) if g[i].tobytes() != e[i].tobytes()]
    raise AssertionError(f"{what}: {len(bad)} of {len(e)} records differ; first at {bad[0]}\n  got      {g[bad[0]]}\n  expected {e[bad[0]]}")


def assert_colors(got, exp, what):
    diff = np.abs(np.asarray(got, dtype=np.float64).reshape(-1, 4) - np.asarray(exp, dtype=np.float64).reshape(-1, 4))
    assert not np.isnan(diff).any(), f"{what}: NaN in a colour"
    worst = float(diff.max())
    print(f"{what}: largest colour difference {worst:.3g}")
    assert worst <= TOL, f"{what}: colours differ by {worst:.3g} at ray {int(diff.max(axis=1).argmax())}"
