"""vx_trace_rays on the GPU: shaded ray batches in host or device memory (voxel-rs_amd/csrc/trace), against the oracle (OracleScene.render for
camera rays, OracleScene.intersect for free rays) and against the entry points it stands beside (vx_render with hit records, vx_physics_step).
Records are compared byte for byte, colours within the project's 5e-6. The cases -- a 64 x 48 view of three worlds, 1237 free rays over two --
are those of tests/trace_cases.py, computed once and left unchanged; test_trace_rays_on_host.py shows from the oracle's results that they hold
every kind of pixel and ray."""
import ctypes as C

import numpy as np
import pytest

import trace_cases as tc
from gpu_harness import to_device
from helpers import orc, vra  # noqa: F401
from physics_cases import DT, heightfield, place_entities
from voxel_rs_amd import hip

pytestmark = pytest.mark.gpu
_vp = C.c_void_p
FORMATS = [hip.VX_FORMAT_RGBA32F, hip.VX_FORMAT_RGBA8]
FORMAT_IDS = ["rgba32f", "rgba8"]


def make_context(c):
    svo = hip.Svo(c.svo_type, c.world.size_in_bytes + (1 << 20))
    svo.set_materials(c.mats)
    svo.set_textures(c.tex, 6)
    svo.update(c.world)
    return svo


@pytest.fixture(scope="module")
def contexts():
    """One context per (world, format), made when first asked for and closed with the module."""
    made = {}

    def get(name, fmt):
        if (name, fmt) not in made:
            made[name, fmt] = make_context(tc.camera_case(name, fmt))
        return made[name, fmt]

    yield get
    for svo in made.values():
        svo.close()


def assert_pixels(fmt, got, exp_colors, what):
    """RGBA32F within 5e-6. RGBA8: a byte may differ by one step only where the expected float lies within 5e-6 * 255 of a rounding boundary."""
    exp = np.asarray(exp_colors, dtype=np.float64).reshape(-1, 4)
    if fmt == hip.VX_FORMAT_RGBA32F:
        tc.assert_colors(got, exp, what)
        return
    scaled = np.clip(exp, 0.0, 1.0) * 255.0 + 0.5
    lo, hi = np.floor(scaled - tc.TOL * 255.0), np.floor(scaled + tc.TOL * 255.0)
    g = np.asarray(got, dtype=np.float64).reshape(-1, 4)
    assert ((g >= lo) & (g <= np.minimum(hi, 255.0))).all(), f"{what}: an RGBA8 byte is not the packing of a colour within 5e-6 of the expected one"


@pytest.mark.parametrize("name,fmt", [(n, f) for n in ("heightfield", "glasshouse", "far_chunks") for f in ("esvo", "csvo")])
def test_camera_rays_are_the_render(contexts, name, fmt):
    """1: the 3072 rays of a 64 x 48 view (or_primary_ray), shadows on, a finite shadow distance, a highlighted block: records are the oracle's
    render's and Svo.render's byte for byte, colours within 5e-6 of both."""
    c, svo = tc.camera_case(name, fmt), contexts(name, fmt)
    rgba, hits = svo.trace_rays(c.u, c.o, c.d, want_hits=True)
    tc.assert_records(hits, c.hits, f"{name}-{fmt} against the oracle")
    tc.assert_colors(rgba, c.img, f"{name}-{fmt} against the oracle")
    img, rhits = svo.render(c.u, tc.W, tc.H, want_hits=True)
    tc.assert_records(hits, rhits, f"{name}-{fmt} against vx_render")
    tc.assert_colors(rgba, img, f"{name}-{fmt} against vx_render")


@pytest.mark.parametrize("fmt", ["esvo", "csvo"])
def test_cam_pos_is_not_the_origin(contexts, fmt):
    """2: the same rays with uniforms.cam_pos 20 blocks away from the view's origin: the oracle's render with those uniforms (it reads cam_pos for
    the specular term only), and at least 20 pixels that differ from case 1's."""
    c, svo = tc.camera_case("heightfield", fmt), contexts("heightfield", fmt)
    rgba, hits = svo.trace_rays(c.u_moved, c.o, c.d, want_hits=True)
    tc.assert_records(hits, c.hits_moved, f"heightfield-{fmt}, cam_pos moved")
    tc.assert_colors(rgba, c.img_moved, f"heightfield-{fmt}, cam_pos moved")
    first, _ = svo.trace_rays(c.u, c.o, c.d)
    assert (np.abs(rgba - first).max(axis=1) > 0).sum() >= 20


@pytest.mark.parametrize("pixel_format", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("name,fmt", [(n, f) for n in ("heightfield", "far_chunks") for f in ("esvo", "csvo")])
def test_free_rays_are_the_oracles_casts(contexts, name, fmt, pixel_format):
    """3: 1237 rays -- a 32 x 32 orthographic grid along one tilted direction, then origins inside the ground, rays towards the sky, signed-zero
    components and rays their max_dst ends -- with ambient = 1 and no shadows: every record field is OracleScene.intersect's, a hit's pixel is
    Result.color, a miss's the float64 restatement of the sky. The grid alone, its one direction through dir_stride = 0, gives the same."""
    c, svo = tc.free_case(name, fmt), contexts(name, fmt)
    rgba, hits = svo.trace_rays(c.u, c.o, c.d, c.m, want_hits=True, fmt=pixel_format)
    tc.assert_records(hits, c.exp, f"{name}-{fmt} free rays")
    assert (hits["shadow_t"] == -1).all() and (hits["flags"] == (c.exp["t"] != -1)).all()
    assert_pixels(pixel_format, rgba, c.color, f"{name}-{fmt} free rays")
    grid_rgba, grid_hits = svo.trace_rays(c.u, c.o[:tc.N_GRID], c.d[0], -1.0, want_hits=True, fmt=pixel_format)
    assert grid_hits.tobytes() == hits[:tc.N_GRID].tobytes() and grid_rgba.tobytes() == rgba[:tc.N_GRID].tobytes()


@pytest.fixture(scope="module", params=["esvo", "csvo"])
def free(request, contexts):
    """Case 4's ground: the heightfield's free rays, its context, and the packed host call in both formats."""
    c = tc.free_case("heightfield", request.param)
    svo = contexts("heightfield", request.param)
    plain = {f: svo.trace_rays(c.u, c.o, c.d, c.m, want_hits=True, fmt=f) for f in FORMATS}
    return c, svo, plain


@pytest.mark.parametrize("pixel_format", FORMATS, ids=FORMAT_IDS)
def test_rays_held_in_picker_tasks(free, pixel_format):
    """4a: origin at +16, dir at +32, max_dst at +0 of vx_picker_task records, strides 48."""
    c, svo, plain = free
    t = np.zeros(len(c.o), dtype=hip.PICKER_TASK_DTYPE)
    t["pos"], t["dir"], t["max_dst"] = c.o, c.d, c.m
    assert t["pos"].strides == (48, 4) and t["dir"].strides == (48, 4) and t["max_dst"].strides == (48,)
    rgba, hits = svo.trace_rays(c.u, t["pos"], t["dir"], t["max_dst"], want_hits=True, fmt=pixel_format)
    assert rgba.tobytes() == plain[pixel_format][0].tobytes() and hits.tobytes() == plain[pixel_format][1].tobytes()


@pytest.mark.parametrize("pixel_format", FORMATS, ids=FORMAT_IDS)
def test_device_memory_equals_host_memory(free, pixel_format):
    """4b: torch tensors, read only after vx_sync."""
    c, svo, plain = free
    rgba, hits = svo.trace_rays(c.u, to_device(c.o), to_device(c.d), to_device(c.m), want_hits=True, fmt=pixel_format)
    svo.sync()
    assert rgba.cpu().numpy().tobytes() == plain[pixel_format][0].tobytes()
    assert hip.trace_hits_to_numpy(hits).tobytes() == plain[pixel_format][1].tobytes()


def test_rgba8_is_the_packing_of_rgba32f(free):
    """4c: clamp, round to the nearest of 255 steps, NaN -> 0, no row flip."""
    c, svo, plain = free
    assert plain[hip.VX_FORMAT_RGBA8][0].dtype == np.uint8
    assert (plain[hip.VX_FORMAT_RGBA8][0] == tc.pack_rgba8(plain[hip.VX_FORMAT_RGBA32F][0])).all()
    assert plain[hip.VX_FORMAT_RGBA8][1].tobytes() == plain[hip.VX_FORMAT_RGBA32F][1].tobytes()


@pytest.mark.parametrize("pixel_format", FORMATS, ids=FORMAT_IDS)
def test_either_output_alone(free, pixel_format):
    """4d: colours only, records only and both together agree."""
    c, svo, plain = free
    only_rgba, none = svo.trace_rays(c.u, c.o, c.d, c.m, fmt=pixel_format)
    assert none is None and only_rgba.tobytes() == plain[pixel_format][0].tobytes()
    none, only_hits = svo.trace_rays(c.u, c.o, c.d, c.m, want_hits=True, want_rgba=False, fmt=pixel_format)
    assert none is None and only_hits.tobytes() == plain[pixel_format][1].tobytes()


@pytest.mark.parametrize("pixel_format", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("count", [1, 65, tc.N_FREE])
def test_counts_and_the_tail_of_the_outputs(free, count, pixel_format):
    """4e, 4f: one ray, one wave and a lane, and all of them; outputs 64 records longer than count, prefilled: the tail stays as it was --
    in host memory and in device memory."""
    import torch

    c, svo, plain = free
    k = tc.N_FREE - count  # (the last `count` rays: the mixed kinds)
    o, d, m = (np.ascontiguousarray(a[k:]) for a in (c.o, c.d, c.m))
    px = 4 if pixel_format == hip.VX_FORMAT_RGBA8 else 16
    exp_rgba, exp_hits = plain[pixel_format][0][k:].tobytes(), plain[pixel_format][1][k:].tobytes()
    rgba, hits = np.full((count + 64) * px, 0x5a, dtype=np.uint8), np.full((count + 64) * 48, 0xa5, dtype=np.uint8)
    svo.trace_rays(c.u, o, d, m, want_hits=True, fmt=pixel_format, out=(rgba, hits))
    assert rgba[:count * px].tobytes() == exp_rgba and hits[:count * 48].tobytes() == exp_hits
    assert (rgba[count * px:] == 0x5a).all() and (hits[count * 48:] == 0xa5).all()
    d_rgba = torch.full(((count + 64) * px,), 0x5a, dtype=torch.uint8, device="cuda")
    d_hits = torch.full(((count + 64) * 48,), 0xa5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the fills run on torch's stream, the batch on the context's)
    svo.trace_rays(c.u, to_device(o), to_device(d), to_device(m), want_hits=True, fmt=pixel_format, out=(d_rgba, d_hits))
    svo.sync()
    assert d_rgba.cpu().numpy().tobytes() == rgba.tobytes() and d_hits.cpu().numpy().tobytes() == hits.tobytes()


def test_ordered_behind_a_physics_step(free):
    """4g: vx_physics_step(VX_MEM_DEVICE) and, with no synchronisation in between, a batch whose origins are the entities' positions (stride 64):
    what it returns is what the same batch returns after a sync."""
    c, svo, _ = free
    h_max = float(c.region[1][1] - 1.0)
    rows = place_entities(c.scene, np.random.default_rng(5), 80, 8, 120, h_max)
    start = hip.entities_from_rows(rows)
    ents = to_device(start.view(np.uint8))
    look = tc.unit([0.3, -0.9, 0.2])
    u = tc.camera_case("heightfield", c.fmt).u  # (shadows on)
    svo.physics_step(ents, DT, 8)
    rgba, hits = svo.trace_rays(u, hip.entity_positions(ents), to_device(look), 40.0, want_hits=True)
    svo.sync()
    stepped = ents.cpu().numpy().view(hip.ENTITY_DTYPE)
    assert (stepped["position"] != start["position"]).any(axis=1).all()  # everybody moved
    after_rgba, after_hits = svo.trace_rays(u, hip.entity_positions(ents), to_device(look), 40.0, want_hits=True)
    svo.sync()
    assert hip.trace_hits_to_numpy(hits).tobytes() == hip.trace_hits_to_numpy(after_hits).tobytes()
    assert rgba.cpu().numpy().tobytes() == after_rgba.cpu().numpy().tobytes()
    exp_rgba, exp_hits = svo.trace_rays(u, hip.entity_positions(stepped), look, 40.0, want_hits=True)  # the host path on the stepped records
    assert exp_hits.tobytes() == hip.trace_hits_to_numpy(hits).tobytes() and exp_rgba.tobytes() == rgba.cpu().numpy().tobytes()
    assert (exp_hits["flags"] & 1).sum() >= 40
    _, before = svo.trace_rays(u, hip.entity_positions(start), look, 40.0, want_hits=True)
    assert before.tobytes() != exp_hits.tobytes()  # (a batch that ran first would say this)


def test_one_batch_through_both_entry_points(free):
    """4h: one vx_ray_batch in device memory -- 65 origins at stride 64 inside entity records, one direction for all, max_dst an array of stride 0
    (one value for all) -- to vx_trace_rays (records only) and to vx_raycast_batch (translucent): both gather it through vx_ray_batch.hpp, so the
    same rays hit, with t, value, face_id and pos bit-equal. 2 blocks along (0.3, -0.9, 0.2) from 0.5 to 3 blocks above the ground: by the oracle
    29 rays hit and 36 end in the air; the last ray, the second wave's only lane, is one that hits."""
    c, svo, _ = free
    rows = place_entities(c.scene, np.random.default_rng(65), 65, 8, 120, float(c.region[1][1] - 1.0))
    rows[[62, 64]] = rows[[64, 62]]  # (62 hits, 64 does not)
    records = hip.entities_from_rows(rows)
    look, reach = tc.unit([0.3, -0.9, 0.2]), 2.0
    by_oracle = np.array([c.scene.intersect(p, look, reach, True)[0].t > 0 for p in np.ascontiguousarray(records["position"])])
    assert by_oracle.sum() >= 10 and (~by_oracle).sum() >= 10 and by_oracle[64]
    ents = to_device(records.view(np.uint8))
    origins, one_dir, one_dst = hip.entity_positions(ents), to_device(look), to_device(np.float32([reach])).expand(65)
    assert hip._ray_vectors("origins", origins, 65, 3)[1] == 64 and hip._ray_vectors("dirs", one_dir, 65, 3)[1] == 0
    assert hip._ray_vectors("max_dst", one_dst, 65, 1) == (one_dst.data_ptr(), 0)
    _, traced = svo.trace_rays(c.u, origins, one_dir, one_dst, want_hits=True, want_rgba=False)
    cast = svo.raycast_batch(origins, one_dir, one_dst, translucent=True)
    svo.sync()
    traced, cast = hip.trace_hits_to_numpy(traced), hip.ray_hits_to_numpy(cast)
    hit = traced["t"] > 0
    assert (hit == (cast["dst"] > 0)).all() and (hit == by_oracle).all()
    assert hit.sum() >= 10 and (~hit).sum() >= 10 and hit[64]
    assert traced["t"][hit].tobytes() == cast["dst"][hit].tobytes() and traced["pos"][hit].tobytes() == cast["pos"][hit].tobytes()
    assert (traced["value"][hit] == cast["value"][hit]).all() and (traced["face_id"][hit] == cast["face_id"][hit]).all()


@pytest.mark.parametrize("fmt", ["esvo", "csvo"])
def test_state(fmt):
    """5: before the first commit VX_ERR_STATE; count = 0 is VX_OK and writes nothing; what a call with a context lacks is refused with the
    field named; after an incremental commit that removes a column of blocks a ray that hit it passes through, by the oracle on the new world."""
    svo_type = tc.SVO[fmt]
    L = hip.lib()
    world, scene_old, tex, mats, h_max = heightfield(svo_type, 7)
    svo = hip.Svo(svo_type, world.size_in_bytes + (1 << 20))
    try:
        svo.set_materials(mats)
        svo.set_textures(tex, 6)
        u = tc.free_uniforms()
        o = np.zeros((8, 3), dtype=np.float32)
        d = np.ascontiguousarray(np.tile(tc.unit([0.05, -1.0, 0.02]), (8, 1)))
        rgba, hits = np.full(8 * 16, 0x5a, dtype=np.uint8), np.full(8 * 48, 0xa5, dtype=np.uint8)
        b = hip.RayBatch(o.ctypes.data, d.ctypes.data, None, 12, 12, 0, -1.0, 0)

        def call(count=8, uniforms=True, rays=True, out_rgba=True, out_hits=True):
            rc = L.vx_trace_rays(svo._h, C.byref(u) if uniforms else None, C.byref(b) if rays else None, count, hip.VX_MEM_HOST,
                                 rgba.ctypes.data_as(_vp) if out_rgba else None, hip.VX_FORMAT_RGBA32F, hits.ctypes.data_as(_vp) if out_hits else None)
            return rc, L.vx_last_error()

        rc, msg = call()
        assert rc == 6 and b"committed" in msg
        svo.update(world)
        for kw, word in ((dict(uniforms=False), b"null uniforms"), (dict(rays=False), b"null rays"), (dict(out_rgba=False, out_hits=False), b"null rgba")):
            rc, msg = call(**kw)
            assert rc == 1 and word in msg, (rc, msg)
        assert call(count=0)[0] == 0 and call(count=0, uniforms=False, rays=False, out_rgba=False, out_hits=False)[0] == 0
        assert (rgba == 0x5a).all() and (hits == 0xa5).all()
        # a chunk column whose ground lies in the lowest chunk (test_raycast_batch.py::test_a_world_change_between_batches): 8 rays down over it
        def ground(x, z):
            r, _, _ = scene_old.intersect(np.float32([x, h_max + 4.0, z]), np.float32([0, -1, 0]), -1.0, False)
            return r.pos[1]

        cx, cz = next((x, z) for x in range(1, 3) for z in range(1, 3) if all(ground(32 * x + fx, 32 * z + fz) < 31.0 for fx in (4, 16, 28) for fz in (4, 16, 28)))
        rng = np.random.default_rng(9)
        o[:, 0], o[:, 1], o[:, 2] = 32 * cx + rng.uniform(3, 29, 8), h_max + 3.0, 32 * cz + rng.uniform(3, 29, 8)
        m = np.full(8, -1.0, dtype=np.float32)
        old_rgba, old_hits = svo.trace_rays(u, o, d, m, want_hits=True)
        chunk = vra.Chunk(cx, 0, cz, 5)
        chunk.set_block(0, 0, 0, 1)  # (not quite empty)
        chunk.compact()
        world.set_chunk((cx, 0, cz), chunk)
        world.serialize()
        svo.update(world)
        new_rgba, new_hits = svo.trace_rays(u, o, d, m, want_hits=True)
        scene_new = orc.OracleScene(svo_type, world.frame(), mats.view(orc.MATERIAL_DTYPE), tex, 6)
        for scene, got_rgba, got_hits in ((scene_old, old_rgba, old_hits), (scene_new, new_rgba, new_hits)):
            for i in range(8):
                r, _, _ = scene.intersect(o[i], d[i], -1.0, True)
                assert got_hits[i]["t"] == np.float32(r.t) and got_hits[i]["value"] == r.value and got_hits[i]["pos"].tobytes() == np.float32(list(r.pos)).tobytes()
                exp = list(r.color) if r.t != -1.0 else tc.sky_color(d[i])[0]
                assert np.abs(got_rgba[i] - exp).max() <= tc.TOL
        assert (old_hits["t"] > 0).all() and ((new_hits["t"] == -1) | (new_hits["t"] > old_hits["t"])).all()  # the rays pass where the ground was
    finally:
        svo.close()
