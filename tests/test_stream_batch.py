"""The nine entry points that read the world's own bytes on the device -- vx_raycast_batch, vx_trace_rays, vx_trace_views, vx_block_points,
vx_read_region, vx_physics_step, vx_scan_points, vx_scan_columns, vx_list_region -- and vx_render on a STREAMED world (tests/stream_cases.py): a depth-10 scene streamed at radius 22 along a
path of four eyes with vx_commit and dirty ranges, about 66 commits, chunks of LOD 5, 4, 3 and 2, loads, unloads, LOD changes, reuse of freed
ranges and three re-basings. Calls are queued between the commits without a sync and compared at the settled states with the oracle on that
commit's frame (records byte for byte, colours within trace_cases.TOL), with the host harnesses (blocks, scans and lists: at every checkpoint),
and with the dense truth; the streamed
context is compared byte for byte with a context that got the final frame whole; and calls issued during pipelined commits show whole versions.
test_stream_cases_on_host.py proves the inputs and the expectations without a GPU."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import list_cases as lc
import scan_cases as scn
import stream_cases as sc
import trace_cases as tc
from batch_cases import first_difference
from blocks_cases import harness, host_points, host_region
from gpu_harness import to_device
from helpers import vra  # noqa: F401
from physics_cases import DT
from voxel_rs_amd import hip, scenes

pytestmark = pytest.mark.gpu
FMTS = ["esvo", "csvo"]
CAPACITY = 16 << 20
SENTINEL = 0x5A5A5A5A  # what a list's device buffer holds before the call, and beyond the list after it
EVERY = 3  # a checkpoint at every third commit of a move (with the first and the last: 26 over the path's 31 + 17 + 1 + 17 commits)


def make_context(fmt):
    svo = hip.Svo(sc.SVO[fmt], CAPACITY)
    svo.set_materials(scenes.synthetic_materials())  # (as stream_cases.Scene hands them to the oracle)
    svo.set_textures(scenes.synthetic_textures(), 6)
    return svo


class Queued:
    """One checkpoint's device calls: the inputs (kept alive until the sync) and each call's own output tensors."""


def filled(records):
    """A device buffer of `records` vx_block_at records, every byte 0x5a."""
    import torch

    return torch.full((records, 2), SENTINEL, dtype=torch.int32, device="cuda")


def voxels(box):
    return box[1][0] * box[1][1] * box[1][2]


def enqueue(svo, inp, scans=sc.MID_SCANS):
    """The device-memory forms of all nine calls and vx_render, enqueued without a sync. A list's total is not known when it is enqueued: each
    goes into a sentinel-filled buffer of the box's voxel count (at most 64^3 records, 2 MiB) with its own total; one more, cut by a capacity
    of 1,000, into 1,002 records. The last scan reads vx_entity.position in place, behind the physics steps."""
    import torch

    q = Queued()
    q.o, q.d, q.m, q.pts = to_device(inp.o), to_device(inp.d), to_device(inp.m), to_device(inp.pts)
    q.hits = svo.raycast_batch(q.o, q.d, q.m)
    q.rgba, q.trace = svo.trace_rays(inp.free_u, q.o, q.d, q.m, want_hits=True)
    q.imgs, q.view_hits = svo.trace_views(inp.views, sc.W, sc.H, want_hits=True, device=True)
    q.cells = svo.block_points(q.pts)
    q.regions = {name: svo.read_region(lo, size, device=True) for name, (lo, size) in inp.regions.items()}
    q.entities = to_device(hip.entities_from_rows(inp.rows).view(np.uint8))
    q.contacts = svo.physics_step(q.entities, DT, steps=sc.STEPS, want_contacts=True)
    q.frame = torch.empty((sc.H, sc.W, 4), dtype=torch.float32, device="cuda")
    q.frame_hits = torch.empty((sc.H * sc.W, 12), dtype=torch.int32, device="cuda")
    svo.render_device(inp.views[0], sc.W, sc.H, q.frame.data_ptr(), q.frame_hits.data_ptr())
    q.scan_points = {(d, reach): svo.scan_points(q.pts, d, reach=reach) for d, reach in scans}
    q.scan_columns = {key: svo.scan_columns(lo, size, key[1], device=True) for key, (lo, size) in inp.scan_boxes.items()}
    q.lists = {(name, sc.EXPOSED_FACES): svo.list_region(*box, sc.EXPOSED_FACES, out=filled(voxels(box))) for name, box in inp.list_boxes.items()}
    q.lists.update({(name, 0): svo.list_region(*inp.list_boxes[name], 0, out=filled(voxels(inp.list_boxes[name]))) for name in sc.SEAM_BOXES})
    q.lists["cut", sc.EXPOSED_FACES] = svo.list_region(*inp.list_boxes[sc.CUT_BOX], sc.EXPOSED_FACES, capacity=sc.CUT, out=filled(sc.CUT + 2))
    q.entity_scan = svo.scan_points(hip.entity_positions(q.entities), hip.VX_DIR_NEG_Y)
    return q


def fetch(q):
    """A synchronised checkpoint's outputs as NumPy arrays, named as in compare()."""
    return dict(hits=hip.ray_hits_to_numpy(q.hits), trace=hip.trace_hits_to_numpy(q.trace), rgba=q.rgba.cpu().numpy(),
                view_hits=hip.trace_hits_to_numpy(q.view_hits).reshape(2, -1), imgs=q.imgs.cpu().numpy(), cells=hip.block_cells_to_numpy(q.cells),
                regions={name: t.cpu().numpy().view(np.uint32) for name, t in q.regions.items()},
                entities=q.entities.cpu().numpy().view(hip.ENTITY_DTYPE), contacts=q.contacts.cpu().numpy(),
                frame=q.frame.cpu().numpy(), frame_hits=hip.trace_hits_to_numpy(q.frame_hits),
                scan_points={key: hip.scan_hits_to_numpy(t) for key, t in q.scan_points.items()},
                scan_columns={key: hip.scan_hits_to_numpy(t) for key, t in q.scan_columns.items()},
                lists={key: hip.block_ats_to_numpy(records) for key, (records, _) in q.lists.items()},
                list_totals={key: total.cpu().numpy().view(np.uint32) for key, (_, total) in q.lists.items()},
                entity_scan=hip.scan_hits_to_numpy(q.entity_scan))


def on_host(svo, inp):
    """The host-memory forms of every call, and vx_render into host memory: the same dictionary."""
    o, d, m = (np.array(a, order="C") for a in (inp.o, inp.d, inp.m))
    rgba, trace = svo.trace_rays(inp.free_u, o, d, m, want_hits=True)
    imgs, view_hits = svo.trace_views(inp.views, sc.W, sc.H, want_hits=True)
    e = hip.entities_from_rows(inp.rows)
    contacts = svo.physics_step(e, DT, steps=sc.STEPS, want_contacts=True)
    frame, frame_hits = svo.render(inp.views[0], sc.W, sc.H, want_hits=True)
    pts = np.array(inp.pts, order="C")
    lists = {(name, flags): svo.list_region(*box, flags) for name, box in inp.list_boxes.items() for flags in lc.FLAG_SETS}
    lists["cut", sc.EXPOSED_FACES] = svo.list_region(*inp.list_boxes[sc.CUT_BOX], sc.EXPOSED_FACES, capacity=sc.CUT)
    return dict(hits=svo.raycast_batch(o, d, m), trace=trace, rgba=rgba, view_hits=view_hits, imgs=imgs, cells=svo.block_points(np.array(inp.pts, order="C")),
                regions={name: svo.read_region(lo, size) for name, (lo, size) in inp.regions.items()}, entities=e,
                contacts=contacts.view(np.float32).reshape(-1, 6), frame=frame, frame_hits=frame_hits.reshape(-1),
                scan_points={(d, reach): svo.scan_points(pts, d, reach=reach) for d, reach in sc.SETTLED_SCANS},
                scan_columns={key: svo.scan_columns(lo, size, key[1]) for key, (lo, size) in inp.scan_boxes.items()},
                lists={key: records for key, (records, _) in lists.items()}, list_totals={key: np.uint32([total]) for key, (_, total) in lists.items()},
                entity_scan=svo.scan_points(hip.entity_positions(e), hip.VX_DIR_NEG_Y))


def compare(got, exp, inp, what):
    """Against the oracle on the checkpoint's frame: ray hits, vx_hit records, entities and contacts byte for byte, colours within TOL."""
    first_difference(got["hits"], exp.hits, what + " raycast_batch", lambda i: f"ray {i} ({inp.kinds[i]}): origin {inp.o[i]!r} dir {inp.d[i]!r} max_dst {inp.m[i]!r}")
    tc.assert_records(got["trace"], exp.trace, what + " trace_rays")
    tc.assert_colors(got["rgba"], exp.color, what + " trace_rays")
    for k in range(len(exp.view_hits)):
        tc.assert_records(got["view_hits"][k], exp.view_hits[k].reshape(-1), f"{what} trace_views view {k}")
        tc.assert_colors(got["imgs"][k], exp.imgs[k], f"{what} trace_views view {k}")
    tc.assert_records(got["frame_hits"], exp.view_hits[0].reshape(-1), what + " render")
    tc.assert_colors(got["frame"], exp.imgs[0], what + " render")
    describe = lambda i: f"entity {i} ({next(r for r, idx in inp.roles.items() if i in idx)}): start {inp.rows[i]!r}"  # noqa: E731
    first_difference(hip.entities_to_rows(got["entities"]), exp.run[-1][0], f"{what} entities after {sc.STEPS} steps", describe)
    first_difference(np.asarray(got["contacts"], dtype=np.float32).reshape(-1, 6), exp.run[-1][1], f"{what} contacts", describe)


def compare_blocks(got, cells, regions, what):
    """vx_block_cell records and regions byte for byte against the host harness's on the same frame."""
    assert got["cells"].tobytes() == cells.tobytes(), f"{what} block_points: {(got['cells'].view(np.uint64) != cells.view(np.uint64)).sum()} records differ from the host harness's"
    for name, exp in regions.items():
        g = got["regions"][name]
        assert g.shape == exp.shape and (g == exp).all(), (what, "read_region", name, np.argwhere(g != exp)[:8])


def compare_lists(got, lists, what):
    """Every list of `got` against the whole list of its box and flags: the total is the list's length whatever the capacity, the records up
    to min(total, capacity) are exact, and what lies beyond them -- in a device buffer -- still holds the sentinel."""
    for (name, flags), records in got["lists"].items():
        exp = lists[(sc.CUT_BOX if name == "cut" else name), flags]
        total = int(got["list_totals"][name, flags][0])
        n = min(len(exp), sc.CUT) if name == "cut" else len(exp)
        assert total == len(exp), f"{what} list_region {name} flags {flags}: total {total}, expected {len(exp)}"
        assert lc.differing(records[:n], exp[:n]) is None, f"{what} list_region {name} flags {flags}: {lc.differing(records[:n], exp[:n])}"
        assert (records[n:].view(np.uint32) == SENTINEL).all(), f"{what} list_region {name} flags {flags}: written beyond its {n} records"


def compare_scans(got, points, columns, entity_scan, what):
    for (d, reach), records in got["scan_points"].items():
        assert scn.differing(records, points[d, reach]) is None, f"{what} scan_points {scn.DIR_NAMES[d]} reach {reach}: {scn.differing(records, points[d, reach])}"
    for (name, d), records in got["scan_columns"].items():
        assert scn.differing(records, columns[name, d]) is None, f"{what} scan_columns {name} {scn.DIR_NAMES[d]}: {scn.differing(records, columns[name, d])}"
    assert scn.differing(got["entity_scan"], entity_scan) is None, f"{what} scan_points under vx_entity.position: {scn.differing(got['entity_scan'], entity_scan)}"


def compare_harness(got, said, what):
    """The blocks, the scans and the lists byte for byte against the host harnesses' on the same frame."""
    compare_blocks(got, said.cells, said.regions, what)
    compare_scans(got, said.points, said.columns, said.entity_scan, what)
    compare_lists(got, said.lists, what)


def harness_blocks(exe, scene, inp):
    cells = host_points(exe, scene, inp.pts, 12, len(inp.pts))
    regions = {name: (host_region(exe, scene, lo, size) if 0 not in size else np.zeros((size[2], size[1], size[0]), dtype=np.uint32)) for name, (lo, size) in inp.regions.items()}
    return cells, regions


def final_positions(exp):
    """Where the oracle's run leaves the entities: what the scan behind vx_physics_step reads in place."""
    return np.ascontiguousarray(exp.run[-1][0][:, 0:3], dtype=np.float32)


class Said:
    """What the host harnesses say of one checkpoint's frame."""


def harnesses():
    return harness(), scn.harness(), lc.harness()


def harness_says(exes, scene, inp, exp, settled):
    """The three harnesses on one frame: points and regions; the scans of the point set (in mid-stream the two of sc.MID_SCANS, settled all
    eighteen), of every scan box and of the entities' final positions; the lists (in mid-stream those the device is asked for, settled every
    box under every flag set: the host-memory forms)."""
    said = Said()
    said.cells, said.regions = harness_blocks(exes[0], scene, inp)
    case = sc.Case(scene)
    scans, lists = scn.HostScans(exes[1], case), lc.HostLists(exes[2], case)
    try:
        said.points = {(d, reach): scans.points(inp.pts, d, reach) for d, reach in (sc.SETTLED_SCANS if settled else sc.MID_SCANS)}
        said.columns = {key: scans.columns(lo, size, key[1]) for key, (lo, size) in inp.scan_boxes.items()}
        said.entity_scan = scans.points(final_positions(exp), hip.VX_DIR_NEG_Y, scn.TO_EDGE)
        keys = [(name, flags) for name in sc.LIST_BOXES for flags in lc.FLAG_SETS if settled or flags == sc.EXPOSED_FACES or (flags == 0 and name in sc.SEAM_BOXES)]
        said.lists = {}
        for name, flags in keys:  # (one run: a buffer of the box's voxel count holds any list of it)
            records, total, _ = lists.buffer(*inp.list_boxes[name], flags, voxels(inp.list_boxes[name]))
            said.lists[name, flags] = records[:total].copy()
    finally:
        scans.close()
        lists.close()
    return said


def expectations(fmt, words, inp, state, exes, settled):
    """(the oracle's answers, the host harnesses' blocks, scans and lists) for one checkpoint's frame; a frame that is the dry run's settled
    one, byte for byte, has the dry run's answers."""
    scene = sc.Scene(fmt, words)
    exp = state.expected if words.tobytes() == state.scene.words.tobytes() else sc.expected(scene, inp)
    return exp, harness_says(exes, scene, inp, exp, settled)


def compare_truth(got, inp, what):
    """Settled: the points and the regions against the dense truth."""
    t, lod = sc.truth(inp.centre)
    sc.check_cells(t, lod, inp.off, inp.pts, got["cells"], what)
    for name, (lo, size) in inp.regions.items():
        exp = sc.dense_region(t, inp.off, lo, size)
        g = got["regions"][name]
        assert g.shape == exp.shape and (g == exp).all(), (what, "read_region against the truth", name, np.argwhere(g != exp)[:8])


def compare_block_truth(got, state, exp, what):
    """Settled: the scans and the lists against scan_cases' and list_cases' numpy truths over the dense arrays."""
    b = state.blocks
    final = final_positions(exp)
    compare_scans(got, b.points, b.columns, scn.points_truth(state.case, final, hip.VX_DIR_NEG_Y, scn.TO_EDGE), what + " against the truth")
    compare_lists(got, b.lists, what + " against the truth")


def stream_move(s, svo, eye, totals):
    """One move of the path, pump by pump: yields (commit index within the move, the pump's stats)."""
    s.move_to(*eye)
    k = 0
    while True:
        st = s.pump(svo._h, 400)
        for name in ("loads", "unloads", "lod_changes", "ranges", "bytes"):
            totals[name] += st[name]
        totals["commits"] += 1
        yield k, st
        if st["pending"] == 0:
            return
        k += 1


@pytest.mark.parametrize("fmt", FMTS)
def test_every_entry_point_between_ranged_commits(fmt):
    """3a. Checkpoints at the first commit after each move_to, at every third commit in mid-stream and at every settled state: the oracle scene
    is built from s.frame() as of that commit and all nine calls and vx_render are enqueued in their device-memory forms (the scans of every
    scan box, the lists of every list box with faces, the plain lists of the two seam boxes, one list cut by its capacity, a scan under the
    entities the physics steps have just moved), each with its own outputs, without a sync -- the next vx_commit has to wait for these reads, and these reads for the upload before. vx_sync only at the
    settled states; then everything queued since the last one is compared: with the oracle, and the blocks, scans and lists with the host
    harnesses on that commit's frame. At the settled states also with the dense truth, and the host-memory forms (every flag set, all six
    directions at three reaches).
    (Every third commit, not every sixth: the path has about 66 commits, and at least 20 checkpoints are asked for.)"""
    states = sc.dry_run(fmt)
    exes = harnesses()
    s = sc.new_streamer(fmt)
    svo = make_context(fmt)
    totals = dict(loads=0, unloads=0, lod_changes=0, ranges=0, bytes=0, commits=0)
    checkpoints = 0
    try:
        for x in states:
            inp = x.inputs
            pending = []  # (what, queued calls, the commit's frame, settled)
            for k, st in stream_move(s, svo, x.eye, totals):
                settled = st["pending"] == 0
                if not (k % EVERY == 0 or settled):
                    continue
                assert (sc.svo_offset(s) == inp.off).all()
                what = f"{fmt} move {x.index} commit {k}" + (" (settled)" if settled else "")
                pending.append((what, enqueue(svo, inp, sc.SETTLED_SCANS if settled else sc.MID_SCANS), s.frame(pad_words=0), settled))
                checkpoints += 1
            # what the oracle and the host harnesses say of each checkpoint's frame, while the device works (the oracle's calls run side by side)
            with ThreadPoolExecutor(max_workers=8) as pool:
                said = list(pool.map(lambda p: expectations(fmt, p[2], inp, x, exes, p[3]), pending))
            svo.sync()
            assert s.resident_chunks == x.resident and st["arena_bytes"] == x.arena_bytes
            for (what, q, _, _), (exp, harness_said) in zip(pending, said):
                got = fetch(q)
                compare(got, exp, inp, what)
                compare_harness(got, harness_said, what)
            compare_truth(got, inp, what)  # (the last one: the settled state)
            compare_block_truth(got, x, exp, what)
            host = on_host(svo, inp)
            compare(host, exp, inp, what + " host memory")
            compare_harness(host, harness_said, what + " host memory")
            compare_truth(host, inp, what + " host memory")
            compare_block_truth(host, x, exp, what + " host memory")
        print(f"\n{fmt}: {checkpoints} checkpoints, {totals}, arena {st['arena_bytes']} bytes")
        assert totals["loads"] >= 10000 and totals["unloads"] >= 2000 and totals["lod_changes"] >= 5000 and checkpoints >= 20
    finally:
        svo.close()


@pytest.mark.parametrize("fmt", FMTS)
def test_a_streamed_world_answers_like_a_full_upload(fmt):
    """3b. After the whole path -- about 66 ranged commits, reuse of freed ranges, three re-basings -- a second context is given s.frame()
    whole; every device-memory call on both contexts gives the same bytes, pixels included: the same kernels on what must be the same bytes."""
    states = sc.dry_run(fmt)
    s = sc.new_streamer(fmt)
    svo, whole = make_context(fmt), make_context(fmt)
    totals = dict(loads=0, unloads=0, lod_changes=0, ranges=0, bytes=0, commits=0)
    try:
        for x in states:
            for _ in stream_move(s, svo, x.eye, totals):
                pass
        assert totals["commits"] >= 50 and totals["ranges"] >= 300
        frame = s.frame(pad_words=0)
        whole.upload_frame(frame, sc.SVO_DEPTH)
        assert svo.get_stats()["depth"] == whole.get_stats()["depth"] == sc.SVO_DEPTH
        inp = states[-1].inputs
        a, b = enqueue(svo, inp, sc.SETTLED_SCANS), enqueue(whole, inp, sc.SETTLED_SCANS)
        svo.sync()
        whole.sync()
        a, b = fetch(a), fetch(b)
        for name in a:
            if name in ("frame", "frame_hits"):  # (vx_render walks the traversal image, which the two contexts built differently: held to the oracle in 3a)
                continue
            if isinstance(a[name], dict):  # regions, scans, lists (the whole buffers: the sentinel beyond a list too) and their totals
                assert a[name].keys() == b[name].keys()
                for r in a[name]:
                    assert a[name][r].tobytes() == b[name][r].tobytes(), (fmt, name, r)
            else:
                assert a[name].tobytes() == b[name].tobytes(), (fmt, name)
        compare_truth(a, inp, f"{fmt} streamed")
        compare_block_truth(a, states[-1], states[-1].expected, f"{fmt} streamed")
        print(f"\n{fmt}: {totals}")
    finally:
        svo.close()
        whole.close()


@pytest.mark.parametrize("fmt", FMTS)
def test_pipelined_commits_show_whole_versions_to_batch_calls(fmt):
    """3c. The first move inline, the second with VX_COMMIT_PIPELINED: per pump, vx_raycast_batch, vx_block_points, vx_read_region,
    vx_scan_columns and vx_list_region (the second state's rays and points and its box over the LOD 5 / LOD 4 boundary: where the move loads
    chunks and changes their LOD; the heightmap over that box and its list with faces) are enqueued at once behind the posted commit and again
    after vx_commit_wait. Each output of the first set is, as a whole, the old version's or the new one's -- a list with its total, its
    records and the sentinel beyond them as one: a count from one version with records from another is neither -- and once a call has shown
    the new one, so do the calls issued after it; the second set is the new version's."""
    states = sc.dry_run(fmt)
    exe, scan_exe, list_exe = harnesses()
    s = sc.new_streamer(fmt)
    svo = make_context(fmt)
    totals = dict(loads=0, unloads=0, lod_changes=0, ranges=0, bytes=0, commits=0)
    inp = states[1].inputs
    n, boxes = 256, [inp.regions["lod5_lod4"], inp.regions["lod4_lod3"]]
    names = ("raycast_batch", "block_points", "read_region", "read_region (the second box)", "scan_columns", "list_region")
    heightmap, listed = inp.scan_boxes["lod5_lod4", hip.VX_DIR_NEG_Y], inp.list_boxes["lod5_lod4"]
    o, d, m, pts = to_device(inp.o[:n]), to_device(inp.d[:n]), to_device(inp.m[:n]), to_device(inp.pts)

    def calls():
        return (svo.raycast_batch(o, d, m), svo.block_points(pts)) + tuple(svo.read_region(*box, device=True) for box in boxes) + (
            svo.scan_columns(*heightmap, hip.VX_DIR_NEG_Y, device=True), svo.list_region(*listed, sc.EXPOSED_FACES, out=filled(voxels(listed))))

    def whole_list(total, records):
        """A list as one array of words: its total, then the buffer -- the records and the sentinel beyond them."""
        return np.concatenate([np.uint32([total]), records.view(np.uint32)])

    def version():
        """What the calls have to give on the world as the streamer holds it now."""
        scene = sc.Scene(fmt, s.frame(pad_words=0))
        case = sc.Case(scene)
        scans, lists = scn.HostScans(scan_exe, case), lc.HostLists(list_exe, case)
        try:
            columns = scans.columns(*heightmap, hip.VX_DIR_NEG_Y)
            records, total, _ = lists.buffer(*listed, sc.EXPOSED_FACES, voxels(listed))  # (the harness fills its buffer with the same 0x5a)
        finally:
            scans.close()
            lists.close()
        assert (records[total:].view(np.uint32) == SENTINEL).all()
        return (sc.oracle_hits(scene.oracle, inp.o[:n], inp.d[:n], inp.m[:n], False), host_points(exe, scene, inp.pts, 12, len(inp.pts))) + tuple(
            host_region(exe, scene, *box) for box in boxes) + (columns, whole_list(total, records))

    def as_numpy(got):
        return (hip.ray_hits_to_numpy(got[0]), hip.block_cells_to_numpy(got[1])) + tuple(t.cpu().numpy().view(np.uint32) for t in got[2:4]) + (
            hip.scan_hits_to_numpy(got[4]), whole_list(int(got[5][1].cpu().numpy().view(np.uint32)[0]), hip.block_ats_to_numpy(got[5][0])))

    try:
        for _ in stream_move(s, svo, states[0].eye, totals):
            pass
        svo.sync()
        svo.set_commit_mode(True)
        s.move_to(*states[1].eye)
        old = version()
        differ = saw_old = pumps = 0
        while True:
            st = s.pump(svo._h, 400)  # posts the job
            first = calls()
            svo.commit_wait()
            second = calls()
            svo.sync()
            new = version()
            pumps += 1
            changed = [a.tobytes() != b.tobytes() for a, b in zip(old, new)]
            differ += any(changed)
            shown = []
            for name, got, a, b, ch in zip(names, as_numpy(first), old, new, changed):
                is_old, is_new = got.tobytes() == a.tobytes(), got.tobytes() == b.tobytes()
                assert is_old or is_new, f"{fmt} pump {pumps}: {name} issued behind a posted commit shows neither the old version nor the new one"
                if ch:
                    shown.append(is_new)
            assert shown == sorted(shown), f"{fmt} pump {pumps}: a call showed the old version after an earlier one had shown the new one: {shown}"
            saw_old += bool(shown) and not shown[0]
            for name, got, b in zip(names, as_numpy(second), new):
                assert got.tobytes() == b.tobytes(), f"{fmt} pump {pumps}: {name} after vx_commit_wait does not show the new version"
            old = new
            if st["pending"] == 0:
                break
        print(f"\n{fmt}: {pumps} pipelined pumps, old and new differ in {differ}, the first call still showed the old version in {saw_old}")
        assert differ >= 5
        svo.set_commit_mode(False)
        s.move_to(*states[2].eye)
        st = s.pump(svo._h, 400)  # inline again: the move in y alone, which re-bases every leaf
        assert st["pending"] == 0
        inp2 = states[2].inputs
        o, d, m, pts = to_device(inp2.o), to_device(inp2.d), to_device(inp2.m), to_device(inp2.pts)  # (alive until the sync)
        got = svo.raycast_batch(o, d, m), svo.block_points(pts), svo.read_region(*inp2.regions["lod5_lod4"], device=True)
        svo.sync()
        hits, cells, region = hip.ray_hits_to_numpy(got[0]), hip.block_cells_to_numpy(got[1]), got[2].cpu().numpy().view(np.uint32)
        scene = sc.Scene(fmt, s.frame(pad_words=0))
        assert hits.tobytes() == sc.oracle_hits(scene.oracle, inp2.o, inp2.d, inp2.m, False).tobytes()
        t, lod = sc.truth(inp2.centre)
        sc.check_cells(t, lod, inp2.off, inp2.pts, cells, f"{fmt} inline again")
        assert (region == sc.dense_region(t, inp2.off, *inp2.regions["lod5_lod4"])).all()
    finally:
        svo.close()


def test_view_tables_outlive_the_context_that_used_them():
    """vx_trace_views into device memory keeps its tables in a ring per device, each slot guarded by an event. That event used to be recorded on
    the calling context's stream, and a context that is destroyed takes its stream with it: the next context's call failed in
    hipEventSynchronize (found by the tests above, in the second format's first checkpoint). Four calls fill the ring, the context goes, another
    context makes four more."""
    x = sc.dry_run("esvo")[0]
    rendered = None
    for _ in range(2):
        svo = make_context("esvo")
        try:
            svo.upload_frame(x.scene.words, sc.SVO_DEPTH)
            out = [svo.trace_views(x.inputs.views, sc.W, sc.H, want_hits=True, device=True) for _ in range(4)]
            svo.sync()
            rendered = [hip.trace_hits_to_numpy(h).reshape(2, -1) for _, h in out]
        finally:
            svo.close()
        for got in rendered:
            for k in range(2):
                tc.assert_records(got[k], x.expected.view_hits[k].reshape(-1), f"view {k}")
