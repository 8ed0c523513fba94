"""Shared by the tests of vx_list_region (test_list_abi.py, test_list_on_host.py, test_list.py): scan_cases.py's three worlds in both formats,
the boxes, and the expected list of each box -- plain numpy over the dense truth: blocks_cases.dense_region of the box padded by one voxel,
the face bits from its six shifted views, the records sorted by (z >> 3, y >> 3, x >> 3, z, y, x). Nothing of the code under test is used.
Also the runner of the host harness (tests/cpp/list_on_host.cpp), a stand-alone program."""

import numpy as np

from blocks_cases import REGIONS, dense_region
from host_harness import HostRunner, build_harness
from scan_cases import SCAN_CASES, make_scan_case  # noqa: F401  (the tests' parameters)
from voxel_rs_amd import hip

FACES, EXPOSED = hip.VX_LIST_FACES, hip.VX_LIST_EXPOSED
FLAG_SETS = (0, FACES, EXPOSED | FACES)
MAIN_BOXES = {"glasshouse": REGIONS["glasshouse"], "far_chunks": REGIONS["far_chunks"], "tower": ((-3, -3, -3), (134, 134, 134))}
# in the terrain, on the brick grid (far_chunks: where all four chunks meet, the LOD chunk among them; tower: in the LOD-5 chunk)
ANCHOR = {"glasshouse": (16, 0, 16), "far_chunks": (12832, 96, 12864), "tower": (8, 0, 8)}
# strictly inside solid ground and walls: the voxels beyond the box's sides hold blocks
INNER = {"glasshouse": ((5, 0, 9), (11, 6, 4)), "far_chunks": ((12813, 97, 12843), (11, 7, 7)), "tower": ((10, 1, 11), (11, 6, 7))}


# ---- the truth: plain numpy over the dense arrays ----------------------------------------------------------------------------------------------


def expected_parts(c, lo, size, flags):
    """(world x, y, z, index, faces, value) of the box's records under `flags`, in the list's order."""
    lo, size = [int(v) for v in lo], [int(v) for v in size]
    if not all(size):
        return tuple(np.zeros(0, dtype=np.int64) for _ in range(6))
    pad = dense_region(c.info, c.truth, [v - 1 for v in lo], [v + 2 for v in size])  # [z][y][x], a voxel more on every side
    air = pad == 0
    core = pad[1:-1, 1:-1, 1:-1]
    m = slice(1, -1)
    shifted = (air[m, m, :-2], air[m, m, 2:], air[m, :-2, m], air[m, 2:, m], air[:-2, m, m], air[2:, m, m])  # -x, +x, -y, +y, -z, +z
    faces = np.zeros(core.shape, dtype=np.int64)
    if flags:
        for f, open_side in enumerate(shifted):
            faces |= open_side.astype(np.int64) << f
    keep = core != 0
    if flags & EXPOSED:
        keep &= faces != 0
    z, y, x = np.nonzero(keep)
    index = (z * size[1] + y) * size[0] + x
    wx, wy, wz = x + lo[0], y + lo[1], z + lo[2]
    order = np.lexsort((wx, wy, wz, wx >> 3, wy >> 3, wz >> 3))  # (the last key is the first; >> floors)
    return tuple(a[order] for a in (wx, wy, wz, index, faces[keep], core[keep].astype(np.int64)))


def records_of(index, faces, value):
    r = np.zeros(len(index), dtype=hip.BLOCK_AT_DTYPE)
    r["where"] = index | (faces << 24)
    r["value"] = value
    return r


def expected_list(c, lo, size, flags):
    """The box's BLOCK_AT_DTYPE records under `flags`."""
    return records_of(*expected_parts(c, lo, size, flags)[3:])


def rebased(records, lo, size, whole_lo, whole_size):
    """A part's records with `where` re-based to the whole box, and their world coordinates: (records, x, y, z)."""
    index, faces = hip.split_where(records["where"].astype(np.int64))
    x, y, z = index % size[0] + lo[0], index // size[0] % size[1] + lo[1], index // (size[0] * size[1]) + lo[2]
    whole = ((z - whole_lo[2]) * whole_size[1] + (y - whole_lo[1])) * whole_size[0] + (x - whole_lo[0])
    return records_of(whole, faces, records["value"]), x, y, z


def merged(parts):
    """[(records, x, y, z)] of the boxes that tile a larger one, as one list in the list's order."""
    r, x, y, z = (np.concatenate(a) for a in zip(*parts))
    return r[np.lexsort((x, y, z, x >> 3, y >> 3, z >> 3))]


# ---- boxes -------------------------------------------------------------------------------------------------------------------------------


def boxes_for(c):
    """[(name, lo, size)]: the main box first, then the small ones, each named for what it catches."""
    lo_all, size = c.info["lo"], c.size
    solid = np.argwhere(c.truth != 0)[0] + lo_all
    g = ANCHOR[c.name]

    def box(name, blo, bsize):
        return name, tuple(int(v) for v in blo), tuple(int(v) for v in bsize)

    out = [box("main", *MAIN_BOXES[c.name]),
           box("one_voxel", solid, (1, 1, 1)),                                               # a wave with one kept voxel
           box("9x1x1", (int(solid[0]) // 8 * 8 - 4, solid[1], solid[2]), (9, 1, 1)),         # two bricks, one row
           box("outside", (size, 0, 8), (5, 4, 3)),                                           # no brick inside the world: total 0
           box("outside_negative", (-40, -9, 3), (8, 9, 3))]
    out += [box(f"grid{s}", [v - 8 * (s // 16) for v in g], (s, s, s)) for s in (8, 16, 24)]  # whole bricks: 1, 8 and 27 of them
    out.append(box("off_grid", (g[0] + 1, g[1] - 7, g[2] + 1), (23, 18, 9)))                  # one voxel off the grid: every brick cut by the box
    out.append(box("world_edge", (-2, -2, -2), (12, 12, 12)))                                 # neighbours outside the world are air
    out.append(box("inner", *INNER[c.name]))                                                  # neighbours outside the box, inside a chunk
    if c.name == "tower":
        out.append(box("lod_seam", (0, 0, 24), (32, 24, 16)))   # z = 32: LOD 5 below, LOD 2 above -- bricks filled by one leaf of side 8, a halo from another chunk
        out.append(box("lod1_chunk", (62, 94, 30), (36, 36, 36)))  # ESVO: leaves of side 16 (two bricks wide), against the world's edge at y = 128
    return out


def split_at(lo, size, axis, cut):
    """The two boxes the plane `cut` (a world coordinate of `axis`) splits the box into."""
    a_size, b_lo, b_size = list(size), list(lo), list(size)
    a_size[axis] = cut - lo[axis]
    b_lo[axis], b_size[axis] = cut, size[axis] - a_size[axis]
    return (tuple(lo), tuple(a_size)), (tuple(b_lo), tuple(b_size))


# ---- the host harness: a stand-alone program -----------------------------------------------------------------------------------------


def harness():
    """tests/_build/list_on_host: host_harness.build_harness's."""
    return build_harness("list_on_host")


class HostLists(HostRunner):
    """The harness on one world: the frame is written once, every call is a run of the program."""

    def buffer(self, lo, size, flags, capacity):
        """(the `capacity` records of a buffer that held 0x5a bytes before the call, total, bricks)"""
        self.run("list", *lo, *size, flags, capacity, self.path("out.bin"))
        raw = self.get("out.bin", np.uint32)
        assert len(raw) == 2 + 2 * capacity
        return raw[2:].view(hip.BLOCK_AT_DTYPE), int(raw[0]), int(raw[1])

    def list(self, lo, size, flags):
        """(the box's whole list, total): counted first, then written into exactly that many records."""
        _, total, _ = self.buffer(lo, size, flags, 0)
        records, again, _ = self.buffer(lo, size, flags, total)
        assert again == total
        return records, total


def differing(got, exp):
    """A message naming the first differing record of two BLOCK_AT_DTYPE arrays, or None."""
    if got.shape != exp.shape:
        return f"lengths differ: {got.shape} vs {exp.shape}"
    if got.tobytes() == exp.tobytes():
        return None
    bad = np.flatnonzero(got.view(np.uint64) != exp.view(np.uint64))
    i = int(bad[0])
    gi, gf = hip.split_where(int(got["where"][i]))
    ei, ef = hip.split_where(int(exp["where"][i]))
    return f"{len(bad)} records differ, first at {i}: got index {gi} faces {gf:06b} value {got['value'][i]}, expected index {ei} faces {ef:06b} value {exp['value'][i]}"
