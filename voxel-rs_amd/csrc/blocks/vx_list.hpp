// The blocks of a box as a compact list, with the faces of each that touch air (vx_list_region; include/voxel_hip.h): the reference's
// get_block (gameplay.rs:161-201) looped over a box and over each block's six neighbours, asked of the world's OWN bytes through
// vx_blocks.hpp's descent. The work is shared out as vx_read_region shares it: a wave owns a brick of 8 x 8 x 8 voxels aligned to the world
// grid, lane l its column (x, y) = (l & 7, l >> 3), eight voxels along z.
//   a column is a mask of 8 bits (bit k: voxel k holds a block). Along z a lane's own mask answers for its neighbours; along x and y the
//   masks of lanes l -+ 1 and l -+ 8 do (the kernel: shuffles; list_region here: array indexing).
//   the brick's six outer faces need the layer of voxels beyond each (the halo): per side one descent to the neighbouring brick
//   (enter_brick_at: wave-uniform), then one voxel a lane through the last three levels -- no load where that brick's descent ended above
//   it or it lies outside the world. The 64 answers of a side are a 64-bit mask every lane holds (the kernel: a ballot), numbered so that
//   the eight bits a bordering column needs are one byte of it (halo_voxel).
//   a brick's records go out slice by slice of z, in lane order inside a slice: dense-index order. Their place in the list is the brick's
//   offset -- an exclusive prefix sum over the bricks' counts -- plus the kept voxels before them in the brick.
// list_region runs the whole call on one thread: count, prefix, write, brick by brick as the kernels run it (the host test harness).
// The reader W is vx_blocks.hpp's. The standard library and voxel_hip.h only -- no HIP header, no HIP call.
#pragma once

#include "vx_blocks.hpp"

namespace vxb {

constexpr uint32_t kListFlags = VX_LIST_FACES | VX_LIST_EXPOSED;  // every known bit
constexpr uint32_t kLanes = kBrick * kBrick;

VXB_FN bool list_wants_faces(uint32_t flags) { return (flags & kListFlags) != 0; }  // (VX_LIST_EXPOSED implies VX_LIST_FACES)

// (wave-uniform) the brick holds no block: outside the world, or its descent ended above it in air -- no load, no halo work
VXB_FN bool brick_is_air(const Brick& b) { return !b.inside || (b.at.done && b.at.value == 0); }

// the brick beyond side f (numbered like face_id) of b
template <int FMT, class W>
VXB_FN Brick enter_neighbour(const W& w, const Brick& b, uint32_t f) {
    const uint32_t d = (f & 1u) ? kBrick : 0u - kBrick;  // (modulo 2^32, like the corners: a brick beyond 0 lies outside the world)
    return enter_brick_at<FMT>(w, b.corner[0] + ((f >> 1) == 0 ? d : 0u), b.corner[1] + ((f >> 1) == 1 ? d : 0u), b.corner[2] + ((f >> 1) == 2 ? d : 0u));
}

// The voxel (0..7 each) of the brick beyond side f that lane l answers for: on the layer that touches b, at (y, z) = (l >> 3, l & 7) beyond
// an x side, (x, z) = (l >> 3, l & 7) beyond a y side, (x, y) = (l & 7, l >> 3) beyond a z side: bit l of the side's mask. So column (i, j)
// finds its eight neighbours beyond -+x in byte j, beyond -+y in byte i, and its one neighbour beyond -+z in bit j * 8 + i, its lane's.
VXB_FN void halo_voxel(uint32_t f, uint32_t lane, uint32_t& x, uint32_t& y, uint32_t& z) {
    const uint32_t a = lane & 7u, c = lane >> 3, layer = (f & 1u) ? 0u : kBrick - 1u, axis = f >> 1;
    x = axis == 0 ? layer : (axis == 1 ? c : a);
    y = axis == 1 ? layer : c;
    z = axis == 2 ? layer : a;
}

// that voxel of the neighbouring brick nb holds a block
template <int FMT, class W>
VXB_FN bool halo_lane(const W& w, const Brick& nb, uint32_t f, uint32_t lane) {
    if (!nb.inside) return false;                  // (wave-uniform, like the next line)
    if (nb.at.done) return nb.at.value != 0;       // air, or a LOD voxel of 8 and more: no load
    uint32_t x, y, z;
    halo_voxel(f, lane, x, y, z);
    Cursor c = nb.at;
    descend<FMT>(w, c, nb.corner[0] + x, nb.corner[1] + y, nb.corner[2] + z, 0);
    return c.value != 0;
}

VXB_FN uint32_t column_mask(const uint32_t value[kBrick]) {
    uint32_t m = 0;
    for (uint32_t k = 0; k < kBrick; ++k) m |= (value[k] != 0 ? 1u : 0u) << k;
    return m;
}

VXB_FN uint32_t mask_byte(uint64_t m, uint32_t n) { return uint32_t(m >> (8u * n)) & 0xffu; }

// open[f], bit k: the neighbour of the column's voxel k on side f holds no block. `col`: the column's own mask; xm, xp, ym, yp: the masks of
// the columns at x - 1, x + 1, y - 1, y + 1 (whatever, where that column lies in another brick); halo[f]: the side's mask.
VXB_FN void column_open(uint32_t i, uint32_t j, uint32_t col, uint32_t xm, uint32_t xp, uint32_t ym, uint32_t yp, const uint64_t halo[6], uint32_t open[6]) {
    open[0] = ~(i > 0 ? xm : mask_byte(halo[0], j)) & 0xffu;
    open[1] = ~(i < kBrick - 1 ? xp : mask_byte(halo[1], j)) & 0xffu;
    open[2] = ~(j > 0 ? ym : mask_byte(halo[2], i)) & 0xffu;
    open[3] = ~(j < kBrick - 1 ? yp : mask_byte(halo[3], i)) & 0xffu;
    const uint32_t lane = j * kBrick + i;
    open[4] = ~((col << 1) | (uint32_t(halo[4] >> lane) & 1u)) & 0xffu;
    open[5] = ~((col >> 1) | ((uint32_t(halo[5] >> lane) & 1u) << 7)) & 0xffu;
}

// bit k: the column's voxel k gives a record -- it holds a block, lies in the box and, under VX_LIST_EXPOSED, has an open face
VXB_FN uint32_t column_keep(const Region& r, const Brick& b, uint32_t i, uint32_t j, uint32_t col, uint32_t flags, const uint32_t open[6]) {
    uint32_t in_box = 0, index;
    for (uint32_t k = 0; k < kBrick; ++k) in_box |= (box_index(r, b, i, j, k, index) ? 1u : 0u) << k;
    const uint32_t any = open[0] | open[1] | open[2] | open[3] | open[4] | open[5];
    return col & in_box & ((flags & VX_LIST_EXPOSED) ? any : 0xffu);
}

// vx_block_at.where of the column's voxel k
VXB_FN uint32_t where_of(uint32_t index, const uint32_t open[6], uint32_t k) {
    uint32_t faces = 0;
    for (uint32_t f = 0; f < 6; ++f) faces |= ((open[f] >> k) & 1u) << f;
    return index | (faces << 24);
}

// What a wave does for its brick, on one thread. write == false: returns the number of records the brick gives. write == true: puts them at
// out[base...], those below `capacity`.
template <int FMT, class W>
inline uint32_t list_brick(const W& w, const Region& r, const Brick& b, uint32_t flags, bool write, uint32_t base, vx_block_at* out, uint32_t capacity) {
    if (brick_is_air(b)) return 0;
    uint32_t value[kLanes][kBrick], col[kLanes], open[kLanes][6], keep[kLanes];
    uint64_t halo[6] = {0, 0, 0, 0, 0, 0};
    if (list_wants_faces(flags))
        for (uint32_t f = 0; f < 6; ++f) {
            const Brick nb = enter_neighbour<FMT>(w, b, f);
            for (uint32_t lane = 0; lane < kLanes; ++lane) halo[f] |= uint64_t(halo_lane<FMT>(w, nb, f, lane) ? 1u : 0u) << lane;
        }
    for (uint32_t lane = 0; lane < kLanes; ++lane) {
        brick_column<FMT>(w, b, lane & 7u, lane >> 3, value[lane]);
        col[lane] = column_mask(value[lane]);
    }
    for (uint32_t lane = 0; lane < kLanes; ++lane) {
        const uint32_t i = lane & 7u, j = lane >> 3;
        for (uint32_t f = 0; f < 6; ++f) open[lane][f] = 0;
        if (list_wants_faces(flags))  // (the kernel's shuffles: lanes l -+ 1, l -+ 8, wrapped where there is none -- never looked at there)
            column_open(i, j, col[lane], col[(lane + kLanes - 1) % kLanes], col[(lane + 1) % kLanes], col[(lane + kLanes - kBrick) % kLanes],
                        col[(lane + kBrick) % kLanes], halo, open[lane]);
        keep[lane] = column_keep(r, b, i, j, col[lane], flags, open[lane]);
    }
    uint32_t n = 0;
    for (uint32_t k = 0; k < kBrick; ++k)
        for (uint32_t lane = 0; lane < kLanes; ++lane) {
            if (!((keep[lane] >> k) & 1u)) continue;
            const uint32_t slot = base + n;
            n += 1;
            if (!write || slot >= capacity) continue;
            uint32_t index;
            box_index(r, b, lane & 7u, lane >> 3, k, index);
            out[slot].where = where_of(index, open[lane], k);
            out[slot].value = value[lane][k];
        }
    return n;
}

// The whole of vx_list_region on one thread, as the three launches run it: counts[brick] = the brick's records; an exclusive prefix sum over
// them in place, counts[bricks] = the total; the records of every brick that has some, from its offset on. `counts`: bricks + 1 dwords.
// Returns the total; min(total, capacity) records are written.
template <int FMT, class W>
inline uint32_t list_region(const W& w, const int32_t lo[3], const uint32_t size[3], uint32_t flags, vx_block_at* out, uint32_t capacity, uint32_t* counts) {
    const Region r = plan_region(lo, size);
    const uint64_t bricks = region_bricks(r);
    for (uint64_t n = 0; n < bricks; ++n) counts[n] = list_brick<FMT>(w, r, enter_brick<FMT>(w, r, uint32_t(n)), flags, false, 0, nullptr, 0);
    uint32_t sum = 0;
    for (uint64_t n = 0; n < bricks; ++n) {
        const uint32_t c = counts[n];
        counts[n] = sum;
        sum += c;
    }
    counts[bricks] = sum;
    for (uint64_t n = 0; n < bricks && capacity; ++n)
        if (counts[n + 1] != counts[n] && counts[n] < capacity) list_brick<FMT>(w, r, enter_brick<FMT>(w, r, uint32_t(n)), flags, true, counts[n], out, capacity);
    return sum;
}

// the rules of the call that need no device: what is wrong, naming the field, or null. (Alignment of device memory: blocks_runtime.cpp.)
inline const char* check_list(const int32_t* lo, const uint32_t* size, uint32_t flags, const void* out, uint32_t capacity, const void* total) {
    if (const char* what = check_region(lo, size)) return what;
    if (flags & ~kListFlags) return "flags holds a bit that is neither VX_LIST_FACES nor VX_LIST_EXPOSED";
    if (!size[0] || !size[1] || !size[2]) return nullptr;  // a box with no voxel: no record, nothing more to refuse
    if (!total) return "null total";
    if (capacity && !out) return "null out with capacity > 0";
    return nullptr;
}

}  // namespace vxb
