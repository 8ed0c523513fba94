// vx_move_boxes' kernel (gfx950): vx_move.hpp's answer for a batch of float boxes and their motions, the world's own bytes read as
// kernels_boxes.hip reads them (vx_world_bytes.hpp: a read beyond the world gives 0). The world is read-only for the launch. No LDS, no
// atomic, no memory between bricks; no kernel waits for another workgroup. The launch shape is kernels_boxes.hip's.
//   a workgroup (one wave) owns one box, blockIdx.x its number.
//   1  every lane reads the box's nine floats and the motion's three through the strides at the same address (scalar loads in the code) and
//      works out validity, mn, mx and the displacement -- in VGPRs, one copy a lane (in_vgpr). No box or no motion: lane 0 writes the
//      record, the wave leaves with no load from the world.
//   2  three passes in the order's sequence; the axis of a pass and its direction are scalars. d == 0: no scan. Else the slab --
//      cross-section times the layers ahead -- as a cover in VGPRs, for the lanes' own tests; its three brick counts go through
//      readfirstlane in one register, and so does the corner of each brick: the loops over brick layers and bricks and enter_brick_at's
//      descent run on scalar registers and wave-uniform addresses.
//   3  the slab's bricks, nearest brick layer first: a brick of air, or one leaf above the brick that only_value refuses, is skipped by a
//      scalar branch; else lane l takes column (l & 7, l >> 3) with vxb::move_brick_lane (lanes outside the slab load nothing) and keeps
//      one key with its value. After each brick layer a ballot ends the walk if any lane holds a key.
//   4  one min-fold of (key, value) by 6 x 2 xor-shuffles a pass (fold_wave, kernels_shared.hpp), which leaves the smallest in every lane,
//      then the pass's float operations, the same in every lane. The file is built with -ffp-contract=off like every other: no multiply of
//      the rule is fused into the add behind it.
//   5  lane 0 writes the record as three 16-byte stores (store_record).
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, ESVO / CSVO / ESVO beyond 4 GiB): 109 / 120 / 106 VGPRs, 90 / 104 / 94 SGPRs. No
// spill, no scratch, no LDS in any of the three. (With the box's floats and the slab's brick range left to the compiler -- in scalar registers
// -- the three builds spilled 12 to 27 SGPRs.)
#include <hip/hip_runtime.h>

#include "kernels_blocks.h"
#include "kernels_shared.hpp"
#include "vx_device.hpp"
#include "vx_world_bytes.hpp"

using namespace vxd;
using namespace vxk;

namespace {

// The box's floats live in VGPRs, one copy a lane: loaded at a uniform address they would all be kept in scalar registers, with the
// descent's cursor, the slab and the loop counters more than there are. (No instruction: the constraint alone places the value.)
__device__ __forceinline__ float in_vgpr(float v) {
    asm volatile("" : "+v"(v));
    return v;
}

__device__ __forceinline__ void load3_in_vgpr(const uint8_t* base, size_t at, float out[3]) {
    load3_at(base, at, out);
    out[0] = in_vgpr(out[0]), out[1] = in_vgpr(out[1]), out[2] = in_vgpr(out[2]);
}

// (each pointer a kernel argument of its own, as in kernels_boxes.hip: the loads address global memory; has_offset, the strides, the order
// and only_value are kernel arguments: wave-uniform branches)
template <int SVO>
__global__ __launch_bounds__(64) void move_boxes_kernel(SceneArgs sa, const uint8_t* __restrict__ origin, const uint8_t* __restrict__ offset,
                                                        const uint8_t* __restrict__ extents, const uint8_t* __restrict__ motion, uint32_t origin_stride,
                                                        uint32_t offset_stride, uint32_t extents_stride, uint32_t motion_stride, uint32_t has_offset,
                                                        uint32_t only_value, float scale, float skin, uint32_t order, vx_move_hit* __restrict__ out) {
    const WorldBytes<SVO> w = {make_scene(sa)};
    const uint32_t n = blockIdx.x, lane = threadIdx.x;
    float o[3], f[3] = {0.0f, 0.0f, 0.0f}, e[3], mot[3];
    load3_in_vgpr(origin, size_t(n) * origin_stride, o);
    if (has_offset) load3_in_vgpr(offset, size_t(n) * offset_stride, f);
    load3_in_vgpr(extents, size_t(n) * extents_stride, e);
    load3_in_vgpr(motion, size_t(n) * motion_stride, mot);
    const uint32_t depth = vxb::depth_of(w.head());
    // (the rule's floats stay in VGPRs with the box: what is scalar of a pass is its axis, its direction and its bricks)
    const float world = in_vgpr(float(1u << depth)), skin_v = in_vgpr(skin);
    vxb::MoveBox m;
    const bool valid = vxb::move_begin(m, o, f, e, has_offset != 0, mot, scale, depth);
    if (!uniform(valid ? 1u : 0u)) {  // (wave-uniform) no load from the world
        if (lane == 0) store_record(out + n, vxb::move_invalid());
        return;
    }
    const uint32_t i = lane & 7u, j = lane >> 3;
#pragma nounroll
    for (uint32_t pass = 0; pass < 3; ++pass) {
        const uint32_t a = vxb::move_axis(order, pass);  // (of a kernel argument: scalar)
        const float d = vxb::pick3(m.d, a);
        const uint32_t dir = uniform(d > 0.0f ? 2u : (d < 0.0f ? 1u : 0u));
        vxb::MoveStep st = {0.0f, 0u, 0u};
        if (dir) {  // (wave-uniform)
            const bool up = dir == 2u;
            // sv: the slab as the lanes hold it (VGPRs, for their own tests); its brick range goes through readfirstlane (SGPRs, for the loops)
            const vxb::Cover sv = vxb::move_slab(m.mn, m.mx, a, d, skin_v, world);
            vxb::MoveKey best = vxb::move_key_none();
            if (uniform(sv.some)) {
                // the slab's brick range stays with the lanes too; scalar are the three counts, in one register, and a brick's corner
                const vxb::BoxBricks rv = vxb::cover_bricks(sv);
                const uint32_t counts = uniform(vxb::pick3(rv.count, a) | ((a == 0 ? rv.count[1] : rv.count[0]) << 8) | ((a == 2 ? rv.count[1] : rv.count[2]) << 16));
                const uint32_t layers = counts & 0xffu, nu = (counts >> 8) & 0xffu, nv = counts >> 16;
#pragma nounroll
                for (uint32_t layer = 0; layer < layers; ++layer) {
#pragma nounroll
                    for (uint32_t bv = 0; bv < nv; ++bv) {
#pragma nounroll
                        for (uint32_t bu = 0; bu < nu; ++bu) {
                            uint32_t cx, cy, cz;
                            vxb::move_brick_corner(rv, a, up, layer, bu, bv, cx, cy, cz);
                            const vxb::Brick b = vxb::enter_brick_at<kFormat<SVO>>(w, uniform(cx), uniform(cy), uniform(cz));  // (wave-uniform)
                            if (!vxb::box_brick_skipped(b, only_value)) vxb::move_brick_lane<kFormat<SVO>>(w, sv, a, up, only_value, b, i, j, best);  // (a scalar branch)
                        }
                    }
                    if (__ballot(best.key != vxb::kBoxNoKey)) break;  // a nearer brick layer cannot be beaten by a farther one
                }
                fold_wave(best, vxb::move_fold);
            }
            st = vxb::move_step(sv, a, d, skin_v, vxb::pick3(m.mn, a), vxb::pick3(m.mx, a), best);  // (every lane the same)
        }
        vxb::move_end_pass(m, a, has_offset != 0, st);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) m.hit.origin[a] = m.origin[a];
    if (lane == 0) store_record(out + n, m.hit);
}

}  // namespace

namespace vxk {

hipError_t launch_move_boxes(int svo, hipStream_t stream, const SceneArgs& sc, const void* origin, const void* offset, const void* extents,
                             const void* motion, uint32_t origin_stride, uint32_t offset_stride, uint32_t extents_stride, uint32_t motion_stride,
                             uint32_t only_value, const vx_move_shape& shape, uint32_t count, vx_move_hit* out) {
    static_assert(sizeof(vx_move_hit) == 48, "three 16-byte stores");
    if (count == 0 || count > vxb::kMaxCount || !vxb::move_order_ok(shape.order)) return hipErrorInvalidValue;
    const dim3 grid(count, 1, 1), block(64);  // (a grid's x may be as large as 2^31 - 1)
    const uint8_t *po = static_cast<const uint8_t*>(origin), *pf = static_cast<const uint8_t*>(offset), *pe = static_cast<const uint8_t*>(extents),
                  *pm = static_cast<const uint8_t*>(motion);
    const uint32_t has_offset = offset ? 1u : 0u;
    return for_format(svo, [&](auto f) {
        hipLaunchKernelGGL((move_boxes_kernel<decltype(f)::value>), grid, block, 0, stream, sc, po, pf, pe, pm, origin_stride, offset_stride, extents_stride, motion_stride,
                           has_offset, only_value, shape.scale, shape.skin, shape.order, out);
    });
}

}  // namespace vxk
