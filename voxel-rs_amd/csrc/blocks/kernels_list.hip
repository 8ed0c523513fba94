// vx_list_region's kernels (gfx950): vx_list.hpp's compact list of a box's blocks with their open faces, the world's own bytes read as
// kernels_blocks.hip reads them (vx_world_bytes.hpp: a read beyond the world gives 0). The world is read-only for the three launches, which
// run one behind the other on one stream: that order is the only dependency between workgroups. No kernel waits for another workgroup, none
// uses an atomic.
//   count    a workgroup (one wave) owns one brick, as in read_region_kernel: the descent to the brick once through wave-uniform addresses;
//            a brick outside the world, or whose descent ended in air, writes 0 and leaves -- a scalar branch, no load, no halo work. Else,
//            with faces: per side one wave-uniform descent to the neighbouring brick and one voxel a lane through its last three levels
//            (none where that descent ended above the brick), the 64 answers gathered by a ballot into a mask every lane holds (SGPRs);
//            then the lane's column (vxb::brick_column) as a mask of 8 bits, its neighbours' masks by four shuffles (lanes l -+ 1, l -+ 8),
//            the bordering columns' from the ballots -- nothing goes through memory. Per z-slice a ballot of the kept voxels; the eight
//            popcounts summed are counts[brick].
//   offsets  ONE workgroup of 1,024 lanes walks the counts 4,096 at a time (16 bytes a lane a trip): a wave scan by shuffles, the 16 wave
//            sums through LDS (64 bytes), the running sum in a register. An exclusive prefix sum in place; counts[bricks] and *total
//            receive the sum. 2^24 voxels are at most about 2.1 M bricks: 512 trips.
//   write    one wave a brick again. It RECOMPUTES the brick -- the descent, the halo, the column: what count did -- rather than read
//            back something count stashed: a stash would be 8 bytes a lane of every brick with a record (64 dwords of column masks and up
//            to six halo masks a brick, against the 4 bytes a brick of workspace there is), written and read once, while the recomputation
//            reads world bytes count has just pulled through the caches and is skipped by every brick without a record (two scalar loads
//            and a branch) and by every brick whose first record lies at or beyond `capacity`. Its cost is count's for the bricks that
//            hold records; profiles/list_bench.py measures both launches together. Per slice the lane's slot is the brick's offset, plus
//            the kept voxels of the slices before, plus popc(ballot & lanes below); one 8-byte store per kept voxel with slot < capacity.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, ESVO / CSVO / ESVO beyond 4 GiB): count without faces 41 / 57 / 40 VGPRs, with
// faces 43 / 57 / 40; write without faces 42 / 57 / 40, with faces 43 / 57 / 40 (the six halo masks live in SGPRs: 49 to 78 of them);
// offsets 36 VGPRs and 64 bytes of LDS. No spill and no scratch in any of the thirteen; no LDS but the offsets kernel's.
#include <hip/hip_runtime.h>

#include "kernels_blocks.h"
#include "kernels_shared.hpp"
#include "vx_device.hpp"
#include "vx_world_bytes.hpp"

using namespace vxd;
using vxk::kFormat;
using vxk::WorldBytes;

namespace {

constexpr uint32_t kScanLanes = 1024, kScanEach = 4;

template <int SVO, bool FACES, bool WRITE>
__global__ __launch_bounds__(64) void list_region_kernel(SceneArgs sa, vxb::Region r, uint32_t flags, uint32_t* __restrict__ counts,
                                                         vx_block_at* __restrict__ out, uint32_t capacity) {
    uint32_t base = 0;
    if (WRITE) {  // (wave-uniform: two scalar loads and a branch)
        base = counts[blockIdx.x];
        if (counts[blockIdx.x + 1] == base || base >= capacity) return;
    }
    const WorldBytes<SVO> w = {make_scene(sa)};
    const vxb::Brick b = vxb::enter_brick<kFormat<SVO>>(w, r, blockIdx.x);  // (wave-uniform)
    const uint32_t lane = threadIdx.x, i = lane & 7u, j = lane >> 3;
    if (vxb::brick_is_air(b)) {  // (wave-uniform; a write wave never comes here: its brick has records)
        if (!WRITE && lane == 0) counts[blockIdx.x] = 0;
        return;
    }
    uint64_t halo[6] = {0, 0, 0, 0, 0, 0};
    if (FACES) {
#pragma unroll
        for (uint32_t f = 0; f < 6; ++f) {
            const vxb::Brick nb = vxb::enter_neighbour<kFormat<SVO>>(w, b, f);  // (wave-uniform)
            halo[f] = __ballot(vxb::halo_lane<kFormat<SVO>>(w, nb, f, lane));
        }
    }
    uint32_t value[vxb::kBrick];
    vxb::brick_column<kFormat<SVO>>(w, b, i, j, value);
    const uint32_t col = vxb::column_mask(value);
    uint32_t open[6] = {0, 0, 0, 0, 0, 0};
    if (FACES) {  // (a lane at the brick's border gets its own mask back from the shuffle: column_open takes the halo's byte there)
        const uint32_t xm = __shfl_up(col, 1, 64), xp = __shfl_down(col, 1, 64), ym = __shfl_up(col, 8, 64), yp = __shfl_down(col, 8, 64);
        vxb::column_open(i, j, col, xm, xp, ym, yp, halo, open);
    }
    const uint32_t keep = vxb::column_keep(r, b, i, j, col, flags, open);
    if (!WRITE) {
        uint32_t n = 0;
#pragma unroll
        for (uint32_t k = 0; k < vxb::kBrick; ++k) n += uint32_t(__popcll(__ballot((keep >> k) & 1u)));
        if (lane == 0) counts[blockIdx.x] = n;
        return;
    }
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (uint32_t k = 0; k < vxb::kBrick; ++k) {
        const bool kept = ((keep >> k) & 1u) != 0;
        const unsigned long long m = __ballot(kept);
        const uint32_t slot = base + uint32_t(__popcll(m & below));
        uint32_t index;
        vxb::box_index(r, b, i, j, k, index);
        if (kept && slot < capacity) *reinterpret_cast<uint2*>(out + slot) = make_uint2(vxb::where_of(index, open, k), value[k]);
        base += uint32_t(__popcll(m));
    }
}

__global__ __launch_bounds__(kScanLanes) void list_offsets_kernel(uint32_t* __restrict__ counts, uint32_t n, uint32_t* __restrict__ total) {
    __shared__ uint32_t wave_sum[kScanLanes / 64];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    uint32_t carry = 0;
    for (uint32_t first = 0; first < n; first += kScanLanes * kScanEach) {  // (uniform over the workgroup: every lane meets every barrier)
        const uint32_t at = first + t * kScanEach;
        const bool whole = at + kScanEach <= n;  // (counts is 16-byte aligned and `at` a multiple of 4)
        uint32_t v[kScanEach];
        if (whole) {
            const uint4 q = *reinterpret_cast<const uint4*>(counts + at);
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        } else {
#pragma unroll
            for (uint32_t q = 0; q < kScanEach; ++q) v[q] = at + q < n ? counts[at + q] : 0u;
        }
        const uint32_t mine = v[0] + v[1] + v[2] + v[3];
        uint32_t inc = mine;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(inc, d, 64);
            if (lane >= d) inc += up;
        }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t q = 0; q < kScanLanes / 64; ++q) {
            const uint32_t s = wave_sum[q];
            before += q < wave ? s : 0u;
            all += s;
        }
        const uint32_t e0 = carry + before + inc - mine, e1 = e0 + v[0], e2 = e1 + v[1], e3 = e2 + v[2];
        if (whole) {
            *reinterpret_cast<uint4*>(counts + at) = make_uint4(e0, e1, e2, e3);
        } else {
            if (at < n) counts[at] = e0;
            if (at + 1 < n) counts[at + 1] = e1;
            if (at + 2 < n) counts[at + 2] = e2;
            if (at + 3 < n) counts[at + 3] = e3;
        }
        carry += all;
        __syncthreads();  // (the next trip writes wave_sum again)
    }
    if (t == 0) {
        counts[n] = carry;
        *total = carry;
    }
}

}  // namespace

namespace vxk {

static hipError_t list_grid(const vxb::Region& r, dim3& grid) {
    const uint64_t bricks = vxb::region_bricks(r);
    if (bricks == 0 || bricks > 0x7fffffffull) return hipErrorInvalidValue;  // (a region of 2^24 voxels has fewer than 2^24 bricks)
    grid = dim3(static_cast<uint32_t>(bricks), 1, 1);
    return hipSuccess;
}

// count (WRITE false: out null, capacity 0) and write share one launch
template <bool WRITE>
static hipError_t launch_list(int svo, hipStream_t stream, const SceneArgs& sc, const vxb::Region& r, uint32_t flags, uint32_t* counts, vx_block_at* out, uint32_t capacity) {
    dim3 grid;
    if (const hipError_t e = list_grid(r, grid); e != hipSuccess) return e;
    const bool faces = vxb::list_wants_faces(flags);
    return for_format(svo, [&](auto f) {
        constexpr int S = decltype(f)::value;
        if (faces) hipLaunchKernelGGL((list_region_kernel<S, true, WRITE>), grid, dim3(64), 0, stream, sc, r, flags, counts, out, capacity);
        else hipLaunchKernelGGL((list_region_kernel<S, false, WRITE>), grid, dim3(64), 0, stream, sc, r, flags, counts, out, capacity);
    });
}

hipError_t launch_list_count(int svo, hipStream_t stream, const SceneArgs& sc, const vxb::Region& r, uint32_t flags, uint32_t* counts) {
    return launch_list<false>(svo, stream, sc, r, flags, counts, nullptr, 0);
}

hipError_t launch_list_offsets(hipStream_t stream, uint32_t* counts, uint32_t bricks, uint32_t* total) {
    hipLaunchKernelGGL(list_offsets_kernel, dim3(1), dim3(kScanLanes), 0, stream, counts, bricks, total);
    return hipGetLastError();
}

hipError_t launch_list_write(int svo, hipStream_t stream, const SceneArgs& sc, const vxb::Region& r, uint32_t flags, uint32_t* counts, vx_block_at* out,
                             uint32_t capacity) {
    static_assert(sizeof(vx_block_at) == 8, "one 8-byte store");
    return launch_list<true>(svo, stream, sc, r, flags, counts, out, capacity);
}

}  // namespace vxk
