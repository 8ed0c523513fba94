// TEST HARNESS ONLY: compiles vx_trace_rays' per-ray device code (voxel-rs_amd/csrc/trace/vx_trace.hpp, over vx_device.hpp) for the host with
// the shims of tests/cpp/shims/hip_on_host.hpp, in the manner of device_on_host.cpp, so that the arithmetic can be held against the oracle without a GPU.
// Never linked into the product libraries; the product has no CPU path.
#include "hip_on_host.hpp"
#include "vx_trace.hpp"

namespace vxd { unsigned char* vx_smem = nullptr; }
using namespace vxd;

// `n` rays as trace_rays_kernel (csrc/trace/kernels_trace.hip) traces them, one lane's stack: packed origins and directions (3 floats a ray), one
// max_dst a ray. rgba32f (4 floats a ray), rgba8 (one word a ray: pack_rgba8) and hits (vx_hit, through the three 16-byte words the kernel
// stores) are all written. The scene's arguments are devhost_ray_batch's.
extern "C" void tracehost_trace_rays(int svo_type, const uint8_t* world, uint64_t world_bytes, const vx_material* mats, uint32_t n_mats, const uint8_t* tex,
                                     uint32_t tw, uint32_t th, uint32_t layers, uint32_t levels, const uint32_t* level_offset, const vx_uniforms* uniforms,
                                     const float* origins, const float* dirs, const float* max_dst, uint32_t n, float* rgba32f, uint32_t* rgba8, vx_hit* hits) {
    const SceneArgs sa = bytes_scene_args(world, world_bytes, mats, n_mats, tex, tw, th, layers, levels, level_offset);
    const DevScene sc = make_scene(sa);
    const RenderParams p = vxt::params_of(*uniforms);
    std::vector<unsigned char> lds(Stack<1>::kBytes + 64);
    vx_smem = lds.data();
    StackSpill spill;
    Stack<1> st;
    st.init(0, &spill);
    for (uint32_t i = 0; i < n; ++i) {
        float color[4];
        vx_hit rec;
        if (svo_type == 1) vxt::trace_ray<1>(sc, p, origins + 3 * i, dirs + 3 * i, max_dst[i], st, color, rec);
        else vxt::trace_ray<2>(sc, p, origins + 3 * i, dirs + 3 * i, max_dst[i], st, color, rec);
        std::memcpy(rgba32f + 4 * i, color, 16);
        rgba8[i] = pack_rgba8(color);
        uint4 w[3];
        vxt::hit_words(rec, w);
        std::memcpy(reinterpret_cast<uint8_t*>(hits + i), w, 48);
    }
}
