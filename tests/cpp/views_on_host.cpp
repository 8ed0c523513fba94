// TEST HARNESS ONLY: compiles vx_trace_views' per-lane device code (voxel-rs_amd/csrc/trace/vx_views.hpp, over vx_trace.hpp and vx_device.hpp) for the
// host with the shims of tests/cpp/shims/hip_on_host.hpp, in the manner of trace_on_host.cpp, so that the arithmetic and the indexing can be held
// against the oracle without a GPU. Never linked into the product libraries; the product has no CPU path.
#include "hip_on_host.hpp"
#include "vx_views.hpp"

namespace vxd { unsigned char* vx_smem = nullptr; }
using namespace vxd;

// Every lane of every workgroup of trace_views_kernel's grid (csrc/trace/kernels_views.hip) for `count` views of width x height pixels, one lane's
// stack: the table of views is made as views_runtime.cpp makes it (view_params_of, on the host), the pixel found as the kernel finds it
// (pixel_of), and a lane inside the image stores at out_index what the kernel stores there: rgba32f (4 floats), rgba8 (one word: pack_rgba8)
// and hits (vx_hit, through the three 16-byte words). `rgba8_rows` is the kernel's rgba8 argument: the row order of a view. writes[i] counts
// the stores to index i (count * width * height entries); tally[0] = lanes that left because their pixel lies outside the image, tally[1] =
// stores to an index outside the outputs (not made), tally[2] = workgroups. The scene's arguments are devhost_ray_batch's.
extern "C" void viewshost_trace_views(int svo_type, const uint8_t* world, uint64_t world_bytes, const vx_material* mats, uint32_t n_mats, const uint8_t* tex,
                                      uint32_t tw, uint32_t th, uint32_t layers, uint32_t levels, const uint32_t* level_offset, const vx_uniforms* views,
                                      uint32_t count, uint32_t width, uint32_t height, uint32_t rgba8_rows, float* rgba32f, uint32_t* rgba8, vx_hit* hits,
                                      uint32_t* writes, uint64_t* tally) {
    const SceneArgs sa = bytes_scene_args(world, world_bytes, mats, n_mats, tex, tw, th, layers, levels, level_offset);
    const DevScene sc = make_scene(sa);
    std::vector<ViewParams> table(count);
    for (uint32_t k = 0; k < count; ++k) table[k] = view_params_of(views[k]);
    std::vector<unsigned char> lds(Stack<1>::kBytes + 64);
    vx_smem = lds.data();
    StackSpill spill;
    Stack<1> st;
    st.init(0, &spill);
    const uint32_t tiles_x = vxv::tiles_across(width), tiles_per_view = tiles_x * vxv::tiles_across(height);
    const size_t total = size_t(count) * width * height;
    tally[0] = tally[1] = 0;
    tally[2] = uint64_t(count) * tiles_per_view;
    for (uint32_t block = 0; block < count * tiles_per_view; ++block) {
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const vxv::Pixel px = vxv::pixel_of(block, lane, tiles_x, tiles_per_view);
            if (px.x >= width || px.y >= height) {
                ++tally[0];
                continue;
            }
            const RenderParams p = vxv::params_of(table[px.view], width, height, rgba8_rows);
            float color[4];
            vx_hit rec;
            if (svo_type == 1) vxv::trace_pixel<1>(sc, p, px.x, px.y, st, color, rec);
            else vxv::trace_pixel<2>(sc, p, px.x, px.y, st, color, rec);
            const size_t i = vxv::out_index(p, px.view, px.x, px.y);
            if (i >= total) {
                ++tally[1];
                continue;
            }
            ++writes[i];
            std::memcpy(rgba32f + 4 * i, color, 16);
            rgba8[i] = pack_rgba8(color);
            uint4 w[3];
            vxt::hit_words(rec, w);
            std::memcpy(reinterpret_cast<uint8_t*>(hits + i), w, 48);
        }
    }
}
