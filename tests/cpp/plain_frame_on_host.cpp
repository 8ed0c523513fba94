// vxk::plain_frame (csrc/hip/vx_args.hpp) on the host: the launch the render kernel's whole-frame builds may serve, and each of its seven conditions
// flipped alone. Prints "<name> <0|1>" per line; tests/test_plain_frame.py reads them.
#include <cstdio>

#include "hip_on_host.hpp"  // (uint2)
#include "vx_args.hpp"

int main() {
    float pixels[4] = {};
    unsigned int table[1] = {};
    unsigned long long counters[4] = {};
    vxd::RenderParams p = {};
    p.tile_count = 1;
    p.rgba8 = 0;
    p.affine_view = 1;
    vxk::PersistentArgs a = {};
    const void* out = pixels;
    std::printf("plain %d\n", int(vxk::plain_frame(p, a, out)));
    {
        vxd::RenderParams q = p;
        q.tile_count = 3;
        std::printf("tile_count %d\n", int(vxk::plain_frame(q, a, out)));
    }
    {
        vxd::RenderParams q = p;
        q.rgba8 = 1;
        std::printf("rgba8 %d\n", int(vxk::plain_frame(q, a, out)));
    }
    std::printf("out %d\n", int(vxk::plain_frame(p, a, nullptr)));
    {
        vxk::PersistentArgs b = a;
        b.order = table;
        std::printf("order %d\n", int(vxk::plain_frame(p, b, out)));
    }
    {
        vxk::PersistentArgs b = a;
        b.cost_cur = table;
        std::printf("cost_cur %d\n", int(vxk::plain_frame(p, b, out)));
    }
    {
        vxk::PersistentArgs b = a;
        b.excursions = counters;
        std::printf("excursions %d\n", int(vxk::plain_frame(p, b, out)));
    }
    {
        vxd::RenderParams q = p;
        q.affine_view = 0;
        std::printf("affine_view %d\n", int(vxk::plain_frame(q, a, out)));
    }
    return 0;
}
