// TEST HARNESS ONLY: what a ray batch is (voxel-rs_amd/csrc/raycast/vx_ray_batch.hpp) compiled for the host with the shims of
// tests/cpp/shims/hip_on_host.hpp -- the rules, the plan, the packing and the kernels' gather for one ray -- so that a batch can be packed the
// way vx_raycast_batch and vx_trace_rays pack it and read back the way their kernels read it, without a GPU (tests/test_ray_batch_on_host.py,
// tests/cpp/sanitize_stress.cpp). Never linked into the product libraries; the product has no CPU path.
#include <string>

#include "hip_on_host.hpp"
#include "vx_ray_batch.hpp"

// (the product's is runtime.cpp's)
static thread_local std::string g_batch_error;
int vxrt::fail(int code, const std::string& msg) {
    g_batch_error = msg;
    return code;
}

extern "C" {

int batchhost_check(const vx_ray_batch* rays, const char* who) {
    g_batch_error.clear();
    return vxrt::check_ray_batch(*rays, who);
}
const char* batchhost_last_error(void) { return g_batch_error.c_str(); }

// out: n_dir, n_dst, at_dir, at_dst, end
void batchhost_plan(const vx_ray_batch* rays, uint32_t n, uint64_t out[5]) {
    const vxrt::RayPlan p = vxrt::plan_rays(*rays, n);
    out[0] = p.n_dir; out[1] = p.n_dst; out[2] = p.at_dir; out[3] = p.at_dst; out[4] = p.end;
}

// `n` rays packed to `scratch` (plan_rays' end bytes of it are written at most), which is its own device view here
void batchhost_pack(const vx_ray_batch* rays, uint32_t n, uint8_t* scratch, vxk::RayBatchArgs* out) {
    *out = vxrt::pack_rays(*rays, n, vxrt::plan_rays(*rays, n), scratch, scratch);
}

void batchhost_in_place(const vx_ray_batch* rays, vxk::RayBatchArgs* out) { *out = vxrt::rays_in_place(*rays); }

// ray i as a kernel's lane gathers it: origin, direction, limit -- 28 bytes
void batchhost_gather(const vxk::RayBatchArgs* a, uint32_t i, float out[7]) {
    vxk::gather_ray(static_cast<const uint8_t*>(a->origin), static_cast<const uint8_t*>(a->dir), static_cast<const uint8_t*>(a->max_dst), a->origin_stride,
                    a->dir_stride, a->max_dst_stride, a->max_dst_all, a->has_max_dst, i, out, out + 3, out[6]);
}

}  // extern "C"
