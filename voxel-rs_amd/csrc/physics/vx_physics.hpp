// Entity physics on the device, per entity: what systems::Physics does with one entity in one step (src/systems/physics.rs:111-185)
// over the AABB ray fan of graphics::svo_picker (src/graphics/svo_picker.rs:183-299). Plain device code over vx_device.hpp -- every
// function is VX_HD, so the CPU test harness (tests/cpp/physics_on_host.cpp) compiles this file for the host with the same shims
// as the traversal.
//
// Numerics contract: bit for bit csrc/host/physics.hpp and svo_picker.hpp (the host mirror that drives vx_raycast): fp32 only, every
// operation written in the reference's order, no contraction (-ffp-contract=off).
#pragma once

#include "vx_device.hpp"
#include "vx_physics_rules.h"

#define VX_HD __device__ __forceinline__

namespace vxp {

constexpr float kPhysicsEpsilon = 0.0005f;  // physics.rs:8
constexpr float kFanMaxDst = 10.0f;         // svo_picker.rs:214: every ray of a fan

VX_HD bool steppable(const vx_entity& e) { return steppable_extents(e.aabb_extents); }  // (vx_physics_rules.h)

// What of a fan does not move with the entity (svo_picker.rs:184-195): grid points every <= 1 block across the box.
// A SLOT is s = point * 3 + axis over the (bx+1)(by+1)(bz+1) grid points, z fastest (the reference's loop order); it is live -- holds a
// ray -- when the point lies on that axis's boundary of the box. The live slots are the reference's tasks, in its order.
struct Fan {
    int blocks[3];
    float step[3];
    uint32_t slots;
};

VX_HD Fan make_fan(const vx_entity& e) {
    Fan f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        f.blocks[a] = int(__builtin_ceilf(e.aabb_extents[a]));
        f.step[a] = e.aabb_extents[a] / float(f.blocks[a]);
    }
    f.slots = uint32_t(f.blocks[0] + 1) * uint32_t(f.blocks[1] + 1) * uint32_t(f.blocks[2] + 1) * 3u;
    return f;
}

// Slot s of the fan at the entity's current position: false = no ray there. `which` = the contact the ray's hit distance folds into:
// 0..2 = neg x, y, z; 3..5 = pos x, y, z (vx_aabb_result's order). svo_picker.rs:197-238.
VX_HD bool fan_ray(const Fan& f, const vx_entity& e, uint32_t s, float ro[3], float rd[3], int& which) {
    if (s >= f.slots) return false;
    const uint32_t point = s / 3u, axis = s - point * 3u;
    const uint32_t nz = uint32_t(f.blocks[2] + 1), ny = uint32_t(f.blocks[1] + 1);
    const uint32_t xy = point / nz;
    const int z = int(point - xy * nz), x = int(xy / ny), y = int(xy - uint32_t(x) * ny);
    const int v = axis == 0 ? x : (axis == 1 ? y : z);
    const int last = axis == 0 ? f.blocks[0] : (axis == 1 ? f.blocks[1] : f.blocks[2]);
    if (v != 0 && v != last) return false;
    ro[0] = e.position[0] + e.aabb_offset[0] + float(x) * f.step[0];
    ro[1] = e.position[1] + e.aabb_offset[1] + float(y) * f.step[1];
    ro[2] = e.position[2] + e.aabb_offset[2] + float(z) * f.step[2];
    const float d = v == 0 ? -1.0f : 1.0f;
    rd[0] = axis == 0 ? d : 0.0f;
    rd[1] = axis == 1 ? d : 0.0f;
    rd[2] = axis == 2 ? d : 0.0f;
    which = int(axis) + (v == 0 ? 0 : 3);
    return true;
}

// The fold of svo_picker.rs:245-299 as running minima, +inf = none yet: a hit distance is a t > 0, never NaN, so the minimum
// over any order of the rays is the reference's value.
struct Contacts {
    float m[6];
};
VX_HD Contacts no_contacts() {
    Contacts c;
#pragma unroll
    for (int k = 0; k < 6; ++k) c.m[k] = __uint_as_float(0x7f800000u);
    return c;
}
VX_HD void fold(Contacts& c, int which, float dst) {
#pragma unroll
    for (int k = 0; k < 6; ++k) c.m[k] = (k == which && dst < c.m[k]) ? dst : c.m[k];
}
VX_HD vx_aabb_result finish(const Contacts& c) {
    vx_aabb_result r;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.neg[k] = c.m[k] == __uint_as_float(0x7f800000u) ? -1.0f : c.m[k];
        r.pos[k] = c.m[3 + k] == __uint_as_float(0x7f800000u) ? -1.0f : c.m[3 + k];
    }
    return r;
}
VX_HD vx_aabb_result no_result() { return finish(no_contacts()); }

// f32::signum: 1.0 for +0.0 and positives, -1.0 for -0.0 and negatives, NaN for NaN
VX_HD float signum(float v) { return v != v ? v : ((__float_as_uint(v) >> 31) ? -1.0f : 1.0f); }
// f32::max (physics.rs:143): the other operand when one is NaN
VX_HD float max_f32(float a, float b) { return a != a ? b : (b != b ? a : (a < b ? b : a)); }

// physics.rs:172-185
VX_HD float apply_axial_physics(float speed, float dst_pos, float dst_neg) {
    const float dst = speed > 0.0f ? dst_pos : dst_neg;
    if (dst == -1.0f) return speed;
    if (dst < 2.0f * kPhysicsEpsilon) return 0.0f;
    if (__builtin_fabsf(speed) > dst) return (dst - kPhysicsEpsilon) * signum(speed);
    return speed;
}

// physics.rs:138-170
VX_HD void update_entity(vx_entity& e, const vx_aabb_result& result, float delta_time) {
    const bool wall_clip = (e.flags & VX_ENTITY_WALL_CLIP) != 0, flying = (e.flags & VX_ENTITY_FLYING) != 0;
    // apply gravity
    if (!flying) {
        e.velocity[1] -= e.gravity * delta_time;
        if (e.velocity[1] < 0.0f) e.velocity[1] = max_f32(e.velocity[1], -e.max_fall_velocity);
    }
    float vx = e.velocity[0] * delta_time, vy = e.velocity[1] * delta_time, vz = e.velocity[2] * delta_time;

    // entity state with the new velocity
    const bool grounded = !flying && (result.neg[1] + vy) < 0.02f && result.neg[1] != -1.0f;
    e.grounded = grounded ? 1u : 0u;
    // reset gravity if the entity stands on the ground already
    if (grounded && e.velocity[1] < 0.0f) e.velocity[1] = 0.0f;

    // constrain the velocity by nearby collisions
    if (!flying) {
        if (!wall_clip) {
            vx = apply_axial_physics(vx, result.pos[0], result.neg[0]);
            vz = apply_axial_physics(vz, result.pos[2], result.neg[2]);
        }
        vy = apply_axial_physics(vy, result.pos[1], result.neg[1]);
    }
    e.position[0] += vx;
    e.position[1] += vy;
    e.position[2] += vz;
}

// One ray of a fan through the world's own bytes, as picker_kernel casts it (picker.glsl:30-51): the hit distance, or a value <= 0
template <int SVO, class ST>
VX_HD float cast_fan_ray(const vxd::DevScene& sc, const float ro[3], const float rd[3], const ST& st) {
    vxd::Result res;
    uint32_t n = 0;
    vxd::intersect<SVO, false, false, true>(sc, ro, rd, kFanMaxDst, false, st, res, n, nullptr, nullptr);
    return res.t;
}

// ---- a step, as physics_kernel runs it: the parts every driver of this header shares (the kernel's wave; the test harness's loop over 64 lanes) ----

constexpr uint32_t kLanes = 64;  // a wave: trips of 64 slots

// the fans a call casts per entity: one per step; steps == 0 casts the fan at the current position and moves nothing
VX_HD uint32_t rounds_of(uint32_t steps) { return steps ? steps : 1u; }

// lane `lane`'s share of one fan: the slots lane, lane + 64, ... cast and folded
template <int SVO, class ST>
VX_HD Contacts lane_contacts(const vxd::DevScene& sc, const Fan& fan, const vx_entity& e, uint32_t lane, const ST& st) {
    Contacts c = no_contacts();
    for (uint32_t s = lane; s < fan.slots; s += kLanes) {
        float ro[3], rd[3];
        int which;
        if (fan_ray(fan, e, s, ro, rd, which)) {
            const float t = cast_fan_ray<SVO>(sc, ro, rd, st);
            if (t > 0.0f) fold(c, which, t);
        }
    }
    return c;
}

// after the lanes' minima have been reduced across the wave: the contacts of this fan, and the entity's update unless the call makes no steps
VX_HD vx_aabb_result finish_round(vx_entity& e, const Contacts& reduced, float delta_time, uint32_t steps) {
    const vx_aabb_result result = finish(reduced);
    if (steps) update_entity(e, result, delta_time);
    return result;
}

// after the last round, by ONE lane: the record (unless nothing moved) and the contacts (if asked for)
VX_HD void write_back(vx_entity* entities, vx_aabb_result* contacts, uint32_t i, const vx_entity& e, const vx_aabb_result& result, uint32_t steps) {
    if (steps) entities[i] = e;
    if (contacts) contacts[i] = result;
}
// ... and for a record that cannot be stepped: its bytes stay, its contacts are "none"
VX_HD void write_back_unsteppable(vx_aabb_result* contacts, uint32_t i) {
    if (contacts) contacts[i] = no_result();
}

}  // namespace vxp
