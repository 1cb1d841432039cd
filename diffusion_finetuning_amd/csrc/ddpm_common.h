// What ddpm_loss.hip, ddpm_prologue.hip and ddpm_sample.hip share: the Philox4x32-10 streams and their Box–Muller / integer-range
// mappings (counter layouts: the block comments of ddpm_prologue.hip and ddpm_sample.hip), the 4-element access type, the
// add_noise arithmetic with every product rounded on its own, and the host helpers that pick a kernel instantiation.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ float u01(uint32_t x) { return ((float)x + 0.5f) * 2.3283064365386963e-10f; }

template <typename T> struct alignas(4 * sizeof(T)) Quad {
    T v[4];
};

__device__ __forceinline__ void philox_normals4(uint64_t g, uint32_t stream, uint32_t seed, uint32_t step, float z[4]) {
    uint32_t r[4];
    philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), stream, 0u, seed, step, r);
    const float r0 = sqrtf(-2.f * logf(u01(r[0]))), r1 = sqrtf(-2.f * logf(u01(r[2])));
    float s0, c0, s1, c1;
    sincosf(6.283185307179586f * u01(r[1]), &s0, &c0);
    sincosf(6.283185307179586f * u01(r[3]), &s1, &c1);
    z[0] = r0 * c0; z[1] = r0 * s0; z[2] = r1 * c1; z[3] = r1 * s1;
}

__device__ __forceinline__ int64_t philox_timestep(uint32_t b, uint32_t seed, uint32_t step, int n_timesteps) {
    uint32_t tr[4];
    philox4x32_10(b, 0u, 1u, 0u, seed, step, tr);
    return (int64_t)(((uint64_t)tr[0] * (uint64_t)n_timesteps) >> 32);
}

// noisy and target with every product rounded on its own — what add_noise_kernel and noise_prologue_kernel compile to — and
// said so here, where the compiler would otherwise fuse them: a step fed with moments then leaves the very bits of the step
// fed with this launch's x0_out / eps_out / t_out.
__device__ __forceinline__ float ddpm_noisy(float a, float s, float x, float e) {
#pragma clang fp contract(off)
    const float ax = a * x, se = s * e;
    return ax + se;
}
__device__ __forceinline__ float ddpm_target(float a, float s, float x, float e, int v_pred) {
#pragma clang fp contract(off)
    const float ae = a * e, sx = s * x;
    return v_pred ? ae - sx : e;
}

template <typename T> bool quad_aligned(const void* p) {  // null: nothing to access
    return (reinterpret_cast<uintptr_t>(p) & (4 * sizeof(T) - 1)) == 0;
}

// One thread per Philox group of 4 consecutive elements, 256 threads a workgroup, grid-stride above 2048 workgroups.
inline unsigned posterior_blocks(int64_t n_total) {
    int64_t blocks = ((n_total + 3) / 4 + 255) / 256;
    return (unsigned)(blocks > 2048 ? 2048 : blocks);
}

}  // namespace
