// Platform layer for the kernels in this directory.
//
// The product build is hipcc --offload-arch=gfx950 (everything below the #else).  The
// MIRA_CPU_EMU branch exists ONLY for tests/emu: it runs the same kernel sources on host
// threads (one OS thread per lane of a workgroup when the kernel uses a barrier) so kernel
// indexing can be checked, and sanitizers run, in a container without a GPU.  It is never
// part of libmira_gpu.so and mira_amd/ never loads it.
#pragma once
#ifdef __HIPCC_RTC__
// Runtime compilation of a specialised cross-term kernel (graph.hip, graph_jit.cuh): hiprtc brings the HIP device
// environment and the fixed-width integer types, but no libc headers; only the device-side arithmetic is needed.
typedef unsigned int uint32_t;
typedef int int32_t;
typedef unsigned long long uint64_t;
typedef long long int64_t;
typedef unsigned long size_t;
#define HD __device__ __forceinline__
#define DEV __device__ __forceinline__
#else
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#endif

#if defined(__HIPCC_RTC__)
#elif !defined(MIRA_CPU_EMU)
#include <hip/hip_runtime.h>
#define HD __host__ __device__ __forceinline__
#define DEV __device__ __forceinline__
#define KERNEL static __global__
#define LAUNCH(kern, grid, block, shmem, stream, ...) \
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), (shmem), (stream), __VA_ARGS__)
#define LAUNCH_BARRIER LAUNCH
#define LAUNCH_BARRIER_FLEX LAUNCH   // kernel is correct for any blockDim (strided loops)
// lanes of one wave exchange data through LDS without a workgroup barrier: the DS unit serves a
// wave's instructions in order; the fence keeps the compiler from moving LDS accesses across it
#define WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
// DPP quads (quad29.cuh): lanes 4 i .. 4 i + 3 of a wave; quad_bcast<K> = every lane reads lane K of its quad
static constexpr bool QUAD_COOPERATIVE = true;
static __device__ __forceinline__ uint32_t quad_lane() { return threadIdx.x & 3u; }
template <int K> static __device__ __forceinline__ uint32_t quad_bcast(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, K * 0x55, 0xF, 0xF, true);   // quad_perm:[K,K,K,K]
}
// a word of mapped host memory the host spins on (ctx.h: rt_wait_flag)
static __device__ __forceinline__ void store_release_system(uint64_t *p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); }
#define DYN_SHARED(type, name) extern __shared__ __attribute__((aligned(16))) unsigned char name##_raw[]; type *name = reinterpret_cast<type *>(name##_raw)
// Global-memory atomics of the hash table in lookup_kernels.cuh (vector-memory atomics: plain HIP builtins)
static __device__ __forceinline__ uint64_t atomic_cas_u64(uint64_t *p, uint64_t cmp, uint64_t val) {
    return (uint64_t)atomicCAS(reinterpret_cast<unsigned long long *>(p), (unsigned long long)cmp, (unsigned long long)val);
}
static __device__ __forceinline__ uint32_t atomic_min_u32(uint32_t *p, uint32_t v) { return atomicMin(p, v); }
// Wave-level aggregation before an atomic on a hot address: among the active lanes of the calling wave, those whose `key`
// equals this lane's form a group; *count = its size, and the return value is true for its lowest lane only (the one that
// issues the group's atomic).  Every pass of the loop retires the group of the lowest remaining lane, so it ends after at
// most 64 passes; no lane waits for another.
static __device__ __forceinline__ bool wave_group_leader(uint64_t key, uint32_t *count, uint32_t *leader_lane = nullptr) {
    uint64_t todo = __ballot(1);
    const uint32_t lane = __lane_id();
    for (;;) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint64_t lk = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(key >> 32), leader) << 32) |
                            (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)key, leader);
        const uint64_t same = __ballot(key == lk);
        if (key == lk) {
            *count = (uint32_t)__popcll(same);
            if (leader_lane) *leader_lane = (uint32_t)leader;
            return lane == (uint32_t)leader;
        }
        todo &= ~same;
    }
}
// v of lane `src` of the calling wave (which must be active)
static __device__ __forceinline__ uint64_t wave_shfl_u64(uint64_t v, uint32_t src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)src);
    return ((uint64_t)hi << 32) | lo;
}
#else
#include "../../tests/emu/emu.h"
// lookup_kernels.cuh: emulated lanes are not in lockstep, so there is no wave to aggregate over; every lane issues its own atomic
// (the values are the same: the atomics are additions and minima)
inline uint64_t atomic_cas_u64(uint64_t *p, uint64_t cmp, uint64_t val) {
    __atomic_compare_exchange_n(p, &cmp, val, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
    return cmp;
}
inline uint32_t atomic_min_u32(uint32_t *p, uint32_t v) {
    uint32_t o = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < o && !__atomic_compare_exchange_n(p, &o, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return o;
}
inline bool wave_group_leader(uint64_t, uint32_t *count, uint32_t *leader_lane = nullptr) { *count = 1; if (leader_lane) *leader_lane = 0; return true; }
inline uint64_t wave_shfl_u64(uint64_t v, uint32_t) { return v; }   // every emulated lane leads its own group: it only ever reads itself
#endif
