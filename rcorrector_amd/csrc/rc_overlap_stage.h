// rc_overlap_stage.h -- what the kernels that keep a wavefront's reads as rc_overlap.h strings in LDS share (device code only;
// k_mate_overlap in rc_overlap.hip, k_read_trim in rc_trim.hip): the barrier of one wavefront and the staging of a read,
// 16 bytes a lane, in ALIGNED 16-byte pieces.
#pragma once
#include "rc_overlap.h"

__device__ __forceinline__ void rc_ov_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// bytes [16 c, 16 c + 16) of the string of len bytes at arena byte o, as four dwords (first byte in the low bits; the bytes at
// or behind len as 0; a chunk behind the string: four zeros, nothing loaded).  The two aligned pieces a chunk straddles are
// shifted together: up to 15 bytes in front of the string and behind it are loaded, within the 16-byte granules its bytes lie in.
__device__ __forceinline__ void rc_ov_load16(const uint8_t *__restrict__ seq, uint32_t o, uint32_t len, uint32_t c, uint32_t (&w)[4])
{
    w[0] = w[1] = w[2] = w[3] = 0;
    if (16u * c < len) {
        const uintptr_t s = (uintptr_t)(seq + o), a0 = s & ~(uintptr_t)15;
        const uint32_t lead = (uint32_t)(s - a0), n_pc = (lead + len + 15u) >> 4;  // aligned pieces that hold a byte of the read
        const uint4 *pc = reinterpret_cast<const uint4 *>(a0) + c;
        const uint4 p0 = pc[0];  // (16 c < len: holds a byte of the read)
        uint4 p1 = make_uint4(0, 0, 0, 0);
        if (lead && c + 1u < n_pc) p1 = pc[1];  // (holds one too)
        typedef unsigned __int128 u128;
        const u128 lo = ((u128)(((uint64_t)p0.w << 32) | p0.z) << 64) | (((uint64_t)p0.y << 32) | p0.x);
        const u128 hi = ((u128)(((uint64_t)p1.w << 32) | p1.z) << 64) | (((uint64_t)p1.y << 32) | p1.x);
        u128 ch = lead ? (lo >> (8u * lead)) | (hi << (128u - 8u * lead)) : lo;
        const uint32_t left = len - 16u * c;  // bytes of the chunk inside the read
        if (left < 16u) ch &= (((u128)1) << (8u * left)) - 1;
        w[0] = (uint32_t)ch;
        w[1] = (uint32_t)(ch >> 32);
        w[2] = (uint32_t)(ch >> 64);
        w[3] = (uint32_t)(ch >> 96);
    }
}

// chunk c of the read of len bases at arena byte o: half a word of its strings (0 / not valid behind the read's end)
__device__ __forceinline__ void rc_ov_chunk(const uint8_t *__restrict__ seq, uint32_t o, uint32_t len, uint32_t c, uint32_t &code, uint32_t &val)
{
    uint32_t w[4];
    rc_ov_load16(seq, o, len, c, w);
    rc_ov_pack16(w, code, val);
}
