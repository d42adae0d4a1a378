// mtr_sample.h — one source sample on the device: what the decode kernels of mtr_source.hip (k_pcm, k_pick, k_plane) compute alike, once.
// A sample is f32 (FMT 0) or packed little-endian integer PCM (FMT MTR_PCM_S16 / _S24 / _S32, include/mtr_engine.h).  The conversion is
// exact by construction: the sample is placed in the TOP bits of an int32 (S16 << 16, S24 << 8: at most 24 significant bits, so
// v_cvt_f32_i32 does not round), S32 is the conversion itself (round to nearest even), and the scale is one multiply by 2^-31.  Every
// function returns the f32 BIT PATTERN: f32 samples move as they are (a NaN keeps its payload), and a kernel that stores floats casts
// the bits back.  The host definition of the same arithmetic is mtr_setup_pcm_decode (mtr_setup.c).
#ifndef MTR_SAMPLE_H
#define MTR_SAMPLE_H

#include <hip/hip_runtime.h>

#include "mtr_engine.h"

constexpr float SAMPLE_SCALE = 0x1p-31f;      // of a sample in the top bits of an int32

template <int FMT> constexpr uint32_t sample_bytes () { return FMT == MTR_PCM_S16 ? 2 : FMT == MTR_PCM_S24 ? 3 : 4; }

__device__ __forceinline__ uint32_t top_bits (uint32_t top) { return __float_as_uint ((float) (int32_t) top * SAMPLE_SCALE); }

// one sample from global memory: integers from single bytes (any alignment), f32 from its dword
template <int FMT> __device__ __forceinline__ uint32_t sample_bytewise (const uint8_t* p)
{
	if constexpr (FMT == 0) return *reinterpret_cast<const uint32_t*> (p);
	else if constexpr (FMT == MTR_PCM_S16) return top_bits (((uint32_t) p[0] << 16) | ((uint32_t) p[1] << 24));
	else if constexpr (FMT == MTR_PCM_S24) return top_bits (((uint32_t) p[0] << 8) | ((uint32_t) p[1] << 16) | ((uint32_t) p[2] << 24));
	else return top_bits ((uint32_t) p[0] | ((uint32_t) p[1] << 8) | ((uint32_t) p[2] << 16) | ((uint32_t) p[3] << 24));
}

// ... and one that lies on its natural alignment (k_pick's staged tile in LDS: S24 has none, and is read byte by byte here too)
template <int FMT> __device__ __forceinline__ uint32_t sample_aligned (const uint8_t* p)
{
	if constexpr (FMT == 0) return *reinterpret_cast<const uint32_t*> (p);
	else if constexpr (FMT == MTR_PCM_S16) return top_bits ((uint32_t) *reinterpret_cast<const uint16_t*> (p) << 16);
	else if constexpr (FMT == MTR_PCM_S24) return sample_bytewise<FMT> (p);
	else return top_bits (*reinterpret_cast<const uint32_t*> (p));
}

// Four consecutive samples from the dwords of one vector load.  S16: two dwords, a sample in each half
__device__ __forceinline__ void four_s16 (uint32_t x, uint32_t y, uint32_t (&v)[4])
{
	v[0] = top_bits (x << 16); v[1] = top_bits (x & 0xffff0000u); v[2] = top_bits (y << 16); v[3] = top_bits (y & 0xffff0000u);
}
// S24: three dwords a b c, bytes a0 a1 a2 | a3 b0 b1 | b2 b3 c0 | c1 c2 c3, each sample moved to the top three bytes of a dword
// (v_alignbyte across the dword seams)
__device__ __forceinline__ void four_s24 (uint32_t a, uint32_t b, uint32_t c, uint32_t (&v)[4])
{
	v[0] = top_bits (a << 8);
	v[1] = top_bits (__builtin_amdgcn_alignbyte (b, a, 2) & 0xffffff00u);
	v[2] = top_bits (__builtin_amdgcn_alignbyte (c, b, 1) & 0xffffff00u);
	v[3] = top_bits (c & 0xffffff00u);
}
// S32: four dwords, the conversion itself
__device__ __forceinline__ void four_s32 (uint4 w, uint32_t (&v)[4])
{
	v[0] = top_bits (w.x); v[1] = top_bits (w.y); v[2] = top_bits (w.z); v[3] = top_bits (w.w);
}

#endif
