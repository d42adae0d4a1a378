// mtr_pcm.hip — k_pcm: rows of packed little-endian integer PCM (MTR_PCM_S16 / S24 / S32, include/mtr_engine.h) to rows of f32.
//
// One row per stream: n samples (frames x channels, interleaved as the meters expect them) from `src + row * src_pitch` bytes to
// `dst + row * dst_pitch` floats.  A pure streaming kernel: a row is cut into TILES of TILE samples, a workgroup takes one tile
// at a time (so that a chunk of few long rows fills the chip as well as one of many short rows), and inside a tile lane t of the
// workgroup takes PIECES t, t + 256, ...: the lanes of a wave cover consecutive 16-byte pieces of the row.
//   aligned row (source and destination row start on 16 bytes: every row the engine stages itself):
//     S16  one 16-byte load  ->  8 samples -> two 16-byte stores
//     S24  three 16-byte loads = 48 bytes -> 16 samples (v_alignbyte across the dword seams) -> four 16-byte stores
//     S32  one 16-byte load  ->  4 samples -> one 16-byte store
//     and the samples behind the row's last whole piece one by one, from single bytes;
//   any other row (mtr_engine_process_device_pcm on a caller's rows: S16 on any even byte, S24 on any byte): every sample from
//     single bytes, one dword store each.  Correct first: the fast path is the staged one.
// The conversion is exact by construction: the sample is placed in the TOP bits of an int32 (S16 << 16, S24 << 8: at most 24
// significant bits, so v_cvt_f32_i32 does not round), S32 is the conversion itself (round to nearest even), and the scale is
// one multiply by 2^-31.  Bounds: a vector piece lies wholly in front of the row's last sample, a single sample is guarded by
// i < n: no byte at or behind n * bytes-per-sample of a row is read, no float at or behind n written.
#include <hip/hip_runtime.h>

#include "mtr_internal.h"

namespace {

constexpr uint32_t PCM_THREADS = 256;
constexpr uint32_t PCM_TILE = 8192;          // samples per tile: 16 KB of S16, 24 KB of S24, 32 KB of S32 in; 32 KB out
constexpr float    PCM_SCALE = 0x1p-31f;     // of a sample in the top bits of an int32

template <int FMT> struct Pcm;
template <> struct Pcm<MTR_PCM_S16> { static constexpr uint32_t BYTES = 2, PIECE = 8; };    // samples per piece
template <> struct Pcm<MTR_PCM_S24> { static constexpr uint32_t BYTES = 3, PIECE = 16; };
template <> struct Pcm<MTR_PCM_S32> { static constexpr uint32_t BYTES = 4, PIECE = 4; };

__device__ __forceinline__ float top_to_f32 (uint32_t top) { return (float) (int32_t) top * PCM_SCALE; }

// one sample from single bytes (any alignment)
template <int FMT> __device__ __forceinline__ float pcm_one (const uint8_t* p)
{
	if constexpr (FMT == MTR_PCM_S16) return top_to_f32 (((uint32_t) p[0] << 16) | ((uint32_t) p[1] << 24));
	else if constexpr (FMT == MTR_PCM_S24) return top_to_f32 (((uint32_t) p[0] << 8) | ((uint32_t) p[1] << 16) | ((uint32_t) p[2] << 24));
	else return top_to_f32 ((uint32_t) p[0] | ((uint32_t) p[1] << 8) | ((uint32_t) p[2] << 16) | ((uint32_t) p[3] << 24));
}

// the dwords of one piece -> its floats
template <int FMT> struct Piece;
template <> struct Piece<MTR_PCM_S16> {
	uint4 w;
	__device__ __forceinline__ void load (const uint4* s) { w = s[0]; }
	__device__ __forceinline__ void store (float4* d) const
	{
		d[0] = make_float4 (top_to_f32 (w.x << 16), top_to_f32 (w.x & 0xffff0000u), top_to_f32 (w.y << 16), top_to_f32 (w.y & 0xffff0000u));
		d[1] = make_float4 (top_to_f32 (w.z << 16), top_to_f32 (w.z & 0xffff0000u), top_to_f32 (w.w << 16), top_to_f32 (w.w & 0xffff0000u));
	}
};
template <> struct Piece<MTR_PCM_S32> {
	uint4 w;
	__device__ __forceinline__ void load (const uint4* s) { w = s[0]; }
	__device__ __forceinline__ void store (float4* d) const { d[0] = make_float4 (top_to_f32 (w.x), top_to_f32 (w.y), top_to_f32 (w.z), top_to_f32 (w.w)); }
};
template <> struct Piece<MTR_PCM_S24> {
	uint4 w[3];
	__device__ __forceinline__ void load (const uint4* s) { w[0] = s[0]; w[1] = s[1]; w[2] = s[2]; }
	// four samples = three dwords a b c: bytes a0 a1 a2 | a3 b0 b1 | b2 b3 c0 | c1 c2 c3, each moved to the top three bytes of a dword
	static __device__ __forceinline__ float4 four (uint32_t a, uint32_t b, uint32_t c)
	{
		return make_float4 (top_to_f32 (a << 8),
		                    top_to_f32 (__builtin_amdgcn_alignbyte (b, a, 2) & 0xffffff00u),
		                    top_to_f32 (__builtin_amdgcn_alignbyte (c, b, 1) & 0xffffff00u),
		                    top_to_f32 (c & 0xffffff00u));
	}
	__device__ __forceinline__ void store (float4* d) const
	{
		d[0] = four (w[0].x, w[0].y, w[0].z);
		d[1] = four (w[0].w, w[1].x, w[1].y);
		d[2] = four (w[1].z, w[1].w, w[2].x);
		d[3] = four (w[2].y, w[2].z, w[2].w);
	}
};

template <int FMT>
__global__ __launch_bounds__ (PCM_THREADS) void k_pcm (const uint8_t* __restrict__ src, uint64_t src_pitch, float* __restrict__ dst, uint64_t dst_pitch,
                                                       uint32_t n_rows, uint64_t n, uint32_t tiles_per_row)
{
	using P = Pcm<FMT>;
	constexpr uint32_t PER_TILE = PCM_TILE / P::PIECE;           // pieces per tile
	constexpr uint32_t UNROLL = PER_TILE / PCM_THREADS;          // ... and per lane: 4 (S16), 2 (S24), 8 (S32)
	static_assert (PER_TILE % PCM_THREADS == 0, "a tile is whole rounds of the workgroup");
	const uint64_t n_units = (uint64_t) n_rows * tiles_per_row;
	const uint64_t n_pieces = n / P::PIECE;                      // whole pieces of a row
	for (uint64_t u = blockIdx.x; u < n_units; u += gridDim.x) {
		const uint32_t row = (uint32_t) (u / tiles_per_row), tile = (uint32_t) (u % tiles_per_row);
		const uint8_t* const s = src + (uint64_t) row * src_pitch;
		float* const d = dst + (uint64_t) row * dst_pitch;
		const uint64_t i0 = (uint64_t) tile * PCM_TILE;            // first sample of the tile
		if ((((uintptr_t) s | (uintptr_t) d) & 15) == 0) {
			const uint64_t p0 = (uint64_t) tile * PER_TILE + threadIdx.x;
			Piece<FMT> pc[UNROLL];
#pragma unroll
			for (uint32_t k = 0; k < UNROLL; ++k) {
				const uint64_t p = p0 + (uint64_t) k * PCM_THREADS;
				if (p < n_pieces) pc[k].load (reinterpret_cast<const uint4*> (s + p * (P::PIECE * P::BYTES)));
			}
#pragma unroll
			for (uint32_t k = 0; k < UNROLL; ++k) {
				const uint64_t p = p0 + (uint64_t) k * PCM_THREADS;
				if (p < n_pieces) pc[k].store (reinterpret_cast<float4*> (d + p * P::PIECE));
			}
			// the samples behind the last whole piece (fewer than PIECE), by the tile they fall into
			const uint64_t i = n_pieces * P::PIECE + threadIdx.x;
			if (threadIdx.x < P::PIECE && i < n && i >= i0 && i < i0 + PCM_TILE) d[i] = pcm_one<FMT> (s + i * P::BYTES);
		} else {
			const uint64_t end = i0 + PCM_TILE < n ? i0 + PCM_TILE : n;
			for (uint64_t i = i0 + threadIdx.x; i < end; i += PCM_THREADS) d[i] = pcm_one<FMT> (s + i * P::BYTES);
		}
	}
}

}   // namespace

int mtr_launch_pcm (int format, const void* src, uint64_t src_pitch, float* dst, uint64_t dst_pitch, uint32_t n_rows, uint64_t n_samples, void* stream)
{
	if (!n_rows || !n_samples) return 0;
	const uint64_t tiles = (n_samples + PCM_TILE - 1) / PCM_TILE;
	if (tiles > 0xffffffffull) return -1;
	const uint64_t units = (uint64_t) n_rows * tiles;
	const uint32_t grid = (uint32_t) (units < (1u << 20) ? units : (1u << 20));      // (the workgroups walk the rest)
	const dim3 g (grid), b (PCM_THREADS);
	const hipStream_t st = (hipStream_t) stream;
	const uint8_t* const s = (const uint8_t*) src;
	switch (format) {
	case MTR_PCM_S16: hipLaunchKernelGGL (k_pcm<MTR_PCM_S16>, g, b, 0, st, s, src_pitch, dst, dst_pitch, n_rows, n_samples, (uint32_t) tiles); break;
	case MTR_PCM_S24: hipLaunchKernelGGL (k_pcm<MTR_PCM_S24>, g, b, 0, st, s, src_pitch, dst, dst_pitch, n_rows, n_samples, (uint32_t) tiles); break;
	case MTR_PCM_S32: hipLaunchKernelGGL (k_pcm<MTR_PCM_S32>, g, b, 0, st, s, src_pitch, dst, dst_pitch, n_rows, n_samples, (uint32_t) tiles); break;
	default: return -1;
	}
	return hipGetLastError () == hipSuccess ? 0 : -1;
}
