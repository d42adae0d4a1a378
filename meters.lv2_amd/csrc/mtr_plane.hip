// mtr_plane.hip — k_plane: PLANAR audio (per stream n_planes planes of one channel each: f32, or packed little-endian integer PCM,
// MTR_PCM_*) to rows of the engine's interleaved frames (n_channels f32 each), channel c of a frame = the same frame of plane map[c].
// Decode and interleave in one pass (mtr_engine_set_plane_layout, include/mtr_planes.h); the definition it is held against is
// mtr_setup_plane_decode.
//
// Plane p of row (stream) r starts at `src + (r * n_planes + p) * plane_pitch` BYTES and holds n_frames samples; the row's frames go to
// `dst + r * dst_pitch` floats.  A row is cut into TILES of PLANE_TILE frames (a multiple of 16: the tile's first sample lies as its
// plane's first does, modulo 16 bytes, in every format), a workgroup takes one tile at a time, and inside a tile lane t takes GROUPS
// t, t + 256, ... of four consecutive frames:
//   1. per engine channel c the group's four samples of plane map[c] — ONE load where that plane starts on the load's alignment (16 bytes
//      of f32 / S32 on 16, 8 bytes of S16 on 8, 12 bytes of S24 on 4: consecutive lanes on consecutive pieces of the plane), else the four
//      samples one by one (f32 from its dword, integers from single bytes: S24 planes start on any byte); a channel whose plane is the one
//      of the channel before it takes that channel's registers instead (1, {0, 0}: the mono file);
//   2. decoded exactly as k_pcm does (the sample in the top bits of an int32, one conversion, one exact scale; f32 samples move as bit
//      patterns) and interleaved in registers — channel and frame of every register are compile-time constants, C is a template
//      parameter, the map is up to eight 4-bit fields of one SGPR —
//   3. C 16-byte pieces: the group's 4 C floats are consecutive in the row, the lanes' pieces together cover the tile without holes.  With
//      more than one channel they go through LDS (C | 1 slots per lane, 12 – 36 KB per workgroup) so that consecutive lanes store consecutive 16 bytes.
//   The frames behind the tile's last whole group (1 .. 3, last tile of the row only; all of a call of n_frames < 4), and every frame of
//   a row whose destination does not start on 16 bytes (no row the engine stages), go float by float, one dword store each.
// Bounds: a group lies wholly in front of the row's n_frames (its loads read exactly 4 samples of a plane), single samples are guarded by
// the same count, a store by n_frames * C floats: no byte at or behind n_frames samples of a plane is read, no float at or behind
// n_frames * C of a destination row written.  Planes the map does not name are never read.
#include <hip/hip_runtime.h>

#include "mtr_internal.h"

namespace {

constexpr uint32_t PLANE_THREADS = 256;
constexpr uint32_t PLANE_TILE = 4096;         // frames per tile: four groups per lane
constexpr float    PLANE_SCALE = 0x1p-31f;    // of a sample in the top bits of an int32

template <int FMT> constexpr uint32_t sample_bytes () { return FMT == MTR_PCM_S16 ? 2 : FMT == MTR_PCM_S24 ? 3 : 4; }
// what the one load of a group needs of its plane's first byte
template <int FMT> constexpr uint32_t group_align () { return FMT == MTR_PCM_S16 ? 8 : FMT == MTR_PCM_S24 ? 4 : 16; }

__device__ __forceinline__ uint32_t top_bits (uint32_t top) { return __float_as_uint ((float) (int32_t) top * PLANE_SCALE); }

// the f32 bit pattern of one sample: integers from single bytes (any alignment), f32 from its dword
template <int FMT> __device__ __forceinline__ uint32_t one_sample (const uint8_t* p)
{
	if constexpr (FMT == 0) return *reinterpret_cast<const uint32_t*> (p);
	else if constexpr (FMT == MTR_PCM_S16) return top_bits (((uint32_t) p[0] << 16) | ((uint32_t) p[1] << 24));
	else if constexpr (FMT == MTR_PCM_S24) return top_bits (((uint32_t) p[0] << 8) | ((uint32_t) p[1] << 16) | ((uint32_t) p[2] << 24));
	else return top_bits ((uint32_t) p[0] | ((uint32_t) p[1] << 8) | ((uint32_t) p[2] << 16) | ((uint32_t) p[3] << 24));
}

struct Dwords3 { uint32_t a, b, c; };          // 12 bytes on 4: four S24 samples

// four consecutive samples of a plane from ONE load (p on group_align<FMT> ())
template <int FMT> __device__ __forceinline__ void four_samples (const uint8_t* p, uint32_t (&v)[4])
{
	if constexpr (FMT == 0) {
		const uint4 w = *reinterpret_cast<const uint4*> (p);
		v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
	} else if constexpr (FMT == MTR_PCM_S32) {
		const uint4 w = *reinterpret_cast<const uint4*> (p);
		v[0] = top_bits (w.x); v[1] = top_bits (w.y); v[2] = top_bits (w.z); v[3] = top_bits (w.w);
	} else if constexpr (FMT == MTR_PCM_S16) {
		const uint2 w = *reinterpret_cast<const uint2*> (p);
		v[0] = top_bits (w.x << 16); v[1] = top_bits (w.x & 0xffff0000u); v[2] = top_bits (w.y << 16); v[3] = top_bits (w.y & 0xffff0000u);
	} else {
		// three dwords a b c: bytes a0 a1 a2 | a3 b0 b1 | b2 b3 c0 | c1 c2 c3, each sample moved to the top three bytes of a dword (k_pcm)
		const Dwords3 w = *reinterpret_cast<const Dwords3*> (p);
		v[0] = top_bits (w.a << 8);
		v[1] = top_bits (__builtin_amdgcn_alignbyte (w.b, w.a, 2) & 0xffffff00u);
		v[2] = top_bits (__builtin_amdgcn_alignbyte (w.c, w.b, 1) & 0xffffff00u);
		v[3] = top_bits (w.c & 0xffffff00u);
	}
}

template <int FMT, uint32_t C>
__global__ __launch_bounds__ (PLANE_THREADS) void k_plane (const uint8_t* __restrict__ src, uint64_t plane_pitch, uint32_t n_planes, uint32_t map,
                                                           uint32_t* __restrict__ dst, uint64_t dst_pitch, uint32_t n_rows, uint64_t n_frames,
                                                           uint32_t tiles_per_row)
{
	constexpr uint32_t B = sample_bytes<FMT> ();
	// A lane's C pieces lie 16 C bytes from its neighbour's: stored from the registers, one store instruction of a wave touches 64 pieces
	// 16 C bytes apart.  Through LDS instead (C > 1): the lane parks its pieces in a row of SLOTS 16-byte slots (odd: the lanes' rows spread
	// over the banks), and the workgroup stores the round's pieces in row order.  Measured against the stores from the registers, which
	// fall from 5.2 TB/s at two channels to 2.9 at eight (profiles/r40_planes.md), and kept.  One channel needs no reordering.
	constexpr bool THROUGH_LDS = C > 1;
	constexpr uint32_t SLOTS = C | 1u;
	__shared__ uint4 pieces[THROUGH_LDS ? PLANE_THREADS * SLOTS : 1];
	const uint64_t n_units = (uint64_t) n_rows * tiles_per_row;
	for (uint64_t u = blockIdx.x; u < n_units; u += gridDim.x) {
		const uint32_t row = (uint32_t) (u / tiles_per_row), tile = (uint32_t) (u % tiles_per_row);
		const uint64_t f0 = (uint64_t) tile * PLANE_TILE;                                       // first frame of the tile
		const uint32_t nf = (uint32_t) (n_frames - f0 < PLANE_TILE ? n_frames - f0 : PLANE_TILE);
		const uint8_t* const s = src + (uint64_t) row * n_planes * plane_pitch + f0 * B;        // the tile's first sample in plane 0 of the row
		uint32_t* const d = dst + (uint64_t) row * dst_pitch;
		uint32_t* const dt = d + f0 * C;
		// (f0 * B and f0 * C * 4 are multiples of 16: a tile lies as its plane and its row do)
		const uint32_t nq = ((uintptr_t) d & 15) == 0 ? nf / 4 : 0;                             // whole groups of the tile
		const uint8_t* pl[C];
#pragma unroll
		for (uint32_t c = 0; c < C; ++c) pl[c] = s + (uint64_t) ((map >> (4 * c)) & 15u) * plane_pitch;
		for (uint32_t q0 = 0; q0 < nq; q0 += PLANE_THREADS) {                                   // a ROUND: the workgroup's next 256 groups (the last one of a row fewer)
			const uint32_t q = q0 + threadIdx.x;
			if (q < nq) {
				uint32_t v[C][4];
#pragma unroll
				for (uint32_t c = 0; c < C; ++c) {
					bool again = false;
					if constexpr (C > 1) again = c > 0 && pl[c] == pl[c ? c - 1 : 0];
					if (again) {
#pragma unroll
						for (uint32_t j = 0; j < 4; ++j) v[c][j] = v[c ? c - 1 : 0][j];
					} else if (((uintptr_t) pl[c] & (group_align<FMT> () - 1)) == 0) {
						four_samples<FMT> (pl[c] + (size_t) q * (4 * B), v[c]);
					} else {
#pragma unroll
						for (uint32_t j = 0; j < 4; ++j) v[c][j] = one_sample<FMT> (pl[c] + ((size_t) q * 4 + j) * B);
					}
				}
#pragma unroll
				for (uint32_t k = 0; k < C; ++k) {                                              // floats 4 k .. 4 k + 3 of the group: channel o mod C of frame o / C
					uint4 o;
					o.x = v[(4 * k) % C][(4 * k) / C];
					o.y = v[(4 * k + 1) % C][(4 * k + 1) / C];
					o.z = v[(4 * k + 2) % C][(4 * k + 2) / C];
					o.w = v[(4 * k + 3) % C][(4 * k + 3) / C];
					if constexpr (THROUGH_LDS) pieces[threadIdx.x * SLOTS + k] = o;
					else reinterpret_cast<uint4*> (dt)[(size_t) q * C + k] = o;
				}
			}
			if constexpr (THROUGH_LDS) {
				// the round's pieces lie in the row in the order (group, k): lane t now takes pieces t, t + 256, ... of the round — consecutive
				// lanes store consecutive 16 bytes
				const uint32_t np = (nq - q0 < PLANE_THREADS ? nq - q0 : PLANE_THREADS) * C;
				__syncthreads ();
				for (uint32_t p = threadIdx.x; p < np; p += PLANE_THREADS) {
					const uint32_t g = p / C, k = p - g * C;
					reinterpret_cast<uint4*> (dt)[(size_t) q0 * C + p] = pieces[g * SLOTS + k];
				}
				__syncthreads ();                                                               // (the next round overwrites the pieces)
			}
		}
		// the floats behind the last whole group, one by one
		const uint32_t no = nf * C;
		for (uint32_t o = 4 * nq * C + threadIdx.x; o < no; o += PLANE_THREADS) {
			const uint32_t fr = o / C, c = o - fr * C;
			dt[o] = one_sample<FMT> (s + (uint64_t) ((map >> (4 * c)) & 15u) * plane_pitch + (size_t) fr * B);
		}
	}
}

template <int FMT>
int launch_fmt (uint32_t C, dim3 g, hipStream_t st, const uint8_t* s, uint64_t pp, uint32_t P, uint32_t map, uint32_t* d, uint64_t dp, uint32_t n_rows,
                uint64_t n_frames, uint32_t tiles)
{
	const dim3 b (PLANE_THREADS);
	switch (C) {
	case 1: hipLaunchKernelGGL ((k_plane<FMT, 1>), g, b, 0, st, s, pp, P, map, d, dp, n_rows, n_frames, tiles); break;
	case 2: hipLaunchKernelGGL ((k_plane<FMT, 2>), g, b, 0, st, s, pp, P, map, d, dp, n_rows, n_frames, tiles); break;
	case 3: hipLaunchKernelGGL ((k_plane<FMT, 3>), g, b, 0, st, s, pp, P, map, d, dp, n_rows, n_frames, tiles); break;
	case 4: hipLaunchKernelGGL ((k_plane<FMT, 4>), g, b, 0, st, s, pp, P, map, d, dp, n_rows, n_frames, tiles); break;
	case 5: hipLaunchKernelGGL ((k_plane<FMT, 5>), g, b, 0, st, s, pp, P, map, d, dp, n_rows, n_frames, tiles); break;
	case 6: hipLaunchKernelGGL ((k_plane<FMT, 6>), g, b, 0, st, s, pp, P, map, d, dp, n_rows, n_frames, tiles); break;
	case 7: hipLaunchKernelGGL ((k_plane<FMT, 7>), g, b, 0, st, s, pp, P, map, d, dp, n_rows, n_frames, tiles); break;
	case 8: hipLaunchKernelGGL ((k_plane<FMT, 8>), g, b, 0, st, s, pp, P, map, d, dp, n_rows, n_frames, tiles); break;
	default: return -1;
	}
	return hipGetLastError () == hipSuccess ? 0 : -1;
}

}   // namespace

int mtr_launch_plane (int format, const void* src, uint64_t plane_pitch, uint32_t n_planes, const uint8_t* map, uint32_t n_channels,
                      float* dst, uint64_t dst_pitch, uint32_t n_rows, uint64_t n_frames, void* stream)
{
	if (!n_rows || !n_frames) return 0;
	if (!n_planes || n_planes > MTR_MAX_FRAME_CHANNELS || !n_channels || n_channels > MTR_MAX_ENGINE_CHANNELS) return -1;
	const size_t sb = format ? mtr_setup_pcm_sample_bytes (format) : sizeof (float);
	if (!sb || plane_pitch < n_frames * sb) return -1;
	uint32_t mbits = 0;
	for (uint32_t c = 0; c < n_channels; ++c) {
		if (map[c] >= n_planes) return -1;
		mbits |= (uint32_t) map[c] << (4 * c);
	}
	const uint64_t tiles = (n_frames + PLANE_TILE - 1) / PLANE_TILE;
	if (tiles > 0xffffffffull) return -1;
	const uint64_t units = (uint64_t) n_rows * tiles;
	const dim3 g ((uint32_t) (units < (1u << 20) ? units : (1u << 20)));                   // (the workgroups walk the rest)
	const hipStream_t st = (hipStream_t) stream;
	const uint8_t* const s = (const uint8_t*) src;
	uint32_t* const d = reinterpret_cast<uint32_t*> (dst);
	switch (format) {
	case 0:           return launch_fmt<0> (n_channels, g, st, s, plane_pitch, n_planes, mbits, d, dst_pitch, n_rows, n_frames, (uint32_t) tiles);
	case MTR_PCM_S16: return launch_fmt<MTR_PCM_S16> (n_channels, g, st, s, plane_pitch, n_planes, mbits, d, dst_pitch, n_rows, n_frames, (uint32_t) tiles);
	case MTR_PCM_S24: return launch_fmt<MTR_PCM_S24> (n_channels, g, st, s, plane_pitch, n_planes, mbits, d, dst_pitch, n_rows, n_frames, (uint32_t) tiles);
	case MTR_PCM_S32: return launch_fmt<MTR_PCM_S32> (n_channels, g, st, s, plane_pitch, n_planes, mbits, d, dst_pitch, n_rows, n_frames, (uint32_t) tiles);
	default: return -1;
	}
}
