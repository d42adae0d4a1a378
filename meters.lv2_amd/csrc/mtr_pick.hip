// mtr_pick.hip — k_pick: rows of WIDE frames (frame_channels samples each: f32, or packed little-endian integer PCM, MTR_PCM_*) to
// rows of the engine's frames (n_channels f32 each), channel c of a frame = source channel map[c] of the same frame.  Decode and pick
// in one pass (mtr_engine_set_frame_layout, include/mtr_engine.h); the definition it is held against is mtr_setup_pick_decode.
//
// One row per stream: n_frames frames from `src + row * src_pitch` bytes to `dst + row * dst_pitch` floats.  A row is cut into TILES
// of tile_frames frames (a multiple of 16, as many as fit PICK_LDS bytes of source: every tile of a row that starts on 16 bytes
// starts on 16 bytes, at the source and at the destination), a workgroup takes one tile at a time:
//   aligned row (source and destination row start on 16 bytes: every row the engine stages itself):
//     1. the tile's source bytes into LDS as they lie, 16-byte global loads -> 16-byte LDS writes, consecutive lanes on consecutive
//        pieces; the bytes behind the row's last whole 16 (fewer than 16, last tile of the row only) one by one;
//     2. lane t takes output PIECES t, t + 256, ...: four consecutive floats of the destination row.  Float o of the tile is channel
//        c = o mod C of frame o / C (C is a template parameter: a multiply and a shift), its sample lies at (frame * fc + map[c]) in
//        LDS — the map is up to eight 4-bit fields of one SGPR, picked with a shift, so no register array is indexed by a run-time value —
//        and is decoded exactly as k_pcm does (the sample in the top bits of an int32, one conversion, one exact scale; f32 samples
//        move as bit patterns); one 16-byte store per piece; the floats behind the row's last whole piece one by one.
//   any other row (the device entry points on a caller's rows: f32 on any 4 bytes, S16 on any even byte, S24 on any byte): every
//     output float from its sample's own bytes in global memory, one dword store each.  Correct first: the fast path is the staged one.
// Bounds: a 16-byte load lies wholly inside the tile's n * fc * bytes-per-sample source bytes, single bytes are guarded by the same
// count, a store by n * C floats: no byte at or behind n_frames * fc samples of a source row is read, no float at or behind
// n_frames * C of a destination row written.  Channels the map does not name reach LDS and are never read from there.
#include <hip/hip_runtime.h>

#include "mtr_internal.h"

namespace {

constexpr uint32_t PICK_THREADS = 256;
constexpr uint32_t PICK_LDS = 32768;         // source bytes of a tile: 1024 frames of eight f32 channels, 16384 of one S16 channel
constexpr float    PICK_SCALE = 0x1p-31f;    // of a sample in the top bits of an int32

template <int FMT> constexpr uint32_t sample_bytes () { return FMT == MTR_PCM_S16 ? 2 : FMT == MTR_PCM_S24 ? 3 : 4; }

__device__ __forceinline__ uint32_t top_bits (uint32_t top) { return __float_as_uint ((float) (int32_t) top * PICK_SCALE); }

// the f32 bit pattern of one sample, from LDS (the sample's natural alignment inside the staged tile: the tile starts on 16 bytes) ...
template <int FMT> __device__ __forceinline__ uint32_t one_lds (const uint8_t* p)
{
	if constexpr (FMT == 0) return *reinterpret_cast<const uint32_t*> (p);
	else if constexpr (FMT == MTR_PCM_S16) return top_bits ((uint32_t) *reinterpret_cast<const uint16_t*> (p) << 16);
	else if constexpr (FMT == MTR_PCM_S24) return top_bits (((uint32_t) p[0] << 8) | ((uint32_t) p[1] << 16) | ((uint32_t) p[2] << 24));
	else return top_bits (*reinterpret_cast<const uint32_t*> (p));
}

// ... and from global memory, integers from single bytes (any alignment), f32 from its dword
template <int FMT> __device__ __forceinline__ uint32_t one_global (const uint8_t* p)
{
	if constexpr (FMT == 0) return *reinterpret_cast<const uint32_t*> (p);
	else if constexpr (FMT == MTR_PCM_S16) return top_bits (((uint32_t) p[0] << 16) | ((uint32_t) p[1] << 24));
	else if constexpr (FMT == MTR_PCM_S24) return top_bits (((uint32_t) p[0] << 8) | ((uint32_t) p[1] << 16) | ((uint32_t) p[2] << 24));
	else return top_bits ((uint32_t) p[0] | ((uint32_t) p[1] << 8) | ((uint32_t) p[2] << 16) | ((uint32_t) p[3] << 24));
}

// byte offset, inside a run of frames, of output float o: channel o mod C of frame o / C
template <int FMT, uint32_t C> __device__ __forceinline__ uint32_t sample_at (uint32_t o, uint32_t fc, uint32_t map)
{
	const uint32_t fr = o / C, c = o - fr * C;
	return (fr * fc + ((map >> (4 * c)) & 15u)) * sample_bytes<FMT> ();
}

template <int FMT, uint32_t C>
__global__ __launch_bounds__ (PICK_THREADS) void k_pick (const uint8_t* __restrict__ src, uint64_t src_pitch, uint32_t* __restrict__ dst, uint64_t dst_pitch,
                                                         uint32_t n_rows, uint64_t n_frames, uint32_t fc, uint32_t map, uint32_t tile_frames,
                                                         uint32_t tiles_per_row)
{
	constexpr uint32_t B = sample_bytes<FMT> ();
	__shared__ uint4 tile_lds[PICK_LDS / 16];
	uint8_t* const lb = reinterpret_cast<uint8_t*> (tile_lds);
	const uint64_t n_units = (uint64_t) n_rows * tiles_per_row;
	for (uint64_t u = blockIdx.x; u < n_units; u += gridDim.x) {
		const uint32_t row = (uint32_t) (u / tiles_per_row), tile = (uint32_t) (u % tiles_per_row);
		const uint8_t* const s = src + (uint64_t) row * src_pitch;
		uint32_t* const d = dst + (uint64_t) row * dst_pitch;
		const uint64_t f0 = (uint64_t) tile * tile_frames;                                     // first frame of the tile
		const uint32_t nf = (uint32_t) (n_frames - f0 < tile_frames ? n_frames - f0 : tile_frames);
		const uint32_t no = nf * C;                                                             // floats the tile writes
		const uint8_t* const st = s + f0 * fc * B;
		uint32_t* const dt = d + f0 * C;
		if ((((uintptr_t) s | (uintptr_t) d) & 15) == 0) {
			const uint32_t nb = nf * fc * B;                                                    // source bytes of the tile (<= PICK_LDS)
			const uint32_t np = nb / 16;
			for (uint32_t p = threadIdx.x; p < np; p += PICK_THREADS) tile_lds[p] = reinterpret_cast<const uint4*> (st)[p];
			{
				const uint32_t i = 16 * np + threadIdx.x;
				if (threadIdx.x < 16 && i < nb) lb[i] = st[i];
			}
			__syncthreads ();
			const uint32_t nq = no / 4;
			for (uint32_t q = threadIdx.x; q < nq; q += PICK_THREADS) {
				uint4 v;
				v.x = one_lds<FMT> (lb + sample_at<FMT, C> (4 * q, fc, map));
				v.y = one_lds<FMT> (lb + sample_at<FMT, C> (4 * q + 1, fc, map));
				v.z = one_lds<FMT> (lb + sample_at<FMT, C> (4 * q + 2, fc, map));
				v.w = one_lds<FMT> (lb + sample_at<FMT, C> (4 * q + 3, fc, map));
				reinterpret_cast<uint4*> (dt)[q] = v;
			}
			{
				const uint32_t o = 4 * nq + threadIdx.x;
				if (threadIdx.x < 4 && o < no) dt[o] = one_lds<FMT> (lb + sample_at<FMT, C> (o, fc, map));
			}
			__syncthreads ();                                                                   // (the next tile overwrites the staged one)
		} else {
			for (uint32_t o = threadIdx.x; o < no; o += PICK_THREADS) dt[o] = one_global<FMT> (st + sample_at<FMT, C> (o, fc, map));
		}
	}
}

template <int FMT>
int launch_fmt (uint32_t C, dim3 g, hipStream_t st, const uint8_t* s, uint64_t sp, uint32_t* d, uint64_t dp, uint32_t n_rows, uint64_t n_frames,
                uint32_t fc, uint32_t map, uint32_t tf, uint32_t tiles)
{
	const dim3 b (PICK_THREADS);
	switch (C) {
	case 1: hipLaunchKernelGGL ((k_pick<FMT, 1>), g, b, 0, st, s, sp, d, dp, n_rows, n_frames, fc, map, tf, tiles); break;
	case 2: hipLaunchKernelGGL ((k_pick<FMT, 2>), g, b, 0, st, s, sp, d, dp, n_rows, n_frames, fc, map, tf, tiles); break;
	case 3: hipLaunchKernelGGL ((k_pick<FMT, 3>), g, b, 0, st, s, sp, d, dp, n_rows, n_frames, fc, map, tf, tiles); break;
	case 4: hipLaunchKernelGGL ((k_pick<FMT, 4>), g, b, 0, st, s, sp, d, dp, n_rows, n_frames, fc, map, tf, tiles); break;
	case 5: hipLaunchKernelGGL ((k_pick<FMT, 5>), g, b, 0, st, s, sp, d, dp, n_rows, n_frames, fc, map, tf, tiles); break;
	case 6: hipLaunchKernelGGL ((k_pick<FMT, 6>), g, b, 0, st, s, sp, d, dp, n_rows, n_frames, fc, map, tf, tiles); break;
	case 7: hipLaunchKernelGGL ((k_pick<FMT, 7>), g, b, 0, st, s, sp, d, dp, n_rows, n_frames, fc, map, tf, tiles); break;
	case 8: hipLaunchKernelGGL ((k_pick<FMT, 8>), g, b, 0, st, s, sp, d, dp, n_rows, n_frames, fc, map, tf, tiles); break;
	default: return -1;
	}
	return hipGetLastError () == hipSuccess ? 0 : -1;
}

}   // namespace

int mtr_launch_pick (int format, const void* src, uint64_t src_pitch, uint32_t frame_channels, const uint8_t* map, uint32_t n_channels,
                     float* dst, uint64_t dst_pitch, uint32_t n_rows, uint64_t n_frames, void* stream)
{
	if (!n_rows || !n_frames) return 0;
	if (!frame_channels || frame_channels > MTR_MAX_FRAME_CHANNELS || !n_channels || n_channels > MTR_MAX_ENGINE_CHANNELS) return -1;
	const size_t sb = format ? mtr_setup_pcm_sample_bytes (format) : sizeof (float);
	if (!sb) return -1;
	uint32_t mbits = 0;
	for (uint32_t c = 0; c < n_channels; ++c) {
		if (map[c] >= frame_channels) return -1;
		mbits |= (uint32_t) map[c] << (4 * c);
	}
	const uint32_t tf = (uint32_t) (PICK_LDS / (frame_channels * sb)) & ~15u;              // >= 1024 frames
	const uint64_t tiles = (n_frames + tf - 1) / tf;
	if (tiles > 0xffffffffull) return -1;
	const uint64_t units = (uint64_t) n_rows * tiles;
	const dim3 g ((uint32_t) (units < (1u << 20) ? units : (1u << 20)));                   // (the workgroups walk the rest)
	const hipStream_t st = (hipStream_t) stream;
	const uint8_t* const s = (const uint8_t*) src;
	uint32_t* const d = reinterpret_cast<uint32_t*> (dst);
	switch (format) {
	case 0:           return launch_fmt<0> (n_channels, g, st, s, src_pitch, d, dst_pitch, n_rows, n_frames, frame_channels, mbits, tf, (uint32_t) tiles);
	case MTR_PCM_S16: return launch_fmt<MTR_PCM_S16> (n_channels, g, st, s, src_pitch, d, dst_pitch, n_rows, n_frames, frame_channels, mbits, tf, (uint32_t) tiles);
	case MTR_PCM_S24: return launch_fmt<MTR_PCM_S24> (n_channels, g, st, s, src_pitch, d, dst_pitch, n_rows, n_frames, frame_channels, mbits, tf, (uint32_t) tiles);
	case MTR_PCM_S32: return launch_fmt<MTR_PCM_S32> (n_channels, g, st, s, src_pitch, d, dst_pitch, n_rows, n_frames, frame_channels, mbits, tf, (uint32_t) tiles);
	default: return -1;
	}
}
