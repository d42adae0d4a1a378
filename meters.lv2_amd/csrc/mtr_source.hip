// mtr_source.hip — the source step: a chunk's first step, the caller's bytes to the staging buffer's f32 frames.  Three kernels for the three
// forms a source takes besides resident f32 frames (mtr_decode_kind), one launcher (mtr_launch_decode), and the host side of the subsystem:
// the engine's source layout (mtr_engine_set_frame_layout / _set_plane_layout), its counters and the host definitions of the decodes
// (mtr_*_decode_host).  The sample arithmetic of all three is mtr_sample.h; the call that runs the step is CallRun::decode (mtr_call.hip).
//
// All three cut a row (a stream's part of the chunk) into TILES, a workgroup takes one tile at a time (so that a chunk of few long rows
// fills the chip as well as one of many short rows), and every row the engine stages itself starts on 16 bytes at the source and at the
// destination: that is the fast path.  Rows of a caller (the device entry points: f32 on any 4 bytes, S16 on any even byte, S24 on any
// byte) go sample by sample, one dword store each.  Correct first: the fast path is the staged one.
//
// k_pcm (MTR_DECODE_ROWS) — rows of packed integer PCM to rows of f32.  One row per stream: n samples (frames x channels, interleaved as
// the meters expect them) from `src + row * src_pitch` bytes to `dst + row * dst_pitch` floats.  Tiles of PCM_TILE samples; inside a tile
// lane t takes PIECES t, t + 256, ...: the lanes of a wave cover consecutive 16-byte pieces of the row.
//   aligned row:
//     S16  one 16-byte load  ->  8 samples -> two 16-byte stores
//     S24  three 16-byte loads = 48 bytes -> 16 samples (four_s24) -> four 16-byte stores
//     S32  one 16-byte load  ->  4 samples -> one 16-byte store
//     and the samples behind the row's last whole piece one by one, from single bytes;
//   any other row: every sample from single bytes.
// Bounds: a vector piece lies wholly in front of the row's last sample, a single sample is guarded by i < n: no byte at or behind
// n * bytes-per-sample of a row is read, no float at or behind n written.
//
// k_pick (MTR_DECODE_FRAMES) — rows of WIDE frames (fc samples each, any format) to rows of the engine's frames (C f32 each), channel c of a
// frame = source channel map[c] of the same frame.  Decode and pick in one pass; the definition it is held against is
// mtr_setup_pick_decode.  n_frames frames from `src + row * src_pitch` bytes to `dst + row * dst_pitch` floats.  Tiles of tile_frames
// frames (a multiple of 16, as many as fit PICK_LDS bytes of source: every tile of a row that starts on 16 bytes starts on 16 bytes, at
// the source and at the destination):
//   aligned row:
//     1. the tile's source bytes into LDS as they lie, 16-byte global loads -> 16-byte LDS writes, consecutive lanes on consecutive
//        pieces; the bytes behind the row's last whole 16 (fewer than 16, last tile of the row only) one by one;
//     2. lane t takes output PIECES t, t + 256, ...: four consecutive floats of the destination row.  Float o of the tile is channel
//        c = o mod C of frame o / C (C is a template parameter: a multiply and a shift), its sample lies at (frame * fc + map[c]) in
//        LDS — the map is up to eight 4-bit fields of one SGPR, picked with a shift, so no register array is indexed by a run-time value;
//        one 16-byte store per piece; the floats behind the row's last whole piece one by one.
//   any other row: every output float from its sample's own bytes in global memory.
// Bounds: a 16-byte load lies wholly inside the tile's n * fc * bytes-per-sample source bytes, single bytes are guarded by the same
// count, a store by n * C floats: no byte at or behind n_frames * fc samples of a source row is read, no float at or behind
// n_frames * C of a destination row written.  Channels the map does not name reach LDS and are never read from there.
//
// k_plane (MTR_DECODE_PLANES) — PLANAR audio (per stream n_planes planes of one channel each, any format) to rows of the engine's
// interleaved frames, channel c of a frame = the same frame of plane map[c].  Decode and interleave in one pass (include/mtr_planes.h); the
// definition it is held against is mtr_setup_plane_decode.  Plane p of row r starts at `src + (r * n_planes + p) * plane_pitch` BYTES and
// holds n_frames samples; the row's frames go to `dst + r * dst_pitch` floats.  Tiles of PLANE_TILE frames (a multiple of 16: the tile's
// first sample lies as its plane's first does, modulo 16 bytes, in every format); inside a tile lane t takes GROUPS t, t + 256, ... of four
// consecutive frames:
//   1. per engine channel c the group's four samples of plane map[c] — ONE load where that plane starts on the load's alignment (16 bytes
//      of f32 / S32 on 16, 8 bytes of S16 on 8, 12 bytes of S24 on 4: consecutive lanes on consecutive pieces of the plane), else the four
//      samples one by one (S24 planes start on any byte); a channel whose plane is the one of the channel before it takes that channel's
//      registers instead (1, {0, 0}: the mono file);
//   2. interleaved in registers — channel and frame of every register are compile-time constants —
//   3. C 16-byte pieces: the group's 4 C floats are consecutive in the row, the lanes' pieces together cover the tile without holes.  With
//      more than one channel they go through LDS (C | 1 slots per lane, 12 – 36 KB per workgroup) so that consecutive lanes store consecutive 16 bytes.
//   The frames behind the tile's last whole group (1 .. 3, last tile of the row only; all of a call of n_frames < 4), and every frame of
//   a row whose destination does not start on 16 bytes (no row the engine stages), go float by float.
// Bounds: a group lies wholly in front of the row's n_frames (its loads read exactly 4 samples of a plane), single samples are guarded by
// the same count, a store by n_frames * C floats: no byte at or behind n_frames samples of a plane is read, no float at or behind
// n_frames * C of a destination row written.  Planes the map does not name are never read.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <utility>

#include "mtr_engine_impl.h"
#include "mtr_sample.h"

namespace {

constexpr uint32_t DECODE_THREADS = 256;
constexpr uint32_t PCM_TILE = 8192;          // samples per tile: 16 KB of S16, 24 KB of S24, 32 KB of S32 in; 32 KB out
constexpr uint32_t PICK_LDS = 32768;         // source bytes of a tile: 1024 frames of eight f32 channels, 16384 of one S16 channel
constexpr uint32_t PLANE_TILE = 4096;        // frames per tile: four groups per lane

__device__ __forceinline__ float4 as_floats (const uint32_t (&v)[4])
{
	return make_float4 (__uint_as_float (v[0]), __uint_as_float (v[1]), __uint_as_float (v[2]), __uint_as_float (v[3]));
}

// ---- k_pcm --------------------------------------------------------------------------------------------------------------------------
// the dwords of one piece -> its floats
template <int FMT> struct Piece;
template <> struct Piece<MTR_PCM_S16> {
	static constexpr uint32_t SAMPLES = 8;
	uint4 w;
	__device__ __forceinline__ void load (const uint4* s) { w = s[0]; }
	__device__ __forceinline__ void store (float4* d) const
	{
		uint32_t v[4];
		four_s16 (w.x, w.y, v); d[0] = as_floats (v);
		four_s16 (w.z, w.w, v); d[1] = as_floats (v);
	}
};
template <> struct Piece<MTR_PCM_S32> {
	static constexpr uint32_t SAMPLES = 4;
	uint4 w;
	__device__ __forceinline__ void load (const uint4* s) { w = s[0]; }
	__device__ __forceinline__ void store (float4* d) const { uint32_t v[4]; four_s32 (w, v); d[0] = as_floats (v); }
};
template <> struct Piece<MTR_PCM_S24> {
	static constexpr uint32_t SAMPLES = 16;
	uint4 w[3];
	__device__ __forceinline__ void load (const uint4* s) { w[0] = s[0]; w[1] = s[1]; w[2] = s[2]; }
	__device__ __forceinline__ void store (float4* d) const
	{
		uint32_t v[4];
		four_s24 (w[0].x, w[0].y, w[0].z, v); d[0] = as_floats (v);
		four_s24 (w[0].w, w[1].x, w[1].y, v); d[1] = as_floats (v);
		four_s24 (w[1].z, w[1].w, w[2].x, v); d[2] = as_floats (v);
		four_s24 (w[2].y, w[2].z, w[2].w, v); d[3] = as_floats (v);
	}
};

template <int FMT>
__global__ __launch_bounds__ (DECODE_THREADS) void k_pcm (const uint8_t* __restrict__ src, uint64_t src_pitch, float* __restrict__ dst, uint64_t dst_pitch,
                                                          uint32_t n_rows, uint64_t n, uint32_t tiles_per_row)
{
	constexpr uint32_t B = sample_bytes<FMT> (), PIECE = Piece<FMT>::SAMPLES;
	constexpr uint32_t PER_TILE = PCM_TILE / PIECE;              // pieces per tile
	constexpr uint32_t UNROLL = PER_TILE / DECODE_THREADS;       // ... and per lane: 4 (S16), 2 (S24), 8 (S32)
	static_assert (PER_TILE % DECODE_THREADS == 0, "a tile is whole rounds of the workgroup");
	const uint64_t n_units = (uint64_t) n_rows * tiles_per_row;
	const uint64_t n_pieces = n / PIECE;                         // whole pieces of a row
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
				const uint64_t p = p0 + (uint64_t) k * DECODE_THREADS;
				if (p < n_pieces) pc[k].load (reinterpret_cast<const uint4*> (s + p * (PIECE * B)));
			}
#pragma unroll
			for (uint32_t k = 0; k < UNROLL; ++k) {
				const uint64_t p = p0 + (uint64_t) k * DECODE_THREADS;
				if (p < n_pieces) pc[k].store (reinterpret_cast<float4*> (d + p * PIECE));
			}
			// the samples behind the last whole piece (fewer than PIECE), by the tile they fall into
			const uint64_t i = n_pieces * PIECE + threadIdx.x;
			if (threadIdx.x < PIECE && i < n && i >= i0 && i < i0 + PCM_TILE) d[i] = __uint_as_float (sample_bytewise<FMT> (s + i * B));
		} else {
			const uint64_t end = i0 + PCM_TILE < n ? i0 + PCM_TILE : n;
			for (uint64_t i = i0 + threadIdx.x; i < end; i += DECODE_THREADS) d[i] = __uint_as_float (sample_bytewise<FMT> (s + i * B));
		}
	}
}

// ---- k_pick -------------------------------------------------------------------------------------------------------------------------
// byte offset, inside a run of frames, of output float o: channel o mod C of frame o / C
template <int FMT, uint32_t C> __device__ __forceinline__ uint32_t sample_at (uint32_t o, uint32_t fc, uint32_t map)
{
	const uint32_t fr = o / C, c = o - fr * C;
	return (fr * fc + ((map >> (4 * c)) & 15u)) * sample_bytes<FMT> ();
}

template <int FMT, uint32_t C>
__global__ __launch_bounds__ (DECODE_THREADS) void k_pick (const uint8_t* __restrict__ src, uint64_t src_pitch, uint32_t* __restrict__ dst, uint64_t dst_pitch,
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
			for (uint32_t p = threadIdx.x; p < np; p += DECODE_THREADS) tile_lds[p] = reinterpret_cast<const uint4*> (st)[p];
			{
				const uint32_t i = 16 * np + threadIdx.x;
				if (threadIdx.x < 16 && i < nb) lb[i] = st[i];
			}
			__syncthreads ();
			const uint32_t nq = no / 4;
			for (uint32_t q = threadIdx.x; q < nq; q += DECODE_THREADS) {
				uint4 v;
				v.x = sample_aligned<FMT> (lb + sample_at<FMT, C> (4 * q, fc, map));
				v.y = sample_aligned<FMT> (lb + sample_at<FMT, C> (4 * q + 1, fc, map));
				v.z = sample_aligned<FMT> (lb + sample_at<FMT, C> (4 * q + 2, fc, map));
				v.w = sample_aligned<FMT> (lb + sample_at<FMT, C> (4 * q + 3, fc, map));
				reinterpret_cast<uint4*> (dt)[q] = v;
			}
			{
				const uint32_t o = 4 * nq + threadIdx.x;
				if (threadIdx.x < 4 && o < no) dt[o] = sample_aligned<FMT> (lb + sample_at<FMT, C> (o, fc, map));
			}
			__syncthreads ();                                                                   // (the next tile overwrites the staged one)
		} else {
			for (uint32_t o = threadIdx.x; o < no; o += DECODE_THREADS) dt[o] = sample_bytewise<FMT> (st + sample_at<FMT, C> (o, fc, map));
		}
	}
}

// ---- k_plane ------------------------------------------------------------------------------------------------------------------------
// what the one load of a group needs of its plane's first byte
template <int FMT> constexpr uint32_t group_align () { return FMT == MTR_PCM_S16 ? 8 : FMT == MTR_PCM_S24 ? 4 : 16; }

struct Dwords3 { uint32_t a, b, c; };          // 12 bytes on 4: four S24 samples

// four consecutive samples of a plane from ONE load (p on group_align<FMT> ())
template <int FMT> __device__ __forceinline__ void four_samples (const uint8_t* p, uint32_t (&v)[4])
{
	if constexpr (FMT == 0) {
		const uint4 w = *reinterpret_cast<const uint4*> (p);
		v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
	} else if constexpr (FMT == MTR_PCM_S32) {
		four_s32 (*reinterpret_cast<const uint4*> (p), v);
	} else if constexpr (FMT == MTR_PCM_S16) {
		const uint2 w = *reinterpret_cast<const uint2*> (p);
		four_s16 (w.x, w.y, v);
	} else {
		const Dwords3 w = *reinterpret_cast<const Dwords3*> (p);
		four_s24 (w.a, w.b, w.c, v);
	}
}

template <int FMT, uint32_t C>
__global__ __launch_bounds__ (DECODE_THREADS) void k_plane (const uint8_t* __restrict__ src, uint64_t plane_pitch, uint32_t n_planes, uint32_t map,
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
	__shared__ uint4 pieces[THROUGH_LDS ? DECODE_THREADS * SLOTS : 1];
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
		for (uint32_t q0 = 0; q0 < nq; q0 += DECODE_THREADS) {                                  // a ROUND: the workgroup's next 256 groups (the last one of a row fewer)
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
						for (uint32_t j = 0; j < 4; ++j) v[c][j] = sample_bytewise<FMT> (pl[c] + ((size_t) q * 4 + j) * B);
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
				const uint32_t np = (nq - q0 < DECODE_THREADS ? nq - q0 : DECODE_THREADS) * C;
				__syncthreads ();
				for (uint32_t p = threadIdx.x; p < np; p += DECODE_THREADS) {
					const uint32_t g = p / C, k = p - g * C;
					reinterpret_cast<uint4*> (dt)[(size_t) q0 * C + p] = pieces[g * SLOTS + k];
				}
				__syncthreads ();                                                               // (the next round overwrites the pieces)
			}
		}
		// the floats behind the last whole group, one by one
		const uint32_t no = nf * C;
		for (uint32_t o = 4 * nq * C + threadIdx.x; o < no; o += DECODE_THREADS) {
			const uint32_t fr = o / C, c = o - fr * C;
			dt[o] = sample_bytewise<FMT> (s + (uint64_t) ((map >> (4 * c)) & 15u) * plane_pitch + (size_t) fr * B);
		}
	}
}

// f (std::integral_constant<int, I>) for the I of the list that `v` is; false: it is none of them
template <int... I, typename F> bool with_constant (int v, std::integer_sequence<int, I...>, F&& f)
{
	return ((v == I && (f (std::integral_constant<int, I> {}), true)) || ...);
}

}   // namespace

int mtr_launch_decode (const mtr_decode_args& a)
{
	if (!a.n_rows || !a.n_frames) return 0;
	const bool rows = a.kind == MTR_DECODE_ROWS;
	const size_t sb = a.format ? mtr_setup_pcm_sample_bytes (a.format) : rows ? 0 : sizeof (float);   // (rows of f32 are the meters' own: nothing to decode)
	if (!sb || !a.n_channels || a.n_channels > MTR_MAX_ENGINE_CHANNELS) return -1;
	uint32_t map = 0;                                                                      // up to eight 4-bit fields
	if (!rows) {
		if (!a.width || a.width > MTR_MAX_FRAME_CHANNELS) return -1;
		for (uint32_t c = 0; c < a.n_channels; ++c) {
			if (a.map[c] >= a.width) return -1;
			map |= (uint32_t) a.map[c] << (4 * c);
		}
	}
	// what a row counts (k_pcm: samples; frames otherwise) and how many of them a tile holds
	uint64_t n = a.n_frames, tile = 0;
	switch (a.kind) {
	case MTR_DECODE_ROWS:   n *= a.n_channels; tile = PCM_TILE; break;
	case MTR_DECODE_FRAMES: tile = (uint32_t) (PICK_LDS / (a.width * sb)) & ~15u; break;           // >= 1024 frames
	case MTR_DECODE_PLANES: if (a.pitch < n * sb) return -1; tile = PLANE_TILE; break;
	default: return -1;
	}
	const uint64_t tiles = (n + tile - 1) / tile;
	if (tiles > 0xffffffffull) return -1;
	const uint64_t units = (uint64_t) a.n_rows * tiles;
	const dim3 g ((uint32_t) (units < (1u << 20) ? units : (1u << 20))), b (DECODE_THREADS);       // (the workgroups walk the rest)
	const hipStream_t st = (hipStream_t) a.stream;
	const uint8_t* const s = (const uint8_t*) a.src;
	uint32_t* const d = reinterpret_cast<uint32_t*> (a.dst);
	const uint32_t tpr = (uint32_t) tiles;
	using Formats = std::integer_sequence<int, 0, MTR_PCM_S16, MTR_PCM_S24, MTR_PCM_S32>;
	using Channels = std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7, 8>;
	// (format, channels) as compile-time constants, once: 32 k_plane, 32 k_pick, 3 k_pcm (which has no f32 form and takes any channels)
	const bool known = with_constant (a.format, Formats {}, [&] (auto format) {
		with_constant ((int) a.n_channels, Channels {}, [&] (auto channels) {
			constexpr int FMT = decltype (format)::value;
			constexpr uint32_t C = decltype (channels)::value;
			if (a.kind == MTR_DECODE_PLANES)
				hipLaunchKernelGGL ((k_plane<FMT, C>), g, b, 0, st, s, a.pitch, a.width, map, d, a.dst_pitch, a.n_rows, a.n_frames, tpr);
			else if (a.kind == MTR_DECODE_FRAMES)
				hipLaunchKernelGGL ((k_pick<FMT, C>), g, b, 0, st, s, a.pitch, d, a.dst_pitch, a.n_rows, a.n_frames, a.width, map, (uint32_t) tile, tpr);
			else if constexpr (FMT != 0)
				hipLaunchKernelGGL (k_pcm<FMT>, g, b, 0, st, s, a.pitch, a.dst, a.dst_pitch, a.n_rows, n, tpr);
		});
	});
	return known && hipGetLastError () == hipSuccess ? 0 : -1;
}

// ---- the engine's source layout -------------------------------------------------------------------------------------------------------
// What both setters are: `width` samples per frame (MTR_DECODE_FRAMES) or planes per stream (MTR_DECODE_PLANES), engine channel c = entry
// map[c] of them; width 0: the default.  `who`, `what`: the setter's and its width's names in the error texts.  A refused call changes
// nothing; an accepted one replaces the whole layout (frames or planes: the two exclude each other).
static int set_layout (mtr_engine* e, mtr_decode_kind kind, uint32_t width, const uint8_t* map, const char* who, const char* what)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	const uint32_t C = e->cfg.n_channels;
	SourceLayout lay;
	if (width) {
		char text[96];
		const char* bad = nullptr;
		bool identity = kind == MTR_DECODE_FRAMES && width == C;
		if (width > MTR_MAX_FRAME_CHANNELS) bad = "%s: %s > MTR_MAX_FRAME_CHANNELS";
		else if (!map) bad = "%s: null map";
		for (uint32_t c = 0; !bad && c < C; ++c) {
			if (map[c] >= width) bad = "%s: a map entry >= %s";
			identity = identity && map[c] == c;
			lay.map[c] = map[c];
		}
		if (bad) { snprintf (text, sizeof (text), bad, who, what); return fail (MTR_ERR_ARG, text); }
		lay.kind = identity ? MTR_DECODE_NONE : kind;                   // (the explicit identity is the default and takes its paths)
		lay.width = width;
		lay.wave51 = kind == MTR_DECODE_FRAMES && e->layout == 8 && C == 5 && width == 6 && map[0] == 0 && map[1] == 1 && map[2] == 2 && map[3] == 4 && map[4] == 5;
	}
	e->src = lay;
	return MTR_OK;
}

// what a getter reads back of `kind`: the layout if it is of that kind, else the identity on `width`
static void get_layout (const mtr_engine* e, mtr_decode_kind kind, uint32_t width, uint32_t* out_width, uint8_t* map)
{
	const bool own = e->src.kind == kind;
	if (out_width) *out_width = own ? e->src.width : width;
	if (map) for (uint32_t c = 0; c < e->cfg.n_channels; ++c) map[c] = own ? e->src.map[c] : (uint8_t) c;
}

extern "C" {

int mtr_engine_set_frame_layout (mtr_engine* e, uint32_t frame_channels, const uint8_t* map)
{
	return set_layout (e, MTR_DECODE_FRAMES, frame_channels, map, "mtr_engine_set_frame_layout", "frame_channels");
}

int mtr_engine_set_plane_layout (mtr_engine* e, uint32_t n_planes, const uint8_t* map)
{
	return set_layout (e, MTR_DECODE_PLANES, n_planes, map, "mtr_engine_set_plane_layout", "n_planes");
}

int mtr_engine_frame_layout (const mtr_engine* e, uint32_t* frame_channels, uint8_t* map)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	get_layout (e, MTR_DECODE_FRAMES, e->cfg.n_channels, frame_channels, map);
	return MTR_OK;
}

int mtr_engine_plane_layout (const mtr_engine* e, uint32_t* n_planes, uint8_t* map)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	get_layout (e, MTR_DECODE_PLANES, 0, n_planes, map);
	return MTR_OK;
}

int mtr_engine_layout_stats (mtr_engine* e, uint64_t* staged_chunks, uint64_t* direct_calls)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	if (staged_chunks) *staged_chunks = e->lay_staged;
	if (direct_calls) *direct_calls = e->lay_direct;
	return MTR_OK;
}

int mtr_engine_plane_stats (mtr_engine* e, uint64_t* staged_chunks)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	if (staged_chunks) *staged_chunks = e->plane_staged;
	return MTR_OK;
}

int mtr_engine_pcm_stats (mtr_engine* e, uint64_t* chunks, uint64_t* bytes, float* decode_ms)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	if (e->pcm_timed) {
		const int rc = mtr_engine_sync (e);
		if (rc) return rc;
		for (uint32_t i = 0; i < e->pcm_timed && (size_t) 2 * i + 1 < e->pcm_ev.size (); ++i) {
			float ms;
			if (hipEventElapsedTime (&ms, e->pcm_ev[2 * i].v, e->pcm_ev[2 * i + 1].v) == hipSuccess) e->pcm_ms += ms;
		}
		e->pcm_timed = 0;
	}
	if (chunks) *chunks = e->pcm_chunks;
	if (bytes) *bytes = e->pcm_bytes;
	if (decode_ms) *decode_ms = e->pcm_ms;
	return MTR_OK;
}

size_t mtr_pcm_sample_bytes (int format) { return mtr_setup_pcm_sample_bytes (format); }

// ---- the host definitions the kernels are held against (mtr_setup.c), behind the C ABI's checks ---------------------------------------
int mtr_pcm_decode_host (int format, const void* src, size_t n_samples, float* dst)
{
	if (!mtr_setup_pcm_sample_bytes (format)) return fail (MTR_ERR_ARG, "unknown PCM format (MTR_PCM_S16, _S24, _S32)");
	if (n_samples && (!src || !dst)) return fail (MTR_ERR_ARG, "mtr_pcm_decode_host: null argument");
	return mtr_setup_pcm_decode (format, src, n_samples, dst) ? fail (MTR_ERR_ARG, "mtr_pcm_decode_host") : MTR_OK;
}

int mtr_pick_decode_host (int format, const void* src, size_t n_frames, uint32_t frame_channels, const uint8_t* map, uint32_t n_channels, float* dst)
{
	if (format && !mtr_setup_pcm_sample_bytes (format)) return fail (MTR_ERR_ARG, "unknown format (0 = f32, MTR_PCM_S16, _S24, _S32)");
	if (!map || !frame_channels || frame_channels > MTR_MAX_FRAME_CHANNELS || !n_channels || n_channels > MTR_MAX_ENGINE_CHANNELS)
		return fail (MTR_ERR_ARG, "mtr_pick_decode_host: map / frame_channels / n_channels");
	if (n_frames && (!src || !dst)) return fail (MTR_ERR_ARG, "mtr_pick_decode_host: null argument");
	return mtr_setup_pick_decode (format, src, n_frames, frame_channels, map, n_channels, dst)
	       ? fail (MTR_ERR_ARG, "mtr_pick_decode_host: a map entry >= frame_channels") : MTR_OK;
}

int mtr_plane_decode_host (int format, const void* src, size_t n_frames, uint64_t stride_frames, uint32_t n_planes, const uint8_t* map, uint32_t n_channels,
                           float* dst)
{
	if (format && !mtr_setup_pcm_sample_bytes (format)) return fail (MTR_ERR_ARG, "unknown format (0 = f32, MTR_PCM_S16, _S24, _S32)");
	if (!map || !n_planes || n_planes > MTR_MAX_FRAME_CHANNELS || !n_channels || n_channels > MTR_MAX_ENGINE_CHANNELS)
		return fail (MTR_ERR_ARG, "mtr_plane_decode_host: map / n_planes / n_channels");
	if (stride_frames < n_frames) return fail (MTR_ERR_ARG, "mtr_plane_decode_host: stride_frames < n_frames");
	if (n_frames && (!src || !dst)) return fail (MTR_ERR_ARG, "mtr_plane_decode_host: null argument");
	return mtr_setup_plane_decode (format, src, n_frames, stride_frames, n_planes, map, n_channels, dst)
	       ? fail (MTR_ERR_ARG, "mtr_plane_decode_host: a map entry >= n_planes") : MTR_OK;
}

} // extern "C"
