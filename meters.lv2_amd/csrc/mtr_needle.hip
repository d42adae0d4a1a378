// mtr_needle.hip — the needle meters (Vumeterdsp, Iec1ppmdsp, Iec2ppmdsp, Msppmdsp: the VU, DIN / Nordic, BBC / EBU and BBC M6 plugins'
// detectors) for a batch, with a reading series (gfx950).
//
// Replaces Iec1ppmdsp::process = Iec2ppmdsp::process (jmeters/iec1ppmdsp.cc:47-80, iec2ppmdsp.cc:47-80), Msppmdsp::processM / processS
// (msppmdsp.cc:50-114) and Vumeterdsp::process (vumeterdsp.cc:45-73), and their read ().  Per group of four frames a PPM does
//     z1 *= w3, z2 *= w3;  four times: t = |x| (M/S: mv |l +- r|), if (t > z1) z1 += w1 (t - z1), if (t > z2) z2 += w2 (t - z2);
//     t = z1 + z2, if (t > m) m = t
// between a clamp of z1, z2 to [0, 20] at the start of a process () and a + 1e-10f at its end; the VU
//     t2 = z2 / 2;  four times: t1 = |x| - t2, z1 += w (t1 - z1);  z2 += 4 w (z1 - z2), if (z2 > m) m = z2
// between a clamp to [-20, 20] and, at the end, the flush of a z that is not finite (to 0, with m = INFINITY), z2 + 1e-10f otherwise.
// The n mod 4 trailing frames of a process () are dropped.  One process () is the engine call, or — with a period P, for the reading
// series — every block of exactly P frames, wherever the calls cut the audio; read () = g m follows each such block.
//
// The attack is not linear (it is a max of two affine maps, as k_tpb's), so there is no weighted-sum form: a chain per
// (stream, channel, filter), serial in time, parallel over the streams only.  Being a plain serial chain it does the reference's own f32
// operations in the reference's own order — this file is compiled without FMA contraction and without fast-math, f32 subnormals are kept
// — and the readings and states are bit for bit the reference's (tests/test_gpu_needle.py).  The comparisons are written as there: a NaN
// sample loses every one of them and is ignored, an Inf sticks until the end of the process () and is clamped at the start of the next.
//
// Lane map.  A workgroup takes 32 / C streams (16 stereo, 32 mono) and has four waves, one per selected kind — a wave without a kind
// only helps to stage — so code and constants are wave-uniform and the audio is read from HBM ONCE however many kinds run.  A PPM wave's lane is (stream, channel, filter): the two
// attack filters of a detector sit in neighbouring lanes and z1 + z2 is formed across the pair (DPP) once per group — half the chain
// of a lane that runs both.  The VU's two stages are coupled: lane = (stream, channel), half the wave.  The streams advance in lock
// step, so where a group or a period stands is the same in every lane: all of the control flow is scalar.
//
// Staging.  The waves of a workgroup stage chunks of 256 frames per stream through two LDS buffers by 16-byte loads from addresses
// that are multiples of 16 — whatever the row's own alignment: each row is fetched from the aligned quad in front of the chunk, so an odd
// stride or an odd base only shifts where the quads land; the chunks at a call's ends, whose quads could reach outside the call's
// frames, are fetched dword by dword — with the next chunk in flight in registers under the chain.  A row is padded by one frame: the
// chain lanes read the same frame of 16 (32) different rows, 2 (1) banks apart.  State lives in registers across the call; a period's
// end inside a chunk is handled in the chain: the end-of-block constants, the point, m = 0, the P mod 4 frames skipped, the clamp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "mtr_engine_impl.h"

/* a detector: per (stream, selected kind, channel).  z1 z2 m are where the chain stands — inside a period the locals of the open
 * process () — s1 s2 what the most recent completed process () stored, `last` the reading of the last completed period */
typedef struct mtr_needle_state {
	float    z1, z2, m, last, s1, s2;
	uint32_t res;                 /* _res: read () has taken the maximum, the next process () starts a new one (period 0) */
	uint32_t pad;
} mtr_needle_state;

/* in front of a stream's detectors: what the state blob needs of the engine (the host's copies rule; export writes them in) */
typedef struct mtr_needle_hdr {
	uint32_t kinds, period, fill, pad;
	float    db[2], mv[2];
} mtr_needle_hdr;

typedef struct mtr_needle_args {
	const float*    audio;        /* [S][stride][C] */
	uint64_t        stride, n_frames;
	uint32_t        n_streams, n_kinds;
	uint32_t        kind[4];      /* the kind of wave i */
	float           w[4][4];      /* ... and its w1 w2 w3 g (VU: w, 4 w, 0, g) */
	float           mv[2];        /* Msppmdsp's gains: M, S */
	uint32_t        period;       /* frames per process (): P, or the call's n_frames */
	uint32_t        fill;         /* frames into the open period on entry */
	uint32_t        series;       /* P > 0: read () after every period, appended to the series */
	uint32_t        capacity;
	uint64_t        point0;       /* periods completed before this call */
	unsigned char*  state;        /* [S] of { mtr_needle_hdr, mtr_needle_state [n_kinds][C] } */
	uint32_t        state_pitch;
	float*          points;       /* [n_kinds][..][capacity][C], from the view's first stream */
	uint64_t        kind_pitch;   /* floats from kind to kind */
	/* the LEN instantiation only (`back` set): */
	const uint32_t* ends;         /* [S] per-stream ends of a ragged call, or NULL: every stream takes the whole call */
	float*          back;         /* [S][n_kinds][C][2] z1 z2 where the group of four frames stood that is open between two calls */
} mtr_needle_args;

namespace {

constexpr int CH = 256;                  // frames per staged chunk
constexpr int NW = 4;                    // waves per workgroup: one per selected kind runs a chain, all of them stage

template <int C> struct Geo {
	static constexpr int NS = 32 / C;            // streams per workgroup
	static constexpr int ROW = CH * C;           // dwords of a row's chunk
	static constexpr int PITCH = ROW + C;        // ... padded by one frame
	static constexpr int NQ = ROW / 4 + 1;       // aligned quads that cover a chunk starting at any of the four alignments
	static constexpr int ITEMS = NS * NQ;
};

__device__ __forceinline__ float pair_other (float v)
{
	return __int_as_float (__builtin_amdgcn_update_dpp (0, __float_as_int (v), 0xB1, 0xF, 0xF, true));   // quad_perm [1, 0, 3, 2]
}

// Iec1ppmdsp / Iec2ppmdsp / Msppmdsp: lane = (row, filter)
// (BACK: the chain keeps what z was in front of a group it entered frame by frame — the group a call may end in)
template <int C, bool MS, bool BACK> struct Ppm {
	float z, m, s, last, w, w3, g, mv, zb;
	uint32_t res, sgn;
	int   base;                                  // the lane's dword in a staged frame 0
	bool  series;

	using Raw = std::conditional_t<MS, float2, float>;
	struct Quad { Raw r[4]; };

	__device__ __forceinline__ Raw raw (const float* buf, int k) const
	{
		if constexpr (MS) return *reinterpret_cast<const float2*> (buf + base + 2 * k);
		else return buf[base + k * C];
	}
	__device__ __forceinline__ Quad load (const float* buf, int k) const { return Quad{{ raw (buf, k), raw (buf, k + 1), raw (buf, k + 2), raw (buf, k + 3) }}; }
	__device__ __forceinline__ float val (Raw x) const
	{
		if constexpr (MS) return mv * fabsf (x.x + __uint_as_float (__float_as_uint (x.y) ^ sgn));         // l + r, l - r
		else return fabsf (x);
	}
	__device__ __forceinline__ void start ()
	{
		z = z > 20 ? 20 : (z < 0 ? 0 : z);
		m = series || res ? 0 : m;
		res = 0;
	}
	template <bool FIRST, bool LAST> __device__ __forceinline__ void one (Raw x)
	{
		const float t = val (x);
		if (FIRST) z *= w3;
		if (t > z) z += w * (t - z);
		if (LAST) {
			const float u = z + pair_other (z);
			if (u > m) m = u;
		}
	}
	__device__ __forceinline__ void step (const float* buf, int k, int q)
	{
		if (q == 0) { if constexpr (BACK) zb = z; one<true, false> (raw (buf, k)); }
		else if (q == 3) one<false, true> (raw (buf, k));
		else one<false, false> (raw (buf, k));
	}
	__device__ __forceinline__ void group (const Quad& x)
	{
		one<true, false> (x.r[0]); one<false, false> (x.r[1]); one<false, false> (x.r[2]); one<false, true> (x.r[3]);
	}
	__device__ __forceinline__ void undo () { z = zb; }          // the open group never happened
	__device__ __forceinline__ float end ()
	{
		z = z + 1e-10f;
		s = z;
		if (series) last = g * m;
		return last;
	}
};

// Vumeterdsp: lane = row
template <int C, bool BACK> struct Vu {
	float z1, z2, t2, m, s1, s2, last, w, w4, g, zb;
	uint32_t res;
	int   base;
	bool  series;

	__device__ __forceinline__ void start ()
	{
		z1 = z1 > 20 ? 20 : (z1 < -20 ? -20 : z1);
		z2 = z2 > 20 ? 20 : (z2 < -20 ? -20 : z2);
		m = series || res ? 0 : m;
		res = 0;
	}
	struct Quad { float r[4]; };
	__device__ __forceinline__ float raw (const float* buf, int k) const { return buf[base + k * C]; }
	__device__ __forceinline__ Quad load (const float* buf, int k) const { return Quad{{ raw (buf, k), raw (buf, k + 1), raw (buf, k + 2), raw (buf, k + 3) }}; }
	template <bool FIRST, bool LAST> __device__ __forceinline__ void one (float x)
	{
		if (FIRST) t2 = z2 / 2;
		const float t1 = fabsf (x) - t2;
		z1 += w * (t1 - z1);
		if (LAST) {
			z2 += w4 * (z1 - z2);
			if (z2 > m) m = z2;
		}
	}
	__device__ __forceinline__ void step (const float* buf, int k, int q)
	{
		if (q == 0) { if constexpr (BACK) zb = z1; one<true, false> (raw (buf, k)); }
		else if (q == 3) one<false, true> (raw (buf, k));
		else one<false, false> (raw (buf, k));
	}
	__device__ __forceinline__ void group (const Quad& x)
	{
		one<true, false> (x.r[0]); one<false, false> (x.r[1]); one<false, false> (x.r[2]); one<false, true> (x.r[3]);
	}
	__device__ __forceinline__ void undo () { z1 = zb; }         // (z2 and m move with a group's last frame only)
	__device__ __forceinline__ float end ()
	{
		if (!isfinite (z1)) { z1 = 0; m = INFINITY; }
		if (!isfinite (z2)) { z2 = 0; m = INFINITY; } else z2 = z2 + 1e-10f;
		s1 = z1; s2 = z2;
		if (series) last = g * m;
		return last;
	}
};

// where the lock-step streams stand in the period, and what happens at its ends: scalar
struct Walk {
	uint32_t j, P, P4;                           // frames into the period, its length, the frames of it that are kept
	uint64_t point;
};

// the `nf` staged frames of a chunk through a chain; `put (reading, point)` stores a point of the series
template <class Chain, class Put>
__device__ __forceinline__ void walk (Chain& c, Walk& w, const float* buf, int nf, Put put)
{
	int k = 0;
	while (k < nf) {
		if (w.j == 0) c.start ();
		if (w.j < w.P4) {
			int run = (int) min ((uint32_t) (nf - k), w.P4 - w.j);
			int q = (int) (w.j & 3);
			w.j += (uint32_t) run;
			for (; run > 0 && q; --run, ++k, q = (q + 1) & 3) c.step (buf, k, q);
			for (; run >= 16; run -= 16, k += 16) {  // four groups: their LDS reads issued together, one exposed wait per 16 frames
				const typename Chain::Quad x0 = c.load (buf, k), x1 = c.load (buf, k + 4), x2 = c.load (buf, k + 8), x3 = c.load (buf, k + 12);
				c.group (x0); c.group (x1); c.group (x2); c.group (x3);
			}
			for (; run >= 4; run -= 4, k += 4) c.group (c.load (buf, k));
			for (; run > 0; --run, ++k, ++q) c.step (buf, k, q);
		} else {                                 // the P mod 4 frames at the period's end: dropped
			const uint32_t skip = min ((uint32_t) (nf - k), w.P - w.j);
			k += (int) skip; w.j += skip;
		}
		if (w.j == w.P) {
			const float r = c.end ();
			if (c.series) put (r, w.point);
			++w.point;
			w.j = 0;
		}
	}
}

// A chunk of a ragged call in which not every lane of the wave takes every frame.  The lock-step walk stays scalar — where a block starts
// and ends is the same for every stream that is still open — and a lane joins what its stream has of it: `lim` frames of the chunk's
// `nf` (0: the stream ended in an earlier chunk, or was closed before the call); `closing`: the stream ends at chunk frame lim, inside
// the call.  The block it ends in is truncated there: the frames from its j & ~3 on are dropped, then the chain's own end () and its
// point, at the index of the open block.  A stream that ends exactly where a block does has completed it and gets nothing more.
// A group that the chunk's first frames continue — the chain entered it frame by frame, in the chunk or the call before — and that the
// lane's end leaves incomplete is undone: the chain kept what stood in front of it.
// The lanes that share a stream (a detector's two filters, its channels) share lim: the pair sum sees both or neither.
template <class Chain, class Put>
__device__ __forceinline__ void walk_ragged (Chain& c, Walk& w, const float* buf, int nf, int lim, bool closing, Put put)
{
	int k = 0;
	if (closing && w.j < w.P4 && (w.j & 3u) && (uint32_t) lim < 4u - (w.j & 3u)) c.undo ();
	while (k < nf) {
		const int ka = k;
		if (w.j == 0 && lim > k) c.start ();
		// the lane's frames of this block end at chunk frame `keep`: its end, less the frames behind the last whole group, if the block holds it
		int keep = lim;
		if (closing && lim > k && (uint32_t) (lim - k) <= w.P - w.j) keep = lim - (int) ((w.j + (uint32_t) (lim - k)) & 3u);
		if (w.j < w.P4) {
			int run = (int) min ((uint32_t) (nf - k), w.P4 - w.j);
			int q = (int) (w.j & 3);
			w.j += (uint32_t) run;
			for (; run > 0 && q; --run, ++k, q = (q + 1) & 3) if (k < keep) c.step (buf, k, q);
			for (; run >= 16; run -= 16, k += 16) {
				if (k + 16 <= keep) {
					const typename Chain::Quad x0 = c.load (buf, k), x1 = c.load (buf, k + 4), x2 = c.load (buf, k + 8), x3 = c.load (buf, k + 12);
					c.group (x0); c.group (x1); c.group (x2); c.group (x3);
				} else {
					for (int g = 0; g < 16; g += 4) if (k + g + 4 <= keep) c.group (c.load (buf, k + g));
				}
			}
			for (; run >= 4; run -= 4, k += 4) if (k + 4 <= keep) c.group (c.load (buf, k));
			for (; run > 0; --run, ++k, ++q) if (k < keep) c.step (buf, k, q);
		} else {
			const uint32_t skip = min ((uint32_t) (nf - k), w.P - w.j);
			k += (int) skip; w.j += skip;
		}
		// the block's end — every lane that had frames of [ka, k) — or, for a closing lane, its own end inside them
		const bool done = w.j == w.P;
		if (done ? lim > ka : (closing && lim > ka && lim <= k)) {
			const float r = c.end ();
			if (c.series) put (r, w.point);
		}
		if (done) { ++w.point; w.j = 0; }
	}
}

// LEN: stream s ends at call frame a.ends[s] (0: not touched; no ends: every stream takes the whole call).  The workgroup runs to the
// last end it holds — every wave, the helpers too, derives that from the same at most 32 ends, so they meet at the same barriers — and
// fetches nothing at or past it.  It is also the kernel of every call that ends inside a group of four frames: what stood in front of
// that group goes to a.back, for a stream that a later call ends before the group is complete.
template <int C, bool LEN>
__global__ __launch_bounds__ (64 * NW) void k_needle (const mtr_needle_args a)
{
	using G = Geo<C>;
	constexpr int NT = 64 * NW, PER = (G::ITEMS + NT - 1) / NT;
	__shared__ float lds[2][G::NS * G::PITCH];

	const int tid = threadIdx.x, lane = tid & 63;
	const int wid = __builtin_amdgcn_readfirstlane (tid >> 6);
	const uint32_t s0 = blockIdx.x * G::NS;
	int64_t last_end = (int64_t) a.n_frames;                           // frames the workgroup walks: the call's, or (LEN) up to the last end it holds
	if (LEN && a.ends) {
		uint32_t m = 0;
		for (int i = 0; i < G::NS; ++i) {                              // (uniform: the same scalar loads in every wave)
			const uint32_t si = s0 + (uint32_t) i;
			const uint32_t v = si < a.n_streams ? a.ends[si] : 0u;
			m = v > m ? v : m;
		}
		last_end = (int64_t) __builtin_amdgcn_readfirstlane ((int) m);
		if (last_end == 0) return;                                     // (the whole workgroup, before any barrier)
	}
	const int64_t rowlen = last_end * C;                              // dwords of a row that belong to the call
	const bool al4 = (reinterpret_cast<size_t> (a.audio) & 3) == 0;
	const uint64_t abase = reinterpret_cast<size_t> (a.audio) >> 2;

	// ---- staging: item i = (row, aligned quad) ----
	float4 pre[PER];
	auto place = [&] (int i, int64_t T, int& r, int64_t& d) __attribute__ ((always_inline)) -> bool {
		r = i / G::NQ;
		const int q = i - r * G::NQ;
		const uint32_t s = s0 + (uint32_t) r;
		if (i >= G::ITEMS || s >= a.n_streams) return false;
		const uint64_t row = (uint64_t) s * a.stride * C;
		const int al = (int) ((abase + row + (uint64_t) T * C) & 3);   // dwords from the aligned quad to the chunk's first
		d = T * C - al + 4 * q;                                        // the quad's first dword in the row
		return true;
	};
	// (a chunk whose quads all lie inside the call's frames, whatever the rows' alignment — every chunk but a call's first and its
	// last two at most, the same for all lanes — is fetched by 16-byte loads alone: a load that shares its registers with the careful
	// path's would be waited for where it is issued)
	auto fetch = [&] (int64_t T) __attribute__ ((always_inline)) {
		if (al4 && T > 0 && (T + CH) * C + 3 < rowlen) {
#pragma unroll
			for (int j = 0; j < PER; ++j) {
				int r; int64_t d;
				float4 v = float4{0.f, 0.f, 0.f, 0.f};
				if (place (tid + j * NT, T, r, d)) v = *reinterpret_cast<const float4*> (a.audio + (uint64_t) (s0 + (uint32_t) r) * a.stride * C + d);
				pre[j] = v;
			}
		} else {
#pragma unroll
			for (int j = 0; j < PER; ++j) {
				int r; int64_t d;
				float4 v = float4{0.f, 0.f, 0.f, 0.f};
				if (place (tid + j * NT, T, r, d)) {
					const float* const p = a.audio + (uint64_t) (s0 + (uint32_t) r) * a.stride * C;
					if (d >= 0 && d < rowlen) v.x = p[d];
					if (d + 1 >= 0 && d + 1 < rowlen) v.y = p[d + 1];
					if (d + 2 >= 0 && d + 2 < rowlen) v.z = p[d + 2];
					if (d + 3 >= 0 && d + 3 < rowlen) v.w = p[d + 3];
				}
				pre[j] = v;
			}
		}
	};
	auto stash = [&] (int b, int64_t T) __attribute__ ((always_inline)) {
#pragma unroll
		for (int j = 0; j < PER; ++j) {
			int r; int64_t d;
			if (place (tid + j * NT, T, r, d)) {
				const int o = (int) (d - T * C);                           // -3 .. ROW
				float* const dst = &lds[b][r * G::PITCH];
				if (o >= 0 && o + 3 < G::ROW) { dst[o] = pre[j].x; dst[o + 1] = pre[j].y; dst[o + 2] = pre[j].z; dst[o + 3] = pre[j].w; }
				else {
					if (o >= 0 && o < G::ROW) dst[o] = pre[j].x;
					if (o + 1 >= 0 && o + 1 < G::ROW) dst[o + 1] = pre[j].y;
					if (o + 2 >= 0 && o + 2 < G::ROW) dst[o + 2] = pre[j].z;
					if (o + 3 >= 0 && o + 3 < G::ROW) dst[o + 3] = pre[j].w;
				}
			}
		}
	};

	// ---- the chains ----
	const uint32_t kind = a.kind[wid < (int) a.n_kinds ? wid : 0];
	const bool vu = kind == MTR_NEEDLE_VU;
	const int row = vu ? (lane & 31) : (lane >> 1);
	const int filt = lane & 1;
	const int sl = row / C, ch = row % C;
	const uint32_t s = s0 + (uint32_t) sl;
	const bool live = s < a.n_streams;
	bool writer = live && (vu ? lane < 32 : true);
	if (LEN && a.ends) writer = writer && a.ends[live ? s : 0] != 0;  // (end 0: the stream's detectors and its series row are not written)
	const int64_t N = last_end;
	const int64_t nchunks = (N + CH - 1) / CH;
	// LEN: the lane's own end (a lane without a stream walks as an open one would, on nothing, and writes nothing)
	int64_t E = 0;
	bool closes = false;
	float* bk = nullptr;                                               // the lane's slot of a.back
	if constexpr (LEN) {
		E = live && a.ends ? (int64_t) a.ends[s] : N;
		closes = live && E < (int64_t) a.n_frames;
	}
	if (wid >= (int) a.n_kinds) {                                      // no chain of its own: this wave only helps to stage
		fetch (0);
		for (int64_t c = 0; c < nchunks; ++c) {
			stash ((int) (c & 1), c * CH);
			__syncthreads ();
			if (c + 1 < nchunks) fetch ((c + 1) * CH);
		}
		return;
	}
	mtr_needle_state* const st = reinterpret_cast<mtr_needle_state*> (a.state + (size_t) (live ? s : 0) * a.state_pitch + sizeof (mtr_needle_hdr)) + wid * C + ch;
	float* const pts = a.points ? a.points + (size_t) wid * a.kind_pitch + (size_t) s * a.capacity * C + ch : nullptr;
	const float w1 = a.w[wid][0], w2 = a.w[wid][1], w3 = a.w[wid][2], g = a.w[wid][3];
	const uint32_t cap = a.capacity;
	if constexpr (LEN) bk = a.back + (((size_t) (live ? s : 0) * a.n_kinds + wid) * C + ch) * 2 + (vu ? 0 : filt);
	// the carried state, here before the first chunk is asked for: nothing in the loop below waits for it behind a chunk's loads
	mtr_needle_state v0 = *st;
	asm volatile ("" : "+v" (v0.z1), "+v" (v0.z2), "+v" (v0.m), "+v" (v0.last), "+v" (v0.s1), "+v" (v0.s2), "+v" (v0.res));

	// One loop per kind: the waves of a workgroup meet at its barrier from different places (the three chains, the helpers), once per chunk each.  Chunk c + 1 is on its
	// way into registers while chunk c goes through the chain; it is stored behind the barrier that says chunk c - 1's readers are done.
	auto run = [&] (auto& chain, auto put) __attribute__ ((always_inline)) {
		Walk wk;
		wk.j = a.fill; wk.P = a.period; wk.P4 = a.period & ~3u; wk.point = a.point0;
		fetch (0);
		for (int64_t c = 0; c < nchunks; ++c) {
			stash ((int) (c & 1), c * CH);
			__syncthreads ();
			if (c + 1 < nchunks) fetch ((c + 1) * CH);
			const int nf = (int) min ((int64_t) CH, N - c * CH);
			if constexpr (LEN) {
				// every lane of the wave takes the whole chunk and none ends with it: the lock-step walk
				const int64_t ce = c * CH + nf;
				const bool whole = closes ? E > ce : E >= ce;
				if (__all (whole)) walk (chain, wk, lds[c & 1], nf, put);
				else {
					const int64_t left = E - c * CH;
					const int lim = left <= 0 ? 0 : left >= nf ? nf : (int) left;
					walk_ragged (chain, wk, lds[c & 1], nf, lim, closes && left > 0 && left <= nf, put);
				}
			} else walk (chain, wk, lds[c & 1], nf, put);
		}
	};
	if (vu) {
		Vu<C, LEN> p;
		if constexpr (LEN) p.zb = *bk;
		p.z1 = v0.z1; p.z2 = v0.z2; p.m = v0.m; p.s1 = v0.s1; p.s2 = v0.s2; p.last = v0.last; p.res = v0.res;
		p.t2 = p.z2 / 2;
		p.w = w1; p.w4 = w2; p.g = g; p.base = sl * G::PITCH + ch; p.series = a.series != 0;
		run (p, [&] (float r, uint64_t point) { if (writer && point < cap) pts[point * C] = r; });
		if (writer) { st->z1 = p.z1; st->z2 = p.z2; st->m = p.m; st->s1 = p.s1; st->s2 = p.s2; st->last = p.last; st->res = p.res; }
		if constexpr (LEN) if (writer) *bk = p.zb;
		return;
	}
	auto ppm = [&] (auto& p) __attribute__ ((always_inline)) {
		if constexpr (LEN) p.zb = *bk;
		p.z = filt ? v0.z2 : v0.z1; p.m = v0.m; p.s = filt ? v0.s2 : v0.s1; p.last = v0.last; p.res = v0.res;
		p.w = filt ? w2 : w1; p.w3 = w3; p.g = g; p.mv = a.mv[ch]; p.sgn = ch ? 0x80000000u : 0u; p.series = a.series != 0;
		run (p, [&] (float r, uint64_t point) { if (writer && !filt && point < cap) pts[point * C] = r; });
		if (!writer) return;
		if constexpr (LEN) *bk = p.zb;
		if (filt) { st->z2 = p.z; st->s2 = p.s; }
		else { st->z1 = p.z; st->s1 = p.s; st->m = p.m; st->last = p.last; st->res = p.res; }
	};
	if (C == 2 && kind == MTR_NEEDLE_MS) {
		Ppm<C, true, LEN> p;
		p.base = sl * G::PITCH;
		ppm (p);
	} else {
		Ppm<C, false, LEN> p;
		p.base = sl * G::PITCH + ch;
		ppm (p);
	}
}

int kind_index (uint32_t kinds, uint32_t kind)
{
	if (!kind || (kind & (kind - 1)) || !(kinds & kind)) return -1;
	return __builtin_popcount (kinds & (kind - 1));
}

}  // namespace

template <int C> static void launch_c (const mtr_needle_args& a, hipStream_t st)
{
	const dim3 grid ((a.n_streams + Geo<C>::NS - 1) / Geo<C>::NS);
	if (a.back) hipLaunchKernelGGL ((k_needle<C, true>), grid, dim3 (64 * NW), 0, st, a);
	else hipLaunchKernelGGL ((k_needle<C, false>), grid, dim3 (64 * NW), 0, st, a);
}

static int mtr_launch_needle (const mtr_needle_args& a, uint32_t n_channels, void* stream)
{
	if (n_channels == 2) launch_c<2> (a, (hipStream_t) stream);
	else launch_c<1> (a, (hipStream_t) stream);
	return hipGetLastError () == hipSuccess ? 0 : -1;
}

// ---- NEEDLE in the engine: set-up, the call's step, the blob's section and the cursors in it, the C entry points ------------------------

constexpr uint32_t NEEDLE_MIN_PERIOD = 16;                      // frames: the shortest period of the reading series
static uint32_t needle_count (const mtr_engine* e) { return (uint32_t) __builtin_popcount (e->nd.kinds); }
static size_t needle_pitch (const mtr_engine* e)
{
	return sizeof (mtr_needle_hdr) + (size_t) needle_count (e) * e->cfg.n_channels * sizeof (mtr_needle_state);
}

// the coefficients of the selected kinds, in the order of their bits: the order of the waves, the states and the series
static void needle_coefs (mtr_engine* e)
{
	uint32_t i = 0;
	for (uint32_t k = 1; k <= MTR_NEEDLE_MS; k <<= 1)
		if (e->nd.kinds & k) { e->nd.kind[i] = k; mtr_setup_needle (k, e->cfg.sample_rate, e->nd.w[i]); ++i; }
}

static int needle_create (mtr_engine* e)
{
	e->nd.kinds = MTR_NEEDLE_IEC2;
	e->nd.ser = {};
	e->nd.db[0] = e->nd.db[1] = 0.f; e->nd.mv[0] = e->nd.mv[1] = 1.0f;   // msppmdsp.cc:34-43 ...
	needle_coefs (e);
	int rc = mtr_engine_needle_set_gain (e, 0, -6.f);                     // ... and src/meters.cc:211-212
	if (rc == MTR_OK) rc = mtr_engine_needle_set_gain (e, 1, -6.f);
	return rc;
}

static int needle_step (mtr_engine* e, const Call& c, Cursors& nx, const StreamEnds& se)
{
	const uint32_t P = e->nd.ser.period, cap = e->nd.ser.cap, C = e->cfg.n_channels;
	mtr_needle_args a;
	memset (&a, 0, sizeof (a));
	a.audio = c.audio; a.stride = c.stride; a.n_frames = c.n_frames;
	a.n_streams = c.cnt; a.n_kinds = needle_count (e);
	memcpy (a.kind, e->nd.kind, sizeof (a.kind));
	memcpy (a.w, e->nd.w, sizeof (a.w));
	a.mv[0] = e->nd.mv[0]; a.mv[1] = e->nd.mv[1];
	a.period = P ? P : (uint32_t) c.n_frames; a.fill = P ? (uint32_t) e->pos.nd.fill : 0; a.series = P != 0;
	a.capacity = cap; a.point0 = e->pos.nd.points;
	a.state_pitch = (uint32_t) needle_pitch (e);
	a.state = e->nd.state.p + (size_t) c.off * a.state_pitch;
	a.kind_pitch = (uint64_t) e->cfg.n_streams * cap * C;
	a.points = P && cap ? e->nd.series.p + (size_t) c.off * cap * C : nullptr;
	if (!a.points) a.capacity = 0;
	// The length-masking kernel takes a ragged call, and every call that ends inside a group of four frames: it alone keeps what stood in
	// front of that group (e->nd.back), which a stream needs that a later call ends before the group is complete
	const uint64_t jn = P ? (e->pos.nd.fill + c.n_frames) % P : 0;
	a.ends = se.ends;
	a.back = se.ends || (jn < (P & ~3u) && (jn & 3)) ? e->nd.back.p + (size_t) c.off * a.n_kinds * C * 2 : nullptr;
	if (mtr_launch_needle (a, C, c.st)) return fail (MTR_ERR_HIP, "k_needle launch");
	nx.nd = series_advance (e->pos.nd, P, c.n_frames);
	return MTR_OK;
}

static void needle_sections (const mtr_engine* e, std::vector<StateSection>& v)
{
	v.push_back ({ e->nd.state.p, needle_pitch (e) });
}

// The blob header: mtr_needle_hdr in front of every stream's detectors.  A blob whose kinds or period are not the engine's is refused; a
// fresh engine takes the rest
constexpr const char* NEEDLE_CORRUPT = "mtr_engine_state_import: corrupt blob (cursors of the needle meters)";

static void needle_hdr_write (const mtr_engine* e, void* out)
{
	mtr_needle_hdr& h = *static_cast<mtr_needle_hdr*> (out);       // (zeroed: so stays the pad)
	h.kinds = e->nd.kinds; h.period = e->nd.ser.period; h.fill = (uint32_t) e->pos.nd.fill;
	memcpy (h.db, e->nd.db, sizeof (h.db)); memcpy (h.mv, e->nd.mv, sizeof (h.mv));
}

static int needle_hdr_check (const mtr_engine* e, const void* in, bool fresh)
{
	const mtr_needle_hdr& h = *static_cast<const mtr_needle_hdr*> (in);
	if (!series_blob_ok (h.period, h.fill, NEEDLE_MIN_PERIOD, 0xFFFFFFFFu) || !h.kinds || (h.kinds & ~15u) || !(h.mv[0] >= 0.f) || !(h.mv[1] >= 0.f))
		return fail (MTR_ERR_STATE, NEEDLE_CORRUPT);
	if (h.kinds != e->nd.kinds || h.period != e->nd.ser.period)
		return fail (MTR_ERR_STATE, "mtr_engine_state_import: the blob's needle meters are configured otherwise (kinds or period)");
	if (!fresh && (h.fill != e->pos.nd.fill || memcmp (h.db, e->nd.db, sizeof (h.db)) || memcmp (h.mv, e->nd.mv, sizeof (h.mv))))
		return fail (MTR_ERR_STATE, "mtr_engine_state_import: the engine does not stand where the blob's streams do (period or gains of the needle meters)");
	return MTR_OK;
}

static void needle_hdr_take (mtr_engine* e, const void* in)
{
	const mtr_needle_hdr& h = *static_cast<const mtr_needle_hdr*> (in);
	e->pos.nd.fill = h.fill;
	memcpy (e->nd.db, h.db, sizeof (h.db)); memcpy (e->nd.mv, h.mv, sizeof (h.mv));
}

static constinit BlobHeader needle_hdr = { .offset = 0, .bytes = sizeof (mtr_needle_hdr), .corrupt = NEEDLE_CORRUPT, .write = needle_hdr_write, .check = needle_hdr_check, .take = needle_hdr_take };
static SeriesView needle_series (mtr_engine* e) { return { &e->nd.ser, &Cursors::nd, &e->nd.points }; }

constinit SideMeter needle_meter = { .bits = MTR_METER_NEEDLE, .max_frames = 0x7fffffffull, .max_text = "NEEDLE: n_frames per call must be < 2^31 - 1 (the reference's int n)",
                                     .create = needle_create, .reset = mtr_engine_needle_reset, .step = needle_step, .sections = needle_sections, .hdr = &needle_hdr, .series = needle_series };

extern "C" {

int mtr_needle_coef (uint32_t kind, float sample_rate, float* out4)
{
	if (!out4 || !(sample_rate >= 1.f)) return fail (MTR_ERR_ARG, "mtr_needle_coef");
	if (mtr_setup_needle (kind, sample_rate, out4)) return fail (MTR_ERR_ARG, "mtr_needle_coef: kind is one of MTR_NEEDLE_VU / _IEC1 / _IEC2 / _MS");
	return MTR_OK;
}

static int no_needle (const mtr_engine* e) { return !e || !(e->cfg.meters & MTR_METER_NEEDLE); }

int mtr_engine_needle_reset (mtr_engine* e)
{
	if (no_needle (e)) return fail (MTR_ERR_ARG, "no NEEDLE in this engine");
	e->snap_valid = false;
	HIPCHK (hipSetDevice (e->cfg.device));
	const uint32_t S = e->cfg.n_streams, per = needle_count (e) * e->cfg.n_channels;
	const size_t pitch = needle_pitch (e);
	if (e->nd.state.reserve ((size_t) S * pitch) || e->nd.back.reserve ((size_t) S * per * 2)) return fail (MTR_ERR_NOMEM, "hipMalloc NEEDLE state");
	std::vector<unsigned char> h ((size_t) S * pitch, 0);             // the constructors: z1 = z2 = m = 0, _res = true
	for (uint32_t s = 0; s < S; ++s)
		for (uint32_t i = 0; i < per; ++i) {
			mtr_needle_state v;
			memset (&v, 0, sizeof (v));
			v.res = 1;
			memcpy (h.data () + (size_t) s * pitch + sizeof (mtr_needle_hdr) + (size_t) i * sizeof (v), &v, sizeof (v));
		}
	HIPCHK (hipStreamSynchronize (e->last_stream));
	HIPCHK (hipMemcpy (e->nd.state.p, h.data (), h.size (), hipMemcpyHostToDevice));
	HIPCHK (hipMemset (e->nd.back.p, 0, (size_t) S * per * 2 * sizeof (float)));
	// (the series: a stream that a ragged call closes early leaves 0.0f behind its own points)
	if (e->nd.series.n) HIPCHK (hipMemset (e->nd.series.p, 0, e->nd.series.n * sizeof (float)));
	e->pos.nd = {};
	e->nd.points.assign (S, 0);
	return MTR_OK;
}

int mtr_engine_needle_configure (mtr_engine* e, uint32_t kinds, uint32_t period_frames, uint32_t capacity_points)
{
	if (no_needle (e)) return fail (MTR_ERR_ARG, "no NEEDLE in this engine");
	if (!kinds || (kinds & ~(uint32_t) (MTR_NEEDLE_VU | MTR_NEEDLE_IEC1 | MTR_NEEDLE_IEC2 | MTR_NEEDLE_MS)))
		return fail (MTR_ERR_ARG, "mtr_engine_needle_configure: kinds is a non-empty subset of MTR_NEEDLE_VU | _IEC1 | _IEC2 | _MS");
	if ((kinds & MTR_NEEDLE_MS) && e->cfg.n_channels != 2)
		return fail (MTR_ERR_UNSUPPORTED, "MTR_NEEDLE_MS meters the sum and the difference of a stereo pair: n_channels 2");
	int rc = series_configure_check (e, "mtr_engine_needle_configure", period_frames, NEEDLE_MIN_PERIOD, "16");
	if (rc || (rc = wait_stream (e))) return rc;
	const uint32_t cap = period_frames ? capacity_points : 0;     // (no period, no series)
	if ((rc = series_ring (e->nd.series, (size_t) __builtin_popcount (kinds) * e->cfg.n_streams * cap * e->cfg.n_channels, "hipMalloc NEEDLE series"))) return rc;
	e->nd.kinds = kinds;
	e->nd.ser = { period_frames, cap };
	needle_coefs (e);
	return mtr_engine_needle_reset (e);
}

int mtr_engine_needle_set_gain (mtr_engine* e, int side, float db)
{
	if (no_needle (e)) return fail (MTR_ERR_ARG, "no NEEDLE in this engine");
	if (side < 0 || side > 1 || !std::isfinite (db)) return fail (MTR_ERR_ARG, "mtr_engine_needle_set_gain: side 0 (M) or 1 (S), a finite gain");
	if (e->nd.db[side] == db) return MTR_OK;                          // msppmdsp.cc:143-145
	e->nd.db[side] = db;
	e->nd.mv[side] = mtr_setup_needle_gain (db);
	return MTR_OK;
}

int mtr_engine_needle_read (mtr_engine* e, uint32_t kind, uint32_t first, uint32_t count, float* level, float* state)
{
	int rc = meter_range (e, !no_needle (e) && level, "no NEEDLE in this engine", first, count);
	if (rc) return rc;
	const int ki = kind_index (e->nd.kinds, kind);
	if (ki < 0) return fail (MTR_ERR_ARG, "mtr_engine_needle_read: kind is one of the engine's selected kinds");
	if ((rc = wait_stream (e))) return rc;
	const uint32_t C = e->cfg.n_channels;
	const size_t pitch = needle_pitch (e);
	std::vector<unsigned char> h ((size_t) count * pitch);
	if (count) HIPCHK (hipMemcpy (h.data (), e->nd.state.p + (size_t) first * pitch, h.size (), hipMemcpyDeviceToHost));
	const float g = e->nd.w[ki][3];
	for (uint32_t i = 0; i < count; ++i)
		for (uint32_t c = 0; c < C; ++c) {
			unsigned char* const at = h.data () + (size_t) i * pitch + sizeof (mtr_needle_hdr) + ((size_t) ki * C + c) * sizeof (mtr_needle_state);
			mtr_needle_state v;
			memcpy (&v, at, sizeof (v));
			if (e->nd.ser.period) level[(size_t) i * C + c] = v.last;
			else {
				level[(size_t) i * C + c] = g * v.m;                      // read (): _res = true; return _g * _m
				v.res = 1;
				memcpy (at, &v, sizeof (v));
			}
			if (state) { state[((size_t) i * C + c) * 2] = v.s1; state[((size_t) i * C + c) * 2 + 1] = v.s2; }
		}
	if (count && !e->nd.ser.period) HIPCHK (hipMemcpy (e->nd.state.p + (size_t) first * pitch, h.data (), h.size (), hipMemcpyHostToDevice));
	return MTR_OK;
}

int mtr_engine_needle_series (mtr_engine* e, uint32_t kind, uint32_t first, uint32_t count, float* out, uint32_t capacity, uint32_t* n_points, uint32_t* dropped)
{
	int rc = meter_range (e, !no_needle (e), "no NEEDLE in this engine", first, count);
	if (rc) return rc;
	const int ki = kind_index (e->nd.kinds, kind);
	if (ki < 0) return fail (MTR_ERR_ARG, "mtr_engine_needle_series: kind is one of the engine's selected kinds");
	const size_t take = series_counts (e->pos.nd.points, e->nd.ser.cap, capacity, n_points, dropped);
	if (!out || !count || !take) return MTR_OK;
	if ((rc = wait_stream (e))) return rc;
	const size_t C = e->cfg.n_channels;
	return series_fetch (out, e->nd.series.p + (size_t) ki * e->cfg.n_streams * e->nd.ser.cap * C, C, first, e->nd.ser.cap, capacity, take, count);
}

} // extern "C"
