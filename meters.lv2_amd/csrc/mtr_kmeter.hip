// mtr_kmeter.hip — Kmeterdsp (the K-meters' and the TP+RMS plugins' RMS / peak detector) for a batch (gfx950).
//
// Replaces Kmeterdsp::process (jmeters/kmeterdsp.cc:56-140) with the semantics of one process () per engine
// call: per channel, on s = x^2,
//     z1 += w (s - z1) for each sample;  z2 += 4 w (z1 - z2) once per group of four samples (n mod 4 trailing
//     samples are dropped, :71);  t = max s;
//     at the end of the call: rms = sqrt (2 z2) (max-held until read), peak = sqrt (t) with the hold / fall-back
//     bookkeeping of :121-138.
//
// Only the state at the END of the call and the maximum of s enter the result, and the two-pole filter is linear
// in s: (z1, z2) after a group = A (z1, z2) + (w (1 - w)^(3 - q) s_q, q = 0..3, into z1 and 4 w times that into
// z2), A = [[a, 0], [4 w a, b]], a = (1 - w)^4, b = 1 - 4 w.  So the end state is a WEIGHTED SUM of the squares —
// the sample in slot q of the group k groups before the last one weighs A^k (1, 4 w) w (1 - w)^(3 - q) — and the
// kernel is a plain coalesced streaming reduction: lane t of a workgroup takes the groups k = k0 + t, k0 + t +
// 256, ... (its A^k advances by the constant A^256 per step, started from the closed form A^k = [[a^k, 0],
// [4 w a (a^k - b^k) / (a - b), b^k]]), sums in double, and a one-thread-per-channel kernel adds the chunks and
// A^G times the carried state and does the per-call bookkeeping.  (First version: pieces run serially from a
// zero state, four groups per lane, and combined in a tree: each lane read its own 128 contiguous bytes — 8.1 ms
// per 31.5 GB.)  The sums are re-associated and carried in double: tests/test_gpu_kmeter.py holds the RMS to
// 4 * 2^-24 relative against the same recurrence in double (oracle mo_kmeter_process_f64).
// A square that is not finite (a sample that is, or |x| > 1.84e19) is not linear: the reference's z1 becomes Inf, the
// next frame makes it NaN (Inf - Inf), :101-102 zero the states — the reading is 0 and the next call starts from 0 —
// unless it is the last frame the stream takes (k == 0, slot 3; with LEN too), where the states end as Inf, the reading
// is Inf and the next call starts from the clamp at 50.  A weighted sum would read Inf wherever the weight is not 0
// and NaN -> 0 where a^k has underflowed: the sums take km_square (s) (mtr_kmeter_dsp.h, the series' and SURROUND's
// rule), a NaN for such a square anywhere but there; the maximum takes s itself (:103 zeroes an infinite one).
//
// LEN (both kernels): the call carries per-stream ends (a.ends, call-relative: mtr_engine_process_*_tracks, or any call once a stream of
// its view is closed).  Stream s ends at frame E = ends [s], workgroup-uniform (one scalar load): a stream that ends inside the call sees
// ONE process (p, E) — E / 4 groups, the weights A^k counted back from ITS last group, fpp = E with the fall-back factor the host
// computed for that fpp (a.falls [s], km_fall) — and a stream with E = n_frames exactly what the dense call gives it
// (the cursor's fall).  A workgroup of k_kmeter_pieces whose chunk lies at or past the stream's groups returns before it touches memory
// and writes NO piece slot: k_kmeter_final adds the stream's own chunks only — it never reads those slots.  E = 0 (a closed stream,
// frames [s] == 0): nothing is written, not even the + 1e-20f.  Groups start on multiples of four frames whatever E is: the 16-byte
// path is the dense one's.  The dense instantiations are the kernels as they always were.
//
// THE READING SERIES (mtr_engine_kmeter_set_period, P > 0: k_kmeter_blocks / k_kmeter_walk; the kernels above are then not launched).
// The streams are metered as by a host that calls process (p, P) + read (rms, peak) on consecutive blocks of exactly P frames wherever
// the engine calls cut the audio (kmeterdsp.cc:56-155).  A call is cut into PIECES as mtr_stcorr.hip and mtr_surround.hip cut it
// (mtr_stcorr_scan.h: the open block's rest, whole blocks, what the call leaves open, each cut at `chunk` = 32768 frames), one workgroup
// per (stream, piece), lane t on the four frames b0 + 4 t, + 4 (t + 256), ... of its piece: 16-byte loads where the piece's first frame
// lies on 16 bytes of the buffer, 8- or 4-byte ones where an odd P or a block that starts mid-row leaves it elsewhere, and nothing outside
// the piece's frames.  The weights are the pointwise ones on s = x^2, and the geometry, the lane's powers, the rule for a square that is
// not finite and the walk's arithmetic are mtr_kmeter_dsp.h's, which derives them (SURROUND's walk takes them from there too).  Frames at
// j >= L - L mod 4 (L = P, or what a ragged call leaves a closing stream of its last block) weigh nothing and do not enter the maximum
// (:79).  One thread per (stream, channel) walks the pieces in order, carries (z1, z2) in closed form (km_carry) — also through a call
// that ends inside a group — and at every block's end does :101-139 in f32, one rounding per operation, and appends (rms, peak).
// Between two calls the open block's (z1, z2) stay doubles and its maximum an f32, with what they were IN FRONT OF the group of four that
// the call left open (bz1, btmax; z2 moves at group ends only): a ragged call that closes the stream before that group completes drops
// the whole group from filter and peak, as the n / 4 groups of the truncated block demand.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "mtr_engine_impl.h"
#include "mtr_kmeter_dsp.h"
#include "mtr_stcorr_scan.h"

/* Kmeterdsp per (stream, channel) state (jmeters/kmeterdsp.h) */
typedef struct mtr_kmeter_state {
	float    z1, z2, rms, peak;
	int32_t  cnt, flag;
} mtr_kmeter_state;

typedef struct mtr_kmeter_args {
	const float*    audio;        /* [S][stride][C] */
	uint64_t        stride, n_groups;   /* n_frames / 4 (kmeterdsp.cc:71) */
	uint32_t        n_streams, n_channels, n_pieces, fpp;
	int32_t         hold;
	float           omega, fall;
	double          pw1[3];       /* A = [[a, 0], [c, b]] per group of four samples */
	mtr_kmeter_state* state;      /* [S][2] */
	double*         piece_state;  /* [S][n_pieces][4]: each chunk's weighted sums (z1, z2 per channel), already carried to the call's end */
	float*          piece_max;    /* [S][n_pieces][2] */
	const uint32_t* ends;         /* [S] per-stream ends of a ragged call (the LEN instantiations), NULL on a dense one ... */
	const float*    falls;        /* [S] ... and the fall-back factor of each stream that ends inside the call */
} mtr_kmeter_args;

/* the reading series: per (stream, channel) the open block between two calls */
typedef struct mtr_kmeter_carry {
	double   z1, z2;              /* where the block stands: exact continuations inside a block, the f32 of :106-107 at its start */
	double   bz1;                 /* z1 in front of the group of four that is open (= z1 where none is) */
	float    tmax, btmax;         /* max x^2 of the open block so far; ... in front of the open group */
} mtr_kmeter_carry;

/* per stream: the section a state blob carries at P > 0.  In front, for the blob (whose header has no room for them): the engine's
 * period, the frames into the open block, Kmeterdsp's _fpp / _fall — the host's copies rule, export writes them in */
typedef struct mtr_kmeter_open {
	uint32_t         period, fill;
	uint32_t         fpp;
	float            fall;
	mtr_kmeter_carry ch[2];
} mtr_kmeter_open;

#define MTR_KMB_PIECE 5            /* doubles per (stream, piece, channel): what the piece's frames give to z1 and z2 at its end, max x^2; what
                                    * those in front of its last group end give to z1 THERE, and their max x^2 */

typedef struct mtr_kmb_args {
	const float*    audio;        /* [S][stride][C] */
	uint64_t        stride, n_frames;
	uint64_t        period;       /* P > 0 */
	uint64_t        e0;           /* call frame at which the block open on entry ends */
	uint32_t        n_streams, n_channels, n_pieces, chunk;
	float           fall;         /* the fall-back factor of fpp = P */
	mtr_km_consts   k;            /* (st1 / sta / stb: a lane's next group of four frames is 4 NT frames on) */
	uint32_t        capacity;     /* points per stream the series hold */
	uint64_t        point0;       /* blocks completed before this call */
	mtr_kmeter_state* state;      /* [S][2]: rms, peak of the last completed block, cnt (z1, z2: the carry's, as f32) */
	mtr_kmeter_open* open;        /* [S] */
	double*         piece;        /* [S][n_pieces][C][MTR_KMB_PIECE] */
	float*          s_rms;        /* [S][capacity][C], NULL if capacity == 0 */
	float*          s_peak;
	const uint32_t* ends;         /* [S] per-stream ends of a ragged call (the LEN instantiations), NULL on a dense one ... */
	const float*    falls;        /* [S] ... and the fall-back factor of the truncated block of each stream that ends inside one */
} mtr_kmb_args;

namespace {

constexpr int NT = 256;                  // threads per workgroup
constexpr int CH = 32 * NT;              // groups (of four samples) per workgroup: 32768 frames

using namespace mtr_km;                  // Mat / mat_pow, and the reading series' geometry, weights and walk (mtr_kmeter_dsp.h)

template <int C, bool LEN>
__global__ __launch_bounds__ (NT) void k_kmeter_pieces (const mtr_kmeter_args a)
{
	const uint32_t chunk = blockIdx.x, s = blockIdx.y;
	uint64_t n_groups = a.n_groups;
	if constexpr (LEN) {
		n_groups = a.ends[s] / 4;
		if ((uint64_t) chunk * CH >= n_groups) return;             // not one of the stream's own chunks
	}
	const float* const src = a.audio + (size_t) s * a.stride * C;
	const float w = a.omega, r = 1.f - w;
	const float u3 = w, u2 = w * r, u1 = u2 * r, u0 = u1 * r;             // weight of slot q inside its own group
	// k = groups after this one; chunk c covers k in [c CH, (c + 1) CH)
	uint64_t k = (uint64_t) chunk * CH + threadIdx.x;
	const uint64_t k_end = min ((uint64_t) (chunk + 1) * CH, n_groups);
	Mat m = mat_pow (a.pw1[0], a.pw1[1], a.pw1[2], (double) k);
	const Mat st = mat_pow (a.pw1[0], a.pw1[1], a.pw1[2], (double) NT);
	const double w4 = 4.0 * (double) w;
	double z1[2] = { 0, 0 }, z2[2] = { 0, 0 };
	float t[2] = { 0.f, 0.f };
	const bool wide = C == 2 ? ((((size_t) s * a.stride) & 1) == 0 && (reinterpret_cast<size_t> (a.audio) & 15) == 0)
	                         : ((((size_t) s * a.stride) & 3) == 0 && (reinterpret_cast<size_t> (a.audio) & 15) == 0);
	for (; k < k_end; k += NT) {
		const float* const p = src + (size_t) (n_groups - 1 - k) * 4 * C;
		float v[4 * C];
		if (wide) {
#pragma unroll
			for (int i = 0; i < C; ++i) {
				const float4 q = reinterpret_cast<const float4*> (p)[i];
				v[4 * i] = q.x; v[4 * i + 1] = q.y; v[4 * i + 2] = q.z; v[4 * i + 3] = q.w;
			}
		} else {
#pragma unroll
			for (int i = 0; i < 4 * C; ++i) v[i] = p[i];
		}
		const double U1 = m.a, U2 = m.c + w4 * m.b;
		const int64_t j0 = (int64_t) (n_groups - 1 - k) * 4, Lg = (int64_t) n_groups * 4;   // the group's first frame; the frames the stream takes
#pragma unroll
		for (int c = 0; c < C; ++c) {
			const float s0 = v[c] * v[c], s1 = v[C + c] * v[C + c], s2 = v[2 * C + c] * v[2 * C + c], s3 = v[3 * C + c] * v[3 * C + c];
			t[c] = t[c] < s0 ? s0 : t[c];                          // kmeterdsp.cc:79: if (t < s) t = s (NaN never enters)
			t[c] = t[c] < s1 ? s1 : t[c];
			t[c] = t[c] < s2 ? s2 : t[c];
			t[c] = t[c] < s3 ? s3 : t[c];
			// a square that is not finite: NaN into the sums, unless it is the last frame the stream takes (km_square; the maximum took s
			// itself).  One test per group: the sum of four squares is finite only if each is, and km_square keeps a finite one as it is
			float q0 = s0, q1 = s1, q2 = s2, q3 = s3;
			if (!isfinite ((s0 + s1) + (s2 + s3))) {
				q0 = km_square (s0, j0, Lg); q1 = km_square (s1, j0 + 1, Lg); q2 = km_square (s2, j0 + 2, Lg); q3 = km_square (s3, j0 + 3, Lg);
			}
			const double g = (double) (u0 * q0) + (double) (u1 * q1) + (double) (u2 * q2) + (double) (u3 * q3);
			z1[c] += U1 * g;
			z2[c] += U2 * g;
		}
		// A^(k + NT) = A^k A^NT
		const double na = m.a * st.a, nc = m.c * st.a + m.b * st.c, nb = m.b * st.b;
		m.a = na; m.c = nc; m.b = nb;
	}
	__shared__ double sh[NT / 64][4];
	__shared__ float sht[NT / 64][2];
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		z1[0] += __shfl_xor (z1[0], d, 64); z2[0] += __shfl_xor (z2[0], d, 64);
		z1[1] += __shfl_xor (z1[1], d, 64); z2[1] += __shfl_xor (z2[1], d, 64);
		t[0] = fmaxf (t[0], __shfl_xor (t[0], d, 64)); t[1] = fmaxf (t[1], __shfl_xor (t[1], d, 64));
	}
	const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
	if (lane == 0) { sh[wid][0] = z1[0]; sh[wid][1] = z2[0]; sh[wid][2] = z1[1]; sh[wid][3] = z2[1]; sht[wid][0] = t[0]; sht[wid][1] = t[1]; }
	__syncthreads ();
	if (threadIdx.x == 0) {
		const size_t o = (size_t) s * a.n_pieces + chunk;
		double e[4] = { 0, 0, 0, 0 };
		float tt[2] = { 0.f, 0.f };
		for (int i = 0; i < NT / 64; ++i) {
			for (int j = 0; j < 4; ++j) e[j] += sh[i][j];
			tt[0] = fmaxf (tt[0], sht[i][0]); tt[1] = fmaxf (tt[1], sht[i][1]);
		}
		for (int j = 0; j < 4; ++j) a.piece_state[o * 4 + j] = e[j];
		a.piece_max[o * 2] = tt[0]; a.piece_max[o * 2 + 1] = tt[1];
	}
}

// one thread per (stream, channel): add the chunks and the carried state, then kmeterdsp.cc:108-138
template <bool LEN>
__global__ void k_kmeter_final (const mtr_kmeter_args a)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= a.n_streams * a.n_channels) return;
	const uint32_t s = i / a.n_channels, c = i % a.n_channels;
	uint64_t n_groups = a.n_groups;
	uint32_t n_pieces = a.n_pieces, fpp = a.fpp;                       // the stream's own (LEN), the call's otherwise
	float fall = a.fall;
	if constexpr (LEN) {
		const uint32_t E = a.ends[s];
		if (E == 0) return;
		if (E != a.fpp) {                                              // the stream ends inside the call: one process (p, E)
			n_groups = E / 4;
			n_pieces = (uint32_t) ((n_groups + CH - 1) / CH);
			fpp = E; fall = a.falls[s];
		}
	}
	mtr_kmeter_state* const st = a.state + (size_t) s * 2 + c;
	float zi1 = st->z1 > 50 ? 50 : (st->z1 < 0 ? 0 : st->z1);         // :66-67 (a NaN state falls through, as there)
	float zi2 = st->z2 > 50 ? 50 : (st->z2 < 0 ? 0 : st->z2);
	double e1 = 0, e2 = 0;
	float t = 0.f;
	for (uint32_t p = 0; p < n_pieces; ++p) {                        // the weights already carry every chunk to the end
		const size_t o = ((size_t) s * a.n_pieces + p) * 4 + 2 * c;
		e1 += a.piece_state[o]; e2 += a.piece_state[o + 1];
		t = fmaxf (t, a.piece_max[((size_t) s * a.n_pieces + p) * 2 + c]);
	}
	const Mat g = mat_pow (a.pw1[0], a.pw1[1], a.pw1[2], (double) n_groups);
	double z1 = g.a * (double) zi1 + e1;
	double z2 = g.c * (double) zi1 + g.b * (double) zi2 + e2;
	if (n_groups == 0) { z1 = (double) zi1; z2 = (double) zi2; }
	const KmClose r = km_close (z1, z2, t);                            // :100-109 (z1, z2: f32 values from here)
	st->z1 = (float) z1;
	st->z2 = (float) z2;
	if (st->flag) { st->rms = r.rms; st->flag = 0; }                   // :112-118
	else if (r.rms > st->rms) st->rms = r.rms;
	km_peak_hold (r.t, st->peak, st->cnt, a.hold, fpp, fall);          // :121-138
}

// ---- the reading series (P > 0) ----------------------------------------------------------------------------------------------------

constexpr uint32_t KMB_CHUNK = 32768;    // frames per piece at most: a multiple of four

using mtr_sc::piece_of;

// LEN: the stream ends at call frame a.ends[s] (0: closed, untouched; n_frames: the dense call's stream).  A piece that starts at or
// behind the end returns before it loads anything; the block an end inside the call cuts has L = the frames the stream has of it.
template <int C, bool LEN>
__global__ __launch_bounds__ (NT) void k_kmeter_blocks (const mtr_kmb_args a)
{
	const uint32_t s = blockIdx.y;
	const Piece pc = piece_of (a, blockIdx.x);
	const int64_t b0 = pc.b0;
	const int64_t blk0 = km_block_start (a.e0, a.period, a.period, b0);
	int64_t end = 0;
	if constexpr (LEN) {
		end = (int64_t) a.ends[s];
		if (b0 >= end) return;                                     // (uniform in the workgroup; end 0: every piece of the stream)
	}
	const KmGeom g = km_geom<LEN> (pc, blk0, a.period, end, a.n_frames);
	const int64_t b1 = g.b1, Lg = g.Lg, E1 = g.E1, pe = g.pe;
	const float* const src = a.audio + (size_t) s * a.stride * C;
	const double up = ipow (a.k.kri, (uint64_t) (E1 - pe));         // from a weight at E1 to the weight at pe
	const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
	// how wide the piece's loads may be: the address of its first frame (every lane's first frame lies 4 frames x a multiple behind it)
	// — the address itself, not base and frame index apart: a call that continues a buffer at an odd frame keeps the wide path
	const size_t a0 = reinterpret_cast<size_t> (src + (size_t) b0 * C);
	const bool w16 = (a0 & 15) == 0;
	const bool w8 = (a0 & 7) == 0;

	// the powers of the lane's first frame from exp (); from one of its groups of four frames to the next (4 NT frames = NT groups) they
	// move by constants
	int64_t f0 = b0 + 4 * (int64_t) tid;
	KmLane lt;
	lt.init (a.k, E1, pe, f0 - blk0);
	double e1[C], e2[C], eb[C];
	float tm[C], tb[C];
#pragma unroll
	for (int c = 0; c < C; ++c) { e1[c] = 0.0; e2[c] = 0.0; eb[c] = 0.0; tm[c] = 0.f; tb[c] = 0.f; }

	for (; f0 < b1; f0 += 4 * NT) {
		float v[4 * C];
		const float* const p = src + (size_t) f0 * C;
		if (f0 + 4 <= b1 && w16) {
#pragma unroll
			for (int i = 0; i < C; ++i) {
				const float4 q = reinterpret_cast<const float4*> (p)[i];
				v[4 * i] = q.x; v[4 * i + 1] = q.y; v[4 * i + 2] = q.z; v[4 * i + 3] = q.w;
			}
		} else if (f0 + 4 <= b1 && w8) {
#pragma unroll
			for (int i = 0; i < 2 * C; ++i) {
				const float2 q = reinterpret_cast<const float2*> (p)[i];
				v[2 * i] = q.x; v[2 * i + 1] = q.y;
			}
		} else {
#pragma unroll
			for (int k = 0; k < 4; ++k)
#pragma unroll
				for (int c = 0; c < C; ++c) v[k * C + c] = f0 + k < b1 ? p[k * C + c] : 0.f;
		}
		const int64_t j0 = f0 - blk0;
		KmLane ln = lt;
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			const int64_t jk = j0 + k;
			if (f0 + k < b1 && jk < Lg) {                           // (jk < E1 with it: E1 = min (Lg, b1 - blk0))
				const bool grp = ln.kt >= 0, front = jk < pe;       // its group ends inside the piece; it lies in front of the last group end
				const double wz1 = ln.z1_weight (), wz2 = ln.z2_weight (), wzb = ln.front_weight (up);
#pragma unroll
				for (int c = 0; c < C; ++c) {
					const float x = v[k * C + c];
					const float s2 = x * x;
					tm[c] = tm[c] < s2 ? s2 : tm[c];                 // kmeterdsp.cc:84: if (t < s) t = s (a NaN never enters)
					if (front) tb[c] = tb[c] < s2 ? s2 : tb[c];
					const float sq = km_square (s2, jk, Lg);
					e1[c] = fma (wz1, (double) sq, e1[c]);
					if (grp) e2[c] = fma (wz2, (double) sq, e2[c]);   // (no 0 x NaN: a later ragged close may drop the open group whole)
					if (front) eb[c] = fma (wzb, (double) sq, eb[c]);
				}
			}
			ln.next_frame (a.k, jk);
		}
		lt.next_step (a.k, NT);
	}

	__shared__ double shd[NT / 64][C][3];
	__shared__ float shf[NT / 64][C][2];
#pragma unroll
	for (int c = 0; c < C; ++c) {
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) {
			e1[c] += __shfl_xor (e1[c], d, 64); e2[c] += __shfl_xor (e2[c], d, 64); eb[c] += __shfl_xor (eb[c], d, 64);
			tm[c] = fmaxf (tm[c], __shfl_xor (tm[c], d, 64)); tb[c] = fmaxf (tb[c], __shfl_xor (tb[c], d, 64));
		}
		if (lane == 0) { shd[wid][c][0] = e1[c]; shd[wid][c][1] = e2[c]; shd[wid][c][2] = eb[c]; shf[wid][c][0] = tm[c]; shf[wid][c][1] = tb[c]; }
	}
	__syncthreads ();
	if (tid < C) {
		double x1 = 0.0, x2 = 0.0, xb = 0.0;
		float m = 0.f, mb = 0.f;
		for (int w = 0; w < NT / 64; ++w) {
			x1 += shd[w][tid][0]; x2 += shd[w][tid][1]; xb += shd[w][tid][2];
			m = fmaxf (m, shf[w][tid][0]); mb = fmaxf (mb, shf[w][tid][1]);
		}
		double* const out = a.piece + (((size_t) s * a.n_pieces + blockIdx.x) * C + tid) * MTR_KMB_PIECE;
		out[0] = x1; out[1] = x2; out[2] = (double) m; out[3] = xb; out[4] = (double) mb;
	}
}

// one thread per (stream, channel): the pieces in order, and kmeterdsp.cc:74-75, 101-139 + read (rms, peak) at every end of a block.
// LEN: the pieces up to the stream's end; an end inside the call and inside a block closes that block there — fpp = its frames, the
// fall-back factor a.falls[s] — as the stream's last point.  end == 0: the stream is not touched.
template <bool LEN>
__global__ void k_kmeter_walk (const mtr_kmb_args a)
{
#pragma clang fp contract(off)     // (the f32 steps at a block's end are the reference's, one rounding each: no fused multiply-add)
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= a.n_streams * a.n_channels) return;
	const uint32_t s = i / a.n_channels, c = i % a.n_channels, C = a.n_channels;
	int64_t end = (int64_t) a.n_frames;
	if constexpr (LEN) {
		end = (int64_t) a.ends[s];
		if (end == 0) return;
	}
	mtr_kmeter_state* const st = a.state + (size_t) s * 2 + c;
	mtr_kmeter_carry* const cy = &a.open[s].ch[c];
	const double kr = 1.0 - (double) a.k.omega;
	double z1 = cy->z1, z2 = cy->z2, bz1 = cy->bz1;
	float tmax = cy->tmax, btmax = cy->btmax;
	float rms = st->rms, peak = st->peak;
	int32_t cnt = st->cnt;
	uint64_t point = a.point0;
	for (uint32_t pi = 0; pi < a.n_pieces; ++pi) {
		const Piece pc = piece_of (a, pi);
		if constexpr (LEN) {
			if (pc.b0 >= end) break;
		}
		const KmGeom g = km_geom<LEN> (pc, km_block_start (a.e0, a.period, a.period, pc.b0), a.period, end, a.n_frames);
		const int64_t p0 = g.p0, E1 = g.E1, pe = g.pe;
		if (p0 == 0) {
			km_open (z1, z2);
			tmax = 0.f;
			bz1 = z1; btmax = 0.f;
		}
		const double* const pv = a.piece + (((size_t) s * a.n_pieces + pi) * C + c) * MTR_KMB_PIECE;
		if (E1 > p0) {
			if (pe >= p0) {                                        // the piece holds a group end: the state in front of its open group
				bz1 = pow (kr, (double) (pe - p0)) * z1 + pv[3];
				const float pb = (float) pv[4];
				btmax = tmax < pb ? pb : tmax;
			}
			km_carry (a.k, p0, E1, pv[0], pv[1], z1, z2);
			const float pm = (float) pv[2];
			tmax = tmax < pm ? pm : tmax;
		} else if (LEN && g.closes && pc.b0 == 0 && g.Lg < p0) {
			// the stream ends before the group that the call before left open completes: that group's frames drop out, all of them
			z1 = bz1; tmax = btmax;
		}
		if (!g.closes) continue;
		const KmClose r = km_close (z1, z2, tmax);
		bz1 = z1; btmax = 0.f; tmax = 0.f;
		rms = r.rms;                                               // :112-121 (a read follows every block: the flag is always set)
		km_peak_hold (r.t, peak, cnt, a.k.hold, (uint32_t) g.L, g.L == (int64_t) a.period ? a.fall : a.falls[s]);
		if (point < a.capacity) {
			const size_t o = ((size_t) s * a.capacity + point) * C + c;
			a.s_rms[o] = rms; a.s_peak[o] = peak;
		}
		++point;
	}
	cy->z1 = z1; cy->z2 = z2; cy->bz1 = bz1; cy->tmax = tmax; cy->btmax = btmax;
	st->z1 = (float) z1; st->z2 = (float) z2; st->rms = rms; st->peak = peak; st->cnt = cnt;
}

}  // namespace

static uint32_t mtr_kmeter_pieces (uint64_t n_groups) { return (uint32_t) ((n_groups + CH - 1) / CH); }

// f (C, LEN): the kernels' template arguments for a call of n_channels (2, or 1), with per-stream ends or without, as integral constants
template <typename F> static void with_c_len (uint32_t n_channels, bool ends, F f)
{
	using One = std::integral_constant<int, 1>;
	using Two = std::integral_constant<int, 2>;
	if (n_channels == 2) { if (ends) f (Two {}, std::true_type {}); else f (Two {}, std::false_type {}); }
	else                 { if (ends) f (One {}, std::true_type {}); else f (One {}, std::false_type {}); }
}

static int mtr_launch_kmeter (const mtr_kmeter_args& a, void* stream)
{
	hipStream_t st = (hipStream_t) stream;
	const uint32_t n = a.n_streams * a.n_channels;
	with_c_len (a.n_channels, a.ends != nullptr, [&] (auto C, auto LEN) {
		if (a.n_pieces) hipLaunchKernelGGL ((k_kmeter_pieces<C.value, LEN.value>), dim3 (a.n_pieces, a.n_streams), dim3 (NT), 0, st, a);
		hipLaunchKernelGGL (k_kmeter_final<LEN.value>, dim3 ((n + 63) / 64), dim3 (64), 0, st, a);
	});
	return hipGetLastError () == hipSuccess ? 0 : -1;
}

static int mtr_launch_kmb (const mtr_kmb_args& a, void* stream)
{
	hipStream_t st = (hipStream_t) stream;
	const dim3 g (a.n_pieces, a.n_streams), b (NT);
	const uint32_t n = a.n_streams * a.n_channels;
	with_c_len (a.n_channels, a.ends != nullptr, [&] (auto C, auto LEN) {
		hipLaunchKernelGGL ((k_kmeter_blocks<C.value, LEN.value>), g, b, 0, st, a);
		hipLaunchKernelGGL (k_kmeter_walk<LEN.value>, dim3 ((n + 63) / 64), dim3 (64), 0, st, a);
	});
	return hipGetLastError () == hipSuccess ? 0 : -1;
}

// ---- KMETER in the engine: the call's step, the blob's section, reset, the reading ------------------------------------------------------

// A K-meter's word of a ragged call: the fall-back factor of each stream of the view that ends inside the call.  Its process () is one of
// f frames (kmeterdsp.cc:60-65 with fpp = f; every other stream takes the cursor's) — with a period P: one of the frames it has of the
// block it ends in, if it ends inside one; `fill`: the frames into the open block where the call started
void kmeter_falls (const mtr_engine* e, const Call& c, uint64_t fill, uint64_t P, uint32_t* own)
{
	float* const fall = reinterpret_cast<float*> (own);
	for (uint32_t i = 0; i < c.cnt; ++i) {
		const uint64_t f = call_frames (e, c, i), kf = P ? (fill + f) % P : f;
		fall[i] = f && f < c.n_frames && kf ? km_fall (e->cfg.sample_rate, kf) : 0.f;
	}
}
static uint64_t kmeter_ends_fill (const mtr_engine* e, const Call& c, uint32_t* own) { kmeter_falls (e, c, e->pos.km.fill, e->km.ser.period, own); return 0; }

static uint32_t kmeter_min_period (const mtr_engine* e) { return (uint32_t) e->cfg.sample_rate / 20; }

// P > 0.  The blocks of the reading series are cut from where the CALL started (e->pos): every chunk of a host call sees the same cuts
static int kmeter_blocks_step (mtr_engine* e, const Call& c, Cursors& nx, const StreamEnds& se)
{
	const size_t vo = c.off;
	const uint64_t P = e->km.ser.period;
	const uint32_t cap = e->km.ser.cap, C = e->cfg.n_channels;
	mtr_kmb_args ka;
	memset (&ka, 0, sizeof (ka));
	ka.audio = c.audio; ka.stride = c.stride; ka.n_frames = c.n_frames;
	ka.period = P; ka.e0 = series_e0 (e->pos.km, P, c.n_frames);
	ka.n_streams = c.cnt; ka.n_channels = C; ka.chunk = KMB_CHUNK;
	ka.n_pieces = mtr_sc::n_pieces (c.n_frames, ka.e0, P, ka.chunk);
	if (nx.km_fpp != (uint32_t) P) {                                   // kmeterdsp.cc:65-70
		nx.km_fall = km_fall (e->cfg.sample_rate, P);
		nx.km_fpp = (uint32_t) P;
	}
	ka.fall = nx.km_fall;
	ka.k = e->km.k;
	ka.capacity = cap; ka.point0 = e->pos.km.points;
	if (e->km.bpiece.reserve ((size_t) e->cfg.n_streams * ka.n_pieces * C * MTR_KMB_PIECE)) return fail (MTR_ERR_NOMEM, "hipMalloc KMETER pieces");
	ka.state = e->km.state.p + vo * 2;
	ka.open = reinterpret_cast<mtr_kmeter_open*> (e->km.open.p) + vo;
	ka.piece = e->km.bpiece.p + vo * ka.n_pieces * C * MTR_KMB_PIECE;
	if (cap) { ka.s_rms = e->km.s_rms.p + vo * cap * C; ka.s_peak = e->km.s_peak.p + vo * cap * C; }
	ka.ends = se.ends; ka.falls = reinterpret_cast<const float*> (se.own);
	if (mtr_launch_kmb (ka, c.st)) return fail (MTR_ERR_HIP, "k_kmeter_blocks launch");
	nx.km = series_advance (e->pos.km, P, c.n_frames);
	return MTR_OK;
}

static int kmeter_step (mtr_engine* e, const Call& c, Cursors& nx, const StreamEnds& se)
{
	if (e->km.ser.period) return kmeter_blocks_step (e, c, nx, se);
	const size_t vo = c.off;
	mtr_kmeter_args ka;
	ka.audio = c.audio; ka.stride = c.stride; ka.n_groups = c.n_frames / 4;
	ka.n_streams = c.cnt; ka.n_channels = e->cfg.n_channels; ka.ends = se.ends; ka.falls = reinterpret_cast<const float*> (se.own);
	ka.n_pieces = mtr_kmeter_pieces (ka.n_groups);
	if (nx.km_fpp != (uint32_t) c.n_frames) {                          // kmeterdsp.cc:60-65
		nx.km_fall = km_fall (e->cfg.sample_rate, c.n_frames);
		nx.km_fpp = (uint32_t) c.n_frames;
	}
	ka.fpp = nx.km_fpp; ka.fall = nx.km_fall;
	ka.hold = e->km.k.hold; ka.omega = e->km.k.omega;
	memcpy (ka.pw1, e->km.k.pw, sizeof (ka.pw1));
	ka.state = e->km.state.p + vo * 2;
	if (e->km.piece.reserve ((size_t) e->cfg.n_streams * std::max<uint32_t> (ka.n_pieces, 1) * 4) || e->km.max.reserve ((size_t) e->cfg.n_streams * std::max<uint32_t> (ka.n_pieces, 1) * 2))
		return fail (MTR_ERR_NOMEM, "hipMalloc KMETER pieces");
	ka.piece_state = e->km.piece.p + vo * ka.n_pieces * 4; ka.piece_max = e->km.max.p + vo * ka.n_pieces * 2;
	if (mtr_launch_kmeter (ka, c.st)) return fail (MTR_ERR_HIP, "k_kmeter launch");
	return MTR_OK;
}

static void kmeter_sections (const mtr_engine* e, std::vector<StateSection>& v)
{
	v.push_back ({ e->km.state.p, 2 * sizeof (mtr_kmeter_state) });
}

// With a period the blob carries one more section, behind every older one (the second row of the meter in SIDE_METERS): the open block.
// Its header: period, the frames into the open block, _fpp / _fall.  An engine takes a blob of its own period only
static void kmeter_open_sections (const mtr_engine* e, std::vector<StateSection>& v)
{
	if (e->km.ser.period) v.push_back ({ e->km.open.p, sizeof (mtr_kmeter_open) });
}

constexpr size_t KM_HDR_BYTES = offsetof (mtr_kmeter_open, ch);
constexpr const char* KM_CORRUPT = "mtr_engine_state_import: corrupt blob (period of the KMETER series)";

static void kmeter_hdr_write (const mtr_engine* e, void* out)
{
	mtr_kmeter_open h;
	memset (&h, 0, KM_HDR_BYTES);
	h.period = e->km.ser.period; h.fill = (uint32_t) e->pos.km.fill; h.fpp = e->pos.km_fpp; h.fall = e->pos.km_fall;
	memcpy (out, &h, KM_HDR_BYTES);
}

static int kmeter_hdr_check (const mtr_engine* e, const void* in, bool fresh)
{
	mtr_kmeter_open h;
	memcpy (&h, in, KM_HDR_BYTES);
	if (!h.period || !series_blob_ok (h.period, h.fill, kmeter_min_period (e), 0x7ffffffeu) || (h.fpp && h.fpp != h.period)) return fail (MTR_ERR_STATE, KM_CORRUPT);
	if (h.period != e->km.ser.period || (!fresh && h.fill != e->pos.km.fill))
		return fail (MTR_ERR_STATE, "mtr_engine_state_import: the engine does not stand where the blob's streams do (period of the KMETER series)");
	return MTR_OK;
}

static void kmeter_hdr_take (mtr_engine* e, const void* in)
{
	mtr_kmeter_open h;
	memcpy (&h, in, KM_HDR_BYTES);
	e->pos.km.fill = h.fill; e->pos.km_fpp = h.fpp; e->pos.km_fall = h.fall;
}

static constinit BlobHeader kmeter_hdr = { .offset = 0, .bytes = KM_HDR_BYTES, .corrupt = KM_CORRUPT, .write = kmeter_hdr_write, .check = kmeter_hdr_check, .take = kmeter_hdr_take };
// (no reset and no step: the meter's first row resets and queues all of it)
constinit SideMeter kmeter_series_meter = { .bits = MTR_METER_KMETER, .sections = kmeter_open_sections, .hdr = &kmeter_hdr };

static SeriesView kmeter_series (mtr_engine* e) { return { &e->km.ser, &Cursors::km, &e->km.points }; }

constinit SideMeter kmeter_meter = { .bits = MTR_METER_KMETER, .max_frames = 0x7fffffffull, .max_text = "KMETER: n_frames per call must be < 2^31 - 1 (the reference's int n)",
                                     .reset = mtr_engine_kmeter_reset, .step = kmeter_step, .sections = kmeter_sections, .series = kmeter_series, .ends_words = 1, .ends_fill = kmeter_ends_fill };

extern "C" {

int mtr_engine_kmeter_reset (mtr_engine* e)
{
	if (!e || !(e->cfg.meters & MTR_METER_KMETER)) return fail (MTR_ERR_ARG, "no KMETER in this engine");
	e->snap_valid = false;
	HIPCHK (hipSetDevice (e->cfg.device));
	const size_t n = (size_t) e->cfg.n_streams * 2;
	if (e->km.state.reserve (n)) return fail (MTR_ERR_NOMEM, "hipMalloc KMETER state");
	km_setup (e->cfg.sample_rate, 4 * NT, &e->km.k);                     // (a lane of k_kmeter_blocks: four frames, every 4 NT)
	HIPCHK (hipStreamSynchronize (e->last_stream));
	HIPCHK (hipMemset (e->km.state.p, 0, n * sizeof (mtr_kmeter_state)));   // :142-146
	e->pos.km_fpp = 0;                                                   // (the next process () works its fall-back factor out again)
	e->pos.km_fall = 0.f;
	// the reading series: emptied (a stream that a ragged call closes early leaves 0.0f behind its own points), the open block gone, P kept
	if (e->km.open.n) HIPCHK (hipMemset (e->km.open.p, 0, e->km.open.n));
	if (e->km.s_rms.n) HIPCHK (hipMemset (e->km.s_rms.p, 0, e->km.s_rms.n * sizeof (float)));
	if (e->km.s_peak.n) HIPCHK (hipMemset (e->km.s_peak.p, 0, e->km.s_peak.n * sizeof (float)));
	e->pos.km = {};
	e->km.points.assign (e->cfg.n_streams, 0);
	return MTR_OK;
}

static int no_kmeter (const mtr_engine* e) { return !e || !(e->cfg.meters & MTR_METER_KMETER); }
static const char* const NO_KMETER = "no KMETER in this engine";

int mtr_engine_kmeter_set_period (mtr_engine* e, uint32_t period_frames, uint32_t capacity_points)
{
	if (no_kmeter (e)) return fail (MTR_ERR_ARG, NO_KMETER);
	int rc = series_configure_check (e, "mtr_engine_kmeter_set_period", period_frames, kmeter_min_period (e), "(uint32_t) sample_rate / 20");
	if (rc || (rc = wait_stream (e))) return rc;
	const size_t n = (size_t) e->cfg.n_streams * capacity_points * e->cfg.n_channels;
	if ((rc = series_ring (e->km.s_rms, n, "hipMalloc KMETER series")) || (rc = series_ring (e->km.s_peak, n, "hipMalloc KMETER series"))) return rc;
	if (period_frames && e->km.open.reserve ((size_t) e->cfg.n_streams * sizeof (mtr_kmeter_open))) return fail (MTR_ERR_NOMEM, "hipMalloc KMETER open blocks");
	e->km.ser = { period_frames, capacity_points };
	return mtr_engine_kmeter_reset (e);
}

int mtr_engine_kmeter_period (const mtr_engine* e, uint32_t* period_frames, uint32_t* capacity_points)
{
	if (no_kmeter (e)) return fail (MTR_ERR_ARG, NO_KMETER);
	if (period_frames) *period_frames = e->km.ser.period;
	if (capacity_points) *capacity_points = e->km.ser.cap;
	return MTR_OK;
}

int mtr_engine_kmeter_series (mtr_engine* e, uint32_t first, uint32_t count, float* rms, float* peak, uint32_t capacity, uint32_t* n_points, uint32_t* dropped)
{
	int rc = meter_range (e, !no_kmeter (e), NO_KMETER, first, count);
	if (rc) return rc;
	const size_t take = series_counts (e->pos.km.points, e->km.ser.cap, capacity, n_points, dropped);
	if ((!rms && !peak) || !count || !take) return MTR_OK;
	if ((rc = wait_stream (e))) return rc;
	const size_t C = e->cfg.n_channels;
	if (rms && (rc = series_fetch (rms, e->km.s_rms.p, C, first, e->km.ser.cap, capacity, take, count))) return rc;
	if (peak && (rc = series_fetch (peak, e->km.s_peak.p, C, first, e->km.ser.cap, capacity, take, count))) return rc;
	return MTR_OK;
}

int mtr_engine_kmeter_read (mtr_engine* e, uint32_t first, uint32_t count, float* rms, float* peak)
{
	int rc = meter_range (e, e && rms && peak && (e->cfg.meters & MTR_METER_KMETER), "no KMETER in this engine", first, count);
	if (rc || (rc = wait_stream (e))) return rc;
	std::vector<mtr_kmeter_state> h ((size_t) count * 2);
	HIPCHK (hipMemcpy (h.data (), e->km.state.p + (size_t) first * 2, h.size () * sizeof (mtr_kmeter_state), hipMemcpyDeviceToHost));
	for (size_t i = 0; i < h.size (); ++i) { rms[i] = h[i].rms; peak[i] = h[i].peak; h[i].flag = 1; }
	if (e->km.ser.period) return MTR_OK;                               // (the last completed block's: a read follows every block, nothing to arm)
	HIPCHK (hipMemcpy (e->km.state.p + (size_t) first * 2, h.data (), h.size () * sizeof (mtr_kmeter_state), hipMemcpyHostToDevice));
	return MTR_OK;
}

} // extern "C"
