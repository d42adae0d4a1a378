// mtr_stcorr.hip — Stcorrdsp (the COR plugin's, the goniometer's and the surround plugins' stereo phase correlation) for a
// batch (gfx950).
//
// Replaces Stcorrdsp::process (jmeters/stcorrdsp.cc:47-76): per frame
//     zl += w1 (l - zl) + 1e-20f, zr alike;  zlr += w2 (zl zr - zlr), zll and zrr alike;
// at the END of a process () each of the five states that is not finite becomes 0 and zlr, zll, zrr get + 1e-10f; read ()
// (:79-82) is zlr / sqrt (zll zrr + 1e-10f).  One process () is the engine call, or — with a period P, for the reading
// series — every block of exactly P frames, wherever the calls cut the audio.
//
// The second stage is linear in the products p = zl zr, zl^2, zr^2:
//     z_end = q^N z_0 + w2 sum_n q^(N - 1 - n) p [n],  q = 1 - w2,
// so a call is cut into PIECES that never span a period boundary (and are at most `chunk` frames, so that one long period
// still fills the chip); one workgroup reduces one (stream, piece) to the three sums carried to the piece's end, and one
// thread per stream walks the pieces in order — z = q^len z + sum — and does the flush, the + 1e-10f, the reading and the
// series append at every period end (stcorr_walk in mtr_stcorr_scan.h, which SURROUND's pairs take too).  Plain and
// deterministic: no atomics.
//
// The products are not pointwise in the input: zl is a one-pole over the samples.  A workgroup takes its piece tile by tile
// (4096 frames, staged in LDS by coalesced 16-byte loads); lane t walks the 16 contiguous frames t of the tile twice: once
// from zero for its run's end value, then — after a (decay, value) prefix scan across the wave (DPP) and the four waves
// (LDS) gave it the state its run starts from — again for the products.  The tiles are aligned to the piece's END, so the
// first tile starts in front of the piece: over those frames (at least `warm`: |1 - w1|^warm < 2^-48) the first-stage state
// is rebuilt from the audio, and they weigh nothing.  In front of frame 0 of the call there is no audio: there the input
// is zero and the carried zl, zr enter at "frame -1", exactly.  Everything is summed in double: the result is the recurrence
// in exact arithmetic on the f32 samples and coefficients, rounded to f32 where the reference holds an f32 between two
// process () calls (tests/test_gpu_stcorr.py holds it to the reference's own distance from exact arithmetic).
//
// Not finite: a NaN or Inf sample sticks in its channel's zl until the end of the process (), where the reference sets it to
// 0.  Here a piece's sums are then not finite, the walk keeps them so to the period's end, and the channel's zl is 0 from
// there on, as the reference's.  The piece that FOLLOWS a period end inside the call cannot know that when it runs: it starts
// from the state rebuilt over the frames in front of it (samples and a carried state that are not finite taken as 0: such a one
// means the period before is flushed) and reports, beside its sums, what they owe to that start state — with rho = (1 - w1)^(frames
// since the period end), zl [n] = zl0 [n] + rho s, so the sums are quadratic in s with the coefficients sum c rho zl, sum c rho zr
// and sum c rho^2 — and the walk, which knows whether the period before was flushed, moves the sums to the start state 0.
// (A finite sample so large that the reference's f32 zll overflows inside a process () — |x| beyond 1e19 — flushes that period
// there; here the double sum may decay back into f32's range before the period ends and a finite reading comes out.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "mtr_engine_impl.h"
#include "mtr_stcorr_scan.h"

/* Stcorrdsp per-stream state (jmeters/stcorrdsp.h: _zl _zr _zlr _zll _zrr), the last reading, and — for the state blob, whose header has
 * no room for them — the engine's period and the frames into the open period (the host's copies rule; export writes them in) */
typedef struct mtr_stcorr_state {
	float    z[5];                /* zl zr zlr zll zrr */
	float    corr;                /* Stcorrdsp::read () at the end of the most recent process (): the call (period 0) or the last completed period */
	uint32_t period, fill;
} mtr_stcorr_state;

typedef struct mtr_stcorr_args {
	const float*    audio;        /* [S][stride][2] */
	uint64_t        stride, n_frames;
	uint64_t        period;       /* frames per process () of the reading series; 0: the call is one process () */
	uint64_t        e0;           /* call frame at which the period open on entry ends (period 0: n_frames) */
	uint32_t        n_streams, n_pieces;
	uint32_t        chunk;        /* a period is cut into pieces of at most this many frames */
	uint32_t        warm;         /* frames in front of a piece over which its first-stage state is rebuilt */
	float           w1, w2;
	uint32_t        capacity;     /* points per stream the series holds */
	uint64_t        point0;       /* periods completed before this call: the series index of the first one that ends in it */
	mtr_stcorr_state* state;      /* [S] */
	double*         piece;        /* [S][n_pieces][MTR_STCORR_PIECE] (mtr_stcorr_scan.h) */
	float*          series;       /* [S][capacity], NULL if capacity == 0 */
	const uint32_t* ends;         /* [S] per-stream ends of a ragged call (the LEN instantiations), NULL on a dense one */
} mtr_stcorr_args;

namespace {

constexpr int NT = 256;                  // threads per workgroup
constexpr int K = 16;                    // frames per lane run
constexpr int TILE = NT * K;             // frames per tile
constexpr int SLOT = K + 1;              // LDS frames per run: lane stride 34 dwords, ds_read_b64 without bank conflicts
constexpr int MAX_TILES = 8;             // tiles per piece (chunk + warm)
constexpr int NPAIR = TILE / 2 + 1;      // 16-byte pairs that cover a tile starting on either parity

using namespace mtr_sc;                  // Piece / piece_of, dppd, ipow, ScanPow / scan: shared with mtr_surround.hip

// frame f of a stream, 0 outside [lo, hi)
__device__ __forceinline__ float2 frame_at (const float* src, int64_t f, int64_t lo, int64_t hi, bool al8)
{
	if (f < lo || f >= hi) return float2{0.f, 0.f};
	if (al8) return *reinterpret_cast<const float2*> (src + 2 * f);
	return float2{src[2 * f], src[2 * f + 1]};
}

// LEN: the stream ends at call frame a.ends[s].  Its piece is [b0, min (b1, end)): one that starts at or behind the end is empty — nothing
// of it is loaded, nothing written, the walk skips it — and a truncated one has its tiles aligned to the stream's end, so that what it
// reports (sums, zl, zr) stands there and nothing at or past the end is read.  end == n_frames: the dense kernel's piece, bit for bit.
template <bool LEN>
__global__ __launch_bounds__ (NT) void k_stcorr_pieces (const mtr_stcorr_args a)
{
	const uint32_t s = blockIdx.y;
	const Piece pc = piece_of (a, blockIdx.x);
	const float* const src = a.audio + (size_t) s * a.stride * 2;
	int64_t pb1 = pc.b1;
	if constexpr (LEN) {
		const int64_t end = (int64_t) a.ends[s];
		if (pc.b0 >= end) return;                                  // (uniform in the workgroup; end 0: every piece of the stream)
		if (end < pb1) pb1 = end;
	}
	const int64_t b0 = pc.b0, b1 = pb1;
	const int64_t warm = b0 == 0 ? 1 : (int64_t) a.warm;          // (the call's first piece: only the slot of frame -1)
	const int nt = (int) ((b1 - b0 + warm + TILE - 1) / TILE);      // <= MAX_TILES: chunk + warm = MAX_TILES * TILE
	const int64_t lo = b0 - warm > 0 ? b0 - warm : 0;              // the first frame that is read
	const int64_t T0 = b1 - (int64_t) nt * TILE;                    // < b0
	const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
	// 16-byte loads: pairs of frames from an even frame of the BUFFER
	const bool al8 = (reinterpret_cast<size_t> (a.audio) & 7) == 0;
	const int64_t base = (int64_t) ((size_t) s * a.stride + (reinterpret_cast<size_t> (a.audio) >> 3));

	const double w1 = (double) a.w1, r = 1.0 - w1, q1 = 1.0 - (double) a.w2, bias = (double) 1e-20f;
	double zc[2] = { (double) a.state[s].z[0], (double) a.state[s].z[1] };         // the carried zl, zr: "frame -1"
	if (pc.after_period) {                                         // (not finite: the period before is flushed, its zl with it)
		if (!isfinite (zc[0])) zc[0] = 0.0;
		if (!isfinite (zc[1])) zc[1] = 0.0;
	}
	ScanPow sp;
	const double r2 = r * r, r4 = r2 * r2, r8 = r4 * r4;
	sp.d1 = r8 * r8; sp.d2 = sp.d1 * sp.d1; sp.d4 = sp.d2 * sp.d2; sp.d8 = sp.d4 * sp.d4;   // (K = 16: d > 0 also where r < 0)
	sp.dp = ipow (sp.d1, (lane & 15) + 1);
	sp.dq = lane >= 32 ? ipow (sp.d1, lane - 31) : 0.0;
	const double dl = ipow (sp.d1, lane);                          // from the wave's first frame to this lane's run
	const double d64 = sp.d8 * sp.d8 * sp.d8 * sp.d8 * sp.d8 * sp.d8 * sp.d8 * sp.d8;   // ... and over a whole wave
	// weight of a run's sums at the piece's end: w2 q^(frames behind the run); from tile to tile it grows by q^-TILE
	double W = (double) a.w2 * pow (q1, (double) ((int64_t) nt * TILE - (int64_t) K * (tid + 1)));
	const double g = pow (q1, (double) -TILE);

	__shared__ float2 lds[NT * SLOT];
	__shared__ double sh_tot[NT / 64][2];
	__shared__ double sh_red[NT / 64][5];
	double zt[2] = { 0.0, 0.0 };                                   // zl, zr in front of the tile (the first one starts from nothing)
	double tot[5] = { 0.0, 0.0, 0.0, 0.0, 0.0 };                   // lr ll rr, and (after a period end) sum c rho zl, sum c rho zr
	double* const out = a.piece + ((size_t) s * a.n_pieces + blockIdx.x) * MTR_STCORR_PIECE;

	float4 pre[(NPAIR + NT - 1) / NT];
	auto fetch = [&] (int64_t T) {
		const int64_t P0 = T - ((base + T) & 1);
#pragma unroll
		for (int j = 0; j < (NPAIR + NT - 1) / NT; ++j) {
			const int i = tid + j * NT;
			const int64_t f = P0 + 2 * (int64_t) i;
			float4 v = float4{0.f, 0.f, 0.f, 0.f};
			if (i < NPAIR) {
				if (al8 && f >= lo && f + 1 < b1) v = *reinterpret_cast<const float4*> (src + 2 * f);
				else {
					const float2 x = frame_at (src, f, lo, b1, al8), y = frame_at (src, f + 1, lo, b1, al8);
					v = float4{x.x, x.y, y.x, y.y};
				}
			}
			pre[j] = v;
		}
	};
	auto stash = [&] (int64_t T) {
		const int64_t P0 = T - ((base + T) & 1);
#pragma unroll
		for (int j = 0; j < (NPAIR + NT - 1) / NT; ++j) {
			const int i = tid + j * NT;
			const int o = (int) (P0 - T) + 2 * i;                  // tile index of the pair's first frame: -1 .. TILE
			if (i < NPAIR) {
				if (o >= 0 && o < TILE) lds[(o >> 4) * SLOT + (o & 15)] = float2{pre[j].x, pre[j].y};
				if (o + 1 < TILE) lds[((o + 1) >> 4) * SLOT + ((o + 1) & 15)] = float2{pre[j].z, pre[j].w};
			}
		}
	};

	fetch (T0);
	for (int t = 0; t < nt; ++t) {
		const int64_t T = T0 + (int64_t) t * TILE;
		stash (T);
		__syncthreads ();
		if (t + 1 < nt) fetch (T + TILE);                          // (in flight under this tile's arithmetic)
		const bool head = T < b0;                                  // frames in front of the piece: they rebuild zl, zr and weigh nothing
		const int64_t f0 = T + (int64_t) K * tid;
		// ---- pass 1: the inputs of the one-pole, and the run's end value from zero ----
		double ul[K], ur[K];
		double vl = 0.0, vr = 0.0;
#pragma unroll
		for (int k = 0; k < K; ++k) {
			float2 x = lds[tid * SLOT + k];
			if (!head) {
				ul[k] = fma (w1, (double) x.x, bias); ur[k] = fma (w1, (double) x.y, bias);
			} else {
				const int64_t f = f0 + k;
				if (pc.after_period && f < b0) {                   // (see the head of the file)
					if (!isfinite (x.x)) x.x = 0.f;
					if (!isfinite (x.y)) x.y = 0.f;
				}
				ul[k] = f >= 0 ? fma (w1, (double) x.x, bias) : f == -1 ? zc[0] : 0.0;
				ur[k] = f >= 0 ? fma (w1, (double) x.y, bias) : f == -1 ? zc[1] : 0.0;
			}
			vl = fma (r, vl, ul[k]); vr = fma (r, vr, ur[k]);
		}
		// ---- the state each run starts from: scan across the wave, then across the waves ----
		vl = scan (vl, sp); vr = scan (vr, sp);
		if (lane == 63) { sh_tot[wid][0] = vl; sh_tot[wid][1] = vr; }
		__syncthreads ();                                          // (and every lane has read its run: the next stash may overwrite the tile)
		double cin[2] = { 0.0, 0.0 };
#pragma unroll
		for (int w = 0; w < NT / 64; ++w) {
			if (w == wid) { cin[0] = zt[0]; cin[1] = zt[1]; }
			zt[0] = fma (d64, zt[0], sh_tot[w][0]); zt[1] = fma (d64, zt[1], sh_tot[w][1]);
		}
		double zl = fma (dl, cin[0], dppd<0x138, 0xF> (vl));       // (wave_shr:1: the scan of the lane to the left, lane 0 reads 0)
		double zr = fma (dl, cin[1], dppd<0x138, 0xF> (vr));
		// ---- pass 2: the products, carried to the run's end ----
		// (behind a period end, while rho is above the sums' resolution: also what the sums owe to the state the piece started from)
		const bool owes = pc.after_period && T < b0 + warm;            // uniform
		double alr = 0.0, all = 0.0, arr = 0.0, abl = 0.0, abr = 0.0;
		double rho = owes && f0 > b0 ? ipow (r, (uint64_t) (f0 - b0)) : 1.0;
#pragma unroll
		for (int k = 0; k < K; ++k) {
			zl = fma (r, zl, ul[k]); zr = fma (r, zr, ur[k]);
			double plr = zl * zr, pll = zl * zl, prr = zr * zr;
			if (head && f0 + k < b0) { plr = 0.0; pll = 0.0; prr = 0.0; }
			alr = fma (alr, q1, plr); all = fma (all, q1, pll); arr = fma (arr, q1, prr);
			if (owes) {
				const int64_t f = f0 + k;
				if (f == b0 - 1) { out[7] = zl; out[8] = zr; }         // the start state itself (one lane of the workgroup)
				const bool in = f >= b0;
				if (in) rho *= r;
				abl = fma (abl, q1, in ? rho * zl : 0.0); abr = fma (abr, q1, in ? rho * zr : 0.0);
			}
		}
		tot[0] = fma (W, alr, tot[0]); tot[1] = fma (W, all, tot[1]); tot[2] = fma (W, arr, tot[2]);
		if (owes) { tot[3] = fma (W, abl, tot[3]); tot[4] = fma (W, abr, tot[4]); }
		W *= g;
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
		for (int j = 0; j < 5; ++j) tot[j] += __shfl_xor (tot[j], d, 64);
	if (lane == 0) for (int j = 0; j < 5; ++j) sh_red[wid][j] = tot[j];
	__syncthreads ();
	if (tid == 0) {
		for (int j = 0; j < 5; ++j) {
			double e = 0.0;
			for (int w = 0; w < NT / 64; ++w) e += sh_red[w][j];
			out[j < 3 ? j : j + 2] = e;
		}
		out[3] = zt[0]; out[4] = zt[1];
	}
}

// one thread per stream: stcorr_walk (mtr_stcorr_scan.h) over the stream's pieces.  LEN, end == 0: the stream is not touched.
template <bool LEN>
__global__ void k_stcorr_final (const mtr_stcorr_args a)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= a.n_streams) return;
	int64_t end = 0;
	if constexpr (LEN) {
		end = (int64_t) a.ends[s];
		if (end == 0) return;
	}
	mtr_stcorr_state* const st = a.state + s;
	const StcorrWalk v = { st->z, &st->corr, a.piece + (size_t) s * a.n_pieces * MTR_STCORR_PIECE, MTR_STCORR_PIECE,
	                       a.capacity ? a.series + (size_t) s * a.capacity : nullptr, 1 };
	stcorr_walk<LEN> (a, v, end);
}

}  // namespace

static void mtr_stcorr_geometry (float w1, uint32_t* warm, uint32_t* chunk)
{
	// |1 - w1|^J < 2^-48: what the rebuilt state lacks is below the resolution of the double sums, not only of an f32.
	// (|1 - w1| < 1 from 8 kHz up — w1 = 1.57 there; a rate so high that J would take half the tiles gets half the tiles.)
	const double ar = fabs (1.0 - (double) w1);
	double J = ar > 0.0 && ar < 1.0 ? ceil (-48.0 * log (2.0) / log (ar)) : 1.0;
	const double most = (double) (MAX_TILES / 2 * TILE);
	if (!(J >= 1.0)) J = 1.0;
	if (J > most) J = most;
	*warm = ((uint32_t) J + K) / K * K;                            // (+ the slot of frame -1)
	*chunk = MAX_TILES * TILE - *warm;
}

static int mtr_launch_stcorr (const mtr_stcorr_args& a, void* stream)
{
	hipStream_t st = (hipStream_t) stream;
	const auto launch = [&] (auto LEN) {                              // (per-stream ends or none: the kernels' template argument)
		hipLaunchKernelGGL (k_stcorr_pieces<LEN.value>, dim3 (a.n_pieces, a.n_streams), dim3 (NT), 0, st, a);
		hipLaunchKernelGGL (k_stcorr_final<LEN.value>, dim3 ((a.n_streams + 63) / 64), dim3 (64), 0, st, a);
	};
	if (a.ends) launch (std::true_type {}); else launch (std::false_type {});
	return hipGetLastError () == hipSuccess ? 0 : -1;
}

// ---- STCORR in the engine: set-up, the call's step, the blob's section and the cursors in it, the C entry points -----------------------

static uint32_t stcorr_min_period (const mtr_engine* e) { return (uint32_t) e->cfg.sample_rate / 20; }

static int stcorr_create (mtr_engine* e)
{
	mtr_setup_stcorr (e->cfg.sample_rate, e->sc.w);
	mtr_stcorr_geometry (e->sc.w[0], &e->sc.warm, &e->sc.chunk);
	return MTR_OK;
}

// The periods of the reading series are cut from where the CALL started (e->pos): every chunk of a host call sees the same cuts
static int stcorr_step (mtr_engine* e, const Call& c, Cursors& nx, const StreamEnds& se)
{
	const size_t vo = c.off;
	const uint64_t P = e->sc.ser.period;
	const uint32_t cap = e->sc.ser.cap;
	mtr_stcorr_args sa;
	sa.audio = c.audio; sa.stride = c.stride; sa.n_frames = c.n_frames;
	sa.period = P; sa.e0 = series_e0 (e->pos.sc, P, c.n_frames);
	sa.n_streams = c.cnt; sa.chunk = e->sc.chunk; sa.warm = e->sc.warm;
	sa.n_pieces = mtr_sc::n_pieces (c.n_frames, sa.e0, P, sa.chunk);
	sa.w1 = e->sc.w[0]; sa.w2 = e->sc.w[1];
	sa.capacity = cap; sa.point0 = e->pos.sc.points;
	if (e->sc.piece.reserve ((size_t) e->cfg.n_streams * sa.n_pieces * MTR_STCORR_PIECE)) return fail (MTR_ERR_NOMEM, "hipMalloc STCORR pieces");
	sa.state = e->sc.state.p + vo; sa.piece = e->sc.piece.p + vo * sa.n_pieces * MTR_STCORR_PIECE;
	sa.series = cap ? e->sc.series.p + vo * cap : nullptr;
	sa.ends = se.ends;
	if (mtr_launch_stcorr (sa, c.st)) return fail (MTR_ERR_HIP, "k_stcorr launch");
	nx.sc = series_advance (e->pos.sc, P, c.n_frames);
	return MTR_OK;
}

static void stcorr_sections (const mtr_engine* e, std::vector<StateSection>& v)
{
	v.push_back ({ e->sc.state.p, sizeof (mtr_stcorr_state) });
}

// The blob header: the period and the frames into the open one, the last two fields of every stream's entry
struct StcorrHdr { uint32_t period, fill; };
static_assert (offsetof (mtr_stcorr_state, fill) == offsetof (mtr_stcorr_state, period) + 4 && sizeof (mtr_stcorr_state) == offsetof (mtr_stcorr_state, period) + sizeof (StcorrHdr), "StcorrHdr");
constexpr const char* STCORR_CORRUPT = "mtr_engine_state_import: corrupt blob (period of the STCORR series)";

static void stcorr_hdr_write (const mtr_engine* e, void* out) { *static_cast<StcorrHdr*> (out) = { e->sc.ser.period, (uint32_t) e->pos.sc.fill }; }

static int stcorr_hdr_check (const mtr_engine* e, const void* in, bool fresh)
{
	const StcorrHdr& h = *static_cast<const StcorrHdr*> (in);
	if (!series_blob_ok (h.period, h.fill, stcorr_min_period (e), 0xFFFFFFFFu)) return fail (MTR_ERR_STATE, STCORR_CORRUPT);
	if (!fresh && (h.period != e->sc.ser.period || h.fill != e->pos.sc.fill))
		return fail (MTR_ERR_STATE, "mtr_engine_state_import: the engine does not stand where the blob's streams do (period of the STCORR series)");
	return MTR_OK;
}

static void stcorr_hdr_take (mtr_engine* e, const void* in)
{
	const StcorrHdr& h = *static_cast<const StcorrHdr*> (in);
	e->sc.ser.period = h.period; e->pos.sc.fill = h.fill;
}

static SeriesView stcorr_series (mtr_engine* e) { return { &e->sc.ser, &Cursors::sc, &e->sc.points }; }

static constinit BlobHeader stcorr_hdr = { .offset = offsetof (mtr_stcorr_state, period), .bytes = sizeof (StcorrHdr), .corrupt = STCORR_CORRUPT,
                                           .write = stcorr_hdr_write, .check = stcorr_hdr_check, .take = stcorr_hdr_take };
constinit SideMeter stcorr_meter = { .bits = MTR_METER_STCORR, .max_frames = 0x7fffffffull, .max_text = "STCORR: n_frames per call must be < 2^31 - 1 (the reference's int n)",
                                     .create = stcorr_create, .reset = mtr_engine_stcorr_reset, .step = stcorr_step, .sections = stcorr_sections, .hdr = &stcorr_hdr, .series = stcorr_series };

extern "C" {

int mtr_stcorr_coef (float sample_rate, float* out2)
{
	if (!out2 || !(sample_rate >= 1.f)) return fail (MTR_ERR_ARG, "mtr_stcorr_coef");
	mtr_setup_stcorr (sample_rate, out2);
	return MTR_OK;
}

static int no_stcorr (const mtr_engine* e) { return !e || !(e->cfg.meters & MTR_METER_STCORR); }

int mtr_engine_stcorr_reset (mtr_engine* e)
{
	if (no_stcorr (e)) return fail (MTR_ERR_ARG, "no STCORR in this engine");
	e->snap_valid = false;
	HIPCHK (hipSetDevice (e->cfg.device));
	const uint32_t S = e->cfg.n_streams;
	if (e->sc.state.reserve (S)) return fail (MTR_ERR_NOMEM, "hipMalloc STCORR state");
	std::vector<mtr_stcorr_state> h (S);
	memset (h.data (), 0, S * sizeof (mtr_stcorr_state));          // stcorrdsp.cc:33-36
	for (auto& v : h) v.period = e->sc.ser.period;
	HIPCHK (hipStreamSynchronize (e->last_stream));
	HIPCHK (hipMemcpy (e->sc.state.p, h.data (), S * sizeof (mtr_stcorr_state), hipMemcpyHostToDevice));
	// (the series: a stream that a ragged call closes early leaves 0.0f behind its own points)
	if (e->sc.series.n) HIPCHK (hipMemset (e->sc.series.p, 0, e->sc.series.n * sizeof (float)));
	e->pos.sc = {};
	e->sc.points.assign (S, 0);
	return MTR_OK;
}

int mtr_engine_stcorr_set_period (mtr_engine* e, uint32_t period_frames, uint32_t capacity_points)
{
	if (no_stcorr (e)) return fail (MTR_ERR_ARG, "no STCORR in this engine");
	int rc = series_configure_check (e, "mtr_engine_stcorr_set_period", period_frames, stcorr_min_period (e), "(uint32_t) sample_rate / 20");
	if (rc || (rc = wait_stream (e))) return rc;
	if ((rc = series_ring (e->sc.series, (size_t) e->cfg.n_streams * capacity_points, "hipMalloc STCORR series"))) return rc;
	e->sc.ser = { period_frames, capacity_points };
	return mtr_engine_stcorr_reset (e);
}

int mtr_engine_stcorr_read (mtr_engine* e, uint32_t first, uint32_t count, float* corr, float* state5)
{
	int rc = meter_range (e, !no_stcorr (e) && corr, "no STCORR in this engine", first, count);
	if (rc || (rc = wait_stream (e))) return rc;
	std::vector<mtr_stcorr_state> h (count);
	if (count) HIPCHK (hipMemcpy (h.data (), e->sc.state.p + first, count * sizeof (mtr_stcorr_state), hipMemcpyDeviceToHost));
	for (uint32_t i = 0; i < count; ++i) {
		corr[i] = h[i].corr;
		if (state5) memcpy (state5 + (size_t) i * 5, h[i].z, sizeof (h[i].z));
	}
	return MTR_OK;
}

int mtr_engine_stcorr_series (mtr_engine* e, uint32_t first, uint32_t count, float* out, uint32_t capacity, uint32_t* n_points, uint32_t* dropped)
{
	int rc = meter_range (e, !no_stcorr (e), "no STCORR in this engine", first, count);
	if (rc) return rc;
	const size_t take = series_counts (e->pos.sc.points, e->sc.ser.cap, capacity, n_points, dropped);
	if (!out || !count || !take) return MTR_OK;
	if ((rc = wait_stream (e))) return rc;
	return series_fetch (out, e->sc.series.p, 1, first, e->sc.ser.cap, capacity, take, count);
}

} // extern "C"
