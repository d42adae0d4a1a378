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
// per 31.5 GB.)  The sums are re-associated and carried in double: tests/test_gpu_kmeter.py states 1e-5
// relative against the restatement.
//
// LEN (both kernels): the call carries per-stream ends (a.ends, call-relative: mtr_engine_process_*_tracks, or any call once a stream of
// its view is closed).  Stream s ends at frame E = ends [s], workgroup-uniform (one scalar load): a stream that ends inside the call sees
// ONE process (p, E) — E / 4 groups, the weights A^k counted back from ITS last group, fpp = E with the fall-back factor the host
// computed for that fpp (a.falls [s], the expression of kmeter_fall) — and a stream with E = n_frames exactly what the dense call gives it
// (the cursor's fall).  A workgroup of k_kmeter_pieces whose chunk lies at or past the stream's groups returns before it touches memory
// and writes NO piece slot: k_kmeter_final adds the stream's own chunks only — it never reads those slots.  E = 0 (a closed stream,
// frames [s] == 0): nothing is written, not even the + 1e-20f.  Groups start on multiples of four frames whatever E is: the 16-byte
// path is the dense one's.  The dense instantiations are the kernels as they always were.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "mtr_engine_impl.h"

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

namespace {

constexpr int NT = 256;                  // threads per workgroup
constexpr int CH = 32 * NT;              // groups (of four samples) per workgroup: 32768 frames

struct Mat { double a, c, b; };          // [[a, 0], [c, b]]
__host__ __device__ inline Mat mat_pow (double a1, double c1, double b1, double k)
{
	// A^k for A = [[a1, 0], [c1, b1]]: c_k = c1 (a1^k - b1^k) / (a1 - b1)
	const double ak = pow (a1, k), bk = pow (b1, k);
	return Mat{ak, c1 * (ak - bk) / (a1 - b1), bk};
}

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
#pragma unroll
		for (int c = 0; c < C; ++c) {
			const float s0 = v[c] * v[c], s1 = v[C + c] * v[C + c], s2 = v[2 * C + c] * v[2 * C + c], s3 = v[3 * C + c] * v[3 * C + c];
			t[c] = t[c] < s0 ? s0 : t[c];                          // kmeterdsp.cc:79: if (t < s) t = s (NaN never enters)
			t[c] = t[c] < s1 ? s1 : t[c];
			t[c] = t[c] < s2 ? s2 : t[c];
			t[c] = t[c] < s3 ? s3 : t[c];
			const double g = (double) (u0 * s0) + (double) (u1 * s1) + (double) (u2 * s2) + (double) (u3 * s3);
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
	float z1 = (float) (g.a * (double) zi1 + e1);
	float z2 = (float) (g.c * (double) zi1 + g.b * (double) zi2 + e2);
	if (n_groups == 0) { z1 = zi1; z2 = zi2; }
	if (isnan (z1)) z1 = 0;                                            // :100-102
	if (isnan (z2)) z2 = 0;
	if (!isfinite (t)) t = 0;
	st->z1 = z1 + 1e-20f;
	st->z2 = z2 + 1e-20f;
	const float r = sqrtf (2.0f * z2);
	t = sqrtf (t);
	if (st->flag) { st->rms = r; st->flag = 0; }                       // :112-118
	else if (r > st->rms) st->rms = r;
	if (t >= st->peak) { st->peak = t; st->cnt = a.hold; }             // :121-138
	else if (st->cnt > 0) st->cnt -= (int32_t) fpp;
	else { st->peak *= fall; st->peak += 1e-10f; }
}

}  // namespace

static void mtr_kmeter_powers (float omega, double* pw1 /* [3] */)
{
	const double w = (double) omega;
	const double a1 = pow (1.0 - w, 4.0), b1 = 1.0 - 4.0 * w, c1 = 4.0 * w * a1;
	pw1[0] = a1; pw1[1] = c1; pw1[2] = b1;
}

static uint32_t mtr_kmeter_pieces (uint64_t n_groups) { return (uint32_t) ((n_groups + CH - 1) / CH); }

static int mtr_launch_kmeter (const mtr_kmeter_args& a, void* stream)
{
	hipStream_t st = (hipStream_t) stream;
	const uint32_t n = a.n_streams * a.n_channels;
	if (a.ends) {
		if (a.n_pieces) {
			if (a.n_channels == 2) hipLaunchKernelGGL ((k_kmeter_pieces<2, true>), dim3 (a.n_pieces, a.n_streams), dim3 (NT), 0, st, a);
			else                   hipLaunchKernelGGL ((k_kmeter_pieces<1, true>), dim3 (a.n_pieces, a.n_streams), dim3 (NT), 0, st, a);
		}
		hipLaunchKernelGGL (k_kmeter_final<true>, dim3 ((n + 63) / 64), dim3 (64), 0, st, a);
		return hipGetLastError () == hipSuccess ? 0 : -1;
	}
	if (a.n_pieces) {
		if (a.n_channels == 2) hipLaunchKernelGGL ((k_kmeter_pieces<2, false>), dim3 (a.n_pieces, a.n_streams), dim3 (NT), 0, st, a);
		else                   hipLaunchKernelGGL ((k_kmeter_pieces<1, false>), dim3 (a.n_pieces, a.n_streams), dim3 (NT), 0, st, a);
	}
	hipLaunchKernelGGL (k_kmeter_final<false>, dim3 ((n + 63) / 64), dim3 (64), 0, st, a);
	return hipGetLastError () == hipSuccess ? 0 : -1;
}

// ---- KMETER in the engine: the call's step, the blob's section, reset, the reading ------------------------------------------------------

// kmeterdsp.cc:60-65: the fall-back factor of a process () of n frames (15 dB/s)
float kmeter_fall (const mtr_engine* e, uint64_t n)
{
	return powf (10.0f, -0.05f * 15.0f * ((float) n / e->cfg.sample_rate));
}

static int kmeter_step (mtr_engine* e, const Call& c, Cursors& nx, const StreamEnds& se)
{
	const size_t vo = c.off;
	mtr_kmeter_args ka;
	ka.audio = c.audio; ka.stride = c.stride; ka.n_groups = c.n_frames / 4;
	ka.n_streams = c.cnt; ka.n_channels = e->cfg.n_channels; ka.ends = se.ends; ka.falls = se.km_fall;
	ka.n_pieces = mtr_kmeter_pieces (ka.n_groups);
	if (nx.km_fpp != (uint32_t) c.n_frames) {                          // kmeterdsp.cc:60-65
		nx.km_fall = kmeter_fall (e, c.n_frames);
		nx.km_fpp = (uint32_t) c.n_frames;
	}
	ka.fpp = nx.km_fpp; ka.fall = nx.km_fall;
	ka.hold = (int32_t) (0.5f * e->cfg.sample_rate + 0.5f);             // :51
	ka.omega = 9.72f / e->cfg.sample_rate;
	memcpy (ka.pw1, e->km.pw1, sizeof (ka.pw1));
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

constinit SideMeter kmeter_meter = { MTR_METER_KMETER, 0x7fffffffull, "KMETER: n_frames per call must be < 2^31 - 1 (the reference's int n)",
                                           nullptr, mtr_engine_kmeter_reset, kmeter_step, kmeter_sections, nullptr };

extern "C" {

int mtr_engine_kmeter_reset (mtr_engine* e)
{
	if (!e || !(e->cfg.meters & MTR_METER_KMETER)) return fail (MTR_ERR_ARG, "no KMETER in this engine");
	e->snap_valid = false;
	HIPCHK (hipSetDevice (e->cfg.device));
	const size_t n = (size_t) e->cfg.n_streams * 2;
	if (e->km.state.reserve (n)) return fail (MTR_ERR_NOMEM, "hipMalloc KMETER state");
	mtr_kmeter_powers (9.72f / e->cfg.sample_rate, e->km.pw1);           // kmeterdsp.cc:52
	HIPCHK (hipStreamSynchronize (e->last_stream));
	HIPCHK (hipMemset (e->km.state.p, 0, n * sizeof (mtr_kmeter_state)));   // :142-146
	e->pos.km_fpp = 0;                                                   // (the next process () works its fall-back factor out again)
	e->pos.km_fall = 0.f;
	return MTR_OK;
}

int mtr_engine_kmeter_read (mtr_engine* e, uint32_t first, uint32_t count, float* rms, float* peak)
{
	int rc = meter_range (e, e && rms && peak && (e->cfg.meters & MTR_METER_KMETER), "no KMETER in this engine", first, count);
	if (rc || (rc = wait_stream (e))) return rc;
	std::vector<mtr_kmeter_state> h ((size_t) count * 2);
	HIPCHK (hipMemcpy (h.data (), e->km.state.p + (size_t) first * 2, h.size () * sizeof (mtr_kmeter_state), hipMemcpyDeviceToHost));
	for (size_t i = 0; i < h.size (); ++i) { rms[i] = h[i].rms; peak[i] = h[i].peak; h[i].flag = 1; }
	HIPCHK (hipMemcpy (e->km.state.p + (size_t) first * 2, h.data (), h.size () * sizeof (mtr_kmeter_state), hipMemcpyHostToDevice));
	return MTR_OK;
}

} // extern "C"
