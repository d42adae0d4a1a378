// mtr_kwmc_body.h — the body of k_kwmc, included by mtr_kwmc.hip once per kernel: KWMC_KERNEL_HEAD is the kernel's template head and
// signature, KWMC_LOCALS what it declares in front of the body (FC, and C where it is no template parameter).  Text, not a function:
// the instantiations of k_kwmc itself compile to the code they always were.
KWMC_KERNEL_HEAD
{
	KWMC_LOCALS
	static_assert (C >= 1 && C <= MTR_MAX_CHANNELS, "1 .. 5 channels (an odd count pads its last pair with a silent channel)");
	static_assert ((K * C) % 4 == 0, "a lane's run is whole 16-byte words");
	static_assert (FC == C || (FC == 6 && C == 5), "the engine's own frames, or WAVE 5.1 on a 5-channel engine");
	static_assert ((K * FC) % 4 == 0, "a lane's run of wide frames is whole 16-byte words");
	constexpr int NP = (C + 1) / 2;                                  // channel pairs of the K-filter
	__shared__ __attribute__ ((aligned (16))) uint32_t words[TP ? 2 * WN : 4];
	uint32_t* const H = words;
	uint32_t* const L = words + WN;
	const int lane = threadIdx.x;

	const uint32_t unit = blockIdx.x;
	const uint32_t s = unit / a.n_segs;
	const uint32_t q = unit - s * a.n_segs;
	const float* const src = a.audio + (size_t) s * a.stride * FC;
	const uint32_t jt0 = a.seg_tile[q], jt1 = a.seg_tile[q + 1];
	const int64_t seg_start = a.tile_start[jt0];
	const int nwarm = (EBU && q > 0) ? (int) a.warm_tiles : 0;
	const int ntile = (int) (jt1 - jt0);
	// the stream's end in this call (N_END: an expression, so that the dense instantiation reads a.n_frames where it always did)
	const int64_t n_end_ = kwmc_end<LEN> (a, s);
#define N_END (LEN ? n_end_ : (int64_t) a.n_frames)
	if (LEN && seg_start >= N_END) return;                             // (wholly past the stream's end: no loads, no products, no writes)
	const int64_t id_end = N_END - 24;                                 // phase 0 of this call ends with frame n_frames - 25

	auto tile_of = [&] (int jj, int64_t& t0, int& len) {
		if (jj < 0) { t0 = seg_start + (int64_t) jj * LT; len = LT; }
		else        { t0 = a.tile_start[jt0 + jj]; len = (int) (a.tile_start[jt0 + jj + 1] - (uint32_t) t0); }
	};

	float* const kz = a.kz + (size_t) s * C * 4;                     // [C][4]: z1 z2 z3 z4 per channel
	v2f k1[NP], k2[NP], k3[NP], k4[NP];                              // carried K-filter state per pair, wave-uniform
#pragma unroll
	for (int p = 0; p < NP; ++p) {
		k1[p] = 0; k2[p] = 0; k3[p] = 0; k4[p] = 0;
		if (EBU && q == 0) {
			const int c0 = 2 * p, c1 = 2 * p + 1;
			k1[p].x = kz[4 * c0 + 0]; k2[p].x = kz[4 * c0 + 1]; k3[p].x = kz[4 * c0 + 2]; k4[p].x = kz[4 * c0 + 3];
			if (c1 < C) { k1[p].y = kz[4 * c1 + 0]; k2[p].y = kz[4 * c1 + 1]; k3[p].y = kz[4 * c1 + 2]; k4[p].y = kz[4 * c1 + 3]; }
		}
	}
	typedef const __attribute__ ((address_space (4))) float* cfloat_p;
	const cfloat_p CM = (cfloat_p) a.scan_m;
	const cfloat_p F = CM + 96;
	float pk[C];                                                     // the segment's peaks so far, per lane and channel
#pragma unroll
	for (int c = 0; c < C; ++c) pk[c] = 0.f;
	const int col8 = 8 * (lane & 15), kg4 = 4 * (lane >> 4);
	const int fo = 2 * col8 + kg4;                                   // + r: output frame of register r inside its block

	for (int jj = -nwarm; jj < ntile; ++jj) {
		int64_t t0; int len;
		tile_of (jj, t0, len);
		if (LEN && t0 >= N_END) break;                                 // (the stream has ended: nothing of it is left in this segment)
		const int64_t f0 = t0 + (int64_t) K * lane;                   // this lane's first frame
		const int rl = min (max (len - K * lane, 0), K);              // frames of the run inside the tile

		// 1. the run: K C floats from frame f0
		float xr[K * C];
		{
			const float* const p = src + f0 * FC;
			if constexpr (FC == C) {
				if (((reinterpret_cast<uintptr_t> (p) & 15) == 0) && f0 + K <= N_END) {
#pragma unroll
					for (int i = 0; i < K * C / 4; ++i) {
						const float4 v = reinterpret_cast<const float4*> (p)[i];
						xr[4 * i] = v.x; xr[4 * i + 1] = v.y; xr[4 * i + 2] = v.z; xr[4 * i + 3] = v.w;
					}
				} else {
#pragma unroll
					for (int i = 0; i < K * C; ++i) xr[i] = f0 + i / C < N_END ? p[i] : 0.f;
				}
			} else {
				// wide sample w = 4 i + j of the run is channel w % FC of frame w / FC: kept at xr [frame * C + c] unless it is the LFE
				auto keep = [&] (int w, float v) {
					const int ch = w % FC;
					if (ch != 3) xr[(w / FC) * C + (ch < 3 ? ch : ch - 1)] = v;
				};
				if (((reinterpret_cast<uintptr_t> (p) & 15) == 0) && f0 + K <= N_END) {
#pragma unroll
					for (int i = 0; i < K * FC / 4; ++i) {
						const float4 v = reinterpret_cast<const float4*> (p)[i];
						keep (4 * i, v.x); keep (4 * i + 1, v.y); keep (4 * i + 2, v.z); keep (4 * i + 3, v.w);
					}
				} else {
#pragma unroll
					for (int i = 0; i < K * C; ++i) xr[i] = f0 + i / C < N_END ? p[(i / C) * FC + wide_ch<C, FC> (i % C)] : 0.f;
				}
			}
#pragma unroll
			for (int i = 0; i < K * C; ++i) if (i / C >= rl) xr[i] = 0.f;   // the next tile's frames (or none)
		}

		if (EBU) {
			mtrw::RowMats rm;
			rm.load (a.scan_m + 96 + 4 * K + 4, lane);
			const v2f e1 = F[4 * K + 0], e2 = F[4 * K + 1], e3 = F[4 * K + 2], e4 = F[4 * K + 3];
			const int last_l = (len - 1) / K, rl_last = len - last_l * K;
			const uint64_t upto = __ballot (lane <= last_l), before = __ballot (lane < last_l);
			const v2f A0 = v2f{a.a0, a.a0}, A1 = v2f{a.a1, a.a1}, A2 = v2f{a.a2, a.a2}, B1 = v2f{a.b1, a.b1}, B2 = v2f{a.b2, a.b2};
			const v2f C3 = v2f{a.c3, a.c3}, C4 = v2f{a.c4, a.c4}, eps2 = v2f{1e-15f, 1e-15f};
			float pw_lane = 0.f;
#pragma unroll
			for (int p = 0; p < NP; ++p) {
				const int c0 = 2 * p, c1 = 2 * p + 1;
				v2f x[K];
#pragma unroll
				for (int n = 0; n < K; ++n) x[n] = v2f{xr[n * C + c0], c1 < C ? xr[n * C + c1] : 0.f};
				// pass 1: end state of the run from a zero start state
				v2f z1 = e1, z2 = e2, z3 = e3, z4 = e4;
#pragma unroll
				for (int n = 0; n < K; ++n) {
					z1 += F[4 * n + 0] * x[n]; z2 += F[4 * n + 1] * x[n]; z3 += F[4 * n + 2] * x[n]; z4 += F[4 * n + 3] * x[n];
				}
				if (rl != K) { z1 = 0; z2 = 0; z3 = 0; z4 = 0; }
				if (lane == 0) {
					const cfloat_p M = CM;
					z1 += M[0] * k1[p] + M[1] * k2[p];
					z2 += M[4] * k1[p] + M[5] * k2[p];
					z3 += M[8] * k1[p] + M[9] * k2[p] + M[10] * k3[p] + M[11] * k4[p];
					z4 += M[12] * k1[p] + M[13] * k2[p] + M[14] * k3[p] + M[15] * k4[p];
				}
				mtrw::scan (z1, z2, z3, z4, CM, rm);
				if (jj < 0) {                                            // warm-up tile: only the state matters
					k1[p] = mtrw::pick (z1, 63); k2[p] = mtrw::pick (z2, 63); k3[p] = mtrw::pick (z3, 63); k4[p] = mtrw::pick (z4, 63);
				} else {
					// pass 2 from the true start state, in kw_pair's hand-scheduled pairs (K is even: no single step)
					z1 = mtrw::from_left (z1); z2 = mtrw::from_left (z2); z3 = mtrw::from_left (z3); z4 = mtrw::from_left (z4);
					if (lane == 0) { z1 = k1[p]; z2 = k2[p]; z3 = k3[p]; z4 = k4[p]; }
					v2f sj = 0;
					[&]<int... P> (std::integer_sequence<int, P...>) {
						(kw_pair<2 * P> (x[2 * P], x[2 * P + 1], z1, z2, z3, z4, sj, A0, A1, A2, B1, B2, C3, C4, eps2, upto, before, rl_last), ...);
					} (std::make_integer_sequence<int, K / 2> {});
					if (rl_last & 1) {
						const v2f w1 = mtrw::pick (z1, last_l), w2 = mtrw::pick (z2, last_l);
						if (lane == last_l) { z1 = w2; z2 = w1; }
					}
					// _chan_gain[c] * sj (ebu_r128_proc.cc:329-330), mono: 2 * sj
					pw_lane += a.gain[c0] * sj.x;
					if (c1 < C) pw_lane += a.gain[c1] * sj.y;
					k1[p] = mtrw::pick (z1, last_l); k2[p] = mtrw::pick (z2, last_l); k3[p] = mtrw::pick (z3, last_l); k4[p] = mtrw::pick (z4, last_l);
				}
				// ebu_r128_proc.cc:331-334: non-finite states are dropped at block ends, per channel
				k1[p] = v2f{scrub1 (k1[p].x), scrub1 (k1[p].y)}; k2[p] = v2f{scrub1 (k2[p].x), scrub1 (k2[p].y)};
				k3[p] = v2f{scrub1 (k3[p].x), scrub1 (k3[p].y)}; k4[p] = v2f{scrub1 (k4[p].x), scrub1 (k4[p].y)};
			}
			if (jj >= 0) {
				const float pw = mtrw::sum63 (pw_lane);
				if (lane == 0) a.tile_power[(size_t) s * a.n_tiles + jt0 + jj] = pw;
			}
		}

		if (TP && jj >= 0) {
			m16::AFrag A;
			A.load (a.mfma_a, lane);
			const int wrun = HALO / 2 + (K / 2) * lane;                  // first word of this lane's run
			// (LEN: the tile's columns in front of the stream's end)
			const int plen_ = LEN ? (int) min ((int64_t) len, N_END - t0) : 0;
#define PLEN (LEN ? plen_ : len)
			const int nb = (PLEN + 255) >> 8;
#pragma unroll
			for (int c = 0; c < C; ++c) {
				// the halo: positions 2 i, 2 i + 1 <-> frames t0 - 48 + 2 i (+ 1), lanes i < 24; history in front of the call
				float g0 = 0.f, g1 = 0.f;
				if (lane < HALO / 2) {
					const int64_t f = t0 - HALO + 2 * lane;
					auto at = [&] (int64_t ff) -> float {
						if (ff >= 0) return (!LEN || ff < N_END) ? src[ff * FC + wide_ch<C, FC> (c)] : 0.f;
						if (ff >= -MTR_FIR_HALO && q == 0) return a.hist[((size_t) s * MTR_FIR_HALO + (size_t) (ff + MTR_FIR_HALO)) * C + c];
						return 0.f;
					};
					g0 = at (f); g1 = at (f + 1);
				}
				float m = 0.f;
#pragma unroll
				for (int n = 0; n < K; ++n) m = fmaxf (m, fabsf (xr[n * C + c]));
				// phase 0: frames of the tile below id_end, and (first tile of the call) frames -24 .. -1 from the halo
				{
					float i0 = m;
					if (t0 + LT > id_end) {
						i0 = 0.f;
						const int64_t lim = id_end - f0;
#pragma unroll
						for (int n = 0; n < K; ++n) if (n < lim) i0 = fmaxf (i0, fabsf (xr[n * C + c]));
					}
					if (q == 0 && jj == 0 && lane >= HALO / 4 && lane < HALO / 2) {
						const int64_t plim = N_END + 24 - t0;
						if (2 * lane < plim)     i0 = fmaxf (i0, fabsf (g0));
						if (2 * lane + 1 < plim) i0 = fmaxf (i0, fabsf (g1));
					}
					pk[c] = fmaxf (pk[c], i0);
				}
				const float hm = fmaxf (fabsf (g0), fabsf (g1));
				const uint32_t emax = __float_as_uint (mtrw::max63 (fmaxf (m, hm))) >> 23;
				float sc, un;
				pow2_scale (emax, sc, un);
				__syncthreads ();                                        // the previous channel's products have read the words
#pragma unroll
				for (int i = 0; i < K / 2; ++i) {
					uint32_t hi, lo;
					m16::split_pair (xr[2 * i * C + c] * sc, xr[(2 * i + 1) * C + c] * sc, hi, lo);
					H[wrun + i] = hi; L[wrun + i] = lo;
				}
				if (lane < HALO / 2) {
					uint32_t hi, lo;
					m16::split_pair (g0 * sc, g1 * sc, hi, lo);
					H[lane] = hi; L[lane] = lo;
				}
				__syncthreads ();
				float pc = 0.f;
				for (int b = 0; b < nb; ++b) {
					// (columns of the last block past the arrays are clamped: their outputs are masked)
					const int w = min (128 * b + col8, 8 * CMAX) + kg4;
					m16::BFrag B;
					m16::fetch_b (B, H, L, w);
					m16::f4 y[3];
					m16::block (A, B, y);
					const int lim = PLEN - 256 * b - fo;                 // registers r < lim are outputs of this tile
#pragma unroll
					for (int p = 0; p < 3; ++p)
#pragma unroll
						for (int r = 0; r < 4; ++r) pc = fmaxf (pc, r < lim ? fabsf (y[p][r]) : 0.f);
				}
				pk[c] = fmaxf (pk[c], pc * un);                          // back to the samples' own scale (exact)
			}
#undef PLEN
		}
	}
#undef N_END
	if (EBU && q == a.n_segs - 1 && lane == 0) {
#pragma unroll
		for (int p = 0; p < NP; ++p) {
			const int c0 = 2 * p, c1 = 2 * p + 1;
			kz[4 * c0 + 0] = k1[p].x; kz[4 * c0 + 1] = k2[p].x; kz[4 * c0 + 2] = k3[p].x; kz[4 * c0 + 3] = k4[p].x;
			if (c1 < C) { kz[4 * c1 + 0] = k1[p].y; kz[4 * c1 + 1] = k2[p].y; kz[4 * c1 + 2] = k3[p].y; kz[4 * c1 + 3] = k4[p].y; }
		}
	}
	if (TP) {
#pragma unroll
		for (int c = 0; c < C; ++c) {
			const float v = mtrw::max63 (pk[c]);
			if (lane == 0) atomicMax (&a.tp_call[(size_t) s * C + c], __float_as_uint (v));
		}
	}
}
