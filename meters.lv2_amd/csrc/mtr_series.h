// mtr_series.h — the reading series of STCORR, NEEDLE, SURROUND, KMETER and SPECTR30: blocks of exactly P frames, cut wherever the calls cut the audio, one
// reading per block appended to a ring of `cap` points per stream (P = 0: the call is the block and nothing is appended).  Here is what
// they share of it on the host that needs neither the engine nor the HIP runtime; series_configure_check, series_ring and
// series_fetch, which need both, are in mtr_engine_impl.h.  What a block IS — a process () of Stcorrdsp, of the needle meters' detectors, of
// the surround meter's, a spectrum_run of the bank — and the smallest P it takes stay the meters' own.  Not installed.
#ifndef MTR_SERIES_H
#define MTR_SERIES_H

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

struct SeriesPos { uint64_t fill = 0, points = 0; };   // frames in the open block; blocks completed since reset (what the ring does not hold of them is dropped)
struct SeriesCfg { uint32_t period = 0, cap = 0; };    // P; points per stream the ring holds

// the call frame at which the block open on entry ends
inline uint64_t series_e0 (const SeriesPos& pos, uint64_t P, uint64_t n_frames) { return P ? P - pos.fill : n_frames; }

// where the series stands behind a call of n_frames that started at `pos`
inline SeriesPos series_advance (const SeriesPos& pos, uint64_t P, uint64_t n_frames)
{
	const uint64_t tot = pos.fill + n_frames;
	return { P ? tot % P : 0, pos.points + (P ? tot / P : 0) };
}

// A ragged call (mtr_ragged.h): a stream that takes `frames` of a call of n_frames which started `fill` frames into a block.  *whole:
// blocks of P it completes; *partial: 1 if it ends inside the call and a truncated block follows them — its last process (), of
// (fill + frames) mod P frames — else 0.  P = 0: the call is the block; no whole ones, and the closing call of a stream that got some frames is
// the truncated one (an open stream's call is no series point).  false: fill >= P > 0 or frames > n_frames.
inline bool series_cut (uint64_t fill, uint64_t P, uint64_t n_frames, uint64_t frames, uint64_t* whole, uint32_t* partial)
{
	if ((P && fill >= P) || frames > n_frames) return false;
	const bool closes = frames > 0 && frames < n_frames;
	const uint64_t tot = fill + frames;
	*whole = P ? tot / P : 0;
	*partial = closes && (P == 0 || tot % P) ? 1 : 0;
	return true;
}

// a state blob's copy of (P, fill): P is 0 or min_period .. max_period, and fill is inside the block
inline bool series_blob_ok (uint32_t period, uint32_t fill, uint32_t min_period, uint32_t max_period)
{
	return period ? fill < period && period >= min_period && period <= max_period : fill == 0;
}

// What a getter answers before it copies: points completed and points dropped (saturated to 32 bits); returns the points per stream to copy
inline size_t series_counts (uint64_t points, uint32_t cap, uint32_t capacity, uint32_t* n_points, uint32_t* dropped)
{
	const uint64_t kept = std::min<uint64_t> (points, cap);
	if (n_points) *n_points = (uint32_t) std::min<uint64_t> (points, 0xFFFFFFFFull);
	if (dropped) *dropped = (uint32_t) std::min<uint64_t> (points - kept, 0xFFFFFFFFull);
	return (size_t) std::min<uint64_t> (kept, capacity);
}

// The host-owned header of a side meter's section of a state blob: `bytes` bytes in each of `count` entries, `pitch` bytes from one
// entry's to the next, the first at `hdr`.  The streams of an engine stand in lock step, so every entry carries the same one: false if
// one differs from the first.
inline bool blob_headers_agree (const unsigned char* hdr, size_t pitch, size_t bytes, uint32_t count)
{
	for (uint32_t k = 1; k < count; ++k)
		if (memcmp (hdr + (size_t) k * pitch, hdr, bytes)) return false;
	return true;
}

#endif
