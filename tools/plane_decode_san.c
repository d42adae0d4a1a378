#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "mtr_internal.h"
/* tools/plane_decode_san.c — mtr_setup_plane_decode (mtr_setup.c: the host definition of a plane layout) under AddressSanitizer + UBSan in a
 * program of its own: `make check-san-plane`.  Every format, P and C 1 .. 8, n_frames 0 .. 9, stride n .. n + 3, against the decoders it is made of. */
/* exact-size heap buffers: any read at or behind n_frames samples of the last plane, or any write behind dst, trips ASan */
int main (void)
{
	int bad = 0;
	for (int format = 0; format <= 3; ++format) {
		const size_t sb = format ? mtr_setup_pcm_sample_bytes (format) : 4;
		for (uint32_t P = 1; P <= 8; ++P) for (uint32_t C = 1; C <= 8; ++C) for (size_t n = 0; n <= 9; ++n) for (size_t extra = 0; extra <= 3; ++extra) {
			const uint64_t stride = n + extra;
			uint8_t map[8];
			for (uint32_t c = 0; c < C; ++c) map[c] = (uint8_t) ((c * 3 + P - 1) % P);
			/* the buffer ends with the n samples of the last plane: nothing behind them exists */
			const size_t bytes = ((size_t) (P - 1) * stride + n) * sb;
			unsigned char* src = malloc (bytes ? bytes : 1);
			for (size_t i = 0; i < bytes; ++i) src[i] = (unsigned char) (i * 37 + 11);
			float* dst = malloc (n && C ? n * C * sizeof (float) : 1);
			if (mtr_setup_plane_decode (format, src, n, stride, P, map, C, dst)) { ++bad; }
			for (size_t i = 0; i < n && !bad; ++i) for (uint32_t c = 0; c < C; ++c) {
				float want;
				const unsigned char* s = src + ((size_t) map[c] * stride + i) * sb;
				if (format) mtr_setup_pcm_decode (format, s, 1, &want); else memcpy (&want, s, 4);
				if (memcmp (&want, dst + i * C + c, 4)) ++bad;
			}
			free (src); free (dst);
		}
	}
	uint8_t m2[2] = { 0, 2 };
	float d[2];
	if (mtr_setup_plane_decode (0, d, 1, 1, 2, m2, 2, d) != -1) ++bad;   /* an entry >= P */
	printf ("bad = %d\n", bad);
	return bad != 0;
}
